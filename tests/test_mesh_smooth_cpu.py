"""The float64 reference of the smoothing stage (tests/helpers/mesh_smooth_ref.py) on its own: what Taubin smoothing is for (a smoother
sphere that keeps its volume, where plain Laplacian smoothing shrinks it), the orientation of the area-weighted normals, the
invariances that make the arrays a function of the face SET, the row-order summation, and mutation tests of the checkers that
tests/test_mesh_smooth_gpu.py applies to the device's arrays: every deliberate error must be caught. No GPU."""
import inspect

import numpy as np
import pytest

from tests.helpers import mc_ref as R
from tests.helpers import mesh_smooth_ref as S


def test_taubin_smooths_the_sphere_and_keeps_its_volume():
    """The marching-cubes mesh of a near-binary alpha sphere is a staircase. Ten lambda | mu iterations at least halve the mean
    deviation of the face normals from the radial direction and change the enclosed volume by at most 2 %; ten plain Laplacian
    iterations (mu = 0) shrink it by at least 5 %. Together: the mu pass is there and has the right sign. Measured on this sphere
    (1332 vertices, valence 4..9): 19.15 -> 5.02 degrees (0.26 x), volume -0.64 %, Laplacian -9.97 %."""
    v, f, _ = S.mc_mesh("sphere")
    assert R.is_closed_oriented_manifold(f) and R.euler_characteristic(len(v), f) == 2
    deg = np.diff(S.adjacency(f, len(v))[0])
    c = S.SPHERE["c"]
    dev0, vol0 = S.mean_normal_deviation_deg(v, f, c), R.signed_volume(v, f)
    t = S.smooth(v, f, iterations=10)
    dev1, vol1 = S.mean_normal_deviation_deg(t, f, c), R.signed_volume(t, f)
    lap = S.smooth(v, f, iterations=10, mu=0.0)
    vol2 = R.signed_volume(lap, f)
    print(f"sphere: V {len(v)} F {len(f)} valence {deg.min()}..{deg.max()}; normal deviation {dev0:.2f} -> {dev1:.2f} deg "
          f"({dev1 / dev0:.2f} x); volume {vol0:.1f} -> {vol1:.1f} ({(vol1 - vol0) / vol0 * 100:+.2f} %); Laplacian {vol2:.1f} "
          f"({(vol2 - vol0) / vol0 * 100:+.2f} %)")
    assert dev1 <= 0.5 * dev0
    assert abs(vol1 - vol0) <= 0.02 * vol0
    assert vol2 <= 0.95 * vol0


@pytest.mark.parametrize("name", ["ellipsoid", "torus"])
def test_vertex_normals_agree_with_the_marching_cubes_normals(name):
    v, f, n = S.mc_mesh(name)
    got = S.vertex_normals(v, f)
    dots = (got.astype(np.float64) * n).sum(-1)
    print(name, "min dot", dots.min())
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert (dots > 0.8).all()


def test_row_sums_run_in_row_order():
    """row_sum against a plain Python loop over every entry, bit for bit, on the small meshes (rows of 1 to 300 entries); values
    whose sum depends on the order, so another order would show."""
    for name, (v, f) in S.small_meshes().items():
        off, nbr = S.adjacency(f, len(v))
        x = (v.astype(np.float64) * 1e8 + np.random.default_rng(1).uniform(-1, 1, v.shape)) * np.array([1.0, 1e-9, 1e9])
        assert S.same_bits(S.row_sum(off, nbr, x), S.row_sum_loop(off, nbr, x)), name
        if np.diff(off).max() >= 8:
            rev = nbr.copy()
            for r in range(len(off) - 1):
                rev[off[r]:off[r + 1]] = nbr[off[r]:off[r + 1]][::-1]
            assert not S.same_bits(S.row_sum(off, rev, x), S.row_sum(off, nbr, x)), name
        voff, vrows = S.vertex_faces(f, len(v))
        cr = S.face_cross(v, f) * 1e3 + 1.0
        assert S.same_bits(S.row_sum(voff, vrows, cr), S.row_sum_loop(voff, vrows, cr)), name


def test_adjacency_definition_on_the_small_meshes():
    meshes = S.small_meshes()
    v, f = meshes["octahedron+loose"]
    off, nbr = S.adjacency(f, len(v))
    assert off.dtype == np.int64 and nbr.dtype == np.int32
    assert np.diff(off).tolist() == [4, 4, 4, 4, 4, 4, 0]
    assert nbr[off[4]:off[5]].tolist() == [0, 1, 2, 3]
    # a duplicated face adds nothing; the degenerate (6, 6, 0) face adds the edge {6, 0} and no loop
    v2, f2 = meshes["duplicate+degenerate"]
    off2, nbr2 = S.adjacency(f2, len(v2))
    assert np.diff(off2).tolist() == [5, 4, 4, 4, 4, 4, 1] and nbr2[off2[6]:off2[7]].tolist() == [0] and 6 in nbr2[off2[0]:off2[1]]
    voff, vrows = S.vertex_faces(f2, len(v2))
    assert vrows[voff[6]:voff[7]].tolist() == [9]           # the face holds vertex 6 twice and counts once
    assert np.all(S.vertex_normals(v2, f2)[6] == 0)         # a vertex of degenerate faces only
    assert np.all(S.vertex_normals(v, f)[6] == 0)           # a vertex of no face
    for k in (63, 64, 65, 300):
        off, _ = S.adjacency(meshes[f"fan{k}"][1], k + 1)
        assert off[1] == k and set(np.diff(off)[1:]) == {3}
    e = np.zeros((0, 3), np.int32)
    off, nbr = S.adjacency(e, 0)
    assert off.tolist() == [0] and nbr.shape == (0,)
    off, nbr = S.adjacency(e, 5)
    assert off.tolist() == [0] * 6 and nbr.shape == (0,)
    assert S.smooth(np.zeros((0, 3), np.float32), e).shape == (0, 3) and S.vertex_normals(np.zeros((0, 3), np.float32), e).shape == (0, 3)


@pytest.mark.parametrize("name", ["noise", "sphere", "fan65", "strip257", "duplicate+degenerate"])
def test_invariant_under_face_order_and_index_rotation(name):
    v, f = S.mc_mesh(name)[:2] if name in ("noise", "sphere") else S.small_meshes()[name]
    rng = np.random.default_rng(7)
    g = f[rng.permutation(len(f))]
    rot = rng.integers(0, 3, len(g))
    g = np.stack([g[np.arange(len(g)), (rot + k) % 3] for k in range(3)], -1).astype(np.int32)
    assert not np.array_equal(f, g)
    a, b = S.adjacency(f, len(v)), S.adjacency(g, len(v))
    assert S.same_bits(a[0], b[0]) and S.same_bits(a[1], b[1])
    assert S.same_bits(S.smooth(v, f, iterations=3), S.smooth(v, g, iterations=3))


@pytest.mark.parametrize("name", ["sphere", "fan65", "octahedron+loose"])
def test_the_checkers_catch_every_mutation(name):
    v, f = S.mc_mesh(name)[:2] if name == "sphere" else S.small_meshes()[name]
    V = len(v)
    off, nbr = S.adjacency(f, V)
    assert S.check_adjacency(off, nbr, f, V) == []
    assert S.check_positions(S.smooth(v, f, iterations=3), v, f, iterations=3) == []
    assert S.check_normals(S.vertex_normals(v, f), v, f) == []
    assert "unsorted" in S.check_adjacency(*S.adjacency(f, V, mutate="unsorted_row"), f, V)
    assert "duplicate" in S.check_adjacency(*S.adjacency(f, V, mutate="duplicate_neighbour"), f, V)
    for m in ("mu_sign", "degree_plus_one", "float32_accumulator"):
        assert S.check_positions(S.smooth(v, f, iterations=3, mutate=m), v, f, iterations=3) == ["bits"], m
    # (a row walked in another order changes the float64 sums by an ulp of float64, which the one rounding to float32 almost always
    # hides: the order is held through the adjacency's rows, which the checker above compares bit for bit)
    wrong = S.vertex_normals(v, f[:, [0, 2, 1]])
    assert S.check_normals(wrong, v, f) == ["bits"]
    assert set(S.MUTATIONS) == {"unsorted_row", "duplicate_neighbour", "mu_sign", "degree_plus_one", "float32_accumulator"}


def test_fixed_vertices_and_zero_iterations():
    v, f, _ = S.mc_mesh("ellipsoid")
    assert S.same_bits(S.smooth(v, f, iterations=0), v)
    fixed = np.zeros(len(v), bool)
    fixed[::3] = True
    out = S.smooth(v, f, iterations=3, fixed=fixed)
    assert S.same_bits(out[fixed], v[fixed]) and not np.array_equal(out[~fixed], v[~fixed])
    loose_v, loose_f = S.small_meshes()["octahedron+loose"]
    assert S.same_bits(S.smooth(loose_v, loose_f, iterations=3)[6], loose_v[6])


def test_public_surface():
    import text2nerf_amd as T
    from text2nerf_amd import _lib, mesh
    assert T.mesh_adjacency is mesh.mesh_adjacency and T.smooth_mesh is mesh.smooth_mesh and T.vertex_normals is mesh.vertex_normals
    assert T.Adjacency is mesh.Adjacency and mesh.Adjacency._fields == ("offsets", "neighbours")
    assert [(p.name, p.default) for p in inspect.signature(mesh.smooth_mesh).parameters.values()] == [
        ("mesh", inspect.Parameter.empty), ("iterations", 10), ("lamb", 0.5), ("mu", -0.53), ("fixed", None), ("adjacency", None)]
    sig = inspect.signature(T.TensorBase.export_surface)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("path", None), ("level", 0.005), ("gridSize", None), ("colors", True), ("normals", True), ("surface", "alpha"), ("smooth", 0)]
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t2n.h")).read()
    declared = set(re.findall(r"\b(t2n_[a-z0-9_]+)\s*\(", hdr))
    for name in ("t2n_mesh_csr_workspace_bytes", "t2n_mesh_edge_keys", "t2n_mesh_face_keys", "t2n_mesh_csr", "t2n_mesh_smooth_pass",
                 "t2n_mesh_vertex_normals"):
        assert name in declared and name in _lib.SIGNATURES, name


def test_library_argument_checks_run_without_a_gpu():
    import ctypes as C
    from text2nerf_amd import _lib
    lib = _lib.load()
    ws = lib.t2n_mesh_csr_workspace_bytes
    assert ws(0) > 0 and ws(6 * 1000) >= 6 * 1000 * 8 + 4 * 24 and ws(-1) == 0 and ws(2**31) == 0 and ws(2**31 - 1) > 0
    one = C.c_void_p(256)            # never dereferenced: every call below is refused before any HIP call
    bad = -1                         # T2N_ERR_INVALID
    big = (2**31 - 1) // 6 + 1
    for fn in (lib.t2n_mesh_edge_keys, lib.t2n_mesh_face_keys):
        assert fn(None, 4, 4, one, None) == bad and b"_keys" in lib.t2n_last_error()
        assert fn(one, 4, 4, None, None) == bad and fn(one, -1, 4, one, None) == bad and fn(one, 4, 2**31, one, None) == bad
        assert fn(one, big, 4, one, None) == bad
    csr = lambda keys=one, n=8, rows=4, off=one, val=one, cnt=one, w=one, nb=1 << 20: lib.t2n_mesh_csr(keys, n, rows, off, val, cnt, w, nb, None)  # noqa: E731
    assert csr(keys=None) == bad and b"t2n_mesh_csr" in lib.t2n_last_error()
    assert csr(off=None) == bad and csr(val=None) == bad and csr(cnt=None) == bad and csr(w=None) == bad
    assert csr(n=-1) == bad and csr(n=2**31) == bad and csr(rows=-1) == bad and csr(rows=2**31) == bad and csr(nb=int(ws(8)) - 1) == bad
    two = C.c_void_p(512)
    sp = lambda a=one, b=two, off=one, nbr=one, E=8, V=4, s=0.5: lib.t2n_mesh_smooth_pass(a, b, off, nbr, E, None, V, s, None)  # noqa: E731
    assert sp(a=None) == bad and b"t2n_mesh_smooth_pass" in lib.t2n_last_error()
    assert sp(b=None) == bad and sp(off=None) == bad and sp(nbr=None) == bad and sp(b=one) == bad
    assert sp(E=-1) == bad and sp(V=-1) == bad and sp(V=2**31) == bad and sp(s=float("nan")) == bad and sp(s=float("inf")) == bad
    vn = lambda v=one, f=one, F=4, off=one, rows=one, E=12, V=4, out=one: lib.t2n_mesh_vertex_normals(v, f, F, off, rows, E, V, out, None)  # noqa: E731
    assert vn(v=None) == bad and b"t2n_mesh_vertex_normals" in lib.t2n_last_error()
    assert vn(f=None) == bad and vn(off=None) == bad and vn(rows=None) == bad and vn(out=None) == bad
    assert vn(F=-1) == bad and vn(F=big) == bad and vn(E=-1) == bad and vn(V=2**31) == bad


def test_no_cpu_fallback(monkeypatch):
    import torch
    from text2nerf_amd import _lib, mesh
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    v, f = S.small_meshes()["tetrahedron"]
    for call in (lambda: mesh.mesh_adjacency(f, 4), lambda: mesh.vertex_normals(v, f), lambda: mesh.smooth_mesh((v, f))):
        with pytest.raises(_lib.T2NError):
            call()
    # what is refused is refused before the device is asked for
    for kw in (dict(iterations=-1), dict(lamb=0.0), dict(lamb=1.5), dict(mu=0.1)):
        with pytest.raises(ValueError):
            mesh.smooth_mesh((v, f), **kw)
