"""The float64 reference of the simplification stage (tests/helpers/mesh_simplify_ref.py) on its own: the definition's properties, what
quadric placement is for (it keeps the enclosed volume closer to the input's than the mean does), that duplicate removal is exercised,
mutation tests of the checkers that tests/test_mesh_simplify_gpu.py applies to the device's arrays (every deliberate error must be
caught), and the argument checks of mesh_clusters / simplify_mesh and of the library, which come before any launch. No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

from tests.helpers import mc_ref as R
from tests.helpers import mesh_simplify_ref as Q
from tests.helpers import mesh_smooth_ref as S

MC = ("sphere", "ellipsoid", "torus", "noise")


def get(name):
    return S.mc_mesh(name)[:2] if name in MC else S.small_meshes()[name]


def shuffled(f, seed=7):
    """The faces in another order, every one with its indices rotated."""
    rng = np.random.default_rng(seed)
    g = f[rng.permutation(len(f))]
    rot = rng.integers(0, 3, len(g))
    return np.stack([g[np.arange(len(g)), (rot + k) % 3] for k in range(3)], -1).astype(np.int32)


@pytest.mark.parametrize("name", MC + ("fan300", "strip257", "duplicate+degenerate"))
def test_output_faces_and_boxes(name):
    """Three distinct indices < K, no rotated triple twice; every representative inside its cell's box, under both placements (the
    float32 rounding may move a point on the box's face by half an ulp: the float64 point is tested, and the float32 one to an ulp)."""
    v, f = get(name)
    for cell in (1.0, 2.0, 3.0, (1.5, 0.7, 2.2)):
        for pl in ("mean", "quadric"):
            out = Q.simplify(v, f, cell, placement=pl)
            K = out.clusters.n_clusters
            assert out.verts.shape == (K, 3) and out.verts.dtype == np.float32 and out.faces.dtype == np.int32
            assert Q.check_faces(out.faces, K) == [], (name, cell, pl)
            o, h = Q.grid(v, cell)
            p, _ = Q.place(v, f, out.clusters, cell, placement=pl)
            c = out.clusters.cells.astype(np.float64)
            lo, hi = o + c * h, o + (c + 1) * h
            if pl == "quadric":
                assert ((p >= lo) & (p <= hi)).all(), (name, cell)
            tol = np.spacing(np.abs(out.verts).astype(np.float32)).astype(np.float64) + 1e-12
            assert ((out.verts >= lo - tol) & (out.verts <= hi + tol)).all(), (name, cell, pl)


def test_clusters_definition():
    v, f, cell, origin = Q.collapse_case()
    cl = Q.clusters(v, cell, origin)
    assert cl.n_clusters == 5 and cl.vertex_map.dtype == np.int32 and cl.offsets.dtype == np.int64 and cl.members.dtype == np.int32
    # ids (c0 n1 + c1) n2 + c2 with n = (5, 5, 2): A (2,0,0) = 20, B (4,0,0) = 40, C (2,2,0) = 24, D (4,2,1) = 45, vertex 7 (0,4,0) = 8
    assert cl.vertex_map.tolist() == [1, 1, 3, 3, 2, 2, 4, 0]
    assert cl.offsets.tolist() == [0, 1, 3, 5, 7, 8] and cl.members.tolist() == [7, 0, 1, 4, 5, 2, 3, 6]
    assert cl.cells.tolist() == [[0, 4, 0], [2, 0, 0], [2, 2, 0], [4, 0, 0], [4, 2, 1]]
    out = Q.simplify(v, f, cell, origin)
    assert out.faces.tolist() == [[1, 3, 2], [1, 2, 3], [1, 3, 4]] and out.n_duplicates == 2 and out.n_degenerate == 2
    assert S.same_bits(out.verts[0], v[7]) and S.same_bits(out.verts[4], v[6])       # clusters of one vertex: itself, with or without faces
    e = Q.clusters(np.zeros((0, 3), np.float32), 1.0)
    assert e.n_clusters == 0 and e.offsets.tolist() == [0] and e.cells.shape == (0, 3)
    es = Q.simplify(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 1.0)
    assert es.verts.shape == (0, 3) and es.faces.shape == (0, 3)


@pytest.mark.parametrize("name", list(S.small_meshes()))
def test_a_cell_that_isolates_every_vertex_permutes_the_mesh(name):
    """Under the mean the positions are the input's bits. Under the quadric a lone vertex lies on the plane of each of its faces, so
    r = n . (x_a - x) is 0 up to its rounding: |r| <= 4 * 2^-52 |n| |x_a - x| (the rounded differences, three products, two sums), and
    |x| <= max |r| / |n| / regularisation <= 1e-12 times the mesh's extent at 1e-3. That moves no coordinate a float32 can tell from
    its neighbour unless the coordinate is itself rounding noise (the fans' sin(pi) = 1e-16): bound, not bits."""
    v, f = get(name)
    h = Q.isolating_cell(v)
    extent = float(np.abs(v.astype(np.float64).max(0) - v.min(0)).max())
    for pl in ("mean", "quadric"):
        out = Q.simplify(v, f, h, placement=pl)
        cl = out.clusters
        assert cl.n_clusters == len(v)
        if pl == "mean":
            assert S.same_bits(out.verts, v[cl.members]), name
        else:
            assert np.abs(out.verts.astype(np.float64) - v[cl.members]).max() <= 1e-12 * extent, name
        live = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]
        want = Q.rotate_min_first(cl.vertex_map[live])
        _, first = np.unique(want, axis=0, return_index=True)             # the input's own duplicate faces leave, nothing else
        assert np.array_equal(out.faces, want[np.sort(first)]), (name, pl)
        if name not in ("duplicate+degenerate",):
            assert len(out.faces) == len(f)


@pytest.mark.parametrize("name", MC + ("fan300", "strip256"))
def test_one_cell_for_everything(name):
    v, f = get(name)
    for pl in ("mean", "quadric"):
        out = Q.simplify(v, f, 1000.0, origin=(-500.0, -500.0, -500.0), placement=pl)
        assert out.clusters.n_clusters == 1 and out.verts.shape == (1, 3) and len(out.faces) == 0 and out.n_degenerate == len(f)


@pytest.mark.parametrize("name", ["noise", "sphere", "fan65", "strip257", "duplicate+degenerate"])
def test_invariant_under_face_order_and_index_rotation(name):
    """Index rotation cannot matter (the quadric rotates every face to its smallest index first). Face order enters through the order of
    the float64 sums alone, an ulp of float64 before the one rounding to float32: the positions are equal on these meshes, the kept
    faces are the same set, in the order of the permuted input."""
    v, f = get(name)
    g = shuffled(f)
    assert not np.array_equal(f, g)
    rolled = np.roll(f, 1, axis=1)
    for cell in (1.0, 2.0):
        a, b, c = Q.simplify(v, f, cell, normals=True), Q.simplify(v, g, cell, normals=True), Q.simplify(v, rolled, cell, normals=True)
        assert all(S.same_bits(x, y) for x, y in zip(a[:3], c[:3])), name
        assert S.same_bits(a.verts, b.verts), name
        key = lambda t: t[np.lexsort(t.T[::-1])]            # noqa: E731
        assert np.array_equal(key(a.faces), key(b.faces)), name


def test_colour_means_are_exact_integers():
    v, f = S.fan(300)
    rng = np.random.default_rng(3)
    for colors in (np.full(v.shape, 255, np.uint8), np.zeros(v.shape, np.uint8), rng.integers(0, 256, v.shape).astype(np.uint8),
                   rng.choice(np.array([0, 255], np.uint8), v.shape)):
        for cell in (1000.0, 0.5):
            out = Q.simplify(v, f, cell, origin=(-500.0,) * 3 if cell == 1000.0 else None, colors=colors)
            cl = out.clusters
            assert out.colors.dtype == np.uint8 and out.colors.shape == (cl.n_clusters, 3)
            for k in range(cl.n_clusters):
                rows = cl.members[cl.offsets[k]:cl.offsets[k + 1]]
                for ch in range(3):
                    tot, n = sum(int(x) for x in colors[rows, ch]), len(rows)
                    assert int(out.colors[k, ch]) == (2 * tot + n) // (2 * n)       # round half up, in integers
    one = Q.simplify(v, f, 1000.0, origin=(-500.0,) * 3, colors=np.full(v.shape, 255, np.uint8))
    assert one.clusters.n_clusters == 1 and one.colors.tolist() == [[255, 255, 255]]      # 301 * 255 = 76755 passes 16 bits


def test_quadric_placement_keeps_the_volume_better_than_the_mean():
    """Sphere, ellipsoid and torus at cells 1, 2 and 3: |volume(quadric) - volume(input)| < |volume(mean) - volume(input)| in all nine
    cases, with the fixed-order cofactor solve. The figures are profiles/mesh_simplify.txt (Q.report)."""
    for line in Q.report():
        print(line)
    for name in ("sphere", "ellipsoid", "torus"):
        v, f, _ = S.mc_mesh(name)
        vol = R.signed_volume(v, f)
        for cell in (1.0, 2.0, 3.0):
            a, b = Q.simplify(v, f, cell, placement="mean"), Q.simplify(v, f, cell)
            va, vb = R.signed_volume(a.verts, a.faces), R.signed_volume(b.verts, b.faces)
            assert abs(vb - vol) < abs(va - vol), (name, cell, vol, va, vb)


def test_duplicate_removal_is_exercised():
    v, f, _ = S.mc_mesh("noise")
    dup = {cell: Q.simplify(v, f, cell).n_duplicates for cell in (1.0, 2.0, 3.0)}
    print("duplicates removed on the noise mesh:", dup)
    assert dup[2.0] > 0 and dup[3.0] > 0


@pytest.mark.parametrize("name", ["sphere", "noise"])
def test_the_checkers_catch_every_mutation(name):
    v, f = get(name)
    colors = np.random.default_rng(5).integers(0, 256, v.shape).astype(np.uint8)
    caught = {m: set() for m in Q.MUTATIONS}
    for cell in (1.0, 2.0, 3.0):
        kw = dict(normals=True, colors=colors)
        good = Q.simplify(v, f, cell, **kw)
        assert Q.check_mesh(good[:4], v, f, cell, **kw) == [] and Q.check_clusters(good.clusters, v, cell) == []
        for m in Q.MUTATIONS:
            caught[m] |= set(Q.check_mesh(Q.simplify(v, f, cell, mutate=m, **kw)[:4], v, f, cell, **kw))
        # degenerate faces and duplicates also fail the structural check, whatever the reference says
        assert "degenerate" in Q.check_faces(Q.simplify(v, f, cell, mutate="degenerate_kept").faces, good.clusters.n_clusters)
        # a face row walked backwards changes the float64 sums by an ulp, which the one rounding to float32 hides on these meshes
        # (caught[...] stays empty): the order is held through the cluster -> face rows, which the GPU file compares bit for bit
        cl = good.clusters
        off, rows = Q.cluster_faces(f, cl.vertex_map, cl.n_clusters)
        assert Q.check_face_rows(off, rows, f, cl.vertex_map, cl.n_clusters) == []
        k = int(np.argmax(np.diff(off) >= 2))
        rev = rows.copy()
        rev[off[k]:off[k + 1]] = rows[off[k]:off[k + 1]][::-1]
        assert "unsorted" in Q.check_face_rows(off, rev, f, cl.vertex_map, cl.n_clusters)
        p64 = Q.place(v, f, cl, cell)[0]
        assert not S.same_bits(p64, Q.place(v, f, cl, cell, mutate="unsorted_faces")[0]), "the order shows in float64"
        # a cluster map off by one vertex
        vm = cl.vertex_map.copy()
        vm[0] = (vm[0] + 1) % cl.n_clusters
        assert "vertex_map" in Q.check_clusters(Q.Clusters(vm, cl.n_clusters, cl.offsets, cl.members, cl.cells), v, cell)
    for m in ("float32_accumulator", "normalised_n", "no_regularisation", "no_cell_fallback"):
        assert "verts" in caught[m], m
    assert "faces" in caught["degenerate_kept"] and "colors" in caught["colour_no_rounding"]
    if name == "noise":             # the mesh with duplicates
        assert "faces" in caught["duplicate_keeps_higher"]
    assert caught["unsorted_faces"] == set()
    assert set(Q.MUTATIONS) == {"float32_accumulator", "unsorted_faces", "normalised_n", "no_regularisation", "no_cell_fallback",
                                "duplicate_keeps_higher", "degenerate_kept", "colour_no_rounding"}


def test_value_errors_come_before_any_launch(monkeypatch):
    """With a loader that fails: every refusal below is raised from the arguments and the positions' min / max alone."""
    from text2nerf_amd import _lib, mesh

    def no_load(*a, **k):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    v, f = S.small_meshes()["tetrahedron"]
    nan, inf = float("nan"), float("inf")
    calls = [lambda **kw: mesh.mesh_clusters(kw.pop("verts", v), kw.pop("cell", 0.5), **kw),
             lambda **kw: mesh.simplify_mesh((kw.pop("verts", v), f), kw.pop("cell", 0.5), **kw)]
    bad_v = v.copy()
    bad_v[2, 1] = nan
    inf_v = v.copy()
    inf_v[1, 0] = -inf
    for call in calls:
        for cell in (0.0, -1.0, nan, inf, (1.0, 2.0), (1.0, 0.0, 1.0), (1.0, 1.0, 1.0, 1.0), "x"):
            with pytest.raises(ValueError):
                call(cell=cell)
        for verts in (bad_v, inf_v, v[:, :2], v.reshape(-1), np.zeros((2, 3, 3), np.float32)):
            with pytest.raises(ValueError):
                call(verts=verts)
        for origin in ((0.5, 0.0, 0.0), (0.0, 0.0, 1e-3), (nan, 0.0, 0.0), (0.0, 0.0)):
            with pytest.raises(ValueError):
                call(origin=origin)
        with pytest.raises(ValueError):
            call(cell=1e-4, verts=v * 10)                       # 12346^3 cells
        with pytest.raises(ValueError):
            call(cell=1e-300)                                   # a quotient that is not finite
        with pytest.raises(ValueError):
            call(cell=1.0, origin=(-3000.0, -3000.0, -3000.0), verts=v)       # 3001^3 cells from a far origin
    for kw in (dict(placement="median"), dict(regularisation=-1e-3), dict(regularisation=nan), dict(regularisation=inf)):
        with pytest.raises(ValueError):
            mesh.simplify_mesh((v, f), 0.5, **kw)
    with pytest.raises(ValueError):
        mesh.simplify_mesh((v,), 0.5)
    with pytest.raises(AssertionError):                         # a good call does reach the loader
        mesh.mesh_clusters(v, 0.5)


def test_no_cpu_fallback(monkeypatch):
    import torch
    from text2nerf_amd import _lib, mesh
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    v, f = S.small_meshes()["tetrahedron"]
    for call in (lambda: mesh.mesh_clusters(v, 0.5), lambda: mesh.simplify_mesh((v, f), 0.5), lambda: mesh.simplify_mesh((v, f), 0.5, placement="mean")):
        with pytest.raises(_lib.T2NError):
            call()


def test_public_surface():
    import text2nerf_amd as T
    from text2nerf_amd import _lib, mesh
    assert T.mesh_clusters is mesh.mesh_clusters and T.simplify_mesh is mesh.simplify_mesh and T.Clusters is mesh.Clusters
    assert mesh.Clusters._fields == ("vertex_map", "n_clusters", "offsets", "members", "cells")
    params = lambda fn: [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]         # noqa: E731
    assert params(mesh.mesh_clusters) == [("verts", inspect.Parameter.empty), ("cell", inspect.Parameter.empty), ("origin", None)]
    assert params(mesh.simplify_mesh) == [("mesh", inspect.Parameter.empty), ("cell", inspect.Parameter.empty), ("origin", None),
                                          ("placement", "quadric"), ("regularisation", 1e-3), ("clusters", None)]
    assert "manifold" in mesh.simplify_mesh.__doc__
    # existing signatures stay as they are
    assert params(mesh.smooth_mesh)[1:] == [("iterations", 10), ("lamb", 0.5), ("mu", -0.53), ("fixed", None), ("adjacency", None)]
    assert [n for n, _ in params(T.TensorBase.export_surface)][1:] == ["path", "level", "gridSize", "colors", "normals", "surface", "smooth"]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "t2n.h")).read()
    declared = set(re.findall(r"\b(t2n_[a-z0-9_]+)\s*\(", hdr))
    for name in ("t2n_mesh_cluster_keys", "t2n_mesh_cluster_rows_workspace_bytes", "t2n_mesh_cluster_rows", "t2n_mesh_cluster_face_keys",
                 "t2n_mesh_cluster_place", "t2n_mesh_cluster_colors", "t2n_mesh_simplify_face_map", "t2n_mesh_simplify_faces_workspace_bytes",
                 "t2n_mesh_simplify_faces"):
        assert name in declared and name in _lib.SIGNATURES, name


def test_library_argument_checks_run_without_a_gpu():
    import ctypes as C
    from text2nerf_amd import _lib
    lib = _lib.load()
    one, two = C.c_void_p(256), C.c_void_p(512)      # never dereferenced: every call below is refused before any HIP call
    bad = -1                                         # T2N_ERR_INVALID
    d3, i3 = (lambda *x: (C.c_double * 3)(*x)), (lambda *x: (C.c_int32 * 3)(*x))
    o, h, n = d3(0, 0, 0), d3(1, 1, 1), i3(4, 4, 4)
    big_f = (2**31 - 1) // 3 + 1
    nan, inf = float("nan"), float("inf")

    keys = lambda v=one, V=4, o=o, h=h, n=n, k=one: lib.t2n_mesh_cluster_keys(v, V, o, h, n, k, None)       # noqa: E731
    assert keys(v=None) == bad and b"t2n_mesh_cluster_keys" in lib.t2n_last_error()
    assert keys(k=None) == bad and keys(V=-1) == bad and keys(V=2**31) == bad and keys(o=None) == bad and keys(h=None) == bad and keys(n=None) == bad
    assert keys(h=d3(1, 0, 1)) == bad and keys(h=d3(1, nan, 1)) == bad and keys(h=d3(inf, 1, 1)) == bad and keys(h=d3(1, 1, -1)) == bad
    assert keys(o=d3(0, nan, 0)) == bad and keys(o=d3(inf, 0, 0)) == bad
    assert keys(n=i3(0, 4, 4)) == bad and keys(n=i3(2048, 1024, 1024)) == bad and keys(n=i3(-1, 4, 4)) == bad

    ws = lib.t2n_mesh_cluster_rows_workspace_bytes
    assert ws(0) > 0 and ws(1000) >= 4 * 4 and ws(-1) == 0 and ws(2**31) == 0 and ws(2**31 - 1) > 0
    rows = lambda k=one, V=4, n=n, vm=one, off=one, mem=one, ce=one, cnt=one, w=one, nb=1 << 20: lib.t2n_mesh_cluster_rows(  # noqa: E731
        k, V, n, vm, off, mem, ce, cnt, w, nb, None)
    assert rows(k=None) == bad and b"t2n_mesh_cluster_rows" in lib.t2n_last_error()
    assert rows(vm=None) == bad and rows(off=None) == bad and rows(mem=None) == bad and rows(ce=None) == bad and rows(cnt=None) == bad
    assert rows(w=None) == bad and rows(V=-1) == bad and rows(V=2**31) == bad and rows(n=None) == bad and rows(n=i3(4, 0, 4)) == bad
    assert rows(nb=int(ws(4)) - 1) == bad

    fk = lambda f=one, F=4, V=4, vm=one, K=2, k=one: lib.t2n_mesh_cluster_face_keys(f, F, V, vm, K, k, None)        # noqa: E731
    assert fk(f=None) == bad and b"t2n_mesh_cluster_face_keys" in lib.t2n_last_error()
    assert fk(vm=None) == bad and fk(k=None) == bad and fk(F=-1) == bad and fk(F=big_f) == bad and fk(V=2**31) == bad and fk(V=-1) == bad
    assert fk(K=-1) == bad and fk(K=5) == bad

    def place(v=one, V=4, f=one, F=4, off=one, mem=one, M=4, ce=one, K=2, foff=one, frow=one, E=6, o=o, h=h, reg=1e-3, q=1, out=two):
        return lib.t2n_mesh_cluster_place(v, V, f, F, off, mem, M, ce, K, foff, frow, E, o, h, reg, q, out, None)
    assert place(v=None) == bad and b"t2n_mesh_cluster_place" in lib.t2n_last_error()
    for kw in (dict(f=None), dict(off=None), dict(mem=None), dict(ce=None), dict(foff=None), dict(frow=None), dict(out=None), dict(o=None),
               dict(h=None), dict(V=-1), dict(V=2**31), dict(F=-1), dict(F=big_f), dict(M=-1), dict(K=-1), dict(K=5), dict(E=-1),
               dict(h=d3(0, 1, 1)), dict(h=d3(1, 1, nan)), dict(o=d3(0, 0, inf)), dict(reg=-1.0), dict(reg=nan), dict(reg=inf), dict(q=2),
               dict(q=-1), dict(q=0, v=None), dict(q=0, out=None)):
        assert place(**kw) == bad, kw

    col = lambda c=one, V=4, off=one, mem=one, M=4, K=2, out=two: lib.t2n_mesh_cluster_colors(c, V, off, mem, M, K, out, None)      # noqa: E731
    assert col(c=None) == bad and b"t2n_mesh_cluster_colors" in lib.t2n_last_error()
    assert col(off=None) == bad and col(mem=None) == bad and col(out=None) == bad and col(V=-1) == bad and col(V=2**31) == bad
    assert col(M=-1) == bad and col(K=-1) == bad and col(K=5) == bad

    fm = lambda f=one, F=4, V=4, vm=one, K=2, r=one, hi=one, lo=one: lib.t2n_mesh_simplify_face_map(f, F, V, vm, K, r, hi, lo, None)      # noqa: E731
    assert fm(f=None) == bad and b"t2n_mesh_simplify_face_map" in lib.t2n_last_error()
    assert fm(vm=None) == bad and fm(r=None) == bad and fm(hi=None) == bad and fm(lo=None) == bad and fm(F=-1) == bad and fm(F=big_f) == bad
    assert fm(V=-1) == bad and fm(V=2**31) == bad and fm(K=-1) == bad and fm(K=5) == bad

    wf = lib.t2n_mesh_simplify_faces_workspace_bytes
    assert wf(0) > 0 and wf(1000) >= 1000 + 4 * 4 and wf(-1) == 0 and wf(big_f) == 0 and wf(big_f - 1) > 0
    sf = lambda r=one, order=one, F=4, out=one, cnt=one, w=one, nb=1 << 20: lib.t2n_mesh_simplify_faces(r, order, F, out, cnt, w, nb, None)   # noqa: E731
    assert sf(r=None) == bad and b"t2n_mesh_simplify_faces" in lib.t2n_last_error()
    assert sf(order=None) == bad and sf(out=None) == bad and sf(cnt=None) == bad and sf(w=None) == bad and sf(F=-1) == bad and sf(F=big_f) == bad
    assert sf(nb=int(wf(4)) - 1) == bad
    # empty inputs that need no launch are accepted without a device
    assert keys(V=0, v=None, k=None) == 0 and fk(F=0, f=None, k=None) == 0 and fm(F=0, f=None) == 0
    assert place(K=0, V=0, v=None, out=None) == 0 and col(K=0, V=0, c=None) == 0
