"""Mesh export without a GPU: the generated case table (tools/gen_mc_table.py -> csrc/t2n_mc_table.h), the numpy restatement the
GPU tests compare with (tests/helpers/mc_ref.py) judged by properties that do not depend on it, the PLY writer, the reference's
signature and the library's argument checks."""
import ctypes as C
import inspect
import itertools
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import mc_ref as R
from text2nerf_amd import _lib, mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GEN = R.GEN


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def test_committed_header_is_the_generators_output():
    assert open(GEN.HEADER).read() == GEN.render()


def test_prototype_numbers():
    assert R.STATS == {"empty_cases": 2, "triangles": 820, "max_triangles": 5, "longest_loop": 7}
    assert R.NTRI.shape == (256,) and R.TRI.shape == (256, 5, 3)
    assert int((R.NTRI == 0).sum()) == 2 and int(R.NTRI.sum()) == 820 and int(R.NTRI.max()) == 5
    assert max(len(loop) for case in range(256) for loop in GEN.loops_of(case)) == 7


def _crossed(case):
    return sorted(e for e in range(12) if (case >> GEN.edge_corners(e)[0] & 1) != (case >> GEN.edge_corners(e)[1] & 1))


def test_numbering_rules():
    for c in range(8):
        assert GEN.corner_offset(c) == (c & 1, c >> 1 & 1, c >> 2 & 1)
    for a, u, v in itertools.product(range(3), range(2), range(2)):
        lo, hi = GEN.edge_corners(4 * a + u + 2 * v)
        olo, ohi = GEN.corner_offset(lo), GEN.corner_offset(hi)
        others = [b for b in range(3) if b != a]
        assert olo[a] == 0 and ohi[a] == 1 and (olo[others[0]], olo[others[1]]) == (u, v) == (ohi[others[0]], ohi[others[1]])
        assert GEN.edge_owner_offset(4 * a + u + 2 * v) == olo


def test_loops_use_each_crossed_edge_exactly_once():
    for case in range(256):
        used = sorted(e for loop in GEN.loops_of(case) for e in loop)
        assert used == _crossed(case), case
        tri_edges = {int(e) for t in R.TRI[case, :R.NTRI[case]] for e in t}
        assert tri_edges == set(used), case
        assert sum(len(loop) - 2 for loop in GEN.loops_of(case)) == R.NTRI[case], case


def test_cells_sharing_a_face_agree_on_its_segments():
    """Every ordered pair of cases, each axis: where the first cell's high face and the second's low face hold equal corner bits, the
    two put the same segments on it (as pairs of grid edges: a face edge of the high side is the low side's edge + the axis step)."""
    for d in range(3):
        lo_face, hi_face = GEN.FACES[2 * d], GEN.FACES[2 * d + 1]
        # the low face's edge that coincides with a high-face edge of the neighbour below: same axis and offsets apart from d
        def twin(e_hi):
            lo_c, hi_c = GEN.edge_corners(e_hi)
            want = (lo_c & ~(1 << d), hi_c & ~(1 << d))
            return next(e for e in lo_face[1] if GEN.edge_corners(e) == want)
        pairs = 0
        for A in range(256):
            bits_hi = tuple(A >> c & 1 for c in hi_face[0])
            seg_a = sorted(tuple(sorted(twin(e) for e in s)) for s in GEN.face_segments(A, hi_face))
            for B in range(256):
                if tuple(B >> c & 1 for c in lo_face[0]) != bits_hi:
                    continue
                pairs += 1
                assert sorted(GEN.face_segments(B, lo_face)) == seg_a, (d, A, B)
        assert pairs == 256 * 16


def test_no_triangle_has_an_in_face_diagonal():
    for case in range(256):
        segs = {s for face in GEN.FACES for s in GEN.face_segments(case, face)}
        for t in R.TRI[case, :R.NTRI[case]]:
            for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                pair = tuple(sorted((int(a), int(b))))
                assert pair in segs or not GEN.same_face(*pair), (case, t)


# ---- the restatement, by properties that do not depend on it ------------------------------------------------------------------------
def test_noise_volume_is_a_closed_oriented_manifold_with_every_case():
    vol = R.noise_volume()
    assert vol.shape == (14, 13, 15)
    inside = vol > 0
    case = sum(inside[(c & 1):13 + (c & 1), (c >> 1 & 1):12 + (c >> 1 & 1), (c >> 2 & 1):14 + (c >> 2 & 1)].astype(int) << c
               for c in range(8))
    assert len(np.unique(case)) == 255
    verts, faces, normals = R.marching_cubes(vol, 0.0)
    assert R.is_closed_oriented_manifold(faces) and np.isfinite(verts).all()
    assert faces.min() == 0 and faces.max() == len(verts) - 1 and len(np.unique(faces)) == len(verts)
    assert np.abs(np.linalg.norm(normals, axis=1) - 1).max() < 1e-6


def test_manifold_check_itself_rejects_broken_meshes():
    _, faces, _ = R.marching_cubes(R.ellipsoid_volume(), 0.0)
    assert R.is_closed_oriented_manifold(faces)
    assert not R.is_closed_oriented_manifold(faces[1:])                       # a hole
    flipped = faces.copy()
    flipped[0] = flipped[0, [0, 2, 1]]
    assert not R.is_closed_oriented_manifold(flipped)                         # one triangle turned over
    assert not R.is_closed_oriented_manifold(np.concatenate([faces, faces[:1]]))


def test_ellipsoid_euler_volume_and_orientation():
    verts, faces, normals = R.marching_cubes(R.ellipsoid_volume(), 0.0)
    assert R.is_closed_oriented_manifold(faces)
    assert R.euler_characteristic(len(verts), faces) == 2
    vol, exact = R.signed_volume(verts, faces), 4.0 / 3.0 * np.pi * 6 * 5 * 7.5
    print("ellipsoid volume", vol, "exact", exact, "ratio", vol / exact)
    assert vol > 0 and abs(vol - exact) <= 0.03 * exact
    # vertex normals point out of the body (towards lower values), like the analytic gradient
    g = (verts - np.array([9.3, 8.1, 11.2])) / np.array([6.0, 5.0, 7.5])**2
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    assert float((g * normals).sum(1).min()) > 0.99


def test_torus_has_characteristic_zero():
    verts, faces, _ = R.marching_cubes(R.torus_volume(), 0.0)
    assert R.is_closed_oriented_manifold(faces) and R.euler_characteristic(len(verts), faces) == 0
    assert R.signed_volume(verts, faces) > 0


def test_nonfinite_volume_gives_finite_vertices():
    vol = R.nonfinite_volume()
    assert np.isinf(vol).any() and np.isnan(vol).any()
    verts, faces, normals = R.marching_cubes(vol, 0.0)
    assert len(verts) > 100 and np.isfinite(verts).all() and np.isfinite(normals).all()
    assert R.is_closed_oriented_manifold(faces)


def test_spacing_origin_flip_and_single_cells():
    vol = R.ellipsoid_volume()
    v1, f1, _ = R.marching_cubes(vol, 0.0)
    v2, f2, _ = R.marching_cubes(vol, 0.0, spacing=(0.5, 2.0, 0.25), origin=(1.0, -2.0, 3.0), flip=True, normals=False)
    assert np.allclose(v2, v1 * np.array([0.5, 2.0, 0.25]) + np.array([1.0, -2.0, 3.0]), atol=1e-5)
    assert np.array_equal(f2, f1[:, [0, 2, 1]])
    for case in range(256):
        v, f, _ = R.marching_cubes(R.single_cell(case), 0.0)
        assert len(f) == R.NTRI[case] and len(v) == len(_crossed(case)), case


# ---- write_ply ------------------------------------------------------------------------------------------------------------------------
def test_write_ply_round_trip(tmp_path):
    verts, faces, normals = R.marching_cubes(R.ellipsoid_volume(), 0.0)
    colors = (np.random.default_rng(5).integers(0, 256, verts.shape)).astype(np.uint8)
    p = str(tmp_path / "plain.ply")
    mesh.write_ply(p, verts, faces)
    header, props, f = R.read_ply(p)
    assert header == ("ply\nformat binary_little_endian 1.0\n"
                      f"element vertex {len(verts)}\nproperty float x\nproperty float y\nproperty float z\n"
                      f"element face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n")
    assert np.array_equal(np.stack([props["x"], props["y"], props["z"]], -1), verts) and np.array_equal(f, faces)
    assert os.path.getsize(p) == len(header) + 12 * len(verts) + 13 * len(faces)
    p = str(tmp_path / "full.ply")
    mesh.write_ply(p, torch.from_numpy(verts), torch.from_numpy(faces), normals=normals, colors=torch.from_numpy(colors))
    header, props, f = R.read_ply(p)
    assert list(props) == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(np.stack([props["nx"], props["ny"], props["nz"]], -1), normals)
    assert np.array_equal(np.stack([props["red"], props["green"], props["blue"]], -1), colors) and np.array_equal(f, faces)
    p = str(tmp_path / "colors.ply")
    mesh.write_ply(p, verts, faces, colors=colors)
    assert list(R.read_ply(p)[1]) == ["x", "y", "z", "red", "green", "blue"]
    with pytest.raises(ValueError):
        mesh.write_ply(p, verts, faces, normals=normals[:-1])


# ---- surface ------------------------------------------------------------------------------------------------------------------------
def test_signature_matches_the_reference():
    ref = json.load(open(os.path.join(GOLDEN, "mesh_signatures.json")))
    assert list(ref) == ["convert_sdf_samples_to_ply"]
    for name, want in ref.items():
        got = [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(getattr(mesh, name)).parameters.values()]
        assert got == want, name


def test_public_names():
    import text2nerf_amd as T
    assert T.marching_cubes is mesh.marching_cubes and T.write_ply is mesh.write_ply and T.Mesh is mesh.Mesh
    assert T.convert_sdf_samples_to_ply is mesh.convert_sdf_samples_to_ply
    sig = inspect.signature(T.TensorBase.export_mesh)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("path", None), ("level", 0.005), ("gridSize", None), ("colors", True), ("normals", True)]
    assert [(p.name, p.default) for p in inspect.signature(mesh.marching_cubes).parameters.values()] == [
        ("volume", inspect.Parameter.empty), ("level", inspect.Parameter.empty), ("spacing", (1., 1., 1.)), ("origin", (0., 0., 0.)),
        ("normals", True), ("flip", False)]


def test_library_argument_checks_run_without_a_gpu():
    lib = _lib.load()
    ws = lib.t2n_mc_workspace_bytes
    assert ws(2, 2, 2) > 0 and ws(300, 300, 300) >= 300**3 * 5
    assert ws(1, 5, 5) == 0 and ws(5, 1, 5) == 0 and ws(5, 5, 1) == 0 and ws(0, 5, 5) == 0 and ws(-3, 5, 5) == 0
    assert ws(2048, 1024, 1024) == 0 and ws(2047, 1024, 1024) > 0            # 2^31 nodes are refused, fewer are not
    # code bytes + two int32 sums per 256-node run + an int32 base per node
    assert ws(70, 65, 67) >= 70 * 65 * 67 * 5 + 2 * 4 * ((70 * 65 * 67 + 255) // 256)
    one = C.c_void_p(256)            # never dereferenced: every call below is refused before any HIP call
    f3 = C.c_float * 3
    org, sp = f3(0, 0, 0), f3(1, 1, 1)
    bad = -1                         # T2N_ERR_INVALID
    assert lib.t2n_mc_count(None, 4, 4, 4, 0.0, one, one, None) == bad
    assert b"t2n_mc_count" in lib.t2n_last_error()
    assert lib.t2n_mc_count(one, 4, 4, 4, 0.0, None, one, None) == bad
    assert lib.t2n_mc_count(one, 4, 4, 4, 0.0, one, None, None) == bad
    assert lib.t2n_mc_count(one, 1, 4, 4, 0.0, one, one, None) == bad
    assert lib.t2n_mc_count(one, 4, 4, 1, 0.0, one, one, None) == bad
    assert lib.t2n_mc_count(one, 2048, 1024, 1024, 0.0, one, one, None) == bad

    def emit(volume=one, dims=(4, 4, 4), workspace=one, origin=org, spacing=sp, verts=one, faces=one):
        return lib.t2n_mc_emit(volume, dims[0], dims[1], dims[2], 0.0, workspace, origin, spacing, 0, verts, None, faces, None)
    assert emit(volume=None) == bad and b"t2n_mc_emit" in lib.t2n_last_error()
    assert emit(workspace=None) == bad and emit(origin=None) == bad and emit(spacing=None) == bad
    assert emit(verts=None) == bad and emit(faces=None) == bad
    assert emit(dims=(4, 1, 4)) == bad and emit(dims=(2048, 1024, 1024)) == bad
    for s in (0.0, -1.0, float("inf"), float("nan")):
        for k in range(3):
            v = [1.0, 1.0, 1.0]
            v[k] = s
            assert emit(spacing=f3(*v)) == bad, (s, k)


def test_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.T2NError):
        mesh.marching_cubes(R.ellipsoid_volume(), 0.0)
    with pytest.raises(ValueError):
        mesh.marching_cubes(np.zeros((4, 4), np.float32), 0.0)
