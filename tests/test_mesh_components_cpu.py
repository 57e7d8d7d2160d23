"""Mesh components without a GPU: the host reference the GPU tests compare with (tests/helpers/cc_ref.py) on hand-made graphs, the
public names and signatures, the library's argument checks and the no-CPU-fallback error."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

from tests.helpers import cc_ref as CC
from tests.helpers import mc_ref as R
from text2nerf_amd import _lib, mesh


# ---- the reference helper on hand-made graphs -----------------------------------------------------------------------------------------
def test_chain_is_one_component():
    faces = np.array([[k, k + 1, k + 2] for k in range(0, 20, 2)], np.int32)          # consecutive faces share one vertex
    labels, K, vc, fc = CC.components(faces, 21)
    assert K == 1 and labels.dtype == np.int32 and not labels.any() and vc.tolist() == [21] and fc.tolist() == [10]
    labels, K, vc, fc = CC.components(faces[::-1], 21)                                # the order of the faces does not matter
    assert K == 1 and not labels.any()


def test_two_triangles_sharing_one_vertex_are_connected():
    labels, K, vc, fc = CC.components([[0, 1, 2], [2, 3, 4]], 5)
    assert K == 1 and vc.tolist() == [5] and fc.tolist() == [2]
    labels, K, vc, fc = CC.components([[0, 1, 2], [3, 4, 5]], 6)
    assert K == 2 and labels.tolist() == [0, 0, 0, 1, 1, 1] and fc.tolist() == [1, 1]


def test_isolated_vertices_are_components_with_no_faces():
    labels, K, vc, fc = CC.components([[0, 1, 3]], 6)
    assert K == 4 and labels.tolist() == [0, 0, 1, 0, 2, 3] and vc.tolist() == [3, 1, 1, 1] and fc.tolist() == [1, 0, 0, 0]
    labels, K, vc, fc = CC.components(np.zeros((0, 3), np.int32), 5)
    assert K == 5 and labels.tolist() == [0, 1, 2, 3, 4] and vc.tolist() == [1] * 5 and fc.tolist() == [0] * 5
    labels, K, vc, fc = CC.components(np.zeros((0, 3), np.int32), 0)
    assert K == 0 and labels.shape == (0,) and vc.shape == (0,) and fc.shape == (0,)


def test_labels_are_numbered_by_smallest_vertex_index():
    # components {0, 9, 5}, {1, 8, 2}, {3, 4, 7}, {6}: given in an order scipy would number differently
    faces = np.array([[3, 4, 7], [8, 1, 2], [9, 0, 5]], np.int32)
    labels, K, vc, fc = CC.components(faces, 10)
    assert K == 4 and labels.tolist() == [0, 1, 1, 2, 2, 0, 3, 2, 1, 0]
    assert vc.tolist() == [3, 3, 3, 1] and fc.tolist() == [1, 1, 1, 0]
    # the component that contains vertex 0 is 0 whatever else there is
    rng = np.random.default_rng(4)
    f = rng.integers(0, 60, (25, 3)).astype(np.int32)
    labels, K, _, _ = CC.components(f, 60)
    first = [int(np.nonzero(labels == c)[0][0]) for c in range(K)]
    assert labels[0] == 0 and first == sorted(first) and sorted(set(labels.tolist())) == list(range(K))


def test_keep_rule_and_tie_order():
    fc = np.array([5, 9, 2, 9, 5, 0], np.int32)
    assert CC.keep_mask(fc, 0).all()
    assert CC.keep_mask(fc, 5).tolist() == [True, True, False, True, True, False]
    assert CC.keep_mask(fc, 0, 1).tolist() == [False, True, False, False, False, False]        # 9 twice: the lower label
    assert CC.keep_mask(fc, 0, 3).tolist() == [True, True, False, True, False, False]          # 5 twice: the lower label
    assert CC.keep_mask(fc, 6, 3).tolist() == [False, True, False, True, False, False]         # both rules hold at once
    assert CC.keep_mask(fc, 0, 10).all()


def test_filter_keeps_order_and_reindexes():
    verts, faces, normals = R.marching_cubes(CC.blob_volume((0, 1, 2)), 0.0, spacing=CC.BLOB_SPACING, origin=CC.BLOB_ORIGIN)
    labels, K, vc, fc = CC.components(faces, len(verts))
    assert K == 3 and fc.tolist() == [1912, 748, 92] and vc.tolist() == [958, 376, 48]
    colors = np.random.default_rng(6).integers(0, 256, verts.shape).astype(np.uint8)
    for c in range(3):
        keep = np.arange(3) == c
        v, f, n, col = CC.filter_mesh(verts, faces, normals, colors, labels, keep)
        one = R.marching_cubes(CC.blob_volume((c,)), 0.0, spacing=CC.BLOB_SPACING, origin=CC.BLOB_ORIGIN)
        assert np.array_equal(v, one[0]) and np.array_equal(f, one[1]) and np.array_equal(n, one[2])
        assert np.array_equal(col, colors[labels == c]) and R.is_closed_oriented_manifold(f)
    v, f, n, col = CC.filter_mesh(verts, faces, None, None, labels, np.zeros(3, bool))
    assert v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == np.int32 and n is None and col is None


def test_test_volumes_have_the_stated_shape():
    v, f, _ = R.marching_cubes(CC.serpentine_volume((48, 30, 8), (4, 12, 20), 3.7, x0=3, x1=44), 0.0)
    labels, K, vc, fc = CC.components(f, len(v))
    assert (len(v), len(f), K) == (1408, 2812, 1) and R.is_closed_oriented_manifold(f)
    a = CC.serpentine_volume((48, 30, 14), (4, 12, 20), 3.7, x0=3, x1=44)
    b = CC.serpentine_volume((48, 30, 14), (8, 16, 24), 9.7, x0=3, x1=44)
    v, f, _ = R.marching_cubes(np.maximum(a, b), 0.0)
    labels, K, vc, fc = CC.components(f, len(v))
    assert (len(v), len(f), K) == (2816, 5624, 2) and fc.tolist() == [2812, 2812]
    assert int((np.diff(labels) != 0).sum()) == 353
    assert [(int(np.nonzero(labels == c)[0][0]), int(np.nonzero(labels == c)[0][-1])) for c in range(2)] == [(0, 2810), (1, 2815)]


# ---- surface ------------------------------------------------------------------------------------------------------------------------
def test_public_names_and_signatures():
    import text2nerf_amd as T
    assert T.mesh_components is mesh.mesh_components and T.filter_components is mesh.filter_components
    assert T.Components is mesh.Components and mesh.Components._fields == ("labels", "n_components", "vert_counts", "face_counts")
    assert [(p.name, p.default) for p in inspect.signature(mesh.mesh_components).parameters.values()] == [
        ("faces", inspect.Parameter.empty), ("n_verts", inspect.Parameter.empty)]
    assert [(p.name, p.default) for p in inspect.signature(mesh.filter_components).parameters.values()] == [
        ("mesh", inspect.Parameter.empty), ("min_faces", 0), ("keep_largest", None), ("components", None)]


def test_library_argument_checks_run_without_a_gpu():
    lib = _lib.load()
    ws = lib.t2n_mesh_components_workspace_bytes
    assert ws(0, 0) > 0 and ws(5, 0) > 0
    # an int32 per vertex and one per 256-run of vertices and of faces
    assert ws(450938, 934979) >= 4 * (450938 + (450938 + 255) // 256 + (934979 + 255) // 256)
    assert ws(-1, 0) == 0 and ws(3, -1) == 0
    assert ws(2**31, 0) == 0 and ws(2**31 - 1, 0) > 0                        # 2^31 vertices are refused, fewer are not
    assert ws(3, (2**31 + 2) // 3) == 0 and ws(3, (2**31 - 1) // 3) > 0      # 3 F >= 2^31 is refused
    one = C.c_void_p(256)            # never dereferenced: every call below is refused before any HIP call
    bad = -1                         # T2N_ERR_INVALID
    big = ws(10, 20)

    def comps(faces=one, F=20, V=10, labels=one, k=one, workspace=one, nbytes=big):
        return lib.t2n_mesh_components(faces, F, V, labels, k, workspace, nbytes, None)
    assert comps(faces=None) == bad and b"t2n_mesh_components" in lib.t2n_last_error()
    assert comps(labels=None) == bad and comps(k=None) == bad and comps(workspace=None) == bad
    assert comps(F=-1) == bad and comps(V=-1) == bad and comps(V=2**31) == bad and comps(F=(2**31 + 2) // 3) == bad
    assert comps(nbytes=big - 1) == bad and comps(nbytes=0) == bad

    def sizes(faces=one, F=20, labels=one, V=10, K=3, vc=one, fc=one):
        return lib.t2n_mesh_component_sizes(faces, F, labels, V, K, vc, fc, None)
    assert sizes(faces=None) == bad and b"t2n_mesh_component_sizes" in lib.t2n_last_error()
    assert sizes(labels=None) == bad and sizes(vc=None) == bad and sizes(fc=None) == bad
    assert sizes(F=-1) == bad and sizes(V=-1) == bad and sizes(K=-1) == bad and sizes(K=11) == bad and sizes(V=2**31) == bad

    def count(faces=one, F=20, labels=one, V=10, keep=one, K=3, workspace=one, nbytes=big, totals=one):
        return lib.t2n_mesh_filter_count(faces, F, labels, V, keep, K, workspace, nbytes, totals, None)
    assert count(faces=None) == bad and b"t2n_mesh_filter_count" in lib.t2n_last_error()
    assert count(labels=None) == bad and count(keep=None) == bad and count(workspace=None) == bad and count(totals=None) == bad
    assert count(F=-1) == bad and count(V=-1) == bad and count(K=-1) == bad and count(K=11) == bad and count(nbytes=big - 1) == bad
    assert count(F=(2**31 + 2) // 3) == bad

    def emit(faces=one, F=20, labels=one, V=10, keep=one, K=3, verts=one, normals=None, colors=None, workspace=one, nbytes=big,
             verts_out=one, normals_out=None, colors_out=None, faces_out=one):
        return lib.t2n_mesh_filter_emit(faces, F, labels, V, keep, K, verts, normals, colors, workspace, nbytes, verts_out, normals_out,
                                        colors_out, faces_out, None)
    assert emit(faces=None) == bad and b"t2n_mesh_filter_emit" in lib.t2n_last_error()
    assert emit(labels=None) == bad and emit(keep=None) == bad and emit(verts=None) == bad and emit(workspace=None) == bad
    assert emit(verts_out=None) == bad and emit(faces_out=None) == bad
    assert emit(normals=one) == bad and emit(normals_out=one) == bad           # normals and colours: in and out together
    assert emit(colors=one) == bad and emit(colors_out=one) == bad
    assert emit(V=-1) == bad and emit(F=-1) == bad and emit(K=11) == bad and emit(nbytes=big - 1) == bad and emit(V=2**31) == bad


def test_python_argument_checks_and_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    faces = np.array([[0, 1, 2], [2, 3, 4]], np.int32)
    verts = np.zeros((5, 3), np.float32)
    with pytest.raises(_lib.T2NError):
        mesh.mesh_components(faces, 5)
    with pytest.raises(_lib.T2NError):
        mesh.mesh_components(torch.from_numpy(faces), 5)
    with pytest.raises(_lib.T2NError):
        mesh.filter_components((verts, faces), min_faces=1)
    with pytest.raises(_lib.T2NError):
        mesh.filter_components(mesh.Mesh(verts, faces, None, None), keep_largest=1)
    # what is wrong with the arguments themselves is a ValueError before the device is asked for
    for bad in (faces.astype(np.float32), faces.reshape(-1), faces[:, :2], faces.astype(bool)):
        with pytest.raises(ValueError):
            mesh.mesh_components(bad, 5)
        with pytest.raises(ValueError):
            mesh.filter_components((verts, bad))
    with pytest.raises(ValueError):
        mesh.mesh_components(faces, -1)
    with pytest.raises(ValueError):
        mesh.filter_components((verts, faces), min_faces=-1)
    with pytest.raises(ValueError):
        mesh.filter_components((verts, faces), keep_largest=0)
    with pytest.raises(ValueError):
        mesh.filter_components((verts.reshape(-1), faces))
    with pytest.raises(ValueError):
        mesh.filter_components((verts,))
