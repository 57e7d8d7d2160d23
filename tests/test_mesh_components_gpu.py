"""Device connected components and floater removal (csrc/t2n_mesh.hip through text2nerf_amd.mesh.mesh_components / filter_components)
against the host reference tests/helpers/cc_ref.py (scipy's connected_components, renumbered canonically; checked on hand-made graphs
by tests/test_mesh_components_cpu.py). Everything is integer or a moved row: every comparison is exact array equality. The meshes come
from mesh.marching_cubes on the device; the vertex / face / component numbers in the asserts are those of the numpy restatement
(tests/helpers/mc_ref.py) on the same volumes. Shapes from the kernels' constants: a workgroup owns 256 vertices or faces, the scan of
the workgroup sums takes 1024 of them a step."""
import numpy as np
import pytest
import torch

from tests.helpers import cc_ref as CC
from tests.helpers import mc_ref as R
from tests.test_hip_parity import dev, make_field
from tests.conftest import TINY
from text2nerf_amd import filter_components, mesh, mesh_components, synth

pytestmark = pytest.mark.gpu

RUN, CHUNK = 256, 1024


def device_mesh(vol, level=0.0, **kw):
    v, f, n = mesh.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol)).to(dev()), level, **kw)
    return mesh.Mesh(v, f, n, None)


def host(x):
    return None if x is None else x.cpu().numpy()


def check_components(m, name=""):
    """mesh_components on the device against the reference: labels, K and both count arrays exactly. Returns (device result, reference)."""
    V = m.verts.shape[0]
    got = mesh_components(m.faces, V)
    assert isinstance(got, mesh.Components) and isinstance(got.n_components, int)
    for t in (got.labels, got.vert_counts, got.face_counts):
        assert t.is_cuda and t.dtype == torch.int32
    want = CC.components(host(m.faces), V)
    if name:
        print(f"{name}: V {V} F {m.faces.shape[0]} K {got.n_components} (reference {want[1]}); largest {sorted(want[3].tolist())[-3:]}")
    assert got.n_components == want[1], name
    assert np.array_equal(host(got.labels), want[0]), name
    assert np.array_equal(host(got.vert_counts), want[2]) and np.array_equal(host(got.face_counts), want[3]), name
    return got, want


def check_filter(m, want, name="", closed=True, **kw):
    """filter_components on the device against the reference filter with the reference keep rule; returns the device Mesh. `closed`:
    the input is a closed oriented 2-manifold (its surface does not reach the border of the volume), so the output must be one."""
    labels, K, vc, fc = want
    keep = CC.keep_mask(fc, kw.get("min_faces", 0), kw.get("keep_largest"))
    ref = CC.filter_mesh(host(m.verts), host(m.faces), host(m.normals), host(m.colors), labels, keep)
    out = filter_components(m, **kw)
    assert isinstance(out, mesh.Mesh) and out.verts.is_cuda and out.faces.dtype == torch.int32 and out.verts.dtype == torch.float32
    if name:
        print(f"{name} {kw}: keeps {int(keep.sum())} of {K} components, V {out.verts.shape[0]} F {out.faces.shape[0]}")
    for a, b in zip(out, ref):
        assert (a is None) == (b is None), name
        if b is not None:
            assert tuple(a.shape) == b.shape and np.array_equal(host(a), b), (name, kw)
    if closed:
        assert R.is_closed_oriented_manifold(host(out.faces)), name
    return out


# ---- noise, many components ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def noise():
    m = device_mesh(R.noise_volume())
    return m, check_components(m, "noise")


def test_noise_labels_and_counts(noise):
    m, (got, want) = noise
    assert (m.verts.shape[0], m.faces.shape[0], got.n_components) == (2824, 5788, 29)
    assert sorted(want[3].tolist(), reverse=True)[:8] == [5172, 180, 116, 32, 24, 24, 16, 16]
    assert int(got.vert_counts.sum()) == 2824 and int(got.face_counts.sum()) == 5788 and int(got.labels[0]) == 0


@pytest.mark.parametrize("kw,kept", [(dict(min_faces=9), (13, 2728, 5660)), (dict(min_faces=50), (3, 2612, 5468)),
                                     (dict(keep_largest=5), (5, None, None)), (dict(min_faces=20, keep_largest=4), (4, None, None)),
                                     (dict(), (29, 2824, 5788)), (dict(min_faces=10**6), (0, 0, 0))])
def test_noise_filters(noise, kw, kept):
    m, (got, want) = noise
    out = check_filter(m, want, "noise", **kw)
    keep = CC.keep_mask(want[3], kw.get("min_faces", 0), kw.get("keep_largest"))
    assert int(keep.sum()) == kept[0]
    if kept[1] is not None:
        assert (out.verts.shape[0], out.faces.shape[0]) == kept[1:]
    again = mesh_components(out.faces, out.verts.shape[0])
    assert again.n_components == kept[0]
    assert np.array_equal(host(again.face_counts), want[3][keep])            # the kept components, in their order
    reuse = filter_components(m, components=got, **kw)                       # an earlier result reused: the same arrays
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(out, reuse))


def test_noise_keep_largest_tie_goes_to_the_lower_label(noise):
    m, (got, want) = noise
    fc = want[3]
    assert fc[18] == 24 and fc[20] == 24
    keep = np.zeros(29, bool)
    keep[[0, 5, 9, 18, 21]] = True
    assert np.array_equal(CC.keep_mask(fc, 0, 5), keep)
    out = filter_components(m, keep_largest=5)
    ref = CC.filter_mesh(host(m.verts), host(m.faces), host(m.normals), None, want[0], keep)
    assert np.array_equal(host(out.verts), ref[0]) and np.array_equal(host(out.faces), ref[1]) and np.array_equal(host(out.normals), ref[2])
    wrong = keep.copy()
    wrong[[18, 20]] = [False, True]
    assert not np.array_equal(host(out.verts), CC.filter_mesh(host(m.verts), host(m.faces), None, None, want[0], wrong)[0])


# ---- three blobs: compaction order and re-indexing are the emitter's own ----------------------------------------------------------------
def test_three_blobs_filtered_equal_the_blobs_alone():
    kw = dict(spacing=CC.BLOB_SPACING, origin=CC.BLOB_ORIGIN)
    full = device_mesh(CC.blob_volume((0, 1, 2)), **kw)
    got, want = check_components(full, "blobs")
    assert got.n_components == 3 and host(got.face_counts).tolist() == [1912, 748, 92] and host(got.vert_counts).tolist() == [958, 376, 48]
    alone = [device_mesh(CC.blob_volume((i,)), **kw) for i in range(3)]
    one = filter_components(full, keep_largest=1)
    assert torch.equal(one.verts, alone[0].verts) and torch.equal(one.normals, alone[0].normals) and torch.equal(one.faces, alone[0].faces)
    assert one.colors is None
    # only label 1: an earlier result reused, with the other two counts put to 0
    only = got._replace(face_counts=got.face_counts * torch.tensor([0, 1, 0], dtype=torch.int32, device=got.labels.device))
    second = filter_components(full, min_faces=1, components=only)
    assert torch.equal(second.verts, alone[1].verts) and torch.equal(second.normals, alone[1].normals)
    assert torch.equal(second.faces, alone[1].faces)
    third = filter_components(full, min_faces=1, components=only._replace(face_counts=got.face_counts * (got.face_counts < 100)))
    assert torch.equal(third.verts, alone[2].verts) and torch.equal(third.normals, alone[2].normals)
    assert torch.equal(third.faces, alone[2].faces)


# ---- long chains, interleaved components ------------------------------------------------------------------------------------------------
def test_serpentine_tube_is_one_component():
    m = device_mesh(CC.serpentine_volume((48, 30, 8), (4, 12, 20), 3.7, x0=3, x1=44))
    got, want = check_components(m, "serpentine")
    assert (m.verts.shape[0], m.faces.shape[0], got.n_components) == (1408, 2812, 1)
    assert not bool(got.labels.any()) and host(got.face_counts).tolist() == [2812] and host(got.vert_counts).tolist() == [1408]
    out = check_filter(m, want, "serpentine", keep_largest=1)
    assert torch.equal(out.verts, m.verts) and torch.equal(out.faces, m.faces)


def test_two_interleaved_tubes_with_equal_face_counts():
    a = CC.serpentine_volume((48, 30, 14), (4, 12, 20), 3.7, x0=3, x1=44)
    b = CC.serpentine_volume((48, 30, 14), (8, 16, 24), 9.7, x0=3, x1=44)
    m = device_mesh(np.maximum(a, b))
    got, want = check_components(m, "two tubes")
    assert (m.verts.shape[0], m.faces.shape[0], got.n_components) == (2816, 5624, 2) and host(got.face_counts).tolist() == [2812, 2812]
    labels = host(got.labels)
    assert int((np.diff(labels) != 0).sum()) == 353
    assert [(int(np.nonzero(labels == c)[0][0]), int(np.nonzero(labels == c)[0][-1])) for c in range(2)] == [(0, 2810), (1, 2815)]
    out = check_filter(m, want, "two tubes", keep_largest=1)                   # the tie goes to label 0; 353 gaps to close
    assert out.verts.shape[0] == 1408 and out.faces.shape[0] == 2812
    assert np.array_equal(host(out.verts), host(m.verts)[labels == 0])
    check_filter(m, want, "two tubes", min_faces=2812)                         # both stay
    check_filter(m, want, "two tubes", min_faces=2813)                         # neither


# ---- more than one scan chunk, one dominant component -----------------------------------------------------------------------------------
def test_multi_chunk_one_dominant_component():
    vol = np.random.default_rng(1).standard_normal((70, 65, 67)).astype(np.float32)
    v, f, n = mesh.marching_cubes(torch.from_numpy(vol).to(dev()), 0.0, normals=False)
    m = mesh.Mesh(v, f, None, None)
    assert (v.shape[0], f.shape[0]) == (450938, 934979) and -(-v.shape[0] // RUN) == 1762 > CHUNK and -(-f.shape[0] // RUN) > CHUNK
    got, want = check_components(m, "70x65x67")
    fc = want[3]
    assert got.n_components == 2946 and int(fc[0]) == 908613 and sorted(fc.tolist())[-2] == 94
    out = check_filter(m, want, "70x65x67", closed=False, min_faces=100)    # unpadded noise: the surface is cut by the border
    assert out.faces.shape[0] == 908613 and out.normals is None
    again = mesh_components(out.faces, out.verts.shape[0])
    assert again.n_components == 1 and int(again.face_counts[0]) == 908613 and int(again.vert_counts[0]) == out.verts.shape[0]


# ---- edge cases -------------------------------------------------------------------------------------------------------------------------
def test_empty_surface():
    m = device_mesh(R.ellipsoid_volume(), 100.0)
    assert m.verts.shape[0] == 0
    got = mesh_components(m.faces, 0)
    assert got.n_components == 0 and tuple(got.labels.shape) == (0,) and tuple(got.vert_counts.shape) == (0,)
    assert tuple(got.face_counts.shape) == (0,) and got.labels.is_cuda and got.labels.dtype == torch.int32
    out = filter_components(m, keep_largest=1)
    assert tuple(out.verts.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3) and tuple(out.normals.shape) == (0, 3)
    assert out.colors is None and out.verts.is_cuda


def test_vertices_without_faces():
    faces = torch.empty(0, 3, dtype=torch.int32, device=dev())
    got = mesh_components(faces, 5)
    assert got.n_components == 5 and host(got.labels).tolist() == [0, 1, 2, 3, 4]
    assert host(got.vert_counts).tolist() == [1] * 5 and host(got.face_counts).tolist() == [0] * 5
    verts = torch.arange(15, dtype=torch.float32, device=dev()).reshape(5, 3)
    out = filter_components((verts, faces), min_faces=1)
    assert tuple(out.verts.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3) and out.normals is None and out.colors is None
    out = filter_components((verts, faces))                                    # min_faces=0 keeps the five lone vertices
    assert torch.equal(out.verts, verts) and tuple(out.faces.shape) == (0, 3)
    # an isolated vertex between two triangles, a hand-made list that marching cubes would never emit, int64 indices
    f = torch.tensor([[5, 6, 4], [0, 2, 1]], dtype=torch.int64, device=dev())
    got = mesh_components(f, 7)
    assert got.n_components == 3 and host(got.labels).tolist() == [0, 0, 0, 1, 2, 2, 2]
    assert host(got.vert_counts).tolist() == [3, 1, 3] and host(got.face_counts).tolist() == [1, 0, 1]


def test_out_of_range_index_is_refused_before_any_launch():
    m = device_mesh(R.ellipsoid_volume())
    V = m.verts.shape[0]
    bad = m.faces.clone()
    bad[7, 1] = V
    with pytest.raises(ValueError):
        mesh_components(bad, V)
    with pytest.raises(ValueError):
        filter_components((m.verts, bad), keep_largest=1)
    bad[7, 1] = -1
    with pytest.raises(ValueError):
        mesh_components(bad, V)
    with pytest.raises(ValueError):
        mesh_components(m.faces, V - 1)
    with pytest.raises(ValueError):
        mesh_components(m.faces.float(), V)
    with pytest.raises(ValueError):
        filter_components(m, min_faces=-1)
    with pytest.raises(ValueError):
        filter_components(m, keep_largest=0)
    with pytest.raises(ValueError):
        filter_components((m.verts, m.faces, m.normals[:-1]))


def test_numpy_in_numpy_out_colours_and_repeatability(noise):
    m, (got, want) = noise
    colors = torch.from_numpy(np.random.default_rng(8).integers(0, 256, tuple(m.verts.shape)).astype(np.uint8)).to(dev())
    full = mesh.Mesh(m.verts, m.faces, m.normals, colors)
    out = check_filter(full, want, "noise + colours", min_faces=9)             # the uint8 rows move with their vertices
    assert out.colors.dtype == torch.uint8 and out.colors.shape == out.verts.shape
    bare = check_filter(mesh.Mesh(m.verts, m.faces, None, None), want, "noise bare", min_faces=9)
    assert bare.normals is None and bare.colors is None and torch.equal(bare.verts, out.verts) and torch.equal(bare.faces, out.faces)
    only_c = filter_components(mesh.Mesh(m.verts, m.faces, None, colors), min_faces=9)
    assert only_c.normals is None and torch.equal(only_c.colors, out.colors)
    # two calls: bit-equal
    again = mesh_components(m.faces, m.verts.shape[0])
    assert again.n_components == got.n_components and all(torch.equal(a, b) for a, b in zip(
        (again.labels, again.vert_counts, again.face_counts), (got.labels, got.vert_counts, got.face_counts)))
    out2 = filter_components(full, min_faces=9)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))
    # numpy (and CPU tensors) in, numpy out, the same arrays; a tuple without normals and colours
    c_np = mesh_components(host(m.faces), m.verts.shape[0])
    assert isinstance(c_np.labels, np.ndarray) and isinstance(c_np.vert_counts, np.ndarray) and isinstance(c_np.face_counts, np.ndarray)
    assert np.array_equal(c_np.labels, want[0]) and c_np.n_components == want[1] and np.array_equal(c_np.face_counts, want[3])
    o_np = filter_components((host(m.verts), host(m.faces), host(m.normals), host(colors)), min_faces=9, components=c_np)
    assert all(isinstance(a, np.ndarray) and np.array_equal(a, host(b)) for a, b in zip(o_np, out))
    o_cpu = filter_components((m.verts.cpu(), m.faces.cpu().long()), min_faces=9)
    assert isinstance(o_cpu.verts, np.ndarray) and o_cpu.normals is None and o_cpu.colors is None
    assert np.array_equal(o_cpu.verts, host(out.verts)) and np.array_equal(o_cpu.faces, host(out.faces))


# ---- through the field --------------------------------------------------------------------------------------------------------------
def open_edges(faces):
    """The directed edges of an oriented mesh that have no opposite, as a sorted [n,2] array; asserts that no directed edge occurs twice
    (the mesh is an oriented manifold, closed iff the result is empty)."""
    f = np.asarray(faces, dtype=np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    n = int(f.max()) + 1 if len(f) else 1
    key, rev = d[:, 0] * n + d[:, 1], d[:, 1] * n + d[:, 0]
    assert len(np.unique(key)) == len(key)
    lone = np.sort(key[~np.isin(key, rev)])
    return np.stack([lone // n, lone % n], -1)


def test_export_mesh_then_keep_the_largest_component():
    """The tuned-shape fixture of tests/test_mesh_gpu.py, filter_components(export_mesh(None, level, gridSize), keep_largest=1): one
    component, colours (and positions, normals) equal to the matching rows of the unfiltered mesh, faces equal to the reference filter.
    Closedness: the fixture's random field is cut by its box at every level (33 x 29 x 25 nodes: alpha reaches 0.9964 on the border and
    0.9613 inside, and the mesh at the median level is open BEFORE filtering), so no filter can return a closed mesh here. What leaving
    out whole components guarantees is asserted instead: the result is an oriented manifold whose open edges are exactly the kept
    component's open edges of the input, so it is closed iff that component was (the closed inputs are the other tests of this file)."""
    params = synth.make_field_params(11, TINY["grid"], density_scale=0.9, aabb=TINY["aabb"])
    field = make_field(params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    g = [33, 29, 25]
    alpha = field.getDenseAlpha(g)[0]
    level = float(alpha.median())
    full = field.export_mesh(None, level=level, gridSize=g)
    comp, want = check_components(full, "export")
    out = filter_components(full, keep_largest=1)
    big = int(np.argmax(want[3]))                                              # argmax: the first of equal counts, the lower label
    after = mesh_components(out.faces, out.verts.shape[0])
    assert after.n_components == 1 and int(after.face_counts[0]) == int(want[3][big]) and out.faces.shape[0] > 100
    rows = torch.from_numpy(want[0] == big).to(dev())
    assert out.colors.dtype == torch.uint8 and torch.equal(out.colors, full.colors[rows])
    assert torch.equal(out.verts, full.verts[rows]) and torch.equal(out.normals, full.normals[rows])
    ref = CC.filter_mesh(host(full.verts), host(full.faces), None, None, want[0], np.arange(want[1]) == big)
    assert np.array_equal(host(out.faces), ref[1])
    f_in = host(full.faces)
    newidx = np.cumsum(want[0] == big) - 1
    want_open = open_edges(newidx[f_in[want[0][f_in[:, 0]] == big]])
    got_open = open_edges(host(out.faces))
    print(f"export: level {level:.6g}, K {want[1]}, keep_largest=1 keeps {out.faces.shape[0]} of {f_in.shape[0]} faces; open edges "
          f"{len(got_open)} (the kept component's in the input: {len(want_open)}; the whole input: {len(open_edges(f_in))})")
    assert np.array_equal(got_open, want_open)
    assert R.is_closed_oriented_manifold(host(out.faces)) == (len(want_open) == 0)
