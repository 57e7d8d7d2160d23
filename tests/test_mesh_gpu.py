"""Device marching cubes (csrc/t2n_mesh.hip through text2nerf_amd.mesh) against the numpy restatement tests/helpers/mc_ref.py (itself
checked by tests/test_mesh_cpu.py): counts, faces and vertex order exactly; positions within 4 * 2^-23 * max |coordinate| (four
correctly rounded fp32 operations on the same inputs; bit-equality is expected and printed); normals within 1e-6 absolute (unit
vectors, a dozen roundings of 6e-8). Shapes: the smallest at which each stage can go wrong, from the kernels' constants: a workgroup
owns kMcRun = 256 nodes, the scan of the workgroup sums takes kMcScanChunk = 1024 of them a step."""
import numpy as np
import pytest
import torch

from tests.helpers import mc_ref as R
from tests.test_hip_parity import dev, make_field
from tests.conftest import TINY
from text2nerf_amd import mesh, synth
from text2nerf_amd._lib import T2NError

pytestmark = pytest.mark.gpu

RUN, CHUNK = 256, 1024          # kMcRun, kMcScanChunk
EPS = 2.0**-23
LAST = {}


def check(vol, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), name="", **kw):
    """marching_cubes on the device (device tensor in) against the restatement; returns the device mesh as numpy arrays."""
    want_v, want_f, want_n = R.marching_cubes(vol, level, spacing=spacing, origin=origin, **kw)
    v, f, n = mesh.marching_cubes(torch.from_numpy(np.ascontiguousarray(vol)).to(dev()), level, spacing=spacing, origin=origin, **kw)
    assert v.is_cuda and f.is_cuda and v.dtype == torch.float32 and f.dtype == torch.int32
    v, f = v.cpu().numpy(), f.cpu().numpy()
    assert v.shape == want_v.shape and f.shape == want_f.shape, (name, v.shape, want_v.shape, f.shape, want_f.shape)
    assert np.array_equal(f, want_f), name
    tol = 4 * EPS * float(np.abs(want_v).max()) if len(want_v) else 0.0
    err = float(np.abs(v - want_v).max()) if len(want_v) else 0.0
    bit = LAST["bit"] = np.array_equal(v, want_v)
    nerr = 0.0
    if want_n is None:
        assert n is None
    else:
        n = n.cpu().numpy()
        assert n.shape == want_n.shape and np.isfinite(n).all()
        nerr = float(np.abs(n - want_n).max()) if len(want_n) else 0.0
    if name:
        print(f"{name}: V {len(v)} F {len(f)} position error {err:.3g} (bound {tol:.3g}, bit-equal {bit}) normal error {nerr:.3g}")
    assert np.isfinite(v).all() and err <= tol, (name, err, tol)
    assert nerr <= 1e-6, (name, nerr)
    return v, f, n


def test_all_256_single_cell_volumes():
    bits = 0
    for case in range(256):
        v, f, n = check(R.single_cell(case), 0.0, spacing=(0.5, 1.25, 2.0), origin=(-1.0, 0.5, 3.0))
        assert len(f) == R.NTRI[case]
        bits += LAST["bit"]
    print("single cells: positions bit-equal in", bits, "of 256 cases")


@pytest.mark.parametrize("shape", [(3, 5, 67), (17, 9, 70), (2, 31, 19), (9, 2, 2)])
def test_shapes_off_the_workgroup_run(shape):
    assert all(s % RUN for s in shape) and np.prod(shape) % RUN
    vol = np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)
    v, f, _ = check(vol, 0.1, spacing=(0.3, 0.7, 1.1), origin=(-2.0, 1.0, 0.5), name=str(shape))
    assert len(v) > 0


def test_multi_chunk_scan():
    """70 x 65 x 67 nodes = 1191 workgroups of 256 nodes: more than one 1024-entry chunk of the block-sum scan. Crossings in the first
    workgroup, in the last, and on both sides of the chunk boundary."""
    shape = (70, 65, 67)
    nb = -(-int(np.prod(shape)) // RUN)
    assert nb > CHUNK
    vol = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    inside = (vol > 0).ravel()
    crossed = np.zeros(inside.size, bool)
    crossed[:-1] = (inside[:-1] != inside[1:]) & ((np.arange(inside.size - 1) % shape[2]) != shape[2] - 1)
    per_block = np.add.reduceat(crossed.astype(np.int64), np.arange(0, crossed.size, RUN))
    assert per_block[0] and per_block[-1] and per_block[CHUNK - 1] and per_block[CHUNK]
    v, f, _ = check(vol, 0.0, name="70x65x67")
    assert len(v) > 400000


def test_padded_noise_every_case_dense_output():
    v, f, n = check(R.noise_volume(), 0.0, name="noise")
    assert R.is_closed_oriented_manifold(f)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6


def test_plateau_level_is_an_attained_value():
    vol = np.pad(np.random.default_rng(2).integers(0, 3, (9, 10, 11)).astype(np.float32), 1, constant_values=0.0)
    assert (vol == 1.0).sum() > 100
    v, f, _ = check(vol, 1.0, name="plateau")           # inside = strictly greater: the 1-valued nodes are outside
    assert R.is_closed_oriented_manifold(f)
    inside = vol > 1.0
    assert len(v) == sum(int((np.diff(inside.astype(np.int8), axis=a) != 0).sum()) for a in range(3))


def test_nonfinite_volume():
    v, f, n = check(R.nonfinite_volume(), 0.0, name="nonfinite")
    assert np.isfinite(v).all() and np.isfinite(n).all() and R.is_closed_oriented_manifold(f)


def test_ellipsoid_and_torus_properties_on_the_device_mesh():
    v, f, _ = check(R.ellipsoid_volume(), 0.0, name="ellipsoid")
    assert R.is_closed_oriented_manifold(f) and R.euler_characteristic(len(v), f) == 2
    exact = 4.0 / 3.0 * np.pi * 6 * 5 * 7.5
    assert abs(R.signed_volume(v, f) - exact) <= 0.03 * exact
    v, f, _ = check(R.torus_volume(), 0.0, name="torus")
    assert R.is_closed_oriented_manifold(f) and R.euler_characteristic(len(v), f) == 0


@pytest.mark.parametrize("level", [-100.0, 100.0])
def test_empty_surface(level):
    vol = torch.from_numpy(R.ellipsoid_volume()).to(dev())
    v, f, n = mesh.marching_cubes(vol, level)
    assert tuple(v.shape) == (0, 3) and tuple(f.shape) == (0, 3) and tuple(n.shape) == (0, 3)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda
    v, f, n = mesh.marching_cubes(R.ellipsoid_volume(), level, normals=False)
    assert isinstance(v, np.ndarray) and v.shape == (0, 3) and f.shape == (0, 3) and f.dtype == np.int32 and n is None


def test_flip_normals_off_conversions_and_repeatability():
    vol = R.noise_volume()
    kw = dict(spacing=(0.25, 0.5, 1.5), origin=(3.0, -1.0, 0.25))
    d = torch.from_numpy(vol).to(dev())
    v0, f0, n0 = mesh.marching_cubes(d, 0.0, **kw)
    v1, f1, n1 = mesh.marching_cubes(d, 0.0, **kw)
    assert torch.equal(v0, v1) and torch.equal(f0, f1) and torch.equal(n0, n1)                      # two calls: bit-equal
    vf, ff, nf = mesh.marching_cubes(d, 0.0, flip=True, **kw)
    assert torch.equal(ff, f0[:, [0, 2, 1]]) and torch.equal(vf, v0) and torch.equal(nf, n0)        # flip: the faces' last two, nothing else
    vn, fn, nn = mesh.marching_cubes(d, 0.0, normals=False, **kw)
    assert nn is None and torch.equal(vn, v0) and torch.equal(fn, f0)
    # a float64 numpy volume comes back as numpy; a permuted device view as device tensors: the same mesh as the contiguous fp32 form
    v64, f64, n64 = mesh.marching_cubes(vol.astype(np.float64), 0.0, **kw)
    assert isinstance(v64, np.ndarray) and isinstance(f64, np.ndarray) and isinstance(n64, np.ndarray)
    assert np.array_equal(v64, v0.cpu().numpy()) and np.array_equal(f64, f0.cpu().numpy()) and np.array_equal(n64, n0.cpu().numpy())
    perm = torch.from_numpy(np.ascontiguousarray(vol.transpose(2, 0, 1))).to(dev()).permute(1, 2, 0)
    assert not perm.is_contiguous() and tuple(perm.shape) == vol.shape
    vp, fp, np_ = mesh.marching_cubes(perm, 0.0, **kw)
    assert vp.is_cuda and torch.equal(vp, v0) and torch.equal(fp, f0) and torch.equal(np_, n0)
    vc, fc, nc = mesh.marching_cubes(torch.from_numpy(vol).half().float(), 0.0, **kw)               # a CPU tensor: numpy out
    assert isinstance(vc, np.ndarray)
    vh, fh, nh = mesh.marching_cubes(torch.from_numpy(vol).half().to(dev()), 0.0, **kw)             # a half volume is converted once
    assert np.array_equal(vh.cpu().numpy(), vc) and np.array_equal(fh.cpu().numpy(), fc)
    with pytest.raises(ValueError):
        mesh.marching_cubes(d, 0.0, spacing=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        mesh.marching_cubes(d[:1], 0.0)


# ---- export_mesh ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def field():
    params = synth.make_field_params(11, TINY["grid"], density_scale=0.9, aabb=TINY["aabb"])
    return make_field(params, TINY["grid"], TINY["aabb"], TINY["near_far"])


def test_export_mesh_on_a_tuned_shape_field(field, tmp_path):
    g = TINY["grid"]                                                    # 24 x 20 x 16
    alpha = field.getDenseAlpha()[0]
    assert tuple(alpha.shape) == tuple(g)
    level = float(alpha.median())                                       # a level the synthetic density certainly crosses
    print("alpha range", float(alpha.min()), float(alpha.max()), "level", level)
    path = str(tmp_path / "scene.ply")
    out = field.export_mesh(path, level=level)
    assert isinstance(out, mesh.Mesh) and out.verts.shape[0] > 100 and out.faces.shape[0] > 100
    aabb = field.aabb.detach().float().cpu()
    spacing = ((aabb[1] - aabb[0]) / (torch.tensor(g, dtype=torch.float32) - 1)).tolist()
    v, f, n = mesh.marching_cubes(alpha, level, spacing=spacing, origin=aabb[0].tolist())
    assert torch.equal(out.verts, v) and torch.equal(out.faces, f) and torch.equal(out.normals, n)
    # against the restatement on the same volume, like every other mesh here
    check(alpha.cpu().numpy(), level, spacing=spacing, origin=aabb[0].tolist(), name="export")
    # colours = shade at the vertices
    rgb = field.shade(field.normalize_coord(v), viewdirs=-n)[1]
    want = (rgb.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8)
    assert out.colors.dtype == torch.uint8 and torch.equal(out.colors, want) and int(want.max()) > int(want.min())
    # the nodes span the box: every vertex lies inside it (a rounding of the last node's position allowed)
    lo, hi = aabb[0].numpy(), aabb[1].numpy()
    vv = v.cpu().numpy()
    slack = 4 * EPS * float(np.abs(np.stack([lo, hi])).max())
    assert (vv >= lo - slack).all() and (vv <= hi + slack).all()
    # the file round-trips
    header, props, faces = R.read_ply(path)
    assert np.array_equal(np.stack([props["x"], props["y"], props["z"]], -1), vv) and np.array_equal(faces, f.cpu().numpy())
    assert np.array_equal(np.stack([props["nx"], props["ny"], props["nz"]], -1), n.cpu().numpy())
    assert np.array_equal(np.stack([props["red"], props["green"], props["blue"]], -1), want.cpu().numpy())
    # colours without normals in the record; neither; another grid
    bare = field.export_mesh(level=level, colors=False, normals=False)
    assert bare.normals is None and bare.colors is None and torch.equal(bare.verts, v) and torch.equal(bare.faces, f)
    cn = field.export_mesh(level=level, normals=False)
    assert cn.normals is None and torch.equal(cn.colors, want)
    other = field.export_mesh(level=level, gridSize=[13, 11, 9], colors=False)
    a2 = field.getDenseAlpha([13, 11, 9])[0]
    sp2 = ((aabb[1] - aabb[0]) / (torch.tensor([13, 11, 9], dtype=torch.float32) - 1)).tolist()
    v2, f2, _ = mesh.marching_cubes(a2, level, spacing=sp2, origin=aabb[0].tolist())
    assert torch.equal(other.verts, v2) and torch.equal(other.faces, f2)
    empty = field.export_mesh(level=2.0)                                # alpha never exceeds 1
    assert empty.verts.shape[0] == 0 and empty.faces.shape[0] == 0 and tuple(empty.colors.shape) == (0, 3)


def test_convert_sdf_samples_to_ply(field, tmp_path):
    alpha = field.getDenseAlpha()[0]
    level = float(alpha.median())
    bbox = field.aabb.detach().float().cpu()
    vol = alpha.cpu()
    for k, (offset, scale) in enumerate([(None, None), (np.array([0.5, -1.0, 2.0], np.float32), 3.0)]):
        path = str(tmp_path / f"ref{k}.ply")
        mesh.convert_sdf_samples_to_ply(vol, path, bbox, level=level, offset=offset, scale=scale)
        want_pts, want_faces = R.convert_points(vol.numpy(), bbox.numpy(), level, offset=offset, scale=scale)
        header, props, faces = R.read_ply(path)
        got = np.stack([props["x"], props["y"], props["z"]], -1)
        assert list(props) == ["x", "y", "z"] and np.array_equal(faces, want_faces)
        # four device roundings and three host ones, on values no larger than 2 max |bbox| + max |offset|; bit-equality is expected
        big = 2 * float(bbox.abs().max()) + (0.0 if offset is None else float(np.abs(offset).max()))
        err, tol = float(np.abs(got - want_pts).max()), 7 * EPS * big
        print("convert", k, "V", len(got), "error", err, "bit-equal", np.array_equal(got, want_pts))
        assert got.shape == want_pts.shape and err <= tol
    with pytest.raises(T2NError):
        mesh.convert_sdf_samples_to_ply(vol, str(tmp_path / "none.ply"), bbox, level=2.0)


def test_export_mesh_on_a_general_shape_field():
    from tests.test_generic_gpu import _build
    m = _build()[0]
    assert m._is_general()
    with pytest.raises(T2NError):
        m.export_mesh(colors=True)
    g = [12, 10, 9]
    alpha = m.getDenseAlpha(g)[0]
    level = float(alpha.median())
    out = m.export_mesh(level=level, gridSize=g, colors=False)
    assert out.colors is None and out.verts.shape[0] > 0 and out.normals.shape == out.verts.shape
    aabb = m.aabb.detach().float().cpu()
    sp = ((aabb[1] - aabb[0]) / (torch.tensor(g, dtype=torch.float32) - 1)).tolist()
    v, f, n = mesh.marching_cubes(alpha, level, spacing=sp, origin=aabb[0].tolist())
    assert torch.equal(out.verts, v) and torch.equal(out.faces, f)
