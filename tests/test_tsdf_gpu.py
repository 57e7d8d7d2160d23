"""The TSDF stages on the device against tests/helpers/tsdf_ref.py (checked on its own in tests/test_tsdf_cpu.py): everything BIT-EQUAL.
`vertex_normals`' bit-equality to numpy (tests/test_mesh_smooth_gpu.py) is the precedent that double divide and sqrt are correctly
rounded on the device.

tsdf_integrate: grids whose last axis runs past one wave and is no multiple of it, (2,2,2), four 33x24 views of which one camera sits
inside the grid (nodes with p_z <= near) and one faces away (it updates nothing), depth pixels holding 0, a negative, NaN and +inf, pixel
weights holding 0 and NaN, both depth kinds, colours / weights / max_weight on and off; views one at a time, `volume=`, two calls.
select_faces against numpy around the 256-element workgroup; tsdf_mesh on the sphere scene; tsdf_volume / export_tsdf_mesh on the
suite's tiny field."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.helpers import mc_ref
from tests.helpers import mesh_levelset_ref as L
from tests.helpers import tsdf_ref as R
from tests.test_hip_parity import dev, make_field
from tests.test_optim_kernels_gpu import Buf, call
from text2nerf_amd import _lib, mesh, synth, tsdf

pytestmark = pytest.mark.gpu

POSES = R.FRONT_POSES[:2] + (R.INSIDE_POSE, R.AWAY_POSE)
# every grid holds a piece of the sphere's near side: the full scene; a 5 x 3 strip through the sphere along z; one cell on its surface
GRIDS = {(37, 21, 70): R.SPHERE["origin"], (5, 3, 65): (-0.15, -0.13, -2.2), (2, 2, 2): (0.0, -0.05, -0.75)}
VARIANTS = {"plain": dict(color=False, weights=False, max_weight=math.inf), "full": dict(color=True, weights=True, max_weight=2.5)}


@functools.lru_cache(maxsize=None)
def scene(shape, kind):
    sc = R.sphere_scene(shape=shape, poses=POSES, kind=kind)
    sc["origin"] = GRIDS[shape]
    return R.with_bad_pixels(sc)


@functools.lru_cache(maxsize=None)
def reference(shape, kind, variant):
    return R.run(scene(shape, kind), **VARIANTS[variant])


def t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def integrate(sc, color, weights, max_weight, views=None, volume=None, numpy_in=False):
    sel = list(range(len(sc["depth"]))) if views is None else list(views)
    conv = (lambda x: x) if numpy_in else t
    return tsdf.tsdf_integrate(conv(sc["depth"][sel]), sc["poses"][sel], sc["intrinsic"], sc["origin"], sc["spacing"], sc["shape"], sc["trunc"],
                               colors=conv(sc["rgb"][sel]) if color else None, weights=conv(sc["pw"][sel]) if weights else None,
                               depth_kind=("ray", "z")[sc["kind"]], max_weight=None if math.isinf(max_weight) else max_weight, volume=volume)


def host(vol):
    return tuple(None if x is None else (x if isinstance(x, np.ndarray) else x.cpu().numpy()) for x in (vol.tsdf, vol.weight, vol.color))


def assert_state(got, want, what):
    for name, a, b in zip(("tsdf", "weight", "color"), got, want):
        if a is None or b is None:
            assert a is None and b is None, (what, name)
            continue
        bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
        assert a.shape == b.shape and len(bad) == 0, (what, name, len(bad), bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", [0, 1], ids=["ray", "z"])
@pytest.mark.parametrize("shape", list(GRIDS), ids=lambda s: "x".join(map(str, s)))
def test_integrate_bit_equal(shape, kind, variant):
    sc, want = scene(shape, kind), reference(shape, kind, variant)
    vol = integrate(sc, **VARIANTS[variant])
    assert vol.tsdf.is_cuda and tuple(vol.tsdf.shape) == shape and (vol.color is None) == (not VARIANTS[variant]["color"])
    assert_state(host(vol), want, "batched")
    # the scene does what the case list asks for
    assert int((want[1] > 0).sum()) > 0 and float(want[0].min()) < 0.0 < float(want[0].max())
    if shape != (2, 2, 2):
        assert int((want[1] == 0).sum()) > 0
        z = sc["origin"][2] + np.arange(shape[2]) * sc["spacing"][2]
        assert (z < R.INSIDE_POSE[2, 3]).any()                  # nodes behind the camera that sits inside the grid
    if variant == "full":
        assert float(want[1].max()) == 2.5                      # the cap was reached
    # two identical calls; views one at a time; numpy in, numpy out
    assert_state(host(integrate(sc, **VARIANTS[variant])), host(vol), "second call")
    part = None
    for v in range(len(POSES)):
        part = integrate(sc, **VARIANTS[variant], views=[v], volume=part)
    assert_state(host(part), want, "one view at a time")
    if kind == 0:
        out = integrate(sc, **VARIANTS[variant], numpy_in=True)
        assert isinstance(out.tsdf, np.ndarray)
        assert_state(host(out), want, "numpy")


def test_integrate_view_facing_away_and_continuation():
    shape = (37, 21, 70)
    sc, kw = scene(shape, 0), VARIANTS["full"]
    away = len(POSES) - 1
    fresh = integrate(sc, **kw, views=[away])
    assert_state(host(fresh), R.fresh(shape, True), "away view on a fresh volume")
    first = integrate(sc, **kw, views=[0, 1])
    before = tuple(x.copy() for x in host(first))
    assert_state(before, R.run(sc, **kw, views=[0, 1]), "two views")
    same = integrate(sc, **kw, views=[away], volume=first)
    assert same.tsdf.data_ptr() == first.tsdf.data_ptr()        # a device volume is continued in place
    assert_state(host(same), before, "away view on an integrated volume")
    rest = integrate(sc, **kw, views=[2, 3], volume=first)
    assert_state(host(rest), reference(shape, 0, "full"), "volume= continues")
    empty = integrate(sc, **kw, views=[], volume=rest)
    assert empty is rest
    none = integrate(sc, **kw, views=[])
    assert_state(host(none), R.fresh(shape, True), "V = 0")


def test_integrate_writes_inside_its_buffers():
    """The raw call on guarded buffers: nothing outside the three state arrays is written."""
    shape = (5, 3, 65)
    sc = scene(shape, 0)
    T0, W0, C0 = R.fresh(shape, True)
    T, Wt, Cl = Buf(T0), Buf(W0), Buf(C0)
    d, rgb, pw, m = t(sc["depth"]), t(sc["rgb"]), t(sc["pw"]), t(sc["w2c"])
    import ctypes as C
    fx, fy, cx, cy = sc["intrinsic"]
    call("t2n_tsdf_integrate", T.ptr, Wt.ptr, Cl.ptr, *shape, _lib.ptr(d), _lib.ptr(rgb), _lib.ptr(pw), _lib.ptr(m), len(POSES), sc["H"], sc["W"],
         fx, fy, cx, cy, (C.c_float * 3)(*sc["origin"]), (C.c_float * 3)(*sc["spacing"]), sc["trunc"], 0.0, 2.5, 0)
    torch.cuda.synchronize()
    assert T.guards_intact() and Wt.guards_intact() and Cl.guards_intact()
    assert_state((T.get(), Wt.get(), Cl.get()), reference(shape, 0, "full"), "raw call")
    lib = _lib.load()
    assert lib.t2n_tsdf_integrate(T.ptr, Wt.ptr, None, 2048, 1024, 1024, _lib.ptr(d), None, None, _lib.ptr(m), 1, sc["H"], sc["W"], fx, fy, cx, cy,
                                  (C.c_float * 3)(*sc["origin"]), (C.c_float * 3)(*sc["spacing"]), sc["trunc"], 0.0, 2.5, 0, None) == -2
    assert lib.t2n_tsdf_integrate(T.ptr, Wt.ptr, None, *shape, _lib.ptr(d), None, None, _lib.ptr(m), 1, sc["H"], sc["W"], 0.0, fy, cx, cy,
                                  (C.c_float * 3)(*sc["origin"]), (C.c_float * 3)(*sc["spacing"]), sc["trunc"], 0.0, 2.5, 0, None) == -1


# ---- select_faces ---------------------------------------------------------------------------------------------------------------------------
def assert_mesh(got, want, what):
    for name, a, b in zip(("verts", "faces", "normals", "colors"), got, want):
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
        assert R.same_bits(a, b), (what, name, None if a is None else a.shape, None if b is None else b.shape)


@pytest.mark.parametrize("name", ["noise", "ellipsoid"])
def test_select_faces_on_marching_cubes_meshes(name):
    vol = mc_ref.noise_volume() if name == "noise" else mc_ref.ellipsoid_volume()
    v, f, n = mc_ref.marching_cubes(vol, 0.0, spacing=(0.5, 0.4, 0.3), origin=(-1.0, 2.0, 0.5))
    c = (np.arange(v.size) % 253).astype(np.uint8).reshape(v.shape)
    rng = np.random.default_rng(5)
    assert len(f) > 600
    for what, keep in (("random", rng.random(len(f)) < 0.4), ("sparse", rng.random(len(f)) < 0.01), ("all", np.ones(len(f), bool)),
                       ("none", np.zeros(len(f), bool))):
        want = R.select_faces(v, f, n, c, keep)
        got = mesh.select_faces(mesh.Mesh(t(v), t(f), t(n), t(c)), t(keep))
        assert got.verts.is_cuda
        assert_mesh(got, want, what)
        assert_mesh(mesh.select_faces((v, f, n, c), keep.astype(np.int64)), want, what + " numpy")
        assert_mesh(mesh.select_faces((t(v), t(f)), t(keep)), (want[0], want[1], None, None), what + " bare")
    assert R.same_bits(want[0], np.zeros((0, 3), np.float32)) and want[1].shape == (0, 3)       # none kept: empty
    whole = mesh.select_faces((t(v), t(f), t(n), t(c)), t(np.ones(len(f), bool)))
    assert_mesh(whole, (v, f, n, c), "all kept is the same mesh")                            # (every vertex of a marching-cubes mesh is used)
    with pytest.raises(ValueError):
        mesh.select_faces((t(v), t(f)), t(np.ones(len(f) - 1, bool)))


def test_select_faces_around_the_workgroup_size():
    rng = np.random.default_rng(11)
    for V in (255, 256, 257):
        for F in (255, 256, 257):
            v = rng.standard_normal((V, 3)).astype(np.float32)
            f = rng.integers(0, V, (F, 3)).astype(np.int32)
            c = rng.integers(0, 256, (V, 3)).astype(np.uint8)
            keep = rng.random(F) < 0.3
            keep[[0, F - 1]] = True
            f[F - 1] = (V - 1, 0, V - 1)                        # the last face and the last vertex stay
            assert_mesh(mesh.select_faces((t(v), t(f), None, t(c)), t(keep)), R.select_faces(v, f, None, c, keep), (V, F))


# ---- tsdf_mesh ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1], ids=["ray", "z"])
def test_tsdf_mesh_on_the_sphere_scene(kind):
    sc = R.sphere_scene(kind=kind)
    state = R.run(sc)
    want, keep, (v0, f0) = R.mesh(state, sc["origin"], sc["spacing"])
    vol = integrate(sc, True, False, math.inf)
    assert_state(host(vol), state, "sphere scene")
    got = tsdf.tsdf_mesh(vol)
    assert 0 < got.faces.shape[0] == int(keep.sum()) < len(f0)
    assert_mesh(got, want, "tsdf_mesh")
    assert float(np.abs(R.sphere_distance(got.verts.cpu().numpy(), sc)).max()) <= 1.5 * max(sc["spacing"])
    bare = tsdf.tsdf_mesh(vol, normals=False, colors=False)
    assert bare.normals is None and bare.colors is None and torch.equal(bare.verts, got.verts) and torch.equal(bare.faces, got.faces)
    # a min_weight above one view keeps less; above every view keeps nothing: empty arrays, not an error
    some = tsdf.tsdf_mesh(vol, min_weight=1.5)
    assert_mesh(some, R.mesh(state, sc["origin"], sc["spacing"], min_weight=1.5)[0], "min_weight 1.5")
    assert 0 < some.faces.shape[0] < got.faces.shape[0]
    none = tsdf.tsdf_mesh(vol, min_weight=float(len(sc["depth"])))
    assert none.verts.shape == (0, 3) and none.faces.shape == (0, 3) and none.normals.shape == (0, 3) and none.colors.shape == (0, 3)
    # numpy in, numpy out; a volume without colour has none
    nv = tsdf.tsdf_mesh(tsdf.TSDFVolume(*state, vol.origin, vol.spacing, vol.trunc))
    assert isinstance(nv.verts, np.ndarray)
    assert_mesh(nv, want, "numpy volume")
    assert tsdf.tsdf_mesh(vol._replace(color=None)).colors is None
    # the result composes with the other mesh stages
    big = mesh.filter_components(got, keep_largest=1)
    assert 0 < big.faces.shape[0] <= got.faces.shape[0]
    assert mesh.smooth_mesh(big, iterations=2).verts.shape == big.verts.shape


# ---- the field's own route -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blob():
    shape = L.SHAPES["tiny"]
    return shape, make_field(L.blob_params(shape), shape["grid"], shape["aabb"], shape["near_far"])


# three cameras inside the box whose rays reach the blob's opaque part well before near_far[1] (with the step of this 24 x 20 x 16 field,
# 0.76, the float64 oracle puts the median depths at 3.5 .. 6.6 from them)
FIELD_POSES = np.stack([synth.look_pose(0.0, 0.0, (-0.8, 1.1, -1.5)), synth.look_pose(0.3, 0.05, (-2.4, 0.8, -1.2)),
                        synth.look_pose(-0.3, -0.05, (0.8, 1.4, -1.2))])
FIELD_INTR = (48.0, 48.0, 24.0, 24.0)


def test_tsdf_volume_and_export_on_the_tiny_field(blob, tmp_path):
    shape, m = blob
    H = W = 48
    g = shape["grid"]
    vol = m.tsdf_volume(FIELD_POSES, FIELD_INTR, H, W)
    assert tuple(vol.tsdf.shape) == tuple(g) and tuple(vol.color.shape) == tuple(g) + (3,)
    aabb = np.asarray(shape["aabb"], np.float32)
    sp = (torch.tensor(aabb[1] - aabb[0]) / (torch.tensor(g, dtype=torch.float32) - 1)).tolist()
    assert vol.origin == tuple(float(x) for x in aabb[0]) and vol.spacing == tuple(float(np.float32(x)) for x in sp)
    assert vol.trunc == 4.0 * max(sp)
    got = tsdf.tsdf_mesh(vol)
    path = str(tmp_path / "scene.ply")
    exp = m.export_tsdf_mesh(path, FIELD_POSES, FIELD_INTR, H, W)
    for a, b in zip(got, exp):
        assert torch.equal(a, b)
    again = tsdf.tsdf_mesh(m.tsdf_volume(FIELD_POSES, FIELD_INTR, H, W))
    for a, b in zip(got, again):
        assert torch.equal(a, b)                                # two calls are bit-equal
    v = got.verts.cpu().numpy()
    print(f"TSDF tiny field: {got.faces.shape[0]} faces, {len(v)} vertices, {int((vol.weight > 0).sum())} of {vol.weight.numel()} nodes observed")
    # (inside the aabb up to the float32 rounding of origin + index * spacing at the box's far faces: 2 ulp of 8)
    assert got.faces.shape[0] > 0 and (v >= aabb[0] - 2e-6).all() and (v <= aabb[1] + 2e-6).all()
    assert got.normals.shape == got.verts.shape and got.colors.dtype == torch.uint8
    header, props, faces = mc_ref.read_ply(path)
    assert np.array_equal(faces, got.faces.cpu().numpy())
    assert np.array_equal(np.stack([props["x"], props["y"], props["z"]], -1), v)
    assert np.array_equal(np.stack([props["red"], props["green"], props["blue"]], -1), got.colors.cpu().numpy())
    assert np.array_equal(np.stack([props["nx"], props["ny"], props["nz"]], -1), got.normals.cpu().numpy())
    # the volume is the hand-made one: the renders of every pose, integrated by tsdf_integrate
    from text2nerf_amd import generate_rays
    ds, cs = [], []
    for c2w in FIELD_POSES:
        rays = generate_rays(H, W, FIELD_INTR, c2w, device=dev())
        geo = m.render_geometry(rays, want=("median",))
        ds.append(torch.where(geo.acc >= 0.5, geo.depth_median, torch.full_like(geo.acc, float(shape["near_far"][1]))).reshape(H, W))
        cs.append(m(rays, white_bg=True, is_train=False, frame_width=W)[0].reshape(H, W, 3))
    # the views see the blob, and part of the mesh is its surface, not the cap that carving draws at near_far[1] (the float64 oracle with
    # the numpy reference behind it: 2693 such pixels, 199 such vertices)
    far = float(shape["near_far"][1])
    assert int((torch.stack(ds) < far - 1.0).sum()) > 500
    cam = torch.from_numpy(FIELD_POSES[:, :3, 3]).to(dev())
    assert int(((got.verts[:, None, :] - cam[None]).norm(dim=-1).amin(1) < far - 1.0).sum()) > 50
    hand = tsdf.tsdf_integrate(torch.stack(ds), FIELD_POSES, FIELD_INTR, vol.origin, vol.spacing, g, vol.trunc, colors=torch.stack(cs))
    # geometry bit for bit (render_geometry involves no frame cache). The colour state is a convex combination of rendered rgb, and two
    # renders of one frame may differ by rounding (a frame before and after the field's caches are built: each within the suite's 1e-4 of
    # the oracle), so the colours agree to 2e-4
    print(f"TSDF tiny field: colour state of tsdf_volume against the hand-made one: max difference {float((vol.color - hand.color).abs().max()):.3g}")
    assert R.same_bits(host(vol)[0], host(hand)[0]) and R.same_bits(host(vol)[1], host(hand)[1])
    assert float((vol.color - hand.color).abs().max()) <= 2e-4 and float(vol.color.max()) > 0.1
    # carve=False observes no more nodes than carve=True; the expected depth and no colours are accepted
    loose = m.tsdf_volume(FIELD_POSES, FIELD_INTR, H, W, carve=False, colors=False, depth="depth")
    assert loose.color is None and 0 < int((loose.weight > 0).sum()) <= int((vol.weight > 0).sum())
    assert m.export_tsdf_mesh(None, FIELD_POSES, FIELD_INTR, H, W, colors=False, normals=False).colors is None
    with pytest.raises(ValueError):
        m.tsdf_volume(FIELD_POSES, FIELD_INTR, H, W, depth="mode")
    # the other exports are what they were
    assert m.export_mesh(level=L.ALPHA_LEVEL).verts.shape[0] > 400
