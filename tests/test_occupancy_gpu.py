"""The kernels that change the field between training phases, element by element against the float64 references and laws of
tests/helpers/occupancy_ref.py on the cases of tests/helpers/occupancy_cases.py (whose claims tests/test_occupancy_cpu.py checks without
a GPU): k_alpha_volume, k_upsample_bilinear, alpha_value through k_alpha_at, k_filter_alpha, k_filter_bbox (also through the
general-shape descriptor), k_compute_alpha in both forms, and the host chain updateAlphaMask -> shrink -> upsample_volume_grid ->
filtering_rays. The C entry points are called directly on caller-made buffers; every output buffer is filled with a pattern first and
carries a guard region behind it. Each test prints `occupancy <case> <elements> <worst error / bound> <undecided> <K>` (pytest -s);
profiles/occupancy_elementwise.txt is that output."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle_torch as O
from text2nerf_amd import _lib
from tests.helpers import occupancy_cases as T
from tests.helpers import occupancy_ref as R
from tests.test_hip_parity import dev

pytestmark = pytest.mark.gpu

GUARD = 64
F32 = np.float32


def record(case, n, ratio, undecided, k):
    print("occupancy %-44s %7d %10.4f %5d %s" % (case, n, ratio, undecided, k))


def call(name, *args):
    d = dev()
    with torch.cuda.device(d):
        _lib.check(getattr(_lib.load(), name)(*args, _lib.current_stream_ptr(d)), name)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


class Out:
    """n elements of `dtype` filled with a pattern, GUARD more behind them that must come back untouched."""

    def __init__(self, n, dtype=torch.float32, fill=None):
        self.n = n
        self.fill = fill if fill is not None else (0xAB if dtype == torch.uint8 else float("nan") if dtype.is_floating_point else -77)
        self.t = torch.full((n + GUARD,), self.fill, dtype=dtype, device=dev())

    @property
    def ptr(self):
        return _lib.ptr(self.t)

    def get(self):
        h = self.t.cpu().numpy()
        tail = h[self.n:]
        assert np.all(np.isnan(tail)) if isinstance(self.fill, float) else np.all(tail == self.fill), "guard region written"
        return h[:self.n].copy()


def make(params, grid, aabb, near_far, step_ratio=1.0):
    from text2nerf_amd import TensorVMSplit
    m = TensorVMSplit(torch.tensor(aabb, dtype=torch.float32), list(grid), dev(), density_n_comp=[16] * 3, appearance_n_comp=[48] * 3,
                      app_dim=27, near_far=list(near_far), shadingMode="MLP_Fea_noview", alphaMask_thres=1e-4, density_shift=-10,
                      distance_scale=25, pos_pe=0, view_pe=0, fea_pe=6, featureC=128, step_ratio=step_ratio, fea2denseAct="softplus")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m


def with_mask(field, volume, box):
    from text2nerf_amd import AlphaGridMask
    field.alphaMask = None if volume is None else AlphaGridMask(dev(), torch.tensor(box, dtype=torch.float32), torch.from_numpy(volume))
    return field.sync_params()


@pytest.fixture(scope="module")
def tiny_field():
    return make(T.tiny_params(), T.TINY["grid"], T.TINY["aabb"], T.TINY["near_far"])


@pytest.fixture(scope="module")
def field_a():
    from text2nerf_amd import synth
    f = make(synth.make_field_params(3, T.FA["grid"], density_scale=0.9, aabb=T.FA["aabb"]), T.FA["grid"], T.FA["aabb"], T.FA["near_far"],
             step_ratio=T.FA["step_ratio"])
    assert float(f.stepSize) == T.STEP_A
    return f


# ---- t2n_alpha_volume ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.volume_cases()))
def test_alpha_volume(name):
    c = T.volume_cases()[name]
    dense = c["dense"]
    gx, gy, gz = dense.shape
    vol, box, src = Out(dense.size), Out(6, torch.int32), up(dense)
    call("t2n_alpha_volume", _lib.ptr(src), gx, gy, gz, C.c_float(c["thres"]), vol.ptr, box.ptr)
    r = R.check_volume(vol.get(), box.get(), dense, c["thres"])
    record("volume/" + name, dense.size, 0.0, 0, "exact")
    assert not r["bad"], (name, r, box.get())


def test_update_alpha_mask_with_nothing_kept_leaves_the_mask_alone(tiny_field):
    """Regression: updateAlphaMask used to attach the all-zero mask before it raised, so a caller that caught the error went on with a
    field that renders nothing and gets no gradient."""
    from text2nerf_amd._lib import T2NError
    f = tiny_field
    old_thres = f.alphaMask_thres
    try:
        for before in (None, (T.mask_volume((5, 7, 11), "binary"), T.MASK_BOXES["same"])):
            with_mask(f, *(before or (None, None)))
            kept = f.alphaMask
            f.alphaMask_thres = 1.5
            with pytest.raises(T2NError):
                f.updateAlphaMask((5, 6, 7))
            assert f.alphaMask is kept
    finally:
        f.alphaMask_thres = old_thres
        with_mask(f, None, None)


# ---- t2n_upsample_bilinear -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", T.RESIZE_PAIRS, ids=lambda p: "%dx%d-%dx%d" % (p[0] + p[1]))
def test_upsample_bilinear(pair):
    (hin, win), (hout, wout) = pair
    for ch in T.RESIZE_CHANNELS:
        src = T.resize_input(ch, hin, win)
        out, dsrc = Out(ch * hout * wout), up(src)
        call("t2n_upsample_bilinear", _lib.ptr(dsrc), ch, hin, win, out.ptr, hout, wout)
        got = out.get().reshape(ch, hout, wout)
        r = R.check_resize(got, src, hout, wout)
        record("resize/%dx%d-%dx%d/C%d" % (hin, win, hout, wout, ch), got.size, r["ratio"], 0,
               "copy" if (hin, win) == (hout, wout) else "K=%d" % R.K_RESIZE)
        assert r["bad"] == 0, (pair, ch, r)


# ---- t2n_alpha_at ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,boxname", [(d, b) for d in T.MASK_DIMS for b in T.MASK_BOXES])
def test_alpha_at(tiny_field, dims, boxname):
    box = T.MASK_BOXES[boxname]
    directed, cloud = T.mask_points(dims, box)
    try:
        for kind in ("binary", "real"):
            vol = T.mask_volume(dims, kind)
            h = with_mask(tiny_field, vol, box)
            for tag, pts in (("directed", directed), ("cloud", cloud)):
                out, dpts = Out(len(pts)), up(pts)
                call("t2n_alpha_at", h, _lib.ptr(dpts), len(pts), out.ptr)
                r = R.check_mask_sample(out.get(), vol, box, pts)
                record("alpha_at/%dx%dx%d/%s/%s/%s" % (dims + (boxname, kind, tag)), len(pts), r["ratio"], r["undecided"], "K=%d" % R.K_ALPHA)
                assert len(r["bad"]) == 0, (kind, tag, r["bad"][:8], pts[r["bad"][:8]])
                assert tag != "directed" or r["undecided"] == 0
    finally:
        with_mask(tiny_field, None, None)


def test_a_mask_replaced_by_one_of_the_same_shape_is_uploaded(tiny_field):
    """Regression: sync_params keyed the uploaded mask by (pointer, version, shape) alone. A mask dropped and another of the same shape
    attached before the next sync usually gets the freed block back, so the new volume was taken for the old one and the kernels went
    on with the stale copy (tests/test_march_list_gpu.py's sparse case after its mask case, when the allocator chose so)."""
    from text2nerf_amd import AlphaGridMask
    f, dims, box = tiny_field, (5, 7, 11), T.MASK_BOXES["same"]
    _, pts = T.mask_points(dims, box)
    dpts = up(pts)
    try:
        for seed in range(4):
            vol = (np.random.default_rng(seed).uniform(size=dims) < 0.5).astype(F32)
            f.alphaMask = None                       # drop the old volume, no sync in between
            f.alphaMask = AlphaGridMask(dev(), torch.tensor(box, dtype=torch.float32), torch.from_numpy(vol))
            out = Out(len(pts))
            call("t2n_alpha_at", f.sync_params(), _lib.ptr(dpts), len(pts), out.ptr)
            r = R.check_mask_sample(out.get(), vol, box, pts)
            assert len(r["bad"]) == 0 and r["undecided"] <= T.UNDECIDED_CAP * len(pts), (seed, len(r["bad"]))
    finally:
        with_mask(f, None, None)


# ---- t2n_filter_rays_alpha -------------------------------------------------------------------------------------------------------------------
def run_filter(h, rays, n):
    out, drays = Out(rays.shape[0], torch.uint8), up(rays)
    call("t2n_filter_rays_alpha", h, _lib.ptr(drays), rays.shape[0], rays.shape[1], n, out.ptr)
    return out.get()


@pytest.mark.parametrize("n", T.FILTER_N)
def test_filter_alpha_directed(field_a, n):
    cfg = T.cfg_a(T.slab_mask())
    h = with_mask(field_a, T.slab_mask(), T.FA["aabb"])
    rays, want = T.filter_rays(n)
    ref = R.filter_alpha(cfg, rays, n)
    assert ref["decided"].all() and np.array_equal(ref["keep"], want)
    for stride in (6, 11):
        got = run_filter(h, T.with_stride(rays, stride), n)
        assert len(R.check_flags(got, ref)["bad"]) == 0, (n, stride, got, want)
    record("filter_alpha/directed/n%d" % n, 2 * len(rays), 0.0, 0, "decision")
    if n == 129:
        for count in T.FILTER_COUNTS:
            r, w = T.tiled(rays, want, count)
            got = run_filter(h, T.with_stride(r, 11), n)
            assert np.array_equal(got, w.astype(np.uint8)), count
            record("filter_alpha/directed/n129/rays%d" % count, count, 0.0, 0, "decision")


def test_filter_alpha_oblique(field_a):
    vol = T.blob_mask()
    h = with_mask(field_a, vol, T.FA["aabb"])
    rays = T.oblique_rays()
    ref = R.filter_alpha(T.cfg_a(vol), rays, 128)
    r = R.check_flags(run_filter(h, rays, 128), ref)
    record("filter_alpha/oblique/n128", len(rays), 0.0, r["undecided"], "decision")
    assert len(r["bad"]) == 0 and r["undecided"] <= T.UNDECIDED_CAP * len(rays)


# ---- t2n_filter_rays_bbox and the general-shape descriptor's form ------------------------------------------------------------------------------
def generic_desc(f):
    d = _lib.GenericDesc()
    a = np.asarray(f["aabb"], F32)
    for k in range(3):
        d.aabb_min[k], d.aabb_max[k] = float(a[0, k]), float(a[1, k])
        d.inv_aabb_size[k] = float(F32(2.0) / (a[1, k] - a[0, k]))
        d.grid[k] = f["grid"][k]
        d.density_n_comp[k], d.app_n_comp[k] = 16, 48
    d.app_dim, d.shading, d.fea_pe, d.view_pe, d.feature_c = 27, _lib.SHADE_IDS["MLP_Fea_noview"], 6, 0, 128
    d.act = _lib.ACT_IDS["softplus"]
    d.density_shift, d.distance_scale, d.weight_thres, d.step_size = -10.0, 25.0, 1e-4, 1.0
    d.near, d.far, d.z_gate = f["near_far"][0], f["near_far"][1], 2.0
    return d


def test_filter_bbox():
    from text2nerf_amd import synth
    f = make(synth.make_field_params(5, T.FB["grid"], density_scale=0.9, aabb=T.FB["aabb"]), T.FB["grid"], T.FB["aabb"], T.FB["near_far"])
    h = f.sync_params()
    desc = generic_desc(T.FB)

    def run(rays, generic):
        out, drays = Out(rays.shape[0], torch.uint8), up(rays)
        if generic:
            call("t2n_generic_filter_rays", C.byref(desc), _lib.ptr(drays), rays.shape[0], rays.shape[1], 0, 1, out.ptr)
        else:
            call("t2n_filter_rays_bbox", h, _lib.ptr(drays), rays.shape[0], rays.shape[1], out.ptr)
        return out.get()

    rays, want, names = T.bbox_rays()
    ref = R.slab(T.FB["aabb"], rays)
    assert ref["decided"].all() and np.array_equal(ref["keep"], want)
    seeded = T.bbox_seeded()
    sref = R.slab(T.FB["aabb"], seeded)
    for generic in (False, True):
        tag = "generic" if generic else "field"
        for stride in (6, 11):
            bad = R.check_flags(run(T.with_stride(rays, stride), generic), ref)["bad"]
            assert len(bad) == 0, (tag, stride, [names[i] for i in bad])
        record("filter_bbox/%s/directed" % tag, 2 * len(rays), 0.0, 0, "decision")
        for count in T.BBOX_COUNTS:
            r, w = T.tiled(rays, want, count)
            assert np.array_equal(run(T.with_stride(r, 11), generic), w.astype(np.uint8)), (tag, count)
            record("filter_bbox/%s/rays%d" % (tag, count), count, 0.0, 0, "decision")
        r = R.check_flags(run(seeded, generic), sref)
        record("filter_bbox/%s/seeded" % tag, len(seeded), 0.0, r["undecided"], "decision")
        assert len(r["bad"]) == 0 and r["undecided"] <= T.UNDECIDED_CAP * len(seeded)


# ---- t2n_compute_alpha / t2n_dense_alpha -----------------------------------------------------------------------------------------------------
def median_length(cfg, pts, bf16):
    s = R.alpha_at_points(cfg, T.tiny_params(), pts, 1.0, bf16=bf16)["sigma"]
    return float(F32(1e-4 / np.median(s)))


@pytest.mark.parametrize("bf16", (False, True), ids=("fp32", "bf16"))
@pytest.mark.parametrize("maskname", list(T.alpha_masks()))
def test_compute_alpha_and_dense_alpha(maskname, bf16):
    """Under bf16 factor storage k_compute_alpha reads the float32 copies of the ROUNDED factors (t2n_api.hip k_relayout writes the
    rounded value to both copies): the reference is the oracle on the bf16-rounded field, the one the marcher renders."""
    mask = T.alpha_masks()[maskname]
    cfg = T.tiny_cfg(mask)
    params = T.tiny_params()
    f = make(params, T.TINY["grid"], T.TINY["aabb"], T.TINY["near_far"])
    f.factor_storage = "bf16" if bf16 else "fp32"
    h = with_mask(f, *(mask or (None, None)))
    tag = "%s/%s" % (maskname, "bf16" if bf16 else "fp32")
    directed, cloud = T.box_points()
    for name, pts in (("directed", directed), ("cloud", cloud)):
        for lname, length in (("step", cfg.step_size), ("saturate", T.LENGTH_SATURATE), ("1e-4", median_length(cfg, pts, bf16))):
            out, dpts = Out(len(pts)), up(pts)
            call("t2n_compute_alpha", h, _lib.ptr(dpts), len(pts), C.c_float(length), out.ptr)
            ref = R.alpha_at_points(cfg, params, pts, length, bf16=bf16)
            r = R.check_alpha(out.get(), ref)
            record("compute_alpha/%s/%s/%s" % (tag, name, lname), len(pts), r["ratio"], r["undecided"], "K=%d x law" % R.K_MARCH)
            assert len(r["bad"]) == 0, (tag, name, lname, r["bad"][:8])
            assert name != "directed" or r["undecided"] == 0
    for g in T.DENSE_GRIDS:
        lins = T.linspaces(g)
        nodes = R.dense_nodes(T.TINY["aabb"], lins).reshape(-1, 3)
        out, at = Out(len(nodes)), Out(len(nodes))
        dl, dnodes = [up(l) for l in lins], up(nodes)
        call("t2n_dense_alpha", h, _lib.ptr(dl[0]), _lib.ptr(dl[1]), _lib.ptr(dl[2]), g[0], g[1], g[2],
             C.c_float(cfg.step_size), out.ptr)
        call("t2n_compute_alpha", h, _lib.ptr(dnodes), len(nodes), C.c_float(cfg.step_size), at.ptr)
        got = out.get()
        ref = R.alpha_at_points(cfg, params, nodes, cfg.step_size, bf16=bf16)
        r = R.check_alpha(got, ref)
        record("dense_alpha/%s/%dx%dx%d" % ((tag,) + tuple(g)), len(nodes), r["ratio"], r["undecided"], "K=%d x law" % R.K_MARCH)
        assert len(r["bad"]) == 0 and r["undecided"] == 0, (tag, g, r["bad"][:8])
        # the kernel's own node positions are the float32 restatement's, bit for bit: same alpha as at those explicit points
        assert np.array_equal(got.view(np.uint32), at.get().view(np.uint32)), g
    if maskname == "none" and not bf16:
        for g in T.DENSE_GRIDS:
            alpha, xyz = f.getDenseAlpha(g)
            assert np.array_equal(xyz.cpu().numpy().view(np.uint32), R.dense_nodes(T.TINY["aabb"], T.linspaces(g)).view(np.uint32)), g
            assert tuple(alpha.shape) == tuple(g)


# ---- host chain ----------------------------------------------------------------------------------------------------------------------------------
def test_host_chain():
    case, params = T.CHAIN, T.chain_params()
    g = case["mask_grid"]
    lins = T.linspaces(g)
    f = make(params, case["grid"], case["aabb"], case["near_far"])
    f.alphaMask_thres = case["thres"]
    cfg0 = O.FieldConfig(aabb=case["aabb"], grid_size=case["grid"], near_far=case["near_far"])
    alpha, xyz = f.getDenseAlpha(g)
    nodes = R.dense_nodes(case["aabb"], lins)
    assert np.array_equal(xyz.cpu().numpy().view(np.uint32), nodes.view(np.uint32)) and float(f.stepSize) == cfg0.step_size
    r = R.check_alpha(alpha.cpu().numpy(), R.alpha_at_points(cfg0, params, nodes.reshape(-1, 3), cfg0.step_size))
    record("chain/dense_alpha", alpha.numel(), r["ratio"], r["undecided"], "K=%d x law" % R.K_MARCH)
    assert len(r["bad"]) == 0
    rays = T.chain_rays()
    c = R.chain(case, params, alpha.cpu().numpy(), lins, rays, 256)

    new_aabb = f.updateAlphaMask(g)
    assert np.array_equal(f.alphaMask.alpha_volume[0, 0].cpu().numpy(), c["volume"])
    assert np.array_equal(new_aabb.cpu().numpy().view(np.uint32), c["new_aabb"].view(np.uint32))
    assert np.array_equal(f.alphaMask.aabb.cpu().numpy(), np.asarray(case["aabb"], F32))
    record("chain/volume", c["volume"].size, 0.0, 0, "exact")

    f.shrink(new_aabb)
    assert f.gridSize.tolist() == c["shrunk_grid"]
    assert np.array_equal(f.aabb.cpu().numpy().view(np.uint32), c["shrunk_aabb"].view(np.uint32))
    sd = {k: v.detach().cpu().numpy() for k, v in f.state_dict().items()}
    for k in R.FACTOR_KEYS:
        assert sd[k].shape == c["cropped"][k].shape and np.array_equal(sd[k].view(np.uint32), c["cropped"][k].view(np.uint32)), k
    record("chain/cropped_factors", sum(c["cropped"][k].size for k in R.FACTOR_KEYS), 0.0, 0, "exact")

    f.upsample_volume_grid(case["upsample"])
    sd = {k: v.detach().cpu().numpy() for k, v in f.state_dict().items()}
    res = case["upsample"]
    worst, count = 0.0, 0
    for i in range(3):
        m0, m1 = ((0, 1), (0, 2), (1, 2))[i]
        v = (2, 1, 0)[i]
        for kind in ("density", "app"):
            for key, (ho, wo) in (("%s_plane.%d" % (kind, i), (res[m1], res[m0])), ("%s_line.%d" % (kind, i), (res[v], 1))):
                assert sd[key].shape[2:] == (ho, wo), key
                r = R.check_resize(sd[key][0], c["cropped"][key][0], ho, wo)
                assert r["bad"] == 0, (key, r)
                worst, count = max(worst, r["ratio"]), count + sd[key].size
    record("chain/resized_factors", count, worst, 0, "K=%d" % R.K_RESIZE)
    assert float(f.stepSize) == c["cfg"].step_size and f.alphaMask is not None

    index = torch.arange(len(rays), dtype=torch.float32).view(-1, 1)
    kept_rays, kept_index = f.filtering_rays(torch.from_numpy(rays), index, N_samples=256, bbox_only=False)
    got = np.zeros(len(rays), np.uint8)
    got[kept_index.view(-1).long().numpy()] = 1
    r = R.check_flags(got, c["filter"])
    record("chain/filtering_rays/n256", len(rays), 0.0, r["undecided"], "decision")
    assert len(r["bad"]) == 0 and r["undecided"] <= T.UNDECIDED_CAP * len(rays)
    assert np.array_equal(kept_rays.numpy(), rays[got == 1])
