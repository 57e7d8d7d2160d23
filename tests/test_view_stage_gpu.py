"""The depth stage of a new view on the MI355X (csrc/t2n_view.hip through text2nerf_amd.warp: sample_filled_pixels,
prepare_depth_merge, finish_view, and the update_known_views=True mask expansion) against the goldens made by executing the reference's
lines (tests/golden/view_stage.npz) and the numpy restatement pinned to them (tests/helpers/view_stage_ref.py). Everything new is
index arithmetic or a fixed sequence of correctly rounded operations: bit-equal. The alignment's scale / shift are held at the bounds of
tests/test_align.py (the same kernel; it reads the estimate as float32 where the reference holds float64); what lies behind the forward
warp at the bounds of tests/test_support_gpu.py (fp64 atomics sum in arrival order)."""
import os
import random
import sys

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN, TINY
from tests.helpers import view_stage_ref as VR
from text2nerf_amd import synth

sys.path.insert(0, GOLDEN)
import make_golden_view_stage_cases as VC  # noqa: E402
from make_golden_support_cases import H, W, support_inputs  # noqa: E402
from make_golden_warp_cases import pose44, warp_poses  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "view_stage.npz"), allow_pickle=False))


def _bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


# ---- 1: the filled-pixel list -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VC.SAMPLE_CASES))
def test_sample_filled_pixels_matches_the_excerpt(gold, name):
    from text2nerf_amd.warp import sample_filled_pixels
    m = VC.sample_mask(name)
    seed = VC.SAMPLE_CASES[name]
    ref_rng = random.Random(seed)
    ref = VR.sample_filled_pixels(m, ref_rng)                          # random.sample of the list, as the reference calls it
    assert np.array_equal(ref, gold[f"sample_{name}"])
    # numpy in -> numpy out, on the module-level generator the reference uses
    random.seed(seed)
    got = sample_filled_pixels(m)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == ref.shape and np.array_equal(got, ref)
    assert random.getstate() == ref_rng.getstate()
    assert [random.getrandbits(32) for _ in range(4)] == gold[f"sample_{name}_next"].tolist()
    # device in -> device out, a generator of the caller's own, the int32 `known` form
    rng = random.Random(seed)
    t = sample_filled_pixels(torch.from_numpy(m.astype(np.int32)).to(DEV), rng=rng)
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and np.array_equal(t.cpu().numpy(), ref)
    assert rng.getstate() == ref_rng.getstate()
    if name == "cap":
        assert int(m.sum()) > 10000 and got.shape == (10000, 2)
        few = sample_filled_pixels(m, max_samples=100, rng=random.Random(5))
        assert np.array_equal(few, VR.sample_filled_pixels(m, random.Random(5), 100))
    if name == "none":
        assert got.shape == (0, 2)


def test_sample_filled_pixels_non_square_and_every_rank():
    from text2nerf_amd.warp import sample_filled_pixels
    m = VC.nonsquare_mask()
    ref_rng, rng = random.Random(31), random.Random(31)
    assert np.array_equal(sample_filled_pixels(m, rng=rng), VR.sample_filled_pixels(m, ref_rng)) and rng.getstate() == ref_rng.getstate()

    class InOrder:                                                     # every rank once, in order: the select kernel gives the list itself
        @staticmethod
        def sample(population, k):
            return list(population)[:k]
    for mask in (m, VC.sample_mask("cols"), (np.random.Generator(np.random.PCG64(9)).uniform(0, 1, (150, 70)) < 0.4).astype(np.int64)):
        got = sample_filled_pixels(mask, max_samples=10 ** 6, rng=InOrder)
        assert np.array_equal(got, np.asarray(VR.filled_pixels(mask), np.int32).reshape(-1, 2))
    fl = m.astype(np.float64) * 0.25                                   # a float map: filled is > 0
    assert np.array_equal(sample_filled_pixels(fl, rng=random.Random(31)), VR.sample_filled_pixels(m, random.Random(31)))


# ---- 2: alignment and the merge network's inputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VC.MERGE_CASES))
def test_prepare_depth_merge(gold, name):
    from oracle import oracle_warp as OW
    from text2nerf_amd.warp import DepthMerge, align_depth_global, prepare_depth_merge
    dr, m, de = VC.merge_inputs(name)
    seed = VC.MERGE_CASES[name][3]
    random.seed(seed)
    out = prepare_depth_merge(dr, m, de, VC.PUSH)
    assert isinstance(out, DepthMerge) and all(isinstance(a, np.ndarray) for a in out[2:])
    assert [random.getrandbits(32) for _ in range(4)] == gold[f"merge_{name}_next"].tolist()
    assert out.pixel_sample.dtype == np.int32 and np.array_equal(out.pixel_sample, gold[f"merge_{name}_pixel_sample"])
    g_scale, g_shift = gold[f"merge_{name}_scale_shift"]
    print(name, "scale", out.scale, g_scale, "shift", out.shift, g_shift)
    if name == "empty":
        # the reference's fallbacks: scale = thresh, shift = max scaled - max rendered, on the float32 estimate the device reads
        de32 = de.astype(np.float32).astype(np.float64)
        thresh = (dr.max() - VC.PUSH) / (de32.max() - VC.PUSH)
        assert out.pixel_sample.shape == (0, 2)
        assert abs(out.scale - thresh) <= 1e-12 * abs(thresh) and abs(out.shift - ((de32 * thresh).max() - dr.max())) <= 1e-12
    assert abs(out.scale - g_scale) <= 2e-6 * abs(g_scale) and abs(out.shift - g_shift) <= 2e-6
    np.testing.assert_allclose(out.depth_shift, gold[f"merge_{name}_depth_shift"], rtol=0, atol=5e-6)
    if name != "empty":
        # the oracle on what the device reads: the rendered depth as float32 (exact for a float32 render times 0 / 1), the estimate rounded
        o_scale, o_shift, o_ds = OW.align_depth_global(dr.astype(np.float32), de.astype(np.float32).astype(np.float64), out.pixel_sample, VC.PUSH)
        assert abs(out.scale - o_scale) <= 1e-9 * abs(o_scale) + 1e-12 and abs(out.shift - o_shift) <= 1e-9 * max(abs(o_shift), 1.0)
    # the merge inputs: the excerpt's arithmetic on the device's own float32 depth_shift and the float64 depth_rendered, bit for bit
    assert out.depth_shift.dtype == np.float32
    ref, src, mask = VR.merge_inputs(dr, m, out.depth_shift, VC.PUSH)
    assert _same_bits(out.depth_ref, ref) and _same_bits(out.depth_src, src) and _same_bits(out.mask, mask)
    assert _same_bits(out.depth_ref, gold[f"merge_{name}_depth_ref"])                  # depth_ref does not depend on the alignment
    # device tensors in -> device tensors out, the same bits; and the device sample list handed to align_depth_global in place
    t = prepare_depth_merge(torch.from_numpy(dr).to(DEV), torch.from_numpy(m).to(DEV), torch.from_numpy(de).to(DEV), VC.PUSH,
                            rng=random.Random(seed))
    assert all(isinstance(a, torch.Tensor) and a.is_cuda for a in t[2:]) and (t.scale, t.shift) == (out.scale, out.shift)
    for a, b in zip(t[2:], out[2:]):
        assert _same_bits(a, b)
    if name != "empty":
        assert t.pixel_sample.dtype == torch.int32
        s_dev = align_depth_global(dr, de, t.pixel_sample, push_depth=VC.PUSH)
        s_host = align_depth_global(dr, de, [tuple(p) for p in out.pixel_sample.tolist()], push_depth=VC.PUSH)
        assert s_dev[:2] == s_host[:2] == (out.scale, out.shift) and _same_bits(s_dev[2], s_host[2]) and _same_bits(s_dev[2], out.depth_shift)


# ---- 3: after the merge network -----------------------------------------------------------------------------------------------------------
def test_view_finish_kernel_matches_the_excerpts(gold):
    from text2nerf_amd import _lib
    from text2nerf_amd.warp import _known32, _view_finish
    dm, img, m = VC.finish_inputs()
    dev = torch.device(DEV)
    d, i, k = _view_finish(_lib.load(), dev, torch.from_numpy(dm).to(dev), torch.from_numpy(img).to(dev), _known32(m, dev), VC.PUSH)
    assert _same_bits(d, gold["finish_depth_new"]) and _same_bits(i, gold["finish_img_new"])
    assert k.dtype == torch.int64 and np.array_equal(k.cpu().numpy(), gold["finish_mask_inpainted"])
    r = VR.finish(dm, img, m, VC.PUSH)
    assert _same_bits(d, r[0]) and _same_bits(i, r[1]) and np.array_equal(k.cpu().numpy(), r[2])


@pytest.fixture(scope="module")
def finished():
    """finish_view on the support-set scene (40 x 56, nine support poses), with and without a training set, and its inputs."""
    from text2nerf_amd import DeviceTrainSet
    from text2nerf_amd.warp import finish_view
    rgb, depth, poses, intrinsic, mask_inp = support_inputs(H, W, 61, 62)
    my_map = 1 - mask_inp
    dm = ((depth - np.float32(VC.PUSH)) * np.float32(12000) / np.float32(32768) - np.float32(1)).astype(np.float32)
    img = np.rint(rgb * 255).astype(np.uint8)
    g = np.random.Generator(np.random.PCG64(77))
    first = [torch.from_numpy(g.uniform(0, 1, (50,) + s).astype(np.float32)) for s in ((6,), (3,), ())]
    ts = DeviceTrainSet(*first, device=DEV)
    plain = finish_view(dm.reshape(1, 1, H, W), img, my_map, VC.PUSH, poses, intrinsic, H, W)
    with_set = finish_view(torch.from_numpy(dm).to(DEV), torch.from_numpy(img).to(DEV), torch.from_numpy(my_map).to(DEV), VC.PUSH, poses,
                           intrinsic, H, W, train_set=ts)
    return dict(dm=dm, img=img, my_map=my_map, poses=poses, intrinsic=intrinsic, plain=plain, with_set=with_set, ts=ts, first=first)


def _check_splat(tag, got, ref):
    """The bounds tests/test_support_gpu.py::_check_warp holds the warped colour and depth to."""
    (img, dep), (r_img, r_dep) = [[np.asarray(a.cpu()) for a in t] for t in (got, ref)]
    print(f"{tag}: image max diff {float(np.abs(img - r_img).max()):.3e} on {float((img != r_img).mean()):.2e} of the values, "
          f"depth max rel diff {float((np.abs(dep - r_dep) / np.abs(r_dep).clip(1e-6)).max()):.3e}")
    assert np.abs(img - r_img).max() <= 1.0 / 255 + 1e-7 and (img != r_img).mean() < 1e-3
    np.testing.assert_allclose(dep.astype(np.float64), r_dep.astype(np.float64), rtol=1e-9, atol=1e-12)


def test_finish_view_stage_by_stage(finished):
    from text2nerf_amd.warp import FinishedView, build_support_set, sparse_bilateral_filtering
    f = finished
    for tag in ("plain", "with_set"):
        v = f[tag]
        assert isinstance(v, FinishedView) and all(t.is_cuda for t in (v.img_new, v.depth_new, v.mask_inpainted) + tuple(v.support))
        d0, i0, k0 = VR.finish(f["dm"], f["img"], f["my_map"], VC.PUSH)                  # pinned to the excerpts on the CPU
        photos, depths = sparse_bilateral_filtering(d0.copy(), i0.copy(), filter_size=[5, 5, 3, 3], depth_threshold=0.02, num_iter=4,
                                                    HR=False, mask=None)
        assert _same_bits(v.img_new, photos[-1]) and _same_bits(v.depth_new, depths[-1])
        assert v.mask_inpainted.dtype == torch.int64 and np.array_equal(v.mask_inpainted.cpu().numpy(), k0)
        ref = build_support_set(v.img_new, v.depth_new, v.mask_inpainted, f["poses"], f["intrinsic"], H, W)
        rows, rgbs, deps, rays_split, rgbs_split, deps_split, poses_t = v.support
        # upstream of the splat's sums: the masks (so the row count and order), the rays, the source view, the poses — exact
        assert rows.shape == ref[0].shape and torch.equal(rows, ref[0]) and torch.equal(rays_split, ref[3]) and torch.equal(poses_t, ref[6])
        assert torch.equal(rgbs_split[0], ref[4][0]) and torch.equal(deps_split[0], ref[5][0])
        assert rgbs.shape == ref[1].shape and deps.shape == ref[2].shape
        # the splat sums in arrival order: warped colour and depth at the warp's bounds
        _check_splat(f"{tag} views", (rgbs_split[1:], deps_split[1:]), (ref[4][1:], ref[5][1:]))
        _check_splat(f"{tag} rows", (rgbs, deps), (ref[1], ref[2]))
    assert f["plain"].lo is None and f["plain"].hi is None


def test_finish_view_appends_to_the_training_set(finished):
    from text2nerf_amd import DeviceTrainSet
    f = finished
    v, ts = f["with_set"], f["ts"]
    by_hand = DeviceTrainSet(*f["first"], device=DEV)
    lo, hi = by_hand.append(v.support[0], v.support[1], v.support[2])
    assert (v.lo, v.hi) == (lo, hi) == (50, 50 + v.support[0].shape[0]) and len(ts) == len(by_hand) == hi
    assert torch.equal(ts.rays, by_hand.rays) and torch.equal(ts.rgbs, by_hand.rgbs) and torch.equal(ts.depths, by_hand.depths)
    assert torch.equal(ts.rays[lo:hi], v.support[0]) and torch.equal(ts.rgbs[:50].cpu(), f["first"][1])


# ---- 4: the mask expansion ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", VC.EXPAND_CASES)
def test_mask_expand_matches_the_excerpt(gold, name):
    from text2nerf_amd import _lib
    from text2nerf_amd.warp import _expand_mask, _known32
    m = VC.expand_mask(name)
    dev = torch.device(DEV)
    eroded, ring = _expand_mask(_lib.load(), dev, _known32(m, dev))
    assert eroded.dtype == torch.int32 and ring.dtype == torch.int64 and ring.shape == m.shape + (3,)
    assert np.array_equal(eroded.cpu().numpy(), gold[f"expand_{name}_eroded"])
    assert np.array_equal(ring.cpu().numpy(), gold[f"expand_{name}_mask_ex"])


NAMES = ("output_image_warp_u8", "myMap_filt", "mask_image", "mask_inv", "mask_ex", "rgb_render", "rgb_render_", "depth_rendered")


def test_pack_with_expansion_matches_the_excerpt(gold):
    from text2nerf_amd.warp import pack_inpaint_inputs
    warp, m, rgb, depth = VC.pack_inputs()
    out = pack_inpaint_inputs(warp, m, rgb, depth, update_known_views=True)
    for k, a in zip(NAMES, out):
        g = gold[f"pack_{k}"]
        assert a.shape == g.shape and np.array_equal(a, g), k
    assert (out[1].dtype, out[4].dtype, out[7].dtype) == (np.int64, np.int64, np.float64)
    # the default is the branch that was there: the same arrays with and without the keyword
    for a, b in zip(pack_inpaint_inputs(warp, m, rgb, depth), pack_inpaint_inputs(warp, m, rgb, depth, update_known_views=False)):
        assert _same_bits(a, b)


S = 48
INTR48 = [float(S), float(S), S // 2, S // 2]
# the fields behind the forward warp's fp64 atomics (arrival order: they differ from run to run in the parent too)
SPLAT_FIELDS = ("warp_image", "warp_depth", "output_image_warp", "output_depth", "output_image_warp_u8")


@pytest.fixture(scope="module")
def scene48(tiny_params):
    """48 x 48, two known views given as frames (no field training), the suite's tiny field for the render of the new pose."""
    from tests.test_hip_parity import make_field
    from text2nerf_amd import render_views
    from text2nerf_amd.warp import build_inpaint_view
    f = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    p = [pose44(q) for q in warp_poses()]
    poses = np.stack([p[0], p[1], p[3]])
    frames = [synth.rgbd_frame(31 + v, S, S) for v in range(2)]
    kw = dict(N_samples=48, known_rgbs=np.stack([a for a, _ in frames]), known_depths=np.stack([b for _, b in frames]))
    rgb, depth = render_views(f, poses[2:3], INTR48, S, S, N_samples=48, white_bg=False)
    views = dict(expand=build_inpaint_view(f, poses, 2, S, S, INTR48, update_known_views=True, **kw),
                 off=build_inpaint_view(f, poses, 2, S, S, INTR48, update_known_views=False, **kw),
                 default=build_inpaint_view(f, poses, 2, S, S, INTR48, **kw))
    return dict(views=views, render=(rgb[0].cpu().numpy(), depth[0].cpu().numpy()))


def test_build_inpaint_view_with_the_mask_expansion(scene48):
    """Against the restatement of the executed :138 + :147-177 (pinned to the golden bit for bit in tests/test_view_stage_cpu.py),
    applied to the builder's own filled warp, the map the fill stage gives for its own warp, and the pinned render of the new pose."""
    from text2nerf_amd.warp import dibr_filter_mask2
    v = scene48["views"]["expand"]
    rgb, depth = scene48["render"]
    _, filled_map, _ = dibr_filter_mask2(v.warp_image.copy(), v.myMap.copy(), output_depth=v.warp_depth.copy())
    ref = VR.pack_expanded(v.output_image_warp, filled_map, rgb, depth)
    print("coverage", float(v.myMap.mean()), "filled", float(filled_map.mean()), "eroded", float(v.myMap_filt.mean()))
    assert 0 < v.myMap_filt.sum() < filled_map.sum()
    for k, r in ref.items():
        got = getattr(v, k)
        assert got.dtype == r.dtype and got.shape == r.shape and np.array_equal(got, r), k
    assert v.output_image is v.rgb_render and np.array_equal(v.mask_ex[..., 0], filled_map - v.myMap_filt)


def test_build_inpaint_view_default_is_unchanged(scene48):
    """update_known_views=False against the call without the keyword: every field that does not pass through the forward warp's
    arrival-order sums is bit-equal; those that do (they vary between two runs of the parent as well) are held at the warp's bounds, and
    each call's packed arrays are exactly the update_known_views=False arithmetic of its own warp."""
    from tests.test_inpaint_view_gpu import _check_pack, _check_warp
    off, default = scene48["views"]["off"], scene48["views"]["default"]
    rgb, depth = scene48["render"]
    for name in off._fields:
        a, b = getattr(off, name), getattr(default, name)
        assert a.dtype == b.dtype and a.shape == b.shape, name
        if name not in SPLAT_FIELDS:
            assert _same_bits(a, b), name
    _check_warp(off.myMap, off.warp_image, off.warp_depth, default.myMap, default.warp_image, default.warp_depth)
    _check_warp(off.myMap_filt, off.output_image_warp, off.output_depth, default.myMap_filt, default.output_image_warp, default.output_depth)
    for v in (off, default):
        _check_pack(v, v.output_image_warp, v.myMap_filt, rgb, depth)
        assert np.array_equal(v.mask_ex[..., 0], v.myMap_filt)
