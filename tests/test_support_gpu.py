"""The support-set builder on the MI355X (csrc/t2n_support.hip through text2nerf_amd.warp): `gt_warping`, `produce_formatted_data`
and `build_support_set` against the reference's goldens (tests/golden/support.npz), the CPU restatement pinned to them
(tests/helpers/support_ref.py) and the existing single-target warp. Bounds for the warp are those tests/test_hip_warp.py::_check_warp
applies to the same arithmetic (fp64 atomics sum in another order than numpy's add.at): masks exact, image within one uint8 level on
fewer than 1e-3 of the values, depth rtol 1e-9 / atol 1e-12. The formatter copies and selects: bit-equal."""
import os
import sys

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN
from tests.helpers import support_ref as SR

sys.path.insert(0, GOLDEN)
from make_golden_support_cases import H, W, support_inputs  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gs():
    return dict(np.load(os.path.join(GOLDEN, "support.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def big():
    """192 x 256 inputs and the CPU restatement's support set for them (masked form)."""
    h, w = 192, 256
    rgb, depth, poses, intrinsic, mask = support_inputs(h, w, 81, 82, n_boxes=5)
    u = SR.gt_warping(rgb, depth, poses[0], poses[1:], h, w, intrinsic)
    m = SR.gt_warping(rgb, depth, poses[0], poses[1:], h, w, intrinsic, mask_gt=mask)
    return dict(h=h, w=w, rgb=rgb, depth=depth, poses=poses, intrinsic=intrinsic, mask=mask, unmasked=u, masked=m)


def _img(u8):
    return (u8 / 255).astype(np.float32)


def _check_warp(tag, got, ref):
    (img, mask, dep), (r_img, r_mask, r_dep) = [[np.asarray(a) for a in t] for t in (got, ref)]
    assert img.dtype == np.float32 and mask.dtype == np.int64 and dep.dtype == np.float64
    assert img.shape == r_img.shape and mask.shape == r_mask.shape and dep.shape == r_dep.shape
    print(f"{tag}: mask diffs {int((mask != r_mask).sum())}, image max diff {float(np.abs(img - r_img).max()):.3e} on "
          f"{float((img != r_img).mean()):.2e} of the values, depth max abs diff {float(np.abs(dep - r_dep).max()):.3e}")
    assert np.array_equal(mask, r_mask)
    assert np.abs(img - r_img).max() <= 1.0 / 255 + 1e-7 and (img != r_img).mean() < 1e-3
    np.testing.assert_allclose(dep, r_dep, rtol=1e-9, atol=1e-12)


def test_gt_warping_vs_reference_golden(gs):
    from text2nerf_amd.warp import gt_warping
    rgb, depth, poses, intrinsic, mask = support_inputs(H, W, 61, 62)
    for tag, m in (("unmasked", None), ("masked", mask)):
        ref = (_img(gs[f"{tag}_rgb_u8"]), gs[f"{tag}_mask"].astype(np.int64), gs[f"{tag}_depth"])
        out = gt_warping(rgb, depth, poses[0], poses[1:], H, W, intrinsic, mask_gt=m, warp_depth=True, bilinear_splat=True)
        assert all(isinstance(a, np.ndarray) for a in out) and out[0].shape == (8, H, W, 3) and out[1].shape == (8, H, W)
        _check_warp(f"golden {tag} numpy", out, ref)
        dev = torch.device("cuda:0")
        t_out = gt_warping(torch.from_numpy(rgb).to(dev), torch.from_numpy(depth).to(dev), poses[0], poses[1:], H, W, intrinsic,
                           mask_gt=None if m is None else torch.from_numpy(m).to(dev), warp_depth=True, bilinear_splat=True)
        assert all(isinstance(a, torch.Tensor) and a.is_cuda for a in t_out)
        assert (t_out[0].dtype, t_out[1].dtype, t_out[2].dtype) == (torch.float32, torch.int64, torch.float64)
        _check_warp(f"golden {tag} tensor", [a.cpu().numpy() for a in t_out], ref)
    two = gt_warping(rgb, depth, poses[0], poses[1:], H, W, intrinsic, bilinear_splat=True)
    assert len(two) == 2 and np.array_equal(two[1], gs["unmasked_mask"])


def test_gt_warping_192x256_vs_cpu_restatement(big):
    from text2nerf_amd.warp import gt_warping
    b = big
    for tag, m in (("unmasked", None), ("masked", b["mask"])):
        out = gt_warping(b["rgb"], b["depth"], b["poses"][0], b["poses"][1:], b["h"], b["w"], b["intrinsic"], mask_gt=m,
                         warp_depth=True, bilinear_splat=True)
        _check_warp(f"192x256 {tag}", out, b[tag])
        fill = out[1].mean((1, 2))
        print(tag, "fill", fill.round(3).tolist())
        assert (0.85 < fill.min() and fill.max() < 0.99) if m is None else (0.38 < fill.min() and fill.max() < 0.55)


def test_gt_warping_logpath_writes_the_reference_layout(tmp_path):
    from text2nerf_amd.warp import gt_warping
    rgb, depth, poses, intrinsic, _ = support_inputs(H, W, 61, 62)
    gt_warping(rgb, depth, poses[0], poses[1:3], H, W, intrinsic, logpath=str(tmp_path), warp_depth=True, bilinear_splat=True)
    for sub in ("warped", "mask", "mask_inv", "warped_depth"):
        assert sorted(os.listdir(tmp_path / "DIBR_gt" / sub)) == ["00001.png", "00002.png"]


def test_gt_warping_agrees_with_the_single_target_warp():
    from text2nerf_amd.warp import bilinear_splat_warping_multiview, gt_warping
    rgb, depth, poses, intrinsic, mask = support_inputs(H, W, 61, 62)
    for m in (None, mask):
        rgbs, masks, deps = gt_warping(rgb, depth, poses[0], poses[1:], H, W, intrinsic, mask_gt=m, warp_depth=True, bilinear_splat=True)
        for v in range(8):
            one = bilinear_splat_warping_multiview([rgb], [depth], poses[:1], poses[1 + v], H, W, intrinsic,
                                                   masks=None if m is None else [m])
            _check_warp(f"view {v}", (rgbs[v], masks[v], deps[v]), (one[1], one[0], one[2]))


def _golden_views(gs):
    rgb, depth, poses, intrinsic, mask = support_inputs(H, W, 61, 62)
    images = np.concatenate([rgb[None], _img(gs["unmasked_rgb_u8"])], 0)
    depths = np.concatenate([depth[None], gs["unmasked_depth"]], 0)
    masks = np.concatenate([mask[None], gs["masked_mask"].astype(np.int64)], 0)
    return images, depths, masks, poses, intrinsic


def test_produce_formatted_data_vs_reference_golden(gs):
    from text2nerf_amd import generate_rays
    from text2nerf_amd.warp import produce_formatted_data
    images, depths, masks, poses, intrinsic = _golden_views(gs)
    out = produce_formatted_data(images, depths, masks, poses, intrinsic, H, W, mode="train")
    assert len(out) == 7 and all(isinstance(t, torch.Tensor) and not t.is_cuda and t.dtype == torch.float32 for t in out)
    rays, rgbs, deps, rays_split, rgbs_split, deps_split, poses_t = [t.numpy() for t in out]
    keep = masks.reshape(9, -1) > 0.5
    assert rays.shape == (10257, 6) and rgbs.shape == (10257, 3) and deps.shape == (10257,) and int(keep.sum()) == 10257
    assert rays_split.shape == (9, H * W, 6) and rgbs_split.shape == (9, H, W, 3) and deps_split.shape == (9, H, W)
    assert poses_t.shape == (9, 4, 4) and np.array_equal(poses_t, gs["poses_tensor"])
    assert np.array_equal(rgbs, gs["all_rgbs"]) and np.array_equal(deps, gs["all_depths"])
    print("all_rays max diff vs golden", float(np.abs(rays - gs["all_rays"]).max()))
    assert np.abs(rays - gs["all_rays"]).max() <= 3e-7 and np.abs(rays_split - gs["all_rays_split"]).max() <= 3e-7
    assert np.array_equal(rays, rays_split[keep])
    assert np.array_equal(rgbs_split, images) and np.array_equal(deps_split, depths.astype(np.float32))
    for i in range(9):
        assert np.array_equal(rays_split[i], generate_rays(H, W, intrinsic, poses[i]).cpu().numpy())
    # device tensors in -> device tensors out, with the same rows; masks in the dtypes a driver may hold them in
    dev = torch.device("cuda:0")
    for mk in (torch.from_numpy(masks), torch.from_numpy(masks.astype(np.float32)) * 0.75, torch.from_numpy(masks > 0),
               torch.from_numpy(masks.astype(np.uint8)), torch.from_numpy(masks.astype(np.int32)), torch.from_numpy(masks.astype(np.float64))):
        t_out = produce_formatted_data(torch.from_numpy(images).to(dev), torch.from_numpy(depths.astype(np.float32)).to(dev), mk.to(dev),
                                       poses, intrinsic, H, W)
        assert all(t.is_cuda for t in t_out)
        for a, b in zip(t_out[:4], (rays, rgbs, deps, rays_split)):
            assert np.array_equal(a.cpu().numpy(), b)
    test = produce_formatted_data(None, None, None, poses, intrinsic, H, W, mode="test")
    assert len(test) == 2 and np.array_equal(test[0].numpy(), rays_split) and np.array_equal(test[1].numpy(), poses_t)


@pytest.mark.parametrize("h,w", [(37, 53), (16, 16)])
def test_produce_formatted_data_empty_full_and_ragged(h, w):
    from text2nerf_amd.warp import produce_formatted_data
    rgb, depth, poses, intrinsic, mask = support_inputs(h, w, 91, 92)
    g = np.random.Generator(np.random.PCG64(93))
    images = g.uniform(0, 1, (3, h, w, 3)).astype(np.float32)
    depths = g.uniform(1, 5, (3, h, w)).astype(np.float32)
    for masks in (np.zeros((3, h, w), np.int64),                                               # K = 0
                  np.stack([np.zeros((h, w), np.int64), np.ones((h, w), np.int64), mask]),      # one empty, one full, one mixed
                  (g.uniform(0, 1, (3, h, w)) > 0.5).astype(np.int64)):
        out = produce_formatted_data(images, depths, masks, poses[:3], intrinsic, h, w)
        ref = SR.produce_formatted_data(images, depths, masks, poses[:3], intrinsic, h, w)
        assert out[0].shape == ref[0].shape == (int(masks.sum()), 6)
        assert torch.equal(out[1], ref[1]) and torch.equal(out[2], ref[2])
        keep = torch.from_numpy(masks.reshape(3, -1) > 0.5)
        assert torch.equal(out[0], out[3][keep]) and (out[3] - ref[3]).abs().max() <= 3e-7


def test_build_support_set_initial_view_form(gs):
    from text2nerf_amd.warp import build_support_set
    rgb, depth, poses, intrinsic, _ = support_inputs(H, W, 61, 62)
    out = build_support_set(rgb, depth, None, poses, intrinsic, H, W)
    assert len(out) == 7 and all(t.is_cuda and t.dtype == torch.float32 for t in out)
    counts = [H * W] + [int(m.sum()) for m in gs["unmasked_mask"]]
    assert out[0].shape == (sum(counts), 6) and out[1].shape == (sum(counts), 3) and out[2].shape == (sum(counts),)
    rays_split = out[3].cpu()
    assert torch.equal(out[0][:H * W].cpu(), rays_split[0])                    # the source view keeps every pixel
    edges = np.cumsum([0] + counts)
    for v in range(1, 9):                                                      # each warp keeps its own coverage, in raster order
        keep = torch.from_numpy(gs["unmasked_mask"][v - 1].reshape(-1) > 0)
        assert torch.equal(out[0][edges[v]:edges[v + 1]].cpu(), rays_split[v][keep])


def test_build_support_set_192x256_vs_cpu_restatement(big):
    """Counts, order and masks exact; rows within the warp's bounds. The rows' depth is the fp64 warp depth rounded to float32 and is
    held to the fp64 bound (rtol 1e-9) all the same: it differs only if an fp64 sum that moved by ~1e-15 sits on a float32 rounding
    boundary (about 2e-8 per value)."""
    from text2nerf_amd.warp import build_support_set
    b = big
    h, w = b["h"], b["w"]
    images = np.concatenate([b["rgb"][None], b["unmasked"][0]], 0)
    depths = np.concatenate([b["depth"][None], b["unmasked"][2]], 0)
    masks = np.concatenate([b["mask"][None], b["masked"][1]], 0)
    ref = SR.produce_formatted_data(images, depths, masks, b["poses"], b["intrinsic"], h, w)
    runs = [build_support_set(b["rgb"], b["depth"], b["mask"], b["poses"], b["intrinsic"], h, w) for _ in range(2)]
    keep = torch.from_numpy(masks.reshape(9, -1) > 0.5)
    for out in runs:
        rays, rgbs, deps, rays_split, rgbs_split, deps_split, poses_t = [t.cpu() for t in out]
        assert rays.shape == ref[0].shape and rgbs.shape == ref[1].shape and deps.shape == ref[2].shape       # K exact (masks are)
        assert torch.equal(rays, rays_split[keep]) and (rays - ref[0]).abs().max() <= 3e-7                    # same pixels, same order
        assert torch.equal(rgbs, rgbs_split.reshape(9, -1, 3)[keep]) and torch.equal(deps, deps_split.reshape(9, -1)[keep])
        _check_warp("support set", (rgbs_split[1:].numpy(), masks[1:], deps_split[1:].numpy().astype(np.float64)),
                    (images[1:], masks[1:], depths[1:].astype(np.float32).astype(np.float64)))
        assert torch.equal(rgbs_split[0], torch.from_numpy(b["rgb"])) and torch.equal(deps_split[0], torch.from_numpy(b["depth"]))
        d = (rgbs - ref[1]).abs()
        print("rows: rgb max diff", float(d.max()), "on", float((d > 0).float().mean()), "depth max rel diff",
              float(((deps - ref[2]).abs() / ref[2].abs().clamp_min(1e-6)).max()))
        assert d.max() <= 1.0 / 255 + 1e-7 and (d > 0).float().mean() < 1e-3
        np.testing.assert_allclose(deps.numpy(), ref[2].numpy(), rtol=1e-9, atol=1e-12)
    assert runs[0][0].shape == runs[1][0].shape and torch.equal(runs[0][0], runs[1][0])                       # counts and order repeat


def test_support_set_on_a_side_stream():
    from text2nerf_amd.warp import build_support_set, gt_warping
    rgb, depth, poses, intrinsic, mask = support_inputs(H, W, 61, 62)
    dev = torch.device("cuda:0")
    base = build_support_set(rgb, depth, mask, poses, intrinsic, H, W)
    base_warp = gt_warping(rgb, depth, poses[0], poses[1:], H, W, intrinsic, bilinear_splat=True)
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        t_rgb, t_depth, t_mask = [torch.from_numpy(a).to(dev) for a in (rgb, depth, mask)]
        out = build_support_set(t_rgb, t_depth, t_mask, poses, intrinsic, H, W)
        total = out[0].sum() + out[1].sum() + out[2].sum()              # consumed on the same stream
        warp = gt_warping(t_rgb, t_depth, poses[0], poses[1:], H, W, intrinsic, bilinear_splat=True)
        covered = warp[1].sum()
    s.synchronize()
    torch.cuda.synchronize()
    assert out[0].shape == base[0].shape and torch.equal(out[0], base[0])
    assert torch.isfinite(total) and int(covered) == int(base_warp[1].sum())
