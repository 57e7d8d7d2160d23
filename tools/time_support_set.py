#!/usr/bin/env python3
"""Time `build_support_set` against the same outputs assembled from the calls that existed before it: 2 x V single-source
`bilinear_splat_warping_multiview` calls (unmasked colour + depth, masked coverage), `generate_rays` per view and torch boolean
indexing. Same box, same process, alternating blocks, warm-up excluded, device events around each call (they include the host work
between launches), median over the blocks. Checks first that both paths select the same rows.

    python tools/time_support_set.py [--size 512] [--views 8] [--blocks 9] [--reps 5] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from text2nerf_amd import generate_rays, synth  # noqa: E402
from text2nerf_amd.warp import bilinear_splat_warping_multiview, build_support_set  # noqa: E402


def separate_calls(rgb, depth, mask, poses, intrinsic, H, W, dev):
    """The support set from the single-target warp, per-view ray generation and boolean indexing; device tensors out."""
    images, depths, masks = [torch.as_tensor(rgb, device=dev)], [torch.as_tensor(depth, device=dev)], [torch.as_tensor(mask, device=dev)]
    for v in range(1, poses.shape[0]):
        _, img, dep = bilinear_splat_warping_multiview([rgb], [depth], poses[:1], poses[v], H, W, intrinsic, device=dev)
        cov, _, _ = bilinear_splat_warping_multiview([rgb], [depth], poses[:1], poses[v], H, W, intrinsic, masks=[mask], device=dev)
        images.append(torch.as_tensor(img, device=dev))
        depths.append(torch.as_tensor(dep, device=dev).float())
        masks.append(torch.as_tensor(cov, device=dev))
    rays_split = torch.stack([generate_rays(H, W, intrinsic, poses[i], device=dev) for i in range(poses.shape[0])])
    images, depths, keep = torch.stack(images), torch.stack(depths), torch.stack(masks).reshape(poses.shape[0], -1) > 0.5
    return (rays_split[keep], images.reshape(poses.shape[0], -1, 3)[keep], depths.reshape(poses.shape[0], -1)[keep], rays_split, images,
            depths, torch.as_tensor(poses, device=dev))


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_support_set.py measures on the GPU only")
    dev = torch.device("cuda:0")
    H = W = a.size
    rgb, depth = synth.rgbd_frame(101, H, W, n_boxes=6)
    poses = synth.local_fixed_like_poses(1 + a.views)
    intrinsic = [float(max(H, W)), float(max(H, W)), W // 2, H // 2]
    mask = np.zeros((H, W), np.int64)
    mask[:, 2 * W // 3:] = 1
    mask[np.random.Generator(np.random.PCG64(102)).uniform(0, 1, (H, W)) > 0.9] = 1
    t_in = [torch.from_numpy(x).to(dev) for x in (rgb, depth, mask)]
    forms = {"device tensors in": t_in, "numpy arrays in": [rgb, depth, mask]}
    lines = [f"build_support_set vs the separate calls, {H}x{W}, {a.views} targets; {torch.cuda.get_device_name(0)}; "
             f"median of {a.blocks} alternating blocks of {a.reps} calls, device events, warm-up excluded"]
    for tag, (r, d, m) in forms.items():
        one = lambda: build_support_set(r, d, m, poses, intrinsic, H, W, device=dev)                 # noqa: E731
        sep = lambda: separate_calls(r, d, m, poses, intrinsic, H, W, dev)                           # noqa: E731
        o, s = one(), sep()
        assert o[0].shape == s[0].shape and torch.equal(o[0], s[0]), "the two paths select different rows"
        assert (o[1] - s[1]).abs().max() <= 1.0 / 255 + 1e-7
        for _ in range(2):
            one(); sep()
        t_one, t_sep = [], []
        for _ in range(a.blocks):
            t_one.append(timed(one, a.reps))
            t_sep.append(timed(sep, a.reps))
        lines.append(f"{tag}: build_support_set {statistics.median(t_one):.3f} ms (min {min(t_one):.3f}, max {max(t_one):.3f}); "
                     f"separate calls {statistics.median(t_sep):.3f} ms (min {min(t_sep):.3f}, max {max(t_sep):.3f}); "
                     f"K = {o[0].shape[0]} of {(1 + a.views) * H * W} rows")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
