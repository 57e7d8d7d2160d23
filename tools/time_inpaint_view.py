#!/usr/bin/env python3
"""Time `build_inpaint_view` against the same outputs assembled from the calls that existed before it: `render_views`, a per-view
`sparse_bilateral_filtering`, `bilinear_splat_warping_multiview` (four launches per source on the interleaved canvas),
`dibr_filter_mask2`, and torch elementwise ops for the inpainter's uint8 image and masks. The benchmark's field (bench.build_field),
device tensors in and out, same box, same process, alternating blocks, warm-up excluded, device events around each call (they include
the host work between launches), median over the blocks. Checks first that both forms produce the same arrays.

    python tools/time_inpaint_view.py [--size 512] [--views 8] [--blocks 7] [--reps 3] [--stages] [--out FILE]

`--once FORM` runs one warmed call of `one` or `separate` and nothing else: the form to put behind a kernel trace."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import build_field  # noqa: E402
from text2nerf_amd import render_views, synth  # noqa: E402
from text2nerf_amd.warp import (bilinear_splat_warping_multiview, build_inpaint_view, dibr_filter_mask2,  # noqa: E402
                                sparse_bilateral_filtering, sparse_bilateral_filtering_views, warp_sources)

SCHEDULE = dict(filter_size=[7, 5, 5, 3, 3], depth_threshold=0.02, num_iter=5)


def pack_torch(img, m, rgb, depth):
    """text2nerf_main.py:138-184 (update_known_views=False) in torch elementwise ops."""
    m8 = m.to(torch.uint8)
    warp_u8 = (img * 255).to(torch.uint8) * m8[..., None]
    rgb_u8 = (rgb.clamp(0.0, 1.0) * 255).to(torch.uint8)
    return (warp_u8, m8 * 255, (1 - m8) * 255, m[..., None].expand(-1, -1, 3).contiguous(), rgb_u8,
            torch.where(m[..., None] > 0, rgb_u8, torch.full_like(rgb_u8, 255)), depth.double() * m)


def separate_calls(field, poses, V, H, W, intrinsic, n_samples):
    rgb, depth = render_views(field, poses[:V], intrinsic, H, W, N_samples=n_samples, white_bg=False)
    rgbs_pre, depths_pre = [], []
    for v in range(V):
        photos, depths = sparse_bilateral_filtering(depth[v], rgb[v], **SCHEDULE)
        rgbs_pre.append(photos[-1])
        depths_pre.append(depths[-1])
    my_map, img, dep = bilinear_splat_warping_multiview(rgbs_pre, depths_pre, poses, poses[V], H, W, intrinsic)
    img, m_filt, dep = dibr_filter_mask2(img, my_map, output_depth=dep)
    rgb_t, depth_t = render_views(field, poses[V:V + 1], intrinsic, H, W, N_samples=n_samples, white_bg=False)
    return (my_map, m_filt, img, dep) + pack_torch(img, m_filt, rgb_t[0], depth_t[0])


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def med(xs):
    return f"{statistics.median(xs):.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--samples", type=int, default=-1)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stages", action="store_true", help="also time the filter and the warp stages of both forms on their own")
    ap.add_argument("--once", choices=["one", "separate"], default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_inpaint_view.py measures on the GPU only")
    dev = torch.device("cuda:0")
    H = W = a.size
    V = a.views
    field = build_field(dev)[0]
    poses = torch.from_numpy(synth.local_fixed_like_poses(V + 1)).to(dev)
    intrinsic = [float(max(H, W)), float(max(H, W)), W // 2, H // 2]
    one = lambda: build_inpaint_view(field, poses, V, H, W, intrinsic, N_samples=a.samples)          # noqa: E731
    sep = lambda: separate_calls(field, poses, V, H, W, intrinsic, a.samples)                        # noqa: E731
    if a.once:
        fn = one if a.once == "one" else sep
        fn()
        torch.cuda.synchronize()
        fn()
        torch.cuda.synchronize()
        return
    o, s = one(), sep()
    assert torch.equal(o.myMap, s[0]) and torch.equal(o.myMap_filt, s[1]), "the two forms fill different pixels"
    assert (o.output_image_warp - s[2]).abs().max() <= 1.0 / 255 + 1e-6
    # the uint8 warp: exact from the call's own filled warp, and within a level of the other form's (its warp sums in another order)
    assert torch.equal(o.output_image_warp_u8, pack_torch(o.output_image_warp, o.myMap_filt, s[2], s[3])[0]), "output_image_warp_u8"
    assert (o.output_image_warp_u8.int() - s[4].int()).abs().max() <= 1, "output_image_warp_u8 against the separate calls"
    names = ("mask_image", "mask_inv", "mask_ex", "rgb_render", "rgb_render_", "depth_rendered")
    for k, t in zip(names, s[5:]):
        assert torch.equal(getattr(o, k), t), k
    for _ in range(2):
        one(); sep()
    t_one, t_sep = [], []
    for _ in range(a.blocks):
        t_one.append(timed(one, a.reps))
        t_sep.append(timed(sep, a.reps))
    lines = [f"build_inpaint_view vs the separate calls, {H}x{W}, {V} known views, bench field, N_samples {a.samples}; "
             f"{torch.cuda.get_device_name(0)}; median of {a.blocks} alternating blocks of {a.reps} calls, device events, warm-up excluded",
             f"whole call: build_inpaint_view {med(t_one)}; separate calls {med(t_sep)}; coverage {float(o.myMap.float().mean()):.3f} -> "
             f"{float(o.myMap_filt.float().mean()):.3f}"]
    if a.stages:
        rgb, depth = render_views(field, poses[:V], intrinsic, H, W, N_samples=a.samples, white_bg=False)
        f_one = lambda: sparse_bilateral_filtering_views(depth, rgb, **SCHEDULE)                                           # noqa: E731
        f_sep = lambda: [sparse_bilateral_filtering(depth[v], rgb[v], **SCHEDULE) for v in range(V)]                       # noqa: E731
        pre = f_one()
        w_one = lambda: warp_sources(pre[0], pre[1], poses, poses[V], H, W, intrinsic)                                     # noqa: E731
        w_sep = lambda: bilinear_splat_warping_multiview(list(pre[0]), list(pre[1]), poses, poses[V], H, W, intrinsic)    # noqa: E731
        r_all = lambda: render_views(field, poses[:V + 1], intrinsic, H, W, N_samples=a.samples, white_bg=False)          # noqa: E731
        for tag, f1, f2 in (("filter", f_one, f_sep), ("warp", w_one, w_sep)):
            f1(); f2()
            t1, t2 = [], []
            for _ in range(a.blocks):
                t1.append(timed(f1, a.reps))
                t2.append(timed(f2, a.reps))
            lines.append(f"{tag}: stack / many-sources form {med(t1)}; per-view form {med(t2)}")
        r_all()
        lines.append(f"renders ({V + 1} frames, common to both forms): {med([timed(r_all, a.reps) for _ in range(a.blocks)])}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
