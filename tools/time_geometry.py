#!/usr/bin/env python3
"""Time t2n_render_geometry (csrc/t2n_geometry.hip) beside the render of the same frame, in one process:

  C2 frame     bench.py's field (300^3, S1-soft, seed 0), one 800 x 800 view, N = 518: render_geometry with all outputs and with
               depth_median alone, beside render_views of the same pose
  pipeline     the same field, one 512 x 512 view at N = 259 (the size the view pipeline renders at)

Each leg is warmed up once (the render's caches are built by its first frames: three warm-up frames), then timed with device events
around `reps` calls; the legs alternate inside a block and the medians of `blocks` blocks are reported with their spread. The rays
are generated once, outside the timed region, for the geometry legs; render_views generates its own (that is what it does). No
threshold and no predecessor: the numbers are a report.

    python tools/time_geometry.py [--blocks 3] [--reps 50] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import bench                                     # build_field: the bench's field
    from text2nerf_amd import generate_rays, render_views, synth
    if not torch.cuda.is_available():
        sys.exit("time_geometry.py measures on the GPU only")
    dev = torch.device("cuda:0")
    field = bench.build_field(dev)[0]
    pose = synth.look_pose()
    lines = [f"geometry outputs, {torch.cuda.get_device_name(0)}; median of {a.blocks} blocks, legs alternating within a block; device events "
             f"around {a.reps} calls after the warm-up calls of each leg",
             "the render_geometry legs take rays generated once, outside the timed region; render_views generates its own inside it, so "
             "the 'x render_views' column compares a march alone with ray generation + march + shading"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, H, W, N in (("C2 frame", 800, 800, 518), ("pipeline view", 512, 512, 259)):
        f = float(max(H, W))
        intr = [f, f, W // 2, H // 2]
        rays = generate_rays(H, W, intr, pose, device=dev)
        legs = {
            "render_views (rgb + depth)": lambda: render_views(field, [pose], intr, H, W, N_samples=N),
            "render_geometry, all outputs": lambda: field.render_geometry(rays, N_samples=N),
            "render_geometry, depth_median alone": lambda: field.render_geometry(rays, N_samples=N, want=("median",)),
        }
        res = {k: [] for k in legs}
        for fn in legs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.blocks):
            for k, fn in legs.items():
                fn()
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                e1.synchronize()
                res[k].append(e0.elapsed_time(e1) / a.reps)
        g = field.render_geometry(rays, N_samples=N)
        lines.append(f"{name}: {H} x {W} rays x {N} samples (mean acc {float(g.acc.mean()):.3f}, share of rays whose weight reaches the "
                     f"quantile 0.5: {float((g.acc >= 0.5).float().mean()):.3f}):")
        base = statistics.median(res["render_views (rgb + depth)"])
        for k, ms in res.items():
            lines.append(f"  {k:38s} {statistics.median(ms):7.3f} ms per frame (blocks {', '.join(f'{v:.3f}' for v in ms)}; spread "
                         f"{max(ms) - min(ms):.3f}) = {statistics.median(ms) / base:.2f} x render_views")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
