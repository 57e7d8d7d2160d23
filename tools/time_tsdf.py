#!/usr/bin/env python3
"""Time the TSDF export (csrc/t2n_tsdf.hip, text2nerf_amd/tsdf.py) on the bench field. There is no predecessor on the device and no
target: the file records what was measured and what bounds the integration kernel.

The bench field (bench.build_field) on its own n^3 grid (default 300), `views` poses (default 40) of `size`^2 pixels (default 512) on a
ring of radius 5 around the box's centre, looking at it. Medians of `blocks` blocks (default 3):
  - the view renders (per pose generate_rays, render_geometry's median depth and accumulated weight, forward's rgb): device events around
    the loop over all poses;
  - `t2n_tsdf_integrate` alone on the rendered stacks (state with colour: 20 B a node read and 20 B written), device events around `reps`
    calls, for all views in one call, for ONE view, and for all views without colour; the state bytes computed from the shape over the
    time; the slope per view between the two says whether the views' arithmetic or the state stream bounds the call;
  - `tsdf_mesh` of the fused volume and the whole `tensorf.tsdf_volume`, host clock, synchronised at both ends;
  - `t2n_alpha_volume` on the same grid in the same run: the yardstick of profiles/prune_timing.txt (4.2 ms there).

    python tools/time_tsdf.py [--blocks 3] [--reps 3] [--n 300] [--views 40] [--size 512] [--out profiles/tsdf_timing.txt]"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from text2nerf_amd import _lib, generate_rays, synth, tsdf  # noqa: E402
from time_mesh import med, timed_device, timed_host  # noqa: E402


def ring_poses(n, radius=5.0):
    return np.stack([synth.look_pose(a, 0.0, (-radius * math.sin(a), 0.0, -radius * math.cos(a)))
                     for a in (2 * math.pi * k / n for k in range(n))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--views", type=int, default=40)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_tsdf.py measures on the GPU only")
    import bench
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n, V, H = a.n, a.views, a.size
    W = H
    field, _, aabb = bench.build_field(dev, grid=n)
    poses = ring_poses(V)
    intr = (float(H), float(H), H / 2.0, H / 2.0)
    far = float(field.near_far[1])
    lines = [f"TSDF export of the bench field at {n}^3 from {V} poses of {H} x {W}; {torch.cuda.get_device_name(0)}; median of {a.blocks} "
             f"blocks; kernels: device events around {a.reps} calls; renders: device events around the loop over the poses; tsdf_mesh and "
             f"tsdf_volume: host clock (synchronised at both ends). No predecessor on the device and no target."]

    depth = torch.empty(V, H, W, device=dev)
    rgb = torch.empty(V, H, W, 3, device=dev)

    def renders():
        with torch.no_grad():
            for v, c2w in enumerate(poses):
                rays = generate_rays(H, W, intr, c2w, device=dev)
                geo = field.render_geometry(rays, want=("median",))
                depth[v] = torch.where(geo.acc >= 0.5, geo.depth_median, torch.full_like(geo.acc, far)).reshape(H, W)
                rgb[v] = field(rays, white_bg=True, is_train=False, frame_width=W)[0].reshape(H, W, 3)
    renders()
    t_r = [timed_device(renders, 1) for _ in range(a.blocks)]
    hit = float((depth < far).float().mean())
    lines.append(f"view renders (generate_rays + render_geometry + forward, {V} poses): {med(t_r)}, "
                 f"{statistics.median(t_r) / V:.3f} ms a pose; {100 * hit:.1f} % of the pixels reach an accumulated weight of 0.5")
    print(lines[-1], flush=True)

    a32 = torch.tensor(aabb, dtype=torch.float32)
    spacing = ((a32[1] - a32[0]) / (n - 1)).tolist()
    origin = a32[0].tolist()
    trunc = 4.0 * max(spacing)
    mats = torch.from_numpy(tsdf.world_to_camera(poses)).to(dev)
    T = torch.ones(n, n, n, device=dev)
    Wt = torch.zeros(n, n, n, device=dev)
    Cl = torch.zeros(n, n, n, 3, device=dev)
    stream = _lib.current_stream_ptr(dev)
    o3, s3 = (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing)

    def integrate(nv, color):
        def fn():
            _lib.check(lib.t2n_tsdf_integrate(_lib.ptr(T), _lib.ptr(Wt), _lib.ptr(Cl) if color else None, n, n, n, _lib.ptr(depth),
                                              _lib.ptr(rgb) if color else None, None, _lib.ptr(mats), nv, H, W, *intr, o3, s3, trunc, 0.0,
                                              math.inf, 0, stream), "t2n_tsdf_integrate")
        return fn
    nodes = n ** 3
    res = {}
    for name, nv, color in (("all views, colour", V, True), ("one view, colour", 1, True), ("all views, no colour", V, False)):
        fn = integrate(nv, color)
        fn()
        ts = [timed_device(fn, a.reps) for _ in range(a.blocks)]
        res[name] = statistics.median(ts)
        state = nodes * (40 if color else 16)                   # tsdf + weight (+ 3 colour floats), read and written
        lines.append(f"t2n_tsdf_integrate, {name} ({nv} x {nodes} node-views): {med(ts)}; state bytes {state / 1e9:.3f} GB (from the shape, "
                     f"every node read and written) over the time: {state / (res[name] * 1e-3) / 1e9:.1f} GB/s; "
                     f"{nv * nodes / (res[name] * 1e-3) / 1e9:.2f} G node-views/s")
        print(lines[-1], flush=True)
    observed = int((Wt > 0).sum())
    if V > 1:
        slope = (res["all views, colour"] - res["one view, colour"]) / (V - 1)
        lines.append(f"per further view {slope:.3f} ms against {res['one view, colour']:.3f} ms for the call with one view (the state stream plus "
                     f"one view): {'the views arithmetic (float64 divides, sqrt)' if slope * V > 2 * res['one view, colour'] else 'the state stream'} "
                     f"bounds the {V}-view call; {observed} of {nodes} nodes observed")
        print(lines[-1], flush=True)

    vol = tsdf.tsdf_integrate(depth, poses, intr, origin, spacing, (n, n, n), trunc, colors=rgb)
    mesh = tsdf.tsdf_mesh(vol)
    t_m = [timed_host(lambda: tsdf.tsdf_mesh(vol)) for _ in range(a.blocks)]
    lines.append(f"tsdf_mesh (marching cubes, face flags, selection, colours, vertex normals): {med(t_m)}; {mesh.verts.shape[0]} vertices, "
                 f"{mesh.faces.shape[0]} faces")
    print(lines[-1], flush=True)
    del vol, mesh
    t_v = [timed_host(lambda: field.tsdf_volume(poses, intr, H, W)) for _ in range(a.blocks)]
    lines.append(f"tensorf.tsdf_volume (renders in chunks of {field.TSDF_VIEW_CHUNK} views, integration, allocations): {med(t_v)}")
    print(lines[-1], flush=True)

    alpha = field.getDenseAlpha([n, n, n])[0].contiguous()
    mask_vol = torch.empty((n, n, n), dtype=torch.float32, device=dev)
    box = torch.empty(6, dtype=torch.int32, device=dev)

    def alpha_volume():
        _lib.check(lib.t2n_alpha_volume(_lib.ptr(alpha), n, n, n, float(field.alphaMask_thres), _lib.ptr(mask_vol), _lib.ptr(box), stream),
                   "t2n_alpha_volume")
    alpha_volume()
    t_av = [timed_device(alpha_volume, 20) for _ in range(a.blocks)]
    lines.append(f"t2n_alpha_volume on the same grid, same run (the yardstick of profiles/prune_timing.txt): {med(t_av)}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
