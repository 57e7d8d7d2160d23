#!/usr/bin/env python3
"""Time the volume component stage (csrc/t2n_volume.hip) and what a pruned mask costs a frame. No predecessor on the device and no
target: the file records what was measured.

Volumes at n^3 (default 300): the mask volume of the bench field (bench.build_field: getDenseAlpha, then t2n_alpha_volume at the
field's alphaMask_thres) and uniform noise with a foreground probability of 0.3. For each: `t2n_volume_components`,
`t2n_volume_component_stats` (with boxes) and `t2n_volume_filter` (keeping the largest component) with device events around `reps`
calls each, beside `t2n_alpha_volume` on a volume of the same size; the achieved bytes/s of each against the least traffic the call
needs (computed from the shape: volume in + labels out = 8 B a voxel for the labelling, labels in = 4 B for the stats, volume and
labels in + volume out = 12 B for the filter, alpha in + volume out = 8 B for t2n_alpha_volume); the whole `volume.filter_volume` call
with a host clock; and `scipy.ndimage.label` on a host copy of the same array (one run, host clock; its labels - 1 are compared with
the device's at this size).

Frames: the C2 frame (800 x 800 rays of the bench field, N_samples = -1) with no mask, with an all-ones mask on the field's grid and
with the mask `prune_floaters(keep_largest=1)` attaches; warm-up frames first (the frame caches are live), then device events around
`frames` frames. Fresh process, median over the blocks.

    python tools/time_prune.py [--blocks 5] [--reps 20] [--frames 20] [--n 300] [--out profiles/prune_timing.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from text2nerf_amd import AlphaGridMask, _lib, synth, volume  # noqa: E402
from time_mesh import med, timed_device, timed_host  # noqa: E402


def rate(least_bytes, ms_list):
    return f"{least_bytes / (statistics.median(ms_list) * 1e-3) / 1e9:.1f} GB/s of least traffic"


def time_volume(lib, name, vol, a, lines):
    from scipy import ndimage
    dev = vol.device
    n0, n1, n2 = (int(s) for s in vol.shape)
    nvox = n0 * n1 * n2
    stream = _lib.current_stream_ptr(dev)
    nbytes = int(lib.t2n_volume_components_workspace_bytes(n0, n1, n2))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    labels = torch.empty((n0, n1, n2), dtype=torch.int32, device=dev)
    k_dev = torch.empty(1, dtype=torch.int64, device=dev)
    out = torch.empty_like(vol)
    for conn in (26, 6):
        def components():
            _lib.check(lib.t2n_volume_components(_lib.ptr(vol), n0, n1, n2, 0.0, conn, _lib.ptr(labels), _lib.ptr(k_dev), _lib.ptr(ws),
                                                 nbytes, stream), "t2n_volume_components")
        components()
        K = int(k_dev.cpu().item())
        counts = torch.empty(K, dtype=torch.int32, device=dev)
        boxes = torch.empty((K, 6), dtype=torch.int32, device=dev)

        def stats():
            _lib.check(lib.t2n_volume_component_stats(_lib.ptr(labels), n0, n1, n2, K, _lib.ptr(counts), _lib.ptr(boxes), stream),
                       "t2n_volume_component_stats")
        stats()
        keep = volume.keep_components(counts, 0, 1).to(torch.uint8).contiguous()

        def filt():
            _lib.check(lib.t2n_volume_filter(_lib.ptr(vol), _lib.ptr(labels), n0, n1, n2, _lib.ptr(keep), K, 0.0, _lib.ptr(out), stream),
                       "t2n_volume_filter")

        def whole():
            return volume.filter_volume(vol, keep_largest=1, connectivity=conn)
        for _ in range(2):
            components(); stats(); filt(); whole()
        t = {k: [] for k in ("components", "stats", "filter", "whole")}
        for _ in range(a.blocks):
            t["components"].append(timed_device(components, a.reps))
            t["stats"].append(timed_device(stats, a.reps))
            t["filter"].append(timed_device(filt, a.reps))
            t["whole"].append(timed_host(whole))
        components()
        host_vol = vol.cpu().numpy()
        t0 = time.perf_counter()
        ref, refK = ndimage.label(host_vol > 0, structure=ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn]))
        t_host = (time.perf_counter() - t0) * 1e3
        equal = refK == K and bool(np.array_equal(ref.astype(np.int32) - 1, labels.cpu().numpy()))
        big = counts.sort(descending=True).values[:3].tolist() if K else []
        line = (f"{name}, connectivity {conn}: {int((vol > 0).sum())} of {nvox} voxels foreground, {K} components (most voxels: {big}); "
                f"t2n_volume_components {med(t['components'])}, {rate(8 * nvox, t['components'])}; t2n_volume_component_stats with "
                f"boxes {med(t['stats'])}, {rate(4 * nvox, t['stats'])}; t2n_volume_filter (keep the largest) {med(t['filter'])}, "
                f"{rate(12 * nvox, t['filter'])}; the three together {statistics.median(t['components']) + statistics.median(t['stats']) + statistics.median(t['filter']):.3f} ms; "
                f"volume.filter_volume (allocations, K read, selection) {med(t['whole'])}; scipy.ndimage.label on the host copy "
                f"{t_host:.0f} ms (one run), labels - 1 {'equal to' if equal else 'DIFFERENT from'} the device's")
        lines.append(line)
        print(line, flush=True)


def time_frames(field, rays, a):
    field.frame_width = 800
    field.materialize_weights = False

    def one():
        with torch.no_grad():
            field(rays, N_samples=-1)
    for _ in range(40):
        one()
    ts = [timed_device(one, a.frames) for _ in range(a.blocks)]
    return med(ts), field.appearance_volume_counts(), field.density_cache_counts()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_prune.py measures on the GPU only")
    import bench
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n = a.n
    field, _, aabb = bench.build_field(dev, grid=n)
    lines = [f"volume components and floater pruning at {n}^3 (tile {volume.TILE}); {torch.cuda.get_device_name(0)}; median of {a.blocks} "
             f"blocks; kernels: device events around {a.reps} calls; filter_volume and scipy: host clock (synchronised at both ends); "
             f"frames: device events around {a.frames} frames after 40 warm-up frames; the same arrays every call, so they are read from a "
             f"warm cache hierarchy; 'least traffic' = the bytes the call must move, from the shape"]
    stream = _lib.current_stream_ptr(dev)
    alpha = field.getDenseAlpha([n, n, n])[0].contiguous()
    mask_vol = torch.empty((n, n, n), dtype=torch.float32, device=dev)
    box = torch.empty(6, dtype=torch.int32, device=dev)

    def alpha_volume():
        _lib.check(lib.t2n_alpha_volume(_lib.ptr(alpha), n, n, n, float(field.alphaMask_thres), _lib.ptr(mask_vol), _lib.ptr(box), stream),
                   "t2n_alpha_volume")
    for _ in range(2):
        alpha_volume()
    t_av = [timed_device(alpha_volume, a.reps) for _ in range(a.blocks)]
    lines.append(f"t2n_alpha_volume on the bench field's dense alpha (threshold {field.alphaMask_thres:g}): {med(t_av)}, "
                 f"{rate(8 * n ** 3, t_av)}")
    print(lines[-1], flush=True)
    time_volume(lib, "the bench field's mask volume", mask_vol, a, lines)
    rng = np.random.default_rng(7)
    noise = torch.from_numpy((rng.random((n, n, n), dtype=np.float32) < 0.3).astype(np.float32)).to(dev)
    time_volume(lib, "noise, p = 0.3", noise, a, lines)
    del noise

    rays = torch.from_numpy(synth.frame_rays_np(800, 800)).to(dev)
    t_none, av, dc = time_frames(field, rays, a)
    lines.append(f"C2 frame (800 x 800 rays, N_samples = {field.nSamples}), no mask: {t_none}; feature-volume frames {av['volume']}, "
                 f"cached-density frames {dc['cached']}")
    field.alphaMask = AlphaGridMask(dev, torch.tensor(aabb), torch.ones((n, n, n), device=dev))
    t_ones, _, _ = time_frames(field, rays, a)
    lines.append(f"C2 frame, all-ones mask on the field's grid: {t_ones}")
    field.alphaMask = None
    rep = field.prune_floaters(keep_largest=1)
    kept = int(rep.voxel_counts[rep.keep].sum())
    t_pruned, _, _ = time_frames(field, rays, a)
    lines.append(f"C2 frame, mask of prune_floaters(keep_largest=1) ({rep.n_components} components, {kept} voxels kept, "
                 f"{rep.removed_voxels} removed): {t_pruned}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
