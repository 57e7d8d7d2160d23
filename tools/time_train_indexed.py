#!/usr/bin/env python3
"""Three ways to feed the fused train step, timed in one process on bench.py's field and a C3-shaped training set (9 x 512^2 rows):

  (a) host tensors, BatchPrefetcher -> train_step          the fast path so far: gather thread, 11 R + 32 words over the link
  (b) device tensors, index_select -> train_step           what a build_support_set user gets without the indexed step (unpipelined)
  (c) DeviceTrainSet, host ids -> train_step_indexed        2 R + 32 words over the link, the step gathers its batch

The legs alternate within each block round; every block starts from the same parameters with a fresh optimiser and its own warm-up,
as bench.py's train leg does (the noisy targets turn the field into fog after ~45 steps). Per leg: ms per step (wall clock, stream
drained at the block's end), host-side ms per loop iteration (the Python thread's time in the loop, stream NOT drained), the bytes the
step stages host -> device — COMPUTED from the slot layouts, not observed; leg (b)'s device-side traffic (three index_select kernels,
four device copy_ launches into the slot, the index reads) is not in that figure — and the spread of the blocks.

`--root DIR` takes the package (and its library) from another checkout — the parent commit's build, legs a and b — so the comparison is
against the parent and not against this change's own code. (T2N_LIB alone does not do it: this package's binding asks the library for
t2n_field_set_train_source, which the parent's library does not export.) Recipe: check the parent commit out beside the tree
(`git worktree add DIR HEAD~1`), `python -m text2nerf_amd.build` there, then
`python tools/time_train_indexed.py --root DIR --legs ab --out F` followed by `python tools/time_train_indexed.py --legs abc --out F`
(--out appends).

    python tools/time_train_indexed.py [--legs abc] [--batches 16384,2048] [--blocks 5] [--iters 20] [--warmup 3] [--root DIR] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="abc")
    ap.add_argument("--batches", default="16384,2048")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--root", default=None, help="checkout whose text2nerf_amd package (and library) is measured")
    ap.add_argument("--tag", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg_root = os.path.abspath(a.root) if a.root else ROOT
    sys.path.insert(0, pkg_root)
    import numpy as np
    import torch
    import text2nerf_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(text2nerf_amd.__file__))) == pkg_root, text2nerf_amd.__file__
    sys.path.insert(1, ROOT)
    import bench                                     # build_field / reference_poses: the bench's field and poses
    from text2nerf_amd import BatchPrefetcher, synth
    from text2nerf_amd.optim import TVAdam
    if not torch.cuda.is_available():
        sys.exit("time_train_indexed.py measures on the GPU only")
    if "c" in a.legs and not hasattr(text2nerf_amd, "DeviceTrainSet"):
        sys.exit("leg c needs train_step_indexed (this package has none): --legs ab")
    dev = torch.device("cuda:0")
    torch.set_num_threads(2)                         # as bench.py's fused train leg
    field, _, _ = bench.build_field(dev)
    n_samples = min(int(1e6), int(synth.cal_n_samples([300] * 3, 1.0) / 2))
    poses = bench.reference_poses("local_fixed")
    allrays = torch.from_numpy(np.concatenate([synth.frame_rays_np(512, 512, c2w=p) for p in poses]))
    g = np.random.Generator(np.random.PCG64(1024))
    with torch.no_grad():                            # targets as bench.py makes them: the scene's own colours / depths + noise
        rgb_s, dep_s, _, _ = field(allrays[::4].to(dev), white_bg=True, is_train=False, N_samples=n_samples)
    n = allrays.shape[0]
    allrgb = (rgb_s.cpu().repeat_interleave(4, 0)[:n] + torch.from_numpy(g.normal(0, 0.05, (n, 3)).astype(np.float32))).clamp(0, 1)
    alldepth = dep_s.cpu().repeat_interleave(4, 0)[:n] + torch.from_numpy(g.normal(0, 0.05, (n,)).astype(np.float32))
    init_state = {k: v.detach().clone() for k, v in field.state_dict().items()}
    np.random.seed(1024)
    perm = torch.from_numpy(np.random.permutation(n))
    perm_d = perm.to(dev)
    rays_d, rgb_d, dep_d = allrays.to(dev), allrgb.to(dev), alldepth.to(dev)
    train_set = text2nerf_amd.DeviceTrainSet(allrays, allrgb, alldepth, device=dev) if "c" in a.legs else None
    tv_terms = [(field.density_plane, 0.1), (field.app_plane, 0.01)]
    H = 32                                            # T2N_TRAIN_HYPER_FLOATS
    lines = [f"train step feeds, {a.tag or ('package at ' + os.path.relpath(pkg_root, ROOT))}; {torch.cuda.get_device_name(0)}; {n} rows, "
             f"{n_samples} samples; {a.blocks} blocks x ({a.warmup} warm-up + {a.iters} timed steps) per leg, legs alternating; "
             f"ms per step = wall clock with the stream drained at the block's end; host ms = Python thread's loop time per step, not drained"]

    for R in [int(x) for x in a.batches.split(",")]:
        def idx_of(k):
            return perm[(k * R) % (n - R):][:R]

        def block(leg):
            torch.manual_seed(1024)
            field.load_state_dict(init_state)
            opt = TVAdam(field.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=field)
            kw = dict(N_samples=n_samples, white_bg=True, tv=tv_terms)
            pf = BatchPrefetcher([allrays, allrgb, alldepth]) if leg == "a" else None
            if pf is not None:
                pf.submit(idx_of(0))

            def it(k):
                if leg == "a":
                    b = pf.get()
                    pf.submit(idx_of(k + 1))
                    return field.train_step(b[0], b[1], b[2], opt, **kw)
                if leg == "b":
                    idx = perm_d[(k * R) % (n - R):][:R]
                    return field.train_step(rays_d.index_select(0, idx), rgb_d.index_select(0, idx), dep_d.index_select(0, idx), opt, **kw)
                return field.train_step_indexed(train_set, idx_of(k), opt, **kw)

            for k in range(a.warmup):
                it(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(a.iters):
                it(a.warmup + k)
            t_host = time.perf_counter() - t0
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            fs = field.__dict__.get("_fused_step")
            fs.sync()
            stats = (fs.pipelined_launches, fs.replays)
            if pf is not None:
                pf.get()
                pf.close()
            return dt / a.iters * 1e3, t_host / a.iters * 1e3, stats

        res = {leg: [] for leg in a.legs}
        block(a.legs[0])                              # (one untimed block: allocations, pinned buffers, first-use costs)
        for _ in range(a.blocks):
            for leg in a.legs:
                res[leg].append(block(leg))
        staged = {"a": (11 * R + H) * 4, "b": (R + H) * 4, "c": (2 * ((R + 3) // 4 * 4) + H) * 4}
        lines.append(f"R = {R}:")
        for leg in a.legs:
            ms, host = [r[0] for r in res[leg]], [r[1] for r in res[leg]]
            pip = res[leg][-1][2]
            lines.append(f"  ({leg}) {statistics.median(ms):.3f} ms per step (blocks {', '.join(f'{v:.3f}' for v in ms)}; spread "
                         f"{max(ms) - min(ms):.3f}); host {statistics.median(host):.3f} ms per step (min {min(host):.3f}, max {max(host):.3f}); "
                         f"{staged[leg]} B staged host -> device per step (computed from the slot layout" + ("; device-side gathers and copies not counted" if leg == "b" else "") + f"); pipelined launches / replays in the last block's driver: {pip[0]} / {pip[1]}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
