#!/usr/bin/env python3
"""What the L1 and ortho regularisers cost the fused train step, timed in one process on bench.py's field and a C3-shaped training
set (9 x 512^2 rows), host batches through BatchPrefetcher as bench.py's train leg feeds them:

  (p) train_step without tv / l1 / ortho                       the step every existing caller runs
  (t) tv only
  (l) tv + the two L1 weights                                  the L1 term rides in the seed launch: no launch, no plane traffic added
  (a) tv + all four new weights                                + the two ortho launches behind the seed

The legs alternate within each block round; every block starts from the same parameters with a fresh optimiser and its own warm-up.
Per leg: ms per step (wall clock, stream drained at the block's end) per block, the median and the spread of the blocks. Then the
ortho launches on their own, by device events around t2n_field_reg_seed with the ortho weights alone against t2n_field_tv_seed with no
weight (both fill the gradient buffer with zeros; the difference is the Gram + gradient launches of the six lines).

The legs train: a regulariser changes where the parameters go (under Adam any non-zero gradient moves an element by a full step), and
with them the appearance rows a step has to process — bench.py's noisy targets turn the field into fog after ~45 steps, and they do
not with the L1 term on. A leg's time over 100 training steps is therefore the time of ITS trajectory. `--freeze` sets every learning
rate to 0: all legs then run the same kernels on the same parameters, and the differences between them are the terms' own cost.

`--root DIR` takes the package (and its library) from another checkout — the parent commit's build, legs p and t — so that the
keyword-free step is compared against the parent's own and not against this change's code.

    python tools/time_reg_terms.py [--legs ptla] [--batches 16384,2048] [--blocks 3] [--iters 100] [--warmup 5] [--freeze] [--root DIR] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L1_WEIGHT, ORTHO_WEIGHT = 8e-5, 1e-3          # configs/: L1_weight_inital, and an Ortho_weight of TensoRF's own order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="ptla")
    ap.add_argument("--batches", default="16384,2048")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--root", default=None, help="checkout whose text2nerf_amd package (and library) is measured")
    ap.add_argument("--freeze", action="store_true", help="learning rates 0: every leg runs the same kernels on the same, unchanging parameters")
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
    from text2nerf_amd import BatchPrefetcher, _lib, synth
    from text2nerf_amd.optim import TVAdam
    if not torch.cuda.is_available():
        sys.exit("time_reg_terms.py measures on the GPU only")
    has_reg = "t2n_field_reg_seed" in _lib.SIGNATURES
    if not has_reg and set(a.legs) - set("pt"):
        sys.exit("legs l and a need train_step(l1=, ortho=) (this package has none): --legs pt")
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
    tv = [(field.density_plane, 0.1), (field.app_plane, 0.01)]
    l1 = [(field.density_plane, L1_WEIGHT), (field.density_line, L1_WEIGHT)]
    ortho = [(field.density_line, ORTHO_WEIGHT), (field.app_line, ORTHO_WEIGHT)]
    terms = {"p": {}, "t": dict(tv=tv), "l": dict(tv=tv, l1=l1), "a": dict(tv=tv, l1=l1, ortho=ortho)}
    lines = [f"L1 / ortho regularisers on the fused train step, {a.tag or ('package at ' + os.path.relpath(pkg_root, ROOT))}; "
             f"{torch.cuda.get_device_name(0)}; {n} rows, {n_samples} samples; {a.blocks} blocks x ({a.warmup} warm-up + {a.iters} timed steps) "
             f"per leg, legs alternating; ms per step = wall clock with the stream drained at the block's end. Legs: p no tv / l1 / ortho, "
             f"t tv only, l tv + L1 ({L1_WEIGHT:g}), a tv + L1 + ortho ({ORTHO_WEIGHT:g})"
             + ("; learning rates 0 (--freeze): the parameters never move, every leg does the same work per step" if a.freeze else "")]

    for R in [int(x) for x in a.batches.split(",")]:
        def idx_of(k):
            return perm[(k * R) % (n - R):][:R]

        def block(leg):
            torch.manual_seed(1024)
            field.load_state_dict(init_state)
            opt = TVAdam(field.get_optparam_groups(*((0.0, 0.0) if a.freeze else (0.02, 1e-3))), betas=(0.9, 0.99), field=field)
            kw = dict(N_samples=n_samples, white_bg=True, **terms[leg])
            pf = BatchPrefetcher([allrays, allrgb, alldepth])
            pf.submit(idx_of(0))

            def it(k):
                b = pf.get()
                pf.submit(idx_of(k + 1))
                return field.train_step(b[0], b[1], b[2], opt, **kw)

            for k in range(a.warmup):
                it(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(a.iters):
                it(a.warmup + k)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            fs = field.__dict__.get("_fused_step")
            fs.sync()
            stats = (fs.pipelined_launches, fs.replays)
            pf.get()
            pf.close()
            return dt / a.iters * 1e3, stats

        res = {leg: [] for leg in a.legs}
        block(a.legs[0])                              # (one untimed block: allocations, pinned buffers, first-use costs)
        for _ in range(a.blocks):
            for leg in a.legs:
                res[leg].append(block(leg))
        lines.append(f"R = {R}:")
        for leg in a.legs:
            ms = [r[0] for r in res[leg]]
            pip = res[leg][-1][1]
            lines.append(f"  ({leg}) {statistics.median(ms):.3f} ms per step (blocks {', '.join(f'{v:.3f}' for v in ms)}; spread "
                         f"{max(ms) - min(ms):.3f}); pipelined launches / replays in the last block's driver: {pip[0]} / {pip[1]}")

    if has_reg:
        # the ortho launches on their own: device events around the seed call with and without them (both zero-fill the whole buffer)
        lib = _lib.load()
        field.load_state_dict(init_state)
        h = field.sync_params()
        field.factor_grad_buffer(_raw=True)
        st = _lib.current_stream_ptr(dev)

        def timed(fn, reps=200):
            out = []
            for _ in range(20):
                fn()
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1) * 1e3)
            return out
        with torch.cuda.device(dev):
            zero = timed(lambda: _lib.check(lib.t2n_field_tv_seed(h, 0.0, 0.0, st), "t2n_field_tv_seed"))
            both = timed(lambda: _lib.check(lib.t2n_field_reg_seed(h, 0.0, 0.0, 0.0, 0.0, ORTHO_WEIGHT, ORTHO_WEIGHT, st), "t2n_field_reg_seed"))
            l1_seed = timed(lambda: _lib.check(lib.t2n_field_reg_seed(h, 1e-3, 1e-4, L1_WEIGHT, L1_WEIGHT, 0.0, 0.0, st), "t2n_field_reg_seed"))
            tv_seed = timed(lambda: _lib.check(lib.t2n_field_tv_seed(h, 1e-3, 1e-4, st), "t2n_field_tv_seed"))
        med = statistics.median
        lines.append(f"seed call alone, device events, 200 calls each, median us (min): zero fill {med(zero):.1f} ({min(zero):.1f}); zero fill + the "
                     f"two ortho launches {med(both):.1f} ({min(both):.1f}) -> the ortho launches {med(both) - med(zero):.1f} us; TV seed "
                     f"{med(tv_seed):.1f} ({min(tv_seed):.1f}); TV + L1 seed {med(l1_seed):.1f} ({min(l1_seed):.1f}) -> L1 in the seed launch "
                     f"{med(l1_seed) - med(tv_seed):+.1f} us")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
