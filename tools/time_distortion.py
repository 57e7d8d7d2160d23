#!/usr/bin/env python3
"""Time the distortion regulariser (csrc/t2n_depth_loss.hip), in one process per package:

  loss stage   t2n_train_loss (the yardstick), t2n_train_loss_ex per depth kind, t2n_train_loss_dist per depth kind with w_dist > 0,
               and t2n_distortion_loss with and without its gradient, on seeded render-shaped inputs (sorted z) at 16 384 x 259 and
               2 048 x 259: device events around `reps` calls, the legs alternating within each block, one warm-up call per leg
               excluded, median of the blocks with their spread. Beside each time: the bytes the call must move at least (weights
               and z_vals read once, d_weights written once) over that time, and for the term the same over the time it adds.
  steps        with --steps: the composed train_step(fused=False) at 16 384 and 2 048 rays on bench.py's field, keyword omitted and
               (where the package has it) distortion > 0, with and without --freeze (learning rates 0: the parameters never move, so
               every leg and every block does the same work; otherwise the legs train different fields). Wall clock over `iters`
               steps after `warmup`, stream drained at the block's end; every block starts from the same parameters with a fresh
               optimiser.

`--root DIR` takes the package (and its library) from another checkout, e.g. the parent commit's build: only what that package has is
run there, which puts the parent's numbers beside this tree's (--out appends). No threshold: the numbers are a report.

    python tools/time_distortion.py [--blocks 3] [--reps 50] [--steps] [--freeze] [--root DIR] [--tag T] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("mse", "gnll", "si_log", "ssi")
W_DIST = 0.01


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", action="store_true", help="also time the composed train_step")
    ap.add_argument("--freeze", action="store_true", help="steps at learning rates 0")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--root", default=None, help="checkout whose text2nerf_amd package (and library) is measured")
    ap.add_argument("--tag", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg_root = os.path.abspath(a.root) if a.root else ROOT
    sys.path.insert(0, pkg_root)
    import numpy as np
    import torch
    import text2nerf_amd
    from text2nerf_amd import _lib
    assert os.path.dirname(os.path.dirname(os.path.abspath(text2nerf_amd.__file__))) == pkg_root, text2nerf_amd.__file__
    if not torch.cuda.is_available():
        sys.exit("time_distortion.py measures on the GPU only")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    has_dist = "t2n_train_loss_dist" in _lib.SIGNATURES
    lines = [f"distortion term, {a.tag or ('package at ' + os.path.relpath(pkg_root, ROOT))}; {torch.cuda.get_device_name(0)}; "
             f"median of {a.blocks} blocks, legs alternating within a block; kernels: device events around {a.reps} calls after one warm-up "
             f"call per leg; steps: wall clock over {a.iters} steps after {a.warmup}, stream drained at the block's end"]
    st = _lib.current_stream_ptr(dev)
    p = _lib.ptr
    for R, N in ((16384, 259), (2048, 259)):
        g = torch.Generator().manual_seed(R)
        rgb, rgb_t = torch.rand(R, 3, generator=g).to(dev), torch.rand(R, 3, generator=g).to(dev)
        depth, dep_t = (torch.rand(R, generator=g) * 6 + 1).to(dev), (torch.rand(R, generator=g) * 5 + 2).to(dev)
        w = (torch.rand(R, N, generator=g) * 0.05).to(dev)
        z = (torch.rand(R, N, generator=g).sort(1)[0] * 7.5 + 0.5).to(dev)
        d_rgb, d_depth, d_w, losses = torch.empty_like(rgb), torch.empty_like(depth), torch.empty_like(w), torch.empty(4, device=dev)
        aux, dist = torch.empty(4, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
        loss1 = torch.empty(1, device=dev)
        nbytes = int((lib.t2n_train_loss_dist_workspace_bytes if has_dist else lib.t2n_train_loss_ex_workspace_bytes)(R))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

        def base():
            _lib.check(lib.t2n_train_loss(p(rgb), p(depth), p(w), p(z), p(rgb_t), p(dep_t), R, N, 0.005, 1e3, 0.1, p(d_rgb), p(d_depth), p(d_w),
                                          p(losses), p(ws), ws.numel(), st), "t2n_train_loss")

        def ex(kind):
            _lib.check(lib.t2n_train_loss_ex(p(rgb), p(depth), p(w), p(z), p(rgb_t), p(dep_t), R, N, 0.005, 1e3, 0.1, kind, 0.1, p(d_rgb),
                                             p(d_depth), p(d_w), p(losses), p(aux), p(ws), ws.numel(), st), "t2n_train_loss_ex")

        def with_dist(kind):
            _lib.check(lib.t2n_train_loss_dist(p(rgb), p(depth), p(w), p(z), p(rgb_t), p(dep_t), R, N, 0.005, 1e3, 0.1, kind, 0.1, W_DIST,
                                               1.0 / 7.5, p(d_rgb), p(d_depth), p(d_w), p(losses), p(aux), p(dist), p(ws), ws.numel(), st),
                       "t2n_train_loss_dist")

        def alone(grad):
            _lib.check(lib.t2n_distortion_loss(p(w), p(z), R, N, 1.0 / 7.5, p(loss1), p(d_w) if grad else None, p(ws), ws.numel(), st),
                       "t2n_distortion_loss")

        legs = {"t2n_train_loss": base}
        for k, name in enumerate(KINDS):
            legs[f"t2n_train_loss_ex {name}"] = (lambda k=k: ex(k))
            if has_dist:
                legs[f"t2n_train_loss_dist {name}"] = (lambda k=k: with_dist(k))
        if has_dist:
            legs["t2n_distortion_loss"] = lambda: alone(True)
            legs["t2n_distortion_loss, no gradient"] = lambda: alone(False)
        res = {name: [] for name in legs}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(a.blocks):
            for name, fn in legs.items():
                fn()
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                e1.synchronize()
                res[name].append(e0.elapsed_time(e1) / a.reps * 1e3)
        med = {name: statistics.median(us) for name, us in res.items()}
        rw = 3 * R * N * 4                                 # weights and z_vals read once, d_weights written once
        lines.append(f"R x N = {R} x {N} (weights + z_vals + d_weights = {rw / 1e6:.1f} MB per call at the least):")
        for name, us in res.items():
            least = 2 * R * N * 4 if name.endswith("no gradient") else rw
            extra = ""
            if name.startswith("t2n_train_loss_dist"):
                d = med[name] - med[name.replace("_dist", "_ex")]
                extra = f"; the term adds {d:.2f} us"
            lines.append(f"  {name:34s} {med[name]:8.2f} us per call (blocks {', '.join(f'{v:.2f}' for v in us)}; spread "
                         f"{max(us) - min(us):.2f}) = {med[name] / med['t2n_train_loss']:.2f} x t2n_train_loss, {least / med[name] / 1e3:.0f} GB/s of "
                         f"the least traffic{extra}")
    if a.steps:
        sys.path.insert(1, ROOT)
        import bench                                     # build_field / reference_poses: the bench's field and poses
        from text2nerf_amd import synth
        from text2nerf_amd.optim import TVAdam
        torch.set_num_threads(2)
        field, _, _ = bench.build_field(dev)
        n_samples = min(int(1e6), int(synth.cal_n_samples([300] * 3, 1.0) / 2))
        allrays = np.concatenate([synth.frame_rays_np(512, 512, c2w=q) for q in bench.reference_poses("local_fixed")])
        init_state = {k: v.detach().clone() for k, v in field.state_dict().items()}
        tv_terms = [(field.density_plane, 0.1), (field.app_plane, 0.01)]
        lrs = (0.0, 0.0) if a.freeze else (0.02, 1e-3)
        legs = {"keyword omitted": {}}
        if has_dist:
            legs[f"distortion={W_DIST}"] = dict(distortion=W_DIST)
            legs[f"distortion={W_DIST}, depth_loss=ssi"] = dict(distortion=W_DIST, depth_loss="ssi")
            legs["depth_loss=ssi"] = dict(depth_loss="ssi")
        for R in (16384, 2048):
            np.random.seed(1024)
            rays = torch.from_numpy(allrays[np.random.permutation(allrays.shape[0])[:R]])
            gen = np.random.Generator(np.random.PCG64(1024))
            with torch.no_grad():                            # targets: the scene's own colours / depths + noise, as bench.py makes them
                rgb_s, dep_s, _, _ = field(rays.to(dev), white_bg=True, is_train=False, N_samples=n_samples)
            rgb_t = (rgb_s.cpu() + torch.from_numpy(gen.normal(0, 0.05, (R, 3)).astype(np.float32))).clamp(0, 1)
            dep_t = (dep_s.cpu() + torch.from_numpy(gen.normal(0, 0.05, (R,)).astype(np.float32))).clamp_min(0.5)
            final = {}

            def block(name):
                torch.manual_seed(1024)
                field.load_state_dict(init_state)
                opt = TVAdam(field.get_optparam_groups(*lrs), betas=(0.9, 0.99), field=field)
                kw = dict(N_samples=n_samples, white_bg=True, tv=tv_terms, fused=False, **legs[name])
                for _ in range(a.warmup):
                    field.train_step(rays, rgb_t, dep_t, opt, **kw)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    last = field.train_step(rays, rgb_t, dep_t, opt, **kw)
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / a.iters * 1e3
                d = getattr(field, "last_distortion", None)
                final[name] = [float(v) for v in last.cpu()] + ([float(d)] if d is not None else [])
                return dt

            res = {k: [] for k in legs}
            block(next(iter(legs)))                           # (one untimed block: allocations, first-use costs)
            for _ in range(a.blocks):
                for k in legs:
                    res[k].append(block(k))
            lines.append(f"composed train_step(fused=False), {R} rays x {n_samples} samples, TV terms on, learning rates {lrs}:")
            for k, ms in res.items():
                lines.append(f"  {k:38s} {statistics.median(ms):.3f} ms per step (blocks {', '.join(f'{v:.3f}' for v in ms)}; spread "
                             f"{max(ms) - min(ms):.3f}); last step's [mse, depth term, transmittance, total(, D)] = "
                             f"[{', '.join(f'{v:.4g}' for v in final[k])}]")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
