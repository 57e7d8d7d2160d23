#!/usr/bin/env python3
"""Time the loss stage of the training step per depth kind, in one process: t2n_train_loss (the yardstick: the kernel every kind
other than "mse" replaces, unchanged) and t2n_train_loss_ex with depth_kind 0..3 on seeded render-shaped inputs at 16 384 x 259 and
2 048 x 259 — device events around `reps` calls, the legs alternating within each block, warm-up excluded, median of the blocks with
their spread — and, with --steps, the composed train_step(fused=False) per kind at 16 384 rays on bench.py's field (wall clock, stream
drained at the block's end; every block starts from the same parameters with a fresh optimiser, as bench.py's train leg does).

`--root DIR` takes the package (and its library) from another checkout, e.g. the parent commit's build: only what that package has is
run there (t2n_train_loss and the "mse" step), which puts the parent's numbers beside this tree's (--out appends). No threshold: the
numbers are a report.

    python tools/time_depth_loss.py [--blocks 3] [--reps 50] [--steps] [--root DIR] [--tag T] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("mse", "gnll", "si_log", "ssi")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", action="store_true", help="also time the composed train_step per kind")
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
    from text2nerf_amd import _lib
    assert os.path.dirname(os.path.dirname(os.path.abspath(text2nerf_amd.__file__))) == pkg_root, text2nerf_amd.__file__
    if not torch.cuda.is_available():
        sys.exit("time_depth_loss.py measures on the GPU only")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    has_ex = "t2n_train_loss_ex" in _lib.SIGNATURES
    lines = [f"loss stage per depth kind, {a.tag or ('package at ' + os.path.relpath(pkg_root, ROOT))}; {torch.cuda.get_device_name(0)}; "
             f"median of {a.blocks} blocks, legs alternating within a block; kernels: device events around {a.reps} calls after one warm-up "
             f"call per leg; steps: wall clock over {a.iters} steps after {a.warmup}, stream drained at the block's end"]
    st = _lib.current_stream_ptr(dev)
    for R, N in ((16384, 259), (2048, 259)):
        g = torch.Generator().manual_seed(R)
        rgb, rgb_t = torch.rand(R, 3, generator=g).to(dev), torch.rand(R, 3, generator=g).to(dev)
        depth, dep_t = (torch.rand(R, generator=g) * 6 + 1).to(dev), (torch.rand(R, generator=g) * 5 + 2).to(dev)
        w = (torch.rand(R, N, generator=g) * 0.05).to(dev)
        z = (torch.rand(R, N, generator=g).sort(1)[0] * 7.5 + 0.5).to(dev)
        d_rgb, d_depth, d_w, losses = torch.empty_like(rgb), torch.empty_like(depth), torch.empty_like(w), torch.empty(4, device=dev)
        aux = torch.empty(4, dtype=torch.float64, device=dev)
        nbytes = int(lib.t2n_train_loss_ex_workspace_bytes(R)) if has_ex else int(lib.t2n_train_loss_workspace_bytes(R))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        p = _lib.ptr

        def base():
            _lib.check(lib.t2n_train_loss(p(rgb), p(depth), p(w), p(z), p(rgb_t), p(dep_t), R, N, 0.005, 1e3, 0.1, p(d_rgb), p(d_depth), p(d_w),
                                          p(losses), p(ws), ws.numel(), st), "t2n_train_loss")

        def ex(kind):
            _lib.check(lib.t2n_train_loss_ex(p(rgb), p(depth), p(w), p(z), p(rgb_t), p(dep_t), R, N, 0.005, 1e3, 0.1, kind, 0.1, p(d_rgb),
                                             p(d_depth), p(d_w), p(losses), p(aux), p(ws), ws.numel(), st), "t2n_train_loss_ex")

        legs = {"t2n_train_loss": base}
        if has_ex:
            for k, name in enumerate(KINDS):
                legs[f"t2n_train_loss_ex {name}"] = (lambda k=k: ex(k))
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
        ref = statistics.median(res["t2n_train_loss"])
        lines.append(f"R x N = {R} x {N} (w and z: {2 * R * N * 4 / 1e6:.1f} MB per read):")
        for name, us in res.items():
            lines.append(f"  {name:28s} {statistics.median(us):8.2f} us per call (blocks {', '.join(f'{v:.2f}' for v in us)}; spread "
                         f"{max(us) - min(us):.2f}) = {statistics.median(us) / ref:.2f} x t2n_train_loss")
    if a.steps:
        sys.path.insert(1, ROOT)
        import bench                                     # build_field / reference_poses: the bench's field and poses
        from text2nerf_amd import synth
        from text2nerf_amd.optim import TVAdam
        torch.set_num_threads(2)
        field, _, _ = bench.build_field(dev)
        n_samples = min(int(1e6), int(synth.cal_n_samples([300] * 3, 1.0) / 2))
        R = 16384
        allrays = np.concatenate([synth.frame_rays_np(512, 512, c2w=q) for q in bench.reference_poses("local_fixed")])
        np.random.seed(1024)
        rays = torch.from_numpy(allrays[np.random.permutation(allrays.shape[0])[:R]])
        gen = np.random.Generator(np.random.PCG64(1024))
        with torch.no_grad():                            # targets: the scene's own colours / depths + noise, as bench.py makes them
            rgb_s, dep_s, _, _ = field(rays.to(dev), white_bg=True, is_train=False, N_samples=n_samples)
        rgb_t = (rgb_s.cpu() + torch.from_numpy(gen.normal(0, 0.05, (R, 3)).astype(np.float32))).clamp(0, 1)
        dep_t = (dep_s.cpu() + torch.from_numpy(gen.normal(0, 0.05, (R,)).astype(np.float32))).clamp_min(0.5)
        init_state = {k: v.detach().clone() for k, v in field.state_dict().items()}
        tv_terms = [(field.density_plane, 0.1), (field.app_plane, 0.01)]
        kinds = KINDS if has_ex else ("mse",)

        def block(kind):
            torch.manual_seed(1024)
            field.load_state_dict(init_state)
            opt = TVAdam(field.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=field)
            kw = dict(N_samples=n_samples, white_bg=True, tv=tv_terms, fused=False)
            if has_ex:
                kw["depth_loss"] = kind
            for _ in range(a.warmup):
                field.train_step(rays, rgb_t, dep_t, opt, **kw)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                last = field.train_step(rays, rgb_t, dep_t, opt, **kw)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.iters * 1e3
            final[kind] = [float(v) for v in last.cpu()]
            return dt

        res, final = {k: [] for k in kinds}, {}
        block(kinds[0])                                   # (one untimed block: allocations, first-use costs)
        for _ in range(a.blocks):
            for k in kinds:
                res[k].append(block(k))
        lines.append(f"composed train_step(fused=False), {R} rays x {n_samples} samples, TV terms on:")
        for k, ms in res.items():
            lines.append(f"  depth_loss={k:7s} {statistics.median(ms):.3f} ms per step (blocks {', '.join(f'{v:.3f}' for v in ms)}; spread "
                         f"{max(ms) - min(ms):.3f}); last step's [mse, depth term, transmittance, total] = "
                         f"[{', '.join(f'{v:.4g}' for v in final[k])}]")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
