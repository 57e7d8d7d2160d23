#!/usr/bin/env python3
"""Time training on the general-shape path: bench.py's wide field (general_shape_ms: 128^3 grid, [32,20,24] density / [96,64,72]
appearance components, app_dim 27, fea_pe 6, featureC 256, MLP_Fea_noview) at N = 259 samples per ray.

  (a) forward + loss + backward through the public autograd surface — OctreeRender_trilinear_fast(is_train=True), the driver's loss as
      torch ops, .backward() — median of 3 calls after 2 warm-up calls, device events on the stream. Uses nothing a checkout without
      the kernel backward lacks, so `--root DIR` measures another checkout (the parent commit's build) with the same tool.
  (b) train_step with TVAdam (composed route; only where the package has it), same protocol.

One invocation measures ONE ray count (`--rays`), so that a job script can give each its own time limit. `--state FILE` carries the
256-ray figure from one invocation to the next: a larger ray count is only started when the cost predicted from it (linear in the
appearance samples, hence in the rays of a seeded random subset) fits `--limit` seconds with a factor of 4 to spare; otherwise the
invocation says so and exits 0 without touching the GPU's time. Nothing is retried.

Beside each measured time the tool prints two derived floors:
  atomics   the factor scatters' float-atomic bytes (6 taps x 4 B per component: density components of every evaluated sample,
            appearance components of every list entry) / 1.3 TB/s (chip-wide float-atomic rate, contiguous rows)
  GEMM      the forward's and the backward's matrix FLOPs per list entry x the entries / the rate k_dense reaches — taken from
            `--kernel-stats FILE`, the *_kernel_stats.csv of one `rocprofv3 --kernel-trace --stats` run of this tool with `--profile`
            (which also lists the backward's kernels by share); without that file the GEMM floor is "not measured".

    python tools/time_generic_train.py --rays 2048 [--root DIR] [--state FILE] [--limit 120] [--tag T] [--out FILE] [--profile]
                                       [--kernel-stats CSV --profile-iters K]"""
import argparse
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, HW, N = 128, 400, 259
DEN, APP, DIM, PE, FC = [32, 20, 24], [96, 64, 72], 27, 6, 256
IN0, NCOL = DIM * (1 + 2 * PE), sum(APP)
ATOMIC_RATE = 1.3e12       # B/s, global float atomics into contiguous rows


def flops_per_entry():
    """Matrix FLOPs per appearance-list entry: (forward, backward). Forward: basis, layers 0 / 1 / 2. Backward: layers 0 / 1 again (the
    activations are rebuilt), three weight-gradient GEMMs + the basis gradient, three input-gradient GEMMs."""
    fwd = 2 * (DIM * NCOL + IN0 * FC + FC * FC + 3 * FC)
    bwd = 2 * (IN0 * FC + FC * FC) + 2 * (3 * FC + FC * FC + FC * IN0 + DIM * NCOL) + 2 * (3 * FC + FC * FC + FC * IN0 + DIM * NCOL)
    return fwd, bwd


def dense_flops_per_entry():
    """What k_dense itself multiplies per entry in forward + kernel backward: layers 0 / 1 twice, G1 W1, G0 W0, gfeat B."""
    return 2 * (2 * (IN0 * FC + FC * FC) + FC * FC + FC * IN0 + DIM * NCOL)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, required=True)
    ap.add_argument("--root", default=None, help="checkout whose text2nerf_amd package (and library) is measured")
    ap.add_argument("--state", default=None)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--tag", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="2 warm-up + --profile-iters calls of (a) only, for a rocprofv3 run")
    ap.add_argument("--profile-iters", type=int, default=3)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    pkg_root = os.path.abspath(a.root) if a.root else ROOT
    tag = a.tag or ("package at " + (os.path.relpath(pkg_root, ROOT) if a.root else "this tree"))
    state = json.load(open(a.state)) if a.state and os.path.exists(a.state) else {}
    key = f"{tag}|256"
    lines = []

    def finish():
        text = "\n".join(lines)
        print(text, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(text + "\n")
        if a.state:
            json.dump(state, open(a.state, "w"))

    calls = 5
    if a.rays > 256 and not a.profile:
        if key not in state:
            lines.append(f"[{tag}] {a.rays} rays: not started — no 256-ray figure to size it from")
            return finish()
        predicted = state[key] * a.rays / 256.0 * calls / 1e3
        if predicted * 4 > a.limit:
            lines.append(f"[{tag}] {a.rays} rays: not started — {calls} calls predicted at {predicted:.1f} s from the 256-ray figure "
                         f"({state[key]:.1f} ms), which does not fit {a.limit:.0f} s with a factor of 4 to spare")
            return finish()

    sys.path.insert(0, pkg_root)
    import numpy as np
    import torch
    import text2nerf_amd
    from text2nerf_amd import OctreeRender_trilinear_fast, TensorVMSplit, synth
    assert os.path.dirname(os.path.dirname(os.path.abspath(text2nerf_amd.__file__))) == pkg_root, text2nerf_amd.__file__
    if not torch.cuda.is_available():
        sys.exit("time_generic_train.py measures on the GPU only")
    dev = torch.device("cuda:0")
    aabb, nf = [[-8.0, -6.0, -7.0], [8.0, 7.0, 6.5]], [0.5, 8.0]
    params = synth.make_field_params(11, [G] * 3, density_n_comp=DEN, app_n_comp=APP, app_dim=DIM, feature_c=FC, fea_pe=PE,
                                     shading_mode="MLP_Fea_noview", density_scale=0.9, aabb=aabb)
    m = TensorVMSplit(torch.tensor(aabb), [G] * 3, dev, density_n_comp=DEN, appearance_n_comp=APP, app_dim=DIM, near_far=nf,
                      shadingMode="MLP_Fea_noview", density_shift=-10, distance_scale=25, pos_pe=0, view_pe=0, fea_pe=PE, featureC=FC,
                      step_ratio=1.0, fea2denseAct="softplus")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    allrays = synth.frame_rays_np(HW, HW, c2w=synth.look_pose(0.3, -0.1, (0.2, 0.1, -1.0)))
    gen = np.random.Generator(np.random.PCG64(1024))
    rays = torch.from_numpy(np.ascontiguousarray(allrays[gen.permutation(allrays.shape[0])[:a.rays]])).to(dev)
    R = rays.shape[0]
    with torch.no_grad():                                # targets: the scene's own colours / depths + noise, as bench.py makes them
        rgb_s, dep_s, _, _ = m(rays, white_bg=True, is_train=False, N_samples=N)
    rgb_t = (rgb_s + torch.from_numpy(gen.normal(0, 0.05, (R, 3)).astype(np.float32)).to(dev)).clamp(0, 1)
    dep_t = (dep_s + torch.from_numpy(gen.normal(0, 0.05, (R,)).astype(np.float32)).to(dev)).clamp_min(0.5)

    def loss_of(rgb, depth, w, z):
        mse = torch.mean((rgb - rgb_t) ** 2)
        dl = torch.mean((depth - dep_t) ** 2)
        mm = (w * ((z - dep_t[:, None] + 0.1) < 0)).mean(1)
        return mse + 0.005 * dl + 1e3 * torch.mean(mm * mm)

    def autograd_call():
        for p in m.parameters():
            p.grad = None
        rgb, _, depth, w, z = OctreeRender_trilinear_fast(rays, m, chunk=R, N_samples=N, white_bg=True, is_train=True, device=dev)
        loss_of(rgb, depth, w, z).backward()

    def timed(fn, warm=2, reps=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1))
        return out

    torch.manual_seed(1024)
    if a.profile:
        timed(autograd_call, reps=a.profile_iters)
        st = m.stats()
        state[f"{tag}|profile"] = dict(rays=R, iters=2 + a.profile_iters, appearance=st["appearance"], evaluated=st["evaluated"])
        lines.append(f"[{tag}] profile run: {2 + a.profile_iters} calls of (a) at {R} rays, list {st['appearance']} entries")
        return finish()
    ms_a = timed(autograd_call)
    st = m.stats()
    napp, nev = st["appearance"], st["evaluated"]
    if a.rays == 256:
        state[key] = statistics.median(ms_a)
    plan = m.general_backward_plan(R, N) if hasattr(m, "general_backward_plan") else None
    atom_bytes = (nev * sum(DEN) + napp * NCOL) * 6 * 4
    fwd, bwd = flops_per_entry()
    dense_rate = None
    if a.kernel_stats and os.path.exists(a.kernel_stats) and f"{tag}|profile" in state:
        pr = state[f"{tag}|profile"]
        rows = list(csv.DictReader(open(a.kernel_stats)))
        dense_ns = sum(float(r["TotalDurationNs"]) for r in rows if "k_dense" in r["Name"] and "sigmoid" not in r["Name"])
        if dense_ns > 0:
            dense_rate = dense_flops_per_entry() * pr["appearance"] * pr["iters"] / (dense_ns * 1e-9)
    lines.append(f"[{tag}] {torch.cuda.get_device_name(0)}; wide field {DEN} / {APP} / {DIM} / {PE} / {FC}, {G}^3 grid, {R} rays x {N} samples, "
                 f"list {napp} entries, {nev} evaluated samples; backward: "
                 f"{'kernel form, ' + str(plan['max_passes']) + ' pass(es) of ' + str(plan['pass_rows']) if plan and plan['kernel_form'] else 'plain form'}")
    lines.append(f"  (a) forward + loss + backward (autograd surface): median {statistics.median(ms_a):10.3f} ms  (calls {', '.join(f'{v:.3f}' for v in ms_a)})")
    lines.append(f"      floor, factor-scatter atomics: {atom_bytes / 1e6:9.1f} MB / 1.3 TB/s = {atom_bytes / ATOMIC_RATE * 1e3:8.3f} ms")
    if dense_rate:
        lines.append(f"      floor, GEMMs: {(fwd + bwd) * napp / 1e9:8.2f} GFLOP (forward {fwd * napp / 1e9:.2f} + backward {bwd * napp / 1e9:.2f}) / "
                     f"{dense_rate / 1e12:.2f} TFLOP/s (k_dense, same box) = {(fwd + bwd) * napp / dense_rate * 1e3:8.3f} ms")
    else:
        lines.append(f"      floor, GEMMs: {(fwd + bwd) * napp / 1e9:8.2f} GFLOP (forward {fwd * napp / 1e9:.2f} + backward {bwd * napp / 1e9:.2f}); "
                     "k_dense rate: not measured")
    if plan is not None:
        from text2nerf_amd.optim import TVAdam
        opt = TVAdam(m.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
        tv = [(m.density_plane, 0.1), (m.app_plane, 0.01)]
        ms_b = timed(lambda: m.train_step(rays, rgb_t, dep_t, opt, N_samples=N, white_bg=True, tv=tv))
        lines.append(f"  (b) train_step with TVAdam (composed route):      median {statistics.median(ms_b):10.3f} ms  (calls {', '.join(f'{v:.3f}' for v in ms_b)})")
    else:
        lines.append("  (b) train_step: this package has none on a general-shape field")
    if a.kernel_stats and os.path.exists(a.kernel_stats) and state.get(f"{tag}|profile", {}).get("rays") == R:
        pr = state[f"{tag}|profile"]
        rows = sorted(csv.DictReader(open(a.kernel_stats)), key=lambda r: -float(r["TotalDurationNs"]))
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        lines.append(f"  kernels of (a) at {pr['rays']} rays (one rocprofv3 --kernel-trace --stats run, {pr['iters']} calls; all kernels "
                     f"{tot / pr['iters'] / 1e6:.3f} ms per call):")
        for r in rows[:12]:
            lines.append(f"      {r['Name'][:64]:64s} {int(r['Calls']):5d} calls {float(r['TotalDurationNs']) / pr['iters'] / 1e6:9.3f} ms per call "
                         f"({float(r['TotalDurationNs']) / tot * 100:5.1f} %)")
    finish()


if __name__ == "__main__":
    main()
