#!/usr/bin/env python3
"""Time the device marching cubes (csrc/t2n_mesh.hip) at 300^3: `t2n_mc_count` (classify + scan) and `t2n_mc_emit` (vertices + triangles)
with device events around `reps` calls each, and the whole `mesh.marching_cubes` call (allocations, the 16-byte read of the counts
between the two, normals) with a host clock. The volume is getDenseAlpha([300] * 3) of a synthetic field (text2nerf_amd.synth), at
upstream's export level 0.005 and at the volume's median (a much denser surface). Fresh process, warm-up excluded, median over the
blocks. There is no predecessor on the device and no target: the file records what was measured.

    python tools/time_mesh.py [--blocks 5] [--reps 200] [--n 300] [--out profiles/mesh_timing.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from text2nerf_amd import TensorVMSplit, _lib, mesh, synth  # noqa: E402

GRID, AABB, NF = [24, 20, 16], [[-8.0, -6.0, -7.0], [8.0, 7.0, 6.5]], [0.5, 8.0]


def timed_device(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def timed_host(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def med(xs):
    return f"{statistics.median(xs):.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_mesh.py measures on the GPU only")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    params = synth.make_field_params(11, GRID, density_scale=0.9, aabb=AABB)
    m = TensorVMSplit(torch.tensor(AABB), GRID, dev, density_n_comp=[16] * 3, appearance_n_comp=[48] * 3, app_dim=27, near_far=NF,
                      shadingMode="MLP_Fea_noview", density_shift=-10, distance_scale=25, pos_pe=0, view_pe=0, fea_pe=6, featureC=128,
                      step_ratio=1.0, fea2denseAct="softplus")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    n = a.n
    vol = m.getDenseAlpha([n, n, n])[0].contiguous()
    lines = [f"device marching cubes at {n}^3 (getDenseAlpha of a synthetic {GRID} field); {torch.cuda.get_device_name(0)}; median of "
             f"{a.blocks} blocks, count / emit: device events around {a.reps} calls, marching_cubes: host clock around one call "
             f"(synchronised at both ends); warm-up excluded; the same volume every call, so it is read from a warm cache hierarchy"]
    ws = torch.empty(int(lib.t2n_mc_workspace_bytes(n, n, n)), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    org, sp = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    stream = _lib.current_stream_ptr(dev)
    for label, level in (("level 0.005", 0.005), ("level = median", float(vol.median()))):
        def count():
            _lib.check(lib.t2n_mc_count(_lib.ptr(vol), n, n, n, level, _lib.ptr(ws), _lib.ptr(counts), stream), "t2n_mc_count")
        count()
        V, F = (int(x) for x in counts.cpu().tolist())
        if V == 0:
            lines.append(f"{label} ({level:.6g}): no edge crosses it, emit not measured")
            continue
        verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
        norms = torch.empty(V, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(F, 3, dtype=torch.int32, device=dev)

        def emit(nrm=norms):
            _lib.check(lib.t2n_mc_emit(_lib.ptr(vol), n, n, n, level, _lib.ptr(ws), org, sp, 0, _lib.ptr(verts), _lib.ptr(nrm),
                                       _lib.ptr(faces), stream), "t2n_mc_emit")

        def whole():
            return mesh.marching_cubes(vol, level)
        for _ in range(3):
            count(); emit(); emit(None); whole()
        t_count, t_emit, t_emit0, t_whole = [], [], [], []
        for _ in range(a.blocks):
            t_count.append(timed_device(count, a.reps))
            t_emit.append(timed_device(emit, a.reps))
            t_emit0.append(timed_device(lambda: emit(None), a.reps))
            t_whole.append(timed_host(whole))
        line = (f"{label} ({level:.6g}): {V} vertices, {F} triangles; count {med(t_count)}; emit with normals {med(t_emit)}; emit without "
                f"normals {med(t_emit0)}; marching_cubes {med(t_whole)}")
        lines.append(line)
        print(line, flush=True)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
