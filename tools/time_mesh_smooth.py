#!/usr/bin/env python3
"""Time the smoothing stage (csrc/t2n_mesh_smooth.hip) on the marching-cubes mesh of the bench field's n^3 volume (bench.build_field,
getDenseAlpha at level 0.005), beside the marching-cubes count + emit of the same volume, and getDenseFeature beside getDenseAlpha:

    adjacency     keys + device sort + t2n_mesh_csr, device events around `reps` builds (the 8-byte read of E is not in it)
    10 iterations twenty t2n_mesh_smooth_pass launches between two float64 buffers, device events around `reps` runs
    normals       vertex -> face rows (keys + sort + t2n_mesh_csr) and t2n_mesh_vertex_normals, device events
    whole calls   mesh.mesh_adjacency, mesh.smooth_mesh(iterations=10) of a mesh with normals, mesh.vertex_normals: host clock around
                  one call (allocations, the index check, the host reads), synchronised at both ends
    dense volumes getDenseAlpha and getDenseFeature at n^3, host clock around one call

Fresh process, warm-up excluded, the stages take turns inside every block (alternating), median over the blocks. The least traffic of
a smoothing pass on float64 positions is V (valence (4 + 24) + 48) bytes (a neighbour index and a float64 position per entry, the
vertex' own position in and out); the achieved rate is printed against it. No predecessor on the device and no target: the file
records what was measured.

    python tools/time_mesh_smooth.py [--blocks 5] [--reps 20] [--n 300] [--out profiles/mesh_smooth_timing.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402
from text2nerf_amd import _lib, mesh  # noqa: E402
from time_mesh import med, timed_device, timed_host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_mesh_smooth.py measures on the GPU only")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n = a.n
    field, _, _ = bench.build_field(dev, grid=n)
    level = 0.005
    vol = field.getDenseAlpha([n, n, n])[0].contiguous()
    verts, faces, norms = mesh.marching_cubes(vol, level)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if V == 0:
        sys.exit(f"no edge of the {n}^3 alpha volume crosses {level}")
    stream = _lib.current_stream_ptr(dev)
    p = _lib.ptr

    mc_ws = torch.empty(int(lib.t2n_mc_workspace_bytes(n, n, n)), dtype=torch.uint8, device=dev)
    mc_counts = torch.empty(2, dtype=torch.int64, device=dev)
    org, sp = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)

    def mc():
        _lib.check(lib.t2n_mc_count(p(vol), n, n, n, level, p(mc_ws), p(mc_counts), stream), "t2n_mc_count")
        _lib.check(lib.t2n_mc_emit(p(vol), n, n, n, level, p(mc_ws), org, sp, 0, p(verts), p(norms), p(faces), stream), "t2n_mc_emit")

    def rows_fn(per, fn, name):
        nk = per * F
        keys = torch.empty(nk, dtype=torch.int64, device=dev)
        nb = int(lib.t2n_mesh_csr_workspace_bytes(nk))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        off = torch.empty(V + 1, dtype=torch.int64, device=dev)
        val = torch.empty(nk, dtype=torch.int32, device=dev)
        cnt = torch.empty(1, dtype=torch.int64, device=dev)

        def run():
            _lib.check(fn(p(faces), F, V, p(keys), stream), name)
            s = torch.sort(keys).values
            _lib.check(lib.t2n_mesh_csr(p(s), nk, V, p(off), p(val), p(cnt), p(ws), nb, stream), "t2n_mesh_csr")
        return run, off, val, cnt
    adjacency, off, nbr, cnt = rows_fn(6, lib.t2n_mesh_edge_keys, "t2n_mesh_edge_keys")
    adjacency()
    E = int(cnt.item())
    vf_rows, voff, vrows, vcnt = rows_fn(3, lib.t2n_mesh_face_keys, "t2n_mesh_face_keys")
    vf_rows()
    Ef = int(vcnt.item())
    x = verts.double()
    y = torch.empty_like(x)
    nout = torch.empty(V, 3, dtype=torch.float32, device=dev)

    def ten_iterations():
        a_, b_ = x, y
        for _ in range(10):
            for s in (0.5, -0.53):
                _lib.check(lib.t2n_mesh_smooth_pass(p(a_), p(b_), p(off), p(nbr), E, None, V, s, stream), "t2n_mesh_smooth_pass")
                a_, b_ = b_, a_

    def normals():
        vf_rows()
        _lib.check(lib.t2n_mesh_vertex_normals(p(verts), p(faces), F, p(voff), p(vrows), Ef, V, p(nout), stream), "t2n_mesh_vertex_normals")

    def normals_kernel():
        _lib.check(lib.t2n_mesh_vertex_normals(p(verts), p(faces), F, p(voff), p(vrows), Ef, V, p(nout), stream), "t2n_mesh_vertex_normals")

    whole = {"mesh_adjacency": lambda: mesh.mesh_adjacency(faces, V),
             "smooth_mesh(iterations=10), normals recomputed": lambda: mesh.smooth_mesh((verts, faces, norms), iterations=10),
             "vertex_normals": lambda: mesh.vertex_normals(verts, faces),
             "getDenseAlpha": lambda: field.getDenseAlpha([n, n, n]),
             "getDenseFeature": lambda: field.getDenseFeature([n, n, n])}
    device = {"marching cubes count + emit with normals": mc, "adjacency (keys, sort, t2n_mesh_csr)": adjacency,
              "10 iterations (20 t2n_mesh_smooth_pass)": ten_iterations, "normals (keys, sort, t2n_mesh_csr, t2n_mesh_vertex_normals)": normals,
              "t2n_mesh_vertex_normals alone": normals_kernel}
    for fn in list(device.values()) + list(whole.values()):
        for _ in range(2):
            fn()
    t = {k: [] for k in list(device) + list(whole)}
    for _ in range(a.blocks):
        for k, fn in device.items():
            t[k].append(timed_device(fn, a.reps))
        for k, fn in whole.items():
            t[k].append(timed_host(fn))
    valence = E / V
    pass_bytes = V * (valence * (4 + 24) + 48)
    it_ms = statistics.median(t["10 iterations (20 t2n_mesh_smooth_pass)"])
    mc_ms = statistics.median(t["marching cubes count + emit with normals"])
    lines = [f"mesh smoothing behind the device marching cubes at {n}^3 (getDenseAlpha of the bench field, level {level}); "
             f"{torch.cuda.get_device_name(0)}; median of {a.blocks} blocks, the stages alternating inside a block; device events around "
             f"{a.reps} calls, whole calls by a host clock around one call (synchronised at both ends); warm-up excluded; the same mesh "
             f"every call, so it is read from a warm cache hierarchy",
             f"mesh: {V} vertices, {F} triangles, {E} directed edges (mean valence {valence:.2f}), {Ef} vertex-face entries"]
    lines += [f"{k}: {med(v)}" for k, v in t.items()]
    lines.append(f"a smoothing pass moves at least V (valence (4 + 24) + 48) = {pass_bytes / 1e6:.2f} MB (float64 positions); 20 passes in "
                 f"{it_ms:.3f} ms = {20 * pass_bytes / (it_ms * 1e-3) / 1e9:.0f} GB/s against that floor (the {V * 24 / 1e6:.1f} MB of positions "
                 f"and the rows are read again by every pass: a rate above HBM's means they stayed in the cache hierarchy)")
    lines.append(f"10 iterations cost {it_ms / mc_ms:.2f} x the marching-cubes count + emit of the same volume"
                 + (": more, because " if it_ms > mc_ms else ": less; ")
                 + f"a pass is one launch over {V} threads that gather {valence:.1f} float64 positions each through an index row, twenty launches "
                 f"in a row, while marching cubes streams {n**3 * 4 / 1e6:.0f} MB of volume in four launches")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
