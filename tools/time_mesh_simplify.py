#!/usr/bin/env python3
"""Time the simplification stage (csrc/t2n_mesh_simplify.hip) on the marching-cubes mesh of the bench field's n^3 volume (bench.build_field,
getDenseAlpha at level 0.005, node spacing 1: the mesh tools/time_mesh_smooth.py uses), at cells of 2 and 4 node spacings:

    whole calls   mesh.simplify_mesh under both placements (no normals, no colours) and mesh.smooth_mesh(iterations=10) of the same
                  mesh as the yardstick: host clock around one call (allocations, the index check, the host reads), synchronised at
                  both ends
    stages        device events around `reps` runs, buffers allocated once, no host read inside:
                  keys + sort   t2n_mesh_cluster_keys and the device sort of the V keys
                  rows          t2n_mesh_cluster_rows
                  placement     t2n_mesh_cluster_face_keys, the sort of the 3 F keys, t2n_mesh_csr, t2n_mesh_cluster_place (quadric);
                                beside it the place kernel alone, quadric and mean
                  faces         t2n_mesh_simplify_face_map, the two stable sorts, t2n_mesh_simplify_faces
                  10 iterations twenty t2n_mesh_smooth_pass launches over a prebuilt adjacency

Fresh process, warm-up excluded, the stages take turns inside every block (alternating), median over the blocks. No predecessor on the
device and no target: the file records what was measured.

    python tools/time_mesh_simplify.py [--blocks 5] [--reps 20] [--n 300] [--out profiles/mesh_simplify_timing.txt]"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402
from text2nerf_amd import _lib, mesh  # noqa: E402
from time_mesh import med, timed_device, timed_host  # noqa: E402


def stages(lib, dev, verts, faces, cell):
    """name -> callable for one cell size, over buffers allocated here, and (V', F', face row entries)."""
    V, F = int(verts.shape[0]), int(faces.shape[0])
    stream = _lib.current_stream_ptr(dev)
    p = _lib.ptr
    _, o, h, dims = mesh._cluster_grid(verts, cell, None, "time_mesh_simplify")
    o3, h3, d3 = (C.c_double * 3)(*o), (C.c_double * 3)(*h), (C.c_int32 * 3)(*dims)
    keys = torch.empty(V, dtype=torch.int64, device=dev)
    sorted_keys = [None]
    nb = int(lib.t2n_mesh_cluster_rows_workspace_bytes(V))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    vmap = torch.empty(V, dtype=torch.int32, device=dev)
    off = torch.empty(V + 1, dtype=torch.int64, device=dev)
    mem = torch.empty(V, dtype=torch.int32, device=dev)
    cells = torch.empty(V, 3, dtype=torch.int32, device=dev)
    cnt = torch.empty(1, dtype=torch.int64, device=dev)

    def keys_sort():
        _lib.check(lib.t2n_mesh_cluster_keys(p(verts), V, o3, h3, d3, p(keys), stream), "t2n_mesh_cluster_keys")
        sorted_keys[0] = torch.sort(keys).values

    def rows():
        _lib.check(lib.t2n_mesh_cluster_rows(p(sorted_keys[0]), V, d3, p(vmap), p(off), p(mem), p(cells), p(cnt), p(ws), nb, stream),
                   "t2n_mesh_cluster_rows")
    keys_sort()
    rows()
    K = int(cnt.item())
    fkeys = torch.empty(3 * F, dtype=torch.int64, device=dev)
    nbc = int(lib.t2n_mesh_csr_workspace_bytes(3 * F))
    wsc = torch.empty(nbc, dtype=torch.uint8, device=dev)
    foff = torch.empty(K + 1, dtype=torch.int64, device=dev)
    frow = torch.empty(3 * F, dtype=torch.int32, device=dev)
    fcnt = torch.empty(1, dtype=torch.int64, device=dev)
    out = torch.empty(K, 3, dtype=torch.float32, device=dev)
    E = [0]

    def face_rows():
        _lib.check(lib.t2n_mesh_cluster_face_keys(p(faces), F, V, p(vmap), K, p(fkeys), stream), "t2n_mesh_cluster_face_keys")
        s = torch.sort(fkeys).values
        _lib.check(lib.t2n_mesh_csr(p(s), 3 * F, K, p(foff), p(frow), p(fcnt), p(wsc), nbc, stream), "t2n_mesh_csr")

    def place(quadric=1):
        _lib.check(lib.t2n_mesh_cluster_place(p(verts), V, p(faces), F, p(off), p(mem), V, p(cells), K, p(foff), p(frow), E[0], o3, h3, 1e-3,
                                              quadric, p(out), stream), "t2n_mesh_cluster_place")

    def placement():
        face_rows()
        place()
    face_rows()
    E[0] = int(fcnt.item())
    rot = torch.empty(F, 3, dtype=torch.int32, device=dev)
    khi = torch.empty(F, dtype=torch.int64, device=dev)
    klo = torch.empty(F, dtype=torch.int64, device=dev)
    nbf = int(lib.t2n_mesh_simplify_faces_workspace_bytes(F))
    wsf = torch.empty(nbf, dtype=torch.uint8, device=dev)
    kept = torch.empty(F, 3, dtype=torch.int32, device=dev)
    kcnt = torch.empty(1, dtype=torch.int64, device=dev)

    def faces_stage():
        _lib.check(lib.t2n_mesh_simplify_face_map(p(faces), F, V, p(vmap), K, p(rot), p(khi), p(klo), stream), "t2n_mesh_simplify_face_map")
        by_lo = torch.sort(klo, stable=True).indices
        order = by_lo[torch.sort(khi[by_lo], stable=True).indices].contiguous()
        _lib.check(lib.t2n_mesh_simplify_faces(p(rot), p(order), F, p(kept), p(kcnt), p(wsf), nbf, stream), "t2n_mesh_simplify_faces")
    faces_stage()
    fns = {"keys + sort": keys_sort, "rows": rows, "placement (face keys, sort, t2n_mesh_csr, quadric place)": placement,
           "t2n_mesh_cluster_place alone, quadric": place, "t2n_mesh_cluster_place alone, mean": lambda: place(0),
           "faces (face map, two stable sorts, t2n_mesh_simplify_faces)": faces_stage}
    rows_len = (off[1:K + 1] - off[:K]).max().item(), (foff[1:] - foff[:-1]).max().item()
    return fns, (K, int(kcnt.item()), E[0]) + rows_len


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_mesh_simplify.py measures on the GPU only")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n = a.n
    field, _, _ = bench.build_field(dev, grid=n)
    level = 0.005
    vol = field.getDenseAlpha([n, n, n])[0].contiguous()
    verts, faces, _ = mesh.marching_cubes(vol, level)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if V == 0:
        sys.exit(f"no edge of the {n}^3 alpha volume crosses {level}")
    stream = _lib.current_stream_ptr(dev)
    p = _lib.ptr
    adj = mesh.mesh_adjacency(faces, V)
    E = int(adj.neighbours.shape[0])
    x = verts.double()
    y = torch.empty_like(x)

    def ten_iterations():
        a_, b_ = x, y
        for _ in range(10):
            for s in (0.5, -0.53):
                _lib.check(lib.t2n_mesh_smooth_pass(p(a_), p(b_), p(adj.offsets), p(adj.neighbours), E, None, V, s, stream), "t2n_mesh_smooth_pass")
                a_, b_ = b_, a_

    device = {"10 smoothing iterations (20 t2n_mesh_smooth_pass)": ten_iterations}
    whole = {"smooth_mesh(iterations=10), no normals": lambda: mesh.smooth_mesh((verts, faces), iterations=10)}
    sizes = {}
    for cell in (2.0, 4.0):
        fns, sizes[cell] = stages(lib, dev, verts, faces, cell)
        for k, fn in fns.items():
            device[f"cell {cell:g}: {k}"] = fn
        for pl in ("quadric", "mean"):
            whole[f"cell {cell:g}: simplify_mesh(placement={pl!r})"] = lambda cell=cell, pl=pl: mesh.simplify_mesh((verts, faces), cell, placement=pl)
    for fn in list(device.values()) + list(whole.values()):
        for _ in range(2):
            fn()
    t = {k: [] for k in list(device) + list(whole)}
    for _ in range(a.blocks):
        for k, fn in device.items():
            t[k].append(timed_device(fn, a.reps))
        for k, fn in whole.items():
            t[k].append(timed_host(fn))
    lines = [f"mesh simplification behind the device marching cubes at {n}^3 (getDenseAlpha of the bench field, level {level}, node spacing "
             f"1); {torch.cuda.get_device_name(0)}; median of {a.blocks} blocks, the stages alternating inside a block; device events "
             f"around {a.reps} calls, whole calls by a host clock around one call (synchronised at both ends); warm-up excluded; the same "
             f"mesh every call, so it is read from a warm cache hierarchy",
             f"mesh: {V} vertices, {F} triangles"]
    for cell, (K, Fk, Ef, mrow, frow) in sizes.items():
        lines.append(f"cell {cell:g}: V' = {K} ({V / K:.1f} x fewer), F' = {Fk} ({F / max(Fk, 1):.1f} x fewer), {Ef} cluster-face entries; the "
                     f"longest member row {mrow}, the longest face row {frow}")
    lines += [f"{k}: {med(v)}" for k, v in t.items()]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
