#!/usr/bin/env python3
"""Time the mesh component stage (csrc/t2n_mesh.hip) on the mesh of tools/time_mesh.py's 300^3 volume: labelling
(`t2n_mesh_components`), sizes (`t2n_mesh_component_sizes`) and the filter (`t2n_mesh_filter_count` + `t2n_mesh_filter_emit`, keeping
the largest component) with device events around `reps` calls each, and the whole `mesh.mesh_components` / `mesh.filter_components`
calls (allocations, the index check, the host reads) with a host clock. Fresh process, warm-up excluded, median over the blocks. The
marching-cubes count + emit of the same volume is timed in the same process for the comparison. No target: the file records what was
measured.

    python tools/time_mesh_components.py [--blocks 5] [--reps 50] [--n 300] [--out profiles/mesh_components_timing.txt]"""
import argparse
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from text2nerf_amd import TensorVMSplit, _lib, mesh, synth  # noqa: E402
from time_mesh import AABB, GRID, NF, med, timed_device, timed_host  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_mesh_components.py measures on the GPU only")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    params = synth.make_field_params(11, GRID, density_scale=0.9, aabb=AABB)
    m = TensorVMSplit(torch.tensor(AABB), GRID, dev, density_n_comp=[16] * 3, appearance_n_comp=[48] * 3, app_dim=27, near_far=NF,
                      shadingMode="MLP_Fea_noview", density_shift=-10, distance_scale=25, pos_pe=0, view_pe=0, fea_pe=6, featureC=128,
                      step_ratio=1.0, fea2denseAct="softplus")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    n = a.n
    vol = m.getDenseAlpha([n, n, n])[0].contiguous()
    lines = [f"mesh components behind the device marching cubes at {n}^3 (getDenseAlpha of a synthetic {GRID} field, the volume of "
             f"profiles/mesh_timing.txt); {torch.cuda.get_device_name(0)}; median of {a.blocks} blocks; components / sizes / filter / "
             f"marching-cubes count + emit: device events around {a.reps} calls; mesh_components / filter_components: host clock around "
             f"one call (synchronised at both ends); warm-up excluded; the same mesh every call, so it is read from a warm cache hierarchy"]
    stream = _lib.current_stream_ptr(dev)
    for label, level in (("level 0.005", 0.005), ("level = median", float(vol.median()))):
        mc_ws = torch.empty(int(lib.t2n_mc_workspace_bytes(n, n, n)), dtype=torch.uint8, device=dev)
        mc_counts = torch.empty(2, dtype=torch.int64, device=dev)
        verts, faces, norms = mesh.marching_cubes(vol, level)
        V, F = int(verts.shape[0]), int(faces.shape[0])
        if V == 0:
            lines.append(f"{label} ({level:.6g}): no edge crosses it, nothing measured")
            continue
        org, sp = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)

        def mc():
            _lib.check(lib.t2n_mc_count(_lib.ptr(vol), n, n, n, level, _lib.ptr(mc_ws), _lib.ptr(mc_counts), stream), "t2n_mc_count")
            _lib.check(lib.t2n_mc_emit(_lib.ptr(vol), n, n, n, level, _lib.ptr(mc_ws), org, sp, 0, _lib.ptr(verts), _lib.ptr(norms),
                                       _lib.ptr(faces), stream), "t2n_mc_emit")

        nbytes = int(lib.t2n_mesh_components_workspace_bytes(V, F))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        labels = torch.empty(V, dtype=torch.int32, device=dev)
        k_dev = torch.empty(1, dtype=torch.int64, device=dev)

        def components():
            _lib.check(lib.t2n_mesh_components(_lib.ptr(faces), F, V, _lib.ptr(labels), _lib.ptr(k_dev), _lib.ptr(ws), nbytes, stream),
                       "t2n_mesh_components")
        components()
        K = int(k_dev.cpu().item())
        vc = torch.empty(K, dtype=torch.int32, device=dev)
        fc = torch.empty(K, dtype=torch.int32, device=dev)

        def sizes():
            _lib.check(lib.t2n_mesh_component_sizes(_lib.ptr(faces), F, _lib.ptr(labels), V, K, _lib.ptr(vc), _lib.ptr(fc), stream),
                       "t2n_mesh_component_sizes")
        sizes()
        top = fc.sort(descending=True, stable=True)
        keep = torch.zeros(K, dtype=torch.uint8, device=dev)
        keep[top.indices[0]] = 1
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        args = (_lib.ptr(faces), F, _lib.ptr(labels), V, _lib.ptr(keep), K)
        _lib.check(lib.t2n_mesh_filter_count(*args, _lib.ptr(ws), nbytes, _lib.ptr(totals), stream), "t2n_mesh_filter_count")
        Vk, Fk = (int(x) for x in totals.cpu().tolist())
        out_v, out_n = torch.empty(Vk, 3, device=dev), torch.empty(Vk, 3, device=dev)
        out_f = torch.empty(Fk, 3, dtype=torch.int32, device=dev)

        def filt():
            _lib.check(lib.t2n_mesh_filter_count(*args, _lib.ptr(ws), nbytes, _lib.ptr(totals), stream), "t2n_mesh_filter_count")
            _lib.check(lib.t2n_mesh_filter_emit(*args, _lib.ptr(verts), _lib.ptr(norms), None, _lib.ptr(ws), nbytes, _lib.ptr(out_v),
                                                _lib.ptr(out_n), None, _lib.ptr(out_f), stream), "t2n_mesh_filter_emit")

        def whole_components():
            return mesh.mesh_components(faces, V)

        def whole_filter():
            return mesh.filter_components((verts, faces, norms), keep_largest=1)
        for _ in range(3):
            mc(); components(); sizes(); filt(); whole_components(); whole_filter()
        t = {k: [] for k in ("mc", "components", "sizes", "filter", "whole_components", "whole_filter")}
        for _ in range(a.blocks):
            t["mc"].append(timed_device(mc, a.reps))
            t["components"].append(timed_device(components, a.reps))
            t["sizes"].append(timed_device(sizes, a.reps))
            t["filter"].append(timed_device(filt, a.reps))
            t["whole_components"].append(timed_host(whole_components))
            t["whole_filter"].append(timed_host(whole_filter))
        big = top.values[:3].tolist()
        line = (f"{label} ({level:.6g}): {V} vertices, {F} triangles, {K} components (most faces: {big}); keep_largest=1 leaves {Vk} "
                f"vertices, {Fk} triangles; marching cubes count + emit with normals {med(t['mc'])}; t2n_mesh_components "
                f"{med(t['components'])}; t2n_mesh_component_sizes (equal labels combined inside a wave) {med(t['sizes'])}; "
                f"t2n_mesh_filter_count + t2n_mesh_filter_emit with normals {med(t['filter'])}; mesh_components "
                f"{med(t['whole_components'])}; filter_components {med(t['whole_filter'])}")
        lines.append(line)
        print(line, flush=True)
    lines.append("The size kernel without the in-wave combining (one atomic per lane) was not built: not measured.")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
