#!/usr/bin/env python3
"""The reference's own density_L1 / vector_comp_diffs (models/tensoRF.py:76-92,173-191,418-422) on small seeded models, by IMPORTING
the reference on the CPU (see make_golden.py for the stubbing) and running them under autograd, in float32 and in float64
(`.double()`). Parameters are rebuilt in the tests from text2nerf_amd.synth with the seeds below; only values and gradients are stored.
Writes tests/golden/reg_terms.npz.    python tests/golden/make_golden_reg.py

Models: TensorVMSplit 23 x 19 x 17 with 16 / 48 components ("split"); TensorVMSplit of the general shape [5,3,4] / [7,6,2] on the same
grid ("general"); TensorVM 17^3 with 16 / 48 ("vm": vector_comp_diffs only, the class has no density_L1); TensorCP 23 x 19 x 17
("cp": density_L1 only)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import TINY, quiet  # noqa: E402  (also seeds sys.path / module stubs)
from models.tensoRF import TensorCP, TensorVM, TensorVMSplit  # noqa: E402
from text2nerf_amd import synth  # noqa: E402

GRID = [23, 19, 17]
VM_GRID = [17, 17, 17]
SEEDS = dict(split=61, general=62, vm=63, cp=64)
GENERAL = dict(density_n_comp=[5, 3, 4], appearance_n_comp=[7, 6, 2])
COMMON = dict(app_dim=27, near_far=TINY["near_far"], shadingMode="MLP_Fea_noview", alphaMask_thres=1e-4, density_shift=-10,
              distance_scale=25, pos_pe=0, view_pe=0, fea_pe=6, featureC=128, step_ratio=1.0, fea2denseAct="softplus")


def vm_state(sd):
    out = {k: v for k, v in sd.items() if not k.startswith(("density_", "app_"))}
    out["plane_coef"] = np.concatenate([np.concatenate([sd[f"app_plane.{k}"], sd[f"density_plane.{k}"]], 1) for k in range(3)], 0)
    out["line_coef"] = np.concatenate([np.concatenate([sd[f"app_line.{k}"], sd[f"density_line.{k}"]], 1) for k in range(3)], 0)
    return out


def cp_state(sd):
    return {k: v for k, v in sd.items() if "plane" not in k and not k.startswith("basis_mat")}


def record(out, tag, model, names):
    """values and autograd gradients of the methods `names`, in the model's own precision (`tag` ends in /f32 or /f64)."""
    for name in names:
        model.zero_grad()
        v = getattr(model, name)()
        v.backward()
        out[f"{tag}/{name}"] = v.detach().numpy()
        for k, p in model.named_parameters():
            if p.grad is not None and ("plane" in k or "line" in k):
                out[f"{tag}/{name}/grad/{k}"] = p.grad.numpy().copy()


def main():
    out = {}
    aabb = torch.tensor(TINY["aabb"])
    sd = synth.make_field_params(SEEDS["split"], GRID, density_scale=0.9, aabb=TINY["aabb"])
    m = quiet(TensorVMSplit, aabb, GRID, "cpu", density_n_comp=[16] * 3, appearance_n_comp=[48] * 3, **COMMON)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    record(out, "split/f32", m, ("density_L1", "vector_comp_diffs"))
    record(out, "split/f64", m.double(), ("density_L1", "vector_comp_diffs"))

    sd = synth.make_field_params(SEEDS["general"], GRID, density_n_comp=GENERAL["density_n_comp"], app_n_comp=GENERAL["appearance_n_comp"],
                                 density_scale=0.9, aabb=TINY["aabb"])
    m = quiet(TensorVMSplit, aabb, GRID, "cpu", **GENERAL, **COMMON)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    record(out, "general/f32", m, ("density_L1", "vector_comp_diffs"))
    record(out, "general/f64", m.double(), ("density_L1", "vector_comp_diffs"))

    sd = vm_state(synth.make_field_params(SEEDS["vm"], VM_GRID, density_scale=0.9, aabb=TINY["aabb"]))
    m = quiet(TensorVM, aabb, VM_GRID, "cpu", density_n_comp=16, appearance_n_comp=48, **COMMON)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    record(out, "vm/f32", m, ("vector_comp_diffs",))
    record(out, "vm/f64", m.double(), ("vector_comp_diffs",))

    full = synth.make_field_params(SEEDS["cp"], GRID, density_scale=0.9, aabb=TINY["aabb"])
    m = quiet(TensorCP, aabb, GRID, "cpu", density_n_comp=[16] * 3, appearance_n_comp=[48] * 3, **COMMON)
    have = m.state_dict()
    sd = {k: torch.from_numpy(full[k]) if k in full and tuple(full[k].shape) == tuple(v.shape) else v for k, v in have.items()}
    m.load_state_dict(sd, strict=True)
    assert all(np.array_equal(m.state_dict()[f"density_line.{k}"].numpy(), full[f"density_line.{k}"]) for k in range(3))
    record(out, "cp/f32", m, ("density_L1",))
    record(out, "cp/f64", m.double(), ("density_L1",))

    path = os.path.join(HERE, "reg_terms.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays,", os.path.getsize(path), "bytes")
    print({k: (v.shape, v.dtype) for k, v in out.items() if "/grad/" not in k})


if __name__ == "__main__":
    main()
