#!/usr/bin/env python3
"""Golden vectors for the support-set builder — the steps after inpainting in the driver (text2nerf_main.py:380-392):
`gt_warping` (utils.py:122-163, the bilinear_splat branch over scripts/Warper.py:21-180) and `produce_formatted_data`
(dataLoader/scene_gen.py:31-98) — produced by IMPORTING the reference on CPU. cv2 / imageio / skimage / ... are inert stubs;
`kornia.create_meshgrid` gets the stand-in of make_golden.py; torchvision is not installed where this runs, so the one thing
`produce_formatted_data` takes from it, `transforms.ToTensor`, is a three-line stand-in with its documented semantics for float
arrays (HWC or HW ndarray -> CHW tensor, no scaling). Inputs are rebuilt from seeds (make_golden_support_cases.py); only outputs are
stored: images as uint8 levels (`(u8 / 255).astype(float32)` rebuilds the reference's float32 image bit for bit — asserted here) and
masks as uint8. Writes tests/golden/support.npz and tests/golden/support_signatures.json.

    python tests/golden/make_golden_support.py
"""
import inspect
import json
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, REF)
for name in ["cv2", "imageio", "imageio.v2", "statsmodels", "statsmodels.api", "skimage", "skimage.io", "skimage.metrics",
             "skimage.measure", "lpips", "plyfile", "configargparse"]:
    sys.modules.setdefault(name, MagicMock())


def _create_meshgrid(height, width, normalized_coordinates=True, device=None, dtype=torch.float32):
    assert not normalized_coordinates
    xs = torch.linspace(0, width - 1, width, dtype=dtype)
    ys = torch.linspace(0, height - 1, height, dtype=dtype)
    return torch.stack(torch.meshgrid([xs, ys], indexing="ij"), dim=-1).permute(1, 0, 2).unsqueeze(0)  # [1,H,W,2], last dim (x, y)


class _ToTensor:
    def __call__(self, a):
        a = a[:, :, None] if a.ndim == 2 else a
        return torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)))


kornia = types.ModuleType("kornia")
kornia.create_meshgrid = _create_meshgrid
sys.modules["kornia"] = kornia
tv, tvt = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
tvt.ToTensor = _ToTensor
tv.transforms = tvt
sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tvt

import utils as ref_utils  # noqa: E402
from dataLoader.scene_gen import produce_formatted_data  # noqa: E402

from make_golden_support_cases import H, W, support_inputs  # noqa: E402


def describe(fn):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def levels(img):
    u8 = np.rint(img * 255.0).astype(np.uint8)
    assert np.array_equal((u8 / 255).astype(np.float32), img)
    return u8


def main():
    rgb, depth, poses, intrinsic, mask = support_inputs(H, W, 61, 62)
    args = (rgb, depth, poses[0], poses[1:], H, W)
    u_rgb, u_mask, u_dep = ref_utils.gt_warping(*args, intrinsic=intrinsic, warp_depth=True, bilinear_splat=True)
    m_rgb, m_mask, m_dep = ref_utils.gt_warping(*args, intrinsic=intrinsic, mask_gt=mask, warp_depth=True, bilinear_splat=True)
    images = np.concatenate([rgb[None], u_rgb], 0)
    depths = np.concatenate([depth[None], u_dep], 0)
    masks = np.concatenate([mask[None], m_mask], 0)
    rays, rgbs, deps, rays_split, _, _, poses_t = produce_formatted_data(images, depths, masks, poses, intrinsic, H, W, mode="train")
    out = {"unmasked_rgb_u8": levels(u_rgb), "unmasked_mask": u_mask.astype(np.uint8), "unmasked_depth": u_dep,
           "masked_rgb_u8": levels(m_rgb), "masked_mask": m_mask.astype(np.uint8), "masked_depth": m_dep,
           "all_rays": rays.numpy(), "all_rgbs": rgbs.numpy(), "all_depths": deps.numpy(), "all_rays_split": rays_split.numpy(),
           "poses_tensor": poses_t.numpy()}
    assert u_rgb.dtype == np.float32 and u_mask.dtype == np.int64 and u_dep.dtype == np.float64
    np.savez_compressed(os.path.join(HERE, "support.npz"), **out)
    with open(os.path.join(HERE, "support_signatures.json"), "w") as fh:
        json.dump({"gt_warping": describe(ref_utils.gt_warping), "produce_formatted_data": describe(produce_formatted_data)}, fh,
                  indent=1, sort_keys=True)
    print({k: (v.shape, str(v.dtype)) for k, v in out.items()})
    print("unmasked fill", [round(float(m.mean()), 3) for m in u_mask], "masked fill", [round(float(m.mean()), 3) for m in m_mask])
    print("K", rays.shape[0], "of", masks.size, "per view", [int((m > 0.5).sum()) for m in masks])
    print("bytes", os.path.getsize(os.path.join(HERE, "support.npz")))


if __name__ == "__main__":
    main()
