#!/usr/bin/env python3
"""Golden vectors for the device SSIM — `rgb_ssim` (utils.py:436-482) — produced by IMPORTING the reference on CPU (needs scipy; cv2 /
imageio / skimage / ... are inert stubs as in make_golden.py). Inputs are rebuilt from seeds (make_golden_ssim_cases.py); only the
reference's outputs are stored: per case the float64 map `<name>/map` and the scalar `<name>/ssim`. float32 cases hand the reference
float32 torch tensors, as `evaluation` does (renderer.py:103-105: `img0**2` is then a float32 product); float64 cases hand it float64
arrays, as extra/compute_metrics.py does. Writes tests/golden/ssim.npz (arrays only) and tests/golden/metrics_signatures.json (the
names and defaults of `rgb_ssim`).

    python tests/golden/make_golden_ssim.py
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
sys.path.insert(0, HERE)
sys.path.insert(0, REF)
for name in ["cv2", "imageio", "imageio.v2", "configargparse", "torchvision", "torchvision.transforms", "statsmodels",
             "statsmodels.api", "lpips", "plyfile", "skimage", "skimage.io", "skimage.metrics", "skimage.measure", "scripts.Warper"]:
    sys.modules.setdefault(name, MagicMock())
kornia = types.ModuleType("kornia")
kornia.create_meshgrid = lambda *a, **k: None      # imported by name only; never called here
sys.modules["kornia"] = kornia
torch.set_num_threads(2)

import utils as ref_utils  # noqa: E402

from make_golden_ssim_cases import cases, inputs  # noqa: E402


def describe(fn):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def main():
    out = {}
    for case in cases():
        name, kind, H, W, dt, mv, fs, sigma, seed = case
        a, b = inputs(case)
        if dt == "float32":
            a, b = torch.from_numpy(a), torch.from_numpy(b)
        m = ref_utils.rgb_ssim(a, b, mv, filter_size=fs, filter_sigma=sigma, return_map=True)
        s = ref_utils.rgb_ssim(a, b, mv, filter_size=fs, filter_sigma=sigma)
        assert m.dtype == np.float64 and m.shape == (H - fs + 1, W - fs + 1, 3), (name, m.dtype, m.shape)
        out[name + "/map"] = m
        out[name + "/ssim"] = np.float64(s)
    assert out["flat_same_float32/ssim"] == 1.0 and out["flat_same_float64/ssim"] == 1.0
    path = os.path.join(HERE, "ssim.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "metrics_signatures.json"), "w") as fh:
        json.dump({"rgb_ssim": describe(ref_utils.rgb_ssim)}, fh, indent=1, sort_keys=True)
    print(len(out) // 2, "cases,", os.path.getsize(path), "bytes")
    for name in sorted(k[:-5] for k in out if k.endswith("/ssim")):
        print(f"  {name:36s} ssim {float(out[name + '/ssim']):.15f} map min {out[name + '/map'].min():+.6f}")


if __name__ == "__main__":
    main()
