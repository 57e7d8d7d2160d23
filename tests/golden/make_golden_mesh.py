#!/usr/bin/env python3
"""The reference's `convert_sdf_samples_to_ply` (utils.py:512-572): its parameter names, kinds and defaults, read by IMPORTING the
reference on CPU (plyfile / skimage / cv2 / ... are inert stubs as in make_golden.py; the function is never called: it needs skimage).
Writes tests/golden/mesh_signatures.json.

    python tests/golden/make_golden_mesh.py
"""
import inspect
import json
import os
import sys
import types
from unittest.mock import MagicMock

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
for name in ["cv2", "imageio", "imageio.v2", "configargparse", "torchvision", "torchvision.transforms", "statsmodels",
             "statsmodels.api", "lpips", "plyfile", "skimage", "skimage.io", "skimage.metrics", "skimage.measure", "scripts.Warper",
             "scipy", "scipy.signal"]:
    sys.modules.setdefault(name, MagicMock())
kornia = types.ModuleType("kornia")
kornia.create_meshgrid = lambda *a, **k: None      # imported by name only; never called here
sys.modules["kornia"] = kornia

import utils as ref_utils  # noqa: E402


def describe(fn):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def main():
    path = os.path.join(HERE, "mesh_signatures.json")
    with open(path, "w") as fh:
        json.dump({"convert_sdf_samples_to_ply": describe(ref_utils.convert_sdf_samples_to_ply)}, fh, indent=1, sort_keys=True)
    print(open(path).read())


if __name__ == "__main__":
    main()
