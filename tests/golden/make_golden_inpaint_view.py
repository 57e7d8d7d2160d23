#!/usr/bin/env python3
"""Golden vectors for the many-sources-to-one-target warp of the inpaint-view builder: the reference's
`bilinear_splat_warping_multiview` (utils.py:83-119 over scripts/Warper.py:21-186) with `masks=` on the nine-view case of
make_golden_inpaint_view_cases.py, produced by IMPORTING the reference on the CPU (cv2 / skimage / imageio are inert stubs, as in
make_golden_warp.py). Inputs are rebuilt from seeds; only outputs are stored. Writes tests/golden/inpaint_view.npz.

    python tests/golden/make_golden_inpaint_view.py
"""
import os
import sys
from unittest.mock import MagicMock

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, REF)
for name in ["cv2", "imageio", "imageio.v2", "torchvision", "torchvision.transforms", "statsmodels", "statsmodels.api",
             "skimage", "skimage.io", "skimage.metrics", "skimage.measure", "lpips", "plyfile", "kornia", "configargparse"]:
    sys.modules.setdefault(name, MagicMock())

import utils as ref_utils  # noqa: E402

from make_golden_inpaint_view_cases import H9, INTRINSIC9, W9, nine_view_case  # noqa: E402


def main():
    rgbs, depths, poses, target, masks = nine_view_case()
    mask, img, dep = ref_utils.bilinear_splat_warping_multiview(list(rgbs), list(depths), poses, target, H9, W9, INTRINSIC9, masks=masks)
    out = {"nine_mask": mask.astype(np.uint8), "nine_image": img, "nine_depth": dep}
    print("coverage", float(mask.mean()))
    np.savez_compressed(os.path.join(HERE, "inpaint_view.npz"), **out)
    print({k: (v.shape, str(v.dtype)) for k, v in out.items()})


if __name__ == "__main__":
    main()
