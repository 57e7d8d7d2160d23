"""Inputs of the support-set goldens (shared by make_golden_support.py and the tests): one synthetic RGB-D source view, the nine
support poses of the reference's pose generator (poses.npz: source = pose 0, targets = 1..8), the intrinsics and the inpaint mask."""
import os

import numpy as np

from text2nerf_amd import synth

from make_golden_warp_cases import H, W  # noqa: F401  (40 x 56)

HERE = os.path.dirname(os.path.abspath(__file__))


def inpaint_mask(h, w, seed):
    """The right third of the frame plus ~10 % speckles, int64 0/1 (shaped like the driver's `current_mask_inpainted`)."""
    m = np.zeros((h, w), np.int64)
    m[:, 2 * w // 3:] = 1
    m[np.random.Generator(np.random.PCG64(seed)).uniform(0, 1, (h, w)) > 0.9] = 1
    return m


def support_inputs(h, w, seed_frame, seed_mask, n_boxes=3):
    """(rgb [h,w,3] f32, depth [h,w] f32, poses [9,4,4] f32, intrinsic, mask [h,w] int64)."""
    rgb, depth = synth.rgbd_frame(seed_frame, h, w, n_boxes=n_boxes)
    poses = np.load(os.path.join(HERE, "poses.npz"))["local_fixed_support_angle0"]
    return rgb, depth, poses, [float(max(h, w)), float(max(h, w)), w // 2, h // 2], inpaint_mask(h, w, seed_mask)
