"""Inputs of the inpaint-view goldens (shared by make_golden_inpaint_view.py and the tests): nine source views into one target on a
37 x 53 frame, across the 8-source chunk of t2n_warp_sources. Source 0 looks away and lands nothing; sources 1..8 are small-baseline
views that each keep one column band of eight, so that every one of them — the ninth, first of the second chunk, included — owns
target pixels no earlier source filled, and holes remain for the fill stage."""
import numpy as np

from text2nerf_amd import synth

H9, W9 = 37, 53
INTRINSIC9 = [53.0, 53.0, 26, 18]


def nine_view_case():
    """(rgbs [9,H,W,3], depths [9,H,W], poses [9,4,4], pose_tar [4,4], masks: list of 9 boolean [H,W])."""
    g = np.random.Generator(np.random.PCG64(7))
    poses = [synth.look_pose(1.2, 0.0, (0.0, 0.0, 0.0))]
    for _ in range(8):
        yaw, pitch = g.uniform(-0.1, 0.1), g.uniform(-0.05, 0.05)
        poses.append(synth.look_pose(yaw, pitch, tuple(g.uniform(-0.15, 0.15, 3))))
    frames = [synth.rgbd_frame(71 + v, H9, W9) for v in range(9)]
    band = np.broadcast_to(np.arange(W9) * 8 // W9, (H9, W9))
    masks = [np.ones((H9, W9), bool)] + [band == v - 1 for v in range(1, 9)]
    target = synth.look_pose(0.05, 0.02, (0.06, -0.04, 0.1))
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), np.stack(poses), target, masks
