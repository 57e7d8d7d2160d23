"""CPU restatement of the support-set builder for the tests: `gt_warping` (utils.py:122-163, bilinear_splat branch) composed per target
from oracle.oracle_warp.forward_warp the way the reference composes Warper.forward_warp, and `produce_formatted_data`
(dataLoader/scene_gen.py:31-98) in plain torch from the oracle's ray functions. TEST INFRASTRUCTURE ONLY. Pinned against the
reference's own outputs (tests/golden/support.npz) by tests/test_support_cpu.py; the larger GPU cases are checked against it."""
import numpy as np
import torch

from oracle import oracle_torch as O
from oracle import oracle_warp as OW


def gt_warping(rgb_gt, depth_gt, pose_gt, poses_tar, H, W, intrinsic, mask_gt=None):
    """(rgbs [V,H,W,3] float32, masks [V,H,W] int64, depths [V,H,W] float64)."""
    T1 = np.linalg.inv(pose_gt)
    K = np.eye(3).astype(np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = intrinsic[0], intrinsic[1], intrinsic[2], intrinsic[3]
    src = (rgb_gt * 255).astype(np.uint8)
    rgbs, masks, depths = [], [], []
    for vv in range(poses_tar.shape[0]):
        f8, known, dep, _ = OW.forward_warp(src, depth_gt, T1, np.linalg.inv(poses_tar[vv]), K, None, mask_gt)
        f8 = f8.copy()
        f8[~known] = 255                                    # utils.py:150-151: white where nothing landed
        rgbs.append((f8 / 255).astype(np.float32))
        masks.append(known.astype(np.int64))
        depths.append(dep)
    return np.stack(rgbs), np.stack(masks), np.stack(depths)


def produce_formatted_data(images, depths, masks, poses, intrinsic, H, W):
    """mode='train': (all_rays, all_rgbs, all_depths, all_rays_split, all_rgbs_split, all_depths_split, poses_tensor), CPU float32."""
    fx, fy, cx, cy = intrinsic
    d = O.ray_directions(H, W, [fx, fy], center=[cx, cy])
    d = d / torch.norm(d, dim=-1, keepdim=True)
    rays, rgbs, deps, rays_split = [], [], [], []
    for i in range(poses.shape[0]):
        img = torch.from_numpy(np.ascontiguousarray(images[i], dtype=np.float32)).reshape(H * W, 3)
        dep = torch.from_numpy(np.ascontiguousarray(depths[i], dtype=np.float32)).reshape(H * W)
        keep = torch.from_numpy(np.ascontiguousarray(masks[i])).reshape(H * W) > 0.5
        ro, rd = O.get_rays(d, torch.FloatTensor(poses[i]))
        r6 = torch.cat([ro, rd], 1)
        rays.append(r6[keep]); rgbs.append(img[keep]); deps.append(dep[keep]); rays_split.append(r6)
    return (torch.cat(rays), torch.cat(rgbs), torch.cat(deps), torch.stack(rays_split),
            torch.from_numpy(np.asarray(images, np.float32)), torch.from_numpy(np.asarray(depths, np.float32)),
            torch.from_numpy(np.asarray(poses, np.float32)))


def support_set(rgb, depth, mask_inpainted, poses, intrinsic, H, W):
    """text2nerf_main.py:380-392 (mask_inpainted given) / scene_gen.py:305-316 (None): (images, depths, masks) fed to the formatter
    and its 7-tuple."""
    u_rgb, u_mask, u_dep = gt_warping(rgb, depth, poses[0], poses[1:], H, W, intrinsic)
    if mask_inpainted is None:
        masks = np.concatenate([np.ones_like(u_mask[:1]), u_mask], 0)
    else:
        _, m_mask, _ = gt_warping(rgb, depth, poses[0], poses[1:], H, W, intrinsic, mask_gt=mask_inpainted)
        masks = np.concatenate([np.asarray(mask_inpainted, np.int64)[None], m_mask], 0)
    images = np.concatenate([rgb[None], u_rgb], 0)
    depths = np.concatenate([depth[None], u_dep], 0)
    return (images, depths, masks), produce_formatted_data(images, depths, masks, poses, intrinsic, H, W)
