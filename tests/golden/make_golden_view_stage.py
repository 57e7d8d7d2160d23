#!/usr/bin/env python3
"""Golden vectors for the depth stage of a new view in `render_warping_inapinting`: the inline code between the inpainter and the support
set (text2nerf_main.py:230-299) and the update_known_views=True mask expansion (:147-162). Like make_golden_align.py, this script
EXECUTES the reference's own lines, read from /root/reference at run time, against synthetic inputs bound to the names the excerpts use
(tests/golden/make_golden_view_stage_cases.py); nothing of the excerpts is stored, and tests/golden/view_stage.npz holds outputs only.

    :233-240        the filled-pixel list and random.sample (`random` seeded per case)
    :233-270        the same followed by the global alignment, for the merge cases
    :275-276        depth_ref / depth_src, with depth_shift bound to a float32 array as the device alignment returns it
    :278, :282      depth_new from the merge network's float32 output
    :285, :296      img_new, current_mask_inpainted
    :147-162        the mask expansion (update_known_views=True); :147-177 once more with the render and the masked render behind it

Each excerpt is asserted on its first and last line, so a moved reference is noticed. The PNG writes inside the excerpts go to a stub.
OpenCV is not installed here: `cv2` is bound to Cv2StandIn (make_golden_view_stage_cases.py), whose `blur` is a float32 5x5 box mean
with reflect-101 borders; the excerpt thresholds it at 0.99, which no summation order can move (25/25 >= 0.9999, 24/25 = 0.96), and
tests/test_view_stage_cpu.py cross-checks the stand-in against scipy.ndimage.uniform_filter(mode="mirror").

    python tests/golden/make_golden_view_stage.py
"""
import os
import random
import sys
import textwrap
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
import make_golden_view_stage_cases as VC  # noqa: E402

REF = "/root/reference/text2nerf_main.py"
SRC = open(REF).read().splitlines()


def excerpt(lo, hi, first, last):
    """Lines lo..hi (1-based, inclusive), dedented and compiled; `first` / `last` must be what the first / last line says."""
    lines = SRC[lo - 1:hi]
    assert lines[0].strip().startswith(first) and lines[-1].strip().startswith(last), f"reference lines {lo}-{hi} moved"
    return compile(textwrap.dedent("\n".join(lines)), "<text2nerf_main.py:%d-%d>" % (lo, hi), "exec")


E_LIST = excerpt(233, 240, "pixel_filled = []", "thresh = (depth_rendered.max()-push_depth)")
E_ALIGN = excerpt(233, 270, "pixel_filled = []", "depth_shift = depth_scaled - shift")
E_MERGE = excerpt(275, 276, "depth_ref = ((depth_rendered - push_depth)", "depth_src = ((depth_shift - push_depth)")
E_NEW1 = excerpt(278, 278, "depth_new = (depth_merged.detach()", "depth_new = (depth_merged.detach()")
E_NEW2 = excerpt(282, 282, "depth_new = (depth_new / 12000 + push_depth)", "depth_new = (depth_new / 12000 + push_depth)")
E_IMG = excerpt(285, 285, "img_new = (img_new/255.)", "img_new = (img_new/255.)")
E_MASK = excerpt(296, 296, "current_mask_inpainted = 1-myMap_filt", "current_mask_inpainted = 1-myMap_filt")
E_EXPAND = excerpt(147, 162, "if update_known_views:", "imageio.imwrite(os.path.join(save_path_warp, 'mask_inv', '%05d_expand.png'")
E_PACK = excerpt(147, 177, "if update_known_views:", "rgb_render_ = (rgb_render_).astype(np.uint8)")

QUIET = {"print": lambda *a, **k: None}


def expand_env(my_map, warp_u8, rgb=None, depth=None):
    """The names :147-177 read, with the PNG writer stubbed and the renderer returning the given frame."""
    renderer = None
    if rgb is not None:
        renderer = lambda *a, **k: (torch.from_numpy(rgb), None, torch.from_numpy(depth), None, None)        # noqa: E731
    return {"np": np, "cv2": VC.Cv2StandIn, "os": os, "torch": torch, "imageio": types.SimpleNamespace(imwrite=lambda *a, **k: None),
            "update_known_views": True, "myMap_filt": my_map.copy(), "output_image_warp": warp_u8.copy(), "save_path_warp": "", "N_iter": 2,
            "H": my_map.shape[0], "W": my_map.shape[1], "all_rays_gen_split": {2: None}, "renderer": renderer, "tensorf": None,
            "args": types.SimpleNamespace(batch_size=4096), "N_samples": -1, "ndc_ray": False, "white_bg": False, "device": "cpu"}


def main():
    out = {}
    # the filled-pixel list
    for name, seed in VC.SAMPLE_CASES.items():
        m = VC.sample_mask(name)
        H = m.shape[0]
        env = dict(QUIET, np=np, random=random, H=H, W=H, myMap_filt=m, depth_rendered=np.full((H, H), 3.0), depth_est=np.full((H, H), 3.5),
                   push_depth=VC.PUSH)
        random.seed(seed)
        exec(E_LIST, env)
        out[f"sample_{name}"] = np.asarray(env["pixel_sample"], np.int32).reshape(-1, 2)
        out[f"sample_{name}_next"] = np.array([random.getrandbits(32) for _ in range(4)], np.int64)     # the generator's state afterwards
        print("sample", name, "filled", len(env["pixel_filled"]), "sampled", len(env["pixel_sample"]))
    # alignment and the merge inputs
    for name, (_, H, _, seed) in VC.MERGE_CASES.items():
        dr, m, de = VC.merge_inputs(name)
        env = dict(QUIET, np=np, random=random, H=H, W=H, myMap_filt=m, depth_rendered=dr, depth_est=de, push_depth=VC.PUSH)
        random.seed(seed)
        exec(E_ALIGN, env)
        out[f"merge_{name}_pixel_sample"] = np.asarray(env["pixel_sample"], np.int32).reshape(-1, 2)
        out[f"merge_{name}_next"] = np.array([random.getrandbits(32) for _ in range(4)], np.int64)
        out[f"merge_{name}_scale_shift"] = np.array([env["scale"], env["shift"]], np.float64)
        ds32 = np.asarray(env["depth_shift"]).astype(np.float32)
        env["depth_shift"] = ds32                       # what the device alignment hands on: float32
        exec(E_MERGE, env)
        assert env["depth_ref"].dtype == np.float64 and env["depth_src"].dtype == np.float32
        out[f"merge_{name}_depth_shift"] = ds32
        out[f"merge_{name}_depth_ref"] = env["depth_ref"].astype(np.float32)         # :277 hands depth_ref.astype(np.float32) on
        out[f"merge_{name}_depth_src"] = env["depth_src"]
        print("merge", name, "samples", len(env["pixel_sample"]), "scale %.6f shift %.6f" % (env["scale"], env["shift"]))
    # after the merge network
    dm, img, m = VC.finish_inputs()
    env = dict(QUIET, np=np, depth_merged=torch.from_numpy(dm), img_new=img, myMap_filt=m, push_depth=VC.PUSH)
    for e in (E_NEW1, E_NEW2, E_IMG, E_MASK):
        exec(e, env)
    assert env["depth_new"].dtype == np.float32 and env["img_new"].dtype == np.float32 and env["current_mask_inpainted"].dtype == np.int64
    out["finish_depth_new"], out["finish_img_new"] = env["depth_new"], env["img_new"]
    out["finish_mask_inpainted"] = env["current_mask_inpainted"].astype(np.int8)
    # the mask expansion
    for name in VC.EXPAND_CASES:
        m = VC.expand_mask(name)
        env = expand_env(m, np.zeros(m.shape + (3,), np.uint8))
        exec(E_EXPAND, env)
        assert env["myMap_filt"].dtype == np.int64 and env["mask_ex"].shape == m.shape + (3,)
        out[f"expand_{name}_eroded"] = env["myMap_filt"].astype(np.int8)
        out[f"expand_{name}_mask_ex"] = env["mask_ex"].astype(np.int8)
        print("expand", name, "set", int(m.sum()), "->", int(env["myMap_filt"].sum()))
    warp, m, rgb, depth = VC.pack_inputs()
    env = expand_env(m, (warp * 255).astype(np.uint8), rgb, depth)               # :138 turns the warp into uint8 before the expansion
    exec(E_PACK, env)
    for key, name, dt in (("output_image_warp", "output_image_warp_u8", np.uint8), ("myMap_filt", "myMap_filt", np.int8),
                          ("mask_image", "mask_image", np.uint8), ("mask_inv", "mask_inv", np.uint8), ("mask_ex", "mask_ex", np.int8),
                          ("rgb_render", "rgb_render", np.uint8), ("rgb_render_", "rgb_render_", np.uint8),
                          ("depth_rendered", "depth_rendered", np.float64)):
        assert np.array_equal(env[key].astype(dt), env[key]), key
        out[f"pack_{name}"] = env[key].astype(dt)
    print("pack: set", int(m.sum()), "->", int(env["myMap_filt"].sum()))
    np.savez_compressed(os.path.join(HERE, "view_stage.npz"), **out)
    print("view_stage.npz", os.path.getsize(os.path.join(HERE, "view_stage.npz")), "bytes")


if __name__ == "__main__":
    main()
