"""the image-space steps either side of the renderer inside `render_warping_inapinting`
(text2nerf_main.py:102-141) with the reference's call surface, running as HIP kernels (csrc/t2n_image.hip):

* ``sparse_bilateral_filtering`` — dataLoader/bilateral_filtering.py:5-35 (an O(H W) Python loop in the reference)
* ``bilinear_splat_warping_multiview`` — utils.py:83-119 over ``Warper.forward_warp`` (scripts/Warper.py:21-186, numpy add.at)
* ``dibr_filter_mask2`` — utils.py:393-409, the raster-order hole filling (skewed wavefronts on the GPU); ``dibr_filter_mask`` —
  utils.py:345-392, its four-stage sibling (unused by the driver)

and the steps after inpainting that turn one inpainted RGB-D view into training rays (csrc/t2n_support.hip):

* ``gt_warping`` — utils.py:122-163 (the bilinear_splat branch every call site takes): one source view to many target poses
* ``produce_formatted_data`` — dataLoader/scene_gen.py:31-98: rays per pose and the ``mask > 0.5`` row selection
* ``build_support_set`` — text2nerf_main.py:380-392 / scene_gen.py:305-316 as one device-resident call

and everything before inpainting as one device-resident call (csrc/t2n_image.hip, csrc/t2n_support.hip):

* ``build_inpaint_view`` — text2nerf_main.py:99-184: known views rendered, filtered as a stack
  (``sparse_bilateral_filtering_views``), warped into the new pose in one launch set per 8 sources (``warp_sources``), hole-filled,
  the new pose rendered, and the inpainter's uint8 image and masks packed (``pack_inpaint_inputs``), with the
  ``update_known_views=True`` mask expansion (:147-162) as a keyword

and the depth stage between the inpainter and the support set (csrc/t2n_view.hip):

* ``sample_filled_pixels`` — text2nerf_main.py:233-239: the filled-pixel list addressed by rank, the draw on the caller's ``random``
* ``prepare_depth_merge`` — :230-276: sampling, the global alignment and the merge network's inputs in one call
* ``finish_view`` — :278-299 and :380-392: the merged depth to ``depth_new`` / ``img_new`` / the inpainted mask, the filter, the support
  set and the training set's new rows in one call

Inputs may be numpy arrays (as in the driver) or torch tensors; numpy in -> numpy out. No CPU fallback."""
from __future__ import annotations

import ctypes as C
import os
import random
from typing import Any, NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import T2NError


def _dev(device=None):
    if not torch.cuda.is_available():
        raise T2NError("text2nerf_amd.warp runs on an MI355X only (no CPU fallback)")
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _to(x, dev, dtype):
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    return t.to(device=dev, dtype=dtype).contiguous()


def sparse_bilateral_filtering(depth, image, filter_size=[7, 7, 5, 5, 5], depth_threshold=0.04, num_iter=5, HR=False, mask=None,
                               device=None):
    """Same signature / return as dataLoader/bilateral_filtering.py:5: ``(save_images, save_depths)``, lists of length
    ``num_iter``. ``save_depths[i]`` is the depth before pass i; every ``save_images`` entry is the SAME array holding the
    image after all passes (the reference appends one array and filters it in place). ``mask`` / ``HR`` are not used by the
    driver and are rejected."""
    if mask is not None or HR:
        raise T2NError("sparse_bilateral_filtering: mask / HR are not on the Text2NeRF path and are not implemented")
    lib = _lib.load()
    as_numpy = isinstance(depth, np.ndarray)
    dev = _dev(device if device is not None else (None if as_numpy else depth.device))
    d = _to(depth, dev, torch.float32)
    im = _to(image, dev, torch.float32)
    H, W = d.shape
    if im.shape != (H, W, 3):
        raise T2NError(f"image shape {tuple(im.shape)} does not match depth {(H, W)}")
    sizes = [int(filter_size[i]) if isinstance(filter_size, (list, tuple)) else int(filter_size) for i in range(num_iter)]
    arr = (C.c_int * num_iter)(*sizes)
    photo = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
    states = torch.empty(num_iter, H, W, device=dev, dtype=torch.float32)
    ws = torch.empty(int(lib.t2n_image_filter_workspace_bytes(H, W)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.t2n_sparse_bilateral_filtering(_lib.ptr(d), _lib.ptr(im), H, W, arr, num_iter, float(depth_threshold),
                                                      _lib.ptr(photo), _lib.ptr(states), _lib.ptr(ws), ws.numel(),
                                                      _lib.current_stream_ptr(dev)), "t2n_sparse_bilateral_filtering")
    if as_numpy:
        p = photo.cpu().numpy()
        s = states.cpu().numpy()
        return [p] * num_iter, [s[i] for i in range(num_iter)]
    return [photo] * num_iter, [states[i] for i in range(num_iter)]


def bilinear_splat_warping_multiview(rgbs, depths, poses, pose_tar, H, W, intrinsic, masks=None, device=None):
    """Same signature / return as utils.py:83: ``(mask_final [H,W] int, output_image [H,W,3] fp32 in [0,1], output_depth
    [H,W] fp64)``. rgbs in [0,1]; poses are camera-to-world 4x4 (inverted here exactly like the reference: numpy, the
    inputs' dtype)."""
    lib = _lib.load()
    as_numpy = isinstance(rgbs[0], np.ndarray)
    dev = _dev(device if device is not None else (None if as_numpy else rgbs[0].device))
    pose_tar = np.asarray(pose_tar.cpu() if isinstance(pose_tar, torch.Tensor) else pose_tar)
    T2 = np.linalg.inv(pose_tar)
    K = np.eye(3).astype(np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = intrinsic[0], intrinsic[1], intrinsic[2], intrinsic[3]
    Ki = np.linalg.inv(K)
    filled = torch.zeros(H, W, dtype=torch.uint8, device=dev)
    img8 = torch.zeros(H, W, 3, dtype=torch.uint8, device=dev)
    dep = torch.zeros(H, W, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.t2n_warp_workspace_bytes(H, W)), dtype=torch.uint8, device=dev)
    d9 = lambda m: (C.c_double * 9)(*np.asarray(m, np.float64).reshape(-1)[:9])       # noqa: E731
    with torch.cuda.device(dev):
        st = _lib.current_stream_ptr(dev)
        for v in range(len(rgbs)):
            pv = np.asarray(poses[v].cpu() if isinstance(poses[v], torch.Tensor) else poses[v])
            T = np.matmul(T2, np.linalg.inv(np.linalg.inv(pv)))       # transformation2 @ inv(transformation1), Warper.py:75
            T12 = (C.c_double * 12)(*np.asarray(T, np.float64)[:3, :4].reshape(-1))
            m1 = None if masks is None else _to(masks[v], dev, torch.uint8)
            rgb = _to(rgbs[v], dev, torch.float32)
            d = _to(depths[v], dev, torch.float32)
            _lib.check(lib.t2n_warp_view(_lib.ptr(rgb), _lib.ptr(d), _lib.ptr(m1), H, W, d9(Ki), T12, d9(K), _lib.ptr(filled),
                                         _lib.ptr(img8), _lib.ptr(dep), _lib.ptr(ws), ws.numel(), st), "t2n_warp_view")
        out_img = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
        out_mask = torch.empty(H, W, dtype=torch.int64, device=dev)
        _lib.check(lib.t2n_warp_finish(_lib.ptr(filled), _lib.ptr(img8), H, W, _lib.ptr(out_img), _lib.ptr(out_mask), st),
                   "t2n_warp_finish")
    if as_numpy:
        return out_mask.cpu().numpy(), out_img.cpu().numpy(), dep.cpu().numpy()
    return out_mask, out_img, dep


def dibr_filter_mask2(output_image, myMap, output_depth=None, device=None):
    """Same signature / return as utils.py:393: ``(output_image, myMap[, output_depth])`` after the raster-order hole filling.
    The reference mutates its numpy arguments in place; here the (new) results are returned — the driver rebinds all three
    (text2nerf_main.py:135)."""
    lib = _lib.load()
    as_numpy = isinstance(output_image, np.ndarray)
    dev = _dev(device if device is not None else (None if as_numpy else output_image.device))
    img = _to(output_image, dev, torch.float32).clone()
    known = _to(myMap, dev, torch.int32).clone()
    H, W = known.shape
    dep = None if output_depth is None else _to(output_depth, dev, torch.float64).clone()
    with torch.cuda.device(dev):
        _lib.check(lib.t2n_dibr_filter_mask2(_lib.ptr(img), _lib.ptr(known), _lib.ptr(dep), H, W, 0.65, _lib.current_stream_ptr(dev)),
                   "t2n_dibr_filter_mask2")
    if as_numpy:
        m = known.cpu().numpy().astype(np.asarray(myMap).dtype)
        out = (img.cpu().numpy(), m)
        return out if dep is None else out + (dep.cpu().numpy(),)
    out = (img, known.to(myMap.dtype))
    return out if dep is None else out + (dep,)


def dibr_filter_mask(output_image, myMap, device=None):
    """Same signature / return as utils.py:345: ``(output_image, myMap)`` after the 5x5 fill scan (threshold 0.6), the 3x3 fill scan, the
    border lines and the erase scan (pixels set to 255 / unknown). The reference's driver does not call it; it is here for scripts that
    do. Results are returned, not written into the numpy arguments."""
    lib = _lib.load()
    as_numpy = isinstance(output_image, np.ndarray)
    dev = _dev(device if device is not None else (None if as_numpy else output_image.device))
    img = _to(output_image, dev, torch.float32).clone()
    known = _to(myMap, dev, torch.int32).clone()
    H, W = known.shape
    with torch.cuda.device(dev):
        _lib.check(lib.t2n_dibr_filter_mask(_lib.ptr(img), _lib.ptr(known), H, W, _lib.current_stream_ptr(dev)), "t2n_dibr_filter_mask")
    if as_numpy:
        return img.cpu().numpy(), known.cpu().numpy().astype(np.asarray(myMap).dtype)
    return img, known.to(myMap.dtype)


def align_depth_global(depth_rendered, depth_est, pixel_sample, push_depth=2.0, device=None):
    """The global stage of the depth alignment in ``render_warping_inapinting`` (text2nerf_main.py:241-270) on the device: scale and
    shift of the monocular estimate against the rendered depth over the caller's sampled pixel list (``random.sample`` of the filled
    pixels, :234-240 — host-side and the caller's, like the reference's). Returns ``(scale, shift, depth_shift)`` with ``depth_shift``
    a float32 [H,W] device tensor (= depth_est * scale - shift) and scale / shift Python floats (one 32-byte read-back).
    ``pixel_sample`` may also be a device int32 [K,2] tensor of (row, col) — what ``sample_filled_pixels`` returns for a device mask —
    which is read in place, with no host hop."""
    lib = _lib.load()
    dev = _dev(device)
    dr = _to(depth_rendered, dev, torch.float32)
    de = _to(depth_est, dev, torch.float32)
    if isinstance(pixel_sample, torch.Tensor) and pixel_sample.is_cuda:
        if pixel_sample.dtype != torch.int32 or pixel_sample.dim() != 2 or pixel_sample.shape[1] != 2:
            raise T2NError(f"align_depth_global: a device pixel_sample must be int32 [K,2], got {pixel_sample.dtype} "
                           f"{tuple(pixel_sample.shape)}")
        ps = pixel_sample.to(dev).contiguous()
    else:
        ps = torch.as_tensor(np.asarray(pixel_sample, dtype=np.int32).reshape(-1, 2)).to(dev).contiguous()
    H, W = dr.shape
    out = torch.empty(H, W, device=dev, dtype=torch.float32)
    ss = torch.empty(4, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(lib.t2n_depth_align_global(_lib.ptr(dr), _lib.ptr(de), H, W, _lib.ptr(ps), int(ps.shape[0]), float(push_depth),
                                              _lib.ptr(out), _lib.ptr(ss), _lib.current_stream_ptr(dev)), "t2n_depth_align_global")
    s = ss.cpu().tolist()
    return s[0], s[1], out


# ---- between the inpainter and the support set: sampling, alignment, the merge network's inputs ----------------------------------------
def _known32(m, dev):
    """A validity map (int64 ``myMap_filt``, int32 ``known``, boolean or a float 0/1 map) as device int32; int32 on `dev` is used in
    place."""
    t = torch.from_numpy(np.ascontiguousarray(m)) if isinstance(m, np.ndarray) else m
    if t.dim() != 2:
        raise T2NError(f"the validity map must be [H,W], got {tuple(t.shape)}")
    if t.is_floating_point() or t.dtype == torch.bool:
        t = t.to(dev) > 0
    return t.to(device=dev, dtype=torch.int32).contiguous()


def _filled_pixels(lib, dev, known, max_samples, rng):
    """Count, draw on the host, select: device int32 [K,2] (row, col). The one host read is the 8-byte count."""
    H, W = known.shape
    ws = torch.empty(int(lib.t2n_filled_pixels_workspace_bytes(H, W)), dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _lib.current_stream_ptr(dev)
        _lib.check(lib.t2n_filled_pixels_count(_lib.ptr(known), H, W, _lib.ptr(ws), _lib.ptr(count), st), "t2n_filled_pixels_count")
        n = int(count.item())
        ranks = rng.sample(range(n), min(n, int(max_samples)))      # random.sample(pixel_filled, num_max) draws exactly these indices
        out = torch.empty(len(ranks), 2, dtype=torch.int32, device=dev)
        if ranks:
            r = torch.tensor(ranks, dtype=torch.int32).to(dev)
            _lib.check(lib.t2n_filled_pixels_select(_lib.ptr(known), H, W, _lib.ptr(ws), _lib.ptr(r), len(ranks), _lib.ptr(out), st),
                       "t2n_filled_pixels_select")
    return out


def sample_filled_pixels(myMap_filt, max_samples=10000, rng=random, device=None):
    """``pixel_sample`` of text2nerf_main.py:233-239 without the image leaving the device: int32 [K,2] of (row, col), K = min(number of
    pixels with ``myMap_filt > 0``, ``max_samples``), bit-compatible with the reference's ``random.sample(pixel_filled, num_max)`` for
    the same generator state, and leaving the generator in the same state.

    The reference lists the filled pixels with ``for i in range(H): for j in range(W): if myMap_filt[j, i] > 0``, whose index ranges
    only make sense for H == W. The order is defined here as COLUMN-MAJOR over the whole image for any H, W: column ascending, and
    inside a column row ascending. ``random.sample(list, k)`` picks ``[list[r] for r in random.sample(range(len(list)), k)]``, so the
    device counts (per-column counts, one scan; the total is the one 8-byte read), ``rng`` draws the ranks on the host (``rng``: the
    ``random`` module or a ``random.Random``; one upload of at most ``max_samples`` int32), and a kernel maps each rank to its pixel.
    ``myMap_filt``: the int64 map of ``InpaintView``, the int32 ``known`` form, boolean or a float 0/1 map. A device mask in -> a device
    tensor out, which ``align_depth_global`` reads in place; a numpy mask in -> a numpy array out. No CPU fallback."""
    lib = _lib.load()
    as_numpy = not _is_cuda(myMap_filt)
    dev = _dev(device if device is not None else _first_device(myMap_filt))
    out = _filled_pixels(lib, dev, _known32(myMap_filt, dev), max_samples, rng)
    return out.cpu().numpy() if as_numpy and device is None else out


class DepthMerge(NamedTuple):
    """What ``render_warping_inapinting`` holds when it reaches the merge network (text2nerf_main.py:230-277).

    ============  =======  =======  ===================================================================================
    scale, shift           float    the global alignment (:254, :268)
    pixel_sample  [K,2]    int32    the sampled filled pixels, (row, col) (:239)
    depth_shift   [H,W]    float32  ``depth_est * scale - shift`` (:270)
    depth_ref     [H,W]    float32  ``((depth_rendered - push) * 12000 / 32768. - 1.) * myMap_filt``, rounded once (:275, :277)
    depth_src     [H,W]    float32  ``(depth_shift - push) * 12000 / 32768. - 1.`` (:276)
    mask          [H,W]    float32  ``myMap_filt``: what ``run_finetune_numpy`` receives as ``mask_ref`` (:277)
    ============  =======  =======  ===================================================================================
    """
    scale: float
    shift: float
    pixel_sample: Any
    depth_shift: Any
    depth_ref: Any
    depth_src: Any
    mask: Any


def prepare_depth_merge(depth_rendered, myMap_filt, depth_est, push_depth, rng=random, max_samples=10000, device=None):
    """From "the depth estimate is here" to "the merge network's inputs are on the device" (text2nerf_main.py:230-276) in one call:
    ``sample_filled_pixels`` -> the global alignment (``align_depth_global``'s kernels) -> one elementwise launch for ``depth_ref`` /
    ``depth_src`` / the float32 mask; returns a ``DepthMerge``.

    ``depth_rendered`` [H,W] is ``InpaintView.depth_rendered`` (float64: the rendered depth times the map; the alignment reads it as
    float32, which is exact for that product), ``myMap_filt`` its map, ``depth_est`` [H,W] the monocular estimate after
    ``/ 12000 + push_depth`` (:230; read as float32, as ``align_depth_global`` does). The arithmetic follows numpy's dtype rules for
    these inputs: ``depth_ref`` in float64, rounded to float32 once; ``depth_src`` in float32 operation by operation. An empty map
    gives the reference's fallbacks (no samples: ``scale = thresh``, ``shift = max scaled - max rendered``). Host reads: the 8-byte
    count and the 32-byte scale / shift record. numpy / CPU inputs -> numpy arrays out; a device tensor among the inputs (or
    ``device=``) -> device tensors out. No CPU fallback."""
    lib = _lib.load()
    inputs = (depth_rendered, myMap_filt, depth_est)
    to_host = device is None and not any(_is_cuda(x) for x in inputs)
    dev = _dev(device if device is not None else _first_device(*inputs))
    known = _known32(myMap_filt, dev)
    H, W = known.shape
    dr64 = _to(depth_rendered, dev, torch.float64)
    de = _to(depth_est, dev, torch.float32)
    if tuple(dr64.shape) != (H, W) or tuple(de.shape) != (H, W):
        raise T2NError(f"prepare_depth_merge: depth_rendered {tuple(dr64.shape)} / depth_est {tuple(de.shape)} do not match the map {(H, W)}")
    dr32 = dr64.to(torch.float32)
    ps = _filled_pixels(lib, dev, known, max_samples, rng)
    f32 = lambda: torch.empty(H, W, device=dev, dtype=torch.float32)                       # noqa: E731
    depth_shift, depth_ref, depth_src, mask = f32(), f32(), f32(), f32()
    ss = torch.empty(4, device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        st = _lib.current_stream_ptr(dev)
        if ps.shape[0] >= 1:
            _lib.check(lib.t2n_depth_align_global(_lib.ptr(dr32), _lib.ptr(de), H, W, _lib.ptr(ps), int(ps.shape[0]), float(push_depth),
                                                  _lib.ptr(depth_shift), _lib.ptr(ss), st), "t2n_depth_align_global")
        else:
            _lib.check(lib.t2n_depth_align_fallback(_lib.ptr(dr32), _lib.ptr(de), H, W, float(push_depth), _lib.ptr(depth_shift),
                                                    _lib.ptr(ss), st), "t2n_depth_align_fallback")
        _lib.check(lib.t2n_depth_merge_inputs(_lib.ptr(dr64), _lib.ptr(known), _lib.ptr(depth_shift), H, W, float(push_depth),
                                              _lib.ptr(depth_ref), _lib.ptr(depth_src), _lib.ptr(mask), st), "t2n_depth_merge_inputs")
    s = ss.cpu().tolist()
    arrays = (ps, depth_shift, depth_ref, depth_src, mask)
    if to_host:
        arrays = tuple(t.cpu().numpy() for t in arrays)
    return DepthMerge(s[0], s[1], *arrays)


# ---- after inpainting: one RGB-D view -> support views -> training rays -------------------------------------------------------------
def _host(x):
    return np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)


def _is01(m):
    m = np.asarray(m)
    return m.dtype == np.bool_ or bool(np.isin(m, (0, 1)).all())


def _mask_u8(m, dev):
    """A 0/1 (or boolean) mask as device uint8."""
    if m is None:
        return None
    if isinstance(m, np.ndarray):
        m = np.ascontiguousarray(m != 0).view(np.uint8)
    return _to(m, dev, torch.uint8)


def _warp_mats(pose_gt, poses_tar, intrinsic):
    """The host matrices of gt_warping (utils.py:138-147) and Warper.compute_transformed_points (Warper.py:75,84), in numpy and the
    inputs' dtype like the reference: inv(K), the first three rows of inv(pose_tar[v]) @ inv(inv(pose_gt)) per target, K."""
    pose_gt, poses_tar = _host(pose_gt), _host(poses_tar)
    T1 = np.linalg.inv(pose_gt)
    K = np.eye(3).astype(np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = intrinsic[0], intrinsic[1], intrinsic[2], intrinsic[3]
    T = [np.matmul(np.linalg.inv(poses_tar[v]), np.linalg.inv(T1)) for v in range(poses_tar.shape[0])]
    T12 = np.stack([np.asarray(t, np.float64)[:3, :4] for t in T]).reshape(-1)
    d9 = lambda m: (C.c_double * 9)(*np.asarray(m, np.float64).reshape(-1)[:9])       # noqa: E731
    return d9(np.linalg.inv(K)), (C.c_double * T12.size)(*T12), d9(K), len(T)


def _warp_views(lib, dev, rgb, depth, m1, maux, H, W, mats, image, mask, depth64, depth32, aux):
    """t2n_warp_views on the current stream of `dev`; outputs are caller tensors (or None)."""
    Ki, T12, K, V = mats
    if rgb.shape != (H, W, 3) or depth.shape != (H, W):
        raise T2NError(f"gt_warping: rgb_gt {tuple(rgb.shape)} / depth_gt {tuple(depth.shape)} do not match (H, W) = {(H, W)}")
    for m in (m1, maux):
        if m is not None and m.shape != (H, W):
            raise T2NError(f"gt_warping: mask shape {tuple(m.shape)} does not match (H, W) = {(H, W)}")
    ws = torch.empty(int(lib.t2n_warp_views_workspace_bytes(H, W, V)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.t2n_warp_views(_lib.ptr(rgb), _lib.ptr(depth), _lib.ptr(m1), _lib.ptr(maux), H, W, V, Ki, T12, K, _lib.ptr(image),
                                      _lib.ptr(mask), _lib.ptr(depth64), _lib.ptr(depth32), _lib.ptr(aux), _lib.ptr(ws), ws.numel(),
                                      _lib.current_stream_ptr(dev)), "t2n_warp_views")


def _png8(a):
    """What imageio makes of a float array written as PNG (its lossy range conversion: min..max -> 0..255), so that the depth previews
    do not depend on which image writer is installed."""
    a = np.asarray(a, np.float64)
    lo, hi = float(np.nanmin(a)), float(np.nanmax(a))
    if hi == lo:
        return a.astype(np.uint8)
    if lo >= 0 and hi <= 1:
        return (a * 255.0 + 0.499999999).astype(np.uint8)
    return ((a - lo) / (hi - lo) * 255.0 + 0.499999999).astype(np.uint8)


def gt_warping(rgb_gt, depth_gt, pose_gt, poses_tar, H, W, intrinsic, logpath=None, mask_gt=None, warp_depth=False, bilinear_splat=False,
               device=None):
    """Same signature / return as utils.py:122 (plus ``device``): one source view forward-warped to every pose of ``poses_tar``
    [V,4,4] (camera-to-world, host arrays or tensors): ``(rgbs [V,H,W,3] float32 in [0,1], white where nothing landed, masks [V,H,W]
    int64[, depths [V,H,W] float64 when warp_depth])``. All V targets are one launch set over one upload of the source.
    ``bilinear_splat=False`` (the reference's default, its nearest-pixel raster loop) is not on the Text2NeRF path — every call site
    passes True — and is rejected. ``mask_gt`` must be boolean or 0/1-valued (the reference multiplies the weights by it): checked for
    numpy input, required of device input. ``rgb_gt`` is float32 in [0,1]. ``logpath``: the reference's previews,
    ``DIBR_gt/{warped,mask,mask_inv,warped_depth}/%05d.png`` numbered from 1."""
    if not bilinear_splat:
        raise T2NError("gt_warping: bilinear_splat=False (the nearest-pixel raster loop) is not on the Text2NeRF path and is not "
                       "implemented; every call site of the driver passes bilinear_splat=True")
    if mask_gt is not None and isinstance(mask_gt, np.ndarray) and not _is01(mask_gt):
        raise T2NError("gt_warping: mask_gt must be boolean or hold only 0 and 1 (it scales the splat weights)")
    lib = _lib.load()
    as_numpy = isinstance(rgb_gt, np.ndarray)
    dev = _dev(device if device is not None else (None if as_numpy else rgb_gt.device))
    mats = _warp_mats(pose_gt, poses_tar, intrinsic)
    V = mats[3]
    rgb, d, m1 = _to(rgb_gt, dev, torch.float32), _to(depth_gt, dev, torch.float32), _mask_u8(mask_gt, dev)
    image = torch.empty(V, H, W, 3, dtype=torch.float32, device=dev)
    mask = torch.empty(V, H, W, dtype=torch.int64, device=dev)
    depth = torch.empty(V, H, W, dtype=torch.float64, device=dev) if warp_depth else None
    if V > 0:
        _warp_views(lib, dev, rgb, d, m1, None, H, W, mats, image, mask, depth, None, None)
    if logpath is not None:
        from .renderer import _imwrite
        root = os.path.join(logpath, "DIBR_gt")
        for sub in ("warped", "mask", "mask_inv") + (("warped_depth",) if warp_depth else ()):
            os.makedirs(os.path.join(root, sub), exist_ok=True)
        img_h, mask_h = image.cpu().numpy(), mask.cpu().numpy()
        depth_h = depth.cpu().numpy() if warp_depth else None
        for vv in range(V):
            name = "%05d.png" % (vv + 1)
            if warp_depth:
                _imwrite(os.path.join(root, "warped_depth", name), _png8(depth_h[vv]))
            _imwrite(os.path.join(root, "warped", name), np.rint(img_h[vv] * 255.0).astype(np.uint8))
            _imwrite(os.path.join(root, "mask", name), (mask_h[vv] * 255).astype(np.uint8))
            _imwrite(os.path.join(root, "mask_inv", name), ((1 - mask_h[vv]) * 255).astype(np.uint8))
    out = (image, mask) + ((depth,) if warp_depth else ())
    return tuple(t.cpu().numpy() for t in out) if as_numpy else out


_MASK_DTYPES = {torch.uint8: _lib.MASK_U8, torch.bool: _lib.MASK_U8, torch.int32: _lib.MASK_I32, torch.int64: _lib.MASK_I64,
                torch.float32: _lib.MASK_F32, torch.float64: _lib.MASK_F64}


def _stack(x):
    if isinstance(x, (list, tuple)):
        return torch.stack(list(x)) if isinstance(x[0], torch.Tensor) else np.stack([np.asarray(a) for a in x])
    return x


def _c2w_rows(poses):
    p = np.ascontiguousarray(_host(poses), dtype=np.float32)
    if p.ndim != 3 or p.shape[1:] != (4, 4):
        raise T2NError(f"produce_formatted_data: poses must be [N,4,4] camera-to-world matrices, got {p.shape}")
    rows = np.ascontiguousarray(p[:, :3, :4]).reshape(-1)
    return p, (C.c_float * rows.size)(*rows.tolist())


def _format_views(lib, dev, images, depths, masks, c2w, N, H, W, intrinsic, want_rows):
    """t2n_format_views on the current stream of `dev`: (rays_split, all_rays, all_rgbs, all_depths, counts). The one host read is
    the record {K, rows per view}; the row tensors are the first K rows of N*H*W-row buffers."""
    fx, fy, cx, cy = [float(v) for v in intrinsic]
    n = H * W
    rays_split = torch.empty(N, n, 6, dtype=torch.float32, device=dev)
    rows = rgbs = deps = record = ws = None
    code = 0
    if want_rows:
        if masks.dtype not in _MASK_DTYPES:
            masks = masks.to(torch.float32)
        code = _MASK_DTYPES[masks.dtype]
        rows = torch.empty(N * n, 6, dtype=torch.float32, device=dev)
        rgbs = torch.empty(N * n, 3, dtype=torch.float32, device=dev)
        deps = torch.empty(N * n, dtype=torch.float32, device=dev)
        record = torch.empty(1 + N, dtype=torch.int64, device=dev)
        ws = torch.empty(int(lib.t2n_format_views_workspace_bytes(H, W, N)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.t2n_format_views(_lib.ptr(images), _lib.ptr(depths), _lib.ptr(masks), code, N, H, W, c2w, fx, fy, cx, cy,
                                        _lib.ptr(rays_split), _lib.ptr(rows), _lib.ptr(rgbs), _lib.ptr(deps), N * n, _lib.ptr(record),
                                        _lib.ptr(ws), 0 if ws is None else ws.numel(), _lib.current_stream_ptr(dev)),
                   "t2n_format_views")
    if not want_rows:
        return rays_split, None, None, None, None
    rec = record.cpu().tolist()                 # K is data dependent: the one read-back
    K = rec[0]
    return rays_split, rows[:K], rgbs[:K], deps[:K], rec[1:]


def produce_formatted_data(images, depths, masks, poses, intrinsic, H, W, mode='train', device=None):
    """Same signature / return as dataLoader/scene_gen.py:31 (plus ``device``). ``mode='train'``: ``(all_rays [K,6], all_rgbs [K,3],
    all_depths [K], all_rays_split [N,H*W,6], all_rgbs_split [N,H,W,3], all_depths_split [N,H,W], poses_tensor [N,4,4])``, all float32;
    the K rows are the pixels with ``mask > 0.5`` in the reference's order (view-major, raster order inside a view). ``mode='test'``:
    ``(all_rays_split, poses_tensor)``. numpy in -> CPU torch tensors (what the reference returns); device tensors in, or ``device=``
    given -> device tensors. RGBA images (the reference's alpha-blend branch) are not on this path and are rejected."""
    if mode not in ("train", "test"):
        raise T2NError(f"produce_formatted_data: mode must be 'train' or 'test', got {mode!r}")
    train = mode == "train"
    if train:
        images, depths, masks = _stack(images), _stack(depths), _stack(masks)
        if images.shape[-1] == 4:
            raise T2NError("produce_formatted_data: images with an alpha channel (RGBA) are not on the Text2NeRF path and are not "
                           "implemented; blend them to RGB first")
        if tuple(images.shape[1:]) != (H, W, 3) or tuple(depths.shape) != tuple(images.shape[:3]) or tuple(masks.shape) != tuple(depths.shape):
            raise T2NError(f"produce_formatted_data: images {tuple(images.shape)}, depths {tuple(depths.shape)}, masks "
                           f"{tuple(masks.shape)} must be [N,{H},{W},3], [N,{H},{W}], [N,{H},{W}]")
    lead = images if train else poses
    on_host = not isinstance(lead, torch.Tensor) or not lead.is_cuda
    p44, c2w = _c2w_rows(poses)
    N = p44.shape[0]
    if train and images.shape[0] != N:
        raise T2NError(f"produce_formatted_data: {images.shape[0]} images but {N} poses")
    lib = _lib.load()
    dev = _dev(device if device is not None else (None if on_host else lead.device))
    to_host = on_host and device is None
    img = dep = msk = None
    if train:
        img, dep = _to(images, dev, torch.float32), _to(depths, dev, torch.float32)
        if isinstance(masks, np.ndarray):
            masks = masks.view(np.uint8) if masks.dtype == np.bool_ else masks
            if masks.dtype not in (np.uint8, np.int32, np.int64, np.float32, np.float64):
                masks = masks.astype(np.float32)
            masks = torch.from_numpy(np.ascontiguousarray(masks))
        msk = masks.to(dev).contiguous()
    rays_split, rows, rgbs, deps, _ = _format_views(lib, dev, img, dep, msk, c2w, N, H, W, intrinsic, train)
    poses_tensor = torch.from_numpy(p44)
    out = (rows, rgbs, deps, rays_split, img, dep, poses_tensor) if train else (rays_split, poses_tensor)
    return tuple(t.cpu() if to_host else t.to(dev) for t in out)


def build_support_set(img_new, depth_new, mask_inpainted, poses_support, intrinsic, H, W, device=None):
    """The driver's support-set block (text2nerf_main.py:380-392) as one device-resident call: the new view ``img_new`` [H,W,3] /
    ``depth_new`` [H,W] (float32) is warped from ``poses_support[0]`` to ``poses_support[1:]`` ONCE — unmasked colour and depth, plus the
    coverage of the ``mask_inpainted`` pixels, which is the mask the driver's second, masked ``gt_warping`` call returns — the source
    view is put in front (its mask: ``mask_inpainted``) and the N = 1 + V views go through the formatter. Returns
    ``produce_formatted_data``'s 7-tuple as device tensors; ``all_depths_split[1:]`` is the warped depth rounded to float32.
    ``mask_inpainted=None`` is the initial-view form (scene_gen.py:305-316): the source keeps every pixel and each warp its own unmasked
    coverage. ``mask_inpainted`` must be boolean or 0/1-valued (checked for numpy input). ``poses_support`` should be a host array
    (it is inverted on the host); the only device read-back is the row-count record."""
    if mask_inpainted is not None and isinstance(mask_inpainted, np.ndarray) and not _is01(mask_inpainted):
        raise T2NError("build_support_set: mask_inpainted must be boolean or hold only 0 and 1")
    lib = _lib.load()
    as_numpy = isinstance(img_new, np.ndarray)
    dev = _dev(device if device is not None else (None if as_numpy else img_new.device))
    p44, c2w = _c2w_rows(poses_support)
    N = p44.shape[0]
    poses_h = _host(poses_support)
    rgb, d, maux = _to(img_new, dev, torch.float32), _to(depth_new, dev, torch.float32), _mask_u8(mask_inpainted, dev)
    images = torch.empty(N, H, W, 3, dtype=torch.float32, device=dev)
    depths = torch.empty(N, H, W, dtype=torch.float32, device=dev)
    masks = torch.empty(N, H, W, dtype=torch.int64, device=dev)
    images[0].copy_(rgb)
    depths[0].copy_(d)
    if maux is None:
        masks[0].fill_(1)
    else:
        masks[0].copy_(maux)
    if N > 1:
        mats = _warp_mats(poses_h[0], poses_h[1:], intrinsic)
        _warp_views(lib, dev, rgb, d, None, maux, H, W, mats, images[1:], masks[1:] if maux is None else None, None, depths[1:],
                    None if maux is None else masks[1:])
    rays_split, rows, rgbs, deps, _ = _format_views(lib, dev, images, depths, masks, c2w, N, H, W, intrinsic, True)
    return rows, rgbs, deps, rays_split, images, depths, torch.from_numpy(p44).to(dev)


# ---- after the merge network: the finished view, its support set, its rows in the training set ------------------------------------------
def _view_finish(lib, dev, depth_merged, img_u8, known, push_depth):
    """t2n_view_finish on the current stream of `dev`: (depth_new fp32 [H,W], img_new fp32 [H,W,3], mask_inpainted int64 [H,W]),
    before the filter."""
    H, W = known.shape
    depth_new = torch.empty(H, W, dtype=torch.float32, device=dev)
    img_new = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    mask_inpainted = torch.empty(H, W, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.t2n_view_finish(_lib.ptr(depth_merged), _lib.ptr(img_u8), _lib.ptr(known), H, W, float(push_depth),
                                       _lib.ptr(depth_new), _lib.ptr(img_new), _lib.ptr(mask_inpainted), _lib.current_stream_ptr(dev)),
                   "t2n_view_finish")
    return depth_new, img_new, mask_inpainted


class FinishedView(NamedTuple):
    """``finish_view``'s return, named after the driver's variables (text2nerf_main.py:278-299, :380-392). Device tensors.

    ==============  =========  =======  =============================================================================
    img_new         [H,W,3]    float32  the inpainted image ``/ 255.`` after the filter (:285, :291)
    depth_new       [H,W]      float32  the merged depth in scene units after the filter (:278, :282, :290)
    mask_inpainted  [H,W]      int64    ``current_mask_inpainted = 1 - myMap_filt`` (:296)
    support                             ``build_support_set``'s 7-tuple for the view (:380-392)
    lo, hi                     int      the row range the view's rays took in ``train_set`` (``None`` without a set)
    ==============  =========  =======  =============================================================================
    """
    img_new: Any
    depth_new: Any
    mask_inpainted: Any
    support: Any
    lo: Any
    hi: Any


def finish_view(depth_merged, img_u8, myMap_filt, push_depth, poses_support, intrinsic, H, W, train_set=None, device=None):
    """From "the merged depth is here" to "the rows are in the training set" (text2nerf_main.py:278-299 and :380-392) in one call:
    one elementwise launch for ``depth_new = ((depth_merged + 1.) * 32768.) / 12000 + push_depth`` (float32 operation by operation, as
    :278 and :282 on the network's float32 output), ``img_new = float32(img_u8 / 255.)`` (:285) and ``1 - myMap_filt`` (:296); the
    depth-aware filter with ``[5, 5, 3, 3]``, 0.02, 4 passes (:287-291); ``build_support_set`` on the filtered pair; and, when
    ``train_set`` (a ``DeviceTrainSet``) is given, ``train_set.append`` of the rows. Returns a ``FinishedView`` of device tensors.

    ``depth_merged``: the merge network's output, H*W float32 values in [-1,1] in any leading shape; ``img_u8`` [H,W,3] uint8, the
    chosen inpainted image; ``myMap_filt`` [H,W] the map the view was built with; ``poses_support`` [N,4,4] as ``build_support_set``
    takes them (host array; ``poses_support[0]`` is the view's own pose). Nothing between the stages is read on the host except
    ``build_support_set``'s row-count record. The PNG previews of :279-293 are not written. No CPU fallback."""
    lib = _lib.load()
    dev = _dev(device if device is not None else _first_device(depth_merged, img_u8, myMap_filt))
    known = _known32(myMap_filt, dev)
    if tuple(known.shape) != (H, W):
        raise T2NError(f"finish_view: myMap_filt {tuple(known.shape)} does not match (H, W) = {(H, W)}")
    dm = _to(depth_merged, dev, torch.float32)
    u8 = _to(img_u8, dev, torch.uint8)
    if dm.numel() != H * W or tuple(u8.shape) != (H, W, 3):
        raise T2NError(f"finish_view: depth_merged {tuple(dm.shape)} / img_u8 {tuple(u8.shape)} do not match (H, W) = {(H, W)}")
    depth0, img0, mask_inpainted = _view_finish(lib, dev, dm.reshape(H, W), u8, known, push_depth)
    photo, keep = _filter_views(lib, dev, depth0[None], img0[None], [5, 5, 3, 3], 0.02, 4)
    img_new, depth_new = photo[0], keep[0]
    with torch.cuda.device(dev):
        support = build_support_set(img_new, depth_new, mask_inpainted, poses_support, intrinsic, H, W, device=dev)
        lo = hi = None
        if train_set is not None:
            lo, hi = train_set.append(support[0], support[1], support[2])
    return FinishedView(img_new, depth_new, mask_inpainted, support, lo, hi)


# ---- before inpainting: known views -> the warped, filled and packed new view ------------------------------------------------------------
def _filter_schedule(filter_size, num_iter):
    sizes = [int(filter_size[i]) if isinstance(filter_size, (list, tuple)) else int(filter_size) for i in range(num_iter)]
    return (C.c_int * num_iter)(*sizes)


def _is_cuda(x):
    if isinstance(x, (list, tuple)):
        return any(_is_cuda(a) for a in x)
    return isinstance(x, torch.Tensor) and x.is_cuda


def _first_device(*xs):
    for x in xs:
        for a in (x if isinstance(x, (list, tuple)) else (x,)):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                return a.device
    return None


def _view_stack(x, dev, dtype, what, shape):
    """A list of frames or a stacked array as one contiguous device tensor of `shape`."""
    t = _to(_stack(x), dev, dtype)
    if tuple(t.shape) != tuple(shape):
        raise T2NError(f"{what}: shape {tuple(t.shape)} does not match {tuple(shape)}")
    return t


def _filter_views(lib, dev, d, im, filter_size, depth_threshold, num_iter):
    """t2n_sparse_bilateral_filtering_views on the current stream of `dev`: device stacks in, (photo, depth kept) out."""
    V, H, W = d.shape
    photo, keep = torch.empty_like(im), torch.empty_like(d)
    ws = torch.empty(int(lib.t2n_image_filter_views_workspace_bytes(H, W, V)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.t2n_sparse_bilateral_filtering_views(_lib.ptr(d), _lib.ptr(im), V, H, W, _filter_schedule(filter_size, num_iter),
                                                            num_iter, float(depth_threshold), _lib.ptr(photo), _lib.ptr(keep), _lib.ptr(ws),
                                                            ws.numel(), _lib.current_stream_ptr(dev)),
                   "t2n_sparse_bilateral_filtering_views")
    return photo, keep


def sparse_bilateral_filtering_views(depths, images, filter_size=[7, 7, 5, 5, 5], depth_threshold=0.04, num_iter=5, device=None):
    """``sparse_bilateral_filtering`` for a stack of views with one schedule, one launch set per pass for all of them: ``depths``
    [V,H,W], ``images`` [V,H,W,3] (stacked arrays or lists of frames) -> ``(photos [V,H,W,3], depths [V,H,W])``, per view what the
    driver keeps of the single-image call (text2nerf_main.py:118-119): ``vis_photos[-1]`` and ``vis_depths[-1]``, bit-equal to it."""
    lib = _lib.load()
    as_numpy = not _is_cuda(depths)
    dev = _dev(device if device is not None else _first_device(depths))
    d = _to(_stack(depths), dev, torch.float32)
    if d.dim() != 3:
        raise T2NError(f"sparse_bilateral_filtering_views: depths must be [V,H,W], got {tuple(d.shape)}")
    im = _view_stack(images, dev, torch.float32, "sparse_bilateral_filtering_views: images", tuple(d.shape) + (3,))
    photo, keep = _filter_views(lib, dev, d, im, filter_size, depth_threshold, num_iter)
    return (photo.cpu().numpy(), keep.cpu().numpy()) if as_numpy else (photo, keep)


def _source_mats(poses, pose_tar, intrinsic):
    """The host matrices of bilinear_splat_warping_multiview (utils.py:88-100) and Warper.compute_transformed_points (Warper.py:75,84),
    in numpy and the inputs' dtype like the reference: inv(K), the first three rows of inv(pose_tar) @ inv(inv(poses[v])) per source, K."""
    T2 = np.linalg.inv(_host(pose_tar))
    K = np.eye(3).astype(np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = intrinsic[0], intrinsic[1], intrinsic[2], intrinsic[3]
    T = [np.matmul(T2, np.linalg.inv(np.linalg.inv(_host(p)))) for p in poses]
    T12 = np.stack([np.asarray(t, np.float64)[:3, :4] for t in T]).reshape(-1)
    d9 = lambda m: (C.c_double * 9)(*np.asarray(m, np.float64).reshape(-1)[:9])       # noqa: E731
    return d9(np.linalg.inv(K)), (C.c_double * T12.size)(*T12), d9(K)


def _warp_sources(lib, dev, rgb, depth, m1, mats):
    """t2n_warp_sources on the current stream of `dev`: device stacks in, (mask int64, image fp32, depth fp64) out."""
    V, H, W = depth.shape
    Ki, T12, K = mats
    image = torch.empty(H, W, 3, dtype=torch.float32, device=dev)
    mask = torch.empty(H, W, dtype=torch.int64, device=dev)
    dep = torch.empty(H, W, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.t2n_warp_sources_workspace_bytes(H, W, V)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.t2n_warp_sources(_lib.ptr(rgb), _lib.ptr(depth), _lib.ptr(m1), H, W, V, Ki, T12, K, _lib.ptr(image), _lib.ptr(mask),
                                        _lib.ptr(dep), _lib.ptr(ws), ws.numel(), _lib.current_stream_ptr(dev)), "t2n_warp_sources")
    return mask, image, dep


def warp_sources(rgbs, depths, poses, pose_tar, H, W, intrinsic, masks=None, device=None):
    """``bilinear_splat_warping_multiview`` (utils.py:83, same arguments and return) with all sources in one launch set per chunk of 8
    instead of four launches per source: ``rgbs`` [V,H,W,3] / ``depths`` [V,H,W] (stacked or lists), ``poses[:V]`` their
    camera-to-world matrices, ``masks`` [V,H,W] boolean or 0/1 -> ``(mask_final [H,W] int64, output_image [H,W,3] fp32, output_depth
    [H,W] fp64)``; earlier sources win."""
    lib = _lib.load()
    as_numpy = not _is_cuda(rgbs)
    dev = _dev(device if device is not None else _first_device(rgbs))
    V = len(rgbs)
    if V < 1:
        raise T2NError("warp_sources: needs at least one source view")
    rgb = _view_stack(rgbs, dev, torch.float32, "warp_sources: rgbs", (V, H, W, 3))
    d = _view_stack(depths, dev, torch.float32, "warp_sources: depths", (V, H, W))
    m1 = None
    if masks is not None:
        m1 = _stack(masks)
        m1 = _view_stack(_mask_u8(m1, dev) if isinstance(m1, np.ndarray) else (m1 != 0), dev, torch.uint8, "warp_sources: masks", (V, H, W))
    out = _warp_sources(lib, dev, rgb, d, m1, _source_mats([poses[v] for v in range(V)], pose_tar, intrinsic))
    return tuple(t.cpu().numpy() for t in out) if as_numpy else out


def _pack(lib, dev, warp, known32, rgb, depth):
    """t2n_inpaint_pack on the current stream of `dev`; returns the eight arrays in the C call's order."""
    H, W = known32.shape
    u8 = lambda *sh: torch.empty(*sh, dtype=torch.uint8, device=dev)                    # noqa: E731
    out = (u8(H, W, 3), torch.empty(H, W, dtype=torch.int64, device=dev), u8(H, W), u8(H, W),
           torch.empty(H, W, 3, dtype=torch.int64, device=dev), u8(H, W, 3), u8(H, W, 3), torch.empty(H, W, dtype=torch.float64, device=dev))
    with torch.cuda.device(dev):
        _lib.check(lib.t2n_inpaint_pack(_lib.ptr(warp), _lib.ptr(known32), _lib.ptr(rgb), _lib.ptr(depth), H, W, *[_lib.ptr(t) for t in out],
                                        _lib.current_stream_ptr(dev)), "t2n_inpaint_pack")
    return out


def _expand_mask(lib, dev, known32):
    """t2n_mask_expand on the current stream of `dev`: (eroded map int32 [H,W], the removed ring int64 [H,W,3])."""
    H, W = known32.shape
    eroded = torch.empty_like(known32)
    ring = torch.empty(H, W, 3, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.t2n_mask_expand(_lib.ptr(known32), H, W, _lib.ptr(eroded), _lib.ptr(ring), _lib.current_stream_ptr(dev)),
                   "t2n_mask_expand")
    return eroded, ring


def pack_inpaint_inputs(output_image_warp, myMap_filt, rgb_render, depth_render, device=None, update_known_views=False):
    """The arrays the driver builds around the inpainter (text2nerf_main.py:138-184) in one launch, from
    the filled warp [H,W,3] fp32, its 0/1 map [H,W], and the target render ``rgb_render`` [H,W,3] (clamped here) / ``depth_render``
    [H,W] fp32. Returns ``(output_image_warp u8 [H,W,3], myMap_filt int64 [H,W], mask_image u8, mask_inv u8, mask_ex int64 [H,W,3],
    rgb_render u8 [H,W,3], rgb_render_ u8 [H,W,3], depth_rendered fp64 [H,W])``. ``update_known_views=True`` is the mask expansion of
    :147-152, one stencil launch in front: the map is eroded (a pixel stays 1 only when its whole 5x5 window, reflected at the border
    as OpenCV's default ``BORDER_REFLECT_101`` does, is 1), the eroded map takes ``myMap_filt``'s place in every output, and
    ``mask_ex`` is the removed ring (the map minus the eroded map) on three channels."""
    lib = _lib.load()
    as_numpy = not _is_cuda(output_image_warp)
    dev = _dev(device if device is not None else _first_device(output_image_warp))
    known = _to(myMap_filt, dev, torch.int32)
    if known.dim() != 2:
        raise T2NError(f"pack_inpaint_inputs: myMap_filt must be [H,W], got {tuple(known.shape)}")
    H, W = known.shape
    warp = _view_stack(output_image_warp, dev, torch.float32, "pack_inpaint_inputs: output_image_warp", (H, W, 3))
    rgb = _to(rgb_render, dev, torch.float32).reshape(-1)
    dep = _to(depth_render, dev, torch.float32).reshape(-1)
    if rgb.numel() != H * W * 3 or dep.numel() != H * W:
        raise T2NError(f"pack_inpaint_inputs: the render does not match (H, W) = {(H, W)}")
    ring = None
    if update_known_views:
        known, ring = _expand_mask(lib, dev, known)
    out = _pack(lib, dev, warp, known, rgb, dep)
    if ring is not None:
        out = out[:4] + (ring,) + out[5:]
    return tuple(t.cpu().numpy() for t in out) if as_numpy else out


class InpaintView(NamedTuple):
    """What ``render_warping_inapinting`` holds when it reaches the inpainter, named after its variables (text2nerf_main.py:99-184).
    numpy arrays or device tensors, as ``build_inpaint_view`` was called.

    ======================  ===========  =======  ===========================================================================
    rgbs_pre                [V,H,W,3]    float32  the frames that were warped: the filtered renders of the known views (:119),
    depths_pre              [V,H,W]      float32  or ``known_rgbs`` / ``known_depths`` as given
    warp_image              [H,W,3]      float32  the merged warp before hole filling, in [0,1], white where nothing landed
    myMap                   [H,W]        int64    1 where a known view landed (:129)
    warp_depth              [H,W]        float64  its depth, 0 where nothing landed
    output_image_warp       [H,W,3]      float32  the warp after ``dibr_filter_mask2`` (:134; = warp_image without the fill stage)
    myMap_filt              [H,W]        int64    its map (= myMap without the fill stage); with ``update_known_views=True`` that map
                                                  eroded (:148-152), which every row below then uses
    output_depth            [H,W]        float64  its depth
    output_image_warp_u8    [H,W,3]      uint8    what the driver rebinds ``output_image_warp`` to: ``* 255`` truncated, zero outside
                                                  the mask (:138,156-157)
    mask_image, mask_inv    [H,W]        uint8    ``myMap_filt * 255``, ``(1 - myMap_filt) * 255`` (:158-159)
    mask_ex                 [H,W,3]      int64    ``myMap_filt`` on three channels (:154); with ``update_known_views=True`` the ring the
                                                  erosion removed (:150-151)
    rgb_render              [H,W,3]      uint8    the new pose rendered, clamped, truncated (:169-170)
    rgb_render_             [H,W,3]      uint8    ``rgb_render`` inside the mask, white outside (:174-177)
    depth_rendered          [H,W]        float64  the rendered depth times the mask (:171)
    output_image            [H,W,3]      uint8    the inpainter's init image: the same array as ``rgb_render`` (:184)
    ======================  ===========  =======  ===========================================================================
    """
    myMap: Any
    myMap_filt: Any
    output_image_warp: Any
    output_depth: Any
    mask_image: Any
    mask_inv: Any
    mask_ex: Any
    rgb_render: Any
    rgb_render_: Any
    depth_rendered: Any
    output_image: Any
    rgbs_pre: Any
    depths_pre: Any
    warp_image: Any
    warp_depth: Any
    output_image_warp_u8: Any


def _render_frames(tensorf, poses, rays, intrinsic, H, W, N_samples, white_bg, ndc_ray):
    """rgb [V,H,W,3] clamped to [0,1] and depth [V,H,W] of whole frames: from `rays` [V,H*W,6] as the driver's renderer call does
    (text2nerf_main.py:110-112), else from rays generated on the device per pose (``render_views``)."""
    from .renderer import OctreeRender_trilinear_fast, _no_materialised_weights, render_views
    if rays is None:
        if ndc_ray:
            raise T2NError("build_inpaint_view: ndc_ray=True needs the caller's NDC rays (rays=)")
        return render_views(tensorf, poses, intrinsic, H, W, N_samples=N_samples, white_bg=white_bg)
    rgbs, depths = [], []
    with torch.no_grad(), _no_materialised_weights(tensorf):
        for v in range(rays.shape[0]):
            rgb, _, depth, _, _ = OctreeRender_trilinear_fast(rays[v], tensorf, N_samples=N_samples, ndc_ray=ndc_ray, white_bg=white_bg,
                                                              is_train=False, device=rays.device)
            rgbs.append(rgb.clamp(0.0, 1.0).reshape(H, W, 3))
            depths.append(depth.reshape(H, W))
    return torch.stack(rgbs), torch.stack(depths)


def build_inpaint_view(tensorf, poses, N_iter, H, W, intrinsic, N_samples=-1, white_bg=False, ndc_ray=False, rays=None, known_rgbs=None,
                       known_depths=None, use_filter_filling=True, device=None, update_known_views=False):
    """The half of ``render_warping_inapinting`` that runs before the inpainter (text2nerf_main.py:99-184) as one device-resident
    call; returns an ``InpaintView``. ``update_known_views=False`` is the branch the driver selects; ``True`` adds the mask expansion
    of :147-152 (see ``pack_inpaint_inputs``) between the fill stage and the pack.

    ``poses`` [>= N_iter + 1, 4, 4] camera-to-world (host array or tensor; inverted on the host): ``poses[:N_iter]`` are the known
    views, ``poses[N_iter]`` the new one. Stages, queued in order with nothing read back in between (the known views render on
    ``render_views``' two alternating streams, which hand over to the current stream; everything else is on the current stream):
    render the known views; filter the stack (``[7,5,5,3,3]``, 0.02, 5 passes, :115-117); warp all of them into the new pose, earlier views win
    (``warp_sources``); ``dibr_filter_mask2`` unless ``use_filter_filling=False``; render the new pose; pack.

    Rays are generated on the device from ``(pose, intrinsic)`` as ``render_views`` does; ``rays`` [N_iter + 1, H*W, 6] (the driver's
    ``all_rays_gen_split``) are used instead when given, and are required with ``ndc_ray``. ``known_rgbs`` [N_iter,H,W,3] /
    ``known_depths`` [N_iter,H,W] is the ``use_rendered_img_to_warp=False`` form: these frames are warped, and the known views are
    neither rendered nor filtered. numpy / CPU inputs -> numpy out; a device tensor among ``poses`` / ``rays`` / ``known_*`` (or
    ``device=``) -> device tensors out. Not here: the PNG writes. No CPU fallback."""
    V = int(N_iter)
    if V < 1:
        raise T2NError(f"build_inpaint_view: N_iter must be >= 1 (the known views to warp), got {N_iter}")
    if (known_rgbs is None) != (known_depths is None):
        raise T2NError("build_inpaint_view: known_rgbs and known_depths go together")
    if len(poses) < V + 1:
        raise T2NError(f"build_inpaint_view: {len(poses)} poses for N_iter = {V}: poses[N_iter] is the new view")
    inputs = (poses, rays, known_rgbs, known_depths)
    to_host = device is None and not any(_is_cuda(x) for x in inputs if x is not None)
    dev = _dev(device if device is not None else (_first_device(*[x for x in inputs if x is not None]) or
                                                  getattr(getattr(getattr(tensorf, "basis_mat", None), "weight", None), "device", None)))
    lib = _lib.load()
    poses_h = np.stack([_host(poses[v]) for v in range(V + 1)])
    if poses_h.shape[1:] != (4, 4):
        raise T2NError(f"build_inpaint_view: poses must be [N,4,4] camera-to-world matrices, got {poses_h.shape}")
    if rays is not None:
        rays = _to(rays if not isinstance(rays, (list, tuple)) else _stack(rays), dev, torch.float32)
        if rays.dim() != 3 or rays.shape[0] < V + 1 or tuple(rays.shape[1:]) != (H * W, 6):
            raise T2NError(f"build_inpaint_view: rays {tuple(rays.shape)} must be [>= {V + 1}, {H * W}, 6]")
    with torch.cuda.device(dev):
        if known_rgbs is not None:
            rgbs_pre = _view_stack(known_rgbs, dev, torch.float32, "build_inpaint_view: known_rgbs", (V, H, W, 3))
            depths_pre = _view_stack(known_depths, dev, torch.float32, "build_inpaint_view: known_depths", (V, H, W))
        else:
            rgb_k, depth_k = _render_frames(tensorf, poses_h[:V], None if rays is None else rays[:V], intrinsic, H, W, N_samples, white_bg,
                                            ndc_ray)
            rgbs_pre, depths_pre = _filter_views(lib, dev, depth_k.contiguous(), rgb_k.contiguous(), [7, 5, 5, 3, 3], 0.02, 5)
        myMap, warp_image, warp_depth = _warp_sources(lib, dev, rgbs_pre, depths_pre, None, _source_mats(poses_h[:V], poses_h[V], intrinsic))
        known = myMap.to(torch.int32)
        filled_image, output_depth = warp_image, warp_depth
        if use_filter_filling:
            filled_image, output_depth = warp_image.clone(), warp_depth.clone()
            _lib.check(lib.t2n_dibr_filter_mask2(_lib.ptr(filled_image), _lib.ptr(known), _lib.ptr(output_depth), H, W, 0.65,
                                                 _lib.current_stream_ptr(dev)), "t2n_dibr_filter_mask2")
        rgb_t, depth_t = _render_frames(tensorf, poses_h[V:V + 1], None if rays is None else rays[V:V + 1], intrinsic, H, W, N_samples,
                                        white_bg, ndc_ray)
        ring = None
        if update_known_views:
            known, ring = _expand_mask(lib, dev, known)
        warp_u8, myMap_filt, mask_image, mask_inv, mask_ex, rgb_u8, rgb_masked, depth_rendered = _pack(
            lib, dev, filled_image, known, rgb_t.contiguous(), depth_t.contiguous())
        if ring is not None:
            mask_ex = ring
    out = InpaintView(myMap=myMap, myMap_filt=myMap_filt, output_image_warp=filled_image, output_depth=output_depth, mask_image=mask_image,
                      mask_inv=mask_inv, mask_ex=mask_ex, rgb_render=rgb_u8, rgb_render_=rgb_masked, depth_rendered=depth_rendered,
                      output_image=rgb_u8, rgbs_pre=rgbs_pre, depths_pre=depths_pre, warp_image=warp_image, warp_depth=warp_depth,
                      output_image_warp_u8=warp_u8)
    if not to_host:
        return out
    host = {id(t): t.cpu().numpy() for t in set(out)}          # aliases (output_image is rgb_render) stay aliases
    return InpaintView(*[host[id(t)] for t in out])
