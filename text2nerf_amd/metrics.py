"""Image metrics of the evaluation loops on the device: SSIM (`rgb_ssim`, utils.py:436-482) and, from the same loads, the squared
error of the PSNR (renderer.py:98). One tile kernel plus one short reduction per STACK of views (csrc/t2n_metrics.hip,
`t2n_ssim_views`) instead of 30 `scipy.signal.convolve2d` calls per view on the host after two device-to-host frame copies.

    rgb_ssim      the reference's function, signature and defaults (tests/golden/metrics_signatures.json): one image pair
    ssim_views    [V,H,W,3] stacks -> device float64 [V], no host synchronisation
    score_views   {"psnr": [V], "ssim": [V]} of a rendered stack against its ground truth, one call, nothing leaves the device

To have `evaluation` report SSIM: `text2nerf_amd.renderer.rgb_ssim = text2nerf_amd.metrics.rgb_ssim`.

Exactness: float32 inputs take the float32 instantiation (products a*a, b*b, a*b rounded to float32 like `img0**2` on a float32
tensor), float64 inputs the float64 one; every window sum and all later arithmetic is float64, as scipy's is. Against the reference
the map differs by summation order only (~1e-13 at max_val 1). Limits: 1 <= filter_size <= 33. No CPU fallback."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

_TILE = 16          # output pixels per tile edge of k_ssim_tiles (csrc/t2n_metrics.hip: kSsimT)
_MAX_FILTER = 33    # kSsimMaxF
_ERR_INVALID = -1   # T2N_ERR_INVALID


def gaussian_taps(filter_size, filter_sigma):
    """The reference's 1-D blur filter, by its own numpy expression (utils.py:448-452): the weights are its to the last bit."""
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    f_i = ((np.arange(filter_size) - hw + shift) / filter_sigma)**2
    filt = np.exp(-0.5 * f_i)
    filt /= np.sum(filt)
    return filt


def _ssim_call(img0, img1, filt, c1, c2, clamp, ssim, ssim_map=None, sq_err=None, workspace=None):
    """t2n_ssim_views on contiguous device stacks [V,H,W,3] of one dtype (float32 / float64). T2N_ERR_INVALID -> ValueError."""
    lib = _lib.load()
    dev = img0.device
    V, H, W, _ = img0.shape
    fs = len(filt)
    taps = (C.c_double * max(fs, 1))(*[float(t) for t in filt])
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = torch.empty(max(int(lib.t2n_ssim_views_workspace_bytes(V, H, W, fs)), 1), dtype=torch.uint8, device=dev)
        rc = lib.t2n_ssim_views(_lib.ptr(img0), _lib.ptr(img1), 0 if img0.dtype == torch.float32 else 1, V, H, W, taps, fs, float(c1),
                                float(c2), 1 if clamp else 0, _lib.ptr(ssim), _lib.ptr(ssim_map), _lib.ptr(sq_err), _lib.ptr(workspace),
                                workspace.numel(), _lib.current_stream_ptr(dev))
    if rc == _ERR_INVALID:
        msg = lib.t2n_last_error()
        raise ValueError(msg.decode() if msg else "t2n_ssim_views: bad argument")
    _lib.check(rc, "t2n_ssim_views")


def _device_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    if not torch.cuda.is_available():
        raise _lib.T2NError("SSIM runs on the MI355X only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _stack_dtype(*xs):
    """float32 only when every input is float32; float64 inputs keep float64; anything else is converted to float64."""
    kinds = {str(x.dtype).replace("torch.", "") for x in xs}
    return torch.float32 if kinds == {"float32"} else torch.float64


def _to_stack(x, dev, dtype):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(device=dev, dtype=dtype).contiguous()


def _check_filter(filter_size, H, W):
    if int(filter_size) != filter_size or not 1 <= filter_size <= _MAX_FILTER:
        raise ValueError(f"filter_size {filter_size} outside 1..{_MAX_FILTER}")
    if H < filter_size or W < filter_size:
        raise ValueError(f"a {H}x{W} image is smaller than the {filter_size}-tap filter (no 'valid' window)")


@torch.no_grad()
def ssim_views(imgs0, imgs1, max_val=1.0, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False, clamp=False):
    """`rgb_ssim` of every pair of two stacks [V,H,W,3] (numpy, CPU or device tensors): a device float64 [V] tensor, and with
    `return_map` also the maps [V,H-fs+1,W-fs+1,3]. `clamp`: imgs0 is clamped to [0,1] as it is read (renderer.py:92). Nothing
    synchronises with the host."""
    s0, s1 = tuple(imgs0.shape), tuple(imgs1.shape)
    if len(s0) != 4 or s0[-1] != 3 or s0 != s1 or s0[0] < 1:
        raise ValueError(f"ssim_views: stacks of shape {s0} and {s1}, need two equal [V,H,W,3]")
    V, H, W, _ = s0
    _check_filter(filter_size, H, W)
    dev = _device_of(imgs0, imgs1)
    dtype = _stack_dtype(imgs0, imgs1)
    a, b = _to_stack(imgs0, dev, dtype), _to_stack(imgs1, dev, dtype)
    filt = gaussian_taps(filter_size, filter_sigma)
    ssim = torch.empty(V, dtype=torch.float64, device=dev)
    maps = torch.empty(V, H - filter_size + 1, W - filter_size + 1, 3, dtype=torch.float64, device=dev) if return_map else None
    _ssim_call(a, b, filt, (k1 * max_val)**2, (k2 * max_val)**2, clamp, ssim, maps)
    return (ssim, maps) if return_map else ssim


@torch.no_grad()
def rgb_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """The reference's `rgb_ssim` (utils.py:436-482) on the device. img0, img1 [H,W,3]: numpy arrays, CPU or device tensors. Returns
    a Python float (the one host read), or with `return_map` the map [H-fs+1,W-fs+1,3] in float64: a numpy array for host inputs, a
    device tensor for device inputs. ValueError where the reference's asserts fail or scipy would raise."""
    s0, s1 = tuple(img0.shape), tuple(img1.shape)
    if len(s0) != 3 or s0[-1] != 3 or s0 != s1:
        raise ValueError(f"rgb_ssim: images of shape {s0} and {s1}, need two equal [H,W,3]")
    on_device = any(isinstance(x, torch.Tensor) and x.is_cuda for x in (img0, img1))
    out = ssim_views(img0[None], img1[None], max_val, filter_size, filter_sigma, k1, k2, return_map=return_map)
    if return_map:
        return out[1][0] if on_device else out[1][0].cpu().numpy()
    return float(out.item())


@torch.no_grad()
def score_views(rgbs, gt_rgbs, max_val=1.0, clamp=True):
    """PSNR and SSIM (reference defaults: 11 taps, sigma 1.5) of a rendered stack [V,H,W,3] — the output of `render_views` or
    `evaluation_frames`' renders — against its ground truth, from ONE kernel pass over the two stacks: {"psnr": [V], "ssim": [V]} as
    device float64 tensors, PSNR = -10 log10(sum((rgb - gt)^2) / (3 H W)) (renderer.py:98). `clamp`: the render is clamped to [0,1] as
    it is read (renderer.py:92). Nothing synchronises with the host."""
    s0, s1 = tuple(rgbs.shape), tuple(gt_rgbs.shape)
    if len(s0) != 4 or s0[-1] != 3 or s0 != s1 or s0[0] < 1:
        raise ValueError(f"score_views: stacks of shape {s0} and {s1}, need two equal [V,H,W,3]")
    V, H, W, _ = s0
    _check_filter(11, H, W)
    dev = _device_of(rgbs, gt_rgbs)
    dtype = _stack_dtype(rgbs, gt_rgbs)
    a, b = _to_stack(rgbs, dev, dtype), _to_stack(gt_rgbs, dev, dtype)
    ssim = torch.empty(V, dtype=torch.float64, device=dev)
    sq = torch.empty(V, dtype=torch.float64, device=dev)
    _ssim_call(a, b, gaussian_taps(11, 1.5), (0.01 * max_val)**2, (0.03 * max_val)**2, clamp, ssim, None, sq)
    psnr = -10.0 * torch.log10(sq / (3 * H * W))
    return {"psnr": psnr, "ssim": ssim}
