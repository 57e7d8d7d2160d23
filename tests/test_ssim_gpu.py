"""The device SSIM (csrc/t2n_metrics.hip through `t2n_ssim_views`, text2nerf_amd/metrics.py) on the MI355X, against the reference's own
`rgb_ssim` outputs (tests/golden/ssim.npz) and, at shapes the fixture does not hold, the numpy restatement pinned to it
(tests/helpers/ssim_ref.py, tests/test_ssim_cpu.py).

Tolerance 1e-11 absolute on the map and the mean, from the arithmetic: a window is at most 33^2 terms of magnitude <= max_val^2 summed in
float64, so each moment carries an error of a few 1e-16 relative to max_val^2; the cancelling E[x^2] - mu^2 is divided by at least
c2 = 9e-4 max_val^2, an amplification of ~1.1e3, which gives ~1e-12: 10x margin, and four orders below the ~1e-7 by which a kernel that forms
the products a*a, b*b, a*b in the wrong dtype moves the map (tests/test_ssim_cpu.py asserts that gap on this fixture)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN, TINY
from tests.helpers import ssim_ref as R
from tests.test_hip_parity import dev, make_field
from text2nerf_amd import _lib, metrics, synth

sys.path.insert(0, GOLDEN)
from make_golden_ssim_cases import cases, inputs  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-11
T = metrics._TILE
EDGES = [1, T - 1, T, T + 1, 2 * T + 1]         # output heights / widths: one pixel, either side of a tile, three tiles with a 1-pixel tail
FS = 11


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "ssim.npz"), allow_pickle=False))


def _stack(V, H, W, seed, dtype, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    a = rng.uniform(lo, hi, (V, H, W, 3))
    b = np.clip(a + 0.1 * rng.standard_normal((V, H, W, 3)), lo, hi)
    return a.astype(dtype), b.astype(dtype)


def _raw(a, b, fs=FS, sigma=1.5, clamp=False, want_map=True, want_sq=True):
    """One t2n_ssim_views call on device stacks: (ssim [V], map or None, sq_err or None)."""
    V, H, W, _ = a.shape
    ssim = torch.empty(V, dtype=torch.float64, device=a.device)
    mp = torch.empty(V, H - fs + 1, W - fs + 1, 3, dtype=torch.float64, device=a.device) if want_map else None
    sq = torch.empty(V, dtype=torch.float64, device=a.device) if want_sq else None
    metrics._ssim_call(a, b, metrics.gaussian_taps(fs, sigma), 1e-4, 9e-4, clamp, ssim, mp, sq)
    return ssim, mp, sq


def test_every_golden_case_map_and_mean(gold):
    """float32 cases enter as float32 torch tensors (the `evaluation` call), float64 cases as numpy arrays (the offline scorer)."""
    worst = 0.0
    for case in cases():
        name, kind, H, W, dt, mv, fs, sigma, seed = case
        a, b = inputs(case)
        if dt == "float32":
            a, b = torch.from_numpy(a), torch.from_numpy(b)
        m = metrics.rgb_ssim(a, b, mv, filter_size=fs, filter_sigma=sigma, return_map=True)
        s = metrics.rgb_ssim(a, b, mv, filter_size=fs, filter_sigma=sigma)
        assert isinstance(m, np.ndarray) and m.dtype == np.float64 and m.shape == (H - fs + 1, W - fs + 1, 3), name
        assert isinstance(s, float)
        e_map, e_mean = float(np.abs(m - gold[name + "/map"]).max()), abs(s - float(gold[name + "/ssim"]))
        print(f"{name:34s} |map - golden| {e_map:.2e} |ssim - golden| {e_mean:.2e}")
        worst = max(worst, e_map, e_mean)
        assert e_map <= TOL and e_mean <= TOL, (name, e_map, e_mean)
    print("worst", worst)
    for dt in (torch.float32, torch.float64):          # identical flat images: exactly 1.0, and a device tensor in gives a device map out
        flat = torch.full((12, 29, 3), 0.5, dtype=dt, device=dev())
        assert metrics.rgb_ssim(flat, flat, 1) == 1.0
        m = metrics.rgb_ssim(flat, flat, 1, return_map=True)
        assert isinstance(m, torch.Tensor) and m.is_cuda and m.dtype == torch.float64 and bool((m == 1.0).all())


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_tile_edges_view_stride_and_single_view_bit_equality(dtype):
    """Output heights and widths independently over {1, T-1, T, T+1, 2T+1}; three different images per stack; every view of the stack
    against the helper and bit-equal to the same view scored alone."""
    worst = 0.0
    for i, oh in enumerate(EDGES):
        for j, ow in enumerate(EDGES):
            H, W = oh + FS - 1, ow + FS - 1
            a, b = _stack(3, H, W, 1000 + 10 * i + j, dtype)
            ta, tb = torch.from_numpy(a).to(dev()), torch.from_numpy(b).to(dev())
            ssim, maps = metrics.ssim_views(ta, tb, return_map=True)
            assert maps.shape == (3, oh, ow, 3) and ssim.shape == (3,) and ssim.dtype == maps.dtype == torch.float64 and ssim.is_cuda
            for v in range(3):
                want = R.ssim_map(a[v], b[v], 1.0)
                e = max(float(np.abs(maps[v].cpu().numpy() - want).max()), abs(float(ssim[v]) - float(want.mean())))
                worst = max(worst, e)
                assert e <= TOL, (oh, ow, v, e)
                s1, m1 = metrics.ssim_views(ta[v:v + 1], tb[v:v + 1], return_map=True)
                assert torch.equal(s1[0], ssim[v]) and torch.equal(m1[0], maps[v]), (oh, ow, v)
    print("worst |device - helper| over the tile-edge shapes", worst)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_repeatable_and_sq_err_owns_every_pixel_once(dtype):
    """2T+1 outputs by T+1 (and transposed): 3 x 2 tiles whose last row and column own the input border. Two runs are bit-equal in ssim,
    sq_err and the map; sq_err equals the float64 sum of the input-dtype squared differences at rtol 1e-12 (a different summation order
    of <= 5e3 non-negative float64 terms: ~1e-15 relative)."""
    for oh, ow in ((2 * T + 1, T + 1), (T + 1, 2 * T + 1), (2 * T + 1, 2 * T + 1)):
        a, b = _stack(3, oh + FS - 1, ow + FS - 1, 77 + oh, dtype)
        ta, tb = torch.from_numpy(a).to(dev()), torch.from_numpy(b).to(dev())
        s0, m0, q0 = _raw(ta, tb)
        s1, m1, q1 = _raw(ta, tb)
        assert torch.equal(s0, s1) and torch.equal(m0, m1) and torch.equal(q0, q1)
        for v in range(3):
            want = R.sq_err(a[v], b[v])
            got = float(q0[v])
            print(oh, ow, v, "sq_err", got, "numpy", want)
            assert abs(got - want) <= 1e-12 * want, (oh, ow, v, got, want)
        s2, _, _ = _raw(ta, tb, want_map=False, want_sq=False)       # the optional outputs change nothing
        assert torch.equal(s0, s2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
def test_clamp_equals_clamping_first(dtype):
    a, b = _stack(2, 2 * T + 7, T + 13, 5, np.float64, lo=-0.5, hi=1.5)
    ta, tb = torch.from_numpy(a).to(dev(), dtype), torch.from_numpy(b).to(dev(), dtype).clamp(0, 1)
    assert bool((ta < 0).any()) and bool((ta > 1).any())
    s0, m0, q0 = _raw(ta, tb, clamp=True)
    s1, m1, q1 = _raw(ta.clamp(0.0, 1.0), tb)
    assert torch.equal(s0, s1) and torch.equal(m0, m1) and torch.equal(q0, q1)
    s2, _, _ = _raw(ta, tb)
    assert not torch.equal(s0, s2)
    assert torch.equal(metrics.ssim_views(ta, tb, clamp=True), s0)


def test_score_views_on_rendered_views(tiny_params):
    """PSNR against `postprocess_frame`'s (two summation orders over the same float32 squares: 1e-6 relative) and SSIM equal to
    `ssim_views` on the same stacks. That nothing in the call synchronises with the host is NOT checked here: the suite has no helper
    that could observe it (the call's only host-side work is ctypes and torch allocations on the current stream)."""
    from text2nerf_amd import postprocess_frame, render_views
    f = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    H, W = 40, 52
    poses = [synth.look_pose(0.2 * v - 0.2, -0.1, (0.2, 0.1, -1.0)) for v in range(3)]
    rgbs, depths = render_views(f, poses, [float(W), float(W), W // 2, H // 2], H, W)
    g = torch.Generator().manual_seed(9)
    gt = (rgbs + 0.05 * torch.randn(rgbs.shape, generator=g).to(rgbs.device)).clamp(0.0, 1.0)
    out = metrics.score_views(rgbs, gt)
    assert set(out) == {"psnr", "ssim"}
    for k in out:
        assert out[k].shape == (3,) and out[k].dtype == torch.float64 and out[k].is_cuda
    assert torch.equal(out["ssim"], metrics.ssim_views(rgbs, gt, clamp=True))
    for v in range(3):
        _, _, want = postprocess_frame(rgbs[v], depths[v], TINY["near_far"], push_depth=2.0, gt_rgb=gt[v])
        got = float(out["psnr"][v])
        print(v, "psnr", got, "postprocess_frame", want, "ssim", float(out["ssim"][v]))
        assert abs(got - want) <= 1e-6 * abs(want), (v, got, want)
        assert 0.0 < float(out["ssim"][v]) < 1.0


def test_invalid_arguments_launch_nothing():
    lib = _lib.load()
    SENT = -123.0
    a, b = _stack(1, 20, 24, 3, np.float32)
    ta, tb = torch.from_numpy(a).to(dev()), torch.from_numpy(b).to(dev())
    ssim = torch.full((1,), SENT, dtype=torch.float64, device=dev())
    mp = torch.full((1, 20, 24, 3), SENT, dtype=torch.float64, device=dev())
    sq = torch.full((1,), SENT, dtype=torch.float64, device=dev())
    ws = torch.zeros(4096, dtype=torch.uint8, device=dev())
    taps = (C.c_double * 40)(*([1.0 / 40] * 40))
    need = int(lib.t2n_ssim_views_workspace_bytes(1, 20, 24, 11))
    assert 0 < need <= ws.numel()
    assert lib.t2n_ssim_views_workspace_bytes(1, 10, 24, 11) == 0 and lib.t2n_ssim_views_workspace_bytes(0, 20, 24, 11) == 0
    assert lib.t2n_ssim_views_workspace_bytes(1, 40, 40, 34) == 0 and lib.t2n_ssim_views_workspace_bytes(1, 40, 40, 0) == 0
    st = _lib.current_stream_ptr(dev())

    def call(V=1, H=20, W=24, fs=11, ws_bytes=ws.numel(), img0=ta, out=ssim):
        return lib.t2n_ssim_views(_lib.ptr(img0), _lib.ptr(tb), 0, V, H, W, taps, fs, 1e-4, 9e-4, 0, _lib.ptr(out), _lib.ptr(mp), _lib.ptr(sq),
                                  _lib.ptr(ws), ws_bytes, st)

    bad = {"H < filter_size": call(H=10), "W < filter_size": call(W=10), "filter_size 0": call(fs=0), "filter_size 34": call(fs=34),
           "short workspace": call(ws_bytes=need - 1), "V < 1": call(V=0), "NULL image": call(img0=None), "NULL ssim": call(out=None)}
    for what, rc in bad.items():
        assert rc == -1, (what, rc)                           # T2N_ERR_INVALID
    assert b"t2n_ssim_views" in lib.t2n_last_error()
    torch.cuda.synchronize()
    assert bool((ssim == SENT).all()) and bool((mp == SENT).all()) and bool((sq == SENT).all())
    # the Python layer turns the code into ValueError
    with pytest.raises(ValueError, match="workspace"):
        metrics._ssim_call(ta, tb, metrics.gaussian_taps(11, 1.5), 1e-4, 9e-4, False, ssim, mp, sq, workspace=ws[:need - 1])
    with pytest.raises(ValueError, match="filter_size"):
        metrics._ssim_call(ta, tb, np.full(34, 1.0 / 34), 1e-4, 9e-4, False, ssim, mp, sq, workspace=ws)
    for fs in (0, 34):
        with pytest.raises(ValueError):
            metrics.rgb_ssim(ta[0], tb[0], 1, filter_size=fs)
    with pytest.raises(ValueError):
        metrics.rgb_ssim(ta[0, :10], tb[0, :10], 1)
    torch.cuda.synchronize()
    assert bool((ssim == SENT).all()) and bool((mp == SENT).all()) and bool((sq == SENT).all())
    assert call() == 0                                        # and the same arguments, valid, run
    torch.cuda.synchronize()
    assert float(ssim[0]) != SENT and abs(float(sq[0]) - R.sq_err(a[0], b[0])) <= 1e-12 * R.sq_err(a[0], b[0])
