"""The general-shape render path (csrc/t2n_generic.hip) across its shapes and kernel forms, through the public surface, against the
oracle: the directed cases and fuzz seeds of tests/helpers/generic_cases.py (whose reach over the forms tests/test_generic_cases_cpu.py
asserts on the CPU). Forward: z_vals, weights, rgb, depth and the appearance count against the float64 oracle on the reference's
float32 sample geometry, eval and train mode. Gradients: tests/test_generic_gpu.py's loss against the float64 oracle's autograd, at a
parameter seed that keeps every ReLU input 5e-6 away from zero, on the evenly spaced rays generic_cases.grad_rays picks. The two
large cases run forward only: more than 262 144 list entries (two head passes with work) and a count just under it; both also as two
single-pass halves, which must give the whole render back.

Bounds are the project's (tests/test_hip_parity.py; depth scaled by far / 8 as tests/test_hip_fuzz.py does). Where a head encodes
with more than 6 octaves the rgb bound is max(RGB_ATOL, 4 x max |oracle32 - oracle64|): two float32 evaluations in different orders may
each sit that far from the float64 value, doubled for slack. Each forward prints a `generic_fuzz` line: max |rgb - oracle64|, the
oracle32-64 term, the bound (profiles/generic_fuzz.txt holds a run's table)."""
import numpy as np
import pytest
import torch

from tests.helpers import generic_cases as G
from tests.test_hip_parity import DEPTH_ATOL, RGB_ATOL, W_ATOL, W_RTOL, _grad_check, close, dev

pytestmark = pytest.mark.gpu

SMALL = [c.name for c in G.all_cases() if not c.large]
LARGE = [c.name for c in G.all_cases() if c.large]


def _supply_draws(mp, jit, add_bg):
    """The render call's train-mode draws, fixed: the per-ray jitter (torch.rand(R, 1) on the CPU generator), the NDC path's shared
    row (torch.rand_like on the rays' device) and the background coin of a black-background train render (torch.rand((1,)) < 0.5)."""
    real = torch.rand

    def rand(*size, **kw):
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        if shape == (1,):
            return torch.tensor([0.25 if add_bg else 0.75])
        if jit is not None and shape == tuple(jit.shape):
            return jit.clone()
        return real(*size, **kw)
    mp.setattr(torch, "rand", rand)
    if jit is not None:
        mp.setattr(torch, "rand_like", lambda x, **kw: jit.to(x))


def _render(case, m, is_train, monkeypatch, idx=None, octree=False):
    """One call of the field as a module (or through OctreeRender_trilinear_fast, one chunk): (rgb, depth, z, w)."""
    from text2nerf_amd import OctreeRender_trilinear_fast
    N, jit, add_bg = G.draws(case, is_train)
    rays = torch.from_numpy(case.rays)
    if idx is not None:
        rays = rays[idx]
        if jit is not None and not case.ndc:
            jit = jit[idx]
    white = case.white_train if is_train else True
    with monkeypatch.context() as mp:
        _supply_draws(mp, jit, add_bg)
        if octree:
            rgb, none, depth, w, z = OctreeRender_trilinear_fast(rays, m, chunk=rays.shape[0], N_samples=N, ndc_ray=case.ndc, white_bg=white,
                                                                 is_train=is_train, device=dev())
            assert none is None
            return rgb, depth, z, w
        return m(rays, is_train=is_train, white_bg=white, ndc_ray=case.ndc, N_samples=N)


def _high_octaves(kw):
    fpe = kw["fea_pe"] if kw["shadingMode"] in ("MLP_Fea_noview", "MLP_Fea") else 0
    vpe = kw["view_pe"] if kw["shadingMode"] in ("MLP_Fea", "MLP") else 0
    return max(fpe, vpe) > 6


def _check_forward(case, m, params, vol, is_train, monkeypatch, octree=False, got=None):
    (o_rgb, o_depth, o_z, o_w), _ = G.oracle(case, params, is_train, vol=vol)
    (s_rgb, _, _, _), _ = G.oracle(case, params, is_train, dtype=torch.float32, vol=vol)
    o32 = float((s_rgb.double() - o_rgb).abs().max())
    bound = max(RGB_ATOL, 4.0 * o32) if _high_octaves(case.kw) else RGB_ATOL
    if got is None:
        with torch.no_grad():
            got = _render(case, m, is_train, monkeypatch, octree=octree)
    rgb, depth, z, w = got
    napp, want = m.stats()["appearance"], int((o_w > 1e-4).sum())
    err = float((rgb.double().cpu() - o_rgb).abs().max())
    print(f"generic_fuzz {case.name:14s} {'train' if is_train else 'eval ':5s} R {case.R:6d} N {o_w.shape[1]:3d} list {napp:7d}  "
          f"max|rgb-oracle64| {err:.2e}  oracle32-64 {o32:.2e}  bound {bound:.2e}  max|w-oracle64| {float((w.double().cpu() - o_w).abs().max()):.2e}")
    assert tuple(w.shape) == tuple(o_w.shape) and tuple(z.shape) == tuple(o_z.shape)
    close(z, o_z.numpy(), atol=0, msg=case.name)
    close(w, o_w.numpy(), atol=W_ATOL, rtol=W_RTOL, msg=case.name)
    close(rgb, o_rgb.numpy(), atol=bound, msg=case.name)
    close(depth, o_depth.numpy(), atol=DEPTH_ATOL * max(1.0, case.near_far[1] / 8.0), msg=case.name)
    assert abs(napp - want) <= 2, (case.name, napp, want)
    return got, want


@pytest.mark.parametrize("name", SMALL)
def test_general_shape_case_vs_oracle(name, monkeypatch):
    case = G.case_by_name(name)
    seed, _, _, idx = G.relu_safe_seed(name)
    params = G.make_params(case, seed)
    vol = G.mask_volume(case, params) if case.mask else None
    m = G.make_field(case, params, dev(), vol)
    assert m._is_general()
    counts = [_check_forward(case, m, params, vol, is_train, monkeypatch)[1] for is_train in (False, True)]
    if name == "empty":
        assert counts == [0, 0]
    # gradients, in the case's mode, on its gradient rays
    (o_rgb, o_depth, _, o_w), P = G.oracle(case, params, case.grad_train, vol=vol, requires_grad=True, idx=idx)
    ca = G.colour_weights(case, len(idx))
    out = _render(case, m, case.grad_train, monkeypatch, idx=idx)
    G.grad_loss(out[0], out[1], out[3], ca.to(dev())).backward()
    ref_loss = G.grad_loss(o_rgb, o_depth, o_w, ca.double())
    if not ref_loss.requires_grad:      # no sample survived the box / z gate: the oracle's graph is empty, all gradients must be zero
        assert all(float(p.grad.abs().max()) == 0.0 for p in m.parameters())
        return
    assert name != "empty"
    ref_loss.backward()
    ref = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in P.items()}
    try:
        _grad_check(m, ref, rel=5e-4)
    finally:
        worst = _grad_check.last["max_rel"]
        k = max(worst, key=worst.get)
        print(f"generic_fuzz {case.name:14s} grad  rays {len(idx):4d} worst max|dg|/max|g| {worst[k]:.1e} ({k})")


@pytest.mark.parametrize("name", LARGE)
def test_multi_pass_head_vs_oracle_and_vs_its_single_pass_halves(name, monkeypatch):
    """More rows than one pass of the matrix-core head holds (262 144): passes at row0 = 0, 262 144, ... clipped to the list count on
    the device. The same rays as two halves run the same kernels in ONE pass each, so the whole render must equal their concatenation
    (rgb, weights to 2e-7; the depth sums to 2e-6 at depths up to 7): nothing may depend on row0."""
    from text2nerf_amd import tensorf
    case = G.DIRECTED[name]
    params = G.make_params(case, case.seed0)
    with torch.no_grad():
        (_, _, _, o_w), _ = G.oracle(case, params, case.count_mode)
    want = int((o_w > 1e-4).sum())
    if name == "two_pass":              # (asserted from the oracle before the GPU is touched)
        assert want > G.PASS_ROWS + 64
    else:
        assert G.PASS_ROWS - 64 < want < G.PASS_ROWS
    m = G.make_field(case, params, dev())
    half = case.R // 2
    assert case.R * case.n_train > G.PASS_ROWS >= (case.R - half) * case.n_train
    try:
        for is_train in (False, True):
            got, count = _check_forward(case, m, params, None, is_train, monkeypatch, octree=True)
            if is_train == case.count_mode:
                assert count == want
            with torch.no_grad():
                a = _render(case, m, is_train, monkeypatch, idx=slice(0, half))
                b = _render(case, m, is_train, monkeypatch, idx=slice(half, case.R))
            for i, tol in ((0, 2e-7), (3, 2e-7), (1, 2e-6)):
                close(torch.cat([a[i], b[i]]), got[i].cpu().numpy(), atol=tol, msg=f"{name}: halves vs whole, output {i}")
            assert torch.equal(torch.cat([a[2], b[2]]), got[2])
            del got, a, b
    finally:
        tensorf._WORKSPACE.clear()
        torch.cuda.empty_cache()
