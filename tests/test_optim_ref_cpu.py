"""CPU checks of tests/helpers/optim_ref.py, the float64 references tests/test_optim_kernels_gpu.py holds the TV, Adam and loss
kernels to: each against the authority the repository already has — losses.TVLoss under float64 autograd, torch.optim.Adam in
float64, the torch restatement of the driver's loss in tests/test_train_step.py under float64 autograd — plus a brute-force
evaluation of the TV stencil's terms (for `mag`, which no autograd gives) and a float32 emulation of k_tv_grad's arithmetic that
shows the GPU test's bound of 1e-6 mag is one the kernel's number format can meet at the shapes and value scales it uses."""
import numpy as np
import pytest
import torch

from tests.helpers import adam_readout as A
from tests.helpers import optim_ref as R


@pytest.mark.parametrize("shape", [(1, 2, 2), (3, 2, 7), (2, 5, 2), (4, 6, 9)])
def test_tv_reference_matches_tvloss_autograd(shape):
    from text2nerf_amd.losses import TVLoss
    rng = np.random.default_rng(1)
    x = rng.normal(0.1, 1.0, (1,) + shape)
    weight = 0.37
    t = torch.from_numpy(x).requires_grad_(True)
    loss = TVLoss(weight)(t)
    loss.backward()
    grad, mag = R.tv_grad(x, weight)
    want = t.grad.numpy()
    assert np.abs(grad - want).max() <= 1e-13 * np.abs(want).max()
    assert abs(R.tv_value(x, weight) - float(loss.detach())) <= 1e-13 * float(loss.detach())
    dh, dw = x[:, :, 1:] - x[:, :, :-1], x[..., 1:] - x[..., :-1]
    assert R.tv_sums(x) == (float((dh * dh).sum()), float((dw * dw).sum()))
    # the terms one by one (what the kernels add up), for mag
    _, c, h, w = x.shape
    sh, sw = weight * 2.0 / (c * (h - 1) * w), weight * 2.0 / (c * h * (w - 1))
    for ci in range(c):
        for y in range(h):
            for xx in range(w):
                v = x[0, ci, y, xx]
                terms = []
                if y > 0: terms.append(sh * 2.0 * (v - x[0, ci, y - 1, xx]))
                if y < h - 1: terms.append(-sh * 2.0 * (x[0, ci, y + 1, xx] - v))
                if xx > 0: terms.append(sw * 2.0 * (v - x[0, ci, y, xx - 1]))
                if xx < w - 1: terms.append(-sw * 2.0 * (x[0, ci, y, xx + 1] - v))
                assert abs(sum(terms) - grad[0, ci, y, xx]) <= 1e-14 * mag[0, ci, y, xx]
                assert abs(sum(abs(t_) for t_ in terms) - mag[0, ci, y, xx]) <= 1e-14 * mag[0, ci, y, xx]
    assert np.all(mag >= np.abs(grad) * (1 - 1e-14))


def tv_grad_f32(x, weight):
    """k_tv_grad's arithmetic in numpy float32 (csrc/t2n_optim.hip: sh, sw as the host rounds them, no contraction). The four passes
    run over the whole array in turn, but each element receives its own terms in the kernel's sequence - up, down, left, right, the
    missing ones skipped - onto an accumulator that starts at 0, so every element sees the kernel's roundings in the kernel's order."""
    f = np.float32
    x = np.asarray(x, f)
    _, c, h, w = x.shape
    sh = f(weight) * f(2) / (f(c) * f(h - 1) * f(w))
    sw = f(weight) * f(2) / (f(c) * f(h) * f(w - 1))
    acc = np.zeros_like(x)
    acc[:, :, 1:, :] += sh * (f(2) * (x[:, :, 1:, :] - x[:, :, :-1, :]))
    acc[:, :, :-1, :] -= sh * (f(2) * (x[:, :, 1:, :] - x[:, :, :-1, :]))
    acc[:, :, :, 1:] += sw * (f(2) * (x[:, :, :, 1:] - x[:, :, :, :-1]))
    acc[:, :, :, :-1] -= sw * (f(2) * (x[:, :, :, 1:] - x[:, :, :, :-1]))
    assert acc.dtype == f
    return acc


@pytest.mark.parametrize("scale", R.VALUE_SCALES)
def test_float32_stencil_meets_the_gpu_bound(scale):
    """1e-6 mag per element is met by a float32 evaluation in the kernel's order at every shape and scale of the GPU test (about a third
    of it at worst), and a stencil that drops its last-row term is far outside it."""
    rng = np.random.default_rng(2)
    worst = 0.0
    for shape in R.TV_GRAD_SHAPES:
        x = R.plane(rng, shape, scale)
        grad, mag = R.tv_grad(x, 0.37)
        err = np.abs(tv_grad_f32(x, 0.37).astype(np.float64) - grad)
        assert np.all(err <= 1e-6 * mag), (shape, float((err / mag).max()))
        worst = max(worst, float((err / np.maximum(mag, 1e-300)).max()))
        broken = grad.copy()
        sh = R.tv_scales(x.shape, 0.37)[0]
        xd = x.astype(np.float64)
        broken[:, :, :-1, :] += 2.0 * sh * (xd[:, :, 1:, :] - xd[:, :, :-1, :])       # the `h < H - 1` term left out
        assert np.mean(np.abs(broken - grad) > 1e-6 * mag) > 0.4, shape
    print(f"float32 emulation, scale {scale}: worst error {worst:.2e} of mag")
    assert worst <= 5.4e-7          # nine roundings


def test_adam_reference_matches_torch_adam_in_float64():
    """Three steps of torch.optim.Adam on float64 tensors with the kernels' float32 betas, two learning rates, gradients with exact
    zeros and magnitudes from 1e-15 to 1e15: parameters and both moments after every step."""
    b1, b2 = A.F32_BETAS
    rng = np.random.default_rng(3)
    shapes = {"a": (7, 5), "b": (33,)}
    lr = {"a": 0.02, "b": 1e-3}
    ps = {k: torch.from_numpy(rng.standard_normal(s)).requires_grad_(True) for k, s in shapes.items()}
    opt = torch.optim.Adam([{"params": [ps[k]], "lr": lr[k]} for k in shapes], betas=(b1, b2), eps=1e-8)
    mine = {k: (ps[k].detach().numpy().copy(), np.zeros(s), np.zeros(s)) for k, s in shapes.items()}
    for t in range(1, 4):
        for k, s in shapes.items():
            g = rng.standard_normal(s) * 10.0 ** rng.uniform(-15, 15, s)
            g[rng.random(s) < 0.2] = 0.0
            ps[k].grad = torch.from_numpy(g.copy())
            mine[k] = R.adam_step(*mine[k][:1], g, *mine[k][1:], lr[k], t)
        opt.step()
        for k in shapes:
            st = opt.state[ps[k]]
            assert int(st["step"]) == t
            for got, want in zip(mine[k], (ps[k].detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy())):
                assert np.all(np.abs(got - want) <= 1e-13 * np.abs(want) + 1e-300), (k, t)
    # (1 - beta) as the kernels form it is what torch forms in double from the float32 beta
    assert A.one_minus(b1) == 1.0 - b1 and A.one_minus(b2) == 1.0 - b2
    # a zero gradient on zero moments leaves the parameter where it is
    p, m, v = R.adam_step(np.array([0.3]), np.array([0.0]), np.array([0.0]), np.array([0.0]), 0.02, 1)
    assert p[0] == 0.3 and m[0] == 0.0 and v[0] == 0.0


@pytest.mark.parametrize("R_,N", [(1, 1), (6, 65), (301, 37)])
def test_driver_loss_reference_matches_torch_loss_autograd(R_, N):
    from tests.test_train_step import torch_loss
    rng = np.random.default_rng(4)
    rgb, rgb_t = rng.random((R_, 3)), rng.random((R_, 3))
    depth, dep_t = rng.random(R_) * 6 + 1, rng.random(R_) * 5 + 2
    if R_ >= 5:
        depth[3] = np.nan
    w, z = rng.random((R_, N)) * 0.05, np.sort(rng.random((R_, N)), 1) * 8
    t = {k: torch.from_numpy(a.copy()).requires_grad_(k in ("rgb", "depth", "w"))
         for k, a in dict(rgb=rgb, depth=depth, w=w, z=z, rgb_t=rgb_t, dep_t=dep_t).items()}
    mse, dl, tl, tot = torch_loss(t["rgb"], t["depth"], t["w"], t["z"], t["rgb_t"], t["dep_t"])
    tot.backward()
    losses, d_rgb, d_depth, d_w = R.driver_loss(rgb, depth, w, z, rgb_t, dep_t, 0.005, 1e3, 0.1)
    want = np.array([float(v.detach()) for v in (mse, dl, tl, tot)])
    assert np.all(np.abs(losses - want) <= 1e-13 * np.abs(want))
    for got, ref in ((d_rgb, t["rgb"].grad), (d_depth, t["depth"].grad), (d_w, t["w"].grad)):
        ref = ref.numpy()
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-13 * np.abs(ref).max() + 1e-300
    if R_ >= 5:
        assert d_depth[3] == 0.0
    mask = (z - dep_t[:, None] + 0.1) < 0
    assert np.all(d_w[~mask] == 0.0) and (N == 1 or mask.any())
    # other weights: the total and the two weighted gradients follow them, the three means do not
    l2, r2, dd2, dw2 = R.driver_loss(rgb, depth, w, z, rgb_t, dep_t, 0.0, 0.0, 0.1)
    assert np.array_equal(l2[:3], losses[:3]) and l2[3] == losses[0]
    assert np.array_equal(r2, d_rgb) and not dd2.any() and not dw2.any()
