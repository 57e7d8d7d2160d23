"""Float64 references of the dense tail of a training step (csrc/t2n_optim.hip, csrc/t2n_loss.hip): the total-variation regulariser
of a [1, C, H, W] plane, torch.optim.Adam's update and the driver's loss with its three upstream gradients. Plain numpy; held to
losses.TVLoss, torch.optim.Adam and the torch restatement of the loss (tests/test_train_step.py) in tests/test_optim_ref_cpu.py.
The GPU tests (tests/test_optim_kernels_gpu.py) hold the kernels to these."""
import numpy as np

from tests.helpers import adam_readout as A


TV_GRAD_SHAPES = [(16, 2, 2), (16, 2, 130), (48, 5, 65), (3, 300, 2), (16, 37, 5), (48, 352, 3)]     # (C, H, W) of the gradient tests
VALUE_SCALES = ("unit", "small", "offset")


def plane(rng, shape, scale):
    """A seeded float32 test plane [1, C, H, W] at one of three value scales: N(0.1, 1), 1e-3 N(0.1, 1), 50 N(0.1, 1) + 1500."""
    n = rng.normal(0.1, 1.0, (1,) + tuple(shape))
    return {"unit": n, "small": 1e-3 * n, "offset": 50.0 * n + 1500.0}[scale].astype(np.float32)


def _plane(x):
    x = np.asarray(x, np.float64)
    assert x.ndim == 4 and x.shape[0] == 1 and x.shape[2] >= 2 and x.shape[3] >= 2, x.shape
    return x


def tv_scales(shape, weight):
    """(sh, sw): weight * 2 / (C (H-1) W) and weight * 2 / (C H (W-1)), the factors of the two sums of squares in TVLoss (batch 1)."""
    _, c, h, w = shape
    return float(weight) * 2.0 / (c * (h - 1) * w), float(weight) * 2.0 / (c * h * (w - 1))


def tv_sums(x):
    """TVLoss's two sums of squares of one plane: sum (x[c,y+1,x] - x[c,y,x])^2 and sum (x[c,y,x+1] - x[c,y,x])^2."""
    x = _plane(x)
    dh = x[:, :, 1:, :] - x[:, :, :-1, :]
    dw = x[:, :, :, 1:] - x[:, :, :, :-1]
    return float((dh * dh).sum()), float((dw * dw).sum())


def tv_grad(x, weight):
    """(grad, mag) of weight * 2 * (sum dh^2 / (C (H-1) W) + sum dw^2 / (C H (W-1))) with respect to the plane x [1, C, H, W]:
    grad[h, w] = sh 2 (x - up) - sh 2 (down - x) + sw 2 (x - left) - sw 2 (right - x), each term only where that neighbour exists;
    mag = the sum of the absolute values of those (up to four) terms, the scale a float32 evaluation's rounding error is relative to."""
    x = _plane(x)
    sh, sw = tv_scales(x.shape, weight)
    dh = 2.0 * sh * (x[:, :, 1:, :] - x[:, :, :-1, :])      # term between rows y and y + 1
    dw = 2.0 * sw * (x[:, :, :, 1:] - x[:, :, :, :-1])
    grad, mag = np.zeros_like(x), np.zeros_like(x)
    grad[:, :, 1:, :] += dh; mag[:, :, 1:, :] += np.abs(dh)      # the lower element of a pair: + sh 2 (x - up)
    grad[:, :, :-1, :] -= dh; mag[:, :, :-1, :] += np.abs(dh)    # the upper one: - sh 2 (down - x)
    grad[:, :, :, 1:] += dw; mag[:, :, :, 1:] += np.abs(dw)
    grad[:, :, :, :-1] -= dw; mag[:, :, :, :-1] += np.abs(dw)
    return grad, mag


def tv_value(x, weight):
    """TVLoss(weight)(x) from the two sums."""
    sh, sw = tv_scales(np.shape(x), weight)
    s = tv_sums(x)
    return sh * s[0] + sw * s[1]


def adam_first_moment(m_prev, g, one_minus_beta1):
    """m_t = m_{t-1} + (g - m_{t-1}) (1 - beta1): exp_avg.lerp_(grad, 1 - beta1)."""
    m_prev = np.asarray(m_prev, np.float64)
    return m_prev + (np.asarray(g, np.float64) - m_prev) * float(one_minus_beta1)


def adam_step(p, g, m, v, lr, step, beta1=A.F32_BETAS[0], beta2=A.F32_BETAS[1], eps=1e-8):
    """One torch.optim.Adam update (no weight decay, no amsgrad) in float64: (p_t, m_t, v_t). The betas are the kernels' float32 values
    by default, and (1 - beta) is evaluated the way the kernels do (adam_readout.one_minus)."""
    m_t = adam_first_moment(m, g, A.one_minus(beta1))
    v_t = A.adam_second_moment(v, g, beta2, A.one_minus(beta2))
    return A.adam_param(p, m_t, v_t, lr, step, beta1, beta2, eps), m_t, v_t


def driver_loss(rgb, depth, w, z, rgb_t, depth_t, w_depth, w_trans, delta):
    """The driver's loss (csrc/t2n_loss.hip:1-5) in float64: mean((rgb - rgb_t)^2) + w_depth mean((depth - depth_t)^2) + w_trans
    mean_r(m_r^2), m_r = mean_n(w[r, n] [z[r, n] - depth_t[r] + delta < 0]); a NaN depth counts as 0 and gets no gradient.
    Returns (losses [mse, depth loss, transmittance loss, total], d_rgb [R, 3], d_depth [R], d_w [R, N])."""
    rgb, depth, w, z = (np.asarray(a, np.float64) for a in (rgb, depth, w, z))
    rgb_t, depth_t = np.asarray(rgb_t, np.float64), np.asarray(depth_t, np.float64)
    R, N = w.shape
    bad = np.isnan(depth)
    dep = np.where(bad, 0.0, depth)
    e = rgb - rgb_t
    dd = dep - depth_t
    mask = ((z - depth_t[:, None]) + float(delta)) < 0
    m = (w * mask).sum(1) / N
    mse, dl, tl = float((e * e).mean()), float((dd * dd).mean()), float((m * m).mean())
    losses = np.array([mse, dl, tl, mse + float(w_depth) * dl + float(w_trans) * tl], np.float64)
    d_rgb = 2.0 * e / (3.0 * R)
    d_depth = np.where(bad, 0.0, 2.0 * float(w_depth) * dd / R)
    d_w = mask * (2.0 * float(w_trans) * m / (R * N))[:, None]
    return losses, d_rgb, d_depth, d_w
