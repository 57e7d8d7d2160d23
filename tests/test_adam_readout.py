"""CPU checks of tests/helpers/adam_readout.py, the float64 readout the full-size fused-step tests (tests/test_train_step_fullsize.py)
depend on: the gradient recovered from Adam's first moments, the float64 recomputation of the parameter update and the channel-last
layout mapping, all against torch.optim.Adam run on known gradients."""
import numpy as np
import torch

from tests.helpers import adam_readout as A

SHAPES = {"plane": (1, 16, 7, 5), "line": (1, 48, 9, 1), "head": (27, 144)}


def _adam_run(steps=3, seed=0):
    """torch.optim.Adam(betas=(0.9, 0.99)) with two learning-rate groups; returns the start and, per step, the known gradient and the
    parameters and moments after the step (float32, as torch keeps them)."""
    g = torch.Generator().manual_seed(seed)
    ps = {k: torch.randn(s, generator=g).requires_grad_(True) for k, s in SHAPES.items()}
    opt = torch.optim.Adam([{"params": [ps["plane"], ps["line"]], "lr": 0.02}, {"params": [ps["head"]], "lr": 1e-3}], betas=(0.9, 0.99))
    lr = {"plane": 0.02, "line": 0.02, "head": 1e-3}
    start = {k: p.detach().clone().numpy() for k, p in ps.items()}
    hist = []
    for _ in range(steps):
        grads = {k: torch.randn(s, generator=g) * float(torch.rand(1, generator=g) * 3 + 0.1) for k, s in SHAPES.items()}
        for k, p in ps.items():
            p.grad = grads[k].clone()
        opt.step()
        hist.append({k: dict(g=grads[k].numpy().copy(), p=p.detach().numpy().copy(), m=opt.state[p]["exp_avg"].numpy().copy(),
                             v=opt.state[p]["exp_avg_sq"].numpy().copy(), step=int(opt.state[p]["step"])) for k, p in ps.items()})
    return start, hist, lr


def test_gradient_recovered_from_first_moments_of_torch_adam():
    start, hist, _ = _adam_run()
    omb1 = float(np.float32(1.0 - 0.9))          # torch's lerp takes (1 - beta1) as a double and multiplies by its float32 value
    for k in SHAPES:
        m_prev = np.zeros(SHAPES[k])
        for t, h in enumerate(hist, 1):
            g = A.recover_grad(m_prev, h[k]["m"], omb1)
            want = h[k]["g"].astype(np.float64)
            err = np.abs(g - want)
            assert float(err.max()) <= 1e-6 * float(np.abs(want).max()), (k, t, float(err.max()))
            assert np.all(err <= 1e-6 * np.abs(want) + 1e-6 * float(np.abs(h[k]["m"]).max())), (k, t)
            m_prev = h[k]["m"]


def test_float64_recomputation_reproduces_torch_adam():
    start, hist, lr = _adam_run()
    omb1, omb2 = float(np.float32(1.0 - 0.9)), float(np.float32(1.0 - 0.99))
    for k in SHAPES:
        p_prev, m_prev, v_prev = start[k], np.zeros(SHAPES[k]), np.zeros(SHAPES[k])
        for t, h in enumerate(hist, 1):
            assert h[k]["step"] == t
            want = A.adam_param(p_prev, h[k]["m"], h[k]["v"], lr[k], t, 0.9, 0.99, 1e-8)
            d = np.abs(h[k]["p"].astype(np.float64) - want)
            tol = A.param_tolerance(h[k]["p"], want - p_prev)
            assert np.all(d <= tol), (k, t, float((d / tol).max()))
            # and the tolerance has teeth: the next step's bias correction, or another group's learning rate, is far outside it
            wrong = A.adam_param(p_prev, h[k]["m"], h[k]["v"], lr[k], t + 1, 0.9, 0.99, 1e-8)
            assert np.mean(np.abs(h[k]["p"] - wrong) > tol) > 0.9, (k, t)
            other = 1e-3 if lr[k] == 0.02 else 0.02
            wrong = A.adam_param(p_prev, h[k]["m"], h[k]["v"], other, t, 0.9, 0.99, 1e-8)
            assert np.mean(np.abs(h[k]["p"] - wrong) > tol) > 0.9, (k, t)
            # second moment from the recovered gradient
            g = A.recover_grad(m_prev, h[k]["m"], omb1)
            v = A.adam_second_moment(v_prev, g, 0.99, omb2)
            assert np.all(np.abs(v - h[k]["v"]) <= 1e-6 * np.abs(h[k]["v"]) + 1e-30), (k, t)
            p_prev, m_prev, v_prev = h[k]["p"], h[k]["m"], h[k]["v"]


def test_kernel_constants():
    assert A.F32_BETAS == (float(np.float32(0.9)), float(np.float32(0.99)))
    assert A.one_minus(0.9) == 0.10000002384185791         # (1.f - 0.9f), the factor k_adam_multi / adam_one multiply by
    assert A.one_minus(0.99) == float(np.float32(1.0) - np.float32(0.99))


def test_channel_last_layout_round_trips():
    rng = np.random.default_rng(3)
    plane = rng.standard_normal((1, 5, 4, 3))
    line = rng.standard_normal((1, 8, 6, 1))
    cl = A.ref_to_cl(plane, line=False)
    assert cl.shape == (5 * 4 * 3,)
    for c, h, w in ((0, 0, 0), (4, 3, 2), (2, 1, 0), (3, 0, 2)):
        assert cl[(h * 3 + w) * 5 + c] == plane[0, c, h, w]        # [H, W, C]
    assert np.array_equal(A.cl_to_ref(cl, plane.shape, line=False), plane)
    assert np.array_equal(A.ref_to_cl(A.cl_to_ref(cl, plane.shape, line=False), line=False), cl)
    cl = A.ref_to_cl(line, line=True)
    for c, l in ((0, 0), (7, 5), (3, 2)):
        assert cl[l * 8 + c] == line[0, c, l, 0]                   # [L, C]
    assert np.array_equal(A.cl_to_ref(cl, line.shape, line=True), line)
    assert np.array_equal(A.ref_to_cl(A.cl_to_ref(cl, line.shape, line=True), line=True), cl)
    # kernel order: planes and lines alternate in groups of three
    assert [A.is_line(i) for i in range(12)] == [False] * 3 + [True] * 3 + [False] * 3 + [True] * 3
