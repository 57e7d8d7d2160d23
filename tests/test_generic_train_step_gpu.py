"""TensorVMSplit.train_step / train_step_indexed on general-shape fields (the composed route: t2n_generic_forward -> t2n_train_loss[_ex]
-> t2n_generic_backward[_staged] -> .grad in the reference layouts -> TVAdam without `field=`): one step with every learning rate 0
against the float64 reference step (render + TV; tests/helpers/generic_train.py), three steps at the driver's learning rates against
the autograd-form step, the indexed form, a depth term other than "mse", and the argument behaviour. Before this route existed every
one of these calls raised T2NError in _kernel_shape()."""
import numpy as np
import pytest
import torch

from tests.helpers import depth_loss_ref as DL
from tests.helpers import generic_cases as G
from tests.helpers import generic_train as T
from tests.helpers import optim_ref
from tests.test_generic_fuzz import _supply_draws
from tests.test_hip_parity import DEPTH_ATOL, RGB_ATOL, W_ATOL, W_RTOL, _grad_check, dev
from tests.test_train_step import assert_same_trajectory, step_autograd

pytestmark = pytest.mark.gpu

REL = 5e-4
LOSS_RTOL = 1e-5            # tests/test_train_step.py: train_step's losses against the autograd-form step's
KERNEL_RTOL = 2e-6          # tests/test_train_step.py::test_fused_loss_kernel_matches_torch_loss_and_autograd: the loss kernel's own float32 sums


def _field(name):
    case, params, vol = T.case_inputs(name)
    m = G.make_field(case, params, dev(), vol)
    assert m._is_general()
    return case, m


def _optimizer(m, lr_spatial=0.02, lr_network=1e-3):
    from text2nerf_amd.optim import TVAdam
    return TVAdam(m.get_optparam_groups(lr_spatial, lr_network), betas=(0.9, 0.99))


def _tv(m, weights=T.TV_WEIGHTS):
    return [(m.density_plane, weights[0]), (m.app_plane, weights[1])]


def _step(case, m, opt, monkeypatch, **kw):
    """One train_step with the case's fixed draws (per-ray jitter, background coin)."""
    N, jit, add_bg = G.draws(case, True)
    rgb_t, dep_t = T.targets(case)
    with monkeypatch.context() as mp:
        _supply_draws(mp, jit, add_bg)
        return m.train_step(torch.from_numpy(case.rays), rgb_t, dep_t, opt, N_samples=N, white_bg=case.white_train, **kw)


def _loss_bounds(case, ref, rgb_t, dep_t):
    """How far the four losses may sit from the oracle's, from the forward tolerances the project already uses (tests/test_generic_fuzz.py):
    an output within d of the oracle's moves a mean of squared errors e^2 by at most mean(2 |e| d + d^2)."""
    e = np.abs(ref["rgb"].astype(np.float64) - rgb_t.numpy())
    b_mse = float((2 * e * RGB_ATOL + RGB_ATOL ** 2).mean())
    dd = DEPTH_ATOL * max(1.0, case.near_far[1] / 8.0)
    ed = np.abs(ref["depth"].astype(np.float64) - dep_t.numpy())
    b_dep = float((2 * ed * dd + dd ** 2).mean())
    w, z = ref["w"].astype(np.float64), np.broadcast_to(ref["z"].astype(np.float64), ref["w"].shape)
    mask = ((z - dep_t.numpy().astype(np.float64)[:, None]) + T.DELTA) < 0
    m = (w * mask).mean(1)
    dm = ((W_ATOL + W_RTOL * np.abs(w)) * mask).mean(1)
    b_tr = float((2 * np.abs(m) * dm + dm ** 2).mean())
    return np.array([b_mse, b_dep, b_tr, b_mse + T.W_DEPTH * b_dep + T.W_TRANS * b_tr]), dd


@pytest.mark.parametrize("name", T.STEP_CASES)
def test_one_step_at_zero_learning_rates_vs_reference_step(name, monkeypatch):
    case, m = _field(name)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    opt = _optimizer(m, 0.0, 0.0)
    losses = _step(case, m, opt, monkeypatch, tv=_tv(m))
    ref = T.reference_step(name, tv_weights=T.TV_WEIGHTS)
    try:
        _grad_check(m, ref["grads"], rel=REL)
    finally:
        worst = _grad_check.last["max_rel"]
        k = max(worst, key=worst.get)
        print(f"generic_train {name:12s} step grads worst max|dg|/max|g| {worst[k]:.1e} ({k})")
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), f"{k} changed at learning rate 0"
    assert all(int(opt.state[p]["step"]) == 1 for p in m.parameters())
    bounds, _ = _loss_bounds(case, ref, *T.targets(case))
    got = losses.double().cpu().numpy()
    print(f"generic_train {name:12s} losses {got}  oracle {ref['losses']}  bounds {bounds}")
    assert losses.shape == (4,) and losses.device.type == "cuda"
    assert np.all(np.abs(got - ref["losses"]) <= bounds + KERNEL_RTOL * np.abs(ref["losses"])), (got, ref["losses"], bounds)


@pytest.mark.parametrize("name", ["odd_rows", "sh_odd"])
def test_three_steps_equal_the_autograd_form(name):
    """text2nerf_main.py:547-601 with decaying learning rates and TV weights, as tests/test_train_step.py drives the tuned path."""
    case, fa = _field(name)
    _, fb = _field(name)
    oa, ob = _optimizer(fa), _optimizer(fb)
    rays = torch.from_numpy(case.rays)
    rgb_t, dep_t = T.targets(case)
    steps = 3
    for it in range(steps):
        w_d, w_a = 0.1 * 0.9 ** it, 0.01 * 0.8 ** it
        for o in (oa, ob):
            for g in o.param_groups:
                g["lr"] = g["lr"] * 0.97
        torch.manual_seed(100 + it)
        la = step_autograd(fa, oa, rays, rgb_t, dep_t)
        oa.step(tv=_tv(fa, (w_d, w_a)))
        torch.manual_seed(100 + it)
        lb = fb.train_step(rays, rgb_t, dep_t, ob, N_samples=-1, white_bg=True, tv=_tv(fb, (w_d, w_a))).clone()
        assert torch.allclose(la, lb, rtol=LOSS_RTOL, atol=1e-9), (it, la, lb)
    assert all(int(ob.state[p]["step"]) == steps for p in fb.parameters())
    assert_same_trajectory(fa, fb, steps=steps)


def test_train_step_indexed_equals_train_step():
    from text2nerf_amd.dataset import DeviceTrainSet
    case, fa = _field("odd_rows")
    _, fb = _field("odd_rows")
    oa, ob = _optimizer(fa), _optimizer(fb)
    rays = torch.from_numpy(case.rays)
    rgb_t, dep_t = T.targets(case)
    source = DeviceTrainSet(rays, rgb_t, dep_t, device=dev())
    ids = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).permutation(case.R)[:150].astype(np.int64))
    torch.manual_seed(7)
    la = fa.train_step(rays[ids], rgb_t[ids], dep_t[ids], oa, tv=_tv(fa)).clone()
    torch.manual_seed(7)
    lb = fb.train_step_indexed(source, ids, ob, tv=_tv(fb)).clone()
    assert torch.allclose(la, lb, rtol=LOSS_RTOL, atol=1e-9), (la, lb)
    assert_same_trajectory(fa, fb, steps=1)


def test_one_step_with_si_log_depth_term(monkeypatch):
    name = "odd_rows"
    case, m = _field(name)
    opt = _optimizer(m, 0.0, 0.0)
    losses = _step(case, m, opt, monkeypatch, depth_loss="si_log")
    assert m.last_depth_aux is not None and m.last_depth_aux.dtype == torch.float64 and m.last_depth_aux.device.type == "cuda"
    ref = T.reference_step(name)
    rgb_t, dep_t = T.targets(case)
    want = DL.si_log(ref["depth"], dep_t.numpy())
    _, dd = _loss_bounds(case, ref, rgb_t, dep_t)
    # |log(mu + d) - log(mu)| <= d / (mu - d) per ray; the term is mean |u_r + alpha| with alpha = -mean u: each |.| moves by at most
    # its own ray's change plus the mean's, so the mean of them by at most twice the mean change
    mu = ref["depth"].astype(np.float64)
    assert float(mu.min()) > 10 * dd
    bound = 2.0 * float((dd / (mu - dd)).mean())
    got = float(losses[1])
    print(f"generic_train {name:12s} si_log term {got:.6f} oracle {want['loss']:.6f} bound {bound:.2e}  alpha {float(m.last_depth_aux[0]):.6f} oracle {want['alpha']:.6f}")
    assert abs(got - want["loss"]) <= bound + KERNEL_RTOL * abs(want["loss"])
    assert abs(float(m.last_depth_aux[0]) - want["alpha"]) <= bound + KERNEL_RTOL * abs(want["alpha"])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_argument_behaviour(monkeypatch):
    from text2nerf_amd._lib import T2NError
    from text2nerf_amd.optim import TVAdam
    case, m = _field("tiny_head")
    opt = _optimizer(m)
    with pytest.raises(T2NError):
        _step(case, m, opt, monkeypatch, fused=True)
    with pytest.raises(T2NError):
        TVAdam(m.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=m)
    # all_reduce runs exactly once, between backward (gradients installed, render terms only) and the step (parameters unchanged, no
    # Adam state yet)
    seen = []
    start = {k: v.detach().clone() for k, v in m.state_dict().items()}

    def all_reduce():
        seen.append((all(p.grad is not None for p in m.parameters()), all(torch.equal(v, start[k]) for k, v in m.state_dict().items()),
                     len(opt.state)))
    _step(case, m, opt, monkeypatch, all_reduce=all_reduce, speculative=True, graph=True)       # (speculative / graph: no effect here)
    assert seen == [(True, True, 0)], seen
    assert any(not torch.equal(v, start[k]) for k, v in m.state_dict().items())
    assert all(int(opt.state[p]["step"]) == 1 for p in m.parameters())
    # any torch.optim optimiser when tv is empty
    sgd = torch.optim.SGD(m.parameters(), lr=0.0)
    assert _step(case, m, sgd, monkeypatch).shape == (4,)


def test_step_on_an_empty_frame_changes_only_what_tv_and_adam_change(monkeypatch):
    """No sample in the box: the render gradients are exactly zero, so the planes listed in `tv` move by Adam's step on the TV gradient
    and every other tensor by Adam's step on a zero gradient, which is no move at all (m = v = 0: the update is 0 / (0 + eps))."""
    case, m = _field("empty")
    start = {k: v.detach().clone() for k, v in m.state_dict().items()}
    opt = _optimizer(m)
    _step(case, m, opt, monkeypatch, tv=_tv(m))
    assert m.stats()["appearance"] == 0
    ref = {k: np.zeros_like(v) for k, v in T.case_inputs("empty")[1].items()}
    for k in range(3):
        for grp, w in (("density_plane", T.TV_WEIGHTS[0]), ("app_plane", T.TV_WEIGHTS[1])):
            ref[f"{grp}.{k}"] = optim_ref.tv_grad(start[f"{grp}.{k}"].cpu().numpy(), w * 1e-2)[0]
    _grad_check(m, ref, rel=2e-6)
    for k, v in m.state_dict().items():
        if "plane" in k:
            assert not torch.equal(v, start[k]), k
        else:
            assert torch.equal(v, start[k]), k
