"""The factor gradients of the backward's scatters element by element, at the bin edges (cases: tests/helpers/grad_cases.py; reference,
per-element bound and checker: tests/helpers/grad_elementwise.py; what the cases reach and what the checker catches is shown without a
GPU in tests/test_grad_elementwise_cpu.py).

Routes: the autograd backward (binned scatters on cases A-D and evalB, the sliding-window atomic fallback on E, whose 435-texel line is
one past the LDS budget of the tile accumulate; A-C twice on the same field: the second run uses the forward-kept activation rows), the
composed train step (loss kernel + backward), the one-call fused step in its two-phase form (the gradient read between the phases;
refused on E with T2N_ERR_UNSUPPORTED, as documented), and A-C again under T2N_BWD_ATOMIC_SCATTER=1 in a child process. Every route
checks |got - g64| <= K * bound per element at K = 8 * max(1, rho32) and exact zeros where no sample reaches, beside guards that the
kernel saw the geometry the reference assumed (z bit for bit, the evaluated count) and the whole-tensor `_grad_check` of all 19 tensors
at the gradient fuzz's bound (tests/test_hip_fuzz.py: 5e-4).

Every run prints one `GRADEW` line with the observed max err / bound per tensor kind (profiles/grad_elementwise.txt keeps them)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import adam_readout as A
from tests.helpers import grad_cases as GC
from tests.helpers import grad_elementwise as GE
from tests.test_hip_fullsize import _NoStep
from tests.test_hip_parity import _grad_check, close, make_field

pytestmark = pytest.mark.gpu
TRAIN = [n for n in GC.CASES if GC.CASES[n].is_train]
BINNED = [n for n in TRAIN if n != "caseE"]
REL = 5e-4          # the whole-tensor bound of test_random_configuration_gradients_vs_oracle_autograd


def _field(b):
    return make_field(b["params"], b["grid"], b["aabb"], list(b["case"].near_far))


def _judge(tag, got, ref):
    """Print the observed ratios, then the element-wise check and the whole-tensor one."""
    obs = GE.ratios(got, ref)
    print(f"GRADEW {tag} K {ref.K():.2f} rho32 {ref.rho32:.3f} observed " + " ".join(f"{k} {v:.3f}" for k, v in obs.items()))
    GE.check(got, ref, ref.K())
    _grad_check(got, ref.g64, rel=REL)


def _grads(f):
    return {k: p.grad for k, p in f.named_parameters()}


@pytest.mark.parametrize("name", list(GC.CASES))
def test_autograd_backward(name):
    b, ref = GC.built(name), GC.reference(name, "fuzz")
    c = b["case"]
    f = _field(b)
    loss = GC.fuzz_loss(b)
    for run in range(2 if name in ("caseA", "caseB", "caseC") else 1):
        for p in f.parameters():
            p.grad = None
        torch.manual_seed(c.seed)           # the forward draws the case's jitter from the CPU generator
        out = f(b["rays"], is_train=c.is_train, white_bg=c.white_bg, N_samples=c.n_samples)
        loss(*out).backward()
        close(out[2], ref.z, atol=0, msg=name)
        st = f.stats()
        print(f"{name}: evaluated {st['evaluated']} (oracle {int(ref.valid.sum())}), appearance {st['appearance']} (oracle "
              f"{int(ref.app_mask.sum())}, {int(ref.app_window.sum())} on the knife edge)")
        assert st["evaluated"] == int(ref.valid.sum())
        assert abs(st["appearance"] - int(ref.app_mask.sum())) <= int(ref.app_window.sum())     # flips on the knife edge only
        _judge(f"{name} autograd run {run}", _grads(f), ref)
        if run == 0 and c.is_train:
            assert f._ctx_rows_hint >= 32       # the next forward keeps its activation rows


@pytest.mark.parametrize("name", TRAIN)
def test_composed_train_step(name):
    """train_step with a stand-in optimiser: render, the loss kernel, the backward as separate calls; the gradients stay in .grad.
    (train_step returns no z: the autograd route guards the geometry of the same rays and jitter.)"""
    b, ref = GC.built(name), GC.reference(name, "driver")
    c = b["case"]
    f = _field(b)
    torch.manual_seed(c.seed)
    losses = f.train_step(b["rays"], b["rgb_t"], b["dep_t"], _NoStep(), N_samples=c.n_samples, white_bg=True).cpu().numpy()
    assert f.stats()["evaluated"] == int(ref.valid.sum())
    np.testing.assert_allclose(losses[3], ref.loss, rtol=2e-5)
    _judge(f"{name} composed step", _grads(f), ref)


def _fused(b):
    from text2nerf_amd.optim import TVAdam
    from text2nerf_amd.trainer import FusedStep, _ladder
    c = b["case"]
    f = _field(b)
    opt = TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f)
    torch.manual_seed(c.seed)
    with torch.no_grad():
        f(b["rays"], is_train=True, white_bg=True, N_samples=c.n_samples)
    fs = f.__dict__["_fused_step"] = FusedStep(f, opt)
    fs.rows_cap = _ladder(int(f.stats()["appearance"] * 1.25) + 4096)        # a capacity that holds the batch: nothing is withheld
    return f, opt, fs


@pytest.mark.parametrize("name", BINNED)
def test_fused_train_step(name):
    """t2n_train_step in its two-phase form: the gradient of phase 1 read where an all-reduce would run (factor gradient buffer + the
    head tensors' .grad), before phase 2's Adam consumes it."""
    b, ref = GC.built(name), GC.reference(name, "driver")
    c = b["case"]
    f, opt, fs = _fused(b)
    seen = {}

    def all_reduce():
        g = A.factor_grads_ref(f)
        for k, p in A.kernel_named(f)[12:]:
            g[k] = p.grad.detach().cpu().numpy().astype(np.float64)
        seen["g"], seen["vote"] = g, float(fs.head_grads[-1])

    torch.manual_seed(c.seed)
    f.train_step(b["rays"], b["rgb_t"], b["dep_t"], opt, N_samples=c.n_samples, white_bg=True, fused=True, all_reduce=all_reduce)
    fs.sync()
    assert seen and seen["vote"] == 0.0 and fs.replays == 0
    np.testing.assert_allclose(fs.losses.cpu().numpy()[3], ref.loss, rtol=2e-5)
    _judge(f"{name} fused step", seen["g"], ref)


def test_fused_train_step_refuses_the_grid_beyond_the_lds_budget():
    """Case E's 435-texel line does not fit the tile accumulate: the fused step needs the binned scatters and says so."""
    from text2nerf_amd._lib import T2NError
    b = GC.built("caseE")
    f, opt, fs = _fused(b)
    before = {k: p.detach().clone() for k, p in f.named_parameters()}
    with pytest.raises(T2NError, match=r"code -2\).*binned scatters"):
        f.train_step(b["rays"], b["rgb_t"], b["dep_t"], opt, N_samples=b["case"].n_samples, white_bg=True, fused=True, graph=False)
    torch.cuda.synchronize()
    assert all(torch.equal(before[k], p.detach()) for k, p in f.named_parameters())


def test_atomic_scatter_switch_on_the_edge_cases():
    """Cases A-C through the sliding-window global-atomic scatter (T2N_BWD_ATOMIC_SCATTER=1, read once per process): the autograd route
    in a fresh child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import pytest\n"
            "sys.exit(pytest.main(['-q', '-x', '-s', '-m', 'gpu', '-p', 'no:cacheprovider', '-k', "
            "'test_autograd_backward and (caseA or caseB or caseC)', %r]))\n") % (root, os.path.abspath(__file__))
    env = dict(os.environ, T2N_BWD_ATOMIC_SCATTER="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print("\n".join("atomic switch: " + l for l in r.stdout.splitlines() if l.startswith("GRADEW")))
    assert r.returncode == 0 and "3 passed" in r.stdout, r.stdout[-3000:]
