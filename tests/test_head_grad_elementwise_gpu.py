"""The gradients of the seven head tensors element by element, at the row-count and range edges of the head backward (cases:
tests/helpers/head_grad_cases.py; reference, per-element bound and checker: tests/helpers/head_grad_elementwise.py; what the cases
reach and what the checker catches is shown without a GPU in tests/test_head_grad_elementwise_cpu.py).

Routes: the autograd backward at default precision (the fused split-f16 chain and k_gemm_tn_b<4, true / false>; 32, 33 and the chunk
case twice on the same field: the second run uses the forward-kept activation rows), the same under mlp_exact_fp32 (k_gemm_tn,
k_gemm_nn, k_colsum), the MLP_Fea head (the five-launch form with k_gemm_nn_h), the composed train_step(speculative=True) with a
stand-in optimiser (the rows_dev re-cut of the chunks and of k_bwd_l2; the second step takes the device-side row count) and the
one-call fused step in its two-phase form (the gradient read between the phases). Every route checks |got - g64| <= K * bound per
element at the CPU-measured K = 8 * max(1, rho32) and exact zeros where no row contributes, beside guards that the kernel saw the
rows the reference assumed (z bit for bit, the evaluated count, the appearance count equal to the target exactly) and the
whole-tensor `_grad_check` of all 19 tensors at 5e-4.

Every run prints one `HEADEW` line with the observed max err / bound per tensor (profiles/head_grad_elementwise.txt keeps them)."""
import numpy as np
import pytest
import torch

from tests.helpers import adam_readout as A
from tests.helpers import grad_elementwise as GE
from tests.helpers import head_grad_cases as HC
from tests.helpers import head_grad_elementwise as HE
from tests.test_hip_fullsize import _NoStep
from tests.test_hip_parity import _grad_check, close, dev

pytestmark = pytest.mark.gpu
REL = 5e-4          # the whole-tensor bound of test_random_configuration_gradients_vs_oracle_autograd
TWICE = ("rows32", "rows33", HC.CHUNK_CASE)
FACTORS_TOO = ("mixed", "zerorows")


def _field(b):
    from text2nerf_amd import TensorVMSplit
    kw = HC.VIEW_HEAD if b["view"] else dict(shadingMode="MLP_Fea_noview", pos_pe=0, view_pe=0, fea_pe=6)
    m = TensorVMSplit(torch.tensor(b["aabb"], dtype=torch.float32), list(b["grid"]), dev(), density_n_comp=[16] * 3, appearance_n_comp=[48] * 3,
                      app_dim=27, near_far=b["near_far"], alphaMask_thres=1e-4, density_shift=-10, distance_scale=25, featureC=128,
                      step_ratio=1.0, fea2denseAct="softplus", **kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in b["params"].items()}, strict=True)
    return m


def _judge(name, route, got, ref, st=None, loss="fuzz"):
    """Print the observed ratios, then the element-wise check and the whole-tensor one."""
    obs = HE.ratios(got, ref)
    print(f"HEADEW {name} {route} K {ref.K():.2f} rho32 {ref.rho32:.3f} rows {ref.rows}" + (f" f16_redo {st['f16_redo']}" if st else "")
          + " observed " + " ".join(f"{HE.short(k)} {v:.3f}" for k, v in obs.items()))
    HE.check(got, ref, ref.K())
    _grad_check(got, HC.g64_all(name, loss), rel=REL)


def _grads(f):
    return {k: p.grad for k, p in f.named_parameters()}


def _autograd(name, route, runs=1, exact=False):
    b, ref = HC.built(name), HC.reference(name)
    f = _field(b)
    f.mlp_exact_fp32 = exact
    loss = HC.fuzz_loss({"cas": b["cas"].to(dev())})
    for run in range(runs):
        for p in f.parameters():
            p.grad = None
        torch.manual_seed(b["seed"])            # the forward draws the case's jitter from the CPU generator
        out = f(b["rays"], is_train=True, white_bg=True, N_samples=b["n_samples"])
        loss(*out).backward()
        close(out[2], ref.z, atol=0, msg=name)
        st = f.stats()
        assert st["evaluated"] == int(ref.valid.sum()) and st["appearance"] == ref.rows == b["target"], st
        _judge(name, f"{route} run {run}", _grads(f), ref, st)
        if name in FACTORS_TOO and not b["view"]:
            fref = HC.factor_reference(name)
            print(f"HEADEW {name} {route} factors K {fref.K():.2f} observed " + " ".join(f"{k} {v:.3f}" for k, v in GE.ratios(_grads(f), fref).items()))
            GE.check(_grads(f), fref, fref.K())
        if run == 0 and runs > 1:
            assert f._ctx_rows_hint >= 32       # the next forward keeps its activation rows


@pytest.mark.parametrize("name", HC.ROW_CASES + HC.RANGE_CASES + HC.WEIGHT_CASES)
def test_autograd_backward(name):
    _autograd(name, "autograd", runs=2 if name in TWICE else 1)


@pytest.mark.parametrize("name", ("rows0", "rows1", "rows33", "rows65", HC.CHUNK_CASE, "2^-40", "mixed"))
def test_exact_fp32_backward(name):
    _autograd(name, "fp32")


@pytest.mark.parametrize("name", HC.VIEW_CASES)
def test_view_dependent_head(name):
    _autograd(name, "mlp_fea")


@pytest.mark.parametrize("name", ("rows1", "rows33", "rows65", HC.CHUNK_CASE))
def test_composed_speculative_train_step(name):
    """train_step(speculative=True) with a stand-in optimiser, twice: the first step learns the capacity on the counted route, the
    second clips to the row count on the device. (train_step returns no z: the autograd route guards the geometry of the same rays.)"""
    b, ref = HC.built(name), HC.reference(name, "driver")
    f = _field(b)
    for step in range(2):
        torch.manual_seed(b["seed"])
        losses = f.train_step(b["rays"], b["rgb_t"], b["dep_t"], _NoStep(), N_samples=b["n_samples"], white_bg=True, speculative=True)
        losses = losses.cpu().numpy()
        st = f.stats()
        assert st["evaluated"] == int(ref.valid.sum()) and st["appearance"] == ref.rows, st
        np.testing.assert_allclose(losses[3], ref.loss, rtol=2e-5)
        assert getattr(f, "device_rows_steps", 0) == step and getattr(f, "device_rows_overflows", 0) == 0
        _judge(name, f"composed step {step}", _grads(f), ref, st, "driver")


@pytest.mark.parametrize("name", ("rows33", "rows257", HC.CHUNK_CASE))
def test_fused_train_step(name):
    """t2n_train_step in its two-phase form: the gradient of phase 1 read where an all-reduce would run (factor gradient buffer + the
    head tensors' .grad), before phase 2's Adam consumes it."""
    from text2nerf_amd.optim import TVAdam
    from text2nerf_amd.trainer import FusedStep, _ladder
    b, ref = HC.built(name), HC.reference(name, "driver")
    f = _field(b)
    opt = TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f)
    torch.manual_seed(b["seed"])
    with torch.no_grad():
        f(b["rays"], is_train=True, white_bg=True, N_samples=b["n_samples"])
    assert f.stats()["appearance"] == ref.rows
    fs = f.__dict__["_fused_step"] = FusedStep(f, opt)
    fs.rows_cap = _ladder(int(ref.rows * 1.25) + 4096)        # a capacity that holds the batch: nothing is withheld
    seen = {}

    def all_reduce():
        g = A.factor_grads_ref(f)
        for k, p in A.kernel_named(f)[12:]:
            g[k] = p.grad.detach().cpu().numpy().astype(np.float64)
        seen["g"], seen["vote"] = g, float(fs.head_grads[-1])

    torch.manual_seed(b["seed"])
    f.train_step(b["rays"], b["rgb_t"], b["dep_t"], opt, N_samples=b["n_samples"], white_bg=True, fused=True, all_reduce=all_reduce)
    fs.sync()
    assert seen and seen["vote"] == 0.0 and fs.replays == 0
    np.testing.assert_allclose(fs.losses.cpu().numpy()[3], ref.loss, rtol=2e-5)
    _judge(name, "fused step", seen["g"], ref, None, "driver")
