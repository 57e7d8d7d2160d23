"""CPU side of the general-shape backward's tests (csrc/t2n_generic_bwd.hip): the Python restatement of t2n_generic_backward_plan
against the C function over every directed case and fuzz seed, the claim that those cases reach every row of the form table, the
reference step of tests/helpers/generic_train.py against an independent torch.autograd evaluation, and the condition that lets the GPU
tests compare whole frames: the float32 oracle's gradients of the driver's loss sit far inside the 5e-4 bound of the float64 ones."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import generic_cases as G
from tests.helpers import generic_train as T

REL = 5e-4                      # the project's general-path gradient bound (tests/test_generic_fuzz.py: _grad_check(rel=5e-4))


def _desc(case):
    from text2nerf_amd import _lib
    d = _lib.GenericDesc()
    kw = case.kw
    for k in range(3):
        d.grid[k] = int(case.grid[k])
        d.density_n_comp[k], d.app_n_comp[k] = int(kw["density_n_comp"][k]), int(kw["appearance_n_comp"][k])
    d.app_dim, d.shading = int(kw["app_dim"]), _lib.SHADE_IDS[kw["shadingMode"]]
    d.fea_pe, d.view_pe, d.feature_c = int(kw["fea_pe"]), int(kw["view_pe"]), int(kw["featureC"])
    return d


@pytest.mark.parametrize("pass_rows", [0, 64, 1000])
def test_plan_restatement_equals_the_c_plan(pass_rows):
    from text2nerf_amd import _lib
    lib = _lib.load()
    for case in G.all_cases():
        plan = _lib.GenericBwdPlan()
        d = _desc(case)
        _lib.check(lib.t2n_generic_backward_plan(C.byref(d), case.R, case.n_train, pass_rows, C.byref(plan)), "t2n_generic_backward_plan")
        got = dict(kernel_form=int(plan.kernel_form), pass_rows=int(plan.pass_rows), max_passes=int(plan.max_passes),
                   workspace_bytes=int(plan.workspace_bytes))
        want = T.backward_plan(case.kw, case.grid, case.R, case.n_train, pass_rows)
        assert got == want, (case.name, pass_rows, got, want)
        assert got["pass_rows"] % 64 == 0 and got["max_passes"] == -(-case.R * case.n_train // got["pass_rows"])
        if pass_rows == 1000 and case.R * case.n_train >= 1024:
            assert got["pass_rows"] == 1024
        assert (got["workspace_bytes"] > 0) == bool(got["kernel_form"])


def test_plan_rejects_bad_arguments():
    from text2nerf_amd import _lib
    lib = _lib.load()
    plan = _lib.GenericBwdPlan()
    d = _desc(G.DIRECTED["odd_rows"])
    assert lib.t2n_generic_backward_plan(C.byref(d), 0, 29, 0, C.byref(plan)) == -1
    assert lib.t2n_generic_backward_plan(C.byref(d), 221, 0, 0, C.byref(plan)) == -1
    assert lib.t2n_generic_backward_plan(None, 221, 29, 0, C.byref(plan)) == -1
    assert lib.t2n_generic_backward_plan(C.byref(d), 221, 29, 0, None) == -1


def test_cases_reach_every_row_of_the_form_table():
    rows = set()
    for case in G.all_cases():
        kw = case.kw
        if T.kernel_form(kw):
            tags = G.form_of(kw, case.R, case.n_train, ndc=case.ndc, mask=case.mask)
            rows |= {f"kernel:{t}" for t in tags & {"head_rows32", "head_rows64", "head_sh", "head_rgb", "mask", "ndc"}}
        elif G.head_lds_bytes(kw) > G.LDS_LIMIT:
            rows.add("plain:lds")
        else:
            assert G.in0_of(kw) > G.ROWS_IN_MAX, case.name
            rows.add("plain:inputs")
    assert rows == {"kernel:head_rows32", "kernel:head_rows64", "kernel:head_sh", "kernel:head_rgb", "kernel:mask", "kernel:ndc",
                    "plain:lds", "plain:inputs"}, rows
    # the cases the GPU tests name sit where the tests say they do
    for name in T.GRAD_CASES:
        assert T.kernel_form(G.case_by_name(name).kw) == 1, name
    for name in T.FALLBACK_CASES:
        assert T.kernel_form(G.case_by_name(name).kw) == 0, name
    assert G.head_lds_bytes(G.DIRECTED["plain"].kw) > G.LDS_LIMIT
    assert all(G.in0_of(G.case_by_name(n).kw) > G.ROWS_IN_MAX for n in ("valu_in520", "fuzz8"))
    assert G.case_by_name("fuzz11").mask and G.case_by_name("fuzz5").ndc and G.case_by_name("fuzz17").mask and G.case_by_name("fuzz17").ndc


def test_reference_step_equals_torch_autograd_with_tvloss():
    """generic_train.reference_step on tiny_head against an independent evaluation: the float64 oracle, the loss from the project's loss
    modules (losses.TransMittanceLoss_mask, losses.TVLoss) and torch.autograd.grad."""
    from text2nerf_amd.losses import TransMittanceLoss_mask, TVLoss
    ref = T.reference_step("tiny_head", tv_weights=T.TV_WEIGHTS)
    case, params, vol = T.case_inputs("tiny_head")
    (rgb, depth, z, w), P = G.oracle(case, params, True, vol=vol, requires_grad=True)
    rgb_t, dep_t = (t.double() for t in T.targets(case))
    z = z.double()
    loss = torch.mean((rgb - rgb_t) ** 2) + T.W_DEPTH * torch.mean((depth - dep_t) ** 2) \
        + T.W_TRANS * TransMittanceLoss_mask()(w, (z - dep_t[:, None] + T.DELTA) < 0)
    reg = TVLoss(1.0)
    loss = loss + sum(reg(P[f"density_plane.{k}"]) * 1e-2 for k in range(3)) * T.TV_WEIGHTS[0] \
        + sum(reg(P[f"app_plane.{k}"]) * 1e-2 for k in range(3)) * T.TV_WEIGHTS[1]
    keys = list(P)
    grads = torch.autograd.grad(loss, [P[k] for k in keys], allow_unused=True)
    got = {k: (np.zeros_like(ref["grads"][k]) if g is None else g.numpy()) for k, g in zip(keys, grads)}
    worst = T.max_rel(got, ref["grads"])
    assert max(worst.values()) <= 1e-12, worst
    assert any(float(np.abs(g).max()) > 0 for g in ref["grads"].values())


@pytest.mark.parametrize("name", sorted(set(T.GRAD_CASES + T.FALLBACK_CASES + T.STEP_CASES)))
def test_float32_oracle_gradients_sit_far_inside_the_bound(name):
    """Whole frame, train mode, the driver's loss: max |g32 - g64| / max |g64| <= 5e-4 / 16 for every tensor. Without this margin a GPU
    comparison at 5e-4 would need ReLU-safe seeds and ray subsets, as the grad_loss comparisons of tests/test_generic_fuzz.py do."""
    r64 = T.reference_step(name)
    r32 = T.reference_step(name, dtype=torch.float32)
    worst = T.max_rel(r32["grads"], r64["grads"])
    k = max(worst, key=worst.get)
    print(f"generic_backward {name:12s} oracle32 vs oracle64: worst max|dg|/max|g| {worst[k]:.1e} ({k})")
    assert worst[k] <= REL / 16, worst
