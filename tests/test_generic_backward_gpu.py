"""The general-shape backward as kernels (csrc/t2n_generic_bwd.hip) through the autograd surface: gradients of the driver's loss on whole
frames in train mode against the float64 oracle (tests/helpers/generic_train.py::reference_step; tests/test_generic_backward_cpu.py
shows the float32 oracle within 5e-4 / 16 of it on every case used here), at the project's general-path bound of 5e-4. The head's passes
over the appearance list at two pass sizes, the shapes that keep the plain backward, and the empty frame."""
import pytest

from tests.helpers import generic_cases as G
from tests.helpers import generic_train as T
from tests.test_generic_fuzz import _render
from tests.test_hip_parity import _grad_check, dev

pytestmark = pytest.mark.gpu

REL = 5e-4


def _field(name):
    case, params, vol = T.case_inputs(name)
    m = G.make_field(case, params, dev(), vol)
    assert m._is_general()
    return case, m


def _backward(case, m, monkeypatch):
    """The driver's loss of a whole train-mode frame, differentiated through the module call; returns the loss terms."""
    rgb_t, dep_t = (t.to(dev()) for t in T.targets(case))
    for p in m.parameters():
        p.grad = None
    rgb, depth, z, w = _render(case, m, True, monkeypatch)
    terms = T.driver_loss_torch(rgb, depth, w, z, rgb_t, dep_t)
    terms[3].backward()
    return terms


def _check(name, m, tag=""):
    ref = T.reference_step(name)["grads"]
    try:
        _grad_check(m, ref, rel=REL)
    finally:
        worst = _grad_check.last["max_rel"]
        k = max(worst, key=worst.get)
        print(f"generic_backward {name:12s} {tag:14s} worst max|dg|/max|g| {worst[k]:.1e} ({k})")


@pytest.mark.parametrize("name", T.GRAD_CASES)
def test_kernel_backward_vs_float64_oracle(name, monkeypatch):
    case, m = _field(name)
    plan = m.general_backward_plan(case.R, case.n_train)
    assert plan["kernel_form"] == 1 and plan["workspace_bytes"] > 0, plan
    _backward(case, m, monkeypatch)
    _check(name, m)


@pytest.mark.parametrize("pass_rows", [1024, 64])
@pytest.mark.parametrize("name", ["odd_rows", "rows64"])
def test_head_passes(name, pass_rows, monkeypatch):
    """Lists of ~2 849 / ~2 926 entries in passes of 1 024 (three with work, the last ending in a partial 64-row tile) and of 64 (about
    45 with work): a row lost or doubled at a pass edge is ~1 / 2 850 of a sum at the first setting and ~45 / 2 850 at the second."""
    case, m = _field(name)
    m.general_backward_pass_rows = pass_rows
    plan = m.general_backward_plan(case.R, case.n_train)
    assert plan["kernel_form"] == 1 and plan["pass_rows"] == pass_rows and plan["max_passes"] > 1, plan
    assert plan["max_passes"] == -(-case.R * case.n_train // pass_rows)
    _backward(case, m, monkeypatch)
    count = m.stats()["appearance"]
    assert count > 2 * 1024 and count % 64 != 0, count           # three passes of 1 024 have work, the last tile is partial
    _check(name, m, f"pass_rows {pass_rows}")


@pytest.mark.parametrize("name", T.FALLBACK_CASES)
def test_shapes_that_keep_the_plain_backward(name, monkeypatch):
    case, m = _field(name)
    plan = m.general_backward_plan(case.R, case.n_train)
    assert plan["kernel_form"] == 0 and plan["workspace_bytes"] == 0, plan
    _backward(case, m, monkeypatch)
    _check(name, m, "plain")


def test_empty_frame_has_exactly_zero_gradients(monkeypatch):
    case, m = _field("empty")
    assert m.general_backward_plan(case.R, case.n_train)["kernel_form"] == 1
    _backward(case, m, monkeypatch)
    assert m.stats()["appearance"] == 0
    for k, p in m.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0, k
