"""The coverage claim of tests/test_generic_fuzz.py, checked without a GPU: tests/helpers/generic_cases.py::form_of restates how
csrc/t2n_generic.hip picks its kernel form from a field's shape; here the directed cases and the fuzz seeds together must reach every
form, every directed case must land on the forms it declares, every case must construct as a general-shape field inside the path's
limits, find a ReLU-safe parameter seed within eight steps, and the two large cases must put the oracle's appearance count where the
multi-pass head needs it."""
import pytest
import torch

from tests.helpers import generic_cases as G

CASES = [c.name for c in G.all_cases()]


def _count(case):
    """The float32 oracle's appearance-list length of the pass a large case's tags speak of."""
    with torch.no_grad():
        (_, _, _, w), _ = G.oracle(case, G.make_params(case, case.seed0), case.count_mode, dtype=torch.float32)
    return int((w > 1e-4).sum())


def _tags(case, count=None):
    N = case.n_train if case.n_eval < 0 else max(case.n_train, case.n_eval)
    return G.form_of(case.kw, case.R, N, count=count, ndc=case.ndc, mask=case.mask)


@pytest.fixture(scope="module")
def large_counts():
    return {name: _count(G.DIRECTED[name]) for name in ("two_pass", "pass_boundary")}


def test_form_of_mirrors_the_selection_arithmetic():
    kw = dict(G.DIRECTED["plain"].kw)
    assert G.head_lds_bytes(kw) == 41728 * 4 > G.LDS_LIMIT and G.form_of(kw, 99, 19) == {"fwd_plain"}
    kw["appearance_n_comp"] = [112, 104, 88]            # 304 columns: 40 960 floats, the staged forward's last shape
    assert G.head_lds_bytes(kw) == G.LDS_LIMIT and "fwd_staged" in G.form_of(kw, 99, 19)
    assert G.in0_of(G.DIRECTED["limits"].kw) == 2211 and G.in0_of(G.DIRECTED["valu_in520"].kw) == 520
    assert G.in0_of(G.DIRECTED["mlp_view"].kw) == 24 + 3 + 6 * 4          # the MLP head ignores fea_pe
    k512 = dict(G.DIRECTED["valu_in520"].kw, app_dim=32, fea_pe=6, view_pe=16, shadingMode="MLP_Fea")     # 32 * 13 + 3 + 96 = 515
    assert G.in0_of(k512) == 515 and "head_valu_mlp" in G.form_of(k512, 10, 10)
    k512["view_pe"] = 15                                                   # 509 inputs
    assert G.form_of(k512, 10, 10) >= {"head_rows32", "out_scalar"}
    assert "multipass" not in G.form_of(G.DIRECTED["two_pass"].kw, 16384, 12) and "multipass" in G.form_of(G.DIRECTED["two_pass"].kw, 21846, 12)


def test_every_form_is_reached(large_counts):
    reached = set()
    for case in G.all_cases():
        reached |= _tags(case, large_counts.get(case.name))
    assert reached >= G.ALL_TAGS, sorted(G.ALL_TAGS - reached)
    assert reached <= G.ALL_TAGS | G.EXTRA_TAGS
    assert len(G.FUZZ_SEEDS) >= 16
    fuzz = [G.fuzz_case(s) for s in G.FUZZ_SEEDS]
    assert sum(c.mask or c.ndc for c in fuzz) * 3 >= len(fuzz) and any(c.mask and c.ndc for c in fuzz)
    assert {c.kw["shadingMode"] for c in fuzz} >= {"MLP_Fea_noview", "MLP_Fea", "MLP", "SH"}
    assert any(c.grad_train for c in fuzz) and any(not c.grad_train for c in fuzz)
    assert any(c.white_train for c in fuzz) and any(not c.white_train for c in fuzz)


@pytest.mark.parametrize("name", list(G.DIRECTED))
def test_directed_case_lands_on_its_declared_forms(name, large_counts):
    case = G.DIRECTED[name]
    assert _tags(case, large_counts.get(name)) == set(case.tags)


def test_large_cases_place_the_oracle_count(large_counts):
    """two_pass: more than 262 144 + 64 list entries, so pass 2 has at least one full tile; pass_boundary: pass 1's last tile is
    partial and pass 2 is empty. The kernels' count may differ from the oracle's by the +-2 the suite allows: both windows keep
    more than that on either side."""
    assert large_counts["two_pass"] > G.PASS_ROWS + 64
    assert G.PASS_ROWS - 64 + 8 <= large_counts["pass_boundary"] <= G.PASS_ROWS - 8
    for name in large_counts:
        case = G.DIRECTED[name]
        assert case.R * case.n_train > G.PASS_ROWS and (case.R // 2 + 1) * case.n_train <= G.PASS_ROWS      # the halves are single-pass


@pytest.mark.parametrize("name", CASES)
def test_case_constructs_as_a_general_field_inside_the_limits(name):
    case = G.case_by_name(name)
    assert G.inside_limits(case.kw)
    assert case.R % 4 and case.R % 64 or case.large
    assert 5 <= case.n_train <= 90
    m = G.make_field(case, G.make_params(case, case.seed0), "cpu")
    assert m._is_general() and not m._needs_embed()
    if case.kw["shadingMode"] in G.MLP_HEADS:
        assert m.renderModule.mlp[0].weight.shape == (case.kw["featureC"], G.in0_of(case.kw))
    if case.n_eval < 0:
        assert m.nSamples == G.make_cfg(case).n_samples


@pytest.mark.parametrize("name", [c.name for c in G.all_cases() if not c.large])
def test_case_finds_a_relu_safe_seed(name):
    seed, steps, margin, idx = G.relu_safe_seed(name)
    case = G.case_by_name(name)
    assert steps < G.SEED_STEPS and margin >= G.RELU_MARGIN and 4 <= len(idx) <= case.R
    if case.mask:       # the mask of the chosen seed does remove voxels, and keeps some
        assert 0.02 < float(G.mask_volume(case, G.make_params(case, seed)).mean()) <= 0.9
