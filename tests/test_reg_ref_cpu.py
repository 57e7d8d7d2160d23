"""tests/helpers/reg_ref.py on the CPU: its float64 L1 / ortho references pinned to the reference's own autograd
(tests/golden/reg_terms.npz, written by tests/golden/make_golden_reg.py in float32 and float64); the case tables of the GPU tests free of
sign-ambiguous pairs; the constructed disjoint-support case; a float32 emulation of the kernels' arithmetic accepted by the per-element
checkers, and five wrong kernels (normaliser C^2, no factor 2, sign(0) = 1, numel of another tensor, the diagonal included) caught."""
import os

import numpy as np
import pytest

from text2nerf_amd import synth
from tests.conftest import TINY
from tests.helpers import reg_ref as R

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "reg_terms.npz"))
GRID, VM_GRID = [23, 19, 17], [17, 17, 17]
SEEDS = dict(split=61, general=62, vm=63, cp=64)
GENERAL = dict(density_n_comp=[5, 3, 4], app_n_comp=[7, 6, 2])


def params(model):
    if model == "general":
        return synth.make_field_params(SEEDS[model], GRID, density_scale=0.9, aabb=TINY["aabb"], **GENERAL)
    return synth.make_field_params(SEEDS[model], VM_GRID if model == "vm" else GRID, density_scale=0.9, aabb=TINY["aabb"])


def f32_band_slack(M):
    """What a float32 Gram matrix (the f32 golden's) may add to an ortho gradient element by taking another sign for a pair inside ITS
    band, |D_ij| <= n 2^-22 |m_i| |m_j|: twice the pair's term."""
    M = R.as_matrix(M)
    C, n = M.shape
    D = M @ M.T
    norm = np.sqrt((M * M).sum(1))
    inside = np.abs(D) <= n * 2.0 ** -22 * norm[:, None] * norm[None, :]
    np.fill_diagonal(inside, False)
    return 2.0 * 2.0 / (C * (C - 1)) * (inside.astype(np.float64) @ np.abs(M))


@pytest.mark.parametrize("model", ["split", "general", "cp"])
def test_l1_reference_against_the_goldens(model):
    sd = params(model)
    keys = [f"density_{kind}.{k}" for k in range(3) for kind in (("line",) if model == "cp" else ("plane", "line"))]
    v = R.l1_value([sd[k] for k in keys])
    assert abs(v - float(GOLD[f"{model}/f64/density_L1"])) <= 1e-13 * v
    assert abs(v - float(GOLD[f"{model}/f32/density_L1"])) <= 1e-5 * v
    for k in keys:
        g = R.l1_grad(sd[k], 1.0)
        g64 = GOLD[f"{model}/f64/density_L1/grad/{k}"]
        assert np.all(np.abs(g - g64) <= R.U * np.abs(g64)), k           # the constant's one float32 rounding
        assert np.array_equal(g.astype(np.float32), GOLD[f"{model}/f32/density_L1/grad/{k}"]), k
        assert np.any(g64 > 0) and np.any(g64 < 0)


@pytest.mark.parametrize("model", ["split", "general", "vm"])
def test_ortho_reference_against_the_goldens(model):
    sd = params(model)
    if model == "vm":       # line_coef [3, 48 + 16, res, 1]: appearance components first, density components last
        g64s, g32s = GOLD["vm/f64/vector_comp_diffs/grad/line_coef"], GOLD["vm/f32/vector_comp_diffs/grad/line_coef"]
        lines = [(sd[f"density_line.{k}"], g64s[k, 48:], g32s[k, 48:]) for k in range(3)] + \
                [(sd[f"app_line.{k}"], g64s[k, :48], g32s[k, :48]) for k in range(3)]
    else:
        names = [f"{grp}_line.{k}" for grp in ("density", "app") for k in range(3)]
        lines = [(sd[k], GOLD[f"{model}/f64/vector_comp_diffs/grad/{k}"], GOLD[f"{model}/f32/vector_comp_diffs/grad/{k}"]) for k in names]
    v = sum(R.ortho_value(M) for M, _, _ in lines)
    assert abs(v - float(GOLD[f"{model}/f64/vector_comp_diffs"])) <= 1e-12 * v
    assert abs(v - float(GOLD[f"{model}/f32/vector_comp_diffs"])) <= 1e-5 * v
    for i, (M, g64, g32) in enumerate(lines):
        assert len(R.ambiguous_pairs(M)) == 0, i
        g = R.ortho_grad(M)
        scale = np.abs(R.as_matrix(M)).sum(0)[None, :] * 2.0 / (M.shape[1] * (M.shape[1] - 1))
        assert np.all(np.abs(g - R.as_matrix(g64)) <= 1e-13 * scale), i
        # the reference in float32: the checker's bound, plus the pairs whose sign a float32 Gram matrix may take differently
        err = np.abs(g - R.as_matrix(g32))
        assert np.all(err <= R.ortho_grad_tolerance(M) + f32_band_slack(M)), (i, float(err.max()))
        assert float(np.abs(g).max()) > 0


def test_case_tables_hold_no_ambiguous_pair():
    cases = R.ortho_cases()
    assert len(cases) == len(R.ORTHO_C) * len(R.ORTHO_N) + 1
    for name, line in cases.items():
        assert len(R.ambiguous_pairs(line)) == 0, name
        assert np.isfinite(R.ortho_value(line)), name
    for shape in R.L1_SHAPES:
        x = R.l1_plane(shape)
        bits = x.view(np.uint32).reshape(-1)
        assert (bits == 0).any() and (bits == 0x80000000).any(), shape                       # +0.0 and -0.0
        den = (bits & 0x7F800000 == 0) & (bits & 0x007FFFFF != 0)
        assert (den & (bits >> 31 == 0)).any() and (den & (bits >> 31 == 1)).any(), shape        # denormals of both signs
        g = R.l1_grad(x, R.L1_WEIGHT)
        assert not g[x == 0].any() and np.all(g[den.reshape(x.shape)] != 0), shape


def test_disjoint_support_pairs_contribute_exactly_nothing():
    line = R.disjoint_line()
    M = R.as_matrix(line)
    D, S = R.gram(line), R.ortho_sign(line)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert D[i, j] == 0.0 and D[j, i] == 0.0 and S[i, j] == 0.0
    assert np.abs(S[3:, :]).sum() == 3 * 5            # the dense rows see every other row
    g = R.ortho_grad(line)
    # row 0's gradient is made of rows 3-5 alone
    want = 2.0 / 30.0 * (S[0, 3:, None] * M[3:]).sum(0)
    assert np.array_equal(g[0], want)


# ---- the checkers: a faithful float32 emulation passes, five wrong kernels do not ------------------------------------------------------
emulate_ortho = R.kernel_model_ortho


CHECK_CASES = ["2x1", "3x17", "16x65", "20x64", "48x63", "disjoint"]


@pytest.mark.parametrize("name", CHECK_CASES)
def test_checkers_accept_the_kernel_arithmetic(name):
    line = R.ortho_cases()[name]
    assert not R.check_ortho_grad(emulate_ortho(line, R.ORTHO_WEIGHT), line, R.ORTHO_WEIGHT)
    assert not R.check_ortho_grad(emulate_ortho(line, R.ORTHO_WEIGHT, R.UPSTREAM), line, R.ORTHO_WEIGHT, R.UPSTREAM)
    prev = (np.random.default_rng(3).standard_normal(R.as_matrix(line).shape) * 1e-3).astype(np.float32)
    added = (prev + emulate_ortho(line, R.ORTHO_WEIGHT)).astype(np.float32)
    assert not R.check_ortho_grad(added, line, R.ORTHO_WEIGHT, prev=prev)
    for shape in R.L1_SHAPES:
        x = R.l1_plane(shape)
        s = np.float32(np.float64(np.float32(R.L1_WEIGHT)) / x.size)
        assert not R.check_l1_set((s * R.sign0(x)).astype(np.float32), x, R.L1_WEIGHT)
        su = np.float32(s * np.float32(R.UPSTREAM))
        assert not R.check_l1_set((su * R.sign0(x)).astype(np.float32), x, R.L1_WEIGHT, R.UPSTREAM)


@pytest.mark.parametrize("name", CHECK_CASES)
def test_checker_catches_wrong_ortho_kernels(name):
    line = R.ortho_cases()[name]
    C = R.as_matrix(line).shape[0]
    assert R.check_ortho_grad(emulate_ortho(line, R.ORTHO_WEIGHT, normaliser=C * C), line, R.ORTHO_WEIGHT), "normaliser C^2"
    assert R.check_ortho_grad(emulate_ortho(line, R.ORTHO_WEIGHT, factor=1.0), line, R.ORTHO_WEIGHT), "missing factor 2"
    assert R.check_ortho_grad(emulate_ortho(line, R.ORTHO_WEIGHT, diagonal=True), line, R.ORTHO_WEIGHT), "diagonal included"
    if name == "disjoint":
        assert R.check_ortho_grad(emulate_ortho(line, R.ORTHO_WEIGHT, sign_of_zero=1.0), line, R.ORTHO_WEIGHT), "sign(0) = 1"


@pytest.mark.parametrize("shape", R.L1_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_checker_catches_wrong_l1_kernels(shape):
    x = R.l1_plane(shape)
    s = np.float32(np.float64(np.float32(R.L1_WEIGHT)) / x.size)
    sign_one = np.where(x == 0, 1.0, R.sign0(x))
    assert R.check_l1_set((s * sign_one).astype(np.float32), x, R.L1_WEIGHT), "sign(0) = 1"
    flushed = np.where(np.abs(x) < np.finfo(np.float32).tiny, 0.0, R.sign0(x))
    assert R.check_l1_set((s * flushed).astype(np.float32), x, R.L1_WEIGHT), "denormals flushed"
    other = np.float32(np.float64(np.float32(R.L1_WEIGHT)) / (x.size // x.shape[1]))      # the numel of one channel: another tensor's
    assert R.check_l1_set((other * R.sign0(x)).astype(np.float32), x, R.L1_WEIGHT), "numel of the wrong tensor"
    prev = np.ones(x.shape, np.float32)
    assert R.check_l1_add((prev + other * R.sign0(x)).astype(np.float32), prev, x, R.L1_WEIGHT), "numel of the wrong tensor (add)"
