"""The element-wise head-gradient check without a kernel (helper: tests/helpers/head_grad_elementwise.py, cases:
tests/helpers/head_grad_cases.py): the claims of the cases (exact row counts, an empty knife window, the restated tn_plan, the
constants found once in the sources), the restated head pinned to oracle_torch's gradients bit for bit, the float32 oracle within its
own bound for every case, and mutation tests that show what the checker catches — on the float32 oracle's gradients, so nothing here
needs a GPU."""
import numpy as np
import pytest

from tests.helpers import grad_elementwise as GE
from tests.helpers import head_grad_cases as HC
from tests.helpers import head_grad_elementwise as HE
from tests.test_hip_parity import _grad_check

NOVIEW = HC.ROW_CASES + HC.RANGE_CASES + HC.WEIGHT_CASES
DRIVER = ("rows1", "rows33", "rows65", "rows257", HC.CHUNK_CASE)
REL = 5e-4


@pytest.fixture(scope="module")
def consts():
    return HC.kernel_constants()


def test_constants_and_tn_plan_restatement(consts):
    assert consts == dict(step=16, tile=32, waves=8, l2=64, min_chunk=64, chunk_round=32, blocks=512), \
        "the row targets aim at these edges of the head backward: choose them anew"
    assert HC.row_targets(consts) == [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 10923]
    T = HC.chunk_target(consts)
    assert HC.tn_plan(T, 351, consts) == (96, (T + 95) // 96, 3) and HC.tn_plan(T - 1, 351, consts)[0] == 64
    assert HC.tn_plan(T, 128, consts) == (64, (T + 63) // 64, 1) and HC.tn_plan(T, 144, consts)[0] == 64
    for N in (351, 128, 144):
        c = HC.tn_plan(T, N, consts)[0]
        assert T % c != 0 and (T % c) % consts["step"] != 0
    assert 0 < T - 64 * 512 / 3 < 16                 # "a little over 10 922"
    # spot values of the C function (csrc/t2n_bwd_mlp.hip): the minimum chunk, the 32-row rounding, one chunk at least
    assert HC.tn_plan(0, 128, consts) == (64, 1, 1) and HC.tn_plan(1, 351, consts) == (64, 1, 3) and HC.tn_plan(65, 144, consts) == (64, 2, 2)
    assert HC.tn_plan(100000, 351, consts) == (608, 165, 3) and HC.tn_plan(1 << 20, 128, consts) == (2048, 512, 1)


@pytest.mark.parametrize("name", HC.ROW_CASES + (HC.RANGE_ROWS,))
def test_row_cases_have_their_count_exactly(name):
    b, ref = HC.built(name), HC.reference(name)
    assert ref.rows == b["target"] == int(name[4:])
    assert int(ref.app_window.sum()) == 0                       # no sample a kernel may list differently
    assert b["rays"].shape == (HC.R_FIX, 6) and int(ref.valid.sum()) > 0
    for r in (ref.rows64, ref.rows32):
        assert all(v.shape[0] == ref.rows for v in r.values())
    if ref.rows == 0:
        assert all(not ref.g64[k].any() and not ref.g32[k].any() and not ref.A[k].any() for k in HE.HEAD_KEYS)


@pytest.mark.parametrize("name", ("rows1", "rows33", "mixed", "outliers", "view_rows33", "view_mixed"))
def test_restated_head_equals_the_oracle_bit_for_bit(name):
    ref = HC.reference(name)
    for k in HE.HEAD_KEYS:
        assert np.array_equal(ref.head64[k], ref.g64[k]), k
    r = ref.rows64
    sums = HE._sums(dict(go=r["go"], g1=r["g1"], g0=r["g0"], gf=r["gf"]), dict(h1=r["h1"], h0=r["h0"], x=r["x"], x144=r["x144"]))
    for k in HE.HEAD_KEYS:          # the per-row quantities are the ones the gradients are sums of
        np.testing.assert_allclose(sums[k], ref.g64[k], rtol=0, atol=1e-12 * max(1e-300, float(ref.A[k].max())))


@pytest.mark.parametrize("name", NOVIEW + HC.VIEW_CASES)
def test_reference_stays_within_its_own_bound(name):
    ref = HC.reference(name)
    print(HC.table_line(name))
    assert np.isfinite(ref.rho32) and ref.K() == 8 * max(1.0, ref.rho32)
    for k in HE.HEAD_KEYS:
        A, g = ref.A[k], ref.g64[k]
        assert np.all(A * (1 + 1e-12) >= np.abs(g)), k
        assert np.all(g[A == 0] == 0) and np.all(ref.g32[k][A == 0] == 0), k
        assert np.all(np.isfinite(ref.bound[k])) and np.all(ref.bound[k][A > 0] > 0), k
    HE.check(ref.g32, ref, ref.K())
    HE.check(ref.g32, ref, 2 * max(1.0, ref.rho32))


@pytest.mark.parametrize("name", DRIVER)
def test_reference_under_the_driver_loss(name):
    ref = HC.reference(name, "driver")
    print(HC.table_line(name, "driver"))
    assert ref.rows == int(name[4:]) and int(ref.app_window.sum()) == 0
    HE.check(ref.g32, ref, ref.K())


@pytest.mark.parametrize("name", ("2^-40", "2^+40", "view_2^-40"))
def test_uniform_power_of_two_scales_the_reference_exactly(name):
    """The float64 reference is linear in a uniform power of two: the case computed on its own equals the s = 1 reference scaled, bound
    included, bit for bit."""
    a, b = HC.reference(name), HC.reference(name, direct=True)
    for k in HE.HEAD_KEYS:
        assert np.array_equal(a.g64[k], b.g64[k]) and np.array_equal(a.g32[k], b.g32[k]), k
        assert np.array_equal(a.A[k], b.A[k]) and np.array_equal(a.bound[k], b.bound[k]), k
    assert a.rho32 == b.rho32


@pytest.mark.parametrize("name", HC.RANGE_CASES + tuple(n for n in HC.VIEW_CASES if not n.startswith("view_rows")))
def test_range_cases_stay_normal_in_float32(name):
    ref = HC.reference(name)
    tiny, huge = float(np.finfo(np.float32).tiny), float(np.finfo(np.float32).max)
    for k in HE.HEAD_KEYS:
        g = np.abs(ref.g64[k][ref.g64[k] != 0])
        assert g.size and g.min() >= tiny and g.max() <= huge, (k, g.min(), g.max())
    for q in ("go", "g1", "g0", "gf"):
        v = np.abs(ref.rows64[q])
        assert v.max() <= huge and (v[v != 0].min() >= tiny), q
    b = HC.built(name)
    if name.endswith("zerorows"):
        dead = ~np.abs(ref.rows64["go"]).any(1)
        assert 0.2 < dead.mean() < 0.5                      # whole zero rows beside live ones
    if name.endswith("mixed"):
        k = np.log2(b["s"])
        assert k.min() == -40 and k.max() == 20 and np.all(k == np.round(k))
    if name == "red":
        assert not ref.rows64["go"][:, 1:].any() and not ref.A[HE.W2][1:].any() and ref.A[HE.W2][0].any()


@pytest.mark.parametrize("name", ("mixed", "zerorows"))
def test_factor_reference_of_the_range_cases(name):
    fref = HC.factor_reference(name)
    GE.check(fref.g32, fref, fref.K())
    assert int(fref.app_mask.sum()) == HC.reference(name).rows


# ---- mutations of the float32 oracle's gradient: each must be flagged at the GPU tests' K -------------------------------------------------
def _row(rows, r, **replace_):
    """What row r adds to the seven tensors, from per-row quantities (optionally with some replaced for that row)."""
    q = {k: replace_.get(k, v[r]) for k, v in rows.items()}
    return {HE.W2: np.outer(q["go"], q["h1"]), HE.B2: q["go"], HE.W1: np.outer(q["g1"], q["h0"]), HE.B1: q["g1"],
            HE.W0: np.outer(q["g0"], q["x"]), HE.B0: q["g0"], HE.BASIS: np.outer(q["gf"], q["x144"])}


def _plus(ref, delta, keys=HE.HEAD_KEYS):
    got = {k: v.copy() for k, v in ref.g32.items()}
    for k in keys:
        got[k] = got[k] + delta[k]
    return got


def _caught(got, ref, keys=None, whole_tensor_passes=None):
    lines = HE.failures(got, ref, ref.K())
    assert lines, "the mutation passed the element-wise check"
    if keys is not None:
        assert {l.split(":")[0] for l in lines} <= set(keys), lines
    if whole_tensor_passes is not None:
        try:
            _grad_check(got, ref.g64, rel=REL)
            passed = True
        except AssertionError:
            passed = False
        assert passed == whole_tensor_passes, _grad_check.last["max_rel"]
    print(lines)
    with pytest.raises(AssertionError, match="element-wise"):
        HE.check(got, ref, ref.K())


def _chunk_rows(key, T):
    return HC.tn_plan(T, {HE.W0: 351, HE.B0: 351, HE.W1: 128, HE.B1: 128, HE.BASIS: 144}[key])[0]


def test_mutation_last_row_of_a_chunk_dropped():
    """What a chunk loop that stops one row early does: the last row of every full chunk missing from that GEMM's tensor."""
    ref = HC.reference(HC.CHUNK_CASE)
    keys = (HE.W0, HE.W1, HE.BASIS)
    got = {k: v.copy() for k, v in ref.g32.items()}
    for k in keys:
        c = _chunk_rows(k, ref.rows)
        for r in range(c - 1, ref.rows, c):
            got[k] = got[k] - _row(ref.rows32, r)[k]
    _caught(got, ref, keys)


def test_mutation_one_row_counted_twice():
    ref = HC.reference(HC.CHUNK_CASE)
    r = int(np.abs(ref.rows32["go"]).sum(1).argmax())
    _caught(_plus(ref, _row(ref.rows32, r)), ref)


def test_mutation_one_row_from_the_f16_hi_part_only():
    """One row's gradient vectors rounded to f16 relative to the row's largest (2^-11 relative on that row)."""
    ref = HC.reference("rows17")
    r = int(np.abs(ref.rows32["go"]).sum(1).argmax())

    def hi(v):
        s = 2.0 ** np.floor(np.log2(np.abs(v).max()))
        return (v / s).astype(np.float16).astype(np.float64) * s
    full, part = _row(ref.rows32, r), _row(ref.rows32, r, **{q: hi(ref.rows32[q][r]) for q in ("go", "g1", "g0", "gf")})
    _caught(_plus(ref, {k: part[k] - full[k] for k in full}), ref, whole_tensor_passes=True)


def test_mutation_relu_mask_shifted_by_one_unit_on_one_row():
    ref = HC.reference("rows257")
    r = 100
    g1 = np.roll(ref.rows32["g1"][r] != 0, 1) * (ref.rows32["go"][r] @ HC.built("rows257")["params"][HE.W2].astype(np.float64))
    full, part = _row(ref.rows32, r), _row(ref.rows32, r, g1=g1)
    _caught(_plus(ref, {k: part[k] - full[k] for k in full}, (HE.W1, HE.B1)), ref, (HE.W1, HE.B1))


def test_mutation_sin_and_cos_blocks_of_one_feature_swapped():
    ref = HC.reference(HC.RANGE_ROWS)
    got = {k: v.copy() for k, v in ref.g32.items()}
    f, D, pe = 26, 27, 6
    s, c = slice(D + f * pe, D + (f + 1) * pe), slice(D + D * pe + f * pe, D + D * pe + (f + 1) * pe)
    got[HE.W0][:, s], got[HE.W0][:, c] = ref.g32[HE.W0][:, c], ref.g32[HE.W0][:, s]
    _caught(got, ref, (HE.W0,))


def test_mutation_bias_gradient_without_the_masked_partial_step():
    ref = HC.reference(HC.CHUNK_CASE)
    T, step = ref.rows, HC.kernel_constants()["step"]
    got = {k: v.copy() for k, v in ref.g32.items()}
    for k, q in ((HE.B0, "g0"), (HE.B1, "g1")):
        last = T - T % _chunk_rows(k, T)
        first = last + (T - last) // step * step
        assert last < first < T
        got[k] = got[k] - ref.rows32[q][first:].sum(0)
    _caught(got, ref, (HE.B0, HE.B1))


def test_mutation_one_small_scale_row_of_the_mixed_case_scaled_by_two():
    """A row whose ray has s_r <= 2^-20 counted twice: far below every whole-tensor measure, and visible where only small rows reach."""
    ref, b = HC.reference("mixed"), HC.built("mixed")
    ray_of = np.nonzero(ref.app_mask)[0]
    small = np.nonzero(b["s"][ray_of] <= 2.0 ** -20)[0]
    assert small.size > 50
    K = ref.K()
    over = [max(float((np.abs(c[k]) / np.maximum(K * ref.bound[k], 1e-300)).max()) for k in (HE.W2, HE.W1))
            for c in (_row(ref.rows32, int(r)) for r in small)]
    r = int(small[int(np.argmax(over))])
    assert max(over) > 2, "no small-scale row is visible on its own"
    _caught(_plus(ref, _row(ref.rows32, r)), ref, whole_tensor_passes=True)


def test_mutation_stray_non_zero_where_no_row_contributes():
    """mlp.0.weight has no padded column of its own (K0 = 351; the kernels' 352nd never reaches the tensor): a row of a hidden unit
    that is never active, and a colour channel without upstream, are the elements where any non-zero is a stray write."""
    ref = HC.reference("rows33")
    for k in (HE.W0, HE.W1, HE.B1):
        idx = tuple(np.argwhere(ref.A[k] == 0)[0])
        got = {kk: v.copy() for kk, v in ref.g32.items()}
        got[k][idx] = 1e-30
        lines = HE.failures(got, ref, ref.K())
        assert len(lines) == 1 and lines[0].startswith(k + ":") and "non-zero where no row" in lines[0], lines
    red = HC.reference("red")
    got = {kk: v.copy() for kk, v in red.g32.items()}
    got[HE.W2][2, 5] = -1e-30
    assert "non-zero where no row" in HE.failures(got, red, red.K())[0]


def test_small_elements_zeroed_pass_the_whole_tensor_check_only():
    """The gap this check closes: every element below 2e-4 of its tensor's largest gradient set to zero."""
    ref = HC.reference(HC.RANGE_ROWS)
    got, n = {}, 0
    for k, g in ref.g32.items():
        small = (np.abs(ref.g64[k]) < 2e-4 * np.abs(ref.g64[k]).max()) & np.array(k in HE.HEAD_KEYS)
        n += int((small & (ref.g64[k] != 0)).sum())
        got[k] = np.where(small, 0.0, g)
    assert n > 100
    _grad_check(got, ref.g64, rel=REL)
    assert len(HE.failures(got, ref, ref.K())) >= 3
