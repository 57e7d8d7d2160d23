"""The forward of the appearance head row by row, at the tile, round and range edges of k_mlp_ss3 (csrc/t2n_mlp_ss.hip), through the
diagnostic entry t2n_field_head_rows (the head alone on caller-made rows: no feature stage, no one-kernel tail, no exact redo), and the
two other head forms (k_shade_coop<false>, k_shade<false>) through f.shade at their count edges. Reference, per-element bound and
checker: tests/helpers/head_rows_ref.py; cases: tests/helpers/head_rows_cases.py; what the checker catches is shown without a GPU in
tests/test_head_rows_cpu.py.

Every launch: app_rgb pre-filled with a sentinel (slots without a live entry must keep it bit for bit), the weight column bit-equal to the
row's column 27, `variant` equal to the CPU's prediction from the weights, |colour - c64| <= K * bound per element at the CPU-measured
K = 8 * max(1, rho32) whenever the range flag stayed down, the flag against the soundness rules of head_rows_ref.flag_rules, and — position
independence — the colours of a pool row the same BITS wherever the row sits: tile t = 0, 1, 2 of a wave, waves 0..3, the first round, a
round past the 256-workgroup grid, the partial last round, dense or slot addressing, as in the plain pool launch that the bound checks
(`_pool_bits`). The three tiles of a wave, the riding and the stand-alone layer 2 and both addressing forms issue the same products
in the same order on every accumulator, so no position is exempt.

Both instantiations: every count, tile_hi, persistence and range case runs under the `tiny` weights (k_mlp_ss3<!TRACK>) and under
`l1_tracked` (k_mlp_ss3<TRACK>: the same weights with layer 1 scaled until the row-norm bound selects the tracked kernel while the true
activations stay small); the other three weight sets run the pool launch and three layouts.

Dead rows: every case runs with its rows without an entry poisoned by NaN and by zeros. Slot form: neither a live bit nor the flag may
change. Dense form: a partial tile's dead rows ARE read (load_feat clamps to the launch's last row, not to the list's last entry), their
columns never meet a live row's, so no live bit may change; the feature maximum of the wave sees them, so the NaN run raises the flag
(recorded in the HEADROWS lines; the zero run must not).

In-range cases may legitimately end flagged (the untracked kernel's row-norm bounds are conservative) — and it may equally be that none of
them does: a flagged launch promises no colours, only sentinels and weights are checked then, and the rules say where the flag MUST stay
down, which covers every pool case.
Cases built to leave the range (head_rows_cases.MUST_FLAG, the bias0 + 1e5 weights) assert the flag only.

Every launch prints one `HEADROWS` line with the observed max err / bound (profiles/head_rows_elementwise.txt keeps them)."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests.conftest import TINY
from tests.helpers import head_rows_cases as HC
from tests.helpers import head_rows_ref as HR
from tests.test_hip_parity import dev, make_field

pytestmark = pytest.mark.gpu
FORMS = ("dense", "slot")
NAN, ZERO = float("nan"), 0.0


@lru_cache(maxsize=None)
def _field(wname):
    return make_field(HC.weights(wname)[0], TINY["grid"], TINY["aabb"], TINY["near_far"])


def _launch(wname, lay, pool_feat, form, poison):
    f = _field(wname)
    feat = torch.from_numpy(lay.feat(pool_feat, form == "slot", poison)).to(dev())
    counters = torch.from_numpy(lay.counters()).to(dev())
    rgb = torch.from_numpy(HR.blank(8 * lay.list_cap)).to(dev())
    out, flag, variant = f.head_rows(feat, counters, lay.list_cap, lay.tile_hi, form == "slot", rgb)
    assert out.data_ptr() == rgb.data_ptr()
    c = counters.cpu().numpy()
    assert np.array_equal(np.delete(c, 32), np.delete(lay.counters(), 32)), "the launch wrote into the counter block beside the flag"
    return out.cpu().numpy(), flag, variant


def _judge(wname, case, lay, ref, form, poison, bits=None, must_flag=False):
    params = HC.weights(wname)[0]
    got, flag, variant = _launch(wname, lay, ref.feat, form, poison)
    assert variant == HR.variant_margin(params)[0], (wname, variant)
    assert flag in (0, 1)
    rows = lay.src[lay.live]
    cnt = np.minimum(np.asarray(lay.counts), lay.list_cap)
    reads_dead = form == "dense" and bool((cnt % 32 != 0).any()) and rows.size > 0
    up, down = HR.flag_rules(params, ref, rows, variant, reads_poison=reads_dead and np.isnan(poison))
    ex = HR.expect(lay, ref)
    values = flag == 0 and not must_flag
    K = ref.K()
    r = HR.ratio(got, ex) if values else float("nan")
    print(f"HEADROWS {wname} {case} {form} poison {'nan' if np.isnan(poison) else 'zero'} rows {rows.size} variant {variant} flag {flag} "
          f"K {K:.2f} rho32 {ref.rho32:.3f} max_err/bound {r:.3f}")
    if up or must_flag:
        assert flag == 1, "a live value at or beyond the f16 maximum and the range flag stayed down"
    if down:
        assert flag == 0, "every live value and bound under half of kRange and the range flag went up"
    HR.check(got, ex, K, values=values)
    if values and bits is not None and rows.size:
        same = (got[ex.live, :3].view(np.int32) == bits[ex.src].view(np.int32)).all(1)
        assert same.all(), f"{int((~same).sum())} row(s) differ in bits from the pool launch; first: slot {int(ex.live[np.flatnonzero(~same)[0]])}"
    return got, flag


@lru_cache(maxsize=None)
def _pool_bits(wname):
    """The pool in order in one dense launch (128 full tiles, 11 rounds): judged by the bound; every other launch of these weights must
    show the same bits per pool row."""
    lay = HR.Layout((512,) * 8, 512)
    lay.src = np.arange(HC.POOL)
    got, flag = _judge(wname, "pool", lay, HC.pool_reference(wname), "dense", NAN, must_flag=HC.weights(wname)[2])
    return got[:, :3].copy() if flag == 0 else None


def _both_poisons(wname, case, lay, ref, form, bits, must_flag=False):
    a, fa = _judge(wname, case, lay, ref, form, NAN, bits, must_flag)
    b, fb = _judge(wname, case, lay, ref, form, ZERO, bits, must_flag)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), "poisoned dead rows changed a live bit"
    if form == "slot":
        assert fa == fb, "poisoned dead slots changed the range flag"
    else:
        assert fb <= fa
    return a


BOTH = ("tiny", "l1_tracked")      # k_mlp_ss3<!TRACK> and k_mlp_ss3<TRACK> (tests/test_head_rows_cpu.py: which set selects which)


@pytest.mark.parametrize("wname", HC.WEIGHT_SETS)
def test_pool_launch(wname):
    bits = _pool_bits(wname)
    assert (bits is None) == HC.weights(wname)[2]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", list(HC.COUNT_CASES))
@pytest.mark.parametrize("wname", BOTH)
def test_row_counts(wname, case, form):
    lay = HC.layout(case)
    got = _both_poisons(wname, case, lay, HC.pool_reference(wname), form, _pool_bits(wname))
    if case == "zero":
        assert (got == HR.SENTINEL).all()
    if case == "clamp1000":
        assert (got[96 + 5:192] == HR.SENTINEL).all() and (got[:96 + 5, 3] != HR.SENTINEL).all()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("tile_hi", HC.TILE_HI)
@pytest.mark.parametrize("wname", BOTH)
def test_tile_hi_cuts_the_lists(wname, tile_hi, form):
    lay = HC.layout("tiles20", tile_hi)
    got = _both_poisons(wname, f"tile_hi{tile_hi}", lay, HC.pool_reference(wname), form, _pool_bits(wname))
    assert (got[lay.slot[~lay.live]] == HR.SENTINEL).all()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wname", BOTH)
def test_persistent_grid_wraps(wname, form):
    """3088 tiles: 258 rounds on 256 workgroups (workgroups 0 and 1 take a second round, whose rows they prefetched and across which the
    tracked kernel carries its maxima), the last round 4 tiles. Judged against the pool's bits. Every list is full: no launch of this
    case has a row without an entry, and the two poison runs differ in nothing — they run for uniformity and must agree bit for bit."""
    lay = HC.layout("persist")
    bits = _pool_bits(wname)
    assert bits is not None
    _both_poisons(wname, "persist", lay, HC.pool_reference(wname), form, bits)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("wname", [w for w in HC.WEIGHT_SETS if w != "tiny"])
def test_weight_sets(wname, form):
    must = HC.weights(wname)[2]
    bits = _pool_bits(wname)
    for case, lay in (("mixed", HC.layout("mixed")), ("tile_hi13", HC.layout("tiles20", 13)), ("n385", HC.layout("n385"))):
        for poison in (NAN, ZERO):
            _judge(wname, case, lay, HC.pool_reference(wname), form, poison, bits, must_flag=must)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", HC.RANGE_CASES)
@pytest.mark.parametrize("wname", BOTH)
def test_ranges(wname, case, form):
    _both_poisons(wname, case, HC.range_layout(), HC.range_reference(wname, case), form, None, must_flag=case in HC.MUST_FLAG)


def test_entry_refuses_what_it_cannot_run():
    """Sizes that do not cover the launch: T2N_ERR_INVALID (-1), and nothing is launched; the exact-fp32 mode: T2N_ERR_UNSUPPORTED."""
    import ctypes
    from text2nerf_amd import _lib
    lib = _lib.load()
    f = _field("tiny")
    h = f.sync_params()
    lay = HC.layout("mixed")
    counters = torch.from_numpy(lay.counters()).to(dev())
    rgb = torch.from_numpy(HR.blank(8 * 128)).to(dev())
    v = ctypes.c_uint32(7)
    s = _lib.current_stream_ptr(dev())

    def call(feat, cap, slot):
        return lib.t2n_field_head_rows(h, _lib.ptr(feat), feat.shape[0], _lib.ptr(counters), cap, 0xffffffff, slot, _lib.ptr(rgb), ctypes.byref(v), s)

    short = torch.zeros((lay.ntiles * 32 - 32, 32), device=dev())
    dense_ok = torch.zeros((lay.ntiles * 32, 32), device=dev())
    assert call(short, 128, 0) == -1                          # one tile short of the dense rows
    assert call(dense_ok, 128, 1) == -1                       # slot rows need a row per list slot
    assert call(dense_ok, 0, 0) == -1
    assert (rgb.cpu().numpy() == HR.SENTINEL).all() and int(counters[32]) == 0 and v.value == 7
    f.mlp_exact_fp32 = True
    try:
        with pytest.raises(_lib.T2NError):
            f.head_rows(dense_ok, counters, 128, app_rgb=rgb)
    finally:
        f.mlp_exact_fp32 = False
        f.sync_params()
    assert (rgb.cpu().numpy() == HR.SENTINEL).all()


# ---- the other two head forms at their count edges (f.shade: t2n_shade_at) ----------------------------------------------------------------
def _shade_case(exact, n):
    f = make_field(HC.weights("tiny")[0], TINY["grid"], TINY["aabb"], TINY["near_far"])
    f.mlp_exact_fp32 = exact
    pts = HC.points()
    idx = np.arange(n) % pts.shape[0]
    feat, rgb = f.shade(torch.from_numpy(pts[idx]).to(dev()))
    if not exact:
        # t2n_shade_at keeps the split launch's f16-range flag in word 0 of its workspace and runs k_shade<false> behind it when the word
        # is up: the figures below are k_shade_coop's only if it stayed down
        from text2nerf_amd import tensorf as tf
        flag = int(tf.workspace(dev(), 256)[:4].view(torch.int32).item())
        assert flag == 0, "k_shade_coop raised its range flag on in-range points: the colours would be the exact redo's"
    feat, rgb = feat.cpu().numpy(), rgb.cpu().numpy()
    first = min(n, pts.shape[0])
    # the colours against the float64 head of the features THIS call returned: the gather is out of the comparison
    ref = HR.reference(HC.weights("tiny")[0], feat[:first])
    K = ref.K(exact=exact)
    bound = ref.bound_exact if exact else ref.bound
    ratio = np.abs(rgb[:first].astype(np.float64) - ref.c64) / bound
    print(f"HEADROWS tiny shade_n{n} {'k_shade<false>' if exact else 'k_shade_coop<false>'} rows {n} K {K:.2f} rho32 {ref.rho32_exact if exact else ref.rho32:.3f} "
          f"max_err/bound {float(ratio.max()):.3f}")
    assert (ratio <= K).all(), (n, float(ratio.max()), int(np.unravel_index(ratio.argmax(), ratio.shape)[0]))
    if n > first:      # the grid-stride wrap: repeats of a point give the bits of its first occurrence
        assert np.array_equal(feat.view(np.int32), feat[idx].view(np.int32)), "features of repeated points differ"
        assert np.array_equal(rgb.view(np.int32), rgb[idx].view(np.int32)), "colours of repeated points differ"


@pytest.mark.parametrize("n", HC.POINT_COUNTS + (HC.WRAP_N,))
@pytest.mark.parametrize("exact", (False, True), ids=("coop", "exact"))
def test_point_shade_forms(exact, n):
    _shade_case(exact, n)
