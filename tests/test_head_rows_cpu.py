"""What the row-wise forward check of the appearance head (tests/helpers/head_rows_ref.py, cases in head_rows_cases.py) rests on, shown
without a GPU: the float64 restatement equals the oracle bit for bit, the float32 oracle sits inside its bound in every case, the
encoder's error law holds for a float32 restatement of the double-angle recurrence, the weight split's floor follows from pack2 and the
scale rule, every weight set selects its instantiation with a factor 2 to spare, the layouts reach the kernel's steps — and the checker
fails for each way the kernel could be subtly wrong (mutations), including the error the frame criterion cannot see."""
import numpy as np
import pytest
import torch

from tests.helpers import head_rows_cases as HC
from tests.helpers import head_rows_ref as HR
from tests.helpers.head_grad_elementwise import B0, B1, B2, SIN_HW, W0, W1, W2


def test_restatement_equals_the_oracle_bit_for_bit():
    for w in ("tiny", "outliers"):
        p = HC.weights(w)[0]
        f = HC.pool_rows()[:, :27]
        for dt in (torch.float64, torch.float32):
            assert torch.equal(HR.head(p, f, dt)["c"], HR.oracle_rows(p, f, dt)), (w, dt)
    ref = HC.pool_reference("tiny")
    assert np.array_equal(ref.c64, HR.oracle_rows(HC.weights("tiny")[0], HC.pool_rows()[:, :27], torch.float64).numpy())
    assert np.array_equal(ref.feat, HC.pool_rows(), equal_nan=True)


@pytest.mark.parametrize("wname", HC.WEIGHT_SETS)
def test_float32_oracle_inside_its_bound(wname):
    """rho32 <= 1 and K = 8 are identities (Nm is a term of the bound): what this test can fail on is a bound that is not finite and
    positive wherever the reference is, an exact bound above the split one, and a float32 oracle further than 1e-4 from float64."""
    refs = {"pool": HC.pool_reference(wname)}
    if wname in ("tiny", "l1_tracked"):
        refs.update({n: HC.range_reference(wname, n) for n in HC.RANGE_CASES})
    for n, r in refs.items():
        assert np.isfinite(r.c64).all() and (r.bound > 0).all() and (r.bound_exact > 0).all(), n
        assert (r.bound_exact <= r.bound).all(), n
        assert r.rho32 <= 1.0 and r.rho32_exact <= 1.0 and r.K() == 8.0 and r.K(exact=True) == 8.0, (n, r.rho32, r.rho32_exact)
        assert np.abs(r.c32 - r.c64).max() <= 1e-4, n


def test_encoder_error_law():
    """enc_err's per-step growth e' = 4 e (1 + e) + 2^-25 against a float32 restatement of the recurrence: with correctly rounded fresh
    values (error <= 2^-25) and with the fresh values pushed by +-e0 in the worst sign pattern, over the features of every range case
    that stays in range."""
    g = np.random.Generator(np.random.PCG64(5))
    f = np.concatenate([HC.pool_rows()[:512, :27], HC.range_rows("x1000")[:, :27], HC.range_rows("x3e4")[:64, :27],
                        g.uniform(-4, 4, (256, 27)).astype(np.float32)])
    a = f.astype(np.float64)[..., None] * 2.0 ** np.arange(6)
    for e0, signs in ((2.0 ** -25, [None]), (SIN_HW, [(1, 1), (1, -1), (-1, 1), (-1, -1)])):
        lim = HR.enc_err(e0)
        for sg in signs:
            pert = None
            if sg is not None:
                # push sin and cos along / against their own signs: the step's error terms c ds + s dc then add up
                # (by e0 - 2^-23: the float32 roundings of the value, 2^-25, and of the pushed value, up to 2^-24 beyond 1, are part of e0)
                pert, amp = np.zeros(f.shape + (2, 2)), e0 - 2.0 ** -23
                for i, o in enumerate((0, 3)):
                    pert[..., i, 0] = sg[0] * amp * np.sign(np.cos(a[..., o]))
                    pert[..., i, 1] = sg[1] * amp * np.sign(np.sin(a[..., o]))
            sn, cs = HR.enc_recurrence32(f, pert)
            err = np.maximum(np.abs(sn - np.sin(a)), np.abs(cs - np.cos(a))).reshape(-1, 6).max(0)
            assert (err <= lim).all(), (e0, sg, err, lim)
            if sg is not None:
                assert err[2] > 4 * e0 and err[5] > 4 * e0       # the law is not idle: two steps amplify by more than one step's 4


def test_weight_split_floor_follows_pack2():
    """pack2 restated (RTN halves of the scaled weight): |w - (hi + lo) / s| <= sqrt((2^-25 / s)^2 + (2^-22 w)^2), the scaled maximum
    lands in [2^12, 2^13), and the floor is <= 2^-37 max|W_l|."""
    for wname in HC.WEIGHT_SETS:
        p = HC.weights(wname)[0]
        for k in (W0, W1, W2):
            w = p[k].astype(np.float32)
            s = np.float32(HR.layer_scale(w))
            mx = float(np.abs(w).max()) * float(s)
            assert 2.0 ** 12 <= mx < 2.0 ** 13, (wname, k, mx)
            ws = w * s
            hi = ws.astype(np.float16)
            lo = (ws - hi.astype(np.float32)).astype(np.float16)
            err = np.abs(w.astype(np.float64) - (hi.astype(np.float64) + lo.astype(np.float64)) / float(s))
            lim = np.sqrt((2.0 ** -25 / float(s)) ** 2 + (2.0 ** -22 * w.astype(np.float64)) ** 2)
            assert (err <= lim).all(), (wname, k)
            assert 2.0 ** -25 / float(s) <= 2.0 ** -37 * float(np.abs(w).max())


def test_every_weight_set_selects_its_kernel_with_margin():
    """A factor 2 on the deciding bound for every set but `outliers`: 300 and -411 in layer 1 put k_ss_scales' b1 at 0.94 of 0.5 kRange
    (margin 1.063, untracked) and nothing that keeps those two weights moves it to a factor 2. What the factor is for — the kernel's own
    float32 sums must not flip the choice — needs far less: a sum of n <= 351 non-negative float32 terms is within n 2^-24 < 2.1e-5
    relative of its exact value, b0 and b1 add four more roundings, so a margin of 1.001 cannot flip; `outliers` is held to 1.05."""
    seen = set()
    for wname in HC.WEIGHT_SETS:
        p, intended, _ = HC.weights(wname)
        v, margin = HR.variant_margin(p)
        assert margin >= (1.05 if wname == "outliers" else 2.0), (wname, v, margin)
        if intended is not None:
            assert v == intended, (wname, v)
        seen.add(v)
    assert seen == {0, 1}                                        # both instantiations are reached
    # the tracked set built from the tiny weights keeps its true activations small: the row-norm bound, not a value, selects the kernel
    r = HC.pool_reference("l1_tracked")
    assert r.amax.max() < 0.5 * HR.KRANGE and np.abs(r.c64 - 0.5).max() < 0.499
    # the set built to leave the range does so on every row
    assert (HC.pool_reference("bias1e5").amax[:, 1] >= HR.F16_MAX).all()


def test_layouts_reach_the_kernels_steps():
    L = HC.layout("persist")
    assert L.ntiles == 3088 and -(-L.ntiles // 12) == 258 and L.ntiles % 12 == 4 and L.n == 98816
    assert HC.layout("tiles20").ntiles == 20
    assert HC.layout("mixed").ntiles == 2 + 1 + 1 + 4 + 1
    c = HC.layout("clamp1000")
    assert c.n == 96 + 5 + 40 and c.slot.max() < 8 * 96 and int(c.counters()[0]) == 1000
    assert HC.layout("cap100").list_cap % 32 != 0
    for hi in HC.TILE_HI:
        t = HC.layout("tiles20", hi)
        assert 0 < t.live.sum() < t.n and (t.tile[t.live] < hi).all()
    for name in HC.COUNT_CASES:
        L = HC.layout(name)
        assert len(np.unique(L.slot)) == L.n and len(np.unique(L.dense)) == L.n and (L.dense < max(L.ntiles, 1) * 32).all()
    # every tile position of a wave (t = 0, 1, 2), every wave, the first round, rounds past the grid and the partial last round show rows
    # of the pool in the persistence case
    pos = np.unique(HC.layout("persist").tile % 12)
    assert pos.size == 12 and HC.layout("persist").tile.max() // 12 == 257


def test_flag_rules_on_the_cases():
    p = HC.weights("tiny")[0]
    ref = HC.pool_reference("tiny")
    assert HR.flag_rules(p, ref, np.arange(HC.POOL), 1) == (False, True)          # the pool is in range: the flag must stay down
    assert HR.flag_rules(p, ref, np.arange(HC.POOL), 1, reads_poison=True) == (False, False)
    for name in HC.MUST_FLAG:
        assert HR.flag_rules(p, HC.range_reference("tiny", name), np.arange(200), 1)[0], name
    assert HR.flag_rules(HC.weights("bias1e5")[0], HC.pool_reference("bias1e5"), np.arange(64), HR.variant_margin(HC.weights("bias1e5")[0])[0])[0]
    assert not HR.flag_rules(p, HC.range_reference("tiny", "at_kRange"), np.arange(200), 1)[1]


# ---- mutations: each way the kernel could be subtly wrong must fail the checker ---------------------------------------------------------
def _rtz16(v):
    """RTZ_f16 of float64 values (the kernels' cvt_pkrtz), as float64."""
    h = np.asarray(v, np.float64).astype(np.float16)
    over = np.abs(h.astype(np.float64)) > np.abs(v)
    h[over] = np.nextafter(h[over], np.float16(0))
    return h.astype(np.float64)


def _forward(p, x, x_in=None, p1_delta=None, h1_hook=None):
    """The head in float64 numpy from its 351 input columns, with hooks for the mutations."""
    g = lambda k: np.asarray(p[k], np.float64)      # noqa: E731
    h0 = np.maximum((x if x_in is None else x_in) @ g(W0).T + g(B0), 0)
    p1 = h0 @ g(W1).T + g(B1)
    if p1_delta is not None:
        p1 = p1 + p1_delta(h0)
    h1 = np.maximum(p1, 0)
    if h1_hook is not None:
        h1 = h1_hook(h1)
    return 1.0 / (1.0 + np.exp(-(h1 @ g(W2).T + g(B2))))


def _mutants():
    p = HC.weights("tiny")[0]
    ref = HC.pool_reference("tiny")
    x = ref.rows64["x"]
    assert np.allclose(_forward(p, x), ref.c64, atol=1e-13)
    out = {}
    out["layer-0 inputs from their f16 hi parts only"] = _forward(p, x, x_in=_rtz16(x))
    s1 = HR.layer_scale(p[W1])
    ws = p[W1].astype(np.float32) * np.float32(s1)
    lo = (ws - ws.astype(np.float16).astype(np.float32)).astype(np.float16).astype(np.float64) / s1
    out["W_lo * x_hi of layer 1 dropped"] = _forward(p, x, p1_delta=lambda h0: -_rtz16(h0) @ lo.T)
    xs = x.copy()
    a, b = 27 + 7 * 6 + 2, 27 + 162 + 7 * 6 + 2
    xs[:, [a, b]] = xs[:, [b, a]]
    out["sin and cos of feature 7, octave 2 swapped"] = _forward(p, xs)
    x13 = x.copy()
    x13[:, 27 + 13 * 6 + 3:27 + 13 * 6 + 6] = 0
    x13[:, 27 + 162 + 13 * 6 + 3:27 + 162 + 13 * 6 + 6] = 0
    out["feature 13 encoded with octaves 0..2 only"] = _forward(p, x13)
    w2 = np.abs(np.asarray(p[W2], np.float64))

    def drop(h1):
        k = (h1[:, None, :] * w2[None]).max(1).argmax(1)
        h1 = h1.copy()
        h1[np.arange(h1.shape[0]), k] = 0
        return h1
    out["the hidden unit with the largest contribution missing"] = _forward(p, x, h1_hook=drop)
    return ref, out


def test_checker_passes_the_float32_oracle_in_every_layout():
    ref = HC.pool_reference("tiny")
    for name in list(HC.COUNT_CASES) + ["tiles20"]:
        for hi in ((0xffffffff,) if name != "tiles20" else HC.TILE_HI):
            L = HC.layout(name, hi)
            assert HR.check(HR.simulate(L, ref), HR.expect(L, ref), ref.K()) <= 1.0


def test_mutations_fail_the_checker():
    ref, mut = _mutants()
    L = HC.layout("mixed")
    ex = HR.expect(L, ref)
    K = ref.K()
    base = HR.simulate(L, ref)
    assert not HR.failures(base, ex, K)
    live, src = ex.live, ex.src
    # arithmetic mutants, ONE row each: the row whose effect / bound is the median over the launch's rows (half the rows show it more)
    for name, c in mut.items():
        eff = (np.abs(c[src] - ref.c64[src]) / ref.bound[src]).max(1)
        i = int(np.argsort(eff)[eff.size // 2])
        got = base.copy()
        got[live[i], :3] = c[src[i]].astype(np.float32)
        lines = HR.failures(got, ex, K)
        assert len(lines) == 1 and "beyond K * bound" in lines[0] and f"slot {int(live[i])} " in lines[0], (name, eff[i], lines)
        assert eff[i] > 2 * K, (name, eff[i])                 # (and not by a hair)
    # addressing mutants
    got = base.copy()
    got[live[:-1], :3] = base[live[1:], :3]
    assert any("beyond" in s for s in HR.failures(got, ex, K)), "row i with row i + 1's colours"
    last = int(np.flatnonzero(L.slot == 32)[0])               # list 0 holds 33 entries: entry 32 is alone in its tile
    got = base.copy()
    got[L.slot[last], :3] = base[L.slot[last - 1], :3]
    assert any("beyond" in s for s in HR.failures(got, ex, K)), "the last live row of a partial tile with its clamped neighbour's output"
    got = base.copy()
    got[33, 2] = np.float32(0.5)                              # slot 33 of list 0: dead
    assert any("without a live entry" in s for s in HR.failures(got, ex, K))
    got = base.copy()
    got[33, 3] = np.float32(-7.250001)                        # one bit beside the sentinel
    assert HR.failures(got, ex, K)
    got = base.copy()
    j = int(np.flatnonzero(ex.weight[:-1] != ex.weight[1:])[0])
    got[live[j], 3] = ex.weight[j + 1]
    assert any("weight column" in s for s in HR.failures(got, ex, K)), "weight column taken from another row"
    # a launch that must not shade past tile_hi and does
    Lh = HC.layout("tiles20", 7)
    got = HR.simulate(HC.layout("tiles20"), ref)
    assert any("without a live entry" in s for s in HR.failures(got, HR.expect(Lh, ref), K))


def test_small_weight_row_error_passes_the_frame_criterion_and_fails_here():
    """The gap this checker closes: a row that carries ray weight 0.01 and a colour error of 5e-3 moves its pixel by 5e-5, inside the
    frame tests' 1e-4 after compositing; row by row it is thousands of bounds off."""
    rows = HC.pool_rows()[:64].copy()
    rows[5, 27] = np.float32(0.01)
    ref = HR.reference(HC.weights("tiny")[0], rows)
    L = HR.Layout((64, 0, 0, 0, 0, 0, 0, 0), 128)
    L.src = np.arange(64)
    ex = HR.expect(L, ref)
    got = HR.simulate(L, ref)
    assert not HR.failures(got, ex, ref.K())
    got[5, 0] += np.float32(5e-3)
    pixel_change = float(got[5, 3]) * 5e-3
    assert pixel_change <= 1e-4                                # tests/test_hip_parity.RGB_ATOL: the frame criterion passes
    lines = HR.failures(got, ex, ref.K())
    assert lines and "slot 5 " in lines[0]
    assert 5e-3 > 1000 * ref.K() * ref.bound[5, 0]
