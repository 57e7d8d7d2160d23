"""Row-by-row reference for the FORWARD of the appearance head (positional encoding + 351 -> 128 -> 128 -> 3 MLP + sigmoid), computed on
the CPU from oracle_torch only; the forward half of tests/helpers/head_grad_elementwise.py, same design. The rows are inputs here: the
27 float32 features of a row carry no error, so everything below is the head's own arithmetic.

Values. `c64[row, 3]` = the head in float64 on the float32 feature row and the float32 weights, with oracle_torch.positional_encoding /
mlp_fea_noview's expressions restated (`head`; tests/test_head_rows_cpu.py pins the restatement to the oracle bit for bit); `c32` = the
plain float32 oracle.

Bound per element ("Forward rounding" of head_grad_elementwise.py). Per operand value v of a product, the split x = hi + lo,
hi = RTZ_f16(x), lo = RTZ_f16(x - hi), has the error o(v)^2 = (2^-24)^2 + (2^-22 v)^2 (F16_STEP: the spacing of the f16 subnormals is
the absolute floor of an unscaled residual). Weights are split AFTER k_ss_scales' power-of-two scale s_l = 2^(13 - k), max|W_l| =
m 2^k with m in [0.5, 1) (frexp), so s_l max|W_l| is in [2^12, 2^13); pack2 rounds to nearest: hi = RTN_f16(s w), lo = RTN_f16(s w - hi).
|s w - hi| <= 2^-11 |s w|, and the rounding of lo is <= 2^-11 of that where lo is normal and <= half the subnormal spacing, 2^-25,
otherwise: ow(w)^2 = (2^-25 / s_l)^2 + (2^-22 w)^2, a floor relative to max|W_l| (2^-25 / s_l <= 2^-37 max|W_l|).
The fp32 accumulation (MFMA partial sums, the three product chains, the bias FMA) adds 2^-22 of the layer's absolute sum
A_l = |in| |W_l|^T + |b_l| (head_grad_elementwise's 2^-22 A term). Independent errors add in quadrature, ReLU is 1-Lipschitz (no mask:
a unit whose pre-activation the error carries across zero still moves by no more than the error):

    dp0^2 = (o(x)^2 + dx^2) W0^2^T + x^2 ow(W0)^2^T + (2^-22 A0)^2,  dh0 = dp0
    dp1^2 = (o(h0)^2 + dh0^2) W1^2^T + h0^2 ow(W1)^2^T + (2^-22 A1)^2,  dh1 = dp1
    dp2^2 = (o(h1)^2 + dh1^2) W2^2^T + h1^2 ow(W2)^2^T + (2^-22 A2)^2

dx is zero on the 27 raw columns (inputs) and ENC_ERR[octave] on the sin / cos columns. The kernel (enc_unit, csrc/t2n_mlp_ss.hip)
takes octaves 0 and 3 fresh from the hardware sine / cosine: SIN_HW = 4.2e-7 absolute (tools/experiments/hw_sincos.hip, the project's
figure). Octaves 1, 2, 4, 5 are double-angle steps s' = fl(2 s c), c' = fl(1 - 2 s^2): with |ds|, |dc| <= e the exact-arithmetic
errors are 2 |c ds + s dc + ds dc| <= 2 sqrt(2) e (1 + e) and |4 s ds + 2 ds^2| <= 4 e (1 + e), and each result (|.| <= 1) rounds by at
most half an ulp, 2^-25: e' = 4 e (1 + e) + 2^-25 per step (`enc_err`; tests/test_head_rows_cpu.py checks the law with a float32 numpy
restatement of the recurrence against float64, fresh values perturbed by +-e adversarially).

The sigmoid. c = rcp(1 + exp(-p)): slope sigma'(p) <= 1/4; where 64 dp2 < 1/2 the slope is sigma'(|p| - 1/2) (sigma' falls with |p| and
no admissible error moves p by more than 1/2; K <= 64 is asserted by check). Hardware terms, absolute, added linearly: the kernel's
__expf(-p) is v_exp_f32(-p log2 e): the product's rounding (2^-24 relative on the argument) is |p| 2^-24 relative on the result and
v_exp_f32 is good to 1 ulp = 2^-23 relative (CDNA ISA guide); the sum 1 + e rounds by 2^-24 relative and v_rcp_f32 is good to 1 ulp:
    hw = c (2^-24 + 2^-23) + c (1 - c) (2^-23 + |p| 2^-24).
`Nm` = |c32 - c64|, the float32-minus-float64 difference of the oracle (a one-draw figure: it only adds).

    bound = slope * dp2 + hw + Nm,   K = 8 * max(1, rho32),   rho32 = max |c32 - c64| / bound

Because Nm is a term of the bound, rho32 <= 1 holds by construction and K is 8 in every case: rho32 says how much of the bound the
float32 oracle's own noise fills (0.10 to 0.33 on the in-range cases), it is no independent measurement of the model. What holds the
model to account is tests/test_head_rows_cpu.py's mutation tests and the laws it checks term by term (encoder, weight split).
rho32 is taken here from the float32 oracle, never from a kernel; the 8 has head_grad_elementwise's meaning (the dropped lo * lo term,
another summation order, quadrature against a correlated draw). The exact-fp32 form (k_shade<false>) is held to the same bound with the
split terms o, ow removed (`bound_exact`, with a rho32 line of its own).

`check(got, expect, K)`: |got - c64| <= K bound per live element, column 3 bit-equal to the row's weight (column 27), every slot that is
not live still the sentinel bit for bit.

Which instantiation runs. `scales_rule` restates k_ss_scales' row-norm bounds and its `ok` word; `variant_margin` is the factor by which
the deciding bound clears 0.5 kRange (the kernel forms the same sums in float32: a factor 2 cannot flip)."""
from dataclasses import dataclass, field
from typing import Dict

import numpy as np
import torch

from oracle import oracle_torch as O
from tests.helpers.head_grad_elementwise import B0, B1, B2, F16_STEP, SIN_HW, W0, W1, W2

FEA_PE = 6
D = 27
K0 = D * (1 + 2 * FEA_PE)
EPS = 2.0 ** -22
KRANGE = 59968.0          # csrc/t2n_mlp_ss.hip kRange
F16_MAX = 65504.0
SENTINEL = np.float32(-7.25)
HEAD_W = (W0, B0, W1, B1, W2, B2)


# ---- the head restated -----------------------------------------------------------------------------------------------------------------
def head(params, feat, dtype=torch.float64):
    """oracle_torch.mlp_fea_noview restated on rows feat [n, 27] (float32 values): returns x, p0, h0, p1, h1, p2, c as `dtype` tensors."""
    P = {k: torch.from_numpy(np.asarray(params[k], np.float32)).to(dtype) for k in HEAD_W}
    f = torch.from_numpy(np.ascontiguousarray(feat, dtype=np.float32)).to(dtype)
    x = torch.cat([f, O.positional_encoding(f, FEA_PE)], -1)
    p0 = x @ P[W0].T + P[B0]
    h0 = torch.relu(p0)
    p1 = h0 @ P[W1].T + P[B1]
    h1 = torch.relu(p1)
    p2 = h1 @ P[W2].T + P[B2]
    return dict(x=x, p0=p0, h0=h0, p1=p1, h1=h1, p2=p2, c=torch.sigmoid(p2))


def oracle_rows(params, feat, dtype):
    P = {k: torch.from_numpy(np.asarray(params[k], np.float32)).to(dtype) for k in HEAD_W}
    f = torch.from_numpy(np.ascontiguousarray(feat, dtype=np.float32)).to(dtype)
    return O.mlp_fea_noview(P, f, FEA_PE)


# ---- the encoder's error ---------------------------------------------------------------------------------------------------------------
def enc_step(e):
    """One double-angle step's error from the error e of (sin, cos) of the octave before (module docstring)."""
    return 4.0 * e * (1.0 + e) + 2.0 ** -25


def enc_err(e0=SIN_HW):
    """Absolute error of the sin / cos columns by octave 0..5: octaves 0 and 3 fresh, the others by double-angle steps."""
    e1 = enc_step(e0)
    e2 = enc_step(e1)
    return np.array([e0, e1, e2, e0, e1, e2], np.float64)


def enc_recurrence32(f, perturb=None):
    """float32 numpy restatement of enc_unit: (sin, cos) [n, 27, 6] of f 2^o; octaves 0 and 3 correctly rounded float32 values (+ an
    optional perturbation [n, 27, 2, 2] on the fresh (octave 0 / 3, sin / cos) values), octaves 1, 2, 4, 5 by s' = 2 s c, c' = 1 - 2 s^2."""
    f = np.asarray(f, np.float32)
    sn = np.zeros(f.shape + (6,), np.float32)
    cs = np.zeros_like(sn)
    for i, o in enumerate((0, 3)):
        a = f.astype(np.float64) * 2.0 ** o
        s, c = np.sin(a).astype(np.float32), np.cos(a).astype(np.float32)
        if perturb is not None:
            s = (s + perturb[..., i, 0].astype(np.float32)).astype(np.float32)
            c = (c + perturb[..., i, 1].astype(np.float32)).astype(np.float32)
        sn[..., o], cs[..., o] = s, c
        for q in (o + 1, o + 2):
            t = (s + s).astype(np.float32)
            s, c = (t * c).astype(np.float32), (np.float32(1) - (t.astype(np.float64) * s.astype(np.float64))).astype(np.float32)   # (fma: one rounding)
            sn[..., q], cs[..., q] = s, c
    return sn, cs


def _enc_cols(e0=SIN_HW):
    """dx per input column [351]: 0 on the raw features, enc_err[octave] on the sin and cos blocks (feature-major, octave-minor)."""
    e = np.tile(enc_err(e0), D)
    return np.concatenate([np.zeros(D), e, e])


# ---- which kernel the weights select ---------------------------------------------------------------------------------------------------
def layer_scale(w):
    """k_ss_scales' power-of-two scale of one layer: 2^(13 - k), max|w| = m 2^k, m in [0.5, 1)."""
    mx = float(np.abs(np.asarray(w, np.float32)).max())
    if not (0.0 < mx < 3e38):
        return 1.0
    return float(2.0 ** (13 - int(np.frexp(np.float32(mx))[1])))


def scales_rule(params):
    """k_ss_scales' row-norm bounds restated in float64 on the float32 weights: m4 (the four maxima), b0 / b1 of the `ok` rule (features
    up to 64) and ok = 1: the untracked kernel may run."""
    w0, b0, w1, b1 = (np.abs(np.asarray(params[k], np.float64)) for k in (W0, B0, W1, B1))
    m4 = np.array([(w0[:, D:].sum(1) + b0).max(), w0[:, :D].sum(1).max(), w1.sum(1).max(), b1.max()])
    B_0 = m4[0] + 64.0 * m4[1]
    B_1 = m4[2] * B_0 + m4[3]
    with np.errstate(invalid="ignore"):
        ok = bool(B_0 < 0.5 * KRANGE and B_1 < 0.5 * KRANGE)
    return dict(m4=m4, b0=B_0, b1=B_1, ok=ok)


def variant_margin(params):
    """(variant, margin): variant 1 = untracked. margin = the factor by which the deciding comparison clears 0.5 kRange: for the untracked
    kernel min over both bounds of 0.5 kRange / b, for the tracked one max(b0, b1) / (0.5 kRange)."""
    r = scales_rule(params)
    if r["ok"]:
        return 1, 0.5 * KRANGE / max(r["b0"], r["b1"])
    return 0, max(r["b0"], r["b1"]) / (0.5 * KRANGE)


def untracked_bounds(params, fmx):
    """The untracked kernel's run-time bounds for a largest |feature| fmx: b0 = fmx bounds[1] + bounds[0], b1 = bounds[2] b0 + bounds[3]
    (the stored bounds carry k_ss_scales' 1.0001)."""
    m = scales_rule(params)["m4"] * 1.0001
    b0 = fmx * m[1] + m[0]
    return b0, m[2] * b0 + m[3]


# ---- reference of a set of rows -------------------------------------------------------------------------------------------------------
@dataclass
class Reference:
    feat: np.ndarray                  # [n, 32] float32 rows as the kernel reads them (column 27 the weight)
    c64: np.ndarray                   # [n, 3]
    c32: np.ndarray
    bound: np.ndarray                 # split products (k_mlp_ss3, k_shade_coop)
    bound_exact: np.ndarray           # exact fp32 (k_shade<false>)
    rho32: float
    rho32_exact: float
    amax: np.ndarray = field(repr=False)      # [n, 3] float64 maxima per row of |feature|, |h0|, |h1|
    rows64: Dict[str, np.ndarray] = field(repr=False, default=None)

    def K(self, exact=False, factor=8.0):
        return factor * max(1.0, self.rho32_exact if exact else self.rho32)


def _bound(params, r, Nm, split):
    g = lambda k: np.asarray(params[k], np.float64)      # noqa: E731
    X, H0, H1, p2, c = (np.abs(r["x"]), np.abs(r["h0"]), np.abs(r["h1"]), r["p2"], r["c"])
    own = (lambda v: F16_STEP ** 2 + (EPS * v) ** 2) if split else (lambda v: np.zeros_like(v))      # noqa: E731

    def layer(inp, din2, wk, bk):
        w, b = g(wk), g(bk)
        ow2 = ((2.0 ** -25 / layer_scale(params[wk])) ** 2 + (EPS * w) ** 2) if split else np.zeros_like(w)
        A = inp @ np.abs(w).T + np.abs(b)
        return (own(inp) + din2) @ (w ** 2).T + (inp ** 2) @ ow2.T + (EPS * A) ** 2

    dx2 = np.broadcast_to(_enc_cols() ** 2, X.shape)
    dp0 = layer(X, dx2, W0, B0)
    dp1 = layer(H0, dp0, W1, B1)
    dp2 = np.sqrt(layer(H1, dp1, W2, B2))
    sp = lambda p: np.exp(-np.abs(p)) / (1.0 + np.exp(-np.abs(p))) ** 2      # noqa: E731  sigma'(p), stable
    slope = np.where(64.0 * dp2 < 0.5, sp(np.maximum(np.abs(p2) - 0.5, 0.0)), 0.25)
    hw = c * (2.0 ** -24 + 2.0 ** -23) + c * (1.0 - c) * (2.0 ** -23 + np.abs(p2) * 2.0 ** -24)
    return slope * dp2 + hw + Nm


def reference(params, feat):
    """The row-wise reference of feature rows feat [n, 32] (or [n, 27]: weight 0) under `params` (a state dict of numpy arrays)."""
    feat = np.asarray(feat, np.float32)
    if feat.shape[1] == D:
        feat = np.concatenate([feat, np.zeros((feat.shape[0], 32 - D), np.float32)], 1)
    f27 = feat[:, :D]
    with np.errstate(all="ignore"):
        r = {k: v.numpy() for k, v in head(params, f27, torch.float64).items()}
        c32 = oracle_rows(params, f27, torch.float32).numpy().astype(np.float64)
        Nm = np.abs(c32 - r["c"])
        b, be = _bound(params, r, Nm, True), _bound(params, r, Nm, False)
        fin = np.isfinite(b).all(1) & np.isfinite(r["c"]).all(1)
        rho = lambda bd: float((Nm[fin] / bd[fin]).max()) if fin.any() else 0.0      # noqa: E731
        amax = np.stack([np.abs(f27.astype(np.float64)).max(1), np.abs(r["h0"]).max(1), np.abs(r["h1"]).max(1)], 1)
    return Reference(feat=feat, c64=r["c"], c32=c32, bound=b, bound_exact=be, rho32=rho(b), rho32_exact=rho(be), amax=amax, rows64=r)


# ---- lists: where a row lives -----------------------------------------------------------------------------------------------------------
@dataclass
class Layout:
    """Eight sub-lists of `counts` entries (the raw counter words: a count above list_cap is clamped by the kernel) at `list_cap` slots
    each; `tile_hi` cuts the 32-entry tiles numbered through the lists in order; entry i of the launch (list order) shows pool row
    src[i]."""
    counts: tuple
    list_cap: int
    tile_hi: int = 0xffffffff
    src: np.ndarray = None

    def __post_init__(self):
        cnt = np.minimum(np.asarray(self.counts, np.int64), self.list_cap)
        tiles = (cnt + 31) // 32
        before = np.concatenate([[0], np.cumsum(tiles)])
        self.ntiles = int(before[-1])
        lst = np.repeat(np.arange(8), cnt)
        e = np.concatenate([np.arange(c) for c in cnt]) if cnt.sum() else np.zeros(0, np.int64)
        self.slot = lst * self.list_cap + e                         # app_rgb / slot-form row of every entry
        self.tile = before[lst] + e // 32
        self.dense = self.tile * 32 + e % 32                        # dense-form row of every entry
        self.live = self.tile < self.tile_hi                        # entries this launch shades
        self.n = int(cnt.sum())

    def place(self, pool_rows, seed):
        """src = a seeded permutation of the pool's rows, repeated when the launch holds more entries than the pool."""
        g = np.random.Generator(np.random.PCG64(seed))
        reps = -(-max(self.n, 1) // pool_rows)
        self.src = np.concatenate([g.permutation(pool_rows) for _ in range(reps)])[:self.n]
        return self

    def counters(self):
        c = np.zeros(8 * 64, np.int64)
        c[::64] = np.asarray(self.counts, np.int64)
        return c.astype(np.uint32).view(np.int32)

    def feat(self, pool_feat, slot_rows, poison):
        """The launch's feature rows: [8 list_cap, 32] by slot or [max(tiles, 1) * 32, 32] by dense tile; rows without an entry hold
        `poison` (nan or 0.0) in every column."""
        rows = 8 * self.list_cap if slot_rows else max(self.ntiles, 1) * 32
        out = np.full((rows, 32), poison, np.float32)
        out[self.slot if slot_rows else self.dense] = pool_feat[self.src]
        return out


@dataclass
class Expect:
    slots: int                 # rows of app_rgb
    live: np.ndarray           # slot of every live entry
    src: np.ndarray            # its pool row
    c64: np.ndarray
    bound: np.ndarray
    weight: np.ndarray         # float32


def expect(layout, ref, exact=False):
    s = layout.src[layout.live]
    return Expect(slots=8 * layout.list_cap, live=layout.slot[layout.live], src=s, c64=ref.c64[s], bound=(ref.bound_exact if exact else ref.bound)[s],
                  weight=ref.feat[s, D])


def blank(slots):
    return np.full((slots, 4), SENTINEL, np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def ratio(got, ex):
    """max |got - c64| / bound over the live elements (for information: what a run observed)."""
    if not ex.live.size:
        return 0.0
    err = np.abs(np.asarray(got, np.float64)[ex.live, :3] - ex.c64)
    return float(np.nan_to_num(err / ex.bound, nan=np.inf).max())


def failures(got, ex, K, values=True):
    """The report lines of everything that misses the check (empty: passed). values=False: sentinels and weights only (a launch whose
    range flag is up promises no colours)."""
    got = np.asarray(got, np.float32).reshape(ex.slots, 4)
    lines = []
    dead = np.ones(ex.slots, bool)
    dead[ex.live] = False
    bad = dead & (_bits(got) != _bits(SENTINEL)).any(1)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        lines.append(f"{int(bad.sum())} slot(s) without a live entry were written; first: slot {i} = {got[i].tolist()}")
    if ex.live.size:
        wbad = _bits(got[ex.live, 3]) != _bits(ex.weight)
        if wbad.any():
            i = int(np.flatnonzero(wbad)[0])
            lines.append(f"{int(wbad.sum())} weight column(s) differ from the row's column 27; first: slot {int(ex.live[i])} got {got[ex.live[i], 3]!r} want {ex.weight[i]!r}")
        if values:
            err = np.abs(got[ex.live, :3].astype(np.float64) - ex.c64)
            miss = ~(err <= K * ex.bound)
            if miss.any():
                score = np.where(miss, np.nan_to_num(err / ex.bound, nan=np.inf), -1.0)
                i, ch = np.unravel_index(int(score.argmax()), score.shape)
                lines.append(f"{int(miss.sum())} element(s) beyond K * bound; worst: slot {int(ex.live[i])} (pool row {int(ex.src[i])}) channel {int(ch)} got "
                             f"{got[ex.live[i], ch]:.9g} want {ex.c64[i, ch]:.9g} err/bound {float(score[i, ch]):.3g}")
    return lines


def check(got, ex, K, values=True):
    """|got - c64| <= K * bound per live element, weights bit-equal, every other slot still the sentinel. Returns max err / bound."""
    assert K <= 64.0, "the sigmoid's slope window assumes K <= 64"
    lines = failures(got, ex, K, values)
    assert not lines, f"head rows miss the row-wise check at K = {K:.3g}:\n" + "\n".join(lines)
    return ratio(got, ex) if values else float("nan")


def simulate(layout, ref, colours=None):
    """What a correct kernel leaves in app_rgb for `layout`: the float32 oracle's colours (or `colours` [pool rows, 3]) and the rows'
    weights in the live slots, the sentinel elsewhere."""
    out = blank(8 * layout.list_cap)
    s = layout.src[layout.live]
    out[layout.slot[layout.live], :3] = (ref.c32 if colours is None else colours)[s].astype(np.float32)
    out[layout.slot[layout.live], 3] = ref.feat[s, D]
    return out


# ---- the range flag ------------------------------------------------------------------------------------------------------------------
def flag_rules(params, ref, rows, variant, reads_poison=False):
    """(must_be_up, must_be_down) for a launch over pool rows `rows`: a live |feature|, |h0| or |h1| at or beyond the f16 maximum forces
    the flag; it must stay down where these float64 maxima — and for the untracked kernel its own bounds b0, b1 at the rows' largest
    |feature| — stay under half of kRange (not decidable when the launch reads non-finite rows that are not live: reads_poison)."""
    if not len(rows):
        return False, True
    with np.errstate(invalid="ignore"):
        a = ref.amax[rows]
        up = bool((~(a < F16_MAX)).any())
        mx = a.max(0)
        down = bool((mx < 0.5 * KRANGE).all()) and not reads_poison
        if down and variant == 1:
            b0, b1 = untracked_bounds(params, mx[0])
            down = bool(b0 < 0.5 * KRANGE and b1 < 0.5 * KRANGE)
    return up, down
