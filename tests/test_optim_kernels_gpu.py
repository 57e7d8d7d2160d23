"""The TV, Adam and loss kernels of csrc/t2n_optim.hip and csrc/t2n_loss.hip called directly through the C ABI on known inputs, each
against the float64 references of tests/helpers/optim_ref.py (checked on the CPU in tests/test_optim_ref_cpu.py): the
reference-layout kernels at shapes that take their lane loops, block caps and tails; the channel-last field kernels
(t2n_field_tv_adam_step, t2n_field_tv_seed) on a native field of grid 37 x 2 x 5 that is only uploaded and stepped, bit for bit
against the reference-layout kernels and against float64; the fused step's TV seed with device-side weights through the difference
of the gradients of steps with and without TV. Every buffer a kernel writes stands between two guard regions that must come back
untouched. Every input comes from a fixed numpy seed."""
import ctypes as C

import numpy as np
import pytest
import torch

from text2nerf_amd import _lib, synth
from tests.conftest import TINY
from tests.helpers import adam_readout as A
from tests.helpers import optim_ref as R
from tests.test_hip_parity import dev, make_field

pytestmark = pytest.mark.gpu

B1, B2 = A.F32_BETAS
EPS = float(np.float32(1e-8))
GUARD = 64                      # 32-bit words in front of and behind every buffer (256 bytes: float4 accesses stay aligned)
PATTERN = 0x7FC0BEEF            # a quiet NaN with a payload
HALF = 2.0 ** -24               # half an ulp, relative: one float32 rounding


def f32(x):
    return float(np.float32(x))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Buf:
    """A device array between two guard regions. `values`: its initial contents (float32 unless they are float64)."""

    def __init__(self, values):
        a = np.ascontiguousarray(values)
        assert a.dtype in (np.float32, np.float64)
        self.shape, self.words = a.shape, a.size * a.itemsize // 4
        self.full = torch.full((2 * GUARD + self.words,), PATTERN, dtype=torch.int32, device=dev())
        self.t = self.full[GUARD:GUARD + self.words].view(torch.float32 if a.dtype == np.float32 else torch.float64)
        self.set(a)

    @property
    def ptr(self):
        return C.c_void_p(self.full.data_ptr() + 4 * GUARD)

    def set(self, a):
        if self.words:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))

    def get(self):
        return self.t.cpu().numpy().reshape(self.shape).copy()

    def guards_intact(self):
        h = self.full.cpu().numpy()
        return bool(np.all(h[:GUARD] == PATTERN) and np.all(h[GUARD + self.words:] == PATTERN))


def call(name, *args):
    d = dev()
    with torch.cuda.device(d):
        _lib.check(getattr(_lib.load(), name)(*args, _lib.current_stream_ptr(d)), name)


# ---- TV on the reference layout -----------------------------------------------------------------------------------------------------------
TV_WEIGHT = 0.37


def assert_accumulated(got, prev, ref, mag, what):
    """got = prev + TV gradient in float32: the TV gradient within 1e-6 mag (nine roundings relative to mag are 5.4e-7), and the one
    addition into the gradient rounds by at most half an ulp of its result. `prev` is the float32 content of the gradient before the
    call: for a second add that is the kernel's own first result, so each call's accumulation is held on its own."""
    err = np.abs(got.astype(np.float64) - (prev.astype(np.float64) + ref))
    tol = 1e-6 * mag + 0.5 * np.spacing(np.abs(got)).astype(np.float64)
    assert np.all(err <= tol), (what, float((err / tol).max()), np.argwhere(err > tol)[:4].tolist())


@pytest.mark.parametrize("scale", R.VALUE_SCALES)
@pytest.mark.parametrize("shape", R.TV_GRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tv_grad_add_and_set_against_float64(shape, scale):
    c, h, w = shape
    rng = np.random.default_rng([7, c, h, w, R.VALUE_SCALES.index(scale)])
    x = R.plane(rng, shape, scale)
    ref, mag = R.tv_grad(x, f32(TV_WEIGHT))
    xb = Buf(x)
    # ADD, twice, into a gradient of the TV gradient's own size
    g0 = (rng.standard_normal(x.shape) * mag.mean()).astype(np.float32)
    gb = Buf(g0)
    call("t2n_tv_grad_add", xb.ptr, gb.ptr, c, h, w, TV_WEIGHT)
    g1 = gb.get()
    assert_accumulated(g1, g0, ref, mag, "first add")
    call("t2n_tv_grad_add", xb.ptr, gb.ptr, c, h, w, TV_WEIGHT)
    g2 = gb.get()
    assert_accumulated(g2, g1, ref, mag, "second add")
    # SET over NaN: no upstream scalar, then a device scalar (one more rounding)
    sb = Buf(np.full(x.shape, np.nan, np.float32))
    call("t2n_tv_grad_set", xb.ptr, sb.ptr, c, h, w, TV_WEIGHT, None)
    s = sb.get()
    assert not np.isnan(s).any()
    err = np.abs(s.astype(np.float64) - ref)
    print(f"{shape} {scale}: worst SET error {float((err / np.maximum(mag, 1e-300)).max()):.2e} of mag")
    assert np.all(err <= 1e-6 * mag), float((err / mag).max())
    up = Buf(np.array([1.7], np.float32))
    sb.set(np.full(x.shape, np.nan, np.float32))
    call("t2n_tv_grad_set", xb.ptr, sb.ptr, c, h, w, TV_WEIGHT, up.ptr)
    s = sb.get()
    assert not np.isnan(s).any()
    err = np.abs(s.astype(np.float64) - f32(1.7) * ref)
    assert np.all(err <= (1e-6 + HALF) * f32(1.7) * mag), float((err / mag).max())
    assert same_bits(xb.get(), x) and f32(up.get()[0]) == f32(1.7)
    assert all(b.guards_intact() for b in (xb, gb, sb, up))


@pytest.mark.parametrize("shape", [(16, 2, 2), (3, 4, 200), (2, 3, 65), (48, 172, 3)], ids=lambda s: "x".join(map(str, s)))
def test_tv_value_against_float64(shape):
    """The two sums of squares over 32 slot pairs, added up as losses._TVPlaneSum adds them; a second call accumulates on top."""
    c, h, w = shape
    rng = np.random.default_rng([8, c, h, w])
    x = R.plane(rng, shape, "unit")
    want = np.array(R.tv_sums(x))
    xb, sums = Buf(x), Buf(np.zeros((32, 2), np.float64))
    for rep in (1, 2):
        call("t2n_tv_value", xb.ptr, c, h, w, sums.ptr)
        got = sums.get().sum(0)
        rel = np.abs(got - rep * want) / (rep * want)
        print(f"{shape} call {rep}: relative error of the sums {rel}")
        assert np.all(rel <= 1e-6), rel
    assert same_bits(xb.get(), x) and xb.guards_intact() and sums.guards_intact()


# ---- Adam on the reference layout ----------------------------------------------------------------------------------------------------------
def assert_adam(p_prev, g, m_prev, v_prev, p, m, v, lr, step, what):
    """One Adam step's outputs (float32 arrays as the kernel left them) against float64: m_t within 1e-6 (|m_{t-1}| + |g|), v_t within
    1e-6 relative (all terms positive), p_t within adam_readout.param_tolerance of the update recomputed from the kernel's own m_t, v_t."""
    m_want = R.adam_first_moment(m_prev, g, A.one_minus(B1))
    tol = 1e-6 * (np.abs(m_prev.astype(np.float64)) + np.abs(g.astype(np.float64)))
    assert np.all(np.abs(m - m_want) <= tol), (what, "first moment")
    v_want = A.adam_second_moment(v_prev, g, B2, A.one_minus(B2))
    assert np.all(np.abs(v - v_want) <= 1e-6 * v_want), (what, "second moment")
    p_want = A.adam_param(p_prev, m, v, f32(lr), step, B1, B2, EPS)
    d = np.abs(p - p_want)
    tol = A.param_tolerance(p, p_want - p_prev)
    assert np.all(d <= tol), (what, "parameter", float((d / tol).max()))


ADAM_SIZES = (1, 255, 256, 257, 1000)


def test_adam_single_and_multi_against_float64():
    """35 tensors in one t2n_adam_step_multi call (two launches of its chunk loop), an empty tensor in the middle, per-tensor learning
    rates and step counts, three consecutive steps on carried moments; gradients with exact zeros and magnitudes from 1e-15 to 1e15
    (g^2 stays between 1e-30 and 1e30: clear of float32 denormals and of overflow). t2n_adam_step on copies of the same inputs must give
    the same bits."""
    rng = np.random.default_rng(11)
    T = 35
    sizes = [0 if i == 17 else ADAM_SIZES[i % 5] for i in range(T)]
    lrs = [(0.02, 1e-3)[i % 2] for i in range(T)]
    steps0 = [(1, 2, 1000, 100000)[i % 4] for i in range(T)]
    assert set(sizes) == set(ADAM_SIZES) | {0} and len({(n, s) for n, s in zip(sizes, steps0)}) >= 20
    p0 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    zero = [rng.random(n) < 0.25 for n in sizes]
    P, M, V = [Buf(a) for a in p0], [Buf(np.zeros(n, np.float32)) for n in sizes], [Buf(np.zeros(n, np.float32)) for n in sizes]
    G = [Buf(np.zeros(n, np.float32)) for n in sizes]
    VP = C.c_void_p * T
    arr = lambda bufs: VP(*[b.ptr.value for b in bufs])      # noqa: E731
    for s in range(3):
        g = []
        for i, n in enumerate(sizes):
            gi = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-15, 15, n)
            gi[zero[i]] = 0.0
            g.append(gi.astype(np.float32))
            G[i].set(g[i])
        prev = [(P[i].get(), M[i].get(), V[i].get()) for i in range(T)]
        steps = [t + s for t in steps0]
        call("t2n_adam_step_multi", T, arr(P), arr(G), arr(M), arr(V), (C.c_int64 * T)(*sizes), (C.c_float * T)(*lrs), B1, B2, EPS,
             (C.c_int64 * T)(*steps))
        for i, n in enumerate(sizes):
            what = (s, i, n, lrs[i], steps[i])
            p, m, v = P[i].get(), M[i].get(), V[i].get()
            assert same_bits(G[i].get(), g[i]), what                                  # the gradient is read only
            assert all(b.guards_intact() for b in (P[i], G[i], M[i], V[i])), what     # nothing past n, nothing in front
            assert_adam(*prev[i][:1], g[i], *prev[i][1:], p, m, v, lrs[i], steps[i], what)
            # zero gradient on zero moments: the parameter never moves
            assert same_bits(p[zero[i]], p0[i][zero[i]]) and not m[zero[i]].any() and not v[zero[i]].any(), what
            if n >= 255:      # (and the others do move: all but the gradients so far below eps that the update is under half an ulp)
                assert np.mean(p[~zero[i]] != prev[i][0][~zero[i]]) > 0.5, what
            # the single-tensor kernel on the same inputs
            sp, sg, sm, sv = Buf(prev[i][0]), Buf(g[i]), Buf(prev[i][1]), Buf(prev[i][2])
            call("t2n_adam_step", sp.ptr, sg.ptr, sm.ptr, sv.ptr, n, lrs[i], B1, B2, EPS, steps[i])
            assert same_bits(sp.get(), p) and same_bits(sm.get(), m) and same_bits(sv.get(), v), what
            assert same_bits(sg.get(), g[i]) and all(b.guards_intact() for b in (sp, sg, sm, sv)), what


# ---- the driver's loss ------------------------------------------------------------------------------------------------------------------------
LOSS_CASES = [(R_, N, wts, "mixed") for R_, N in ((1, 1), (5, 64), (6, 65), (301, 37), (1029, 3)) for wts in ((0.005, 1e3, 0.1), (0.0, 0.0, 0.1))] \
    + [(6, 65, (0.005, 1e3, 0.1), "all-true"), (6, 65, (0.005, 1e3, 0.1), "all-false")]


@pytest.mark.parametrize("R_,N,wts,mask_kind", LOSS_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_train_loss_against_float64(R_, N, wts, mask_kind):
    """k_train_loss + its reduce: one ray and one sample, N on both sides of a wave, 258 partial sums (R = 1029: the reduce's second
    trip), one NaN depth, the driver's weights and zero weights, masks that are all true / all false. z is built at least 1e-3 away
    from the mask's threshold, so float32 and float64 cannot disagree about the mask."""
    w_depth, w_trans, delta = wts
    rng = np.random.default_rng([12, R_, N, int(w_trans), ("mixed", "all-true", "all-false").index(mask_kind)])
    rgb, rgb_t = rng.random((R_, 3)).astype(np.float32), rng.random((R_, 3)).astype(np.float32)
    depth, dep_t = (rng.random(R_) * 6 + 1).astype(np.float32), (rng.random(R_) * 5 + 2).astype(np.float32)
    nan_at = 3 if R_ >= 5 else None
    if nan_at is not None:
        depth[nan_at] = np.nan
    w = (rng.random((R_, N)) * 0.05).astype(np.float32)
    u = {"mixed": rng.uniform(-4, 4, (R_, N)), "all-true": -rng.uniform(0.5, 3, (R_, N)), "all-false": rng.uniform(0.5, 3, (R_, N))}[mask_kind]
    u = np.where(np.abs(u + delta) < 5e-3, u + 0.02, u)
    z = (dep_t[:, None].astype(np.float64) + u).astype(np.float32)
    margin = (z.astype(np.float64) - dep_t[:, None].astype(np.float64)) + f32(delta)
    assert np.all(np.abs(margin) >= 1e-3)
    mask = margin < 0
    assert {"mixed": 0 < mask.sum() < mask.size or mask.size == 1, "all-true": mask.all(), "all-false": not mask.any()}[mask_kind]
    losses, d_rgb, d_depth, d_w = R.driver_loss(rgb, depth, w, z, rgb_t, dep_t, f32(w_depth), f32(w_trans), f32(delta))
    ws_bytes = int(_lib.load().t2n_train_loss_workspace_bytes(R_))
    assert ws_bytes > 0
    ins = [Buf(a) for a in (rgb, depth, w, z, rgb_t, dep_t)]
    nan = lambda *s: Buf(np.full(s, np.nan, np.float32))      # noqa: E731
    o_rgb, o_depth, o_w, o_losses, ws = nan(R_, 3), nan(R_), nan(R_, N), nan(4), nan(ws_bytes // 4)
    call("t2n_train_loss", *[b.ptr for b in ins], R_, N, w_depth, w_trans, delta, o_rgb.ptr, o_depth.ptr, o_w.ptr, o_losses.ptr, ws.ptr,
         ws_bytes)
    got = o_losses.get().astype(np.float64)
    print(f"losses {got} want {losses}")
    assert np.all(np.abs(got - losses) <= 2e-6 * np.abs(losses) + 1e-9), (got, losses)
    for name, g, want in (("d_rgb", o_rgb.get(), d_rgb), ("d_depth", o_depth.get(), d_depth), ("d_w", o_w.get(), d_w)):
        assert not np.isnan(g).any(), name
        assert float(np.abs(g - want).max()) <= 1e-6 * float(np.abs(want).max()) + 1e-12, name
    assert not o_w.get()[~mask].any()
    if w_trans and mask_kind != "all-false":
        assert np.all(o_w.get()[mask] > 0)
    if nan_at is not None:
        assert o_depth.get()[nan_at] == 0.0
    assert all(b.guards_intact() for b in ins + [o_rgb, o_depth, o_w, o_losses, ws])
    assert all(same_bits(b.get(), a) for b, a in zip(ins, (rgb, depth, w, z, rgb_t, dep_t)))      # inputs are read only


# ---- the channel-last field kernels on known gradients ---------------------------------------------------------------------------------------
FIELD_GRID = [37, 2, 5]         # planes of 74 (one block + 10, H = 2), 185 (tail 57) and 10 positions (W = 2); lines of 5, 2 and 37
TV_PAIRS = [(1e-3, 1e-4), (1e-3, 0.0), (0.0, 1e-4), (0.0, 0.0)]


def small_field():
    params = synth.make_field_params(21, FIELD_GRID, density_scale=0.9, aabb=TINY["aabb"])
    f = make_field(params, FIELD_GRID, TINY["aabb"], TINY["near_far"])
    f.sync_params()
    buf = f.factor_grad_buffer()
    named = A.kernel_named(f)[:12]
    shapes = [tuple(p.shape) for _, p in named]
    assert sorted(s[2] * s[3] for s in shapes[:3]) == [10, 74, 185] and sorted(s[2] for s in shapes[3:6]) == [2, 5, 37]
    assert [s[1] for s in shapes] == [16] * 6 + [48] * 6
    offs = A.shard_offsets(f)
    covered = np.zeros(buf.numel(), bool)
    for (off, n), (_, p) in zip(offs, named):
        assert n == p.numel() and off % 64 == 0 and not covered[off:off + n].any()
        covered[off:off + n] = True
    return f, buf, named, shapes, offs, covered


def tv_weight_of(i, pair):
    return pair[0] if i < 3 else (pair[1] if 6 <= i < 9 else 0.0)


@pytest.mark.parametrize("pair", TV_PAIRS, ids=lambda p: f"{p[0]:g}-{p[1]:g}")
def test_field_tv_adam_step_bitwise_and_against_float64(pair):
    """t2n_field_tv_adam_step, called as optim.TVAdam._step_factors_on_device calls it, on seeded gradients written into the field's
    channel-last buffer: two steps (zero moments, then carried ones with a fresh gradient), per-tensor learning rates and step counts.
    (a) parameters (the nn.Parameters and the channel-last master copies), the gradient with its TV term and both moments equal, bit for
    bit, t2n_tv_grad_add + t2n_adam_step on reference-layout copies; (b) the same outputs against float64 with the bounds of the
    reference-layout tests, so those kernels are not the only witness."""
    f, buf, named, shapes, offs, covered = small_field()
    rng = np.random.default_rng([13, TV_PAIRS.index(pair)])
    lrs = [(0.02, 1e-3)[i % 2] for i in range(12)]
    M = [Buf(np.zeros(p.numel(), np.float32)) for _, p in named]
    V = [Buf(np.zeros(p.numel(), np.float32)) for _, p in named]
    VP = C.c_void_p * 12
    ps = f._all_params()
    for t in (1, 2):
        steps = [t + 7 * (i % 3) for i in range(12)]
        p_prev = [p.detach().cpu().numpy().copy() for _, p in named]
        m_prev = [A.cl_to_ref(M[i].get(), shapes[i], A.is_line(i)) for i in range(12)]
        v_prev = [A.cl_to_ref(V[i].get(), shapes[i], A.is_line(i)) for i in range(12)]
        # gradients of the TV gradient's size and smaller and larger, so that neither vanishes in the other
        g = [(rng.standard_normal(s) * 10.0 ** rng.uniform(-7, -3, s)).astype(np.float32) for s in shapes]
        host = np.full(buf.numel(), np.nan, np.float32)
        for i, (off, n) in enumerate(offs):
            host[off:off + n] = A.ref_to_cl(g[i], A.is_line(i))
        buf.copy_(torch.from_numpy(host))
        with torch.cuda.device(dev()):
            pst = f._param_struct([p.detach() for p in ps])
            call("t2n_field_tv_adam_step", f._handle, C.byref(pst), VP(*[b.ptr.value for b in M]), VP(*[b.ptr.value for b in V]),
                 (C.c_float * 12)(*lrs), (C.c_int64 * 12)(*steps), B1, B2, EPS, pair[0], pair[1])
        torch.cuda.synchronize()
        after = buf.cpu().numpy()
        assert np.isnan(after[~covered]).all() and same_bits(after[~covered], host[~covered])      # alignment gaps: untouched
        master = A.master_copies(f)
        for i, (k, p) in enumerate(named):
            what = (pair, t, k)
            line, shape = A.is_line(i), shapes[i]
            _, c, h, w = shape
            tvw = tv_weight_of(i, pair)
            p_new = p.detach().cpu().numpy()
            g_tot = A.cl_to_ref(after[offs[i][0]:offs[i][0] + offs[i][1]], shape, line)
            m_new, v_new = A.cl_to_ref(M[i].get(), shape, line), A.cl_to_ref(V[i].get(), shape, line)
            assert M[i].guards_intact() and V[i].guards_intact(), what
            # (a) the reference-layout kernels on the same p, g, m, v
            rp, rg, rm, rv = Buf(p_prev[i]), Buf(g[i]), Buf(m_prev[i]), Buf(v_prev[i])
            if tvw != 0.0:
                call("t2n_tv_grad_add", rp.ptr, rg.ptr, c, h, w, tvw)
            call("t2n_adam_step", rp.ptr, rg.ptr, rm.ptr, rv.ptr, p.numel(), lrs[i], B1, B2, EPS, steps[i])
            assert same_bits(g_tot, rg.get()), (what, "gradient + TV")
            assert same_bits(m_new, rm.get()) and same_bits(v_new, rv.get()), (what, "moments")
            assert same_bits(p_new, rp.get()), (what, "nn.Parameter")
            assert same_bits(master[k], rp.get()), (what, "master copy")
            # (b) float64
            if tvw != 0.0:
                ref, mag = R.tv_grad(p_prev[i], f32(tvw))
                assert float(np.abs(ref).max()) > 0
                assert_accumulated(g_tot, g[i], ref, mag, (what, "gradient + TV against float64"))
            else:
                assert same_bits(g_tot, g[i]), what
            assert_adam(p_prev[i], g_tot, m_prev[i], v_prev[i], p_new, m_new, v_new, lrs[i], steps[i], what)
            assert np.mean(p_new != p_prev[i]) > 0.5, what


@pytest.mark.parametrize("pair", TV_PAIRS, ids=lambda p: f"{p[0]:g}-{p[1]:g}")
def test_field_tv_seed_bitwise_and_against_float64(pair):
    """t2n_field_tv_seed over a NaN-filled buffer: every float of the 12 slices written, zero where the weight is zero and on every line,
    bit-equal to t2n_tv_grad_set (no upstream scalar) on the reference-layout planes and within 1e-6 mag of float64; the floats between
    the slices stay as they were."""
    f, buf, named, shapes, offs, covered = small_field()
    buf.fill_(float("nan"))
    before = buf.cpu().numpy()
    call("t2n_field_tv_seed", f._handle, pair[0], pair[1])
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert same_bits(after[~covered], before[~covered])
    for i, (k, p) in enumerate(named):
        what = (pair, k)
        shape = shapes[i]
        _, c, h, w = shape
        tvw = tv_weight_of(i, pair)
        got = A.cl_to_ref(after[offs[i][0]:offs[i][0] + offs[i][1]], shape, A.is_line(i))
        assert not np.isnan(got).any(), what
        if tvw == 0.0:
            assert not bits(got).any(), what          # +0.0 everywhere
            continue
        x = p.detach().cpu().numpy()
        xb, sb = Buf(x), Buf(np.full(shape, np.nan, np.float32))
        call("t2n_tv_grad_set", xb.ptr, sb.ptr, c, h, w, tvw, None)
        assert same_bits(got, sb.get()), what
        ref, mag = R.tv_grad(x, f32(tvw))
        err = np.abs(got.astype(np.float64) - ref)
        assert float(np.abs(ref).max()) > 0 and np.all(err <= 1e-6 * mag), (what, float((err / mag).max()))


# ---- the fused step's TV seed with device-side weights ------------------------------------------------------------------------------------
FUSED_GRID = [23, 19, 17]       # planes of 437 / 391 / 323 positions: every one with a tail
FUSED_TV_W = 1000.0             # the TV weight of the step with TV (x 1e-2 in the kernels); see the test's docstring


def test_fused_step_tv_seed_with_device_side_weights():
    """launch_tv_seed_dev recomputes sh / sw on the device from the step's weights and is reachable only through t2n_train_step. Three
    fresh fields from the same parameters take one fused step each on the same 512 rays (40 samples) behind the same seed: two without
    TV, one with TV weight FUSED_TV_W on both plane groups. The gradients come out of Adam's first moments (zero before the step). The
    data gradient does not depend on the TV weight, so g_w - g_0a is the TV gradient up to `noise`, the run-to-run difference of the
    data gradient's atomic sums, measured here as max |g_0a - g_0b| per tensor:
        |(g_w - g_0a) - tv_grad(p, w 1e-2)| <= 1e-6 mag + 2e-7 |g_w| + 2 noise
    (2e-7 |g_w|: the float32 rounding of the moment the gradient is read from; 2 noise: the difference of two samples). The whole
    tolerance must stay below 1e-3 of the plane's largest TV gradient, or it would hide a wrong stencil. Lines carry no TV: their two
    gradients differ by no more than 2 noise + 1e-6 max |g_0a| of the tensor. The second term is not in the issue's bound (2 noise) and
    stands for the order of the float32 atomics that one pair of samples does not show: every element is a float32 sum whose order may
    change from run to run, a changed order moves it by ulps (6e-8) of its partial sums, and those are of the size of the tensor's
    largest gradients; the term allows 16 such ulps. Measured on the MI355X: with noise exactly 0 between the two steps without TV,
    density lines of the step with TV were 1.5e-10 and 2.9e-10 off (max |g| 6.4e-3 and 3.6e-3: one ulp of a large element's moment,
    8e-8 of max |g|) in one run and 0 in another; appearance lines 1.1e-12 off at a noise of 5.7e-13. Over 8 steps without and 4 with TV
    the largest difference between any two was 4.6e-8 of max |g| on density and 1.9e-7 on appearance lines, with and without TV alike;
    21 of 28 like pairs of density_line.0 measured 0. A TV term leaked into a line
    would be of the planes' size, 4e-3 to 1e-1: five decades and more above this bound."""
    from text2nerf_amd.optim import TVAdam
    params = synth.make_field_params(31, FUSED_GRID, density_scale=0.9, aabb=TINY["aabb"])
    g = np.random.Generator(np.random.PCG64(3))
    rays = torch.from_numpy(synth.frame_rays_np(16, 32, c2w=synth.look_pose(0.3, -0.1, (0.2, 0.1, -1.0))))
    assert rays.shape[0] == 512
    rgb_t = torch.from_numpy(g.uniform(0, 1, (512, 3)).astype(np.float32))
    dep_t = torch.from_numpy(g.uniform(2, 7, (512,)).astype(np.float32))

    def one_step(w):
        f = make_field(params, FUSED_GRID, TINY["aabb"], TINY["near_far"])
        opt = TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f)
        torch.manual_seed(77)
        f.train_step(rays, rgb_t, dep_t, opt, N_samples=40, white_bg=True, tv=[(f.density_plane, w), (f.app_plane, w)], fused=True, graph=False)
        fs = f._fused_step
        fs.sync()
        cur = A.snapshot(f, opt)
        assert all(s == 1 for s in cur["step"].values()), cur["step"]
        assert A.train_record(f)[1] == 1
        return {k: A.recover_grad(np.zeros_like(m), m, A.one_minus(B1)) for k, m in cur["m"].items()}, fs.replays

    g0a, _ = one_step(0.0)
    g0b, _ = one_step(0.0)
    gw, replays = one_step(FUSED_TV_W)
    print(f"TV weight {FUSED_TV_W:g}, replays of the step with TV: {replays}")
    failures = []
    for k in g0a:
        if "plane" not in k and "line" not in k:
            continue
        noise = float(np.abs(g0a[k] - g0b[k]).max())
        assert float(np.abs(g0a[k]).max()) > 0, k         # the rays reached this tensor
        d = gw[k] - g0a[k]
        if "line" in k:
            print(f"{k}: noise {noise:.3e}, max |g| {float(np.abs(g0a[k]).max()):.3e}, max |g_w - g_0a| {float(np.abs(d).max()):.3e}")
            if not float(np.abs(d).max()) <= 2 * noise + 1e-6 * float(np.abs(g0a[k]).max()):
                failures.append((k, "line gradient moved with the TV weight"))
            continue
        ref, mag = R.tv_grad(params[k], f32(f32(FUSED_TV_W) * 1e-2))
        tol = 1e-6 * mag + 2e-7 * np.abs(gw[k]) + 2 * noise
        err = np.abs(d - ref)
        print(f"{k}: noise {noise:.3e}, max |data g| {float(np.abs(g0a[k]).max()):.3e}, max |tv| {float(np.abs(ref).max()):.3e}, "
              f"max tolerance {float(tol.max()):.3e} ({float(tol.max() / np.abs(ref).max()):.2e} of max |tv|), worst error / tolerance "
              f"{float((err / tol).max()):.3f}")
        if not float(tol.max()) < 1e-3 * float(np.abs(ref).max()):
            failures.append((k, "tolerance too wide to see a wrong stencil"))
        if not np.all(err <= tol):
            failures.append((k, "TV gradient", float((err / tol).max())))
    assert not failures, failures
