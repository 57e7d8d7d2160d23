"""The L1 and ortho regulariser kernels of csrc/t2n_reg.hip (and their channel-last forms inside csrc/t2n_optim.hip's seed / TV
launches) called directly through the C ABI, against the float64 references and per-element checkers of tests/helpers/reg_ref.py
(checked on the CPU in tests/test_reg_ref_cpu.py): the reference-layout kernels on the case tables of that module — planes that hold
+0.0, -0.0 and denormals; lines of 2 .. 96 components by 1 .. 300 positions and one with rows of disjoint support — in their ADD and SET
forms, with and without the device upstream scalar; the field forms (t2n_field_reg_seed, t2n_field_reg_adam_step) on the 37 x 2 x 5
field of the TV tests, bit for bit against the reference-layout kernels; t2n_field_reg_seed with the new weights zero against
t2n_field_tv_seed; two calls giving the same bits; C = 1 refused. Every buffer a kernel writes stands between guard regions."""
import ctypes as C

import numpy as np
import pytest
import torch

from text2nerf_amd import _lib
from tests.helpers import adam_readout as A
from tests.helpers import reg_ref as R
from tests.test_hip_parity import dev
from tests.test_optim_kernels_gpu import B1, B2, EPS, Buf, bits, call, same_bits, small_field

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_WORKSPACE = -1, -4


def rc_of(name, *args):
    d = dev()
    with torch.cuda.device(d):
        return int(getattr(_lib.load(), name)(*args, _lib.current_stream_ptr(d)))


def nan_like(shape):
    return Buf(np.full(shape, np.nan, np.float32))


# ---- L1 on the reference layout -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.L1_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_l1_value_add_and_set(shape):
    x = R.l1_plane(shape)
    n = x.size
    xb = Buf(x)
    # value: T2N_REG_SLOTS partial sums, written (not added): NaN before, the same bits after a second call
    sums = Buf(np.full(_lib.REG_SLOTS, np.nan, np.float64))
    call("t2n_l1_value", xb.ptr, n, sums.ptr)
    s1 = sums.get()
    call("t2n_l1_value", xb.ptr, n, sums.ptr)
    assert np.array_equal(s1.view(np.uint64), sums.get().view(np.uint64))
    got, want = float(s1.sum()), R.l1_value([x])            # (the partial sums come divided by n)
    print(f"{shape}: mean|x| {got!r} want {want!r}")
    assert abs(got - want) <= 2 * (n + 8 + _lib.REG_SLOTS) * 2.0 ** -53 * want    # each side: at most n + 8 float64 roundings of positive terms, + one division per slot
    # ADD, twice, on a gradient of the term's own size
    rng = np.random.default_rng([51, *shape])
    g0 = (rng.standard_normal(x.shape) * R.L1_WEIGHT / n).astype(np.float32)
    gb = Buf(g0)
    call("t2n_l1_grad_add", xb.ptr, gb.ptr, n, R.L1_WEIGHT)
    g1 = gb.get()
    assert not R.check_l1_add(g1, g0, x, R.L1_WEIGHT)
    call("t2n_l1_grad_add", xb.ptr, gb.ptr, n, R.L1_WEIGHT)
    assert not R.check_l1_add(gb.get(), g1, x, R.L1_WEIGHT)
    # SET over NaN: without the upstream scalar, with it, and again (the same bits)
    sb = nan_like(x.shape)
    call("t2n_l1_grad_set", xb.ptr, sb.ptr, n, R.L1_WEIGHT, None)
    assert not R.check_l1_set(sb.get(), x, R.L1_WEIGHT)
    up = Buf(np.array([R.UPSTREAM], np.float32))
    sb.set(np.full(x.shape, np.nan, np.float32))
    call("t2n_l1_grad_set", xb.ptr, sb.ptr, n, R.L1_WEIGHT, up.ptr)
    s_up = sb.get()
    assert not R.check_l1_set(s_up, x, R.L1_WEIGHT, R.UPSTREAM)
    assert np.count_nonzero(s_up) == np.count_nonzero(x) and np.count_nonzero(x) < n       # zeros stay out, denormals count
    sb.set(np.full(x.shape, np.nan, np.float32))
    call("t2n_l1_grad_set", xb.ptr, sb.ptr, n, R.L1_WEIGHT, up.ptr)
    assert same_bits(sb.get(), s_up)
    assert same_bits(xb.get(), x) and all(b.guards_intact() for b in (xb, gb, sb, up, sums))


def test_l1_on_a_misaligned_slice():
    """A slice of a stacked tensor may start on any 4-byte boundary: the scalar path (12 bytes past a 16-byte boundary, odd length)."""
    x = R.l1_plane((3, 4, 200))
    flat = x.reshape(-1)[: 2399]
    xb, sb = Buf(np.concatenate([np.zeros(3, np.float32), flat])), nan_like(3 + flat.size)
    xp, sp = C.c_void_p(xb.ptr.value + 12), C.c_void_p(sb.ptr.value + 12)
    call("t2n_l1_grad_set", xp, sp, flat.size, R.L1_WEIGHT, None)
    got = sb.get()
    assert np.isnan(got[:3]).all() and not R.check_l1_set(got[3:], flat, R.L1_WEIGHT)
    assert xb.guards_intact() and sb.guards_intact()


# ---- ortho on the reference layout ---------------------------------------------------------------------------------------------------------
def ortho_value_tolerance(line):
    """Both float64 Gram matrices lie within n 2^-53 |m_i| |m_j| of the true D_ij; the sum of C^2 terms adds C^2 2^-53 of the value."""
    M = R.as_matrix(line)
    Cn, n = M.shape
    norm = np.sqrt((M * M).sum(1))
    pairs = norm.sum() ** 2 - (norm * norm).sum()
    return (n * 2.0 ** -52 * pairs) / (Cn * (Cn - 1)) + Cn * Cn * 2.0 ** -52 * R.ortho_value(line)


def run_ortho_case(name, line):
    M = R.as_matrix(line)
    Cn, n = M.shape
    xb = Buf(np.asarray(line, np.float32))
    ws_bytes = int(_lib.load().t2n_ortho_workspace_bytes(Cn))
    assert ws_bytes == Cn * Cn * 8
    ws = Buf(np.full(Cn * Cn, np.nan, np.float64))
    val = Buf(np.full(1, np.nan, np.float64))
    call("t2n_ortho_value", xb.ptr, Cn, n, val.ptr, ws.ptr, ws_bytes)
    v1, d1 = val.get().copy(), ws.get().copy()
    want = R.ortho_value(line)
    assert abs(float(v1[0]) - want) <= ortho_value_tolerance(line), (name, float(v1[0]), want)
    assert np.array_equal(d1.reshape(Cn, Cn), d1.reshape(Cn, Cn).T)                   # D is written symmetric
    assert np.all(np.sign(d1.reshape(Cn, Cn)) == np.sign(R.gram(line))), name           # every sign, the diagonal included
    call("t2n_ortho_value", xb.ptr, Cn, n, val.ptr, ws.ptr, ws_bytes)
    assert np.array_equal(v1.view(np.uint64), val.get().view(np.uint64)) and np.array_equal(d1.view(np.uint64), ws.get().view(np.uint64)), name
    # SET without / with the upstream scalar, twice
    sb = nan_like(line.shape)
    call("t2n_ortho_grad_set", xb.ptr, sb.ptr, Cn, n, R.ORTHO_WEIGHT, None, ws.ptr, ws_bytes)
    s0 = sb.get()
    bad = R.check_ortho_grad(s0, line, R.ORTHO_WEIGHT)
    assert not bad, (name, bad)
    up = Buf(np.array([R.UPSTREAM], np.float32))
    sb.set(np.full(line.shape, np.nan, np.float32))
    call("t2n_ortho_grad_set", xb.ptr, sb.ptr, Cn, n, R.ORTHO_WEIGHT, up.ptr, ws.ptr, ws_bytes)
    s_up = sb.get()
    bad = R.check_ortho_grad(s_up, line, R.ORTHO_WEIGHT, R.UPSTREAM)
    assert not bad, (name, bad)
    sb.set(np.full(line.shape, np.nan, np.float32))
    call("t2n_ortho_grad_set", xb.ptr, sb.ptr, Cn, n, R.ORTHO_WEIGHT, up.ptr, ws.ptr, ws_bytes)
    assert same_bits(sb.get(), s_up), name
    # ADD, twice, on a gradient of the term's own size
    rng = np.random.default_rng([52, Cn, n])
    g0 = (rng.standard_normal(line.shape) * max(float(np.abs(s0).max()), 1e-6)).astype(np.float32)
    gb = Buf(g0)
    call("t2n_ortho_grad_add", xb.ptr, gb.ptr, Cn, n, R.ORTHO_WEIGHT, ws.ptr, ws_bytes)
    g1 = gb.get()
    bad = R.check_ortho_grad(g1, line, R.ORTHO_WEIGHT, prev=g0)
    assert not bad, (name, "first add", bad)
    assert same_bits(g1, (g0 + s0).astype(np.float32)), name                           # the SET value, added once
    call("t2n_ortho_grad_add", xb.ptr, gb.ptr, Cn, n, R.ORTHO_WEIGHT, ws.ptr, ws_bytes)
    bad = R.check_ortho_grad(gb.get(), line, R.ORTHO_WEIGHT, prev=g1)
    assert not bad, (name, "second add", bad)
    # a workspace one byte short is refused
    assert rc_of("t2n_ortho_value", xb.ptr, Cn, n, val.ptr, ws.ptr, ws_bytes - 1) == ERR_WORKSPACE
    assert same_bits(xb.get(), np.asarray(line, np.float32)) and all(b.guards_intact() for b in (xb, ws, val, sb, up, gb)), name
    return s0


@pytest.mark.parametrize("Cn", R.ORTHO_C)
def test_ortho_value_and_grads(Cn):
    for n in R.ORTHO_N:
        run_ortho_case(f"{Cn}x{n}", R.ortho_line(Cn, n))


def test_ortho_disjoint_support_adds_exactly_nothing():
    """Rows 0 / 1 / 2 share no position: D_01 = D_02 = D_12 = 0 in any order, and the kernel's gradient is bit for bit the float32 sum
    over the other rows alone (tests/helpers/reg_ref.kernel_model_ortho with sign(0) = 0)."""
    line = R.disjoint_line()
    s0 = run_ortho_case("disjoint", line)
    assert same_bits(s0, R.kernel_model_ortho(line, R.ORTHO_WEIGHT).reshape(line.shape))
    assert not same_bits(s0, R.kernel_model_ortho(line, R.ORTHO_WEIGHT, sign_of_zero=1.0).reshape(line.shape))


def test_one_component_is_refused():
    x, g = Buf(np.ones((1, 1, 5, 1), np.float32)), nan_like((1, 1, 5, 1))
    ws, val = Buf(np.zeros(4, np.float64)), Buf(np.zeros(1, np.float64))
    assert int(_lib.load().t2n_ortho_workspace_bytes(1)) == 0
    assert rc_of("t2n_ortho_value", x.ptr, 1, 5, val.ptr, ws.ptr, 32) == ERR_INVALID
    assert rc_of("t2n_ortho_grad_add", x.ptr, g.ptr, 1, 5, 1.0, ws.ptr, 32) == ERR_INVALID
    assert rc_of("t2n_ortho_grad_set", x.ptr, g.ptr, 1, 5, 1.0, None, ws.ptr, 32) == ERR_INVALID
    assert np.isnan(g.get()).all() and g.guards_intact() and ws.guards_intact()


# ---- the channel-last field forms against the reference-layout kernels, bit for bit ------------------------------------------------------------
#            tv density, tv app, l1 planes, l1 lines, ortho density, ortho app
REG_SETS = [(1e-3, 1e-4, 0.7, 0.3, 0.9, 0.5),
            (0.0, 0.0, 0.7, 0.3, 0.9, 0.5),
            (1e-3, 1e-4, 0.7, 0.0, 0.0, 0.0),
            (0.0, 1e-4, 0.0, 0.3, 0.0, 0.5),
            (1e-3, 0.0, 0.0, 0.0, 0.9, 0.0)]


def weights_of(i, w):
    """(tv, l1, ortho) weight of factor tensor i (density planes 0-2, density lines 3-5, appearance planes 6-8, appearance lines 9-11)."""
    tv = w[0] if i < 3 else (w[1] if 6 <= i < 9 else 0.0)
    l1 = w[2] if i < 3 else (w[3] if i < 6 else 0.0)
    ortho = w[4] if 3 <= i < 6 else (w[5] if i >= 9 else 0.0)
    return tv, l1, ortho


def add_terms_reference_layout(rp, rg, shape, w_i, set_form):
    """TV, L1, ortho on reference-layout copies, in that order (SET form: the buffer starts as zero / the TV gradient)."""
    _, c, h, w = shape
    tv, l1, ortho = w_i
    if tv != 0.0:
        call("t2n_tv_grad_set" if set_form else "t2n_tv_grad_add", rp.ptr, rg.ptr, c, h, w, tv, *([None] if set_form else []))
    if l1 != 0.0:
        call("t2n_l1_grad_add", rp.ptr, rg.ptr, c * h * w, l1)
    if ortho != 0.0:
        ws = Buf(np.zeros(c * c, np.float64))
        call("t2n_ortho_grad_add", rp.ptr, rg.ptr, c, h, ortho, ws.ptr, c * c * 8)


@pytest.mark.parametrize("w", REG_SETS, ids=lambda w: "-".join(f"{v:g}" for v in w))
def test_field_reg_seed_bitwise(w):
    f, buf, named, shapes, offs, covered = small_field()
    buf.fill_(float("nan"))
    before = buf.cpu().numpy()
    call("t2n_field_reg_seed", f._handle, *w)
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert same_bits(after[~covered], before[~covered])
    call("t2n_field_reg_seed", f._handle, *w)
    torch.cuda.synchronize()
    assert same_bits(buf.cpu().numpy()[covered], after[covered])                       # two calls, the same bits
    for i, (k, p) in enumerate(named):
        shape = shapes[i]
        got = A.cl_to_ref(after[offs[i][0]:offs[i][0] + offs[i][1]], shape, A.is_line(i))
        x = p.detach().cpu().numpy()
        rp, rg = Buf(x), Buf(np.zeros(shape, np.float32))
        add_terms_reference_layout(rp, rg, shape, weights_of(i, w), True)
        assert same_bits(got, rg.get()), (w, k)
        if any(weights_of(i, w)):
            assert np.count_nonzero(got) > 0, (w, k)
        else:
            assert not bits(got).any(), (w, k)


@pytest.mark.parametrize("pair", [(1e-3, 1e-4), (0.0, 0.0)], ids=lambda p: f"{p[0]:g}-{p[1]:g}")
def test_field_reg_seed_without_the_new_terms_is_the_tv_seed(pair):
    f, buf, named, shapes, offs, covered = small_field()
    buf.fill_(float("nan"))
    call("t2n_field_tv_seed", f._handle, *pair)
    torch.cuda.synchronize()
    tv = buf.cpu().numpy()
    buf.fill_(float("nan"))
    call("t2n_field_reg_seed", f._handle, *pair, 0.0, 0.0, 0.0, 0.0)
    torch.cuda.synchronize()
    assert same_bits(buf.cpu().numpy(), tv)


@pytest.mark.parametrize("w", REG_SETS[:2] + REG_SETS[3:4], ids=lambda w: "-".join(f"{v:g}" for v in w))
def test_field_reg_adam_step_bitwise(w):
    """t2n_field_reg_adam_step on seeded gradients in the field's channel-last buffer, against t2n_tv_grad_add, t2n_l1_grad_add,
    t2n_ortho_grad_add and t2n_adam_step on reference-layout copies: gradient with its terms, moments, nn.Parameters and master copies."""
    f, buf, named, shapes, offs, covered = small_field()
    rng = np.random.default_rng([53, REG_SETS.index(w)])
    lrs = [(0.02, 1e-3)[i % 2] for i in range(12)]
    M = [Buf(np.zeros(p.numel(), np.float32)) for _, p in named]
    V = [Buf(np.zeros(p.numel(), np.float32)) for _, p in named]
    VP = C.c_void_p * 12
    ps = f._all_params()
    steps = [1 + 7 * (i % 3) for i in range(12)]
    p_prev = [p.detach().cpu().numpy().copy() for _, p in named]
    g = [(rng.standard_normal(s) * 10.0 ** rng.uniform(-5, -2, s)).astype(np.float32) for s in shapes]
    host = np.full(buf.numel(), np.nan, np.float32)
    for i, (off, n) in enumerate(offs):
        host[off:off + n] = A.ref_to_cl(g[i], A.is_line(i))
    buf.copy_(torch.from_numpy(host))
    with torch.cuda.device(dev()):
        pst = f._param_struct([p.detach() for p in ps])
        call("t2n_field_reg_adam_step", f._handle, C.byref(pst), VP(*[b.ptr.value for b in M]), VP(*[b.ptr.value for b in V]),
             (C.c_float * 12)(*lrs), (C.c_int64 * 12)(*steps), B1, B2, EPS, *w)
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert same_bits(after[~covered], host[~covered])
    master = A.master_copies(f)
    for i, (k, p) in enumerate(named):
        shape, line = shapes[i], A.is_line(i)
        g_tot = A.cl_to_ref(after[offs[i][0]:offs[i][0] + offs[i][1]], shape, line)
        rp, rg = Buf(p_prev[i]), Buf(g[i])
        rm, rv = Buf(np.zeros(shape, np.float32)), Buf(np.zeros(shape, np.float32))
        add_terms_reference_layout(rp, rg, shape, weights_of(i, w), False)
        call("t2n_adam_step", rp.ptr, rg.ptr, rm.ptr, rv.ptr, p.numel(), lrs[i], B1, B2, EPS, steps[i])
        assert same_bits(g_tot, rg.get()), (w, k, "gradient + terms")
        assert same_bits(A.cl_to_ref(M[i].get(), shape, line), rm.get()) and same_bits(A.cl_to_ref(V[i].get(), shape, line), rv.get()), (w, k)
        assert same_bits(p.detach().cpu().numpy(), rp.get()) and same_bits(master[k], rp.get()), (w, k, "parameters")
        assert M[i].guards_intact() and V[i].guards_intact(), (w, k)
