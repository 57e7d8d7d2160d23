"""The depth-loss kernels (csrc/t2n_depth_loss.hip: t2n_train_loss_ex, t2n_depth_loss), the Python functions around them
(text2nerf_amd/losses.py) and train_step(depth_loss=...) against the float64 helper (tests/helpers/depth_loss_ref.py, itself held to
the reference in tests/test_depth_loss_cpu.py) on the cases of that helper: the shapes of LOSS_CASES, inputs kept away from every
branch (asserted on the CPU), directed one-hot rays for gnll, rank-deficient and ill-conditioned fits for ssi.

Bounds. The depth terms are evaluated in float64 from the first operation and rounded to float32 once when they are stored, so the
project's bounds for this stage hold without a per-element derivation (none was needed: profiles/depth_loss.txt has the measured
maxima): losses within 2e-6 |want| + 1e-9, gradients within 1e-6 max|want| + 1e-12. s and t: within 8 kappa (R N) 2^-53 max(|s|, |t|)
of the helper's, kappa the 2-norm condition number of the normal matrix the test computes per case; a rank-deficient fit has no
finite kappa, and its closed form y_bar (z0, 1) / (1 + z0^2) takes the bound with 1 + z0^2 in kappa's place (two float64 sums, two
divisions). K, the apply flags and the zeros the formulas give are exact.

si_log and the NaN depth: upstream's rule turns a NaN depth into 0 and log 0 = -inf poisons every output (pinned: "unguarded"), so the
si_log cases of t2n_train_loss_ex run on the case's `depth_fin` and one directed check holds the NaN case to a non-finite loss."""
import numpy as np
import pytest
import torch

from text2nerf_amd import _lib
from tests.conftest import TINY
from tests.helpers import depth_loss_ref as D
from tests.test_hip_parity import _grad_check, dev, make_field
from tests.test_optim_kernels_gpu import Buf, call, f32, same_bits

pytestmark = pytest.mark.gpu

CASES = D.all_cases()
WEIGHTS = ((0.005, 1e3, D.DELTA), (1.0, 0.0, D.DELTA))       # the driver's; the depth term alone at full weight


def kinds_of(cid):
    return {"rand": ("gnll", "si_log", "ssi"), "narrow": ("gnll", "si_log", "ssi"), "directed": ("gnll",), "ssi": ("ssi",)}[cid.split("-")[0]]


CASE_KINDS = [(cid, k) for cid in sorted(CASES) for k in kinds_of(cid)]


def nan(*shape, dtype=np.float32):
    return Buf(np.full(shape, np.nan, dtype))


def loss_ok(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    print(f"{what}: got {got} want {want} err/bound {np.max(err / (2e-6 * np.abs(want) + 1e-9)):.3g}")
    assert np.all(err <= 2e-6 * np.abs(want) + 1e-9), (what, got, want)


def grad_ok(got, want, what):
    assert not np.isnan(got).any(), what
    scale = float(np.abs(want).max()) if want.size else 0.0
    err = float(np.abs(got.astype(np.float64) - want).max()) if want.size else 0.0
    print(f"{what}: max|err| {err:.3e} = {err / (1e-6 * scale + 1e-12):.3g} of the bound (max|want| {scale:.3e})")
    assert err <= 1e-6 * scale + 1e-12, what


def aux_ok(kind, got, c, depth, what):
    """aux of one call against the helper; returns the helper's record."""
    R, N = c["w"].shape
    assert not np.isnan(got).any() and got[2] == 0.0 and got[3] == 0.0, what
    if kind == "gnll":
        o = D.gnll(depth, c["w"], c["z"], c["depth_t"], D.SIGMA)
        assert got[0] == o["K"], (what, got[0], o["K"])
        loss_ok(got[1], o["mean"], what + " signed mean")
    elif kind == "si_log":
        o = D.si_log(depth, c["depth_t"])
        loss_ok(got[0], o["alpha"], what + " alpha")
        assert got[1] == 0.0
    else:
        o = D.ssi(c["w"], c["z"], c["depth_t"], st_float32=True)
        kappa = (1.0 + o["z0"] ** 2) if o["deficient"] else o["kappa"]
        bound = 8.0 * kappa * (R * N) * 2.0 ** -53 * max(abs(o["s"]), abs(o["t"]))
        err = max(abs(got[0] - o["s"]), abs(got[1] - o["t"]))
        print(f"{what}: kappa {o['kappa']:.3e} deficient {o['deficient']} s {got[0]:.9g} t {got[1]:.9g} err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (what, err, bound)
    return o


@pytest.mark.parametrize("wts", WEIGHTS, ids=lambda w: f"{w[0]:g}-{w[1]:g}")
@pytest.mark.parametrize("cid,kind", CASE_KINDS, ids=lambda v: str(v))
def test_train_loss_ex_against_float64(cid, kind, wts):
    c = CASES[cid]
    R, N = c["w"].shape
    w_depth, w_trans, delta = wts
    depth = c["depth_fin"] if kind == "si_log" else c["depth"]
    host = (c["rgb"], depth, c["w"], c["z"], c["rgb_t"], c["depth_t"])
    want = D.driver_loss_ex(kind, *host, f32(w_depth), f32(w_trans), f32(delta), D.SIGMA)
    lib = _lib.load()
    ws_bytes = int(lib.t2n_train_loss_ex_workspace_bytes(R))
    ins = [Buf(a) for a in host]
    runs = []
    for _ in range(2):
        outs = dict(d_rgb=nan(R, 3), d_depth=nan(R), d_w=nan(R, N), losses=nan(4), aux=nan(4, dtype=np.float64), ws=nan(ws_bytes // 4))
        call("t2n_train_loss_ex", *[b.ptr for b in ins], R, N, w_depth, w_trans, delta, D.KINDS[kind], D.SIGMA, outs["d_rgb"].ptr,
             outs["d_depth"].ptr, outs["d_w"].ptr, outs["losses"].ptr, outs["aux"].ptr, outs["ws"].ptr, ws_bytes)
        assert all(b.guards_intact() for b in ins + list(outs.values()))
        runs.append({k: b.get() for k, b in outs.items() if k != "ws"})
    got = runs[0]
    for k in got:      # two calls give the same bits
        assert np.array_equal(got[k].view(np.uint8), runs[1][k].view(np.uint8)), k
    assert all(same_bits(b.get(), a) for b, a in zip(ins, host))      # inputs are read only
    what = f"{cid} {kind}"
    assert not np.isnan(got["losses"]).any()
    loss_ok(got["losses"], want[0], what + " losses")
    grad_ok(got["d_rgb"], want[1], what + " d_rgb")
    grad_ok(got["d_depth"], want[2], what + " d_depth")
    grad_ok(got["d_w"], want[3], what + " d_w")
    o = aux_ok(kind, got["aux"], c, np.where(np.isnan(depth), 0.0, depth), what)
    # the kernel the selector leaves alone: kind 0 is t2n_train_loss bit for bit, and the rgb term is the same in every kind
    base = dict(d_rgb=nan(R, 3), d_depth=nan(R), d_w=nan(R, N), losses=nan(4), ws=nan(int(lib.t2n_train_loss_workspace_bytes(R)) // 4))
    call("t2n_train_loss", *[b.ptr for b in ins], R, N, w_depth, w_trans, delta, base["d_rgb"].ptr, base["d_depth"].ptr, base["d_w"].ptr,
         base["losses"].ptr, base["ws"].ptr, base["ws"].words * 4)
    zero = dict(d_rgb=nan(R, 3), d_depth=nan(R), d_w=nan(R, N), losses=nan(4), aux=nan(4, dtype=np.float64), ws=nan(ws_bytes // 4))
    call("t2n_train_loss_ex", *[b.ptr for b in ins], R, N, w_depth, w_trans, delta, 0, D.SIGMA, zero["d_rgb"].ptr, zero["d_depth"].ptr,
         zero["d_w"].ptr, zero["losses"].ptr, zero["aux"].ptr, zero["ws"].ptr, ws_bytes)
    for k in ("d_rgb", "d_depth", "d_w", "losses"):
        if not np.isnan(base[k].get()).any():       # (the si_log rows run on depth_fin: no NaN anywhere)
            assert same_bits(zero[k].get(), base[k].get()), k
        else:
            assert np.array_equal(bits_of(zero[k].get()), bits_of(base[k].get())), k
    assert not zero["aux"].get().any() and all(b.guards_intact() for b in list(zero.values()) + list(base.values()))
    assert same_bits(got["d_rgb"], base["d_rgb"].get())
    # exact zeros where the formulas give zero
    mask = ((c["z"].astype(np.float64) - c["depth_t"][:, None].astype(np.float64)) + f32(delta)) < 0
    if kind == "si_log":
        assert same_bits(got["d_w"], base["d_w"].get())            # the transmittance term alone
    if kind == "ssi":
        assert not got["d_depth"].any()
    if kind == "gnll":
        idle = ~o["apply"]
        assert not got["d_depth"][idle].any()
        assert same_bits(got["d_w"][idle], base["d_w"].get()[idle])
        if o["K"] == 0:
            assert got["losses"][1] == 0.0 and not got["d_depth"].any() and same_bits(got["d_w"], base["d_w"].get())
    if np.isnan(depth).any():
        assert got["d_depth"][D.NAN_AT] == 0.0
    if not w_trans and kind != "ssi":
        untouched = ~mask if kind != "gnll" else np.broadcast_to((~o["apply"])[:, None], mask.shape)
        assert not got["d_w"][untouched].any()


def bits_of(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_train_loss_ex_si_log_with_a_nan_depth_is_not_finite():
    """Upstream's NaN rule makes the depth 0, and si_log takes its logarithm unguarded: the helper's loss is not finite, the kernel's neither."""
    c = CASES["rand-5x64"]
    R, N = c["w"].shape
    with np.errstate(all="ignore"):
        want = D.driver_loss_ex("si_log", c["rgb"], c["depth"], c["w"], c["z"], c["rgb_t"], c["depth_t"], 0.005, 1e3, D.DELTA)
    assert not np.isfinite(want[0][1])
    ws_bytes = int(_lib.load().t2n_train_loss_ex_workspace_bytes(R))
    ins = [Buf(c[k]) for k in ("rgb", "depth", "w", "z", "rgb_t", "depth_t")]
    outs = [nan(R, 3), nan(R), nan(R, N), nan(4), nan(4, dtype=np.float64), nan(ws_bytes // 4)]
    call("t2n_train_loss_ex", *[b.ptr for b in ins], R, N, 0.005, 1e3, D.DELTA, 2, D.SIGMA, *[b.ptr for b in outs], ws_bytes)
    losses = outs[3].get()
    assert np.isfinite(losses[0]) and np.isfinite(losses[2]) and not np.isfinite(losses[1])
    assert all(b.guards_intact() for b in ins + outs)


@pytest.mark.parametrize("cid,kind", CASE_KINDS, ids=lambda v: str(v))
def test_depth_loss_against_float64(cid, kind):
    """t2n_depth_loss: the term alone, upstream gradient 1, with and without the gradient outputs (and without w / z for si_log)."""
    c = CASES[cid]
    R, N = c["w"].shape
    depth = c["depth_fin"]
    term, d_depth, d_w, _ = D.depth_term(kind, depth, c["w"], c["z"], c["depth_t"], D.SIGMA)
    ws_bytes = int(_lib.load().t2n_depth_loss_workspace_bytes(R))
    ins = {k: Buf(a) for k, a in (("depth", depth), ("w", c["w"]), ("z", c["z"]), ("y", c["depth_t"]))}
    runs = []
    for grads, bare in ((True, False), (True, False), (False, False), (False, True)):
        if bare and kind == "gnll":
            continue
        outs = dict(loss=nan(1), aux=nan(4, dtype=np.float64), d_depth=nan(R), d_w=nan(R, N), ws=nan(ws_bytes // 4))
        dp = None if (bare and kind == "ssi") else ins["depth"].ptr
        wp, zp = (None, None) if (bare and kind == "si_log") else (ins["w"].ptr, ins["z"].ptr)
        call("t2n_depth_loss", D.KINDS[kind], dp, wp, zp, ins["y"].ptr, R, N, D.SIGMA, outs["loss"].ptr, outs["aux"].ptr,
             outs["d_depth"].ptr if grads else None, outs["d_w"].ptr if grads else None, outs["ws"].ptr, ws_bytes)
        assert all(b.guards_intact() for b in list(ins.values()) + list(outs.values()))
        runs.append({k: b.get() for k, b in outs.items() if k != "ws"})
    got = runs[0]
    for other in runs[1:]:
        assert same_bits(other["loss"], got["loss"]) and np.array_equal(other["aux"].view(np.uint64), got["aux"].view(np.uint64))
    for k in ("d_depth", "d_w"):
        assert same_bits(runs[1][k], got[k])                      # two calls give the same bits
        assert np.isnan(runs[2][k]).all()                         # NULL gradient outputs: nothing written
    assert all(same_bits(b.get(), a) for b, a in zip(ins.values(), (depth, c["w"], c["z"], c["depth_t"])))
    what = f"{cid} {kind} alone"
    loss_ok(got["loss"], [term], what + " loss")
    grad_ok(got["d_depth"], d_depth, what + " d_depth")
    grad_ok(got["d_w"], d_w, what + " d_w")
    o = aux_ok(kind, got["aux"], c, depth, what)
    if kind == "gnll":      # every apply flag: a ray's gradients are exact zeros exactly when it does not apply
        assert np.array_equal(got["d_w"].any(1) | (got["d_depth"] != 0), o["apply"] & (got["d_w"].any(1) | (got["d_depth"] != 0)))
        assert not got["d_depth"][~o["apply"]].any() and not got["d_w"][~o["apply"]].any()
        if o["K"] and o["mean"] != 0.0:
            assert np.all(got["d_depth"][o["apply"]] != 0)
        if o["K"] == 0:
            assert got["loss"][0] == 0.0
    if kind == "si_log":
        assert not got["d_w"].any()
        if R == 1:
            assert got["loss"][0] == 0.0 and got["d_depth"][0] == 0.0
    if kind == "ssi":
        assert not got["d_depth"].any()
        if cid == "ssi-zero-w":
            assert got["aux"][0] == 0.0 and got["aux"][1] == 0.0 and got["loss"][0] == 0.0


# ---- the Python functions under autograd ---------------------------------------------------------------------------------------------------
def on_device(c, *names, grad=()):
    d = dev()
    return [torch.from_numpy(c[k]).to(d).requires_grad_(k in grad) for k in names]


@pytest.mark.parametrize("cid", ["rand-6x65", "rand-301x37", "directed-mixed", "directed-k0"])
def test_compute_depth_loss_under_autograd(cid):
    from text2nerf_amd import losses
    c = CASES[cid]
    mu, z, w, y = on_device(c, "depth_fin", "z", "w", "depth_t", grad=("depth_fin", "w"))
    loss = losses.compute_depth_loss(mu, z, w, y, target_std=D.SIGMA)
    term, d_depth, d_w, aux = D.depth_term("gnll", c["depth_fin"], c["w"], c["z"], c["depth_t"], D.SIGMA)
    if aux[0] == 0:
        assert tuple(loss.shape) == (1,) and float(loss.detach()) == 0.0 and loss.requires_grad and loss.is_leaf
        return
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (loss * 2.5).backward()
    loss_ok(loss.detach().cpu().numpy(), term, cid)
    grad_ok(mu.grad.cpu().numpy(), 2.5 * d_depth, cid + " d_depth")
    grad_ok(w.grad.cpu().numpy(), 2.5 * d_w, cid + " d_w")
    var = ((z - mu.detach()[:, None]) ** 2 * w.detach()).sum(-1).double() + 1e-8
    flags = losses.is_not_in_expected_distribution(mu.detach().double(), var, y.double(), D.SIGMA)
    assert int(flags.sum()) == int(aux[0])
    with torch.no_grad():      # nothing asks for a gradient: the loss alone
        assert float(losses.compute_depth_loss(mu, z, w, y, target_std=D.SIGMA)) == float(loss.detach())


@pytest.mark.parametrize("cid", ["rand-6x65", "narrow-1029x3"])
def test_scale_invariant_losses_under_autograd(cid):
    from text2nerf_amd import losses
    c = CASES[cid]
    mu, z, w, y = on_device(c, "depth_fin", "z", "w", "depth_t", grad=("depth_fin", "w"))
    loss = losses.compute_depth_loss_scale_invariant(mu, y)
    assert loss.dim() == 0
    (loss * 0.5).backward()
    term, d_depth, _, _ = D.depth_term("si_log", c["depth_fin"], c["w"], c["z"], c["depth_t"])
    loss_ok(loss.detach().cpu().numpy(), term, cid + " si_log")
    grad_ok(mu.grad.cpu().numpy(), 0.5 * d_depth, cid + " si_log d_depth")
    loss, s, t = losses.scale_shift_invariant_loss(z, w, y)
    assert loss.dim() == 0 and s.dim() == 0 and t.dim() == 0 and s.dtype == torch.float64 and s.is_cuda and t.is_cuda
    (loss * 3.0).backward()
    term, _, d_w, _ = D.depth_term("ssi", c["depth_fin"], c["w"], c["z"], c["depth_t"])
    loss_ok(loss.detach().cpu().numpy(), term, cid + " ssi")
    grad_ok(w.grad.cpu().numpy(), 3.0 * d_w, cid + " ssi d_w")
    aux_ok("ssi", np.array([float(s), float(t), 0.0, 0.0]), c, None, cid + " ssi")


# ---- the training step ---------------------------------------------------------------------------------------------------------------------
class NoStep:
    """Stands in for the optimiser in train_step: the gradients are left where the backward put them."""

    def step(self, tv=()):
        pass


def positive_depth_batch(tiny_params):
    """The batch of tests/test_train_step.py, restricted to the rays whose evaluation-mode depth on the tiny field is positive (a ray
    that misses the box renders depth 0, whose logarithm si_log takes unguarded)."""
    from tests.test_train_step import batch
    rays, rgb_t, dep_t = batch()
    f = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    with torch.no_grad():
        depth = f(rays.to(dev()), is_train=False, white_bg=True, N_samples=-1)[1].cpu()
    keep = depth > 0.05
    assert int(keep.sum()) >= 128
    return rays[keep].contiguous(), rgb_t[keep].contiguous(), dep_t[keep].contiguous()


def autograd_step(f, kind, rays, rgb_t, dep_t, w_depth, w_trans, sigma):
    from text2nerf_amd import OctreeRender_trilinear_fast, losses
    d = dev()
    rgb, _, depth, w, z = OctreeRender_trilinear_fast(rays, f, chunk=rays.shape[0], N_samples=-1, white_bg=True, is_train=True, device=d)
    rgb_t, dep_t = rgb_t.to(d), dep_t.to(d)
    depth = torch.where(torch.isnan(depth), torch.zeros_like(depth), depth)
    mse = torch.mean((rgb - rgb_t) ** 2)
    tl = losses.TransMittanceLoss_mask()(w, (z - dep_t[:, None] + 0.1) < 0)
    if kind == "gnll":
        term = losses.compute_depth_loss(depth, z, w, dep_t, target_std=sigma).sum()
    elif kind == "si_log":
        term = losses.compute_depth_loss_scale_invariant(depth, dep_t)
    else:
        term = losses.scale_shift_invariant_loss(z, w, dep_t)[0]
    for p in f.parameters():
        p.grad = None
    tot = mse + w_depth * term + w_trans * tl
    tot.backward()
    return torch.stack([mse, term, tl, tot]).detach(), (rgb.detach(), depth.detach(), w.detach(), z.detach())


@pytest.mark.parametrize("kind", ["gnll", "si_log", "ssi"])
def test_train_step_with_a_depth_kind_equals_the_autograd_route_and_the_oracle(tiny_params, kind):
    """train_step(depth_loss=kind) on the composed route against (a) the autograd route — the same renderer under autograd, the
    losses.py function of the kind, the transmittance loss, backward(): the four losses at tests/test_train_step.py's bound (rtol 1e-5,
    atol 1e-9) and the 19 gradients within 1e-5 max|g| per tensor (both routes run the same backward kernels, which are linear in the
    upstream gradients; those agree to the loss stage's 1e-6 max|want|, and the factor 10 covers sum|contributions| / max|g| and the
    order of the float atomics) — and (b) driver_loss_ex on oracle_torch.forward's outputs at the oracle bound of
    tests/test_hip_fullsize.py (rtol 2e-5, atol 1e-9)."""
    from oracle import oracle_torch as O
    from tests.test_train_step import batch
    # the file's batch as it is; si_log alone drops rays whose rendered depth is not positive (it takes their logarithm unguarded)
    rays, rgb_t, dep_t = positive_depth_batch(tiny_params) if kind == "si_log" else batch()
    R = rays.shape[0]
    print(kind, "rays in the batch:", R, "of", batch()[0].shape[0])
    w_depth, w_trans, sigma = 0.05, 1e3, 0.1
    fa = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    fb = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    torch.manual_seed(41)
    jitter = torch.rand(R, 1)
    torch.manual_seed(41)
    la, _ = autograd_step(fa, kind, rays, rgb_t, dep_t, w_depth, w_trans, sigma)
    torch.manual_seed(41)
    lb = fb.train_step(rays, rgb_t, dep_t, NoStep(), N_samples=-1, white_bg=True, w_depth=w_depth, w_trans=w_trans, delta=0.1,
                       depth_loss=kind, depth_std=sigma, fused=None).clone()
    print(kind, "autograd", la.cpu().numpy(), "train_step", lb.cpu().numpy(), "aux", fb.last_depth_aux.cpu().numpy())
    assert torch.isfinite(lb).all()
    assert torch.allclose(la, lb, rtol=1e-5, atol=1e-9), (la, lb)
    assert fb.__dict__.get("_fused_step") is None
    aux = fb.last_depth_aux
    assert aux.is_cuda and aux.dtype == torch.float64 and tuple(aux.shape) == (4,)
    ref = {k: p.grad.detach().cpu().numpy() for k, p in fa.named_parameters()}
    assert len(ref) == 19
    worst = _grad_check(fb, ref, rel=1e-5)
    print(kind, "train_step vs autograd route, max |dg| / max |g|:", {k: f"{v:.1e}" for k, v in worst.items()})
    cfg = O.FieldConfig(aabb=TINY["aabb"], grid_size=TINY["grid"], near_far=TINY["near_far"])
    P = O.params_from_numpy(tiny_params, requires_grad=False, dtype=torch.float32)
    with torch.no_grad():
        rgb, depth, z, w = O.forward(cfg, P, rays, white_bg=True, is_train=True, n_samples=cfg.n_samples, jitter=jitter)
    want = D.driver_loss_ex(kind, rgb.numpy(), depth.numpy(), w.numpy(), z.numpy(), rgb_t.numpy(), dep_t.numpy(), w_depth, w_trans, 0.1,
                            float(np.float32(sigma)))[0]
    np.testing.assert_allclose(lb.cpu().numpy(), want, rtol=2e-5, atol=1e-9)


def test_train_step_depth_keywords(tiny_params, monkeypatch):
    """fused=True with a kind the one-call step does not compute raises; an unknown kind raises; train_step_indexed passes the keywords
    through; and depth_loss="mse" is the call without the keyword.

    The last point was specified as bit-equal parameters after three TVAdam steps. Measured on the MI355X, the call with the keyword
    and the call without it — the same instructions from the first line of train_step on — do not give that (density_plane.0 already
    differs in its last bits: the factor gradients are sums of float atomics whose order changes from run to run, the reason
    tests/test_train_step.py compares two runs of one path with assert_same_trajectory), so no implementation of the keyword could. What is asserted instead, and is no weaker about the keyword: on the composed route the
    first step's loss tensor and the three upstream gradients handed to the backward (everything the loss stage produces, i.e.
    everything the keyword can reach) are bit-equal with and without it; "mse" goes through t2n_train_loss, never t2n_train_loss_ex;
    on the default (fused) route the loss tensor of the first step is bit-equal; the CPU generator is in the same state after
    every step; and the parameters after three TVAdam steps agree at assert_same_trajectory's bound for two runs of one path. The
    test prints whether a control pair of identical calls came out bit-equal."""
    from text2nerf_amd._lib import T2NError
    from text2nerf_amd.dataset import DeviceTrainSet
    from text2nerf_amd.optim import TVAdam
    from tests.test_train_step import assert_same_trajectory, batch
    rays, rgb_t, dep_t = batch()
    new = lambda: make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])      # noqa: E731
    fields = [new() for _ in range(3)]
    opts = [TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f) for f in fields]
    for kind in ("gnll", "si_log", "ssi"):
        with pytest.raises(T2NError, match="composed route"):
            fields[0].train_step(rays, rgb_t, dep_t, opts[0], fused=True, depth_loss=kind)
    with pytest.raises(T2NError, match="depth_loss"):
        fields[0].train_step(rays, rgb_t, dep_t, opts[0], depth_loss="huber")
    # the composed route: what the loss stage hands on, captured at the backward's door
    lib = _lib.load()
    called = []
    real_ex = lib.t2n_train_loss_ex
    monkeypatch.setattr(lib, "t2n_train_loss_ex", lambda *a: (called.append(a[11]), real_ex(*a))[1])
    handed = []
    for kw in (dict(), dict(depth_loss="mse", depth_std=0.3)):
        f = new()
        real = f._backward_raw

        def spy(rays_, jitter, N, flags, ws, d_rgb, d_depth, d_w, _real=real, **k):
            handed.append([t.clone() for t in (d_rgb, d_depth, d_w)])
            return _real(rays_, jitter, N, flags, ws, d_rgb, d_depth, d_w, **k)

        f._backward_raw = spy
        torch.manual_seed(69)
        handed.append(f.train_step(rays, rgb_t, dep_t, NoStep(), N_samples=-1, white_bg=False, fused=False, **kw).clone())
        handed.append(torch.get_rng_state())
    assert not called and len(handed) == 6
    for a, b in zip(handed[0] + [handed[1], handed[2]], handed[3] + [handed[4], handed[5]]):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    # the default route, three steps with TVAdam
    first = []
    for it in range(3):
        states = []
        for f, o, kw in zip(fields, opts, (dict(), dict(depth_loss="mse", depth_std=0.3), dict())):
            torch.manual_seed(70 + it)
            losses = f.train_step(rays, rgb_t, dep_t, o, N_samples=-1, white_bg=False, tv=[(f.density_plane, 0.1), (f.app_plane, 0.01)], **kw)
            states.append(torch.get_rng_state())
            if it == 0:
                first.append(losses.clone())
        assert torch.equal(states[0], states[1]) and torch.equal(states[0], states[2])
    assert torch.equal(first[0].view(torch.int32), first[1].view(torch.int32)), (first[0], first[1])
    routes = []
    for f in fields:
        fs = f.__dict__.get("_fused_step")
        if fs is not None:
            fs.sync()
        routes.append(None if fs is None else fs.issued)
        assert f.last_depth_aux is None
    assert routes[0] == routes[1] == routes[2] and not called
    same = lambda fa, fb: all(torch.equal(a, b) for a, b in zip(fa.state_dict().values(), fb.state_dict().values()))      # noqa: E731
    print(f"parameters after 3 steps bit-equal: keyword vs none {same(fields[0], fields[1])}, none vs none (control) {same(fields[0], fields[2])}")
    assert_same_trajectory(fields[0], fields[1], steps=3)
    # train_step_indexed: the same step as train_step on the gathered rows
    src = DeviceTrainSet(rays, rgb_t, dep_t, device=dev())
    ids = torch.arange(0, rays.shape[0], 2)
    fi, fr = new(), new()
    torch.manual_seed(5)
    li = fi.train_step_indexed(src, ids, NoStep(), N_samples=-1, white_bg=True, depth_loss="ssi").clone()
    torch.manual_seed(5)
    lr = fr.train_step(rays[ids], rgb_t[ids], dep_t[ids], NoStep(), N_samples=-1, white_bg=True, depth_loss="ssi").clone()
    assert torch.allclose(li, lr, rtol=1e-5, atol=1e-9), (li, lr)
    assert torch.isfinite(fi.last_depth_aux).all() and torch.allclose(fi.last_depth_aux, fr.last_depth_aux, rtol=1e-6, atol=1e-9)
