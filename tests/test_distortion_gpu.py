"""The distortion regulariser on the device (csrc/t2n_depth_loss.hip: t2n_distortion_loss, t2n_train_loss_dist), losses.distortion_loss
and train_step(distortion=w), against the float64 double sum of tests/helpers/distortion_ref.py (held to itself in
tests/test_distortion_cpu.py) on that helper's cases: N on both sides of the 64-sample tile carry, R on both sides of the four rays
of a workgroup, dense / box-like / directed weights, repeated depths.

Bounds. Gradient: |got - want| <= 2^-23 |want| + 1e-12 A_i / R with A_i = 2 sum_j w_j (|m_i| + |m_j|) + 2/3 w_i delta_i: the one
float32 rounding of the stored value, and the float64 summation order (4 N 2^-53 <= 1e-12 for N <= 2048; only the order differs from
the reference). The loss takes the same form with A = sum_i w_i A_i / 2. Where a float32 sum is stored (t2n_train_loss_dist's total and
d_weights: the old value plus the term) one ulp of that sum is added. The train_step checks use the bounds of
tests/test_depth_loss_gpu.py::test_train_step_with_a_depth_kind_equals_the_autograd_route_and_the_oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

from text2nerf_amd import _lib
from tests.conftest import TINY
from tests.helpers import distortion_ref as D
from tests.test_depth_loss_gpu import NoStep, nan, positive_depth_batch
from tests.test_hip_parity import _grad_check, dev, make_field
from tests.test_optim_kernels_gpu import Buf, call, f32, same_bits

pytestmark = pytest.mark.gpu

RHO = 1.0 / D.Z_RANGE
CASES = D.all_cases()
_REF = {}


def ref(cid):
    """(D, dD/dw) of a case by the double sum, computed once and left unchanged."""
    if cid not in _REF:
        d, g = D.distortion(CASES[cid]["w"], CASES[cid]["z"], RHO)
        g.setflags(write=False)
        _REF[cid] = (d, g)
    return _REF[cid]


def ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def run_distortion(w, z, grad=True):
    R, N = w.shape
    nbytes = int(_lib.load().t2n_distortion_loss_workspace_bytes(R))
    assert nbytes % 8 == 0 and nbytes >= 8
    wb, zb, loss, ws = Buf(w), Buf(z), nan(1), nan(nbytes // 4)
    dw = nan(R, N) if grad else None
    call("t2n_distortion_loss", wb.ptr, zb.ptr, R, N, RHO, loss.ptr, dw.ptr if grad else None, ws.ptr, nbytes)
    assert all(b.guards_intact() for b in (wb, zb, loss, ws) + ((dw,) if grad else ()))
    assert same_bits(wb.get(), w) and same_bits(zb.get(), z)
    return float(loss.get()[0]), (dw.get() if grad else None)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_distortion_loss_against_float64(cid):
    c = CASES[cid]
    w, z = c["w"], c["z"]
    want_l, want_g = ref(cid)
    got_l, got_g = run_distortion(w, z)
    lb, gb = D.loss_bound(w, z, RHO, want_l), D.grad_bound(w, z, RHO, want_g)
    el, eg = abs(got_l - want_l), np.abs(got_g.astype(np.float64) - want_g)
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"{cid}: D {got_l:.9g} want {want_l:.17g} err/bound {el / lb if lb else 0:.3g}; gradient max err/bound "
              f"{np.nanmax(np.where(gb > 0, eg / gb, 0.0)):.3g}, max|want| {np.abs(want_g).max():.3e}")
    assert not np.isnan(got_g).any() and np.isfinite(got_l)
    assert el <= lb, (cid, got_l, want_l, lb)
    assert np.all(eg <= gb), (cid, np.argwhere(eg > gb)[:4].tolist())
    # exact zeros: a ray without weight, and everything when all depths are equal
    idle = ~w.any(axis=1)
    assert not got_g[idle].any()
    if cid.startswith("equalz"):
        assert got_l == 0.0 and not got_g.any()
    if c["pattern"] == "box":
        assert idle.any()
    # two calls give the same bits; the loss alone (no gradient buffer) is the same loss
    again_l, again_g = run_distortion(w, z)
    assert same_bits(np.float32([again_l]), np.float32([got_l])) and same_bits(again_g, got_g)
    alone_l, _ = run_distortion(w, z, grad=False)
    assert same_bits(np.float32([alone_l]), np.float32([got_l]))


def test_directed_rays_on_the_device():
    """The directed rays of the CPU test at N = 65 (second tile: one sample) against their closed forms."""
    N = 65
    z = (2.0 + np.arange(N, dtype=np.float64) / 16.0).astype(np.float32)       # exact: steps of 1/16
    step = RHO / 16.0
    rows = dict(D.directed_rays(N))
    w = np.stack([rows["one"], rows["last"], rows["two"], np.zeros(N, np.float32)])
    zz = np.broadcast_to(z, w.shape).copy()
    per = []
    for r in range(4):          # each ray alone: its loss
        per.append(run_distortion(w[r:r + 1], zz[r:r + 1])[0])
    i, j = 0, (2 * N) // 3
    want = [0.75 ** 2 * step / 3.0, 0.0, 2 * (j - i) * step + 2 * step / 3.0, 0.0]
    print("directed:", per, want)
    assert per[1] == 0.0 and per[3] == 0.0
    assert abs(per[0] - want[0]) <= 2.0 ** -23 * want[0] and abs(per[2] - want[2]) <= 2.0 ** -23 * want[2]
    # the ray whose only weight sits on the last sample (N - 1 = 64: alone in the second tile)
    _, g = run_distortion(w[1:2], zz[1:2])
    assert g[0, N - 1] == 0.0 and np.all(g[0, :N - 1] > 0)


def test_a_ray_inside_a_batch_is_bit_equal_to_that_ray_alone():
    """R = 4 (the gradient's 1/R is a power of two: exact) for the ray alone, and one ray at two positions of two 5-ray batches."""
    c = CASES["dense-4x1025"]
    _, g = run_distortion(c["w"], c["z"])
    for r in range(4):
        _, alone = run_distortion(c["w"][r:r + 1], c["z"][r:r + 1])
        assert same_bits(g[r:r + 1] * np.float32(4.0), alone), r
    b = CASES["box-5x129"]
    w2, z2 = b["w"][::-1].copy(), b["z"][::-1].copy()
    _, ga = run_distortion(b["w"], b["z"])
    _, gb = run_distortion(w2, z2)
    assert same_bits(ga, gb[::-1])


# ---- t2n_train_loss_dist ------------------------------------------------------------------------------------------------------------------
LOSS_CASES = ["dense-1x1", "dense-5x64", "box-3x65", "dense-301x65", "dense-4x1025"]
W_DEPTH, W_TRANS, DELTA, SIGMA = 0.005, 1e3, 0.1, f32(0.1)


def loss_inputs(cid):
    c = CASES[cid]
    R, N = c["w"].shape
    rng = np.random.default_rng([23, R, N])
    rgb, rgb_t = rng.uniform(0, 1, (R, 3)).astype(np.float32), rng.uniform(0, 1, (R, 3)).astype(np.float32)
    depth, depth_t = rng.uniform(2.5, 5.5, R).astype(np.float32), rng.uniform(2.0, 6.0, R).astype(np.float32)
    return [rgb, depth, c["w"], c["z"], rgb_t, depth_t]


OUTS = ("d_rgb", "d_depth", "d_w", "losses", "aux")


def run_train_loss(name, host, kind, w_dist=None):
    R, N = host[2].shape
    lib = _lib.load()
    nbytes = int(getattr(lib, name + "_workspace_bytes")(R))
    ins = [Buf(a) for a in host]
    outs = dict(d_rgb=nan(R, 3), d_depth=nan(R), d_w=nan(R, N), losses=nan(4), aux=nan(4, dtype=np.float64), ws=nan((nbytes + 3) // 4))
    head = [b.ptr for b in ins] + [R, N, W_DEPTH, W_TRANS, DELTA]
    if name == "t2n_train_loss":
        call(name, *head, outs["d_rgb"].ptr, outs["d_depth"].ptr, outs["d_w"].ptr, outs["losses"].ptr, outs["ws"].ptr, nbytes)
        outs.pop("aux")
    elif name == "t2n_train_loss_ex":
        call(name, *head, kind, SIGMA, outs["d_rgb"].ptr, outs["d_depth"].ptr, outs["d_w"].ptr, outs["losses"].ptr, outs["aux"].ptr,
             outs["ws"].ptr, nbytes)
    else:
        outs["dist"] = nan(1, dtype=np.float64)
        call(name, *head, kind, SIGMA, w_dist, RHO, outs["d_rgb"].ptr, outs["d_depth"].ptr, outs["d_w"].ptr, outs["losses"].ptr,
             outs["aux"].ptr, outs["dist"].ptr, outs["ws"].ptr, nbytes)
    assert all(b.guards_intact() for b in ins + list(outs.values()))
    assert all(same_bits(b.get(), a) for b, a in zip(ins, host))
    return {k: b.get() for k, b in outs.items() if k != "ws"}


def bits64(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
@pytest.mark.parametrize("cid", LOSS_CASES)
def test_train_loss_dist_against_train_loss_ex_and_float64(cid, kind):
    host = loss_inputs(cid)
    w, z = host[2], host[3]
    R = w.shape[0]
    want_l, want_g = ref(cid)
    ex = run_train_loss("t2n_train_loss_ex", host, kind)
    # w_dist = 0: t2n_train_loss_ex bit for bit (kind 0: t2n_train_loss too); D is still reported
    zero = run_train_loss("t2n_train_loss_dist", host, kind, 0.0)
    for k in OUTS:
        assert np.array_equal(bits64(zero[k]), bits64(ex[k])), (k, "w_dist = 0")
    if kind == 0:
        base = run_train_loss("t2n_train_loss", host, kind)
        for k in ("d_rgb", "d_depth", "d_w", "losses"):
            assert np.array_equal(bits64(zero[k]), bits64(base[k])), (k, "kind 0")
    lb = D.loss_bound(w, z, RHO, want_l)
    assert abs(zero["dist"][0] - want_l) <= lb
    # w_dist > 0
    w_dist = f32(0.37)
    got = run_train_loss("t2n_train_loss_dist", host, kind, w_dist)
    again = run_train_loss("t2n_train_loss_dist", host, kind, w_dist)
    for k in OUTS + ("dist",):
        assert np.array_equal(bits64(got[k]), bits64(again[k])), (k, "two calls")
    for k in ("d_rgb", "d_depth", "aux"):
        assert np.array_equal(bits64(got[k]), bits64(ex[k])), k
    assert np.array_equal(bits64(got["losses"][:3]), bits64(ex["losses"][:3]))
    assert abs(got["dist"][0] - want_l) <= lb, (got["dist"], want_l, lb)
    total = float(ex["losses"][3]) + w_dist * want_l
    e_tot = abs(float(got["losses"][3]) - total)
    assert e_tot <= ulp(total) + w_dist * lb, (got["losses"], total)
    want_dw = ex["d_w"].astype(np.float64) + w_dist * want_g
    e_dw = np.abs(got["d_w"].astype(np.float64) - want_dw)
    b_dw = w_dist * D.grad_bound(w, z, RHO, want_g) + ulp(want_dw)
    print(f"{cid} kind {kind}: total err {e_tot:.3e}; d_w max err/bound {np.max(e_dw / b_dw):.3g}; D {got['dist'][0]:.12g}")
    assert np.all(e_dw <= b_dw), np.argwhere(e_dw > b_dw)[:4].tolist()
    # exact zeros where no term contributes: a ray without weight whose samples all lie behind the target's gate
    idle = ~w.any(axis=1)
    if idle.any() and kind in (0, 2):
        assert np.array_equal(bits64(got["d_w"][idle]), bits64(ex["d_w"][idle]))


SENTINEL = np.float32(-7.25)
ERR_INVALID, ERR_WORKSPACE = -1, -4          # T2N_ERR_INVALID, T2N_ERR_WORKSPACE of include/t2n.h


def test_train_loss_dist_and_distortion_loss_refuse_bad_arguments_before_writing():
    host = loss_inputs("dense-5x64")
    R, N = host[2].shape
    lib = _lib.load()
    nbytes = int(lib.t2n_train_loss_dist_workspace_bytes(R))
    assert nbytes % 8 == 0 and nbytes > int(lib.t2n_train_loss_ex_workspace_bytes(R))
    ins = [Buf(a) for a in host]
    new = lambda *s, dtype=np.float32: Buf(np.full(s, SENTINEL, dtype))      # noqa: E731
    outs = dict(d_rgb=new(R, 3), d_depth=new(R), d_w=new(R, N), losses=new(4), aux=new(4, dtype=np.float64), dist=new(1, dtype=np.float64),
                ws=new(nbytes // 4 + 2))
    st = _lib.current_stream_ptr(dev())

    def train(**kw):
        a = dict(rgb=ins[0].ptr, depth=ins[1].ptr, w=ins[2].ptr, z=ins[3].ptr, rgb_t=ins[4].ptr, depth_t=ins[5].ptr, R=R, N=N, kind=1,
                 sigma=SIGMA, w_dist=0.5, rho=RHO, ws=outs["ws"].ptr, nbytes=nbytes, **{k: outs[k].ptr for k in OUTS + ("dist",)})
        a.update(kw)
        with torch.cuda.device(dev()):
            return lib.t2n_train_loss_dist(a["rgb"], a["depth"], a["w"], a["z"], a["rgb_t"], a["depth_t"], a["R"], a["N"], W_DEPTH, W_TRANS, DELTA,
                                           a["kind"], a["sigma"], a["w_dist"], a["rho"], a["d_rgb"], a["d_depth"], a["d_w"], a["losses"],
                                           a["aux"], a["dist"], a["ws"], a["nbytes"], st)

    off4 = C.c_void_p(outs["ws"].ptr.value + 4)
    invalid = [dict(rgb=None), dict(w=None), dict(z=None), dict(d_w=None), dict(losses=None), dict(aux=None), dict(dist=None), dict(ws=None),
               dict(R=0), dict(N=0), dict(N=-3), dict(kind=4), dict(kind=-1), dict(kind=1, sigma=0.0), dict(rho=0.0), dict(rho=-0.25),
               dict(rho=float("inf")), dict(rho=float("nan")), dict(w_dist=-1.0), dict(w_dist=float("inf")), dict(w_dist=float("nan")),
               dict(ws=off4)]
    for kw in invalid:
        assert train(**kw) == ERR_INVALID, kw
    assert train(nbytes=nbytes - 8) == ERR_WORKSPACE and train(nbytes=0) == ERR_WORKSPACE
    # the term alone
    dl, dd, dws = new(1), new(R, N), new(int(lib.t2n_distortion_loss_workspace_bytes(R)) // 4 + 2)

    def alone(**kw):
        a = dict(w=ins[2].ptr, z=ins[3].ptr, R=R, N=N, rho=RHO, loss=dl.ptr, d_w=dd.ptr, ws=dws.ptr, nbytes=int(lib.t2n_distortion_loss_workspace_bytes(R)))
        a.update(kw)
        with torch.cuda.device(dev()):
            return lib.t2n_distortion_loss(a["w"], a["z"], a["R"], a["N"], a["rho"], a["loss"], a["d_w"], a["ws"], a["nbytes"], st)

    for kw in (dict(w=None), dict(z=None), dict(loss=None), dict(ws=None), dict(R=0), dict(N=0), dict(rho=0.0), dict(rho=-1.0),
               dict(rho=float("inf")), dict(rho=float("nan")), dict(ws=C.c_void_p(dws.ptr.value + 4))):
        assert alone(**kw) == ERR_INVALID, kw
    assert alone(nbytes=0) == ERR_WORKSPACE
    torch.cuda.synchronize()
    for b in list(outs.values()) + [dl, dd, dws]:
        got = b.get()
        assert b.guards_intact() and np.all(got == got.dtype.type(SENTINEL)), "an output was written by a refused call"
    # and the same buffers are written by a good call
    assert train() == 0 and alone() == 0
    torch.cuda.synchronize()
    assert all(not np.any(outs[k].get() == SENTINEL) for k in ("losses", "dist")) and dl.get()[0] != SENTINEL


# ---- losses.distortion_loss ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["dense-5x64", "box-301x65"])
def test_distortion_loss_under_autograd(cid):
    from text2nerf_amd import losses
    c = CASES[cid]
    want_l, want_g = ref(cid)
    w = torch.from_numpy(c["w"]).to(dev()).requires_grad_(True)
    z = torch.from_numpy(c["z"]).to(dev())
    loss = losses.distortion_loss(w, z, D.Z_RANGE)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda
    assert abs(float(loss.detach()) - want_l) <= D.loss_bound(c["w"], c["z"], RHO, want_l)
    up = 2.5
    (loss * up).backward()
    got = w.grad.cpu().numpy().astype(np.float64)
    bound = up * D.grad_bound(c["w"], c["z"], RHO, want_g) + 2.0 ** -23 * np.abs(up * want_g)      # (the product rounds once more)
    assert np.all(np.abs(got - up * want_g) <= bound)
    assert z.grad is None
    # no gradient wanted: the loss alone
    with torch.no_grad():
        assert float(losses.distortion_loss(w, z, D.Z_RANGE)) == float(loss.detach())
    with pytest.raises(_lib.T2NError):
        losses.distortion_loss(w.detach().cpu(), z, D.Z_RANGE)
    with pytest.raises(_lib.T2NError):
        losses.distortion_loss(w, z.cpu(), D.Z_RANGE)
    with pytest.raises(_lib.T2NError):
        losses.distortion_loss(w, z, 0.0)


# ---- train_step(distortion=w) -------------------------------------------------------------------------------------------------------------
W_DIST = 0.2
TINY_RANGE = TINY["near_far"][1] - TINY["near_far"][0]


def autograd_step(f, kind, rays, rgb_t, dep_t, w_depth, w_trans, sigma, w_dist, z_range):
    """The autograd route: the renderer under autograd, the driver's loss with the kind's depth term, + w_dist * distortion_loss."""
    from text2nerf_amd import OctreeRender_trilinear_fast, losses
    d = dev()
    rgb, _, depth, w, z = OctreeRender_trilinear_fast(rays, f, chunk=rays.shape[0], N_samples=-1, white_bg=True, is_train=True, device=d)
    rgb_t, dep_t = rgb_t.to(d), dep_t.to(d)
    depth = torch.where(torch.isnan(depth), torch.zeros_like(depth), depth)
    mse = torch.mean((rgb - rgb_t) ** 2)
    tl = losses.TransMittanceLoss_mask()(w, (z - dep_t[:, None] + 0.1) < 0)
    if kind == "mse":
        term = torch.mean((depth - dep_t) ** 2)
    else:
        term = losses.scale_shift_invariant_loss(z, w, dep_t)[0]
    dist = losses.distortion_loss(w, z, z_range)
    for p in f.parameters():
        p.grad = None
    tot = mse + w_depth * term + w_trans * tl + w_dist * dist
    tot.backward()
    return torch.stack([mse, term, tl, tot]).detach(), dist.detach(), (w.detach(), z.detach())


def check_last_distortion(f, w, z, z_range):
    got = f.last_distortion
    assert got.is_cuda and got.dtype == torch.float64 and got.dim() == 0
    w, z = w.cpu().numpy(), z.cpu().numpy()
    want, _ = D.distortion(w, z, 1.0 / z_range)
    assert abs(float(got) - want) <= D.loss_bound(w, z, 1.0 / z_range, want), (float(got), want)
    return want


@pytest.mark.parametrize("form", ["mse", "ssi", "indexed"])
def test_train_step_with_distortion_equals_the_autograd_route(tiny_params, form):
    from text2nerf_amd.dataset import DeviceTrainSet
    rays, rgb_t, dep_t = positive_depth_batch(tiny_params)
    R = rays.shape[0]
    kind = "ssi" if form == "ssi" else "mse"
    w_depth, w_trans, sigma = 0.05, 1e3, 0.1
    fa = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    fb = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    torch.manual_seed(41)
    la, da, (w, z) = autograd_step(fa, kind, rays, rgb_t, dep_t, w_depth, w_trans, sigma, W_DIST, TINY_RANGE)
    seen = {}
    real = fb._render_raw

    def spy(*a, **k):
        out = real(*a, **k)
        seen["z"], seen["w"] = out[2].clone(), out[3].clone()
        return out

    fb._render_raw = spy
    torch.manual_seed(41)
    kw = dict(N_samples=-1, white_bg=True, w_depth=w_depth, w_trans=w_trans, delta=0.1, depth_loss=kind, depth_std=sigma, fused=None,
              distortion=W_DIST)
    if form == "indexed":
        src = DeviceTrainSet(rays, rgb_t, dep_t, device=dev())
        lb = fb.train_step_indexed(src, torch.arange(R), NoStep(), **kw).clone()
    else:
        lb = fb.train_step(rays, rgb_t, dep_t, NoStep(), **kw).clone()
    print(form, "autograd", la.cpu().numpy(), float(da), "train_step", lb.cpu().numpy(), float(fb.last_distortion))
    assert torch.isfinite(lb).all()
    assert torch.allclose(la, lb, rtol=1e-5, atol=1e-9), (la, lb)
    assert fb.__dict__.get("_fused_step") is None
    assert (fb.last_depth_aux is None) == (kind == "mse")
    want = check_last_distortion(fb, seen["w"], seen["z"], TINY_RANGE)
    assert want > 0 and abs(float(da) - want) <= 2e-6 * want
    ref_g = {k: p.grad.detach().cpu().numpy() for k, p in fa.named_parameters()}
    assert len(ref_g) == 19
    worst = _grad_check(fb, ref_g, rel=1e-5)
    print(form, "train_step vs autograd route, max |dg| / max |g|:", {k: f"{v:.1e}" for k, v in worst.items()})


def test_train_step_with_distortion_on_a_general_shape_field():
    """One TVAdam step (no `field=`) of train_step(distortion=w) against the autograd-form step with the same optimiser and draw."""
    from tests.test_generic_train_step_gpu import LOSS_RTOL, _field, _optimizer, _tv
    from tests.helpers import generic_train as T
    from tests.test_train_step import assert_same_trajectory
    case, fa = _field("odd_rows")
    _, fb = _field("odd_rows")
    oa, ob = _optimizer(fa), _optimizer(fb)
    rays = torch.from_numpy(case.rays)
    rgb_t, dep_t = T.targets(case)
    z_range = float(fb.near_far[1]) - float(fb.near_far[0])
    torch.manual_seed(100)
    la, da, _ = autograd_step(fa, "mse", rays, rgb_t, dep_t, 0.005, 1e3, 0.1, W_DIST, z_range)
    oa.step(tv=_tv(fa))
    seen = {}
    real = fb._general_forward

    def spy(*a, **k):
        out = real(*a, **k)
        seen["z"], seen["w"] = out[2].clone(), out[3].clone()
        return out

    fb._general_forward = spy
    torch.manual_seed(100)
    lb = fb.train_step(rays, rgb_t, dep_t, ob, N_samples=-1, white_bg=True, tv=_tv(fb), distortion=W_DIST).clone()
    print("general: autograd", la.cpu().numpy(), float(da), "train_step", lb.cpu().numpy(), float(fb.last_distortion))
    assert torch.allclose(la, lb, rtol=LOSS_RTOL, atol=1e-9), (la, lb)
    z = seen["z"].expand_as(seen["w"]) if seen["z"].shape != seen["w"].shape else seen["z"]
    want = check_last_distortion(fb, seen["w"], z.contiguous(), z_range)
    assert abs(float(da) - want) <= 2e-6 * want
    assert all(int(ob.state[p]["step"]) == 1 for p in fb.parameters())
    assert_same_trajectory(fa, fb, steps=1)


def test_train_step_distortion_keywords(tiny_params, monkeypatch):
    """distortion=0.0 is the call without the keyword; fused=True / graph=True with a weight raise and change nothing; fused=None runs.

    Bit-equal PARAMETERS after optimiser steps cannot be asserted of two calls here, not even of two identical ones: the factor
    gradients are sums of float atomics whose order changes from run to run (tests/test_depth_loss_gpu.py::
    test_train_step_depth_keywords measured it). As there: everything the keyword can reach — the loss tensor and the three upstream
    gradients handed to the backward — is bit-equal with distortion=0.0 and without, neither call reaches t2n_train_loss_dist, the CPU
    generator is left in the same state, `last_distortion` is None, and the parameters after three TVAdam steps on the default route
    agree at assert_same_trajectory's bound for two runs of one path."""
    from text2nerf_amd._lib import T2NError
    from text2nerf_amd.optim import TVAdam
    from tests.test_train_step import assert_same_trajectory, batch
    rays, rgb_t, dep_t = batch()
    new = lambda: make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])      # noqa: E731
    lib = _lib.load()
    called = []
    real_dist = lib.t2n_train_loss_dist
    monkeypatch.setattr(lib, "t2n_train_loss_dist", lambda *a: (called.append(a[13]), real_dist(*a))[1])
    handed = []
    for kw in (dict(), dict(distortion=0.0)):
        f = new()
        real = f._backward_raw

        def spy(rays_, jitter, N, flags, ws, d_rgb, d_depth, d_w, _real=real, **k):
            handed.append([t.clone() for t in (d_rgb, d_depth, d_w)])
            return _real(rays_, jitter, N, flags, ws, d_rgb, d_depth, d_w, **k)

        f._backward_raw = spy
        torch.manual_seed(69)
        handed.append(f.train_step(rays, rgb_t, dep_t, NoStep(), N_samples=-1, white_bg=False, fused=False, **kw).clone())
        handed.append(torch.get_rng_state())
        assert f.last_distortion is None
    assert not called and len(handed) == 6
    for a, b in zip(handed[0] + [handed[1], handed[2]], handed[3] + [handed[4], handed[5]]):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    # the default route, three steps with TVAdam
    fields = [new(), new()]
    opts = [TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f) for f in fields]
    for it in range(3):
        out = []
        for f, o, kw in zip(fields, opts, (dict(), dict(distortion=0.0))):
            torch.manual_seed(70 + it)
            out.append(f.train_step(rays, rgb_t, dep_t, o, N_samples=-1, white_bg=False, tv=[(f.density_plane, 0.1), (f.app_plane, 0.01)], **kw).clone())
            assert f.last_distortion is None
        assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))
    for f in fields:
        fs = f.__dict__.get("_fused_step")
        if fs is not None:
            fs.sync()
    same = all(torch.equal(a, b) for a, b in zip(fields[0].state_dict().values(), fields[1].state_dict().values()))
    print("parameters after 3 steps bit-equal, distortion=0.0 vs omitted:", same)
    assert_same_trajectory(fields[0], fields[1], steps=3)
    assert not called
    # the refusals: nothing has changed afterwards
    f = new()
    o = TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f)
    before = {k: v.detach().clone() for k, v in f.state_dict().items()}
    state = torch.get_rng_state()
    for kw in (dict(fused=True), dict(graph=True), dict(fused=True, graph=True)):
        with pytest.raises(T2NError, match="composed route"):
            f.train_step(rays, rgb_t, dep_t, o, distortion=0.1, **kw)
    with pytest.raises(T2NError, match="distortion"):
        f.train_step(rays, rgb_t, dep_t, o, distortion=-0.1)
    with pytest.raises(T2NError, match="distortion"):
        f.train_step(rays, rgb_t, dep_t, o, distortion=float("nan"))
    torch.cuda.synchronize()
    assert all(torch.equal(v, before[k]) for k, v in f.state_dict().items()) and torch.equal(state, torch.get_rng_state())
    assert not called and not o.state
    # fused=None with a weight: the composed route
    losses = f.train_step(rays, rgb_t, dep_t, o, distortion=0.1, tv=[(f.density_plane, 0.1), (f.app_plane, 0.01)])
    assert called == [pytest.approx(0.1)] and torch.isfinite(losses).all() and f.__dict__.get("_fused_step") is None
    assert f.last_distortion is not None and float(f.last_distortion) > 0
    assert any(not torch.equal(v, before[k]) for k, v in f.state_dict().items())
    # speculative=True carries the term too
    f.train_step(rays, rgb_t, dep_t, o, distortion=0.1, speculative=True)
    assert len(called) == 2 and float(f.last_distortion) > 0


def test_training_with_the_term_lowers_the_distortion_of_held_out_rays(tiny_params):
    """30 steps from equal parameters with and without the term; D of a fixed held-out batch must come out lower with it (a sign check)."""
    from text2nerf_amd import OctreeRender_trilinear_fast, losses
    from text2nerf_amd.optim import TVAdam
    from text2nerf_amd import synth
    from tests.test_train_step import batch
    rays, rgb_t, dep_t = batch()
    held = torch.from_numpy(synth.frame_rays_np(16, 24, c2w=synth.look_pose(0.25, -0.05, (0.2, 0.1, -1.0))))      # a neighbouring view
    result = {}
    for name, w in (("without", 0.0), ("with", 1.0)):
        f = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
        o = TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f)
        torch.manual_seed(7)
        for _ in range(30):
            f.train_step(rays, rgb_t, dep_t, o, N_samples=-1, white_bg=True, fused=False, distortion=w)
        torch.manual_seed(8)
        with torch.no_grad():
            _, _, _, wts, z = OctreeRender_trilinear_fast(held, f, chunk=held.shape[0], N_samples=-1, white_bg=True, is_train=True, device=dev())
            result[name] = float(losses.distortion_loss(wts, z, TINY_RANGE))
    print("held-out D after 30 steps:", result)
    assert result["with"] < result["without"]
