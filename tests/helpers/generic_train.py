"""Shared pieces of the general-shape backward / train_step tests (csrc/t2n_generic_bwd.hip, TensorVMSplit.train_step on a general-shape
field): the Python restatement of t2n_generic_backward_plan (kernel form, passes, scratch bytes), the seeded batch targets of a case,
and the float64 reference step — generic_cases.oracle(requires_grad=True), the driver's loss as a torch expression (the formulae of
tests/helpers/optim_ref.py::driver_loss), optional TV terms (oracle_torch.tv_loss, weighted as TVAdam.step weighs them) — computed once
per (case, dtype, TV weights) and shared, read-only, by the tests that need it."""
import functools

import numpy as np
import torch

from oracle import oracle_torch as O
from tests.helpers import generic_cases as G

W_DEPTH, W_TRANS, DELTA = 0.005, 1e3, 0.1          # the driver's weights (text2nerf_main.py:547-590), train_step's defaults
PASS_ROWS_DEFAULT = 262144                         # genb_pass_rows: pass_rows = 0
COL_CHUNKS = 128                                   # kColChunks
MAT0, MAT1, VECM = (0, 0, 1), (1, 2, 2), (2, 1, 0)  # plane k is [C, grid[MAT1[k]], grid[MAT0[k]]], line k is [C, grid[VECM[k]]]

# the cases of the GPU tests
GRAD_CASES = ["odd_rows", "rows64", "mlp_view", "tiny_head", "sh_odd", "rgb_odd", "fuzz11", "fuzz5", "fuzz17"]
FALLBACK_CASES = ["valu_in520", "plain", "fuzz8"]
STEP_CASES = ["odd_rows", "rows64", "sh_odd", "fuzz11", "valu_in520"]
TV_WEIGHTS = (0.1, 0.01)                           # (density planes, appearance planes), as tests/test_train_step.py's first step


def _a256(n):
    return (n + 255) // 256 * 256


def tn_plan(rows, N):
    """tn_plan of csrc/t2n_bwd_mlp.hip: (chunk_rows, chunks, ng, ldp)."""
    ng = (N + 127) // 128
    c = (rows * ng + 511) // 512
    c = max(64, (c + 31) // 32 * 32)
    return c, max(1, (rows + c - 1) // c), ng, ng * 128


def kernel_form(kw):
    """genb_kernel_form (no environment switch set): the forward ran staged, and the head is SH, RGB or an MLP with <= 512 inputs."""
    if G.head_lds_bytes(kw) > G.LDS_LIMIT:
        return 0
    if kw["shadingMode"] in G.MLP_HEADS:
        return int(G.in0_of(kw) <= G.ROWS_IN_MAX)
    return int(kw["shadingMode"] in ("SH", "RGB"))


def backward_plan(kw, grid, R, N, pass_rows=0):
    """t2n_generic_backward_plan restated: dict(kernel_form, pass_rows, max_passes, workspace_bytes)."""
    tot = R * N
    tot64 = (tot + 63) // 64 * 64
    pr = min((pass_rows + 63) // 64 * 64 if pass_rows else PASS_ROWS_DEFAULT, tot64)
    out = dict(kernel_form=kernel_form(kw), pass_rows=pr, max_passes=(tot + pr - 1) // pr, workspace_bytes=0)
    if not out["kernel_form"]:
        return out
    o = 0
    for q in range(4):                               # the channel-last gradient copies: density planes, lines, appearance planes, lines
        for k in range(3):
            C = (kw["density_n_comp"] if q < 2 else kw["appearance_n_comp"])[k]
            pos = grid[VECM[k]] if q & 1 else grid[MAT1[k]] * grid[MAT0[k]]
            o += _a256(pos * C * 4)
    mlp = kw["shadingMode"] in G.MLP_HEADS
    fc = kw["featureC"] if mlp else 0
    D, in0, ncol = kw["app_dim"], G.in0_of(kw), sum(kw["appearance_n_comp"])
    o += _a256(max(ncol, fc, in0) * 4)               # the zero bias
    o += _a256(tot * 4) + _a256(out["max_passes"] * 4)
    ldg, ldgf, ldX = (fc + 127) // 128 * 128, 32 if D <= 32 else 128, (ncol + 15) // 16 * 16
    if mlp:
        o += _a256(fc * fc * 4) + _a256(fc * in0 * 4) + _a256(pr * 32 * 4) + 2 * _a256(pr * ldg * 4) + _a256(pr * ((in0 + 15) // 16 * 16) * 4)
    o += _a256(ncol * D * 4) + _a256(pr * ldgf * 4) + 2 * _a256(pr * ldX * 4)
    part = 0
    for n in (fc, in0, ncol):
        if n > 0:
            _, chunks, _, ldp = tn_plan(pr, n)
            part = max(part, chunks * 128 * ldp * 4)
    o += _a256(part) + _a256(COL_CHUNKS * max(fc, 32) * 4)
    out["workspace_bytes"] = o
    return out


def targets(case):
    """Seeded batch targets of a case's rays: rgb ~ U[0, 1], depth ~ U[1, 5] (float32)."""
    g = np.random.Generator(np.random.PCG64(case.seed0 + 11))
    return (torch.from_numpy(g.uniform(0.0, 1.0, (case.R, 3)).astype(np.float32)),
            torch.from_numpy(g.uniform(1.0, 5.0, (case.R,)).astype(np.float32)))


def driver_loss_torch(rgb, depth, w, z, rgb_t, dep_t, w_depth=W_DEPTH, w_trans=W_TRANS, delta=DELTA):
    """optim_ref.driver_loss's formulae as a differentiable torch expression: (mse, depth loss, transmittance loss, total)."""
    depth = torch.where(torch.isnan(depth), torch.zeros_like(depth), depth)
    mse = ((rgb - rgb_t) ** 2).mean()
    dl = ((depth - dep_t) ** 2).mean()
    mask = ((z - dep_t[:, None]) + delta) < 0
    m = (w * mask).sum(1) / w.shape[1]
    tl = (m * m).mean()
    return mse, dl, tl, mse + w_depth * dl + w_trans * tl


def tv_terms(P, tv_weights):
    """What TVAdam.step(tv=[(density_plane, wd), (app_plane, wa)]) adds to the loss: sum_planes w * 1e-2 * TVLoss(plane)."""
    wd, wa = tv_weights
    return sum(O.tv_loss(P[f"density_plane.{k}"]) * 1e-2 * wd for k in range(3)) + sum(O.tv_loss(P[f"app_plane.{k}"]) * 1e-2 * wa for k in range(3))


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(case, params at seed0, mask volume or None)."""
    case = G.case_by_name(name)
    params = G.make_params(case, case.seed0)
    return case, params, (G.mask_volume(case, params) if case.mask else None)


@functools.lru_cache(maxsize=None)
def reference_step(name, dtype=torch.float64, tv_weights=None):
    """The reference step of a case at seed0, whole frame, train mode: dict(grads {name: array}, losses [4], rgb, depth, w, z). Cached:
    treat the arrays as read-only."""
    case, params, vol = case_inputs(name)
    (rgb, depth, z, w), P = G.oracle(case, params, True, dtype=dtype, vol=vol, requires_grad=True)
    rgb_t, dep_t = (t.to(dtype) for t in targets(case))
    mse, dl, tl, tot = driver_loss_torch(rgb, depth, w, z.to(dtype), rgb_t, dep_t)
    full = tot + tv_terms(P, tv_weights) if tv_weights is not None else tot
    if full.requires_grad:
        full.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach().numpy().astype(np.float64) for k, v in P.items()}
    return dict(grads=grads, losses=np.array([float(v.detach()) for v in (mse, dl, tl, tot)]), rgb=rgb.detach().numpy(),
                depth=depth.detach().numpy(), w=w.detach().numpy(), z=z.detach().numpy())


def max_rel(got, ref):
    """Per tensor max |got - ref| / max |ref| (the measure of tests/test_hip_parity.py::_grad_check)."""
    return {k: float(np.abs(np.asarray(got[k], np.float64).reshape(g.shape) - g).max()) / (float(np.abs(g).max()) + 1e-12) for k, g in ref.items()}
