"""Element-by-element reference for the gradients of the seven head tensors (basis_mat.weight and the three Linear layers of
renderModule.mlp), computed on the CPU from oracle_torch only. The head half of tests/helpers/grad_elementwise.py, same design.

`_grad_check` bounds max |dg| / max |g| per tensor: an element worth 1e-3 of its tensor's maximum (a high-octave encoding column of
mlp.0.weight, a row whose hidden unit is rarely active, a basis_mat column of a sparse component) may be 50 % wrong and pass. Here
every element has a bound of its own, built from per-row quantities of the oracle's head over the appearance rows r:

    x144 [rows,144] the factor products, f = x144 basis^T [rows,27], x [rows,K0] = the head's input columns (f, its encoding, for a
    view-dependent head also the view direction and its encoding), h0 = relu(x W0^T + b0), h1 = relu(h0 W1^T + b1),
    go = dL/d(h1 W2^T + b2) (= ray weight * dL/drgb * sigmoid'), g1 = (go W2) [h1 > 0], g0 = (g1 W1) [h0 > 0], gx = g0 W0,
    gf = gx's feature columns + the encoding's chain rule.

    dW2 = go^T h1, dW1 = g1^T h0, dW0 = g0^T x, dbasis = gf^T x144, biases = column sums of go / g1 / g0.

The helper restates the head (`head_rows`) with the oracle's own expressions under autograd, seeded with the oracle run's dL/drgb per
row; tests/test_head_grad_elementwise_cpu.py pins its seven gradients to the oracle's bit for bit in float64.

* `A_e`: the absolute-contribution sum. The same network with every weight, activation and upstream replaced by its absolute value,
  same ReLU masks, |sin| / |cos| as the encoding's derivative factors: G1 = (|go| |W2|) [h1 > 0], G0 = (G1 |W1|) [h0 > 0],
  Gx = G0 |W0|, Gf likewise; A(W2) = |go|^T h1, A(W1) = G1^T h0, A(W0) = G0^T |x|, A(basis) = Gf^T |x144|, biases the column sums.
  A_e >= |g_e|, A_e bounds every partial sum any summation order or split product can form, and A_e == 0 exactly where no row
  contributes (a colour channel without upstream, a hidden unit that is never active).
* `Nm_e`: the float32 noise. The same sums with one factor replaced by the float32-minus-float64 difference of that per-row quantity,
  sum_r |dg_ri| |x_rj| + G_ri |dx_rj| (|x| and G the larger of the two runs'), over the rows both oracles list; the sin / cos
  columns of x carry 4.2e-7 more, the absolute error of the hardware sine the kernels recompute the encoding with
  (csrc/t2n_gemm_h.hip, comment at k_gemm_tn_b).
* Knife edges, as in grad_elementwise.reference(): float64 runs with the list threshold at thres -+ KNIFE and with every ReLU switching
  at -+ RELU_KNIFE state what a row that may be listed or not, or a hidden unit that may switch, changes; the same formula on (that run
  - the base run) adds the affected rows' exact change to Nm_e, and A_e is the elementwise maximum over the base run and the two runs
  that list / switch on more (so `A_e == 0` holds for every such kernel too).

* Forward rounding (added after the first GPU run). `A_e` multiplies each row gradient with the VALUE of an activation, but the
  default forward forms that value from split-f16 products (csrc/t2n_mlp_ss.hip: x = hi + lo, hi = RTZ_f16(x), lo = RTZ_f16(x - hi),
  activations split unscaled where they are produced, the lo * lo term dropped), whose error is relative to the absolute products, not
  to a cancelled sum, and has an absolute floor: for |x| < 2^-3 the residual x - hi is an f16 subnormal, spaced 2^-24. The finding:
  W0[20, 10] of the 255 - 257 row cases has ONE contributing row, whose raw feature 10 is 1.67e-4 (144 products, absolute sum 0.039);
  the default routes were 3.0e-8 off in that feature — the same 1.79e-4 relative error of the element under two different losses,
  42 and 47 times the bound without this term — and the exact-fp32 route met the bound at 0.44. Per operand value v of a product the
  split's error is o(v)^2 = (2^-24)^2 + (2^-22 v)^2; independent errors add in quadrature (K's factor 8 is the margin over that):
      df^2 = o(x144)^2 basis^2^T,  dx^2 = df^2 on the raw columns and 4^o df^2 on octave o's sin / cos columns,
      dh0^2 = [h0 > 0] (o(x)^2 + dx^2) W0^2^T,  dh1^2 likewise from h0, dh0,  dp2^2 likewise from h1, dh1,
      dgo = |go| dp2 (|d log sigmoid'| <= 1), propagated the same way to dG1, dG0, dGx, dGf
  and Nm_e gains sum_r dG_ri |x_rj| + G_ri dx_rj (rows add linearly). A one-draw float32-minus-float64 difference cannot stand for
  this: on an element that one or two rows reach it may be near zero by chance.

    bound_e = 2^-22 * A_e + Nm_e,   K = 8 * max(1, rho32),   rho32 = max_e |g32_e - g64_e| / bound_e

rho32 is measured on the CPU from the float32 oracle, never from a kernel; the 8 has grad_elementwise.py's meaning (the dropped lo * lo
term of the split products, another summation order). `check(got, ref, K)`: |got - g64| <= K * bound per element, got == 0 exactly
where A_e == 0. g64 = float64 arithmetic on the float32 sample geometry, g32 = the plain float32 oracle; numpy float64 by name.

A uniform power-of-two factor on dL/drgb scales g64, g32, A, Nm and therefore the bound exactly (`Reference.scaled`): the range cases
reuse one reference."""
from dataclasses import dataclass, field, replace
from typing import Dict

import numpy as np
import torch

from oracle import oracle_torch as O
from tests.helpers.grad_elementwise import KNIFE, RELU_KNIFE

W0, B0, W1, B1, W2, B2, BASIS = ("renderModule.mlp.0.weight", "renderModule.mlp.0.bias", "renderModule.mlp.2.weight",
                                 "renderModule.mlp.2.bias", "renderModule.mlp.4.weight", "renderModule.mlp.4.bias", "basis_mat.weight")
HEAD_KEYS = (BASIS, W0, B0, W1, B1, W2, B2)
SIN_HW = 4.2e-7        # absolute error of the kernels' hardware sine on the reduced argument (csrc/t2n_gemm_h.hip)
ROW_KEYS = ("x144", "x", "h0", "h1", "go", "g1", "g0", "gx", "gf")       # the per-row quantities head_rows returns


def layout(cfg, app_dim=27):
    """Column layout of the head's input x: (K0, first column of the feature encoding's sines, octaves of it)."""
    if cfg.shading_mode == "MLP_Fea_noview":
        return app_dim * (1 + 2 * cfg.fea_pe), app_dim, cfg.fea_pe
    if cfg.shading_mode == "MLP_Fea":
        return app_dim * (1 + 2 * cfg.fea_pe) + 3 * (1 + 2 * cfg.view_pe), app_dim + 3, cfg.fea_pe
    raise NotImplementedError(cfg.shading_mode)


def _input_columns(cfg, feat, viewdirs):
    """oracle_torch.mlp_fea_noview / mlp_view_head's torch.cat, restated."""
    if cfg.shading_mode == "MLP_Fea_noview":
        return torch.cat([feat, O.positional_encoding(feat, cfg.fea_pe)], -1) if cfg.fea_pe > 0 else feat
    cols = [feat, viewdirs]
    if cfg.fea_pe > 0:
        cols.append(O.positional_encoding(feat, cfg.fea_pe))
    if cfg.view_pe > 0:
        cols.append(O.positional_encoding(viewdirs, cfg.view_pe))
    return torch.cat(cols, -1)


def head_rows(cfg, params, dtype, xn, viewdirs, dc, relu_shift=None):
    """The head restated over the rows of one oracle run: xn [M,3] the rows' normalised coordinates, viewdirs [M,3], dc [M,3] =
    dL/d(colour) of the run. Returns (grads of the seven tensors, per-row quantities by ROW_KEYS), float64 numpy."""
    P = O.params_from_numpy(params, dtype=dtype)
    P = {k: v.requires_grad_(k in HEAD_KEYS) for k, v in P.items()}
    M = int(xn.shape[0])
    app_dim, n_comp = P[BASIS].shape
    if M == 0:
        K0 = P[W0].shape[1]
        z = lambda *s: np.zeros(s, np.float64)    # noqa: E731
        return ({k: z(*P[k].shape) for k in HEAD_KEYS},
                dict(x144=z(0, n_comp), x=z(0, K0), h0=z(0, 128), h1=z(0, 128), go=z(0, 3), g1=z(0, 128), g0=z(0, 128), gx=z(0, K0), gf=z(0, app_dim)))

    def act(p):
        return torch.relu(p) if relu_shift is None else p * (p > relu_shift).to(p.dtype)

    with torch.no_grad():
        x144 = O.app_feature({**P, BASIS: torch.eye(n_comp, dtype=dtype)}, xn)
    f = O.app_feature(P, xn)
    x = _input_columns(cfg, f, viewdirs)
    p0 = x @ P[W0].T + P[B0]
    h0 = act(p0)
    p1 = h0 @ P[W1].T + P[B1]
    h1 = act(p1)
    p2 = h1 @ P[W2].T + P[B2]
    c = torch.sigmoid(p2)
    for t in (f, x, p0, p1, p2):
        t.retain_grad()
    torch.autograd.backward([c], [dc.to(dtype)])
    n = lambda t: t.detach().numpy().astype(np.float64)       # noqa: E731
    rows = dict(x144=n(x144), x=n(x), h0=n(h0), h1=n(h1), go=n(p2.grad), g1=n(p1.grad), g0=n(p0.grad), gx=n(x.grad), gf=n(f.grad))
    return {k: n(P[k].grad) for k in HEAD_KEYS}, rows


def _run(cfg, params, rays, jitter, n_samples, loss, dtype, geom_dtype, thres=None, relu_shift=None):
    """One oracle forward + backward (train mode, white background) with `shade` wrapped: the gradients of all 19 tensors, the lists,
    and the restated head's per-row quantities of this run. A batch without appearance rows is fine."""
    from tests.helpers.grad_elementwise import _mlp_layers_shifted
    P = O.params_from_numpy(params, dtype=dtype, requires_grad=True)
    seen = []
    orig_shade, orig_app, orig_t, orig_m = O.shade, O.app_feature, cfg.ray_march_weight_thres, O._mlp_layers

    def shade(cfg_, p, viewdirs, feat, pts=None, pre=None):
        out = orig_shade(cfg_, p, viewdirs, feat, pts=pts, pre=pre)
        out.retain_grad()
        seen.append((viewdirs.detach(), out))
        return out

    def app_feature(p, xyz_norm):
        seen_xn.append(xyz_norm.detach())
        return orig_app(p, xyz_norm)

    seen_xn = []
    O.shade, O.app_feature = shade, app_feature
    try:
        if thres is not None:
            cfg.ray_march_weight_thres = thres
        if relu_shift is not None:
            O._mlp_layers = _mlp_layers_shifted(relu_shift)
        rgb, depth, z, w, aux = O.forward(cfg, P, rays, white_bg=True, is_train=True, n_samples=n_samples, jitter=jitter,
                                          return_aux=True, geom_dtype=geom_dtype)
        value = loss(rgb, depth, z, w)
        value.backward()
    finally:
        O.shade, O.app_feature, cfg.ray_march_weight_thres, O._mlp_layers = orig_shade, orig_app, orig_t, orig_m
    grads = {k: (v.grad.numpy().astype(np.float64) if v.grad is not None else np.zeros(tuple(v.shape), np.float64)) for k, v in P.items()}
    mask = aux["app_mask"]
    if seen:
        (vd, out), xn = seen[0], seen_xn[0]
        dc = out.grad if out.grad is not None else torch.zeros_like(out)
    else:
        vd, xn, dc = torch.zeros(0, 3), torch.zeros(0, 3), torch.zeros(0, 3, dtype=dtype)
    hg, rows = head_rows(cfg, params, dtype, xn, vd, dc.detach(), relu_shift)
    return dict(grads=grads, head=hg, rows=rows, app_mask=mask, valid=aux["valid"], z=z.detach(), loss=float(value.detach()),
                relu_pre=aux["relu_pre"] or [])


def absolute_rows(cfg, params, rows):
    """The absolute network's row gradients G1, G0, Gx, Gf and |go| of per-row quantities (float64)."""
    P = {k: np.abs(np.asarray(params[k], np.float64)) for k in HEAD_KEYS}
    K0, s0, pe = layout(cfg, P[BASIS].shape[0])
    D = P[BASIS].shape[0]
    ago = np.abs(rows["go"])
    G1 = (ago @ P[W2]) * (rows["h1"] != 0)
    G0 = (G1 @ P[W1]) * (rows["h0"] != 0)
    Gx = G0 @ P[W0]
    Gf = Gx[:, :D].copy()
    if pe > 0 and Gx.shape[0]:
        bands = 2.0 ** np.arange(pe)
        sin = np.abs(rows["x"][:, s0:s0 + D * pe]).reshape(-1, D, pe)
        cos = np.abs(rows["x"][:, s0 + D * pe:s0 + 2 * D * pe]).reshape(-1, D, pe)
        Gs = Gx[:, s0:s0 + D * pe].reshape(-1, D, pe)
        Gc = Gx[:, s0 + D * pe:s0 + 2 * D * pe].reshape(-1, D, pe)
        Gf += ((Gs * cos + Gc * sin) * bands).sum(-1)
    return dict(go=ago, g1=G1, g0=G0, gx=Gx, gf=Gf)


def _sums(G, X):
    """The seven tensors' sums from row gradients G (go, g1, g0, gf) and row inputs X (h1, h0, x, x144), all >= 0."""
    return {W2: G["go"].T @ X["h1"], B2: G["go"].sum(0), W1: G["g1"].T @ X["h0"], B1: G["g1"].sum(0), W0: G["g0"].T @ X["x"],
            B0: G["g0"].sum(0), BASIS: G["gf"].T @ X["x144"]}


def absolute_sums(cfg, params, rows):
    return _sums(absolute_rows(cfg, params, rows), {k: np.abs(rows[k]) for k in ("h1", "h0", "x", "x144")})


def noise(cfg, params, base, alt, keep=None, sin_hw=0.0):
    """sum_r |dg_ri| |x_rj| + G_ri |dx_rj| for the seven tensors, d = alt - base over the same rows (`keep`: only these rows), |x| and
    the absolute network's G the larger of the two runs'; `sin_hw`: added to |dx| on the encoding's sin / cos columns."""
    if keep is not None:
        base, alt = ({k: v * keep[:, None] for k, v in r.items()} for r in (base, alt))
    Ga, Gb = absolute_rows(cfg, params, base), absolute_rows(cfg, params, alt)
    G = {k: np.maximum(Ga[k], Gb[k]) for k in Ga}
    X = {k: np.maximum(np.abs(base[k]), np.abs(alt[k])) for k in ("h1", "h0", "x", "x144")}
    dG = {k: np.abs(alt[k] - base[k]) for k in ("go", "g1", "g0", "gf")}
    dX = {k: np.abs(alt[k] - base[k]) for k in ("h1", "h0", "x", "x144")}
    if sin_hw:
        K0, s0, pe = layout(cfg, base["gf"].shape[1])
        live = (np.abs(base["go"]).sum(1) > 0) if keep is None else (keep > 0)
        dX["x"][:, s0:s0 + 2 * base["gf"].shape[1] * pe] += sin_hw * live[:, None]
    a, b = _sums(dG, X), _sums(G, dX)
    out = {k: a[k] + b[k] for k in a}
    for k in (B0, B1, B2):       # (a bias has no second factor)
        out[k] = a[k]
    return out


F16_STEP = 2.0 ** -24       # spacing of the f16 subnormals: the absolute floor of an unscaled hi / lo split (lo = RTZ_f16(x - hi))


def forward_noise(cfg, params, rows, eps=2.0 ** -22, floor=F16_STEP):
    """What the rounding of the FORWARD's split products adds to the seven sums (module docstring, "Forward rounding"). Errors of the
    products of one dot product, and of the layers behind one another, are independent and add in quadrature; rows add linearly."""
    P = {k: np.asarray(params[k], np.float64) ** 2 for k in HEAD_KEYS}
    D = P[BASIS].shape[0]
    K0, s0, pe = layout(cfg, D)
    G = absolute_rows(cfg, params, rows)
    X = {k: np.abs(rows[k]) for k in ("h1", "h0", "x", "x144")}
    m0, m1 = rows["h0"] != 0, rows["h1"] != 0
    own = lambda v: floor ** 2 + (eps * v) ** 2                          # noqa: E731  (one operand's split error, squared)
    df2 = own(X["x144"]) @ P[BASIS].T
    dx2 = np.zeros_like(X["x"])
    dx2[:, :D] = df2
    bands2 = 4.0 ** np.arange(pe)
    enc = (df2[:, :, None] * bands2).reshape(df2.shape[0], D * pe)       # |d sin(f 2^o)| <= 2^o |df|, feature-major like the encoding
    dx2[:, s0:s0 + D * pe] = enc
    dx2[:, s0 + D * pe:s0 + 2 * D * pe] = enc
    dh02 = m0 * ((own(X["x"]) + dx2) @ P[W0].T)
    dh12 = m1 * ((own(X["h0"]) + dh02) @ P[W1].T)
    dp22 = (own(X["h1"]) + dh12) @ P[W2].T
    dgo2 = rows["go"] ** 2 * dp22                                        # |d log sigmoid'(p) / dp| = |1 - 2 sigmoid(p)| <= 1
    dG12 = (dgo2 @ P[W2]) * m1
    dG02 = (dG12 @ P[W1]) * m0
    dGx2 = dG02 @ P[W0]
    both = lambda g: (g[:, s0:s0 + D * pe] + g[:, s0 + D * pe:s0 + 2 * D * pe]).reshape(-1, D, pe)      # noqa: E731
    dGf2 = dGx2[:, :D] + (both(dGx2) * bands2).sum(-1) + (both(G["gx"] ** 2) * bands2 * bands2).sum(-1) * df2
    r = np.sqrt
    a = _sums(dict(go=r(dgo2), g1=r(dG12), g0=r(dG02), gf=r(dGf2)), X)
    b = _sums(G, dict(h1=r(dh12), h0=r(dh02), x=r(dx2), x144=eps * X["x144"]))
    out = {k: a[k] + b[k] for k in a}
    for k in (B0, B1, B2):
        out[k] = a[k]
    return out


@dataclass
class Reference:
    g64: Dict[str, np.ndarray]        # all 19 tensors
    g32: Dict[str, np.ndarray]        # all 19 tensors
    A: Dict[str, np.ndarray]          # the 7 head tensors from here on
    Nm: Dict[str, np.ndarray]
    bound: Dict[str, np.ndarray]
    rho32: float
    rho32_key: Dict[str, float]
    rows64: Dict[str, np.ndarray] = field(repr=False)     # per-row quantities of the float64 run, rows in list order
    rows32: Dict[str, np.ndarray] = field(repr=False)
    head64: Dict[str, np.ndarray] = field(repr=False)     # the restated head's gradients of the float64 run
    z: np.ndarray = field(repr=False)
    valid: np.ndarray = field(repr=False)
    app_mask: np.ndarray = field(repr=False)
    app_window: np.ndarray = field(repr=False)
    relu_window: int
    loss: float

    def K(self, factor=8.0):
        return factor * max(1.0, self.rho32)

    @property
    def rows(self):
        return int(self.app_mask.sum())

    def scaled(self, s):
        """The reference of the same case with dL/drgb times the power of two `s`: exact for the head tensors (they see the loss through
        the colour only); g64 / g32 of the twelve factor tensors are NOT carried over (they also see depth and weights)."""
        m = lambda d: {k: v * s for k, v in d.items() if k in HEAD_KEYS}      # noqa: E731
        rs = lambda r: {k: (v * s if k[0] == "g" else v) for k, v in r.items()}      # noqa: E731
        return replace(self, g64=m(self.g64), g32=m(self.g32), A=m(self.A), Nm=m(self.Nm), bound=m(self.bound), rows64=rs(self.rows64),
                       rows32=rs(self.rows32), head64=m(self.head64), loss=float("nan"))


def _on(union, mask, rows):
    """Per-row quantities of a run with list `mask` placed on the rows of `union` (zero where the run does not list the row)."""
    sel = mask[union].numpy()
    out = {}
    for k, v in rows.items():
        o = np.zeros((sel.shape[0], v.shape[1]), np.float64)
        o[sel] = v
        out[k] = o
    return out


def reference(cfg, params, rays, jitter, n_samples, loss):
    """The element-wise head reference of one case (train mode, white background). `loss`: callable on (rgb, depth, z, w) that works
    on oracle tensors of either precision."""
    rays = torch.as_tensor(rays, dtype=torch.float32)
    jitter = torch.as_tensor(jitter, dtype=torch.float32)
    thres = float(cfg.ray_march_weight_thres)
    args = (cfg, params, rays, jitter, n_samples, loss)
    r64 = _run(*args, torch.float64, torch.float32)
    rlo = _run(*args, torch.float64, torch.float32, thres=thres - KNIFE)
    rhi = _run(*args, torch.float64, torch.float32, thres=thres + KNIFE)
    r32 = _run(*args, torch.float32, None)
    rel = [_run(*args, torch.float64, torch.float32, relu_shift=sh) for sh in (-RELU_KNIFE, RELU_KNIFE)]
    for r in rel:
        assert torch.equal(r["app_mask"], r64["app_mask"])
    for r in [rlo, rhi, r32] + rel:
        assert torch.equal(r["valid"], r64["valid"]) and torch.equal(r["z"], r64["z"]), "sample sets of the oracle runs differ"
    U = rlo["app_mask"]
    assert bool((r64["app_mask"] <= U).all()) and bool((rhi["app_mask"] <= r64["app_mask"]).all())
    assert bool((r32["app_mask"] <= U).all()) and bool((rhi["app_mask"] <= r32["app_mask"]).all()), \
        "the float32 oracle's appearance list leaves the knife-edge window"
    base = _on(U, r64["app_mask"], r64["rows"])
    both = (r64["app_mask"] & r32["app_mask"])[U].numpy().astype(np.float64)
    Nm = noise(cfg, params, base, _on(U, r32["app_mask"], r32["rows"]), keep=both, sin_hw=SIN_HW)
    A = absolute_sums(cfg, params, base)
    for k, v in forward_noise(cfg, params, base).items():
        Nm[k] = Nm[k] + v
    for r in (rlo, rhi, rel[0], rel[1]):
        alt = _on(U, r["app_mask"], r["rows"])
        for k, v in noise(cfg, params, base, alt).items():
            Nm[k] = Nm[k] + v
        if r is rlo or r is rel[0]:
            for k, v in absolute_sums(cfg, params, alt).items():
                A[k] = np.maximum(A[k], v)
    g64, g32 = r64["grads"], r32["grads"]
    bound = {k: 2.0 ** -22 * A[k] + Nm[k] for k in HEAD_KEYS}
    rho = {k: _max_ratio(g32[k] - g64[k], bound[k], A[k] > 0) for k in HEAD_KEYS}
    return Reference(g64=g64, g32=g32, A=A, Nm=Nm, bound=bound, rho32=max(rho.values()), rho32_key=rho, rows64=r64["rows"], rows32=r32["rows"],
                     head64=r64["head"], z=r64["z"].numpy(), valid=r64["valid"].numpy(), app_mask=r64["app_mask"].numpy(),
                     app_window=(U & ~rhi["app_mask"]).numpy(),
                     relu_window=int(sum(int((p.abs() < RELU_KNIFE).sum()) for p in r64["relu_pre"])), loss=r64["loss"])


def _max_ratio(err, bound, live):
    return float((np.abs(err)[live] / bound[live]).max()) if live.any() else 0.0


def _as_np(x, shape):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x.astype(np.float64).reshape(shape)


def short(key):
    return key.replace("renderModule.mlp.", "mlp").replace(".weight", ".w").replace(".bias", ".b").replace("basis_mat", "basis")


def ratios(got, ref):
    """max |got - g64| / bound over the elements with A_e > 0, per head tensor (for information: what a run observed)."""
    return {k: _max_ratio(_as_np(got[k], ref.g64[k].shape) - ref.g64[k], ref.bound[k], ref.A[k] > 0) for k in HEAD_KEYS}


def failures(got, ref, K):
    """The elements that miss the check, as a list of report lines (empty: passed)."""
    lines = []
    for k in HEAD_KEYS:
        h = _as_np(got[k], ref.g64[k].shape)
        err = np.abs(h - ref.g64[k])
        live = ref.A[k] > 0
        for what, bad in (("beyond K * bound", live & ~(err <= K * ref.bound[k])), ("non-zero where no row contributes", ~live & (h != 0))):
            n = int(bad.sum())
            if not n:
                continue
            score = np.where(bad, np.nan_to_num(err / np.maximum(ref.bound[k], 1e-300), nan=np.inf) if what[0] == "b" else np.abs(h), -1.0)
            idx = np.unravel_index(int(score.argmax()), score.shape)
            a = float(ref.A[k][idx])
            lines.append(f"{k}: {n} element(s) {what}; worst at {tuple(int(i) for i in idx)} got {h[idx]:.6e} want {ref.g64[k][idx]:.6e} "
                         f"err/bound {float(err[idx] / max(ref.bound[k][idx], 1e-300)):.3g} err/A {float(err[idx] / a) if a else float('inf'):.3g}")
    return lines


def check(got, ref, K):
    """|got - g64| <= K * bound element by element and got == 0 exactly where A_e == 0, for the seven head tensors. `got`: gradients by
    state_dict name (tensors or arrays). Returns the observed max err / bound per tensor."""
    lines = failures(got, ref, K)
    assert not lines, f"head gradients miss the element-wise check at K = {K:.3g}:\n" + "\n".join(lines)
    return ratios(got, ref)
