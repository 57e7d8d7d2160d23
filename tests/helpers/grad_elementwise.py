"""Element-by-element reference for the factor gradients (the 12 plane / line tensors), computed on the CPU from oracle_torch only.

The whole-tensor metrics of `_grad_check` (max |h - g| / max |g| and friends) let an element whose own gradient is a small fraction of
its tensor's maximum be wrong by 100 %. Here every element gets a bound of its own, from two scales the oracle can state per element:

* `A_e`: the sum of the ABSOLUTE contributions of all samples to element e (the lookups are multilinear with non-negative weights, so
  differentiating `sum |upstream| * lookup(|params|)` w.r.t. |params| yields exactly that). `A_e >= |g_e|`, and `A_e == 0` iff no
  sample touches e.
* `Nm_e`: the same sum with the upstream replaced by `delta`, the largest float32-against-float64 difference of the upstream gradient
  over the samples of the sample's ray: what float32 arithmetic in front of the scatter (head, compositing) moves the upstream by.

    bound_e = 2^-22 * A'_e + Nm'_e,      X' = X + 2^-20 * dilate(X)

with dilate = the 3x3 maximum over a plane's spatial axes / the 3-maximum along a line: a sample within an ulp of a cell boundary may
touch one texel more in a kernel than in the reference. `check(got, ref, K)` asserts |got - g64| <= K * bound element by element and
got == 0 exactly wherever dilate(A) == 0 (stray writes). K = 8 * max(1, rho32) with rho32 = max_e |g32 - g64| / bound_e, the float32
oracle's own ratio (measured on the CPU, never on a kernel): the 8 covers the backward's split-f16 products (dropped lo * lo term,
2^-21 = 8 * 2^-24 of a row's maximum) and another scan / summation order.

Two knife edges belong to the noise as well (reference() has the reasoning): an appearance sample whose weight lies within float32
rounding of the 1e-4 list threshold, and a hidden unit of the head whose pre-activation lies within the split-f16 products' rounding of
zero, may go either way in a float32 implementation. Extra float64 runs with the threshold / the ReLU switch moved to either side of
the window give the exact change of every sample's upstream; it is added to that sample's delta.

g64 = float64 arithmetic on the reference's own float32 sample geometry (oracle_torch.forward(geom_dtype=float32)); g32 = the plain
float32 oracle. Everything returned is numpy float64 by state_dict name."""
from dataclasses import dataclass, field
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle_torch as O

FACTOR_KEYS = tuple(f"{q}_{s}.{k}" for q in ("density", "app") for s in ("plane", "line") for k in range(3))
KINDS = ("density_plane", "density_line", "app_plane", "app_line")
BLOCK_EDGE = {"density": 15, "app": 16}     # cells per density block edge / texels per appearance tile edge (csrc/t2n_backward.h)


def kind_of(key):
    return key.split(".")[0]


def dilate(x):
    """3x3 maximum over the two spatial axes of a plane [1,C,H,W]; 3-maximum along a line [1,C,L,1]. numpy in, numpy out."""
    t = torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64)
    if t.shape[-1] == 1:
        return F.max_pool2d(t, kernel_size=(3, 1), stride=1, padding=(1, 0)).numpy()
    return F.max_pool2d(t, kernel_size=3, stride=1, padding=1).numpy()


@dataclass
class Reference:
    g64: Dict[str, np.ndarray]        # all 19 tensors
    g32: Dict[str, np.ndarray]        # all 19 tensors
    A: Dict[str, np.ndarray]          # the 12 factor tensors from here on
    Nm: Dict[str, np.ndarray]
    bound: Dict[str, np.ndarray]
    touched: Dict[str, np.ndarray]    # dilate(A) > 0
    rho32: float                      # max over all factor elements of |g32 - g64| / bound
    rho32_kind: Dict[str, float]      # the same per tensor kind
    z: np.ndarray                     # [R,N] float32 sample depths
    valid: np.ndarray                 # [R,N] in-box (and z-gated) samples
    app_mask: np.ndarray              # [R,N] samples above the appearance threshold
    app_window: np.ndarray            # [R,N] samples within KNIFE of it (listed or not)
    relu_window: int                  # ReLU inputs of the head within RELU_KNIFE of zero
    xn: np.ndarray                    # [R,N,3] float32 normalised coordinates
    loss: float                       # the float64 run's loss value
    out64: tuple = field(default=None, repr=False)     # (rgb, depth) of the float64 run, numpy
    samples: dict = field(default=None, repr=False)    # xn_d [V,3], up_d [V], xn_a [M',3], up_a [M', app_dim]: the float64 run's lookups

    def K(self, factor=8.0):
        return factor * max(1.0, self.rho32)


def _mlp_layers_shifted(shift):
    """oracle_torch._mlp_layers with every ReLU's switch moved from 0 to `shift`: h = p * [p > shift]."""
    def act(p):
        return p * (p > shift).to(p.dtype)

    def layers(params, x, pre=None):
        p0 = x @ params["renderModule.mlp.0.weight"].T + params["renderModule.mlp.0.bias"]
        p1 = act(p0) @ params["renderModule.mlp.2.weight"].T + params["renderModule.mlp.2.bias"]
        if pre is not None:
            pre += [p0.detach(), p1.detach()]
        return torch.sigmoid(act(p1) @ params["renderModule.mlp.4.weight"].T + params["renderModule.mlp.4.bias"])
    return layers


def _run(cfg, params, rays, jitter, n_samples, is_train, white_bg, loss, dtype, geom_dtype, thres=None, relu_shift=None):
    """One oracle forward + backward with the two factor lookups wrapped for the duration of the call: returns a dict with the gradients,
    the loss value, the outputs, aux, and per sample the lookups' inputs and upstream gradients dL/dfeature (`up_d` [V] density, `up_a`
    [M, app_dim] appearance, float64). `thres`: the appearance threshold of this run (default: the configuration's); `relu_shift`: the
    head's ReLUs switch at this pre-activation instead of 0."""
    P = O.params_from_numpy(params, dtype=dtype, requires_grad=True)
    seen = {"d": [], "a": []}
    orig_d, orig_a, orig_t, orig_m = O.density_feature, O.app_feature, cfg.ray_march_weight_thres, O._mlp_layers

    def wrap(fn, tag):
        def inner(p, xyz_norm):
            out = fn(p, xyz_norm)
            out.retain_grad()
            seen[tag].append((xyz_norm, out))
            return out
        return inner

    O.density_feature, O.app_feature = wrap(orig_d, "d"), wrap(orig_a, "a")
    try:
        if thres is not None:
            cfg.ray_march_weight_thres = thres
        if relu_shift is not None:
            O._mlp_layers = _mlp_layers_shifted(relu_shift)
        rgb, depth, z, w, aux = O.forward(cfg, P, rays, white_bg=white_bg, is_train=is_train, n_samples=n_samples,
                                          jitter=jitter if is_train else None, return_aux=True, geom_dtype=geom_dtype)
        value = loss(rgb, depth, z, w)
        value.backward()
    finally:
        O.density_feature, O.app_feature, cfg.ray_march_weight_thres, O._mlp_layers = orig_d, orig_a, orig_t, orig_m
    assert len(seen["d"]) == 1 and len(seen["a"]) == 1, "the case must have density and appearance samples"
    out = dict(grads={k: (v.grad.numpy().astype(np.float64) if v.grad is not None else np.zeros(tuple(v.shape), np.float64)) for k, v in P.items()},
               loss=float(value.detach()), rgb=rgb.detach(), depth=depth.detach(), z=z.detach(), w=w.detach(), valid=aux["valid"],
               app_mask=aux["app_mask"], relu_pre=aux["relu_pre"])
    for tag in ("d", "a"):
        xn, res = seen[tag][0]
        out["xn_" + tag] = xn.detach()
        out["up_" + tag] = (res.grad if res.grad is not None else torch.zeros_like(res)).detach().to(torch.float64)
    return out


def _per_ray_max(d, ray_of, n_rays):
    """d [S] >= 0 per sample -> max over the samples of each sample's ray, [S]."""
    m = np.zeros(n_rays, np.float64)
    np.maximum.at(m, ray_of, d)
    return m[ray_of]


def _scales(P64, xn_d, xn_a, wd, wa):
    """Gradient w.r.t. |params| of sum wd * density_feature(|P|, xn_d) + sum wa * app_feature(|P|, xn_a): per element of every plane and
    line the sum over its samples of weight * |tap weight * partner factor (* basis row)|."""
    Pabs = {k: v.detach().abs().clone().requires_grad_(k in FACTOR_KEYS) for k, v in P64.items()}
    s = (wd * O.density_feature(Pabs, xn_d)).sum() + (wa * O.app_feature(Pabs, xn_a)).sum()
    s.backward()
    return {k: Pabs[k].grad.numpy().astype(np.float64) for k in FACTOR_KEYS}


KNIFE = 2.0 ** -22     # half-width of the appearance threshold's knife edge, see reference()
RELU_KNIFE = 5e-6      # half-width of a ReLU's knife edge (tests/helpers/generic_cases.py RELU_MARGIN, tests/golden/make_golden_shapes.py)


def reference(cfg, params, rays, jitter, n_samples, is_train=True, white_bg=True, loss=None):
    """The element-wise reference of one case. `loss`: callable on (rgb, depth, z, w) that works on oracle tensors of either precision
    (and on the kernel's device tensors).

    The appearance threshold's knife edge. A sample enters the appearance list when its weight exceeds ray_march_weight_thres (1e-4). The
    weight is alpha * T with alpha = 1 - exp(-sigma dist), in float32 a difference of two numbers near 1: its absolute error reaches 2
    ulp(1) = 2^-22 whatever alpha's size, 2.4e-3 of the threshold. A few thousand samples of a case have weights within a factor of two of
    the threshold, so some ten of them sit inside that window, and the float32 oracle's list already differs from the float64 one's by a
    sample or two: the two runs' appearance sample sets cannot be required to be equal (their density sample sets are). A sample that
    flips moves its own appearance contribution in or out whole, and through d loss / d weight (the colour term) the density upstream
    of its ray. Both are stated exactly by two more float64 runs with the threshold at thres -+ KNIFE (lists L_lo >= L >= L_hi; the
    float32 run's list must lie between them, asserted): per sample of L_lo (upstream 0 where a run does not list it)
        knife = |up_lo - up| + |up_hi - up|
    is added to that sample's own delta in Nm (no per-ray maximum: it is that sample's change, not rounding noise), for the density
    upstream likewise, and A counts a sample of L_lo outside L with its upstream of the low run, so that `touched` holds every element a
    kernel with a slightly different weight may write.

    The ReLUs' knife edge. The head's 256 hidden pre-activations per appearance sample are sums of up to 351 products; the default head
    forms them from split-f16 products (2^-21 relative each), so a pre-activation carries an error of a few 1e-6 (sum |x w| ~ 10) and
    one that lies within RELU_KNIFE = 5e-6 of zero — the margin the project's goldens already keep (make_golden_shapes.py::relu_margin)
    — may switch the other way than in the reference: that unit's whole path drops out of (or enters) the sample's upstream gradient,
    some 1e-2 of it. A case has millions of ReLU inputs and therefore tens inside the window; no seed avoids them. Two more float64
    runs with every ReLU switching at -+ RELU_KNIFE instead of 0 state the change exactly, and enter `knife` the same way."""
    rays = torch.as_tensor(rays, dtype=torch.float32)
    jitter = None if jitter is None else torch.as_tensor(jitter, dtype=torch.float32)
    thres = float(cfg.ray_march_weight_thres)
    args = (cfg, params, rays, jitter, n_samples, is_train, white_bg, loss)
    r64 = _run(*args, torch.float64, torch.float32)
    rlo = _run(*args, torch.float64, torch.float32, thres=thres - KNIFE)
    rhi = _run(*args, torch.float64, torch.float32, thres=thres + KNIFE)
    r32 = _run(*args, torch.float32, None)
    relu_runs = [_run(*args, torch.float64, torch.float32, relu_shift=sh) for sh in (-RELU_KNIFE, RELU_KNIFE)]
    for r in relu_runs:
        assert torch.equal(r["app_mask"], r64["app_mask"])
    for r in [rlo, rhi, r32] + relu_runs:
        assert torch.equal(r["valid"], r64["valid"]) and torch.equal(r["xn_d"], r64["xn_d"]) and torch.equal(r["z"], r64["z"]), \
            "density sample sets of the oracle runs differ"
    U = rlo["app_mask"]
    assert bool((r64["app_mask"] <= U).all()) and bool((rhi["app_mask"] <= r64["app_mask"]).all())
    assert bool((r32["app_mask"] <= U).all()) and bool((rhi["app_mask"] <= r32["app_mask"]).all()), \
        "the float32 oracle's appearance list leaves the knife-edge window"
    xa = rlo["xn_a"]

    def on_U(r):       # a run's appearance upstream on the samples of L_lo, zero where the run does not list the sample
        up = torch.zeros_like(rlo["up_a"])
        up[r["app_mask"][U]] = r["up_a"]
        return up

    ua, ua_lo, ua_hi, ua_32 = on_U(r64), rlo["up_a"], on_U(rhi), on_U(r32)
    knife_d = sum((r["up_d"] - r64["up_d"]).abs() for r in [rlo, rhi] + relu_runs)
    knife_a = (ua_lo - ua).abs() + (ua_hi - ua).abs() + sum((on_U(r) - ua).abs() for r in relu_runs)
    both = (r64["app_mask"] & r32["app_mask"])[U]
    R = rays.shape[0]
    ray_d = torch.nonzero(r64["valid"])[:, 0].numpy()
    ray_a = torch.nonzero(U)[:, 0].numpy()
    ud = r64["up_d"]
    dd = torch.from_numpy(_per_ray_max((r32["up_d"] - ud).abs().numpy(), ray_d, R)) + knife_d
    noise_a = torch.where(both, (ua_32 - ua).abs().amax(-1), torch.zeros(ua.shape[0], dtype=torch.float64))
    da = torch.from_numpy(_per_ray_max(noise_a.numpy(), ray_a, R))[:, None] + knife_a
    P64 = O.params_from_numpy(params, dtype=torch.float64)
    A = _scales(P64, r64["xn_d"], xa, ud.abs(), torch.maximum(ua.abs(), ua_lo.abs()))
    Nm = _scales(P64, r64["xn_d"], xa, dd, da)
    g64, g32 = r64["grads"], r32["grads"]
    bound, touched = {}, {}
    for k in FACTOR_KEYS:
        dA = dilate(A[k])
        touched[k] = dA > 0
        bound[k] = 2.0 ** -22 * (A[k] + 2.0 ** -20 * dA) + (Nm[k] + 2.0 ** -20 * dilate(Nm[k]))
    rho_kind = {kind: 0.0 for kind in KINDS}
    for k in FACTOR_KEYS:
        rho_kind[kind_of(k)] = max(rho_kind[kind_of(k)], _max_ratio(g32[k] - g64[k], bound[k], touched[k]))
    xn = O.normalize_coord(cfg, rays[:, None, :3] + rays[:, None, 3:6] * r64["z"][..., None]).numpy()
    return Reference(g64=g64, g32=g32, A=A, Nm=Nm, bound=bound, touched=touched, rho32=max(rho_kind.values()), rho32_kind=rho_kind,
                     z=r64["z"].numpy(), valid=r64["valid"].numpy(), app_mask=r64["app_mask"].numpy(), app_window=(U & ~rhi["app_mask"]).numpy(),
                     relu_window=int(sum(int((p.abs() < RELU_KNIFE).sum()) for p in r64["relu_pre"])),
                     xn=xn, loss=r64["loss"], out64=(r64["rgb"].numpy(), r64["depth"].numpy()),
                     samples=dict(xn_d=r64["xn_d"], up_d=ud, xn_a=xa, up_a=ua))


def _max_ratio(err, bound, touched):
    err = np.abs(err)
    return float((err[touched] / bound[touched]).max()) if touched.any() else 0.0


def _as_np(x, shape):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x.astype(np.float64).reshape(shape)


def ratios(got, ref):
    """max |got - g64| / bound over the touched elements, per tensor kind (for information: what a run observed)."""
    out = {kind: 0.0 for kind in KINDS}
    for k in FACTOR_KEYS:
        out[kind_of(k)] = max(out[kind_of(k)], _max_ratio(_as_np(got[k], ref.g64[k].shape) - ref.g64[k], ref.bound[k], ref.touched[k]))
    return out


def failures(got, ref, K):
    """The elements that miss the check, as a list of report lines (empty: passed)."""
    lines = []
    for k in FACTOR_KEYS:
        h = _as_np(got[k], ref.g64[k].shape)
        err = np.abs(h - ref.g64[k])
        edge = BLOCK_EDGE[k.split("_")[0]]
        for what, bad in (("beyond K * bound", ref.touched[k] & (err > K * ref.bound[k])), ("stray write", ~ref.touched[k] & (h != 0))):
            n = int(bad.sum())
            if not n:
                continue
            score = np.where(bad, err / np.maximum(ref.bound[k], 1e-300) if what[0] == "b" else np.abs(h), -1.0)
            idx = np.unravel_index(int(score.argmax()), score.shape)
            sp = [int(i) for i in (idx[2:] if h.shape[-1] > 1 else idx[2:3])]
            a = float(ref.A[k][idx])
            lines.append(f"{k}: {n} element(s) {what}; worst at {tuple(int(i) for i in idx)} got {h[idx]:.6e} want {ref.g64[k][idx]:.6e} "
                         f"err/bound {float(err[idx] / max(ref.bound[k][idx], 1e-300)):.3g} err/A {float(err[idx] / a) if a else float('inf'):.3g} "
                         f"{'block' if edge == 15 else 'tile'} {tuple(i // edge for i in sp)} local {tuple(i % edge for i in sp)}")
    return lines


def check(got, ref, K):
    """|got - g64| <= K * bound element by element and got == 0 wherever no sample reaches, for the 12 factor tensors. `got`: gradients
    by state_dict name (tensors or arrays). Returns the observed max err / bound per tensor kind."""
    lines = failures(got, ref, K)
    assert not lines, f"factor gradients miss the element-wise check at K = {K:.3g}:\n" + "\n".join(lines)
    return ratios(got, ref)


def sample_contribution(params, ref, kind, index):
    """What ONE sample adds to the factor gradients (float64): sample `index` of the density lookup (kind "d") or of the appearance
    lookup (kind "a"), from the float64 run's upstream. By state_dict name; zero for the other quantity's tensors."""
    P = O.params_from_numpy(params, dtype=torch.float64)
    P = {k: v.requires_grad_(k in FACTOR_KEYS) for k, v in P.items()}
    xn = ref.samples["xn_" + kind][index:index + 1]
    up = ref.samples["up_" + kind][index:index + 1]
    ((O.density_feature if kind == "d" else O.app_feature)(P, xn) * up).sum().backward()
    return {k: (P[k].grad.numpy().astype(np.float64) if P[k].grad is not None else np.zeros(tuple(P[k].shape))) for k in FACTOR_KEYS}
