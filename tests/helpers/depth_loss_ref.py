"""Float64 references of the reference's depth losses (utils.py:301-342; csrc/t2n_depth_loss.hip) with their gradients, the driver's loss
with one of them as its depth term (`driver_loss_ex`, on optim_ref.driver_loss), and the seeded cases the CPU and GPU tests share. Plain
numpy. tests/test_depth_loss_cpu.py holds these functions to the reference's own (tests/golden/depth_loss.npz: upstream's functions run
on float64 tensors under autograd) and asserts the margins the case builder promises; tests/test_depth_loss_gpu.py holds the kernels
to them.

gnll   var = sum (z - mu)^2 w + 1e-8, apply = (|mu - y| - sigma > 0) or (sigma^2 < var), K = #apply, v = max(var, 1e-3),
       L = |1/K sum_apply 1/2 (log v + (mu - y)^2 / v)|; g = sign(signed mean) / K on applying rays, 0 elsewhere,
       dL/dvar = 1/2 g (1/v - (mu - y)^2 / v^2) (the clamp passes the gradient through), d_w[n] = dL/dvar (z_n - mu)^2,
       d_depth = g (mu - y) / v - 2 dL/dvar sum (z - mu) w. K = 0: everything 0.
si_log d = log mu - log y, alpha = -mean d, L = mean |d + alpha|, d_depth = (sign(d + alpha) - mean sign) / (R mu).
ssi    (t, s) = pinv(sqrt(w) [1, z]) sqrt(w) y over all R N samples (y broadcast along N), L = mean(w (s z + t - y)^2),
       d_w = (s z + t - y)^2 / (R N), no gradient to anything else."""
import numpy as np

from tests.helpers import optim_ref

KINDS = {"mse": 0, "gnll": 1, "si_log": 2, "ssi": 3}
SHAPES = ((1, 1), (5, 64), (6, 65), (301, 37), (1029, 3))       # LOSS_CASES of tests/test_optim_kernels_gpu.py
SIGMA = float(np.float32(0.1))                                  # target_std as the kernels receive it
DELTA = float(np.float32(0.1))
NAN_AT = 3


def f64(*arrays):
    return tuple(np.asarray(a, np.float64) for a in arrays)


def gnll(depth, w, z, y, sigma):
    mu, w, z, y = f64(depth, w, z, y)
    sigma = float(sigma)
    dz = z - mu[:, None]
    var = (dz * dz * w).sum(1) + 1e-8
    c = (dz * w).sum(1)
    e = mu - y
    apply = ((np.abs(e) - sigma) > 0) | (sigma * sigma < var)
    K = int(apply.sum())
    v = np.maximum(var, 1e-3)
    out = dict(var=var, apply=apply, K=K, v=v)
    if K == 0:
        out.update(loss=0.0, mean=0.0, d_depth=np.zeros_like(mu), d_w=np.zeros_like(w))
        return out
    mean = float((0.5 * (np.log(v) + e * e / v))[apply].sum() / K)
    g = np.where(apply, np.sign(mean) / K, 0.0)
    dvar = 0.5 * g * (1.0 / v - e * e / (v * v))
    out.update(loss=abs(mean), mean=mean, d_depth=g * e / v - 2.0 * dvar * c, d_w=dvar[:, None] * dz * dz)
    return out


def si_log(depth, y):
    mu, y = f64(depth, y)
    R = mu.shape[0]
    d = np.log(mu) - np.log(y)
    alpha = float(-d.sum() / R)
    u = d + alpha
    sg = np.sign(u)
    return dict(loss=float(np.abs(u).sum() / R), alpha=alpha, u=u, d_depth=(sg - sg.sum() / R) / (R * mu))


def ssi_moments(w, z, y):
    w, z, y = f64(w, z, y)
    yy = np.broadcast_to(y[:, None], z.shape)
    return float(w.sum()), float((w * z).sum()), float((w * z * z).sum()), float((w * yy).sum()), float((w * z * yy).sum())


def ssi(w, z, y, st_float32=False):
    """`st_float32`: s and t rounded to float32 before they meet z, as upstream's product with float32 tensors (and the kernels' pass 2)
    does; False: the float64 evaluation (what the reference gives on float64 tensors). `kappa`: the 2-norm condition number of the
    normal matrix [[S0, S1], [S1, S2]]; `deficient`: the rule of the kernels (weighted variance of z <= 1e-12 S2 / S0, or S0 = 0) with
    `closed` = the pseudo-inverse's closed form there: (t, s) = ybar (1, z0) / (1 + z0^2)."""
    w, z, y = f64(w, z, y)
    R, N = z.shape
    yy = np.broadcast_to(y[:, None], z.shape)
    sw = np.sqrt(w).reshape(-1)
    X = np.stack([np.ones(R * N), z.reshape(-1)], 1) * sw[:, None]
    t, s = (float(v) for v in np.linalg.pinv(X) @ (yy.reshape(-1) * sw))
    S0, S1, S2, Sy, Szy = ssi_moments(w, z, y)
    with np.errstate(all="ignore"):
        kappa = float(np.linalg.cond(np.array([[S0, S1], [S1, S2]]))) if S0 > 0 else float("inf")
    deficient, closed = True, (0.0, 0.0)
    if S0 > 0:
        zb, yb = S1 / S0, Sy / S0
        deficient = (S2 / S0 - zb * zb) <= 1e-12 * (S2 / S0)
        closed = (yb * zb / (1 + zb * zb), yb / (1 + zb * zb))       # (s, t)
    su, tu = (float(np.float32(s)), float(np.float32(t))) if st_float32 else (s, t)
    res = su * z + tu - yy
    return dict(loss=float((w * res * res).sum() / (R * N)), s=s, t=t, kappa=kappa, deficient=bool(deficient), closed=closed,
                d_w=res * res / (R * N), z0=(S1 / S0 if S0 > 0 else 0.0))


def depth_term(kind, depth, w, z, y, sigma=SIGMA, st_float32=True):
    """(term, d_depth [R], d_w [R, N], aux [4]) of one kind for upstream gradient 1; aux as t2n_depth_loss reports it."""
    w64 = np.asarray(w, np.float64)
    if kind == "gnll":
        o = gnll(depth, w, z, y, sigma)
        return o["loss"], o["d_depth"], o["d_w"], np.array([o["K"], o["mean"], 0.0, 0.0])
    if kind == "si_log":
        o = si_log(depth, y)
        return o["loss"], o["d_depth"], np.zeros_like(w64), np.array([o["alpha"], 0.0, 0.0, 0.0])
    assert kind == "ssi", kind
    o = ssi(w, z, y, st_float32)
    return o["loss"], np.zeros(w64.shape[0]), o["d_w"], np.array([o["s"], o["t"], 0.0, 0.0])


def driver_loss_ex(kind, rgb, depth, w, z, rgb_t, depth_t, w_depth, w_trans, delta, sigma=SIGMA):
    """optim_ref.driver_loss with the depth term `kind`: (losses [mse, term, transmittance, total], d_rgb, d_depth, d_w, aux). NaN depths
    count as 0 and get no d_depth (text2nerf_main.py:559-560), whatever the kind."""
    losses, d_rgb, d_depth, d_w = optim_ref.driver_loss(rgb, depth, w, z, rgb_t, depth_t, w_depth, w_trans, delta)
    if kind == "mse":
        return losses, d_rgb, d_depth, d_w, np.zeros(4)
    _, _, _, d_w_trans = optim_ref.driver_loss(rgb, depth, w, z, rgb_t, depth_t, 0.0, w_trans, delta)
    dep = np.asarray(depth, np.float64)
    bad = np.isnan(dep)
    term, g_depth, g_w, aux = depth_term(kind, np.where(bad, 0.0, dep), w, z, depth_t, sigma)
    out = np.array([losses[0], term, losses[2], losses[0] + float(w_depth) * term + float(w_trans) * losses[2]], np.float64)
    return out, d_rgb, np.where(bad, 0.0, float(w_depth) * g_depth), d_w_trans + float(w_depth) * g_w, aux


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
def margins(c, sigma=SIGMA, delta=DELTA):
    """The smallest distance of a case's inputs from every branch of the kernels, as the issue lists them: mean, var against sigma^2
    (relative to sigma^2), var against the 1e-3 clamp, |d + alpha| (inf for R = 1, where it is exactly 0), the transmittance mask."""
    y = c["depth_t"].astype(np.float64)
    out = dict(mean=np.inf, var_sigma=np.inf, var_clamp=np.inf)
    for dep in (np.where(np.isnan(c["depth"]), 0.0, c["depth"]), c["depth_fin"]):
        o = gnll(dep, c["w"], c["z"], y, sigma)
        out["mean"] = min(out["mean"], float(np.abs(np.abs(np.asarray(dep, np.float64) - y) - sigma).min()))
        out["var_sigma"] = min(out["var_sigma"], float(np.abs(o["var"] - sigma * sigma).min() / (sigma * sigma)))
        out["var_clamp"] = min(out["var_clamp"], float(np.abs(o["var"] - 1e-3).min()))
    out["si"] = float(np.abs(si_log(c["depth_fin"], y)["u"]).min()) if y.shape[0] > 1 else np.inf
    out["mask"] = float(np.abs((c["z"].astype(np.float64) - y[:, None]) + delta).min())
    return out


MARGIN_FLOORS = dict(mean=1e-3, var_sigma=1e-3, var_clamp=1e-4, si=1e-3, mask=1e-3)


def random_case(R, N, narrow=False):
    """A seeded float32 case: rgb / rgb_t in [0, 1), w ~ U[0, 0.05], z increasing along n in [0.5, 8] (`narrow`: in [6, 6.4], an
    ill-conditioned fit: kappa >= 1e3), depth in [1, 7] drawn on its own (independent of sum w z), targets in [2, 7], `depth` with one
    NaN when R >= 5 and `depth_fin` with a finite value in its place. Inputs are nudged until every margin of `margins` holds with room
    (5x the floor), so that float32 and float64 agree about every branch; no element is ever left out of a comparison."""
    rng = np.random.default_rng([31, R, N, int(narrow)])
    rgb, rgb_t = rng.random((R, 3)).astype(np.float32), rng.random((R, 3)).astype(np.float32)
    y = (rng.random(R) * 5 + 2).astype(np.float32)
    mu = (rng.random(R) * 6 + 1).astype(np.float32)
    w = (rng.random((R, N)) * 0.05).astype(np.float32)
    lo, hi = (6.0, 6.4) if narrow else (0.5, 8.0)
    z = np.sort(rng.uniform(lo, hi, (R, N)), 1)
    z = np.where(np.abs(z - y[:, None].astype(np.float64) + DELTA) < 5e-3, z + 0.02, z)
    z = np.sort(np.clip(z, 0.5, 8.0), 1).astype(np.float32)
    for _ in range(100):      # the mean margin and the log-ratio margin both move mu: repeat until neither has a violator
        e = mu.astype(np.float64) - y
        near = np.abs(np.abs(e) - SIGMA) < 5e-3
        mu = np.where(near, mu + np.float32(0.02) * np.where(e >= 0, 1, -1).astype(np.float32), mu).astype(np.float32)
        u = si_log(mu, y)["u"]
        close = (np.abs(u) < 5e-3) & (R > 1)
        mu = np.where(close, mu * np.float32(1.02), mu).astype(np.float32)
        if not near.any() and not close.any():
            break
    else:
        raise AssertionError("random_case: the depth margins did not settle")
    nan_at = NAN_AT if R >= 5 else None
    for _ in range(100):      # var scales with the ray's weights: shrink them where var sits on sigma^2 or on the clamp
        bad = np.zeros(R, bool)
        for dep in ((np.where(np.arange(R) == nan_at, 0.0, mu) if nan_at is not None else mu), mu):
            var = gnll(dep, w, z, y, SIGMA)["var"]
            bad |= (np.abs(var - SIGMA * SIGMA) < 5e-3 * SIGMA * SIGMA) | (np.abs(var - 1e-3) < 5e-4)
        if not bad.any():
            break
        w = np.where(bad[:, None], w * np.float32(0.7), w).astype(np.float32)
    else:
        raise AssertionError("random_case: the variance margins did not settle")
    depth = mu.copy()
    if nan_at is not None:
        depth[nan_at] = np.nan
    return dict(rgb=rgb, rgb_t=rgb_t, depth=depth, depth_fin=mu, w=w, z=z, depth_t=y)


DIRECTED = {"mixed": "naavmvm", "k0": "nnnnn", "k1": "nnvnn", "all": "mvmv"}      # n: not applying, m: through the mean, v: the variance


def directed_case(name):
    """gnll rays from one-hot weights (N = 5, the hot sample at n = 2, so var = (z_2 - mu)^2 + 1e-8 exactly as float64 sees the float32
    inputs): 'n' |mu - y| = 0.05 and var = 0.0025 (does not apply), 'm' mu - y = 0.5 and z_2 = mu: var = 1e-8, clamped to 1e-3 (applies
    through the mean only), 'v' |mu - y| = 0.05 and var = 1 (through the variance only), 'a' both. `classes`: the string."""
    classes = DIRECTED[name]
    R, N = len(classes), 5
    rng = np.random.default_rng([32, R, sum(map(ord, name))])
    y = (rng.random(R) * 3 + 2).astype(np.float32)
    de = {"n": 0.05, "m": 0.5, "v": 0.05, "a": 0.5}
    off = {"n": 0.05, "m": 0.0, "v": 1.0, "a": 1.0}
    mu = (y + np.array([de[k] for k in classes], np.float32)).astype(np.float32)
    offs = np.tile(np.array([-1.0, -0.5, 0.0, 1.5, 2.0], np.float32), (R, 1))
    offs[:, 2] = [off[k] for k in classes]
    z = (mu[:, None] + offs).astype(np.float32)
    w = np.zeros((R, N), np.float32)
    w[:, 2] = 1.0
    rgb, rgb_t = rng.random((R, 3)).astype(np.float32), rng.random((R, 3)).astype(np.float32)
    return dict(rgb=rgb, rgb_t=rgb_t, depth=mu.copy(), depth_fin=mu, w=w, z=z, depth_t=y, classes=classes)


def ssi_special_case(name, R=6, N=65):
    """The rank-deficient fits — 'zero-w' all weights 0 (s = t = 0), 'equal-z' every z the same z0 ((t, s) = ybar (1, z0) / (1 + z0^2)) —
    and 'affine', a full-rank fit with residual 0."""
    c = random_case(R, N)
    if name == "zero-w":
        c["w"] = np.zeros_like(c["w"])
    elif name == "affine":
        # a perfect fit: z constant along each ray and y = 0.5 z + 1.5 exactly (float32-exact values), so the residual is 0 and the
        # loss's expanded six-moment form in the kernel cancels completely: the loss is held to the stage's absolute floor
        zr = np.array([1.0, 2.0, 3.5, 4.5, 5.5, 7.0], np.float32)[:R]
        c["z"] = np.repeat(zr[:, None], N, 1)
        c["depth_t"] = (np.float32(0.5) * zr + np.float32(1.5)).astype(np.float32)
    else:
        assert name == "equal-z", name
        c["z"] = np.full_like(c["z"], np.float32(3.25))
    return c


def all_cases():
    """{case id: case} of everything the fixture and the tests run."""
    out = {}
    for R, N in SHAPES:
        out[f"rand-{R}x{N}"] = random_case(R, N)
        out[f"narrow-{R}x{N}"] = random_case(R, N, narrow=True)
    for name in DIRECTED:
        out[f"directed-{name}"] = directed_case(name)
    for name in ("zero-w", "equal-z", "affine"):
        out[f"ssi-{name}"] = ssi_special_case(name)
    return out
