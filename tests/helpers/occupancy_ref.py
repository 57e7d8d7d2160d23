"""Float64 references, error laws and checkers of the stages that change the field between training phases: the occupancy volume
(k_alpha_volume), the bilinear resize (k_upsample_bilinear), the mask sample (alpha_value / axis_taps of csrc/t2n_device.h through
k_alpha_at), the two ray filters (k_filter_alpha, k_filter_bbox) and alpha at points or dense nodes (k_compute_alpha).

Each reference restates the OPERATION in float64 from the float32 inputs the kernel gets; none follows the kernel's instruction
order. The library is built without contraction, so every float32 operation of a kernel rounds once: u = 2^-24 relative.

LAWS (first order; K counts the roundings that reach one term of the output, read off the kernel's code).

  volume, box      clamp, max and compare are exact: equality, the volume as an array and the six indices as integers.

  resize           src = dst (in - 1) / (out - 1).  The float32 index sh * y carries two roundings (the quotient sh, the product):
                   |d| <= 2^-23 (in - 1) per axis; it is exact (d = 0) when in == out, in == 1 or out == 1.  The output is piecewise
                   linear and continuous in the index, so  b = dy |row difference| + dx |column difference| + K_RESIZE u sum |w v|.
                   The differences are those of the texel's own cell, and of the neighbouring cell too where the exact index lies
                   within d of the cell's edge.  K_RESIZE = 6: w0 = 1 - w1 (1; w1 = src - floor is exact), w v (1), the row's
                   addition (1), h0 = 1 - h1 (1), h (...) (1), the closing addition (1).  in == out on both axes: bit-equal copy.

  mask sample      ix = ((t - 1) + 1) / 2 (S - 1),  t = (p - a_min) a_inv.  a_inv = (1 / (a_max - a_min)) 2 carries 2 roundings, the
                   subtraction p - a_min 1, the product 1: t has 4 u |t|; then t - 1 (u |t - 1|), + 1 (u |t|), the product with S - 1
                   (u |ix|):  d_ix = u ((S - 1) / 2 (5 |t| + |t - 1|) + |ix|) cells.
                   value:  b = K_ALPHA u sum |w v| + sum over axes d_ix |difference along that axis|,  K_ALPHA = 13: three weights
                   (1 each at most: w0 = 1 - w1), their two products (2), v w (1), seven additions (7).
                   decision (> 0, volumes without negative values): the sum is positive iff an occupied tap has three non-zero
                   weights, i.e. the float32 index lies in the open support (n - 1, n + 1)^3 of an occupied node n.  margin = the
                   largest over occupied nodes of min over axes (1 - |ix - n|), in cells: hit iff margin > 0; a point with
                   |margin| <= max d_ix is UNDECIDED.

  alpha filter     the samples are the oracle's sample_ray in float64.  t_min: numerator (1), quotient (1): 2 u |t_min|;
                   z = t_min + step i: the product (u step i), the sum (u |z|); p = o + d z: u |d z| + u |p|.  Mapped to cells by
                   a_inv (S - 1) / 2 and added to d_ix above.  A ray is kept iff a sample hits: decided kept if a sample's margin
                   exceeds its d, decided dropped if every sample's margin is below -d, else UNDECIDED.

  slab test        six quotients (a - o) / v: numerator (1), quotient (1): each within 2 u of its float64 value, and exact where the
                   float64 value is a float32 number and the numerator too.  min and max are exact and monotone, so the kernel's
                   t_min lies in [lo, hi] of the quotients' intervals, likewise t_max.  kept iff t_max > t_min: decided kept if
                   t_max's lower end exceeds t_min's upper end, decided dropped if t_max's upper end <= t_min's lower end.

  alpha            tests/helpers/march_ref.py's law carried to 1 - exp(-sigma length): feature GAMMA_F A, activation C_ACT, the
                   exponent's one product, exp (C_EXP) and the closing subtraction (u absolute).  The device is held to K = 4 times
                   the law as there; the profile records the ratio to 1 x the law.

Checkers return a dict with `bad` (indices or a count; empty / 0 means passed), `ratio` (worst error / bound) and `undecided`."""
import math

import numpy as np
import torch

from oracle import oracle_torch as O
from tests.helpers.geometry_ref import GAMMA_F, density_grad, params64_of
from tests.helpers.march_ref import C_ACT, C_EXP, K as K_MARCH

U = 2.0 ** -24
K_RESIZE = 6
K_ALPHA = 13
INT_MAX = 0x7FFFFFFF
TINY64 = 1e-300

VOLUME_MUTATIONS = ("no_transpose", "pool6", "gt", "box_max_off", "box_before_dilation")
RESIZE_MUTATIONS = ("align_false", "round_index", "clamp_early")
SAMPLE_MUTATIONS = ("border",)
FILTER_MUTATIONS = ("first64", "n_plus_1")
SLAB_MUTATIONS = ("ge", "no_substitution")


def f32(x):
    return np.asarray(x, np.float32)


# ---- occupancy volume ------------------------------------------------------------------------------------------------------------------
def alpha_volume(dense, thres, mutate=None):
    """dense [gx,gy,gz] float32, finite. Returns (volume [gz,gy,gx] float32 of 0 / 1, box int64 [6] = min x,y,z, max x,y,z; the
    initial INT_MAX / -1 where nothing is kept)."""
    assert mutate is None or mutate in VOLUME_MUTATIONS
    d = np.clip(f32(dense).astype(np.float64), 0.0, 1.0)
    a = d if mutate == "no_transpose" else d.transpose(2, 1, 0)
    D, H, W = a.shape
    pad = np.full((D + 2, H + 2, W + 2), -np.inf)
    pad[1:-1, 1:-1, 1:-1] = a
    m = np.full(a.shape, -np.inf)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                if mutate == "pool6" and (dz != 1) + (dy != 1) + (dx != 1) > 1:
                    continue
                m = np.maximum(m, pad[dz:dz + D, dy:dy + H, dx:dx + W])
    t = float(np.float32(thres))
    keep = m > t if mutate == "gt" else m >= t
    src = (a > t if mutate == "gt" else a >= t) if mutate == "box_before_dilation" else keep
    box = np.array([INT_MAX] * 3 + [-1] * 3, np.int64)
    if src.any():
        idx = np.argwhere(src)[:, ::-1]        # (z, y, x) -> (x, y, z); for no_transpose the axes are already wrong
        box = np.concatenate([idx.min(0), idx.max(0)]).astype(np.int64)
        if mutate == "box_max_off":
            box[3:] -= 1
    return keep.astype(np.float32), box


def check_volume(vol, box, dense, thres):
    """vol: the n floats the kernel wrote (any shape), box: its six integers."""
    want_v, want_b = alpha_volume(dense, thres)
    got = f32(vol).reshape(-1)
    bad = []
    if got.shape != want_v.reshape(-1).shape or not np.array_equal(got.view(np.uint32), want_v.reshape(-1).view(np.uint32)):
        bad.append("volume")
    if not np.array_equal(np.asarray(box, np.int64).reshape(-1), want_b):
        bad.append("box")
    return {"bad": bad, "ratio": 0.0, "undecided": 0, "kept": int(want_v.sum())}


def node_coord(a0, a1, s):
    """getDenseAlpha's node coordinate a0 (1 - s) + a1 s in float32, operation by operation."""
    a0, a1, s = f32(a0), f32(a1), f32(s)
    return (a0 * (np.float32(1.0) - s) + a1 * s).astype(np.float32)


def dense_nodes(aabb, lins):
    """dense_xyz [gx,gy,gz,3] float32 of getDenseAlpha from the three linspace(0, 1, g) arrays."""
    a = f32(aabb)
    ax = [node_coord(a[0, k], a[1, k], lins[k]) for k in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).astype(np.float32)


def box_to_aabb(aabb, lins, box):
    """updateAlphaMask's new_aabb [2,3] float32 from the six indices."""
    a = f32(aabb)
    lo = [node_coord(a[0, k], a[1, k], lins[k][int(box[k])]) for k in range(3)]
    hi = [node_coord(a[0, k], a[1, k], lins[k][int(box[3 + k])]) for k in range(3)]
    return np.array([lo, hi], np.float32)


# ---- bilinear resize -----------------------------------------------------------------------------------------------------------------------
def _axis(n_in, n_out, mutate=None):
    """Exact source index of every output index: cell i0 (int), fraction fr (float64 of the exact rational), second tap i1, the
    float32 index's error bound d, and whether the exact index is an integer strictly inside (0, n_in - 1)."""
    y = np.arange(n_out, dtype=np.int64)
    den = max(n_out - 1, 1)
    num = y * (n_in - 1) if n_out > 1 else np.zeros_like(y)
    i0, rem = num // den, num % den
    fr = rem.astype(np.float64) / den
    if mutate == "round_index":
        i0 = np.minimum(i0 + (fr >= 0.5), n_in - 1)
    lim = n_in - 2 if mutate == "clamp_early" else n_in - 1
    i1 = i0 + (i0 < lim)
    d = 0.0 if (n_in == n_out or n_in == 1 or n_out == 1) else 2.0 ** -23 * (n_in - 1)
    interior = (rem == 0) & (i0 > 0) & (i0 < n_in - 1)
    return i0, i1, fr, d, interior


def integer_source_rows(n_in, n_out):
    """Output indices whose exact source index is an integer other than 0 and n_in - 1."""
    return np.nonzero(_axis(n_in, n_out)[4])[0]


def resize(src, h_out, w_out, mutate=None):
    """src [C,Hin,Win] float32 -> (out [C,h_out,w_out] float64, bound [C,h_out,w_out]) of the align_corners=True bilinear resize."""
    assert mutate is None or mutate in RESIZE_MUTATIONS
    v = f32(src).astype(np.float64)
    C, Hin, Win = v.shape
    if mutate == "align_false":
        out = torch.nn.functional.interpolate(torch.from_numpy(v)[None], size=(h_out, w_out), mode="bilinear", align_corners=False)
        return out[0].numpy(), None
    y0, y1, fy, dy, _ = _axis(Hin, h_out, mutate)
    x0, x1, fx, dx, _ = _axis(Win, w_out, mutate)
    FY, FX = fy[None, :, None], fx[None, None, :]

    def at(yy, xx):
        return v[:, yy][:, :, xx]

    v00, v01, v10, v11 = at(y0, x0), at(y0, x1), at(y1, x0), at(y1, x1)
    out = (1 - FY) * ((1 - FX) * v00 + FX * v01) + FY * ((1 - FX) * v10 + FX * v11)
    mag = (1 - FY) * ((1 - FX) * np.abs(v00) + FX * np.abs(v01)) + FY * ((1 - FX) * np.abs(v10) + FX * np.abs(v11))

    def row_diff(c):          # |rows c + 1 - c| at the texel's columns, 0 for cells outside the grid
        ok = (c >= 0) & (c <= Hin - 2)
        cc = np.clip(c, 0, max(Hin - 2, 0))
        c1 = np.minimum(cc + 1, Hin - 1)
        d = (1 - FX) * np.abs(at(c1, x0) - at(cc, x0)) + FX * np.abs(at(c1, x1) - at(cc, x1))
        return d * ok[None, :, None]

    def col_diff(c):
        ok = (c >= 0) & (c <= Win - 2)
        cc = np.clip(c, 0, max(Win - 2, 0))
        c1 = np.minimum(cc + 1, Win - 1)
        d = (1 - FY) * np.abs(at(y0, c1) - at(y0, cc)) + FY * np.abs(at(y1, c1) - at(y1, cc))
        return d * ok[None, None, :]

    sy = np.maximum(row_diff(y0), np.maximum(row_diff(y0 - 1) * (fy <= dy)[None, :, None], row_diff(y0 + 1) * (1 - fy <= dy)[None, :, None]))
    sx = np.maximum(col_diff(x0), np.maximum(col_diff(x0 - 1) * (fx <= dx)[None, None, :], col_diff(x0 + 1) * (1 - fx <= dx)[None, None, :]))
    bound = dy * sy + dx * sx + K_RESIZE * U * mag
    return out, bound


def check_resize(got, src, h_out, w_out):
    got = f32(got)
    src = f32(src)
    want, bound = resize(src, h_out, w_out)
    if got.shape != want.shape:
        return {"bad": -1, "ratio": math.inf, "undecided": 0}
    if src.shape[1:] == (h_out, w_out):
        same = np.array_equal(got.view(np.uint32), src.view(np.uint32))
        return {"bad": 0 if same else int((got.view(np.uint32) != src.view(np.uint32)).sum()), "ratio": 0.0, "undecided": 0}
    err = np.abs(got.astype(np.float64) - want)
    bad = int(((err > bound) | ~np.isfinite(got)).sum())
    ratio = float((err / np.maximum(bound, TINY64))[bound > 0].max()) if (bound > 0).any() else 0.0
    if np.any((bound == 0) & (err != 0)):
        ratio = math.inf
    return {"bad": bad, "ratio": ratio, "undecided": 0}


# ---- mask sample ------------------------------------------------------------------------------------------------------------------------
def _tri(vol, ix, iy, iz, border=False):
    """Trilinear read of vol [D,H,W] (float64) at index coordinates; zeros padding (or border clamping). Returns (value, sum |w v|)."""
    D, H, W = vol.shape
    val, mag = np.zeros(ix.shape), np.zeros(ix.shape)
    if border:
        ix, iy, iz = np.clip(ix, 0, W - 1), np.clip(iy, 0, H - 1), np.clip(iz, 0, D - 1)
    x0, y0, z0 = np.floor(ix), np.floor(iy), np.floor(iz)
    fx, fy, fz = ix - x0, iy - y0, iz - z0
    x0, y0, z0 = x0.astype(np.int64), y0.astype(np.int64), z0.astype(np.int64)
    for dz, wz in ((0, 1 - fz), (1, fz)):
        for dy, wy in ((0, 1 - fy), (1, fy)):
            for dx, wx in ((0, 1 - fx), (1, fx)):
                xx, yy, zz = x0 + dx, y0 + dy, z0 + dz
                ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H) & (zz >= 0) & (zz < D)
                t = vol[np.clip(zz, 0, D - 1), np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)] * ok * (wx * wy * wz)
                val += t
                mag += np.abs(t)
    return val, mag


def mask_index(mask_aabb, dims, pts):
    """Index coordinates [n,3] (x, y, z order) of world points in the mask grid, float64 from the float32 inputs, and the bound
    d [n,3] of the float32 index's error in cells."""
    return _index64(mask_aabb, dims, f32(pts).astype(np.float64))


def _index64(mask_aabb, dims, p):
    a = f32(mask_aabb).astype(np.float64)
    S = np.array([dims[2], dims[1], dims[0]], np.float64)        # W, H, D
    t = (p - a[0]) * (2.0 / (a[1] - a[0]))
    ix = ((t - 1) + 1) / 2 * (S - 1)
    d = U * ((S - 1) / 2 * (5 * np.abs(t) + np.abs(t - 1)) + np.abs(ix))
    return ix, d


def support_margin(vol, ix, chunk=20000):
    """max over the nodes with vol != 0 of min over axes (1 - |ix - n|), in cells; -inf for an empty volume."""
    nodes = np.argwhere(np.asarray(vol) != 0)[:, ::-1].astype(np.float64)     # (x, y, z)
    out = np.full(ix.shape[0], -np.inf)
    if not len(nodes):
        return out
    for s in range(0, ix.shape[0], chunk):
        d = 1.0 - np.abs(ix[s:s + chunk, None, :] - nodes[None])
        out[s:s + chunk] = d.min(-1).max(-1)
    return out


def mask_sample(vol, mask_aabb, pts, mutate=None):
    """Returns dict: value [n] float64, bound [n], hit [n] bool (value > 0), decided [n] bool (meaningful where vol has no negative
    value), margin [n], d [n] (the largest index error over the axes)."""
    assert mutate is None or mutate in SAMPLE_MUTATIONS
    v = f32(vol).astype(np.float64)
    ix, d = mask_index(mask_aabb, v.shape, pts)
    val, mag = _tri(v, ix[:, 0], ix[:, 1], ix[:, 2], border=mutate == "border")
    slope = np.zeros_like(ix)
    for a in range(3):
        f0 = np.floor(ix[:, a])
        fr = ix[:, a] - f0
        for c, use in ((f0, np.ones(len(f0), bool)), (f0 - 1, fr <= d[:, a]), (f0 + 1, 1 - fr <= d[:, a])):
            lo, hi = ix.copy(), ix.copy()
            lo[:, a], hi[:, a] = c, c + 1
            s = np.abs(_tri(v, hi[:, 0], hi[:, 1], hi[:, 2])[0] - _tri(v, lo[:, 0], lo[:, 1], lo[:, 2])[0])
            slope[:, a] = np.maximum(slope[:, a], s * use)
    bound = K_ALPHA * U * mag + (d * slope).sum(-1)
    margin = support_margin(v, ix)
    dm = d.max(-1)
    return {"value": val, "bound": bound, "hit": val > 0, "decided": np.abs(margin) > dm, "margin": margin, "d": dm}


def check_mask_sample(got, vol, mask_aabb, pts):
    got = f32(got).astype(np.float64)
    r = mask_sample(vol, mask_aabb, pts)
    err = np.abs(got - r["value"])
    bad = (err > r["bound"]) | ~np.isfinite(got)
    und = 0
    if not (f32(vol) < 0).any():
        dec = r["decided"]
        bad |= dec & ((got > 0) != r["hit"])
        und = int((~dec).sum())
    pos = r["bound"] > 0
    ratio = float((err[pos] / r["bound"][pos]).max()) if pos.any() else 0.0
    if np.any(~pos & (err != 0)):
        ratio = math.inf
    return {"bad": np.nonzero(bad)[0], "ratio": ratio, "undecided": und}


# ---- alpha filter -------------------------------------------------------------------------------------------------------------------------
def filter_alpha(cfg, rays, n_samples, mutate=None, chunk_rays=64):
    """cfg: oracle FieldConfig with alpha_volume / alpha_aabb (0 / 1 volume). rays [R, >= 6] float32.
    Returns dict: keep [R] bool, decided [R] bool, margin [R] (the decisive sample's margin minus / plus its d)."""
    assert mutate is None or mutate in FILTER_MUTATIONS
    n = {"first64": min(n_samples, 64), "n_plus_1": n_samples + 1}.get(mutate, n_samples)
    r = torch.from_numpy(f32(rays)[:, :6].astype(np.float64))
    vol = np.asarray(cfg.alpha_volume, np.float32)
    a = f32(cfg.alpha_aabb).astype(np.float64)
    S = np.array([vol.shape[2], vol.shape[1], vol.shape[0]], np.float64)
    scale = (2.0 / (a[1] - a[0])) * (S - 1) / 2
    R = r.shape[0]
    keep, dk, dd, mg = np.zeros(R, bool), np.zeros(R, bool), np.zeros(R, bool), np.zeros(R)
    step = float(np.float32(cfg.step_size))
    for s in range(0, R, chunk_rays):
        o, d = r[s:s + chunk_rays, :3], r[s:s + chunk_rays, 3:6]
        pts, z, _ = O.sample_ray(cfg, o, d, n)
        pts, z, dn = pts.numpy(), z.numpy(), np.abs(d.numpy())
        i = np.arange(n, dtype=np.float64)[None]
        dz = 2 * U * np.abs(z[:, :1]) + U * step * i + U * np.abs(z)
        dp = dn[:, None, :] * dz[..., None] + U * dn[:, None, :] * np.abs(z)[..., None] + U * np.abs(pts)
        ix, dix = _index64(cfg.alpha_aabb, vol.shape, pts.reshape(-1, 3))
        dix = dix + dp.reshape(-1, 3) * scale
        m = support_margin(vol, ix).reshape(z.shape)
        e = dix.max(-1).reshape(z.shape)
        keep[s:s + chunk_rays] = (m > 0).any(-1)
        dk[s:s + chunk_rays] = (m > e).any(-1)
        dd[s:s + chunk_rays] = (m < -e).all(-1)
        mg[s:s + chunk_rays] = np.where((m > 0).any(-1), (m - e).max(-1), (-m - e).min(-1))
    return {"keep": keep, "decided": dk | dd, "margin": mg}


def check_flags(got, ref):
    """got: the bytes a filter kernel wrote; ref: a dict with keep / decided. Every byte must be 0 or 1."""
    g = np.asarray(got).reshape(-1)
    if g.shape != ref["keep"].shape:
        return {"bad": np.array([-1]), "ratio": 0.0, "undecided": 0}
    bad = ~np.isin(g, (0, 1)) | (ref["decided"] & ((g != 0) != ref["keep"]))
    return {"bad": np.nonzero(bad)[0], "ratio": 0.0, "undecided": int((~ref["decided"]).sum())}


# ---- slab test -------------------------------------------------------------------------------------------------------------------------------
def slab(aabb, rays, mutate=None):
    """filtering_rays(bbox_only=True) on the LINE of each ray. Returns dict: keep, decided, margin (t_max - t_min in float64)."""
    assert mutate is None or mutate in SLAB_MUTATIONS
    a = f32(aabb).astype(np.float64)
    r32 = f32(rays)[:, :6]
    o, d = r32[:, :3].astype(np.float64), r32[:, 3:6].astype(np.float64)
    v = d if mutate == "no_substitution" else np.where(d == 0, float(np.float32(1e-6)), d)
    qs, lo_t, hi_t = [], [], []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k in (1, 0):
            num = a[k] - o
            q = num / v
            exact = (num == num.astype(np.float32)) & (q == q.astype(np.float32))
            e = np.where(exact | ~np.isfinite(q), 0.0, 2 * U * np.abs(q))
            qs.append(q)
            lo_t.append(q - e)
            hi_t.append(q + e)
    mn, mx = np.fmin, np.fmax         # fminf / fmaxf: a NaN operand is ignored
    tmin = mx.reduce(mn(qs[0], qs[1]), axis=-1)
    tmax = mn.reduce(mx(qs[0], qs[1]), axis=-1)
    tmin_lo, tmin_hi = mx.reduce(mn(lo_t[0], lo_t[1]), axis=-1), mx.reduce(mn(hi_t[0], hi_t[1]), axis=-1)
    tmax_lo, tmax_hi = mn.reduce(mx(lo_t[0], lo_t[1]), axis=-1), mn.reduce(mx(hi_t[0], hi_t[1]), axis=-1)
    keep = tmax >= tmin if mutate == "ge" else tmax > tmin
    decided = (tmax_lo > tmin_hi) | (tmax_hi <= tmin_lo)
    return {"keep": keep, "decided": decided, "margin": tmax - tmin}


# ---- alpha at points / dense nodes -------------------------------------------------------------------------------------------------------
def alpha_at_points(cfg, params, pts, length, bf16=False):
    """1 - exp(-sigma length) at world points [n,3] (float32), sigma = 0 where cfg's mask (a 0 / 1 volume) samples <= 0.
    params: numpy state dict. The normalised position is the field's float32 one (tests/helpers/geometry_ref.py holds it bit-equal
    to the kernels'); everything behind it is float64. Returns dict: alpha, bound (1 x the law), decided (mask decision), masked."""
    p = torch.from_numpy(f32(pts).reshape(-1, 3))
    n = p.shape[0]
    live, decided = np.ones(n, bool), np.ones(n, bool)
    if cfg.alpha_volume is not None:
        r = mask_sample(np.asarray(cfg.alpha_volume, np.float32), cfg.alpha_aabb, p.numpy())
        live, decided = r["hit"], r["decided"]
    xn = O.normalize_coord(cfg, p)
    a32 = torch.tensor(cfg.aabb, dtype=torch.float32)
    inv = (2.0 / (a32[1] - a32[0])).numpy()
    f, _, A, _ = density_grad(params64_of(params, bf16=bf16), xn, inv, cfg.grid_size)
    f, A = f.numpy(), A.numpy()
    df = GAMMA_F * A
    if cfg.fea2dense_act == "relu":
        sigma, ds = np.maximum(f, 0.0), df
    else:
        x = f + cfg.density_shift
        sigma = np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, 20.0))))
        ds = 1.0 / (1.0 + np.exp(-x)) * (df + U * np.abs(x)) + C_ACT * U * sigma
    L = float(np.float32(length))
    t = sigma * L
    alpha = -np.expm1(-t)
    bound = np.exp(-t) * (abs(L) * ds + U * t + C_EXP * U) + U
    return {"alpha": np.where(live, alpha, 0.0), "bound": np.where(live, bound, 0.0), "decided": decided, "masked": ~live,
            "alpha_live": alpha, "bound_live": bound, "sigma": sigma}


def check_alpha(got, ref, k=K_MARCH):
    """Held to k x the law; an undecided mask point may be either the live value or exactly 0."""
    got = f32(got).reshape(-1).astype(np.float64)
    err = np.abs(got - ref["alpha"])
    ok = err <= k * ref["bound"]
    und = ~ref["decided"]
    ok |= und & ((got == 0) | (np.abs(got - ref["alpha_live"]) <= k * ref["bound_live"]))
    ok &= np.isfinite(got)
    dec = ref["decided"] & (ref["bound"] > 0)
    ratio = float((err[dec] / ref["bound"][dec]).max()) if dec.any() else 0.0
    if np.any(ref["decided"] & (ref["bound"] == 0) & (err != 0)):
        ratio = math.inf
    return {"bad": np.nonzero(~ok)[0], "ratio": ratio, "undecided": int(und.sum())}


# ---- host chain: updateAlphaMask -> shrink -> upsample_volume_grid -> filtering_rays ------------------------------------------------------------
FACTOR_KEYS = tuple("%s_%s.%d" % (kind, what, i) for kind in ("density", "app") for what in ("plane", "line") for i in range(3))


def chain(case, params, dense_alpha, lins, rays, n_samples):
    """Everything downstream of a dense alpha [gx,gy,gz] (the device's own, itself held to check_alpha): the volume and box, the new
    aabb, the cropped factors with their aabb and grid (the oracle's shrink_field, slicing and float32 index arithmetic), and the
    filter's decisions on the shrunk, resized field with the mask on the OLD box. The resized factors are checked one by one with
    check_resize against the cropped ones."""
    cfg0 = O.FieldConfig(aabb=case["aabb"], grid_size=case["grid"], near_far=case["near_far"])
    vol, box = alpha_volume(dense_alpha, case["thres"])
    new_aabb = box_to_aabb(case["aabb"], lins, box)
    cropped, s_aabb, s_grid = O.shrink_field(cfg0, O.params_from_numpy(params), torch.from_numpy(new_aabb), mask_grid=list(case["mask_grid"]))
    cfg1 = O.FieldConfig(aabb=s_aabb.tolist(), grid_size=case["upsample"], near_far=case["near_far"], alpha_volume=torch.from_numpy(vol),
                         alpha_aabb=case["aabb"])
    return {"volume": vol, "box": box, "new_aabb": new_aabb, "cropped": {k: cropped[k].numpy() for k in FACTOR_KEYS},
            "shrunk_aabb": s_aabb.numpy(), "shrunk_grid": [int(x) for x in s_grid], "cfg": cfg1,
            "filter": filter_alpha(cfg1, rays, n_samples)}
