"""ORACLE (test infrastructure — NOT the product): CPU restatement of Text2NeRF's TensoRF VM-split
ray-marching path in plain PyTorch tensor arithmetic.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import this
module, and only as the checker. The shipped renderer (text2nerf_amd) never imports it.

Parity status: PINNED. Every function below is checked against golden vectors produced by importing the
reference itself on CPU (tests/golden/make_golden.py -> tests/golden/*.npz; tests/test_oracle_golden.py).
The arithmetic lives in a third-party dependency of the reference (PyTorch ATen, pinned
torch==1.13.1+cu116, requirements.txt:164): ``F.grid_sample`` (bilinear, zeros padding,
align_corners=True), ``F.softplus``, ``torch.cumprod``, ``nn.Linear``. Those are restated here as
explicit floor / tap-gather / lerp arithmetic (no grid_sample call), following the published ATen
algorithm: unnormalise ``((g+1)/2)*(size-1)``, corner = floor, weights by subtraction, out-of-range taps
contribute zero.

Each function cites the reference lines it follows. Everything is float32 unless ``dtype`` says
otherwise (float64 runs are used by tests to size tolerances).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence

import torch

MAT_MODE = ((0, 1), (0, 2), (1, 2))   # models/tensorBase.py:190
VEC_MODE = (2, 1, 0)                  # models/tensorBase.py:191

# models/sh.py:4-14 (degree <= 2 constants)
SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)


@dataclass
class FieldConfig:
    """Scalars that parameterise the path (models/tensorBase.py:163-231)."""
    aabb: Sequence[Sequence[float]]
    grid_size: Sequence[int]
    near_far: Sequence[float] = (0.5, 8.0)
    density_shift: float = -10.0
    distance_scale: float = 25.0
    ray_march_weight_thres: float = 1e-4
    step_ratio: float = 1.0
    fea_pe: int = 6
    view_pe: int = 6
    pos_pe: int = 6
    shading_mode: str = "MLP_Fea_noview"
    fea2dense_act: str = "softplus"
    z_gate: float = 2.0   # models/tensorBase.py:460 (hard-coded 2.)
    alpha_volume: Optional[torch.Tensor] = None   # AlphaGridMask volume [D(z), H(y), W(x)] or None (models/tensorBase.py:41-59)
    alpha_aabb: Optional[Sequence[Sequence[float]]] = None
    step_size: float = field(init=False)
    n_samples: int = field(init=False)

    def __post_init__(self):
        self.step_size, self.n_samples = update_step_size(self.aabb, self.grid_size, self.step_ratio)


def update_step_size(aabb, grid_size, step_ratio):
    """models/tensorBase.py:220-231 — all in float32 tensors like the reference."""
    a = torch.tensor(aabb, dtype=torch.float32)
    size = a[1] - a[0]
    g = torch.tensor(list(grid_size), dtype=torch.int64)
    units = size / (g - 1)
    step = torch.mean(units) * step_ratio
    diag = torch.sqrt(torch.sum(torch.square(size)))
    n = int((diag / step).item()) + 1
    return float(step.item()), n


# ------------------------------------------------------------------------------------------------
# a-1 / a-2  ray generation
# ------------------------------------------------------------------------------------------------
def ray_directions(H, W, focal, center=None, dtype=torch.float32):
    """dataLoader/ray_utils.py:24-42: pixel centres (+0.5), ((i-cx)/fx, (j-cy)/fy, 1). Not normalised."""
    xs = torch.arange(W, dtype=dtype) + 0.5
    ys = torch.arange(H, dtype=dtype) + 0.5
    i = xs[None, :].expand(H, W)
    j = ys[:, None].expand(H, W)
    cent = center if center is not None else [W / 2, H / 2]
    return torch.stack([(i - cent[0]) / focal[0], (j - cent[1]) / focal[1], torch.ones_like(i)], -1)


def normalize_directions(d):
    """dataLoader/scene_gen.py:45."""
    return d / torch.sqrt((d * d).sum(-1, keepdim=True))


def get_rays(directions, c2w):
    """dataLoader/ray_utils.py:66-87: rotate, no re-normalisation; origin broadcast."""
    c2w = torch.as_tensor(c2w, dtype=directions.dtype)
    rd = directions @ c2w[:3, :3].T
    ro = c2w[:3, 3].expand(rd.shape)
    return ro.reshape(-1, 3), rd.reshape(-1, 3)


# ------------------------------------------------------------------------------------------------
# a-5  sampling
# ------------------------------------------------------------------------------------------------
def sample_ray(cfg: FieldConfig, rays_o, rays_d, n_samples, jitter=None):
    """models/tensorBase.py:304-323. ``jitter`` [R,1] in [0,1) reproduces the train-time draw."""
    dt = rays_o.dtype
    aabb = torch.tensor(cfg.aabb, dtype=dt)
    near, far = cfg.near_far
    vec = torch.where(rays_d == 0, torch.full_like(rays_d, 1e-6), rays_d)
    rate_a = (aabb[1] - rays_o) / vec
    rate_b = (aabb[0] - rays_o) / vec
    t_min = torch.minimum(rate_a, rate_b).amax(-1).clamp(min=near, max=far)
    rng = torch.arange(n_samples, dtype=dt)[None]
    if jitter is not None:
        rng = rng.repeat(rays_d.shape[0], 1) + jitter.to(dt)
    step = torch.tensor(cfg.step_size, dtype=dt) * rng
    z = t_min[:, None] + step
    pts = rays_o[:, None, :] + rays_d[:, None, :] * z[..., None]
    outside = ((aabb[0] > pts) | (pts > aabb[1])).any(-1)
    return pts, z, ~outside


def normalize_coord(cfg: FieldConfig, xyz):
    """models/tensorBase.py:224,245-246."""
    aabb = torch.tensor(cfg.aabb, dtype=xyz.dtype)
    inv = 2.0 / (aabb[1] - aabb[0])
    return (xyz - aabb[0]) * inv - 1


def sample_alpha(cfg: FieldConfig, xyz):
    """AlphaGridMask.sample_alpha (models/tensorBase.py:52-59): 3-D grid_sample (trilinear, zeros padding,
    align_corners=True) of the occupancy volume at world points, restated as 8 explicit taps."""
    vol = cfg.alpha_volume.to(xyz.dtype)
    D, H, W = vol.shape
    a = torch.tensor(cfg.alpha_aabb, dtype=xyz.dtype)
    g = (xyz - a[0]) * (1.0 / (a[1] - a[0]) * 2) - 1
    ix, iy, iz = _unnormalize(g[..., 0], W), _unnormalize(g[..., 1], H), _unnormalize(g[..., 2], D)
    x0, y0, z0 = torch.floor(ix), torch.floor(iy), torch.floor(iz)
    fx, fy, fz = ix - x0, iy - y0, iz - z0
    x0, y0, z0 = x0.long(), y0.long(), z0.long()
    out = torch.zeros_like(ix)
    for dz, wz in ((0, 1 - fz), (1, fz)):
        for dy, wy in ((0, 1 - fy), (1, fy)):
            for dx, wx in ((0, 1 - fx), (1, fx)):
                xx, yy, zz = x0 + dx, y0 + dy, z0 + dz
                ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H) & (zz >= 0) & (zz < D)
                v = vol[zz.clamp(0, D - 1), yy.clamp(0, H - 1), xx.clamp(0, W - 1)] * ok.to(vol.dtype)
                out = out + v * (wx * wy * wz)
    return out


# ------------------------------------------------------------------------------------------------
# a-9 / a-12  factor lookup (ATen grid_sampler_2d, bilinear / zeros / align_corners=True, restated)
# ------------------------------------------------------------------------------------------------
def _unnormalize(g, size):
    return ((g + 1) / 2) * (size - 1)


def bilinear_plane(plane, gx, gy):
    """plane [1,C,H,W]; gx->W axis, gy->H axis; returns [C,V]."""
    _, C, H, W = plane.shape
    ix, iy = _unnormalize(gx, W), _unnormalize(gy, H)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    wx1, wy1 = ix - x0, iy - y0
    wx0, wy0 = 1 - wx1, 1 - wy1
    x0, y0 = x0.long(), y0.long()
    out = None
    for dy, wy in ((0, wy0), (1, wy1)):
        for dx, wx in ((0, wx0), (1, wx1)):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            v = plane[0][:, yy.clamp(0, H - 1), xx.clamp(0, W - 1)] * ok.to(plane.dtype)
            term = v * (wy * wx)
            out = term if out is None else out + term
    return out


def linear_line(line, gv):
    """line [1,C,L,1] sampled at grid (x=0, y=gv) -> [C,V] (the W=1 axis degenerates to weight 1)."""
    _, C, L, _ = line.shape
    iy = _unnormalize(gv, L)
    y0 = torch.floor(iy)
    w1 = iy - y0
    w0 = 1 - w1
    y0 = y0.long()
    out = None
    for dy, w in ((0, w0), (1, w1)):
        yy = y0 + dy
        ok = (yy >= 0) & (yy < L)
        v = line[0, :, :, 0][:, yy.clamp(0, L - 1)] * ok.to(line.dtype)
        out = v * w if out is None else out + v * w
    return out


def _cp_products(params, prefix, xyz_norm):
    """TensorCP (models/tensoRF.py:334-366): product over the three axes of the linearly interpolated line factors, [C, n]."""
    c = xyz_norm.detach()
    out = None
    for k in range(3):
        l = linear_line(params[f"{prefix}_line.{k}"], c[:, VEC_MODE[k]])
        out = l if out is None else out * l
    return out


def density_feature(params: Dict[str, torch.Tensor], xyz_norm):
    """models/tensoRF.py:205-220 (VM split); :334-349 for a CP parameter dict (no planes)."""
    if "density_plane.0" not in params:
        return _cp_products(params, "density", xyz_norm).sum(0)
    feat = torch.zeros(xyz_norm.shape[0], dtype=xyz_norm.dtype)
    c = xyz_norm.detach()
    for k in range(3):
        m0, m1 = MAT_MODE[k]
        p = bilinear_plane(params[f"density_plane.{k}"], c[:, m0], c[:, m1])
        l = linear_line(params[f"density_line.{k}"], c[:, VEC_MODE[k]])
        feat = feat + (p * l).sum(0)
    return feat


def feature2density(cfg: FieldConfig, feat):
    """models/tensorBase.py:406-410 (softplus beta=1, threshold=20)."""
    if cfg.fea2dense_act == "relu":
        return torch.relu(feat)
    x = feat + cfg.density_shift
    return torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))


def app_feature(params, xyz_norm):
    """models/tensoRF.py:223-239: [A,144] products -> basis_mat (no bias) -> [A,app_dim]; :351-366 for a CP dict."""
    if "app_plane.0" not in params:
        return _cp_products(params, "app", xyz_norm).T @ params["basis_mat.weight"].T
    c = xyz_norm.detach()
    prods = []
    for k in range(3):
        m0, m1 = MAT_MODE[k]
        p = bilinear_plane(params[f"app_plane.{k}"], c[:, m0], c[:, m1])
        l = linear_line(params[f"app_line.{k}"], c[:, VEC_MODE[k]])
        prods.append(p * l)
    x = torch.cat(prods, 0).T
    return x @ params["basis_mat.weight"].T


# ------------------------------------------------------------------------------------------------
# a-13  shading heads
# ------------------------------------------------------------------------------------------------
def positional_encoding(x, freqs):
    """models/tensorBase.py:11-17: feature-major, frequency-minor; all sines then all cosines."""
    bands = (2 ** torch.arange(freqs, dtype=torch.float32)).to(x.dtype)
    p = (x[..., None] * bands).reshape(x.shape[:-1] + (freqs * x.shape[-1],))
    return torch.cat([torch.sin(p), torch.cos(p)], -1)


def _mlp_layers(params, x, pre=None):
    """Linear-ReLU-Linear-ReLU-Linear-sigmoid; ``pre`` (a list) collects the two hidden layers' pre-activations (the ReLU inputs)."""
    p0 = x @ params["renderModule.mlp.0.weight"].T + params["renderModule.mlp.0.bias"]
    p1 = torch.relu(p0) @ params["renderModule.mlp.2.weight"].T + params["renderModule.mlp.2.bias"]
    if pre is not None:
        pre += [p0.detach(), p1.detach()]
    return torch.sigmoid(torch.relu(p1) @ params["renderModule.mlp.4.weight"].T + params["renderModule.mlp.4.bias"])


def mlp_fea_noview(params, feat, fea_pe, pre=None):
    """models/tensorBase.py:88-109."""
    x = torch.cat([feat, positional_encoding(feat, fea_pe)], -1) if fea_pe > 0 else feat
    return _mlp_layers(params, x, pre)


def sh_bases_deg2(d):
    """models/sh.py:87-112 for deg=2."""
    x, y, z = d.unbind(-1)
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return torch.stack([torch.full_like(x, SH_C0), -SH_C1 * y, SH_C1 * z, -SH_C1 * x,
                        SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.0 * zz - xx - yy),
                        SH_C2[3] * xz, SH_C2[4] * (xx - yy)], -1)


def sh_render(viewdirs, feat, pre=None):
    """models/tensorBase.py:29-33."""
    b = sh_bases_deg2(viewdirs)[:, None]
    x = (b * feat.view(-1, 3, b.shape[-1])).sum(-1) + 0.5
    if pre is not None:
        pre.append(x.detach())
    return torch.relu(x)


def mlp_view_head(cfg: FieldConfig, params, pts, viewdirs, feat, pre=None):
    """The view-dependent heads, models/tensorBase.py:62-86 (MLP_Fea), :111-135 (MLP_PE), :137-159 (MLP): the reference's
    torch.cat column order, three Linear layers with ReLU, sigmoid."""
    cols = [feat, viewdirs]
    if cfg.shading_mode == "MLP_Fea" and cfg.fea_pe > 0:
        cols.append(positional_encoding(feat, cfg.fea_pe))
    if cfg.shading_mode == "MLP_PE" and cfg.pos_pe > 0:
        cols.append(positional_encoding(pts, cfg.pos_pe))
    if cfg.view_pe > 0:
        cols.append(positional_encoding(viewdirs, cfg.view_pe))
    return _mlp_layers(params, torch.cat(cols, -1), pre)


def shade(cfg: FieldConfig, params, viewdirs, feat, pts=None, pre=None):
    """``pre``: an optional list that receives the heads' ReLU inputs (hidden pre-activations of the MLP heads, SH's pre-ReLU colours)."""
    if cfg.shading_mode == "MLP_Fea_noview":
        return mlp_fea_noview(params, feat, cfg.fea_pe, pre)
    if cfg.shading_mode in ("MLP_Fea", "MLP_PE", "MLP"):
        return mlp_view_head(cfg, params, pts, viewdirs, feat, pre)
    if cfg.shading_mode == "SH":
        return sh_render(viewdirs, feat, pre)
    if cfg.shading_mode == "RGB":
        return feat
    raise NotImplementedError(cfg.shading_mode)


# ------------------------------------------------------------------------------------------------
# a-11  transmittance
# ------------------------------------------------------------------------------------------------
def raw2alpha(sigma, dist):
    """models/tensorBase.py:19-26; sequential product like torch.cumprod."""
    alpha = 1.0 - torch.exp(-sigma * dist)
    T = torch.cumprod(torch.cat([torch.ones(alpha.shape[0], 1, dtype=alpha.dtype), 1.0 - alpha + 1e-10], -1), -1)
    return alpha, alpha * T[:, :-1], T[:, -1:]


# ------------------------------------------------------------------------------------------------
# a-4  forward, a-3 chunked harness
# ------------------------------------------------------------------------------------------------
def sample_ray_ndc(cfg: FieldConfig, rays_o, rays_d, n_samples, jitter_row=None):
    """models/tensorBase.py:293-302: ONE depth row for all rays, linspace(near, far, N) (+ jitter_row * (far - near) / N in
    train mode, jitter_row [1,N] = the captured rand_like draw); points, z [1,N], in-box mask."""
    near, far = cfg.near_far
    z = torch.linspace(near, far, n_samples).unsqueeze(0).to(rays_o)
    if jitter_row is not None:
        z = z + jitter_row.to(rays_o) * ((far - near) / n_samples)
    pts = rays_o[..., None, :] + rays_d[..., None, :] * z[..., None]
    a = torch.tensor(cfg.aabb, dtype=pts.dtype)
    out = ((a[0] > pts) | (pts > a[1])).any(dim=-1)
    return pts, z, ~out


def forward(cfg: FieldConfig, params, rays, white_bg=True, is_train=False, n_samples=-1, jitter=None,
            bg_coin: Optional[bool] = None, return_aux=False, ndc=False, geom_dtype=None):
    """models/tensorBase.py:436-507 (ndc_ray=False, alphaMask=None — the driver's configuration).

    ``jitter``: [R,1] uniform draw used when is_train. ``bg_coin``: outcome of the reference's
    ``torch.rand((1,)) < 0.5`` (only consulted when white_bg is False and is_train).
    ``geom_dtype``: the sample geometry (z values, points, normalised and grid coordinates, bilinear weights) in this dtype, as the
    reference computes it in float32, while everything that depends on the parameters runs in theirs (float64 arithmetic on the
    reference's own sample positions: a texel that many rays cross sums contributions that cancel, and there a 1e-5 change of a grid
    coordinate — one float32 ulp near 150 — moves its gradient by far more than the arithmetic under test)."""
    n = n_samples if n_samples > 0 else cfg.n_samples
    if is_train and jitter is None:
        raise ValueError("train-mode oracle needs the captured jitter draw")
    if geom_dtype is not None:
        rays = rays.to(geom_dtype)
        jitter = None if jitter is None else jitter.to(geom_dtype)
    ro, rd = rays[:, :3], rays[:, 3:6]
    if ndc:     # models/tensorBase.py:441-446 (`jitter` is then the [1,N] shared row)
        pts, z, valid = sample_ray_ndc(cfg, ro, rd, n, jitter if is_train else None)
        dists = torch.cat([z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])], -1)
        norm = torch.norm(rd, dim=-1, keepdim=True)
        dists = dists * norm
        rd = rd / norm
    else:
        pts, z, valid = sample_ray(cfg, ro, rd, n, jitter if is_train else None)
        dists = torch.cat([z[:, 1:] - z[:, :-1], torch.zeros_like(z[:, :1])], -1)
    if cfg.alpha_volume is not None and valid.any():      # models/tensorBase.py:451-456
        keep = sample_alpha(cfg, pts[valid]) > 0
        valid = valid.clone()
        valid[valid.clone()] = keep
    if not is_train:
        valid = valid & (pts[:, :, -1] > cfg.z_gate)
    fdt = pts.dtype if geom_dtype is None else next(iter(params.values())).dtype
    sigma = torch.zeros(pts.shape[:-1], dtype=fdt)
    rgb = torch.zeros(pts.shape[:2] + (3,), dtype=fdt)
    relu_pre = [] if return_aux else None
    xn = normalize_coord(cfg, pts)
    if valid.any():
        s = feature2density(cfg, density_feature(params, xn[valid]))
        sigma = _scatter(sigma, valid, s)
    alpha, weight, bg = raw2alpha(sigma, dists * cfg.distance_scale)
    app_mask = weight > cfg.ray_march_weight_thres
    if app_mask.any():
        vd = rd[:, None, :].expand(pts.shape)
        f = app_feature(params, xn[app_mask])
        c = shade(cfg, params, vd[app_mask], f, pts=xn[app_mask], pre=relu_pre)
        rgb = _scatter(rgb, app_mask, c)
    acc = weight.sum(-1)
    rgb_map = (weight[..., None] * rgb).sum(-2)
    if white_bg or (is_train and bool(bg_coin)):
        rgb_map = rgb_map + (1.0 - acc[..., None])
    rgb_raw = rgb_map
    rgb_map = rgb_map.clamp(0, 1)
    depth = (weight * z).sum(-1) + (1.0 - acc) * rays[..., -1]
    if return_aux:
        return rgb_map, depth, z, weight, dict(sigma=sigma, valid=valid, app_mask=app_mask, acc=acc, alpha=alpha, rgb_pre_clamp=rgb_raw,
                                                  relu_pre=relu_pre)
    return rgb_map, depth, z, weight


def _scatter(dst, mask, src):
    out = dst.clone()
    out[mask] = src
    return out


def render(cfg, params, rays, chunk=4096, n_samples=-1, white_bg=True, is_train=False, jitter=None):
    """renderer.py:28-42: chunk loop + cat; 5-tuple with None in slot 1."""
    outs = [[], [], [], []]
    R = rays.shape[0]
    for k in range(R // chunk + int(R % chunk > 0)):
        sl = slice(k * chunk, (k + 1) * chunk)
        o = forward(cfg, params, rays[sl], white_bg, is_train, n_samples, None if jitter is None else jitter[sl])
        for lst, t in zip(outs, o):
            lst.append(t)
    rgb, depth, z, w = [torch.cat(x) for x in outs]
    return rgb, None, depth, w, z


def tv_loss(x, weight=1.0):
    """utils.py:488-504."""
    b, c, h, w = x.shape
    count_h = c * (h - 1) * w
    count_w = c * h * (w - 1)
    h_tv = ((x[:, :, 1:, :] - x[:, :, :h - 1, :]) ** 2).sum()
    w_tv = ((x[:, :, :, 1:] - x[:, :, :, :w - 1]) ** 2).sum()
    return weight * 2 * (h_tv / count_h + w_tv / count_w) / b


def params_from_numpy(sd, dtype=torch.float32, requires_grad=False):
    out = {}
    for k, v in sd.items():
        t = torch.as_tensor(v).to(dtype).clone()
        t.requires_grad_(requires_grad)
        out[k] = t
    return out


# ------------------------------------------------------------------------------------------------
# occupancy mask maintenance and coarse-to-fine resampling
# ------------------------------------------------------------------------------------------------
def compute_alpha(cfg: FieldConfig, params, xyz_world, length=1.0):
    """models/tensorBase.py:412-434."""
    xyz = xyz_world.reshape(-1, 3)
    mask = torch.ones(xyz.shape[0], dtype=torch.bool)
    if cfg.alpha_volume is not None:
        mask = sample_alpha(cfg, xyz) > 0
    sigma = torch.zeros(xyz.shape[0], dtype=xyz.dtype)
    if mask.any():
        sigma[mask] = feature2density(cfg, density_feature(params, normalize_coord(cfg, xyz[mask])))
    return (1 - torch.exp(-sigma * length)).view(xyz_world.shape[:-1])


def dense_alpha(cfg: FieldConfig, params, grid_size):
    """models/tensorBase.py:328-344 (getDenseAlpha): nodes aabb0*(1-s) + aabb1*s, s = linspace(0,1,g) per axis."""
    g = [int(x) for x in grid_size]
    samples = torch.stack(torch.meshgrid(*[torch.linspace(0, 1, n) for n in g], indexing="ij"), -1)
    aabb = torch.tensor(cfg.aabb, dtype=torch.float32)
    dense_xyz = aabb[0] * (1 - samples) + aabb[1] * samples
    alpha = compute_alpha(cfg, params, dense_xyz.view(-1, 3), cfg.step_size).view(g)
    return alpha, dense_xyz


def alpha_volume(alpha, dense_xyz, thres):
    """models/tensorBase.py:349-368 (updateAlphaMask): clamp, transpose(0,2), 3x3x3 max pool with -inf padding restated
    as the max over 27 shifted copies, binarise, bounding box of the kept nodes. Returns (volume [gz,gy,gx], new_aabb)."""
    a = alpha.clamp(0, 1).transpose(0, 2).contiguous()
    D, H, W = a.shape
    pad = torch.full((D + 2, H + 2, W + 2), -math.inf, dtype=a.dtype)
    pad[1:-1, 1:-1, 1:-1] = a
    m = torch.full_like(a, -math.inf)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                m = torch.maximum(m, pad[dz:dz + D, dy:dy + H, dx:dx + W])
    vol = (m >= thres).to(a.dtype)
    xyz = dense_xyz.transpose(0, 2).contiguous()[vol > 0.5]
    return vol, torch.stack((xyz.amin(0), xyz.amax(0)))


def upsample_bilinear(x, h_out, w_out):
    """F.interpolate(x [1,C,H,W], size=(h_out,w_out), mode='bilinear', align_corners=True) restated (ATen
    upsample_bilinear2d): src = dst*(in-1)/(out-1), taps floor / floor+1 (clamped), weights by subtraction."""
    _, C, H, W = x.shape

    def taps(n_in, n_out):
        scale = torch.tensor((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0, dtype=torch.float32)
        src = scale * torch.arange(n_out, dtype=torch.float32)
        i0 = src.to(torch.int64)
        i1 = i0 + (i0 < n_in - 1).to(torch.int64)
        l1 = src - i0.to(torch.float32)
        return i0, i1, 1 - l1, l1

    y0, y1, h0, h1 = taps(H, h_out)
    x0, x1, w0, w1 = taps(W, w_out)
    r0, r1 = x[0][:, y0], x[0][:, y1]                         # [C, h_out, W]
    top = w0 * r0[:, :, x0] + w1 * r0[:, :, x1]
    bot = w0 * r1[:, :, x0] + w1 * r1[:, :, x1]
    return (h0[None, :, None] * top + h1[None, :, None] * bot)[None]


def upsample_field(params, res_target):
    """models/tensoRF.py:258-280 (up_sampling_VM / upsample_volume_grid) on a state_dict-shaped dict; returns a new dict."""
    out = dict(params)
    r = [int(v) for v in res_target]
    for i in range(3):
        m0, m1 = MAT_MODE[i]
        for kind in ("density", "app"):
            out[f"{kind}_plane.{i}"] = upsample_bilinear(params[f"{kind}_plane.{i}"], r[m1], r[m0])
            out[f"{kind}_line.{i}"] = upsample_bilinear(params[f"{kind}_line.{i}"], r[VEC_MODE[i]], 1)
    return out


def shrink_field(cfg: FieldConfig, params, new_aabb, mask_grid=None):
    """models/tensoRF.py:282-320: crop range per axis, cropped factors, corrected aabb and new grid size."""
    aabb = torch.tensor(cfg.aabb, dtype=torch.float32)
    grid = torch.tensor([int(g) for g in cfg.grid_size])
    units = (aabb[1] - aabb[0]) / (grid - 1)
    new_aabb = torch.as_tensor(new_aabb, dtype=torch.float32)
    t_l, b_r = (new_aabb[0] - aabb[0]) / units, (new_aabb[1] - aabb[0]) / units
    t_l, b_r = torch.round(torch.round(t_l)).long(), torch.round(b_r).long() + 1
    b_r = torch.stack([b_r, grid]).amin(0)
    out = dict(params)
    for i in range(3):
        v = VEC_MODE[i]
        m0, m1 = MAT_MODE[i]
        for kind in ("density", "app"):
            out[f"{kind}_line.{i}"] = params[f"{kind}_line.{i}"][..., t_l[v]:b_r[v], :]
            out[f"{kind}_plane.{i}"] = params[f"{kind}_plane.{i}"][..., t_l[m1]:b_r[m1], t_l[m0]:b_r[m0]]
    if mask_grid is None or not bool(torch.all(torch.tensor(mask_grid) == grid)):
        t_l_r, b_r_r = t_l / (grid - 1), (b_r - 1) / (grid - 1)
        new_aabb = torch.stack(((1 - t_l_r) * aabb[0] + t_l_r * aabb[1], (1 - b_r_r) * aabb[0] + b_r_r * aabb[1]))
    return out, new_aabb, (b_r - t_l).tolist()


def filter_rays_alpha(cfg: FieldConfig, rays, n_samples):
    """filtering_rays(bbox_only=False), models/tensorBase.py:393-395."""
    pts, _, _ = sample_ray(cfg, rays[:, :3], rays[:, 3:6], n_samples, jitter=None)
    return (sample_alpha(cfg, pts.reshape(-1, 3)).view(pts.shape[:-1]) > 0).any(-1)


# ---- bf16 factor storage (BASELINE.json configs[4]; golden G11) ------------------------------------------------------------
FACTOR_PREFIXES = ("density_plane", "density_line", "app_plane", "app_line")


def round_factors_bf16(params):
    """The 12 plane / line tensors rounded to bf16 (nearest-even) and widened back to fp32; basis_mat / MLP untouched.
    This is the field a bf16-storage render must reproduce (tests/golden/make_golden_bf16.py does the same to the
    reference's own parameters)."""
    out = {}
    for k, v in params.items():
        if k.startswith(FACTOR_PREFIXES):
            out[k] = v.detach().to(torch.bfloat16).to(torch.float32).requires_grad_(v.requires_grad)
        else:
            out[k] = v
    return out


# ---- f-2: frame post-processing of `evaluation` / `evaluation_path` ------------------------------------------------------
def jet_table_bgr():
    """OpenCV COLORMAP_JET as a [256,3] uint8 table in B,G,R order. cv2 is absent from this image, so this is a restatement
    of OpenCV's published table (imgproc/src/colormap.cpp: r,g,b = clamp(1.5 - |4x - {3,2,1}|, 0, 1) at x = i/255, scaled by
    255 and rounded half-to-even by saturate_cast) — PARITY UNPINNED for this table: entries that fall on exact .5 ties
    may differ from cv2 by one level."""
    import numpy as np
    i = np.arange(256, dtype=np.int64)
    out = np.zeros((256, 3), np.uint8)
    for ch, centre in enumerate((1, 2, 3)):           # B, G, R
        twice = np.clip(765 - 2 * np.abs(4 * i - 255 * centre), 0, 510)
        r = twice >> 1
        r = r + ((twice & 1) & (r & 1))
        out[:, ch] = r.astype(np.uint8)
    return out


def postprocess_frame(rgb, depth, near_far, push_depth=None, gt_rgb=None):
    """renderer.py:91-113 (push_depth given) / :168-176 (None) + utils.py:241-257 in numpy, as the reference runs them on
    the host. Returns (rgb8, depth8_bgr, psnr|None)."""
    import numpy as np
    rgb = np.clip(np.asarray(rgb, np.float32), 0.0, 1.0)
    d = np.asarray(depth, np.float32)
    if push_depth is not None:
        d = (d - np.float32(push_depth)) + np.float32(0.8)          # torch: two fp32 ops (renderer.py:94)
        d = np.maximum(d, 0)
    x = np.nan_to_num(d)
    mi, ma = near_far
    x = (x - np.float32(mi)) / np.float32(ma - mi + 1e-8)
    x = np.maximum(x, 0)
    with np.errstate(over='ignore', invalid='ignore'):
        y = 255 * x
    # x86 float->uint8 cast (cvttss2si + truncation): wraps modulo 256, out-of-int32-range values give 0
    idx = np.where(y < 2147483648.0, np.minimum(y, 2147483520.0).astype(np.int64) & 255, 0).astype(np.uint8)
    depth8 = jet_table_bgr()[idx]
    psnr = None
    if gt_rgb is not None:
        loss = float(np.mean((rgb.astype(np.float64) - np.asarray(gt_rgb, np.float64)) ** 2))
        psnr = -10.0 * np.log(loss) / np.log(10.0)
    rgb8 = (rgb * 255).astype(np.uint8)
    return rgb8, depth8, psnr


# ---- dda / ray_marcher (dataLoader/ray_utils.py:174-228): the AABB-clipped linspace sampler (no call sites in the driver) ----
def dda(rays_o, rays_d, bbox):
    """:174-181. bbox [2,3]. Returns (t_min [N,1], t_max [N,1])."""
    inv = 1.0 / (rays_d + 1e-6)
    t0, t1 = (bbox[0] - rays_o) * inv, (bbox[1] - rays_o) * inv
    return (torch.minimum(t0, t1).max(-1, keepdim=True)[0], torch.maximum(t0, t1).min(-1, keepdim=True)[0])


def ray_marcher(rays, n_samples=64, lindisp=False, perturb_draws=None, bbox=None):
    """:184-228 with the perturbation draws handed in (already scaled by `perturb`). Returns (xyz [N,S,3], z_vals [N,S])."""
    o, d = rays[:, 0:3], rays[:, 3:6]
    near, far = (rays[:, 6:7], rays[:, 7:8]) if bbox is None else dda(o, d, bbox)
    s = torch.linspace(0, 1, n_samples)
    z = near * (1 - s) + far * s if not lindisp else 1 / (1 / near * (1 - s) + 1 / far * s)
    z = z.expand(rays.shape[0], n_samples)
    if perturb_draws is not None:
        mid = 0.5 * (z[:, :-1] + z[:, 1:])
        upper, lower = torch.cat([mid, z[:, -1:]], -1), torch.cat([z[:, :1], mid], -1)
        z = lower + (upper - lower) * perturb_draws
    return o[:, None, :] + d[:, None, :] * z[:, :, None], z


# ---- TensorVM (models/tensoRF.py:4-136): stacked coefficients -> the VM-split parameter dict this oracle works on ----------
def vm_to_split(vm_params, density_n_comp, app_n_comp):
    """plane_coef [3, A + D, res, res], line_coef [3, A + D, res, 1] (appearance first, density last, :29-36,57-58) ->
    density_plane.k / density_line.k / app_plane.k / app_line.k; the other keys pass through."""
    out = {k: v for k, v in vm_params.items() if k not in ("plane_coef", "line_coef")}
    P, L = vm_params["plane_coef"], vm_params["line_coef"]
    for k in range(3):
        out[f"density_plane.{k}"] = P[k:k + 1, -density_n_comp:]
        out[f"density_line.{k}"] = L[k:k + 1, -density_n_comp:]
        out[f"app_plane.{k}"] = P[k:k + 1, :app_n_comp]
        out[f"app_line.{k}"] = L[k:k + 1, :app_n_comp]
    return out


def sh_bases(deg, d):
    """models/sh.py:87-133 for any degree 0..4 (sh_bases_deg2 above is the fused head's degree): [..., (deg+1)^2]."""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    one = torch.ones_like(x)
    cols = [0.28209479177387814 * one]
    if deg > 0:
        cols += [-0.4886025119029199 * y, 0.4886025119029199 * z, -0.4886025119029199 * x]
    if deg > 1:
        cols += [1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.31539156525252005 * (2.0 * zz - xx - yy),
                 -1.0925484305920792 * xz, 0.5462742152960396 * (xx - yy)]
    if deg > 2:
        cols += [-0.5900435899266435 * y * (3 * xx - yy), 2.890611442640554 * xy * z, -0.4570457994644658 * y * (4 * zz - xx - yy),
                 0.3731763325901154 * z * (2 * zz - 3 * xx - 3 * yy), -0.4570457994644658 * x * (4 * zz - xx - yy),
                 1.445305721320277 * z * (xx - yy), -0.5900435899266435 * x * (xx - 3 * yy)]
    if deg > 3:
        cols += [2.5033429417967046 * xy * (xx - yy), -1.7701307697799304 * yz * (3 * xx - yy), 0.9461746957575601 * xy * (7 * zz - 1),
                 -0.6690465435572892 * yz * (7 * zz - 3), 0.10578554691520431 * (zz * (35 * zz - 30) + 3),
                 -0.6690465435572892 * xz * (7 * zz - 3), 0.47308734787878004 * (xx - yy) * (7 * zz - 1),
                 -1.7701307697799304 * xz * (xx - 3 * yy), 0.6258357354491761 * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))]
    return torch.stack(cols, -1)


def ndc_rays(H, W, focal, near, rays_o, rays_d, blender=True):
    """dataLoader/ray_utils.py:88-105 (ndc_rays_blender, blender=True) / :107-124 (ndc_rays)."""
    s = -1.0 if blender else 1.0
    t = (-(near + rays_o[..., 2]) if blender else (near - rays_o[..., 2])) / rays_d[..., 2]
    o = rays_o + t[..., None] * rays_d
    kx, ky = s * 1.0 / (W / (2.0 * focal)), s * 1.0 / (H / (2.0 * focal))
    o0, o1 = kx * o[..., 0] / o[..., 2], ky * o[..., 1] / o[..., 2]
    o2 = 1.0 - s * 2.0 * near / o[..., 2]
    d0 = kx * (rays_d[..., 0] / rays_d[..., 2] - o[..., 0] / o[..., 2])
    d1 = ky * (rays_d[..., 1] / rays_d[..., 2] - o[..., 1] / o[..., 2])
    d2 = s * 2.0 * near / o[..., 2]
    return torch.stack([o0, o1, o2], -1), torch.stack([d0, d1, d2], -1)
