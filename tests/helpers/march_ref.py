"""Float64 reference, forward error law and checkers of the marchers' per-ray records and appearance lists (t2n_march.hip: k_march,
k_composite; t2n_march_tiles.hip: k_march_tiles, k_compact_list).

The geometry — z values, distances, box window, float32 normalised positions — is the oracle's float32 geometry (RayRef of
tests/helpers/geometry_ref.py, which the suite holds bit-equal to the kernels'); everything that depends on the factors is float64.

THE LAW. One number b_i per evaluated sample bounds, to first order, the forward error of a float32 evaluation of w_i. u = 2^-24 is one
float32 rounding (relative); an instruction of 1 ulp accuracy (v_exp_f32, v_log_f32) counts 2 u.

    feature        df = GAMMA_F A_i                       A_i = sum of |channel products|; GAMMA_F: 26 roundings (geometry_ref.py)
    activation     x = f + shift (1 rounding: u |x|)
                   ds = sigmoid(x) (df + u |x|) + C_ACT u sigma      d softplus / dx = sigmoid(x) <= softplus(x)
                   relu: ds = df
      C_EXP = 3    exp_finite: the product x log2 e is carried in two pieces (error ~2^-48); a = (ph - n) + pl rounds once (|a| <= 1/2,
                   so at most u ln 2 / 2 of the result: counted 1); v_exp_f32 (2); v_ldexp_f32 is exact
      C_LOG1P = 5  log1p_pos: v_log_f32 (2); r0 = y ln2 (1; r1 carries its error); r0 + r1 (1); the closing fma (1). The rounding of
                   1 + t is restored by the correction term, v_rcp_f32 acts on that term only
      C_ACT = C_EXP + C_LOG1P = 8
    exponent       t = sigma (dist scale): dist scale (1), the product (1):   dt = (dist scale) ds + 2 u t
    alpha          a = 1 - exp(-t):   da = exp(-t) (dt + C_EXP u) + u       the last u: the subtraction, absolute (a <= 1)
    transmittance  dT / T = sum_{j < i} (da_j + u) / (1 - a_j + 1e-10)        every sample of the row, evaluated or not (the float64
                   reference multiplies by 1 + 1e-10 where float32 multiplies by 1)
    weight         b_i = T da + a dT + u w
    acc            sum b_i + n u acc                      n evaluated samples, one addition each
    depth          sum z_i b_i + n u sum w z + |last| b_acc + u |depth|

The device is held to K b with K = 4; tests/test_march_list_cpu.py holds the float32 oracles to 1 x b (rho32).

CHECKERS. Each returns the indices of the offending rays and never asserts; `detail` of the last call holds the largest err / (K b).
`mutate` switches on one deliberate error: the arithmetic ones change the reference (RAY_MUTATIONS in RayRef, the others here), the
list ones (LIST_MUTATIONS) edit a copy of the lists handed in."""
import functools

import numpy as np
import torch

from oracle import oracle_torch as O
from tests.helpers.geometry_ref import EPS32, GAMMA_F, RayRef, params64_of

U = EPS32
K = 4
C_EXP = 3
C_LOG1P = 5
C_ACT = C_EXP + C_LOG1P
TINY32 = float(np.finfo(np.float32).tiny)

RAY_MUTATIONS = ("sigma_scale", "unscaled_dist", "last_dist", "drop_carry")
REF_MUTATIONS = RAY_MUTATIONS + ("alpha_threshold", "depth_no_last", "no_bg", "no_clamp", "skip_8", "last_twice")
LIST_MUTATIONS = ("drop_entry", "add_entry", "swap_entries", "next_position", "z_ulp", "rgb_w_ulp", "n_valid", "first")


def host(lists):
    """A lists dict (tests/helpers/march_lists.py: frame_lists plus the call's outputs) as numpy arrays."""
    return {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in lists.items()}


def subset(lists, rows):
    """The lists of the rays `rows` (ascending), entries included."""
    L = host(lists)
    n = np.where(L["slot0"] >= 0, L["ray_app"][:, 0], 0)
    start = np.cumsum(n) - n
    keep = np.concatenate([np.arange(start[r], start[r] + n[r]) for r in rows]) if len(rows) else np.zeros(0, np.int64)
    out = {}
    for k, v in L.items():
        if k in ("entries", "app_rgb"):
            out[k] = v[keep.astype(np.int64)]
        elif k == "app_ray":
            out[k] = np.repeat(np.arange(len(rows)), n[rows])
        elif isinstance(v, np.ndarray) and v.shape[:1] == n.shape:
            out[k] = v[rows]
        else:
            out[k] = v
    out["total"] = int(len(keep))
    return out


class MarchRef:
    def __init__(self, cfg, params, rays, N, bf16=False, train=False, jitter=None, mutate=None):
        assert mutate is None or mutate in REF_MUTATIONS, mutate
        self.cfg, self.mutate = cfg, mutate
        self.ray = r = RayRef(cfg, params64_of(params, bf16=bf16), rays, N, mutate=mutate if mutate in RAY_MUTATIONS else None,
                              train=train, jitter=jitter, samples=True)
        self.R, self.N = r.R, r.N
        self.thr = float(np.float32(cfg.ray_march_weight_thres))
        v = r.valid
        d = r.dist * float(np.float32(cfg.distance_scale))
        df = GAMMA_F * r.A
        if cfg.fea2dense_act == "relu":
            ds = df
        else:
            x = r.f + cfg.density_shift
            ds = 1.0 / (1.0 + np.exp(-x)) * (df + U * np.abs(x)) + C_ACT * U * r.sigma
        t = r.sigma * d
        dt = d * ds + 2 * U * t
        da = np.where(v, np.exp(-t) * (dt + C_EXP * U) + U, 0.0)
        step = (da + U) / (1.0 - r.alpha + 1e-10)
        dT_rel = np.cumsum(step, -1) - step
        self.w = r.w
        self.b = np.where(v, r.T * da + r.alpha * r.T * dT_rel + U * self.w, 0.0)
        n = v.sum(-1)
        self.acc = r.acc
        self.b_acc = self.b.sum(-1) + n * U * self.acc
        wz = (self.w * r.z).sum(-1)
        self.depth = wz if mutate == "depth_no_last" else r.depth
        self.b_depth = (np.abs(r.z) * self.b).sum(-1) + n * U * (self.w * np.abs(r.z)).sum(-1) + np.abs(r.last) * self.b_acc \
            + U * np.abs(self.depth)
        key = r.alpha if mutate == "alpha_threshold" else self.w
        self.must = v & (key > self.thr + K * self.b)
        self.absent = ~v | (key < self.thr - K * self.b)
        self.either = v & ~self.must & ~self.absent
        self.band = v & (self.w >= self.thr / 2) & (self.w <= 2 * self.thr)
        self.word = np.where(r.Lw > 0, r.first | (r.Lw << 11), 0)
        self.detail = {}

    # ---- conditions on the reference alone ----------------------------------------------------------------------------------------
    def band_stats(self):
        return {"band": int(self.band.sum()), "either": int(self.either.sum()), "below": int((self.band & (self.w < self.thr)).sum()),
                "above": int((self.band & (self.w > self.thr)).sum()), "evaluated": int(self.ray.valid.sum())}

    def n_app(self):
        return (self.ray.valid & (self.w > self.thr)).sum(-1)

    def rho(self, w, acc, depth):
        """max err / b of float32 weights rows [R,N], acc [R] and depth [R] (1 x the law)."""
        v = self.ray.valid
        ew = np.abs(np.asarray(w, np.float64) - self.w)
        out = {"w": float((ew[v] / self.b[v]).max()) if v.any() else 0.0,
               "acc": float((np.abs(np.asarray(acc, np.float64) - self.acc) / np.maximum(self.b_acc, TINY32)).max()),
               "depth": float((np.abs(np.asarray(depth, np.float64) - self.depth) / np.maximum(self.b_depth, TINY32)).max())}
        if (ew[~v] != 0).any():
            out["w"] = float("inf")
        return out

    # ---- checkers -------------------------------------------------------------------------------------------------------------------
    def check_records(self, lists, mutate=None):
        L = mutated(host(lists), mutate, self)
        ra = L["ray_app"].astype(np.int64)
        lo = self.must.sum(-1)
        hi = lo + self.either.sum(-1)
        bad = (ra[:, 1] != self.ray.nvalid) | (ra[:, 2] != self.word) | (ra[:, 0] < lo) | (ra[:, 0] > hi)
        return np.nonzero(bad)[0]

    def _match(self, ent_ray, pos):
        """Sample index of each entry: the evaluated sample of its ray with the same float32 position bits, or -1."""
        r = self.ray
        rr, ii = np.nonzero(r.valid)
        ref = np.concatenate([rr[:, None].astype(np.int64), np.ascontiguousarray(r.xn[rr, ii]).view(np.int32).astype(np.int64)], 1)
        ent = np.concatenate([ent_ray[:, None].astype(np.int64), np.ascontiguousarray(pos, np.float32).view(np.int32).astype(np.int64)], 1)
        _, inv = np.unique(np.concatenate([ref, ent]), axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        table = np.full(int(inv.max()) + 1 if inv.size else 1, -1, np.int64)
        table[inv[:len(ref)]] = ii
        return table[inv[len(ref):]]

    def check_entries(self, lists, mutate=None):
        L = mutated(host(lists), mutate, self)
        R = self.R
        listed = L["slot0"] >= 0
        n = np.where(listed, L["ray_app"][:, 0], 0).astype(np.int64)
        ent, rgb = L["entries"], L["app_rgb"]
        assert ent.shape[0] == int(n.sum()), (ent.shape, int(n.sum()))
        er = np.repeat(np.arange(R), n)
        idx = self._match(er, ent[:, :3])
        found = idx >= 0
        bad = np.zeros(R, bool)
        bad[er[~found]] = True                                                        # no evaluated sample has this position
        if "app_ray" in L:
            bad[er[L["app_ray"] != er]] = True                                          # app_ray[slot] is the ray
        same = er[1:] == er[:-1]
        bad[er[1:][same & found[1:] & found[:-1] & (idx[1:] <= idx[:-1])]] = True     # strictly increasing in sample index
        present = np.zeros((R, self.N), bool)
        present[er[found], idx[found]] = True
        bad |= listed & ((self.must & ~present) | (self.absent & present)).any(-1)    # membership
        w = ent[:, 3].astype(np.float64)
        e, i = er[found], idx[found]
        ratio = np.abs(w[found] - self.w[e, i]) / (K * self.b[e, i])
        bad[e[~(ratio <= 1.0)]] = True                                                # |w - w64| <= K b
        wbits = np.ascontiguousarray(ent[:, 3]).view(np.int32) != np.ascontiguousarray(rgb[:, 3]).view(np.int32)
        bad[er[wbits]] = True                                                         # app_rgb.w is app_pos.w
        self.detail = {"entries": int(ent.shape[0]), "w": float(ratio.max()) if ratio.size else 0.0,
                       "either_present": int((self.either & present).sum())}
        return np.nonzero(bad)[0]

    def check_acc_depth(self, acc, depth):
        ra = np.abs(np.asarray(acc, np.float64) - self.acc) / (K * np.maximum(self.b_acc, TINY32))
        rd = np.abs(np.asarray(depth, np.float64) - self.depth) / (K * np.maximum(self.b_depth, TINY32))
        self.detail = {"acc": float(ra.max()), "depth": float(rd.max())}
        return np.nonzero(~(ra <= 1.0) | ~(rd <= 1.0))[0]

    def check_weights_rows(self, weights, z_vals):
        v = self.ray.valid
        w = np.asarray(weights, np.float64)
        ratio = np.where(v, np.abs(w - self.w) / (K * np.where(v, self.b, 1.0)), 0.0)
        bad = ~(ratio <= 1.0).all(-1) | ((w != 0) & ~v).any(-1) | (np.asarray(z_vals, np.float64) != self.ray.z).any(-1)
        self.detail = {"rows": float(ratio.max())}
        return np.nonzero(bad)[0]

    def check_composite(self, lists, rgb_out, white_bg=True, mutate=None):
        """The composite of the device's own entries, colours and acc (k_composite); rays without a list slice are skipped."""
        assert mutate is None or mutate in REF_MUTATIONS, mutate
        L = host(lists)
        R = self.R
        listed = L["slot0"] >= 0
        n = np.where(listed, L["ray_app"][:, 0], 0).astype(np.int64)
        er = np.repeat(np.arange(R), n)
        k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)              # the entry's number in its ray
        rgb = L["app_rgb"].astype(np.float64)
        wk = rgb[:, 3:4].copy()
        if mutate == "skip_8":
            wk[k == 8] = 0.0
        if mutate == "last_twice":
            wk[k == n[er] - 1] *= 2.0
        c = np.zeros((R, 3))
        s = np.zeros((R, 3))
        np.add.at(c, er, wk * rgb[:, :3])
        np.add.at(s, er, np.abs(rgb[:, 3:4] * rgb[:, :3]))
        bg = 1.0 - L["acc"].astype(np.float64) if white_bg else np.zeros(R)
        if mutate != "no_bg":
            c = c + bg[:, None]
        if mutate != "no_clamp":
            c = np.clip(c, 0.0, 1.0)
        bound = (n[:, None] + 2) * U * (s + np.abs(bg)[:, None]) + U
        ratio = np.abs(np.asarray(rgb_out, np.float64) - c) / bound
        self.detail = {"composite": float(ratio[listed].max()) if listed.any() else 0.0, "bound": float(bound[listed].max()) if listed.any() else 0.0}
        return np.nonzero(listed & ~(ratio <= 1.0).all(-1))[0]


def mutated(L, mutate, ref):
    """A copy of the lists with one deliberate error (LIST_MUTATIONS); the victim is picked on the reference."""
    if mutate is None:
        return L
    assert mutate in LIST_MUTATIONS, mutate
    L = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in L.items()}
    n = np.where(L["slot0"] >= 0, L["ray_app"][:, 0], 0).astype(np.int64)
    start = np.cumsum(n) - n
    er = np.repeat(np.arange(ref.R), n)
    idx = ref._match(er, L["entries"][:, :3])
    w64 = np.where(idx >= 0, ref.w[er, np.maximum(idx, 0)], 0.0)
    if mutate in ("n_valid", "first"):
        r = int(np.nonzero(ref.ray.Lw > 1)[0][0])
        L["ray_app"][r, 1 if mutate == "n_valid" else 2] += 1
        return L
    if mutate == "drop_entry":          # the entry whose weight is nearest to 1.5 thr
        e = int(np.argmin(np.abs(w64 - 1.5 * ref.thr)))
        assert abs(w64[e] / ref.thr - 1.5) < 0.2, w64[e]
        for k in ("entries", "app_rgb", "app_ray"):
            if k in L:
                L[k] = np.delete(L[k], e, 0)
        L["ray_app"][er[e], 0] -= 1
        L["total"] -= 1
        return L
    if mutate == "add_entry":           # the evaluated sample whose weight is nearest to 0.7 thr, in its place in its ray's slice
        cand = np.where(ref.ray.valid, np.abs(ref.w - 0.7 * ref.thr), np.inf)
        cand[L["slot0"] < 0] = np.inf
        r, i = np.unravel_index(int(np.argmin(cand)), cand.shape)
        assert abs(ref.w[r, i] / ref.thr - 0.7) < 0.1, ref.w[r, i]
        at = int(start[r] + (idx[er == r] < i).sum())
        row = np.concatenate([ref.ray.xn[r, i], [np.float32(ref.w[r, i])]]).astype(np.float32)
        L["entries"] = np.insert(L["entries"], at, row, 0)
        L["app_rgb"] = np.insert(L["app_rgb"], at, np.array([0.5, 0.5, 0.5, row[3]], np.float32), 0)
        if "app_ray" in L:
            L["app_ray"] = np.insert(L["app_ray"], at, r)
        L["ray_app"][r, 0] += 1
        L["total"] += 1
        return L
    r = int(np.nonzero(n >= 2)[0][0])   # the first ray with two entries
    e = int(start[r])
    if mutate == "swap_entries":
        for k in ("entries", "app_rgb"):
            L[k][[e, e + 1]] = L[k][[e + 1, e]]
    elif mutate == "next_position":
        L["entries"][e, :3] = ref.ray.xn[r, idx[e] + 1 if idx[e] + 1 < ref.N else idx[e] - 1]
    elif mutate == "z_ulp":
        L["entries"][e, 2] = np.nextafter(L["entries"][e, 2], np.float32(2.0))
    elif mutate == "rgb_w_ulp":
        L["app_rgb"][e, 3] = np.nextafter(L["app_rgb"][e, 3], np.float32(2.0))
    return L


# ---- lists of the float32 oracle (no device) ---------------------------------------------------------------------------------------------
def oracle_lists(ref, params, rays, bf16=False, train=False, jitter=None, seed=0):
    """What a marcher would leave behind if its arithmetic were oracle_torch.forward's float32: records, entries, acc, depth, weights
    rows, and a float32 composite of colours drawn in [-0.2, 1.2] (a head without a sigmoid; k_composite takes them as given)."""
    cfg = ref.cfg
    P = O.params_from_numpy(params)
    if bf16:
        P = O.round_factors_bf16(P)
    rays_t = torch.as_tensor(np.asarray(rays, np.float32))
    jit = torch.as_tensor(np.asarray(jitter, np.float32)).reshape(-1, 1) if train else None
    with torch.no_grad():
        _, depth, z, w, aux = O.forward(cfg, P, rays_t, white_bg=True, is_train=train, n_samples=ref.N, jitter=jit, return_aux=True)
    mask = aux["app_mask"].numpy()
    rr, ii = np.nonzero(mask)
    w32 = w.numpy()
    ent = np.concatenate([ref.ray.xn[rr, ii], w32[rr, ii][:, None]], 1).astype(np.float32)
    n = mask.sum(-1)
    rng = np.random.default_rng(seed)
    col = rng.uniform(-0.2, 1.2, (ent.shape[0], 3)).astype(np.float32)
    acc = aux["acc"].numpy().astype(np.float32)
    c = np.zeros((ref.R, 3), np.float32)
    start = np.cumsum(n) - n
    for k in range(int(n.max()) if n.size else 0):
        rows = np.nonzero(n > k)[0]
        e = start[rows] + k
        c[rows] = c[rows] + ent[e, 3:4] * col[e]
    c = np.clip(c + (np.float32(1.0) - acc)[:, None], np.float32(0.0), np.float32(1.0))
    return {"acc": acc, "ray_app": np.stack([n, aux["valid"].numpy().sum(-1), ref.word], 1).astype(np.int32),
            "slot0": start.astype(np.int32), "entries": ent, "app_rgb": np.concatenate([col, ent[:, 3:4]], 1), "app_ray": rr.astype(np.int32),
            "total": int(n.sum()), "depth": depth.numpy(), "rgb_out": c, "weights": w32, "z_vals": z.numpy()}


# ---- the cases of tests/test_march_list_cpu.py and tests/test_march_list_gpu.py -----------------------------------------------------------
GRIDS = {"9x13x17": [9, 13, 17], "16x16x16": [16, 16, 16]}
FRAMES = {"8x8": (8, 8), "13x11": (13, 11), "24x16": (24, 16)}
CAMERAS = ("inside", "outside", "axis")
FIELD_SEED, FIELD_SCALE = 41, 0.8          # tests/test_march_feature_fusion.py's fields
GEOMETRY = tuple(f"{g}/{fr}/{c}" for g in GRIDS for fr in FRAMES for c in CAMERAS)
VARIANTS = tuple(f"{v}/{c}" for v in ("relu", "bf16", "mask", "sparse") for c in ("inside", "outside"))
# relu: at density_scale 0.8 a feature's A_i is ~10, so K b of a sample in front of the surface (T = 1, dist scale = 12) is above the
# threshold itself and every sample with a negative feature (w = 0) is an "either" sample: 895 of them against 28 in the band. At 0.15
# the inside frame holds 88 band samples and no "either" one (chosen on the reference alone: tests/test_march_list_cpu.py).
RELU_SCALE = 0.15
# mask: alpha_mask() of tests/test_density_cache.py (a third of its nodes empty) rejects no sample of these frames: a sample is rejected
# only where all eight nodes around it are empty. sparse: the same recipe with four fifths empty rejects 58 % of the inside frame's
# samples and leaves a gap in every ray's window.
MASK_EMPTY = {"mask": 0.35, "sparse": 0.8}
ROUTES = ("compact", "finisher", "gather", "train")
FINISHER_STRIDE = 13                        # the finisher frame's reference: every 13th ray (coprime with the width: every tile column)


def samples_of(frame):
    """N = 40 on the one-tile frame, 32 on the others: the largest of the two at which a launch of the frame gets a feature row per
    list slot (tests/test_march_feature_fusion.py::test_sizing_rule_row_per_slot), which the fused forms need."""
    return 40 if frame == "8x8" else 32


def mask_volume(kind="mask", seed=3):
    """alpha_mask() of tests/test_density_cache.py, the volume alone; MASK_EMPTY[kind] of its nodes are empty."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.random((7, 6, 5)) > MASK_EMPTY[kind]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """Everything a case needs but the device: cfg (oracle FieldConfig), params, rays, N, frame (H, W) and its switches."""
    from text2nerf_amd import synth
    from tests.conftest import GOLDEN, TINY
    from tests.test_density_cache import AABB, NEAR_FAR, camera_rays
    from tests.test_march_summed_table import pinhole_rays
    out = dict(name=name, act="softplus", bf16=False, mask=False, train=False, jitter=None, thres=1e-4, budget=0, rows=None,
               aabb=AABB, near_far=NEAR_FAR, seed=FIELD_SEED, scale=FIELD_SCALE)
    if name in GEOMETRY:
        g, fr, cam = name.split("/")
        out.update(grid=GRIDS[g], HW=FRAMES[fr], N=samples_of(fr), rays=camera_rays(cam, *FRAMES[fr]))
    elif name in VARIANTS:
        v, cam = name.split("/")
        out.update(grid=GRIDS["16x16x16"], HW=FRAMES["24x16"], N=32, rays=camera_rays(cam, 24, 16), act="relu" if v == "relu" else "softplus",
                   bf16=v == "bf16", mask=v if v in MASK_EMPTY else False, scale=RELU_SCALE if v == "relu" else FIELD_SCALE)
    elif name == "compact":        # tests/test_march_feature_fusion.py::test_rays_through_compact_list
        out.update(grid=GRIDS["16x16x16"], HW=(24, 16), N=32, rays=camera_rays("inside", 24, 16), seed=42, thres=1e-6)
    elif name == "finisher":       # tests/test_list_budget.py::test_overflowing_budget_is_detected_and_repaired
        rays = synth.frame_rays_np(256, 256, c2w=synth.look_pose(0.3, -0.1, (0.2, 0.1, -1.0)))
        out.update(grid=TINY["grid"], aabb=TINY["aabb"], near_far=TINY["near_far"], HW=(256, 256), seed=11, scale=0.9, budget=2,
                   all_rays=rays, rows=np.arange(0, rays.shape[0], FINISHER_STRIDE))
        out.update(rays=rays[out["rows"]], N=None)
    elif name == "gather":         # tests/test_march_summed_table.py::test_mixed_table_and_gather_pairs
        out.update(grid=[300] * 3, aabb=[[-8.0] * 3, [8.0] * 3], near_far=[0.5, 8.0], HW=(24, 24), N=45, seed=7,
                   rays=pinhole_rays(24, 24, 100.0, synth.look_pose(-0.15, 0.1, (0.2, -0.1, 1.9))))
    elif name == "train":          # tests/test_hip_parity.py::test_g6_forward_train_rng_stream, its first 64 rays
        import os
        rays = np.load(os.path.join(GOLDEN, "tiny.npz"), allow_pickle=False)["tiny_rays"][:64]
        torch.manual_seed(123)
        out.update(grid=TINY["grid"], aabb=TINY["aabb"], near_far=TINY["near_far"], HW=(0, 0), N=40, seed=11, scale=0.9, train=True,
                   rays=rays, jitter=torch.rand(rays.shape[0], 1).numpy().reshape(-1))
    else:
        raise KeyError(name)
    out["params"] = field_params(out["seed"], tuple(out["grid"]), out["scale"], tuple(map(tuple, out["aabb"])))
    kw = dict(alpha_volume=torch.from_numpy(mask_volume(out["mask"])), alpha_aabb=out["aabb"]) if out["mask"] else {}
    out["cfg"] = O.FieldConfig(aabb=out["aabb"], grid_size=out["grid"], near_far=out["near_far"], fea2dense_act=out["act"],
                               ray_march_weight_thres=out["thres"], **kw)
    if out["N"] is None:
        out["N"] = out["cfg"].n_samples
    return out


@functools.lru_cache(maxsize=None)
def field_params(seed, grid, scale, aabb):
    from text2nerf_amd import synth
    return synth.make_field_params(seed, list(grid), density_scale=scale, aabb=[list(a) for a in aabb])


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 reference of a case: computed once, shared by every test that needs it, never modified."""
    c = case(name)
    return MarchRef(c["cfg"], c["params"], c["rays"], c["N"], bf16=c["bf16"], train=c["train"], jitter=c["jitter"])


def mutant(name, mutate):
    c = case(name)
    return MarchRef(c["cfg"], c["params"], c["rays"], c["N"], bf16=c["bf16"], train=c["train"], jitter=c["jitter"], mutate=mutate)


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    c = case(name)
    return oracle_lists(reference(name), c["params"], c["rays"], bf16=c["bf16"], train=c["train"], jitter=c["jitter"])
