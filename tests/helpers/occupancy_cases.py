"""The case table of tests/test_occupancy_{cpu,gpu}.py: every input is made here from fixed seeds, in numpy, so that the CPU file can
check the claims (each case reaches the edge it names, the directed ones are decided by the reference alone, the seeded ones leave at
most 2 % undecided) before any kernel runs. Directed coordinates are dyadic so that the float32 arithmetic on them is exact."""
import functools

import numpy as np

from oracle import oracle_torch as O

F32 = np.float32
UNDECIDED_CAP = 0.02


def _rng(seed):
    return np.random.default_rng(seed)


# ---- t2n_alpha_volume --------------------------------------------------------------------------------------------------------------------
BIG = (13, 15, 16)        # 3120 nodes: 13 workgroups of 256, the last with 48 threads
LASTWG = (60, 51, 1)      # 3060 nodes: 12 workgroups, the last with 244 threads
HOT = F32(0.3)


def _single(grid, nodes, value=F32(0.9), seed=5):
    """Background in [-0.5, 0.2) (below every threshold used with it, some below 0), `nodes` set to `value`."""
    d = _rng(seed).uniform(-0.5, 0.2, grid).astype(F32)
    for n in nodes:
        d[n] = value
    return d


@functools.lru_cache(maxsize=None)
def volume_cases():
    c = {}
    for i, g in enumerate([(1, 1, 1), (1, 5, 7), (2, 2, 2), (17, 1, 3), (7, 11, 13)]):
        c["random_%dx%dx%d" % g] = dict(dense=_rng(20 + i).uniform(-0.5, 1.5, g).astype(F32), thres=0.7)      # below 0 and above 1
    c["tail_257"] = dict(dense=_single((257, 1, 1), [(256, 0, 0)]), thres=0.5, hot=[(256, 0, 0)])
    c["corner"] = dict(dense=_single(BIG, [(0, 0, 0)]), thres=0.5, hot=[(0, 0, 0)])
    c["far_corner"] = dict(dense=_single(BIG, [(12, 14, 15)]), thres=0.5, hot=[(12, 14, 15)])
    c["face"] = dict(dense=_single(BIG, [(6, 0, 8)]), thres=0.5, hot=[(6, 0, 8)])
    c["interior"] = dict(dense=_single(BIG, [(6, 7, 8)]), thres=0.5, hot=[(6, 7, 8)])
    c["last_workgroup"] = dict(dense=_single(LASTWG, [(30, 49, 0)]), thres=0.5, hot=[(30, 49, 0)])
    c["two_workgroups"] = dict(dense=_single(BIG, [(1, 1, 1), (11, 13, 14)]), thres=0.5, hot=[(1, 1, 1), (11, 13, 14)])
    c["above_one"] = dict(dense=_single(BIG, [(6, 7, 8)], value=F32(7.5)), thres=1.0, hot=[(6, 7, 8)])        # clamps to 1 >= 1
    below = np.nextafter(HOT, F32(0))
    d = _single(BIG, [(2, 3, 4)], value=HOT)
    d[9, 10, 11] = below
    c["at_threshold"] = dict(dense=d, thres=float(HOT), hot=[(2, 3, 4)])
    c["ulp_below_threshold"] = dict(dense=_single(BIG, [(2, 3, 4)], value=below), thres=float(HOT), hot=[])
    c["thres_zero"] = dict(dense=_single((5, 6, 7), []), thres=0.0)
    c["thres_above_one"] = dict(dense=_rng(31).uniform(-0.5, 2.0, (5, 6, 7)).astype(F32), thres=1.5)
    return c


def neighbourhood(grid, hot):
    """The clipped 3x3x3 neighbourhoods of the hot nodes as a [gz,gy,gx] 0 / 1 array."""
    v = np.zeros(grid[::-1], F32)
    for (x, y, z) in hot:
        v[max(z - 1, 0):z + 2, max(y - 1, 0):y + 2, max(x - 1, 0):x + 2] = 1
    return v


# ---- t2n_upsample_bilinear ------------------------------------------------------------------------------------------------------------------
RESIZE_PAIRS = [((1, 1), (5, 1)), ((4, 1), (10, 1)), ((5, 7), (5, 7)), ((2, 2), (9, 33)), ((4, 6), (10, 16)), ((24, 20), (47, 39)),
                ((9, 7), (4, 3)), ((6, 5), (1, 1))]
RESIZE_CHANNELS = (1, 3, 48)
# pairs that claim output indices with an integer source index strictly inside the grid: (along H, along W)
RESIZE_INTEGER = {((4, 1), (10, 1)): (True, False), ((4, 6), (10, 16)): (True, True), ((24, 20), (47, 39)): (True, True),
                  ((9, 7), (4, 3)): (False, True)}


def resize_input(C, hin, win, seed=0):
    """Alternating +-1000 with patches of ~1e-3 values: large neighbouring differences next to small magnitudes. No zero (and so no
    -0.0, which a sum with +0 does not copy)."""
    r = _rng(1000 + 97 * C + 13 * hin + win + seed)
    c, y, x = np.meshgrid(np.arange(C), np.arange(hin), np.arange(win), indexing="ij")
    v = 1000.0 * (1 - 2 * ((x + y + c) % 2)) * r.uniform(0.5, 1.0, (C, hin, win))
    small = r.uniform(size=v.shape) < 0.3
    v[small] = 1e-3 * r.uniform(0.25, 1.0, int(small.sum())) * np.sign(r.uniform(-1, 1, int(small.sum())))
    return v.astype(F32)


# ---- t2n_alpha_at ---------------------------------------------------------------------------------------------------------------------------
FIELD_AABB = [[-8.0, -6.0, -7.0], [8.0, 7.0, 6.5]]
MASK_BOXES = {"same": FIELD_AABB, "larger": [[-10.0, -9.0, -8.5], [11.0, 9.0, 9.25]], "offset": [[-5.0, -1.5, -7.5], [9.5, 10.0, 2.0]]}
MASK_DIMS = [(5, 7, 11), (3, 1, 4)]          # [aD][aH][aW]


def mask_volume(dims, kind):
    """binary: the x slabs [0, W // 3] and the last x node occupied over all y, z (so that every node but the two x columns next to a
    slab is either occupied or two cells away from one); real: seeded values in [-1, 2)."""
    D, H, W = dims
    if kind == "real":
        return _rng(77 + W).uniform(-1.0, 2.0, dims).astype(F32)
    v = np.zeros(dims, F32)
    v[:, :, :W // 3 + 1] = 1
    v[:, :, W - 1] = 1
    return v


def _undecidable_columns(dims):
    W = dims[2]
    return {W // 3 + 1, W - 2} - set(range(W // 3 + 1)) - {W - 1}


def mask_points(dims, box, seed=3):
    """(directed [n,3], cloud [m,3]) float32 world points."""
    a = np.asarray(box, np.float64)
    D, H, W = dims
    S = (W, H, D)
    skip = _undecidable_columns(dims)

    def world(ix, iy, iz):       # index coordinates -> world (axes of length 1: the box centre)
        f = [np.asarray(i, np.float64) / max(s - 1, 1) if s > 1 else np.full(np.shape(i), 0.5) for i, s in zip((ix, iy, iz), S)]
        return np.stack([a[0, k] + (a[1, k] - a[0, k]) * f[k] for k in range(3)], -1)

    xs = [x for x in range(W) if x not in skip]
    gx, gy, gz = np.meshgrid(xs, np.arange(H), np.arange(D), indexing="ij")
    nodes = world(gx.ravel(), gy.ravel(), gz.ravel())
    mx, my, mz = np.meshgrid(np.arange(W - 1) + 0.5, np.arange(max(H - 1, 1)) + 0.5 * (H > 1), np.arange(D - 1) + 0.5, indexing="ij")
    mids = world(mx.ravel(), my.ravel(), mz.ravel())
    inner = world(0.3 * (W - 1), 0.6 * (H - 1), 0.45 * (D - 1)).astype(F32)      # inside the first slab's support
    faces = []
    for k in range(3):
        for side in (0, 1):
            f = F32(a[side, k])
            out_dir = F32(-np.inf) if side == 0 else F32(np.inf)
            for val in (f, np.nextafter(f, -out_dir), np.nextafter(f, out_dir)):
                p = inner.copy()
                p[k] = val
                faces.append(p)
    size = a[1] - a[0]
    far = np.array([a[0] - 3 * size, a[1] + 3 * size, [a[0, 0] - 50 * size[0], inner[1], inner[2]], [inner[0], a[1, 1] + 1e4, inner[2]]])
    if H == 1:       # a length-1 axis: the coordinate along it does not matter, however far away
        far = np.concatenate([far, [[inner[0], a[1, 1] + 100 * size[1], inner[2]], [inner[0], a[0, 1] - 100 * size[1], inner[2]]]])
    directed = np.concatenate([nodes, mids, np.asarray(faces, np.float64), far]).astype(F32)
    r = _rng(seed + W)
    cloud = (a[0] - 0.6 * size + r.uniform(size=(1500, 3)) * 2.2 * size).astype(F32)
    return directed, cloud


# ---- the ray filters -------------------------------------------------------------------------------------------------------------------------
# Field A: cube [-4, 4]^3, grid 9^3 (unit cells), step_ratio 2^-6 -> step 2^-6; near 1/8. Mask 9^3 on the same box (unit cells) with
# the x slab at node 6 (x = 2) occupied over all y, z: open support 1 < x < 3 for |y|, |z| < 5.
FA = dict(aabb=[[-4.0, -4.0, -4.0], [4.0, 4.0, 4.0]], grid=[9, 9, 9], near_far=[0.125, 64.0], step_ratio=2.0 ** -6)
STEP_A = 2.0 ** -6
FILTER_N = (1, 63, 64, 65, 128, 129, 256)
FILTER_COUNTS = (1, 3, 4, 5, 1027)
NAN = F32(np.nan)


def slab_mask():
    v = np.zeros((9, 9, 9), F32)
    v[:, :, 6] = 1
    return v


def blob_mask(seed=9):
    z, y, x = np.meshgrid(*[np.arange(9.0)] * 3, indexing="ij")
    v = ((x - 5.2) ** 2 + (y - 3.1) ** 2 + (z - 4.4) ** 2 < 5.0) | (_rng(seed).uniform(size=(9, 9, 9)) < 0.02)
    return v.astype(F32)


def cfg_a(volume):
    import torch
    return O.FieldConfig(aabb=FA["aabb"], grid_size=FA["grid"], near_far=FA["near_far"], step_ratio=FA["step_ratio"],
                         alpha_volume=torch.from_numpy(volume), alpha_aabb=FA["aabb"])


def filter_ks(n):
    return sorted(k for k in {0, 1, 63, 64, 65, n - 1, n} if 0 <= k <= n)


def filter_rays(n):
    """One ray along +x per k in filter_ks(n) whose first sample inside the slab's support is sample k (k == n: none is), the support's
    face half a step in front of it; then a ray that runs beside the support and one that misses the field's box altogether.
    Returns (rays [R,6] float32, want [R] bool)."""
    rows, want = [], []
    for k in filter_ks(n):
        x_start = 1.0 - STEP_A * (k - 0.5)
        rows.append([x_start - FA["near_far"][0], 0.25, -0.5, 1.0, 0.0, 0.0])
        want.append(k < n)
    rows.append([-3.0, -3.5, -0.5, 0.0, 1.0, 0.0])       # along y at x = -3: never within a cell of the slab
    rows.append([-8.0, 6.0, 0.0, 1.0, 0.0, 0.0])         # y = 6: outside the box and outside the support
    want += [False, False]
    return np.asarray(rows, F32), np.asarray(want)


def with_stride(rays, stride, fill=NAN):
    out = np.full((rays.shape[0], stride), fill, F32)
    out[:, :6] = rays[:, :6]
    return out


def tiled(rays, want, count):
    idx = np.arange(count) % rays.shape[0]
    return rays[idx], want[idx]


def oblique_rays(R=600, seed=4):
    r = _rng(seed)
    o = r.uniform(-6, 6, (R, 3))
    d = r.normal(size=(R, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.concatenate([o, d], -1).astype(F32)


# Field B (slab test): box [-4, 4] x [-2, 2] x [-1, 2], all dyadic.
FB = dict(aabb=[[-4.0, -2.0, -1.0], [4.0, 2.0, 2.0]], grid=[9, 5, 4], near_far=[0.125, 64.0], step_ratio=1.0)
BBOX_COUNTS = (1, 255, 256, 257)


def bbox_rays():
    """(rays [R,6] float32, want [R] bool, names [R])."""
    e = 2.0 ** -22            # 4 - e is the float32 number in front of 4
    rows = [
        ("graze_edge", [2, 4, 0, 1, -1, 0], False),                 # x leaves at t = 2 where y enters: t_max == t_min
        ("graze_corner", [2, 4, 0, 1, -1, 1], False),               # ... and z leaves at t = 2 too
        ("graze_face_in_plane", [-8, 2, 0, 1, 0, 0], False),        # lies in the face y = 2: that slab's interval ends at 0
        ("clip_edge_one_step", [2, 4 - e, 0, 1, -1, 0], True),      # y enters at 2 - e: t_max - t_min is one float32 step
        ("clip_corner_one_step", [2, 4 - e, 0, 1, -1, 1], True),
        ("through_corner", [6, 4, 4, -1, -1, -1], True),
        ("inside", [0.5, -0.25, 0.5, 0.25, 0.5, -1], True),
        ("away", [8, 0, 0, 1, 0, 0], True),                         # the test is on the line
        ("miss", [-8, 3, 0, 1, 0.125, 0], False),
        ("on_face_zero_dir_pos", [-4, -4, 0, 0.0, 1, 0], True),     # origin ON the face x = -4, d_x = +0: [0, 8e6] with the substitution
        ("on_face_zero_dir_neg", [-4, -4, 0, -0.0, 1, 0], True),
    ]
    inside, outside = [0.5, -0.25, 0.5], [6.0, 3.0, 4.0]
    for a in range(3):                  # travel along axis a from outside the box
        for b in range(3):
            if b == a:
                continue
            for zero, tag in ((0.0, "p"), (-0.0, "n")):
                for where, o_b in (("in", inside[b]), ("out", outside[b])):
                    o = list(inside)
                    o[a] = -8.0
                    o[b] = o_b
                    d = [zero] * 3
                    d[a] = 1.0
                    rows.append(("axis%d_zero%d%s_%s" % (a, b, tag, where), o + d, where == "in"))
    return (np.asarray([r[1] for r in rows], F32), np.asarray([r[2] for r in rows]), [r[0] for r in rows])


def bbox_seeded(R=700, seed=6):
    r = _rng(seed)
    o = r.uniform(-8, 8, (R, 3))
    d = r.normal(size=(R, 3))
    d[r.uniform(size=(R, 3)) < 0.05] = 0.0
    d[np.all(d == 0, -1)] = 1.0
    return np.concatenate([o, d], -1).astype(F32)


# ---- compute_alpha / dense alpha -------------------------------------------------------------------------------------------------------------
TINY = dict(grid=[24, 20, 16], aabb=FIELD_AABB, near_far=[0.5, 8.0])
DENSE_GRIDS = [(1, 1, 1), (3, 5, 7), (5, 3, 2), (8, 8, 1), (9, 7, 11)]      # nodes x 4 lanes: 4, 420, 120, 256 (whole block), 2772
LENGTH_SATURATE = 1.0e6


@functools.lru_cache(maxsize=None)
def tiny_params():
    from text2nerf_amd import synth
    return synth.concentrate_density(synth.make_field_params(11, TINY["grid"], density_scale=0.9, aabb=TINY["aabb"]))


def tiny_cfg(mask=None):
    """mask: None or (volume, box)."""
    import torch
    kw = {} if mask is None else dict(alpha_volume=torch.from_numpy(mask[0]), alpha_aabb=mask[1])
    return O.FieldConfig(aabb=TINY["aabb"], grid_size=TINY["grid"], near_far=TINY["near_far"], **kw)


def alpha_masks():
    return {"none": None, "same": (mask_volume((5, 7, 11), "binary"), MASK_BOXES["same"]),
            "offset": (mask_volume((5, 7, 11), "binary"), MASK_BOXES["offset"])}


def box_points():
    """The 8 corners and 6 face centres of the field's box, each coordinate on the face also one float32 step inside and outside, and
    a seeded cloud over 1.2 x the box."""
    a = np.asarray(TINY["aabb"], np.float64)
    mid = ((a[0] + a[1]) / 2 + [0.37, -0.21, 0.13])
    pts = []
    for cx in (0, 1):
        for cy in (0, 1):
            for cz in (0, 1):
                pts.append([a[cx, 0], a[cy, 1], a[cz, 2]])
    pts = [np.asarray(p, F32) for p in pts]
    for k in range(3):
        for side in (0, 1):
            f = F32(a[side, k])
            out_dir = F32(-np.inf) if side == 0 else F32(np.inf)
            for val in (f, np.nextafter(f, -out_dir), np.nextafter(f, out_dir)):
                p = mid.astype(F32)
                p[k] = val
                pts.append(p)
    corner_out = np.array([np.nextafter(F32(a[0, 0]), F32(-np.inf)), np.nextafter(F32(a[1, 1]), F32(np.inf)),
                           np.nextafter(F32(a[1, 2]), F32(np.inf))], F32)
    pts.append(corner_out)
    size = a[1] - a[0]
    cloud = (a[0] - 0.1 * size + _rng(8).uniform(size=(800, 3)) * 1.2 * size).astype(F32)
    return np.asarray(pts, F32), cloud


def linspaces(g):
    import torch
    return [torch.linspace(0, 1, int(n)).numpy() for n in g]


# ---- host chain --------------------------------------------------------------------------------------------------------------------------------
CHAIN = dict(grid=[12, 10, 9], aabb=[[-3.0, -2.0, -2.5], [3.5, 2.5, 2.0]], near_far=[0.25, 16.0], mask_grid=(11, 9, 7), upsample=[17, 13, 12],
             thres=1e-3)


@functools.lru_cache(maxsize=None)
def chain_params():
    from text2nerf_amd import synth
    return synth.concentrate_density(synth.make_field_params(23, CHAIN["grid"], density_scale=0.9, aabb=CHAIN["aabb"]))


def chain_rays(R=300, seed=12):
    r = _rng(seed)
    o = np.asarray([0.2, -6.0, 0.1]) + r.normal(scale=0.3, size=(R, 3))
    t = r.uniform(-1, 1, (R, 3)) * [4.5, 1.0, 3.5]
    d = t - o
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.concatenate([o, d], -1).astype(F32)
