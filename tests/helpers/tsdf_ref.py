"""numpy float64 restatement of the TSDF stages (csrc/t2n_tsdf.hip, t2n_mesh_select_faces; definitions in include/t2n.h) in exactly
their order of operations, the float32 state rounded after every view; and the small analytic scenes the tests run them on. Every
numpy expression below is one IEEE operation per written operation (ufuncs do not contract), np.sqrt and / are correctly rounded: the
device is asked for these bits.

    world_to_camera   c2w poses -> [V,12] float64 (each 4x4 inverted by numpy, as text2nerf_amd.tsdf.world_to_camera does)
    integrate         the view loop over all nodes at once; `mutate` breaks one rule (MUTATIONS) for the checker's own tests
    face_flags        the observed-cells rule; select_faces: the order-preserving compaction; sample_colors: trilinear over observed corners
    mesh              the whole of tsdf_mesh: mc_ref.marching_cubes(-tsdf), flags, selection, colours, mesh_smooth_ref.vertex_normals
    sphere_scene      a sphere seen by pinhole cameras: depth maps from the closed-form ray hit in both depth kinds, 0 where the ray misses"""
import math

import numpy as np

from tests.helpers import mc_ref
from tests.helpers import mesh_smooth_ref as S

f32, f64 = np.float32, np.float64
MUTATIONS = ("views_reversed", "pixel_centre", "double_state")      # integrate's; face_flags has "first_vertex"


def world_to_camera(poses):
    p = np.asarray(poses)
    out = np.zeros((p.shape[0], 12), f64)
    for v in range(p.shape[0]):
        m = np.eye(4, dtype=f64)
        m[:3] = p[v, :3].astype(f64)
        out[v] = np.linalg.inv(m)[:3].reshape(12)
    return out


def fresh(shape, color=False):
    """An untouched volume: tsdf 1, weight 0, colour 0."""
    shape = tuple(shape)
    return np.ones(shape, f32), np.zeros(shape, f32), np.zeros(shape + (3,), f32) if color else None


def _frame(origin, spacing):
    return [f64(f32(t)) for t in origin], [f64(f32(t)) for t in spacing]


def integrate(state, depth, rgb, pw, w2c, intrinsic, origin, spacing, trunc, near=0.0, max_weight=math.inf, kind=0, mutate=None):
    """(tsdf, weight, color) after the views of depth [V,H,W] (rgb [V,H,W,3] or None, pw [V,H,W] or None), float32; the inputs are not
    modified."""
    T, Wt, Cl = state
    work = f64 if mutate == "double_state" else f32
    T, Wt = T.astype(work), Wt.astype(work)
    Cl = None if Cl is None else Cl.astype(work)
    depth = np.asarray(depth, f32)
    V, H, W = depth.shape
    fx, fy, cx, cy = (f64(t) for t in intrinsic)
    o, s = _frame(origin, spacing)
    idx = np.indices(T.shape)
    x = [o[k] + idx[k].astype(f64) * s[k] for k in range(3)]
    trunc, near, max_weight = f64(trunc), f64(near), f64(max_weight)
    order = range(V - 1, -1, -1) if mutate == "views_reversed" else range(V)
    with np.errstate(all="ignore"):
        for v in order:
            M = np.asarray(w2c[v], f64).reshape(3, 4)
            p = [((M[k, 0] * x[0] + M[k, 1] * x[1]) + M[k, 2] * x[2]) + M[k, 3] for k in range(3)]
            ok = p[2] > near
            u = (fx * p[0]) / p[2] + cx
            w_ = (fy * p[1]) / p[2] + cy
            ok &= (u >= 0) & (u < W) & (w_ >= 0) & (w_ < H)
            shift = 0.5 if mutate == "pixel_centre" else 0.0
            i = np.clip(np.floor(np.where(ok, u, 0.0) - shift), 0, W - 1).astype(np.int64)
            j = np.clip(np.floor(np.where(ok, w_, 0.0) - shift), 0, H - 1).astype(np.int64)
            d = depth[v][j, i]
            ok &= np.isfinite(d) & (d > 0)
            wt = np.ones(T.shape, f64)
            if pw is not None:
                q = np.asarray(pw, f32)[v][j, i]
                ok &= np.isfinite(q) & (q > 0)
                wt = np.where(ok, q.astype(f64), 1.0)
            r = np.sqrt((p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]) if kind == 0 else p[2]
            sdf = d.astype(f64) - r
            ok &= ~(sdf < -trunc)
            sv = np.minimum(1.0, sdf / trunc)
            Wo = Wt.astype(f64)
            Wn = Wo + wt
            T = np.where(ok, ((Wo * T.astype(f64) + wt * sv) / Wn).astype(work), T)
            if Cl is not None:
                c = np.asarray(rgb, f32)[v][j, i].astype(f64)
                Cl = np.where(ok[..., None], ((Wo[..., None] * Cl.astype(f64) + wt[..., None] * c) / Wn[..., None]).astype(work), Cl)
            Wt = np.where(ok, np.minimum(Wn, max_weight).astype(work), Wt)
    return T.astype(f32), Wt.astype(f32), None if Cl is None else Cl.astype(f32)


def _cells(g, n):
    """clamp(floor(g), 0, n - 2) per axis, a NaN giving 0; g [m,3] float64."""
    fl = np.floor(g)
    top = np.asarray(n, f64) - 2.0
    return np.where(fl >= top, top, np.where(fl > 0.0, fl, 0.0)).astype(np.int64)


def face_flags(verts, faces, weight, origin, spacing, min_weight=0.0, mutate=None):
    """keep [F] uint8: all eight corners of the cell that holds the face's centroid have weight > min_weight."""
    v = np.asarray(verts, f32).astype(f64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    o, s = _frame(origin, spacing)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    cen = a if mutate == "first_vertex" else ((a + b) + c) / 3.0
    cell = _cells((cen - np.array(o)) / np.array(s), weight.shape)
    seen = np.asarray(weight, f32).astype(f64) > f64(min_weight)
    keep = np.ones(len(f), bool)
    for q in range(8):
        keep &= seen[cell[:, 0] + (q >> 2 & 1), cell[:, 1] + (q >> 1 & 1), cell[:, 2] + (q & 1)]
    return keep.astype(np.uint8)


def select_faces(verts, faces, normals, colors, keep):
    """(verts, faces, normals, colors) of the flagged faces: unreferenced vertices leave, orders stay, faces are re-indexed."""
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    k = np.asarray(keep).reshape(-1) != 0
    V = len(verts)
    used = np.zeros(V, bool)
    used[f[k].reshape(-1)] = True
    new = (np.cumsum(used) - 1).astype(np.int32)
    rows = lambda x: None if x is None else np.ascontiguousarray(np.asarray(x)[used])     # noqa: E731
    return rows(verts), np.ascontiguousarray(new[f[k]]).reshape(-1, 3).astype(np.int32), rows(normals), rows(colors)


def sample_colors(verts, weight, color, origin, spacing, min_weight=0.0):
    """[V,3] uint8: trilinear over the observed corners of every vertex's cell, corners in the order axis 2 fastest."""
    v = np.asarray(verts, f32).astype(f64).reshape(-1, 3)
    o, s = _frame(origin, spacing)
    g = (v - np.array(o)) / np.array(s)
    cell = _cells(g, weight.shape)
    fr = np.clip(g - cell.astype(f64), 0.0, 1.0)
    seen = np.asarray(weight, f32).astype(f64) > f64(min_weight)
    col = np.asarray(color, f32)
    sw = np.zeros(len(v), f64)
    sc = np.zeros((len(v), 3), f64)
    for q in range(8):
        d = (q >> 2 & 1, q >> 1 & 1, q & 1)
        node = tuple(cell[:, k] + d[k] for k in range(3))
        a = [fr[:, k] if d[k] else 1.0 - fr[:, k] for k in range(3)]
        wq = np.where(seen[node], (a[0] * a[1]) * a[2], 0.0)
        on = seen[node]
        sw = np.where(on, sw + wq, sw)
        sc = np.where(on[:, None], sc + wq[:, None] * col[node].astype(f64), sc)
    with np.errstate(all="ignore"):
        out = np.where((sw > 0.0)[:, None], sc / np.where(sw > 0.0, sw, 1.0)[:, None], 0.0)
    return np.rint(np.clip(out, 0.0, 1.0) * 255.0).astype(np.uint8)       # np.rint rounds half to even


def mesh(state, origin, spacing, min_weight=0.0, normals=True, colors=True, mutate=None):
    """tsdf_mesh on the reference: (verts, faces, normals or None, colors or None) and the flags over the unfiltered faces."""
    T, Wt, Cl = state
    verts, faces, _ = mc_ref.marching_cubes(-np.asarray(T, f32), 0.0, spacing=spacing, origin=origin, normals=False)
    keep = face_flags(verts, faces, Wt, origin, spacing, min_weight, mutate)
    v, f, _, _ = select_faces(verts, faces, None, None, keep)
    c = sample_colors(v, Wt, Cl, origin, spacing, min_weight) if colors and Cl is not None else None
    n = S.vertex_normals(v, f) if normals else None
    return (v, f, n, c), keep, (verts, faces)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def look_pose(yaw=0.0, pitch=0.0, center=(0.0, 0.0, 0.0)):
    """OpenCV-convention c2w [4,4] float64 (x right, y down, z forward): yaw about y, then pitch about x."""
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    m = np.eye(4)
    m[:3, :3] = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    m[:3, 3] = center
    return m


def sphere_depth(pose, intrinsic, H, W, centre, radius, kind):
    """[H,W] float32 depth of the sphere from the pinhole camera `pose` through the pixel centres (i + 0.5, j + 0.5): the nearer root of
    |o + t d - c|^2 = r^2 with |d| = 1 (kind 0: t, the distance along the ray; kind 1: t d_z in camera space), 0 where the ray misses."""
    fx, fy, cx, cy = intrinsic
    i, j = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5, indexing="xy")
    dc = np.stack([(i - cx) / fx, (j - cy) / fy, np.ones_like(i)], -1)
    dc /= np.linalg.norm(dc, axis=-1, keepdims=True)
    dw = dc @ pose[:3, :3].T
    oc = pose[:3, 3] - np.asarray(centre, f64)
    b = dw @ oc
    disc = b * b - (oc @ oc - radius * radius)
    t = -b - np.sqrt(np.maximum(disc, 0.0))
    hit = (disc > 0) & (t > 0)
    return np.where(hit, t * (dc[..., 2] if kind == 1 else 1.0), 0.0).astype(f32)


SPHERE = dict(shape=(37, 21, 45), origin=(-1.8, -1.0, -2.2), spacing=(0.1, 0.1, 0.1), centre=(0.05, -0.03, 0.1), radius=0.8, trunc=0.3,
              H=24, W=33, intrinsic=(40.0, 40.0, 16.5, 12.0))
# three cameras in front of the sphere (all of them see its near cap: some node integrates every view) ...
FRONT_POSES = (look_pose(0.0, 0.0, (0.0, 0.0, -3.6)), look_pose(0.22, 0.03, (-0.8, -0.1, -3.4)), look_pose(-0.2, -0.04, (0.75, 0.15, -3.5)))
# ... one INSIDE the grid (nodes behind it have p_z <= near) and one that faces away from the grid (it updates nothing)
INSIDE_POSE = look_pose(0.05, 0.0, (0.0, 0.0, -1.6))
AWAY_POSE = look_pose(math.pi, 0.0, (0.1, 0.0, -3.5))


def sphere_scene(shape=None, poses=FRONT_POSES, kind=0, seed=0):
    """The committed scene as a dict: frame, intrinsic, poses [V,4,4], w2c, depth [V,H,W] of `kind`, rgb [V,H,W,3] and pixel weights
    [V,H,W] (both random, float32). `shape` replaces the grid's node counts (same origin and spacing)."""
    sc = dict(SPHERE)
    if shape is not None:
        sc["shape"] = tuple(shape)
    poses = np.stack(poses)
    rng = np.random.default_rng(seed)
    V, H, W = len(poses), sc["H"], sc["W"]
    sc.update(poses=poses, w2c=world_to_camera(poses), kind=kind,
              depth=np.stack([sphere_depth(p, sc["intrinsic"], H, W, sc["centre"], sc["radius"], kind) for p in poses]),
              rgb=rng.random((V, H, W, 3), dtype=f32), pw=(0.25 + 1.5 * rng.random((V, H, W), dtype=f32)).astype(f32))
    return sc


def with_bad_pixels(sc, seed=1):
    """A copy of the scene whose hit pixels also hold a negative, a NaN and +inf depth, and whose pixel weights hold 0 and NaN (the
    misses already hold depth 0): none of them is a measurement."""
    out = dict(sc)
    d, pw = sc["depth"].copy(), sc["pw"].copy()
    rng = np.random.default_rng(seed)
    for v in range(d.shape[0]):
        hit = np.argwhere(d[v] > 0)
        if len(hit) < 8:
            continue
        pick = hit[rng.choice(len(hit), 8, replace=False)]
        for (j, i), val in zip(pick[:4], (-0.7, np.nan, np.inf, 0.0)):
            d[v, j, i] = val
        for (j, i), val in zip(pick[4:], (0.0, np.nan, -1.0, np.inf)):
            pw[v, j, i] = val
    out.update(depth=d, pw=pw)
    return out


def run(sc, color=True, weights=False, max_weight=math.inf, state=None, views=None, mutate=None, near=0.0):
    """integrate() over the scene's views (or the index list `views`) from `state` (default: a fresh volume)."""
    sel = list(range(len(sc["depth"]))) if views is None else list(views)
    st = fresh(sc["shape"], color) if state is None else state
    return integrate(st, sc["depth"][sel], sc["rgb"][sel] if color else None, sc["pw"][sel] if weights else None, sc["w2c"][sel],
                     sc["intrinsic"], sc["origin"], sc["spacing"], sc["trunc"], near, max_weight, sc["kind"], mutate)


def sphere_distance(verts, sc):
    """Signed distance of every vertex to the scene's sphere (negative inside), float64."""
    return np.linalg.norm(np.asarray(verts, f64) - np.asarray(sc["centre"], f64), axis=-1) - sc["radius"]


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
