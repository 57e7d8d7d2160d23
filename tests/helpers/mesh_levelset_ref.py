"""Reference of the level-set export (TensorBase.feature_level / getDenseFeature / export_surface(surface="feature")): the level
formula, the float64 density feature at getDenseAlpha's nodes and at mesh vertices, the fields of the cases and the counted bounds.

Nodes and normalised coordinates are the kernels' own float32 values (occupancy_ref.dense_nodes and the oracle's normalize_coord, which
the suite holds bit-equal to the device); everything behind them is float64 (geometry_ref.density_grad, any component count).

Counted bounds, 2^-24 = one float32 rounding, A_f = the float64 sum of the absolute values of the feature's channel products.
  node values    |feat - f64| <= (m + 2) 2^-24 A_f, m = the float32 roundings on the kernel's longest chain:
      tuned shape (k_compute_alpha: taps_plane 7, taps_line 3, the lane's 12 fma, the quad reduction's 2 additions)          m = 24
      general shape (gen_density_feature: gen_plane 7 [w0 on two axes 2, their product 1, tap x weight 1, three fma 3],
      gen_line 3 [w0 1, product 1, fma 1], then ONE serial chain of sum(density_n_comp) fma)             m = 10 + sum(density_n_comp)
  vertices at the field's own grid, where the feature is linear along the crossed edge (a, b): in units of 2^-24
      the level           f* -> float32                                                                 1 x |f*|
      the node values     (1 - t) err_a + t err_b, A_f linear along the edge too                        (m + 2) x A_f(v)
      t                   (level - v0) / (v1 - v0): three roundings of t <= 1, df/dt = f_b - f_a          3 x (|f_a| + |f_b|)
      the position        p = index + t (1), p * spacing (1), origin + . (1), spacing itself (2: the difference of the box corners
                          and the division), each relative to a coordinate of at most g - 1 cells, and the float64 reference's own
                          map back through the box, relative to |x| <= r (g - 1) cells with r = max |aabb| / extent: (5 + r)(g - 1)
                          cells x 2^-24 on each of the three axes. Along the edge a cell is worth |f_b - f_a|; across it the two
                          other axes are taken to be worth no more than 2 A_f(v) each (neighbouring texels of the size of the
                          cell's own, which holds for these fields and is not a theorem)                 (5 + r)(g - 1) x (|f_a| + |f_b| + 4 A_f(v))
  K = 4 (5 + r)(g - 1) + m + 2 + 3 covers all of them in K 2^-24 (|f_a| + |f_b| + |f*| + A_f(v))."""
import math

import numpy as np
import torch

from oracle import oracle_torch as O
from tests.helpers import geometry_ref as G
from tests.helpers import occupancy_ref as R
from text2nerf_amd import synth

U = 2.0 ** -24
M_TUNED = 24
ALPHA_LEVEL = 0.005


def m_general(density_n_comp):
    return 10 + int(sum(density_n_comp))


def gamma(m):
    return (m + 2) * U


def vertex_K(aabb, grid, m):
    a = np.asarray(aabb, np.float64)
    r = float((np.abs(a).max(0) / (a[1] - a[0])).max())
    return int(math.ceil(4 * (5 + r) * (max(grid) - 1))) + m + 2 + 3


def feature_level(alpha_level, length, distance_scale=25.0, density_shift=-10.0, act="softplus"):
    """f* with alpha(f*) = alpha_level over `length`, in double."""
    sigma = -math.log1p(-alpha_level) / (length * distance_scale)
    if act == "relu":
        return sigma
    return sigma - density_shift if sigma > 20.0 else math.log(math.expm1(sigma)) - density_shift


def export_level(alpha_level, step, distance_scale=25.0, density_shift=-10.0, act="softplus"):
    """The level export_surface(surface="feature") hands marching cubes: getDenseAlpha's alpha is compute_alpha's 1 - exp(-sigma step),
    WITHOUT distance_scale, hence the length step / distance_scale."""
    return feature_level(alpha_level, step / distance_scale, distance_scale, density_shift, act)


def dense_alpha_of_feature(f, step, density_shift=-10.0, act="softplus"):
    """getDenseAlpha's alpha (compute_alpha: no distance_scale) of a float64 feature."""
    return alpha_of_feature(f, step, 1.0, density_shift, act)


def alpha_of_feature(f, length, distance_scale=25.0, density_shift=-10.0, act="softplus"):
    """The oracle's feature2density and the renderer's alpha formula (raw2alpha over length * distance_scale) on a float64 feature."""
    cfg = O.FieldConfig(aabb=[[-1.0] * 3, [1.0] * 3], grid_size=[3, 3, 3], density_shift=density_shift, distance_scale=distance_scale,
                        fea2dense_act=act)
    sigma = O.feature2density(cfg, torch.as_tensor(f, dtype=torch.float64))
    return 1.0 - torch.exp(-sigma * length * distance_scale)


# ---- the fields ---------------------------------------------------------------------------------------------------------------------------
SHAPES = {"tiny": dict(grid=[24, 20, 16], aabb=[[-8.0, -6.0, -7.0], [8.0, 7.0, 6.5]], near_far=[0.5, 8.0]), "37x23x29": G.GRID37}
WIDE = dict(grid=[21, 18, 15], aabb=[[-3.0, -2.5, -2.0], [3.0, 2.5, 4.0]], near_far=[0.3, 7.0], density_n_comp=[20, 20, 20])
MASK_GRID, MASK_THRES = (12, 10, 8), 0.02
BLOB_AMP = 14.0


def blob_params(shape, seed=4, **kw):
    """A weak random field (features of a few hundredths) with a blob written into density component 0: a smooth bump of height
    BLOB_AMP off the box's centre, so that one closed surface exists at every level between the noise and the bump."""
    g = shape["grid"]
    p = synth.make_field_params(seed, g, density_scale=0.05, aabb=shape["aabb"], **kw)
    bump = [np.exp(-0.5 * ((np.arange(n) - c * (n - 1)) / (0.17 * n)) ** 2).astype(np.float32) for n, c in zip(g, (0.45, 0.55, 0.5))]
    for k in range(3):
        m0, m1 = G.MAT_MODE[k]
        p[f"density_plane.{k}"][0, 0] = np.float32(0.0)
        p[f"density_line.{k}"][0, 0, :, 0] = np.float32(0.0)
    m0, m1 = G.MAT_MODE[0]
    p["density_plane.0"][0, 0] = np.outer(bump[m1], bump[m0]).astype(np.float32)
    p["density_line.0"][0, 0, :, 0] = (np.float32(BLOB_AMP) * bump[G.VEC_MODE[0]]).astype(np.float32)
    return p


def cfg_of(shape, volume=None):
    kw = {} if volume is None else dict(alpha_volume=torch.as_tensor(volume, dtype=torch.float32), alpha_aabb=shape["aabb"])
    return O.FieldConfig(aabb=shape["aabb"], grid_size=shape["grid"], near_far=shape["near_far"], **kw)


def linspaces(g):
    return [torch.linspace(0, 1, int(n)).numpy() for n in g]


def feature_at(cfg, params, pts, bf16=False):
    """f64 feature and A_f at world points [n,3]: float32 points go through the field's float32 normalisation (the kernels' cells),
    float64 points through the continuous float64 form."""
    p = torch.from_numpy(np.ascontiguousarray(pts).reshape(-1, 3))
    xn = O.normalize_coord(cfg, p)
    a32 = torch.tensor(cfg.aabb, dtype=torch.float32)
    f, _, A, _ = G.density_grad(G.params64_of(params, bf16=bf16), xn, (2.0 / (a32[1] - a32[0])).numpy(), cfg.grid_size)
    return f.numpy(), A.numpy()


def dense_feature(cfg, params, g, bf16=False):
    """What t2n_dense_feature must write on the grid g: dict of feat [n] float64 (the live value everywhere), A [n], masked [n] bool
    (the mask samples <= 0: -inf is due) and decided [n] bool (the mask decision does not hang on a rounding)."""
    nodes = R.dense_nodes(cfg.aabb, linspaces(g)).reshape(-1, 3)
    f, A = feature_at(cfg, params, nodes, bf16)
    masked, decided = np.zeros(len(nodes), bool), np.ones(len(nodes), bool)
    if cfg.alpha_volume is not None:
        r = R.mask_sample(np.asarray(cfg.alpha_volume, np.float32), cfg.alpha_aabb, nodes)
        masked, decided = ~r["hit"], r["decided"]
    return dict(feat=f, A=A, masked=masked, decided=decided, nodes=nodes)


def check_dense_feature(got, ref, m):
    """Indices of the nodes that break the rule, the largest error / bound ratio among the live nodes, the undecided count."""
    got = np.asarray(got, np.float32).reshape(-1).astype(np.float64)
    live_ok = np.abs(got - ref["feat"]) <= gamma(m) * ref["A"]
    dead_ok = np.isneginf(got)
    ok = np.where(ref["decided"], np.where(ref["masked"], dead_ok, live_ok), dead_ok | live_ok)
    live = ref["decided"] & ~ref["masked"] & (ref["A"] > 0)
    ratio = float((np.abs(got - ref["feat"])[live] / (gamma(m) * ref["A"][live])).max()) if live.any() else 0.0
    return np.nonzero(~ok)[0], ratio, int((~ref["decided"]).sum())


def vertex_edges(verts, aabb, grid):
    """The crossed grid edge of every vertex of an export at the field's own grid: the node indices [V,3] of its two ends (a below b
    on the one axis where the vertex lies between nodes; a == b for a vertex on a node)."""
    a = np.asarray(aabb, np.float32).astype(np.float64)
    p = (np.asarray(verts, np.float64) - a[0]) / ((a[1] - a[0]) / (np.asarray(grid, np.float64) - 1))
    near = np.rint(p)
    axis = np.abs(p - near).argmax(-1)
    lo = near.copy()
    rows = np.arange(len(p))
    lo[rows, axis] = np.floor(p[rows, axis])
    hi = lo.copy()
    hi[rows, axis] = np.minimum(lo[rows, axis] + 1, np.asarray(grid)[axis] - 1)
    on_node = np.abs(p - near).max(-1) < 1e-4
    hi[on_node] = lo[on_node] = near[on_node]
    return lo.astype(np.int64), hi.astype(np.int64)


def vertex_ratio(verts, cfg, params, g, level, K, node_f=None):
    """max over the vertices of |f64(v) - f*| / (K 2^-24 (|f_a| + |f_b| + |f*| + A_f(v))), and the largest |f64(v) - f*|. f64 at
    the float32 vertex through the continuous float64 form; f_a, f_b: the float64 feature at the ends of the vertex' edge."""
    v = np.asarray(verts, np.float32)
    f, A = feature_at(cfg, params, v.astype(np.float64))
    if node_f is None:
        node_f = dense_feature(cfg, params, g)["feat"]
    nf = np.asarray(node_f, np.float64).reshape(tuple(g))
    lo, hi = vertex_edges(v, cfg.aabb, g)
    fa, fb = nf[lo[:, 0], lo[:, 1], lo[:, 2]], nf[hi[:, 0], hi[:, 1], hi[:, 2]]
    err = np.abs(f - level)
    bound = K * U * (np.abs(fa) + np.abs(fb) + abs(level) + A)
    return float((err / bound).max()), float(err.max())
