"""numpy restatement of the device marching cubes (csrc/t2n_mesh.hip): the ownership scheme, the generator's table
(tools/gen_mc_table.py), float32 arithmetic in the kernels' order. Plus what the tests judge a mesh by without trusting this file:
directed-edge manifold check, Euler characteristic, signed volume; a small PLY reader; the reference's
`convert_sdf_samples_to_ply` arithmetic (utils.py:531-550) around a given marching-cubes function."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _load_generator():
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _load_generator()
_NTRI, _TRI, STATS = GEN.build_table()
NTRI = np.array(_NTRI, dtype=np.int64)                       # [256]
TRI = np.array(_TRI, dtype=np.int64)                         # [256][5][3]
EDGE_AXIS = np.array([e >> 2 for e in range(12)])
EDGE_OWNER = np.array([GEN.edge_owner_offset(e) for e in range(12)])   # [12][3]
f32 = np.float32


def _shift(a, axis):
    """a at the next node along `axis` (the last layer repeats itself; callers mask it)."""
    idx = np.minimum(np.arange(a.shape[axis]) + 1, a.shape[axis] - 1)
    return np.take(a, idx, axis=axis)


def _gradient(vol, spacing):
    """Node gradients [3][n0,n1,n2]: central differences / (2 s), one-sided / s at a border; float32 step by step."""
    out = []
    for a in range(3):
        n = vol.shape[a]
        up = np.take(vol, np.minimum(np.arange(n) + 1, n - 1), axis=a)
        dn = np.take(vol, np.maximum(np.arange(n) - 1, 0), axis=a)
        shape = [1, 1, 1]
        shape[a] = n
        inner = ((np.arange(n) > 0) & (np.arange(n) < n - 1)).reshape(shape)
        with np.errstate(all="ignore"):
            d = (up - dn).astype(f32)
            g = np.where(inner, d / (f32(2.0) * f32(spacing[a])), d / f32(spacing[a])).astype(f32)
        out.append(g)
    return out


def marching_cubes(volume, level, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), normals=True, flip=False):
    """(verts [V,3] float32, faces [F,3] int32, normals [V,3] float32 or None), vertices in node-linear order (axis 0, 1, 2 inside
    a node), triangles in cell-linear order (table order inside a cell)."""
    vol = np.ascontiguousarray(volume, dtype=f32)
    n0, n1, n2 = vol.shape
    level = f32(level)
    spacing = [f32(s) for s in spacing]
    origin = [f32(o) for o in origin]
    inside = vol > level
    n = vol.size
    strides = np.array([n1 * n2, n2, 1])
    crossed = []
    for a in range(3):
        c = inside != _shift(inside, a)
        sl = [slice(None)] * 3
        sl[a] = -1
        c[tuple(sl)] = False
        crossed.append(c.ravel())
    count = crossed[0].astype(np.int64) + crossed[1] + crossed[2]
    base = np.cumsum(count) - count
    rank = [np.zeros(n, np.int64), crossed[0].astype(np.int64), crossed[0].astype(np.int64) + crossed[1]]
    V = int(count.sum())
    verts = np.zeros((V, 3), f32)
    norms = np.zeros((V, 3), f32) if normals else None
    grad = _gradient(vol, spacing) if normals else None
    ijk = np.stack(np.unravel_index(np.arange(n), vol.shape), -1)
    flat = vol.ravel()
    for a in range(3):
        nodes = np.nonzero(crossed[a])[0]
        vid = base[nodes] + rank[a][nodes]
        v0, v1 = flat[nodes], flat[nodes + strides[a]]
        with np.errstate(all="ignore"):
            t = ((level - v0).astype(f32) / (v1 - v0).astype(f32)).astype(f32)
        t = np.fmin(np.fmax(t, f32(0)), f32(1)).astype(f32)
        p = ijk[nodes].astype(f32)
        p[:, a] = (p[:, a] + t).astype(f32)
        for c in range(3):
            verts[vid, c] = (origin[c] + (p[:, c] * spacing[c]).astype(f32)).astype(f32)
        if normals:
            with np.errstate(all="ignore"):
                g = []
                for c in range(3):
                    g0, g1 = grad[c].ravel()[nodes], grad[c].ravel()[nodes + strides[a]]
                    g.append((g0 + (t * (g1 - g0).astype(f32)).astype(f32)).astype(f32))
                ln = np.sqrt(((g[0] * g[0]).astype(f32) + (g[1] * g[1]).astype(f32)).astype(f32) + (g[2] * g[2]).astype(f32)).astype(f32)
                ok = (ln > 0) & (ln < np.inf)
                for c in range(3):
                    norms[vid, c] = np.where(ok, (-g[c]) / np.where(ok, ln, f32(1)), f32(0)).astype(f32)
    # cells, addressed by their lowest node
    cell = np.ones(vol.shape, bool)
    cell[-1, :, :] = cell[:, -1, :] = cell[:, :, -1] = False
    case = np.zeros(vol.shape, np.int64)
    for c in range(8):
        s = inside
        for a in range(3):
            if c >> a & 1:
                s = _shift(s, a)
        case |= s.astype(np.int64) << c
    case = np.where(cell, case, 0).ravel()
    ntri = NTRI[case]
    tbase = np.cumsum(ntri) - ntri
    F = int(ntri.sum())
    faces = np.zeros((F, 3), np.int32)
    for q in range(5):
        cells = np.nonzero(ntri > q)[0]
        for m in range(3):
            e = TRI[case[cells], q, m]
            owner = cells + EDGE_OWNER[e] @ strides
            a = EDGE_AXIS[e]
            r = np.where(a == 0, rank[0][owner], np.where(a == 1, rank[1][owner], rank[2][owner]))
            faces[tbase[cells] + q, m] = base[owner] + r
    if flip:
        faces = faces[:, [0, 2, 1]]
    return verts, np.ascontiguousarray(faces), norms


# ---- properties of a mesh that do not depend on the restatement -----------------------------------------------------------------
def is_closed_oriented_manifold(faces):
    """Every directed edge occurs exactly once and its opposite exactly once."""
    f = np.asarray(faces, dtype=np.int64)
    if len(f) == 0:
        return True
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    if (d[:, 0] == d[:, 1]).any():
        return False
    key = d[:, 0] * (f.max() + 1) + d[:, 1]
    rev = d[:, 1] * (f.max() + 1) + d[:, 0]
    uk, cnt = np.unique(key, return_counts=True)
    return bool((cnt == 1).all() and np.array_equal(uk, np.unique(rev)))


def euler_characteristic(n_verts, faces):
    f = np.asarray(faces, dtype=np.int64)
    d = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return int(n_verts) - len(np.unique(d, axis=0)) + len(f)


def signed_volume(verts, faces):
    v = np.asarray(verts, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


# ---- test volumes -----------------------------------------------------------------------------------------------------------------
def noise_volume():
    """12 x 11 x 13 white noise inside one layer of -10: 255 of the 256 cases occur at level 0."""
    return np.pad(np.random.default_rng(0).standard_normal((12, 11, 13)).astype(f32), 1, constant_values=-10.0)


def _grid(shape):
    return np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij")


def ellipsoid_volume(shape=(20, 17, 23), c=(9.3, 8.1, 11.2), r=(6.0, 5.0, 7.5)):
    x, y, z = _grid(shape)
    return (1.0 - np.sqrt(((x - c[0]) / r[0])**2 + ((y - c[1]) / r[1])**2 + ((z - c[2]) / r[2])**2)).astype(f32)


def torus_volume(shape=(20, 17, 23), c=(9.3, 8.1, 11.2), R=5.0, r=1.9):
    x, y, z = _grid(shape)
    q = np.sqrt((x - c[0])**2 + (y - c[1])**2) - R
    return (r - np.sqrt(q**2 + (z - c[2])**2)).astype(f32)


def nonfinite_volume():
    """+-inf and NaN among finite values, inside one layer of -10."""
    rng = np.random.default_rng(3)
    v = rng.standard_normal((7, 6, 9)).astype(f32)
    pick = rng.integers(0, 8, v.shape)
    v[pick == 0] = np.inf
    v[pick == 1] = -np.inf
    v[pick == 2] = np.nan
    return np.pad(v, 1, constant_values=-10.0)


def single_cell(case):
    v = np.zeros((2, 2, 2), f32)
    for c in range(8):
        v[c & 1, c >> 1 & 1, c >> 2 & 1] = 1.0 + 0.125 * c if case >> c & 1 else -0.5 - 0.0625 * c
    return v


# ---- PLY ----------------------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"float": "<f4", "uchar": "u1", "int": "<i4"}


def read_ply(path):
    """Binary little-endian PLY as write_ply writes it -> (header text, {property: array [V]}, faces [F,3] int32)."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii")
    lines = header.split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = nf = 0
    props, element = [], None
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            element = w[1]
            if element == "vertex":
                nv = int(w[2])
            else:
                nf = int(w[2])
        elif w[:1] == ["property"] and element == "vertex":
            props.append((w[2], _PLY_TYPES[w[1]]))
        elif w[:1] == ["property"]:
            assert w == ["property", "list", "uchar", "int", "vertex_indices"]
    vt = np.dtype(props)
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    v = np.frombuffer(raw, vt, nv, end)
    f = np.frombuffer(raw, ft, nf, end + nv * vt.itemsize)
    assert end + nv * vt.itemsize + nf * ft.itemsize == len(raw) and (f["n"] == 3).all()
    return header, {k: v[k].copy() for k, _ in props}, f["v"].astype(np.int32)


# ---- the reference's convert_sdf_samples_to_ply arithmetic (utils.py:531-550) -----------------------------------------------------
def convert_points(volume, bbox, level, offset=None, scale=None, mc=marching_cubes):
    """(mesh_points [V,3] float32, faces) of utils.py:531-550 with `mc` in skimage's place: voxel_size = (bbox[1] - bbox[0]) /
    shape (not shape - 1), points = bbox[0] + verts, then / scale, then - offset, all float32. Faces keep the orientation whose
    right-hand normals point to lower values."""
    bbox = np.asarray(bbox, dtype=f32)
    voxel = ((bbox[1] - bbox[0]).astype(f32) / np.array(volume.shape, dtype=f32)).astype(f32)
    verts, faces, _ = mc(volume, level, spacing=tuple(float(s) for s in voxel), normals=False)
    pts = np.zeros_like(verts)
    for c in range(3):
        pts[:, c] = bbox[0, c] + verts[:, c]
    if scale is not None:
        pts = (pts / np.asarray(scale, dtype=f32)).astype(f32)
    if offset is not None:
        pts = (pts - np.asarray(offset, dtype=f32)).astype(f32)
    return pts, faces
