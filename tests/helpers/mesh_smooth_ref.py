"""Float64 numpy reference of the smoothing stage (text2nerf_amd.mesh: mesh_adjacency, smooth_mesh, vertex_normals), the meshes the CPU
and GPU files share, and the checkers the GPU file applies to the device's arrays (tests/test_mesh_smooth_cpu.py shows that each of
them catches every deliberate error of `MUTATIONS`).

Row sums run in the row's own order: `row_sum` adds the k-th entry of every row in step k, so each row is accumulated first entry
first from 0.0, one rounding per addition (the CPU file compares it with a plain Python loop). Everything else is elementwise float64
in the order smooth_mesh and vertex_normals document: sum / degree, - x, * s, + x; cross products as (u1 w2 - u2 w1, u2 w0 - u0 w2,
u0 w1 - u1 w0) of u = x_b - x_a, w = x_c - x_a; prescale by the largest |component|, divide by the norm, round to float32 once."""
import functools

import numpy as np

from tests.helpers import mc_ref as R

MUTATIONS = ("unsorted_row", "duplicate_neighbour", "mu_sign", "degree_plus_one", "float32_accumulator")


# ---- rows -----------------------------------------------------------------------------------------------------------------------------
def _csr(rows, values, n_rows):
    """Sorted unique (row, value) pairs as (offsets [n_rows + 1] int64, values [E] int32)."""
    keys = np.unique(rows.astype(np.int64) << 32 | values.astype(np.int64))
    offsets = np.searchsorted(keys, np.arange(n_rows + 1, dtype=np.int64) << 32).astype(np.int64)
    return offsets, (keys & 0xffffffff).astype(np.int32)


def adjacency(faces, n_verts, mutate=None):
    """N(v) = the u != v sharing a face edge with v: offsets [V+1] int64, neighbours [E] int32, rows ascending and unique."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a = np.concatenate([f[:, 0], f[:, 1], f[:, 1], f[:, 2], f[:, 2], f[:, 0]])
    b = np.concatenate([f[:, 1], f[:, 0], f[:, 2], f[:, 1], f[:, 0], f[:, 2]])
    keep = a != b
    off, nbr = _csr(a[keep], b[keep], int(n_verts))
    if mutate == "unsorted_row":
        v = int(np.argmax(np.diff(off) >= 2))
        nbr[off[v]], nbr[off[v] + 1] = nbr[off[v] + 1], nbr[off[v]]
    if mutate == "duplicate_neighbour":
        v = int(np.argmax(np.diff(off) >= 1))
        nbr = np.insert(nbr, off[v], nbr[off[v]])
        off = off.copy()
        off[v + 1:] += 1
    return off, nbr


def vertex_faces(faces, n_verts):
    """The faces that contain v, each once, ascending: offsets [V+1] int64, face indices [E] int32."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    t = np.repeat(np.arange(len(f), dtype=np.int64), 3)
    return _csr(f.reshape(-1), t, int(n_verts))


def row_sum(offsets, values, x, dtype=np.float64):
    """[V, x.shape[1]] sums of x[values] over every row, accumulated from 0.0 in the row's order."""
    deg = np.diff(offsets)
    out = np.zeros((len(deg), x.shape[1]), dtype)
    x = x.astype(dtype)
    for k in range(int(deg.max()) if len(deg) else 0):
        rows = np.nonzero(deg > k)[0]
        out[rows] = out[rows] + x[values[offsets[rows] + k]]
    return out


def row_sum_loop(offsets, values, x):
    """row_sum as a plain Python loop over every row entry."""
    out = np.zeros((len(offsets) - 1, x.shape[1]), np.float64)
    for v in range(len(offsets) - 1):
        for c in range(x.shape[1]):
            s = 0.0
            for q in range(int(offsets[v]), int(offsets[v + 1])):
                s = s + float(x[values[q], c])
            out[v, c] = s
    return out


# ---- smoothing and normals ----------------------------------------------------------------------------------------------------------------
def smooth_pass(x, offsets, nbr, s, fixed=None, mutate=None):
    deg = np.diff(offsets)
    acc = np.float32 if mutate == "float32_accumulator" else np.float64
    tot = row_sum(offsets, nbr, x, acc).astype(np.float64)
    move = deg > 0
    if fixed is not None:
        move &= ~np.asarray(fixed, bool)
    d = (deg + (1 if mutate == "degree_plus_one" else 0)).astype(np.float64)[:, None]
    y = x.copy()
    with np.errstate(all="ignore"):
        new = x + s * (tot / np.where(d == 0, 1.0, d) - x)
    y[move] = new[move]
    return y


def smooth(verts, faces, iterations=10, lamb=0.5, mu=-0.53, fixed=None, adj=None, mutate=None):
    """smooth_mesh's positions [V,3] float32."""
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    if iterations == 0 or len(v32) == 0:
        return v32.copy()
    off, nbr = adj if adj is not None else adjacency(faces, len(v32))
    x = v32.astype(np.float64)
    for _ in range(iterations):
        x = smooth_pass(x, off, nbr, float(lamb), fixed, mutate)
        if mu != 0:
            x = smooth_pass(x, off, nbr, abs(float(mu)) if mutate == "mu_sign" else float(mu), fixed, mutate)
    return x.astype(np.float32)


def face_cross(verts, faces):
    """(x_b - x_a) x (x_c - x_a) per face, float64 from the float32 positions."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    u, w = b - a, c - a
    return np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], -1)


def vertex_normals(verts, faces):
    """vertex_normals' [V,3] float32."""
    V = len(np.asarray(verts).reshape(-1, 3))
    off, rows = vertex_faces(faces, V)
    n = row_sum(off, rows, face_cross(verts, faces).reshape(-1, 3))
    m = np.abs(n).max(-1) if V else np.zeros(0)
    with np.errstate(all="ignore"):
        ok = (m > 0) & np.isfinite(m) & ~np.isnan(n).any(-1)
        h = n / np.where(ok, m, 1.0)[:, None]
        ln = np.sqrt(h[:, 0] * h[:, 0] + h[:, 1] * h[:, 1] + h[:, 2] * h[:, 2])
        out = h / np.where(ok, ln, 1.0)[:, None]
    out[~ok] = 0.0
    return out.astype(np.float32)


# ---- checkers (what the GPU file applies to the device's arrays) ------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_adjacency(offsets, neighbours, faces, n_verts):
    """Problems of an adjacency against the definition (an empty list: none). The structure is tested on its own, then the bits."""
    off, nbr = np.asarray(offsets), np.asarray(neighbours)
    bad = []
    if off.dtype != np.int64 or nbr.dtype != np.int32 or off.shape != (n_verts + 1,) or nbr.ndim != 1:
        return ["types"]
    if off[0] != 0 or off[-1] != len(nbr) or (np.diff(off) < 0).any():
        return ["offsets"]
    inner = np.ones(len(nbr), bool)
    inner[off[:-1][off[:-1] < len(nbr)]] = False            # the first entry of every row has no predecessor in its row
    step = np.diff(nbr.astype(np.int64), prepend=-1)
    if (inner & (step < 0)).any():
        bad.append("unsorted")
    if (inner & (step == 0)).any():
        bad.append("duplicate")
    w_off, w_nbr = adjacency(faces, n_verts)
    if not (same_bits(off, w_off) and same_bits(nbr, w_nbr)):
        bad.append("bits")
    return bad


def check_positions(got, verts, faces, **kw):
    """Problems of smoothed positions: anything but the reference's bits."""
    return [] if same_bits(np.asarray(got), smooth(verts, faces, **kw)) else ["bits"]


def check_normals(got, verts, faces):
    return [] if same_bits(np.asarray(got), vertex_normals(verts, faces)) else ["bits"]


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------
SPHERE = dict(shape=(28, 26, 30), c=(13.3, 12.6, 14.4), r=8.0, sharp=12.0, level=0.005)


def sphere_alpha_volume():
    """A near-binary alpha volume of a sphere: 1 - exp(-softplus(sharp (r - d))), about 1 inside and about 0 outside within a cell."""
    x, y, z = R._grid(SPHERE["shape"])
    c = SPHERE["c"]
    d = np.sqrt((x - c[0])**2 + (y - c[1])**2 + (z - c[2])**2)
    return (1.0 - np.exp(-np.logaddexp(0.0, SPHERE["sharp"] * (SPHERE["r"] - d)))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def mc_mesh(name):
    """(verts, faces, marching-cubes normals) of a named volume of mc_ref or of the sphere; cached, do not write into the arrays."""
    vol, level = {"ellipsoid": (R.ellipsoid_volume, 0.0), "torus": (R.torus_volume, 0.0), "noise": (R.noise_volume, 0.0),
                  "sphere": (sphere_alpha_volume, SPHERE["level"])}[name]
    out = R.marching_cubes(vol(), level)
    for a in out:
        a.setflags(write=False)
    return out


def fan(valence):
    """A triangle fan: vertex 0 in the middle of `valence` rim vertices on a wavy circle; the centre has that valence."""
    t = np.arange(valence) * (2 * np.pi / valence)
    rim = np.stack([np.cos(t), np.sin(t), 0.1 * np.sin(3 * t)], -1) * (1.0 + 0.05 * np.cos(5 * t))[:, None]
    verts = np.concatenate([[[0.013, -0.021, 0.3]], rim]).astype(np.float32)
    k = np.arange(valence)
    faces = np.stack([np.zeros(valence, np.int64), 1 + k, 1 + (k + 1) % valence], -1).astype(np.int32)
    return verts, faces


def strip(n_verts, seed=0):
    """A triangle strip over n_verts jittered vertices (n_verts - 2 faces of alternating corner order)."""
    rng = np.random.default_rng(seed + n_verts)
    k = np.arange(n_verts)
    verts = (np.stack([k // 2, k % 2, np.zeros(n_verts)], -1) + rng.uniform(-0.2, 0.2, (n_verts, 3))).astype(np.float32)
    t = np.arange(n_verts - 2)
    faces = np.where((t % 2 == 0)[:, None], np.stack([t, t + 1, t + 2], -1), np.stack([t + 1, t, t + 2], -1)).astype(np.int32)
    return verts, faces


def small_meshes():
    """name -> (verts [V,3] float32, faces [F,3] int32): the hand-made cases."""
    out = {}
    out["tetrahedron"] = (np.array([[0, 0, 0], [1, 0.1, 0], [0.2, 1, 0], [0.3, 0.2, 1]], np.float32),
                          np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32))
    octa_v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1.1, 0], [0, -0.9, 0], [0, 0, 1.2], [0, 0, -0.8], [5, 5, 5]], np.float32)
    octa_f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    out["octahedron+loose"] = (octa_v, octa_f)            # vertex 6 is referenced by no face
    # face 0 twice, a degenerate (a, a, b) face, and vertex 6 only in the degenerate face
    out["duplicate+degenerate"] = (octa_v, np.concatenate([octa_f, octa_f[:1], [[6, 6, 0]], octa_f[3:4]]).astype(np.int32))
    for k in (63, 64, 65, 300):
        out[f"fan{k}"] = fan(k)
    for n in (255, 256, 257):
        out[f"strip{n}"] = strip(n)
    return out


def mean_normal_deviation_deg(verts, faces, centre):
    """Mean angle in degrees between the right-hand face normals and the radial direction from `centre` at the face centroids."""
    v = np.asarray(verts, np.float64)
    n = face_cross(np.asarray(verts, np.float32), faces)
    ctr = v[np.asarray(faces, np.int64)].mean(1) - np.asarray(centre, np.float64)
    ok = np.linalg.norm(n, axis=1) > 0
    cosang = (n[ok] * ctr[ok]).sum(-1) / (np.linalg.norm(n[ok], axis=1) * np.linalg.norm(ctr[ok], axis=1))
    return float(np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0))).mean())
