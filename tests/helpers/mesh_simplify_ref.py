"""Float64 numpy reference of the simplification stage (text2nerf_amd.mesh: mesh_clusters, simplify_mesh), and the checkers the GPU
file applies to the device's arrays (tests/test_mesh_simplify_cpu.py shows that they catch every deliberate error of `MUTATIONS`).

Everything is elementwise float64, one rounding per operation, in the order include/t2n.h fixes:
    cell       c_k = floor(((double)x_k - o_k) / h_k); id = (c0 n1 + c1) n2 + c2; clusters = the occupied cells in ascending id
    mean       the members' float64 sum from 0.0 in ascending vertex index, / (double)count
    quadric    over the faces with a corner in the cluster, ascending face index, each once; (a, b, c) = the face's corners rotated
               so that its smallest vertex index comes first; u = x_b - x_a, w = x_c - x_a; n = (u1 w2 - u2 w1, u2 w0 - u0 w2,
               u0 w1 - u1 w0), skipped when all zero or not finite; d = x_a - mean; r = (n0 d0 + n1 d1) + n2 d2;
               A00 += n0 n0, A01 += n0 n1, A02 += n0 n2, A11 += n1 n1, A12 += n1 n2, A22 += n2 n2; b_k += n_k r
    solve      t = (A00 + A11) + A22; e = regularisation t; M_kk = A_kk + e;
               C00 = M11 M22 - A12 A12, C01 = A02 A12 - A01 M22, C02 = A01 A12 - A02 M11,
               C11 = M00 M22 - A02 A02, C12 = A01 A02 - M00 A12, C22 = M00 M11 - A01 A01;
               det = (M00 C00 + A01 C01) + A02 C02; x_0 = ((C00 b0 + C01 b1) + C02 b2) / det, x_1 with (C01, C11, C12), x_2 with
               (C02, C12, C22); p = mean + x
    box        lo_k = o_k + (double)c_k h_k, hi_k = o_k + (double)(c_k + 1) h_k; p stays iff lo_k <= p_k <= hi_k on every axis (a p
               that is not finite fails), else the mean
Row sums run in the row's own order through mesh_smooth_ref.row_sum (the k-th entry of every row in step k)."""
from typing import NamedTuple, Optional

import numpy as np

from tests.helpers import mesh_smooth_ref as S

MUTATIONS = ("float32_accumulator", "unsorted_faces", "normalised_n", "no_regularisation", "no_cell_fallback", "duplicate_keeps_higher",
             "degenerate_kept", "colour_no_rounding")


class Clusters(NamedTuple):
    vertex_map: np.ndarray      # [V] int32
    n_clusters: int
    offsets: np.ndarray         # [K+1] int64
    members: np.ndarray         # [V] int32
    cells: np.ndarray           # [K,3] int32


class Simplified(NamedTuple):
    verts: np.ndarray           # [K,3] float32
    faces: np.ndarray           # [F',3] int32
    normals: Optional[np.ndarray]
    colors: Optional[np.ndarray]
    clusters: Clusters
    n_duplicates: int           # faces dropped because an earlier face has the same rotated triple
    n_degenerate: int           # faces dropped because two corners share a cluster
    fell_back: np.ndarray       # [K] bool: quadric placement that returned the mean


def grid(verts, cell, origin=None):
    """(o [3], h [3]) float64: the caller's, or the componentwise minimum of the float32 positions."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    h = np.broadcast_to(np.asarray(cell, np.float64), (3,)).copy()
    o = np.asarray(origin, np.float64).reshape(3).copy() if origin is not None else (
        v.min(0).astype(np.float64) if len(v) else np.zeros(3))
    return o, h


def clusters(verts, cell, origin=None):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    V = len(v)
    if V == 0:
        return Clusters(np.zeros(0, np.int32), 0, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros((0, 3), np.int32))
    o, h = grid(v, cell, origin)
    c = np.floor((v.astype(np.float64) - o) / h).astype(np.int64)
    assert (c >= 0).all(), "a vertex below the origin"
    n = c.max(0) + 1
    assert int(n[0]) * int(n[1]) * int(n[2]) < 2**31
    ids = (c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2]
    uid, vmap, cnt = np.unique(ids, return_inverse=True, return_counts=True)
    members = np.argsort(ids, kind="stable").astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    cells = np.stack([uid // (n[1] * n[2]), uid // n[2] % n[1], uid % n[2]], -1).astype(np.int32)
    return Clusters(vmap.reshape(-1).astype(np.int32), len(uid), offsets, members, cells)


def rotate_min_first(f):
    """Every row of f [F,3] rotated cyclically so that its smallest entry (the first of equal ones) comes first."""
    f = np.asarray(f).reshape(-1, 3)
    k = np.argmin(f, axis=1)
    r = np.arange(len(f))
    return np.stack([f[r, k], f[r, (k + 1) % 3], f[r, (k + 2) % 3]], -1)


def cluster_faces(faces, vertex_map, K):
    """The faces with a corner in cluster k, each once, ascending: offsets [K+1] int64, face indices [E] int32."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    t = np.repeat(np.arange(len(f), dtype=np.int64), 3)
    return S._csr(np.asarray(vertex_map, np.int64)[f.reshape(-1)], t, int(K))


def place(verts, faces, cl, cell, origin=None, placement="quadric", regularisation=1e-3, mutate=None):
    """([K,3] float64 representatives before the one rounding, [K] bool fell back to the mean)."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    K = cl.n_clusters
    acc = np.float32 if mutate == "float32_accumulator" else np.float64
    cnt = np.diff(cl.offsets).astype(np.float64)[:, None]
    mean = S.row_sum(cl.offsets, cl.members, v.astype(np.float64), acc).astype(np.float64) / cnt
    if placement == "mean" or K == 0:
        return mean, np.ones(K, bool)
    o, h = grid(v, cell, origin)
    f = rotate_min_first(np.asarray(faces, np.int64).reshape(-1, 3))
    x = v.astype(np.float64)
    xa = x[f[:, 0]]
    u, w = x[f[:, 1]] - xa, x[f[:, 2]] - xa
    with np.errstate(all="ignore"):
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], -1)
        good = np.isfinite(n).all(-1) & (n != 0).any(-1)
        if mutate == "normalised_n":
            n = n / np.sqrt((n * n).sum(-1))[:, None]
    foff, frow = cluster_faces(faces, cl.vertex_map, K)
    owner = np.repeat(np.arange(K), np.diff(foff))
    keep = good[frow]
    owner, frow = owner[keep], frow[keep]
    foff = np.searchsorted(owner, np.arange(K + 1)).astype(np.int64)
    if mutate == "unsorted_faces":
        for k in range(K):
            frow[foff[k]:foff[k + 1]] = frow[foff[k]:foff[k + 1]][::-1]
    with np.errstate(all="ignore"):
        ne = n[frow]
        d = xa[frow] - mean[owner]
        r = (ne[:, 0] * d[:, 0] + ne[:, 1] * d[:, 1]) + ne[:, 2] * d[:, 2]
        terms = np.stack([ne[:, 0] * ne[:, 0], ne[:, 0] * ne[:, 1], ne[:, 0] * ne[:, 2], ne[:, 1] * ne[:, 1], ne[:, 1] * ne[:, 2],
                          ne[:, 2] * ne[:, 2], ne[:, 0] * r, ne[:, 1] * r, ne[:, 2] * r], -1)
        q = S.row_sum(foff, np.arange(len(frow)), terms, acc).astype(np.float64)
        A00, A01, A02, A11, A12, A22, b0, b1, b2 = (q[:, i] for i in range(9))
        t = (A00 + A11) + A22
        e = (0.0 if mutate == "no_regularisation" else float(regularisation)) * t
        M00, M11, M22 = A00 + e, A11 + e, A22 + e
        C00 = M11 * M22 - A12 * A12
        C01 = A02 * A12 - A01 * M22
        C02 = A01 * A12 - A02 * M11
        C11 = M00 * M22 - A02 * A02
        C12 = A01 * A02 - M00 * A12
        C22 = M00 * M11 - A01 * A01
        det = (M00 * C00 + A01 * C01) + A02 * C02
        sol = np.stack([((C00 * b0 + C01 * b1) + C02 * b2) / det, ((C01 * b0 + C11 * b1) + C12 * b2) / det,
                        ((C02 * b0 + C12 * b1) + C22 * b2) / det], -1)
        p = mean + sol
        c = cl.cells.astype(np.int64)
        lo, hi = o + c.astype(np.float64) * h, o + (c + 1).astype(np.float64) * h
        inside = ((p >= lo) & (p <= hi)).all(-1)
        if mutate == "no_cell_fallback":
            inside = np.isfinite(p).all(-1)
        ok = (t > 0) & np.isfinite(t) & inside
    return np.where(ok[:, None], p, mean), ~ok


def simplify(verts, faces, cell, origin=None, placement="quadric", regularisation=1e-3, normals=False, colors=None, mutate=None):
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    cl = clusters(v, cell, origin)
    K = cl.n_clusters
    p, fell = place(v, f, cl, cell, origin, placement, regularisation, mutate)
    out_v = p.astype(np.float32)
    m = cl.vertex_map.astype(np.int64)[f] if len(f) else np.zeros((0, 3), np.int64)
    degenerate = (m[:, 0] == m[:, 1]) | (m[:, 1] == m[:, 2]) | (m[:, 2] == m[:, 0])
    rot = rotate_min_first(m)
    live = np.ones(len(f), bool) if mutate == "degenerate_kept" else ~degenerate
    idx = np.nonzero(live)[0]
    keep = np.zeros(len(f), bool)
    if len(idx):
        if mutate == "duplicate_keeps_higher":
            _, first = np.unique(rot[idx][::-1], axis=0, return_index=True)
            first = len(idx) - 1 - first
        else:
            _, first = np.unique(rot[idx], axis=0, return_index=True)
        keep[idx[first]] = True
    out_f = rot[keep].astype(np.int32).reshape(-1, 3)
    out_c = None
    if colors is not None:
        cnt = np.diff(cl.offsets)
        tot = np.zeros((K, 3), np.int64)
        np.add.at(tot, cl.vertex_map, np.asarray(colors, np.uint8).astype(np.int64))
        half = 0 if mutate == "colour_no_rounding" else cnt[:, None] // 2
        out_c = ((tot + half) // cnt[:, None]).astype(np.uint8)
    out_n = S.vertex_normals(out_v, out_f) if normals else None
    return Simplified(out_v, out_f, out_n, out_c, cl, int(live.sum() - keep.sum()), int(degenerate.sum()), fell)


# ---- checkers (what the GPU file applies to the device's arrays) ------------------------------------------------------------------------
def check_clusters(got, verts, cell, origin=None):
    """Problems of a Clusters-like (vertex_map, K, offsets, members, cells) against the definition (an empty list: none)."""
    want = clusters(verts, cell, origin)
    vmap, K, off, mem, cells = (np.asarray(x) if i != 1 else int(x) for i, x in enumerate(tuple(got)))
    bad = []
    if K != want.n_clusters:
        return ["K"]
    for name, a, b in (("vertex_map", vmap, want.vertex_map), ("offsets", off, want.offsets), ("members", mem, want.members),
                       ("cells", cells, want.cells)):
        if not S.same_bits(a, b):
            bad.append(name)
    return bad


def check_face_rows(offsets, rows, faces, vertex_map, K):
    """Problems of the cluster -> face rows: every row ascending and unique, and the reference's bits."""
    off, rows = np.asarray(offsets), np.asarray(rows)
    bad = []
    inner = np.ones(len(rows), bool)
    inner[off[:-1][off[:-1] < len(rows)]] = False
    step = np.diff(rows.astype(np.int64), prepend=-1)
    if (inner & (step <= 0)).any():
        bad.append("unsorted")
    w = cluster_faces(faces, vertex_map, K)
    if not (S.same_bits(off, w[0]) and S.same_bits(rows, w[1])):
        bad.append("bits")
    return bad


def check_faces(faces, K):
    """Problems of an output face list on its own: three distinct indices below K, no rotated triple twice."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    bad = []
    if len(f) and (f.min() < 0 or f.max() >= K):
        bad.append("range")
    if ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])).any():
        bad.append("degenerate")
    if len(np.unique(rotate_min_first(f), axis=0)) != len(f):
        bad.append("duplicate")
    return bad


def check_mesh(got, verts, faces, cell, **kw):
    """Problems of (verts, faces, normals, colors) against simplify(...): the names of the arrays whose bits differ."""
    want = simplify(verts, faces, cell, **kw)
    bad = []
    for name, a, b in zip(("verts", "faces", "normals", "colors"), tuple(got), tuple(want)[:4]):
        if (a is None) != (b is None) or (a is not None and not S.same_bits(np.asarray(a), b)):
            bad.append(name)
    return bad


def collapse_case():
    """(verts, faces, cell, origin) for the face rules at cell 1 from the origin: clusters A, B, C, D hold (0, 1), (2, 3), (4, 5), (6);
    vertex 7 is referenced by no face and alone in its cell.
        faces 0, 1, 3   collapse to the triple (A, B, C): only face 0 stays
        face 2          (A, C, B), the oppositely oriented twin: stays
        face 4          two corners in A: dropped
        face 5          an input face with one vertex twice: skipped in the quadrics, dropped
        face 6          (A, B, D): stays; D is a cluster of one vertex"""
    v = np.array([[0.3, 0.4, 0.5], [0.7, 0.2, 0.6], [2.2, 0.5, 0.4], [2.6, 0.7, 0.3], [0.4, 2.3, 0.7], [0.8, 2.6, 0.2], [2.5, 2.5, 1.5],
                  [-1.5, 4.5, 0.5]], np.float32)
    f = np.array([[0, 2, 4], [1, 3, 5], [0, 4, 3], [3, 5, 1], [0, 1, 2], [2, 2, 4], [1, 2, 6]], np.int32)
    return v, f, 1.0, (-2.0, 0.0, 0.0)


def isolating_cell(verts):
    """A cubic cell below the smallest Chebyshev distance of two vertices: no cell holds two of them, so K = V."""
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    d = np.abs(v[:, None, :] - v[None, :, :]).max(-1)
    d[np.arange(len(v)), np.arange(len(v))] = np.inf
    return 0.9 * float(d.min())


def report():
    """The lines of profiles/mesh_simplify.txt: the reference's own figures on the marching-cubes meshes at cells 1, 2 and 3."""
    from tests.helpers import mc_ref as R
    lines = ["vertex clustering by the float64 reference (tests/helpers/mesh_simplify_ref.py), regularisation 1e-3; no GPU involved",
             "mesh cell | V F volume | K F' | volume: mean placement, quadric placement | duplicates removed, collapsed faces | "
             "share of clusters whose quadric placement fell back to the mean"]
    for name in ("sphere", "ellipsoid", "torus", "noise"):
        v, f, _ = S.mc_mesh(name)
        for cell in (1.0, 2.0, 3.0):
            a, b = simplify(v, f, cell, placement="mean"), simplify(v, f, cell)
            lines.append(f"{name} {cell:g} | {len(v)} {len(f)} {R.signed_volume(v, f):.1f} | {b.clusters.n_clusters} {len(b.faces)} | "
                         f"{R.signed_volume(a.verts, a.faces):.1f}, {R.signed_volume(b.verts, b.faces):.1f} | {b.n_duplicates}, "
                         f"{b.n_degenerate} | {b.fell_back.mean():.3f}")
    return lines


if __name__ == "__main__":
    print("\n".join(report()))
