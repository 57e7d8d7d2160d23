#!/usr/bin/env python3
"""Rounding of the tile marcher's density feature under three summation orders, fp32 emulated in numpy against float64 (CPU only):
  per-ray   the per-ray marcher: per pair and channel the bilinear plane value and the linear line value, then one FMA per channel
  pairs     three pair tables D_k = P_k L_k^T, per pair four plane weights x two line rows (the tile marcher before the summed table)
  summed    S = (D_0 + D_1) + D_2 per cell corner, ONE trilinear read (t2n_march_tiles.hip: table_sum / table_read3)
An FMA is emulated as the fp32 rounding of the float64 product-sum; the MFMA's four-term accumulation as sequential FMAs.
    python tools/experiments/march_sum_rounding.py [points] > profiles/march_summed_table_rounding.txt"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from text2nerf_amd import synth  # noqa: E402

F = np.float32
MAT, VEC = ((0, 1), (0, 2), (1, 2)), (2, 1, 0)


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
    g = [300] * 3
    sd = synth.make_field_params(0, g, scene="S1-soft", aabb=[[-8.0] * 3, [8.0] * 3])
    P = [np.ascontiguousarray(sd[f"density_plane.{k}"][0].transpose(1, 2, 0)) for k in range(3)]   # [H][W][16]
    L = [np.ascontiguousarray(sd[f"density_line.{k}"][0, :, :, 0].T) for k in range(3)]            # [L][16]
    rng = np.random.Generator(np.random.PCG64(1))
    x = rng.uniform(-1, 1, size=(n, 3)).astype(F)
    ix = (((x + F(1)) / F(2)).astype(F) * F(g[0] - 1)).astype(F)
    i0 = np.floor(ix).astype(np.int64)
    w1 = (ix - np.floor(ix)).astype(F)
    w0 = (F(1) - w1).astype(F)
    i1 = np.minimum(i0 + 1, g[0] - 1)
    idx, w = (i0, i1), (w0, w1)

    # float64 reference
    ref = np.zeros(n)
    for k in range(3):
        m0, m1, v = MAT[k][0], MAT[k][1], VEC[k]
        pl = sum(P[k][idx[b][:, m1], idx[a][:, m0]].astype(np.float64) * (w[b][:, m1].astype(np.float64) * w[a][:, m0])[:, None]
                 for a in (0, 1) for b in (0, 1))
        ln = sum(L[k][idx[c][:, v]].astype(np.float64) * w[c][:, v].astype(np.float64)[:, None] for c in (0, 1))
        ref += (pl * ln).sum(1)

    # per-ray marcher's order
    per_ray = np.zeros(n, F)
    for k in range(3):
        m0, m1, v = MAT[k][0], MAT[k][1], VEC[k]
        wy0, wy1, wx0, wx1 = w[0][:, m1], w[1][:, m1], w[0][:, m0], w[1][:, m0]
        for c in range(16):
            t = (P[k][i0[:, m1], i0[:, m0], c] * (wy0 * wx0).astype(F)).astype(F)
            t = fma(P[k][i0[:, m1], i1[:, m0], c], (wy0 * wx1).astype(F), t)
            t = fma(P[k][i1[:, m1], i0[:, m0], c], (wy1 * wx0).astype(F), t)
            t = fma(P[k][i1[:, m1], i1[:, m0], c], (wy1 * wx1).astype(F), t)
            l = fma(L[k][i1[:, v], c], w[1][:, v], (L[k][i0[:, v], c] * w[0][:, v]).astype(F))
            per_ray = fma(t, l, per_ray)

    # table entries D_k[corner of the plane][line row] (fp32, sequential FMAs over the 16 components)
    def entry(k, a, b, c):
        m0, m1, v = MAT[k][0], MAT[k][1], VEC[k]
        p, ln = P[k][idx[b][:, m1], idx[a][:, m0]], L[k][idx[c][:, v]]
        d = np.zeros(n, F)
        for ch in range(16):
            d = fma(p[:, ch], ln[:, ch], d)
        return d

    D = [{(a, b, c): entry(k, a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)} for k in range(3)]   # a: m0 tap, b: m1 tap, c: line tap

    def read(get, wx, wy, wz):   # v0 / v1 over the plane (x fastest), then the third axis
        wnw, wne, wsw, wse = (wy[0] * wx[0]).astype(F), (wy[0] * wx[1]).astype(F), (wy[1] * wx[0]).astype(F), (wy[1] * wx[1]).astype(F)
        vs = []
        for c in (0, 1):
            t = (get(0, 0, c) * wnw).astype(F)
            t = fma(get(1, 0, c), wne, t)
            t = fma(get(0, 1, c), wsw, t)
            t = fma(get(1, 1, c), wse, t)
            vs.append(t)
        return vs

    pairs = np.zeros(n, F)
    for k in range(3):
        m0, m1, v = MAT[k][0], MAT[k][1], VEC[k]
        v0, v1 = read(lambda a, b, c: D[k][(a, b, c)], (w[0][:, m0], w[1][:, m0]), (w[0][:, m1], w[1][:, m1]), None)
        pairs = fma(v0, w[0][:, v], pairs)
        pairs = fma(v1, w[1][:, v], pairs)

    # S[z][y][x] = (D_0[z][(y, x)] + D_1[y][(z, x)]) + D_2[x][(z, y)], corner (tx, ty, tz)
    def S(tx, ty, tz):
        return ((D[0][(tx, ty, tz)] + D[1][(tx, tz, ty)]).astype(F) + D[2][(ty, tz, tx)]).astype(F)

    v0, v1 = read(lambda a, b, c: S(a, b, c), (w[0][:, 0], w[1][:, 0]), (w[0][:, 1], w[1][:, 1]), None)
    summed = fma(v1, w[1][:, 2], (v0 * w[0][:, 2]).astype(F))

    print(f"S1-soft 300^3, {n} uniform points, |feature| up to {np.abs(ref).max():.1f}")
    print(f"{'order':28s} {'max abs error':>14s} {'p99.9':>10s} {'mean':>10s}")
    for name, val in (("per-ray marcher's order", per_ray), ("pair tables", pairs), ("summed table", summed)):
        e = np.abs(val.astype(np.float64) - ref)
        print(f"{name:28s} {e.max():14.1e} {np.quantile(e, 0.999):10.1e} {e.mean():10.1e}")
    print(f"max |pair tables - per-ray| {np.abs(pairs - per_ray).max():.1e}, max |summed table - per-ray| {np.abs(summed - per_ray).max():.1e}, "
          f"max |summed table - pair tables| {np.abs(summed - pairs).max():.1e}")


if __name__ == "__main__":
    main()
