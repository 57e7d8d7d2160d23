"""How large is the texel box of a feature-stage tile? CPU only (oracle_c).

The feature stage (k_app_features_p) takes the appearance list 32 entries at a time. The tile marcher writes the list region by region:
one region per 8 x 8-pixel tile, inside it ray by ray (row-major in the tile), inside a ray step by step. This script renders 8-row
bands of the C2 frame (300^3 field, 800 x 800 view) with the C oracle, rebuilds that order, cuts every region into groups of 32
entries and prints, per plane / line, the bounding box of a group's taps (low-tap cells plus the high tap: max - min + 2 per axis),
the bytes of the boxes over the bytes the gather moves (32 entries x 18 taps), and the share of (group, pair) units that fit the
staged path's LDS box (plane box + line span <= SLOTS slots). Groups that straddle two regions are not modelled: they are the
tail of one region plus the head of the next (about 1 group in 13) and mostly do not fit.

    python tools/experiments/tap_box_stats.py [--rows 0,80,160,...] [--slots 64]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from oracle import oracle_torch as O
from oracle.oracle_c import COracle
from text2nerf_amd import synth

MAT = ((0, 1), (0, 2), (1, 2))   # plane k: (column axis, row axis); line k: axis 2 - k
NAMES = ("xy", "xz", "yz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default=",".join(str(r) for r in range(0, 800, 80)), help="first rows of the 8-row bands")
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--grid", type=int, default=300)
    args = ap.parse_args()
    G, W = args.grid, 800
    aabb = [[-8.0] * 3, [8.0] * 3]
    params = synth.make_field_params(0, [G] * 3, scene="S1-soft", aabb=aabb)
    cfg = O.FieldConfig(aabb=aabb, grid_size=[G] * 3)
    co = COracle(cfg, params)
    rays_all = synth.frame_rays_np(800, 800).reshape(800, 800, 6)
    lo, hi = np.asarray(aabb[0], np.float32), np.asarray(aabb[1], np.float32)
    plane = [[] for _ in range(3)]
    line = [[] for _ in range(3)]
    entries = groups = 0
    for r0 in (int(r) for r in args.rows.split(",")):
        rays = rays_all[r0:r0 + 8].reshape(-1, 6)
        _, _, z, w = co.render(rays, n_samples=cfg.n_samples)
        m = w > cfg.ray_march_weight_thres
        pts = rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]
        cell = np.clip(np.floor((pts - lo) / (hi - lo) * (G - 1)), 0, G - 1).astype(np.int32)      # low tap per axis
        m = m.reshape(8, W, -1)
        cell = cell.reshape(8, W, -1, 3)
        for tx in range(0, W, 8):                                       # one region per 8 x 8-pixel tile
            c = cell[:, tx:tx + 8][m[:, tx:tx + 8]]                     # boolean indexing: (row, column, step) order = ray-major, then step
            entries += c.shape[0]
            for g0 in range(0, c.shape[0], 32):
                g = c[g0:g0 + 32]
                ext = g.max(0) - g.min(0) + 2
                groups += 1
                for k in range(3):
                    plane[k].append(int(ext[MAT[k][0]] * ext[MAT[k][1]]))
                    line[k].append(int(ext[2 - k]))
    print(f"appearance entries {entries}, groups {groups} ({entries / max(groups, 1):.1f} entries per group)")
    fmt = lambda v: f"mean {np.mean(v):5.1f}  p90 {np.percentile(v, 90):4.0f}  p99 {np.percentile(v, 99):4.0f}  max {np.max(v):4d}"   # noqa: E731
    for k in range(3):
        print(f"plane {NAMES[k]}: box texels  {fmt(plane[k])}")
    for k in range(3):
        print(f"line {'zyx'[k]} (pair {NAMES[k]}): taps  {fmt(line[k])}")
    box = sum(np.sum(plane[k]) + np.sum(line[k]) for k in range(3))
    print(f"box bytes / gathered bytes: {box / (entries * 18):.3f}")
    fit = [np.mean((np.asarray(plane[k]) + np.asarray(line[k])) <= args.slots) for k in range(3)]
    loads = [np.mean(np.ceil((np.asarray(plane[k]) + np.asarray(line[k])) * 4 / 64)) for k in range(3)]
    print(f"units that fit {args.slots} slots: " + "  ".join(f"{NAMES[k]} {fit[k]:.4f}" for k in range(3)) + f"  all {np.mean(fit):.4f}")
    print("wave-wide 16-B loads per 16-channel chunk: " + "  ".join(f"{NAMES[k]} {loads[k]:.2f}" for k in range(3)) +
          f"  -> {3 * sum(loads):.1f} per tile (gather: 108)")


if __name__ == "__main__":
    main()
