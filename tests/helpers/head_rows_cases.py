"""Cases of the row-wise forward check of the appearance head (reference, bound, checker: tests/helpers/head_rows_ref.py): the pool of
feature rows, the weight sets, the list layouts at the kernel's own steps and the range rows. CPU only; every reference is computed once
per process and shared (functools.lru_cache), and nothing here is modified by a test."""
from functools import lru_cache

import numpy as np
import torch

from oracle import oracle_torch as O
from tests.conftest import TINY
from tests.helpers import head_rows_ref as HR
from tests.helpers.head_grad_elementwise import B0, W1, W2

POOL = 4096               # rows of the main pool (all in range under every in-range weight set)
REAL = 3712               # of which real appearance features of the tiny fixture; then 192 rows x 2^-20, 192 subnormal / +-0 rows
SEED = 20261


@lru_cache(maxsize=None)
def tiny_params():
    from text2nerf_amd import synth
    return synth.make_field_params(11, TINY["grid"], density_scale=0.9, aabb=TINY["aabb"])


@lru_cache(maxsize=None)
def real_features(n=REAL, seed=SEED):
    """The tiny fixture's appearance features (float32 oracle) at seeded points of the normalised cube."""
    g = np.random.Generator(np.random.PCG64(seed))
    xyz = torch.from_numpy(g.uniform(-1, 1, (n, 3)).astype(np.float32))
    return O.app_feature(O.params_from_numpy(tiny_params()), xyz).numpy().astype(np.float32)


def _rows(f27, seed):
    """[n, 32] kernel rows of features f27: column 27 a seeded weight in [0, 1] (every 16th row exactly 0, the next one exactly 1),
    columns 28..31 junk the kernel must not read (1e30 and NaN)."""
    g = np.random.Generator(np.random.PCG64(seed))
    n = f27.shape[0]
    out = np.empty((n, 32), np.float32)
    out[:, :27] = f27
    w = g.uniform(0, 1, n).astype(np.float32)
    w[::16] = 0.0
    w[1::16] = 1.0
    out[:, 27] = w
    out[:, 28:] = np.array([1e30, np.nan, -1e30, np.nan], np.float32)
    return out


@lru_cache(maxsize=None)
def pool_rows():
    f = real_features()
    small = (f[:192] * np.float32(2.0 ** -20)).astype(np.float32)
    sub = (f[192:384] * np.float32(2.0 ** -100)).astype(np.float32) * np.float32(2.0 ** -30)       # float32 subnormals
    sub[::3, ::2] = 0.0
    sub[1::3, 1::2] = -0.0
    out = _rows(np.concatenate([f, small, sub]), SEED + 1)
    assert out.shape == (POOL, 32)
    return out


# ---- weight sets ------------------------------------------------------------------------------------------------------------------------
def _copy(p):
    return {k: np.array(v, np.float32) for k, v in p.items()}


@lru_cache(maxsize=None)
def weights(name):
    """(params, intended variant or None, must the pool launch end flagged)."""
    p = _copy(tiny_params())
    if name == "tiny":
        return p, 1, False
    if name == "l1_tracked":
        # layer 1 scaled by the smallest power of two that puts k_ss_scales' b1 at or beyond kRange (twice the deciding 0.5 kRange);
        # layer 2 scaled back so that the colours stay off the sigmoid's rails. The true |h1| grows by the same factor and stays small
        # against the row-norm bound (asserted in tests/test_head_rows_cpu.py).
        r = HR.scales_rule(p)
        s = 2.0 ** int(np.ceil(np.log2(HR.KRANGE / r["b1"])))
        p[W1] = (p[W1] * np.float32(s)).astype(np.float32)
        p[W2] = (p[W2] * np.float32(1.0 / s)).astype(np.float32)
        return p, 0, False
    if name == "outliers":
        p[W1][3, 5] = 300.0
        p[W1][17, 9] = -411.0
        return p, None, False
    if name == "bias400":
        p[B0] = p[B0] + np.float32(400.0)
        return p, None, False
    if name == "bias1e5":
        p[B0] = p[B0] + np.float32(1.0e5)
        p[W1] = p[W1] * np.float32(1e-3)
        return p, None, True
    raise KeyError(name)


WEIGHT_SETS = ("tiny", "l1_tracked", "outliers", "bias400", "bias1e5")


@lru_cache(maxsize=None)
def pool_reference(wname):
    return HR.reference(weights(wname)[0], pool_rows())


# ---- list layouts at the kernel's steps -------------------------------------------------------------------------------------------------
def _one(n):
    return (n, 0, 0, 0, 0, 0, 0, 0)


def _cap(n):
    return 128 if n <= 128 else (n + 31) // 32 * 32


MIXED = (33, 0, 1, 32, 0, 97, 31, 0)
TILES20 = (100, 64, 0, 70, 33, 128, 33, 90)       # 4 + 2 + 0 + 3 + 2 + 4 + 2 + 3 = 20 tiles
COUNT_CASES = {"zero": (_one(0), 128), "first1": (_one(1), 128), "last1": ((0, 0, 0, 0, 0, 0, 0, 1), 128)}
for _n in (31, 32, 33, 95, 96, 97, 383, 384, 385):
    COUNT_CASES[f"n{_n}"] = (_one(_n), _cap(_n))
COUNT_CASES["mixed"] = (MIXED, 128)
COUNT_CASES["clamp1000"] = ((1000, 5, 0, 0, 0, 0, 0, 40), 96)      # list 0's counter beyond its 96 slots: list 1's slots 5.. stay untouched
COUNT_CASES["cap100"] = ((100, 0, 37, 100, 0, 0, 0, 100), 100)     # a capacity that is no multiple of 32 (list_capacity_budget returns such)
TILE_HI = (4, 7, 12, 13)
PERSIST = ((12352,) * 8, 12352)                   # 3088 tiles: 258 rounds on 256 workgroups, the last one 4 tiles


@lru_cache(maxsize=None)
def layout(name, tile_hi=0xffffffff):
    counts, cap = PERSIST if name == "persist" else ((TILES20, 128) if name == "tiles20" else COUNT_CASES[name])
    return HR.Layout(counts, cap, tile_hi).place(POOL, SEED + 7 + sum(counts) + cap)


# ---- range rows (each case a launch of its own: the range flag is per launch) ---------------------------------------------------------------
RANGE_COUNTS = ((97, 0, 103, 0, 0, 0, 0, 0), 128)
SCALES = {"x2^-20": 2.0 ** -20, "x1": 1.0, "x16": 16.0, "x64": 64.0, "x1000": 1000.0, "x3e4": 3e4}
EDGE_COLUMNS = (0, 12, 13, 14, 26)
RANGE_CASES = tuple(SCALES) + ("subnormal", "one_large", "at_kRange", "above_kRange", "above_f16")
MUST_FLAG = ("above_f16",)                        # built to leave the f16 range: the flag only


@lru_cache(maxsize=None)
def range_rows(name):
    f = real_features()[1000:1200].copy()
    if name in SCALES:
        f = (f * np.float32(SCALES[name])).astype(np.float32)
    elif name == "subnormal":
        f = pool_rows()[REAL + 192:REAL + 392 - 8, :27].copy()
        f = np.concatenate([f, np.zeros((8, 27), np.float32)])
        f[-4:] = -0.0
    else:
        v = {"one_large": 1000.0, "at_kRange": HR.KRANGE, "above_kRange": 62000.0, "above_f16": 70000.0}[name]
        for i in range(f.shape[0]):
            f[i, EDGE_COLUMNS[i % 5]] = np.float32(v if (i // 5) % 2 == 0 else -v)
    return _rows(f, SEED + 3)


@lru_cache(maxsize=None)
def range_reference(wname, name):
    return HR.reference(weights(wname)[0], range_rows(name))


@lru_cache(maxsize=None)
def range_layout():
    return HR.Layout(*RANGE_COUNTS).place(200, SEED + 11)


# ---- explicit points for the other two head forms -----------------------------------------------------------------------------------------
POINT_COUNTS = (1, 31, 32, 33, 127, 128, 129)
WRAP_POOL, WRAP_N = 2048, 65536 + 129


@lru_cache(maxsize=None)
def points(n=WRAP_POOL):
    g = np.random.Generator(np.random.PCG64(SEED + 13))
    return g.uniform(-1, 1, (n, 3)).astype(np.float32)


def cpu_table():
    """rho32, K and the bound's median / maximum per weight set and case (profiles/head_rows_elementwise.txt, CPU part)."""
    lines = []
    for w in WEIGHT_SETS:
        v, margin = HR.variant_margin(weights(w)[0])
        cases = [("pool", pool_reference(w))] + ([(n, range_reference(w, n)) for n in RANGE_CASES] if w in ("tiny", "l1_tracked") else [])
        for n, r in cases:
            lines.append(f"{w:10s} {n:12s} rows {r.c64.shape[0]:5d} variant {v} margin {margin:7.3f} | split rho32 {r.rho32:.3f} K {r.K():.2f} bound median "
                         f"{np.median(r.bound):.3e} max {r.bound.max():.3e} | exact rho32 {r.rho32_exact:.3f} K {r.K(exact=True):.2f} bound median "
                         f"{np.median(r.bound_exact):.3e} max {r.bound_exact.max():.3e} | max |f| {r.amax[:, 0].max():.3g} |h0| {r.amax[:, 1].max():.3g} "
                         f"|h1| {r.amax[:, 2].max():.3g}")
    return lines


if __name__ == "__main__":
    print("\n".join(cpu_table()))
