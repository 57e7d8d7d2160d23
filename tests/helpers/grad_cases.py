"""The cases of the element-wise factor-gradient tests: small fields whose grid sizes, ray sets and sample counts aim at the off-by-one
geometry of the backward's binned scatters (csrc/t2n_backward.h / .hip):

| case  | grid        | rays x N  | aimed at                                                                                          |
| A     | 15,15,15    | 1536 x 64 | all interior cells in density block (0,0,0): > kDenSeg records in one block, >= 2 segments; one    |
|       |             |           | appearance tile per plane: many >= T2N_ACC_SEG_MIN-record segments; > 128 rays: all counter copies |
| B     | 16,30,31    | 1024 x 48 | size 16: block 1 = cells 14-15, tile 1 = cell 15; size 30: third block = the high face only; 31    |
| C     | 29,32,45    | 1024 x 48 | 29 = 14 (mod 15); size 32: third tile = cell 31 only; size 45: fourth block = face only, 3 tiles   |
| D     | 17,16,434   | 1024 x 64 | the longest line the binned path takes (LDS budget of the tile accumulate)                         |
| E     | 16,17,435   | 1024 x 64 | one texel longer: the atomic fallback, reached without the environment switch                      |
| evalB | as B        |           | is_train=False, black background: the <false> instantiations                                       |

Every case has an anisotropic box and, besides random picks from one camera inside and one outside the box: 12 axis-parallel rays lying
in the six faces (a normalised coordinate of exactly -1 / +1 for every sample), 3 rays along box edges and 4 axis-parallel rays through
grid-node coordinates (tap weights 0 / 1 up to rounding). tests/test_grad_elementwise_cpu.py asserts that the cases reach what the table
claims. Everything here runs on the CPU."""
import functools
import os
import re
from dataclasses import dataclass

import numpy as np
import torch

from oracle import oracle_torch as O
from text2nerf_amd import synth
from tests.helpers import grad_elementwise as GE

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N_SPECIAL = 19


@dataclass(frozen=True)
class Case:
    name: str
    grid: tuple
    aabb: tuple
    n_rays: int
    n_samples: int
    seed: int
    is_train: bool = True
    white_bg: bool = True
    near_far: tuple = (0.1, 30.0)
    density_scale: float = 0.7


# (the boxes start at z = 2.5: every in-box sample passes the eval-mode z > 2 gate; extents are such that (hi - lo) * (2 / (hi - lo)) == 2
# in float32, so a sample on a high face has the normalised coordinate +1 exactly — asserted by the CPU tests)
CASES = {c.name: c for c in (
    Case("caseA", (15, 15, 15), ((-2.0, -1.5, 2.5), (2.0, 1.5, 7.5)), 1536, 64, 11),
    Case("caseB", (16, 30, 31), ((-3.0, -2.0, 2.5), (5.0, 2.0, 8.5)), 1024, 48, 12),
    Case("caseC", (29, 32, 45), ((-2.0, -3.0, 2.5), (2.0, 3.0, 10.5)), 1024, 48, 13),
    Case("caseD", (17, 16, 434), ((-2.0, -1.5, 2.5), (2.0, 1.5, 10.5)), 1024, 64, 14),
    Case("caseE", (16, 17, 435), ((-1.5, -2.0, 2.5), (1.5, 2.0, 10.5)), 1024, 64, 15),
    Case("evalB", (16, 30, 31), ((-3.0, -2.0, 2.5), (5.0, 2.0, 8.5)), 1024, 48, 12, is_train=False, white_bg=False),
)}


def special_rays(case):
    """The 19 hand-placed rays: 12 in the faces, 3 along edges, 4 through grid nodes. All axis-parallel, starting 0.5 in front of the box."""
    lo, hi = (np.asarray(v, np.float32) for v in case.aabb)
    ext = hi - lo
    rays = []

    def ray(fixed, along):
        o = np.zeros(3, np.float32)
        d = np.zeros(3, np.float32)
        for a, v in fixed.items():
            o[a] = v
        o[along] = lo[along] - np.float32(0.5)
        d[along] = 1.0
        rays.append(np.concatenate([o, d]))

    frac = iter(np.float32([0.31, 0.67, 0.23, 0.58, 0.44, 0.81, 0.37, 0.52, 0.71, 0.29, 0.63, 0.47]))
    for a in range(3):                      # the six faces, two directions each
        b, c = [x for x in range(3) if x != a]
        for face in (lo[a], hi[a]):
            ray({a: face, c: lo[c] + next(frac) * ext[c]}, b)
            ray({a: face, b: lo[b] + next(frac) * ext[b]}, c)
    ray({0: lo[0], 1: hi[1]}, 2)            # three edges
    ray({0: hi[0], 2: lo[2]}, 1)
    ray({1: lo[1], 2: hi[2]}, 0)
    node = lambda a, i: lo[a] + ext[a] * np.float32(min(i, case.grid[a] - 1)) / np.float32(case.grid[a] - 1)     # noqa: E731
    ray({0: node(0, 14), 1: node(1, 15)}, 2)    # grid nodes at the block / tile edges
    ray({0: node(0, 15), 2: node(2, 14)}, 1)
    ray({1: node(1, 14), 2: node(2, 16)}, 0)
    ray({0: node(0, 0), 1: node(1, 29)}, 2)
    assert len(rays) == N_SPECIAL
    return np.stack(rays).astype(np.float32)


def build(case):
    """cfg, params, rays [R,6], jitter [R,1] (None in eval mode) and the two losses' constants of a case, all seeded by the case."""
    g = np.random.Generator(np.random.PCG64(7000 + case.seed))
    lo, hi = (np.asarray(v, np.float32) for v in case.aabb)
    grid, aabb = list(case.grid), [list(map(float, lo)), list(map(float, hi))]
    params = synth.make_field_params(8000 + case.seed, grid, density_scale=case.density_scale, aabb=aabb)
    cfg = O.FieldConfig(aabb=aabb, grid_size=grid, near_far=list(case.near_far))
    inside = tuple(float(v) for v in lo + (hi - lo) * np.float32([0.45, 0.55, 0.15]))
    outside = (float(lo[0] + 0.6 * (hi[0] - lo[0])), float(lo[1] + 0.4 * (hi[1] - lo[1])), float(lo[2] - 2.0))
    # the central 48 x 48 pixels of two 96 x 96 frames (+-14 degrees: most rays cross the box lengthwise)
    centre = np.add.outer(np.arange(24, 72) * 96, np.arange(24, 72)).reshape(-1)
    frames = np.concatenate([synth.frame_rays_np(96, 96, c2w=synth.look_pose(0.12, -0.06, inside))[centre],
                             synth.frame_rays_np(96, 96, c2w=synth.look_pose(-0.05, 0.04, outside))[centre]])
    pick = np.sort(g.choice(frames.shape[0], case.n_rays - N_SPECIAL, replace=False))
    rays = torch.from_numpy(np.concatenate([frames[pick], special_rays(case)]).astype(np.float32))
    R = rays.shape[0]
    torch_state = torch.get_rng_state()
    try:
        torch.manual_seed(case.seed)
        jitter = torch.rand(R, 1) if case.is_train else None
    finally:
        torch.set_rng_state(torch_state)
    return dict(case=case, cfg=cfg, params=params, grid=grid, aabb=aabb, rays=rays, jitter=jitter,
                ca=torch.from_numpy(g.uniform(-1, 1, (R, 3)).astype(np.float32)),
                rgb_t=torch.from_numpy(g.uniform(0, 1, (R, 3)).astype(np.float32)),
                dep_t=torch.from_numpy(g.uniform(1.0, 5.0, (R,)).astype(np.float32)))


def fuzz_loss(b):
    """tests/test_hip_fuzz.py's gradient loss: (rgb * ca).sum() + 0.1 * depth.sum() + (w ** 2).sum()."""
    ca = b["ca"]
    return lambda rgb, depth, z, w: (rgb * ca.to(rgb)).sum() + 0.1 * depth.sum() + (w ** 2).sum()


def driver_loss(b):
    """The driver's loss as tests/test_hip_fullsize.py states it (hip_driver_loss): what train_step's loss kernel evaluates."""
    from tests.test_hip_fullsize import hip_driver_loss
    rgb_t, dep_t = b["rgb_t"], b["dep_t"]
    return lambda rgb, depth, z, w: hip_driver_loss(rgb, depth, z, w, rgb_t.to(rgb.device), dep_t.to(rgb.device))[3]


@functools.lru_cache(maxsize=None)
def built(name):
    return build(CASES[name])


@functools.lru_cache(maxsize=None)
def reference(name, loss="fuzz"):
    """The element-wise reference of a case under one of the two losses, computed once per process and left unchanged."""
    b = built(name)
    c = b["case"]
    fn = fuzz_loss(b) if loss == "fuzz" else driver_loss(b)
    return GE.reference(b["cfg"], b["params"], b["rays"], b["jitter"], c.n_samples, is_train=c.is_train, white_bg=c.white_bg, loss=fn)


# ---- the kernels' bin geometry, restated for the claims ---------------------------------------------------------------------------------
def kernel_constants():
    """kBlk, kBinTile, kDenSeg (csrc/t2n_backward.h) and T2N_ACC_SEG_MIN, kAccThreads (csrc/t2n_backward.hip), read from the sources: a
    change there fails the claims test instead of silently un-covering."""
    src = os.path.join(ROOT, "text2nerf_amd", "csrc")
    with open(os.path.join(src, "t2n_backward.h")) as fh:
        h = fh.read()
    with open(os.path.join(src, "t2n_backward.hip")) as fh:
        hip = fh.read()

    def one(pattern, text):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return int(m[0])

    return dict(kBlk=one(r"constexpr\s+int\s+kBlk\s*=\s*(\d+)\s*;", h), kBinTile=one(r"constexpr\s+int\s+kBinTile\s*=\s*(\d+)\s*;", h),
                kDenSeg=one(r"constexpr\s+unsigned\s+kDenSeg\s*=\s*(\d+)\s*;", h),
                kBinCopies=one(r"constexpr\s+int\s+kBinCopies\s*=\s*(\d+)\s*;", h),
                T2N_ACC_SEG_MIN=one(r"#define\s+T2N_ACC_SEG_MIN\s+(\d+)", hip),
                kAccThreads=one(r"constexpr\s+int\s+kAccThreads\s*=\s*(\d+)\s*;", hip))


def axis_cell(g, size):
    """csrc/t2n_device.h axis_cell in float32: the clamped floor index, -1 ... size - 1."""
    g = np.asarray(g, np.float32)
    ix = ((g + np.float32(1)) / np.float32(2)) * np.float32(size - 1)
    return np.clip(np.floor(ix), -1, size - 1).astype(np.int64)


def tile_accum_lds(grid, k, channels=16, threads=None):
    """tile_accum_lds (csrc/t2n_backward.hip): doubles for the tile + line accumulators, floats for the staged values, per-wave tap tables."""
    threads = k["kAccThreads"] if threads is None else threads
    cells = (k["kBinTile"] + 1) ** 2 * channels + (max(grid) + 2) * channels
    return cells * 8 + cells * 4 + (threads // 64) * 64 * 3 * 16


if __name__ == "__main__":      # python -m tests.helpers.grad_cases: the CPU-measured part of profiles/grad_elementwise.txt
    import numpy as np
    for name, c in CASES.items():
        for loss in ("fuzz", "driver") if c.is_train else ("fuzz",):
            ref = reference(name, loss)
            share = np.concatenate([ref.K() * ref.bound[k][ref.A[k] > 0] / ref.A[k][ref.A[k] > 0] for k in GE.FACTOR_KEYS if "plane" in k])
            small = np.mean([float((np.abs(ref.g64[k])[ref.A[k] > 0] < 2e-4 * np.abs(ref.g64[k]).max()).mean()) for k in GE.FACTOR_KEYS if "plane" in k])
            print(f"{name:6s} {loss:6s} rho32 {ref.rho32:.3f} | " + " ".join(f"{k} {v:.3f}" for k, v in ref.rho32_kind.items())
                  + f" | samples {int(ref.valid.sum())} appearance {int(ref.app_mask.sum())} threshold window {int(ref.app_window.sum())}"
                  f" relu window {ref.relu_window} | planes: K*bound/A median {np.median(share):.1e} p99 {np.percentile(share, 99):.1e},"
                  f" touched elements below 2e-4 of max|g| {100 * small:.0f} %")
