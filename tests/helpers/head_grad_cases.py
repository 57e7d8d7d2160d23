"""The cases of the element-wise head-gradient tests (reference and checker: tests/helpers/head_grad_elementwise.py): grad_cases.caseA's
field and box (the tuned shape 16 / 48 / 27, fea_pe 6, 128 wide, grid 15^3), N_samples 64, train mode, white background.

Row-count cases `rows<T>`: R_FIX rays whose oracle appearance-row count is T exactly. Every ray SLOT has its own jitter value (the
forward draws torch.rand(R_FIX, 1) under the case seed) and 2 + N_CAND candidate rays: one that cuts a corner of the box (0 - 2 rows),
one that passes the box by, and N_CAND from caseA's two camera frames; a multiple-choice subset-sum over the candidates' oracle counts
picks one ray per slot. Candidates with a sample inside the list threshold's knife-edge window are never picked, so a kernel's count
cannot differ from the oracle's. The targets come from constants read out of the sources (`kernel_constants`):

    0, 1 | step -1/0/+1 (k_gemm_tn_b's 16-row step) | tile -1/0/+1 (the chain's 32-row tile) | l2 -1/0/+1 (k_bwd_l2's 64-row tile =
    tn_plan's minimum chunk) | round -1/0/+1 (8 waves x 32 rows of the chain's workgroup) | `chunk`: the first count at which tn_plan
    gives chunk_rows 96 for N = 351 (still 64 for N = 128 and 144) with a partial last chunk whose length is no multiple of the step.

Range cases on the fixed ray set RANGE_ROWS (about 1 000 rows): loss (rgb * ca * s_r).sum() + 0.1 depth.sum() + (w^2).sum() with a
per-ray factor s_r: uniform 2^-40, 2^-20, 2^20, 2^40 (their references are the s = 1 reference scaled, exactly), `mixed` (s_r = 2^k_r,
k_r a seeded integer in [-40, 20]), `zerorows` (every third ray s_r = 0) and `red` (only ca's red channel non-zero).
Weight-range cases, s_r = 1: `mlp_small` (renderModule.mlp x 1/1024), `basis_small` (basis_mat x 1/1024), `outliers` (the two
weights of test_hip_range.test_weight_beyond_256_and_large_activations: one weight fixes its matrix's power of two for all others).
`view_*`: the same rays through the MLP_Fea head (view_pe 2, fea_pe 2: tests/test_heads.py's "fea").

Everything here runs on the CPU, seeded, and is cached per process. python -m tests.helpers.head_grad_cases prints rho32 and K per case
(the CPU half of profiles/head_grad_elementwise.txt)."""
import functools
import os
import re

import numpy as np
import torch

from oracle import oracle_torch as O
from text2nerf_amd import synth
from tests.helpers import grad_cases as GC
from tests.helpers import grad_elementwise as GE
from tests.helpers import head_grad_elementwise as HE

N_SAMPLES = 64
R_FIX = 1024
N_CAND = 4
SEED = 41
RANGE_ROWS = "rows1000"
VIEW_HEAD = dict(shadingMode="MLP_Fea", view_pe=2, fea_pe=2, pos_pe=0)
UNIFORM = {"2^-40": -40, "2^-20": -20, "2^+20": 20, "2^+40": 40}


def kernel_constants():
    """The row geometry of the head backward, read from the sources: a change there fails the claims test instead of un-covering."""
    src = os.path.join(GC.ROOT, "text2nerf_amd", "csrc")
    text = {n: open(os.path.join(src, n)).read() for n in ("t2n_gemm_h.hip", "t2n_mlp_bwd_ss.hip", "t2n_bwd_mlp.hip")}

    def one(pattern, name):
        m = set(re.findall(pattern, text[name]))
        assert len(m) == 1, (pattern, m)
        return int(m.pop())

    return dict(step=one(r"for \(; kt \+ \d+ <= nrows; kt \+= (\d+)\) step\(kt, std::false_type", "t2n_gemm_h.hip"),
                tile=one(r"const long long ntiles = \(a\.rows_dev [^;]*\) / (\d+);", "t2n_mlp_bwd_ss.hip"),
                waves=one(r"const long long nrounds = \(ntiles \+ \d+\) / (\d+);", "t2n_mlp_bwd_ss.hip"),
                l2=one(r"const long long tiles = \(rows \+ \d+\) / (\d+);", "t2n_bwd_mlp.hip"),
                min_chunk=one(r"if \(c < (\d+)\) c = \d+;", "t2n_bwd_mlp.hip"),
                chunk_round=one(r"c = \(c \+ \d+\) / (\d+) \* \d+;", "t2n_bwd_mlp.hip"),
                blocks=one(r"#define\s+T2N_TN_BLOCKS\s+(\d+)", "t2n_bwd_mlp.hip"))


def tn_plan(rows, N, k=None):
    """csrc/t2n_bwd_mlp.hip tn_plan restated: (chunk_rows, chunks, ng)."""
    k = k or kernel_constants()
    ng = (N + 127) // 128
    c = (rows * ng + k["blocks"] - 1) // k["blocks"]
    c = (c + k["chunk_round"] - 1) // k["chunk_round"] * k["chunk_round"]
    c = max(c, k["min_chunk"])
    return c, max(1, (rows + c - 1) // c), ng


def chunk_target(k=None):
    """The first row count past the point where N = 351 leaves the minimum chunk, whose last chunk (for every N of the head: 351, 128,
    144) is partial with a length that is no multiple of the GEMM's row step."""
    k = k or kernel_constants()
    rows = k["min_chunk"] * k["blocks"] // 3 + 1
    while tn_plan(rows, 351, k)[0] <= k["min_chunk"] or any(rows % tn_plan(rows, N, k)[0] % k["step"] == 0 for N in (351, 128, 144)):
        rows += 1
    return rows


def row_targets(k=None):
    k = k or kernel_constants()
    edges = [k["step"], k["tile"], k["l2"], k["tile"] * k["waves"]]
    return [0, 1] + [e + d for e in edges for d in (-1, 0, 1)] + [chunk_target(k)]


def _corner_rays(aabb, n, g, miss=False):
    """Rays that cut the x = lo / y = lo edge of the box with a chord of about one sample step: few in-box samples, often none listed.
    `miss`: the same rays moved outward past the edge, no sample in the box."""
    lo, hi = (np.asarray(v, np.float64) for v in aabb)
    t = -g.uniform(0.5, 1.0, n) if miss else g.uniform(0.05, 0.35, n)
    z = g.uniform(lo[2] + 0.2, hi[2] - 0.2, n)
    o = np.stack([np.full(n, lo[0] - 1.0), lo[1] + t + 1.0, z], 1)
    d = np.stack([np.ones(n), -np.ones(n), g.uniform(-0.2, 0.2, n)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pool():
    """caseA's field and R_FIX slots x (2 + N_CAND) candidate rays with their oracle row counts at the slot's jitter."""
    c = GC.CASES["caseA"]
    g = np.random.Generator(np.random.PCG64(9000 + SEED))
    lo, hi = (np.asarray(v, np.float32) for v in c.aabb)
    grid, aabb = list(c.grid), [list(map(float, lo)), list(map(float, hi))]
    params = synth.make_field_params(8000 + c.seed, grid, density_scale=c.density_scale, aabb=aabb)
    cfg = O.FieldConfig(aabb=aabb, grid_size=grid, near_far=list(c.near_far))
    inside = tuple(float(v) for v in lo + (hi - lo) * np.float32([0.45, 0.55, 0.15]))
    outside = (float(lo[0] + 0.6 * (hi[0] - lo[0])), float(lo[1] + 0.4 * (hi[1] - lo[1])), float(lo[2] - 2.0))
    centre = np.add.outer(np.arange(24, 72) * 96, np.arange(24, 72)).reshape(-1)
    frames = np.concatenate([synth.frame_rays_np(96, 96, c2w=synth.look_pose(0.12, -0.06, inside))[centre],
                             synth.frame_rays_np(96, 96, c2w=synth.look_pose(-0.05, 0.04, outside))[centre]])
    pick = g.choice(frames.shape[0], R_FIX * N_CAND, replace=False)
    cand = np.concatenate([_corner_rays(aabb, R_FIX, g)[:, None], _corner_rays(aabb, R_FIX, g, miss=True)[:, None],
                           frames[pick].reshape(R_FIX, N_CAND, 6)], 1).astype(np.float32)
    state = torch.get_rng_state()
    try:
        torch.manual_seed(SEED)
        jitter = torch.rand(R_FIX, 1)
    finally:
        torch.set_rng_state(state)
    C = cand.shape[1]
    rays = torch.from_numpy(cand.reshape(-1, 6))
    jit = jitter.repeat_interleave(C, 0)
    P = O.params_from_numpy(params, dtype=torch.float64)
    thres = float(cfg.ray_march_weight_thres)
    with torch.no_grad():
        w = O.forward(cfg, P, rays, white_bg=True, is_train=True, n_samples=N_SAMPLES, jitter=jit, geom_dtype=torch.float32)[3]
    count = (w > thres).sum(1).reshape(R_FIX, C).numpy()
    window = ((w > thres - GE.KNIFE) & ~(w > thres + GE.KNIFE)).sum(1).reshape(R_FIX, C).numpy()
    ca = torch.from_numpy(g.uniform(-1, 1, (R_FIX, 3)).astype(np.float32))
    k_mixed = g.integers(-40, 21, R_FIX)
    return dict(cfg=cfg, params=params, grid=grid, aabb=aabb, near_far=list(c.near_far), cand=cand, jitter=jitter, count=count,
                usable=window == 0, ca=ca, k_mixed=k_mixed,
                rgb_t=torch.from_numpy(g.uniform(0, 1, (R_FIX, 3)).astype(np.float32)),
                dep_t=torch.from_numpy(g.uniform(1.0, 5.0, (R_FIX,)).astype(np.float32)))


def pick_rays(target):
    """One candidate per slot with the counts summing to `target` exactly: the corner ray and the passing ray are preferred, so the listed
    rows sit in as few rays as the target allows. Returns the candidate index per slot."""
    p = pool()
    count, usable = p["count"], p["usable"]
    reach = np.zeros((R_FIX + 1, target + 1), bool)
    reach[0, 0] = True
    for i in range(R_FIX):
        for c in range(count.shape[1]):
            n = int(count[i, c])
            if usable[i, c] and n <= target:
                reach[i + 1, n:] |= reach[i, :target + 1 - n]
    assert reach[R_FIX, target], f"no ray subset with {target} appearance rows"
    choice, t = np.zeros(R_FIX, np.int64), target
    for i in range(R_FIX - 1, -1, -1):
        for c in range(count.shape[1]):
            n = int(count[i, c])
            if usable[i, c] and n <= t and reach[i, t - n]:
                choice[i], t = c, t - n
                break
        else:
            raise AssertionError("subset-sum backtracking failed")
    assert t == 0
    return choice


def _params_of(name):
    p = {k: v.copy() for k, v in pool()["params"].items()}
    if name == "mlp_small":
        for k in p:
            if k.startswith("renderModule.mlp"):
                p[k] = p[k] * np.float32(1.0 / 1024)
    elif name == "basis_small":
        p[HE.BASIS] = p[HE.BASIS] * np.float32(1.0 / 1024)
    elif name == "outliers":
        p[HE.W1][3, 5] = 300.0
        p[HE.W1][17, 9] = -411.0
    return p


def _view_params():
    """The factor tensors of the pool's field with a freshly seeded MLP_Fea head."""
    p = pool()
    head = synth.make_field_params(8100 + SEED, p["grid"], aabb=p["aabb"], shading_mode=VIEW_HEAD["shadingMode"], fea_pe=VIEW_HEAD["fea_pe"],
                                   view_pe=VIEW_HEAD["view_pe"], pos_pe=VIEW_HEAD["pos_pe"])
    return {k: (head[k] if k in HE.HEAD_KEYS else v.copy()) for k, v in p["params"].items()}


def _scale_of(name):
    """Per-ray factor s_r [R_FIX] (float64, exact in float32) and the colour mask of a range case."""
    p = pool()
    s, chan = np.ones(R_FIX), np.ones(3)
    if name in UNIFORM:
        s = s * 2.0 ** UNIFORM[name]
    elif name == "mixed":
        s = 2.0 ** p["k_mixed"].astype(np.float64)
    elif name == "zerorows":
        s[::3] = 0.0
    elif name == "red":
        chan = np.array([1.0, 0.0, 0.0])
    return s, chan


ROW_CASES = tuple(f"rows{t}" for t in row_targets())
RANGE_CASES = tuple(UNIFORM) + ("mixed", "zerorows", "red")
WEIGHT_CASES = ("mlp_small", "basis_small", "outliers")
VIEW_CASES = ("view_rows33", "view_rows257", "view_2^-40", "view_2^+40", "view_mixed", "view_zerorows")
CHUNK_CASE = ROW_CASES[-1]


@functools.lru_cache(maxsize=None)
def built(name, loss="fuzz"):
    """cfg, params, rays [R_FIX,6], jitter, the loss' colour factors `cas` [R_FIX,3] float32 (= ca * s_r) and the driver loss' targets."""
    p = pool()
    view = name.startswith("view_")
    core = name[5:] if view else name
    target = int(core[4:]) if core.startswith("rows") else int(RANGE_ROWS[4:])
    choice = pick_rays(target)
    rays = torch.from_numpy(p["cand"][np.arange(R_FIX), choice].copy())
    s, chan = _scale_of(core)
    cas = torch.from_numpy((p["ca"].numpy().astype(np.float64) * s[:, None] * chan[None]).astype(np.float32))
    cfg, params = p["cfg"], _params_of(core)
    if view:
        cfg = O.FieldConfig(aabb=p["aabb"], grid_size=p["grid"], near_far=p["near_far"], shading_mode=VIEW_HEAD["shadingMode"],
                            fea_pe=VIEW_HEAD["fea_pe"], view_pe=VIEW_HEAD["view_pe"], pos_pe=VIEW_HEAD["pos_pe"])
        params = _view_params()
    return dict(name=name, target=target, cfg=cfg, params=params, grid=p["grid"], aabb=p["aabb"], near_far=p["near_far"], rays=rays,
                jitter=p["jitter"], cas=cas, s=s, rgb_t=p["rgb_t"], dep_t=p["dep_t"], seed=SEED, n_samples=N_SAMPLES, view=view)


def fuzz_loss(b):
    cas = b["cas"]
    return lambda rgb, depth, z, w: (rgb * cas.to(rgb)).sum() + 0.1 * depth.sum() + (w ** 2).sum()


def driver_loss(b):
    return GC.driver_loss(b)


def _base_of(name):
    """A uniform power-of-two case is its s = 1 case scaled: (base case name, factor) or None."""
    view = "view_" if name.startswith("view_") else ""
    core = name[len(view):]
    return (view + RANGE_ROWS, 2.0 ** UNIFORM[core]) if core in UNIFORM else None


@functools.lru_cache(maxsize=None)
def reference(name, loss="fuzz", direct=False):
    """The element-wise head reference of a case, computed once per process and left unchanged. `direct`: a uniform case computed on
    its own instead of scaled from the s = 1 reference (the CPU test compares the two)."""
    base = _base_of(name)
    if base is not None and loss == "fuzz" and not direct:
        return reference(base[0], "fuzz").scaled(base[1])
    b = built(name)
    fn = fuzz_loss(b) if loss == "fuzz" else driver_loss(b)
    return HE.reference(b["cfg"], b["params"], b["rays"], b["jitter"], b["n_samples"], fn)


def g64_all(name, loss="fuzz"):
    """The float64 gradients of all 19 tensors (a scaled reference carries the head tensors only: the case is then computed directly)."""
    ref = reference(name, loss)
    return ref.g64 if len(ref.g64) == 19 else reference(name, loss, direct=True).g64


@functools.lru_cache(maxsize=None)
def factor_reference(name):
    """grad_elementwise's reference of the twelve factor tensors for the same case (fuzz loss)."""
    b = built(name)
    return GE.reference(b["cfg"], b["params"], b["rays"], b["jitter"], b["n_samples"], is_train=True, white_bg=True, loss=fuzz_loss(b))


def table_line(name, loss="fuzz"):
    ref = reference(name, loss)
    return (f"{name:12s} {loss:6s} rows {ref.rows:5d} rho32 {ref.rho32:.3f} K {ref.K():.2f} | "
            + " ".join(f"{HE.short(k)} {v:.3f}" for k, v in ref.rho32_key.items())
            + f" | threshold window {int(ref.app_window.sum())} relu window {ref.relu_window}")


if __name__ == "__main__":
    for n in ROW_CASES + RANGE_CASES + WEIGHT_CASES + VIEW_CASES:
        print(table_line(n))
    for n in ("rows1", "rows33", "rows65", "rows257", CHUNK_CASE):
        print(table_line(n, "driver"))
