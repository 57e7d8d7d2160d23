"""Cases for the general-shape render path (text2nerf_amd/csrc/t2n_generic.hip), shared by tests/test_generic_cases_cpu.py (the
coverage claim, on the CPU) and tests/test_generic_fuzz.py (the kernels against the oracle, on the GPU).

The path picks its kernel form from the descriptor's shape without telling anyone. `form_of` restates that selection in Python so
that a CPU test can assert that the directed cases and the fuzz seeds together reach every form; the oracle and `synth` generate every
input, nothing is stored."""
import functools
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from oracle import oracle_torch as O
from text2nerf_amd import synth

# ---- the selection arithmetic of t2n_generic.hip ------------------------------------------------------------------------------------
PASS_ROWS = 262144          # kGenPassRows: list entries per pass of the matrix-core head
LDS_LIMIT = 160 * 1024      # t2n_generic_forward: `lds <= 160 * 1024` selects the staged forward
ROWS_IN_MAX = 512           # gen_stage_carve: `mlp && in0 <= 512 && fc <= 512` gives the matrix-core head its x0 / h0 / h1 rows
DIM_MAX, HID_MAX, IN_MAX, PE_MAX = 64, 256, 4096, 16      # kGenDimMax, kGenHidMax, kGenInMax, gen_fill's octave limit
MLP_HEADS = ("MLP_Fea_noview", "MLP_Fea", "MLP")

ALL_TAGS = frozenset({
    "fwd_plain", "fwd_staged",                                         # k_gen_march + k_gen_shade<false> | k_gen_stage ... head
    "head_rows32", "head_rows64", "head_valu_mlp", "head_sh", "head_rgb",
    "multipass", "pass2_nonempty",                                     # R N > kGenPassRows | the list count itself is above it
    "den_scalar", "app_scalar", "app_vec",                             # component counts not / a multiple of 4
    "out_scalar", "out_vec",                                           # k_gen_out: featureC % 16
    "ndc", "mask"})
EXTRA_TAGS = frozenset({"ldh_pad", "pass1_partial_tile"})             # reported, not part of the coverage claim


def in0_of(kw):
    """gen_fill: `a.in0 = a.app_dim * (1 + 2 * fpe) + (view ? 3 + 6 * d->view_pe : 0)`, fpe = 0 for the MLP head; 0 for SH / RGB."""
    if kw["shadingMode"] not in MLP_HEADS:
        return 0
    fpe = 0 if kw["shadingMode"] == "MLP" else kw["fea_pe"]
    view = kw["shadingMode"] != "MLP_Fea_noview"
    return kw["app_dim"] * (1 + 2 * fpe) + (3 + 6 * kw["view_pe"] if view else 0)


def head_lds_bytes(kw):
    """gen_head_lds(desc) (rows_only = false, the value t2n_generic_forward tests): (ncol D + 64 D + 16 * 64 + 64 max(4 D, fC)) floats."""
    ncol, D = sum(kw["appearance_n_comp"]), kw["app_dim"]
    return (ncol * D + D * 64 + 16 * 64 + max(4 * D, kw["featureC"]) * 64) * 4


def inside_limits(kw):
    """gen_fill's rejections (and tensorf.py::_is_general's): a case outside them would raise on construction or at the first render."""
    ok = 1 <= kw["app_dim"] <= DIM_MAX and all(c >= 1 for c in kw["density_n_comp"] + kw["appearance_n_comp"])
    if kw["shadingMode"] == "SH":
        ok = ok and kw["app_dim"] == 27
    if kw["shadingMode"] == "RGB":
        ok = ok and kw["app_dim"] == 3
    if kw["shadingMode"] in MLP_HEADS:
        ok = ok and 1 <= kw["featureC"] <= HID_MAX and in0_of(kw) <= IN_MAX and 0 <= kw["fea_pe"] <= PE_MAX and 0 <= kw["view_pe"] <= PE_MAX
    return ok


def form_of(kw, R, N, count=None, ndc=False, mask=False):
    """The kernel forms a render of R rays x N samples of shape `kw` runs, as a set of tags. Mirrors t2n_generic_forward (the
    `!plain && sc.total <= workspace_bytes && lds <= 160 * 1024` test: the Python surface always passes
    t2n_generic_workspace_bytes_desc bytes, so only the LDS term decides; then `sc.x0 && fa.w0p && !valu_head`, the `app_dim <= 32`
    choice of k_gen_head_rows<32 / 64> and the pass loop `row0 < tot` in steps of rows_cap), gen_head_body's `(C & 3) == 0`,
    k_gen_out's `(fC & 15) == 0` and gen_stage_carve's ldh = fC rounded up to 4. `count`: the appearance-list length, when known (the
    oracle's), decides whether a second pass has work."""
    tags = set()
    if ndc:
        tags.add("ndc")
    if mask:
        tags.add("mask")
    if head_lds_bytes(kw) > LDS_LIMIT:
        return tags | {"fwd_plain"}          # k_gen_march + k_gen_shade<false>: no staging, no component branches, no head kernels
    tags.add("fwd_staged")
    if any(c % 4 for c in kw["density_n_comp"]):
        tags.add("den_scalar")               # (k_gen_sigma's loop is scalar for every count; the tag marks rows that are no float4 multiple)
    if any(c % 4 for c in kw["appearance_n_comp"]):
        tags.add("app_scalar")
    if any(c % 4 == 0 for c in kw["appearance_n_comp"]):
        tags.add("app_vec")
    sh = kw["shadingMode"]
    if sh == "SH":
        tags.add("head_sh")
    elif sh == "RGB":
        tags.add("head_rgb")
    elif in0_of(kw) > ROWS_IN_MAX:
        tags.add("head_valu_mlp")
    else:
        tags.add("head_rows64" if kw["app_dim"] > 32 else "head_rows32")
        tags.add("out_scalar" if kw["featureC"] % 16 else "out_vec")
        if kw["featureC"] % 4:
            tags.add("ldh_pad")
        if R * N > PASS_ROWS:
            tags.add("multipass")
            if count is not None and count > PASS_ROWS:
                tags.add("pass2_nonempty")
            if count is not None and PASS_ROWS - 64 < count < PASS_ROWS:
                tags.add("pass1_partial_tile")
    return tags


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
GRID0, AABB0, NF0 = [23, 19, 17], [[-3.0, -2.5, -2.0], [3.0, 2.5, 4.0]], [0.3, 7.0]
AABB_HI = [[-3.0, -2.5, 2.5], [3.0, 2.5, 8.5]]        # the same box lifted above the eval z gate (2.0): eval and train keep the same samples


@dataclass
class Case:
    name: str
    kw: dict                                   # TensorVMSplit's shape keywords
    rays: np.ndarray                           # [R, 6] float32
    n_train: int
    grid: list = field(default_factory=lambda: list(GRID0))
    aabb: list = field(default_factory=lambda: [list(AABB0[0]), list(AABB0[1])])
    near_far: list = field(default_factory=lambda: list(NF0))
    step_ratio: float = 1.0
    density_shift: float = -10.0
    density_scale: float = 0.8
    app_scale: float = 0.3                     # appearance features of ~0.1 (synth's default 0.1 gives ~0.01, to which the small heads' colours hardly react)
    white_train: bool = True
    grad_train: bool = True                    # the mode of the gradient comparison
    n_eval: int = -1
    ndc: bool = False
    mask: bool = False
    seed0: int = 100
    tags: Optional[frozenset] = None           # declared (directed cases)
    large: bool = False                        # forward only, no seed walk
    count_mode: Optional[bool] = None          # large cases: is_train of the pass whose list count the tags speak of

    @property
    def R(self):
        return int(self.rays.shape[0])


def frame(H, W, yaw=0.2, pitch=-0.1, centre=(0.1, 0.2, -2.5)):
    """An H x W frame of rays (odd H and W: the ray count is then no multiple of 4 or 64)."""
    return np.ascontiguousarray(synth.frame_rays_np(H, W, c2w=synth.look_pose(yaw, pitch, centre)), np.float32)


def centre_rays(R, centre):
    """R rays from one point, directions over a 160-degree cone around +z (every ray starts inside the box)."""
    g = np.random.Generator(np.random.PCG64(77))
    d = g.normal(size=(R, 3))
    d[:, 2] = np.abs(d[:, 2]) + 0.15
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([np.broadcast_to(np.asarray(centre, np.float64), d.shape), d], 1).astype(np.float32)


def ndc_frame(H, W):
    d = torch.from_numpy(synth.frame_rays_np(H, W)[:, 3:6].copy())
    d[:, 1:] = -d[:, 1:]
    o = torch.zeros_like(d)
    o[:, 0] = torch.linspace(-0.2, 0.2, d.shape[0])
    a, b = O.ndc_rays(H, W, float(W), 1.0, o, d, blender=True)
    return torch.cat([a, b], 1).float().numpy()


def _kw(den, app, dim, head, fea_pe, view_pe, fC):
    return dict(density_n_comp=list(den), appearance_n_comp=list(app), app_dim=dim, shadingMode=head, fea_pe=fea_pe, view_pe=view_pe,
                pos_pe=0, featureC=fC)


def _t(*names):
    return frozenset(names)


_TWO_PASS_KW = _kw([20, 17, 24], [52, 49, 56], 16, "MLP_Fea", 3, 2, 77)       # in0 = 127, odd featureC
_LARGE = dict(aabb=AABB_HI, density_shift=-4.5, density_scale=0.05, n_eval=12, large=True, count_mode=True)
R_TWO_PASS, R_BOUNDARY = 32768, 26302

DIRECTED = {c.name: c for c in [
    # odd everything on the matrix-core head: scalar component loads, scalar k_gen_out, ldh = 132 for 130 units
    Case("odd_rows", _kw([33, 17, 18], [50, 49, 51], 27, "MLP_Fea_noview", 6, 0, 130), frame(13, 17), 29,
         tags=_t("fwd_staged", "head_rows32", "den_scalar", "app_scalar", "out_scalar", "ldh_pad")),
    # 520 MLP inputs: k_gen_head's VALU layers
    Case("valu_in520", _kw([17, 5, 9], [49, 7, 66], 40, "MLP_Fea_noview", 6, 0, 200), frame(11, 13), 23,
         tags=_t("fwd_staged", "head_valu_mlp", "den_scalar", "app_scalar")),
    # every limit at once: 64 features, 256 units, 16 + 16 octaves, 2 211 inputs
    # (16 octaves multiply a feature's float32 rounding by 32 768: at features of ~0.1 the float32 oracle's own gradients sit 4e-4 from
    # the float64 ones and a ReLU input moves by more than the 5e-6 margin; synth's default scale keeps the reference well conditioned)
    Case("limits", _kw([20, 16, 12], [52, 48, 40], 64, "MLP_Fea", 16, 16, 256), frame(7, 9), 12, app_scale=0.1,
         tags=_t("fwd_staged", "head_valu_mlp", "app_vec")),
    # high octaves through the input rows of the matrix-core head (angle doubling)
    Case("octaves10", _kw([20, 20, 20], [64, 64, 64], 12, "MLP_Fea_noview", 10, 0, 96), frame(13, 17), 31,
         tags=_t("fwd_staged", "head_rows32", "app_vec", "out_vec")),
    Case("octaves16", _kw([20, 20, 20], [64, 64, 64], 12, "MLP_Fea_noview", 16, 0, 96), frame(13, 17), 31, app_scale=0.1,
         tags=_t("fwd_staged", "head_rows32", "app_vec", "out_vec")),
    # 41 728 floats of LDS for the staged head against 40 960: the plain forward
    Case("plain", _kw([20, 16, 16], [112, 104, 100], 64, "MLP_Fea_noview", 2, 0, 256), frame(9, 11), 19,
         tags=_t("fwd_plain")),
    # 7 units, 5 features on a wide field: per = 2 with a one-unit tail, ldh = 8
    Case("tiny_head", _kw([18, 20, 17], [48, 30, 9], 5, "MLP_Fea_noview", 2, 0, 7), frame(13, 17), 37,
         tags=_t("fwd_staged", "head_rows32", "den_scalar", "app_scalar", "app_vec", "out_scalar", "ldh_pad")),
    # the MLP head (view directions only, fea_pe ignored) on wide components
    Case("mlp_view", _kw([40, 24, 32], [96, 80, 64], 24, "MLP", 6, 4, 144), frame(13, 17), 27,
         tags=_t("fwd_staged", "head_rows32", "app_vec", "out_vec")),
    # more than 32 features on the matrix-core head
    Case("rows64", _kw([17, 24, 9], [51, 64, 33], 48, "MLP_Fea", 2, 3, 100), frame(13, 17), 33,
         tags=_t("fwd_staged", "head_rows64", "den_scalar", "app_scalar", "app_vec", "out_scalar")),
    Case("sh_odd", _kw([18, 7, 21], [50, 13, 27], 27, "SH", 6, 6, 128), frame(13, 17), 41,
         tags=_t("fwd_staged", "head_sh", "den_scalar", "app_scalar")),
    Case("rgb_odd", _kw([5, 19, 3], [49, 2, 7], 3, "RGB", 6, 6, 128), frame(13, 17), 41,
         tags=_t("fwd_staged", "head_rgb", "den_scalar", "app_scalar")),
    # no sample in the box: the camera looks away from it (empty list, all-zero gradients)
    Case("empty", _kw([17, 24, 9], [51, 64, 33], 48, "MLP_Fea", 2, 3, 100), frame(5, 7, yaw=3.1, centre=(0.0, 0.0, -6.0)), 16,
         tags=_t("fwd_staged", "head_rows64", "den_scalar", "app_scalar", "app_vec", "out_scalar")),
    # more than 262 144 + 64 appearance samples: two head passes with work (and a third, empty one: 393 216 samples)
    Case("two_pass", _TWO_PASS_KW, centre_rays(R_TWO_PASS, (0.0, 0.0, 5.5)), 12,
         tags=_t("fwd_staged", "head_rows32", "multipass", "pass2_nonempty", "den_scalar", "app_scalar", "app_vec", "out_scalar", "ldh_pad"),
         **_LARGE),
    # a count just below 262 144: the last tile of pass 1 is partial, pass 2 has nothing
    Case("pass_boundary", _TWO_PASS_KW, centre_rays(R_TWO_PASS, (0.0, 0.0, 5.5))[:R_BOUNDARY], 12,
         tags=_t("fwd_staged", "head_rows32", "multipass", "pass1_partial_tile", "den_scalar", "app_scalar", "app_vec", "out_scalar", "ldh_pad"),
         **_LARGE),
]}

FUZZ_SEEDS = list(range(18))


@functools.lru_cache(maxsize=None)
def fuzz_case(seed):
    """A seeded random general-shape configuration: anisotropic grid, independent component counts per plane, any head, head sizes
    over the whole admitted range (fea_pe / view_pe up to 10), box, near / far, step ratio, a camera inside the box and one outside,
    a ragged ray count, train sample count, modes; every third seed carries an AlphaGridMask, NDC rays or both."""
    g = np.random.Generator(np.random.PCG64(31000 + seed))
    grid = [int(g.integers(9, 46)) for _ in range(3)]
    lo = (-g.uniform(2.0, 9.0, 3)).astype(np.float32)
    hi = g.uniform(3.0, 9.0, 3).astype(np.float32)
    head = str(g.choice(["MLP_Fea_noview", "MLP_Fea", "MLP", "SH", "RGB"], p=[0.3, 0.3, 0.15, 0.15, 0.1]))
    den = [int(g.integers(1, 81)) for _ in range(3)]
    app = [int(g.integers(1, 81)) for _ in range(3)]
    if max(den) <= 16 and max(app) <= 48:          # at least one count beyond the tuned 16 / 48: the case is general
        app[int(g.integers(0, 3))] = int(g.integers(49, 81))
    dim = 27 if head == "SH" else 3 if head == "RGB" else int(g.integers(1, 65))
    kw = _kw(den, app, dim, head, int(g.integers(0, 11)), int(g.integers(0, 11)), int(g.integers(1, 257)))
    kind = (seed // 3) % 3 if seed % 3 == 2 else -1      # every third seed: mask, NDC rays, both, in turn
    mask, ndc = kind in (0, 2), kind in (1, 2)
    near_far = [float(g.uniform(0.05, 1.0)), float(g.uniform(4.0, 12.0))]
    if ndc:
        rays = ndc_frame(int(g.integers(6, 10)), int(g.integers(7, 12)))
        if rays.shape[0] % 2 == 0:
            rays = rays[:-1]
    else:
        centre = tuple(float(v) for v in (lo + (hi - lo) * g.uniform(0.2, 0.8, 3)))
        outside = tuple(float(v) for v in (np.array([0.0, 0.0, lo[2]]) - np.array([0.0, 0.0, g.uniform(0.5, 3.0)])))
        rays = np.concatenate([
            synth.frame_rays_np(int(g.integers(6, 10)), int(g.integers(7, 12)), c2w=synth.look_pose(float(g.uniform(-3, 3)), float(g.uniform(-1, 1)), centre)),
            synth.frame_rays_np(int(g.integers(5, 8)), int(g.integers(5, 9)), c2w=synth.look_pose(float(g.uniform(-0.4, 0.4)), float(g.uniform(-0.3, 0.3)), outside)),
            np.array([[centre[0], centre[1], centre[2], 0, 0, 1], [centre[0], centre[1], centre[2], 1, 0, 0],
                      [lo[0] - 1, lo[1] - 1, lo[2] - 1, 0.577, 0.577, 0.577]], np.float32)]).astype(np.float32)
        if rays.shape[0] % 2 == 0:                   # an odd count: no multiple of 4 or 64
            rays = rays[:-1]
    return Case(f"fuzz{seed}", kw, np.ascontiguousarray(rays), int(g.integers(5, 91)), grid=grid, aabb=[lo.tolist(), hi.tolist()],
                near_far=near_far, step_ratio=float(g.choice([0.5, 1.0, 2.0])), density_scale=float(g.uniform(0.5, 1.4)),
                white_train=bool(g.integers(0, 2)), grad_train=bool(g.integers(0, 2)), ndc=bool(ndc), mask=bool(mask), seed0=32000 + 16 * seed)


def all_cases():
    return list(DIRECTED.values()) + [fuzz_case(s) for s in FUZZ_SEEDS]


def case_by_name(name):
    return DIRECTED[name] if name in DIRECTED else fuzz_case(int(name[len("fuzz"):]))


# ---- building a case: parameters, oracle configuration, field, random draws ----------------------------------------------------------
def make_params(case, seed):
    kw = case.kw
    return synth.make_field_params(int(seed), case.grid, density_n_comp=kw["density_n_comp"], app_n_comp=kw["appearance_n_comp"],
                                   app_dim=kw["app_dim"], feature_c=kw["featureC"], fea_pe=kw["fea_pe"], shading_mode=kw["shadingMode"],
                                   density_scale=case.density_scale, app_scale=case.app_scale, aabb=case.aabb, view_pe=kw["view_pe"], pos_pe=kw["pos_pe"])


MASK_GRID = (21, 18, 15)


def mask_volume(case, params):
    """The oracle's getDenseAlpha / updateAlphaMask of this field on MASK_GRID. The threshold is a percentile of the dense alphas
    themselves — the first of 70 / 85 / 95 / 99 whose 3 x 3 x 3-dilated volume drops at least a tenth of the voxels — so that the mask
    does remove samples whatever the field's density scale."""
    cfg = make_cfg(case)
    alpha, xyz = O.dense_alpha(cfg, O.params_from_numpy(params), MASK_GRID)
    for q in (0.70, 0.85, 0.95, 0.99):
        vol, _ = O.alpha_volume(alpha, xyz, max(float(torch.quantile(alpha.reshape(-1), q)), 1e-30))
        if float(vol.mean()) <= 0.9:
            break
    return vol.numpy().astype(np.float32)


def make_cfg(case, vol=None):
    kw = case.kw
    return O.FieldConfig(aabb=case.aabb, grid_size=case.grid, near_far=case.near_far, density_shift=float(case.density_shift),
                         step_ratio=case.step_ratio, fea_pe=kw["fea_pe"], view_pe=kw["view_pe"], pos_pe=kw["pos_pe"],
                         shading_mode=kw["shadingMode"], alpha_volume=None if vol is None else torch.from_numpy(vol),
                         alpha_aabb=None if vol is None else case.aabb)


def make_field(case, params, device, vol=None):
    from text2nerf_amd import AlphaGridMask, TensorVMSplit
    m = TensorVMSplit(torch.tensor(case.aabb, dtype=torch.float32), list(case.grid), device, near_far=list(case.near_far),
                      alphaMask_thres=1e-4, density_shift=case.density_shift, distance_scale=25, step_ratio=case.step_ratio,
                      fea2denseAct="softplus", **case.kw)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    if vol is not None:
        m.alphaMask = AlphaGridMask(device, torch.tensor(case.aabb, dtype=torch.float32), torch.from_numpy(vol).to(device))
    return m


def draws(case, is_train):
    """What the render call draws in train mode, fixed per case: (N, jitter, add_bg). jitter: [R, 1] per-ray offsets, or the [1, N]
    shared row on NDC rays; add_bg: the background the call composites (white_bg, or the train-mode coin on a black one)."""
    if not is_train:
        return case.n_eval, None, True
    N = case.n_train
    g = np.random.Generator(np.random.PCG64(case.seed0 + 7))
    jit = torch.from_numpy(g.uniform(0.0, 1.0, (1, N) if case.ndc else (case.R, 1)).astype(np.float32))
    coin = bool(g.integers(0, 2))
    return N, jit, True if case.white_train else coin


def oracle(case, params, is_train, dtype=torch.float64, vol=None, requires_grad=False, return_aux=False, idx=None):
    """oracle_torch.forward on this case: float64 parameters on the reference's float32 sample geometry by default (the
    high-precision reference form of tests/test_train_step_fullsize.py); dtype float32: the plain float32 oracle. `idx`: a subset
    of the case's rays (with their jitter draws)."""
    N, jit, add_bg = draws(case, is_train)
    rays = torch.from_numpy(case.rays)
    if idx is not None:
        rays = rays[idx]
        if jit is not None and not case.ndc:
            jit = jit[idx]
    cfg = make_cfg(case, vol)
    P = O.params_from_numpy(params, dtype=dtype, requires_grad=requires_grad)
    out = O.forward(cfg, P, rays, white_bg=add_bg, is_train=is_train, n_samples=N, jitter=jit, ndc=case.ndc,
                    return_aux=return_aux, geom_dtype=torch.float32 if dtype == torch.float64 else None)
    return out, P


def grad_loss(rgb, depth, w, ca):
    return (rgb * ca).sum() + 0.1 * depth.sum() + (w ** 2).sum()       # tests/test_generic_gpu.py's


def colour_weights(case, n):
    g = np.random.Generator(np.random.PCG64(case.seed0 + 9))
    return torch.from_numpy(g.uniform(-1, 1, (case.R, 3)).astype(np.float32))[:n]


RELU_MARGIN = 5e-6          # tests/golden/make_golden_shapes.py::relu_margin
SEED_STEPS = 8
RELU_INPUTS = 25000         # ReLU inputs of the gradient pass (see grad_rays)


def grad_rays(case):
    """Indices of the rays of the gradient comparison. A pass with n ReLU inputs of density p near zero keeps all of them RELU_MARGIN
    away from zero with probability exp(-2 RELU_MARGIN n p): for p ~ 1.3 (pre-activations of spread 0.3) and n = 25 000 that is
    seven seeds in ten (one in two for a head whose pre-activations are three times narrower), so eight steps almost always find one;
    at the 700 000 inputs of a whole 221-ray frame with 130 units no seed ever passes. The subset is therefore evenly spaced rays, as many as keep 2 featureC (3 for SH) inputs per appearance sample of the
    seed0 field under RELU_INPUTS; the RGB head has no ReLU and keeps every ray."""
    head, R = case.kw["shadingMode"], case.R
    per = 2 * case.kw["featureC"] if head in MLP_HEADS else 3 if head == "SH" else 0
    if not per:
        return np.arange(R)
    params = make_params(case, case.seed0)
    vol = mask_volume(case, params) if case.mask else None
    with torch.no_grad():
        (_, _, _, w), _ = oracle(case, params, case.grad_train, dtype=torch.float32, vol=vol)
    A = int((w > 1e-4).sum())
    k = R if A * per <= RELU_INPUTS else max(4, int(R * RELU_INPUTS / (A * per)))
    return np.unique(np.linspace(0, R - 1, k).astype(np.int64))


@functools.lru_cache(maxsize=None)
def relu_safe_seed(name):
    """The first parameter seed from the case's seed0 upwards whose gradient pass keeps every ReLU input of the head (hidden
    pre-activations, SH's pre-ReLU colours; float64 oracle) at least RELU_MARGIN away from zero: (seed, steps walked, margin, ray
    indices of the gradient pass). Deterministic, CPU only; raises after SEED_STEPS steps."""
    case = case_by_name(name)
    idx = grad_rays(case)
    for step in range(SEED_STEPS):
        seed = case.seed0 + step
        params = make_params(case, seed)
        vol = mask_volume(case, params) if case.mask else None
        with torch.no_grad():
            (_, _, _, _, aux), _ = oracle(case, params, case.grad_train, vol=vol, return_aux=True, idx=idx)
        margin = min([float(p.abs().min()) for p in aux["relu_pre"] if p.numel()] or [float("inf")])
        if margin >= RELU_MARGIN:
            return seed, step, margin, idx
    raise AssertionError(f"{name}: no ReLU-safe parameter seed within {SEED_STEPS} steps of {case.seed0}")
