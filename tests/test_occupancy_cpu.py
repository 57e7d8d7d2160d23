"""CPU half of the element-wise checks of the occupancy-mask, resize and ray-filter stages (tests/test_occupancy_gpu.py runs the kernels):
the float64 references of tests/helpers/occupancy_ref.py pinned against torch and the oracle, the claims of the case table
(tests/helpers/occupancy_cases.py: every case reaches the edge it names, every directed case is decided by the reference alone, the
seeded ones leave at most 2 % undecided), the float32 oracle held to the same laws as the device, and every mutation rejected."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from oracle import oracle_torch as O
from tests.helpers import occupancy_cases as T
from tests.helpers import occupancy_ref as R

F32 = np.float32


# ---- occupancy volume --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.volume_cases()))
def test_volume_reference_is_max_pool3d_and_the_oracle(name):
    c = T.volume_cases()[name]
    dense, thres = c["dense"], c["thres"]
    vol, box = R.alpha_volume(dense, thres)
    a = torch.from_numpy(dense).clamp(0, 1).transpose(0, 2).contiguous()
    pooled = Fn.max_pool3d(a[None, None], kernel_size=3, padding=1, stride=1)[0, 0]
    assert np.array_equal(vol, (pooled >= thres).float().numpy())
    g = dense.shape
    lins = T.linspaces(g)
    xyz = torch.from_numpy(R.dense_nodes(T.FIELD_AABB, lins))
    if vol.any():
        o_vol, o_aabb = O.alpha_volume(torch.from_numpy(dense), xyz, thres)
        assert np.array_equal(vol, o_vol.numpy())
        assert np.array_equal(R.box_to_aabb(T.FIELD_AABB, lins, box), o_aabb.numpy())
    else:
        assert box.tolist() == [R.INT_MAX] * 3 + [-1] * 3


def test_volume_cases_reach_their_edges():
    C = T.volume_cases()
    for name in ("tail_257", "corner", "far_corner", "face", "interior", "last_workgroup", "two_workgroups", "above_one", "at_threshold"):
        c = C[name]
        vol, box = R.alpha_volume(c["dense"], c["thres"])
        g = c["dense"].shape
        want = T.neighbourhood(g, c["hot"])
        assert np.array_equal(vol, want), name
        z, y, x = np.nonzero(want)
        assert box.tolist() == [x.min(), y.min(), z.min(), x.max(), y.max(), z.max()], name
    assert C["tail_257"]["dense"].size == 257
    wg = lambda vol: set((np.flatnonzero(vol.reshape(-1)) // 256).tolist())       # the kernel's thread index is the volume's flat index
    v, _ = R.alpha_volume(C["last_workgroup"]["dense"], 0.5)
    n = v.size
    assert wg(v) == {(n - 1) // 256} and n % 256 and (n + 255) // 256 == 12
    v, box = R.alpha_volume(C["two_workgroups"]["dense"], 0.5)
    assert len(wg(v)) >= 4 and box.tolist() == [0, 0, 0, 12, 14, 15] and v.size == 3120 and (v.size + 255) // 256 == 13
    v, _ = R.alpha_volume(C["corner"]["dense"], 0.5)
    assert v.sum() == 8 and v[0, 0, 0] == 1
    v, _ = R.alpha_volume(C["face"]["dense"], 0.5)
    assert v.sum() == 18
    assert C["above_one"]["dense"].max() > 1 and min(c["dense"].min() for c in C.values()) < 0
    v, box = R.alpha_volume(C["ulp_below_threshold"]["dense"], C["ulp_below_threshold"]["thres"])
    assert not v.any() and box.tolist() == [R.INT_MAX] * 3 + [-1] * 3
    d = C["at_threshold"]["dense"]
    assert d[2, 3, 4] == F32(C["at_threshold"]["thres"]) and d[9, 10, 11] < F32(C["at_threshold"]["thres"]) and d[9, 10, 11] > 0.29999
    v, box = R.alpha_volume(C["thres_zero"]["dense"], 0.0)
    assert v.all() and box.tolist() == [0, 0, 0, 4, 5, 6] and C["thres_zero"]["dense"].max() < 0.2
    v, _ = R.alpha_volume(C["thres_above_one"]["dense"], 1.5)
    assert not v.any() and C["thres_above_one"]["dense"].max() > 1.5
    assert np.gcd.reduce([7, 11, 13]) == 1


@pytest.mark.parametrize("mutate", R.VOLUME_MUTATIONS)
def test_volume_mutations_are_rejected(mutate):
    rejected = []
    for name, c in T.volume_cases().items():
        vol, box = R.alpha_volume(c["dense"], c["thres"], mutate=mutate)
        if R.check_volume(vol, box, c["dense"], c["thres"])["bad"]:
            rejected.append(name)
        assert not R.check_volume(*R.alpha_volume(c["dense"], c["thres"]), c["dense"], c["thres"])["bad"]
    must = {"no_transpose": "random_7x11x13", "pool6": "interior", "gt": "at_threshold", "box_max_off": "corner",
            "box_before_dilation": "interior"}[mutate]
    assert must in rejected, (mutate, rejected)


# ---- resize ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", T.RESIZE_PAIRS, ids=lambda p: "%dx%d-%dx%d" % (p[0] + p[1]))
def test_resize_reference_is_interpolate_and_float32_meets_the_law(pair):
    (hin, win), (hout, wout) = pair
    for C in T.RESIZE_CHANNELS:
        src = T.resize_input(C, hin, win)
        want, bound = R.resize(src, hout, wout)
        t = Fn.interpolate(torch.from_numpy(src).double()[None], size=(hout, wout), mode="bilinear", align_corners=True)[0].numpy()
        assert np.abs(want - t).max() <= 1e-12 * np.abs(src).max()
        got = O.upsample_bilinear(torch.from_numpy(src)[None], hout, wout)[0].numpy()          # the float32 restatement of ATen's
        r = R.check_resize(got, src, hout, wout)
        assert r["bad"] == 0 and r["ratio"] <= 1.0, (pair, C, r)
        t32 = Fn.interpolate(torch.from_numpy(src)[None], size=(hout, wout), mode="bilinear", align_corners=True)[0].numpy()
        if (hin, win) != (hout, wout):
            assert R.check_resize(t32, src, hout, wout)["bad"] == 0


def test_resize_cases_reach_their_edges():
    for ((hin, win), (hout, wout)), (rows, cols) in T.RESIZE_INTEGER.items():
        assert (len(R.integer_source_rows(hin, hout)) > 0) == rows and (len(R.integer_source_rows(win, wout)) > 0) == cols
    pairs = T.RESIZE_PAIRS
    assert any(p[0][0] == 1 for p in pairs) and any(p[1] == (1, 1) for p in pairs) and any(p[0] == p[1] for p in pairs)
    assert any(p[0][0] == 2 for p in pairs) and any(p[1][0] < p[0][0] for p in pairs)
    # the index term is exercised: somewhere it is the larger part of the bound
    src = T.resize_input(3, 24, 20)
    _, b = R.resize(src, 47, 39)
    mag_only = R.K_RESIZE * R.U * 1000.0
    assert (b > 2 * mag_only).any()
    assert not (T.resize_input(48, 24, 20) == 0).any()


@pytest.mark.parametrize("mutate", R.RESIZE_MUTATIONS)
def test_resize_mutations_are_rejected(mutate):
    rejected = []
    for (hin, win), (hout, wout) in T.RESIZE_PAIRS:
        src = T.resize_input(3, hin, win)
        got = R.resize(src, hout, wout, mutate=mutate)[0]
        if R.check_resize(got.astype(F32), src, hout, wout)["bad"]:
            rejected.append(((hin, win), (hout, wout)))
    assert ((24, 20), (47, 39)) in rejected and ((4, 6), (10, 16)) in rejected, (mutate, rejected)


# ---- mask sample ------------------------------------------------------------------------------------------------------------------------------
MASK_CASES = [(d, b) for d in T.MASK_DIMS for b in T.MASK_BOXES]


def grid_sample64(vol, box, pts):
    a = torch.tensor(box, dtype=torch.float32).double()
    g = (torch.from_numpy(pts).double() - a[0]) * (2.0 / (a[1] - a[0])) - 1
    return Fn.grid_sample(torch.from_numpy(vol).double()[None, None], g.view(1, -1, 1, 1, 3), mode="bilinear", padding_mode="zeros",
                          align_corners=True).view(-1).numpy()


@pytest.mark.parametrize("dims,boxname", MASK_CASES)
def test_mask_sample_reference_claims_and_float32_oracle(dims, boxname):
    box = T.MASK_BOXES[boxname]
    directed, cloud = T.mask_points(dims, box)
    for kind in ("binary", "real"):
        vol = T.mask_volume(dims, kind)
        cfg = O.FieldConfig(aabb=T.FIELD_AABB, grid_size=[24, 20, 16], alpha_volume=torch.from_numpy(vol), alpha_aabb=box)
        for pts, is_directed in ((directed, True), (cloud, False)):
            r = R.mask_sample(vol, box, pts)
            scale = np.abs(vol).max()
            assert np.abs(r["value"] - grid_sample64(vol, box, pts)).max() <= 1e-9 * scale
            assert np.abs(r["value"] - O.sample_alpha(cfg, torch.from_numpy(pts).double()).numpy()).max() <= 1e-9 * scale
            if kind == "binary":
                und = (~r["decided"]).sum()
                assert und == 0 if is_directed else und <= T.UNDECIDED_CAP * len(pts), (und, len(pts))
                assert r["hit"].any() and (~r["hit"]).any()
            got = O.sample_alpha(cfg, torch.from_numpy(pts)).numpy()                # float32, the operations the kernel restates
            c = R.check_mask_sample(got, vol, box, pts)
            assert len(c["bad"]) == 0 and c["ratio"] <= 1.0, (kind, is_directed, c)
    # the directed set holds the points it names: nodes, one float32 step inside and outside every face, far away
    ix, _ = R.mask_index(box, dims, directed)
    S = np.array([dims[2], dims[1], dims[0]])
    assert (np.abs(ix - np.round(ix)).max(-1) < 1e-5).sum() >= (dims[0] * dims[1] * (dims[2] - 2))
    a = np.asarray(box, F32)
    for k in range(3):
        for side in (0, 1):
            col = directed[:, k]
            f = a[side, k]
            assert (col == f).any() and (col == np.nextafter(f, F32(np.inf))).any() and (col == np.nextafter(f, F32(-np.inf))).any()
    assert (np.abs(ix) > 2 * S.max()).any()


def test_mask_sample_border_mutation_is_rejected():
    dims, box = (5, 7, 11), T.MASK_BOXES["larger"]
    directed, cloud = T.mask_points(dims, box)
    pts = np.concatenate([directed, cloud])
    for kind in ("binary", "real"):
        vol = T.mask_volume(dims, kind)
        got = R.mask_sample(vol, box, pts, mutate="border")["value"].astype(F32)
        assert len(R.check_mask_sample(got, vol, box, pts)["bad"]) > 0
        assert len(R.check_mask_sample(R.mask_sample(vol, box, pts)["value"].astype(F32), vol, box, pts)["bad"]) == 0


# ---- alpha filter ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", T.FILTER_N)
def test_filter_directed_rays_are_decided_and_the_float32_oracle_agrees(n):
    cfg = T.cfg_a(T.slab_mask())
    assert cfg.step_size == T.STEP_A
    rays, want = T.filter_rays(n)
    ref = R.filter_alpha(cfg, rays, n)
    assert ref["decided"].all() and np.array_equal(ref["keep"], want)
    assert set(T.filter_ks(n)) == {k for k in (0, 1, 63, 64, 65, n - 1, n) if 0 <= k <= n}
    # the first sample inside the support really is sample k, half a step behind the support's face
    pts, _, _ = O.sample_ray(cfg, torch.from_numpy(rays[:, :3]).double(), torch.from_numpy(rays[:, 3:6]).double(), n)
    x = pts[:len(T.filter_ks(n)), :, 0].numpy()
    for row, k in zip(x, T.filter_ks(n)):
        inside = (row > 1) & (row < 3)
        assert (np.argmax(inside) == k and row[k] - 1 == T.STEP_A / 2) if k < n else not inside.any()
    got = O.filter_rays_alpha(cfg, torch.from_numpy(rays), n).numpy()
    assert len(R.check_flags(got.astype(np.uint8), ref)["bad"]) == 0


def test_filter_oblique_rays_undecided_share():
    cfg = T.cfg_a(T.blob_mask())
    rays = T.oblique_rays()
    ref = R.filter_alpha(cfg, rays, 128)
    und = int((~ref["decided"]).sum())
    assert und <= T.UNDECIDED_CAP * len(rays), und
    assert 0.1 < ref["keep"].mean() < 0.9
    got = O.filter_rays_alpha(cfg, torch.from_numpy(rays), 128).numpy()
    assert len(R.check_flags(got.astype(np.uint8), ref)["bad"]) == 0


@pytest.mark.parametrize("mutate", R.FILTER_MUTATIONS)
def test_filter_mutations_are_rejected(mutate):
    cfg = T.cfg_a(T.slab_mask())
    rejected = []
    for n in T.FILTER_N:
        rays, _ = T.filter_rays(n)
        ref = R.filter_alpha(cfg, rays, n)
        got = R.filter_alpha(cfg, rays, n, mutate=mutate)["keep"].astype(np.uint8)
        if len(R.check_flags(got, ref)["bad"]):
            rejected.append(n)
    assert rejected == ([65, 128, 129, 256] if mutate == "first64" else list(T.FILTER_N)), rejected
    ref = R.filter_alpha(cfg, *T.filter_rays(64)[:1], 64)
    assert len(R.check_flags(np.full(len(ref["keep"]), 0xAB, np.uint8), ref)["bad"]) == len(ref["keep"])      # an unwritten byte


# ---- slab test ------------------------------------------------------------------------------------------------------------------------------------
def slab32(aabb, rays):
    """models/tensorBase.py:385-391 in float32 torch."""
    a = torch.tensor(aabb, dtype=torch.float32)
    r = torch.from_numpy(rays)
    o, d = r[:, :3], r[:, 3:6]
    vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
    ra, rb = (a[1] - o) / vec, (a[0] - o) / vec
    return (torch.maximum(ra, rb).amin(-1) > torch.minimum(ra, rb).amax(-1)).numpy()


def test_slab_directed_rays_are_decided():
    rays, want, names = T.bbox_rays()
    ref = R.slab(T.FB["aabb"], rays)
    assert ref["decided"].all(), [n for n, d in zip(names, ref["decided"]) if not d]
    assert np.array_equal(ref["keep"], want), [n for n, k, w in zip(names, ref["keep"], want) if k != w]
    m = dict(zip(names, ref["margin"]))
    assert m["graze_edge"] == 0 and m["graze_corner"] == 0 and m["clip_edge_one_step"] == 2.0 ** -22 == m["clip_corner_one_step"]
    assert np.array_equal(slab32(T.FB["aabb"], rays), want)
    signs = {(n.split("_")[1][-1], bool(np.signbit(r[3:6][r[3:6] == 0]).any())) for n, r in zip(names, rays) if n.startswith("axis")}
    assert signs == {("p", False), ("n", True)}
    assert len(rays) == 11 + 24


def test_slab_seeded_rays_undecided_share():
    rays = T.bbox_seeded()
    ref = R.slab(T.FB["aabb"], rays)
    assert (~ref["decided"]).sum() <= T.UNDECIDED_CAP * len(rays)
    assert 0.1 < ref["keep"].mean() < 0.9 and (rays[:, 3:6] == 0).any()
    assert len(R.check_flags(slab32(T.FB["aabb"], rays).astype(np.uint8), ref)["bad"]) == 0


@pytest.mark.parametrize("mutate", R.SLAB_MUTATIONS)
def test_slab_mutations_are_rejected(mutate):
    rays, _, names = T.bbox_rays()
    ref = R.slab(T.FB["aabb"], rays)
    got = R.slab(T.FB["aabb"], rays, mutate=mutate)["keep"].astype(np.uint8)
    bad = {names[i] for i in R.check_flags(got, ref)["bad"]}
    assert bad == ({"graze_edge", "graze_corner"} if mutate == "ge" else {"on_face_zero_dir_pos", "on_face_zero_dir_neg"}), bad


# ---- alpha at points and dense nodes -----------------------------------------------------------------------------------------------------------
def small_length(cfg, pts):
    """The length that puts the median live alpha at 1e-4 (the default alphaMask_thres), as a float32 number."""
    s = R.alpha_at_points(cfg, T.tiny_params(), pts, 1.0)["sigma"]
    return float(F32(1e-4 / np.median(s)))


@pytest.mark.parametrize("maskname", list(T.alpha_masks()))
def test_alpha_reference_claims_and_float32_oracle(maskname):
    mask = T.alpha_masks()[maskname]
    cfg = T.tiny_cfg(mask)
    params = T.tiny_params()
    directed, cloud = T.box_points()
    nodes = [R.dense_nodes(T.TINY["aabb"], T.linspaces(g)).reshape(-1, 3) for g in T.DENSE_GRIDS]
    assert [4 * len(n) % 256 for n in nodes] == [4, 420 % 256, 120, 0, 2772 % 256]
    directed = np.concatenate([directed] + nodes)
    P64 = O.params_from_numpy(params, dtype=torch.float64)
    P32 = O.params_from_numpy(params)
    for bf16 in (False, True):
        if bf16:
            P64, P32 = O.round_factors_bf16(P64), O.round_factors_bf16(P32)
        for pts, is_directed in ((directed, True), (cloud, False)):
            L_small = small_length(cfg, pts)
            for length in (cfg.step_size, T.LENGTH_SATURATE, L_small):
                ref = R.alpha_at_points(cfg, params, pts, length, bf16=bf16)
                und = int((~ref["decided"]).sum())
                assert und == 0 if is_directed else und <= T.UNDECIDED_CAP * len(pts)
                # pinned to the all-float64 oracle: they differ by the float32 rounding of the normalised position only (some 1e-6 of a
                # cell times the feature's slope, carried through the activation; the law itself is held on the float32 oracle below)
                o64 = O.compute_alpha(cfg, P64, torch.from_numpy(pts).double(), float(F32(length))).numpy()
                assert np.abs(o64 - ref["alpha"])[ref["decided"]].max() <= 2e-4 * max(ref["alpha"].max(), 1e-30)
                got = O.compute_alpha(cfg, P32, torch.from_numpy(pts), float(F32(length))).numpy()
                c = R.check_alpha(got, ref)
                assert len(c["bad"]) == 0, (maskname, bf16, length, c)
                live = ~ref["masked"]
                if length == T.LENGTH_SATURATE:
                    assert (ref["alpha"][live] >= 1 - 2.0 ** -26).any()
                if length == L_small:
                    assert ((ref["alpha"][live] > 0.5e-4) & (ref["alpha"][live] < 2e-4)).any()
            if mask is not None:
                assert ref["masked"].any() and (~ref["masked"]).any()
    # a wrong density (bf16 factors where float32 ones are stored) does not pass
    ref = R.alpha_at_points(cfg, params, cloud, cfg.step_size, bf16=False)
    got = O.compute_alpha(cfg, O.round_factors_bf16(O.params_from_numpy(params)), torch.from_numpy(cloud), cfg.step_size).numpy()
    assert len(R.check_alpha(got, ref)["bad"]) > 0


def test_dense_nodes_restate_the_reference_lerp():
    for g in T.DENSE_GRIDS:
        lins = T.linspaces(g)
        a = torch.tensor(T.TINY["aabb"], dtype=torch.float32)
        s = torch.stack(torch.meshgrid(*[torch.from_numpy(l) for l in lins], indexing="ij"), -1)
        want = (a[0] * (1 - s) + a[1] * s).numpy()
        assert np.array_equal(R.dense_nodes(T.TINY["aabb"], lins).view(np.uint32), want.view(np.uint32))


# ---- host chain ------------------------------------------------------------------------------------------------------------------------------------
def test_chain_case_shrinks_and_filters():
    case, params = T.CHAIN, T.chain_params()
    g = case["mask_grid"]
    cfg0 = O.FieldConfig(aabb=case["aabb"], grid_size=case["grid"], near_far=case["near_far"])
    alpha, _ = O.dense_alpha(cfg0, O.params_from_numpy(params), g)
    rays = T.chain_rays()
    c = R.chain(case, params, alpha.numpy(), T.linspaces(g), rays, 256)
    assert len(set(g)) == 3 and len(set(case["grid"])) == 3
    assert c["shrunk_grid"] != list(case["grid"]) and all(n >= 2 for n in c["shrunk_grid"])      # shrink crops, on every axis a grid remains
    assert 0 < c["volume"].mean() < 1
    f = c["filter"]
    assert (~f["decided"]).sum() <= T.UNDECIDED_CAP * len(rays) and 0.1 < f["keep"].mean() < 0.9
    assert any(a != b for a, b in zip(c["shrunk_grid"], case["upsample"]))
