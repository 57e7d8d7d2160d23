"""The marchers' per-ray records and appearance lists, entry by entry against float64 (k_march, k_march_tiles in every form a frame
runs, k_compact_list, k_composite), and the hand-written activation on chosen arguments.

Reference, law (K = 4) and checkers: tests/helpers/march_ref.py; tests/test_march_list_cpu.py settles the law on the float32 oracles and
shows that every checker catches its mutations. Every case here proves which path ran (density_cache_counts, feature_fusion_counts,
row_staging_counts, stats) and then runs every checker its outputs allow: records, entries, acc_depth, composite (fused MLP head, white
background), weights_rows (materialised weights). One `MARCHLIST gpu` line per launch keeps the largest err / (K b) per checker
(profiles/march_list_elementwise.txt).

Out of scope:
- early termination: the entries behind a terminated ray depend on the eight-pair look cadence (tests/test_early_termination.py bounds it);
- NDC rays and general-shape fields;
- t2n_train_step's own workspace;
- the colours of the rays k_finish_rays finishes (tests/test_list_budget.py): their records, acc and depth are checked here."""
import numpy as np
import pytest
import torch

from text2nerf_amd import _lib, tensorf
from tests.helpers import march_ref as M
from tests.helpers.march_lists import dev, frame_lists, list_shape

pytestmark = pytest.mark.gpu

TILE_LISTS = ("tile_uncached", "tile_cached", "tile_direct", "tile_staged")      # the lists-only forms of the tile marcher
FORMS = ("per_ray", "per_ray_dense") + TILE_LISTS + ("tile_dense",)
_FIELDS = {}


def field_of(c):
    key = (c["seed"], tuple(c["grid"]), c["scale"], c["act"])
    if key not in _FIELDS:
        from text2nerf_amd import TensorVMSplit
        f = TensorVMSplit(torch.tensor(c["aabb"], dtype=torch.float32), list(c["grid"]), dev(), density_n_comp=[16] * 3,
                          appearance_n_comp=[48] * 3, app_dim=27, near_far=c["near_far"], shadingMode="MLP_Fea_noview", alphaMask_thres=1e-4,
                          density_shift=-10, distance_scale=25, pos_pe=0, view_pe=0, fea_pe=6, featureC=128, step_ratio=1.0,
                          fea2denseAct=c["act"])
        f.load_state_dict({k: torch.from_numpy(v) for k, v in c["params"].items()}, strict=True)
        f.appearance_volume_min_frames = 1          # the feature volume exists from the first tile-marcher frame
        _FIELDS[key] = f
    f = _FIELDS[key]
    f.rayMarch_weight_thres = c["thres"]
    f.factor_storage = "bf16" if c["bf16"] else "fp32"
    f.alphaMask = None
    if c["mask"]:
        from tests.test_density_cache import alpha_mask
        f.alphaMask = alpha_mask() if c["mask"] == "mask" else tensorf.AlphaGridMask(dev(), torch.tensor(c["aabb"]),
                                                                                   torch.from_numpy(M.mask_volume(c["mask"])))
        assert torch.equal(f.alphaMask.alpha_volume.cpu().reshape(7, 6, 5), torch.from_numpy(M.mask_volume(c["mask"])))
    return f


def paths(f):
    d, u = f.density_cache_counts(), f.feature_fusion_counts()
    return np.array([d["cached"], d["uncached"], u["fused"], u["unfused"]])


def launch(f, c, form, rays, budget=0):
    """One frame of the case in the form, with the proof of the path it took; the lists it left and its outputs, on the host."""
    (H, W), N, R = c["HW"], c["N"], rays.shape[0]
    tile = form.startswith("tile")
    f.frame_width = W if tile else 0
    f.materialize_weights = form.endswith("dense")
    f.density_cache = form != "tile_uncached"
    f.feature_fusion = form in ("tile_direct", "tile_staged")
    f.row_staging = form != "tile_direct"
    fusable = form in ("tile_direct", "tile_staged") and not c["mask"]
    want = {"per_ray": (0, 0, 0, 0), "per_ray_dense": (0, 0, 0, 0), "tile_uncached": (0, 1, 0, 1), "tile_cached": (1, 0, 0, 1),
            "tile_direct": (1, 0, 1, 0) if fusable else (1, 0, 0, 1), "tile_staged": (1, 0, 1, 0) if fusable else (1, 0, 0, 1),
            "tile_dense": (1, 0, 0, 1)}[form]
    if fusable:
        assert list_shape(R, N, budget)["fusable"]
    for attempt in range(3):      # the first tile-marcher frame of a factor version builds the feature volume, the second the table
        p0 = paths(f)
        with torch.no_grad():
            rgb, depth, z, w = f(rays, N_samples=N)
        took = tuple(paths(f) - p0)
        if took == want:
            break
    assert took == want, (form, took, want)
    st = f.stats()
    waves = f.row_staging_counts() if fusable else {"staged": 0, "direct": 0}
    if form == "tile_direct" and fusable:
        assert waves == {"staged": 0, "direct": 0}, waves
    assert (w is not None) == form.endswith("dense")
    L = frame_lists(R, N, budget, finished=budget > 0)
    L.update(depth=depth, rgb_out=rgb, weights=w, z_vals=z)
    L = M.host(L)
    L["stats"], L["waves"] = st, waves
    kept = (L["slot0"] >= 0) & (L["ray_app"][:, 0] > 0) & (L["ray_app"][:, 0] <= max(N // 4, 1))     # rays whose entries stayed in their wave's region
    if form == "tile_staged" and fusable and kept.any():
        assert waves["staged"] + waves["direct"] > 0, waves
    if not budget:
        assert st["evaluated"] == int(L["ray_app"][:, 1].sum()) and st["appearance"] == int(L["ray_app"][:, 0].sum())
    return L


def check_all(name, form, ref, L):
    """Every checker the launch's outputs allow; prints the MARCHLIST line, then asserts."""
    bad = {"records": ref.check_records(L), "entries": ref.check_entries(L)}
    d = dict(ref.detail)
    bad["acc_depth"] = ref.check_acc_depth(L["acc"], L["depth"])
    d.update(ref.detail)
    bad["composite"] = ref.check_composite(L, L["rgb_out"])
    d.update(ref.detail)
    if L["weights"] is not None:
        bad["weights_rows"] = ref.check_weights_rows(L["weights"], L["z_vals"])
        d.update(ref.detail)
    st = ref.band_stats()
    print(f"MARCHLIST gpu {name} {form} rays {ref.R} N {ref.N} entries {d['entries']} band {st['band']} either {st['either']} "
          f"(present {d['either_present']}) waves {L['waves']} err/(K b): w {d['w']:.3f} acc {d['acc']:.3f} depth {d['depth']:.3f} "
          f"composite {d['composite']:.3f}" + (f" rows {d['rows']:.3f}" if "rows" in d else "") + f" finished {int((L['slot0'] < 0).sum())}")
    assert all(len(v) == 0 for v in bad.values()), (name, form, {k: v[:8].tolist() for k, v in bad.items() if len(v)})


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.int32), np.ascontiguousarray(b[k]).view(np.int32))
               for k in ("entries", "ray_app", "acc", "depth"))


def run_case(name, forms):
    c, ref = M.case(name), M.reference(name)
    f = field_of(c)
    rays = torch.from_numpy(c["rays"]).to(dev())
    out = {}
    try:
        for form in forms:
            out[form] = launch(f, c, form, rays)
            check_all(name, form, ref, out[form])
    finally:
        f.frame_width, f.materialize_weights, f.density_cache, f.feature_fusion, f.row_staging = 0, True, True, True, True
        f.alphaMask, f.factor_storage = None, "fp32"
    # position independence: a ray's entries and record are the same bits in every form of the tile marcher, so the float64 check of
    # one form speaks for the others
    tiles = [k for k in forms if k.startswith("tile")]
    for k in tiles[1:]:
        assert same_bits(out[tiles[0]], out[k]), f"{name}: {k} differs from {tiles[0]}"
    return out


# ---- forms: cameras x frames over the softplus fp32 field of both grids ---------------------------------------------------------------
@pytest.mark.parametrize("name", M.GEOMETRY)
def test_forms(name):
    run_case(name, FORMS)


# ---- variants ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", M.VARIANTS)
def test_variants(name):
    out = run_case(name, FORMS)
    if name.startswith("sparse"):
        ra = out["tile_cached"]["ray_app"]
        assert int(((ra[:, 2] >> 11) - ra[:, 1] > 0).sum()) > 0       # windows with gaps


# ---- routes ------------------------------------------------------------------------------------------------------------------------------
def test_compact_list():
    """Rays with more entries than their staging slice holds (N / 4) go through k_compact_list."""
    out = run_case("compact", FORMS)
    n_app = out["tile_staged"]["ray_app"][:, 0]
    assert int((n_app > M.case("compact")["N"] // 4).sum()) > 0


def test_direct_gather_pairs():
    """Step pairs whose taps span more than four texels gather directly; both kinds occur in this frame."""
    from tests.test_march_summed_table import step_pairs
    c = M.case("gather")
    for dense in (False, True):
        pairs = step_pairs(c["rays"], *c["HW"], c["aabb"], c["grid"], c["near_far"], c["N"], dense)
        n_table = sum(1 for p in pairs if p[0])
        assert n_table >= 50 and len(pairs) - n_table >= 50, (dense, n_table, len(pairs))
    field_of(c).appearance_volume = False        # (a 300^3 feature volume is not what this case is about)
    run_case("gather", ("per_ray", "tile_uncached", "tile_cached", "tile_dense"))


def test_training_form():
    """The per-ray marcher through f(rays, is_train=True): the jitter draw is captured by test_g6_forward_train_rng_stream's recipe."""
    c, ref = M.case("train"), M.reference("train")
    f = field_of(c)
    f.frame_width, f.materialize_weights = 0, True
    rays = torch.from_numpy(c["rays"])
    p0 = paths(f)
    torch.manual_seed(123)
    with torch.no_grad():
        rgb, depth, z, w = f(rays, is_train=True, white_bg=True, N_samples=c["N"])
    assert tuple(paths(f) - p0) == (0, 0, 0, 0)
    assert np.array_equal(z.cpu().numpy().astype(np.float64), ref.ray.z), "the captured jitter is not the draw the forward made"
    L = frame_lists(rays.shape[0], c["N"])
    L.update(depth=depth, rgb_out=rgb, weights=w, z_vals=z)
    L = M.host(L)
    L["waves"] = {"staged": 0, "direct": 0}
    check_all("train", "per_ray_train", ref, L)


def test_finisher():
    """An overflowing budget (tests/test_list_budget.py's frame, 2 entries per ray where ~5 are needed): the rays k_finish_rays colours
    have ray_app.x < 0 and correct records, acc and depth; every other ray passes every checker. The reference covers every 13th ray."""
    c, ref = M.case("finisher"), M.reference("finisher")
    f = field_of(c)
    rays = torch.from_numpy(c["all_rays"]).to(dev())
    R, N = rays.shape[0], c["N"]
    assert N == f.nSamples
    f.workspace_bytes_override = int(_lib.load().t2n_render_workspace_bytes_budget(R, N, c["budget"]))
    try:
        L = launch(f, c, "tile_staged", rays, budget=c["budget"])
        assert L["stats"]["list_retry"] == 1
        part = M.subset(L, c["rows"])
        finished = int((part["slot0"] < 0).sum())
        assert 0 < finished < len(c["rows"]), finished
        check_all("finisher", "tile_staged", ref, part)
    finally:
        f.workspace_bytes_override = None
        f.frame_width, f.materialize_weights = 0, True
        tensorf._WORKSPACE.clear()


# ---- the activation on chosen arguments ------------------------------------------------------------------------------------------------
def sweep_arguments():
    def ulps(v, k=4):
        out, lo, hi = [np.float32(v)], np.float32(v), np.float32(v)
        for _ in range(k):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            out += [lo, hi]
        return out
    x = list(np.arange(-120.0, 30.0 + 1e-9, 0.125, dtype=np.float64).astype(np.float32))
    for v in (20.0, -87.33, -103.3, 0.0):
        x += ulps(v)
    return np.asarray(x, np.float32)


def ulp_error(got, want64):
    """|got - want| in ulps of want (float32 spacing); below float32's smallest normal in units of that number."""
    tiny = float(np.finfo(np.float32).tiny)
    with np.errstate(over="ignore"):
        unit = np.where(np.abs(want64) >= tiny, np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64), tiny)
    return np.abs(np.asarray(got, np.float64) - want64) / unit


@pytest.mark.parametrize("act", ["softplus", "relu"])
def test_activation_sweep(act):
    """feature2density (exp_finite, log_ge1, log1p_pos of t2n_device.h) through t2n_density_at at the nodes of a 33^3 field whose only
    non-zero density entries are plane 0 / channel 0 (the 1089 arguments) and line 0 / channel 0 (1). density_shift is 0, so the argument
    feat + shift is the feature itself and every chosen float32 is reached exactly; the reference input is the device's returned feat.
    softplus: within the worst error of torch's float32 softplus on the CPU over the same inputs + 2 ulps (one exp, one log1p of at most
    1 ulp each, t2n_device.h's claim). relu: exact."""
    from text2nerf_amd import TensorVMSplit, synth
    g = 33
    aabb = [[-1.0] * 3, [1.0] * 3]
    params = synth.make_field_params(3, [g] * 3, density_scale=0.0, aabb=aabb)
    f = TensorVMSplit(torch.tensor(aabb), [g] * 3, dev(), density_n_comp=[16] * 3, appearance_n_comp=[48] * 3, app_dim=27, near_far=[0.1, 4.0],
                      shadingMode="MLP_Fea_noview", density_shift=0.0, distance_scale=25, pos_pe=0, view_pe=0, fea_pe=6, featureC=128,
                      step_ratio=1.0, fea2denseAct=act)
    node = (2.0 * np.arange(g, dtype=np.float32) / np.float32(g - 1) - 1.0).astype(np.float32)
    yy, xx = np.meshgrid(node, node, indexing="ij")
    pts = torch.from_numpy(np.stack([xx.reshape(-1), yy.reshape(-1), np.zeros(g * g, np.float32)], 1)).to(dev())
    x_all = sweep_arguments()
    worst_dev = worst_ref = 0.0
    for k in range(0, len(x_all), g * g):
        vals = np.zeros(g * g, np.float32)
        chunk = x_all[k:k + g * g]
        vals[:len(chunk)] = chunk
        for key in params:
            if key.startswith("density_"):
                params[key] = np.zeros_like(params[key])
        params["density_plane.0"][0, 0] = vals.reshape(g, g)
        params["density_line.0"][0, 0, :, 0] = 1.0
        f.load_state_dict({k2: torch.from_numpy(v) for k2, v in params.items()}, strict=True)
        feat = f.compute_densityfeature(pts).cpu().numpy()[:len(chunk)]
        sigma = f.compute_sigma(pts).cpu().numpy()[:len(chunk)]
        normal = (np.abs(chunk) >= np.finfo(np.float32).tiny) | (chunk == 0)      # (a subnormal entry may come back as 0)
        assert np.array_equal(feat[normal], chunk[normal]), "a node does not return its own plane entry"
        if act == "relu":
            assert np.array_equal(sigma, np.maximum(feat, np.float32(0.0)))
            continue
        x64 = torch.from_numpy(feat.astype(np.float64))
        want = torch.nn.functional.softplus(x64).numpy()
        ref32 = torch.nn.functional.softplus(torch.from_numpy(feat)).numpy()
        e_dev, e_ref = ulp_error(sigma, want), ulp_error(ref32, want)
        i = int(np.argmax(e_dev))
        print(f"MARCHLIST gpu sweep arguments {k}..{k + len(chunk)}: device worst {e_dev.max():.3f} ulp at x = {feat[i]!r}, "
              f"torch float32 softplus worst {e_ref.max():.3f} ulp at x = {feat[int(np.argmax(e_ref))]!r}")
        worst_dev, worst_ref = max(worst_dev, float(e_dev.max())), max(worst_ref, float(e_ref.max()))
    if act == "softplus":
        print(f"MARCHLIST gpu sweep {len(x_all)} arguments: device {worst_dev:.3f} ulp, torch float32 softplus {worst_ref:.3f} ulp")
        assert worst_dev <= worst_ref + 2.0, (worst_dev, worst_ref)
