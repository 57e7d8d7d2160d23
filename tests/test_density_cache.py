"""The tile marcher's cached summed density table (t2n_march_tiles.hip: k_density_sum_table, k_march_tiles<.., CACHED>).

The table S[z][y][x] = (D0 + D1) + D2 that every wave of the tile marcher rebuilds per step pair is a function of the density factors
alone. With TensorBase.density_cache (default on) the second consecutive tile-marcher frame of a factor version builds it once for
the whole grid and frames read their entries there. Everything here is an EQUALITY (torch.equal): the cached frame and the uncached
frame are the same bits — outputs, per-ray list records, list entries, sample counters — and a table entry is the same bits
whichever 4 x 4 x 4 box it was computed in. No tolerance appears in this file.

Which step pairs read the table and which gather directly is decided the same way on both paths (the two forms round differently:
tests/test_march_summed_table.py); the frames below hold both kinds."""
import numpy as np
import pytest
import torch

from text2nerf_amd import synth, tensorf
from tests.helpers.march_lists import frame_lists, list_capacity      # noqa: F401 (other test files import them from here)
from tests.test_hip_parity import dev, make_field
from tests.test_march_summed_table import pinhole_rays, step_pairs

pytestmark = pytest.mark.gpu

AABB = [[-3.0, -2.5, 1.0], [3.0, 3.5, 8.0]]     # (the eval z gate keeps samples with world z > 2)
NEAR_FAR = [0.3, 9.0]
N = 40
GRIDS = {"9x13x17": [9, 13, 17], "16x16x16": [16, 16, 16]}
FRAMES = {"16x16": (16, 16), "13x11": (13, 11), "8x8": (8, 8)}      # (H, W): whole tiles, ragged tiles, one tile


def camera_rays(kind, H, W):
    if kind == "inside":
        return pinhole_rays(H, W, 1.2 * max(H, W), synth.look_pose(0.2, -0.1, (0.3, 0.2, 2.5)))
    if kind == "outside":        # six units in front of the live part of the box, aimed at its +x edge: a third of the rays miss it
        return pinhole_rays(H, W, 80.0, synth.look_pose(0.37, 0.05, (0.5, 0.0, -4.0)))
    assert kind == "axis"        # orthographic along +z: two direction components are exactly 0; the outer rays pass beside the box
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    o = np.stack([-3.2 + 0.11 * xs, -2.7 + 0.13 * ys, np.zeros_like(xs)], -1).reshape(-1, 3)
    d = np.broadcast_to(np.asarray([0.0, 0.0, 1.0], np.float32), o.shape)
    return np.concatenate([o, d], 1).astype(np.float32)


_FIELDS = {}


def field_for(grid_key, act):
    key = (grid_key, act)
    if key not in _FIELDS:
        grid = GRIDS[grid_key]
        params = synth.make_field_params(11 + len(_FIELDS), grid, density_scale=0.8, aabb=AABB)
        from text2nerf_amd import TensorVMSplit
        m = TensorVMSplit(torch.tensor(AABB, dtype=torch.float32), list(grid), dev(), density_n_comp=[16] * 3, appearance_n_comp=[48] * 3,
                          app_dim=27, near_far=NEAR_FAR, shadingMode="MLP_Fea_noview", alphaMask_thres=1e-4, density_shift=-10,
                          distance_scale=25, pos_pe=0, view_pe=0, fea_pe=6, featureC=128, step_ratio=1.0, fea2denseAct=act)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        _FIELDS[key] = m
    return _FIELDS[key]


def alpha_mask(seed=3):
    """A coarse occupancy volume with holes: about a third of its cells are empty."""
    from text2nerf_amd.tensorf import AlphaGridMask
    rng = np.random.Generator(np.random.PCG64(seed))
    vol = (rng.random((7, 6, 5)) > 0.35).astype(np.float32)
    return AlphaGridMask(dev(), torch.tensor(AABB), torch.from_numpy(vol))


def render(f, rays, W, cache):
    f.density_cache = cache
    f.frame_width = W
    with torch.no_grad():
        rgb, depth, z, w = f(rays, N_samples=N)
    st = f.stats()
    out = {"rgb": rgb, "depth": depth, "z_vals": z, "weights": w, "evaluated": st["evaluated"], "appearance": st["appearance"]}
    out.update(frame_lists(rays.shape[0], N))
    return out


def assert_same_frame(a, b, what):
    for k in ("rgb", "depth", "acc", "ray_app", "entries", "z_vals", "weights"):
        if a[k] is None:
            assert b[k] is None, (what, k)
        else:
            assert torch.equal(a[k], b[k]), f"{what}: {k} differs"
    for k in ("evaluated", "appearance", "total"):
        assert a[k] == b[k], f"{what}: {k} {a[k]} != {b[k]}"


def cached_vs_uncached(f, rays, W, what):
    """Frames with the cache on until one is served from it (the second of a new factor version; the first when the table is
    current), then the same frame with the cache off. Returns the cached frame."""
    c0 = f.density_cache_counts()
    a = render(f, rays, W, True)
    c1 = f.density_cache_counts()
    if c1["cached"] == c0["cached"]:
        first = a
        a = render(f, rays, W, True)
        c2 = f.density_cache_counts()
        assert c2["cached"] == c1["cached"] + 1 and c2["builds"] == c1["builds"] + 1, (what, c0, c1, c2)
    else:
        first = None
    c = f.density_cache_counts()
    ref = render(f, rays, W, False)
    d = f.density_cache_counts()
    assert d["uncached"] == c["uncached"] + 1 and d["cached"] == c["cached"], (what, c, d)
    f.density_cache = True
    assert_same_frame(a, ref, what)
    if first is not None:
        assert_same_frame(first, ref, what + " (first frame of the version)")
    return a


# ---- 1. cached == uncached, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("camera", ["inside", "outside", "axis"])
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("grid_key", list(GRIDS))
def test_cached_frame_equals_uncached(grid_key, frame, camera):
    H, W = FRAMES[frame]
    rays_np = camera_rays(camera, H, W)
    rays = torch.from_numpy(rays_np).to(dev())
    if camera != "axis":
        pairs = step_pairs(rays_np, H, W, AABB, GRIDS[grid_key], NEAR_FAR, N, False)
        n_table = sum(1 for p in pairs if p[0])
        print(f"{grid_key} {frame} {camera}: {n_table} table step pairs, {len(pairs) - n_table} gathered")
        assert n_table >= 1, "no step pair of this frame reads the table"
    seen = 0
    for act in ("softplus", "relu"):
        f = field_for(grid_key, act)
        for storage in ("fp32", "bf16"):
            f.factor_storage = storage
            for mask in (None, alpha_mask()):
                f.alphaMask = mask
                for weights, eps in ((True, 0.0), (False, 0.0), (False, 1e-4)):     # weights rows; lists only; early termination on
                    f.materialize_weights, f.early_termination = weights, eps
                    a = cached_vs_uncached(f, rays, W, f"{act} {storage} mask={mask is not None} weights={weights} eps={eps}")
                    seen += a["evaluated"]
        f.factor_storage, f.alphaMask, f.materialize_weights, f.early_termination, f.frame_width = "fp32", None, True, 0.0, 0
    assert seen > 0, "no sample of any of these frames was evaluated"
    if camera != "axis":
        misses = int((a["ray_app"][:, 1] == 0).sum())
        print(f"rays without a sample: {misses} of {rays.shape[0]}")
        if camera == "outside":
            assert 0 < misses < rays.shape[0]


# ---- 2. a table entry does not depend on the box it was computed in -------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("grid_key", list(GRIDS))
def test_table_entry_is_independent_of_the_box_origin(grid_key, storage):
    """The builder runs the marcher's own table_build<2> + table_sum<2> on boxes anchored at 4 b - shift: over the shifts 0..3 of an axis
    a cell sits at every position of its box, i.e. the box is anchored at the cell and at its three neighbours down that axis. All
    64 shift triples give the same bits, and the one past-the-end entry per axis repeats the clamped texel's."""
    f = field_for(grid_key, "softplus")
    f.factor_storage = storage
    g = GRIDS[grid_key]
    ref = f.density_sum_table((0, 0, 0))
    assert tuple(ref.shape) == (g[2] + 1, g[1] + 1, g[0] + 1) and bool(torch.isfinite(ref).all())
    for sz in range(4):
        for sy in range(4):
            for sx in range(4):
                t = f.density_sum_table((sx, sy, sz))
                if not torch.equal(t, ref):
                    bad = torch.nonzero(t != ref)[0].tolist()
                    raise AssertionError(f"shift {(sx, sy, sz)}: entry z, y, x = {bad} is {float(t[tuple(bad)])!r}, at shift 0 "
                                         f"{float(ref[tuple(bad)])!r}")
    assert torch.equal(ref[-1], ref[-2]) and torch.equal(ref[:, -1], ref[:, -2]) and torch.equal(ref[:, :, -1], ref[:, :, -2])
    # the entries are the factor products they claim to be (fp64 restatement; the fp32 sum of 48 products of O(1) values)
    sd = {k: v.detach().double() for k, v in f.state_dict().items() if k.startswith("density_")}
    if storage == "bf16":
        sd = {k: v.float().bfloat16().double() for k, v in sd.items()}
    P = [sd[f"density_plane.{i}"][0] for i in range(3)]      # [C, g[mat1], g[mat0]]
    L = [sd[f"density_line.{i}"][0, :, :, 0] for i in range(3)]      # [C, g[vec]]
    want = (torch.einsum("cyx,cz->zyx", P[0], L[0]) + torch.einsum("czx,cy->zyx", P[1], L[1]) + torch.einsum("czy,cx->zyx", P[2], L[2]))
    err = float((ref[:-1, :-1, :-1].double().cpu() - want.cpu()).abs().max())
    scale = float(want.abs().max())
    print(f"{grid_key} {storage}: max |S - fp64 S| = {err:.3e} at scale {scale:.3e}")
    assert err <= 48 * 2.0 ** -23 * max(scale, 1.0) * 4      # 48 fp32 products and sums of terms below `scale`
    f.factor_storage = "fp32"


# ---- 3. invalidation --------------------------------------------------------------------------------------------------------------------
def _frame():
    H, W = 16, 16
    return torch.from_numpy(camera_rays("inside", H, W)).to(dev()), W


def _new_field(seed, grid=(16, 16, 16)):
    params = synth.make_field_params(seed, list(grid), density_scale=0.8, aabb=AABB)
    return params, make_field(params, list(grid), AABB, NEAR_FAR)


def _check_rebuild(f, rays, W, what):
    """After a change of the density factors: the next frame is uncached, the one after it is served from a rebuilt table, both equal
    the uncached render of the new parameters."""
    c0 = f.density_cache_counts()
    a = render(f, rays, W, True)
    c1 = f.density_cache_counts()
    assert (c1["cached"], c1["uncached"], c1["builds"]) == (c0["cached"], c0["uncached"] + 1, c0["builds"]), (what, c0, c1)
    b = render(f, rays, W, True)
    c2 = f.density_cache_counts()
    assert (c2["cached"], c2["uncached"], c2["builds"]) == (c1["cached"] + 1, c1["uncached"], c1["builds"] + 1), (what, c1, c2)
    ref = render(f, rays, W, False)
    f.density_cache = True
    assert_same_frame(a, ref, what + ": first frame")
    assert_same_frame(b, ref, what + ": rebuilt table")
    return ref


def test_invalidation_by_every_route():
    from text2nerf_amd.optim import TVAdam
    rays, W = _frame()
    params, f = _new_field(21)
    f.materialize_weights = False
    first = _check_rebuild(f, rays, W, "new field")
    c = f.density_cache_counts()
    again = render(f, rays, W, True)                # unchanged factors: served from the table, no build
    d = f.density_cache_counts()
    assert (d["cached"], d["builds"]) == (c["cached"] + 1, c["builds"])
    assert_same_frame(again, first, "unchanged factors")

    other = synth.make_field_params(22, [16, 16, 16], density_scale=0.8, aabb=AABB)
    f.load_state_dict({k: torch.from_numpy(v) for k, v in other.items()}, strict=True)
    loaded = _check_rebuild(f, rays, W, "load_state_dict")
    assert not torch.equal(loaded["depth"], first["depth"])

    # one TVAdam.step on the gradients of a training forward (in place on the device copies)
    opt = TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f)
    g = torch.Generator().manual_seed(5)
    tr = rays[torch.randperm(rays.shape[0], generator=g)[:128].to(dev())].contiguous()
    tgt = torch.rand(tr.shape[0], 3, generator=g).to(dev())
    f.frame_width = 0
    rgb, _, _, _ = f(tr, is_train=True, N_samples=N)
    opt.zero_grad()
    torch.mean((rgb - tgt) ** 2).backward()
    opt.step(tv=[(f.density_plane, 0.1), (f.app_plane, 0.01)])
    stepped = _check_rebuild(f, rays, W, "TVAdam.step")
    assert not torch.equal(stepped["depth"], loaded["depth"])

    # one fused train_step
    dep_t = torch.rand(tr.shape[0], generator=g).to(dev()) * 4 + 1
    f.train_step(tr, tgt, dep_t, opt, N_samples=N, white_bg=True, fused=True)
    trained = _check_rebuild(f, rays, W, "train_step")
    assert not torch.equal(trained["depth"], stepped["depth"])

    # factor_storage flip, both ways
    f.factor_storage = "bf16"
    half = _check_rebuild(f, rays, W, "factor_storage bf16")
    assert not torch.equal(half["depth"], trained["depth"])
    f.factor_storage = "fp32"
    back = _check_rebuild(f, rays, W, "factor_storage fp32")
    assert_same_frame(back, trained, "fp32 storage again")

    # grid changes: a new native field
    f.upsample_volume_grid([20, 18, 22])
    _check_rebuild(f, rays, W, "upsample_volume_grid")
    f.shrink(torch.tensor([[-2.0, -2.0, 2.0], [2.5, 3.0, 7.0]], device=dev()))
    _check_rebuild(f, rays, W, "shrink")


# ---- 4. fallbacks -------------------------------------------------------------------------------------------------------------------------
def test_cap_switch_and_release():
    rays, W = _frame()
    _, f = _new_field(23)
    f.materialize_weights = False
    ref = render(f, rays, W, False)
    cells_bytes = 16 * 16 * 16 * 4
    # cap below the grid: never cached
    f.density_cache_cap_bytes = cells_bytes - 1
    c0 = f.density_cache_counts()
    for _ in range(3):
        assert_same_frame(render(f, rays, W, True), ref, "cap below the grid")
    c1 = f.density_cache_counts()
    assert (c1["cached"], c1["uncached"], c1["builds"], c1["bytes"]) == (c0["cached"], c0["uncached"] + 3, c0["builds"], 0)
    # cap at the grid: cached
    f.density_cache_cap_bytes = cells_bytes
    assert_same_frame(render(f, rays, W, True), ref, "cap at the grid")
    c2 = f.density_cache_counts()
    assert (c2["cached"], c2["builds"]) == (c1["cached"] + 1, c1["builds"] + 1) and c2["bytes"] >= 17 ** 3 * 4
    # switch off: uncached, the table stays; on again: served at once
    for _ in range(2):
        assert_same_frame(render(f, rays, W, False), ref, "switched off")
    c3 = f.density_cache_counts()
    assert (c3["cached"], c3["uncached"], c3["builds"]) == (c2["cached"], c2["uncached"] + 2, c2["builds"])
    assert_same_frame(render(f, rays, W, True), ref, "switched on again")
    c4 = f.density_cache_counts()
    assert (c4["cached"], c4["builds"]) == (c3["cached"] + 1, c3["builds"])
    # release_workspaces frees the table; two frames later it is back
    assert c4["bytes"] > 0
    tensorf.release_workspaces(dev())
    assert f.density_cache_counts()["bytes"] == 0
    assert_same_frame(render(f, rays, W, True), ref, "after release, first frame")
    assert_same_frame(render(f, rays, W, True), ref, "after release, second frame")
    c5 = f.density_cache_counts()
    assert (c5["cached"], c5["uncached"], c5["builds"]) == (c4["cached"] + 1, c4["uncached"] + 1, c4["builds"] + 1)


# ---- the parity suites run the cached path -----------------------------------------------------------------------------------------
def test_oracle_parity_frame_is_served_from_the_table():
    """The whole-frame parity tests (tests/test_march_summed_table.py::test_index_mapping and its neighbours, with the cache at its
    default) render every frame at least twice on one field — weights rows, then lists only — so their second tile-marcher frame is a
    cached one. The same sequence here, with the counters read: the frame compared with oracle_c is served from the table. Bounds:
    that test's (RGB_ATOL / DEPTH_ATOL of tests/test_hip_parity.py)."""
    from tests.test_march_summed_table import AABB as A2, GRID, NEAR_FAR as NF2, N_SAMPLES, check_against_oracle_c, render_modes
    params = synth.make_field_params(5, GRID, density_scale=0.8, aabb=A2)
    f = make_field(params, GRID, A2, NF2)
    assert f.density_cache is True
    H, W = 37, 53
    rays_np = pinhole_rays(H, W, 4.0 * max(H, W), synth.look_pose(0.25, -0.15, (0.3, 0.2, 0.4)))
    out, _ = render_modes(f, torch.from_numpy(rays_np).to(dev()), W, N_SAMPLES)
    c = f.density_cache_counts()
    assert (c["cached"], c["uncached"], c["builds"]) == (1, 1, 1), c      # (per-ray marcher,) tile frame uncached, tile frame cached
    check_against_oracle_c(params, A2, GRID, NF2, rays_np, N_SAMPLES, out)


# ---- 5. memory --------------------------------------------------------------------------------------------------------------------------
def test_memory_of_the_table():
    """The table is (grid + 1)^3 floats in one device allocation of the field, nothing per frame. The field's buffers are not torch's:
    torch's reserved bytes must not move at all, and the device's free memory falls by less than 1.2 x the table (the driver hands out
    whole pages: 2 MiB granules)."""
    grid = (64, 64, 64)
    rays, W = _frame()
    _, f = _new_field(24, grid)
    f.materialize_weights = False
    render(f, rays, W, True)                      # first frame of the version: workspace and field buffers exist, no table
    torch.cuda.synchronize()
    assert f.density_cache_counts()["bytes"] == 0
    reserved0 = torch.cuda.memory_reserved(dev())
    free0, _ = torch.cuda.mem_get_info(dev())
    for _ in range(4):
        render(f, rays, W, True)
    torch.cuda.synchronize()
    c = f.density_cache_counts()
    table = 65 ** 3 * 4
    assert c["builds"] == 1 and table <= c["bytes"] <= table + 64       # cells x 4 B plus the padding, one allocation
    free1, _ = torch.cuda.mem_get_info(dev())
    grown = torch.cuda.memory_reserved(dev()) - reserved0
    # (the device's free memory is printed only: other processes share the device)
    print(f"table {table} B, memory_reserved grew by {grown} B, device free memory fell by {free0 - free1} B")
    assert grown < 1.2 * table
    tensorf.release_workspaces(dev())
    assert f.density_cache_counts()["bytes"] == 0
