"""Staged rows in the tile marcher's tail (t2n_march_tiles.hip, t2n_app_rows.h): a fused launch with row staging on reads the corners of
its feature rows from 4 x 4 x 4 corner boxes copied to LDS, one per emitting step pair, and walks its entries in emission order.

Slots, entries and rows are the direct tail's, so every staged frame is compared BITWISE with the frame of the same field with staging
off (both fused): rgb, depth, acc, per-ray records, entries, counter sums, and the feature row of every live slot as int32, read from
the workspace ray by ray (which slot a ray gets depends on the order of the waves' reservations). Every case proves through
t2n_field_row_staging_counts which tails ran staged and which direct. The dense rows of k_app_features_vol stay the reference of record
(fused_vs_unfused, assert_rows_of_slots of tests/test_march_feature_fusion.py).

Every compared frame keeps every wave region inside its sub-list (assert_regions_fit): where regions overflow a sub-list the waves that
reserve last send their rays through k_compact_list, where they are counted a second time, and the raw counter sum depends on the order
of the reservations — in the direct tail as well.

Both factor sets of a field share one grid in this library, so the launch's guard against unequal grids cannot be reached from here:
the "not staged" case is the switch off."""
import pytest
import torch

from text2nerf_amd import _lib, synth, tensorf
from tests.conftest import TINY
from tests.test_density_cache import camera_rays
from tests.test_hip_parity import dev, make_field
from tests.test_march_feature_fusion import (GRIDS, N, assert_bitwise, assert_rows_of_slots, frame, fused_vs_unfused, launch_state, list_shape,
                                             new_field)

gpu = pytest.mark.gpu


def slot_rows_by_ray(R, n, budget=0):
    """The feature rows of the last launch's live slots, ray by ray in sample order, as int32 [entries, 32]."""
    st = launch_state(R, n, budget)
    ra = st["ray_app"]
    cnt = ra[:, 1].long()
    assert int(ra[:, 0].min()) >= 0
    start = torch.repeat_interleave(ra[:, 0].long(), cnt)
    first = torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
    idx = start + (torch.arange(int(cnt.sum()), device=ra.device) - first)
    return st["feat"].view(-1, 32)[idx].view(torch.int32).clone()


def staged_frame(f, rays, W, staging, n=N, rows=True):
    """One fused frame with the staging switch set; adds the waves' counts and (rows) the rows of the live slots."""
    f.row_staging = staging
    out = frame(f, rays, W, True, n)
    assert (out["fused"], out["unfused"]) == (1, 0), (out["fused"], out["unfused"])
    out["waves"] = f.row_staging_counts()
    if rows:
        out["rows"] = slot_rows_by_ray(rays.shape[0], n)
    return out


def poison_workspace():
    """0xff into every byte of the stream's workspace: a slot, entry or row the next launch skips shows as a difference or a raised flag."""
    tensorf._WORKSPACE[tensorf._ws_key(dev())].fill_(255)


def assert_regions_fit(out, cap, what):
    """Every wave region fitted its sub-list: no counter passed list_cap, so the raw counter sums are a function of the frame."""
    assert int(out["counts"].max()) <= cap, f"{what}: a sub-list counter passed list_cap {cap}: {out['counts'].tolist()}"


def staged_vs_direct(f, rays, W, what, n=N, poison=False):
    frame(f, rays, W, True, n)                            # the version's first frames build the volume and the table
    frame(f, rays, W, True, n)
    ref = staged_frame(f, rays, W, False, n)
    assert ref["waves"] == {"staged": 0, "direct": 0}, (what, ref["waves"])
    if poison:
        poison_workspace()
    out = staged_frame(f, rays, W, True, n)
    print(f"{what}: {out['appearance']} entries, counters {out['counts'].tolist()}, waves {out['waves']}")
    cap = list_shape(rays.shape[0], n)["list_cap"]
    assert_regions_fit(ref, cap, what)
    assert_regions_fit(out, cap, what)
    assert_bitwise(out, ref, what)
    assert out["rows"].shape == ref["rows"].shape and torch.equal(out["rows"], ref["rows"]), f"{what}: feature rows differ"
    assert out["rows"].shape[0] == out["appearance"]
    assert out["f16_redo"] == 0 and out["flag"] == 0
    print(f"{what}: {out['appearance']} entries, waves {out['waves']}")
    return ref, out


# 1. staged equals direct, bit for bit ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["outside", "axis", "inside"])
@pytest.mark.parametrize("HW", [(8, 8), (24, 16), (13, 11)])
def test_staged_frame_equals_direct(kind, HW):
    H, W = HW
    f = new_field(61, GRIDS["9x13x17"])
    if kind == "inside":
        # At the default threshold this camera's tiles hold more entries than their sub-list has slots (8 x 8: 423 for 288; 13 x 11: four
        # tiles with 943 for the 672 of the one list they share). The waves that reserve last do not fit, their rays go through
        # k_compact_list and are counted a second time, so the raw counter sum depends on which waves came first — in the direct tail as
        # well. At 0.05 (18 / 94 / 40 entries) every region fits and the sums are a function of the frame.
        f.rayMarch_weight_thres = 5e-2
    rays = torch.from_numpy(camera_rays(kind, H, W)).to(dev())
    assert list_shape(H * W, N)["fusable"]
    ref, out = staged_vs_direct(f, rays, W, f"{kind} {H}x{W}")
    assert out["appearance"] > 0
    if kind == "inside":      # focal 1.2 max(H, W): a tile spans many voxels, its emitting pairs leave the table path
        assert out["waves"]["direct"] > 0, out["waves"]
    else:                     # a tile stays within four taps
        assert out["waves"]["staged"] > 0, out["waves"]


# 2. staged equals unfused: the dense rows of k_app_features_vol stay the reference -------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["outside", "axis"])
def test_staged_frame_equals_unfused(kind):
    H, W = 24, 16
    f = new_field(62, GRIDS["16x16x16"])
    f.row_staging = True
    rays = torch.from_numpy(camera_rays(kind, H, W)).to(dev())
    ref, out = fused_vs_unfused(f, rays, W, f"staged vs unfused, {kind}")
    waves = f.row_staging_counts()
    assert waves["staged"] > 0, waves
    checked, _ = assert_rows_of_slots(f, launch_state(H * W, N))
    assert checked == out["appearance"] and checked > 0


# 3. log overflow and mixed waves ---------------------------------------------------------------------------------------------------------
@gpu
def test_log_overflow_turns_a_wave_direct(tiny_params):
    """The log holds 32 step pairs: a wave overflows it when its lanes together emit on more than 32 pairs. A ray with more than 64
    entries is sufficient for that (not necessary: several rays, or rays later handed over, can fill the log too). A fused launch that
    long needs budgeted lists (worst-case lists hold a row per slot up to ~42 samples per ray only), i.e. a frame of 65 536 rays that
    averages fewer than ~38 entries per ray. The tiny field sampled at a fifth of its step from outside the box (163 samples across it,
    staging slices of 512 entries at N = 2048) does that: ~18 entries per ray, the longest ~74. Every tile that holds such a ray must
    run the direct tail: the count of direct waves is at least the count of those tiles. Every region fits its sub-list (no counter
    passes list_cap, no ray is handed over), the workspace is poisoned before the staged frame, and the frame is the frame of staging
    off."""
    from text2nerf_amd import TensorVMSplit
    n = 2048
    f = TensorVMSplit(torch.tensor(TINY["aabb"], dtype=torch.float32), list(TINY["grid"]), dev(), density_n_comp=[16] * 3,
                      appearance_n_comp=[48] * 3, app_dim=27, near_far=TINY["near_far"], shadingMode="MLP_Fea_noview", alphaMask_thres=1e-4,
                      density_shift=-10, distance_scale=25, pos_pe=0, view_pe=0, fea_pe=6, featureC=128, step_ratio=0.2,
                      fea2denseAct="softplus")                      # tests/test_hip_parity.py's make_field at a fifth of the step
    f.load_state_dict({k: torch.from_numpy(v) for k, v in tiny_params.items()}, strict=True)
    f.materialize_weights = False
    f.appearance_volume_min_frames = 1
    W = 256
    rays = torch.from_numpy(synth.frame_rays_np(256, W, c2w=synth.look_pose(1.2, -0.1, (-12.0, 0.1, -1.0)))).to(dev())
    R = rays.shape[0]
    budget = 38                                            # (the largest budget whose carve is smaller than the unfusable ones above 63)
    assert list_shape(R, n, budget)["fusable"]
    f.workspace_bytes_override = int(_lib.load().t2n_render_workspace_bytes_budget(R, n, budget))
    f.frame_width = W

    def one(staging, warm=False):
        f.row_staging = staging
        c0 = f.feature_fusion_counts()
        with torch.no_grad():
            rgb, depth, _, _ = f(rays, N_samples=n)
        st = f.stats()
        c1 = f.feature_fusion_counts()
        if warm:                                           # the version's first frames build the volume and the table
            return None
        assert (c1["fused"] - c0["fused"], c1["unfused"] - c0["unfused"]) == (1, 0)
        waves = f.row_staging_counts()
        ls = launch_state(R, n, budget)
        print(f"thin field, staging {staging}: {st['appearance']} entries ({st['appearance'] / R:.1f} per ray), most of a ray "
              f"{int(ls['ray_app'][:, 1].max())}, waves {waves}, list retries {st['list_retry']}, counters {ls['counters'][::64].tolist()} "
              f"of {ls['cap']}")
        assert st["list_retry"] == 0 and int(ls["counters"][35]) == 0, "the budget must hold the frame"
        return {"rgb": rgb, "depth": depth, "evaluated": st["evaluated"], "appearance": st["appearance"], "f16_redo": st["f16_redo"],
                "counts": ls["counters"][::64].clone(), "flag": int(ls["counters"][32]), "waves": waves, "state": ls}

    try:
        one(True, warm=True)
        one(True, warm=True)
        ref = one(False)
        poison_workspace()
        out = one(True)
        assert ref["waves"] == {"staged": 0, "direct": 0}
        for o in (ref, out):
            assert_regions_fit(o, o["state"]["cap"], "log overflow")
            assert int(o["state"]["ray_app"][:, 0].min()) >= 0
        n_app = out["state"]["ray_app"][:, 1]
        assert int(n_app.max()) <= n // 4, "no ray is handed over: every entry is the marcher's"
        long_tiles = int((n_app.view(32, 8, 32, 8) > 64).any(3).any(1).sum())     # 8 x 8 tiles that hold a ray with more than 64 entries
        print(f"thin field: {long_tiles} tiles hold a ray with more than 64 entries, waves {out['waves']}")
        assert long_tiles > 0, "a ray must emit on more step pairs than the log holds"
        assert out["waves"]["direct"] >= long_tiles and out["waves"]["staged"] > 0, (long_tiles, out["waves"])
        assert int(n_app.sum()) == int(ref["state"]["ray_app"][:, 1].sum()) == out["appearance"]
        assert_bitwise(out, ref, "log overflow")
        assert out["flag"] == 0 and out["f16_redo"] == 0
        checked, _ = assert_rows_of_slots(f, out["state"])
        assert checked > 0
    finally:
        f.workspace_bytes_override = None
        tensorf._WORKSPACE.clear()


# 4. hand-over and voids ------------------------------------------------------------------------------------------------------------------
@gpu
def test_staged_rays_through_compact_list():
    """Rays with more entries than a staging slice holds (N / 4) are handed to k_compact_list. They are logged for their first N / 4
    entries like any other ray, so the staged walk must mask them out. First tests/test_march_feature_fusion.py's dense scene with
    staging on, against the unfused frame. Then the orthographic camera, where EVERY wave with rows runs staged (direct = 0) and a good
    part of their rays is handed over, with the workspace poisoned before the staged frame: an entry or row the walk wrote for a
    handed-over ray, or one it dropped from its neighbours, differs from the frame of staging off."""
    H, W = 24, 16
    f = new_field(42, GRIDS["16x16x16"], density_scale=0.8)
    f.rayMarch_weight_thres = 1e-6
    f.row_staging = True
    rays = torch.from_numpy(camera_rays("inside", H, W)).to(dev())
    ref, out = fused_vs_unfused(f, rays, W, "dense scene, staged")
    assert int((out["ray_app"][:, 0] > N // 4).sum()) > 0
    g = new_field(61, GRIDS["9x13x17"])
    rays = torch.from_numpy(camera_rays("axis", H, W)).to(dev())
    ref, out = staged_vs_direct(g, rays, W, "axis, hand-over", poison=True)
    n_app = out["ray_app"][:, 0]
    handed, kept = int((n_app > N // 4).sum()), int(((n_app > 0) & (n_app <= N // 4)).sum())
    print(f"axis, hand-over: {handed} rays handed over, {kept} rays kept by their waves, waves {out['waves']}")
    t = n_app.view(H // 8, 8, W // 8, 8)
    mixed = int(((t > N // 4).any(3).any(1) & ((t > 0) & (t <= N // 4)).any(3).any(1)).sum())      # tiles that hold both kinds of ray
    assert handed > 0 and kept > 0 and mixed > 0, (handed, kept, mixed)
    assert out["waves"]["staged"] >= mixed and out["waves"]["direct"] == 0, (mixed, out["waves"])
    checked, _ = assert_rows_of_slots(g, launch_state(H * W, N))
    assert checked == out["appearance"]


@gpu
def test_staged_overflowing_budget(tiny_params):
    """tests/test_march_feature_fusion.py's overflowing budget with staging on: voided regions get their rows from the direct form, rays
    that fit nowhere reach the finisher. Its comparison rules: bitwise where both frames own list entries, 5e-6 for rays finished in one
    of them; the row of every slot below the clamped counts against k_app_features_vol."""
    lib = _lib.load()
    f = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    f.materialize_weights = False
    f.frame_width = 256
    f.appearance_volume_min_frames = 1
    rays = torch.from_numpy(synth.frame_rays_np(256, 256, c2w=synth.look_pose(0.3, -0.1, (0.2, 0.1, -1.0)))).to(dev())
    R, Ns = rays.shape[0], f.nSamples
    f.workspace_bytes_override = int(lib.t2n_render_workspace_bytes_budget(R, Ns, 2))

    def one(fused, staging):
        f.feature_fusion = fused
        f.row_staging = staging
        with torch.no_grad():
            rgb, depth, _, _ = f(rays)
        return rgb, depth, f.stats(), f.row_staging_counts(), launch_state(R, Ns, 2)

    try:
        one(False, True)
        ref = one(False, True)
        assert ref[3] == {"staged": 0, "direct": 0} and ref[2]["list_retry"] == 1
        for poison in (float("nan"), 255):
            ws = tensorf.workspace(dev(), f.workspace_bytes_override)
            if poison == 255:
                ws.fill_(255)
            else:
                ws[: f.workspace_bytes_override // 4 * 4].view(torch.float32).fill_(poison)
            out = one(True, True)
            assert out[3]["staged"] > 0 and out[3]["direct"] > 0, out[3]
            assert out[2]["list_retry"] == 1 and out[2]["f16_redo"] == 0 and int(out[4]["counters"][32]) == 0
            assert torch.equal(out[1], ref[1])
            assert out[2]["appearance"] == ref[2]["appearance"] and out[2]["evaluated"] == ref[2]["evaluated"]
            listed = (ref[4]["ray_app"][:, 0] >= 0) & (out[4]["ray_app"][:, 0] >= 0)
            assert int(listed.sum()) > 0 and int((~listed).sum()) > 0
            assert torch.equal(out[0][listed].view(torch.int32), ref[0][listed].view(torch.int32)), "a ray with list entries in both frames differs"
            d = (out[0] - ref[0]).abs().max(1).values
            assert float(d.max()) <= 5e-6
            checked, voided = assert_rows_of_slots(f, out[4])
            print(f"overflowing budget, staged, poison {poison}: waves {out[3]}, rows of {checked} slots checked, {voided} voided")
            assert voided > 0
    finally:
        f.workspace_bytes_override = None
        tensorf._WORKSPACE.clear()


# 5. poisoned workspace -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("poison", ["nan", "0xff"])
def test_staged_poisoned_workspace(poison):
    """A slot whose row the staged tail skipped shows as a difference or as a raised range flag."""
    H, W = 24, 16
    f = new_field(64, GRIDS["9x13x17"])
    rays = torch.from_numpy(camera_rays("outside", H, W)).to(dev())
    nbytes = int(_lib.load().t2n_render_workspace_bytes(H * W, N))
    f.workspace_bytes_override = nbytes
    try:
        frame(f, rays, W, True)
        frame(f, rays, W, True)
        ref = staged_frame(f, rays, W, False)
        ws = tensorf.workspace(dev(), nbytes)
        if poison == "nan":
            ws[: nbytes // 4 * 4].view(torch.float32).fill_(float("nan"))
        else:
            ws.fill_(255)
        out = staged_frame(f, rays, W, True)
        assert out["waves"]["staged"] > 0, out["waves"]
        assert_bitwise(out, ref, f"poison {poison}")
        assert torch.equal(out["rows"], ref["rows"])
        assert out["flag"] == 0 and out["f16_redo"] == 0
    finally:
        f.workspace_bytes_override = None
        tensorf._WORKSPACE.clear()


# 6. staging off --------------------------------------------------------------------------------------------------------------------------
@gpu
def test_staging_off_counts_nothing():
    H, W = 24, 16
    f = new_field(65, GRIDS["16x16x16"])
    rays = torch.from_numpy(camera_rays("outside", H, W)).to(dev())
    frame(f, rays, W, True)
    frame(f, rays, W, True)
    on = staged_frame(f, rays, W, True)
    off = staged_frame(f, rays, W, False)
    assert on["waves"]["staged"] > 0 and off["waves"] == {"staged": 0, "direct": 0}, (on["waves"], off["waves"])
    assert_bitwise(off, on, "staging off")
    assert torch.equal(off["rows"], on["rows"])
    f.feature_fusion = False                               # an unfused launch writes no rows in its tail: nothing to count
    f.row_staging = True
    unfused = frame(f, rays, W, False)
    assert f.row_staging_counts() == {"staged": 0, "direct": 0}
    assert_bitwise(unfused, on, "unfused")


# 7. RELU activation and bf16 factor storage -------------------------------------------------------------------------------------------------
@gpu
def test_relu_and_bf16_storage():
    H, W = 24, 16
    rays = torch.from_numpy(camera_rays("outside", H, W)).to(dev())
    f = new_field(66, GRIDS["16x16x16"])
    f.fea2denseAct = "relu"
    ref, out = staged_vs_direct(f, rays, W, "relu")
    assert out["waves"]["staged"] > 0 and out["appearance"] > 0
    g = new_field(67, GRIDS["16x16x16"])
    g.factor_storage = "bf16"
    try:
        ref, out = staged_vs_direct(g, rays, W, "bf16 storage")
        assert out["waves"]["staged"] > 0 and out["appearance"] > 0
    finally:
        g.factor_storage = "fp32"
