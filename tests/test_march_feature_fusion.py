"""Feature rows in the tile marcher's tail (t2n_march_tiles.hip, t2n_app_rows.h) and the head's slot-addressed reads (t2n_mlp_ss.hip).

A fused launch — cached density table, current feature volume, a feature row per list slot — writes the rows where it writes the list
entries and runs no feature kernel. The rows are the bits k_app_features_vol computes from the same entries and the head does the same
arithmetic per row, so a fused frame is compared BITWISE with the unfused frame of the same field and volume: rgb, depth, acc, per-ray
records, list entries, counters. Every case proves through t2n_field_feature_fusion_counts which path it ran.

In the overflowing-budget case, which rays find no room in the lists depends on the order in which the waves reserve their regions (two
UNFUSED frames differ there too), and a ray the finisher colours runs the exact-fp32 head instead of the split-f16 one. There every ray
that owns list entries in both frames (ray_app.x >= 0) is still compared bitwise; only the rays finished in one of the two frames are
held to tests/test_list_budget.py's 5e-6. Depth and counts are bitwise for all of them, and the rows of every slot below the clamped
counts, voided ones included, are checked against k_app_features_vol."""
import ctypes as C

import pytest
import torch

from text2nerf_amd import _lib, synth, tensorf
from tests.conftest import TINY
from tests.helpers.march_lists import counters_now, frame_lists, list_shape
from tests.test_density_cache import AABB, NEAR_FAR, camera_rays
from tests.test_hip_parity import dev, make_field

GRIDS = {"9x13x17": [9, 13, 17], "16x16x16": [16, 16, 16]}      # tests/test_app_volume_gpu.py's
N = 32      # samples per ray: 8 x list_cap <= 32 rows per ray + 1024 for both frame sizes, so the worst-case carve holds a row per slot


# ---- the host-side sizing rule (no GPU) -------------------------------------------------------------------------------------------
def test_sizing_rule_row_per_slot():
    lib = _lib.load()
    for R in (64, 384):                                   # the tiny frames of the GPU cases: fusable at N, the larger one not at 40
        s = list_shape(R, N)
        assert s["fusable"] and s["feat_rows"] >= 8 * s["list_cap"] and s["feat_rows"] % 128 == 0, s
    assert not list_shape(384, 40)["fusable"]
    # worst-case lists of a C2 frame never get a row per slot (42 GB): 32 rows per ray
    c2 = list_shape(640000, 518)
    assert not c2["fusable"] and c2["feat_rows"] <= 640000 * 32 + 1024 + 127 and 8 * c2["list_cap"] * 128 > 40e9, c2
    # budgeted lists always do, and pay for it: 128 B more per entry than half a row per slot
    for b in (2, 14, 22, 63):
        s = list_shape(640000, 518, b)
        assert s["fusable"] and 8 * s["list_cap"] <= s["feat_rows"] < 8 * s["list_cap"] + 128, (b, s)
    rows_14 = list_shape(640000, 518, 14)["feat_rows"] * 128
    assert 1.1e9 < rows_14 < 1.2e9, rows_14
    assert int(lib.t2n_render_workspace_bytes_budget(640000, 518, 22)) < int(lib.t2n_render_workspace_bytes(640000, 518)) // 3
    # a budget at or above the samples per ray is the worst case: no row per slot
    assert list_shape(384, 40, 40)["list_cap"] == list_shape(384, 40)["list_cap"] and not list_shape(384, 40, 40)["fusable"]
    out = (C.c_uint64 * 6)()
    assert lib.t2n_render_list_shape(0, 32, 0, out) != 0 and lib.t2n_render_list_shape(64, 32, -1, out) != 0


# ---- frames -------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


def new_field(seed, grid, density_scale=0.8):
    params = synth.make_field_params(seed, list(grid), density_scale=density_scale, aabb=AABB)
    f = make_field(params, list(grid), AABB, NEAR_FAR)
    f.materialize_weights = False
    f.appearance_volume_min_frames = 1          # the volume exists from the first frame
    return f


def frame(f, rays, W, fused, n=N, lists=True):
    """One frame with the switch set; asserts through the counter which path its launches took."""
    f.feature_fusion = fused
    f.frame_width = W
    c0 = f.feature_fusion_counts()
    with torch.no_grad():
        rgb, depth, _, _ = f(rays, N_samples=n)
    st = f.stats()
    c1 = f.feature_fusion_counts()
    out = {"rgb": rgb, "depth": depth, "evaluated": st["evaluated"], "appearance": st["appearance"], "f16_redo": st["f16_redo"],
           "fused": c1["fused"] - c0["fused"], "unfused": c1["unfused"] - c0["unfused"]}
    if lists:
        out.update(frame_lists(rays.shape[0], n))
        cnt = counters_now(rays.shape[0], n)
        out["counts"] = cnt[::64].clone()
        out["flag"] = int(cnt[32])
    return out


def assert_bitwise(a, b, what):
    for k in ("rgb", "depth", "acc", "ray_app", "entries"):
        if k in a:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{what}: {k} differs"
    if "counts" in a:   # (which sub-list a handed-over ray lands on depends on the order of the reservations: the sum does not)
        assert int(a["counts"].sum()) == int(b["counts"].sum()), f"{what}: list counters differ"
    for k in ("evaluated", "appearance", "f16_redo", "total", "flag"):
        if k in a:
            assert a[k] == b[k], f"{what}: {k} {a[k]} != {b[k]}"


def fused_vs_unfused(f, rays, W, what, n=N, lists=True, launches=1):
    frame(f, rays, W, False, n, lists)                    # the version's first frame: builds the volume; the second builds the table
    ref = frame(f, rays, W, False, n, lists)
    assert (ref["fused"], ref["unfused"]) == (0, launches), (what, ref["fused"], ref["unfused"])
    out = frame(f, rays, W, True, n, lists)
    assert (out["fused"], out["unfused"]) == (launches, 0), (what, out["fused"], out["unfused"])
    assert_bitwise(out, ref, what)
    assert out["f16_redo"] == 0 and ("flag" not in out or out["flag"] == 0)
    return ref, out


@gpu
@pytest.mark.parametrize("kind", ["inside", "outside"])
@pytest.mark.parametrize("HW", [(8, 8), (24, 16)])
def test_fused_frame_equals_unfused(kind, HW):
    H, W = HW
    f = new_field(41, GRIDS["9x13x17"])
    rays = torch.from_numpy(camera_rays(kind, H, W)).to(dev())
    assert list_shape(H * W, N)["fusable"]
    ref, out = fused_vs_unfused(f, rays, W, f"{kind} {H}x{W}")
    counts = out["counts"].tolist()
    print(f"{kind} {H}x{W}: {out['appearance']} appearance entries, sub-list counts {counts}")
    if kind == "inside":
        assert out["appearance"] > 0 and float(out["rgb"].min()) < 0.99
    # partial tiles (and with them the head's clamp to the sub-list's last live slot) are exercised
    assert any(c % 32 for c in counts), counts


@gpu
def test_rays_through_compact_list():
    """A dense field: rays with more appearance samples than their staging slice holds (cap = N / 4) are handed to k_compact_list, which
    fills their slots and writes their rows."""
    H, W = 24, 16
    f = new_field(42, GRIDS["16x16x16"], density_scale=0.8)
    f.rayMarch_weight_thres = 1e-6
    rays = torch.from_numpy(camera_rays("inside", H, W)).to(dev())
    ref, out = fused_vs_unfused(f, rays, W, "dense scene")
    n_app = out["ray_app"][:, 0]
    print(f"dense scene: most appearance entries of a ray {int(n_app.max())} (staging slice {N // 4}), {int((n_app > N // 4).sum())} rays handed over")
    assert int((n_app > N // 4).sum()) > 0


@gpu
@pytest.mark.parametrize("poison", ["nan", "0xff"])
def test_poisoned_workspace(poison):
    """Any slot whose row nobody wrote shows up as a difference or as a raised f16-range flag."""
    H, W = 24, 16
    f = new_field(43, GRIDS["9x13x17"])
    rays = torch.from_numpy(camera_rays("outside", H, W)).to(dev())
    nbytes = int(_lib.load().t2n_render_workspace_bytes(H * W, N))
    f.workspace_bytes_override = nbytes
    try:
        frame(f, rays, W, False)
        ref = frame(f, rays, W, False)
        ws = tensorf.workspace(dev(), nbytes)
        if poison == "nan":
            ws[: nbytes // 4 * 4].view(torch.float32).fill_(float("nan"))
        else:
            ws.fill_(255)
        out = frame(f, rays, W, True)
        assert (out["fused"], out["unfused"]) == (1, 0)
        assert_bitwise(out, ref, f"poison {poison}")
        assert out["flag"] == 0 and out["f16_redo"] == 0
    finally:
        f.workspace_bytes_override = None
        tensorf._WORKSPACE.clear()


@gpu
def test_bf16_storage_and_early_termination():
    H, W = 24, 16
    rays = torch.from_numpy(camera_rays("inside", H, W)).to(dev())
    f = new_field(44, GRIDS["16x16x16"])
    f.factor_storage = "bf16"
    fused_vs_unfused(f, rays, W, "bf16 storage")
    f.factor_storage = "fp32"
    g = new_field(45, GRIDS["16x16x16"])
    g.early_termination = 1e-4
    ref, out = fused_vs_unfused(g, rays, W, "early termination")
    plain = new_field(45, GRIDS["16x16x16"])
    full = frame(plain, rays, W, False)
    assert out["evaluated"] <= full["evaluated"]


@gpu
def test_stale_volume_and_weights_stay_unfused():
    H, W = 16, 16
    rays = torch.from_numpy(camera_rays("inside", H, W)).to(dev())
    f = new_field(46, GRIDS["16x16x16"])
    f.appearance_volume_min_frames = 3
    got = []
    for i in range(4):                                # frames 1, 2 of the version run the direct form (unfused), frame 3 builds
        got.append(frame(f, rays, W, True))
    assert [(o["fused"], o["unfused"]) for o in got] == [(0, 1), (0, 1), (1, 0), (1, 0)], [(o["fused"], o["unfused"]) for o in got]
    assert_bitwise(got[3], got[2], "volume frames")
    # the appearance tensors change: the stale volume must not be read, the next frame is unfused and follows the new tensors
    with torch.no_grad():
        f.basis_mat.weight.mul_(-1.5)
    changed = frame(f, rays, W, True)
    assert (changed["fused"], changed["unfused"]) == (0, 1)
    assert float((changed["rgb"] - got[3]["rgb"]).abs().max()) > 1e-3
    f.feature_fusion = False
    f.appearance_volume = False
    direct = frame(f, rays, W, False)
    assert torch.equal(direct["rgb"], changed["rgb"])
    f.appearance_volume = True
    # weights materialised (the --weights 1 form): the separate kernel
    g = new_field(47, GRIDS["16x16x16"])
    frame(g, rays, W, True)
    fused = frame(g, rays, W, True)
    assert (fused["fused"], fused["unfused"]) == (1, 0)
    g.materialize_weights = True
    with_w = frame(g, rays, W, True)
    assert (with_w["fused"], with_w["unfused"]) == (0, 1)
    assert float((with_w["rgb"] - fused["rgb"]).abs().max()) <= 1e-4 and float((with_w["depth"] - fused["depth"]).abs().max()) <= 2e-4


@gpu
def test_split_call():
    """A workspace that holds 192 rays' worst case: the 24 x 16 frame runs as three sub-launches of one 8-row band, each fused."""
    H, W = 24, 16
    f = new_field(48, GRIDS["9x13x17"])
    rays = torch.from_numpy(camera_rays("inside", H, W)).to(dev())
    whole = frame(f, rays, W, False)
    whole = frame(f, rays, W, False)
    f.workspace_bytes_override = int(_lib.load().t2n_render_workspace_bytes(192, N))
    try:
        assert list_shape(128, N)["fusable"]
        ref, out = fused_vs_unfused(f, rays, W, "split call", lists=False, launches=3)
        assert torch.equal(out["rgb"], whole["rgb"]) and torch.equal(out["depth"], whole["depth"])
    finally:
        f.workspace_bytes_override = None
        tensorf._WORKSPACE.clear()


def launch_state(R, n, budget=0):
    """What the last launch left in the stream's workspace: per-ray records, counter block, list entries and slot-addressed rows."""
    s = list_shape(R, n, budget)
    cap = s["list_cap"]
    ws = tensorf._WORKSPACE[tensorf._ws_key(dev())]
    up = lambda v: (v + 255) // 256 * 256
    o_ray_app = s["o_counters"] + up(8 * 64 * 4) + up(R * 4)          # carve_workspace: counters | acc | ray_app | app_pos | ...
    assert o_ray_app + up(R * 16) == s["o_pos"]
    return {"cap": cap,
            "ray_app": ws[o_ray_app:o_ray_app + R * 16].view(torch.int32).view(R, 4).clone(),
            "counters": ws[s["o_counters"]:s["o_counters"] + 8 * 64 * 4].view(torch.int32).clone(),
            "app_pos": ws[s["o_pos"]:s["o_pos"] + 8 * cap * 16].view(torch.float32).view(8, cap, 4).clone(),
            "feat": ws[s["o_feat"]:s["o_feat"] + 8 * cap * 128].view(torch.float32).view(8, cap, 32).clone()}


def assert_rows_of_slots(f, st):
    """feat[slot] of every slot below each sub-list's clamped count — filled or voided — equals bitwise the row k_app_features_vol computes
    from app_pos[slot] (t2n_field_feature_rows, dense tile -> slot mapped here). Returns (slots checked, voided slots among them)."""
    cap, app_pos, feat = st["cap"], st["app_pos"], st["feat"]
    counters = st["counters"].clone()
    counts = [min(int(c), cap) for c in counters[::64].tolist()]
    tiles = [(c + 31) // 32 for c in counts]
    rows = 32 * max(sum(tiles), 1)
    counters[32] = 0
    dense = torch.full((rows, 32), float("nan"), dtype=torch.float32, device=dev())
    _lib.check(_lib.load().t2n_field_feature_rows(f.sync_params(), _lib.ptr(app_pos), _lib.ptr(counters), cap, 1, _lib.ptr(dense), rows,
                                                  _lib.current_stream_ptr(dev())), "t2n_field_feature_rows")
    torch.cuda.synchronize()
    voided = 0
    for l, c in enumerate(counts):                       # tiles are numbered through the sub-lists
        t0 = 32 * sum(tiles[:l])
        assert torch.equal(feat[l, :c].view(torch.int32), dense[t0:t0 + c].view(torch.int32)), f"sub-list {l}: {c} rows"
        assert torch.equal(feat[l, :c, 27].view(torch.int32), app_pos[l, :c, 3].view(torch.int32))
        voided += int((app_pos[l, :c].view(torch.int32) == 0).all(-1).sum())      # void_entries: the all-zero entry
    return sum(counts), voided


@gpu
def test_overflowing_budget(tiny_params):
    """tests/test_list_budget.py's frame: a budget of 2 entries per ray where ~5 are needed. Wave regions that do not fit are voided (and
    get rows), k_compact_list loses races for list tails, sub-lists are full (the head's clamp), most rays reach the finisher.
    A ray that kept its list entries in BOTH frames (ray_app.x >= 0) is compared bitwise; only the rays whose finisher membership can
    differ (module docstring) are held to that test's 5e-6. After the poisoned launches the row of every slot below the clamped counts,
    the voided ones included, is checked against k_app_features_vol."""
    lib = _lib.load()
    f = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    f.materialize_weights = False
    f.frame_width = 256
    f.appearance_volume_min_frames = 1
    rays = torch.from_numpy(synth.frame_rays_np(256, 256, c2w=synth.look_pose(0.3, -0.1, (0.2, 0.1, -1.0)))).to(dev())
    R, Ns = rays.shape[0], f.nSamples
    assert list_shape(R, Ns, 2)["fusable"]
    f.workspace_bytes_override = int(lib.t2n_render_workspace_bytes_budget(R, Ns, 2))

    def one(fused):
        f.feature_fusion = fused
        c0 = f.feature_fusion_counts()
        with torch.no_grad():
            rgb, depth, _, _ = f(rays)
        c1 = f.feature_fusion_counts()
        return rgb, depth, f.stats(), (c1["fused"] - c0["fused"], c1["unfused"] - c0["unfused"]), launch_state(R, Ns, 2)

    try:
        one(False)
        ref = one(False)
        assert ref[3] == (0, 1) and ref[2]["list_retry"] == 1
        for poison in (None, float("nan"), 255):
            ws = tensorf.workspace(dev(), f.workspace_bytes_override)
            if poison == 255:
                ws.fill_(255)
            elif poison is not None:
                ws[: f.workspace_bytes_override // 4 * 4].view(torch.float32).fill_(poison)
            out = one(True)
            assert out[3] == (1, 0), out[3]
            assert out[2]["list_retry"] == 1 and out[2]["f16_redo"] == 0 and int(out[4]["counters"][32]) == 0
            assert torch.equal(out[1], ref[1])
            assert out[2]["appearance"] == ref[2]["appearance"] and out[2]["evaluated"] == ref[2]["evaluated"]
            # rays that own list entries in both frames: the same bits
            listed = (ref[4]["ray_app"][:, 0] >= 0) & (out[4]["ray_app"][:, 0] >= 0)
            shaded = listed & (out[4]["ray_app"][:, 1] > 0)
            assert int(shaded.sum()) > 0 and int((~listed).sum()) > 0, (int(shaded.sum()), int((~listed).sum()))
            assert torch.equal(out[0][listed].view(torch.int32), ref[0][listed].view(torch.int32)), "a ray with list entries in both frames differs"
            d = (out[0] - ref[0]).abs().max(1).values
            print(f"overflowing budget, poison {poison}: {int(shaded.sum())} rays with list entries in both frames (bitwise), "
                  f"{int((~listed).sum())} finished in one of them: max |rgb difference| = {float(d.max()):.3e}, {int((d > 0).sum())} differ")
            assert float(d.max()) <= 5e-6
            if poison is not None:
                checked, voided = assert_rows_of_slots(f, out[4])
                print(f"  rows of {checked} slots checked, {voided} of them voided")
                assert voided > 0
    finally:
        f.workspace_bytes_override = None
        tensorf._WORKSPACE.clear()


@gpu
def test_masked_field_stays_unfused():
    """A field with an alpha mask keeps the feature stage (its marcher already spills at five waves): by the counter, and the frame is the
    frame of the switch off."""
    from tests.test_density_cache import alpha_mask
    H, W = 24, 16
    f = new_field(50, GRIDS["16x16x16"])
    rays = torch.from_numpy(camera_rays("inside", H, W)).to(dev())
    fused = fused_vs_unfused(f, rays, W, "no mask")[1]
    f.alphaMask = alpha_mask()
    frame(f, rays, W, False)
    off = frame(f, rays, W, False)
    on = frame(f, rays, W, True)
    assert (on["fused"], on["unfused"]) == (0, 1), (on["fused"], on["unfused"])
    assert_bitwise(on, off, "masked field")
    assert on["appearance"] > 0 and float(on["rgb"].min()) < 0.99      # the frame still renders
    print(f"masked field: {on['appearance']} appearance entries ({fused['appearance']} without the mask), unfused by the counter")
    f.alphaMask = None


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("HW", [(8, 8), (24, 16)])
def test_rows_of_a_fused_launch(HW):
    """After one fused launch, the row of every live slot equals bitwise the row the feature kernel computes from the same entry."""
    H, W = HW
    f = new_field(49, GRIDS["9x13x17"])
    rays = torch.from_numpy(camera_rays("outside", H, W)).to(dev())
    frame(f, rays, W, True)
    out = frame(f, rays, W, True)
    assert (out["fused"], out["unfused"]) == (1, 0)
    checked, _ = assert_rows_of_slots(f, launch_state(H * W, N))
    assert checked == out["appearance"] and checked > 0
