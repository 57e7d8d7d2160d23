"""The cached appearance feature volume (t2n_app_volume.hip): k_app_volume_build + the second form of the feature stage,
k_app_features_vol, against the direct form (k_app_features_p) and the float64 reference (tests/helpers/app_volume_ref.py).

Rows: the feature stage alone on hand-made lists (t2n_field_feature_rows), volume against direct: weight and zero columns bit-equal,
features within four times the direct form's own largest error against float64 (the volume form adds one interpolation's roundings to
the same products). Frames: volume on (min_frames = 1) against off — everything the marcher makes is equal, rgb within the suite's
1e-4. Staleness, trigger and cap: by the counters."""
import ctypes as C

import numpy as np
import pytest
import torch

from text2nerf_amd import _lib, synth, tensorf
from tests.helpers import app_volume_ref as R
from tests.test_density_cache import AABB, N, NEAR_FAR, camera_rays, frame_lists
from tests.test_hip_parity import RGB_ATOL, dev, make_field

pytestmark = pytest.mark.gpu

GRIDS = {"9x13x17": [9, 13, 17], "16x16x16": [16, 16, 16]}
COUNTS = [0, 1, 31, 32, 33, 97, 5, 64]      # entries of the eight sub-lists
LIST_CAP = 128


def new_field(seed, grid):
    params = synth.make_field_params(seed, list(grid), density_scale=0.8, aabb=AABB)
    f = make_field(params, list(grid), AABB, NEAR_FAR)
    f.materialize_weights = False
    return params, f


def feature_rows(f, pos, counts, volume):
    lib = _lib.load()
    h = f.sync_params()
    tiles = [(n + 31) // 32 for n in counts]
    rows = 32 * sum(tiles)
    app_pos = torch.zeros((8, LIST_CAP, 4), dtype=torch.float32, device=dev())
    counters = torch.zeros(8 * 64, dtype=torch.int32, device=dev())
    index, o = [], 0
    for l, n in enumerate(counts):
        app_pos[l, :n] = pos[o:o + n]
        counters[64 * l] = n
        index += [32 * sum(tiles[:l]) + i for i in range(n)]
        o += n
    feat = torch.full((rows, 32), float("nan"), dtype=torch.float32, device=dev())
    _lib.check(lib.t2n_field_feature_rows(h, _lib.ptr(app_pos), _lib.ptr(counters), LIST_CAP, 1 if volume else 0, _lib.ptr(feat), rows,
                                          _lib.current_stream_ptr(dev())), "t2n_field_feature_rows")
    torch.cuda.synchronize()
    assert int(counters[32]) == 0          # the f16-range flag stayed down
    return feat.cpu(), torch.tensor(index)


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("grid_key", list(GRIDS))
def test_rows_volume_against_direct(grid_key, storage):
    grid = GRIDS[grid_key]
    params, f = new_field(31, grid)
    f.factor_storage = storage
    total = sum(COUNTS)
    pts = R.test_points(grid, 80, seed=3)
    assert pts.shape[0] >= total
    pts = pts[np.random.Generator(np.random.PCG64(1)).permutation(pts.shape[0])[:total]]
    w = np.linspace(0.01, 0.9, total, dtype=np.float32)
    pos = torch.from_numpy(np.concatenate([pts, w[:, None]], 1)).to(dev())
    direct, index = feature_rows(f, pos, COUNTS, False)
    c0 = f.appearance_volume_counts()
    vol, _ = feature_rows(f, pos, COUNTS, True)
    c1 = f.appearance_volume_counts()
    assert c1["builds"] == c0["builds"] + 1 and c1["bytes"] >= (grid[0] + 1) * (grid[1] + 1) * (grid[2] + 1) * 128
    # weight column and zero columns: the same bits in every row, padded rows included
    assert torch.equal(direct[:, 27:].view(torch.int32), vol[:, 27:].view(torch.int32))
    assert torch.equal(vol[index, 27], torch.from_numpy(w)) and float(vol[:, 28:].abs().max()) == 0.0
    pad = torch.ones(vol.shape[0], dtype=torch.bool)
    pad[index] = False
    assert float(vol[pad][:, :28].abs().max()) == 0.0 if bool(pad.any()) else True       # dead entries: weight 0 on a finite corner
    state = {k: v for k, v in params.items()}
    if storage == "bf16":
        state = {k: (torch.from_numpy(v).bfloat16().float().numpy() if k.startswith("app_") else v) for k, v in state.items()}
    planes, lines, basis = R.factors_from_state(state, grid)
    ref = R.direct_features(planes, lines, basis, grid, pts)
    e_direct = float(np.abs(direct[index, :27].double().numpy() - ref).max())
    e_vol = float(np.abs(vol[index, :27].double().numpy() - ref).max())
    print(f"{grid_key} {storage}: max |direct - fp64| = {e_direct:.3e}, max |volume - fp64| = {e_vol:.3e}, scale {np.abs(ref).max():.3e}")
    assert e_direct > 0.0 and e_vol <= 4.0 * e_direct
    f.factor_storage = "fp32"


def render(f, rays, W, volume, min_frames=1):
    f.appearance_volume = volume
    f.appearance_volume_min_frames = min_frames
    f.frame_width = W
    with torch.no_grad():
        rgb, depth, _, _ = f(rays, N_samples=N)
    st = f.stats()
    out = {"rgb": rgb, "depth": depth, "evaluated": st["evaluated"], "appearance": st["appearance"]}
    out.update(frame_lists(rays.shape[0], N))
    return out


def assert_same_but_rgb(a, b, what):
    for k in ("depth", "acc", "ray_app", "entries"):
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"
    for k in ("evaluated", "appearance", "total"):
        assert a[k] == b[k], f"{what}: {k} {a[k]} != {b[k]}"
    d = float((a["rgb"] - b["rgb"]).abs().max())
    assert d <= RGB_ATOL, f"{what}: rgb differs by {d}"
    return d


@pytest.mark.parametrize("kind", ["inside", "outside"])
@pytest.mark.parametrize("HW", [(8, 8), (24, 16)])
def test_frames_volume_against_direct(kind, HW):
    H, W = HW
    _, f = new_field(32, GRIDS["9x13x17"])
    rays = torch.from_numpy(camera_rays(kind, H, W)).to(dev())
    off = render(f, rays, W, False)
    c0 = f.appearance_volume_counts()
    on = render(f, rays, W, True)
    c1 = f.appearance_volume_counts()
    assert (c1["builds"], c1["volume"]) == (c0["builds"] + 1, c0["volume"] + 1), (c0, c1)
    d = assert_same_but_rgb(on, off, f"{kind} {H}x{W}")
    if kind == "inside":
        assert off["appearance"] > 0 and float(off["rgb"].min()) < 0.99
    print(f"{kind} {H}x{W}: {off['appearance']} appearance entries, max |rgb(volume) - rgb(direct)| = {d:.3e}")


def _frame():
    return torch.from_numpy(camera_rays("inside", 16, 16)).to(dev()), 16


def _follows(f, rays, W, before, what, rebuilt=True):
    """The next volume frame follows the current parameters (= the direct frame of them), with or without a rebuild."""
    c0 = f.appearance_volume_counts()
    on = render(f, rays, W, True)
    c1 = f.appearance_volume_counts()
    assert c1["builds"] == c0["builds"] + (1 if rebuilt else 0) and c1["volume"] == c0["volume"] + 1, (what, c0, c1)
    off = render(f, rays, W, False)
    assert_same_but_rgb(on, off, what)
    if before is not None and rebuilt:
        assert float((off["rgb"] - before["rgb"]).abs().max()) > 10 * RGB_ATOL, what + ": the change did not show"
    return off


def test_stale_volume_is_never_read():
    from text2nerf_amd.optim import TVAdam
    rays, W = _frame()
    params, f = new_field(33, GRIDS["16x16x16"])
    first = _follows(f, rays, W, None, "new field")
    _follows(f, rays, W, first, "unchanged", rebuilt=False)
    # a density-only change (a writable view of a density plane leaves the library): the density table is stale, the volume is not
    p = C.c_void_p()
    _lib.check(_lib.load().t2n_field_factor_buffer(f.sync_params(), 0, C.byref(p)), "t2n_field_factor_buffer")
    _follows(f, rays, W, first, "density-only change", rebuilt=False)
    # basis_mat upload
    with torch.no_grad():
        f.basis_mat.weight.mul_(-1.5)
    basis = _follows(f, rays, W, first, "basis_mat upload")
    # one TVAdam.step: the field Adam launch rewrites the appearance planes in place
    opt = TVAdam(f.get_optparam_groups(0.05, 1e-3), betas=(0.9, 0.99), field=f)
    g = torch.Generator().manual_seed(5)
    tr = rays[torch.randperm(rays.shape[0], generator=g)[:128].to(dev())].contiguous()
    tgt = torch.rand(tr.shape[0], 3, generator=g).to(dev())
    f.frame_width = 0
    rgb, _, _, _ = f(tr, is_train=True, N_samples=N)
    opt.zero_grad()
    torch.mean((rgb - tgt) ** 2).backward()
    opt.step(tv=[(f.density_plane, 0.1), (f.app_plane, 0.01)])
    stepped = _follows(f, rays, W, basis, "factor Adam")
    # one fused train_step
    dep_t = torch.rand(tr.shape[0], generator=g).to(dev()) * 4 + 1
    f.train_step(tr, tgt, dep_t, opt, N_samples=N, white_bg=True, fused=True)
    _follows(f, rays, W, stepped, "train_step")


def test_trigger_counts_and_cap():
    from text2nerf_amd.optim import TVAdam
    rays, W = _frame()
    _, f = new_field(34, GRIDS["16x16x16"])
    assert f.appearance_volume is True and f.appearance_volume_min_frames == 0        # defaults: on, the library's frame count
    ref = render(f, rays, W, False)
    c0 = f.appearance_volume_counts()
    for i in range(1, 6):                       # (the direct frame above was the version's first tile frame: 2 more are direct)
        out = render(f, rays, W, True, min_frames=3)
        c = f.appearance_volume_counts()
        want_vol = max(0, i - 1)                # frames 2 (direct), 3.. (volume) of the version
        assert (c["volume"] - c0["volume"], c["builds"] - c0["builds"]) == (want_vol, 1 if want_vol else 0), (i, c0, c)
        assert_same_but_rgb(out, ref, f"frame {i + 1}")
        if not want_vol:
            assert torch.equal(out["rgb"], ref["rgb"])
    # an alternating step / frame loop never builds, whatever min_frames > 1
    opt = TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f)
    g = torch.Generator().manual_seed(6)
    tr = rays[:128].contiguous()
    tgt = torch.rand(tr.shape[0], 3, generator=g).to(dev())
    dep_t = torch.rand(tr.shape[0], generator=g).to(dev()) * 4 + 1
    c1 = f.appearance_volume_counts()
    for _ in range(4):
        f.train_step(tr, tgt, dep_t, opt, N_samples=N, white_bg=True, fused=True)
        render(f, rays, W, True, min_frames=2)
    c2 = f.appearance_volume_counts()
    assert c2["builds"] == c1["builds"] and c2["volume"] == c1["volume"] and c2["direct"] == c1["direct"] + 4, (c1, c2)
    # over the cap nothing is allocated; at the cap it is
    tensorf.release_workspaces(dev())
    assert f.appearance_volume_counts()["bytes"] == 0
    f.appearance_volume_cap_bytes = 16 ** 3 * 128 - 1
    for _ in range(2):
        render(f, rays, W, True, min_frames=1)
    c3 = f.appearance_volume_counts()
    assert c3["bytes"] == 0 and c3["builds"] == c2["builds"], c3
    f.appearance_volume_cap_bytes = 16 ** 3 * 128
    render(f, rays, W, True, min_frames=1)
    c4 = f.appearance_volume_counts()
    assert c4["bytes"] >= 17 ** 3 * 128 and c4["builds"] == c3["builds"] + 1, c4


def test_finisher_takes_its_features_from_the_volume(tiny_params):
    """A budget of 2 entries per ray leaves nearly every ray to k_finish_rays. In a volume frame those rays read the volume as well
    (every row of a frame comes from one form): against the worst-case volume frame depth is equal and rgb within the finisher's
    exact-vs-split head tolerance of tests/test_list_budget.py (5e-6)."""
    import os
    from tests.conftest import TINY
    lib = _lib.load()
    f = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    f.materialize_weights = False
    f.frame_width = 256
    f.appearance_volume_min_frames = 1
    rays = torch.from_numpy(synth.frame_rays_np(256, 256, c2w=synth.look_pose(0.3, -0.1, (0.2, 0.1, -1.0)))).to(dev())
    R, Ns = rays.shape[0], f.nSamples

    def full():
        with torch.no_grad():
            return f(rays)

    os.environ["T2N_NO_BUDGET"] = "1"
    try:
        tensorf._WORKSPACE.clear()
        ref = full()
        ref_st = f.stats()
    finally:
        os.environ.pop("T2N_NO_BUDGET")
    assert f.appearance_volume_counts()["volume"] == 1
    f.workspace_bytes_override = int(lib.t2n_render_workspace_bytes_budget(R, Ns, 2))
    out = full()
    st = f.stats()
    c = f.appearance_volume_counts()
    assert c["volume"] == 2 and c["builds"] == 1
    assert st["list_retry"] == 1 and st["appearance"] == ref_st["appearance"]
    assert torch.equal(out[1], ref[1])
    d = float((out[0] - ref[0]).abs().max())
    print(f"finished rays against list rays, both from the volume: max |rgb difference| = {d:.3e}")
    assert d <= 5e-6
    f.workspace_bytes_override = None
    tensorf._WORKSPACE.clear()
