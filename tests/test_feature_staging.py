"""Feature stage of the default eval path (k_app_features_p): taps read from a per-tile texel box in LDS against taps gathered one by
one. The staged form promises the SAME feature rows bit for bit, so every case renders a frame through the tile marcher with
`feature_staging` on and off and asks for torch.equal on rgb and depth, and renders the staged form twice (bit-stable). The field is
non-cubic (41 x 23 x 35: the three planes differ in both sizes) in a non-cubic box; the camera stands outside the box, so the rays
enter through its faces, cross it and leave through the far faces: samples land in the first and the last cell of the axes (the high
tap's clamp). Geometry of the cases (SceneGen intrinsics, focal = max(H, W): the same field of view at every frame size):

  32 x 32   rays ~1 voxel apart at the box: most (tile, pair) units fit the box -> staged count > 0
  36 x 32   a width that is no multiple of the 8-pixel tile; 24 x 40: more regions than a wave has tiles in flight, tiles straddle them
  16 x 16   rays ~2 voxels apart: the 8 x 8-pixel tiles' boxes outgrow the 64 slots -> gathered count > 0
  256 x 256 with lists budgeted at 2 entries per ray over a poisoned workspace: stale slots decode to arbitrary positions; they
            must not fault and the frame must not depend on the switch
"""
import pytest
import torch

from text2nerf_amd import _lib, synth
from tests.test_hip_parity import dev, make_field

pytestmark = pytest.mark.gpu

GRID = [41, 23, 35]
AABB = [[-6.0, -3.5, -5.0], [6.3, 3.4, 5.2]]
NEAR_FAR = [0.5, 16.0]
N_SAMPLES = 96
POSE = dict(yaw=0.12, pitch=-0.05, center=(0.4, 0.2, -9.0))


@pytest.fixture(scope="module")
def params():
    return synth.make_field_params(5, GRID, density_scale=0.9, aabb=AABB)


def field(params, storage="fp32"):
    f = make_field(params, GRID, AABB, NEAR_FAR)
    f.materialize_weights = False
    f.factor_storage = storage
    return f


def frame(W, H):
    return torch.from_numpy(synth.frame_rays_np(H, W, c2w=synth.look_pose(**POSE))).to(dev())


def render(f, rays, W, staging):
    f.feature_staging = staging
    f.frame_width = W
    before = f.feature_staging_counts() if f._handle is not None else (0, 0)
    with torch.no_grad():
        rgb, depth, _, _ = f(rays, N_samples=N_SAMPLES)
    st = f.stats()
    after = f.feature_staging_counts()
    return rgb, depth, st, (after[0] - before[0], after[1] - before[1])


def on_off(f, rays, W):
    """on, on again, off: all three frames equal; returns the stats and the (staged, gathered) units of the staged and the gathered frame"""
    rgb, depth, st, c_on = render(f, rays, W, True)
    rgb2, depth2, _, c_on2 = render(f, rays, W, True)
    rgb0, depth0, st0, c_off = render(f, rays, W, False)
    print(f"frame width {W}: {rays.shape[0]} rays, {st['appearance']} appearance entries, staged/gathered units on {c_on} off {c_off}")
    assert st["appearance"] == st0["appearance"] and st["list_retry"] == 0 and st0["list_retry"] == 0
    assert torch.equal(rgb, rgb2) and torch.equal(depth, depth2)
    assert torch.equal(rgb, rgb0) and torch.equal(depth, depth0)
    # (the regions of a list land in the order their waves reserve them, so the tiles that straddle two regions - and with them the
    # split between staged and gathered units - differ from frame to frame; the rows do not)
    assert c_on2[0] + c_on2[1] > 0 and c_off[0] == 0 and c_off[1] > 0      # the switch is honoured
    assert float(rgb.min()) < 0.99                                # the frame shows the field, not the background alone
    return st, c_on


def test_staged_rows_equal_gathered_rows(params):
    f = field(params)
    st, c = on_off(f, frame(32, 32), 32)
    assert st["appearance"] >= 2000        # a few thousand entries: dozens of tiles, ragged last tiles included
    assert c[0] > 0


@pytest.mark.parametrize("W,H", [(36, 32), (24, 40)])
def test_ragged_and_straddling_tiles(params, W, H):
    f = field(params)
    st, c = on_off(f, frame(W, H), W)
    assert st["appearance"] > 0 and c[0] > 0


def test_wide_rays_fall_back_to_the_gather(params):
    f = field(params)
    st, c = on_off(f, frame(16, 16), 16)
    # tiles that straddle two marcher regions are gathered at every frame size (32 x 32: just under half of the units); here the
    # rays of ONE region are ~2 voxels apart, its 5-ray groups span ~10 cells per image axis and most boxes outgrow the 64 slots
    assert st["appearance"] > 0 and c[1] > c[0]


def test_bf16_storage_keeps_the_gather(params):
    f = field(params, "bf16")
    st, c = on_off(f, frame(32, 32), 32)
    assert c[0] == 0 and c[1] > 0          # 8-byte texels: this storage mode is not staged


def test_overflowed_list_with_poisoned_slots(params):
    """tests/test_list_budget.py's forced overflow: the slots a failed reservation leaves unwritten hold whatever the scratch held. The
    feature stage runs over them (their boxes come out huge, or tiny and far away): no fault, and the live rows unchanged.

    Which rays find no room depends on the order of the reservations, so two overflowed frames are not equal pixel for pixel, staged
    or not: a ray that found room has the worst-case frame's colour bit for bit (its feature rows went through the feature stage), a
    ray finished on the device has the finisher's (exact-fp32 head on its staging slice: the feature stage has no part in it, within
    5e-6 of the other: tests/test_list_budget.py). Every overflowed frame - three gathered, six staged - is therefore held against
    the worst-case frame with every tap gathered: depth bitwise, colour within 5e-6, some rays off the worst-case colour and not all.
    A staging error below 5e-6 on a ray that found room would pass here; the cases above are the bitwise check of the rows. (A
    finished ray's colour is NOT the same from frame to frame - measured: of ~1 900 such rays of a staged frame, ~100 differ in the
    last bits from every gathered frame that finished them too - so it cannot serve as a second bitwise reference; the test prints
    the same count between gathered frames for comparison.)"""
    import os
    from text2nerf_amd import tensorf as tf
    lib = _lib.load()
    f = field(params)
    W = 256
    rays = frame(W, W)
    R = rays.shape[0]
    os.environ["T2N_NO_BUDGET"] = "1"
    try:
        tf._WORKSPACE.clear()
        ref_rgb, ref_depth, ref_st, _ = render(f, rays, W, False)      # worst-case lists, every tap gathered
    finally:
        os.environ.pop("T2N_NO_BUDGET")
    assert ref_st["list_retry"] == 0
    f.workspace_bytes_override = int(lib.t2n_render_workspace_bytes_budget(R, N_SAMPLES, 2))
    assert f.workspace_bytes_override < int(lib.t2n_render_workspace_bytes(R, N_SAMPLES))

    def poisoned(poison, staging):
        buf = tf.workspace(dev(), f.workspace_bytes_override)
        if poison == 255:
            buf.fill_(255)
        else:
            buf[: f.workspace_bytes_override // 4 * 4].view(torch.float32).fill_(poison)
        rgb, depth, st, c = render(f, rays, W, staging)
        assert st["list_retry"] == 1 and st["appearance"] == ref_st["appearance"]
        assert torch.equal(depth, ref_depth)
        assert float((rgb - ref_rgb).abs().max()) <= 5e-6
        return rgb, c

    try:
        poisons = (1e30, float("nan"), 255)
        off = [poisoned(p, False) for p in poisons]
        assert all(c[0] == 0 and c[1] > 0 for _, c in off)
        finished = [(rgb != ref_rgb).any(1) for rgb, _ in off]        # rays the gathered frames show off the worst-case colour
        assert all(0 < int(fin.sum()) < R for fin in finished)

        def unlike(rgb, changed, others):      # rays off the worst-case colour that another frame finished too, with another colour
            n = 0
            for g, fin in others:
                n += int((changed & fin & (rgb != g).any(1)).sum())
            return n

        print(f"gathered frames: {[int(x.sum()) for x in finished]} rays off the worst-case colour; frame 0 against frames 1, 2: "
              f"{unlike(off[0][0], finished[0], [(off[1][0], finished[1]), (off[2][0], finished[2])])} with another colour")
        for p in poisons:
            for rep in range(2):                                        # the staged form twice per poison
                rgb, c = poisoned(p, True)
                assert c[0] > 0
                changed = (rgb != ref_rgb).any(1)
                assert 0 < int(changed.sum()) < R
                print(f"poison {p} staged frame {rep}: units {c}, {int(changed.sum())} rays off the worst-case colour; against the "
                      f"gathered frames: {unlike(rgb, changed, [(g, fin) for (g, _), fin in zip(off, finished)])} with another colour")
    finally:
        f.workspace_bytes_override = None
        tf._WORKSPACE.clear()
