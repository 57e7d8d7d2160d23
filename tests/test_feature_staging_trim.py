"""Feature stage (k_app_features_p<false>) with one loop per form: a wave's main loop runs the staged form only and sets the tiles it
cannot stage aside in a per-wave queue, which a second loop drains with the gathered form when it is full and at the end. Same rows bit
for bit, so every case asks for torch.equal on rgb and depth between staging on, on again and off: there is no tolerance anywhere.
Geometry, pose and sample count are those of tests/test_feature_staging.py (field 41 x 23 x 35 in the non-cubic box, 96 samples).

Frames (regions per 8 x 8-pixel tile, groups of 32 entries; counted with the C oracle on the CPU):

  frame     groups   ragged   units by staging loads per chunk (1 / 2 / 3 / 4)   units not fitting
  32 x 32     112      12       4 /  36 /  85 /  69                                142
  48 x 48     258      28      26 / 137 / 221 / 164                                226
  64 x 64     449      41      47 / 268 / 432 / 270                                330

so all four load counts of the staging and both forms run in each of them, and nearly all groups touch a border cell of some axis
(the high tap's clamp). A tile with one pair that does not fit is gathered whole (three gathered units).

Queue overflow. The queue's capacity and the grid's size are run-time values of the launch (t2n_field_set_feature_stage_shape; the
defaults are 16 tiles and up to 512 workgroups, with which no wave of these small frames sees more than one tile). The overflow case
renders 64 x 64 with ONE workgroup (8 waves) and a capacity of 2: at least 330 / 3 = 110 tiles hold a pair that does not fit, 8 waves
share them, so some wave sets aside at least 14 > 2 tiles and drains a full queue several times. The test checks that premise on the
counters of the frame it rendered (gathered units / 3 > 8 x capacity) before it compares the frames.
"""
import pytest
import torch

from tests.test_feature_staging import field, frame, on_off, params, render  # noqa: F401  (params: the module's fixture)

pytestmark = pytest.mark.gpu


def whole_tiles(c):
    """per-tile fallback: both counters move in steps of one tile = three (tile, pair) units"""
    return c[0] % 3 == 0 and c[1] % 3 == 0


@pytest.mark.parametrize("W,H", [(32, 32), (48, 48), (64, 64)])
def test_both_forms_side_by_side(params, W, H):
    f = field(params)
    st, c = on_off(f, frame(W, H), W)
    print(f"{W} x {H}: staged / gathered units {c}")
    assert c[0] > 0 and c[1] > 0 and whole_tiles(c)            # staged tiles next to deferred ones
    assert c[0] + c[1] >= 3 * ((st["appearance"] + 31) // 32)   # every tile counted once, in one form or the other


def test_ragged_width_and_many_regions(params):
    f = field(params)
    st, c = on_off(f, frame(40, 36), 40)
    assert st["appearance"] > 0 and c[0] > 0 and whole_tiles(c)


def test_full_queue_is_drained_and_refilled(params):
    W = 64
    rays = frame(W, W)
    f = field(params)
    rgb_ref, depth_ref, _, c_ref = render(f, rays, W, True)     # default launch shape
    cap, waves = 2, 8
    f.feature_stage_shape = (1, cap)
    try:
        rgb, depth, st, c = render(f, rays, W, True)
        rgb2, depth2, _, c2 = render(f, rays, W, True)
        rgb0, depth0, _, c0 = render(f, rays, W, False)
    finally:
        f.feature_stage_shape = (0, 0)
    print(f"one workgroup, capacity {cap}: units on {c} / {c2}, off {c0}; default shape {c_ref}")
    for cc in (c, c2):
        assert whole_tiles(cc) and cc[0] > 0
        assert cc[1] // 3 > waves * cap        # pigeonhole: some wave set aside more tiles than its queue holds
    assert c0[0] == 0 and c0[1] // 3 > waves * cap
    # every tile once, in one form or the other: the frame's tile count is what the gathered-only frame counted, and the
    # default-shape frame, where no wave has two tiles and no queue ever fills, counted the same
    tiles3 = c0[1]
    assert c_ref[0] + c_ref[1] == tiles3 and c[0] + c[1] == tiles3 and c2[0] + c2[1] == tiles3
    for a, b in ((rgb, depth), (rgb2, depth2), (rgb0, depth0)):
        assert torch.equal(a, rgb_ref) and torch.equal(b, depth_ref)


def test_three_staged_frames_are_one_frame(params):
    W = 48
    rays = frame(W, W)
    f = field(params)
    frames = [render(f, rays, W, True) for _ in range(3)]
    assert all(c[0] > 0 for _, _, _, c in frames)
    for rgb, depth, _, _ in frames[1:]:
        assert torch.equal(rgb, frames[0][0]) and torch.equal(depth, frames[0][1])


def test_staging_off_defers_every_tile(params):
    W = 48
    rays = frame(W, W)
    f = field(params)
    rgb, depth, st, c_on = render(f, rays, W, True)
    rgb0, depth0, st0, c_off = render(f, rays, W, False)
    assert c_off[0] == 0 and whole_tiles(c_off)
    assert c_off[1] >= 3 * ((st0["appearance"] + 31) // 32)     # every tile of every list went through the queue
    assert c_on[0] > 0 and st["appearance"] == st0["appearance"]
    assert torch.equal(rgb, rgb0) and torch.equal(depth, depth0)
