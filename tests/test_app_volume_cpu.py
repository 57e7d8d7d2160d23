"""The identity behind the cached appearance feature volume, in float64 numpy (no GPU): the features a sample gets from blending its
plane and line taps pair by pair equal the trilinear interpolation of the per-corner feature volume, to float64 rounding."""
import numpy as np
import pytest

from tests.helpers import app_volume_ref as R


@pytest.mark.parametrize("grid,C,n_feat", [([9, 13, 17], 48, 27), ([16, 16, 16], 48, 27), ([5, 4, 6], 8, 3)])
def test_direct_form_equals_interpolated_corner_volume(grid, C, n_feat):
    planes, lines, basis = R.random_factors(grid, C, n_feat, seed=sum(grid))
    pts = R.test_points(grid, 200, seed=7)
    direct = R.direct_features(planes, lines, basis, grid, pts)
    F = R.corner_volume(planes, lines, basis, grid)
    vol = R.volume_features(F, grid, pts)
    scale = np.abs(direct).max()
    assert scale > 0.1
    # 3 C products of O(1) factors per feature, each side a few float64 roundings per term
    assert np.abs(direct - vol).max() <= 64 * 3 * C * np.finfo(np.float64).eps * scale


def test_corner_positions_return_the_corner():
    grid = [9, 13, 17]
    planes, lines, basis = R.random_factors(grid, 48, 27, seed=1)
    F = R.corner_volume(planes, lines, basis, grid)
    idx = np.asarray([[0, 0, 0], [8, 12, 16], [3, 12, 5], [8, 0, 16]])
    pts = (idx / (np.asarray(grid) - 1.0) * 2.0 - 1.0).astype(np.float32)       # (exactly representable ends; inner corners to fp32)
    got = R.volume_features(F, grid, pts[[0, 1]])
    assert np.array_equal(got, F[idx[[0, 1], 2], idx[[0, 1], 1], idx[[0, 1], 0]])
    near = R.volume_features(F, grid, pts)
    assert np.abs(near - F[idx[:, 2], idx[:, 1], idx[:, 0]]).max() <= 1e-5 * np.abs(F).max()
