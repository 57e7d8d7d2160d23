"""The device SSIM without a GPU: (1) the numpy restatement the GPU tests lean on (tests/helpers/ssim_ref.py) reproduces the reference's
own `rgb_ssim` maps (tests/golden/ssim.npz); (2) `text2nerf_amd.metrics.rgb_ssim` keeps the reference's signature; (3) the fixture can
tell the float32 instantiation from the float64 one at the GPU tests' tolerance; (4) argument errors are raised before any device is
touched."""
import inspect
import json
import os
import sys

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.helpers import ssim_ref as R
from text2nerf_amd import metrics

sys.path.insert(0, GOLDEN)
from make_golden_ssim_cases import SIZES, cases, inputs  # noqa: E402

CASES = cases()


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "ssim.npz"), allow_pickle=False))


def test_fixture_covers_the_sizes_dtypes_ranges_and_filters():
    pairs = [c for c in CASES if c[1] == "pair"]
    assert {(c[2], c[3]) for c in pairs} == set(SIZES)
    for H, W in SIZES:
        mine = [c for c in pairs if (c[2], c[3]) == (H, W)]
        assert {c[4] for c in mine} == {"float32", "float64"} and {c[5] for c in mine} == {1, 255}
    assert {(c[6], c[7]) for c in pairs} == {(11, 1.5), (8, 1.0), (5, 0.8)}
    assert {c[1] for c in CASES} == {"pair", "flat_same", "flat_diff"}


def test_restatement_matches_the_reference_golden(gold):
    """1e-12 absolute on the map and the mean (two float64 summation orders of the same terms; 1.8e-13 at the worst when written)."""
    worst = 0.0
    for case in CASES:
        name, kind, H, W, dt, mv, fs, sigma, seed = case
        a, b = inputs(case)
        assert a.dtype == np.dtype(dt)
        m = R.ssim_map(a, b, mv, filter_size=fs, filter_sigma=sigma)
        want = gold[name + "/map"]
        assert m.shape == want.shape == (H - fs + 1, W - fs + 1, 3) and m.dtype == np.float64, name
        err = float(np.abs(m - want).max())
        worst = max(worst, err)
        assert err <= 1e-12, (name, err)
        assert abs(R.ssim(a, b, mv, filter_size=fs, filter_sigma=sigma) - float(gold[name + "/ssim"])) <= 1e-12, name
    print("worst |helper - golden|", worst)
    assert float(gold["flat_same_float32/ssim"]) == 1.0 and float(gold["flat_same_float64/ssim"]) == 1.0
    assert np.array_equal(R.taps(8, 1.0), metrics.gaussian_taps(8, 1.0)) and np.array_equal(R.taps(11, 1.5), metrics.gaussian_taps(11, 1.5))


def test_signature_matches_the_reference():
    ref = json.load(open(os.path.join(GOLDEN, "metrics_signatures.json")))
    for name, want in ref.items():
        got = [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(getattr(metrics, name)).parameters.values()]
        assert got == want, name


def test_golden_float32_and_float64_maps_differ_beyond_the_gpu_tolerance(gold):
    """The two cases of a pair hold the same pixel values and differ only in the dtype of the products a*a, b*b, a*b: their reference
    maps are more than 1e-9 apart somewhere (1.9e-8 to 2.5e-7 when written), two orders above the 1e-11 the GPU tests
    allow, so a kernel that forms the products in the wrong dtype fails them."""
    seen = 0
    for case in CASES:
        name, kind, H, W, dt, mv, fs, sigma, seed = case
        if kind != "pair" or dt != "float32":
            continue
        a32, b32 = inputs(case)
        other = name.replace("float32", "float64")
        a64, b64 = inputs(next(c for c in CASES if c[0] == other))
        assert np.array_equal(a32.astype(np.float64), a64) and np.array_equal(b32.astype(np.float64), b64)
        gap = float(np.abs(gold[name + "/map"] - gold[other + "/map"]).max())
        print(name, "float32 vs float64 map gap", gap)
        assert gap > 1e-9, (name, gap)
        seen += 1
    assert seen == len([c for c in CASES if c[1] == "pair"]) // 2


def test_argument_errors_come_before_the_device_check():
    a = np.zeros((12, 29, 3), np.float32)
    with pytest.raises(ValueError):
        metrics.rgb_ssim(a[..., 0], a[..., 0], 1)                       # not [H,W,3]
    with pytest.raises(ValueError):
        metrics.rgb_ssim(a[..., :2], a[..., :2], 1)
    with pytest.raises(ValueError):
        metrics.rgb_ssim(a, a[:11], 1)                                  # shapes differ
    with pytest.raises(ValueError):
        metrics.rgb_ssim(a[:10], a[:10], 1)                             # H < filter_size: scipy raises there too
    for fs in (0, 34):
        with pytest.raises(ValueError):
            metrics.rgb_ssim(np.zeros((40, 40, 3)), np.zeros((40, 40, 3)), 1, filter_size=fs)
    with pytest.raises(ValueError):
        metrics.ssim_views(a, a)                                        # not a stack
    with pytest.raises(ValueError):
        metrics.score_views(a[None, :10], a[None, :10])
    assert metrics._TILE == 16
