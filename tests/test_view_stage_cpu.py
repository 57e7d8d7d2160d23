"""The depth stage of a new view (text2nerf_main.py:147-162, :230-299), the parts that need no GPU: the equivalence the device sampling
rests on (random.sample of a list = the list indexed by random.sample of a range, generator state included), the numpy restatement
(tests/helpers/view_stage_ref.py) against the goldens made by executing the reference's lines (tests/golden/make_golden_view_stage.py),
the OpenCV stand-in those goldens were made with against scipy, and the public signatures."""
import inspect
import os
import random
import sys

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.helpers import view_stage_ref as VR

sys.path.insert(0, GOLDEN)
import make_golden_view_stage_cases as VC  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "view_stage.npz"), allow_pickle=False))


# ---- the draw ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(20000, 10000), (70000, 10000), (1076, 1076), (1, 1), (0, 0)])
def test_sampling_a_list_is_indexing_it_by_a_sample_of_its_range(n, k):
    """CPython's sample() has a pool branch (n <= setsize: 20 000 with k = 10 000) and a set branch (70 000); k = n < 10 000 and n = 0
    are the reference's `min(len(pixel_filled), 10000)` below the cap."""
    setsize = 21 + 4 ** int(np.ceil(np.log(k * 3) / np.log(4))) if k > 5 else 21
    assert (n <= setsize) == (n in (20000, 1076, 1, 0))                              # the branches the cases are there for
    items = [(i * 7919 % 1013, i) for i in range(n)]
    for seed in (0, 1, 12345):
        a, b = random.Random(seed), random.Random(seed)
        by_list = a.sample(items, k)
        by_rank = [items[r] for r in b.sample(range(n), k)]
        assert by_list == by_rank and a.getstate() == b.getstate()


# ---- the restatement against the executed excerpts --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(VC.SAMPLE_CASES))
def test_restated_pixel_list_matches_the_excerpt(gold, name):
    m = VC.sample_mask(name)
    rng = random.Random(VC.SAMPLE_CASES[name])
    got = VR.sample_filled_pixels(m, rng)
    assert got.dtype == np.int32 and np.array_equal(got, gold[f"sample_{name}"])
    assert [rng.getrandbits(32) for _ in range(4)] == gold[f"sample_{name}_next"].tolist()
    pixels = VR.filled_pixels(m)
    assert len(pixels) == int(m.sum()) and all(m[y, x] > 0 for y, x in pixels)
    assert pixels == sorted(pixels, key=lambda p: (p[1], p[0]))                      # column-major, rows ascending inside a column
    if name == "cap":
        assert len(pixels) > 10000 and len(got) == 10000
    if name == "cols":
        per_col = m.sum(0)
        assert (per_col == 0).sum() >= 5 and (per_col == 64).sum() == 1 and per_col[0] > 0 and per_col[63] > 0


def test_restated_pixel_list_on_a_non_square_map():
    m = VC.nonsquare_mask()
    assert m.shape == (40, 56)
    pixels = VR.filled_pixels(m)
    slow = [(j, i) for i in range(56) for j in range(40) if m[j, i] > 0]               # the reference's loop with its ranges put right
    assert pixels == slow and len(pixels) == int(m.sum())


@pytest.mark.parametrize("name", list(VC.MERGE_CASES))
def test_restated_merge_inputs_match_the_excerpt(gold, name):
    dr, m, _ = VC.merge_inputs(name)
    ref, src, mask = VR.merge_inputs(dr, m, gold[f"merge_{name}_depth_shift"], VC.PUSH)
    for got, key in ((ref, "depth_ref"), (src, "depth_src")):
        g = gold[f"merge_{name}_{key}"]
        assert got.dtype == g.dtype == np.float32 and np.array_equal(got.view(np.uint32), g.view(np.uint32)), key       # bits: -0.0 too
    assert np.array_equal(mask, m.astype(np.float32))
    rng = random.Random(VC.MERGE_CASES[name][3])
    assert np.array_equal(VR.sample_filled_pixels(m, rng), gold[f"merge_{name}_pixel_sample"])
    if name == "empty":
        assert gold["merge_empty_pixel_sample"].shape == (0, 2) and not m.any()
    else:
        assert np.signbit(ref[m == 0]).any()                                          # the masked-out zeros carry numpy's sign


def test_restated_finish_matches_the_excerpt(gold):
    dm, img, m = VC.finish_inputs()
    d, i, k = VR.finish(dm, img, m, VC.PUSH)
    assert np.array_equal(d.view(np.uint32), gold["finish_depth_new"].view(np.uint32))
    assert i.dtype == np.float32 and np.array_equal(i, gold["finish_img_new"]) and len(np.unique(img)) == 256
    assert k.dtype == np.int64 and np.array_equal(k, gold["finish_mask_inpainted"])


@pytest.mark.parametrize("name", VC.EXPAND_CASES)
def test_restated_erosion_matches_the_excerpt(gold, name):
    m = VC.expand_mask(name)
    eroded, mask_ex = VR.erode5(m)
    assert eroded.dtype == mask_ex.dtype == np.int64
    assert np.array_equal(eroded, gold[f"expand_{name}_eroded"]) and np.array_equal(mask_ex, gold[f"expand_{name}_mask_ex"])
    if name == "border":
        assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any() and m[0, 0] and m[0, -1] and m[-1, 0] and m[-1, -1]
        zero = np.ones_like(m)                                                        # the border rule decides: with zeros outside the
        p = np.pad(m, 2, mode="constant")                                             # image no pixel of the outer two rings survives
        for dy in range(5):
            for dx in range(5):
                zero &= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
        assert eroded[0].any() and eroded[-1].any() and eroded[:, 0].any() and eroded[:, -1].any() and not np.array_equal(zero, eroded)
    if name == "ones":
        assert eroded.all() and not mask_ex.any()
    if name == "zeros":
        assert not eroded.any() and not mask_ex.any()


def test_restated_pack_with_expansion_matches_the_excerpt(gold):
    warp, m, rgb, depth = VC.pack_inputs()
    got = VR.pack_expanded(warp, m, rgb, depth)
    for k, v in got.items():
        g = gold[f"pack_{k}"]
        assert v.shape == g.shape and np.array_equal(v, g), k
    assert got["depth_rendered"].dtype == np.float64 and 0 < got["myMap_filt"].sum() < m.sum()


# ---- the OpenCV stand-in ----------------------------------------------------------------------------------------------------------------
def test_cv2_stand_in_is_a_reflect_101_box_mean():
    from scipy.ndimage import uniform_filter
    g = np.random.Generator(np.random.PCG64(7))
    for shape, p in (((37, 53), 0.9), ((48, 48), 0.97), ((20, 31), 0.5)):
        m = (g.uniform(0, 1, shape) < p).astype(np.float32)
        mine = VC.Cv2StandIn.blur(m, (5, 5))
        ref = uniform_filter(m.astype(np.float64), size=5, mode="mirror")
        assert mine.dtype == np.float32
        assert np.abs(mine.astype(np.float64) - ref).max() <= np.spacing(np.float32(1.0))          # 1 ulp at the top of the range
        assert np.array_equal(mine > 0.99, ref > 0.99)
        assert np.array_equal((mine > 0.99) * 1, VR.erode5(m.astype(np.int64))[0])


# ---- the public surface -----------------------------------------------------------------------------------------------------------------
def test_public_signatures():
    from text2nerf_amd import warp
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]         # noqa: E731
    E = inspect.Parameter.empty
    assert sig(warp.sample_filled_pixels) == [("myMap_filt", E), ("max_samples", 10000), ("rng", random), ("device", None)]
    assert sig(warp.prepare_depth_merge) == [("depth_rendered", E), ("myMap_filt", E), ("depth_est", E), ("push_depth", E), ("rng", random),
                                             ("max_samples", 10000), ("device", None)]
    assert sig(warp.finish_view) == [("depth_merged", E), ("img_u8", E), ("myMap_filt", E), ("push_depth", E), ("poses_support", E),
                                     ("intrinsic", E), ("H", E), ("W", E), ("train_set", None), ("device", None)]
    assert warp.DepthMerge._fields == ("scale", "shift", "pixel_sample", "depth_shift", "depth_ref", "depth_src", "mask")
    assert warp.FinishedView._fields == ("img_new", "depth_new", "mask_inpainted", "support", "lo", "hi")
    for f in (warp.build_inpaint_view, warp.pack_inpaint_inputs):
        p = inspect.signature(f).parameters["update_known_views"]
        assert p.default is False
    before = ["tensorf", "poses", "N_iter", "H", "W", "intrinsic", "N_samples", "white_bg", "ndc_ray", "rays", "known_rgbs", "known_depths",
              "use_filter_filling", "device"]
    assert list(inspect.signature(warp.build_inpaint_view).parameters)[:len(before)] == before      # the earlier arguments keep their places
    assert "pixel_sample" in inspect.signature(warp.align_depth_global).parameters

