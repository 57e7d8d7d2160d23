"""The claims tests/test_volume_components_gpu.py rests on, checked without a GPU: the reference (scipy.ndimage.label, tests/helpers/
volume_cc_ref.py) against a plain BFS labeller, its numbering, the keep rule, the tile properties the named cases are named for
(computed from volume.TILE where the library is built, from the documented default otherwise), and that the checker rejects wrong
labellings."""
import numpy as np
import pytest

from tests.helpers import volume_cc_ref as R

TILE = R.tile()
SMALL_SHAPES = [(1, 1, 1), (1, 1, 9), (5, 1, 1), (2, 2, 2), (3, 4, 5), (6, 7, 9)]


def test_tile_is_the_documented_one():
    assert TILE == R.DEFAULT_TILE
    assert TILE[2] % 64 == 0          # a wave reads 256 contiguous bytes


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
def test_reference_equals_bfs(connectivity):
    for n, shape in enumerate(SMALL_SHAPES):
        for p in (0.2, 0.35, 0.6):
            vol = R.random_volume(shape, p, 100 * n + int(p * 100))
            labels, K, counts, boxes = R.components(vol, 0.0, connectivity)
            bl, bK = R.bfs_components(R.foreground(vol), connectivity)
            assert K == bK and np.array_equal(labels, bl), (shape, p)
            assert labels.dtype == np.int32 and np.all(labels[~R.foreground(vol)] == -1)
            assert counts.sum() == R.foreground(vol).sum()
            for c in range(K):
                idx = np.argwhere(labels == c)
                assert counts[c] == len(idx)
                assert boxes[c].tolist() == idx.min(0).tolist() + idx.max(0).tolist()


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
def test_reference_numbers_by_smallest_index(connectivity):
    for seed in range(4):
        labels, K, _, _ = R.components(R.random_volume((9, 10, 21), 0.07, seed), 0.0, connectivity)
        assert K > 3 and R.numbered_by_smallest_index(labels)
    swapped = labels.copy()
    swapped[labels == 0], swapped[labels == 1] = 1, 0
    assert not R.numbered_by_smallest_index(swapped)


def test_row_link_rule_unites_every_touching_pair_of_runs_once():
    """The local stage's rule (vol_row_links, restated in the helper): for two rows of 64 voxels and a reach of 0 or 1 along the row, the
    lanes unite exactly the pairs of runs that touch, each pair once."""
    rng = np.random.default_rng(1)
    edge = [0, 1, 1 << 63, (1 << 64) - 1, 0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0x8000000000000001]
    pairs = [(a, b) for a in edge for b in edge]
    for p in (0.1, 0.3, 0.5, 0.7, 0.9):
        bits = rng.random((300, 2, 64)) < p
        pairs += [tuple(int(sum(1 << k for k in range(64) if row[k])) for row in pair) for pair in bits]
    for mine, theirs in pairs:
        for reach in (0, 1):
            want = sorted((s, s2) for s, e in R.runs(mine) for s2, e2 in R.runs(theirs) if s2 <= e + reach and e2 >= s - reach)
            assert sorted(R.row_links(mine, theirs, reach)) == want, (hex(mine), hex(theirs), reach)


def test_offsets():
    assert [len(R.offsets(c)) for c in R.CONNECTIVITIES] == [6, 18, 26]


def test_keep_rule():
    counts = np.array([5, 9, 9, 1, 9, 3], np.int32)
    assert R.keep_mask(counts).all()
    assert R.keep_mask(counts, min_voxels=5).tolist() == [True, True, True, False, True, False]
    assert R.keep_mask(counts, keep_largest=1).tolist() == [False, True, False, False, False, False]        # tie: the lower label
    assert R.keep_mask(counts, keep_largest=2).tolist() == [False, True, True, False, False, False]
    assert R.keep_mask(counts, keep_largest=4).tolist() == [True, True, True, False, True, False]
    assert R.keep_mask(counts, min_voxels=9, keep_largest=4).tolist() == [False, True, True, False, True, False]
    assert R.keep_mask(counts, min_voxels=10, keep_largest=2).tolist() == [False] * 6
    assert R.keep_mask(counts, keep_largest=99).all()
    assert R.keep_mask(np.zeros(0, np.int32), keep_largest=1).shape == (0,)


def test_filter_reference():
    vol = R.special_values((3, 5, 9))
    labels, K, counts, _ = R.components(vol, R.SPECIAL_LEVEL, 6)
    keep = R.keep_mask(counts, keep_largest=1)
    out = R.filter_volume(vol, labels, keep, fill=-7.0)
    gone = (labels >= 0) & ~keep[np.maximum(labels, 0)]
    assert gone.any() and np.all(out[gone] == np.float32(-7.0))
    assert np.array_equal(out[~gone].view(np.uint32), vol[~gone].view(np.uint32))        # NaN and -inf backgrounds keep their bits


@pytest.mark.parametrize("how", ["face", "edge", "corner"])
def test_pairs_touch_only_where_they_say(how):
    vol, a, b = R.touching_pair(TILE, how)
    assert vol.sum() == 2.0
    differ = [a[x] != b[x] for x in range(3)]
    assert sum(differ) == {"face": 1, "edge": 2, "corner": 3}[how]
    assert max(abs(a[x] - b[x]) for x in range(3)) == 1
    ta, tb = R.tile_of(a, TILE), R.tile_of(b, TILE)
    assert [ta[x] != tb[x] for x in range(3)] == differ         # the tiles share exactly a face / an edge / a corner
    for c in R.CONNECTIVITIES:
        assert R.components(vol, 0.0, c)[1] == R.PAIR_COMPONENTS[how][c]


def test_serpentine_crosses_tile_borders_again_and_again():
    vol = R.serpentine(TILE)
    fg = R.foreground(vol)
    for c in R.CONNECTIVITIES:
        assert R.components(vol, 0.0, c)[1] == 1
    pts = np.argwhere(fg)
    tiles = {R.tile_of(p, TILE) for p in pts}
    assert len(tiles) >= 12 and R.border_crossings(fg, TILE) >= 12
    assert len({t[2] for t in tiles}) == 2                      # it straddles a border along the fastest axis all the way
    # the root (the smallest linear index) lies tiles away from the voxel with the largest index, and the tube between them is longer
    first, last = pts[0], pts[-1]
    assert abs(int(last[0]) - int(first[0])) // TILE[0] + abs(int(last[1]) - int(first[1])) // TILE[1] >= 5
    assert fg.sum() > 500


def test_checkerboard_components():
    vol = R.checkerboard((2 * TILE[0] + 1, 2 * TILE[1] + 1, TILE[2] + 3))
    n = int(R.foreground(vol).sum())
    assert R.components(vol, 0.0, 6)[1] == n
    assert R.components(vol, 0.0, 18)[1] == 1 and R.components(vol, 0.0, 26)[1] == 1


def test_case_shapes_reach_every_path():
    cases = R.gpu_cases(TILE)
    assert cases["one_tile"][0].shape == TILE
    assert cases["tile_plus_one"][0].shape == tuple(t + 1 for t in TILE)
    assert cases["13x17x70"][0].shape == (13, 17, 70)
    assert not R.foreground(*cases["all_background"]).any() and R.foreground(*cases["all_foreground"]).all()
    vol, level = cases["special_values"]
    fg = R.foreground(vol, level)
    assert np.isnan(vol).any() and not fg[np.isnan(vol)].any()
    assert (vol == np.float32(level)).any() and not fg[vol == np.float32(level)].any()
    assert fg[vol == np.inf].all() and (vol == np.inf).any() and not fg[vol == -np.inf].any() and (vol == -np.inf).any()
    # the random volumes bracket the 6-connectivity percolation threshold (~0.31): scattered specks below, one giant component above
    for p, giant in ((0.1, False), (0.25, False), (0.5, True)):
        _, K, counts, _ = R.components(*cases[f"random_p{p}"], 6)
        assert (counts.max() > 0.5 * counts.sum()) == giant
    assert all(v.size <= 40 * 40 * 130 for v, _ in cases.values())


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
def test_checker_rejects_wrong_labellings(connectivity):
    vol = R.random_volume((9, 11, 70), 0.3, 5)
    labels, K, counts, boxes = R.components(vol, 0.0, connectivity)
    assert K >= 2 and R.check(vol, 0.0, connectivity, labels, K, counts, boxes) is None
    swapped = labels.copy()
    swapped[labels == 0], swapped[labels == K - 1] = K - 1, 0
    assert R.check(vol, 0.0, connectivity, swapped, K) is not None
    one = labels.copy()
    v = tuple(np.argwhere(labels >= 0)[-1])
    one[v] = (one[v] + 1) % K
    assert R.check(vol, 0.0, connectivity, one, K) is not None
    bg = labels.copy()
    bg[tuple(np.argwhere(labels < 0)[0])] = 0
    assert R.check(vol, 0.0, connectivity, bg, K) is not None
    assert R.check(vol, 0.0, connectivity, labels, K + 1) is not None
    assert R.check(vol, 0.0, connectivity, labels, K, counts + 1, boxes) is not None
    assert R.check(vol, 0.0, connectivity, labels, K, counts, boxes + 1) is not None
    assert R.check(vol, 0.0, connectivity, labels.astype(np.int64), K) is not None


def test_checker_rejects_18_for_26():
    vol = R.touching_pair(TILE, "corner")[0]
    l18, K18, c18, b18 = R.components(vol, 0.0, 18)
    assert R.check(vol, 0.0, 26, l18, K18, c18, b18) is not None
    vol = R.random_volume((9, 11, 70), 0.2, 6)
    l18, K18, c18, b18 = R.components(vol, 0.0, 18)
    assert R.check(vol, 0.0, 26, l18, K18, c18, b18) is not None


def test_python_surface_refuses_before_any_launch():
    """ValueError for what the library would refuse, raised before the device is asked for (this test has none)."""
    from text2nerf_amd import volume
    ok = np.zeros((2, 3, 4), np.float32)
    for bad in (np.zeros((3, 4), np.float32), np.zeros((2, 3, 4), np.float64), np.zeros((2, 3, 4), np.int32), np.zeros((0, 3, 4), np.float32)):
        with pytest.raises(ValueError):
            volume.volume_components(bad)
        with pytest.raises(ValueError):
            volume.filter_volume(bad)
    for conn in (4, 8, 27, "26", None):
        with pytest.raises(ValueError):
            volume.volume_components(ok, connectivity=conn)
    for level in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            volume.volume_components(ok, level=level)
    with pytest.raises(ValueError):
        volume.filter_volume(ok, min_voxels=-1)
    with pytest.raises(ValueError):
        volume.filter_volume(ok, keep_largest=0)
