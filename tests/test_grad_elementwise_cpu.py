"""The element-wise factor-gradient check without a kernel: the helper's invariants, that the cases of tests/helpers/grad_cases.py reach
the bin edges their table claims (computed from the oracle's sample positions and the constants read out of csrc/t2n_backward.h / .hip),
and mutation tests that show what the checker catches — on the float32 oracle's gradients, so nothing here needs a GPU.

The last mutation is the gap the element-wise check closes, stated as a test: zeroing every element below 2e-4 of its tensor's largest
gradient passes the whole-tensor `_grad_check(rel=2e-4)` and fails `check`."""
import numpy as np
import pytest

from tests.helpers import grad_cases as GC
from tests.helpers import grad_elementwise as GE
from tests.test_hip_parity import _grad_check

ALL = list(GC.CASES)
PAIRS = [(n, "fuzz") for n in ALL] + [(n, "driver") for n in ALL if GC.CASES[n].is_train]


@pytest.fixture(scope="module")
def consts():
    return GC.kernel_constants()


@pytest.mark.parametrize("name,loss", PAIRS)
def test_helper_invariants(name, loss):
    ref = GC.reference(name, loss)
    assert np.isfinite(ref.rho32) and ref.rho32 > 0, ref.rho32
    print(f"{name} / {loss} loss: rho32 {ref.rho32:.3f} " + " ".join(f"{k} {v:.3f}" for k, v in ref.rho32_kind.items())
          + f"; samples {int(ref.valid.sum())}, appearance {int(ref.app_mask.sum())}, on the threshold's knife edge {int(ref.app_window.sum())}")
    untouched_plane = 0
    for k in GE.FACTOR_KEYS:
        A, g = ref.A[k], ref.g64[k]
        assert np.all(A * (1 + 1e-12) >= np.abs(g)), k            # (two float64 summation orders)
        assert np.all(g[A == 0] == 0) and np.all(ref.g32[k][A == 0] == 0), k
        assert np.all(np.isfinite(ref.bound[k])) and np.all(ref.bound[k][ref.touched[k]] > 0), k
        if "plane" in k:
            untouched_plane += int((~ref.touched[k]).sum())
    assert untouched_plane > 0, "no element for the stray-write check to bite on"
    assert 0 < int(ref.app_window.sum()) < 0.01 * int(ref.app_mask.sum())      # the knife edge exists and stays a handful of samples
    GE.check(ref.g32, ref, K=2 * max(1.0, ref.rho32))


def _cells(ref, mask, grid):
    xn = ref.xn[mask]
    return np.stack([GC.axis_cell(xn[:, a], grid[a]) for a in range(3)], 1)


@pytest.mark.parametrize("name", ALL)
def test_cases_reach_what_the_table_claims(name, consts):
    kBlk, kTile, kDenSeg, seg_min = consts["kBlk"], consts["kBinTile"], consts["kDenSeg"], consts["T2N_ACC_SEG_MIN"]
    assert (kBlk, kTile) == (15, 16), "the cases' grid sizes aim at 15-cell blocks and 16-texel tiles: choose them anew"
    b, ref = GC.built(name), GC.reference(name, "fuzz")
    grid, case = b["grid"], b["case"]
    nb = [(s + kBlk) // kBlk for s in grid]          # block_geom / bin_geom: cell + 1 in [0, size]
    nt = [(s + kTile) // kTile for s in grid]
    want = {"caseA": ([2, 2, 2], [1, 1, 1]), "caseB": ([2, 3, 3], [2, 2, 2]), "evalB": ([2, 3, 3], [2, 2, 2]), "caseC": ([2, 3, 4], [2, 3, 3]),
            "caseD": ([2, 2, 29], [2, 2, 28]), "caseE": ([2, 2, 30], [2, 2, 28])}[name]
    assert (nb, nt) == want
    den, app = _cells(ref, ref.valid, grid), _cells(ref, ref.app_mask, grid)
    # samples with a normalised coordinate of exactly -1 / +1 on every axis and side (cell -1 never occurs inside the box: xn >= -1)
    xn = ref.xn[ref.valid]
    for a in range(3):
        assert int((xn[:, a] == -1).sum()) > 0 and int((xn[:, a] == 1).sum()) > 0, (name, a)
        assert den[:, a].min() == 0 and den[:, a].max() == grid[a] - 1
        # every block and every tile along every axis holds samples, the last of each the high face (cell == size - 1) among them
        blocks, tiles = (den[:, a] + 1) // kBlk, (app[:, a] + 1) // kTile
        assert sorted(set(blocks.tolist())) == list(range(nb[a])), (name, a)
        assert sorted(set(tiles.tolist())) == list(range(nt[a])), (name, a)
        if grid[a] % kBlk == 0:       # the last block holds the face only
            assert set(den[blocks == nb[a] - 1, a].tolist()) == {grid[a] - 1}
        if grid[a] % kTile == 0:      # the last tile holds one cell only
            assert set(app[tiles == nt[a] - 1, a].tolist()) == {grid[a] - 1}
    _, per_block = np.unique((den + 1) // kBlk, axis=0, return_counts=True)
    if name == "caseA":
        assert per_block.max() > kDenSeg, per_block.max()                 # one block cut into >= 2 segments
        assert int(ref.app_mask.sum()) >= 4 * seg_min                        # one tile per plane: several segments of >= seg_min records
        assert case.n_rays > 4 * consts["kBinCopies"]                        # all privatised counter copies
    if name in ("caseB", "evalB"):
        assert grid[0] == kTile and grid[1] == 2 * kBlk and set(den[(den[:, 0] + 1) // kBlk == 1, 0].tolist()) == {14, 15}
    if name == "caseC":
        assert grid[0] % kBlk == 14 and grid[1] == 2 * kTile and grid[2] == 3 * kBlk
    if name in ("caseD", "caseE"):
        # binned_scatter_ok: tile_accum_lds(., 16) <= 160 KiB; the 8-channel half-group form (80 KiB) has the same limit
        lds16, lds8 = GC.tile_accum_lds(grid, consts, 16), GC.tile_accum_lds(grid, consts, 8, 256)
        assert (lds16 <= 160 * 1024) == (name == "caseD") and (lds8 <= 80 * 1024) == (name == "caseD"), (lds16, lds8)
        longer = [s + (1 if s == max(grid) else 0) for s in grid]
        shorter = [s - (1 if s == max(grid) else 0) for s in grid]
        other = GC.tile_accum_lds(longer if name == "caseD" else shorter, consts, 16)
        assert (other <= 160 * 1024) == (name == "caseE")                   # D and E sit on either side of the limit, one texel apart


# ---- mutations of the float32 oracle's gradient: each must be flagged at the GPU tests' K -------------------------------------------------
@pytest.fixture(scope="module")
def refB():
    return GC.reference("caseB", "fuzz")


def _mutated(ref, key, fn):
    got = {k: v.copy() for k, v in ref.g32.items()}
    got[key] = fn(got[key])
    return got


def _flagged(got, ref, key):
    lines = GE.failures(got, ref, ref.K())
    assert lines and all(l.startswith(key + ":") for l in lines), lines
    return lines


@pytest.mark.parametrize("key", ["density_plane.0", "app_plane.0", "density_line.1", "app_line.1"])
def test_mutation_block_edge_row_scaled(refB, key):
    """Texel row 14 (the last row a 15-cell block owns) scaled by 0.97."""
    def fn(g):
        g[:, :, 14] *= 0.97
        return g
    print(_flagged(_mutated(refB, key, fn), refB, key))


@pytest.mark.parametrize("key", ["density_plane.1", "app_plane.2", "density_line.0", "app_line.2"])
def test_mutation_last_row_or_column_zeroed(refB, key):
    def fn(g):
        if g.shape[-1] > 1:
            g[..., -1] = 0
        else:
            g[:, :, -1] = 0
        return g
    print(_flagged(_mutated(refB, key, fn), refB, key))


@pytest.mark.parametrize("key", ["density_plane.2", "app_plane.1"])
def test_mutation_plane_shifted_by_one_texel(refB, key):
    print(_flagged(_mutated(refB, key, lambda g: np.roll(g, 1, axis=-1)), refB, key))


@pytest.mark.parametrize("kind", ["d", "a"])
def test_mutation_one_sample_removed(refB, kind):
    """The contribution of ONE sample of typical weight (the median |upstream| of its lookup) taken out of the six tensors it reaches:
    flagged in at least one of them, and in no tensor of the other quantity."""
    up = refB.samples["up_" + kind].abs()
    up = up if up.dim() == 1 else up.amax(-1)
    index = int(np.argsort(up.numpy())[up.numel() // 2])
    c = GE.sample_contribution(GC.built("caseB")["params"], refB, kind, index)
    got = {k: refB.g32[k] - c.get(k, 0.0) for k in refB.g32}
    lines = GE.failures(got, refB, refB.K())
    prefix = "density" if kind == "d" else "app"
    assert lines and all(l.startswith(prefix + "_") for l in lines), lines
    print(lines)


def test_mutation_small_elements_zeroed_passes_the_whole_tensor_check_only(refB):
    """Every element below 2e-4 of its tensor's max |g| set to zero: invisible to max |dg| / max |g| <= 2e-4, caught element by element."""
    got, n = {}, 0
    for k, g in refB.g32.items():
        small = np.abs(refB.g64[k]) < 2e-4 * np.abs(refB.g64[k]).max()
        if k in GE.FACTOR_KEYS:
            n += int((small & (refB.A[k] > 0)).sum())
        got[k] = np.where(small & np.array(k in GE.FACTOR_KEYS), 0.0, g)
    assert n > 100
    _grad_check(got, refB.g64, rel=2e-4)
    lines = GE.failures(got, refB, refB.K())
    assert len(lines) >= 6, lines
    with pytest.raises(AssertionError, match="element-wise"):
        GE.check(got, refB, refB.K())


def test_stray_write_is_flagged(refB):
    key = next(k for k in GE.FACTOR_KEYS if "plane" in k and (~refB.touched[k]).any())
    idx = tuple(np.argwhere(~refB.touched[key])[0])

    def fn(g):
        g[idx] = 1e-30
        return g
    assert "stray write" in _flagged(_mutated(refB, key, fn), refB, key)[0]
