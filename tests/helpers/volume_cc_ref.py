"""Host reference of the volume component stage (text2nerf_amd.volume.volume_components / filter_volume, TensorBase.prune_floaters)
over `scipy.ndimage.label` with `generate_binary_structure(3, 1 | 2 | 3)`: the labels (scipy numbers components in the order of their
smallest linear index, which tests/test_volume_components_cpu.py checks; minus one, so that background is -1), counts, boxes, the keep
rule and the filter; a plain BFS labeller that shares nothing with scipy; the checker the GPU tests use; and the named test volumes with
the tile properties they are named for. Nothing here runs on the device."""
import collections
import itertools

import numpy as np
from scipy import ndimage

f32 = np.float32
DEFAULT_TILE = (4, 8, 64)            # the tile csrc/t2n_volume.hip documents; the tests take volume.TILE where the library is built
CONNECTIVITIES = (6, 18, 26)
RANK = {6: 1, 18: 2, 26: 3}          # generate_binary_structure's second argument = how many coordinates may differ


def tile():
    """volume.TILE (read from the library where it is built, the documented default otherwise)."""
    from text2nerf_amd import volume
    return tuple(volume.TILE)


def foreground(volume, level=0.0):
    with np.errstate(invalid="ignore"):
        return np.asarray(volume) > f32(level)       # strict: NaN is background


def components(volume, level=0.0, connectivity=26):
    """(labels [n0,n1,n2] int32, K, voxel_counts [K] int32, boxes [K,6] int32): scipy's labels - 1."""
    fg = foreground(volume, level)
    lab, K = ndimage.label(fg, structure=ndimage.generate_binary_structure(3, RANK[connectivity]))
    labels = lab.astype(np.int32) - 1
    counts = np.bincount(labels[fg], minlength=K).astype(np.int32)
    boxes = np.zeros((K, 6), np.int32)
    for c, sl in enumerate(ndimage.find_objects(lab)):
        boxes[c] = [s.start for s in sl] + [s.stop - 1 for s in sl]
    return labels, int(K), counts, boxes


def offsets(connectivity):
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(x != 0 for x in o) <= RANK[connectivity]]


def bfs_components(fg, connectivity):
    """Labels by breadth-first search from every unlabelled foreground voxel in linear order: -1 on background, components numbered in
    the order of their smallest linear index by construction. For small volumes."""
    fg = np.asarray(fg, bool)
    labels = np.full(fg.shape, -1, np.int32)
    offs = offsets(connectivity)
    K = 0
    for seed in zip(*np.nonzero(fg)):            # np.nonzero walks in C order
        if labels[seed] >= 0:
            continue
        labels[seed] = K
        todo = collections.deque([seed])
        while todo:
            p = todo.popleft()
            for o in offs:
                q = (p[0] + o[0], p[1] + o[1], p[2] + o[2])
                if all(0 <= q[a] < fg.shape[a] for a in range(3)) and fg[q] and labels[q] < 0:
                    labels[q] = K
                    todo.append(q)
        K += 1
    return labels, K


def numbered_by_smallest_index(labels):
    """True iff the labels are dense 0 .. K-1 and the first occurrence of label c in linear order comes before that of c + 1."""
    flat = np.asarray(labels).reshape(-1)
    fgl = flat[flat >= 0]
    if fgl.size == 0:
        return True
    vals, first = np.unique(fgl, return_index=True)
    return bool(np.array_equal(vals, np.arange(len(vals))) and np.all(np.diff(first) > 0))


def keep_mask(voxel_counts, min_voxels=0, keep_largest=None):
    """Component c stays iff voxel_counts[c] >= min_voxels and, with keep_largest = k, c is among the k components with the most voxels;
    ties go to the lower label."""
    vc = np.asarray(voxel_counts, dtype=np.int64)
    keep = vc >= min_voxels
    if keep_largest is not None:
        order = np.argsort(-vc, kind="stable")
        top = np.zeros(len(vc), bool)
        top[order[:keep_largest]] = True
        keep &= top
    return keep


def filter_volume(volume, labels, keep, fill=0.0):
    """out = keep[label] ? volume : fill on foreground (label >= 0), volume on background; bits preserved where nothing is filled."""
    out = np.array(volume, dtype=f32, copy=True)
    labels = np.asarray(labels)
    keep = np.asarray(keep, bool)
    fgm = labels >= 0
    drop = np.zeros(labels.shape, bool)
    drop[fgm] = ~keep[labels[fgm]]
    out[drop] = f32(fill)
    return out


def check(volume, level, connectivity, labels, K, counts=None, boxes=None):
    """None when (labels, K, counts, boxes) are exactly the reference's for this volume, else a sentence saying what differs."""
    rl, rK, rc, rb = components(volume, level, connectivity)
    labels = np.asarray(labels)
    if labels.shape != rl.shape or labels.dtype != np.int32:
        return f"labels of shape {labels.shape} and dtype {labels.dtype}, the reference has {rl.shape} int32"
    if int(K) != rK:
        return f"K = {K}, the reference has {rK}"
    if not np.array_equal(labels, rl):
        bad = np.argwhere(labels != rl)
        return f"{len(bad)} labels differ, the first at {tuple(bad[0])}: {labels[tuple(bad[0])]} against {rl[tuple(bad[0])]}"
    if counts is not None and not np.array_equal(np.asarray(counts), rc):
        return "voxel counts differ"
    if boxes is not None and not np.array_equal(np.asarray(boxes), rb):
        return "boxes differ"
    return None


# ---- the local stage's rule for uniting the runs of two rows (csrc/t2n_volume.hip, vol_row_links), restated on Python ints ----------
def _bit(m, j):
    return 0 <= j < 64 and (m >> j) & 1 == 1


def run_start(m, j):
    below = ~m & ((1 << j) - 1)
    return below.bit_length() if below else 0


def runs(m):
    """[(first, last)] of the runs of set bits of a 64-bit mask."""
    out, k = [], 0
    while k < 64:
        if _bit(m, k):
            s = k
            while _bit(m, k):
                k += 1
            out.append((s, k - 1))
        else:
            k += 1
    return out


def row_links(mine, theirs, reach):
    """The (run start in this row, run start in the other row) pairs the 64 lanes unite, as a list (a pair united twice shows twice)."""
    out = []
    for k in range(64):
        if not _bit(mine, k) or not theirs:
            continue
        s = run_start(mine, k)
        if reach == 0:
            if _bit(theirs, k) and (k == s or not _bit(theirs, k - 1)):
                out.append((s, run_start(theirs, k)))
            continue
        if _bit(theirs, k + 1) and not _bit(theirs, k):
            out.append((s, k + 1))
        if k == s:
            if _bit(theirs, k - 1):
                out.append((s, run_start(theirs, k - 1)))
            elif _bit(theirs, k):
                out.append((s, k))
    return out


# ---- the named test volumes -----------------------------------------------------------------------------------------------------
def _zeros(shape):
    return np.zeros(shape, f32)


def checkerboard(shape):
    i, j, k = np.indices(shape)
    return ((i + j + k) % 2 == 0).astype(f32)


def touching_pair(tile3, how):
    """Two foreground voxels in a volume of 2 x 2 x 2 tiles that touch only across a tile face ("face": they differ on axis 2 alone),
    a tile edge ("edge": on axes 1 and 2) or a tile corner ("corner": on all three), each pair straddling the tile borders it names.
    Returns (volume, a, b)."""
    t0, t1, t2 = tile3
    vol = _zeros((2 * t0, 2 * t1, 2 * t2))
    a = (t0 - 1, t1 - 1, t2 - 1)
    b = {"face": (t0 - 1, t1 - 1, t2), "edge": (t0 - 1, t1, t2), "corner": (t0, t1, t2)}[how]
    vol[a] = 1.0
    vol[b] = 1.0
    return vol, a, b


PAIR_COMPONENTS = {"face": {6: 1, 18: 1, 26: 1}, "edge": {6: 2, 18: 1, 26: 1}, "corner": {6: 2, 18: 2, 26: 1}}


def tile_of(p, tile3):
    return tuple(int(p[a]) // tile3[a] for a in range(3))


def serpentine(tile3):
    """The serpentine tube of tests/helpers/cc_ref.py laid so that its long runs go along axis 0 (the axis with the shortest tile) and
    its rows step along axis 1: one component at every connectivity that crosses tile borders again and again, a union chain whose
    root (its smallest voxel) lies far from its tail. Foreground = volume > 0."""
    from tests.helpers import cc_ref
    t0, t1, t2 = tile3
    shape = (6 * t0 + 3, 4 * t1 + 1, t2 + 9)
    rows = [4.0 + 6.0 * r for r in range((shape[1] - 8) // 6 + 1)]
    return cc_ref.serpentine_volume(shape, rows, z=float(t2) - 0.5, radius=1.6)


def border_crossings(fg, tile3):
    """How many pairs of face-adjacent foreground voxels lie in different tiles."""
    fg = np.asarray(fg, bool)
    n = 0
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        idx = np.arange(fg.shape[a] - 1)
        crosses = (idx // tile3[a]) != ((idx + 1) // tile3[a])
        both = fg[tuple(lo)] & fg[tuple(hi)]
        shape = [1, 1, 1]
        shape[a] = -1
        n += int((both & crosses.reshape(shape)).sum())
    return n


def random_volume(shape, p, seed):
    """Uniform noise shifted so that volume > 0 with probability p."""
    rng = np.random.default_rng(seed)
    return (f32(p) - rng.random(shape, dtype=f32)).astype(f32)


def special_values(shape, seed=3):
    """Values equal to the level, NaN and both infinities sprinkled over noise; for level = 0.25."""
    rng = np.random.default_rng(seed)
    vol = rng.random(shape, dtype=f32)
    pick = rng.integers(0, 6, size=shape)
    vol[pick == 0] = f32(0.25)           # equal to the level: background
    vol[pick == 1] = f32(np.nan)         # background
    vol[pick == 2] = f32(np.inf)         # foreground
    vol[pick == 3] = f32(-np.inf)        # background
    return vol


SPECIAL_LEVEL = 0.25


def gpu_cases(tile3):
    """name -> (volume, level): every case of tests/test_volume_components_gpu.py; small enough for a few seconds each."""
    t0, t1, t2 = tile3
    N = 2 * t2 + 7
    cases = {
        "1x1x1_fg": (np.ones((1, 1, 1), f32), 0.0),
        "1x1x1_bg": (_zeros((1, 1, 1)), 0.0),
        "1x1xN": (random_volume((1, 1, N), 0.6, 11), 0.0),
        "Nx1x1": (random_volume((N, 1, 1), 0.6, 12), 0.0),
        "2x2x2": (random_volume((2, 2, 2), 0.5, 13), 0.0),
        "one_tile": (random_volume((t0, t1, t2), 0.3, 14), 0.0),
        "tile_plus_one": (random_volume((t0 + 1, t1 + 1, t2 + 1), 0.3, 15), 0.0),
        "13x17x70": (random_volume((13, 17, 70), 0.3, 16), 0.0),
        "all_background": (_zeros((t0 + 1, t1 + 2, t2 + 3)) - f32(1.0), 0.0),
        "all_foreground": (np.ones((t0 + 1, t1 + 2, t2 + 3), f32), 0.0),
        "special_values": (special_values((2 * t0 + 1, t1 + 3, t2 + 5)), SPECIAL_LEVEL),
        "checkerboard": (checkerboard((2 * t0 + 1, 2 * t1 + 1, t2 + 3)), 0.0),
        "serpentine": (serpentine(tile3), 0.0),
    }
    for how in ("face", "edge", "corner"):
        cases["pair_" + how] = (touching_pair(tile3, how)[0], 0.0)
    for p in (0.1, 0.25, 0.31, 0.5):
        cases[f"random_p{p}"] = (random_volume((40, 40, 130), p, int(p * 100)), 0.0)
    return cases
