"""Inputs of the view-stage goldens (shared by make_golden_view_stage.py and the tests): validity maps for the filled-pixel list and
the mask expansion, the merge-input and finish inputs, and the stand-in for the one OpenCV call the excerpts make (OpenCV is not
installed where the goldens are made). Everything is rebuilt from seeds; view_stage.npz holds outputs only."""
import numpy as np

from text2nerf_amd import synth

PUSH = 2.0


def _g(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ---- the filled-pixel list (text2nerf_main.py:233-240). Square maps: the excerpt indexes myMap_filt[j, i] over range(H) x range(W) ----------
def sample_mask(name):
    """int64 0/1 maps. cap: 128 x 128 with more than 10 000 filled pixels (the cap of :238 is active); cols: 64 x 64 with empty columns,
    one full column and the first and last columns filled; one: a single filled pixel; none: the empty map."""
    if name == "cap":
        m = (_g(301).uniform(0, 1, (128, 128)) < 0.75).astype(np.int64)
    elif name == "cols":
        m = (_g(302).uniform(0, 1, (64, 64)) < 0.3).astype(np.int64)
        m[:, [1, 2, 17, 40, 41, 42, 62]] = 0
        m[:, 23] = 1
        m[:, 0] = 0
        m[[0, 5, 63], 0] = 1
        m[:, 63] = 0
        m[[0, 31, 63], 63] = 1
    elif name == "one":
        m = np.zeros((16, 16), np.int64)
        m[11, 6] = 1
    elif name == "none":
        m = np.zeros((16, 16), np.int64)
    else:
        raise KeyError(name)
    return m


SAMPLE_CASES = {"cap": 11, "cols": 12, "one": 13, "none": 14}          # name -> seed of `random`


def nonsquare_mask():
    """40 x 56 (W no multiple of 64, H no multiple of the row slices' 64-row step): checked against the restatement only."""
    m = (_g(303).uniform(0, 1, (40, 56)) < 0.5).astype(np.int64)
    m[:, [3, 55]] = 0
    m[:, 54] = 1
    return m


# ---- alignment and the merge inputs (:233-276) ------------------------------------------------------------------------------------------
MERGE_CASES = {"m0": (0, 48, False, 21), "m1": (1, 40, False, 22), "empty": (0, 40, True, 23)}   # name -> (seed, H, empty map, seed of `random`)


def merge_inputs(name):
    """(depth_rendered float64 [H,H] = the float32 render times the map, as InpaintView.depth_rendered is; myMap_filt int64; depth_est
    float64), from synth.align_inputs."""
    seed, H, empty, _ = MERGE_CASES[name]
    dr, de, mm = synth.align_inputs(seed, H)
    m = np.zeros((H, H), np.int64) if empty else (mm > 0).astype(np.int64)
    return dr * m, m, de


# ---- after the merge network (:278, :282, :285, :296) -------------------------------------------------------------------------------------
FINISH_HW = (23, 37)             # 851 pixels: four 256-thread blocks, the last one ragged


def finish_inputs():
    """(depth_merged float32 [H,W] in [-1,1] with the endpoints, img_u8 [H,W,3] holding every uint8 level, myMap_filt int64)."""
    h, w = FINISH_HW
    g = _g(304)
    dm = g.uniform(-1, 1, (h, w)).astype(np.float32)
    dm.reshape(-1)[:4] = np.float32([-1.0, 1.0, 0.0, -0.0])
    img = g.permutation(np.resize(np.arange(256, dtype=np.uint8), h * w * 3)).reshape(h, w, 3)
    m = (g.uniform(0, 1, (h, w)) < 0.6).astype(np.int64)
    return dm, img, m


# ---- the mask expansion (:147-162) ------------------------------------------------------------------------------------------------------
def expand_mask(name):
    """int64 0/1 maps. border: 37 x 53, known pixels touching all four borders and corners, with 1-pixel holes (on the border, one and two
    pixels inside it, and in the interior); seams: 48 x 48 with edges straddling rows / columns 15|16 and 31|32, the
    seams of the 16 x 16 tiles; ones / zeros: 20 x 20."""
    if name == "border":
        m = np.ones((37, 53), np.int64)
        m[12:20, 20:31] = 0
        for y, x in [(0, 7), (36, 40), (9, 0), (25, 52), (1, 30), (35, 12), (18, 1), (20, 51), (2, 2), (30, 30), (4, 45)]:
            m[y, x] = 0
    elif name == "seams":
        m = np.zeros((48, 48), np.int64)
        m[3:16, 2:32] = 1            # bottom edge on the 15|16 row seam, right edge on the 31|32 column seam
        m[16:45, 16:47] = 1          # top edge on the 15|16 row seam, left edge on the 15|16 column seam
        m[32:48, 0:16] = 1           # top edge on the 31|32 row seam, right edge on the 15|16 column seam, touching two borders
        m[38, 30] = 0
    elif name == "ones":
        m = np.ones((20, 20), np.int64)
    elif name == "zeros":
        m = np.zeros((20, 20), np.int64)
    else:
        raise KeyError(name)
    return m


EXPAND_CASES = ("border", "seams", "ones", "zeros")
PACK_HW = (48, 48)


def pack_inputs():
    """Inputs of the executed :147-177 (update_known_views=True) at 48 x 48: (filled warp float32 [H,W,3] in [0,1], its map int64, the
    renderer's rgb [H*W,3] float32 with values below 0 and above 1, its depth [H*W] float32)."""
    h, w = PACK_HW
    warp, _ = synth.rgbd_frame(41, h, w)
    rgb, depth = synth.rgbd_frame(42, h, w)
    g = _g(305)
    rgb = rgb.reshape(-1, 3).copy()
    rgb[:30] = g.uniform(-0.5, 0.0, (30, 3)).astype(np.float32)
    rgb[30:60] = g.uniform(1.0, 1.6, (30, 3)).astype(np.float32)
    m = (g.uniform(0, 1, (h, w)) < 0.97).astype(np.int64)
    m[:, 30:36] = 0
    m[20:24, :] = 0
    return warp, m, rgb, depth.reshape(-1).copy()


# ---- cv2 stand-in -----------------------------------------------------------------------------------------------------------------------
class Cv2StandIn:
    """`cv2.blur(src, (5, 5))` for a float32 [H,W] array with OpenCV's default border, BORDER_REFLECT_101 (the edge pixel is not
    repeated: numpy's pad mode 'reflect', scipy's 'mirror'): the float32 mean of the 25 taps. The excerpts threshold the result of a
    0 / 1 map at 0.99; 25 set taps give >= 0.9999 and 24 give 0.96 in float32 in any summation order, so the thresholded map does not
    depend on how OpenCV sums."""

    @staticmethod
    def blur(src, ksize):
        assert tuple(ksize) == (5, 5) and src.dtype == np.float32 and src.ndim == 2
        h, w = src.shape
        p = np.pad(src, 2, mode="reflect")
        acc = np.zeros((h, w), np.float32)
        for dy in range(5):
            for dx in range(5):
                acc = acc + p[dy:dy + h, dx:dx + w]
        return acc / np.float32(25)
