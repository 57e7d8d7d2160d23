"""The depth stage of a new view on the CPU in plain numpy, in the project's own words: what csrc/t2n_view.hip has to compute. Pinned bit
for bit to the goldens made by executing the reference's lines (tests/golden/make_golden_view_stage.py) in tests/test_view_stage_cpu.py,
and the checker for what those lines cannot run: non-square maps, and arithmetic on arrays the device produced."""
import numpy as np


def filled_pixels(my_map):
    """The (row, col) of every pixel with my_map > 0, column by column: column ascending, inside a column row ascending."""
    cols, rows = np.nonzero(np.asarray(my_map).T > 0)
    return list(zip(rows.tolist(), cols.tolist()))


def sample_filled_pixels(my_map, rng, max_samples=10000):
    """int32 [K,2]: rng.sample of the list above, K = min(len, max_samples)."""
    pixels = filled_pixels(my_map)
    return np.asarray(rng.sample(pixels, min(len(pixels), max_samples)), np.int32).reshape(-1, 2)


def merge_inputs(depth_rendered, my_map, depth_shift, push):
    """(depth_ref, depth_src, mask), all float32. depth_rendered float64 and my_map int64: float64 arithmetic, rounded once.
    depth_shift float32: float32 operation by operation."""
    assert depth_rendered.dtype == np.float64 and depth_shift.dtype == np.float32 and my_map.dtype == np.int64
    ref = ((depth_rendered - np.float64(push)) * np.float64(12000) / np.float64(32768) - np.float64(1)) * my_map.astype(np.float64)
    p = np.float32(push)
    src = (depth_shift - p) * np.float32(12000) / np.float32(32768) - np.float32(1)
    assert src.dtype == np.float32
    return ref.astype(np.float32), src, my_map.astype(np.float32)


def finish(depth_merged, img_u8, my_map, push):
    """(depth_new float32, img_new float32, mask_inpainted int64) before the filter."""
    assert depth_merged.dtype == np.float32 and img_u8.dtype == np.uint8 and my_map.dtype == np.int64
    d = (depth_merged + np.float32(1)) * np.float32(32768)
    d = d / np.float32(12000) + np.float32(push)
    assert d.dtype == np.float32
    return d, (img_u8.astype(np.float64) / 255.0).astype(np.float32), 1 - my_map


def erode5(my_map):
    """(eroded int64 [H,W], mask_ex int64 [H,W,3]): a pixel stays 1 only when all 25 taps of its 5x5 window, reflected at the border
    without repeating the edge pixel, are 1; mask_ex is the removed ring on three channels."""
    m = (np.asarray(my_map) != 0).astype(np.int64)
    h, w = m.shape
    p = np.pad(m, 2, mode="reflect")
    out = np.ones((h, w), np.int64)
    for dy in range(5):
        for dx in range(5):
            out &= p[dy:dy + h, dx:dx + w]
    ring = m - out
    return out, np.repeat(ring[:, :, None], 3, axis=2)


def pack_expanded(output_image_warp, my_map, rgb, depth):
    """The packed arrays with the expansion in front (what :138 and :147-177 build with update_known_views=True). rgb is the renderer's
    output before the clamp."""
    h, w = my_map.shape
    eroded, mask_ex = erode5(my_map)
    u8 = (output_image_warp * np.float32(255)).astype(np.uint8) * eroded[:, :, None].astype(np.uint8)
    rgb_u8 = (np.clip(rgb.reshape(h, w, 3), np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
    masked = np.where(eroded[:, :, None] > 0, rgb_u8, np.uint8(255))
    return dict(output_image_warp_u8=u8, myMap_filt=eroded, mask_image=(eroded * 255).astype(np.uint8),
                mask_inv=((1 - eroded) * 255).astype(np.uint8), mask_ex=mask_ex, rgb_render=rgb_u8, rgb_render_=masked,
                depth_rendered=depth.reshape(h, w) * eroded)
