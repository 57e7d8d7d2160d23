"""The SSIM golden cases (tests/golden/ssim.npz): inputs rebuilt from seeds, shared by the generator (make_golden_ssim.py) and the tests
(tests/test_ssim_cpu.py, tests/test_ssim_gpu.py). Only the reference's outputs are stored.

An image pair [H,W,3] in [0,1]: uniform noise and a perturbed copy of it, with the top-left quarter IDENTICAL in both images (sigma01
meets its sqrt(sigma00 sigma11) clamp there) and the bottom-right quarter FLAT at 0.25 in both (E[x^2] - mu^2 cancels to rounding noise,
which the max(0, .) clamp cuts). `max_val` 255 scales both images by 255. Pixel values are float32 values in BOTH dtypes (the float64
case is the float32 one widened), so the two cases of a pair differ in nothing but the dtype the products a*a, b*b, a*b are formed in.
Two flat pairs besides: identical (the reference returns exactly 1.0) and 0.3 against 0.7."""
import numpy as np

SIZES = [(11, 11), (12, 29), (23, 37), (64, 45)]
FILTERS = [(11, 1.5), (8, 1.0), (5, 0.8)]       # the default; an even length (the `shift` term of the taps); a short one


def image_pair(H, W, seed, dtype, max_val=1):
    rng = np.random.default_rng(seed)
    a = rng.random((H, W, 3))
    b = np.clip(a + 0.15 * rng.standard_normal((H, W, 3)), 0.0, 1.0)
    b[:H // 2, :W // 2] = a[:H // 2, :W // 2]
    a[H - H // 2:, W - W // 2:] = 0.25
    b[H - H // 2:, W - W // 2:] = 0.25
    a, b = a.astype(np.float32), b.astype(np.float32)
    if max_val != 1:
        a, b = a * np.float32(max_val), b * np.float32(max_val)
    return a.astype(dtype), b.astype(dtype)


def flat_pair(H, W, v0, v1, dtype):
    return np.full((H, W, 3), v0, dtype), np.full((H, W, 3), v1, dtype)


def cases():
    """[(name, kind, H, W, dtype name, max_val, filter_size, filter_sigma, seed)]; the largest size keeps the default filter only
    so that the fixture stays small."""
    out = []
    for si, (H, W) in enumerate(SIZES):
        for fs, sigma in FILTERS:
            if fs > min(H, W):
                continue
            for dt in ("float32", "float64"):
                for mv in (1, 255):
                    if (H, W) == SIZES[-1] and fs != 11:
                        continue
                    out.append((f"pair_{H}x{W}_f{fs}_{dt}_m{mv}", "pair", H, W, dt, mv, fs, sigma, 100 + si))
    for dt in ("float32", "float64"):
        out.append((f"flat_same_{dt}", "flat_same", 12, 29, dt, 1, 11, 1.5, 0))
        out.append((f"flat_diff_{dt}", "flat_diff", 12, 29, dt, 1, 11, 1.5, 0))
    return out


def inputs(case):
    name, kind, H, W, dt, mv, fs, sigma, seed = case
    dtype = getattr(np, dt)
    if kind == "pair":
        return image_pair(H, W, seed, dtype, mv)
    if kind == "flat_same":
        return flat_pair(H, W, 0.5, 0.5, dtype)
    return flat_pair(H, W, 0.3, 0.7, dtype)
