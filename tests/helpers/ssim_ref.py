"""SSIM on the CPU in plain numpy, in the project's own words: what the device kernel (csrc/t2n_metrics.hip) has to compute, checked
against the reference's outputs (tests/golden/ssim.npz) by tests/test_ssim_cpu.py and leaned on by the GPU tests at shapes the fixture
does not hold. No scipy: the separable "valid" convolution is written as ONE full 2-D window, weight[i, j] = g[i] g[j], summed in
float64 over a sliding-window view (so its summation order is neither scipy's nor the kernel's). The products a*a, b*b, a*b are
formed in the INPUT dtype (float32 or float64) and widened afterwards, as `img0**2` is in the reference."""
import numpy as np


def taps(filter_size, filter_sigma):
    """Normalised 1-D Gaussian taps; an even length is centred between its two middle taps."""
    g = np.exp(-0.5 * ((np.arange(filter_size) - (filter_size - 1) / 2) / filter_sigma)**2)
    return g / np.sum(g)


def window_mean(z, g):
    """[H,W,3] -> [H-fs+1,W-fs+1,3]: every fs x fs window weighted by flip(g) x flip(g) (a convolution), in float64."""
    z = np.asarray(z, np.float64)
    fs = len(g)
    w2 = np.outer(g[::-1], g[::-1])
    win = np.lib.stride_tricks.sliding_window_view(z, (fs, fs), axis=(0, 1))      # [OH,OW,3,fs,fs]
    return np.einsum("hwcij,ij->hwc", win, w2)


def ssim_map(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, window_mean=window_mean):
    """`window_mean`: another form of the same windowed mean (tools/time_ssim.py times the host route with a separable scipy one)."""
    a, b = np.asarray(img0), np.asarray(img1)
    if a.dtype not in (np.float32, np.float64):
        a, b = a.astype(np.float64), b.astype(np.float64)
    assert a.shape == b.shape and a.ndim == 3 and a.shape[-1] == 3 and a.dtype == b.dtype
    g = taps(filter_size, filter_sigma)
    mu0, mu1 = window_mean(a, g), window_mean(b, g)
    var0 = np.maximum(window_mean(a * a, g) - mu0 * mu0, 0.0)
    var1 = np.maximum(window_mean(b * b, g) - mu1 * mu1, 0.0)
    cov = window_mean(a * b, g) - mu0 * mu1
    cov = np.sign(cov) * np.minimum(np.sqrt(var0 * var1), np.abs(cov))
    c1, c2 = (k1 * max_val)**2, (k2 * max_val)**2
    return ((2 * mu0 * mu1 + c1) * (2 * cov + c2)) / ((mu0 * mu0 + mu1 * mu1 + c1) * (var0 + var1 + c2))


def ssim(img0, img1, max_val, **kw):
    return float(np.mean(ssim_map(img0, img1, max_val, **kw)))


def sq_err(img0, img1):
    """Sum of the squared differences: difference and square in the input dtype, the sum in float64."""
    d = np.asarray(img0) - np.asarray(img1)
    return float(np.sum((d * d).astype(np.float64)))
