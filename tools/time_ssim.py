#!/usr/bin/env python3
"""Time `metrics.ssim_views` (one tile kernel + one reduction per stack, csrc/t2n_metrics.hip) against the route that existed before it:
both stacks copied to the host and every view scored there with 30 separable `scipy.signal.convolve2d` calls (the arithmetic of
tests/helpers/ssim_ref.py with a separable scipy window instead of its full 2-D one). Device float32 stacks in, sizes 512^2 and 800^2,
V = 1 and 9, same process, alternating blocks, warm-up excluded, median over the blocks. The device leg is timed with device events
around `reps` calls; the host leg with a host clock around one call that starts at a synchronised device and ends with the last view's
float. Checks first that both routes agree to 1e-11. Without scipy the comparison leg is skipped and the printed note says so. No
threshold: there is no device predecessor to regress against.

    python tools/time_ssim.py [--blocks 5] [--reps 20] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import ssim_ref  # noqa: E402
from text2nerf_amd import metrics  # noqa: E402

try:
    import scipy.signal
except ImportError:
    scipy = None


def separable_mean(z, g):
    z = np.asarray(z, np.float64)
    return np.stack([scipy.signal.convolve2d(scipy.signal.convolve2d(z[..., c], g[:, None], mode="valid"), g[None, :], mode="valid")
                     for c in range(3)], -1)


def host_route(a, b):
    """What a caller did before: two device-to-host copies of the stacks, then the host SSIM of every view."""
    an, bn = a.cpu().numpy(), b.cpu().numpy()
    return [float(np.mean(ssim_ref.ssim_map(an[v], bn[v], 1.0, window_mean=separable_mean))) for v in range(an.shape[0])]


def timed_device(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def timed_host(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def med(xs):
    return f"{statistics.median(xs):.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_ssim.py measures on the GPU only")
    dev = torch.device("cuda:0")
    lines = [f"ssim_views vs the host route (D2H copies + scipy convolve2d per view), float32 device stacks, 11 taps; "
             f"{torch.cuda.get_device_name(0)}; median of {a.blocks} alternating blocks, device leg: device events around {a.reps} calls, "
             f"host leg: host clock around one call; warm-up excluded"]
    if scipy is None:
        lines.append("note: scipy is not installed here, the host leg was skipped (not measured)")
    g = torch.Generator().manual_seed(0)
    for size in (512, 800):
        for V in (1, 9):
            x = torch.rand(V, size, size, 3, generator=g).to(dev)
            y = (x + 0.05 * torch.randn(x.shape, generator=g).to(dev)).clamp(0.0, 1.0)
            one = lambda: metrics.ssim_views(x, y)                    # noqa: E731
            both = lambda: metrics.score_views(x, y)                  # noqa: E731
            got = one().cpu().numpy()
            if scipy is not None:
                want = np.array(host_route(x, y))
                assert np.abs(got - want).max() <= 1e-11, (size, V, np.abs(got - want).max())
            for _ in range(3):
                one(); both()
            t_dev, t_both, t_host = [], [], []
            for _ in range(a.blocks):
                t_dev.append(timed_device(one, a.reps))
                t_both.append(timed_device(both, a.reps))
                if scipy is not None:
                    t_host.append(timed_host(lambda: host_route(x, y)))
            line = f"{size}x{size}, V={V}: ssim_views {med(t_dev)}; score_views (psnr + ssim) {med(t_both)}"
            line += f"; host route {med(t_host)}" if t_host else "; host route not measured"
            lines.append(line)
            print(line, flush=True)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
