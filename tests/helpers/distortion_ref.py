"""Float64 reference of the distortion regulariser (the definition in include/t2n.h), written from the definition: the double sum over
sample pairs and its analytic gradient, on float32 inputs promoted to float64. Also the prefix-sum form the kernel uses (for the CPU
test of the identity), the magnitudes A_i / A of the error bound, and the case table shared by tests/test_distortion_cpu.py and
tests/test_distortion_gpu.py.

For one ray: delta_n = (z[n+1] - z[n]) rho (0 for the last sample), m_n = ((z[n] - z[0]) + (z[n+1] - z[n]) / 2) rho,
L = sum_ij w_i w_j |m_i - m_j| + 1/3 sum_i w_i^2 delta_i, dL/dw_i = 2 sum_j w_j |m_i - m_j| + 2/3 w_i delta_i, D = mean_r L_r."""
import numpy as np

Z_RANGE = 4.0            # near_far = [2, 6]
N_SHAPES = (1, 2, 63, 64, 65, 129, 259, 1025)
R_SHAPES = (1, 3, 4, 5, 301)
NARROW = (1029, 3)


def geometry(z, inv_range):
    """(m, delta) [R, N] float64 of float32 z_vals [R, N]."""
    z = np.asarray(z, np.float32).astype(np.float64)
    rho = float(inv_range)
    dz = np.zeros_like(z)
    dz[:, :-1] = z[:, 1:] - z[:, :-1]
    return ((z - z[:, :1]) + dz / 2.0) * rho, dz * rho


def per_ray(w, z, inv_range):
    """(L [R], dL/dw [R, N]) by the double sum."""
    w = np.asarray(w, np.float32).astype(np.float64)
    m, delta = geometry(z, inv_range)
    inner = np.empty_like(w)                                          # sum_j w_j |m_i - m_j|
    for r in range(w.shape[0]):
        inner[r] = np.abs(m[r][:, None] - m[r][None, :]) @ w[r]
    L = np.sum(w * inner, axis=1) + np.sum(w * w * delta, axis=1) / 3.0
    g = 2.0 * inner + (2.0 / 3.0) * w * delta
    return L, g


def distortion(w, z, inv_range):
    """(D, dD/dw [R, N]) = (mean_r L_r, (1/R) dL_r/dw)."""
    L, g = per_ray(w, z, inv_range)
    R = L.shape[0]
    return float(np.sum(L) / R), g / R


def per_ray_prefix(w, z, inv_range):
    """(L, dL/dw) by the sorted-order identity: exclusive prefix sums of (w, w m), suffix = total - prefix - self."""
    w = np.asarray(w, np.float32).astype(np.float64)
    m, delta = geometry(z, inv_range)
    wm = w * m
    W_lt = np.cumsum(w, axis=1) - w
    WM_lt = np.cumsum(wm, axis=1) - wm
    W_gt = w.sum(1, keepdims=True) - W_lt - w
    WM_gt = wm.sum(1, keepdims=True) - WM_lt - wm
    before = m * W_lt - WM_lt
    L = 2.0 * np.sum(w * before, axis=1) + np.sum(w * w * delta, axis=1) / 3.0
    g = 2.0 * (before + (WM_gt - m * W_gt)) + (2.0 / 3.0) * w * delta
    return L, g


def magnitudes(w, z, inv_range):
    """(A_i [R, N], A_r [R]) of the bounds, per ray and unscaled: A_i = 2 sum_j |w_j| (|m_i| + |m_j|) + 2/3 |w_i| delta_i, the sum of
    the magnitudes of the terms of dL/dw_i; A_r = sum_i |w_i| A_i / 2, the same for L_r."""
    w = np.abs(np.asarray(w, np.float32).astype(np.float64))
    m, delta = geometry(z, inv_range)
    am = np.abs(m)
    Ai = 2.0 * (am * w.sum(1, keepdims=True) + (w * am).sum(1, keepdims=True)) + (2.0 / 3.0) * w * delta
    return Ai, np.sum(w * Ai, axis=1) / 2.0


def grad_bound(w, z, inv_range, want):
    """|got - want| <= 2^-23 |want| + 1e-12 A_i / R: one float32 rounding, and the float64 summation order (4 N 2^-53 <= 1e-12 for
    N <= 2048)."""
    Ai, _ = magnitudes(w, z, inv_range)
    return 2.0 ** -23 * np.abs(want) + 1e-12 * Ai / Ai.shape[0]


def loss_bound(w, z, inv_range, want):
    _, Ar = magnitudes(w, z, inv_range)
    return 2.0 ** -23 * abs(want) + 1e-12 * float(np.sum(Ar)) / Ar.shape[0]


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
def sorted_z(rng, R, N):
    """Sorted depths in [2, 6], float32, with some values repeated along a ray."""
    z = np.sort(rng.uniform(2.0, 6.0, (R, N)), axis=1).astype(np.float32)
    if N >= 3:
        for r in range(R):
            i = rng.integers(0, N - 1, size=max(1, N // 16))
            z[r, i + 1] = z[r, i]
        z = np.sort(z, axis=1)
    return z


def directed_rays(N):
    """The directed rays of the CPU test at N samples (N >= 2): (name, w [N]) — one sample, only the last, two unit spikes."""
    one = np.zeros(N, np.float32)
    one[N // 3] = 0.75
    last = np.zeros(N, np.float32)
    last[N - 1] = 0.5
    two = np.zeros(N, np.float32)
    two[0] = 1.0
    two[N - 1 if N < 4 else (2 * N) // 3] = 1.0
    return [("one", one), ("last", last), ("two", two)]


def make_case(R, N, pattern, seed):
    rng = np.random.default_rng([11, R, N, seed])
    z = sorted_z(rng, R, N)
    if pattern == "dense":
        w = (rng.uniform(0.0, 1.0, (R, N)) * (2.0 / N)).astype(np.float32)
    elif pattern == "box":
        # exact zeros outside a window per ray; the middle ray has no weight at all
        w = np.zeros((R, N), np.float32)
        for r in range(R):
            lo = int(rng.integers(0, N))
            hi = int(rng.integers(lo, N)) + 1
            w[r, lo:hi] = rng.uniform(0.1, 1.0, hi - lo).astype(np.float32)
        w[R // 2] = 0.0
    else:
        assert pattern == "directed" and N >= 2
        rows = directed_rays(N)
        w = np.stack([rows[r % 3][1] for r in range(R)])
    return {"w": w, "z": z, "pattern": pattern}


def all_cases():
    """id -> case. Dense weights at every N x a rotating R (every R appears, 301 at N = 259), box weights and the directed rays at the
    tile edges, the narrow case, and one all-equal-z case."""
    cases = {}
    for i, N in enumerate(N_SHAPES):
        R = R_SHAPES[i % len(R_SHAPES)] if N != 259 else 301
        cases[f"dense-{R}x{N}"] = make_case(R, N, "dense", 0)
    for R in R_SHAPES:
        if not any(k.startswith(f"dense-{R}x") for k in cases):
            cases[f"dense-{R}x65"] = make_case(R, 65, "dense", 1)
    for R, N in ((5, 63), (4, 64), (3, 65), (5, 129), (301, 65), (1, 1), (3, 2)):
        cases[f"box-{R}x{N}"] = make_case(R, N, "box", 2)
    for R, N in ((3, 2), (5, 64), (4, 65), (3, 259), (1, 1025)):
        cases[f"directed-{R}x{N}"] = make_case(R, N, "directed", 3)
    cases[f"dense-{NARROW[0]}x{NARROW[1]}"] = make_case(*NARROW, "dense", 4)
    flat = make_case(5, 65, "dense", 5)
    flat["z"][:] = np.float32(3.25)
    cases["equalz-5x65"] = flat
    return cases
