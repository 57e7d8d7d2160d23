"""Float64 references, case tables and per-element checkers for the L1 and ortho regularisers (csrc/t2n_reg.hip;
models/tensoRF.py:173-191). numpy only. Pinned to the reference's own autograd in tests/test_reg_ref_cpu.py (tests/golden/reg_terms.npz),
used on the GPU by tests/test_reg_kernels_gpu.py and tests/test_reg_train_step_gpu.py.

L1:    value = sum_t mean|t|;  gradient of one tensor T under weight w = float32(w / numel(T)) * sign(t), sign(+-0) = 0.
Ortho: M [C, n];  D = M M^T;  value = sum_{i != j} |D_ij| / (C (C - 1));  gradient = 2 / (C (C - 1)) * S M, S = sign(D) off the diagonal.

Bounds (derived, not tuned):
* an L1 SET gradient equals float32(float32(w / numel) [* up]) * sign exactly: one constant with a sign bit, no arithmetic per element;
* an ortho gradient element (a, b) is a sum of at most C terms +-M_jb, times one float32 constant: within
  (C + 4) 2^-24 * |w up| 2 / (C (C - 1)) * sum_{j != a} |M_jb| of the oracle (C - 1 additions, the constant's own rounding, its
  product with the upstream scalar, the final product; the worst case of a sequential float32 sum — the kernels sum in float64 and
  sit far inside it);
* the sign band: the kernel's float64 D and this module's differ by the order of n - 1 additions of exact products, each side within
  n 2^-53 |m_i| |m_j| of the true value: a pair is AMBIGUOUS when |D_ij| <= n 2^-50 |m_i| |m_j|. Random cases must hold none
  (asserted on the CPU); rows of disjoint support give D_ij = 0 exactly in any order, and such a pair must add exactly nothing."""
import numpy as np

U = 2.0 ** -24          # one float32 rounding, relative


def f32(x):
    return float(np.float32(x))


# ---- L1 -------------------------------------------------------------------------------------------------------------------------------
def l1_value(tensors):
    return float(sum(np.abs(np.asarray(t, np.float64)).mean() for t in tensors))


def l1_scale(w, numel, up=None):
    """The constant the kernels multiply the sign by: float32(w / numel) in float64 arithmetic, then one float32 product with `up`."""
    s = np.float32(np.float64(np.float32(w)) / np.float64(numel))
    return float(s if up is None else np.float32(s * np.float32(up)))


def sign0(x):
    """sign with sign(+-0) = 0 and denormals counted (numpy's float32 comparisons keep them)."""
    x = np.asarray(x)
    return (x > 0).astype(np.float64) - (x < 0).astype(np.float64)


def l1_grad(x, w, up=None, numel=None):
    x = np.asarray(x)
    return l1_scale(w, x.size if numel is None else numel, up) * sign0(x)


def check_l1_set(got, x, w, up=None):
    """Failures (a list, empty = pass) of an L1 SET gradient against the exact expectation."""
    want = l1_grad(x, w, up).astype(np.float32)
    got = np.asarray(got, np.float32)
    bad = np.argwhere(got != want)          # (+0.0 == -0.0: the sign of a zero gradient is not pinned)
    return [("l1 set", tuple(i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:4]]


def check_l1_add(got, prev, x, w):
    """got = prev + L1 gradient in float32: one addition of the exact constant."""
    want = (np.asarray(prev, np.float32) + l1_grad(x, w).astype(np.float32)).astype(np.float32)
    got = np.asarray(got, np.float32)
    bad = np.argwhere(got != want)
    return [("l1 add", tuple(i), float(got[tuple(i)]), float(want[tuple(i)])) for i in bad[:4]]


# ---- ortho ----------------------------------------------------------------------------------------------------------------------------
def as_matrix(line):
    """[1, C, n, 1] / [C, n, 1] / [C, n] -> float64 [C, n]."""
    a = np.asarray(line, np.float64)
    if a.ndim == 4:
        a = a[0]
    if a.ndim == 3:
        a = a[:, :, 0]
    return a


def gram(M):
    M = as_matrix(M)
    return M @ M.T


def ortho_value(M):
    D = gram(M)
    C = D.shape[0]
    return float((np.abs(D).sum() - np.abs(np.diag(D)).sum()) / (C * (C - 1)))


def ortho_sign(M):
    S = np.sign(gram(M))
    np.fill_diagonal(S, 0.0)
    return S


def ortho_grad(M, w=1.0):
    M = as_matrix(M)
    C = M.shape[0]
    return float(w) * 2.0 / (C * (C - 1)) * (ortho_sign(M) @ M)


def ambiguous_pairs(M):
    """Off-diagonal pairs (i, j) whose sign the float64 accumulation order could change: 0 < |D_ij| <= n 2^-50 |m_i| |m_j|. (D_ij = 0 from
    products that are all exactly 0 is not ambiguous: it is 0 in any order.)"""
    M = as_matrix(M)
    D = M @ M.T
    norm = np.sqrt((M * M).sum(1))
    band = M.shape[1] * 2.0 ** -50 * norm[:, None] * norm[None, :]
    exact_zero = (np.abs(M)[:, None, :] * np.abs(M)[None, :, :]).max(-1) == 0.0
    amb = (np.abs(D) <= band) & ~exact_zero
    np.fill_diagonal(amb, False)
    return np.argwhere(amb)


def ortho_grad_tolerance(M, w=1.0, up=1.0):
    M = as_matrix(M)
    C = M.shape[0]
    col = np.abs(M).sum(0)[None, :] - np.abs(M)          # sum_{j != a} |M_jb|
    return (C + 4) * U * abs(float(w) * float(up)) * 2.0 / (C * (C - 1)) * col


def check_ortho_grad(got, M, w=1.0, up=1.0, prev=None):
    """Failures (empty = pass) of an ortho gradient [C, n] (SET, or ADD on top of `prev` with half an ulp of the result for the one
    addition) against float64, element by element."""
    M = as_matrix(M)
    got = as_matrix(got)
    want = ortho_grad(M, float(w) * float(up))
    tol = ortho_grad_tolerance(M, w, up)
    if prev is not None:
        want = want + as_matrix(prev)
        tol = tol + 0.5 * np.spacing(np.abs(got).astype(np.float32)).astype(np.float64)
    err = np.abs(got - want)
    bad = np.argwhere(~(err <= tol))
    return [("ortho grad", tuple(i), float(got[tuple(i)]), float(want[tuple(i)]), float(tol[tuple(i)])) for i in bad[:4]]


def kernel_model_ortho(M, w, up=None, normaliser=None, factor=2.0, sign_of_zero=0.0, diagonal=False):
    """The ortho gradient kernel's arithmetic in numpy: float64 Gram matrix, a float64 sum over j = 0 .. C - 1 in that order, the constant
    (times the upstream scalar) in float64, one rounding to float32. The keyword arguments build WRONG kernels for the checkers' own tests."""
    M32 = as_matrix(M).astype(np.float32)
    C, n = M32.shape
    D = M32.astype(np.float64) @ M32.astype(np.float64).T
    S = np.sign(D)
    S[D == 0] = sign_of_zero
    if not diagonal:
        np.fill_diagonal(S, 0.0)
    norm = C * (C - 1) if normaliser is None else normaliser
    scale = np.float64(np.float32(w)) * factor / norm
    if up is not None:
        scale = scale * np.float64(np.float32(up))
    acc = np.zeros((C, n), np.float64)
    for j in range(C):
        acc = acc + S[:, j, None] * M32[j][None, :].astype(np.float64)
    return (scale * acc).astype(np.float32)


# ---- case tables ------------------------------------------------------------------------------------------------------------------------
L1_SHAPES = [(16, 2, 2), (3, 4, 200), (2, 3, 65), (48, 23, 19), (16, 1, 1)]
ORTHO_C = (2, 3, 16, 20, 48, 96)
ORTHO_N = (1, 2, 17, 63, 64, 65, 300)
L1_WEIGHT, ORTHO_WEIGHT, UPSTREAM = 0.37, 0.83, 1.7


def l1_plane(shape):
    """A [1, C, H, W] float32 plane from the shape's own seed, holding +0.0, -0.0, float32 denormals of both signs and normal values."""
    c, h, w = shape
    rng = np.random.default_rng([41, c, h, w])
    x = rng.standard_normal((1, c, h, w)).astype(np.float32)
    flat = x.reshape(-1)
    kinds = rng.integers(0, 8, flat.size)
    flat[kinds == 0] = 0.0
    flat[kinds == 1] = -0.0
    flat[kinds == 2] = np.float32(1e-41)
    flat[kinds == 3] = np.float32(-3e-42)
    # (every kind present whatever the draw: the first five elements)
    flat[:5] = np.array([0.0, -0.0, 1e-41, -3e-42, 1.5], np.float32)
    return x


def ortho_line(C, n):
    """A [1, C, n, 1] float32 line from the case's own seed (0.1-scale normals, the field's initialisation)."""
    rng = np.random.default_rng([43, C, n])
    return (0.1 * rng.standard_normal((1, C, n, 1))).astype(np.float32)


def disjoint_line():
    """[1, 6, 12, 1]: rows 0 / 1 / 2 live on positions 0-3 / 4-7 / 8-11 (pairwise D = 0 exactly, in any order); rows 3-5 are dense, so
    every row still has pairs that count."""
    rng = np.random.default_rng(47)
    M = np.zeros((6, 12), np.float32)
    for r in range(3):
        M[r, 4 * r:4 * r + 4] = rng.standard_normal(4).astype(np.float32)
    M[3:] = rng.standard_normal((3, 12)).astype(np.float32)
    return M[None, :, :, None].copy()


def ortho_cases():
    out = {f"{C}x{n}": ortho_line(C, n) for C in ORTHO_C for n in ORTHO_N}
    out["disjoint"] = disjoint_line()
    return out
