"""float64 restatement of both sides of the identity behind the cached appearance feature volume (t2n_app_volume.hip).

Feature j of a sample is sum_k sum_c B[j, C k + c] * (bilinear tap of plane k)[c] * (linear tap of line k)[c]; in every plane / line pair
the four plane taps times the two line taps are the eight corners of the sample's cell, so the features are the trilinear interpolation
of F_j(corner) = sum_k sum_c B[j, C k + c] P_k[corner][c] L_k[corner][c]. Both sides are computed here from the same fp32 factors in
float64, with the reference's taps (grid_sample, align_corners=True: ix = (g + 1) / 2 * (size - 1), corner = floor, weights by
subtraction; positions lie in [-1, 1], the high tap is clamped to the last texel where its weight is 0).

Layouts: planes[k] is [H_k, W_k, C] and lines[k] is [L_k, C] (channel-last), with matMode = [[0, 1], [0, 2], [1, 2]] and
vecMode = [2, 1, 0]: W_k = grid[matMode[k][0]], H_k = grid[matMode[k][1]], L_k = grid[vecMode[k]]; basis is [n_feat, 3 C]."""
import numpy as np

MAT = [(0, 1), (0, 2), (1, 2)]
VEC = [2, 1, 0]


def random_factors(grid, C, n_feat, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    planes = [rng.standard_normal((grid[MAT[k][1]], grid[MAT[k][0]], C)).astype(np.float32) for k in range(3)]
    lines = [rng.standard_normal((grid[VEC[k]], C)).astype(np.float32) for k in range(3)]
    basis = (rng.standard_normal((n_feat, 3 * C)) / np.sqrt(3 * C)).astype(np.float32)
    return planes, lines, basis


def factors_from_state(params, grid):
    """The same layouts from a TensorVMSplit state dict (app_plane.k [1, C, H, W], app_line.k [1, C, L, 1], basis_mat.weight)."""
    planes = [np.ascontiguousarray(np.asarray(params[f"app_plane.{k}"])[0].transpose(1, 2, 0)) for k in range(3)]
    lines = [np.ascontiguousarray(np.asarray(params[f"app_line.{k}"])[0, :, :, 0].T) for k in range(3)]
    return planes, lines, np.asarray(params["basis_mat.weight"])


def axis_taps(g, size):
    """(low index, high index, low weight, high weight) per position, float64 (g: fp32 coordinates in [-1, 1])"""
    ix = (np.asarray(g, np.float64) + 1.0) / 2.0 * (size - 1)
    f0 = np.floor(ix)
    w1 = ix - f0
    i0 = np.clip(f0.astype(np.int64), 0, size - 1)
    i1 = np.minimum(i0 + 1, size - 1)
    return i0, i1, 1.0 - w1, w1


def direct_features(planes, lines, basis, grid, pts):
    """[n, n_feat]: blend the plane and the line taps per pair, multiply, contract with the basis"""
    C = lines[0].shape[1]
    t = [axis_taps(pts[:, a], grid[a]) for a in range(3)]
    out = np.zeros((pts.shape[0], basis.shape[0]))
    B = basis.astype(np.float64)
    for k in range(3):
        ax, ay, al = t[MAT[k][0]], t[MAT[k][1]], t[VEC[k]]
        P = planes[k].astype(np.float64)
        L = lines[k].astype(np.float64)
        pv = (P[ay[0], ax[0]] * (ay[2] * ax[2])[:, None] + P[ay[0], ax[1]] * (ay[2] * ax[3])[:, None] +
              P[ay[1], ax[0]] * (ay[3] * ax[2])[:, None] + P[ay[1], ax[1]] * (ay[3] * ax[3])[:, None])
        lv = L[al[0]] * al[2][:, None] + L[al[1]] * al[3][:, None]
        out += (pv * lv) @ B[:, C * k:C * (k + 1)].T
    return out


def corner_volume(planes, lines, basis, grid):
    """F[z, y, x, n_feat] of every grid corner"""
    C = lines[0].shape[1]
    B = basis.astype(np.float64)
    gx, gy, gz = grid
    z, y, x = np.meshgrid(np.arange(gz), np.arange(gy), np.arange(gx), indexing="ij")
    c = [x, y, z]
    F = np.zeros((gz, gy, gx, basis.shape[0]))
    for k in range(3):
        P = planes[k].astype(np.float64)[c[MAT[k][1]], c[MAT[k][0]]]
        L = lines[k].astype(np.float64)[c[VEC[k]]]
        F += (P * L) @ B[:, C * k:C * (k + 1)].T
    return F


def volume_features(F, grid, pts):
    """[n, n_feat]: trilinear interpolation of the corner volume with the same taps"""
    tx, ty, tz = (axis_taps(pts[:, a], grid[a]) for a in range(3))
    out = np.zeros((pts.shape[0], F.shape[-1]))
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                w = tx[2 + dx] * ty[2 + dy] * tz[2 + dz]
                out += F[tz[dz], ty[dy], tx[dx]] * w[:, None]
    return out


def test_points(grid, n, seed):
    """fp32 positions in [-1, 1]^3: cell interiors, positions exactly on corners, positions on the upper faces of the box"""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = np.asarray(grid)
    inner = rng.uniform(-1.0, 1.0, (n, 3))
    corners = rng.integers(0, g, (n, 3)) / (g - 1.0) * 2.0 - 1.0
    faces = rng.uniform(-1.0, 1.0, (n, 3))
    faces[np.arange(n), rng.integers(0, 3, n)] = 1.0
    last = rng.uniform(0.0, 1.0, (n, 3)) * (2.0 / (g - 1.0)) + (1.0 - 2.0 / (g - 1.0))     # inside the last cell of every axis
    return np.clip(np.concatenate([inner, corners, faces, last]), -1.0, 1.0).astype(np.float32)
