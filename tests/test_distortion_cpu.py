"""The float64 reference of the distortion regulariser (tests/helpers/distortion_ref.py) held to itself on the CPU: its analytic
gradient against torch.autograd and central finite differences of its own loss, the prefix-sum identity the kernel uses against the
double sum, directed rays against hand-computed values, and the case table against the shapes the GPU test relies on. One check reads
the library's header and the Python surface, so that this file fails where the feature is missing."""
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import distortion_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO = 1.0 / D.Z_RANGE
CASES = D.all_cases()
SMALL = [cid for cid, c in sorted(CASES.items()) if c["w"].size <= 2048]


def torch_loss(w, z, rho):
    """The definition as torch ops in float64 (the double sum), differentiable in w."""
    z = z.double()
    dz = torch.zeros_like(z)
    dz[:, :-1] = z[:, 1:] - z[:, :-1]
    m = ((z - z[:, :1]) + dz / 2) * rho
    pair = (w[:, :, None] * w[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum((1, 2))
    return (pair + (w * w * dz * rho).sum(1) / 3).mean()


@pytest.mark.parametrize("cid", SMALL)
def test_gradient_equals_autograd_of_the_double_sum(cid):
    c = CASES[cid]
    w = torch.from_numpy(c["w"]).double().requires_grad_(True)
    loss = torch_loss(w, torch.from_numpy(c["z"]), RHO)
    loss.backward()
    want_l, want_g = D.distortion(c["w"], c["z"], RHO)
    Ai, Ar = D.magnitudes(c["w"], c["z"], RHO)
    R = c["w"].shape[0]
    assert abs(float(loss.detach()) - want_l) <= 1e-12 * float(Ar.sum()) / R + 1e-300
    assert np.all(np.abs(w.grad.numpy() - want_g) <= 1e-12 * Ai / R + 1e-300)


@pytest.mark.parametrize("cid", ["dense-3x2", "dense-5x64", "box-3x65", "directed-4x65"])
def test_gradient_equals_central_differences(cid):
    """L is a quadratic form in w: the central difference of step h is exact up to rounding, |error| ~ eps |D| / h."""
    c = CASES[cid]
    w, z = c["w"][:, :40], c["z"][:, :40]
    _, g = D.distortion(w, z, RHO)
    w64 = w.astype(np.float64)
    h = 2.0 ** -10

    def value(wq):
        # (per_ray takes float32 weights; the perturbed ones are float64, so the definition is restated on them)
        m, delta = D.geometry(z, RHO)
        L = np.einsum("ri,rij,rj->r", wq, np.abs(m[:, :, None] - m[:, None, :]), wq) + np.sum(wq * wq * delta, axis=1) / 3.0
        return float(L.sum() / wq.shape[0])

    base = abs(value(w64)) + 1.0
    rng = np.random.default_rng(5)
    for r, n in zip(rng.integers(0, w.shape[0], 12), rng.integers(0, w.shape[1], 12)):
        up, dn = w64.copy(), w64.copy()
        up[r, n] += h
        dn[r, n] -= h
        fd = (value(up) - value(dn)) / (2 * h)
        assert abs(fd - g[r, n]) <= 64 * 2.0 ** -53 * base / h, (cid, r, n, fd, g[r, n])


@pytest.mark.parametrize("cid", sorted(CASES))
def test_prefix_sum_identity_equals_the_double_sum(cid):
    c = CASES[cid]
    L, g = D.per_ray(c["w"], c["z"], RHO)
    Lp, gp = D.per_ray_prefix(c["w"], c["z"], RHO)
    Ai, Ar = D.magnitudes(c["w"], c["z"], RHO)
    assert np.all(np.abs(L - Lp) <= 1e-12 * Ar)
    assert np.all(np.abs(g - gp) <= 1e-12 * Ai)


def test_directed_values():
    N = 9
    z = np.linspace(2.0, 6.0, N, dtype=np.float32)[None]       # exact in float32: steps of 0.5
    step = 0.5 * RHO
    # one non-zero sample: L = w^2 delta / 3
    w = np.zeros((1, N), np.float32)
    w[0, 3] = 0.75
    L, g = D.per_ray(w, z, RHO)
    assert L[0] == 0.75 ** 2 * step / 3.0
    assert g[0, 3] == (2.0 / 3.0) * 0.75 * step and g[0, 0] == 2 * 0.75 * 3 * step
    # only the last sample: exactly 0 (its interval is 0)
    w = np.zeros((1, N), np.float32)
    w[0, N - 1] = 0.5
    L, g = D.per_ray(w, z, RHO)
    assert L[0] == 0.0 and g[0, N - 1] == 0.0
    # two unit spikes at samples 1 and 6: 2 |m_1 - m_6| + the two self terms
    w = np.zeros((1, N), np.float32)
    w[0, 1] = w[0, 6] = 1.0
    L, _ = D.per_ray(w, z, RHO)
    assert abs(L[0] - (2 * 5 * step + 2 * step / 3.0)) <= 4 * 2.0 ** -53 * L[0]
    # the second spike on the last sample: its self term is gone, its midpoint is the sample itself (half a step less)
    w = np.zeros((1, N), np.float32)
    w[0, 1] = w[0, N - 1] = 1.0
    L, _ = D.per_ray(w, z, RHO)
    assert abs(L[0] - (2 * 6.5 * step + step / 3.0)) <= 4 * 2.0 ** -53 * L[0]
    # all-equal z: exactly 0, gradient included
    c = CASES["equalz-5x65"]
    L, g = D.per_ray(c["w"], c["z"], RHO)
    assert not L.any() and not g.any()
    Lp, gp = D.per_ray_prefix(c["w"], c["z"], RHO)
    assert not Lp.any() and not gp.any()


def test_the_case_table_has_the_tile_edges_and_ray_counts():
    shapes = {c["w"].shape for c in CASES.values()}
    assert {n for _, n in shapes} >= set(D.N_SHAPES)
    assert {r for r, _ in shapes} >= set(D.R_SHAPES)
    assert D.NARROW in shapes
    for pattern in ("dense", "box", "directed"):
        ns = {c["w"].shape[1] for c in CASES.values() if c["pattern"] == pattern}
        assert ns & {63, 64} and 65 in ns, pattern              # both sides of the 64-sample tile carry
        assert any(c["w"].shape[0] % 4 for c in CASES.values() if c["pattern"] == pattern)     # a partial workgroup
    for cid, c in CASES.items():
        z = c["z"]
        assert z.dtype == np.float32 and c["w"].dtype == np.float32
        assert np.all(np.diff(z, axis=1) >= 0) and z.min() >= 2.0 and z.max() <= 6.0, cid
    assert any(np.any(np.diff(c["z"], axis=1) == 0) for c in CASES.values() if c["z"].shape[1] > 2)      # repeated depths
    box = [c for c in CASES.values() if c["pattern"] == "box"]
    assert all(not c["w"][c["w"].shape[0] // 2].any() for c in box)          # one ray without weight
    assert any((c["w"] == 0).any() and (c["w"] != 0).any() for c in box)


def test_the_feature_is_declared_on_every_layer():
    header = open(os.path.join(ROOT, "include", "t2n.h")).read()
    for name in ("t2n_distortion_loss", "t2n_distortion_loss_workspace_bytes", "t2n_train_loss_dist", "t2n_train_loss_dist_workspace_bytes"):
        assert re.search(r"\b" + name + r"\(", header), name
    from text2nerf_amd import _lib, losses
    import inspect
    from text2nerf_amd.tensorf import TensorVMSplit
    assert {"t2n_distortion_loss", "t2n_train_loss_dist"} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["t2n_train_loss_dist"][1]) == len(_lib.SIGNATURES["t2n_train_loss_ex"][1]) + 3
    assert callable(losses.distortion_loss)
    for fn in (TensorVMSplit.train_step, TensorVMSplit.train_step_indexed):
        assert inspect.signature(fn).parameters["distortion"].default == 0.0
    with pytest.raises(_lib.T2NError):
        losses.distortion_loss(torch.zeros(2, 3), torch.zeros(2, 3), 4.0)        # CPU tensors: no fallback
