"""The float64 reference of the geometry outputs (tests/helpers/geometry_ref.py) held to the reference's own operator, the ray-level
claims of include/t2n.h checked on it, the condition that keeps the device bounds from hiding a failure, and mutation tests of the
checkers that tests/test_geometry_gpu.py applies to the device's results: every deliberate error must be caught. No GPU."""
import numpy as np
import pytest
import torch

from tests.conftest import GOLDEN, TINY
from tests.helpers import geometry_ref as G
from text2nerf_amd import synth

MISS = 8.0


@pytest.fixture(scope="module")
def pool():
    import os
    return G.pool_rays(np.load(os.path.join(GOLDEN, "tiny.npz"), allow_pickle=False)["tiny_rays"])


@pytest.fixture(scope="module")
def cases():
    """kind -> (cfg, float64 factors) of the ray-level field."""
    params = G.ray_params(TINY)
    vol = G.oracle_mask_volume(TINY, params)
    assert 0.02 < float(vol.mean()) < 0.98, "the mask must drop some samples and keep others"
    return {"plain": (G.make_cfg(TINY), G.params64_of(params)), "mask": (G.make_cfg(TINY, vol), G.params64_of(params)),
            "bf16": (G.make_cfg(TINY), G.params64_of(params, bf16=True))}


@pytest.fixture(scope="module")
def refs(cases, pool):
    return {(kind, N): G.RayRef(cfg, P, pool, N) for kind, (cfg, P) in cases.items() for N in G.NS}


@pytest.fixture(scope="module")
def fine_refs(cases):
    """(kind, N) -> reference of the nine long rays on the same fields at step_ratio FINE_RATIO (windows of up to four blocks)."""
    out = {}
    for kind, (cfg, P) in cases.items():
        fine = G.make_cfg(TINY, cfg.alpha_volume, step_ratio=G.FINE_RATIO)
        for N in G.FINE_NS:
            out[(kind, N)] = G.RayRef(fine, P, G.fine_rays(), N)
    return out


def grid_sample_field(P, xn):
    """compute_densityfeature as the reference writes it (models/tensoRF.py:205-220), float64, differentiable in xn."""
    f = torch.zeros(xn.shape[0], dtype=torch.float64)
    for k in range(3):
        m0, m1 = G.MAT_MODE[k]
        v = G.VEC_MODE[k]
        cp = torch.stack((xn[:, m0], xn[:, m1]), -1).view(1, -1, 1, 2)
        cl = torch.stack((torch.zeros_like(xn[:, v]), xn[:, v]), -1).view(1, -1, 1, 2)
        p = torch.nn.functional.grid_sample(P[f"density_plane.{k}"], cp, align_corners=True).view(-1, xn.shape[0])
        l = torch.nn.functional.grid_sample(P[f"density_line.{k}"], cl, align_corners=True).view(-1, xn.shape[0])
        f = f + (p * l).sum(0)
    return f


@pytest.mark.parametrize("shape", [TINY, G.GRID37], ids=["tiny", "37x23x29"])
def test_reference_is_grid_sample_and_its_autograd(shape):
    grid = shape["grid"]
    P = G.params64_of(synth.make_field_params(3, grid, density_scale=0.9, aabb=shape["aabb"]))
    rng = np.random.default_rng(1)
    # cell index + a fraction at least 1e-3 of a cell away from either face
    idx = np.stack([rng.integers(0, g - 1, 400) + rng.uniform(1e-3, 1 - 1e-3, 400) for g in grid], -1)
    xn = torch.tensor(2.0 * idx / (np.asarray(grid) - 1.0) - 1.0, dtype=torch.float64, requires_grad=True)
    want_f = grid_sample_field(P, xn)
    (want_dn,) = torch.autograd.grad(want_f.sum(), xn)
    a = torch.tensor(shape["aabb"], dtype=torch.float32)
    inv = (2.0 / (a[1] - a[0])).numpy()
    f, g, Af, A = G.density_grad(P, xn.detach(), inv, grid)
    want_g = want_dn * torch.from_numpy(inv).double()      # d(normalised) / d(world) = inv_aabb_size
    assert float((f - want_f.detach()).abs().max()) <= 1e-12 * float(Af.max())
    assert float(((g - want_g).abs() / A).max()) <= 1e-12
    assert float(g.abs().max()) > 1.0                       # (not a comparison of zeros)


def test_gradient_is_one_sided_at_faces_and_zero_on_the_upper_face():
    grid = TINY["grid"]
    P = G.params64_of(synth.make_field_params(3, grid, density_scale=0.9, aabb=TINY["aabb"]))
    inv = np.ones(3, np.float32)
    # x exactly on node 5 (float32: 2 * 5 / 23 - 1 lands on it or an ulp beside it): the gradient is that of the cell floor() picks
    x = np.float32(2.0) * np.float32(5) / np.float32(23) - np.float32(1.0)
    p = torch.tensor([[x, 0.1, 0.2]], dtype=torch.float32)
    cell = int(torch.floor(((p[0, 0] + 1) / 2) * 23))
    inside = torch.tensor([[2.0 * (cell + 0.5) / 23 - 1.0, 0.1, 0.2]], dtype=torch.float64)
    gx = G.density_grad(P, p, inv, grid)[1][0, 0]
    # same cell, same y / z taps (float32 and float64 coordinates of 0.1 / 0.2 differ by 1e-8: the x derivative moves by 1e-7 relative)
    assert abs(float(gx - G.density_grad(P, inside, inv, grid)[1][0, 0])) <= 1e-6 * abs(float(gx))
    up = torch.tensor([[1.0, 0.1, 0.2], [0.3, 1.0, 0.2], [0.3, 0.1, 1.0]], dtype=torch.float32)
    g = G.density_grad(P, up, inv, grid)[1]
    assert [float(g[a, a]) for a in range(3)] == [0.0, 0.0, 0.0]


def test_ray_level_claims(refs, pool):
    for (kind, N), ref in refs.items():
        ln = np.linalg.norm(ref.normal, axis=-1)
        assert np.all(ln <= ref.acc + 1e-12), (kind, N)
        dead = ref.nvalid == 0
        assert dead.sum() >= 4 and np.all(ref.acc[dead] == 0) and np.all(ref.var[dead] == 0) and np.all(ref.normal[dead] == 0)
        assert np.all(ref.median(0.5, MISS)[0][ref.acc < 0.5] == MISS)
        if N == 1:
            assert np.all(ref.acc == 0)            # the last interval is 0: one sample has no weight at all
            continue
        # monotone and continuous in the quantile: no jump where the crossing sample changes
        taus = np.linspace(0.01, 0.99, 197)
        meds = np.stack([ref.median(t, 1e30)[0] for t in taus])      # (a ray that runs out of weight jumps to miss_depth and stays)
        assert np.all(np.diff(meds, axis=0) >= -1e-12), (kind, N)
        for r in np.nonzero(ref.acc > 0.3)[0]:
            k = int(np.nonzero(ref.cum[r] >= 0.2)[0][0])
            c = ref.cum[r, k]                       # tau crossing from sample k to the next one with weight
            if c + 1e-9 < ref.acc[r]:
                below, above = ref.median(c - 1e-12, MISS)[0][r], ref.median(c + 1e-12, MISS)[0][r]
                nxt = k + 1 + int(np.nonzero(ref.w[r, k + 1:] > 0)[0][0])
                # the mass of k ends at z_k + dist_k; the next sample with weight starts at its own z (equal when adjacent)
                slope = ref.dist[r, nxt] / ref.w[r, nxt]          # d median / d tau inside sample nxt
                assert abs(below - (ref.z[r, k] + ref.dist[r, k])) <= 1e-9 and abs(above - ref.z[r, nxt]) <= 2e-12 * slope + 1e-9
                if nxt == k + 1:
                    assert abs(above - below) <= 2e-12 * slope + 1e-6    # (z_k + dist_k is z_{k+1} up to the float32 subtraction)
    assert (refs[("mask", 65)].nvalid < refs[("plain", 65)].nvalid).any(), "the mask drops samples of these rays"


@pytest.mark.parametrize("kind", G.KINDS)
def test_bounds_are_informative(cases, refs, fine_refs, pool, kind):
    """In every case at least 90 % of the rays with acc >= 0.6 have a median interval narrower than a tenth of the step, a normal
    bound below 1e-2 and a variance bound below 10 % of Var + 1e-6; and the condition speaks of many rays: ten of the pool's 22, at
    least two in every batch window of three rays or more, the single ray of R = 1, and five of the nine long rays."""
    for N in G.NS:
        for tau in G.TAUS:
            share, n = refs[(kind, N)].informative(tau, MISS)
            print(f"{kind} N={N} tau={tau}: {share:.2f} of {n} rays")
            assert share >= 0.9, (kind, N, tau, share, n)
            assert n >= 10 or N == 1, (kind, N, n)
        if N > 1:
            opaque = refs[(kind, N)].acc >= 0.6
            for R, b in G.BATCHES.items():
                assert opaque[b:b + R].sum() >= min(R, 2), (kind, N, R)
    for N in G.FINE_NS:
        for tau in G.TAUS:
            share, n = fine_refs[(kind, N)].informative(tau, MISS)
            print(f"{kind} fine N={N} tau={tau}: {share:.2f} of {n} rays")
            assert share >= 0.9, (kind, N, tau, share, n)
            assert n >= (5 if N >= 128 else 1), (kind, N, n)


@pytest.mark.parametrize("kind", G.KINDS)
def test_fine_windows_span_blocks(fine_refs, kind):
    """What the long rays are for: windows on either side of the 64-sample block edges, windows of three blocks, and opaque rays
    whose quantile is crossed in the second and in the third block of the window (the carries of the transmittance and of the
    cumulative weight, the latch of the first crossing); every window of more than 64 samples takes the wide form of the
    validity-interval search, whose conservative range holds the window."""
    for N in (64, 65, 128, 129):
        assert (fine_refs[(kind, N)].Lw == N).sum() >= 3, (kind, N)          # rays whose window begins at sample 0
    ref = fine_refs[(kind, 200)]
    assert (ref.Lw > 64).sum() >= 6 and (ref.Lw > 128).sum() >= 5 and (ref.Lw > 192).sum() >= 1, ref.Lw.tolist()
    assert ((ref.Lw > 0) & (ref.Lw <= 64)).any() and (ref.Lw == 0).any()
    assert (ref.first > 0).any() and (ref.first == 0).any()
    blocks = set()
    for tau in G.TAUS:
        ks = ref.median(tau, MISS)[1]
        hit = (ks >= 0) & (ref.acc >= 0.6)
        blocks |= set(((ks - ref.first)[hit] // 64).tolist())
    assert {0, 1, 2} <= blocks, blocks


# ---- mutation tests of the checkers ------------------------------------------------------------------------------------------------
def _pointwise(mutate):
    grid = G.GRID37["grid"]
    P = G.params64_of(synth.make_field_params(4, grid, density_scale=0.9, aabb=G.GRID37["aabb"]))
    xn = torch.from_numpy(G.points(grid))
    a = torch.tensor(G.GRID37["aabb"], dtype=torch.float32)
    inv = (2.0 / (a[1] - a[0])).numpy()
    _, want, _, A = G.density_grad(P, xn, inv, grid)
    got = G.density_grad(P, xn, inv, grid, mutate=mutate)[1]
    return G.pointwise_ratio(got.numpy().astype(np.float32), want, A)


def test_pointwise_checker_accepts_the_rounded_reference():
    assert _pointwise(None) <= 1.0 / (G.M_GRAD + 2)       # float32 rounding of the exact value: half an ulp


@pytest.mark.parametrize("mutate", ["swap_axis", "drop_line"])
def test_pointwise_checker_catches(mutate):
    assert _pointwise(mutate) > 1.0


def test_ray_checkers_accept_the_reference_and_catch_mutations(cases, refs, fine_refs, pool):
    cfg, P = cases["plain"]
    ref = refs[("plain", 65)]
    f32 = lambda x: np.asarray(x, np.float32)            # noqa: E731
    for tau in G.TAUS:
        assert ref.check_median(f32(ref.median(tau, MISS)[0]), tau, MISS).size == 0
    assert ref.check_var(f32(ref.var)).size == 0 and ref.check_normal(f32(ref.normal)).size == 0
    assert ref.check_acc_depth(f32(ref.acc), f32(ref.depth)).size == 0
    scaled = G.RayRef(cfg, P, pool, 65, mutate="scaled_dist_median")
    assert ref.check_median(f32(scaled.median(0.5, MISS)[0]), 0.5, MISS).size > 0
    mean = G.RayRef(cfg, P, pool, 65, mutate="var_about_mean")
    assert ref.check_var(f32(mean.var)).size > 0
    swapped = G.RayRef(cfg, P, pool, 65, mutate="swap_axis")
    assert ref.check_normal(f32(swapped.normal)).size > 0
    dropped = G.RayRef(cfg, P, pool, 65, mutate="drop_line")
    assert ref.check_normal(f32(dropped.normal)).size > 0
    # a forgotten carry across the 64-sample blocks: caught on the long rays wherever a later block holds weight, and only there (at
    # N = 65 the second block of a window that begins at sample 0 is the ray's last sample, whose interval and weight are 0)
    fcfg = G.make_cfg(TINY, step_ratio=G.FINE_RATIO)
    for N in (128, 129, 200):
        fine = fine_refs[("plain", N)]
        nocarry = G.RayRef(fcfg, P, G.fine_rays(), N, mutate="drop_carry")
        assert fine.check_acc_depth(f32(nocarry.acc), f32(nocarry.depth)).size > 0, N
        assert fine.check_var(f32(nocarry.var)).size > 0 and fine.check_normal(f32(nocarry.normal)).size > 0, N
        noccum = G.RayRef(fcfg, P, G.fine_rays(), N, mutate="drop_ccum")
        if N >= 128:
            assert any(fine.check_median(f32(noccum.median(tau, MISS)[0]), tau, MISS).size > 0 for tau in G.TAUS), N
    short = G.RayRef(cfg, P, pool, 130, mutate="drop_carry")
    assert refs[("plain", 130)].check_acc_depth(f32(short.acc), f32(short.depth)).size == 0, "one block: no carry to forget"
    # a median handed to a ray that must miss, and the other way round
    wrong = f32(ref.median(0.5, MISS)[0])
    r = int(np.nonzero(ref.acc < 0.5 - ref.delta)[0][0])
    wrong[r] = 3.0
    assert r in ref.check_median(wrong, 0.5, MISS)
    wrong = f32(ref.median(0.5, MISS)[0])
    r = int(np.nonzero(ref.acc > 0.5 + ref.delta)[0][0])
    wrong[r] = MISS
    assert r in ref.check_median(wrong, 0.5, MISS)
