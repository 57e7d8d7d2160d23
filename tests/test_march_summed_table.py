"""The tile marcher's summed density table (t2n_march_tiles.hip: table_sum / table_read3): per step pair the three pair tables
D_k = P_k L_k^T are added into ONE 4 x 4 x 4 table S[z][y][x] and every sample interpolates its eight corners from it.

Every test first restates on the CPU, from the rays and the grid alone, which step pairs of which 8 x 8 tiles take the table path (the
kernel's rule: the low taps of both steps of all live lanes span at most 3 indices per axis, + 1 for the high tap) and asserts the share
its case needs: a frame that silently fell back to direct gathers would pass every comparison below without running the code under
test. The restatement is fp32 numpy, one rounding per operation like the kernels (they are compiled without FMA contraction).

Bounds: those of tests/test_hip_parity.py::test_tile_marcher_matches_per_ray_marcher against the per-ray marcher (the two differ by
the order of fp32 additions only), RGB_ATOL / DEPTH_ATOL against oracle_c."""
import numpy as np
import pytest
import torch

from text2nerf_amd import synth
from tests.test_hip_parity import DEPTH_ATOL, RGB_ATOL, close, dev, make_field

pytestmark = pytest.mark.gpu

F32 = np.float32
Z_GATE = F32(2.0)          # models/tensorBase.py:460
GRID = [41, 23, 35]


def host_scalars(aabb, grid, step_ratio=1.0):
    """update_stepSize (models/tensorBase.py:220-231) in fp32: (inverse half extents, step size)."""
    a = np.asarray(aabb, F32)
    size = a[1] - a[0]
    units = size / (np.asarray(grid, F32) - F32(1))
    step = torch.mean(torch.from_numpy(units)).numpy() * F32(step_ratio)
    return (F32(2.0) / size).astype(F32), F32(step)


def pinhole_rays(H, W, focal, c2w):
    """synth.frame_rays_np with a focal length of its own choosing."""
    d = synth.ray_directions_np(H, W, focal, focal, W // 2, H // 2).reshape(-1, 3)
    c2w = np.asarray(c2w, F32)[:3]
    rd = (d @ c2w[:, :3].T).astype(F32)
    return np.concatenate([np.broadcast_to(c2w[:, 3], rd.shape).astype(F32), rd], 1).astype(F32)


def sample_taps(rays, aabb, grid, near_far, N):
    """Per ray and sample index: validity (box test, z gate, inside the ray's conservative interval) and the low tap index per axis
    (t2n_device.h: ray_tmin, ray_interval, sample_z, sample_point, axis_taps_inbox), plus the rays' intervals [lo, hi]."""
    a = np.asarray(aabb, F32)
    inv, step = host_scalars(aabb, grid)
    near, far = F32(near_far[0]), F32(near_far[1])
    o, d = rays[:, :3].astype(F32), rays[:, 3:6].astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(d == 0, F32(1e-6), d)
        t = np.minimum((a[1] - o) / v, (a[0] - o) / v).max(1)
        tmin = np.minimum(np.maximum(t, near), far).astype(F32)
        ta, tb = (a[0] - o) / d, (a[1] - o) / d
        assert np.all(d != 0)
        t0, t1 = np.minimum(ta, tb).max(1), np.maximum(ta, tb).min(1)
        tg = (Z_GATE - o[:, 2]) / d[:, 2]
        t0 = np.where(d[:, 2] > 0, np.maximum(t0, tg), t0)
        t1 = np.where(d[:, 2] > 0, t1, np.minimum(t1, tg))
        flo = np.floor((t0 - tmin) / step) - F32(3)
        fhi = np.ceil((t1 - tmin) / step) + F32(3)
    lo = np.minimum(np.maximum(flo, F32(0)), F32(N)).astype(np.int64)
    hi = np.minimum(np.maximum(fhi, F32(-1)), F32(N - 1)).astype(np.int64)
    none = ~(t1 >= t0)
    lo[none], hi[none] = N, -1
    idx = np.arange(N)
    z = (tmin[:, None] + step * idx.astype(F32)[None, :]).astype(F32)
    p = (o[:, None, :] + (d[:, None, :] * z[:, :, None]).astype(F32)).astype(F32)
    ok = np.all((p >= a[0]) & (p <= a[1]), -1) & (p[..., 2] > Z_GATE)
    ok &= (idx[None, :] >= lo[:, None]) & (idx[None, :] <= hi[:, None])
    g = (((p - a[0]).astype(F32) * inv).astype(F32) - F32(1)).astype(F32)
    ix = (((g + F32(1)) / F32(2)).astype(F32) * (np.asarray(grid, F32) - F32(1))).astype(F32)
    return ok, np.floor(ix).astype(np.int64), lo, hi


def step_pairs(rays, H, W, aabb, grid, near_far, N, dense):
    """One record per step pair of every 8 x 8 tile that has a live sample: (table path?, amn[3], highest low tap[3]). `dense`: the
    weights-writing instantiation starts its pairs at a multiple of 16, the other one at the tile's first candidate sample."""
    ok, i0, lo, hi = sample_taps(rays, aabb, grid, near_far, N)
    out = []
    for ty in range((H + 7) // 8):
        for tx in range((W + 7) // 8):
            py, px = np.meshgrid(np.arange(ty * 8, min(ty * 8 + 8, H)), np.arange(tx * 8, min(tx * 8 + 8, W)), indexing="ij")
            r = (py * W + px).reshape(-1)
            wlo, whi = int(lo[r].min()), int(hi[r].max())
            b, e = (wlo & ~15, min(N - 1, whi | 15)) if dense else (wlo, whi)
            for i in range(b, e + 1, 2):
                m = ok[r, i:min(i + 2, e + 1)]
                if not m.any():
                    continue
                t = i0[r, i:min(i + 2, e + 1)][m]
                mn, mx = t.min(0), t.max(0)
                out.append((bool((mx - mn).max() + 2 <= 4), mn, mx))
    return out


def table_share(pairs):
    return sum(1 for p in pairs if p[0]) / max(1, len(pairs))


def render_modes(f, rays, W, N):
    """(per-ray marcher, tile marcher with weights rows, tile marcher without) and their sample counters."""
    out, st = [], []
    with torch.no_grad():
        for fw, mat in ((0, True), (W, True), (W, False)):
            f.frame_width, f.materialize_weights = fw, mat
            out.append(f(rays, N_samples=N))
            st.append(f.stats())
    f.frame_width, f.materialize_weights = 0, True
    return out, st


def check_against_per_ray(out, st, min_app, modes_bit_equal=True):
    """`modes_bit_equal`: the two output modes pair the steps differently (see step_pairs); where every pair of both pairings is on
    the table path their arithmetic is the same, sample by sample. A pair that gathers in one mode only is not."""
    (a, b, c), (sa, sb, sc) = out, st
    assert sa["evaluated"] == sb["evaluated"] == sc["evaluated"] and sa["evaluated"] > 0
    assert abs(sa["appearance"] - sb["appearance"]) <= 2 and sb["appearance"] == sc["appearance"]
    assert sa["appearance"] >= min_app, f"only {sa['appearance']} samples above the weight threshold"
    assert torch.equal(a[2], b[2])                                   # z_vals
    close(b[3], a[3].cpu().numpy(), atol=2e-6, rtol=2e-5)            # weights
    for o in (b, c):
        close(o[0], a[0].cpu().numpy(), atol=2e-5)
        close(o[1], a[1].cpu().numpy(), atol=5e-5)
    print(f"the two output modes: max |rgb difference| {float((b[0] - c[0]).abs().max()):.2e}, max |depth difference| "
          f"{float((b[1] - c[1]).abs().max()):.2e}")
    if modes_bit_equal:
        assert torch.equal(b[0], c[0]) and torch.equal(b[1], c[1])


def check_against_oracle_c(params, aabb, grid, near_far, rays_np, N, out):
    from oracle import oracle_torch as O
    from oracle.oracle_c import COracle
    co = COracle(O.FieldConfig(aabb=aabb, grid_size=grid, near_far=near_far), params)
    o_rgb, o_depth, _, _ = co.render(rays_np, n_samples=N, want_weights=False)
    for o in out[1:]:
        close(o[0], o_rgb, atol=RGB_ATOL)
        close(o[1], o_depth, atol=DEPTH_ATOL)


# ---- the anisotropic field of tests 1-3: three different grid sizes, three different extents, camera inside the box ------------------
AABB = [[-5.0, -3.5, -1.0], [6.0, 4.0, 9.5]]
NEAR_FAR = [0.5, 12.0]
N_SAMPLES = 120


@pytest.fixture(scope="module")
def aniso():
    params = synth.make_field_params(5, GRID, density_scale=0.8, aabb=AABB)
    return params, make_field(params, GRID, AABB, NEAR_FAR)


@pytest.mark.parametrize("H,W", [(64, 72), (37, 53)])
def test_index_mapping(aniso, H, W):
    """Random factors on a 41 x 23 x 35 grid in a non-cubic box: S[z][y][x] must take pair 0's entry at [z][(y, x)], pair 1's at
    [y][(z, x)] and pair 2's at [x][(z, y)] — any swapped axis changes every sample's density (a cubic, symmetric scene could hide
    it). Whole and ragged tiles, both output modes, against the per-ray marcher and oracle_c."""
    params, f = aniso
    rays_np = pinhole_rays(H, W, 4.0 * max(H, W), synth.look_pose(0.25, -0.15, (0.3, 0.2, 0.4)))
    for dense in (False, True):
        share = table_share(step_pairs(rays_np, H, W, AABB, GRID, NEAR_FAR, N_SAMPLES, dense))
        print(f"{H}x{W}, weights rows {dense}: {share:.3f} of the step pairs on the table path")
        assert share >= 0.9
        assert share == 1.0      # (this camera: needed for the bit-equality of the two output modes, see check_against_per_ray)
    out, st = render_modes(f, torch.from_numpy(rays_np).to(dev()), W, N_SAMPLES)
    check_against_per_ray(out, st, min_app=300)
    check_against_oracle_c(params, AABB, GRID, NEAR_FAR, rays_np, N_SAMPLES, out)


# ---- box faces ------------------------------------------------------------------------------------------------------------------------
CORNER_NEAR_FAR = [0.5, 14.0]
CORNER_SIZE = (8.0, 8.0, 16.0)


def corner_scene(H=32, W=32, N=N_SAMPLES):
    """Camera at the origin, inside the box, looking at the box's (+x, +y, +z) corner: every ray leaves through one of the three
    faces there. A sample lies in the LAST cell of an axis (low tap = size - 1, high tap clamped, weight 0) only when it sits on the
    face itself, so each face is put exactly through one sample: with the origin at 0 a sample's coordinate is the single product
    d * z, the face takes that value, and the box keeps a power-of-two extent — position - aabb_min, the scaling by 2 / extent and the
    unnormalisation are then exact and the sample's cell index is size - 1 whatever the rounding elsewhere. The sample distances do
    not move with the faces (t_min is `near` for a camera inside, the step depends on the extents only)."""
    rays = pinhole_rays(H, W, 12.0 * max(H, W), synth.look_pose(0.5248, -0.4046, (0.0, 0.0, 0.0)))
    hi = np.asarray((5.5, 4.7, 9.5), F32)
    size = np.asarray(CORNER_SIZE, F32)
    _, step = host_scalars([list(hi - size), list(hi)], GRID)
    z = (F32(CORNER_NEAR_FAR[0]) + step * np.arange(N, dtype=F32)).astype(F32)
    d = rays[:, 3:6]
    t_exit = hi[None, :] / d
    face = hi.copy()
    for a in range(3):      # the ray that leaves through face a with the widest margin to the other two; its last sample in front of it
        r = int(np.argmax(np.delete(t_exit, a, 1).min(1) - t_exit[:, a]))
        p = (d[r, a] * z).astype(F32)
        face[a] = p[np.nonzero(p <= hi[a])[0].max()]
    aabb = [[float(F32(face[a] - size[a])) for a in range(3)], [float(face[a]) for a in range(3)]]
    assert all(F32(aabb[1][a]) - F32(aabb[0][a]) == size[a] for a in range(3))
    return aabb, rays


def test_box_faces():
    """The clamped high tap read at low + 1 (weight 0, a finite entry) and boxes that end on the grid's last texel: samples in the last
    cell of an axis on table-path pairs, and table-path pairs whose fourth tap IS the last texel."""
    H = W = 32
    aabb, rays_np = corner_scene(H, W)
    for dense in (False, True):
        pairs = step_pairs(rays_np, H, W, aabb, GRID, CORNER_NEAR_FAR, N_SAMPLES, dense)
        edge = sum(1 for t, mn, mx in pairs if t and any(mn[a] + 3 == GRID[a] - 1 for a in range(3)))
        last = sum(1 for t, mn, mx in pairs if t and any(mx[a] == GRID[a] - 1 for a in range(3)))
        print(f"weights rows {dense}: {len(pairs)} step pairs, {table_share(pairs):.3f} on the table path, {edge} of them with amn + 3 == "
              f"size - 1, {last} with a sample in the last cell of an axis")
        assert edge >= 1 and last >= 1
        assert table_share(pairs) == 1.0      # (for the bit-equality of the two output modes)
    params = synth.make_field_params(6, GRID, density_scale=0.8, aabb=aabb)
    f = make_field(params, GRID, aabb, CORNER_NEAR_FAR)
    out, st = render_modes(f, torch.from_numpy(rays_np).to(dev()), W, N_SAMPLES)
    check_against_per_ray(out, st, min_app=100)
    check_against_oracle_c(params, aabb, GRID, CORNER_NEAR_FAR, rays_np, N_SAMPLES, out)


# ---- independence of the tile grouping ------------------------------------------------------------------------------------------------
def test_tile_grouping_does_not_change_a_ray(aniso):
    """A table entry is a function of its texel alone (not of the box origin) and a sample's eight reads and ten multiply-adds come in a
    fixed order, so a ray renders to the same bits whichever 63 rays share its tile: columns 4..67 of a 72-wide frame as a frame of
    their own shift every tile by half a tile. A missing fence or a stale S entry breaks the equality."""
    params, f = aniso
    H, W = 64, 72
    full_np = pinhole_rays(H, W, 8.0 * W, synth.look_pose(0.25, -0.15, (0.3, 0.2, 0.4)))
    cols = (np.arange(H)[:, None] * W + np.arange(4, 68)[None, :]).reshape(-1)
    sub_np = np.ascontiguousarray(full_np[cols])
    for dense in (False, True):
        for rays_np, w in ((full_np, W), (sub_np, 64)):
            pairs = step_pairs(rays_np, H, w, AABB, GRID, NEAR_FAR, N_SAMPLES, dense)
            assert len(pairs) > 500 and all(p[0] for p in pairs), "a step pair of this frame gathers directly"
    idx = torch.from_numpy(cols).to(dev())
    with torch.no_grad():
        for mat in (False, True):
            f.materialize_weights = mat
            f.frame_width = W
            a = f(torch.from_numpy(full_np).to(dev()), N_samples=N_SAMPLES)
            assert f.stats()["appearance"] >= 300
            f.frame_width = 64
            b = f(torch.from_numpy(sub_np).to(dev()), N_samples=N_SAMPLES)
            assert torch.equal(a[0][idx], b[0]) and torch.equal(a[1][idx], b[1])
    f.frame_width, f.materialize_weights = 0, True


# ---- mixed paths ----------------------------------------------------------------------------------------------------------------------
def test_mixed_table_and_gather_pairs():
    """24 x 24 pixels over a 300^3 field, the camera just below the z gate: the first live samples are half a unit away, where a tile's
    taps fit the table, the last ones nearly three units, where they span more and the step pair gathers directly. Both kinds of
    step pair in one frame, about half and half, both output modes."""
    aabb, grid, nf, N = [[-8.0] * 3, [8.0] * 3], [300] * 3, [0.5, 8.0], 45
    H = W = 24
    rays_np = pinhole_rays(H, W, 100.0, synth.look_pose(-0.15, 0.1, (0.2, -0.1, 1.9)))
    for dense in (False, True):
        pairs = step_pairs(rays_np, H, W, aabb, grid, nf, N, dense)
        n_table = sum(1 for p in pairs if p[0])
        print(f"weights rows {dense}: {n_table} table-path and {len(pairs) - n_table} gather step pairs")
        assert n_table >= 50 and len(pairs) - n_table >= 50
    f = make_field(synth.make_field_params(7, grid, density_scale=0.8, aabb=aabb), grid, aabb, nf)
    out, st = render_modes(f, torch.from_numpy(rays_np).to(dev()), W, N)
    check_against_per_ray(out, st, min_app=100, modes_bit_equal=False)
