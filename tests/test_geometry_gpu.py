"""t2n_density_grad_at and t2n_render_geometry (csrc/t2n_geometry.hip) through the C ABI, and their Python surface, against the
float64 reference of tests/helpers/geometry_ref.py (held to grid_sample / autograd and mutation-tested in tests/test_geometry_cpu.py).

Point-wise bound, per element of grad_world: |got - want| <= gamma A, A the float64 sum of the absolute values of the element's
terms, gamma = (m + 2) 2^-24 with m = 24 float32 roundings on the kernel's longest chain (counted in geometry_ref.py, next to
M_GRAD). Every launch prints a `GEOMEW` line with the measured error / bound ratio (profiles/geometry_elementwise.txt keeps a run's).
Ray-level bounds: those of include/t2n.h's definitions at the tolerances tests/test_hip_parity.py holds the eval forward to
(W_ATOL, DEPTH_ATOL); `GEOMRAY` lines carry the measured ratios. Every buffer a kernel writes stands between guard words."""
import numpy as np
import pytest
import torch

from text2nerf_amd import _lib, synth
from text2nerf_amd._lib import T2NError
from tests.conftest import GOLDEN, TINY
from tests.helpers import geometry_ref as G
from tests.test_hip_parity import DEPTH_ATOL, W_ATOL, dev, make_field
from tests.test_optim_kernels_gpu import Buf, call, same_bits

pytestmark = pytest.mark.gpu

assert (G.T_W, G.T_D) == (W_ATOL, DEPTH_ATOL)
MISS = 7.25          # not near_far[1], not a depth any of these rays has
OUTPUTS = ("acc", "depth", "median", "var", "normal")


def nan_buf(*shape):
    return Buf(np.full(shape, np.nan, np.float32))


def geometry(m, rays, N, tau, miss=MISS, want=OUTPUTS):
    """One t2n_render_geometry call on guarded buffers; outputs not in `want` are passed as NULL."""
    h = m.sync_params()
    rays = np.ascontiguousarray(rays, np.float32)
    R = rays.shape[0]
    rb = Buf(rays)
    outs = {k: nan_buf(R, 3) if k == "normal" else nan_buf(R) for k in want}
    p = lambda k: outs[k].ptr if k in outs else None      # noqa: E731
    call("t2n_render_geometry", h, rb.ptr, R, rays.shape[1], int(N), float(tau), float(miss), p("acc"), p("depth"), p("median"), p("var"),
         p("normal"))
    torch.cuda.synchronize()
    assert same_bits(rb.get(), rays) and rb.guards_intact(), "the rays came back changed"
    assert all(b.guards_intact() for b in outs.values()), "a guard word was overwritten"
    got = {k: b.get() for k, b in outs.items()}
    assert not any(np.isnan(v).any() for v in got.values()), "an output element was not written"
    return got


def grad_at(m, pts):
    h = m.sync_params()
    n = pts.shape[0]
    xb, fb, gb, f2 = Buf(pts), nan_buf(n), nan_buf(n, 3), nan_buf(n)
    call("t2n_density_grad_at", h, xb.ptr, n, fb.ptr, gb.ptr)
    call("t2n_density_at", h, xb.ptr, n, f2.ptr, None)
    torch.cuda.synchronize()
    assert same_bits(xb.get(), pts) and all(b.guards_intact() for b in (xb, fb, gb, f2))
    f, g = fb.get(), gb.get()
    assert not np.isnan(f).any() and not np.isnan(g).any()
    assert same_bits(f, f2.get()), "feat is t2n_density_at's, bit for bit"
    # either output alone: same bits
    fo, go = nan_buf(n), nan_buf(n, 3)
    call("t2n_density_grad_at", h, xb.ptr, n, fo.ptr, None)
    call("t2n_density_grad_at", h, xb.ptr, n, None, go.ptr)
    torch.cuda.synchronize()
    assert same_bits(fo.get(), f) and same_bits(go.get(), g) and fo.guards_intact() and go.guards_intact()
    return f, g


@pytest.fixture(scope="module")
def pool():
    import os
    return G.pool_rays(np.load(os.path.join(GOLDEN, "tiny.npz"), allow_pickle=False)["tiny_rays"])


@pytest.fixture(scope="module")
def fields():
    """kind -> (field, oracle config, float64 factors) of the ray-level field (geometry_ref.RAY_SEED / RAY_SCALE)."""
    out = {}
    params = G.ray_params(TINY)
    for kind in G.KINDS:
        m = make_field(params, TINY["grid"], TINY["aabb"], TINY["near_far"])
        vol = None
        if kind == "mask":
            m.alphaMask_thres = G.MASK_THRES
            m.updateAlphaMask(G.MASK_GRID)
            v = m.alphaMask.alpha_volume
            vol = v.reshape(v.shape[-3:]).cpu()
            assert 0.02 < float(vol.mean()) < 0.98
        if kind == "bf16":
            m.factor_storage = "bf16"
        out[kind] = (m, G.make_cfg(TINY, vol), G.params64_of(params, bf16=kind == "bf16"))
    return out


@pytest.fixture(scope="module")
def fine_fields():
    """The same three fields at step_ratio FINE_RATIO (the mask is built at step_ratio 1 first, as geometry_ref.oracle_mask_volume
    builds the CPU file's): windows of up to four 64-sample blocks."""
    out = {}
    params = G.ray_params(TINY)
    for kind in G.KINDS:
        m = make_field(params, TINY["grid"], TINY["aabb"], TINY["near_far"])
        vol = None
        if kind == "mask":
            m.alphaMask_thres = G.MASK_THRES
            m.updateAlphaMask(G.MASK_GRID)
            v = m.alphaMask.alpha_volume
            vol = v.reshape(v.shape[-3:]).cpu()
        if kind == "bf16":
            m.factor_storage = "bf16"
        m.step_ratio = G.FINE_RATIO
        m.update_stepSize(TINY["grid"])
        cfg = G.make_cfg(TINY, vol, step_ratio=G.FINE_RATIO)
        assert float(m.stepSize) == np.float32(cfg.step_size)
        out[kind] = (m, cfg, G.params64_of(params, bf16=kind == "bf16"))
    return out


# ---- point-wise ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", [TINY, G.GRID37], ids=["tiny", "37x23x29"])
def test_density_grad_at_elementwise(shape, storage):
    """m = 24 (geometry_ref.M_GRAD): |got - want| <= 26 x 2^-24 x A per element of grad_world, at n = 1, 63, 64, 65, 257 points that
    hold the exact upper and lower box faces, grid nodes (cell faces), an axis-aligned line and interior points; feat bit-equal to
    t2n_density_at; under bf16 storage against the reference on the bf16-rounded factors."""
    grid = shape["grid"]
    params = synth.make_field_params(4, grid, density_scale=0.9, aabb=shape["aabb"])
    m = make_field(params, grid, shape["aabb"], shape["near_far"])
    m.factor_storage = storage
    P = G.params64_of(params, bf16=storage == "bf16")
    inv = m.invaabbSize.detach().float().cpu().numpy()
    pts = G.points(grid)
    for n in G.POINT_NS:
        f, g = grad_at(m, pts[:n])
        wf, wg, Af, A = G.density_grad(P, torch.from_numpy(pts[:n]), inv, grid)
        rf, rg = G.pointwise_ratio(f, wf, Af, G.GAMMA_F), G.pointwise_ratio(g, wg, A)
        print(f"GEOMEW {'x'.join(map(str, grid))} {storage} n={n}: grad err/bound {rg:.3f}, feat err/bound {rf:.3f}")
        assert rg <= 1.0 and rf <= 1.0, (n, rg, rf)
    up = np.nonzero(pts == 1.0)
    assert up[0].size >= 5 and np.all(g[up] == 0.0), "0 along an axis on its exact upper face"
    assert float(np.abs(g).max()) > 1.0


# ---- analytic fields ----------------------------------------------------------------------------------------------------------------
def ramp_params(axis):
    """All density factors zero except component 0 of pair 0 (plane x-y, line z). axis 2: the plane constant 1, the line a linear
    ramp 0 -> 11 along z (f rises with z: the normal is -z). axis 0: the plane a ramp 11 -> 2 along x, the line constant 1 (f falls
    with x: the normal is +x)."""
    params = synth.make_field_params(2, TINY["grid"], density_scale=0.9, aabb=TINY["aabb"])
    for k, v in params.items():
        if k.startswith("density_"):
            v[...] = 0.0
    gx, gy, gz = TINY["grid"]
    if axis == 2:
        params["density_plane.0"][0, 0] = 1.0
        params["density_line.0"][0, 0, :, 0] = np.linspace(0.0, 11.0, gz, dtype=np.float32)
    else:
        params["density_plane.0"][0, 0] = np.linspace(11.0, 2.0, gx, dtype=np.float32)[None, :]
        params["density_line.0"][0, 0, :, 0] = 1.0
    return params


@pytest.mark.parametrize("axis,sign", [(2, -1.0), (0, 1.0)], ids=["line-ramp-z", "plane-ramp-x"])
def test_analytic_ramp(pool, axis, sign):
    params = ramp_params(axis)
    m = make_field(params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    others = [a for a in range(3) if a != axis]
    _, g = grad_at(m, G.points(TINY["grid"]))
    assert np.all(g[:, others] == 0.0), "the other two components of grad_world are exactly 0"
    assert np.all(sign * g[:, axis] <= 0.0) and np.any(g[:, axis] != 0.0)
    N, tau = 65, 0.5
    got = geometry(m, pool, N, tau)
    ref = G.RayRef(G.make_cfg(TINY), G.params64_of(params), pool, N)
    assert np.all(got["normal"][:, others] == 0.0), "the other two components of the normal are exactly 0"
    acc = got["acc"].astype(np.float64)
    off = np.abs(got["normal"][:, axis].astype(np.float64) - sign * acc)
    assert (acc > 0.5).sum() >= 5 and np.all(off <= 2 * G.ulp32(acc)), float((off / G.ulp32(acc)).max())
    want, ks = ref.median(tau, MISS)
    hit = ks >= 0
    assert hit.sum() >= 5 and ref.check_acc_depth(got["acc"], got["depth"]).size == 0
    idx = np.arange(ref.R)[hit]
    zk, dk = ref.z[idx, ks[hit]], ref.dist[idx, ks[hit]]
    med = got["median"][hit].astype(np.float64)
    assert np.all((med >= zk) & (med <= zk + dk)), "depth_median lies in the interval of the crossing sample"
    assert np.all(got["median"][ref.acc < tau - ref.delta] == np.float32(MISS))


# ---- ray level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", G.NS)
@pytest.mark.parametrize("kind", G.KINDS)
def test_render_geometry_against_float64(fields, pool, kind, N):
    """R = 1, 3, 4, 5, 9 (windows of the 22-ray pool) x tau = 0.1, 0.5, 0.9 at this N, on the plain / masked / bf16 field."""
    against_float64(fields[kind], [G.batch(pool, R) for R in G.BATCHES], N, kind)


@pytest.mark.parametrize("N", G.FINE_NS)
@pytest.mark.parametrize("kind", G.KINDS)
def test_render_geometry_multiblock_against_float64(fine_fields, kind, N):
    """The block loop run more than once: the nine long rays of geometry_ref.fine_rays at a tenth of the step, R = 1, 3, 4, 5, 9 x
    tau = 0.1, 0.5, 0.9, at N on either side of the window's own block edges (64, 65, 128, 129) and at 200 (three and four blocks;
    the quantile crossed in the first, second and third block: tests/test_geometry_cpu.py::test_fine_windows_span_blocks). The same
    bounds as at one block; the CPU file shows that a forgotten transmittance or cumulative-weight carry breaks them."""
    against_float64(fine_fields[kind], [G.fine_batch(G.fine_rays(), R) for R in G.FINE_BATCHES], N, kind + " fine")


def against_float64(field, batches, N, kind):
    m, cfg, P = field
    worst = dict(acc=0.0, depth=0.0, var=0.0, normal=0.0)
    for rays in batches:
        R = rays.shape[0]
        ref = G.RayRef(cfg, P, rays, N)
        for tau in G.TAUS:
            got = geometry(m, rays, N, tau)
            tag = (kind, N, R, tau)
            assert ref.check_acc_depth(got["acc"], got["depth"]).size == 0, tag
            bad = ref.check_median(got["median"], tau, MISS)
            assert bad.size == 0, (tag, bad.tolist(), got["median"][bad].tolist(), ref.median(tau, MISS)[0][bad].tolist())
            bad = ref.check_var(got["var"])
            assert bad.size == 0, (tag, bad.tolist(), got["var"][bad].tolist(), ref.var[bad].tolist(), ref.var_bound[bad].tolist())
            bad = ref.check_normal(got["normal"])
            assert bad.size == 0, (tag, bad.tolist(), got["normal"][bad].tolist(), ref.normal[bad].tolist())
            worst["acc"] = max(worst["acc"], float(np.abs(got["acc"] - ref.acc).max() / (N * G.T_W)))
            worst["depth"] = max(worst["depth"], float(np.abs(got["depth"] - ref.depth).max() / G.T_D))
            live = ref.nvalid > 0
            if live.any():
                worst["var"] = max(worst["var"], float((np.abs(got["var"] - ref.var)[live] / ref.var_bound[live]).max()))
                worst["normal"] = max(worst["normal"], float((np.abs(got["normal"] - ref.normal)[live] / ref.normal_bound[live, None]).max()))
            # rays without a valid sample: exact
            dead = ~live
            assert np.all(got["acc"][dead] == 0) and np.all(got["var"][dead] == 0) and np.all(got["normal"][dead] == 0), tag
            assert np.all(got["median"][dead] == np.float32(MISS)) and same_bits(got["depth"][dead], rays[dead, -1]), tag
            if N == 1:
                assert np.all(got["acc"] == 0) and np.all(got["median"] == np.float32(MISS)), "one sample has no weight at all"
    print(f"GEOMRAY {kind} N={N}: err/bound acc {worst['acc']:.3f} depth {worst['depth']:.3f} var {worst['var']:.3f} normal {worst['normal']:.3f}")


@pytest.mark.parametrize("kind", G.KINDS)
def test_render_geometry_is_reproducible_and_per_ray(fields, pool, kind):
    exactness(fields[kind][0], G.batch(pool, 9), 130, 0.5)


@pytest.mark.parametrize("tau", [0.5, 0.9])
@pytest.mark.parametrize("kind", G.KINDS)
def test_multiblock_is_reproducible_and_per_ray(fine_fields, kind, tau):
    """The same exactness on windows of up to four blocks (N = 200, the nine long rays)."""
    exactness(fine_fields[kind][0], G.fine_rays(), 200, tau)


def exactness(m, rays, N, tau):
    a = geometry(m, rays, N, tau)
    b = geometry(m, rays, N, tau)
    assert all(same_bits(a[k], b[k]) for k in OUTPUTS), "two calls give the same bits"
    for k in OUTPUTS:            # an output asked for alone (the others NULL) is the one asked for with the others
        alone = geometry(m, rays, N, tau, want=(k,))
        assert list(alone) == [k] and same_bits(alone[k], a[k]), k
    for r in range(9):           # ray r of the batch of 9 is ray r alone
        one = geometry(m, rays[r:r + 1], N, tau)
        assert all(same_bits(one[k], a[k][r:r + 1]) for k in OUTPUTS), r
    wide = np.concatenate([rays, np.full((9, 3), 0.5, np.float32)], 1)      # ray_stride 9: the LAST channel feeds the background term
    c = geometry(m, wide, N, tau)
    assert all(same_bits(c[k], a[k]) for k in ("acc", "median", "normal"))
    dead = a["acc"] == 0
    assert dead.any() and np.all(c["depth"][dead] == 0.5)


# ---- Python surface -------------------------------------------------------------------------------------------------------------------
def test_python_render_geometry_is_the_c_call(fields, pool):
    m, _, _ = fields["plain"]
    rays = G.batch(pool, 9)
    N = m.nSamples
    want = geometry(m, rays, N, 0.3, miss=TINY["near_far"][1])
    g = m.render_geometry(torch.from_numpy(rays).to(dev()), quantile=0.3)
    assert type(g).__name__ == "Geometry" and g._fields == ("acc", "depth", "depth_median", "depth_var", "normal")
    for k, t in zip(OUTPUTS, g):
        assert t.is_cuda and same_bits(t.cpu().numpy(), want[k]), k
    g = m.render_geometry(torch.from_numpy(rays).to(dev()), N_samples=64, quantile=0.3, miss_depth=MISS, want=("median",))
    assert g.depth is None and g.depth_var is None and g.normal is None
    assert same_bits(g.depth_median.cpu().numpy(), geometry(m, rays, 64, 0.3)["median"])
    g = m.render_geometry(torch.empty(0, 6, device=dev()))
    assert g.acc.shape == (0,) and g.normal.shape == (0, 3)
    xyz = torch.tensor([[0.5, -1.0, 3.0], [7.0, 6.0, 6.0], [-2.0, 3.5, 2.5]], device=dev())
    f, grad = m.density_gradient(xyz)
    wf, wg = grad_at(m, m.normalize_coord(xyz).cpu().numpy())
    assert f.shape == (3,) and grad.shape == (3, 3) and same_bits(f.cpu().numpy(), wf) and same_bits(grad.cpu().numpy(), wg)
    assert torch.equal(f, m.compute_densityfeature(m.normalize_coord(xyz)))


def test_render_geometry_views(fields):
    from text2nerf_amd import generate_rays, render_geometry_views, render_views
    m, _, _ = fields["plain"]
    H, W = 12, 16
    poses = [synth.look_pose(0.2, -0.1, (0.2, 0.1, -1.0)), synth.look_pose(-0.3, 0.15, (-0.5, 0.3, -0.5))]
    intr = [16.0, 16.0, 8.0, 6.0]
    world = render_geometry_views(m, poses, intr, H, W, quantile=0.4, camera_space=False)
    cam = render_geometry_views(m, poses, intr, H, W, quantile=0.4)
    assert world.depth.shape == (2, H, W) and world.normal.shape == (2, H, W, 3) and world.acc.shape == (2, H, W)
    for v, c2w in enumerate(poses):
        g = m.render_geometry(generate_rays(H, W, intr, c2w, device=dev()), quantile=0.4)
        for got, want in zip(world, g):
            assert torch.equal(got[v].reshape(want.shape), want)
        rot = torch.from_numpy(np.asarray(c2w, np.float32)[:3, :3]).to(dev())
        assert torch.equal(cam.normal[v].reshape(-1, 3), g.normal @ rot)
        assert torch.equal(cam.depth_median[v], world.depth_median[v])
    depth = render_views(m, poses, intr, H, W)[1]
    assert float((depth - world.depth).abs().max()) <= DEPTH_ATOL
    assert float(world.acc.max()) > 0.6 and float(world.normal.abs().max()) > 0.3


def test_export_mesh_field_normals(fields):
    from text2nerf_amd import marching_cubes
    m, _, _ = fields["plain"]
    vol = m.export_mesh(level=0.005, normals=True)
    fld = m.export_mesh(level=0.005, normals="field")
    assert vol.verts.shape[0] > 100
    assert torch.equal(fld.verts, vol.verts) and torch.equal(fld.faces, vol.faces) and torch.equal(fld.colors, vol.colors)
    g = m.density_gradient(fld.verts)[1]
    g64 = g.double()
    want = -g64 / g64.norm(dim=-1, keepdim=True).clamp_min(float(torch.finfo(torch.float32).tiny))
    # the float32 normalisation: the scaling by the largest component, three squares and two sums, the root, the division (7 roundings)
    assert float((fld.normals.double() - want).abs().max()) <= 8 * 2.0 ** -24 and not torch.equal(fld.normals, vol.normals)
    ln = fld.normals.norm(dim=-1)
    assert bool(((ln - 1).abs() <= 1e-6).logical_or(ln == 0).all())
    # normals=True is what it was: marching_cubes called directly
    grid = [int(x) for x in m.gridSize]
    alpha, _ = m.getDenseAlpha(grid)
    a = m.aabb.detach().float().cpu()
    spacing = (a[1] - a[0]) / (torch.tensor(grid, dtype=torch.float32) - 1)
    v, f, n = marching_cubes(alpha, 0.005, spacing=spacing.tolist(), origin=a[0].tolist(), normals=True)
    assert torch.equal(v, vol.verts) and torch.equal(f, vol.faces) and torch.equal(n, vol.normals)
    assert m.export_mesh(level=0.005, normals=False, colors=False).normals is None
    with pytest.raises(T2NError):
        m.export_mesh(normals="volume")


def test_refusals(fields, pool):
    from text2nerf_amd import TensorVMSplit
    m, _, _ = fields["plain"]
    rays = torch.from_numpy(G.batch(pool, 4)).to(dev())
    for q in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(T2NError, match="quantile"):
            m.render_geometry(rays, quantile=q)
    lib, h = _lib.load(), m.sync_params()
    out = torch.empty(4, device=dev())
    with torch.cuda.device(dev()):
        rc = lib.t2n_render_geometry(h, _lib.ptr(rays), 4, 6, 65, 1.0, 8.0, _lib.ptr(out), None, None, None, None, _lib.current_stream_ptr(dev()))
        assert rc == -1                                   # T2N_ERR_INVALID
        assert lib.t2n_render_geometry(h, _lib.ptr(rays), 4, 5, 65, 0.5, 8.0, _lib.ptr(out), None, None, None, None, _lib.current_stream_ptr(dev())) == -1
        assert lib.t2n_density_grad_at(None, _lib.ptr(rays), 4, _lib.ptr(out), None, _lib.current_stream_ptr(dev())) == -1
    with pytest.raises(T2NError, match="NDC"):
        m.render_geometry(rays, ndc_ray=True)
    with pytest.raises(T2NError, match="CPU"):
        m.render_geometry(rays.cpu())
    with pytest.raises(T2NError, match="unknown outputs"):
        m.render_geometry(rays, want=("depth", "curvature"))
    wide = TensorVMSplit(torch.tensor(TINY["aabb"]), TINY["grid"], dev(), density_n_comp=[24] * 3, appearance_n_comp=[48] * 3, app_dim=27,
                         near_far=TINY["near_far"], shadingMode="MLP_Fea_noview", fea_pe=6, featureC=128)
    with pytest.raises(T2NError, match="general-shape"):
        wide.render_geometry(rays)
    with pytest.raises(T2NError):
        wide.density_gradient(rays[:, :3])
    with pytest.raises(T2NError, match="general-shape"):
        wide.export_mesh(normals="field", colors=False)
