"""The level-set export on the device against tests/helpers/mesh_levelset_ref.py (checked on its own in tests/test_mesh_levelset_cpu.py).

t2n_dense_feature / t2n_generic_dense_feature: every node within (m + 2) 2^-24 A_f of the float64 feature at the kernel's own float32
node (m counted in the helper: 24 on the tuned chain, 10 + sum(density_n_comp) on the general one), -inf exactly where an attached
mask samples <= 0, fp32 and bf16 factor storage. export_surface(surface="feature") at the field's own grid: the faces of the alpha
export index for index, every vertex within K 2^-24 (|f_a| + |f_b| + |f*| + A_f(v)) of the level in float64 (K counted in the helper).
export_surface(smooth=k): smooth_mesh of the unsmoothed export, colours and faces untouched. export_mesh itself: unchanged.
Every check prints a `LEVELSET` line with the measured ratio (profiles/mesh_levelset.txt keeps a run's)."""
import numpy as np
import pytest
import torch

from tests.helpers import mesh_levelset_ref as L
from tests.helpers import mesh_smooth_ref as S
from tests.test_hip_parity import dev, make_field
from tests.test_optim_kernels_gpu import Buf, call
from text2nerf_amd import _lib, mesh
from text2nerf_amd._lib import T2NError

pytestmark = pytest.mark.gpu


def with_mask(m, shape):
    """Attach updateAlphaMask(MASK_GRID)'s mask; returns the oracle config that carries the same volume."""
    m.alphaMask_thres = L.MASK_THRES
    m.updateAlphaMask(L.MASK_GRID)
    v = m.alphaMask.alpha_volume
    vol = v.reshape(v.shape[-3:]).cpu()
    assert 0.02 < float(vol.mean()) < 0.98
    return L.cfg_of(shape, vol)


def wide_field(params):
    from text2nerf_amd import TensorVMSplit
    w = L.WIDE
    m = TensorVMSplit(torch.tensor(w["aabb"], dtype=torch.float32), list(w["grid"]), dev(), density_n_comp=w["density_n_comp"],
                      appearance_n_comp=[48] * 3, app_dim=27, near_far=w["near_far"], shadingMode="MLP_Fea_noview", alphaMask_thres=1e-4,
                      density_shift=-10, distance_scale=25, pos_pe=0, view_pe=0, fea_pe=6, featureC=128, step_ratio=1.0,
                      fea2denseAct="softplus")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    assert m._is_general()
    return m


def raw_dense_feature(m, g):
    """t2n_dense_feature by hand on a guarded buffer."""
    h = m.sync_params()
    lins = [torch.linspace(0, 1, n).to(dev()) for n in g]
    out = Buf(np.full(int(np.prod(g)), np.nan, np.float32))
    call("t2n_dense_feature", h, _lib.ptr(lins[0]), _lib.ptr(lins[1]), _lib.ptr(lins[2]), g[0], g[1], g[2], out.ptr)
    torch.cuda.synchronize()
    assert out.guards_intact()
    got = out.get()
    assert not np.isnan(got).any(), "a node was not written"
    return got


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("name", list(L.SHAPES))
def test_dense_feature_elementwise(name, masked, storage):
    shape = L.SHAPES[name]
    params = L.blob_params(shape)
    m = make_field(params, shape["grid"], shape["aabb"], shape["near_far"])
    cfg = with_mask(m, shape) if masked else L.cfg_of(shape)
    m.factor_storage = storage
    for g in (shape["grid"], [13, 11, 9]):       # the field's own grid (every node on a texel) and one that is not
        ref = L.dense_feature(cfg, params, g, bf16=storage == "bf16")
        got = raw_dense_feature(m, g)
        bad, ratio, und = L.check_dense_feature(got, ref, L.M_TUNED)
        print(f"LEVELSET dense_feature {name} {'mask' if masked else 'plain'} {storage} {'x'.join(map(str, g))}: err/bound {ratio:.3f}, "
              f"{int(ref['masked'].sum())} masked nodes, {und} undecided")
        assert len(bad) == 0 and ratio <= 1.0, (g, bad[:8], ratio)
        # (undecided: nodes on the edge of the mask's support, where a rounding of the index decides; either value is right there.
        # The reference alone fixes how many there are: at most 6 % of the nodes on these grids)
        assert und <= 0.06 * got.size and (ref["decided"] & ~ref["masked"]).sum() > 100
        assert not masked or (ref["decided"] & ref["masked"]).sum() > 100
        assert bool(np.isneginf(got).any()) == masked
        feat, xyz = m.getDenseFeature(g)
        assert tuple(feat.shape) == tuple(g) and np.array_equal(feat.cpu().numpy().reshape(-1).view(np.uint32), got.view(np.uint32))
        assert torch.equal(xyz, m.getDenseAlpha(g)[1])
        # -inf exactly where dense alpha is forced to 0 by the mask, and alpha's inside / outside at the export level everywhere else
        alpha = m.getDenseAlpha(g)[0].cpu().numpy().reshape(-1)
        assert (alpha[np.isneginf(got)] == 0).all()


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "mask"])
def test_generic_dense_feature_elementwise(masked):
    w = L.WIDE
    params = L.blob_params(w, density_n_comp=w["density_n_comp"])
    m = wide_field(params)
    cfg = with_mask(m, w) if masked else L.cfg_of(w)
    mcount = L.m_general(w["density_n_comp"])
    for g in (w["grid"], [13, 11, 9]):
        ref = L.dense_feature(cfg, params, g)
        feat, _ = m.getDenseFeature(g)
        got = feat.cpu().numpy().reshape(-1)
        bad, ratio, und = L.check_dense_feature(got, ref, mcount)
        print(f"LEVELSET generic_dense_feature {'mask' if masked else 'plain'} {'x'.join(map(str, g))}: m = {mcount}, err/bound {ratio:.3f}, "
              f"{int(ref['masked'].sum())} masked nodes, {und} undecided")
        assert len(bad) == 0 and ratio <= 1.0, (g, bad[:8], ratio)
        assert bool(np.isneginf(got).any()) == masked
    # the export: colours are refused as before, the feature surface is accepted without them
    with pytest.raises(T2NError):
        m.export_surface(surface="feature")
    with pytest.raises(T2NError):
        m.export_surface(surface="feature", colors=False, normals="field")
    if not masked:
        fe = m.export_surface(level=L.ALPHA_LEVEL, colors=False, surface="feature")
        al = m.export_mesh(level=L.ALPHA_LEVEL, colors=False)
        assert fe.colors is None and fe.verts.shape[0] > 100 and torch.equal(fe.faces, al.faces)
        K = L.vertex_K(w["aabb"], w["grid"], mcount)
        level = L.export_level(L.ALPHA_LEVEL, float(m.stepSize))
        r, e = L.vertex_ratio(fe.verts.cpu().numpy(), cfg, params, w["grid"], level, K)
        print(f"LEVELSET generic export: K = {K}, max |f(v) - f*| {e:.3g}, ratio {r:.3g}")
        assert r <= 1.0


@pytest.fixture(scope="module")
def blob():
    shape = L.SHAPES["tiny"]
    params = L.blob_params(shape)
    return shape, params, make_field(params, shape["grid"], shape["aabb"], shape["near_far"]), L.cfg_of(shape)


def test_export_feature_surface_at_the_fields_own_grid(blob):
    """Measured on the MI355X (profiles/mesh_levelset.txt): 452 vertices, 900 faces, K = 539; the feature surface's largest
    |f(v) - f*| is 4.2e-6, 0.0066 of the bound (the counted K is dominated by worst-case position roundings of (5 + r)(g - 1) cells
    on three axes, which do not add up in practice); the alpha surface's is 0.745, 1.2e3 x the bound, its vertices up to 0.29 cell
    (median 0.10) away. At 31x27x19, not the field's grid: 0.132 / 0.0039 (max / median) against the alpha surface's 0.478 / 0.105."""
    shape, params, m, cfg = blob
    g = shape["grid"]
    al = m.export_mesh(level=L.ALPHA_LEVEL)
    fe = m.export_surface(level=L.ALPHA_LEVEL, surface="feature")
    assert fe.verts.shape[0] > 400 and torch.equal(fe.faces, al.faces) and fe.verts.shape == al.verts.shape
    level = L.export_level(L.ALPHA_LEVEL, float(m.stepSize))
    assert level == m.feature_level(L.ALPHA_LEVEL, float(m.stepSize) / float(m.distance_scale))
    K = L.vertex_K(shape["aabb"], g, L.M_TUNED)
    rf, ef = L.vertex_ratio(fe.verts.cpu().numpy(), cfg, params, g, level, K)
    ra, ea = L.vertex_ratio(al.verts.cpu().numpy(), cfg, params, g, level, K)
    sp = (np.asarray(shape["aabb"][1]) - np.asarray(shape["aabb"][0])) / (np.asarray(g) - 1)
    cells = (np.abs(fe.verts.cpu().numpy().astype(np.float64) - al.verts.cpu().numpy()) / sp).max(-1)
    print(f"LEVELSET export own grid {'x'.join(map(str, g))}: K = {K}, V {fe.verts.shape[0]} F {fe.faces.shape[0]}; feature surface max "
          f"|f(v) - f*| {ef:.3g} ratio {rf:.3g}; alpha surface {ea:.3g} ratio {ra:.3g}; vertices differ by up to {cells.max():.2f} cell "
          f"(median {np.median(cells):.2f})")
    assert rf <= 1.0
    # by hand: marching cubes on getDenseFeature at the level, normals the feature volume's, colours at the NEW vertices
    aabb = m.aabb.detach().float().cpu()
    spacing = ((aabb[1] - aabb[0]) / (torch.tensor(g, dtype=torch.float32) - 1)).tolist()
    v, f, n = mesh.marching_cubes(m.getDenseFeature(g)[0], level, spacing=spacing, origin=aabb[0].tolist())
    assert torch.equal(fe.verts, v) and torch.equal(fe.faces, f) and torch.equal(fe.normals, n)
    rgb = m.shade(m.normalize_coord(v), viewdirs=-n)[1]
    assert torch.equal(fe.colors, (rgb.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8))
    # the two volumes' normals point the same way
    dots = (fe.normals * al.normals).sum(-1)
    assert float(dots.min()) > 0.0
    # normals="field": the field's gradient at the new vertices; verts, faces, colours unchanged
    ff = m.export_surface(level=L.ALPHA_LEVEL, surface="feature", normals="field")
    assert torch.equal(ff.verts, v) and torch.equal(ff.faces, f) and torch.equal(ff.colors, fe.colors)
    assert float((ff.normals * fe.normals).sum(-1).min()) > 0.5
    bare = m.export_surface(level=L.ALPHA_LEVEL, surface="feature", colors=False, normals=False)
    assert bare.normals is None and bare.colors is None and torch.equal(bare.verts, v)
    with pytest.raises(T2NError):
        m.export_surface(level=2.0, surface="feature")
    # at a grid that is not the field's the interpolation is no longer exact: recorded, not asserted
    g2 = [31, 27, 19]
    fe2 = m.export_surface(level=L.ALPHA_LEVEL, gridSize=g2, surface="feature", colors=False)
    al2 = m.export_mesh(level=L.ALPHA_LEVEL, gridSize=g2, colors=False)
    e_f = np.abs(L.feature_at(cfg, params, fe2.verts.cpu().numpy().astype(np.float64))[0] - level)
    e_a = np.abs(L.feature_at(cfg, params, al2.verts.cpu().numpy().astype(np.float64))[0] - level)
    print(f"LEVELSET export other grid {'x'.join(map(str, g2))}: max / median |f(v) - f*| feature surface {e_f.max():.3g} / "
          f"{np.median(e_f):.3g}, alpha surface {e_a.max():.3g} / {np.median(e_a):.3g}")


def test_export_smooth(blob):
    shape, params, m, cfg = blob
    for surface in ("alpha", "feature"):
        base = m.export_surface(level=L.ALPHA_LEVEL, surface=surface)
        sm = m.export_surface(level=L.ALPHA_LEVEL, surface=surface, smooth=3)
        assert torch.equal(sm.faces, base.faces) and torch.equal(sm.colors, base.colors)
        want = mesh.smooth_mesh(base, iterations=3)
        assert torch.equal(sm.verts, want.verts) and not torch.equal(sm.verts, base.verts)
        assert torch.equal(sm.normals, mesh.vertex_normals(sm.verts, sm.faces)) and torch.equal(sm.normals, want.normals)
        v, f = base.verts.cpu().numpy(), base.faces.cpu().numpy()
        assert S.check_positions(sm.verts.cpu().numpy(), v, f, iterations=3) == []
        assert S.check_normals(sm.normals.cpu().numpy(), sm.verts.cpu().numpy(), f) == []
        fld = m.export_surface(level=L.ALPHA_LEVEL, surface=surface, smooth=3, normals="field")
        fld0 = m.export_surface(level=L.ALPHA_LEVEL, surface=surface, normals="field")
        assert torch.equal(fld.verts, sm.verts) and torch.equal(fld.normals, fld0.normals) and torch.equal(fld.colors, base.colors)
        bare = m.export_surface(level=L.ALPHA_LEVEL, surface=surface, smooth=3, normals=False, colors=False)
        assert bare.normals is None and bare.colors is None and torch.equal(bare.verts, sm.verts)
    empty = m.export_surface(level=0.999999, smooth=2)
    assert empty.verts.shape[0] == 0 and tuple(empty.normals.shape) == (0, 3)


def test_export_mesh_is_unchanged(blob, tmp_path):
    """export_mesh, and export_surface with its defaults, against marching_cubes(getDenseAlpha(...)) composed by hand."""
    shape, params, m, cfg = blob
    g = shape["grid"]
    alpha = m.getDenseAlpha()[0]
    aabb = m.aabb.detach().float().cpu()
    spacing = ((aabb[1] - aabb[0]) / (torch.tensor(g, dtype=torch.float32) - 1)).tolist()
    v, f, n = mesh.marching_cubes(alpha, L.ALPHA_LEVEL, spacing=spacing, origin=aabb[0].tolist())
    rgb = m.shade(m.normalize_coord(v), viewdirs=-n)[1]
    want = (rgb.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8)
    for out in (m.export_mesh(level=L.ALPHA_LEVEL), m.export_surface(level=L.ALPHA_LEVEL), m.export_surface(str(tmp_path / "a.ply"), L.ALPHA_LEVEL),
                m.export_surface(level=L.ALPHA_LEVEL, surface="alpha", smooth=0)):
        assert torch.equal(out.verts, v) and torch.equal(out.faces, f) and torch.equal(out.normals, n) and torch.equal(out.colors, want)
    d = m.export_mesh()
    v0, f0, n0 = mesh.marching_cubes(alpha, 0.005, spacing=spacing, origin=aabb[0].tolist())
    assert torch.equal(d.verts, v0) and torch.equal(d.faces, f0) and torch.equal(d.normals, n0)
