"""The smoothing stage on the device (csrc/t2n_mesh_smooth.hip through text2nerf_amd.mesh, and once through the raw C calls) against
the float64 reference tests/helpers/mesh_smooth_ref.py (checked and mutation-tested by tests/test_mesh_smooth_cpu.py): adjacency,
smoothed positions and vertex normals BIT-EQUAL. That is the claim: every float64 operation of a pass and of a normal is a single
IEEE operation in a documented order, and the rows are sorted.

Shapes: a workgroup owns kCcRun = 256 vertices, faces or keys (V = 255, 256, 257; fans whose centre row is 63, 64, 65 and 300 long),
the hand-made cases of the definition (an unreferenced vertex, a duplicated face, a degenerate face), the marching-cubes meshes of
mc_ref and the sphere (1332 vertices, 7980 directed edges: 32 workgroups of keys), and empty inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import mesh_smooth_ref as S
from tests.test_hip_parity import dev
from text2nerf_amd import _lib, mesh

pytestmark = pytest.mark.gpu

MC = ("ellipsoid", "torus", "noise", "sphere")


def get(name):
    return S.mc_mesh(name)[:2] if name in MC else S.small_meshes()[name]


def names():
    return list(S.small_meshes()) + list(MC)


def to_dev(x):
    return torch.from_numpy(np.array(x)).to(dev())          # a copy: the cached meshes are read-only


@pytest.mark.parametrize("name", names())
def test_adjacency_positions_and_normals_bit_equal(name):
    v, f = get(name)
    V = len(v)
    dv, df = to_dev(v), to_dev(f)
    adj = mesh.mesh_adjacency(df, V)
    assert isinstance(adj, mesh.Adjacency) and adj.offsets.is_cuda and adj.neighbours.is_cuda
    assert S.check_adjacency(adj.offsets.cpu().numpy(), adj.neighbours.cpu().numpy(), f, V) == [], name
    again = mesh.mesh_adjacency(df, V)
    assert torch.equal(adj.offsets, again.offsets) and torch.equal(adj.neighbours, again.neighbours)
    n = mesh.vertex_normals(dv, df)
    assert n.is_cuda and n.dtype == torch.float32 and S.check_normals(n.cpu().numpy(), v, f) == [], name
    assert torch.equal(n, mesh.vertex_normals(dv, df))
    fixed = np.zeros(V, bool)
    fixed[::3] = True
    cases = [dict(iterations=0), dict(iterations=1), dict(iterations=3), dict(iterations=10), dict(iterations=3, mu=0.0),
             dict(iterations=3, fixed=fixed), dict(iterations=2, lamb=1.0, mu=-0.9)]
    for kw in cases:
        dkw = dict(kw, fixed=to_dev(fixed)) if "fixed" in kw else kw
        out = mesh.smooth_mesh(mesh.Mesh(dv, df, n, None), **dkw)
        assert isinstance(out, mesh.Mesh) and out.verts.is_cuda and out.verts.dtype == torch.float32 and out.colors is None
        assert S.check_positions(out.verts.cpu().numpy(), v, f, **kw) == [], (name, kw)
        assert torch.equal(out.faces, df)
        if kw["iterations"] == 0:
            assert torch.equal(out.verts, dv) and torch.equal(out.normals, n)
        else:
            assert S.check_normals(out.normals.cpu().numpy(), out.verts.cpu().numpy(), f) == [], (name, kw)
        if "fixed" in kw:
            assert torch.equal(out.verts[to_dev(fixed)], dv[to_dev(fixed)])
    # two calls; a given adjacency; no normals in, none out
    a = mesh.smooth_mesh((dv, df), iterations=3)
    b = mesh.smooth_mesh((dv, df), iterations=3, adjacency=adj)
    assert a.normals is None and torch.equal(a.verts, b.verts) and torch.equal(a.verts, mesh.smooth_mesh((dv, df), iterations=3).verts)


def test_face_order_and_index_rotation_do_not_matter_on_the_device():
    v, f = get("noise")
    rng = np.random.default_rng(7)
    g = f[rng.permutation(len(f))]
    rot = rng.integers(0, 3, len(g))
    g = np.stack([g[np.arange(len(g)), (rot + k) % 3] for k in range(3)], -1).astype(np.int32)
    a, b = mesh.mesh_adjacency(to_dev(f), len(v)), mesh.mesh_adjacency(to_dev(g), len(v))
    assert torch.equal(a.offsets, b.offsets) and torch.equal(a.neighbours, b.neighbours)
    assert torch.equal(mesh.smooth_mesh((to_dev(v), to_dev(f)), iterations=3).verts, mesh.smooth_mesh((to_dev(v), to_dev(g)), iterations=3).verts)


def test_empty_inputs():
    e3f, e3i = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    adj = mesh.mesh_adjacency(to_dev(e3i), 0)
    assert adj.offsets.cpu().tolist() == [0] and tuple(adj.neighbours.shape) == (0,) and adj.neighbours.dtype == torch.int32
    adj = mesh.mesh_adjacency(to_dev(e3i), 5)
    assert adj.offsets.cpu().tolist() == [0] * 6 and adj.offsets.dtype == torch.int64
    assert tuple(mesh.vertex_normals(to_dev(e3f), to_dev(e3i)).shape) == (0, 3)
    out = mesh.smooth_mesh((to_dev(e3f), to_dev(e3i), to_dev(e3f), None), iterations=3)
    assert tuple(out.verts.shape) == (0, 3) and tuple(out.faces.shape) == (0, 3) and tuple(out.normals.shape) == (0, 3)
    # vertices without a single face: nothing moves, every normal is 0
    v = np.random.default_rng(0).standard_normal((7, 3)).astype(np.float32)
    out = mesh.smooth_mesh((to_dev(v), to_dev(e3i), to_dev(v), None), iterations=2)
    assert np.array_equal(out.verts.cpu().numpy(), v) and not out.normals.cpu().numpy().any()


def test_numpy_in_numpy_out_and_pass_through():
    v, f = (np.array(x) for x in get("ellipsoid"))          # copies: the cached meshes are read-only
    n0 = S.mc_mesh("ellipsoid")[2].astype(np.float32)
    colors = np.random.default_rng(5).integers(0, 256, v.shape).astype(np.uint8)
    adj = mesh.mesh_adjacency(f.astype(np.int64), len(v))
    assert isinstance(adj.offsets, np.ndarray) and isinstance(adj.neighbours, np.ndarray)
    assert S.check_adjacency(adj.offsets, adj.neighbours, f, len(v)) == []
    n = mesh.vertex_normals(v, f)
    assert isinstance(n, np.ndarray) and S.check_normals(n, v, f) == []
    out = mesh.smooth_mesh(mesh.Mesh(v, f, n0, colors), iterations=3, adjacency=adj)
    assert all(isinstance(x, np.ndarray) for x in out)
    assert S.check_positions(out.verts, v, f, iterations=3) == [] and S.check_normals(out.normals, out.verts, f) == []
    assert np.array_equal(out.faces, f) and out.faces.dtype == np.int32 and np.array_equal(out.colors, colors)
    t = mesh.smooth_mesh((torch.from_numpy(v), torch.from_numpy(f)), iterations=1)          # CPU tensors: numpy out
    assert isinstance(t.verts, np.ndarray) and t.normals is None and t.colors is None


def test_value_errors_come_before_any_launch(monkeypatch):
    v, f = get("tetrahedron")
    dv, df = to_dev(v), to_dev(f)
    lib = _lib.load()

    class NoLaunch:
        def __getattr__(self, name):
            if name.endswith("_workspace_bytes"):
                return getattr(lib, name)
            raise AssertionError(f"{name} was called")
    monkeypatch.setattr(_lib, "load", lambda *a, **k: NoLaunch())
    bad = [dict(iterations=-1), dict(iterations=1.5), dict(lamb=0.0), dict(lamb=-0.5), dict(lamb=1.01), dict(mu=0.01), dict(mu=float("nan")),
           dict(fixed=to_dev(np.zeros(3, bool)))]
    for kw in bad:
        with pytest.raises(ValueError):
            mesh.smooth_mesh((dv, df), **kw)
    for faces in (to_dev(np.array([[0, 1, 4]], np.int32)), to_dev(np.array([[0, 1, -1]], np.int32)), df[:, :2], df.float()):
        with pytest.raises(ValueError):
            mesh.smooth_mesh((dv, faces))
        with pytest.raises(ValueError):
            mesh.mesh_adjacency(faces, 4)
        with pytest.raises(ValueError):
            mesh.vertex_normals(dv, faces)
    with pytest.raises(ValueError):
        mesh.smooth_mesh((dv[:, :2], df))
    with pytest.raises(ValueError):
        mesh.vertex_normals(dv[:, :2], df)
    with pytest.raises(ValueError):
        mesh.smooth_mesh((dv, df, dv[:3], None))
    with pytest.raises(ValueError):
        mesh.smooth_mesh((dv,))
    # an adjacency that is not the rows of these vertices
    off, nbr = S.adjacency(f, 4)
    for a in ((off[:-1], nbr), (off, np.where(nbr == 3, 4, nbr).astype(np.int32)), (off + 1, nbr), (off[::-1].copy(), nbr),
              (np.concatenate([off[:-1], [off[-1] + 1]]), nbr)):
        with pytest.raises(ValueError):
            mesh.smooth_mesh((dv, df), adjacency=a)


def test_raw_c_calls():
    """The six entry points by hand on the noise mesh: keys, a sort, rows, two passes between two buffers, normals."""
    lib = _lib.load()
    v, f = get("noise")
    V, F = len(v), len(f)
    d = dev()
    df, dv = to_dev(f), to_dev(v)
    stream = _lib.current_stream_ptr(d)
    p = _lib.ptr

    def rows(fn, per):
        n = per * F
        keys = torch.empty(n, dtype=torch.int64, device=d)
        assert fn(p(df), F, V, p(keys), stream) == 0
        keys = torch.sort(keys).values
        nb = int(lib.t2n_mesh_csr_workspace_bytes(n))
        ws = torch.empty(nb, dtype=torch.uint8, device=d)
        off = torch.full((V + 1,), -7, dtype=torch.int64, device=d)
        val = torch.full((n,), -7, dtype=torch.int32, device=d)
        cnt = torch.empty(1, dtype=torch.int64, device=d)
        assert lib.t2n_mesh_csr(p(keys), n, V, p(off), p(val), p(cnt), p(ws), nb, stream) == 0
        E = int(cnt.item())
        assert (val[E:] == -7).all(), "values behind the count were written"
        return off, val[:E].contiguous()
    off, nbr = rows(lib.t2n_mesh_edge_keys, 6)
    assert S.check_adjacency(off.cpu().numpy(), nbr.cpu().numpy(), f, V) == []
    x = dv.double()
    y = torch.full_like(x, float("nan"))
    assert lib.t2n_mesh_smooth_pass(p(x), p(y), p(off), p(nbr), nbr.shape[0], None, V, C.c_double(0.5), stream) == 0
    assert lib.t2n_mesh_smooth_pass(p(y), p(x), p(off), p(nbr), nbr.shape[0], None, V, C.c_double(-0.53), stream) == 0
    assert S.check_positions(x.float().cpu().numpy(), v, f, iterations=1) == []
    w_off, w_nbr = S.adjacency(f, V)
    want64 = S.smooth_pass(S.smooth_pass(v.astype(np.float64), w_off, w_nbr, 0.5), w_off, w_nbr, -0.53)
    assert S.same_bits(x.cpu().numpy(), want64), "the float64 positions between the passes, bit for bit"
    voff, vrows = rows(lib.t2n_mesh_face_keys, 3)
    w = S.vertex_faces(f, V)
    assert S.same_bits(voff.cpu().numpy(), w[0]) and S.same_bits(vrows.cpu().numpy(), w[1])
    n = torch.full((V, 3), float("nan"), dtype=torch.float32, device=d)
    assert lib.t2n_mesh_vertex_normals(p(dv), p(df), F, p(voff), p(vrows), vrows.shape[0], V, p(n), stream) == 0
    assert S.check_normals(n.cpu().numpy(), v, f) == []
