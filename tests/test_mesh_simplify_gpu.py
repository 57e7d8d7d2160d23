"""The simplification stage on the device (csrc/t2n_mesh_simplify.hip through text2nerf_amd.mesh, and once through the raw C calls) against
the float64 reference tests/helpers/mesh_simplify_ref.py (checked and mutation-tested by tests/test_mesh_simplify_cpu.py): vertex_map,
offsets, members, cells, float32 positions, faces, colours and normals BIT-EQUAL. That is the claim: every float64 operation of a
placement is a single IEEE operation in a documented order, the rows are sorted, and everything else is integer.

Shapes: a workgroup owns kCcRun = 256 vertices, clusters or faces (strips of V = 255, 256, 257 in one cell and with every vertex alone,
which gives K = 255, 256, 257; fan(300) in one cluster: a member row and a face row past 256), the hand-made cases of the face rules
(tests/helpers/mesh_simplify_ref.collapse_case), the marching-cubes meshes of mc_ref and the sphere at cells 1, 2 and 3, one cell for
everything, and empty inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import mesh_simplify_ref as Q
from tests.helpers import mesh_smooth_ref as S
from tests.test_hip_parity import dev
from text2nerf_amd import _lib, mesh

pytestmark = pytest.mark.gpu

MC = ("ellipsoid", "torus", "noise", "sphere")
FAR = (-500.0, -500.0, -500.0)          # with a cell of 1000: one cell for everything


def get(name):
    return S.mc_mesh(name) if name in MC else S.small_meshes()[name] + (None,)


def names():
    return list(S.small_meshes()) + list(MC)


def to_dev(x):
    return None if x is None else torch.from_numpy(np.array(x)).to(dev())       # a copy: the cached meshes are read-only


def host(m):
    return tuple(None if x is None else x.cpu().numpy() for x in m)


def colours_of(v, seed=5):
    return np.random.default_rng(seed).integers(0, 256, v.shape).astype(np.uint8)


def grids(name, v):
    """(cell, origin) of a mesh: cells 1, 2 and 3, an anisotropic one, one cell for everything, and, where the grid stays below 2^31
    cells (the hand-made meshes), a cell that isolates every vertex."""
    out = [(1.0, None), (2.0, None), (3.0, None), ((1.5, 0.7, 2.2), None), (1000.0, FAR)]
    if name not in MC:
        out.append((Q.isolating_cell(v), None))
    return out


@pytest.mark.parametrize("name", names())
def test_clusters_positions_faces_colours_and_normals_bit_equal(name):
    v, f, n = get(name)
    V = len(v)
    colors = colours_of(v)
    dv, df, dc = to_dev(v), to_dev(f), to_dev(colors)
    dn = to_dev(n.astype(np.float32)) if n is not None else mesh.vertex_normals(dv, df)
    for cell, origin in grids(name, v):
        cl = mesh.mesh_clusters(dv, cell, origin)
        assert isinstance(cl, mesh.Clusters) and all(x.is_cuda for x in (cl.vertex_map, cl.offsets, cl.members, cl.cells))
        assert Q.check_clusters(host(cl[:1]) + (cl.n_clusters,) + host(cl[2:]), v, cell, origin) == [], (name, cell)
        again = mesh.mesh_clusters(dv, cell, origin)
        assert again.n_clusters == cl.n_clusters and all(torch.equal(a, b) for a, b in zip(cl[:1] + cl[2:], again[:1] + again[2:]))
        if origin is FAR:
            assert cl.n_clusters == 1
        for pl in ("mean", "quadric"):
            kw = dict(origin=origin, placement=pl)
            out = mesh.simplify_mesh(mesh.Mesh(dv, df, dn, dc), cell, **kw)
            assert isinstance(out, mesh.Mesh) and all(x.is_cuda for x in out)
            assert out.verts.dtype == torch.float32 and out.faces.dtype == torch.int32 and out.colors.dtype == torch.uint8
            assert Q.check_mesh(host(out), v, f, cell, normals=True, colors=colors, **kw) == [], (name, cell, pl)
            assert Q.check_faces(out.faces.cpu().numpy(), cl.n_clusters) == [], (name, cell, pl)
            # two calls; given clusters; no normals or colours in, none out
            b = mesh.simplify_mesh((dv, df), cell, clusters=cl, **kw)
            assert b.normals is None and b.colors is None and torch.equal(out.verts, b.verts) and torch.equal(out.faces, b.faces)
            c = mesh.simplify_mesh(mesh.Mesh(dv, df, dn, dc), cell, **kw)
            assert all(torch.equal(x, y) for x, y in zip(out, c))


def test_the_face_rules_and_a_given_origin_with_negative_coordinates():
    v, f, cell, origin = Q.collapse_case()
    assert (v < 0).any() and min(origin) < 0
    dv, df = to_dev(v), to_dev(f)
    cl = mesh.mesh_clusters(dv, cell, origin)
    assert cl.n_clusters == 5 and cl.vertex_map.cpu().tolist() == [1, 1, 3, 3, 2, 2, 4, 0]
    assert cl.cells.cpu().tolist() == [[0, 4, 0], [2, 0, 0], [2, 2, 0], [4, 0, 0], [4, 2, 1]]
    for pl in ("mean", "quadric"):
        out = mesh.simplify_mesh((dv, df), cell, origin=origin, placement=pl)
        # faces 1 and 3 repeat face 0's triple and leave, the oppositely oriented twin stays, the two collapsed faces leave
        assert out.faces.cpu().tolist() == [[1, 3, 2], [1, 2, 3], [1, 3, 4]]
        assert Q.check_mesh(host(out), v, f, cell, origin=origin, placement=pl) == []
        got = out.verts.cpu().numpy()
        assert S.same_bits(got[0], v[7]) and S.same_bits(got[4], v[6])      # the unreferenced vertex: the mean; one vertex with a face
    # the default origin is the minimum: other cells, the same rules
    assert Q.check_mesh(host(mesh.simplify_mesh((dv, df), cell)), v, f, cell) == []


@pytest.mark.parametrize("V", [255, 256, 257])
def test_the_256_wide_workgroup_edge(V):
    v, f = S.strip(V)
    dv, df = to_dev(v), to_dev(f)
    dc = to_dev(colours_of(v))
    h = Q.isolating_cell(v)
    for cell, origin, K in ((h, None, V), (1000.0, FAR, 1), (8.0, None, None)):
        cl = mesh.mesh_clusters(dv, cell, origin)
        assert K is None or cl.n_clusters == K
        assert Q.check_clusters(host(cl[:1]) + (cl.n_clusters,) + host(cl[2:]), v, cell, origin) == []
        for pl in ("mean", "quadric"):
            out = mesh.simplify_mesh((dv, df, None, dc), cell, origin=origin, placement=pl)
            assert Q.check_mesh(host(out), v, f, cell, origin=origin, placement=pl, colors=colours_of(v)) == [], (V, cell, pl)
            if K == V:
                assert len(out.faces) == len(f)
            if K == 1:
                assert tuple(out.faces.shape) == (0, 3) and out.faces.dtype == torch.int32


def test_rows_past_256_and_colour_sums_past_16_bits():
    """fan(300) in one cluster: 301 members, 300 faces in the quadric's row, every face collapses; colours of 0 and 255."""
    v, f = S.fan(300)
    dv, df = to_dev(v), to_dev(f)
    rng = np.random.default_rng(3)
    for colors in (np.full(v.shape, 255, np.uint8), np.zeros(v.shape, np.uint8), rng.choice(np.array([0, 255], np.uint8), v.shape)):
        for cell, origin in ((1000.0, FAR), (0.5, None)):
            out = mesh.simplify_mesh((dv, df, None, to_dev(colors)), cell, origin=origin)
            assert Q.check_mesh(host(out), v, f, cell, origin=origin, colors=colors) == []
            if origin is FAR:
                assert out.verts.shape[0] == 1 and out.faces.shape[0] == 0
                assert out.colors.cpu().tolist() == [[int(colors[0, 0])] * 3] or colors.min() != colors.max()
    # the centre alone in a fine grid: a cluster of one vertex with a face row of 300
    out = mesh.simplify_mesh((dv, df), 0.05)
    assert Q.check_mesh(host(out), v, f, 0.05) == []


def test_face_order_and_index_rotation_on_the_device():
    v, f, _ = get("noise")
    rng = np.random.default_rng(7)
    g = f[rng.permutation(len(f))]
    rot = rng.integers(0, 3, len(g))
    g = np.stack([g[np.arange(len(g)), (rot + k) % 3] for k in range(3)], -1).astype(np.int32)
    dv = to_dev(v)
    for cell in (1.0, 2.0):
        a, b = mesh.simplify_mesh((dv, to_dev(f)), cell), mesh.simplify_mesh((dv, to_dev(g)), cell)
        c = mesh.simplify_mesh((dv, to_dev(np.roll(f, 1, axis=1))), cell)
        assert torch.equal(a.verts, c.verts) and torch.equal(a.faces, c.faces)         # index rotation: the same bits
        assert torch.equal(a.verts, b.verts)
        fa, fb = a.faces.cpu().numpy(), b.faces.cpu().numpy()
        assert np.array_equal(fa[np.lexsort(fa.T[::-1])], fb[np.lexsort(fb.T[::-1])])  # face order: the same set
        assert Q.check_mesh(host(b), v, g, cell) == []


def test_numpy_in_numpy_out():
    v, f, n = (np.array(x) for x in get("ellipsoid"))           # copies: the cached meshes are read-only
    colors = colours_of(v)
    cl = mesh.mesh_clusters(v, 2.0)
    assert all(isinstance(x, np.ndarray) for x in (cl.vertex_map, cl.offsets, cl.members, cl.cells)) and isinstance(cl.n_clusters, int)
    assert Q.check_clusters(cl, v, 2.0) == []
    out = mesh.simplify_mesh(mesh.Mesh(v, f.astype(np.int64), n.astype(np.float32), colors), 2.0, clusters=cl)
    assert all(isinstance(x, np.ndarray) for x in out) and out.faces.dtype == np.int32
    assert Q.check_mesh(out, v, f, 2.0, normals=True, colors=colors) == []
    t = mesh.simplify_mesh((torch.from_numpy(v), torch.from_numpy(f)), (2.0, 2.0, 2.0), placement="mean")      # CPU tensors: numpy out
    assert isinstance(t.verts, np.ndarray) and t.normals is None and t.colors is None
    assert Q.check_mesh(t, v, f, 2.0, placement="mean") == []
    d = mesh.simplify_mesh((v.astype(np.float64), f), 2.0, regularisation=0.0)          # float64 positions are rounded to float32 first
    assert Q.check_mesh(d, v, f, 2.0, regularisation=0.0) == []


def test_empty_inputs_launch_nothing(monkeypatch):
    e3f, e3i = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    lib = _lib.load()

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called")
    monkeypatch.setattr(_lib, "load", lambda *a, **k: NoLaunch())
    cl = mesh.mesh_clusters(to_dev(e3f), 1.0)
    assert cl.n_clusters == 0 and cl.offsets.cpu().tolist() == [0] and cl.offsets.dtype == torch.int64
    assert tuple(cl.vertex_map.shape) == (0,) and tuple(cl.members.shape) == (0,) and tuple(cl.cells.shape) == (0, 3)
    out = mesh.simplify_mesh((to_dev(e3f), to_dev(e3i), to_dev(e3f), to_dev(np.zeros((0, 3), np.uint8))), 1.0)
    assert all(tuple(x.shape) == (0, 3) for x in out) and out.faces.dtype == torch.int32 and out.colors.dtype == torch.uint8
    monkeypatch.setattr(_lib, "load", lambda *a, **k: lib)
    # vertices without a single face: every cluster is its mean, no face comes out, the normals are 0
    v = np.random.default_rng(0).standard_normal((7, 3)).astype(np.float32)
    out = mesh.simplify_mesh((to_dev(v), to_dev(e3i), to_dev(v), None), 0.5)
    assert Q.check_mesh(host(out), v, e3i, 0.5, normals=True) == [] and not out.normals.cpu().numpy().any()


def test_value_errors_come_before_any_launch(monkeypatch):
    v, f = S.small_meshes()["tetrahedron"]
    dv, df = to_dev(v), to_dev(f)
    good = mesh.mesh_clusters(dv, 0.5)
    lib = _lib.load()

    class NoLaunch:
        def __getattr__(self, name):
            if name.endswith("_workspace_bytes"):
                return getattr(lib, name)
            raise AssertionError(f"{name} was called")
    monkeypatch.setattr(_lib, "load", lambda *a, **k: NoLaunch())
    nan = float("nan")
    bad_v = dv.clone()
    bad_v[1, 2] = nan
    for kw in (dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(cell=(1.0, 2.0)), dict(origin=(0.5, 0.0, 0.0)), dict(origin=(nan, 0, 0)),
               dict(cell=1e-4, verts=dv * 10), dict(verts=bad_v), dict(verts=dv[:, :2])):
        args = dict(verts=dv, cell=0.5, origin=None)
        args.update(kw)
        with pytest.raises(ValueError):
            mesh.mesh_clusters(args["verts"], args["cell"], args["origin"])
        with pytest.raises(ValueError):
            mesh.simplify_mesh((args["verts"], df), args["cell"], origin=args["origin"])
    for kw in (dict(placement="median"), dict(regularisation=-1.0), dict(regularisation=nan)):
        with pytest.raises(ValueError):
            mesh.simplify_mesh((dv, df), 0.5, **kw)
    for faces in (to_dev(np.array([[0, 1, 4]], np.int32)), to_dev(np.array([[0, 1, -1]], np.int32)), df[:, :2], df.float()):
        with pytest.raises(ValueError):
            mesh.simplify_mesh((dv, faces), 0.5)
    with pytest.raises(ValueError):
        mesh.simplify_mesh((dv, df, dv[:3], None), 0.5)
    with pytest.raises(ValueError):
        mesh.simplify_mesh((dv, df, None, dv[:3].to(torch.uint8)), 0.5)
    # clusters that are not the rows of these vertices
    vm, K, off, mem, cells = good
    for c in ((vm[:-1], K, off, mem, cells), (vm, K, off[:-1], mem, cells), (vm, K + 1, off, mem, cells), (vm + 1, K, off, mem, cells),
              (vm, K, off + 1, mem, cells), (vm, K, off, mem + 1, cells), (vm, K, off, mem - 1, cells), (vm, K, off, mem, cells[:-1]),
              (vm, K, torch.flip(off, [0]), mem, cells), (vm, K, off, mem)):
        with pytest.raises(ValueError):
            mesh.simplify_mesh((dv, df), 0.5, clusters=c)


def test_raw_c_calls_with_clipped_rows_and_bad_indices():
    """The entry points by hand on the noise mesh at cell 2, then again through arrays that lie: rows that run past their arrays, a
    member, a face row entry, a face corner and a map entry outside their ranges. Status codes are returned, what a lying array points
    at is skipped, and nothing behind the arrays' ends is written (canaries)."""
    lib = _lib.load()
    v, f, _ = get("noise")
    V, F = len(v), len(f)
    d = dev()
    dv, df = to_dev(v), to_dev(f)
    stream = _lib.current_stream_ptr(d)
    p = _lib.ptr
    cell = 2.0
    o, h = Q.grid(v, cell)
    want = Q.simplify(v, f, cell)
    wcl = want.clusters
    K = wcl.n_clusters
    dims = (wcl.cells.max(0) + 1).tolist()
    o3, h3, d3 = (C.c_double * 3)(*o), (C.c_double * 3)(*h), (C.c_int32 * 3)(*dims)

    keys = torch.empty(V, dtype=torch.int64, device=d)
    assert lib.t2n_mesh_cluster_keys(p(dv), V, o3, h3, d3, p(keys), stream) == 0
    keys = torch.sort(keys).values
    nb = int(lib.t2n_mesh_cluster_rows_workspace_bytes(V))
    ws = torch.empty(nb, dtype=torch.uint8, device=d)
    vmap = torch.full((V + 3,), -7, dtype=torch.int32, device=d)
    off = torch.full((V + 1,), -7, dtype=torch.int64, device=d)
    mem = torch.full((V + 3,), -7, dtype=torch.int32, device=d)
    cells = torch.full((V + 1, 3), -7, dtype=torch.int32, device=d)
    cnt = torch.empty(1, dtype=torch.int64, device=d)
    assert lib.t2n_mesh_cluster_rows(p(keys), V, d3, p(vmap), p(off), p(mem), p(cells), p(cnt), p(ws), nb, stream) == 0
    assert int(cnt.item()) == K
    assert (vmap[V:] == -7).all() and (mem[V:] == -7).all() and (off[K + 1:] == -7).all() and (cells[K:] == -7).all()
    got = (vmap[:V].cpu().numpy(), K, off[:K + 1].cpu().numpy(), mem[:V].cpu().numpy(), cells[:K].cpu().numpy())
    assert Q.check_clusters(got, v, cell) == []
    vmap, off, mem, cells = vmap[:V].contiguous(), off[:K + 1].contiguous(), mem[:V].contiguous(), cells[:K].contiguous()

    def face_rows(vm):
        fkeys = torch.empty(3 * F, dtype=torch.int64, device=d)
        assert lib.t2n_mesh_cluster_face_keys(p(df), F, V, p(vm), K, p(fkeys), stream) == 0
        fkeys = torch.sort(fkeys).values
        nbc = int(lib.t2n_mesh_csr_workspace_bytes(3 * F))
        wsc = torch.empty(nbc, dtype=torch.uint8, device=d)
        foff = torch.empty(K + 1, dtype=torch.int64, device=d)
        frow = torch.full((3 * F,), -7, dtype=torch.int32, device=d)
        fcnt = torch.empty(1, dtype=torch.int64, device=d)
        assert lib.t2n_mesh_csr(p(fkeys), 3 * F, K, p(foff), p(frow), p(fcnt), p(wsc), nbc, stream) == 0
        return foff, frow[:int(fcnt.item())].contiguous()
    foff, frow = face_rows(vmap)
    assert Q.check_face_rows(foff.cpu().numpy(), frow.cpu().numpy(), f, wcl.vertex_map, K) == []

    def place(off_=off, mem_=mem, M=V, foff_=foff, frow_=frow, E=None, faces=df, quadric=1):
        out = torch.full((K + 1, 3), float("nan"), dtype=torch.float32, device=d)
        E = int(frow_.shape[0]) if E is None else E
        assert lib.t2n_mesh_cluster_place(p(dv), V, p(faces), F, p(off_), p(mem_), M, p(cells), K, p(foff_), p(frow_), E, o3, h3,
                                          C.c_double(1e-3), quadric, p(out), stream) == 0
        assert torch.isnan(out[K]).all(), "a row behind the last cluster was written"
        return out[:K].cpu().numpy()
    assert S.same_bits(place(), want.verts)
    assert S.same_bits(place(quadric=0), Q.simplify(v, f, cell, placement="mean").verts)

    # lying arrays. Member rows clipped to M = V - 5 and one member out of range: those vertices leave the means; a face row entry and a
    # face corner out of range: those faces leave the quadrics; offsets that run past the arrays. The result is the reference's on
    # the arrays as the kernel must read them.
    M = V - 5
    lie_mem = mem.clone()
    lie_mem[3] = V + 100
    lie_mem[10] = -1
    lie_off = off.clone()
    lie_off[K] = V + 1000
    lie_foff = foff.clone()
    lie_foff[K] = int(frow.shape[0]) + 1000
    lie_frow = frow.clone()
    lie_frow[5] = F + 100
    lie_frow[9] = -3
    lie_f = df.clone()
    lie_f[int(frow[20].item()), 1] = V + 7
    E = int(frow.shape[0]) - 4
    got = place(lie_off, lie_mem, M, lie_foff, lie_frow, E, lie_f)
    # the same through the reference: drop what must be skipped, then place
    mem_h, off_h = lie_mem.cpu().numpy(), np.minimum(lie_off.cpu().numpy(), M)
    frow_h, foff_h = lie_frow.cpu().numpy()[:E], np.minimum(lie_foff.cpu().numpy(), E)
    f_h = lie_f.cpu().numpy()
    x = v.astype(np.float64)
    exp = np.zeros((K, 3), np.float32)
    for k in range(K):
        rows = [int(m) for m in mem_h[off_h[k]:off_h[k + 1]] if 0 <= m < V]
        if not rows:
            continue
        s = np.zeros(3)
        for m in rows:
            s = s + x[m]
        mean = s / float(len(rows))
        sub_cl = Q.Clusters(np.zeros(V, np.int32), 1, np.array([0, len(rows)], np.int64), np.array(rows, np.int32), wcl.cells[k:k + 1])
        ts = [int(t) for t in frow_h[foff_h[k]:foff_h[k + 1]] if 0 <= t < F and (f_h[t] >= 0).all() and (f_h[t] < V).all()]
        # a one-cluster problem whose face row is exactly ts: a map that sends the corners of those faces to cluster 0
        vm1 = np.full(V, -1, np.int64)
        sub_f = f_h[ts].astype(np.int64)
        pk, _ = Q.place(v, sub_f, sub_cl._replace(vertex_map=np.zeros(V, np.int32)), cell, origin=o)
        assert vm1.shape == (V,) and np.array_equal(mean, Q.place(v, sub_f, sub_cl, cell, origin=o, placement="mean")[0][0])
        exp[k] = pk[0].astype(np.float32)
    assert S.same_bits(got, exp)

    # colours through the same lying member rows
    colors = colours_of(v)
    dc = to_dev(colors)
    cout = torch.full((K + 1, 3), 77, dtype=torch.uint8, device=d)
    assert lib.t2n_mesh_cluster_colors(p(dc), V, p(lie_off), p(lie_mem), M, K, p(cout), stream) == 0
    assert (cout[K] == 77).all()
    cexp = np.zeros((K, 3), np.uint8)
    for k in range(K):
        rows = [int(m) for m in mem_h[off_h[k]:off_h[k + 1]] if 0 <= m < V]
        if rows:
            tot = colors[rows].astype(np.int64).sum(0)
            cexp[k] = (tot + len(rows) // 2) // len(rows)
    assert np.array_equal(cout[:K].cpu().numpy(), cexp)
    assert lib.t2n_mesh_cluster_colors(p(dc), V, p(off), p(mem), V, K, p(cout), stream) == 0
    assert np.array_equal(cout[:K].cpu().numpy(), Q.simplify(v, f, cell, colors=colors).colors)

    # faces: a map entry and a corner out of range drop their faces; an `order` entry out of range is skipped
    def faces_out(vm, faces, spoil_order=False):
        rot = torch.full((F + 1, 3), -7, dtype=torch.int32, device=d)
        khi = torch.full((F + 1,), -7, dtype=torch.int64, device=d)
        klo = torch.full((F + 1,), -7, dtype=torch.int64, device=d)
        assert lib.t2n_mesh_simplify_face_map(p(faces), F, V, p(vm), K, p(rot), p(khi), p(klo), stream) == 0
        assert (rot[F] == -7).all() and int(khi[F]) == -7 and int(klo[F]) == -7
        by_lo = torch.sort(klo[:F], stable=True).indices
        order = by_lo[torch.sort(khi[:F][by_lo], stable=True).indices].contiguous()
        if spoil_order:
            order[-1] = F + 5           # the last slot holds a dropped face or the last triple's only holder: nothing else changes
        nbf = int(lib.t2n_mesh_simplify_faces_workspace_bytes(F))
        wsf = torch.empty(nbf, dtype=torch.uint8, device=d)
        kept = torch.full((F + 1, 3), -7, dtype=torch.int32, device=d)
        fcnt = torch.empty(1, dtype=torch.int64, device=d)
        assert lib.t2n_mesh_simplify_faces(p(rot), p(order), F, p(kept), p(fcnt), p(wsf), nbf, stream) == 0
        n = int(fcnt.item())
        assert (kept[n:] == -7).all(), "faces behind the count were written"
        return kept[:n].cpu().numpy(), rot[:F].cpu().numpy()
    kept, _ = faces_out(vmap, df)
    assert S.same_bits(kept, want.faces)
    lie_vm = vmap.clone()
    lie_vm[int(f[0, 0])] = K + 3
    lie_vm[int(f[1, 1])] = -2
    kept, rot = faces_out(lie_vm, lie_f)
    vm_h = lie_vm.cpu().numpy().astype(np.int64)
    m = np.where((f_h >= 0) & (f_h < V), vm_h[np.clip(f_h, 0, V - 1)], -1)
    ok = ((f_h >= 0) & (f_h < V)).all(-1) & ((m >= 0) & (m < K)).all(-1) & (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 2] != m[:, 0])
    assert (rot[~ok] == -1).all() and np.array_equal(rot[ok], Q.rotate_min_first(m[ok]))
    idx = np.nonzero(ok)[0]
    _, first = np.unique(rot[idx], axis=0, return_index=True)
    assert np.array_equal(kept, rot[np.sort(idx[first])])
    assert faces_out(vmap, df, spoil_order=True)[0].shape[0] in (len(want.faces), len(want.faces) - 1)
    # refusals return the status code and the message
    assert lib.t2n_mesh_cluster_rows(p(keys), V, d3, p(vmap), p(off), p(mem), p(cells), p(cnt), p(ws), nb - 1, stream) == -1
    assert b"t2n_mesh_cluster_rows" in lib.t2n_last_error()
    assert lib.t2n_mesh_cluster_place(p(dv), V, p(df), F, p(off), p(mem), V, p(cells), K + V, p(foff), p(frow), 0, o3, h3, C.c_double(1e-3), 1,
                                      p(dv), stream) == -1
