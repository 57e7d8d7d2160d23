"""Mesh export on the device: marching cubes over a dense volume (csrc/t2n_mesh.hip, `t2n_mc_count` / `t2n_mc_emit`) and a PLY
writer, in the place of `skimage.measure.marching_cubes` on a host copy followed by a Python loop per vertex and per face into
`plyfile` records (`convert_sdf_samples_to_ply`, utils.py:512-572). Neither package is needed.

    marching_cubes               volume, level -> (verts, faces, normals); device tensors in, device tensors out
    convert_sdf_samples_to_ply   the reference's function, signature and defaults (tests/golden/mesh_signatures.json)
    write_ply                    binary little-endian PLY by numpy `tofile`, property names as plyfile writes them
    Mesh                         what `TensorBase.export_mesh` returns: verts, faces, normals, colors
    mesh_components              faces, n_verts -> Components(labels, n_components, vert_counts, face_counts)
    filter_components            a Mesh without its unwanted components ("floaters"): min_faces and / or keep_largest
    select_faces                 a Mesh reduced to the faces a per-face flag array keeps (what text2nerf_amd.tsdf's observed-cells rule uses)
    mesh_adjacency               faces, n_verts -> Adjacency(offsets, neighbours): sorted unique CSR rows (csrc/t2n_mesh_smooth.hip)
    smooth_mesh                  Taubin lambda | mu smoothing in float64 over those rows, normals recomputed
    vertex_normals               area-weighted normals of a mesh's faces, float64 sums in ascending face order
    mesh_clusters                verts, cell -> Clusters(vertex_map, n_clusters, offsets, members, cells): the occupied cells of a uniform grid
    simplify_mesh                one vertex per cluster at its quadric-optimal point or its mean (csrc/t2n_mesh_simplify.hip); NOT manifold-preserving

The meshes are closed oriented 2-manifolds (the case table is generated from rules, tools/gen_mc_table.py); the right-hand normal of
every triangle, and every vertex normal, points towards LOWER values: out of the dense region of an alpha volume. Vertex and face order
are functions of the input alone (no atomics): two calls give bit-equal arrays. No CPU fallback.

A Text2NeRF alpha volume at the export level holds the scene's surface plus detached blobs. The documented route to a usable mesh:

    m = tensorf.export_mesh(None)                 # colours and normals as before
    m = filter_components(m, keep_largest=1)      # or min_faces=...
    m = smooth_mesh(m, iterations=10)             # optional: Taubin smoothing, after the floaters have left
    m = simplify_mesh(m, cell=2 * node_spacing)   # optional: vertex clustering, last (it does not preserve manifoldness)
    write_ply("scene.ply", *m)

Components are all-integer (lock-free union-find whose roots are each component's smallest vertex, integer counts, scans): labels,
counts and the compacted arrays are functions of the face list alone as well."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib


class Mesh(NamedTuple):
    verts: torch.Tensor                 # [V,3] float32, world space
    faces: torch.Tensor                 # [F,3] int32
    normals: Optional[torch.Tensor]     # [V,3] float32 unit vectors towards lower values, or None
    colors: Optional[torch.Tensor]      # [V,3] uint8, or None


class Components(NamedTuple):
    labels: torch.Tensor                # [V] int32, 0 .. K-1 in the order of each component's smallest vertex index
    n_components: int                   # K
    vert_counts: torch.Tensor           # [K] int32
    face_counts: torch.Tensor           # [K] int32


class Adjacency(NamedTuple):
    offsets: torch.Tensor               # [V+1] int64: row v is neighbours[offsets[v] : offsets[v+1]]
    neighbours: torch.Tensor            # [E] int32, every row sorted ascending and unique


class Clusters(NamedTuple):
    vertex_map: torch.Tensor            # [V] int32: the cluster of every vertex
    n_clusters: int                     # K: the occupied cells, numbered in ascending cell id
    offsets: torch.Tensor               # [K+1] int64: cluster k is members[offsets[k] : offsets[k+1]]
    members: torch.Tensor               # [V] int32, every row in ascending vertex index
    cells: torch.Tensor                 # [K,3] int32: the cell (c0, c1, c2) of every cluster


def _device():
    if not torch.cuda.is_available():
        raise _lib.T2NError("the mesh stages run on the MI355X only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _three(x, what):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().tolist()
    v = [float(t) for t in np.asarray(x, dtype=np.float64).reshape(-1)]
    if len(v) != 3:
        raise ValueError(f"marching_cubes: {what} needs three values, got {len(v)}")
    return v


@torch.no_grad()
def marching_cubes(volume, level, spacing=(1., 1., 1.), origin=(0., 0., 0.), normals=True, flip=False):
    """Triangle mesh of the surface volume == level. volume [n0,n1,n2]: a device tensor (device tensors come back), or a numpy array /
    CPU tensor (numpy arrays come back, through the device); any float dtype and any strides, converted once to contiguous float32.
    Returns (verts [V,3] float32, faces [F,3] int32, normals [V,3] float32 or None). Node (i,j,k) sits at origin + (i,j,k) * spacing.
    A node is inside iff its value > level (NaN is outside); right-hand face normals and the vertex normals point to lower values,
    `flip` swaps the last two indices of every face. A level that no edge crosses gives empty arrays. ValueError for what the library
    refuses (a dimension < 2, 2^31 nodes and more, a spacing that is not finite and positive); T2NError for a surface of 2^31 vertices
    or triangles and more."""
    lib = _lib.load()
    on_device = isinstance(volume, torch.Tensor) and volume.is_cuda
    if len(volume.shape) != 3:
        raise ValueError(f"marching_cubes: a volume of shape {tuple(volume.shape)}, need [n0,n1,n2]")
    dev = volume.device if on_device else _device()
    t = volume if isinstance(volume, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(volume))
    if not t.is_floating_point():
        t = t.to(torch.float32)
    vol = t.detach().to(device=dev, dtype=torch.float32).contiguous()
    n0, n1, n2 = (int(s) for s in vol.shape)
    sp, org = _three(spacing, "spacing"), _three(origin, "origin")
    nbytes = int(lib.t2n_mc_workspace_bytes(n0, n1, n2)) if max(n0, n1, n2) < 2**31 else 0
    if nbytes == 0 or not all(math.isfinite(s) and s > 0 for s in sp):
        raise ValueError(f"marching_cubes: shape {(n0, n1, n2)} (every dimension >= 2, fewer than 2^31 nodes) with spacing {sp} "
                         "(finite and positive) is refused")
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        stream = _lib.current_stream_ptr(dev)
        _lib.check(lib.t2n_mc_count(_lib.ptr(vol), n0, n1, n2, float(level), _lib.ptr(ws), _lib.ptr(counts), stream), "t2n_mc_count")
        V, F = (int(x) for x in counts.cpu().tolist())          # the one 16-byte read
        if V >= 2**31 or F >= 2**31:
            raise _lib.T2NError(f"marching_cubes: {V} vertices and {F} triangles do not fit int32 indices")
        verts = torch.empty(V, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
        norms = torch.empty(V, 3, dtype=torch.float32, device=dev) if normals else None
        if V > 0:                                               # nothing is launched on empty buffers
            _lib.check(lib.t2n_mc_emit(_lib.ptr(vol), n0, n1, n2, float(level), _lib.ptr(ws), (C.c_float * 3)(*org), (C.c_float * 3)(*sp),
                                       1 if flip else 0, _lib.ptr(verts), _lib.ptr(norms), _lib.ptr(faces), stream), "t2n_mc_emit")
    if on_device:
        return verts, faces, norms
    return verts.cpu().numpy(), faces.cpu().numpy(), None if norms is None else norms.cpu().numpy()


# ---- connected components and floater removal -----------------------------------------------------------------------------------------
def _is_device(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _faces_on_device(faces, n_verts, who):
    """faces as a contiguous int32 device tensor [F,3], every index inside [0, n_verts): ValueError otherwise, before any launch of
    ours (one device min / max, read once)."""
    t = faces if isinstance(faces, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(faces))
    if t.dim() != 2 or t.shape[1] != 3 or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"{who}: faces of shape {tuple(t.shape)} and dtype {t.dtype}, need [F,3] integer")
    V = int(n_verts)
    if V < 0 or V >= 2**31 or 3 * t.shape[0] >= 2**31:
        raise ValueError(f"{who}: {V} vertices and {t.shape[0]} faces (need 0 <= V < 2^31 and 3 F < 2^31)")
    dev = t.device if t.is_cuda else _device()
    t = t.detach().to(dev)
    if t.shape[0]:
        lo, hi = (int(x) for x in torch.stack(torch.aminmax(t)).cpu().tolist())
        if lo < 0 or hi >= V:
            raise ValueError(f"{who}: face indices span [{lo}, {hi}], outside [0, {V})")
    return t.to(torch.int32).contiguous(), dev


def _components(lib, f, V, dev):
    """Components of checked device faces; device tensors."""
    F = int(f.shape[0])
    labels = torch.empty(V, dtype=torch.int32, device=dev)
    if V == 0:                                                  # nothing is launched
        e = torch.empty(0, dtype=torch.int32, device=dev)
        return Components(labels, 0, e, e.clone()), None
    with torch.cuda.device(dev):
        nbytes = int(lib.t2n_mesh_components_workspace_bytes(V, F))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        k = torch.empty(1, dtype=torch.int64, device=dev)
        stream = _lib.current_stream_ptr(dev)
        _lib.check(lib.t2n_mesh_components(_lib.ptr(f), F, V, _lib.ptr(labels), _lib.ptr(k), _lib.ptr(ws), nbytes, stream),
                   "t2n_mesh_components")
        K = int(k.cpu().item())                                 # the one 8-byte read
        vc = torch.empty(K, dtype=torch.int32, device=dev)
        fc = torch.empty(K, dtype=torch.int32, device=dev)
        _lib.check(lib.t2n_mesh_component_sizes(_lib.ptr(f), F, _lib.ptr(labels), V, K, _lib.ptr(vc), _lib.ptr(fc), stream),
                   "t2n_mesh_component_sizes")
    return Components(labels, K, vc, fc), ws


@torch.no_grad()
def mesh_components(faces, n_verts):
    """Connected components of a triangle list: Components(labels [V] int32, n_components K, vert_counts [K] int32, face_counts [K]
    int32). faces [F,3] integer: a device tensor (device tensors come back) or a numpy array / CPU tensor (numpy arrays come back,
    through the device). Two vertices are connected when a face contains both; a vertex that no face references is a component of its
    own with 0 faces. Labels are dense and numbered in the order of each component's smallest vertex index, so `labels` is one fixed
    array for a given face list; two calls give bit-equal arrays. Host reads: the index check's min / max and the 8 bytes of K.
    ValueError: faces that are not [F,3] integer, an index outside [0, n_verts). T2NError without a GPU."""
    lib = _lib.load()
    f, dev = _faces_on_device(faces, n_verts, "mesh_components")
    c, _ = _components(lib, f, int(n_verts), dev)
    if _is_device(faces):
        return c
    return Components(c.labels.cpu().numpy(), c.n_components, c.vert_counts.cpu().numpy(), c.face_counts.cpu().numpy())


def _rows(x, V, dtype, dev, what, who="filter_components"):
    if x is None:
        return None
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if tuple(t.shape) != (V, 3):
        raise ValueError(f"{who}: {what} of shape {tuple(t.shape)} for {V} vertices, need [V,3]")
    return t.detach().to(device=dev, dtype=dtype).contiguous()


@torch.no_grad()
def filter_components(mesh, min_faces=0, keep_largest=None, components=None):
    """`mesh` (a Mesh, or (verts, faces[, normals[, colors]])) without the components the caller does not want, as a Mesh. Component c
    stays iff face_counts[c] >= min_faces and, with keep_largest = k, c is among the k components with the most faces (ties go to the
    lower label). Kept vertices keep their relative order and their verts / normals / colors rows move together; kept faces keep
    their relative order and are re-indexed: whole components leave, so a closed oriented 2-manifold stays one. `components`: an
    earlier mesh_components(faces, V) result for the same mesh, to skip the labelling. Device tensors in, device tensors out; numpy
    arrays / CPU tensors in, numpy arrays out. normals and colors that are None stay None. Host reads: the index check's min / max,
    K when `components` is not given, and the 16 bytes of the new totals. ValueError: min_faces < 0, keep_largest < 1, faces that are
    not [F,3] integer or hold an index outside [0, V), rows that do not match verts. T2NError without a GPU."""
    lib = _lib.load()
    parts = tuple(mesh)
    if not 2 <= len(parts) <= 4:
        raise ValueError(f"filter_components: a mesh of {len(parts)} parts, need (verts, faces[, normals[, colors]])")
    verts, faces, normals, colors = parts + (None,) * (4 - len(parts))
    if int(min_faces) < 0:
        raise ValueError(f"filter_components: min_faces {min_faces} < 0")
    if keep_largest is not None and int(keep_largest) < 1:
        raise ValueError(f"filter_components: keep_largest {keep_largest} < 1")
    if len(verts.shape) != 2 or verts.shape[1] != 3:
        raise ValueError(f"filter_components: verts of shape {tuple(verts.shape)}, need [V,3]")
    V = int(verts.shape[0])
    f, dev = _faces_on_device(faces, V, "filter_components")
    F = int(f.shape[0])
    v = _rows(verts, V, torch.float32, dev, "verts")
    n = _rows(normals, V, torch.float32, dev, "normals")
    c = _rows(colors, V, torch.uint8, dev, "colors")
    ws = None
    if components is None:
        comp, ws = _components(lib, f, V, dev)
    else:
        labels, K, _, fc = components
        as_i32 = lambda x: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(
            device=dev, dtype=torch.int32).contiguous()
        comp = Components(as_i32(labels), int(K), None, as_i32(fc))
        if tuple(comp.labels.shape) != (V,) or tuple(comp.face_counts.shape) != (comp.n_components,) or comp.n_components > V:
            raise ValueError(f"filter_components: components of {tuple(comp.labels.shape)} labels and {comp.n_components} counts do not "
                             f"belong to a mesh of {V} vertices")
    K = comp.n_components
    with torch.cuda.device(dev):
        keep = comp.face_counts >= int(min_faces)
        if keep_largest is not None and K > 0:
            order = torch.sort(comp.face_counts, descending=True, stable=True).indices     # ties: the lower label first
            top = torch.zeros(K, dtype=torch.bool, device=dev)
            top[order[:int(keep_largest)]] = True
            keep &= top
        keep = keep.to(torch.uint8).contiguous()
        Vk = Fk = 0
        if V > 0:                                               # nothing is launched on an empty mesh
            nbytes = int(lib.t2n_mesh_components_workspace_bytes(V, F))
            if ws is None:
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            totals = torch.empty(2, dtype=torch.int64, device=dev)
            stream = _lib.current_stream_ptr(dev)
            args = (_lib.ptr(f), F, _lib.ptr(comp.labels), V, _lib.ptr(keep), K)
            _lib.check(lib.t2n_mesh_filter_count(*args, _lib.ptr(ws), nbytes, _lib.ptr(totals), stream), "t2n_mesh_filter_count")
            Vk, Fk = (int(x) for x in totals.cpu().tolist())    # the one 16-byte read
        out_v = torch.empty(Vk, 3, dtype=torch.float32, device=dev)
        out_f = torch.empty(Fk, 3, dtype=torch.int32, device=dev)
        out_n = None if n is None else torch.empty(Vk, 3, dtype=torch.float32, device=dev)
        out_c = None if c is None else torch.empty(Vk, 3, dtype=torch.uint8, device=dev)
        if Vk > 0:
            _lib.check(lib.t2n_mesh_filter_emit(*args, _lib.ptr(v), _lib.ptr(n), _lib.ptr(c), _lib.ptr(ws), nbytes, _lib.ptr(out_v),
                                                _lib.ptr(out_n), _lib.ptr(out_c), _lib.ptr(out_f), stream), "t2n_mesh_filter_emit")
    if _is_device(verts):
        return Mesh(out_v, out_f, out_n, out_c)
    host = lambda x: None if x is None else x.cpu().numpy()
    return Mesh(host(out_v), host(out_f), host(out_n), host(out_c))


def _select_faces(lib, v, f, n, c, keep, dev):
    """select_faces on checked device tensors (keep [F] uint8); a Mesh of device tensors. Reads the 16 bytes of the new totals."""
    V, F = int(v.shape[0]), int(f.shape[0])
    Vk = Fk = 0
    with torch.cuda.device(dev):
        if V > 0 and F > 0:                                     # nothing is launched on an empty mesh
            nbytes = int(lib.t2n_mesh_select_faces_workspace_bytes(V, F))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            totals = torch.empty(2, dtype=torch.int64, device=dev)
            stream = _lib.current_stream_ptr(dev)
            _lib.check(lib.t2n_mesh_select_faces_count(_lib.ptr(f), F, V, _lib.ptr(keep), _lib.ptr(ws), nbytes, _lib.ptr(totals), stream),
                       "t2n_mesh_select_faces_count")
            Vk, Fk = (int(x) for x in totals.cpu().tolist())    # the one 16-byte read
        out_v = torch.empty(Vk, 3, dtype=torch.float32, device=dev)
        out_f = torch.empty(Fk, 3, dtype=torch.int32, device=dev)
        out_n = None if n is None else torch.empty(Vk, 3, dtype=torch.float32, device=dev)
        out_c = None if c is None else torch.empty(Vk, 3, dtype=torch.uint8, device=dev)
        if Vk > 0:
            _lib.check(lib.t2n_mesh_select_faces_emit(_lib.ptr(f), F, V, _lib.ptr(keep), _lib.ptr(v), _lib.ptr(n), _lib.ptr(c), _lib.ptr(ws),
                                                      nbytes, _lib.ptr(out_v), _lib.ptr(out_n), _lib.ptr(out_c), _lib.ptr(out_f), stream),
                       "t2n_mesh_select_faces_emit")
    return Mesh(out_v, out_f, out_n, out_c)


@torch.no_grad()
def select_faces(mesh, keep):
    """`mesh` (a Mesh, or (verts, faces[, normals[, colors]])) reduced to the faces whose flag in `keep` ([F], bool or any integer
    dtype: nonzero = stay) is set, as a Mesh. A vertex stays iff a kept face references it; kept vertices and kept faces keep their
    relative order, the verts / normals / colors rows move together, faces are re-indexed. All integer (the vertices' flags are
    idempotent byte stores, the rest scans): two calls give bit-equal arrays. All flags set returns the mesh without its unreferenced
    vertices; none set returns empty arrays. `filter_components` is this stage with flags that are constant on a component. Device
    tensors in, device tensors out; numpy arrays / CPU tensors in, numpy arrays out, through the device. Host reads: the index check's
    min / max and the 16 bytes of the new totals. ValueError (before any launch): faces that are not [F,3] integer or hold an index
    outside [0, V), rows or a `keep` that do not match. T2NError without a GPU."""
    lib = _lib.load()
    parts = tuple(mesh)
    if not 2 <= len(parts) <= 4:
        raise ValueError(f"select_faces: a mesh of {len(parts)} parts, need (verts, faces[, normals[, colors]])")
    verts, faces, normals, colors = parts + (None,) * (4 - len(parts))
    if len(verts.shape) != 2 or verts.shape[1] != 3:
        raise ValueError(f"select_faces: verts of shape {tuple(verts.shape)}, need [V,3]")
    V = int(verts.shape[0])
    if tuple(keep.shape) != (int(faces.shape[0]),):
        raise ValueError(f"select_faces: keep of shape {tuple(keep.shape)} for faces of shape {tuple(faces.shape)}, need [F]")
    f, dev = _faces_on_device(faces, V, "select_faces")
    v = _rows(verts, V, torch.float32, dev, "verts", "select_faces")
    n = _rows(normals, V, torch.float32, dev, "normals", "select_faces")
    c = _rows(colors, V, torch.uint8, dev, "colors", "select_faces")
    k = (_as_tensor(keep).detach().to(dev) != 0).to(torch.uint8).contiguous()
    out = _select_faces(lib, v, f, n, c, k, dev)
    if _is_device(verts):
        return out
    host = lambda x: None if x is None else x.cpu().numpy()     # noqa: E731
    return Mesh(*(host(x) for x in out))


# ---- adjacency, Taubin smoothing, vertex normals -----------------------------------------------------------------------------------------
def _csr(lib, f, V, dev, edges):
    """The sorted, unique rows of checked device faces as (offsets [V+1] int64, values [E] int32): vertex -> neighbouring vertices
    (edges) or vertex -> faces. Keys row << 32 | value from one launch, a device sort, t2n_mesh_csr; the 8 bytes of E are read."""
    F = int(f.shape[0])
    n = (6 if edges else 3) * F
    if n == 0:                                                  # nothing is launched
        return torch.zeros(V + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        name = "t2n_mesh_edge_keys" if edges else "t2n_mesh_face_keys"
        _lib.check(getattr(lib, name)(_lib.ptr(f), F, V, _lib.ptr(keys), _lib.current_stream_ptr(dev)), name)
    return _csr_rows(lib, keys, V, dev)


def _csr_rows(lib, keys, n_rows, dev):
    """(offsets [n_rows+1] int64, values [E] int32) of unsorted keys row << 32 | value: a device sort, t2n_mesh_csr, the 8-byte read of E."""
    n, V = int(keys.shape[0]), int(n_rows)
    with torch.cuda.device(dev):
        stream = _lib.current_stream_ptr(dev)
        keys = torch.sort(keys).values                          # integer keys: the sorted array does not depend on how it was sorted
        nbytes = int(lib.t2n_mesh_csr_workspace_bytes(n))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        offsets = torch.empty(V + 1, dtype=torch.int64, device=dev)
        values = torch.empty(n, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(lib.t2n_mesh_csr(_lib.ptr(keys), n, V, _lib.ptr(offsets), _lib.ptr(values), _lib.ptr(count), _lib.ptr(ws), nbytes,
                                    stream), "t2n_mesh_csr")
        E = int(count.cpu().item())                             # the one 8-byte read
        return offsets, values[:E].clone()


def _smooth_faces(faces, V, who):
    f, dev = _faces_on_device(faces, V, who)
    if 6 * int(f.shape[0]) >= 2**31:
        raise ValueError(f"{who}: {f.shape[0]} faces (need 6 F < 2^31)")
    return f, dev


@torch.no_grad()
def mesh_adjacency(faces, n_verts):
    """Vertex adjacency of a triangle list as CSR: Adjacency(offsets [V+1] int64, neighbours [E] int32); row v = neighbours[offsets[v]
    : offsets[v+1]] = N(v), the u != v that share a face edge with v (both directions of {a,b}, {b,c}, {c,a}; an edge whose two ends
    are the same index is ignored; duplicate faces add nothing). Every row is sorted ascending and unique, so the arrays are a function
    of the face SET alone: face order, the rotation of a face's indices and thread order do not matter, two calls give the same bits.
    faces [F,3] integer: a device tensor (device tensors come back) or a numpy array / CPU tensor (numpy arrays come back, through the
    device). Host reads: the index check's min / max and the 8 bytes of E. ValueError: faces that are not [F,3] integer, an index
    outside [0, n_verts), 6 F >= 2^31. T2NError without a GPU."""
    lib = _lib.load()
    f, dev = _smooth_faces(faces, n_verts, "mesh_adjacency")
    off, nbr = _csr(lib, f, int(n_verts), dev, True)
    if _is_device(faces):
        return Adjacency(off, nbr)
    return Adjacency(off.cpu().numpy(), nbr.cpu().numpy())


def _vertex_normals(lib, v, f, dev):
    V, F = int(v.shape[0]), int(f.shape[0])
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    if V == 0:                                                  # nothing is launched
        return out
    off, rows = _csr(lib, f, V, dev, False)
    with torch.cuda.device(dev):
        _lib.check(lib.t2n_mesh_vertex_normals(_lib.ptr(v), _lib.ptr(f), F, _lib.ptr(off), _lib.ptr(rows), int(rows.shape[0]), V,
                                               _lib.ptr(out), _lib.current_stream_ptr(dev)), "t2n_mesh_vertex_normals")
    return out


@torch.no_grad()
def vertex_normals(verts, faces):
    """Area-weighted vertex normals [V,3] float32: n_v = sum of (x_b - x_a) x (x_c - x_a) over the faces (a, b, c) that contain v, each
    face once, in ascending face index (a sorted vertex -> face CSR, built like the adjacency), in float64 from the float32 positions;
    normalised as export_mesh(normals="field") normalises (prescale by the largest |component|, then divide by the norm) and rounded
    to float32 once. Exactly 0 for a vertex of no face or of degenerate faces only. Right-hand orientation: `marching_cubes`' (out of
    the dense region). A function of the positions and the face list with its order; two calls give the same bits. Device tensors in,
    a device tensor out; numpy arrays / CPU tensors in, a numpy array out. ValueError as `mesh_adjacency`, and for verts that are not
    [V,3]. T2NError without a GPU."""
    lib = _lib.load()
    if len(verts.shape) != 2 or verts.shape[1] != 3:
        raise ValueError(f"vertex_normals: verts of shape {tuple(verts.shape)}, need [V,3]")
    V = int(verts.shape[0])
    f, dev = _smooth_faces(faces, V, "vertex_normals")
    out = _vertex_normals(lib, _rows(verts, V, torch.float32, dev, "verts", "vertex_normals"), f, dev)
    return out if _is_device(verts) else out.cpu().numpy()


def _checked_adjacency(adjacency, V, dev):
    """A caller's Adjacency on the device, refused (ValueError) unless its rows can be walked: one host read of five integers."""
    as_t = lambda x, dt: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).detach().to(   # noqa: E731
        device=dev, dtype=dt).contiguous()
    if len(tuple(adjacency)) != 2:
        raise ValueError("smooth_mesh: adjacency is not an Adjacency(offsets, neighbours)")
    off, nbr = as_t(adjacency[0], torch.int64), as_t(adjacency[1], torch.int32)
    if tuple(off.shape) != (V + 1,) or nbr.dim() != 1:
        raise ValueError(f"smooth_mesh: adjacency of {tuple(off.shape)} offsets and {tuple(nbr.shape)} neighbours does not belong to a "
                         f"mesh of {V} vertices")
    E = int(nbr.shape[0])
    step = (off[1:] - off[:-1]).amin() if V else off.new_zeros(())
    lo, hi = torch.aminmax(nbr) if E else (nbr.new_zeros(()), nbr.new_zeros(()))
    first, last, step, lo, hi = (int(x) for x in torch.stack([off[0], off[-1], step, lo.long(), hi.long()]).cpu().tolist())
    if first != 0 or last != E or step < 0 or lo < 0 or (E and hi >= V):
        raise ValueError(f"smooth_mesh: adjacency offsets run from {first} to {last} (smallest step {step}) over {E} neighbours that "
                         f"span [{lo}, {hi}]: not the rows of a mesh of {V} vertices")
    return off, nbr


@torch.no_grad()
def smooth_mesh(mesh, iterations=10, lamb=0.5, mu=-0.53, fixed=None, adjacency=None):
    """Taubin (lambda | mu) smoothing of `mesh` (a Mesh, or (verts, faces[, normals[, colors]])), as a Mesh. One iteration is a pass with
    s = lamb followed by a pass with s = mu; the mu pass is skipped when mu == 0 (plain Laplacian smoothing, which shrinks). A pass is
    x_v <- x_v + s * (mean_{u in N(v)} x_u - x_v) over `mesh_adjacency`'s rows, in float64: the sum starts at 0.0 and runs over the row
    in its ascending order, is divided by the degree, then the subtraction, the product with s, the addition, each rounded on its own.
    A vertex without neighbours, or with fixed[v] set (`fixed`: an optional [V] bool), keeps its position. Positions stay float64
    between the passes and are rounded to float32 once at the end, so the result is a function of the positions and the face set:
    face order, index rotation and thread order do not matter, two calls give the same bits.

    Faces and colours pass through untouched. If the mesh has normals, the output's are `vertex_normals` of the smoothed mesh.
    iterations=0 returns the input's bits, normals included. `adjacency`: an earlier mesh_adjacency(faces, V) of the same faces, to
    skip building it. With floater removal the order is `filter_components` first, then `smooth_mesh`. Device tensors in, device
    tensors out; numpy arrays / CPU tensors in, numpy arrays out. ValueError (before any launch): iterations < 0, lamb outside (0, 1],
    mu > 0, faces that are not [F,3] integer or hold an index outside [0, V), rows or a `fixed` that do not match verts, an adjacency
    that is not the rows of V vertices. T2NError without a GPU."""
    parts = tuple(mesh)
    if not 2 <= len(parts) <= 4:
        raise ValueError(f"smooth_mesh: a mesh of {len(parts)} parts, need (verts, faces[, normals[, colors]])")
    verts, faces, normals, colors = parts + (None,) * (4 - len(parts))
    if int(iterations) != iterations or int(iterations) < 0:
        raise ValueError(f"smooth_mesh: iterations {iterations!r} (an integer >= 0)")
    lamb, mu = float(lamb), float(mu)
    if not 0.0 < lamb <= 1.0:
        raise ValueError(f"smooth_mesh: lamb {lamb} outside (0, 1]")
    if not (mu <= 0.0 and math.isfinite(mu)):
        raise ValueError(f"smooth_mesh: mu {mu} (finite and <= 0; 0 skips the pass)")
    if len(verts.shape) != 2 or verts.shape[1] != 3:
        raise ValueError(f"smooth_mesh: verts of shape {tuple(verts.shape)}, need [V,3]")
    V = int(verts.shape[0])
    if fixed is not None and tuple(fixed.shape) != (V,):
        raise ValueError(f"smooth_mesh: fixed of shape {tuple(fixed.shape)} for {V} vertices, need [V]")
    lib = _lib.load()
    f, dev = _smooth_faces(faces, V, "smooth_mesh")
    v = _rows(verts, V, torch.float32, dev, "verts", "smooth_mesh")
    n = _rows(normals, V, torch.float32, dev, "normals", "smooth_mesh")
    c = _rows(colors, V, torch.uint8, dev, "colors", "smooth_mesh")
    fx = None
    if fixed is not None:
        fx = (fixed if isinstance(fixed, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(fixed))).detach().to(dev)
        fx = (fx != 0).to(torch.uint8).contiguous()
    adj = None if adjacency is None else _checked_adjacency(adjacency, V, dev)
    if int(iterations) > 0 and V > 0:
        off, nbr = adj if adj is not None else _csr(lib, f, V, dev, True)
        with torch.cuda.device(dev):
            stream = _lib.current_stream_ptr(dev)
            x = v.to(torch.float64)
            y = torch.empty_like(x)
            for _ in range(int(iterations)):
                for s in (lamb, mu):
                    if s == 0.0:
                        continue
                    _lib.check(lib.t2n_mesh_smooth_pass(_lib.ptr(x), _lib.ptr(y), _lib.ptr(off), _lib.ptr(nbr), int(nbr.shape[0]),
                                                        _lib.ptr(fx), V, s, stream), "t2n_mesh_smooth_pass")
                    x, y = y, x
            v = x.to(torch.float32)                             # the one rounding
        if n is not None:
            n = _vertex_normals(lib, v, f, dev)
    if _is_device(verts):
        return Mesh(v, f, n, c)
    host = lambda x: None if x is None else x.cpu().numpy()     # noqa: E731
    return Mesh(host(v), host(f), host(n), host(c))


# ---- simplification: vertex clustering with quadric placement ---------------------------------------------------------------------------
def _as_tensor(x):
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))


def _cluster_grid(verts, cell, origin, who):
    """(positions as a float32 tensor where they live, o [3], h [3], dims [3]) of a clustering: every refusal of the definition, from
    the arguments and one aminmax of the positions (six floats on the host); dims is None for V == 0. No launch of the library's."""
    try:
        h = [float(t) for t in np.asarray(cell.detach().cpu() if isinstance(cell, torch.Tensor) else cell, dtype=np.float64).reshape(-1)]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: cell {cell!r} (a positive finite scalar or three)") from None
    if len(h) == 1:
        h = h * 3
    if len(h) != 3 or not all(math.isfinite(t) and t > 0 for t in h):
        raise ValueError(f"{who}: cell {cell!r} (a positive finite scalar or three)")
    if len(verts.shape) != 2 or verts.shape[1] != 3:
        raise ValueError(f"{who}: verts of shape {tuple(verts.shape)}, need [V,3]")
    o = None
    if origin is not None:
        o = _three(origin, "origin")
        if not all(math.isfinite(t) for t in o):
            raise ValueError(f"{who}: origin {o} is not finite")
    v = _as_tensor(verts).detach().to(torch.float32)
    if int(v.shape[0]) >= 2**31:
        raise ValueError(f"{who}: {v.shape[0]} vertices (need V < 2^31)")
    if v.shape[0] == 0:
        return v, o or [0.0, 0.0, 0.0], h, None
    lo, hi = torch.aminmax(v, dim=0)
    lo, hi = (([float(t) for t in x]) for x in torch.stack([lo, hi]).cpu().tolist())      # the one read: six floats
    if not all(math.isfinite(t) for t in lo + hi):
        raise ValueError(f"{who}: a vertex is not finite (the positions span {lo} to {hi})")
    if o is None:
        o = lo
    elif any(a < b for a, b in zip(lo, o)):
        raise ValueError(f"{who}: a vertex at {lo} lies below the origin {o}")
    top = [(b - a) / s for a, b, s in zip(o, hi, h)]           # the device's own operations on the largest coordinate
    if not all(math.isfinite(t) for t in top):
        raise ValueError(f"{who}: a cell of {h} over positions up to {hi} gives 2^31 cells and more")
    dims = [int(math.floor(t)) + 1 for t in top]
    if dims[0] * dims[1] * dims[2] >= 2**31:
        raise ValueError(f"{who}: a grid of {dims} cells (need n0 n1 n2 < 2^31)")
    return v, o, h, dims


def _clusters(lib, v, dev, o, h, dims):
    """Clusters of checked device positions [V,3] float32, V > 0; device tensors. Reads the 8 bytes of K."""
    V = int(v.shape[0])
    with torch.cuda.device(dev):
        stream = _lib.current_stream_ptr(dev)
        d3 = (C.c_int32 * 3)(*dims)
        keys = torch.empty(V, dtype=torch.int64, device=dev)
        _lib.check(lib.t2n_mesh_cluster_keys(_lib.ptr(v), V, (C.c_double * 3)(*o), (C.c_double * 3)(*h), d3, _lib.ptr(keys), stream),
                   "t2n_mesh_cluster_keys")
        keys = torch.sort(keys).values                          # integer keys: the sorted array does not depend on how it was sorted
        nbytes = int(lib.t2n_mesh_cluster_rows_workspace_bytes(V))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        vmap = torch.empty(V, dtype=torch.int32, device=dev)
        off = torch.empty(V + 1, dtype=torch.int64, device=dev)
        mem = torch.empty(V, dtype=torch.int32, device=dev)
        cells = torch.empty(V, 3, dtype=torch.int32, device=dev)
        k = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.check(lib.t2n_mesh_cluster_rows(_lib.ptr(keys), V, d3, _lib.ptr(vmap), _lib.ptr(off), _lib.ptr(mem), _lib.ptr(cells), _lib.ptr(k),
                                             _lib.ptr(ws), nbytes, stream), "t2n_mesh_cluster_rows")
        K = int(k.cpu().item())                                 # the one 8-byte read
        return Clusters(vmap, K, off[:K + 1].clone(), mem, cells[:K].clone())


def _empty_clusters(dev):
    return Clusters(torch.empty(0, dtype=torch.int32, device=dev), 0, torch.zeros(1, dtype=torch.int64, device=dev),
                    torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev))


def _clusters_to_host(c):
    return Clusters(c.vertex_map.cpu().numpy(), c.n_clusters, c.offsets.cpu().numpy(), c.members.cpu().numpy(), c.cells.cpu().numpy())


@torch.no_grad()
def mesh_clusters(verts, cell, origin=None):
    """The clusters of a uniform grid over `verts` [V,3]: Clusters(vertex_map [V] int32, n_clusters K, offsets [K+1] int64, members [V]
    int32, cells [K,3] int32). `cell` is the grid's spacing in world units, a positive finite scalar or three values; `origin` (three
    values) defaults to the componentwise minimum of the positions. Vertex v lies in cell c_k = floor(((double)x_k - o_k) / h_k),
    every step a single float64 operation; with n_k = max c_k + 1 the cell's id is (c0 n1 + c1) n2 + c2. Clusters are the occupied
    cells, numbered 0 .. K-1 in ascending id, so the numbering is a function of the positions and the grid alone; row k of `members`
    (members[offsets[k] : offsets[k+1]]) holds cluster k's vertices in ascending index, cells[k] its (c0, c1, c2). V == 0 gives empty
    arrays and launches nothing. Device tensors in, device tensors out; numpy arrays / CPU tensors in, numpy arrays out, through the
    device. Host reads: the positions' min / max and the 8 bytes of K. ValueError (before any launch): a cell that is not finite and
    positive, a vertex that is not finite, a vertex below a given origin, n0 n1 n2 >= 2^31, verts that are not [V,3]. T2NError
    without a GPU."""
    v, o, h, dims = _cluster_grid(verts, cell, origin, "mesh_clusters")
    lib = _lib.load()
    dev = v.device if v.is_cuda else _device()
    c = _empty_clusters(dev) if dims is None else _clusters(lib, v.to(dev).contiguous(), dev, o, h, dims)
    return c if _is_device(verts) else _clusters_to_host(c)


def _checked_clusters(clusters, V, dev):
    """A caller's Clusters on the device, refused (ValueError) unless its rows can be walked: one host read of eight integers."""
    as_t = lambda x, dt: _as_tensor(x).detach().to(device=dev, dtype=dt).contiguous()      # noqa: E731
    if len(tuple(clusters)) != 5:
        raise ValueError("simplify_mesh: clusters is not a Clusters(vertex_map, n_clusters, offsets, members, cells)")
    K = int(clusters[1])
    vmap, off, mem, cells = as_t(clusters[0], torch.int32), as_t(clusters[2], torch.int64), as_t(clusters[3], torch.int32), as_t(clusters[4], torch.int32)
    if not 0 <= K <= V or (K == 0) != (V == 0) or tuple(vmap.shape) != (V,) or tuple(off.shape) != (K + 1,) or tuple(mem.shape) != (V,) or \
            tuple(cells.shape) != (K, 3):
        raise ValueError(f"simplify_mesh: clusters of {tuple(vmap.shape)} map entries, {K} clusters, {tuple(off.shape)} offsets, "
                         f"{tuple(mem.shape)} members and {tuple(cells.shape)} cells do not belong to a mesh of {V} vertices")
    if V:
        step = (off[1:] - off[:-1]).amin()
        (mlo, mhi), (vlo, vhi) = torch.aminmax(mem), torch.aminmax(vmap)
        first, last, step, mlo, mhi, vlo, vhi, clo = (int(x) for x in torch.stack(
            [off[0], off[-1], step, mlo.long(), mhi.long(), vlo.long(), vhi.long(), cells.amin().long()]).cpu().tolist())
        if first != 0 or last != V or step < 1 or mlo < 0 or mhi >= V or vlo < 0 or vhi >= K or clo < 0:
            raise ValueError(f"simplify_mesh: cluster offsets run from {first} to {last} (smallest step {step}) over members that span "
                             f"[{mlo}, {mhi}] and a map that spans [{vlo}, {vhi}]: not the {K} clusters of a mesh of {V} vertices")
    return Clusters(vmap, K, off, mem, cells)


@torch.no_grad()
def simplify_mesh(mesh, cell, origin=None, placement="quadric", regularisation=1e-3, clusters=None):
    """`mesh` (a Mesh, or (verts, faces[, normals[, colors]])) simplified by vertex clustering on a uniform grid of spacing `cell`
    (Lindstrom's out-of-core simplification), as a Mesh: one output vertex per occupied cell, in `mesh_clusters`' order (`cell` and
    `origin` as there). No priority queue, float64 sums in a fixed order, no float atomics: the output is a function of the input
    alone, two calls give the same bits.

    Position of cluster k. placement="mean": the float64 sum of its members' positions in ascending vertex index, divided by the
    count, rounded to float32 once. placement="quadric": the point closest (in the squared-area-weighted sense) to the planes of the
    input faces with at least one corner in the cluster, each face once, in ascending face index: with the face's corners rotated so
    that the smallest vertex index comes first, n = (x_b - x_a) x (x_c - x_a) in float64 from the float32 positions, unnormalised (no
    square root anywhere; a face whose n is zero or not finite is skipped), r = n . (x_a - mean), A += n n^T, b += n r; t = trace A;
    (A + regularisation t I) x = b by cofactors in the order include/t2n.h fixes; p = mean + x. The Tikhonov term pulls flat and
    creased clusters towards the mean and keeps the system positive definite. p is the representative if it lies in the cluster's
    cell [o + c h, o + (c + 1) h] on every axis; otherwise, and when t is not > 0 or not finite (a cluster without faces), the mean.

    Faces: every index goes through vertex_map; a face with two equal mapped indices is dropped; the rest are rotated so that the
    smallest index comes first (cyclic order kept); of faces with the same rotated triple only the one with the lowest input index
    stays (an oppositely oriented twin (a, c, b) is a different triangle and stays); kept faces keep their relative order. Colours:
    per channel (sum of the members + count / 2) / count in integers. Normals, if the mesh has them, are `vertex_normals` of the
    output. The positions do not depend on the rotation of a face's indices; face order enters through the order of the float64 sums.

    Clustering does NOT preserve manifoldness: two sheets that pass through one cell are welded, and an edge may end up with more
    than two faces. The documented order is `filter_components`, `smooth_mesh`, then `simplify_mesh`. `clusters`: an earlier
    mesh_clusters(verts, cell, origin) of the same arguments, to skip building it. Device tensors in, device tensors out; numpy
    arrays / CPU tensors in, numpy arrays out, through the device; normals and colours that are None stay None. Host reads: the
    positions' min / max, the 8 bytes of K, of the face rows' length and of F', and the index check's min / max. ValueError (before
    any launch): as `mesh_clusters`; a placement other than "mean" / "quadric"; a regularisation that is negative or not finite; faces
    that are not [F,3] integer or hold an index outside [0, V); rows that do not match verts; clusters that are not the rows of V
    vertices. T2NError without a GPU."""
    parts = tuple(mesh)
    if not 2 <= len(parts) <= 4:
        raise ValueError(f"simplify_mesh: a mesh of {len(parts)} parts, need (verts, faces[, normals[, colors]])")
    verts, faces, normals, colors = parts + (None,) * (4 - len(parts))
    if placement not in ("mean", "quadric"):
        raise ValueError(f"simplify_mesh: placement {placement!r} (\"mean\" or \"quadric\")")
    reg = float(regularisation)
    if not (reg >= 0.0 and math.isfinite(reg)):
        raise ValueError(f"simplify_mesh: regularisation {regularisation!r} (finite and >= 0)")
    v, o, h, dims = _cluster_grid(verts, cell, origin, "simplify_mesh")
    V = int(v.shape[0])
    lib = _lib.load()
    f, dev = _faces_on_device(faces, V, "simplify_mesh")
    F = int(f.shape[0])
    v = v.to(dev).contiguous()
    n = _rows(normals, V, torch.float32, dev, "normals", "simplify_mesh")
    c = _rows(colors, V, torch.uint8, dev, "colors", "simplify_mesh")
    if clusters is not None:
        cl = _checked_clusters(clusters, V, dev)
    else:
        cl = _empty_clusters(dev) if V == 0 else _clusters(lib, v, dev, o, h, dims)
    K = cl.n_clusters
    out_v = torch.empty(K, 3, dtype=torch.float32, device=dev)
    out_f = torch.empty(0, 3, dtype=torch.int32, device=dev)
    out_c = None if c is None else torch.empty(K, 3, dtype=torch.uint8, device=dev)
    if K > 0:                                                   # nothing is launched on an empty mesh
        quadric = placement == "quadric"
        foff = frow = None
        if quadric:
            keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
            with torch.cuda.device(dev):
                _lib.check(lib.t2n_mesh_cluster_face_keys(_lib.ptr(f), F, V, _lib.ptr(cl.vertex_map), K, _lib.ptr(keys),
                                                          _lib.current_stream_ptr(dev)), "t2n_mesh_cluster_face_keys")
            foff, frow = (_csr_rows(lib, keys, K, dev) if F else
                          (torch.zeros(K + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)))
        with torch.cuda.device(dev):
            stream = _lib.current_stream_ptr(dev)
            p = _lib.ptr
            _lib.check(lib.t2n_mesh_cluster_place(p(v), V, p(f), F, p(cl.offsets), p(cl.members), V, p(cl.cells), K, p(foff), p(frow),
                                                  int(frow.shape[0]) if quadric else 0, (C.c_double * 3)(*o), (C.c_double * 3)(*h), reg,
                                                  1 if quadric else 0, p(out_v), stream), "t2n_mesh_cluster_place")
            if c is not None:
                _lib.check(lib.t2n_mesh_cluster_colors(p(c), V, p(cl.offsets), p(cl.members), V, K, p(out_c), stream), "t2n_mesh_cluster_colors")
            if F > 0:
                rot = torch.empty(F, 3, dtype=torch.int32, device=dev)
                key_hi = torch.empty(F, dtype=torch.int64, device=dev)
                key_lo = torch.empty(F, dtype=torch.int64, device=dev)
                _lib.check(lib.t2n_mesh_simplify_face_map(p(f), F, V, p(cl.vertex_map), K, p(rot), p(key_hi), p(key_lo), stream),
                           "t2n_mesh_simplify_face_map")
                # two stable integer sorts, least significant key first: equal triples end up together in ascending face index
                by_lo = torch.sort(key_lo, stable=True).indices
                order = by_lo[torch.sort(key_hi[by_lo], stable=True).indices].contiguous()
                nbytes = int(lib.t2n_mesh_simplify_faces_workspace_bytes(F))
                ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                kept = torch.empty(F, 3, dtype=torch.int32, device=dev)
                count = torch.empty(1, dtype=torch.int64, device=dev)
                _lib.check(lib.t2n_mesh_simplify_faces(p(rot), p(order), F, p(kept), p(count), p(ws), nbytes, stream), "t2n_mesh_simplify_faces")
                out_f = kept[:int(count.cpu().item())].clone()          # the one 8-byte read
    out_n = None if n is None else _vertex_normals(lib, out_v, out_f, dev)
    if _is_device(verts):
        return Mesh(out_v, out_f, out_n, out_c)
    host = lambda x: None if x is None else x.cpu().numpy()     # noqa: E731
    return Mesh(host(out_v), host(out_f), host(out_n), host(out_c))


def _host(x, dtype):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=dtype)


def write_ply(path, verts, faces, normals=None, colors=None):
    """Binary little-endian PLY: vertex properties `float x y z`, with `normals` `float nx ny nz`, with `colors` `uchar red green
    blue`; faces as `property list uchar int vertex_indices` (plyfile's names). verts [V,3], faces [F,3], normals [V,3], colors [V,3]
    uint8: numpy arrays or tensors. Two structured arrays and two `tofile` calls: no loop per element."""
    v, f = _host(verts, "<f4"), _host(faces, "<i4")
    n, c = _host(normals, "<f4"), _host(colors, "u1")
    if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3:
        raise ValueError(f"write_ply: verts {v.shape} and faces {f.shape}, need [V,3] and [F,3]")
    for name, a in (("normals", n), ("colors", c)):
        if a is not None and a.shape != v.shape:
            raise ValueError(f"write_ply: {name} of shape {a.shape} for verts of shape {v.shape}")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}", "property float x", "property float y",
            "property float z"]
    if n is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        head += ["property float nx", "property float ny", "property float nz"]
    if c is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    vrec = np.empty(v.shape[0], dtype=np.dtype(fields))
    for k, name in enumerate(("x", "y", "z")):
        vrec[name] = v[:, k]
    if n is not None:
        for k, name in enumerate(("nx", "ny", "nz")):
            vrec[name] = n[:, k]
    if c is not None:
        for k, name in enumerate(("red", "green", "blue")):
            vrec[name] = c[:, k]
    frec = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    frec["n"] = 3
    frec["v"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        vrec.tofile(fh)
        frec.tofile(fh)


def convert_sdf_samples_to_ply(pytorch_3d_sdf_tensor, ply_filename_out, bbox, level=0.5, offset=None, scale=None):
    """The reference's function (utils.py:512-572) with the device marching cubes in skimage's place and `write_ply` in plyfile's.
    Its arithmetic is kept, in float32: voxel_size = (bbox[1] - bbox[0]) / shape (shape, not shape - 1: upstream's quirk, the mesh is
    (n - 1) / n of the box it samples), points = bbox[0] + verts, then / scale, then - offset. The volume may be a CPU tensor (as
    upstream hands it over), a device tensor or a numpy array.

    Faces are written so that their right-hand normals point to lower values. The reference reverses skimage's faces ("inverse face
    orientation"), which reads as aiming at the same orientation; skimage is not available where this was written, so that could NOT
    be checked against it. An empty surface raises T2NError (the reference: skimage's ValueError)."""
    b = bbox.detach().cpu().numpy() if isinstance(bbox, torch.Tensor) else np.asarray(bbox)
    b = b.astype(np.float32).reshape(2, 3)
    shape = np.array(tuple(pytorch_3d_sdf_tensor.shape), dtype=np.float32)
    voxel_size = ((b[1] - b[0]).astype(np.float32) / shape).astype(np.float32)
    verts, faces, _ = marching_cubes(pytorch_3d_sdf_tensor, level, spacing=[float(s) for s in voxel_size], normals=False)
    if isinstance(verts, torch.Tensor):
        verts, faces = verts.cpu().numpy(), faces.cpu().numpy()
    if verts.shape[0] == 0:
        raise _lib.T2NError(f"convert_sdf_samples_to_ply: no surface at level {level}")
    mesh_points = np.zeros_like(verts)
    mesh_points[:, 0] = b[0, 0] + verts[:, 0]
    mesh_points[:, 1] = b[0, 1] + verts[:, 1]
    mesh_points[:, 2] = b[0, 2] + verts[:, 2]
    if scale is not None:
        mesh_points = (mesh_points / np.asarray(scale, dtype=np.float32)).astype(np.float32)
    if offset is not None:
        off = offset.detach().cpu().numpy() if isinstance(offset, torch.Tensor) else np.asarray(offset)
        mesh_points = (mesh_points - off.astype(np.float32)).astype(np.float32)
    print("saving mesh to %s" % (ply_filename_out))
    write_ply(ply_filename_out, mesh_points, faces)
