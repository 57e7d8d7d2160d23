"""Mesh export on the device: marching cubes over a dense volume (csrc/t2n_mesh.hip, `t2n_mc_count` / `t2n_mc_emit`) and a PLY
writer, in the place of `skimage.measure.marching_cubes` on a host copy followed by a Python loop per vertex and per face into
`plyfile` records (`convert_sdf_samples_to_ply`, utils.py:512-572). Neither package is needed.

    marching_cubes               volume, level -> (verts, faces, normals); device tensors in, device tensors out
    convert_sdf_samples_to_ply   the reference's function, signature and defaults (tests/golden/mesh_signatures.json)
    write_ply                    binary little-endian PLY by numpy `tofile`, property names as plyfile writes them
    Mesh                         what `TensorBase.export_mesh` returns: verts, faces, normals, colors

The meshes are closed oriented 2-manifolds (the case table is generated from rules, tools/gen_mc_table.py); the right-hand normal of
every triangle, and every vertex normal, points towards LOWER values: out of the dense region of an alpha volume. Vertex and face order
are functions of the input alone (no atomics): two calls give bit-equal arrays. No CPU fallback."""
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


def _device():
    if not torch.cuda.is_available():
        raise _lib.T2NError("marching_cubes runs on the MI355X only (no CPU fallback)")
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
