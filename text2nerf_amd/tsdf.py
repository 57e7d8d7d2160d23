"""TSDF fusion of depth views on the device (csrc/t2n_tsdf.hip; definitions in include/t2n.h): the mesh route for a scene whose
trustworthy surface is its rendered depth rather than a level of alpha. Depth maps (and colours) from known poses are integrated into a
truncated signed distance volume, and the zero level is meshed only where the volume was observed; users of the reference do this on the
host with Open3D after dumping depth maps.

    tsdf_integrate   depth views -> TSDFVolume(tsdf, weight, color, origin, spacing, trunc); `volume=` continues an earlier one
    tsdf_mesh        TSDFVolume -> mesh.Mesh: marching cubes of the zero level, faces kept where their cell was observed
    world_to_camera  c2w poses -> the [V,12] float64 rows the kernel reads (inverted on the host)

The volume's frame is marching_cubes': node (a,b,c) at origin + (a,b,c) * spacing, float32 values. All arithmetic is float64 in a fixed
order, the state float32 and rounded after every view: V calls of one view equal one call of V views bit for bit, two calls give the same
bits, no atomics. Device tensors in, device tensors out; numpy arrays / CPU tensors in, numpy arrays out, through the device. No CPU
fallback. The documented route:

    vol = tensorf.tsdf_volume(poses, intrinsic, H, W)          # or tsdf_integrate(depths, poses, ...) on the pipeline's own RGB-D
    m = tsdf_mesh(vol)                                         # observed cells only: no shell behind the surface, no fog
    m = filter_components(m, keep_largest=1)                   # optional, then smooth_mesh / simplify_mesh as for export_mesh
    write_ply("scene.ply", *m)"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from . import mesh as M

DEPTH_KINDS = {"ray": 0, "z": 1}     # the renderer returns the distance along the ray, the warp stages treat depth as camera z


class TSDFVolume(NamedTuple):
    tsdf: torch.Tensor                  # [n0,n1,n2] float32 in [-1, 1]; 1 where nothing was integrated
    weight: torch.Tensor                # [n0,n1,n2] float32 >= 0; 0 where nothing was integrated
    color: Optional[torch.Tensor]       # [n0,n1,n2,3] float32, or None
    origin: tuple                       # three floats (float32 values): node (0,0,0)
    spacing: tuple                      # three floats (float32 values)
    trunc: float                        # the truncation distance, world units


def _f32_three(x, what):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().tolist()
    v = np.asarray(x, dtype=np.float64).reshape(-1)
    if v.shape[0] != 3:
        raise ValueError(f"tsdf: {what} needs three values, got {v.shape[0]}")
    with np.errstate(over="ignore"):
        return tuple(float(np.float32(t)) for t in v)


def _frame(origin, spacing, shape, trunc):
    """(origin, spacing, shape, trunc) checked: every refusal of the frame, no device involved."""
    o, s = _f32_three(origin, "origin"), _f32_three(spacing, "spacing")
    try:
        n = tuple(int(t) for t in shape)
    except (TypeError, ValueError):
        raise ValueError(f"tsdf: shape {shape!r} (three integers)") from None
    if len(n) != 3 or min(n) < 1:
        raise ValueError(f"tsdf: shape {n} (three dimensions >= 1)")
    if n[0] * n[1] * n[2] >= 2**31:
        raise ValueError(f"tsdf: a grid of {n} has 2^31 nodes and more")
    if not all(math.isfinite(t) and t > 0 for t in s):
        raise ValueError(f"tsdf: spacing {s} (finite and positive)")
    if not all(math.isfinite(t) for t in o):
        raise ValueError(f"tsdf: origin {o} is not finite")
    trunc = float(trunc)
    if not (math.isfinite(trunc) and trunc > 0):
        raise ValueError(f"tsdf: trunc {trunc} (finite and positive)")
    return o, s, n, trunc


def world_to_camera(poses):
    """[V,12] float64: the rows of the 3x4 world-to-camera matrix of every camera-to-world pose in `poses` ([V,3,4] or [V,4,4]; OpenCV
    convention, z forward: `generate_rays`'), each 4x4 inverted on the host by numpy in float64. ValueError for a pose that is not
    finite or not invertible."""
    p = poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else np.asarray(poses)
    if p.ndim != 3 or p.shape[1] not in (3, 4) or p.shape[2] != 4:
        raise ValueError(f"tsdf: poses of shape {tuple(p.shape)}, need [V,3,4] or [V,4,4]")
    out = np.zeros((p.shape[0], 12), np.float64)
    for v in range(p.shape[0]):
        m = np.eye(4, dtype=np.float64)
        m[:3] = p[v, :3].astype(np.float64)
        if not np.isfinite(m).all():
            raise ValueError(f"tsdf: pose {v} is not finite")
        try:
            inv = np.linalg.inv(m)
        except np.linalg.LinAlgError:
            raise ValueError(f"tsdf: pose {v} is not invertible") from None
        if not np.isfinite(inv).all():
            raise ValueError(f"tsdf: pose {v} is not invertible")
        out[v] = inv[:3].reshape(12)
    return out


def _views(x, shape, dev, what):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"tsdf: {what} of shape {tuple(t.shape)}, need {tuple(shape)}")
    return t if dev is None else t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _state(x, shape, dev, what):
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"tsdf: the volume's {what} of shape {tuple(t.shape)}, need {tuple(shape)}")
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _c3(v):
    return (C.c_float * 3)(*v)


@torch.no_grad()
def tsdf_integrate(depths, poses, intrinsic, origin, spacing, shape, trunc, colors=None, weights=None, depth_kind="ray", near=0.0,
                   max_weight=None, volume=None):
    """Integrate V depth views into a TSDF volume of `shape` nodes (node (a,b,c) at origin + (a,b,c) * spacing) and return it as a
    TSDFVolume. depths [V,H,W] (a pixel that is 0, negative or not finite is no measurement), poses [V,3,4] or [V,4,4] camera-to-world,
    intrinsic (fx, fy, cx, cy) with pixel i spanning [i, i+1) as in `generate_rays`; colors [V,H,W,3] in [0,1] (the volume then carries a
    colour), weights [V,H,W] (per-pixel weights instead of 1; a pixel that is 0, negative or not finite is skipped). depth_kind "ray":
    depth is the distance along the ray (what the renderer returns), "z": the camera-space z (what the warp stages use). A node takes the
    views in their order: camera point p, skipped unless p_z > near and its nearest pixel holds a measurement d; sdf = d - |p| (or d -
    p_z), skipped if sdf < -trunc; tsdf <- (W tsdf + w min(1, sdf / trunc)) / (W + w), colour alike, W <- min(W + w, max_weight), in
    float64 with the state rounded to float32 after every view (include/t2n.h has every operation): views one at a time give the bits of
    all at once. `volume`: a TSDFVolume of the same frame and trunc to continue; device tensors are updated IN PLACE and returned. V = 0
    returns the fresh or given volume unchanged. ValueError (before any launch): shapes that do not match, a trunc or spacing that is not
    finite and positive, fx or fy zero or an intrinsic that is not finite, a pose that is not finite or not invertible, an unknown
    depth_kind, a max_weight that is not > 0, 2^31 nodes and more, a `volume` of another frame, trunc or colour state. T2NError without a
    GPU."""
    o, s, n, trunc = _frame(origin, spacing, shape, trunc)
    if depth_kind not in DEPTH_KINDS:
        raise ValueError(f"tsdf_integrate: depth_kind {depth_kind!r} ({' or '.join(repr(k) for k in DEPTH_KINDS)})")
    if len(depths.shape) != 3 or min(int(t) for t in depths.shape[1:]) < 1:
        raise ValueError(f"tsdf_integrate: depths of shape {tuple(depths.shape)}, need [V,H,W]")
    V, H, W = (int(t) for t in depths.shape)
    try:
        fx, fy, cx, cy = (float(t) for t in (intrinsic.detach().cpu().tolist() if isinstance(intrinsic, torch.Tensor) else intrinsic))
    except (TypeError, ValueError):
        raise ValueError(f"tsdf_integrate: intrinsic {intrinsic!r} (fx, fy, cx, cy)") from None
    if not all(math.isfinite(t) for t in (fx, fy, cx, cy)) or fx == 0.0 or fy == 0.0:
        raise ValueError(f"tsdf_integrate: intrinsic {(fx, fy, cx, cy)} (finite, fx and fy not zero)")
    near = float(near)
    if not math.isfinite(near):
        raise ValueError(f"tsdf_integrate: near {near} is not finite")
    cap = math.inf if max_weight is None else float(max_weight)
    if not cap > 0:
        raise ValueError(f"tsdf_integrate: max_weight {max_weight!r} (> 0, or None for no cap)")
    w2c = world_to_camera(poses)
    if w2c.shape[0] != V:
        raise ValueError(f"tsdf_integrate: {w2c.shape[0]} poses for {V} depth views")
    _views(depths, (V, H, W), None, "depths")
    if colors is not None:
        _views(colors, (V, H, W, 3), None, "colors")
    if weights is not None:
        _views(weights, (V, H, W), None, "weights")
    if volume is not None:
        if len(tuple(volume)) != 6:
            raise ValueError("tsdf_integrate: volume is not a TSDFVolume(tsdf, weight, color, origin, spacing, trunc)")
        if tuple(volume.tsdf.shape) != n or tuple(volume.origin) != o or tuple(volume.spacing) != s or float(volume.trunc) != trunc:
            raise ValueError(f"tsdf_integrate: the volume's frame (shape {tuple(volume.tsdf.shape)}, origin {tuple(volume.origin)}, spacing "
                             f"{tuple(volume.spacing)}, trunc {volume.trunc}) is not this call's ({n}, {o}, {s}, {trunc})")
        if V > 0 and (volume.color is None) != (colors is None):
            raise ValueError("tsdf_integrate: colours on one side only (the volume's colour state and this call's `colors`)")
        if V == 0:
            return volume
    on_device = M._is_device(depths)
    lib = _lib.load()
    dev = depths.device if on_device else M._device()
    with torch.cuda.device(dev):
        if volume is None:
            T = torch.ones(n, dtype=torch.float32, device=dev)
            Wt = torch.zeros(n, dtype=torch.float32, device=dev)
            Cl = None if colors is None else torch.zeros(n + (3,), dtype=torch.float32, device=dev)
        else:
            T, Wt = _state(volume.tsdf, n, dev, "tsdf"), _state(volume.weight, n, dev, "weight")
            Cl = None if volume.color is None else _state(volume.color, n + (3,), dev, "color")
        if V > 0:
            d = _views(depths, (V, H, W), dev, "depths")
            rgb = None if colors is None else _views(colors, (V, H, W, 3), dev, "colors")
            pw = None if weights is None else _views(weights, (V, H, W), dev, "weights")
            mats = torch.from_numpy(w2c).to(dev)
            p = _lib.ptr
            _lib.check(lib.t2n_tsdf_integrate(p(T), p(Wt), p(Cl), n[0], n[1], n[2], p(d), p(rgb), p(pw), p(mats), V, H, W, fx, fy, cx, cy,
                                              _c3(o), _c3(s), trunc, near, cap, DEPTH_KINDS[depth_kind], _lib.current_stream_ptr(dev)),
                       "t2n_tsdf_integrate")
            if not on_device:
                torch.cuda.current_stream(dev).synchronize()    # `mats` and the uploads go out of scope behind the launch
    if on_device:
        return TSDFVolume(T, Wt, Cl, o, s, trunc)
    return TSDFVolume(T.cpu().numpy(), Wt.cpu().numpy(), None if Cl is None else Cl.cpu().numpy(), o, s, trunc)


@torch.no_grad()
def tsdf_mesh(volume, min_weight=0.0, normals=True, colors=True):
    """The observed zero level of a TSDFVolume as a mesh.Mesh: `marching_cubes(-tsdf, 0.0, spacing, origin)` (inside is tsdf < 0; the
    negation is exact, the faces' right-hand normals point out of the surface, towards the cameras), then only the faces whose cell
    was observed stay (`select_faces`): the cell that holds the face's centroid must have weight > min_weight at all eight corners.
    That removes what marching cubes makes of the jump to the untouched nodes (tsdf 1): the shell at -trunc behind every surface and
    the walls at the edge of the views. colors: the volume's colour at the vertices, trilinear over the observed corners of the
    vertex's cell, uint8 (None if the volume has none or colors=False). normals=True: `vertex_normals` of the SELECTED mesh; the
    volume's finite differences are polluted by that jump. An empty result is empty arrays. Device tensors in, device tensors out;
    numpy in, numpy out, through the device. ValueError: a volume whose parts do not match, a dimension < 2, a min_weight that is NaN.
    T2NError without a GPU."""
    if len(tuple(volume)) != 6:
        raise ValueError("tsdf_mesh: volume is not a TSDFVolume(tsdf, weight, color, origin, spacing, trunc)")
    o, s, n, _ = _frame(volume.origin, volume.spacing, tuple(volume.tsdf.shape), volume.trunc)
    if min(n) < 2:
        raise ValueError(f"tsdf_mesh: a volume of shape {n} (every dimension >= 2)")
    min_weight = float(min_weight)
    if math.isnan(min_weight):
        raise ValueError("tsdf_mesh: min_weight is NaN")
    if tuple(volume.weight.shape) != n or (volume.color is not None and tuple(volume.color.shape) != n + (3,)):
        raise ValueError(f"tsdf_mesh: weight / color do not match a tsdf of shape {n}")
    on_device = M._is_device(volume.tsdf)
    lib = _lib.load()
    dev = volume.tsdf.device if on_device else M._device()
    T, Wt = _state(volume.tsdf, n, dev, "tsdf"), _state(volume.weight, n, dev, "weight")
    Cl = _state(volume.color, n + (3,), dev, "color") if colors and volume.color is not None else None
    verts, faces, _ = M.marching_cubes(-T, 0.0, spacing=s, origin=o, normals=False)
    Vn, F = int(verts.shape[0]), int(faces.shape[0])
    p = _lib.ptr
    with torch.cuda.device(dev):
        stream = _lib.current_stream_ptr(dev)
        keep = torch.empty(F, dtype=torch.uint8, device=dev)
        if F > 0:                                               # nothing is launched on an empty mesh
            _lib.check(lib.t2n_tsdf_face_flags(p(verts), Vn, p(faces), F, p(Wt), n[0], n[1], n[2], _c3(o), _c3(s), min_weight, p(keep),
                                               stream), "t2n_tsdf_face_flags")
        sel = M._select_faces(lib, verts, faces, None, None, keep, dev)
        rgb8 = None
        if Cl is not None:
            rgb8 = torch.empty(sel.verts.shape[0], 3, dtype=torch.uint8, device=dev)
            if sel.verts.shape[0] > 0:
                _lib.check(lib.t2n_tsdf_sample_colors(p(sel.verts), int(sel.verts.shape[0]), p(Wt), p(Cl), n[0], n[1], n[2], _c3(o), _c3(s),
                                                      min_weight, p(rgb8), stream), "t2n_tsdf_sample_colors")
    nrm = M._vertex_normals(lib, sel.verts, sel.faces, dev) if normals else None
    out = M.Mesh(sel.verts, sel.faces, nrm, rgb8)
    if on_device:
        return out
    return M.Mesh(*(None if x is None else x.cpu().numpy() for x in out))
