"""Connected components of a dense volume on the device (csrc/t2n_volume.hip) and the filter that removes the unwanted ones, in the
place of `scipy.ndimage.label` on a host copy of the alpha volume and a mask built by hand.

    volume_components   volume, level, connectivity -> VolumeComponents(labels, n_components, voxel_counts, boxes)
    filter_volume       the volume with the unwanted components set to `fill`: min_voxels and / or keep_largest
    TILE                the tile (t0, t1, t2) a workgroup of the local stage owns (`t2n_volume_components_tile`)

A voxel is foreground iff volume > level (strict: NaN is background). connectivity 6 / 18 / 26 = face / + edge / + corner neighbours,
scipy's `generate_binary_structure(3, 1 | 2 | 3)`. Labels are -1 on background and dense on foreground, 0 .. K-1 in the order of each
component's smallest linear voxel index: `scipy.ndimage.label(volume > level, structure)[0] - 1` bit for bit. Everything is integer
(block-based union-find whose roots are each component's smallest voxel, integer counts, scans): two calls give bit-equal arrays.
Device tensor in, device tensors out; numpy array / CPU tensor in, numpy arrays out, through the device. No CPU fallback.

`TensorBase.prune_floaters` is the field-level call built on these."""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _lib

DEFAULT_TILE = (4, 8, 64)      # what csrc/t2n_volume.hip is written with; TILE is read from the library where it is built


def _tile():
    if not os.path.exists(_lib.LIB_PATH):
        return DEFAULT_TILE
    try:
        lib = _lib.load()
    except AttributeError:      # a library from before a new export: `python -m text2nerf_amd.build` imports this package to rebuild it
        return DEFAULT_TILE
    t = (C.c_int * 3)()
    _lib.check(lib.t2n_volume_components_tile(t), "t2n_volume_components_tile")
    return tuple(int(x) for x in t)


TILE = _tile()


class VolumeComponents(NamedTuple):
    labels: object                      # [n0,n1,n2] int32: -1 on background, 0 .. K-1 in the order of each component's smallest index
    n_components: int                   # K
    voxel_counts: object                # [K] int32
    boxes: object                       # [K,6] int32: min0, min1, min2, max0, max1, max2 (inclusive)


def _device():
    if not torch.cuda.is_available():
        raise _lib.T2NError("the volume stages run on the MI355X only (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _is_device(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _volume_on_device(volume, level, connectivity, who):
    """The volume as a contiguous float32 device tensor; ValueError for what the library would refuse, before any launch."""
    t = volume if isinstance(volume, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(volume))
    if t.dim() != 3 or t.dtype != torch.float32:
        raise ValueError(f"{who}: a volume of shape {tuple(t.shape)} and dtype {t.dtype}, need [n0,n1,n2] float32")
    if min(t.shape) < 1 or math.prod(int(s) for s in t.shape) >= 2**31:
        raise ValueError(f"{who}: shape {tuple(t.shape)} (every dimension >= 1, fewer than 2^31 voxels) is refused")
    if connectivity not in (6, 18, 26):
        raise ValueError(f"{who}: connectivity {connectivity!r} (6, 18 or 26)")
    if not math.isfinite(float(level)):
        raise ValueError(f"{who}: level {level!r} is not finite")
    dev = t.device if t.is_cuda else _device()
    return t.detach().to(dev).contiguous(), dev


def _components(lib, vol, level, connectivity, dev):
    n0, n1, n2 = (int(s) for s in vol.shape)
    with torch.cuda.device(dev):
        nbytes = int(lib.t2n_volume_components_workspace_bytes(n0, n1, n2))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        labels = torch.empty((n0, n1, n2), dtype=torch.int32, device=dev)
        k = torch.empty(1, dtype=torch.int64, device=dev)
        stream = _lib.current_stream_ptr(dev)
        _lib.check(lib.t2n_volume_components(_lib.ptr(vol), n0, n1, n2, float(level), int(connectivity), _lib.ptr(labels), _lib.ptr(k),
                                             _lib.ptr(ws), nbytes, stream), "t2n_volume_components")
        K = int(k.cpu().item())                                 # the one 8-byte read
        counts = torch.empty(K, dtype=torch.int32, device=dev)
        boxes = torch.empty((K, 6), dtype=torch.int32, device=dev)
        if K > 0:                                               # nothing is launched for an all-background volume
            _lib.check(lib.t2n_volume_component_stats(_lib.ptr(labels), n0, n1, n2, K, _lib.ptr(counts), _lib.ptr(boxes), stream),
                       "t2n_volume_component_stats")
    return VolumeComponents(labels, K, counts, boxes)


def _host(c):
    return VolumeComponents(c.labels.cpu().numpy(), c.n_components, c.voxel_counts.cpu().numpy(), c.boxes.cpu().numpy())


@torch.no_grad()
def volume_components(volume, level=0.0, connectivity=26):
    """Connected components of the voxels with volume > level: VolumeComponents(labels [n0,n1,n2] int32, n_components K, voxel_counts
    [K] int32, boxes [K,6] int32 = min0, min1, min2, max0, max1, max2 inclusive). volume [n0,n1,n2] float32: a device tensor (device
    tensors come back) or a numpy array / CPU tensor (numpy arrays come back, through the device). Labels are -1 on background and
    dense on foreground, numbered in the order of each component's smallest linear index, so `labels` is one fixed array for a given
    volume; two calls give bit-equal arrays. Host read: the 8 bytes of K. ValueError before any launch: a volume that is not 3-D
    float32, an empty or too large one (2^31 voxels and more), a connectivity other than 6, 18, 26, a level that is not finite.
    T2NError without a GPU."""
    vol, dev = _volume_on_device(volume, level, connectivity, "volume_components")
    c = _components(_lib.load(), vol, level, connectivity, dev)
    return c if _is_device(volume) else _host(c)


def keep_components(voxel_counts, min_voxels=0, keep_largest=None):
    """keep [K] bool on the device of `voxel_counts` (a device int32 tensor): component c stays iff voxel_counts[c] >= min_voxels and,
    with keep_largest = k, c is among the k components with the most voxels; ties go to the lower label (filter_components' rule)."""
    keep = voxel_counts >= int(min_voxels)
    if keep_largest is not None and voxel_counts.shape[0] > 0:
        order = torch.sort(voxel_counts, descending=True, stable=True).indices        # ties: the lower label first
        top = torch.zeros_like(keep)
        top[order[:int(keep_largest)]] = True
        keep &= top
    return keep


@torch.no_grad()
def filter_volume(volume, min_voxels=0, keep_largest=None, level=0.0, connectivity=26, fill=0.0, components=None):
    """(volume_out, components, keep): `volume` with every foreground voxel (volume > level) of an unwanted component set to `fill`;
    the other voxels, background included, keep their bits. Component c stays iff voxel_counts[c] >= min_voxels and, with keep_largest
    = k, c is among the k components with the most voxels (ties go to the lower label); the selection runs on the device. keep is [K]
    bool. `components`: an earlier volume_components result for the same volume, level and connectivity, to skip the labelling. The
    input is not written. Device tensor in, device tensors out; numpy array / CPU tensor in, numpy arrays out. ValueError before any
    launch: volume_components' cases, min_voxels < 0, keep_largest < 1, components that do not belong to the volume."""
    if int(min_voxels) < 0:
        raise ValueError(f"filter_volume: min_voxels {min_voxels} < 0")
    if keep_largest is not None and int(keep_largest) < 1:
        raise ValueError(f"filter_volume: keep_largest {keep_largest} < 1")
    vol, dev = _volume_on_device(volume, level, connectivity, "filter_volume")
    n0, n1, n2 = (int(s) for s in vol.shape)
    lib = _lib.load()
    if components is None:
        comp = _components(lib, vol, level, connectivity, dev)
    else:
        as_i32 = lambda x: (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(
            device=dev, dtype=torch.int32).contiguous()
        comp = VolumeComponents(as_i32(components[0]), int(components[1]), as_i32(components[2]), as_i32(components[3]))
        if (tuple(comp.labels.shape) != (n0, n1, n2) or tuple(comp.voxel_counts.shape) != (comp.n_components,)
                or not 0 <= comp.n_components <= n0 * n1 * n2):
            raise ValueError(f"filter_volume: components of {tuple(comp.labels.shape)} labels and {comp.n_components} counts do not "
                             f"belong to a volume of shape {(n0, n1, n2)}")
    K = comp.n_components
    with torch.cuda.device(dev):
        keep = keep_components(comp.voxel_counts, min_voxels, keep_largest)
        keep8 = keep.to(torch.uint8).contiguous()
        out = torch.empty_like(vol)
        _lib.check(lib.t2n_volume_filter(_lib.ptr(vol), _lib.ptr(comp.labels), n0, n1, n2, _lib.ptr(keep8), K, float(fill), _lib.ptr(out),
                                         _lib.current_stream_ptr(dev)), "t2n_volume_filter")
    if _is_device(volume):
        return out, comp, keep
    return out.cpu().numpy(), _host(comp), keep.cpu().numpy()
