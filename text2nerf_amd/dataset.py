"""The training set on the device: what the driver keeps as ``allrays`` / ``allrgbs`` / ``alldepth`` on the host and rebuilds with
``torch.cat`` at every new view (text2nerf_main.py:509-516, 530-532), kept where ``warp.build_support_set`` leaves its rows.

``TensorVMSplit.train_step_indexed(source, ids, optimizer)`` trains on rows of it: the host sends the row indices, the step gathers
``rays[ids]``, ``rgbs[ids]``, ``depths[ids]`` itself (T2N_FLAG_GATHER_BATCH, include/t2n.h).
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import T2NError


def _rows(x, width, dev):
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not torch.is_tensor(t):
        raise T2NError("DeviceTrainSet: rows must be torch tensors or numpy arrays")
    t = t.detach()
    t = t.reshape(-1) if width is None else t.reshape(-1, width)
    return t.to(device=dev, dtype=torch.float32)


def check_ids(ids, n_rows):
    """The host-side gate of ``train_step_indexed``: an integer tensor (int64 as SimpleSampler returns it, or int32) whose entries are
    rows of a set of ``n_rows`` (< 2**31: the kernel reads 32-bit indices). Raises T2NError; returns the ids flat. Host ids are checked
    in full; device ids by dtype only (reading them back would wait for the device: the kernel clamps what it is given)."""
    if not torch.is_tensor(ids) or ids.dtype not in (torch.int64, torch.int32):
        raise T2NError(f"train_step_indexed: ids must be an int64 or int32 tensor, not {getattr(ids, 'dtype', type(ids))}")
    n_rows = int(n_rows)
    if n_rows < 1 or n_rows >= 2 ** 31:
        raise T2NError(f"train_step_indexed: a training set of {n_rows} rows (1 .. 2**31 - 1)")
    ids = ids.reshape(-1)
    if ids.numel() < 1:
        raise T2NError("train_step_indexed: no ids")
    if ids.device.type == "cpu":
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= n_rows:
            raise T2NError(f"train_step_indexed: ids span [{lo}, {hi}], the set has rows [0, {n_rows})")
    return ids


class DeviceTrainSet:
    """Rays [n, 6], colours [n, 3] and depths [n] as contiguous float32 tensors on one device, growing by ``append``.

    ``append`` writes behind the live rows; when they do not fit, capacity doubles (``reserve`` pre-sizes it) and the live rows are
    copied to new storage — bitwise, once per doubling, instead of the driver's ``torch.cat`` of everything at every view. Row numbers
    never change, so a second sampler over the newest view is ``SimpleSampler(hi - lo, batch).nextids() + lo`` on the same set.

    Lifetime of replaced storage: a step submitted earlier may still be gathering from it, on a library-owned stream torch's allocator
    does not know. The choice made here: ``append`` records an event on the current stream — the stream the steps are submitted on; every
    gather submitted before is joined into it by then — and keeps a reference to the replaced tensors until that event has passed
    (checked at the next ``append`` / ``release_retired``). Independently, ``FusedStep`` holds the tensors a slot gathered from until the
    slot is reused. Rows are written on the current stream: change them through ``append`` only.
    """

    def __init__(self, rays, rgbs, depths, device=None, reserve=0):
        if device is None:
            device = rays.device if torch.is_tensor(rays) else "cuda"
        self.device = torch.device(device)
        self._n = 0
        self._cap = 0
        self._rays = self._rgbs = self._depths = None
        self._retired = []
        self.moves = 0            # reallocations so far
        r, c, d = self._check(rays, rgbs, depths)
        self._alloc(max(int(reserve), r.shape[0], 1))
        self._write(r, c, d)

    @classmethod
    def from_support_set(cls, support, device=None, reserve=0):
        """From ``warp.build_support_set``'s 7-tuple (rows, colours, depths first)."""
        return cls(support[0], support[1], support[2], device=device, reserve=reserve)

    # ---- storage ----------------------------------------------------------------------------------------------------------------------
    def _check(self, rays, rgbs, depths):
        r, c, d = _rows(rays, 6, self.device), _rows(rgbs, 3, self.device), _rows(depths, None, self.device)
        if not (r.shape[0] == c.shape[0] == d.shape[0]):
            raise T2NError(f"DeviceTrainSet: {r.shape[0]} rays, {c.shape[0]} colours, {d.shape[0]} depths")
        return r, c, d

    def _alloc(self, cap):
        dev = self.device
        new = (torch.empty(cap, 6, dtype=torch.float32, device=dev), torch.empty(cap, 3, dtype=torch.float32, device=dev),
               torch.empty(cap, dtype=torch.float32, device=dev))
        if self._n:
            for dst, src in zip(new, (self._rays, self._rgbs, self._depths)):
                dst[:self._n].copy_(src[:self._n])
        if self._rays is not None:
            ev = None
            if dev.type == "cuda":
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(dev))
            self._retired.append((ev, (self._rays, self._rgbs, self._depths)))
            self.moves += 1
        self._rays, self._rgbs, self._depths = new
        self._cap = cap

    def _write(self, r, c, d):
        lo, hi = self._n, self._n + r.shape[0]
        self._rays[lo:hi].copy_(r, non_blocking=True)
        self._rgbs[lo:hi].copy_(c, non_blocking=True)
        self._depths[lo:hi].copy_(d, non_blocking=True)
        self._n = hi
        return lo, hi

    def release_retired(self):
        """Drop the replaced storage whose event has passed; returns how many are still held."""
        self._retired = [(ev, t) for ev, t in self._retired if ev is not None and not ev.query()]
        return len(self._retired)

    def append(self, rays, rgbs, depths):
        """Add rows; returns the row range (lo, hi) they occupy."""
        r, c, d = self._check(rays, rgbs, depths)
        self.release_retired()
        need = self._n + r.shape[0]
        if need >= 2 ** 31:
            raise T2NError("DeviceTrainSet: 2**31 rows or more (the step reads 32-bit row indices)")
        if need > self._cap:
            cap = max(self._cap, 1)
            while cap < need:
                cap *= 2
            self._alloc(cap)
        return self._write(r, c, d)

    # ---- views ------------------------------------------------------------------------------------------------------------------------
    def __len__(self):
        return self._n

    @property
    def capacity(self):
        return self._cap

    @property
    def rays(self):
        return self._rays[:self._n]

    @property
    def rgbs(self):
        return self._rgbs[:self._n]

    @property
    def depths(self):
        return self._depths[:self._n]

    def storage(self):
        """The three backing tensors (all `capacity` rows): what a submitted step reads and must outlive."""
        return self._rays, self._rgbs, self._depths

    def rows(self, ids):
        """(rays[ids], rgbs[ids], depths[ids]) by ``index_select``: what the fused step's gather leaves in its batch buffer."""
        ids = ids.reshape(-1).to(device=self.device, dtype=torch.int64)
        return self.rays.index_select(0, ids), self.rgbs.index_select(0, ids), self.depths.index_select(0, ids)
