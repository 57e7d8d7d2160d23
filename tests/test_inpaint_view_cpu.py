"""The inpaint-view builder without a GPU: it refuses to run (no CPU fallback), its three entry points are declared in
include/t2n.h (tests/test_host_cpu.py then holds every declared symbol against the built library), and the workspace of the
many-sources warp is bounded by its 8-source chunk."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_build_inpaint_view_has_no_cpu_fallback(monkeypatch):
    import torch
    from text2nerf_amd._lib import T2NError
    from text2nerf_amd.warp import InpaintView, build_inpaint_view
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    poses = np.stack([np.eye(4, dtype=np.float32)] * 2)
    frames = np.zeros((1, 8, 8, 3), np.float32)
    with pytest.raises(T2NError, match="no CPU fallback"):
        build_inpaint_view(None, poses, 1, 8, 8, [8.0, 8.0, 4, 4], known_rgbs=frames, known_depths=frames[..., 0])
    with pytest.raises(T2NError, match="N_iter"):            # argument errors come before the device check
        build_inpaint_view(None, poses, 0, 8, 8, [8.0, 8.0, 4, 4])
    assert InpaintView._fields[:4] == ("myMap", "myMap_filt", "output_image_warp", "output_depth")


def test_entry_points_are_declared_and_bound():
    from text2nerf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "t2n.h")).read()
    declared = set(re.findall(r"\b(t2n_[a-z0-9_]+)\s*\(", hdr))
    for name in ("t2n_warp_sources", "t2n_sparse_bilateral_filtering_views", "t2n_inpaint_pack", "t2n_warp_sources_workspace_bytes"):
        assert name in declared and name in _lib.SIGNATURES, name
    lib = _lib.load()
    # argument validation happens before any HIP call
    assert lib.t2n_warp_sources(None, None, None, 4, 4, 1, None, None, None, None, None, None, None, 0, None) == -1
    assert lib.t2n_inpaint_pack(None, None, None, None, 4, 4, None, None, None, None, None, None, None, None, None) == -1


def test_warp_sources_workspace_is_bounded_by_the_chunk():
    from text2nerf_amd import _lib
    lib = _lib.load()
    for h, w in ((37, 53), (512, 512)):
        b = [int(lib.t2n_warp_sources_workspace_bytes(h, w, v)) for v in range(1, 20)]
        assert all(b[i] < b[i + 1] for i in range(7)), b                 # one more canvas per source up to 8
        assert all(x == b[7] for x in b[7:]), b                          # flat beyond: the chunk's canvases are reused
        canvas = (h + 2) * (w + 2) * 5 * 8
        assert canvas <= b[1] - b[0] < canvas + 256
        assert b[0] >= canvas + 4 * h * w                                # + the running filled / uint8 image state
    assert lib.t2n_warp_sources_workspace_bytes(0, 5, 1) == 0 and lib.t2n_warp_sources_workspace_bytes(5, 5, 0) == 0
