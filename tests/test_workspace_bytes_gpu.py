"""The backward's and the fused train step's workspace carves, pinned byte for byte: t2n_backward_workspace_bytes and
t2n_train_step_workspace_bytes of a tuned-shape field on a grid of three unequal lengths (a swapped axis in the tile / block geometry
changes the bin counts) against tests/golden/workspace_bytes.json, recorded from the library before the two drivers were taken apart.
Byte counts only: nothing of these sizes is allocated."""
import json
import os

import pytest

from text2nerf_amd import synth
from tests.conftest import TINY
from tests.test_hip_parity import make_field

pytestmark = pytest.mark.gpu

GRID = [20, 24, 28]
SHAPES = [(4, 8, 32), (1500, 64, 4096), (16384, 259, 131072)]      # (n_rays, n_samples, rows)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_bytes.json")


def workspace_bytes():
    from text2nerf_amd import _lib
    lib = _lib.load()
    f = make_field(synth.make_field_params(11, GRID, density_scale=0.9, aabb=TINY["aabb"]), GRID, TINY["aabb"], TINY["near_far"])
    f.sync_params()
    return {f"{R}x{N}x{rows}": {"backward": int(lib.t2n_backward_workspace_bytes(f._handle, rows, R, N)),
                               "train_step": int(lib.t2n_train_step_workspace_bytes(f._handle, R, N, rows))}
            for R, N, rows in SHAPES}


def test_workspace_bytes_match_the_recorded_carves():
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = workspace_bytes()
    assert sorted(got) == sorted(want)
    for shape in got:
        print(shape, got[shape], want[shape])
        assert got[shape]["backward"] > 0 and got[shape]["train_step"] > 0
        assert got[shape] == want[shape], shape
