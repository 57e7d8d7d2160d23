"""The appearance list's tile addressing (csrc/t2n_lists.h: list_live, tile_prefix, row_to_entry, slot_to_row) run on the CPU: a host
program (tests/helpers/list_tiles_host.hip, built under AddressSanitizer and UBSan) prints, for every count case of the head's row check
plus three extremes, the tile prefix, the tile total, every row's entry and every live slot's row; compared with an enumeration that
walks the sub-lists in order and pads each to a multiple of 32."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.helpers import head_rows_cases as HC

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
CASES = dict(HC.COUNT_CASES)
CASES["all_zero"] = ((0,) * 8, 128)
CASES["all_at_capacity"] = ((100,) * 8, 100)
CASES["only_list7"] = ((0, 0, 0, 0, 0, 0, 0, 1), 96)


def enumerate_rows(counts, cap):
    """(prefix [9], live counts [8], rows [(live, slot index)], row of each live slot {slot index: row}) by walking the sub-lists."""
    live = [min(c, cap) for c in counts]
    prefix, rows, back = [], [], {}
    for l, n in enumerate(live):
        prefix.append(len(rows) // 32)
        for s in range((n + 31) // 32 * 32):
            if s < n:
                back[l * cap + s] = len(rows)
            rows.append((1 if s < n else 0, l * cap + s))
    prefix.append(len(rows) // 32)
    return prefix, live, rows, back


@pytest.fixture(scope="module")
def host_output(tmp_path_factory):
    if HIPCC is None:
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("list_tiles") / "list_tiles_host")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "text2nerf_amd", "csrc"),
                    os.path.join(ROOT, "tests", "helpers", "list_tiles_host.hip"), "-o", exe], check=True)
    text = "".join(f"{cap} {' '.join(str(c) for c in counts)}\n" for counts, cap in CASES.values())
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    blocks = out.stdout.split("case ")[1:]
    assert len(blocks) == len(CASES)
    return dict(zip(CASES, blocks))


@pytest.mark.parametrize("name", list(CASES))
def test_rows_and_slots_match_the_enumeration(host_output, name):
    counts, cap = CASES[name]
    lines = host_output[name].strip().split("\n")
    assert int(lines[0]) == cap
    prefix, live, rows, back = enumerate_rows(counts, cap)
    assert [int(x) for x in lines[1].split()[1:]] == prefix
    assert [int(x) for x in lines[2].split()[1:]] == live
    assert int(lines[3].split()[1]) == prefix[-1] == len(rows) // 32
    got_rows = np.array([[int(x) for x in l.split()[1:]] for l in lines if l.startswith("row ")], np.int64).reshape(-1, 3)
    got_back = np.array([[int(x) for x in l.split()[1:]] for l in lines if l.startswith("slot ")], np.int64).reshape(-1, 2)
    assert got_rows.shape[0] == len(rows)
    assert np.array_equal(got_rows[:, 0], np.arange(len(rows)))
    assert np.array_equal(got_rows[:, 1:], np.array(rows, np.int64).reshape(-1, 2))
    # every live slot exactly once, and back to the row that maps to it
    assert got_back.shape[0] == sum(live) == int(got_rows[:, 1].sum())
    assert dict(map(tuple, got_back.tolist())) == back
    row_of = dict(map(tuple, got_back.tolist()))
    for r, lv, idx in got_rows.tolist():
        if lv:
            assert row_of[idx] == r
