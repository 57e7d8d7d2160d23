"""The indexed train step (TensorVMSplit.train_step_indexed on a dataset.DeviceTrainSet: the fused step gathers its batch by row index,
T2N_FLAG_GATHER_BATCH) at the full C3 batch, held to what tests/test_train_step_fullsize.py holds the host-batch step to — same
helpers, same bounds, same float64 oracle.

The training set is the C3 batch's 16 384 rows scattered at seeded random positions among as many decoy rows FILLED WITH NaN (rays,
colours and depths); `ids` are the positions of the C3 rows in batch order, rows 0 and n - 1 among them. One wrong row poisons every
loss and gradient; the gathered sections of the slot's device buffer are also compared bitwise with `source.rows(ids)`."""
import os

import numpy as np
import pytest
import torch

from tests.conftest import TINY
from tests.helpers import adam_readout as A
from tests import test_train_step_fullsize as T
from tests.test_hip_parity import make_field
from tests.test_train_step import assert_same_trajectory, batch
from tests.test_train_step_fullsize import c3, oracle0  # noqa: F401  (module-scoped fixtures: the C3 batch, the oracle at step 1)

pytestmark = pytest.mark.gpu
R_C3, N, SEEDS = T.R_C3, T.N, T.SEEDS


def _dev():
    return torch.device("cuda:0")


def _decoy_set(c3, R=R_C3, decoys=None, seed=77):  # noqa: F811
    """(DeviceTrainSet, ids): the first R rows of the C3 batch at seeded random positions of a set of R + decoys rows, NaN elsewhere.
    ids[k] = position of batch row k; ids[1] = 0 and ids[2] = n - 1. No spare capacity: the first append moves the storage."""
    from text2nerf_amd import DeviceTrainSet
    _, _, rays, rgb_t, dep_t = c3
    decoys = R if decoys is None else decoys
    n = R + decoys
    g = np.random.Generator(np.random.PCG64(seed))
    pos = 1 + g.permutation(n - 2)[:R]
    pos[1], pos[2] = 0, n - 1
    ids = torch.from_numpy(pos.astype(np.int64))
    full = [torch.full((n, 6), float("nan")), torch.full((n, 3), float("nan")), torch.full((n,), float("nan"))]
    for dst, src in zip(full, (rays, rgb_t, dep_t)):
        dst[ids] = src[:R]
    s = DeviceTrainSet(*full, device=_dev())
    assert len(s) == n and s.capacity == n
    return s, ids


def _step(f, opt, src, ids, seed, **kw):
    torch.manual_seed(seed)
    return f.train_step_indexed(src, ids, opt, N_samples=N, white_bg=True, tv=[(getattr(f, name), w) for name, w in T.TV], **kw)


def _presized(f, opt, c3, seed, R=R_C3):  # noqa: F811
    return T._presized_fused_step(f, opt, c3, seed, R)


def _check_gather(fs, src, ids, tag=""):
    """Check 1: the rays | rgb | depth sections of the device buffer of the LAST submitted step == source.rows(ids), bit for bit."""
    R = int(ids.numel())
    lay = fs._layout(R, 6, True)
    buf = fs.inbuf[(fs.issued - 1) % len(fs.inbuf)]
    assert buf.numel() == lay["n"]
    want = src.rows(ids)
    assert all(bool(torch.isfinite(w).all()) for w in want), "the test's own ids point at decoys"
    for name, k, w in (("rays", 6, want[0]), ("rgb", 3, want[1]), ("depth", 1, want[2])):
        got = buf[lay[name]:lay[name] + k * R]
        same = torch.equal(got.view(torch.int32), w.reshape(-1).view(torch.int32))
        print(f"{tag} gather {name}: {'bitwise equal' if same else 'DIFFERS'} ({k * R} words)")
        assert same, (tag, name, int((got.view(torch.int32) != w.reshape(-1).view(torch.int32)).sum()))
    assert torch.equal(buf[:R].view(torch.int32).cpu(), ids.reshape(-1).to(torch.int32).cpu())        # the ids the slot holds


def _step1_checks(tag, f, opt, fs, prev, oracle0):  # noqa: F811
    cur = A.snapshot(f, opt)
    want, ref = oracle0
    T._check_losses(tag, fs.losses.cpu().numpy().astype(np.float64), want)
    g = T._recovered(prev, cur)
    T._check_adam(f, opt, prev, cur, g, 1)
    T._check_master_copies(f, cur)
    assert all(s == 1 for s in cur["step"].values()), cur["step"]
    T._check_grads(tag, g, ref)
    return cur


@pytest.mark.parametrize("R", [R_C3, 4097, 4096])
def test_gather_exactness(c3, R, seed=2024):  # noqa: F811
    """One indexed step at 16 384 rays and either side of the early-binning threshold: the slot's buffer holds exactly the rows asked for
    (ids include row 0 and row n - 1), the host copy covered ids | jitter | hyper only, and the losses are finite (no decoy was read)."""
    assert "T2N_DEN_EARLY" not in os.environ
    f, opt = T._field(c3)
    src, ids = _decoy_set(c3, R)
    assert 0 in ids.tolist() and len(src) - 1 in ids.tolist()
    fs = _presized(f, opt, c3, seed, R)
    _step(f, opt, src, ids, seed, fused=True, graph=False)
    fs.sync()
    assert fs.replays == 0 and fs.issued == 1
    _check_gather(fs, src, ids, f"{R} rays")
    assert bool(torch.isfinite(fs.losses).all()), fs.losses


def test_gather_exactness_with_duplicate_ids(c3, seed=2025):  # noqa: F811
    """A decoy-free set and ids drawn WITH replacement (rows 0 and n - 1 forced in): duplicates gather the same row into every place."""
    from text2nerf_amd import DeviceTrainSet
    f, opt = T._field(c3)
    src = DeviceTrainSet(c3[2], c3[3], c3[4], device=_dev())
    g = np.random.Generator(np.random.PCG64(5))
    pos = g.integers(0, len(src), R_C3)
    pos[0], pos[1], pos[2], pos[3] = 0, len(src) - 1, 0, len(src) - 1
    ids = torch.from_numpy(pos.astype(np.int64))
    assert len(set(pos.tolist())) < R_C3
    _step(f, opt, src, ids, seed, fused=True, graph=False)
    fs = f._fused_step
    fs.sync()                                   # (a withheld first step is replayed from its slot: the buffer is the replay's)
    _check_gather(fs, src, ids, "duplicates")
    assert bool(torch.isfinite(fs.losses).all())


def test_indexed_trajectory_three_steps_vs_oracle(c3, oracle0):  # noqa: F811
    """test_fused_trajectory_three_steps_vs_oracle on row indices: step 1 serial, steps 2 and 3 pipelined; at every step the four losses,
    the 19 gradients from Adam's moments, Adam's update in float64, the master copies and the step counts. Steps 2-3 are held to the
    autograd form like there."""
    assert "T2N_DEN_EARLY" not in os.environ
    f, opt = T._field(c3)
    src, ids = _decoy_set(c3)
    prev = A.snapshot(f, opt)
    for t, seed in enumerate(SEEDS, 1):
        _step(f, opt, src, ids, seed, fused=True, graph=False)
        fs = f._fused_step
        fs.sync()
        losses = fs.losses.cpu().numpy().astype(np.float64)
        cur = A.snapshot(f, opt)
        rec = A.train_record(f)
        want, ref = oracle0 if t == 1 else T._oracle(c3, {k: v.astype(np.float32) for k, v in prev["p"].items()}, seed)
        print(f"step {t}: replays {fs.replays}, pipelined launches {fs.pipelined_launches}, row needs {fs.needs}, capacity {fs.rows_cap}")
        T._check_losses(f"indexed step {t}", losses, want)
        g = T._recovered(prev, cur)
        T._check_adam(f, opt, prev, cur, g, t)
        T._check_master_copies(f, cur)
        assert all(s == t for s in cur["step"].values()), cur["step"]
        assert rec[1] == t and rec[2] == fs.replays, rec[:3]
        if t == 1:
            T._check_grads(f"indexed step {t}", g, ref)
        else:
            auto = T._autograd_form(c3, {k: v.astype(np.float32) for k, v in prev["p"].items()}, seed)
            try:
                T._check_grads(f"indexed step {t}", g, ref)
            except AssertionError as e:
                print(f"   (indexed step vs oracle, not asserted: {str(e).splitlines()[0][:160]})")
            T._check_grads(f"indexed step {t} vs autograd form", g, auto)
            _check_gather(fs, src, ids, f"step {t}")
        prev = cur
    assert fs.pipelined_launches >= 2, fs.pipelined_launches


def test_withheld_indexed_step_replayed_from_its_slot(c3, oracle0):  # noqa: F811
    """cap_once below the need: no update; the replay runs from the slot's buffer (ids and gathered rows as they were) and is step 1."""
    from text2nerf_amd.trainer import FusedStep
    f, opt = T._field(c3)
    src, ids = _decoy_set(c3)
    f.sync_params()
    fs = f.__dict__["_fused_step"] = FusedStep(f, opt)
    fs.cap_once = 256
    prev = A.snapshot(f, opt)
    _step(f, opt, src, ids, SEEDS[0], fused=True, graph=False)
    torch.cuda.synchronize()
    rec = A.train_record(f)
    assert (rec[1], rec[2]) == (0, 1), rec[:3]
    mid = A.snapshot(f, opt)
    for key in ("p", "m", "v"):
        for k in prev[key]:
            assert np.array_equal(mid[key][k], prev[key][k]), (key, k)
    fs.sync()
    assert fs.replays == 1
    rec = A.train_record(f)
    assert (rec[1], rec[2]) == (1, 1), rec[:3]
    _step1_checks("replayed indexed step", f, opt, fs, prev, oracle0)
    _check_gather(fs, src, ids, "replay")


def test_append_between_pipelined_steps(c3):  # noqa: F811
    """Two steps (the second pipelined), then an append that moves the set's storage, then a step whose ids alternate between old rows
    and appended rows: its buffer holds the right rows and its losses are the oracle's for that batch at the parameters it started from."""
    f, opt = T._field(c3)
    src, ids = _decoy_set(c3)
    fs = _presized(f, opt, c3, SEEDS[0])
    for seed in SEEDS[:2]:
        _step(f, opt, src, ids, seed, fused=True, graph=False)
    assert fs.pipelined_launches == 1
    # appended block: the C3 rows once more, in reverse order, behind a block of NaN decoys
    _, _, rays, rgb_t, dep_t = c3
    nan = float("nan")
    ptr0, n0, moves0 = src.storage()[0].data_ptr(), len(src), src.moves
    lo, hi = src.append(torch.cat([torch.full((100, 6), nan), rays.flip(0)]), torch.cat([torch.full((100, 3), nan), rgb_t.flip(0)]),
                        torch.cat([torch.full((100,), nan), dep_t.flip(0)]))
    assert (lo, hi) == (n0, n0 + 100 + R_C3) and src.moves == moves0 + 1 and src.storage()[0].data_ptr() != ptr0
    k = torch.arange(R_C3)
    new_ids = lo + 100 + (R_C3 - 1 - k)                      # batch row k in the appended block
    mixed = torch.where(k % 2 == 0, ids, new_ids)
    assert int((mixed < n0).sum()) == R_C3 // 2
    fs.sync()
    prev = A.snapshot(f, opt)
    _step(f, opt, src, mixed, SEEDS[2], fused=True, graph=False)
    fs.sync()
    _check_gather(fs, src, mixed, "after append")
    want, _ = T._oracle(c3, {k: v.astype(np.float32) for k, v in prev["p"].items()}, SEEDS[2])
    T._check_losses("indexed step after append", fs.losses.cpu().numpy().astype(np.float64), want)
    # and pipelined again from the next step on, on the moved storage
    _step(f, opt, src, mixed, 4242, fused=True, graph=False)
    fs.sync()
    assert fs.pipelined_launches >= 2
    _check_gather(fs, src, mixed, "pipelined after append")


def test_all_reduce_form(c3, oracle0):  # noqa: F811
    """Phase 1 | an averaging all-reduce on a world of 1 (identity) | phase 2: step 1."""
    f, opt = T._field(c3)
    src, ids = _decoy_set(c3)
    fs = _presized(f, opt, c3, SEEDS[0])
    calls = []
    prev = A.snapshot(f, opt)
    _step(f, opt, src, ids, SEEDS[0], fused=True, all_reduce=lambda: calls.append(float(fs.head_grads[-1])))
    fs.sync()
    assert calls == [0.0] and fs.replays == 0
    _step1_checks("indexed two-phase step", f, opt, fs, prev, oracle0)
    _check_gather(fs, src, ids, "two-phase")


def test_graph_form_recaptures_after_append(c3, oracle0):  # noqa: F811
    """graph=True: step 1 (eager, as every first step), step 2 captured once per input buffer and replayed; an append that moves the
    storage changes the graph key — the next step re-captures and gathers from the new storage."""
    f, opt = T._field(c3)
    src, ids = _decoy_set(c3)
    fs = _presized(f, opt, c3, SEEDS[0])
    prev = A.snapshot(f, opt)
    _step(f, opt, src, ids, SEEDS[0], fused=True, graph=True)
    fs.sync()
    assert fs.replays == 0
    _step1_checks("indexed graph step 1", f, opt, fs, prev, oracle0)
    _step(f, opt, src, ids, SEEDS[1], fused=True, graph=True)
    fs.sync()
    assert (fs.graph_launches, fs.graph_captures) == (1, 4), (fs.graph_launches, fs.graph_captures)
    _check_gather(fs, src, ids, "graph replay")
    captures = fs.graph_captures
    _, _, rays, rgb_t, dep_t = c3
    lo, hi = src.append(rays[:64], rgb_t[:64], dep_t[:64])
    assert src.moves == 1
    mixed = ids.clone()
    mixed[:64] = torch.arange(lo, hi)                      # batch rows 0..63 from the appended block: the same batch
    _step(f, opt, src, mixed, SEEDS[2], fused=True, graph=True)
    fs.sync()
    assert fs.graph_captures == captures + 4 and fs.graph_launches == 2, (fs.graph_captures, captures, fs.graph_launches)
    _check_gather(fs, src, mixed, "graph after append")
    assert bool(torch.isfinite(fs.losses).all())


def test_fallback_equals_train_step_on_gathered_rows(tiny_params):
    """Where the fused step does not apply (strict-fp32 head), train_step_indexed IS train_step on source.rows(ids): same trajectory
    from equal seeds and parameters, within what test_train_step_equals_the_autograd_step holds two step forms to (losses rtol 1e-5,
    assert_same_trajectory)."""
    from text2nerf_amd import DeviceTrainSet
    from text2nerf_amd.optim import TVAdam
    rays, rgb_t, dep_t = batch()
    n = rays.shape[0]
    perm = torch.from_numpy(np.random.Generator(np.random.PCG64(9)).permutation(n))
    src = DeviceTrainSet(rays, rgb_t, dep_t, device=_dev())
    fa = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    fb = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    fa.mlp_exact_fp32 = fb.mlp_exact_fp32 = True
    oa = TVAdam(fa.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=fa)
    ob = TVAdam(fb.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=fb)
    steps = 5
    for it in range(steps):
        ids = perm.roll(37 * it)[:256]
        tv = lambda f: [(f.density_plane, 0.1), (f.app_plane, 0.01)]     # noqa: E731
        torch.manual_seed(50 + it)
        la = fa.train_step(*src.rows(ids), oa, N_samples=-1, white_bg=True, tv=tv(fa)).clone()
        torch.manual_seed(50 + it)
        lb = fb.train_step_indexed(src, ids, ob, N_samples=-1, white_bg=True, tv=tv(fb)).clone()
        assert torch.allclose(la, lb, rtol=1e-5, atol=1e-9), (it, la, lb)
    assert fb.__dict__.get("_fused_step") is None
    assert_same_trajectory(fa, fb, steps=steps)


def test_out_of_range_ids_are_rejected_before_anything_is_queued(c3):  # noqa: F811
    from text2nerf_amd._lib import T2NError
    f, opt = T._field(c3)
    src, ids = _decoy_set(c3, 4096)
    fs = _presized(f, opt, c3, SEEDS[0], 4096)
    _step(f, opt, src, ids, SEEDS[0], fused=True, graph=False)
    fs.sync()
    before, rec0 = A.snapshot(f, opt), A.train_record(f)
    torch.manual_seed(11)
    rng = torch.get_rng_state()
    for bad in (ids.clone().index_fill_(0, torch.tensor([5]), len(src)), ids.clone().index_fill_(0, torch.tensor([9]), -1), ids.float()):
        with pytest.raises(T2NError):
            f.train_step_indexed(src, bad, opt, N_samples=N, white_bg=False, fused=True, graph=False)
    torch.cuda.synchronize()
    after, rec1 = A.snapshot(f, opt), A.train_record(f)
    assert rec1[0] == rec0[0] == 1 and rec1[:3] == rec0[:3] and fs.issued == 1
    assert torch.equal(torch.get_rng_state(), rng)
    for key in ("p", "m", "v"):
        for k in before[key]:
            assert np.array_equal(after[key][k], before[key][k]), (key, k)
    assert after["step"] == before["step"]
