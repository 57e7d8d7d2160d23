"""Host side of the indexed train step (TensorVMSplit.train_step_indexed on a dataset.DeviceTrainSet): the set's bookkeeping on
device="cpu", the id gate, the slot layout and the C-ABI additions. No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch


def _rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 6, generator=g), torch.rand(n, 3, generator=g), torch.rand(n, generator=g)


def test_append_returns_contiguous_ranges_and_rows_survive_growth_bitwise():
    from text2nerf_amd import DeviceTrainSet
    parts = [_rows(n, 10 + k) for k, n in enumerate((5, 7, 30, 1, 100))]
    parts[2][0][3, 2] = float("nan")                       # (bitwise: a NaN payload survives too)
    s = DeviceTrainSet(*parts[0], device="cpu")
    assert len(s) == 5 and s.capacity == 5 and s.moves == 0
    lo_expected, caps = 5, [s.capacity]
    for p in parts[1:]:
        lo, hi = s.append(*p)
        assert (lo, hi) == (lo_expected, lo_expected + p[0].shape[0])
        lo_expected = hi
        caps.append(s.capacity)
    assert len(s) == 143 and s.moves >= 2, (len(s), s.moves, caps)      # at least two growths
    assert all(b % a == 0 and (b // a) & (b // a - 1) == 0 for a, b in zip(caps, caps[1:])), caps     # growth doubles the capacity
    want = [torch.cat([p[k] for p in parts]) for k in range(3)]
    for got, w in zip((s.rays, s.rgbs, s.depths), want):
        assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == w.shape
        assert np.array_equal(got.numpy().view(np.uint32), w.numpy().view(np.uint32))
    assert s.release_retired() == 0


def test_reserve_presizes_and_numpy_rows_are_accepted():
    from text2nerf_amd import DeviceTrainSet
    r, c, d = _rows(8, 3)
    s = DeviceTrainSet(r.numpy(), c.numpy().astype(np.float64), d.numpy()[:, None], device="cpu", reserve=64)
    assert s.capacity == 64 and len(s) == 8 and s.depths.shape == (8,)
    base = s.storage()[0].data_ptr()
    assert s.append(*_rows(56, 4)) == (8, 64)
    assert s.storage()[0].data_ptr() == base and s.moves == 0          # fitted: nothing moved
    assert s.append(*_rows(1, 5)) == (64, 65)
    assert s.capacity == 128 and s.moves == 1
    assert torch.equal(s.rays[:8], r) and torch.equal(s.rgbs[:8], c.double().float())
    from text2nerf_amd._lib import T2NError
    with pytest.raises(T2NError):
        s.append(r, c[:3], d)


def test_rows_equals_index_select():
    from text2nerf_amd import DeviceTrainSet
    r, c, d = _rows(50, 6)
    s = DeviceTrainSet(r, c, d, device="cpu")
    ids = torch.tensor([0, 49, 7, 7, 13, 0], dtype=torch.int64)
    for form in (ids, ids.int()):
        got = s.rows(form)
        assert torch.equal(got[0], r.index_select(0, ids)) and torch.equal(got[1], c.index_select(0, ids)) and torch.equal(got[2], d.index_select(0, ids))


def test_from_support_set_round_trips():
    """build_support_set's 7-tuple starts with the rows, colours and depths of the kept pixels."""
    from text2nerf_amd import DeviceTrainSet
    r, c, d = _rows(33, 8)
    support = (r, c, d, torch.zeros(2, 4, 6), torch.zeros(2, 2, 2, 3), torch.zeros(2, 2, 2), torch.eye(4)[None])
    s = DeviceTrainSet.from_support_set(support, device="cpu")
    assert len(s) == 33 and torch.equal(s.rays, r) and torch.equal(s.rgbs, c) and torch.equal(s.depths, d)
    lo, hi = s.append(*support[:3])
    assert (lo, hi) == (33, 66) and torch.equal(s.rays[lo:hi], r)


def test_id_gate_rejects_out_of_range_negative_and_float_ids():
    from text2nerf_amd._lib import T2NError
    from text2nerf_amd.dataset import check_ids
    ok = check_ids(torch.tensor([[0, 9], [3, 3]]), 10)
    assert ok.shape == (4,) and ok.dtype == torch.int64
    assert check_ids(torch.tensor([0, 9], dtype=torch.int32), 10).dtype == torch.int32
    for bad in (torch.tensor([0, 10]), torch.tensor([-1, 3]), torch.tensor([0.0, 1.0]), torch.tensor([1, 2], dtype=torch.int16),
                torch.tensor([], dtype=torch.int64), [0, 1]):
        with pytest.raises(T2NError):
            check_ids(bad, 10)
    with pytest.raises(T2NError):
        check_ids(torch.tensor([0]), 2 ** 31)
    with pytest.raises(T2NError):
        check_ids(torch.tensor([0]), 0)


def test_train_step_indexed_rejects_bad_ids_before_anything_else():
    """The gate is the method's first act: no field state, optimiser or RNG draw is reached (a bare object stands in for the field)."""
    from text2nerf_amd import DeviceTrainSet, TensorVMSplit
    from text2nerf_amd._lib import T2NError
    s = DeviceTrainSet(*_rows(10, 1), device="cpu")
    torch.manual_seed(5)
    state = torch.get_rng_state()
    for bad in (torch.tensor([0, 10]), torch.tensor([-1]), torch.tensor([0.5])):
        with pytest.raises(T2NError):
            TensorVMSplit.train_step_indexed(object(), s, bad, None)
    assert torch.equal(torch.get_rng_state(), state)


@pytest.mark.parametrize("R", [16384, 4097, 4096, 5])
def test_indexed_slot_layout(R):
    """Host-copied part first (ids | jitter | hyper: 2 R + 32 words at R % 4 == 0), every section on a 16-byte boundary, none overlapping."""
    from text2nerf_amd import _lib
    from text2nerf_amd.trainer import FusedStep
    lay = FusedStep._layout(R, 6, True)
    H = _lib.TRAIN_HYPER_FLOATS
    sizes = dict(ids=R, jitter=R, hyper=H, rays=6 * R, rgb=3 * R, depth=R)
    order = sorted(sizes, key=lambda k: lay[k])
    assert order == ["ids", "jitter", "hyper", "rays", "rgb", "depth"]
    for a, b in zip(order, order[1:] + [None]):
        assert lay[a] % 4 == 0
        assert lay[a] + sizes[a] <= (lay[b] if b else lay["n"])
    assert lay["host"] == lay["rays"] == lay["hyper"] + H
    if R % 4 == 0:
        assert lay["host"] == 2 * R + H
    if R == 16384:
        assert lay["host"] * 4 == 131200
    plain = FusedStep._layout(R, 6, False)      # the plain form is what it was: rays | jitter | rgb | depth | hyper, all of it copied
    assert (plain["rays"], plain["jitter"], plain["rgb"], plain["depth"], plain["hyper"]) == (0, 6 * R, 7 * R, 10 * R, 11 * R)
    assert plain["n"] == plain["host"] == 11 * R + H


def test_c_abi_additions():
    from text2nerf_amd import _lib
    # sizeof(t2n_train_step_args) as read on the parent commit (8325a2f): the struct must not change
    assert C.sizeof(_lib.TrainStepArgs) == 616
    assert _lib.FLAG_GATHER_BATCH == 128
    assert "t2n_field_set_train_source" in _lib.SIGNATURES
    assert _lib.SIGNATURES["t2n_field_set_train_source"][1][1]._type_ is _lib.TrainSource
    assert C.sizeof(_lib.TrainSource) == 48
    lib = _lib.load()
    assert lib.t2n_field_set_train_source(None, None) == -1       # argument validation comes before any HIP call
