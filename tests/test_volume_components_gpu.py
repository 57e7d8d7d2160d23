"""Device connected components of a dense volume (csrc/t2n_volume.hip through text2nerf_amd.volume and the C ABI) against the host
reference tests/helpers/volume_cc_ref.py (scipy.ndimage.label - 1, checked by tests/test_volume_components_cpu.py). Everything is
integer or a moved float: labels, K, counts, boxes and filtered volumes are compared for exact equality, and every call runs twice with
bit-equal results. The shapes come from the local stage's tile (volume.TILE): one tile, one voxel more on each axis, pairs that touch
only across a tile face / edge / corner, a tube that crosses tile borders again and again."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.helpers import volume_cc_ref as R
from tests.test_hip_parity import dev
from text2nerf_amd import _lib, volume
from text2nerf_amd import VolumeComponents, filter_volume, volume_components

pytestmark = pytest.mark.gpu

TILE = R.tile()
CASES = R.gpu_cases(TILE)


def host(x):
    return x.cpu().numpy()


def on_device(vol):
    return torch.from_numpy(np.array(vol, order="C", copy=True)).to(dev())        # (a copy: the shared references are read-only)


@pytest.fixture(scope="module")
def reference():
    """name, connectivity -> the reference's (labels, K, counts, boxes): computed once, shared, never written."""
    out = {}
    for name, (vol, level) in CASES.items():
        for c in R.CONNECTIVITIES:
            out[name, c] = R.components(vol, level, c)
            for a in (out[name, c][0], out[name, c][2], out[name, c][3]):
                a.setflags(write=False)
    return out


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_labels_counts_boxes(name, connectivity, reference):
    vol, level = CASES[name]
    d = on_device(vol)
    got = volume_components(d, level=level, connectivity=connectivity)
    again = volume_components(d, level=level, connectivity=connectivity)
    assert isinstance(got, VolumeComponents) and isinstance(got.n_components, int)
    for t in (got.labels, got.voxel_counts, got.boxes):
        assert t.is_cuda and t.dtype == torch.int32
    want = reference[name, connectivity]
    print(f"{name} c{connectivity}: shape {vol.shape} K {got.n_components} (reference {want[1]})")
    assert tuple(got.boxes.shape) == (got.n_components, 6) and tuple(got.voxel_counts.shape) == (got.n_components,)
    assert R.check(vol, level, connectivity, host(got.labels), got.n_components, host(got.voxel_counts), host(got.boxes)) is None
    assert got.n_components == want[1] and np.array_equal(host(got.labels), want[0])
    assert again.n_components == got.n_components
    for a, b in zip((got.labels, got.voxel_counts, got.boxes), (again.labels, again.voxel_counts, again.boxes)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("how", ["face", "edge", "corner"])
def test_pairs_across_tile_borders(how):
    vol = on_device(R.touching_pair(TILE, how)[0])
    got = {c: volume_components(vol, connectivity=c).n_components for c in R.CONNECTIVITIES}
    assert got == R.PAIR_COMPONENTS[how]


def test_checkerboard():
    vol = CASES["checkerboard"][0]
    d = on_device(vol)
    assert volume_components(d, connectivity=6).n_components == int(vol.sum())
    assert volume_components(d, connectivity=18).n_components == 1 and volume_components(d, connectivity=26).n_components == 1


def test_numpy_in_numpy_out(reference):
    vol, level = CASES["13x17x70"]
    got = volume_components(vol, level=level, connectivity=18)
    assert all(isinstance(a, np.ndarray) for a in (got.labels, got.voxel_counts, got.boxes))
    assert R.check(vol, level, 18, got.labels, got.n_components, got.voxel_counts, got.boxes) is None
    out, comp, keep = filter_volume(torch.from_numpy(vol), keep_largest=2, connectivity=18)        # a CPU tensor comes back as numpy too
    assert isinstance(out, np.ndarray) and isinstance(keep, np.ndarray) and keep.dtype == bool and isinstance(comp.labels, np.ndarray)


# ---- the C ABI directly: all background writes nothing past the labels, aliasing, argument errors ------------------------------------
def abi_components(lib, vol, level, conn, guard=64):
    """t2n_volume_components on a device volume with guard words behind labels and K; returns (labels, K, guards intact)."""
    n0, n1, n2 = vol.shape
    n = vol.numel()
    nbytes = int(lib.t2n_volume_components_workspace_bytes(n0, n1, n2))
    assert nbytes >= 4 * n
    ws = torch.empty(nbytes, dtype=torch.uint8, device=vol.device)
    labels = torch.full((n + guard,), -77, dtype=torch.int32, device=vol.device)
    k = torch.full((1 + guard,), -77, dtype=torch.int64, device=vol.device)
    _lib.check(lib.t2n_volume_components(_lib.ptr(vol), n0, n1, n2, float(level), conn, _lib.ptr(labels), _lib.ptr(k), _lib.ptr(ws), nbytes,
                                         _lib.current_stream_ptr(vol.device)), "t2n_volume_components")
    torch.cuda.synchronize()
    intact = bool((labels[n:] == -77).all()) and bool((k[1:] == -77).all())
    return labels[:n].reshape(n0, n1, n2), int(k[0]), intact


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
def test_all_background_writes_labels_and_k_only(connectivity):
    lib = _lib.load()
    vol, level = CASES["all_background"]
    labels, K, intact = abi_components(lib, on_device(vol), level, connectivity)
    assert K == 0 and intact and bool((labels == -1).all())
    # stats and filter with K = 0: nothing to write, NULL counts and keep are accepted, the volume comes back bit for bit
    d = on_device(vol)
    out = torch.full_like(d, 5.0)
    s = _lib.current_stream_ptr(d.device)
    assert lib.t2n_volume_component_stats(_lib.ptr(labels.contiguous()), *vol.shape, 0, None, None, s) == 0
    assert lib.t2n_volume_filter(_lib.ptr(d), _lib.ptr(labels.contiguous()), *vol.shape, None, 0, 9.0, _lib.ptr(out), s) == 0
    assert torch.equal(out, d)


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
def test_guards_stay_intact_on_odd_shapes(connectivity, reference):
    lib = _lib.load()
    for name in ("tile_plus_one", "13x17x70", "1x1xN", "Nx1x1"):
        vol, level = CASES[name]
        labels, K, intact = abi_components(lib, on_device(vol), level, connectivity)
        assert intact and K == reference[name, connectivity][1] and np.array_equal(host(labels), reference[name, connectivity][0]), name


@pytest.mark.parametrize("fill", [0.0, -123.5])
@pytest.mark.parametrize("aliased", [False, True])
def test_filter_abi(fill, aliased, reference):
    lib = _lib.load()
    vol, level = CASES["special_values"]
    labels, K, counts, _ = reference["special_values", 6]
    keep = R.keep_mask(counts, min_voxels=2)
    assert 0 < keep.sum() < K
    want = R.filter_volume(vol, labels, keep, fill)
    d, dl, dk = on_device(vol), on_device(labels), on_device(keep.astype(np.uint8))
    out = d if aliased else torch.full_like(d, 77.0)
    for _ in range(2 if not aliased else 1):
        _lib.check(lib.t2n_volume_filter(_lib.ptr(d), _lib.ptr(dl), *vol.shape, _lib.ptr(dk), K, fill, _lib.ptr(out),
                                         _lib.current_stream_ptr(d.device)), "t2n_volume_filter")
    got = host(out)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))            # NaN, -inf and the level-valued backgrounds bit for bit
    if not aliased:
        assert np.array_equal(host(d).view(np.uint32), vol.view(np.uint32))     # the input is not written


@pytest.mark.parametrize("kw", [dict(min_voxels=3), dict(keep_largest=1), dict(keep_largest=3, min_voxels=2), dict(),
                                dict(keep_largest=2, fill=-1.0)])
def test_filter_volume_python(kw, reference):
    vol, level = CASES["random_p0.1"]
    labels, K, counts, boxes = reference["random_p0.1", 26]
    keep = R.keep_mask(counts, kw.get("min_voxels", 0), kw.get("keep_largest"))
    want = R.filter_volume(vol, labels, keep, kw.get("fill", 0.0))
    d = on_device(vol)
    out, comp, got_keep = filter_volume(d, level=level, **kw)
    out2, _, keep2 = filter_volume(d, level=level, components=comp, **kw)
    assert out.is_cuda and got_keep.dtype == torch.bool and comp.n_components == K
    assert np.array_equal(host(got_keep), keep) and np.array_equal(host(out).view(np.uint32), want.view(np.uint32))
    assert torch.equal(out, out2) and torch.equal(got_keep, keep2)
    assert np.array_equal(host(d).view(np.uint32), vol.view(np.uint32))


def test_keep_ties_go_to_the_lower_label():
    vol = np.zeros((3, 3, 40), np.float32)
    for k in (2, 9, 20, 30):
        vol[1, 1, k:k + 3] = 1.0             # four components of three voxels
    vol[1, 1, 36:38] = 1.0                   # and one of two
    out, comp, keep = filter_volume(on_device(vol), keep_largest=2)
    assert comp.n_components == 5 and host(comp.voxel_counts).tolist() == [3, 3, 3, 3, 2]
    assert host(keep).tolist() == [True, True, False, False, False]
    assert host(out).sum() == 6.0 and host(out)[1, 1, 2:5].all() and host(out)[1, 1, 9:12].all()


def test_argument_errors():
    lib = _lib.load()
    d = on_device(np.ones((2, 3, 4), np.float32))
    n = d.numel()
    nbytes = int(lib.t2n_volume_components_workspace_bytes(2, 3, 4))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d.device)
    labels = torch.full((n,), -5, dtype=torch.int32, device=d.device)
    k = torch.full((1,), -5, dtype=torch.int64, device=d.device)
    s = _lib.current_stream_ptr(d.device)
    P = _lib.ptr
    INVALID = -1        # T2N_ERR_INVALID
    t3 = (C.c_int * 3)()
    assert lib.t2n_volume_components_tile(t3) == 0 and tuple(t3) == volume.TILE and tuple(t3)[2] % 64 == 0
    assert lib.t2n_volume_components_tile(None) != 0
    for shape in ((0, 3, 4), (2, -1, 4), (2, 3, 0), (2048, 1024, 1024), (46341, 46341, 1)):
        assert lib.t2n_volume_components_workspace_bytes(*shape) == 0
    assert lib.t2n_volume_components_workspace_bytes(1, 1, 1) > 0
    good = dict(volume=P(d), n0=2, n1=3, n2=4, level=0.0, conn=26, labels=P(labels), k=P(k), ws=P(ws), nbytes=nbytes)
    bad = [dict(volume=None), dict(labels=None), dict(k=None), dict(ws=None), dict(n0=0), dict(n1=-2), dict(n2=0), dict(conn=8),
           dict(conn=0), dict(conn=27), dict(level=float("nan")), dict(level=float("inf")), dict(level=float("-inf")),
           dict(nbytes=nbytes - 1), dict(nbytes=0), dict(n0=2048, n1=1024, n2=1024)]
    for b in bad:
        a = dict(good, **b)
        rc = lib.t2n_volume_components(a["volume"], a["n0"], a["n1"], a["n2"], a["level"], a["conn"], a["labels"], a["k"], a["ws"],
                                       a["nbytes"], s)
        assert rc == INVALID, b
    for K in (-1, n + 1):
        assert lib.t2n_volume_component_stats(P(labels), 2, 3, 4, K, P(labels), None, s) == INVALID
        assert lib.t2n_volume_filter(P(d), P(labels), 2, 3, 4, P(ws), K, 0.0, P(d), s) == INVALID
    assert lib.t2n_volume_component_stats(None, 2, 3, 4, 1, P(labels), None, s) == INVALID
    assert lib.t2n_volume_component_stats(P(labels), 2, 3, 4, 1, None, None, s) == INVALID
    assert lib.t2n_volume_component_stats(P(labels), 2, 0, 4, 1, P(labels), None, s) == INVALID
    for b in (dict(v=None), dict(l=None), dict(o=None), dict(keep=None), dict(n1=0)):
        a = dict(dict(v=P(d), l=P(labels), keep=P(ws), o=P(d), n1=3), **b)
        assert lib.t2n_volume_filter(a["v"], a["l"], 2, a["n1"], 4, a["keep"], 1, 0.0, a["o"], s) == INVALID, b
    torch.cuda.synchronize()
    assert bool((labels == -5).all()) and int(k[0]) == -5 and bool((d == 1.0).all())      # no refused call launched anything
    # the Python surface: ValueError before any launch
    for badvol in (d[0], d.double(), d.int(), d[:0]):
        with pytest.raises(ValueError):
            volume_components(badvol)
    for conn in (8, 0, "6"):
        with pytest.raises(ValueError):
            volume_components(d, connectivity=conn)
        with pytest.raises(ValueError):
            filter_volume(d, connectivity=conn)
    with pytest.raises(ValueError):
        volume_components(d, level=float("nan"))
    with pytest.raises(ValueError):
        filter_volume(d, min_voxels=-1)
    with pytest.raises(ValueError):
        filter_volume(d, keep_largest=0)
    with pytest.raises(ValueError):
        filter_volume(d, components=volume_components(on_device(np.ones((2, 3, 5), np.float32))))
    # a volume that is not contiguous is labelled as the array it shows
    t = on_device(R.random_volume((9, 8, 70), 0.3, 9)).permute(1, 0, 2)
    got = volume_components(t, connectivity=6)
    assert R.check(host(t), 0.0, 6, host(got.labels), got.n_components, host(got.voxel_counts), host(got.boxes)) is None
