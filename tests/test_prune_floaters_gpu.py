"""TensorBase.prune_floaters on the MI355X: a 48^3 TensorVMSplit whose density is two rank-1 bumps, one large blob and one small detached
blob (the floater), every other density component zero; and a second, general-shape field (20 density components a plane) with the
same two bumps. The mask volume the call attaches is compared bit for bit with the host reference (tests/helpers/volume_cc_ref.py:
scipy's labels of the volume updateAlphaMask attaches, the keep rule, the filter); frames are compared for equality of their bits.

Which frames can be compared bit for bit. On an MI355X, 40 identical renders of one unchanged field of this scene gave (rgb frames
that differ from the last one, depth frames that differ, most colour values that differ in a frame):
    no mask, tile marcher, defaults                     (0, 0, 0) in one process, but two such frames differed in another (1 value, 6e-8)
    no mask, tile marcher, feature_staging = False      (37, 0, 1)
    no mask, tile marcher, appearance_volume = False    (2, 0, 1)
    no mask, per-ray marcher (frame_width = 0)          (0, 0, 0)
    a mask attached, tile marcher, all seven settings   (0, 0, 0)
So an unmasked tile-marcher frame of the renderer as it stands is reproducible in its depth and to one colour value of 6e-8 in its
colour, whatever this call does, while masked frames and per-ray frames are reproducible in every bit. The asserts follow that:
  * pruned against hand-masked, and pruned against pruned again: tile-marcher frames with the caches live (asserted through
    appearance_volume_counts()), every bit;
  * "alphaMask = None restores the first frame bit for bit": the field's first frame by the per-ray marcher, every bit; for the
    tile-marcher frames before and after, the depth in every bit and the colour within 1e-4, the suite's bound between the two forms
    of the feature stage (the first frame runs the direct form, later frames read the cached feature volume).
"""
import numpy as np
import pytest
import torch

from tests.helpers import volume_cc_ref as R
from tests.test_hip_parity import dev
from tests.test_march_summed_table import pinhole_rays
from text2nerf_amd import AlphaGridMask, PruneReport, TensorVMSplit, mesh_components, synth
from text2nerf_amd._lib import T2NError

pytestmark = pytest.mark.gpu

AABB = [[-3.0, -3.0, 2.5], [3.0, 3.0, 8.5]]       # above the eval z gate (2.0)
NEAR_FAR = [0.3, 9.0]
GRID = [48, 48, 48]
N = 96
H = W = 24
BIG = ((-0.8, 0.4, 6.2), 0.8)                     # centre, Gaussian width: inside alphaMask_thres out to ~1.7 widths
FLOATER = ((1.9, 0.4, 4.2), 0.2)
CAMERA = (0.4, 0.4, -1.0)
AMP = 40.0
TUNED = dict(density_n_comp=[16] * 3, appearance_n_comp=[48] * 3)
GENERAL = dict(density_n_comp=[20] * 3, appearance_n_comp=[48] * 3)       # more than 16 density components: the general-shape path


def two_blob_params(kind, seed=5):
    """Random appearance and head; density = AMP * (bump_big + bump_floater) as components 0 and 1 of the xy-plane / z-line pair, every
    other density factor zero. density_shift = -10: the feature is 30 above the shift at the centres and -10 far away."""
    kw = TUNED if kind == "tuned" else GENERAL
    sd = synth.make_field_params(seed, GRID, density_n_comp=kw["density_n_comp"], app_n_comp=kw["appearance_n_comp"], aabb=AABB)
    for k in sd:
        if k.startswith("density_"):
            sd[k][...] = 0.0
    axes = [np.linspace(AABB[0][a], AABB[1][a], GRID[a]) for a in range(3)]
    for c, (centre, width) in enumerate((BIG, FLOATER)):
        bump = [np.exp(-((axes[a] - centre[a]) / width) ** 2) for a in range(3)]
        sd["density_plane.0"][0, c] = np.outer(bump[1], bump[0]).astype(np.float32)          # [gy, gx]
        sd["density_line.0"][0, c, :, 0] = (AMP * bump[2]).astype(np.float32)                # [gz]
    return sd


def new_field(kind, params):
    kw = TUNED if kind == "tuned" else GENERAL
    f = TensorVMSplit(torch.tensor(AABB, dtype=torch.float32), list(GRID), dev(), app_dim=27, near_far=NEAR_FAR,
                      shadingMode="MLP_Fea_noview", alphaMask_thres=1e-3, density_shift=-10, distance_scale=25, pos_pe=0, view_pe=0,
                      fea_pe=6, featureC=128, step_ratio=1.0, fea2denseAct="softplus", **kw)
    f.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    assert f._is_general() == (kind == "general")
    return f


def frame_rays():
    return torch.from_numpy(pinhole_rays(H, W, 0.9 * W, synth.look_pose(0.0, 0.0, CAMERA))).to(dev())


def floater_rays():
    """Rays from the camera through points within a quarter of a width of the floater's centre: they pass the big blob by > 1.5."""
    o = np.asarray(CAMERA, np.float64)
    rng = np.random.default_rng(2)
    targets = np.asarray(FLOATER[0]) + rng.uniform(-0.25, 0.25, (32, 3)) * FLOATER[1]
    d = targets - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = ((np.asarray(BIG[0]) - o) * d).sum(1, keepdims=True)
    assert np.linalg.norm(o + t * d - np.asarray(BIG[0]), axis=1).min() > BIG[1] * 1.7 + 0.5
    return torch.from_numpy(np.concatenate([np.broadcast_to(o, d.shape), d], 1).astype(np.float32)).to(dev())


def frame(f, rays):
    f.materialize_weights = False
    f.frame_width = W
    with torch.no_grad():
        rgb, depth, _, _ = f(rays, N_samples=N)
    return rgb.clone(), depth.clone()


def per_ray_frame(f, rays):
    f.materialize_weights = False
    with torch.no_grad():
        rgb, depth, _, _ = f(rays, N_samples=N, frame_width=0)
    return rgb.clone(), depth.clone()


def close_frames(a, b):
    """The depth in every bit, the colour within the suite's bound between the forms of the feature stage."""
    return torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and float((a[0] - b[0]).abs().max()) <= 1e-4


def acc_rgb(f, rays):
    f.materialize_weights = True
    with torch.no_grad():
        rgb, _, _, w = f(rays, N_samples=N, frame_width=0)
    f.materialize_weights = False
    return w.sum(-1), rgb


def live_frame(f, rays, least=1):
    """Frames until one reads the cached feature volume; returns (that frame, frames rendered)."""
    for n in range(1, 80):
        c0 = f.appearance_volume_counts()
        out = frame(f, rays)
        c1 = f.appearance_volume_counts()
        if c1["volume"] == c0["volume"] + 1 and n >= least:
            assert c1["bytes"] > 0
            return out, n
    raise AssertionError(f"no frame read the cached feature volume: {f.appearance_volume_counts()}")


def same(a, b):
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def mask_volume_of(kind, params):
    """The volume updateAlphaMask(GRID) attaches to a field of these parameters, on the host."""
    g = new_field(kind, params)
    g.updateAlphaMask(tuple(GRID))
    return g.alphaMask.alpha_volume.reshape(GRID[2], GRID[1], GRID[0]).cpu().numpy()


def reference_volume(vol, **kw):
    labels, K, counts, boxes = R.components(vol, 0.0, kw.pop("connectivity", 26))
    keep = R.keep_mask(counts, **kw)
    return R.filter_volume(vol, labels, keep, 0.0), K, counts, keep


@pytest.fixture(scope="module")
def tuned():
    params = two_blob_params("tuned")
    return params, mask_volume_of("tuned", params)


def test_tuned_field(tuned, tmp_path):
    params, vol = tuned
    ref, K, counts, keep = reference_volume(vol, keep_largest=1)
    assert K == 2 and sorted(keep.tolist()) == [False, True] and counts.min() >= 27 and counts.max() > 20 * counts.min()
    f = new_field("tuned", params)
    rays, fl = frame_rays(), floater_rays()

    # the unpruned field: its first frame by the per-ray marcher and by the tile marcher, then frames until the caches are live (> 33)
    first_per_ray = per_ray_frame(f, rays)
    first = frame(f, rays)
    live, n = live_frame(f, rays, least=33)
    assert n + 1 > 33 and f.appearance_volume_counts()["volume"] >= 1 and f.density_cache_counts()["cached"] >= 1
    assert close_frames(first, live)                                                                # the two forms: rounding only
    acc0, _ = acc_rgb(f, fl)
    print(f"tuned: {n + 1} frames, floater rays acc before {float(acc0.min()):.4f} .. {float(acc0.max()):.4f}, voxels {counts.tolist()}")
    assert float(acc0.min()) > 0.5
    m0 = f.export_mesh(None, colors=False)
    assert mesh_components(m0.faces, m0.verts.shape[0]).n_components == 2

    # dry run and both error paths: no mask before, none after
    dry = f.prune_floaters(keep_largest=1, dry_run=True)
    assert isinstance(dry, PruneReport) and dry.n_components == 2 and f.alphaMask is None
    with pytest.raises(T2NError):
        f.prune_floaters(min_voxels=int(counts.max()) + 1)
    thres, f.alphaMask_thres = f.alphaMask_thres, 2.0
    with pytest.raises(T2NError):
        f.prune_floaters(keep_largest=1)
    f.alphaMask_thres = thres
    assert f.alphaMask is None
    for bad in (dict(connectivity=8), dict(min_voxels=-1), dict(keep_largest=0)):
        with pytest.raises(ValueError):
            f.prune_floaters(**bad)

    # the call
    rep = f.prune_floaters(keep_largest=1)
    assert rep.n_components == 2 and rep.keep.cpu().numpy().tolist() == keep.tolist()
    assert rep.voxel_counts.cpu().numpy().tolist() == counts.tolist() and rep.removed_voxels == int(counts.min())
    assert rep.keep.dtype == torch.bool and rep.keep.is_cuda and rep.components.n_components == 2
    assert torch.equal(rep.keep, dry.keep) and torch.equal(rep.components.labels, dry.components.labels)
    got = f.alphaMask.alpha_volume.reshape(GRID[2], GRID[1], GRID[0]).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert torch.equal(f.alphaMask.aabb.cpu(), torch.tensor(AABB)) and f.alphaMask.gridSize.tolist() == GRID
    assert torch.equal(f.aabb.cpu(), torch.tensor(AABB))                                            # no shrinking

    # a frame of the pruned field (caches live: it reads the feature volume) = the frame of a fresh field with the reference volume
    # attached by hand, once that field's frames read its feature volume too
    c0 = f.appearance_volume_counts()
    pruned = frame(f, rays)
    c1 = f.appearance_volume_counts()
    assert c1["volume"] == c0["volume"] + 1 and c1["builds"] == c0["builds"]
    h = new_field("tuned", params)
    h.alphaMask = AlphaGridMask(dev(), torch.tensor(AABB), torch.from_numpy(ref).to(dev()))
    fresh_first = frame(h, rays)
    fresh, _ = live_frame(h, rays)
    assert same(pruned, fresh)
    assert close_frames(pruned, fresh_first)
    assert not torch.equal(pruned[0], live[0])                                                     # the floater was in the frame

    # rays that cross only the floater
    acc1, rgb1 = acc_rgb(f, fl)
    assert float(acc1.abs().max()) == 0.0 and bool((rgb1 == 1.0).all())

    # a second call removes nothing; dry run and error paths leave the mask the same object
    mask = f.alphaMask
    again = f.prune_floaters(keep_largest=1, dry_run=True)
    assert again.n_components == 1 and again.removed_voxels == 0 and f.alphaMask is mask
    assert again.voxel_counts.cpu().numpy().tolist() == [int(counts.max())]
    with pytest.raises(T2NError):
        f.prune_floaters(min_voxels=int(counts.max()) + 1)
    f.alphaMask_thres = 2.0
    with pytest.raises(T2NError):
        f.prune_floaters()
    f.alphaMask_thres = thres
    assert f.alphaMask is mask
    again = f.prune_floaters(keep_largest=1)
    assert again.n_components == 1 and again.removed_voxels == 0 and f.alphaMask is not mask
    assert np.array_equal(f.alphaMask.alpha_volume.reshape(GRID[2], GRID[1], GRID[0]).cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert same(frame(f, rays), pruned)

    # the mesh afterwards
    m1 = f.export_mesh(str(tmp_path / "pruned.ply"), colors=False)
    assert mesh_components(m1.faces, m1.verts.shape[0]).n_components == 1 and 0 < m1.faces.shape[0] < m0.faces.shape[0]

    # undo: the first frame comes back bit for bit (per-ray marcher); the tile-marcher frames, whose colour the renderer reproduces
    # to one value of 6e-8 only (docstring), in their depth bits and within the bound between the forms
    f.alphaMask = None
    assert same(per_ray_frame(f, rays), first_per_ray)
    c0 = f.appearance_volume_counts()
    back = frame(f, rays)
    c1 = f.appearance_volume_counts()
    assert c1["volume"] == c0["volume"] + 1 and close_frames(back, live) and close_frames(back, first)
    print(f"tuned: restored tile frame against the unpruned one: {int((back[0] != live[0]).sum())} colour values differ, "
          f"max {float((back[0] - live[0]).abs().max()):.2e}")
    acc2, _ = acc_rgb(f, fl)
    assert torch.equal(acc2, acc0)


def test_min_voxels_and_connectivity(tuned):
    params, vol = tuned
    f = new_field("tuned", params)
    for kw in (dict(min_voxels=0), dict(min_voxels=28, connectivity=6), dict(keep_largest=2, connectivity=18)):
        ref, K, counts, keep = reference_volume(vol, **kw)
        rep = f.prune_floaters(dry_run=True, **kw)
        assert rep.n_components == K and rep.keep.cpu().numpy().tolist() == keep.tolist()
        assert rep.removed_voxels == int(counts[~keep].sum()) and f.alphaMask is None
    # a coarser grid than the field's own
    g = (30, 26, 22)
    twin = new_field("tuned", params)
    twin.updateAlphaMask(g)
    coarse = twin.alphaMask.alpha_volume.reshape(g[2], g[1], g[0]).cpu().numpy()
    ref, K, counts, keep = reference_volume(coarse, keep_largest=1)
    rep = f.prune_floaters(gridSize=g, keep_largest=1)
    assert rep.n_components == K == 2 and f.alphaMask.gridSize.tolist() == list(g)
    assert np.array_equal(f.alphaMask.alpha_volume.reshape(g[2], g[1], g[0]).cpu().numpy().view(np.uint32), ref.view(np.uint32))


def test_general_shape_field():
    params = two_blob_params("general")
    vol = mask_volume_of("general", params)
    ref, K, counts, keep = reference_volume(vol, keep_largest=1)
    assert K == 2
    f = new_field("general", params)
    rays, fl = frame_rays(), floater_rays()
    first = frame(f, rays)
    acc0, _ = acc_rgb(f, fl)
    assert float(acc0.min()) > 0.5
    assert f.prune_floaters(keep_largest=1, dry_run=True).n_components == 2 and f.alphaMask is None
    with pytest.raises(T2NError):
        f.prune_floaters(min_voxels=int(counts.max()) + 1)
    assert f.alphaMask is None
    rep = f.prune_floaters(keep_largest=1)
    assert rep.n_components == 2 and rep.removed_voxels == int(counts.min()) and rep.keep.cpu().numpy().tolist() == keep.tolist()
    assert np.array_equal(f.alphaMask.alpha_volume.reshape(GRID[2], GRID[1], GRID[0]).cpu().numpy().view(np.uint32), ref.view(np.uint32))
    pruned = frame(f, rays)
    h = new_field("general", params)
    h.alphaMask = AlphaGridMask(dev(), torch.tensor(AABB), torch.from_numpy(ref).to(dev()))
    assert same(pruned, frame(h, rays)) and not torch.equal(pruned[0], first[0])
    acc1, rgb1 = acc_rgb(f, fl)
    assert float(acc1.abs().max()) == 0.0 and bool((rgb1 == 1.0).all())
    mask = f.alphaMask
    again = f.prune_floaters(keep_largest=1, dry_run=True)
    assert again.n_components == 1 and again.removed_voxels == 0 and f.alphaMask is mask
    m1 = f.export_mesh(None, colors=False)
    assert mesh_components(m1.faces, m1.verts.shape[0]).n_components == 1
    f.alphaMask = None
    assert close_frames(frame(f, rays), first)      # (unmasked frames: the bound of the docstring; the tuned field's undo is exact)
    m0 = f.export_mesh(None, colors=False)
    assert mesh_components(m0.faces, m0.verts.shape[0]).n_components == 2
