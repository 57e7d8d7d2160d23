"""The general-shape path (csrc/t2n_generic.hip) with the reference loop's occupancy and NDC steps: AlphaGridMask and NDC sampling in
the render kernels (forward and backward), getDenseAlpha / updateAlphaMask / filtering_rays on wide fields (t2n_generic_dense_alpha,
t2n_generic_filter_rays), against the reference's outputs (tests/golden/general_occupancy.npz, pinned for the oracle by
tests/test_general_occupancy_oracle.py) and against the oracle on a larger wide field, a checkpoint with its mask, and a short loop shaped
like text2nerf_main.py's."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import oracle_torch as O
from tests.conftest import GOLDEN
from tests.golden import make_golden_general_occupancy_cases as K
from tests.test_general_occupancy_oracle import case_cfg, case_params
from tests.test_hip_parity import DEPTH_ATOL, RGB_ATOL, W_ATOL, W_RTOL, _grad_check, close, dev
from text2nerf_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def go():
    return dict(np.load(os.path.join(GOLDEN, "general_occupancy.npz"), allow_pickle=False))


def build(tag, params=None):
    from text2nerf_amd import TensorVMSplit
    m = TensorVMSplit(torch.tensor(K.AABB), K.GRID, dev(), **K.FIELD, **K.CASES[tag])
    m.load_state_dict({k: torch.from_numpy(v) for k, v in (params or case_params(tag)).items()}, strict=True)
    assert m._is_general()
    return m


def attach(m, vol, aabb):
    from text2nerf_amd import AlphaGridMask
    m.alphaMask = AlphaGridMask(dev(), torch.tensor(aabb), torch.from_numpy(np.asarray(vol, np.float32)).to(dev()))


def kept(m, rays, **kw):
    idx = torch.arange(rays.shape[0], dtype=torch.float32)[:, None]
    _, got = m.filtering_rays(rays, idx, **kw)
    out = np.zeros(rays.shape[0], np.uint8)
    out[got[:, 0].long().numpy()] = 1
    return out


def shared_jitter(monkeypatch, row):
    """forward draws sample_ray_ndc's shared jitter row with torch.rand_like on the rays' device; hand it the reference's captured row."""
    monkeypatch.setattr(torch, "rand_like", lambda x, **k: torch.from_numpy(row).to(x))


@pytest.mark.parametrize("tag", list(K.CASES))
def test_masked_and_ndc_renders_vs_reference(go, monkeypatch, tag):
    from text2nerf_amd import OctreeRender_trilinear_fast
    m = build(tag)
    attach(m, go[f"{tag}_mask"], K.AABB)
    rays, nrays = torch.from_numpy(go["rays"]), torch.from_numpy(go["ndc_rays"])
    with torch.no_grad():
        rgb, _, depth, w, _ = OctreeRender_trilinear_fast(rays, m, chunk=64, N_samples=-1, white_bg=True, device=dev())
    close(w, go[f"{tag}_eval_w"], atol=W_ATOL, rtol=W_RTOL)
    close(rgb, go[f"{tag}_eval_rgb"], atol=RGB_ATOL)
    close(depth, go[f"{tag}_eval_depth"], atol=DEPTH_ATOL)
    with torch.no_grad():
        rgb, depth, z, w = m(nrays, ndc_ray=True, white_bg=True)
    assert tuple(z.shape) == (1, go[f"{tag}_ndc_eval_w"].shape[1])
    close(w, go[f"{tag}_ndc_eval_w"], atol=W_ATOL, rtol=W_RTOL)
    close(rgb, go[f"{tag}_ndc_eval_rgb"], atol=RGB_ATOL)
    close(depth, go[f"{tag}_ndc_eval_depth"], atol=DEPTH_ATOL)
    torch.manual_seed(77)
    rgb, depth, _, w = m(rays, is_train=True, white_bg=True, N_samples=K.N_TRAIN)
    close(w, go[f"{tag}_train_w"], atol=W_ATOL, rtol=W_RTOL)
    close(rgb, go[f"{tag}_train_rgb"], atol=RGB_ATOL)
    close(depth, go[f"{tag}_train_depth"], atol=DEPTH_ATOL)
    if tag == "mlp":      # the gradients of the masked train render against the reference's autograd
        ca = torch.from_numpy(go["ca"]).to(dev())
        ((rgb * ca).sum() + 0.1 * depth.sum() + (w ** 2).sum()).backward()
        _grad_check(m, {k[len("mlp_grad."):]: v for k, v in go.items() if k.startswith("mlp_grad.")}, rel=5e-4)
    # NDC train with the reference's shared jitter row: outputs against the reference, gradients against the oracle's autograd (the
    # heads' directions are divided by |d| on this path only)
    m.zero_grad(set_to_none=True)
    with monkeypatch.context() as mp:
        shared_jitter(mp, go[f"{tag}_ndc_jit"])
        rgb, depth, z, w = m(nrays, ndc_ray=True, is_train=True, white_bg=True, N_samples=K.N_TRAIN)
    close(z, go[f"{tag}_ndc_train_z"], atol=2e-6)
    close(w, go[f"{tag}_ndc_train_w"], atol=W_ATOL, rtol=W_RTOL)
    close(rgb, go[f"{tag}_ndc_train_rgb"], atol=RGB_ATOL)
    close(depth, go[f"{tag}_ndc_train_depth"], atol=DEPTH_ATOL)
    ca = torch.from_numpy(np.random.Generator(np.random.PCG64(4)).uniform(-1, 1, (nrays.shape[0], 3)).astype(np.float32))
    ((rgb * ca.to(dev())).sum() + 0.1 * depth.sum() + (w ** 2).sum()).backward()
    P = O.params_from_numpy(case_params(tag), requires_grad=True)
    o = O.forward(case_cfg(tag, go[f"{tag}_mask"]), P, nrays, ndc=True, is_train=True, n_samples=K.N_TRAIN,
                  jitter=torch.from_numpy(go[f"{tag}_ndc_jit"]))
    ((o[0] * ca).sum() + 0.1 * o[1].sum() + (o[3] ** 2).sum()).backward()
    _grad_check(m, {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in P.items()}, rel=5e-4)


@pytest.mark.parametrize("tag", list(K.CASES))
def test_dense_alpha_mask_and_filters_vs_reference(go, tag):
    m = build(tag)
    frays = torch.from_numpy(go["filter_rays"])
    a0, xyz = m.getDenseAlpha(K.DENSE_GRID)
    assert tuple(xyz.shape) == tuple(K.DENSE_GRID) + (3,)
    close(a0, go[f"{tag}_dense0"], atol=1e-6, rtol=1e-5)
    assert np.array_equal(kept(m, frays, bbox_only=True), go[f"{tag}_filter_bbox"])
    new_aabb = m.updateAlphaMask(K.MASK_GRID)
    vol = m.alphaMask.alpha_volume[0, 0].cpu().numpy().astype(np.uint8)
    ref = go[f"{tag}_mask"]
    # a voxel may differ only where its 3x3x3 neighbourhood's largest dense alpha lies within rounding of the threshold
    d = np.clip(go[f"{tag}_mask_dense"], 0, 1).transpose(2, 1, 0)
    pad = np.pad(d, 1, constant_values=-np.inf)
    D, H, W = d.shape
    pooled = np.max([pad[i:i + D, j:j + H, k:k + W] for i in range(3) for j in range(3) for k in range(3)], axis=0)
    bad = (vol != ref) & (np.abs(pooled - K.ALPHA_THRES) > 1e-5)
    assert not bad.any(), f"{int(bad.sum())} mask voxels differ away from the threshold"
    if np.array_equal(vol, ref):
        close(new_aabb, go[f"{tag}_new_aabb"], atol=1e-6)
    attach(m, ref, K.AABB)          # the reference's mask: the gated dense alpha and the alpha filter on exactly that volume
    close(m.getDenseAlpha(K.DENSE_GRID)[0], go[f"{tag}_dense1"], atol=1e-6, rtol=1e-5)
    assert np.array_equal(kept(m, frays, N_samples=64, bbox_only=False), go[f"{tag}_filter_alpha"])


LGRID, LAABB, LNF = [41, 37, 33], [[-3.0, -2.5, -2.0], [3.0, 2.5, 4.0]], [0.3, 7.0]
LKW = dict(density_n_comp=[24, 20, 32], appearance_n_comp=[64, 72, 56], app_dim=27, shadingMode="MLP_Fea", fea_pe=2, view_pe=2, pos_pe=0,
           featureC=160)


def large_field(seed=3):
    from text2nerf_amd import TensorVMSplit
    params = synth.make_field_params(seed, LGRID, density_n_comp=LKW["density_n_comp"], app_n_comp=LKW["appearance_n_comp"], app_dim=27,
                                     feature_c=160, fea_pe=2, view_pe=2, pos_pe=0, shading_mode="MLP_Fea", density_scale=0.8, aabb=LAABB)
    m = TensorVMSplit(torch.tensor(LAABB), LGRID, dev(), near_far=LNF, alphaMask_thres=0.05, density_shift=-10, distance_scale=25,
                      step_ratio=1.0, fea2denseAct="softplus", **LKW)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m, params


def large_cfg(vol=None):
    return O.FieldConfig(aabb=LAABB, grid_size=LGRID, near_far=LNF, shading_mode="MLP_Fea", fea_pe=2, view_pe=2, pos_pe=0,
                         alpha_volume=None if vol is None else torch.from_numpy(vol), alpha_aabb=None if vol is None else LAABB)


def ndc_rays(H, W):
    d = torch.from_numpy(synth.frame_rays_np(H, W)[:, 3:6].copy())
    d[:, 1:] = -d[:, 1:]
    o = torch.zeros_like(d)
    o[:, 0] = torch.linspace(-0.2, 0.2, d.shape[0])
    a, b = O.ndc_rays(H, W, float(W), 1.0, o, d, blender=True)
    return torch.cat([a, b], 1).float()


def test_larger_wide_field_with_mask_and_ndc_vs_oracle():
    m, params = large_field()
    m.updateAlphaMask((48, 40, 36))
    vol = m.alphaMask.alpha_volume[0, 0].cpu().numpy()
    assert 0.02 < vol.mean() < 0.98
    cfg, P = large_cfg(vol), O.params_from_numpy(params)
    for ndc, rays in ((False, torch.from_numpy(synth.frame_rays_np(40, 56, c2w=synth.look_pose(0.2, -0.1, (0.1, 0.2, -2.5))))),
                      (True, ndc_rays(40, 56))):
        with torch.no_grad():
            rgb, depth, _, w = m(rays, ndc_ray=ndc, white_bg=True)
        st = m.stats()
        o_rgb, o_depth, _, o_w, aux = O.forward(cfg, P, rays, ndc=ndc, return_aux=True)
        close(w, o_w.numpy(), atol=W_ATOL, rtol=W_RTOL)
        close(rgb, o_rgb.numpy(), atol=RGB_ATOL)
        close(depth, o_depth.numpy(), atol=DEPTH_ATOL)
        assert st["evaluated"] == int(aux["valid"].sum()) > 0
        # the mask removes samples: the same frame without it evaluates more
        o_nomask = O.forward(large_cfg(), P, rays, ndc=ndc, return_aux=True)[4]
        assert int(o_nomask["valid"].sum()) > st["evaluated"]


def test_checkpoint_with_mask_renders_with_it(tmp_path):
    from text2nerf_amd import TensorVMSplit
    m, params = large_field(seed=4)
    m.updateAlphaMask((48, 40, 36))
    path = str(tmp_path / "wide.th")
    m.save(path)
    ckpt = torch.load(path, map_location=dev(), weights_only=False)
    kw = dict(ckpt["kwargs"])
    kw.update(device=dev())
    m2 = TensorVMSplit(**kw)
    m2.load(ckpt)
    assert m2.alphaMask is not None
    rays = torch.from_numpy(synth.frame_rays_np(24, 32, c2w=synth.look_pose(0.2, -0.1, (0.1, 0.2, -2.5))))
    with torch.no_grad():
        a = m(rays)
        b = m2(rays)
    close(b[0], a[0].cpu().numpy(), atol=0)
    close(b[3], a[3].cpu().numpy(), atol=0)
    vol = m2.alphaMask.alpha_volume[0, 0].cpu().numpy()
    o = O.forward(large_cfg(vol), O.params_from_numpy(params), rays)
    close(b[0], o[0].numpy(), atol=RGB_ATOL)


def test_reference_shaped_loop_on_a_wide_field():
    """text2nerf_main.py's order: filtering_rays(bbox_only=True) -> steps -> updateAlphaMask -> shrink -> upsample_volume_grid ->
    filtering_rays(bbox_only=False) -> steps -> evaluation."""
    from text2nerf_amd import OctreeRender_trilinear_fast, evaluation
    m, _ = large_field(seed=6)
    H, W = 24, 32
    poses = [synth.look_pose(0.2 * v - 0.2, -0.1, (0.1, 0.2, -2.5)) for v in range(3)]
    all_rays = torch.cat([torch.from_numpy(synth.frame_rays_np(H, W, c2w=p)) for p in poses])
    all_rgbs = torch.rand(all_rays.shape[0], 3, generator=torch.Generator().manual_seed(2))
    rays, rgbs = m.filtering_rays(all_rays, all_rgbs, bbox_only=True)
    assert 0 < rays.shape[0] <= all_rays.shape[0]
    opt = torch.optim.Adam(m.get_optparam_groups(0.02, 0.001), betas=(0.9, 0.99))

    def steps(n, rays, rgbs):
        g = torch.Generator().manual_seed(n)
        for _ in range(n):
            idx = torch.randint(0, rays.shape[0], (512,), generator=g)
            rgb, _, _, _, _ = OctreeRender_trilinear_fast(rays[idx], m, chunk=512, N_samples=-1, white_bg=True, is_train=True, device=dev())
            loss = ((rgb - rgbs[idx].to(dev())) ** 2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            assert torch.isfinite(loss)
    steps(3, rays, rgbs)
    new_aabb = m.updateAlphaMask((40, 36, 32))
    m.shrink(new_aabb)
    m.upsample_volume_grid([44, 40, 36])
    opt = torch.optim.Adam(m.get_optparam_groups(0.02, 0.001), betas=(0.9, 0.99))
    rays, rgbs = m.filtering_rays(all_rays, all_rgbs, bbox_only=False)
    assert 0 < rays.shape[0]
    steps(3, rays, rgbs)
    for p in m.parameters():
        assert bool(torch.isfinite(p).all())

    class _Dataset:
        split, img_wh, near_far = "test", (W, H), LNF
        all_rays_split = all_rays.view(3, H * W, -1)
    args = SimpleNamespace(batch_size=4096, push_depth=2.0)
    evaluation(_Dataset(), m, args, OctreeRender_trilinear_fast, None, N_vis=-1, N_samples=-1, white_bg=True, compute_extra_metrics=False,
               device=dev())
    # the final masked frame against the oracle on the field's current parameters, box and mask
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    vol = m.alphaMask.alpha_volume[0, 0].cpu().numpy()
    cfg = O.FieldConfig(aabb=m.aabb.cpu().tolist(), grid_size=[int(g) for g in m.gridSize], near_far=LNF, shading_mode="MLP_Fea", fea_pe=2,
                        view_pe=2, pos_pe=0, alpha_volume=torch.from_numpy(vol), alpha_aabb=m.alphaMask.aabb.cpu().tolist())
    frame = all_rays[:H * W]
    with torch.no_grad():
        rgb, depth, _, w = m(frame)
    assert bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(depth).all())
    o = O.forward(cfg, O.params_from_numpy(sd), frame)
    close(w, o[3].numpy(), atol=W_ATOL, rtol=W_RTOL)
    close(rgb, o[0].numpy(), atol=RGB_ATOL)
    close(depth, o[1].numpy(), atol=DEPTH_ATOL)
