"""GPU parity tests proper: the HIP path (through the C-ABI of libt2n_hip.so) against (a) the golden vectors generated
from the reference and (b) the oracle on seeded inputs. Run with `-m gpu` on an MI355X.

Tolerances (BASELINE.json north_star): <= 1e-4 RGB, <= 1e-5 sigma (atol + rtol, SURVEY.md §7: fp32 features reach
|40|, so sigma/feature checks carry an rtol of a few fp32 ulp)."""
import numpy as np
import pytest
import torch

from text2nerf_amd import synth
from tests.conftest import TINY

pytestmark = pytest.mark.gpu

RGB_ATOL = 1e-4
SIGMA_ATOL, SIGMA_RTOL = 1e-5, 1e-5
W_ATOL, W_RTOL = 5e-6, 5e-5
DEPTH_ATOL = 2e-4


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def close(a, b, atol, rtol=0.0, msg=""):
    a = a.detach().float().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    np.testing.assert_allclose(a, b, atol=atol, rtol=rtol, err_msg=msg)


def make_field(params, grid, aabb, near_far, shading="MLP_Fea_noview"):
    from text2nerf_amd import TensorVMSplit
    m = TensorVMSplit(torch.tensor(aabb, dtype=torch.float32), list(grid), dev(), density_n_comp=[16] * 3,
                      appearance_n_comp=[48] * 3, app_dim=27, near_far=near_far, shadingMode=shading,
                      alphaMask_thres=1e-4, density_shift=-10, distance_scale=25, pos_pe=0, view_pe=0, fea_pe=6,
                      featureC=128, step_ratio=1.0, fea2denseAct="softplus")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m                    # (product defaults: early termination is opt-in, tests/test_early_termination.py switches it on)


@pytest.fixture(scope="module")
def field(tiny_params):
    return make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])


def test_library_is_native():
    from text2nerf_amd import _lib
    lib = _lib.load()
    assert lib.t2n_version() >= 100


def test_g1_ray_generation(tiny):
    from text2nerf_amd import get_ray_directions, get_rays, generate_rays
    d = get_ray_directions(6, 8, [9.0, 7.5], center=[4, 3])
    close(d, tiny["g1_dirs_raw"], atol=1e-7)
    dn = get_ray_directions(6, 8, [9.0, 7.5], center=[4, 3], normalize=True)
    ro, rd = get_rays(dn, torch.from_numpy(tiny["g1_c2w"]))
    close(torch.cat([ro, rd], 1), tiny["g1_rays"], atol=3e-7)
    r6 = generate_rays(6, 8, [9.0, 7.5, 4, 3], tiny["g1_c2w"])
    close(r6, tiny["g1_rays"], atol=3e-7)


def test_g3_density(tiny, field):
    xyz = torch.from_numpy(tiny["g3_xyz"]).to(dev())
    close(field.compute_densityfeature(xyz), tiny["g3_feat"], atol=2e-5, rtol=SIGMA_RTOL)
    close(field.compute_sigma(xyz), tiny["g3_sigma"], atol=SIGMA_ATOL, rtol=SIGMA_RTOL)
    close(field.normalize_coord(torch.from_numpy(tiny["g3_norm_in"]).to(dev())), tiny["g3_norm_out"], atol=0)


def test_g3_density_out_of_range_points(field):
    """zeros padding: far-outside points read nothing; half-outside points read the in-range taps only."""
    from oracle import oracle_torch as O
    xyz = torch.tensor([[5.0, 0.0, 0.0], [-3.0, -3.0, -3.0], [1.02, 0.1, -0.2], [-1.03, 0.99, 1.04], [0.3, 1.001, -1.0],
                        [1e6, 0, 0]], dtype=torch.float32)
    P = O.params_from_numpy({k: v.detach().cpu().numpy() for k, v in field.state_dict().items()})
    ref = O.density_feature(P, xyz)
    close(field.compute_densityfeature(xyz.to(dev())), ref.numpy(), atol=2e-5, rtol=1e-5)


def test_g4_raw2alpha(tiny):
    from text2nerf_amd import raw2alpha
    a, w, bg = raw2alpha(torch.from_numpy(tiny["g4_sigma"]).to(dev()), torch.from_numpy(tiny["g4_dist"]).to(dev()))
    close(a, tiny["g4_alpha"], atol=2e-7)
    close(w, tiny["g4_weight"], atol=5e-7, rtol=1e-5)
    close(bg, tiny["g4_bg"], atol=5e-7, rtol=1e-5)


@pytest.mark.parametrize("exact", [False, True])
def test_g5_appearance_mlp(tiny, field, exact):
    """basis_mat + PE + MLP on the matrix cores: default = f16 two-way-split products (22-bit mantissa, fp32 accumulate),
    exact = fp32 MFMA. Both must sit far inside the 1e-4 RGB budget."""
    xyz = torch.from_numpy(tiny["g3_xyz"][:1024]).to(dev())
    field.mlp_exact_fp32 = exact
    try:
        feat, rgb = field.shade(xyz)
        close(feat, tiny["g5_appfeat"], atol=5e-6, rtol=1e-5, msg="app features (gather + basis_mat)")
        close(rgb, tiny["g5_rgb_mlp"], atol=1e-5 if not exact else 2e-6, msg="PE + MLP + sigmoid")
        close(field.compute_appfeature(xyz[:77]), tiny["g5_appfeat"][:77], atol=5e-6, rtol=1e-5)   # ragged tile
        err = float((rgb.cpu() - torch.from_numpy(tiny["g5_rgb_mlp"])).abs().max())
        print(f"MLP head max |rgb - reference| ({'fp32 MFMA' if exact else 'f16x2 split'}): {err:.2e}")
    finally:
        field.mlp_exact_fp32 = False


def test_g5_sh_head(tiny, tiny_params_sh):
    f = make_field(tiny_params_sh, TINY["grid"], TINY["aabb"], TINY["near_far"], shading="SH")
    xyz = torch.from_numpy(tiny["g3_xyz"][:1024]).to(dev())
    feat, rgb = f.shade(xyz, viewdirs=torch.from_numpy(tiny["g5_viewdirs"]).to(dev()))
    # the SH field shares every factor tensor with the MLP field (same seed), so features match g5 too
    close(feat, tiny["g5_appfeat"], atol=5e-6, rtol=1e-5)
    close(rgb, tiny["g5_rgb_sh"], atol=5e-6)


@pytest.mark.parametrize("tag,kw", [("eval", dict(is_train=False, white_bg=True, N_samples=-1)),
                                    ("eval70", dict(is_train=False, white_bg=True, N_samples=70)),
                                    ("evalblack", dict(is_train=False, white_bg=False, N_samples=-1))])
def test_g6_forward_eval(tiny, field, tag, kw):
    rays = torch.from_numpy(tiny["tiny_rays"])          # arrives on the CPU like the reference's rays
    with torch.no_grad():
        rgb, depth, z, w = field(rays, **kw)
    close(z, np.broadcast_to(tiny[f"g6_{tag}_z"], z.shape), atol=0, msg="z_vals are bit-exact")
    close(w, tiny[f"g6_{tag}_w"], atol=W_ATOL, rtol=W_RTOL)
    close(rgb, tiny[f"g6_{tag}_rgb"], atol=RGB_ATOL)
    close(depth, tiny[f"g6_{tag}_depth"], atol=DEPTH_ATOL)
    if tag != "eval70":
        # which samples exist must agree exactly: box mask (golden G2) AND the eval z gate, counted by the kernel
        n_valid = int((tiny["g2_eval_valid"] & (tiny["g2_eval_pts"][..., 2] > 2.0)).sum())
        assert field.stats()["evaluated"] == n_valid


def test_g6_forward_train_rng_stream(tiny, field):
    rays = torch.from_numpy(tiny["tiny_rays"])
    torch.manual_seed(123)
    with torch.no_grad():
        rgb, depth, z, w = field(rays, is_train=True, white_bg=True, N_samples=40)
    close(z, tiny["g6_train_z"], atol=0, msg="jitter drawn from the CPU generator like the reference")
    close(w, tiny["g6_train_w"], atol=W_ATOL, rtol=W_RTOL)
    close(rgb, tiny["g6_train_rgb"], atol=RGB_ATOL)
    close(depth, tiny["g6_train_depth"], atol=DEPTH_ATOL)


def test_g6_sh_field(tiny, tiny_params_sh):
    f = make_field(tiny_params_sh, TINY["grid"], TINY["aabb"], TINY["near_far"], shading="SH")
    with torch.no_grad():
        rgb, depth, _, _ = f(torch.from_numpy(tiny["tiny_rays"]))
    close(rgb, tiny["g6_sh_rgb"], atol=RGB_ATOL)
    close(depth, tiny["g6_sh_depth"], atol=DEPTH_ATOL)


def test_g7_harness(tiny, field):
    from text2nerf_amd import OctreeRender_trilinear_fast
    with torch.no_grad():
        out = OctreeRender_trilinear_fast(torch.from_numpy(tiny["tiny_rays"]), field, chunk=64, N_samples=-1,
                                          ndc_ray=False, white_bg=True, is_train=False, device=dev())
    assert len(out) == 5 and out[1] is None
    close(out[0], tiny["g7_rgb"], atol=RGB_ATOL)
    close(out[2], tiny["g7_depth"], atol=DEPTH_ATOL)
    close(out[3], tiny["g7_w"], atol=W_ATOL, rtol=W_RTOL)
    close(out[4], np.broadcast_to(tiny["g7_z"], out[4].shape), atol=0)
    # weights not materialised: same images, None in the slots the reference's evaluation() discards
    field.materialize_weights = False
    try:
        with torch.no_grad():
            o2 = OctreeRender_trilinear_fast(torch.from_numpy(tiny["tiny_rays"]), field, chunk=64)
    finally:
        field.materialize_weights = True
    assert o2[3] is None and o2[4] is None
    assert torch.equal(o2[0], out[0]) and torch.equal(o2[2], out[2])


def test_empty_and_ragged(field):
    with torch.no_grad():
        rgb, depth, z, w = field(torch.zeros(0, 6))
    assert rgb.shape == (0, 3) and depth.shape == (0,) and w.shape == (0, field.nSamples)
    rays = torch.tensor([[30.0, 0, 0, 0, 1, 0]])       # one ray that misses the box: pure background
    with torch.no_grad():
        rgb, depth, z, w = field(rays)
    assert torch.all(rgb == 1.0) and float(w.abs().sum()) == 0.0
    assert float(depth[0]) == 0.0                      # (1-acc) * d_z with d_z = 0


@pytest.mark.parametrize("scene,seed", [("S1-soft", 0), ("S2", 1)])
def test_big300_golden_and_oracle(big300, scene, seed):
    aabb = [[-8.0] * 3, [8.0] * 3]
    params = synth.make_field_params(seed, [300] * 3, scene=scene, aabb=aabb)
    f = make_field(params, [300] * 3, aabb, [0.5, 8.0])
    assert f.nSamples == 518
    full = synth.frame_rays_np(800, 800)
    rays = torch.from_numpy(full[big300[f"{scene}_idx"]])
    with torch.no_grad():
        rgb, depth, z, w = f(rays)
    close(rgb, big300[f"{scene}_rgb"], atol=RGB_ATOL)
    close(depth, big300[f"{scene}_depth"], atol=DEPTH_ATOL)
    close(w.sum(-1), big300[f"{scene}_acc"], atol=2e-5)
    close(w[:16], big300[f"{scene}_w_first16"], atol=W_ATOL, rtol=W_RTOL)
    napp = int((w > 1e-4).sum())
    assert abs(napp - int(big300[f"{scene}_napp"].sum())) <= 3
    assert f.stats()["appearance"] == napp
    torch.manual_seed(5)
    with torch.no_grad():
        rgb, depth, z, w = f(rays, is_train=True, N_samples=259)
    close(rgb, big300[f"{scene}_train_rgb"], atol=RGB_ATOL)
    close(depth, big300[f"{scene}_train_depth"], atol=DEPTH_ATOL)
    close(w.sum(-1), big300[f"{scene}_train_acc"], atol=2e-5)

    # oracle on a seeded batch the goldens do not cover (random pose, 2048 rays)
    from oracle import oracle_torch as O
    cfg = O.FieldConfig(aabb=aabb, grid_size=[300] * 3)
    P = O.params_from_numpy(params)
    pose = synth.look_pose(yaw=0.4, pitch=-0.15, center=(0.5, -0.2, 0.3))
    r2 = synth.frame_rays_np(800, 800, c2w=pose)
    sel = np.random.Generator(np.random.PCG64(9)).choice(r2.shape[0], 2048, replace=False)
    r2 = torch.from_numpy(r2[np.sort(sel)])
    o_rgb, o_depth, o_z, o_w = O.forward(cfg, P, r2)
    with torch.no_grad():
        rgb, depth, z, w = f(r2)
    close(rgb, o_rgb.numpy(), atol=RGB_ATOL)
    close(depth, o_depth.numpy(), atol=DEPTH_ATOL)
    close(w, o_w.numpy(), atol=W_ATOL, rtol=W_RTOL)
    close(z, o_z.numpy(), atol=0)


def test_full_frame_properties_and_sharding():
    """C2 size (800x800, N=518, 300^3): size-independent properties + shard equivalence + sub-launch equivalence."""
    import os
    aabb = [[-8.0] * 3, [8.0] * 3]
    f = make_field(synth.make_field_params(0, [300] * 3, scene="S1-soft", aabb=aabb), [300] * 3, aabb, [0.5, 8.0])
    f.materialize_weights = False
    rays = torch.from_numpy(synth.frame_rays_np(800, 800)).to(dev())
    with torch.no_grad():
        rgb, depth, _, _ = f(rays)
        st = f.stats()
        rgb2, depth2, _, _ = f(rays)
    assert torch.equal(rgb, rgb2) and torch.equal(depth, depth2), "render is deterministic run to run"
    assert float(rgb.min()) >= 0.0 and float(rgb.max()) <= 1.0 and bool(torch.isfinite(depth).all())
    R = rays.shape[0]
    assert 0.20 < st["evaluated"] / (R * 518) < 0.27          # 23.4 % of nominal samples are evaluated
    assert 5.0 < st["appearance"] / R < 9.0                    # 6.7 appearance samples per ray on S1-soft
    # ray-tile sharding: rendering two halves (what two ranks do) is bitwise the whole frame
    with torch.no_grad():
        a = f(rays[: R // 2])
        b = f(rays[R // 2:])
    assert torch.equal(torch.cat([a[0], b[0]]), rgb) and torch.equal(torch.cat([a[1], b[1]]), depth)
    # forcing many sub-launches through a small workspace changes nothing
    old = os.environ.get("T2N_WORKSPACE_GIB")
    os.environ["T2N_WORKSPACE_GIB"] = "0.5"
    try:
        from text2nerf_amd import tensorf as tf
        tf._WORKSPACE.clear()
        with torch.no_grad():
            c = f(rays)
    finally:
        if old is None:
            os.environ.pop("T2N_WORKSPACE_GIB")
        else:
            os.environ["T2N_WORKSPACE_GIB"] = old
        tf._WORKSPACE.clear()
    assert torch.equal(c[0], rgb) and torch.equal(c[1], depth)
    # weights materialised: sum of weights == 1 - background weight, z_vals start at near
    f.materialize_weights = True
    with torch.no_grad():
        rgb3, depth3, z, w = f(rays[:4096])
    assert torch.equal(rgb3, rgb[:4096])
    assert float((w.sum(-1) - 1).max()) < 1e-5 and float(w.min()) >= 0.0
    assert torch.all(z[:, 0] == 0.5)


def test_unsupported_configs_fail_loudly():
    from text2nerf_amd import TensorVMSplit
    from text2nerf_amd._lib import T2NError
    aabb = torch.tensor([[-1.0] * 3, [1.0] * 3])
    with pytest.raises(T2NError):
        TensorVMSplit(aabb, [8, 8, 8], dev(), shadingMode="MLP_PE")
    base = dict(density_n_comp=[16] * 3, appearance_n_comp=[48] * 3, shadingMode="MLP_Fea_noview", fea_pe=6, step_ratio=1.0)
    for kw in (dict(featureC=512), dict(fea_pe=17), dict(app_dim=65)):
        with pytest.raises(T2NError):       # beyond even the general-shape path: rejected at construction
            TensorVMSplit(aabb, [8, 8, 8], dev(), **dict(base, **kw))
    for kw in (dict(density_n_comp=[32, 16, 16]), dict(appearance_n_comp=[96, 48, 48]), dict(featureC=256), dict(fea_pe=8), dict(app_dim=30)):
        wide = TensorVMSplit(aabb, [8, 8, 8], dev(), **dict(base, **kw))     # beyond the tuned kernels: the general-shape path renders it
        with torch.no_grad():
            rgb, depth, _, _ = wide(torch.tensor([[0.0, 0.0, -3.0, 0.0, 0.0, 1.0]] * 4))
        assert rgb.shape == (4, 3) and bool(torch.isfinite(rgb).all())
        for call in (lambda: wide.sync_params(), lambda: wide.compute_alpha(torch.zeros(4, 3, device=dev()))):
            with pytest.raises(T2NError):   # ... but it has no native field: the stage entry points say so
                call()
    ok = TensorVMSplit(aabb, [8, 8, 8], dev(), density_n_comp=[16] * 3, appearance_n_comp=[48] * 3,
                       shadingMode="MLP_Fea_noview", fea_pe=6, step_ratio=1.0)
    with pytest.raises(T2NError):
        ok.cpu()(torch.zeros(4, 6))   # parameters moved off the GPU: no host fallback


def _grad_check(f, named_ref, rel, rel_l2=None, cos_gap=None):
    """Per tensor: max |dg| / max |g| <= rel (sensitive to ONE flipped sample); optionally also relative L2 error <= rel_l2 and
    1 - cosine <= cos_gap (whole-tensor agreement, insensitive to a single knife-edge element). Returns the worst of the first.
    `f`: a field (its parameters' .grad are checked) or a dict of gradient arrays by parameter name."""
    worst, l2, cg = {}, {}, {}
    got = f if isinstance(f, dict) else {k: p.grad for k, p in f.named_parameters()}
    for k, h in got.items():
        g = named_ref[k].astype(np.float64)
        assert h is not None, k
        h = h.detach().cpu().numpy() if isinstance(h, torch.Tensor) else np.asarray(h)
        h = h.astype(np.float64).reshape(g.shape)
        scale = float(np.abs(g).max()) + 1e-12
        worst[k] = float(np.abs(h - g).max()) / scale
        ng, nh = float(np.linalg.norm(g)), float(np.linalg.norm(h))
        l2[k] = float(np.linalg.norm(h - g)) / (ng + 1e-30)
        cg[k] = 1.0 - float((h * g).sum()) / (ng * nh + 1e-30) if ng > 0 and nh > 0 else 0.0
    _grad_check.last = {"max_rel": worst, "rel_l2": l2, "one_minus_cos": cg}     # (set first: a failing caller can still print them)
    bad = {k: v for k, v in worst.items() if v > rel}
    assert not bad, f"gradient mismatch (max abs err / max |g|): {bad}"
    if rel_l2 is not None:
        bad = {k: v for k, v in l2.items() if v > rel_l2}
        assert not bad, f"gradient mismatch (relative L2 error): {bad}"
    if cos_gap is not None:
        bad = {k: v for k, v in cg.items() if v > cos_gap}
        assert not bad, f"gradient mismatch (1 - cosine): {bad}"
    return worst


def test_g8_gradients_vs_reference_autograd(tiny, tiny_params):
    """a-15: backward through the whole path (train mode, captured jitter) vs the reference's autograd (golden G8)."""
    f = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    rays = torch.from_numpy(tiny["tiny_rays"])
    torch.manual_seed(123)
    rgb, depth, z, w = f(rays, is_train=True, white_bg=True, N_samples=40)
    assert rgb.requires_grad and w.requires_grad and not z.requires_grad
    ca, cb, cc = [torch.from_numpy(tiny[k]).to(dev()) for k in ("g8_ca", "g8_cb", "g8_cc")]
    loss = (rgb * ca).sum() + (depth * cb).sum() + (w * cc).sum()
    close(loss, tiny["g8_loss"], atol=5e-4)
    loss.backward()
    ref = {k[len("g8_grad."):]: v for k, v in tiny.items() if k.startswith("g8_grad.")}
    worst = _grad_check(f, ref, rel=2e-4)
    print("max relative gradient errors:", {k: f"{v:.1e}" for k, v in worst.items()})
    # an optimiser step on the reference-layout parameters re-uploads transparently
    opt = torch.optim.Adam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
    before = f.density_plane[0].detach().clone()
    opt.step()
    assert not torch.equal(before, f.density_plane[0].detach())
    with torch.no_grad():
        rgb2, _, _, _ = f(rays)
    assert bool(torch.isfinite(rgb2).all())


def test_g8_gradients_with_forward_kept_activation_rows(tiny, tiny_params):
    """From the second iteration on the training forward keeps the MLP activation rows in spare KEEP_CTX workspace (sized from
    the previous backward's row count) and the backward skips its appearance recompute: same gradients against the
    reference's autograd (golden G8) — with an ample guess, with a guess that is too small (the backward falls back to
    recomputing) and with the feature switched off."""
    rays = torch.from_numpy(tiny["tiny_rays"])
    ca, cb, cc = [torch.from_numpy(tiny[k]).to(dev()) for k in ("g8_ca", "g8_cb", "g8_cc")]
    ref = {k[len("g8_grad."):]: v for k, v in tiny.items() if k.startswith("g8_grad.")}
    f = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])

    def run(expect_rgb=None):
        for p in f.parameters():
            p.grad = None
        torch.manual_seed(123)
        rgb, depth, z, w = f(rays, is_train=True, white_bg=True, N_samples=40)
        loss = (rgb * ca).sum() + (depth * cb).sum() + (w * cc).sum()
        close(loss, tiny["g8_loss"], atol=5e-4)
        loss.backward()
        return _grad_check(f, ref, rel=2e-4), rgb.detach().clone()

    _, rgb0 = run()                               # first iteration: no guess yet -> recompute path
    assert f._ctx_rows_hint >= 32
    hint = f._ctx_rows_hint
    w1, rgb1 = run()                              # kept rows
    close(rgb1, rgb0.cpu().numpy(), atol=2e-6)    # exact-fp32 head instead of the f16-split one in the forward
    f._ctx_rows_hint = 32                         # far too small: the forward keeps one tile, the backward recomputes
    run()
    f.keep_activation_rows = False
    run()
    assert f._ctx_rows_hint == 0
    f.keep_activation_rows = True
    run(); f._ctx_rows_hint = hint
    w2, _ = run()
    print("kept-rows max relative gradient errors:", {k: f"{v:.1e}" for k, v in w2.items()})


def test_train_batch_gradients_vs_oracle_300():
    """C3-shaped: 300^3 field, random rays of a small-baseline pose set, N=259, is_train — gradients vs the oracle's
    autograd (fp32 CPU). Only rgb/depth/weights losses of the driver's form (MSE + transmittance-style weight term)."""
    from oracle import oracle_torch as O
    aabb = [[-8.0] * 3, [8.0] * 3]
    params = synth.make_field_params(0, [300] * 3, scene="S1-soft", aabb=aabb)
    f = make_field(params, [300] * 3, aabb, [0.5, 8.0])
    poses = synth.local_fixed_like_poses(9)
    rng = np.random.Generator(np.random.PCG64(1024))
    allr = np.concatenate([synth.frame_rays_np(64, 64, c2w=p) for p in poses])
    rays = torch.from_numpy(allr[rng.choice(allr.shape[0], 384, replace=False)])
    tgt = torch.from_numpy(rng.uniform(0, 1, (384, 3)).astype(np.float32))
    tgd = torch.from_numpy(rng.uniform(2, 7, (384,)).astype(np.float32))

    def loss_fn(rgb, depth, z, w, d):
        m = (z < (tgd.to(d)[:, None] - 0.1)).float()
        return ((rgb - tgt.to(d)) ** 2).mean() + 0.005 * ((depth - tgd.to(d)) ** 2).mean() + 1e3 * ((w * m) ** 2).mean()

    torch.manual_seed(77)
    jit = torch.rand(384, 1)
    torch.manual_seed(77)
    out = f(rays, is_train=True, white_bg=True, N_samples=259)
    loss_fn(*out, dev()).backward()
    cfg = O.FieldConfig(aabb=aabb, grid_size=[300] * 3)
    P = O.params_from_numpy(params, requires_grad=True)
    o = O.forward(cfg, P, rays, white_bg=True, is_train=True, n_samples=259, jitter=jit)
    lo = loss_fn(*o, "cpu")
    lo.backward()
    ref = {k: v.grad.numpy() for k, v in P.items()}
    worst = _grad_check(f, ref, rel=1e-3)
    print("300^3 train-batch max relative gradient errors:", {k: f"{v:.1e}" for k, v in worst.items()})


def test_tile_marcher_matches_per_ray_marcher(big300):
    """frame_width hint -> 8x8-pixel tile marcher (shared per-step dot-product tables, sequential transmittance): same samples (exact
    counts, bit-exact z), weights/rgb/depth equal to the per-ray marcher within fp32 scan re-association, goldens hold,
    ragged image sizes (not multiples of 8) and multi-band sub-launches covered."""
    import os
    from text2nerf_amd import tensorf as tf
    aabb = [[-8.0] * 3, [8.0] * 3]
    f = make_field(synth.make_field_params(0, [300] * 3, scene="S1-soft", aabb=aabb), [300] * 3, aabb, [0.5, 8.0])
    for (H, W) in ((200, 200), (37, 53)):
        rays = torch.from_numpy(synth.frame_rays_np(H, W, c2w=synth.look_pose(0.2, -0.1, (0.3, 0.1, -0.5)))).to(dev())
        with torch.no_grad():
            f.frame_width = 0
            a = f(rays)
            sa = f.stats()
            f.frame_width = W
            b = f(rays)
            sb = f.stats()
        assert sa["evaluated"] == sb["evaluated"] and abs(sa["appearance"] - sb["appearance"]) <= 2
        assert torch.equal(a[2], b[2])                                   # z_vals
        close(b[3], a[3].cpu().numpy(), atol=2e-6, rtol=2e-5)            # weights
        close(b[0], a[0].cpu().numpy(), atol=2e-5)
        close(b[1], a[1].cpu().numpy(), atol=5e-5)
    # golden rays embedded in a full 800x800 frame rendered by the tile marcher through several sub-launches
    full = torch.from_numpy(synth.frame_rays_np(800, 800)).to(dev())
    f.frame_width = 800
    f.materialize_weights = False
    old = os.environ.get("T2N_WORKSPACE_GIB")
    os.environ["T2N_WORKSPACE_GIB"] = "1.0"
    try:
        tf._WORKSPACE.clear()
        with torch.no_grad():
            rgb, depth, _, _ = f(full)
    finally:
        if old is None:
            os.environ.pop("T2N_WORKSPACE_GIB")
        else:
            os.environ["T2N_WORKSPACE_GIB"] = old
        tf._WORKSPACE.clear()
    idx = torch.from_numpy(big300["S1-soft_idx"]).to(dev())
    close(rgb[idx], big300["S1-soft_rgb"], atol=RGB_ATOL)
    close(depth[idx], big300["S1-soft_depth"], atol=DEPTH_ATOL)


def test_tile_marcher_with_alpha_mask_matches_per_ray_marcher():
    """AlphaGridMask branch (models/tensorBase.py:451-456) on the tile marcher: a checkerboard-ish occupancy volume leaves gaps
    inside every ray's sample window; same evaluated counts, outputs equal to the per-ray marcher in both output modes, also
    with rays pushed over the staging capacity (their spill rows must stay gap-free)."""
    from text2nerf_amd import AlphaGridMask
    aabb = [[-8.0] * 3, [8.0] * 3]
    f = make_field(synth.make_field_params(0, [128] * 3, scene="S1-soft", aabb=aabb, density_scale=1.0), [128] * 3, aabb, [0.5, 8.0])
    g = np.random.Generator(np.random.PCG64(77))
    vol = (g.uniform(size=(24, 20, 28)) < 0.55).astype(np.float32)
    f.alphaMask = AlphaGridMask(dev(), torch.tensor(aabb), torch.from_numpy(vol))
    for (H, W, n) in ((64, 72, 200), (33, 40, 40)):
        rays = torch.from_numpy(synth.frame_rays_np(H, W, c2w=synth.look_pose(0.3, 0.05, (0.0, 0.0, 2.0)))).to(dev())
        with torch.no_grad():
            f.frame_width = 0
            f.materialize_weights = True
            a = f(rays, N_samples=n)
            sa = f.stats()
            f.frame_width = W
            b = f(rays, N_samples=n)
            sb = f.stats()
            f.materialize_weights = False
            c = f(rays, N_samples=n)
            sc = f.stats()
        assert sa["evaluated"] == sb["evaluated"] == sc["evaluated"] and 0 < sa["evaluated"]
        assert abs(sa["appearance"] - sb["appearance"]) <= 2 and sb["appearance"] == sc["appearance"]
        assert torch.equal(a[2], b[2])
        close(b[3], a[3].cpu().numpy(), atol=2e-6, rtol=2e-5)
        for out in (b, c):
            close(out[0], a[0].cpu().numpy(), atol=2e-5)
            close(out[1], a[1].cpu().numpy(), atol=5e-5)
    f.frame_width = 0
    f.materialize_weights = True


def test_tile_marcher_low_resolution_frames_gather_directly():
    """Frames whose neighbouring rays are many texels apart (24x24 pixels over a 300^3 field): a tile's taps span more than the
    4x4 table on most steps, which then gather directly; steps near the camera still take the table path. Odd sample counts
    and ragged sizes through both output modes (whole weights / z_vals rows, and rgb / depth only)."""
    aabb = [[-8.0] * 3, [8.0] * 3]
    f = make_field(synth.make_field_params(0, [300] * 3, scene="S1-soft", aabb=aabb), [300] * 3, aabb, [0.5, 8.0])
    for (H, W, n) in ((24, 24, 45), (40, 56, 131)):
        rays = torch.from_numpy(synth.frame_rays_np(H, W, c2w=synth.look_pose(-0.15, 0.1, (0.2, -0.1, -0.4)))).to(dev())
        with torch.no_grad():
            f.frame_width = 0
            f.materialize_weights = True
            a = f(rays, N_samples=n)
            sa = f.stats()
            f.frame_width = W
            b = f(rays, N_samples=n)
            sb = f.stats()
            f.materialize_weights = False
            c = f(rays, N_samples=n)
            sc = f.stats()
        assert sa["evaluated"] == sb["evaluated"] == sc["evaluated"] and sa["evaluated"] > 0
        assert abs(sa["appearance"] - sb["appearance"]) <= 2 and sb["appearance"] == sc["appearance"]
        assert torch.equal(a[2], b[2])                                   # z_vals rows, bit-exact
        close(b[3], a[3].cpu().numpy(), atol=2e-6, rtol=2e-5)            # weights rows
        for out in (b, c):
            close(out[0], a[0].cpu().numpy(), atol=2e-5)
            close(out[1], a[1].cpu().numpy(), atol=5e-5)
        assert torch.equal(b[0], c[0]) and torch.equal(b[1], c[1])       # the two output modes run the same arithmetic


@pytest.mark.parametrize("seed", [7, 8, 9, 10])
def test_g6_train_black_background_coin(tiny, field, seed):
    """RNG stream parity: jitter draw, then the background coin (models/tensorBase.py:313-317,497), both on the CPU generator."""
    torch.manual_seed(seed)
    with torch.no_grad():
        rgb, depth, _, _ = field(torch.from_numpy(tiny["tiny_rays"]), is_train=True, white_bg=False, N_samples=40)
    close(rgb, tiny[f"g6_trainblack{seed}_rgb"], atol=RGB_ATOL)
    close(depth, tiny[f"g6_trainblack{seed}_depth"], atol=DEPTH_ATOL)


def test_g16_filtering_rays_bbox(tiny, field):
    rays = torch.from_numpy(tiny["g16_rays"])
    kept, rgbs = field.filtering_rays(rays, torch.zeros(rays.shape[0], 3), bbox_only=True)
    assert np.array_equal(kept.numpy(), tiny["g16_kept"]) and rgbs.shape[0] == kept.shape[0]


def test_anisotropic_grid_outside_rays_and_long_sampling():
    """Grid 96x64x48 in a non-cubic box, rays starting OUTSIDE the box from all sides, N up to 1500 (> one LDS chunk many
    times over) and N = 1: vs the oracle."""
    from oracle import oracle_torch as O
    grid, aabb, nf = [96, 64, 48], [[-3.0, -2.0, -1.5], [3.0, 2.0, 1.5]], [0.1, 12.0]
    params = synth.make_field_params(21, grid, density_scale=0.8, aabb=aabb)
    f = make_field(params, grid, aabb, nf)
    f.z_gate = -100.0          # the hard-coded eval gate (world z > 2) would hide this small box: move it out of the way
    f._handle = None           # re-create the native field with the new scalar
    f._uploaded_key = None
    g = np.random.Generator(np.random.PCG64(17))
    o = g.normal(0, 1, (600, 3)).astype(np.float32)
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * 7.0
    tgt = g.uniform(-1, 1, (600, 3)).astype(np.float32) * np.array([2.5, 1.5, 1.0], np.float32)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = torch.from_numpy(np.concatenate([o, d], 1).astype(np.float32))
    cfg = O.FieldConfig(aabb=aabb, grid_size=grid, near_far=nf, z_gate=-100.0)
    P = O.params_from_numpy(params)
    for n in (-1, 1500, 1, 64, 65):
        o_rgb, o_depth, o_z, o_w = O.forward(cfg, P, rays, n_samples=n)
        with torch.no_grad():
            rgb, depth, z, w = f(rays, N_samples=n)
        close(z, o_z.numpy(), atol=0)
        close(w, o_w.numpy(), atol=W_ATOL, rtol=W_RTOL, msg=f"N={n}")
        close(rgb, o_rgb.numpy(), atol=RGB_ATOL)
        close(depth, o_depth.numpy(), atol=DEPTH_ATOL)
        assert f.stats()["appearance"] == int((o_w > 1e-4).sum()) or abs(f.stats()["appearance"] - int((o_w > 1e-4).sum())) <= 2


def test_f1_fused_tv_adam_matches_torch(tiny, tiny_params):
    """TVAdam (HIP TV-gradient + Adam kernels) vs the reference-form step (TV terms in the loss graph +
    torch.optim.Adam) over several iterations on the same render loss."""
    from text2nerf_amd.losses import TVLoss
    from text2nerf_amd.optim import TVAdam
    rays = torch.from_numpy(tiny["tiny_rays"])
    tgt = torch.from_numpy(tiny["g6_train_rgb"]).to(dev()) * 0.5

    def run(fused):
        f = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
        groups = f.get_optparam_groups(0.02, 1e-3)
        if fused == "device":     # factor tensors stepped on the device's channel-last copies from device-side gradients
            opt = TVAdam(groups, betas=(0.9, 0.99), field=f)
        else:
            opt = TVAdam(groups, betas=(0.9, 0.99)) if fused else torch.optim.Adam(groups, betas=(0.9, 0.99))
        tv = TVLoss()
        torch.manual_seed(5)
        for it in range(4):
            rgb, depth, z, w = f(rays, is_train=True, white_bg=True, N_samples=40)
            loss = ((rgb - tgt) ** 2).mean() + 0.005 * (depth ** 2).mean()
            if not fused:
                loss = loss + f.TV_loss_density(tv) * 0.1 + f.TV_loss_app(tv) * 0.01
            opt.zero_grad()
            loss.backward()
            if fused:
                opt.step(tv=[(f.density_plane, 0.1), (f.app_plane, 0.01)])
            else:
                opt.step()
            if fused == "device":
                assert all(p.grad is None for p in f._all_params()[:12]) and f.basis_mat.weight.grad is not None
        if fused == "device":
            # the device copies the optimiser wrote (only the head is re-uploaded) are exactly what the nn.Parameters hold
            with torch.no_grad():
                own = f(rays, is_train=False, N_samples=40)
                fresh = make_field({k: v.detach().cpu().numpy() for k, v in f.state_dict().items()}, TINY["grid"], TINY["aabb"],
                                   TINY["near_far"])(rays, is_train=False, N_samples=40)
            assert torch.equal(own[0], fresh[0]) and torch.equal(own[1], fresh[1]) and torch.equal(own[3], fresh[3])
        return {k: v.detach().clone() for k, v in f.state_dict().items()}

    a = run(False)
    for b in (run(True), run("device")):
        for k in a:
            d = float((a[k] - b[k]).abs().max())
            # Adam normalises the step: an fp32 ulp of difference in a tiny gradient can move a parameter by a fraction of
            # lr in rare elements, so compare against the lr scale (0.02 spatial / 1e-3 network) rather than bitwise
            lr = 0.02 if ("plane" in k or "line" in k) else 1e-3
            frac = float(((a[k] - b[k]).abs() > 0.02 * lr).float().mean())
            assert d <= 2.5 * lr * 4 and frac < 1e-3, (k, d, frac)


def test_f1_device_side_step_survives_coarse_to_fine(tiny, tiny_params):
    """TVAdam(field=...) across an upsample_volume_grid (text2nerf_main.py:596-601 re-creates the optimiser after it): the
    native field, its gradient buffers and the device copies are rebuilt; the first step after the resize matches the
    reference-layout TVAdam from the same state."""
    from text2nerf_amd.optim import TVAdam
    rays = torch.from_numpy(tiny["tiny_rays"])
    tgt = torch.from_numpy(tiny["g6_train_rgb"]).to(dev()) * 0.5

    def step(f, opt, seed):
        torch.manual_seed(seed)
        rgb, depth, z, w = f(rays, is_train=True, white_bg=True, N_samples=40)
        loss = ((rgb - tgt) ** 2).mean() + 0.005 * (depth ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step(tv=[(f.density_plane, 0.1), (f.app_plane, 0.01)])
        return float(loss.detach())

    f = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    opt = TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f)
    for it in range(2):
        step(f, opt, 11 + it)
    new_grid = [int(g * 1.5) for g in TINY["grid"]]
    f.upsample_volume_grid(new_grid)
    state = {k: v.detach().cpu().numpy().copy() for k, v in f.state_dict().items()}
    opt = TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f)
    la = step(f, opt, 21)
    ref = make_field(state, new_grid, TINY["aabb"], TINY["near_far"])
    ropt = TVAdam(ref.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
    lb = step(ref, ropt, 21)
    assert abs(la - lb) <= 1e-6 * max(1.0, abs(lb))
    a, b = f.state_dict(), ref.state_dict()
    for k in a:
        lr = 0.02 if ("plane" in k or "line" in k) else 1e-3
        frac = float(((a[k] - b[k]).abs() > 0.02 * lr).float().mean())
        assert frac < 1e-3, (k, frac)
    step(f, opt, 22)   # and keeps going (head-only upload path)


def test_render_views_and_wide_ray_rows(tiny, field):
    """render_views (device-side rays per pose) equals rendering host-built rays; rays with extra channels use their
    LAST channel for the depth background term (models/tensorBase.py:505)."""
    from text2nerf_amd import render_views
    from oracle import oracle_torch as O
    poses = [synth.look_pose(0.35, -0.2, (0.4, -0.3, -1.0)), synth.look_pose(-0.2, 0.1, (0.0, 0.2, -0.5))]
    H, W = 12, 16
    rgb, depth = render_views(field, poses, [16.0, 16.0, 8, 6], H, W)
    assert rgb.shape == (2, H, W, 3) and depth.shape == (2, H, W)
    close(rgb[0].reshape(-1, 3), tiny["g6_eval_rgb"][:192], atol=RGB_ATOL)
    close(depth[0].reshape(-1), tiny["g6_eval_depth"][:192], atol=DEPTH_ATOL)
    rays8 = torch.cat([torch.from_numpy(tiny["tiny_rays"]), torch.full((200, 2), 3.25)], 1)
    cfg = O.FieldConfig(aabb=TINY["aabb"], grid_size=TINY["grid"], near_far=TINY["near_far"])
    P = O.params_from_numpy({k: v.detach().cpu().numpy() for k, v in field.state_dict().items()})
    o = O.forward(cfg, P, rays8)
    with torch.no_grad():
        g = field(rays8)
    close(g[1], o[1].numpy(), atol=DEPTH_ATOL)
    close(g[0], o[0].numpy(), atol=RGB_ATOL)


def test_g7a_alpha_mask_branch(tiny, tiny_params):
    """a-7: AlphaGridMask (models/tensorBase.py:41-59,451-456) — sample_alpha, forward eval/train with a mask, gradients with
    a mask vs the oracle, checkpoint round trip with the bit-packed volume."""
    import io
    from oracle import oracle_torch as O
    from text2nerf_amd import AlphaGridMask, TensorVMSplit
    f = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    f.alphaMask = AlphaGridMask(dev(), torch.from_numpy(tiny["g7a_aabb"]), torch.from_numpy(tiny["g7a_volume"]))
    rays = torch.from_numpy(tiny["tiny_rays"])
    with torch.no_grad():
        rgb, depth, z, w = f(rays)
    al = f.alphaMask.sample_alpha(torch.from_numpy(tiny["g7a_pts"]).to(dev()))
    close(al, tiny["g7a_alpha"], atol=1e-6)
    assert np.array_equal(al.cpu().numpy() > 0, tiny["g7a_alpha"] > 0)
    close(w, tiny["g7a_eval_w"], atol=W_ATOL, rtol=W_RTOL)
    close(rgb, tiny["g7a_eval_rgb"], atol=RGB_ATOL)
    close(depth, tiny["g7a_eval_depth"], atol=DEPTH_ATOL)
    torch.manual_seed(321)
    with torch.no_grad():
        rgb, depth, z, w = f(rays, is_train=True, N_samples=40)
    close(w, tiny["g7a_train_w"], atol=W_ATOL, rtol=W_RTOL)
    close(rgb, tiny["g7a_train_rgb"], atol=RGB_ATOL)
    # gradients through a masked field vs the oracle's autograd
    cfg = O.FieldConfig(aabb=TINY["aabb"], grid_size=TINY["grid"], near_far=TINY["near_far"],
                        alpha_volume=torch.from_numpy(tiny["g7a_volume"]), alpha_aabb=tiny["g7a_aabb"].tolist())
    P = O.params_from_numpy(tiny_params, requires_grad=True)
    torch.manual_seed(321)
    jit = torch.rand(rays.shape[0], 1)
    o = O.forward(cfg, P, rays, is_train=True, n_samples=40, jitter=jit)
    ((o[0] ** 2).sum() + (o[1] * 0.1).sum() + (o[3] ** 2).sum()).backward()
    torch.manual_seed(321)
    g = f(rays, is_train=True, N_samples=40)
    ((g[0] ** 2).sum() + (g[1] * 0.1).sum() + (g[3] ** 2).sum()).backward()
    _grad_check(f, {k: v.grad.numpy() for k, v in P.items()}, rel=2e-4)
    # checkpoint round trip (bit-packed mask, models/tensorBase.py:275-290)
    buf = io.BytesIO()
    f.save(buf)
    buf.seek(0)
    ck = torch.load(buf, weights_only=False)
    assert "alphaMask.mask" in ck and not any(k.startswith("alphaMask") for k in ck["state_dict"])
    f2 = TensorVMSplit(**{**ck["kwargs"], "device": dev()})
    f2.load(ck)
    with torch.no_grad():
        r2 = f2(rays)
        r1 = f(rays)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[3], r2[3])


def test_c1_config_128_grid_200x200_n64_whole_frame_vs_oracles():
    """BASELINE.json configs[0]: TensorVMSplit 128^3, 200x200 view, 64 samples/ray — the whole frame against the plain-C
    oracle, a subset against the PyTorch oracle (weights / z_vals too)."""
    from oracle import oracle_torch as O
    from oracle.oracle_c import COracle
    aabb = [[-8.0] * 3, [8.0] * 3]
    params = synth.make_field_params(3, [128] * 3, scene="S2", aabb=aabb)
    f = make_field(params, [128] * 3, aabb, [0.5, 8.0])
    assert f.nSamples == 220                                      # golden G9: update_stepSize at 128^3
    rays_np = synth.frame_rays_np(200, 200, c2w=synth.look_pose(0.2, -0.1, (0.3, 0.1, -0.5)))
    rays = torch.from_numpy(rays_np)
    with torch.no_grad():
        rgb, depth, z, w = f(rays, N_samples=64)
    cfg = O.FieldConfig(aabb=aabb, grid_size=[128] * 3)
    co = COracle(cfg, params)
    c_rgb, c_depth, c_z, c_w = co.render(rays_np, n_samples=64)
    assert f.stats()["evaluated"] == co.last_stats["evaluated"]
    close(rgb, c_rgb, atol=RGB_ATOL)
    close(depth, c_depth, atol=DEPTH_ATOL)
    close(z, c_z, atol=0)
    close(w, c_w, atol=W_ATOL, rtol=W_RTOL)
    sel = np.sort(np.random.Generator(np.random.PCG64(4)).choice(rays_np.shape[0], 3000, replace=False))
    o_rgb, o_depth, o_z, o_w = O.forward(cfg, O.params_from_numpy(params), rays[sel], n_samples=64)
    close(rgb[sel], o_rgb.numpy(), atol=RGB_ATOL)
    close(w[sel], o_w.numpy(), atol=W_ATOL, rtol=W_RTOL)
    assert f.stats()["appearance"] / rays_np.shape[0] > 2.0      # S2 (fog): a high appearance fraction


def test_c4_shape_1600x1600_eight_ray_tiles_equal_whole_frame():
    """BASELINE.json configs[3]: 1600x1600 render of the 300^3 scene split into 8 ray tiles (what 8 ranks render before the
    all-gather): the concatenated tiles are bitwise the single-launch frame; ragged tile sizes included."""
    from text2nerf_amd.parallel import shard_bounds
    aabb = [[-8.0] * 3, [8.0] * 3]
    f = make_field(synth.make_field_params(0, [300] * 3, scene="S1-soft", aabb=aabb), [300] * 3, aabb, [0.5, 8.0])
    f.materialize_weights = False
    from text2nerf_amd import generate_rays
    rays = generate_rays(1600, 1600, [1600.0, 1600.0, 800, 800], np.eye(4, dtype=np.float32), device=dev())
    R = rays.shape[0]
    assert R == 2560000
    with torch.no_grad():
        rgb, depth, _, _ = f(rays)
        whole_stats = f.stats()
        parts, ev = [], 0
        for r in range(8):
            lo, hi = shard_bounds(R - 3, 8, r)                    # ragged: the last three rays form a ninth sliver
            parts.append(f(rays[lo:hi]))
            ev += f.stats()["evaluated"]
        parts.append(f(rays[R - 3:]))
        ev += f.stats()["evaluated"]
    assert torch.equal(torch.cat([p[0] for p in parts]), rgb) and torch.equal(torch.cat([p[1] for p in parts]), depth)
    assert ev == whole_stats["evaluated"]


def test_eval_mode_gradients_black_background_vs_oracle(tiny, tiny_params):
    """Backward through an EVAL-mode render (z gate active, no jitter, white_bg=False: no background term) vs the oracle's
    autograd — the renderer's other differentiable configuration (render_warping_inapinting-style fine-tuning passes)."""
    from oracle import oracle_torch as O
    f = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    rays = torch.from_numpy(tiny["tiny_rays"])
    g = np.random.Generator(np.random.PCG64(12))
    ca = torch.from_numpy(g.uniform(-1, 1, (rays.shape[0], 3)).astype(np.float32))
    cb = torch.from_numpy(g.uniform(-1, 1, (rays.shape[0],)).astype(np.float32))
    out = f(rays, is_train=False, white_bg=False, N_samples=-1)
    ((out[0] * ca.to(dev())).sum() + (out[1] * cb.to(dev())).sum() + (out[3] ** 2).sum()).backward()
    cfg = O.FieldConfig(aabb=TINY["aabb"], grid_size=TINY["grid"], near_far=TINY["near_far"])
    P = O.params_from_numpy(tiny_params, requires_grad=True)
    o = O.forward(cfg, P, rays, white_bg=False, is_train=False)
    ((o[0] * ca).sum() + (o[1] * cb).sum() + (o[3] ** 2).sum()).backward()
    close(out[0], o[0].detach().numpy(), atol=RGB_ATOL)
    _grad_check(f, {k: v.grad.numpy() for k, v in P.items()}, rel=2e-4)


def test_c1_config_gradients_128_grid_vs_oracle():
    """BASELINE configs[0] shape (128^3, N=64): train-mode gradients of an MSE loss vs the oracle's autograd."""
    from oracle import oracle_torch as O
    aabb = [[-8.0] * 3, [8.0] * 3]
    params = synth.make_field_params(3, [128] * 3, scene="S2", aabb=aabb)
    f = make_field(params, [128] * 3, aabb, [0.5, 8.0])
    allr = synth.frame_rays_np(200, 200, c2w=synth.look_pose(0.2, -0.1, (0.3, 0.1, -0.5)))
    rng = np.random.Generator(np.random.PCG64(8))
    rays = torch.from_numpy(allr[np.sort(rng.choice(allr.shape[0], 1024, replace=False))])
    tgt = torch.from_numpy(rng.uniform(0, 1, (1024, 3)).astype(np.float32))
    torch.manual_seed(31)
    jit = torch.rand(1024, 1)
    torch.manual_seed(31)
    out = f(rays, is_train=True, white_bg=True, N_samples=64)
    (((out[0] - tgt.to(dev())) ** 2).mean() + 0.01 * out[1].mean()).backward()
    cfg = O.FieldConfig(aabb=aabb, grid_size=[128] * 3)
    P = O.params_from_numpy(params, requires_grad=True)
    o = O.forward(cfg, P, rays, white_bg=True, is_train=True, n_samples=64, jitter=jit)
    (((o[0] - tgt) ** 2).mean() + 0.01 * o[1].mean()).backward()
    _grad_check(f, {k: v.grad.numpy() for k, v in P.items()}, rel=5e-4)


def test_atomic_scatter_fallback_path_gradients():
    """The sliding-window global-atomic scatter (the backward's fallback when a grid's lines do not fit the LDS budget) stays
    correct: the G8 gradient check in a subprocess with T2N_BWD_ATOMIC_SCATTER=1 (the switch is read once per process)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import pytest\n"
            "sys.exit(pytest.main(['-q', '-x', '-m', 'gpu', '-k', 'test_g8_gradients_vs_reference_autograd or test_g7a_alpha_mask_branch', "
            "%r]))\n") % (root, os.path.join(root, "tests", "test_hip_parity.py"))
    env = dict(os.environ, T2N_BWD_ATOMIC_SCATTER="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-2000:]


def test_single_stream_backward_path_gradients():
    """The backward runs its density scatter on a side stream by default; T2N_BWD_SERIAL=1 keeps everything on the caller's stream.
    The G8 gradient check and the kept-rows variant in a subprocess under that switch (read once per process)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import pytest\n"
            "sys.exit(pytest.main(['-q', '-x', '-m', 'gpu', '-p', 'no:cacheprovider', '-k', "
            "'test_g8_gradients_vs_reference_autograd or test_g8_gradients_with_forward_kept_activation_rows', %r]))\n") % (
                root, os.path.join(root, "tests", "test_hip_parity.py"))
    env = dict(os.environ, T2N_BWD_SERIAL="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=600)
    assert r.returncode == 0 and "2 passed" in r.stdout, r.stdout[-2000:]


def test_tile_marcher_inline_compaction_overflow_rays():
    """Lazy-output eval frames compact the appearance list inside the tile marcher (<= N/4 staged entries per ray); rays with
    more appearance samples than that go through the overflow list (k_compact_list). A fog field with few samples per ray
    forces both: results equal the per-ray marcher's within the usual tolerances, sample counts exactly."""
    aabb = [[-8.0] * 3, [8.0] * 3]
    f = make_field(synth.make_field_params(1, [64] * 3, scene="S2", aabb=aabb), [64] * 3, aabb, [0.5, 8.0])
    f.materialize_weights = False
    rays = torch.from_numpy(synth.frame_rays_np(72, 88, c2w=synth.look_pose(0.1, 0.05, (0.2, -0.1, 2.0)))).to(dev())   # behind the z > 2 gate
    for n in (8, 40):                      # cap = 2 and 10 staged entries per ray
        with torch.no_grad():
            f.frame_width = 0
            a = f(rays, N_samples=n)
            sa = f.stats()
            f.materialize_weights = True
            w = f(rays, N_samples=n)[3]
            f.materialize_weights = False
            f.frame_width = 88
            b = f(rays, N_samples=n)
            sb = f.stats()
        per_ray = (w > 1e-4).sum(-1)
        if n == 8:
            assert int((per_ray > n // 4).sum()) > 50, "the scene must push rays over the staging capacity"
        assert sa["evaluated"] == sb["evaluated"] and abs(sa["appearance"] - sb["appearance"]) <= 3
        close(b[0], a[0].cpu().numpy(), atol=3e-5)
        close(b[1], a[1].cpu().numpy(), atol=1e-4)


def test_drop_in_evaluation_call_detects_the_raster(tiny_params):
    """OctreeRender_trilinear_fast in eval mode with all rays of one image and no frame_width hint (the reference's evaluation loop,
    renderer.py:85-89) detects the raster width and takes the tile marcher: bitwise the outputs of the explicit hint; shuffled rays
    keep the per-ray marcher (bitwise the outputs without any hint)."""
    from text2nerf_amd import OctreeRender_trilinear_fast
    f = make_field(tiny_params, TINY["grid"], TINY["aabb"], TINY["near_far"])
    rays = torch.from_numpy(synth.frame_rays_np(40, 56, c2w=synth.look_pose(0.3, -0.1, (0.2, 0.1, -1.0))))
    with torch.no_grad():
        auto = OctreeRender_trilinear_fast(rays, f, chunk=4096, N_samples=-1, white_bg=True, is_train=False, device=dev())
        assert f.frame_width == 0                    # the caller's setting is restored
        f.frame_width = 56
        hinted = f(rays, is_train=False, white_bg=True, N_samples=-1)
        f.frame_width = 0
        f.auto_frame_width = False
        plain = OctreeRender_trilinear_fast(rays, f, chunk=4096, N_samples=-1, white_bg=True, is_train=False, device=dev())
        f.auto_frame_width = True
        perm = torch.randperm(rays.shape[0], generator=torch.Generator().manual_seed(3))
        shuffled = OctreeRender_trilinear_fast(rays[perm], f, chunk=4096, N_samples=-1, white_bg=True, is_train=False, device=dev())
    assert torch.equal(auto[0], hinted[0]) and torch.equal(auto[2], hinted[1]) and torch.equal(auto[3], hinted[3])
    assert torch.equal(shuffled[0], plain[0][perm.to(plain[0].device)])
    close(auto[0], plain[0].cpu().numpy(), atol=RGB_ATOL)
