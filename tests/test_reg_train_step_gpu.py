"""The L1 and ortho regularisers (models/tensoRF.py:173-191) on every route of the training step: train_step(..., l1=..., ortho=...)
fused and fused-indexed (hyper[21..24] of t2n_train_step), composed with the seeded gradient buffer (t2n_field_reg_seed) and without
(t2n_field_reg_adam_step), speculative, a general-shape field with optim.TVAdam (reference-layout kernels), and the autograd loop with
density_L1() / vector_comp_diffs() in the loss.

Method (tests/test_optim_kernels_gpu.py's for the TV seed): fresh fields from the same parameters take the same step on the same rays
behind the same generator seed: once without the keywords, twice with the new weights zero, then with the L1 weights set, with the ortho
weights set, and with all four set. The gradient Adam consumed is read out of its first moment (tests/helpers/adam_readout.py), or is
`.grad` itself where the route leaves one. The data gradient does not depend on the weights, so g_w - g_0a is the regulariser gradient
t (tests/helpers/reg_ref.py, float64; t = 0 on a tensor the run's weights do not reach, which is asserted like any other).

Tolerance per element e of a tensor:
    4 * 2^-24 (|g_w| + |g_0a|)  +  noise  +  K * 2^-24 * (|t_e| + 2 M)
* 4 * 2^-24 (...): the readout of two float32 moments and the roundings of the term itself.
* noise: the largest difference of the tensor between any two of the three runs WITHOUT weights (the keyword-free one and the two with
  zero weights are the same step): the run-to-run difference of the scatters' float32 atomics, existing code. No other run enters it.
* K * 2^-24 * (|t_e| + 2 M): the float32 additions that build the element. The scatters add up to K = rays x samples contributions
  d_i to it (a sample reaches an element at most once), each addition rounding by at most 2^-24 of its partial sum. On the seeded
  routes the buffer STARTS as the term, so the partial sums of the run with weights are bounded by |t_e| + sum |d_i|, those of the run
  without by sum |d_i|; in any order of the atomics. sum |d_i| is not observable from outside: M, the tensor's largest |g_0a|, stands
  in for it. The two sums differ by up to K 2^-24 (|t_e| + 2 sum |d_i|) whatever the code under test does: three weight-free runs do not
  sample this (most pairs are bit-equal, then one differs in elements whose contributions cancel), and a tensor no weight reaches can
  differ between two runs by ten times 4 * 2^-24 (|g_w| + |g_0a|). With K = 20 480 the allowance is 1.2e-3 (|t_e| + 2 M): a term that
  is lost, doubled, mis-scaled by a normaliser (C^2 for C (C - 1): 2 % at 48 components) or leaked into a tensor it must not reach
  (|t| ~ M) is far outside it; the arithmetic of the terms to the last bit is held by tests/test_reg_kernels_gpu.py.
A term must exceed ten times its tolerance (asserted). The figures are printed ("reg_terms:" lines) and, with T2N_REG_TERMS_OUT=FILE
in the environment, appended to FILE: profiles/reg_terms.txt is one such run.

Weights: L1 30 on the density planes (30 / numel = 4.3e-3 per element on the 23 x 19 plane) and 1 on the density lines (3.7e-3), ortho
0.1 on the density lines (~1e-2) and 0.01 on the appearance lines (~3.5e-5), against data gradients of ~4e-3 (density) and ~2e-5
(appearance): every term is one to three times the data gradient, neither lost beside it nor drowning it."""
import os

import numpy as np
import pytest
import torch

from text2nerf_amd import synth
from text2nerf_amd._lib import T2NError
from tests.conftest import TINY
from tests.helpers import adam_readout as A
from tests.helpers import reg_ref as R
from tests.test_hip_parity import dev, make_field

pytestmark = pytest.mark.gpu

B1 = A.F32_BETAS[0]
U = 2.0 ** -24
W_L1_PLANE, W_L1_LINE, W_ORTHO_DEN, W_ORTHO_APP = 30.0, 1.0, 0.1, 0.01
RUNS = ((None, None), ("0a", False), ("0b", False), ("l1", "l1"), ("ortho", "ortho"), ("all", "all"))
GRIDS = {"23x19x17": [23, 19, 17], "64x65x5": [64, 65, 5]}      # 64 x 65 x 5: a line of exactly one 64-position block, one of a block + 1
N_RAYS, N_SAMPLES = 512, 40
FIELD_ROUTES = ["fused", "fused-indexed", "composed-seeded", "composed", "speculative", "autograd"]


def batch():
    g = np.random.Generator(np.random.PCG64(3))
    rays = torch.from_numpy(synth.frame_rays_np(16, 32, c2w=synth.look_pose(0.3, -0.1, (0.2, 0.1, -1.0))))
    assert rays.shape[0] == N_RAYS
    return rays, torch.from_numpy(g.uniform(0, 1, (N_RAYS, 3)).astype(np.float32)), torch.from_numpy(g.uniform(2, 7, (N_RAYS,)).astype(np.float32))


def terms(f, on):
    """(l1, ortho) lists: None = call without the keywords, False = the keywords with zero weights, "l1" / "ortho" / "all" = the weights of
    this file for that term (the other term's keyword present with zero weights)."""
    if on is None:
        return {}
    a, b = switches(on)
    return dict(l1=[(f.density_plane, a * W_L1_PLANE), (f.density_line, a * W_L1_LINE)],
                ortho=[(f.density_line, b * W_ORTHO_DEN), (f.app_line, b * W_ORTHO_APP)])


def switches(on):
    return (1.0 if on in ("l1", "all") else 0.0), (1.0 if on in ("ortho", "all") else 0.0)


def expected(params):
    """The two regulariser gradients (L1, ortho) of every factor tensor (float64, reference layout) at float32 parameters
    `params` {name: array}."""
    out = {}
    for k, p in params.items():
        p32 = np.asarray(p, np.float32)
        l1, ortho = np.zeros(p32.shape, np.float64), np.zeros(p32.shape, np.float64)
        if k.startswith("density_plane"):
            l1 = R.l1_grad(p32, W_L1_PLANE)
        if k.startswith("density_line"):
            l1, ortho = R.l1_grad(p32, W_L1_LINE), R.ortho_grad(p32, W_ORTHO_DEN).reshape(p32.shape)
        if k.startswith("app_line"):
            ortho = R.ortho_grad(p32, W_ORTHO_APP).reshape(p32.shape)
        out[k] = (l1, ortho)
    return out


def autograd_step(f, rays, rgb_t, dep_t, on):
    """text2nerf_main.py:547-590 as an autograd loop, the two terms in the loss as the reference's driver adds them."""
    from text2nerf_amd import OctreeRender_trilinear_fast
    from tests.test_train_step import torch_loss
    d = dev()
    rgb, _, depth, w, z = OctreeRender_trilinear_fast(rays, f, chunk=rays.shape[0], N_samples=N_SAMPLES, white_bg=True, is_train=True, device=d)
    mse, dl, tl, tot = torch_loss(rgb, depth, w, z, rgb_t.to(d), dep_t.to(d))
    if on is not None:
        s, t = switches(on)
        # (density_L1 carries ONE weight in the reference's driver: planes and lines are weighted separately here through two calls'
        # worth of terms, so that the expectation above is the same on every route)
        from text2nerf_amd.losses import l1_terms, ortho_terms
        tot = tot + s * W_L1_PLANE * l1_terms(list(f.density_plane)) + s * W_L1_LINE * l1_terms(list(f.density_line)) \
            + t * W_ORTHO_DEN * ortho_terms(list(f.density_line)) + t * W_ORTHO_APP * ortho_terms(list(f.app_line))
    f.zero_grad()
    tot.backward()
    return torch.stack([mse, dl, tl, tot]).detach()


def one_run(route, params, grid, on, monkeypatch, warm=0):
    """A fresh field, `warm` steps without the keywords, then the measured step: (gradients by name, parameters before the step,
    parameters after it, the step's loss tensor)."""
    from text2nerf_amd import tensorf as tf
    from text2nerf_amd.optim import TVAdam
    rays, rgb_t, dep_t = batch()
    f = make_field(params, grid, TINY["aabb"], TINY["near_far"])
    names = [k for k, _ in A.kernel_named(f)]
    if route == "autograd":
        torch.manual_seed(77)
        before = {k: p.detach().cpu().numpy().copy() for k, p in A.kernel_named(f)}
        losses = autograd_step(f, rays, rgb_t, dep_t, on)
        grads = {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in A.kernel_named(f)}
        return grads, before, before, losses.cpu().numpy()
    monkeypatch.setattr(tf, "_SEED_MIN_RAYS", 0 if route == "composed-seeded" else 1 << 30)
    opt = TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f)
    kw = dict(N_samples=N_SAMPLES, white_bg=True)
    kw.update({"fused": dict(fused=True, graph=False), "fused-indexed": dict(fused=True, graph=False), "composed-seeded": dict(fused=False),
               "composed": dict(fused=False), "speculative": dict(fused=False, speculative=True)}[route])

    def step(extra):
        torch.manual_seed(77)
        if route == "fused-indexed":
            from text2nerf_amd.dataset import DeviceTrainSet
            src = DeviceTrainSet(rays, rgb_t, dep_t, device=dev())
            out = f.train_step_indexed(src, torch.arange(N_RAYS, dtype=torch.int64), opt, **kw, **extra)
        else:
            out = f.train_step(rays, rgb_t, dep_t, opt, **kw, **extra)
        if route.startswith("fused"):
            f._fused_step.sync()          # (a step whose rows did not fit has been replayed: the step count below is that of applied steps)
        return out.clone()

    for _ in range(warm):
        step({})
    torch.cuda.synchronize()
    prev = A.snapshot(f, opt)
    losses = step(terms(f, on))
    torch.cuda.synchronize()
    cur = A.snapshot(f, opt)
    assert all(cur["step"][k] == warm + 1 for k in names), cur["step"]
    assert f.last_depth_aux is None
    grads = {k: A.recover_grad(prev["m"][k], cur["m"][k], A.one_minus(B1)) for k in names}
    return grads, prev["p"], cur["p"], losses.cpu().numpy()


def noise_of(*samples):
    """The largest difference of one tensor's gradient between any two weight-free runs of the same step."""
    return max(float(np.abs(a - b).max()) for i, a in enumerate(samples) for b in samples[i + 1:])


def report(line):
    print(line)
    out = os.environ.get("T2N_REG_TERMS_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def tolerance(gw, g0a, noise, ref, adds):
    """The module docstring's bound and its first two terms alone (the latter is reported, not asserted)."""
    plain = 4 * U * (np.abs(gw) + np.abs(g0a)) + noise
    return plain + adds * U * (np.abs(ref) + 2 * float(np.abs(g0a).max())), plain


def check_route(route, runs, what, adds=N_RAYS * N_SAMPLES):
    """runs: {None, '0a', '0b', 'l1', 'ortho', 'all'} -> (grads, p_before, p_after, losses). `adds`: rays x samples of the batch."""
    g_none, g0a, g0b = (runs[k][0] for k in (None, "0a", "0b"))
    failures = []
    for k in g0a:
        report(f"reg_terms: {what} {route} {k}: noise of three weight-free runs {noise_of(g0a[k], g0b[k], g_none[k]):.3e}, "
               f"max |data g| {float(np.abs(g0a[k]).max()):.3e}")
    for tag in ("l1", "ortho", "all"):
        gw = runs[tag][0]
        want = expected({k: v for k, v in runs[tag][1].items() if "plane" in k or "line" in k})
        a, b = switches(tag)
        worst = {True: (0.0, 0.0, ""), False: (0.0, 0.0, "")}
        for k in gw:
            noise = noise_of(g0a[k], g0b[k], g_none[k])
            e_l1, e_or = want.get(k, (np.zeros_like(gw[k]), np.zeros_like(gw[k])))
            ref = a * e_l1 + b * e_or
            tol, plain = tolerance(gw[k], g0a[k], noise, ref, adds)
            err = np.abs((gw[k] - g0a[k]) - ref)
            has = float(np.abs(ref).max()) > 0
            r, rp = float((err / tol).max()), float((err / np.maximum(plain, 1e-300)).max())
            if r >= worst[has][0]:
                worst[has] = (r, rp, k)
            if ("plane" in k or "line" in k) and not float(np.abs(g0a[k]).max()) > 0:
                failures.append((tag, k, "the rays did not reach this tensor"))
            if has and not float(np.abs(ref).max()) > 10 * float(tol.max()):
                failures.append((tag, k, "the term is lost in the tolerance"))
            if not np.all(err <= tol):
                failures.append((tag, k, "regulariser gradient" if has else "a tensor the weights do not reach moved", r))
        report(f"reg_terms: {what} {route} [{tag}]: worst error / tolerance {worst[True][0]:.4f} ({worst[True][2]}; {worst[True][1]:.2f} of the "
               f"first two terms alone) on tensors with a term, {worst[False][0]:.4f} ({worst[False][2]}; {worst[False][1]:.2f}) on tensors without")
        # the returned losses carry no regulariser (like TV): they come from the forward alone
        if route != "autograd" and not np.allclose(runs["0a"][3], runs[tag][3], rtol=1e-6, atol=0):
            failures.append((tag, "losses changed with the weights", runs["0a"][3].tolist(), runs[tag][3].tolist()))
    assert not failures, failures


@pytest.mark.parametrize("grid", list(GRIDS), ids=list(GRIDS))
@pytest.mark.parametrize("route", FIELD_ROUTES)
def test_regulariser_gradient_on_every_route(route, grid, monkeypatch):
    params = synth.make_field_params(31, GRIDS[grid], density_scale=0.9, aabb=TINY["aabb"])
    warm = 1 if route == "speculative" else 0          # (the first speculative step takes the counted route: measure the second)
    runs = {tag: one_run(route, params, GRIDS[grid], on, monkeypatch, warm) for tag, on in RUNS}
    check_route(route, runs, grid)


SPIED = ("t2n_train_step", "t2n_field_tv_seed", "t2n_field_tv_adam_step", "t2n_field_reg_seed", "t2n_field_reg_adam_step",
         "t2n_l1_grad_add", "t2n_ortho_grad_add")


def record_calls(mp, log):
    """Every C entry point of the optimiser side a step goes through, with its scalar arguments (t2n_train_step: flags and phases), and
    the hyper block the fused step stages."""
    from text2nerf_amd import _lib, trainer
    lib = _lib.load()
    for name in SPIED:
        def spy(*a, _n=name, _o=getattr(lib, name)):
            if _n == "t2n_train_step":
                log.append((_n, int(a[1]._obj.flags), int(a[1]._obj.phases)))
            else:
                log.append((_n,) + tuple(x for x in a if isinstance(x, float)))
            return _o(*a)
        mp.setattr(lib, name, spy)
    orig = trainer.FusedStep._hyper

    def hyper(self, *a, **k):
        out = orig(self, *a, **k)
        log.append(("hyper", tuple(out[0]), int(self._reg_flags)))
        return out
    mp.setattr(trainer.FusedStep, "_hyper", hyper)


@pytest.mark.parametrize("route", ["fused", "fused-indexed", "composed-seeded", "composed", "speculative"])
def test_zero_weights_are_the_keyword_free_step(route, monkeypatch):
    """The step with the new weights zero IS the step without the keywords: the same C entry points with the same scalar arguments —
    t2n_field_tv_seed / t2n_field_tv_adam_step, never the reg_ forms — the same flags on t2n_train_step and the same hyper block, so the
    updated parameters are those of the keyword-free step to the bit wherever the device's own arithmetic is (the scatters' atomics are
    not: that is why this is asserted on the calls). With the weights set the log differs (the check can fail)."""
    grid = GRIDS["23x19x17"]
    params = synth.make_field_params(31, grid, density_scale=0.9, aabb=TINY["aabb"])
    logs = {}
    for tag, on in ((None, None), ("0", False), ("all", "all")):
        with monkeypatch.context() as mp:
            log = []
            record_calls(mp, log)
            one_run(route, params, grid, on, mp, 1 if route == "speculative" else 0)
            logs[tag] = log
    assert logs[None] and logs[None] == logs["0"], (logs[None], logs["0"])
    assert not any("reg" in c[0] for c in logs["0"]) and not any(c[0] == "t2n_train_step" and c[1] & 0x300 for c in logs["0"])
    assert all(h[1][21:25] == (0.0,) * 4 and h[2] == 0 for h in logs["0"] if h[0] == "hyper")
    assert logs["all"] != logs[None]
    if route.startswith("fused"):
        assert any(c[0] == "t2n_train_step" and c[1] & 0x300 == 0x300 for c in logs["all"])
        assert [h[1][21:25] for h in logs["all"] if h[0] == "hyper"][-1] == (W_L1_PLANE, W_L1_LINE, W_ORTHO_DEN, W_ORTHO_APP)
    else:
        assert any(c[0] in ("t2n_field_reg_seed", "t2n_field_reg_adam_step") for c in logs["all"])


def test_regulariser_gradient_general_shape_with_tvadam(monkeypatch):
    """A general-shape field ([33,17,18] / [50,49,51] components): the composed route leaves `.grad` in the reference layouts and
    TVAdam (without field=) adds the terms to it through the reference-layout kernels: `.grad` after the step is data + terms."""
    from text2nerf_amd.optim import TVAdam
    from tests.helpers import generic_cases as G
    from tests.helpers import generic_train as T
    from tests.test_generic_fuzz import _supply_draws
    case, params, vol = T.case_inputs("odd_rows")
    N, jit, add_bg = G.draws(case, True)
    rgb_t, dep_t = T.targets(case)

    def run(on, optimizer=None):
        m = G.make_field(case, params, dev(), vol)
        assert m._is_general()
        opt = optimizer(m) if optimizer else TVAdam(m.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99))
        before = {k: p.detach().cpu().numpy().copy() for k, p in m.named_parameters()}
        with monkeypatch.context() as mp:
            _supply_draws(mp, jit, add_bg)
            losses = m.train_step(torch.from_numpy(case.rays), rgb_t, dep_t, opt, N_samples=N, white_bg=case.white_train, **terms(m, on)).clone()
        grads = {k: p.grad.detach().cpu().numpy().astype(np.float64) for k, p in m.named_parameters()}
        after = {k: p.detach().cpu().numpy().copy() for k, p in m.named_parameters()}
        return grads, before, after, losses.cpu().numpy()

    runs = {tag: run(on) for tag, on in RUNS}
    check_route("general", runs, "odd_rows", adds=case.R * N)
    with pytest.raises(T2NError):
        run("all", optimizer=lambda m: torch.optim.Adam(m.parameters(), lr=1e-3))


@pytest.mark.parametrize("route", ["fused", "composed-seeded"])
def test_a_weight_changed_between_two_steps_takes_effect(route, monkeypatch):
    """An L1 schedule switches weights mid-run (L1_weight_inital -> L1_weight_rest): two fields take the same first step (TV only; the
    seeded route writes the NEXT step's seed ahead, keyed by its weights), then one takes a second step like the first and the other a
    second step with the new weights set. Their second gradients differ by the regulariser gradient at the parameters after step one:
    a seed taken under a stale key would make them equal."""
    from text2nerf_amd import tensorf as tf
    from text2nerf_amd.optim import TVAdam
    monkeypatch.setattr(tf, "_SEED_MIN_RAYS", 0)
    grid = GRIDS["23x19x17"]
    params = synth.make_field_params(31, grid, density_scale=0.9, aabb=TINY["aabb"])
    rays, rgb_t, dep_t = batch()
    kw = dict(N_samples=N_SAMPLES, white_bg=True, **(dict(fused=True, graph=False) if route == "fused" else dict(fused=False)))

    def two_steps(on):
        f = make_field(params, grid, TINY["aabb"], TINY["near_far"])
        opt = TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f)
        tv = [(f.density_plane, 0.1), (f.app_plane, 0.01)]
        snaps = []
        for it, extra in enumerate(({}, terms(f, on))):
            torch.manual_seed(90 + it)
            f.train_step(rays, rgb_t, dep_t, opt, tv=tv, **kw, **extra)
            if route == "fused":
                f._fused_step.sync()
            torch.cuda.synchronize()
            snaps.append(A.snapshot(f, opt))
        g2 = {k: A.recover_grad(snaps[0]["m"][k], snaps[1]["m"][k], A.one_minus(B1)) for k in snaps[0]["m"]}
        return g2, snaps[0]["p"]

    g0a, p1 = two_steps(False)
    g0b, _ = two_steps(False)
    g0c, _ = two_steps(None)
    failures = []
    for tag in ("l1", "ortho"):
        gw, p1w = two_steps(tag)
        a, b = switches(tag)
        want = expected({k: v for k, v in p1w.items() if "plane" in k or "line" in k})
        for k in gw:
            e_l1, e_or = want.get(k, (np.zeros_like(gw[k]), np.zeros_like(gw[k])))
            ref = a * e_l1 + b * e_or
            tol, _ = tolerance(gw[k], g0a[k], noise_of(g0a[k], g0b[k], g0c[k]), ref, N_RAYS * N_SAMPLES)
            err = np.abs((gw[k] - g0a[k]) - ref)
            if float(np.abs(ref).max()) > 0 and not float(np.abs(ref).max()) > 10 * float(tol.max()):
                failures.append((tag, k, "the term is lost in the tolerance"))
            if not np.all(err <= tol):
                failures.append((tag, k, float((err / tol).max())))
    assert not failures, failures


def test_routes_that_do_not_carry_the_terms_refuse_them(monkeypatch):
    from text2nerf_amd.optim import TVAdam
    grid = GRIDS["23x19x17"]
    params = synth.make_field_params(31, grid, density_scale=0.9, aabb=TINY["aabb"])
    rays, rgb_t, dep_t = batch()
    f = make_field(params, grid, TINY["aabb"], TINY["near_far"])
    opt = TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f)
    before = {k: v.detach().clone() for k, v in f.state_dict().items()}
    on = terms(f, "all")

    class Sharded:          # what train_step recognises a parallel.ShardedExchange by
        world, rank = 2, 0

        def reduce(self, fs):
            raise AssertionError("the exchange must not start")

        def gather(self, fs):
            raise AssertionError("the exchange must not start")

    for kw in (dict(graph=True), dict(all_reduce=Sharded())):
        for one in (dict(l1=on["l1"]), dict(ortho=on["ortho"])):
            with pytest.raises(T2NError):
                f.train_step(rays, rgb_t, dep_t, opt, N_samples=N_SAMPLES, white_bg=True, **kw, **one)
    with pytest.raises(T2NError):      # an optimiser that would drop the terms
        f.train_step(rays, rgb_t, dep_t, torch.optim.Adam(f.parameters(), lr=1e-3), N_samples=N_SAMPLES, white_bg=True, fused=False, **on)
    with pytest.raises(T2NError):      # entries other than the field's own lists, as for tv
        f.train_step(rays, rgb_t, dep_t, opt, N_samples=N_SAMPLES, white_bg=True, l1=[(f.app_plane, 1.0)])
    with pytest.raises(T2NError):
        opt.step(ortho=[(f.density_plane, 1.0)])
    # zero weights pass everywhere: graph=True with the keywords present but nothing to apply
    torch.cuda.synchronize()
    for k, v in f.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert not opt.state or all(int(s.get("step", 0)) == 0 for s in opt.state.values())
    f.train_step(rays, rgb_t, dep_t, opt, N_samples=N_SAMPLES, white_bg=True, graph=True, **terms(f, False))
    f._fused_step.sync()
    # the C entry points refuse on their own: a captured step and a sharded step with the flags set
    import ctypes as C
    from text2nerf_amd import _lib
    fs = f._fused_step
    a, _ = fs._args_of(0, dict(fs.slots[0]["meta"]), 3, fs.slots[0]["cap"])
    flags0 = int(a.flags)
    try:
        a.flags = flags0 | _lib.FLAG_REG_L1
        h = C.c_void_p()
        with torch.cuda.device(dev()):
            st = _lib.current_stream_ptr(dev())
            assert _lib.load().t2n_train_graph_capture(f._handle, C.byref(a), st, C.byref(h)) == -2 and not h.value
            a.flags = flags0 | _lib.FLAG_REG_ORTHO
            a.phases, a.shard_world, a.shard_rank = 1, 2, 0
            assert _lib.load().t2n_train_step(f._handle, C.byref(a), st) == -2
            assert b"sharded" in _lib.load().t2n_last_error()
    finally:
        a.flags, a.phases, a.shard_world, a.shard_rank = flags0, 3, 0, 0


def test_depth_aux_and_losses_do_not_see_the_terms(monkeypatch):
    """A depth term other than "mse" on the composed route: `last_depth_aux` and the loss tensor are those of the step without weights."""
    from text2nerf_amd.optim import TVAdam
    grid = GRIDS["23x19x17"]
    params = synth.make_field_params(31, grid, density_scale=0.9, aabb=TINY["aabb"])
    rays, rgb_t, dep_t = batch()
    out = []
    for on in (False, "all"):
        f = make_field(params, grid, TINY["aabb"], TINY["near_far"])
        opt = TVAdam(f.get_optparam_groups(0.02, 1e-3), betas=(0.9, 0.99), field=f)
        torch.manual_seed(77)
        losses = f.train_step(rays, rgb_t, dep_t, opt, N_samples=N_SAMPLES, white_bg=True, depth_loss="si_log", **terms(f, on)).clone()
        assert f.last_depth_aux is not None
        out.append((losses.cpu().numpy(), f.last_depth_aux.cpu().numpy().copy()))
    # (two runs of the same forward and loss kernels: equal to the float32 rounding of their sums at the very most)
    assert np.allclose(out[0][0], out[1][0], rtol=1e-6, atol=0) and np.allclose(out[0][1], out[1][1], rtol=1e-6, atol=0), out


def test_logging_values_are_kernel_backed_and_match_float64():
    """density_L1() / vector_comp_diffs() on a device field: float32 device scalars from the kernels, equal to the float64 sums to float32
    rounding; their backward is the regulariser gradient."""
    grid = GRIDS["23x19x17"]
    params = synth.make_field_params(31, grid, density_scale=0.9, aabb=TINY["aabb"])
    f = make_field(params, grid, TINY["aabb"], TINY["near_far"])
    with torch.no_grad():
        l1, ortho = f.density_L1(), f.vector_comp_diffs()
    assert l1.is_cuda and l1.dtype == torch.float32 and ortho.is_cuda and ortho.dtype == torch.float32
    want_l1 = R.l1_value([params[f"density_{kind}.{k}"] for k in range(3) for kind in ("plane", "line")])
    want_o = sum(R.ortho_value(params[f"{grp}_line.{k}"]) for grp in ("density", "app") for k in range(3))
    assert abs(float(l1) - want_l1) <= 1.01 * U * want_l1 and abs(float(ortho) - want_o) <= 1.01 * U * want_o, (float(l1), want_l1, float(ortho), want_o)
    f.zero_grad()
    (f.density_L1() * 2.0 + f.vector_comp_diffs() * 3.0).backward()
    for k in range(3):
        p = params[f"density_line.{k}"]
        ref = R.l1_grad(p, 2.0) + R.ortho_grad(p, 3.0).reshape(p.shape)
        got = f.density_line[k].grad.cpu().numpy().astype(np.float64)
        tol = R.ortho_grad_tolerance(p, 3.0).reshape(p.shape) + 2 * U * np.abs(ref) + U * np.abs(R.l1_grad(p, 2.0))
        assert np.all(np.abs(got - ref) <= tol), k
        assert not R.check_l1_set(f.density_plane[k].grad.cpu().numpy(), params[f"density_plane.{k}"], 1.0, 2.0), k
