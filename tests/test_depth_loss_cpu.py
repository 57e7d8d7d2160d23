"""The depth losses without a GPU: the float64 helper (tests/helpers/depth_loss_ref.py) against the reference's own functions
(tests/golden/depth_loss.npz: upstream run on float64 tensors under autograd, tests/golden/make_golden_depth_loss.py), the public
functions' signatures against the reference's, the guarantees of the case builder that let float32 kernels and the float64 helper
agree about every branch, and the C entry points' argument checks (made before any launch)."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import depth_loss_ref as D

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = D.all_cases()


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "depth_loss.npz")))


def close(got, want, what, rel=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    scale = float(np.abs(want).max()) if want.size else 0.0
    err = float(np.abs(got - want).max()) if want.size else 0.0
    assert err <= rel * scale + 1e-300, (what, err, scale)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_helper_equals_the_reference_run_in_float64(cid, gold):
    c = CASES[cid]
    y = c["depth_t"]
    ran = 0
    if f"{cid}/gnll_loss" in gold:
        o = D.gnll(c["depth_fin"], c["w"], c["z"], y, D.SIGMA)
        close(o["loss"], gold[f"{cid}/gnll_loss"], "gnll loss")
        close(o["d_depth"], gold[f"{cid}/gnll_d_depth"], "gnll d_depth")
        close(o["d_w"], gold[f"{cid}/gnll_d_w"], "gnll d_w")
        assert np.array_equal(o["apply"], gold[f"{cid}/gnll_apply"])
        assert tuple(gold[f"{cid}/gnll_shape"]) == ((1,) if o["K"] == 0 else ())        # the (1,) zero of "no ray selected"
        ran += 1
    if f"{cid}/si_loss" in gold:
        o = D.si_log(c["depth_fin"], y)
        close(o["loss"], gold[f"{cid}/si_loss"], "si_log loss")
        close(o["d_depth"], gold[f"{cid}/si_d_depth"], "si_log d_depth")
        ran += 1
    if f"{cid}/ssi_loss" in gold:
        o = D.ssi(c["w"], c["z"], y)
        print(f"{cid}: kappa {o['kappa']:.3e} deficient {o['deficient']} s {o['s']:.6g} t {o['t']:.6g}")
        close(o["loss"], gold[f"{cid}/ssi_loss"], "ssi loss")
        close([o["s"], o["t"]], gold[f"{cid}/ssi_st"], "ssi s, t")
        close(o["d_w"], gold[f"{cid}/ssi_d_w"], "ssi d_w")
        ran += 1
    assert ran


@pytest.mark.parametrize("cid", sorted(CASES))
def test_case_builder_keeps_every_branch_margin(cid):
    c = CASES[cid]
    R, N = c["w"].shape
    z = c["z"].astype(np.float64)
    assert np.all(np.diff(z, axis=1) >= 0) and z.min() >= 0.5 and z.max() <= 8.0 + 1e-6
    assert c["w"].min() >= 0 and all(a.dtype == np.float32 for a in c.values() if isinstance(a, np.ndarray))
    assert int(np.isnan(c["depth"]).sum()) == (1 if R >= 5 and cid.startswith(("rand-", "narrow-", "ssi-")) else 0)
    assert not np.isnan(c["depth_fin"]).any()
    m = D.margins(c)
    print(cid, {k: f"{v:.3g}" for k, v in m.items()})
    checked = {"rand": ("mean", "var_sigma", "var_clamp", "si", "mask"), "narrow": ("mean", "var_sigma", "var_clamp", "si", "mask"),
               "directed": ("mean", "var_sigma", "var_clamp", "mask"), "ssi": ("mask",)}[cid.split("-")[0]]
    for k in checked:
        assert m[k] >= D.MARGIN_FLOORS[k], (cid, k, m[k])


def test_directed_rays_are_what_they_claim():
    for name, classes in D.DIRECTED.items():
        c = D.directed_case(name)
        o = D.gnll(c["depth_fin"], c["w"], c["z"], c["depth_t"], D.SIGMA)
        e = np.abs(c["depth_fin"].astype(np.float64) - c["depth_t"])
        for r, k in enumerate(classes):
            by_mean, by_var = e[r] - D.SIGMA > 0, D.SIGMA ** 2 < o["var"][r]
            assert (by_mean, by_var) == {"n": (False, False), "m": (True, False), "v": (False, True), "a": (True, True)}[k], (name, r)
            if k == "n":
                assert e[r] <= 0.1 and o["var"][r] <= 0.01
            if k == "m":
                assert o["var"][r] == 1e-8 and o["v"][r] == 1e-3
        assert o["K"] == sum(k != "n" for k in classes)
    assert D.gnll(*[D.directed_case("k0")[k] for k in ("depth_fin", "w", "z", "depth_t")], D.SIGMA)["K"] == 0
    assert D.gnll(*[D.directed_case("k1")[k] for k in ("depth_fin", "w", "z", "depth_t")], D.SIGMA)["K"] == 1
    o = D.gnll(*[D.directed_case("mixed")[k] for k in ("depth_fin", "w", "z", "depth_t")], D.SIGMA)
    assert 0 < o["K"] < len(D.DIRECTED["mixed"])


def test_ssi_cases_cover_the_conditioning_and_the_rank_deficient_rule():
    for R, N in D.SHAPES:
        c = D.random_case(R, N, narrow=True)
        o = D.ssi(c["w"], c["z"], c["depth_t"])
        print(f"narrow-{R}x{N}: kappa {o['kappa']:.3e}")
        assert o["kappa"] >= 1e3
    for cid, c in CASES.items():
        if cid.startswith("directed-"):
            continue
        o = D.ssi(c["w"], c["z"], c["depth_t"])
        want_deficient = cid in ("ssi-zero-w", "ssi-equal-z") or c["w"].shape[1] == 1
        assert o["deficient"] == want_deficient, cid
        if o["deficient"]:      # the closed form of the pseudo-inverse, as the kernels evaluate it
            assert abs(o["closed"][0] - o["s"]) <= 1e-12 * max(abs(o["s"]), 1e-300) + 1e-300, cid
            assert abs(o["closed"][1] - o["t"]) <= 1e-12 * max(abs(o["t"]), 1e-300) + 1e-300, cid
    a = D.ssi(*[CASES["ssi-affine"][k] for k in ("w", "z", "depth_t")])
    assert abs(a["s"] - 0.5) <= 1e-12 and abs(a["t"] - 1.5) <= 1e-12 and a["loss"] <= 1e-28      # the perfect fit
    z = D.ssi(*[CASES["ssi-zero-w"][k] for k in ("w", "z", "depth_t")])
    assert z["s"] == 0.0 and z["t"] == 0.0 and z["loss"] == 0.0


def test_driver_loss_ex_is_driver_loss_with_the_term_swapped():
    from tests.helpers import optim_ref
    c = CASES["rand-6x65"]
    a = (c["rgb"], c["depth"], c["w"], c["z"], c["rgb_t"], c["depth_t"], 0.005, 1e3, D.DELTA)
    base = optim_ref.driver_loss(*a)
    same = D.driver_loss_ex("mse", *a)
    assert all(np.array_equal(x, y) for x, y in zip(base, same[:4]))
    for kind in ("gnll", "ssi"):
        losses, d_rgb, d_depth, d_w, aux = D.driver_loss_ex(kind, *a)
        term, g_depth, g_w, aux2 = D.depth_term(kind, np.where(np.isnan(c["depth"]), 0.0, c["depth"]), c["w"], c["z"], c["depth_t"])
        assert losses[0] == base[0][0] and losses[2] == base[0][2] and losses[1] == term
        assert losses[3] == losses[0] + 0.005 * term + 1e3 * losses[2]
        assert np.array_equal(d_rgb, base[1]) and d_depth[D.NAN_AT] == 0.0 and np.array_equal(aux, aux2)
        zero_depth = optim_ref.driver_loss(c["rgb"], c["depth"], c["w"], c["z"], c["rgb_t"], c["depth_t"], 0.0, 1e3, D.DELTA)
        assert np.array_equal(d_w, zero_depth[3] + 0.005 * g_w)


def test_signatures_are_the_references():
    from text2nerf_amd import losses
    ref = json.load(open(os.path.join(GOLDEN, "depth_loss_signatures.json")))
    assert sorted(ref) == ["compute_depth_loss", "compute_depth_loss_scale_invariant", "is_not_in_expected_distribution",
                           "scale_shift_invariant_loss"]
    for name, want in ref.items():
        got = [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
               for p in inspect.signature(getattr(losses, name)).parameters.values()]
        assert got == want, name


def test_cpu_tensors_are_refused_and_the_elementwise_predicate_is_upstreams():
    from text2nerf_amd import losses
    from text2nerf_amd._lib import T2NError
    c = CASES["rand-5x64"]
    mu, w, z, y = (torch.from_numpy(c[k]) for k in ("depth_fin", "w", "z", "depth_t"))
    with pytest.raises(T2NError, match="no CPU fallback"):
        losses.compute_depth_loss(mu, z, w, y)
    with pytest.raises(T2NError, match="no CPU fallback"):
        losses.compute_depth_loss_scale_invariant(mu, y)
    with pytest.raises(T2NError, match="no CPU fallback"):
        losses.scale_shift_invariant_loss(z, w, y)
    empty = losses.compute_depth_loss(mu[:0], z[:0], w[:0], y[:0])
    assert tuple(empty.shape) == (1,) and float(empty.detach()) == 0.0 and empty.requires_grad
    o = D.gnll(c["depth_fin"], c["w"], c["z"], c["depth_t"], D.SIGMA)
    got = losses.is_not_in_expected_distribution(mu.double(), torch.from_numpy(o["var"]), y.double(), D.SIGMA)
    assert np.array_equal(got.numpy(), o["apply"])


def test_c_entry_points_check_their_arguments_before_any_launch():
    import ctypes as C
    from text2nerf_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "t2n.h")).read()
    for name in ("t2n_train_loss_ex", "t2n_train_loss_ex_workspace_bytes", "t2n_depth_loss", "t2n_depth_loss_workspace_bytes"):
        assert name in _lib.SIGNATURES and name + "(" in hdr, name
    assert _lib.DEPTH_KINDS == D.KINDS
    p = C.c_void_p(4096)      # never dereferenced: every call below is refused before a launch
    R, N = 8, 4
    big = 1 << 20
    ex = lambda kind, std, ws=big, rays=R: lib.t2n_train_loss_ex(p, p, p, p, p, p, rays, N, 0.005, 1e3, 0.1, kind, std, p, p, p, p, p, p, ws, None)   # noqa: E731
    assert ex(4, 0.1) == -1 and b"depth_kind" in lib.t2n_last_error()
    assert ex(-1, 0.1) == -1
    assert ex(1, 0.0) == -1 and b"target_std" in lib.t2n_last_error()
    assert ex(1, -1.0) == -1
    assert ex(1, 0.1, rays=0) == -1
    need = int(lib.t2n_train_loss_ex_workspace_bytes(R))
    assert need >= int(lib.t2n_train_loss_workspace_bytes(R)) > 0 and lib.t2n_train_loss_ex_workspace_bytes(0) == 0
    for kind in (0, 1, 2, 3):
        assert ex(kind, 0.1, ws=need - 1) == -4, kind
    assert lib.t2n_train_loss_ex(p, p, p, p, p, p, R, N, 0.005, 1e3, 0.1, 3, 0.1, p, p, p, p, None, p, big, None) == -1      # no aux
    dl = lambda kind, std, ws=big, w=p, dep=p: lib.t2n_depth_loss(kind, dep, w, w, p, R, N, std, p, p, None, None, p, ws, None)   # noqa: E731
    assert dl(0, 0.1) == -1 and dl(4, 0.1) == -1
    assert dl(1, 0.0) == -1
    assert dl(1, 0.1, w=None) == -1 and dl(3, 0.1, w=None) == -1 and dl(2, 0.1, dep=None) == -1
    need = int(lib.t2n_depth_loss_workspace_bytes(R))
    assert need > 0
    for kind, kw in ((1, {}), (2, dict(w=None)), (3, dict(dep=None))):
        assert dl(kind, 0.1, ws=need - 1, **kw) == -4, kind
