"""The marchers' per-entry law and checkers, on the CPU (tests/helpers/march_ref.py; the device half is tests/test_march_list_gpu.py).

1. The law is honest: on every case of the device file the float32 oracles (oracle_torch.forward, oracle_c) lie within 1 x the bound
   (rho32 = max err / b <= 1; the device is held to K = 4). One `MARCHLIST cpu` line per case (profiles/march_list_elementwise.txt).
2. The bound cannot hide a failure: conditions on the reference alone (share of "either" samples, population of the threshold band,
   the n_app values at k_composite's trip edges, rays beyond the staging slice).
3. Every checker catches its mutations, and passes the clean lists. The lists are the float32 oracle's (oracle_lists): no device.
4. The gap this file closes: an entry of weight 2e-4 missing from a ray moves its colour by less than the frame tests' 1e-4."""
import numpy as np
import pytest

from oracle import oracle_torch as O
from tests.helpers import march_ref as M

ALL = M.GEOMETRY + M.VARIANTS + M.ROUTES
GROUPS = {"forms": M.GEOMETRY, "variants": M.VARIANTS, "routes": M.ROUTES}
BIG = "16x16x16/24x16/inside"       # the case of the mutation tests: 4063 entries, rays with up to 14


# ---- 1. rho32 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_law_holds_the_float32_oracles(name):
    c, ref, L = M.case(name), M.reference(name), M.oracle_of(name)
    rho = ref.rho(L["weights"], L["acc"], L["depth"])
    line = f"MARCHLIST cpu {name} rays {ref.R} N {ref.N} rho32 torch w {rho['w']:.3f} acc {rho['acc']:.3f} depth {rho['depth']:.3f}"
    flips = int(((L["weights"] > np.float32(ref.thr)) != (ref.w > ref.thr))[ref.ray.valid].sum())
    assert max(rho.values()) <= 1.0, line
    if not c["mask"]:               # (oracle_c has no alpha mask)
        from oracle.oracle_c import COracle
        params = c["params"]
        if c["bf16"]:
            params = {k: v.numpy() for k, v in O.round_factors_bf16(O.params_from_numpy(params)).items()}
        _, depth, _, w = COracle(c["cfg"], params).render(c["rays"], n_samples=ref.N, is_train=c["train"], jitter=c["jitter"])
        rc = ref.rho(w, w.sum(-1, dtype=np.float32), depth)
        line += f" | c w {rc['w']:.3f} acc {rc['acc']:.3f} depth {rc['depth']:.3f}"
        assert max(rc.values()) <= 1.0, line
    st = ref.band_stats()
    print(f"{line} | evaluated {st['evaluated']} band {st['band']} ({st['below']} below, {st['above']} above) either {st['either']} "
          f"float32 flips {flips} max b/thr in band {float((ref.b[ref.band] / ref.thr).max()) if st['band'] else 0.0:.2e}")


# ---- 2. conditions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", list(GROUPS))
def test_either_samples_are_few(group):
    st = [M.reference(n).band_stats() for n in GROUPS[group]]
    either, band = sum(s["either"] for s in st), sum(s["band"] for s in st)
    print(f"{group}: {either} either samples, {band} samples with w64 in [thr / 2, 2 thr]")
    assert band > 0 and either <= 0.05 * band


@pytest.mark.parametrize("name", [f"{g}/24x16/{c}" for g in M.GRIDS for c in ("inside", "axis")])
def test_large_frames_populate_the_threshold(name):
    st = M.reference(name).band_stats()
    assert st["below"] >= 100 and st["above"] >= 100, st


def test_entry_counts_at_the_composite_edges():
    seen, over = set(), 0
    for name in ALL:
        ref = M.reference(name)
        n = ref.n_app()
        seen |= set(int(v) for v in n)
        over += int((n > ref.N // 4).sum())
    print(f"n_app values over all cases: {sorted(seen)}; {over} rays above N / 4")
    assert {0, 1, 7, 8, 9, 15, 16, 17} <= seen and max(seen) >= 25
    assert over > 0


def test_masks_reject_samples():
    """`mask` (the suite's alpha_mask()) rejects nothing on these frames; `sparse` leaves gaps in every window of the inside frame, and
    the records still give the box window."""
    plain, mask, sparse = (M.reference(f"{v}/inside") for v in ("bf16", "mask", "sparse"))
    assert np.array_equal(mask.ray.valid, plain.ray.valid)
    assert sparse.ray.valid.sum() < 0.5 * plain.ray.valid.sum()
    assert ((sparse.ray.Lw - sparse.ray.nvalid) > 0).all() and np.array_equal(sparse.word, plain.word)


# ---- 3. mutations -----------------------------------------------------------------------------------------------------------------------
def checkers(ref, L, mutate=None):
    """Offending rays per checker; a list mutation goes to the two checkers that take lists."""
    return {"records": ref.check_records(L, mutate), "entries": ref.check_entries(L, mutate),
            "acc_depth": ref.check_acc_depth(L["acc"], L["depth"]), "weights_rows": ref.check_weights_rows(L["weights"], L["z_vals"]),
            "composite": ref.check_composite(L, L["rgb_out"])}


@pytest.mark.parametrize("name", ALL)
def test_clean_lists_pass_every_checker(name):
    bad = checkers(M.reference(name), M.oracle_of(name))
    assert all(len(v) == 0 for v in bad.values()), {k: v[:8] for k, v in bad.items()}


@pytest.mark.parametrize("mutate,name,caught_by", [("sigma_scale", "relu/inside", ("entries", "weights_rows")),
                                                   ("unscaled_dist", BIG, ("entries", "weights_rows", "acc_depth")),
                                                   ("last_dist", "gather", ("weights_rows", "acc_depth", "entries")),
                                                   ("alpha_threshold", BIG, ("entries", "records")),
                                                   ("depth_no_last", BIG, ("acc_depth",))])
def test_reference_mutations(mutate, name, caught_by):
    """sigma (1 + 1e-4) is caught on the relu field, whose features have A ~ 0.7. On the softplus fields (density_scale 0.8, A ~ 20) the
    feature term of the law alone is K GAMMA_F A = 1.2e-4 relative: the mutation reaches 0.82 K b there (measured on the reference, no
    device) and passes. A sigma error is visible on those fields from 1.3e-4 relative on, eight times under the 1e-3 that passes today.
    The last sample's dist shows where a ray's last sample lies in the box with transmittance left: the 45-sample rays of `gather`."""
    bad = checkers(M.mutant(name, mutate), M.oracle_of(name))
    print(mutate, {k: len(v) for k, v in bad.items()})
    for k in caught_by:
        assert len(bad[k]) > 0, (mutate, k)


def test_dropped_carry():
    """The transmittance restarted every 64 samples: a case of its own, windows of up to 151 samples (the device cases stop at 45)."""
    c = M.case("16x16x16/8x8/inside")
    cfg = O.FieldConfig(aabb=c["aabb"], grid_size=c["grid"], near_far=c["near_far"], step_ratio=0.1)
    clean = M.MarchRef(cfg, c["params"], c["rays"], 200)
    assert int(clean.ray.Lw.max()) > 64
    L = M.oracle_lists(clean, c["params"], c["rays"])
    assert all(len(v) == 0 for v in checkers(clean, L).values())
    bad = checkers(M.MarchRef(cfg, c["params"], c["rays"], 200, mutate="drop_carry"), L)
    assert len(bad["entries"]) > 0 and len(bad["weights_rows"]) > 0 and len(bad["acc_depth"]) > 0, {k: len(v) for k, v in bad.items()}


@pytest.mark.parametrize("mutate,caught_by", [("drop_entry", "entries"), ("add_entry", "entries"), ("swap_entries", "entries"),
                                              ("next_position", "entries"), ("z_ulp", "entries"), ("rgb_w_ulp", "entries"),
                                              ("n_valid", "records"), ("first", "records")])
def test_list_mutations(mutate, caught_by):
    ref, L = M.reference(BIG), M.oracle_of(BIG)
    bad = {"records": ref.check_records(L, mutate), "entries": ref.check_entries(L, mutate)}
    print(mutate, {k: v.tolist() for k, v in bad.items()})
    assert len(bad[caught_by]) == 1, (mutate, bad)          # one ray was touched: that ray and no other


@pytest.mark.parametrize("mutate", ["no_bg", "no_clamp", "skip_8", "last_twice"])
def test_composite_mutations(mutate):
    ref, L = M.reference(BIG), M.oracle_of(BIG)
    assert int(L["ray_app"][:, 0].max()) >= 9
    bad = ref.check_composite(L, L["rgb_out"], mutate=mutate)
    print(mutate, len(bad), "rays")
    assert len(bad) > 0
    if mutate == "skip_8":
        assert set(bad) <= set(np.nonzero(L["ray_app"][:, 0] >= 9)[0])


# ---- 4. the gap --------------------------------------------------------------------------------------------------------------------------
def test_missing_entry_passes_the_frame_tolerance_and_fails_here():
    """An entry of weight 2e-4 removed from one ray: its colour moves by w |rgb| < 1e-4, the tolerance at which frames are compared with
    oracle_c, and check_entries names the ray."""
    ref, L = M.reference(BIG), M.oracle_of(BIG)
    w, col = L["entries"][:, 3], np.abs(L["app_rgb"][:, :3]).max(-1)
    cand = np.nonzero((np.abs(w - 2e-4) < 2e-5) & (col < 0.45))[0]
    assert len(cand) > 0
    e = int(cand[0])
    ray = int(L["app_ray"][e])
    assert float(w[e] * col[e]) < 1e-4 and ref.must[ray].sum() > 0
    cut = dict(L)
    for k in ("entries", "app_rgb", "app_ray"):
        cut[k] = np.delete(L[k], e, 0)
    cut["ray_app"] = L["ray_app"].copy()
    cut["ray_app"][ray, 0] -= 1
    cut["total"] = L["total"] - 1
    assert ref.check_entries(cut).tolist() == [ray] and ref.check_records(cut).tolist() == [ray]
