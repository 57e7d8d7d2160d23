"""The TSDF reference (tests/helpers/tsdf_ref.py) on its own, without a device: what the observed-cells rule does to the sphere scene,
views one at a time against all at once, mutations of the definition that the bit comparison must catch, and the refusals of
text2nerf_amd.tsdf that need no device. tests/test_tsdf_gpu.py asks the device for this reference's bits.

The committed scene (profiles/tsdf_mesh.txt): a 37x21x45 grid of spacing 0.1, a sphere of radius 0.8, three 33x24 views, trunc 0.3.
Ray distance: 605 of 2188 faces kept, kept vertices within 0.030 inside / 0.044 outside of the sphere, the unfiltered mesh reaches
0.346 inside (the shell at -trunc behind the surface). z-depth: 611 of 2216, 0.029 / 0.046, 0.346."""
import math

import numpy as np
import pytest

from tests.helpers import tsdf_ref as R


@pytest.fixture(scope="module", params=[0, 1], ids=["ray", "z"])
def fused(request):
    sc = R.sphere_scene(kind=request.param)
    return sc, R.run(sc)


def test_some_node_integrates_every_view(fused):
    sc, (T, Wt, Cl) = fused
    V = len(sc["depth"])
    assert float(Wt.max()) == V and int((Wt == V).sum()) > 100
    assert 0 < int((Wt > 0).sum()) < Wt.size                    # and the views do not cover the grid
    assert (T[Wt == 0] == 1).all() and (Cl[Wt == 0] == 0).all()  # untouched nodes keep the fresh state
    assert float(T.min()) >= -1.0 and float(T.max()) <= 1.0 and float(Cl.min()) >= 0.0 and float(Cl.max()) <= 1.0


def test_observed_cells_rule_keeps_the_surface_and_drops_the_shell(fused):
    sc, st = fused
    h = max(sc["spacing"])
    (v, f, n, c), keep, (v0, f0) = R.mesh(st, sc["origin"], sc["spacing"])
    kept, total = int(keep.sum()), len(f0)
    d, d0 = R.sphere_distance(v, sc), R.sphere_distance(v0, sc)
    print(f"TSDF mesh kind {sc['kind']}: {kept} of {total} faces kept, {len(v)} of {len(v0)} vertices; kept vertices {-d.min():.4f} inside "
          f"/ {d.max():.4f} outside of the sphere; unfiltered {-d0.min():.4f} inside / {d0.max():.4f} outside; spacing {h}")
    assert 0 < kept < total and len(f) == kept
    assert np.abs(d).max() <= 1.5 * h                           # every kept vertex lies near the sphere
    assert -d0.min() >= 3.0 * h                                 # the unfiltered mesh has the shell at -trunc behind the surface
    assert f.min() == 0 and f.max() == len(v) - 1 and len(np.unique(f)) == len(v)     # no unreferenced vertex is left
    assert c.shape == v.shape and c.dtype == np.uint8 and n.shape == v.shape
    # the kept faces look at the cameras: their normals point out of the sphere
    out = (v.astype(np.float64) - np.asarray(sc["centre"])) / np.linalg.norm(v - np.asarray(sc["centre"]), axis=-1, keepdims=True)
    assert float((n * out).sum(-1).min()) > 0.5


def test_views_one_at_a_time_equal_all_at_once(fused):
    sc, st = fused
    for weights, cap in ((False, math.inf), (True, 2.5)):
        whole = st if not weights else R.run(sc, weights=True, max_weight=cap)
        part = None
        for v in range(len(sc["depth"])):
            part = R.run(sc, weights=weights, max_weight=cap, state=part, views=[v])
        assert all(R.same_bits(a, b) for a, b in zip(whole, part))
    assert float(whole[1].max()) == 2.5                         # the cap was reached


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_integrate_mutations_are_caught(fused, mutation):
    sc, st = fused
    bad = R.run(sc, mutate=mutation)
    assert not R.same_bits(st[0], bad[0]) and not R.same_bits(st[2], bad[2])


def test_face_rule_mutation_is_caught(fused):
    sc, st = fused
    _, keep, (v0, f0) = R.mesh(st, sc["origin"], sc["spacing"])
    bad = R.face_flags(v0, f0, st[1], sc["origin"], sc["spacing"], mutate="first_vertex")
    assert int((bad != keep).sum()) > 0


def test_bad_pixels_are_no_measurement(fused):
    sc, st = fused
    bad = R.with_bad_pixels(sc)
    assert np.isnan(bad["depth"]).any() and np.isinf(bad["depth"]).any() and (bad["depth"] < 0).any() and np.isnan(bad["pw"]).any()
    T, Wt, Cl = R.run(bad, weights=True)
    assert np.isfinite(T).all() and np.isfinite(Wt).all() and np.isfinite(Cl).all()
    assert int((Wt > 0).sum()) < int((R.run(sc, weights=True)[1] > 0).sum())


def test_select_faces_reference():
    v = np.arange(18, dtype=np.float32).reshape(6, 3)
    f = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 0]], np.int32)
    c = (np.arange(18) % 251).astype(np.uint8).reshape(6, 3)
    ov, of, on, oc = R.select_faces(v, f, None, c, np.array([0, 1, 0]))
    assert np.array_equal(ov, v[2:5]) and np.array_equal(of, [[0, 1, 2]]) and on is None and np.array_equal(oc, c[2:5])
    ov, of, _, _ = R.select_faces(v, f, None, None, np.zeros(3))
    assert ov.shape == (0, 3) and of.shape == (0, 3)
    ov, of, _, _ = R.select_faces(v, f, None, None, np.ones(3))
    assert np.array_equal(ov, v) and np.array_equal(of, f)


def test_refusals_that_need_no_device():
    from text2nerf_amd import tsdf
    sc = R.sphere_scene()
    d, p, k = sc["depth"], sc["poses"], sc["intrinsic"]
    good = dict(origin=sc["origin"], spacing=sc["spacing"], shape=sc["shape"], trunc=sc["trunc"])

    def refused(depths=d, poses=p, intrinsic=k, **kw):
        with pytest.raises(ValueError):
            tsdf.tsdf_integrate(depths, poses, intrinsic, **{**good, **kw})

    refused(trunc=0.0)
    refused(trunc=math.nan)
    refused(spacing=(0.1, 0.0, 0.1))
    refused(spacing=(0.1, math.inf, 0.1))
    refused(intrinsic=(0.0, 40.0, 16.5, 12.0))
    refused(intrinsic=(40.0, math.nan, 16.5, 12.0))
    refused(depth_kind="disparity")
    refused(shape=(2048, 1024, 1024))                           # 2^31 nodes
    refused(shape=(37, 21))
    refused(poses=p[:2])                                        # mismatched shapes
    refused(depths=d[0])
    refused(colors=sc["rgb"][:, :, :-1])
    refused(weights=sc["pw"][:, :-1])
    refused(max_weight=0.0)
    nan_pose = p.copy()
    nan_pose[1, 0, 3] = np.nan
    refused(poses=nan_pose)
    flat = p.copy()
    flat[2, :3, :3] = 0.0
    refused(poses=flat)                                         # not invertible
    T, Wt, Cl = R.fresh(sc["shape"])
    vol = tsdf.TSDFVolume(T, Wt, Cl, tuple(float(np.float32(t)) for t in sc["origin"]), tuple(float(np.float32(t)) for t in sc["spacing"]),
                          float(sc["trunc"]))
    refused(volume=vol._replace(trunc=0.25))
    refused(volume=vol._replace(origin=(0.0, 0.0, 0.0)))
    refused(volume=vol._replace(tsdf=T[:-1], weight=Wt[:-1]))
    refused(volume=vol, colors=sc["rgb"])                       # colours on one side only
    # V = 0 hands a given volume back as it is, without a device
    assert tsdf.tsdf_integrate(d[:0], p[:0], k, volume=vol, **good) is vol
    assert np.array_equal(tsdf.world_to_camera(p), sc["w2c"])
    with pytest.raises(ValueError):
        tsdf.tsdf_mesh(vol, min_weight=math.nan)
    with pytest.raises(ValueError):
        tsdf.tsdf_mesh(vol._replace(weight=Wt[:-1]))
