"""CPU test of gfs_host::OptimizeSim3 (geoflowslam_amd/host/gfs_adaptors.hpp) on mock KeyFrame / MapPoint classes
(tests/host/sim3_opt_adaptor_test.cpp) with the host restatement as the solve: the gather pair by pair against an independent
statement -- every skip branch, the i2 < 0 branch with bAllPoints on and off, the float arithmetic, the counters -- and the write-back:
vpMatches1 nulled exactly where a plain sequential run nulls it, g2oS12 and mAcumHessian left alone by the early return.  No GPU."""
import numpy as np
import pytest

import sim3_opt_support as S


def _check_gather(scene, o, all_points):
    prob, idx, in2, cnt = S.expected_gather(scene, all_points)
    n = len(idx)
    assert o["status_n"][0] == 1 and o["flat_n"][0] == n and o["flat_n"][1] == int(scene["fix_scale"])
    assert o["flat_n"][2:3].view(np.float32)[0] == scene["th2"] and o["s12_seen"].tobytes() == prob["s12"].tobytes()
    for k, mine in (("x1c", "x1c"), ("x2c", "x2c"), ("obs1", "obs1"), ("obs2", "obs2"), ("w1", "inv_sigma2_1"), ("w2", "inv_sigma2_2")):
        assert o[k][:n].tobytes() == prob[mine].tobytes(), k
    assert [int(v) for v in o["counters"][:5]] == [cnt[k] for k in ("nCorrespondences", "nBadMPs", "nInKF2", "nOutKF2", "nMatchWithoutMP")]
    return prob, idx, in2


def _check_write_back(scene, o, prob, idx, in2):
    r = S.run(prob)  # the plain sequential run on what the gather made
    matched = scene["kind"] != S.KIND_NO_MATCH  # every match the gather skipped stays as it was
    matched[idx[r["pair_state"] != 0]] = False
    assert (o["matched"].astype(bool) == matched).all()
    assert o["counters"][5] == r["n_bad"] and o["counters"][6] == ((r["pair_state"] == 1) & ~in2).sum()
    assert (o["status_n"][1], o["status_n"][2], o["status_n"][3]) == (r["status"], r["n_in"], r["n_bad"])
    if r["status"] == 1:
        assert o["ret"] == r["n_in"] > 0 and o["s12"].tobytes() == r["s12"].tobytes() and (o["hessian"] == 0).all()
    else:
        assert o["ret"] == 0 and o["s12"].tobytes() == prob["s12"].tobytes() and (o["hessian"] == 7.0).all(), "early return: untouched"
    return r


@pytest.mark.parametrize("all_points", [False, True])
@pytest.mark.parametrize("fix_scale", [True, False])
def test_gather_and_write_back(all_points, fix_scale):
    scene = S.adaptor_scene(11, n_good=20, n_gross=3, fix_scale=fix_scale)
    o = S.run_adaptor(scene, all_points)
    prob, idx, in2 = _check_gather(scene, o, all_points)
    assert (4 in idx) == all_points and not {0, 1, 2, 3, 5} & set(idx.tolist())
    if all_points:  # the i2 < 0 pair: float x / z, y / z as its observation, and level 0's weight although mnTrackScaleLevel is 3
        k = list(idx).index(4)
        assert prob["inv_sigma2_2"][k] == scene["sigma"][1][0] != scene["sigma"][1][3] and not in2[k]
        assert prob["obs2"][k, 0] == np.float64(np.float32(prob["x2c"][k, 0]) * (np.float32(1) / np.float32(prob["x2c"][k, 2])))
    r = _check_write_back(scene, o, prob, idx, in2)
    assert r["status"] == 1 and r["n_bad"] >= 3 and (r["pair_state"][-3:] == 1).all()


def test_early_return_leaves_s12_and_hessian():
    scene = S.adaptor_scene(12, n_good=8, n_gross=4)
    o = S.run_adaptor(scene, False)
    prob, idx, in2 = _check_gather(scene, o, False)
    r = _check_write_back(scene, o, prob, idx, in2)
    assert r["status"] == 0 and r["n_bad"] >= 4 and len(idx) - r["n_bad"] < 10
    assert not o["matched"][idx[r["pair_state"] == 1]].any(), "the first check's removals are nulled before the early return"


def test_no_pair_at_all():
    scene = S.adaptor_scene(13, n_good=0, n_gross=0)
    o = S.run_adaptor(scene, False)
    assert o["flat_n"][0] == 0 and o["ret"] == 0 and o["s12"].tobytes() == np.asarray(scene["s12"]).tobytes()
    assert (o["matched"].astype(bool) == (scene["kind"] != S.KIND_NO_MATCH)).all()


@pytest.mark.parametrize("camera_kind", [1, 2])
def test_two_camera_or_non_pinhole_key_frames_throw(camera_kind):
    scene = S.adaptor_scene(11)
    o = S.run_adaptor(scene, False, camera_kind=camera_kind)
    assert o["ret"] == -100 and o["status_n"][0] == 0
