"""gfs_map_points_update (k_map_points, geoflowslam_amd/csrc/map_points.hip) on the MI355X against the sequential CPU restatement
(tests/host/map_point_restatement.cpp): bit equality of the best observation, its median, the normal, both distances and the
status, no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import map_point_support as MS
from geoflowslam_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def updater(gpu_api):
    u = gpu_api.MapPointUpdater(max_points=1024, max_observations=32768)
    yield u
    u.close()


@pytest.mark.parametrize("count", MS.COUNTS)
def test_every_observation_count(updater, count):
    prob, want = MS.uniform(count)
    MS.assert_equal(updater.update(prob), want, count)


def test_all_counts_in_one_problem(updater):
    prob, want = MS.mixed()
    got = updater.update(prob)
    MS.assert_equal(got, want, "mixed")
    assert len(got["status"]) == 2 * len(MS.COUNTS) and set(got["status"].tolist()) >= {0, 3}


@pytest.mark.parametrize("n_points", MS.N_POINTS)
def test_point_counts(updater, n_points):
    prob, want = MS.sized(n_points)
    got = updater.update(prob)
    assert len(got["best_obs"]) == n_points
    MS.assert_equal(got, want, n_points)


def test_normals_only_mode(updater):
    prob, want = MS.mixed()
    got = updater.update(prob, normals_only=True)
    MS.assert_equal(got, want, "normals only", MS.NORMAL_FIELDS)
    MS.assert_equal(got, MS.restate(prob, normals_only=True), "normals only")
    assert (got["best_obs"] == -1).all() and (got["best_median"] == -1).all()
    assert (got["status"] == (want["status"] & 1)).all()


def test_constructed_points(updater):
    prob, labels = MS.constructed()
    got = updater.update(prob)
    MS.check_constructed(prob, labels, got)
    MS.assert_equal(got, MS.restate(prob), "constructed")


def test_same_problem_twice_gives_identical_bytes(updater):
    prob, _ = MS.mixed()
    a, b = updater.update(prob), updater.update(prob)
    for k in MS.FIELDS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_refusals_leave_the_handle_usable(gpu_api):
    """One above each reserve -> GFS_ERR_CAPACITY; a NULL array, obs_start[0] != 0, a decreasing obs_start, an unknown mode ->
    GFS_ERR_INVALID_ARG.  Nothing is truncated, and after every refusal the previous call gives identical bytes."""
    CAP, INV = -4, -1
    hdr = open(os.path.join(MS.ROOT, "include", "gfs_abi.h")).read()
    assert "GFS_ERR_INVALID_ARG = -1," in hdr and "GFS_ERR_CAPACITY = -4," in hdr
    prob = synth.map_point_update_problem(31, n_points=40, obs_counts=(1, 20))
    n_obs = int(prob["obs_start"][-1])
    u = gpu_api.MapPointUpdater(max_points=40, max_observations=n_obs)
    base = u.update(prob)
    MS.assert_equal(base, MS.restate(prob), "at the reserve exactly")
    L = gpu_api.lib()

    def again(what):
        got = u.update(prob)
        for k in MS.FIELDS:
            assert got[k].tobytes() == base[k].tobytes(), (what, k)

    def refused(p, code, what, normals_only=False, edit=None):
        P, R, keep = gpu_api.map_points_structs(p, normals_only)
        if edit:
            edit(P, R)
        assert L.gfs_map_points_update(u.h, C.byref(P), C.byref(R)) == code, what
        assert all((keep[k] == keep[k].flat[0]).all() for k in MS.FIELDS), (what, "a result array was written")
        again(what)

    more_points = synth.map_point_update_problem(32, n_points=41, obs_counts=1)
    refused(more_points, CAP, "41 points")
    counts = np.diff(prob["obs_start"]).astype(np.int64)
    counts[7] += 1
    more_obs = synth.map_point_update_problem(31, n_points=40, obs_counts=counts)
    assert int(more_obs["obs_start"][-1]) == n_obs + 1
    refused(more_obs, CAP, "one observation more")
    with pytest.raises(gpu_api.GfsError) as e:
        u.update(more_obs)
    assert e.value.code == CAP
    again("raised")
    for name in ("obs_start", "obs_Ow", "obs_desc", "obs_flags", "pos", "ref_Ow", "level_scale", "max_scale"):
        refused(prob, INV, name, edit=lambda P, R, name=name: setattr(P, name, None))
    for name in MS.FIELDS:
        refused(prob, INV, name, edit=lambda P, R, name=name: setattr(R, name, None))
    shifted = dict(prob, obs_start=np.r_[1, prob["obs_start"][1:]].astype(np.int32))
    refused(shifted, INV, "obs_start[0] = 1")
    down = prob["obs_start"].copy()
    down[5] = down[4] - 1
    refused(dict(prob, obs_start=down), INV, "obs_start decreases")
    refused(prob, INV, "mode 2", edit=lambda P, R: setattr(P, "mode", 2))
    # a normals-only call needs no descriptors
    P, R, keep = gpu_api.map_points_structs(prob, normals_only=True)
    assert P.obs_desc is None and L.gfs_map_points_update(u.h, C.byref(P), C.byref(R)) == 0
    MS.assert_equal(gpu_api.map_points_results(P, keep), base, "normals only, no descriptors", MS.NORMAL_FIELDS)
    again("normals only")
    u.close()
