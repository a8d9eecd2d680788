"""gfs_search_local_points (geoflowslam_amd/csrc/local_points.hip: frustum cull, scale prediction, stable compaction, map search -- the
second loop of Tracking::SearchLocalPoints, reference src/Tracking.cc:4312-4358, in one device call) against the sequential CPU
restatement (tests/host/local_points_restatement.cpp), bit for bit: no tolerance appears anywhere."""
import numpy as np
import pytest

import local_points_support as LPS

pytestmark = pytest.mark.gpu

CAPACITY, INVALID_ARG = -4, -1


@pytest.fixture(scope="module")
def matcher(gpu_api):
    m = gpu_api.ProjectionMatcher(max_last=4096, max_cur=1024, max_batch=4)
    m.reserve_local(4096)
    yield m
    m.close()


@pytest.mark.parametrize("case", LPS.CASES, ids=lambda c: "n_mp=%d-n_cur=%d" % c)
def test_random_frames(matcher, case):
    prob, want = LPS.frame(*case)
    LPS.assert_equal(matcher.search_local_points(prob), want, case)


@pytest.mark.parametrize("which", ("sf=1.1", "th=3", "hard"))
def test_other_scale_factor_window_and_order_dependent_matches(matcher, which):
    prob, want = dict(LPS.all_frames())[which]
    LPS.assert_equal(matcher.search_local_points(prob), want, which)


def test_ragged_batch_equals_single_calls(matcher):
    cases = [(1025, 500), (63, 1), (3000, 500)]
    probs = [LPS.frame(*c)[0] for c in cases]
    batch = matcher.search_local_points(probs)
    for c, b, p in zip(cases, batch, probs):
        LPS.assert_equal(b, LPS.frame(*c)[1], c)
        single = matcher.search_local_points(p)
        for k in LPS.OUT_KEYS:
            assert LPS.same_bits(b[k], single[k]), (c, k)  # (every byte, the fields the ABI leaves open included)


def test_constructed_points(matcher):
    for name, prob, labels in LPS.constructed_frames():
        want = LPS.restate(prob)
        LPS.check_constructed(name, prob, labels, want, want["index"])
        got = matcher.search_local_points(prob)
        LPS.assert_equal(got, want, name)
        searched = np.nonzero((got["in_view"] != 0) & ~((got["depth"] > prob["th_far_points"]) & bool(prob["far_points"])))[0]
        LPS.check_constructed(name, prob, labels, got, searched)


def test_equivalent_to_the_map_search_on_the_compacted_fields(matcher):
    """Ties the new path to gfs_search_by_projection_map, which tests/test_gpu_sbp.py checks."""
    for key in ((3000, 500), (1023, 500), (257, 1)):
        prob, want = LPS.frame(*key)
        cm, nm = matcher.SearchByProjectionMap(LPS.compacted(prob, want, want["index"]))
        got = matcher.search_local_points(prob)
        assert got["nmatches"] == nm and LPS.same_bits(got["cur_match"], LPS.map_back(cm, want["index"])), key


def _rc(fn):
    try:
        return 0, fn()
    except Exception as e:  # GfsError carries the library's code
        return getattr(e, "code", None), None


def test_refusals_leave_the_handle_usable(gpu_api):
    m = gpu_api.ProjectionMatcher(max_last=64, max_cur=512, max_batch=2)
    m.reserve_local(1100)
    base, base_want = LPS.frame(1025, 500)
    v = np.nonzero((base_want["in_view"] != 0))[0]
    assert base_want["n_searched"] > 65

    def cut(k):
        """the frame's first points up to and including the k-th member of the search set"""
        n = int(base_want["index"][k - 1]) + 1
        p = dict(base)
        for key in ("mp_xw", "mp_normal", "mp_min_dist", "mp_max_dist", "mp_desc", "mp_has_obs"):
            p[key] = np.asarray(base[key])[:n]
        return p

    p64, p65 = cut(64), cut(65)
    w64 = LPS.restate(p64)
    assert w64["n_searched"] == 64 and LPS.restate(p65)["n_searched"] == 65
    rc, first = _rc(lambda: m.search_local_points(p64))
    assert rc == 0
    LPS.assert_equal(first, w64, "64")
    rc, _ = _rc(lambda: m.search_local_points(p65))           # a search set of 65 > max_last
    assert rc == CAPACITY
    rc, again = _rc(lambda: m.search_local_points(p64))
    assert rc == 0 and all(LPS.same_bits(again[k], first[k]) for k in LPS.OUT_KEYS)
    rc, _ = _rc(lambda: m.search_local_points(LPS.frame(3000, 500)[0]))  # n_mp above the reserve
    assert rc == CAPACITY
    rc, again = _rc(lambda: m.search_local_points(p64))
    assert rc == 0 and all(LPS.same_bits(again[k], first[k]) for k in LPS.OUT_KEYS)
    bad = dict(p64)
    bad["scale_factors"] = np.ones(17, np.float32)
    bad["n_levels"] = 17
    rc, _ = _rc(lambda: m.search_local_points(bad))
    assert rc == INVALID_ARG
    for _ in range(3):  # three identical calls in a row give identical bytes
        rc, again = _rc(lambda: m.search_local_points(p64))
        assert rc == 0 and all(LPS.same_bits(again[k], first[k]) for k in LPS.OUT_KEYS)
        assert (again["n_to_match"], again["n_searched"], again["nmatches"]) == (first["n_to_match"], first["n_searched"], first["nmatches"])
    m.close()


def test_overflow_still_delivers_the_per_point_outputs(gpu_api):
    """The search is skipped on the device, the flag comes back with the results: GFS_ERR_CAPACITY, and the caller's arrays hold the
    per-point outputs and the counts."""
    import ctypes as C
    m = gpu_api.ProjectionMatcher(max_last=64, max_cur=512, max_batch=1)
    m.reserve_local(1100)
    prob, want = LPS.frame(1025, 500)
    P, R, keep = gpu_api.local_points_structs(prob)
    rc = gpu_api.lib().gfs_search_local_points(m.h, C.byref(P), 1, C.byref(R))
    assert rc == CAPACITY
    got = gpu_api.local_points_result(P, R, keep)
    assert got["n_to_match"] == want["n_to_match"] and got["n_searched"] == want["n_searched"] and got["nmatches"] == 0
    assert LPS.same_bits(got["in_view"], want["in_view"]) and (got["cur_match"] == -1).all()
    m.close()


def test_null_array_is_refused(gpu_api):
    import ctypes as C
    m = gpu_api.ProjectionMatcher(max_last=64, max_cur=512, max_batch=1)
    m.reserve_local(256)
    P, R, keep = gpu_api.local_points_structs(LPS.frame(63, 1)[0])
    P.mp_normal = None
    assert gpu_api.lib().gfs_search_local_points(m.h, C.byref(P), 1, C.byref(R)) == INVALID_ARG
    m.close()
