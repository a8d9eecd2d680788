"""gfs_sim3_search (k_sim3_search, geoflowslam_amd/csrc/sim3_search.hip, and the replay of the dependency between points) on the
MI355X against the sequential CPU restatement (tests/host/sim3_search_restatement.cpp): bit equality of exit, best index, best
distance and level in the three modes, no tolerance."""
import numpy as np
import pytest

import sim3_search_support as SS
from geoflowslam_amd import synth

pytestmark = pytest.mark.gpu
KEYS = ("exit", "best_idx", "best_dist", "level")


@pytest.fixture(scope="module")
def matcher(gpu_api):
    m = gpu_api.ProjectionMatcher(max_last=64, max_cur=4096, max_batch=1)
    m.reserve_sim3_search(5, 2304, 8)
    yield m
    m.close()


def _search(m, prob):
    return m.sim3_search(prob["lists"], prob["problems"])


@pytest.mark.parametrize("mode,n_mp,n_kp", SS.CASES, ids=["%s-%d-%d" % (SS.MODE_NAMES[m], n, c) for m, n, c in SS.CASES])
def test_every_wave_and_workgroup_edge(matcher, mode, n_mp, n_kp):
    prob, want, st = SS.problem(mode, n_mp, n_kp)
    got = _search(matcher, prob)
    SS.assert_equal(got, want, (mode, n_mp, n_kp))
    assert len(got[0]["exit"]) == n_mp
    if n_mp >= 255 and n_kp == 500:
        assert got[0]["n_matched"] > 0 and (np.bincount(got[0]["exit"], minlength=9) > 0).sum() >= 8


@pytest.mark.parametrize("mode", SS.MODES, ids=[SS.MODE_NAMES[m] for m in SS.MODES])
def test_full_key_point_table(matcher, mode):
    prob, want, st = SS.problem(mode, 600, 4096)
    SS.assert_equal(_search(matcher, prob), want, "4096 key-points")
    assert want[0]["n_matched"] > 0


@pytest.mark.parametrize("mode", SS.MODES, ids=[SS.MODE_NAMES[m] for m in SS.MODES])
def test_a_workgroup_walks_several_chunks(gpu_api, matcher, mode):
    """2 300 points are nine chunks of 256: with two problems and three workgroups allowed a workgroup walks all nine, with eight
    allowed four walk two or three each, and a workgroup a chunk is the one-chunk launch; the results are the same bytes."""
    prob, want, st = SS.problem(mode, 2300, 700, n_problems=2)
    try:
        for groups in (3, 8, -1, 0):
            assert gpu_api.lib().gfs_test_sim3_search_groups(matcher.h, groups) == 0
            SS.assert_equal(_search(matcher, prob), want, ("groups", groups))
    finally:
        gpu_api.lib().gfs_test_sim3_search_groups(matcher.h, 0)
    assert mode == SS.FUSE or st["displaced_by_earlier"] > 0


def test_one_list_in_five_problems(matcher):
    prob, want = SS.five_problems()
    got = _search(matcher, prob)
    SS.assert_equal(got, want, "batch of five")
    assert len({o["exit"].tobytes() for o in got}) == 5  # five different searches
    for f, pr in enumerate(prob["problems"]):  # ... and each equals its own single call
        SS.assert_equal([matcher.sim3_search(prob["lists"], pr)], [got[f]], ("single", f))


def test_two_lists_of_different_lengths(matcher):
    prob, want = SS.two_lists()
    got = _search(matcher, prob)
    SS.assert_equal(got, want, "two lists")
    assert [len(o["exit"]) for o in got] == [777, 130, 777, 130, 777]


def test_constructed_points(matcher):
    prob, labels, extra = SS.constructed()
    got = _search(matcher, prob)
    SS.check_constructed(prob, labels, got)
    SS.assert_equal(got, SS.restate(prob), "constructed")


@pytest.mark.parametrize("mode", SS.MODES, ids=[SS.MODE_NAMES[m] for m in SS.MODES])
def test_masks_given_and_null(matcher, mode):
    """kp_taken and mp_skip given, one of them, neither: each against the restatement, and the four outputs differ."""
    prob, want, st = SS.problem(mode, 700, 500)
    p = prob["problems"][0]
    seen = set()
    for taken, skip in ((True, True), (True, False), (False, True), (False, False)):
        if mode == SS.FUSE and taken:
            continue
        q = dict(lists=prob["lists"], problems=[dict(p, kp_taken=p["kp_taken"] if taken else None, mp_skip=p["mp_skip"] if skip else None)])
        got = _search(matcher, q)
        SS.assert_equal(got, SS.restate(q), (mode, taken, skip))
        assert ((got[0]["exit"] == SS.SKIPPED) == (p["mp_skip"] != 0)).all() if skip else (got[0]["exit"] != SS.SKIPPED).all()
        seen.add(got[0]["exit"].tobytes() + got[0]["best_idx"].tobytes())
    assert len(seen) == (2 if mode == SS.FUSE else 4)


def _refused(gpu_api, m, lists, problems, code):
    with pytest.raises(gpu_api.GfsError) as e:
        m.sim3_search(lists, problems)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals_leave_the_handle_usable(gpu_api):
    """One above each reserve -> GFS_ERR_CAPACITY; an unknown mode, 17 levels, an octave outside the pyramid, a `list` index out of
    range, a NULL array, kp_taken in FUSE mode, a ratio that is negative, NaN or lets 256 pass -> GFS_ERR_INVALID_ARG.  Nothing is
    truncated, and after every refusal the previous call gives identical bytes."""
    CAP, INV = -4, -1
    hdr = open(SS.os.path.join(SS.ROOT, "include", "gfs_abi.h")).read()
    assert "GFS_ERR_INVALID_ARG = -1," in hdr and "GFS_ERR_CAPACITY = -4," in hdr
    m = gpu_api.ProjectionMatcher(max_last=64, max_cur=512, max_batch=1)
    before = gpu_api.ProjectionMatcher(max_last=64, max_cur=512, max_batch=1)
    prob, want = SS.two_lists()  # 2 lists (777 and 130 points), 5 problems of 500 / 300 key-points
    lists, problems = prob["lists"], prob["problems"]
    m.reserve_sim3_search(2, 777, 5)
    base = _search(m, prob)
    SS.assert_equal(base, want, "at the reserve exactly")

    def again(what):
        got = _search(m, prob)
        for g, b in zip(got, base):
            assert all(SS.same_bits(g[k], b[k]) for k in KEYS) and g["n_matched"] == b["n_matched"], what

    big = synth.sim3_search_problem(803, SS.SBP, n_points=778, n_kp=100)
    _refused(gpu_api, m, [big["lists"][0], lists[1]], [dict(q, mp_skip=None) for q in problems], CAP)  # a list one longer than the reserve
    again("long list")
    _refused(gpu_api, m, lists + lists[1:], problems, CAP)      # three lists
    again("lists")
    _refused(gpu_api, m, lists, problems + problems[:1], CAP)   # six problems
    again("problems")
    wide = synth.sim3_search_problem(804, SS.SBP, n_points=130, n_kp=513)["problems"][0]
    _refused(gpu_api, m, lists, problems[:4] + [dict(wide, list=1, mp_skip=None)], CAP)  # 513 key-points, max_cur = 512
    again("key-points")
    p0 = problems[0]  # SBP_KFS on list 0
    for mode in (-1, 3):
        _refused(gpu_api, m, lists, [dict(p0, mode=mode)], INV)
    again("mode")
    _refused(gpu_api, m, lists, [dict(p0, n_levels=17, scale_factors=np.ones(17, np.float32))], INV)
    _refused(gpu_api, m, lists, [dict(p0, n_levels=0)], INV)
    again("levels")
    for octave in (-1, 8):
        kps = p0["kps_un"].copy()
        kps["octave"][17] = octave
        _refused(gpu_api, m, lists, [dict(p0, kps_un=kps)], INV)
    again("octave")
    for bad_list in (-1, 2):
        _refused(gpu_api, m, lists, [dict(p0, list=bad_list, mp_skip=None)], INV)
    again("list index")
    _refused(gpu_api, m, lists, [dict(p0, mode=SS.FUSE)], INV)  # kp_taken given in FUSE mode
    _search(m, dict(lists=lists, problems=[dict(p0, mode=SS.FUSE, kp_taken=None)]))
    again("kp_taken in FUSE mode")
    for ratio in (-0.5, float("nan"), 5.12, float("inf")):
        _refused(gpu_api, m, lists, [dict(p0, ratio_hamming=np.float32(ratio))], INV)
    _search(m, dict(lists=lists, problems=[dict(p0, ratio_hamming=np.float32(5.119))]))  # 50 * 5.119 < 256 is taken
    _search(m, dict(lists=lists, problems=[dict(p0, mode=SS.FUSE, kp_taken=None, ratio_hamming=np.float32(-1))]))  # not read in FUSE mode
    again("ratio")
    L = gpu_api.lib()
    for what in ("list", "result", "kps", "desc", "scale"):
        LL, PP, RR, keep = gpu_api.sim3_search_structs(lists, problems)
        if what == "list":
            LL[1].mp_normal = None
        elif what == "result":
            RR[3].best_dist = None
        elif what == "kps":
            PP[2].kps_un = None
        elif what == "desc":
            PP[2].desc = None
        else:
            PP[4].scale_factors = None
        assert L.gfs_sim3_search(m.h, LL, 2, PP, 5, RR) == INV, what
    again("NULL arrays")
    # a handle that never reserved refuses, and its other entry points are as before
    LL, PP, RR, keep = gpu_api.sim3_search_structs(lists, problems)
    assert L.gfs_sim3_search(before.h, LL, 2, PP, 5, RR) == CAP
    p = synth.sbp_pair(3, n_points=60, n_extra_cur=40)
    a, b = before.SearchByProjection(p), m.SearchByProjection(p)
    assert a[1] == b[1] and SS.same_bits(a[0], b[0])
    m.close()
    before.close()
