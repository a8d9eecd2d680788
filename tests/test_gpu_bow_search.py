"""gfs_search_by_bow (k_bow_search, geoflowslam_amd/csrc/bow_search.hip) on the MI355X against the sequential CPU restatement
(tests/host/bow_search_restatement.cpp): byte equality of match12 and n_matches, no tolerance."""
import os

import numpy as np
import pytest

import bow_search_support as BS
from geoflowslam_amd import synth

pytestmark = pytest.mark.gpu

CAP, INV = -4, -1


@pytest.fixture(scope="module")
def matcher(gpu_api):
    m = gpu_api.ProjectionMatcher(max_last=64, max_cur=320, max_batch=1)
    m.reserve_bow(60, 60 * 11)
    yield m
    m.close()


def test_constructed_cases(matcher):
    cases = BS.constructed()
    for label, (prob, want) in cases.items():
        got = matcher.search_by_bow(prob)
        assert [o["match12"].tolist() for o in got] == want, label
        assert [o["n_matches"] for o in got] == [sum(v >= 0 for v in w) for w in want], label
    got = matcher.search_by_bow([p for p, _ in cases.values()])  # ... and all of them in one call
    for (label, (prob, want)), g in zip(cases.items(), got):
        BS.assert_equal(g, BS.restate(prob), label)


@pytest.mark.parametrize("n1,n2", [(n1, n2) for n1 in (1, 70) for n2 in (63, 64, 65, 130)])
def test_one_node_at_the_chunk_boundaries(matcher, n1, n2):
    prob, want = BS.problem(100 + n2, n1, n2, n_kf2=2, n_nodes=1, one_sided_frac=0.0, wrong_node_frac=0.0, max_flip_bits=60)
    assert len(prob["kf1"]["node_id"]) == 1 and all(len(k["node_id"]) == 1 and k["node_start"][1] == n2 for k in prob["kf2"])
    BS.assert_equal(matcher.search_by_bow(prob), want, (n1, n2))


def test_one_node_holding_all_300_key_points_of_both_frames(matcher):
    prob, want = BS.problem(7, 300, 300, n_kf2=2, n_nodes=1, one_sided_frac=0.0, wrong_node_frac=0.0, dup_frac=0.15)
    _, traces = BS.restate(prob, with_traces=True)
    assert prob["kf1"]["node_start"].tolist() == [0, 300] and traces[:, 0].min() > 64 and traces[:, 3].min() > 0  # taken across chunks
    BS.assert_equal(matcher.search_by_bow(prob), want, "300 x 300")


def test_one_key_point_and_nodes_of_one_key_point_each(matcher):
    prob, want = BS.problem(8, 1, 1, n_kf2=3, n_nodes=1, one_sided_frac=0.0, wrong_node_frac=0.0, no_mp_frac=0.0, max_flip_bits=30)
    BS.assert_equal(matcher.search_by_bow(prob), want, "one key point")
    assert sum(o["n_matches"] for o in want) > 0
    n = 90  # key-point i alone in node i, on both sides
    rng = np.random.default_rng(9)
    d1 = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    d2 = synth._flip_bits(rng, d1, rng.integers(0, 70, n))
    nodes = [(2 * i, [i]) for i in range(n)]
    prob = BS.prob(BS.kf(d1, nodes, angle=rng.random(n) * 360), BS.kf(d2, nodes, angle=rng.random(n) * 360), check_orientation=True)
    want = BS.restate(prob)
    assert 0 < want[0]["n_matches"] < n
    BS.assert_equal(matcher.search_by_bow(prob), want, "nodes of one key point")


def test_random_sweep(matcher):
    """300 random problems in five calls.  First: the restatement's traces show that every branch is taken somewhere in the sweep."""
    probs, want, traces = BS.sweep()
    total = dict(zip(BS.TRACES, traces.sum(0).tolist()))
    assert all(v > 0 for v in total.values()), total
    for a in range(0, 300, 60):
        got = matcher.search_by_bow(probs[a:a + 60])
        for b, g in enumerate(got):
            BS.assert_equal(g, want[a + b], ("sweep", a + b))


def test_batch_independence_and_repeatability(matcher):
    probs, want, _ = BS.sweep()
    p = probs[10]
    alone = matcher.search_by_bow(p)
    BS.assert_equal(alone, want[10], "alone")
    for at in (0, 3, 7):
        batch = probs[20:27]
        batch = batch[:at] + [p] + batch[at:]
        BS.assert_equal(matcher.search_by_bow(batch)[at], alone, ("inside a batch of 7 others", at))
    BS.assert_equal(matcher.search_by_bow(p), alone, "the same call twice")


def _refused(gpu_api, m, probs, code):
    with pytest.raises(gpu_api.GfsError) as e:
        m.search_by_bow(probs)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals_write_nothing_and_leave_the_handle_usable(gpu_api):
    """Above each reserve or without one -> GFS_ERR_CAPACITY; each invalid argument -> GFS_ERR_INVALID_ARG; the caller's arrays are
    not written, and after every refusal the previous call gives identical bytes."""
    hdr = open(os.path.join(BS.ROOT, "include", "gfs_abi.h")).read()
    assert "GFS_ERR_INVALID_ARG = -1," in hdr and "GFS_ERR_CAPACITY = -4," in hdr
    prob, want = BS.problem(11, 200, 190, n_kf2=3, n_nodes=12)
    m = gpu_api.ProjectionMatcher(max_last=64, max_cur=200, max_batch=1)
    before = gpu_api.ProjectionMatcher(max_last=64, max_cur=200, max_batch=1)
    m.reserve_bow(2, 6)
    base = m.search_by_bow([prob, prob])  # at every reserve exactly
    BS.assert_equal(base[0], want, "at the reserve")
    BS.assert_equal(base[1], want, "at the reserve")

    def again(what):
        for g in m.search_by_bow([prob, prob]):
            BS.assert_equal(g, want, what)

    def raw(handle, probs, code, what):
        """the call on ctypes views: the documented code, and the result arrays keep their fill pattern"""
        PP, RP, keep = gpu_api.bow_structs(probs)
        assert gpu_api.lib().gfs_search_by_bow(handle.h, PP, len(probs), RP) == code, what
        for k in keep:
            if isinstance(k, tuple):
                assert all((o == -9).all() for o in k[2]) and all(k[1][i].n_matches == -9 for i in range(len(k[2]))), what

    raw(m, [prob, prob, prob], CAP, "three problems, reserve 2")
    again("problems")
    raw(m, [prob, dict(prob, kf2=prob["kf2"] + prob["kf2"][:1])], CAP, "seven key frames 2, reserve 6")
    again("key frames 2")
    raw(before, [prob], CAP, "never reserved")
    wide = synth.bow_search_problem(5, n_kp=201, n_kf2=1, n_nodes=12)
    raw(m, [wide], INV, "201 key-points, max_cur = 200")
    raw(m, [dict(prob, kf2=[prob["kf2"][0], wide["kf2"][0]])], INV, "201 key-points in a key frame 2")
    again("key-points")

    def kf1_with(**kw):
        return dict(prob, kf1=dict(prob["kf1"], **kw))

    def kf2_with(**kw):
        return dict(prob, kf2=[prob["kf2"][0], dict(prob["kf2"][1], **kw), prob["kf2"][2]])

    feat = prob["kf2"][1]["feat_idx"].copy()
    feat[3] = feat[4]
    raw(m, [kf2_with(feat_idx=feat)], INV, "an index listed twice")
    feat[3] = 190
    raw(m, [kf2_with(feat_idx=feat)], INV, "an index outside [0, n_kp)")
    feat[3] = -1
    raw(m, [prob, kf2_with(feat_idx=feat)], INV, "a negative index, in the second problem")
    again("feature index")
    ids = prob["kf1"]["node_id"].copy()
    ids[2] = ids[1]
    raw(m, [kf1_with(node_id=ids)], INV, "node ids not strictly ascending")
    ids[2], ids[1] = prob["kf1"]["node_id"][1], prob["kf1"]["node_id"][2]
    raw(m, [kf1_with(node_id=ids)], INV, "node ids descending")
    ns = prob["kf2"][1]["node_start"].copy()
    ns[-1] += 1
    raw(m, [kf2_with(node_start=ns)], INV, "node_start beyond n_kp")
    again("node arrays")
    _refused(gpu_api, m, kf1_with(node_id=ids), INV)  # ... and as the Python binding raises it
    _refused(gpu_api, m, [prob, prob, prob], CAP)
    for field in ("angle", "desc", "has_mp", "node_id", "node_start", "feat_idx"):
        for side in (1, 2):
            PP, RP, keep = gpu_api.bow_structs([prob])
            setattr(PP[0].kf1 if side == 1 else PP[0].kf2[1], field, None)
            assert gpu_api.lib().gfs_search_by_bow(m.h, PP, 1, RP) == INV, (field, side)
            assert all((o == -9).all() for o in keep[-1][2])
    PP, RP, keep = gpu_api.bow_structs([prob])
    RP[0][1].match12 = None
    assert gpu_api.lib().gfs_search_by_bow(m.h, PP, 1, RP) == INV
    assert (keep[-1][2][0] == -9).all() and (keep[-1][2][2] == -9).all()
    again("NULL arrays")
    # valid: no problem, a problem without key frames 2, key frames without nodes
    assert gpu_api.lib().gfs_search_by_bow(m.h, None, 0, None) == 0
    assert m.search_by_bow(dict(prob, kf2=[])) == []
    none = dict(node_id=np.zeros(0, np.int32), node_start=np.zeros(1, np.int32), feat_idx=np.zeros(0, np.int32))
    got = m.search_by_bow(dict(prob, kf2=[dict(prob["kf2"][0], **none), prob["kf2"][1]]))
    assert got[0]["n_matches"] == 0 and (got[0]["match12"] == -1).all()
    BS.assert_equal(got[1:], want[1:2], "beside a key frame without nodes")
    assert all(o["n_matches"] == 0 for o in m.search_by_bow(kf1_with(**none)))
    again("valid edge cases")
    p = synth.sbp_pair(3, n_points=60, n_extra_cur=40)  # the handle's other entries are as on a handle that never reserved
    a, b = before.SearchByProjection(p), m.SearchByProjection(p)
    assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes()
    m.close()
    before.close()


def test_detection_shape(gpu_api):
    """The workload's shape, once: 3 candidates x 11 key frames 2 of 2 000 key-points over 100 nodes."""
    probs = [synth.bow_search_problem(40 + c, n_kp=2000, n_kf2=11, n_nodes=100) for c in range(3)]
    want = BS.restate(probs)
    m = gpu_api.ProjectionMatcher(max_last=64, max_cur=2000, max_batch=1)
    m.reserve_bow(3, 33)
    got = m.search_by_bow(probs)
    m.close()
    for b, (g, w) in enumerate(zip(got, want)):
        BS.assert_equal(g, w, ("detection", b))
    assert min(o["n_matches"] for w in want for o in w) >= 20
