"""ORBmatcher::SearchByBoW(pKF1, pKF2, ...) (reference src/ORBmatcher.cc:936-1053) on the CPU: the sequential restatement
(tests/host/bow_search_restatement.cpp, written from the reference's text) and the rule header's host build
(geoflowslam_amd/csrc/bow_search_rule.hpp, gfs_bow::search_pair) on the hand-built cases, whose outputs are stated by hand, and on
the random sweep, where the two must agree byte for byte.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import bow_search_support as BS

CASES = BS.constructed()


@pytest.mark.parametrize("label", list(CASES))
@pytest.mark.parametrize("which", ["restatement", "rule"])
def test_constructed_case(which, label):
    prob, want = CASES[label]
    got = (BS.restate if which == "restatement" else BS.rule_host)(prob)
    assert [o["match12"].tolist() for o in got] == want, label
    assert [o["n_matches"] for o in got] == [sum(v >= 0 for v in w) for w in want], label
    assert all(o["match12"].dtype == np.int32 for o in got)


def test_ratio_in_float32_agrees_with_the_rational_comparison():
    """With 0.9f every pair (bestDist1 < 50, bestDist2 <= 256) compares as 9/10 does exactly; the ties are the five multiples of
    (9, 10) below TH_LOW and all are rejected.  0.75f is exact as well; 0.6f lies above 3/5, so its ties (15, 25), ... are ACCEPTED:
    for the sweep's other ratios the rule is compared with the float32 product itself."""
    ties = []
    for num, den, r in ((9, 10, 0.9), (3, 5, 0.6), (3, 4, 0.75)):
        for d1 in range(0, 50):
            for d2 in range(0, 257):
                exact = Fraction(d1) < Fraction(num, den) * d2
                in_float = bool(np.float32(d1) < np.float32(np.float32(r) * np.float32(d2)))
                assert BS.rule_accept(d1, d2, r) == in_float, (r, d1, d2)
                if r != 0.6:
                    assert in_float == exact, (r, d1, d2)
                if r == 0.9 and d1 > 0 and Fraction(d1) == Fraction(num, den) * d2:
                    ties.append((d1, d2))
    assert BS.rule_accept(15, 25, 0.6) and not BS.rule_accept(15, 20, 0.75)
    assert ties == [(9, 10), (18, 20), (27, 30), (36, 40), (45, 50)]
    for d2 in (50, 100, 256):  # TH_LOW is strict whatever the second best
        assert BS.rule_accept(49, 256, 0.9) and not BS.rule_accept(50, 256, 0.9) and not BS.rule_accept(50, d2, 1.5)


def test_taken_case_depends_on_the_list_order():
    """The same idx1 placed first in the list matches differently: the case proves that vbMatched2 is honoured in list order."""
    a, b = CASES["taken candidate: list order 0, 1"], CASES["taken candidate: list order 1, 0"]
    assert a[1] != b[1]
    (_, ta), (_, tb) = BS.restate(a[0], with_traces=True), BS.restate(b[0], with_traces=True)
    assert ta[0].tolist() == [2, 0, 0, 1, 0] and tb[0].tolist() == [2, 0, 0, 1, 0]  # one idx1 each whose outcome a taken candidate changed


def test_traces_count_what_they_say():
    _, t = BS.restate(CASES["ratio ties rejected, neighbours accepted"][0], with_traces=True)
    assert t[0].tolist() == [2, 0, 5, 0, 0]
    _, t = BS.restate(CASES["TH_LOW: 49 accepted, 50 rejected, single 49 accepted"][0], with_traces=True)
    assert t[0].tolist() == [2, 1, 0, 0, 0]
    _, t = BS.restate(CASES["orientation: 0.1 rule cuts second and third"][0], with_traces=True)
    assert t[0].tolist() == [25, 0, 0, 0, 4]
    _, t = BS.restate(CASES["complement pair: no usable candidate"][0], with_traces=True)
    assert t[0].tolist() == [0, 1, 0, 0, 0]


def test_sweep_rule_equals_restatement_and_every_branch_is_taken():
    probs, want, traces = BS.sweep()
    assert len(probs) == 300 and len(traces) == sum(len(p["kf2"]) for p in probs)
    total = dict(zip(BS.TRACES, traces.sum(0).tolist()))
    assert all(v > 0 for v in total.values()), total
    assert {len(p["kf2"]) for p in probs} == set(range(1, 12)) and {bool(p["check_orientation"]) for p in probs} == {True, False}
    assert {float(p["nn_ratio"]) for p in probs} == {float(np.float32(r)) for r in BS.RATIOS}
    assert max(len(p["kf1"]["angle"]) for p in probs) <= 256 and max(len(p["kf1"]["node_id"]) for p in probs) <= 40
    got = BS.rule_host(probs)
    for b, (g, w) in enumerate(zip(got, want)):
        BS.assert_equal(g, w, b)
    for p, w in zip(probs, want):  # invariants of any result
        for k2, o in zip(p["kf2"], w):
            m = o["match12"]
            hit = m[m >= 0]
            assert len(set(hit.tolist())) == len(hit) == o["n_matches"]
            assert p["kf1"]["has_mp"][m >= 0].all() and k2["has_mp"][hit].all()


def test_unshuffled_lists_and_shuffled_lists_differ_somewhere():
    """The list order matters in the random problems too (equal distances, taken candidates): the same key frames with ascending
    lists give other matches in at least one slot of the sweep's first problems."""
    differ = 0
    for s in range(40):
        p = BS.sweep_problem(s)
        q = dict(p, kf1=_ascending(p["kf1"]), kf2=[_ascending(k) for k in p["kf2"]])
        differ += any(a["match12"].tobytes() != b["match12"].tobytes() for a, b in zip(BS.restate(p), BS.restate(q)))
    assert differ > 0


def _ascending(k):
    feat = k["feat_idx"].copy()
    for a, b in zip(k["node_start"][:-1], k["node_start"][1:]):
        feat[a:b] = np.sort(feat[a:b])
    return dict(k, feat_idx=feat)
