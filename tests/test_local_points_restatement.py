"""The CPU restatement of Tracking::SearchLocalPoints' second loop (tests/host/local_points_restatement.cpp: Frame::isInFrustum,
MapPoint::PredictScale on the host's logf, the far-points filter, oracle/sbp_oracle.cpp's search on the compacted list) against an
independent numpy.float32 statement of DESIGN.md section 12, bit for bit -- after the conditions on the inputs: the frames the
CPU and GPU tests share take every exit of the rule.  No GPU."""
import numpy as np
import pytest

import local_points_support as LPS


def test_input_conditions():
    """Asserted on the restatement's output alone, before anything is compared with it."""
    frames = LPS.all_frames()
    exits = np.zeros(len(LPS.EXITS), np.int64)
    far_removed = low = high = 0
    for name, (prob, r) in frames:
        n = len(prob["mp_xw"])
        if n:
            exits += np.bincount(r["exits"], minlength=len(LPS.EXITS))
        v = r["in_view"] != 0
        assert r["n_to_match"] == int(v.sum()), name
        far_removed += r["n_to_match"] - r["n_searched"]
        low += int((r["raw_level"][v] < 0).sum())
        high += int((r["raw_level"][v] >= prob["n_levels"]).sum())
        if n >= LPS.MAIN_MIN:
            assert 0.2 <= v.mean() <= 0.8, (name, v.mean())
        if len(prob["cur_kps_un"]) and n:
            assert r["nmatches"] > 0, name
        if n >= LPS.MAIN_MIN:  # the clamped levels are really delivered as 0 / n_levels - 1
            assert (r["level"][v][r["raw_level"][v] >= prob["n_levels"]] == prob["n_levels"] - 1).all()
            assert (r["level"][v][r["raw_level"][v] < 0] == 0).all()
    for k, name in enumerate(LPS.EXITS):
        if name != "not_finite":  # (0 / 0 needs a constructed point: test_constructed_points)
            assert exits[k] > 0, name
    assert far_removed > 0 and low > 0 and high > 0, (far_removed, low, high)


@pytest.mark.parametrize("which", range(len(LPS.CASES) + 3))
def test_restatement_equals_numpy_statement(which, oracle):
    name, (prob, r) = LPS.all_frames()[which]
    q = LPS.numpy_statement(prob)
    assert LPS.same_bits(r["in_view"], q["in_view"]) and r["n_to_match"] == q["n_to_match"], name
    assert LPS.same_bits(r["proj"][:, :2], q["proj"][:, :2]), name
    v = q["in_view"] != 0
    for k in ("proj", "depth", "view_cos", "level"):
        assert LPS.same_bits(r[k][v], q[k][v]), (name, k)
    assert LPS.same_bits(r["index"], q["index"]) and r["n_searched"] == len(q["index"]), name
    # the matches: the oracle's map search fed with the numpy statement's compacted fields, mapped back through its index list
    cm, nm = oracle.search_by_projection_map(LPS.compacted(prob, q, q["index"]))
    assert nm == r["nmatches"], name
    assert LPS.same_bits(LPS.map_back(cm, q["index"]), r["cur_match"]), name


def test_constructed_points(oracle):
    for name, prob, labels in LPS.constructed_frames():
        r, q = LPS.restate(prob), LPS.numpy_statement(prob)
        LPS.check_constructed(name, prob, labels, r, r["index"])
        LPS.check_constructed(name, prob, labels, q, q["index"])
        v = q["in_view"] != 0
        assert LPS.same_bits(r["in_view"], q["in_view"]) and LPS.same_bits(r["proj"][:, :2], q["proj"][:, :2]), name
        for k in ("proj", "depth", "view_cos", "level"):
            assert LPS.same_bits(r[k][v], q[k][v]), (name, k)
        assert LPS.same_bits(r["index"], q["index"]), name
        cm, nm = oracle.search_by_projection_map(LPS.compacted(prob, q, q["index"]))
        assert nm == r["nmatches"] and LPS.same_bits(LPS.map_back(cm, q["index"]), r["cur_match"]), name
    # every level boundary really decides: 1.2f^k and its upper neighbour land on different levels somewhere
    name, prob, labels = LPS.constructed_frames()[0]
    r = LPS.restate(prob)
    lv = {l: int(r["raw_level"][i]) for l, (i, _, _) in labels.items() if l.startswith("ratio=")}
    assert sorted(set(lv.values())) == list(range(0, 10)), lv
