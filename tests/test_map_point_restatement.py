"""The sequential CPU restatement of the map-point update (tests/host/map_point_restatement.cpp) against an independent numpy
statement of DESIGN.md section 15, bit for bit, on 32 random problems and the constructed points; first that the inputs exercise the
rule at all.  No GPU."""
import numpy as np
import pytest

import map_point_support as MS


@pytest.fixture(scope="module")
def problems():
    probs = [MS.random_problem(seed) for seed in range(32)]
    return probs, [MS.restate(p, with_ties=True) for p in probs]


def test_inputs_exercise_the_rule(problems):
    probs, outs = problems
    n3 = tied = moved = flags_differ = no_desc = empty = long_lists = 0
    for prob, (out, ties) in zip(probs, outs):
        start, fl = prob["obs_start"], prob["obs_flags"]
        for p in range(len(start) - 1):
            f = fl[start[p]:start[p + 1]]
            nd = int(((f & 2) != 0).sum())
            empty += len(f) == 0
            no_desc += len(f) > 0 and nd == 0
            flags_differ += bool((((f & 1) != 0) != ((f & 2) != 0)).any())
            long_lists += nd > 64
            if nd >= 3:
                n3 += 1
                tied += ties[p] > 1
                first = int(np.nonzero(f & 2)[0][0])
                moved += out["best_obs"][p] != first
    assert n3 > 400, n3
    assert tied >= n3 / 4, (tied, n3)    # several rows share the best median
    assert moved >= n3 / 4, (moved, n3)  # the best row is not the first
    assert flags_differ > 50 and no_desc > 20 and empty > 10 and long_lists > 50, (flags_differ, no_desc, empty, long_lists)


def test_restatement_equals_numpy_statement(problems):
    probs, outs = problems
    for seed, (prob, (out, _)) in enumerate(zip(probs, outs)):
        MS.assert_equal(out, MS.numpy_statement(prob), ("seed", seed))


def test_normals_only_mode(problems):
    probs, outs = problems
    for seed in (0, 1, 2):
        got = MS.restate(probs[seed], normals_only=True)
        MS.assert_equal(got, outs[seed][0], ("seed", seed), MS.NORMAL_FIELDS)
        MS.assert_equal(got, MS.numpy_statement(probs[seed], normals_only=True), ("seed", seed))
        assert (got["best_obs"] == -1).all() and (got["best_median"] == -1).all() and not (got["status"] & 2).any()


def test_constructed_points():
    prob, labels = MS.constructed()
    out = MS.restate(prob)
    MS.check_constructed(prob, labels, out)
    MS.assert_equal(out, MS.numpy_statement(prob), "constructed")
