"""The CPU restatement of the Sim3 searches of loop closing (tests/host/sim3_search_restatement.cpp) against an independent
numpy.float32 statement of DESIGN.md section 20, bit for bit, on random problems over the three modes and on constructed points that
sit exactly on each decision.  First of all the restatement's own output is checked for taking every path: a checker that never
leaves through an exit, never meets a taken key-point and never sees a tie checks nothing there.  No GPU."""
import numpy as np
import pytest

import sim3_search_support as SS
from geoflowslam_amd import synth

SEEDS = range(30)


def _random(seed):
    mode = SS.MODES[seed % 3]
    sf = 1.1 if seed % 4 == 3 else 1.2
    th, ratio = ((4.0, 1.0), (3.0, 1.5), (8.0, 1.5), (5.0, 1.0))[(seed // 3) % 4] if mode else ((4.0, 3.0, 1.5)[(seed // 3) % 3], 1.0)
    return synth.sim3_search_problem(seed, mode, n_points=120 + 7 * seed, n_kp=150 + 11 * seed, n_problems=1 + seed % 2, scale_factor=sf,
                                     th=th, ratio_hamming=ratio, masks=seed % 5 != 4)


@pytest.mark.parametrize("mode", SS.MODES, ids=[SS.MODE_NAMES[m] for m in SS.MODES])
def test_restatement_takes_every_path(mode):
    """On the restatement's own output, for the shared problems with n_mp >= 255 and n_kp = 500: every exit occurs, Hamming ties
    occur, and in the projection modes taken key-points are met and at least one matched point's key-point is not the one it would
    get with an empty taken set -- nor the one the entry's taken set alone would leave it: an earlier point of the list took that."""
    exits, stats = np.zeros(9, np.int64), dict.fromkeys(SS.STATS, 0)
    for n_mp in (255, 256, 257, 1000):
        prob, out, st = SS.problem(mode, n_mp, 500)
        exits += np.bincount(out[0]["exit"], minlength=9)
        for k in SS.STATS:
            stats[k] += st[k]
    assert (exits > 0).all(), dict(zip(SS.EXITS, exits))
    assert stats["ties"] > 0 and stats["ties_other_cell"] > 0, stats
    if mode != SS.FUSE:
        assert stats["taken_skips"] > 0 and stats["displaced"] > 0 and stats["displaced_by_earlier"] > 0, stats
    # the largest problem takes every exit and shows the dependency by itself
    prob, out, st = SS.problem(mode, 1000, 500)
    assert (np.bincount(out[0]["exit"], minlength=9) > 0).all() and (mode == SS.FUSE or st["displaced_by_earlier"] > 0)


@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_equals_numpy_statement(seed):
    prob = _random(seed)
    SS.assert_equal(SS.restate(prob), SS.numpy_statement(prob), seed)


def test_shared_problems_equal_numpy_statement():
    for prob, want in (SS.five_problems(), SS.two_lists(), SS.problem(SS.SBP, 257, 500)[:2], SS.problem(SS.SBP_KFS, 65, 1)[:2],
                       SS.problem(SS.FUSE, 64, 0)[:2], SS.problem(SS.SBP, 0, 500)[:2]):
        SS.assert_equal(want, SS.numpy_statement(prob))


def test_modes_differ_where_they_should():
    """One scene under the three modes: Fuse ignores the taken state, so it matches points the projection searches cannot; the two
    projection forms agree on almost every point (the exits may differ only through one more rounding)."""
    a = synth.sim3_search_problem(5, SS.SBP, n_points=600, n_kp=500, th=4.0, ratio_hamming=1.0)
    as_fuse = dict(lists=a["lists"], problems=[dict(a["problems"][0], mode=SS.FUSE, kp_taken=None)])
    as_kfs = dict(lists=a["lists"], problems=[dict(a["problems"][0], mode=SS.SBP_KFS)])
    o, of, ok = SS.restate(a)[0], SS.restate(as_fuse)[0], SS.restate(as_kfs)[0]
    assert of["n_matched"] > o["n_matched"] > 0
    assert (o["exit"] != ok["exit"]).mean() < 0.02


def test_constructed_points():
    prob, labels, extra = SS.constructed()
    assert extra["u_pinhole"] != extra["u_invz"]
    out = SS.restate(prob)
    SS.check_constructed(prob, labels, out)
    ns = SS.numpy_statement(prob)
    SS.check_constructed(prob, labels, ns)
    SS.assert_equal(out, ns, "constructed")
    # the chain is longer than what the device lists per point
    assert (1, "chain%d" % (SS.LISTED + 2)) in labels and labels[(1, "chain%d" % (SS.LISTED + 1))][2] == SS.MATCHED
