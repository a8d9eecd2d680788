"""The CPU restatement of the ORBmatcher::Fuse search (tests/host/fuse_restatement.cpp) against an independent numpy.float32
statement of DESIGN.md section 13, bit for bit, on random problems and on constructed points that sit exactly on each decision.
No GPU."""
import numpy as np
import pytest

import fuse_support as FS
from geoflowslam_amd import synth

SEEDS = range(32)


def _random(seed):
    sf = 1.1 if seed % 4 == 3 else 1.2
    return synth.fuse_problem(seed, n_points=120 + 7 * seed, n_kp=150 + 11 * seed, n_keyframes=1 + seed % 3, scale_factor=sf,
                              th=(3.0, 5.0, 1.5)[seed % 3])


def test_random_problems_take_every_path():
    """On the restatement's own output: every exit occurs, both branches of the chi2 gate accept and reject, Hamming ties occur
    (some across cells).  A checker that never leaves through an exit checks nothing there."""
    exits, stats = np.zeros(8, np.int64), dict.fromkeys(FS.STATS, 0)
    for seed in SEEDS:
        out, st = FS.restate(_random(seed), with_stats=True)
        for o in out:
            exits += np.bincount(o["exit"], minlength=8)
        for k in FS.STATS:
            stats[k] += st[k]
    assert (exits > 0).all(), dict(zip(FS.EXITS, exits))
    assert 0 < stats["stereo_rejected"] < stats["stereo"] and 0 < stats["mono_rejected"] < stats["mono"], stats
    assert stats["ties"] > 0 and stats["ties_other_cell"] > 0, stats
    # one problem of the generator's default kind takes every exit by itself
    prob, out = FS.problem(1000, 500)
    assert (np.bincount(out[0]["exit"], minlength=8) > 0).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_equals_numpy_statement(seed):
    prob = _random(seed)
    FS.assert_equal(FS.restate(prob), FS.numpy_statement(prob), seed)


def test_shared_problems_equal_numpy_statement():
    for prob, want in (FS.five_keyframes(), FS.two_lists(), FS.problem(257, 500), FS.problem(65, 1), FS.problem(64, 0), FS.problem(0, 500)):
        FS.assert_equal(want, FS.numpy_statement(prob))


def test_constructed_points():
    prob, labels = FS.constructed()
    out = FS.restate(prob)
    FS.check_constructed(prob, labels, out)
    ns = FS.numpy_statement(prob)
    FS.check_constructed(prob, labels, ns)
    FS.assert_equal(out, ns, "constructed")
    # the constants around which the chi2 points are built straddle the gates
    for c in (5.99, 7.8):
        lo, hi = FS.around(c)
        assert float(lo) <= c < float(hi) and np.nextafter(lo, np.float32(np.inf)) == hi
