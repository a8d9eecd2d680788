"""CPU tests of the oracle's scripted LocalBundleAdjustment (oracle/lba_oracle.cpp: gfso_lba_solve_scripted) and of the windows the GPU
stop-flag tests use (tests/lba_stop_support.py): the script must say exactly what a stop at each look leaves, because
tests/test_gpu_lba_stop.py holds the GPU to it."""
import numpy as np
import pytest

import lba_stop_support as S

OUT = ("pose_q", "pose_t", "points", "edge_chi2", "edge_depth_positive")


def _same(a, b, keys=OUT + ("iterations_run", "final_chi2", "final_lambda")):
    return all(np.array_equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize("name", list(S.WINDOWS))
def test_window_is_well_conditioned(oracle, name):
    """(i) - (iii) of lba_stop_support's docstring, and the recorded trial sequence"""
    seq, min_rho, sens, same_sequence = S.check_window(oracle, S.window(name))
    print(name, S.window(name)["n_edges"], seq, f"min|rho| = {min_rho:.3g}, edge-order sensitivity = {sens:.2g}")
    assert seq == S.WINDOWS[name][5]
    assert "R" in seq, "the window rejects no trial"
    assert same_sequence
    assert sens <= 1e-8
    assert min_rho >= 1e-3


@pytest.mark.parametrize("name", list(S.WINDOWS))
def test_number_of_looks(oracle, name):
    """2 (the entry check, the top of iteration 0) + the accepted iterations that are not the last + the rejections that are retried"""
    r, tr = S.scripted(oracle, name)
    it, acc = tr["iteration"], tr["accepted"]
    n_iterations = len(set(it.tolist()))
    assert n_iterations == r["iterations_run"]
    retried = sum(1 for k in range(len(it) - 1) if it[k + 1] == it[k])
    assert all(acc[k] == 0 for k in range(len(it) - 1) if it[k + 1] == it[k])
    assert tr["looks"] == 2 + (n_iterations - 1) + retried
    assert tr["looks"] == len(S.looks_of(oracle, name))


@pytest.mark.parametrize("name", list(S.WINDOWS))
def test_script_past_the_last_look_is_the_unscripted_solve(oracle, name):
    w = S.window(name)
    ref = oracle.lba_solve(w)
    r, tr = S.scripted(oracle, name)
    assert _same(r, ref)
    for extra in (0, 1, 50):
        rs, trs = oracle.lba_solve_scripted(w, stop_at_look=tr["looks"] + extra)
        assert _same(rs, ref) and trs["looks"] == tr["looks"], extra
    rc, trc = oracle.lba_solve_scripted(w, close_at_trial=len(tr["accepted"]))
    assert _same(rc, ref) and S.sequence(trc) == S.sequence(tr)


@pytest.mark.parametrize("name", list(S.WINDOWS))
def test_stop_at_every_look(oracle, name):
    w = S.window(name)
    looks = S.looks_of(oracle, name)
    at_top = None  # the stop at the last accept-look
    for look, (kind, k) in enumerate(looks):
        r, tr = S.scripted(oracle, name, stop_at_look=look)
        assert tr["looks"] == look + 1
        if kind == "entry":  # src/Optimizer.cc:1955-1956: returns before optimising
            assert r is None and len(tr["accepted"]) == 0
            continue
        if kind == "top":  # k iterations are complete: optimize(k), byte for byte
            ref = oracle.lba_solve(dict(w, iterations=k))
            assert r["iterations_run"] == k
            if k == 0:  # (optimize(0) of the oracle evaluates the errors for its callers; a stopped optimize(10) evaluates nothing)
                assert _same(r, ref, ("pose_q", "pose_t", "points", "iterations_run"))
                assert not r["edge_chi2"].any()
            else:
                assert _same(r, ref), (look, k)
            at_top, top_k = r, k
            continue
        # after the j-th consecutive rejected trial of iteration top_k: the estimates of the preceding top, the iteration counted,
        # lambda grown by 2 * 4 * ... * 2^j = 2^(j (j + 1) / 2) (_currentLambda *= _ni; _ni *= 2; _ni = 2 on accept), the edges with
        # the rejected trial's errors
        j = k
        assert _same(r, at_top, ("pose_q", "pose_t", "points", "edge_depth_positive"))
        assert r["iterations_run"] == top_k + 1
        if top_k > 0:  # lambda / chi2 at the top of iteration top_k: what optimize(top_k) left ...
            assert r["final_chi2"] == at_top["final_chi2"]
            assert r["final_lambda"] == at_top["final_lambda"] * 2.0 ** (j * (j + 1) // 2)
        else:  # ... or, before any iteration, computeLambdaInit's value: the first rejection doubles it, and so on
            r1, _ = S.scripted(oracle, name, stop_at_look=look - j + 1)
            assert r["final_lambda"] == r1["final_lambda"] * 2.0 ** (j * (j + 1) // 2 - 1)
            assert r["final_chi2"] == r1["final_chi2"]
        assert not np.array_equal(r["edge_chi2"], at_top["edge_chi2"])
        assert tr["accepted"][-1] == 0 and tr["rho"][-1] < 0


@pytest.mark.parametrize("name", list(S.WINDOWS))
def test_close_at_every_trial(oracle, name):
    """the batched entry's rule: trial r + 1 is evaluated and dropped -- the estimates, lambda and chi2 of the r trials before it, the
    iteration counted, the dropped trial's errors on the edges"""
    w = S.window(name)
    full, tr = S.scripted(oracle, name)
    looks = S.looks_of(oracle, name)
    n = len(tr["accepted"])
    for r_ in range(n):
        c, trc = S.scripted(oracle, name, close_at_trial=r_)
        assert S.sequence(trc) == S.sequence(tr)[:r_] + "C"
        # the stop at the look that precedes trial r_ saw the same state: look 1 + r_ (one look in front of every trial)
        kind, k = looks[1 + r_]
        s, _ = S.scripted(oracle, name, stop_at_look=1 + r_)
        assert _same(c, s, ("pose_q", "pose_t", "points", "edge_depth_positive"))
        assert c["iterations_run"] == int(tr["iteration"][r_]) + 1
        if r_ > 0:
            assert c["final_lambda"] == s["final_lambda"]
            assert c["final_chi2"] == s["final_chi2"]
        assert not np.array_equal(c["edge_chi2"], s["edge_chi2"])


def test_lidar_restatement_takes_the_same_script(oracle):
    """tests/host/lba_lidar_restatement.cpp carries its own copy of the LM loop: without lidar edges it must be the oracle under the
    same stop_at_look, byte for byte, at every look of a window that rejects"""
    import lba_lidar_support as LLS
    name = "s9_6x300_rrr"
    w = S.window(name)
    n = len(S.looks_of(oracle, name))
    for look in list(range(n + 1)) + [-1]:
        ro, tr = S.scripted(oracle, name, stop_at_look=look)
        r, _ = LLS.solve(w, lidar=False, stop_at_look=look)
        assert (r is None) == (ro is None) == (look == 0)
        if r is not None:
            assert _same(r, ro), look
            assert r["looks"] == tr["looks"], look
