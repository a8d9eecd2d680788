"""The sequential restatement of Optimizer::OptimizeSim3 (tests/host/sim3_opt_restatement.cpp; reference src/Optimizer.cc:2797-3054):
its inputs reach the branches the GPU tests rely on, one linearisation equals an independent statement bit for bit, and float64 and
long double agree on the flags of the free-scale cases the device is compared on.  CPU only."""
import math

import numpy as np
import pytest

import sim3_opt_support as S
from geoflowslam_amd import api, synth


@pytest.fixture(scope="module")
def cases():
    return S.constructed_cases()


@pytest.fixture(scope="module")
def runs(cases):
    return {k: S.run(p) for k, p in cases.items() if isinstance(p, dict)}


def test_constants():
    assert S.constants() == dict(first_iterations=5, more_iterations_after_removal=10, more_iterations=5, min_correspondences=10,
                                 numeric_delta=1e-9)


def test_more_iterations_depend_on_a_removal(cases, runs):
    """nBad == 0 allows 5 more iterations, nBad > 0 allows 10: a second phase that the iterations alone stop, after each count."""
    a, b = runs["no_removal"], runs["removal"]
    assert a["n_bad"] == 0 and a["status"] == api.SIM3_OPT_BOTH_PHASES and a["iterations_run"][1] <= 5
    assert b["n_bad"] > 0 and b["status"] == api.SIM3_OPT_BOTH_PHASES and b["iterations_run"][1] <= 10
    five, ten = runs["five_more"], runs["ten_more"]
    assert five["n_bad"] == 0 and five["iterations_run"][1] == 5 and five["trace"]["end_reason"][1] == S.END_ITERATIONS
    assert ten["n_bad"] > 0 and ten["iterations_run"][1] == 10 and ten["trace"]["end_reason"][1] == S.END_ITERATIONS


def test_early_return_at_nine_and_not_at_ten(cases, runs):
    nine, ten = runs["nine_left"], runs["ten_left"]
    assert len(cases["nine_left"]["x1c"]) - nine["n_bad"] == 9 and nine["status"] == api.SIM3_OPT_EARLY_RETURN
    assert nine["ret"] == 0 and nine["n_in"] == 0 and nine["iterations_run"][1] == 0
    assert nine["s12"].tobytes() == np.asarray(cases["nine_left"]["s12"], np.float64).tobytes(), "g2oS12 untouched"
    assert (nine["pair_state"] != api.SIM3_PAIR_REMOVED_FINAL).all() and (nine["pair_state"] == 1).sum() == nine["n_bad"]
    assert len(cases["ten_left"]["x1c"]) - ten["n_bad"] == 10 and ten["status"] == api.SIM3_OPT_BOTH_PHASES and ten["n_in"] == ten["ret"] > 0
    assert ten["s12"].tobytes() != np.asarray(cases["ten_left"]["s12"], np.float64).tobytes()


def test_no_pairs_is_the_early_return():
    p = S.sized_problem(0, False)
    r = S.run(p)
    assert (r["status"], r["n_in"], r["n_bad"], r["iterations_run"]) == (0, 0, 0, (0, 0)) and r["s12"].tobytes() == p["s12"].tobytes()


def test_pair_removed_by_the_final_check_alone(runs):
    r = runs["final_only"]
    assert (r["pair_state"] == api.SIM3_PAIR_REMOVED_FINAL).sum() >= 1
    assert r["n_in"] == (r["pair_state"] == 0).sum() and r["n_bad"] == (r["pair_state"] == 1).sum()


def test_phase_endings_and_rejected_trials(runs):
    assert S.END_QMAX in runs["ends_qmax"]["trace"]["end_reason"]
    assert S.END_NBAD in runs["ends_nbad"]["trace"]["end_reason"]
    assert sum(runs["rejected_trial"]["trace"]["rejected_trials"]) > 0
    assert all(sum(r["trace"]["failed_solves"]) == 0 for k, r in runs.items() if k not in S.DEGENERATE_CASES)
    assert set(S.DEGENERATE_CASES) <= set(runs)


def test_failed_solves_apply_the_x_the_solver_kept(cases, runs):
    """The solver's x outlives a failed solve and both optimize() calls (OptimizeSim3 quirks, item 7): each case reaches the
    part of it that it is named for."""
    t = runs["failed_first_solve"]["trace"]
    assert min(t["failed_solves"]) > 0 and t["stale_x_applied"] == (0, 0) and t["failed_after_success"] == (0, 0), "x stays 0"
    assert runs["failed_first_solve"]["s12"].tobytes() == np.asarray(cases["failed_first_solve"]["s12"], np.float64).tobytes()
    assert t["final_lambda"] == (0.0, 0.0)
    t = runs["failed_after_success"]["trace"]
    assert t["stale_x_applied"][0] > 0 and t["failed_after_success"][0] == 1
    r = runs["failed_across_phases"]
    t = r["trace"]
    # failed_solves[1] > 0 with no failure after a success: the second optimize()'s first solve failed, and what it applied is the
    # x of the first optimize()
    assert t["failed_solves"][0] == 0 and r["iterations_run"][0] > 0 and t["failed_solves"][1] > 0 and t["failed_after_success"][1] == 0
    assert t["stale_x_applied"][1] == t["failed_solves"][1] > 0
    for k in ("failed_first_solve", "failed_after_success", "failed_across_phases"):
        assert runs[k]["status"] == api.SIM3_OPT_BOTH_PHASES and np.isfinite(runs[k]["s12"]).all() and np.isfinite(runs[k]["chi2"]).all(), k


def test_non_finite_pairs_reach_both_checks(cases, runs):
    """`chi2 > th2` is false for a NaN: a pair whose chi2 is NaN is removed only through its other edge.  The NaN is once at an even
    lane's first register edge of the kernel and once beyond the fourth (tests/sim3_opt_support.py)."""
    for name, k in S.NAN_PAIR.items():
        r, n = runs[name], len(cases[name]["x1c"])
        assert (n, 2 * k < 256, 2 * k >= 1024) in ((40, True, False), (600, False, True))
        assert np.isnan(r["chi2"][k, 0]) and r["pair_state"][k] == api.SIM3_PAIR_INLIER and r["status"] == api.SIM3_OPT_BOTH_PHASES
        # in the graph in the second phase: every one of its solves fails on a NaN system, and the pair is counted an inlier
        assert r["trace"]["failed_solves"][1] == r["iterations_run"][1] > 0 and r["trace"]["failed_solves"][0] == 5
        assert r["n_in"] == (r["pair_state"] == 0).sum() and np.isnan(r["chi2"]).any(1).sum() == 1
        assert r["s12"].tobytes() == np.asarray(cases[name]["s12"], np.float64).tobytes(), "no trial was kept"
    for name, pair in (("nan_observation", 3), ("nan_point", 7)):  # removed through the pair's other edge; the NaN chi2 is reported
        r = runs[name]
        assert np.isnan(r["chi2"][pair]).any() and r["pair_state"][pair] == api.SIM3_PAIR_REMOVED_FIRST
        assert r["trace"]["failed_solves"] == (5, 0) and r["status"] == api.SIM3_OPT_BOTH_PHASES and np.isfinite(r["s12"]).all()
    r = runs["inf_observation"]
    assert np.isinf(r["chi2"][5, 1]) and r["pair_state"][5] == api.SIM3_PAIR_REMOVED_FIRST and r["trace"]["failed_solves"] == (5, 0)
    r = runs["z_zero"]  # a division by z = 0: an infinite error, and a first phase that goes far enough astray for the early return
    assert r["status"] == api.SIM3_OPT_EARLY_RETURN and r["pair_state"][6] == api.SIM3_PAIR_REMOVED_FIRST and sum(r["trace"]["failed_solves"]) == 0
    for name, pair in (("behind_camera", 6), ("huge_observation", 2)):
        r = runs[name]
        assert r["status"] == api.SIM3_OPT_BOTH_PHASES and r["pair_state"][pair] == api.SIM3_PAIR_REMOVED_FIRST and np.isfinite(r["s12"]).all()
        assert sum(r["trace"]["failed_solves"]) == 0
    assert runs["huge_observation"]["chi2"][2, 0] > 1e300
    r = runs["fewer_than_ten_after_nan"]  # the NaN pair is one of the nine that are left
    assert r["status"] == api.SIM3_OPT_EARLY_RETURN and len(cases["fewer_than_ten_after_nan"]["x1c"]) - r["n_bad"] == 9
    assert r["pair_state"][2] == api.SIM3_PAIR_INLIER and np.isnan(r["chi2"][2, 0]) and r["iterations_run"] == (5, 0)


def test_first_check_reads_stale_errors(cases, runs):
    """The first optimize() ended on a rejected trial; the edges keep that trial's errors, and here a pair's flag depends on it:
    recomputing the errors in front of the first check (what the final check does) would flag it differently."""
    t = runs["stale"]["trace"]
    assert t["last_trial_rejected"][0] == 1 and t["end_reason"][0] in (S.END_QMAX, S.END_RHO_ZERO)
    assert t["stale_largest_difference"] > 0 and t["stale_flag_differences"] >= 1
    # and where every trial of the last iteration was accepted there is nothing stale
    assert runs["removal"]["trace"]["last_trial_rejected"][0] == 0 and runs["removal"]["trace"]["stale_largest_difference"] == 0


def test_chi2_on_each_side_of_th2_within_a_few_ulps(cases, runs):
    k = cases["tie_pair"]
    th2 = np.float64(np.float32(cases["tie_below"]["th2"]))
    below, above = runs["tie_below"], runs["tie_above"]
    assert 0 <= th2 - below["chi2"][k, 0] <= 4 * np.spacing(th2) and below["pair_state"][k] == api.SIM3_PAIR_INLIER  # `>`: a tie stays
    assert 0 < above["chi2"][k, 0] - th2 <= 4 * np.spacing(th2) and above["pair_state"][k] != api.SIM3_PAIR_INLIER
    assert below["n_in"] == above["n_in"] + 1


def test_fixed_scale_keeps_the_scale_and_a_zero_column():
    p = S.sized_problem(65, True)
    r = S.run(p)
    assert r["s12"][7] == p["s12"][7]
    _, J, H, b, _ = S.linearize(p, True)
    assert (J[:, :, 6] == 0).all() and (H[6] == 0).all() and (H[:, 6] == 0).all() and b[6] == 0
    pf = S.sized_problem(65, True, fix_scale=False)
    _, Jf, Hf, _, _ = S.linearize(pf, True)
    assert (Jf[:, :, 6] != 0).any() and Hf[6, 6] > 0


# ---- an independent statement of one linearisation in Python floats (IEEE double, no contraction; math.exp is libm's)

def _rotate(q, v):
    ux, uy, uz = 2 * (q[1] * v[2] - q[2] * v[1]), 2 * (q[2] * v[0] - q[0] * v[2]), 2 * (q[0] * v[1] - q[1] * v[0])
    return [v[0] + q[3] * ux + (q[1] * uz - q[2] * uy), v[1] + q[3] * uy + (q[2] * ux - q[0] * uz), v[2] + q[3] * uz + (q[0] * uy - q[1] * ux)]


def _exp_small(u):
    """Sim3(update) for |omega| < 1e-5 (sim3.h:70-142): the only branch a 1e-9 perturbation takes."""
    om, ups, sigma = u[:3], u[3:6], u[6]
    assert math.sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]) < 0.00001
    O = [0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0]
    O2 = [O[3 * r] * O[c] + O[3 * r + 1] * O[3 + c] + O[3 * r + 2] * O[6 + c] for r in range(3) for c in range(3)]
    s = math.exp(sigma)
    if abs(sigma) < 0.00001:
        A, B, Cc = 1. / 2., 1. / 6., 1.0
    else:
        sigma2 = sigma * sigma
        Cc, A, B = (s - 1) / sigma, ((sigma - 1) * s + 1) / sigma2, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
    eye = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    R = [eye[i] + O[i] + O2[i] for i in range(9)]
    t = R[0] + R[4] + R[8]
    assert t > 0
    t = math.sqrt(t + 1.0)
    w = 0.5 * t
    t = 0.5 / t
    q = [(R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t, w]
    W = [A * O[i] + B * O2[i] + Cc * eye[i] for i in range(9)]
    return q, [W[3 * r] * ups[0] + W[3 * r + 1] * ups[1] + W[3 * r + 2] * ups[2] for r in range(3)], s


def _mul(a, b):
    p, q = a[0], b[0]
    qq = [p[3] * q[0] + p[0] * q[3] + p[1] * q[2] - p[2] * q[1], p[3] * q[1] + p[1] * q[3] + p[2] * q[0] - p[0] * q[2],
          p[3] * q[2] + p[2] * q[3] + p[0] * q[1] - p[1] * q[0], p[3] * q[3] - p[0] * q[0] - p[1] * q[1] - p[2] * q[2]]
    rt = _rotate(p, b[1])
    return qq, [a[2] * rt[i] + a[1][i] for i in range(3)], a[2] * b[2]


def _inverse(a):
    q = [-a[0][0], -a[0][1], -a[0][2], a[0][3]]
    k = -1. / a[2]
    return q, _rotate(q, [k * a[1][0], k * a[1][1], k * a[1][2]]), 1. / a[2]


def _error(Sx, X, cam, obs):
    r = _rotate(Sx[0], X)
    m = [Sx[2] * r[i] + Sx[1][i] for i in range(3)]
    return [obs[0] - (cam[0] * m[0] / m[2] + cam[2]), obs[1] - (cam[1] * m[1] / m[2] + cam[3])]


@pytest.mark.parametrize("fix_scale,robust", [(True, True), (True, False), (False, True)])
def test_one_linearisation_equals_an_independent_statement_bit_for_bit(fix_scale, robust):
    p = synth.sim3_opt_problem(31, n_pairs=12, fix_scale=fix_scale, outlier_share=0.3)
    err, J, H, b, chi = S.linearize(p, robust)
    S12 = ([float(v) for v in p["s12"][:4]], [float(v) for v in p["s12"][4:7]], float(p["s12"][7]))
    delta = float(np.float32(math.sqrt(np.float32(p["th2"]))))
    dsqr = delta * delta
    Hp, bp, chip = [[0.0] * 7 for _ in range(7)], [0.0] * 7, 0.0
    for e in range(24):
        i, inv = e // 2, e % 2 == 1
        X = [float(v) for v in (p["x1c"] if inv else p["x2c"])[i]]
        obs = [float(v) for v in (p["obs2"] if inv else p["obs1"])[i]]
        cam = [float(v) for v in (p["cam2"] if inv else p["cam1"])]
        w = float((p["inv_sigma2_2"] if inv else p["inv_sigma2_1"])[i])
        at = lambda Sx: _error(_inverse(Sx) if inv else Sx, X, cam, obs)
        r = at(S12)
        assert r == list(err[e])
        c = r[0] * w * r[0] + r[1] * w * r[1]
        rho0, rho1 = (c, 1.0) if c <= dsqr or not robust else (2 * math.sqrt(c) * delta - dsqr, delta / math.sqrt(c))
        chip += rho0
        Je = [[0.0] * 7, [0.0] * 7]
        for d in range(7):
            ep, em = [at(_mul(_exp_small([(sgn * 1e-9 if k == d and not (fix_scale and k == 6) else 0.0) for k in range(7)]), S12))
                      for sgn in (1.0, -1.0)]
            for k in range(2):
                Je[k][d] = (1.0 / (2 * 1e-9)) * (ep[k] - em[k])
        assert np.array(Je).tobytes() == J[e].tobytes()
        om = [-(w * r[0]) * rho1, -(w * r[1]) * rho1] if robust else [-(w * r[0]), -(w * r[1])]
        ww = rho1 * w if robust else w
        for a in range(7):
            bp[a] += Je[0][a] * om[0] + Je[1][a] * om[1]
            for cc in range(7):
                Hp[a][cc] += (Je[0][a] * ww) * Je[0][cc] + (Je[1][a] * ww) * Je[1][cc]
    assert np.array(Hp).tobytes() == H.tobytes() and np.array(bp).tobytes() == b.tobytes() and chip == chi


def test_free_scale_cases_have_flags_that_rounding_does_not_flip():
    """The free-scale problems of tests/test_gpu_sim3_opt.py: float64 and long double agree on every flag and both iteration counts.
    Prints the float64 - long double distance of s12, the unit of the bar the device is held to there."""
    for name, p, r, dist in S.free_scale_cases():
        rl = S.run(p, long_double=True)
        print(f"{name}: |s12(float64) - s12(long double)| = {dist:.3e}, iterations {r['iterations_run']}, nIn {r['n_in']}, nBad {r['n_bad']}")
        assert S.same_flags(r, rl) and r["status"] == api.SIM3_OPT_BOTH_PHASES and dist > 0 and not p["fix_scale"]
        assert r["s12"][7] != p["s12"][7], "the scale moved"


def test_float64_long_double_distance_of_the_fixed_scale_cases(cases):
    """Recorded for every case the GPU file compares: how far double's own rounding moves s12."""
    named = [(k, p) for k, p in cases.items() if isinstance(p, dict)]
    named += [(f"n{n}_{'out' if o else 'clean'}", S.sized_problem(n, o)) for n in S.SIZES for o in (False, True)]
    for name, p in named:
        d = S.s12_distance(S.run(p), S.run(p, long_double=True))
        print(f"{name}: {d:.3e}")
        assert d < 1e-3  # both solve the same problem: no more apart than the solve's own precision allows
