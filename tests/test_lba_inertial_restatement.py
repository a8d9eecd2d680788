"""The sequential restatement of LocalInertialBA (tests/host/lba_inertial_restatement.cpp over csrc/lba_inertial_rule.hpp) on the CPU:
its first Levenberg trial against an independent numpy statement over the full, unreduced system; the branches of the Levenberg fork
on constructed windows, asserted on the trace so that the GPU test that byte-compares the same windows is known to cover them;
convergence and the erase verdicts on 20 seeded windows; the stand-alone program under the host sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import lba_inertial_support as S
from geoflowslam_amd import synth

# Relative bars (largest difference over the largest magnitude of the quantity), each about ten times the larger of
#   (a) the restatement against numpy float64 and (b) numpy float64 against numpy longdouble, measured on the four windows below
# (the largest of N = 1, 2, 3, 10; DESIGN.md section 26 has the table):
#                 (a)       (b)
#   errors        1.8e-15   6.8e-15      chi2, rho   1.8e-15   3.6e-15      H, Hll, Hpl   5.9e-16   5.7e-15
#   b, bl         5.6e-16   5.8e-15      M           2.3e-16   4.1e-16      bs            1.2e-14   1.4e-14
#   dx            1.9e-12   3.2e-13      dxl         8.9e-13   5.5e-13      state         5.5e-14   (from dx)
BARS = dict(vis_err=7e-14, small_err=7e-14, edge_rho0=4e-14, small_chi=4e-14, chi2=4e-14, H=6e-14, Hll=6e-14, Hpl_full=6e-14, b=6e-14, bl=6e-14,
            M=5e-15, bs=2e-13, dx=2e-11, dxl=1e-11, state=6e-13)


@pytest.fixture(scope="module", params=[1, 2, 3, 10])
def first_trial(request):
    N = request.param
    w = synth.lba_inertial_window(200 + N, n_opt=N, n_fixed=2, n_points=60)
    return w, S.restatement_first_trial(w), S.np_first_trial(w), S.np_first_trial(w, np.longdouble)


def test_first_trial_against_numpy(first_trial):
    w, rst, f64, ld = first_trial
    for k, bar in BARS.items():
        if k == "state":
            a, b = S.rel(rst["trial_state"], S.np_updated_state(w, f64["dx"])), 0.0
        else:
            a, b = S.rel(rst[k], f64[k]), S.rel(f64[k], ld[k])
        print(f"N={w['n_opt']} {k}: restatement vs float64 {a:.1e}, float64 vs longdouble {b:.1e}, bar {bar:.0e}")
        assert a <= bar and b <= bar, (k, a, b, bar)
    assert np.float32(rst["chi2"]) == np.float32(rst["err"]) or abs(rst["chi2"] - rst["err"]) <= 1e-6 * abs(rst["err"])  # err is the float cast


def test_the_step_solves_the_full_system(first_trial):
    """dx and the points' steps together solve (H + lambda I) x = b of the UNREDUCED system as numpy assembled it."""
    w, rst, f64, _ = first_trial
    D = 15 * w["n_opt"]
    lam = w["lambda_init"]
    top = (f64["H"] + lam * np.eye(D)) @ rst["dx"] + f64["Hpl_full"] @ rst["dxl"].ravel() - f64["b"]
    assert np.abs(top).max() <= 1e-9 * max(np.abs(f64["b"]).max(), 1.0)


def _trace(name):
    w = S.trace_cases()[name]
    return w, S.run(w, trace=True)


def test_trace_first_trial_accepted():
    w, r = _trace("first_trial_accepted")
    tr = r["trace"]
    assert S.has_first_trial_accept(r) and tr["lambda"][0] == w["lambda_init"] and tr["accepted"][0] == 1 and tr["rho"][0] > 0
    t = 2 * tr["rho"][0] - 1  # rule P: the cube by multiplication
    assert tr["lambda"][1] == w["lambda_init"] * max(1.0 / 3.0, min(1.0 - (t * t) * t, 2.0 / 3.0))


def test_trace_rejected_then_accepted():
    w, r = _trace("rejected_then_accepted")
    tr = r["trace"]
    assert S.has_reject_then_accept(r)
    it = next(i for i in range(r["iterations_run"]) if len(S.iteration_rows(tr, i)) >= 2)
    rows = S.iteration_rows(tr, it)
    assert tr["rho"][rows[0]] < 0 and tr["ok2"][rows[0]] == 1
    # _ni doubles: lambda * 2, then * 4, ...
    for q in range(1, len(rows)):
        assert tr["lambda"][rows[q]] == tr["lambda"][rows[q - 1]] * 2.0 ** q


def test_trace_ten_trials_leave_the_rejected_state_in_the_edges():
    w, r = _trace("ten_trials")
    tr = r["trace"]
    assert S.has_exhausted(r) and r["iterations_run"] < w["iterations"]  # Terminate: qmax == 10
    rows = S.iteration_rows(tr, r["iterations_run"] - 1)
    assert (tr["rho"][rows] < 0).all() and (tr["ok2"][rows] == 1).all()
    # err_end and edge_chi2 are the LAST rejected trial's; the estimate is the restored one: re-running from the returned estimate
    # with no iteration gives the restored state's chi2, which differs
    assert np.float64(r["err_end"]) == np.float64(np.float32(tr["temp_chi"][rows[-1]]))
    back = S.run(dict(w, window=r["window"], points=r["points"], iterations=0))
    assert back["edge_chi2"].tobytes() != r["edge_chi2"].tobytes() and tr["temp_chi"][rows[-1]] > np.float64(back["err"]) * (1 - 1e-6)


def test_trace_nbad_stop():
    w, r = _trace("nbad_stop")
    tr = r["trace"]
    assert S.has_nbad_stop(r, w)
    # the last three iterations each gained less than a thousandth of their starting chi2
    first = np.float64(r["err"])
    chis = [first] + [tr["temp_chi"][S.iteration_rows(tr, it)[-1]] for it in range(r["iterations_run"])]
    bad = [(chis[i] - chis[i + 1]) * 1e3 < chis[i] for i in range(len(chis) - 1)]
    assert bad[-3:] == [True, True, True] and (len(bad) == 3 or not bad[-4])  # the stop came at the third in a row, not later


def test_trace_failed_factorisation():
    w, r = _trace("failed_factorisation")
    tr = r["trace"]
    assert tr["ok2"][0] == 0 and tr["temp_chi"][0] == np.finfo(np.float64).max and tr["rho"][0] == -np.inf and tr["accepted"][0] == 0
    assert tr["lambda"][1] == 2 * tr["lambda"][0]
    # rule F: a failed trial moves nothing -- one iteration of trials that all fail returns the caller's state
    fails = int(np.argmax(tr["ok2"] == 1)) if (tr["ok2"] == 1).any() else len(tr["ok2"])
    assert fails >= 2


def test_trace_nan_observation():
    w, r = _trace("nan_observation")
    tr = r["trace"]
    # NaN chi2: the solve fails on a NaN pivot, rho is NaN, `rho > 0` and `rho < 0` are both false: one rejected trial an iteration,
    # OK returned, every iteration run, lambda doubling and _ni never reset
    assert r["iterations_run"] == w["iterations"] and r["trials_run"] == w["iterations"]
    assert np.isnan(tr["rho"]).all() and (tr["accepted"] == 0).all() and (tr["ok2"] == 0).all()
    assert np.isnan(r["err"]) and np.isnan(r["err_end"])
    assert r["final_lambda"] == w["lambda_init"] * 2.0 ** sum(range(1, w["iterations"] + 1))
    assert r["points"].tobytes() == np.ascontiguousarray(w["points"], np.float64).tobytes()


def test_convergence_on_seeded_windows():
    for k, (w, r) in enumerate(zip(S.sweep(), S.sweep_results())):
        e0, e1 = S.position_error(w, w["window"]), S.position_error(w, r["window"])
        out, erase = w["is_outlier"], r["edge_erase"].astype(bool)
        print(f"window {k}: N={w['n_opt']} points={w['n_points']} edges={w['n_edges']} position {e0:.4f} -> {e1:.4f} m, "
              f"outliers flagged {erase[out].mean():.3f}, inliers flagged {erase[~out].mean():.4f}")
        assert e1 <= e0 + 0.01, (k, e0, e1)
        assert out.sum() > 0 and erase[out].mean() >= 0.9 and erase[~out].mean() <= 0.02, (k, erase[out].mean(), erase[~out].mean())
        assert not (2 * r["err"] < r["err_end"]) and r["err_end"] < r["err"]


def test_iterations_zero_returns_the_callers_state():
    w = S.size_cases()["iterations_0"]
    r = S.run(w, trace=True)
    assert r["iterations_run"] == 0 and r["trials_run"] == 0 and len(r["trace"]["lambda"]) == 0 and r["final_lambda"] == w["lambda_init"]
    assert np.float32(r["err"]).tobytes() == np.float32(r["err_end"]).tobytes()
    assert r["points"].tobytes() == np.ascontiguousarray(w["points"], np.float64).tobytes()


def test_erase_verdicts_follow_the_float_gates():
    w = S.sweep()[0]
    r = S.sweep_results()[0]
    c2, close, dp, st = r["edge_chi2"], w["close"].astype(bool), r["edge_depth_positive"].astype(bool), w["stereo"].astype(bool)
    m, s = np.float64(np.float32(5.991)), np.float64(np.float32(7.815))
    mc = np.float64(np.float32(1.5) * np.float32(5.991))
    want = np.where(st, c2 > s, ((c2 > m) & ~close) | ((c2 > mc) & close) | ~dp)
    assert (r["edge_erase"].astype(bool) == want).all()


def test_restatement_under_the_sanitizers():
    """The restatement and the rule header as a program of their own under -fsanitize=address,undefined (plain g++, CPU only, never
    loaded into python): no report, and the same lines as the unsanitized build of the same program."""
    main = os.path.join(S.ROOT, "tests", "host", "lba_inertial_restatement_main.cpp")
    outs = []
    for exe, flags in ((os.path.join(S.ROOT, "tests", "host", "_lba_inertial_restatement_asan"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]),
                       (os.path.join(S.ROOT, "tests", "host", "_lba_inertial_restatement_plain"), [])):
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", *flags, "-o", exe, main], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "" and r.stdout.endswith("lba_inertial_restatement_main: ok\n"), r.stderr[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1] and outs[0].count("\n") > 80
    assert sum(" failed 0 " not in line for line in outs[0].splitlines()[:-1]) > 10  # failed factorisations were among the runs
