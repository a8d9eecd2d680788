"""Conditions on the INPUTS of the GPU tests in which Levenberg's damping decides something, checked on the CPU with the restatement
(tests/pose_graph_support.py).  No GPU.

The first trial (tests/test_gpu_pose_graph_step.py): at lambda = k x max |diag H| the restatement's step differs from its step at
1e-16, in every block row that has a step at all, by more than 1000 x the bar the device's x is held to there, so a device that left
lambda out, or put it on other rows, misses the bar.

The full solves (tests/test_gpu_pose_graph.py, pose_graph_support.LEVENBERG_SEARCHES): each case's trace has the shape it is named
for, the run ends by using its iterations up, every decision in it -- the sign of current - temp, and (ini - current) 1e3 < ini --
holds at 1e-4 of chi2 or more (100 x the 1e-6 relative bar the device's final chi2 is held to), and float64 and long double take the
same decisions.  The inputs that are no numbers: the restatement rejects every trial and returns the estimate it was given."""
import numpy as np
import pytest

import pose_graph_support as pg
import test_gpu_pose_graph_step as step


@pytest.mark.parametrize("factor", step.LAMBDA_FACTORS)
@pytest.mark.parametrize("name", step.LAMBDA_CASES)
def test_lambda_moves_the_step_by_far_more_than_its_bar(name, factor):
    p = step.lambda_problem(name, factor)
    G = pg.PoseGraph(p)
    H, b, _ = G.system(G.est)
    x = G.step(G.est, H, b, p["lambda_init"])[0]
    x0 = G.step(G.est, H, b, 1e-16)[0]
    Gl = pg.PoseGraph(p, np.longdouble)
    Hl, bl, _ = Gl.system(Gl.est)
    xl = Gl.step(Gl.est, Hl, bl, p["lambda_init"])[0]
    assert p["lambda_init"] == factor * np.abs(np.diag(H)).max() and p["lambda_init"] > 1e-4
    ratios = []
    for f in range(G.F):
        rows = slice(G.dim * f, G.dim * f + G.dim)
        if f in step.edgeless_free_slots(p):  # lambda alone on the diagonal: the step is exactly zero at any lambda
            assert (x[rows] == 0).all() and (x0[rows] == 0).all() and (H[rows] == 0).all()
            continue
        bar = 4 * float(np.abs(x[rows] - xl[rows].astype(np.float64)).max())  # the step test's: 4 x the float64 / long-double spread
        ratios.append(float(np.abs(x[rows] - x0[rows]).max()) / bar)
    print(f"{name} at {factor:g} x max |diag H| = {p['lambda_init']:.3g}: |x(lambda) - x(1e-16)| is {min(ratios):.3g} .. {max(ratios):.3g} bars")
    assert min(ratios) > 1000


SHAPES = {"rejected_then_accepted_fixed": (True, False), "rejected_then_accepted_free": (False, False), "ends_qmax": (False, True),
          "unclamped_alpha": (False, False)}


@pytest.mark.parametrize("name", sorted(pg.LEVENBERG_SEARCHES))
def test_levenberg_case_has_its_shape_and_its_margins(name):
    p, seed = pg.levenberg_case(name)
    a, b = pg.levenberg_solution(name), pg.levenberg_solution(name, np.longdouble)
    rows, rows_l = pg.decisions(a), pg.decisions(b)
    seqs = [r[0] for r in rows]
    dq, dt, ds = pg.pose_difference(a["est"], b["est"].astype(np.float64))
    lam, lam_l = float(a["final_lambda"]), float(b["final_lambda"])
    print(f"{name}: seed {seed}, lambda_init {p['lambda_init']:g}, {p['iterations']} iterations, trials {' '.join(seqs)}; smallest margin "
          f"{min(r[1] for r in rows):.1e}; float64 against long double: dq {dq:.1e} dt {dt:.1e} ds {ds:.1e}, final lambda {lam:.17g} "
          f"against {lam_l:.17g} ({abs(lam - lam_l) / lam_l:.1e} relative)")
    fix_scale, at_qmax = SHAPES[name]
    assert bool(p["fix_scale"]) == fix_scale and len(p["vertex_s"]) == 10
    # the run ends by using its iterations up (ends_qmax: in the iteration that uses its ten trials up as well)
    assert a["iterations_run"] == b["iterations_run"] == p["iterations"] == len(rows) >= 2
    if at_qmax:
        assert seqs[-1] == "r" * 10 and any("A" in s for s in seqs[:-1])
    else:
        more = pg.PoseGraph(p).optimize(p["iterations"] + 1, p["lambda_init"])
        assert more["iterations_run"] == p["iterations"] + 1, "another criterion ended the run"
        assert all(s.endswith("A") for s in seqs)
    if name.startswith("rejected_then_accepted") or name == "unclamped_alpha":
        assert any("r" in s and s.endswith("A") for s in seqs[:-1]), "a grown lambda's result is kept and linearised at again"
    if name == "unclamped_alpha":
        assert any(al is not None and 1 / 3 < float(al) < 2 / 3 for al in a["alphas"])
        assert lam != lam_l, "the final lambda carries rho, and with it computeScale"
    assert min(r[1] for r in rows) >= pg.DECISION_MARGIN and min(r[1] for r in rows_l) >= pg.DECISION_MARGIN
    assert seqs == [r[0] for r in rows_l] and len(a["trace"]) == len(b["trace"])
    assert dq <= pg.INPUTS_BAR and dt <= pg.INPUTS_BAR
    assert abs(lam - lam_l) <= 1e-3 * lam_l


@pytest.mark.parametrize("name", sorted(pg.non_finite_problems()))
def test_non_finite_inputs_reject_every_trial(name):
    """A chi2 that is NaN makes rho NaN: `rho > 0` is false, so the trial is rejected, and `rho < 0` is false, so the iteration ends
    after that one trial; qmax == 10, rho == 0 and (ini - current) 1e3 < ini are all false, so every iteration runs."""
    p, s = pg.non_finite_problems()[name], pg.non_finite_solution(name)
    assert s["iterations_run"] == p["iterations"] == 20 and len(s["trace"]) == 20 and not any(t[1] for t in s["trace"])
    assert np.isnan(float(s["final_chi2"]))
    given = pg.PoseGraph(p).est
    assert s["est"].tobytes() == given.tobytes()
    bad = np.isnan(s["edge_chi2"])
    assert 1 <= bad.sum() < len(bad) and np.isfinite(s["edge_chi2"][~bad]).all()
    assert float(s["final_lambda"]) == 1e-16 * 2.0 ** (20 * 21 // 2)  # lambda x 2, x 4, ... : _ni is not reset by a rejection
