"""GPU test of gfs_essential_graph_optimize against the float64 restatement (tests/pose_graph_support.py) on the maps that
tests/test_pose_graph_oracle_inputs.py holds to the inputs condition: rings of 10, 24 and 40 key-frames, fixed and free scale, with
and without ICP edges.  Final poses within the project's pose bar of 1e-5 (translation in metres, quaternion components after fixing
the sign), the final chi2 within 1e-6 relative, every edge's chi2 within 1e-5 relative plus 1e-12; iterations_run is reported, not
compared (after convergence the accept / reject decisions are rounding noise).  Also: a smaller map on a used handle (stale tiles),
iterations = 0, the refusals, and the map points moved with the poses the GPU itself returned, bit for bit.

On pose_graph_support.LEVENBERG_SEARCHES' cases the decisions are no noise (tests/test_pose_graph_levenberg_inputs.py: every one holds
at 1e-4 of chi2): there iterations_run and the number of trials equal the restatement's, and the final lambda is within 4 x the
case's float64 - long double distance of the float64 restatement's.  Estimates and measurements that are no numbers (the entry does
not validate them) are rejected trial by trial, as the restatement rejects them, and leave the handle as good as new."""
import numpy as np
import pytest

import pose_graph_support as pg

pytestmark = pytest.mark.gpu
POSE_BAR = 1e-5


@pytest.fixture(scope="module")
def opt(gpu_api):
    o = gpu_api.EssentialGraphOptimizer(max_vertices=64, max_edges=256, max_points=1024)
    yield o
    o.close()


def _est(r):
    return np.concatenate([r["vertex_q"], r["vertex_t"], r["vertex_s"][:, None]], 1)


@pytest.mark.parametrize("name", sorted(pg.MAPS))
def test_full_solve(gpu_api, opt, name):
    p = pg.map_problem(name)
    ref = pg.map_solution(name)
    r = opt.OptimizeEssentialGraph(p)
    info = opt.last_info()
    dq, dt, ds = pg.pose_difference(_est(r), ref["est"])
    chi = abs(r["final_chi2"] / float(ref["final_chi2"]) - 1)
    edge = np.abs(r["edge_chi2"] - ref["edge_chi2"]) - 1e-5 * np.abs(ref["edge_chi2"])
    print(f"{name}: dq {dq:.1e} dt {dt:.1e} ds {ds:.1e}; chi2 {r['final_chi2']:.9g} rel {chi:.1e}; edge chi2 excess over 1e-5 relative {edge.max():.1e}; "
          f"iterations {r['iterations_run']} (restatement {ref['iterations_run']}), trials {info['trials']}, launches {info['launches']}, "
          f"{info['n_free']} x {info['dimension']} in {info['panels']} panels")
    assert info["n_free"] == len(p["vertex_s"]) - 1 and info["dimension"] == (6 if p["fix_scale"] else 7)
    assert dq <= POSE_BAR and dt <= POSE_BAR and ds <= POSE_BAR
    assert chi <= 1e-6
    assert 1 <= r["iterations_run"] <= p["iterations"] and r["final_lambda"] > 0
    # the map points: the restatement's arithmetic at the Sim3s the GPU returned, bit for bit
    want = pg.correct_points(pg.PoseGraph(p).est, _est(r), p["points"], p["point_ref"])
    assert r["points"].tobytes() == want.tobytes()
    assert (r["points"][p["point_ref"] < 0] == p["points"][p["point_ref"] < 0]).all()
    assert np.abs(r["points"] - p["points"]).max() > 0.01


@pytest.mark.parametrize("name", sorted(pg.MAPS))
def test_edge_chi2(opt, name):
    """every edge's chi2 within 1e-5 relative plus 1e-12 absolute of the restatement's"""
    p, ref = pg.map_problem(name), pg.map_solution(name)
    r = opt.OptimizeEssentialGraph(p)
    allowed = 1e-5 * np.abs(ref["edge_chi2"]) + 1e-12
    ratio = np.abs(r["edge_chi2"] - ref["edge_chi2"]) / allowed
    print(f"{name}: largest |edge chi2 - restatement| = {ratio.max():.2f} of the allowance, at an edge of chi2 {ref['edge_chi2'][ratio.argmax()]:.2e}")
    assert (ratio <= 1).all()


def test_smaller_map_on_a_used_handle(gpu_api, opt):
    big, small = pg.map_problem("ring40_free_icp"), pg.map_problem("ring10_fixed")
    opt.OptimizeEssentialGraph(big)
    a = opt.OptimizeEssentialGraph(small)
    fresh = gpu_api.EssentialGraphOptimizer(max_vertices=16, max_edges=64, max_points=256)
    b = fresh.OptimizeEssentialGraph(small)
    fresh.close()
    for k in ("vertex_q", "vertex_t", "vertex_s", "points", "edge_chi2"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["iterations_run"], a["final_chi2"], a["final_lambda"]) == (b["iterations_run"], b["final_chi2"], b["final_lambda"])


def test_no_iteration_returns_the_input(opt):
    p = dict(pg.map_problem("ring10_free_icp"), iterations=0)
    r = opt.OptimizeEssentialGraph(p)
    G = pg.PoseGraph(p)
    chi = G.errors(G.est)[1]
    assert r["iterations_run"] == 0 and r["final_lambda"] == 0
    assert _est(r).tobytes() == G.est.tobytes()
    assert abs(r["final_chi2"] - float(G.total(chi))) <= 1e-12 * float(G.total(chi))
    assert np.allclose(r["edge_chi2"], chi, rtol=1e-9, atol=1e-18)
    assert r["points"].tobytes() == pg.correct_points(G.est, G.est, p["points"], p["point_ref"]).tobytes()


def test_no_free_vertex(opt):
    p = dict(pg.map_problem("ring10_fixed"))
    p["vertex_fixed"] = np.ones(10, np.uint8)
    r = opt.OptimizeEssentialGraph(p)
    assert r["iterations_run"] == 0 and _est(r).tobytes() == pg.PoseGraph(p).est.tobytes()


def test_refusals(gpu_api, opt):
    p = pg.map_problem("ring10_fixed")
    for change in (dict(edge_i=np.where(np.arange(len(p["edge_i"])) == 3, 10, p["edge_i"])),       # a vertex outside the graph
                   dict(edge_j=np.where(np.arange(len(p["edge_j"])) == 0, -1, p["edge_j"])),
                   dict(edge_i=p["edge_j"]),                                                          # an edge from a vertex to itself
                   dict(point_ref=np.where(np.arange(len(p["point_ref"])) == 1, 10, p["point_ref"])),  # a point on an unknown vertex
                   dict(vertex_s=np.where(np.arange(10) == 2, 0.0, p["vertex_s"])),
                   dict(lambda_init=0.0)):
        with pytest.raises(gpu_api.GfsError):
            opt.OptimizeEssentialGraph(dict(p, **change))
    with pytest.raises(gpu_api.GfsError):  # above the handle's limits
        small = gpu_api.EssentialGraphOptimizer(max_vertices=8, max_edges=64, max_points=256)
        try:
            small.OptimizeEssentialGraph(p)
        finally:
            small.close()
    r = opt.OptimizeEssentialGraph(p)  # the handle is as usable as before
    assert r["iterations_run"] >= 1


@pytest.mark.parametrize("name", sorted(pg.LEVENBERG_SEARCHES))
def test_levenberg_decisions(opt, name):
    """A rejected trial followed by an accepted one (the grown lambda's step is kept), an iteration that uses its ten trials up, an
    accepted trial whose alpha is not clamped (the final lambda carries rho, and through it computeScale's lambda x term)."""
    p = pg.levenberg_case(name)[0]
    ref, ref_l = pg.levenberg_solution(name), pg.levenberg_solution(name, np.longdouble)
    r = opt.OptimizeEssentialGraph(p)
    info = opt.last_info()
    dq, dt, ds = pg.pose_difference(_est(r), ref["est"])
    chi = abs(r["final_chi2"] / float(ref["final_chi2"]) - 1)
    lam, dist = float(ref["final_lambda"]), abs(float(ref["final_lambda"]) - float(ref_l["final_lambda"]))
    err = abs(r["final_lambda"] - lam)
    print(f"{name}: dq {dq:.1e} dt {dt:.1e} ds {ds:.1e}; chi2 rel {chi:.1e}; iterations {r['iterations_run']} (restatement {ref['iterations_run']}), trials "
          f"{info['trials']} ({len(ref['trace'])}); final lambda {r['final_lambda']:.17g} against {lam:.17g}: |GPU - float64| = {err:.1e}, float64 - long double "
          f"{dist:.1e}, ratio {err / dist if dist else float(err != 0):.3f}")
    assert dq <= POSE_BAR and dt <= POSE_BAR and ds <= POSE_BAR
    assert chi <= 1e-6
    assert r["iterations_run"] == ref["iterations_run"] == p["iterations"]
    assert info["trials"] == len(ref["trace"])
    assert err <= 4 * dist if dist else r["final_lambda"] == lam


@pytest.fixture(scope="module")
def clean_on_a_fresh_handle(gpu_api):
    fresh = gpu_api.EssentialGraphOptimizer(max_vertices=16, max_edges=64, max_points=256)
    r = fresh.OptimizeEssentialGraph(pg.map_problem("ring10_fixed"))
    fresh.close()
    return r


@pytest.mark.parametrize("name", sorted(pg.non_finite_problems()))
def test_non_finite_estimates_and_measurements(gpu_api, clean_on_a_fresh_handle, name):
    """NaN in a free vertex's translation, inf in a measurement's translation, NaN in the fixed vertex's quaternion: some edge's chi2
    is NaN, so the sum and rho are NaN (a failed solve gives (NaN - DBL_MAX) / 1e-3, NaN as well).  Why the device's loops end:
    b_decide accepts only if rho > 0 and sets `again` only if rho < 0 -- both false for a NaN -- so every trial is rejected, eg_solve's
    for (;;) leaves after the iteration's first trial (h_flags[0] == 0), and b_decide's terminate needs qmax == 10, rho == 0 or
    (ini - current) 1e3 < ini three times, all false; the outer loop then runs its 20 iterations and stops.  No kernel loops on a
    value: the factorisation returns at the first pivot that is no number (k_gba_diag), the later kernels of the trial return on
    solve_ok == 0.  So: iterations and trials as the restatement, the estimate that was given returned bit for bit, the same edges
    NaN, and the handle's next solve of a clean map equal to a fresh handle's byte for byte."""
    p, ref = pg.non_finite_problems()[name], pg.non_finite_solution(name)
    h = gpu_api.EssentialGraphOptimizer(max_vertices=16, max_edges=64, max_points=256)
    try:
        r = h.OptimizeEssentialGraph(p)
        info = h.last_info()
        after = h.OptimizeEssentialGraph(pg.map_problem("ring10_fixed"))
    finally:
        h.close()
    assert r["iterations_run"] == ref["iterations_run"] == 20 and info["trials"] == len(ref["trace"]) == 20
    assert ref["est"].tobytes() == pg.PoseGraph(p).est.tobytes() and _est(r).tobytes() == ref["est"].tobytes()
    assert (np.isnan(r["edge_chi2"]) == np.isnan(ref["edge_chi2"])).all() and np.isnan(ref["edge_chi2"]).any()
    ok = ~np.isnan(ref["edge_chi2"])
    assert np.allclose(r["edge_chi2"][ok], ref["edge_chi2"][ok], rtol=1e-5, atol=1e-12)
    assert np.isnan(r["final_chi2"]) and r["final_lambda"] == float(ref["final_lambda"])
    for k in ("vertex_q", "vertex_t", "vertex_s", "points", "edge_chi2"):
        assert after[k].tobytes() == clean_on_a_fresh_handle[k].tobytes(), k
    assert (after["iterations_run"], after["final_chi2"], after["final_lambda"]) == \
        (clean_on_a_fresh_handle["iterations_run"], clean_on_a_fresh_handle["final_chi2"], clean_on_a_fresh_handle["final_lambda"])
