"""CPU conditions on the inputs of the GlobalBundleAdjustment GPU tests (no GPU): the bRobust = false convention on the oracle side, and
the robustness of every map the GPU solves completely (tests/gba_support.py)."""
import numpy as np
import pytest

import gba_support as G
import lba_stop_support as ST


def _Fp(api):
    return api.gba_panel_rows() // 6


def _bits(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("pose_q", "pose_t", "points", "edge_chi2", "edge_depth_positive")) + \
        np.array([r["iterations_run"], r["final_chi2"], r["final_lambda"]], np.float64).tobytes()


def test_infinite_huber_threshold_is_the_kernel_free_arithmetic(api, oracle):
    """bRobust = false is huber = +inf: RobustKernelHuber::robustify takes e <= dsqr, rho = (e, 1, 0), and a threshold so large that
    no edge passes it (1e150: its square is finite) gives the same bits -- with outliers in the map, unlike the finite g2o values"""
    w = G.gmap(_Fp(api) + 1, 200, 905)
    r_inf = oracle.lba_solve(dict(w, huber_mono=np.inf, huber_stereo=np.inf))
    r_big = oracle.lba_solve(dict(w, huber_mono=1e150, huber_stereo=1e150))
    r_rob = oracle.lba_solve(w)
    assert _bits(r_inf) == _bits(r_big)
    assert _bits(r_inf) != _bits(r_rob), "the map has no edge beyond the Huber thresholds: the convention is not exercised"


@pytest.mark.parametrize("name", G.FULL_SOLVES)
def test_full_solve_maps_do_not_hang_on_rounding(api, oracle, name):
    w = G.full_solve_map(name, _Fp(api))
    r, rs = oracle.lba_solve(w), oracle.lba_solve(ST.permuted(w))
    d = dict(pose_q=max(ST.rel(rs["pose_q"][i], r["pose_q"][i]) for i in range(w["n_poses"])),
             pose_t=max(ST.rel(rs["pose_t"][i], r["pose_t"][i]) for i in range(w["n_poses"])), points=ST.rel(rs["points"], r["points"]))
    print(name, w["n_poses"], w["n_points"], w["n_edges"], "iterations", r["iterations_run"], rs["iterations_run"], d)
    assert r["iterations_run"] == rs["iterations_run"] and r["iterations_run"] >= 2, name
    assert max(d.values()) <= 1e-7, (name, d)


def test_stop_map_rejects_trials_and_is_well_conditioned(api, oracle):
    w = G.stop_map(_Fp(api))
    seq, min_rho, sens, same = ST.check_window(oracle, w)
    print("stop map:", seq, min_rho, sens, same)
    assert "R" in seq and "A" in seq and same
    assert sens <= 1e-8 and min_rho >= 1e-3
