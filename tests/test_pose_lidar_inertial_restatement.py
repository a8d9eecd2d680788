"""The sequential restatement of PoseLidarVisualInertialOptimization (tests/host/pose_lidar_inertial_restatement.cpp over
csrc/pose_lidar_inertial_rule.hpp) on the CPU: anchored against the PoseInertialOptimization restatement where the two must agree,
its lidar edge against an independent numpy statement, the quirks of DESIGN.md section 27 on its trace, convergence on synthetic
truth, and a run of the stand-alone program under the sanitizers.

Bars of the comparisons with the numpy statement: the statement's own float64-against-longdouble spread, measured over seeds 21-23 in
both modes on 300 edges (relative to the largest entry), times ten:
    error 3.2e-14 -> 3e-13;  numeric Jacobian 2.8e-7 -> 3e-6 (a +-1e-9 step amplifies rounding by 5e8);  H 7.9e-10 -> 8e-9;
    b 9.4e-10 -> 1e-8;  dx 3.0e-8 -> 3e-7;  returned Hessian 2.9e-10 -> 3e-9.
The restatement's distances measured with them: error 5.9e-14, Jacobian 4.8e-7, H 2.3e-9, b 1.8e-9, dx 4.0e-8, returned Hessian 8.5e-10;
numeric against analytic derivative 4.8e-7 (the longdouble central difference itself: 1.7e-10)."""
import os
import subprocess

import numpy as np
import pytest

import pose_inertial_support as PIS
import pose_lidar_inertial_support as S

KF, FR = S.KF, S.FR
SMALL = dict(width=160, height=120)
LD = np.longdouble
BAR = dict(err=3e-13, J=3e-6, H=8e-9, b=1e-8, dx=3e-7, Hfinal=3e-9)


def rel(a, b):
    return float(np.abs(np.asarray(a, LD) - np.asarray(b, LD)).max() / np.abs(np.asarray(b, LD)).max())


# ------------------------------------------------------------------------------------------------ anchor
@pytest.mark.parametrize("n_cloud", [0, 49])
@pytest.mark.parametrize("mode,n_rounds", [(KF, 1), (KF, 2), (KF, 3), (KF, 4), (FR, 4)])
def test_without_lidar_edges_it_is_pose_inertial(mode, n_rounds, n_cloud):
    p = S.case(3, mode, n_obs=150, n_cloud=n_cloud, n_rounds=n_rounds, **SMALL)
    r = S.run(p, trace=True)
    assert r["round_edges"] == [0, 0, 0, 0] and (r["trace"]["chi2_imu"] <= 15).all()
    assert S.common_bytes(r) == PIS.result_bytes(PIS.run(p))
    assert r["n_lidar_inliers"] == 0 and r["residual"] == 0


def test_frame_mode_three_rounds_drops_the_kernel_after_round_1():
    p = S.case(3, FR, n_obs=150, n_cloud=0, n_rounds=3, inconsistent=True, **SMALL)
    r = S.run(p, trace=True)
    assert r["trace"]["robust"].tolist() == [1, 1, 0, -1]
    assert S.common_bytes(r) != PIS.result_bytes(PIS.run(p))
    assert S.run(S.case(3, FR, n_obs=150, n_cloud=0, n_rounds=1, **SMALL), trace=True)["trace"]["robust"].tolist() == [1, -1, -1, -1]
    assert S.run(S.case(3, KF, n_obs=150, n_cloud=0, n_rounds=4, **SMALL), trace=True)["trace"]["robust"].tolist() == [1, 1, 1, 0]
    assert S.run(S.case(3, FR, n_obs=150, n_cloud=0, n_rounds=4, **SMALL), trace=True)["trace"]["robust"].tolist() == [1, 1, 1, 0]


# ------------------------------------------------------------------------------------------------ the lidar edge, independently
@pytest.fixture(scope="module", params=[(KF, 21), (FR, 22)])
def edge_case(request):
    mode, seed = request.param
    p = S.case(seed, mode, n_obs=150, n_cloud=300, **SMALL)
    edges = S.round0_edges(p)
    assert len(edges[0]) > 100
    return S.orthonormal(p), edges


def test_error_and_numeric_jacobian(edge_case):
    p, edges = edge_case
    err, J = S.lidar_linearize(p, edges)
    e_ld, J_ld = S.np_lidar_error(p, edges, LD), S.np_lidar_jacobian_numeric(p, edges, LD)
    d = dict(err=rel(err, e_ld), J=rel(J, J_ld), own_err=rel(S.np_lidar_error(p, edges), e_ld), own_J=rel(S.np_lidar_jacobian_numeric(p, edges), J_ld))
    print(d)
    assert d["err"] < BAR["err"] and d["J"] < BAR["J"], d
    assert d["own_err"] < BAR["err"] / 3 and d["own_J"] < BAR["J"] / 3, d


def test_numeric_jacobian_against_the_analytic_derivative(edge_case):
    p, edges = edge_case
    _, J = S.lidar_linearize(p, edges)
    Ja = S.np_lidar_jacobian_analytic(p, edges, LD)
    d = dict(rule=rel(J, Ja), longdouble=rel(S.np_lidar_jacobian_numeric(p, edges, LD), Ja))
    print(d)
    assert d["rule"] < BAR["J"] and d["longdouble"] < 1e-8, d


def test_one_gauss_newton_step_and_the_returned_hessian(edge_case):
    p, edges = edge_case
    g1, g0 = S.gn_step(p, edges), PIS.gn_step(p)  # with and without the lidar edges
    e_ld, J_ld = S.np_lidar_error(p, edges, LD), S.np_lidar_jacobian_numeric(p, edges, LD)
    H6, b6 = S.np_lidar_blocks(p, edges, J_ld, e_ld)
    H, b = np.asarray(g0["H"], LD).copy(), np.asarray(g0["b"], LD).copy()
    H[:6, :6] += H6
    b[:6] += b6
    dx = np.linalg.solve(H.astype(np.float64), b.astype(np.float64))
    off = 15 if p["mode"] == FR else 0
    Hf = np.asarray(PIS.final_hessian(p), LD).copy()
    Hf[off:off + 6, off:off + 6] += S.np_lidar_blocks(p, edges, J_ld, e_ld, robust=False)[0]
    got = S.final_hessian(p, edges)
    d = dict(H=rel(g1["H"][:6, :6], H[:6, :6]), b=rel(g1["b"][:6], b[:6]), dx=rel(g1["dx"], dx),
             Hfinal=rel(got[off:off + 6, off:off + 6], Hf[off:off + 6, off:off + 6]))
    print(d)
    assert g1["ok"] and all(d[k] < BAR[k] for k in d), d
    assert g1["H"][6:, 6:].tobytes() == g0["H"][6:, 6:].tobytes() and g1["b"][6:].tobytes() == g0["b"][6:].tobytes()  # the pose block only
    keep = np.ones(got.shape, bool)
    keep[off:off + 6, off:off + 6] = False
    assert (got[keep] == PIS.final_hessian(p)[keep]).all()


# ------------------------------------------------------------------------------------------------ the quirks, on the trace
def test_shift_in_frame_mode_only():
    for mode in (KF, FR):
        p = S.case(4, mode, n_obs=100, n_cloud=200, **SMALL)
        M = S.run(p, trace=True)["trace"]["init_pose"].reshape(4, 3, 4)
        plain = S.first_init_pose(KF, p["q"], p["t"])
        assert (M[0][:, :3] == plain[:, :3]).all()
        assert (M[0][:, 3] == plain[:, 3] + (0.1 if mode == FR else 0.0)).all()
        # later rounds: the float Sophus chain from the estimate, no shift; near the true camera position
        Twc = -(p["Rcb"] @ p["truth"]["Rwb"].T).T @ (p["Rcb"] @ (-p["truth"]["Rwb"].T @ p["truth"]["twb"]) + p["tcb"])
        assert np.abs(M[1][:, 3] - Twc).max() < 0.02 and np.abs(M[0][:, 3] - (0.1 if mode == FR else 0.0) - Twc).max() < 0.2


def test_next_init_pose_is_the_inverse_camera_pose():
    p = S.case(4, KF, n_obs=100, n_cloud=200, **SMALL)
    M = S.next_init_pose(p["cur"]["Rwb"], p["cur"]["twb"], p["tcb_q"], p["tcb_t"])
    Rwc = p["cur"]["Rwb"] @ p["Rbc"]
    twc = p["cur"]["Rwb"] @ p["tbc"] + p["cur"]["twb"]
    assert np.abs(M[:, :3] - Rwc).max() < 1e-6 and np.abs(M[:, 3] - twc).max() < 2e-6  # float arithmetic on metres
    assert (M == M.astype(np.float32)).all()


@pytest.mark.parametrize("gap,info", [(0.79, 1e2), (0.81, 1e4), (-1.0, 1e2)])
def test_kf_time_gap(gap, info):
    t = S.run(S.case(4, KF, n_obs=100, n_cloud=200, kf_time_gap=gap, **SMALL), trace=True)["trace"]
    assert (t["lidar_info"] == info).all()
    assert (S.run(S.case(4, FR, n_obs=100, n_cloud=200, kf_time_gap=gap, **SMALL), trace=True)["trace"]["lidar_info"] == 1e2).all()


@pytest.mark.parametrize("n_rounds,its", [(2, 2), (3, 0)])
def test_its_at_the_final_hessian(n_rounds, its):
    """20 updates leave VP's counter at 2: the perturbed poses of the final linearisation are normalised; 30 leave it at 0."""
    p = S.case(4, KF, n_obs=100, n_cloud=200, n_rounds=n_rounds, **SMALL)
    r = S.run(p, trace=True, edges=True)
    assert r["trace"]["iterations"][:n_rounds].tolist() == [10] * n_rounds and r["trace"]["final_its"][0] == its
    assert r["trace"]["final_round"][0] == n_rounds - 1
    edges = r["edges"][n_rounds - 1]
    after = r["trace"]["pose_after"][n_rounds - 1]
    end = dict(p, cur=dict(r["cur"], Rcw=after[:9].reshape(3, 3), tcw=after[9:]))  # the final estimate as the problem's state
    J_its, J_other = S.lidar_linearize(end, edges, its)[1], S.lidar_linearize(end, edges, 2 - its)[1]
    assert J_its.tobytes() != J_other.tobytes()
    # the returned Hessian is the restatement's at the end state, with the outlier flags as returned, under `its` -- and not under the
    # other value; its pose block less the other edges' share is these edges' J' Omega J with the perturbed poses as `its` makes them
    assert (r["trace"]["info_scale"][:n_rounds] == 1.0).all()
    assert S.final_hessian(end, edges, its, outlier=r["outlier"]).tobytes() == r["H"].tobytes()
    assert S.final_hessian(end, edges, 2 - its, outlier=r["outlier"]).tobytes() != r["H"].tobytes()
    none = tuple(a[:0] for a in edges)
    got = r["H"][:6, :6] - S.final_hessian(end, none, its, outlier=r["outlier"])[:6, :6]
    with_its, with_other = (J_its * 1e2).T @ J_its, (J_other * 1e2).T @ J_other
    d_its, d_other = np.abs(got - with_its).max(), np.abs(got - with_other).max()
    print(d_its, d_other, np.abs(with_its).max())
    assert d_its < d_other / 10, (d_its, d_other)


def test_the_edge_count_break():
    for mode, small in ((KF, 5), (FR, 6)):
        r = S.run(S.case(4, mode, n_obs=2, n_cloud=0, **SMALL), trace=True)
        assert r["rounds_run"] == 1 and r["trace"]["edges_total"].tolist() == [small, -1, -1, -1]
        r = S.run(S.case(4, mode, n_obs=2, n_cloud=200, **SMALL), trace=True)
        assert r["rounds_run"] == 4 and min(r["round_edges"]) >= 5 and (r["trace"]["edges_total"] == small + np.array(r["round_edges"])).all()


def test_far_map_gives_no_edges():
    for mode in (KF, FR):
        p = S.case(4, mode, n_obs=100, n_cloud=200, map_shift=50.0, **SMALL)
        r = S.run(p)
        assert r["round_edges"] == [0, 0, 0, 0] and r["rounds_run"] == 4 and r["n_lidar_inliers"] == 0 and r["residual"] == 0
        assert S.common_bytes(r) == S.common_bytes(S.run(S.without_cloud(p)))


def test_chi2_imu_branch_in_consecutive_rounds():
    """Read at the top of a round, in both modes: 0 before the first optimize, then the stale error under the information as left.  An
    inconsistent preintegration trips the gate at the top of rounds 1 and 2.  In frame mode the free previous frame absorbs it unless
    its prior holds it still (prior_scale); without that the same function reads chi2IMU and the information stays."""
    for mode, kw in ((KF, {}), (FR, dict(prior_scale=1e6))):
        t = S.run(S.case(4, mode, n_obs=100, n_cloud=200, inconsistent=True, **kw, **SMALL), trace=True)["trace"]
        assert t["chi2_imu"][0] == 0 and (t["chi2_imu"][1:3] > 15).all() and t["chi2_imu"][3] <= 15, (mode, t["chi2_imu"])
        assert np.allclose(t["info_scale"], [1.0, 1e-2, 1e-4, 1e-4], rtol=1e-12), (mode, t["info_scale"])
    t = S.run(S.case(4, FR, n_obs=100, n_cloud=200, inconsistent=True, **SMALL), trace=True)["trace"]
    assert t["chi2_imu"][0] == 0 and (t["chi2_imu"][1:] > 0).all() and (t["info_scale"] == 1.0).all(), t["chi2_imu"]


# ------------------------------------------------------------------------------------------------ convergence
@pytest.mark.parametrize("mode,seed", [(KF, 31), (KF, 33), (FR, 31), (FR, 32)])
def test_convergence(mode, seed):
    p = S.case(seed, mode, n_obs=150, n_cloud=300, **SMALL)
    start = S.position_error(p, dict(cur=p["cur"]))
    with_cloud, without = S.position_error(p, S.run(p)), S.position_error(p, S.run(S.without_cloud(p)))
    print(start, with_cloud, without)
    assert with_cloud <= start and without <= start and with_cloud <= without


# ------------------------------------------------------------------------------------------------ the sanitizers
def test_restatement_under_the_sanitizers():
    """The restatement and the rule headers as a program of their own under -fsanitize=address,undefined (plain g++, CPU only, never
    loaded into python): no report, and the same lines as the unsanitized build of the same program."""
    outs = []
    host = os.path.join(S.ROOT, "tests", "host")
    for exe, flags in ((os.path.join(host, "_pose_lidar_inertial_restatement_asan"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]),
                       (os.path.join(host, "_pose_lidar_inertial_restatement_plain"), [])):
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", *S.INCLUDES, *flags, "-o", exe, S.MAIN], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "" and r.stdout.endswith("pose_lidar_inertial_restatement_main: ok\n"), r.stderr[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1] and outs[0].count("\n") > 90
    assert any(" edges 0 0 0 0 " not in line for line in outs[0].splitlines()[:-1])
