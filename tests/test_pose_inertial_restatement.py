"""The rule of PoseInertialOptimization (geoflowslam_amd/csrc/pose_inertial_rule.hpp, through tests/host/pose_inertial_restatement.cpp)
against an independent statement in numpy float64 (tests/pose_inertial_support.py: numpy.arccos, numpy.linalg.svd, numpy.linalg.solve,
plain matrix products), step by step, and the schedule's branches on hand-built problems.  No GPU.

The bars of (a) and (b) are ten times the largest relative difference measured over the sweep of 2 x 40 problems, rounded up to a power
of ten.  Measured (restatement against numpy | numpy float64 against numpy longdouble, the noise floor):
    dx          8.9e-11 | 6.0e-13      H (system)  3.6e-16 | 4.2e-16      b           4.6e-12 | 2.2e-15
    visual err  3.4e-15 | 5.4e-15      visual chi2 1.1e-15 | 5.6e-15      small err   9.1e-11 | 1.1e-14
    small chi2  9.2e-12 | 4.1e-15      H (prior)   3.6e-16 | 6.0e-16
dx and the small edges' errors sit above the floor because the float dR of GetDeltaRotation can differ by one float ulp of an
off-diagonal entry (1.5e-11 absolute) between rules N + E, which round once, and numpy's float32 product and SVD."""
import functools

import numpy as np
import pytest

import pose_inertial_support as S
from geoflowslam_amd import synth

KF, FR = S.KF, S.FR
BARS = dict(dx=1e-9, H=1e-14, b=1e-10, vis_err=1e-13, vis_chi2=1e-13, small_err=1e-9, small_chi2=1e-10, Hf=1e-14)


@functools.lru_cache(maxsize=None)
def measured():
    """Largest relative difference over the sweep per quantity: (restatement vs numpy float64, numpy float64 vs longdouble)."""
    mx, floor = {}, {}
    for mode in (KF, FR):
        for k, p in enumerate(S.sweep(mode)):
            a, b = S.gn_step(p), S.np_gn_step(p)
            c = S.np_gn_step(p, np.longdouble) if k % 4 == 0 else None  # the floor on every fourth problem
            assert a["ok"]
            for q in ("dx", "H", "b", "vis_err", "vis_chi2", "small_err", "small_chi2"):
                mx[q] = max(mx.get(q, 0.0), S.rel(a[q], b[q]))
                if c is not None:
                    floor[q] = max(floor.get(q, 0.0), S.rel(b[q], c[q]))
            hb = S.np_final_hessian(p)
            mx["Hf"] = max(mx.get("Hf", 0.0), S.rel(S.final_hessian(p), hb))
            if c is not None:
                floor["Hf"] = max(floor.get("Hf", 0.0), S.rel(hb, S.np_final_hessian(p, np.longdouble)))
    return mx, floor


@pytest.mark.parametrize("q", ["dx", "H", "b", "vis_err", "vis_chi2", "small_err", "small_chi2"])
def test_a_one_gauss_newton_step(q):
    mx, floor = measured()
    print(f"{q}: restatement vs numpy {mx[q]:.2e}, numpy float64 vs longdouble {floor[q]:.2e}, bar {BARS[q]:.0e}")
    assert mx[q] <= BARS[q]


def test_b_hessian_of_the_new_prior():
    mx, floor = measured()
    print(f"Hf: restatement vs numpy {mx['Hf']:.2e}, numpy float64 vs longdouble {floor['Hf']:.2e}, bar {BARS['Hf']:.0e}")
    assert mx["Hf"] <= BARS["Hf"]
    # the layout: 15 x 15 in key-frame mode, 30 x 30 with the previous frame first in frame mode; what run() returns is this matrix
    # with the outliers' blocks left out
    for mode, D in ((KF, 15), (FR, 30)):
        p = S.sweep(mode)[0]
        r = S.run(p)
        assert r["H"].shape == (D, D)
        inl = S.with_obs(p, np.nonzero(r["outlier"] == 0)[0])
        inl["cur"] = dict(p["cur"], **{k: r["cur"][k] for k in ("Rwb", "twb", "v", "bg", "ba")})
        # (the camera pose of the final state, as ImuCamPose::Update derives it)
        inl["cur"]["Rcw"] = p["Rcb"] @ r["cur"]["Rwb"].T
        inl["cur"]["tcw"] = p["Rcb"] @ (-r["cur"]["Rwb"].T @ r["cur"]["twb"]) + p["tcb"]
        inl["other"] = dict(p["other"], **{k: r["other"][k] for k in ("Rwb", "twb", "v", "bg", "ba")})
        assert S.rel(r["H"], S.np_final_hessian(inl)) < 1e-9


# ---- (c) every written rule alone


def _rotations(rng, n, scale=1.0):
    return [S.np_exp_so3(scale * rng.normal(size=3)) for _ in range(n)]


def test_c_rule_N_nearest_rotation():
    rng = np.random.default_rng(1)
    worst = 0.0
    for R in _rotations(rng, 200):
        M = R + 1e-3 * rng.normal(size=(3, 3))  # far rougher than any input of the rule
        got, want = S.rule_nearest_rotation(M), S._nearest_rotation(M)
        worst = max(worst, np.abs(got - want).max())
        assert np.abs(got @ got.T - np.eye(3)).max() < 1e-15
    print("rule N against numpy.linalg.svd, perturbation 1e-3:", worst)
    assert worst < 1e-13  # measured 4.3e-15: numpy's own SVD is no closer to orthogonal than that
    R = _rotations(rng, 1)[0]
    assert np.abs(S.rule_nearest_rotation(R) - R).max() < 5e-16  # a rotation stays
    Mf = (R + 1e-6 * rng.normal(size=(3, 3))).astype(np.float32)
    assert np.abs(S.rule_nearest_rotation_f(Mf).astype(np.float64) - S._nearest_rotation(Mf.astype(np.float64))).max() < 6e-8
    assert not np.isfinite(S.rule_nearest_rotation(np.zeros((3, 3)))).any()  # a singular input: inf / NaN, as stated


def test_c_rule_E_float_exponential():
    rng = np.random.default_rng(2)
    for scale in (1.0, 1e-2, 1e-4, 3e-6, 1e-8, 0.0):  # |v|^2 on either side of 1e-10
        for _ in range(20):
            v = (scale * rng.normal(size=3)).astype(np.float32)
            got = S.rule_exp_so3f(v).astype(np.float64)
            assert np.abs(got - S.np_exp_so3f(v)).max() <= 6e-8, (scale, v)
    assert (S.rule_exp_so3f(np.zeros(3, np.float32)) == np.eye(3, dtype=np.float32)).all()


def test_c_rule_L_acos_distance_to_the_host_libm():
    rng = np.random.default_rng(3)
    x = np.r_[rng.uniform(-1, 1, 400000), 1 - 10.0 ** rng.uniform(-16, 0, 100000), -1 + 10.0 ** rng.uniform(-16, 0, 100000),
              10.0 ** rng.uniform(-300, 0, 20000), [1.0, -1.0, 0.0, 0.5, -0.5, np.nextafter(1.0, 0), np.nextafter(-1.0, 0)]]
    x = x[np.abs(x) <= 1]
    got, want = S.rule_acos(x), np.arccos(x)
    ulp = np.abs(got - want) / np.spacing(np.abs(want))
    print("rule L: largest distance to numpy.arccos in ulp", ulp.max(), "share of arguments that differ", (ulp > 0).mean())
    assert ulp.max() <= 1.0
    assert S.rule_acos(np.array([1.0]))[0] == 0.0 and S.rule_acos(np.array([-1.0]))[0] == np.pi and np.isnan(S.rule_acos(np.array([np.nan]))[0])


def test_c_log_and_exp_at_the_branch_points():
    rng = np.random.default_rng(4)
    for d in (0.5e-5, 0.999e-5, 1.001e-5, 2e-5, 1e-3, 0.3, 2.0, 3.0):  # d on either side of 1e-5, and beyond glibc_math's 2.4
        u = rng.normal(size=3)
        w = d * u / np.linalg.norm(u)
        got, want = S.rule_exp_so3(w), S.np_exp_so3(w)
        assert np.abs(got - want).max() < 1e-15, d
        assert np.abs(S.rule_inverse_right_jacobian(w) - S.np_inv_right_jacobian(w)).max() < 1e-9 * max(1.0, 1 / (np.pi - d) ** 2), d
        assert np.abs(S.rule_right_jacobian(w) - S.np_right_jacobian(w)).max() < 1e-12, d
        if d < 3.0:
            assert np.abs(S.rule_log_so3(want) - S.np_log_so3(want)).max() < 1e-9 * d + 1e-16, d
    I = np.eye(3)
    # costheta at +1 and -1 and just outside: outside, w is returned as it is
    for R in (I, np.diag([1.0, -1.0, -1.0]), I * (1 + 1e-15), np.diag([1.0, -1.0, -1.0]) * (1 + 1e-15)):
        assert (S.rule_log_so3(R) == S.np_log_so3(R)).all()
    out = I * (1 + 1e-12) + 1e-3 * S._hat(np.array([1.0, 2.0, 3.0]), np.float64)
    assert (S.rule_log_so3(out) == 1e-3 * np.array([1.0, 2.0, 3.0])).all()
    # |sin theta| < 1e-5 near theta = 0 and near pi: w unscaled
    for th in (0.5e-5, np.pi - 0.5e-5):
        R = S.np_exp_so3(np.array([th, 0, 0]))
        w = S.rule_log_so3(R)
        assert (w == np.array([(R[2, 1] - R[1, 2]) / 2, (R[0, 2] - R[2, 0]) / 2, (R[1, 0] - R[0, 1]) / 2])).all()
    x = np.r_[rng.uniform(-2.4, 2.4, 1000), rng.uniform(-40, 40, 1000)]
    s, c = S.rule_sincos(x)
    assert np.abs(s - np.sin(x)).max() < 1e-14 and np.abs(c - np.cos(x)).max() < 1e-14


def test_c_preintegration_deltas_and_the_non_finite_bias():
    p = S.sweep(KF)[1]
    bg, ba = p["other"]["bg"] + 1e-3, p["other"]["ba"] - 2e-3
    for a, b, tol in zip(S.rule_preint_deltas(p, bg, ba), S.np_preint_deltas(p, bg, ba)[:3], (1.2e-7, 0, 0)):
        assert np.abs(a - b).max() <= tol  # dV and dP are the same float operations: equal
    for bad in (np.array([np.nan, 0, 0]), np.array([0, np.inf, 0])):
        dR, dV, dP = S.rule_preint_deltas(p, bad, ba)
        dRn, dVn, dPn, _ = S.np_preint_deltas(p, bad, ba)
        assert np.isfinite(dR).all() and np.abs(dR - dRn).max() <= 1.2e-7  # the replacement (1e-6, 1e-6, 1e-5) enters the rotation only
        assert not np.isfinite(dV).all() and not np.isfinite(dVn).all()


def test_c_pose_update_and_its_counter():
    p = S.sweep(KF)[2]
    rng = np.random.default_rng(6)
    ups = 0.01 * rng.normal(size=(7, 6))
    Rwb, twb = p["cur"]["Rwb"].copy(), p["cur"]["twb"].copy()
    for k in range(7):
        twb = twb + Rwb @ ups[k, 3:]
        W = S._hat(ups[k, :3], np.float64)
        d = np.linalg.norm(ups[k, :3])
        Rwb = Rwb @ S._nearest_rotation(np.eye(3) + W * np.sin(d) / d + W @ W * (1 - np.cos(d)) / d ** 2)
        if (k + 1) % 3 == 0:
            Rwb = S._nearest_rotation(Rwb)
        got = S.rule_pose_update(p, ups[:k + 1])
        Rcw = p["Rcb"] @ Rwb.T
        for a, b in zip(got, (Rwb, twb, Rcw, p["Rcb"] @ (-Rwb.T @ twb) + p["tcb"])):
            assert np.abs(a - b).max() < 1e-14, k


def test_c_dense_solve_and_its_positive_gate():
    rng = np.random.default_rng(7)
    for N in (15, 30):
        M = rng.normal(size=(N, N))
        A = M @ M.T + np.diag(10.0 ** rng.uniform(-3, 6, N))  # pivots far from index order
        b = rng.normal(size=N)
        ok, x = S.rule_ldlt(A, b)
        assert ok and S.rel(x, np.linalg.solve(A, b)) < 1e-9
        A2 = A.copy()
        A2[3, 3] = -A2[3, 3] - 1e8
        ok, x = S.rule_ldlt(A2, b)
        assert not ok and (x == 0).all()  # not positive: x is left as it was
        ok, x = S.rule_ldlt(-A, b)
        assert not ok
        ok, x = S.rule_ldlt(np.zeros((N, N)), b)
        assert not ok


# ---- the schedule


@pytest.mark.parametrize("mode", [KF, FR])
def test_stale_chi2(mode):
    """The chi2 a round reads is that of the state before the round's last update; an edge that was an outlier is re-computed at the
    state after it."""
    p = S.sweep(mode)[5]
    r = S.run(p, trace=True)
    t = r["trace"]
    assert r["rounds_run"] == 4
    seen_fresh = False
    for it in range(4):
        before = S.np_visual_chi2(p, t["pose_before"][it, :9].reshape(3, 3), t["pose_before"][it, 9:])
        after = S.np_visual_chi2(p, t["pose_after"][it, :9].reshape(3, 3), t["pose_after"][it, 9:])
        fresh = t["round_fresh"][it] != 0
        got = t["round_chi2"][it]
        # re-computed are exactly the edges the rounds so far left as outliers
        assert (fresh == (S.run(dict(p, n_rounds=it))["outlier"] != 0 if it else np.zeros(len(got), bool))).all()
        assert np.allclose(got[fresh], after[fresh], rtol=1e-9, atol=1e-12)
        if it == 0:
            # every edge is active and stale.  The round's last update still moves the chi2 by `gap`; what the round read is the
            # chi2 before it, far closer than that gap, and as far from the chi2 after it as the gap
            gap = np.abs(before - after).max()
            print("largest change of a chi2 by the last update:", gap, "; read vs before:", np.abs(got - before).max(), "; read vs after:", np.abs(got - after).max())
            assert gap > 1e-10 and np.abs(got - before).max() < 0.05 * gap and np.abs(got - after).max() > 0.5 * gap
        seen_fresh |= fresh.any()
    assert seen_fresh


def test_fewer_than_ten_edges_break():
    c = S.hand_built()
    assert S.run(c["kf_edges_6"])["rounds_run"] == 1 and S.run(c["kf_edges_7"])["rounds_run"] == 4
    assert S.run(c["fr_edges_5"])["rounds_run"] == 1 and S.run(c["fr_edges_6"])["rounds_run"] == 4


def test_chi2_imu_branch_twice_in_a_row():
    r = S.run(S.hand_built()["kf_imu_twice"], trace=True)
    t = r["trace"]
    assert t["chi2_imu"][0] > 15 and t["chi2_imu"][1] > 15 and t["chi2_imu"][2] <= 15
    assert np.allclose(t["info_scale"], [1e-2, 1e-4, 1e-4, 1e-4], rtol=1e-12)
    # frame mode has no such branch
    f = S.run(synth.pose_inertial_problem(41, FR, n_obs=200, inconsistent=True), trace=True)
    assert (f["trace"]["info_scale"] == 1.0).all()


@pytest.mark.parametrize("tag", ["kf", "fr"])
def test_recovery_pass(tag):
    c = S.hand_built()
    r0, r1 = S.run(c[f"{tag}_few_inliers_rec0"], trace=True), S.run(c[f"{tag}_few_inliers_rec1"], trace=True)
    assert r0["n_inliers"] == r1["n_inliers"] < 30
    assert r0["trace"]["recovery_ran"][0] == 1 and r1["trace"]["recovery_ran"][0] == 0
    assert r1["n_good"] == r1["n_inliers"] and r0["n_good"] > r1["n_good"]
    assert (r0["outlier"] <= r1["outlier"]).all() and r0["outlier"].sum() < r1["outlier"].sum()  # flags are only ever cleared
    for k in ("Rwb", "twb", "v", "bg", "ba"):
        assert r0["cur"][k].tobytes() == r1["cur"][k].tobytes()


@pytest.mark.parametrize("tag", ["kf", "fr"])
def test_mono_edge_behind_the_camera(tag):
    r = S.run(S.hand_built()[f"{tag}_behind"], trace=True)
    assert r["outlier"][5] == 1 and (r["trace"]["round_chi2"][:, 5] < 1.0).all()  # far inside every gate: the depth test alone rejects it


@pytest.mark.parametrize("tag,mode", [("kf", KF), ("fr", FR)])
def test_close_and_far_mono_edges_with_the_same_chi2(tag, mode):
    r = S.run(S.hand_built()[f"{tag}_close_far"], trace=True)
    c3, c4 = r["trace"]["round_chi2"][3, 3], r["trace"]["round_chi2"][3, 4]
    # (the far edge, an outlier since an earlier round, is re-computed after the last update; the close one is stale: equal to 1e-9)
    assert np.float32(5.991) < np.float32(c3) < np.float32(1.5 * 5.991) and np.float32(5.991) < np.float32(c4) < np.float32(1.5 * 5.991) and abs(c3 - c4) < 1e-9 * c3
    assert r["outlier"][3] == 0 and r["outlier"][4] == 1


def test_indefinite_prior_fails_the_positive_gate():
    p = S.hand_built()["fr_indefinite_prior"]
    r = S.run(p, trace=True)
    t = r["trace"]
    assert (t["solve_failed"] == 1).all() and (t["iterations"] == 1).all() and r["rounds_run"] == 4
    # x was never written: the update adds zeros, the estimates stay (the rotation up to ExpSO3(0)'s projection)
    for k in ("twb", "v", "bg", "ba"):
        assert (r["cur"][k] == p["cur"][k]).all() and (r["other"][k] == p["other"][k]).all()
    assert np.abs(r["cur"]["Rwb"] - p["cur"]["Rwb"]).max() < 1e-6


@pytest.mark.parametrize("mode", [KF, FR])
def test_no_observations(mode):
    r = S.run(S.hand_built()["kf_no_obs" if mode == KF else "fr_no_obs"], trace=True)
    assert r["rounds_run"] == 1 and r["n_good"] == 0 and r["n_inliers"] == 0 and np.isnan(r["avg_reproj"]) and len(r["outlier"]) == 0
    assert r["trace"]["iterations"][0] == 10 and np.isfinite(r["H"]).all()


def test_restatement_under_the_sanitizers():
    """The restatement and the rule header as a program of their own under -fsanitize=address,undefined (plain g++, CPU only, never
    loaded into python): no report, and the same lines as the unsanitized build of the same program."""
    import os
    import subprocess
    main = os.path.join(S.ROOT, "tests", "host", "pose_inertial_restatement_main.cpp")
    outs = []
    for exe, flags in ((os.path.join(S.ROOT, "tests", "host", "_pose_inertial_restatement_asan"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]),
                       (os.path.join(S.ROOT, "tests", "host", "_pose_inertial_restatement_plain"), [])):
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", *flags, "-o", exe, main], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "" and r.stdout.endswith("pose_inertial_restatement_main: ok\n"), r.stderr[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1] and outs[0].count("\n") > 40
