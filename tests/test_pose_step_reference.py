"""CPU tests of the longdouble reference of Optimizer::PoseOptimization (tests/pose_step_support.py), before it is applied to k_pose_opt
(tests/test_gpu_pose_step.py):

 1. its Jacobians are the derivative of its own error function: central differences under exp(delta) T, in longdouble, to 1e-9;
 2. every case of the list meets the conditions that make it a case -- bars under the caps, every edge farther than 1e-6 from its
    gate, every trial of an its <= 3 run decided by a gain ratio above 1e-3 -- with the reference alone;
 3. the float64 restatement (oracle/pose_oracle.cpp: the bits the kernel's edge-order mode is held to) agrees with the reference on
    every case, after one, two and three LM iterations and after the full 4 x 10 schedule: pose within bar(), every edge's chi2 within
    chi2_bar(), outlier flags, n_inliers, rounds_run and iterations_run equal.

Measured here, the restatement against the reference (max |[R | t] - reference|; the bar; the worst edge's |chi2 - reference| as a
fraction of chi2_bar):
  its = 1, 2, 3   1.7e-17 ... 5.9e-14 (seed20: 15 degrees / 0.8 m of initial error), at most 0.12 of the bar;  bars 2.5e-14 (the
                  floor, 1.4e-14 ||pose||) ... 9.6e-13 (seed20; far_start 4.8e-13; every other case within 4x the floor);  chi2 <= 0.013
  4 x 10          3.5e-17 ... 1.0e-14 (far_start), at most 0.06 of the bar;  bars 2.5e-14 ... 2.8e-11 (seed13, all mono: the two runs
                  of the reference part at a toss over a step of 2e-9), then far_start 1.7e-13, seed20 9.8e-14, the rest at the
                  floor;  chi2 <= 0.003;  iterations_run equal in all 25
Seeds replaced (see the support module): 18 -> 48 and size 13878 -> seed 18878 (the last round ends one iteration apart), size 256
-> seed 2256 (with 1256 the restatement is 8.3e-13 from the reference after a toss over a step of 2e-12, bar 2.5e-14).
The reference with the exact V in place of SE3Quat::exp's small-angle branch parts from the restatement by up to 4e-11 over the full
schedule; a normwise bar on chi2 at the pose's relative bar would fail `near` after one and two iterations (4e-14, 1e-13 against
1.4e-14: the point at z = 0.02 carries the norm and pays 50x for the rounding of R X + t), hence chi2_bar().
"""
import numpy as np
import pytest

import pose_step_support as S

if not S.LONGDOUBLE_OK:
    pytest.skip("np.longdouble is not wider than float64 on this machine", allow_module_level=True)

LD = S.LD
NAMES = [c["name"] for c in S.case_list()]


@pytest.mark.parametrize("name", ["seed11", "seed13", "seed14", "behind", "near", "far_start"])
def test_jacobians_are_the_derivative_of_the_error(name):
    """Central differences of e(delta) = obs - pi(exp(delta) T X) (the smooth error: without the float 1 / z), h = 1e-6 and h / 2
    extrapolated to h^4 (a point at z = 0.02 has (h / z)^2 = 2.5e-9 of truncation error at h = 1e-6 otherwise)"""
    p = S.frame(name)
    P = S.problem(p)
    T = (S.quat_to_R(p["q"]), np.asarray(p["t"], LD))
    J = S.edge_jacobians(P, T)

    def central(h):
        D = np.zeros_like(J)
        for j in range(6):
            d = np.zeros(6, LD)
            d[j] = h
            D[:, :, j] = (S.edge_errors(P, S.oplus(T, d), float_invz=False) - S.edge_errors(P, S.oplus(T, -d), float_invz=False)) / (2 * h)
        return D

    h = LD(1e-6)
    D = (4 * central(h / 2) - central(h)) / 3
    rel = np.abs(J - D).max((1, 2)) / np.abs(J).max((1, 2))
    e = int(np.argmax(rel))
    assert rel[e] < 1e-9, (name, e, float(rel[e]), bool(P["stereo"][e]))
    assert (J[~P["stereo"], 2] == 0).all()
    if name in ("behind", "near"):  # the placed points are there, and carry the frame's largest / an ordinary Jacobian
        z = (P["xw"] @ T[0].T + T[1])[:, 2]
        assert (z < 0).sum() == 2 if name == "behind" else (np.abs(z) < 0.1).sum() == 2


def test_exp_is_a_rigid_motion_and_first_order_right():
    u = np.array([0.03, -0.11, 0.07, 0.2, -0.1, 0.05], LD)
    R, t = S.se3_exp(u)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-17 and abs(np.linalg.det(R.astype(np.float64)) - 1) < 1e-15
    R2, t2 = S.se3_exp(2 * u)  # exp(2u) = exp(u) exp(u)
    assert np.abs(R @ R - R2).max() < 1e-17 and np.abs(R @ t + t - t2).max() < 1e-17
    Rb, tb = S.se3_exp(np.array([0.9, 0.4, -0.3, 0.2, -0.1, 0.05], LD))  # the closed form (theta >= 0.5) against the series
    Rh, th = S.se3_exp(np.array([0.45, 0.2, -0.15, 0.1, -0.05, 0.025], LD))
    assert np.abs(Rh @ Rh - Rb).max() < 1e-17 and np.abs(Rh @ th + th - tb).max() < 1e-17
    Rs, ts = S.se3_exp(np.array([3e-6, 0, 0, 0, 1e-3, 0], LD))  # SE3Quat::exp below 1e-5: V = I + W + W^2, twice the first-order term
    assert abs(ts[2] - LD(3e-9)) < 1e-14 and abs(Rs[2, 1] - LD(3e-6)) < 1e-16


@pytest.mark.parametrize("name", NAMES)
def test_case_meets_the_conditions_of_the_list(name):
    c = S.conditions(name)
    print(name, {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in c.items()})
    assert c["bar_step"] <= S.BAR_CAP_STEP and c["bar_full"] <= S.BAR_CAP_FULL, c
    assert c["margin"] > S.GATE_MARGIN, c
    assert c["rho"] > S.RHO_MARGIN and c["tosses_in_steps"] == 0, c


def test_case_list_covers_what_it_has_to():
    cases = S.case_list()
    sizes = sorted(c["n_obs"] for c in cases if c["boundary"])
    assert sizes == sorted(S.BOUNDARY_SIZES) and max(c["n_obs"] for c in cases) == S.MAX_OBS
    assert sum(c["small"] for c in cases) >= 10  # two batches of five: the LM-step tests place a case at every slot of a batch
    frames = {c["name"]: S.frame(c["name"]) for c in cases}
    assert any(f["stereo"].all() for f in frames.values()) and any(not f["stereo"].any() for f in frames.values())
    assert min(f["n_obs"] for f in frames.values()) <= 30 and any(f["n_obs"] == 7000 for f in frames.values())
    assert (frames["info1e30"]["inv_sigma2"] == np.float32(1e30)).sum() == 5


@pytest.mark.parametrize("schedule", S.SCHEDULES, ids=["its1", "its2", "its3", "full"])
@pytest.mark.parametrize("name", NAMES)
def test_restatement_agrees_with_the_reference(oracle, name, schedule):
    its, nr = schedule
    R = S.ref(name, its, nr)
    o = oracle.pose_optimization(S.scheduled(name, its, nr))
    absolute, rel = S.bar(name, its, nr)
    d, (ex, e) = S.pose_diff(o, R), S.chi2_excess(o, name, its, nr)
    print(f"{name} its={its}: pose {d:.2e} (bar {absolute:.2e}, {rel:.2e} rel), chi2 {ex:.2e} of its bar (edge {e}, normwise {S.chi2_rel(o, R):.2e}), "
          f"iterations {o['iterations_run']} / {R['iterations_run']}")
    assert np.array_equal(o["outlier"], R["outlier"]) and o["n_inliers"] == R["n_inliers"] and o["rounds_run"] == R["rounds_run"]
    assert o["iterations_run"] == R["iterations_run"]
    assert d <= absolute, (d, absolute)
    assert ex <= 1.0, (ex, e)
    a, b = np.float32(o["avg_reproj_error"]), np.float32(R["avg_reproj_error"])  # the same floats added in the same order, up to float(chi2)
    assert abs(a - b) <= 1e-6 * abs(b), (a, b)


@pytest.mark.parametrize("n_obs", [0, 2, 3, 8, 9, 10])
def test_small_frames_follow_the_quirks(oracle, n_obs):
    """n < 3 gives 0 and the normalised input pose; n < 10 runs one round"""
    from geoflowslam_amd import synth
    p = synth.pose_frame(50 + n_obs, n_obs=n_obs, outlier_frac=0.0)
    R, o = S.reference(p), oracle.pose_optimization(p)
    assert R["rounds_run"] == o["rounds_run"] == (0 if n_obs < 3 else 1 if n_obs < 10 else 4)
    assert R["n_inliers"] == o["n_inliers"] and np.array_equal(R["outlier"], o["outlier"])
    assert S.pose_diff(o, R) < 1e-9  # (3 ... 10 edges: an ill-conditioned solve, held to the integers and loosely to the pose)
    if n_obs < 3:
        assert S.pose_diff(dict(q=p["q"], t=p["t"]), R) < 1e-17


def test_a_seeded_fault_in_the_reference_shows_after_one_step(monkeypatch):
    """The one-step comparison is sharp: the reference with the sign of one Jacobian column's stereo row flipped, or rho' left out of b, parts
    from itself by more than 1e-6 after one LM iteration -- seven orders above the bar."""
    name, base = "seed11", S.ref("seed11", 1, 1)
    absolute = S.bar(name, 1, 1)[0]
    p = S.scheduled(name, 1, 1)
    jac, neq = S.edge_jacobians, S.normal_equations

    def flipped(P, T):
        J = jac(P, T)
        J[:, 2, 1] = -J[:, 2, 1]
        return J

    def no_rho_in_b(P, T, r, chi2, active, robust):
        H, _ = neq(P, T, r, chi2, active, robust)
        return H, neq(P, T, r, chi2, active, False)[1]

    for attr, fault in (("edge_jacobians", flipped), ("normal_equations", no_rho_in_b)):
        monkeypatch.setattr(S, attr, fault)
        d = S.pose_diff(S.reference(p), base)
        monkeypatch.undo()
        assert d > 1e-6 > 1e6 * absolute, (attr, d)
