"""Shared by the PoseInertialOptimization tests: builds and calls the sequential CPU restatement
(tests/host/pose_inertial_restatement.cpp), states the edges, one Gauss-Newton step and the Hessian of the new prior INDEPENDENTLY in
numpy float64 (numpy.arccos, numpy.linalg.svd, numpy.linalg.solve, plain matrix products: no code shared with
csrc/pose_inertial_rule.hpp), and constructs the cases the tests need, computed once and shared.  Not a test module."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from geoflowslam_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "geoflowslam_amd", "csrc")
_DEPS = [os.path.join(_CSRC, f) for f in ("pose_inertial_rule.hpp", "so3_quat_rule.hpp", "glibc_math.hpp", "glibc_tables.inc")] + \
    [os.path.join(ROOT, "include", "gfs_abi.h")]
_SRC = os.path.join(ROOT, "tests", "host", "pose_inertial_restatement.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_pose_inertial_restatement.so")
_L = None
KF, FR = api.POSE_INERTIAL_LAST_KEYFRAME, api.POSE_INERTIAL_LAST_FRAME


def _build(so, src, deps, extra=()):
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", tmp, src, *extra], check=True)
        os.replace(tmp, so)
    return C.CDLL(so)


class Trace(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("round_chi2", "round_fresh", "pose_before", "pose_after", "chi2_imu", "info_scale", "iterations",
                                          "solve_failed", "recovery_ran")]


def restatement():
    global _L
    if _L is None:
        L = _build(_SO, _SRC, [_SRC] + _DEPS)
        vp, i = C.c_void_p, C.c_int
        L.pir_optimize.argtypes = [C.POINTER(api.PoseInertialProblem), C.POINTER(api.PoseInertialSolution), vp]
        L.pir_gn_step.argtypes = [C.POINTER(api.PoseInertialProblem)] + [vp] * 7
        L.pir_final_hessian.argtypes = [C.POINTER(api.PoseInertialProblem), vp]
        for name in ("pir_nearest_rotation", "pir_nearest_rotation_f", "pir_exp_so3f", "pir_exp_so3", "pir_log_so3", "pir_inverse_right_jacobian",
                     "pir_right_jacobian"):
            getattr(L, name).argtypes = [vp, vp]
        L.pir_acos.argtypes = [vp, vp, C.c_int64]
        L.pir_sincos.argtypes = [vp, vp, vp, C.c_int64]
        L.pir_pose_update.argtypes = [C.POINTER(api.PoseInertialProblem), vp, i, vp, vp, vp, vp]
        L.pir_preint_deltas.argtypes = [C.POINTER(api.PoseInertialProblem)] + [vp] * 5
        L.pir_ldlt.argtypes = [vp, vp, i, vp]
        L.pir_constants.argtypes = [vp]
        _L = L
    return _L


def run(prob, trace=False):
    """The restatement on one problem dict -> result dict as api.PoseInertialOptimizer.optimize's; with trace, plus `trace`: what the
    rounds read (round_chi2 / round_fresh [4, n], pose_before / pose_after [4, 12], chi2_imu, info_scale, iterations, solve_failed [4],
    recovery_ran)."""
    P, S, keep, n = api.pose_inertial_structs(prob)
    t, arrs = None, None
    if trace:
        arrs = dict(round_chi2=np.full((4, max(n, 1)), np.nan), round_fresh=np.zeros((4, max(n, 1)), np.uint8), pose_before=np.zeros((4, 12)),
                    pose_after=np.zeros((4, 12)), chi2_imu=np.zeros(4, np.float32), info_scale=np.zeros(4), iterations=np.zeros(4, np.int32),
                    solve_failed=np.zeros(4, np.int32), recovery_ran=np.zeros(1, np.int32))
        t = Trace(**{k: v.ctypes.data for k, v in arrs.items()})
    rc = restatement().pir_optimize(C.byref(P), C.byref(S), C.byref(t) if t is not None else None)
    assert rc == 0, rc
    res = api.pose_inertial_result(S, keep, n, P.mode)
    if trace:
        arrs["round_chi2"], arrs["round_fresh"] = arrs["round_chi2"][:, :n], arrs["round_fresh"][:, :n]
        res["trace"] = arrs
    return res


def result_bytes(r):
    """Everything gfs_pose_inertial_optimize returns, as bytes."""
    parts = [r[e][k] for e in ("cur", "other") for k in ("Rwb", "twb", "v", "bg", "ba")]
    parts += [r["outlier"], np.array([r["n_good"], r["n_inliers"], r["rounds_run"]], np.int32), np.array([r["avg_reproj"]], np.float32), r["H"]]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def assert_same(dev, prob, what=""):
    """A device result against the restatement, byte for byte; returns the restatement's."""
    ref = run(prob)
    for e in ("cur", "other"):
        for k in ("Rwb", "twb", "v", "bg", "ba"):
            assert dev[e][k].tobytes() == ref[e][k].tobytes(), (what, e, k, dev[e][k], ref[e][k])
    assert (dev["outlier"] == ref["outlier"]).all(), (what, "outlier", np.nonzero(dev["outlier"] != ref["outlier"])[0])
    for k in ("n_good", "n_inliers", "rounds_run"):
        assert dev[k] == ref[k], (what, k, dev[k], ref[k])
    assert np.float32(dev["avg_reproj"]).tobytes() == np.float32(ref["avg_reproj"]).tobytes(), (what, "avg_reproj", dev["avg_reproj"], ref["avg_reproj"])
    assert dev["H"].tobytes() == ref["H"].tobytes(), (what, "H", np.abs(dev["H"] - ref["H"]).max())
    assert result_bytes(dev) == result_bytes(ref)
    return ref


def gn_step(prob):
    """One Gauss-Newton step of the restatement from the problem's state -> dict(dx, H, b, vis_err, vis_chi2, small_err, small_chi2, ok)."""
    P, S, keep, n = api.pose_inertial_structs(prob)
    D = 30 if P.mode == FR else 15
    o = dict(dx=np.zeros(D), H=np.zeros((D, D)), b=np.zeros(D), vis_err=np.zeros((max(n, 1), 3)), vis_chi2=np.zeros(max(n, 1)), small_err=np.zeros(30),
             small_chi2=np.zeros(4))
    ok = restatement().pir_gn_step(C.byref(P), *(v.ctypes.data for v in o.values()))
    o["vis_err"], o["vis_chi2"], o["ok"] = o["vis_err"][:n], o["vis_chi2"][:n], bool(ok)
    return o


def final_hessian(prob):
    P, S, keep, n = api.pose_inertial_structs(prob)
    D = 30 if P.mode == FR else 15
    H = np.zeros((D, D))
    restatement().pir_final_hessian(C.byref(P), H.ctypes.data)
    return H


def constants():
    out = np.zeros(32)
    restatement().pir_constants(out.ctypes.data)
    return dict(chi2_mono_keyframe=out[0:4].tolist(), chi2_mono_frame=out[4:8].tolist(), chi2_stereo=out[8:12].tolist(), huber_inertial=out[12],
                huber_inertial_weak=out[13], huber_prior=out[14], chi2_imu_gate=out[15], info_down=out[16], chi2_mono_out=out[17],
                chi2_stereo_out=out[18], few_inliers=int(out[19]), min_edges=int(out[20]), iterations=int(out[21]), small_angle=out[22],
                gravity=out[23], dbg_replacement=out[24:27].tolist(), huber_mono=out[27], huber_stereo=out[28], normalize_every=int(out[29]),
                track_depth_close=out[30])


def _call2(name, a, out):
    a = np.ascontiguousarray(a)
    getattr(restatement(), name)(a.ctypes.data, out.ctypes.data)
    return out


def rule_nearest_rotation(M):
    return _call2("pir_nearest_rotation", np.asarray(M, np.float64), np.zeros((3, 3)))


def rule_nearest_rotation_f(M):
    return _call2("pir_nearest_rotation_f", np.asarray(M, np.float32), np.zeros((3, 3), np.float32))


def rule_exp_so3f(v):
    return _call2("pir_exp_so3f", np.asarray(v, np.float32), np.zeros((3, 3), np.float32))


def rule_exp_so3(w):
    return _call2("pir_exp_so3", np.asarray(w, np.float64), np.zeros((3, 3)))


def rule_log_so3(R):
    return _call2("pir_log_so3", np.asarray(R, np.float64), np.zeros(3))


def rule_inverse_right_jacobian(v):
    return _call2("pir_inverse_right_jacobian", np.asarray(v, np.float64), np.zeros((3, 3)))


def rule_right_jacobian(v):
    return _call2("pir_right_jacobian", np.asarray(v, np.float64), np.zeros((3, 3)))


def rule_acos(x):
    x = np.ascontiguousarray(x, np.float64)
    y = np.zeros_like(x)
    restatement().pir_acos(x.ctypes.data, y.ctypes.data, x.size)
    return y


def rule_sincos(x):
    x = np.ascontiguousarray(x, np.float64)
    s, c = np.zeros_like(x), np.zeros_like(x)
    restatement().pir_sincos(x.ctypes.data, s.ctypes.data, c.ctypes.data, x.size)
    return s, c


def rule_pose_update(prob, updates):
    P, S, keep, n = api.pose_inertial_structs(prob)
    u = np.ascontiguousarray(updates, np.float64).reshape(-1, 6)
    o = [np.zeros((3, 3)), np.zeros(3), np.zeros((3, 3)), np.zeros(3)]
    restatement().pir_pose_update(C.byref(P), u.ctypes.data, len(u), *(a.ctypes.data for a in o))
    return o


def rule_preint_deltas(prob, bg, ba):
    P, S, keep, n = api.pose_inertial_structs(prob)
    bg, ba = np.ascontiguousarray(bg, np.float64), np.ascontiguousarray(ba, np.float64)
    o = [np.zeros((3, 3)), np.zeros(3), np.zeros(3)]
    restatement().pir_preint_deltas(C.byref(P), bg.ctypes.data, ba.ctypes.data, *(a.ctypes.data for a in o))
    return o


def rule_ldlt(A, b):
    A, b = np.ascontiguousarray(A, np.float64), np.ascontiguousarray(b, np.float64)
    x = np.zeros(len(b))
    ok = restatement().pir_ldlt(A.ctypes.data, b.ctypes.data, len(b), x.ctypes.data)
    return bool(ok), x


# ---------------------------------------------------------------------------------------------------------------------------------
# The independent statement: the formulas of the reference's edges in numpy, at precision `ft` (float64, or longdouble for the noise
# floor).  Only the float arithmetic of the preintegration's bias correction is float32, as in the reference.


def _hat(v, ft):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], ft)


def _nearest_rotation(M):
    U, _, Vt = np.linalg.svd(np.asarray(M, np.float64))  # (LAPACK has no long double: the projection is float64 at both precisions)
    return U @ Vt


def np_exp_so3(w, ft=np.float64):
    w = np.asarray(w, ft)
    d2 = w @ w
    d = np.sqrt(d2)
    W = _hat(w, ft)
    if d < 1e-5:
        R = np.eye(3, dtype=ft) + W + ft(0.5) * (W @ W)
    else:
        R = np.eye(3, dtype=ft) + W * np.sin(d) / d + (W @ W) * (1 - np.cos(d)) / d2
    return _nearest_rotation(R).astype(ft)


def np_log_so3(R, ft=np.float64):
    R = np.asarray(R, ft)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], ft) / 2
    c = (np.trace(R) - 1) * ft(0.5)
    if c > 1 or c < -1:
        return w
    th = np.arccos(c)
    s = np.sin(th)
    return w if abs(s) < 1e-5 else th * w / s


def np_inv_right_jacobian(v, ft=np.float64):
    v = np.asarray(v, ft)
    d2 = v @ v
    d = np.sqrt(d2)
    if d < 1e-5:
        return np.eye(3, dtype=ft)
    W = _hat(v, ft)
    return np.eye(3, dtype=ft) + W / 2 + (W @ W) * (1 / d2 - (1 + np.cos(d)) / (2 * d * np.sin(d)))


def np_right_jacobian(v, ft=np.float64):
    v = np.asarray(v, ft)
    d2 = v @ v
    d = np.sqrt(d2)
    if d < 1e-5:
        return np.eye(3, dtype=ft)
    W = _hat(v, ft)
    return np.eye(3, dtype=ft) - W * (1 - np.cos(d)) / d2 + (W @ W) * (d - np.sin(d)) / (d2 * d)


def np_exp_so3f(v):
    """Sophus::SO3f::exp(v).matrix() in float64 (the rule rounds the same rotation to float once)."""
    v = np.asarray(v, np.float64)
    th = np.linalg.norm(v)
    W = _hat(v, np.float64)
    if th < 1e-9:
        return np.eye(3) + W
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * (W @ W)


def np_preint_deltas(prob, bg, ba):
    f = np.float32
    dbg, dba = np.asarray(bg, np.float64).astype(f) - prob["preint_bg"].astype(f), np.asarray(ba, np.float64).astype(f) - prob["preint_ba"].astype(f)
    dbr = dbg if np.isfinite(dbg).all() else np.array([1e-6, 1e-6, 1e-5], f)
    # float, as the reference: the exponential as a float matrix, the product in float, the projection's result a float matrix
    dR = _nearest_rotation(prob["dR"].astype(f) @ np_exp_so3f(prob["JRg"].astype(f) @ dbr).astype(f)).astype(f).astype(np.float64)
    dV = prob["dV"].astype(f) + prob["JVg"].astype(f) @ dbg + prob["JVa"].astype(f) @ dba
    dP = prob["dP"].astype(f) + prob["JPg"].astype(f) @ dbg + prob["JPa"].astype(f) @ dba
    return dR, dV.astype(np.float64), dP.astype(np.float64), dbg.astype(np.float64)


def _huber(chi2, delta):
    return 1.0 if chi2 <= delta * delta else delta / np.sqrt(chi2)


def np_edges(prob, ft=np.float64):
    """Every edge at the problem's state: a list of (err, J [E, D], information, huber delta or None) in insertion order, J over the
    unknowns of the dense system (VP, VV, VG, VA, then the other end's in frame mode)."""
    A = lambda x: np.asarray(x, ft)
    frame = prob["mode"] == FR
    D = 30 if frame else 15
    cur, oth = prob["cur"], prob["other"]
    Rcb, Rbc, tbc = A(prob["Rcb"]), A(prob["Rbc"]), A(prob["tbc"])
    Rcw, tcw = A(cur["Rcw"]), A(cur["tcw"])
    fx, fy, cx, cy, bf = (ft(prob[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    edges = []
    for e in range(prob["n_obs"]):
        X = Rcw @ A(prob["xw"][e]) + tcw
        Xb = Rbc @ X + tbc
        st = bool(prob["stereo"][e])
        u, v = fx * X[0] / X[2] + cx, fy * X[1] / X[2] + cy
        pj = np.array([[fx / X[2], 0, -fx * X[0] / X[2] ** 2], [0, fy / X[2], -fy * X[1] / X[2] ** 2]], ft)
        if st:
            err = A(prob["obs"][e]) - np.array([u, v, u - bf / X[2]], ft)
            pj = np.vstack([pj, pj[0] + np.array([0, 0, bf / X[2] ** 2], ft)])
        else:
            err = A(prob["obs"][e][:2]) - np.array([u, v], ft)
        dv = np.hstack([-_hat(Xb, ft), np.eye(3, dtype=ft)])
        J = np.zeros((len(err), D), ft)
        J[:, :6] = pj @ Rcb @ dv
        edges.append((err, J, np.eye(len(err), dtype=ft) * ft(prob["inv_sigma2"][e]), float(np.float32(np.sqrt(7.815 if st else 5.991)))))
    # the inertial edge
    dR, dV, dP, dbg = np_preint_deltas(prob, oth["bg"], oth["ba"])
    dR, dV, dP, dbg = A(dR), A(dV), A(dP), A(dbg)
    dt = ft(prob["dT"])
    g = np.array([0, 0, -float(np.float32(9.81))], ft)
    R1, R2 = A(oth["Rwb"]), A(cur["Rwb"])
    eR = dR.T @ R1.T @ R2
    er = np_log_so3(eR, ft)
    av = R1.T @ (A(cur["v"]) - A(oth["v"]) - g * dt)
    ap = R1.T @ (A(cur["twb"]) - A(oth["twb"]) - A(oth["v"]) * dt - g * dt * dt / 2)
    err = np.r_[er, av - dV, ap - dP]
    invJr = np_inv_right_jacobian(er, ft)
    JRg = A(prob["JRg"])
    blocks = dict(P1=np.zeros((9, 6), ft), V1=np.zeros((9, 3), ft), G1=np.zeros((9, 3), ft), A1=np.zeros((9, 3), ft), P2=np.zeros((9, 6), ft),
                  V2=np.zeros((9, 3), ft))
    blocks["P1"][0:3, 0:3] = -invJr @ R2.T @ R1
    blocks["P1"][3:6, 0:3] = _hat(av, ft)
    blocks["P1"][6:9, 0:3] = _hat(ap, ft)
    blocks["P1"][6:9, 3:6] = -np.eye(3)
    blocks["V1"][3:6] = -R1.T
    blocks["V1"][6:9] = -R1.T * dt
    blocks["G1"][0:3] = -invJr @ eR.T @ np_right_jacobian(JRg @ dbg, ft) @ JRg
    blocks["G1"][3:6] = -A(prob["JVg"])
    blocks["G1"][6:9] = -A(prob["JPg"])
    blocks["A1"][3:6] = -A(prob["JVa"])
    blocks["A1"][6:9] = -A(prob["JPa"])
    blocks["P2"][0:3, 0:3] = invJr
    blocks["P2"][6:9, 3:6] = R1.T @ R2
    blocks["V2"][3:6] = R1.T
    J = np.zeros((9, D), ft)
    J[:, 0:6], J[:, 6:9] = blocks["P2"], blocks["V2"]
    if frame:
        J[:, 15:21], J[:, 21:24], J[:, 24:27], J[:, 27:30] = blocks["P1"], blocks["V1"], blocks["G1"], blocks["A1"]
    edges.append((err, J, A(prob["info_inertial"]), 6.0))
    for key, at, info in (("bg", 9, "info_gyro_rw"), ("ba", 12, "info_acc_rw")):
        J = np.zeros((3, D), ft)
        J[:, at:at + 3] = np.eye(3)
        if frame:
            J[:, at + 15:at + 18] = -np.eye(3)
        edges.append((A(cur[key]) - A(oth[key]), J, A(prob[info]), None))
    if frame:
        Rp = A(prob["prior_Rwb"])
        er = np_log_so3(Rp.T @ R1, ft)
        err = np.r_[er, Rp.T @ (A(oth["twb"]) - A(prob["prior_twb"])), A(oth["v"]) - A(prob["prior_vwb"]), A(oth["bg"]) - A(prob["prior_bg"]),
                    A(oth["ba"]) - A(prob["prior_ba"])]
        J = np.zeros((15, D), ft)
        J[0:3, 15:18] = np_inv_right_jacobian(er, ft)
        J[3:6, 18:21] = Rp.T @ R1
        J[6:15, 21:30] = np.eye(9)
        edges.append((err, J, A(prob["prior_H"]), 5.0))
    return edges


def np_gn_step(prob, ft=np.float64):
    """-> dict(dx, H, b, vis_err [n, 3], vis_chi2, small_err [30], small_chi2 [4]) of one Gauss-Newton step with every edge active."""
    edges = np_edges(prob, ft)
    n = prob["n_obs"]
    D = 30 if prob["mode"] == FR else 15
    H, b = np.zeros((D, D), ft), np.zeros(D, ft)
    chi2s = []
    for err, J, info, delta in edges:
        chi2 = err @ info @ err
        chi2s.append(chi2)
        rho1 = ft(1.0) if delta is None else ft(_huber(float(chi2), delta))
        H += J.T @ (rho1 * info) @ J
        b -= rho1 * (J.T @ (info @ err))
    dx = np.linalg.solve(H.astype(np.float64), b.astype(np.float64)) if ft is np.float64 else _solve_ld(H, b)
    vis_err = np.zeros((n, 3), ft)
    for e in range(n):
        vis_err[e, :len(edges[e][0])] = edges[e][0]
    small = np.zeros(30, ft)
    small[0:9], small[9:12], small[12:15] = edges[n][0], edges[n + 1][0], edges[n + 2][0]
    sc = np.zeros(4, ft)
    sc[:3] = chi2s[n:n + 3]
    if prob["mode"] == FR:
        small[15:30], sc[3] = edges[n + 3][0], chi2s[n + 3]
    return dict(dx=dx, H=H, b=b, vis_err=vis_err, vis_chi2=np.array(chi2s[:n], ft), small_err=small, small_chi2=sc)


def _solve_ld(H, b):
    """Gaussian elimination with partial pivoting in the array's own precision (numpy.linalg has no long double)."""
    A = np.hstack([H.copy(), b.reshape(-1, 1).copy()])
    n = len(b)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]] = A[[p, k]]
        A[k + 1:] -= np.outer(A[k + 1:, k] / A[k, k], A[k])
    x = np.zeros(n, A.dtype)
    for k in range(n - 1, -1, -1):
        x[k] = (A[k, n] - A[k, k + 1:n] @ x[k + 1:]) / A[k, k]
    return x


def np_final_hessian(prob, ft=np.float64):
    """The Hessian of the new prior with every visual edge an inlier, in the layout of the reference (frame mode: the previous frame's
    15 first)."""
    edges = np_edges(prob, ft)
    D = 30 if prob["mode"] == FR else 15
    H = np.zeros((D, D), ft)
    for err, J, info, delta in edges:
        H += J.T @ info @ J
    if prob["mode"] == FR:
        perm = np.r_[15:30, 0:15]
        H = H[np.ix_(perm, perm)]
    return H


def np_visual_chi2(prob, Rcw, tcw):
    """chi2 of every visual edge at camera pose (Rcw, tcw)."""
    X = prob["xw"] @ np.asarray(Rcw).T + np.asarray(tcw)
    u, v = prob["fx"] * X[:, 0] / X[:, 2] + prob["cx"], prob["fy"] * X[:, 1] / X[:, 2] + prob["cy"]
    e = np.stack([prob["obs"][:, 0] - u, prob["obs"][:, 1] - v, np.where(prob["stereo"] != 0, prob["obs"][:, 2] - (u - prob["bf"] / X[:, 2]), 0.0)], 1)
    return (e * e).sum(1) * prob["inv_sigma2"].astype(np.float64)


def np_marginalize_prior(H30):
    """Optimizer::Marginalize(H, 0, 14) followed by ConstraintPoseImu's eigenvalue clamp, in numpy: the Schur complement of the previous
    frame's block through a pseudo-inverse that drops singular values below 1e-6, then eigenvalues below 1e-12 set to zero."""
    Haa, Hab, Hbb = H30[:15, :15], H30[:15, 15:], H30[15:, 15:]
    U, s, Vt = np.linalg.svd(Haa)
    sinv = np.where(s > 1e-6, 1.0 / np.where(s > 1e-6, s, 1.0), 0.0)
    Hm = Hbb - Hab.T @ (Vt.T @ np.diag(sinv) @ U.T) @ Hab
    Hm = (Hm + Hm.T) / 2
    w, V = np.linalg.eigh(Hm)
    w[w < 1e-12] = 0
    return V @ np.diag(w) @ V.T


def rel(a, b):
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), np.finfo(np.float64).tiny))


# ---------------------------------------------------------------------------------------------------------------------------------
# Cases


@functools.lru_cache(maxsize=None)
def sweep(mode):
    """The 40 seeded problems of a mode: n_obs 150..400, 10-30 % outliers, about a quarter with an inconsistent preintegration."""
    out = []
    for k in range(40):
        rng = np.random.default_rng(9000 + 100 * mode + k)
        out.append(synth.pose_inertial_problem(500 + 100 * mode + k, mode, n_obs=int(rng.integers(150, 401)), outlier_share=float(rng.uniform(0.1, 0.3)),
                                               inconsistent=bool(k % 4 == 3)))
    return out


def with_obs(prob, keep):
    """The problem with the visual edges `keep` (indices) only."""
    keep = np.asarray(keep, np.int64)
    p = dict(prob)
    for k in ("xw", "obs", "inv_sigma2", "stereo", "close", "is_outlier"):
        p[k] = prob[k][keep].copy()
    p["n_obs"] = len(keep)
    return p


def _project(prob, Rcw, tcw, xw):
    X = np.asarray(Rcw) @ xw + np.asarray(tcw)
    u = prob["fx"] * X[0] / X[2] + prob["cx"]
    return np.array([u, prob["fy"] * X[1] / X[2] + prob["cy"], u - prob["bf"] / X[2]]), X


def true_camera(prob):
    """Rcw, tcw of the true current pose."""
    t = prob["truth"]
    Rcw = prob["Rcb"] @ t["Rwb"].T
    return Rcw, prob["Rcb"] @ (-t["Rwb"].T @ t["twb"]) + prob["tcb"]


def behind_camera_case(mode):
    """All mono; edge 5 is a point BEHIND the camera observed exactly where the pinhole formula puts it: its chi2 is tiny, only
    isDepthPositive() rejects it."""
    p = synth.pose_inertial_problem(71 + mode, mode, n_obs=120, stereo_share=0.0, outlier_share=0.1)
    Rcw, tcw = true_camera(p)
    xc = np.array([0.3, -0.2, -4.0])
    p["xw"][5] = np.asarray(Rcw.T @ (xc - tcw), np.float32).astype(np.float64)
    uv, _ = _project(p, Rcw, tcw, p["xw"][5])
    p["obs"][5] = [np.float32(uv[0]), np.float32(uv[1]), -1.0]
    p["inv_sigma2"][5], p["stereo"][5], p["close"][5] = 1.0, 0, 1
    return p


def close_far_case(mode):
    """Mono edges 3 (close) and 4 (far) see the same point 2.7 px off: chi2 ~ 7.3, between the last gate 5.991 and 1.5 x it."""
    p = synth.pose_inertial_problem(81 + mode, mode, n_obs=300, outlier_share=0.1, pose_error=0.3)
    Rcw, tcw = true_camera(p)
    xc = np.array([0.4, 0.1, 5.0])
    for e, close in ((3, 1), (4, 0)):
        p["xw"][e] = np.asarray(Rcw.T @ (xc - tcw), np.float32).astype(np.float64)
        uv, _ = _project(p, Rcw, tcw, p["xw"][e])
        p["obs"][e] = [np.float32(uv[0] + 2.7), np.float32(uv[1]), -1.0]
        p["inv_sigma2"][e], p["stereo"][e], p["close"][e] = 1.0, 0, close
    return p


@functools.lru_cache(maxsize=None)
def hand_built():
    """name -> problem, the cases both the CPU and the GPU tests run."""
    c = {}
    for n in (6, 7):
        c[f"kf_edges_{n}"] = synth.pose_inertial_problem(20 + n, KF, n_obs=n, outlier_share=0.0)
    for n in (5, 6):
        c[f"fr_edges_{n}"] = synth.pose_inertial_problem(30 + n, FR, n_obs=n, outlier_share=0.0)
    c["kf_imu_twice"] = synth.pose_inertial_problem(41, KF, n_obs=200, inconsistent=True)
    for mode, tag in ((KF, "kf"), (FR, "fr")):
        for ri in (0, 1):
            c[f"{tag}_few_inliers_rec{ri}"] = synth.pose_inertial_problem(51 + mode, mode, n_obs=40, outlier_share=0.55, outlier_px=4.0, rec_init=bool(ri))
        c[f"{tag}_behind"] = behind_camera_case(mode)
        c[f"{tag}_close_far"] = close_far_case(mode)
        c[f"{tag}_no_obs"] = synth.pose_inertial_problem(61 + mode, mode, n_obs=0)
    bad = synth.pose_inertial_problem(91, FR, n_obs=150)
    bad["prior_H"] = np.diag(np.r_[np.full(7, -1e12), np.full(8, 1e4)])
    c["fr_indefinite_prior"] = bad
    return c


def next_frame_problem(prev, sol, seed):
    """The frame-mode problem that follows `prev` solved as `sol`: the other end is the solved current frame as SetImuPoseVelocity
    and IMU::Bias leave it (floats), its prior the marginalised Hessian, the truth goes on from prev's."""
    start = dict(prev["truth"], Rcb=prev["Rcb"], tcb=prev["tcb"])
    p = synth.pose_inertial_problem(seed, FR, n_obs=prev["n_obs"], start=start)
    f = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    Rwb, twb = f(sol["cur"]["Rwb"]), f(sol["cur"]["twb"])
    p["other"] = dict(Rwb=Rwb, twb=twb, Rcw=f(p["Rcb"] @ Rwb.T), tcw=f(p["Rcb"] @ (-Rwb.T @ twb) + p["tcb"]), v=f(sol["cur"]["v"]), bg=f(sol["cur"]["bg"]),
                      ba=f(sol["cur"]["ba"]))
    p["cur"] = dict(p["cur"], bg=p["other"]["bg"].copy(), ba=p["other"]["ba"].copy())
    # the constraint keeps the doubles of the estimate (ConstraintPoseImu(VP->estimate().Rwb, ...))
    p["prior_Rwb"], p["prior_twb"], p["prior_vwb"] = sol["cur"]["Rwb"].copy(), sol["cur"]["twb"].copy(), sol["cur"]["v"].copy()
    p["prior_bg"], p["prior_ba"] = sol["cur"]["bg"].copy(), sol["cur"]["ba"].copy()
    p["prior_H"] = np_marginalize_prior(sol["H"])
    return p


def variant(prob, kind):
    """The problem all-mono, all-stereo or as it is (mixed)."""
    p = dict(prob)
    if kind == "mono":
        p["stereo"] = np.zeros_like(prob["stereo"])
    elif kind == "stereo":
        p["stereo"] = np.ones_like(prob["stereo"])
        obs = prob["obs"].copy()
        Rcw, tcw = true_camera(prob)
        for e in np.nonzero(prob["stereo"] == 0)[0]:  # a right coordinate for the edges that had none
            X = Rcw @ prob["xw"][e] + tcw
            obs[e, 2] = np.float32(obs[e, 0] - prob["bf"] / X[2])
        p["obs"] = obs
    return p
