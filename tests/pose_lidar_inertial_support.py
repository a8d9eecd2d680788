"""Shared by the PoseLidarVisualInertialOptimization tests: builds and calls the sequential CPU restatement
(tests/host/pose_lidar_inertial_restatement.cpp), states the lidar edge, its derivative, one Gauss-Newton step and the returned Hessian
INDEPENDENTLY in numpy (rotation matrices, numpy.linalg.solve, float64 or longdouble: no code shared with
csrc/pose_lidar_inertial_rule.hpp), and constructs the cases the tests need, computed once and shared.  Not a test module."""
import ctypes as C
import functools
import os

import numpy as np

import pose_inertial_support as PIS
from geoflowslam_amd import api, synth

ROOT = PIS.ROOT
_CSRC = os.path.join(ROOT, "geoflowslam_amd", "csrc")
_HOST = os.path.join(ROOT, "tests", "host")
DEPS = [os.path.join(_CSRC, f) for f in ("pose_lidar_inertial_rule.hpp", "pose_inertial_rule.hpp", "so3_quat_rule.hpp", "glibc_math.hpp",
                                         "glibc_tables.inc")] + \
    [os.path.join(ROOT, "include", "gfs_abi.h"), os.path.join(_HOST, "pose_lidar_restatement.cpp"), os.path.join(ROOT, "oracle", "g2o_se3.hpp")]
SRC = os.path.join(_HOST, "pose_lidar_inertial_restatement.cpp")
MAIN = os.path.join(_HOST, "pose_lidar_inertial_restatement_main.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "oracle"), "-I" + os.path.join(ROOT, "include")]
_SO = os.path.join(_HOST, "_pose_lidar_inertial_restatement.so")
_L = None
KF, FR = api.POSE_INERTIAL_LAST_KEYFRAME, api.POSE_INERTIAL_LAST_FRAME
TRACE_FIELDS = ("round_chi2", "round_fresh", "pose_before", "pose_after", "chi2_imu", "info_scale", "iterations", "solve_failed", "recovery_ran",
                "init_pose", "lidar_info", "robust", "edges_total", "final_round", "final_its")


class Trace(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in TRACE_FIELDS]


def restatement():
    global _L
    if _L is None:
        L = PIS._build(_SO, SRC, [SRC] + DEPS, INCLUDES)
        vp, i = C.c_void_p, C.c_int
        PP = C.POINTER(api.PoseLidarInertialProblem)
        L.plir_optimize.argtypes = [PP, vp, i, C.POINTER(api.PoseLidarInertialSolution), vp, vp, vp, vp]
        L.plir_optimize_batch.argtypes = [vp, vp, vp, i, vp]
        L.plir_round0_edges.argtypes = [PP, vp, i, vp, vp, vp, vp]
        L.plir_lidar_linearize.argtypes = [PP, i, vp, vp, vp, i, vp, vp]
        L.plir_gn_step.argtypes = [PP, i, vp, vp, vp, vp, vp, vp]
        L.plir_final_hessian.argtypes = [PP, i, vp, vp, vp, i, vp, vp]
        L.plir_first_init_pose.argtypes = [i, vp, vp, vp]
        L.plir_next_init_pose.argtypes = [vp, vp, vp, vp, vp]
        L.plir_constants.argtypes = [vp]
        _L = L
    return _L


def _map_of(prob):
    m = np.ascontiguousarray(prob["map_xyz"], np.float32).reshape(-1, 3)
    return m


def run(prob, trace=False, edges=False):
    """The restatement on one problem dict (synth.pose_lidar_inertial_problem) -> result dict as api.PoseLidarInertialOptimizer.optimize's;
    with `edges`, plus `edges`: per round (index, plane, s); with `trace`, plus `trace` (the fields of the restatement's Trace)."""
    P, S, keep, n = api.pose_lidar_inertial_structs(prob)
    m = _map_of(prob)
    nc = P.n_cloud
    t, arrs = None, None
    if trace:
        z = lambda shape, dt=np.float64: np.zeros(shape, dt)
        arrs = dict(round_chi2=np.full((4, max(n, 1)), np.nan), round_fresh=z((4, max(n, 1)), np.uint8), pose_before=z((4, 12)), pose_after=z((4, 12)),
                    chi2_imu=z(4, np.float32), info_scale=z(4), iterations=z(4, np.int32), solve_failed=z(4, np.int32), recovery_ran=z(1, np.int32),
                    init_pose=z((4, 12)), lidar_info=z(4), robust=np.full(4, -1, np.int32), edges_total=np.full(4, -1, np.int32),
                    final_round=z(1, np.int32), final_its=z(1, np.int32))
        t = Trace(**{k: v.ctypes.data for k, v in arrs.items()})
    ei, ep, es = np.zeros((4, max(nc, 1)), np.int32), np.zeros((4, max(nc, 1), 4), np.float32), np.zeros((4, max(nc, 1)), np.float32)
    rc = restatement().plir_optimize(C.byref(P), m.ctypes.data, len(m), C.byref(S), C.byref(t) if t is not None else None, ei.ctypes.data,
                                     ep.ctypes.data, es.ctypes.data)
    assert rc == 0, rc
    res = api.pose_lidar_inertial_result(S, keep, n, P.vi.mode)
    if edges:
        res["edges"] = [(ei[r, :k].copy(), ep[r, :k].copy(), es[r, :k].copy()) for r, k in enumerate(res["round_edges"])]
    if trace:
        arrs["round_chi2"], arrs["round_fresh"] = arrs["round_chi2"][:, :n], arrs["round_fresh"][:, :n]
        res["trace"] = arrs
    return res


@functools.lru_cache(maxsize=None)
def case(seed, mode, **kw):
    """A synthetic problem, made once (the tests do not modify it)."""
    return synth.pose_lidar_inertial_problem(seed, mode, **kw)


@functools.lru_cache(maxsize=None)
def reference(seed, mode, **kw):
    """The restatement's result with edges for case(seed, mode, **kw), computed once."""
    return run(case(seed, mode, **kw), edges=True)


def result_bytes(r):
    """Everything gfs_pose_lidar_inertial_optimize returns, as bytes."""
    parts = [np.array([r["n_lidar_inliers"]] + list(r["round_edges"]) + list(r["round_valid"]), np.int32), np.array([r["residual"]], np.float32),
             np.asarray(r["round_chi2"], np.float32)]
    return PIS.result_bytes(r) + b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def assert_same(dev, ref, what="", dev_edges=None):
    """A device result against the restatement's (run(prob, edges=True)), byte for byte; dev_edges: per round (index, plane, s)."""
    for e in ("cur", "other"):
        for k in ("Rwb", "twb", "v", "bg", "ba"):
            assert dev[e][k].tobytes() == ref[e][k].tobytes(), (what, e, k, dev[e][k], ref[e][k])
    assert (dev["outlier"] == ref["outlier"]).all(), (what, "outlier", np.nonzero(dev["outlier"] != ref["outlier"])[0])
    for k in ("n_good", "n_inliers", "rounds_run", "n_lidar_inliers", "round_edges", "round_valid"):
        assert dev[k] == ref[k], (what, k, dev[k], ref[k])
    for k in ("avg_reproj", "residual", "round_chi2"):
        assert np.asarray(dev[k], np.float32).tobytes() == np.asarray(ref[k], np.float32).tobytes(), (what, k, dev[k], ref[k])
    assert dev["H"].tobytes() == ref["H"].tobytes(), (what, "H", np.abs(dev["H"] - ref["H"]).max())
    assert result_bytes(dev) == result_bytes(ref)
    if dev_edges is not None:
        for r, (d, e) in enumerate(zip(dev_edges, ref["edges"])):
            for a, b, name in zip(d, e, ("index", "plane", "s")):
                assert a.tobytes() == b.tobytes(), (what, "edges of round", r, name)


def common_bytes(r):
    """The outputs shared with gfs_pose_inertial_optimize."""
    return PIS.result_bytes(r)


# ---------------------------------------------------------------------------------------------------------------------------------
# pieces of the restatement
def round0_edges(prob):
    P, S, keep, n = api.pose_lidar_inertial_structs(prob)
    m, nc = _map_of(prob), max(P.n_cloud, 1)
    idx, pl, s, M = np.zeros(nc, np.int32), np.zeros((nc, 4), np.float32), np.zeros(nc, np.float32), np.zeros(12)
    k = restatement().plir_round0_edges(C.byref(P), m.ctypes.data, len(m), idx.ctypes.data, pl.ctypes.data, s.ctypes.data, M.ctypes.data)
    return idx[:k].copy(), pl[:k].copy(), s[:k].copy(), M.reshape(3, 4)


def lidar_linearize(prob, edges, its=0):
    P, S, keep, n = api.pose_lidar_inertial_structs(prob)
    idx, pl, s = (np.ascontiguousarray(a) for a in edges[:3])
    err, J = np.zeros(len(idx)), np.zeros((len(idx), 6))
    restatement().plir_lidar_linearize(C.byref(P), len(idx), idx.ctypes.data, pl.ctypes.data, s.ctypes.data, int(its), err.ctypes.data, J.ctypes.data)
    return err, J


def gn_step(prob, edges):
    P, S, keep, n = api.pose_lidar_inertial_structs(prob)
    idx, pl, s = (np.ascontiguousarray(a) for a in edges[:3])
    D = 30 if P.vi.mode == FR else 15
    dx, H, b = np.zeros(D), np.zeros((D, D)), np.zeros(D)
    ok = restatement().plir_gn_step(C.byref(P), len(idx), idx.ctypes.data, pl.ctypes.data, s.ctypes.data, dx.ctypes.data, H.ctypes.data, b.ctypes.data)
    return dict(dx=dx, H=H, b=b, ok=bool(ok))


def final_hessian(prob, edges, its=0, outlier=None):
    """The returned Hessian at the problem's state with VP's counter at `its`, the given lidar edges and, of the visual edges, those
    that `outlier` [n] (default: none) does not flag."""
    P, S, keep, n = api.pose_lidar_inertial_structs(prob)
    idx, pl, s = (np.ascontiguousarray(a) for a in edges[:3])
    D = 30 if P.vi.mode == FR else 15
    H = np.zeros((D, D))
    out = np.zeros(max(n, 1), np.uint8) if outlier is None else np.ascontiguousarray(outlier, np.uint8)
    restatement().plir_final_hessian(C.byref(P), len(idx), idx.ctypes.data, pl.ctypes.data, s.ctypes.data, int(its), out.ctypes.data, H.ctypes.data)
    return H


def first_init_pose(mode, q, t):
    q, t, M = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32), np.zeros(12)
    restatement().plir_first_init_pose(int(mode), q.ctypes.data, t.ctypes.data, M.ctypes.data)
    return M.reshape(3, 4)


def next_init_pose(Rwb, twb, tcb_q, tcb_t):
    a = [np.ascontiguousarray(Rwb, np.float64), np.ascontiguousarray(twb, np.float64), np.ascontiguousarray(tcb_q, np.float32),
         np.ascontiguousarray(tcb_t, np.float32)]
    M = np.zeros(12)
    restatement().plir_next_init_pose(*(x.ctypes.data for x in a), M.ctypes.data)
    return M.reshape(3, 4)


def constants():
    out = np.zeros(16)
    restatement().plir_constants(out.ctypes.data)
    names = ("lidar_info", "lidar_info_far", "kf_time_gap", "lidar_valid_chi2", "chi2_imu_gate", "huber_inertial_weak", "info_down", "huber_lidar",
             "init_shift", "min_cloud", "kernel_drop_round_keyframe", "kernel_drop_from_end_frame", "numeric_delta", "min_edges", "iterations",
             "perturbed")
    return dict(zip(names, out.tolist()))


# ---------------------------------------------------------------------------------------------------------------------------------
# the independent statement: rotation matrices throughout, any numpy float type
def _hat(w, dt):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dt)


def _exp(w, dt):
    w = np.asarray(w, dt)
    th = np.sqrt(w @ w)
    W = _hat(w, dt)
    if th < 1e-7:
        return np.eye(3, dtype=dt) + W + W @ W / dt(2)
    return np.eye(3, dtype=dt) + np.sin(th) / th * W + (1 - np.cos(th)) / (th * th) * (W @ W)


def np_lidar_error(prob, edges, dt=np.float64, Rwb=None, twb=None):
    """s (n . (Rwc p + twc) + d) for every edge, with Rwc = Rwb Rbc, twc = Rwb tbc + twb."""
    idx, pl, s = edges[:3]
    Rwb = np.asarray(prob["cur"]["Rwb"] if Rwb is None else Rwb, dt)
    twb = np.asarray(prob["cur"]["twb"] if twb is None else twb, dt)
    Rbc, tbc = np.asarray(prob["Rbc"], dt), np.asarray(prob["tbc"], dt)
    p = np.asarray(prob["cloud"], np.float32)[idx].astype(dt)
    pw = (p @ Rbc.T + tbc) @ Rwb.T + twb
    pl = np.asarray(pl, np.float32).astype(dt)
    return np.asarray(s, np.float32).astype(dt) * ((pw * pl[:, :3]).sum(1) + pl[:, 3])


def np_lidar_jacobian_numeric(prob, edges, dt=np.float64, delta=1e-9):
    """The central difference over ImuCamPose::Update's right update (twb += Rwb dt, Rwb <- Rwb Exp(dr)), columns (dr, dt)."""
    Rwb, twb = np.asarray(prob["cur"]["Rwb"], dt), np.asarray(prob["cur"]["twb"], dt)
    J = np.zeros((len(edges[0]), 6), dt)
    for d in range(6):
        e = []
        for sign in (1, -1):
            u = np.zeros(6, dt)
            u[d] = dt(sign) * dt(delta)
            e.append(np_lidar_error(prob, edges, dt, Rwb @ _exp(u[:3], dt), twb + Rwb @ u[3:]))
        J[:, d] = (e[0] - e[1]) / (dt(2) * dt(delta))
    return J


def np_lidar_jacobian_analytic(prob, edges, dt=np.float64):
    """d e / d (dr, dt) for the right update: with pb = Rbc p + tbc,  e = s (n . (Rwb pb + twb) + d):
    d e / d dr = -s n' Rwb [pb]x = s (pb x Rwb' n)',  d e / d dt = s n' Rwb."""
    idx, pl, s = edges[:3]
    Rwb = np.asarray(prob["cur"]["Rwb"], dt)
    Rbc, tbc = np.asarray(prob["Rbc"], dt), np.asarray(prob["tbc"], dt)
    pb = np.asarray(prob["cloud"], np.float32)[idx].astype(dt) @ Rbc.T + tbc
    nR = np.asarray(pl, np.float32).astype(dt)[:, :3] @ Rwb
    sc = np.asarray(s, np.float32).astype(dt)[:, None]
    return np.concatenate([sc * np.cross(pb, nR), sc * nR], 1)


def np_lidar_blocks(prob, edges, J, err, robust=True):
    """(H6 [6, 6], b6 [6]) the lidar edges add to the pose block and to b; robust: under Huber 1, else information() alone."""
    info = 1e4 if (prob["mode"] == KF and prob["kf_time_gap"] > 0.8) else 1e2
    chi2 = info * err * err
    rho1 = np.where(chi2 <= 1.0, 1.0, 1.0 / np.sqrt(np.maximum(chi2, 1e-300))) if robust else np.ones_like(err)
    H6 = (J * (rho1 * info)[:, None]).T @ J
    b6 = -(J * (rho1 * info * err)[:, None]).sum(0)
    return H6, b6


def orthonormal(prob):
    """The problem with Rwb and Rcb replaced by the nearest rotations in double (SVD) and the camera pose recomputed from them.  The
    problem's own matrices are floats widened, orthonormal to about 2^-23 only; the edge takes Rcw through a unit quaternion where
    the independent statement multiplies the matrices as they are, so on them the two differ by that much times the point's distance.
    On this variant they state the same function and differ by rounding alone."""
    def near(M):
        U, _, Vt = np.linalg.svd(np.asarray(M, np.float64))
        return U @ Vt
    Rwb, Rcb = near(prob["cur"]["Rwb"]), near(prob["Rcb"])
    tcb, twb = np.asarray(prob["tcb"], np.float64), np.asarray(prob["cur"]["twb"], np.float64)
    cur = dict(prob["cur"], Rwb=Rwb, Rcw=Rcb @ Rwb.T, tcw=Rcb @ (-Rwb.T @ twb) + tcb)
    return dict(prob, cur=cur, Rcb=Rcb, Rbc=Rcb.T.copy(), tbc=-Rcb.T @ tcb)


def position_error(prob, res):
    return float(np.linalg.norm(res["cur"]["twb"] - prob["truth"]["twb"]))


def without_cloud(prob):
    return dict(prob, cloud=None)
