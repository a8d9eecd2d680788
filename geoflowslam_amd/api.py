"""Python mirror of the reference's four C++ seams on top of the C ABI (include/gfs_abi.h, libgfs_hip.so).

The product is the shared library; this module is the thin host-side binding used by tests and bench.py.
It mirrors the reference interfaces by name and argument meaning:
    ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)(image, lapping) -> (monoIndex, keypoints, descriptors)
        reference include/ORBextractor.h:53-64
    ORBmatcher.DescriptorDistance(a, b) / ORBmatcher.match(d1, d2)     reference include/ORBmatcher.h:41, src/ORBmatcher.cc:755-756
    RegistrationGICP.RegisterPointClouds(target, source, init_T)       reference include/RegistrationGICP.h:25-28
    Optimizer.LocalBundleAdjustment(problem)                           reference include/Optimizer.h:62-65
There is no CPU fallback here: if the library is missing, or no gfx950 device is present, calls raise GfsError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libgfs_hip.so")
_lib = None

KP_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
     ("class_id", "<i4")]
)


class GfsError(RuntimeError):
    pass


class OrbConfig(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("scale_factor", C.c_float), ("nlevels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("max_rows", C.c_int32),
                ("max_cols", C.c_int32), ("max_batch", C.c_int32), ("device", C.c_int32),
                ("blur_taps_variant", C.c_int32)]


def _i32_fields(names):
    return [(n, C.c_int32) for n in names.split()]


class OrbGeometryInfo(C.Structure):  # gfs_test_orb_geometry_info (include/gfs_abi_test.h)
    _fields_ = _i32_fields("supported pyr_strips pyr_strips_fine pyr_in_lds xtab_in_lds xtab_in_lds_fine kp_cap octree_on_device "
                           "oct_node_cap n_cells n_blur_tiles fast_lds_wave")


class OrbLevelInfo(C.Structure):  # gfs_test_orb_level_info
    _fields_ = _i32_fields("rows cols n_cell_cols n_cell_rows w_cell h_cell n_cells max_cell_w max_cell_h quota n_ini kp_cap "
                           "octree_on_device")


class OrbPaths(C.Structure):  # gfs_test_orb_paths
    _fields_ = _i32_fields("octree_on_device pyr_kernel pyr_fine_cut geometry_builds last_batch rows cols")


ORB_PYR_NONE, ORB_PYR_LDS, ORB_PYR_HBM = 0, 1, 2  # GFS_TEST_ORB_PYR_*


class GicpConfig(C.Structure):
    _fields_ = [("num_threads", C.c_int32), ("downsampling_resolution", C.c_double),
                ("max_correspondence_distance", C.c_double), ("rotation_eps", C.c_double),
                ("translation_eps", C.c_double), ("max_iterations", C.c_int32), ("num_neighbors", C.c_int32)]


class GicpResult(C.Structure):
    _fields_ = [("T", C.c_double * 16), ("converged", C.c_int32), ("iterations", C.c_uint64),
                ("num_inliers", C.c_uint64), ("H", C.c_double * 36), ("b", C.c_double * 6), ("error", C.c_double),
                ("n_target_ds", C.c_int32), ("n_source_ds", C.c_int32), ("n_linearize", C.c_int32),
                ("n_error_evals", C.c_int32)]


class LbaProblem(C.Structure):
    _fields_ = [("n_poses", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32), ("pose_q", C.c_void_p),
                ("pose_t", C.c_void_p), ("pose_fixed", C.c_void_p), ("points", C.c_void_p), ("edge_pose", C.c_void_p),
                ("edge_point", C.c_void_p), ("edge_obs", C.c_void_p), ("edge_inv_sigma2", C.c_void_p),
                ("edge_stereo", C.c_void_p), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("bf", C.c_double), ("huber_mono", C.c_double), ("huber_stereo", C.c_double),
                ("iterations", C.c_int32)]


class LbaSolution(C.Structure):
    _fields_ = [("pose_q", C.c_void_p), ("pose_t", C.c_void_p), ("points", C.c_void_p), ("edge_chi2", C.c_void_p),
                ("edge_depth_positive", C.c_void_p), ("iterations_run", C.c_int32), ("final_chi2", C.c_double),
                ("final_lambda", C.c_double)]


class LbaTrial(C.Structure):  # gfs_test_lba_trial (include/gfs_abi_test.h)
    _fields_ = [("Dinv", C.c_void_p), ("Hs", C.c_void_p), ("bs", C.c_void_p), ("xp", C.c_void_p), ("xl", C.c_void_p),
                ("lambda_", C.c_double), ("scale", C.c_double), ("solve_ok", C.c_int32)]


class GbaInfo(C.Structure):  # gfs_gba_info (include/gfs_abi.h)
    _fields_ = [("n_free", C.c_int32), ("panel_rows", C.c_int32), ("panels", C.c_int32), ("block_pairs", C.c_int64),
                ("contributions", C.c_int64), ("system_bytes", C.c_int64), ("trials", C.c_int32), ("launches", C.c_int32)]


class EssentialGraphProblem(C.Structure):  # gfs_essential_graph_problem (include/gfs_abi.h)
    _fields_ = [("n_vertices", C.c_int32), ("n_edges", C.c_int32), ("n_points", C.c_int32), ("vertex_q", C.c_void_p),
                ("vertex_t", C.c_void_p), ("vertex_s", C.c_void_p), ("vertex_fixed", C.c_void_p), ("edge_i", C.c_void_p),
                ("edge_j", C.c_void_p), ("edge_q", C.c_void_p), ("edge_t", C.c_void_p), ("edge_s", C.c_void_p), ("edge_w", C.c_void_p),
                ("fix_scale", C.c_int32), ("iterations", C.c_int32), ("lambda_init", C.c_double), ("points", C.c_void_p),
                ("point_ref", C.c_void_p)]


class EssentialGraphSolution(C.Structure):
    _fields_ = [("vertex_q", C.c_void_p), ("vertex_t", C.c_void_p), ("vertex_s", C.c_void_p), ("points", C.c_void_p),
                ("edge_chi2", C.c_void_p), ("iterations_run", C.c_int32), ("final_chi2", C.c_double), ("final_lambda", C.c_double)]


class EssentialGraphInfo(C.Structure):
    _fields_ = [("n_free", C.c_int32), ("dimension", C.c_int32), ("panels", C.c_int32), ("blocks", C.c_int64), ("trials", C.c_int32),
                ("launches", C.c_int32), ("system_bytes", C.c_int64)]


class EssentialGraphTrial(C.Structure):  # gfs_test_essential_graph_trial (include/gfs_abi_test.h)
    _fields_ = [("H", C.c_void_p), ("b", C.c_void_p), ("x", C.c_void_p), ("chi2", C.c_double), ("trial_chi2", C.c_double),
                ("scale", C.c_double), ("n_free", C.c_int32), ("dimension", C.c_int32), ("solve_ok", C.c_int32)]


class LbaLidar(C.Structure):
    _fields_ = [("map", C.c_void_p), ("pose_local", C.c_void_p), ("matches_inliers", C.c_void_p), ("cloud_begin", C.c_void_p),
                ("cloud", C.c_void_p), ("two_camera", C.c_int32)]


def lba_lidar_struct(prob, map_handle=None):
    """ctypes view of the lidar half of a LocalVisualLidarBA problem dict (pose_local, matches_inliers, cloud_begin, cloud,
    optional two_camera); shared with the CPU restatement's tests."""
    L = LbaLidar()
    keep = dict(pose_local=np.ascontiguousarray(prob["pose_local"], np.uint8),
                matches_inliers=np.ascontiguousarray(prob["matches_inliers"], np.int32),
                cloud_begin=np.ascontiguousarray(prob["cloud_begin"], np.int32),
                cloud=np.ascontiguousarray(prob["cloud"], np.float32).reshape(-1, 3))
    for k, v in keep.items():
        setattr(L, k, v.ctypes.data)
    L.map = map_handle
    L.two_camera = int(prob.get("two_camera", 0))
    return L, keep


class PoseProblem(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("n_obs", C.c_int32), ("xw", C.c_void_p), ("obs", C.c_void_p),
                ("inv_sigma2", C.c_void_p), ("stereo", C.c_void_p), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double), ("n_rounds", C.c_int32), ("its", C.c_int32)]


class PoseSolution(C.Structure):
    _fields_ = [("outlier", C.c_void_p), ("chi2", C.c_void_p), ("q", C.c_double * 4), ("t", C.c_double * 3),
                ("avg_reproj_error", C.c_float), ("n_inliers", C.c_int32), ("rounds_run", C.c_int32),
                ("iterations_run", C.c_int32)]


def pose_structs(prob):
    """ctypes views of one PoseOptimization problem dict (shared with oracle/oracle.py: same struct layout)."""
    P, S = PoseProblem(), PoseSolution()
    n = int(prob["n_obs"]) if "n_obs" in prob else len(prob["xw"])
    keep = dict(xw=np.ascontiguousarray(prob["xw"], np.float64).reshape(-1, 3), obs=np.ascontiguousarray(prob["obs"], np.float64).reshape(-1, 3),
                inv_sigma2=np.ascontiguousarray(prob["inv_sigma2"], np.float32), stereo=np.ascontiguousarray(prob["stereo"], np.uint8),
                outlier=np.zeros(max(n, 1), np.uint8), chi2=np.zeros(max(n, 1), np.float64))
    P.q[:] = [float(v) for v in prob["q"]]
    P.t[:] = [float(v) for v in prob["t"]]
    P.n_obs = n
    for name in ("xw", "obs", "inv_sigma2", "stereo"):
        setattr(P, name, keep[name].ctypes.data)
    for name in ("fx", "fy", "cx", "cy", "bf"):
        setattr(P, name, float(prob[name]))
    P.n_rounds = int(prob.get("n_rounds", 4))
    P.its = int(prob.get("its", 10))
    S.outlier = keep["outlier"].ctypes.data
    S.chi2 = keep["chi2"].ctypes.data
    return P, S, keep, n


def pose_result(S, keep, n):
    return dict(outlier=keep["outlier"][:n].astype(bool), chi2=keep["chi2"][:n].copy(), q=np.array(S.q[:]), t=np.array(S.t[:]),
                avg_reproj_error=float(S.avg_reproj_error), n_inliers=int(S.n_inliers), rounds_run=int(S.rounds_run),
                iterations_run=int(S.iterations_run))


class Sim3OptProblem(C.Structure):
    _fields_ = [("s12", C.c_double * 8), ("cam1", C.c_double * 4), ("cam2", C.c_double * 4), ("th2", C.c_float),
                ("fix_scale", C.c_int32), ("n_pairs", C.c_int32), ("x1c", C.c_void_p), ("x2c", C.c_void_p), ("obs1", C.c_void_p),
                ("obs2", C.c_void_p), ("inv_sigma2_1", C.c_void_p), ("inv_sigma2_2", C.c_void_p)]


class Sim3OptSolution(C.Structure):
    _fields_ = [("s12", C.c_double * 8), ("n_in", C.c_int32), ("n_bad", C.c_int32), ("status", C.c_int32),
                ("iterations_run", C.c_int32 * 2), ("pair_state", C.c_void_p), ("chi2", C.c_void_p)]


SIM3_OPT_EARLY_RETURN, SIM3_OPT_BOTH_PHASES = 0, 1  # GFS_SIM3_OPT_* (include/gfs_abi.h)
SIM3_PAIR_INLIER, SIM3_PAIR_REMOVED_FIRST, SIM3_PAIR_REMOVED_FINAL = 0, 1, 2  # GFS_SIM3_PAIR_*


def sim3_opt_structs(prob):
    """ctypes views of one OptimizeSim3 problem dict (synth.sim3_opt_problem; shared with the CPU restatement's tests)."""
    P, S = Sim3OptProblem(), Sim3OptSolution()
    n = int(prob["n_pairs"]) if "n_pairs" in prob else len(prob["x1c"])
    keep = dict(x1c=np.ascontiguousarray(prob["x1c"], np.float64).reshape(-1, 3), x2c=np.ascontiguousarray(prob["x2c"], np.float64).reshape(-1, 3),
                obs1=np.ascontiguousarray(prob["obs1"], np.float64).reshape(-1, 2), obs2=np.ascontiguousarray(prob["obs2"], np.float64).reshape(-1, 2),
                inv_sigma2_1=np.ascontiguousarray(prob["inv_sigma2_1"], np.float32), inv_sigma2_2=np.ascontiguousarray(prob["inv_sigma2_2"], np.float32),
                pair_state=np.zeros(max(n, 1), np.uint8), chi2=np.zeros((max(n, 1), 2), np.float64))
    P.s12[:] = [float(v) for v in prob["s12"]]
    P.cam1[:] = [float(v) for v in prob["cam1"]]
    P.cam2[:] = [float(v) for v in prob["cam2"]]
    P.th2 = float(prob["th2"])
    P.fix_scale = int(bool(prob["fix_scale"]))
    P.n_pairs = n
    for name in ("x1c", "x2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"):
        setattr(P, name, keep[name].ctypes.data)
    S.pair_state = keep["pair_state"].ctypes.data
    S.chi2 = keep["chi2"].ctypes.data
    return P, S, keep, n


def sim3_opt_result(S, keep, n):
    return dict(s12=np.array(S.s12[:]), n_in=int(S.n_in), n_bad=int(S.n_bad), status=int(S.status),
                iterations_run=(int(S.iterations_run[0]), int(S.iterations_run[1])), pair_state=keep["pair_state"][:max(n, 0)].copy(),
                chi2=keep["chi2"][:max(n, 0)].copy())


class Sim3RansacProblem(C.Structure):
    _fields_ = [("n_pairs", C.c_int32), ("x3d_c1", C.c_void_p), ("x3d_c2", C.c_void_p), ("max_err1", C.c_void_p), ("max_err2", C.c_void_p),
                ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float), ("fx2", C.c_float), ("fy2", C.c_float),
                ("cx2", C.c_float), ("cy2", C.c_float), ("fix_scale", C.c_int32), ("min_inliers", C.c_int32), ("n_iterations", C.c_int32),
                ("draws", C.c_void_p)]


class Sim3RansacSolution(C.Structure):
    _fields_ = [("T12", C.c_float * 16), ("R12", C.c_float * 9), ("t12", C.c_float * 3), ("s12", C.c_float), ("n_inliers", C.c_int32),
                ("iterations", C.c_int32), ("status", C.c_int32), ("inlier", C.c_void_p), ("counts", C.c_void_p)]


SIM3_RANSAC_CONVERGED, SIM3_RANSAC_NO_MORE, SIM3_RANSAC_TOO_FEW = 0, 1, 2  # GFS_SIM3_RANSAC_* (include/gfs_abi.h)


def sim3_ransac_structs(prob):
    """ctypes views of one Sim3Solver problem dict (synth.sim3_ransac_problem; shared with the CPU restatement's tests): x3d_c1 /
    x3d_c2 [n, 3], max_err1 / max_err2 [n], cam1 / cam2 (fx, fy, cx, cy), fix_scale, min_inliers, draws [n_iterations, 3]."""
    P, S = Sim3RansacProblem(), Sim3RansacSolution()
    n = len(prob["x3d_c1"])
    draws = np.ascontiguousarray(prob["draws"], np.int32).reshape(-1, 3)
    H = int(prob.get("n_iterations", len(draws)))
    keep = dict(x3d_c1=np.ascontiguousarray(prob["x3d_c1"], np.float32).reshape(-1, 3), x3d_c2=np.ascontiguousarray(prob["x3d_c2"], np.float32).reshape(-1, 3),
                max_err1=np.ascontiguousarray(prob["max_err1"], np.float32), max_err2=np.ascontiguousarray(prob["max_err2"], np.float32),
                draws=draws, inlier=np.zeros(max(n, 1), np.uint8), counts=np.full(max(H, 1), -1, np.int32))
    P.n_pairs = n
    for name in ("x3d_c1", "x3d_c2", "max_err1", "max_err2", "draws"):
        setattr(P, name, keep[name].ctypes.data)
    P.fx1, P.fy1, P.cx1, P.cy1 = (float(v) for v in prob["cam1"])
    P.fx2, P.fy2, P.cx2, P.cy2 = (float(v) for v in prob["cam2"])
    P.fix_scale, P.min_inliers, P.n_iterations = int(bool(prob["fix_scale"])), int(prob["min_inliers"]), H
    S.inlier, S.counts = keep["inlier"].ctypes.data, keep["counts"].ctypes.data
    return P, S, keep, n


def sim3_ransac_result(S, keep, n):
    return dict(T12=np.array(S.T12[:], np.float32).reshape(4, 4), R12=np.array(S.R12[:], np.float32).reshape(3, 3), t12=np.array(S.t12[:], np.float32),
                s12=np.float32(S.s12), n_inliers=int(S.n_inliers), iterations=int(S.iterations), status=int(S.status),
                inlier=keep["inlier"][:n].copy(), counts=keep["counts"].copy())


class ImuState(C.Structure):
    _fields_ = [("Rwb", C.c_double * 9), ("twb", C.c_double * 3), ("Rcw", C.c_double * 9), ("tcw", C.c_double * 3), ("v", C.c_double * 3),
                ("bg", C.c_double * 3), ("ba", C.c_double * 3)]


class ImuEstimate(C.Structure):
    _fields_ = [("Rwb", C.c_double * 9), ("twb", C.c_double * 3), ("v", C.c_double * 3), ("bg", C.c_double * 3), ("ba", C.c_double * 3)]


class PoseInertialProblem(C.Structure):
    _fields_ = [("mode", C.c_int32), ("n_obs", C.c_int32), ("n_rounds", C.c_int32), ("rec_init", C.c_int32), ("xw", C.c_void_p), ("obs", C.c_void_p),
                ("inv_sigma2", C.c_void_p), ("stereo", C.c_void_p), ("close", C.c_void_p), ("fx", C.c_double), ("fy", C.c_double),
                ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double), ("Rcb", C.c_double * 9), ("tcb", C.c_double * 3),
                ("Rbc", C.c_double * 9), ("tbc", C.c_double * 3), ("cur", ImuState), ("other", ImuState), ("dR", C.c_float * 9),
                ("dV", C.c_float * 3), ("dP", C.c_float * 3), ("JRg", C.c_float * 9), ("JVg", C.c_float * 9), ("JVa", C.c_float * 9),
                ("JPg", C.c_float * 9), ("JPa", C.c_float * 9), ("preint_bg", C.c_float * 3), ("preint_ba", C.c_float * 3), ("dT", C.c_float),
                ("info_inertial", C.c_double * 81), ("info_gyro_rw", C.c_double * 9), ("info_acc_rw", C.c_double * 9),
                ("prior_Rwb", C.c_double * 9), ("prior_twb", C.c_double * 3), ("prior_vwb", C.c_double * 3), ("prior_bg", C.c_double * 3),
                ("prior_ba", C.c_double * 3), ("prior_H", C.c_double * 225)]


class PoseInertialSolution(C.Structure):
    _fields_ = [("cur", ImuEstimate), ("other", ImuEstimate), ("outlier", C.c_void_p), ("n_good", C.c_int32), ("n_inliers", C.c_int32),
                ("rounds_run", C.c_int32), ("avg_reproj", C.c_float), ("H", C.c_double * 900)]


POSE_INERTIAL_LAST_KEYFRAME, POSE_INERTIAL_LAST_FRAME = 0, 1  # GFS_POSE_INERTIAL_* (include/gfs_abi.h)


def _fill(dst, src):
    a = np.ascontiguousarray(src).ravel()
    assert len(a) == len(dst), (len(a), len(dst))
    dst[:] = a.tolist()


def pose_inertial_structs(prob):
    """ctypes views of one problem dict (synth.pose_inertial_problem; shared with the CPU restatement's tests).  Arrays are row-major;
    keys as the fields of gfs_pose_inertial_problem, `cur` / `other` dicts of Rwb, twb, Rcw, tcw, v, bg, ba."""
    P, S = PoseInertialProblem(), PoseInertialSolution()
    n = int(prob["n_obs"])
    keep = dict(xw=np.ascontiguousarray(prob["xw"], np.float64).reshape(-1, 3), obs=np.ascontiguousarray(prob["obs"], np.float64).reshape(-1, 3),
                inv_sigma2=np.ascontiguousarray(prob["inv_sigma2"], np.float32), stereo=np.ascontiguousarray(prob["stereo"], np.uint8),
                close=np.ascontiguousarray(prob["close"], np.uint8), outlier=np.zeros(max(n, 1), np.uint8))
    P.mode, P.n_obs, P.n_rounds, P.rec_init = int(prob["mode"]), n, int(prob["n_rounds"]), int(prob["rec_init"])
    for name in ("xw", "obs", "inv_sigma2", "stereo", "close"):
        setattr(P, name, keep[name].ctypes.data if n > 0 or len(keep[name]) else None)
    for name in ("fx", "fy", "cx", "cy", "bf", "dT"):
        setattr(P, name, float(prob[name]))
    for name in ("Rcb", "tcb", "Rbc", "tbc", "dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "preint_bg", "preint_ba", "info_inertial",
                 "info_gyro_rw", "info_acc_rw", "prior_Rwb", "prior_twb", "prior_vwb", "prior_bg", "prior_ba", "prior_H"):
        _fill(getattr(P, name), prob[name])
    for end in ("cur", "other"):
        for name in ("Rwb", "twb", "Rcw", "tcw", "v", "bg", "ba"):
            _fill(getattr(getattr(P, end), name), prob[end][name])
    S.outlier = keep["outlier"].ctypes.data
    return P, S, keep, n


def pose_inertial_result(S, keep, n, mode):
    D = 30 if mode == POSE_INERTIAL_LAST_FRAME else 15
    est = lambda e: dict(Rwb=np.array(e.Rwb[:]).reshape(3, 3), twb=np.array(e.twb[:]), v=np.array(e.v[:]), bg=np.array(e.bg[:]), ba=np.array(e.ba[:]))
    return dict(cur=est(S.cur), other=est(S.other), outlier=keep["outlier"][:max(n, 0)].copy(), n_good=int(S.n_good), n_inliers=int(S.n_inliers),
                rounds_run=int(S.rounds_run), avg_reproj=np.float32(S.avg_reproj), H=np.array(S.H[:D * D]).reshape(D, D))


class PoseLidarInertialProblem(C.Structure):  # gfs_pose_lidar_inertial_problem
    _fields_ = [("vi", PoseInertialProblem), ("q", C.c_float * 4), ("t", C.c_float * 3), ("tcb_q", C.c_float * 4), ("tcb_t", C.c_float * 3),
                ("kf_time_gap", C.c_double), ("n_cloud", C.c_int32), ("cloud", C.c_void_p), ("map", C.c_void_p)]


class PoseLidarInertialSolution(C.Structure):  # gfs_pose_lidar_inertial_solution
    _fields_ = [("vi", PoseInertialSolution), ("n_lidar_inliers", C.c_int32), ("residual", C.c_float), ("round_edges", C.c_int32 * 4),
                ("round_chi2", C.c_float * 4), ("round_valid", C.c_int32 * 4)]


def pose_lidar_inertial_structs(prob, map_handle=None):
    """ctypes views of one problem dict (synth.pose_lidar_inertial_problem; shared with the CPU restatement's tests): the keys of
    pose_inertial_structs plus q, t (the stored float Tcw), tcb_q, tcb_t, kf_time_gap and cloud [n][3] (None: a null cloud)."""
    P, S = PoseLidarInertialProblem(), PoseLidarInertialSolution()
    P.vi, S.vi, keep, n = pose_inertial_structs(prob)
    cloud = np.zeros((0, 3), np.float32) if prob.get("cloud") is None else np.ascontiguousarray(prob["cloud"], np.float32).reshape(-1, 3)
    keep["cloud"] = cloud
    for name in ("q", "t", "tcb_q", "tcb_t"):
        _fill(getattr(P, name), np.asarray(prob[name], np.float32))
    P.kf_time_gap = float(prob["kf_time_gap"])
    P.n_cloud = len(cloud)
    P.cloud = cloud.ctypes.data if len(cloud) else None
    P.map = map_handle
    return P, S, keep, n


def pose_lidar_inertial_result(S, keep, n, mode):
    r = pose_inertial_result(S.vi, keep, n, mode)
    r.update(n_lidar_inliers=int(S.n_lidar_inliers), residual=np.float32(S.residual), round_edges=list(S.round_edges),
             round_chi2=np.array(S.round_chi2[:], np.float32), round_valid=list(S.round_valid))
    return r


class LbaInertialEdge(C.Structure):
    _fields_ = [("dR", C.c_float * 9), ("dV", C.c_float * 3), ("dP", C.c_float * 3), ("JRg", C.c_float * 9), ("JVg", C.c_float * 9),
                ("JVa", C.c_float * 9), ("JPg", C.c_float * 9), ("JPa", C.c_float * 9), ("preint_bg", C.c_float * 3), ("preint_ba", C.c_float * 3),
                ("dT", C.c_float), ("info_inertial", C.c_double * 81), ("info_gyro_rw", C.c_double * 9), ("info_acc_rw", C.c_double * 9)]


class LbaInertialProblem(C.Structure):
    _fields_ = [("n_opt", C.c_int32), ("n_fixed", C.c_int32), ("n_points", C.c_int32), ("n_edges", C.c_int32), ("iterations", C.c_int32),
                ("n_cameras", C.c_int32), ("lambda_init", C.c_double), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("bf", C.c_double), ("Rcb", C.c_double * 9), ("tcb", C.c_double * 3), ("Rbc", C.c_double * 9),
                ("tbc", C.c_double * 3), ("window", C.c_void_p), ("window_imu", C.c_void_p), ("prev", ImuState), ("fixed_Rcw", C.c_void_p),
                ("fixed_tcw", C.c_void_p), ("inertial", C.c_void_p), ("points", C.c_void_p), ("point_edge_begin", C.c_void_p),
                ("edge_kf", C.c_void_p), ("obs", C.c_void_p), ("inv_sigma2", C.c_void_p), ("stereo", C.c_void_p), ("close", C.c_void_p)]


class LbaInertialSolution(C.Structure):
    _fields_ = [("window", C.c_void_p), ("points", C.c_void_p), ("edge_chi2", C.c_void_p), ("edge_depth_positive", C.c_void_p),
                ("edge_erase", C.c_void_p), ("err", C.c_float), ("err_end", C.c_float), ("iterations_run", C.c_int32),
                ("trials_run", C.c_int32), ("final_lambda", C.c_double)]


_IMU_STATE_KEYS = ("Rwb", "twb", "Rcw", "tcw", "v", "bg", "ba")


def lba_inertial_structs(prob):
    """ctypes views of one window dict (synth.lba_inertial_window; shared with the CPU restatement's tests): keys as the fields of
    gfs_lba_inertial_problem, `window` a list of state dicts (Rwb, twb, Rcw, tcw, v, bg, ba), `prev` one, `inertial` a list of dicts
    with the fields of gfs_lba_inertial_edge.  A key whose value is None becomes a NULL pointer."""
    P, S = LbaInertialProblem(), LbaInertialSolution()
    N, F, n_pts, n_e = (int(prob[k]) for k in ("n_opt", "n_fixed", "n_points", "n_edges"))
    keep = dict(window=(ImuState * max(len(prob["window"]), 1))(), inertial=(LbaInertialEdge * max(len(prob["inertial"]), 1))(),
                out_window=(ImuState * max(N, 1))(), out_points=np.zeros((max(n_pts, 1), 3)), edge_chi2=np.zeros(max(n_e, 1)),
                edge_depth_positive=np.zeros(max(n_e, 1), np.uint8), edge_erase=np.zeros(max(n_e, 1), np.uint8))
    for i, st in enumerate(prob["window"]):
        for name in _IMU_STATE_KEYS:
            _fill(getattr(keep["window"][i], name), st[name])
    for i, ed in enumerate(prob["inertial"]):
        for name, _ in LbaInertialEdge._fields_:
            if name == "dT":
                keep["inertial"][i].dT = float(ed["dT"])
            else:
                _fill(getattr(keep["inertial"][i], name), ed[name])
    for name in _IMU_STATE_KEYS:
        _fill(getattr(P.prev, name), prob["prev"][name])
    for name, dt in (("window_imu", np.uint8), ("fixed_Rcw", np.float64), ("fixed_tcw", np.float64), ("points", np.float64),
                     ("point_edge_begin", np.int32), ("edge_kf", np.int32), ("obs", np.float64), ("inv_sigma2", np.float32), ("stereo", np.uint8),
                     ("close", np.uint8)):
        if prob.get(name) is None:
            setattr(P, name, None)
            continue
        a = np.ascontiguousarray(prob[name], dt)
        keep[name] = a if a.size else np.zeros(1, dt)
        setattr(P, name, keep[name].ctypes.data)
    P.window = C.addressof(keep["window"]) if prob.get("window_null") is None else None
    P.inertial = C.addressof(keep["inertial"]) if prob.get("inertial_null") is None else None
    P.n_opt, P.n_fixed, P.n_points, P.n_edges = N, F, n_pts, n_e
    P.iterations, P.n_cameras, P.lambda_init = int(prob["iterations"]), int(prob.get("n_cameras", 1)), float(prob["lambda_init"])
    for name in ("fx", "fy", "cx", "cy", "bf"):
        setattr(P, name, float(prob[name]))
    for name in ("Rcb", "tcb", "Rbc", "tbc"):
        _fill(getattr(P, name), prob[name])
    S.window, S.points = C.addressof(keep["out_window"]), keep["out_points"].ctypes.data
    S.edge_chi2, S.edge_depth_positive, S.edge_erase = (keep[k].ctypes.data for k in ("edge_chi2", "edge_depth_positive", "edge_erase"))
    return P, S, keep


def lba_inertial_result(S, keep, prob):
    N, n_pts, n_e = max(int(prob["n_opt"]), 0), max(int(prob["n_points"]), 0), max(int(prob["n_edges"]), 0)
    win = [{name: np.array(getattr(keep["out_window"][i], name)[:]).reshape((3, 3) if name[0] == "R" else (3,)) for name in _IMU_STATE_KEYS}
           for i in range(N)]
    return dict(window=win, points=keep["out_points"][:n_pts].copy(), edge_chi2=keep["edge_chi2"][:n_e].copy(),
                edge_depth_positive=keep["edge_depth_positive"][:n_e].copy(), edge_erase=keep["edge_erase"][:n_e].copy(), err=np.float32(S.err),
                err_end=np.float32(S.err_end), iterations_run=int(S.iterations_run), trials_run=int(S.trials_run),
                final_lambda=float(S.final_lambda))


class ClaheConfig(C.Structure):
    _fields_ = [("clip_limit", C.c_double), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32), ("residual_variant", C.c_int32)]


CLAHE_RESIDUAL_STEPPED, CLAHE_RESIDUAL_CONTIGUOUS = 0, 1  # GFS_CLAHE_RESIDUAL_* (include/gfs_abi.h)


class GmsProblem(C.Structure):
    _fields_ = [("n1", C.c_int32), ("n2", C.c_int32), ("kp1", C.c_void_p), ("kp2", C.c_void_p), ("width1", C.c_int32),
                ("height1", C.c_int32), ("width2", C.c_int32), ("height2", C.c_int32), ("n_matches", C.c_int32),
                ("query_idx", C.c_void_p), ("train_idx", C.c_void_p)]


class SbpProblem(C.Structure):
    _fields_ = [("n_last", C.c_int32), ("last_xw", C.c_void_p), ("last_desc", C.c_void_p), ("last_octave", C.c_void_p),
                ("last_angle", C.c_void_p), ("last_mp_has_obs", C.c_void_p), ("n_cur", C.c_int32), ("cur_kps_un", C.c_void_p),
                ("cur_u_right", C.c_void_p), ("cur_desc", C.c_void_p), ("cur_has_mp_obs", C.c_void_p),
                ("Tcw_q", C.c_float * 4), ("Tcw_t", C.c_float * 3), ("Tlw_q", C.c_float * 4), ("Tlw_t", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("b", C.c_float),
                ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("grid_w_inv", C.c_float), ("grid_h_inv", C.c_float), ("scale_factors", C.c_void_p), ("n_levels", C.c_int32),
                ("th", C.c_float), ("mono", C.c_int32), ("check_orientation", C.c_int32)]


class SbpMapProblem(C.Structure):
    _fields_ = [("n_mp", C.c_int32), ("mp_proj", C.c_void_p), ("mp_level", C.c_void_p), ("mp_view_cos", C.c_void_p),
                ("mp_desc", C.c_void_p), ("mp_has_obs", C.c_void_p), ("n_cur", C.c_int32), ("cur_kps_un", C.c_void_p),
                ("cur_u_right", C.c_void_p), ("cur_desc", C.c_void_p), ("cur_has_mp_obs", C.c_void_p), ("min_x", C.c_float),
                ("min_y", C.c_float), ("grid_w_inv", C.c_float), ("grid_h_inv", C.c_float), ("scale_factors", C.c_void_p),
                ("n_levels", C.c_int32), ("th", C.c_float), ("nn_ratio", C.c_float)]


class LocalPointsProblem(C.Structure):
    _fields_ = [("n_mp", C.c_int32), ("mp_xw", C.c_void_p), ("mp_normal", C.c_void_p), ("mp_min_dist", C.c_void_p),
                ("mp_max_dist", C.c_void_p), ("mp_desc", C.c_void_p), ("mp_has_obs", C.c_void_p), ("Rcw", C.c_float * 9),
                ("tcw", C.c_float * 3), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("bf", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float),
                ("max_y", C.c_float), ("grid_w_inv", C.c_float), ("grid_h_inv", C.c_float), ("scale_factors", C.c_void_p),
                ("n_levels", C.c_int32), ("log_scale_factor", C.c_float), ("view_cos_limit", C.c_float), ("far_points", C.c_int32),
                ("th_far_points", C.c_float), ("th", C.c_float), ("nn_ratio", C.c_float), ("n_cur", C.c_int32),
                ("cur_kps_un", C.c_void_p), ("cur_u_right", C.c_void_p), ("cur_desc", C.c_void_p), ("cur_has_mp_obs", C.c_void_p)]


class LocalPointsResult(C.Structure):
    _fields_ = [("in_view", C.c_void_p), ("proj", C.c_void_p), ("depth", C.c_void_p), ("view_cos", C.c_void_p), ("level", C.c_void_p),
                ("cur_match", C.c_void_p), ("n_to_match", C.c_int32), ("n_searched", C.c_int32), ("nmatches", C.c_int32)]


def local_points_structs(prob):
    """ctypes views of one SearchLocalPoints problem dict (keys of gfs_local_points_problem; shared with the CPU restatement's
    tests: same layout) -> (problem, result, arrays kept alive).  The result arrays are pre-filled with a pattern no output has."""
    P, R = LocalPointsProblem(), LocalPointsResult()
    keep = dict(mp_xw=np.ascontiguousarray(prob["mp_xw"], np.float32).reshape(-1, 3),
                mp_normal=np.ascontiguousarray(prob["mp_normal"], np.float32).reshape(-1, 3),
                mp_min_dist=np.ascontiguousarray(prob["mp_min_dist"], np.float32),
                mp_max_dist=np.ascontiguousarray(prob["mp_max_dist"], np.float32),
                mp_desc=np.ascontiguousarray(prob["mp_desc"], np.uint8).reshape(-1, 32),
                mp_has_obs=np.ascontiguousarray(prob["mp_has_obs"], np.uint8),
                cur_kps_un=np.ascontiguousarray(prob["cur_kps_un"], KP_DTYPE),
                cur_u_right=np.ascontiguousarray(prob["cur_u_right"], np.float32),
                cur_desc=np.ascontiguousarray(prob["cur_desc"], np.uint8).reshape(-1, 32),
                cur_has_mp_obs=np.ascontiguousarray(prob["cur_has_mp_obs"], np.uint8),
                scale_factors=np.ascontiguousarray(prob["scale_factors"], np.float32))
    n, nc = len(keep["mp_xw"]), len(keep["cur_kps_un"])
    P.n_mp, P.n_cur = n, nc
    for name, a in keep.items():
        setattr(P, name, a.ctypes.data)
    for name in ("Rcw", "tcw", "Ow"):
        getattr(P, name)[:] = [float(np.float32(v)) for v in np.asarray(prob[name]).reshape(-1)]
    for name in ("fx", "fy", "cx", "cy", "bf", "min_x", "max_x", "min_y", "max_y", "grid_w_inv", "grid_h_inv", "log_scale_factor",
                 "view_cos_limit", "th_far_points", "th", "nn_ratio"):
        setattr(P, name, float(np.float32(prob[name])))
    P.n_levels = int(prob.get("n_levels", len(keep["scale_factors"])))
    P.far_points = int(prob.get("far_points", 0))
    out = dict(in_view=np.full(max(n, 1), 0xEE, np.uint8), proj=np.full((max(n, 1), 3), -7.0, np.float32),
               depth=np.full(max(n, 1), -7.0, np.float32), view_cos=np.full(max(n, 1), -7.0, np.float32),
               level=np.full(max(n, 1), -9, np.int32), cur_match=np.full(max(nc, 1), -9, np.int32))
    for name, a in out.items():
        setattr(R, name, a.ctypes.data)
    keep.update(out)
    return P, R, keep


def local_points_result(P, R, keep):
    n, nc = P.n_mp, P.n_cur
    return dict(in_view=keep["in_view"][:n].copy(), proj=keep["proj"][:n].copy(), depth=keep["depth"][:n].copy(),
                view_cos=keep["view_cos"][:n].copy(), level=keep["level"][:n].copy(), cur_match=keep["cur_match"][:nc].copy(),
                n_to_match=int(R.n_to_match), n_searched=int(R.n_searched), nmatches=int(R.nmatches))


FUSE_EXITS = ("neg_depth", "not_in_image", "too_near", "too_far", "view_angle", "empty_window", "no_candidate", "matched")  # GFS_FUSE_*


class FusePoints(C.Structure):
    _fields_ = [("n_mp", C.c_int32), ("mp_xw", C.c_void_p), ("mp_normal", C.c_void_p), ("mp_min_dist", C.c_void_p),
                ("mp_max_dist", C.c_void_p), ("mp_desc", C.c_void_p)]


class FuseKeyframe(C.Structure):
    _fields_ = [("Tcw_q", C.c_float * 4), ("Tcw_t", C.c_float * 3), ("Ow", C.c_float * 3), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float),
                ("max_y", C.c_float), ("grid_w_inv", C.c_float), ("grid_h_inv", C.c_float), ("scale_factors", C.c_void_p),
                ("inv_level_sigma2", C.c_void_p), ("n_levels", C.c_int32), ("log_scale_factor", C.c_float), ("th", C.c_float),
                ("n_kp", C.c_int32), ("kps_un", C.c_void_p), ("u_right", C.c_void_p), ("desc", C.c_void_p), ("list", C.c_int32)]


class FuseResult(C.Structure):
    _fields_ = [("exit", C.c_void_p), ("best_idx", C.c_void_p), ("best_dist", C.c_void_p), ("level", C.c_void_p), ("n_matched", C.c_int32)]


def _fill_search_keyframe(K, src, arrays):
    """The fields gfs_fuse_keyframe and gfs_sim3_search_problem share, from the dict src: the pointers of `arrays` (named as the
    struct's fields), the pose, the intrinsics and image bounds, the level count, the key-point count and the list index."""
    for name, v in arrays.items():
        setattr(K, name, v.ctypes.data)
    for name in ("Tcw_q", "Tcw_t", "Ow"):
        getattr(K, name)[:] = [float(np.float32(v)) for v in np.asarray(src[name]).reshape(-1)]
    for name in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "grid_w_inv", "grid_h_inv", "log_scale_factor", "th"):
        setattr(K, name, float(np.float32(src[name])))
    K.n_levels = int(src.get("n_levels", len(arrays["scale_factors"])))
    K.n_kp = len(arrays["kps_un"])
    K.list = int(src.get("list", 0))


def _prefilled_results(R, n_mp):
    """Points a gfs_fuse_result at arrays for n_mp points, pre-filled with a pattern no output has -> the arrays by field name."""
    n = max(n_mp, 1)
    out = dict(exit=np.full(n, 0xEE, np.uint8), best_idx=np.full(n, -9, np.int32), best_dist=np.full(n, -9, np.int32),
               level=np.full(n, -9, np.int32))
    for name, v in out.items():
        setattr(R, name, v.ctypes.data)
    R.n_matched = -9
    return out


def fuse_structs(lists, keyframes):
    """ctypes views of one gfs_fuse_search call (shared with the CPU restatement's tests: same layout).  lists: dicts with the keys
    of gfs_fuse_points; keyframes: dicts with the keys of gfs_fuse_keyframe (kps_un = KP_DTYPE array; `list` defaults to 0)
    -> (lists array, key frames array, results array, arrays kept alive).  The result arrays are pre-filled with a pattern no
    output has."""
    nl, B = len(lists), len(keyframes)
    LL, KK, RR = (FusePoints * max(nl, 1))(), (FuseKeyframe * max(B, 1))(), (FuseResult * max(B, 1))()
    keep = []
    for l, pts in enumerate(lists):
        a = dict(mp_xw=np.ascontiguousarray(pts["mp_xw"], np.float32).reshape(-1, 3),
                 mp_normal=np.ascontiguousarray(pts["mp_normal"], np.float32).reshape(-1, 3),
                 mp_min_dist=np.ascontiguousarray(pts["mp_min_dist"], np.float32),
                 mp_max_dist=np.ascontiguousarray(pts["mp_max_dist"], np.float32),
                 mp_desc=np.ascontiguousarray(pts["mp_desc"], np.uint8).reshape(-1, 32))
        LL[l].n_mp = len(a["mp_xw"])
        for name, v in a.items():
            setattr(LL[l], name, v.ctypes.data)
        keep.append(a)
    for f, kf in enumerate(keyframes):
        a = dict(scale_factors=np.ascontiguousarray(kf["scale_factors"], np.float32),
                 inv_level_sigma2=np.ascontiguousarray(kf["inv_level_sigma2"], np.float32),
                 kps_un=np.ascontiguousarray(kf["kps_un"], KP_DTYPE), u_right=np.ascontiguousarray(kf["u_right"], np.float32),
                 desc=np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1, 32))
        K = KK[f]
        _fill_search_keyframe(K, kf, a)
        K.bf = float(np.float32(kf["bf"]))
        a.update(_prefilled_results(RR[f], LL[K.list].n_mp if 0 <= K.list < nl else 0))
        keep.append(a)
    return LL, KK, RR, keep


def fuse_results(LL, KK, RR, keep, n_lists):
    out = []
    for f in range(len(keep) - n_lists):
        a, n = keep[n_lists + f], LL[KK[f].list].n_mp
        out.append(dict(exit=a["exit"][:n].copy(), best_idx=a["best_idx"][:n].copy(), best_dist=a["best_dist"][:n].copy(),
                        level=a["level"][:n].copy(), n_matched=int(RR[f].n_matched)))
    return out


SIM3_FUSE, SIM3_SBP, SIM3_SBP_KFS = 0, 1, 2   # GFS_SIM3_*
SIM3_SEARCH_EXITS = FUSE_EXITS + ("skipped",)  # GFS_FUSE_* 0..7, GFS_FUSE_SKIPPED
SIM3_SEARCH_LISTED = 4                         # GFS_SIM3_SEARCH_LISTED
INT_MAX = 2147483647


class Sim3SearchProblem(C.Structure):
    _fields_ = [("mode", C.c_int32), ("ratio_hamming", C.c_float), ("Tcw_q", C.c_float * 4), ("Tcw_t", C.c_float * 3), ("Ow", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float),
                ("min_y", C.c_float), ("max_y", C.c_float), ("grid_w_inv", C.c_float), ("grid_h_inv", C.c_float),
                ("scale_factors", C.c_void_p), ("n_levels", C.c_int32), ("log_scale_factor", C.c_float), ("th", C.c_float),
                ("n_kp", C.c_int32), ("kps_un", C.c_void_p), ("desc", C.c_void_p), ("kp_taken", C.c_void_p), ("mp_skip", C.c_void_p),
                ("list", C.c_int32)]


Sim3SearchResult = FuseResult  # gfs_sim3_search_result has gfs_fuse_result's layout


def sim3_search_structs(lists, problems):
    """ctypes views of one gfs_sim3_search call (shared with the CPU restatement's tests: same layout).  lists: dicts with the keys
    of gfs_fuse_points; problems: dicts with the keys of gfs_sim3_search_problem (kps_un = KP_DTYPE array; `list` defaults to 0,
    ratio_hamming to 1, kp_taken and mp_skip to None = NULL) -> (lists array, problems array, results array, arrays kept alive).
    The result arrays are pre-filled with a pattern no output has."""
    nl, B = len(lists), len(problems)
    LL, _, _, keep = fuse_structs(lists, [])
    PP, RR = (Sim3SearchProblem * max(B, 1))(), (Sim3SearchResult * max(B, 1))()
    for f, pr in enumerate(problems):
        a = dict(scale_factors=np.ascontiguousarray(pr["scale_factors"], np.float32), kps_un=np.ascontiguousarray(pr["kps_un"], KP_DTYPE),
                 desc=np.ascontiguousarray(pr["desc"], np.uint8).reshape(-1, 32))
        for name in ("kp_taken", "mp_skip"):
            if pr.get(name) is not None:
                a[name] = np.ascontiguousarray(pr[name], np.uint8)
        K = PP[f]
        _fill_search_keyframe(K, pr, a)
        K.mode = int(pr["mode"])
        K.ratio_hamming = float(np.float32(pr.get("ratio_hamming", 1.0)))
        assert "kp_taken" not in a or len(a["kp_taken"]) == K.n_kp, "kp_taken must have one byte per key-point"
        assert "mp_skip" not in a or not (0 <= K.list < nl) or len(a["mp_skip"]) == LL[K.list].n_mp, "mp_skip must have one byte per listed point"
        a.update(_prefilled_results(RR[f], LL[K.list].n_mp if 0 <= K.list < nl else 0))
        keep.append(a)
    return LL, PP, RR, keep


def sim3_search_results(LL, PP, RR, keep, n_lists):
    return fuse_results(LL, PP, RR, keep, n_lists)


MAP_POINTS_FULL, MAP_POINTS_NORMALS_ONLY = 0, 1            # GFS_MAP_POINTS_*
MAP_POINT_OBS_IN_NORMAL, MAP_POINT_OBS_IN_DESC = 1, 2      # GFS_MAP_POINT_OBS_*
MAP_POINT_NORMAL_SET, MAP_POINT_DESC_SET = 1, 2            # GFS_MAP_POINT_*_SET


class MapPointsProblem(C.Structure):
    _fields_ = [("n_points", C.c_int32), ("mode", C.c_int32), ("obs_start", C.c_void_p), ("obs_Ow", C.c_void_p), ("obs_desc", C.c_void_p),
                ("obs_flags", C.c_void_p), ("pos", C.c_void_p), ("ref_Ow", C.c_void_p), ("level_scale", C.c_void_p),
                ("max_scale", C.c_void_p)]


class MapPointsResult(C.Structure):
    _fields_ = [("best_obs", C.c_void_p), ("best_median", C.c_void_p), ("normal", C.c_void_p), ("min_dist", C.c_void_p),
                ("max_dist", C.c_void_p), ("status", C.c_void_p)]


def map_points_structs(prob, normals_only=False):
    """ctypes views of one gfs_map_points_update call (shared with the CPU restatement's tests: same layout).  prob: a dict with the
    keys of gfs_map_points_problem (n_points is len(obs_start) - 1) -> (problem, result, arrays kept alive).  A normals-only call
    passes no descriptors.  The result arrays are pre-filled with a pattern no output has."""
    a = dict(obs_start=np.ascontiguousarray(prob["obs_start"], np.int32),
             obs_Ow=np.ascontiguousarray(prob["obs_Ow"], np.float32).reshape(-1, 3),
             obs_flags=np.ascontiguousarray(prob["obs_flags"], np.uint8),
             pos=np.ascontiguousarray(prob["pos"], np.float32).reshape(-1, 3),
             ref_Ow=np.ascontiguousarray(prob["ref_Ow"], np.float32).reshape(-1, 3),
             level_scale=np.ascontiguousarray(prob["level_scale"], np.float32),
             max_scale=np.ascontiguousarray(prob["max_scale"], np.float32))
    if not normals_only:
        a["obs_desc"] = np.ascontiguousarray(prob["obs_desc"], np.uint8).reshape(-1, 32)
    P, R = MapPointsProblem(), MapPointsResult()
    P.n_points = len(a["obs_start"]) - 1
    P.mode = MAP_POINTS_NORMALS_ONLY if normals_only else MAP_POINTS_FULL
    for name, v in a.items():
        setattr(P, name, v.ctypes.data)
    n = max(P.n_points, 1)
    out = dict(best_obs=np.full(n, -9, np.int32), best_median=np.full(n, -9, np.int32), normal=np.full((n, 3), -9.0, np.float32),
               min_dist=np.full(n, -9.0, np.float32), max_dist=np.full(n, -9.0, np.float32), status=np.full(n, 0xEE, np.uint8))
    for name, v in out.items():
        setattr(R, name, v.ctypes.data)
    a.update(out)
    return P, R, a


def map_points_results(P, keep):
    n = P.n_points
    return {k: keep[k][:n].copy() for k in ("best_obs", "best_median", "normal", "min_dist", "max_dist", "status")}


TRI_EXITS = ("no_match", "low_parallax", "svd_w_zero", "unproject_failed", "behind_1", "behind_2", "reproj_1", "reproj_2", "zero_dist", "far",
             "scale", "created")  # GFS_TRI_*


class TriKeyframe(C.Structure):
    _fields_ = [("Tcw", C.c_float * 12), ("Ow", C.c_float * 3), ("Rwc", C.c_float * 9), ("twc", C.c_float * 3), ("fx", C.c_float),
                ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("invfx", C.c_float), ("invfy", C.c_float), ("mbf", C.c_float),
                ("mb", C.c_float), ("scale_factors", C.c_void_p), ("level_sigma2", C.c_void_p), ("n_levels", C.c_int32), ("n_kp", C.c_int32),
                ("kps_un", C.c_void_p), ("kps", C.c_void_p), ("u_right", C.c_void_p), ("depth", C.c_void_p), ("desc", C.c_void_p),
                ("has_mp", C.c_void_p), ("n_nodes", C.c_int32), ("node_id", C.c_void_p), ("node_start", C.c_void_p), ("feat_idx", C.c_void_p)]


class TriNeighbour(C.Structure):
    _fields_ = [("kf", TriKeyframe), ("ep", C.c_float * 2), ("F12", C.c_float * 9)]


class TriProblem(C.Structure):
    _fields_ = [("cur", TriKeyframe), ("neighbours", C.POINTER(TriNeighbour)), ("n_neighbours", C.c_int32), ("only_stereo", C.c_int32),
                ("coarse", C.c_int32), ("check_orientation", C.c_int32), ("inertial", C.c_int32), ("far_points", C.c_int32),
                ("th_far_points", C.c_float), ("ratio_factor", C.c_float)]


class TriResult(C.Structure):
    _fields_ = [("match12", C.c_void_p), ("exit", C.c_void_p), ("x3d", C.c_void_p), ("point_stereo", C.c_void_p), ("n_matches", C.c_int32),
                ("n_created", C.c_int32)]


def _tri_keyframe(K, kf, keep):
    a = dict(scale_factors=np.ascontiguousarray(kf["scale_factors"], np.float32), level_sigma2=np.ascontiguousarray(kf["level_sigma2"], np.float32),
             kps_un=np.ascontiguousarray(kf["kps_un"], KP_DTYPE), kps=np.ascontiguousarray(kf["kps"], KP_DTYPE),
             u_right=np.ascontiguousarray(kf["u_right"], np.float32), depth=np.ascontiguousarray(kf["depth"], np.float32),
             desc=np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1, 32), has_mp=np.ascontiguousarray(kf["has_mp"], np.uint8),
             node_id=np.ascontiguousarray(kf["node_id"], np.int32), node_start=np.ascontiguousarray(kf["node_start"], np.int32),
             feat_idx=np.ascontiguousarray(kf["feat_idx"], np.int32))
    for name, v in a.items():
        setattr(K, name, v.ctypes.data)
    for name in ("Tcw", "Ow", "Rwc", "twc"):
        getattr(K, name)[:] = [float(np.float32(v)) for v in np.asarray(kf[name]).reshape(-1)]
    for name in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mbf", "mb"):
        setattr(K, name, float(np.float32(kf[name])))
    K.n_levels = int(kf.get("n_levels", len(a["scale_factors"])))
    K.n_kp = len(a["kps_un"])
    K.n_nodes = len(a["node_id"])
    keep.append(a)


def tri_structs(problems):
    """ctypes views of one gfs_create_new_map_points call (shared with the CPU restatement's tests: same layout).  problems: dicts
    with `cur` (keys of gfs_tri_keyframe; kps_un / kps = KP_DTYPE arrays), `neighbours` (the same keys plus ep, F12) and the flags of
    gfs_tri_problem -> (problems array, array of result pointers, arrays kept alive).  The result arrays are pre-filled with a pattern
    no output has."""
    B = len(problems)
    PP, RP = (TriProblem * max(B, 1))(), (C.POINTER(TriResult) * max(B, 1))()
    keep = []
    for b, prob in enumerate(problems):
        P, nbs = PP[b], list(prob["neighbours"])
        _tri_keyframe(P.cur, prob["cur"], keep)
        NN, RR = (TriNeighbour * max(len(nbs), 1))(), (TriResult * max(len(nbs), 1))()
        n, outs = max(P.cur.n_kp, 1), []
        for i, nb in enumerate(nbs):
            _tri_keyframe(NN[i].kf, nb, keep)
            NN[i].ep[:] = [float(np.float32(v)) for v in np.asarray(nb["ep"]).reshape(-1)]
            NN[i].F12[:] = [float(np.float32(v)) for v in np.asarray(nb["F12"]).reshape(-1)]
            out = dict(match12=np.full(n, -9, np.int32), exit=np.full(n, 0xEE, np.uint8), x3d=np.full((n, 3), np.nan, np.float32),
                       point_stereo=np.full(n, 0xEE, np.uint8))
            for name, v in out.items():
                setattr(RR[i], name, v.ctypes.data)
            RR[i].n_matches = RR[i].n_created = -9
            outs.append(out)
        P.neighbours, P.n_neighbours = NN, len(nbs)
        RP[b] = RR
        for name in ("only_stereo", "coarse", "check_orientation", "inertial", "far_points"):
            setattr(P, name, int(bool(prob.get(name, False))))
        P.th_far_points = float(np.float32(prob.get("th_far_points", 0.0)))
        P.ratio_factor = float(np.float32(prob["ratio_factor"]))
        keep.append((NN, RR, outs))
    return PP, RP, keep


def tri_results(PP, RP, keep, B):
    """-> per problem a list with one dict per neighbour: match12, exit (index into TRI_EXITS), x3d, point_stereo, n_matches, n_created."""
    res, blocks = [], [k for k in keep if isinstance(k, tuple)]
    for b in range(B):
        NN, RR, outs = blocks[b]
        n = PP[b].cur.n_kp
        res.append([dict(match12=o["match12"][:n].copy(), exit=o["exit"][:n].copy(), x3d=o["x3d"][:n].copy(),
                         point_stereo=o["point_stereo"][:n].copy(), n_matches=int(RR[i].n_matches), n_created=int(RR[i].n_created))
                    for i, o in enumerate(outs)])
    return res


def tri_candidate_pairs(prob):
    """Sum of n1 * n2 over the common nodes of all neighbours of a problem (what gfs_sbp_reserve_triangulation bounds)."""
    cur, total = prob["cur"], 0
    n1 = dict(zip(np.asarray(cur["node_id"]).tolist(), np.diff(np.asarray(cur["node_start"])).tolist()))
    for nb in prob["neighbours"]:
        for nid, n2 in zip(np.asarray(nb["node_id"]).tolist(), np.diff(np.asarray(nb["node_start"])).tolist()):
            total += n1.get(nid, 0) * n2
    return total


class BowKeyframe(C.Structure):  # gfs_bow_keyframe
    _fields_ = [("n_kp", C.c_int32), ("angle", C.c_void_p), ("desc", C.c_void_p), ("has_mp", C.c_void_p), ("n_nodes", C.c_int32),
                ("node_id", C.c_void_p), ("node_start", C.c_void_p), ("feat_idx", C.c_void_p)]


class BowProblem(C.Structure):  # gfs_bow_problem
    _fields_ = [("kf1", BowKeyframe), ("kf2", C.POINTER(BowKeyframe)), ("n_kf2", C.c_int32), ("nn_ratio", C.c_float),
                ("check_orientation", C.c_int32)]


class BowResult(C.Structure):  # gfs_bow_result
    _fields_ = [("match12", C.c_void_p), ("n_matches", C.c_int32)]


def _bow_keyframe(K, kf, keep):
    a = dict(angle=np.ascontiguousarray(kf["angle"], np.float32), desc=np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1, 32),
             has_mp=np.ascontiguousarray(kf["has_mp"], np.uint8), node_id=np.ascontiguousarray(kf["node_id"], np.int32),
             node_start=np.ascontiguousarray(kf["node_start"], np.int32), feat_idx=np.ascontiguousarray(kf["feat_idx"], np.int32))
    for name, v in a.items():
        setattr(K, name, v.ctypes.data)
    K.n_kp = len(a["angle"])
    K.n_nodes = len(a["node_id"])
    keep.append(a)


def bow_structs(problems):
    """ctypes views of one gfs_search_by_bow call (shared with the CPU restatement's tests: same layout).  problems: dicts with `kf1`
    (keys of gfs_bow_keyframe), `kf2` (a list of such dicts), nn_ratio and check_orientation -> (problems array, array of result
    pointers, arrays kept alive).  The result arrays are pre-filled with a pattern no output has."""
    B = len(problems)
    PP, RP = (BowProblem * max(B, 1))(), (C.POINTER(BowResult) * max(B, 1))()
    keep = []
    for b, prob in enumerate(problems):
        P, k2s = PP[b], list(prob["kf2"])
        _bow_keyframe(P.kf1, prob["kf1"], keep)
        KK, RR = (BowKeyframe * max(len(k2s), 1))(), (BowResult * max(len(k2s), 1))()
        n, outs = max(P.kf1.n_kp, 1), []
        for i, k2 in enumerate(k2s):
            _bow_keyframe(KK[i], k2, keep)
            out = np.full(n, -9, np.int32)
            RR[i].match12, RR[i].n_matches = out.ctypes.data, -9
            outs.append(out)
        P.kf2, P.n_kf2 = KK, len(k2s)
        P.nn_ratio = float(np.float32(prob["nn_ratio"]))
        P.check_orientation = int(bool(prob.get("check_orientation", True)))
        RP[b] = RR
        keep.append((KK, RR, outs))
    return PP, RP, keep


def bow_results(PP, RP, keep, B):
    """-> per problem a list with one dict per key frame 2: match12 [kf1.n_kp] (idx2 or -1), n_matches."""
    res, blocks = [], [k for k in keep if isinstance(k, tuple)]
    for b in range(B):
        KK, RR, outs = blocks[b]
        n = PP[b].kf1.n_kp
        res.append([dict(match12=o[:n].copy(), n_matches=int(RR[i].n_matches)) for i, o in enumerate(outs)])
    return res


class BowVocabularyStruct(C.Structure):  # gfs_bow_vocabulary
    _fields_ = [("k", C.c_int32), ("L", C.c_int32), ("scoring", C.c_int32), ("weighting", C.c_int32), ("n_nodes", C.c_int32),
                ("parent", C.c_void_p), ("child_start", C.c_void_p), ("children", C.c_void_p), ("desc", C.c_void_p), ("weight", C.c_void_p),
                ("word_id", C.c_void_p)]


class BowVectors(C.Structure):  # gfs_bow_vectors
    _fields_ = [("n_words", C.c_int32), ("word_id", C.c_void_p), ("word_value", C.c_void_p), ("n_nodes", C.c_int32), ("node_id", C.c_void_p),
                ("node_start", C.c_void_p), ("feat_idx", C.c_void_p), ("word_of_feature", C.c_void_p)]


def bow_vocabulary_struct(vocab):
    """vocab: dict(k, L, scoring, weighting, parent, child_start, children, desc [n_nodes, 32], weight, word_id) -> (struct, keep)"""
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    keep = dict(parent=i32(vocab["parent"]), child_start=i32(vocab["child_start"]), children=i32(vocab["children"]),
                desc=np.ascontiguousarray(vocab["desc"], np.uint8).reshape(-1, 32), weight=np.ascontiguousarray(vocab["weight"], np.float64),
                word_id=i32(vocab["word_id"]))
    V = BowVocabularyStruct(int(vocab["k"]), int(vocab["L"]), int(vocab.get("scoring", 0)), int(vocab.get("weighting", 0)),
                            int(vocab.get("n_nodes", len(keep["word_id"]))))
    for k, a in keep.items():
        setattr(V, k, a.ctypes.data)
    return V, keep


def bow_frames(descs):
    """one descriptor array [n, 32] or a list of them -> (single, [contiguous uint8 [n, 32]])"""
    single = isinstance(descs, np.ndarray)
    return single, [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in ([descs] if single else list(descs))]


def bow_vectors_alloc(B, cap, with_words=True):
    """B gfs_bow_vectors with arrays of `cap` entries (node_start cap + 1) -> (array of structs, keep)"""
    VV, keep = (BowVectors * max(B, 1))(), []
    for b in range(B):
        k = dict(word_id=np.full(cap, -7, np.int32), word_value=np.full(cap, np.nan), node_id=np.full(cap, -7, np.int32),
                 node_start=np.full(cap + 1, -7, np.int32), feat_idx=np.full(cap, -7, np.int32),
                 word_of_feature=np.full(cap, -7, np.int32) if with_words else None)
        for name, a in k.items():
            setattr(VV[b], name, a.ctypes.data if a is not None else None)
        keep.append(k)
    return VV, keep


def bow_vectors_results(VV, keep, counts):
    """-> per frame dict(word_id, word_value, node_id, node_start, feat_idx, word_of_feature): the BowVector in ascending word id, the
    FeatureVector in the layout of gfs_bow_keyframe, the word id of every feature (-1 when stopped)"""
    out = []
    for b, k in enumerate(keep):
        nw, nn = VV[b].n_words, VV[b].n_nodes
        m = int(k["node_start"][nn])
        out.append(dict(word_id=k["word_id"][:nw].copy(), word_value=k["word_value"][:nw].copy(), node_id=k["node_id"][:nn].copy(),
                        node_start=k["node_start"][:nn + 1].copy(), feat_idx=k["feat_idx"][:m].copy(),
                        word_of_feature=None if k["word_of_feature"] is None or counts is None else k["word_of_feature"][:counts[b]].copy()))
    return out


def sbp_map_struct(prob):
    P = SbpMapProblem()
    keep = dict(mp_proj=np.ascontiguousarray(prob["mp_proj"], np.float32).reshape(-1, 3),
                mp_level=np.ascontiguousarray(prob["mp_level"], np.int32),
                mp_view_cos=np.ascontiguousarray(prob["mp_view_cos"], np.float32),
                mp_desc=np.ascontiguousarray(prob["mp_desc"], np.uint8).reshape(-1, 32),
                mp_has_obs=np.ascontiguousarray(prob["mp_has_obs"], np.uint8),
                cur_kps_un=np.ascontiguousarray(prob["cur_kps_un"], KP_DTYPE),
                cur_u_right=np.ascontiguousarray(prob["cur_u_right"], np.float32),
                cur_desc=np.ascontiguousarray(prob["cur_desc"], np.uint8).reshape(-1, 32),
                cur_has_mp_obs=np.ascontiguousarray(prob["cur_has_mp_obs"], np.uint8),
                scale_factors=np.ascontiguousarray(prob["scale_factors"], np.float32))
    P.n_mp, P.n_cur = len(keep["mp_proj"]), len(keep["cur_kps_un"])
    for name, a in keep.items():
        setattr(P, name, a.ctypes.data)
    for name in ("min_x", "min_y", "grid_w_inv", "grid_h_inv", "th", "nn_ratio"):
        setattr(P, name, float(np.float32(prob[name])))
    P.n_levels = len(keep["scale_factors"])
    return P, keep


def sbp_struct(prob):
    """ctypes view of one SearchByProjection problem dict (keys as in gfs_sbp_problem; cur_kps_un = KP_DTYPE array)."""
    P = SbpProblem()
    keep = dict(last_xw=np.ascontiguousarray(prob["last_xw"], np.float32).reshape(-1, 3),
                last_desc=np.ascontiguousarray(prob["last_desc"], np.uint8).reshape(-1, 32),
                last_octave=np.ascontiguousarray(prob["last_octave"], np.int32),
                last_angle=np.ascontiguousarray(prob["last_angle"], np.float32),
                last_mp_has_obs=np.ascontiguousarray(prob["last_mp_has_obs"], np.uint8),
                cur_kps_un=np.ascontiguousarray(prob["cur_kps_un"], KP_DTYPE),
                cur_u_right=np.ascontiguousarray(prob["cur_u_right"], np.float32),
                cur_desc=np.ascontiguousarray(prob["cur_desc"], np.uint8).reshape(-1, 32),
                cur_has_mp_obs=np.ascontiguousarray(prob["cur_has_mp_obs"], np.uint8),
                scale_factors=np.ascontiguousarray(prob["scale_factors"], np.float32))
    P.n_last, P.n_cur = len(keep["last_xw"]), len(keep["cur_kps_un"])
    for name, a in keep.items():
        setattr(P, name, a.ctypes.data)
    for name in ("Tcw_q", "Tcw_t", "Tlw_q", "Tlw_t"):
        getattr(P, name)[:] = [float(np.float32(v)) for v in prob[name]]
    for name in ("fx", "fy", "cx", "cy", "bf", "b", "min_x", "max_x", "min_y", "max_y", "grid_w_inv", "grid_h_inv", "th"):
        setattr(P, name, float(np.float32(prob[name])))
    P.n_levels = len(keep["scale_factors"])
    P.mono = int(prob.get("mono", 0))
    P.check_orientation = int(prob.get("check_orientation", 1))
    return P, keep


class PoseLidarProblem(C.Structure):
    _fields_ = [("q", C.c_float * 4), ("t", C.c_float * 3), ("n_obs", C.c_int32), ("xw", C.c_void_p), ("obs", C.c_void_p),
                ("inv_sigma2", C.c_void_p), ("stereo", C.c_void_p), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("bf", C.c_double), ("n_cloud", C.c_int32), ("cloud", C.c_void_p), ("map", C.c_void_p),
                ("n_iterations", C.c_int32), ("two_camera", C.c_int32)]


class PoseLidarSolution(C.Structure):
    _fields_ = [("outlier", C.c_void_p), ("chi2", C.c_void_p), ("q", C.c_double * 4), ("t", C.c_double * 3), ("qf", C.c_float * 4),
                ("tf", C.c_float * 3), ("avg_reproj_error", C.c_float), ("n_inliers", C.c_int32), ("n_lidar_inliers", C.c_int32),
                ("residual", C.c_float), ("lidar_rounds", C.c_int32), ("rounds_run", C.c_int32), ("iterations_run", C.c_int32),
                ("round_edges", C.c_int32 * 4), ("round_chi2", C.c_float * 4), ("round_valid", C.c_int32 * 4)]


class LidarMapInput(C.Structure):
    _fields_ = [("n_keyframes", C.c_int32), ("q", C.c_void_p), ("t", C.c_void_p), ("cloud_begin", C.c_void_p), ("cloud", C.c_void_p),
                ("leaf", C.c_float)]


class LidarMapInfo(C.Structure):
    _fields_ = [("n_in", C.c_int32), ("n_out", C.c_int32), ("passthrough", C.c_int32), ("div", C.c_int32 * 3)]


class FrameCloudConfig(C.Structure):
    _fields_ = [("horizontal_angle", C.c_double), ("max_distance", C.c_double), ("local_map_resolution", C.c_double),
                ("downsize_resolution", C.c_float), ("angle_guard_deg", C.c_double)]


class FrameCloudInfo(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("n_in", "n_scans", "n_edge_raw", "n_surf_raw", "n_edge_voxel", "n_surf_voxel", "n_edge", "n_surf",
                                         "n_down", "host_scan_split")] + [("passthrough", C.c_int32 * 3)]


class FrameCloudStageBuffers(C.Structure):  # gfs_test_frame_cloud_stage_buffers (include/gfs_abi_test.h)
    _fields_ = [("scans", C.c_void_p), ("cap_scans", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("edge_raw", "surf_raw", "edge_voxel", "surf_voxel", "edge", "surf")] + [("cap_points", C.c_int32)]


def frame_cloud_info(I):
    d = {k: int(getattr(I, k)) for k, _ in FrameCloudInfo._fields_[:10]}
    d["passthrough"] = tuple(int(v) for v in I.passthrough)
    return d


def lidar_map_info(I):
    return dict(n_in=int(I.n_in), n_out=int(I.n_out), passthrough=int(I.passthrough), div=tuple(int(v) for v in I.div))


def pose_lidar_structs(prob, map_handle=None):
    """ctypes views of one PoseLidarVisualOptimization problem dict (shared with the CPU restatement's tests: same layout).
    prob: q, t (float Tcw), xw, obs, inv_sigma2, stereo, fx, fy, cx, cy, bf, cloud [n][3], n_iterations (+ optional
    n_lidar_inliers / residual: the caller's values of the in/out parameters, two_camera)."""
    P, S = PoseLidarProblem(), PoseLidarSolution()
    xw = np.ascontiguousarray(prob["xw"], np.float64).reshape(-1, 3)
    n = len(xw)
    cloud = np.ascontiguousarray(prob["cloud"], np.float32).reshape(-1, 3)
    keep = dict(xw=xw, obs=np.ascontiguousarray(prob["obs"], np.float64).reshape(-1, 3),
                inv_sigma2=np.ascontiguousarray(prob["inv_sigma2"], np.float32), stereo=np.ascontiguousarray(prob["stereo"], np.uint8),
                cloud=cloud, outlier=np.zeros(max(n, 1), np.uint8), chi2=np.zeros(max(n, 1), np.float64))
    P.q[:] = [float(v) for v in np.asarray(prob["q"], np.float32)]
    P.t[:] = [float(v) for v in np.asarray(prob["t"], np.float32)]
    P.n_obs = n
    for name in ("xw", "obs", "inv_sigma2", "stereo", "cloud"):
        setattr(P, name, keep[name].ctypes.data)
    for name in ("fx", "fy", "cx", "cy", "bf"):
        setattr(P, name, float(prob[name]))
    P.n_cloud = len(cloud)
    P.map = map_handle
    P.n_iterations = int(prob.get("n_iterations", 3))
    P.two_camera = int(prob.get("two_camera", 0))
    S.outlier = keep["outlier"].ctypes.data
    S.chi2 = keep["chi2"].ctypes.data
    S.n_lidar_inliers = int(prob.get("n_lidar_inliers", 0))
    S.residual = float(prob.get("residual", 0.0))
    return P, S, keep, n


def pose_lidar_result(S, keep, n):
    return dict(outlier=keep["outlier"][:n].astype(bool), chi2=keep["chi2"][:n].copy(), q=np.array(S.q[:]), t=np.array(S.t[:]),
                qf=np.array(S.qf[:], np.float32), tf=np.array(S.tf[:], np.float32), avg_reproj_error=np.float32(S.avg_reproj_error),
                n_inliers=int(S.n_inliers), n_lidar_inliers=int(S.n_lidar_inliers), residual=np.float32(S.residual),
                lidar_rounds=int(S.lidar_rounds), rounds_run=int(S.rounds_run), iterations_run=int(S.iterations_run),
                round_edges=list(S.round_edges), round_chi2=np.array(S.round_chi2[:], np.float32), round_valid=list(S.round_valid))


# every symbol include/gfs_abi.h declares (tests/test_abi.py checks the built library exports all of them)
ABI_SYMBOLS = [
    "gfs_abi_version", "gfs_last_error", "gfs_device_count",
    "gfs_orb_default_config", "gfs_orb_create", "gfs_orb_destroy", "gfs_orb_get_tables", "gfs_orb_max_keypoints",
    "gfs_orb_extract", "gfs_orb_extract_batch", "gfs_orb_extract_batch_device", "gfs_orb_device_results",
    "gfs_orb_fetch", "gfs_orb_level_size", "gfs_orb_fetch_level", "gfs_orb_fetch_candidates", "gfs_orb_octree_host",
    "gfs_orb_octree_device", "gfs_test_sort_replica", "gfs_test_heap_sort_replica", "gfs_test_glibc_math", "gfs_test_traffic",
    "gfs_test_orb_blur_tiles", "gfs_test_orb_geometry", "gfs_test_orb_last_paths",
    "gfs_hamming256", "gfs_matcher_create", "gfs_matcher_destroy", "gfs_bf_match_hamming",
    "gfs_bf_match_hamming_batch_device",
    "gfs_gicp_default_config", "gfs_gicp_create", "gfs_gicp_destroy", "gfs_gicp_align", "gfs_gicp_align_batch_device",
    "gfs_gicp_fetch_preprocessed", "gfs_gicp_tile_stats", "gfs_gicp_knn_stats", "gfs_gicp_coop_stats", "gfs_test_gicp_coop_hold", "gfs_test_gicp_coop_release", "gfs_test_gicp_coop_in_use", "gfs_frame_rgbd", "gfs_gicp_align_next", "gfs_gicp_align_next_batch_device", "gfs_test_voxel_sort", "gfs_test_voxel_sort_paths", "gfs_test_wave_std_sort",
    "gfs_lba_create", "gfs_lba_destroy", "gfs_lba_solve", "gfs_lba_solve_bool", "gfs_lba_linearize", "gfs_lba_batch_create", "gfs_lba_batch_destroy",
    "gfs_lba_solve_batch", "gfs_lba_lidar_reserve", "gfs_lba_solve_lidar", "gfs_lba_solve_lidar_bool", "gfs_lba_linearize_lidar",
    "gfs_lba_fetch_lidar_edges", "gfs_test_lba_stop_at_look", "gfs_test_lba_last_looks", "gfs_test_lba_first_trial",
    "gfs_gba_create", "gfs_gba_destroy", "gfs_gba_solve", "gfs_gba_solve_bool", "gfs_gba_last_info", "gfs_test_gba_first_trial",
    "gfs_test_gba_panel_rows", "gfs_test_gba_lists", "gfs_test_gba_tile_layout",
    "gfs_essential_graph_create", "gfs_essential_graph_destroy", "gfs_essential_graph_optimize", "gfs_essential_graph_correct_points",
    "gfs_essential_graph_last_info", "gfs_test_essential_graph_first_trial", "gfs_test_essential_graph_lists",
    "gfs_sim3_opt_create", "gfs_sim3_opt_destroy", "gfs_sim3_optimize", "gfs_test_glibc_exp",
    "gfs_sim3_ransac_iterations", "gfs_sim3_ransac_create", "gfs_sim3_ransac_solve", "gfs_sim3_ransac_destroy",
    "gfs_pose_inertial_create", "gfs_pose_inertial_optimize", "gfs_pose_inertial_destroy",
    "gfs_pose_lidar_inertial_create", "gfs_pose_lidar_inertial_optimize", "gfs_pose_lidar_inertial_destroy",
    "gfs_pose_lidar_inertial_fetch_edges",
    "gfs_lba_inertial_create", "gfs_lba_inertial_solve", "gfs_lba_inertial_destroy",
    "gfs_frame_create", "gfs_frame_destroy", "gfs_depth_to_cloud", "gfs_depth_to_cloud_batch_device", "gfs_depth_convert_u16_batch_device", "gfs_stereo_from_rgbd",
    "gfs_stereo_from_rgbd_batch_device",
    "gfs_pose_create", "gfs_pose_destroy", "gfs_pose_optimize", "gfs_pose_set_sum_order",
    "gfs_lidar_mapper_create", "gfs_lidar_mapper_destroy", "gfs_lidar_map_build", "gfs_lidar_map_fetch", "gfs_voxel_grid_filter",
    "gfs_test_lidar_map_grid",
    "gfs_frame_cloud_default_config", "gfs_frame_cloud_create", "gfs_frame_cloud_destroy", "gfs_frame_cloud_extract",
    "gfs_frame_cloud_extract_device", "gfs_test_frame_cloud_stages", "gfs_test_frame_cloud_radius",
    "gfs_lidar_map_create", "gfs_lidar_map_set", "gfs_lidar_map_destroy", "gfs_pose_lidar_create", "gfs_pose_lidar_destroy",
    "gfs_pose_lidar_set_sum_order", "gfs_pose_lidar_optimize", "gfs_pose_lidar_fetch_edges",
    "gfs_gms_create", "gfs_gms_destroy", "gfs_gms_inlier_mask", "gfs_gms_inlier_mask_batch_device",
    "gfs_sbp_create", "gfs_sbp_destroy", "gfs_search_by_projection", "gfs_search_by_projection_map",
    "gfs_sbp_reserve_local", "gfs_search_local_points", "gfs_sbp_reserve_fuse", "gfs_fuse_search", "gfs_test_glibc_logf",
    "gfs_sbp_reserve_sim3_search", "gfs_sim3_search", "gfs_test_sim3_search_groups",
    "gfs_sbp_reserve_triangulation", "gfs_create_new_map_points", "gfs_sbp_reserve_bow", "gfs_search_by_bow",
    "gfs_map_points_create", "gfs_map_points_destroy", "gfs_map_points_update",
    "gfs_bow_create", "gfs_bow_destroy", "gfs_bow_transform", "gfs_bow_transform_device",
    "gfs_bow_db_create", "gfs_bow_db_destroy", "gfs_bow_db_add", "gfs_bow_db_erase", "gfs_bow_db_query",
    "gfs_klt_create", "gfs_klt_destroy", "gfs_klt_layout", "gfs_klt_pyramid_create", "gfs_klt_pyramid_destroy",
    "gfs_klt_build_pyramid", "gfs_klt_build_pyramid_device", "gfs_klt_pyramid_download", "gfs_klt_track", "gfs_klt_fb_track",
    "gfs_klt_fb_track_device",
    "gfs_fmat_create", "gfs_fmat_destroy", "gfs_find_fundamental_ransac", "gfs_find_fundamental_ransac_device",
    "gfs_klt_compact_tracks_device", "gfs_klt_apply_mask_device",
    "gfs_clahe_default_config", "gfs_clahe_create", "gfs_clahe_destroy", "gfs_clahe_apply", "gfs_clahe_apply_device",
    "gfs_clahe_download_luts", "gfs_klt_build_pyramid_clahe", "gfs_klt_build_pyramid_clahe_device",
    "gfs_timer_create", "gfs_timer_destroy", "gfs_timer_start", "gfs_timer_stop", "gfs_timer_elapsed_ms",
    "gfs_profile_enable", "gfs_profile_report", "gfs_profile_reset",
]


def lib():
    """Load libgfs_hip.so (built in-tree by __graft_entry__.build()). Raises GfsError if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise GfsError(f"{_LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
        L = C.CDLL(_LIB_PATH)
        L.gfs_last_error.restype = C.c_char_p
        vp, ip, i = C.c_void_p, C.POINTER(C.c_int), C.c_int
        L.gfs_orb_default_config.argtypes = [C.POINTER(OrbConfig)]
        L.gfs_orb_create.argtypes = [C.POINTER(OrbConfig), C.POINTER(vp)]
        L.gfs_orb_destroy.argtypes = [vp]
        L.gfs_orb_get_tables.argtypes = [vp] * 7
        L.gfs_orb_max_keypoints.argtypes = [vp]
        L.gfs_orb_extract.argtypes = [vp, vp, i, i, i, i, i, vp, vp, i, ip]
        L.gfs_orb_extract_batch.argtypes = [vp, vp, i, i, i, i, i, i, vp, vp, i, vp, vp]
        L.gfs_orb_extract_batch_device.argtypes = [vp, vp, i, i, i, i, i, vp]
        L.gfs_orb_device_results.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), ip]
        L.gfs_orb_fetch.argtypes = [vp, i, vp, vp, i, ip, ip]
        L.gfs_orb_level_size.argtypes = [vp, i, ip, ip]
        L.gfs_orb_fetch_level.argtypes = [vp, i, i, i, vp]
        L.gfs_orb_fetch_candidates.argtypes = [vp, i, i, vp, vp, vp, i]
        L.gfs_test_orb_geometry.argtypes = [i, i, i, i, C.c_float, C.POINTER(OrbGeometryInfo), vp, i]
        L.gfs_test_orb_last_paths.argtypes = [vp, C.POINTER(OrbPaths)]
        L.gfs_orb_octree_host.argtypes = [vp, vp, vp, i, i, i, i, i, i, vp, i]
        L.gfs_orb_octree_device.argtypes = [i, vp, vp, vp, i, i, i, i, i, i, vp, vp, vp, i]
        L.gfs_test_glibc_math.argtypes = [i, vp, i, vp, vp, vp]
        L.gfs_test_glibc_logf.argtypes = [i, vp, i, vp]
        L.gfs_sbp_reserve_local.argtypes = [vp, i]
        L.gfs_search_local_points.argtypes = [vp, C.POINTER(LocalPointsProblem), i, C.POINTER(LocalPointsResult)]
        L.gfs_sbp_reserve_fuse.argtypes = [vp, i, i, i]
        L.gfs_fuse_search.argtypes = [vp, C.POINTER(FusePoints), i, C.POINTER(FuseKeyframe), i, C.POINTER(FuseResult)]
        L.gfs_sbp_reserve_sim3_search.argtypes = [vp, i, i, i]
        L.gfs_sim3_search.argtypes = [vp, C.POINTER(FusePoints), i, C.POINTER(Sim3SearchProblem), i, C.POINTER(Sim3SearchResult)]
        L.gfs_test_sim3_search_groups.argtypes = [vp, i]
        L.gfs_sbp_reserve_triangulation.argtypes = [vp, i, C.c_int64]
        L.gfs_create_new_map_points.argtypes = [vp, C.POINTER(TriProblem), i, C.POINTER(C.POINTER(TriResult))]
        L.gfs_sbp_reserve_bow.argtypes = [vp, i, i]
        L.gfs_search_by_bow.argtypes = [vp, C.POINTER(BowProblem), i, C.POINTER(C.POINTER(BowResult))]
        L.gfs_map_points_create.argtypes = [i, i, i, C.POINTER(vp)]
        L.gfs_map_points_destroy.argtypes = [vp]
        L.gfs_map_points_update.argtypes = [vp, C.POINTER(MapPointsProblem), C.POINTER(MapPointsResult)]
        L.gfs_test_traffic.argtypes = [i, i, C.c_longlong, C.c_longlong, i, C.POINTER(C.c_longlong)]
        L.gfs_hamming256.argtypes = [vp, vp]
        L.gfs_matcher_create.argtypes = [i, i, i, i, C.POINTER(vp)]
        L.gfs_matcher_destroy.argtypes = [vp]
        L.gfs_bf_match_hamming.argtypes = [vp, vp, i, vp, i, vp, vp]
        L.gfs_bf_match_hamming_batch_device.argtypes = [vp, vp, vp, vp, vp, i, i, vp, vp, vp]
        if hasattr(L, "gfs_gicp_create"):
            L.gfs_gicp_default_config.argtypes = [C.POINTER(GicpConfig)]
            L.gfs_gicp_create.argtypes = [i, i, i, C.POINTER(vp)]
            L.gfs_gicp_destroy.argtypes = [vp]
            L.gfs_gicp_align.argtypes = [vp, vp, i, vp, i, vp, C.POINTER(GicpConfig), C.POINTER(GicpResult)]
            L.gfs_gicp_align_batch_device.argtypes = [vp, vp, vp, vp, vp, i, i, vp, C.POINTER(GicpConfig), vp, vp]
            L.gfs_gicp_fetch_preprocessed.argtypes = [vp, i, i, vp, vp, i, ip]
            L.gfs_gicp_tile_stats.argtypes = [vp, vp, i]
            L.gfs_gicp_knn_stats.argtypes = [vp, i, i, vp, vp, i]
            L.gfs_gicp_coop_stats.argtypes = [vp, vp]
            L.gfs_test_gicp_coop_hold.argtypes = [vp, i]
            L.gfs_test_gicp_coop_release.argtypes = [vp, i]
            L.gfs_test_gicp_coop_in_use.argtypes = [i]
            L.gfs_test_voxel_sort.argtypes = [vp, vp, i, vp]
            L.gfs_test_voxel_sort_paths.argtypes = [vp, vp]
            L.gfs_test_wave_std_sort.argtypes = [i, vp, i, vp]
            L.gfs_gicp_align_next.argtypes = [vp, vp, i, vp, C.POINTER(GicpConfig), C.POINTER(GicpResult)]
            L.gfs_gicp_align_next_batch_device.argtypes = [vp, vp, vp, i, i, vp, C.POINTER(GicpConfig), vp, vp]
        if hasattr(L, "gfs_lba_create"):
            L.gfs_lba_create.argtypes = [i, i, i, i, C.POINTER(vp)]
            L.gfs_lba_destroy.argtypes = [vp]
            L.gfs_lba_solve.argtypes = [vp, C.POINTER(LbaProblem), C.POINTER(LbaSolution), vp]
            L.gfs_lba_solve_bool.argtypes = [vp, C.POINTER(LbaProblem), C.POINTER(LbaSolution), vp]
            L.gfs_lba_linearize.argtypes = [vp, C.POINTER(LbaProblem), vp, vp, vp, vp, vp, vp, C.POINTER(C.c_double)]
            L.gfs_lba_batch_create.argtypes = [i, i, i, i, i, C.POINTER(vp)]
            L.gfs_lba_batch_destroy.argtypes = [vp]
            L.gfs_lba_solve_batch.argtypes = [vp, vp, vp, i, vp]
            L.gfs_test_lba_stop_at_look.argtypes = [i]
            L.gfs_test_lba_last_looks.argtypes = [C.POINTER(C.c_int32)] * 4
            L.gfs_test_lba_first_trial.argtypes = [vp, C.POINTER(LbaProblem), C.POINTER(LbaTrial)]
        if hasattr(L, "gfs_gba_create"):
            L.gfs_gba_create.argtypes = [i, i, i, i, C.POINTER(vp)]
            L.gfs_gba_destroy.argtypes = [vp]
            L.gfs_gba_solve.argtypes = [vp, C.POINTER(LbaProblem), C.POINTER(LbaSolution), vp]
            L.gfs_gba_solve_bool.argtypes = [vp, C.POINTER(LbaProblem), C.POINTER(LbaSolution), vp]
            L.gfs_gba_last_info.argtypes = [vp, C.POINTER(GbaInfo)]
            L.gfs_test_gba_first_trial.argtypes = [vp, C.POINTER(LbaProblem), C.POINTER(LbaTrial)]
            L.gfs_test_gba_panel_rows.argtypes = []
            L.gfs_test_gba_lists.argtypes = [i, i, i, vp, vp, vp, vp, vp, vp, vp, C.c_int64, vp, C.c_int64, vp, vp]
            L.gfs_test_gba_tile_layout.argtypes = [C.c_int64, C.c_int64, C.c_int64, vp]
        if hasattr(L, "gfs_essential_graph_create"):
            L.gfs_essential_graph_create.argtypes = [i, i, i, i, C.POINTER(vp)]
            L.gfs_essential_graph_destroy.argtypes = [vp]
            L.gfs_essential_graph_optimize.argtypes = [vp, C.POINTER(EssentialGraphProblem), C.POINTER(EssentialGraphSolution)]
            L.gfs_essential_graph_correct_points.argtypes = [vp, i, vp, vp, i, vp, vp, vp]
            L.gfs_essential_graph_last_info.argtypes = [vp, C.POINTER(EssentialGraphInfo)]
            L.gfs_test_essential_graph_first_trial.argtypes = [vp, C.POINTER(EssentialGraphProblem), C.POINTER(EssentialGraphTrial)]
            L.gfs_test_essential_graph_lists.argtypes = [i, i, vp, vp, vp, vp, vp, vp, vp, C.c_int64, vp, C.c_int64]
        if hasattr(L, "gfs_sim3_opt_create"):
            L.gfs_sim3_opt_create.argtypes = [i, i, i, C.POINTER(vp)]
            L.gfs_sim3_opt_destroy.argtypes = [vp]
            L.gfs_sim3_optimize.argtypes = [vp, vp, i, vp]
            L.gfs_test_glibc_exp.argtypes = [i, vp, i, vp]
        if hasattr(L, "gfs_pose_inertial_create"):
            L.gfs_pose_inertial_create.argtypes = [i, i, i, C.POINTER(vp)]
            L.gfs_pose_inertial_destroy.argtypes = [vp]
            L.gfs_pose_inertial_optimize.argtypes = [vp, vp, i, vp]
        if hasattr(L, "gfs_pose_lidar_inertial_create"):
            L.gfs_pose_lidar_inertial_create.argtypes = [i, i, i, i, C.POINTER(vp)]
            L.gfs_pose_lidar_inertial_destroy.argtypes = [vp]
            L.gfs_pose_lidar_inertial_optimize.argtypes = [vp, vp, i, vp]
            L.gfs_pose_lidar_inertial_fetch_edges.argtypes = [vp, i, i, vp, vp, vp, i, C.POINTER(C.c_int32)]
        if hasattr(L, "gfs_lba_inertial_create"):
            L.gfs_lba_inertial_create.argtypes = [i, i, i, i, i, C.POINTER(vp)]
            L.gfs_lba_inertial_destroy.argtypes = [vp]
            L.gfs_lba_inertial_solve.argtypes = [vp, C.POINTER(LbaInertialProblem), C.POINTER(LbaInertialSolution)]
        if hasattr(L, "gfs_sim3_ransac_create"):
            L.gfs_sim3_ransac_iterations.argtypes = [i, C.c_double, i, i]
            L.gfs_sim3_ransac_create.argtypes = [i, i, i, i, C.POINTER(vp)]
            L.gfs_sim3_ransac_destroy.argtypes = [vp]
            L.gfs_sim3_ransac_solve.argtypes = [vp, vp, i, vp]
        L.gfs_bow_create.argtypes = [i, C.POINTER(BowVocabularyStruct), i, i, C.POINTER(vp)]
        L.gfs_bow_destroy.argtypes = [vp]
        L.gfs_bow_destroy.restype = None
        L.gfs_bow_transform.argtypes = [vp, C.POINTER(vp), vp, i, i, C.POINTER(BowVectors)]
        L.gfs_bow_transform_device.argtypes = [vp, vp, vp, i, i, i, C.POINTER(BowVectors)]
        L.gfs_bow_db_create.argtypes = [i, i, i, C.POINTER(vp)]
        L.gfs_bow_db_destroy.argtypes = [vp]
        L.gfs_bow_db_destroy.restype = None
        L.gfs_bow_db_add.argtypes = [vp, i, i, vp, vp]
        L.gfs_bow_db_erase.argtypes = [vp, i]
        L.gfs_bow_db_query.argtypes = [vp, i, vp, vp, vp, vp, vp]
        if hasattr(L, "gfs_lba_solve_lidar"):
            L.gfs_lba_lidar_reserve.argtypes = [vp, i]
            L.gfs_lba_solve_lidar.argtypes = [vp, C.POINTER(LbaProblem), C.POINTER(LbaLidar), C.POINTER(LbaSolution), vp, vp]
            L.gfs_lba_solve_lidar_bool.argtypes = [vp, C.POINTER(LbaProblem), C.POINTER(LbaLidar), C.POINTER(LbaSolution), vp, vp]
            L.gfs_lba_linearize_lidar.argtypes = [vp, C.POINTER(LbaProblem), C.POINTER(LbaLidar), vp, vp, vp, vp, vp, vp,
                                                  C.POINTER(C.c_double), vp, i, vp]
            L.gfs_lba_fetch_lidar_edges.argtypes = [vp, i, vp, vp, vp, i, vp]
        if hasattr(L, "gfs_lidar_map_build"):
            L.gfs_lidar_mapper_create.argtypes = [i, i, i, C.POINTER(vp)]
            L.gfs_lidar_mapper_destroy.argtypes = [vp]
            L.gfs_lidar_map_build.argtypes = [vp, C.POINTER(LidarMapInput), vp, C.POINTER(LidarMapInfo)]
            L.gfs_lidar_map_fetch.argtypes = [vp, vp, i, C.POINTER(C.c_int32)]
            L.gfs_voxel_grid_filter.argtypes = [vp, vp, i, C.c_float, vp, i, C.POINTER(LidarMapInfo)]
            L.gfs_test_lidar_map_grid.argtypes = [vp, vp, i, vp, vp, i, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.gfs_frame_cloud_default_config.argtypes = [C.POINTER(FrameCloudConfig)]
        L.gfs_frame_cloud_default_config.restype = None
        L.gfs_frame_cloud_create.argtypes = [i, i, C.POINTER(FrameCloudConfig), C.POINTER(vp)]
        L.gfs_frame_cloud_destroy.argtypes = [vp]
        L.gfs_frame_cloud_extract.argtypes = [vp, vp, i, vp, i, vp, i, C.POINTER(FrameCloudInfo)]
        L.gfs_frame_cloud_extract_device.argtypes = [vp, vp, vp, vp, i, vp, i, C.POINTER(FrameCloudInfo)]
        L.gfs_test_frame_cloud_stages.argtypes = [vp, C.POINTER(FrameCloudStageBuffers)]
        L.gfs_test_frame_cloud_radius.argtypes = [vp, vp, i, i, vp, i, C.POINTER(C.c_int32)]
        if hasattr(L, "gfs_frame_create"):
            f = C.c_float
            L.gfs_frame_create.argtypes = [i, i, i, i, C.POINTER(vp)]
            L.gfs_frame_destroy.argtypes = [vp]
            L.gfs_depth_to_cloud.argtypes = [vp, vp, i, i, i, i, f, f, f, f, vp, i, ip]
            L.gfs_depth_to_cloud_batch_device.argtypes = [vp, vp, i, i, i, i, f, f, f, f, vp, i, vp, vp]
            L.gfs_depth_convert_u16_batch_device.argtypes = [vp, vp, i, i, i, f, vp, vp]
            L.gfs_stereo_from_rgbd.argtypes = [vp, vp, vp, i, vp, i, i, i, f, vp, vp]
            L.gfs_frame_rgbd.argtypes = [vp, vp, vp, i, vp, i, i, i, f, i, f, f, f, f, vp, vp, vp, i, ip, vp, vp, ip]
            L.gfs_stereo_from_rgbd_batch_device.argtypes = [vp, vp, vp, vp, i, i, vp, i, i, f, vp, vp, vp]
        if hasattr(L, "gfs_klt_create"):
            f, d = C.c_float, C.c_double
            L.gfs_klt_create.argtypes = [i, i, i, i, i, i, i, C.POINTER(vp)]
            L.gfs_klt_destroy.argtypes = [vp]
            L.gfs_klt_layout.argtypes = [vp, vp, vp, vp]
            L.gfs_klt_pyramid_create.argtypes = [vp, C.POINTER(vp)]
            L.gfs_klt_pyramid_destroy.argtypes = [vp]
            L.gfs_klt_build_pyramid.argtypes = [vp, vp, vp, i, i]
            L.gfs_klt_build_pyramid_device.argtypes = [vp, vp, vp, i, i, vp]
            L.gfs_klt_pyramid_download.argtypes = [vp, vp, i, vp, vp]
            L.gfs_klt_track.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp, i, i, d, i, d]
            L.gfs_klt_fb_track.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, vp, i, f, f]
            L.gfs_klt_fb_track_device.argtypes = [vp, vp, vp, i, i, vp, vp, vp, vp, vp, i, f, f, vp]
            L.gfs_klt_compact_tracks_device.argtypes = [vp, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp]
            L.gfs_klt_apply_mask_device.argtypes = [vp, i, i, vp, vp, vp, vp, vp]
        L.gfs_clahe_default_config.argtypes = [C.POINTER(ClaheConfig)]
        L.gfs_clahe_default_config.restype = None
        L.gfs_clahe_create.argtypes = [i, i, i, i, C.POINTER(ClaheConfig), C.POINTER(vp)]
        L.gfs_clahe_destroy.argtypes = [vp]
        L.gfs_clahe_apply.argtypes = [vp, vp, i, i, i, i, vp, i]
        L.gfs_clahe_apply_device.argtypes = [vp, vp, i, i, i, i, vp, i, vp]
        L.gfs_clahe_download_luts.argtypes = [vp, i, vp]
        L.gfs_klt_build_pyramid_clahe.argtypes = [vp, vp, vp, vp, i, i, vp, i]
        L.gfs_klt_build_pyramid_clahe_device.argtypes = [vp, vp, vp, vp, i, i, vp, i, vp]
        if hasattr(L, "gfs_fmat_create"):
            L.gfs_fmat_create.argtypes = [i, i, i, C.POINTER(vp)]
            L.gfs_fmat_destroy.argtypes = [vp]
            L.gfs_find_fundamental_ransac.argtypes = [vp, i, vp, vp, vp, C.c_double, C.c_double, i, vp, vp, vp]
            L.gfs_find_fundamental_ransac_device.argtypes = [vp, i, i, vp, vp, vp, C.c_double, C.c_double, i, vp, vp, vp]
        L.gfs_timer_create.argtypes = [i, C.POINTER(vp)]
        L.gfs_timer_destroy.argtypes = [vp]
        L.gfs_timer_start.argtypes = [vp, vp]
        L.gfs_timer_stop.argtypes = [vp, vp]
        L.gfs_timer_elapsed_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.gfs_profile_report.argtypes = [vp, vp, vp, i]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _check(rc, what):
    if rc < 0:
        err = GfsError(f"{what} failed ({rc}): {lib().gfs_last_error().decode()}")
        err.code = rc  # GFS_ERR_* (include/gfs_abi.h)
        raise err
    return rc


def device_count():
    return lib().gfs_device_count()


class ORBextractor:
    """ORB_SLAM3::ORBextractor (reference include/ORBextractor.h:46-118) backed by gfs_orb_*."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7, max_rows=480,
                 max_cols=640, max_batch=1, device=0, blur_taps_variant=0):
        L = lib()
        cfg = OrbConfig()
        L.gfs_orb_default_config(C.byref(cfg))
        cfg.nfeatures, cfg.scale_factor, cfg.nlevels = nfeatures, scaleFactor, nlevels
        cfg.ini_th_fast, cfg.min_th_fast = iniThFAST, minThFAST
        cfg.max_rows, cfg.max_cols, cfg.max_batch, cfg.device = max_rows, max_cols, max_batch, device
        cfg.blur_taps_variant = blur_taps_variant
        self.nlevels = nlevels
        self.h = C.c_void_p()
        _check(L.gfs_orb_create(C.byref(cfg), C.byref(self.h)), "gfs_orb_create")
        self.cap = L.gfs_orb_max_keypoints(self.h)

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_orb_destroy(self.h)
        self.h = None

    __del__ = close

    def GetLevels(self):
        return self.nlevels

    def tables(self):
        n = self.nlevels
        sc, inv, s2, is2 = (np.zeros(n, np.float32) for _ in range(4))
        feats = np.zeros(n, np.int32)
        umax = np.zeros(16, np.int32)
        _check(lib().gfs_orb_get_tables(self.h, _p(sc), _p(inv), _p(s2), _p(is2), _p(feats), _p(umax)), "get_tables")
        return dict(scale=sc, inv_scale=inv, sigma2=s2, inv_sigma2=is2, feats=feats, umax=umax)

    def GetScaleFactors(self):
        return self.tables()["scale"]

    def GetInverseScaleFactors(self):
        return self.tables()["inv_scale"]

    def GetScaleSigmaSquares(self):
        return self.tables()["sigma2"]

    def GetInverseScaleSigmaSquares(self):
        return self.tables()["inv_sigma2"]

    def __call__(self, image, vLappingArea=(0, 0)):
        """operator(): -> (monoIndex or -1, keypoints[KP_DTYPE], descriptors [N,32] u8)"""
        if image is None or image.size == 0:
            return -1, np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        assert image.dtype == np.uint8 and image.ndim == 2, "CV_8UC1 expected (src/ORBextractor.cc:1153)"
        stride = image.strides[0]
        assert image.strides[1] == 1
        kps = np.zeros(self.cap, KP_DTYPE)
        desc = np.zeros((self.cap, 32), np.uint8)
        n = C.c_int(0)
        r = lib().gfs_orb_extract(self.h, C.c_void_p(image.ctypes.data), image.shape[0], image.shape[1], stride,
                                  vLappingArea[0], vLappingArea[1], _p(kps), _p(desc), self.cap, C.byref(n))
        if r < -1:
            err = GfsError(f"gfs_orb_extract failed ({r + 100}): {lib().gfs_last_error().decode()}")
            err.code = r + 100  # GFS_ERR_* (include/gfs_abi.h)
            raise err
        return r, kps[:n.value].copy(), desc[:n.value].copy()

    def extract_batch(self, images, vLappingArea=(0, 0)):
        imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
        B = len(imgs)
        rows, cols = imgs[0].shape
        ptrs = (C.c_void_p * B)(*[im.ctypes.data for im in imgs])
        kps = np.zeros((B, self.cap), KP_DTYPE)
        desc = np.zeros((B, self.cap, 32), np.uint8)
        n = np.zeros(B, np.int32)
        mono = np.zeros(B, np.int32)
        _check(lib().gfs_orb_extract_batch(self.h, ptrs, B, rows, cols, cols, vLappingArea[0], vLappingArea[1], _p(kps),
                                           _p(desc), self.cap, _p(n), _p(mono)), "gfs_orb_extract_batch")
        return [(int(mono[b]), kps[b, :n[b]].copy(), desc[b, :n[b]].copy()) for b in range(B)]

    def extract_batch_device(self, dev_ptr, B, rows, cols, vLappingArea=(0, 0), stream=None):
        _check(lib().gfs_orb_extract_batch_device(self.h, C.c_void_p(dev_ptr), B, rows, cols, vLappingArea[0],
                                                  vLappingArea[1], C.c_void_p(stream) if stream else None),
               "gfs_orb_extract_batch_device")

    def device_results(self):
        k, d, c, m = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        cap = C.c_int()
        _check(lib().gfs_orb_device_results(self.h, C.byref(k), C.byref(d), C.byref(c), C.byref(m), C.byref(cap)),
               "gfs_orb_device_results")
        return dict(kps=k.value, desc=d.value, counts=c.value, mono=m.value, cap=cap.value)

    def fetch(self, b):
        kps = np.zeros(self.cap, KP_DTYPE)
        desc = np.zeros((self.cap, 32), np.uint8)
        n, mono = C.c_int(), C.c_int()
        _check(lib().gfs_orb_fetch(self.h, b, _p(kps), _p(desc), self.cap, C.byref(n), C.byref(mono)), "gfs_orb_fetch")
        return mono.value, kps[:n.value].copy(), desc[:n.value].copy()

    def level_size(self, l):
        r, c = C.c_int(), C.c_int()
        _check(lib().gfs_orb_level_size(self.h, l, C.byref(r), C.byref(c)), "gfs_orb_level_size")
        return r.value, c.value

    def level(self, l, b=0, blurred=False):
        r, c = self.level_size(l)
        a = np.zeros((r, c), np.uint8)
        _check(lib().gfs_orb_fetch_level(self.h, b, l, int(blurred), _p(a)), "gfs_orb_fetch_level")
        return a

    def candidates(self, l, b=0):
        n = _check(lib().gfs_orb_fetch_candidates(self.h, b, l, None, None, None, 0), "gfs_orb_fetch_candidates")
        x, y, s = (np.zeros(max(n, 1), np.int32) for _ in range(3))
        lib().gfs_orb_fetch_candidates(self.h, b, l, _p(x), _p(y), _p(s), n)
        return x[:n], y[:n], s[:n]


    def last_paths(self):
        """gfs_test_orb_last_paths: the paths of the handle's last call and its count of geometry rebuilds (test hook)."""
        P = OrbPaths()
        _check(lib().gfs_test_orb_last_paths(self.h, C.byref(P)), "gfs_test_orb_last_paths")
        return {n: int(getattr(P, n)) for n, _ in OrbPaths._fields_}


def orb_geometry(rows, cols, nfeatures=1000, nlevels=8, scale_factor=1.2):
    """gfs_test_orb_geometry (host only): what OrbGeometry::build decides for rows x cols -> dict of the frame's figures with
    "levels": a list of per-level dicts; "supported" is False (and "levels" empty) for a size build refuses."""
    I = OrbGeometryInfo()
    Lv = (OrbLevelInfo * nlevels)()
    rc = lib().gfs_test_orb_geometry(rows, cols, nfeatures, nlevels, scale_factor, C.byref(I), C.cast(Lv, C.c_void_p), nlevels)
    out = {n: int(getattr(I, n)) for n, _ in OrbGeometryInfo._fields_}
    out["supported"] = bool(out["supported"])
    if rc == -5:  # GFS_ERR_UNSUPPORTED: build refuses the size
        return dict(out, levels=[])
    _check(rc, "gfs_test_orb_geometry")
    return dict(out, levels=[{n: int(getattr(Lv[l], n)) for n, _ in OrbLevelInfo._fields_} for l in range(nlevels)])


def wave_std_sort_perm(keys, device=0):
    """csrc/wave_std_sort.hpp on the GPU: the permutation std::sort leaves (test hook)."""
    k = np.ascontiguousarray(keys, np.uint32)
    perm = np.zeros(max(len(k), 1), np.uint16)
    _check(lib().gfs_test_wave_std_sort(device, _p(k), len(k), _p(perm)), "gfs_test_wave_std_sort")
    return perm[:len(k)].astype(np.int64)


def octree_host(x, y, score, min_x, max_x, min_y, max_y, n_features):
    """The library's host DistributeOctTree (no GPU needed)."""
    x = np.ascontiguousarray(x, np.int32)
    y = np.ascontiguousarray(y, np.int32)
    score = np.ascontiguousarray(score, np.int32)
    out = np.zeros(max(len(x), 1), np.int32)
    n = lib().gfs_orb_octree_host(_p(x), _p(y), _p(score), len(x), min_x, max_x, min_y, max_y, n_features, _p(out),
                                  len(out))
    return out[:n]


def octree_device(x, y, score, min_x, max_x, min_y, max_y, n_features, device=0):
    """The library's device DistributeOctTree (k_octree) -> kept (x, y, score) arrays in list order."""
    x = np.ascontiguousarray(x, np.int32)
    y = np.ascontiguousarray(y, np.int32)
    score = np.ascontiguousarray(score, np.int32)
    cap = n_features + 64
    ox, oy, os_ = (np.zeros(cap, np.int32) for _ in range(3))
    n = _check(lib().gfs_orb_octree_device(device, _p(x), _p(y), _p(score), len(x), min_x, max_x, min_y, max_y, n_features,
                                           _p(ox), _p(oy), _p(os_), cap), "gfs_orb_octree_device")
    return ox[:n], oy[:n], os_[:n]


class ORBmatcher:
    """The brute-force Hamming part of ORB_SLAM3::ORBmatcher (reference src/ORBmatcher.cc:744-778, 2536-2550)."""

    def __init__(self, max_query=4096, max_train=4096, max_batch=1, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_matcher_create(device, max_query, max_train, max_batch, C.byref(self.h)), "gfs_matcher_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_matcher_destroy(self.h)
        self.h = None

    __del__ = close

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        return int(lib().gfs_hamming256(_p(a), _p(b)))

    def match(self, query, train):
        """cv::BFMatcher(NORM_HAMMING).match(query, train) -> (trainIdx[nq], distance[nq]); empty if no train rows."""
        q = np.ascontiguousarray(query, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(train, np.uint8).reshape(-1, 32)
        ti = np.zeros(len(q), np.int32)
        di = np.zeros(len(q), np.int32)
        n = _check(lib().gfs_bf_match_hamming(self.h, _p(q), len(q), _p(t), len(t), _p(ti), _p(di)),
                   "gfs_bf_match_hamming")
        return ti[:n], di[:n]

    def match_batch_device(self, d_query, d_nq, d_train, d_nt, B, stride_rows, d_idx, d_dist, stream=None):
        _check(lib().gfs_bf_match_hamming_batch_device(self.h, C.c_void_p(d_query), C.c_void_p(d_nq), C.c_void_p(d_train),
                                                       C.c_void_p(d_nt), B, stride_rows, C.c_void_p(d_idx),
                                                       C.c_void_p(d_dist), C.c_void_p(stream) if stream else None),
               "gfs_bf_match_hamming_batch_device")


def gicp_default_config():
    c = GicpConfig()
    lib().gfs_gicp_default_config(C.byref(c))
    return c


def _result_dict(res):
    return dict(
        T=np.array(res.T).reshape(4, 4).T.copy(), converged=bool(res.converged), iterations=int(res.iterations),
        num_inliers=int(res.num_inliers), H=np.array(res.H).reshape(6, 6).T.copy(), b=np.array(res.b),
        error=float(res.error), n_target_ds=res.n_target_ds, n_source_ds=res.n_source_ds,
        n_linearize=res.n_linearize, n_error_evals=res.n_error_evals)


class RegistrationGICP:
    """RegistrationGICP (reference include/RegistrationGICP.h:19-31, src/RegistrationGICP.cc:5-20)."""

    def __init__(self, max_points=40960, max_batch=1, device=0):
        self.h = C.c_void_p()
        self.max_points = max_points
        _check(lib().gfs_gicp_create(device, max_points, max_batch, C.byref(self.h)), "gfs_gicp_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_gicp_destroy(self.h)
        self.h = None

    __del__ = close

    def RegisterPointClouds(self, target_points, source_points, init_T_target_source=None, cfg=None):
        t = np.ascontiguousarray(target_points, np.float32).reshape(-1, 4)
        s = np.ascontiguousarray(source_points, np.float32).reshape(-1, 4)
        T0 = np.eye(4) if init_T_target_source is None else np.asarray(init_T_target_source, np.float64)
        T0c = np.ascontiguousarray(T0.T.reshape(-1))
        cfg = cfg or gicp_default_config()
        res = GicpResult()
        _check(lib().gfs_gicp_align(self.h, _p(t), len(t), _p(s), len(s), _p(T0c), C.byref(cfg), C.byref(res)),
               "gfs_gicp_align")
        return _result_dict(res)

    def voxel_sort_perm(self, keys):
        """Test hook: permutation of the preprocessing's voxel sort (small_gicp quick_sort_omp replica) for caller keys."""
        k = np.ascontiguousarray(keys, np.uint64)
        perm = np.zeros(max(len(k), 1), np.uint32)
        _check(lib().gfs_test_voxel_sort(self.h, _p(k), len(k), _p(perm)), "gfs_test_voxel_sort")
        return perm[:len(k)].astype(np.int64)

    def voxel_sort_paths(self):
        """Test hook: leaf ranges of the last voxel sort on this handle by path -> dict(tie_free, harmless, replica)."""
        out = np.zeros(3, np.int32)
        _check(lib().gfs_test_voxel_sort_paths(self.h, _p(out)), "gfs_test_voxel_sort_paths")
        return dict(tie_free=int(out[0]), harmless=int(out[1]), replica=int(out[2]))

    def RegisterNext(self, source_points, init_T_target_source=None, cfg=None):
        """Streaming form: the target is the source cloud of the previous call on this object (kept preprocessed in HBM), as in
        Tracking::PredictStateICP; bit-identical to RegisterPointClouds(previous source, source_points)."""
        s = np.ascontiguousarray(source_points, np.float32).reshape(-1, 4)
        T0 = np.eye(4) if init_T_target_source is None else np.asarray(init_T_target_source, np.float64)
        T0c = np.ascontiguousarray(T0.T.reshape(-1))
        cfg = cfg or gicp_default_config()
        res = GicpResult()
        _check(lib().gfs_gicp_align_next(self.h, _p(s), len(s), _p(T0c), C.byref(cfg), C.byref(res)), "gfs_gicp_align_next")
        return _result_dict(res)

    def align_next_batch_device(self, d_source, d_ns, B, stride_pts, init_T=None, cfg=None, stream=None, raw=False):
        cfg = cfg or gicp_default_config()
        out = (GicpResult * B)()
        T0 = None
        if init_T is not None:
            T0 = np.ascontiguousarray(np.asarray(init_T, np.float64).transpose(0, 2, 1).reshape(B, 16))
        _check(lib().gfs_gicp_align_next_batch_device(self.h, C.c_void_p(d_source), C.c_void_p(d_ns), B, stride_pts, _p(T0),
                                                      C.byref(cfg), out, C.c_void_p(stream) if stream else None),
               "gfs_gicp_align_next_batch_device")
        return out if raw else [_result_dict(r) for r in out]

    def align_batch_device(self, d_target, d_nt, d_source, d_ns, B, stride_pts, init_T=None, cfg=None, stream=None,
                           raw=False):
        """raw=True returns the ctypes array of gfs_gicp_result (no per-pair Python conversion on the hot path)."""
        cfg = cfg or gicp_default_config()
        out = (GicpResult * B)()
        T0 = None
        if init_T is not None:
            T0 = np.ascontiguousarray(np.asarray(init_T, np.float64).transpose(0, 2, 1).reshape(B, 16))
        _check(lib().gfs_gicp_align_batch_device(self.h, C.c_void_p(d_target), C.c_void_p(d_nt), C.c_void_p(d_source),
                                                 C.c_void_p(d_ns), B, stride_pts, _p(T0), C.byref(cfg), out,
                                                 C.c_void_p(stream) if stream else None), "gfs_gicp_align_batch_device")
        if raw:
            return out
        return [_result_dict(r) for r in out]

    def tile_stats(self, reset=True):
        """The handle's diagnostics counter block (eight words; written by the -DGFS_KNN_UTIL / -DGFS_LIN_UTIL variant builds only: lanes at
        work, steps, queries, waves of the neighbour searches, slot by slot in gfs_gicp_tile_stats' comment)."""
        out = np.zeros(8, np.uint64)
        _check(lib().gfs_gicp_tile_stats(self.h, _p(out), int(reset)), "gfs_gicp_tile_stats")
        return out

    def coop_stats(self):
        """dict(launches, last_workgroups, failed, budget) of the cooperative LM kernel on this handle: gfs_gicp_coop_stats."""
        out = np.zeros(4, np.int32)
        _check(lib().gfs_gicp_coop_stats(self.h, _p(out)), "gfs_gicp_coop_stats")
        return dict(launches=int(out[0]), last_workgroups=int(out[1]), failed=bool(out[2]), budget=int(out[3]))

    def coop_hold(self, n):
        """Test hook (gfs_test_gicp_coop_hold): take exactly n workgroups out of the device's cooperative budget, as another handle's
        launch in flight would; GfsError (GFS_ERR_CAPACITY) when n are not free.  Only coop_release(n) gives them back."""
        _check(lib().gfs_test_gicp_coop_hold(self.h, int(n)), "gfs_test_gicp_coop_hold")

    def coop_release(self, n):
        """Test hook (gfs_test_gicp_coop_release): give back n workgroups taken with coop_hold."""
        _check(lib().gfs_test_gicp_coop_release(self.h, int(n)), "gfs_test_gicp_coop_release")

    def knn_stats(self, b, which, cap=256):
        """(points, deferred to the r = 2 pass, deferred to the isolated-point pass), bounds of the latter: gfs_gicp_knn_stats."""
        out = np.zeros(3, np.int32)
        dk = np.zeros(cap)
        _check(lib().gfs_gicp_knn_stats(self.h, b, which, _p(out), _p(dk), cap), "gfs_gicp_knn_stats")
        return out, dk[:min(int(out[2]), cap)]

    def preprocessed(self, b, which, cap=None):
        cap = cap or self.max_points
        pts = np.zeros((cap, 4))
        covs = np.zeros((cap, 9))
        m = C.c_int()
        _check(lib().gfs_gicp_fetch_preprocessed(self.h, b, which, _p(pts), _p(covs), cap, C.byref(m)),
               "gfs_gicp_fetch_preprocessed")
        return pts[:m.value], covs[:m.value].reshape(-1, 3, 3).transpose(0, 2, 1).copy()


def gicp_coop_in_use(device=0):
    """Test hook (gfs_test_gicp_coop_in_use): workgroups of the device's cooperative budget that are taken right now."""
    return int(lib().gfs_test_gicp_coop_in_use(device))


class Timer:
    def __init__(self, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_timer_create(device, C.byref(self.h)), "gfs_timer_create")

    def start(self, stream=None):
        _check(lib().gfs_timer_start(self.h, C.c_void_p(stream) if stream else None), "gfs_timer_start")

    def stop(self, stream=None):
        _check(lib().gfs_timer_stop(self.h, C.c_void_p(stream) if stream else None), "gfs_timer_stop")

    def elapsed_ms(self):
        ms = C.c_float()
        _check(lib().gfs_timer_elapsed_ms(self.h, C.byref(ms)), "gfs_timer_elapsed_ms")
        return ms.value

    def __del__(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_timer_destroy(self.h)
        self.h = None


def profile_enable(on=True):
    lib().gfs_profile_enable(int(on))


def profile_reset():
    lib().gfs_profile_reset()


def profile_report():
    cap = 64
    names = (C.c_char * 64 * cap)()
    tot = np.zeros(cap)
    cnt = np.zeros(cap, np.int64)
    n = lib().gfs_profile_report(names, _p(tot), _p(cnt), cap)
    return {names[i].value.decode(): (float(tot[i]), int(cnt[i])) for i in range(min(n, cap))}


def _lba_problem(prob):
    P = LbaProblem()
    keep = {}
    for name, dt in (("pose_q", np.float64), ("pose_t", np.float64), ("pose_fixed", np.uint8), ("points", np.float64),
                     ("edge_pose", np.int32), ("edge_point", np.int32), ("edge_obs", np.float64),
                     ("edge_inv_sigma2", np.float64), ("edge_stereo", np.uint8)):
        keep[name] = np.ascontiguousarray(prob[name], dt)
        setattr(P, name, keep[name].ctypes.data)
    for name in ("n_poses", "n_points", "n_edges", "iterations"):
        setattr(P, name, int(prob[name]))
    for name in ("fx", "fy", "cx", "cy", "bf", "huber_mono", "huber_stereo"):
        setattr(P, name, float(prob[name]))
    return P, keep


def lba_stop_at_look(look):
    """Test hook (include/gfs_abi_test.h): script the stop flag of THIS thread's next LocalBundleAdjustment / LocalVisualLidarBA /
    batch call -- from its look-th evaluation on the flag reads as raised (look 0 = the entry check); negative disarms.  The call
    needs a stop_flag array."""
    _check(lib().gfs_test_lba_stop_at_look(int(look)), "gfs_test_lba_stop_at_look")


def lba_last_looks():
    """-> dict(looks, discarded, forced_decides, ahead_at_stop) of this thread's last LBA solve (gfs_test_lba_last_looks)."""
    v = [C.c_int32() for _ in range(4)]
    _check(lib().gfs_test_lba_last_looks(*[C.byref(x) for x in v]), "gfs_test_lba_last_looks")
    return dict(looks=v[0].value, discarded=v[1].value, forced_decides=v[2].value, ahead_at_stop=v[3].value)


def lba_first_trial(opt, prob, fill=np.nan, _entry="gfs_test_lba_first_trial"):
    """Test hook (include/gfs_abi_test.h: gfs_test_lba_first_trial): the linear step of the first LM trial of `prob` on the Optimizer
    `opt`, through the product's dispatch -> dict(lam, Dinv [n_points, 6], Hs (packed lower triangle), bs, xp [6F], xl [n_points, 3],
    solve_ok, scale).  The arrays are pre-written with `fill`: an entry the library did not deliver still holds it."""
    P, keep = _lba_problem(prob)
    nf = int((np.asarray(prob["pose_fixed"]) == 0).sum())
    n, NP = 6 * nf, P.n_points
    # (one spare element each: a window without free poses or landmarks still hands in non-NULL arrays)
    buf = dict(Dinv=np.full(6 * NP + 1, fill), Hs=np.full(n * (n + 1) // 2 + 1, fill), bs=np.full(n + 1, fill),
               xp=np.full(n + 1, fill), xl=np.full(3 * NP + 1, fill))
    T = LbaTrial()
    for k, v in buf.items():
        setattr(T, k, v.ctypes.data)
    _check(getattr(lib(), _entry)(opt.h, C.byref(P), C.byref(T)), _entry)
    return dict(lam=T.lambda_, scale=T.scale, solve_ok=int(T.solve_ok), Dinv=buf["Dinv"][:-1].reshape(NP, 6).copy(),
                Hs=buf["Hs"][:-1].copy(), bs=buf["bs"][:-1].copy(), xp=buf["xp"][:-1].copy(), xl=buf["xl"][:-1].reshape(NP, 3).copy())


def gba_first_trial(opt, prob, fill=np.nan):
    """Test hook (gfs_test_gba_first_trial): lba_first_trial's dict for the GlobalOptimizer `opt`, through gfs_gba_solve's sequence."""
    return lba_first_trial(opt, prob, fill, _entry="gfs_test_gba_first_trial")


def gba_panel_rows():
    """Rows of a tile of GlobalBundleAdjustment's tiled reduced system (gfs_test_gba_panel_rows)."""
    return int(lib().gfs_test_gba_panel_rows())


def gba_lists(prob):
    """Host test hook (gfs_test_gba_lists, no GPU): the structure lists of the Schur assembly for `prob` -> dict(n_free, order [E],
    blk_ij [B, 2], blk_begin [B + 1], contrib [C, 2], pose_begin [F + 1], pose_edges); edge ids are landmark-major positions."""
    fixed = np.ascontiguousarray(prob["pose_fixed"], np.uint8)
    ep, el = np.ascontiguousarray(prob["edge_pose"], np.int32), np.ascontiguousarray(prob["edge_point"], np.int32)
    NQ, NP, E = int(prob["n_poses"]), int(prob["n_points"]), int(prob["n_edges"])
    counts = np.zeros(3, np.int64)
    rc = lib().gfs_test_gba_lists(NQ, NP, E, _p(fixed), _p(ep), _p(el), _p(counts), None, None, None, 0, None, 0, None, None)
    if rc not in (0, -4):
        _check(rc, "gfs_test_gba_lists")
    F, B, Cn = (int(v) for v in counts)
    order, blk, beg = np.zeros(E + 1, np.int32), np.zeros((B + 1, 2), np.int32), np.zeros(B + 2, np.int64)
    con, pb, pe = np.zeros((Cn + 1, 2), np.int32), np.zeros(F + 2, np.int64), np.zeros(E + 1, np.int32)
    _check(lib().gfs_test_gba_lists(NQ, NP, E, _p(fixed), _p(ep), _p(el), _p(counts), _p(order), _p(blk), _p(beg), B, _p(con), Cn, _p(pb),
                                    _p(pe)), "gfs_test_gba_lists")
    return dict(n_free=F, order=order[:E], blk_ij=blk[:B], blk_begin=beg[:B + 1], contrib=con[:Cn], pose_begin=pb[:F + 1],
                pose_edges=pe[:int(pb[F])])


def gba_tile_layout(n, r, c):
    """Host test hook (gfs_test_gba_tile_layout, no GPU) -> dict(panels, storage_bytes, tile_index, byte_offset) as Python ints."""
    out = np.zeros(4, np.uint64)
    _check(lib().gfs_test_gba_tile_layout(int(n), int(r), int(c), _p(out)), "gfs_test_gba_tile_layout")
    return dict(zip(("panels", "storage_bytes", "tile_index", "byte_offset"), (int(v) for v in out)))


class GlobalOptimizer:
    """The numeric core of ORB_SLAM3::Optimizer::GlobalBundleAdjustemnt / BundleAdjustment (reference src/Optimizer.cc:47-363) on a
    flattened problem (gfs_lba_problem): the full map, the reduced pose system tiled over the whole device (gfs_gba_solve)."""

    def __init__(self, max_poses=512, max_points=32768, max_edges=524288, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_gba_create(device, max_poses, max_points, max_edges, C.byref(self.h)), "gfs_gba_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_gba_destroy(self.h)
        self.h = None

    __del__ = close

    def BundleAdjustment(self, prob, stop_flag=None, robust=True):
        """optimizer.optimize(prob["iterations"]).  robust=False (bRobust = false: LoopClosing::RunGlobalBundleAdjustment) puts +inf
        in the place of the two Huber thresholds.  stop_flag: an int32 array read live (pbStopFlag); a flag that is already up gives
        iterations_run = 0 and the input estimate, never None."""
        if not robust:
            prob = dict(prob, huber_mono=np.inf, huber_stereo=np.inf)
        P, keep = _lba_problem(prob)
        out = dict(pose_q=np.zeros((P.n_poses, 4)), pose_t=np.zeros((P.n_poses, 3)), points=np.zeros((P.n_points, 3)),
                   edge_chi2=np.zeros(P.n_edges), edge_depth_positive=np.zeros(P.n_edges, np.uint8))
        S = LbaSolution()
        for k, v in out.items():
            setattr(S, k, v.ctypes.data)
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        _check(lib().gfs_gba_solve(self.h, C.byref(P), C.byref(S), stop), "gfs_gba_solve")
        out.update(iterations_run=S.iterations_run, final_chi2=S.final_chi2, final_lambda=S.final_lambda)
        return out

    def last_info(self):
        I = GbaInfo()
        _check(lib().gfs_gba_last_info(self.h, C.byref(I)), "gfs_gba_last_info")
        return {k: int(getattr(I, k)) for k, _ in GbaInfo._fields_}


# optimize(20), setUserLambdaInit(1e-16), covisibility weight minFeat = 100, the ICP edges' 3 x information (reference
# src/Optimizer.cc:2362, :2059, :2145, :2306)
ESSENTIAL_GRAPH_ITERATIONS = 20
ESSENTIAL_GRAPH_LAMBDA_INIT = 1e-16
ESSENTIAL_GRAPH_MIN_FEAT = 100
ESSENTIAL_GRAPH_ICP_WEIGHT = 3.0


def _essential_graph_problem(prob):
    P = EssentialGraphProblem()
    keep = {}
    for name, dt in (("vertex_q", np.float64), ("vertex_t", np.float64), ("vertex_s", np.float64), ("vertex_fixed", np.uint8),
                     ("edge_i", np.int32), ("edge_j", np.int32), ("edge_q", np.float64), ("edge_t", np.float64), ("edge_s", np.float64),
                     ("edge_w", np.float64), ("points", np.float32), ("point_ref", np.int32)):
        default = np.zeros((0, 3), np.float32) if name == "points" else np.zeros(0, np.int32)
        keep[name] = np.ascontiguousarray(prob.get(name, default), dt)
        setattr(P, name, keep[name].ctypes.data)
    P.n_vertices, P.n_edges, P.n_points = len(keep["vertex_s"]), len(keep["edge_i"]), len(keep["point_ref"])
    P.fix_scale = int(bool(prob.get("fix_scale", True)))
    P.iterations = int(prob.get("iterations", ESSENTIAL_GRAPH_ITERATIONS))
    P.lambda_init = float(prob.get("lambda_init", ESSENTIAL_GRAPH_LAMBDA_INIT))
    return P, keep


def essential_graph_lists(vertex_fixed, edge_i, edge_j):
    """Host test hook (gfs_test_essential_graph_lists, no GPU): the structure lists of the essential graph's pose system ->
    dict(n_free, free_index [V], blk_ij [B, 2], blk_begin [B + 1], contrib [C] = 4 edge + kind)."""
    fixed = np.ascontiguousarray(vertex_fixed, np.uint8)
    ei, ej = np.ascontiguousarray(edge_i, np.int32), np.ascontiguousarray(edge_j, np.int32)
    V, E = len(fixed), len(ei)
    counts = np.zeros(3, np.int64)
    rc = lib().gfs_test_essential_graph_lists(V, E, _p(fixed), _p(ei), _p(ej), _p(counts), None, None, None, 0, None, 0)
    if rc not in (0, -4):
        _check(rc, "gfs_test_essential_graph_lists")
    F, B, Cn = (int(v) for v in counts)
    fi, blk, beg, con = np.zeros(V + 1, np.int32), np.zeros((B + 1, 2), np.int32), np.zeros(B + 2, np.int64), np.zeros(Cn + 1, np.int32)
    _check(lib().gfs_test_essential_graph_lists(V, E, _p(fixed), _p(ei), _p(ej), _p(counts), _p(fi), _p(blk), _p(beg), B, _p(con), Cn),
           "gfs_test_essential_graph_lists")
    return dict(n_free=F, free_index=fi[:V], blk_ij=blk[:B], blk_begin=beg[:B + 1], contrib=con[:Cn])


def essential_graph_first_trial(opt, prob, fill=np.nan):
    """Test hook (gfs_test_essential_graph_first_trial): the first Levenberg trial of `prob` on the EssentialGraphOptimizer `opt`,
    through the product's launch sequence -> dict(H (packed lower triangle, lambda on the diagonal), b, x, chi2, trial_chi2, scale,
    n_free, dimension, solve_ok).  The arrays are pre-written with `fill`."""
    P, keep = _essential_graph_problem(prob)
    n = (6 if P.fix_scale else 7) * int((keep["vertex_fixed"] == 0).sum())
    buf = dict(H=np.full(n * (n + 1) // 2 + 1, fill), b=np.full(n + 1, fill), x=np.full(n + 1, fill))
    T = EssentialGraphTrial()
    for k, v in buf.items():
        setattr(T, k, v.ctypes.data)
    _check(lib().gfs_test_essential_graph_first_trial(opt.h, C.byref(P), C.byref(T)), "gfs_test_essential_graph_first_trial")
    return dict(H=buf["H"][:-1].copy(), b=buf["b"][:-1].copy(), x=buf["x"][:-1].copy(), chi2=T.chi2, trial_chi2=T.trial_chi2,
                scale=T.scale, n_free=int(T.n_free), dimension=int(T.dimension), solve_ok=int(T.solve_ok))


class EssentialGraphOptimizer:
    """The numeric core of ORB_SLAM3::Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:2042-2413) on a flattened Sim3
    pose graph (gfs_essential_graph_problem): Levenberg on VertexSim3Expmap / EdgeSim3 with g2o's numeric Jacobians, the pose system
    tiled over the whole device, then the map points moved with their reference key-frames."""

    def __init__(self, max_vertices=512, max_edges=8192, max_points=65536, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_essential_graph_create(device, max_vertices, max_edges, max_points, C.byref(self.h)), "gfs_essential_graph_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_essential_graph_destroy(self.h)
        self.h = None

    __del__ = close

    def OptimizeEssentialGraph(self, prob):
        """prob: vertex_q [V, 4] (x, y, z, w), vertex_t, vertex_s, vertex_fixed; edge_i, edge_j, edge_q, edge_t, edge_s, edge_w in the
        reference's creation order; fix_scale, iterations (20), lambda_init (1e-16); points [M, 3] float32 and point_ref [M] (optional)
        -> dict(vertex_q, vertex_t, vertex_s, points, edge_chi2, iterations_run, final_chi2, final_lambda)."""
        P, keep = _essential_graph_problem(prob)
        out = dict(vertex_q=np.zeros((P.n_vertices, 4)), vertex_t=np.zeros((P.n_vertices, 3)), vertex_s=np.zeros(P.n_vertices),
                   points=np.zeros((P.n_points, 3), np.float32), edge_chi2=np.zeros(P.n_edges))
        S = EssentialGraphSolution()
        for k, v in out.items():
            setattr(S, k, v.ctypes.data)
        _check(lib().gfs_essential_graph_optimize(self.h, C.byref(P), C.byref(S)), "gfs_essential_graph_optimize")
        out.update(iterations_run=S.iterations_run, final_chi2=S.final_chi2, final_lambda=S.final_lambda)
        return out

    def correct_points(self, before, after, points, point_ref):
        """correctedSwr.map(Srw.map(P)) alone: before / after [V, 8] = (q, t, s) of every vertex before and after a correction,
        points [M, 3] float32, point_ref [M] (-1: as is) -> [M, 3] float32."""
        b, a = np.ascontiguousarray(before, np.float64), np.ascontiguousarray(after, np.float64)
        pts, ref = np.ascontiguousarray(points, np.float32), np.ascontiguousarray(point_ref, np.int32)
        out = np.zeros((len(ref), 3), np.float32)
        _check(lib().gfs_essential_graph_correct_points(self.h, len(b), _p(b), _p(a), len(ref), _p(pts), _p(ref), _p(out)),
               "gfs_essential_graph_correct_points")
        return out

    def last_info(self):
        I = EssentialGraphInfo()
        _check(lib().gfs_essential_graph_last_info(self.h, C.byref(I)), "gfs_essential_graph_last_info")
        return {k: int(getattr(I, k)) for k, _ in EssentialGraphInfo._fields_}


class Optimizer:
    """The numeric core of ORB_SLAM3::Optimizer::LocalBundleAdjustment (reference include/Optimizer.h:62-65,
    src/Optimizer.cc:1588-2040) on a flattened problem (see gfs_lba_problem in include/gfs_abi.h)."""

    def __init__(self, max_poses=64, max_points=8192, max_edges=131072, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_lba_create(device, max_poses, max_points, max_edges, C.byref(self.h)), "gfs_lba_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_lba_destroy(self.h)
        self.h = None

    __del__ = close

    def LocalBundleAdjustment(self, prob, stop_flag=None):
        P, keep = _lba_problem(prob)
        out = dict(pose_q=np.zeros((P.n_poses, 4)), pose_t=np.zeros((P.n_poses, 3)), points=np.zeros((P.n_points, 3)),
                   edge_chi2=np.zeros(P.n_edges), edge_depth_positive=np.zeros(P.n_edges, np.uint8))
        S = LbaSolution()
        for k, v in out.items():
            setattr(S, k, v.ctypes.data)
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        rc = lib().gfs_lba_solve(self.h, C.byref(P), C.byref(S), stop)
        if rc == -6:  # GFS_ERR_STOPPED: the reference returns without touching the map (src/Optimizer.cc:1955-1956)
            return None
        _check(rc, "gfs_lba_solve")
        out.update(iterations_run=S.iterations_run, final_chi2=S.final_chi2, final_lambda=S.final_lambda)
        return out

    def _lidar(self, prob, lidar_map):
        L, keep = lba_lidar_struct(prob, lidar_map.h)
        cb = keep["cloud_begin"]
        need = int(cb[-1] - cb[0]) if len(cb) else 0
        if need > getattr(self, "lidar_cap", 0):  # (the library refuses a window beyond the reserve: it never truncates)
            _check(lib().gfs_lba_lidar_reserve(self.h, need), "gfs_lba_lidar_reserve")
            self.lidar_cap = need
        return L, keep

    def LocalVisualLidarBA(self, prob, lidar_map, stop_flag=None):
        """ORB_SLAM3::Optimizer::LocalVisualLidarBA (reference src/Optimizer.cc:1101-1587): LocalBundleAdjustment's window plus the
        point-to-plane edges of the local key-frames against lidar_map (a LidarMap).  prob: the LocalBundleAdjustment dict plus
        pose_local [n_poses], matches_inliers [n_poses], cloud_begin [n_poses + 1], cloud [n][3].  -> LocalBundleAdjustment's dict
        plus pose_lidar_edges [n_poses], or None when the stop flag was raised before the call."""
        P, keep = _lba_problem(prob)
        L, lkeep = self._lidar(prob, lidar_map)
        out = dict(pose_q=np.zeros((P.n_poses, 4)), pose_t=np.zeros((P.n_poses, 3)), points=np.zeros((P.n_points, 3)),
                   edge_chi2=np.zeros(P.n_edges), edge_depth_positive=np.zeros(P.n_edges, np.uint8))
        S = LbaSolution()
        for k, v in out.items():
            setattr(S, k, v.ctypes.data)
        ple = np.zeros(max(P.n_poses, 1), np.int32)
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        rc = lib().gfs_lba_solve_lidar(self.h, C.byref(P), C.byref(L), C.byref(S), _p(ple), stop)
        if rc == -6:  # GFS_ERR_STOPPED (src/Optimizer.cc:1502-1503)
            return None
        _check(rc, "gfs_lba_solve_lidar")
        out.update(iterations_run=S.iterations_run, final_chi2=S.final_chi2, final_lambda=S.final_lambda,
                   pose_lidar_edges=ple[:P.n_poses].copy())
        return out

    def linearize_lidar(self, prob, lidar_map):
        """linearize() with the lidar edges of LocalVisualLidarBA: their terms in Hpp / bp / chi2, plus lidar_edge_chi2 (every lidar
        edge in g2o's order: key-frames in pose order, then cloud order) and pose_lidar_edges."""
        P, keep = _lba_problem(prob)
        L, lkeep = self._lidar(prob, lidar_map)
        nf = int((np.asarray(prob["pose_fixed"]) == 0).sum())
        Hpp = np.zeros((nf, 36)); Hll = np.zeros((P.n_points, 9)); Hpl = np.zeros((P.n_edges, 18))
        bp = np.zeros((nf, 6)); bl = np.zeros((P.n_points, 3)); chi = np.zeros(P.n_edges)
        cap = max(int(lkeep["cloud_begin"][-1]) if len(lkeep["cloud_begin"]) else 0, 1)
        lchi, ple = np.zeros(cap), np.zeros(max(P.n_poses, 1), np.int32)
        tot = C.c_double()
        _check(lib().gfs_lba_linearize_lidar(self.h, C.byref(P), C.byref(L), _p(Hpp), _p(Hll), _p(Hpl), _p(bp), _p(bl), _p(chi),
                                             C.byref(tot), _p(lchi), cap, _p(ple)), "gfs_lba_linearize_lidar")
        ple = ple[:P.n_poses].copy()
        return dict(Hpp=Hpp.reshape(nf, 6, 6).transpose(0, 2, 1).copy(), Hll=Hll.reshape(-1, 3, 3).transpose(0, 2, 1).copy(),
                    Hpl=Hpl.reshape(-1, 3, 6).transpose(0, 2, 1).copy(), bp=bp, bl=bl, edge_chi2=chi, chi2=tot.value,
                    lidar_edge_chi2=lchi[:int(ple.sum())].copy(), pose_lidar_edges=ple)

    def fetch_lidar_edges(self, pose):
        """The lidar edges of `pose` in the last lidar call: (index [n] in the pose's cloud, plane [n][4], s [n]), all of them."""
        n = C.c_int32()
        _check(lib().gfs_lba_fetch_lidar_edges(self.h, pose, None, None, None, 0, C.byref(n)), "gfs_lba_fetch_lidar_edges")
        m = n.value
        idx, pl, s = np.zeros(max(m, 1), np.int32), np.zeros((max(m, 1), 4), np.float32), np.zeros(max(m, 1), np.float32)
        _check(lib().gfs_lba_fetch_lidar_edges(self.h, pose, _p(idx), _p(pl), _p(s), m, C.byref(n)), "gfs_lba_fetch_lidar_edges")
        if n.value != m:
            raise GfsError(f"gfs_lba_fetch_lidar_edges: {n.value} edges, expected {m}")
        return idx[:m].copy(), pl[:m].copy(), s[:m].copy()

    def linearize(self, prob):
        P, keep = _lba_problem(prob)
        nf = int((np.asarray(prob["pose_fixed"]) == 0).sum())
        Hpp = np.zeros((nf, 36)); Hll = np.zeros((P.n_points, 9)); Hpl = np.zeros((P.n_edges, 18))
        bp = np.zeros((nf, 6)); bl = np.zeros((P.n_points, 3)); chi = np.zeros(P.n_edges)
        tot = C.c_double()
        _check(lib().gfs_lba_linearize(self.h, C.byref(P), _p(Hpp), _p(Hll), _p(Hpl), _p(bp), _p(bl), _p(chi),
                                       C.byref(tot)), "gfs_lba_linearize")
        return dict(Hpp=Hpp.reshape(nf, 6, 6).transpose(0, 2, 1).copy(), Hll=Hll.reshape(-1, 3, 3).transpose(0, 2, 1).copy(),
                    Hpl=Hpl.reshape(-1, 3, 6).transpose(0, 2, 1).copy(), bp=bp, bl=bl, edge_chi2=chi, chi2=tot.value)


class BatchOptimizer:
    """n independent LocalBundleAdjustment windows solved together (gfs_lba_solve_batch)."""

    def __init__(self, max_windows=64, max_poses=32, max_points=4096, max_edges=65536, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_lba_batch_create(device, max_windows, max_poses, max_points, max_edges, C.byref(self.h)), "gfs_lba_batch_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_lba_batch_destroy(self.h)
        self.h = None

    __del__ = close

    def prepare(self, probs):
        """ctypes views (kept alive by the returned object) so that repeated solves pay no Python conversion"""
        n = len(probs)
        P = (LbaProblem * n)()
        S = (LbaSolution * n)()
        keep, outs = [], []
        for k, prob in enumerate(probs):
            pk, kp = _lba_problem(prob)
            P[k] = pk
            keep.append(kp)
            out = dict(pose_q=np.zeros((pk.n_poses, 4)), pose_t=np.zeros((pk.n_poses, 3)), points=np.zeros((pk.n_points, 3)),
                       edge_chi2=np.zeros(pk.n_edges), edge_depth_positive=np.zeros(pk.n_edges, np.uint8))
            for name, v in out.items():
                setattr(S[k], name, v.ctypes.data)
            outs.append(out)
        keep.append(outs)  # S points into these arrays: whoever holds `keep` keeps them alive
        return P, S, outs, keep

    def solve_prepared(self, P, S, n, stop_flag=None):
        stop = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        _check(lib().gfs_lba_solve_batch(self.h, P, S, n, stop), "gfs_lba_solve_batch")

    def LocalBundleAdjustment(self, probs, stop_flag=None):
        P, S, outs, keep = self.prepare(probs)
        self.solve_prepared(P, S, len(probs), stop_flag)
        for k, out in enumerate(outs):
            out.update(iterations_run=S[k].iterations_run, final_chi2=S[k].final_chi2, final_lambda=S[k].final_lambda)
        return outs


class GmsMatcher:
    """gms_matcher(kp1, size1, kp2, size2, matches).GetInlierMask(mask, false, false) (reference
    Thirdparty/GMS/include/gms_matcher.h; call sites src/ORBmatcher.cc:761-762, 812-813, 893-894)."""

    def __init__(self, max_keypoints=4096, max_batch=64, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_gms_create(device, max_keypoints, max_batch, C.byref(self.h)), "gfs_gms_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_gms_destroy(self.h)
        self.h = None

    __del__ = close

    def GetInlierMask(self, kp1, size1, kp2, size2, query_idx, train_idx):
        """size = (width, height) like cv::Size -> (mask bool [n_matches], n_inliers)"""
        kp1 = np.ascontiguousarray(kp1, KP_DTYPE)
        kp2 = np.ascontiguousarray(kp2, KP_DTYPE)
        q = np.ascontiguousarray(query_idx, np.int32)
        t = np.ascontiguousarray(train_idx, np.int32)
        P = GmsProblem(len(kp1), len(kp2), kp1.ctypes.data, kp2.ctypes.data, int(size1[0]), int(size1[1]), int(size2[0]),
                       int(size2[1]), len(q), q.ctypes.data, t.ctypes.data)
        mask = np.zeros(max(len(q), 1), np.uint8)
        ptrs = (C.c_void_p * 1)(mask.ctypes.data)
        n = np.zeros(1, np.int32)
        _check(lib().gfs_gms_inlier_mask(self.h, C.byref(P), 1, ptrs, _p(n)), "gfs_gms_inlier_mask")
        return mask[:len(q)].astype(bool), int(n[0])

    def GetInlierMaskBatch(self, problems):
        """problems: a list of (kp1, size1, kp2, size2, query_idx, train_idx), filtered in ONE gfs_gms_inlier_mask call
        -> a list of (mask bool [n_matches], n_inliers)"""
        B = len(problems)
        P = (GmsProblem * B)()
        ptrs = (C.c_void_p * B)()
        keep, masks = [], []
        for f, (kp1, size1, kp2, size2, query_idx, train_idx) in enumerate(problems):
            kp1 = np.ascontiguousarray(kp1, KP_DTYPE)
            kp2 = np.ascontiguousarray(kp2, KP_DTYPE)
            q = np.ascontiguousarray(query_idx, np.int32)
            t = np.ascontiguousarray(train_idx, np.int32)
            P[f] = GmsProblem(len(kp1), len(kp2), kp1.ctypes.data, kp2.ctypes.data, int(size1[0]), int(size1[1]), int(size2[0]),
                              int(size2[1]), len(q), q.ctypes.data, t.ctypes.data)
            masks.append(np.zeros(max(len(q), 1), np.uint8))
            ptrs[f] = masks[f].ctypes.data
            keep.append((kp1, kp2, q, t))
        n = np.zeros(max(B, 1), np.int32)
        _check(lib().gfs_gms_inlier_mask(self.h, P, B, ptrs, _p(n)), "gfs_gms_inlier_mask")
        return [(masks[f][:P[f].n_matches].astype(bool), int(n[f])) for f in range(B)]

    def inlier_mask_batch_device(self, d_kps1, d_n1, d_kps2, d_n2, B, kp_stride, d_train_idx, width, height, d_mask, d_counts,
                                 stream=None):
        _check(lib().gfs_gms_inlier_mask_batch_device(self.h, C.c_void_p(d_kps1), C.c_void_p(d_n1), C.c_void_p(d_kps2),
                                                      C.c_void_p(d_n2), B, kp_stride, C.c_void_p(d_train_idx), width, height,
                                                      C.c_void_p(d_mask), C.c_void_p(d_counts),
                                                      C.c_void_p(stream) if stream else None), "gfs_gms_inlier_mask_batch_device")


KLT_USE_INITIAL_FLOW, KLT_GET_MIN_EIGENVALS = 4, 8


class Clahe:
    """cv::CLAHE on 8-bit single-channel images (cv::createCLAHE(3.0, cv::Size(8, 8)) of src/Frame.cc:367), DESIGN.md section 16.
    residual_variant: CLAHE_RESIDUAL_STEPPED (OpenCV >= 3.4) or CLAHE_RESIDUAL_CONTIGUOUS (OpenCV <= 3.3)."""

    def __init__(self, max_width=640, max_height=480, max_batch=1, clip_limit=3.0, tiles=(8, 8),
                 residual_variant=CLAHE_RESIDUAL_STEPPED, device=0):
        cfg = ClaheConfig()
        lib().gfs_clahe_default_config(C.byref(cfg))
        cfg.clip_limit, cfg.tiles_x, cfg.tiles_y, cfg.residual_variant = float(clip_limit), tiles[0], tiles[1], residual_variant
        self.tiles = (int(tiles[0]), int(tiles[1]))
        self.h = C.c_void_p()
        _check(lib().gfs_clahe_create(device, max_width, max_height, max_batch, C.byref(cfg), C.byref(self.h)), "gfs_clahe_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_clahe_destroy(self.h)
        self.h = None

    __del__ = close

    def apply(self, images, out=None):
        """images: one [H, W] u8 array or a list of equally sized ones; rows may be padded (a view with a row stride), all images
        with the same stride.  -> the equalised image(s), written into `out` (same form as `images`, may be `images`) when given."""
        single = isinstance(images, np.ndarray) and images.ndim == 2
        imgs = [images] if single else list(images)
        outs = [np.empty(im.shape, np.uint8) for im in imgs] if out is None else ([out] if single else list(out))
        H, W = imgs[0].shape
        for a in imgs + outs:
            if a.dtype != np.uint8 or a.shape != (H, W) or a.strides[1] != 1 or a.strides[0] < W:
                raise GfsError("Clahe.apply: images must be equally sized u8 arrays with contiguous rows")
        if len({im.strides[0] for im in imgs}) != 1 or len({o.strides[0] for o in outs}) != 1 or len(outs) != len(imgs):
            raise GfsError("Clahe.apply: one stride for all images, one for all outputs")
        ip = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        op = (C.c_void_p * len(outs))(*[o.ctypes.data for o in outs])
        _check(lib().gfs_clahe_apply(self.h, ip, W, H, imgs[0].strides[0], len(imgs), op, outs[0].strides[0]), "gfs_clahe_apply")
        return outs[0] if single else outs

    def apply_device(self, d_in, width, height, in_stride, B, d_out, out_stride, stream=None):
        """Device pointers ([B][height][stride] bytes); d_out may be d_in when the strides are equal."""
        _check(lib().gfs_clahe_apply_device(self.h, C.c_void_p(d_in), width, height, in_stride, B, C.c_void_p(d_out), out_stride,
                                            C.c_void_p(stream) if stream else None), "gfs_clahe_apply_device")

    def luts(self, f=0):
        """The look-up tables of frame f of the last call -> [tiles_y, tiles_x, 256] u8."""
        lut = np.zeros((self.tiles[1], self.tiles[0], 256), np.uint8)
        _check(lib().gfs_clahe_download_luts(self.h, f, _p(lut)), "gfs_clahe_download_luts")
        return lut


class KltPyramid:
    """The optical-flow pyramids (cv::buildOpticalFlowPyramid output, images + derivatives) of a batch of frames, resident in HBM."""

    def __init__(self, tracker):
        self.tracker = tracker
        self.h = C.c_void_p()
        _check(lib().gfs_klt_pyramid_create(tracker.h, C.byref(self.h)), "gfs_klt_pyramid_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None and getattr(self.tracker, "h", None):
            _lib.gfs_klt_pyramid_destroy(self.h)
        self.h = None

    __del__ = close

    def download(self, f=0):
        """-> (img u8 [total], deriv i16 [total, 2]) of frame f in the layout of KltTracker.layout()."""
        total = int(self.tracker.layout()[2][-1])
        img = np.zeros(total, np.uint8)
        der = np.zeros((total, 2), np.int16)
        _check(lib().gfs_klt_pyramid_download(self.tracker.h, self.h, f, _p(img), _p(der)), "gfs_klt_pyramid_download")
        return img, der


class KltTracker:
    """The optical-flow front end of the reference: cv::buildOpticalFlowPyramid (src/Frame.cc:373), cv::calcOpticalFlowPyrLK and
    ORBmatcher::fbKltTracking (src/ORBmatcher.cc:2186-2297).  win = LKWindowSize, max_level = 3 as in Frame.cc:371."""

    def __init__(self, width, height, win, max_level=3, max_batch=1, max_points=4096, device=0):
        self.width, self.height, self.win = width, height, win
        self.h = C.c_void_p()
        _check(lib().gfs_klt_create(device, width, height, win, max_level, max_batch, max_points, C.byref(self.h)), "gfs_klt_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_klt_destroy(self.h)
        self.h = None

    __del__ = close

    def layout(self):
        lw, lh, off = np.zeros(8, np.int32), np.zeros(8, np.int32), np.zeros(9, np.int64)
        n = lib().gfs_klt_layout(self.h, _p(lw), _p(lh), _p(off))
        if n <= 0:
            raise GfsError("gfs_klt_layout failed")
        return lw[:n].copy(), lh[:n].copy(), off[:n + 1].copy()

    def buildOpticalFlowPyramid(self, images, pyramid=None, clahe=None, return_equalized=False):
        """images: one [H, W] u8 array or a list of them -> KltPyramid (reused when given).  clahe: a Clahe whose equalisation runs
        on the device between the upload and the pyramid (src/Frame.cc:366-373); return_equalized: -> (KltPyramid, Frame::image as
        one array or a list, like `images`)."""
        single = isinstance(images, np.ndarray) and images.ndim == 2
        if single:
            images = [images]
        imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
        for im in imgs:
            if im.shape != (self.height, self.width):
                raise GfsError(f"image shape {im.shape} != {(self.height, self.width)}")
        if return_equalized and clahe is None:
            raise GfsError("buildOpticalFlowPyramid: return_equalized needs a Clahe")
        pyr = pyramid if pyramid is not None else KltPyramid(self)
        ptrs = (C.c_void_p * len(imgs))(*[im.ctypes.data for im in imgs])
        if clahe is None:
            _check(lib().gfs_klt_build_pyramid(self.h, pyr.h, ptrs, self.width, len(imgs)), "gfs_klt_build_pyramid")
            return pyr
        eq = [np.empty_like(im) for im in imgs] if return_equalized else None
        eptrs = (C.c_void_p * len(imgs))(*[e.ctypes.data for e in eq]) if eq else None
        _check(lib().gfs_klt_build_pyramid_clahe(self.h, clahe.h, pyr.h, ptrs, self.width, len(imgs), eptrs, self.width),
               "gfs_klt_build_pyramid_clahe")
        return (pyr, eq[0] if single else eq) if return_equalized else pyr

    def build_pyramid_device(self, d_images, stride, B, pyramid, stream=None):
        _check(lib().gfs_klt_build_pyramid_device(self.h, pyramid.h, C.c_void_p(d_images), stride, B,
                                                  C.c_void_p(stream) if stream else None), "gfs_klt_build_pyramid_device")

    def build_pyramid_clahe_device(self, clahe, d_images, stride, B, pyramid, d_equalized=None, eq_stride=0, stream=None):
        """The device form with CLAHE in front; d_equalized None: the equalised images stay in the Clahe handle's scratch."""
        _check(lib().gfs_klt_build_pyramid_clahe_device(self.h, clahe.h, pyramid.h, C.c_void_p(d_images), stride, B,
                                                        C.c_void_p(d_equalized) if d_equalized else None, eq_stride,
                                                        C.c_void_p(stream) if stream else None), "gfs_klt_build_pyramid_clahe_device")

    @staticmethod
    def _lists(pts):
        if isinstance(pts, np.ndarray):
            pts = [pts]
        return [np.ascontiguousarray(p, np.float32).reshape(-1, 2) for p in pts]

    def calcOpticalFlowPyrLK(self, prev, nxt, prev_pts, next_pts=None, max_level=3, max_iter=30, eps=0.01, flags=0, min_eig_thr=1e-4):
        """Batched cv::calcOpticalFlowPyrLK: prev_pts = [n, 2] array or one per pair -> list of (next_pts, status, err) (a single
        tuple when a single array was given)."""
        single = isinstance(prev_pts, np.ndarray)
        P = self._lists(prev_pts)
        B = len(P)
        N = [np.zeros((max(len(p), 1), 2), np.float32) for p in P]
        if next_pts is not None:
            for dst, src in zip(N, self._lists(next_pts)):
                dst[:len(src)] = src
        S = [np.zeros(max(len(p), 1), np.uint8) for p in P]
        E = [np.zeros(max(len(p), 1), np.float32) for p in P]
        n = np.array([len(p) for p in P], np.int32)
        arr = lambda L: (C.c_void_p * B)(*[a.ctypes.data for a in L])
        _check(lib().gfs_klt_track(self.h, prev.h, nxt.h, B, _p(n), arr(P), arr(N), arr(S), arr(E), max_level, max_iter, float(eps),
                                   flags, float(min_eig_thr)), "gfs_klt_track")
        out = [(N[b][:n[b]].copy(), S[b][:n[b]].copy(), E[b][:n[b]].copy()) for b in range(B)]
        return out[0] if single else out

    def fbKltTracking(self, prev, cur, nbpyrlvl, ferr, fmax_fbklt_dist, kps, priors):
        """Batched ORBmatcher::fbKltTracking -> list of (priors_out, kpstatus bool, n_good) (a single tuple for a single array)."""
        single = isinstance(kps, np.ndarray)
        K = self._lists(kps)
        B = len(K)
        Pr = [np.zeros((max(len(k), 1), 2), np.float32) for k in K]
        for dst, src in zip(Pr, self._lists(priors)):
            dst[:len(src)] = src
        S = [np.zeros(max(len(k), 1), np.uint8) for k in K]
        n = np.array([len(k) for k in K], np.int32)
        good = np.zeros(B, np.int32)
        arr = lambda L: (C.c_void_p * B)(*[a.ctypes.data for a in L])
        _check(lib().gfs_klt_fb_track(self.h, prev.h, cur.h, B, _p(n), arr(K), arr(Pr), arr(S), _p(good), nbpyrlvl, ferr,
                                      fmax_fbklt_dist), "gfs_klt_fb_track")
        out = [(Pr[b][:n[b]].copy(), S[b][:n[b]].astype(bool), int(good[b])) for b in range(B)]
        return out[0] if single else out

    def compact_tracks_device(self, B, pt_stride, d_n, d_kps, d_priors, d_kpstatus, d_a, d_b, d_index, d_m, stream=None):
        _check(lib().gfs_klt_compact_tracks_device(self.h, B, pt_stride, C.c_void_p(d_n), C.c_void_p(d_kps), C.c_void_p(d_priors),
                                                   C.c_void_p(d_kpstatus), C.c_void_p(d_a), C.c_void_p(d_b), C.c_void_p(d_index),
                                                   C.c_void_p(d_m), C.c_void_p(stream) if stream else None),
               "gfs_klt_compact_tracks_device")

    def apply_mask_device(self, B, pt_stride, d_m, d_index, d_mask, d_kpstatus, stream=None):
        _check(lib().gfs_klt_apply_mask_device(self.h, B, pt_stride, C.c_void_p(d_m), C.c_void_p(d_index), C.c_void_p(d_mask),
                                               C.c_void_p(d_kpstatus), C.c_void_p(stream) if stream else None),
               "gfs_klt_apply_mask_device")

    def fb_track_device(self, prev, cur, B, pt_stride, d_n, d_kps, d_priors, d_kpstatus, d_n_good, nbpyrlvl=3, ferr=15.0,
                        fmax_fbklt_dist=0.5, stream=None):
        _check(lib().gfs_klt_fb_track_device(self.h, prev.h, cur.h, B, pt_stride, C.c_void_p(d_n), C.c_void_p(d_kps),
                                             C.c_void_p(d_priors), C.c_void_p(d_kpstatus), C.c_void_p(d_n_good), nbpyrlvl, ferr,
                                             fmax_fbklt_dist, C.c_void_p(stream) if stream else None), "gfs_klt_fb_track_device")


class FundamentalMatcher:
    """cv::findFundamentalMat(pts1, pts2, cv::FM_RANSAC, threshold, confidence, mask) (reference call sites src/ORBmatcher.cc:236,
    2399, 2463; src/Tracking.cc:1974): RANSAC for 15 or more points, LMedS for 8 .. 14 like the cv:: wrapper."""

    def __init__(self, max_points=4096, max_batch=1, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_fmat_create(device, max_points, max_batch, C.byref(self.h)), "gfs_fmat_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_fmat_destroy(self.h)
        self.h = None

    __del__ = close

    def findFundamentalMat(self, pts1, pts2, threshold=3.0, confidence=0.99, max_iters=1000):
        """pts1 / pts2: [n, 2] arrays or lists of them -> (mask bool [n], F [3, 3] or None, n_inliers) per problem."""
        single = isinstance(pts1, np.ndarray)
        P1 = [np.ascontiguousarray(p, np.float32).reshape(-1, 2) for p in ([pts1] if single else pts1)]
        P2 = [np.ascontiguousarray(p, np.float32).reshape(-1, 2) for p in ([pts2] if single else pts2)]
        B = len(P1)
        n = np.array([len(p) for p in P1], np.int32)
        M = [np.zeros(max(len(p), 1), np.uint8) for p in P1]
        F = np.zeros((B, 9))
        cnt = np.zeros(B, np.int32)
        arr = lambda L: (C.c_void_p * B)(*[a.ctypes.data for a in L])
        _check(lib().gfs_find_fundamental_ransac(self.h, B, _p(n), arr(P1), arr(P2), float(threshold), float(confidence), max_iters,
                                                 arr(M), _p(F), _p(cnt)), "gfs_find_fundamental_ransac")
        out = [(M[b][:n[b]].astype(bool), F[b].reshape(3, 3).copy() if cnt[b] > 0 and F[b].any() else None, int(cnt[b])) for b in range(B)]
        return out[0] if single else out

    def find_device(self, B, stride, d_n, d_pts1, d_pts2, d_mask, threshold=3.0, confidence=0.99, max_iters=1000):
        """Device-resident batch -> (F [B, 3, 3], n_inliers [B]); the masks are written to d_mask [B][stride]."""
        F = np.zeros((B, 9))
        cnt = np.zeros(B, np.int32)
        _check(lib().gfs_find_fundamental_ransac_device(self.h, B, stride, C.c_void_p(d_n), C.c_void_p(d_pts1), C.c_void_p(d_pts2),
                                                        float(threshold), float(confidence), max_iters, C.c_void_p(d_mask), _p(F),
                                                        _p(cnt)), "gfs_find_fundamental_ransac_device")
        return F.reshape(B, 3, 3), cnt


class ProjectionMatcher:
    """ORB_SLAM3::ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (reference include/ORBmatcher.h,
    src/ORBmatcher.cc:1853-2063) on flattened single-camera frame pairs (gfs_sbp_problem in include/gfs_abi.h)."""

    def __init__(self, max_last=2048, max_cur=2048, max_batch=64, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_sbp_create(device, max_last, max_cur, max_batch, C.byref(self.h)), "gfs_sbp_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_sbp_destroy(self.h)
        self.h = None

    __del__ = close

    def SearchByProjection(self, pairs):
        """pairs: one problem dict or a list -> (cur_match int32 [n_cur], nmatches) per pair."""
        single = isinstance(pairs, dict)
        probs = [pairs] if single else list(pairs)
        B = len(probs)
        PP = (SbpProblem * B)()
        keeps, outs = [], []
        ptrs = (C.c_void_p * B)()
        for f, prob in enumerate(probs):
            P, keep = sbp_struct(prob)
            PP[f] = P
            keeps.append(keep)
            outs.append(np.full(max(P.n_cur, 1), -9, np.int32))
            ptrs[f] = outs[f].ctypes.data
        nm = np.zeros(B, np.int32)
        _check(lib().gfs_search_by_projection(self.h, PP, B, ptrs, _p(nm)), "gfs_search_by_projection")
        res = [(outs[f][:PP[f].n_cur].copy(), int(nm[f])) for f in range(B)]
        return res[0] if single else res


    def SearchByProjectionMap(self, frames):
        """ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) (src/ORBmatcher.cc:43-206):
        one problem dict (keys of gfs_sbp_map_problem) or a list -> (cur_match int32 [n_cur], nmatches) per frame."""
        single = isinstance(frames, dict)
        probs = [frames] if single else list(frames)
        B = len(probs)
        PP = (SbpMapProblem * B)()
        keeps, outs = [], []
        ptrs = (C.c_void_p * B)()
        for f, prob in enumerate(probs):
            P, keep = sbp_map_struct(prob)
            PP[f] = P
            keeps.append(keep)
            outs.append(np.full(max(P.n_cur, 1), -9, np.int32))
            ptrs[f] = outs[f].ctypes.data
        nm = np.zeros(B, np.int32)
        _check(lib().gfs_search_by_projection_map(self.h, PP, B, ptrs, _p(nm)), "gfs_search_by_projection_map")
        res = [(outs[f][:PP[f].n_cur].copy(), int(nm[f])) for f in range(B)]
        return res[0] if single else res


    def reserve_local(self, max_local_points):
        """Workspace of search_local_points for lists of up to max_local_points map points per frame."""
        _check(lib().gfs_sbp_reserve_local(self.h, int(max_local_points)), "gfs_sbp_reserve_local")
        self.max_local = int(max_local_points)

    def search_local_points(self, frames):
        """Tracking::SearchLocalPoints from its second loop on (src/Tracking.cc:4312-4358): Frame::isInFrustum + PredictScale for
        every listed local map point, the far-points filter and SearchByProjection over the survivors, in one device call.
        One problem dict (keys of gfs_local_points_problem) or a list -> per frame a dict in_view, proj [n][3], depth, view_cos,
        level, cur_match (indices into the caller's list), n_to_match, n_searched, nmatches.  Raises GfsError (code
        GFS_ERR_CAPACITY) when a list exceeds the reserve or a search set exceeds max_last."""
        single = isinstance(frames, dict)
        probs = [frames] if single else list(frames)
        B = len(probs)
        if getattr(self, "max_local", 0) <= 0:
            self.reserve_local(max(max(len(p["mp_xw"]) for p in probs), 64))
        PP, RR = (LocalPointsProblem * B)(), (LocalPointsResult * B)()
        keeps = []
        for f, prob in enumerate(probs):
            PP[f], RR[f], keep = local_points_structs(prob)
            keeps.append(keep)
        _check(lib().gfs_search_local_points(self.h, PP, B, RR), "gfs_search_local_points")
        res = [local_points_result(PP[f], RR[f], keeps[f]) for f in range(B)]
        return res[0] if single else res

    def reserve_fuse(self, max_lists, max_points_per_list, max_keyframes):
        """Workspace of fuse_search: up to max_lists point lists of up to max_points_per_list map points, searched in up to
        max_keyframes key frames per call."""
        _check(lib().gfs_sbp_reserve_fuse(self.h, int(max_lists), int(max_points_per_list), int(max_keyframes)), "gfs_sbp_reserve_fuse")
        self.fuse_reserve = (int(max_lists), int(max_points_per_list), int(max_keyframes))

    def fuse_search(self, lists, keyframes):
        """The search of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:1424-1526) for every listed map point, any number
        of (list, key frame) pairs in one device call.  lists: one dict (keys of gfs_fuse_points) or a list of them; keyframes:
        one dict (keys of gfs_fuse_keyframe, `list` = index of its point list) or a list -> per key frame a dict exit (index into
        FUSE_EXITS), best_idx, best_dist, level, n_matched.  Raises GfsError (code GFS_ERR_CAPACITY) beyond the reserve."""
        single = isinstance(keyframes, dict)
        lists = [lists] if isinstance(lists, dict) else list(lists)
        kfs = [keyframes] if single else list(keyframes)
        if not hasattr(self, "fuse_reserve"):
            self.reserve_fuse(max(len(lists), 1), max(max([len(p["mp_xw"]) for p in lists] + [64]), 64), max(len(kfs), 1))
        LL, KK, RR, keep = fuse_structs(lists, kfs)
        _check(lib().gfs_fuse_search(self.h, LL, len(lists), KK, len(kfs), RR), "gfs_fuse_search")
        res = fuse_results(LL, KK, RR, keep, len(lists))
        return res[0] if single else res

    def reserve_sim3_search(self, max_lists, max_points_per_list, max_problems):
        """Workspace of sim3_search: up to max_lists point lists of up to max_points_per_list map points, searched in up to
        max_problems problems per call."""
        _check(lib().gfs_sbp_reserve_sim3_search(self.h, int(max_lists), int(max_points_per_list), int(max_problems)), "gfs_sbp_reserve_sim3_search")
        self.sim3_reserve = (int(max_lists), int(max_points_per_list), int(max_problems))

    def sim3_search(self, lists, problems):
        """The three Sim3 searches of loop closing -- ORBmatcher::Fuse(pKF, Scw, ...) (src/ORBmatcher.cc:1550-1654, mode SIM3_FUSE) and
        the two SearchByProjection(pKF, Scw, ...) (:432-529 SIM3_SBP, :531-636 SIM3_SBP_KFS) -- for every listed map point, any number
        of (list, problem) pairs in one device call.  lists: one dict (keys of gfs_fuse_points) or a list of them; problems: one dict
        (keys of gfs_sim3_search_problem, `list` = index of its point list) or a list -> per problem a dict exit (index into
        SIM3_SEARCH_EXITS), best_idx, best_dist, level, n_matched; in the projection modes after the dependency between the points
        of a list.  Raises GfsError (code GFS_ERR_CAPACITY beyond the reserve, GFS_ERR_INVALID_ARG for what the entry refuses)."""
        single = isinstance(problems, dict)
        lists = [lists] if isinstance(lists, dict) else list(lists)
        probs = [problems] if single else list(problems)
        if not hasattr(self, "sim3_reserve"):
            self.reserve_sim3_search(max(len(lists), 1), max(max([len(p["mp_xw"]) for p in lists] + [64]), 64), max(len(probs), 1))
        LL, PP, RR, keep = sim3_search_structs(lists, probs)
        _check(lib().gfs_sim3_search(self.h, LL, len(lists), PP, len(probs), RR), "gfs_sim3_search")
        res = sim3_search_results(LL, PP, RR, keep, len(lists))
        return res[0] if single else res

    def reserve_triangulation(self, max_neighbours, max_candidate_pairs):
        """Workspace of create_new_map_points: up to max_neighbours neighbour key frames per problem, and up to max_candidate_pairs
        for the sum of n1 * n2 over the common vocabulary nodes of all neighbours of one problem."""
        _check(lib().gfs_sbp_reserve_triangulation(self.h, int(max_neighbours), int(max_candidate_pairs)), "gfs_sbp_reserve_triangulation")
        self.tri_reserve = (int(max_neighbours), int(max_candidate_pairs))

    def create_new_map_points(self, problems):
        """LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:846-1100) for one problem dict or a list of them (tri_structs), one
        device call: per problem a list with one dict per neighbour, in the loop's order: match12 (SearchForTriangulation's pairs),
        exit (index into TRI_EXITS), x3d, point_stereo, n_matches, n_created.  A point created at one neighbour takes its idx1 out of
        the searches at the later ones.  Raises GfsError (code GFS_ERR_CAPACITY) beyond the reserve."""
        single = isinstance(problems, dict)
        probs = [problems] if single else list(problems)
        if not hasattr(self, "tri_reserve"):
            self.reserve_triangulation(max([len(p["neighbours"]) for p in probs] + [1]), max([tri_candidate_pairs(p) for p in probs] + [1]))
        PP, RP, keep = tri_structs(probs)
        _check(lib().gfs_create_new_map_points(self.h, PP, len(probs), RP), "gfs_create_new_map_points")
        res = tri_results(PP, RP, keep, len(probs))
        return res[0] if single else res

    def reserve_bow(self, max_problems, max_kf2_per_call):
        """Workspace of search_by_bow: up to max_problems key frames 1 and up to max_kf2_per_call key frames 2 (over all problems)
        per call."""
        _check(lib().gfs_sbp_reserve_bow(self.h, int(max_problems), int(max_kf2_per_call)), "gfs_sbp_reserve_bow")
        self.bow_reserve = (int(max_problems), int(max_kf2_per_call))

    def search_by_bow(self, problems):
        """ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (src/ORBmatcher.cc:936-1053) for one problem dict or a list of them
        (bow_structs), every (key frame 1, key frame 2) pair in one device call: per problem a list with one dict per key frame 2:
        match12 (idx2 or -1, after the orientation check) and n_matches.  Raises GfsError (code GFS_ERR_CAPACITY beyond the
        reserve, GFS_ERR_INVALID_ARG for what the entry refuses)."""
        single = isinstance(problems, dict)
        probs = [problems] if single else list(problems)
        if not hasattr(self, "bow_reserve"):
            self.reserve_bow(max(len(probs), 1), max(sum(len(p["kf2"]) for p in probs), 1))
        PP, RP, keep = bow_structs(probs)
        _check(lib().gfs_search_by_bow(self.h, PP, len(probs), RP), "gfs_search_by_bow")
        res = bow_results(PP, RP, keep, len(probs))
        return res[0] if single else res


class MapPointUpdater:
    """MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:376-448, :468-532) for
    any number of map points in one device call (gfs_map_points_problem in include/gfs_abi.h)."""

    def __init__(self, max_points=4096, max_observations=65536, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_map_points_create(device, int(max_points), int(max_observations), C.byref(self.h)), "gfs_map_points_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_map_points_destroy(self.h)
        self.h = None

    __del__ = close

    def update(self, problem, normals_only=False):
        """problem: a dict with the keys of gfs_map_points_problem (synth.map_point_update_problem) -> dict of best_obs, best_median,
        normal [n, 3], min_dist, max_dist, status.  normals_only: UpdateNormalAndDepth alone; no descriptor is uploaded and best_obs
        and best_median are -1."""
        P, R, keep = map_points_structs(problem, normals_only)
        _check(lib().gfs_map_points_update(self.h, C.byref(P), C.byref(R)), "gfs_map_points_update")
        return map_points_results(P, keep)


class PoseOptimizer:
    """ORB_SLAM3::Optimizer::PoseOptimization (reference include/Optimizer.h, src/Optimizer.cc:763-1098), conventional-SLAM
    branch, on flattened frames (gfs_pose_problem in include/gfs_abi.h).  A batch of frames is one kernel launch."""

    SUMS_TREE, SUMS_EDGE_ORDER = 0, 1  # GFS_POSE_SUMS_* (include/gfs_abi.h)

    def __init__(self, max_obs=4096, max_batch=64, device=0, sums=None):
        """sums: None = the library's default (g2o's edge order on one lane: the bits of the sequential code, the reference's outlier
        flags), "edge_order" = the same, said explicitly, or "tree" (opt-in: sums over the edges by a fixed-shape tree, about half the
        latency of a single frame, flags equal up to chi2-threshold ties)."""
        self.h = C.c_void_p()
        _check(lib().gfs_pose_create(device, max_obs, max_batch, C.byref(self.h)), "gfs_pose_create")
        if sums is not None:
            _check(lib().gfs_pose_set_sum_order(self.h, {"tree": 0, "edge_order": 1}[sums]), "gfs_pose_set_sum_order")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_pose_destroy(self.h)
        self.h = None

    __del__ = close

    def PoseOptimization(self, frames):
        """frames: one problem dict or a list of them -> result dict(s) (outlier, chi2, q, t, avg_reproj_error, n_inliers)."""
        single = isinstance(frames, dict)
        probs = [frames] if single else list(frames)
        B = len(probs)
        PP, SS = (PoseProblem * B)(), (PoseSolution * B)()
        keeps = []
        for f, prob in enumerate(probs):
            P, S, keep, n = pose_structs(prob)
            PP[f], SS[f] = P, S
            keeps.append((keep, n))
        _check(lib().gfs_pose_optimize(self.h, PP, B, SS), "gfs_pose_optimize")
        res = [pose_result(SS[f], *keeps[f]) for f in range(B)]
        return res[0] if single else res


class Sim3Optimizer:
    """ORB_SLAM3::Optimizer::OptimizeSim3 (reference src/Optimizer.cc:2797-3054) on flattened pairs (gfs_sim3_opt_problem in
    include/gfs_abi.h).  A batch of problems is one kernel launch, one workgroup each."""

    def __init__(self, max_batch=16, max_pairs=2048, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_sim3_opt_create(device, int(max_batch), int(max_pairs), C.byref(self.h)), "gfs_sim3_opt_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_sim3_opt_destroy(self.h)
        self.h = None

    __del__ = close

    def OptimizeSim3(self, problems):
        """problems: one problem dict or a list of them (sim3_opt_structs) -> result dict(s): s12 [8] (the input after the early
        return), n_in, n_bad, status (SIM3_OPT_*), iterations_run (two), pair_state [n] (SIM3_PAIR_*), chi2 [n, 2].  Raises GfsError
        (code GFS_ERR_CAPACITY / GFS_ERR_INVALID_ARG) on a refusal; the handle stays usable."""
        single = isinstance(problems, dict)
        probs = [problems] if single else list(problems)
        B = len(probs)
        PP, SS = (Sim3OptProblem * max(B, 1))(), (Sim3OptSolution * max(B, 1))()
        keeps = []
        for f, prob in enumerate(probs):
            P, S, keep, n = sim3_opt_structs(prob)
            PP[f], SS[f] = P, S
            keeps.append((keep, n))
        _check(lib().gfs_sim3_optimize(self.h, PP, B, SS), "gfs_sim3_optimize")
        res = [sim3_opt_result(SS[f], *keeps[f]) for f in range(B)]
        return res[0] if single else res


class Sim3RansacSolver:
    """ORB_SLAM3::Sim3Solver (reference src/Sim3Solver.cc) on flattened pairs (gfs_sim3_ransac_problem in include/gfs_abi.h; DESIGN.md
    section 23): every hypothesis of every problem of a call is scored at once, the result is what the sequential loop returns."""

    def __init__(self, max_batch=8, max_pairs=2048, max_iterations=300, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_sim3_ransac_create(device, int(max_batch), int(max_pairs), int(max_iterations), C.byref(self.h)), "gfs_sim3_ransac_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_sim3_ransac_destroy(self.h)
        self.h = None

    __del__ = close

    @staticmethod
    def iterations(n_pairs, probability=0.99, min_inliers=6, max_iterations=300):
        """Sim3Solver::SetRansacParameters: mRansacMaxIts for n_pairs correspondences."""
        return int(lib().gfs_sim3_ransac_iterations(int(n_pairs), float(probability), int(min_inliers), int(max_iterations)))

    def solve(self, problems):
        """problems: one problem dict or a list of them (sim3_ransac_structs) -> result dict(s): T12 [4, 4], R12 [3, 3], t12 [3], s12,
        n_inliers, iterations, status (SIM3_RANSAC_*), inlier [n], counts [n_iterations] (every hypothesis's count).  Raises GfsError
        (code GFS_ERR_CAPACITY / GFS_ERR_INVALID_ARG) on a refusal; the handle stays usable."""
        single = isinstance(problems, dict)
        probs = [problems] if single else list(problems)
        B = len(probs)
        PP, SS = (Sim3RansacProblem * max(B, 1))(), (Sim3RansacSolution * max(B, 1))()
        keeps = []
        for f, prob in enumerate(probs):
            P, S, keep, n = sim3_ransac_structs(prob)
            PP[f], SS[f] = P, S
            keeps.append((keep, n))
        _check(lib().gfs_sim3_ransac_solve(self.h, PP, B, SS), "gfs_sim3_ransac_solve")
        res = [sim3_ransac_result(SS[f], *keeps[f]) for f in range(B)]
        return res[0] if single else res


class PoseInertialOptimizer:
    """Optimizer::PoseInertialOptimizationLastKeyFrame / ...LastFrame (reference src/Optimizer.cc:5899-6283, 6762-7171) on flattened
    problems (gfs_pose_inertial_problem in include/gfs_abi.h): a batch of problems, the two modes mixed freely,
    in one device call; every output is the sequential restatement's byte for byte."""

    def __init__(self, max_obs=2048, max_batch=8, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_pose_inertial_create(device, int(max_obs), int(max_batch), C.byref(self.h)), "gfs_pose_inertial_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_pose_inertial_destroy(self.h)
        self.h = None

    __del__ = close

    def optimize(self, problems):
        """problems: one problem dict or a list of them (pose_inertial_structs) -> result dict(s): cur / other (Rwb, twb, v, bg, ba as
        doubles), outlier [n], n_good (the reference's return value), n_inliers, rounds_run, avg_reproj (float32), H [15, 15] or
        [30, 30] before Marginalize.  Raises GfsError (GFS_ERR_CAPACITY / GFS_ERR_INVALID_ARG) on a refusal; the handle stays usable."""
        single = isinstance(problems, dict)
        probs = [problems] if single else list(problems)
        B = len(probs)
        PP, SS = (PoseInertialProblem * max(B, 1))(), (PoseInertialSolution * max(B, 1))()
        keeps = []
        for f, prob in enumerate(probs):
            P, S, keep, n = pose_inertial_structs(prob)
            PP[f], SS[f] = P, S
            keeps.append((keep, n, P.mode))
        _check(lib().gfs_pose_inertial_optimize(self.h, PP, B, SS), "gfs_pose_inertial_optimize")
        res = [pose_inertial_result(SS[f], *keeps[f]) for f in range(B)]
        return res[0] if single else res


class PoseLidarInertialOptimizer:
    """Optimizer::PoseLidarVisualInertialOptimizationLastKeyFrame / ...LastFrame (reference src/Optimizer.cc:6285-6760, 7173-7678) on
    flattened problems (gfs_pose_lidar_inertial_problem in include/gfs_abi.h): the inertial pose graph plus, in
    every round, the point-to-plane edges of the frame's cloud against a LidarMap.  A problem dict carries its map under "map" (a
    LidarMap, or None without a cloud); every output is the sequential restatement's byte for byte."""

    def __init__(self, max_obs=2048, max_cloud=8192, max_batch=8, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_pose_lidar_inertial_create(device, int(max_obs), int(max_cloud), int(max_batch), C.byref(self.h)),
               "gfs_pose_lidar_inertial_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_pose_lidar_inertial_destroy(self.h)
        self.h = None

    __del__ = close

    def optimize(self, problems):
        """problems: one problem dict or a list of them (pose_lidar_inertial_structs) -> result dict(s): those of
        PoseInertialOptimizer.optimize plus n_lidar_inliers, residual (float32), round_edges / round_chi2 / round_valid [4].  Raises
        GfsError (GFS_ERR_CAPACITY / GFS_ERR_INVALID_ARG) on a refusal; the handle stays usable."""
        single = isinstance(problems, dict)
        probs = [problems] if single else list(problems)
        B = len(probs)
        PP, SS = (PoseLidarInertialProblem * max(B, 1))(), (PoseLidarInertialSolution * max(B, 1))()
        keeps = []
        for f, prob in enumerate(probs):
            m = prob.get("map")
            P, S, keep, n = pose_lidar_inertial_structs(prob, m.h if m is not None else None)
            PP[f], SS[f] = P, S
            keeps.append((keep, n, P.vi.mode))
        _check(lib().gfs_pose_lidar_inertial_optimize(self.h, PP, B, SS), "gfs_pose_lidar_inertial_optimize")
        res = [pose_lidar_inertial_result(SS[f], *keeps[f]) for f in range(B)]
        return res[0] if single else res

    def fetch_edges(self, b, rnd, cap=8192):
        """The lidar edges problem b of the last call generated in round rnd: (index [n], plane [n][4], s [n])."""
        idx, pl, s, n = np.zeros(cap, np.int32), np.zeros((cap, 4), np.float32), np.zeros(cap, np.float32), C.c_int32()
        _check(lib().gfs_pose_lidar_inertial_fetch_edges(self.h, b, rnd, _p(idx), _p(pl), _p(s), cap, C.byref(n)),
               "gfs_pose_lidar_inertial_fetch_edges")
        m = min(n.value, cap)
        return idx[:m].copy(), pl[:m].copy(), s[:m].copy()


class LocalInertialBA:
    """Optimizer::LocalInertialBA's numeric core (reference src/Optimizer.cc:3589-3626) on one flattened window
    (gfs_lba_inertial_problem in include/gfs_abi.h): one Levenberg optimize() over the window's key frames
    (15 unknowns each), the marginalised map points and the inertial edges, queued at once with the trial decisions on the device;
    every output is the sequential restatement's byte for byte."""

    def __init__(self, max_opt=20, max_fixed=200, max_points=4096, max_edges=65536, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_lba_inertial_create(device, int(max_opt), int(max_fixed), int(max_points), int(max_edges), C.byref(self.h)),
               "gfs_lba_inertial_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_lba_inertial_destroy(self.h)
        self.h = None

    __del__ = close

    def solve(self, problem):
        """problem: a window dict (lba_inertial_structs) -> dict(window: list of state dicts as doubles, points [P, 3], edge_chi2 [E],
        edge_depth_positive, edge_erase [E] uint8, err, err_end (float32), iterations_run, trials_run, final_lambda).  Raises GfsError
        (GFS_ERR_CAPACITY / GFS_ERR_INVALID_ARG / GFS_ERR_UNSUPPORTED) on a refusal; the handle stays usable."""
        P, S, keep = lba_inertial_structs(problem)
        _check(lib().gfs_lba_inertial_solve(self.h, C.byref(P), C.byref(S)), "gfs_lba_inertial_solve")
        return lba_inertial_result(S, keep, problem)


class BowVocabulary:
    """DBoW2::TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) (TF_IDF, L1_NORM) as KeyFrame::ComputeBoW and
    Frame::ComputeBoW call it, for any number of frames in one device call (gfs_bow_* in include/gfs_abi.h).
    vocab_dict: the tree as gfs_bow_vocabulary lays it out (synth.bow_vocabulary builds one); it is validated, repacked and uploaded."""

    def __init__(self, vocab_dict, max_batch=8, max_features=2048, device=0):
        self.h = C.c_void_p()
        self.max_features = int(max_features)
        V, keep = bow_vocabulary_struct(vocab_dict)
        _check(lib().gfs_bow_create(device, C.byref(V), int(max_batch), int(max_features), C.byref(self.h)), "gfs_bow_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_bow_destroy(self.h)
        self.h = None

    __del__ = close

    def transform(self, descs, levelsup=4):
        """descs: one uint8 array [n, 32] or a list of them -> result dict(s) (bow_vectors_results).  Raises GfsError (code
        GFS_ERR_CAPACITY / GFS_ERR_INVALID_ARG) on a refusal; the handle stays usable."""
        single, frames = bow_frames(descs)
        B = len(frames)
        ptrs = (C.c_void_p * max(B, 1))(*[f.ctypes.data for f in frames])
        n = np.array([len(f) for f in frames], np.int32)
        VV, keep = bow_vectors_alloc(B, self.max_features)
        _check(lib().gfs_bow_transform(self.h, ptrs, _p(n), B, int(levelsup), VV), "gfs_bow_transform")
        res = bow_vectors_results(VV, keep, n)
        return res[0] if single else res

    def transform_device(self, dev_desc, dev_counts, stride, B, levelsup=4, counts=None):
        """The same on descriptors in HBM as ORBextractor.device_results() leaves them ([B][stride][32] u8, [B] int32 counts); counts:
        the host's copy of the counts where it has one (word_of_feature is cut to it, else left out)."""
        VV, keep = bow_vectors_alloc(B, self.max_features)
        _check(lib().gfs_bow_transform_device(self.h, C.c_void_p(dev_desc), C.c_void_p(dev_counts), int(stride), int(B), int(levelsup), VV),
               "gfs_bow_transform_device")
        return bow_vectors_results(VV, keep, counts)


class BowDatabase:
    """The numeric core of KeyFrameDatabase::DetectNBestCandidates (reference src/KeyFrameDatabase.cc:596-645): a fixed-stride store of
    BowVectors, one slot per key frame, and the query of one BowVector against all of them (gfs_bow_db_* in include/gfs_abi.h)."""

    def __init__(self, max_entries=1024, max_words=2048, device=0):
        self.h = C.c_void_p()
        self.max_entries = int(max_entries)
        _check(lib().gfs_bow_db_create(device, int(max_entries), int(max_words), C.byref(self.h)), "gfs_bow_db_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_bow_db_destroy(self.h)
        self.h = None

    __del__ = close

    @staticmethod
    def _vector(word_id, word_value):
        ids, vals = np.ascontiguousarray(word_id, np.int32).ravel(), np.ascontiguousarray(word_value, np.float64).ravel()
        if len(ids) != len(vals):
            raise ValueError("BowDatabase: word_id and word_value differ in length")
        return ids, vals

    def add(self, slot, word_id, word_value):
        ids, vals = self._vector(word_id, word_value)
        _check(lib().gfs_bow_db_add(self.h, int(slot), len(ids), _p(ids), _p(vals)), "gfs_bow_db_add")

    def erase(self, slot):
        _check(lib().gfs_bow_db_erase(self.h, int(slot)), "gfs_bow_db_erase")

    def query(self, word_id, word_value):
        """-> dict(n_common, first_word, score), each [max_entries]: mnPlaceRecognitionWords, the lowest common word id (-1: none) and
        (float)L1Scoring::score of every slot against the query"""
        ids, vals = self._vector(word_id, word_value)
        out = dict(n_common=np.full(self.max_entries, -7, np.int32), first_word=np.full(self.max_entries, -7, np.int32),
                   score=np.full(self.max_entries, np.nan, np.float32))
        _check(lib().gfs_bow_db_query(self.h, len(ids), _p(ids), _p(vals), _p(out["n_common"]), _p(out["first_word"]), _p(out["score"])),
               "gfs_bow_db_query")
        return out


class LidarMap:
    """The local map of PoseLidarVisualOptimization (laserCloudSurfFromMapDS, reference src/Optimizer.cc:7698-8059) on the device:
    uploaded once with set(), reused by every frame until the next set() (gfs_lidar_map_* in include/gfs_abi.h)."""

    def __init__(self, max_points=65536, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_lidar_map_create(device, max_points, C.byref(self.h)), "gfs_lidar_map_create")

    def set(self, xyz):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        _check(lib().gfs_lidar_map_set(self.h, _p(xyz), len(xyz)), "gfs_lidar_map_set")
        return self

    def fetch(self):
        """The map's points in map-index order (LidarMapping::GetLocalMap), float32 [n][3]."""
        n = C.c_int32()
        _check(lib().gfs_lidar_map_fetch(self.h, None, 0, C.byref(n)), "gfs_lidar_map_fetch")
        xyz = np.zeros((max(n.value, 1), 3), np.float32)
        _check(lib().gfs_lidar_map_fetch(self.h, _p(xyz), n.value, C.byref(n)), "gfs_lidar_map_fetch")
        return xyz[:n.value].copy()

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_lidar_map_destroy(self.h)
        self.h = None

    __del__ = close


class LidarMapper:
    """The local map of LidarMapping::viewer (reference src/LidarMapping.cc:130-185) built on the device: the key-frames' clouds
    transformed by their poses, concatenated, voxel-filtered under the rule of DESIGN.md section 11 and laid out in the search grid of
    a LidarMap (gfs_lidar_mapper_* / gfs_lidar_map_build in include/gfs_abi.h)."""

    def __init__(self, max_points_in=131072, max_keyframes=30, device=0):
        self.h = C.c_void_p()
        self.max_points_in = max_points_in
        _check(lib().gfs_lidar_mapper_create(device, max_points_in, max_keyframes, C.byref(self.h)), "gfs_lidar_mapper_create")

    def build(self, lidar_map, q, t, clouds, leaf):
        """q [K][4], t [K][3]: the key-frames' stored Tcw; clouds: K arrays [n_k][3] (camera frame; empty ones allowed); leaf:
        LidarMapping.LocalResolution.  Fills lidar_map; -> info dict (n_in, n_out, passthrough, div).  A refused build raises and leaves
        lidar_map as it was."""
        q = np.ascontiguousarray(q, np.float32).reshape(-1, 4)
        t = np.ascontiguousarray(t, np.float32).reshape(-1, 3)
        clouds = [np.asarray(c, np.float32).reshape(-1, 3) for c in clouds]
        if not (len(q) == len(t) == len(clouds)):
            raise ValueError("LidarMapper.build: q, t and clouds differ in length")
        cb = np.r_[0, np.cumsum([len(c) for c in clouds])].astype(np.int32)
        cloud = np.ascontiguousarray(np.concatenate(clouds) if clouds else np.zeros((0, 3)), np.float32).reshape(-1, 3)
        I = LidarMapInput(len(q), q.ctypes.data, t.ctypes.data, cb.ctypes.data, cloud.ctypes.data, float(np.float32(leaf)))
        info = LidarMapInfo()
        self.last_info = info
        _check(lib().gfs_lidar_map_build(self.h, C.byref(I), lidar_map.h, C.byref(info)), "gfs_lidar_map_build")
        return lidar_map_info(info)

    def voxel_filter(self, xyz, leaf, cap=None):
        """pcl::VoxelGrid (default settings) of one cloud under the same rule -> (xyz [n_out][3] float32, info)."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        cap = len(xyz) if cap is None else cap
        out, info = np.zeros((max(cap, 1), 3), np.float32), LidarMapInfo()
        self.last_info = info
        _check(lib().gfs_voxel_grid_filter(self.h, _p(xyz), len(xyz), float(np.float32(leaf)), _p(out), cap, C.byref(info)),
               "gfs_voxel_grid_filter")
        return out[:info.n_out].copy(), lidar_map_info(info)

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_lidar_mapper_destroy(self.h)
        self.h = None

    __del__ = close


class FrameCloud:
    """The lidar-feature tail of the Frame constructor (reference src/Frame.cc:378-393, src/LidarProcess.cc:20-204) on the device:
    featureExtraction of the camera-frame cloud, surf ++ edge (mpPointCloud) and its pcl::VoxelGrid at downsizeResolution()
    (mpPointCloudDownsampled).  The rule is DESIGN.md section 17 (gfs_frame_cloud_* in include/gfs_abi.h)."""

    def __init__(self, max_points=32768, downsize_resolution=0.05, horizontal_angle=None, max_distance=None, local_map_resolution=None,
                 angle_guard_deg=None, device=0):
        """The LidarParam fields default to the reference's (70.0, 9.0, 0.05); angle_guard_deg to 1e-9."""
        cfg = FrameCloudConfig()
        lib().gfs_frame_cloud_default_config(C.byref(cfg))
        cfg.downsize_resolution = float(np.float32(downsize_resolution))
        for k, v in (("horizontal_angle", horizontal_angle), ("max_distance", max_distance), ("local_map_resolution", local_map_resolution),
                     ("angle_guard_deg", angle_guard_deg)):
            if v is not None:
                setattr(cfg, k, float(v))
        self.cfg, self.max_points, self.h = cfg, max_points, C.c_void_p()
        _check(lib().gfs_frame_cloud_create(device, max_points, C.byref(cfg), C.byref(self.h)), "gfs_frame_cloud_create")

    def _call(self, fn, what, args, cap, cap_down, want_cloud):
        cloud = np.zeros((max(cap, 1), 3), np.float32) if want_cloud else None
        down, info = np.zeros((max(cap_down, 1), 3), np.float32), FrameCloudInfo()
        self.last_info = info
        _check(fn(self.h, *args, _p(cloud), cap, _p(down), cap_down, C.byref(info)), what)
        I = frame_cloud_info(info)
        return (cloud[:I["n_surf"] + I["n_edge"]].copy() if want_cloud else None), down[:I["n_down"]].copy(), I

    def extract(self, xyzw, cap=None, cap_down=None, want_cloud=True):
        """xyzw [n][4] (or [n][3]): the cloud of ConvertDepthToPointCloud in push_back order -> (cloud [n_surf + n_edge][3] surf
        first, or None; downsampled cloud [n_down][3]; info dict).  A refused call raises GfsError (err.code)."""
        xyzw = np.asarray(xyzw, np.float32)
        xyzw = xyzw.reshape(-1, xyzw.shape[-1] if xyzw.ndim == 2 else 4)
        if xyzw.shape[1] == 3:
            xyzw = np.concatenate([xyzw, np.ones((len(xyzw), 1), np.float32)], 1)
        xyzw = np.ascontiguousarray(xyzw, np.float32)
        n = len(xyzw)
        return self._call(lib().gfs_frame_cloud_extract, "gfs_frame_cloud_extract", (_p(xyzw) if n else xyzw.ctypes.data_as(C.c_void_p), n),
                          n if cap is None else cap, n if cap_down is None else cap_down, want_cloud)

    def extract_device(self, dev_xyzw, dev_count, cap=None, cap_down=None, want_cloud=True):
        """Same on the cloud Frame.FrameRGBD left on the device (its dev_cloud / dev_count addresses)."""
        return self._call(lib().gfs_frame_cloud_extract_device, "gfs_frame_cloud_extract_device", (C.c_void_p(dev_xyzw), C.c_void_p(dev_count)),
                          self.max_points if cap is None else cap, self.max_points if cap_down is None else cap_down, want_cloud)

    def stages(self):
        """The stages of the last call through the test hook -> dict(scans [n_scans][4], edge_raw, surf_raw, edge_voxel, surf_voxel,
        edge, surf: [n][3] each)."""
        I = frame_cloud_info(self.last_info)
        names = ("edge_raw", "surf_raw", "edge_voxel", "surf_voxel", "edge", "surf")
        out = {k: np.zeros((max(I["n_" + k], 1), 3), np.float32) for k in names}
        out["scans"] = np.zeros((max(I["n_scans"], 1), 4), np.int32)
        B = FrameCloudStageBuffers()
        B.scans, B.cap_scans, B.cap_points = out["scans"].ctypes.data, len(out["scans"]), max(max(I["n_" + k] for k in names), 1)
        for k in names:
            setattr(B, k, out[k].ctypes.data)
        _check(lib().gfs_test_frame_cloud_stages(self.h, C.byref(B)), "gfs_test_frame_cloud_stages")
        out["scans"] = out["scans"][:I["n_scans"]]
        for k in names:
            out[k] = out[k][:I["n_" + k]]
        return out

    def radius_filter(self, xyz, min_pts):
        """The handle's RadiusOutlierRemoval on its own (test hook; radius = local_map_resolution) -> kept points [m][3]."""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        out, n = np.zeros((max(len(xyz), 1), 3), np.float32), C.c_int32()
        _check(lib().gfs_test_frame_cloud_radius(self.h, _p(xyz), len(xyz), min_pts, _p(out), len(xyz), C.byref(n)), "gfs_test_frame_cloud_radius")
        return out[:n.value].copy()

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_frame_cloud_destroy(self.h)
        self.h = None

    __del__ = close


class PoseLidarOptimizer:
    """ORB_SLAM3::Optimizer::PoseLidarVisualOptimization (reference src/Optimizer.cc:7698-8059), conventional-SLAM branch, on
    flattened frames (gfs_pose_lidar_problem in include/gfs_abi.h): the visual edges of PoseOptimization plus point-to-plane edges
    of the frame's cloud against a LidarMap.  A frame dict carries its map under "map" (a LidarMap)."""

    SUMS_TREE, SUMS_EDGE_ORDER = 0, 1

    def __init__(self, max_obs=4096, max_cloud=8192, max_batch=64, device=0, sums=None):
        """sums: None / "edge_order" (g2o's order: the bits of the sequential restatement) or "tree" (opt-in, toleranced)."""
        self.h = C.c_void_p()
        _check(lib().gfs_pose_lidar_create(device, max_obs, max_cloud, max_batch, C.byref(self.h)), "gfs_pose_lidar_create")
        if sums is not None:
            _check(lib().gfs_pose_lidar_set_sum_order(self.h, {"tree": 0, "edge_order": 1}[sums]), "gfs_pose_lidar_set_sum_order")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_pose_lidar_destroy(self.h)
        self.h = None

    __del__ = close

    def PoseLidarVisualOptimization(self, frames):
        """frames: one problem dict or a list of them -> result dict(s): outlier, chi2, q, t (g2o estimate), qf, tf (SetPose),
        avg_reproj_error, n_inliers (the return value), n_lidar_inliers, residual, lidar_rounds, rounds_run, iterations_run,
        round_edges / round_chi2 / round_valid."""
        single = isinstance(frames, dict)
        probs = [frames] if single else list(frames)
        B = len(probs)
        PP, SS = (PoseLidarProblem * B)(), (PoseLidarSolution * B)()
        keeps = []
        for f, prob in enumerate(probs):
            P, S, keep, n = pose_lidar_structs(prob, prob["map"].h)
            PP[f], SS[f] = P, S
            keeps.append((keep, n))
        _check(lib().gfs_pose_lidar_optimize(self.h, PP, B, SS), "gfs_pose_lidar_optimize")
        res = [pose_lidar_result(SS[f], *keeps[f]) for f in range(B)]
        return res[0] if single else res

    def fetch_edges(self, b, rnd, cap=8192):
        """The lidar edges frame b of the last call generated in round rnd: (index [n], plane [n][4], s [n])."""
        idx, pl, s, n = np.zeros(cap, np.int32), np.zeros((cap, 4), np.float32), np.zeros(cap, np.float32), C.c_int32()
        _check(lib().gfs_pose_lidar_fetch_edges(self.h, b, rnd, _p(idx), _p(pl), _p(s), cap, C.byref(n)), "gfs_pose_lidar_fetch_edges")
        m = min(n.value, cap)
        return idx[:m].copy(), pl[:m].copy(), s[:m].copy()


class Frame:
    """The two Frame members next to the hot path (reference src/Frame.cc:590-623 and 1314-1332)."""

    def __init__(self, max_rows=720, max_cols=1280, max_keypoints=8192, device=0):
        self.h = C.c_void_p()
        _check(lib().gfs_frame_create(device, max_rows, max_cols, max_keypoints, C.byref(self.h)), "gfs_frame_create")

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.gfs_frame_destroy(self.h)
        self.h = None

    __del__ = close

    @staticmethod
    def _rows_view(depth):
        """-> (float32 map, row stride in elements): a view whose rows are contiguous is passed as it is (cv::Mat::step)"""
        depth = np.asarray(depth, np.float32)
        if depth.ndim != 2 or depth.strides[1] != 4 or depth.strides[0] % 4 or depth.strides[0] < depth.shape[1] * 4:
            depth = np.ascontiguousarray(depth)
        return depth, depth.strides[0] // 4

    def ConvertDepthToPointCloud(self, depth, downSample, fx, fy, cx, cy):
        depth = np.asarray(depth, np.float32)
        if depth.size == 0:
            return np.zeros((0, 4), np.float32)
        rows, cols = depth.shape
        stride = depth.strides[0] // 4
        out = np.zeros((rows * cols, 4), np.float32)
        n = C.c_int()
        _check(lib().gfs_depth_to_cloud(self.h, C.c_void_p(depth.ctypes.data), rows, cols, stride, downSample, fx, fy, cx, cy,
                                        _p(out), len(out), C.byref(n)), "gfs_depth_to_cloud")
        return out[:n.value].copy()

    def ComputeStereoFromRGBD(self, kps, depth, bf, kps_un_x=None):
        depth, stride = self._rows_view(depth)
        kps = np.ascontiguousarray(kps)
        n = len(kps)
        ur = np.zeros(max(n, 1), np.float32)
        vd = np.zeros(max(n, 1), np.float32)
        unx = np.ascontiguousarray(kps_un_x, np.float32) if kps_un_x is not None else None
        _check(lib().gfs_stereo_from_rgbd(self.h, _p(kps), _p(unx), n, C.c_void_p(depth.ctypes.data), depth.shape[0], depth.shape[1],
                                          stride, bf, _p(ur), _p(vd)), "gfs_stereo_from_rgbd")
        return ur[:n], vd[:n]

    def FrameRGBD(self, kps, depth, bf, downSample, fx, fy, cx, cy, kps_un_x=None, host_cloud=True, shape=None):
        """The RGB-D tail of the Frame constructor (ComputeStereoFromRGBD + ConvertDepthToPointCloud, src/Frame.cc:1314-1332,
        590-623) in one call: gfs_frame_rgbd.  Returns (mvuRight, mvDepth, cloud or None, (dev_cloud, dev_count, stride, n)).
        depth=None (with shape=(rows, cols)): the depth map of the previous call, still on the device; downSample=0: no cloud."""
        if depth is not None:
            depth, row_stride = self._rows_view(depth)
            rows, cols = depth.shape
        else:
            (rows, cols), row_stride = shape, shape[1]
        kps = np.ascontiguousarray(kps)
        n = len(kps)
        ur = np.empty(max(n, 1), np.float32)
        vd = np.empty(max(n, 1), np.float32)
        unx = np.ascontiguousarray(kps_un_x, np.float32) if kps_un_x is not None else None
        want_cloud = host_cloud and downSample > 0
        out = np.empty((rows * cols // (downSample * downSample) + rows + cols, 4), np.float32) if want_cloud else None
        nc, stride = C.c_int(), C.c_int()
        dc, dn = C.c_void_p(), C.c_void_p()
        _check(lib().gfs_frame_rgbd(self.h, _p(kps), _p(unx), n, C.c_void_p(depth.ctypes.data) if depth is not None else None, rows, cols,
                                    row_stride, bf, downSample, fx, fy, cx, cy, _p(ur),
                                    _p(vd), _p(out), len(out) if out is not None else 0, C.byref(nc), C.byref(dc), C.byref(dn),
                                    C.byref(stride)), "gfs_frame_rgbd")
        return ur[:n], vd[:n], (out[:nc.value] if out is not None else None), (dc.value, dn.value, stride.value, nc.value)

    def depth_convert_u16_batch_device(self, d_u16, B, rows, cols, factor, d_f32, stream=None):
        """imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) for CV_16U depth maps already in HBM (src/Tracking.cc:1622-1623)"""
        _check(lib().gfs_depth_convert_u16_batch_device(self.h, C.c_void_p(d_u16), B, rows, cols, float(factor), C.c_void_p(d_f32),
                                                        C.c_void_p(stream) if stream else None), "gfs_depth_convert_u16_batch_device")

    def depth_to_cloud_batch_device(self, d_depth, B, rows, cols, ds, fx, fy, cx, cy, d_out, stride_pts, d_counts, stream=None):
        _check(lib().gfs_depth_to_cloud_batch_device(self.h, C.c_void_p(d_depth), B, rows, cols, ds, fx, fy, cx, cy,
                                                     C.c_void_p(d_out), stride_pts, C.c_void_p(d_counts),
                                                     C.c_void_p(stream) if stream else None), "gfs_depth_to_cloud_batch_device")

    def stereo_from_rgbd_batch_device(self, d_kps, d_kps_un_x, d_counts, B, kp_stride, d_depth, rows, cols, bf, d_u_right, d_depth_out,
                                      stream=None):
        """ComputeStereoFromRGBD for B frames in HBM: key-points [B, kp_stride] (counts[b] valid), depth maps [B, rows, cols];
        d_kps_un_x None / 0: the undistorted x is the key-point's own"""
        _check(lib().gfs_stereo_from_rgbd_batch_device(self.h, C.c_void_p(d_kps), C.c_void_p(d_kps_un_x) if d_kps_un_x else None,
                                                       C.c_void_p(d_counts), B, kp_stride, C.c_void_p(d_depth), rows, cols, float(bf),
                                                       C.c_void_p(d_u_right), C.c_void_p(d_depth_out),
                                                       C.c_void_p(stream) if stream else None), "gfs_stereo_from_rgbd_batch_device")
