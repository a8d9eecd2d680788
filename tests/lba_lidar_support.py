"""Shared by the LocalVisualLidarBA tests: builds and calls the sequential CPU restatement (tests/host/lba_lidar_restatement.cpp,
which includes oracle/lba_oracle.cpp and tests/host/pose_lidar_restatement.cpp), and makes windows.  Not a test module."""
import ctypes as C
import os
import subprocess

import numpy as np

from geoflowslam_amd import api, synth
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "lba_lidar_restatement.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_lba_lidar_restatement.so")
_L = None


def restatement():
    global _L
    if _L is None:
        deps = [_SRC, os.path.join(ROOT, "tests", "host", "pose_lidar_restatement.cpp"), os.path.join(ROOT, "oracle", "lba_oracle.cpp"),
                os.path.join(ROOT, "oracle", "g2o_se3.hpp"), os.path.join(ROOT, "oracle", "gfs_oracle.h"),
                os.path.join(ROOT, "include", "gfs_abi.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            tmp = _SO + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "oracle"),
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "host"), "-o", tmp, _SRC],
                           check=True)
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        vp = C.c_void_p
        L.lblr_linearize.argtypes = [C.POINTER(O.LbaProblem), vp, vp, C.c_int] + [vp] * 11
        L.lblr_linearize.restype = C.c_double
        L.lblr_solve.argtypes = [C.POINTER(O.LbaProblem), vp, vp, C.c_int, C.POINTER(O.LbaSolution), vp, vp, vp, vp]
        L.lblr_solve.restype = C.c_int
        L.lblr_solve_scripted.argtypes = L.lblr_solve.argtypes + [C.c_int, C.POINTER(C.c_int32)]
        L.lblr_solve_scripted.restype = C.c_int
        L.lblr_constants.argtypes = [vp]
        _L = L
    return _L


def _lidar(prob):
    if "cloud" not in prob:
        return None, None
    Lr, keep = api.lba_lidar_struct(prob, None)
    return Lr, keep


def _edges(prob, pe, idx, pl, s):
    out, at = {}, 0
    for i in range(int(prob["n_poses"])):
        n = int(pe[i])
        out[i] = (idx[at:at + n].copy(), pl[at:at + n].copy(), s[at:at + n].copy())
        at += n
    return out


def _bufs(prob):
    n = max(int(np.asarray(prob["cloud_begin"])[-1]) if "cloud" in prob else 0, 1)
    return (np.zeros(max(int(prob["n_poses"]), 1), np.int32), np.zeros(n, np.int32), np.zeros((n, 4), np.float32), np.zeros(n, np.float32))


def solve(prob, lidar=True, stop_at_look=-1):
    """The restatement's optimize(10) -> (LocalBundleAdjustment's dict + pose_lidar_edges, edges {pose: (index, plane, s)}).
    stop_at_look >= 0: with the stop flag raised from its stop_at_look-th evaluation on (oracle.lba_solve_scripted's script); the dict
    then has `looks`, and is None when the entry check stopped the call."""
    L = restatement()
    P, keep = O._lba_struct(O.LbaProblem, prob)
    Lr, lkeep = _lidar(prob) if lidar else (None, None)
    mp = np.ascontiguousarray(prob.get("map_xyz", np.zeros((5, 3))), np.float32).reshape(-1, 3)
    out = dict(pose_q=np.zeros((P.n_poses, 4)), pose_t=np.zeros((P.n_poses, 3)), points=np.zeros((P.n_points, 3)),
               edge_chi2=np.zeros(P.n_edges), edge_depth_positive=np.zeros(P.n_edges, np.uint8))
    S = O.LbaSolution()
    for k, v in out.items():
        setattr(S, k, v.ctypes.data)
    pe, idx, pl, s = _bufs(prob)
    looks = C.c_int32()
    rc = L.lblr_solve_scripted(C.byref(P), C.byref(Lr) if Lr is not None else None, mp.ctypes.data, len(mp), C.byref(S), pe.ctypes.data,
                               idx.ctypes.data, pl.ctypes.data, s.ctypes.data, int(stop_at_look), C.byref(looks))
    if rc < 0:
        return None, {}
    out["looks"] = looks.value
    out.update(iterations_run=S.iterations_run, final_chi2=S.final_chi2, final_lambda=S.final_lambda, pose_lidar_edges=pe[:P.n_poses].copy())
    return out, _edges(prob, pe, idx, pl, s)


def linearize(prob, lidar=True):
    """One buildSystem at the initial estimates -> oracle.lba_linearize's dict + lidar_edge_chi2, pose_lidar_edges, edges."""
    L = restatement()
    P, keep = O._lba_struct(O.LbaProblem, prob)
    Lr, lkeep = _lidar(prob) if lidar else (None, None)
    mp = np.ascontiguousarray(prob.get("map_xyz", np.zeros((5, 3))), np.float32).reshape(-1, 3)
    nf = int((np.asarray(prob["pose_fixed"]) == 0).sum())
    Hpp = np.zeros((nf, 36)); Hll = np.zeros((P.n_points, 9)); Hpl = np.zeros((P.n_edges, 18))
    bp = np.zeros((nf, 6)); bl = np.zeros((P.n_points, 3)); chi = np.zeros(P.n_edges)
    pe, idx, pl, s = _bufs(prob)
    lchi = np.zeros(len(idx))
    tot = L.lblr_linearize(C.byref(P), C.byref(Lr) if Lr is not None else None, mp.ctypes.data, len(mp), Hpp.ctypes.data,
                           Hll.ctypes.data, Hpl.ctypes.data, bp.ctypes.data, bl.ctypes.data, chi.ctypes.data, lchi.ctypes.data,
                           pe.ctypes.data, idx.ctypes.data, pl.ctypes.data, s.ctypes.data)
    ne = int(pe[:P.n_poses].sum())
    return dict(Hpp=Hpp.reshape(nf, 6, 6).transpose(0, 2, 1).copy(), Hll=Hll.reshape(-1, 3, 3).transpose(0, 2, 1).copy(),
                Hpl=Hpl.reshape(-1, 3, 6).transpose(0, 2, 1).copy(), bp=bp, bl=bl, edge_chi2=chi, chi2=float(tot),
                lidar_edge_chi2=lchi[:ne].copy(), pose_lidar_edges=pe[:P.n_poses].copy(), edges=_edges(prob, pe, idx, pl, s))


def constants():
    out = np.zeros(5)
    restatement().lblr_constants(out.ctypes.data)
    return out


def window(seed, **kw):
    """A small window for the CPU tests (the brute-force 5-NN of the restatement is O(cloud x map))."""
    kw.setdefault("n_free", 5)
    kw.setdefault("n_fixed", 2)
    kw.setdefault("n_points", 300)
    kw.setdefault("n_cloud", 300)
    kw.setdefault("voxel", 0.1)
    return synth.lba_lidar_window(seed, **kw)
