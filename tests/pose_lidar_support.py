"""Shared by the PoseLidarVisualOptimization tests: builds and calls the sequential CPU restatement
(tests/host/pose_lidar_restatement.cpp), and makes random frames.  Not a test module."""
import ctypes as C
import os
import subprocess

import numpy as np

from geoflowslam_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "pose_lidar_restatement.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_pose_lidar_restatement.so")
_L = None


def restatement():
    global _L
    if _L is None:
        deps = [_SRC, os.path.join(ROOT, "oracle", "g2o_se3.hpp"), os.path.join(ROOT, "include", "gfs_abi.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "oracle"),
                            "-I" + os.path.join(ROOT, "include"), "-o", _SO, _SRC], check=True)
        L = C.CDLL(_SO)
        vp = C.c_void_p
        L.plr_pose_lidar.argtypes = [C.POINTER(api.PoseLidarProblem), vp, C.c_int, C.POINTER(api.PoseLidarSolution), vp, vp, vp]
        L.plr_pose_lidar.restype = C.c_int
        L.plr_qr_plane.argtypes = [vp, vp]
        L.plr_knn5.argtypes = [vp, C.c_int, vp, vp, vp]
        L.plr_point_edge.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp]
        L.plr_point_edge.restype = C.c_int
        L.plr_constants.argtypes = [vp]
        _L = L
    return _L


def run(prob):
    """The restatement on one frame dict (see api.pose_lidar_structs; the map is prob["map_xyz"]) -> (rc, result, edges), edges =
    per round (index, plane, s)."""
    L = restatement()
    P, S, keep, n = api.pose_lidar_structs(prob, None)
    mp = np.ascontiguousarray(prob["map_xyz"], np.float32).reshape(-1, 3)
    nc = max(int(P.n_cloud), 1)
    idx, pl, s = np.zeros((4, nc), np.int32), np.zeros((4, nc, 4), np.float32), np.zeros((4, nc), np.float32)
    rc = L.plr_pose_lidar(C.byref(P), mp.ctypes.data, len(mp), C.byref(S), idx.ctypes.data, pl.ctypes.data, s.ctypes.data)
    res = api.pose_lidar_result(S, keep, n)
    edges = [(idx[r, :res["round_edges"][r]].copy(), pl[r, :res["round_edges"][r]].copy(), s[r, :res["round_edges"][r]].copy())
             for r in range(4)]
    return rc, res, edges


def qr_plane(pts5):
    x = np.zeros(3, np.float32)
    restatement().plr_qr_plane(np.ascontiguousarray(pts5, np.float32).ctypes.data, x.ctypes.data)
    return x


def point_edge(mp, po, q=(0, 0, 0, 1), t=(0, 0, 0)):
    """The edge generator on one frame point -> (kept, plane, s, diag); diag = (largest |n.p + d| of the neighbours, weight s) as
    the floats the gates compare, NaN when the 5-NN gate already failed."""
    mp = np.ascontiguousarray(mp, np.float32).reshape(-1, 3)
    q, t, po = (np.ascontiguousarray(v, np.float32) for v in (q, t, po))
    plane, s, diag = np.zeros(4, np.float32), np.zeros(1, np.float32), np.full(2, np.nan, np.float32)
    keep = restatement().plr_point_edge(mp.ctypes.data, len(mp), q.ctypes.data, t.ctypes.data, po.ctypes.data, plane.ctypes.data,
                                        s.ctypes.data, diag.ctypes.data)
    return keep, plane, s[0], diag


def gate_literal_cases():
    """Two frame points built so that a gate compares a float that equals its literal rounded to float: the largest plane
    residual is exactly 0.2f (> 0.2 as a double: the plane is rejected; a float comparison would keep it), and the weight is
    exactly 0.1f (> 0.1 as a double: the edge is kept; a float comparison would drop it).  -> [(map [5][3], point [3], kept)]"""
    cases = []
    # plane gate: four points on z = 0.1, a fifth lifted by h; bisect h to the residual 0.2f, then walk over neighbouring floats.
    # (The residual is a float sum ending in "+ pd": the plane and the points sit within 0.25 of the origin so that every operand is
    # on the grid of 0.2f -- with pd near 1 the sum could only take multiples of 2^-23 and never equal 0.2f.)
    base = np.array([[-0.1, -0.1, 0.1], [0.1, -0.1, 0.1], [-0.1, 0.1, 0.1], [0.1, 0.1, 0.1]], np.float32)
    p = np.array([0.0, 0.0, 0.1], np.float32)
    found = None
    for dx in np.linspace(0.0, 0.1, 101, dtype=np.float32):  # the fifth point's x: another residual-vs-lift curve each time
        top = lambda h: np.concatenate([base, [[dx, 0.0, 0.1 + h]]]).astype(np.float32)
        lo, hi = np.float32(0.05), np.float32(0.9)
        for _ in range(60):
            h = np.float32((lo + hi) / 2)
            if point_edge(top(h), p)[3][0] > np.float32(0.2):
                hi = h
            else:
                lo = h
        h = np.nextafter(lo, np.float32(0.0))
        for _ in range(8):
            if point_edge(top(h), p)[3][0] == np.float32(0.2):
                found = (top(h), p, 0)
                break
            h = np.nextafter(h, np.float32(2.0))
        if found:
            break
    if found:
        cases.append(found)
    # weight gate: neighbours on z = -0.05 near the axis, the point above them at the height where s = 1 - 0.9 |pd2| / |p|^(1/2)
    # reaches 0.1; scan the point's z over neighbouring floats (and its x, which moves |p| by a little) until s == 0.1f
    nb = np.array([[0, 0, -0.05], [0.1, 0, -0.05], [0, 0.1, -0.05], [-0.1, 0, -0.05], [0, -0.1, -0.05]], np.float32)
    found = None
    for x in np.linspace(0.0, 0.02, 81, dtype=np.float32):
        z = np.float32(0.897)
        lo, hi = np.float32(0.85), np.float32(0.95)
        for _ in range(60):
            z = np.float32((lo + hi) / 2)
            _, _, _, d = point_edge(nb, np.array([x, 0, z], np.float32))
            if d[1] > np.float32(0.1):
                lo = z
            else:
                hi = z
        for zz in (lo, hi):
            for k in range(-20, 21):
                zk = zz
                for _ in range(abs(k)):
                    zk = np.nextafter(zk, np.float32(2.0 if k > 0 else 0.0))
                po = np.array([x, 0, zk], np.float32)
                _, _, _, d = point_edge(nb, po)
                if d[1] == np.float32(0.1):
                    found = (nb.copy(), po, 1)
                    break
            if found:
                break
        if found:
            break
    if found:
        cases.append(found)
    return cases


def random_frame(seed, n_obs=None, n_cloud=None, n_map=None, n_iterations=None):
    """A random frame of the fuzz: planes-and-boxes scene, mono / stereo / mixed, gross outliers, cloud and map sizes drawn
    from wide ranges (small sizes more often, so that the brute-force restatement stays quick)."""
    rng = np.random.default_rng(seed)
    if n_obs is None:
        n_obs = int(rng.choice([0, 2, 5, 9, 40, 150, 400, 1500], p=[.03, .04, .05, .05, .28, .3, .2, .05]))
    if n_cloud is None:
        n_cloud = int(rng.choice([0, 30, 60, 300, 1000, 3000, 6000], p=[.03, .05, .1, .4, .27, .1, .05]))
    if n_map is None:
        n_map = int(rng.choice([5, 40, 600, 3000, 12000, 40000], p=[.03, .07, .35, .35, .15, .05]))
    if n_iterations is None:
        n_iterations = int(rng.integers(1, 5))
    mono = rng.random()
    mono_frac = 0.0 if mono < 0.3 else (1.0 if mono < 0.45 else 0.2)
    f = synth.pose_lidar_frame(int(seed) % 997, n_obs=max(n_obs, 1), n_cloud=max(n_cloud, 1), width=160, height=120,
                               mono_frac=mono_frac, outlier_frac=float(rng.uniform(0, 0.3)), n_iterations=n_iterations,
                               rot_deg=float(rng.uniform(0.2, 3.0)), trans=float(rng.uniform(0.005, 0.1)), n_keyframes=2)
    for k in ("xw", "obs", "inv_sigma2", "stereo"):
        f[k] = f[k][:n_obs]
    f["cloud"] = f["cloud"][:n_cloud]
    mp = f["map_xyz"]
    if n_map <= len(mp):
        mp = mp[np.sort(rng.choice(len(mp), n_map, replace=False))]
    else:  # denser: jittered copies
        extra = mp[rng.integers(0, len(mp), n_map - len(mp))] + rng.normal(0, 0.03, (n_map - len(mp), 3))
        mp = np.concatenate([mp, extra])
    f["map_xyz"] = np.ascontiguousarray(rng.permutation(mp), np.float32)
    f["n_lidar_inliers"] = int(rng.integers(-5, 5))
    f["residual"] = float(np.float32(rng.uniform(-1, 1)))
    return f
