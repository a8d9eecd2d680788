"""Shared by the lidar local-map tests: builds and calls the sequential CPU restatement (tests/host/lidar_map_restatement.cpp), and
makes windows and constructed clouds.  Not a test module."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from geoflowslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "lidar_map_restatement.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_lidar_map_restatement.so")
_L = None

OK, INVALID_ARG, CAPACITY, UNSUPPORTED = 0, -1, -4, -5
LEAVES = (0.02, 0.04, 0.1, 0.2)
PASSTHROUGH_LEAF = 0.001  # a few metres of extent at 1 mm: more than INT32_MAX cells


def restatement():
    global _L
    if _L is None:
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < os.path.getmtime(_SRC):
            tmp = _SO + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, _SRC], check=True)
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        vp, i, f = C.c_void_p, C.c_int, C.c_float
        L.lmr_pose_matrix.argtypes = [vp, vp, vp]
        L.lmr_transform.argtypes = [i, vp, vp, vp, vp, vp]
        L.lmr_voxel_filter.argtypes = [vp, i, f, vp, i, vp]
        L.lmr_build.argtypes = [i, vp, vp, vp, vp, f, vp, i, vp]
        _L = L
    return _L


def _info(a):
    return dict(n_in=int(a[0]), n_out=int(a[1]), passthrough=int(a[2]), div=tuple(int(v) for v in a[3:6]))


def _inputs(w):
    q = np.ascontiguousarray(w["q"], np.float32).reshape(-1, 4)
    t = np.ascontiguousarray(w["t"], np.float32).reshape(-1, 3)
    cb = np.ascontiguousarray(w["cloud_begin"], np.int32)
    cloud = np.ascontiguousarray(w["cloud"], np.float32).reshape(-1, 3)
    return q, t, cb, cloud


def transform(w):
    """The restatement's transformPointCloud over a window (synth.lidar_map_window's dict) -> world points [n][3]."""
    q, t, cb, cloud = _inputs(w)
    out = np.zeros((max(len(cloud), 1), 3), np.float32)
    restatement().lmr_transform(len(q), q.ctypes.data, t.ctypes.data, cb.ctypes.data, cloud.ctypes.data, out.ctypes.data)
    return out[:len(cloud)]


def voxel_filter(xyz, leaf, cap=None):
    """The restatement's filter -> (rc, points [n_out][3], info)."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    cap = len(xyz) if cap is None else cap
    out, info = np.zeros((max(cap, 1), 3), np.float32), np.zeros(6, np.int32)
    rc = restatement().lmr_voxel_filter(xyz.ctypes.data, len(xyz), float(np.float32(leaf)), out.ctypes.data, cap, info.ctypes.data)
    I = _info(info)
    return rc, (out[:I["n_out"]].copy() if rc == 0 else None), I


def build(w, leaf, cap=None):
    """The restatement's whole build of a window -> (rc, map points [n_out][3] in map-index order, info)."""
    q, t, cb, cloud = _inputs(w)
    cap = len(cloud) if cap is None else cap
    out, info = np.zeros((max(cap, 1), 3), np.float32), np.zeros(6, np.int32)
    rc = restatement().lmr_build(len(q), q.ctypes.data, t.ctypes.data, cb.ctypes.data, cloud.ctypes.data, float(np.float32(leaf)),
                                 out.ctypes.data, cap, info.ctypes.data)
    I = _info(info)
    return rc, (out[:I["n_out"]].copy() if rc == 0 else None), I


@functools.lru_cache(maxsize=None)
def window(seed, n_keyframes=7, n_cloud=600, empty=(), scaled=False, width=80, height=60):
    """A seeded window; scaled: the stored quaternions are off unit length by up to 1e-3."""
    qs = None
    if scaled:
        qs = 1.0 + np.random.default_rng(seed + 5).uniform(-1e-3, 1e-3, n_keyframes)
    return synth.lidar_map_window(seed, n_keyframes=n_keyframes, n_cloud=n_cloud, empty=empty, quat_scale=qs, width=width, height=height)


# (seed, key-frames, leaf): 32 windows over 1 / 2 / 7 / 30 key-frames and the four leaves
WINDOWS = [(s, (1, 2, 7, 30)[s % 4], LEAVES[(s // 4) % 4]) for s in range(32)]


def overflow_pair():
    """Two points whose grid passes PCL's int64 check (d = 1290^3 <= INT32_MAX) but not its int arithmetic (div = 1291^3)."""
    return np.array([[0.9, 0.9, 0.9], [1290.1, 1290.1, 1290.1]], np.float32), 1.0


def constructed_clouds():
    """[(name, xyz, leaf)]: the filter's constructed cases (every one is filtered or passed through; the refusal is overflow_pair)."""
    rng = np.random.default_rng(99)
    out = []
    k = np.arange(-6, 7, dtype=np.float32)
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    g = g[rng.permutation(len(g))]
    out.append(("multiples_quarter", np.concatenate([g * np.float32(0.25), g * np.float32(0.125)]).astype(np.float32), 0.25))
    out.append(("multiples_tenth", np.concatenate([g * np.float32(0.1), g * np.float32(0.1) + np.float32(0.05)]).astype(np.float32), 0.1))
    out.append(("multiples_fifth", (g * np.float32(0.2)).astype(np.float32), 0.2))
    p = rng.uniform(-1, 1, (300, 3)).astype(np.float32)
    out.append(("duplicates", np.concatenate([p, p[::3], p[::-1], p[:50]]), 0.1))
    out.append(("one_voxel", (np.float32(0.31) + rng.uniform(0, 0.05, (700, 3))).astype(np.float32), 0.1))
    out.append(("one_point", np.array([[0.3, -1.7, 2.2]], np.float32), 0.1))
    out.append(("one_point_negative_zero", np.array([[-0.0, 0.0, -0.0]], np.float32), 0.1))
    out.append(("passthrough", rng.uniform(-2, 3, (500, 3)).astype(np.float32) * np.float32([1.0, 0.8, 0.5]), PASSTHROUGH_LEAF))
    out.append(("far_from_origin", (rng.uniform(-1, 1, (800, 3)) + [9.0e5, -9.0e5, 5.0e5]).astype(np.float32), 0.2))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


# ------------------------------------------------------------------ consumers' problems whose map comes from key-frame clouds

POSE_SEEDS = tuple(range(12))
POSE_LEAF = 0.1
LBA_CFG = dict(seed=3, n_free=4, n_fixed=1, n_points=120, n_cloud=1500, voxel=0.1, lidar=(0, 1, 2, 3), width=120, height=90)


@functools.lru_cache(maxsize=None)
def pose_problem(seed):
    """A PoseLidarVisualOptimization frame and the three key-frames (poses, clouds) of the same scene around it that its local map is
    built from -> (frame dict without a map, window)."""
    f = synth.pose_lidar_frame(seed, n_obs=300, n_cloud=1500, width=160, height=120)
    Rcw = synth._rot_from_quat(f["q_gt"])
    T = np.eye(4)
    T[:3, :3] = Rcw.T
    T[:3, 3] = -Rcw.T @ f["t_gt"]
    w = synth.lidar_map_window(seed, n_keyframes=3, n_cloud=3000, width=160, height=120, around=T, trans=0.12, rot_deg=3.0)
    f = dict(f)
    del f["map_xyz"]
    return f, w


@functools.lru_cache(maxsize=None)
def lba_problem():
    """A LocalVisualLidarBA window and the map input made of its own key-frames' clouds at their true poses."""
    cfg = dict(LBA_CFG)
    cfg["lidar"] = list(cfg["lidar"])
    w = synth.lba_lidar_window(**cfg)
    w = dict(w)
    del w["map_xyz"]
    mw = dict(q=np.asarray(w["gt_q"], np.float32), t=np.asarray(w["gt_t"], np.float32), cloud_begin=w["cloud_begin"], cloud=w["cloud"])
    cb = w["cloud_begin"]
    mw["clouds"] = [w["cloud"][cb[i]:cb[i + 1]] for i in range(len(cb) - 1)]
    return w, mw


def grid(api, lidar_map):
    """The map's search grid through the test hook -> dict(start [nb + 1], pts [n][3], index [n], nb, n)."""
    nb, n = C.c_int32(), C.c_int32()
    rc = api.lib().gfs_test_lidar_map_grid(lidar_map.h, None, 0, None, None, 0, C.byref(nb), C.byref(n))
    assert rc == 0, rc
    start, pts, index = np.zeros(nb.value + 1, np.int32), np.zeros((max(n.value, 1), 3), np.float32), np.zeros(max(n.value, 1), np.int32)
    rc = api.lib().gfs_test_lidar_map_grid(lidar_map.h, start.ctypes.data, len(start), pts.ctypes.data, index.ctypes.data, n.value,
                                           C.byref(nb), C.byref(n))
    assert rc == 0, rc
    return dict(start=start, pts=pts[:n.value], index=index[:n.value], nb=nb.value, n=n.value)


def same_grid(a, b):
    return (a["nb"] == b["nb"] and a["n"] == b["n"] and a["start"].tobytes() == b["start"].tobytes()
            and a["pts"].tobytes() == b["pts"].tobytes() and a["index"].tobytes() == b["index"].tobytes())
