"""GPU tests of LocalVisualLidarBA (Optimizer::LocalVisualLidarBA, reference src/Optimizer.cc:1101-1587): the edges bit for bit
against the sequential CPU restatement (tests/host/lba_lidar_restatement.cpp), the normal equations within 1e-10 relative, the solve
within test_gpu_lba.py's bars, the no-edge window bit for bit gfs_lba_solve, determinism, the stop flag, a shared LidarMap, the
refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import lba_lidar_support as LLS
from geoflowslam_amd import synth

pytestmark = pytest.mark.gpu

BENCH = dict(seed=0, n_free=20, n_fixed=5, n_points=3000, n_cloud=3000, voxel=0.08)


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


@functools.lru_cache(maxsize=None)
def _window(**kw):
    return synth.lba_lidar_window(width=120, height=90, **kw)


def _win(cfg):
    return _window(**{k: tuple(v) if isinstance(v, list) else v for k, v in cfg.items()})


def _map(gpu_api, w):
    return gpu_api.LidarMap(max_points=len(w["map_xyz"])).set(w["map_xyz"])


SMALL = [dict(seed=s, n_free=4, n_fixed=1, n_points=120, n_cloud=400, voxel=0.1, init_fixed=bool(s % 3 == 0),
              lidar=[0, 1, 2, 3] if s % 2 else None) for s in range(20)]


def test_fetch_lidar_edges_bit_exact(gpu_api):
    opt = gpu_api.Optimizer(max_poses=16, max_points=1024, max_edges=16384)
    total = 0
    for cfg in SMALL:
        w = _win(cfg)
        m = _map(gpu_api, w)
        r = opt.linearize_lidar(w, m)
        ref = LLS.linearize(w)
        assert (r["pose_lidar_edges"] == ref["pose_lidar_edges"]).all(), cfg
        for i in range(w["n_poses"]):
            idx, pl, s = opt.fetch_lidar_edges(i)
            ri, rp, rs = ref["edges"][i]
            assert (idx == ri).all() and (pl.view(np.uint32) == rp.view(np.uint32)).all() and (s.view(np.uint32) == rs.view(np.uint32)).all(), \
                (cfg, i)
            total += len(idx)
    assert total > 1000


def test_linearize_lidar_matches_restatement(gpu_api):
    w = _win(BENCH)
    m = _map(gpu_api, w)
    opt = gpu_api.Optimizer(max_poses=32, max_points=4096, max_edges=200000)
    L = opt.linearize_lidar(w, m)
    Lr = LLS.linearize(w)
    assert int(L["pose_lidar_edges"].sum()) > 2000
    for k in ("Hpp", "Hll", "Hpl", "bp", "bl", "edge_chi2"):
        assert _rel(L[k], Lr[k]) < 1e-10, (k, _rel(L[k], Lr[k]))
    assert (L["lidar_edge_chi2"] == Lr["lidar_edge_chi2"]).all()
    assert abs(L["chi2"] - Lr["chi2"]) <= 1e-9 * Lr["chi2"]
    # the lidar terms are really in there: Hpp differs from the plain linearisation for the lidar key-frames only
    L0 = opt.linearize(w)
    free = np.flatnonzero(w["pose_fixed"] == 0)
    for f, pose in enumerate(free):
        same = (L["Hpp"][f] == L0["Hpp"][f]).all()
        assert same == (L["pose_lidar_edges"][pose] == 0), pose


SOLVE = [BENCH,
         dict(seed=1, n_free=4, n_fixed=2, n_points=200, n_cloud=600, voxel=0.1),
         dict(seed=7, n_free=80, n_fixed=4, n_points=800, n_cloud=400, voxel=0.1),
         dict(seed=2, n_free=8, n_fixed=2, n_points=400, n_cloud=800, voxel=0.1, init_fixed=True, lidar=[0, 1, 3, 5]),
         dict(seed=3, n_free=8, n_fixed=2, n_points=400, n_cloud=800, voxel=0.1, lidar=[]),
         dict(seed=4, n_free=8, n_fixed=2, n_points=400, n_cloud=800, voxel=0.1, lidar=[1, 2, 3, 5, 6], short_cloud=(1, 3),
              empty_cloud=(5,)),
         dict(seed=5, n_free=8, n_fixed=2, n_points=400, n_cloud=800, voxel=0.1, map_shift=(100.0, 0.0, 0.0)),
         dict(seed=6, n_free=31, n_fixed=2, n_points=500, n_cloud=400, voxel=0.1),
         dict(seed=8, n_free=3, n_fixed=1, n_points=80, n_cloud=500, voxel=0.1, mono_frac=1.0, lidar=[0, 1, 2])]


@pytest.mark.parametrize("cfg", SOLVE, ids=[f"s{c['seed']}_{c['n_free']}" for c in SOLVE])
def test_solve_matches_restatement(gpu_api, cfg):
    w = _win(cfg)
    m = _map(gpu_api, w)
    opt = gpu_api.Optimizer(max_poses=96, max_points=4096, max_edges=200000)
    r = opt.LocalVisualLidarBA(w, m)
    ro, _ = LLS.solve(w)
    assert (r["pose_lidar_edges"] == ro["pose_lidar_edges"]).all()
    assert r["iterations_run"] == ro["iterations_run"]
    for i in range(w["n_poses"]):
        assert _rel(r["pose_q"][i], ro["pose_q"][i]) < 1e-5 and _rel(r["pose_t"][i], ro["pose_t"][i]) < 1e-5, i
    # Over ALL points the restatement's own answer is not defined to 1e-5: on the s4 window, observations perturbed by 1e-15 relative
    # (a few ulps) move its points by 1.6e-5 .. 2.7e-5 relative, and the points seen by two or more edges by ~1e-7 (poses ~2e-7).  The
    # numeric Jacobian (delta 1e-9) turns last-bit pose differences into ~1e-7 relative changes of the lidar blocks, and a point seen
    # by one key-frame has no depth constraint beyond lambda.  The GPU measured 1.7e-5 there.
    seen = np.bincount(w["edge_point"], minlength=w["n_points"]) >= 2
    assert _rel(r["points"][seen], ro["points"][seen]) < 1e-5
    assert _rel(r["points"], ro["points"]) < 1e-4
    assert abs(r["final_chi2"] - ro["final_chi2"]) <= 1e-6 * ro["final_chi2"]
    th = np.where(w["edge_stereo"] == 1, 7.815, 5.991)
    away = np.abs(ro["edge_chi2"] - th) > 1e-3 * th
    assert ((r["edge_chi2"] > th) == (ro["edge_chi2"] > th))[away].all()
    assert (r["edge_depth_positive"] == ro["edge_depth_positive"]).all()


@pytest.mark.parametrize("cfg", [SOLVE[4], SOLVE[6]], ids=["above75", "no_edges"])
def test_no_lidar_edges_is_lba_bit_for_bit(gpu_api, cfg):
    w = _win(cfg)
    m = _map(gpu_api, w)
    opt = gpu_api.Optimizer(max_poses=32, max_points=4096, max_edges=200000)
    r = opt.LocalVisualLidarBA(w, m)
    r0 = opt.LocalBundleAdjustment(w)
    assert r["pose_lidar_edges"].sum() == 0
    for k in ("pose_q", "pose_t", "points", "edge_chi2", "edge_depth_positive"):
        assert np.array_equal(r[k].view(np.uint8), r0[k].view(np.uint8)), k
    assert (r["iterations_run"], r["final_chi2"], r["final_lambda"]) == (r0["iterations_run"], r0["final_chi2"], r0["final_lambda"])


def test_deterministic_and_lidar_changes_the_answer(gpu_api):
    w = _win(BENCH)
    m = _map(gpu_api, w)
    opt = gpu_api.Optimizer(max_poses=32, max_points=4096, max_edges=200000)
    a, b = opt.LocalVisualLidarBA(w, m), opt.LocalVisualLidarBA(w, m)
    for k in ("pose_q", "pose_t", "points", "edge_chi2"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert a["final_chi2"] == b["final_chi2"]
    r0 = opt.LocalBundleAdjustment(w)
    assert not np.array_equal(a["pose_t"], r0["pose_t"])


def test_stop_flag_before_the_call_writes_nothing(gpu_api):
    api = gpu_api
    w = _win(SOLVE[1])
    m = _map(api, w)
    opt = api.Optimizer(max_poses=16, max_points=1024, max_edges=16384)
    assert opt.LocalVisualLidarBA(w, m, stop_flag=np.ones(1, np.int32)) is None
    P, keep = api._lba_problem(w)
    L, lkeep = opt._lidar(w, m)
    q = np.full((P.n_poses, 4), 7.0)
    S = api.LbaSolution()
    S.pose_q, S.iterations_run = q.ctypes.data, -3
    ple = np.full(P.n_poses, -9, np.int32)
    stop = np.ones(1, np.int32)
    rc = api.lib().gfs_lba_solve_lidar(opt.h, C.byref(P), C.byref(L), C.byref(S), ple.ctypes.data, stop.ctypes.data)
    assert rc == -6 and (q == 7.0).all() and S.iterations_run == -3 and (ple == -9).all()
    flag = np.ones(1, np.uint8)
    rc = api.lib().gfs_lba_solve_lidar_bool(opt.h, C.byref(P), C.byref(L), C.byref(S), ple.ctypes.data, flag.ctypes.data)
    assert rc == -6 and (q == 7.0).all()


def test_shared_lidar_map(gpu_api):
    api = gpu_api
    w = _win(SOLVE[1])
    f = synth.pose_lidar_frame(3, n_obs=200, n_cloud=800, width=160, height=120)
    shared = api.LidarMap(max_points=max(len(w["map_xyz"]), len(f["map_xyz"])))
    po = api.PoseLidarOptimizer(max_obs=512, max_cloud=1024, max_batch=1)
    opt = api.Optimizer(max_poses=16, max_points=1024, max_edges=16384)
    fresh_pose = po.PoseLidarVisualOptimization(dict(f, map=api.LidarMap(max_points=len(f["map_xyz"])).set(f["map_xyz"])))
    fresh_lba = opt.LocalVisualLidarBA(w, _map(api, w))
    for _ in range(2):
        shared.set(f["map_xyz"])
        rp = po.PoseLidarVisualOptimization(dict(f, map=shared))
        shared.set(w["map_xyz"])
        rl = opt.LocalVisualLidarBA(w, shared)
        assert np.array_equal(rp["q"], fresh_pose["q"]) and np.array_equal(rp["t"], fresh_pose["t"])
        for k in ("pose_q", "pose_t", "points"):
            assert np.array_equal(rl[k], fresh_lba[k]), k


def test_refusals(gpu_api):
    api = gpu_api
    w = _win(SOLVE[1])
    opt = api.Optimizer(max_poses=16, max_points=1024, max_edges=16384)
    with pytest.raises(api.GfsError):
        opt.LocalVisualLidarBA(w, api.LidarMap(max_points=1000))  # never set
    m = _map(api, w)
    with pytest.raises(api.GfsError):
        opt.LocalVisualLidarBA(dict(w, two_camera=1), m)
    P, keep = api._lba_problem(w)
    L, lkeep = api.lba_lidar_struct(w, m.h)
    out = dict(pose_q=np.zeros((P.n_poses, 4)), pose_t=np.zeros((P.n_poses, 3)), points=np.zeros((P.n_points, 3)))
    S = api.LbaSolution()
    for k, v in out.items():
        setattr(S, k, v.ctypes.data)
    assert api.lib().gfs_lba_lidar_reserve(opt.h, 100) == 0
    rc = api.lib().gfs_lba_solve_lidar(opt.h, C.byref(P), C.byref(L), C.byref(S), None, None)
    assert rc == -4  # GFS_ERR_CAPACITY: the clouds are not truncated
    assert (out["pose_q"] == 0).all()
    if api.device_count() > 1:  # a map on another device
        m1 = api.LidarMap(max_points=len(w["map_xyz"]), device=1).set(w["map_xyz"])
        L1, k1 = api.lba_lidar_struct(w, m1.h)
        assert api.lib().gfs_lba_lidar_reserve(opt.h, 1 << 16) == 0
        assert api.lib().gfs_lba_solve_lidar(opt.h, C.byref(P), C.byref(L1), C.byref(S), None, None) == -1
