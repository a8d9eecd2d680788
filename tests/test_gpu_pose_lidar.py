"""PoseLidarVisualOptimization on the MI355X (geoflowslam_amd/csrc/pose_lidar.hip) against the sequential CPU restatement
(tests/host/pose_lidar_restatement.cpp): bit for bit in the default edge order, toleranced in tree mode."""
import numpy as np
import pytest

import pose_lidar_support as PLS
from geoflowslam_amd import synth

pytestmark = pytest.mark.gpu

SCALARS = ("avg_reproj_error", "n_inliers", "n_lidar_inliers", "residual", "lidar_rounds", "rounds_run", "iterations_run",
           "round_edges", "round_valid")


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32) if a.dtype.kind == "f" else a


def _same(r, ro, where):
    for k in ("q", "t", "qf", "tf", "chi2", "round_chi2"):
        assert np.array_equal(_bits(r[k]), _bits(ro[k])), (where, k, r[k], ro[k])
    assert np.array_equal(r["outlier"], ro["outlier"]), (where, "outlier")
    for k in SCALARS:
        a, b = r[k], ro[k]
        if isinstance(a, np.floating):
            assert _bits(np.float32(a)) == _bits(np.float32(b)), (where, k, a, b)
        else:
            assert a == b, (where, k, a, b)


def _same_edges(opt, b, edges, where):
    for rnd in range(4):
        idx, pl, s = opt.fetch_edges(b, rnd, cap=8192)
        io, plo, so = edges[rnd]
        assert np.array_equal(idx, io), (where, rnd, len(idx), len(io))
        assert np.array_equal(_bits(pl), _bits(plo)) and np.array_equal(_bits(s), _bits(so)), (where, rnd)


def test_edge_order_bit_identical_to_restatement(gpu_api):
    opt = gpu_api.PoseLidarOptimizer(max_obs=1536, max_cloud=6144, max_batch=1)
    mp = gpu_api.LidarMap(max_points=40000)
    n_frames = 0
    for seed in range(500):
        f = PLS.random_frame(seed)
        rc, ro, edges = PLS.run(f)
        assert rc >= 0
        f["map"] = mp.set(f["map_xyz"])
        r = opt.PoseLidarVisualOptimization(f)
        _same(r, ro, seed)
        _same_edges(opt, 0, edges, seed)
        n_frames += 1
    assert n_frames == 500


def test_grid_borders_and_distance_ties(gpu_api):
    """Map points at float squared distance 1.0 and its neighbours (1 ulp either side) from queries sitting on the 1.25 m cell
    borders, and exact 5th / 6th distance ties (duplicated points): the edges of the device grid are those of the brute force."""
    rng = np.random.default_rng(5)
    opt = gpu_api.PoseLidarOptimizer(max_obs=64, max_cloud=512, max_batch=1)
    mp = gpu_api.LidarMap(max_points=8192)
    for trial in range(20):
        q = (np.round(rng.uniform(-4, 4, (80, 3)) / 1.25) * 1.25).astype(np.float32)  # on cell borders
        q += rng.choice([0.0, 1e-6, -1e-6], q.shape).astype(np.float32)
        pts = []
        for p in q:
            for _ in range(4):  # near-plane neighbours around the query, a few at squared distance ~1
                v = rng.normal(size=3)
                v[2] *= 0.05
                v /= np.linalg.norm(v)
                r = np.float32(rng.choice([0.3, 0.999, 1.0, 1.0001]))
                pts.append(p + r * v.astype(np.float32))
            for ax in range(3):  # axis-aligned at exactly 1.0 and one ulp either side
                e = np.zeros(3, np.float32)
                e[ax] = np.nextafter(np.float32(1.0), np.float32(rng.choice([0.0, 2.0]))) if rng.random() < 0.6 else 1.0
                pts.append(p + e)
        pts = np.array(pts, np.float32)
        dup = pts[rng.integers(0, len(pts), len(pts) // 3)]  # exact ties
        mpx = np.concatenate([pts, dup])
        mpx = mpx[rng.permutation(len(mpx))]
        f = dict(q=np.array([0, 0, 0, 1], np.float32), t=np.zeros(3, np.float32), xw=np.zeros((0, 3)), obs=np.zeros((0, 3)),
                 inv_sigma2=np.zeros(0, np.float32), stereo=np.zeros(0, np.uint8), fx=500.0, fy=500.0, cx=320.0, cy=240.0, bf=40.0,
                 cloud=q, map_xyz=mpx, n_iterations=1)
        f2 = dict(f, xw=np.tile([[0.0, 0.0, 3.0]], (5, 1)), obs=np.tile([[320.0, 240.0, 306.0]], (5, 1)),
                  inv_sigma2=np.ones(5, np.float32), stereo=np.ones(5, np.uint8))
        rc, ro, edges = PLS.run(f2)
        f2["map"] = mp.set(mpx)
        r = opt.PoseLidarVisualOptimization(f2)
        _same(r, ro, trial)
        _same_edges(opt, 0, edges, trial)


def test_batches_and_map_reuse(gpu_api):
    frames = [PLS.random_frame(1000 + s, n_map=int(np.random.default_rng(s).choice([600, 3000]))) for s in range(12)]
    opt = gpu_api.PoseLidarOptimizer(max_obs=1536, max_cloud=6144, max_batch=16)
    maps = [gpu_api.LidarMap(max_points=40000).set(frames[0]["map_xyz"]), gpu_api.LidarMap(max_points=40000).set(frames[1]["map_xyz"])]
    for i, f in enumerate(frames):  # two maps shared by the frames
        f["map_xyz"] = frames[i % 2]["map_xyz"]
        f["map"] = maps[i % 2]
    single = [opt.PoseLidarVisualOptimization(f) for f in frames]
    for lo, hi in ((0, 5), (5, 6), (6, 12)):  # ragged batches
        got = opt.PoseLidarVisualOptimization(frames[lo:hi])
        for k, (r, ro) in enumerate(zip(got, single[lo:hi])):
            _same(r, ro, (lo, k))
    for i in (0, 1):
        _, ro, _ = PLS.run(frames[i])
        _same(single[i], ro, ("restatement", i))
    fresh = gpu_api.LidarMap(max_points=40000).set(frames[0]["map_xyz"])  # reuse == re-upload
    f0 = dict(frames[0], map=fresh)
    _same(opt.PoseLidarVisualOptimization(f0), single[0], "re-upload")
    maps[0].set(frames[0]["map_xyz"])
    _same(opt.PoseLidarVisualOptimization(frames[0]), single[0], "set again")


def test_tree_mode_tolerance(gpu_api):
    """GFS_POSE_SUMS_TREE against the default edge order on 60 frames that all have observations and lidar edges.  Round 0's
    association and chi2Lidar / valid_edge do not depend on the sums: they must be bit-identical in every frame.  The pose is
    compared wherever both modes built the same edge sets in every round (a later round's association starts from the pose of the
    previous LM, which the tree may move by rounding); at least 50 of the 60 frames must get that far."""
    ed = gpu_api.PoseLidarOptimizer(max_obs=1536, max_cloud=6144, max_batch=1)
    tr = gpu_api.PoseLidarOptimizer(max_obs=1536, max_cloud=6144, max_batch=1, sums="tree")
    mp = gpu_api.LidarMap(max_points=40000)
    worst, compared = 0.0, 0
    for seed in range(60):
        rng = np.random.default_rng(seed)
        f = PLS.random_frame(2000 + seed, n_obs=int(rng.choice([40, 150, 400, 1500])), n_cloud=int(rng.choice([300, 1000, 3000])),
                             n_map=int(rng.choice([600, 3000, 12000])), n_iterations=3)
        f["map"] = mp.set(f["map_xyz"])
        a = ed.PoseLidarVisualOptimization(f)
        ea = ed.fetch_edges(0, 0)
        b = tr.PoseLidarVisualOptimization(f)
        eb = tr.fetch_edges(0, 0)
        assert a["round_edges"][0] > 0, seed
        assert a["round_edges"][0] == b["round_edges"][0] and a["round_valid"][0] == b["round_valid"][0], seed
        assert np.array_equal(_bits(a["round_chi2"][:1]), _bits(b["round_chi2"][:1])), seed
        for x, y in zip(ea, eb):
            assert np.array_equal(_bits(x), _bits(y)), seed
        if a["round_edges"] != b["round_edges"]:
            continue
        compared += 1
        rel = np.linalg.norm(np.r_[a["q"] - b["q"], a["t"] - b["t"]]) / max(1.0, np.linalg.norm(np.r_[a["q"], a["t"]]))
        assert rel < 1e-6, (seed, rel)  # measured: at most 3.4e-7
        worst = max(worst, rel)
        flips = np.nonzero(a["outlier"] != b["outlier"])[0]
        st = np.asarray(f["stereo"], bool)
        for e in flips:  # a flag may flip only where the chi2 sits within rounding of its threshold
            th = 7.815 if st[e] else 5.991
            assert abs(a["chi2"][e] - th) < 1e-5 * th, (seed, e, a["chi2"][e])
    print(f"tree vs edge order: {compared} of 60 frames compared, worst relative pose difference {worst:.2e}")
    assert compared >= 50, compared


def test_gate_literals_on_device(gpu_api):
    """The two built cases of the float / double gate literals (pose_lidar_support.gate_literal_cases: a plane residual of
    exactly 0.2f, rejected; a weight of exactly 0.1f, kept), as frames of 60 copies of the point: the kernel's edges are the
    restatement's."""
    opt = gpu_api.PoseLidarOptimizer(max_obs=64, max_cloud=128, max_batch=1)
    mp = gpu_api.LidarMap(max_points=64)
    cases = PLS.gate_literal_cases()
    assert [k for _, _, k in cases] == [0, 1]
    for mpx, po, kept in cases:
        f = dict(q=np.array([0, 0, 0, 1], np.float32), t=np.zeros(3, np.float32), xw=np.tile([[0.0, 0.0, 3.0]], (5, 1)),
                 obs=np.tile([[320.0, 240.0, 306.0]], (5, 1)), inv_sigma2=np.ones(5, np.float32), stereo=np.ones(5, np.uint8),
                 fx=500.0, fy=500.0, cx=320.0, cy=240.0, bf=40.0, cloud=np.tile(po, (60, 1)), map_xyz=mpx, n_iterations=1)
        rc, ro, edges = PLS.run(f)
        assert ro["round_edges"][0] == 60 * kept
        f["map"] = mp.set(mpx)
        r = opt.PoseLidarVisualOptimization(f)
        _same(r, ro, kept)
        _same_edges(opt, 0, edges, kept)


def test_refusals(gpu_api):
    f = PLS.random_frame(7, n_obs=40, n_cloud=300, n_map=600, n_iterations=2)
    opt = gpu_api.PoseLidarOptimizer(max_obs=64, max_cloud=512, max_batch=2)
    mp = gpu_api.LidarMap(max_points=1000)
    f["map"] = mp.set(f["map_xyz"])
    opt.PoseLidarVisualOptimization(f)
    with pytest.raises(gpu_api.GfsError):
        opt.PoseLidarVisualOptimization([f, f, f])  # batch
    with pytest.raises(gpu_api.GfsError):
        opt.PoseLidarVisualOptimization(dict(f, cloud=np.zeros((600, 3), np.float32)))  # cloud capacity
    with pytest.raises(gpu_api.GfsError):
        opt.PoseLidarVisualOptimization(dict(f, xw=np.zeros((65, 3)), obs=np.zeros((65, 3)), inv_sigma2=np.ones(65, np.float32),
                                             stereo=np.ones(65, np.uint8)))
    with pytest.raises(gpu_api.GfsError):
        opt.PoseLidarVisualOptimization(dict(f, n_iterations=5))
    with pytest.raises(gpu_api.GfsError, match="two-camera"):
        opt.PoseLidarVisualOptimization(dict(f, two_camera=1))
    with pytest.raises(gpu_api.GfsError):
        mp.set(f["map_xyz"][:4])
    with pytest.raises(gpu_api.GfsError):
        mp.set(np.zeros((1001, 3), np.float32))
    with pytest.raises(gpu_api.GfsError):  # a map that was never uploaded
        opt.PoseLidarVisualOptimization(dict(f, map=gpu_api.LidarMap(max_points=100)))


def test_end_to_end_closer_than_visual_only(gpu_api):
    """The purpose of the lidar edges: on a pose_lidar_frame scene the refined pose is closer to the truth than
    PoseOptimization's (whose pose the reference drops, SURVEY F12, but which is its best visual-only estimate)."""
    from scipy.spatial.transform import Rotation
    wins = 0
    for seed in range(4):
        f = synth.pose_lidar_frame(seed, n_obs=300, n_cloud=3000, outlier_frac=0.1)
        mp = gpu_api.LidarMap(max_points=len(f["map_xyz"])).set(f["map_xyz"])
        r = gpu_api.PoseLidarOptimizer(max_obs=512, max_cloud=4096, max_batch=1).PoseLidarVisualOptimization(dict(f, map=mp))
        pv = dict(q=f["q"].astype(np.float64), t=f["t"].astype(np.float64), xw=f["xw"], obs=f["obs"], inv_sigma2=f["inv_sigma2"],
                  stereo=f["stereo"], fx=f["fx"], fy=f["fy"], cx=f["cx"], cy=f["cy"], bf=f["bf"])
        v = gpu_api.PoseOptimizer(max_obs=512, max_batch=1).PoseOptimization(pv)

        def err(q, t):
            dr = (Rotation.from_quat(q) * Rotation.from_quat(f["q_gt"]).inv()).magnitude()
            return np.linalg.norm(np.asarray(t) - f["t_gt"]) + dr

        wins += err(r["q"], r["t"]) < err(v["q"], v["t"])
        assert r["lidar_rounds"] == 3 and r["n_lidar_inliers"] > 1000
    assert wins >= 3, wins
