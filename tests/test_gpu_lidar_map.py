"""GPU tests of the lidar local-map build (LidarMapping::viewer, reference src/LidarMapping.cc:130-185; gfs_lidar_mapper_* in
include/gfs_abi.h): the voxel filter and the whole build bit for bit against the sequential CPU restatement
(tests/host/lidar_map_restatement.cpp); the search grid byte for byte against gfs_lidar_map_set of the same points, directly and
through PoseLidarVisualOptimization / LocalVisualLidarBA; the refusals (which leave the previous map as it was); determinism; the
passthrough branch."""
import ctypes as C

import numpy as np
import pytest

import lba_lidar_support as LLS
import lidar_map_support as LMS
import pose_lidar_support as PLS

pytestmark = pytest.mark.gpu

CAP = 20000  # the filter tests' mapper capacity
F = np.float32


def _filter_rc(api, mapper, xyz, leaf, cap=None):
    """gfs_voxel_grid_filter with its status -> (rc, points or None, info)."""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    cap = len(xyz) if cap is None else cap
    out, info = np.full((max(cap, 1), 3), np.nan, F), api.LidarMapInfo()
    rc = api.lib().gfs_voxel_grid_filter(mapper.h, xyz.ctypes.data, len(xyz), C.c_float(leaf), out.ctypes.data, cap, C.byref(info))
    I = api.lidar_map_info(info)
    return rc, (out[:I["n_out"]].copy() if rc == 0 else out), I


def _build_rc(api, mapper, lidar_map, w, leaf):
    """gfs_lidar_map_build with its status -> (rc, info)."""
    q = np.ascontiguousarray(w["q"], F).reshape(-1, 4)
    t = np.ascontiguousarray(w["t"], F).reshape(-1, 3)
    cb = np.ascontiguousarray(w["cloud_begin"], np.int32)
    cloud = np.ascontiguousarray(w["cloud"], F).reshape(-1, 3)
    I = api.LidarMapInput(len(q), q.ctypes.data, t.ctypes.data, cb.ctypes.data, cloud.ctypes.data, float(F(leaf)))
    info = api.LidarMapInfo()
    rc = api.lib().gfs_lidar_map_build(mapper.h, C.byref(I), lidar_map.h, C.byref(info))
    return rc, api.lidar_map_info(info)


def _check_filter(api, mapper, xyz, leaf, tag):
    rc, pts, info = _filter_rc(api, mapper, xyz, leaf)
    rrc, rpts, rinfo = LMS.voxel_filter(xyz, leaf)
    assert rc == rrc == 0, (tag, rc, rrc, api.lib().gfs_last_error())
    assert info == rinfo, (tag, info, rinfo)
    assert LMS.same_bits(pts, rpts), tag
    return info


# ------------------------------------------------------------------ 4. the filter

def test_voxel_filter_random_clouds_bit_exact(gpu_api):
    mapper = gpu_api.LidarMapper(CAP, 4)
    rng = np.random.default_rng(2024)
    sizes = [1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, CAP - 1, CAP]
    sizes += [int(v) for v in np.exp(rng.uniform(0, np.log(CAP), 30))]
    merged = 0
    for k, n in enumerate(sizes):
        leaf = LMS.LEAVES[k % 4]
        ext = rng.uniform(0.2, 3.0, 3) * rng.choice([1.0, 0.1], 3, p=[0.8, 0.2])
        xyz = (rng.uniform(-1, 1, (n, 3)) * ext + rng.uniform(-3, 3, 3)).astype(F)
        info = _check_filter(gpu_api, mapper, xyz, leaf, (k, n, leaf))
        assert info["passthrough"] == 0
        merged += info["n_out"] < n
    assert len(sizes) >= 40 and merged >= 20


def test_voxel_filter_constructed_clouds_bit_exact(gpu_api):
    mapper = gpu_api.LidarMapper(CAP, 4)
    for name, xyz, leaf in LMS.constructed_clouds():
        info = _check_filter(gpu_api, mapper, xyz, leaf, name)
        assert info["passthrough"] == (1 if name == "passthrough" else 0), name
    # 5000 points in one voxel: one thread adds them in input order
    rng = np.random.default_rng(5)
    xyz = (F(1.203) + rng.uniform(0, 0.09, (5000, 3))).astype(F)
    info = _check_filter(gpu_api, mapper, xyz, 0.1, "5000 in one voxel")
    assert info["n_out"] == 1
    # ... and next to ordinary voxels
    xyz = np.concatenate([rng.uniform(-2, 2, (3000, 3)).astype(F), xyz, rng.uniform(-2, 2, (3000, 3)).astype(F)])
    info = _check_filter(gpu_api, mapper, xyz[rng.permutation(len(xyz))], 0.1, "5000 in one voxel among others")
    assert 1 < info["n_out"] < 6001
    # the Python wrapper
    pts, info = mapper.voxel_filter(xyz, 0.2)
    assert LMS.same_bits(pts, LMS.voxel_filter(xyz, 0.2)[1])


# ------------------------------------------------------------------ 5. + 6. (directly) the build, the fetch, the grid

def _windows():
    ws = [(LMS.window(s, n_keyframes=k, scaled=bool(s % 2)), leaf, f"s{s}_k{k}_l{leaf}") for s, k, leaf in LMS.WINDOWS[:20]]
    ws.append((LMS.window(40, n_keyframes=7, empty=(0, 3, 6)), 0.1, "empty_0_3_6"))
    ws.append((LMS.window(43, n_keyframes=30, empty=(1, 2, 29)), 0.04, "empty_1_2_29"))
    # a large window, then small ones on the same mapper and map: nothing of the large one may survive
    ws.append((LMS.window(44, n_keyframes=30, n_cloud=3000, width=160, height=120), 0.04, "large"))
    ws.append((LMS.window(45, n_keyframes=1, n_cloud=100), 0.2, "small_after_large"))
    ws.append((LMS.window(46, n_keyframes=2, n_cloud=40), 0.02, "smaller"))
    return ws


def test_build_fetch_and_grid_bit_exact(gpu_api):
    mapper = gpu_api.LidarMapper(90000, 30)
    built, second = gpu_api.LidarMap(max_points=90000), gpu_api.LidarMap(max_points=90000)
    ws = _windows()
    assert len(ws) >= 20
    for w, leaf, tag in ws:
        rrc, rpts, rinfo = LMS.build(w, leaf)
        assert rrc == 0, tag
        info = mapper.build(built, w["q"], w["t"], w["clouds"], leaf)
        assert info == rinfo, (tag, info, rinfo)
        got = built.fetch()
        assert LMS.same_bits(got, rpts), tag
        # the grid, byte for byte that of gfs_lidar_map_set on the same points
        second.set(got)
        ga, gb = LMS.grid(gpu_api, built), LMS.grid(gpu_api, second)
        assert ga["n"] == info["n_out"] and ga["start"][0] == 0 and ga["start"][-1] == ga["n"], tag
        assert LMS.same_grid(ga, gb), tag
        assert LMS.same_bits(second.fetch(), rpts), tag


# ------------------------------------------------------------------ 6. through the consumers

def _pose_fields(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("outlier", "chi2", "q", "t", "qf", "tf", "avg_reproj_error", "n_inliers",
                                                                  "n_lidar_inliers", "residual", "lidar_rounds", "rounds_run",
                                                                  "iterations_run", "round_edges", "round_chi2", "round_valid"))


def _pose_run(opt, f, m):
    r = opt.PoseLidarVisualOptimization(dict(f, map=m))
    edges = [opt.fetch_edges(0, rnd) for rnd in range(4)]
    return r, _pose_fields(r) + b"".join(a.tobytes() for e in edges for a in e)


def test_pose_optimization_same_bits_with_device_built_map(gpu_api):
    mapper = gpu_api.LidarMapper(16384, 8)
    opt = gpu_api.PoseLidarOptimizer(max_obs=512, max_cloud=2048, max_batch=1)
    assert len(LMS.POSE_SEEDS) >= 10
    for seed in LMS.POSE_SEEDS:
        f, w = LMS.pose_problem(seed)
        built, second = gpu_api.LidarMap(max_points=16384), gpu_api.LidarMap(max_points=16384)
        mapper.build(built, w["q"], w["t"], w["clouds"], LMS.POSE_LEAF)
        second.set(built.fetch())
        ra, a = _pose_run(opt, f, built)
        rb, b = _pose_run(opt, f, second)
        assert a == b, seed
        # not vacuous: the restatement on the restated map finds >= 100 lidar edges in the first round, and so does the device
        rrc, rmap, _ = LMS.build(w, LMS.POSE_LEAF)
        assert rrc == 0 and LMS.same_bits(built.fetch(), rmap)
        _, ref, _ = PLS.run(dict(f, map_xyz=rmap))
        assert ref["round_edges"][0] >= 100, (seed, ref["round_edges"])
        assert list(ra["round_edges"]) == list(ref["round_edges"]) and ra["round_edges"][0] >= 100, seed


def test_local_ba_same_bits_with_device_built_map(gpu_api):
    w, mw = LMS.lba_problem()
    mapper = gpu_api.LidarMapper(16384, 8)
    built, second = gpu_api.LidarMap(max_points=16384), gpu_api.LidarMap(max_points=16384)
    mapper.build(built, mw["q"], mw["t"], mw["clouds"], 0.1)
    second.set(built.fetch())
    opt = gpu_api.Optimizer(max_poses=16, max_points=1024, max_edges=16384)

    def run(m):
        r = opt.LocalVisualLidarBA(w, m)
        e = [opt.fetch_lidar_edges(i) for i in range(w["n_poses"])]
        blob = b"".join(np.ascontiguousarray(r[k]).tobytes() for k in sorted(r)) + b"".join(a.tobytes() for x in e for a in x)
        return r, blob

    ra, a = run(built)
    rb, b = run(second)
    assert a == b
    rrc, rmap, _ = LMS.build(mw, 0.1)
    assert rrc == 0 and LMS.same_bits(built.fetch(), rmap)
    ref, _ = LLS.solve(dict(w, map_xyz=rmap))
    lidar = list(LMS.LBA_CFG["lidar"])
    assert (ref["pose_lidar_edges"][lidar] > 0).all(), ref["pose_lidar_edges"]
    assert (ra["pose_lidar_edges"] == ref["pose_lidar_edges"]).all() and (ra["pose_lidar_edges"][lidar] > 0).all()


# ------------------------------------------------------------------ 7. refusals

def _good(gpu_api):
    f, w = LMS.pose_problem(0)
    n_out = LMS.build(w, LMS.POSE_LEAF)[2]["n_out"]
    mapper = gpu_api.LidarMapper(9000, 4)
    m = gpu_api.LidarMap(max_points=n_out)  # exactly what the good build needs
    mapper.build(m, w["q"], w["t"], w["clouds"], LMS.POSE_LEAF)
    opt = gpu_api.PoseLidarOptimizer(max_obs=512, max_cloud=2048, max_batch=1)
    return f, w, mapper, m, opt


def _ident(clouds):
    clouds = [np.asarray(c, F).reshape(-1, 3) for c in clouds]
    k = len(clouds)
    return dict(q=np.tile(F([0, 0, 0, 1]), (k, 1)), t=np.zeros((k, 3), F), clouds=clouds,
                cloud_begin=np.r_[0, np.cumsum([len(c) for c in clouds])].astype(np.int32),
                cloud=np.concatenate(clouds).astype(F).reshape(-1, 3))


def test_refusals_keep_the_previous_map(gpu_api):
    f, w, mapper, m, opt = _good(gpu_api)
    grid0, fetch0 = LMS.grid(gpu_api, m), m.fetch()
    _, blob0 = _pose_run(opt, f, m)
    rng = np.random.default_rng(8)
    box = rng.uniform(-1, 1, (200, 3)).astype(F)
    nan = box.copy()
    nan[77, 2] = np.nan
    inf = box.copy()
    inf[5, 0] = np.inf
    far = _ident([box])
    far["t"] = F([[2.5e6, 0, 0]])
    corners, _ = LMS.overflow_pair()
    dense = LMS.window(47, n_keyframes=4, n_cloud=2200, width=160, height=120)  # more map points at 0.02 m than the map holds
    assert LMS.build(dense, 0.02)[2]["n_out"] > grid0["n"] and len(dense["cloud"]) <= 9000
    cases = [
        ("points beyond the mapper's capacity", _ident([np.tile(box, (46, 1))]), 0.1, LMS.CAPACITY),
        ("key-frames beyond the mapper's capacity", _ident([box] * 5), 0.1, LMS.CAPACITY),
        ("map points beyond the map's capacity", dense, 0.02, LMS.CAPACITY),
        ("a NaN point", _ident([box, nan]), 0.1, LMS.INVALID_ARG),
        ("an infinite point", _ident([inf]), 0.1, LMS.INVALID_ARG),
        ("a point beyond 1e6 m after the transform", far, 0.1, LMS.INVALID_ARG),
        ("fewer than 5 map points", _ident([box + F(2)]), 100.0, LMS.INVALID_ARG),
        ("fewer than 5 input points", _ident([box[:2], box[2:4]]), 0.1, LMS.INVALID_ARG),
        ("zero points", _ident([box[:0], box[:0]]), 0.1, LMS.INVALID_ARG),
        ("leaf 0", _ident([box]), 0.0, LMS.INVALID_ARG),
        ("leaf negative", _ident([box]), -0.1, LMS.INVALID_ARG),
        ("leaf NaN", _ident([box]), np.nan, LMS.INVALID_ARG),
        ("leaf infinite", _ident([box]), np.inf, LMS.INVALID_ARG),
        ("div overflow", _ident([np.repeat(corners, 3, axis=0)]), 1.0, LMS.UNSUPPORTED),
    ]
    for name, win, leaf, want in cases:
        rc, info = _build_rc(gpu_api, mapper, m, win, leaf)
        assert rc == want, (name, rc, gpu_api.lib().gfs_last_error())
        if want != LMS.CAPACITY and name != "div overflow" and "leaf" not in name:
            assert LMS.build(win, leaf)[0] == want, name  # the restatement refuses the same
        assert LMS.same_grid(LMS.grid(gpu_api, m), grid0), name
    assert LMS.voxel_filter(np.repeat(corners, 3, axis=0), 1.0)[0] == LMS.UNSUPPORTED
    # the filter's own refusals; nothing is truncated
    rc, out, info = _filter_rc(gpu_api, mapper, box, 0.1, cap=10)
    assert rc == LMS.CAPACITY and info["n_out"] > 10 and np.isnan(out).all()
    assert _filter_rc(gpu_api, mapper, np.tile(box, (46, 1)), 0.1)[0] == LMS.CAPACITY
    assert _filter_rc(gpu_api, mapper, nan, 0.1)[0] == LMS.INVALID_ARG
    assert _filter_rc(gpu_api, mapper, box, 0.0)[0] == LMS.INVALID_ARG
    assert _filter_rc(gpu_api, mapper, corners, 1.0)[0] == LMS.UNSUPPORTED
    assert _filter_rc(gpu_api, mapper, box[:1], 0.1)[0] == 0  # any n >= 1
    # the map is the one built before the refused calls: same points, same grid, same bits out of the optimizer
    assert LMS.same_bits(m.fetch(), fetch0) and LMS.same_grid(LMS.grid(gpu_api, m), grid0)
    assert _pose_run(opt, f, m)[1] == blob0
    # and the mapper still builds
    info = mapper.build(m, w["q"], w["t"], w["clouds"], LMS.POSE_LEAF)
    assert info["n_out"] == grid0["n"] and LMS.same_grid(LMS.grid(gpu_api, m), grid0)


def test_refusal_map_on_another_device(gpu_api):
    if gpu_api.device_count() < 2:
        pytest.skip("map on another device: this machine shows one device")
    f, w = LMS.pose_problem(0)
    mapper = gpu_api.LidarMapper(9000, 4, device=0)
    other = gpu_api.LidarMap(max_points=9000, device=1)
    rc, _ = _build_rc(gpu_api, mapper, other, w, 0.1)
    assert rc == LMS.INVALID_ARG


# ------------------------------------------------------------------ 8. determinism

def test_three_builds_are_identical(gpu_api):
    f, w = LMS.pose_problem(1)
    big = LMS.window(44, n_keyframes=30, n_cloud=3000, width=160, height=120)
    mapper = gpu_api.LidarMapper(90000, 30)
    opt = gpu_api.PoseLidarOptimizer(max_obs=512, max_cloud=2048, max_batch=1)
    blobs, bigs = [], []
    for _ in range(3):
        m = gpu_api.LidarMap(max_points=90000)
        mapper.build(m, big["q"], big["t"], big["clouds"], 0.04)
        g = LMS.grid(gpu_api, m)
        bigs.append(m.fetch().tobytes() + g["start"].tobytes() + g["pts"].tobytes() + g["index"].tobytes())
        mapper.build(m, w["q"], w["t"], w["clouds"], LMS.POSE_LEAF)
        g = LMS.grid(gpu_api, m)
        blobs.append(m.fetch().tobytes() + g["start"].tobytes() + g["index"].tobytes() + _pose_run(opt, f, m)[1])
    assert blobs[0] == blobs[1] == blobs[2]
    assert bigs[0] == bigs[1] == bigs[2]


# ------------------------------------------------------------------ 9. passthrough

def test_passthrough_build(gpu_api):
    f, w = LMS.pose_problem(2)
    mapper = gpu_api.LidarMapper(9000, 4)
    built, second = gpu_api.LidarMap(max_points=9000), gpu_api.LidarMap(max_points=9000)
    info = mapper.build(built, w["q"], w["t"], w["clouds"], LMS.PASSTHROUGH_LEAF)
    world = LMS.transform(w)
    assert info == dict(n_in=len(world), n_out=len(world), passthrough=1, div=(0, 0, 0))
    assert info == LMS.build(w, LMS.PASSTHROUGH_LEAF)[2]
    assert LMS.same_bits(built.fetch(), world)  # the transformed input, in input order
    second.set(world)
    assert LMS.same_grid(LMS.grid(gpu_api, built), LMS.grid(gpu_api, second))
    opt = gpu_api.PoseLidarOptimizer(max_obs=512, max_cloud=2048, max_batch=1)
    ra, a = _pose_run(opt, f, built)
    assert a == _pose_run(opt, f, second)[1] and ra["round_edges"][0] >= 100
