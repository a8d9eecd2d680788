"""Shared by tests/test_gpu_knn_cov_parent_bits.py and tools/record_knn_cov_parent.py: the clouds whose neighbourhood covariances
(k_knn_cov, k_knn_cov_far, k_knn_cov_far_wg of csrc/gicp.hip, through csrc/eig3_direct.hpp) are pinned to a recording made with the
library of the commit before the closed form moved into that header, and the one way both run them.  Not a test module.

The clouds: those of tests/knn_row_walk_support.py that hold at most 1 200 raw points (`faces_and_corners` and `wide_extent` hold
more), two lattice planes (the
covariance of every neighbourhood has rank 2, with a row of exact zeros), a straight line with x == y bit for bit (rank 1, equal
diagonal entries), seven points (every query uses all seven) and one ragged batch of three of them in one call."""
import os

import numpy as np

import knn_row_walk_support as W

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_cov_parent.npz")
MAX_POINTS = 1200
SUPPORT = tuple(n for n in W.NAMES if n not in ("faces_and_corners", "wide_extent"))
OWN = ("plane_z", "plane_y", "line_xy", "seven")
NAMES = SUPPORT + OWN
BATCH = ("x_planes", "line_xy", "seven")  # 1 152, 100 and 7 points in one call (default leaf, as a batch shares its configuration)
PATHS = ("default", "exact")               # exact: GFS_GICP_KNN_EXACT=1, every query through the deferred passes


def _f4(xyz):
    xyz = np.asarray(xyz, np.float64)
    return np.ascontiguousarray(np.c_[xyz, np.ones(len(xyz))], np.float32)


def cloud(name):
    """float32 [n, 4] (w = 1), deterministic; the lattices step by 0.03, so every point keeps a voxel (leaf 0.02) of its own."""
    if name in W.NAMES:
        return W.cloud(name)
    i, j = (g.ravel() for g in np.meshgrid(np.arange(18), np.arange(18)))
    if name == "plane_z":
        return _f4(np.c_[0.03 * i, 0.03 * j, np.full(len(i), 0.5)])
    if name == "plane_y":
        return _f4(np.c_[0.03 * i, np.full(len(i), 0.25), 0.03 * j])
    if name == "line_xy":
        t = 0.03 * np.arange(100)
        return _f4(np.c_[t, t, np.full(len(t), 0.5)])
    if name == "seven":
        rng = np.random.default_rng(7)
        site = rng.permutation(27)[:7]  # seven sites of a 3 x 3 x 3 lattice of step 0.05, each jittered inside its own voxels
        return _f4(np.stack([site // 9, site // 3 % 3, site % 3], 1) * 0.05 + rng.uniform(0, 0.019, (7, 3)))
    raise KeyError(name)


def cov6(cov):
    """[m, 3, 3] as api.RegistrationGICP.preprocessed returns it -> [m, 6] = (xx, xy, xz, yy, yz, zz); the matrices must be symmetric."""
    cov = np.asarray(cov, np.float64)
    assert cov.transpose(0, 2, 1).tobytes() == cov.tobytes()
    return np.ascontiguousarray(np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1))


def _cfg(api, name=None):
    cfg = api.gicp_default_config()
    cfg.max_iterations = 1
    return W.config(name, cfg) if name in W.NAMES else cfg


def run_single(api, clouds):
    """{name: cov6} of every cloud alone through one handle."""
    reg = api.RegistrationGICP(max_points=MAX_POINTS)
    out = {}
    for name, c in clouds.items():
        reg.RegisterPointClouds(c, c, None, _cfg(api, name))
        out[name] = cov6(reg.preprocessed(0, 0)[1])
    reg.close()
    return out


def run_batch(api, clouds, hip):
    """[cov6] of the clouds of BATCH in one align_batch_device call; hip: tests/test_gpu_gms.py's _Hip."""
    B = len(BATCH)
    c0, n0 = np.zeros((B, MAX_POINTS, 4), np.float32), np.zeros(B, np.int32)
    for b, name in enumerate(BATCH):
        c0[b, :len(clouds[name])], n0[b] = clouds[name], len(clouds[name])
    d = [hip.to_device(x) for x in (c0, n0)]
    reg = api.RegistrationGICP(max_points=MAX_POINTS, max_batch=B)
    reg.align_batch_device(d[0], d[1], d[0], d[1], B, MAX_POINTS, cfg=_cfg(api))
    out = [cov6(reg.preprocessed(b, 0)[1]) for b in range(B)]
    reg.close()
    return out


def run_all(api, clouds, hip):
    """{(path, key): cov6}, key a cloud's name or 'batch<b>', once on the default path and once under GFS_GICP_KNN_EXACT=1."""
    assert "GFS_GICP_KNN_EXACT" not in os.environ and "GFS_GICP_CELL" not in os.environ
    out = {}
    for path in PATHS:
        if path == "exact":
            os.environ["GFS_GICP_KNN_EXACT"] = "1"
        try:
            for k, v in run_single(api, clouds).items():
                out[path, k] = v
            for b, v in enumerate(run_batch(api, clouds, hip)):
                out[path, "batch%d" % b] = v
        finally:
            os.environ.pop("GFS_GICP_KNN_EXACT", None)
    return out


def load():
    """-> (clouds {name: float32 [n, 4]}, golden {(path, key): float64 [m, 6]}, the commit the recording was made on).  A recording
    whose bytes equal an earlier one's is stored once, with its key in `same_as`."""
    z = np.load(FIXTURE)
    clouds = {n: np.ascontiguousarray(np.c_[z["cloud/" + n], np.ones(len(z["cloud/" + n]), np.float32)], np.float32) for n in NAMES}
    same = dict(s.split("=") for s in z["same_as"].tolist())
    golden = {}
    for path in PATHS:
        for key in NAMES + tuple("batch%d" % b for b in range(len(BATCH))):
            k = "cov/%s/%s" % (path, key)
            golden[path, key] = z[same.get(k, k)]
    return clouds, golden, str(z["parent_commit"])
