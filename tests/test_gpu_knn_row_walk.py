"""GPU half of the row-walk tests (MI355X): k_knn_cov walks every row of its 27-cell cube outwards from the query's x and stops a side
once nothing ahead can be among the k nearest (csrc/gicp.hip: KnnRowWalk, knn_search_cube).  The clouds of
tests/knn_row_walk_support.py are the smallest shapes at which that walk can go wrong; tests/test_knn_row_walk_reference.py pins
their caps on the CPU.  For every cloud:
  (a) points and covariances are bit-equal to the same call under GFS_GICP_KNN_EXACT=1 (every query through the exact deferred
      passes, which know nothing of the walk) -- no point is left out;
  (b) the covariances are within 1e-9 + d_or_cov of the brute-force reference on every point with a defined normal and no exact tie;
  (c) gfs_gicp_knn_stats: no more queries deferred than the true k-th distances and the keys' resolution allow, none at all where
      every k-th distance is within one cell -- a walk that stops too early shows here or in (a).
And one batch call of three of the clouds and a VGA depth-camera cloud gives the bits of the single calls."""
import os

import numpy as np
import pytest

import gicp_geometry_support as G
import knn_row_walk_support as W

pytestmark = pytest.mark.gpu
CAP = 8192
CAP_VGA = 20480  # a VGA depth image at stride 4 holds 19 200 points


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _run(api, reg, c, name=None):
    cfg = api.gicp_default_config()
    cfg.max_iterations = 1
    if name is not None:
        W.config(name, cfg)
    reg.RegisterPointClouds(c, c, None, cfg)
    pts, cov = reg.preprocessed(0, 0)
    return dict(pts=pts, cov=cov, stats=reg.knn_stats(0, 0)[0].astype(np.int64))


def _vga_cloud(api):
    from geoflowslam_amd import synth
    return synth.frame_pair(1000)["cloud0"]


def _collect(api):
    reg = api.RegistrationGICP(max_points=CAP)
    out = {name: _run(api, reg, W.cloud(name), name) for name in W.NAMES}
    reg.close()
    reg = api.RegistrationGICP(max_points=CAP_VGA)
    out["vga"] = _run(api, reg, _vga_cloud(api))
    reg.close()
    return out


@pytest.fixture(scope="module")
def runs(gpu_api):
    """(default, exact): every cloud once through a fresh handle, and once more under GFS_GICP_KNN_EXACT=1."""
    assert "GFS_GICP_KNN_EXACT" not in os.environ and "GFS_GICP_CELL" not in os.environ
    default = _collect(gpu_api)
    os.environ["GFS_GICP_KNN_EXACT"] = "1"
    try:
        exact = _collect(gpu_api)
    finally:
        del os.environ["GFS_GICP_KNN_EXACT"]
    return default, exact


@pytest.mark.parametrize("name", W.NAMES + ("vga",))
def test_exact_passes_give_the_same_bits(runs, name):
    """(a)"""
    d, e = runs[0][name], runs[1][name]
    assert int(e["stats"][1]) == int(e["stats"][0]) == len(e["pts"]) == len(d["pts"]), (name, d["stats"], e["stats"])
    assert np.array_equal(_bits(d["pts"]), _bits(e["pts"])), name
    diff = int((_bits(d["cov"]) != _bits(e["cov"])).any(axis=(1, 2)).sum())
    print(f"{name}: m {len(d['pts'])} deferred by default {int(d['stats'][1])}, covariances that differ from the exact passes' {diff}")
    assert diff == 0, (name, diff, d["stats"])


@pytest.mark.parametrize("name", W.NAMES)
def test_covariances_match_brute_force(runs, name):
    """(b)"""
    f = W.facts(name)
    d = runs[0][name]
    po, m = f["po"], len(f["po"])
    assert len(d["pts"]) == m
    ig, io = G.lexorder(d["pts"]), G.lexorder(po)
    assert (d["pts"][ig] == po[io]).all(), "voxel means differ"
    cov = np.zeros_like(d["cov"])
    cov[io] = d["cov"][ig]
    assert int(f["tie"].sum()) == 0 and int((f["gap"] <= G.GAP_MIN).sum()) <= 0.05 * m and f["d_or_cov"] <= 1e-9  # the caps, again
    if m < 5:
        assert (cov == np.eye(3)).all()
        return
    good = f["good"]
    d_ref = np.abs(cov - f["ref"]).reshape(m, -1).max(1)
    d_or = np.abs(cov - f["co"]).reshape(m, -1).max(1)
    print(f"{name}: m {m} compared {int(good.sum())} |gpu - reference| {d_ref[good].max():.2e} |gpu - oracle| {d_or[good].max():.2e} "
          f"d_or_cov {f['d_or_cov']:.2e}")
    w = int(np.argmax(np.where(good, d_ref, -1)))
    assert d_ref[good].max() <= 1e-9 + f["d_or_cov"], (name, w, d_ref[w], f["d10"][w], po[w], d["stats"])
    assert d_or[good].max() < 1e-9, name


@pytest.mark.parametrize("name", W.NAMES)
def test_the_pass_that_answered(runs, name):
    """(c)"""
    pc = G.path_counts(W.facts(name))
    m, to_r2, to_iso = (int(x) for x in runs[0][name]["stats"])
    print(f"{name}: m {m} (certified, r = 2, isolated) = ({m - to_r2}, {to_r2 - to_iso}, {to_iso}); brute force {pc}")
    assert m == pc["m"] and 0 <= to_iso <= to_r2 <= m
    assert to_r2 <= pc["beyond_cell"] + pc["near_ties"]
    if name in W.ALL_CERTIFIED:
        assert pc["beyond_cell"] + pc["near_ties"] == 0 and to_r2 == 0


def test_one_batch_call_gives_the_bits_of_the_single_calls(gpu_api, runs):
    from test_gpu_gms import _Hip
    names = list(W.BATCHED) + ["vga"]
    clouds = [W.cloud(n) for n in W.BATCHED] + [_vga_cloud(gpu_api)]
    B = len(names)
    c0, n0 = np.zeros((B, CAP_VGA, 4), np.float32), np.zeros(B, np.int32)
    for b, c in enumerate(clouds):
        c0[b, :len(c)], n0[b] = c, len(c)
    hip = _Hip()
    d = [hip.to_device(x) for x in (c0, n0)]
    cfg = gpu_api.gicp_default_config()
    cfg.max_iterations = 1
    reg = gpu_api.RegistrationGICP(max_points=CAP_VGA, max_batch=B)
    reg.align_batch_device(d[0], d[1], d[0], d[1], B, CAP_VGA, cfg=cfg)
    for b, name in enumerate(names):
        for which in (0, 1):
            pts, cov = reg.preprocessed(b, which)
            assert np.array_equal(reg.knn_stats(b, which)[0], runs[0][name]["stats"]), (name, which)
            assert np.array_equal(_bits(pts), _bits(runs[0][name]["pts"])), (name, which)
            assert np.array_equal(_bits(cov), _bits(runs[0][name]["cov"])), (name, which)
    reg.close()
    hip.free()
