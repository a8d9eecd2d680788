"""GPU half of the deferred-pass tests (MI355X).  k_knn_cov_far scans the rows of the r = 2 cube, keeps the candidates within the
bound in a list of 64 per query and ranks them by counting; it and k_knn_cov_far_wg leave each query's neighbour list in its
covariance slot and k_knn_cov_settle turns the lists into covariances (csrc/gicp.hip).  None of this may change a bit: for every
cloud of tests/knn_far_rows_support.py (tests/test_knn_far_rows_reference.py pins what they are on the CPU)
  (a) the covariances are bit-equal to tests/golden/knn_far_rows_parent.npz -- recorded by tools/record_knn_far_rows_parent.py with
      the library of the commit named in the fixture, before these kernels were touched -- on the default path and under
      GFS_GICP_KNN_EXACT=1, where every query goes through the deferred passes;
  (b) both paths agree bit for bit;
  (c) the counts of gfs_gicp_knn_stats and the sorted bounds handed to k_knn_cov_far_wg equal the recording; on box_corner every
      query is deferred and exactly the brute-force count of k-th distances beyond two cells goes on to the third pass;
  (d) except on tie_shell, the covariances are within 1e-9 + d_or_cov of the brute force (the bar of tests/test_gpu_knn_row_walk.py);
      on tie_shell within 1e-9 of the oracle's arithmetic on the (distance, index) list of the points as the device holds them;
and one ragged batch of all of them and an empty cloud gives the single calls' bits, as does the streaming call behind it, whose
target slot keeps its covariances (k_knn_cov_settle honours `only`)."""
import numpy as np
import pytest

import gicp_geometry_support as G
import knn_far_rows_support as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return S.load()


@pytest.fixture(scope="module")
def runs(gpu_api, recorded):
    """Everything once, from the clouds as the fixture holds them."""
    from test_gpu_gms import _Hip
    hip = _Hip()
    out = S.run_all(gpu_api, recorded[0], hip)
    hip.free()
    return out


def _mat(c6):
    return np.stack([c6[:, [0, 1, 2]], c6[:, [1, 3, 4]], c6[:, [2, 4, 5]]], 1)


@pytest.mark.parametrize("path", S.PATHS)
@pytest.mark.parametrize("name", S.NAMES)
def test_covariances_counts_and_bounds_are_the_parents(runs, recorded, path, name):
    """(a), (c)"""
    got, want = runs[path]["single"][name], recorded[1][path, name]
    assert got["cov"].dtype == want["cov"].dtype == np.float64 and got["cov"].shape == want["cov"].shape, (path, name)
    diff = (got["cov"].view(np.uint64) != want["cov"].view(np.uint64)).any(1)
    print(f"{path} {name}: {len(diff)} points, stats {got['stats']} (parent {want['stats']}), covariances that differ {int(diff.sum())}")
    assert not diff.any(), (path, name, int(diff.sum()), np.nonzero(diff)[0][:8], got["cov"][diff][:2], want["cov"][diff][:2])
    assert np.array_equal(got["stats"], want["stats"]), (path, name, got["stats"], want["stats"])
    assert got["dnext"].tobytes() == np.ascontiguousarray(want["dnext"], np.float64).tobytes(), (path, name)
    if path == "exact":
        assert got["stats"][1] == got["stats"][0]


@pytest.mark.parametrize("name", S.NAMES)
def test_default_and_exact_paths_agree(runs, name):
    """(b)"""
    d, e = runs["default"]["single"][name], runs["exact"]["single"][name]
    assert d["pts"].tobytes() == e["pts"].tobytes() and d["cov"].tobytes() == e["cov"].tobytes(), name
    # (what k_knn_cov certifies the r = 2 pass settles: the same queries reach the third pass, with the same bounds)
    assert d["stats"][2] == e["stats"][2] and d["dnext"].tobytes() == e["dnext"].tobytes(), name


def test_box_corner_every_query_is_deferred_and_the_corners_reach_the_third_pass(runs):
    """(c)"""
    f = S.facts("box_corner")
    m, to_r2, to_iso = (int(x) for x in runs["default"]["single"]["box_corner"]["stats"])
    assert m == len(f["po"]) == to_r2 and to_iso == int((f["d10"] > 2 * G.CELL).sum()) == 8


@pytest.mark.parametrize("name", S.NAMES)
def test_covariances_match_brute_force(runs, oracle, name):
    """(d)"""
    f, d = S.facts(name), runs["default"]["single"][name]
    po, m = f["po"], len(f["po"])
    assert len(d["pts"]) == m
    cov = _mat(d["cov"])
    if m < 5:
        assert (cov == np.eye(3)).all()
        return
    if name == "tie_shell":  # ties: the list is (distance, then the lower index among the points as the device holds them)
        want = G.closed_form_cov(d["pts"], S.order_list(d["pts"]), oracle)
        worst = np.abs(cov - want).reshape(m, -1).max(1)
        print(f"{name}: m {m} |gpu - (distance, index) list| {worst.max():.2e}")
        assert worst.max() <= 1e-9, (name, int(np.argmax(worst)), worst.max())
        return
    ig, io = G.lexorder(d["pts"]), G.lexorder(po)
    assert (d["pts"][ig] == po[io]).all(), "voxel means differ"
    c = np.zeros_like(cov)
    c[io] = cov[ig]
    good = f["good"]
    d_ref = np.abs(c - f["ref"]).reshape(m, -1).max(1)
    print(f"{name}: m {m} compared {int(good.sum())} |gpu - reference| {d_ref[good].max():.2e} d_or_cov {f['d_or_cov']:.2e}")
    assert f["d_or_cov"] <= 1e-9 and d_ref[good].max() <= 1e-9 + f["d_or_cov"], (name, int(np.argmax(np.where(good, d_ref, -1))))


@pytest.mark.parametrize("path", S.PATHS)
def test_ragged_batch_and_the_streaming_call_give_the_single_calls_bits(runs, path):
    diffs = S.batch_differences(runs[path])
    assert not diffs, (path, diffs)
