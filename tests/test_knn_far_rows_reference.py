"""CPU half of the deferred-pass tests: the clouds of tests/knn_far_rows_support.py are what that module says they are, by brute force
on the oracle's voxel means -- which queries k_knn_cov must defer, which of them the r = 2 pass of csrc/gicp.hip can settle and which
go on to k_knn_cov_far_wg, how many candidates survive in the r = 2 cube, where the exact ties are -- so that the GPU half
(tests/test_gpu_knn_far_rows.py) compares the kernels with figures that do not come from the kernels.  The fixture
tests/golden/knn_far_rows_parent.npz holds these very clouds."""
import numpy as np
import pytest

import gicp_geometry_support as G
import knn_far_rows_support as S

CELL = G.CELL


def _cells(po):
    return np.floor(np.asarray(po)[:, :3] * (1.0 / CELL)).astype(np.int64)


def _cube(po, r):
    """[m, m] bool: point b lies in the cube of +-r cells around point a's cell."""
    c = _cells(po)
    return np.abs(c[:, None, :] - c[None, :, :]).max(2) <= r


def _covers(po, r=2):
    """[m] bool: the cube of +-r cells around the point's cell covers the occupied box."""
    c = _cells(po)
    return ((c - r <= c.min(0)) & (c + r >= c.max(0))).all(1)


@pytest.mark.parametrize("name", S.NAMES)
def test_every_point_keeps_a_voxel_of_its_own_and_the_fixture_holds_the_cloud(name):
    c, f = S.cloud(name), S.facts(name)
    assert c.dtype == np.float32 and len(c) <= S.MAX_POINTS and (c[:, 3] == 1).all()
    assert len(f["po"]) == len(c), (name, len(f["po"]), len(c))
    assert (f["po"][G.lexorder(f["po"])][:, :3] == c[G.lexorder(c)][:, :3].astype(np.float64)).all(), name  # a mean of one point is the point
    clouds, golden, commit = S.load()
    assert commit == "4ff4b15" and clouds[name].tobytes() == c.tobytes() and len(clouds["empty"]) == 0
    assert set(golden) == {(p, n) for p in S.PATHS for n in S.NAMES}
    if name != "tie_shell":  # the bar of the brute-force comparison is the row-walk tests': no exact tie, the oracle within 1e-9
        assert int(f["tie"].sum()) == 0 and f["d_or_cov"] <= 1e-9 and f["good"].sum() >= 0.9 * len(c)


def test_shell_blob_six_unbounded_queries_with_more_survivors_than_any_list():
    f = S.facts("shell_blob")
    po, pc = f["po"], G.path_counts(f)
    own = np.nonzero(f["cube"] < G.K)[0]
    assert len(po) == 306 and len(own) == 6 and pc["beyond_cell"] == 6 and pc["near_ties"] == 0
    in2 = _cube(po, 2)[own]
    assert (in2.sum(1) == 306).all()  # unbounded: every candidate of the probe survives, 306 > 4 lists of 64
    d = np.sqrt(G._sqdist(po[own, :3], po[:, :3]))
    blob = np.delete(np.arange(len(po)), own)
    fourth = np.sort(d[:, blob], 1)[:, 3]  # the 10th neighbour is the 4th of the blob, 0.16 - 0.2 m away
    assert 0.15 < d[:, blob].min() < 0.17 and (fourth > 1.5 * CELL).all() and (fourth < 2.01 * CELL).all() and (fourth == f["d10"][own]).all()
    assert _covers(po)[own].all()  # the r = 2 pass settles all six (its cube covers the occupied box)
    c = _cells(po)
    assert len({(a[1], a[2]) for a in c}) == 4 and (np.ptp(c[:, 1]) + 1) * (np.ptp(c[:, 2]) + 1) == 9  # nine rows, five of them empty
    assert (np.abs(f["d10"][own] / (2 * CELL) - 1) > 1e-6).all() and (f["d10"][blob] < CELL).all()


def test_tie_shell_the_tenth_neighbour_is_one_of_many_at_one_exact_distance():
    c, f = S.cloud("tie_shell"), S.facts("tie_shell")
    units = c[:, :3].astype(np.float64) / S.U
    assert (units == np.round(units)).all()  # multiples of 2^-6 m: every difference, square and sum below is exact
    off = np.round(units).astype(np.int64) - np.array(S.TIE_Q)
    n2 = (off * off).sum(1)
    assert (n2 == 0).sum() == 1 and (n2 < 100).sum() == 9 and len(set(n2[n2 < 100])) == 9
    assert (n2 == S.TIE_N).sum() >= S.TIE_MIN and (n2 == S.FILL_N).sum() >= S.FILL_MIN and set(n2[n2 >= 100]) == {S.TIE_N, S.FILL_N}
    po = f["po"]
    q = int(np.nonzero((po[:, :3] == np.array(S.TIE_Q) * S.U).all(1))[0][0])
    assert f["cube"][q] == 9 and bool(f["tie"][q])  # unbounded, and the 10th and 11th are equally far
    sq = G._sqdist(po[q:q + 1, :3], po[:, :3])[0]
    assert (sq == S.TIE_N / 4096.0).sum() == (n2 == S.TIE_N).sum() and f["sq"][q, -1] == S.TIE_N / 4096.0
    assert CELL < np.sqrt(S.TIE_N) * S.U < np.sqrt(S.FILL_N) * S.U < 2 * CELL
    assert _cube(po, 2)[q].sum() == len(po) > 64 + 10  # the survivors do not fit one list: the batch path runs with the ties in it
    assert int(f["tie"].sum()) >= 24  # the tied points' own queries see ties as well (the lattice is symmetric)


def test_box_corner_every_query_is_deferred_and_the_corners_go_on():
    f = S.facts("box_corner")
    po, pc, d10 = f["po"], G.path_counts(f), f["d10"]
    m = len(po)
    assert m == 108 and pc["near_ties"] == 0 and int(f["tie"].sum()) == 0
    assert (d10 > 1.5 * CELL * (1 + 1e-6)).all()  # beyond what k_knn_cov can certify wherever the query sits in its cell
    assert (np.abs(d10 / (2 * CELL) - 1) > 1e-6).all() and not _covers(po).any()
    iso = d10 > 2 * CELL
    c = _cells(po)
    corner = ((c == c.min(0)) | (c == c.max(0))).all(1)
    assert iso.sum() == pc["must_isolated"] == 8 and (iso == ((f["cube"] < G.K) & corner)).all()
    # clamped probes: rows (y, z) of the +-2 cube inside the occupied box, and rows among them that hold no point
    lo, hi = c.min(0), c.max(0)
    rows = np.array([(min(a[1] + 2, hi[1]) - max(a[1] - 2, lo[1]) + 1) * (min(a[2] + 2, hi[2]) - max(a[2] - 2, lo[2]) + 1) for a in c])
    assert rows.min() == 9 and rows.max() == 15 and len(set(rows)) >= 2  # (the lanes beyond the last row scan empty runs)


@pytest.mark.parametrize("m", S.TINY)
def test_tiny_clouds_want_below_ten_and_cubes_that_do_and_do_not_cover_the_box(m):
    f = S.facts("tiny_%d" % m)
    po = f["po"]
    assert len(po) == m and int(f["tie"].sum()) == 0
    ext = _cells(po).max(0) - _cells(po).min(0)
    assert (ext <= [3, 2, 2]).all()
    if m >= 7:
        cov = _covers(po)
        assert cov.any() and not cov.all() and (f["d10"][~cov] > 2 * CELL * (1 + 1e-6)).all()  # those go on to k_knn_cov_far_wg
    if m < 5:
        assert (f["ref"] == np.eye(3)).all()  # fewer than five found: the invalid-normal covariance
