"""CPU half of tests/test_gpu_knn_row_walk.py: pins, for the reference alone, the caps that the GPU test rests on and the shapes the
clouds of tests/knn_row_walk_support.py are built to have (as tests/test_gicp_geometry_reference.py does for its clouds).  Caps:
  raw points                                               <= 4 000 per cloud
  exact ties between the 10th and 11th squared distance    0 per cloud
  points with relative eigen-gap <= 1e-3                   <= 5 % of a cloud
  d_or_cov = max |oracle cov - reference_cov| (gap > 1e-3) <= 1e-9
  ALL_CERTIFIED clouds                                     every k-th distance within one cell, no near tie"""
import numpy as np
import pytest

import gicp_geometry_support as G
import knn_row_walk_support as W


@pytest.mark.parametrize("name", W.NAMES)
def test_caps_hold_for_the_reference_alone(oracle, name):
    c = W.cloud(name)
    assert c.dtype == np.float32 and c.shape[1] == 4 and len(c) <= 4000 and np.array_equal(c, W.cloud(name)) and np.isfinite(c).all()
    f = W.facts(name)
    m = len(f["po"])
    bad = int((f["gap"] <= G.GAP_MIN).sum())
    pc = G.path_counts(f)
    print(f"{name}: raw {len(c)} m {m} ties {int(f['tie'].sum())} gap<=1e-3 {bad} d_or_cov {f['d_or_cov']:.2e} {pc}")
    assert int(f["tie"].sum()) == 0
    assert bad <= 0.05 * m
    assert f["d_or_cov"] <= 1e-9
    assert not (np.abs(f["d10"] - G.CELL) <= 1e-9 * G.CELL).any()
    if name in W.ALL_CERTIFIED:
        assert pc["beyond_cell"] == 0 and pc["near_ties"] == 0
    if name.startswith("tiny_"):
        assert m == int(name[5:])
    else:
        assert pc["within_cell"] - pc["near_ties"] >= 0.5 * m  # the walk, not the deferred passes, answers most of the cloud


def _strip_counts(f, dy, dz):
    """For every point: points in the cells cx - 1, cx, cx + 1 of the row (cy + dy, cz + dz)."""
    c, _ = W.rows_of(f["po"])
    key = {}
    for x, y, z in c:
        key[(x, y, z)] = key.get((x, y, z), 0) + 1
    return np.array([[key.get((x + k, y + dy, z + dz), 0) for k in (-1, 0, 1)] for x, y, z in c])


def test_row_patterns_has_every_combination_of_empty_cells():
    f = W.facts("row_patterns")
    seen = set()
    for dy, dz in ((1, 0), (0, 1), (1, 1), (-1, 0), (0, -1)):
        seen |= {tuple(r) for r in (_strip_counts(f, dy, dz) > 0).tolist()}
    print(sorted(seen))
    # middle cell empty between two full ones; only left; only right; middle alone; all three
    for want in ((True, False, True), (True, False, False), (False, False, True), (False, True, False), (True, True, True)):
        assert want in seen, want


def test_short_rows_have_one_to_five_points():
    f = W.facts("short_rows")
    _, own = W.rows_of(f["po"])
    assert set(range(1, 6)) <= set(own.tolist()), sorted(set(own.tolist()))
    nb = _strip_counts(f, 1, 0).sum(1)
    assert set(range(1, 6)) <= set(nb.tolist()), sorted(set(nb.tolist()))


def test_x_planes_stay_inside_their_cell_and_slice():
    po = W.facts("x_planes")["po"]
    a, b = po[po[:, 0] < 0.5], po[po[:, 0] > 0.5]
    assert len(a) > 400 and len(b) > 400
    assert (np.floor(a[:, 0] * 10) == 0).all() and len(np.unique(np.floor(a[:, 0] * 640))) >= 3  # one cell, several slices
    assert (np.floor(b[:, 0] * 640) == 10 * 64 + 32).all()                                        # one slice
    assert len(np.unique(np.floor(po[:, 1:3] * 10), axis=0)) >= 25                                # 25 rows


def test_faces_and_corners_keep_queries_with_u_zero():
    po = W.facts("faces_and_corners")["po"][:, :3]
    u = po * 10.0 - np.floor(po * 10.0)
    on = u == 0.0
    print("on a face per axis", on.sum(0).tolist(), "edges", int((on.sum(1) == 2).sum()), "corners", int(on.all(1).sum()))
    assert (on.sum(0) >= 40).all() and (on.sum(1) == 2).sum() >= 20 and on.all(1).sum() >= 1
    close = (np.abs(po) < 2e-12) & (po != 0)                                         # within 1e-12 of a face at 0, not on it
    assert close.all(1).sum() >= 1 and (close.sum(1) == 2).sum() >= 3 and (close.sum(1) == 1).sum() >= 3  # corner, edges, faces
    f = W.facts("faces_and_corners")  # no two neighbours of any query closer to each other than the keys resolve (see the support module)
    assert not ((f["sq"][:, 2:] - f["sq"][:, 1:-1]) <= 2.0 ** -31 * f["sq"][:, 2:]).any()
    assert ((u > 1 - 1e-6) | ((u > 0) & (u < 1e-6))).any(1).sum() >= 8            # one float32 step from a face


def test_dense_cell_holds_200_means_next_to_sparse_cells():
    f = W.facts("dense_cell")
    c, _ = W.rows_of(f["po"])
    _, n = np.unique(c, axis=0, return_counts=True)
    print("points a cell: max", n.max(), "median", int(np.median(n)))
    assert n.max() >= 200 and np.median(n) <= 10


def test_wide_extent_has_no_dense_grid():
    po = W.facts("wide_extent")["po"]
    ext = np.ceil((po[:, :3].max(0) - po[:, :3].min(0)) / G.CELL)
    assert ext.prod() > 2 ** 24  # far beyond any dense grid of cells: the sorted-cell look-up (lower_bound_u64) answers


def test_shuffled_clouds_hold_the_same_points():
    a, b, c = (W.facts(n)["po"] for n in ("row_patterns", "shuffled_reversed", "shuffled_random"))
    assert len(a) == len(b) == len(c)
    for x in (b, c):
        assert np.array_equal(a[G.lexorder(a)], x[G.lexorder(x)])
    r = W.cloud("row_patterns")
    assert np.array_equal(W.cloud("shuffled_reversed"), r[::-1]) and not np.array_equal(W.cloud("shuffled_random"), r)
