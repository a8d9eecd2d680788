"""Shared by tests/test_knn_row_walk_reference.py (CPU) and tests/test_gpu_knn_row_walk.py (GPU): the clouds on which the row walk of
k_knn_cov (csrc/gicp.hip: KnnRowWalk, knn_search_cube) can go wrong, each at most 4 000 raw points.  Not a test module.  The
brute-force references are those of tests/gicp_geometry_support.py, used as a library.

The kernel searches the voxel means (leaf 0.02) in cells of 0.1; a ROW is the three cells cx - 1, cx, cx + 1 at one (y, z) cell, its
points ordered by slices of 1 / 64 of a cell along x.  A query walks its own row from itself outwards and then every neighbouring
row within its k-th distance from where its x falls among the points of that row's middle cell, four candidates a step."""
import functools

import numpy as np

import gicp_geometry_support as G

SEED = 0
LEAF_DENSE = 0.005  # downsampling_resolution of `dense_cell` (everything else: the default 0.02)
TINY = (1, 4, 5, 9, 10, 11)
NAMES = ("row_patterns", "short_rows", "x_planes", "faces_and_corners", "dense_cell", "wide_extent", "shuffled_reversed",
         "shuffled_random") + tuple("tiny_%d" % m for m in TINY)
BATCHED = ("row_patterns", "short_rows", "x_planes")  # the three that share one batch call with a depth-camera cloud
# clouds whose every k-th distance is within one cell and that have no near tie (pinned by the CPU module): nothing may be deferred
ALL_CERTIFIED = ("short_rows", "x_planes")


def _box(rng, lo, hi, n):
    return rng.uniform(lo, hi, (n, 3))


def _row_patterns(rng):
    """A full row (y, z cell 0, 0; x cells 0 .. 11) hugging the face y = 0.1, and three neighbouring rows with holes: (1, 0) every other
    cell (a query under a hole: middle cell empty, n1 = 0, the start falls on the seam of left and right; under a full cell: the
    middle alone), (0, 1) in pairs (only a left / only a right / left + middle / middle + right cell), (1, 1) one cell in three."""
    parts = [_box(rng, [0, 0.055, 0.045], [1.2, 0.1, 0.1], 150)]
    for cx in range(12):
        x0 = 0.1 * cx
        if cx % 2 == 0:
            parts.append(_box(rng, [x0, 0.1, 0.045], [x0 + 0.1, 0.135, 0.1], 9))
        if cx % 4 < 2:
            parts.append(_box(rng, [x0, 0.055, 0.1], [x0 + 0.1, 0.1, 0.135], 9))
        if cx % 3 == 0:
            parts.append(_box(rng, [x0, 0.1, 0.1], [x0 + 0.1, 0.13, 0.13], 5))
    return np.concatenate(parts)


def _short_rows(rng):
    """A dense row next to rows of exactly 1, 2, 3, 4 and 5 points (every clamp of the four slots; the first and last point of a row
    have one side dead from the first step), the groups three cells apart so that a strip of three cells holds one group."""
    parts = [_box(rng, [0, 0.06, 0.05], [1.6, 0.1, 0.1], 220)]
    for n in range(1, 6):
        x0 = 0.1 + 0.3 * (n - 1)
        parts.append(np.c_[x0 + 0.01 + 0.021 * np.arange(n) + rng.uniform(0, 0.004, n), rng.uniform(0.102, 0.118, n), rng.uniform(0.06, 0.09, n)])
        parts.append(np.c_[x0 + 0.09 - 0.021 * np.arange(n) - rng.uniform(0, 0.004, n), rng.uniform(0.06, 0.09, n), rng.uniform(0.102, 0.118, n)])
    return np.concatenate(parts)


def _x_planes(rng):
    """No stop from the gap in x: a plane x = const through 25 rows whose jitter crosses slices, and one inside a single slice
    (slice 32 of its cell: 0.05 <= x < 0.0515625), both on a 0.021 lattice jittered in y and z."""
    gy, gz = np.meshgrid(np.arange(24), np.arange(24))
    yz = np.stack([gy.ravel() * 0.021, gz.ravel() * 0.021], 1)
    a = np.c_[0.0531 + rng.normal(0, 0.002, len(yz)), yz + rng.normal(0, 0.002, yz.shape)]
    b = np.c_[1.05 + rng.uniform(2e-4, 1.3e-3, len(yz)), yz + rng.normal(0, 0.002, yz.shape)]
    return np.concatenate([a, b])


def _faces_and_corners(rng):
    """Queries exactly on cell faces, edges and corners (coordinates 0 and 0.5: exact in float32, and 10 x exact in double, so u = 0
    and the row below / behind has row2 = 0), and within 1e-12 (at 0) or one float32 step (at 0.5) of them, in a uniform background."""
    parts = []
    for c in (0.0, 0.5):
        parts.append(_box(rng, [c - 0.2] * 3, [c + 0.2] * 3, 900))
        for ax in range(3):  # faces, then edges
            f = _box(rng, [c - 0.2] * 3, [c + 0.2] * 3, 40)
            f[:, ax] = c
            e = _box(rng, [c - 0.2] * 3, [c + 0.2] * 3, 12)
            e[:, ax] = c
            e[:, (ax + 1) % 3] = c
            e[:, (ax + 2) % 3] = c + rng.choice([-1.0, 1.0], 12) * rng.uniform(0.03, 0.2, 12)  # (outside the corner's own voxel)
            parts += [f, e]
        if c:
            parts.append(np.full((1, 3), c))  # the corner itself
    # Within 1e-12 of a corner, an edge and a face at 0 (where float32 resolves it), one float32 step from them at 0.5.  No two
    # points of the cloud are that close to EACH OTHER (so no exact corner at 0): two neighbours whose distances from a query agree
    # to 2^-32 are listed by index in the key list and by distance in the exact passes, and the covariance sum is folded in
    # that order (csrc/gicp.hip, TopKey11) -- with the corner at 0 next to these points one covariance of 1 959 differed in its last
    # bits from the exact passes', on the full-scan kernel before the row walk as well.
    t = rng.uniform(0.5e-12, 1.5e-12, (13, 3)) * rng.choice([-1.0, 1.0], (13, 3))
    t[0] = -np.abs(t[0])                                                     # a corner
    t[1:5, 2] = rng.choice([-1.0, 1.0], 4) * rng.uniform(0.03, 0.2, 4)       # an edge
    t[5:, 1:] = rng.choice([-1.0, 1.0], (8, 2)) * rng.uniform(0.03, 0.2, (8, 2))  # a face
    parts = [p[np.abs(p).max(1) >= 0.02] for p in parts]  # (the eight voxels at the origin hold the near-corner point alone)
    h = np.float64(np.nextafter(np.float32(0.5), np.float32(0))), np.float64(np.nextafter(np.float32(0.5), np.float32(1)))
    near = np.array([[h[0], h[0], h[0]], [h[1], h[0], 0.43], [h[0], 0.57, 0.43], [0.43, h[1], 0.56]])
    return np.concatenate(parts + [t, near])


def _dense_cell(rng):
    """One cell of >= 200 voxel means (leaf 0.005) among cells of 6: lanes of one wave have no surviving neighbour row and eight."""
    return np.concatenate([_box(rng, [0.1, 0.1, 0.1], [0.2, 0.2, 0.2], 320), _box(rng, [-0.1, -0.1, -0.1], [0.4, 0.4, 0.4], 750)])


def cloud(name):
    """float32 [n, 4] (w = 1), deterministic."""
    rng = np.random.default_rng([91, SEED, sum(map(ord, name.split("_")[0]))])
    if name.startswith("tiny_"):
        return G.cloud(name, SEED)
    if name == "wide_extent":  # the lower_bound_u64 branch of row_cells3 (no dense grid: gi[6] == 0)
        return G.cloud(name, SEED, n=400)
    if name.startswith("shuffled_"):  # the walk may rely on the order of the slices only, not on the order inside a slice
        c = cloud("row_patterns")
        return c[::-1].copy() if name == "shuffled_reversed" else c[np.random.default_rng(5).permutation(len(c))]
    return G._f4({"row_patterns": _row_patterns, "short_rows": _short_rows, "x_planes": _x_planes, "faces_and_corners": _faces_and_corners,
                  "dense_cell": _dense_cell}[name](rng))


def leaf(name):
    return LEAF_DENSE if name == "dense_cell" else None


def config(name, default):
    """The configuration of `name` from `default` (api.gicp_default_config() or oracle.gicp_default_cfg())."""
    if leaf(name) is not None:
        default.downsampling_resolution = leaf(name)
    return default


@functools.lru_cache(maxsize=None)
def facts(name):
    """G.facts_of for the cloud; with another leaf, the same facts from the oracle's preprocessing under that configuration."""
    c = cloud(name)
    if leaf(name) is None:
        return G.facts_of(c)
    from oracle import oracle as O
    po, co, _ = O.gicp_preprocess(c, config(name, O.gicp_default_cfg()))
    co = co[:, :3, :3]
    idx, sq, tie, near = G.brute_knn(po, G.K, True)
    ref, gap = G.reference_cov(po, idx)
    good = (gap > G.GAP_MIN) & ~tie
    return dict(raw=c, po=po, co=co, idx=idx, sq=sq, tie=tie, ref=ref, gap=gap, d10=np.sqrt(sq[:, -1]), good=good,
                d_or_cov=float(np.abs(co - ref).reshape(len(po), -1).max(1)[good].max()) if good.any() else 0.0,
                near_ties=int(near.sum()), cube=G.cube_counts(po), extent=po[:, :3].max(0) - po[:, :3].min(0))


def rows_of(po, cell=G.CELL):
    """(cell coordinates [m, 3], for every point the number of points in the strip cx - 1 .. cx + 1 of its own row)."""
    c = np.floor(np.asarray(po)[:, :3] * (1.0 / cell)).astype(np.int64)
    same = (c[:, None, 1:] == c[None, :, 1:]).all(2) & (np.abs(c[:, None, 0] - c[None, :, 0]) <= 1)
    return c, same.sum(1)
