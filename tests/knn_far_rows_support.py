"""Shared by tests/test_knn_far_rows_reference.py (CPU), tests/test_gpu_knn_far_rows.py (GPU) and tools/record_knn_far_rows_parent.py:
the clouds on which the deferred 10-NN passes of csrc/gicp.hip can go wrong -- k_knn_cov_far (rows of the r = 2 cube, survivors
ranked by counting), k_knn_cov_far_wg and k_knn_cov_settle -- each at most 2 048 points, and the one way all three run them.  Not a
test module.  The brute-force references are those of tests/gicp_geometry_support.py, used as a library.

The kernels search the voxel means (leaf 0.02) in cells of 0.1.  The r = 2 pass probes the cube of +-2 cells around the query's cell,
clamped to the occupied box: at most 25 rows (y, z) of up to five cells.  A query is UNBOUNDED when its 27-cell cube holds fewer than
ten points (every candidate of the probe survives) and BOUNDED otherwise (the candidates within the k-th distance of the 27 cells).

  shell_blob   six points in one cell and, two cells away on the diagonal of x and y, a lattice of 300: the six are unbounded, 306
               candidates survive (several times any survivor list), the 10th neighbour is in the blob within two cells.
  tie_shell    coordinates in multiples of 2^-6 m (differences, squares and sums are exact): a query with eight more points near it
               (nine in its 27 cells: unbounded, and its 10th neighbour is in the shell) and, between 1 and 2 cells away, TIE_MIN or
               more points at ONE squared distance TIE_N / 4096, then FILL_MIN or more at FILL_N / 4096: the 10th neighbour is the
               tied point of the lowest index, and the survivors exceed a list of 64.
  box_corner   a jittered cubic lattice of step 0.115 in a box of 0.6 x 0.6 x 0.3 m (6 x 6 x 3 points): the 10th neighbour of a
               point inside, on a face or on an edge is step * sqrt(2) = 0.163 m away -- beyond the 1.5 cells k_knn_cov can certify
               at most, within the 2 cells of the r = 2 pass -- and that of a corner 2 steps = 0.23 m: every query is deferred, the
               eight corners go on to the third pass; probes are clamped at corners and edges (9 to 15 rows of 25, some empty).
               (A lattice of 0.07 - 0.09 m has its 10th neighbours at 0.10 - 0.13 m, 0.18 m at a corner: most queries would be
               certified by k_knn_cov and none would leave the r = 2 pass, so the step is the smallest that defers every query.)
  tiny_<m>     m = 1, 4, 7, 12 points in 0.38 x 0.28 x 0.28 m (4 x 3 x 3 cells): fewer than five found (the invalid-normal
               covariance), want = m < 10, and the cube of a query in the outer x cells does not cover the box while the others' does.
"""
import functools
import os

import numpy as np

import gicp_geometry_support as G

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "knn_far_rows_parent.npz")
MAX_POINTS = 2048
TINY = (1, 4, 7, 12)
NAMES = ("shell_blob", "tie_shell", "box_corner") + tuple("tiny_%d" % m for m in TINY)
BATCH = NAMES + ("empty",)  # one ragged call: every cloud and an empty one
PATHS = ("default", "exact")  # exact: GFS_GICP_KNN_EXACT=1, every query through the deferred passes
U = 2.0 ** -6               # tie_shell's unit
TIE_Q = (3, 3, 3)           # its query, in units: the middle of cell (0, 0, 0)
TIE_N, FILL_N = 117, 125    # squared distances (units^2) of the tied points and of the filler behind them
TIE_MIN, FILL_MIN = 24, 40
LEAF = 0.02


def _f4(xyz):
    xyz = np.asarray(xyz, np.float64)
    return np.ascontiguousarray(np.c_[xyz, np.ones(len(xyz))], np.float32)


def _own_voxels(p):
    """The points of p (float64 [n, 3]) that do not fall into the voxel (leaf 0.02) of an earlier one."""
    v = np.floor(np.asarray(p, np.float32).astype(np.float64) * (1.0 / LEAF)).astype(np.int64)
    _, first = np.unique(v, axis=0, return_index=True)
    return p[np.sort(first)]


def _shell(n2):
    """Integer offsets (units) of squared length n2 that lie outside the query's 27 cells and inside its r = 2 cube: the query is at
    unit 3 of a cell of 6.4 units, so offsets -9 .. 9 are within one cell of its own and -15 .. 16 within two."""
    r = np.arange(-15, 17)
    o = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    return o[((o * o).sum(1) == n2) & (np.abs(o).max(1) >= 10)]


def _tie_shell():
    near = np.array([[0, 0, 0], [1, 2, 0], [-2, 1, 1], [0, -3, 2], [3, 1, -2], [-1, -2, -4], [2, 3, 3], [-3, 3, -1], [4, -1, 1]])
    assert len(set((near * near).sum(1))) == len(near)  # nine distinct distances, the query first
    return _own_voxels((np.concatenate([near, _shell(TIE_N), _shell(FILL_N)]) + np.array(TIE_Q)) * U)


def _shell_blob(rng):
    own = np.array([[0.09, 0.09, 0.05], [0.07, 0.09, 0.03], [0.09, 0.07, 0.07], [0.07, 0.07, 0.05], [0.09, 0.09, 0.01], [0.07, 0.09, 0.09]])
    i, j, k = (g.ravel() for g in np.meshgrid(np.arange(5), np.arange(5), np.arange(12), indexing="ij"))
    blob = np.c_[0.2005 + 0.021 * i, 0.2005 + 0.021 * j, -0.1995 + 0.021 * k]  # x, y in cell 2; z over cells -2 .. 0
    return np.concatenate([own + rng.uniform(0, 0.003, own.shape), blob + rng.uniform(0, 0.0005, blob.shape)])


def _box_corner(rng):
    i, j, k = (g.ravel() for g in np.meshgrid(np.arange(6), np.arange(6), np.arange(3), indexing="ij"))
    return np.c_[i, j, k] * 0.115 + 0.01 + rng.uniform(-0.004, 0.004, (len(i), 3))


def _tiny(rng, m):
    return _own_voxels(rng.uniform([0.01, 0.01, 2.01], [0.39, 0.29, 2.29], (m, 3)))


def cloud(name):
    """float32 [n, 4] (w = 1), deterministic."""
    rng = np.random.default_rng([93, sum(map(ord, name))])
    if name == "empty":
        return np.zeros((0, 4), np.float32)
    if name.startswith("tiny_"):
        return _f4(_tiny(rng, int(name[5:])))
    return _f4({"shell_blob": _shell_blob, "tie_shell": lambda r: _tie_shell(), "box_corner": _box_corner}[name](rng))


@functools.lru_cache(maxsize=None)
def facts(name):
    """G.facts_of for the cloud (the oracle's preprocessing, brute-force neighbours, reference covariances)."""
    return G.facts_of(cloud(name))


def order_list(pts, k=G.K):
    """[m, min(k, m)] neighbour indices of every point of pts (float64 [m, >= 3], the order the device holds them in) by (exact squared
    distance in the kernels' expression, then the lower index)."""
    idx, _, _ = G.brute_knn(pts, k)
    return idx


def cov6(cov):
    """[m, 3, 3] as api.RegistrationGICP.preprocessed returns it -> [m, 6] = (xx, xy, xz, yy, yz, zz); the matrices must be symmetric."""
    cov = np.asarray(cov, np.float64)
    assert cov.transpose(0, 2, 1).tobytes() == cov.tobytes()
    return np.ascontiguousarray(np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1))


def _cfg(api):
    cfg = api.gicp_default_config()
    cfg.max_iterations = 1
    return cfg


def _entry(reg, b, which):
    pts, cov = reg.preprocessed(b, which)
    stats, dnext = reg.knn_stats(b, which, cap=MAX_POINTS)
    return dict(pts=pts, cov=cov6(cov) if len(cov) else np.zeros((0, 6)), stats=stats.astype(np.int64), dnext=np.sort(dnext))


def run_single(api, clouds):
    """{name: dict(pts, cov [m, 6], stats [3], dnext sorted)} of every cloud alone through one handle."""
    reg = api.RegistrationGICP(max_points=MAX_POINTS)
    out = {}
    for name in NAMES:
        reg.RegisterPointClouds(clouds[name], clouds[name], None, _cfg(api))
        out[name] = _entry(reg, 0, 0)
    reg.close()
    return out


def run_batch(api, clouds, hip):
    """One align_batch_device call of BATCH (targets) against BATCH rolled by one (sources), then one align_next_batch_device call
    with BATCH rolled by two as the new sources -> (first [B] of (target entry, source entry), after [B] of the same): `after`'s
    targets are the first call's sources, kept on the device.  hip: tests/test_gpu_gms.py's _Hip."""
    B = len(BATCH)

    def pack(shift):
        c, n = np.zeros((B, MAX_POINTS, 4), np.float32), np.zeros(B, np.int32)
        for b in range(B):
            x = clouds[BATCH[(b + shift) % B]]
            c[b, :len(x)], n[b] = x, len(x)
        return [hip.to_device(a) for a in (c, n)]

    t, s, s2 = pack(0), pack(1), pack(2)
    reg = api.RegistrationGICP(max_points=MAX_POINTS, max_batch=B)
    reg.align_batch_device(t[0], t[1], s[0], s[1], B, MAX_POINTS, cfg=_cfg(api))
    first = [(_entry(reg, b, 0), _entry(reg, b, 1)) for b in range(B)]
    reg.align_next_batch_device(s2[0], s2[1], B, MAX_POINTS, cfg=_cfg(api))
    after = [(_entry(reg, b, 0), _entry(reg, b, 1)) for b in range(B)]
    reg.close()
    return first, after


def run_all(api, clouds, hip):
    """{path: dict(single={name: entry}, first=[...], after=[...])}, once on the default path and once under GFS_GICP_KNN_EXACT=1."""
    assert "GFS_GICP_KNN_EXACT" not in os.environ and "GFS_GICP_CELL" not in os.environ
    out = {}
    for path in PATHS:
        if path == "exact":
            os.environ["GFS_GICP_KNN_EXACT"] = "1"
        try:
            first, after = run_batch(api, clouds, hip)
            out[path] = dict(single=run_single(api, clouds), first=first, after=after)
        finally:
            os.environ.pop("GFS_GICP_KNN_EXACT", None)
    return out


def same_entry(a, b):
    """None, or what differs between two entries (bits of points and covariances, counts, sorted bounds)."""
    for k in ("pts", "cov", "dnext"):
        x, y = np.ascontiguousarray(a[k], np.float64), np.ascontiguousarray(b[k], np.float64)
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            return k
    return None if np.array_equal(a["stats"], b["stats"]) else "stats %s %s" % (a["stats"], b["stats"])


def batch_differences(run):
    """[(what, which part)] where one path's batch calls differ from its single calls: in the first call slot b holds BATCH[b] as the
    target and BATCH[b + 1] as the source; after the streaming call the targets are those sources, kept on the device (k_knn_cov_settle
    and the passes before it honour `only`), and the sources BATCH[b + 2]."""
    B, single, out = len(BATCH), dict(run["single"], empty=None), []
    for b in range(B):
        for what, got, name in (("first target", run["first"][b][0], BATCH[b]), ("first source", run["first"][b][1], BATCH[(b + 1) % B]),
                                ("kept target", run["after"][b][0], BATCH[(b + 1) % B]), ("next source", run["after"][b][1], BATCH[(b + 2) % B])):
            if name == "empty":
                if len(got["pts"]) or got["stats"].any():
                    out.append(("%s %d %s" % (what, b, name), "not empty"))
                continue
            d = same_entry(got, single[name])
            if what == "kept target" and d is None:  # ... and nothing has touched the slot since the first call
                d = same_entry(got, run["first"][b][1])
            if d is not None:
                out.append(("%s %d %s" % (what, b, name), d))
    return out


def load():
    """-> (clouds {name: float32 [n, 4]}, golden {(path, name): dict(cov, stats, dnext)}, the commit the recording was made on)."""
    z = np.load(FIXTURE)
    clouds = {n: np.ascontiguousarray(np.c_[z["cloud/" + n], np.ones(len(z["cloud/" + n]), np.float32)], np.float32).reshape(-1, 4)
              for n in BATCH}
    golden = {(p, n): dict(cov=z["cov/%s/%s" % (p, n)], stats=z["stats/%s/%s" % (p, n)], dnext=z["dnext/%s/%s" % (p, n)])
              for p in PATHS for n in NAMES}
    return clouds, golden, str(z["parent_commit"])
