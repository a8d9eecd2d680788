"""Shared by tests/test_gicp_geometry_reference.py, tests/test_gpu_gicp_geometry.py and tests/fuzz_gpu.py section 8: point clouds the
GICP neighbour searches were NOT tuned on (every other cloud of the suite is a depth-camera raster) and brute-force numpy references
that share nothing with the kernels (cell grid, key merge) or with the oracle's KdTree.  Not a test module.

References are written from the formulas of small_gicp: util/normal_estimation.hpp:66-92 (covariance of the k nearest, eigenvector of
the smallest eigenvalue, cov = V diag(1e-3, 1, 1) V^T), factors/gicp_factor.hpp:35-73 (one GICP linearisation)."""
import functools

import numpy as np

K = 10              # registration_helper.cpp:60-61 num_neighbors
CELL = 0.1          # the kernels' search cell = max_correspondence_distance (csrc/gicp.hip prm.cell)
MAX_DIST = 0.1      # max_correspondence_distance
GAP_MIN = 1e-3      # relative eigen-gap (l1 - l0) / l2 below which the plane normal is not defined by the data
TINY = (1, 4, 5, 9, 10, 11, 12)
NAMES = ("sparse_uniform", "medium_uniform", "density_gradient", "clusters_and_loners", "wall_and_cell_faces", "ribbon", "line",
         "far_from_origin", "dense_blob", "wide_extent") + tuple("tiny_%d" % m for m in TINY)
SEEDS = (0,)        # what the GPU tests run; the CPU module pins the caps for exactly these
LD = np.longdouble


def _f4(xyz):
    xyz = np.asarray(xyz, np.float32)
    return np.concatenate([xyz, np.ones((len(xyz), 1), np.float32)], 1)


def _patch(rng):
    gx, gy = np.meshgrid(np.arange(70), np.arange(50))
    p = np.stack([gx.ravel() * 0.021, gy.ravel() * 0.021, 0.3 * np.sin(gx.ravel() * 0.05) + 0.2 * np.cos(gy.ravel() * 0.07)], 1)
    return p + rng.normal(0, 0.001, p.shape)


def _along_a_line(rng, lateral_a, lateral_b, n=1500, step=0.03):
    t = np.arange(n) * step
    u = np.array([1.0, 0.3, 0.1])
    u /= np.linalg.norm(u)
    a = np.cross(u, [0, 0, 1.0])
    a /= np.linalg.norm(a)
    b = np.cross(u, a)
    return np.array([-20.0, -5, 1.0]) + t[:, None] * u + rng.normal(0, lateral_a, (n, 1)) * a + rng.normal(0, lateral_b, (n, 1)) * b


def cloud(name, seed, **kw):
    """float32 [n, 4] (w = 1), deterministic in (name, seed).  kw overrides a generator's parameters (the fuzzer draws them):
    n (points), scale (lengths), offset (3-vector added last)."""
    rng = np.random.default_rng([77, int(seed), sum(map(ord, name))])
    n, s = kw.get("n"), float(kw.get("scale", 1.0))
    if name == "sparse_uniform":        # < 10 points in almost every 27-cube: unbounded ring doubling, isolated pass
        p = rng.uniform([-3, -2, 0.5], [3, 2, 3.5], (n or 3000, 3))
    elif name == "medium_uniform":      # 10th neighbour at 0.15 - 0.2 m: the r = 2 pass answers most
        p = rng.uniform([-1.25, -0.8, 1.0], [1.25, 0.8, 2.55], (n or 3000, 3))
    elif name == "density_gradient":    # all three passes in one cloud, within one wave
        z = 0.5 * np.exp(rng.uniform(0, np.log(16), n or 6000))
        p = np.c_[rng.uniform(-0.6, 0.6, (len(z), 2)) * z[:, None], z]
    elif name == "clusters_and_loners":  # probes of 10+ rings, whole rows, the clamp to the occupied box
        c = rng.uniform([-4, -3, 1], [4, 3, 6], (40, 3))
        cl = (c[:, None, :] + rng.normal(0, 0.03, (40, (n or 2400) // 40, 3))).reshape(-1, 3)
        p = np.concatenate([cl, rng.uniform([-6, -5, 0.5], [6, 5, 9], (30, 3))])
    elif name == "wall_and_cell_faces":  # points exactly on cell faces (x = float32(k * 0.1f)): fast_floor_d, ux = 0
        gx, gy = np.meshgrid(np.arange(80), np.arange(60))
        wall = np.stack([gx.ravel() * 0.025 - 1.0, gy.ravel() * 0.025 - 0.75, np.full(gx.size, 2.0)], 1) + rng.normal(0, 0.002, (gx.size, 3))
        k = rng.integers(-10, 10, 400)
        face = np.stack([(k.astype(np.float32) * np.float32(0.1)).astype(np.float64), rng.uniform(-0.75, 0.75, 400), 2.0 + rng.uniform(-0.05, 0.05, 400)], 1)
        p = np.concatenate([wall, face])
        s = 1.0                          # (scaling would move the faces off the cell boundaries)
    elif name == "ribbon":              # one occupied row after another, every neighbour along the line, negative coordinates
        p = _along_a_line(rng, 0.006, 0.0005, n or 1500)
    elif name == "line":                # rank-1 neighbourhoods: no plane normal in the data
        p = _along_a_line(rng, 0.0, 0.0, n or 1500) + rng.normal(0, 0.001, (n or 1500, 3))
    elif name == "far_from_origin":     # cancellation in sum_cross - mean * sum
        p = _patch(rng) + np.array([30.0, -20.0, 15.0])
    elif name == "dense_blob":          # ~100 voxel means per cell: long own-row walks
        p = rng.uniform(-0.15, 0.15, (n or 6000, 3)) + np.array([0.05, -0.03, 1.2])
    elif name == "wide_extent":         # occupied box > kGridCap cells: no dense grid, non-compact voxel keys
        p = np.concatenate([rng.uniform([-150, -150, -60], [150, 150, 60], (n or 800, 3)), _patch(rng) + np.array([1.0, 1.0, 2.0])])
    elif name.startswith("tiny_"):      # n < 5: identity; want = m < 10; exactly k and k + 1 points
        p = rng.uniform(-0.5, 0.5, (int(name[5:]), 3)) + [0, 0, 2]
    else:
        raise KeyError(name)
    if s != 1.0:
        ctr = p.mean(0)
        p = (p - ctr) * s + ctr
    return _f4(p + np.asarray(kw.get("offset", (0.0, 0.0, 0.0)), np.float64))


def rotvec(r):
    """Rodrigues' formula."""
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th == 0:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def _about(ctr, R, t):
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = ctr + t - R @ ctr
    return T


def moved(c, seed):
    """(source, init_T, T_true): the cloud under a small rigid motion ABOUT ITS CENTROID (so that a cloud 40 m from the origin keeps
    its correspondences) plus 2 mm noise, with target = T_true * source up to the noise; init_T is T_true a few millimetres and
    0.3 degrees off."""
    rng = np.random.default_rng([78, int(seed), len(c)])
    x = c[:, :3].astype(np.float64)
    ctr = x.mean(0) if len(x) else np.zeros(3)
    Rg, tg = rotvec([0.01, -0.015, 0.008]), np.array([0.02, -0.01, 0.015])
    T_true = _about(ctr, Rg, tg)
    src = c.copy()
    src[:, :3] = ((x - T_true[:3, 3]) @ T_true[:3, :3] + rng.normal(0, 0.002, x.shape)).astype(np.float32)
    init_T = _about(ctr, Rg @ rotvec([0.004, 0.002, -0.003]), tg + np.array([0.003, 0.002, -0.003]))
    return src, init_T, T_true


def _sqdist(q, p):
    d = q[:, None, :] - p[None, :, :]
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]  # the reference's expression (traits: (a - b).squaredNorm())


def _knn(points, k, chunk=256):
    """(idx [n, k1], sqd [n, k1]) with k1 = min(k + 1, n): one more than asked for, so that ties at the k-th place show."""
    p = np.ascontiguousarray(np.asarray(points, np.float64)[:, :3])
    n = len(p)
    k1 = min(k + 1, n)
    idx, sq = np.zeros((n, k1), np.int64), np.zeros((n, k1))
    for a in range(0, n, chunk):
        D = _sqdist(p[a:a + chunk], p)
        o = np.argsort(D, axis=1, kind="stable")[:, :k1]
        idx[a:a + chunk], sq[a:a + chunk] = o, np.take_along_axis(D, o, 1)
    return idx, sq


def brute_knn(points, k, with_near=False):
    """(idx [n, kk], sqd [n, kk], tie [n]) with kk = min(k, n): the kk nearest of every point among the cloud (itself included, as
    the reference's search on its own cloud), ascending, equal distances by index; tie = the k-th and (k+1)-th distance are EQUAL.
    with_near: also the near_ties() mask."""
    idx, sq = _knn(points, k)
    n, kk = len(idx), min(k, len(idx))
    tie = sq[:, k - 1] == sq[:, k] if n > k else np.zeros(n, bool)
    if with_near:
        near = sq[:, k] - sq[:, k - 1] <= KEY_RESOLUTION * sq[:, k - 1] if n > k else np.zeros(n, bool)
        return idx[:, :kk], sq[:, :kk], tie, near
    return idx[:, :kk], sq[:, :kk], tie


KEY_RESOLUTION = 2.0 ** -31


def near_ties(points, k):
    """Number of points whose k-th and (k+1)-th squared distances agree to 2^-31: k_knn_cov's keys (TopKey11: the low 20 of the 52
    mantissa bits hold the point index, so a key is the distance to 2^-32) cannot order those and hand the query to the exact pass.
    2^-31 leaves a factor two for the kernel's own rounding of the distance."""
    return int(brute_knn(points, k, True)[3].sum())


def cube_counts(points, cell=CELL, chunk=1024):
    """Points inside the 27-cell cube around every point's own cell (itself included): below k, the first probe cannot bound the next."""
    c = np.floor(np.asarray(points, np.float64)[:, :3] * (1.0 / cell)).astype(np.int64)
    out = np.zeros(len(c), np.int64)
    for a in range(0, len(c), chunk):
        out[a:a + chunk] = (np.abs(c[a:a + chunk, None, :] - c[None, :, :]).max(2) <= 1).sum(1)
    return out


def reference_cov(points, idx):
    """(cov [n, 3, 3], gap [n]): the scatter of each neighbourhood summed in long double ABOUT ITS MEAN (no cancellation), LAPACK's
    eigh for the plane normal n, cov = I - (1 - 1e-3) n n^T; gap = (l1 - l0) / l2.  Fewer than 5 neighbours: identity, gap 1."""
    p = np.asarray(points, np.float64)[:, :3]
    n, kk = idx.shape
    if kk < 5:
        return np.broadcast_to(np.eye(3), (n, 3, 3)).copy(), np.ones(n)
    S = scatter(p, idx)
    w, V = np.linalg.eigh(S)
    v0 = V[:, :, 0]
    return np.eye(3)[None] - (1 - 1e-3) * v0[:, :, None] * v0[:, None, :], (w[:, 1] - w[:, 0]) / np.maximum(w[:, 2], 1e-300)


def scatter(points, idx):
    """[n, 3, 3] covariance of each neighbourhood about its mean (long double sums, rounded to double at the end)."""
    P = np.asarray(points, np.float64)[:, :3][idx].astype(LD)
    d = P - P.mean(1)[:, None, :]
    return (np.einsum("nki,nkj->nij", d, d) / idx.shape[1]).astype(np.float64)


def closed_form_cov(points, idx, oracle, sel=None):
    """The brute-force neighbour set with the ORACLE'S arithmetic: sums in the reference's order (util/normal_estimation.hpp:66-92,
    neighbours in ascending distance, cov = (sum_cross - mean * sum) / n) and oracle.eig3_direct for the eigenvectors.  For the
    ill-conditioned points, where the normal depends on the eigen solver.  sel: the points wanted (all by default)."""
    p = np.asarray(points, np.float64)[:, :3]
    sel = np.arange(len(p)) if sel is None else np.asarray(sel)
    out = np.zeros((len(sel), 3, 3))
    kk = idx.shape[1]
    for o, i in enumerate(sel):
        if kk < 5:
            out[o] = np.eye(3)
            continue
        sp, sc = np.zeros(3), np.zeros((3, 3))
        for j in idx[i]:
            sp = sp + p[j]
            sc = sc + p[j][:, None] * p[j][None, :]
        cov = (sc - (sp / kk)[:, None] * sp[None, :]) / kk
        _, V = oracle.eig3_direct(cov)
        out[o] = (V * np.array([1e-3, 1.0, 1.0])[None, :]) @ V.T
    return out


def _skew(p):
    z = np.zeros(len(p), p.dtype)
    return np.stack([np.stack([z, -p[:, 2], p[:, 1]], 1), np.stack([p[:, 2], z, -p[:, 0]], 1), np.stack([-p[:, 1], p[:, 0], z], 1)], 1)


def reference_linearize(pt, ct, ps, cs, T, max_dist=MAX_DIST, chunk=256):
    """One GICP linearisation at T (factors/gicp_factor.hpp:35-73) with a brute-force 1-NN of T * source in the target, everything
    after the search in long double: dict(H [6, 6], b [6], error, num_inliers, nn_ties, at_gate).  nn_ties = sources whose nearest
    and second nearest target are equally far, at_gate = nearest distances within 1e-12 of max_dist^2: both must be 0 for the
    inlier count to be defined independently of the search's rounding."""
    pt, ps = np.asarray(pt, np.float64)[:, :3], np.asarray(ps, np.float64)[:, :3]
    ct, cs = np.asarray(ct, np.float64)[:, :3, :3], np.asarray(cs, np.float64)[:, :3, :3]
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    tp = ps @ R.T + t
    n = len(tp)
    nn, d2, d2b = np.zeros(n, np.int64), np.full(n, np.inf), np.full(n, np.inf)
    if len(pt):
        for a in range(0, n, chunk):
            D = _sqdist(tp[a:a + chunk], pt)
            o = np.argsort(D, 1, kind="stable")[:, :2]
            nn[a:a + chunk], d2[a:a + chunk] = o[:, 0], np.take_along_axis(D, o[:, :1], 1)[:, 0]
            if D.shape[1] > 1:
                d2b[a:a + chunk] = np.take_along_axis(D, o[:, 1:2], 1)[:, 0]
    g2 = max_dist * max_dist
    keep = d2 <= g2  # (the reference rejects sq_dist > max_correspondence_distance^2)
    k = nn[keep]
    Rl = R.astype(LD)
    RCR = ct[k].astype(LD) + Rl @ cs[keep].astype(LD) @ Rl.T
    M = np.linalg.inv(RCR.astype(np.float64)).astype(LD) if len(k) else np.zeros((0, 3, 3), LD)
    M = M @ (2 * np.eye(3, dtype=LD) - RCR @ M)  # one Newton step: the inverse to long double precision
    p = ps[keep].astype(LD)
    res = pt[k].astype(LD) - (p @ Rl.T + t.astype(LD))
    J = np.concatenate([Rl @ _skew(p), np.broadcast_to(-Rl, (len(p), 3, 3))], 2)
    H = np.einsum("nij,nik,nkl->jl", J, M, J)
    b = np.einsum("nij,nik,nk->j", J, M, res)
    e = 0.5 * np.einsum("ni,nij,nj->", res, M, res)
    return dict(H=H.astype(np.float64), b=b.astype(np.float64), error=float(e), num_inliers=int(keep.sum()),
                nn_ties=int((keep & (d2 == d2b)).sum()), at_gate=int((np.abs(d2 - g2) < 1e-12).sum()))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def lin_distance(got, ref):
    """The largest of the relative distances of H (Frobenius), b (2-norm) and error from the reference's."""
    e = abs(got["error"] - ref["error"]) / abs(ref["error"]) if ref["error"] else abs(got["error"])
    return max(rel(got["H"], ref["H"]), rel(got["b"], ref["b"]), e)


def lexorder(p):
    return np.lexsort((p[:, 2], p[:, 1], p[:, 0]))


@functools.lru_cache(maxsize=None)
def facts(name, seed, source=False):
    """facts_of(cloud(name, seed)), or of the pair's source moved(cloud)[0]: computed once per process."""
    c = cloud(name, seed)
    return facts_of(moved(c, seed)[0] if source else c)


def facts_of(c):
    """Everything the tests need about one raw cloud that does not involve the GPU: the oracle's preprocessing (voxel means in the
    oracle's order), the brute-force neighbours, the reference covariance and eigen-gaps, d_or_cov, what path_counts needs."""
    from oracle import oracle as O
    po, co, _ = O.gicp_preprocess(c)
    co = co[:, :3, :3]
    m = len(po)
    idx, sq, tie, near = brute_knn(po, K, True)
    ref, gap = reference_cov(po, idx)
    d10 = np.sqrt(sq[:, -1])  # distance to the min(k, m)-th neighbour (the point itself is the first)
    good = (gap > GAP_MIN) & ~tie
    d_or_cov = float(np.abs(co - ref).reshape(m, -1).max(1)[good].max()) if good.any() else 0.0
    return dict(raw=c, po=po, co=co, idx=idx, sq=sq, tie=tie, ref=ref, gap=gap, d10=d10, good=good, d_or_cov=d_or_cov,
                near_ties=int(near.sum()), cube=cube_counts(po), extent=(po[:, :3].max(0) - po[:, :3].min(0)) if m else np.zeros(3))


def path_counts(f):
    """What the kernels cannot avoid, from the true distance d10 to the k-th neighbour (cell 0.1 m): k_knn_cov certifies at most
    reach = 1.5 cells, the r = 2 pass at most 2 cells (unless its cube covers the occupied box: clouds within 0.5 m); and what they
    must manage: d10 <= one cell is certified by k_knn_cov unless the keys cannot order the k-th and (k+1)-th candidate."""
    d10 = f["d10"]
    return dict(m=len(d10), within_cell=int((d10 <= CELL).sum()), beyond_cell=int((d10 > CELL).sum()),
                must_r2=int((d10 > 1.5 * CELL * (1 + 1e-6)).sum()), must_isolated=int((d10 > 2 * CELL * (1 + 1e-6)).sum()),
                unbounded=int((f["cube"] < min(K, len(d10))).sum()), near_ties=f["near_ties"])


@functools.lru_cache(maxsize=None)
def pair_facts(name, seed):
    """The pair (cloud, moved(cloud)): the oracle's one-iteration sums at init_T and reference_linearize on the oracle's preprocessed
    clouds; d_or_lin = their distance."""
    from oracle import oracle as O
    ft = facts(name, seed)
    src, init_T, T_true = moved(ft["raw"], seed)
    pso, cso, _ = O.gicp_preprocess(src)
    cfg = O.gicp_default_cfg()
    cfg.max_iterations = 1
    ro = O.gicp_align(ft["raw"], src, init_T, cfg)
    ref = reference_linearize(ft["po"], ft["co"], pso, cso[:, :3, :3], init_T)
    return dict(target=ft["raw"], source=src, init_T=init_T, T_true=T_true, oracle1=ro, ref=ref,
                d_or_lin=lin_distance(ro, ref) if ref["num_inliers"] else 0.0)
