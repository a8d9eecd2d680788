"""The linear step of one Levenberg-Marquardt trial of the local bundle adjustment -- Dinv, the Schur complement, the reduced solve,
the landmark back-substitution, computeScale -- in np.longdouble, stage by stage, with the rounding bars a float64 implementation has
to meet; the windows of the case list; and the edits of a window's edge lists that make them.

Every stage is handed THE INPUTS THE CODE UNDER TEST HAD at that stage (its own Dinv for the Schur sums, its own Hs / bs for the
solve, its own xp for the back-substitution, ...), so an error made in one stage is not charged to the next, and a defect shows in the
stage that has it.  The bars are elementwise and derived from the length of the sums (u = 2^-53), not measured:

  lambda   bit-equal to 1e-5 * max(|diag Hpp|, |diag Hll|): one multiplication.
  Dinv     max |Dinv (Hll + lambda I) - I| <= 64 u kappa_1(Hll + lambda I) per landmark.  (The kernel inverts by cofactors; a landmark
           with one monocular observation is nearly singular, hence the condition number in the bar.)
  Hs, bs   |Hs - ref| <= (m_ij + 16) u A_ij with A = |Hpp| + lambda + sum_l |B_i| |Dinv_l| |B_j|^T and m_ij the number of landmarks the
           two poses share: a sum of m_ij terms in any order, each a 6 x 3 x 3 x 6 product of a few roundings.  Likewise bs.
  eta      the normwise backward error ||Hs xp - bs|| / (||Hs|| ||xp|| + ||bs||) (infinity norms, evaluated in longdouble) at most
           max(16 eta_numpy, 6F 2^-52), eta_numpy being numpy.linalg.solve's on the same system.
  xp       ||xp - xp_longdouble|| <= kappa_inf(Hs) * (the bar of eta) * ||xp_longdouble||; the worst row is named.
  xl       |xl - ref| <= (6 k_l + 16) u A_l, A_l = |Dinv_l| (|bl| + sum_f |B_f|^T |xp_f|), k_l the free poses that see landmark l: the
           kernel subtracts the 6 k_l products one after the other, then multiplies by Dinv_l.
  scale    |scale - ref| <= (n_terms + 16) u sum |x| (lambda |x| + |b|), n_terms = 6F + 3N.
"""
import numpy as np

from geoflowslam_amd import synth

LD = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(np.longdouble).eps < 2.0 ** -60)
U = LD(2) ** -53
K_SCHUR_CHUNK = 64  # kSchurPts = kSchurMPts of csrc/lba_dev.hpp
_EDGE_KEYS = ("edge_pose", "edge_point", "edge_obs", "edge_inv_sigma2", "edge_stereo")


# ---------------------------------------------------------------------------------------------------------------- windows
def window(F, n_fixed, N, seed, mono_frac=0.1):
    """synth.lba_window with exactly F free poses: with n_fixed = 0 lba_window pins pose 0, so one more pose is asked for"""
    if n_fixed == 0:
        w = synth.lba_window(seed, n_free=F + 1, n_fixed=0, n_points=N, mono_frac=mono_frac)
    else:
        w = synth.lba_window(seed, n_free=F, n_fixed=n_fixed, n_points=N, mono_frac=mono_frac)
    assert int((w["pose_fixed"] == 0).sum()) == F
    return w


def take_edges(w, idx):
    """the window with the edges idx (a subset, a permutation, ...) in that order"""
    idx = np.asarray(idx)
    w2 = dict(w)
    for k in _EDGE_KEYS:
        w2[k] = np.ascontiguousarray(w[k][idx])
    w2["n_edges"] = len(idx)
    return w2


def with_second_camera_edges(w, seed, frac=0.15):
    """the window with a second edge between some (key-frame, point) pairs, the way a two-camera rig adds a right-camera
    observation of a point the left camera sees too (src/Optimizer.cc:1859-1925): a monocular observation ~0.7 px away"""
    rng = np.random.default_rng(seed)
    E = w["n_edges"]
    pick = np.sort(rng.choice(E, int(frac * E), replace=False))
    w2 = dict(w)
    obs2 = w["edge_obs"][pick].copy()
    obs2[:, :2] += rng.normal(0, 0.7, (len(pick), 2))
    obs2[:, 2] = 0
    # point-major order like the reference builds it: the second edge right after the first
    order = np.argsort(np.r_[np.arange(E), pick + 0.5], kind="stable")
    for k, extra in (("edge_pose", w["edge_pose"][pick]), ("edge_point", w["edge_point"][pick]), ("edge_obs", obs2),
                     ("edge_inv_sigma2", w["edge_inv_sigma2"][pick]), ("edge_stereo", np.zeros(len(pick), w["edge_stereo"].dtype))):
        w2[k] = np.ascontiguousarray(np.concatenate([w[k], extra])[order])
    w2["n_edges"] = E + len(pick)
    return w2


def shuffled_edges(w, seed):
    return take_edges(w, np.random.default_rng(seed).permutation(w["n_edges"]))


def isolated_pose(w):
    """a free pose that shares no landmark with any other pose: it keeps every third landmark it sees, alone"""
    free = np.nonzero(w["pose_fixed"] == 0)[0]
    p = free[len(free) // 2]
    own = np.unique(w["edge_point"][w["edge_pose"] == p])[::3]
    assert len(own) >= 2
    is_p, is_own = w["edge_pose"] == p, np.isin(w["edge_point"], own)
    return take_edges(w, np.nonzero(is_p == is_own)[0]), int(p)


def landmark_of_fixed_poses_only(w):
    """a landmark that only fixed poses see: nothing of it enters Hs, and xl = Dinv bl"""
    fixed_edge = w["pose_fixed"][w["edge_pose"]] != 0
    cand = np.unique(w["edge_point"][fixed_edge])
    l = int(cand[len(cand) // 2])
    return take_edges(w, np.nonzero(~((w["edge_point"] == l) & ~fixed_edge))[0]), l


def single_mono_landmark(w):
    """a landmark with ONE monocular observation, by a free pose: Hll has rank 2, Hll + lambda I is ill-conditioned"""
    free_edge = w["pose_fixed"][w["edge_pose"]] == 0
    cand = np.unique(w["edge_point"][free_edge])
    l = int(cand[len(cand) // 3])
    e = int(np.nonzero(free_edge & (w["edge_point"] == l))[0][0])
    w2 = take_edges(w, np.nonzero((w["edge_point"] != l) | (np.arange(w["n_edges"]) == e))[0])
    k = int(np.nonzero(w2["edge_point"] == l)[0][0])
    w2["edge_stereo"] = w2["edge_stereo"].copy()
    w2["edge_obs"] = w2["edge_obs"].copy()
    w2["edge_stereo"][k] = 0
    w2["edge_obs"][k, 2] = -1.0
    return w2, l


def all_poses_fixed(w):
    return dict(w, pose_fixed=np.ones_like(w["pose_fixed"]))


def _structure_cases(F):
    N, s = 40, 300 + F
    base = lambda: window(F, 2, N, s)  # noqa: E731
    return [(f"isolated-pose-F{F}", lambda: isolated_pose(base())[0]),
            (f"fixed-only-landmark-F{F}", lambda: landmark_of_fixed_poses_only(base())[0]),
            (f"single-mono-landmark-F{F}", lambda: single_mono_landmark(base())[0]),
            (f"all-mono-F{F}", lambda: window(F, 2, N, s + 1, mono_frac=1.0)),
            (f"second-camera-F{F}", lambda: with_second_camera_edges(base(), s)),
            (f"shuffled-edges-F{F}", lambda: shuffled_edges(base(), s)),
            (f"all-fixed-P{F}", lambda: all_poses_fixed(base()))]


def _size_cases():
    out = []
    # free poses: 1, 2 smallest; 21 | 22: one 128 x 128 block of the matrix-core Schur kernel | two, the last partial; 30 | 31: the
    # reduced system factored in LDS | in HBM; 42 | 43: two | three block rows.  Few landmarks; with and without fixed poses.
    for F in (1, 2, 21, 22, 30, 31, 42, 43):
        for n_fixed in (0, 2):
            out.append((f"F{F}-fixed{n_fixed}-N20", lambda F=F, x=n_fixed: window(F, x, 20, 100 + 2 * F + x)))
    # landmarks: around kSchurSub = 8 staged at a time, around the chunk of 64, and 129 = two chunks + a partial one
    for N in (7, 8, 9, 63, 64, 65, 129):
        out.append((f"F3-fixed2-N{N}", lambda N=N: window(3, 2, N, 200 + N)))
    for N in (65, 129):  # ... and several chunks under two 128 x 128 blocks
        out.append((f"F22-fixed2-N{N}", lambda N=N: window(22, 2, N, 250 + N)))
    return out


STRUCTURE_CASES = _structure_cases(6) + _structure_cases(22)
CASES = _size_cases() + STRUCTURE_CASES
# what runs again under each of the two vector Schur kernels (GFS_LBA_SCHUR = chunks | pairs)
KNOB_CASES = STRUCTURE_CASES + [(f"F{F}-fixed2-N70", lambda F=F: window(F, 2, 70, 400 + F)) for F in (2, 22, 31)]


def case(name, cases=None):
    return dict(cases or CASES + KNOB_CASES)[name]()


# ------------------------------------------------------------------------------------------------------ the window's structure
def structure(w):
    """free slots, and which free pose sees which landmark"""
    fixed = np.asarray(w["pose_fixed"]) != 0
    free_index = np.where(~fixed, np.cumsum(~fixed) - 1, -1)
    F, N = int((~fixed).sum()), int(w["n_points"])
    ef, el = free_index[w["edge_pose"]], np.asarray(w["edge_point"])
    seen = np.zeros((F, N), bool)
    seen[ef[ef >= 0], el[ef >= 0]] = True
    return dict(F=F, N=N, free_index=free_index, free_pose=np.nonzero(~fixed)[0], edge_free=ef, edge_point=el, seen=seen,
                shared=seen.astype(np.int64) @ seen.astype(np.int64).T)


def fold_blocks(Hpl, st):
    """B [F, N, 6, 3]: the per-edge blocks of linearize() summed per (free pose, landmark) pair, as g2o keeps ONE block a vertex pair
    (core/block_solver.hpp:143-295).  In float64 and in landmark-major edge order: the build kernel's own sum, so B is the input the
    Schur and back-substitution kernels had."""
    B = np.zeros((st["F"], st["N"], 6, 3))
    for e in np.argsort(st["edge_point"], kind="stable"):
        f = st["edge_free"][e]
        if f >= 0:
            B[f, st["edge_point"][e]] += Hpl[e]
    return B


def unpack_lower(packed, n):
    """packed lower triangle, row by row -> the full symmetric matrix"""
    H = np.zeros((n, n), np.asarray(packed).dtype)
    i, j = np.tril_indices(n)
    H[i, j] = packed
    H[j, i] = packed
    return H


def pack_lower(H):
    i, j = np.tril_indices(len(H))
    return np.ascontiguousarray(H[i, j])


def sym6_to_33(d6):
    d6 = np.asarray(d6)
    return d6[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)


def sym33_to_6(d):
    return np.ascontiguousarray(np.asarray(d).reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]])


# ------------------------------------------------------------------------------------------------------------ the stages
def lambda_ref(Hpp, Hll):
    """computeLambdaInit, tau = 1e-5, in float64: the one multiplication the kernel does"""
    d = [np.abs(np.einsum("fii->fi", np.asarray(Hpp, np.float64))).ravel(), np.abs(np.einsum("lii->li", np.asarray(Hll, np.float64))).ravel()]
    return np.float64(1e-5) * np.float64(max([v.max() for v in d if v.size] + [0.0]))


def dinv_ref(Hll, lam):
    """-> ((Hll + lambda I)^-1 [N, 3, 3] in longdouble, kappa_1 of Hll + lambda I [N])"""
    M = np.asarray(Hll, LD).reshape(-1, 3, 3) + LD(lam) * np.eye(3, dtype=LD)
    a, b, c, d, e, f = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]
    c00, c01, c02 = d * f - e * e, c * e - b * f, b * e - c * d
    det = a * c00 + b * c01 + c * c02
    inv6 = np.stack([c00, c01, c02, a * f - c * c, b * c - a * e, a * d - b * b], 1) / det[:, None]
    inv = sym6_to_33(inv6)
    # one Newton step X <- X (2 I - M X) in longdouble: the cofactor form loses kappa * 2^-64, the step squares what is left
    inv = inv @ (2 * np.eye(3, dtype=LD) - M @ inv)
    inv = (inv + inv.transpose(0, 2, 1)) / 2
    kappa = np.abs(M).sum(1).max(1) * np.abs(inv).sum(1).max(1)
    return inv, kappa


def dinv_residual(Dinv6, Hll, lam):
    """-> (max |Dinv M - I| per landmark, its bar 64 u kappa_1(M))"""
    M = np.asarray(Hll, LD).reshape(-1, 3, 3) + LD(lam) * np.eye(3, dtype=LD)
    _, kappa = dinv_ref(Hll, lam)
    R = sym6_to_33(np.asarray(Dinv6, LD)) @ M - np.eye(3, dtype=LD)
    return np.abs(R).reshape(-1, 9).max(1), 64 * U * kappa


def schur_ref(Hpp, B, Dinv, bp, bl, lam, st):
    """Hs = [i = j](Hpp + lambda I) - sum_l B_i Dinv_l B_j^T, bs = bp - sum_l B_i Dinv_l bl, in longdouble from the given Dinv [N, 3, 3]
    -> (Hs [6F, 6F], its elementwise bar, bs [6F], its bar)"""
    F, N, n = st["F"], st["N"], 6 * st["F"]
    S, A, sb, Ab = np.zeros((n, n), LD), np.zeros((n, n), LD), np.zeros(n, LD), np.zeros(n, LD)
    Dinv, bl = np.asarray(Dinv, LD), np.asarray(bl, LD)
    for l in range(N):
        idx = np.nonzero(st["seen"][:, l])[0]
        if not len(idx):
            continue
        W = np.asarray(B[idx, l], LD)                     # [k, 6, 3]
        WD, aWD = W @ Dinv[l], np.abs(W) @ np.abs(Dinv[l])
        rows = (6 * idx[:, None] + np.arange(6)).ravel()
        k6 = 6 * len(idx)
        S[np.ix_(rows, rows)] += WD.reshape(k6, 3) @ W.reshape(k6, 3).T
        A[np.ix_(rows, rows)] += aWD.reshape(k6, 3) @ np.abs(W).reshape(k6, 3).T
        sb[rows] += WD.reshape(k6, 3) @ bl[l]
        Ab[rows] += aWD.reshape(k6, 3) @ np.abs(bl[l])
    Hs, bs = -S, np.asarray(bp, LD).ravel() - sb
    Ab += np.abs(np.asarray(bp, LD)).ravel()
    for f in range(F):
        s = slice(6 * f, 6 * f + 6)
        Hs[s, s] += np.asarray(Hpp[f], LD) + LD(lam) * np.eye(6, dtype=LD)
        A[s, s] += np.abs(np.asarray(Hpp[f], LD)) + LD(lam) * np.eye(6, dtype=LD)
    m = np.kron(st["shared"], np.ones((6, 6), np.int64)) if F else np.zeros((0, 0), np.int64)
    return Hs, (m + 16) * U * A, bs, (np.diag(m) + 16) * U * Ab


def solve_ld(A, Bm):
    """A X = Bm in longdouble (numpy.linalg has no longdouble): Gaussian elimination with partial pivoting on the system scaled to a
    unit diagonal by powers of two (exact; the systems here are symmetric positive definite with pose and landmark entries of very
    different size, and the scaling takes that out of the condition number), then two steps of iterative refinement"""
    A = np.array(A, LD)
    n = len(A)
    Bm = np.array(Bm, LD).reshape(n, -1)
    if n == 0:
        return Bm
    d = np.abs(np.diag(A))
    s = LD(2) ** -np.round(np.log2(np.where(d > 0, d, 1).astype(np.float64)) / 2)
    As, Bs = A * s[:, None] * s[None, :], Bm * s[:, None]
    M = np.concatenate([As, np.eye(n, dtype=LD)], 1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        if k + 1 < n:
            M[k + 1:, k:] -= np.outer(M[k + 1:, k] / M[k, k], M[k, k:])
    inv = np.zeros((n, n), LD)
    for k in range(n - 1, -1, -1):
        inv[k] = (M[k, n:] - M[k, k + 1:n] @ inv[k + 1:]) / M[k, k]
    X = inv @ Bs
    for _ in range(2):
        X += inv @ (Bs - As @ X)
    return X * s[:, None]


def _inf_norm(M):
    M = np.abs(np.asarray(M, LD))
    return M.sum(1).max() if M.ndim == 2 else M.max()


def backward_error(Hs, bs, x):
    """normwise backward error of x for Hs x = bs, infinity norms, evaluated in longdouble"""
    Hs, bs, x = np.asarray(Hs, LD), np.asarray(bs, LD), np.asarray(x, LD)
    den = _inf_norm(Hs) * _inf_norm(x) + _inf_norm(bs)
    return _inf_norm(Hs @ x - bs) / den if den > 0 else LD(0)


def solve_bars(Hs, bs, xp):
    """the reduced solve against its two bars, from the system the code under test solved (float64 Hs [n, n], bs)
    -> dict(eta, eta_numpy, eta_bar, err, err_bar, worst_row, kappa)"""
    n = len(bs)
    if n == 0:
        z = LD(0)
        return dict(eta=z, eta_numpy=z, eta_bar=z, err=z, err_bar=z, worst_row=-1, kappa=z)
    eta = backward_error(Hs, bs, xp)
    eta_np = backward_error(Hs, bs, np.linalg.solve(np.asarray(Hs, np.float64), np.asarray(bs, np.float64)))
    eta_bar = max(16 * eta_np, n * LD(2) ** -52)
    X = solve_ld(Hs, np.concatenate([np.asarray(bs, LD)[:, None], np.eye(n, dtype=LD)], 1))
    x_ld, inv = X[:, 0], X[:, 1:]
    kappa = _inf_norm(Hs) * _inf_norm(inv)
    d = np.abs(np.asarray(xp, LD) - x_ld)
    return dict(eta=eta, eta_numpy=eta_np, eta_bar=eta_bar, err=d.max(), err_bar=kappa * eta_bar * _inf_norm(x_ld),
                worst_row=int(np.argmax(d)), kappa=kappa, x=x_ld)


def backsub_ref(Dinv, bl, B, xp, st):
    """xl = Dinv (bl - sum over the free poses of B_f^T xp_f) in longdouble -> (xl [N, 3], its elementwise bar)"""
    Dinv, bl, Bl = np.asarray(Dinv, LD), np.asarray(bl, LD), np.asarray(B, LD)
    x = np.asarray(xp, LD).reshape(st["F"], 6)
    cl, acl = bl.copy(), np.abs(bl)
    for f in range(st["F"]):  # (B is zero where pose f does not see the landmark)
        cl -= np.einsum("lac,a->lc", Bl[f], x[f])
        acl += np.einsum("lac,a->lc", np.abs(Bl[f]), np.abs(x[f]))
    xl = np.einsum("lrc,lc->lr", Dinv, cl)
    A = np.einsum("lrc,lc->lr", np.abs(Dinv), acl)
    k = st["seen"].sum(0).astype(np.int64)
    return xl, (6 * k[:, None] + 16) * U * A


def scale_ref(xp, xl, bp, bl, lam):
    """computeScale: sum x (lambda x + b) over the pose and landmark steps -> (the sum in longdouble, its bar)"""
    x = np.concatenate([np.asarray(xp, LD).ravel(), np.asarray(xl, LD).ravel()])
    b = np.concatenate([np.asarray(bp, LD).ravel(), np.asarray(bl, LD).ravel()])
    return (x * (LD(lam) * x + b)).sum(), (len(x) + 16) * U * (np.abs(x) * (LD(lam) * np.abs(x) + np.abs(b))).sum()


def _worst(err, bar):
    """the largest err / bar of an elementwise bar (0 / 0 = 0, x / 0 = inf)"""
    err, bar = np.asarray(err, LD).ravel(), np.asarray(bar, LD).ravel()
    if not err.size:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bar)
    return float(r.max())


def check_step(blocks, st, trial):
    """Every stage of `trial` (dict(lam, Dinv [N, 6], Hs packed, bs, xp, xl, scale): the hook's, or a restatement's) against the
    longdouble reference evaluated from the blocks of linearize() and from the trial's OWN inputs to that stage.
    -> (figs, failed): figs[name] = (measured, allowed), failed = the names whose measured value is above what is allowed."""
    F, N, n = st["F"], st["N"], 6 * st["F"]
    lam = trial["lam"]
    B = fold_blocks(blocks["Hpl"], st)
    figs = {}
    figs["lambda"] = (float(abs(np.float64(lam) - lambda_ref(blocks["Hpp"], blocks["Hll"]))), 0.0)
    res, bar = dinv_residual(trial["Dinv"], blocks["Hll"], lam)
    figs["Dinv"] = (_worst(res, bar), 1.0)
    D33 = sym6_to_33(np.asarray(trial["Dinv"], np.float64))
    Hs_ref, Hs_bar, bs_ref, bs_bar = schur_ref(blocks["Hpp"], B, D33, blocks["bp"], blocks["bl"], lam, st)
    Hs = unpack_lower(np.asarray(trial["Hs"], np.float64), n)
    figs["Hs"] = (_worst(np.abs(Hs - Hs_ref), Hs_bar), 1.0)
    figs["bs"] = (_worst(np.abs(np.asarray(trial["bs"], LD) - bs_ref), bs_bar), 1.0)
    sb = solve_bars(Hs, trial["bs"], trial["xp"])
    figs["eta"] = (float(sb["eta"]), float(sb["eta_bar"]))
    figs["eta_numpy"] = (float(sb["eta_numpy"]), np.inf)  # the yardstick, reported
    figs["xp"] = (float(sb["err"]), float(sb["err_bar"]))
    figs["xp_worst_row"] = (sb["worst_row"], np.inf)
    xl_ref, xl_bar = backsub_ref(D33, blocks["bl"], B, trial["xp"], st)
    figs["xl"] = (_worst(np.abs(np.asarray(trial["xl"], LD) - xl_ref), xl_bar), 1.0)
    sc, sc_bar = scale_ref(trial["xp"], trial["xl"], blocks["bp"], blocks["bl"], lam)
    figs["scale"] = (float(abs(LD(trial["scale"]) - sc)), float(sc_bar))
    failed = [k for k, (v, a) in figs.items() if not v <= a]
    return figs, failed


def unshared_blocks_are_zero(Hs_packed, st):
    """the 6 x 6 blocks of pose pairs without a common landmark hold exact zeros -> the pairs that do not"""
    Hs = unpack_lower(np.asarray(Hs_packed, np.float64), 6 * st["F"])
    return [(i, j) for i in range(st["F"]) for j in range(i) if st["shared"][i, j] == 0 and (Hs[6 * i:6 * i + 6, 6 * j:6 * j + 6] != 0).any()]


# ---------------------------------------------------------------------------------------------- the step tied to the solve
def quat_to_R(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def oplus_mismatch(w, xp, solved, st, se3_exp):
    """VertexSE3Expmap::oplusImpl with se3_exp (the oracle's exponential): exp(xp_f) * pose_f against the solved free poses
    -> the largest absolute difference of the rotation matrices and of the translations relative to 1 + |t|"""
    worst = 0.0
    for f, p in enumerate(st["free_pose"]):
        T = se3_exp(np.asarray(xp, np.float64)[6 * f:6 * f + 6])
        R = T[:3, :3] @ quat_to_R(w["pose_q"][p])
        t = T[:3, :3] @ w["pose_t"][p] + T[:3, 3]
        worst = max(worst, np.abs(quat_to_R(solved["pose_q"][p]) - R).max(),
                    np.abs(solved["pose_t"][p] - t).max() / (1 + np.abs(t).max()))
    return worst
