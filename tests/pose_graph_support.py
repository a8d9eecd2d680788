"""numpy restatement of Optimizer::OptimizeEssentialGraph's numeric core (reference src/Optimizer.cc:2042-2413 on a flattened graph):
g2o's Sim3 arithmetic (Thirdparty/g2o/g2o/types/sim3.h:70-272), VertexSim3Expmap's oplus and EdgeSim3's error
(types_seven_dof_expmap.h:60-69, :106-114), the numeric Jacobians of BaseBinaryEdge (core/base_binary_edge.hpp:147-200), the quadratic
form (:55-90), Levenberg's loop (core/optimization_algorithm_levenberg.cpp:61-168) with the user's first lambda, a dense L D L^T, and
the map-point correction (src/Optimizer.cc:2387-2409).

Everything is vectorised over a leading axis and generic over the dtype: np.float64 is the statement the device is compared with, in
the operation order of geoflowslam_amd/csrc/sim3_dev.hpp (tests/test_pose_graph_restatement.py holds the two bit for bit);
np.longdouble is the same rule at higher precision, which measures how far float64 rounding moves the answer.  A Sim3 is eight numbers:
the quaternion (x, y, z, w), the translation, the scale.  In float64 the libm calls go through math.*, element by element: numpy's own
vector routines need not round like libm.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np

EPS = 0.00001  # sim3.h:90, :165
DELTA = 1e-9   # core/base_binary_edge.hpp:147
BRANCH_SIGMA, BRANCH_ANGLE = 1, 2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "pose_graph_restatement.cpp")
_HDR = os.path.join(ROOT, "geoflowslam_amd", "csrc", "sim3_dev.hpp")
_SO = os.path.join(ROOT, "tests", "host", "_pose_graph_restatement.so")
_L = None


def host():
    """tests/host/pose_graph_restatement.cpp: csrc/sim3_dev.hpp compiled with g++ (built on demand)"""
    global _L
    if _L is None:
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(_SRC), os.path.getmtime(_HDR)):
            tmp = _SO + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", tmp, _SRC], check=True)
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        vp, i = C.c_void_p, C.c_int
        L.pgr_constants.argtypes = [vp]
        L.pgr_exp.argtypes = [i, vp, vp, vp]
        L.pgr_log.argtypes = [i, vp, vp, vp]
        L.pgr_mul.argtypes = [i, vp, vp, vp]
        L.pgr_inverse.argtypes = [i, vp, vp]
        L.pgr_map.argtypes = [i, vp, vp, vp]
        L.pgr_oplus.argtypes = [i, vp, vp, i, vp]
        L.pgr_residual.argtypes = [i, vp, vp, vp, vp, vp]
        L.pgr_jacobians.argtypes = [i, vp, vp, vp, i, vp, vp]
        L.pgr_optimize.argtypes = [vp, vp]
        _L = L
    return _L


def host_call(name, n, *arrays, outs, flag=None):
    """one batch call: inputs as float64 arrays, outs = [(shape, dtype)] -> the outputs"""
    ins = [np.ascontiguousarray(a, np.float64) for a in arrays]
    res = [np.zeros(s, d) for s, d in outs]
    args = [n] + [a.ctypes.data for a in ins] + ([int(flag)] if flag is not None else []) + [r.ctypes.data for r in res]
    getattr(host(), name)(*args)
    return res


def libm(name, x):
    x = np.asarray(x)
    if x.dtype == np.float64:
        f = getattr(math, name)
        return np.array([f(v) for v in x.ravel().tolist()], np.float64).reshape(x.shape)
    return getattr(np, {"acos": "arccos"}.get(name, name))(x)


def quat_rotate(q, v):
    ux = 2 * (q[:, 1] * v[:, 2] - q[:, 2] * v[:, 1])
    uy = 2 * (q[:, 2] * v[:, 0] - q[:, 0] * v[:, 2])
    uz = 2 * (q[:, 0] * v[:, 1] - q[:, 1] * v[:, 0])
    return np.stack([v[:, 0] + q[:, 3] * ux + (q[:, 1] * uz - q[:, 2] * uy),
                     v[:, 1] + q[:, 3] * uy + (q[:, 2] * ux - q[:, 0] * uz),
                     v[:, 2] + q[:, 3] * uz + (q[:, 0] * uy - q[:, 1] * ux)], 1)


def quat_mul(a, b):
    w = a[:, 3] * b[:, 3] - a[:, 0] * b[:, 0] - a[:, 1] * b[:, 1] - a[:, 2] * b[:, 2]
    x = a[:, 3] * b[:, 0] + a[:, 0] * b[:, 3] + a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
    y = a[:, 3] * b[:, 1] + a[:, 1] * b[:, 3] + a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
    z = a[:, 3] * b[:, 2] + a[:, 2] * b[:, 3] + a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return np.stack([x, y, z, w], 1)


def quat_to_R(q):
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
                     1 - (txx + tyy)], 1)


def R_to_quat(m):
    """Quaterniond(R), Eigen 3.4: not normalised"""
    half = m.dtype.type(0.5)
    with np.errstate(all="ignore"):
        tr = m[:, 0] + m[:, 4] + m[:, 8]
        t = np.sqrt(tr + 1)
        k = half / t
        q_pos = np.stack([(m[:, 7] - m[:, 5]) * k, (m[:, 2] - m[:, 6]) * k, (m[:, 3] - m[:, 1]) * k, half * t], 1)
        i = np.where(m[:, 4] > m[:, 0], 1, 0)
        i = np.where(m[:, 8] > np.where(i == 0, m[:, 0], m[:, 4]), 2, i)
        t0 = np.sqrt(m[:, 0] - m[:, 4] - m[:, 8] + 1)
        k0 = half / t0
        q0 = np.stack([half * t0, (m[:, 3] + m[:, 1]) * k0, (m[:, 6] + m[:, 2]) * k0, (m[:, 7] - m[:, 5]) * k0], 1)
        t1 = np.sqrt(m[:, 4] - m[:, 8] - m[:, 0] + 1)
        k1 = half / t1
        q1 = np.stack([(m[:, 1] + m[:, 3]) * k1, half * t1, (m[:, 7] + m[:, 5]) * k1, (m[:, 2] - m[:, 6]) * k1], 1)
        t2 = np.sqrt(m[:, 8] - m[:, 0] - m[:, 4] + 1)
        k2 = half / t2
        q2 = np.stack([(m[:, 2] + m[:, 6]) * k2, (m[:, 5] + m[:, 7]) * k2, half * t2, (m[:, 3] - m[:, 1]) * k2], 1)
    neg = np.where((i == 0)[:, None], q0, np.where((i == 1)[:, None], q1, q2))
    return np.where((tr > 0)[:, None], q_pos, neg)


def skew_and_square(om):
    z = np.zeros_like(om[:, 0])
    O = np.stack([z, -om[:, 2], om[:, 1], om[:, 2], z, -om[:, 0], -om[:, 1], om[:, 0], z], 1)
    O2 = np.stack([O[:, 3 * r] * O[:, c] + O[:, 3 * r + 1] * O[:, 3 + c] + O[:, 3 * r + 2] * O[:, 6 + c] for r in range(3) for c in range(3)], 1)
    return O, O2


def _eye9(like):
    return np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], like.dtype)[None, :]


def w_coefficients(sigma, s, theta, small, sin_t, cos_t):
    """A, B, C of W = A Omega + B Omega^2 + C I (sim3.h:91-135, :168-213); theta is any finite value where `small`"""
    dt = sigma.dtype.type
    with np.errstate(all="ignore"):
        theta2, sigma2 = theta * theta, sigma * sigma
        A00, B00 = np.full_like(sigma, dt(1) / dt(2)), np.full_like(sigma, dt(1) / dt(6))
        A01, B01 = (1 - cos_t) / theta2, (theta - sin_t) / (theta2 * theta)
        C1 = (s - 1) / sigma
        A10, B10 = ((sigma - 1) * s + 1) / sigma2, ((dt(0.5) * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
        a, b = s * sin_t, s * cos_t
        c = theta2 + sigma2
        A11 = (a * sigma + (1 - b) * theta) / (theta * c)
        B11 = (C1 - ((b - 1) * sigma + a * theta) / c) * 1 / theta2
    tiny = np.abs(sigma) < EPS
    A = np.where(tiny, np.where(small, A00, A01), np.where(small, A10, A11))
    B = np.where(tiny, np.where(small, B00, B01), np.where(small, B10, B11))
    C = np.where(tiny, np.ones_like(sigma), C1)
    return A, B, C


def sim3_exp(u):
    """Sim3(const Vector7d&) -> ([N, 8], branch [N])"""
    om, ups, sigma = u[:, 0:3], u[:, 3:6], u[:, 6]
    theta = np.sqrt(om[:, 0] * om[:, 0] + om[:, 1] * om[:, 1] + om[:, 2] * om[:, 2])
    O, O2 = skew_and_square(om)
    s = libm("exp", sigma)
    small = theta < EPS
    sin_t, cos_t = libm("sin", theta), libm("cos", theta)
    A, B, C = w_coefficients(sigma, s, theta, small, sin_t, cos_t)
    I = _eye9(u)
    with np.errstate(all="ignore"):
        ca, cb = sin_t / theta, (1 - cos_t) / (theta * theta)
        R = np.where(small[:, None], I + O + O2, I + ca[:, None] * O + cb[:, None] * O2)
    W = A[:, None] * O + B[:, None] * O2 + C[:, None] * I
    t = np.stack([W[:, 3 * r] * ups[:, 0] + W[:, 3 * r + 1] * ups[:, 1] + W[:, 3 * r + 2] * ups[:, 2] for r in range(3)], 1)
    branch = np.where(np.abs(sigma) < EPS, 0, BRANCH_SIGMA) | np.where(small, 0, BRANCH_ANGLE)
    return np.concatenate([R_to_quat(R), t, s[:, None]], 1), branch


def lu_solve3(W, t):
    """W.lu().solve(t): 3 x 3 partial pivoting (the first largest entry of the column), column-oriented triangular solves"""
    a = [[W[:, 3 * r + c] for c in range(3)] for r in range(3)]
    c = [t[:, 0], t[:, 1], t[:, 2]]

    def swap_rows(cond, r0, r1):
        for k in range(3):
            a[r0][k], a[r1][k] = np.where(cond, a[r1][k], a[r0][k]), np.where(cond, a[r0][k], a[r1][k])
        c[r0], c[r1] = np.where(cond, c[r1], c[r0]), np.where(cond, c[r0], c[r1])

    p = np.where(np.abs(a[1][0]) > np.abs(a[0][0]), 1, 0)
    p = np.where(np.abs(a[2][0]) > np.abs(np.where(p == 0, a[0][0], a[1][0])), 2, p)
    swap_rows(p == 1, 0, 1)
    swap_rows(p == 2, 0, 2)
    a[1][0] = a[1][0] / a[0][0]
    a[2][0] = a[2][0] / a[0][0]
    a[1][1] = a[1][1] - a[1][0] * a[0][1]
    a[1][2] = a[1][2] - a[1][0] * a[0][2]
    a[2][1] = a[2][1] - a[2][0] * a[0][1]
    a[2][2] = a[2][2] - a[2][0] * a[0][2]
    swap_rows(np.abs(a[2][1]) > np.abs(a[1][1]), 1, 2)
    a[2][1] = a[2][1] / a[1][1]
    a[2][2] = a[2][2] - a[2][1] * a[1][2]
    c[1] = c[1] - c[0] * a[1][0]
    c[2] = c[2] - c[0] * a[2][0]
    c[2] = c[2] - c[1] * a[2][1]
    x2 = c[2] / a[2][2]
    c[1] = c[1] - x2 * a[1][2]
    c[0] = c[0] - x2 * a[0][2]
    x1 = c[1] / a[1][1]
    c[0] = c[0] - x1 * a[0][1]
    x0 = c[0] / a[0][0]
    return np.stack([x0, x1, x2], 1)


def sim3_log(S):
    """Sim3::log -> ([N, 7], branch [N])"""
    dt = S.dtype.type
    s = S[:, 7]
    sigma = libm("log", s)
    R = quat_to_R(S[:, 0:4])
    d = dt(0.5) * (R[:, 0] + R[:, 4] + R[:, 8] - 1)
    dR = np.stack([R[:, 7] - R[:, 5], R[:, 2] - R[:, 6], R[:, 3] - R[:, 1]], 1)
    small = d > 1 - EPS
    d_safe = np.where(small, np.zeros_like(d), d)
    theta = np.where(small, np.zeros_like(d), libm("acos", d_safe))
    k = np.where(small, np.full_like(d, dt(0.5)), theta / (2 * np.sqrt(1 - d_safe * d_safe)))
    om = k[:, None] * dR
    th_safe = np.where(small, np.ones_like(d), theta)
    A, B, C = w_coefficients(sigma, s, theta, small, libm("sin", th_safe), libm("cos", th_safe))
    O, _ = skew_and_square(om)
    BO = B[:, None] * O
    BOO = np.stack([BO[:, 3 * r] * O[:, c] + BO[:, 3 * r + 1] * O[:, 3 + c] + BO[:, 3 * r + 2] * O[:, 6 + c] for r in range(3) for c in range(3)], 1)
    W = A[:, None] * O + BOO + C[:, None] * _eye9(S)
    ups = lu_solve3(W, S[:, 4:7])
    branch = np.where(np.abs(sigma) < EPS, 0, BRANCH_SIGMA) | np.where(small, 0, BRANCH_ANGLE)
    return np.concatenate([om, ups, sigma[:, None]], 1), branch


def sim3_mul(a, b):
    q = quat_mul(a[:, 0:4], b[:, 0:4])
    t = a[:, 7:8] * quat_rotate(a[:, 0:4], b[:, 4:7]) + a[:, 4:7]
    return np.concatenate([q, t, (a[:, 7] * b[:, 7])[:, None]], 1)


def sim3_inverse(a):
    dt = a.dtype.type
    q = np.concatenate([-a[:, 0:3], a[:, 3:4]], 1)
    k = dt(-1) / a[:, 7]
    return np.concatenate([q, quat_rotate(q, k[:, None] * a[:, 4:7]), (dt(1) / a[:, 7])[:, None]], 1)


def sim3_map(a, xyz):
    return a[:, 7:8] * quat_rotate(a[:, 0:4], xyz) + a[:, 4:7]


def sim3_oplus(est, update, fix_scale):
    u = np.array(update, est.dtype, copy=True)
    if fix_scale:
        u[:, 6] = 0
    return sim3_mul(sim3_exp(u)[0], est)


def edge_residual(C, v0, v1):
    """EdgeSim3::computeError -> ([N, 7], the log's branch)"""
    return sim3_log(sim3_mul(sim3_mul(C, v0), sim3_inverse(v1)))


def numeric_jacobians(C, v0, v1, fix_scale, delta=DELTA):
    """linearizeOplus -> (Ji, Jj) [N, 7, dim]: central differences through the vertex's oplus, column by column"""
    dt = C.dtype.type
    dim = 6 if fix_scale else 7
    scalar = dt(1) / (2 * dt(delta))
    out = []
    for side in (0, 1):
        J = np.zeros((len(C), 7, dim), C.dtype)
        for d in range(dim):
            add = np.zeros((len(C), 7), C.dtype)
            add[:, d] = dt(delta)
            moved = sim3_oplus(v1 if side else v0, add, fix_scale)
            ep = edge_residual(C, v0 if side else moved, moved if side else v1)[0]
            add[:, d] = -dt(delta)
            moved = sim3_oplus(v1 if side else v0, add, fix_scale)
            em = edge_residual(C, v0 if side else moved, moved if side else v1)[0]
            J[:, :, d] = scalar * (ep - em)
        out.append(J)
    return out


def pack8(q, t, s, dtype):
    return np.concatenate([np.asarray(q, dtype).reshape(-1, 4), np.asarray(t, dtype).reshape(-1, 3), np.asarray(s, dtype).reshape(-1, 1)], 1)


def ldlt_solve(H, b):
    """dense L D L^T without pivoting in H's dtype -> (x, ok): a zero or non-finite pivot fails the solve"""
    A = np.array(H, copy=True)
    n = len(b)
    for c in range(n):
        d = A[c, c]
        if d == 0 or not np.isfinite(d):
            return np.zeros_like(b), False
        w = A[c + 1:, c].copy()
        l = w / d
        A[c + 1:, c] = l
        A[c + 1:, c + 1:] -= np.outer(l, w)
    y = np.array(b, copy=True)
    for c in range(n):
        y[c + 1:] -= A[c + 1:, c] * y[c]
    y = y / np.diag(A)
    for c in range(n - 1, -1, -1):
        y[:c] -= A[c, :c] * y[c]
    return y, True


class PoseGraph:
    """The flattened problem in one dtype, the quantities of one linearisation and the Levenberg loop."""

    def __init__(self, prob, dtype=np.float64):
        self.dt = dtype
        self.fix_scale = bool(prob.get("fix_scale", True))
        self.dim = 6 if self.fix_scale else 7
        self.est = pack8(prob["vertex_q"], prob["vertex_t"], prob["vertex_s"], dtype)
        self.meas = pack8(prob["edge_q"], prob["edge_t"], prob["edge_s"], dtype) if len(prob["edge_i"]) else np.zeros((0, 8), dtype)
        self.ei, self.ej = np.asarray(prob["edge_i"], np.int64), np.asarray(prob["edge_j"], np.int64)
        self.w = np.asarray(prob["edge_w"], dtype)
        fixed = np.asarray(prob["vertex_fixed"]).astype(bool)
        self.free_index = np.where(fixed, -1, np.cumsum(~fixed) - 1)
        self.free_vert = np.nonzero(~fixed)[0]
        self.F = len(self.free_vert)
        self.n = self.dim * self.F

    def errors(self, est):
        """-> (err [E, 7], chi2 [E]): e . (w e), k ascending"""
        if not len(self.ei):
            return np.zeros((0, 7), self.dt), np.zeros(0, self.dt)
        err = edge_residual(self.meas, est[self.ei], est[self.ej])[0]
        chi = np.zeros(len(err), self.dt)
        for k in range(7):
            chi = chi + err[:, k] * (self.w * err[:, k])
        return err, chi

    @staticmethod
    def total(chi):
        t = chi.dtype.type(0)
        for v in chi:  # edge order
            t = t + v
        return t

    def edge_blocks(self, est):
        """constructQuadraticForm with omega = w I -> (Hii, Hij, Hjj [E, dim, dim], bi, bj [E, dim], chi2 [E])"""
        err, chi = self.errors(est)
        E, dim = len(err), self.dim
        if not E:
            z = np.zeros((0, dim, dim), self.dt)
            return z, z, z, np.zeros((0, dim), self.dt), np.zeros((0, dim), self.dt), chi
        A, B = numeric_jacobians(self.meas, est[self.ei], est[self.ej], self.fix_scale)
        omega_r = -(self.w[:, None] * err)
        At, Bt = A * self.w[:, None, None], B * self.w[:, None, None]  # [E, k, a]
        Hii, Hij, Hjj = (np.zeros((E, dim, dim), self.dt) for _ in range(3))
        bi, bj = np.zeros((E, dim), self.dt), np.zeros((E, dim), self.dt)
        for k in range(7):
            Hii = Hii + At[:, k, :, None] * A[:, k, None, :]
            Hij = Hij + At[:, k, :, None] * B[:, k, None, :]
            Hjj = Hjj + Bt[:, k, :, None] * B[:, k, None, :]
            bi = bi + A[:, k, :] * omega_r[:, k, None]
            bj = bj + B[:, k, :] * omega_r[:, k, None]
        return Hii, Hij, Hjj, bi, bj, chi

    def system(self, est):
        """-> (H [n, n] symmetric without lambda, b [n], chi2 [E]): the edges' blocks added in edge order"""
        Hii, Hij, Hjj, bi, bj, chi = self.edge_blocks(est)
        n, dim = self.n, self.dim
        H, b = np.zeros((n, n), self.dt), np.zeros(n, self.dt)
        for e in range(len(self.ei)):
            fi, fj = self.free_index[self.ei[e]], self.free_index[self.ej[e]]
            if fi >= 0:
                H[dim * fi:dim * fi + dim, dim * fi:dim * fi + dim] += Hii[e]
                b[dim * fi:dim * fi + dim] += bi[e]
            if fj >= 0:
                H[dim * fj:dim * fj + dim, dim * fj:dim * fj + dim] += Hjj[e]
                b[dim * fj:dim * fj + dim] += bj[e]
            if fi >= 0 and fj >= 0:
                H[dim * fi:dim * fi + dim, dim * fj:dim * fj + dim] += Hij[e]
                H[dim * fj:dim * fj + dim, dim * fi:dim * fi + dim] += Hij[e].T
        return H, b, chi

    def step(self, est, H, b, lam):
        """one trial: (H + lambda I) x = b, the oplus of every free vertex -> (x, ok, trial estimate, computeScale)"""
        dt = self.dt
        x, ok = ldlt_solve(H + dt(lam) * np.eye(self.n, dtype=dt), b) if self.n else (np.zeros(0, dt), True)
        trial = est.copy()
        scale = dt(0)
        if ok and self.F:
            upd = np.zeros((self.F, 7), dt)
            upd[:, :self.dim] = x.reshape(self.F, self.dim)
            trial[self.free_vert] = sim3_oplus(est[self.free_vert], upd, self.fix_scale)
            for f in range(self.F):  # vertex order, each vertex's terms first
                loc = dt(0)
                for a in range(self.dim):
                    xa = x[self.dim * f + a]
                    loc = loc + xa * (dt(lam) * xa + b[self.dim * f + a])
                scale = scale + loc
        return x, ok, trial, scale

    def optimize(self, iterations=20, lambda_init=1e-16):
        """optimize(iterations) -> dict(est, edge_chi2, iterations_run, final_chi2, final_lambda, trace, alphas, gains); trace: one
        (iteration, accepted, chi2 before, chi2 of the trial) per trial; alphas: per trial 1 - (2 rho - 1)^3 where it was accepted, else
        None; gains: per iteration (chi2 it began with, chi2 it ended with), the two sides of `(ini - current) 1e3 < ini`"""
        dt = self.dt
        est = self.est.copy()
        lam, ni, n_bad, iters = dt(lambda_init), dt(2), 0, 0
        trace, alphas, gains = [], [], []
        last_chi = None
        runs = iterations > 0 and self.F > 0
        for it in range(iterations if runs else 0):
            H, b, chi = self.system(est)
            current = ini = self.total(chi)
            rho, qmax = dt(0), 0
            while True:
                x, ok, trial, scale = self.step(est, H, b, lam)
                temp = self.total(self.errors(trial)[1]) if ok else dt(np.finfo(np.float64).max)
                rho = (current - temp) / (scale + dt(1e-3))
                accepted = bool(rho > 0 and np.isfinite(temp))
                trace.append((it, accepted, current, temp))
                alphas.append(1 - (2 * rho - 1) ** 3 if accepted else None)
                if accepted:
                    alpha = 1 - (2 * rho - 1) ** 3
                    alpha = min(alpha, dt(2) / dt(3))
                    lam = lam * max(dt(1) / dt(3), alpha)
                    ni = dt(2)
                    current = temp
                    est = trial
                else:
                    lam = lam * ni
                    ni = ni * 2
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            iters += 1
            last_chi = current
            gains.append((ini, current))
            if qmax == 10 or rho == 0:
                break
            n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
            if n_bad >= 3:
                break
        chi = self.errors(est)[1]
        return dict(est=est, edge_chi2=chi, iterations_run=iters, final_chi2=last_chi if runs else self.total(chi),
                    final_lambda=lam if runs else dt(0), trace=trace, alphas=alphas, gains=gains)


def correct_points(before, after, points, ref):
    """src/Optimizer.cc:2387-2409 in float64: correctedSwr.map(Srw.map(P)) cast to float; ref < 0 leaves the point"""
    before, after = np.asarray(before, np.float64), np.asarray(after, np.float64)
    pts, ref = np.asarray(points, np.float32), np.asarray(ref, np.int64)
    out = pts.copy()
    m = ref >= 0
    if m.any():
        P = pts[m].astype(np.float64)
        out[m] = sim3_map(sim3_inverse(after[ref[m]]), sim3_map(before[ref[m]], P)).astype(np.float32)
    return out


def relabel(prob, perm):
    """the same graph with vertex v renamed perm[v]; the edges keep their order"""
    perm = np.asarray(perm)
    inv = np.argsort(perm)
    out = dict(prob)
    for k in ("vertex_q", "vertex_t", "vertex_s", "vertex_fixed"):
        out[k] = np.asarray(prob[k])[inv]
    out["edge_i"], out["edge_j"] = perm[np.asarray(prob["edge_i"])], perm[np.asarray(prob["edge_j"])]
    if "point_ref" in prob:
        r = np.asarray(prob["point_ref"])
        out["point_ref"] = np.where(r >= 0, perm[np.maximum(r, 0)], -1)
    return out


# ---- the maps the GPU solves completely (tests/test_pose_graph_oracle_inputs.py holds each to the inputs condition) ----------------
MAPS = {
    "ring10_fixed": dict(seed=4, n_keyframes=10, fix_scale=True, icp_edges=False, drift=0.05),
    "ring10_free_icp": dict(seed=1, n_keyframes=10, fix_scale=False, icp_edges=True, drift=0.01),
    "ring24_fixed_icp": dict(seed=4, n_keyframes=24, fix_scale=True, icp_edges=True, drift=0.05),
    "ring24_free": dict(seed=8, n_keyframes=24, fix_scale=False, icp_edges=False, drift=0.05),
    "ring40_fixed": dict(seed=4, n_keyframes=40, fix_scale=True, icp_edges=False, drift=0.05),
    "ring40_free_icp": dict(seed=21, n_keyframes=40, fix_scale=False, icp_edges=True, drift=0.05),
}
_cache = {}


def map_problem(name):
    from geoflowslam_amd import synth
    if ("p", name) not in _cache:
        _cache[("p", name)] = synth.pose_graph(**MAPS[name])
    return _cache[("p", name)]


def map_solution(name, dtype=np.float64):
    """the restatement's optimize() of a map, computed once"""
    key = ("s", name, np.dtype(dtype).name)
    if key not in _cache:
        p = map_problem(name)
        _cache[key] = PoseGraph(p, dtype).optimize(p["iterations"], p["lambda_init"])
    return _cache[key]


# ---- full solves whose Levenberg decisions are not rounding noise (tests/test_pose_graph_levenberg_inputs.py holds each to its shape
# and its margins on the CPU; tests/test_gpu_pose_graph.py compares iterations, trials and the final lambda on them) -------------------
DECISION_MARGIN = 1e-4  # of chi2: 100 x the 1e-6 relative bar the GPU's final chi2 is held to


def decisions(sol):
    """an optimize() result -> per iteration (accept / reject sequence "rrA", smallest relative margin of its decisions, an accepted
    trial has 1/3 < alpha < 2/3).  The decisions: the sign of current - temp in every trial, relative to current, and
    (ini - current) 1e3 < ini at the iteration's end, relative to ini.  A failed solve or a chi2 that is no number has margin 0."""
    out = []
    for (it, accepted, current, temp), alpha in zip(sol["trace"], sol["alphas"]):
        current, temp = float(current), float(temp)
        margin = abs(current - temp) / abs(current) if np.isfinite(temp) and np.isfinite(current) and current != 0 and temp < 1e300 else 0.0
        if it == len(out):
            out.append(["", np.inf, False])
        out[it][0] += "A" if accepted else "r"
        out[it][1] = min(out[it][1], margin)
        out[it][2] = out[it][2] or (alpha is not None and 1 / 3 < float(alpha) < 2 / 3)
    for row, (ini, current) in zip(out, sol["gains"]):
        ini, current = float(ini), float(current)
        row[1] = min(row[1], abs((ini - current) * 1e3 - ini) / abs(ini) if np.isfinite(ini) and ini != 0 else 0.0)
    return [tuple(r) for r in out]


def _ring10():
    V = 10
    return [1] + [0] * (V - 1), [(i, i - 1) for i in range(1, V)] + [(i, i - 2) for i in range(2, V)] + [(V - 1, 0), (0, V - 2)]


def _far_start_ring(seed):
    """a ring of nine free vertices, fixed scale, consistent measurements, whose estimates start about a radian and two metres away
    from them: far enough from linear for Levenberg to reject steps (synth.pose_graph's fixed-scale maps never do before chi2 has
    converged), and with small residuals at the end, so that the rule's own rounding noise stays small"""
    fixed, edges = _ring10()
    p = random_graph(seed, fixed, edges, True)
    rng = np.random.default_rng(2000 + seed)
    V = len(fixed)
    u = np.concatenate([rng.normal(0, 1.0, (V, 3)), rng.normal(0, 2.0, (V, 3)), np.zeros((V, 1))], 1)
    u[0] = 0
    est = sim3_mul(sim3_exp(u)[0], pack8(p["vertex_q"], p["vertex_t"], p["vertex_s"], np.float64))
    est[:, :4] /= np.linalg.norm(est[:, :4], axis=1)[:, None]
    return dict(p, vertex_q=est[:, :4].copy(), vertex_t=est[:, 4:7].copy())


def _drifted_ring(seed):
    from geoflowslam_amd import synth
    return synth.pose_graph(seed, n_keyframes=10, fix_scale=False, icp_edges=True, drift=0.3)


def _rejected_then_accepted(rows):
    return any("r" in r[0] and r[0].endswith("A") for r in rows)


# name -> (problem of a seed, first lambda, what the decisions must show, the seeds searched, the run ends at qmax == 10)
LEVENBERG_SEARCHES = {
    "rejected_then_accepted_fixed": (_far_start_ring, 1e-6, _rejected_then_accepted, range(0, 200), False),
    "rejected_then_accepted_free": (_drifted_ring, 1.0, _rejected_then_accepted, range(0, 200), False),
    "ends_qmax": (lambda seed: map_problem("ring10_free_icp"), 1e-16,
                  lambda rows: len(rows) > 1 and rows[-1][0] == "r" * 10 and any("A" in r[0] for r in rows[:-1]), range(1), True),
    "unclamped_alpha": (_drifted_ring, 1e-6, lambda rows: any(r[2] for r in rows), range(95, 200), False),  # (of range(200), 95 is the first)
}
INPUTS_BAR = 1e-6  # tests/test_pose_graph_oracle_inputs.py's: float64 and long double agree to this on a map that is a fair test


def levenberg_case(name):
    """The first seed whose float64 run shows what the case is named for within the iterations all of whose decisions hold at
    DECISION_MARGIN, and on which the long-double run takes the same decisions and ends within INPUTS_BAR of the float64 poses.
    `iterations` is the number of those iterations (for ends_qmax: up to the iteration that uses its ten trials), and less than the
    run would go on for, so the run ends by using its iterations up -> (problem, seed), computed once."""
    if ("l", name) not in _cache:
        make, lam, wanted, seeds, at_qmax = LEVENBERG_SEARCHES[name]
        for seed in seeds:
            p = make(seed)
            rows = decisions(PoseGraph(p).optimize(20, lam))
            good = 0
            while good < len(rows) and rows[good][1] >= DECISION_MARGIN:
                good += 1
            # (an iteration that the 20-iteration run went on from did not end it: a run of that many iterations uses them up)
            n = good if at_qmax else min(good, len(rows) - 1)
            if n < 1 or (at_qmax and n != len(rows)) or not wanted(rows[:n]):
                continue
            p = dict(p, iterations=n, lambda_init=lam)
            a, b = PoseGraph(p).optimize(n, lam), PoseGraph(p, np.longdouble).optimize(n, lam)
            if [r[0] for r in decisions(a)] != [r[0] for r in decisions(b)] or max(pose_difference(a["est"], b["est"].astype(np.float64))[:2]) > INPUTS_BAR:
                continue
            _cache[("l", name)] = (p, seed)
            _cache[("ls", name, "float64")], _cache[("ls", name, "longdouble")] = a, b
            break
        else:
            raise AssertionError(f"{name}: no seed gives the wanted decisions")
    return _cache[("l", name)]


def levenberg_solution(name, dtype=np.float64):
    key = ("ls", name, np.dtype(dtype).name)
    if key not in _cache:
        p = levenberg_case(name)[0]
        _cache[key] = PoseGraph(p, dtype).optimize(p["iterations"], p["lambda_init"])
    return _cache[key]


# ---- estimates and measurements that are no numbers (eg_check validates scales and weights only) ---------------------------------
def non_finite_problems():
    """name -> ring10_fixed with one entry replaced: NaN in a free vertex's translation, inf in a measurement's, NaN in the fixed
    vertex's quaternion"""
    p = map_problem("ring10_fixed")
    assert p["vertex_fixed"][0] and not p["vertex_fixed"][4]

    def put(key, index, value):
        a = np.array(p[key], np.float64, copy=True)
        a[index] = value
        return dict(p, **{key: a})
    return {"nan_free_vertex_t": put("vertex_t", (4, 1), np.nan), "inf_edge_t": put("edge_t", (5, 0), np.inf),
            "nan_fixed_vertex_q": put("vertex_q", (0, 2), np.nan)}


def non_finite_solution(name):
    """the float64 restatement's optimize() of one of non_finite_problems(), computed once"""
    if ("n", name) not in _cache:
        p = non_finite_problems()[name]
        with np.errstate(all="ignore"):
            _cache[("n", name)] = PoseGraph(p).optimize(p["iterations"], p["lambda_init"])
    return _cache[("n", name)]


def pose_difference(a, b):
    """(max |dq| after fixing the sign, max |dt|, max |ds|) of two [V, 8] estimates"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    sign = np.where((a[:, :4] * b[:, :4]).sum(1) < 0, -1.0, 1.0)[:, None]
    return float(np.abs(a[:, :4] - sign * b[:, :4]).max()), float(np.abs(a[:, 4:7] - b[:, 4:7]).max()), float(np.abs(a[:, 7] - b[:, 7]).max())


# ---- structure cases shared by the list test (CPU) and the step test (GPU): (fixed, edges) ------------------------------------------
STRUCTURE_CASES = {
    # (every case has a cycle through a fixed vertex: a tree could be solved to a zero residual, and a graph that no fixed vertex
    #  holds has a singular system)
    "chain": ([1, 0, 0, 0], [(1, 0), (2, 1), (3, 2), (3, 0), (2, 0)]),
    "duplicates_both_orientations": ([1, 0, 0, 0], [(1, 0), (1, 2), (2, 1), (1, 2), (3, 1), (1, 3), (2, 1), (3, 0), (0, 2)]),
    "edge_between_fixed": ([1, 1, 0, 0], [(0, 1), (2, 1), (3, 2), (1, 0), (3, 0), (2, 0)]),
    "free_vertex_without_edge": ([1, 0, 0, 0, 0], [(1, 0), (3, 1), (4, 3), (4, 0), (3, 0), (4, 1)]),
    "fixed_in_the_middle": ([0, 0, 1, 0, 0], [(1, 0), (2, 1), (3, 2), (4, 3), (4, 0), (0, 4)]),
}


def random_graph(seed, fixed, edges, fix_scale, step_updates=None, extent=3.0):
    """a problem on a given structure: vertices a few metres apart, every measurement the vertices' relative Sim3 times a small step
    (step_updates [E, 7]: the steps' tangent vectors, so that a caller can put the residuals where it wants them)"""
    rng = np.random.default_rng(seed)
    V, E = len(fixed), len(edges)
    u = np.concatenate([rng.normal(0, 0.4, (V, 3)), rng.uniform(-extent, extent, (V, 3)), np.zeros((V, 1)) if fix_scale else rng.uniform(-0.1, 0.1, (V, 1))], 1)
    v = sim3_exp(u)[0]
    v[:, :4] /= np.linalg.norm(v[:, :4], axis=1)[:, None]
    if step_updates is None:
        step_updates = np.concatenate([rng.normal(0, 0.02, (E, 3)), rng.normal(0, 0.05, (E, 3)), np.zeros((E, 1)) if fix_scale else rng.normal(0, 0.02, (E, 1))], 1)
    ei, ej = np.array([e[0] for e in edges], np.int32), np.array([e[1] for e in edges], np.int32)
    meas = sim3_mul(sim3_exp(np.asarray(step_updates, np.float64))[0], sim3_mul(v[ej], sim3_inverse(v[ei]))) if E else np.zeros((0, 8))
    return dict(vertex_q=v[:, :4].copy(), vertex_t=v[:, 4:7].copy(), vertex_s=v[:, 7].copy(), vertex_fixed=np.array(fixed, np.uint8), edge_i=ei, edge_j=ej,
                edge_q=meas[:, :4].copy(), edge_t=meas[:, 4:7].copy(), edge_s=meas[:, 7].copy(), edge_w=np.where(np.arange(E) % 3 == 2, 3.0, 1.0),
                fix_scale=fix_scale, iterations=20, lambda_init=1e-16)
