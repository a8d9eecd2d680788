"""Shared by the CreateNewMapPoints tests: builds and calls the sequential CPU restatement (tests/host/triangulate_restatement.cpp),
an independent numpy statement of DESIGN.md section 14 (candidate gates, rotation histogram, triangulation with the two written
rules, its own Jacobi), the random problems and the constructed cases.  Not a test module."""
import copy
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from geoflowslam_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "triangulate_restatement.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_triangulate_restatement.so")
_L = None

EXITS = api.TRI_EXITS
(NO_MATCH, LOW_PARALLAX, SVD_W_ZERO, UNPROJECT_FAILED, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, ZERO_DIST, FAR, SCALE, CREATED) = range(12)
STATS = ("mono_ok", "mono_rejected", "stereo_ok", "stereo_rejected", "ties", "rematched")
CONSTANTS = ("TH_LOW", "HISTO_LENGTH", "epipole_factor", "epipolar_chi2", "cos_parallax", "cos_parallax_inertial", "chi2_mono", "chi2_stereo",
             "ratio_factor", "nn", "nn_monocular")
f32, f64 = np.float32, np.float64


def restatement():
    global _L
    if _L is None:
        rule = os.path.join(ROOT, "geoflowslam_amd", "csrc", "triangulate_rule.hpp")
        deps = [_SRC, rule, os.path.join(ROOT, "include", "gfs_abi.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            tmp = _SO + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I" + os.path.join(ROOT, "include"),
                            "-I" + os.path.dirname(rule), "-o", tmp, _SRC], check=True)
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        vp = C.c_void_p
        L.tr_create_new_map_points.argtypes = [C.POINTER(api.TriProblem), C.c_int, C.POINTER(C.POINTER(api.TriResult)), vp]
        L.tr_create_new_map_points.restype = C.c_int
        L.tr_null_vector.argtypes = [vp, C.c_int, vp]
        L.tr_cos_stereo.argtypes = [C.c_float, vp, C.c_int, vp]
        L.tr_constants.argtypes = [vp]
        _L = L
    return _L


def restate(probs, with_stats=False):
    """The restatement on one problem dict or a list -> what api.ProjectionMatcher.create_new_map_points returns."""
    single = isinstance(probs, dict)
    pl = [probs] if single else list(probs)
    PP, RP, keep = api.tri_structs(pl)
    stats = np.zeros(6, np.int64)
    assert restatement().tr_create_new_map_points(PP, len(pl), RP, stats.ctypes.data) == 0
    out = api.tri_results(PP, RP, keep, len(pl))
    out = out[0] if single else out
    return (out, dict(zip(STATS, (int(v) for v in stats)))) if with_stats else out


def rule_null_vector(A):
    A = np.ascontiguousarray(A, f32).reshape(-1, 16)
    out = np.zeros((len(A), 4), f32)
    restatement().tr_null_vector(A.ctypes.data, len(A), out.ctypes.data)
    return out


def rule_cos_stereo(mb, depth):
    depth = np.ascontiguousarray(depth, f32)
    out = np.zeros(len(depth), f32)
    restatement().tr_cos_stereo(float(f32(mb)), depth.ctypes.data, len(depth), out.ctypes.data)
    return out


def rule_constants():
    out = np.zeros(len(CONSTANTS), f64)
    restatement().tr_constants(out.ctypes.data)
    return dict(zip(CONSTANTS, out.tolist()))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_equal(got, want, what=""):
    """Bit equality of everything gfs_create_new_map_points delivers for ONE problem, neighbour by neighbour."""
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        for k in ("n_matches", "n_created"):
            assert g[k] == w[k], (what, i, k, g[k], w[k])
        for k in ("match12", "exit", "point_stereo"):
            assert same_bits(g[k], w[k]), (what, i, k, np.nonzero(np.asarray(g[k]) != np.asarray(w[k]))[0][:8])
        assert same_bits(g["x3d"], w["x3d"]), (what, i, "x3d", np.nonzero((g["x3d"].view(np.uint32) != w["x3d"].view(np.uint32)).any(1))[0][:8])


# ---------------------------------------------------------------- the numpy statement

def jacobi_null_vector(Af):
    """Written rule 2: one-sided Jacobi in float64 on the columns of the float32 4 x 4 matrix, cyclic order, rotate when
    |ap . aq| > 2^-52 sqrt(|ap|^2 |aq|^2), at most 30 sweeps; V's column of the smallest column norm, lowest index on ties."""
    A = [[f64(Af[r][c]) for c in range(4)] for r in range(4)]
    V = [[f64(1.0 if r == c else 0.0) for c in range(4)] for r in range(4)]
    eps = f64(2.0) ** -52

    def dot(p, q):
        return ((A[0][p] * A[0][q] + A[1][p] * A[1][q]) + A[2][p] * A[2][q]) + A[3][p] * A[3][q]

    sweeps = 0
    with np.errstate(all="ignore"):
        for _ in range(30):
            rotated = False
            for p, q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
                alpha, beta, gamma = dot(p, p), dot(q, q), dot(p, q)
                if not abs(gamma) > eps * np.sqrt(alpha * beta):
                    continue
                rotated = True
                zeta = (beta - alpha) / (f64(2.0) * gamma)
                r = abs(zeta) + np.sqrt(f64(1.0) + zeta * zeta)
                t = f64(-1.0) / r if zeta < 0 else f64(1.0) / r
                c = f64(1.0) / np.sqrt(f64(1.0) + t * t)
                s = c * t
                for M in (A, V):
                    for k in range(4):
                        mp, mq = M[k][p], M[k][q]
                        M[k][p] = c * mp - s * mq
                        M[k][q] = s * mp + c * mq
            if not rotated:
                break
            sweeps += 1
        norms = [dot(c, c) for c in range(4)]
    best = 0
    for c in range(1, 4):
        if norms[c] < norms[best]:
            best = c
    return [f32(V[k][best]) for k in range(4)], sweeps


def cos_stereo(mb, depth):
    """Written rule 1: the float nearest to (d^2 - h^2) / (d^2 + h^2) in float64, h = mb / 2 in float32."""
    h = f32(f32(mb) / f32(2))
    with np.errstate(all="ignore"):
        d2, h2 = f64(depth) * f64(depth), f64(h) * f64(h)
        return f32((d2 - h2) / (d2 + h2))


def _rot_bin(a1, a2):
    rot = f32(a1 - a2)
    if rot < 0:
        rot = f32(rot + f32(360))
    v = float(f32(rot * f32(f32(1) / f32(30))))
    b = int(np.floor(abs(v) + 0.5) * (1 if v >= 0 else -1))  # round half away from zero
    return 0 if b == 30 else b


def _three_maxima(hist):
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(hist):
        if s > m1:
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif s > m2:
            m3, m2, i3, i2 = m2, s, i2, i
        elif s > m3:
            m3, i3 = s, i
    if f32(m2) < f32(f32(0.1) * f32(m1)):
        i2 = i3 = -1
    elif f32(m3) < f32(f32(0.1) * f32(m1)):
        i3 = -1
    return i1, i2, i3


def _dot3(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def _row(T, r, p):
    return f32(_dot3(T[r, :3], p) + T[r, 3])


def _reproj_ok(kf, i, P, z, mbf, T, info, tag):
    g = {k: f32(kf[k]) for k in ("fx", "fy", "cx", "cy")}
    s2 = f32(kf["level_sigma2"][int(kf["kps_un"]["octave"][i])])
    x, y = _row(T, 0, P), _row(T, 1, P)
    invz = f32(f64(1.0) / f64(z))
    kx, ky, ur = f32(kf["kps_un"]["x"][i]), f32(kf["kps_un"]["y"][i]), f32(kf["u_right"][i])
    if not ur >= 0:
        u, v = f32(f32(f32(g["fx"] * x) / z) + g["cx"]), f32(f32(f32(g["fy"] * y) / z) + g["cy"])
        ex, ey = f32(u - kx), f32(v - ky)
        e2, chi = f32(f32(ex * ex) + f32(ey * ey)), 5.991
    else:
        u = f32(f32(f32(g["fx"] * x) * invz) + g["cx"])
        ur_ = f32(u - f32(mbf * invz))
        v = f32(f32(f32(g["fy"] * y) * invz) + g["cy"])
        ex, ey, er = f32(u - kx), f32(v - ky), f32(ur_ - ur)
        e2, chi = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er)), 7.8
    info[tag] = (e2, chi, s2)
    return not f64(e2) > f64(chi) * f64(s2)


def match_statement(prob, nb, i1, i2, info=None):
    """One match of DESIGN.md section 14: -> (exit, x3d, point_stereo).  info (a dict) receives the decisive quantities."""
    info = {} if info is None else info
    k1, k2 = prob["cur"], nb
    T1, T2 = np.asarray(k1["Tcw"], f32).reshape(3, 4), np.asarray(k2["Tcw"], f32).reshape(3, 4)
    zero = np.zeros(3, f32)
    with np.errstate(all="ignore"):
        ur1, ur2 = f32(k1["u_right"][i1]), f32(k2["u_right"][i2])
        st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)
        xn = []
        for kf, i in ((k1, i1), (k2, i2)):
            xn.append([f32(f32(f32(kf["kps_un"]["x"][i]) - f32(kf["cx"])) / f32(kf["fx"])),
                       f32(f32(f32(kf["kps_un"]["y"][i]) - f32(kf["cy"])) / f32(kf["fy"])), f32(1)])
        rays = [[_dot3(T[:, r], x) for r in range(3)] for T, x in ((T1, xn[0]), (T2, xn[1]))]
        n1, n2 = np.sqrt(_dot3(rays[0], rays[0])), np.sqrt(_dot3(rays[1], rays[1]))
        cos_rays = f32(_dot3(rays[0], rays[1]) / f32(n1 * n2))
        info["cos_rays"] = cos_rays
        cs1 = cs2 = f32(cos_rays + f32(1))
        if st1:
            cs1 = cos_stereo(k1["mb"], k1["depth"][i1])
        elif st2:
            cs2 = cos_stereo(k2["mb"], k2["depth"][i2])
        cs = cs2 if cs2 < cs1 else cs1
        lim = 0.9996 if prob.get("inertial") else 0.9998
        stereo = 0
        if cos_rays < cs and cos_rays > 0 and (st1 or st2 or f64(cos_rays) < f64(lim)):
            A = [[f32(f32(xn[0][0] * T1[2, c]) - T1[0, c]) for c in range(4)], [f32(f32(xn[0][1] * T1[2, c]) - T1[1, c]) for c in range(4)],
                 [f32(f32(xn[1][0] * T2[2, c]) - T2[0, c]) for c in range(4)], [f32(f32(xn[1][1] * T2[2, c]) - T2[1, c]) for c in range(4)]]
            info["A"] = np.array(A, f32)
            h, info["sweeps"] = jacobi_null_vector(A)
            if h[3] == 0:
                return SVD_W_ZERO, zero, 0
            P = np.array([f32(h[k] / h[3]) for k in range(3)], f32)
        elif (st1 and cs1 < cs2) or (st2 and cs2 < cs1):
            kf, i = (k1, i1) if (st1 and cs1 < cs2) else (k2, i2)
            stereo = 1
            zd = f32(kf["depth"][i])
            if not zd > 0:
                return UNPROJECT_FAILED, zero, 1
            x = f32(f32(f32(f32(kf["kps"]["x"][i]) - f32(kf["cx"])) * zd) * f32(kf["invfx"]))
            y = f32(f32(f32(f32(kf["kps"]["y"][i]) - f32(kf["cy"])) * zd) * f32(kf["invfy"]))
            Rwc, twc = np.asarray(kf["Rwc"], f32).reshape(3, 3), np.asarray(kf["twc"], f32)
            P = np.array([f32(_dot3(Rwc[r], [x, y, zd]) + twc[r]) for r in range(3)], f32)
        else:
            return LOW_PARALLAX, zero, 0
        z1 = _row(T1, 2, P)
        if z1 <= 0:
            return BEHIND_1, P, stereo
        z2 = _row(T2, 2, P)
        if z2 <= 0:
            return BEHIND_2, P, stereo
        mbf = f32(k1["mbf"])
        if not _reproj_ok(k1, i1, P, z1, mbf, T1, info, "chi1"):
            return REPROJ_1, P, stereo
        if not _reproj_ok(k2, i2, P, z2, mbf, T2, info, "chi2"):
            return REPROJ_2, P, stereo
        a, b = [f32(P[k] - f32(k1["Ow"][k])) for k in range(3)], [f32(P[k] - f32(k2["Ow"][k])) for k in range(3)]
        d1, d2 = np.sqrt(_dot3(a, a)), np.sqrt(_dot3(b, b))
        if d1 == 0 or d2 == 0:
            return ZERO_DIST, P, stereo
        th = f32(prob.get("th_far_points", 0))
        if prob.get("far_points") and (d1 >= th or d2 >= th):
            return FAR, P, stereo
        rd = f32(d2 / d1)
        ro = f32(f32(k1["scale_factors"][int(k1["kps_un"]["octave"][i1])]) / f32(k2["scale_factors"][int(k2["kps_un"]["octave"][i2])]))
        rf = f32(prob["ratio_factor"])
        info["ratio"] = (rd, ro, rf)
        if f32(rd * rf) < ro or rd > f32(ro * rf):
            return SCALE, P, stereo
        return CREATED, P, stereo


def candidate_matrix(prob, nb, l1, l2):
    """Per pair (list positions of one common node) the descriptor distance where the pair passes the entry-state filters and the
    gates of DESIGN.md section 14, 255 otherwise; float32 arrays, one rounding per operation."""
    k1, k2 = prob["cur"], nb
    only_stereo, coarse = bool(prob.get("only_stereo")), bool(prob.get("coarse"))
    F = np.asarray(nb["F12"], f32).reshape(3, 3)
    ep = np.asarray(nb["ep"], f32)
    with np.errstate(all="ignore"):
        x1, y1 = k1["kps_un"]["x"][l1].astype(f32)[:, None], k1["kps_un"]["y"][l1].astype(f32)[:, None]
        x2, y2 = k2["kps_un"]["x"][l2].astype(f32)[None, :], k2["kps_un"]["y"][l2].astype(f32)[None, :]
        st1, st2 = (np.asarray(k1["u_right"], f32)[l1] >= 0)[:, None], (np.asarray(k2["u_right"], f32)[l2] >= 0)[None, :]
        ok = (np.asarray(k1["has_mp"])[l1] == 0)[:, None] & (np.asarray(k2["has_mp"])[l2] == 0)[None, :]
        if only_stereo:
            ok = ok & st1 & st2
        b1 = np.unpackbits(np.asarray(k1["desc"], np.uint8).reshape(-1, 32)[l1], axis=1).astype(np.int32)
        b2 = np.unpackbits(np.asarray(k2["desc"], np.uint8).reshape(-1, 32)[l2], axis=1).astype(np.int32)
        dist = b1 @ (1 - b2).T + (1 - b1) @ b2.T
        ok = ok & (dist <= 50)
        oct2 = k2["kps_un"]["octave"][l2]
        sc2, sg2 = np.asarray(k2["scale_factors"], f32)[oct2][None, :], np.asarray(k2["level_sigma2"], f32)[oct2][None, :]
        ex, ey = ep[0] - x2, ep[1] - y2
        near = (ex * ex + ey * ey) < f32(100) * sc2
        ok = ok & ~(~st1 & ~st2 & near)
        if not coarse:
            a = (x1 * F[0, 0] + y1 * F[1, 0]) + F[2, 0]
            b = (x1 * F[0, 1] + y1 * F[1, 1]) + F[2, 1]
            c = (x1 * F[0, 2] + y1 * F[1, 2]) + F[2, 2]
            num = (a * x2 + b * y2) + c
            den = (a * a + b * b) + np.zeros_like(num)
            dsqr = (num * num) / den
            assert dsqr.dtype == f32
            ok = ok & (den != 0) & (dsqr.astype(f64) < f64(3.84) * sg2.astype(f64))
    return np.where(ok, dist, 255)


def numpy_statement(prob):
    """DESIGN.md section 14 for one problem -> the list of per-neighbour dicts."""
    k1 = prob["cur"]
    n = len(k1["kps_un"])
    has1 = np.asarray(k1["has_mp"]).astype(bool).copy()
    id1 = {int(v): j for j, v in enumerate(np.asarray(k1["node_id"]))}
    out = []
    for nb in prob["neighbours"]:
        m12 = np.full(n, -1, np.int32)
        for j2, nid in enumerate(np.asarray(nb["node_id"])):
            j1 = id1.get(int(nid))
            if j1 is None:
                continue
            l1 = np.asarray(k1["feat_idx"])[k1["node_start"][j1]:k1["node_start"][j1 + 1]]
            l2 = np.asarray(nb["feat_idx"])[nb["node_start"][j2]:nb["node_start"][j2 + 1]]
            if len(l1) == 0 or len(l2) == 0:
                continue
            M = candidate_matrix(prob, nb, l1, l2)
            taken = np.zeros(len(l2), bool)
            for a, i1 in enumerate(l1):
                if has1[i1]:
                    continue
                d = np.where(taken, 255, M[a])
                if d.min() == 255:
                    continue
                b = len(l2) - 1 - int(np.argmin(d[::-1]))  # the minimum, the last position among equals
                taken[b] = True
                m12[i1] = l2[b]
        if prob.get("check_orientation"):
            bins = {int(i): _rot_bin(f32(k1["kps_un"]["angle"][i]), f32(nb["kps_un"]["angle"][m12[i]])) for i in np.nonzero(m12 >= 0)[0]}
            keep = _three_maxima(np.bincount(list(bins.values()), minlength=30).tolist())
            for i, b in bins.items():
                if b not in keep:
                    m12[i] = -1
        ex, x3d, ps = np.zeros(n, np.uint8), np.zeros((n, 3), f32), np.zeros(n, np.uint8)
        for i in np.nonzero(m12 >= 0)[0]:
            ex[i], x3d[i], ps[i] = match_statement(prob, nb, int(i), int(m12[i]))
        has1 |= ex == CREATED
        out.append(dict(match12=m12, exit=ex, x3d=x3d, point_stereo=ps, n_matches=int((m12 >= 0).sum()), n_created=int((ex == CREATED).sum())))
    return out


# ---------------------------------------------------------------- problems

def random_problem(seed):
    """The 32 seeded problems of the CPU tests: small, every flag somewhere."""
    return synth.triangulation_problem(1000 + seed, n_kp=90 + 5 * seed, n_neighbours=1 + seed % 4, n_nodes=6 + seed % 7, mono_frac=0.35,
                                       bad_depth_frac=0.03, check_orientation=seed % 3 == 1, only_stereo=seed % 8 == 5, coarse=seed % 8 == 6,
                                       inertial=seed % 4 == 2, far_points=seed % 2 == 1, th_far_points=5.0,
                                       scale_factor=1.1 if seed % 5 == 4 else 1.2)


@functools.lru_cache(maxsize=None)
def problem(n_kp, n_kp_nb, n_neighbours=2, n_nodes=None, **kw):
    """A seeded problem of the GPU tests and its restatement (computed once, shared, left unchanged)."""
    n_nodes = max(1, max(n_kp, n_kp_nb) // 12) if n_nodes is None else n_nodes
    prob = synth.triangulation_problem(7 * n_kp + n_kp_nb + 13 * n_neighbours, n_kp=n_kp, n_kp_neighbour=n_kp_nb, n_neighbours=n_neighbours,
                                       n_nodes=n_nodes, bad_depth_frac=0.02, far_points=True, th_far_points=7.0, **kw)
    return prob, restate(prob)


def _kf(n, nodes, desc, xy, ur, depth, octave=0, has_mp=None, T_wc=None, angle=None):
    """A hand-made key frame: nodes = [(id, [indices])]."""
    fx, fy, cx, cy = (f32(v) for v in synth.intrinsics(640, 480))
    T = np.eye(4) if T_wc is None else T_wc
    R, t = T[:3, :3].T, -T[:3, :3].T @ T[:3, 3]
    kps = np.zeros(n, api.KP_DTYPE)
    kps["x"], kps["y"] = np.asarray(xy, f32)[:, 0], np.asarray(xy, f32)[:, 1]
    kps["octave"] = octave
    kps["angle"] = 0 if angle is None else angle
    scale = (f32(1.2) ** np.arange(8)).astype(f32)
    Ow = (-(R.T @ t)).astype(f32)
    return dict(Tcw=np.concatenate([R, t[:, None]], 1).astype(f32).reshape(-1), Ow=Ow, Rwc=R.T.astype(f32).reshape(-1), twc=Ow.copy(), fx=fx, fy=fy,
                cx=cx, cy=cy, invfx=f32(1) / fx, invfy=f32(1) / fy, mbf=f32(f32(0.0745) * fx), mb=f32(0.0745), scale_factors=scale,
                level_sigma2=(scale * scale).astype(f32), n_levels=8, kps_un=kps, kps=kps.copy(), u_right=np.asarray(ur, f32),
                depth=np.asarray(depth, f32), desc=np.asarray(desc, np.uint8).reshape(n, 32),
                has_mp=np.zeros(n, np.uint8) if has_mp is None else np.asarray(has_mp, np.uint8),
                node_id=np.array([k for k, _ in nodes], np.int32), node_start=np.concatenate([[0], np.cumsum([len(l) for _, l in nodes])]).astype(np.int32),
                feat_idx=np.array([i for _, l in nodes for i in l], np.int32))


def _desc(*n_bits):
    """Descriptors at the given Hamming distances from the all-zero descriptor."""
    d = np.zeros((len(n_bits), 256), np.uint8)
    for r, b in enumerate(n_bits):
        d[r, :b] = 1
    return np.packbits(d, axis=1)


def _geometry(world, T_wc, noise=0.0):
    """Projects world points into a camera at T_wc -> pixel positions, depths, u_right."""
    fx, fy, cx, cy = synth.intrinsics(640, 480)
    R, t = T_wc[:3, :3].T, -T_wc[:3, :3].T @ T_wc[:3, 3]
    Pc = np.asarray(world, f64) @ R.T + t
    xy = np.stack([fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy], 1)
    return xy, Pc[:, 2], xy[:, 0] - 0.0745 * fx / Pc[:, 2]


def _with_F(cur, nb):
    """ep / F12 of a hand-made pair, as synth.triangulation_problem computes them."""
    fx, fy, cx, cy = cur["fx"], cur["fy"], cur["cx"], cur["cy"]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)
    Kinv = np.linalg.inv(K.astype(f64)).astype(f32)
    T1, T2 = cur["Tcw"].reshape(3, 4), nb["Tcw"].reshape(3, 4)
    R1, t1, R2, t2 = T1[:, :3], T1[:, 3], T2[:, :3], T2[:, 3]
    C2 = (R2 @ cur["Ow"] + t2).astype(f32)
    with np.errstate(all="ignore"):
        nb["ep"] = np.array([fx * C2[0] / C2[2] + cx, fy * C2[1] / C2[2] + cy], f32)
    R12 = (R1 @ R2.T).astype(f32)
    t12 = (t1 - R12 @ t2).astype(f32)
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]], f32)
    nb["F12"] = (((Kinv.T @ tx).astype(f32) @ R12).astype(f32) @ Kinv).astype(f32).reshape(-1)
    return nb


def _shift(dx, dy=0.0, dz=0.0):
    T = np.eye(4)
    T[:3, 3] = (dx, dy, dz)
    return T


def _prob(cur, nbs, **kw):
    return dict(dict(cur=cur, neighbours=[_with_F(cur, nb) for nb in nbs], ratio_factor=f32(f32(1.5) * f32(1.2)), coarse=True), **kw)


def constructed():
    """Hand-made problems, each with the result its label promises: -> {label: (problem, check(result))}.  All are `coarse` (the
    epipolar-line gate is the subject of its own cases below) and stereo, so every listed pair is a candidate by its distance alone."""
    cases = {}
    world = np.array([[0.3 * k - 0.6, 0.1 * k - 0.2, 3.0 + 0.2 * k] for k in range(6)])
    Tc, Tn, Tn2 = _shift(0, 0, 0), _shift(0.3, 0, 0), _shift(-0.25, 0.05, 0)

    def kf(T, nodes, desc, n=None, **kw):
        n = len(desc) if n is None else n
        xy, z, ur = _geometry(world[:n], T)
        return _kf(n, nodes, desc, xy, ur, z, octave=2, T_wc=T, **kw)

    # distance 50 accepted, 51 rejected
    p = _prob(kf(Tc, [(5, [0]), (6, [1])], _desc(0, 0)), [kf(Tn, [(5, [0]), (6, [1])], _desc(50, 51))])
    cases["distance 50 accepted, 51 rejected"] = (p, lambda r: r[0]["match12"].tolist() == [0, -1])
    # two idx1 want one idx2: the first in node order gets it, the second its next best (list order 1, 0: idx1 1 goes first)
    p = _prob(kf(Tc, [(5, [1, 0])], _desc(0, 0)), [kf(Tn, [(5, [0, 1])], _desc(10, 30))])
    cases["two idx1 wanting one idx2"] = (p, lambda r: r[0]["match12"].tolist() == [1, 0])
    # equal distances: the last in list order wins
    p = _prob(kf(Tc, [(5, [0])], _desc(0)), [kf(Tn, [(5, [2, 0, 1])], _desc(20, 20, 20))])
    cases["equal distances, last in list order"] = (p, lambda r: r[0]["match12"].tolist() == [1])
    # a CREATED at neighbour 0 removes idx1 0 at neighbour 1, and idx1 1 gets the idx2 that idx1 0 would have taken
    nb0 = kf(Tn, [(5, [0])], _desc(5))
    nb1 = kf(Tn2, [(5, [0, 1])], _desc(10, 30))
    p = _prob(kf(Tc, [(5, [0, 1])], _desc(0, 0)), [nb0, nb1])
    cases["created at neighbour 0 changes neighbour 1"] = (
        p, lambda r: r[0]["match12"].tolist() == [0, -1] and r[0]["exit"][0] == CREATED and r[1]["match12"].tolist() == [-1, 0] and r[1]["exit"][0] == NO_MATCH)
    q = copy.deepcopy(p)  # ... and without the creation (the neighbour-0 key-point is somewhere else: reprojection fails) idx1 0 keeps it
    q["neighbours"][0]["kps_un"]["x"] += f32(40)
    q["neighbours"][0]["u_right"] = q["neighbours"][0]["u_right"] + f32(40)
    cases["failed gate at neighbour 0 is searched again"] = (
        q, lambda r: r[0]["match12"].tolist() == [0, -1] and r[0]["exit"][0] in (REPROJ_1, REPROJ_2) and r[1]["match12"].tolist() == [0, 1])
    # nodes present in only one key frame
    p = _prob(kf(Tc, [(2, [0]), (5, [1]), (9, [2])], _desc(0, 0, 0)), [kf(Tn, [(1, [0]), (5, [1]), (7, [2])], _desc(0, 0, 0))])
    cases["nodes present in only one key frame"] = (p, lambda r: r[0]["match12"].tolist() == [-1, 1, -1])
    # den == 0: a zero F12 makes every epipolar line [0 0 0]
    p = _prob(kf(Tc, [(5, [0])], _desc(0)), [kf(Tn, [(5, [0])], _desc(0))], coarse=False)
    q = copy.deepcopy(p)
    q["neighbours"][0]["F12"] = np.zeros(9, f32)
    cases["den != 0 control"] = (p, lambda r: r[0]["match12"].tolist() == [0])
    cases["den == 0"] = (q, lambda r: r[0]["match12"].tolist() == [-1])
    # the SVD's w == 0: a sheared second pose whose rays are not parallel but whose system has a zero third column
    p = _prob(kf(Tc, [(5, [0])], _desc(0)), [kf(Tn, [(5, [0])], _desc(0))])
    for k_ in (p["cur"], p["neighbours"][0]):
        k_["kps_un"]["x"], k_["kps_un"]["y"], k_["u_right"], k_["depth"] = k_["cx"], k_["cy"], np.full(1, -1, f32), np.full(1, -1, f32)
    p["neighbours"][0]["Tcw"] = np.array([1, 0, 0, -0.3, 0, 1, 0, 0.1, 0.5, 0, 1, 0], f32)
    cases["svd w == 0"] = (p, lambda r: r[0]["exit"].tolist() == [SVD_W_ZERO])
    # dist2 == 0: the neighbour's camera centre is given as the point itself
    p = _prob(kf(Tc, [(5, [0])], _desc(0)), [kf(Tn, [(5, [0])], _desc(0))])
    base = restate(p)
    q = copy.deepcopy(p)
    q["neighbours"][0]["Ow"] = base[0]["x3d"][0].copy()
    cases["zero distance"] = (q, lambda r, b=base: b[0]["exit"].tolist() == [CREATED] and r[0]["exit"].tolist() == [ZERO_DIST])
    return cases


def straddle(bound_of, lo, hi):
    """The adjacent float32 pair (a, b = nextafter(a)) in [lo, hi] with bound_of(a) False and bound_of(b) True (bisection)."""
    lo, hi = f32(lo), f32(hi)
    assert not bound_of(lo) and bound_of(hi)
    while np.nextafter(lo, f32(np.inf)) != hi:
        mid = f32((f64(lo) + f64(hi)) / 2)
        if mid == lo or mid == hi:
            break
        if bound_of(mid):
            hi = mid
        else:
            lo = mid
    return lo, hi
