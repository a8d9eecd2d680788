"""Shared by the ORBmatcher::Fuse tests: builds and calls the sequential CPU restatement (tests/host/fuse_restatement.cpp), an
independent numpy.float32 statement of the per-(point, key frame) rule, the random problems and the
constructed points.  Not a test module."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from geoflowslam_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "fuse_restatement.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_fuse_restatement.so")
_L = None

EXITS = api.FUSE_EXITS
NEG_DEPTH, NOT_IN_IMAGE, TOO_NEAR, TOO_FAR, VIEW_ANGLE, EMPTY_WINDOW, NO_CANDIDATE, MATCHED = range(8)
STATS = ("stereo", "mono", "stereo_rejected", "mono_rejected", "ties", "ties_other_cell")


def restatement():
    global _L
    if _L is None:
        deps = [_SRC, os.path.join(ROOT, "include", "gfs_abi.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            tmp = _SO + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I" + os.path.join(ROOT, "include"),
                            "-o", tmp, _SRC], check=True)
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        vp = C.c_void_p
        L.fr_fuse_search.argtypes = [C.POINTER(api.FusePoints), C.c_int, C.POINTER(api.FuseKeyframe), C.c_int, C.POINTER(api.FuseResult), vp]
        L.fr_fuse_search.restype = C.c_int
        L.fr_fuse_point.argtypes = [C.POINTER(api.FuseKeyframe), vp, vp, C.c_float, C.c_float, vp, vp]
        L.fr_fuse_point.restype = None
        L.fr_constants.argtypes = [vp]
        _L = L
    return _L


def restate(prob, with_stats=False):
    """The restatement on a problem dict (lists, keyframes) -> the list of dicts api.ProjectionMatcher.fuse_search returns."""
    LL, KK, RR, keep = api.fuse_structs(prob["lists"], prob["keyframes"])
    stats = np.zeros(6, np.int64)
    rc = restatement().fr_fuse_search(LL, len(prob["lists"]), KK, len(prob["keyframes"]), RR, stats.ctypes.data)
    assert rc == 0
    out = api.fuse_results(LL, KK, RR, keep, len(prob["lists"]))
    return (out, dict(zip(STATS, (int(v) for v in stats)))) if with_stats else out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_equal(got, want, what=""):
    """Bit equality of everything gfs_fuse_search delivers, key frame by key frame; level where it is defined (exit >= empty window)."""
    assert len(got) == len(want), what
    for f, (g, w) in enumerate(zip(got, want)):
        assert g["n_matched"] == w["n_matched"], (what, f, "n_matched", g["n_matched"], w["n_matched"])
        for k in ("exit", "best_idx", "best_dist"):
            assert same_bits(g[k], w[k]), (what, f, k, np.nonzero(np.asarray(g[k]) != np.asarray(w[k]))[0][:8])
        d = w["exit"] >= EMPTY_WINDOW
        assert same_bits(g["level"][d], w["level"][d]), (what, f, "level")


_libm = C.CDLL("libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]


def libm_logf(x):
    return np.float32(_libm.logf(C.c_float(float(x))))


def _so3_act(q, p):
    f = np.float32
    uv = [f(f(q[1] * p[2]) - f(q[2] * p[1])), f(f(q[2] * p[0]) - f(q[0] * p[2])), f(f(q[0] * p[1]) - f(q[1] * p[0]))]
    uv = [f(x + x) for x in uv]
    c = [f(f(q[1] * uv[2]) - f(q[2] * uv[1])), f(f(q[2] * uv[0]) - f(q[0] * uv[2])), f(f(q[0] * uv[1]) - f(q[1] * uv[0]))]
    return [f(f(p[k] + f(q[3] * uv[k])) + c[k]) for k in range(3)]


def camera_point(kf, P):
    """Pc of DESIGN.md section 13 step 1 (what the constructed points are checked with)."""
    q, t = np.asarray(kf["Tcw_q"], np.float32), np.asarray(kf["Tcw_t"], np.float32)
    with np.errstate(all="ignore"):
        return [np.float32(a + t[k]) for k, a in enumerate(_so3_act(q, np.asarray(P, np.float32)))]


def predict_level(mx, dist, log_sf, n_levels):
    f = np.float32
    with np.errstate(all="ignore"):
        c = np.ceil(f(libm_logf(f(f(mx) / f(dist))) / f(log_sf)))
    lv = int(c) if (np.isfinite(c) and -2147483648.0 <= float(c) < 2147483648.0) else 0
    return min(max(lv, 0), n_levels - 1)


def numpy_statement(prob):
    """DESIGN.md section 13 in numpy.float32 scalars, pair after pair: every operation one float32 rounding, sums left to right, the
    two chi2 gates and the viewing-angle gate compared in float64; logf through ctypes on libm; the grid a dict of cells."""
    f, d64 = np.float32, np.float64
    out = []
    for kf in prob["keyframes"]:
        pts = prob["lists"][int(kf.get("list", 0))]
        xw = np.ascontiguousarray(pts["mp_xw"], f).reshape(-1, 3)
        nrm = np.ascontiguousarray(pts["mp_normal"], f).reshape(-1, 3)
        desc = np.ascontiguousarray(pts["mp_desc"], np.uint8).reshape(-1, 32)
        q, t, Ow = (np.asarray(kf[k], f) for k in ("Tcw_q", "Tcw_t", "Ow"))
        g = {k: f(kf[k]) for k in ("fx", "fy", "cx", "cy", "bf", "min_x", "max_x", "min_y", "max_y", "grid_w_inv", "grid_h_inv",
                                   "log_scale_factor", "th")}
        scale, inv_s2 = np.asarray(kf["scale_factors"], f), np.asarray(kf["inv_level_sigma2"], f)
        nl = int(kf.get("n_levels", len(scale)))
        kps, kur = kf["kps_un"], np.asarray(kf["u_right"], f)
        kbits = np.unpackbits(np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1, 32), axis=1)
        cells = {}
        with np.errstate(all="ignore"):
            for j in range(len(kps)):
                # Frame::PosInGrid rounds half away from zero (np.round would round half to even)
                vx, vy = f(f(kps["x"][j] - g["min_x"]) * g["grid_w_inv"]), f(f(kps["y"][j] - g["min_y"]) * g["grid_h_inv"])
                px = int(np.floor(abs(float(vx)) + 0.5) * (1 if vx >= 0 else -1))
                py = int(np.floor(abs(float(vy)) + 0.5) * (1 if vy >= 0 else -1))
                if 0 <= px < 64 and 0 <= py < 48:
                    cells.setdefault((px, py), []).append(j)
        n = len(xw)
        ex_, bi, bd, lv = np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.full(n, 256, np.int32), np.zeros(n, np.int32)
        with np.errstate(all="ignore"):
            for i in range(n):
                P, Pn = xw[i], nrm[i]
                Pc = [f(a + t[k]) for k, a in enumerate(_so3_act(q, P))]
                if Pc[2] < f(0):
                    ex_[i] = NEG_DEPTH
                    continue
                invz = f(f(1) / Pc[2])
                u = f(f(f(g["fx"] * Pc[0]) / Pc[2]) + g["cx"])
                v = f(f(f(g["fy"] * Pc[1]) / Pc[2]) + g["cy"])
                if not (u >= g["min_x"] and u < g["max_x"] and v >= g["min_y"] and v < g["max_y"]):
                    ex_[i] = NOT_IN_IMAGE
                    continue
                ur = f(u - f(g["bf"] * invz))
                PO = [f(P[k] - Ow[k]) for k in range(3)]
                dist = np.sqrt(f(f(f(PO[0] * PO[0]) + f(PO[1] * PO[1])) + f(PO[2] * PO[2])))
                mn, mx = f(pts["mp_min_dist"][i]), f(pts["mp_max_dist"][i])
                if dist < f(f(0.8) * mn):
                    ex_[i] = TOO_NEAR
                    continue
                if dist > f(f(1.2) * mx):
                    ex_[i] = TOO_FAR
                    continue
                dot = f(f(f(PO[0] * Pn[0]) + f(PO[1] * Pn[1])) + f(PO[2] * Pn[2]))
                if d64(dot) < d64(0.5) * d64(dist):
                    ex_[i] = VIEW_ANGLE
                    continue
                level = predict_level(mx, dist, g["log_scale_factor"], nl)
                lv[i] = level
                r = f(g["th"] * scale[level])
                ex_[i] = EMPTY_WINDOW
                x0 = max(0, int(np.floor(f(f(f(u - g["min_x"]) - r) * g["grid_w_inv"]))))
                x1 = min(63, int(np.ceil(f(f(f(u - g["min_x"]) + r) * g["grid_w_inv"]))))
                y0 = max(0, int(np.floor(f(f(f(v - g["min_y"]) - r) * g["grid_h_inv"]))))
                y1 = min(47, int(np.ceil(f(f(f(v - g["min_y"]) + r) * g["grid_h_inv"]))))
                if x0 >= 64 or x1 < 0 or y0 >= 48 or y1 < 0:
                    continue
                pbits = np.unpackbits(desc[i])
                any_in = False
                for ix in range(x0, x1 + 1):
                    for iy in range(y0, y1 + 1):
                        for j in cells.get((ix, iy), ()):
                            kx, ky = f(kps["x"][j]), f(kps["y"][j])
                            if not (abs(f(kx - u)) < r and abs(f(ky - v)) < r):
                                continue
                            any_in = True
                            o = int(kps["octave"][j])
                            if o < level - 1 or o > level:
                                continue
                            ex, ey = f(u - kx), f(v - ky)
                            if kur[j] >= 0:
                                er = f(ur - kur[j])
                                e2 = f(f(f(ex * ex) + f(ey * ey)) + f(er * er))
                                if d64(f(e2 * inv_s2[o])) > d64(7.8):
                                    continue
                            else:
                                e2 = f(f(ex * ex) + f(ey * ey))
                                if d64(f(e2 * inv_s2[o])) > d64(5.99):
                                    continue
                            dd = int((pbits != kbits[j]).sum())
                            if dd < bd[i]:
                                bd[i], bi[i] = dd, j
                if any_in:
                    ex_[i] = MATCHED if bd[i] <= 50 else NO_CANDIDATE
        out.append(dict(exit=ex_, best_idx=bi, best_dist=bd, level=lv, n_matched=int((ex_ == MATCHED).sum())))
    return out


# The random problems of the tests: every wave and workgroup boundary (64 lanes, 256 threads) crossed with n_kp in {0, 1, 500}.
N_MP = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
N_KP = (0, 1, 500)
CASES = [(n, c) for n in N_MP for c in N_KP]


@functools.lru_cache(maxsize=None)
def problem(n_mp, n_kp, n_keyframes=1, seed=None, scale_factor=1.2, th=3.0):
    """(problem dict, restatement output), computed once and shared; the arrays must not be modified."""
    s = (n_mp * 7 + n_kp + 1000 * n_keyframes) if seed is None else seed
    prob = synth.fuse_problem(s, n_points=n_mp, n_kp=n_kp, n_keyframes=n_keyframes, scale_factor=scale_factor, th=th)
    return prob, restate(prob)


@functools.lru_cache(maxsize=None)
def five_keyframes():
    """One list against five key frames of different poses, th and scale factor (1.2 and 1.1)."""
    a = synth.fuse_problem(501, n_points=700, n_kp=600, n_keyframes=3, scale_factor=1.2)
    b = synth.fuse_problem(501, n_points=700, n_kp=450, n_keyframes=3, scale_factor=1.1)  # same seed: same poses and points
    kfs = [dict(a["keyframes"][0], th=np.float32(3.0)), dict(b["keyframes"][1], th=np.float32(5.0)), dict(a["keyframes"][2], th=np.float32(1.5)),
           dict(b["keyframes"][0], th=np.float32(3.0)), dict(a["keyframes"][1], th=np.float32(7.0))]
    prob = dict(lists=a["lists"], keyframes=kfs)
    return prob, restate(prob)


@functools.lru_cache(maxsize=None)
def two_lists():
    """Two lists of different lengths in one call: three key frames on the long one, two on the short one, interleaved."""
    a = synth.fuse_problem(601, n_points=777, n_kp=500, n_keyframes=3)
    b = synth.fuse_problem(602, n_points=130, n_kp=300, n_keyframes=2)
    kfs = [dict(a["keyframes"][0], list=0), dict(b["keyframes"][0], list=1), dict(a["keyframes"][1], list=0),
           dict(b["keyframes"][1], list=1), dict(a["keyframes"][2], list=0)]
    prob = dict(lists=[a["lists"][0], b["lists"][0]], keyframes=kfs)
    return prob, restate(prob)


# ---- constructed points: each sits exactly on one decision of the rule ----
FLT_MIN = np.float32(1.1754943508222875e-38)


def _up(x, n=1):
    x = np.float32(x)
    for _ in range(n):
        x = np.nextafter(x, np.float32(np.inf))
    return x


def _down(x, n=1):
    x = np.float32(x)
    for _ in range(n):
        x = np.nextafter(x, np.float32(-np.inf))
    return x


def around(c):
    """(largest float32 <= c, smallest float32 > c) for a double constant c."""
    a = np.float32(c)
    return (_down(a), a) if float(a) > c else (a, _up(a))


def _flip(desc, nbits, start=0):
    d = np.array(desc, np.uint8).copy()
    for b in range(start, start + nbits):
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


@functools.lru_cache(maxsize=None)
def constructed():
    """-> (problem dict, {label: (key frame, point index, expected exit, expected best_idx or None, expected best_dist or None)}).

    Key frame A (list 0): a camera at the origin looking along z, q = (0, 0, 0, 1), t = 0, fx = fy = 1, cx = cy = 0, bf = 0, so for
    a point (x, y, 1) Pc = P, u = x, v = y and ur = u exactly; a point (0, 0, d) has dist = sqrtf(d * d) = d exactly.  Its
    inv_level_sigma2 is 1 except on levels 3 .. 6, which hold the floats next to 5.99 and 7.8: a key-point one pixel beside the
    projection has e2 = 1, so e2 * inv_level_sigma2 IS the table entry.  Points that are searched sit 40 pixels apart, far more
    than any window.  Key frame B (list 1): the same camera with t = (0, 0, 1) and Ow = 0, P = Ow: dist = 0 in front of the camera.
    Key frame Z (list 2): q = (0, 0, -1e-30, -1) (the rule takes the quaternion as it comes), for which P = (1, 1, -0) gives
    Pc[2] = -0."""
    f = np.float32
    rng = np.random.default_rng(2024)
    n_levels = 8
    scale = np.cumprod(np.r_[1.0, np.full(n_levels - 1, 1.2)]).astype(np.float32)
    log_sf = libm_logf(f(1.2))
    lo599, hi599 = around(5.99)
    lo78, hi78 = around(7.8)
    inv_s2 = np.ones(n_levels, np.float32)
    inv_s2[3:7] = [lo599, hi599, lo78, hi78]
    min_x, max_x, min_y, max_y = f(-300.5), f(339.5), f(-220.25), f(259.75)
    pts, labels, kp = [], {}, []  # kp: (x, y, octave, u_right, desc)

    def facing(P):
        P = np.array(P, np.float64)
        nrm = np.linalg.norm(P)
        return tuple(P / nrm) if nrm > 0 else (0.0, 0.0, 1.0)

    def add(label, P, n=None, mn=0.0, mx=1000.0, exit=None, idx=None, dist=None, desc=None):
        labels[label] = (0, len(pts), exit, idx, dist)
        pts.append((np.array(P, f), np.array(facing(P) if n is None else n, f), f(mn), f(mx),
                    rng.integers(0, 256, 32, dtype=np.uint8) if desc is None else desc))
        return pts[-1][4]

    def add_kp(x, y, octave, ur, desc):
        kp.append((f(x), f(y), int(octave), f(ur), np.array(desc, np.uint8)))
        return len(kp) - 1

    # image bounds, half open: on min is in, on max is out
    for name, axis, lo, hi in (("u", 0, min_x, max_x), ("v", 1, min_y, max_y)):
        for tag, val, inside in (("==min", lo, True), ("<min", _down(lo), False), ("==max", hi, False), ("<max", _down(hi), True)):
            P = [f(3), f(2), f(1)]
            P[axis] = val
            add(name + tag, P, exit=None if inside else NOT_IN_IMAGE)
    # Pc[2] = +0 (0 / 0 and 1 / 0: NaN and inf fail IsInImage by themselves), -FLT_MIN, +FLT_MIN
    add("z=+0,x=0", (0.0, 0.0, 0.0), exit=NOT_IN_IMAGE)
    add("z=+0,x=1", (1.0, 1.0, 0.0), exit=NOT_IN_IMAGE)
    add("z=-FLT_MIN,x=0", (0.0, 0.0, -FLT_MIN), n=(0, 0, 1), exit=NEG_DEPTH)
    add("z=-FLT_MIN,x=1", (1.0, 1.0, -FLT_MIN), exit=NEG_DEPTH)
    add("z=+FLT_MIN,x=0", (0.0, 0.0, FLT_MIN), n=(0, 0, 1))  # dist = sqrtf(underflow) = 0, min = 0: searched, level 0 by the chosen rule
    # distance gates: dist == 0.8f min and dist == 1.2f max stay, one ulp beyond goes
    m, M = f(3.7), f(2.3)
    d_near, d_far = f(f(0.8) * m), f(f(1.2) * M)
    add("dist==0.8min", (0, 0, d_near), mn=m, mx=100.0)
    add("dist<0.8min", (0, 0, _down(d_near)), mn=m, mx=100.0, exit=TOO_NEAR)
    add("dist==1.2max", (0, 0, d_far), mn=0.0, mx=M)
    add("dist>1.2max", (0, 0, _up(d_far)), mn=0.0, mx=M, exit=TOO_FAR)
    # viewing angle in double: dot = 2 * 0.5 == 0.5 * 2 passes, one ulp less does not, one ulp more does
    add("dot==half", (0, 0, 2), n=(0, 0, 0.5))
    add("dot<half", (0, 0, 2), n=(0, 0, _down(0.5)), exit=VIEW_ANGLE)
    add("dot>half", (0, 0, 2), n=(0, 0, _up(0.5)))
    # level boundaries: max / dist == 1.2f^k (a float product), one ulp below and above, k = 0 .. 8
    pk = f(1)
    for k in range(n_levels + 1):
        for tag, r in (("-1ulp", _down(pk)), ("", pk), ("+1ulp", _up(pk))):
            add("ratio=1.2^%d%s" % (k, tag), (0, 0, 2), mx=f(f(2) * r))
        pk = f(pk * f(1.2))

    # searched points: (u, v, 1) on a 40-pixel lattice right of the image centre (u > 0: a key-point there may carry mvuRight = u),
    # the predicted level chosen through max
    slot = [0]

    def searched(label, level, u=None, v=None):
        s = slot[0]
        slot[0] += 1
        u = f(20 + 40 * (s % 8)) if u is None else f(u)
        v = f(-200 + 40 * (s // 8)) if v is None else f(v)
        dist = np.sqrt(f(f(f(u * u) + f(v * v)) + f(1)))
        mx = f(float(dist) * 1.2 ** (level - 0.5))
        assert predict_level(mx, dist, log_sf, n_levels) == level
        d = add(label, (u, v, 1), mx=mx)
        return u, v, d

    def expect(label, *e):
        labels[label] = labels[label][:2] + e

    # chi2 gates: the table entry is the product
    for label, level, stereo, ok in (("mono<=5.99", 3, False, True), ("mono>5.99", 4, False, False), ("stereo>5.99", 4, True, True),
                                    ("stereo<=7.8", 5, True, True), ("stereo>7.8", 6, True, False)):
        u, v, d = searched(label, level)
        j = add_kp(u + f(1), v, level, u if stereo else -1.0, _flip(d, 7))
        expect(label, *((MATCHED, j, 7) if ok else (NO_CANDIDATE, -1, 256)))
    # mvuRight = -1, -0.0f, 0, +FLT_MIN: `>= 0` sends all but the first to the stereo branch, where er = u - 0 is far beyond 7.8
    for label, ur, ok in (("ur=-1", f(-1), True), ("ur=-0", f(-0.0), False), ("ur=0", f(0), False), ("ur=+FLT_MIN", FLT_MIN, False)):
        u, v, d = searched(label, 2)
        j = add_kp(u, v, 2, ur, _flip(d, 3))
        expect(label, *((MATCHED, j, 3) if ok else (NO_CANDIDATE, -1, 256)))
    # octave = level - 2 .. level + 1
    for k, ok in ((-2, False), (-1, True), (0, True), (1, False)):
        label = "octave=level%+d" % k
        u, v, d = searched(label, 2)
        j = add_kp(u, v, 2 + k, -1.0, _flip(d, 5))
        expect(label, *((MATCHED, j, 5) if ok else (NO_CANDIDATE, -1, 256)))
    # best distance 50 and 51 (TH_LOW)
    for nb, ok in ((50, True), (51, False)):
        label = "dist=%d" % nb
        u, v, d = searched(label, 2)
        j = add_kp(u, v, 2, -1.0, _flip(d, nb))
        expect(label, MATCHED if ok else NO_CANDIDATE, j, nb)
    # two candidates at equal distance in different cells (10-pixel cells, PosInGrid rounds): the first VISITED wins, and it has the
    # higher index.  Columns: x - min_x = 203 -> column 20, 207 -> column 21.  Rows: y - min_y = 203 -> row 20, 207 -> row 21.
    u, v, d = searched("tie_columns", 2, u=min_x + f(205))
    add_kp(u + f(2), v, 2, -1.0, _flip(d, 9, 100))
    j = add_kp(u - f(2), v, 2, -1.0, _flip(d, 9))
    expect("tie_columns", MATCHED, j, 9)
    u, v, d = searched("tie_rows", 2, v=min_y + f(205))
    add_kp(u, v + f(2), 2, -1.0, _flip(d, 9, 100))
    j = add_kp(u, v - f(2), 2, -1.0, _flip(d, 9))
    expect("tie_rows", MATCHED, j, 9)
    # a tie inside one cell: the lower index wins
    u, v, d = searched("tie_cell", 2)
    j = add_kp(u + f(0.25), v, 2, -1.0, _flip(d, 9))
    add_kp(u - f(0.25), v, 2, -1.0, _flip(d, 9, 100))
    expect("tie_cell", MATCHED, j, 9)

    kps = np.zeros(len(kp), api.KP_DTYPE)
    kps["x"], kps["y"], kps["octave"] = [k[0] for k in kp], [k[1] for k in kp], [k[2] for k in kp]
    kps["size"], kps["class_id"] = 31.0, -1

    def lst(ps):
        return dict(mp_xw=np.array([p[0] for p in ps], f), mp_normal=np.array([p[1] for p in ps], f), mp_min_dist=np.array([p[2] for p in ps], f),
                    mp_max_dist=np.array([p[3] for p in ps], f), mp_desc=np.array([p[4] for p in ps], np.uint8))

    A = dict(Tcw_q=np.array([0, 0, 0, 1], f), Tcw_t=np.zeros(3, f), Ow=np.zeros(3, f), fx=f(1), fy=f(1), cx=f(0), cy=f(0), bf=f(0),
             min_x=min_x, max_x=max_x, min_y=min_y, max_y=max_y, grid_w_inv=f(64) / f(max_x - min_x), grid_h_inv=f(48) / f(max_y - min_y),
             scale_factors=scale, inv_level_sigma2=inv_s2, n_levels=n_levels, log_scale_factor=log_sf, th=f(3), kps_un=kps,
             u_right=np.array([k[3] for k in kp], f), desc=np.array([k[4] for k in kp], np.uint8).reshape(-1, 32), list=0)
    some = rng.integers(0, 256, 32, dtype=np.uint8)
    B = dict(A, Tcw_t=np.array([0, 0, 1], f), list=1)
    ptsB = [(np.zeros(3, f), np.array((0, 0, 1), f), f(0), f(10), some), (np.zeros(3, f), np.array((0, 0, 1), f), f(0.5), f(10), some)]
    labels["dist==0,min=0"] = (1, 0, None, None, None)  # 0 < 0.8f * 0 is false: searched, level 0 (max / 0 = inf: chosen rule 2)
    labels["dist==0,min>0"] = (1, 1, TOO_NEAR, None, None)
    Z = dict(A, Tcw_q=np.array([0, 0, -1e-30, -1], f), Tcw_t=np.array([0, 0, -0.0], f), list=2)
    ptsZ = [(np.array((1, 1, -0.0), f), np.array((0, 0, 1), f), f(0), f(1000), some)]
    labels["z=-0,x=1"] = (2, 0, NOT_IN_IMAGE, None, None)  # -0 is not < 0; 1 / -0 = -inf < min_x
    prob = dict(lists=[lst(pts), lst(ptsB), lst(ptsZ)], keyframes=[A, B, Z])
    return prob, labels


def check_constructed(prob, labels, out):
    """The expectations written next to the points, on any implementation's output."""
    pc = camera_point(prob["keyframes"][2], prob["lists"][2]["mp_xw"][0])
    assert pc[2] == 0 and np.signbit(pc[2]), "key frame Z must put its point at Pc[2] = -0"
    pc = camera_point(prob["keyframes"][0], prob["lists"][0]["mp_xw"][labels["z=+0,x=0"][1]])
    assert pc[2] == 0 and not np.signbit(pc[2])
    for label, (f, i, ex, idx, dist) in labels.items():
        o = out[f]
        if ex is None:
            assert int(o["exit"][i]) >= EMPTY_WINDOW, (label, int(o["exit"][i]))
        else:
            assert int(o["exit"][i]) == ex, (label, int(o["exit"][i]), ex)
        if idx is not None:
            assert int(o["best_idx"][i]) == idx, (label, int(o["best_idx"][i]), idx)
        if dist is not None:
            assert int(o["best_dist"][i]) == dist, (label, int(o["best_dist"][i]), dist)
    assert out[0]["level"][labels["z=+FLT_MIN,x=0"][1]] == 0 and out[1]["level"][0] == 0
    lv = [int(out[0]["level"][labels["ratio=1.2^%d%s" % (k, tag)][1]]) for k in range(9) for tag in ("-1ulp", "", "+1ulp")]
    assert lv == sorted(lv) and lv[0] == 0 and lv[-1] == 7 and set(lv) == set(range(8)), lv
