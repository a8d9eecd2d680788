"""Shared by the tests of the Sim3 searches of loop closing (gfs_sim3_search): builds and calls the sequential
CPU restatement (tests/host/sim3_search_restatement.cpp), an independent numpy.float32 statement of the per-(point, problem) rule
with a live taken array, the random problems and the constructed points.  Not a test module."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import fuse_support as FS
from fuse_support import _down, _flip, _up, libm_logf, predict_level, same_bits  # noqa: F401
from geoflowslam_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "sim3_search_restatement.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_sim3_search_restatement.so")
_L = None

EXITS = api.SIM3_SEARCH_EXITS
NEG_DEPTH, NOT_IN_IMAGE, TOO_NEAR, TOO_FAR, VIEW_ANGLE, EMPTY_WINDOW, NO_CANDIDATE, MATCHED, SKIPPED = range(9)
FUSE, SBP, SBP_KFS = api.SIM3_FUSE, api.SIM3_SBP, api.SIM3_SBP_KFS
MODES = (FUSE, SBP, SBP_KFS)
MODE_NAMES = {FUSE: "fuse", SBP: "sbp", SBP_KFS: "sbp_kfs"}
LISTED = api.SIM3_SEARCH_LISTED
INT_MAX = api.INT_MAX
STATS = ("ties", "ties_other_cell", "taken_skips", "displaced", "displaced_by_earlier")


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
        L.sr_sim3_search.argtypes = [C.POINTER(api.FusePoints), C.c_int, C.POINTER(api.Sim3SearchProblem), C.c_int,
                                     C.POINTER(api.Sim3SearchResult), vp]
        L.sr_sim3_search.restype = C.c_int
        L.sr_sim3_point.argtypes = [C.POINTER(api.Sim3SearchProblem), vp, vp, C.c_float, C.c_float, vp, vp, vp]
        L.sr_sim3_point.restype = None
        L.sr_constants.argtypes = [vp]
        _L = L
    return _L


def restate(prob, with_stats=False):
    """The restatement on a problem dict (lists, problems) -> the list of dicts api.ProjectionMatcher.sim3_search returns."""
    LL, PP, RR, keep = api.sim3_search_structs(prob["lists"], prob["problems"])
    stats = np.zeros(len(STATS), np.int64)
    rc = restatement().sr_sim3_search(LL, len(prob["lists"]), PP, len(prob["problems"]), RR, stats.ctypes.data)
    assert rc == 0
    out = api.sim3_search_results(LL, PP, RR, keep, len(prob["lists"]))
    return (out, dict(zip(STATS, (int(v) for v in stats)))) if with_stats else out


def assert_equal(got, want, what=""):
    """Bit equality of everything gfs_sim3_search delivers, problem by problem; level where it is defined (the window was reached)."""
    assert len(got) == len(want), what
    for f, (g, w) in enumerate(zip(got, want)):
        assert g["n_matched"] == w["n_matched"], (what, f, "n_matched", g["n_matched"], w["n_matched"])
        for k in ("exit", "best_idx", "best_dist"):
            assert same_bits(g[k], w[k]), (what, f, k, np.nonzero(np.asarray(g[k]) != np.asarray(w[k]))[0][:8])
        d = (w["exit"] >= EMPTY_WINDOW) & (w["exit"] <= MATCHED)
        assert same_bits(g["level"][d], w["level"][d]), (what, f, "level")


def numpy_statement(prob):
    """DESIGN.md section 20 in numpy.float32 scalars, point after point: every operation one float32 rounding, sums left to right,
    the viewing-angle gate compared in float64, the acceptance test of the projection modes a float32 product; logf through ctypes
    on libm; the grid a dict of cells; the taken set a Python set that grows with every match."""
    f, d64 = np.float32, np.float64
    out = []
    for pr in prob["problems"]:
        mode = int(pr["mode"])
        pts = prob["lists"][int(pr.get("list", 0))]
        xw = np.ascontiguousarray(pts["mp_xw"], f).reshape(-1, 3)
        nrm = np.ascontiguousarray(pts["mp_normal"], f).reshape(-1, 3)
        desc = np.ascontiguousarray(pts["mp_desc"], np.uint8).reshape(-1, 32)
        q, t, Ow = (np.asarray(pr[k], f) for k in ("Tcw_q", "Tcw_t", "Ow"))
        g = {k: f(pr[k]) for k in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "grid_w_inv", "grid_h_inv", "log_scale_factor", "th")}
        ratio = f(pr.get("ratio_hamming", 1.0))
        scale = np.asarray(pr["scale_factors"], f)
        nl = int(pr.get("n_levels", len(scale)))
        kps = pr["kps_un"]
        kbits = np.unpackbits(np.ascontiguousarray(pr["desc"], np.uint8).reshape(-1, 32), axis=1)
        taken = set(np.nonzero(np.asarray(pr["kp_taken"]))[0].tolist()) if pr.get("kp_taken") is not None else set()
        skip = np.asarray(pr["mp_skip"]) if pr.get("mp_skip") is not None else None
        cells = {}
        with np.errstate(all="ignore"):
            for j in range(len(kps)):
                vx, vy = f(f(kps["x"][j] - g["min_x"]) * g["grid_w_inv"]), f(f(kps["y"][j] - g["min_y"]) * g["grid_h_inv"])
                px = int(np.floor(abs(float(vx)) + 0.5) * (1 if vx >= 0 else -1))  # round half away from zero
                py = int(np.floor(abs(float(vy)) + 0.5) * (1 if vy >= 0 else -1))
                if 0 <= px < 64 and 0 <= py < 48:
                    cells.setdefault((px, py), []).append(j)
        n = len(xw)
        first = INT_MAX if mode == FUSE else 256
        ex_, bi, bd, lv = np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.full(n, first, np.int32), np.zeros(n, np.int32)
        with np.errstate(all="ignore"):
            for i in range(n):
                if skip is not None and skip[i]:
                    ex_[i] = SKIPPED
                    continue
                P, Pn = xw[i], nrm[i]
                Pc = [f(a + t[k]) for k, a in enumerate(FS._so3_act(q, P))]
                if Pc[2] < f(0):
                    ex_[i] = NEG_DEPTH
                    continue
                if mode == SBP_KFS:
                    invz = f(f(1) / Pc[2])
                    u = f(f(g["fx"] * f(Pc[0] * invz)) + g["cx"])
                    v = f(f(g["fy"] * f(Pc[1] * invz)) + g["cy"])
                else:
                    u = f(f(f(g["fx"] * Pc[0]) / Pc[2]) + g["cx"])
                    v = f(f(f(g["fy"] * Pc[1]) / Pc[2]) + g["cy"])
                if not (u >= g["min_x"] and u < g["max_x"] and v >= g["min_y"] and v < g["max_y"]):
                    ex_[i] = NOT_IN_IMAGE
                    continue
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
                            if mode != FUSE and j in taken:
                                continue
                            o = int(kps["octave"][j])
                            if o < level - 1 or o > level:
                                continue
                            dd = int((pbits != kbits[j]).sum())
                            if dd < bd[i]:
                                bd[i], bi[i] = dd, j
                if any_in:
                    ok = bd[i] <= 50 if mode == FUSE else f(bd[i]) <= f(f(50) * ratio)
                    ex_[i] = MATCHED if ok else NO_CANDIDATE
                    if ok and mode != FUSE:
                        taken.add(int(bi[i]))
        out.append(dict(exit=ex_, best_idx=bi, best_dist=bd, level=lv, n_matched=int((ex_ == MATCHED).sum())))
    return out


# The random problems of the tests: every wave and workgroup boundary (64 lanes, 256 threads) crossed with n_kp in {0, 1, 500}.
N_MP = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
N_KP = (0, 1, 500)
CASES = [(m, n, c) for m in MODES for n in N_MP for c in N_KP]


@functools.lru_cache(maxsize=None)
def problem(mode, n_mp, n_kp, n_problems=1, seed=None, masks=True, **kw):
    """(problem dict, restatement output, restatement stats), computed once and shared; the arrays must not be modified."""
    s = (n_mp * 7 + n_kp + 1000 * n_problems + 31 * mode) if seed is None else seed
    prob = synth.sim3_search_problem(s, mode, n_points=n_mp, n_kp=n_kp, n_problems=n_problems, masks=masks, **kw)
    out, st = restate(prob, with_stats=True)
    return prob, out, st


@functools.lru_cache(maxsize=None)
def five_problems():
    """One list against five problems of different pose, th, ratio and mode."""
    a = synth.sim3_search_problem(701, SBP, n_points=700, n_kp=600, n_problems=3)
    b = synth.sim3_search_problem(701, SBP, n_points=700, n_kp=450, n_problems=3, scale_factor=1.1)  # same seed: same poses and points
    f = np.float32
    ps = [dict(a["problems"][0], mode=SBP_KFS, th=f(8), ratio_hamming=f(1.5)), dict(b["problems"][1], mode=FUSE, th=f(4), kp_taken=None),
          dict(a["problems"][2], mode=SBP, th=f(3), ratio_hamming=f(1.5)), dict(b["problems"][0], mode=SBP, th=f(5), ratio_hamming=f(1.0)),
          dict(a["problems"][1], mode=FUSE, th=f(2.5), kp_taken=None, mp_skip=None)]
    prob = dict(lists=a["lists"], problems=ps)
    return prob, restate(prob)


@functools.lru_cache(maxsize=None)
def two_lists():
    """Two lists of different lengths in one call: three problems on the long one, two on the short one, interleaved, modes mixed."""
    a = synth.sim3_search_problem(801, SBP_KFS, n_points=777, n_kp=500, n_problems=3)
    b = synth.sim3_search_problem(802, SBP, n_points=130, n_kp=300, n_problems=2)
    ps = [dict(a["problems"][0], list=0), dict(b["problems"][0], list=1), dict(a["problems"][1], list=0, mode=FUSE, kp_taken=None),
          dict(b["problems"][1], list=1), dict(a["problems"][2], list=0)]
    prob = dict(lists=[a["lists"][0], b["lists"][0]], problems=ps)
    return prob, restate(prob)


# ---- constructed points: each sits exactly on one decision of the rule ----
def projection_pair():
    """A camera-frame point (fx = 607, cx = 319.5) whose two projection forms give different u: fx * X / Z + cx against
    fx * (X * (1 / Z)) + cx, found by a seeded search -> (X, Y, Z, u of Pinhole::project, u of the invz form)."""
    f = np.float32
    rng = np.random.default_rng(99)
    fx, cx = f(607.0), f(319.5)
    for _ in range(10000):
        X, Z = f(rng.uniform(-0.4, 0.4)), f(rng.uniform(1.0, 3.0))
        ua = f(f(f(fx * X) / Z) + cx)
        ub = f(f(fx * f(X * f(f(1) / Z))) + cx)
        if ua != ub and 10 < ua < 630:
            return X, f(0.125), Z, ua, ub
    raise AssertionError("no point found on which the two projection forms differ")


@functools.lru_cache(maxsize=None)
def constructed():
    """-> (problem dict, {(problem, label): (problem, point index, expected exit or None = reaches the window, best_idx or None, best_dist or None)}).

    Problems 0 (FUSE), 1 (SBP, ratio 1.5), 2 (SBP_KFS, ratio 1.5) and 3 (SBP, ratio 1.0) share key frame A of
    fuse_support.constructed: a camera at the origin looking along z, q = (0, 0, 0, 1), t = 0, fx = fy = 1, cx = cy = 0, so a point
    (x, y, 1) projects to u = x, v = y exactly in both projection forms (1 / 1 = 1).  Each problem has a list of its own.  The gate
    points (bounds, depth, distance, angle, level) are in the lists of problems 0, 1 and 2 alike.  Searched points sit 40 pixels
    apart, far more than any window (th = 3).  Problems 4 (FUSE), 5 (SBP) and 6 (SBP_KFS) are a VGA camera with one point on which
    the two projection forms differ in u."""
    f = np.float32
    rng = np.random.default_rng(2025)
    n_levels = 8
    scale = np.cumprod(np.r_[1.0, np.full(n_levels - 1, 1.2)]).astype(np.float32)
    log_sf = libm_logf(f(1.2))
    min_x, max_x, min_y, max_y = f(-300.5), f(339.5), f(-220.25), f(259.75)
    FLT_MIN = FS.FLT_MIN
    labels = {}
    lists = [[] for _ in range(4)]   # per problem: (P, normal, min, max, desc)
    kps = [[] for _ in range(4)]     # per problem: (x, y, octave, desc, taken)

    def facing(P):
        P = np.array(P, np.float64)
        nrm = np.linalg.norm(P)
        return tuple(P / nrm) if nrm > 0 else (0.0, 0.0, 1.0)

    def add(p, label, P, n=None, mn=0.0, mx=1000.0, exit=None, idx=None, dist=None, desc=None):
        labels[(p, label)] = (p, len(lists[p]), exit, idx, dist)
        lists[p].append((np.array(P, f), np.array(facing(P) if n is None else n, f), f(mn), f(mx),
                         rng.integers(0, 256, 32, dtype=np.uint8) if desc is None else np.array(desc, np.uint8)))
        return lists[p][-1][4]

    def add_kp(p, x, y, octave, desc, taken=0):
        kps[p].append((f(x), f(y), int(octave), np.array(desc, np.uint8), taken))
        return len(kps[p]) - 1

    for p in (0, 1, 2):
        for name, axis, lo, hi in (("u", 0, min_x, max_x), ("v", 1, min_y, max_y)):
            for tag, val, inside in (("==min", lo, True), ("<min", _down(lo), False), ("==max", hi, False), ("<max", _down(hi), True)):
                P = [f(3), f(2), f(1)]
                P[axis] = val
                add(p, name + tag, P, exit=None if inside else NOT_IN_IMAGE)
        add(p, "z=+0,x=0", (0.0, 0.0, 0.0), exit=NOT_IN_IMAGE)   # 0 / 0: NaN fails IsInImage by itself
        add(p, "z=+0,x=1", (1.0, 1.0, 0.0), exit=NOT_IN_IMAGE)   # 1 / 0 (or 1 * inf): inf fails it too
        add(p, "z=-FLT_MIN,x=0", (0.0, 0.0, -FLT_MIN), n=(0, 0, 1), exit=NEG_DEPTH)
        add(p, "z=-FLT_MIN,x=1", (1.0, 1.0, -FLT_MIN), exit=NEG_DEPTH)
        m, M = f(3.7), f(2.3)
        d_near, d_far = f(f(0.8) * m), f(f(1.2) * M)
        add(p, "dist==0.8min", (0, 0, d_near), mn=m, mx=100.0)
        add(p, "dist<0.8min", (0, 0, _down(d_near)), mn=m, mx=100.0, exit=TOO_NEAR)
        add(p, "dist==1.2max", (0, 0, d_far), mn=0.0, mx=M)
        add(p, "dist>1.2max", (0, 0, _up(d_far)), mn=0.0, mx=M, exit=TOO_FAR)
        add(p, "dot==half", (0, 0, 2), n=(0, 0, 0.5))
        add(p, "dot<half", (0, 0, 2), n=(0, 0, _down(0.5)), exit=VIEW_ANGLE)
        add(p, "dot>half", (0, 0, 2), n=(0, 0, _up(0.5)))
        pk = f(1)
        for k in range(n_levels + 1):
            for tag, r in (("-1ulp", _down(pk)), ("", pk), ("+1ulp", _up(pk))):
                add(p, "ratio=1.2^%d%s" % (k, tag), (0, 0, 2), mx=f(f(2) * r))
            pk = f(pk * f(1.2))

    slot = [0, 0, 0, 0]

    def place(p):
        """the next free position of problem p's 40-pixel lattice right of the image centre"""
        n = slot[p]
        slot[p] += 1
        assert n < 88
        return f(20 + 40 * (n % 8)), f(-200 + 40 * (n // 8))

    def searched(p, label, level=2, u=None, v=None, desc=None):
        pu, pv = place(p) if (u is None or v is None) else (u, v)
        u = pu if u is None else f(u)
        v = pv if v is None else f(v)
        dist = np.sqrt(f(f(f(u * u) + f(v * v)) + f(1)))
        mx = f(float(dist) * 1.2 ** (level - 0.5))
        assert predict_level(mx, dist, log_sf, n_levels) == level
        d = add(p, label, (u, v, 1), mx=mx, desc=desc)
        return u, v, d

    def expect(p, label, *e):
        labels[(p, label)] = labels[(p, label)][:2] + e

    for p in (0, 1, 2):
        nothing = (-1, INT_MAX) if p == 0 else (-1, 256)
        # octave = level - 2 .. level + 1
        for k, ok in ((-2, False), (-1, True), (0, True), (1, False)):
            label = "octave=level%+d" % k
            u, v, d = searched(p, label)
            j = add_kp(p, u, v, 2 + k, _flip(d, 5))
            expect(p, label, *((MATCHED, j, 5) if ok else (NO_CANDIDATE,) + nothing))
        # a candidate at Hamming distance 256: INT_MAX lets it in (best_idx set, not matched), 256 does not
        u, v, d = searched(p, "dist=256")
        j = add_kp(p, u, v, 2, _flip(d, 256))
        expect(p, "dist=256", NO_CANDIDATE, *((j, 256) if p == 0 else (-1, 256)))
        # ties: different columns (the first VISITED wins, and it has the higher index), different rows, one cell
        u, v, d = searched(p, "tie_columns", u=min_x + f(205))
        add_kp(p, u + f(2), v, 2, _flip(d, 9, 100))
        j = add_kp(p, u - f(2), v, 2, _flip(d, 9))
        expect(p, "tie_columns", MATCHED, j, 9)
        u, v, d = searched(p, "tie_rows", v=min_y + f(205))
        add_kp(p, u, v + f(2), 2, _flip(d, 9, 100))
        j = add_kp(p, u, v - f(2), 2, _flip(d, 9))
        expect(p, "tie_rows", MATCHED, j, 9)
        u, v, d = searched(p, "tie_cell")
        j = add_kp(p, u + f(0.25), v, 2, _flip(d, 9))
        add_kp(p, u - f(0.25), v, 2, _flip(d, 9, 100))
        expect(p, "tie_cell", MATCHED, j, 9)
    # the acceptance tests: TH_LOW in Fuse; 50 * 1.5 = 75 and 50 * 1.0 = 50 in the projection searches
    for p, edge in ((0, 50), (1, 75), (2, 75), (3, 50)):
        for nb in (edge, edge + 1):
            label = "dist=%d" % nb
            u, v, d = searched(p, label)
            j = add_kp(p, u, v, 2, _flip(d, nb))
            expect(p, label, MATCHED if nb == edge else NO_CANDIDATE, j, nb)
    for p in (1, 2, 3):
        # the best key-point is taken at entry: the second best wins
        u, v, d = searched(p, "best_taken")
        add_kp(p, u, v, 2, _flip(d, 2), taken=1)
        j = add_kp(p, u + f(0.5), v, 2, _flip(d, 6))
        expect(p, "best_taken", MATCHED, j, 6)
        # the only candidate is taken: the window is not empty, nothing survives
        u, v, d = searched(p, "only_taken")
        add_kp(p, u, v, 2, _flip(d, 2), taken=1)
        expect(p, "only_taken", NO_CANDIDATE, -1, 256)
        # a chain: LISTED + 2 points on one pixel with one descriptor against LISTED + 2 key-points at distances 1, 2, ...: point i
        # gets key-point i (beyond what the device lists per point), and one more point gets none
        cu, cv = place(p)
        cd = rng.integers(0, 256, 32, dtype=np.uint8)
        js = [add_kp(p, cu + f(0.125) * (c - 2), cv, 2, _flip(cd, c + 1)) for c in range(LISTED + 2)]
        for c in range(LISTED + 3):
            searched(p, "chain%d" % c, u=cu, v=cv, desc=cd)
            expect(p, "chain%d" % c, *((MATCHED, js[c], c + 1) if c < LISTED + 2 else (NO_CANDIDATE, -1, 256)))
        # an equal-distance pair in different columns and two points: the first visited goes to the first, the other to the second
        # (left of the image centre, where no lattice point is; x - min_x = 243 -> column 24, 247 -> column 25)
        tu, tv = min_x + f(245), place(p)[1]
        td = rng.integers(0, 256, 32, dtype=np.uint8)
        j_right = add_kp(p, tu + f(2), tv, 2, _flip(td, 9, 100))
        j_left = add_kp(p, tu - f(2), tv, 2, _flip(td, 9))
        for c, j in ((0, j_left), (1, j_right)):
            searched(p, "tie_pair%d" % c, u=tu, v=tv, desc=td)
            expect(p, "tie_pair%d" % c, MATCHED, j, 9)
    # chain in FUSE mode: no dependency, every point gets key-point 0
    cu, cv = place(0)
    cd = rng.integers(0, 256, 32, dtype=np.uint8)
    js = [add_kp(0, cu + f(0.125) * (c - 2), cv, 2, _flip(cd, c + 1)) for c in range(LISTED + 2)]
    for c in range(LISTED + 3):
        searched(0, "chain%d" % c, u=cu, v=cv, desc=cd)
        expect(0, "chain%d" % c, MATCHED, js[0], 1)

    def lst(ps):
        return dict(mp_xw=np.array([q[0] for q in ps], f), mp_normal=np.array([q[1] for q in ps], f), mp_min_dist=np.array([q[2] for q in ps], f),
                    mp_max_dist=np.array([q[3] for q in ps], f), mp_desc=np.array([q[4] for q in ps], np.uint8))

    def kf(p, mode, ratio):
        k = np.zeros(len(kps[p]), api.KP_DTYPE)
        k["x"], k["y"], k["octave"] = [c[0] for c in kps[p]], [c[1] for c in kps[p]], [c[2] for c in kps[p]]
        k["size"], k["class_id"] = 31.0, -1
        return dict(mode=mode, ratio_hamming=f(ratio), Tcw_q=np.array([0, 0, 0, 1], f), Tcw_t=np.zeros(3, f), Ow=np.zeros(3, f), fx=f(1), fy=f(1),
                    cx=f(0), cy=f(0), min_x=min_x, max_x=max_x, min_y=min_y, max_y=max_y, grid_w_inv=f(64) / f(max_x - min_x),
                    grid_h_inv=f(48) / f(max_y - min_y), scale_factors=scale, n_levels=n_levels, log_scale_factor=log_sf, th=f(3), kps_un=k,
                    desc=np.array([c[3] for c in kps[p]], np.uint8).reshape(-1, 32),
                    kp_taken=None if mode == FUSE else np.array([c[4] for c in kps[p]], np.uint8), mp_skip=None, list=p)

    problems = [kf(0, FUSE, 1.0), kf(1, SBP, 1.5), kf(2, SBP_KFS, 1.5), kf(3, SBP, 1.0)]
    # The two projection forms on one point (problems 4 FUSE, 5 SBP, 6 SBP_KFS; a VGA camera at the origin): level 0, so the radius
    # is th = 3 exactly.  Key-point 0 sits exactly 3 pixels from Pinhole::project's u on the side of the invz form's u -- not inside
    # the first window (`<` is strict), inside the second by the one ulp the forms differ in -- and key-point 1 the other way round.
    X, Y, Z, ua, ub = projection_pair()
    fx, cx, cy = f(607.0), f(319.5), f(239.5)
    va = f(f(f(fx * Y) / Z) + cy)
    sgn = f(1) if ub > ua else f(-1)
    k0, k1 = f(ua + sgn * f(3)), f(ub - sgn * f(3))
    assert abs(f(k0 - ua)) == 3 and abs(f(k0 - ub)) < 3 and abs(f(k1 - ub)) == 3 and abs(f(k1 - ua)) < 3
    P = np.array((X, Y, Z), f)
    dist = np.sqrt(f(f(f(X * X) + f(Y * Y)) + f(Z * Z)))
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    k = np.zeros(2, api.KP_DTYPE)
    k["x"], k["y"], k["octave"], k["size"], k["class_id"] = [k0, k1], va, 0, 31.0, -1
    V = dict(Tcw_q=np.array([0, 0, 0, 1], f), Tcw_t=np.zeros(3, f), Ow=np.zeros(3, f), fx=fx, fy=fx, cx=cx, cy=cy, min_x=f(0), max_x=f(640),
             min_y=f(0), max_y=f(480), grid_w_inv=f(64) / f(640), grid_h_inv=f(48) / f(480), scale_factors=scale, n_levels=n_levels,
             log_scale_factor=log_sf, th=f(3), kps_un=k, desc=np.stack([d, d]), kp_taken=None, mp_skip=None, list=4, ratio_hamming=f(1.5))
    lists.append([(P, np.array(facing(P), f), f(0), f(float(dist) * 1.2 ** -0.5), d)])
    problems += [dict(V, mode=FUSE), dict(V, mode=SBP), dict(V, mode=SBP_KFS)]
    for p, j in ((4, 1), (5, 1), (6, 0)):
        labels[(p, "projection")] = (p, 0, MATCHED, j, 0)
    prob = dict(lists=[lst(q) for q in lists], problems=problems)
    return prob, labels, dict(u_pinhole=float(ua), u_invz=float(ub))


def check_constructed(prob, labels, out):
    """The expectations written next to the points, on any implementation's output."""
    for (p, label), (f, i, ex, idx, dist) in labels.items():
        o = out[f]
        if ex is None:
            assert EMPTY_WINDOW <= int(o["exit"][i]) <= MATCHED, (p, label, int(o["exit"][i]))
        else:
            assert int(o["exit"][i]) == ex, (p, label, int(o["exit"][i]), ex)
        if idx is not None:
            assert int(o["best_idx"][i]) == idx, (p, label, int(o["best_idx"][i]), idx)
        if dist is not None:
            assert int(o["best_dist"][i]) == dist, (p, label, int(o["best_dist"][i]), dist)
    for p in (0, 1, 2):
        lv = [int(out[p]["level"][labels[(p, "ratio=1.2^%d%s" % (k, tag))][1]]) for k in range(9) for tag in ("-1ulp", "", "+1ulp")]
        assert lv == sorted(lv) and lv[0] == 0 and lv[-1] == 7 and set(lv) == set(range(8)), lv
