"""Shared by the map-point update tests: builds and calls the sequential CPU restatement (tests/host/map_point_restatement.cpp), an
independent numpy statement of the rule, the random problems and the constructed points.  Not a test
module."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from geoflowslam_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "map_point_restatement.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_map_point_restatement.so")
_L = None

FIELDS = ("best_obs", "best_median", "normal", "min_dist", "max_dist", "status")
NORMAL_FIELDS = ("normal", "min_dist", "max_dist")
# the observation counts at which the kernel changes what it does: none, the short lists, the 64-lane chunk edges of the normal's
# walk and of the median's two paths, and a long list
COUNTS = (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300)
N_POINTS = (0, 1, 63, 64, 65, 257, 1000)


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
        L.mr_update.argtypes = [C.POINTER(api.MapPointsProblem), C.POINTER(api.MapPointsResult), C.c_void_p]
        L.mr_update.restype = C.c_int
        L.mr_constants.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.mr_constants.restype = None
        _L = L
    return _L


def restate(prob, normals_only=False, with_ties=False):
    """The restatement on a problem dict -> the dict api.MapPointUpdater.update returns (and the rows sharing the best median)."""
    P, R, keep = api.map_points_structs(prob, normals_only)
    ties = np.zeros(max(P.n_points, 1), np.int32)
    assert restatement().mr_update(C.byref(P), C.byref(R), ties.ctypes.data) == 0
    out = api.map_points_results(P, keep)
    return (out, ties[:P.n_points]) if with_ties else out


def same_bits(a, b):
    """Bit equality; two NaNs are the same value whatever their sign and payload, which IEEE 754 leaves to the implementation."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        return bool((na == nb).all()) and a[~na].tobytes() == b[~nb].tobytes()
    return a.tobytes() == b.tobytes()


def assert_equal(got, want, what="", fields=FIELDS):
    for k in fields:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert same_bits(g, w), (what, k, [(int(i), g[i].tolist(), w[i].tolist()) for i in np.nonzero((g != w).reshape(len(g), -1).any(1))[0][:4]])


def _norm(v):
    f = np.float32
    return f(np.sqrt(f(f(f(v[0] * v[0]) + f(v[1] * v[1])) + f(v[2] * v[2]))))


def numpy_statement(prob, normals_only=False):
    """DESIGN.md section 15 in numpy, point after point: the Hamming table from unpacked bits, np.sort of every row, the element
    int(0.5 * (N - 1)), the first argmin; the normal and the depths in numpy.float32 scalars, one operation at a time."""
    f = np.float32
    start = np.asarray(prob["obs_start"], np.int64)
    n = len(start) - 1
    Ow = np.ascontiguousarray(prob["obs_Ow"], f).reshape(-1, 3)
    flags = np.asarray(prob["obs_flags"], np.uint8)
    pos, ref = np.ascontiguousarray(prob["pos"], f).reshape(-1, 3), np.ascontiguousarray(prob["ref_Ow"], f).reshape(-1, 3)
    ls, ms = np.asarray(prob["level_scale"], f), np.asarray(prob["max_scale"], f)
    out = dict(best_obs=np.full(n, -1, np.int32), best_median=np.full(n, -1, np.int32), normal=np.zeros((n, 3), f),
               min_dist=np.zeros(n, f), max_dist=np.zeros(n, f), status=np.zeros(n, np.uint8))
    with np.errstate(all="ignore"):
        for p in range(n):
            a, b = int(start[p]), int(start[p + 1])
            if a == b:
                continue
            if not normals_only:
                idx = np.nonzero(flags[a:b] & 2)[0]
                if len(idx):
                    bits = np.unpackbits(np.ascontiguousarray(prob["obs_desc"], np.uint8).reshape(-1, 32)[a + idx], axis=1).astype(np.int32)
                    table = (bits[:, None, :] != bits[None, :, :]).sum(2)
                    med = np.sort(table, axis=1)[:, int(0.5 * (len(idx) - 1))]
                    row = int(np.argmin(med))
                    out["best_obs"][p], out["best_median"][p] = idx[row], med[row]
                    out["status"][p] |= 2
            s, cnt = [f(0), f(0), f(0)], 0
            for o in range(a, b):
                if not flags[o] & 1:
                    continue
                d = [f(pos[p][c] - Ow[o][c]) for c in range(3)]
                ln = _norm(d)
                s = [f(s[c] + f(d[c] / ln)) for c in range(3)]
                cnt += 1
            out["normal"][p] = [f(s[c] / f(cnt)) for c in range(3)]
            dist = _norm([f(pos[p][c] - ref[p][c]) for c in range(3)])
            out["max_dist"][p] = f(dist * ls[p])
            out["min_dist"][p] = f(out["max_dist"][p] / ms[p])
            out["status"][p] |= 1
    return out


def _bits(*ones):
    b = np.zeros(256, np.uint8)
    b[list(ones)] = 1
    return np.packbits(b)


@functools.lru_cache(maxsize=None)
def constructed():
    """One problem of hand-made points -> (problem, {label: point index}).  Every observation carries both flags unless said."""
    rng = np.random.default_rng(7)
    pts, labels = [], {}
    ZERO, ONES = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)

    def add(label, descs, pos=None, Ow=None, ref=None, flags=None):
        n = len(descs)
        labels[label] = len(pts)
        pts.append(dict(desc=np.array(descs, np.uint8).reshape(n, 32), pos=np.array(pos if pos is not None else rng.uniform(2, 6, 3), np.float32),
                        Ow=np.array(Ow if Ow is not None else rng.normal(size=(n, 3)), np.float32).reshape(n, 3),
                        ref=None if ref is None else np.array(ref, np.float32), flags=np.array(flags if flags is not None else [3] * n, np.uint8)))

    rnd = lambda n: rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    for n in (1, 2, 3, 4):
        add(f"N={n}", rnd(n))
    add("identical", [rnd(1)[0]] * 5)
    # d01 = 10, d02 = 30, d12 = 24: rows 0 and 1 share the median 10, row 1 has the smaller sum (34 < 40); the first wins
    add("equal median, later smaller sum", [ZERO, _bits(*range(10)), _bits(*range(8), *range(10, 32))])
    # N = 4: the median is the smallest distance to another row; without the row's own 0 it would be the second smallest
    for seed in range(1000):
        r = np.random.default_rng(seed)
        base = np.unpackbits(r.integers(0, 256, size=32, dtype=np.uint8))
        d = []
        for _ in range(4):
            b = base.copy()
            b[r.choice(256, size=int(r.integers(0, 60)), replace=False)] ^= 1
            d.append(np.packbits(b))
        bits = np.unpackbits(np.array(d), axis=1).astype(np.int32)
        t = np.sort((bits[:, None] != bits[None]).sum(2), axis=1)
        if np.argmin(t[:, 1]) != np.argmin(t[:, 2]) and len(set(t[:, 1])) == 4:
            break
    add("self-distance counts", d)
    add("distance 256", [ZERO, ONES, ONES])                 # row 0's median is 256
    add("distance 256, long", [ZERO] + [ONES] * 64)         # ... on the long-list path
    add("Pos == Ow", rnd(3), pos=[1, 2, 3], Ow=[[0, 0, 0], [1, 2, 3], [2, 0, 1]])
    add("Pos == ref Ow", rnd(3), pos=[1, 2, 3], ref=[1, 2, 3])
    add("no IN_DESC", rnd(3), flags=[1, 1, 1])
    add("no flag at all", rnd(2), flags=[0, 0])            # n = 0 of a list that is not empty: 0 / 0
    add("IN_DESC skips the first", rnd(4), flags=[1, 3, 3, 3])
    add("empty", rnd(0))
    start = np.cumsum([0] + [len(q["desc"]) for q in pts]).astype(np.int32)
    prob = dict(obs_start=start, obs_Ow=np.concatenate([q["Ow"] for q in pts]), obs_desc=np.concatenate([q["desc"] for q in pts]),
                obs_flags=np.concatenate([q["flags"] for q in pts]), pos=np.array([q["pos"] for q in pts], np.float32),
                ref_Ow=np.array([q["ref"] if q["ref"] is not None else (q["Ow"][0] if len(q["Ow"]) else [0, 0, 0]) for q in pts], np.float32),
                level_scale=np.full(len(pts), np.float32(1.2) ** 3, np.float32), max_scale=np.full(len(pts), np.float32(1.2) ** 7, np.float32))
    return prob, labels


def check_constructed(prob, labels, out):
    """What the constructed points were made for, on any implementation's output."""
    at = lambda label: labels[label]
    bo, bm = out["best_obs"], out["best_median"]
    assert [int(bo[at(f"N={n}")]) >= 0 for n in (1, 2, 3, 4)] == [True] * 4
    assert bo[at("N=1")] == 0 and bm[at("N=1")] == 0
    assert bo[at("N=2")] == 0 and bm[at("N=2")] == 0       # index int(0.5 * 1) = 0: the row's own 0
    assert bm[at("N=3")] > 0 and bm[at("N=4")] > 0          # index 1: the nearest other row (even N: the lower middle)
    assert bo[at("identical")] == 0 and bm[at("identical")] == 0
    assert bo[at("equal median, later smaller sum")] == 0 and bm[at("equal median, later smaller sum")] == 10
    a = int(prob["obs_start"][at("self-distance counts")])
    bits = np.unpackbits(prob["obs_desc"][a:a + 4], axis=1).astype(np.int32)
    t = np.sort((bits[:, None] != bits[None]).sum(2), axis=1)
    assert bo[at("self-distance counts")] == np.argmin(t[:, 1]) != np.argmin(t[:, 2]) and bm[at("self-distance counts")] == t[:, 1].min()
    for label in ("distance 256", "distance 256, long"):
        assert bo[at(label)] == 1 and bm[at(label)] == 0
    assert np.isnan(out["normal"][at("Pos == Ow")]).all() and out["status"][at("Pos == Ow")] == 3
    assert out["max_dist"][at("Pos == ref Ow")] == 0 and out["min_dist"][at("Pos == ref Ow")] == 0
    assert bo[at("no IN_DESC")] == -1 and bm[at("no IN_DESC")] == -1 and out["status"][at("no IN_DESC")] == 1
    assert np.isnan(out["normal"][at("no flag at all")]).all() and out["status"][at("no flag at all")] == 1
    assert bo[at("IN_DESC skips the first")] >= 1
    e = at("empty")
    assert out["status"][e] == 0 and bo[e] == -1 and not out["normal"][e].any() and out["max_dist"][e] == 0


@functools.lru_cache(maxsize=None)
def uniform(count):
    prob = synth.map_point_update_problem(900 + count, n_points=5, obs_counts=count, n_keyframes=48)
    return prob, restate(prob)


@functools.lru_cache(maxsize=None)
def mixed():
    counts = np.array(COUNTS + COUNTS[::-1], np.int64)
    prob = synth.map_point_update_problem(977, n_points=len(counts), obs_counts=counts, n_keyframes=48)
    return prob, restate(prob)


@functools.lru_cache(maxsize=None)
def sized(n_points):
    prob = synth.map_point_update_problem(1200 + n_points, n_points=n_points, obs_counts=(1, 20))
    return prob, restate(prob)


def random_problem(seed):
    """The problems of the CPU tests: counts from 0 to 300, most of them short."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(20, 60))
    counts = np.where(rng.random(n) < 0.15, rng.integers(40, 301, size=n), rng.integers(0, 24, size=n))
    return synth.map_point_update_problem(seed, n_points=n, obs_counts=counts, n_keyframes=int(rng.integers(20, 80)))
