"""Shared by the Sim3Solver tests: builds and calls the sequential CPU restatement (tests/host/sim3_ransac_restatement.cpp) and the
adaptor harness (tests/host/sim3_ransac_adaptor_test.cpp), and constructs the cases the tests need, computed once and shared.  Not a
test module."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from geoflowslam_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RULE = os.path.join(ROOT, "geoflowslam_amd", "csrc", "sim3_ransac_rule.hpp")
_ABI = os.path.join(ROOT, "include", "gfs_abi.h")
_SRC = os.path.join(ROOT, "tests", "host", "sim3_ransac_restatement.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_sim3_ransac_restatement.so")
_L = None


def _build(so, src, deps, extra=()):
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", tmp, src, *extra], check=True)
        os.replace(tmp, so)
    return C.CDLL(so)


def restatement():
    global _L
    if _L is None:
        L = _build(_SO, _SRC, [_SRC, _RULE, _ABI])
        vp, i = C.c_void_p, C.c_int
        L.s3rr_solve.argtypes = [C.POINTER(api.Sim3RansacProblem), i, C.POINTER(api.Sim3RansacSolution), vp, vp]
        L.s3rr_compute_sim3.argtypes = [vp, vp, i, vp, vp, vp, vp, vp]
        L.s3rr_resolve_draws.argtypes = [i, vp, vp]
        L.s3rr_pick.argtypes = [vp, i, i, vp]
        L.s3rr_iterations.argtypes = [i, C.c_double, i, i]
        L.s3rr_constants.argtypes = [vp]
        _L = L
    return _L


def run(prob, early_stop=True):
    """The restatement on one problem dict -> result dict as api.Sim3RansacSolver.solve's (counts: -1 where the early stop left an
    iteration out), plus err1 / err2 [n]: both errors of every pair under the returned hypothesis."""
    P, S, keep, n = api.sim3_ransac_structs(prob)
    err1, err2 = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
    restatement().s3rr_solve(C.byref(P), int(early_stop), C.byref(S), err1.ctypes.data, err2.ctypes.data)
    res = api.sim3_ransac_result(S, keep, n)
    res["err1"], res["err2"] = err1[:n], err2[:n]
    return res


def compute_sim3(P1, P2, fix_scale):
    """The rule's ComputeSim3 on two triples [3 points, 3] -> R [3, 3], t [3], s, T12 [3, 4], T21 [3, 4] (float32)."""
    a, b = np.ascontiguousarray(P1, np.float32), np.ascontiguousarray(P2, np.float32)
    R, t, s, T12, T21 = np.zeros((3, 3), np.float32), np.zeros(3, np.float32), np.zeros(1, np.float32), np.zeros((3, 4), np.float32), np.zeros((3, 4), np.float32)
    restatement().s3rr_compute_sim3(a.ctypes.data, b.ctypes.data, int(fix_scale), *(x.ctypes.data for x in (R, t, s, T12, T21)))
    return R, t, s[0], T12, T21


def resolve_draws(n, r):
    r, out = np.ascontiguousarray(r, np.int32), np.zeros(3, np.int32)
    restatement().s3rr_resolve_draws(int(n), r.ctypes.data, out.ctypes.data)
    return out.tolist()


def pick(counts, min_inliers):
    c, out = np.ascontiguousarray(counts, np.int32), np.zeros(3, np.int32)
    restatement().s3rr_pick(c.ctypes.data, len(c), int(min_inliers), out.ctypes.data)
    return tuple(out.tolist())


def constants():
    out = np.zeros(6)
    restatement().s3rr_constants(out.ctypes.data)
    return dict(chi2=float(out[0]), default_probability=float(out[1]), default_min_inliers=int(out[2]), default_max_iterations=int(out[3]),
                jacobi_sweeps=int(out[4]), jacobi_eps=float(out[5]))


SOLUTION_KEYS = ("T12", "R12", "t12", "s12", "n_inliers", "iterations", "status", "inlier")


def solution_bytes(r):
    """Everything gfs_sim3_ransac_solve returns but the counts, as bytes."""
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in SOLUTION_KEYS)


def assert_same(dev, prob, what=""):
    """A device result against the restatement: the solution against the loop with its early stop, the counts against the loop
    without it; byte for byte."""
    ref, full = run(prob, early_stop=True), run(prob, early_stop=False)
    for k in SOLUTION_KEYS:
        assert np.ascontiguousarray(dev[k]).tobytes() == np.ascontiguousarray(ref[k]).tobytes(), (what, k, dev[k], ref[k])
    if ref["status"] != api.SIM3_RANSAC_TOO_FEW:
        assert (dev["counts"] == full["counts"]).all(), (what, "counts")
        ran = ref["counts"] >= 0
        assert ran.sum() == ref["iterations"] and (ref["counts"][ran] == full["counts"][ran]).all(), (what, "early-stop counts")
    assert solution_bytes(full) == solution_bytes(ref), (what, "the loop without its early stop returns another solution")
    return ref


# ---- hand-built problems: a clean cloud whose exact Sim3 makes every pair an inlier, so that a hypothesis's count is decided by which
# pairs are then spoiled


def clean_problem(seed, n, fix_scale=True, **kw):
    return synth.sim3_ransac_problem(seed, n_pairs=n, inlier_share=1.1, fix_scale=fix_scale, noise_px=0.0, **kw)


def with_draws(prob, draws, min_inliers=None):
    p = dict(prob)
    p["draws"] = np.ascontiguousarray(draws, np.int32).reshape(-1, 3)
    p["n_iterations"] = len(p["draws"])
    if min_inliers is not None:
        p["min_inliers"] = int(min_inliers)
    return p


def spoiled(prob, which, shift=1.0):
    """The pairs `which` made gross outliers: their point in camera 1 moved sideways by `shift` metres."""
    p = dict(prob)
    p["x3d_c1"] = prob["x3d_c1"].copy()
    p["x3d_c1"][list(which), 0] += np.float32(shift)
    return p


def draws_for(n, triple):
    """The draws (r0, r1, r2) that make the sampling pick the index triple (i0, i1, i2), by running the swap-with-back list."""
    avail, out = list(range(n)), []
    for idx in triple:
        r = avail.index(idx)
        out.append(r)
        avail[r] = avail[-1]
        avail.pop()
    return out


@functools.lru_cache(maxsize=None)
def hand_built():
    """name -> problem.  40 pairs, pairs 30..39 spoiled: a triple of clean pairs scores 30, a triple with a spoiled pair far fewer."""
    base = spoiled(clean_problem(11, 40), range(30, 40))
    good, bad, bad2 = draws_for(40, (0, 1, 2)), draws_for(40, (0, 1, 35)), draws_for(40, (3, 36, 4))
    cases = {}
    cases["n3_min3"] = with_draws(clean_problem(12, 3), [[0, 0, 0]], min_inliers=3)  # N == minInliers: one iteration, cannot converge
    cases["converges_at_0"] = with_draws(base, [good] + [bad] * 5, min_inliers=15)
    cases["converges_at_last"] = with_draws(base, [bad] * 4 + [bad2] * 3 + [good], min_inliers=15)
    cases["never_tied"] = with_draws(base, [bad, good, bad2, draws_for(40, (5, 6, 7)), bad], min_inliers=30)  # two score 30, not > 30
    for fs in (0, 1):
        p = with_draws(spoiled(clean_problem(13, 40, fix_scale=bool(fs), scale=1.01), range(30, 40)), [bad, good, bad2], min_inliers=15)
        cases[f"fix_scale_{fs}"] = p
    return cases


# ---- gfs_host::Sim3RansacSolver on mock key frames (tests/host/sim3_ransac_adaptor_test.cpp)

_ADAPTOR_SRC = os.path.join(ROOT, "tests", "host", "sim3_ransac_adaptor_test.cpp")
_ADAPTOR_SO = os.path.join(ROOT, "tests", "host", "_sim3_ransac_adaptor_test.so")


def adaptor_harness():
    libdir = os.path.dirname(api._LIB_PATH)
    deps = [_ADAPTOR_SRC, _SRC, _RULE, _ABI, os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp")]
    return _build(_ADAPTOR_SO, _ADAPTOR_SRC, deps, ["-L" + libdir, "-lgfs_hip", "-Wl,-rpath," + libdir])


KIND_NO_MATCH, KIND_PAIR, KIND_NO_MP1, KIND_BAD_MP1, KIND_BAD_MP2, KIND_NO_INDEX1, KIND_NO_INDEX2 = range(7)
FRONT_KINDS = [KIND_NO_MATCH, KIND_BAD_MP1, KIND_BAD_MP2, KIND_NO_MP1, KIND_NO_INDEX1, KIND_NO_INDEX2]


def adaptor_scene(seed, n_good=40, n_out=20, different_kfs=False, fix_scale=True, min_inliers=15, probability=0.99, max_iterations=300,
                  step=20, set_parameters=True, triples=None):
    """Three mock key frames (1, 2 and a covisible one) and N1 key-points of key frame 1, one of every kind the constructor's filter
    treats differently in front, then n_good pairs related by one Sim3 and n_out gross outliers.  The map of key frame 2 is the map of
    key frame 1 moved by a Sim3 (the drift a loop closes).  With different_kfs every pMP2 is indexed in key frame 2 or in the covisible
    one, whose level sigmas differ.  stream: the recorded rand() values; with `triples` (a list of pair-index triples) it is made so
    that iteration k draws triples[k]."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    N1, M = len(FRONT_KINDS) + n_good + n_out, len(FRONT_KINDS) + n_good + n_out + 7
    kind = np.full(N1, KIND_PAIR, np.int32)
    kind[:len(FRONT_KINDS)] = FRONT_KINDS
    cams = np.array([synth.intrinsics(640, 480), synth.intrinsics(640, 480), synth.intrinsics(1280, 720)], f32)
    pose = np.zeros((3, 12), f32)
    for k in range(3):
        pose[k, :9] = synth._rot(*(np.deg2rad(3.0 * k) * rng.uniform(-1, 1, 3))).astype(f32).ravel()
        pose[k, 9:] = (0.1 * k * rng.uniform(-1, 1, 3)).astype(f32)
    z = rng.uniform(1.5, 5.0, N1)
    pos1 = np.stack([rng.uniform(-0.4, 0.4, N1) * z, rng.uniform(-0.3, 0.3, N1) * z, z], 1)
    Rd, td, sd = synth._rot(*(np.deg2rad(8.0) * rng.uniform(-1, 1, 3))), 0.3 * rng.uniform(-1, 1, 3), 1.0 if fix_scale else 1.15
    pos2 = sd * pos1 @ Rd.T + td + 0.002 * rng.normal(size=(N1, 3))
    first_out = len(FRONT_KINDS) + n_good
    pos2[first_out:] += rng.uniform(0.5, 1.0, (n_out, 3)) * rng.choice([-1.0, 1.0], (n_out, 3))
    idx1, idx2 = rng.permutation(M)[:N1].astype(np.int32), rng.permutation(M)[:N1].astype(np.int32)
    kfm = (rng.integers(1, 3, N1) if different_kfs else np.ones(N1)).astype(np.int32)
    kp_oct = rng.integers(0, 8, (3, M)).astype(np.int32)
    sigma = np.stack([(f32(sf) ** np.arange(8, dtype=f32)) ** 2 for sf in (1.2, 1.25, 1.5)]).astype(f32)
    scene = dict(N1=N1, M=M, kind=kind, pos1=pos1.astype(f32), pos2=pos2.astype(f32), idx1=idx1, idx2=idx2, kfm=kfm, different_kfs=bool(different_kfs),
                 kp_oct=kp_oct, pose=pose, cam=cams, sigma=sigma, fix_scale=bool(fix_scale), set_parameters=bool(set_parameters),
                 probability=float(probability), min_inliers=int(min_inliers), max_iterations=int(max_iterations), step=int(step))
    n = int((kind == KIND_PAIR).sum())
    H = expected_iterations(scene, n)
    if triples is None:
        scene["stream"] = rng.integers(0, 2 ** 31, 3 * H + 5).astype(np.int32)
    else:
        assert len(triples) == H
        vals = []
        for t in triples:
            for k, r in enumerate(draws_for(n, t)):
                vals.append(int((r + 0.5) / (n - k) * 2 ** 31))
        scene["stream"] = np.array(vals + [0] * 5, np.int32)
    return scene


def expected_iterations(scene, n):
    args = (scene["probability"], scene["min_inliers"], scene["max_iterations"]) if scene["set_parameters"] else (0.99, 6, 300)
    return synth.sim3_ransac_iterations(n, *args)


def run_adaptor(scene, use_device=False, camera_kind=0, max_steps=64):
    L = adaptor_harness()
    N1 = scene["N1"]
    o = dict(flat_n=np.zeros(6, np.int32), x1=np.zeros((N1, 3), np.float32), x2=np.zeros((N1, 3), np.float32), max1=np.zeros(N1, np.float32),
             max2=np.zeros(N1, np.float32), indices1=np.zeros(N1, np.int32), draws=np.zeros((scene["max_iterations"], 3), np.int32),
             flags=np.zeros((max_steps, 4), np.int32), n_steps=np.zeros(1, np.int32), inliers=np.zeros(N1, np.uint8), est=np.zeros(13, np.float32),
             T=np.zeros(16, np.float32))
    ins1 = [np.ascontiguousarray(scene[k]) for k in ("kind", "pos1", "pos2", "idx1", "idx2", "kfm")]
    ins2 = [np.ascontiguousarray(scene[k]) for k in ("kp_oct", "pose", "cam", "sigma")]
    stream = np.ascontiguousarray(scene["stream"], np.int32)
    i, vp = C.c_int, C.c_void_p
    L.sim3_ransac_adaptor_test.argtypes = [i] * 3 + [vp] * 6 + [i] + [vp] * 4 + [i, i, i, C.c_double, i, i, i, vp, i, i] + [vp] * len(o)
    ret = L.sim3_ransac_adaptor_test(int(use_device), N1, scene["M"], *[a.ctypes.data for a in ins1], int(scene["different_kfs"]),
                                     *[a.ctypes.data for a in ins2], int(camera_kind), int(scene["fix_scale"]), int(scene["set_parameters"]),
                                     scene["probability"], scene["min_inliers"], scene["max_iterations"], scene["step"], stream.ctypes.data,
                                     len(stream), max_steps, *[v.ctypes.data for v in o.values()])
    o["ret"] = np.array([ret], np.int32)
    return o


def adaptor_constants():
    L = adaptor_harness()
    out = np.zeros(4)
    L.sim3_ransac_adaptor_constants.argtypes = [C.c_void_p]
    L.sim3_ransac_adaptor_constants(out.ctypes.data)
    return dict(probability=float(out[0]), max_iterations=int(out[1]), step=int(out[2]), bow_inliers=int(out[3]))


def expected_gather(scene):
    """The constructor's filter and gather (:43-116) stated independently in float32 -> (problem dict for the restatement with the draws
    the recorded stream gives, mvnIndices1)."""
    f32 = np.float32
    R = [scene["pose"][k, :9].reshape(3, 3) for k in range(3)]
    t = [scene["pose"][k, 9:] for k in range(3)]
    cam_pt = lambda k, p: np.array([f32(f32(f32(R[k][r, 0] * p[0]) + f32(R[k][r, 1] * p[1])) + f32(R[k][r, 2] * p[2])) + t[k][r] for r in range(3)], f32)
    rows, idx = [], []
    for i in range(scene["N1"]):
        if scene["kind"][i] != KIND_PAIR:  # no match; no pMP1; a bad point; a point without an index in its key frame
            continue
        kf = int(scene["kfm"][i]) if scene["different_kfs"] else 1
        s1 = scene["sigma"][0][scene["kp_oct"][0][scene["idx1"][i]]]
        s2 = scene["sigma"][kf][scene["kp_oct"][kf][scene["idx2"][i]]]  # pKFm's key-point and level sigmas ...
        rows.append((cam_pt(0, scene["pos1"][i]), cam_pt(1, scene["pos2"][i]),  # ... but pKF2's pose
                     f32(np.floor(9.210 * np.float64(s1))), f32(np.floor(9.210 * np.float64(s2)))))
        idx.append(i)
    n = len(rows)
    H = expected_iterations(scene, n)
    mi = scene["min_inliers"] if scene["set_parameters"] else 6
    draws = np.zeros((H, 3), np.int32)
    if n >= max(mi, 3):
        v = scene["stream"][:3 * H].astype(np.float64).reshape(H, 3)
        draws = (v / 2.0 ** 31 * (n - np.arange(3))).astype(np.int32)
    prob = dict(x3d_c1=np.array([r[0] for r in rows], f32).reshape(-1, 3), x3d_c2=np.array([r[1] for r in rows], f32).reshape(-1, 3),
                max_err1=np.array([r[2] for r in rows], f32), max_err2=np.array([r[3] for r in rows], f32), cam1=scene["cam"][0], cam2=scene["cam"][1],
                fix_scale=scene["fix_scale"], min_inliers=mi, n_iterations=H, draws=draws)
    return prob, np.array(idx, np.int32)


def expected_steps(ref, H, step):
    """The flag sequence (bNoMore, bConverge, nInliers) of iterate(step) driven until one flag is up, from a restatement result."""
    if ref["status"] == api.SIM3_RANSAC_TOO_FEW:
        return [(1, 0, 0)]
    out, done = [], 0
    while True:
        end = min(H, done + step)
        if ref["status"] == api.SIM3_RANSAC_CONVERGED and ref["iterations"] <= end:
            return out + [(0, 1, ref["n_inliers"])]
        done = end
        if done >= H:
            return out + [(1, 0, 0)]
        out.append((0, 0, 0))
