"""Shared by the OptimizeSim3 tests: builds and calls the sequential CPU restatement (tests/host/sim3_opt_restatement.cpp, in double
and in long double), and constructs the cases the tests need -- each found by a seeded search on the restatement itself, computed once
and shared.  Not a test module."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from geoflowslam_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "sim3_opt_restatement.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_sim3_opt_restatement.so")
_L = None

END_NOT_RUN, END_ITERATIONS, END_QMAX, END_RHO_ZERO, END_NBAD = range(5)


class Trace(C.Structure):
    _fields_ = [("end_reason", C.c_int32 * 2), ("rejected_trials", C.c_int32 * 2), ("failed_solves", C.c_int32 * 2),
                ("last_trial_rejected", C.c_int32 * 2), ("stale_flag_differences", C.c_int32), ("pad", C.c_int32),
                ("final_lambda", C.c_double * 2), ("stale_largest_difference", C.c_double), ("stale_x_applied", C.c_int32 * 2),
                ("failed_after_success", C.c_int32 * 2)]


def restatement():
    global _L
    if _L is None:
        deps = [_SRC, os.path.join(ROOT, "include", "gfs_abi.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", _SO, _SRC], check=True)
        L = C.CDLL(_SO)
        vp = C.c_void_p
        for f in (L.s3r_optimize, L.s3r_optimize_ld):
            f.argtypes = [C.POINTER(api.Sim3OptProblem), C.POINTER(api.Sim3OptSolution), C.POINTER(Trace)]
            f.restype = C.c_int
        L.s3r_optimize_batch.argtypes = [vp, C.c_int, vp]
        L.s3r_linearize.argtypes = [C.POINTER(api.Sim3OptProblem), C.c_int, vp, vp, vp, vp, vp]
        L.s3r_constants.argtypes = [vp]
        _L = L
    return _L


def run(prob, long_double=False):
    """The restatement on one problem dict -> result dict as api.Sim3Optimizer.OptimizeSim3's, plus "trace" (dict) and "ret"."""
    L = restatement()
    P, S, keep, n = api.sim3_opt_structs(prob)
    T = Trace()
    ret = (L.s3r_optimize_ld if long_double else L.s3r_optimize)(C.byref(P), C.byref(S), C.byref(T))
    res = api.sim3_opt_result(S, keep, n)
    res["ret"] = ret
    res["trace"] = dict(end_reason=tuple(T.end_reason), rejected_trials=tuple(T.rejected_trials), failed_solves=tuple(T.failed_solves),
                        last_trial_rejected=tuple(T.last_trial_rejected), stale_flag_differences=int(T.stale_flag_differences),
                        final_lambda=tuple(T.final_lambda), stale_largest_difference=float(T.stale_largest_difference),
                        stale_x_applied=tuple(T.stale_x_applied), failed_after_success=tuple(T.failed_after_success))
    return res


def linearize(prob, robust):
    """One linearisation at the problem's estimate -> err [2n, 2], J [2n, 2, 7], H [7, 7], b [7], chi (edge order e12(0), e21(0), ...)."""
    P, _, keep, n = api.sim3_opt_structs(prob)
    err, J, H, b, chi = np.zeros((2 * n, 2)), np.zeros((2 * n, 2, 7)), np.zeros((7, 7)), np.zeros(7), np.zeros(1)
    restatement().s3r_linearize(C.byref(P), int(robust), *(a.ctypes.data for a in (err, J, H, b, chi)))
    return err, J, H, b, chi[0]


def constants():
    out = np.zeros(5)
    restatement().s3r_constants(out.ctypes.data)
    return dict(first_iterations=int(out[0]), more_iterations_after_removal=int(out[1]), more_iterations=int(out[2]),
                min_correspondences=int(out[3]), numeric_delta=float(out[4]))


RESULT_KEYS = ("s12", "n_in", "n_bad", "status", "iterations_run", "pair_state", "chi2")


def result_bytes(r):
    """Everything gfs_sim3_optimize returns, as bytes."""
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in RESULT_KEYS)


def same_flags(a, b):
    return (a["n_in"], a["n_bad"], a["status"], tuple(a["iterations_run"])) == (b["n_in"], b["n_bad"], b["status"], tuple(b["iterations_run"])) \
        and (a["pair_state"] == b["pair_state"]).all()


def s12_distance(a, b):
    """Largest absolute difference of the eight numbers of two Sim3s (unit quaternion, metres, scale near 1: one common unit)."""
    return float(np.max(np.abs(np.asarray(a["s12"]) - np.asarray(b["s12"]))))


SIZES = (0, 1, 9, 10, 11, 63, 64, 65, 255, 256, 257, 600)


def sized_problem(n, outliers, fix_scale=True, seed=None):
    return synth.sim3_opt_problem(1000 + n if seed is None else seed, n_pairs=n, fix_scale=fix_scale,
                                  outlier_share=0.15 if outliers else 0.0, outlier_px=40.0)


def _search(make, wanted, seeds):
    for seed in seeds:
        p = make(seed)
        r = run(p)
        if wanted(p, r):
            return p, r
    raise AssertionError("no seed gives the wanted case")


@functools.lru_cache(maxsize=None)
def constructed_cases():
    """name -> problem dict, every one found by a seeded search on the float64 restatement (fixed scale):
      no_removal / removal   nBad == 0 and nBad > 0, both phases run
      five_more / ten_more   a start so far off that the second phase uses every iteration it is given: 5 when nBad == 0, 10 when
                             nBad > 0 (th2 = 4e4, so that the far start does not empty the graph)
      nine_left / ten_left   9 and 10 pairs survive the first check: the early return and not
      final_only             a pair removed by the final check alone
      ends_qmax / ends_nbad  a phase that ends at qmax == 10 and one that ends by _nBad >= 3
      rejected_trial         a popped Levenberg trial
      stale                  the first check's flags differ from what recomputed errors would give
      tie_below / tie_above  one chi2 within a few ulps of th2 on either side, by bisecting an observation"""
    cases = {}
    clean = lambda seed, n=40, **kw: synth.sim3_opt_problem(seed, n_pairs=n, outlier_share=0.0, noise_px=0.3, **kw)
    dirty = lambda seed, n=60, **kw: synth.sim3_opt_problem(seed, n_pairs=n, outlier_share=0.2, **kw)
    cases["no_removal"] = _search(clean, lambda p, r: r["n_bad"] == 0 and r["status"] == 1, range(100, 140))[0]
    cases["removal"] = _search(dirty, lambda p, r: r["n_bad"] > 0 and r["status"] == 1, range(200, 240))[0]

    wide = lambda share: (lambda seed: synth.sim3_opt_problem(seed, n_pairs=40, outlier_share=share, noise_px=0.5, estimate_rot_deg=60.0,
                                                              estimate_trans=2.0, th2=4e4, outlier_px=2000.0))
    used_up = lambda removal, its: (lambda p, r: r["status"] == 1 and (r["n_bad"] > 0) == removal and r["iterations_run"][1] == its and
                                    r["trace"]["end_reason"][1] == END_ITERATIONS)
    cases["five_more"] = _search(wide(0.0), used_up(False, 5), range(50, 1000))[0]
    cases["ten_more"] = _search(wide(0.2), used_up(True, 10), range(50, 1000))[0]

    def left(k):  # k inliers and gross outliers on top: exactly k pairs survive
        def make(seed):
            p = synth.sim3_opt_problem(seed, n_pairs=k + 6, outlier_share=0.0, noise_px=0.2)
            p["obs1"][k:] += 80.0
            return p
        return _search(make, lambda p, r: len(p["x1c"]) - r["n_bad"] == k, range(300, 400))[0]

    cases["nine_left"], cases["ten_left"] = left(9), left(10)
    cases["final_only"] = _search(lambda s: synth.sim3_opt_problem(s, n_pairs=50, outlier_share=0.1, noise_px=1.2, outlier_px=4.0),
                                  lambda p, r: r["status"] == 1 and (r["pair_state"] == 2).any(), range(400, 600))[0]
    far = lambda s: synth.sim3_opt_problem(s, n_pairs=30, outlier_share=0.3, noise_px=1.0, estimate_rot_deg=6.0, estimate_trans=0.4)
    cases["ends_qmax"] = _search(far, lambda p, r: END_QMAX in r["trace"]["end_reason"], range(600, 1600))[0]
    cases["ends_nbad"] = _search(dirty, lambda p, r: END_NBAD in r["trace"]["end_reason"], range(1600, 1800))[0]
    cases["rejected_trial"] = _search(far, lambda p, r: sum(r["trace"]["rejected_trials"]) > 0 and r["status"] == 1, range(1800, 2400))[0]
    cases["stale"] = _stale_case(far)
    cases["tie_below"], cases["tie_above"], cases["tie_pair"] = _tie_cases(cases["no_removal"])
    cases.update(_degenerate_cases())
    return cases


PROBLEM_ARRAYS = ("x1c", "x2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")
DEGENERATE_CASES = ("failed_first_solve", "failed_after_success", "failed_across_phases", "nan_observation", "inf_observation", "nan_point",
                    "nan_survives_first_check", "nan_survives_first_check_600", "z_zero", "behind_camera", "huge_observation",
                    "fewer_than_ten_after_nan")
NAN_PAIR = {"nan_survives_first_check": 4, "nan_survives_first_check_600": 520}  # case -> the pair whose x2c is NaN


def changed(p, **changes):
    """A copy of problem p with entries set: changed(p, obs1=((3, 0), nan)) sets obs1[3, 0]; a callable value is applied to the array."""
    q = dict(p)
    for k, v in changes.items():
        q[k] = p[k].copy()
        if callable(v):
            v(q[k])
        else:
            q[k][v[0]] = v[1]
    return q


def _degenerate_cases():
    """The part of constructed_cases() named by DEGENERATE_CASES: inputs on which the 7 x 7 solve fails or an edge's chi2 is not finite, every one found by a seeded search
    on the float64 restatement (fixed scale; tests/test_sim3_opt_restatement.py asserts that each reaches what it is named for).  A
    negative information is a test device only: it makes a system that is not positive, as lba_inertial_support._failed does.
      failed_first_solve     all information zero: lambda = 0, no pivot, every solve fails and the solver's x stays 0
      failed_after_success   negative information on the first 40 % of the pairs: in the first optimize() a solve fails after one that
                             succeeded, and the x it kept is applied again
      failed_across_phases   the first optimize() has no failed solve, the second fails at its first solve and applies the x that the
                             first one left behind (the inliers carry a small negative information, the gross outliers hold the
                             system positive until the first check removes them)
      nan_observation / inf_observation / nan_point   one non-finite number in obs1, obs2 (an e21 edge: an odd lane), x1c (e21)
      nan_survives_first_check       x2c of pair 4 is NaN (edge 8: an even lane's first register edge): its chi2 is NaN at the first
                                     check, `NaN > th2` is false, the pair stays INLIER and every solve of the second phase fails
      nan_survives_first_check_600   the same at pair 520 of 600 (edge 1040: beyond the four register edges, through global memory)
      z_zero / behind_camera / huge_observation   a point with z = 0 in camera 1, with z = -3, an observation of 1e300 px
      fewer_than_ten_after_nan   nine pairs survive the first check, one of them with a NaN chi2: the early return"""
    nan, inf = float("nan"), float("inf")
    dirty = lambda seed, n=40, **kw: synth.sim3_opt_problem(seed, n_pairs=n, outlier_share=0.2, **kw)
    both = lambda r: r["status"] == 1
    cases = {}

    def negated(share, factor=-1.0, of=None):
        def make(seed):
            p = synth.sim3_opt_problem(seed, n_pairs=40, outlier_share=0.5 if of else 0.2)
            m = ~p["outlier"] if of else np.arange(40) < int(share * 40)

            def scale(a):
                a[m] *= np.float32(factor)
            return changed(p, inv_sigma2_1=scale, inv_sigma2_2=scale)
        return make

    def zero(a):
        a[:] = 0
    cases["failed_first_solve"] = _search(lambda s: changed(dirty(s), inv_sigma2_1=zero, inv_sigma2_2=zero),
                                          lambda p, r: both(r) and min(r["trace"]["failed_solves"]) > 0 and r["trace"]["stale_x_applied"] == (0, 0), range(31, 41))[0]
    cases["failed_after_success"] = _search(negated(0.4), lambda p, r: both(r) and r["trace"]["stale_x_applied"][0] > 0 and
                                            r["trace"]["failed_after_success"][0] == 1, range(31, 71))[0]
    # (failed_solves[1] > 0 without a failure after a success: the phase's first solve is among the failed ones)
    cases["failed_across_phases"] = _search(negated(None, -0.01, of="inliers"), lambda p, r: both(r) and r["trace"]["failed_solves"][0] == 0 and
                                            r["trace"]["failed_solves"][1] > 0 and r["trace"]["failed_after_success"][1] == 0 and
                                            r["trace"]["stale_x_applied"][1] > 0, range(31, 131))[0]
    finite_s12 = lambda p, r: both(r) and np.isfinite(r["s12"]).all()
    cases["nan_observation"] = _search(lambda s: changed(dirty(s), obs1=((3, 0), nan)), finite_s12, range(31, 41))[0]
    cases["inf_observation"] = _search(lambda s: changed(dirty(s), obs2=((5, 1), inf)), finite_s12, range(31, 41))[0]
    cases["nan_point"] = _search(lambda s: changed(dirty(s), x1c=((7, 1), nan)), finite_s12, range(31, 41))[0]
    for name, n in (("nan_survives_first_check", 40), ("nan_survives_first_check_600", 600)):
        k = NAN_PAIR[name]
        cases[name] = _search(lambda s: changed(dirty(s, n), x2c=(k, nan)),
                              lambda p, r: both(r) and r["pair_state"][k] == api.SIM3_PAIR_INLIER and np.isnan(r["chi2"][k, 0]) and
                              r["trace"]["failed_solves"][1] == r["iterations_run"][1] > 0, range(31, 71))[0]
    cases["z_zero"] = changed(dirty(31), x1c=((6, 2), 0.0))
    cases["behind_camera"] = _search(lambda s: changed(dirty(s), x1c=((6, 2), -3.0)), finite_s12, range(31, 41))[0]
    cases["huge_observation"] = _search(lambda s: changed(dirty(s), obs1=(2, 1e300)), finite_s12, range(31, 41))[0]

    def nine(seed):  # nine pairs with small errors, one of them not a number, and six gross outliers
        p = synth.sim3_opt_problem(seed, n_pairs=15, outlier_share=0.0, noise_px=0.2)
        p["obs1"][9:] += 80.0
        return changed(p, obs1=((2, 1), nan))
    cases["fewer_than_ten_after_nan"] = _search(nine, lambda p, r: r["status"] == 0 and 15 - r["n_bad"] == 9 and r["pair_state"][2] == 0, range(300, 400))[0]
    return cases


def same_where_finite(a, b):
    """tests/test_gpu_pose_step.py's rule for results that hold a NaN: equal integers, equal NaN masks and equal bits where a number
    is one (a NaN's payload is nobody's contract) -> the first key that differs, or None"""
    for k in RESULT_KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.dtype.kind != "f":
            if x.tobytes() != y.tobytes():
                return k
            continue
        nx, ny = np.isnan(x), np.isnan(y)
        if (nx != ny).any() or x[~nx].tobytes() != y[~ny].tobytes():
            return k
    return None


def _tie_cases(base, pair=0):
    """(below, above, pair): `pair`'s e12 chi2 is within a few ulps of th2, below in one problem and above in the other.  A chi2 that
    went through the solve cannot be placed that finely (the numeric Jacobians make the estimate a rough function of an observation
    at the 1e-8 level), so the pair is taken out of the solve's reach: information 1e-30 and an observation 3e15 px away, where both
    perturbed projections round to the same error (a zero Jacobian row: the pair adds exact zeros to H and b) and one ulp of the
    observation moves the chi2 by less than two of its ulps.  Both checks then read the same chi2, at any estimate."""
    p = dict(base)
    p["inv_sigma2_1"] = base["inv_sigma2_1"].copy()
    p["inv_sigma2_1"][pair] = np.float32(1e-30)
    reach = float(np.sqrt(np.float64(np.float32(base["th2"])) / np.float64(p["inv_sigma2_1"][pair])))
    p["obs1"] = base["obs1"].copy()
    p["obs1"][pair, 0] += 0.99 * reach
    below, above = _bisect_observation(p, pair, lambda r: r["pair_state"][pair] != 0, reach=0.02 * reach)
    return below, above, pair


def _bisect_observation(base, pair, flagged, reach=30.0, axis=0):
    """Pair `pair`'s first observation moved along u (axis 0) or v (1), bisected down to two neighbouring doubles: flagged(result) is false at the
    first and true at the second -> the two problems (a chi2 just below and just above th2, whichever check reads it)."""
    def with_u(u):
        p = dict(base)
        p["obs1"] = base["obs1"].copy()
        p["obs1"][pair, axis] = u
        return p

    lo = float(base["obs1"][pair, axis])
    hi = lo + reach  # the pair's chi2 grows with the shift
    if flagged(run(with_u(lo))) or not flagged(run(with_u(hi))):
        return None
    while np.nextafter(lo, hi) < hi:
        mid = 0.5 * (lo + hi)
        if flagged(run(with_u(mid))):
            hi = mid
        else:
            lo = mid
    return with_u(lo), with_u(hi)


def _stale_case(make):
    """A problem whose first optimize() ends on a rejected trial (the edges then hold the errors of that trial, not of the restored
    estimate), with one observation bisected until a chi2 the first check reads is on one side of th2 and the recomputed one on the
    other."""
    for seed in range(600, 3000):
        base = make(seed)
        t = run(base)["trace"]
        if not (t["last_trial_rejected"][0] and t["stale_largest_difference"] > 0):
            continue
        for pair in range(4):
            found = _bisect_observation(base, pair, lambda r: r["pair_state"][pair] == 1)
            for p in found or ():
                if run(p)["trace"]["stale_flag_differences"] > 0:
                    return p
    raise AssertionError("no seed gives a stale first check")


@functools.lru_cache(maxsize=None)
def free_scale_cases():
    """Free-scale problems on which the float64 and the long double restatement agree on every flag and both iteration counts (so that
    no flip is expected from rounding) -> list of (name, problem, float64 result, float64 - long double distance of s12)."""
    out = []
    for n, outliers in ((11, False), (65, True), (150, True), (257, False), (600, True)):
        for seed in range(7000 + n, 7040 + n):
            p = sized_problem(n, outliers, fix_scale=False, seed=seed)
            r, rl = run(p), run(p, long_double=True)
            if same_flags(r, rl) and r["status"] == 1:
                out.append((f"free_{n}_{'out' if outliers else 'clean'}", p, r, s12_distance(r, rl)))
                break
        else:
            raise AssertionError(f"no free-scale seed with agreeing flags at n = {n}")
    return out


# ---- gfs_host::OptimizeSim3 on mock key frames (tests/host/sim3_opt_adaptor_test.cpp)

_ADAPTOR_SRC = os.path.join(ROOT, "tests", "host", "sim3_opt_adaptor_test.cpp")
_ADAPTOR_SO = os.path.join(ROOT, "tests", "host", "_sim3_opt_adaptor_test.so")
KIND_NO_MATCH, KIND_PAIR, KIND_NO_MP1, KIND_BAD_MP1, KIND_BAD_MP2 = range(5)


def adaptor_harness():
    deps = [_ADAPTOR_SRC, _SRC, os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp"), os.path.join(ROOT, "include", "gfs_abi.h")]
    if not os.path.exists(_ADAPTOR_SO) or os.path.getmtime(_ADAPTOR_SO) < max(os.path.getmtime(p) for p in deps):
        tmp = _ADAPTOR_SO + f".{os.getpid()}.tmp"
        libdir = os.path.dirname(api._LIB_PATH)
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", tmp, _ADAPTOR_SRC, "-L" + libdir,
                        "-lgfs_hip", "-Wl,-rpath," + libdir], check=True)
        os.replace(tmp, _ADAPTOR_SO)
    return C.CDLL(_ADAPTOR_SO)


def adaptor_scene(seed, n_good=20, n_gross=3, fix_scale=True):
    """Two mock key frames that see common points, with one key-point of every kind the gather treats differently in front:
    0 no match, 1 pMP1 bad, 2 pMP2 bad, 3 no pMP1, 4 pMP2 not in key frame 2 (i2 < 0; its mnTrackScaleLevel is 3), 5 behind camera 2,
    then n_good pairs, then n_gross pairs whose observation in key frame 1 is 60 px off."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    N = 6 + n_good + n_gross
    kind = np.full(N, KIND_PAIR, np.int32)
    kind[:4] = [KIND_NO_MATCH, KIND_BAD_MP1, KIND_BAD_MP2, KIND_NO_MP1]
    fx, fy, cx, cy = (f32(v) for v in synth.intrinsics(640, 480))
    R2 = synth._rot(*(np.deg2rad(2.0) * rng.uniform(-1, 1, 3))).astype(f32)
    t2 = (0.05 * rng.uniform(-1, 1, 3)).astype(f32)
    pose = np.zeros((2, 12), f32)
    pose[0, :9], pose[1, :9], pose[1, 9:] = np.eye(3, dtype=f32).ravel(), R2.ravel(), t2
    z = rng.uniform(1.5, 5.0, N)
    pw = np.stack([rng.uniform(-0.4, 0.4, N) * z, rng.uniform(-0.3, 0.3, N) * z, z], 1).astype(f32)
    pw[5] = [0.1, 0.1, -2.0]  # behind both cameras: P3D2c(2) < 0
    pos1, pos2 = pw.copy(), (pw + 0.001 * rng.normal(size=(N, 3))).astype(f32)
    p2 = (pw.astype(np.float64) @ R2.astype(np.float64).T + t2)
    proj = lambda p: np.stack([fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy], 1)
    kp1 = np.concatenate([proj(pw.astype(np.float64)) + 0.5 * rng.normal(size=(N, 2)), rng.integers(0, 8, (N, 1))], 1).astype(f32)
    M = N + 5
    order = rng.permutation(M)[:N]  # pMP2's index in key frame 2
    i2 = order.astype(np.int32)
    i2[4] = -1
    kp2 = np.zeros((M, 3), f32)
    kp2[:, 2] = rng.integers(0, 8, M)
    kp2[order, :2] = (proj(p2) + 0.5 * rng.normal(size=(N, 2))).astype(f32)
    kp1[6 + n_good:, 0] += 60.0
    sigma = np.stack([(f32(1.2) ** np.arange(8, dtype=f32)) ** -2, (f32(1.25) ** np.arange(8, dtype=f32)) ** -2]).astype(f32)
    track_level = np.full(N, 3, np.int32)
    Rt = R2.astype(np.float64).T
    s_true = 1.0
    Re = synth._rot(*(np.deg2rad(0.4) * rng.uniform(-1, 1, 3))) @ Rt
    s12 = np.concatenate([synth._quat_xyzw(Re), -Rt @ t2 + 0.01 * rng.uniform(-1, 1, 3), [s_true if fix_scale else 1.01]])
    return dict(N=N, M=M, kind=kind, pos1=pos1, pos2=pos2, i2=i2, track_level=track_level, kp1=kp1, kp2=kp2, pose=pose,
                cam=np.array([[fx, fy, cx, cy], [fx, fy, cx, cy]], f32), sigma=sigma, th2=f32(10.0), fix_scale=bool(fix_scale), s12=s12)


def run_adaptor(scene, all_points, use_device=False, camera_kind=0):
    L = adaptor_harness()
    N = scene["N"]
    o = dict(flat_n=np.zeros(3, np.int32), x1c=np.zeros((N, 3)), x2c=np.zeros((N, 3)), obs1=np.zeros((N, 2)), obs2=np.zeros((N, 2)),
             w1=np.zeros(N, np.float32), w2=np.zeros(N, np.float32), s12_seen=np.zeros(8), matched=np.zeros(N, np.uint8),
             s12=np.array(scene["s12"], np.float64), hessian=np.full(49, 7.0), counters=np.zeros(7, np.int32), status_n=np.zeros(4, np.int32))
    ins = [np.ascontiguousarray(scene[k]) for k in ("kind", "pos1", "pos2", "i2", "track_level", "kp1", "kp2", "pose", "cam", "sigma")]
    L.sim3_opt_adaptor_test.argtypes = [C.c_int] * 3 + [C.c_void_p] * len(ins) + [C.c_int, C.c_float, C.c_int, C.c_int] + [C.c_void_p] * len(o)
    o["ret"] = L.sim3_opt_adaptor_test(int(use_device), N, scene["M"], *[a.ctypes.data for a in ins], int(camera_kind), float(scene["th2"]),
                                       int(scene["fix_scale"]), int(all_points), *[v.ctypes.data for v in o.values()])
    return o


def expected_gather(scene, all_points):
    """The gather of :2853-2984 stated independently, in float32 where the reference computes in float -> (problem dict, vnIndexEdge,
    in key frame 2?, counters nCorrespondences / nBadMPs / nInKF2 / nOutKF2 / nMatchWithoutMP)."""
    f32 = np.float32
    R = [scene["pose"][k, :9].reshape(3, 3) for k in range(2)]
    t = [scene["pose"][k, 9:] for k in range(2)]
    cam_pt = lambda k, p: np.array([f32(f32(f32(R[k][r, 0] * p[0]) + f32(R[k][r, 1] * p[1])) + f32(R[k][r, 2] * p[2])) + t[k][r] for r in range(3)], f32)
    rows, idx, in2, cnt = [], [], [], dict(nCorrespondences=0, nBadMPs=0, nInKF2=0, nOutKF2=0, nMatchWithoutMP=0)
    for i in range(scene["N"]):
        kind, i2 = scene["kind"][i], int(scene["i2"][i])
        if kind == KIND_NO_MATCH:
            continue
        if kind in (KIND_BAD_MP1, KIND_BAD_MP2):
            cnt["nBadMPs"] += 1
            continue
        if kind == KIND_NO_MP1:
            cnt["nMatchWithoutMP"] += 1
            continue
        c1, c2 = cam_pt(0, scene["pos1"][i]), cam_pt(1, scene["pos2"][i])
        if (i2 < 0 and not all_points) or c2[2] < 0:
            continue
        cnt["nCorrespondences"] += 1
        k1 = scene["kp1"][i]
        if i2 >= 0:
            k2 = scene["kp2"][i2]
            o2, w2 = k2[:2], scene["sigma"][1][int(k2[2])]
            cnt["nInKF2"] += 1
        else:
            invz = f32(1) / c2[2]
            o2, w2 = np.array([c2[0] * invz, c2[1] * invz], f32), scene["sigma"][1][0]  # the level went into the key-point's size: octave 0
            cnt["nOutKF2"] += 1
        rows.append((c1.astype(np.float64), c2.astype(np.float64), k1[:2].astype(np.float64), o2.astype(np.float64), scene["sigma"][0][int(k1[2])], w2))
        idx.append(i)
        in2.append(i2 >= 0)
    col = lambda j, shape, dt=np.float64: np.array([r[j] for r in rows], dt).reshape(shape)
    prob = dict(s12=np.array(scene["s12"], np.float64), cam1=scene["cam"][0].astype(np.float64), cam2=scene["cam"][1].astype(np.float64),
                th2=float(scene["th2"]), fix_scale=scene["fix_scale"], x1c=col(0, (-1, 3)), x2c=col(1, (-1, 3)), obs1=col(2, (-1, 2)),
                obs2=col(3, (-1, 2)), inv_sigma2_1=col(4, (-1,), np.float32), inv_sigma2_2=col(5, (-1,), np.float32))
    return prob, np.array(idx, np.int64), np.array(in2, bool), cnt
