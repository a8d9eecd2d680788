"""The CPU restatement of LocalMapping::CreateNewMapPoints (tests/host/triangulate_restatement.cpp, on the rule header) against an
independent numpy statement of DESIGN.md section 14, bit for bit, on random problems and on constructed cases that sit on each
decision; the two written rules (the 4 x 4 null vector, the stereo parallax cosine) against numpy's SVD and the host's libm.
No GPU."""
import copy
import ctypes as C

import numpy as np
import pytest

import triangulate_support as TS

SEEDS = range(32)
f32, f64 = np.float32, np.float64


def test_random_problems_take_every_path():
    """On the restatement's own output: every exit occurs (the SVD's w == 0 and a zero distance need the constructed problems: no
    rigid pose pair reaches them), both branches of the chi2 gates accept and reject, Hamming ties occur, and an idx1 whose match
    failed a gate is matched again at a later neighbour."""
    exits, stats = np.zeros(12, np.int64), dict.fromkeys(TS.STATS, 0)
    for seed in SEEDS:
        out, st = TS.restate(TS.random_problem(seed), with_stats=True)
        for o in out:
            exits += np.bincount(o["exit"], minlength=12)
        for k in TS.STATS:
            stats[k] += st[k]
    random_exits = exits.copy()
    for prob, _ in TS.constructed().values():
        for o in TS.restate(prob):
            exits += np.bincount(o["exit"], minlength=12)
    assert (exits > 0).all(), dict(zip(TS.EXITS, exits))
    assert set(np.nonzero(random_exits == 0)[0]) <= {TS.SVD_W_ZERO, TS.ZERO_DIST}, dict(zip(TS.EXITS, random_exits))
    assert all(stats[k] > 0 for k in TS.STATS), stats


@pytest.mark.parametrize("seed", SEEDS)
def test_restatement_equals_numpy_statement(seed):
    prob = TS.random_problem(seed)
    TS.assert_equal(TS.restate(prob), TS.numpy_statement(prob), seed)


def test_shared_problems_equal_numpy_statement():
    for args, kw in (((63, 65), {}), ((64, 0), {}), ((0, 64), {}), ((65, 65), dict(n_nodes=1)), ((257, 1000), {})):
        prob, want = TS.problem(*args, **kw)
        TS.assert_equal(want, TS.numpy_statement(prob), (args, kw))


@pytest.mark.parametrize("label", sorted(TS.constructed()))
def test_constructed_case(label):
    prob, check = TS.constructed()[label]
    out, ns = TS.restate(prob), TS.numpy_statement(prob)
    assert check(out), (label, [(o["match12"].tolist(), o["exit"].tolist()) for o in out])
    assert check(ns), label
    TS.assert_equal(out, ns, label)


def _pair(stereo1, stereo2, oct1=2, oct2=2, world=(0.4, -0.2, 3.0), dx=0.3, noise=0.35):
    """One current key-point and one neighbour key-point of one world point, a little off its projections: -> problem (coarse)."""
    W = np.array([world])
    T1, T2 = TS._shift(0, 0, 0), TS._shift(dx, 0.02, 0)
    kfs = []
    for T, st, oc, n in ((T1, stereo1, oct1, noise), (T2, stereo2, oct2, -noise)):
        xy, z, ur = TS._geometry(W, T)
        xy = xy + n
        kfs.append(TS._kf(1, [(5, [0])], TS._desc(3), xy, ur + n if st else [-1.0], z if st else [-1.0], octave=oc, T_wc=T))
    return TS._prob(kfs[0], [kfs[1]])


def _exit(prob):
    out, ns = TS.restate(prob), TS.numpy_statement(prob)
    TS.assert_equal(out, ns)
    return int(out[0]["exit"][0])


@pytest.mark.parametrize("view,stereo,chi", [(0, False, 5.991), (0, True, 7.8), (1, False, 5.991), (1, True, 7.8)])
def test_one_float_either_side_of_the_chi2_bounds(view, stereo, chi):
    """level_sigma2 one float below the value at which chi * sigma2 reaches the squared error rejects, the next float accepts."""
    prob = _pair(stereo and view == 0, stereo and view == 1)
    info = {}
    ex, _, _ = TS.match_statement(prob, prob["neighbours"][0], 0, 0, info)
    assert ex == TS.CREATED
    e2, c, s2 = info["chi1" if view == 0 else "chi2"]
    assert c == chi and e2 > 0
    lo, hi = TS.straddle(lambda s: not f64(e2) > f64(chi) * f64(s), 1e-12, 1e6)
    assert f64(chi) * f64(lo) < f64(e2) <= f64(chi) * f64(hi) and np.nextafter(lo, f32(np.inf)) == hi
    for s, want in ((lo, TS.REPROJ_1 + view), (hi, TS.CREATED)):
        q = copy.deepcopy(prob)
        kf = q["cur"] if view == 0 else q["neighbours"][0]
        kf["level_sigma2"] = kf["level_sigma2"].copy()
        kf["level_sigma2"][2] = s
        assert _exit(q) == want, (view, stereo, s)


@pytest.mark.parametrize("oct1,oct2", [(5, 1), (1, 5)])
def test_one_float_either_side_of_the_scale_ratio_bound(oct1, oct2):
    """ratioDist * ratioFactor < ratioOctave (octave ratio above the distance ratio) and ratioDist > ratioOctave * ratioFactor
    (below it): the ratio factor one float short of the bound rejects, the next float accepts."""
    prob = _pair(True, True, oct1, oct2)
    big = dict(prob, ratio_factor=f32(100))
    info = {}
    assert TS.match_statement(big, big["neighbours"][0], 0, 0, info)[0] == TS.CREATED
    rd, ro, _ = info["ratio"]
    ok = (lambda rf: not f32(rd * rf) < ro) if ro > rd else (lambda rf: not rd > f32(ro * rf))
    lo, hi = TS.straddle(ok, 1.0, 100.0)
    assert np.nextafter(lo, f32(np.inf)) == hi and hi > f32(1.01)
    assert _exit(dict(prob, ratio_factor=lo)) == TS.SCALE and _exit(dict(prob, ratio_factor=hi)) == TS.CREATED


@pytest.mark.parametrize("inertial,bound", [(False, 0.9998), (True, 0.9996)])
def test_either_side_of_the_parallax_bound(inertial, bound):
    """Two mono key-points: moving the neighbour's key-point by single floats takes cosParallaxRays across the bound; the float at
    or above it is low parallax, the float below it is triangulated."""
    prob = dict(_pair(False, False, world=(0.1, 0.05, 9.0), dx=0.12, noise=0.0), inertial=inertial)

    def cos_at(x):
        q = copy.deepcopy(prob)
        q["neighbours"][0]["kps_un"]["x"][0] = x
        info = {}
        ex = TS.match_statement(q, q["neighbours"][0], 0, 0, info)[0]
        return q, ex, info["cos_rays"]

    x0 = f32(prob["neighbours"][0]["kps_un"]["x"][0])
    assert cos_at(x0)[1] == TS.LOW_PARALLAX and cos_at(x0 - f32(30))[1] != TS.LOW_PARALLAX
    lo, hi = TS.straddle(lambda d: cos_at(f32(x0 - d))[1] != TS.LOW_PARALLAX, 0.0, 30.0)
    (qa, ea, ca), (qb, eb, cb) = cos_at(f32(x0 - lo)), cos_at(f32(x0 - hi))
    assert f64(ca) >= bound > f64(cb), (ca, cb)
    assert abs(int(ca.view(np.int32)) - int(cb.view(np.int32))) <= 2  # neighbouring floats around the bound
    assert _exit(qa) == TS.LOW_PARALLAX and _exit(qb) != TS.LOW_PARALLAX


def _own_matrices():
    """The 4 x 4 systems of the random problems' own triangulated matches."""
    mats = []
    for seed in SEEDS:
        prob = TS.random_problem(seed)
        for nb, o in zip(prob["neighbours"], TS.restate(prob)):
            for i in np.nonzero(o["match12"] >= 0)[0]:
                info = {}
                TS.match_statement(prob, nb, int(i), int(o["match12"][i]), info)
                if "A" in info:
                    mats.append((info["A"], info["sweeps"]))
    return np.array([m for m, _ in mats], f32), max(s for _, s in mats)


def test_null_vector_rule_against_lapack():
    """Written rule 2 on the problems' own matrices: x3D against numpy.linalg.svd in float64; the yardstick is numpy's float32 SVD
    of the same matrices.  The rule's maximum relative error is at most twice the yardstick's.  (Measured: DESIGN.md section 14.)"""
    A, sweeps = _own_matrices()
    assert len(A) > 1500 and sweeps <= 30
    h = TS.rule_null_vector(A)
    assert all(TS.same_bits(np.array(TS.jacobi_null_vector(A[k])[0], f32), h[k]) for k in range(0, len(A), 7))
    v64 = np.linalg.svd(A.astype(f64))[2][:, 3, :]
    v32 = np.linalg.svd(A)[2][:, 3, :]
    assert v32.dtype == f32
    with np.errstate(all="ignore"):
        ref = v64[:, :3] / v64[:, 3:]
        rule = (h[:, :3] / h[:, 3:]).astype(f64)
        yard = (v32[:, :3] / v32[:, 3:]).astype(f64)
    nrm = np.linalg.norm(ref, axis=1)
    keep = np.isfinite(nrm) & (nrm > 0)
    e_rule = np.linalg.norm(rule - ref, axis=1)[keep] / nrm[keep]
    e_yard = np.linalg.norm(yard - ref, axis=1)[keep] / nrm[keep]
    print(f"null vector rule: {keep.sum()} matrices, at most {sweeps} sweeps; relative x3D error median {np.median(e_rule):.3g} max {e_rule.max():.3g}; "
          f"numpy float32 SVD median {np.median(e_yard):.3g} max {e_yard.max():.3g}")
    assert e_rule.max() <= 2 * e_yard.max(), (e_rule.max(), e_yard.max())


def test_cos_stereo_rule_against_libm():
    """Written rule 1 against cosf(2.f * atan2f(mb / 2, depth)) of the host's libm on a fixed sweep of 200 000 depths: under 1 %
    differ, each by one ulp.  (Measured: DESIGN.md section 14.)"""
    libm = C.CDLL("libm.so.6")
    for fn, n in (("cosf", 1), ("atan2f", 2)):
        getattr(libm, fn).restype = C.c_float
        getattr(libm, fn).argtypes = [C.c_float] * n
    mb = f32(0.0745)
    depth = np.random.default_rng(20261018).uniform(0.3, 10.0, 200000).astype(f32)
    h = float(f32(mb / f32(2)))
    want = np.array([libm.cosf(float(f32(f32(2) * f32(libm.atan2f(h, float(d)))))) for d in depth], f32)
    got = TS.rule_cos_stereo(mb, depth)
    assert TS.same_bits(got[::97], np.array([TS.cos_stereo(mb, d) for d in depth[::97]], f32))
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    share = float((ulps > 0).mean())
    print(f"cos rule: {int((ulps > 0).sum())} of {len(depth)} differ from libm ({100 * share:.3f} %), max {ulps.max()} ulp")
    assert share < 0.01 and ulps.max() <= 1
