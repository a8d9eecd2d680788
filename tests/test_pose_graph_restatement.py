"""CPU tests of the essential graph's arithmetic: geoflowslam_amd/csrc/sim3_dev.hpp compiled with g++
(tests/host/pose_graph_restatement.cpp) against the numpy restatement (tests/pose_graph_support.py) bit for bit in float64, on
inputs that take every branch; log(exp(u)) = u; the numeric Jacobians against a long-double reference within the noise their own
rule predicts; the literals of the reference against what the header, the binding and the adaptor compile in.  No GPU."""
import os
import re

import numpy as np
import pytest

import pose_graph_support as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
N = 2000


def _updates(seed, n=N):
    """[n, 7] tangent vectors: a quarter each with (small, small), (small sigma, angle), (sigma, small angle), (sigma, angle); among
    the angles some that exp takes as large and log as small (1e-5 < theta < 4e-3)"""
    rng = np.random.default_rng(seed)
    u = np.zeros((n, 7))
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    k = np.arange(n) % 4
    theta = np.where(k % 2 == 0, rng.uniform(0, 0.9e-5, n), np.where(rng.random(n) < 0.25, rng.uniform(2e-5, 4e-3, n), rng.uniform(0.01, 2.8, n)))
    sigma = np.where(k < 2, rng.uniform(-0.9e-5, 0.9e-5, n), rng.uniform(0.002, 0.4, n) * rng.choice([-1, 1], n))
    sigma[:8] = 0.0
    u[:, 0:3] = axis * theta[:, None]
    u[:, 3:6] = rng.uniform(-10, 10, (n, 3))
    u[:, 6] = sigma
    return u


def _sim3s(seed, n=N):
    return pg.sim3_exp(_updates(seed, n))[0]


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_exp_and_log_bitwise_on_every_branch():
    u = _updates(1)
    S, br = pg.sim3_exp(u)
    Sc, brc = pg.host_call("pgr_exp", N, u, outs=[((N, 8), np.float64), (N, np.int32)])
    hits = np.bincount(br, minlength=4)
    print("exp branch hits", hits)
    assert (hits > 0).all() and (br == brc).all()
    assert _same(S, Sc)
    L, bl = pg.sim3_log(S)
    Lc, blc = pg.host_call("pgr_log", N, S, outs=[((N, 7), np.float64), (N, np.int32)])
    hits = np.bincount(bl, minlength=4)
    print("log branch hits", hits)
    assert (hits > 0).all() and (bl == blc).all()
    assert _same(L, Lc)
    # a large angle for exp that is a small one for log: the two eps tests are not the same test
    assert ((br & pg.BRANCH_ANGLE != 0) & (bl & pg.BRANCH_ANGLE == 0)).any()


def test_products_bitwise():
    a, b, c = _sim3s(2), _sim3s(3), _sim3s(4)
    assert _same(pg.sim3_mul(a, b), pg.host_call("pgr_mul", N, a, b, outs=[((N, 8), np.float64)])[0])
    assert _same(pg.sim3_inverse(a), pg.host_call("pgr_inverse", N, a, outs=[((N, 8), np.float64)])[0])
    xyz = np.random.default_rng(5).uniform(-20, 20, (N, 3))
    assert _same(pg.sim3_map(a, xyz), pg.host_call("pgr_map", N, a, xyz, outs=[((N, 3), np.float64)])[0])
    # residuals of every log branch: c = (small step) * b * a^-1 ... so that C v0 v1^-1 is the small step
    step = _sim3s(6)
    meas = pg.sim3_mul(step, pg.sim3_mul(b, pg.sim3_inverse(a)))
    r, br = pg.edge_residual(meas, a, b)
    rc, brc = pg.host_call("pgr_residual", N, meas, a, b, outs=[((N, 7), np.float64), (N, np.int32)])
    hits = np.bincount(br, minlength=4)
    print("residual branch hits", hits)
    assert (hits > 0).all() and (br == brc).all()
    assert _same(r, rc)
    r2 = pg.edge_residual(c, a, b)[0]
    assert _same(r2, pg.host_call("pgr_residual", N, c, a, b, outs=[((N, 7), np.float64), (N, np.int32)])[0])
    upd = _updates(7) * 1e-3
    for fix in (0, 1):
        assert _same(pg.sim3_oplus(a, upd, bool(fix)), pg.host_call("pgr_oplus", N, a, upd, outs=[((N, 8), np.float64)], flag=fix)[0])


def test_log_inverts_exp_away_from_the_seams():
    rng = np.random.default_rng(8)
    n = 1000
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    big = np.arange(n) % 2 == 0
    theta = np.where(big, rng.uniform(0.1, 2.5, n), rng.uniform(0, 1e-7, n))
    sigma = np.where(np.arange(n) % 4 < 2, rng.uniform(0.01, 0.5, n) * rng.choice([-1, 1], n), rng.uniform(-1e-6, 1e-6, n))
    u = np.concatenate([axis * theta[:, None], rng.uniform(-1, 1, (n, 3)), sigma[:, None]], 1)
    back = pg.sim3_log(pg.sim3_exp(u)[0])[0]
    err = np.abs(back - u).max()
    print("max |log(exp(u)) - u|", err)
    assert err <= 1e-12


def test_numeric_jacobians_bitwise_and_within_their_own_noise():
    n = 200
    a, b = _sim3s(9, n), _sim3s(10, n)
    step = pg.sim3_exp(_updates(11, n) * np.array([1, 1, 1, 0.01, 0.01, 0.01, 1]))[0]
    meas = pg.sim3_mul(step, pg.sim3_mul(b, pg.sim3_inverse(a)))
    for fix in (True, False):
        Ji, Jj = pg.numeric_jacobians(meas, a, b, fix)
        dim = 6 if fix else 7
        Jic, Jjc = pg.host_call("pgr_jacobians", n, meas, a, b, outs=[((n, 7, 7), np.float64), ((n, 7, 7), np.float64)], flag=int(fix))
        assert _same(Ji, np.ascontiguousarray(Jic[:, :, :dim])) and _same(Jj, np.ascontiguousarray(Jjc[:, :, :dim]))
        assert (Jic[:, :, dim:] == 0).all() and (Jjc[:, :, dim:] == 0).all()
        # the reference: the same central difference with delta = 1e-5 in long double (truncation ~ delta^2, rounding ~ 1e-19 / delta)
        ld = np.longdouble
        Ri, Rj = pg.numeric_jacobians(meas.astype(ld), a.astype(ld), b.astype(ld), fix, delta=1e-5)
        # ... whose own truncation error is not small everywhere: on the small-angle branch with |sigma| >= eps sim3.h:199 has
        # B = ((sigma^2 / 2 - sigma + 1) s) / sigma^3, of the order of sigma^-3, so W carries a term B Omega^2 with a curvature of 1e6
        # at sigma = 0.01.  The same difference at delta / 2 measures it (Richardson: error(delta) = 4/3 of the change); twice the
        # change is allowed on top.
        Hi, Hj = pg.numeric_jacobians(meas.astype(ld), a.astype(ld), b.astype(ld), fix, delta=0.5e-5)
        # What delta = 1e-9 predicts in float64: a column is (e+ - e-) / (2 delta), and a residual is a chain of about a hundred
        # operations on numbers as large as the translations |t|, so each e carries up to ~32 eps |t|: 2 x 32 eps |t| / (2 delta).
        # On top of that the coefficients of W cancel as the source writes them, and the translation rows inherit it through
        # upsilon = W^-1 t: C = (s - 1) / sigma loses a factor 1 / |sigma|; A = ((sigma - 1) s + 1) / sigma^2 (small angle) has an
        # absolute error of 2 eps / sigma^2 and multiplies Omega ~ theta; A = (a sigma + (1 - b) theta) / (theta c) has eps / c, times
        # theta; A = (1 - cos theta) / theta^2 has eps / theta^2, times theta.  In units of eps |t|:
        scale = np.maximum(1.0, np.abs(np.concatenate([meas[:, 4:7], a[:, 4:7], b[:, 4:7]], 1)).max(1))
        r0, br0 = pg.edge_residual(meas, a, b)
        th, sg = np.linalg.norm(r0[:, 0:3], axis=1), np.abs(r0[:, 6])
        small, has_sigma = (br0 & pg.BRANCH_ANGLE) == 0, (br0 & pg.BRANCH_SIGMA) != 0
        with np.errstate(all="ignore"):
            amp = 32 + np.where(has_sigma, 1 / sg + np.where(small, 2 * th / sg**2, th / (th**2 + sg**2)), 0) + np.where(small, 0, 1 / th)
        bound = 2 * np.finfo(np.float64).eps * scale * amp / (2 * pg.DELTA)
        # The reference's own step of 1e-5 must not carry a residual across a seam: the angle seam of the log lies at
        # acos(1 - eps) = 4.47e-3, and with a free scale the step moves sigma itself, so |sigma| has to stay on its side of eps
        # (the |sigma| < eps branches are compared with the scale fixed, where sigma does not move).
        valid = (np.abs(th - np.arccos(1 - pg.EPS)) > 1e-4) & (fix | (sg > 1e-3))
        assert valid.sum() >= 50 and set(br0[valid]) == ({0, 1, 2, 3} if fix else {1, 3})
        worst = 0.0
        for J, R, H in ((Ji, Ri, Hi), (Jj, Rj, Hj)):
            own = 2 * np.abs(R - H).astype(np.float64)
            rel = (np.maximum(np.abs(J - R.astype(np.float64)) - own, 0)).max(axis=(1, 2)) / bound
            worst = max(worst, float(rel[valid].max()))
        print(f"fix_scale={fix}: max |J - J_ref| = {worst:.3f} of the predicted noise ({float(bound.max()):.2e} at most)")
        assert worst <= 1.0


def _ref(path):
    return open(os.path.join(REF, path), errors="replace").read()


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="the reference tree is not present")
def test_reference_literals(api):
    k = np.zeros(2)
    pg.host().pgr_constants(k.ctypes.data)
    sim3 = _ref("Thirdparty/g2o/g2o/types/sim3.h")
    eps = re.findall(r"double eps = ([0-9.e-]+);", sim3)
    assert len(eps) == 2 and all(float(v) == k[0] == pg.EPS for v in eps)
    edge = _ref("Thirdparty/g2o/g2o/core/base_binary_edge.hpp")
    delta = re.findall(r"const double delta = ([0-9.e-]+);", edge)
    assert len(delta) == 1 and float(delta[0]) == k[1] == pg.DELTA
    body = "\n".join(_ref("src/Optimizer.cc").splitlines()[2041:2413])
    assert body.lstrip().startswith("void Optimizer::OptimizeEssentialGraph(")
    lam = float(re.search(r"setUserLambdaInit\(([0-9.e-]+)\)", body).group(1))
    min_feat = int(re.search(r"const int minFeat = (\d+);", body).group(1))
    iters = int(re.search(r"optimizer\.optimize\((\d+)", body).group(1))
    icp = float(re.search(r"eicp->information\(\) = matLambda \* (\d+);", body).group(1))
    gates = re.search(r"result\.converged && result\.num_inliers > (\d+) &&\s*\(result\.error / result\.num_inliers\) < ([0-9.]+)", body)
    assert (lam, min_feat, iters, icp) == (1e-16, 100, 20, 3.0)
    assert (api.ESSENTIAL_GRAPH_LAMBDA_INIT, api.ESSENTIAL_GRAPH_MIN_FEAT, api.ESSENTIAL_GRAPH_ITERATIONS, api.ESSENTIAL_GRAPH_ICP_WEIGHT) == \
        (lam, min_feat, iters, icp)
    ad = open(os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp")).read()
    assert float(re.search(r"kEssentialGraphLambdaInit = ([0-9.e-]+);", ad).group(1)) == lam
    assert int(re.search(r"kEssentialGraphMinFeat = (\d+);", ad).group(1)) == min_feat
    assert int(re.search(r"kEssentialGraphIterations = (\d+);", ad).group(1)) == iters
    assert float(re.search(r"kEssentialGraphIcpInformation = ([0-9.]+);", ad).group(1)) == icp
    assert int(re.search(r"kEssentialGraphIcpMinInliers = (\d+);", ad).group(1)) == int(gates.group(1))
    assert float(re.search(r"kEssentialGraphIcpMaxError = ([0-9.]+);", ad).group(1)) == float(gates.group(2))
    from geoflowslam_amd import synth
    p = synth.pose_graph(0, 10)
    assert (p["iterations"], p["lambda_init"]) == (iters, lam)


def test_new_entry_points(api):
    L = api.lib()
    for s in ("gfs_essential_graph_create", "gfs_essential_graph_destroy", "gfs_essential_graph_optimize", "gfs_essential_graph_correct_points",
              "gfs_essential_graph_last_info", "gfs_test_essential_graph_first_trial", "gfs_test_essential_graph_lists"):
        assert hasattr(L, s), s
        assert s in api.ABI_SYMBOLS, s
    for m in ("OptimizeEssentialGraph", "correct_points", "last_info"):
        assert callable(getattr(api.EssentialGraphOptimizer, m, None)), m
    assert callable(api.essential_graph_first_trial)
    if api.device_count() == 0:
        with pytest.raises(api.GfsError):
            api.EssentialGraphOptimizer(max_vertices=8, max_edges=16, max_points=16)
        assert L.gfs_essential_graph_optimize(None, None, None) == -1
