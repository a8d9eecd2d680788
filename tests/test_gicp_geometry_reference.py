"""CPU half of the GICP geometry tests (tests/test_gpu_gicp_geometry.py is the GPU half): pins the brute-force references of
tests/gicp_geometry_support.py against the oracle, and the caps the GPU tests rest on, for the REFERENCE ALONE -- before any kernel
is involved.  Every cloud here is something other than a depth-camera raster; this is also the first time the oracle's KdTree sees
such geometry.  Caps (not to be raised: if a parameter change breaks one, pick another seed):
  exact ties between the 10th and 11th squared distance   0 per cloud
  points with relative eigen-gap <= 1e-3                   <= 5 % of a cloud (`line`: all of them, by construction)
  1-NN ties / distances within 1e-12 of the gate           0 per pair
  d_or_cov = max |oracle cov - reference_cov| (gap > 1e-3) <= 1e-9
  d_or_lin = oracle's one-iteration sums vs reference      <= 1e-12"""
import numpy as np
import pytest

import gicp_geometry_support as G

CASES = [(n, s) for s in G.SEEDS for n in G.NAMES]
PAIRS = [(n, s) for n, s in CASES if not (n.startswith("tiny_") and int(n[5:]) < 10)]


def test_generators_are_deterministic_and_shaped():
    for name, seed in CASES:
        a, b = G.cloud(name, seed), G.cloud(name, seed)
        assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 4 and (a[:, 3] == 1).all() and np.array_equal(a, b), name
        assert np.isfinite(a).all()
        s1, T1, _ = G.moved(a, seed)
        s2, T2, _ = G.moved(a, seed)
        assert np.array_equal(s1, s2) and np.array_equal(T1, T2) and s1.shape == a.shape and s1.dtype == np.float32
    assert [len(G.cloud("tiny_%d" % m, 0)) for m in G.TINY] == list(G.TINY)
    # points exactly on cell faces survive the float32 round trip
    w = G.cloud("wall_and_cell_faces", 0)[-400:, 0]
    k = np.rint(w.astype(np.float64) * 10).astype(np.int64)
    assert (w == k.astype(np.float32) * np.float32(0.1)).all()
    assert not np.array_equal(G.cloud("sparse_uniform", 0), G.cloud("sparse_uniform", 1))


def test_brute_force_helpers_on_hand_made_input():
    # a 1-D lattice: the point at 0 has neighbours at +-1, +-2, ...: every k-th / (k+1)-th pair with even k ties exactly
    p = np.zeros((25, 3))
    p[:, 0] = np.arange(25) - 12.0
    idx, sq, tie = G.brute_knn(p, 2)
    assert idx[12].tolist() == [12, 11] and sq[12].tolist() == [0.0, 1.0] and tie[12] and not tie[0]  # equal distances: lower index
    idx, sq, tie = G.brute_knn(p, 3)
    assert set(idx[12]) == {11, 12, 13} and not tie[12] and sq[0].tolist() == [0.0, 1.0, 4.0]
    assert G.near_ties(p, 2) == 23 and G.near_ties(p, 3) == 0 and G.near_ties(p[:2], 2) == 0
    q = p.copy()
    q[13, 0] += 1e-13  # not an exact tie any more, but below the keys' resolution
    assert not G.brute_knn(q, 2)[2][12] and G.near_ties(q, 2) == 23
    q[13, 0] += 1e-6  # the points at 0, 1 and 2 lose their ties
    assert G.near_ties(q, 2) == 20
    assert G.cube_counts(p * 0.1 + 0.05).tolist() == [2] + [3] * 23 + [2]
    # fewer points than k: every point is a neighbour; < 5 neighbours: identity
    idx, sq, tie = G.brute_knn(p[:4], 10)
    assert idx.shape == (4, 4) and not tie.any()
    cov, gap = G.reference_cov(p[:4], idx)
    assert (cov == np.eye(3)).all() and (gap == 1).all()
    # a plane z = 0: normal (0, 0, 1), cov = diag(1, 1, 1e-3)
    rng = np.random.default_rng(0)
    pl = np.c_[rng.uniform(0, 1, (30, 2)), np.zeros(30)]
    idx, _, _ = G.brute_knn(pl, 10)
    cov, gap = G.reference_cov(pl, idx)
    assert np.abs(cov - np.diag([1, 1, 1e-3])).max() < 1e-14 and gap.min() > 1e-3


def test_reference_linearize_is_the_gradient_and_gauss_newton_matrix_of_its_error():
    """H and b of reference_linearize against central differences of its own error in the right-multiplied twist (rotation first):
    b = de/dx exactly (the Mahalanobis matrix does not depend on the translation, and on the rotation only through R Cs R^T, which
    the factor holds fixed while it differentiates: so the check moves the points only)."""
    rng = np.random.default_rng(3)
    pt = np.c_[rng.uniform(-1, 1, (200, 3)), np.ones(200)]
    ps = pt + np.c_[rng.normal(0, 0.003, (200, 3)), np.zeros(200)]
    cov = np.broadcast_to(np.eye(3), (200, 3, 3)).copy()  # isotropic: R Cs R^T does not depend on R
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = G.rotvec([0.01, 0.02, -0.01]), [0.004, -0.002, 0.003]
    r0 = G.reference_linearize(pt, cov, ps, cov, T)
    assert r0["num_inliers"] == 200 and r0["nn_ties"] == 0 and r0["at_gate"] == 0
    h = 1e-6
    g = np.zeros(6)
    for a in range(6):
        e = []
        for sgn in (1, -1):
            d = np.zeros(6)
            d[a] = sgn * h
            D = np.eye(4)
            D[:3, :3], D[:3, 3] = G.rotvec(d[:3]), d[3:]
            e.append(G.reference_linearize(pt, cov, ps, cov, T @ D)["error"])
        g[a] = (e[0] - e[1]) / (2 * h)
    assert np.abs(g - r0["b"]).max() <= 1e-6 * np.abs(r0["b"]).max(), (g, r0["b"])
    assert np.abs(r0["H"] - r0["H"].T).max() <= 1e-12 * np.abs(r0["H"]).max() and np.linalg.eigvalsh(r0["H"]).min() > 0
    # beyond the gate: no inliers, zero sums
    far = ps.copy()
    far[:, 2] += 5
    rz = G.reference_linearize(pt, cov, far, cov, np.eye(4))
    assert rz["num_inliers"] == 0 and not rz["H"].any() and rz["error"] == 0


@pytest.mark.parametrize("name,seed", CASES)
def test_oracle_kdtree_returns_the_brute_force_neighbours(oracle, name, seed):
    for which in (False, True):
        f = G.facts(name, seed, which)
        po, m = f["po"], len(f["po"])
        kk = min(G.K, m)
        oi, osq = oracle.knn(po, po, kk)
        ok = ~f["tie"]
        assert ok.all(), "exact 10th/11th ties: see the caps"
        assert (np.sort(oi, 1) == np.sort(f["idx"], 1)).all(), int((np.sort(oi, 1) != np.sort(f["idx"], 1)).any(1).sum())
        assert np.abs(np.sort(osq, 1) - f["sq"]).max() <= 1e-15 * max(f["sq"].max(), 1e-300)
        assert (oi[:, 0] == np.arange(m)).all() and (osq[:, 0] == 0).all()


@pytest.mark.parametrize("name,seed", CASES)
def test_caps_hold_for_the_reference_alone(oracle, name, seed):
    for which in (False, True):
        f = G.facts(name, seed, which)
        m = len(f["po"])
        bad = int((f["gap"] <= G.GAP_MIN).sum())
        print(f"{name} s{seed} {'source' if which else 'target'}: m {m} ties {int(f['tie'].sum())} near-ties {f['near_ties']} gap<=1e-3 {bad}")
        assert int(f["tie"].sum()) <= 0
        if which:
            continue  # (a source's covariances reach the checks only as the GPU's own, through reference_linearize)
        if name == "line":
            assert bad == m
        else:
            assert bad <= 0.05 * m
        # no k-th distance sits on the one threshold the path test uses without a margin (one cell, to the keys' resolution)
        assert not (np.abs(f["d10"] - G.CELL) <= 1e-9 * G.CELL).any()
    if (name, seed) in PAIRS:
        r = G.pair_facts(name, seed)["ref"]
        print(f"{name} s{seed} pair: inliers {r['num_inliers']} 1-NN ties {r['nn_ties']} at the gate {r['at_gate']}")
        assert r["nn_ties"] == 0 and r["at_gate"] == 0


@pytest.mark.parametrize("name,seed", CASES)
def test_oracle_is_within_its_caps_of_the_independent_references(oracle, name, seed):
    f = G.facts(name, seed)
    print(f"{name} s{seed}: d_or_cov {f['d_or_cov']:.2e}")
    assert f["d_or_cov"] <= 1e-9
    assert np.abs(f["co"] - f["co"].transpose(0, 2, 1)).max() <= 1e-15 if len(f["co"]) else True
    if len(f["po"]) < 5:
        assert (f["co"] == np.eye(3)).all() and (f["ref"] == np.eye(3)).all()
    if (name, seed) in PAIRS:
        p = G.pair_facts(name, seed)
        ro, r = p["oracle1"], p["ref"]
        print(f"{name} s{seed}: d_or_lin {p['d_or_lin']:.2e} inliers {r['num_inliers']} of {ro['n_source_ds']}")
        assert ro["num_inliers"] == r["num_inliers"] and ro["iterations"] == 0
        assert r["num_inliers"] >= 0.5 * ro["n_source_ds"]  # no vacuous pair (far_from_origin: the motion is about the centroid)
        assert p["d_or_lin"] <= 1e-12


def test_ill_conditioned_points_with_the_oracles_own_eigen_arithmetic(oracle):
    """Where the eigen-gap is below 1e-3 the oracle is compared with closed_form_cov: the brute-force neighbours, the oracle's sums and
    eig3_direct.  Same arithmetic on the same set: equal to rounding of the final products; and the oracle's normal minimises the scatter."""
    for name, seed in CASES:
        f = G.facts(name, seed)
        sel = np.nonzero(f["gap"] <= G.GAP_MIN)[0]
        if not len(sel):
            continue
        cf = G.closed_form_cov(f["po"], f["idx"], oracle, sel)
        d = float(np.abs(cf - f["co"][sel]).max())
        print(f"{name} s{seed}: {len(sel)} ill-conditioned points, |oracle - closed_form_cov| {d:.2e}")
        assert d <= 1e-12
        w, _ = np.linalg.eigh(f["co"][sel])
        assert np.abs(w - np.array([1e-3, 1, 1])).max() <= 1e-9


def test_every_pass_owns_at_least_500_points():
    """The path assertions of the GPU test are not vacuous: from the true k-th distances, each of k_knn_cov (d10 within a cell: must be
    certified), the r = 2 pass (0.15 < d10 <= 0.2: must be deferred once, may not need the isolated pass) and the isolated pass
    (d10 > 0.2) has at least 500 points that can only be its own; and the unbounded probe (fewer than k points in the 27-cube)."""
    tot = dict(certified=0, r2=0, isolated=0, unbounded=0)
    for name, seed in CASES:
        f = G.facts(name, seed)
        pc = G.path_counts(f)
        wide = bool((f["extent"] > 0.5).any())
        print(f"{name} s{seed}: {pc}" + ("" if wide else " (within 0.5 m: lower bounds not asserted)"))
        tot["certified"] += pc["within_cell"] - pc["near_ties"]
        if wide:
            tot["r2"] += pc["must_r2"] - pc["must_isolated"]
            tot["isolated"] += pc["must_isolated"]
            tot["unbounded"] += pc["unbounded"]
        if name in ("wall_and_cell_faces", "dense_blob", "far_from_origin"):
            assert pc["beyond_cell"] + pc["near_ties"] == 0  # these must defer nothing at all
    print(tot)
    assert min(tot.values()) >= 500, tot
