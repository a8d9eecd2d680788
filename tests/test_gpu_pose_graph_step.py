"""GPU test of the essential graph's linear step (gfs_test_essential_graph_first_trial: the production launch sequence up to the
first trial) against the float64 restatement (tests/pose_graph_support.py): the assembled system block row by block row, the
right-hand side, the step x and the trial's chi2.

The tolerance is the reference rule's own noise, measured per case: the spread between the float64 and the long-double restatement,
relative to the largest entry of the block row (of the vector; of chi2).  Two float64 evaluations each sit within one spread of the
exact value, and a factor 2 on top is for the device's acos / log / exp differing from glibc's by a few ulp: the GPU gets 4 x the
spread.  A tolerance above 1e-5 would mean the case is ill-posed.  Structural zeros -- blocks of pairs that share no edge, and with a
fixed scale the absence of a scale dimension -- are exactly zero.

Every case runs at the first lambda of the full solves, 1e-16, which in double leaves H as it is; LAMBDA_CASES run also at 1e-3, 1 and
1e3 times the largest diagonal entry of H, where a lambda that is missing, or on the wrong rows, moves x by far more than the bar
(tests/test_pose_graph_levenberg_inputs.py holds the inputs to that, without a GPU)."""
import numpy as np
import pytest

import pose_graph_support as pg

pytestmark = pytest.mark.gpu


def _ring(F, fix_scale):
    """F free vertices behind one fixed vertex, joined the way an essential graph is: every vertex to its predecessor and to the one
    two back, the ends closed on vertex 0, a few edges the other way round.  Every measurement carries noise of its own: on
    synth.pose_graph's maps most edges are measured on the estimates themselves, their right-hand side is rounding noise alone and a
    spread relative to it says nothing."""
    V = F + 1
    edges = [(i, i - 1) for i in range(1, V)] + [(i, i - 2) for i in range(2, V)] + [(V - 1, 0), (0, V - 1)] + [(i - 3, i) for i in range(3, V, 5)] + \
        [(i, i - 4) for i in range(4, V)] + [(i, 0) for i in range(2, V, 3)]
    # (seeds at which the float64 / long-double spread of the step stays below 1e-5 / 4 with room: about two of three seeds do)
    seed = {(1, True): 63, (2, True): 66, (16, True): 66, (17, True): 62, (33, True): 64, (1, False): 71, (13, False): 69, (14, False): 65,
            (28, False): 67}[(F, fix_scale)]
    return pg.random_graph(seed, [1] + [0] * F, edges, fix_scale, extent=1.0)


def _branch_map():
    """free scale, residuals on both sides of eps in sigma and in the angle (the log's angle seam is at acos(1 - eps) = 4.5e-3)"""
    rng = np.random.default_rng(8)
    V = 16
    edges = [(i, i - 1) for i in range(1, V)] + [(i, i - 3) for i in range(3, V)] + [(i - 5, i) for i in range(5, V)] + [(i, 0) for i in range(2, V, 2)]
    E = len(edges)
    k = np.arange(E) % 4
    axis = rng.normal(size=(E, 3))
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    # (sigma well away from zero on its large side: sim3.h:199's B grows like sigma^-3 and would make the case ill-posed)
    theta = np.where(k % 2 == 0, rng.uniform(1e-4, 1e-3, E), rng.uniform(0.01, 0.05, E))
    sigma = np.where(k < 2, rng.uniform(-8e-6, 8e-6, E), rng.uniform(0.02, 0.05, E) * rng.choice([-1, 1], E))
    steps = np.concatenate([axis * theta[:, None], rng.normal(0, 0.05, (E, 3)), sigma[:, None]], 1)
    return pg.random_graph(8, [1] + [0] * (V - 1), edges, False, steps, extent=1.0)


CASES = {f"fixed_scale_F{F}": (lambda F=F: _ring(F, True)) for F in (1, 2, 16, 17, 33)}
CASES.update({f"free_scale_F{F}": (lambda F=F: _ring(F, False)) for F in (1, 13, 14, 28)})
CASES.update({f"structure_{k}_{'fixed' if fs else 'free'}": (lambda k=k, fs=fs: pg.random_graph(7, *pg.STRUCTURE_CASES[k], fs, extent=1.0))
              for k in pg.STRUCTURE_CASES for fs in (True, False)})
CASES["eps_branches"] = _branch_map


LAMBDA_CASES = ["fixed_scale_F1", "fixed_scale_F17", "fixed_scale_F33", "free_scale_F14", "free_scale_F28"] + \
    [f"structure_{k}_{fs}" for k in ("free_vertex_without_edge", "duplicates_both_orientations") for fs in ("fixed", "free")]
LAMBDA_FACTORS = (1e-3, 1.0, 1e3)


def lambda_problem(name, factor):
    """the case with lambda_init = factor x the largest diagonal entry of the float64 restatement's H at the starting estimate"""
    p = CASES[name]()
    G = pg.PoseGraph(p)
    return dict(p, lambda_init=float(factor * np.abs(np.diag(G.system(G.est)[0])).max()))


def edgeless_free_slots(p):
    """free slots of the vertices that no edge touches"""
    G = pg.PoseGraph(p)
    return [f for f, v in enumerate(G.free_vert) if v not in set(G.ei.tolist()) | set(G.ej.tolist())]


@pytest.fixture(scope="module")
def opt(gpu_api):
    o = gpu_api.EssentialGraphOptimizer(max_vertices=48, max_edges=256, max_points=16)
    yield o
    o.close()


def _reference(p, dtype):
    G = pg.PoseGraph(p, dtype)
    H, b, chi = G.system(G.est)
    x, ok, trial, scale = G.step(G.est, H, b, p["lambda_init"])
    return G, H + dtype(p["lambda_init"]) * np.eye(G.n, dtype=dtype), b, x, G.total(chi), G.total(G.errors(trial)[1]), ok


@pytest.mark.parametrize("name", sorted(CASES))
def test_first_trial(gpu_api, opt, name):
    _check_first_trial(gpu_api, opt, name, CASES[name]())


@pytest.mark.parametrize("factor", LAMBDA_FACTORS)
@pytest.mark.parametrize("name", LAMBDA_CASES)
def test_first_trial_at_a_lambda_that_matters(gpu_api, opt, name, factor):
    """The same comparison, under the same bars, at lambda = factor x max |diag H|: lambda on every diagonal entry of every free
    vertex (the scale's too, the second panel's too) and in computeScale's lambda x term, or H, x and the trial's chi2 miss the bars
    by orders of magnitude.  A free vertex without an edge has lambda I for its diagonal block and a step of exactly zero."""
    p = lambda_problem(name, factor)
    t = _check_first_trial(gpu_api, opt, f"{name} at lambda {p['lambda_init']:.3g}", p)
    G = pg.PoseGraph(p)
    Hg = np.zeros((G.n, G.n))
    Hg[np.tril_indices(G.n)] = t["H"]
    slots = edgeless_free_slots(p)
    assert bool(slots) == ("free_vertex_without_edge" in name)
    for f in slots:
        rows = slice(G.dim * f, G.dim * f + G.dim)
        assert (Hg[rows, rows] == p["lambda_init"] * np.eye(G.dim)).all() and (Hg[rows, :G.dim * f] == 0).all() and (Hg[G.dim * f + G.dim:, rows] == 0).all()
        assert (t["x"][rows] == 0).all() and (t["b"][rows] == 0).all()


def _check_first_trial(gpu_api, opt, name, p):
    G, H, b, x, chi, trial_chi, ok = _reference(p, np.float64)
    _, Hl, bl, xl, chil, trial_chil, _ = _reference(p, np.longdouble)
    t = gpu_api.essential_graph_first_trial(opt, p)
    n, dim, F = G.n, G.dim, G.F
    assert (t["n_free"], t["dimension"], t["solve_ok"]) == (F, dim, 1) and ok
    info = opt.last_info()
    assert info["panels"] == -(-n // gpu_api.gba_panel_rows()) and info["trials"] == 1
    if name == "eps_branches":
        br = pg.edge_residual(G.meas, G.est[G.ei], G.est[G.ej])[1]
        assert (np.bincount(br, minlength=4) > 0).all(), np.bincount(br, minlength=4)
    Hg = np.zeros((n, n))
    Hg[np.tril_indices(n)] = t["H"]  # packed lower triangle, row by row
    assert np.isfinite(t["H"]).all() and np.isfinite(t["b"]).all() and np.isfinite(t["x"]).all()
    # structural zeros: where the restatement never added anything the device holds exactly +0
    L = np.tril(np.ones((n, n), bool))
    never = (np.asarray(H) == 0) & L
    assert (Hg[never] == 0).all()
    worst = dict(H=0.0, b=0.0, x=0.0)
    tol_max = 0.0
    for f in range(F):
        rows = slice(dim * f, dim * f + dim)
        for key, got, ref, refl in (("H", np.tril(Hg)[rows], np.tril(H)[rows], np.tril(np.asarray(Hl))[rows]),
                                    ("b", t["b"][rows], b[rows], bl[rows]), ("x", t["x"][rows], x[rows], xl[rows])):
            big = float(np.abs(refl).max())
            if big == 0:  # a free vertex without an edge: lambda alone on the diagonal, nothing in b and x
                assert (got == ref).all()
                continue
            spread = float(np.abs(ref - refl.astype(np.float64)).max()) / big
            err = float(np.abs(got - ref).max()) / big
            tol_max = max(tol_max, 4 * spread)
            worst[key] = max(worst[key], err / spread if spread > 0 else (0.0 if err == 0 else np.inf))
    spread_chi = abs(float(trial_chi) - float(trial_chil)) / float(trial_chil)
    err_chi = abs(t["trial_chi2"] - float(trial_chi)) / float(trial_chil)
    print(f"{name}: n = {n}; GPU error in units of the float64 / long-double spread: H {worst['H']:.2f} b {worst['b']:.2f} x {worst['x']:.2f}; "
          f"largest tolerance {tol_max:.1e}; trial chi2: spread {spread_chi:.1e} GPU {err_chi:.1e}; chi2 {t['chi2']:.6g}")
    assert tol_max <= 1e-5 and 4 * spread_chi <= 1e-5, "the case is ill-posed: replace it"
    assert t["chi2"] == float(chi) or abs(t["chi2"] - float(chi)) <= 4 * abs(float(chi) - float(chil))
    assert max(worst.values()) <= 4.0
    assert err_chi <= 4 * spread_chi
    return t
