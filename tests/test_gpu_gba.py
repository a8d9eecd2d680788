"""GPU tests of GlobalBundleAdjustment (MI355X), gfs_gba_solve: the first Levenberg-Marquardt trial stage by stage against the
longdouble reference and the derived bars of tests/lba_step_support.py (through gfs_test_gba_first_trial, a tap in the product's own
sequence); complete solves against oracle.lba_solve under the bars of tests/test_gpu_lba.py; the same input twice; the scripted stop
flag; and gfs_lba_solve's bits against the digest recorded from the parent commit.

P = gba_panel_rows() rows make a tile of the reduced system, Fp = P // 6 free poses fill one.  The free-pose counts are the smallest at
which each path of the tiled factorisation runs: 1, 2, Fp (one tile), Fp + 1 (a second panel, the first trailing update), 2 Fp,
2 Fp + 1 (a tile that is updated twice).  The maps are tests/gba_support.py's."""
import numpy as np
import pytest

import gba_support as G
import lba_parent_support as LP
import lba_step_support as S
import lba_stop_support as ST

pytestmark = pytest.mark.gpu
if not S.LONGDOUBLE_OK:
    pytest.skip("np.longdouble is not wider than float64 on this machine", allow_module_level=True)

_CAP = dict(max_poses=48, max_points=512, max_edges=16384)
_FILL = -7.25e301  # pre-written into the hook's arrays: no step holds it
_TRIAL_KEYS = ("Dinv", "Hs", "bs", "xp", "xl")
_OUT_KEYS = ("pose_q", "pose_t", "points", "edge_chi2", "edge_depth_positive")


@pytest.fixture(scope="module")
def Fp(gpu_api):
    return gpu_api.gba_panel_rows() // 6


@pytest.fixture(scope="module")
def gopt(gpu_api):
    o = gpu_api.GlobalOptimizer(**_CAP)
    yield o
    o.close()


@pytest.fixture(scope="module")
def lopt(gpu_api):
    o = gpu_api.Optimizer(**_CAP)  # gfs_lba_linearize: the blocks of the state the first trial starts from (the same build kernels)
    yield o
    o.close()


def _fmt(figs):
    return " ".join(f"{k}={v:.3g}/{a:.3g}" for k, (v, a) in figs.items())


def _bits(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in _OUT_KEYS) + \
        np.array([r["iterations_run"], r["final_chi2"], r["final_lambda"]], np.float64).tobytes()


@pytest.mark.parametrize("index", range(13))
def test_first_trial_stage_by_stage(gpu_api, gopt, lopt, Fp, index):
    name, make = G.step_cases(Fp)[index]
    w = make()
    L = lopt.linearize(w)
    T = gpu_api.gba_first_trial(gopt, w, fill=_FILL)
    st = S.structure(w)
    for k in _TRIAL_KEYS:
        assert not (T[k] == _FILL).any(), (name, k, "entries not delivered", int((T[k] == _FILL).sum()))
        assert np.isfinite(T[k]).all(), (name, k)
    assert T["solve_ok"] == 1, name
    figs, failed = S.check_step(L, st, T)
    info = gopt.last_info()
    print(f"{name}: F={st['F']} N={st['N']} panels={info['panels']} blocks={info['block_pairs']} {_fmt(figs)}")
    assert not failed, (name, failed, _fmt(figs))
    assert not S.unshared_blocks_are_zero(T["Hs"], st), (name, "a pose pair without a common landmark has a non-zero block")
    assert info["n_free"] == st["F"] and info["panel_rows"] == 6 * Fp and info["panels"] == -(-st["F"] // Fp) and info["trials"] == 1
    unshared = int(np.tril(st["shared"] == 0, -1).sum())
    assert info["block_pairs"] == st["F"] * (st["F"] + 1) // 2 - unshared
    # the lists the product built from its own preparation are the ones the host hook builds (tests/test_gba_lists.py checks those)
    lists = gpu_api.gba_lists(w)
    assert info["block_pairs"] == len(lists["blk_ij"]) and info["contributions"] == len(lists["contrib"])
    if st["F"] > Fp:
        assert unshared > 0, "every pair of this map shares a landmark: sparsity is not exercised"
    if name == "isolated-pose":
        assert (st["shared"] - np.diag(np.diag(st["shared"])) == 0).all(1).any()
    if name == "fixed-only-landmark":
        assert (~st["seen"].any(0)).any()


def test_zero_pivot_ends_the_solve_like_the_local_one(gpu_api, gopt, lopt, Fp):
    """every information matrix zero on the isolated-pose map: lambda = 0, the reduced system has no finite pivot.  solve_ok = 0 from
    the first panel, every later kernel of the trial leaves, and the LM loop ends the way gfs_lba_solve ends it: ten rejected trials,
    one iteration counted, the estimate untouched."""
    w = dict(G.structure_cases(Fp)[0][1](), iterations=10)
    w["edge_inv_sigma2"] = np.zeros_like(w["edge_inv_sigma2"])
    T = gpu_api.gba_first_trial(gopt, w, fill=_FILL)
    assert T["solve_ok"] == 0 and T["lam"] == 0.0
    r, rl = gopt.BundleAdjustment(w), lopt.LocalBundleAdjustment(w)
    assert r["iterations_run"] == rl["iterations_run"] == 1
    assert gopt.last_info()["trials"] == 10
    for k in ("pose_q", "pose_t", "points"):
        assert np.array_equal(r[k], rl[k]), k
    assert np.array_equal(r["points"], w["points"]) and r["final_chi2"] == rl["final_chi2"]


@pytest.fixture(scope="module")
def oracle_solutions(oracle, Fp):
    """every full-solve map solved once by the oracle, shared"""
    return {name: oracle.lba_solve(G.full_solve_map(name, Fp)) for name in G.FULL_SOLVES}


@pytest.mark.parametrize("name", G.FULL_SOLVES)
def test_solve_matches_oracle(gopt, oracle_solutions, Fp, name):
    w = G.full_solve_map(name, Fp)
    r = gopt.BundleAdjustment(w)
    info = gopt.last_info()
    print(name, "F", info["n_free"], "panels", info["panels"], "trials", info["trials"], "launches", info["launches"])
    ST.assert_matches_oracle(w, r, oracle_solutions[name], name, lam=False)
    assert info["panels"] == -(-info["n_free"] // Fp)


def test_robust_false_substitutes_infinite_thresholds(gopt, Fp):
    w = G.full_solve_map("Fp+1-robust", Fp)
    plain = G.full_solve_map("Fp+1-plain", Fp)
    assert _bits(gopt.BundleAdjustment(w, robust=False)) == _bits(gopt.BundleAdjustment(plain))
    assert _bits(gopt.BundleAdjustment(w)) != _bits(gopt.BundleAdjustment(plain))


def test_same_input_twice_gives_the_same_bits(gpu_api, gopt, Fp):
    w = G.full_solve_map("2Fp+1-robust", Fp)
    first = _bits(gopt.BundleAdjustment(w))
    gopt.BundleAdjustment(G.full_solve_map("Fp+1-plain", Fp))  # (another map in between)
    assert _bits(gopt.BundleAdjustment(w)) == first
    fresh = gpu_api.GlobalOptimizer(**_CAP)
    assert _bits(fresh.BundleAdjustment(w)) == first
    fresh.close()


def test_scripted_stop_flag(gpu_api, oracle, gopt, Fp):
    w = G.stop_map(Fp)
    ro, trace = oracle.lba_solve_scripted(w)
    looks = G.gba_looks(trace, w["iterations"])
    assert any(kind == "reject" for kind, _ in looks) and looks[0] == ("top", 0)
    flag = np.zeros(1, np.int32)
    free = gopt.BundleAdjustment(w, stop_flag=flag)
    ST.assert_matches_oracle(w, free, ro, "unstopped", lam=False)
    assert gpu_api.lba_last_looks()["looks"] == len(looks)
    for look, (kind, k) in enumerate(looks):
        gpu_api.lba_stop_at_look(look)
        r = gopt.BundleAdjustment(w, stop_flag=flag)
        seen = gpu_api.lba_last_looks()
        assert seen["looks"] == look + 1, (look, seen)
        if look == 0:  # no entry check: GFS_OK, nothing run, the caller's estimate bit for bit
            assert r["iterations_run"] == 0
            for key in ("pose_q", "pose_t", "points"):
                assert r[key].tobytes() == np.ascontiguousarray(w[key], np.float64).tobytes(), key
            continue
        want, _ = oracle.lba_solve_scripted(w, stop_at_look=look + 1)
        if kind == "reject":
            # the oracle's edges keep the rejected trial's errors; gfs_gba_solve reports them at the estimate it returns
            want = dict(want, edge_chi2=oracle.lba_solve(dict(w, iterations=0, pose_q=want["pose_q"], pose_t=want["pose_t"],
                                                              points=want["points"]))["edge_chi2"])
            assert seen["forced_decides"] == 1
        ST.assert_matches_oracle(w, r, want, f"look {look} ({kind} {k})", lam=False)
        if kind == "top":  # the state after k complete iterations: the same handle asked for k iterations
            assert r["iterations_run"] == k
            assert _bits(r) == _bits(gopt.BundleAdjustment(dict(w, iterations=k))), (look, k)


def test_capacity_is_refused(gpu_api, gopt, Fp):
    w = G.gmap(_CAP["max_poses"], 100, 3)  # one key-frame more than the handle holds
    with pytest.raises(gpu_api.GfsError) as e:
        gopt.BundleAdjustment(w)
    assert e.value.code == -4


def test_local_bundle_adjustment_keeps_the_parents_bits(gpu_api):
    rec = LP.load()
    assert rec["parent_commit"] == "8dc13f6" and rec["window"] == LP.WINDOW
    got = LP.digests(gpu_api)
    assert got["window"] == rec["sha256"]["window"], "the window is not the recorded one"
    assert got == rec["sha256"], [k for k in got if got[k] != rec["sha256"][k]]
