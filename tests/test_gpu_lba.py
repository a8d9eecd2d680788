"""GPU parity tests for LocalBundleAdjustment (MI355X): normal-equation blocks within 1e-10 relative of the CPU
oracle, optimised poses / points within 1e-5 relative Frobenius (BASELINE.json north_star tolerance), identical
outlier classification, LM iteration counts equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

from geoflowslam_amd import synth
from lba_step_support import with_second_camera_edges as _with_second_camera_edges

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300)


def test_linearize_blocks_match_oracle(gpu_api, oracle):
    w = synth.lba_window(0, n_free=20, n_fixed=5, n_points=3000)  # BASELINE.json configs[4]
    opt = gpu_api.Optimizer()
    L = opt.linearize(w)
    Lo = oracle.lba_linearize(w)
    for k in ("Hpp", "Hll", "Hpl", "bp", "bl", "edge_chi2"):
        assert _rel(L[k], Lo[k]) < 1e-10, (k, _rel(L[k], Lo[k]))
    assert abs(L["chi2"] - Lo["chi2"]) < 1e-9 * Lo["chi2"]


@pytest.mark.parametrize("cfg", [dict(seed=0, n_free=20, n_fixed=5, n_points=3000),
                                 dict(seed=1, n_free=8, n_fixed=3, n_points=600),
                                 dict(seed=2, n_free=3, n_fixed=1, n_points=80, mono_frac=1.0),
                                 dict(seed=3, n_free=30, n_fixed=2, n_points=400),
                                 dict(seed=5, n_free=31, n_fixed=2, n_points=500),    # first size factored in HBM instead of LDS
                                 dict(seed=6, n_free=48, n_fixed=6, n_points=1500),
                                 dict(seed=7, n_free=80, n_fixed=4, n_points=800)])
def test_solve_matches_oracle(gpu_api, oracle, cfg):
    w = synth.lba_window(**cfg)
    opt = gpu_api.Optimizer(max_poses=96, max_points=4096, max_edges=200000)
    r = opt.LocalBundleAdjustment(w)
    ro = oracle.lba_solve(w)
    assert r["iterations_run"] == ro["iterations_run"]
    for i in range(w["n_poses"]):
        assert _rel(r["pose_q"][i], ro["pose_q"][i]) < 1e-5 and _rel(r["pose_t"][i], ro["pose_t"][i]) < 1e-5
    assert _rel(r["points"], ro["points"]) < 1e-5
    assert _rel(r["final_chi2"], ro["final_chi2"]) < 1e-6
    thr = np.where(w["edge_stereo"] == 1, 7.815, 5.991)
    near = np.abs(ro["edge_chi2"] - thr) < 1e-4 * thr
    assert ((r["edge_chi2"] > thr) == (ro["edge_chi2"] > thr))[~near].all()
    assert (r["edge_depth_positive"] == ro["edge_depth_positive"]).all()


def test_edge_cases(gpu_api, oracle):
    opt = gpu_api.Optimizer()
    w = synth.lba_window(4, n_free=3, n_fixed=2, n_points=50)
    # shuffled (not landmark-major) edge order gives the same answer
    perm = np.random.default_rng(0).permutation(w["n_edges"])
    ws = dict(w)
    for k in ("edge_pose", "edge_point", "edge_obs", "edge_inv_sigma2", "edge_stereo"):
        ws[k] = w[k][perm]
    r, rs = opt.LocalBundleAdjustment(w), opt.LocalBundleAdjustment(ws)
    assert _rel(rs["points"], r["points"]) < 1e-9 and _rel(rs["edge_chi2"], r["edge_chi2"][perm]) < 1e-6
    # zero iterations: estimates untouched
    w0 = dict(w); w0["iterations"] = 0
    r0 = opt.LocalBundleAdjustment(w0)
    assert r0["iterations_run"] == 0 and np.allclose(r0["points"], w["points"])
    # every pose fixed: only landmarks move
    wf = dict(w); wf["pose_fixed"] = np.ones_like(w["pose_fixed"])
    rf, of = opt.LocalBundleAdjustment(wf), oracle.lba_solve(wf)
    assert (rf["pose_t"] == w["pose_t"]).all() and _rel(rf["points"], of["points"]) < 1e-5
    # stop flag already raised: the reference returns before optimising (src/Optimizer.cc:1955-1956)
    assert opt.LocalBundleAdjustment(w, stop_flag=np.ones(1, np.int32)) is None
    # stop flag present but not raised: normal result
    rn = opt.LocalBundleAdjustment(w, stop_flag=np.zeros(1, np.int32))
    assert _rel(rn["points"], r["points"]) == 0


def test_stop_flag_raised_while_solving(gpu_api, oracle):
    """setForceStopFlag semantics (src/Optimizer.cc:1679): raising the flag during optimize() ends it at the next check
    (top of an iteration / end of an LM trial); the estimate is then a state some earlier iteration reached."""
    import threading
    import time
    w = synth.lba_window(0, n_free=20, n_fixed=5, n_points=3000)
    opt = gpu_api.Optimizer()
    full = opt.LocalBundleAdjustment(w)
    flag = np.zeros(1, np.int32)

    def raiser():
        time.sleep(0.0015)
        flag[0] = 1

    t = threading.Thread(target=raiser)
    t.start()
    r = opt.LocalBundleAdjustment(w, stop_flag=flag)
    t.join()
    assert r is not None and 0 <= r["iterations_run"] <= full["iterations_run"]
    assert np.isfinite(r["points"]).all() and np.isfinite(r["pose_t"]).all()
    if r["iterations_run"] < full["iterations_run"]:  # stopped early: the cost is not above the starting cost
        chi0 = oracle.lba_linearize(w)["chi2"]
        assert r["final_chi2"] <= chi0 * (1 + 1e-12)


def test_stopped_solve_is_exactly_the_state_after_its_last_iteration(gpu_api):
    """gfs_lba_solve's host loop runs one LM iteration ahead of the flags it has read (round 6).  When the caller's stop flag goes up while
    an iteration is running ahead, that iteration is discarded: the result must be, bit for bit, what optimize(k) leaves for the k
    iterations the stopped call reports -- estimates, per-edge chi2, final chi2, lambda.  The flag is scripted
    (gfs_test_lba_stop_at_look) to go up at every look of the solve in turn: the top of every iteration, and past the last one.
    (This window accepts every trial; tests/test_gpu_lba_stop.py does the same on windows that reject.)"""
    w = synth.lba_window(0, n_free=20, n_fixed=5, n_points=3000)
    opt = gpu_api.Optimizer()
    full = opt.LocalBundleAdjustment(w)
    r = opt.LocalBundleAdjustment(w, stop_flag=np.zeros(1, np.int32))
    n_looks = gpu_api.lba_last_looks()["looks"]
    assert n_looks == 1 + full["iterations_run"] and np.array_equal(r["points"], full["points"])
    seen = set()
    for look in range(1, n_looks + 1):
        gpu_api.lba_stop_at_look(look)
        r = opt.LocalBundleAdjustment(w, stop_flag=np.zeros(1, np.int32))
        L = gpu_api.lba_last_looks()
        assert r is not None
        k = r["iterations_run"]
        assert k == look - 1, (look, k)   # look 1 + k is the top of iteration k; look n_looks is never made
        seen.add(k)
        # every stop with 0 < k < the full count goes through the discard: the next iteration is always running ahead when the flags are read
        assert L["discarded"] == (1 if 0 < k < full["iterations_run"] else 0), (look, L)
        wk = dict(w)
        wk["iterations"] = k
        ref = opt.LocalBundleAdjustment(wk)  # no flag: the loop runs ahead, nothing is discarded
        if k == 0:  # the flag was up before the first iteration: nothing was evaluated (g2o computes no errors either), the estimates stand
            assert np.array_equal(r["points"], ref["points"]) and np.array_equal(r["pose_t"], ref["pose_t"]), look
            continue
        for key in ("points", "pose_t", "pose_q", "edge_chi2"):
            assert np.array_equal(r[key], ref[key]), (look, k, key)
        assert r["final_chi2"] == ref["final_chi2"] and r["final_lambda"] == ref["final_lambda"] and r["iterations_run"] == ref["iterations_run"], (look, k)
    assert seen == set(range(full["iterations_run"] + 1)), seen


def test_stop_flag_raised_while_a_batch_is_solving(gpu_api, oracle):
    """the same for gfs_lba_solve_batch: every window closes its running iteration and returns what it has"""
    import threading
    import time
    wins = [synth.lba_window(60 + k, n_free=20, n_fixed=5, n_points=2500) for k in range(6)]
    bat = gpu_api.BatchOptimizer(max_windows=len(wins), max_poses=32, max_points=4096, max_edges=65536)
    full = bat.LocalBundleAdjustment(wins)
    flag = np.zeros(1, np.int32)

    def raiser():
        time.sleep(0.002)
        flag[0] = 1

    t = threading.Thread(target=raiser)
    t.start()
    got = bat.LocalBundleAdjustment(wins, stop_flag=flag)
    t.join()
    for w, r, f in zip(wins, got, full):
        assert 0 <= r["iterations_run"] <= f["iterations_run"]
        assert np.isfinite(r["points"]).all() and np.isfinite(r["pose_t"]).all() and np.isfinite(r["pose_q"]).all()
        if r["iterations_run"] < f["iterations_run"]:
            assert r["final_chi2"] <= oracle.lba_linearize(w)["chi2"] * (1 + 1e-12)
    # the handle is usable afterwards
    again = bat.LocalBundleAdjustment(wins)
    for a, f in zip(again, full):
        assert np.array_equal(a["points"], f["points"]) and a["iterations_run"] == f["iterations_run"]


@pytest.mark.parametrize("cfg", [dict(seed=11, n_free=20, n_fixed=5, n_points=3000), dict(seed=12, n_free=6, n_fixed=2, n_points=300),
                                 dict(seed=13, n_free=30, n_fixed=3, n_points=500)])
def test_several_edges_between_one_pose_and_one_point(gpu_api, oracle, cfg):
    """g2o takes any number of edges between two vertices (their Hpl contributions share one block,
    Thirdparty/g2o/g2o/core/block_solver.hpp:143-295): blocks, solution and flags against the oracle; alone and in a batch."""
    w = _with_second_camera_edges(synth.lba_window(**cfg), cfg["seed"])
    opt = gpu_api.Optimizer(max_poses=64, max_points=4096, max_edges=100000)
    L, Lo = opt.linearize(w), oracle.lba_linearize(w)
    for k in ("Hpp", "Hll", "Hpl", "bp", "bl", "edge_chi2"):
        assert _rel(L[k], Lo[k]) < 1e-10, (k, _rel(L[k], Lo[k]))
    r, ro = opt.LocalBundleAdjustment(w), oracle.lba_solve(w)
    assert r["iterations_run"] == ro["iterations_run"]
    assert _rel(r["pose_q"], ro["pose_q"]) < 1e-5 and _rel(r["pose_t"], ro["pose_t"]) < 1e-5 and _rel(r["points"], ro["points"]) < 1e-5
    assert _rel(r["final_chi2"], ro["final_chi2"]) < 1e-6
    assert (r["edge_depth_positive"] == ro["edge_depth_positive"]).all()
    bat = gpu_api.BatchOptimizer(max_windows=2, max_poses=64, max_points=4096, max_edges=100000)
    rb = bat.LocalBundleAdjustment([w, synth.lba_window(1, n_free=8, n_fixed=3, n_points=600)])[0]
    for k in ("pose_q", "pose_t", "points", "edge_chi2"):
        assert np.array_equal(rb[k], r[k]), k


def test_lba_batch_with_degenerate_windows(gpu_api, oracle):
    """A batch mixing ordinary windows with the degenerate ones: every pose fixed (only landmarks move), zero iterations (estimates
    untouched), a single free pose, a tiny window, a window too wide for the LDS solve — each equal, bit for bit, to the same window
    solved alone."""
    base = synth.lba_window(4, n_free=3, n_fixed=2, n_points=50)
    all_fixed = dict(base, pose_fixed=np.ones_like(base["pose_fixed"]))
    zero_it = dict(base, iterations=0)
    wins = [synth.lba_window(31, n_free=12, n_fixed=3, n_points=800), all_fixed, zero_it, synth.lba_window(32, n_free=1, n_fixed=2, n_points=40),
            synth.lba_window(33, n_free=2, n_fixed=1, n_points=12), synth.lba_window(34, n_free=24, n_fixed=2, n_points=300),
            synth.lba_window(35, n_free=40, n_fixed=3, n_points=500)]  # (> 30 free poses: reduced system factored in HBM, not LDS)
    bat = gpu_api.BatchOptimizer(max_windows=len(wins), max_poses=48, max_points=1024, max_edges=65536)
    got = bat.LocalBundleAdjustment(wins)
    one = gpu_api.Optimizer(max_poses=48, max_points=1024, max_edges=65536)
    for w, r in zip(wins, got):
        r1 = one.LocalBundleAdjustment(w)
        for k in ("pose_q", "pose_t", "points", "edge_chi2", "edge_depth_positive"):
            assert np.array_equal(r[k], r1[k]), k
        assert r["iterations_run"] == r1["iterations_run"] and r["final_chi2"] == r1["final_chi2"] and r["final_lambda"] == r1["final_lambda"]
    assert got[2]["iterations_run"] == 0 and np.allclose(got[2]["points"], base["points"])
    # ... and a batch of nothing but zero-iteration windows still evaluates the errors
    only0 = bat.LocalBundleAdjustment([zero_it, zero_it])
    r1 = one.LocalBundleAdjustment(zero_it)
    for r in only0:
        assert r["iterations_run"] == 0 and np.array_equal(r["edge_chi2"], r1["edge_chi2"]) and r["final_chi2"] == r1["final_chi2"]
    assert (got[1]["pose_t"] == base["pose_t"]).all()
    of = oracle.lba_solve(all_fixed)
    assert _rel(got[1]["points"], of["points"]) < 1e-5


def test_lba_batched_windows_match_oracle_and_single(gpu_api, oracle):
    """gfs_lba_solve_batch: windows of different sizes (3 ... 20 free key-frames, 80 ... 3000 points, different iteration
    counts and numbers of rejected trials) solved together; every window against the oracle and, bit for bit, against the same
    window solved alone."""
    cfgs = [(1, 20, 5, 3000), (2, 4, 2, 120), (3, 3, 2, 80), (4, 12, 4, 1200), (5, 8, 3, 600), (6, 20, 5, 2500), (7, 5, 2, 300),
            (8, 16, 3, 2000)] * 2
    wins = [synth.lba_window(100 + k if k >= 8 else s, n_free=f, n_fixed=x, n_points=n) for k, (s, f, x, n) in enumerate(cfgs)]
    wins[3]["iterations"] = 4          # optimize(4) next to optimize(10)
    bat = gpu_api.BatchOptimizer(max_windows=len(wins), max_poses=32, max_points=4096, max_edges=65536)
    got = bat.LocalBundleAdjustment(wins)
    one = gpu_api.Optimizer(max_poses=32, max_points=4096, max_edges=65536)
    its = set()
    for w, r in zip(wins, got):
        ro = oracle.lba_solve(w)
        assert r["iterations_run"] == ro["iterations_run"]
        assert np.linalg.norm(r["points"] - ro["points"]) <= 1e-5 * np.linalg.norm(ro["points"])
        assert np.abs(r["pose_t"] - ro["pose_t"]).max() <= 1e-6
        assert np.array_equal(r["edge_depth_positive"], ro["edge_depth_positive"])
        r1 = one.LocalBundleAdjustment(w)
        for k in ("pose_q", "pose_t", "points", "edge_chi2", "edge_depth_positive"):
            assert np.array_equal(r[k], r1[k]), k
        assert r["iterations_run"] == r1["iterations_run"] and r["final_chi2"] == r1["final_chi2"] and r["final_lambda"] == r1["final_lambda"]
        its.add(r["iterations_run"])
    assert len(its) >= 2  # the windows really finish at different times
    # the stop flag raised before the call: nothing is optimised (src/Optimizer.cc:1955-1956)
    with pytest.raises(gpu_api.GfsError):
        bat.LocalBundleAdjustment(wins[:2], stop_flag=np.ones(1, np.int32))


def test_batch_mixing_one_block_and_several_block_schur_windows(gpu_api):
    """A batch that mixes windows whose reduced system is one 128 x 128 block of pose pairs (<= 21 free poses) with wider ones
    (several blocks): each window must be solved by the Schur-product instance gfs_lba_solve launches for it alone
    (k_lba_schur_mfma<true> / <false>), so the batch stays bit-identical to the single solves."""
    wins = [synth.lba_window(70 + i, n_free=nf, n_fixed=3, n_points=npt) for i, (nf, npt) in
            enumerate([(4, 300), (40, 900), (20, 800), (26, 700), (21, 500), (22, 500), (60, 1200), (3, 200)])]
    bat = gpu_api.BatchOptimizer(max_windows=8, max_poses=80, max_points=2048, max_edges=200000)
    opt = gpu_api.Optimizer(max_poses=80, max_points=2048, max_edges=200000)
    got = bat.LocalBundleAdjustment(wins)
    for w, r in zip(wins, got):
        r1 = opt.LocalBundleAdjustment(w)
        assert r["iterations_run"] == r1["iterations_run"]
        for key in ("pose_q", "pose_t", "points", "edge_chi2", "edge_depth_positive"):
            assert np.array_equal(r[key], r1[key]), (w["n_poses"], key)


_SOLVED = ("pose_q", "pose_t", "points", "edge_chi2", "edge_depth_positive")
_SCHUR_KERNELS = {"chunks": "lba_schur_chunks", "pairs": "lba_schur"}  # behind k_ (one window) and kb_ (batch)


def _fallback_windows():
    """the smallest shapes at which the vector Schur kernels can still go wrong"""
    base = synth.lba_window(4, n_free=3, n_fixed=2, n_points=50)
    return [synth.lba_window(2, n_free=3, n_fixed=1, n_points=80, mono_frac=1.0),  # 6 pose pairs: one partial tile; 2 chunks of kSchurPts = 64
            synth.lba_window(34, n_free=24, n_fixed=2, n_points=300),  # 300 pose pairs > kMk = 256: two pair tiles; 5 chunks, the last partial
            _with_second_camera_edges(synth.lba_window(12, n_free=6, n_fixed=2, n_points=300), 12),  # several edges a (pose, point): e_dup
            dict(base, pose_fixed=np.ones_like(base["pose_fixed"]))]  # n_free = 0: no Schur launch at all


def _collect_fallbacks(api):
    """every window alone and all of them in one batch, the blocks of the first, and which kernels were launched"""
    wins = _fallback_windows()
    api.profile_enable(True)
    opt = api.Optimizer(max_poses=32, max_points=512, max_edges=16384)
    bat = api.BatchOptimizer(max_windows=len(wins), max_poses=32, max_points=512, max_edges=16384)
    out = {}
    for tag, res in (("one", [opt.LocalBundleAdjustment(w) for w in wins]), ("bat", bat.LocalBundleAdjustment(wins))):
        for i, r in enumerate(res):
            for k in _SOLVED:
                out[f"{tag}{i}/{k}"] = r[k]
            out[f"{tag}{i}/stats"] = np.array([r["iterations_run"], r["final_chi2"], r["final_lambda"]], np.float64)
    for k, v in opt.linearize(wins[0]).items():
        out["lin/" + k] = np.asarray(v)
    out["launched"] = np.array(sorted(name for name, (_, n) in api.profile_report().items() if n > 0))
    return out


def _child(tmp_path, env_knob, value):
    out = str(tmp_path / f"{env_knob}_{value}.npz")
    env = dict(os.environ)
    env[env_knob] = value
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__), out], env=env, cwd=ROOT, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, (env_knob, value, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return dict(np.load(out))


def test_vector_schur_fallbacks_in_a_child_process(gpu_api, oracle, tmp_path):
    """GFS_LBA_SCHUR=chunks / pairs select the two vector Schur kernels (b_schur_chunks + b_schur_reduce, b_schur), which are also the
    fallbacks of windows too wide for the matrix-core kernel's partial blocks.  The knob is read once per process: each value runs
    _collect_fallbacks() in a fresh child (one at a time; a failing child fails the test and no further one starts).  Solutions and
    blocks are held to the oracle with the bars of test_solve_matches_oracle and test_linearize_blocks_match_oracle, and every batched
    window to the bits of the same window solved alone in that child.  No bit-equality with the default is claimed: the matrix-core
    kernel folds the sums in another order."""
    wins = _fallback_windows()
    solved = [oracle.lba_solve(w) for w in wins]
    Lo = oracle.lba_linearize(wins[0])
    for value in ("chunks", "pairs"):
        got = _child(tmp_path, "GFS_LBA_SCHUR", value)
        schur = sorted(n for n in got["launched"] if "lba_schur" in n and "reduce" not in n)
        assert schur == ["k_" + _SCHUR_KERNELS[value], "kb_" + _SCHUR_KERNELS[value]], (value, schur)
        for i, (w, ro) in enumerate(zip(wins, solved)):
            r = {k: got[f"one{i}/{k}"] for k in _SOLVED}
            its, final_chi2, _ = got[f"one{i}/stats"]
            assert its == ro["iterations_run"], (value, i)
            for j in range(w["n_poses"]):
                assert _rel(r["pose_q"][j], ro["pose_q"][j]) < 1e-5 and _rel(r["pose_t"][j], ro["pose_t"][j]) < 1e-5, (value, i, j)
            assert _rel(r["points"], ro["points"]) < 1e-5, (value, i)
            assert _rel(final_chi2, ro["final_chi2"]) < 1e-6, (value, i)
            thr = np.where(w["edge_stereo"] == 1, 7.815, 5.991)
            near = np.abs(ro["edge_chi2"] - thr) < 1e-4 * thr
            assert ((r["edge_chi2"] > thr) == (ro["edge_chi2"] > thr))[~near].all(), (value, i)
            assert (r["edge_depth_positive"] == ro["edge_depth_positive"]).all(), (value, i)
            for k in _SOLVED + ("stats",):
                assert np.array_equal(got[f"bat{i}/{k}"], got[f"one{i}/{k}"]), (value, i, k)
        for k in ("Hpp", "Hll", "Hpl", "bp", "bl", "edge_chi2"):
            assert _rel(got["lin/" + k], Lo[k]) < 1e-10, (value, k, _rel(got["lin/" + k], Lo[k]))
        assert abs(float(got["lin/chi2"]) - Lo["chi2"]) < 1e-9 * Lo["chi2"], value


if __name__ == "__main__":  # the child of test_vector_schur_fallbacks_in_a_child_process: _collect_fallbacks() under the inherited environment
    from geoflowslam_amd import api as A
    A.lib()
    assert A.device_count() >= 1
    np.savez(sys.argv[1], **_collect_fallbacks(A))
