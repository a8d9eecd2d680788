"""k_pose_opt (gfs_pose_optimize, both sum modes) against the independent longdouble reference of tests/pose_step_support.py -- after
one, two and three LM iterations, where a wrong Jacobian term, Huber weight, lambda0 or exp-map shows at 1e-3 and the bar is 1e-14
-- and on the paths no other test reaches: frames of 255 ... 13 879 edges (the register / global edge split at 256 and 512 a thread's
edges, the second pass of the chi2 slab above 6 939 and of the classification sum above 13 878), a handle used for a small frame
after a large one, and degenerate and non-finite inputs.

The bars are derived per case by the support module (16 x the reference's own float64 spread, floored at 64 * 2^-52 * ||pose||; every
edge's chi2 through its own Jacobian) and the cases are admitted by the reference alone (tests/test_pose_step_reference.py).

Measured on an MI355X (max |[R | t] - reference| over the cases; the worst fraction of a case's bar; the worst edge's chi2 as a
fraction of its bar; the bars are those of tests/test_pose_step_reference.py: 2.5e-14 ... 9.6e-13 for its <= 3, ... 2.8e-11 for 4 x 10):
                   its = 1, 2, 3 (19 cases x 3)                          4 x 10 (25 cases)
  edge order       5.9e-14 (seed20), 0.11 bar, chi2 0.010, median 2e-16   1.0e-14 (far_start, bar 1.7e-13), 0.06 bar, chi2 0.003
  tree             8.1e-15 (seed20), 0.04 bar, chi2 0.004, median 1e-16   1.5e-13 (seed13, bar 2.8e-11), 0.02 bar, chi2 0.002
  integers         equal in both modes                                    equal in both modes (no flipped flag, no iteration apart)
The edge-order figures are the restatement's (bit-equal to it on all 25 cases).  Seeded in scratch copies of the kernel, one at a
time, with these tests run against each (pose after ONE iteration on seed11): J[13]'s bf term with the other sign 4.7e-4, rho' left
out of b 2.7e-2, lambda0 = 1e-4 max |diag H| 3.6e-4 -- test_lm_steps red for its = 1, 2, 3 in both modes; b and c swapped in
pose_oplus_fast 2.3e-4 -- red in tree mode (edge-order mode does not call it); the chi2 slab of compute_active cut to one pass --
size6940 (and seed19, size13878, size13879; not size6939) red in test_full_schedule[edge_order] and in the bit-for-bit test.
The degenerate frames found one deviation, fixed in csrc/pose.hip: a mono point at camera z = 0 makes activeRobustChi2 = inf, an
unsolved trial (counted as DBL_MAX) is then "accepted", and the kernel took that DBL_MAX for the next iteration's chi2 instead of
computing it afresh as g2o does -- round 0 ended after 2 iterations instead of 10 (iterations_run 15 against 23).  With that fixed,
tree mode has the restatement's flags, n_inliers and iterations_run on all fourteen degenerate frames.
"""
import numpy as np
import pytest

import pose_step_support as S
from test_gpu_pose import _flips_are_proved_ties

pytestmark = pytest.mark.gpu

if not S.LONGDOUBLE_OK:
    pytest.skip("np.longdouble is not wider than float64 on this machine", allow_module_level=True)

MODES = ["edge_order", "tree"]
CASES = S.case_list()
SMALL = [c["name"] for c in CASES if c["small"]]
ALL = [c["name"] for c in CASES]
MAX_BATCH = 5


@pytest.fixture(scope="module")
def handle(gpu_api):
    made = {}

    def get(sums):
        if sums not in made:
            made[sums] = gpu_api.PoseOptimizer(max_obs=S.MAX_OBS, max_batch=MAX_BATCH, sums=sums)
        return made[sums]

    yield get
    for h in made.values():
        h.close()


def _run(po, names, its=None, n_rounds=None):
    """the cases in batches of five, in the order of `names` (case k at slot k % 5 of call k // 5: every slot of a batch is used)"""
    out = {}
    for i in range(0, len(names), MAX_BATCH):
        chunk = names[i:i + MAX_BATCH]
        for name, r in zip(chunk, po.PoseOptimization([S.scheduled(n, its, n_rounds) for n in chunk])):
            out[name] = r
    return out


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _same_bits(a, b, what=("q", "t", "chi2", "outlier")):
    """equal bits where finite, equal NaN masks (the payload of a NaN is nobody's contract)"""
    for k in what:
        x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
        nan = np.isnan(x)
        if not (np.array_equal(nan, np.isnan(y)) and np.array_equal(_bits(x)[~nan], _bits(y)[~nan])):
            return False
    fa, fb = np.float32(a["avg_reproj_error"]), np.float32(b["avg_reproj_error"])
    return bool((np.isnan(fa) and np.isnan(fb)) or fa.view(np.uint32) == fb.view(np.uint32)) and \
        all(a[k] == b[k] for k in ("n_inliers", "rounds_run", "iterations_run"))


def _against_reference(results, its, n_rounds, sums, full):
    """prints every case's figures, then asserts them"""
    rows, bad = [], []
    for name, r in results.items():
        R = S.ref(name, its, n_rounds)
        absolute, rel = S.bar(name, its, n_rounds)
        d, (ex, e) = S.pose_diff(r, R), S.chi2_excess(r, name, its, n_rounds)
        rows.append(f"  {name:10s} {sums:10s} its={its}: pose {d:.2e} = {d / absolute:.3f} bar ({absolute:.2e}), chi2 {ex:.3f} of its bar (edge {e}), "
                    f"iterations {r['iterations_run']} / {R['iterations_run']}, inliers {r['n_inliers']} / {R['n_inliers']}")
        ok = d <= absolute and ex <= 1.0 and r["rounds_run"] == R["rounds_run"]
        if full and sums == "tree":  # the rule of tests/test_gpu_pose.py for the tree sums at a converged state
            nflip = _flips_are_proved_ties(r, dict(outlier=R["outlier"], chi2=np.asarray(R["chi2"], np.float64)))
            ok = ok and abs(r["n_inliers"] - R["n_inliers"]) <= nflip and abs(r["iterations_run"] - R["iterations_run"]) <= 2
        else:
            ok = ok and np.array_equal(r["outlier"], R["outlier"]) and r["n_inliers"] == R["n_inliers"] and r["iterations_run"] == R["iterations_run"]
        if not ok:
            bad.append(rows[-1])
    print("\n".join(rows))
    assert not bad, "\n" + "\n".join(bad)


@pytest.mark.parametrize("its", [1, 2, 3])
@pytest.mark.parametrize("sums", MODES)
def test_lm_steps_match_the_reference(handle, sums, its):
    """One, two, three LM iterations of round 0 (n_rounds = 1) on the cases of up to 1 000 edges: pose and chi2 within the case's bar,
    iterations_run, outlier flags and n_inliers equal -- in tree mode too: no trial of these runs is decided by rounding (conditions()),
    and this is where pose_oplus_fast and ldlt6_solve_spd_fast work away from convergence (steps of 0.05 ... 0.2)."""
    _against_reference(_run(handle(sums), SMALL, its, 1), its, 1, sums, full=False)


@pytest.mark.parametrize("sums", MODES)
def test_full_schedule_matches_the_reference(handle, sums):
    """4 x 10 on every case, the eleven boundary sizes among them: both modes within the bar; the integers equal in edge-order mode, and
    under the proved-tie rule with |delta iterations| <= 2 in tree mode."""
    _against_reference(_run(handle(sums), ALL), None, None, sums, full=True)


def test_boundary_sizes_are_the_restatement_bit_for_bit(handle, oracle):
    """255 ... 13 879 edges in edge-order mode: q, t, chi2, flags, counts and avg are the sequential restatement's bits -- across the
    edges kept in registers and those in global memory, and across the second pass of either LDS slab."""
    names = [c["name"] for c in CASES if c["boundary"]]
    res = _run(handle("edge_order"), names)
    differ = [n for n in names if not _same_bits(res[n], oracle.pose_optimization(S.frame(n)))]
    assert not differ, differ


@pytest.mark.parametrize("sums", MODES)
def test_ragged_batch_of_boundary_sizes(handle, gpu_api, sums):
    """[13879, 2, 257, 0, 6940] in one call: each frame has the bits it has alone"""
    from geoflowslam_amd import synth
    empty = dict(synth.pose_frame(3, n_obs=0), xw=np.zeros((0, 3)), obs=np.zeros((0, 3)), inv_sigma2=np.zeros(0, np.float32),
                 stereo=np.zeros(0, np.uint8), n_obs=0)
    frames = [S.frame("size13879"), synth.pose_frame(102, n_obs=2), S.frame("size257"), empty, S.frame("size6940")]
    po = handle(sums)
    together = po.PoseOptimization(frames)
    for i, (p, r) in enumerate(zip(frames, together)):
        assert _same_bits(po.PoseOptimization(p), r), i
    assert together[1]["rounds_run"] == 0 and together[3]["rounds_run"] == 0 and together[0]["rounds_run"] == 4


@pytest.mark.parametrize("sums", MODES)
def test_handle_reuse_large_small_large(gpu_api, sums):
    """13 879 edges, then 600, then 13 879 again on one handle (err and level of the edges beyond a thread's second live in the handle
    across calls, at a stride that changes with the call): every result has the bits a fresh handle gives."""
    big, small = S.frame("size13879"), S.frame("seed17")
    assert small["n_obs"] == 600
    used = gpu_api.PoseOptimizer(max_obs=S.MAX_OBS, max_batch=1, sums=sums)
    seq = [used.PoseOptimization(p) for p in (big, small, big)]
    for p, r in zip((big, small, big), seq):
        fresh = gpu_api.PoseOptimizer(max_obs=S.MAX_OBS, max_batch=1, sums=sums)
        assert _same_bits(fresh.PoseOptimization(p), r), p["n_obs"]
        fresh.close()
    used.close()


DEGENERATE = S.degenerate_frames()


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_and_non_finite_inputs(handle, oracle, name):
    """A 60-edge frame with a NaN / inf observation, a NaN point, a point at camera z = 0 (off and on the axis), behind the camera, at
    z = 0.02, all-zero, 1e30 or infinite information, or all points coincident.  (The lambda loop runs at most 10 trials, the iteration
    loop at most `its` and the round loop at most n_rounds, whatever the numbers are: the calls return.)
    Edge-order mode is the restatement: integers equal, NaN masks equal, bits equal where finite.  Tree mode returns, and its integer
    outputs -- outlier flags, n_inliers, rounds_run, iterations_run -- are the restatement's, its NaN masks too."""
    p = DEGENERATE[name]
    ro = oracle.pose_optimization(p)
    r = handle("edge_order").PoseOptimization(p)
    print(f"  {name}: iterations {r['iterations_run']} / {ro['iterations_run']}, inliers {r['n_inliers']} / {ro['n_inliers']}, avg {r['avg_reproj_error']} / "
          f"{ro['avg_reproj_error']}, NaN chi2 {int(np.isnan(r['chi2']).sum())} / {int(np.isnan(ro['chi2']).sum())}, q {r['q']} / {ro['q']}")
    assert _same_bits(r, ro)
    rt = handle("tree").PoseOptimization(p)
    print(f"  {name} (tree): iterations {rt['iterations_run']}, inliers {rt['n_inliers']}, flags apart {int((rt['outlier'] != ro['outlier']).sum())}, "
          f"avg {rt['avg_reproj_error']}, q {rt['q']}")
    assert np.array_equal(rt["outlier"], ro["outlier"]) and rt["n_inliers"] == ro["n_inliers"]
    assert rt["rounds_run"] == ro["rounds_run"] and rt["iterations_run"] == ro["iterations_run"]
    assert np.array_equal(np.isnan(rt["chi2"]), np.isnan(ro["chi2"])) and np.isnan(rt["avg_reproj_error"]) == np.isnan(ro["avg_reproj_error"])
    assert np.array_equal(np.isnan(rt["q"]), np.isnan(ro["q"])) and np.array_equal(np.isnan(rt["t"]), np.isnan(ro["t"]))
