"""The rule of Sim3Solver (geoflowslam_amd/csrc/sim3_ransac_rule.hpp, through tests/host/sim3_ransac_restatement.cpp) against
independent statements in Python: ComputeSim3 against a numpy transcription (numpy.linalg.eigh, Rodrigues through the reference's
angle-axis route), SetRansacParameters against a direct evaluation, the sampling against a list doing the swap-with-back, the pick
against a loop written the reference's way."""
import numpy as np
import pytest

import sim3_ransac_support as S
from geoflowslam_amd import api, synth

f32, f64 = np.float32, np.float64
ULP1 = 2.0 ** -23  # one float ulp of 1.0
MIN_GAP = 1e-6     # triples whose two largest eigenvalues of N are closer than this (relative) are left out


def triples(seed, count):
    """Random non-collinear triples in camera 2's frustum and their images under a random Sim3 with a little noise -> (P1, P2)
    [count, 3 points, 3].  A triple whose second singular value is under 5 % of its first is drawn again: three points are always
    coplanar, the two largest eigenvalues of N are then s1^2 + s2^2 and s1^2 - s2^2, so the relative gap is at least 2 * 0.05^2."""
    rng = np.random.default_rng(seed)
    P1, P2 = [], []
    while len(P1) < count:
        z = rng.uniform(1.0, 6.0, 3)
        x2 = np.stack([rng.uniform(-0.5, 0.5, 3) * z, rng.uniform(-0.4, 0.4, 3) * z, z], 1)
        sv = np.linalg.svd(x2 - x2.mean(0), compute_uv=False)
        if sv[1] < 0.05 * sv[0]:
            continue
        R = synth._rot(*(np.deg2rad(170.0) * rng.uniform(-1, 1, 3)))
        x1 = rng.uniform(0.5, 2.0) * x2 @ R.T + rng.uniform(-1, 1, 3) + 0.01 * rng.normal(size=(3, 3))
        P1.append(x1.astype(f32))
        P2.append(x2.astype(f32))
    return np.array(P1), np.array(P2)


def transcription(P1, P2, fix_scale, tail=f64):
    """ComputeSim3 (reference src/Sim3Solver.cc:289-392) in numpy.  Steps 1-3 are float in the source and are float32 here, every
    operation written out elementwise so that it is rounded once (rule C's order); the eigenvector, the angle-axis vector and the
    Rodrigues formula, which the source leaves to Eigen and Sophus, are float64.  Steps 5-7 run in `tail`: float64, or float32 as the
    source has them (R rounded to float first) for the float-versus-float64 spread.  -> R [3, 3], t [3], s, relative eigenvalue gap."""
    A, B = P1.astype(f32).T, P2.astype(f32).T  # columns are points
    O1 = ((A[:, 0] + A[:, 1]) + A[:, 2]) / f32(3)
    O2 = ((B[:, 0] + B[:, 1]) + B[:, 2]) / f32(3)
    Pr1, Pr2 = A - O1[:, None], B - O2[:, None]
    M = np.zeros((3, 3), f32)
    for i in range(3):
        for j in range(3):
            M[i, j] = (Pr2[i, 0] * Pr1[j, 0] + Pr2[i, 1] * Pr1[j, 1]) + Pr2[i, 2] * Pr1[j, 2]
    N11, N12, N13, N14 = (M[0, 0] + M[1, 1]) + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]
    N22, N23, N24 = (M[0, 0] - M[1, 1]) - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]
    N33, N34, N44 = (-M[0, 0] + M[1, 1]) - M[2, 2], M[1, 2] + M[2, 1], (-M[0, 0] - M[1, 1]) + M[2, 2]
    N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]], f32).astype(f64)
    lam, vec = np.linalg.eigh(N)
    q = vec[:, 3]
    gap = (lam[3] - lam[2]) / np.abs(lam).max()
    v = q[1:4]
    ang = np.arctan2(np.linalg.norm(v), q[0])
    w = 2 * ang * v / np.linalg.norm(v)  # angle-axis; the quaternion's angle is the half
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    Rt = R.astype(f32).astype(tail) if tail is f32 else R
    Pr1t, Pr2t, O1t, O2t = Pr1.astype(tail), Pr2.astype(tail), O1.astype(tail), O2.astype(tail)
    P3 = np.array([[(Rt[r, 0] * Pr2t[0, c] + Rt[r, 1] * Pr2t[1, c]) + Rt[r, 2] * Pr2t[2, c] for c in range(3)] for r in range(3)], tail)
    s = tail(1)
    if not fix_scale:
        nom = den = None
        for c in range(3):
            for r in range(3):
                a, b = Pr1t[r, c] * P3[r, c], P3[r, c] * P3[r, c]
                nom, den = (a, b) if nom is None else (nom + a, den + b)
        s = tail(f64(nom) / f64(den))
    sR = s * Rt
    t = np.array([O1t[r] - ((sR[r, 0] * O2t[0] + sR[r, 1] * O2t[1]) + sR[r, 2] * O2t[2]) for r in range(3)], tail)
    return R, t.astype(f64), f64(s), gap, float(np.abs(O1).max())


@pytest.fixture(scope="module")
def compared():
    P1, P2 = triples(1, 2000)
    rows = []
    for a, b in zip(P1, P2):
        for fix in (False, True):
            R64, t64, s64, gap, scale = transcription(a, b, fix, f64)
            _, t32, s32, _, _ = transcription(a, b, fix, f32)
            R, t, s, T12, T21 = S.compute_sim3(a, b, fix)
            rows.append(dict(gap=gap, dR=np.abs(R.astype(f64) - R64).max(), ds=abs(f64(s) - s64) / s64, ds_spread=abs(s32 - s64) / s64,
                             dt=np.abs(t.astype(f64) - t64).max() / scale, dt_spread=np.abs(t32 - t64).max() / scale, R=R, t=t, s=s, T12=T12,
                             T21=T21, fix=fix))
    return rows


def test_rotation_within_one_ulp(compared):
    """R12 entry by entry against the float64 transcription: one float ulp of 1.0.  The rule's double result and the transcription's
    differ by about 1e-16 / gap, far less than an ulp, so after the one rounding to float the two can only land on the same or on
    neighbouring floats.  Measured on these 4 000 solves: largest difference 2.98e-08 (a quarter of that ulp), smallest relative gap 4.4e-03, none left out."""
    kept = [r for r in compared if r["gap"] >= MIN_GAP]
    assert 1 - len(kept) / len(compared) < 0.01
    worst = max(r["dR"] for r in kept)
    print(f"largest |R12 - R64| = {worst:.3g}, smallest gap = {min(r['gap'] for r in compared):.3g}, left out {len(compared) - len(kept)}")
    assert worst <= ULP1


def test_scale_and_translation_within_the_float_spread(compared):
    """s12 and t12 against the float64 transcription.  The bar is measured, not chosen: the largest difference between the
    transcription run with its steps 5-7 in float (as the source has them) and in float64 on the same triples, times 4 for the
    different summation order.  s12 relative to itself, t12's largest component difference relative to the largest coordinate of
    the centroid O1 (t12 = O1 - s R O2 cancels, so its own size is no measure of its rounding).  Measured on these 4 000 solves:
    spread 2.72e-07 (s12) and 3.47e-07 (t12); the rule's largest differences 2.72e-07 and 3.47e-07, the same
    figures: behind R12 the rule is the source's float arithmetic."""
    kept = [r for r in compared if r["gap"] >= MIN_GAP]
    bar_s, bar_t = 4 * max(r["ds_spread"] for r in kept), 4 * max(r["dt_spread"] for r in kept)
    worst_s, worst_t = max(r["ds"] for r in kept), max(r["dt"] for r in kept)
    print(f"spread s12 {bar_s / 4:.3g} t12 {bar_t / 4:.3g}; rule s12 {worst_s:.3g} t12 {worst_t:.3g}")
    assert 0 < bar_s < 1e-5 and 0 < bar_t < 1e-5  # the spread itself is a float rounding, not a blunder of the transcription
    assert worst_s <= bar_s and worst_t <= bar_t
    assert all(r["s"] == 1.0 for r in kept if r["fix"])


def test_transforms_are_built_from_the_parts(compared):
    """mT12i = [s R | t] and mT21i = [(1 / s) R^T | -sRinv t] with the products the header states: float, the double scalar 1.0 / s
    rounded to float once."""
    for r in compared[:200]:
        R, t, s = r["R"], r["t"], f32(r["s"])
        assert r["T12"][:, :3].tobytes() == (s * R).astype(f32).tobytes() and r["T12"][:, 3].tobytes() == t.tobytes()
        inv = f32(f64(1.0) / f64(s))
        sRinv = (inv * R.T).astype(f32)
        assert r["T21"][:, :3].tobytes() == sRinv.tobytes()
        tinv = np.array([((-sRinv[k, 0]) * t[0] + (-sRinv[k, 1]) * t[1]) + (-sRinv[k, 2]) * t[2] for k in range(3)], f32)
        assert r["T21"][:, 3].tobytes() == tinv.tobytes()


def test_identity_and_sign_cases():
    """Identical clouds: the quaternion is (1, 0, 0, 0), where the reference takes its vec.norm() == 0 branch; the rule gives the
    identity matrix exactly.  A half turn (w == 0) is a rotation matrix too."""
    P = triples(2, 1)[1][0]
    R, t, s, _, _ = S.compute_sim3(P, P, True)
    assert R.tobytes() == np.eye(3, dtype=f32).tobytes() and s == 1.0 and np.abs(t).max() < 1e-6
    half = (P.astype(f64) @ np.diag([1.0, -1.0, -1.0])).astype(f32)
    R, t, s, _, _ = S.compute_sim3(half, P, True)
    assert np.abs(R.astype(f64) - np.diag([1.0, -1.0, -1.0])).max() < 1e-6


def test_set_ransac_parameters():
    L = S.restatement()
    for n in list(range(0, 45)) + [100, 150, 400, 2000, 100000]:
        for m in (0, 1, 3, 6, 15, 20, 40, 150):
            for p, mx in ((0.99, 300), (0.999, 300), (0.5, 10), (0.99, 5)):
                assert L.s3rr_iterations(n, p, m, mx) == synth.sim3_ransac_iterations(n, p, m, mx), (n, m, p, mx)
    assert L.s3rr_iterations(15, 0.99, 15, 300) == 1 and L.s3rr_iterations(10, 0.99, 15, 300) == 1  # N == minInliers; N < minInliers
    assert L.s3rr_iterations(20, 0.99, 15, 300) == 9 and L.s3rr_iterations(150, 0.99, 15, 300) == 300


def test_sampling_against_a_list():
    rng = np.random.default_rng(3)
    cases = [(n, r0, r1, r2) for n in (3, 4, 5) for r0 in range(n) for r1 in range(n - 1) for r2 in range(n - 2)]
    for _ in range(2000):
        n = int(rng.integers(3, 500))
        cases.append((n, *(int(rng.integers(0, n - k)) for k in range(3))))
    for n, *r in cases:
        avail, want = list(range(n)), []
        for randi in r:
            want.append(avail[randi])
            avail[randi] = avail[-1]
            avail.pop()
        assert S.resolve_draws(n, r) == want and len(set(want)) == 3, (n, r)
        assert S.draws_for(n, want) == r  # the support's inverse, which the hand-built cases rely on


def test_pick_against_the_sequential_loop():
    rng = np.random.default_rng(4)
    for _ in range(3000):
        H = int(rng.integers(1, 40))
        counts = rng.integers(0, int(rng.integers(1, 12)), H).astype(np.int32)
        m = int(rng.integers(0, 12))
        best, best_i, out = 0, None, None  # mnBestInliers = 0 (:39)
        for i, c in enumerate(counts):
            if c >= best:
                best, best_i = c, i
                if c > m:
                    out = (i, i + 1, api.SIM3_RANSAC_CONVERGED)
                    break
        if out is None:
            out = (best_i, H, api.SIM3_RANSAC_NO_MORE)
        assert S.pick(counts, m) == out, (counts, m)


def test_restatement_without_its_early_stop_returns_the_same():
    for k in range(40):
        p = synth.sim3_ransac_problem(300 + k, n_pairs=30 + 5 * k, inlier_share=0.1 + 0.02 * k, fix_scale=bool(k & 1), max_iterations=40)
        a, b = S.run(p, True), S.run(p, False)
        assert S.solution_bytes(a) == S.solution_bytes(b)
        pk = S.pick(b["counts"], p["min_inliers"])
        assert (pk[1], pk[2]) == (a["iterations"], a["status"]) and b["counts"][pk[0]] == a["n_inliers"]


def test_restatement_under_the_sanitizers():
    """The restatement and the rule header as a program of their own under -fsanitize=address,undefined (plain g++, CPU only, never
    loaded into python): no report, and the same sums as the unsanitized build of the same program."""
    import os
    import subprocess
    main = os.path.join(S.ROOT, "tests", "host", "sim3_ransac_restatement_main.cpp")
    outs = []
    for exe, flags in ((os.path.join(S.ROOT, "tests", "host", "_sim3_ransac_restatement_asan"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]),
                       (os.path.join(S.ROOT, "tests", "host", "_sim3_ransac_restatement_plain"), [])):
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", *flags, "-o", exe, main], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "" and r.stdout.endswith("sim3_ransac_restatement_main: ok\n"), r.stderr[-2000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1] and outs[0].count("\n") > 40
