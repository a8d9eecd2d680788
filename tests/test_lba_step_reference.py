"""CPU tests of the longdouble reference of the LBA linear step (tests/lba_step_support.py) and of its bars, before they are applied
to the kernels (tests/test_gpu_lba_step.py):

 1. the reference is validated WITHOUT Schur elimination: the full (6F + 3N) damped normal matrix of two small windows, assembled
    densely in longdouble and solved, gives the xp, xl of schur_ref + solve + backsub_ref to 1e-15 relative where longdouble can
    resolve that (see the test), and to kappa * 2^-63 at the LM loop's own first damping;
 2. the bars can be met: a straightforward float64 restatement of the three stages (per-landmark loops, numpy.linalg.inv per 3 x 3,
    numpy.linalg.solve) passes every bar on every shape of the GPU case list;
 3. the bars notice a subtly wrong step: the same restatement with one seeded defect fails them, in the stage that has the defect.
"""
import numpy as np
import pytest

import lba_step_support as S

if not S.LONGDOUBLE_OK:
    pytest.skip("np.longdouble is not wider than float64 on this machine", allow_module_level=True)

LD = S.LD


def restated_step(blocks, st, defect=None):
    """The linear step in float64, the plain way.  defect: None, or one of
       drop       one landmark left out of one pose pair's sum
       transpose  one off-diagonal 6 x 6 block transposed
       lambda     lambda left off one diagonal entry
       chunk      the last staged landmark of a chunk of 64 counted twice
       swap       xp of two poses swapped"""
    F, N, n = st["F"], st["N"], 6 * st["F"]
    B = S.fold_blocks(blocks["Hpl"], st)
    lam = S.lambda_ref(blocks["Hpp"], blocks["Hll"])
    Hll, bl, bp = np.asarray(blocks["Hll"]), np.asarray(blocks["bl"]), np.asarray(blocks["bp"])
    Dinv = np.array([np.linalg.inv(Hll[l] + lam * np.eye(3)) for l in range(N)]).reshape(N, 3, 3)
    Dinv = (Dinv + Dinv.transpose(0, 2, 1)) / 2  # (the packed form holds one triangle)
    Hs, bs = np.zeros((n, n)), bp.ravel().copy()
    for f in range(F):
        Hs[6 * f:6 * f + 6, 6 * f:6 * f + 6] = blocks["Hpp"][f] + lam * np.eye(6)
    pair = None
    if defect in ("drop", "transpose", "swap"):  # the first two poses that share most landmarks
        sh = st["shared"] - np.diag(np.diag(st["shared"]))
        i, j = np.unravel_index(np.argmax(np.tril(sh)), sh.shape)
        pair = (int(i), int(j), int(np.nonzero(st["seen"][i] & st["seen"][j])[0][-1]))
        assert sh[i, j] > 0
    staged = np.nonzero(st["seen"][:, :S.K_SCHUR_CHUNK].any(0))[0]  # the first chunk's landmarks that a free pose sees
    twice = int(staged[-1]) if len(staged) else -1
    for l in range(N):
        idx = np.nonzero(st["seen"][:, l])[0]
        for rep in range(2 if defect == "chunk" and l == twice else 1):
            for i in idx:
                BD = B[i, l] @ Dinv[l]
                bs[6 * i:6 * i + 6] -= BD @ bl[l]
                for j in idx:
                    if defect == "drop" and (i, j, l) == pair:
                        continue
                    Hs[6 * i:6 * i + 6, 6 * j:6 * j + 6] -= BD @ B[j, l].T
    if defect == "transpose":
        i, j, _ = pair
        Hs[6 * i:6 * i + 6, 6 * j:6 * j + 6] = Hs[6 * i:6 * i + 6, 6 * j:6 * j + 6].T.copy()
    if defect == "lambda":
        Hs[n // 2, n // 2] -= lam
    Hs = S.unpack_lower(S.pack_lower(Hs), n)  # what the packed lower triangle holds
    xp = np.linalg.solve(Hs, bs) if n else np.zeros(0)
    if defect == "swap":
        i, j, _ = pair
        xp = xp.copy()
        xp[6 * i:6 * i + 6], xp[6 * j:6 * j + 6] = xp[6 * j:6 * j + 6].copy(), xp[6 * i:6 * i + 6].copy()
    xl = np.zeros((N, 3))
    for l in range(N):
        c = bl[l].copy()
        for f in np.nonzero(st["seen"][:, l])[0]:
            c -= B[f, l].T @ xp[6 * f:6 * f + 6]
        xl[l] = Dinv[l] @ c
    scale = float((xp * (lam * xp + bp.ravel())).sum() + (xl * (lam * xl + bl)).sum())
    return dict(lam=lam, Dinv=S.sym33_to_6(Dinv), Hs=S.pack_lower(Hs), bs=bs, xp=xp, xl=xl, scale=scale)


@pytest.mark.parametrize("name", ["F2-fixed2-N20", "second-camera-F6"])
@pytest.mark.parametrize("damping", [1024, 1])
def test_reference_agrees_with_the_dense_system(oracle, name, damping):
    """Schur elimination + reduced solve + back-substitution of the reference against the full damped normal equations solved at once:
    1e-15 relative.  Longdouble resolves that only where kappa * 2^-64 is well below it.  With the LM loop's own first damping
    (tau = 1e-5: kappa ~ 1e5 by construction, every window) the two routes differ by the amplified roundings of their longdouble
    inputs, measured 2e-16 ... 3e-15 on small windows: the 1e-15 is asserted at 1024 x that damping (kappa ~ 1e2, the same
    algebra: blocks, signs, transposes, folding of duplicate edges), and at the loop's own damping the bar is what the number
    format allows, max(1e-15, kappa_inf(H) * 2^-63)."""
    w = S.case(name)
    st, L = S.structure(w), oracle.lba_linearize(w)
    F, N, n = st["F"], st["N"], 6 * st["F"]
    B = S.fold_blocks(L["Hpl"], st)
    lam = damping * S.lambda_ref(L["Hpp"], L["Hll"])
    H, b = np.zeros((n + 3 * N, n + 3 * N), LD), np.concatenate([np.asarray(L["bp"], LD).ravel(), np.asarray(L["bl"], LD).ravel()])
    for f in range(F):
        H[6 * f:6 * f + 6, 6 * f:6 * f + 6] = L["Hpp"][f]
        for l in range(N):
            H[6 * f:6 * f + 6, n + 3 * l:n + 3 * l + 3] = B[f, l]
            H[n + 3 * l:n + 3 * l + 3, 6 * f:6 * f + 6] = B[f, l].T
    for l in range(N):
        H[n + 3 * l:n + 3 * l + 3, n + 3 * l:n + 3 * l + 3] = L["Hll"][l]
    H += LD(lam) * np.eye(n + 3 * N, dtype=LD)
    X = S.solve_ld(H, np.concatenate([b[:, None], np.eye(len(b), dtype=LD)], 1))
    x, kappa = X[:, 0], np.abs(H).sum(1).max() * np.abs(X[:, 1:]).sum(1).max()
    Dinv, _ = S.dinv_ref(L["Hll"], lam)
    Hs, _, bs, _ = S.schur_ref(L["Hpp"], B, Dinv, L["bp"], L["bl"], lam, st)
    xp = S.solve_ld(Hs, bs)[:, 0]
    xl, _ = S.backsub_ref(Dinv, L["bl"], B, xp, st)
    ep = np.abs(xp - x[:n]).max() / np.abs(x[:n]).max()
    el = np.abs(xl.ravel() - x[n:]).max() / np.abs(x[n:]).max()
    bar = 1e-15 if damping > 1 else max(1e-15, float(kappa) * 2.0 ** -63)
    print(f"{name} damping x{damping}: kappa_inf {float(kappa):.2e}, dense against eliminated: xp {float(ep):.2e} xl {float(el):.2e} (bar {bar:.2e})")
    assert kappa * 2.0 ** -63 < 1e-16 or damping == 1
    assert ep <= bar and el <= bar, (float(ep), float(el), bar)


def _fmt(figs):
    return " ".join(f"{k}={v:.3g}/{a:.3g}" for k, (v, a) in figs.items())


@pytest.mark.parametrize("name", [n for n, _ in S.CASES + S.KNOB_CASES[len(S.STRUCTURE_CASES):]])
def test_a_plain_float64_step_meets_every_bar(oracle, name):
    w = S.case(name)
    st, L = S.structure(w), oracle.lba_linearize(w)
    figs, failed = S.check_step(L, st, restated_step(L, st))
    print(name, _fmt(figs))
    assert not failed, (failed, _fmt(figs))


_STAGE_OF = {"drop": ["Hs"], "transpose": ["Hs"], "lambda": ["Hs"], "chunk": ["Hs", "bs"], "swap": ["eta", "xp"]}


@pytest.mark.parametrize("name", ["F22-fixed2-N65", "F3-fixed2-N129", "single-mono-landmark-F6"])
@pytest.mark.parametrize("defect", sorted(_STAGE_OF))
def test_a_seeded_defect_fails_the_bars(oracle, name, defect):
    """... and only in the stage that has it: every stage is fed the inputs the step under test had"""
    w = S.case(name)
    st, L = S.structure(w), oracle.lba_linearize(w)
    figs, failed = S.check_step(L, st, restated_step(L, st, defect))
    print(name, defect, _fmt(figs))
    assert failed == [k for k in figs if k in _STAGE_OF[defect]], (defect, failed, _fmt(figs))


def test_most_first_trials_are_accepted(oracle):
    """the tie between the hook and gfs_lba_solve (tests/test_gpu_lba_step.py) is conditional on the first trial being accepted: that is the rule"""
    taken = [oracle.lba_solve_scripted(dict(S.case(n), iterations=1))[1]["accepted"][0] == 1 for n, _ in S.CASES]
    assert sum(taken) >= 0.9 * len(taken), sum(taken)


def test_window_edits_do_what_they_say():
    w, p = S.isolated_pose(S.window(6, 2, 40, 306))
    st = S.structure(w)
    f = st["free_index"][p]
    assert st["shared"][f, f] >= 2 and st["shared"][f].sum() == st["shared"][f, f]
    w, l = S.landmark_of_fixed_poses_only(S.window(6, 2, 40, 306))
    assert not S.structure(w)["seen"][:, l].any() and (w["edge_point"] == l).any()
    w, l = S.single_mono_landmark(S.window(6, 2, 40, 306))
    e = np.nonzero(w["edge_point"] == l)[0]
    assert len(e) == 1 and w["edge_stereo"][e[0]] == 0 and S.structure(w)["seen"][:, l].sum() == 1
    assert S.structure(S.all_poses_fixed(S.window(6, 2, 40, 306)))["F"] == 0
    w = S.with_second_camera_edges(S.window(6, 2, 40, 306), 306)
    pairs = np.stack([w["edge_pose"], w["edge_point"]], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs)
    for F in (1, 22, 43):
        for n_fixed in (0, 2):
            assert S.structure(S.window(F, n_fixed, 20, 1))["F"] == F
