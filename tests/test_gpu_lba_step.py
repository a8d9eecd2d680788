"""GPU tests of the linear step of the local bundle adjustment, stage by stage (MI355X): lambda, Dinv, the reduced system Hs / bs as the
Schur stage leaves it, the pose step xp, the landmark step xl and the computeScale sum of the FIRST Levenberg-Marquardt trial, taken
through the product's own dispatch by gfs_test_lba_first_trial (include/gfs_abi_test.h), against the longdouble reference and the
derived bars of tests/lba_step_support.py (validated on the CPU by tests/test_lba_step_reference.py).  The loop around the step hides
a subtly wrong step -- it still descends to the same minimum -- so the converged results of tests/test_gpu_lba.py do not see it.

The shapes are the smallest at which each path can go wrong: free poses around one | two 128 x 128 blocks of the matrix-core Schur
kernel (21 | 22), the LDS | HBM factorisation (30 | 31), two | three block rows (42 | 43); landmarks around the 8 staged at a time and
the chunk of 64; and the structure cases (an isolated pose, a landmark of fixed poses only, a single monocular observation, all-mono,
second-camera duplicate edges, shuffled edges, every pose fixed).  The two vector Schur kernels (GFS_LBA_SCHUR = chunks | pairs, read
once per process) run the structure cases and F = 2, 22, 31 in a fresh child each."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lba_step_support as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not S.LONGDOUBLE_OK:
    pytest.skip("np.longdouble is not wider than float64 on this machine", allow_module_level=True)

_CAP = dict(max_poses=48, max_points=256, max_edges=16384)
_FILL = -7.25e301  # pre-written into the hook's arrays: no step holds it
_TRIAL_KEYS = ("Dinv", "Hs", "bs", "xp", "xl")
_BLOCK_KEYS = ("Hpp", "Hll", "Hpl", "bp", "bl")


@pytest.fixture(scope="module")
def opt(gpu_api):
    o = gpu_api.Optimizer(**_CAP)
    yield o
    o.close()


def _fmt(figs):
    return " ".join(f"{k}={v:.3g}/{a:.3g}" for k, (v, a) in figs.items())


def _check(name, w, L, T):
    """every assertion on one observed step"""
    st = S.structure(w)
    for k in _TRIAL_KEYS:
        assert not (T[k] == _FILL).any(), (name, k, "entries not delivered", int((T[k] == _FILL).sum()))
        assert np.isfinite(T[k]).all(), (name, k)
    assert T["solve_ok"] == 1, name
    figs, failed = S.check_step(L, st, T)
    print(f"{name}: F={st['F']} N={st['N']} {_fmt(figs)}")
    assert not failed, (name, failed, _fmt(figs))
    assert not S.unshared_blocks_are_zero(T["Hs"], st), (name, "a pose pair without a common landmark has a non-zero block")
    return st, figs


@pytest.mark.parametrize("name", [n for n, _ in S.CASES])
def test_first_trial_stage_by_stage(gpu_api, oracle, opt, name):
    w = S.case(name)
    L = opt.linearize(w)
    T = gpu_api.lba_first_trial(opt, w, fill=_FILL)
    st, _ = _check(name, w, L, T)
    if "isolated-pose" in name:
        assert (st["shared"] - np.diag(np.diag(st["shared"])) == 0).all(1).any()
    if "fixed-only-landmark" in name:
        _, l = S.landmark_of_fixed_poses_only(S.window(st["F"], 2, 40, 300 + st["F"]))
        assert not st["seen"][:, l].any()
    # ---- the hook observes the path the product runs: the same window solved with one iteration
    w1 = dict(w, iterations=1)
    r = opt.LocalBundleAdjustment(w1)
    _, trace = oracle.lba_solve_scripted(w1)
    if r["final_chi2"] < L["chi2"] and trace["accepted"][0] == 1:  # the first trial was taken
        assert np.array_equal(r["points"], w["points"] + T["xl"]), name
        d = S.oplus_mismatch(w, T["xp"], r, st, oracle.se3_exp)
        assert d <= 1e-14, (name, d)
        fixed = w["pose_fixed"] != 0
        assert np.array_equal(r["pose_t"][fixed], w["pose_t"][fixed]), name
    else:
        print(f"{name}: the first trial was not accepted (chi2 {L['chi2']:.6g} -> {r['final_chi2']:.6g}, oracle {trace['accepted'][:3]})")
    # the hook leaves the handle as a solve leaves it
    assert np.array_equal(opt.LocalBundleAdjustment(w1)["points"], r["points"])


def test_default_schur_kernel_is_the_matrix_core_one(gpu_api):
    gpu_api.profile_enable(True)
    gpu_api.profile_reset()
    try:
        o = gpu_api.Optimizer(**_CAP)
        gpu_api.lba_first_trial(o, S.case("F22-fixed2-N65"))
        launched = {n for n, (_, c) in gpu_api.profile_report().items() if c > 0}
        o.close()
    finally:
        gpu_api.profile_enable(False)
    assert "k_lba_schur_mfma" in launched and "k_lba_solve" in launched and "k_lba_update" in launched, launched
    assert not {"k_lba_schur", "k_lba_schur_chunks", "k_lba_decide"} & launched, launched


def test_refusals_leave_the_handle_usable(gpu_api, opt):
    import ctypes as C
    w = S.case("F3-fixed2-N9")
    before = opt.LocalBundleAdjustment(w)
    P, keep = gpu_api._lba_problem(w)
    arrays = {k: np.zeros(4096) for k in _TRIAL_KEYS}

    def trial(without=None):
        T = gpu_api.LbaTrial()
        for k, v in arrays.items():
            setattr(T, k, None if k == without else v.ctypes.data)
        return T

    f = gpu_api.lib().gfs_test_lba_first_trial
    assert f(None, C.byref(P), C.byref(trial())) == -1      # GFS_ERR_INVALID_ARG
    assert f(opt.h, None, C.byref(trial())) == -1
    assert f(opt.h, C.byref(P), None) == -1
    for k in _TRIAL_KEYS:
        assert f(opt.h, C.byref(P), C.byref(trial(without=k))) == -1, k
    assert f(opt.h, C.byref(P), C.byref(trial())) == 0
    after = opt.LocalBundleAdjustment(w)
    for k in ("pose_q", "pose_t", "points", "edge_chi2"):
        assert np.array_equal(after[k], before[k]), k
    assert after["iterations_run"] == before["iterations_run"] and after["final_chi2"] == before["final_chi2"]


# ---- the two vector Schur kernels, each in a fresh child process ----------------------------------------------------------------
_SCHUR_KERNELS = {"chunks": "k_lba_schur_chunks", "pairs": "k_lba_schur"}


def _collect(api):
    """linearize() and the first trial of every knob case, and which kernels were launched"""
    api.profile_enable(True)
    o = api.Optimizer(**_CAP)
    out = {}
    for name, make in S.KNOB_CASES:
        w = make()
        L, T = o.linearize(w), api.lba_first_trial(o, w, fill=_FILL)
        for k in _BLOCK_KEYS:
            out[f"{name}/{k}"] = L[k]
        for k in _TRIAL_KEYS:
            out[f"{name}/{k}"] = T[k]
        out[f"{name}/scalars"] = np.array([T["lam"], T["scale"], T["solve_ok"]], np.float64)
    out["launched"] = np.array(sorted(n for n, (_, c) in api.profile_report().items() if c > 0))
    return out


def _child(tmp_path, value):
    out = str(tmp_path / f"step_{value}.npz")
    env = dict(os.environ)
    env["GFS_LBA_SCHUR"] = value
    env["PYTHONPATH"] = os.pathsep.join([ROOT] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__), out], env=env, cwd=ROOT, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, (value, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return dict(np.load(out))


def test_vector_schur_kernels_stage_by_stage_in_a_child_process(gpu_api, tmp_path):
    """one child at a time; a failing child fails the test and no further one starts"""
    for value in ("chunks", "pairs"):
        got = _child(tmp_path, value)
        schur = sorted(n for n in got["launched"] if "lba_schur" in n and "reduce" not in n)
        assert schur == [_SCHUR_KERNELS[value]], (value, schur)
        for name, make in S.KNOB_CASES:
            lam, scale, ok = got[f"{name}/scalars"]
            T = dict({k: got[f"{name}/{k}"] for k in _TRIAL_KEYS}, lam=lam, scale=scale, solve_ok=int(ok))
            _check(f"{value}:{name}", make(), {k: got[f"{name}/{k}"] for k in _BLOCK_KEYS}, T)


if __name__ == "__main__":  # the child: _collect() under the inherited environment
    from geoflowslam_amd import api as A
    A.lib()
    assert A.device_count() >= 1
    np.savez(sys.argv[1], **_collect(A))
