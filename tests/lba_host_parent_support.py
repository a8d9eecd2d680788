"""Every host path of gfs_lba_solve / _lidar / _batch / _linearize and gfs_gba_solve as SHA-256 digests: what
tools/record_lba_host_parent.py records into tests/golden/lba_host_parent_digest.json with the library of the commit before the host
code of lba.hip was restated once, and what tests/test_gpu_lba_host_parent.py compares the current library's bits with.

Each case sits at the smallest size at which its path differs.  A case's digest covers every output array, the three scalars and, where
they exist, the stop counters (gfs_test_lba_last_looks), pose_lidar_edges and all fields of gfs_gba_last_info.  The stop flag is
scripted (gfs_test_lba_stop_at_look); the number of looks of a case is the library's own count in the unstopped run.  Only the public
api and the windows and maps of the other support modules are used: the module imports at the recorded commit."""
import hashlib
import json
import os

import numpy as np

import gba_support as G
import lba_step_support as SS
import lba_stop_support as S
from geoflowslam_amd import synth

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lba_host_parent_digest.json")
LOCAL = ("s6_3x80", "s22_6x300_last", "s11_31x300_hbm")  # accepts and rejects; rejects with nothing queued ahead; k_lba_solve<false>
BATCH = ("s6_3x80", "s9_6x300_rrr", "s11_31x300_hbm")    # test_gpu_lba_stop.py::test_batch_closed_at_every_round's batch
LIDAR = dict(full=(dict(seed=8, n_free=3, n_fixed=1, n_points=80, n_cloud=200, voxel=0.15, lidar=(0, 1, 2)), None),
             rejecting=(dict(seed=3, n_free=3, n_fixed=1, n_points=80, n_cloud=200, voxel=0.15, lidar=(0, 1, 2)), (0, 5, 0.3)))
GBA_SMALLEST, GBA_TWO_PANELS = "mono-initial-map", "Fp+1-robust"
_CAP = dict(max_poses=48, max_points=4096, max_edges=65536)
_GCAP = dict(max_poses=48, max_points=512, max_edges=16384)
_SCALARS = ("iterations_run", "final_chi2", "final_lambda")
_FILL = -7.25e301


def _sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(p)
    return h.hexdigest()


def _arrays(d):
    """the bytes of every array of a result dict, by name, and of its scalars as float64"""
    out = []
    for k in sorted(d):
        v = d[k]
        out.append(k.encode())
        out.append(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else np.array([v], np.float64).tobytes())
    return out


def _digest(r, *counters):
    """r: a result dict, a list of them, or None (the entry check refused the call); counters: dicts of ints"""
    rs = r if isinstance(r, list) else [r]
    parts = []
    for x in rs:
        parts += [b"stopped before optimisation"] if x is None else _arrays(x)
    for c in counters:
        parts.append(json.dumps(c, sort_keys=True).encode())
    return _sha(*parts)


def lidar_window(which):
    cfg, pert = LIDAR[which]
    w = synth.lba_lidar_window(width=120, height=90, **cfg)
    return S.perturb(w, cfg["seed"], *pert) if pert else w


def batch_windows():
    return [S.window(n) for n in BATCH] + [synth.lba_window(0), dict(S.window("s6_3x80"), iterations=0)]


def _sweep(api, out, name, solve, first_look=0):
    """`name`: the unstopped run; `name@k`: the script armed at look k, for every look of the unstopped run from first_look on"""
    flag = np.zeros(1, np.int32)
    api.lba_stop_at_look(-1)
    r = solve(flag)
    L = api.lba_last_looks()
    out[name] = _digest(r, L)
    for look in range(first_look, L["looks"]):
        api.lba_stop_at_look(look)
        r = solve(flag)
        out[f"{name}@{look}"] = _digest(r, api.lba_last_looks())
    api.lba_stop_at_look(-1)
    return L["looks"]


def digests(api):
    """-> {case: sha256}"""
    out = {}
    Fp = api.gba_panel_rows() // 6
    opt = api.Optimizer(**_CAP)
    # ---- local: unstopped and stopped at every look
    for name in LOCAL:
        w = S.window(name)
        assert _sweep(api, out, f"local/{name}", lambda flag, w=w: opt.LocalBundleAdjustment(w, stop_flag=flag)) > 2
        out[f"local/{name}/no-flag"] = _digest(opt.LocalBundleAdjustment(w), api.lba_last_looks())
    # ---- local, no LM loop
    s6 = S.window("s6_3x80")
    out["local/iterations-0"] = _digest(opt.LocalBundleAdjustment(dict(s6, iterations=0)))
    out["local/no-free-pose"] = _digest(opt.LocalBundleAdjustment(SS.all_poses_fixed(s6)))
    # ---- mode 1 and the tap path
    out["linearize/s6_3x80"] = _digest(opt.linearize(s6))
    out["first-trial/s6_3x80"] = _digest(api.lba_first_trial(opt, s6, fill=_FILL))
    opt.close()
    # ---- lidar
    for which in LIDAR:
        w = lidar_window(which)
        m = api.LidarMap(max_points=len(w["map_xyz"])).set(w["map_xyz"])
        lopt = api.Optimizer(max_poses=16, max_points=1024, max_edges=16384)
        _sweep(api, out, f"lidar/{which}", lambda flag: lopt.LocalVisualLidarBA(w, m, stop_flag=flag))
        if which == "full":
            out["linearize-lidar/full"] = _digest(lopt.linearize_lidar(w, m))
        lopt.close()
        m.close()
    # ---- batch: unstopped and closed at every round (look r + 1 stands in front of round r)
    wins = batch_windows()
    bat = api.BatchOptimizer(max_windows=len(wins), **_CAP)
    _sweep(api, out, "batch", lambda flag: bat.LocalBundleAdjustment(wins, stop_flag=flag), first_look=1)
    bat.close()
    # ---- global
    gopt = api.GlobalOptimizer(**_GCAP)

    def gba(w, flag=None):
        r = gopt.BundleAdjustment(w, stop_flag=flag)
        return dict(r, **{"info." + k: v for k, v in gopt.last_info().items()})

    for name in (GBA_SMALLEST, GBA_TWO_PANELS):
        out[f"global/{name}"] = _digest(gba(G.full_solve_map(name, Fp)))
    two = G.full_solve_map(GBA_TWO_PANELS, Fp)
    assert gopt.last_info()["panels"] == 2
    sm = G.stop_map(Fp)
    assert _sweep(api, out, "global/stop-map", lambda flag: gba(sm, flag)) > 2
    out["global/iterations-0"] = _digest(gba(dict(two, iterations=0)))
    api.lba_stop_at_look(0)  # BundleAdjustment has no entry check: the first look is the top of iteration 0
    out["global/flag-up-at-the-first-look"] = _digest(gba(two, np.zeros(1, np.int32)), api.lba_last_looks())
    api.lba_stop_at_look(-1)
    out["first-trial/global-two-panels"] = _digest(dict(api.gba_first_trial(gopt, two, fill=_FILL),
                                                        **{"info." + k: v for k, v in gopt.last_info().items()}))
    gopt.close()
    # ---- the inputs themselves
    inputs = [S.window(n) for n in LOCAL] + [lidar_window(k) for k in LIDAR] + wins + [G.full_solve_map(GBA_SMALLEST, Fp), two, sm]
    out["inputs"] = _sha(*[np.ascontiguousarray(w[k]).tobytes() for w in inputs for k in sorted(w) if isinstance(w[k], np.ndarray)])
    return out


def load():
    with open(FIXTURE) as f:
        return json.load(f)
