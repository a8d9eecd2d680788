"""Timing of LocalInertialBA, the inertial local BA of LocalMapping (not bench.py).  Workloads: synth.lba_inertial_window with about
2 000 points, each seen from 8 to 16 key frames where it is in view, and 10 other fixed key frames -- a window of 10 key frames (w10: 8 iterations, lambda 1e0) and one of 20 with the bLarge
settings (w20_large: 4 iterations, lambda 1e-2).  Three paths, timed alternately in blocks in one process after a warm-up:

    device      the synchronous gfs_lba_inertial_solve call (staging, one upload, the queued kernels, one download)
    host        the sequential restatement on ONE host thread (tests/host/lba_inertial_restatement.cpp), which returns the same bytes.
                It is NOT g2o: the reference's g2o and Eigen are not built here, so this says nothing about the reference's own time
    visual      gfs_lba_solve on the same visual edges from the same start with the window's poses free (6 unknowns each, no IMU)
                and the same iteration count: the size-matched visual-only figure

Reports the median and p90 wall time of each over all calls, the ratios of the medians with the minimum and maximum of the per-block
ratios (the run-to-run spread), and checks that device and host return the same bytes.  Prints one JSON line; --out writes it.

    python tools/bench_lba_inertial.py [--blocks 5] [--calls 10] [--out profiles/lba_inertial_bench.json]
    python tools/bench_lba_inertial.py --loop 20 [--only w10] [--profile]   # only device calls; --profile: per-kernel device time
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WORKLOADS = [dict(name="w10", n_opt=10, large=False), dict(name="w20_large", n_opt=20, large=True)]


class Job:
    def __init__(self, wl):
        import lba_inertial_support as S
        from geoflowslam_amd import api, synth
        self.S, self.api = S, api
        self.w = w = synth.lba_inertial_window(900 + wl["n_opt"], n_opt=wl["n_opt"], n_fixed=10, n_points=2000, large=wl["large"], noise_scale=0.5,
                                                  obs_per_point=(8, 16))
        self.ba = api.LocalInertialBA(max_opt=20, max_fixed=10, max_points=2048, max_edges=32768)
        self.L, self.R = api.lib(), S.restatement()
        self.sets = [api.lba_inertial_structs(w) for _ in range(2)]  # device, host: their own structs and output arrays
        K = w["n_opt"] + 1 + w["n_fixed"]
        cams = [w["window"][i]["Rcw"] for i in range(w["n_opt"])] + [w["prev"]["Rcw"]] + list(w["fixed_Rcw"])
        ts = [w["window"][i]["tcw"] for i in range(w["n_opt"])] + [w["prev"]["tcw"]] + list(w["fixed_tcw"])
        fixed = np.ones(K, np.uint8)
        fixed[:w["n_opt"]] = 0
        self.vprob = dict(n_poses=K, n_points=w["n_points"], n_edges=w["n_edges"], pose_q=np.array([synth._quat_from_R(R) for R in cams]),
                          pose_t=np.array(ts, np.float64), pose_fixed=fixed, points=w["points"], edge_pose=w["edge_kf"],
                          edge_point=np.repeat(np.arange(w["n_points"], dtype=np.int32), np.diff(w["point_edge_begin"])), edge_obs=w["obs"],
                          edge_inv_sigma2=w["inv_sigma2"].astype(np.float64), edge_stereo=w["stereo"], fx=w["fx"], fy=w["fy"], cx=w["cx"], cy=w["cy"],
                          bf=w["bf"], huber_mono=float(np.float32(np.sqrt(5.991))), huber_stereo=float(np.float32(np.sqrt(7.815))),
                          iterations=w["iterations"])
        self.vis = api.Optimizer(max_poses=K, max_points=2048, max_edges=32768)
        self.vis_out = None

    def device(self):
        P, Sl, _ = self.sets[0]
        rc = self.L.gfs_lba_inertial_solve(self.ba.h, C.byref(P), C.byref(Sl))
        assert rc == 0, self.L.gfs_last_error()

    def host(self):
        P, Sl, _ = self.sets[1]
        assert self.R.lir_solve(C.byref(P), C.byref(Sl), None) == 0

    def visual(self):
        self.vis_out = self.vis.LocalBundleAdjustment(self.vprob)

    def result(self, which):
        P, Sl, keep = self.sets[which]
        return self.api.lba_inertial_result(Sl, keep, self.w)

    def same(self):
        return self.S.result_bytes(self.result(0)) == self.S.result_bytes(self.result(1))


def _timed(fn, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def measure(a):
    res = {}
    for wl in WORKLOADS:
        if a.only and wl["name"] != a.only:
            continue
        j = Job(wl)
        for _ in range(3):  # warm-up
            j.host()
            j.device()
            j.visual()
        same = j.same()
        ts, r_host, r_vis = dict(device=[], host=[], visual=[]), [], []
        for _ in range(a.blocks):
            blk = {k: _timed(getattr(j, k), a.calls) for k in ("device", "host", "visual")}
            for k in ts:
                ts[k] += blk[k]
            r_host.append(float(np.median(blk["host"]) / np.median(blk["device"])))
            r_vis.append(float(np.median(blk["device"]) / np.median(blk["visual"])))
        same = same and j.same()
        med = {k: float(np.median(v)) for k, v in ts.items()}
        r, w = j.result(0), j.w
        res[wl["name"]] = dict(n_opt=w["n_opt"], n_fixed=w["n_fixed"], n_points=w["n_points"], n_edges=w["n_edges"], iterations=w["iterations"],
                               lambda_init=w["lambda_init"], iterations_run=r["iterations_run"], trials_run=r["trials_run"], err=float(r["err"]),
                               err_end=float(r["err_end"]), visual_iterations_run=int(j.vis_out["iterations_run"]), calls=a.blocks * a.calls,
                               device_ms_median=med["device"], device_ms_p90=float(np.percentile(ts["device"], 90)),
                               device_ms_min=float(np.min(ts["device"])), host_restatement_ms_median=med["host"],
                               host_restatement_ms_p90=float(np.percentile(ts["host"], 90)), visual_only_ms_median=med["visual"],
                               visual_only_ms_p90=float(np.percentile(ts["visual"], 90)), ratio_host_over_device=med["host"] / med["device"],
                               ratio_host_over_device_per_block=[min(r_host), max(r_host)], ratio_device_over_visual=med["device"] / med["visual"],
                               ratio_device_over_visual_per_block=[min(r_vis), max(r_vis)], same_results=bool(same))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loop", type=int, default=0, help="only run this many device calls of each workload")
    ap.add_argument("--only", default=None, help="this workload alone")
    ap.add_argument("--profile", action="store_true", help="with --loop: print the per-kernel device time (HIP events around each launch)")
    a = ap.parse_args()
    if a.loop:
        from geoflowslam_amd import api
        for wl in WORKLOADS:
            if a.only and wl["name"] != a.only:
                continue
            j = Job(wl)
            j.device()
            if a.profile:
                api.profile_reset()
                api.profile_enable(True)
            for _ in range(a.loop):
                j.device()
            if a.profile:
                api.profile_enable(False)
                rows = sorted(((ms / a.loop, n // a.loop, name) for name, (ms, n) in api.profile_report().items()), reverse=True)
                print(json.dumps(dict(workload=wl["name"], per_call_ms={nm: round(t, 4) for t, _, nm in rows}, launches_per_call={nm: c for _, c, nm in rows})))
        return
    out = dict(metric="lba_inertial", latency="wall time of the synchronous call, alternating blocks in one process",
               host_path="the sequential restatement on one host thread, not g2o", workloads=measure(a))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
