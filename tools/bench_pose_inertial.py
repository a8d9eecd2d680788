"""Timing of PoseInertialOptimization, the IMU pose step of TrackLocalMap (not bench.py).  Workloads: synth.pose_inertial_problem with
300 visual edges, 15 % outliers, 4 rounds -- one problem in key-frame mode (kf_b1), one in frame mode (fr_b1), and a batch of 16 with
the modes alternating (mixed_b16).  Three paths, timed alternately in blocks in one process after a warm-up:

    device      the synchronous gfs_pose_inertial_optimize call (staging, one upload, one kernel, one download)
    host        the sequential restatement on ONE host thread (tests/host/pose_inertial_restatement.cpp), which returns the same bytes.
                It is NOT g2o: the reference's g2o and Eigen are not built here, so this says nothing about the reference's own time
    visual      gfs_pose_optimize (edge-order sums, the ABI default) on the same visual edges from the same start: the visual twin,
                an LM solve of 6 unknowns; device - visual is what the inertial part costs on top

Reports the median and p90 wall time of each over all calls, the ratios of the medians with the minimum and maximum of the per-block
ratios (the run-to-run spread), and checks that device and host return the same bytes.  Prints one JSON line; --out writes it.

    python tools/bench_pose_inertial.py [--blocks 10] [--calls 20] [--out profiles/pose_inertial_bench.json]
    python tools/bench_pose_inertial.py --loop 30 [--only fr_b1]     # only device calls (for a kernel trace)
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
N_OBS = 300
WORKLOADS = [dict(name="kf_b1", modes=[0]), dict(name="fr_b1", modes=[1]), dict(name="mixed_b16", modes=[k % 2 for k in range(16)])]


class Job:
    def __init__(self, wl):
        import pose_inertial_support as S
        from geoflowslam_amd import api, synth
        self.S, self.api, self.B = S, api, len(wl["modes"])
        self.probs = [synth.pose_inertial_problem(800 + 7 * f, m, n_obs=N_OBS, outlier_share=0.15) for f, m in enumerate(wl["modes"])]
        self.opt = api.PoseInertialOptimizer(max_obs=N_OBS, max_batch=self.B)
        self.vis = api.PoseOptimizer(max_obs=N_OBS, max_batch=self.B, sums="edge_order")
        self.L, self.R = api.lib(), S.restatement()
        self.R.pir_optimize_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self.sets = []
        for _ in range(2):  # device, host: their own structs and output arrays
            PP, SS, keeps = (api.PoseInertialProblem * self.B)(), (api.PoseInertialSolution * self.B)(), []
            for f, p in enumerate(self.probs):
                P, Sl, keep, n = api.pose_inertial_structs(p)
                PP[f], SS[f] = P, Sl
                keeps.append((keep, n, P.mode))
            self.sets.append((PP, SS, keeps))
        self.VP, self.VS, self.vkeep = (api.PoseProblem * self.B)(), (api.PoseSolution * self.B)(), []
        for f, p in enumerate(self.probs):
            q = synth._quat_from_R(p["cur"]["Rcw"])
            P, Sl, keep, n = api.pose_structs(dict(q=q, t=p["cur"]["tcw"], n_obs=N_OBS, xw=p["xw"], obs=p["obs"], inv_sigma2=p["inv_sigma2"],
                                                   stereo=p["stereo"], fx=p["fx"], fy=p["fy"], cx=p["cx"], cy=p["cy"], bf=p["bf"], n_rounds=4, its=10))
            self.VP[f], self.VS[f] = P, Sl
            self.vkeep.append(keep)

    def device(self):
        PP, SS, _ = self.sets[0]
        rc = self.L.gfs_pose_inertial_optimize(self.opt.h, PP, self.B, SS)
        assert rc == 0, self.L.gfs_last_error()

    def host(self):
        PP, SS, _ = self.sets[1]
        assert self.R.pir_optimize_batch(C.cast(PP, C.c_void_p), self.B, C.cast(SS, C.c_void_p)) == 0

    def visual(self):
        rc = self.L.gfs_pose_optimize(self.vis.h, self.VP, self.B, self.VS)
        assert rc == 0, self.L.gfs_last_error()

    def results(self, which):
        _, SS, keeps = self.sets[which]
        return [self.api.pose_inertial_result(SS[f], *keeps[f]) for f in range(self.B)]

    def same(self):
        return all(self.S.result_bytes(a) == self.S.result_bytes(b) for a, b in zip(self.results(0), self.results(1)))


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
        for _ in range(5):  # warm-up
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
        r = j.results(0)
        res[wl["name"]] = dict(n_obs=N_OBS, batch=j.B, modes=wl["modes"], n_good=[x["n_good"] for x in r], rounds_run=[x["rounds_run"] for x in r],
                               calls=a.blocks * a.calls, device_ms_median=med["device"], device_ms_p90=float(np.percentile(ts["device"], 90)),
                               device_ms_min=float(np.min(ts["device"])), host_restatement_ms_median=med["host"],
                               host_restatement_ms_p90=float(np.percentile(ts["host"], 90)), visual_twin_ms_median=med["visual"],
                               visual_twin_ms_p90=float(np.percentile(ts["visual"], 90)), ratio_host_over_device=med["host"] / med["device"],
                               ratio_host_over_device_per_block=[min(r_host), max(r_host)], ratio_device_over_visual=med["device"] / med["visual"],
                               ratio_device_over_visual_per_block=[min(r_vis), max(r_vis)], same_results=bool(same))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loop", type=int, default=0, help="only run this many device calls of each workload")
    ap.add_argument("--only", default=None, help="this workload alone")
    a = ap.parse_args()
    if a.loop:
        for wl in WORKLOADS:
            if a.only and wl["name"] != a.only:
                continue
            j = Job(wl)
            for _ in range(a.loop):
                j.device()
        return
    out = dict(metric="pose_inertial", latency="wall time of the synchronous call, alternating blocks in one process",
               host_path="the sequential restatement on one host thread, not g2o", workloads=measure(a))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
