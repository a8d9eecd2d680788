"""Map-point update timing (not bench.py).  Workloads: synth.map_point_update_problem with
1 000 points of 2..20 observations (a guess at the tail of LocalMapping::SearchInNeighbors: nobody has measured the distribution of
the observation counts in a real run), 1 000 points of 20..80, 3 000 points in normals-only mode (the write-back of local bundle
adjustment) and 50 points (expected to be bound by the call's latency).  Two ways to get the same results, timed alternately in
blocks in one process:

    device      the synchronous gfs_map_points_update call (staging, one upload, k_map_points, one download)
    host        the path it replaces: the sequential restatement of the per-point loops on one host thread
                (tests/host/map_point_restatement.cpp: N x N table, a sort per row, the serial normal sum)

Reports the median and p90 wall time of each over all calls, the per-block medians' ratio host / device (its minimum and maximum over
the blocks are the run-to-run spread), whether the device won, and checks that both paths return the same bytes.  Prints one JSON
line; --out writes it.

    python tools/bench_map_point_update.py [--blocks 10] [--calls 20] [--out profiles/map_point_update_bench.json]
    python tools/bench_map_point_update.py --loop 50 [--only 1000pts_2to20]     # only device calls (for a kernel trace)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WORKLOADS = [dict(name="1000pts_2to20", n_points=1000, counts=(2, 20), normals_only=False),
             dict(name="1000pts_20to80", n_points=1000, counts=(20, 80), normals_only=False),
             dict(name="3000pts_normals_only", n_points=3000, counts=(2, 20), normals_only=True),
             dict(name="50pts_2to20", n_points=50, counts=(2, 20), normals_only=False)]
STEP_TIMEOUT_S = 900
KEYS = ("best_obs", "best_median", "normal", "min_dist", "max_dist", "status")


class Job:
    def __init__(self, wl):
        import map_point_support as MS
        from geoflowslam_amd import api, synth
        prob = synth.map_point_update_problem(300 + wl["n_points"] + wl["counts"][1], n_points=wl["n_points"], obs_counts=wl["counts"],
                                              n_keyframes=100)
        self.n, self.n_obs = wl["n_points"], int(prob["obs_start"][-1])
        self.u = api.MapPointUpdater(max_points=self.n, max_observations=max(self.n_obs, 1))
        self.L, self.R = api.lib(), MS.restatement()
        self.dev = api.map_points_structs(prob, wl["normals_only"])
        self.hst = api.map_points_structs(prob, wl["normals_only"])

    def device(self):
        P, R, _ = self.dev
        rc = self.L.gfs_map_points_update(self.u.h, C.byref(P), C.byref(R))
        assert rc == 0, self.L.gfs_last_error()

    def host(self):
        P, R, _ = self.hst
        assert self.R.mr_update(C.byref(P), C.byref(R), None) == 0

    def same(self):
        import map_point_support as MS
        return all(MS.same_bits(self.dev[2][k][:self.n], self.hst[2][k][:self.n]) for k in KEYS)


def _timed(fn, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def step_measure(a):
    res = {}
    for wl in WORKLOADS:
        j = Job(wl)
        for _ in range(5):  # warm-up
            j.host()
            j.device()
        same = j.same()
        ts = dict(device=[], host=[])
        ratios = []
        for _ in range(a.blocks):
            blk = {k: _timed(getattr(j, k), a.calls) for k in ("device", "host")}
            for k in ts:
                ts[k] += blk[k]
            ratios.append(float(np.median(blk["host"]) / np.median(blk["device"])))
        same = same and j.same()
        med = {k: float(np.median(v)) for k, v in ts.items()}
        res[wl["name"]] = dict(n_points=j.n, n_observations=j.n_obs, normals_only=wl["normals_only"], calls=a.blocks * a.calls,
                               device_ms_median=med["device"], device_ms_p90=float(np.percentile(ts["device"], 90)),
                               host_path_ms_median=med["host"], host_path_ms_p90=float(np.percentile(ts["host"], 90)),
                               ratio_host_over_device=med["host"] / med["device"], ratio_per_block_min=min(ratios),
                               ratio_per_block_max=max(ratios), device_won=bool(min(ratios) > 1.0), device_lost=bool(max(ratios) < 1.0),
                               same_results=bool(same))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loop", type=int, default=0, help="only run this many device calls of each workload")
    ap.add_argument("--only", default=None, help="with --loop: this workload alone")
    ap.add_argument("--step", default=None, choices=["measure"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.loop:
        for wl in WORKLOADS:
            if a.only and wl["name"] != a.only:
                continue
            j = Job(wl)
            for _ in range(a.loop):
                j.device()
        return
    if a.step:  # child
        print(json.dumps(step_measure(a)))
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "measure", "--blocks", str(a.blocks), "--calls", str(a.calls)],
                       capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"the measurement failed with exit status {r.returncode}")
    out = dict(metric="map_point_update", latency="wall time of the synchronous call, alternating blocks in one process",
               workloads=json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
