"""Timing of the Sim3 searches of loop closing (not bench.py).  Workloads: synth.sim3_search_problem at VGA with 1 000 key-points a
key frame: SearchByProjection with vpPointsKFs (5 000 points x 1 key frame, th 8, ratio 1.5), SearchByProjection (5 000 x 1, th 3,
ratio 1.5), Fuse as LoopClosing::SearchAndFuse calls it (8 000 points x 40 key frames, th 4) and Fuse 1 000 x 1.  Two ways to get the
same per-point results, timed alternately in blocks in one process:

    device      the synchronous gfs_sim3_search call (staging, two uploads, k_sim3_search, download, the replay of the dependency)
    host        the path it replaces: the sequential restatement of the loops on one host thread
                (tests/host/sim3_search_restatement.cpp: grid, projection, gates, PredictScale, window search, live vpMatched)

Reports the median and p90 wall time of each over all calls, the per-block medians' ratio host / device (its minimum and maximum over
the blocks are the run-to-run spread), and checks that both paths return the same bytes.  Prints one JSON line; --out writes it.

    python tools/bench_sim3_search.py [--blocks 10] [--calls 20] [--out profiles/sim3_search_bench.json]
    python tools/bench_sim3_search.py --loop 30 [--only fuse_8000pts_x40kf] [--groups -1]   # only device calls (for a kernel trace)

--groups sets how many workgroups a launch may hold (gfs_test_sim3_search_groups): 0 the default (what the device holds at once; a
workgroup then keeps its grid and walks several 256-point chunks), -1 a workgroup a chunk.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WORKLOADS = [dict(name="sbp_kfs_5000pts_x1kf", mode=2, n_points=5000, n_problems=1, th=8.0, ratio=1.5, calls=1.0),
             dict(name="sbp_5000pts_x1kf", mode=1, n_points=5000, n_problems=1, th=3.0, ratio=1.5, calls=1.0),
             dict(name="fuse_8000pts_x40kf", mode=0, n_points=8000, n_problems=40, th=4.0, ratio=1.0, calls=0.15),
             dict(name="fuse_1000pts_x1kf", mode=0, n_points=1000, n_problems=1, th=4.0, ratio=1.0, calls=1.0)]
STEP_TIMEOUT_S = 1100
KEYS = ("exit", "best_idx", "best_dist", "level")


class Job:
    def __init__(self, wl, groups=0):
        import sim3_search_support as SS
        from geoflowslam_amd import api, synth
        prob = synth.sim3_search_problem(300 + wl["n_problems"], wl["mode"], n_points=wl["n_points"], n_kp=1000, n_problems=wl["n_problems"],
                                         th=wl["th"], ratio_hamming=wl["ratio"])
        self.n, self.B = wl["n_points"], wl["n_problems"]
        self.m = api.ProjectionMatcher(max_last=64, max_cur=1024, max_batch=1)
        self.m.reserve_sim3_search(1, self.n, self.B)
        self.L, self.R = api.lib(), SS.restatement()
        if groups:
            assert self.L.gfs_test_sim3_search_groups(self.m.h, groups) == 0
        self.dev = api.sim3_search_structs(prob["lists"], prob["problems"])
        self.hst = api.sim3_search_structs(prob["lists"], prob["problems"])

    def device(self):
        LL, PP, RR, _ = self.dev
        rc = self.L.gfs_sim3_search(self.m.h, LL, 1, PP, self.B, RR)
        assert rc == 0, self.L.gfs_last_error()

    def host(self):
        LL, PP, RR, _ = self.hst
        assert self.R.sr_sim3_search(LL, 1, PP, self.B, RR, None) == 0

    def same(self):
        ok = True
        for f in range(self.B):
            a, b = self.dev[3][1 + f], self.hst[3][1 + f]
            searched = (b["exit"][:self.n] >= 5) & (b["exit"][:self.n] <= 7)  # level is defined where the window was reached
            ok &= all(np.array_equal(a[k][:self.n], b[k][:self.n]) for k in KEYS[:3]) and np.array_equal(a["level"][:self.n][searched], b["level"][:self.n][searched])
            ok &= int(self.dev[2][f].n_matched) == int(self.hst[2][f].n_matched)
        return bool(ok)


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
        if a.only and wl["name"] != a.only:
            continue
        j = Job(wl, a.groups)
        calls = max(2, int(round(a.calls * wl["calls"])))
        for _ in range(3):  # warm-up
            j.host()
            j.device()
        same = j.same()
        ts = dict(device=[], host=[])
        ratios = []
        for _ in range(a.blocks):
            blk = {k: _timed(getattr(j, k), calls) for k in ("device", "host")}
            for k in ts:
                ts[k] += blk[k]
            ratios.append(float(np.median(blk["host"]) / np.median(blk["device"])))
        same = same and j.same()
        med = {k: float(np.median(v)) for k, v in ts.items()}
        res[wl["name"]] = dict(mode=wl["mode"], n_points=j.n, n_kp=1000, n_problems=j.B, th=wl["th"], ratio_hamming=wl["ratio"],
                               n_matched=[int(j.dev[2][f].n_matched) for f in range(j.B)][:4], calls=a.blocks * calls,
                               device_ms_median=med["device"], device_ms_p90=float(np.percentile(ts["device"], 90)),
                               host_path_ms_median=med["host"], host_path_ms_p90=float(np.percentile(ts["host"], 90)),
                               ratio_host_over_device=med["host"] / med["device"], ratio_per_block_min=min(ratios),
                               ratio_per_block_max=max(ratios), same_results=bool(same))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loop", type=int, default=0, help="only run this many device calls of each workload")
    ap.add_argument("--only", default=None, help="this workload alone")
    ap.add_argument("--groups", type=int, default=0, help="workgroups a launch may hold: 0 default, -1 a workgroup a chunk")
    ap.add_argument("--step", default=None, choices=["measure"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.loop:
        for wl in WORKLOADS:
            if a.only and wl["name"] != a.only:
                continue
            j = Job(wl, a.groups)
            for _ in range(a.loop):
                j.device()
        return
    if a.step:  # child
        print(json.dumps(step_measure(a)))
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "measure", "--blocks", str(a.blocks), "--calls", str(a.calls), "--groups", str(a.groups)]
    r = subprocess.run(cmd + (["--only", a.only] if a.only else []), capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"the measurement failed with exit status {r.returncode}")
    out = dict(metric="sim3_search", latency="wall time of the synchronous call, alternating blocks in one process", groups=a.groups,
               workloads=json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
