"""ORBmatcher::Fuse search timing (not bench.py).  Workloads: synth.fuse_problem at VGA with 1 000 key-points a key frame:
1 000 points x 1 key frame, 1 000 points x 30 key frames (the first direction of LocalMapping::SearchInNeighbors: the current key
frame's points in every target) and 20 000 points x 1 key frame (the second direction: the targets' points in the current key
frame).  Two ways to get the same per-point results, timed alternately in blocks in one process:

    device      the synchronous gfs_fuse_search call (staging, two uploads, k_fuse, download)
    host        the path it replaces: the sequential restatement of the loop on one host thread
                (tests/host/fuse_restatement.cpp: grid, projection, gates, PredictScale, window search)

Reports the median and p90 wall time of each over all calls, the per-block medians' ratio host / device (its minimum and maximum over
the blocks are the run-to-run spread), and checks that both paths return the same bytes.  Prints one JSON line; --out writes it.

    python tools/bench_fuse.py [--blocks 10] [--calls 20] [--out profiles/fuse_bench.json]
    python tools/bench_fuse.py --loop 50 [--only 1000pts_x30kf]     # only device calls (for a kernel trace)
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
WORKLOADS = [dict(name="1000pts_x1kf", n_points=1000, n_keyframes=1), dict(name="1000pts_x30kf", n_points=1000, n_keyframes=30),
             dict(name="20000pts_x1kf", n_points=20000, n_keyframes=1)]
STEP_TIMEOUT_S = 900
KEYS = ("exit", "best_idx", "best_dist", "level")


class Job:
    def __init__(self, wl):
        import fuse_support as FS
        from geoflowslam_amd import api, synth
        prob = synth.fuse_problem(200 + wl["n_keyframes"], n_points=wl["n_points"], n_kp=1000, n_keyframes=wl["n_keyframes"])
        self.n, self.B = wl["n_points"], wl["n_keyframes"]
        self.m = api.ProjectionMatcher(max_last=64, max_cur=1024, max_batch=1)
        self.m.reserve_fuse(1, self.n, self.B)
        self.L, self.R = api.lib(), FS.restatement()
        self.dev = api.fuse_structs(prob["lists"], prob["keyframes"])
        self.hst = api.fuse_structs(prob["lists"], prob["keyframes"])

    def device(self):
        LL, KK, RR, _ = self.dev
        rc = self.L.gfs_fuse_search(self.m.h, LL, 1, KK, self.B, RR)
        assert rc == 0, self.L.gfs_last_error()

    def host(self):
        LL, KK, RR, _ = self.hst
        assert self.R.fr_fuse_search(LL, 1, KK, self.B, RR, None) == 0

    def same(self):
        ok = True
        for f in range(self.B):
            a, b = self.dev[3][1 + f], self.hst[3][1 + f]
            searched = b["exit"][:self.n] >= 5  # level is defined from "empty window" on
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
        res[wl["name"]] = dict(n_points=j.n, n_kp=1000, n_keyframes=j.B, n_matched=[int(j.dev[2][f].n_matched) for f in range(j.B)][:4],
                               calls=a.blocks * a.calls, device_ms_median=med["device"], device_ms_p90=float(np.percentile(ts["device"], 90)),
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
    out = dict(metric="fuse_search", latency="wall time of the synchronous call, alternating blocks in one process",
               workloads=json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
