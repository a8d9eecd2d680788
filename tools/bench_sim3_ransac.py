"""Timing of Sim3Solver, the RANSAC step of loop detection (not bench.py).  Workloads: synth.sim3_ransac_problem with 150 pairs, fixed
scale, min_inliers 15, 300 iterations (what SetRansacParameters(0.99, 15, 300) gives for 150 pairs), at three inlier shares that
decide how long the sequential loop runs -- 0.6 (converges within the first few iterations), 0.25 (tens of iterations), 0.05 (never:
all 300 run) -- one problem a call (B = 1) and three (B = 3: the candidates of one DetectCommonRegionsFromBoW).  Two ways to get the
same bytes, timed alternately in blocks in one process:

    device      the synchronous gfs_sim3_ransac_solve call (staging, one upload, two kernels, one download): every hypothesis scored
    host        the path it replaces, restated: the sequential loop on one host thread WITH its early stop, as the reference runs it
                (tests/host/sim3_ransac_restatement.cpp)

Reports the median and p90 wall time of each over all calls, the ratio host / device of the medians with the minimum and maximum of
the per-block ratios (the run-to-run spread), the iterations the sequential loop ran, and checks that both paths return the same
bytes.  Prints one JSON line; --out writes it.

    python tools/bench_sim3_ransac.py [--blocks 10] [--calls 20] [--out profiles/sim3_ransac_bench.json]
    python tools/bench_sim3_ransac.py --loop 30 [--only share0.05_b3]     # only device calls (for a kernel trace)
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
WORKLOADS = [dict(name=f"share{s}_b{B}", share=s, B=B) for s in (0.6, 0.25, 0.05) for B in (1, 3)]
N_PAIRS, MIN_INLIERS, ITERATIONS = 150, 15, 300


class Job:
    def __init__(self, wl):
        import sim3_ransac_support as S
        from geoflowslam_amd import api, synth
        self.S, self.api, self.B = S, api, wl["B"]
        probs = [synth.sim3_ransac_problem(700 + 13 * f + int(100 * wl["share"]), n_pairs=N_PAIRS, inlier_share=wl["share"], fix_scale=True,
                                           min_inliers=MIN_INLIERS, n_iterations=ITERATIONS) for f in range(self.B)]
        self.solver = api.Sim3RansacSolver(max_batch=self.B, max_pairs=N_PAIRS, max_iterations=ITERATIONS)
        self.L, self.R = api.lib(), S.restatement()
        self.R.s3rr_solve_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self.sets = []
        for _ in range(2):  # device, host: their own structs and output arrays
            PP, SS, keeps = (api.Sim3RansacProblem * self.B)(), (api.Sim3RansacSolution * self.B)(), []
            for f, p in enumerate(probs):
                P, Sl, keep, n = api.sim3_ransac_structs(p)
                PP[f], SS[f] = P, Sl
                keeps.append((keep, n))
            self.sets.append((PP, SS, keeps))

    def device(self):
        PP, SS, _ = self.sets[0]
        rc = self.L.gfs_sim3_ransac_solve(self.solver.h, PP, self.B, SS)
        assert rc == 0, self.L.gfs_last_error()

    def host(self):
        PP, SS, _ = self.sets[1]
        assert self.R.s3rr_solve_batch(C.cast(PP, C.c_void_p), self.B, C.cast(SS, C.c_void_p)) == 0

    def results(self, which):
        _, SS, keeps = self.sets[which]
        return [self.api.sim3_ransac_result(SS[f], *keeps[f]) for f in range(self.B)]

    def same(self):
        return all(self.S.solution_bytes(a) == self.S.solution_bytes(b) for a, b in zip(self.results(0), self.results(1)))


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
        same = j.same()
        ts, ratios = dict(device=[], host=[]), []
        for _ in range(a.blocks):
            blk = {k: _timed(getattr(j, k), a.calls) for k in ("device", "host")}
            for k in ts:
                ts[k] += blk[k]
            ratios.append(float(np.median(blk["host"]) / np.median(blk["device"])))
        same = same and j.same()
        med = {k: float(np.median(v)) for k, v in ts.items()}
        r = j.results(0)
        res[wl["name"]] = dict(n_pairs=N_PAIRS, batch=j.B, inlier_share=wl["share"], min_inliers=MIN_INLIERS, hypotheses_scored_by_device=ITERATIONS,
                               iterations_run_by_host=[x["iterations"] for x in r], status=[x["status"] for x in r],
                               n_inliers=[x["n_inliers"] for x in r], calls=a.blocks * a.calls, device_ms_median=med["device"],
                               device_ms_p90=float(np.percentile(ts["device"], 90)), host_path_ms_median=med["host"],
                               host_path_ms_p90=float(np.percentile(ts["host"], 90)), ratio_host_over_device=med["host"] / med["device"],
                               ratio_per_block_min=min(ratios), ratio_per_block_max=max(ratios), same_results=bool(same))
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
    out = dict(metric="sim3_ransac", latency="wall time of the synchronous call, alternating blocks in one process", workloads=measure(a))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
