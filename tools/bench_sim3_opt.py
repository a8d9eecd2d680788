"""Timing of OptimizeSim3, the Sim3 refinement of loop verification (not bench.py).  Workloads: synth.sim3_opt_problem with 60, 150 and
400 pairs, fixed scale, 15 % gross outliers; one problem a call (B = 1) and twelve (B = 12: the candidates of
DetectCommonRegionsFromBoW, each followed by up to three covisible key frames).  Two ways to get the same bytes, timed alternately in
blocks in one process:

    device      the synchronous gfs_sim3_optimize call (staging, one upload, k_sim3_opt, one download)
    host        the path it replaces, restated: the sequential per-edge loops of g2o on one host thread
                (tests/host/sim3_opt_restatement.cpp, float64)

Reports the median and p90 wall time of each over all calls, the ratio host / device of the medians with the minimum and maximum of
the per-block ratios (the run-to-run spread), and checks that both paths return the same bytes.  Prints one JSON line; --out writes it.

    python tools/bench_sim3_opt.py [--blocks 10] [--calls 20] [--out profiles/sim3_opt_bench.json]
    python tools/bench_sim3_opt.py --loop 30 [--only pairs400_b1]     # only device calls (for a kernel trace)
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
WORKLOADS = [dict(name=f"pairs{n}_b{B}", n_pairs=n, B=B) for n in (60, 150, 400) for B in (1, 12)]


class Job:
    def __init__(self, wl):
        import sim3_opt_support as S
        from geoflowslam_amd import api, synth
        self.S, self.api, self.B, self.n = S, api, wl["B"], wl["n_pairs"]
        probs = [synth.sim3_opt_problem(500 + 17 * f + wl["n_pairs"], n_pairs=wl["n_pairs"], fix_scale=True, outlier_share=0.15) for f in range(self.B)]
        self.opt = api.Sim3Optimizer(max_batch=self.B, max_pairs=self.n)
        self.L, self.R = api.lib(), S.restatement()
        self.sets = []
        for _ in range(2):  # device, host: their own structs and output arrays
            PP, SS, keeps = (api.Sim3OptProblem * self.B)(), (api.Sim3OptSolution * self.B)(), []
            for f, p in enumerate(probs):
                P, Sl, keep, n = api.sim3_opt_structs(p)
                PP[f], SS[f] = P, Sl
                keeps.append((keep, n))
            self.sets.append((PP, SS, keeps))

    def device(self):
        PP, SS, _ = self.sets[0]
        rc = self.L.gfs_sim3_optimize(self.opt.h, PP, self.B, SS)
        assert rc == 0, self.L.gfs_last_error()

    def host(self):
        PP, SS, _ = self.sets[1]
        assert self.R.s3r_optimize_batch(C.cast(PP, C.c_void_p), self.B, C.cast(SS, C.c_void_p)) == 0

    def results(self, which):
        _, SS, keeps = self.sets[which]
        return [self.api.sim3_opt_result(SS[f], *keeps[f]) for f in range(self.B)]

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
        res[wl["name"]] = dict(n_pairs=j.n, batch=j.B, fix_scale=True, outlier_share=0.15, n_in=[x["n_in"] for x in r][:4],
                               n_bad=[x["n_bad"] for x in r][:4], iterations_run=[list(x["iterations_run"]) for x in r][:4],
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
    out = dict(metric="sim3_opt", latency="wall time of the synchronous call, alternating blocks in one process", workloads=measure(a))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
