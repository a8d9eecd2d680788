"""LocalMapping::CreateNewMapPoints timing (not bench.py).  Workloads: synth.triangulation_problem at VGA with about 100 vocabulary
nodes: 1 000 key-points x 10 neighbours (the live RGB-D shape), x 30 neighbours (the monocular neighbour count), 2 000 key-points x
10 neighbours, and B = 8 problems of the live shape in one call.  Two ways to get the same results, timed alternately in blocks in
one process:

    device      the synchronous gfs_create_new_map_points call (staging, one upload, k_tri_candidates, k_tri_resolve, download)
    host        the path it replaces: the sequential restatement of the loop on one host thread
                (tests/host/triangulate_restatement.cpp: merge loop, Hamming search with gates, triangulation and gates)

Reports the median and p90 wall time of each over all calls, the per-block medians' ratio host / device (its minimum and maximum over
the blocks are the run-to-run spread), and checks that both paths return the same bytes.  Prints one JSON line; --out writes it.

    python tools/bench_triangulate.py [--blocks 10] [--calls 10] [--out profiles/triangulate_bench.json]
    python tools/bench_triangulate.py --loop 50 [--only 1000kp_x10nb]     # only device calls (for a kernel trace)
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
WORKLOADS = [dict(name="1000kp_x10nb", n_kp=1000, n_neighbours=10, B=1), dict(name="1000kp_x30nb", n_kp=1000, n_neighbours=30, B=1),
             dict(name="2000kp_x10nb", n_kp=2000, n_neighbours=10, B=1), dict(name="1000kp_x10nb_B8", n_kp=1000, n_neighbours=10, B=8)]
STEP_TIMEOUT_S = 900
KEYS = ("match12", "exit", "x3d", "point_stereo")


class Job:
    def __init__(self, wl):
        import triangulate_support as TS
        from geoflowslam_amd import api, synth
        self.B, self.nb, self.n = wl["B"], wl["n_neighbours"], wl["n_kp"]
        probs = [synth.triangulation_problem(300 + 7 * b + self.nb, n_kp=self.n, n_neighbours=self.nb, n_nodes=100) for b in range(self.B)]
        self.pairs = [api.tri_candidate_pairs(p) for p in probs]
        self.m = api.ProjectionMatcher(max_last=64, max_cur=self.n, max_batch=self.B)
        self.m.reserve_triangulation(self.nb, max(self.pairs))
        self.L, self.R = api.lib(), TS.restatement()
        self.dev = api.tri_structs(probs)
        self.hst = api.tri_structs(probs)

    def device(self):
        PP, RP, _ = self.dev
        rc = self.L.gfs_create_new_map_points(self.m.h, PP, self.B, RP)
        assert rc == 0, self.L.gfs_last_error()

    def host(self):
        PP, RP, _ = self.hst
        assert self.R.tr_create_new_map_points(PP, self.B, RP, None) == 0

    def results(self, which):
        from geoflowslam_amd import api
        PP, RP, keep = which
        return api.tri_results(PP, RP, keep, self.B)

    def same(self):
        a, b = self.results(self.dev), self.results(self.hst)
        return bool(all(x[k].tobytes() == y[k].tobytes() for pa, pb in zip(a, b) for x, y in zip(pa, pb) for k in KEYS) and
                    all(x["n_created"] == y["n_created"] and x["n_matches"] == y["n_matches"] for pa, pb in zip(a, b) for x, y in zip(pa, pb)))


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
        r0 = j.results(j.dev)[0]
        res[wl["name"]] = dict(n_kp=j.n, n_neighbours=j.nb, n_nodes=100, problems=j.B, candidate_pairs=j.pairs[0],
                               n_matches=sum(o["n_matches"] for o in r0), n_created=sum(o["n_created"] for o in r0),
                               calls=a.blocks * a.calls, device_ms_median=med["device"], device_ms_p90=float(np.percentile(ts["device"], 90)),
                               host_path_ms_median=med["host"], host_path_ms_p90=float(np.percentile(ts["host"], 90)),
                               ratio_host_over_device=med["host"] / med["device"], ratio_per_block_min=min(ratios),
                               ratio_per_block_max=max(ratios), same_results=bool(same))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--calls", type=int, default=10)
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
    out = dict(metric="create_new_map_points", latency="wall time of the synchronous call, alternating blocks in one process",
               workloads=json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
