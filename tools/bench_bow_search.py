"""Timing of SearchByBoW, the BoW-guided matching of loop detection (not bench.py).  Workloads: synth.bow_search_problem,

    pair_1000       one pair of key frames of 1 000 key-points over 100 nodes
    candidate_1000  one candidate: one key frame 1 against 11 key frames 2, 1 000 key-points, 100 nodes
    detection_2000  the detection shape: 3 candidates x 11 key frames 2, 2 000 key-points, 100 nodes

matcherBoW(0.9, true).  Two ways to get the same bytes, timed alternately in blocks in one process:

    device      the synchronous gfs_search_by_bow call (validation, staging, one upload, k_bow_search, one download)
    host        the path it replaces, restated: the sequential loops of ORBmatcher::SearchByBoW on one host thread
                (tests/host/bow_search_restatement.cpp; its trace pass, which scans every idx1 a second time, is compiled in, so the
                host figure is an upper bound of about twice the plain loop -- host_plain is the rule header's host build without it)

Reports the median and p90 wall time of each over all calls, the ratio host / device of the medians with the minimum and maximum of
the per-block ratios (the run-to-run spread), and checks that the paths return the same bytes.  Prints one JSON line; --out writes it.

    python tools/bench_bow_search.py [--blocks 10] [--calls 20] [--out profiles/bow_search_bench.json]
    python tools/bench_bow_search.py --loop 30 [--only detection_2000]     # only device calls (for a kernel trace)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
WORKLOADS = [dict(name="pair_1000", n_kp=1000, n_kf2=1, B=1), dict(name="candidate_1000", n_kp=1000, n_kf2=11, B=1),
             dict(name="detection_2000", n_kp=2000, n_kf2=11, B=3)]


class Job:
    def __init__(self, wl):
        import bow_search_support as BS
        from geoflowslam_amd import api, synth
        self.BS, self.api, self.wl = BS, api, wl
        self.probs = [synth.bow_search_problem(700 + 13 * b + wl["n_kp"], n_kp=wl["n_kp"], n_kf2=wl["n_kf2"], n_nodes=100, nn_ratio=0.9,
                                               check_orientation=True) for b in range(wl["B"])]
        self.m = api.ProjectionMatcher(max_last=64, max_cur=wl["n_kp"], max_batch=1)
        self.m.reserve_bow(wl["B"], wl["B"] * wl["n_kf2"])
        self.L, self.R = api.lib(), BS.restatement()
        self.sets = [api.bow_structs(self.probs) for _ in range(3)]  # device, host, host_plain: their own structs and output arrays

    def device(self):
        PP, RP, _ = self.sets[0]
        rc = self.L.gfs_search_by_bow(self.m.h, PP, len(self.probs), RP)
        assert rc == 0, self.L.gfs_last_error()

    def host(self):
        PP, RP, _ = self.sets[1]
        assert self.R.bw_search_by_bow(PP, len(self.probs), RP, None) == 0

    def host_plain(self):
        PP, RP, _ = self.sets[2]
        assert self.R.bw_rule_search_by_bow(PP, len(self.probs), RP) == 0

    def results(self, which):
        PP, RP, keep = self.sets[which]
        return self.api.bow_results(PP, RP, keep, len(self.probs))

    def same(self):
        a = self.results(0)
        for other in (self.results(1), self.results(2)):
            for g, w in zip(a, other):
                self.BS.assert_equal(g, w, self.wl["name"])
        return True


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
            j.host_plain()
            j.device()
        same = j.same()
        kinds = ("device", "host", "host_plain")
        ts, ratios = {k: [] for k in kinds}, []
        for _ in range(a.blocks):
            blk = {k: _timed(getattr(j, k), a.calls) for k in kinds}
            for k in ts:
                ts[k] += blk[k]
            ratios.append(float(np.median(blk["host_plain"]) / np.median(blk["device"])))
        same = same and j.same()
        med = {k: float(np.median(v)) for k, v in ts.items()}
        r = j.results(0)
        res[wl["name"]] = dict(n_kp=wl["n_kp"], n_kf2=wl["n_kf2"], problems=wl["B"], n_nodes=100, nn_ratio=0.9, check_orientation=True,
                               n_matches=[[o["n_matches"] for o in x][:4] for x in r], calls=a.blocks * a.calls,
                               device_ms_median=med["device"], device_ms_p90=float(np.percentile(ts["device"], 90)),
                               host_path_ms_median=med["host"], host_path_ms_p90=float(np.percentile(ts["host"], 90)),
                               host_plain_ms_median=med["host_plain"], host_plain_ms_p90=float(np.percentile(ts["host_plain"], 90)),
                               ratio_host_plain_over_device=med["host_plain"] / med["device"], ratio_per_block_min=min(ratios),
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
    workloads = measure(a)
    import ctypes
    name = ctypes.create_string_buffer(256)
    if ctypes.CDLL("libamdhip64.so").hipDeviceGetName(name, 256, 0) != 0 or not name.value:  # (the runtime the library has loaded)
        name.value = b"gfx950 (the runtime reports no marketing name)"  # the library runs on nothing else
    out = dict(metric="bow_search", command=" ".join(["python", "tools/bench_bow_search.py"] + sys.argv[1:]), device=name.value.decode(),
               latency="wall time of the synchronous call, alternating blocks in one process", host="one thread", workloads=workloads)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
