"""SearchLocalPoints timing (not bench.py).  Workloads: synth.local_points_frame, one VGA frame with 1 000 key-points and 2 000 /
6 000 local map points, and a batch of 64 of the 2 000-point frame.  Two ways to get the same matches, timed alternately in blocks in
one process:

    device      the synchronous gfs_search_local_points call (staging, upload, frustum + compaction + search kernels, download)
    host        what there was before it: the sequential restatement's frustum loop on one host thread
                (tests/host/local_points_restatement.cpp: isInFrustum, PredictScale, the compaction), then
                gfs_search_by_projection_map on its output, and the matches mapped back to list indices

Reports the median and p90 wall time of each over all calls, the per-block medians' ratio host / device (its minimum and maximum over
the blocks are the run-to-run spread), and checks that both paths return the same matches.  Prints one JSON line; --out writes it.

    python tools/bench_local_points.py [--blocks 10] [--calls 20] [--out profiles/local_points_bench.json]
    python tools/bench_local_points.py --loop 50      # only device calls (for a kernel trace)
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
WORKLOADS = [dict(name="2000pts_1000kps", n_points=2000, batch=1), dict(name="6000pts_1000kps", n_points=6000, batch=1),
             dict(name="2000pts_1000kps_b64", n_points=2000, batch=64)]
STEP_TIMEOUT_S = 900


class Job:
    def __init__(self, wl):
        import local_points_support as LPS
        from geoflowslam_amd import api, synth
        self.api, self.B = api, wl["batch"]
        B = self.B
        probs = [synth.local_points_frame(100 + f, n_points=wl["n_points"], n_cur=1000) for f in range(B)]
        self.n_mp, self.n_cur = wl["n_points"], 1000
        self.m = api.ProjectionMatcher(max_last=8192, max_cur=1024, max_batch=B)
        self.m.reserve_local(wl["n_points"])
        self.L, self.R = api.lib(), LPS.restatement()
        # device path
        self.PP, self.RR = (api.LocalPointsProblem * B)(), (api.LocalPointsResult * B)()
        self.keeps = []
        for f, p in enumerate(probs):
            self.PP[f], self.RR[f], keep = api.local_points_structs(p)
            self.keeps.append(keep)
        # host path: the restatement's per-point outputs and compacted arrays, then the existing map search
        self.HR = (api.LocalPointsResult * B)()
        self.MP = (api.SbpMapProblem * B)()
        self.hk, self.cm = [], []
        self.ptrs = (C.c_void_p * B)()
        self.nm = np.zeros(B, np.int32)
        n = wl["n_points"]
        for f, p in enumerate(probs):
            _, self.HR[f], hkeep = api.local_points_structs(p)
            c = dict(index=np.zeros(n, np.int32), proj=np.zeros((n, 3), np.float32), level=np.zeros(n, np.int32),
                     cos=np.zeros(n, np.float32), desc=np.zeros((n, 32), np.uint8), obs=np.zeros(n, np.uint8),
                     match=np.zeros(self.n_cur, np.int32))
            M, k = self.MP[f], self.keeps[f]
            M.mp_proj, M.mp_level, M.mp_view_cos = c["proj"].ctypes.data, c["level"].ctypes.data, c["cos"].ctypes.data
            M.mp_desc, M.mp_has_obs, M.n_cur = c["desc"].ctypes.data, c["obs"].ctypes.data, self.n_cur
            for name in ("cur_kps_un", "cur_u_right", "cur_desc", "cur_has_mp_obs", "scale_factors"):
                setattr(M, name, k[name].ctypes.data)
            P = self.PP[f]
            M.min_x, M.min_y, M.grid_w_inv, M.grid_h_inv = P.min_x, P.min_y, P.grid_w_inv, P.grid_h_inv
            M.n_levels, M.th, M.nn_ratio = P.n_levels, P.th, P.nn_ratio
            self.ptrs[f] = c["match"].ctypes.data
            self.hk.append((hkeep, c))
        self.host_match = [None] * B

    def device(self):
        rc = self.L.gfs_search_local_points(self.m.h, self.PP, self.B, self.RR)
        assert rc == 0, self.L.gfs_last_error()

    def host(self):
        for f in range(self.B):
            c = self.hk[f][1]
            self.MP[f].n_mp = self.R.lpr_frustum_compact(C.byref(self.PP[f]), C.byref(self.HR[f]), c["index"].ctypes.data, c["proj"].ctypes.data,
                                                         c["level"].ctypes.data, c["cos"].ctypes.data, c["desc"].ctypes.data, c["obs"].ctypes.data)
        rc = self.L.gfs_search_by_projection_map(self.m.h, self.MP, self.B, self.ptrs, C.c_void_p(self.nm.ctypes.data))
        assert rc == 0, self.L.gfs_last_error()
        for f in range(self.B):  # back to list indices
            c = self.hk[f][1]
            cm = c["match"]
            self.host_match[f] = np.where(cm >= 0, c["index"][np.maximum(cm, 0)], cm)

    def same(self):
        ok = True
        for f in range(self.B):
            dev = self.keeps[f]["cur_match"][:self.n_cur]
            ok &= bool(np.array_equal(dev, self.host_match[f])) and int(self.RR[f].nmatches) == int(self.nm[f])
            ok &= bool(np.array_equal(self.keeps[f]["in_view"][:self.n_mp], self.hk[f][0]["in_view"][:self.n_mp]))
        return ok


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
        res[wl["name"]] = dict(n_points=wl["n_points"], n_cur=j.n_cur, batch=j.B, n_to_match=int(j.RR[0].n_to_match),
                               n_searched=int(j.RR[0].n_searched), nmatches=int(j.RR[0].nmatches), calls=a.blocks * a.calls,
                               device_ms_median=med["device"], device_ms_p90=float(np.percentile(ts["device"], 90)),
                               host_path_ms_median=med["host"], host_path_ms_p90=float(np.percentile(ts["host"], 90)),
                               ratio_host_over_device=med["host"] / med["device"], ratio_per_block_min=min(ratios),
                               ratio_per_block_max=max(ratios), same_matches=bool(same))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loop", type=int, default=0, help="only run this many device calls of each workload")
    ap.add_argument("--step", default=None, choices=["measure"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.loop:
        for wl in WORKLOADS:
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
    out = dict(metric="search_local_points", latency="wall time of the synchronous call, alternating blocks in one process",
               workloads=json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
