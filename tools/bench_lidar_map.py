"""Lidar local-map build timing (not bench.py).  Workloads: synth.lidar_map_window key-frames of ~3 000 points each,
25 key-frames at 0.04 m (the scale of profiles/lba_lidar_bench.json's map) and 30 key-frames at 0.1 m (the shipped
LidarMapping.LocalResolution).  Three ways to get the same gfs_lidar_map, timed alternately in blocks in one process:

    device      the synchronous gfs_lidar_map_build call (staging, upload, kernels, the read-back of the control block)
    host        what there was before it: the sequential restatement's transform + voxel filter on one host thread
                (tests/host/lidar_map_restatement.cpp), then gfs_lidar_map_set of its output
    set_only    gfs_lidar_map_set alone, for scale

Reports the median wall time of each over all calls, the per-block medians' ratio host / device (its minimum and maximum over the
blocks are the run-to-run spread), and checks that the two maps hold the same bits.  Prints one JSON line; --out writes it.

    python tools/bench_lidar_map.py [--blocks 10] [--calls 20] [--out profiles/lidar_map_bench.json]
    python tools/bench_lidar_map.py --loop 50      # only device builds (for a kernel trace)
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
WORKLOADS = [dict(name="25kf_0.04m", n_keyframes=25, leaf=0.04), dict(name="30kf_0.1m", n_keyframes=30, leaf=0.1)]
STEP_TIMEOUT_S = 900


class Job:
    def __init__(self, wl):
        import lidar_map_support as LMS
        from geoflowslam_amd import api, synth
        self.api, self.LMS, self.leaf = api, LMS, float(np.float32(wl["leaf"]))
        w = synth.lidar_map_window(0, n_keyframes=wl["n_keyframes"], n_cloud=3000, width=160, height=120)
        self.q, self.t, self.cb, self.cloud = LMS._inputs(w)
        self.n = len(self.cloud)
        self.mapper = api.LidarMapper(self.n, wl["n_keyframes"])
        self.map_dev, self.map_host = api.LidarMap(max_points=self.n), api.LidarMap(max_points=self.n)
        self.inp = api.LidarMapInput(len(self.q), self.q.ctypes.data, self.t.ctypes.data, self.cb.ctypes.data, self.cloud.ctypes.data, self.leaf)
        self.info = api.LidarMapInfo()
        self.out = np.zeros((self.n, 3), np.float32)
        self.rinfo = np.zeros(6, np.int32)
        self.L, self.R = api.lib(), LMS.restatement()

    def device(self):
        rc = self.L.gfs_lidar_map_build(self.mapper.h, C.byref(self.inp), self.map_dev.h, C.byref(self.info))
        assert rc == 0, self.L.gfs_last_error()

    def host(self):
        rc = self.R.lmr_build(len(self.q), self.q.ctypes.data, self.t.ctypes.data, self.cb.ctypes.data, self.cloud.ctypes.data, self.leaf,
                              self.out.ctypes.data, self.n, self.rinfo.ctypes.data)
        assert rc == 0
        self.set_only()

    def set_only(self):
        rc = self.L.gfs_lidar_map_set(self.map_host.h, C.c_void_p(self.out.ctypes.data), int(self.rinfo[1]))
        assert rc == 0, self.L.gfs_last_error()


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
        same = j.LMS.same_grid(j.LMS.grid(j.api, j.map_dev), j.LMS.grid(j.api, j.map_host))
        ts = dict(device=[], host=[], set_only=[])
        ratios = []
        for _ in range(a.blocks):
            blk = {k: _timed(getattr(j, k), a.calls) for k in ("device", "host", "set_only")}
            for k in ts:
                ts[k] += blk[k]
            ratios.append(float(np.median(blk["host"]) / np.median(blk["device"])))
        med = {k: float(np.median(v)) for k, v in ts.items()}
        res[wl["name"]] = dict(n_keyframes=wl["n_keyframes"], leaf=wl["leaf"], n_in=j.n, n_out=int(j.info.n_out), calls=a.blocks * a.calls,
                               device_build_ms_median=med["device"], device_build_ms_p90=float(np.percentile(ts["device"], 90)),
                               host_path_ms_median=med["host"], set_only_ms_median=med["set_only"],
                               ratio_host_over_device=med["host"] / med["device"], ratio_per_block_min=min(ratios),
                               ratio_per_block_max=max(ratios), same_map_bits=bool(same))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loop", type=int, default=0, help="only run this many device builds of each workload")
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
    out = dict(metric="lidar_map_build", latency="wall time of the synchronous call, alternating blocks in one process",
               workloads=json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
