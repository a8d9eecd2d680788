"""Frame-cloud timing (not bench.py).  Workloads: the depth map of synth.frame_pair(0, 640, 480) turned into a cloud on the device by
gfs_frame_rgbd at stride 4 (160 x 120, ~19 k points) and stride 3 (214 x 160, ~34 k points), shipped LidarParam defaults,
downsizeResolution 0.05.  Two ways to get mpPointCloud / mpPointCloudDownsampled, timed alternately in blocks in one process:

    device      the synchronous gfs_frame_cloud_extract_device call on the cloud already on the device (kernels, one read-back)
    host        the sequential restatement on one host thread for the host copy of the same cloud
                (tests/host/frame_cloud_restatement.cpp: a plain sequential filter over a cell map, NOT PCL's kd-tree filters)

Reports the median wall time of each over all calls, the per-block medians' ratio host / device (its minimum and maximum over the
blocks are the run-to-run spread), and checks that both give the same bits.  Prints one JSON line; --out writes it.

    python tools/bench_frame_cloud.py [--blocks 10] [--calls 20] [--out profiles/frame_cloud_bench.json]
    python tools/bench_frame_cloud.py --loop 30      # only device calls (for a kernel trace)
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
WORKLOADS = [dict(name="160x120_stride4", stride=4), dict(name="214x160_stride3", stride=3)]
STEP_TIMEOUT_S = 900


class Job:
    def __init__(self, wl):
        import frame_cloud_support as FCS
        from geoflowslam_amd import api, synth
        self.api, self.FCS = api, FCS
        depth = synth.frame_pair(0, 640, 480)["depth0"]
        fx, fy, cx, cy = (float(np.float32(v)) for v in synth.intrinsics(640, 480))
        self.frame = api.Frame(max_rows=480, max_cols=640, max_keypoints=16)
        _, _, host, (self.dc, self.dn, _, self.n) = self.frame.FrameRGBD(np.zeros(0, api.KP_DTYPE), depth, 40.0, wl["stride"], fx, fy, cx, cy)
        self.host_cloud = np.ascontiguousarray(host, np.float32)
        self.fc = api.FrameCloud(max_points=self.n)
        self.cloud, self.down = np.zeros((self.n, 3), np.float32), np.zeros((self.n, 3), np.float32)
        self.info = api.FrameCloudInfo()
        self.L, self.R = api.lib(), FCS.restatement()

    def device(self):
        rc = self.L.gfs_frame_cloud_extract_device(self.fc.h, C.c_void_p(self.dc), C.c_void_p(self.dn), self.cloud.ctypes.data, self.n,
                                                   self.down.ctypes.data, self.n, C.byref(self.info))
        assert rc == 0, self.L.gfs_last_error()

    def host(self):
        c = self.FCS.DEFAULTS
        rc = self.R.fcr_run(self.host_cloud.ctypes.data, self.n, c["horizontal_angle"], c["max_distance"], c["local_map_resolution"],
                            c["downsize_resolution"])
        assert rc == 0

    def same_bits(self):
        self.device()
        I = self.api.frame_cloud_info(self.info)
        ref = self.FCS.restate(self.host_cloud)
        return I == ref["info"] and self.FCS.same_bits(self.down[:I["n_down"]], ref["down"]) and \
            self.FCS.same_bits(self.cloud[:I["n_surf"] + I["n_edge"]], ref["cloud"])


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
        same = j.same_bits()
        ts = dict(device=[], host=[])
        ratios, blocks = [], []
        for _ in range(a.blocks):
            blk = {k: _timed(getattr(j, k), a.calls) for k in ("device", "host")}
            for k in ts:
                ts[k] += blk[k]
            blocks.append(dict(device_ms=float(np.median(blk["device"])), host_ms=float(np.median(blk["host"]))))
            ratios.append(blocks[-1]["host_ms"] / blocks[-1]["device_ms"])
        med = {k: float(np.median(v)) for k, v in ts.items()}
        I = j.api.frame_cloud_info(j.info)
        res[wl["name"]] = dict(stride=wl["stride"], info=I, calls=a.blocks * a.calls, device_ms_median=med["device"],
                               device_ms_p90=float(np.percentile(ts["device"], 90)),
                               device_ms_per_block_min=min(b["device_ms"] for b in blocks), device_ms_per_block_max=max(b["device_ms"] for b in blocks),
                               host_ms_median=med["host"], host_ms_per_block_min=min(b["host_ms"] for b in blocks),
                               host_ms_per_block_max=max(b["host_ms"] for b in blocks), ratio_host_over_device=med["host"] / med["device"],
                               ratio_per_block_min=min(ratios), ratio_per_block_max=max(ratios), same_bits=bool(same))
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
    out = dict(metric="frame_cloud_extract_device", latency="wall time of the synchronous call, alternating blocks in one process",
               host="sequential restatement on one thread (plain cell-map radius filter, not PCL)",
               workloads=json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
