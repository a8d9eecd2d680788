"""CLAHE timing (not bench.py).  VGA frames (synth.clahe_image), B = 1 and B = 64, 8 x 8 tiles, clip limit 3.0, optical-flow window 35.
Timed alternately in blocks in one process:

    apply           the synchronous gfs_clahe_apply (staging, upload, k_clahe_lut, k_clahe_interp, download)
    build_clahe     gfs_klt_build_pyramid_clahe: one upload, CLAHE, the pyramid, no download of the equalised image
    build_plain     gfs_klt_build_pyramid on the same frames: what a build costs without CLAHE (the call is unchanged by CLAHE)
    host_route      the route without the device CLAHE: the sequential restatement of the rule on one host thread
                    (tests/host/clahe_restatement.cpp; cv::CLAHE itself is not available to time), then gfs_klt_build_pyramid

and, on device-resident frames, the device time of gfs_clahe_apply_device between two events on its stream, with the per-kernel
times of the library's profiler.  Reports medians and p90 over all calls, the per-block ratios' minimum and maximum as the
run-to-run spread, and checks that both routes give the same pyramid bytes.  Prints one JSON line; --out writes it.

    python tools/bench_clahe.py [--blocks 10] [--calls 20] [--out profiles/clahe_bench.json]
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
W, H, WIN = 640, 480, 35
BATCHES = (1, 64)
STEP_TIMEOUT_S = 900


class Job:
    def __init__(self, B):
        import clahe_support as CS
        from geoflowslam_amd import api, synth
        self.B, self.api, self.L, self.R = B, api, api.lib(), CS.restatement()
        self.imgs = [synth.clahe_image(100 + f, W, H) for f in range(B)]
        self.out = [np.empty_like(im) for im in self.imgs]
        self.eq = [np.empty_like(im) for im in self.imgs]
        self.luts = np.zeros((8, 8, 256), np.uint8)
        self.cl = api.Clahe(W, H, max_batch=B)
        self.trk = api.KltTracker(W, H, WIN, max_batch=B, max_points=16)
        self.pyr_a, self.pyr_b = api.KltPyramid(self.trk), api.KltPyramid(self.trk)
        arr = lambda xs: (C.c_void_p * B)(*[x.ctypes.data for x in xs])
        self.ip, self.op, self.ep = arr(self.imgs), arr(self.out), arr(self.eq)

    def apply(self):
        assert self.L.gfs_clahe_apply(self.cl.h, self.ip, W, H, W, self.B, self.op, W) == 0

    def build_clahe(self):
        assert self.L.gfs_klt_build_pyramid_clahe(self.trk.h, self.cl.h, self.pyr_a.h, self.ip, W, self.B, None, 0) == 0

    def build_plain(self):
        assert self.L.gfs_klt_build_pyramid(self.trk.h, self.pyr_b.h, self.ip, W, self.B) == 0

    def host_route(self):
        for im, e in zip(self.imgs, self.eq):
            assert self.R.cr_clahe(im.ctypes.data, W, H, W, 3.0, 8, 8, 0, e.ctypes.data, W, self.luts.ctypes.data, None, None, None) == 0
        assert self.L.gfs_klt_build_pyramid(self.trk.h, self.pyr_b.h, self.ep, W, self.B) == 0

    def same(self):
        self.build_clahe()
        self.host_route()
        return all(a.tobytes() == b.tobytes() for f in range(self.B) for a, b in zip(self.pyr_a.download(f), self.pyr_b.download(f)))

    def device_times(self, calls):
        """-> (median ms between two events around one gfs_clahe_apply_device, {kernel: mean ms per launch})."""
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        src = np.stack(self.imgs)
        d_in, d_out, st = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(d_in), src.nbytes) == 0 and hip.hipMalloc(C.byref(d_out), src.nbytes) == 0
        assert hip.hipMemcpy(d_in, src.ctypes.data, src.nbytes, 1) == 0 and hip.hipStreamCreate(C.byref(st)) == 0
        tm, ts = self.api.Timer(), []
        for k in range(calls + 5):
            tm.start(st.value)
            self.cl.apply_device(d_in.value, W, H, W, self.B, d_out.value, W, stream=st.value)
            tm.stop(st.value)
            if k >= 5:
                ts.append(tm.elapsed_ms())
        self.api.profile_enable(True)
        self.api.profile_reset()
        for _ in range(calls):
            self.cl.apply_device(d_in.value, W, H, W, self.B, d_out.value, W, stream=st.value)
        assert hip.hipStreamSynchronize(st) == 0
        rep = {k: t / max(c, 1) for k, (t, c) in self.api.profile_report().items()}
        self.api.profile_enable(False)
        got = np.empty_like(src)
        assert hip.hipMemcpy(got.ctypes.data, d_out, src.nbytes, 2) == 0
        self.apply()
        assert all(got[f].tobytes() == self.out[f].tobytes() for f in range(self.B))
        hip.hipFree(d_in)
        hip.hipFree(d_out)
        return float(np.median(ts)), rep


def _timed(fn, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def step_measure(a):
    res = {}
    keys = ("apply", "build_clahe", "build_plain", "host_route")
    for B in BATCHES:
        j = Job(B)
        for k in keys:
            for _ in range(3):
                getattr(j, k)()
        same = j.same()
        ts = {k: [] for k in keys}
        r_plain, r_host = [], []
        host_calls = a.calls if B == 1 else max(a.calls // 10, 2)  # B = 64 on one host thread takes tens of milliseconds a call
        for _ in range(a.blocks):
            blk = {k: _timed(getattr(j, k), host_calls if k == "host_route" else a.calls) for k in keys}
            for k in keys:
                ts[k] += blk[k]
            r_plain.append(float(np.median(blk["build_clahe"]) / np.median(blk["build_plain"])))
            r_host.append(float(np.median(blk["host_route"]) / np.median(blk["build_clahe"])))
        dev_ms, rep = j.device_times(a.blocks * a.calls)
        out = dict(frames=B, width=W, height=H, window=WIN, calls=a.blocks * a.calls, same_pyramids=bool(same and j.same()),
                   apply_device_ms_median=dev_ms, kernels_ms_per_launch=rep)
        for k in keys:
            out[k + "_ms_median"], out[k + "_ms_p90"] = float(np.median(ts[k])), float(np.percentile(ts[k], 90))
        out.update(ratio_build_clahe_over_plain=out["build_clahe_ms_median"] / out["build_plain_ms_median"],
                   ratio_build_clahe_over_plain_per_block=[min(r_plain), max(r_plain)],
                   ratio_host_route_over_build_clahe=out["host_route_ms_median"] / out["build_clahe_ms_median"],
                   ratio_host_route_over_build_clahe_per_block=[min(r_host), max(r_host)],
                   fused_build_won=bool(min(r_host) > 1.0), fused_build_lost=bool(max(r_host) < 1.0))
        res[f"vga_x{B}"] = out
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=["measure"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:  # child
        print(json.dumps(step_measure(a)))
        return
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "measure", "--blocks", str(a.blocks), "--calls", str(a.calls)],
                       capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    if r.returncode != 0:
        sys.stderr.write(r.stdout + r.stderr)
        raise SystemExit(f"the measurement failed with exit status {r.returncode}")
    out = dict(metric="clahe", latency="wall time of the synchronous calls, alternating blocks in one process; device time between HIP events",
               workloads=json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
