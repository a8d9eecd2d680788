"""Timing of PoseLidarVisualInertialOptimization, the pose step that ends TrackLocalMap with point-cloud observations (not bench.py).
Workloads: synth.pose_lidar_inertial_problem at 640 x 480 with 300 visual edges, a 3 000-point cloud, 4 rounds and a local map of 3
key-frame renders voxel-averaged at --voxel metres (0.04 m, the voxel of DESIGN.md section 9's figure: 12 000 - 28 000 map points) -- one
problem in key-frame mode (kf_b1), one in frame mode (fr_b1), and a batch of 16 with the modes alternating, each problem with its
own scene and map (mixed_b16).  Three paths, timed alternately in blocks in one process after a warm-up:

    device      the synchronous gfs_pose_lidar_inertial_optimize call (staging, one upload, 2 + 2 x 4 launches, one download)
    host        the sequential restatement on ONE host thread (tests/host/pose_lidar_inertial_restatement.cpp), which returns the same
                bytes.  It is NOT g2o, and its 5-NN is a brute force over the whole map where the reference has a k-d tree: this says
                nothing about the reference's own time.  It is slow, so it runs --host-calls times a block
    halves      gfs_pose_inertial_optimize plus gfs_pose_lidar_optimize (4 rounds) on the same visual edges, cloud and map from the
                same start: a floor for what the two halves cost apart (they solve other problems and return other numbers)

Reports the median and p90 wall time of each over all calls, the ratios of the medians with the minimum and maximum of the per-block
ratios, and checks that device and host return the same bytes.  Prints one JSON line; --out writes it.

    python tools/bench_pose_lidar_inertial.py [--blocks 5] [--calls 20] [--host-calls 2] [--out profiles/pose_lidar_inertial_bench.json]
    python tools/bench_pose_lidar_inertial.py --loop 30 [--only kf_b1]     # only device calls (for a kernel trace)
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
N_OBS, N_CLOUD, ROUNDS = 300, 3000, 4
WORKLOADS = [dict(name="kf_b1", modes=[0]), dict(name="fr_b1", modes=[1]), dict(name="mixed_b16", modes=[k % 2 for k in range(16)])]


class Job:
    def __init__(self, wl, voxel):
        import pose_lidar_inertial_support as S
        from geoflowslam_amd import api, synth
        self.S, self.api, self.B = S, api, len(wl["modes"])
        self.probs = [synth.pose_lidar_inertial_problem(800 + 7 * f, m, n_obs=N_OBS, n_cloud=N_CLOUD, voxel=voxel, width=640, height=480,
                                                        outlier_share=0.15, n_rounds=ROUNDS) for f, m in enumerate(wl["modes"])]
        self.map_xyz = [np.ascontiguousarray(p["map_xyz"], np.float32) for p in self.probs]
        self.maps = [api.LidarMap(max_points=len(m)).set(m) for m in self.map_xyz]
        self.opt = api.PoseLidarInertialOptimizer(max_obs=N_OBS, max_cloud=N_CLOUD, max_batch=self.B)
        self.pio = api.PoseInertialOptimizer(max_obs=N_OBS, max_batch=self.B)
        self.plo = api.PoseLidarOptimizer(max_obs=N_OBS, max_cloud=N_CLOUD, max_batch=self.B)
        self.L, self.R = api.lib(), S.restatement()
        self.sets = []
        for _ in range(2):  # device, host: their own structs and output arrays
            PP, SS, keeps = (api.PoseLidarInertialProblem * self.B)(), (api.PoseLidarInertialSolution * self.B)(), []
            for f, p in enumerate(self.probs):
                P, Sl, keep, n = api.pose_lidar_inertial_structs(p, self.maps[f].h)
                PP[f], SS[f] = P, Sl
                keeps.append((keep, n, P.vi.mode))
            self.sets.append((PP, SS, keeps))
        self.map_ptrs = (C.c_void_p * self.B)(*[m.ctypes.data for m in self.map_xyz])
        self.map_n = np.array([len(m) for m in self.map_xyz], np.int32)
        # the two halves apart
        self.IP, self.IS, self.ikeep = (api.PoseInertialProblem * self.B)(), (api.PoseInertialSolution * self.B)(), []
        self.LP, self.LS, self.lkeep = (api.PoseLidarProblem * self.B)(), (api.PoseLidarSolution * self.B)(), []
        for f, p in enumerate(self.probs):
            P, Sl, keep, n = api.pose_inertial_structs(p)
            self.IP[f], self.IS[f] = P, Sl
            self.ikeep.append(keep)
            P, Sl, keep, n = api.pose_lidar_structs(dict(q=p["q"], t=p["t"], xw=p["xw"], obs=p["obs"], inv_sigma2=p["inv_sigma2"], stereo=p["stereo"],
                                                         fx=p["fx"], fy=p["fy"], cx=p["cx"], cy=p["cy"], bf=p["bf"], cloud=p["cloud"],
                                                         n_iterations=ROUNDS), self.maps[f].h)
            self.LP[f], self.LS[f] = P, Sl
            self.lkeep.append(keep)

    def device(self):
        PP, SS, _ = self.sets[0]
        rc = self.L.gfs_pose_lidar_inertial_optimize(self.opt.h, PP, self.B, SS)
        assert rc == 0, self.L.gfs_last_error()

    def host(self):
        PP, SS, _ = self.sets[1]
        rc = self.R.plir_optimize_batch(C.cast(PP, C.c_void_p), C.cast(self.map_ptrs, C.c_void_p), self.map_n.ctypes.data, self.B, C.cast(SS, C.c_void_p))
        assert rc == 0, rc

    def halves(self):
        rc = self.L.gfs_pose_inertial_optimize(self.pio.h, self.IP, self.B, self.IS)
        assert rc == 0, self.L.gfs_last_error()
        rc = self.L.gfs_pose_lidar_optimize(self.plo.h, self.LP, self.B, self.LS)
        assert rc == 0, self.L.gfs_last_error()

    def results(self, which):
        _, SS, keeps = self.sets[which]
        return [self.api.pose_lidar_inertial_result(SS[f], *keeps[f]) for f in range(self.B)]

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
        j = Job(wl, a.voxel)
        j.host()
        for _ in range(5):  # warm-up
            j.device()
            j.halves()
        same = j.same()
        ts, r_host, r_halves = dict(device=[], host=[], halves=[]), [], []
        for _ in range(a.blocks):
            blk = dict(device=_timed(j.device, a.calls), host=_timed(j.host, a.host_calls), halves=_timed(j.halves, a.calls))
            for k in ts:
                ts[k] += blk[k]
            r_host.append(float(np.median(blk["host"]) / np.median(blk["device"])))
            r_halves.append(float(np.median(blk["device"]) / np.median(blk["halves"])))
        same = same and j.same()
        med = {k: float(np.median(v)) for k, v in ts.items()}
        r = j.results(0)
        res[wl["name"]] = dict(n_obs=N_OBS, n_cloud=N_CLOUD, map_points=[int(v) for v in j.map_n], batch=j.B, modes=wl["modes"],
                               n_good=[x["n_good"] for x in r], round_edges=[x["round_edges"] for x in r], rounds_run=[x["rounds_run"] for x in r],
                               device_calls=a.blocks * a.calls, host_calls=a.blocks * a.host_calls, device_ms_median=med["device"],
                               device_ms_p90=float(np.percentile(ts["device"], 90)), device_ms_min=float(np.min(ts["device"])),
                               host_restatement_ms_median=med["host"], host_restatement_ms_max=float(np.max(ts["host"])),
                               halves_apart_ms_median=med["halves"], halves_apart_ms_p90=float(np.percentile(ts["halves"], 90)),
                               ratio_host_over_device=med["host"] / med["device"], ratio_host_over_device_per_block=[min(r_host), max(r_host)],
                               ratio_device_over_halves=med["device"] / med["halves"], ratio_device_over_halves_per_block=[min(r_halves), max(r_halves)],
                               same_results=bool(same))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=2)
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loop", type=int, default=0, help="only run this many device calls of each workload")
    ap.add_argument("--only", default=None, help="this workload alone")
    a = ap.parse_args()
    if a.loop:
        for wl in WORKLOADS:
            if a.only and wl["name"] != a.only:
                continue
            j = Job(wl, a.voxel)
            for _ in range(a.loop):
                j.device()
        return
    out = dict(metric="pose_lidar_inertial", latency="wall time of the synchronous call, alternating blocks in one process",
               host_path="the sequential restatement on one host thread with a brute-force 5-NN, not g2o", voxel=a.voxel, workloads=measure(a))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
