"""PoseLidarVisualOptimization timing (not bench.py).  Scenes: synth.pose_lidar_frame at 640 x 480 with 600 observations, ~3 000 cloud
points, 3 rounds, and a local map of 3 key-frame renders voxel-averaged at --voxel metres (0.04 m: ~20 000 map points, the size of
the g1 configuration's local map; its cells are as full as that map's).  Reports, per sum mode, the one-frame latency as the wall
time of the synchronous call (host packing, copies, the kernels, read-back; median and p90 of --frames calls) and frames/s at
B = 64, and the sequential CPU restatement's single-thread time on the same frames.  Every step runs in a child process under its
own time limit.  Prints one JSON line; --out writes it to a file.

    python tools/bench_pose_lidar.py [--frames 200] [--cpu-frames 5] [--voxel 0.04] [--out FILE]
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
STEP_TIMEOUT_S = {"edge_order": 600, "tree": 600, "cpu": 900}


def scenes(a):
    from geoflowslam_amd import synth
    return [synth.pose_lidar_frame(s, n_obs=600, n_cloud=3000, width=640, height=480, voxel=a.voxel, n_iterations=3)
            for s in range(a.scenes)]


def step_gpu(a, mode):
    from geoflowslam_amd import api
    sc = scenes(a)
    maps = [api.LidarMap(max_points=len(f["map_xyz"])).set(f["map_xyz"]) for f in sc]
    for f, m in zip(sc, maps):
        f["map"] = m
    opt = api.PoseLidarOptimizer(max_obs=1024, max_cloud=4096, max_batch=64, sums=mode)
    for f in sc[:3]:
        opt.PoseLidarVisualOptimization(f)  # warm-up
    wall = []
    for i in range(a.frames):
        f = sc[i % len(sc)]
        t0 = time.perf_counter()
        opt.PoseLidarVisualOptimization(f)
        wall.append((time.perf_counter() - t0) * 1e3)
    batch = [sc[i % len(sc)] for i in range(64)]
    opt.PoseLidarVisualOptimization(batch)
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        opt.PoseLidarVisualOptimization(batch)
    fps = 64 * reps / (time.perf_counter() - t0)
    return dict(latency_ms_median=float(np.median(wall)), latency_ms_p90=float(np.percentile(wall, 90)), frames_per_s_B64=fps,
                n_map=int(np.mean([len(f["map_xyz"]) for f in sc])), n_cloud=int(np.mean([len(f["cloud"]) for f in sc])))


def step_cpu(a):
    import pose_lidar_support as PLS
    sc = scenes(a)
    cpu = []
    for i in range(a.cpu_frames):
        t0 = time.perf_counter()
        PLS.run(sc[i % len(sc)])
        cpu.append((time.perf_counter() - t0) * 1e3)
    return dict(cpu_restatement_ms_median=float(np.median(cpu)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--cpu-frames", type=int, default=5)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, choices=sorted(STEP_TIMEOUT_S), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:  # child
        print(json.dumps(step_cpu(a) if a.step == "cpu" else step_gpu(a, a.step)))
        return
    out = dict(metric="pose_lidar", n_obs=600, rounds=3, voxel=a.voxel, latency="wall time of the synchronous call")
    args = ["--frames", str(a.frames), "--cpu-frames", str(a.cpu_frames), "--scenes", str(a.scenes), "--voxel", str(a.voxel)]
    for step in ("edge_order", "tree", "cpu"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step] + args, capture_output=True, text=True,
                           timeout=STEP_TIMEOUT_S[step])
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"step {step} failed with exit status {r.returncode}")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        if step == "cpu":
            out.update(res)
        else:
            out["n_map"], out["n_cloud"] = res.pop("n_map"), res.pop("n_cloud")
            out[step] = res
    out["speedup_edge_order"] = out["cpu_restatement_ms_median"] / out["edge_order"]["latency_ms_median"]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
