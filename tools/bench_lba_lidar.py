"""LocalVisualLidarBA timing (not bench.py).  One bench-size window: synth.lba_lidar_window with 20 free + 5 fixed key-frames, 3 000
landmarks, every other local key-frame with lidar edges, ~3 000 cloud points each and a local map voxel-averaged at --voxel metres.
Reports the median wall time of the synchronous call (host packing, copies, association, LM loop, read-back) over --calls calls after
warm-up, the same window through gfs_lba_solve without lidar edges, and the sequential CPU restatement's single-thread time.  Prints
one JSON line; --out writes it to a file.

    python tools/bench_lba_lidar.py [--calls 100] [--cpu-calls 3] [--voxel 0.04] [--out FILE]

The per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_lba_lidar.py
--calls 20 --cpu-calls 0` (kernel tracing only).  `--profile-db DIR/.../NAME_results.db --out FILE` then adds it to FILE's result line
(the kernels of the lidar calls, which come first, per call), without running anything on the GPU.
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


def kernel_split(db):
    """ms per lidar call of every kernel of the profiled run: its calls up to the first plain LBA call (k_lba_init without a
    k_lba_lidar_assoc before it)"""
    import re
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    calls, per, seen_assoc = 0, {}, False
    for name, start, end in rows:
        m = re.search(r"(k_\w+)", name)
        k = m.group(1) if m else name
        if k == "k_lba_lidar_assoc":
            seen_assoc = True
            calls += 1
        elif k == "k_lba_init" and not seen_assoc:
            break  # the first call without an association: the plain-LBA part of the run
        elif k == "k_lba_init":
            seen_assoc = False
        per[k] = per.get(k, 0.0) + (end - start) * 1e-6
    split = {k: v / calls for k, v in sorted(per.items(), key=lambda kv: -kv[1])}
    lm = sum(v for k, v in split.items() if k not in ("k_lba_lidar_assoc", "k_lba_lidar_compact"))
    return dict(source="rocprofv3 --kernel-trace --stats, a separate run", lidar_calls=calls, kernel_ms_per_call=split,
                association_ms=split.get("k_lba_lidar_assoc", 0.0) + split.get("k_lba_lidar_compact", 0.0), lm_phases_ms=lm)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--cpu-calls", type=int, default=3)
    ap.add_argument("--voxel", type=float, default=0.04)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-db", default=None, help="add the per-kernel split of a rocprofv3 run to --out (no GPU run)")
    a = ap.parse_args()
    if a.profile_db:
        out = json.load(open(a.out))
        out["kernel_split"] = kernel_split(a.profile_db)
        line = json.dumps(out)
        print(line)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        return
    from geoflowslam_amd import api, synth
    import lba_lidar_support as LLS
    w = synth.lba_lidar_window(0, n_free=20, n_fixed=5, n_points=3000, n_cloud=3000, voxel=a.voxel, width=320, height=240)
    m = api.LidarMap(max_points=len(w["map_xyz"])).set(w["map_xyz"])
    opt = api.Optimizer(max_poses=32, max_points=4096, max_edges=200000)

    def timed(fn, n):
        for _ in range(5):
            fn()
        t = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t)), float(np.percentile(t, 90))

    r = opt.LocalVisualLidarBA(w, m)
    lid = timed(lambda: opt.LocalVisualLidarBA(w, m), a.calls)
    plain = timed(lambda: opt.LocalBundleAdjustment(w), a.calls)
    cpu = []
    for _ in range(a.cpu_calls):
        t0 = time.perf_counter()
        LLS.solve(w)
        cpu.append((time.perf_counter() - t0) * 1e3)
    out = dict(metric="lba_lidar", n_free=20, n_fixed=5, n_points=3000, n_edges=int(w["n_edges"]), voxel=a.voxel,
               n_map=int(len(w["map_xyz"])), lidar_keyframes=int((r["pose_lidar_edges"] > 0).sum()),
               lidar_edges=int(r["pose_lidar_edges"].sum()), cloud_points_per_kf=3000, iterations_run=int(r["iterations_run"]),
               latency="wall time of the synchronous call", lidar_ms_median=lid[0], lidar_ms_p90=lid[1], lba_no_lidar_ms_median=plain[0],
               lba_no_lidar_ms_p90=plain[1], cpu_restatement_ms_median=float(np.median(cpu)),
               speedup_vs_cpu_restatement=float(np.median(cpu)) / lid[0])
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
