"""OptimizeEssentialGraph timing (not bench.py).  synth.pose_graph rings of --keyframes key-frames (fixed scale unless --free-scale,
20 iterations, the map's points moved along).  For every map: the median and the 90th percentile of the wall time of the synchronous
EssentialGraphOptimizer.OptimizeEssentialGraph call (structure lists, copies, LM loop with a host round trip per trial, read-back,
point correction) over --calls calls after --warmup warm-up calls, and what gfs_essential_graph_last_info reports.  Prints one JSON
line; --out writes it to a file.

    python tools/bench_essential_graph.py [--keyframes 200,480,1000,2000] [--calls 20] [--out FILE]

The per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python
tools/bench_essential_graph.py --keyframes 2000 --calls 2 --warmup 0` (kernel tracing only).  `--profile-db DIR/.../NAME_results.db
--out FILE` then adds it to FILE's result line without running anything on the GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = dict(k_eg_linearize="linearize", k_eg_assemble="assemble", k_gba_diag="factor_diag", k_gba_panel="factor_panel",
              k_gba_trail="factor_trailing", k_gba_scale="substitutions", k_gba_back="substitutions", k_eg_update="update_and_errors",
              k_eg_errors="update_and_errors", k_lba_decide="decide")


def kernel_split(db):
    """ms per profiled call (one k_eg_init each) of every group of kernels"""
    import re
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    calls, per, launches, trials = 0, {}, 0, 0
    for name, start, end in rows:
        m = re.search(r"(kb?_\w+)", name)
        k = m.group(1) if m else name
        calls += k == "k_eg_init"
        trials += k == "k_eg_assemble"
        launches += 1
        g = GROUPS.get(k, "everything_else")
        per[g] = per.get(g, 0.0) + (end - start) * 1e-6
    calls = max(calls, 1)
    return dict(source="rocprofv3 --kernel-trace --stats, a separate run", profiled_calls=calls, launches_per_call=launches / calls,
                trials_per_call=trials / calls, kernel_ms_per_call={k: v / calls for k, v in sorted(per.items(), key=lambda kv: -kv[1])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="200,480,1000,2000")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--free-scale", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-db", default=None, help="add the per-kernel split of a rocprofv3 run to --out (no GPU run)")
    ap.add_argument("--profile-map", type=int, default=None, help="key-frames of the map the profiled run solved (default: the largest in --out)")
    a = ap.parse_args()
    if a.profile_db:
        out = json.load(open(a.out))
        m = next((x for x in out["maps"] if x["keyframes"] == a.profile_map), out["maps"][-1])
        m["kernel_split"] = kernel_split(a.profile_db)
        line = json.dumps(out)
        print(line)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        return
    from geoflowslam_amd import api, synth
    results = []
    for nk in [int(s) for s in a.keyframes.split(",")]:
        print(f"# map of {nk} key-frames", file=sys.stderr, flush=True)
        p = synth.pose_graph(nk, nk, fix_scale=not a.free_scale, drift=0.05)
        opt = api.EssentialGraphOptimizer(max_vertices=nk, max_edges=len(p["edge_i"]), max_points=len(p["point_ref"]))
        for _ in range(a.warmup):
            opt.OptimizeEssentialGraph(p)
        t, r = [], None
        for _ in range(a.calls):
            t0 = time.perf_counter()
            r = opt.OptimizeEssentialGraph(p)
            t.append((time.perf_counter() - t0) * 1e3)
        info = opt.last_info()
        m = dict(keyframes=nk, n_edges=len(p["edge_i"]), n_points=len(p["point_ref"]), fix_scale=bool(p["fix_scale"]),
                 iterations_run=int(r["iterations_run"]), final_chi2=float(r["final_chi2"]), info=info, ms_median=float(np.median(t)),
                 ms_p90=float(np.percentile(t, 90)), ms_per_trial=float(np.median(t)) / max(info["trials"], 1), calls=len(t))
        results.append(m)
        print("# " + json.dumps(m), file=sys.stderr, flush=True)
        opt.close()
    out = dict(metric="essential_graph", latency="wall time of the synchronous call", iterations=20, maps=results)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
