"""GlobalBundleAdjustment timing (not bench.py).  synth.gba_map corridors of --keyframes key-frames with ~--points-per-kf points each,
10 iterations, robust.  For every map: the median wall time of the synchronous GlobalOptimizer.BundleAdjustment call (host
preparation, structure lists, copies, LM loop, read-back) over --calls calls after --warmup warm-up calls; the host time of the
structure lists alone (the same builder through its test hook); what gfs_gba_last_info reports; and, for maps of at most
--lba-max-keyframes key-frames, the same map through Optimizer.LocalBundleAdjustment (gfs_lba_solve, whose reduced solve runs on one
workgroup; the library's own entry, whose bits tests/test_gpu_gba.py pins to the commit before gfs_gba_solve), alternating with the new
entry call by call, with the two results compared under the bars of tests/test_gpu_lba.py.  The CPU oracle is timed where one solve
stays under --oracle-max-s seconds (estimated from the next smaller map; once a map is over, no larger one is tried).  Prints one JSON
line; --out writes it to a file.

    python tools/bench_gba.py [--keyframes 200,480,1000,2000] [--calls 20] [--lba-calls 20] [--out FILE]

The per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python tools/bench_gba.py
--keyframes 2000 --calls 2 --warmup 0 --lba-max-keyframes 0 --oracle-max-s 0` (kernel tracing only).  `--profile-db
DIR/.../NAME_results.db --out FILE` then adds it to FILE's result line without running anything on the GPU: ms per call of the Schur
assembly, the three factorisation kernels, the substitutions and everything else, and the trailing update's achieved FP64 rate
(n^3 / 3 flops a factorisation over its kernel time; MI355X_MICROARCH lists no FP64 matrix peak, so it is a rate, not a share of one).
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

GROUPS = dict(k_gba_assemble="schur_assembly", k_gba_diag="factor_diag", k_gba_panel="factor_panel", k_gba_trail="factor_trailing",
              k_gba_scale="substitutions", k_gba_back="substitutions")


def kernel_split(db, n_rows=None):
    """ms per profiled call (one k_lba_init each) of every group of kernels; the trials are the profiled run's own (its assemblies)"""
    import re
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    calls, per, launches, n_trials = 0, {}, 0, 0
    for name, start, end in rows:
        m = re.search(r"(kb?_\w+)", name)
        k = m.group(1) if m else name
        calls += k == "k_lba_init"
        n_trials += k == "k_gba_assemble"  # one assembly a trial
        launches += 1
        g = GROUPS.get(k, "everything_else")
        per[g] = per.get(g, 0.0) + (end - start) * 1e-6
    calls = max(calls, 1)
    out = dict(source="rocprofv3 --kernel-trace --stats, a separate run", profiled_calls=calls, launches_per_call=launches / calls,
               trials_per_call=n_trials / calls, kernel_ms_per_call={k: v / calls for k, v in sorted(per.items(), key=lambda kv: -kv[1])})
    if n_rows and n_trials and per.get("factor_trailing"):
        out["trailing_update_fp64_flops_per_s"] = (n_rows ** 3 / 3.0) * n_trials / (per["factor_trailing"] * 1e-3)
        out["trailing_update_rate_note"] = "n^3/3 flops a factorisation over the kernel's time; no FP64 matrix peak is documented: a rate, not a share of peak"
    return out


def _rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(np.asarray(b)), 1e-300))


def agree(w, r, ro):
    """the bars of tests/test_gpu_lba.py::test_solve_matches_oracle between two solutions -> (ok, figures)"""
    d = dict(iterations=(int(r["iterations_run"]), int(ro["iterations_run"])),
             pose_q=max(_rel(r["pose_q"][i], ro["pose_q"][i]) for i in range(w["n_poses"])),
             pose_t=max(_rel(r["pose_t"][i], ro["pose_t"][i]) for i in range(w["n_poses"])), points=_rel(r["points"], ro["points"]),
             final_chi2=_rel(r["final_chi2"], ro["final_chi2"]))
    thr = np.where(w["edge_stereo"] == 1, 7.815, 5.991)
    near = np.abs(ro["edge_chi2"] - thr) < 1e-4 * thr
    same_class = bool(((r["edge_chi2"] > thr) == (ro["edge_chi2"] > thr))[~near].all())
    ok = d["iterations"][0] == d["iterations"][1] and max(d["pose_q"], d["pose_t"], d["points"]) < 1e-5 and d["final_chi2"] < 1e-6 and same_class
    return bool(ok), dict(d, classification_equal=same_class)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="200,480,1000,2000")
    ap.add_argument("--points-per-kf", type=int, default=50)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lba-calls", type=int, default=20)
    ap.add_argument("--lba-max-keyframes", type=int, default=485)
    ap.add_argument("--oracle-max-s", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-db", default=None, help="add the per-kernel split of a rocprofv3 run to --out (no GPU run)")
    ap.add_argument("--profile-map", type=int, default=None, help="key-frames of the map the profiled run solved (default: the largest in --out)")
    a = ap.parse_args()
    if a.profile_db:
        out = json.load(open(a.out))
        maps = out["maps"]
        m = next((x for x in maps if x["keyframes"] == a.profile_map), maps[-1])
        m["kernel_split"] = kernel_split(a.profile_db, 6 * m["info"]["n_free"])
        line = json.dumps(out)
        print(line)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        return
    from geoflowslam_amd import api, synth
    from oracle import oracle as O
    sizes = [int(s) for s in a.keyframes.split(",")]
    results, oracle_s, oracle_over = [], 0.0, False
    for nk in sizes:
        print(f"# map of {nk} key-frames", file=sys.stderr, flush=True)
        w = synth.gba_map(nk, nk, nk * a.points_per_kf)
        t0 = time.perf_counter()
        L = api.gba_lists(w)
        lists_ms = (time.perf_counter() - t0) * 1e3
        gopt = api.GlobalOptimizer(max_poses=nk, max_points=int(w["n_points"]), max_edges=int(w["n_edges"]))
        lopt = api.Optimizer(max_poses=nk, max_points=int(w["n_points"]), max_edges=int(w["n_edges"])) if nk <= a.lba_max_keyframes else None
        for _ in range(a.warmup):
            gopt.BundleAdjustment(w)
            if lopt and a.lba_calls:
                lopt.LocalBundleAdjustment(w)
        tg, tl, r, rl = [], [], None, None
        print("# timing", file=sys.stderr, flush=True)
        for c in range(max(a.calls, a.lba_calls if lopt else 0)):  # alternating
            if c < a.calls:
                t0 = time.perf_counter()
                r = gopt.BundleAdjustment(w)
                tg.append((time.perf_counter() - t0) * 1e3)
            if lopt and c < a.lba_calls:
                t0 = time.perf_counter()
                rl = lopt.LocalBundleAdjustment(w)
                tl.append((time.perf_counter() - t0) * 1e3)
        info = gopt.last_info()
        m = dict(keyframes=nk, n_points=int(w["n_points"]), n_edges=int(w["n_edges"]), iterations_run=int(r["iterations_run"]), info=info,
                 launches_per_trial=info["launches"] / max(info["trials"], 1), gba_ms_median=float(np.median(tg)),
                 gba_ms_p90=float(np.percentile(tg, 90)), structure_lists_host_ms=lists_ms, calls=len(tg))
        if tl:
            ok, figs = agree(w, r, rl)
            m.update(lba_ms_median=float(np.median(tl)), lba_calls=len(tl), speedup_vs_lba=float(np.median(tl) / np.median(tg)),
                     agrees_with_lba=ok, agreement=figs)
        # the oracle's dense LDL^T is cubic in the free poses: estimate from the last measured size before starting a long one
        est = oracle_s * (nk / results[-1]["keyframes"]) ** 3 if results and oracle_s else 0.0
        if a.oracle_max_s > 0 and est < a.oracle_max_s and not oracle_over:
            print(f"# oracle on {nk} key-frames (estimate {est:.0f} s)", file=sys.stderr, flush=True)
            t0 = time.perf_counter()
            ro = O.lba_solve(w)
            oracle_s = time.perf_counter() - t0
            if oracle_s < a.oracle_max_s:
                ok, figs = agree(w, r, ro)
                m.update(cpu_oracle_ms=oracle_s * 1e3, agrees_with_oracle=ok, oracle_agreement=figs)
            else:
                oracle_over = True
        else:
            oracle_over = True  # (cubic: no larger map is tried either)
        results.append(m)
        print("# " + json.dumps(m), file=sys.stderr, flush=True)
        gopt.close()
        if lopt:
            lopt.close()
        del L
    out = dict(metric="gba", latency="wall time of the synchronous call", iterations=10, points_per_keyframe=a.points_per_kf, maps=results)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
