"""The library used the way the SLAM process uses it: Tracking, LocalMapping and LoopClosing as host threads with handles of their own,
a fourth thread whose GICP handle contends with Tracking's for the cooperative workgroup budget, and two threads on ONE handle.  Run
as a program it is the child of tests/test_gpu_concurrent_handles.py: a FRESH process, so that what the library does once per process
(the LDS-limit raises behind lba_host.hpp / gba_host.hpp's `static bool done[64]`, the first use of every kernel) happens while the
threads race for it.

Every thread creates its handles after a common barrier, runs its script R times and keeps the bytes of every output.  After the
threads the same scripts run once more, one after the other on the main thread, and every kept output is compared with those bytes:
the inputs are the smallest ones of each feature's own test file, where that serial call is held to its oracle or restatement.  (The
serial pass comes AFTER the threads, not before them: ahead of them it would do the once-per-process work alone.)  A thread also
checks after each call that its thread-local gfs_last_error() text is still its own; the fourth thread makes one refused call a round
and checks its code and text.  While the four threads run, all but COOP_FREE workgroups of the cooperative GICP budget are held
through the test hook, so that the two GICP handles meet in it (partial grants and refusals, as they come).  No call is repeated on a
mismatch; the child runs once.

stdout: one JSON line per thread -- thread, rounds, mismatches [[thread, round, call, output key], ...], errors -- and one for the run
(R, seconds of the threaded parts, how the two GICP handles' calls were driven).  Not a test module."""
import json
import sys
import threading
import time
import traceback

import numpy as np

R = 200  # ~2 s of threads on an MI355X
GFS_ERR_CAPACITY = -4  # include/gfs_abi.h
# Workgroups of the cooperative GICP budget left free while the four threads run (the rest is held through the test hook, as a third
# handle's launch would hold it): the two GICP handles want 20 (at least 10) and 80 (at least 40), so whichever comes second while
# the other's kernel is in flight gets 65 of 80 -- below the 66 chunks of its cloud: one workgroup serves two -- or 5 of 20, a refusal
# and the launch-per-step rounds.  With the whole budget free (512 on an MI355X) the two would never meet.
COOP_FREE = 85


def flatten(out, prefix="", acc=None):
    """A call's output (arrays, numbers, None, in dicts / lists / tuples) -> {key path: bytes with dtype and shape}"""
    acc = {} if acc is None else acc
    if isinstance(out, dict):
        for k in sorted(out):
            flatten(out[k], f"{prefix}/{k}", acc)
    elif isinstance(out, (list, tuple)):
        for i, v in enumerate(out):
            flatten(v, f"{prefix}[{i}]", acc)
    elif out is None:
        acc[prefix] = b"None"
    elif isinstance(out, (bytes, str)):
        acc[prefix] = out if isinstance(out, bytes) else out.encode()
    else:
        a = np.ascontiguousarray(out)
        assert a.dtype != object, (prefix, type(out))
        acc[prefix] = f"{a.dtype.str}{a.shape}".encode() + a.tobytes()
    return acc


# ---------------------------------------------------------------- inputs (built once, on the main thread, never modified)

def inputs():
    import bow_search_support as BS
    import fuse_support as FS
    import gba_support as G
    import local_points_support as LPS
    import map_point_support as MS
    import pose_graph_support as PG
    import sim3_opt_support as S3
    import sim3_search_support as SS
    import triangulate_support as TS
    from geoflowslam_amd import synth
    I = {}
    fp = synth.frame_pair(77, 160, 120, 2)  # (the frames of tests/golden/orb_160x120.npz)
    I["gray"] = (fp["gray0"], fp["gray1"])
    I["klt"] = [synth.klt_texture_pair(s, 160, 120, shift=sh)[:2] for s, sh in ((3, (1.0, 0.5)), (4, (-0.7, 1.2)))]
    rng = np.random.default_rng(0)
    I["klt_pts"] = [np.stack([rng.uniform(12, 148, 24), rng.uniform(12, 108, 24)], 1).astype(np.float32) for _ in range(2)]
    I["fmat"] = synth.two_view_points(41, 60, 0.2)[:2]
    I["sbp"] = synth.sbp_pair(80, n_points=65, n_extra_cur=40)
    I["local"] = [LPS.frame(64, 63)[0], LPS.frame(65, 65)[0]]
    I["pose"] = synth.pose_frame(3, n_obs=60)
    small, big = synth.frame_pair(301, 160, 120, stride=2), synth.frame_pair(300, 160, 120, stride=1)
    I["cloud5120"] = (small["cloud0"], small["cloud1"])
    I["cloud20480"] = (big["cloud0"], big["cloud1"])
    I["too_many"] = np.zeros((20481, 4), np.float32)
    I["lba"] = synth.lba_window(1, n_free=4, n_fixed=2, n_points=120)
    I["fuse"] = [FS.problem(63, 65, n_keyframes=2)[0], FS.problem(65, 64, n_keyframes=1)[0]]
    I["tri"] = TS.problem(65, 63, n_neighbours=2)[0]
    I["map_points"] = MS.sized(64)[0]
    I["bow"] = BS.problem(41, 65, 63, n_kf2=2, n_nodes=3)[0]
    I["ransac"] = [synth.sim3_ransac_problem(s, n_pairs=64, inlier_share=0.6, fix_scale=bool(s % 2)) for s in (3, 4)]
    I["sim3_search"] = SS.problem(SS.SBP, 65, 64)[0]
    I["sim3_opt"] = S3.sized_problem(64, True)
    I["essential_graph"] = PG.map_problem("ring10_fixed")
    I["gba"] = G.gmap(2, 76, 502)  # gba_support.size_cases' "F2"
    I["desc"] = [rng.integers(0, 256, (n, 32)).astype(np.uint8) for n in (200, 190, 130, 257)]
    return I


# ---------------------------------------------------------------- the threads' scripts: (A, I, shared handles) -> (calls, handles to close)

def _klt_call(trk, imgs, pts):
    def call():
        p0, p1 = trk.buildOpticalFlowPyramid(imgs[0]), trk.buildOpticalFlowPyramid(imgs[1])
        out = trk.fbKltTracking(p0, p1, 3, 15.0, 0.5, pts, pts.copy())
        p0.close()
        p1.close()
        return out
    return call


def _gicp_call(reg, clouds):
    """RegisterPointClouds, and what the call was granted: 0 = the rounds, else the workgroups of its cooperative launch"""
    reg.grants = []

    def call():
        before = reg.coop_stats()["launches"]
        out = reg.RegisterPointClouds(*clouds)
        st = reg.coop_stats()
        reg.grants.append(st["last_workgroups"] if st["launches"] > before else 0)
        return out
    return call


def tracking(A, I, _):
    orb = A.ORBextractor(300, 1.2, 3, 20, 7, max_rows=120, max_cols=160)
    trk = A.KltTracker(160, 120, 15, max_batch=1, max_points=64)
    fm = A.FundamentalMatcher(max_points=64)
    m = A.ProjectionMatcher(max_last=128, max_cur=128, max_batch=1)
    m.reserve_local(128)
    po = A.PoseOptimizer(max_obs=64, max_batch=1)
    reg = A.RegistrationGICP(max_points=5120)
    calls = [("orb_extract", lambda: orb(I["gray"][0])),
             ("fbKltTracking", _klt_call(trk, I["klt"][0], I["klt_pts"][0])),
             ("findFundamentalMat", lambda: fm.findFundamentalMat(I["fmat"][0], I["fmat"][1], 2.0, 0.99, 200)),
             ("SearchByProjection", lambda: m.SearchByProjection(I["sbp"])),
             ("search_local_points", lambda: m.search_local_points(I["local"][0])),
             ("PoseOptimization", lambda: po.PoseOptimization(I["pose"])),
             ("RegisterPointClouds_5120", _gicp_call(reg, I["cloud5120"]))]
    return calls, [orb, trk, fm, m, po, reg]


def local_mapping(A, I, _):
    lba = A.Optimizer(max_poses=8, max_points=256, max_edges=4096)
    m = A.ProjectionMatcher(max_last=128, max_cur=128, max_batch=1)
    m.reserve_fuse(1, 128, 2)
    m.reserve_triangulation(2, 1 << 16)
    upd = A.MapPointUpdater(max_points=128, max_observations=4096)
    f = I["fuse"][0]
    calls = [("LocalBundleAdjustment", lambda: lba.LocalBundleAdjustment(I["lba"])),
             ("fuse_search", lambda: m.fuse_search(f["lists"], f["keyframes"])),
             ("create_new_map_points", lambda: m.create_new_map_points(I["tri"])),
             ("map_point_update", lambda: upd.update(I["map_points"]))]
    return calls, [lba, m, upd]


def loop_closing(A, I, _):
    m = A.ProjectionMatcher(max_last=128, max_cur=128, max_batch=1)
    m.reserve_bow(1, 2)
    m.reserve_sim3_search(1, 128, 1)
    rs = A.Sim3RansacSolver(max_batch=1, max_pairs=128)
    so = A.Sim3Optimizer(max_batch=1, max_pairs=128)
    eg = A.EssentialGraphOptimizer(max_vertices=64, max_edges=256, max_points=1024)
    gba = A.GlobalOptimizer(max_poses=48, max_points=512, max_edges=16384)
    s = I["sim3_search"]
    calls = [("search_by_bow", lambda: m.search_by_bow(I["bow"])),
             ("sim3_ransac_solve", lambda: rs.solve(I["ransac"][0])),
             ("sim3_search", lambda: m.sim3_search(s["lists"], s["problems"])),
             ("OptimizeSim3", lambda: so.OptimizeSim3(I["sim3_opt"])),
             ("OptimizeEssentialGraph", lambda: eg.OptimizeEssentialGraph(I["essential_graph"])),
             ("GlobalBundleAdjustment", lambda: gba.BundleAdjustment(I["gba"]))]
    return calls, [m, rs, so, eg, gba]


def registration(A, I, _):
    """the second GICP handle (80 chunks against Tracking's 20), and a refused call a round: its code and its text are this thread's"""
    reg = A.RegistrationGICP(max_points=20480)

    def refused():
        try:
            reg.RegisterPointClouds(I["cloud20480"][0], I["too_many"])
        except A.GfsError as e:
            return dict(code=e.code, text=A.lib().gfs_last_error())
        return dict(code=0, text=b"")

    return [("RegisterPointClouds_20480", _gicp_call(reg, I["cloud20480"])), ("refused_call", refused)], [reg]


def shared_handles(A):
    m = A.ProjectionMatcher(max_last=128, max_cur=128, max_batch=1)
    m.reserve_local(128)
    m.reserve_fuse(1, 128, 2)
    return dict(m=m, bf=A.ORBmatcher(max_query=512, max_train=512), rs=A.Sim3RansacSolver(max_batch=1, max_pairs=128),
                trk=A.KltTracker(160, 120, 15, max_batch=1, max_points=64))


def _shared(k):
    def script(A, I, H):
        f = I["fuse"][k]
        search = (lambda: H["m"].fuse_search(f["lists"], f["keyframes"])) if k == 0 else (lambda: H["m"].search_local_points(I["local"][1]))
        return [("fuse_search" if k == 0 else "search_local_points", search),
                ("bf_match", lambda: H["bf"].match(I["desc"][2 * k], I["desc"][2 * k + 1])),
                ("sim3_ransac_solve", lambda: H["rs"].solve(I["ransac"][k])),
                ("fbKltTracking", _klt_call(H["trk"], I["klt"][k], I["klt_pts"][k]))], []
    return script


SEPARATE = dict(tracking=tracking, local_mapping=local_mapping, loop_closing=loop_closing, registration=registration)
SHARED = dict(shared_a=_shared(0), shared_b=_shared(1))
OWN_ERRORS = ("registration",)  # threads whose script sets gfs_last_error() itself


# ---------------------------------------------------------------- the runs

def _run(A, I, H, name, script, rounds, barrier, rec):
    """the thread's body (and, with barrier = None, the serial pass): rec = dict(got {(round, call): flat}, rounds, mismatches, errors, stats)"""
    handles = []
    try:
        if barrier is not None:
            barrier.wait(timeout=120)
        calls, handles = script(A, I, H)
        mine = A.lib().gfs_last_error()
        for r in range(rounds):
            for cname, fn in calls:
                rec["got"][(r, cname)] = flatten(fn())
                if name not in OWN_ERRORS and A.lib().gfs_last_error() != mine:
                    rec["mismatches"].append([name, r, cname, "gfs_last_error"])
                if cname == "refused_call":
                    g = rec["got"][(r, cname)]
                    if g["/code"] != flatten(GFS_ERR_CAPACITY)[""] or len(g["/text"]) == 0:
                        rec["mismatches"].append([name, r, cname, "code or text"])
            rec["rounds"] = r + 1
        for h in handles:
            if hasattr(h, "grants"):  # a GICP handle: how its calls were driven
                want = -(-h.max_points // 256)
                rec["stats"][f"gicp{h.max_points}"] = dict(h.coop_stats(), calls=len(h.grants), rounds=h.grants.count(0), full=h.grants.count(want),
                                                            partial=sum(0 < g < want for g in h.grants), least_grant=min(h.grants))
    except BaseException:  # noqa: B036  (reported, not raised: the other threads finish and the parent sees every record)
        rec["errors"].append(traceback.format_exc()[-1500:])
    finally:
        for h in handles:
            h.close()


def _new_rec():
    return dict(got={}, rounds=0, mismatches=[], errors=[], stats={})


def _threads(A, I, H, scripts, rounds):
    barrier = threading.Barrier(len(scripts))
    recs = {name: _new_rec() for name in scripts}
    ts = [threading.Thread(target=_run, args=(A, I, H, name, s, rounds, barrier, recs[name]), name=name) for name, s in scripts.items()]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    return recs, time.perf_counter() - t0


def main(rounds=R):
    from geoflowslam_amd import api as A
    A.lib()
    assert A.device_count() >= 1
    assert len(SEPARATE) + 1 <= 5 and len(SHARED) + 1 <= 5  # at most five threads
    I = inputs()
    holder = A.RegistrationGICP(max_points=1024)
    hold = max(0, holder.coop_stats()["budget"] - COOP_FREE)
    holder.coop_hold(hold)
    try:
        recs, sec_separate = _threads(A, I, None, SEPARATE, rounds)
    finally:
        holder.coop_release(hold)
    holder.close()
    H = shared_handles(A)
    more, sec_shared = _threads(A, I, H, SHARED, rounds)
    recs.update(more)
    scripts = dict(SEPARATE, **SHARED)
    for name, rec in recs.items():  # the serial pass: one round of the same script, alone
        ref = _new_rec()
        _run(A, I, H, name, scripts[name], 1, None, ref)
        rec["errors"] += ["serial pass: " + e for e in ref["errors"]] + [f"serial pass: {m}" for m in ref["mismatches"]]
        for (r, cname), flat in sorted(rec["got"].items()):
            want = ref["got"].get((0, cname), {})
            rec["mismatches"] += [[name, r, cname, k] for k in sorted(set(flat) | set(want)) if flat.get(k) != want.get(k)]
        print(json.dumps(dict(thread=name, rounds=rec["rounds"], calls=len(rec["got"]), mismatches=rec["mismatches"], errors=rec["errors"],
                              stats=rec["stats"])), flush=True)
    for h in H.values():
        h.close()
    print(json.dumps(dict(run=True, R=rounds, coop_held=hold, seconds_separate=round(sec_separate, 3), seconds_shared=round(sec_shared, 3),
                          coop_in_use=A.gicp_coop_in_use())), flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else R)
