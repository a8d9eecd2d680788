"""The Sim3 searches of loop closing as adaptor code (geoflowslam_amd/host/gfs_adaptors.hpp: gfs_host::FuseSim3, both SearchAndFuse
overloads, both SearchByProjectionSim3 overloads, Sim3Searcher) over plain-struct KeyFrame / MapPoint classes
(tests/host/sim3_search_adaptor_test.cpp).  The CPU tests plug the sequential restatement in as the device call and compare the end
state (every key frame's map-point slots, vpMatched / vpMatchedKF, every point's bad flag / observations / replaced pointer /
descriptor updates, the counts) with a plain sequential loop that searches point by point against the live state; the GPU test runs
the same through Sim3Searcher.  Also: the product's host statement of the rule (csrc/sim3_search_rule.hpp, what the replays
recompute with) against the restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sim3_search_support as SS
from geoflowslam_amd import api as A
from geoflowslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(ROOT, "tests", "host", "_sim3_search_adaptor_test.so")
SEARCH_AND_FUSE_MAP, SEARCH_AND_FUSE_KFS, FUSE_ONE, SBP, SBP_KFS = range(5)
ADAPTOR, ADAPTOR_GPU, SEQUENTIAL, SEQUENTIAL_STALE, TWO_CAMERA, FISHEYE = range(6)
N_LIST, N_HOLD, N_KP = 300, 100, 350


@pytest.fixture(scope="module")
def harness(api):
    src = os.path.join(ROOT, "tests", "host", "sim3_search_adaptor_test.cpp")
    csrc = os.path.join(ROOT, "geoflowslam_amd", "csrc")
    deps = [src, os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp"), os.path.join(ROOT, "include", "gfs_abi.h"),
            os.path.join(csrc, "sim3_search_rule.hpp"), os.path.join(csrc, "fuse_rule.hpp"), os.path.join(csrc, "glibc_math.hpp")]
    if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
        libdir = os.path.join(ROOT, "geoflowslam_amd")
        tmp = _SO + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", tmp, src, "-L" + libdir,
                        "-lgfs_hip", "-ldl", "-lpthread", "-Wl,-rpath," + libdir], check=True)
        os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    L.sim3_adaptor_test.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(A.Sim3SearchProblem), C.c_int, C.POINTER(A.FusePoints), C.c_int] + \
        [C.c_void_p] * 10
    L.sim3_host_rule.argtypes = [C.POINTER(A.FusePoints), C.c_int, C.POINTER(A.Sim3SearchProblem), C.c_int, C.POINTER(A.Sim3SearchResult)]
    return L


def _points(seed, mode, n_kfs, th, ratio=1.0):
    """N_LIST list points and N_HOLD more that only sit in key frames, one gfs_fuse_points of N_LIST + N_HOLD"""
    rng = np.random.default_rng(seed)
    prob = synth.sim3_search_problem(seed, mode, n_points=N_LIST, n_kp=N_KP, n_problems=n_kfs, th=th, ratio_hamming=ratio, masks=False)
    lst = {k: np.array(v) for k, v in prob["lists"][0].items()}
    pick = rng.integers(0, N_LIST, N_HOLD)
    pts = {k: np.concatenate([v, v[pick]]) for k, v in lst.items()}
    pts["mp_desc"][N_LIST:] = rng.integers(0, 256, (N_HOLD, 32), dtype=np.uint8)
    kfs = [dict(k, kps_un=k["kps_un"].copy(), desc=k["desc"].copy(), kp_taken=None, mp_skip=None) for k in prob["problems"]]
    return rng, lst, pts, kfs


def _scene(seed, crafted=True):
    """Three key frames whose key-points hold nothing, a point that is not in the list (100 of 350), or a list point (30: it is
    already found there); one in twenty points is bad; (crafted) exactly what each scenario needs."""
    rng, lst, pts, kfs = _points(seed, SS.FUSE, 3, 4.0)
    M = N_LIST + N_HOLD
    slots = []
    for _ in kfs:
        s = np.full(N_KP, -1, np.int32)
        where = rng.permutation(N_KP)
        s[where[:N_HOLD]] = N_LIST + rng.permutation(N_HOLD)
        s[where[N_HOLD:N_HOLD + 30]] = rng.permutation(N_LIST)[:30]
        slots.append(s)
    bad = (rng.random(M) < 0.05).astype(np.uint8)
    extra = rng.integers(0, 5, M).astype(np.int32)
    alt = rng.integers(0, 256, (M, 32), dtype=np.uint8)
    has_alt = (rng.random(M) < 0.2).astype(np.uint8)
    info = {}
    if crafted:
        r = SS.restate(dict(lists=[lst], problems=kfs))
        inside = set(np.concatenate(slots).tolist())
        seen0, seen1, ok = set(), set(), []
        for i in range(N_LIST):
            j0, j1 = int(r[0]["best_idx"][i]), int(r[1]["best_idx"][i])
            if r[0]["exit"][i] == SS.MATCHED and r[1]["exit"][i] == SS.MATCHED and i not in inside and j0 not in seen0 and j1 not in seen1 and \
                    (j1 + 1) % N_KP not in seen1:
                ok.append(i)
                seen0.add(j0)
                seen1.update((j1, (j1 + 1) % N_KP))
        others = [o for o in range(N_LIST, M)]
        for i in ok[:8]:
            bad[i] = has_alt[i] = 0
        # every other list point that would meet a scenario's key-points is taken out of the way
        for i in range(N_LIST):
            if i not in ok[:8] and (int(r[0]["best_idx"][i]) in seen0 or int(r[1]["best_idx"][i]) in seen1):
                bad[i] = 1

        def free(o):
            for s in slots:
                s[s == o] = -1
            bad[o] = 0

        # two list points on one key-point: the first is added (AddMapPoint), the second gets a replace entry for it
        ia, ib = sorted(ok[0:2])
        for k in pts:
            pts[k][ib] = pts[k][ia]
        j0 = int(r[0]["best_idx"][ia])
        slots[0][j0] = -1
        slots[0][int(r[0]["best_idx"][ib])] = -1
        info["pair"] = (ia, ib, j0)
        # a key-point that already has a bad point: nothing is added, nothing replaced
        ic, o = ok[2], others[0]
        free(o)
        j0 = int(r[0]["best_idx"][ic])
        slots[0][j0] = o
        bad[o] = 1
        info["bad_holder"] = (ic, o, j0)
        # Replace makes a list point already-found in a later key frame: o sits on p's key-point in key frame 0 and somewhere else in
        # key frame 1, so after o->Replace(p) key frame 1 holds p, and p is not searched there
        ip, o = ok[3], others[1]
        free(o)
        j0, j1 = int(r[0]["best_idx"][ip]), int(r[1]["best_idx"][ip])
        jx = next(j for j in range(N_KP) if j not in seen1 and slots[1][j] == -1 and not (r[1]["best_idx"] == j).any())
        slots[0][j0], slots[1][jx], slots[1][j1] = o, o, -1
        info["found_later"] = (ip, o, jx, j1)
        # Replace changes a list point's descriptor: o sits on c's key-point in key frame 0; o->Replace(c) ends in
        # c->ComputeDistinctiveDescriptors(), and with the new descriptor c matches a DIFFERENT key-point in key frame 1
        c, o = ok[4], others[2]
        free(o)
        j0, j1 = int(r[0]["best_idx"][c]), int(r[1]["best_idx"][c])
        slots[0][j0] = o
        jn = (j1 + 1) % N_KP  # a key-point half a pixel beside j1 that carries exactly the new descriptor
        k1 = kfs[1]
        for fld in ("x", "y", "octave"):
            k1["kps_un"][fld][jn] = k1["kps_un"][fld][j1]
        k1["kps_un"]["x"][jn] += np.float32(0.5)
        k1["desc"][jn] = alt[c]
        has_alt[c] = 1
        slots[1][[j1, jn]] = -1
        info["changed"] = (c, j1, jn)
    return dict(kfs=kfs, pts=pts, slots=slots, bad=bad, extra=extra, alt=alt, has_alt=has_alt, info=info,
                point_kf=rng.integers(0, 16, M).astype(np.int32))


def _projection_scene(seed, mode):
    """One key frame; vpMatched holds nothing, a point that is not in the list (a fifth) or a list point (one in ten: already found)."""
    rng, lst, pts, kfs = _points(seed, mode, 1, {SS.SBP: 3.0, SS.SBP_KFS: 8.0}[mode], 1.5)
    M = N_LIST + N_HOLD
    s = np.full(N_KP, -1, np.int32)
    where = rng.permutation(N_KP)
    s[where[:70]] = N_LIST + rng.permutation(N_HOLD)[:70]
    s[where[70:105]] = rng.permutation(N_LIST)[:35]
    return dict(kfs=kfs, pts=pts, slots=[s], bad=(rng.random(M) < 0.05).astype(np.uint8), extra=np.zeros(M, np.int32),
                alt=np.zeros((M, 32), np.uint8), has_alt=np.zeros(M, np.uint8), info={}, point_kf=rng.integers(0, 16, M).astype(np.int32))


def _run(L, what, mode, S):
    SS.restatement()
    LL, PP, _, keep = A.sim3_search_structs([S["pts"]], S["kfs"])
    slots = np.concatenate(S["slots"]).astype(np.int32)
    M = len(S["pts"]["mp_xw"])
    o = dict(final=np.full(len(slots), -9, np.int32), state=np.full((M, 4), -9, np.int32), matched_kf=np.full(len(S["slots"][0]), -9, np.int32),
             counts=np.full(5, -9, np.int32))
    arrs = [slots, S["bad"], S["extra"], np.ascontiguousarray(S["alt"]), S["has_alt"], S["point_kf"], o["final"], o["state"], o["matched_kf"],
            o["counts"]]
    o["rc"] = L.sim3_adaptor_test(SS._SO.encode(), what, mode, PP, len(S["kfs"]), LL, N_LIST, *[a.ctypes.data for a in arrs])
    o["per_kf"] = np.split(o["final"], np.cumsum([len(s) for s in S["slots"]])[:-1])
    return o


def _same(a, b, counts=(0, 1, 4)):
    assert a["rc"] == 0 and b["rc"] == 0
    assert SS.same_bits(a["final"], b["final"]), np.nonzero(a["final"] != b["final"])[0][:8]
    assert SS.same_bits(a["state"], b["state"]), np.nonzero((a["state"] != b["state"]).any(1))[0][:8]
    assert SS.same_bits(a["matched_kf"], b["matched_kf"])
    assert a["counts"][list(counts)].tolist() == b["counts"][list(counts)].tolist()


@pytest.mark.parametrize("what", [SEARCH_AND_FUSE_MAP, SEARCH_AND_FUSE_KFS])
@pytest.mark.parametrize("seed", [31, 32])
def test_search_and_fuse_ends_as_the_sequential_loop(harness, what, seed):
    S = _scene(seed)
    seq, ada = _run(harness, what, SEQUENTIAL, S), _run(harness, what, ADAPTOR, S)
    _same(ada, seq)
    assert ada["counts"][3] == 1 and ada["counts"][4] == 3  # one device call for the three key frames; the map lock once a key frame
    assert seq["counts"][0] > 30 and seq["counts"][1] > 5
    st, info, start = seq["state"], S["info"], S["slots"]
    assert (st[:, 0] != S["bad"]).sum() > 5 and (seq["final"] != np.concatenate(start)).sum() > 20
    # two list points on one key-point: a is added, b gets a replace entry for a, and a->Replace(b) leaves b there
    a, b, j0 = info["pair"]
    assert start[0][j0] == -1 and seq["per_kf"][0][j0] == b and st[a, 0] == 1 and st[a, 2] == b and st[b, 0] == 0
    # a key-point that holds a bad point: counted as fused, nothing added or replaced
    c, o, j0 = info["bad_holder"]
    assert seq["per_kf"][0][j0] == o and st[c, 2] == -1 and st[o, 2] == -1
    # already found in key frame 1 through the Replace of key frame 0: not searched there
    p, o, jx, j1 = info["found_later"]
    assert st[o, 0] == 1 and st[o, 2] == p and seq["per_kf"][1][jx] == p and seq["per_kf"][1][j1] == -1
    # descriptor changed by the Replace of key frame 0 -> a different key-point in key frame 1, through the recompute path
    c, j1, jn = info["changed"]
    assert ada["counts"][2] >= 1
    assert seq["per_kf"][1][jn] == c and seq["per_kf"][1][j1] == -1
    stale = _run(harness, what, SEQUENTIAL_STALE, S)  # the same loop fed the uploaded descriptors: a replay without the recompute
    assert stale["rc"] == 0 and stale["per_kf"][1][j1] == c and stale["per_kf"][1][jn] == -1
    assert not SS.same_bits(stale["final"], seq["final"])


def test_fuse_sim3_on_one_key_frame_and_plain_scenes(harness):
    S = _scene(33)
    _same(_run(harness, FUSE_ONE, ADAPTOR, S), _run(harness, FUSE_ONE, SEQUENTIAL, S))
    S = _scene(34, crafted=False)
    for what in (SEARCH_AND_FUSE_MAP, SEARCH_AND_FUSE_KFS, FUSE_ONE):
        _same(_run(harness, what, ADAPTOR, S), _run(harness, what, SEQUENTIAL, S))


@pytest.mark.parametrize("what,mode", [(SBP, SS.SBP), (SBP_KFS, SS.SBP_KFS)])
def test_search_by_projection_ends_as_the_sequential_loop(harness, what, mode):
    S = _projection_scene(41 + what, mode)
    seq, ada = _run(harness, what, SEQUENTIAL, S), _run(harness, what, ADAPTOR, S)
    _same(ada, seq)
    start, end = S["slots"][0], seq["per_kf"][0]
    new = np.nonzero(end != start)[0]
    assert ada["counts"][3] == 1 and seq["counts"][0] == len(new) > 20 and (start[new] == -1).all() and (end[new] < N_LIST).all()
    assert not S["bad"][end[new]].any() and not np.isin(end[new], start).any()  # no bad point, none that was already found
    if what == SBP_KFS:  # vpMatchedKF is filled where vpMatched is, with the matched point's key frame
        assert (seq["matched_kf"][new] == S["point_kf"][end[new]]).all() and (np.delete(seq["matched_kf"], new) == -1).all()
    else:
        assert (seq["matched_kf"] == -1).all()


def test_two_camera_and_fisheye_key_frames_are_refused(harness):
    S = _scene(34, crafted=False)
    for what in (SEARCH_AND_FUSE_MAP, SEARCH_AND_FUSE_KFS, FUSE_ONE):
        assert _run(harness, what, TWO_CAMERA, dict(S, kfs=S["kfs"][:1], slots=S["slots"][:1]) if what == FUSE_ONE else S)["rc"] == -200
        assert _run(harness, what, FISHEYE, dict(S, kfs=S["kfs"][:1], slots=S["slots"][:1]) if what == FUSE_ONE else S)["rc"] == -200
    P = _projection_scene(44, SS.SBP)
    assert _run(harness, SBP, TWO_CAMERA, P)["rc"] == -200 and _run(harness, SBP_KFS, FISHEYE, P)["rc"] == -200


def _host_rule(L, prob):
    LL, PP, RR, keep = A.sim3_search_structs(prob["lists"], prob["problems"])
    assert L.sim3_host_rule(LL, len(prob["lists"]), PP, len(prob["problems"]), RR) == 0
    return A.sim3_search_results(LL, PP, RR, keep, len(prob["lists"]))


def test_host_rule_equals_the_restatement(harness):
    """csrc/sim3_search_rule.hpp compiled for the host (projection forms, gates, level, the acceptance tests: the code the kernel
    runs, and the linear scan in visiting order against a taken array that stands in for the grid) gives the restatement's bits on
    random and constructed problems."""
    for mode in SS.MODES:
        for n, c in ((257, 500), (1000, 500), (65, 1), (64, 0)):
            prob, want, st = SS.problem(mode, n, c)
            SS.assert_equal(_host_rule(harness, prob), want, (mode, n, c))
    for prob, want in (SS.five_problems(), SS.two_lists()):
        SS.assert_equal(_host_rule(harness, prob), want)
    prob, labels, extra = SS.constructed()
    out = _host_rule(harness, prob)
    SS.check_constructed(prob, labels, out)
    SS.assert_equal(out, SS.restate(prob), "constructed")


@pytest.mark.gpu
@pytest.mark.parametrize("what", [SEARCH_AND_FUSE_MAP, SEARCH_AND_FUSE_KFS, FUSE_ONE, SBP, SBP_KFS])
def test_adaptors_end_to_end_on_gpu(harness, gpu_api, what):
    S = _scene(31) if what <= FUSE_ONE else _projection_scene(41 + what, SS.SBP if what == SBP else SS.SBP_KFS)
    cpu, gpu = _run(harness, what, ADAPTOR, S), _run(harness, what, ADAPTOR_GPU, S)
    _same(gpu, cpu, counts=(0, 1, 2, 3, 4))
    assert what > SEARCH_AND_FUSE_KFS or gpu["counts"][2] >= 1
