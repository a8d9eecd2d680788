"""Tracking::SearchLocalPoints as adaptor code (geoflowslam_amd/host/gfs_adaptors.hpp: gfs_host::SearchLocalPoints and
LocalPointsSearcher) over plain-struct Frame / MapPoint classes (tests/host/local_points_adaptor_test.cpp).  The CPU test plugs the
sequential restatement in as the solver and checks the first loop's effects, which points are listed, every field written back and
the IncreaseVisible counts against a statement of the function in Python around the same restatement; the GPU test runs the same
through LocalPointsSearcher and must give the same bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import local_points_support as LPS
from geoflowslam_amd import api as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(ROOT, "tests", "host", "_local_points_adaptor_test.so")
STALE = -7.0  # what the harness leaves in the mTrack* fields before the call


@pytest.fixture(scope="module")
def harness(api):
    src = os.path.join(ROOT, "tests", "host", "local_points_adaptor_test.cpp")
    deps = [src, os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp"), os.path.join(ROOT, "include", "gfs_abi.h")]
    if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
        libdir = os.path.join(ROOT, "geoflowslam_amd")
        tmp = _SO + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-o", tmp, src, "-L" + libdir, "-lgfs_hip", "-ldl",
                        "-lpthread", "-Wl,-rpath," + libdir], check=True)
        os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    L.local_points_adaptor_test.argtypes = [C.c_char_p, C.c_int, C.POINTER(A.LocalPointsProblem)] + [C.c_void_p] * 3 + [C.c_float] + \
        [C.c_void_p] * 7
    return L


def _scene(seed, n_mp=400, n_cur=300):
    prob = dict(LPS.frame(n_mp, n_cur, seed=seed, hard=True)[0])
    rng = np.random.default_rng(seed)
    n, nc = len(prob["mp_xw"]), len(prob["cur_kps_un"])
    bad = (rng.random(n) < 0.1).astype(np.uint8)
    obs = np.where(np.asarray(prob["mp_has_obs"]) != 0, rng.integers(1, 5, n), 0).astype(np.int32)
    held = np.where(rng.random(nc) < 0.2, rng.integers(0, max(n, 1), nc), -1).astype(np.int32) if n else np.full(nc, -1, np.int32)
    return prob, bad, obs, held


def _run(L, mode, prob, bad, obs, held, th):
    P, _, keep = A.local_points_structs(prob)
    n, nc = max(P.n_mp, 1), max(P.n_cur, 1)
    o = dict(visible=np.zeros(n, np.int32), last_seen=np.zeros(n, np.int32), in_view=np.zeros(n, np.uint8),
             track=np.zeros((n, 6), np.float32), project=np.zeros((n, 3), np.float32), final=np.zeros(nc, np.int32),
             counts=np.zeros(3, np.int32))
    LPS.restatement()
    o["rc"] = L.local_points_adaptor_test(LPS._SO.encode(), mode, C.byref(P), bad.ctypes.data, obs.ctypes.data, held.ctypes.data, th,
                                          *[o[k].ctypes.data for k in ("visible", "last_seen", "in_view", "track", "project", "final", "counts")])
    return o


def _expected(prob, bad, obs, held, th):
    """Tracking::SearchLocalPoints, src/Tracking.cc:4294-4359, around the restatement."""
    n, nc = len(prob["mp_xw"]), len(prob["cur_kps_un"])
    visible, seen = np.zeros(n, np.int32), np.zeros(n, bool)
    final = held.copy()
    for i in range(nc):  # the first loop
        h = held[i]
        if h < 0:
            continue
        if bad[h]:
            final[i] = -1
        else:
            visible[h] += 1
            seen[h] = True
    listed = np.array([j for j in range(n) if not seen[j] and not bad[j]], np.int64)
    sub = dict(prob)
    for k in ("mp_xw", "mp_normal", "mp_min_dist", "mp_max_dist", "mp_desc"):
        sub[k] = np.asarray(prob[k])[listed]
    sub["mp_has_obs"] = (obs[listed] > 0).astype(np.uint8)
    sub["cur_has_mp_obs"] = np.array([final[i] >= 0 and obs[final[i]] > 0 for i in range(nc)], np.uint8)
    sub.update(th=np.float32(th), view_cos_limit=np.float32(0.5), nn_ratio=np.float32(0.8))
    r = LPS.restate(sub)
    in_view = np.full(n, 3, np.uint8)  # mbTrackInView | mbTrackInViewR << 1: stale `true` where nothing writes them
    in_view[seen] = 0
    track = np.full((n, 6), STALE, np.float32)
    project = np.zeros((n, 3), np.float32)
    for k, j in enumerate(listed):
        v = int(r["in_view"][k])
        in_view[j] = v | 2
        track[j, 0:2] = r["proj"][k, 0:2]
        if v:
            track[j, 2], track[j, 3], track[j, 4], track[j, 5] = r["proj"][k, 2], r["view_cos"][k], r["depth"][k], r["level"][k]
            visible[j] += 1
            project[j] = (1, r["proj"][k, 0], r["proj"][k, 1])
    hit = r["cur_match"] >= 0
    final[hit] = listed[r["cur_match"][hit]]
    return dict(visible=visible, last_seen=np.where(seen, 42, 41).astype(np.int32), in_view=in_view, track=track, project=project,
                final=final.astype(np.int32), counts=(len(listed), r["nmatches"])), r


def _check(o, e):
    assert o["rc"] == 0
    assert tuple(o["counts"][:2]) == e["counts"]
    for k in ("visible", "last_seen", "in_view", "track", "project", "final"):
        assert LPS.same_bits(o[k][:len(e[k])], e[k]), k


@pytest.mark.parametrize("seed,th", [(11, 1.0), (12, 3.0)])
def test_adaptor_against_restatement(harness, seed, th):
    prob, bad, obs, held = _scene(seed)
    e, r = _expected(prob, bad, obs, held, th)
    # the scene exercises what it is meant to: bad and held points exist, some key-point held a bad point, matches are written
    assert bad.any() and (held >= 0).any() and any(bad[h] for h in held if h >= 0) and r["nmatches"] > 0
    assert 0 < e["counts"][0] < len(bad) and (e["visible"] > 1).any()
    _check(_run(harness, 0, prob, bad, obs, held, th), e)


def test_empty_list_and_no_key_points(harness):
    prob, bad, obs, held = _scene(13, n_mp=0, n_cur=50)
    _check(_run(harness, 0, prob, bad, obs, held, 1.0), _expected(prob, bad, obs, held, 1.0)[0])
    prob, bad, obs, held = _scene(14, n_mp=100, n_cur=0)
    _check(_run(harness, 0, prob, bad, obs, held, 1.0), _expected(prob, bad, obs, held, 1.0)[0])


def test_two_camera_and_fisheye_frames_are_refused(harness):
    prob, bad, obs, held = _scene(11)
    assert _run(harness, 2, prob, bad, obs, held, 1.0)["rc"] == -200
    assert _run(harness, 3, prob, bad, obs, held, 1.0)["rc"] == -200


@pytest.mark.gpu
def test_adaptor_end_to_end_on_gpu(harness, gpu_api):
    prob, bad, obs, held = _scene(11)
    e, _ = _expected(prob, bad, obs, held, 1.0)
    _check(_run(harness, 1, prob, bad, obs, held, 1.0), e)
