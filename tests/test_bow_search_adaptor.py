"""gfs_host::SearchByBoW and gfs_host::BowMatchesOfCandidate (geoflowslam_amd/host/gfs_adaptors.hpp) on mock KeyFrame / MapPoint
classes (tests/host/bow_search_adaptor_test.cpp) with the host restatement as the search: the gather (map points folded into has_mp,
bad ones included; null and bad key frames 2 left out), the indices mapped back to map points, and the merge of reference
src/LoopClosing.cc:717-730 against an independent statement.  The GPU test runs the same through gfs_host::BowSearcher."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bow_search_support as BS
from geoflowslam_amd import api as A
from geoflowslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(ROOT, "tests", "host", "_bow_search_adaptor_test.so")
NONE, GOOD, BAD = 0, 1, 2       # kinds of a key-point's map point
KF, KF_NULL, KF_BAD = 0, 1, 2   # states of an entry of vpCovKFi


@pytest.fixture(scope="module")
def harness(api):
    src = os.path.join(ROOT, "tests", "host", "bow_search_adaptor_test.cpp")
    csrc = os.path.join(ROOT, "geoflowslam_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tests", "host", "bow_search_restatement.cpp"), os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp"),
            os.path.join(ROOT, "include", "gfs_abi.h"), os.path.join(csrc, "bow_search_rule.hpp")]
    if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
        libdir = os.path.dirname(api._LIB_PATH)
        tmp = _SO + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        "-o", tmp, src, "-L" + libdir, "-lgfs_hip", "-Wl,-rpath," + libdir], check=True)
        os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    L.bow_adaptor_test.argtypes = [C.c_int, C.POINTER(A.BowProblem)] + [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 6
    return L


def scene(seed, n_kf2=4, n_kp=120, states=None, bad_frac=0.08, share_frac=0.5):
    """A problem, the kind of every key-point's map point, and identities for the points of side 2: key-point i of a key frame 2
    observes point src-of-i with probability share_frac (so key frames 2 share points) and a point of its own otherwise."""
    p = synth.bow_search_problem(seed, n_kp=n_kp, n_kf2=n_kf2, n_nodes=10, max_flip_bits=40, nn_ratio=0.9, check_orientation=True)
    rng = np.random.default_rng(seed + 77)
    n_points = n_kp + n_kf2 * n_kp
    bad_point = rng.random(n_points) < bad_frac
    kinds2, ids2 = [], []
    for j, k2 in enumerate(p["kf2"]):
        shared = rng.permutation(n_kp)  # a point of the shared range at most once per key frame
        own = n_kp + j * n_kp + np.arange(n_kp)
        ids = np.where(rng.random(n_kp) < share_frac, shared, own).astype(np.int32)
        kind = np.where(k2["has_mp"] == 0, NONE, np.where(bad_point[ids], BAD, GOOD)).astype(np.uint8)
        kinds2.append(kind)
        ids2.append(ids)
    kind1 = np.where(p["kf1"]["has_mp"] == 0, NONE, np.where(rng.random(n_kp) < bad_frac, BAD, GOOD)).astype(np.uint8)
    return dict(problem=p, kind1=kind1, kinds2=kinds2, ids2=ids2, n_points=n_points, bad_point=bad_point,
                states=np.zeros(n_kf2, np.int32) if states is None else np.asarray(states, np.int32))


def run(L, sc, gpu=False, two_cameras=False):
    p = sc["problem"]
    kinds = dict(p, kf1=dict(p["kf1"], has_mp=sc["kind1"]), kf2=[dict(k, has_mp=kd) for k, kd in zip(p["kf2"], sc["kinds2"])])
    PP, RP, keep = A.bow_structs([kinds])
    n, m = len(sc["kind1"]), len(p["kf2"])
    id1, id2 = np.arange(n, dtype=np.int32), np.concatenate(sc["ids2"] + [np.zeros(1, np.int32)]).astype(np.int32)
    o = dict(list_size=np.full(m, -9, np.int32), match_id=np.full((m, n), -9, np.int32), n_matches=np.full(m, -9, np.int32),
             merged_id=np.full(n, -9, np.int32), merged_kf=np.full(n, -9, np.int32), summary=np.full(3, -9, np.int32))
    o["ret"] = L.bow_adaptor_test(int(gpu), PP, id1.ctypes.data, id2.ctypes.data, sc["states"].ctypes.data, sc["n_points"], int(two_cameras),
                                  *[v.ctypes.data for v in o.values()])
    return o


def expected(sc):
    """The restatement on the key frames that are searched, the map points folded into has_mp; then :706-730 in plain Python."""
    p, st = sc["problem"], sc["states"]
    used = [j for j in range(len(p["kf2"])) if st[j] == KF]
    q = dict(p, kf1=dict(p["kf1"], has_mp=(sc["kind1"] == GOOD).astype(np.uint8)),
             kf2=[dict(p["kf2"][j], has_mp=(sc["kinds2"][j] == GOOD).astype(np.uint8)) for j in used])
    res = dict(zip(used, BS.restate(q)))
    n, m = len(sc["kind1"]), len(p["kf2"])
    match_id, n_matches, sizes = np.full((m, n), -1, np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32)
    most, index_most = 0, 0
    for j in used:
        m12 = res[j]["match12"]
        match_id[j] = np.where(m12 >= 0, sc["ids2"][j][np.maximum(m12, 0)], -1)
        n_matches[j], sizes[j] = res[j]["n_matches"], n
        if n_matches[j] > most:
            most, index_most = int(n_matches[j]), j
    merged_id, merged_kf, seen = np.full(n, -1, np.int32), np.full(n, -1, np.int32), set()
    for j in range(m):
        for k in range(sizes[j]):
            pid = int(match_id[j, k])
            if pid < 0 or sc["bad_point"][pid] or pid in seen:
                continue
            seen.add(pid)
            merged_id[k], merged_kf[k] = pid, j
    return dict(list_size=sizes, match_id=match_id, n_matches=n_matches, merged_id=merged_id, merged_kf=merged_kf,
                summary=np.array([len(seen), index_most, most], np.int32))


def check(o, want):
    assert o["ret"] == 0, o["ret"]
    for k, w in want.items():
        assert o[k].tobytes() == w.tobytes(), (k, o[k], w)


@pytest.mark.parametrize("seed", range(3))
def test_search_and_merge_equal_the_sequential_statement(harness, seed):
    sc = scene(20 + seed)
    o, want = run(harness, sc), expected(sc)
    check(o, want)
    ids = want["match_id"]
    twice = [pid for pid in np.unique(ids[ids >= 0]) if (ids == pid).any(1).sum() >= 2]
    assert len(twice) > 0, "a point matched through two key frames"
    assert want["summary"][0] < (ids >= 0).sum() and want["summary"][0] >= 20  # not taken again; enough for nBoWMatches
    assert (sc["kind1"] == BAD).any() and any((k == BAD).any() for k in sc["kinds2"])
    assert not (ids[:, sc["kind1"] != GOOD] >= 0).any()  # a bad or missing pMP1 is never searched
    assert not sc["bad_point"][ids[ids >= 0]].any()      # a bad pMP2 is never a candidate


def test_null_and_bad_key_frames_are_skipped_and_leave_their_lists_empty(harness):
    sc = scene(31, n_kf2=5, states=[KF, KF_NULL, KF, KF_BAD, KF])
    o, want = run(harness, sc), expected(sc)
    check(o, want)
    assert o["list_size"].tolist() == [120, 0, 120, 0, 120] and o["n_matches"][1] == o["n_matches"][3] == 0
    assert not np.isin(o["merged_kf"], [1, 3]).any() and want["summary"][2] > 0
    only = scene(31, n_kf2=2, states=[KF_NULL, KF_BAD])  # nothing to search: no device call, everything empty
    o = run(harness, only)
    check(o, expected(only))
    assert o["summary"].tolist() == [0, 0, 0] and (o["merged_id"] == -1).all()


def test_most_matches_index_is_the_first_maximum(harness):
    """num > nMostBoWNumMatches is strict: of two key frames 2 with the same matches the first keeps the index."""
    sc = scene(33, n_kf2=2)
    p = sc["problem"]
    sc["problem"] = dict(p, kf2=[p["kf2"][0], p["kf2"][0]])
    sc["kinds2"], sc["ids2"] = [sc["kinds2"][0]] * 2, [sc["ids2"][0]] * 2
    o, want = run(harness, sc), expected(sc)
    check(o, want)
    assert o["n_matches"][0] == o["n_matches"][1] > 0 and o["summary"][1] == 0
    assert (o["merged_kf"] <= 0).all()  # every point was already claimed through key frame 0


def test_two_camera_key_frames_are_refused(harness):
    assert run(harness, scene(34, n_kf2=1), two_cameras=True)["ret"] == -100


@pytest.mark.gpu
def test_adaptor_on_the_gpu(harness, gpu_api):
    sc = scene(35, n_kf2=5, states=[KF, KF, KF_NULL, KF, KF_BAD])
    check(run(harness, sc, gpu=True), expected(sc))
