"""ORBmatcher::Fuse / LocalMapping::SearchInNeighbors as adaptor code (geoflowslam_amd/host/gfs_adaptors.hpp: gfs_host::Fuse,
SearchInNeighborsFuse, FuseSearcher) over plain-struct KeyFrame / MapPoint classes (tests/host/fuse_adaptor_test.cpp).  The CPU tests
plug the sequential restatement in as the device call and compare the end state (every key frame's map-point slots, every point's
bad flag / observations / replaced pointer / update calls, the counts) with a plain sequential loop that searches point by point
against the live state; the GPU test runs the same through FuseSearcher.  Also: the product's host statement of the rule
(csrc/fuse_rule.hpp, what the replay recomputes with) against the restatement, pair by pair."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fuse_support as FS
from geoflowslam_amd import api as A
from geoflowslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(ROOT, "tests", "host", "_fuse_adaptor_test.so")


@pytest.fixture(scope="module")
def harness(api):
    src = os.path.join(ROOT, "tests", "host", "fuse_adaptor_test.cpp")
    deps = [src, os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp"), os.path.join(ROOT, "include", "gfs_abi.h"),
            os.path.join(ROOT, "geoflowslam_amd", "csrc", "fuse_rule.hpp"), os.path.join(ROOT, "geoflowslam_amd", "csrc", "glibc_math.hpp")]
    if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
        libdir = os.path.join(ROOT, "geoflowslam_amd")
        tmp = _SO + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", tmp, src, "-L" + libdir,
                        "-lgfs_hip", "-ldl", "-lpthread", "-Wl,-rpath," + libdir], check=True)
        os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    L.fuse_adaptor_test.argtypes = [C.c_char_p, C.c_int, C.POINTER(A.FuseKeyframe), C.c_int, C.POINTER(A.FusePoints)] + [C.c_void_p] * 8
    L.fuse_host_rule.argtypes = [C.POINTER(A.FusePoints), C.c_int, C.POINTER(A.FuseKeyframe), C.c_int, C.POINTER(A.FuseResult)]
    return L


def _scene(seed, crafted=True):
    """Key frame 0 = the current one (it holds 200 of the 300 points, one of them twice, with null slots in between), key frames
    1 and 2 = targets whose key-points hold other points, nothing, or (crafted) exactly what the scenario needs."""
    rng = np.random.default_rng(seed)
    prob = synth.fuse_problem(seed, n_points=300, n_kp=350, n_keyframes=3)
    pts = {k: np.array(v) for k, v in prob["lists"][0].items()}
    kfs = [dict(k, kps_un=k["kps_un"].copy(), u_right=k["u_right"].copy(), desc=k["desc"].copy()) for k in prob["keyframes"]]
    M, n_kp = 300, 350
    perm = rng.permutation(M)
    held, others = perm[:200], list(perm[200:])
    slots = [np.full(n_kp, -1, np.int32) for _ in kfs]
    slots[0][:200] = held
    slots[0][[3, 77]] = -1               # null entries inside the list
    slots[0][201] = slots[0][5]          # a duplicate in the list
    bad = (rng.random(M) < 0.05).astype(np.uint8)
    bad[slots[0][10]] = 1                # a bad entry for sure
    extra = rng.integers(0, 5, M).astype(np.int32)
    alt = rng.integers(0, 256, (M, 32), dtype=np.uint8)
    has_alt = (rng.random(M) < 0.2).astype(np.uint8)
    for f in (1, 2):                     # a third of the targets' key-points hold a point the current key frame does not
        take = rng.permutation(n_kp)[:len(others)]
        for j, o in zip(take[:n_kp // 3], others):
            slots[f][j] = o
    info = {}
    if crafted:
        lst = {k: v[np.maximum(slots[0], 0)] for k, v in pts.items()}
        r = FS.restate(dict(lists=[lst], keyframes=[dict(kfs[1], list=0), dict(kfs[2], list=0)]))
        ok = [i for i in range(200) if slots[0][i] >= 0 and i not in (5, 201) and r[0]["exit"][i] == FS.MATCHED and
              r[1]["exit"][i] == FS.MATCHED and not has_alt[slots[0][i]]]
        # scenario: list entry a and a later entry b pick the same key-point of key frame 1 (b's descriptor and position are a's);
        # once with a holding more observations, once fewer (the second meets the first and Replace goes either way)
        pairs = []
        for (ia, ib), more in zip(((ok[0], ok[1]), (ok[2], ok[3])), (True, False)):
            a, b = slots[0][ia], slots[0][ib]
            for k in pts:
                pts[k][b] = pts[k][a]
            j1 = int(r[0]["best_idx"][ia])
            slots[1][j1] = -1
            slots[1][slots[1] == a] = -1
            bad[a] = bad[b] = 0
            extra[a], extra[b] = (4, 0) if more else (0, 4)
            pairs.append((int(a), int(b), j1))
        # scenario: p goes bad in key frame 1 (the point there has more observations) and is skipped in key frame 2
        ip = ok[4]
        p, j1 = slots[0][ip], int(r[0]["best_idx"][ip])
        o = others[-1]
        slots[1][slots[1] == o] = -1
        slots[1][j1] = o
        bad[p] = bad[o] = 0
        extra[p], extra[o] = 0, 9
        info["goes_bad"] = (int(p), int(o), int(r[1]["best_idx"][ip]))
        # scenario: c's descriptor is changed by Replace in key frame 1 (the point there has fewer observations: it is replaced by c,
        # which ends in c->ComputeDistinctiveDescriptors()), and with the new descriptor c matches a DIFFERENT key-point in key frame 2
        ic = ok[5]
        c, j1, j2 = slots[0][ic], int(r[0]["best_idx"][ic]), int(r[1]["best_idx"][ic])
        o = others[-2]
        slots[1][slots[1] == o] = -1
        slots[2][slots[2] == o] = -1
        slots[1][j1] = o
        bad[c] = bad[o] = 0
        extra[c], extra[o] = 7, 0
        jn = (j2 + 1) % n_kp  # a key-point half a pixel beside j2 that carries exactly the new descriptor
        k2 = kfs[2]
        for fld in ("x", "y", "octave"):
            k2["kps_un"][fld][jn] = k2["kps_un"][fld][j2]
        k2["kps_un"]["x"][jn] += np.float32(0.5)
        k2["u_right"][jn] = -1
        k2["desc"][jn] = alt[c]
        has_alt[c] = 1
        slots[2][[j2, jn]] = -1
        info.update(changed=(int(c), j2, jn), pairs=pairs)
    return dict(kfs=kfs, pts=pts, slots=slots, bad=bad, extra=extra, alt=alt, has_alt=has_alt, info=info)


def _run(L, mode, S):
    FS.restatement()
    LL, KK, _, keep = A.fuse_structs([S["pts"]], S["kfs"])
    slots = np.concatenate(S["slots"]).astype(np.int32)
    M = len(S["pts"]["mp_xw"])
    o = dict(final=np.full(len(slots), -9, np.int32), state=np.full((M, 5), -9, np.int32), counts=np.full(5, -9, np.int32))
    arrs = [slots, S["bad"], S["extra"], np.ascontiguousarray(S["alt"]), S["has_alt"], o["final"], o["state"], o["counts"]]
    o["rc"] = L.fuse_adaptor_test(FS._SO.encode(), mode, KK, len(S["kfs"]), LL, *[a.ctypes.data for a in arrs])
    o["per_kf"] = np.split(o["final"], np.cumsum([len(s) for s in S["slots"]])[:-1])
    return o


def _same(a, b):
    assert a["rc"] == 0 and b["rc"] == 0
    assert FS.same_bits(a["final"], b["final"]), np.nonzero(a["final"] != b["final"])[0][:8]
    assert FS.same_bits(a["state"], b["state"]), np.nonzero((a["state"] != b["state"]).any(1))[0][:8]
    assert a["counts"][[0, 1, 3]].tolist() == b["counts"][[0, 1, 3]].tolist()


@pytest.mark.parametrize("seed", [21, 22])
def test_adaptor_end_state_equals_the_sequential_loop(harness, seed):
    S = _scene(seed)
    seq, ada = _run(harness, 2, S), _run(harness, 0, S)
    _same(ada, seq)
    assert ada["counts"][4] == 2  # one device call for all targets, one for the current key frame
    assert seq["counts"][0] > 20 and seq["counts"][1] > 0 and seq["counts"][3] == 1
    st, info = seq["state"], S["info"]
    # the scene exercises what it is meant to: points went bad, were replaced both ways round, got observations added
    assert (st[:, 0] != S["bad"]).sum() > 5 and (st[:, 2] >= 0).sum() > 5
    # two list points on one key-point: the second meets the first there and Replace goes by the observation count
    (a, b, j1), (a2, b2, j12) = info["pairs"]
    assert seq["per_kf"][1][j1] == a and st[b, 0] == 1 and st[b, 2] == a       # a had more observations: b is replaced by a
    assert seq["per_kf"][1][j12] == b2 and st[a2, 0] == 1 and st[a2, 2] == b2  # fewer: a is replaced by b
    # bad in key frame 1, skipped in key frame 2
    p, o, j2 = info["goes_bad"]
    assert st[p, 0] == 1 and st[p, 2] == o and seq["per_kf"][2][j2] != p
    # descriptor changed by Replace in key frame 1 -> a different key-point in key frame 2, through the recompute path
    c, j2, jn = info["changed"]
    assert ada["counts"][2] >= 1
    assert seq["per_kf"][2][jn] == c and seq["per_kf"][2][j2] == -1
    stale = _run(harness, 3, S)  # the same loop searching with the descriptors of the upload: what a replay without the recompute gives
    assert stale["rc"] == 0 and stale["per_kf"][2][j2] == c and stale["per_kf"][2][jn] == -1
    assert not FS.same_bits(stale["final"], seq["final"])


def test_plain_scene_and_empty_inputs(harness):
    S = _scene(23, crafted=False)
    _same(_run(harness, 0, S), _run(harness, 2, S))
    S["slots"][0][:] = -1  # the current key frame holds nothing: an all-null list
    _same(_run(harness, 0, S), _run(harness, 2, S))
    S2 = _scene(24, crafted=False)
    S2["kfs"], S2["slots"] = S2["kfs"][:1], S2["slots"][:1]  # no targets
    a = _run(harness, 0, S2)
    _same(a, _run(harness, 2, S2))
    assert a["counts"][4] == 1 and a["counts"][3] == 1


def test_two_camera_and_fisheye_key_frames_are_refused(harness):
    S = _scene(23, crafted=False)
    assert _run(harness, 4, S)["rc"] == -200
    assert _run(harness, 5, S)["rc"] == -200


def _host_rule(L, prob):
    LL, KK, RR, keep = A.fuse_structs(prob["lists"], prob["keyframes"])
    assert L.fuse_host_rule(LL, len(prob["lists"]), KK, len(prob["keyframes"]), RR) == 0
    return A.fuse_results(LL, KK, RR, keep, len(prob["lists"]))


def test_host_rule_equals_the_restatement(harness):
    """csrc/fuse_rule.hpp compiled for the host (projection, gates, level, candidate filters: the code k_fuse runs, and the linear
    scan in visiting order that stands in for the grid) gives the restatement's bits on random and constructed problems."""
    for n, c in ((257, 500), (1000, 500), (65, 1), (64, 0)):
        prob, want = FS.problem(n, c)
        FS.assert_equal(_host_rule(harness, prob), want, (n, c))
    for prob, want in (FS.five_keyframes(), FS.two_lists()):
        FS.assert_equal(_host_rule(harness, prob), want)
    prob, labels = FS.constructed()
    out = _host_rule(harness, prob)
    FS.check_constructed(prob, labels, out)
    FS.assert_equal(out, FS.restate(prob), "constructed")


@pytest.mark.gpu
def test_adaptor_end_to_end_on_gpu(harness, gpu_api):
    S = _scene(21)
    cpu, gpu = _run(harness, 0, S), _run(harness, 1, S)
    _same(gpu, cpu)
    assert gpu["counts"].tolist() == cpu["counts"].tolist() and gpu["counts"][2] >= 1
