"""Shared by the SearchByBoW tests: builds and calls the sequential CPU restatement (tests/host/bow_search_restatement.cpp) and the
rule header's host build, the hand-built cases with the outputs their labels promise, and the random problems.  Not a test module."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from geoflowslam_amd import api, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "bow_search_restatement.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_bow_search_restatement.so")
_L = None

TRACES = ("accepted", "rejected_th_low", "rejected_ratio", "changed_by_taken", "removed_by_orientation")
CONSTANTS = ("TH_LOW", "HISTO_LENGTH", "initial_distance", "loop_nn_ratio", "loop_check_orientation", "nBoWMatches")
f32 = np.float32


def restatement():
    global _L
    if _L is None:
        csrc = os.path.join(ROOT, "geoflowslam_amd", "csrc")
        deps = [_SRC, os.path.join(csrc, "bow_search_rule.hpp"), os.path.join(csrc, "triangulate_rule.hpp"), os.path.join(ROOT, "include", "gfs_abi.h")]
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
            tmp = _SO + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-I" + os.path.join(ROOT, "include"),
                            "-I" + csrc, "-o", tmp, _SRC], check=True)
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        vp = C.c_void_p
        L.bw_search_by_bow.argtypes = [C.POINTER(api.BowProblem), C.c_int, C.POINTER(C.POINTER(api.BowResult)), vp]
        L.bw_rule_search_by_bow.argtypes = [C.POINTER(api.BowProblem), C.c_int, C.POINTER(C.POINTER(api.BowResult))]
        L.bw_rule_accept.argtypes = [C.c_int, C.c_int, C.c_float]
        L.bw_constants.argtypes = [vp]
        _L = L
    return _L


def _as_list(probs):
    single = isinstance(probs, dict)
    return single, ([probs] if single else list(probs))


def restate(probs, with_traces=False):
    """The restatement on one problem dict or a list -> what api.ProjectionMatcher.search_by_bow returns; with_traces adds an int64
    array [slots, 5] (TRACES), the slots problem by problem, key frame 2 by key frame 2."""
    single, pl = _as_list(probs)
    PP, RP, keep = api.bow_structs(pl)
    traces = np.zeros((max(sum(len(p["kf2"]) for p in pl), 1), 5), np.int64)
    assert restatement().bw_search_by_bow(PP, len(pl), RP, traces.ctypes.data) == 0
    out = api.bow_results(PP, RP, keep, len(pl))
    out = out[0] if single else out
    return (out, traces[:sum(len(p["kf2"]) for p in pl)]) if with_traces else out


def rule_host(probs):
    """The rule header's host build (gfs_bow::search_pair) on one problem dict or a list."""
    single, pl = _as_list(probs)
    PP, RP, keep = api.bow_structs(pl)
    assert restatement().bw_rule_search_by_bow(PP, len(pl), RP) == 0
    out = api.bow_results(PP, RP, keep, len(pl))
    return out[0] if single else out


def rule_accept(d1, d2, ratio):
    return bool(restatement().bw_rule_accept(int(d1), int(d2), float(f32(ratio))))


def rule_constants():
    out = np.zeros(len(CONSTANTS), np.float64)
    restatement().bw_constants(out.ctypes.data)
    return dict(zip(CONSTANTS, out.tolist()))


def assert_equal(got, want, what=""):
    """Byte equality of everything gfs_search_by_bow delivers for ONE problem, key frame 2 by key frame 2."""
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["n_matches"] == w["n_matches"], (what, i, g["n_matches"], w["n_matches"])
        assert g["match12"].dtype == w["match12"].dtype and g["match12"].tobytes() == w["match12"].tobytes(), \
            (what, i, np.nonzero(g["match12"] != w["match12"])[0][:8])


# ---------------------------------------------------------------- an independent statement in Python

_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def python_scan(dists):
    """The scan of :978-1006 over the distances of the candidates in list order, statement by statement (a candidate that the
    reference skips is given as 256: it improves on nothing) -> (bestDist1, position of bestIdx2 in the list or -1, bestDist2)"""
    bestDist1, bestPos2, bestDist2 = 256, -1, 256
    for i2, dist in enumerate(dists):
        dist = int(dist)
        if dist < bestDist1:
            bestDist2 = bestDist1
            bestDist1 = dist
            bestPos2 = i2
        elif dist < bestDist2:
            bestDist2 = dist
    return bestDist1, bestPos2, bestDist2


def numpy_scan(d):
    """python_scan on an int array in three numpy calls: the strict `<` keeps the FIRST position at the minimum; bestDist2 ends as the
    smallest of all other entries (an equal one included) and of the initial 256."""
    if len(d) == 0:
        return 256, -1, 256
    pos = int(d.argmin())
    best1 = int(d[pos])
    if best1 >= 256:
        return 256, -1, 256
    best2 = min(int(d[:pos].min()) if pos else 256, int(d[pos + 1:].min()) if pos + 1 < len(d) else 256, 256)
    return best1, pos, best2


def _round_half_away(x):
    """C's round() of a float that is exact as a double"""
    x = float(x)
    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))


def python_search(prob, detail=False):
    """An independent statement of ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) in sequential Python, written from the reference's
    text (src/ORBmatcher.cc:936-1053, ComputeThreeMaxima :2500-2532) and sharing nothing with bow_search_rule.hpp or the C++
    restatement: the feature vectors as dicts walked in key order with lower_bound, the scan of every idx1 in list order over the
    candidates that have a map point and are not in vbMatched2 (numpy only computes the node's Hamming distances and the scan's two
    minima, numpy_scan), TH_LOW, the float32 ratio product, rotHist as thirty lists, the three maxima and the 0.1f cuts.  A bin
    outside [0, 30) trips the reference's assert; as in DESIGN.md section 22 such a match is in no bin and the check removes it.
    -> what restate(prob) returns for ONE problem; detail=True adds per key frame 2 `before` (match12 before the orientation check) and
    `changed`: (idx1, list position of the candidate it would have taken had none been taken before it, or -1) of every idx1 whose
    outcome a taken candidate changed."""
    TH_LOW, HISTO_LENGTH = 50, 30
    factor = f32(1.0) / f32(HISTO_LENGTH)
    mfNNratio, mbCheckOrientation = f32(prob["nn_ratio"]), bool(prob.get("check_orientation", True))
    k1 = prob["kf1"]
    desc1, has1, ang1 = np.asarray(k1["desc"], np.uint8).reshape(-1, 32), np.asarray(k1["has_mp"]), np.asarray(k1["angle"], f32)

    def feature_vector(k):
        return {int(v): [int(i) for i in k["feat_idx"][a:b]] for v, a, b in zip(k["node_id"], k["node_start"][:-1], k["node_start"][1:])}

    def lower_bound(keys, v):
        lo, hi = 0, len(keys)
        while lo < hi:
            mid = (lo + hi) // 2
            if keys[mid] < v:
                lo = mid + 1
            else:
                hi = mid
        return lo

    vFeatVec1 = feature_vector(k1)
    keys1 = sorted(vFeatVec1)
    out = []
    for k2 in prob["kf2"]:
        desc2, has2, ang2 = np.asarray(k2["desc"], np.uint8).reshape(-1, 32), np.asarray(k2["has_mp"]), np.asarray(k2["angle"], f32)
        vFeatVec2 = feature_vector(k2)
        keys2 = sorted(vFeatVec2)
        vpMatches12 = [-1] * len(desc1)
        vbMatched2 = np.zeros(len(desc2), bool)
        rotHist = [[] for _ in range(HISTO_LENGTH)]
        no_bin, changed = [], []
        nmatches = 0
        f1it, f2it = 0, 0
        while f1it != len(keys1) and f2it != len(keys2):
            if keys1[f1it] == keys2[f2it]:
                list1, list2 = vFeatVec1[keys1[f1it]], np.array(vFeatVec2[keys2[f2it]], np.int64)
                eligible = [idx1 for idx1 in list1 if has1[idx1]]  # `if (!pMP1) continue; if (pMP1->isBad()) continue;`
                if eligible and len(list2):
                    dist = _POPCOUNT[desc1[eligible][:, None, :] ^ desc2[list2][None, :, :]].sum(-1, dtype=np.int32)  # DescriptorDistance
                    pMP2 = has2[list2] != 0
                    for row, idx1 in enumerate(eligible):
                        usable = pMP2 & ~vbMatched2[list2]  # `if (vbMatched2[idx2] || !pMP2) continue;`
                        bestDist1, pos, bestDist2 = numpy_scan(np.where(usable, dist[row], 256))
                        matched = False
                        if bestDist1 < TH_LOW:
                            if f32(bestDist1) < mfNNratio * f32(bestDist2):
                                bestIdx2 = int(list2[pos])
                                vpMatches12[idx1] = bestIdx2
                                vbMatched2[bestIdx2] = True
                                matched = True
                                if mbCheckOrientation:
                                    rot = ang1[idx1] - ang2[bestIdx2]
                                    if rot < 0.0:
                                        rot = rot + f32(360.0)
                                    b = _round_half_away(f32(rot * factor))
                                    if b == HISTO_LENGTH:
                                        b = 0
                                    (rotHist[b] if 0 <= b < HISTO_LENGTH else no_bin).append(idx1)
                                nmatches += 1
                        if detail:
                            fd1, fpos, fd2 = numpy_scan(np.where(pMP2, dist[row], 256))
                            free = fd1 < TH_LOW and bool(f32(fd1) < mfNNratio * f32(fd2))
                            if free != matched or (matched and fpos != pos):
                                changed.append((idx1, fpos if free else -1))
                f1it += 1
                f2it += 1
            elif keys1[f1it] < keys2[f2it]:
                f1it = lower_bound(keys1, keys2[f2it])
            else:
                f2it = lower_bound(keys2, keys1[f1it])
        before = np.array(vpMatches12, np.int32).reshape(-1)
        if mbCheckOrientation:
            max1 = max2 = max3 = 0
            ind1 = ind2 = ind3 = -1
            for i in range(HISTO_LENGTH):
                s = len(rotHist[i])
                if s > max1:
                    max3, max2, max1 = max2, max1, s
                    ind3, ind2, ind1 = ind2, ind1, i
                elif s > max2:
                    max3, max2 = max2, s
                    ind3, ind2 = ind2, i
                elif s > max3:
                    max3, ind3 = s, i
            if f32(max2) < f32(0.1) * f32(max1):
                ind2 = ind3 = -1
            elif f32(max3) < f32(0.1) * f32(max1):
                ind3 = -1
            for i in range(HISTO_LENGTH):
                if i == ind1 or i == ind2 or i == ind3:
                    continue
                for idx1 in rotHist[i]:
                    vpMatches12[idx1] = -1
                    nmatches -= 1
            for idx1 in no_bin:
                vpMatches12[idx1] = -1
                nmatches -= 1
        o = dict(match12=np.array(vpMatches12, np.int32).reshape(-1), n_matches=nmatches)
        if detail:
            o.update(before=before, changed=changed)
        out.append(o)
    return out


def list_positions(k2):
    """-> position of every key-point of a key frame in its node's list (-1: in no list)"""
    pos = np.full(len(k2["angle"]), -1, np.int64)
    for a, b in zip(k2["node_start"][:-1], k2["node_start"][1:]):
        pos[k2["feat_idx"][a:b]] = np.arange(b - a)
    return pos


# ---------------------------------------------------------------- hand-built cases

def bits(*ranges):
    """One descriptor with the bits of the given (first, count) ranges set."""
    b = np.zeros(256, np.uint8)
    for a, n in ranges:
        b[a:a + n] = 1
    return np.packbits(b)


def weight(n):
    """A descriptor at Hamming distance n from the zero descriptor."""
    return bits((0, n))


def kf(desc, nodes, has_mp=None, angle=None):
    """A hand-made key frame: desc = a list of descriptors, nodes = [(id, [indices in list order])]."""
    n = len(desc)
    return dict(angle=np.zeros(n, f32) if angle is None else np.asarray(angle, f32),
                desc=np.asarray(desc, np.uint8).reshape(n, 32) if n else np.zeros((0, 32), np.uint8),
                has_mp=np.ones(n, np.uint8) if has_mp is None else np.asarray(has_mp, np.uint8), node_id=np.array([k for k, _ in nodes], np.int32),
                node_start=np.concatenate([[0], np.cumsum([len(l) for _, l in nodes])]).astype(np.int32),
                feat_idx=np.array([i for _, l in nodes for i in l], np.int32))


def prob(k1, k2, nn_ratio=0.9, check_orientation=False):
    return dict(kf1=k1, kf2=k2 if isinstance(k2, list) else [k2], nn_ratio=f32(nn_ratio), check_orientation=check_orientation)


def _pairs_problem(pairs, **kw):
    """One idx1 (the zero descriptor) per node, its candidates at the given distances: pairs = [(d, ...), ...]."""
    d2, n1, n2 = [], [], []
    for i, ds in enumerate(pairs):
        n1.append((3 * i + 1, [i]))
        n2.append((3 * i + 1, list(range(len(d2), len(d2) + len(ds)))))
        d2 += [weight(d) for d in ds]
    return prob(kf([weight(0)] * len(pairs), n1), kf(d2, n2), **kw)


def _orientation_problem(angles, **kw):
    """One idx1 per node with its one candidate (distance 0): angles = [(angle1, angle2), ...] -> every pair matches before the check."""
    n = len(angles)
    nodes = [(i, [i]) for i in range(n)]
    return prob(kf([weight(0)] * n, nodes, angle=[a for a, _ in angles]), kf([weight(0)] * n, nodes, angle=[b for _, b in angles]), **kw)


def constructed():
    """Hand-made problems with the outputs their labels promise: -> {label: (problem, [match12 per key frame 2])}.  n_matches is the
    count of non-negative entries."""
    cases = {}
    # the ratio: with 0.9f the five ties d1 = 0.9 d2 are rejected (strict <), their neighbours accepted
    ties = [(9, 10), (18, 20), (27, 30), (36, 40), (45, 50), (8, 10), (44, 50)]
    cases["ratio ties rejected, neighbours accepted"] = (_pairs_problem(ties), [[-1, -1, -1, -1, -1, 10, 12]])
    # TH_LOW is strict; a single candidate leaves bestDist2 at 256
    cases["TH_LOW: 49 accepted, 50 rejected, single 49 accepted"] = (_pairs_problem([(49, 55), (50, 200), (49,)]), [[0, -1, 4]])
    cases["second best first in the list"] = (_pairs_problem([(55, 49), (200, 50), (20, 10, 30)]), [[1, -1, 5]])
    # the only candidate is the complement: distance 256 improves on nothing, bestIdx2 stays -1 and is never read
    cases["complement pair: no usable candidate"] = (prob(kf([weight(0)], [(4, [0])]), kf([weight(256)], [(4, [0])])), [[-1]])
    # two identical candidates at the minimum: bestDist2 == bestDist1, no match, and both stay available: the later idx1 1 has C at
    # 24 and the twins at 26, 24 < 0.9f * 26 = 23.4 is false (with the twins taken its second best would be 256)
    A, Cc = bits((0, 10)), bits((100, 40))
    cases["duplicate candidates match nothing and stay available"] = (
        prob(kf([weight(0), bits((100, 16))], [(4, [0, 1])]), kf([A, A, Cc], [(4, [0, 1, 2])])), [[-1, -1]])
    cases["... control: without the twins that idx1, now first in the list, matches"] = (
        prob(kf([weight(0), bits((100, 16))], [(4, [1, 0])]), kf([A, A, Cc], [(4, [0, 1, 2])], has_mp=[0, 0, 1])), [[-1, 2]])
    # equal best distances under a ratio above 1 (the third equal candidate has no map point): the first LIST position wins -- index
    # order would give 0, the last position 2
    eq = [bits((0, 20)), bits((20, 20)), bits((40, 20)), bits((60, 20))]
    cases["two at the best distance: first list position"] = (
        prob(kf([weight(0)], [(4, [0])]), kf(eq, [(4, [3, 1, 0, 2])], has_mp=[1, 1, 1, 0]), nn_ratio=1.5), [[1]])
    cases["... and never under a ratio below 1"] = (prob(kf([weight(0)], [(4, [0])]), kf(eq, [(4, [3, 1, 0, 2])], has_mp=[1, 1, 1, 0])), [[-1]])
    # taken candidates: P is 5 from idx1 0 and 2 from idx1 1, Q is 40 and 43.  In list order 0, 1 idx1 0 takes P and idx1 1 matches
    # its second, Q, under the changed ratio (43 against 256); in list order 1, 0 idx1 1 takes P and idx1 0 gets Q
    d1, d2 = [weight(0), weight(3)], [bits((0, 5)), bits((100, 40))]
    cases["taken candidate: list order 0, 1"] = (prob(kf(d1, [(4, [0, 1])]), kf(d2, [(4, [0, 1])])), [[0, 1]])
    cases["taken candidate: list order 1, 0"] = (prob(kf(d1, [(4, [1, 0])]), kf(d2, [(4, [0, 1])])), [[1, 0]])
    # interleaved ids so that both lower_bound branches run; a node in one frame only; empty lists on either side
    k1 = kf([weight(0)] * 6, [(1, [0]), (4, [1]), (6, []), (9, [2]), (12, [3]), (13, [4]), (30, [5])])
    k2 = kf([weight(10)] * 7, [(2, [0]), (4, [1]), (5, [2]), (6, [3]), (9, [4]), (10, []), (11, [5]), (12, []), (30, [6])])
    cases["interleaved node ids, one-sided nodes, empty lists"] = (prob(k1, k2), [[-1, 1, 4, -1, -1, 6]])
    # has_mp = 0 on either side
    k1 = kf([weight(0)] * 3, [(4, [0, 1, 2])], has_mp=[1, 0, 1])
    k2 = kf([weight(5), weight(6), weight(40)], [(4, [0, 1, 2])], has_mp=[0, 1, 1])
    cases["no map point on either side"] = (prob(k1, k2), [[1, -1, 2]])
    cases["several key frames 2, one without nodes"] = (prob(kf([weight(0)], [(4, [0])]), [kf([weight(3)], [(4, [0])]), kf([weight(3)], []),
                                                                                           kf([], []), kf([weight(60)], [(4, [0])])]), [[0], [-1], [-1], [-1]])
    cases["key frame 1 without key points"] = (prob(kf([], []), [kf([weight(3)], [(4, [0])])]), [[]])
    # ---- orientation.  Four bins of one match each: the first three in bin order are kept (equal counts: the lower index first)
    ang = [(15.0, 0.0), (45.0, 0.0), (75.0, 0.0), (105.0, 0.0)]  # bins 1, 2, 3, 4 (x.5 rounds away from zero)
    cases["orientation: bin boundaries, equal counts"] = (_orientation_problem(ang, check_orientation=True), [[0, 1, 2, -1]])
    cases["orientation: off"] = (_orientation_problem(ang, check_orientation=False), [[0, 1, 2, 3]])
    # 7.5 -> bin 0 (0.25), 14.0 -> bin 0, 15 -> bin 1, 22.5 -> bin 1 (0.75), 44.0 -> 1: bins 0 0 1 1 1, then singles in 5, 6
    ang = [(7.5, 0.0), (14.0, 0.0), (15.0, 0.0), (22.5, 0.0), (44.0, 0.0), (150.0, 0.0), (180.0, 0.0)]
    cases["orientation: 7.5 to the bin"] = (_orientation_problem(ang, check_orientation=True), [[0, 1, 2, 3, 4, 5, -1]])
    # a negative difference (10 - 20 + 360 = 350 -> bin 12) joins 345 and 359 in bin 12; 890 - 0 rounds to bin 30, which is bin 0, with 5
    ang = [(10.0, 20.0), (345.0, 0.0), (359.0, 0.0), (890.0, 0.0), (5.0, 0.0), (100.0, 0.0), (101.0, 0.0), (200.0, 0.0)]
    cases["orientation: negative difference, bin 30 is bin 0"] = (_orientation_problem(ang, check_orientation=True), [[0, 1, 2, 3, 4, 5, 6, -1]])
    # the 0.1 rule: 21 / 2 / 2 -> 2 < 0.1f * 21 cuts the second and the third; 20 / 2 / 1 -> 2 < 2 is false, 1 < 2 cuts the third
    ang = [(0.0, 0.0)] * 21 + [(60.0, 0.0)] * 2 + [(120.0, 0.0)] * 2
    cases["orientation: 0.1 rule cuts second and third"] = (_orientation_problem(ang, check_orientation=True), [list(range(21)) + [-1] * 4])
    ang = [(0.0, 0.0)] * 20 + [(60.0, 0.0)] * 2 + [(120.0, 0.0)]
    cases["orientation: 0.1 rule cuts the third"] = (_orientation_problem(ang, check_orientation=True), [list(range(22)) + [-1]])
    return cases


# ---------------------------------------------------------------- random problems

RATIOS = (0.6, 0.75, 0.9)


def sweep_problem(s):
    """Problem s of the 300 of the random sweep: n_kp <= 256, 1..11 key frames 2, 1..40 nodes, both check_orientation values, the
    three ratios; few bits flipped and many near-copies, so that candidates are taken and ratios fail."""
    rng = np.random.default_rng(5000 + s)
    n_kp = int(rng.integers(1, 257))
    return synth.bow_search_problem(9000 + s, n_kp=n_kp, n_kf2=1 + s % 11, n_nodes=1 + int(rng.integers(0, 40)),
                                    n_kp2=int(rng.integers(1, 257)), no_mp_frac=0.15, dup_frac=0.15, shuffle_lists=s % 4 != 3,
                                    nn_ratio=RATIOS[s % 3], check_orientation=s % 2 == 0)


@functools.lru_cache(maxsize=None)
def sweep():
    """The sweep's problems and their restatement with traces (computed once, shared, left unchanged)."""
    probs = [sweep_problem(s) for s in range(300)]
    want, traces = restate(probs, with_traces=True)
    return probs, want, traces


@functools.lru_cache(maxsize=None)
def problem(seed, n_kp, n_kp2, n_kf2=1, n_nodes=1, **kw):
    """A seeded problem of the GPU tests and its restatement (computed once, shared, left unchanged)."""
    p = synth.bow_search_problem(seed, n_kp=n_kp, n_kf2=n_kf2, n_nodes=n_nodes, n_kp2=n_kp2, **kw)
    return p, restate(p)


# ---------------------------------------------------------------- key frames of up to 4096 key-points

def capacity_cases():
    """Problems at the sizes where k_bow_search first uses the high bits of a lane's 64-bit chunk mask and a second stride of its
    per-key-point loops, each the smallest such shape: -> {label: (problem, restatement)}.  The seeds were chosen on the CPU so that the
    restatement accepts matches at the list positions and key-point indices that tests/test_bow_capacity_cases.py asserts."""
    one = dict(n_nodes=1, one_sided_frac=0.0, wrong_node_frac=0.0)
    return {
        "one node, n2 = 4096: 64 chunks": problem(21, 200, 4096, n_kf2=2, **one),
        "one node, n2 = 2048: 32 chunks": problem(3, 200, 2048, n_kf2=2, **one),
        "one node, n2 = 2049: 33 chunks": problem(11, 200, 2049, n_kf2=2, **one),
        "N1 = 1025 over 100 nodes": problem(3, 1025, 1025, n_kf2=4, n_nodes=100),
        "N1 = 4096 over 100 nodes": problem(3, 4096, 4096, n_kf2=2, n_nodes=100),
        "one key-point": problem(8, 1, 1, n_kf2=3, no_mp_frac=0.0, max_flip_bits=30, **one),
    }
