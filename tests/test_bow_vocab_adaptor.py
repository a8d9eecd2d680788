"""gfs_host::ComputeBoW and gfs_host::DetectNBestCandidates (geoflowslam_amd/host/gfs_adaptors.hpp) on mock KeyFrame / Map classes
(tests/host/bow_vocab_adaptor_test.cpp) against an independent statement of reference src/KeyFrameDatabase.cc:583-718 in plain
Python, with the host restatement as the transform and the query.  The GPU variants run the same scenes through the device entries."""
import ctypes as C

import numpy as np
import pytest

import bow_vocab_support as BV
from geoflowslam_amd import synth

N, MAX_ENTRIES, MAX_WORDS, ID_RANGE, CAP, N_CAND = 16, 20, 128, 600, 8, 3
Q = 0                      # the query key frame
CONNECTED = (1, 2)         # share its place and are connected to it
TWINS = (3, 4)             # identical BowVectors, no covisibles: equal accumulated scores
BAD_KF, OTHER_MAP, BAD_MAP, FAR = 5, (6, 7), 8, (9, 10)
MAPS = np.array([0, 0, 0, 0, 0, 0, 1, 1, 2, 0, 0, 0, 0, 0, 0, 0], np.int32)
# adds in an order that is not index order; 9 leaves and 13 takes its slot: a low slot with a late sequence number
SCRIPT = [(0, k) for k in (7, 3, 9, 1, 4, 11, 5, 2, 6, 8, 10, 12)] + [(1, 9), (0, 13), (0, 14), (2, Q), (1, 3), (1, 15), (2, Q), (0, 3), (2, Q)]
COVISIBLE = {12: [11, 13], 6: [7], 7: [6], 13: [5, 1]}  # (5 is bad and scores; 1 is connected and is never this query's)
# the words a key frame shares with the query's place: the bad key frame shares most, so that it sets maxCommonWords
COMMON = {1: 40, 2: 41, 3: 39, 4: 39, 5: 46, 6: 38, 7: 38, 8: 40, 9: 5, 10: 4, 11: 38, 12: 37, 13: 38, 14: 30, 15: 38}


def scene(seed=1):
    rng = np.random.default_rng(seed)
    ids_q = np.sort(rng.choice(ID_RANGE, 50, replace=False))
    others = np.setdiff1d(np.arange(ID_RANGE), ids_q)
    bow = [BV.bow_vector(seed * 100, 0, 0, ids=ids_q)]
    for k in range(1, N):
        ids = np.sort(np.concatenate([rng.choice(ids_q, COMMON[k], replace=False), rng.choice(others, 15 + int(rng.integers(20)), replace=False)]))
        bow.append(BV.bow_vector(seed * 100 + k, 0, 0, ids=ids))
    bow[TWINS[1]] = (bow[TWINS[0]][0].copy(), bow[TWINS[0]][1].copy())
    bad = np.zeros(N, np.int32)
    bad[BAD_KF] = 1
    return dict(bow=bow, bad=bad, map_bad=np.array([0, 0, 1], np.int32))


def run(sc, gpu=False):
    L = BV.harness()
    bow = sc["bow"]
    bs = np.concatenate([[0], np.cumsum([len(b[0]) for b in bow])]).astype(np.int32)
    bi, bv = np.concatenate([b[0] for b in bow]).astype(np.int32), np.concatenate([b[1] for b in bow]).astype(np.float64)
    cs = np.concatenate([[0], np.cumsum([len(COVISIBLE.get(k, [])) for k in range(N)])]).astype(np.int32)
    cv = np.array([c for k in range(N) for c in COVISIBLE.get(k, [])] + [0], np.int32)
    script = np.array(SCRIPT, np.int32)
    nq = int((script[:, 0] == 2).sum())
    conn_start = (np.arange(nq + 1) * len(CONNECTED)).astype(np.int32)
    conn = np.array(list(CONNECTED) * nq, np.int32)
    o = dict(loop=np.full((nq, CAP), -9, np.int32), merge=np.full((nq, CAP), -9, np.int32), counts=np.full((nq, 2), -9, np.int32),
             words=np.full((nq, N), -9, np.int32), score=np.full((nq, N), np.nan, np.float32), queried=np.full((nq, N), -9, np.int32),
             slot_of=np.full((nq, N), -9, np.int32))
    rc = L.bow_detect_test(int(gpu), N, bs.ctypes.data, bi.ctypes.data, bv.ctypes.data, MAPS.ctypes.data, len(sc["map_bad"]), sc["map_bad"].ctypes.data,
                           sc["bad"].ctypes.data, cs.ctypes.data, cv.ctypes.data, len(script), script.ctypes.data, conn_start.ctypes.data,
                           conn.ctypes.data, MAX_ENTRIES, MAX_WORDS, N_CAND, CAP, *[o[k].ctypes.data for k in ("loop", "merge", "counts", "words", "score", "queried", "slot_of")])
    assert rc == 0, rc
    return o


def expected(sc):
    """:583-718 in plain Python for every query of SCRIPT: the sharing list by the walk over per-word lists in add order, float
    arithmetic in np.float32, the stable sort, the split."""
    f32 = np.float32
    order, out = [], []
    for op, k in SCRIPT:
        if op == 0:
            order = [x for x in order if x != k] + [k]
        elif op == 1:
            order = [x for x in order if x != k]
        else:
            bow = sc["bow"]
            r = BV.python_query({x: bow[x] for x in order}, order, N, *bow[k])
            words, score, queried = np.zeros(N, np.int32), np.zeros(N, f32), np.zeros(N, np.int32)
            sharing = []
            for x in r["list"].tolist():
                if x in CONNECTED:
                    words[x] = 1
                    continue
                words[x], queried[x] = r["n_common"][x], 1
                sharing.append(x)
            loop, merge = [], []
            if sharing:
                min_common = int(f32(max(words[x] for x in sharing)) * f32(0.8))
                scored = [x for x in sharing if words[x] > min_common]
                for x in scored:
                    score[x] = r["score"][x]
                acc = []
                for x in scored:
                    best, best_kf, a = score[x], x, score[x]
                    for y in COVISIBLE.get(x, [])[:10]:
                        if not queried[y]:
                            continue
                        a = f32(a + score[y])
                        if score[y] > best:
                            best, best_kf = score[y], y
                    acc.append((a, best_kf))
                acc = sorted(acc, key=lambda t: -float(t[0]))  # stable
                added = set()
                for a, x in acc:
                    if not (len(loop) < N_CAND or len(merge) < N_CAND):
                        break
                    if sc["bad"][x] or x in added:
                        continue
                    if MAPS[x] == MAPS[k] and len(loop) < N_CAND:
                        loop.append(x)
                    elif MAPS[x] != MAPS[k] and len(merge) < N_CAND and not sc["map_bad"][MAPS[x]]:
                        merge.append(x)
                    added.add(x)
            out.append(dict(loop=loop, merge=merge, words=words, score=score, queried=queried, list=sharing, order=list(order),
                            acc=acc if sharing else []))
    return out


def _check(got, want):
    for q, w in enumerate(want):
        assert got["loop"][q][:got["counts"][q][0]].tolist() == w["loop"], (q, got["loop"][q], w["loop"])
        assert got["merge"][q][:got["counts"][q][1]].tolist() == w["merge"], (q, got["merge"][q], w["merge"])
        assert got["words"][q].tolist() == w["words"].tolist(), q
        assert got["score"][q].tobytes() == w["score"].tobytes(), q
        assert got["queried"][q].tolist() == w["queried"].tolist(), q


def test_scene_exercises_the_rules(api):
    """What the scenes must contain, checked on the CPU, before any comparison means anything."""
    sc = scene()
    want, got = expected(sc), run(sc)
    w = want[0]
    assert set(CONNECTED) <= set(np.nonzero(w["words"] == 1)[0].tolist()) and not set(CONNECTED) & set(w["list"])  # connected, sharing, excluded
    assert all(x in w["list"] for x in TWINS + OTHER_MAP + (BAD_KF, BAD_MAP, 13))
    accs = dict((x, a) for a, x in w["acc"])
    assert accs[TWINS[0]] == accs[TWINS[1]] and w["loop"].index(TWINS[0]) + 1 == w["loop"].index(TWINS[1])  # equal scores keep list order
    assert w["list"].index(TWINS[0]) < w["list"].index(TWINS[1])
    assert BAD_KF not in w["loop"] and BAD_MAP not in w["merge"] and set(w["merge"]) <= set(OTHER_MAP) and len(w["merge"]) > 0
    assert any(x in FAR for x in w["order"]) and not any(w["score"][x] for x in FAR)  # sharing too few words: never scored
    # list order differs from slot order, so the (first_word, sequence) rule decides
    slots = [int(got["slot_of"][0][x]) for x in w["list"]]
    assert slots != sorted(slots) and got["slot_of"][0][13] == 2 and got["slot_of"][0][9] == -1
    # the key frame erased between the queries is gone from the second, back (at the end of its lists) in the third
    assert TWINS[0] in want[0]["list"] and TWINS[0] not in want[1]["list"] and TWINS[0] in want[2]["list"]
    assert want[2]["list"].index(TWINS[1]) < want[2]["list"].index(TWINS[0]) and want[1]["loop"] != want[0]["loop"]


def test_detect_n_best_candidates(api):
    sc = scene()
    _check(run(sc), expected(sc))
    sc2 = scene(2)
    _check(run(sc2), expected(sc2))


@pytest.mark.gpu
def test_detect_n_best_candidates_gpu(gpu_api):
    for seed in (1, 2):
        sc = scene(seed)
        got = run(sc, gpu=True)
        _check(got, expected(sc))
        host = run(sc)
        for k in got:
            assert got[k].tobytes() == host[k].tobytes(), k


def _compute_bow(v, desc, gpu, keyframe_guard=1, guard_case=0):
    V, keep = BV.api.bow_vocabulary_struct(v)
    n = len(desc)
    o = dict(n_words=C.c_int32(-9), word_id=np.full(n + 2, -9, np.int32), word_value=np.full(n + 2, np.nan), n_nodes=C.c_int32(-9),
             node_id=np.full(n + 2, -9, np.int32), node_start=np.full(n + 3, -9, np.int32), feat_idx=np.full(n + 2, -9, np.int32))
    rc = BV.harness().bow_compute_bow_test(int(gpu), C.byref(V), desc.ctypes.data, n, keyframe_guard, guard_case,
                                           *[C.addressof(o[k]) if isinstance(o[k], C.c_int32) else o[k].ctypes.data
                                             for k in ("n_words", "word_id", "word_value", "n_nodes", "node_id", "node_start", "feat_idx")])
    assert rc == 0, rc
    nw, nn = o["n_words"].value, o["n_nodes"].value
    return dict(word_id=o["word_id"][:nw], word_value=o["word_value"][:nw], node_id=o["node_id"][:nn], node_start=o["node_start"][:nn + 1],
                feat_idx=o["feat_idx"][:o["node_start"][nn]], word_of_feature=None)


def _compute_bow_cases(gpu):
    v = BV.vocabulary(31, 4, 5, 0.1, 0.0, True)  # levelsup 4 of L = 5: the root's children
    desc = synth.bow_features(7, v, 150, 10, 0.3)
    rc, want = BV.restate(v, desc, 4)
    assert rc == 0 and len(want["node_id"]) > 1
    BV.assert_vectors_equal(_compute_bow(v, desc, gpu), want, "both empty")
    BV.assert_vectors_equal(_compute_bow(v, desc, gpu, keyframe_guard=0), want, "Frame: mBowVec empty")
    BV.assert_vectors_equal(_compute_bow(v, desc[:0], gpu), BV.restate(v, desc[:0], 4)[1], "no descriptors")
    kept = _compute_bow(v, desc, gpu, guard_case=1)  # both filled: untouched
    assert kept["word_id"].tolist() == [7] and kept["node_id"].tolist() == [3] and kept["feat_idx"].tolist() == [2]
    BV.assert_vectors_equal(_compute_bow(v, desc, gpu, keyframe_guard=1, guard_case=2), want, "KeyFrame: mFeatVec empty recomputes")
    kept = _compute_bow(v, desc, gpu, keyframe_guard=0, guard_case=2)  # Frame looks at mBowVec only
    assert kept["word_id"].tolist() == [7] and len(kept["node_id"]) == 0


def test_compute_bow(api):
    _compute_bow_cases(False)


@pytest.mark.gpu
def test_compute_bow_gpu(gpu_api):
    _compute_bow_cases(True)
