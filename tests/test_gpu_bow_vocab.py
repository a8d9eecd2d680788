"""gfs_bow_transform / gfs_bow_transform_device and gfs_bow_db_* on the GPU (include/gfs_abi.h section 18):
everything the device returns is compared byte for byte with the sequential CPU restatement (tests/host/bow_vocab_restatement.cpp):
ids, double values, lists, counts and float scores.  No tolerance anywhere: the rule fixes every rounding.  The shapes are the
smallest at which the kernels can go wrong: group and wave edges, children beyond one group's 16 lanes, irregular trees, empty and
full frames, slot counts that are no multiple of the waves of a workgroup, entries at the 64-word block edges."""
import ctypes as C

import numpy as np
import pytest

import bow_vocab_support as BV
from geoflowslam_amd import synth

pytestmark = pytest.mark.gpu


def _check_frames(got, want, what):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        BV.assert_vectors_equal(g, w, (what, j))


@pytest.mark.parametrize("label", list(BV.constructed()))
def test_constructed_cases(gpu_api, label):
    v, desc, levelsup, want = BV.constructed()[label]
    voc = gpu_api.BowVocabulary(v, max_batch=1, max_features=16)
    if want is None:
        with pytest.raises(gpu_api.GfsError) as e:
            voc.transform(desc, levelsup)
        assert e.value.code == BV.ERR_INVALID_ARG
        v2, desc2, levelsup2, want2 = BV.constructed()["... and accepted one level up"]
        BV.assert_vectors_equal(voc.transform(desc2, levelsup2), want2, label)  # the handle stays usable
        return
    BV.assert_vectors_equal(voc.transform(desc, levelsup), want, label)


TREES = {
    "k=10 L=4, 300 features, duplicates, stopped words": dict(seed=3, k=10, L=4, counts=(300,)),
    "irregular tree, shuffled children": dict(seed=4, k=5, L=4, counts=(200, 77), prune_frac=0.3, shuffle_children=True),
    "k=17: the group loops": dict(seed=5, k=17, L=2, counts=(150,)),
    "k=20: the group loops": dict(seed=6, k=20, L=2, counts=(150,)),
    "k=1": dict(seed=7, k=1, L=3, counts=(40,)),
    "group and wave edges": dict(seed=8, k=10, L=3, counts=(63, 64, 65, 15, 16, 17)),
}


@pytest.mark.parametrize("label", list(TREES))
def test_trees(gpu_api, label):
    v, descs, levelsup, want = BV.problem(**TREES[label])
    voc = gpu_api.BowVocabulary(v, max_batch=len(descs), max_features=320)
    _check_frames(voc.transform(descs, levelsup), want, label)
    if label.startswith("k=10 L=4"):
        w = want[0]
        assert (w["word_of_feature"] < 0).any() and len(w["word_id"]) < int((w["word_of_feature"] >= 0).sum()) and len(w["node_id"]) > 1


def test_batch_of_empty_one_and_full_frames(gpu_api):
    v, descs, levelsup, want = BV.problem(9, 10, 3, (0, 1, 256))
    voc = gpu_api.BowVocabulary(v, max_batch=3, max_features=256)
    got = voc.transform(descs, levelsup)
    _check_frames(got, want, "0, 1, max_features")
    assert len(got[0]["word_id"]) == 0 and got[0]["node_start"].tolist() == [0] and len(got[0]["word_of_feature"]) == 0
    assert voc.transform([], levelsup) == []  # B == 0


def test_large_then_small_call_and_two_handles(gpu_api):
    v1, d1, l1, w1 = BV.problem(10, 10, 3, (256, 200))
    v2, d2, l2, w2 = BV.problem(11, 4, 4, (9,), prune_frac=0.2, shuffle_children=True)
    a, b = gpu_api.BowVocabulary(v1, max_batch=2, max_features=256), gpu_api.BowVocabulary(v2, max_batch=2, max_features=64)
    _check_frames(a.transform(d1, l1), w1, "large")
    _check_frames(b.transform(d2, l2), w2, "other handle")
    _check_frames([a.transform(d1[1][:5], l1)], [BV.restate(v1, d1[1][:5], l1)[1]], "small after large")
    _check_frames(b.transform(d2, l2), w2, "other handle again")
    _check_frames(a.transform(d1, l1), w1, "large again")


def test_device_descriptor_entry(gpu_api):
    hip = C.CDLL("libamdhip64.so")  # the HIP runtime the library itself uses
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]

    def to_device(a):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(a.nbytes, 4)) == 0 and hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p
    v, descs, levelsup, want = BV.problem(12, 10, 3, (100, 0, 33))
    stride = 112
    rng = np.random.default_rng(1)
    host = rng.integers(0, 256, (3, stride, 32)).astype(np.uint8)  # garbage in the padding
    for j, d in enumerate(descs):
        host[j, :len(d)] = d
    counts = np.array([len(d) for d in descs], np.int32)
    d_desc, d_counts = to_device(host), to_device(counts)
    voc = gpu_api.BowVocabulary(v, max_batch=3, max_features=128)
    got = voc.transform_device(d_desc.value, d_counts.value, stride, 3, levelsup, counts=counts)
    _check_frames(got, want, "device entry")
    _check_frames(got, voc.transform(descs, levelsup), "device entry against host entry")
    # a frame with more key-points than the handle holds is found by the kernel: refused, nothing truncated, the handle usable
    small = gpu_api.BowVocabulary(v, max_batch=3, max_features=64)
    with pytest.raises(gpu_api.GfsError) as e:
        small.transform_device(d_desc.value, d_counts.value, stride, 3, levelsup, counts=counts)
    assert e.value.code == BV.ERR_CAPACITY
    _check_frames(small.transform(descs[2:], levelsup), want[2:], "after the refusal")
    for p in (d_desc, d_counts):
        hip.hipFree(p)


def test_chain_into_search_by_bow(gpu_api):
    """The transform's feature vectors of two frames straight into gfs_search_by_bow, against the restatement of both steps."""
    import bow_search_support as BS
    v = BV.vocabulary(13, 10, 3, 0.05)
    d1 = synth.bow_features(1300, v, 200, 8, 0.1)
    d2 = synth._flip_bits(np.random.default_rng(5), d1[np.random.default_rng(6).permutation(200)], np.random.default_rng(7).integers(0, 12, 200))
    voc = gpu_api.BowVocabulary(v, max_batch=2, max_features=256)
    levelsup = 2  # the nodes are the root's children: lists long enough to compete
    got = voc.transform([d1, d2], levelsup)
    rc, want = BV.restate(v, [d1, d2], levelsup)
    assert rc == 0
    _check_frames(got, want, "chain")
    rng = np.random.default_rng(8)

    def kf(desc, r):
        return dict(angle=(rng.random(len(desc)) * 360).astype(np.float32), desc=desc, has_mp=(rng.random(len(desc)) > 0.1).astype(np.uint8),
                    node_id=r["node_id"], node_start=r["node_start"], feat_idx=r["feat_idx"])
    k1, k2 = kf(d1, got[0]), kf(d2, got[1])
    prob = dict(kf1=k1, kf2=[k2], nn_ratio=np.float32(0.9), check_orientation=False)
    res = gpu_api.ProjectionMatcher(max_last=64, max_cur=256, max_batch=1).search_by_bow(prob)
    ref = BS.restate(dict(prob, kf1=dict(k1, **{k: want[0][k] for k in ("node_id", "node_start", "feat_idx")}),
                          kf2=[dict(k2, **{k: want[1][k] for k in ("node_id", "node_start", "feat_idx")})]))
    BS.assert_equal(res, ref, "chain")
    assert res[0]["n_matches"] > 20


def test_transform_refusals(gpu_api):
    v, descs, levelsup, want = BV.problem(14, 10, 3, (20, 7))
    voc = gpu_api.BowVocabulary(v, max_batch=2, max_features=32)
    L = gpu_api.lib()

    def refused(code, fn, *a):
        with pytest.raises(gpu_api.GfsError) as e:
            fn(*a)
        assert e.value.code == code, (e.value.code, code)
        _check_frames(voc.transform(descs, levelsup), want, "after a refusal")  # the handle stays usable, the bytes right

    refused(BV.ERR_CAPACITY, voc.transform, descs + descs[:1], levelsup)                     # B > max_batch
    refused(BV.ERR_CAPACITY, voc.transform, [synth.bow_features(1, v, 33)], levelsup)       # n > max_features
    refused(BV.ERR_INVALID_ARG, voc.transform, descs, -1)                                   # levelsup < 0
    VV, keep = gpu_api.bow_vectors_alloc(1, 32)
    n = np.array([-1], np.int32)
    ptr = (C.c_void_p * 1)(descs[0].ctypes.data)
    assert L.gfs_bow_transform(voc.h, ptr, n.ctypes.data, 1, levelsup, VV) == BV.ERR_INVALID_ARG            # n < 0
    n[0] = 5
    assert L.gfs_bow_transform(voc.h, None, n.ctypes.data, 1, levelsup, VV) == BV.ERR_INVALID_ARG           # a NULL array
    assert L.gfs_bow_transform(voc.h, (C.c_void_p * 1)(None), n.ctypes.data, 1, levelsup, VV) == BV.ERR_INVALID_ARG
    VV[0].node_start = None
    assert L.gfs_bow_transform(voc.h, ptr, n.ctypes.data, 1, levelsup, VV) == BV.ERR_INVALID_ARG
    _check_frames(voc.transform(descs, levelsup), want, "after the NULL refusals")


def test_create_refusals(gpu_api):
    ok, bad = BV.malformed()
    gpu_api.BowVocabulary(ok, 1, 16)
    for label, v in bad.items():
        with pytest.raises(gpu_api.GfsError) as e:
            gpu_api.BowVocabulary(v, 1, 16)
        assert e.value.code == BV.ERR_INVALID_ARG, label
    with pytest.raises(gpu_api.GfsError) as e:
        gpu_api.BowVocabulary(ok, 1, 4097)
    assert e.value.code == BV.ERR_UNSUPPORTED
    with pytest.raises(gpu_api.GfsError) as e:
        gpu_api.BowDatabase(4, 4097)
    assert e.value.code == BV.ERR_UNSUPPORTED


# ---------------------------------------------------------------- the database

MAX_ENTRIES, MAX_WORDS, ID_RANGE = 70, 200, 1000  # 70: no multiple of the four waves of a workgroup


def _both(gpu_api):
    return gpu_api.BowDatabase(MAX_ENTRIES, MAX_WORDS), BV.RestatedDatabase(MAX_ENTRIES)


def test_query_entry_sizes_and_common_counts(gpu_api):
    dev, ref = _both(gpu_api)
    q = BV.bow_vector(1, 150, ID_RANGE)
    BV.assert_query_equal(dev.query(*q), ref.query(*q), "empty database")
    rng = np.random.default_rng(2)
    others = np.setdiff1d(np.arange(ID_RANGE), q[0])
    entries = {}
    # entries of 1, 63, 64, 65, 129 and max_words words (random overlap with the query)
    for slot, n in zip((0, 5, 6, 7, 33, 69), (1, 63, 64, 65, 129, MAX_WORDS)):
        entries[slot] = BV.bow_vector(100 + slot, n, ID_RANGE)
    # common counts of exactly 0, 1, 64 and 65
    for slot, c in zip((10, 11, 12, 13), (0, 1, 64, 65)):
        ids = np.sort(np.concatenate([rng.choice(q[0], c, replace=False), rng.choice(others, 100 - c, replace=False)]))
        entries[slot] = BV.bow_vector(200 + slot, 0, 0, ids=ids)
    # the single common word at the last id of both vectors
    entries[20] = BV.bow_vector(300, 0, 0, ids=np.concatenate([others[others < q[0][-1]][:40], q[0][-1:]]))
    entries[21] = (q[0].copy(), q[1].copy())  # an entry identical to the query
    for s, e in entries.items():
        dev.add(s, *e)
        ref.add(s, *e)
    got, want = dev.query(*q), ref.query(*q)
    BV.assert_query_equal(got, want, "sizes and counts")
    assert got["n_common"][[10, 11, 12, 13]].tolist() == [0, 1, 64, 65] and got["n_common"][20] == 1 and got["first_word"][20] == q[0][-1]
    assert got["score"][21] == np.float32(1.0) and got["n_common"][21] == 150 and got["n_common"][69] > 0  # the highest slot
    BV.assert_query_equal(got, BV.rule_query(entries, MAX_ENTRIES, *q), "rule")
    BV.assert_query_equal(dev.query(np.zeros(0, np.int32), np.zeros(0)), ref.query(np.zeros(0, np.int32), np.zeros(0)), "empty query")
    # erase then re-add of a slot; add replacing an occupied slot; erase of an empty slot
    for db in (dev, ref):
        db.erase(12)
        db.erase(12)
        db.erase(50)
    BV.assert_query_equal(dev.query(*q), ref.query(*q), "after erase")
    assert dev.query(*q)["n_common"][12] == 0
    for db in (dev, ref):
        db.add(12, *entries[13])
        db.add(7, *entries[0])  # 65 words replaced by one: nothing of the old entry is left
    got = dev.query(*q)
    BV.assert_query_equal(got, ref.query(*q), "after re-add and replace")
    assert got["n_common"][12] == 65 and got["n_common"][7] == got["n_common"][0]


def test_query_refusals(gpu_api):
    dev, ref = _both(gpu_api)
    q = BV.bow_vector(3, 120, ID_RANGE)
    e = BV.bow_vector(4, 90, ID_RANGE)
    dev.add(3, *e)
    ref.add(3, *e)
    want = ref.query(*q)
    big = BV.bow_vector(5, MAX_WORDS + 1, ID_RANGE)
    unsorted = (np.array([5, 4, 9], np.int32), np.array([0.2, 0.3, 0.5]))
    twice = (np.array([4, 4, 9], np.int32), np.array([0.2, 0.3, 0.5]))
    negative = (np.array([-1, 4, 9], np.int32), np.array([0.2, 0.3, 0.5]))
    nan = (np.array([1, 4, 9], np.int32), np.array([0.2, np.nan, 0.5]))
    inf = (np.array([1, 4, 9], np.int32), np.array([0.2, 0.3, np.inf]))
    calls = [(BV.ERR_CAPACITY, dev.query, big), (BV.ERR_CAPACITY, dev.add, (1,) + big)]
    for bad in (unsorted, twice, negative, nan, inf):
        calls += [(BV.ERR_INVALID_ARG, dev.query, bad), (BV.ERR_INVALID_ARG, dev.add, (1,) + bad)]
    calls += [(BV.ERR_INVALID_ARG, dev.add, (-1,) + e), (BV.ERR_INVALID_ARG, dev.add, (MAX_ENTRIES,) + e), (BV.ERR_INVALID_ARG, dev.erase, (-1,)),
              (BV.ERR_INVALID_ARG, dev.erase, (MAX_ENTRIES,))]
    for code, fn, a in calls:
        with pytest.raises(gpu_api.GfsError) as err:
            fn(*a)
        assert err.value.code == code, (fn, a[0], err.value.code)
        BV.assert_query_equal(dev.query(*q), want, "after a refusal")  # the handle stays usable, slot 1 stays empty
