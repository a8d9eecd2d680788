"""k_bow_descend, k_bow_vectors, k_bow_score (geoflowslam_amd/csrc/bow_vocab.hip) and k_bow_search (csrc/bow_search.hip) at the sizes
they are built for and their suites never reached: frames of 512 .. 4096 features (every sort width up to the second stride, the
scan's last wave, a run of 4096 serial additions, more than 1024 words), trees of six levels, ties across the two rounds of a
16-lane group, vectors of 4096 words, node lists of 2048 / 2049 / 4096 candidates (bits 31, 32 and 63 of a lane's chunk mask) and key
frames of 1025 / 4096 key-points.  Every comparison is byte equality with the sequential restatement; there is no tolerance.
tests/test_bow_capacity_cases.py holds the restatement to an independent Python statement on the same cases and asserts that each
case still hits its edge."""
import ctypes as C

import numpy as np
import pytest

import bow_search_support as BS
import bow_vocab_support as BV

pytestmark = pytest.mark.gpu

CASES = BV.capacity_cases()
BATCH, AFTER = "a batch of 4096, 0, 1 and 2049 features", "... then 5 features on the same handle"
REPEATED = "n = 4096, 3 % of the words stopped"


def _check_frames(got, want, what):
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        BV.assert_vectors_equal(g, w, (what, j))


def _same_bytes(a, b, what):
    for j, (x, y) in enumerate(zip(a, b)):
        for k in BV.VECTOR_KEYS:
            assert x[k].tobytes() == y[k].tobytes(), (what, j, k)


@pytest.fixture(scope="module")
def handles(gpu_api):
    """one handle of the capacity (4 frames of 4096 features) per vocabulary, shared by the module's tests"""
    made = {}

    def get(v):
        if id(v) not in made:
            made[id(v)] = (v, gpu_api.BowVocabulary(v, max_batch=4, max_features=4096))
        return made[id(v)][1]
    yield get
    for _, h in made.values():
        h.close()


@pytest.mark.parametrize("label", [l for l in CASES if l not in (BATCH, AFTER)])
def test_transform_cases(handles, label):
    c = CASES[label]
    got = handles(c["vocab"]).transform(c["descs"], c["levelsup"])
    _check_frames(got, c["want"], label)
    if c["hand"] is not None:
        BV.assert_vectors_equal(got[0], c["hand"], (label, "by hand"))


def test_ragged_batch_then_a_small_frame_on_the_same_handle(handles):
    c, s = CASES[BATCH], CASES[AFTER]
    voc = handles(c["vocab"])
    got = voc.transform(c["descs"], c["levelsup"])  # one call: the stride is 4096, the frames hold 4096, 0, 1 and 2049 features
    _check_frames(got, c["want"], BATCH)
    assert got[1]["node_start"].tolist() == [0] and len(got[1]["word_of_feature"]) == 0
    _check_frames(voc.transform(s["descs"], s["levelsup"]), s["want"], AFTER)  # nothing of the 4096 features is left behind
    _check_frames(voc.transform(c["descs"][::-1], c["levelsup"]), c["want"][::-1], "the batch in reverse order")


def test_transform_twice_and_on_a_fresh_handle(gpu_api, handles):
    c = CASES[REPEATED]
    voc = handles(c["vocab"])
    first, second = voc.transform(c["descs"], c["levelsup"]), voc.transform(c["descs"], c["levelsup"])
    fresh = gpu_api.BowVocabulary(c["vocab"], max_batch=1, max_features=4096)
    third = fresh.transform(c["descs"], c["levelsup"])
    fresh.close()
    _check_frames(first, c["want"], REPEATED)
    _same_bytes(first, second, "the same handle twice")
    _same_bytes(first, third, "a fresh handle")


def test_device_entry_refuses_a_count_above_the_stride(gpu_api, handles):
    """2049 features lie within the handle's 4096 but above a stride of 2048: the kernel finds it, the call is refused with
    GFS_ERR_CAPACITY, nothing is truncated, and the handle serves the same frame under a sufficient stride."""
    hip = C.CDLL("libamdhip64.so")  # the HIP runtime the library itself uses
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]

    def to_device(a):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), max(a.nbytes, 4)) == 0 and hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p
    c = CASES["n = 2049"]
    voc, d = handles(c["vocab"]), c["descs"][0]
    rows = 2064  # the buffer holds every row either stride names
    host = np.random.default_rng(2).integers(0, 256, (rows, 32)).astype(np.uint8)  # garbage in the padding
    host[:2049] = d
    counts = np.array([2049], np.int32)
    d_desc, d_counts = to_device(host), to_device(counts)
    try:
        with pytest.raises(gpu_api.GfsError) as e:
            voc.transform_device(d_desc.value, d_counts.value, 2048, 1, c["levelsup"], counts=counts)
        assert e.value.code == BV.ERR_CAPACITY
        _check_frames(voc.transform_device(d_desc.value, d_counts.value, rows, 1, c["levelsup"], counts=counts), c["want"], "stride 2064")
        _check_frames(voc.transform(c["descs"], c["levelsup"]), c["want"], "the host entry after the refusal")
    finally:
        for p in (d_desc, d_counts):
            hip.hipFree(p)


# ---------------------------------------------------------------- the database

@pytest.mark.parametrize("max_entries", [1, 4, 5, 70])
def test_query_vectors_of_4096_words(gpu_api, max_entries):
    queries, entries, stores = BV.capacity_database()
    dev, ref = gpu_api.BowDatabase(max_entries, 4096), BV.RestatedDatabase(max_entries)
    by_slot, order = {}, []
    for slot, name in stores[max_entries]:
        dev.add(slot, *entries[name])
        ref.add(slot, *entries[name])
        by_slot[slot] = entries[name]
        order.append(slot)
    for label, q in queries.items():
        got = dev.query(*q)
        BV.assert_query_equal(got, ref.query(*q), (max_entries, label))
        BV.assert_query_equal(got, BV.python_query(by_slot, order, max_entries, *q), (max_entries, label, "python"))
    BV.assert_query_equal(dev.query(*queries["4096 words"]), ref.query(*queries["4096 words"]), (max_entries, "the large query again"))
    dev.close()


# ---------------------------------------------------------------- SearchByBoW

SEARCH = BS.capacity_cases()
CHUNKS_64 = "one node, n2 = 4096: 64 chunks"


@pytest.fixture(scope="module")
def matcher(gpu_api):
    m = gpu_api.ProjectionMatcher(max_last=64, max_cur=4096, max_batch=1)
    m.reserve_bow(2, 8)
    yield m
    m.close()


@pytest.mark.parametrize("label", list(SEARCH))
def test_search_cases(matcher, label):
    prob, want = SEARCH[label]
    BS.assert_equal(matcher.search_by_bow(prob), want, label)


def test_a_4096_key_point_problem_beside_a_1_key_point_problem(matcher):
    (big, want_big), (small, want_small) = SEARCH["N1 = 4096 over 100 nodes"], SEARCH["one key-point"]
    for probs, wants in (([big, small], [want_big, want_small]), ([small, big], [want_small, want_big])):
        got = matcher.search_by_bow(probs)
        for g, w in zip(got, wants):
            BS.assert_equal(g, w, "mixed call")
    alone = matcher.search_by_bow(small)  # after the large call: the small problem alone, identical bytes
    BS.assert_equal(alone, want_small, "alone after the mixed call")
    BS.assert_equal(alone, got[0], "alone against inside the mixed call")


def test_search_twice_and_on_a_fresh_handle(gpu_api, matcher):
    prob, want = SEARCH[CHUNKS_64]
    first, second = matcher.search_by_bow(prob), matcher.search_by_bow(prob)
    fresh = gpu_api.ProjectionMatcher(max_last=64, max_cur=4096, max_batch=1)
    third = fresh.search_by_bow(prob)
    fresh.close()
    BS.assert_equal(first, want, CHUNKS_64)
    BS.assert_equal(second, first, "the same handle twice")
    BS.assert_equal(third, first, "a fresh handle")
