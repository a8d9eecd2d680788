"""The cases of tests/test_gpu_bow_capacity.py on the CPU (frames of up to 4096 features, entries of up to 4096 words, key frames of up
to 4096 key-points; DESIGN.md sections 22 and 24).  For every case: the sequential restatement equals an independent statement in
plain Python byte for byte (python_transform, python_query, python_search), and the case still has the property it was built for,
computed from the restatement's output: the sort width, the survivors, the words, the chunks, the list positions and key-point indices
of the matches, the trace counts.  A changed generator fails here instead of silently testing less.  No GPU."""
import inspect

import numpy as np
import pytest

import bow_search_support as BS
import bow_vocab_support as BV

# ---------------------------------------------------------------- the transform

CASES = BV.capacity_cases()


def _survivors(w):
    return int((w["word_of_feature"] >= 0).sum())


@pytest.mark.parametrize("label", list(CASES))
def test_transform_restatement_equals_python_and_rule(label):
    c = CASES[label]
    rrc, rule, why = BV.rule_host(c["vocab"], c["descs"], c["levelsup"])
    assert rrc == 0, why
    for j, (d, w) in enumerate(zip(c["descs"], c["want"])):
        BV.assert_vectors_equal(w, BV.python_transform(c["vocab"], d, c["levelsup"]), (label, "python", j))
        BV.assert_vectors_equal(w, rule[j], (label, "rule", j))
        assert len(w["word_of_feature"]) == len(d) and len(w["feat_idx"]) == _survivors(w) == w["node_start"][-1]
        if c["hand"] is not None:
            BV.assert_vectors_equal(w, c["hand"], (label, "by hand"))


def test_frame_sizes_reach_every_sort_width():
    """P = 512 (half the threads hold a key), 1024 from both sides, 2048 (every thread of the bitonic loop active) from both sides, 4096
    (a second stride) from 2049, 4095 and 4096; in every frame a few stopped features, so that the survivors end inside the last tenth."""
    assert [BV.sort_width(n) for n in BV.CAPACITY_SIZES] == [512, 1024, 1024, 2048, 2048, 4096, 4096, 4096]
    assert [BV.sort_width(n) for n in (1, 64, 65, 300, 320)] == [64, 64, 128, 512, 512]  # ... and the suite's sizes until now: <= 512
    for n in BV.CAPACITY_SIZES:
        c = CASES["n = %d" % n]
        w = c["want"][0]
        assert len(c["descs"][0]) == n and BV.rule_validate(c["vocab"])[0] == 4096
        assert n * 9 // 10 < _survivors(w) < n and len(w["word_id"]) < _survivors(w)  # stopped features, words that several features share
        assert len(w["node_id"]) == 64 and BV.node_depths(c["vocab"])[w["node_id"]].tolist() == [2] * 64


def test_full_frames():
    none, few, every = (CASES["n = 4096, " + s]["want"][0] for s in ("no stopped word", "3 % of the words stopped", "every word stopped"))
    # no stopped word: m == P == 4096, the last survivor is the last key; more than 1024 words: the norm loop runs more than 16 rounds
    assert _survivors(none) == 4096 == BV.sort_width(4096) and len(none["word_id"]) > 1024 and len(none["word_id"]) == 2084
    assert abs(none["word_value"].sum() - 1.0) < 1e-12
    # stopped words, and the survivors still reach wave 15 of the scan (keys 3840 ..)
    assert 3841 <= _survivors(few) < 4096 and _survivors(few) == 3952
    assert (CASES["n = 4096, 3 % of the words stopped"]["descs"][0] == CASES["n = 4096, no stopped word"]["descs"][0]).all()
    # every word stopped
    assert _survivors(every) == 0 and len(every["word_id"]) == len(every["node_id"]) == len(every["feat_idx"]) == 0
    assert every["node_start"].tolist() == [0] and (every["word_of_feature"] == -1).all() and len(every["word_of_feature"]) == 4096
    # one word: a run of 4096 serial additions
    one = CASES["4096 copies of one descriptor"]["want"][0]
    assert one["word_id"].tolist() == [1234] and one["word_value"].tolist() == [1.0] and one["feat_idx"].tolist() == list(range(4096))
    assert len(one["node_id"]) == 1 and one["node_start"].tolist() == [0, 4096] and (one["word_of_feature"] == 1234).all()


def test_ragged_batch_and_the_small_frame_after_it():
    c = CASES["a batch of 4096, 0, 1 and 2049 features"]
    assert [len(d) for d in c["descs"]] == [4096, 0, 1, 2049] and [BV.sort_width(max(len(d), 1)) for d in c["descs"]] == [4096, 64, 64, 4096]
    w = c["want"]
    assert _survivors(w[0]) > 3840 and len(w[1]["word_id"]) == 0 and w[1]["node_start"].tolist() == [0] and _survivors(w[3]) > 1024
    assert len(w[2]["word_of_feature"]) == 1
    s = CASES["... then 5 features on the same handle"]
    assert s["vocab"] is c["vocab"] and len(s["descs"][0]) == 5 and 0 < _survivors(s["want"][0]) <= 5


def test_deep_trees():
    c = CASES["k = 3, L = 6, levelsup = 4"]
    v, w = c["vocab"], c["want"][0]
    depth = BV.node_depths(v)
    assert (v["k"], v["L"], c["levelsup"]) == (3, 6, 4) and BV.rule_validate(v) == (729, 6) and depth.max() == 6
    assert set(depth[w["node_id"]].tolist()) == {2} and len(w["node_id"]) > 1 and _survivors(w) < 300  # the nodes two levels down; stopped words
    c = CASES["k = 10, L = 6, pruned, shuffled children"]
    v, w = c["vocab"], c["want"][0]
    depth = BV.node_depths(v)
    leaf_of_word = np.zeros(BV.rule_validate(v)[0], np.int64)
    leaf_of_word[v["word_id"][v["word_id"] >= 0]] = np.nonzero(v["word_id"] >= 0)[0]
    reached = depth[leaf_of_word[w["word_id"]]]
    assert (v["k"], v["L"]) == (10, 6) and v["n_nodes"] < 1000 and depth.max() == 6 and BV.rule_validate(v)[1] == 1 and c["levelsup"] == 5
    assert reached.max() == 6 and reached.min() < 6  # six dependent levels, and leaves that end the descent early
    assert set(depth[v["word_id"] >= 0].tolist()) == {1, 2, 3, 4, 5, 6}
    kids = [v["children"][a:b] for a, b in zip(v["child_start"][:-1], v["child_start"][1:]) if b - a == 10]
    assert len(kids) > 10 and any((np.diff(k) < 0).any() for k in kids)  # child ids neither contiguous nor ascending


@pytest.mark.parametrize("lo,hi", BV.TIE_PAIRS)
def test_ties_across_the_rounds_of_a_group_by_hand(lo, hi):
    """Child c of a node is looked at by lane c % 16 of the feature's group in round c // 16."""
    if (lo, hi) == (2, 17):
        assert hi // 16 == 1 and lo // 16 == 0 and hi % 16 < lo % 16  # a later round of a LOWER lane against a first round
    else:
        assert hi == lo + 16  # one lane's first round against its second
    for moved, winner in ((False, lo), (True, hi)):
        label = ("k = 20: positions %d and %d tie, the lower wins" % (lo, hi)) if not moved else \
            ("k = 20: position %d one bit further, position %d wins" % (lo, hi))
        c = CASES[label]
        v, f = c["vocab"], np.unpackbits(c["descs"][0][0])
        kids = v["children"][v["child_start"][0]:v["child_start"][1]]
        dist = [int((np.unpackbits(v["desc"][k]) != f).sum()) for k in kids]  # the distances, counted bit by bit
        assert len(kids) == 20 and dist[hi] == 4 and dist[lo] == (5 if moved else 4) and min(d for i, d in enumerate(dist) if i not in (lo, hi)) >= 30
        first_of_min = dist.index(min(dist))  # `if (d < best_d)` over the children in order
        assert first_of_min == winner and v["word_id"][kids[winner]] == winner
        assert c["want"][0]["word_id"].tolist() == [winner] and c["want"][0]["word_of_feature"].tolist() == [winner]


# ---------------------------------------------------------------- the database

def _store(max_entries):
    queries, entries, stores = BV.capacity_database()
    db, by_slot, order = BV.RestatedDatabase(max_entries), {}, []
    for slot, name in stores[max_entries]:
        db.add(slot, *entries[name])
        by_slot[slot] = entries[name]
        order.append(slot)
    return db, by_slot, order, {name: slot for slot, name in stores[max_entries]}


@pytest.mark.parametrize("max_entries", [1, 4, 5, 70])
def test_query_restatement_equals_python_and_rule(max_entries):
    queries, entries, stores = BV.capacity_database()
    db, by_slot, order, slot_of = _store(max_entries)
    for label, q in queries.items():
        got = db.query(*q)
        want = BV.python_query(by_slot, order, max_entries, *q)
        BV.assert_query_equal(got, want, (max_entries, label, "python"))
        assert got["list"].tolist() == want["list"].tolist()
        BV.assert_query_equal(BV.rule_query(by_slot, max_entries, *q), got, (max_entries, label, "rule"))


def test_database_cases_have_their_properties():
    queries, entries, stores = BV.capacity_database()
    q, q1 = queries["4096 words"], queries["one word, the last of the 4096-word entry"]
    assert len(q[0]) == 4096 and len(q1[0]) == 1 and (np.diff(q[0]) > 0).all()
    assert [len(entries[k][0]) for k in ("4095 words", "4096 words", "4096 words, none common", "one word")] == [4095, 4096, 4096, 1]
    assert sorted(stores) == [1, 4, 5, 70] and all(max(s for s, _ in stores[e]) == e - 1 for e in stores)  # the highest slot is used
    assert {n for _, n in stores[70]} == set(entries)
    db, by_slot, order, slot_of = _store(70)
    got = db.query(*q)
    assert got["n_common"][slot_of["identical to the query"]] == 4096 and got["first_word"][slot_of["identical to the query"]] == q[0][0]
    last = slot_of["one common word, the last id of both"]
    assert got["n_common"][last] == 1 and got["first_word"][last] == q[0][-1] == by_slot[last][0][-1]
    assert got["n_common"][slot_of["4096 words, none common"]] == 0 and got["score"][slot_of["4096 words, none common"]] == 0
    assert got["n_common"][slot_of["one word"]] == 1 and got["first_word"][slot_of["one word"]] == q[0][2000]
    for k in ("4095 words", "4096 words"):  # random overlap: common words in many of the 64 blocks of an entry
        common = np.nonzero(np.isin(entries[k][0], q[0]))[0]
        assert got["n_common"][slot_of[k]] == len(common) > 64 and len(set((common // 64).tolist())) == 64
    got1 = db.query(*q1)
    e = entries["4096 words"][0]
    assert q1[0][0] == e[-1] and got1["n_common"][slot_of["4096 words"]] == 1 and got1["first_word"][slot_of["4096 words"]] == e[-1]
    assert got1["n_common"].sum() == 1 + int(np.isin(q1[0], entries["4095 words"][0]).sum()) + int(np.isin(q1[0], q[0]).sum())


# ---------------------------------------------------------------- SearchByBoW

def test_python_search_shares_nothing_with_the_rule():
    src = "".join(inspect.getsource(f) for f in (BS.python_search, BS.python_scan, BS.numpy_scan, BS._round_half_away))
    assert "restatement(" not in src and "rule_" not in src and "restate(" not in src.replace("what restate(prob) returns", "")
    c = BS.rule_constants()  # its literals, cross-checked only
    assert "TH_LOW, HISTO_LENGTH = 50, 30" in src and "bestDist1, bestPos2, bestDist2 = 256, -1, 256" in src
    assert (c["TH_LOW"], c["HISTO_LENGTH"], c["initial_distance"]) == (50, 30, 256)


def test_numpy_scan_is_the_sequential_scan():
    rng = np.random.default_rng(1)
    for trial in range(2000):
        n = int(rng.integers(0, 12))
        d = rng.choice([3, 7, 7, 20, 49, 50, 255, 256], n) if trial % 2 else rng.integers(0, 257, n)
        assert BS.numpy_scan(np.asarray(d, np.int64)) == BS.python_scan(d), d
    assert BS.python_scan([256, 256]) == (256, -1, 256) and BS.python_scan([7, 7]) == (7, 0, 7) and BS.python_scan([9, 7, 8]) == (7, 1, 8)


def test_python_search_equals_restatement_on_the_constructed_cases():
    for label, (prob, want) in BS.constructed().items():
        got = BS.python_search(prob)
        assert [o["match12"].tolist() for o in got] == want, label  # the answers stated by hand
        BS.assert_equal(got, BS.restate(prob), label)


def test_python_search_equals_restatement_on_the_sweep():
    probs, want, traces = BS.sweep()
    slot = 0
    for b, (p, w) in enumerate(zip(probs, want)):
        got = BS.python_search(p, detail=True)
        BS.assert_equal(got, w, ("sweep", b))
        for g in got:  # ... and its own count of the outcomes changed by a taken candidate is the restatement's trace
            assert len(g["changed"]) == traces[slot, 3], ("sweep", b)
            slot += 1
    assert slot == len(traces)


SEARCH = BS.capacity_cases()


@pytest.mark.parametrize("label", list(SEARCH))
def test_python_search_equals_restatement_on_the_capacity_cases(label):
    prob, want = SEARCH[label]
    BS.assert_equal(BS.python_search(prob), want, label)


def _match_positions(prob, res):
    """per key frame 2 the list positions (within their node) of the matched idx2, ascending"""
    return [np.sort(BS.list_positions(k2)[o["match12"][o["match12"] >= 0]]) for k2, o in zip(prob["kf2"], res)]


def _one_node(prob, n1, n2):
    assert prob["kf1"]["node_start"].tolist() == [0, n1] and all(k["node_start"].tolist() == [0, n2] for k in prob["kf2"])
    assert all(k["node_id"].tolist() == prob["kf1"]["node_id"].tolist() for k in prob["kf2"])
    return (n2 + 63) // 64


def test_64_chunks_use_the_high_bits_of_the_mask():
    prob, want = SEARCH["one node, n2 = 4096: 64 chunks"]
    assert _one_node(prob, 200, 4096) == 64
    pos = _match_positions(prob, want)
    assert max(p.max() for p in pos) >= 4032 and all((p >= 2048).sum() > 10 for p in pos)  # chunk 63; bits 32 .. 63 set and read
    _, traces = BS.restate(prob, with_traces=True)
    detail = BS.python_search(prob, detail=True)
    assert [len(d["changed"]) for d in detail] == traces[:, 3].tolist() and traces[:, 3].min() > 0
    # a candidate taken at a position beyond chunk 31 changed what a later idx1 got: the bit was cleared and the clearing was seen
    assert all(sum(1 for _, p in d["changed"] if p >= 2048) > 0 for d in detail)
    for d, o in zip(detail, want):
        assert (d["before"] >= 0).sum() > o["n_matches"] > 0  # the orientation check removes some


def test_either_side_of_bit_32():
    prob, want = SEARCH["one node, n2 = 2048: 32 chunks"]
    assert _one_node(prob, 200, 2048) == 32
    assert max(p.max() for p in _match_positions(prob, want)) >= 1984  # chunk 31: the last bit of the low word
    prob, want = SEARCH["one node, n2 = 2049: 33 chunks"]
    assert _one_node(prob, 200, 2049) == 33
    assert max(p.max() for p in _match_positions(prob, want)) == 2048  # chunk 32 holds that one position: bit 32, lane 0


@pytest.mark.parametrize("n1,n_kf2", [(1025, 4), (4096, 2)])
def test_key_point_loops_take_a_second_stride(n1, n_kf2):
    prob, want = SEARCH["N1 = %d over 100 nodes" % n1]
    assert len(prob["kf1"]["angle"]) == n1 and len(prob["kf2"]) == n_kf2 and prob["check_orientation"] and 90 <= len(prob["kf1"]["node_id"]) <= 100
    off = BS.restate(dict(prob, check_orientation=False))
    kept = sum(int((o["match12"][1024:] >= 0).sum()) for o in want)
    removed = sum(int(((o["match12"][1024:] < 0) & (f["match12"][1024:] >= 0)).sum()) for o, f in zip(want, off))
    assert kept > 0 and removed > 0, (kept, removed)  # index >= 1024: the -1 fill, the histogram and the removal in their second stride
    _, traces = BS.restate(prob, with_traces=True)
    assert traces[:, 4].sum() == sum(int(((o["match12"] < 0) & (f["match12"] >= 0)).sum()) for o, f in zip(want, off))


def test_the_small_problem_of_the_mixed_call():
    prob, want = SEARCH["one key-point"]
    assert len(prob["kf1"]["angle"]) == 1 and all(len(k["angle"]) == 1 for k in prob["kf2"]) and sum(o["n_matches"] for o in want) > 0
