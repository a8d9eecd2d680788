"""The sequential restatement of the vocabulary transform and of the database query (tests/host/bow_vocab_restatement.cpp) against an
independent statement in plain Python and against the rule header's host build (geoflowslam_amd/csrc/bow_vocab_rule.hpp); the
hand-built cases whose outputs their labels promise; the tree validator; gfs_host::LoadVocabularyText on files the test writes.  No
GPU."""
import numpy as np
import pytest

import bow_vocab_support as BV
from geoflowslam_amd import synth

TREES = [dict(k=10, L=3, stop_frac=0.1), dict(k=3, L=4, stop_frac=0.2, prune_frac=0.3, shuffle_children=True), dict(k=17, L=2),
         dict(k=1, L=3), dict(k=4, L=5, prune_frac=0.2, shuffle_children=True)]


@pytest.mark.parametrize("t", range(len(TREES)))
def test_restatement_against_python_and_rule(t):
    v = BV.vocabulary(11 + t, **TREES[t])
    n_words, min_leaf = BV.rule_validate(v)
    assert n_words == int((v["word_id"] >= 0).sum())
    for levelsup in sorted({0, 1, v["L"] - min_leaf, v["L"], v["L"] + 2}):
        descs = [synth.bow_features(50 * t + j, v, n, 10, 0.3) for j, n in enumerate((0, 1, 37))]
        rc, want = BV.restate(v, descs, levelsup)
        rrc, rule, why = BV.rule_host(v, descs, levelsup)
        defined = v["L"] - levelsup <= 0 or min_leaf >= v["L"] - levelsup
        assert (rrc == 0) == defined, (levelsup, rrc, why)
        if not defined:
            # the restatement notices the unassigned node unless no feature happens to reach a shallow leaf
            assert rc in (0, -2)
            continue
        assert rc == 0
        for j, d in enumerate(descs):
            BV.assert_vectors_equal(want[j], rule[j], ("rule", t, levelsup, j))
            BV.assert_vectors_equal(want[j], BV.python_transform(v, d, levelsup), ("python", t, levelsup, j))
        w = want[2]
        assert len(w["word_id"]) > 0 and (np.diff(w["word_id"]) > 0).all() and (np.diff(w["node_id"]) > 0).all()
        assert all((np.diff(w["feat_idx"][a:b]) > 0).all() for a, b in zip(w["node_start"][:-1], w["node_start"][1:]))
        assert len(w["feat_idx"]) == int((w["word_of_feature"] >= 0).sum())


def test_duplicates_and_stopped_words_occur():
    v, descs, levelsup, want = BV.problem(3, 10, 3, (300,))
    w = want[0]
    assert (w["word_of_feature"] < 0).any() and len(w["word_id"]) < int((w["word_of_feature"] >= 0).sum())  # stopped, and shared words
    assert abs(w["word_value"].sum() - 1.0) < 1e-12


@pytest.mark.parametrize("label", list(BV.constructed()))
def test_constructed_cases(label):
    v, desc, levelsup, want = BV.constructed()[label]
    rc, got = BV.restate(v, desc, levelsup)
    rrc, rule, why = BV.rule_host(v, desc, levelsup)
    if want is None:
        assert rc == -2 and rrc == -2 and BV.python_transform(v, desc, levelsup) is None
        return
    assert rc == 0 and rrc == 0, why
    BV.assert_vectors_equal(got, want, label)
    BV.assert_vectors_equal(rule, want, label)
    BV.assert_vectors_equal(BV.python_transform(v, desc, levelsup), want, label)


def test_validator():
    ok, bad = BV.malformed()
    assert BV.rule_validate(ok) == (4, 2)
    for label, v in bad.items():
        assert isinstance(BV.rule_validate(v), str), label
    assert "cycle" in BV.rule_validate(bad["a cycle"]) and "twice" in BV.rule_validate(bad["a child listed under two parents"])
    assert "out of range" in BV.rule_validate(bad["an index out of range"]) and "leaf has children" in BV.rule_validate(bad["a leaf with children"])


def _database(seed, n_entries, id_range=400):
    rng = np.random.default_rng(seed)
    entries, order = {}, []
    for s in rng.permutation(n_entries + 3)[:n_entries]:
        entries[int(s)] = BV.bow_vector(seed * 1000 + int(s), int(rng.integers(1, 120)), id_range)
        order.append(int(s))
    return entries, order


@pytest.mark.parametrize("seed", range(4))
def test_query_restatement_against_python_and_rule(seed):
    E = 40
    entries, order = _database(seed, 30)
    db = BV.RestatedDatabase(E)
    for s in order:
        db.add(s, *entries[s])
    gone = order[3]
    db.erase(gone)
    db.erase(gone)  # an empty slot: nothing happens
    back = order[7]
    db.add(back, *entries[back])  # re-added: now the last of every list it is in
    live = {s: e for s, e in entries.items() if s != gone}
    order2 = [s for s in order if s not in (gone, back)] + [back]
    q = BV.bow_vector(900 + seed, 90, 400)
    got = db.query(*q)
    want = BV.python_query(live, order2, E, *q)
    BV.assert_query_equal(got, want, seed)
    assert got["list"].tolist() == want["list"].tolist()
    BV.assert_query_equal(BV.rule_query(live, E, *q), got, ("rule", seed))
    # the order of the sharing list IS (lowest common word, add sequence)
    seq = {s: i for i, s in enumerate(order2)}
    sharing = [s for s in live if got["n_common"][s] > 0]
    assert sorted(sharing, key=lambda s: (got["first_word"][s], seq[s])) == got["list"].tolist()
    assert sorted(sharing) != got["list"].tolist()  # ... and not slot order
    assert got["n_common"][gone] == 0 and got["first_word"][gone] == -1 and got["score"][gone] == 0


def test_query_edges():
    E = 6
    db = BV.RestatedDatabase(E)
    q = BV.bow_vector(1, 50, 100)
    empty = db.query(*q)
    assert (empty["n_common"] == 0).all() and (empty["first_word"] == -1).all() and (empty["score"] == 0).all() and len(empty["list"]) == 0
    db.add(2, *q)
    db.add(4, np.array([q[0][-1]], np.int32), np.array([1.0]))
    got = db.query(*q)
    assert got["n_common"].tolist() == [0, 0, 50, 0, 1, 0] and got["score"][2] == np.float32(1.0)  # an entry identical to the query
    assert got["first_word"][4] == q[0][-1]
    BV.assert_query_equal(BV.rule_query({2: q, 4: (np.array([q[0][-1]], np.int32), np.array([1.0]))}, E, *q), got)
    none = db.query(np.zeros(0, np.int32), np.zeros(0))
    assert (none["n_common"] == 0).all() and len(none["list"]) == 0
    L = BV.restatement()
    ids, bad_ids, neg = np.array([1, 5, 9], np.int32), np.array([1, 5, 5], np.int32), np.array([-1, 5, 9], np.int32)
    vals, nan = np.array([0.2, 0.3, 0.5]), np.array([0.2, np.nan, 0.5])
    assert L.bv_rule_valid_vector(3, ids.ctypes.data, vals.ctypes.data) == 1
    for i, v in ((bad_ids, vals), (neg, vals), (ids, nan)):
        assert L.bv_rule_valid_vector(3, i.ctypes.data, v.ctypes.data) == 0


@pytest.mark.parametrize("trailing_newline", (True, False))
def test_load_vocabulary_text(api, tmp_path, trailing_newline):
    """gfs_host::LoadVocabularyText on a file the test writes: node id = line order, children in line order, word ids in leaf line
    order; the empty line behind a trailing newline builds no node; the loaded tree transforms like the one that was written."""
    v = BV.vocabulary(21, 3, 3, 0.1, 0.3)  # ids in line order: what a file can hold
    path = str(tmp_path / "voc.txt")
    BV.write_vocabulary_text(v, path, trailing_newline)
    got = BV.load_vocabulary_text(path)
    assert got is not None and got["n_nodes"] == v["n_nodes"] and (got["k"], got["L"], got["scoring"], got["weighting"]) == (3, 3, 0, 0)
    for k in ("parent", "child_start", "children", "desc", "weight", "word_id"):
        a, b = np.asarray(got[k]), np.asarray(v[k])
        if k in ("parent", "desc"):  # the root has no line
            a, b = a[1:], b[1:]
        assert a.tobytes() == b.astype(a.dtype).tobytes(), k
    assert isinstance(BV.rule_validate(got), tuple)
    d = synth.bow_features(5, v, 40, 8, 0.2)
    BV.assert_vectors_equal(BV.restate(got, d, 2)[1], BV.restate(v, d, 2)[1])


def test_load_vocabulary_text_shuffled_children_and_refusals(api, tmp_path):
    """A tree whose ids are shuffled cannot be written as it is (a line's parent must precede it): written in breadth-first order, the
    loaded tree is the same tree under new ids, and words keep their descriptors and weights.  Files the loader refuses."""
    v = BV.vocabulary(22, 3, 3, 0.1, 0.2, True)
    order, at = [0], 0
    while at < len(order):
        n = order[at]
        order += v["children"][v["child_start"][n]:v["child_start"][n + 1]].tolist()
        at += 1
    new = np.zeros(v["n_nodes"], np.int64)
    new[order] = np.arange(len(order))
    w = dict(v, parent=new[v["parent"][order]], desc=v["desc"][order], weight=v["weight"][order], word_id=v["word_id"][order])
    path = str(tmp_path / "voc.txt")
    BV.write_vocabulary_text(w, path)
    got = BV.load_vocabulary_text(path)
    assert got is not None and isinstance(BV.rule_validate(got), tuple)
    d = synth.bow_features(6, v, 60, 8, 0.2)
    a, b = BV.restate(got, d, 3)[1], BV.restate(v, d, 3)[1]
    # the same leaves are reached: per feature the same weight; word ids are renumbered in leaf line order
    wa = np.where(a["word_of_feature"] >= 0, got["weight"][np.nonzero(got["word_id"] >= 0)[0][np.argsort(got["word_id"][got["word_id"] >= 0])]][a["word_of_feature"]], 0)
    wb = np.where(b["word_of_feature"] >= 0, v["weight"][np.nonzero(v["word_id"] >= 0)[0][np.argsort(v["word_id"][v["word_id"] >= 0])]][b["word_of_feature"]], 0)
    assert wa.tobytes() == wb.tobytes() and np.sort(a["word_value"]).tobytes() == np.sort(b["word_value"]).tobytes()
    for header in ("21 3 0 0", "3 0 0 0", "3 11 0 0", "3 3 6 0", "3 3 0 4", "-1 3 0 0"):
        open(path, "w").write(header + "\n0 1 " + " ".join(["0"] * 32) + " 1.0\n")
        assert BV.load_vocabulary_text(path) is None, header
    open(path, "w").write("3 3 0 0\n5 1 " + " ".join(["0"] * 32) + " 1.0\n")  # a parent that no line has defined yet
    assert BV.load_vocabulary_text(path) is None
    assert BV.load_vocabulary_text(str(tmp_path / "missing.txt")) is None
