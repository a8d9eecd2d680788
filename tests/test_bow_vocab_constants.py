"""The constants of the vocabulary transform, of the loader and of KeyFrameDatabase::DetectNBestCandidates (levelsup 4 at both
ComputeBoW sites, 0.8f, GetBestCovisibilityKeyFrames(10), nNumCandidates 3, `w > 0`, `d < best_d`, the loader's bounds):
tests/golden/bow_vocab_constants.json holds the reference's values, parsed from the reference itself when it is on the machine, and is
compared with what the rule header and the adaptors compile in.  Also: the new entry points are exported, and the rule header's host
build under the sanitizers as a program of its own.  No GPU."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import bow_vocab_support as BV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "bow_vocab_constants.json")))


def _squeeze(s):
    return re.sub(r"\s+", " ", s)


def _body(src, head):
    a = src.index(head)
    return src[a:src.index("\n}\n", a)]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="the reference sources are not on this machine")
def test_fixture_is_the_reference():
    src = lambda *p: open(os.path.join(REF, *p)).read()
    kf = _squeeze(_body(src("src", "KeyFrame.cc"), "void KeyFrame::ComputeBoW() {"))
    fr = _squeeze(_body(src("src", "Frame.cc"), "void Frame::ComputeBoW() {"))
    sites = [re.search(r"mpORBvocabulary->transform\(vCurrentDesc, mBowVec, mFeatVec, (\d+)\);", b).group(1) for b in (kf, fr)]
    assert sites == [str(GOLDEN["levelsup"])] * 2
    assert "if (mBowVec.empty() || mFeatVec.empty()) {" in kf and "if (mBowVec.empty()) {" in fr  # the guards the adaptor restates
    db = _squeeze(_body(src("src", "KeyFrameDatabase.cc"), "void KeyFrameDatabase::DetectNBestCandidates("))
    assert float(re.search(r"int minCommonWords = maxCommonWords \* ([0-9.]+)f;", db).group(1)) == GOLDEN["min_common_share"]
    assert int(re.search(r"GetBestCovisibilityKeyFrames\((\d+)\);", db).group(1)) == GOLDEN["covisibles"]
    assert "lAccScoreAndMatch.sort(compFirst);" in db and "if (pKFi->mnPlaceRecognitionWords > minCommonWords) {" in db
    loop = _squeeze(src("src", "LoopClosing.cc"))
    assert int(re.search(r"DetectNBestCandidates\(mpCurrentKF, vpLoopBowCand, vpMergeBowCand, (\d+)\);", loop).group(1)) == GOLDEN["nNumCandidates"]
    voc = src("Thirdparty", "DBoW2", "DBoW2", "TemplatedVocabulary.h")
    c = GOLDEN["comparisons"]
    assert voc.count("if(%s) // not stopped" % c["not_stopped"]) == 2 and "if(%s)" % c["closer_child"] in voc
    assert "if(%s)" % c["loader_bounds"] in voc
    m = re.search(r"m_k<0 \|\| m_k>(\d+) \|\| m_L<1 \|\| m_L>(\d+)", voc)
    assert (int(m.group(1)), int(m.group(2))) == (GOLDEN["max_k"], GOLDEN["max_L"])
    bow = _squeeze(src("Thirdparty", "DBoW2", "DBoW2", "BowVector.h"))
    assert re.search(r"enum WeightingType \{ TF_IDF,", bow) and re.search(r"enum ScoringType \{ L1_NORM,", bow)  # both are 0
    sc = src("Thirdparty", "DBoW2", "DBoW2", "ScoringObject.cpp")
    assert "score += fabs(vi - wi) - fabs(vi) - fabs(wi);" in sc and "score = -score/2.0;" in sc


def test_constants_compiled_into_the_rule_and_the_adaptors():
    got = BV.rule_constants()
    for k in ("levelsup", "covisibles", "nNumCandidates", "max_k", "max_L", "scoring", "weighting"):
        assert got[k] == float(GOLDEN[k]), (k, got[k])
    assert got["min_common_share"] == float(np.float32(GOLDEN["min_common_share"]))
    assert got["w_gt_0"] == 1 and got["d_lt_best_d"] == 1
    rule = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "bow_vocab_rule.hpp")).read()
    for line in ("return !(weight > 0);", "return fabs(vi - wi) - fabs(vi) - fabs(wi);", "return (float)(-score / 2.0);", "if (norm > 0.0)"):
        assert line in rule, line
    ad = open(os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp")).read()
    for line in ("int minCommonWords = maxCommonWords * gfs_bowv::kMinCommonShare;", "GetBestCovisibilityKeyFrames(gfs_bowv::kCovisibles);",
                 "int nNumCandidates = gfs_bowv::kLoopNumCandidates)", "gfs_bowv::kLevelsUp, &o)", "k > gfs_bowv::kMaxK || L < 1 || L > gfs_bowv::kMaxL",
                 "if (pKFi->mnPlaceRecognitionWords > minCommonWords) {", "std::stable_sort(lAccScoreAndMatch.begin()"):
        assert line in ad, line
    hip = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "bow_vocab.hip")).read()
    for call in ("child_key(", "key_position(", "stopped(", "l1_term(", "l1_finish(", "sort_key(", "nid_defined(", "pack_tree(", "valid_bow_vector("):
        assert call in hip, call
    mk = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "Makefile")).read()
    assert "bow_vocab.hip" in mk and "EXACT := -ffp-contract=off" in mk


def test_new_symbols_exported(api):
    L = api.lib()
    for s in ("gfs_bow_create", "gfs_bow_destroy", "gfs_bow_transform", "gfs_bow_transform_device", "gfs_bow_db_create", "gfs_bow_db_destroy",
              "gfs_bow_db_add", "gfs_bow_db_erase", "gfs_bow_db_query"):
        assert hasattr(L, s), s
        assert s in api.ABI_SYMBOLS, s
    for m in ("transform", "transform_device"):
        assert hasattr(api.BowVocabulary, m)
    for m in ("add", "erase", "query"):
        assert hasattr(api.BowDatabase, m)
    hdr = open(os.path.join(ROOT, "include", "gfs_abi.h")).read()
    for name in ("gfs_bow_vocabulary", "gfs_bow_vectors"):
        assert "} %s;" % name in hdr, name


def test_rule_check_under_the_sanitizers():
    """tests/host/bow_vocab_rule_check.cpp: the tree validator and the rule's host build on malformed and well-formed trees whose
    arrays are sized exactly, as a program of its own under -fsanitize=address,undefined (plain g++, CPU only, never loaded into
    python): no report, every case as its label says."""
    src = os.path.join(ROOT, "tests", "host", "bow_vocab_rule_check.cpp")
    exe = os.path.join(ROOT, "tests", "host", "_bow_vocab_rule_check_asan")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g",
                    "-I" + os.path.join(ROOT, "include"), "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and r.stdout.endswith("bow_vocab_rule_check: ok\n"), (r.stdout[-1500:], r.stderr[-2000:])
    for label in ("a cycle", "a child listed under two parents", "an index out of range", "a leaf with children"):
        assert re.search(r"^%s +refused: " % re.escape(label), r.stdout, re.M), label
    assert r.stdout.count("accepted") == 5
