"""The constants of ORBmatcher::SearchByBoW and of its caller in loop detection (TH_LOW, HISTO_LENGTH, the initial 256s,
matcherBoW(0.9, true), nBoWMatches, the operators of the four comparisons): tests/golden/bow_search_constants.json holds the
reference's values, parsed from the reference itself when it is on the machine, and is compared with what the rule header compiles
in.  Also: the new entry points are exported.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import bow_search_support as BS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "bow_search_constants.json")))


def _body(src, head):
    a = src.index(head)
    return src[a:src.index("\n}\n", a)]


def _squeeze(s):
    return re.sub(r"\s+", " ", s)


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference sources are not on this machine")
def test_fixture_is_the_reference():
    orb = open(os.path.join(REF, "ORBmatcher.cc")).read()
    sbb = _squeeze(_body(orb, "int ORBmatcher::SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2,"))
    loop = _squeeze(_body(open(os.path.join(REF, "LoopClosing.cc")).read(), "bool LoopClosing::DetectCommonRegionsFromBoW("))
    m = re.search(r"ORBmatcher matcherBoW\(([0-9.]+), (true|false)\);", loop)
    got = dict(
        TH_LOW=int(re.search(r"const int ORBmatcher::TH_LOW = (\d+);", orb).group(1)),
        HISTO_LENGTH=int(re.search(r"const int ORBmatcher::HISTO_LENGTH = (\d+);", orb).group(1)),
        initial_distance=int(re.search(r"int bestDist1 = (\d+);", sbb).group(1)),
        loop_nn_ratio=float(m.group(1)), loop_check_orientation=m.group(2) == "true",
        nBoWMatches=int(re.search(r"int nBoWMatches = (\d+);", loop).group(1)))
    assert re.search(r"int bestDist2 = (\d+);", sbb).group(1) == str(got["initial_distance"]) and "int bestIdx2 = -1;" in sbb
    for k in BS.CONSTANTS:
        assert got[k] == GOLDEN[k], k
    c = GOLDEN["comparisons"]
    assert "if (%s) {" % c["best"] in sbb and "} else if (%s) {" % c["second_best"] in sbb
    assert "if (%s) { if (%s) {" % (c["th_low"], c["ratio"]) in sbb
    # what the rule relies on besides: the skips, the order of the walk, and the call site
    assert "if (vbMatched2[idx2] || !pMP2) continue;" in sbb and "if (pMP2->isBad()) continue;" in sbb
    assert "if (!pMP1) continue; if (pMP1->isBad()) continue;" in sbb
    assert "f1it = vFeatVec1.lower_bound(f2it->first);" in sbb and "f2it = vFeatVec2.lower_bound(f1it->first);" in sbb
    assert "matcherBoW.SearchByBoW(mpCurrentKF, vpCovKFi[j], vvpMatchedMPs[j]);" in loop
    assert "// pMostBoWMatchesKF = vpCovKFi[pMostBoWMatchesKF];" in loop  # nIndexMostBoWMatchesKF is computed and never used
    assert "if (numBoWMatches >= nBoWMatches)" in loop


def test_constants_compiled_into_the_rule():
    got = BS.rule_constants()
    for k in BS.CONSTANTS:
        want = float(np.float32(GOLDEN[k])) if k == "loop_nn_ratio" else float(GOLDEN[k])
        assert got[k] == want, (k, got[k], GOLDEN[k])
    rule = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "bow_search_rule.hpp")).read()
    # the operators of the four comparisons, as the reference writes them
    for line in ("if (dist < key_dist(b.key1)) {", "} else if (dist < b.dist2) {", "if (bestDist1 < kThLow) {",
                 "if ((float)bestDist1 < nn_ratio * (float)bestDist2) return true;"):
        assert line in rule, line
    assert '#include "triangulate_rule.hpp"' in rule and "rot_bin(" not in rule.split("namespace gfs_bow {")[0]
    assert "int rot_bin(" not in rule and "void three_maxima(" not in rule  # used, not copied
    hip = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "bow_search.hip")).read()
    for call in ("gfs_bow::best_offer(", "gfs_bow::accept(", "gfs_tri::rot_bin(", "gfs_tri::three_maxima(", "gfs_bow::bin_kept("):
        assert call in hip, call
    mk = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "Makefile")).read()
    assert "bow_search.hip" in mk and "EXACT := -ffp-contract=off" in mk


def test_new_symbols_exported(api):
    L = api.lib()
    for s in ("gfs_sbp_reserve_bow", "gfs_search_by_bow"):
        assert hasattr(L, s), s
        assert s in api.ABI_SYMBOLS, s
    assert hasattr(api.ProjectionMatcher, "search_by_bow") and hasattr(api.ProjectionMatcher, "reserve_bow")
    hdr = open(os.path.join(ROOT, "include", "gfs_abi.h")).read()
    for name in ("gfs_bow_keyframe", "gfs_bow_problem", "gfs_bow_result"):
        assert "} %s;" % name in hdr, name
