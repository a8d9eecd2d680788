"""The constants and comparison operators of ORBmatcher::Fuse's search (TH_LOW, the chi2 gates, the viewing-angle factor, the
distance factors, KeyFrame::IsInImage, the mvuRight test, the level window): tests/golden/fuse_constants.json holds the reference's
values, parsed from the reference itself when it is on the machine, and is compared with what the CPU restatement, the HIP source
(the rule header the kernel is built from) and the adaptor compile in.  Also: the new entry points are exported.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import fuse_support as FS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "fuse_constants.json")))
NAMES = ("th_low", "chi2_stereo", "chi2_mono", "view_cos_half", "min_distance_factor", "max_distance_factor", "depth_test", "is_in_image",
         "u_right_test", "level_window", "best_test", "match_test")


def _body(src, head):
    a = src.index(head)
    return src[a:src.index("\n}\n", a)]


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference sources are not on this machine")
def test_fixture_is_the_reference():
    orb = open(os.path.join(REF, "ORBmatcher.cc")).read()
    fuse = _body(orb, "int ORBmatcher::Fuse(KeyFrame *pKF, const vector<MapPoint *> &vpMapPoints,")
    mp = open(os.path.join(REF, "MapPoint.cc")).read()
    img = _body(open(os.path.join(REF, "KeyFrame.cc")).read(), "bool KeyFrame::IsInImage(")
    m = re.search(r"return \(x (\S+) mnMinX && x (\S+) mnMaxX && y (\S+) mnMinY && y (\S+) mnMaxY\);", img)
    lw = re.search(r"if \(kpLevel < nPredictedLevel( - \d+)? \|\| kpLevel > nPredictedLevel( [-+] \d+)?\) continue;", fuse)
    off = lambda g: int(g.replace(" ", "")) if g else 0
    got = dict(
        th_low=int(re.search(r"const int ORBmatcher::TH_LOW = (\d+);", orb).group(1)),
        chi2_stereo=float(re.search(r"er \* er;\s+if \(e2 \* pKF->mvInvLevelSigma2\[kpLevel\] > ([0-9.]+)\) continue;", fuse).group(1)),
        chi2_mono=float(re.search(r"ey \* ey;\s+if \(e2 \* pKF->mvInvLevelSigma2\[kpLevel\] > ([0-9.]+)\) continue;", fuse).group(1)),
        view_cos_half=float(re.search(r"if \(PO\.dot\(Pn\) < ([0-9.]+) \* dist3D\)", fuse).group(1)),
        min_distance_factor=float(re.search(r"return ([0-9.]+)f \* mfMinDistance;", mp).group(1)),
        max_distance_factor=float(re.search(r"return ([0-9.]+)f \* mfMaxDistance;", mp).group(1)),
        depth_test=re.search(r"if \(p3Dc\(2\) (\S+) 0\.0f\)", fuse).group(1),
        is_in_image=list(m.groups()),
        u_right_test=re.search(r"if \(pKF->mvuRight\[idx\] (\S+) 0\)", fuse).group(1),
        level_window=[off(lw.group(1)), off(lw.group(2))],
        best_test=re.search(r"if \(dist (\S+) bestDist\)", fuse).group(1),
        match_test=re.search(r"if \(bestDist (\S+) TH_LOW\)", fuse).group(1))
    for k in NAMES:
        assert got[k] == GOLDEN[k], k


def _check_source(text, names):
    """a statement of the rule in C++: `names` gives its spelling of the variables"""
    g = GOLDEN
    n = names
    assert re.search(r"if \(%s (\S+) 0\.0f\) return" % re.escape(n["z"]), text).group(1) == g["depth_test"]
    m = re.search(r"if \(!\(u (\S+) \S*min_x && u (\S+) \S*max_x && v (\S+) \S*min_y && v (\S+) \S*max_y\)\) return", text)
    assert list(m.groups()) == g["is_in_image"]
    assert re.search(r"if \(%s (\S+) 0\) \{" % n["ur"], text).group(1) == g["u_right_test"]
    lw = re.search(r"if \(%s < %s( - \d+)? \|\| %s > %s( [-+] \d+)?\) (continue|return false);" % (n["oct"], n["lv"], n["oct"], n["lv"]), text)
    off = lambda s: int(s.replace(" ", "")) if s else 0
    assert [off(lw.group(1)), off(lw.group(2))] == g["level_window"]
    assert re.search(r"if \(%s (\S+) %s\) \{" % (n["d"], n["best"]), text).group(1) == g["best_test"]


def test_constants_in_restatement_rule_and_adaptor():
    g = GOLDEN
    f = np.float32
    out = np.zeros(3, np.float32)
    FS.restatement().fr_constants(out.ctypes.data)
    assert out[0] == g["th_low"] and out[1] == f(g["min_distance_factor"]) and out[2] == f(g["max_distance_factor"])
    rst = open(os.path.join(ROOT, "tests", "host", "fuse_restatement.cpp")).read()
    _check_source(rst, dict(z=r"p3Dc[2]", ur=r"k\.u_right\[idx\]", oct="kpLevel", lv="nPredictedLevel", d="dist", best="bestDist"))
    assert float(re.search(r"er \* er;\s+st\.stereo\+\+;\s+if \(e2 \* k\.inv_level_sigma2\[kpLevel\] > ([0-9.]+)\)", rst).group(1)) == g["chi2_stereo"]
    assert float(re.search(r"ey \* ey;\s+st\.mono\+\+;\s+if \(e2 \* k\.inv_level_sigma2\[kpLevel\] > ([0-9.]+)\)", rst).group(1)) == g["chi2_mono"]
    assert float(re.search(r"if \(dot < ([0-9.]+) \* dist3D\)", rst).group(1)) == g["view_cos_half"]
    assert re.search(r"o\.exit = bestDist (\S+) TH_LOW \? GFS_FUSE_MATCHED", rst).group(1) == g["match_test"]
    # the HIP source: the kernel is built from the rule header, and keeps the best under the same operator
    rule = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "fuse_rule.hpp")).read()
    _check_source(rule, dict(z=r"Pc[2]", ur="kur", oct="oct", lv=r"R\.level", d="d", best=r"o\.best_dist \|\| \(d == o\.best_dist && o\.best_idx >= 0 && earlier\)"))
    assert int(re.search(r"kThLow = (\d+);", rule).group(1)) == g["th_low"]
    assert float(re.search(r"kMinDistFactor = ([0-9.]+)f;", rule).group(1)) == g["min_distance_factor"]
    assert float(re.search(r"kMaxDistFactor = ([0-9.]+)f;", rule).group(1)) == g["max_distance_factor"]
    assert float(re.search(r"kViewCosHalf = ([0-9.]+);", rule).group(1)) == g["view_cos_half"]
    assert float(re.search(r"kChi2Stereo = ([0-9.]+);", rule).group(1)) == g["chi2_stereo"]
    assert float(re.search(r"kChi2Mono = ([0-9.]+);", rule).group(1)) == g["chi2_mono"]
    assert "if (dist < kMinDistFactor * min_dist) return" in rule and "if (dist > kMaxDistFactor * max_dist) return" in rule
    assert "if ((double)dot < kViewCosHalf * (double)dist) return" in rule
    assert "if ((double)(e2 * K.inv_sigma2[oct]) > kChi2Stereo) return false;" in rule
    assert "if ((double)(e2 * K.inv_sigma2[oct]) > kChi2Mono) return false;" in rule
    assert re.search(r"best_dist (\S+) kThLow \? kMatched : kNoCandidate", rule).group(1) == g["match_test"]
    hip = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "fuse.hip")).read()
    k = hip[hip.index("void k_fuse("):hip.index("}  // namespace")]
    assert "gfs_fuse::project(K, P, Pn, mp_min[at], mp_max[at])" in k and "gfs_fuse::candidate_ok(K, R, kx, ky, s_ur[j], (int)s_oct[j])" in k
    assert re.search(r"if \(d (\S+) best_dist\) \{", k).group(1) == g["best_test"] and "gfs_fuse::search_exit(any, best_dist)" in k
    # the adaptor acts on the device's verdict and on nothing else
    ada = open(os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp")).read()
    assert "if (exit != GFS_FUSE_MATCHED) continue;" in ada and "if (pMPinKF->Observations() > pMP->Observations())" in ada


def test_gates_behave_as_written():
    """The operators above, observed on the constructed points: on a bound or a gate one way, its neighbour the other."""
    prob, labels = FS.constructed()
    out = FS.restate(prob)
    ex = lambda label: int(out[labels[label][0]]["exit"][labels[label][1]])
    for inside, outside in (("u==min", "u<min"), ("u<max", "u==max"), ("v==min", "v<min"), ("v<max", "v==max")):
        assert ex(inside) >= FS.EMPTY_WINDOW and ex(outside) == FS.NOT_IN_IMAGE, inside
    assert ex("dist==0.8min") >= FS.EMPTY_WINDOW and ex("dist<0.8min") == FS.TOO_NEAR
    assert ex("dist==1.2max") >= FS.EMPTY_WINDOW and ex("dist>1.2max") == FS.TOO_FAR
    assert ex("dot==half") >= FS.EMPTY_WINDOW and ex("dot<half") == FS.VIEW_ANGLE
    assert ex("ur=-1") == FS.MATCHED and ex("ur=-0") == FS.NO_CANDIDATE and ex("ur=0") == FS.NO_CANDIDATE
    assert ex("dist=50") == FS.MATCHED and ex("dist=51") == FS.NO_CANDIDATE


def test_new_symbols_exported(api):
    L = api.lib()
    for s in ("gfs_sbp_reserve_fuse", "gfs_fuse_search"):
        assert hasattr(L, s), s
        assert s in api.ABI_SYMBOLS, s
    assert L.gfs_abi_version() == 1
    assert hasattr(api.ProjectionMatcher, "fuse_search") and hasattr(api.ProjectionMatcher, "reserve_fuse")
    hdr = open(os.path.join(ROOT, "include", "gfs_abi.h")).read()
    for i, name in enumerate(api.FUSE_EXITS):
        assert re.search(r"#define GFS_FUSE_%s %d\b" % (name.upper(), i), hdr), name
