"""The constants and comparison operators of the three Sim3 searches of loop closing (TH_LOW, the viewing-angle factor, the level
window, `<` and `<=`, what bestDist starts at, the acceptance tests, the two projection forms, where the taken test stands):
tests/golden/sim3_search_constants.json holds the reference's values, parsed from the reference itself when it is on the machine,
and is compared with what the rule header, the CPU restatement and the kernel source state.  Also: the new entry points are
exported.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import sim3_search_support as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "sim3_search_constants.json")))
HEADS = dict(fuse="int ORBmatcher::Fuse(KeyFrame *pKF, Sophus::Sim3f &Scw,",
             sbp="int ORBmatcher::SearchByProjection(KeyFrame *pKF, Sophus::Sim3f &Scw,",
             sbp_kfs="int ORBmatcher::SearchByProjection(KeyFrame *pKF, Sophus::Sim3<float> &Scw,")


def _body(src, head):
    a = src.index(head)
    return src[a:src.index("\n}\n", a)]


def _parse(fn):
    """what one of the reference's three functions states"""
    lw = re.search(r"if \(kpLevel < nPredictedLevel( - \d+)? \|\| kpLevel > nPredictedLevel( [-+] \d+)?\) continue;", fn)
    off = lambda g: int(g.replace(" ", "")) if g else 0
    dist = re.search(r"if \((dist\w*) < minDistance \|\| (dist\w*) > maxDistance\) continue;", fn)
    invz = re.search(r"const float invz = 1 / p3Dc\(2\);\s+const float x = p3Dc\(0\) \* invz;\s+const float y = p3Dc\(1\) \* invz;\s+"
                     r"const float u = fx \* x \+ cx;\s+const float v = fy \* y \+ cy;", fn)
    taken, level = fn.find("if (vpMatched[idx]) continue;"), fn.find("if (kpLevel < nPredictedLevel")
    m = re.search(r"if \(bestDist (\S+) TH_LOW( \* ratioHamming)?\) \{", fn)
    return dict(
        th_type=re.search(r"(int|float) th,", fn).group(1),
        depth_test=re.search(r"if \(p3Dc\(2\) (\S+) 0\.0f?\) continue;", fn).group(1),
        projection="invz" if invz else ("pinhole" if "pKF->mpCamera->project(p3Dc)" in fn else "?"),
        distance_gate=[dist.group(1) == dist.group(2), "<", ">"],
        view_cos_half=float(re.search(r"if \(PO\.dot\(Pn\) < ([0-9.]+) \* dist\w*\) continue;", fn).group(1)),
        radius="th * pKF->mvScaleFactors[nPredictedLevel]" in fn,
        empty_window="if (vIndices.empty()) continue;" in fn,
        first_best_dist=re.search(r"int bestDist = (\w+);", fn).group(1),
        taken_test="before the level window" if 0 <= taken < level else ("none" if taken < 0 else "after the level window"),
        level_window=[off(lw.group(1)), off(lw.group(2))],
        best_test=re.search(r"if \(dist (\S+) bestDist\) \{", fn).group(1),
        match_test=m.group(1), match_ratio=bool(m.group(2)),
        no_chi2="mvInvLevelSigma2" not in fn and "mvuRight" not in fn and "mbf" not in fn)


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference sources are not on this machine")
def test_fixture_is_the_reference():
    orb = open(os.path.join(REF, "ORBmatcher.cc")).read()
    assert int(re.search(r"const int ORBmatcher::TH_LOW = (\d+);", orb).group(1)) == GOLDEN["th_low"]
    for name, head in HEADS.items():
        assert _parse(_body(orb, head)) == GOLDEN[name], name
    loop = open(os.path.join(REF, "LoopClosing.cc")).read()
    calls = re.findall(r"matcher\w*\.Fuse\(\w+, Scw, vpMapPoints, (\d+), vpReplacePoints\);", loop)
    assert calls and {int(c) for c in calls} == {GOLDEN["fuse_th_at_call_sites"]}


def test_the_three_functions_differ_only_where_the_rule_says():
    f, s, k = GOLDEN["fuse"], GOLDEN["sbp"], GOLDEN["sbp_kfs"]
    differ = lambda a, b: sorted(n for n in a if a[n] != b[n])
    assert differ(f, s) == ["first_best_dist", "match_ratio", "taken_test", "th_type"]
    assert differ(s, k) == ["projection"]
    assert all(g["no_chi2"] and g["radius"] and g["empty_window"] and g["depth_test"] == "<" for g in (f, s, k))


def test_constants_in_rule_restatement_and_kernel():
    g = GOLDEN
    f32 = np.float32
    out = np.zeros(4, np.float32)
    SS.restatement().sr_constants(out.ctypes.data)
    assert out[0] == g["th_low"] and out[1] == f32(0.8) and out[2] == f32(1.2) and out[3] == SS.LISTED
    csrc = os.path.join(ROOT, "geoflowslam_amd", "csrc")
    rule, base = open(os.path.join(csrc, "sim3_search_rule.hpp")).read(), open(os.path.join(csrc, "fuse_rule.hpp")).read()
    # ---- the rule header (the kernel and the host replays are built from it)
    assert int(re.search(r"kThLow = (\d+);", base).group(1)) == g["th_low"]
    assert float(re.search(r"kViewCosHalf = ([0-9.]+);", base).group(1)) == g["fuse"]["view_cos_half"] == g["sbp"]["view_cos_half"]
    assert "if ((double)dot < kViewCosHalf * (double)dist) return" in base
    assert "if (dist < kMinDistFactor * min_dist) return" in base and "if (dist > kMaxDistFactor * max_dist) return" in base
    assert "R.radius = K.th * K.scale[R.level];" in base
    assert re.search(r"if \(Pc\[2\] (\S+) 0\.0f\) return", rule).group(1) == g["fuse"]["depth_test"] == g["sbp_kfs"]["depth_test"]
    assert "return mode == kFuse ? kIntMax : 256;" in rule and "kIntMax = 2147483647;" in rule
    assert g["fuse"]["first_best_dist"] == "INT_MAX" and g["sbp"]["first_best_dist"] == g["sbp_kfs"]["first_best_dist"] == "256"
    m = re.search(r"return mode == kFuse \? best_dist (\S+) gfs_fuse::kThLow : \(float\)best_dist (\S+) \(float\)gfs_fuse::kThLow \* ratio_hamming;", rule)
    assert m.group(1) == g["fuse"]["match_test"] and m.group(2) == g["sbp"]["match_test"] == g["sbp_kfs"]["match_test"]
    assert not g["fuse"]["match_ratio"] and g["sbp"]["match_ratio"] and g["sbp_kfs"]["match_ratio"]
    proj = rule[rule.index("GFS_HD Proj project("):rule.index("// the level filter")]
    kfs_form, pinhole_form = proj[proj.index("if (mode == kSbpKfs) {"):proj.index("} else {")], proj[proj.index("} else {"):]
    assert "const float invz = 1.0f / Pc[2];" in kfs_form and "x = Pc[0] * invz, y = Pc[1] * invz;" in kfs_form
    assert "u = K.fx * x + K.cx;" in kfs_form and "v = K.fy * y + K.cy;" in kfs_form
    assert "u = K.fx * Pc[0] / Pc[2] + K.cx;" in pinhole_form and "v = K.fy * Pc[1] / Pc[2] + K.cy;" in pinhole_form
    assert g["sbp_kfs"]["projection"] == "invz" and g["fuse"]["projection"] == g["sbp"]["projection"] == "pinhole"
    lw = re.search(r"return !\(oct < R\.level( - \d+)? \|\| oct > R\.level( [-+] \d+)?\);", rule)
    off = lambda s: int(s.replace(" ", "")) if s else 0
    assert [off(lw.group(1)), off(lw.group(2))] == g["fuse"]["level_window"] == g["sbp"]["level_window"] == g["sbp_kfs"]["level_window"]
    host = rule[rule.index("inline PointResult search_point("):]
    assert 0 < host.index("if (mode != kFuse && taken && taken[j]) continue;") < host.index("if (!level_ok(R, oct)) continue;")
    assert g["sbp"]["taken_test"] == g["sbp_kfs"]["taken_test"] == "before the level window" and g["fuse"]["taken_test"] == "none"
    assert re.search(r"if \(d (\S+) o\.best_dist \|\|", host).group(1) == g["fuse"]["best_test"]
    # ---- the kernel and the entry's replay
    hip = open(os.path.join(csrc, "sim3_search.hip")).read()
    k = hip[hip.index("void k_sim3_search("):hip.index("using Layout")]
    assert "gfs_sim3::project(K, mode, P, Pn, mp_min[at], mp_max[at])" in k and "gfs_fuse::in_window(R, s_kx[j], s_ky[j])" in k
    assert 0 < k.index("if (o & kTakenBit) return false;") < k.index("return gfs_sim3::level_ok(R, o);")  # (the walk's gate)
    assert "const int first = gfs_sim3::first_best_dist(mode)" in k and "if (d >= first) return;" in k
    assert re.search(r"if \(d (\S+) c_dist\[kListed - 1\]\) \{", k).group(1) == g["sbp"]["best_test"]
    assert re.search(r"if \(c_dist\[s\] (\S+) c_dist\[s - 1\]\) \{", k).group(1) == g["sbp"]["best_test"]
    entry = hip[hip.index("int gfs_sim3_search("):]
    assert "if (gfs_sim3::accepted(k.mode, dist, k.ratio_hamming)) {" in entry and "gfs_sim3::ratio_ok(k.ratio_hamming)" in entry
    assert "(float)gfs_fuse::kThLow * ratio_hamming < 256.0f" in rule
    # ---- the restatement
    rst = open(os.path.join(ROOT, "tests", "host", "sim3_search_restatement.cpp")).read()
    fuse, sbp = rst[rst.index("Out fuse_point("):rst.index("// :453-526")], rst[rst.index("Out sbp_point("):rst.index("}  // namespace")]
    assert re.search(r"if \(p3Dc\[2\] (\S+) 0\.0f\) return o;", fuse).group(1) == g["fuse"]["depth_test"]
    assert re.search(r"if \(p3Dc\[2\] (\S+) 0\.0\) return o;", sbp).group(1) == g["sbp"]["depth_test"]
    assert "int bestDist = INT_MAX, bestIdx = -1;" in fuse and "int bestDist = 256, bestIdx = -1;" in sbp
    assert re.search(r"o\.exit = bestDist (\S+) TH_LOW \? GFS_FUSE_MATCHED", fuse).group(1) == g["fuse"]["match_test"]
    assert re.search(r"if \(bestDist (\S+) TH_LOW \* k\.ratio_hamming\) \{", sbp).group(1) == g["sbp"]["match_test"]
    assert "const float invz = 1 / p3Dc[2];" in sbp and "u = k.fx * x + k.cx;" in sbp and "u = k.fx * p3Dc[0] / p3Dc[2] + k.cx;" in sbp
    assert "u = k.fx * p3Dc[0] / p3Dc[2] + k.cx;" in fuse and "invz" not in fuse
    loop = rst[rst.index("void best_candidate("):rst.index("// :1572-1650")]
    assert 0 < loop.index("if (taken && taken[idx]) {") < loop.index("if (kpLevel < nPredictedLevel - 1 || kpLevel > nPredictedLevel) continue;")
    assert re.search(r"if \(dist (\S+) \*bestDist\) \{", loop).group(1) == g["sbp"]["best_test"]
    assert float(re.search(r"if \(dot < ([0-9.]+) \* dist\) return GFS_FUSE_VIEW_ANGLE;", rst).group(1)) == g["sbp"]["view_cos_half"]
    assert "constexpr int TH_LOW = %d;" % g["th_low"] in rst
    # ---- the adaptors act on the entry's verdict; SearchAndFuse passes the call sites' th
    ada = open(os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp")).read()
    assert "if (exit != GFS_FUSE_MATCHED) continue;" in ada and "if (!pMPinKF->isBad()) vpReplacePoint[iMP] = pMPinKF;" in ada
    assert ada.count("std::vector<MapPoint*>& vpMapPoints, float th = %.1ff)" % g["fuse_th_at_call_sites"]) == 2


def test_gates_behave_as_written():
    """The operators above, observed on the constructed points: on a bound or a gate one way, its neighbour the other."""
    prob, labels, extra = SS.constructed()
    out = SS.restate(prob)
    ex = lambda p, label: int(out[labels[(p, label)][0]]["exit"][labels[(p, label)][1]])
    for p in (0, 1, 2):
        for inside, outside in (("u==min", "u<min"), ("u<max", "u==max"), ("v==min", "v<min"), ("v<max", "v==max")):
            assert SS.EMPTY_WINDOW <= ex(p, inside) <= SS.MATCHED and ex(p, outside) == SS.NOT_IN_IMAGE, inside
        assert ex(p, "dist==0.8min") >= SS.EMPTY_WINDOW and ex(p, "dist<0.8min") == SS.TOO_NEAR
        assert ex(p, "dist==1.2max") >= SS.EMPTY_WINDOW and ex(p, "dist>1.2max") == SS.TOO_FAR
        assert ex(p, "dot==half") >= SS.EMPTY_WINDOW and ex(p, "dot<half") == SS.VIEW_ANGLE
    assert ex(0, "dist=50") == SS.MATCHED and ex(0, "dist=51") == SS.NO_CANDIDATE
    assert ex(1, "dist=75") == SS.MATCHED and ex(1, "dist=76") == SS.NO_CANDIDATE
    assert ex(3, "dist=50") == SS.MATCHED and ex(3, "dist=51") == SS.NO_CANDIDATE


def test_new_symbols_exported(api):
    L = api.lib()
    for s in ("gfs_sbp_reserve_sim3_search", "gfs_sim3_search", "gfs_test_sim3_search_groups"):
        assert hasattr(L, s), s
        assert s in api.ABI_SYMBOLS, s
    assert L.gfs_abi_version() == 1
    assert hasattr(api.ProjectionMatcher, "sim3_search") and hasattr(api.ProjectionMatcher, "reserve_sim3_search")
    hdr = open(os.path.join(ROOT, "include", "gfs_abi.h")).read()
    for i, name in enumerate(api.SIM3_SEARCH_EXITS):
        assert re.search(r"#define GFS_FUSE_%s %d\b" % (name.upper(), i), hdr), name
    for name, v in (("FUSE", api.SIM3_FUSE), ("SBP", api.SIM3_SBP), ("SBP_KFS", api.SIM3_SBP_KFS), ("SEARCH_LISTED", api.SIM3_SEARCH_LISTED)):
        assert re.search(r"#define GFS_SIM3_%s %d\b" % (name, v), hdr), name
    assert "between gfs_fuse_search and gfs_gba_solve" not in hdr
