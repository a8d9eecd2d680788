"""The constants of Tracking::SearchLocalPoints / Frame::isInFrustum / RadiusByViewingCos: read from the reference when it is on the
machine, else from tests/golden/local_points_constants.json, and compared with what the CPU restatement, the HIP source and the
adaptor compile in.  Also: the new entry points are exported.  No GPU."""
import json
import os
import re

import numpy as np

import local_points_support as LPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
GOLDEN = os.path.join(ROOT, "tests", "golden", "local_points_constants.json")
NAMES = ("min_distance_factor", "max_distance_factor", "view_cos_limit", "nn_ratio", "depth_test", "bounds_tests", "radius_cos_threshold",
         "radius_near", "radius_far")


def _body(src, head):
    a = src.index(head)
    return src[a:src.index("\n}\n", a)]


def _expected():
    if os.path.isdir(REF):
        mp = open(os.path.join(REF, "MapPoint.cc")).read()
        tr = _body(open(os.path.join(REF, "Tracking.cc")).read(), "void Tracking::SearchLocalPoints()")
        fr = _body(open(os.path.join(REF, "Frame.cc")).read(), "bool Frame::isInFrustum(")
        fr = fr[:fr.index("} else {")]  # the Nleft == -1 branch
        rad = _body(open(os.path.join(REF, "ORBmatcher.cc")).read(), "float ORBmatcher::RadiusByViewingCos(")
        bx = re.search(r"if \(uv\(0\) (\S+) mnMinX \|\| uv\(0\) (\S+) mnMaxX\) return false;", fr)
        by = re.search(r"if \(uv\(1\) (\S+) mnMinY \|\| uv\(1\) (\S+) mnMaxY\) return false;", fr)
        return dict(
            min_distance_factor=float(re.search(r"return ([0-9.]+)f \* mfMinDistance;", mp).group(1)),
            max_distance_factor=float(re.search(r"return ([0-9.]+)f \* mfMaxDistance;", mp).group(1)),
            view_cos_limit=float(re.search(r"isInFrustum\(pMP, ([0-9.]+)\)", tr).group(1)),
            nn_ratio=float(re.search(r"ORBmatcher matcher\(([0-9.]+)\);", tr).group(1)),
            depth_test=re.search(r"if \(PcZ (\S+) 0\.0f\) return false;", fr).group(1),
            bounds_tests=[bx.group(1), bx.group(2), by.group(1), by.group(2)],
            radius_cos_threshold=float(re.search(r"viewCos > ([0-9.]+)\)", rad).group(1)),
            radius_near=float(re.findall(r"return ([0-9.]+);", rad)[0]),
            radius_far=float(re.findall(r"return ([0-9.]+);", rad)[1]))
    return json.load(open(GOLDEN))


def _ops(text, u, v):
    """the comparison operators of the four image-bounds tests in a source text that names the projection u / v"""
    bx = re.search(r"if \(%s (\S+) \S*min_x \|\| %s (\S+) \S*max_x\) break;" % (u, u), text) or \
        (re.search(r"if \(%s (\S+) \S*min_x\) return" % u, text), re.search(r"if \(%s (\S+) \S*max_x\) return" % u, text))
    by = re.search(r"if \(%s (\S+) \S*min_y \|\| %s (\S+) \S*max_y\) break;" % (v, v), text) or \
        (re.search(r"if \(%s (\S+) \S*min_y\) return" % v, text), re.search(r"if \(%s (\S+) \S*max_y\) return" % v, text))
    flat = lambda m: [m.group(1), m.group(2)] if not isinstance(m, tuple) else [m[0].group(1), m[1].group(1)]
    return flat(bx) + flat(by)


def test_constants_match_reference():
    exp = _expected()
    golden = json.load(open(GOLDEN))
    for k in NAMES:
        assert exp[k] == golden[k], k  # the fixture is the reference's values
    f = np.float32
    # the restatement
    out = np.zeros(2, np.float32)
    LPS.restatement().lpr_constants(out.ctypes.data)
    assert out[0] == f(exp["min_distance_factor"]) and out[1] == f(exp["max_distance_factor"])
    rst = open(os.path.join(ROOT, "tests", "host", "local_points_restatement.cpp")).read()
    assert _ops(rst, "u", "v") == exp["bounds_tests"]
    assert re.search(r"if \(Pc\[2\] (\S+) 0\.0f\) return", rst).group(1) == exp["depth_test"]
    orc = open(os.path.join(ROOT, "oracle", "sbp_oracle.cpp")).read()
    m = re.search(r"mp_view_cos\[l\] > ([0-9.]+) \? ([0-9.]+)f : ([0-9.]+)f;", orc)
    assert [float(v) for v in m.groups()] == [exp["radius_cos_threshold"], exp["radius_near"], exp["radius_far"]]
    # the HIP source
    hip = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "local_points.hip")).read()
    assert float(re.search(r"kLpMinDistFactor = ([0-9.]+)f;", hip).group(1)) == exp["min_distance_factor"]
    assert float(re.search(r"kLpMaxDistFactor = ([0-9.]+)f;", hip).group(1)) == exp["max_distance_factor"]
    assert "dist < kLpMinDistFactor * min_dist[at] || dist > kLpMaxDistFactor * mx" in hip
    assert _ops(hip, "u", "v") == exp["bounds_tests"]
    assert re.search(r"if \(Pc\[2\] (\S+) 0\.0f\) break;", hip).group(1) == exp["depth_test"]
    sbp = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "sbp.hip")).read()  # the search radius is k_sbp's
    m = re.search(r"last_angle\[l\] > ([0-9.]+) \? ([0-9.]+)f : ([0-9.]+)f;", sbp)
    assert [float(v) for v in m.groups()] == [exp["radius_cos_threshold"], exp["radius_near"], exp["radius_far"]]
    # what the adaptor passes for the two arguments Tracking fixes
    ada = open(os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp")).read()
    assert float(re.search(r"kSearchLocalPointsViewCosLimit = ([0-9.]+)f;", ada).group(1)) == exp["view_cos_limit"]
    assert float(re.search(r"kSearchLocalPointsNNRatio = ([0-9.]+)f;", ada).group(1)) == exp["nn_ratio"]


def test_inclusive_bounds_and_distance_gates_behave_as_written():
    """The operators above, observed: a point exactly on a bound or a gate stays, its neighbour one ulp outside goes."""
    name, prob, labels = LPS.constructed_frames()[0]
    r = LPS.restate(prob)
    for on, off in (("u==min_x", "u==min_x+1ulp_out"), ("u==max_x", "u==max_x+1ulp_out"), ("v==min_y", "v==min_y+1ulp_out"),
                    ("v==max_y", "v==max_y+1ulp_out"), ("dist==0.8min", "dist<0.8min"), ("dist==1.2max", "dist>1.2max"),
                    ("cos==limit", "cos<limit")):
        assert r["in_view"][labels[on][0]] == 1 and r["in_view"][labels[off][0]] == 0, on


def test_new_symbols_exported(api):
    L = api.lib()
    for s in ("gfs_sbp_reserve_local", "gfs_search_local_points", "gfs_test_glibc_logf"):
        assert hasattr(L, s), s
        assert s in api.ABI_SYMBOLS, s
    assert L.gfs_abi_version() == 1
    assert hasattr(api.ProjectionMatcher, "search_local_points") and hasattr(api.ProjectionMatcher, "reserve_local")
