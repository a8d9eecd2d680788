"""The choices MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth compile in (the median's index expression, the `<` of
the best-median test, the `-1` tests of the indices): tests/golden/map_point_constants.json holds the reference's, parsed from the
reference itself when it is on the machine, and is compared with the CPU restatement, the rule header the kernel is built from and
the adaptor.  Also: the new entry points are exported, and MapPointUpdater refuses loudly without a GPU.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import map_point_support as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "map_point_constants.json")))


def _body(src, head):
    a = src.index(head)
    return src[a:src.index("\n}\n", a)]


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference sources are not on this machine")
def test_fixture_is_the_reference():
    mp = open(os.path.join(REF, "MapPoint.cc")).read()
    cdd = _body(mp, "void MapPoint::ComputeDistinctiveDescriptors() {")
    und = _body(mp, "void MapPoint::UpdateNormalAndDepth() {")
    m = re.search(r"if \(leftIndex (\S+ -1)\s*&& leftIndex (\S+) pKF->mDescriptors\.rows\)", cdd)
    got = dict(median_index=re.search(r"int median = vDists\[(.+?)\];", cdd).group(1),
               best_test=re.search(r"if \(median (\S+) BestMedian\)", cdd).group(1),
               best_median_start=re.search(r"int BestMedian = (\w+);", cdd).group(1),
               desc_index_test=m.group(1), desc_rows_test=m.group(2),
               normal_index_test=re.search(r"if \(leftIndex (\S+ -1)\) \{\s+Eigen::Vector3f Owi = pKF->GetCameraCenter\(\);", und).group(1))
    for k, v in got.items():
        assert v == GOLDEN[k], k
    assert "Distances[i][i] = 0;" in cdd and "normal = normal + normali / normali.norm();" in und and "mNormalVector = normal / n;" in und
    assert "mfMaxDistance = dist * levelScaleFactor;" in und and "mfMinDistance = mfMaxDistance / pRefKF->mvScaleFactors[nLevels - 1];" in und


def test_constants_in_restatement_rule_and_adaptor():
    g = GOLDEN
    assert g["median_index"] == "0.5 * (N - 1)" and g["best_test"] == "<" and g["best_median_start"] == "INT_MAX"
    rst = open(os.path.join(ROOT, "tests", "host", "map_point_restatement.cpp")).read()
    assert re.search(r"int median = vDists\[(.+?)\];", rst).group(1) == g["median_index"]
    assert re.search(r"if \(median (\S+) BestMedian\)", rst).group(1) == g["best_test"]
    assert re.search(r"int BestMedian = (\w+);", rst).group(1) == g["best_median_start"]
    out = np.zeros(2, np.int32)
    for N in range(1, 40):  # what the expression converts to: even N takes the lower middle
        MS.restatement().mr_constants(N, 3, 3, out.ctypes.data)
        assert out[0] == int(0.5 * (N - 1)) == (N - 1) // 2 and out[1] == 0
    MS.restatement().mr_constants(5, 2, 3, out.ctypes.data)
    assert out[1] == 1
    # the rule header the kernel and the host path are built from
    rule = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "map_point_rule.hpp")).read()
    assert re.search(r"int median_index\(int n\) \{ return \(int\)\((.+?)\); \}", rule).group(1) == g["median_index"].replace("N", "n")
    assert re.search(r"bool better_median\(int median, int best\) \{ return median (\S+) best; \}", rule).group(1) == g["best_test"]
    assert "int best = 0x7fffffff;  // INT_MAX" in rule
    hip = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "map_points.hip")).read()
    assert hip.count("gfs_mp::better_median(") == 2 and hip.count("gfs_mp::median_index(nd)") == 1 and "int best = 0x7fffffff" in hip
    assert "gfs_mp::normal_term(pos, Ow, t)" in hip and "gfs_mp::finish_normal(sum, cnt, pos, ref," in hip
    # the adaptor's flags are the reference's index tests
    ada = open(os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp")).read()
    assert "if (leftIndex %s) {\n        if (!pKF) throw" % g["normal_index_test"] in ada
    assert "if (with_desc && pKF && !pKF->isBad() && leftIndex %s && leftIndex %s Access::descriptor_rows(*pKF)) {" % (g["desc_index_test"], g["desc_rows_test"]) in ada
    assert "at == observations.end() ? 0 : std::get<0>(at->second)" in ada


def test_new_symbols_exported(api):
    L = api.lib()
    for s in ("gfs_map_points_create", "gfs_map_points_destroy", "gfs_map_points_update"):
        assert hasattr(L, s), s
        assert s in api.ABI_SYMBOLS, s
    assert L.gfs_abi_version() == 1
    assert hasattr(api.MapPointUpdater, "update") and hasattr(api, "map_points_structs") and hasattr(api, "map_points_results")
    hdr = open(os.path.join(ROOT, "include", "gfs_abi.h")).read()
    for name, v in (("GFS_MAP_POINTS_FULL", api.MAP_POINTS_FULL), ("GFS_MAP_POINTS_NORMALS_ONLY", api.MAP_POINTS_NORMALS_ONLY),
                    ("GFS_MAP_POINT_OBS_IN_NORMAL", api.MAP_POINT_OBS_IN_NORMAL), ("GFS_MAP_POINT_OBS_IN_DESC", api.MAP_POINT_OBS_IN_DESC),
                    ("GFS_MAP_POINT_NORMAL_SET", api.MAP_POINT_NORMAL_SET), ("GFS_MAP_POINT_DESC_SET", api.MAP_POINT_DESC_SET)):
        assert re.search(r"#define %s\s+%d\b" % (name, v), hdr), name


def test_updater_refuses_loudly_without_a_gpu(api):
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(api.GfsError) as e:
        api.MapPointUpdater(16, 64)
    assert e.value.code == -2 and "no CPU fallback" in str(e.value)
