"""The constants of the frame cloud (LaserProcessingClass::featureExtraction, LidarParam's defaults): parsed from the reference when it
is on the machine (skipped otherwise) and compared with tests/golden/frame_cloud_constants.json; the fixture is compared with what the
CPU restatement, the kernel's rule header and the adaptor compile in.  Also: the new symbols are exported and api.FrameCloud refuses
loudly without a GPU."""
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
GOLDEN = os.path.join(ROOT, "tests", "golden", "frame_cloud_constants.json")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def parse_reference():
    lp, lidar = open(os.path.join(REF, "LidarProcess.cc")).read(), open(os.path.join(REF, "Lidar.cc")).read()
    one = lambda pat, text: re.search(pat, text, re.S).group(1)
    flat = lambda t: re.sub(r"\s+", " ", t).strip()
    g = {}
    g["scan_break_deg"] = float(one(r"fabs\(angle - last_angle\) > ([0-9.]+)\)", lp))
    g["min_scan_count"] = int(one(r"if \(count > (\d+)\)", lp))
    g["pad_copies"] = sorted(set(int(v) for v in re.findall(r"for \(int k = 0; k < (\d+); k\+\+\) \{\s*PointType point_temp;", lp)))
    g["pad_margin_start"] = flat(one(r"if \(start_angle > (.*?)\) \{", lp))
    g["pad_margin_end"] = flat(one(r"if \(end_angle < (.*?)\) \{", lp))
    g["edge_min_value"] = float(one(r"cloudCurvature\[i\]\.value <= ([0-9.]+)\)", lp))
    g["max_edge_picks"] = int(one(r"largestPickedNum <= (\d+)\)", lp))
    g["pick_halo"] = [int(v) for v in re.search(r"for \(int k = (-?\d+); k <= (\d+); k\+\+\) \{\s*if \(k != 0\) picked_points", lp).groups()]
    g["edge_min_neighbors"] = int(one(r"edge_noise_filter\.setMinNeighborsInRadius\((\d+)\)", lp))
    g["surf_min_neighbors"] = int(one(r"surf_noise_filter\.setMinNeighborsInRadius\((\d+)\)", lp))
    g["edge_leaf_divisor"] = float(one(r"edge_downsize_filter\.setLeafSize\(map_resolution / ([0-9.]+),", lp))
    g["surf_leaf_divisor"] = float(one(r"surf_downsize_filter\.setLeafSize\(map_resolution / ([0-9.]+),", lp))
    g["radius_is_map_resolution"] = "edge_noise_filter.setRadiusSearch(map_resolution)" in lp and "surf_noise_filter.setRadiusSearch(map_resolution)" in lp
    g["init_reads"] = one(r"double map_resolution = lidar_param\.(\w+)\(\)", lp)
    for k in ("max_distance", "horizontal_angle", "local_map_resolution"):
        g["default_" + k] = float(one(r'%s = readDouble\(node, "%s", ([0-9.]+)\)' % (k, k), lidar))
    g["curvature"] = flat(one(r"Double2d distance\(\s*j, (.*?)\);", lp))
    g["angle"] = flat(one(r"double angle =\s*(atan2.*?);", lp))
    g["sort_compare"] = flat(one(r"\[\]\(const Double2d& a, const Double2d& b\) \{ (.*?) \}", lp))
    return g


def test_constants_match_reference():
    if not os.path.isdir(REF):
        pytest.skip("the reference is not on this machine")
    assert parse_reference() == json.load(open(GOLDEN))


def test_restatement_rule_header_and_adaptor_hold_the_constants():
    g = json.load(open(GOLDEN))
    res, rule = _read("tests", "host", "frame_cloud_restatement.cpp"), _read("geoflowslam_amd", "csrc", "frame_cloud_rule.hpp")
    ada, hip = _read("geoflowslam_amd", "host", "gfs_adaptors.hpp"), _read("geoflowslam_amd", "csrc", "frame_cloud.hip")
    num = lambda v: repr(float(v)).rstrip("0") if float(v) != int(v) else "%.1f" % v
    # the sequential restatement, literally
    assert "std::fabs(angle - last_angle) > %s" % num(g["scan_break_deg"]) in res and "if (count > %d)" % g["min_scan_count"] in res
    assert g["pad_copies"] == [5] and res.count("for (int k = 0; k < 5; k++) s.push_back") == 2
    assert g["pad_margin_start"] == "-lidar_param.getHorizontalAngle() / 2.0 + 5.0" and "> -horizontal_angle / 2.0 + 5.0" in res
    assert g["pad_margin_end"] == "lidar_param.getHorizontalAngle() / 2.0 - 5.0" and "< horizontal_angle / 2.0 - 5.0" in res
    assert "cv[i].value <= %s" % num(g["edge_min_value"]) in res and "if (picks <= %d)" % g["max_edge_picks"] in res
    assert g["pick_halo"] == [-5, 5] and "for (int k = -5; k <= 5; k++) picked[id + k] = 1;" in res
    assert "resolution, %d, &g_stage[4]" % g["edge_min_neighbors"] in res and "resolution, %d, &g_stage[5]" % g["surf_min_neighbors"] in res
    assert "(float)(resolution / %s)" % num(g["edge_leaf_divisor"]) in res and "(float)(resolution / %s)" % num(g["surf_leaf_divisor"]) in res
    assert g["curvature"] == "diffX * diffX + diffY * diffY + diffZ * diffZ / point_distance" and g["curvature"] in res and g["curvature"] in rule
    assert g["angle"].startswith("atan2(") and g["angle"].endswith("* 180 / M_PI") and "* 180 / M_PI" in res and "* 180 / M_PI" in rule
    assert g["sort_compare"] == "return a.value < b.value;" and g["sort_compare"] in res
    assert g["radius_is_map_resolution"] and g["init_reads"] == "getLocalMapResolution"
    # the kernel's rule header, by name
    for name, v in (("kScanBreakDeg", g["scan_break_deg"]), ("kPadMarginDeg", 5.0), ("kEdgeMinValue", g["edge_min_value"]),
                    ("kEdgeLeafDivisor", g["edge_leaf_divisor"]), ("kSurfLeafDivisor", g["surf_leaf_divisor"]),
                    ("kDefaultHorizontalAngle", g["default_horizontal_angle"]), ("kDefaultMaxDistance", g["default_max_distance"]),
                    ("kDefaultLocalMapResolution", g["default_local_map_resolution"])):
        assert re.search(r"\b%s = %s\b" % (name, re.escape(num(v))), rule), name
    for name, v in (("kMinScanCount", g["min_scan_count"]), ("kPad", g["pad_copies"][0]), ("kMaxEdgePicks", g["max_edge_picks"]),
                    ("kPickHalo", g["pick_halo"][1]), ("kEdgeMinNeighbors", g["edge_min_neighbors"]),
                    ("kSurfMinNeighbors", g["surf_min_neighbors"]), ("kMaxCandidates", 1024)):
        assert re.search(r"\bconstexpr int %s = %d;" % (name, v), rule), name
    assert "d > kScanBreakDeg" in hip and "ib - run > kMinScanCount" in hip and "<= kEdgeMinValue" in hip and "largest > kMaxEdgePicks" in hip
    assert "kSurfMinNeighbors, nullptr" in hip and "kEdgeMinNeighbors, &c->n_surf" in hip
    # the adaptor reads the reference's getters
    for getter in ("getHorizontalAngle()", "getMaxDistance()", "getLocalMapResolution()"):
        assert "lp." + getter in ada
    assert "-ffp-contract=off" in _read("tests", "frame_cloud_support.py") and "EXACT := -ffp-contract=off" in _read("geoflowslam_amd", "csrc", "Makefile")


def test_default_config(api):
    g = json.load(open(GOLDEN))
    cfg = api.FrameCloudConfig()
    api.lib().gfs_frame_cloud_default_config(cfg)
    assert (cfg.horizontal_angle, cfg.max_distance, cfg.local_map_resolution, cfg.angle_guard_deg) == \
        (g["default_horizontal_angle"], g["default_max_distance"], g["default_local_map_resolution"], 1e-9)


def test_new_symbols_exported(api):
    L = api.lib()
    for s in ("gfs_frame_cloud_default_config", "gfs_frame_cloud_create", "gfs_frame_cloud_destroy", "gfs_frame_cloud_extract",
              "gfs_frame_cloud_extract_device", "gfs_test_frame_cloud_stages", "gfs_test_frame_cloud_radius"):
        assert hasattr(L, s), s
        assert s in api.ABI_SYMBOLS, s
    assert L.gfs_abi_version() == 1
    for m in ("extract", "extract_device", "stages"):
        assert callable(getattr(api.FrameCloud, m, None)), m


def test_frame_cloud_raises_without_gpu(api):
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(api.GfsError):
        api.FrameCloud()
