"""The constants of PoseLidarVisualOptimization / GenerateLidarEdge: read from the reference when it is on the machine, else from
tests/golden/pose_lidar_constants.json, and compared with what the CPU restatement and the HIP source compile in.  Also: the new
entry points are exported, and the new classes refuse to run without a GPU.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import pose_lidar_support as PLS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src/Optimizer.cc"
NAMES = ("k_neighbours", "sqdis_gate", "plane_gate", "weight_slope", "min_weight", "lidar_information", "huber_delta_lidar",
         "valid_chi2", "min_cloud")


def _expected():
    if os.path.exists(REF):
        src = open(REF).read()
        a = src.index("int Optimizer::PoseLidarVisualOptimization(")
        body = src[a:src.index("\n}\n", a)]
        g = src.index("vector<EdgeType*> Optimizer::GenerateLidarEdge(")
        gen = src[g:src.index("\n}\n", g)]
        return dict(
            k_neighbours=int(re.search(r"nearestKSearch\(pointSel, (\d+),", gen).group(1)),
            sqdis_gate=float(re.search(r"pointSearchSqDis\[4\] < ([0-9.]+)\)", gen).group(1)),
            plane_gate=float(re.search(r"pd\) > ([0-9.]+)\)", gen).group(1)),
            weight_slope=float(re.search(r"float s = 1 - ([0-9.]+) \* fabs\(pd2\)", gen).group(1)),
            min_weight=float(re.search(r"if \(s > ([0-9.]+)\)", gen).group(1)),
            lidar_information=float(re.search(r"information\(0, 0\) = ([0-9.e]+);", body).group(1)),
            huber_delta_lidar=float(np.sqrt(float(re.search(r"thHuberLidar = sqrt\(([0-9.]+)\)", body).group(1)))),
            valid_chi2=float(re.search(r"if \(edge->chi2\(\) < ([0-9.]+)\) valid_edge", body).group(1)),
            min_cloud=int(re.search(r"mpPointCloudDownsampled->size\(\) < (\d+)\)", gen).group(1)),
            its=[int(v) for v in re.search(r"const int its\[4\] = \{([^}]*)\}", body).group(1).split(",")])
    return json.load(open(os.path.join(ROOT, "tests", "golden", "pose_lidar_constants.json")))


def test_constants_match_reference():
    exp = _expected()
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_lidar_constants.json")))
    for k in NAMES + ("its",):
        assert exp[k] == golden[k], k  # the fixture is the reference's values
    out = np.zeros(14)
    PLS.restatement().plr_constants(out.ctypes.data)
    assert list(out[:9]) == [float(exp[k]) for k in NAMES]
    assert list(out[9:13]) == [float(v) for v in exp["its"]]
    hip = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "pose_lidar.hip")).read()
    got = dict(
        sqdis_gate=float(re.search(r"kSqDisGate = ([0-9.e]+);", hip).group(1)),
        plane_gate=float(re.search(r"kPlaneGate = ([0-9.e]+);", hip).group(1)),
        weight_slope=float(re.search(r"kWeightSlope = ([0-9.e]+);", hip).group(1)),
        min_weight=float(re.search(r"kMinWeight = ([0-9.e]+);", hip).group(1)),
        lidar_information=float(re.search(r"kLidarInfo = ([0-9.e]+);", hip).group(1)),
        huber_delta_lidar=float(re.search(r"kThHuberLidar = ([0-9.e]+);", hip).group(1)),
        valid_chi2=float(re.search(r"kLidarValidChi2 = ([0-9.e]+);", hip).group(1)),
        min_cloud=int(re.search(r"kMinCloud = (\d+);", hip).group(1)),
        k_neighbours=len(re.findall(r"float d\[5\];", hip)) and 5,
        its=[int(v) for v in re.search(r"kIts\[4\] = \{([^}]*)\}", hip).group(1).split(",")])
    for k in got:
        assert got[k] == exp[k], k
    assert "double kSqDisGate" in hip and "double kPlaneGate" in hip and "double kMinWeight" in hip  # compared as doubles


def test_new_symbols_exported(api):
    L = api.lib()
    for s in ("gfs_lidar_map_create", "gfs_lidar_map_set", "gfs_lidar_map_destroy", "gfs_pose_lidar_create", "gfs_pose_lidar_destroy",
              "gfs_pose_lidar_set_sum_order", "gfs_pose_lidar_optimize", "gfs_pose_lidar_fetch_edges"):
        assert hasattr(L, s), s
        assert s in api.ABI_SYMBOLS, s


def test_new_classes_raise_without_gpu(api):
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(api.GfsError):
        api.LidarMap()
    with pytest.raises(api.GfsError):
        api.PoseLidarOptimizer()
