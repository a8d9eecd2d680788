"""The constants of PoseLidarVisualInertialOptimizationLastKeyFrame / LastFrame that csrc/pose_lidar_inertial_rule.hpp compiles in beside
those of pose_inertial_rule.hpp: the lidar information 1e2 and its 1e2 factor behind the 0.8 s gap, the 4.0 validity gate, chi2IMU's
15.0 / 2.0 / 1e-2, the lidar Huber width sqrt(1.0), the 0.1 shift of frame mode, the 50-point gate of GenerateLidarEdge, both kernel-drop
conditions and the numeric Jacobian's 1e-9.  tests/golden/pose_lidar_inertial_constants.json holds the reference's values, parsed from
the reference itself when it is on the machine, and is compared with what the rule states through the restatement.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import pose_lidar_inertial_support as S

ROOT = S.ROOT
REF = "/root/reference"
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_lidar_inertial_constants.json")))


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="the reference sources are not on this machine")
def test_fixture_is_the_reference():
    opt = open(os.path.join(REF, "src", "Optimizer.cc")).read()
    unary = open(os.path.join(REF, "Thirdparty", "g2o", "g2o", "core", "base_unary_edge.hpp")).read()

    def body(name):
        a = opt.index("int Optimizer::" + name + "(")
        return opt[a:opt.index("\n}\n", a)]

    kf, fr = body("PoseLidarVisualInertialOptimizationLastKeyFrame"), body("PoseLidarVisualInertialOptimizationLastFrame")
    parsed = {}
    for tag, fn in (("keyframe", kf), ("frame", fr)):
        weak = re.search(r"float chi2IMU = ei->chi2\(\);\s+if \(chi2IMU > ([0-9.]+)\) \{\s+g2o::RobustKernelHuber\* rk = new g2o::RobustKernelHuber;\s+"
                         r"rk->setDelta\(([0-9.]+)\);\s+ei->setRobustKernel\(rk\);\s+ei->setInformation\(ei->information\(\) \* ([0-9.e-]+)\);", fn)
        one = dict(lidar_info=float(re.search(r"information\(0, 0\) = ([0-9.e]+);", fn).group(1)),
                   lidar_valid_chi2=float(re.search(r"if \(edge->chi2\(\) < ([0-9.]+)\) valid_edge\+\+;", fn).group(1)),
                   huber_lidar_squared=float(re.search(r"const float thHuberLidar = sqrt\(([0-9.]+)\);", fn).group(1)),
                   chi2_imu_gate=float(weak.group(1)), huber_inertial_weak=float(weak.group(2)), info_down=float(weak.group(3)),
                   min_edges=int(re.search(r"if \(optimizer\.edges\(\)\.size\(\) < (\d+)\)", fn).group(1)))
        for k, v in one.items():
            assert parsed.setdefault(k, v) == v, (tag, k)
        assert fn.index("float chi2IMU = ei->chi2();") < fn.index("optimizer.optimize(its[it]);")  # read at the top of the round
        assert fn.index("if (optimizer.edges().size() <") < fn.index("optimizer.removeEdge(edge)")  # the break sits before removeEdge
    far = re.search(r"if \(abs\(pFrame->mTimeStamp - pKF->mTimeStamp > ([0-9.]+)\)\) \{\s+edge->setInformation\(information \* ([0-9.e]+)\);", kf)
    parsed["kf_time_gap"], parsed["lidar_info_far"] = float(far.group(1)), float(far.group(2))
    assert "mTimeStamp - " not in fr
    shift = re.search(r"initPose\.block<3, 1>\(0, 3\) \+= Eigen::Vector3d\(([0-9.]+), ([0-9.]+), ([0-9.]+)\);", fr)
    parsed["init_shift"] = [float(shift.group(k)) for k in (1, 2, 3)]
    assert "initPose.block<3, 1>(0, 3) +=" not in kf
    parsed["kernel_drop_keyframe"] = sorted(set(re.findall(r"if \(it == ([^)]+)\) e->setRobustKernel\(0\);", kf)))
    parsed["kernel_drop_frame"] = sorted(set(re.findall(r"if \(it == ([^)]+)\) e->setRobustKernel\(0\);", fr)))
    gen = opt[opt.index("GenerateLidarEdge("):]
    parsed["min_cloud"] = int(re.search(r"mpPointCloudDownsampled->size\(\) < (\d+)", gen).group(1))
    parsed["numeric_delta"] = float(re.search(r"const double delta = ([0-9.e-]+);", unary).group(1))
    assert parsed == {k: v for k, v in GOLDEN.items() if k != "source"}


def test_constants_in_the_rule():
    g, c = GOLDEN, S.constants()
    assert (c["lidar_info"], c["lidar_info_far"], c["kf_time_gap"], c["lidar_valid_chi2"]) == (g["lidar_info"], g["lidar_info_far"], g["kf_time_gap"], g["lidar_valid_chi2"])
    assert (c["chi2_imu_gate"], c["huber_inertial_weak"], c["info_down"]) == (g["chi2_imu_gate"], g["huber_inertial_weak"], g["info_down"])
    assert c["huber_lidar"] == float(np.float32(np.sqrt(g["huber_lidar_squared"])))
    assert g["init_shift"] == [c["init_shift"]] * 3 and c["min_cloud"] == g["min_cloud"] and c["min_edges"] == g["min_edges"]
    assert c["numeric_delta"] == g["numeric_delta"] and c["perturbed"] == 12
    assert g["kernel_drop_keyframe"] == [str(int(c["kernel_drop_round_keyframe"]))]
    assert g["kernel_drop_frame"] == [f"nIterations - {int(c['kernel_drop_from_end_frame'])}"]
    rule = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "pose_lidar_inertial_rule.hpp")).read()
    assert "if (mode == kKeyFrame && kf_time_gap > kKfTimeGap) info = info * kLidarInfoFar;" in rule and "if (chi2IMU > kChi2ImuGate) {" in rule
    assert "if (mode == kFrame)\n    for (int r = 0; r < 3; r++) M[4 * r + 3] += kInitShift;" in rule
    for text in (open(os.path.join(ROOT, "tests", "host", "pose_lidar_inertial_restatement.cpp")).read(),
                 open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "pose_lidar_inertial.hip")).read()):
        assert "< R::kLidarValidChi2" in text or "c < kLidarValidChi2" in text
        assert "n_cloud < R::kMinCloud" in text or "LH.n_cloud < kMinCloud" in text
    hip = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "pose_lidar_inertial.hip")).read()
    lidar = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "pose_lidar.hip")).read()
    gates = re.search(r"kSqDisGate = ([0-9.]+), kPlaneGate = ([0-9.]+), kWeightSlope = ([0-9.]+), kMinWeight = ([0-9.]+);", hip).groups()
    assert [float(v) for v in gates] == [float(re.search(rf"constexpr double {k} = ([0-9.]+);", lidar).group(1))
                                         for k in ("kSqDisGate", "kPlaneGate", "kWeightSlope", "kMinWeight")]


def test_entry_points_are_declared_and_listed():
    from geoflowslam_amd import api
    head = open(os.path.join(ROOT, "include", "gfs_abi.h")).read()
    for name in ("gfs_pose_lidar_inertial_create", "gfs_pose_lidar_inertial_optimize", "gfs_pose_lidar_inertial_destroy",
                 "gfs_pose_lidar_inertial_fetch_edges"):
        assert name + "(" in head and name in api.ABI_SYMBOLS
