"""The constants of PoseInertialOptimizationLastKeyFrame / LastFrame that csrc/pose_inertial_rule.hpp compiles in: both gate tables, the
Huber widths 6 / 2 / 5, 15.0 and 1e-2, 18 / 24, 30, 10 edges and the 10 iterations, the 1e-5 branch thresholds, GRAVITY_VALUE, the
non-finite replacement.  tests/golden/pose_inertial_constants.json holds the reference's values, parsed from the reference itself when it
is on the machine, and is compared with what the rule states through the restatement.  Also: the entry points are declared and listed.
No GPU."""
import json
import os
import re

import numpy as np
import pytest

import pose_inertial_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_inertial_constants.json")))


def _floats(text):
    return [float(v.rstrip("f")) for v in text.split(",")]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="the reference sources are not on this machine")
def test_fixture_is_the_reference():
    opt = open(os.path.join(REF, "src", "Optimizer.cc")).read()
    g2o = open(os.path.join(REF, "src", "G2oTypes.cc")).read()
    imu = open(os.path.join(REF, "src", "ImuTypes.cc")).read()
    imu_h = open(os.path.join(REF, "include", "ImuTypes.h")).read()

    def body(name):
        a = opt.index("int Optimizer::" + name + "(")
        return opt[a:opt.index("\n}\n", a)]

    parsed = {}
    for tag, fn in (("keyframe", body("PoseInertialOptimizationLastKeyFrame")), ("frame", body("PoseInertialOptimizationLastFrame"))):
        parsed[f"chi2_mono_{tag}"] = _floats(re.search(r"float chi2Mono\[4\] = \{([^}]*)\};", fn).group(1))
        parsed[f"chi2_stereo_{tag}"] = _floats(re.search(r"float chi2Stereo\[4\] = \{([^}]*)\};", fn).group(1))
        parsed[f"iterations_{tag}"] = [int(v) for v in re.search(r"int its\[4\] = \{([^}]*)\};", fn).group(1).split(",")]
        # what both functions share, each stated once per function: the same in both
        one = dict(
            huber_mono_squared=float(re.search(r"const float thHuberMono = sqrt\(([0-9.]+)\);", fn).group(1)),
            huber_stereo_squared=float(re.search(r"const float thHuberStereo = sqrt\(([0-9.]+)\);", fn).group(1)),
            huber_inertial=float(re.search(r"ei->setRobustKernel\(rk\);\s+rk->setDelta\(([0-9.]+)\);", fn).group(1)),
            chi2_close_factor=float(re.search(r"float chi2close = ([0-9.]+) \* chi2Mono\[it\];", fn).group(1)),
            chi2_mono_out=float(re.search(r"const float chi2MonoOut = ([0-9.]+)f;", fn).group(1)),
            chi2_stereo_out=float(re.search(r"const float chi2StereoOut = ([0-9.]+)f;", fn).group(1)),
            few_inliers=int(re.search(r"if \(\(nInliers < (\d+)\) && !bRecInit\)", fn).group(1)),
            min_edges=int(re.search(r"if \(optimizer\.edges\(\)\.size\(\) < (\d+)\)", fn).group(1)),
            track_depth_close=float(re.search(r"mTrackDepth < ([0-9.]+)f;", fn).group(1)))
        for k, v in one.items():
            assert parsed.setdefault(k, v) == v, (tag, k)
    kf, fr = body("PoseInertialOptimizationLastKeyFrame"), body("PoseInertialOptimizationLastFrame")
    weak = re.search(r"if \(chi2IMU > ([0-9.]+)\) \{\s+g2o::RobustKernelHuber\* rk = new g2o::RobustKernelHuber;\s+rk->setDelta\(([0-9.]+)\);\s+"
                     r"ei->setRobustKernel\(rk\);\s+ei->setInformation\(ei->information\(\) \* ([0-9.e-]+)\);", kf)
    parsed["chi2_imu_gate"], parsed["huber_inertial_weak"], parsed["info_down"] = float(weak.group(1)), float(weak.group(2)), float(weak.group(3))
    assert "chi2IMU" not in fr
    parsed["huber_prior"] = float(re.search(r"ep->setRobustKernel\(rkp\);\s+rkp->setDelta\(([0-9.]+)\);", fr).group(1))
    upd = g2o[g2o.index("void ImuCamPose::Update(const double* pu) {"):g2o.index("void ImuCamPose::UpdateW(")]
    parsed["normalize_every"] = int(re.search(r"if \(its >= (\d+)\) \{", upd).group(1))
    so3 = g2o[g2o.index("// SO3 FUNCTIONS"):]
    parsed["small_angle_thresholds"] = [float(v) for v in re.findall(r"if \((?:d|fabs\(s\)) < ([0-9.e-]+)\)", so3)]
    parsed["gravity"] = float(re.search(r"const float GRAVITY_VALUE = ([0-9.]+);", imu_h).group(1))
    rot = imu[imu.index("Eigen::Matrix3f Preintegrated::GetDeltaRotation(const Bias &b_) {"):]
    parsed["dbg_replacement"] = _floats(re.search(r"if\(!dbg\.allFinite\(\)\)\{\s+dbg = Eigen::Vector3f\(([^)]*)\);", rot).group(1))
    assert parsed == {k: v for k, v in GOLDEN.items() if k != "source"}


def test_constants_in_the_rule():
    g, c = GOLDEN, S.constants()
    f32 = lambda v: [float(np.float32(x)) for x in v]
    assert c["chi2_mono_keyframe"] == f32(g["chi2_mono_keyframe"]) and c["chi2_mono_frame"] == f32(g["chi2_mono_frame"])
    assert c["chi2_stereo"] == f32(g["chi2_stereo_keyframe"]) == f32(g["chi2_stereo_frame"])
    assert g["iterations_keyframe"] == g["iterations_frame"] == [c["iterations"]] * 4
    assert c["huber_mono"] == float(np.float32(np.sqrt(g["huber_mono_squared"]))) and c["huber_stereo"] == float(np.float32(np.sqrt(g["huber_stereo_squared"])))
    assert (c["huber_inertial"], c["huber_inertial_weak"], c["huber_prior"]) == (g["huber_inertial"], g["huber_inertial_weak"], g["huber_prior"])
    assert (c["chi2_imu_gate"], c["info_down"]) == (g["chi2_imu_gate"], g["info_down"])
    assert (c["chi2_mono_out"], c["chi2_stereo_out"], c["few_inliers"], c["min_edges"]) == (g["chi2_mono_out"], g["chi2_stereo_out"], g["few_inliers"], g["min_edges"])
    assert c["track_depth_close"] == g["track_depth_close"] and c["normalize_every"] == g["normalize_every"]
    assert set(g["small_angle_thresholds"]) == {c["small_angle"]} and len(g["small_angle_thresholds"]) == 4
    assert c["gravity"] == float(np.float32(g["gravity"])) and c["dbg_replacement"] == f32(g["dbg_replacement"])
    rule = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "pose_inertial_rule.hpp")).read()
    assert f"(float)({g['chi2_close_factor']} * (double)chi2_mono_gate(mode, it))" in rule
    # the comparison operators of the re-classification, the recovery and the two gates
    assert "(chi2 > chi2_mono_gate(mode, it) && !close) || (close && chi2 > chi2_close_gate(mode, it)) || !depth_positive" in rule
    assert "return chi2 > chi2_stereo_gate(it);" in rule and "if (chi2IMU > kChi2ImuGate) {" in rule and "if (s.its >= kNormalizeEvery) {" in rule
    rst = open(os.path.join(ROOT, "tests", "host", "pose_inertial_restatement.cpp")).read()
    assert "if (nInliers < kFewInliers && !h.rec_init) {" in rst and "if (edge_count(h.mode, n) < kMinEdges) break;" in rst
    assert "< (st ? kChi2StereoOut : kChi2MonoOut)) ve[e].outlier = 0;" in rst
    hip = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "pose_inertial.hip")).read()
    assert "if (nInliers < kFewInliers && !h.rec_init) {" in hip and "if (edge_count(mode, n) < kMinEdges) break;" in hip


def test_entry_points_are_declared_and_listed():
    from geoflowslam_amd import api
    head = open(os.path.join(ROOT, "include", "gfs_abi.h")).read()
    for name in ("gfs_pose_inertial_create", "gfs_pose_inertial_optimize", "gfs_pose_inertial_destroy"):
        assert name + "(" in head and name in api.ABI_SYMBOLS
    assert [int(v) for v in re.findall(r"#define GFS_POSE_INERTIAL_LAST_\w+ (\d)", head)] == [api.POSE_INERTIAL_LAST_KEYFRAME, api.POSE_INERTIAL_LAST_FRAME]
    assert "gfs_abi_version" in head
