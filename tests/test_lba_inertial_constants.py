"""The constants of Optimizer::LocalInertialBA that csrc/lba_inertial_rule.hpp compiles in: the window sizes 10 / 20, the iterations
8 / 4, lambda 1e0 / 1e-2, the Huber widths sqrt(16.0), sqrt(5.991), sqrt(7.815), the 1e-2 of the last inertial edge, the erase gates
5.991 / 7.815 / 1.5f / 10.f, maxFixKF, maxCovKF, the fail gate's factor, and the Levenberg fork's ten trials, 1e-3 and _nBad >= 3.
tests/golden/lba_inertial_constants.json holds the reference's values, parsed from the reference itself when it is on the machine, and
is compared with what the rule states through the restatement.  Also: the entry points are declared and listed.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import lba_inertial_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "lba_inertial_constants.json")))


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="the reference sources are not on this machine")
def test_fixture_is_the_reference():
    opt = open(os.path.join(REF, "src", "Optimizer.cc")).read()
    a = opt.index("void Optimizer::LocalInertialBA(")
    fn = opt[a:opt.index("\n}\n", a)]
    lm = open(os.path.join(REF, "Thirdparty", "g2o", "g2o", "core", "optimization_algorithm_levenberg.cpp")).read()
    num = r"([0-9.e-]+)"
    m = re.search(r"int maxOpt = (\d+);\s+int opt_it = (\d+);\s+if \(bLarge\) \{\s+maxOpt = (\d+);\s+opt_it = (\d+);", fn)
    lam = re.search(r"if \(bLarge\) \{.*?setUserLambdaInit\(\s*" + num + r"\);.*?\} else \{.*?setUserLambdaInit\(" + num + r"\);", fn, re.S)
    parsed = dict(
        max_opt=[int(m.group(1)), int(m.group(3))], opt_it=[int(m.group(2)), int(m.group(4))], lambda_init=[float(lam.group(2)), float(lam.group(1))],
        huber_inertial_squared=float(re.search(r"rki->setDelta\(sqrt\(" + num + r"\)\);", fn).group(1)),
        info_down_last=float(re.search(r"if \(i == N - 1\) vei\[i\]->setInformation\(vei\[i\]->information\(\) \* " + num + r"\);", fn).group(1)),
        huber_mono_squared=float(re.search(r"const float thHuberMono = sqrt\(" + num + r"\);", fn).group(1)),
        huber_stereo_squared=float(re.search(r"const float thHuberStereo = sqrt\(" + num + r"\);", fn).group(1)),
        chi2_mono2=float(re.search(r"const float chi2Mono2 = " + num + ";", fn).group(1)),
        chi2_stereo2=float(re.search(r"const float chi2Stereo2 = " + num + ";", fn).group(1)),
        chi2_close_factor=float(re.search(r"e->chi2\(\) > " + num + r"f \* chi2Mono2 && bClose", fn).group(1)),
        track_depth_close=float(re.search(r"bool bClose = pMP->mTrackDepth < " + num + "f;", fn).group(1)),
        max_fix_kf=int(re.search(r"const int maxFixKF = (\d+);", fn).group(1)), max_cov_kf=int(re.search(r"const int maxCovKF = (\d+);", fn).group(1)),
        fail_gate_factor=int(re.search(r"if \(\((\d+) \* err < err_end \|\| isnan\(err\) \|\| isnan\(err_end\)\) && !bLarge\)", fn).group(1)),
        max_trials=int(re.search(r'_maxTrialsAfterFailure = _properties.makeProperty<Property<int> >\("maxTrialsAfterFailure", (\d+)\);', lm).group(1)),
        scale_guard=float(re.search(r"scale \+= " + num + ";", lm).group(1)), n_bad_stop=int(re.search(r"if\(_nBad>=(\d+)\)", lm).group(1)))
    assert "bRecInit" not in fn[fn.index("{"):].replace("// if (i == N - 1 || bRecInit) {", "")  # unused by the function
    assert re.search(r"optimizer\.optimize\(opt_it\);[^\n]*\n\s+float err_end = optimizer\.activeRobustChi2\(\);\s+if \(pbStopFlag\) optimizer\.setForceStopFlag", fn)
    assert parsed == {k: v for k, v in GOLDEN.items() if k != "source"}


def test_constants_in_the_rule():
    g, c = GOLDEN, S.constants()
    assert [c["max_window"], c["max_window_large"]] == g["max_opt"] and [c["opt_it"], c["opt_it_large"]] == g["opt_it"]
    assert [c["lambda_init"], c["lambda_init_large"]] == g["lambda_init"]
    assert c["huber_inertial"] == np.sqrt(g["huber_inertial_squared"]) and c["info_down_last"] == g["info_down_last"]
    assert c["huber_mono"] == float(np.float32(np.sqrt(g["huber_mono_squared"]))) and c["huber_stereo"] == float(np.float32(np.sqrt(g["huber_stereo_squared"])))
    assert c["chi2_mono2"] == float(np.float32(g["chi2_mono2"])) and c["chi2_stereo2"] == float(np.float32(g["chi2_stereo2"]))
    assert c["close_factor"] == g["chi2_close_factor"] and c["track_depth_close"] == g["track_depth_close"]
    assert (c["max_fix_kf"], c["max_cov_kf"], c["fail_gate_factor"], c["max_trials"]) == (g["max_fix_kf"], g["max_cov_kf"], g["fail_gate_factor"], g["max_trials"])
    assert (c["chunk"], c["lds_rows"]) == (S.CHUNK, S.LDS_ROWS) and c["max_trials"] == S.MAX_TRIALS
    rule = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "lba_inertial_rule.hpp")).read()
    # the comparisons of the classification loops and of the Levenberg fork, as the rule states them
    assert "return (chi2 > kChi2Mono2 && !close) || (chi2 > kCloseFactor * kChi2Mono2 && close) || !depth_positive;" in rule
    assert "return chi2 > kChi2Stereo2;" in rule and "GFS_HD double huber_inertial_lba() { return sqrt(16.0); }" in rule
    assert f"const double scale = scale_raw + {g['scale_guard']:g};".replace("0.001", "1e-3") in rule
    assert "if (rho > 0 && finite) {" in rule and "if (rho < 0 && c.qmax < kMaxTrials) return accepted;" in rule
    assert "if (c.qmax == kMaxTrials || rho == 0) {" in rule and "if ((c.ini_chi - c.current_chi) * 1e3 < c.ini_chi) c.n_bad++;" in rule
    assert f"if (c.n_bad >= {g['n_bad_stop']}) c.done = 1;" in rule
    adaptors = open(os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp")).read()
    assert "gfs_li::kFailGateFactor * err < err_end" in adaptors and "gfs_li::kMaxFixKF" in adaptors


def test_entry_points_are_declared_and_listed():
    from geoflowslam_amd import api
    head = open(os.path.join(ROOT, "include", "gfs_abi.h")).read()
    for name in ("gfs_lba_inertial_create", "gfs_lba_inertial_solve", "gfs_lba_inertial_destroy"):
        assert name + "(" in head and name in api.ABI_SYMBOLS
