"""computeLambdaInit's maximum over the diagonal (geoflowslam_amd/csrc/lm_lambda_rule.hpp, what lm_lambda_init of k_pose_opt and
k_pl_round calls) on the host: tests/host/lm_lambda_rule_check.cpp holds it to std::max(fabs(h), maxDiagonal) taken in order, as g2o
writes it -- finite diagonals with the maximum at every place, and a NaN first, in the middle, last, twice and everywhere (a NaN is
kept only when it is the last entry; fmax would drop it everywhere)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_max_abs_diagonal_follows_std_max_with_nan(tmp_path):
    exe = tmp_path / "lm_lambda_rule_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", ROOT,
                           os.path.join(ROOT, "tests", "host", "lm_lambda_rule_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok: "), out.stdout + out.stderr
