"""gfs_glibc::exp (geoflowslam_amd/csrc/glibc_math.hpp: glibc 2.35's exp restated, used by k_sim3_opt for the scale of a
VertexSim3Expmap update, Thirdparty/g2o/g2o/types/sim3.h:82) compiled for the HOST and compared bit for bit with this machine's libm
-- the library the CPU restatement (and the reference) calls."""
import os
import platform
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _glibc_with_fma():
    if platform.machine() != "x86_64" or platform.libc_ver()[0] != "glibc":
        return False
    try:
        return "fma" in open("/proc/cpuinfo").read().split("flags", 1)[1].split("\n", 1)[0].split()
    except Exception:
        return False


@pytest.mark.skipif(not _glibc_with_fma(), reason="needs an x86-64 glibc host with FMA (the libm the restatement calls)")
def test_restated_exp_equals_the_host_libm(tmp_path):
    exe = tmp_path / "glibc_exp_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", os.path.join(ROOT, "tests", "host", "glibc_exp_check.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe), "5000000"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("exp 0 of 5000000")
