"""gfs_glibc::logf (geoflowslam_amd/csrc/glibc_math.hpp: glibc 2.35's flt-32/e_logf.c restated, used by the frustum kernel for
MapPoint::PredictScale, reference src/MapPoint.cc:565-579) compiled for the HOST and compared bit for bit with this machine's
libm on EVERY positive finite float and the special values; the committed table must be what tools/extract_glibc_tables.py
reads out of that libm."""
import os
import platform
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

needs_glibc = pytest.mark.skipif(platform.machine() != "x86_64" or platform.libc_ver()[0] != "glibc",
                                 reason="needs an x86-64 glibc host (the libm the restatement calls)")


@needs_glibc
def test_restated_logf_equals_the_host_libm_on_every_positive_float(tmp_path):
    exe = tmp_path / "glibc_logf_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-pthread",
                           os.path.join(ROOT, "tests", "host", "glibc_logf_check.cpp"), "-o", str(exe)])
    threads = max(1, min(16, len(os.sched_getaffinity(0))))
    out = subprocess.run([str(exe), str(threads)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    # 0x7f7fffff positive finite floats + the 10 special values (0, -0, +-inf, NaN, negatives, 1, 1.2f)
    assert out.stdout.strip().endswith("logf 0 of %d" % (0x7f7fffff + 10)), out.stdout


@needs_glibc
def test_regenerated_tables_equal_the_committed_ones(tmp_path):
    if platform.libc_ver()[1] != "2.35":
        pytest.skip("tables were read from glibc 2.35")
    inc = os.path.join(ROOT, "geoflowslam_amd", "csrc", "glibc_tables.inc")
    fresh = tmp_path / "glibc_tables.inc"  # (never the tracked file: touching it would make every object of the library stale)
    subprocess.check_call(["python3", os.path.join(ROOT, "tools", "extract_glibc_tables.py"), "--out", str(fresh)], stdout=subprocess.DEVNULL)
    text = open(inc).read()
    assert open(fresh).read() == text
    assert "GFS_GLIBC_LOGF_TAB" in text and "GFS_GLIBC_LOGF_HDR" in text
