"""The staging-block layouts (geoflowslam_amd/csrc/staging.hpp, block_layouts.hpp) on the host: tests/host/staging_layout_check.cpp
compares every field offset and block size with the closed-form sums the handles used to compute by hand, at sizes that are no
multiple of the alignment (batches of 1 and 3; counts 0, 1, 63, 64, 65), and checks order, overlap, alignment and zero-count fields."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layouts_equal_the_hand_written_offsets(tmp_path):
    exe = tmp_path / "staging_layout_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", ROOT,
                           os.path.join(ROOT, "tests", "host", "staging_layout_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok: "), out.stdout + out.stderr
