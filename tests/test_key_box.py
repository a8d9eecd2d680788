"""The key box of the voxel and cell sorts (geoflowslam_amd/csrc/key_box.hpp) on the host: tests/host/key_box_check.cpp packs and
unpacks seeded random boxes in both field layouts (voxel keys 21 / 42, cell sort keys 25 / 45) and checks the round trip, that packing
keeps the order of valid keys and the invalid key on top, that every width is the smallest b >= 1 with range < 2^b (ranges 0, 2^b - 1
and 2^b among them), the 31- and 32-bit limits of the 4-byte sorts, and the kinfo slots."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_key_box_packs_in_order_and_round_trips(tmp_path):
    exe = tmp_path / "key_box_check"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", ROOT,
                           os.path.join(ROOT, "tests", "host", "key_box_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok: "), out.stdout + out.stderr
