"""The host paths of the bundle adjustments against the parent's bits (MI355X): tests/golden/lba_host_parent_digest.json holds SHA-256
digests recorded with the library of commit e9c8145 (tools/record_lba_host_parent.py) for every case of
tests/lba_host_parent_support.py -- the local windows unstopped and stopped at every look, the runs without an LM loop, the lidar
windows, the batch closed at every round, the global solves with their gfs_gba_last_info, mode 1 and the two first-trial hooks.  The
current library recomputes them.  A digest matches or it does not: a mismatch is a defect in the library, never a reason to record again."""
import pytest

import lba_host_parent_support as HP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def got(gpu_api):
    return HP.digests(gpu_api)


def test_the_inputs_are_the_recorded_ones(got):
    rec = HP.load()
    assert rec["parent_commit"] == "e9c8145"
    assert got["inputs"] == rec["sha256"]["inputs"], "the windows and maps are not the recorded ones"


def test_every_case_has_the_parents_bits(got):
    want = HP.load()["sha256"]
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    assert all(any(k.startswith(p) for k in want) for p in ("local/", "lidar/", "batch@", "global/", "linearize", "first-trial/"))
    differ = sorted(k for k in want if got[k] != want[k])
    assert not differ, differ
