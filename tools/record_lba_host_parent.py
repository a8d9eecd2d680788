"""Records tests/golden/lba_host_parent_digest.json on an MI355X: SHA-256 digests of what every host path of the local, lidar, batched
and global bundle adjustment returns for the cases of tests/lba_host_parent_support.py.

The recording pins the bits, the stop counters and gfs_gba_last_info of the PARENT of the commit that restated the host code of
lba.hip once (one LM phase queue for the local and the global loop): it was run with geoflowslam_amd/libgfs_hip.so built from commit
e9c8145 (`k_bf_hamming: Hamming distances as an i8 product on the matrix cores`).  Every case is run twice and nothing is written
unless both runs agree.  Run it again only with a library whose bundle adjustments are meant to become the new reference, and change
PARENT_COMMIT with it.

    python tools/record_lba_host_parent.py [--out tests/golden/lba_host_parent_digest.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PARENT_COMMIT = "e9c8145"


def main():
    import lba_host_parent_support as S
    from geoflowslam_amd import api
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=S.FIXTURE)
    a = ap.parse_args()
    first, second = S.digests(api), S.digests(api)
    differ = sorted(k for k in set(first) | set(second) if first.get(k) != second.get(k))
    assert not differ, f"two runs of the same library disagree, nothing to pin: {differ}"
    with open(a.out, "w") as f:
        json.dump(dict(parent_commit=PARENT_COMMIT, sha256=first), f, indent=1, sort_keys=True)
        f.write("\n")
    print(a.out, len(first), "cases")


if __name__ == "__main__":
    main()
