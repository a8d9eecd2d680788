"""Records tests/golden/lba_parent_digest.json on an MI355X: SHA-256 digests of everything Optimizer.LocalBundleAdjustment returns for
synth.lba_window(0, 20, 5, 3000) (tests/lba_parent_support.py).

The recording pins the bits of the PARENT of the commit that added the global bundle adjustment (gfs_gba_solve), which shares the
Levenberg-Marquardt kernels and the host preparation of gfs_lba_solve: it was run with geoflowslam_amd/libgfs_hip.so built from commit
8dc13f6 (`Deferred 10-NN passes: rows once, ranks by counting, covariances apart`).  Run it again only with a library whose local
bundle adjustment is meant to become the new reference, and change PARENT_COMMIT with it.

    python tools/record_lba_parent.py [--out tests/golden/lba_parent_digest.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PARENT_COMMIT = "8dc13f6"


def main():
    import lba_parent_support as S
    from geoflowslam_amd import api
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=S.FIXTURE)
    a = ap.parse_args()
    first, second = S.digests(api), S.digests(api)
    assert first == second, "two runs of the same library disagree: nothing to pin"
    with open(a.out, "w") as f:
        json.dump(dict(parent_commit=PARENT_COMMIT, window=S.WINDOW, sha256=first), f, indent=1, sort_keys=True)
        f.write("\n")
    print(a.out, json.dumps(first))


if __name__ == "__main__":
    main()
