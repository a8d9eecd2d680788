"""Records tests/golden/knn_cov_parent.npz on an MI355X: the clouds of tests/knn_cov_parent_support.py as float32 and the six
covariance doubles a point that api.RegistrationGICP.preprocessed returns for them, on the default path and under
GFS_GICP_KNN_EXACT=1, single calls and one ragged batch.

The recording pins the bits of the PARENT of the commit that moved the closed-form eigen-decomposition into csrc/eig3_direct.hpp, so
it was run with geoflowslam_amd/libgfs_hip.so built from commit 9651a99 (`k_knn_cov: walk every row outwards from the query's x, rows
in one loop`), where gicp.hip still indexed its private arrays by i0, k and l.  Run it again only with a library whose covariances
are meant to become the new reference, and change PARENT_COMMIT with it.

    python tools/record_knn_cov_parent.py [--out tests/golden/knn_cov_parent.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PARENT_COMMIT = "9651a99"


def main():
    import knn_cov_parent_support as S
    from geoflowslam_amd import api
    from test_gpu_gms import _Hip
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=S.FIXTURE)
    a = ap.parse_args()
    clouds = {n: S.cloud(n) for n in S.NAMES}
    for n, c in clouds.items():
        assert len(c) <= S.MAX_POINTS and (c[:, 3] == 1).all(), n
    hip = _Hip()
    runs = S.run_all(api, clouds, hip)
    hip.free()
    arrays, same, seen = {"cloud/" + n: np.ascontiguousarray(c[:, :3]) for n, c in clouds.items()}, [], {}
    for (path, key), cov in runs.items():
        k = "cov/%s/%s" % (path, key)
        b = cov.tobytes()
        if b in seen:  # the same bytes as an earlier recording: stored once
            same.append("%s=%s" % (k, seen[b]))
        else:
            seen[b] = k
            arrays[k] = cov
        print(f"{k:<34} {len(cov):>5} points" + (f"  = {seen[b]}" if seen[b] != k else ""))
    np.savez_compressed(a.out, parent_commit=np.array(PARENT_COMMIT), same_as=np.array(same), **arrays)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, {len(arrays)} arrays, {len(same)} stored as another's")


if __name__ == "__main__":
    main()
