"""Records tests/golden/knn_far_rows_parent.npz on an MI355X: the clouds of tests/knn_far_rows_support.py as float32 and, for each of
them on the default path and under GFS_GICP_KNN_EXACT=1, the six covariance doubles a point that api.RegistrationGICP.preprocessed
returns, the three counts of gfs_gicp_knn_stats and the sorted bounds of the queries handed to k_knn_cov_far_wg.

The recording pins the deferred 10-NN passes of the PARENT of the commit that made k_knn_cov_far scan rows and rank its survivors by
counting, so it was run with geoflowslam_amd/libgfs_hip.so built from commit 4ff4b15 (`Voxel and cell sorts: one key box header,
shared top-level helpers`), before any kernel was touched.  The ragged batch and the streaming call behind it must give the single
calls' bits on that library too, which is asserted here and not stored.  Run it again only with a library whose covariances are meant
to become the new reference, and change PARENT_COMMIT with it.

    python tools/record_knn_far_rows_parent.py [--out tests/golden/knn_far_rows_parent.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PARENT_COMMIT = "4ff4b15"


def main():
    import knn_far_rows_support as S
    from geoflowslam_amd import api
    from test_gpu_gms import _Hip
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=S.FIXTURE)
    a = ap.parse_args()
    clouds = {n: S.cloud(n) for n in S.BATCH}
    for n, c in clouds.items():
        assert len(c) <= S.MAX_POINTS and (c[:, 3] == 1).all(), n
    hip = _Hip()
    runs = S.run_all(api, clouds, hip)
    hip.free()
    arrays = {"cloud/" + n: np.ascontiguousarray(c[:, :3]) for n, c in clouds.items()}
    for path, run in runs.items():
        for n, e in run["single"].items():
            arrays["cov/%s/%s" % (path, n)], arrays["stats/%s/%s" % (path, n)], arrays["dnext/%s/%s" % (path, n)] = e["cov"], e["stats"], e["dnext"]
            print(f"{path:<8}{n:<12} stats {e['stats']} dnext {e['dnext'][:4]}")
        for what, msg in S.batch_differences(run):
            raise SystemExit("the parent's batch differs from its single calls: %s %s %s" % (path, what, msg))
    np.savez_compressed(a.out, parent_commit=np.array(PARENT_COMMIT), **arrays)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
