"""gfs_lba_solve on the configs[4] window, as a digest: what tools/record_lba_parent.py records into tests/golden/lba_parent_digest.json
with the library of the commit before the global bundle adjustment, and what tests/test_gpu_gba.py compares the current library's
bits with."""
import hashlib
import json
import os

import numpy as np

from geoflowslam_amd import synth

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lba_parent_digest.json")
WINDOW = dict(seed=0, n_free=20, n_fixed=5, n_points=3000)
ARRAYS = ("pose_q", "pose_t", "points", "edge_chi2", "edge_depth_positive")
SCALARS = ("iterations_run", "final_chi2", "final_lambda")


def digests(api):
    """-> {name: sha256 of the bytes of every output of Optimizer.LocalBundleAdjustment on the window}"""
    w = synth.lba_window(**WINDOW)
    opt = api.Optimizer()
    r = opt.LocalBundleAdjustment(w)
    opt.close()
    out = {k: hashlib.sha256(np.ascontiguousarray(r[k]).tobytes()).hexdigest() for k in ARRAYS}
    out["scalars"] = hashlib.sha256(np.array([r[k] for k in SCALARS], np.float64).tobytes()).hexdigest()
    out["window"] = hashlib.sha256(b"".join(np.ascontiguousarray(w[k]).tobytes() for k in sorted(w) if isinstance(w[k], np.ndarray))).hexdigest()
    return out


def load():
    with open(FIXTURE) as f:
        return json.load(f)
