"""Writes tests/golden/clahe_assumptions.npz: the CLAHE case list's images up to 240 x 136 and the outputs of the sequential
restatement (tests/host/clahe_restatement.cpp) for both residual variants.  Run from the repository root:
    python tests/golden/make_clahe_assumptions.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import clahe_support as CS  # noqa: E402

arrays = dict(clip_limit=np.float64(3.0), tiles=np.array([8, 8], np.int32))
for k, (W, H) in enumerate(CS.SMALL_SIZES):
    img = CS.image(W, H)
    arrays[f"image_{k}"] = img
    arrays[f"stepped_{k}"] = CS.restate(img, variant=CS.STEPPED)[0]
    arrays[f"contiguous_{k}"] = CS.restate(img, variant=CS.CONTIGUOUS)[0]
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "clahe_assumptions.npz"), **arrays)
