"""Checks the written CLAHE rule against a real OpenCV.  Stand-alone: numpy and cv2 only.
    python tests/golden/check_clahe_with_opencv.py
clahe_assumptions.npz (next to this file) holds images and, for each, what the rule gives with the stepped residual
(OpenCV >= 3.4) and with the contiguous residual (OpenCV <= 3.3).  cv2.createCLAHE(3.0, (8, 8)).apply must reproduce one of the two
on every image; the script prints PASS / FAIL per variant and names the gfs_clahe_config.residual_variant to use."""
import os
import sys

import cv2
import numpy as np

z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "clahe_assumptions.npz"))
tiles = tuple(int(v) for v in z["tiles"])
clahe = cv2.createCLAHE(clipLimit=float(z["clip_limit"]), tileGridSize=tiles)
n = sum(1 for k in z.files if k.startswith("image_"))
ok = {"stepped": True, "contiguous": True}
for k in range(n):
    img = z[f"image_{k}"]
    got = clahe.apply(np.ascontiguousarray(img))
    for name in ok:
        bad = int((got != z[f"{name}_{k}"]).sum())
        ok[name] &= bad == 0
        print(f"image {k} {img.shape[1]}x{img.shape[0]} {name}: {bad} of {img.size} bytes differ")
print("OpenCV", cv2.__version__)
for i, name in enumerate(ok):
    print(("PASS" if ok[name] else "FAIL"), f"{name} (residual_variant = {i})")
match = [name for name in ok if ok[name]]
if len(match) == 2:
    print("both variants match: these images do not tell them apart")
print("this OpenCV follows:", match[0] if len(match) == 1 else ("neither variant: the written rule is wrong somewhere" if not match else "either"))
sys.exit(0 if match else 1)
