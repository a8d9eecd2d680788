"""Shared by the CLAHE tests: builds and calls the sequential CPU restatement (tests/host/clahe_restatement.cpp), an independent
numpy statement of the rule, the case list and the images.  Not a test module."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from geoflowslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "clahe_restatement.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_clahe_restatement.so")
_L = None

STEPPED, CONTIGUOUS = 0, 1
VARIANTS = (STEPPED, CONTIGUOUS)
# (width, height): divides evenly (tile 20 x 15, clip limit 3); tile area 510 so that the table scale is exactly 0.5f and every
# odd prefix sum is a rounding tie; extended in both directions; the width divides and is extended by a whole 8 columns;
# tile 1 x 1; an extension longer than the image; VGA
SIZES = ((160, 120), (240, 136), (163, 117), (160, 117), (8, 8), (5, 3), (640, 480))
SMALL_SIZES = SIZES[:-1]
SEEDS = tuple(range(8))


def restatement():
    global _L
    if _L is None:
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < os.path.getmtime(_SRC):
            tmp = _SO + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", tmp, _SRC], check=True)
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        vp, i = C.c_void_p, C.c_int
        L.cr_clahe.argtypes = [vp, i, i, i, C.c_double, i, i, i, vp, i, vp, vp, vp, vp]
        L.cr_clahe.restype = C.c_int
        _L = L
    return _L


def restate(img, clip_limit=3.0, tiles=(8, 8), variant=STEPPED, diagnostics=False):
    """The restatement on one [H, W] u8 image -> (equalised [H, W] u8, luts [ty, tx, 256] u8) and, when asked, a dict of
    tile_info [tiles, 2] (clipped, residual), lut_tie [ty, tx, 256] and pix_tie [H, W]."""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape
    tx, ty = tiles
    out, luts = np.zeros_like(img), np.zeros((ty, tx, 256), np.uint8)
    info, lt, pt = np.zeros((tx * ty, 2), np.int32), np.zeros((ty, tx, 256), np.uint8), np.zeros((H, W), np.uint8)
    p = lambda a: a.ctypes.data if diagnostics else None
    rc = restatement().cr_clahe(img.ctypes.data, W, H, W, float(clip_limit), tx, ty, variant, out.ctypes.data, W, luts.ctypes.data,
                                p(info), p(lt), p(pt))
    assert rc == 0, rc
    return (out, luts, dict(tile_info=info, lut_tie=lt, pix_tie=pt)) if diagnostics else (out, luts)


def _reflect_index(n_ext, n):
    """BORDER_REFLECT_101 source index of 0 .. n_ext - 1 in closed form: the index runs up and down with period 2 (n - 1)."""
    if n == 1:
        return np.zeros(n_ext, np.int64)
    m = np.arange(n_ext) % (2 * (n - 1))
    return np.where(m < n, m, 2 * (n - 1) - m)


def numpy_statement(img, clip_limit=3.0, tiles=(8, 8), variant=STEPPED):
    """DESIGN.md section 16 in numpy, whole arrays at a time: np.bincount per tile, np.cumsum, np.rint (ties to even), the blend in
    float32 arrays one operation at a time.  -> (equalised, luts)."""
    f = np.float32
    img = np.asarray(img, np.uint8)
    H, W = img.shape
    tx, ty = tiles
    if W % tx == 0 and H % ty == 0:
        ext = img
    else:
        ext = img[_reflect_index(H + ty - H % ty, H)][:, _reflect_index(W + tx - W % tx, W)]
    tw, th = ext.shape[1] // tx, ext.shape[0] // ty
    area = tw * th
    scale = f(255.0) / f(area)
    clip = max(int(clip_limit * area / 256), 1) if clip_limit > 0 else 0
    luts = np.zeros((ty, tx, 256), np.uint8)
    for j in range(ty):
        for i in range(tx):
            h = np.bincount(ext[j * th:(j + 1) * th, i * tw:(i + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if clip > 0:
                clipped = int(np.maximum(h - clip, 0).sum())
                h = np.minimum(h, clip) + clipped // 256
                residual = clipped % 256
                if residual:
                    if variant == STEPPED:
                        h[np.arange(residual) * max(256 // residual, 1)] += 1
                    else:
                        h[:residual] += 1
            luts[j, i] = np.clip(np.rint(np.cumsum(h).astype(f) * scale), 0, 255).astype(np.uint8)

    def axis(n, t, nt):
        tf = np.arange(n).astype(f) * (f(1.0) / f(t)) - f(0.5)
        t1 = np.floor(tf)
        a = tf - t1
        t1 = t1.astype(np.int64)
        return np.maximum(t1, 0), np.minimum(t1 + 1, nt - 1), a.astype(f), (f(1.0) - a).astype(f)

    x1, x2, xa, xa1 = axis(W, tw, tx)
    y1, y2, ya, ya1 = axis(H, th, ty)
    L = luts.astype(f)
    g = lambda jy, ix: L[jy[:, None], ix[None, :], img]
    top = g(y1, x1) * xa1[None, :] + g(y1, x2) * xa[None, :]
    bot = g(y2, x1) * xa1[None, :] + g(y2, x2) * xa[None, :]
    res = top * ya1[:, None] + bot * ya[:, None]
    assert res.dtype == f
    return np.clip(np.rint(res), 0, 255).astype(np.uint8), luts


@functools.lru_cache(maxsize=None)
def image(width, height, seed=0):
    im = synth.clahe_image(seed, width, height)
    im.setflags(write=False)
    return im


@functools.lru_cache(maxsize=None)
def expected(width, height, seed=0, clip_limit=3.0, tiles=(8, 8), variant=STEPPED):
    """The restatement's (equalised, luts) of image(width, height, seed), computed once and shared; read-only."""
    out, luts = restate(image(width, height, seed), clip_limit, tiles, variant)
    out.setflags(write=False)
    luts.setflags(write=False)
    return out, luts
