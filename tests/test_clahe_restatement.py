"""The sequential CPU restatement of CLAHE (tests/host/clahe_restatement.cpp) against an independent numpy statement of DESIGN.md
section 16, bit for bit, look-up tables and image, on the case list x 8 seeds x both residual variants; first that the inputs
exercise the rule at all; then answers known in closed form, the committed fixture for the check against a real OpenCV, and the
restatement as a program of its own under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import clahe_support as CS

ROOT = CS.ROOT
_MAIN = os.path.join(ROOT, "tests", "host", "clahe_restatement_main.cpp")
_EXE = os.path.join(ROOT, "tests", "host", "_clahe_restatement_asan")
_GOLDEN = os.path.join(ROOT, "tests", "golden", "clahe_assumptions.npz")


@pytest.mark.parametrize("size", CS.SIZES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_numpy_statement(size):
    W, H = size
    for seed in CS.SEEDS:
        img = CS.image(W, H, seed)
        for variant in CS.VARIANTS:
            got, want = CS.restate(img, variant=variant), CS.numpy_statement(img, variant=variant)
            assert got[1].tobytes() == want[1].tobytes(), ("luts", size, seed, variant, int((got[1] != want[1]).sum()))
            assert got[0].tobytes() == want[0].tobytes(), ("image", size, seed, variant, int((got[0] != want[0]).sum()))


@pytest.mark.parametrize("kw", [dict(clip_limit=0.0), dict(tiles=(4, 2)), dict(tiles=(16, 16)), dict(clip_limit=40.0), dict(tiles=(1, 1))], ids=str)
def test_other_configurations_equal_numpy_statement(kw):
    for W, H in ((160, 120), (163, 117)):
        for variant in CS.VARIANTS:
            got, want = CS.restate(CS.image(W, H), variant=variant, **kw), CS.numpy_statement(CS.image(W, H), variant=variant, **kw)
            assert got[1].tobytes() == want[1].tobytes() and got[0].tobytes() == want[0].tobytes(), (W, H, variant)


def test_inputs_exercise_the_rule():
    """Every branch of the rule is taken by the case list, by the restatement's own diagnostics."""
    d = {}
    for size in CS.SIZES:
        for variant in CS.VARIANTS:
            d[size, variant] = CS.restate(CS.image(*size), variant=variant, diagnostics=True)
    for variant in CS.VARIANTS:
        for size in ((160, 120), (640, 480)):
            info = d[size, variant][2]["tile_info"]
            assert (info[:, 0] > 0).sum() == 64, (size, variant)                              # every tile is clipped
            assert (info[:, 1] >= 129).sum() >= 5, (size, variant, info[:, 1].tolist())       # step 1
            assert ((info[:, 1] >= 1) & (info[:, 1] <= 128)).sum() >= 5, (size, variant)      # step >= 2
            assert d[size, variant][2]["pix_tie"].sum() >= 100, (size, variant)               # res exactly k + 0.5
        for size in ((163, 117), (160, 117), (5, 3)):
            assert d[size, variant][2]["pix_tie"].sum() >= 1, (size, variant)
        assert (d[(8, 8), variant][2]["tile_info"] == 0).all()                                # tiles that clip nothing
        assert (d[(5, 3), variant][2]["tile_info"] == 0).all()
        # tile area 510: the table scale is exactly 0.5f and every odd prefix sum is a tie
        assert np.float32(255.0) / np.float32(510) == np.float32(0.5)
        assert d[(240, 136), variant][2]["lut_tie"].sum() >= 3000, variant
    for size in ((160, 120), (640, 480)):
        differ = (d[size, CS.STEPPED][0] != d[size, CS.CONTIGUOUS][0]).mean()
        assert differ >= 0.01, (size, differ)                                                 # the two variants are told apart
        assert (d[size, CS.STEPPED][1] != d[size, CS.CONTIGUOUS][1]).any()


def test_tiles_of_one_pixel():
    """8 x 8 with 8 x 8 tiles: area 1, scale 255, clip limit max(int(3 / 256), 1) = 1 and nothing to clip, so a tile's table is 0
    below its pixel's value and 255 from it on.  A pixel then blends, with weights 1/2 x 1/2, the tables of its own tile and of its
    left, upper and upper-left neighbours (its own again at the border) at its own value: 255 times the share of those four whose
    value is not above its own.  So an image that never decreases to the right or downwards gives all 255 -- not any image."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (8, 8), dtype=np.uint8)
    for variant in CS.VARIANTS:
        out, luts, diag = CS.restate(img, variant=variant, diagnostics=True)
        assert (diag["tile_info"] == 0).all()
        want_luts = np.where(np.arange(256)[None, None, :] >= img[:, :, None], 255, 0)
        assert np.array_equal(luts, want_luts)
        up, left = np.maximum(np.arange(8) - 1, 0), np.maximum(np.arange(8) - 1, 0)
        share = sum((img[np.ix_(a, b)] <= img).astype(np.int64) for a in (up, np.arange(8)) for b in (left, np.arange(8)))
        assert np.array_equal(out, np.array([0, 64, 128, 191, 255], np.uint8)[share])         # 63.75, 127.5 (to even), 191.25
        assert (share < 4).any()
        ramp = np.sort(np.sort(img, axis=1), axis=0)
        assert (CS.restate(ramp, variant=variant)[0] == 255).all()


def test_constant_image_stays_constant():
    """One bin holds the whole tile; clipped and redistributed or not, the prefix sum at that bin counts every bin up to it, and all
    tiles have the same table, so the blend returns one value everywhere."""
    for size in ((160, 120), (163, 117), (5, 3), (8, 8)):
        for value in (0, 77, 255):
            for variant in CS.VARIANTS:
                out, luts = CS.restate(np.full(size[::-1], value, np.uint8), variant=variant)
                assert (luts == luts[0, 0]).all() and (out == out[0, 0]).all(), (size, value, variant)
    assert (CS.restate(np.full((8, 8), 77, np.uint8))[0] == 255).all()
    assert (CS.restate(np.full((120, 160), 255, np.uint8))[0] == 255).all()                   # the last bin's prefix sum is the area


def test_clip_limit_zero_is_plain_tile_equalisation():
    img = CS.image(160, 120)
    out, luts = CS.restate(img, clip_limit=0.0)
    for j in range(8):
        for i in range(8):
            h = np.bincount(img[j * 15:(j + 1) * 15, i * 20:(i + 1) * 20].ravel(), minlength=256)
            want = np.rint(np.cumsum(h).astype(np.float32) * (np.float32(255.0) / np.float32(300)))
            assert np.array_equal(luts[j, i], want.astype(np.uint8)), (j, i)
    assert luts[:, :, 255].min() == 255
    for variant in CS.VARIANTS:
        assert CS.restate(img, clip_limit=0.0, variant=variant)[0].tobytes() == out.tobytes()
        assert CS.restate(img, clip_limit=-1.0, variant=variant)[0].tobytes() == out.tobytes()


def test_hand_built_tile():
    """One 16 x 16 tile (tiles 1 x 1): area 256, scale 255 / 256, clip limit int(3.0 * 256 / 256) = 3.  Bin 10 holds 200 pixels,
    bins 20 .. 75 one each (56): clipped = 197, batch 0, residual 197, step max(256 / 197, 1) = 1.  Both variants add 1 to bins
    0 .. 196.  Prefix sums: i + 1 up to bin 9; 14 at bin 10 (10 + 3 + 1); i + 4 up to bin 19; bins 20 .. 75 hold 2: 23 + 2 (i - 19);
    bins 76 .. 196 hold 1: 135 + (i - 75); 256, the area, from bin 196 on (what was clipped came back)."""
    img = np.full(256, 10, np.uint8)
    img[:56] = np.arange(20, 76)
    img = np.random.default_rng(1).permutation(img).reshape(16, 16)
    i = np.arange(256)
    sums = np.where(i < 10, i + 1, np.where(i < 20, i + 4, np.where(i < 76, 23 + 2 * (i - 19), np.where(i < 197, 135 + (i - 75), 256))))
    assert sums[10] == 14 and sums[19] == 23 and sums[20] == 25 and sums[75] == 135 and sums[196] == 256
    want = np.clip(np.rint(sums.astype(np.float32) * (np.float32(255.0) / np.float32(256))), 0, 255).astype(np.uint8)
    for variant in CS.VARIANTS:
        out, luts, diag = CS.restate(img, tiles=(1, 1), variant=variant, diagnostics=True)
        assert diag["tile_info"].tolist() == [[197, 197]]
        assert np.array_equal(luts[0, 0], want), variant
        assert np.array_equal(out, want[img])                                                  # one tile: no blend
    # residual 100: step 2 (stepped: bins 0, 2, .. 198) against bins 0 .. 99 (contiguous)
    img2 = np.full(256, 10, np.uint8)
    img2[:153] = np.arange(20, 173)
    img2 = img2.reshape(16, 16)
    h = np.bincount(img2.ravel(), minlength=256)
    assert h[10] == 103
    hs, hc = np.minimum(h, 3), np.minimum(h, 3)
    hs[0:200:2] += 1
    hc[:100] += 1
    for variant, hh in ((CS.STEPPED, hs), (CS.CONTIGUOUS, hc)):
        _, luts, diag = CS.restate(img2, tiles=(1, 1), variant=variant, diagnostics=True)
        assert diag["tile_info"].tolist() == [[100, 100]]
        assert np.array_equal(luts[0, 0], np.rint(np.cumsum(hh).astype(np.float32) * (np.float32(255.0) / np.float32(256))).astype(np.uint8))


def test_committed_fixture_for_the_opencv_check():
    """tests/golden/clahe_assumptions.npz (read by tests/golden/check_clahe_with_opencv.py where a real OpenCV exists) holds the
    case list's images up to 240 x 136 and what the restatement gives for both variants."""
    assert os.path.getsize(_GOLDEN) < 512 * 1024
    z = np.load(_GOLDEN)
    assert float(z["clip_limit"]) == 3.0 and z["tiles"].tolist() == [8, 8]
    for k, (W, H) in enumerate(CS.SMALL_SIZES):
        img = z[f"image_{k}"]
        assert img.shape == (H, W) and np.array_equal(img, CS.image(W, H))
        assert np.array_equal(z[f"stepped_{k}"], CS.restate(img, variant=CS.STEPPED)[0])
        assert np.array_equal(z[f"contiguous_{k}"], CS.restate(img, variant=CS.CONTIGUOUS)[0])
    script = open(os.path.join(ROOT, "tests", "golden", "check_clahe_with_opencv.py")).read()
    assert "geoflowslam" not in script and "import cv2" in script                              # stand-alone: numpy + cv2 only


def test_restatement_alone_under_sanitizers():
    """The restatement with its own main on 5 x 3, 163 x 117 and 160 x 117 (packed and padded rows, out of place and in place),
    built with -fsanitize=address,undefined and run as a program: it is never loaded into python.  The sanitizer runtimes are
    linked statically, so the program runs in whatever environment the suite was given."""
    deps = [_MAIN, os.path.join(ROOT, "tests", "host", "clahe_restatement.cpp"), os.path.abspath(__file__)]
    if not os.path.exists(_EXE) or os.path.getmtime(_EXE) < max(os.path.getmtime(d) for d in deps):
        tmp = _EXE + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-o", tmp, _MAIN], check=True)
        os.replace(tmp, _EXE)
    r = subprocess.run([_EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "clahe_restatement_main: ok" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-2000:])
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines() if line[:1].isdigit()]
    assert len(rows) == 12
    for W, H, variant, pad, total, lut_total in rows:
        y, x = np.mgrid[0:H, 0:W]
        img = (100 + (x * 7 + y * 13 + (x * y) % 5) % 40).astype(np.uint8)
        out, luts = CS.restate(img, variant=variant)
        assert (int(out.sum()), int(luts.sum())) == (total, lut_total), (W, H, variant, pad)
