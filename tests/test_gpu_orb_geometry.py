"""GPU tests (MI355X) of ORB extraction at edge geometries, quotas and handle reuse: the rows of tests/orb_geometry_support.py (one-cell
levels, nlevels = 1, the automatic host-quadtree fallback, portrait and 4 : 1 images, quotas of 0, 1 and 2), the lapping area at its
inclusive bounds, the batch entry with stride > cols, an unaligned device pointer, one handle across image sizes and the capacity rule.

Every comparison is bit equality with oracle.OrbOracle through _compare_full of tests/test_gpu_orb_match.py: pyramid planes, FAST
candidates, blurred planes, key-point fields, angle bits, descriptors and the mono index.  There is no tolerance anywhere.  The paths a
row claims are read from the handle (gfs_test_orb_last_paths) and from OrbGeometry::build (gfs_test_orb_geometry)."""
import ctypes as C

import numpy as np
import pytest

from geoflowslam_amd import synth

import orb_geometry_support as S
from test_gpu_gms import _Hip
from test_gpu_orb_match import _compare_full

pytestmark = pytest.mark.gpu


def _same(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def _compare_batch(ext, orc, imgs, results=None, lap=(0, 0)):
    """_compare_full for every frame of the batch the handle ran last (level(), candidates(), level(blurred=True) with b up to B - 1)."""
    out = []
    for b, im in enumerate(imgs):
        out.append(_compare_full(S.BatchFrame(ext, b, None if results is None else results[b]), orc, im, lap))
    return out


def _assert_paths(api, ext, c, B=1):
    p, g = ext.last_paths(), api.orb_geometry(c["h"], c["w"], c["nf"], c["nl"], S.SCALE)
    assert p["octree_on_device"] == (c["octree"] == "device") == bool(g["octree_on_device"]), f"row {c['key']}: quadtree path {p}"
    assert p["pyr_kernel"] == (api.ORB_PYR_NONE if c["nl"] == 1 else api.ORB_PYR_LDS), f"row {c['key']}: pyramid kernel {p}"
    assert p["pyr_fine_cut"] == int(c["nl"] > 1 and g["pyr_strips_fine"] > 0 and B * g["pyr_strips"] < 128), f"row {c['key']}: strip cut {p}"
    assert (p["last_batch"], p["rows"], p["cols"], p["geometry_builds"]) == (B, c["h"], c["w"], 1), f"row {c['key']}: {p}"
    return p, g


@pytest.mark.parametrize("key", [c["key"] for c in S.CASES])
def test_row_matches_the_oracle(gpu_api, oracle, key):
    """Cases a to g: every row on its noise image (and one row a group on the rendered scene), on a handle created for that size."""
    c = S.CASE[key]
    ext, orc = S.make_extractor(gpu_api, c), S.make_oracle(oracle, c)
    for rendered in (False, True) if c["rendered"] else (False,):
        _, k, _ = _compare_full(ext, orc, S.image(c, rendered=rendered))
        assert all(n >= 1 for n in S.level_counts(orc, c["nl"])), f"row {key}: a level without key points compares nothing"
    p, g = _assert_paths(gpu_api, ext, c)
    if c["group"] == "d":  # the per-level verdict of OrbGeometry::build is what sent (or did not send) the call to the host
        assert tuple(bool(L["octree_on_device"]) for L in g["levels"]) == c["device_levels"], f"row {key}: per-level verdict"
        assert p["octree_on_device"] == all(c["device_levels"]), f"row {key}: one level outside sends the whole call to the host"
    if "n_ini" in c:
        assert tuple(L["n_ini"] for L in g["levels"]) == c["n_ini"], f"row {key}: nIni"
    if "quotas" in c:
        assert tuple(ext.tables()["feats"]) == c["quotas"], f"row {key}: quotas"


@pytest.mark.parametrize("key", ["b68", "b67"])
def test_one_level_batches(gpu_api, oracle, key):
    """Case b: nlevels = 1 (no pyramid launch at all) as extract_batch of B = 1, 2, 3 and 9 frames.  With one cell a frame fast_map cuts
    the frame's cell list into 8 / B' parts of one cell, so all but one part of a frame are empty."""
    c = S.CASE[key]
    ext, orc = S.make_extractor(gpu_api, c, max_batch=9), S.make_oracle(oracle, c)
    pool = [S.image(c, i) for i in range(9)]
    single = [ext(im) for im in pool]
    for B in (1, 2, 3, 9):
        imgs = pool[9 - B:] if B < 9 else pool  # (another frame in front each time)
        res = ext.extract_batch(imgs)
        for b in range(B):
            assert _same(res[b], single[9 - B + b if B < 9 else b]), (key, B, b)
        _compare_batch(ext, orc, imgs, res)
        p = ext.last_paths()
        assert (p["pyr_kernel"], p["last_batch"], p["octree_on_device"]) == (gpu_api.ORB_PYR_NONE, B, 1), (key, B, p)


@pytest.mark.parametrize("octree", ["device", "host"])
def test_lapping_area_inclusive_bounds(gpu_api, oracle, monkeypatch, octree):
    """Case h: x >= lap0 && x <= lap1 with a key point exactly on each bound (k_kp_finalize on the device path, the host loop of
    run_batch on the host-quadtree path); the laps one integer off move that key point to the other block."""
    if octree == "host":
        monkeypatch.setenv("GFS_ORB_OCTREE", "host")
    L = S.LAP
    ext = gpu_api.ORBextractor(L["nf"], S.SCALE, L["nl"], S.INI_TH, S.MIN_TH, max_rows=L["h"], max_cols=L["w"])
    orc = oracle.OrbOracle(L["nf"], S.SCALE, L["nl"], S.INI_TH, S.MIN_TH)
    for rendered in (False, True):
        img = S.image(L, rendered=rendered)
        probes, _ = S.lap_probes(orc, img, L["nl"])
        for name, lap, others in probes:
            m, k, _ = _compare_full(ext, orc, img, lap)
            for o in others:
                mo, ko, _ = _compare_full(ext, orc, img, o)
                assert mo > m and len(ko) == len(k), f"case h, {name}: lap {lap} against {o}"
        m, k, _ = ext(img, probes[0][1])
        assert m == 0 and (rendered or len(k) == 506), "case h: every key point stereo"
        assert ext(img, probes[1][1])[0] == len(k), "case h: every key point mono"
    assert ext.last_paths()["octree_on_device"] == (octree == "device")


def test_batch_entry_with_stride_beyond_cols(gpu_api, oracle):
    """Case i: gfs_orb_extract_batch with stride > cols (the api wrapper always passes cols): 3 frames of 322 x 242, each a view into a
    340-wide buffer, give the bytes of their contiguous copies."""
    W, H, B, stride = 322, 242, 3, 340
    bufs = [synth.noise_image(S.SEED + 40 + b, stride, H + 5) for b in range(B)]
    views = [bufs[b][2 + b:2 + b + H, 5 + b:5 + b + W] for b in range(B)]
    assert all(v.strides == (stride, 1) and not v.flags["C_CONTIGUOUS"] for v in views)
    ext = gpu_api.ORBextractor(500, S.SCALE, 6, S.INI_TH, S.MIN_TH, max_rows=H, max_cols=W, max_batch=B)
    orc = oracle.OrbOracle(500, S.SCALE, 6, S.INI_TH, S.MIN_TH)
    copies = [np.ascontiguousarray(v) for v in views]
    want = ext.extract_batch(copies)
    ptrs = (C.c_void_p * B)(*[v.ctypes.data for v in views])
    kps, desc = np.zeros((B, ext.cap), gpu_api.KP_DTYPE), np.zeros((B, ext.cap, 32), np.uint8)
    n, mono = np.zeros(B, np.int32), np.zeros(B, np.int32)
    rc = gpu_api.lib().gfs_orb_extract_batch(ext.h, ptrs, B, H, W, stride, 0, 0, gpu_api._p(kps), gpu_api._p(desc), ext.cap, gpu_api._p(n),
                                             gpu_api._p(mono))
    assert rc == 0, gpu_api.lib().gfs_last_error()
    got = [(int(mono[b]), kps[b, :n[b]].copy(), desc[b, :n[b]].copy()) for b in range(B)]
    for b in range(B):
        assert _same(got[b], want[b]), f"case i: frame {b} differs from its contiguous copy"
    _compare_batch(ext, orc, copies, got)
    # stride < cols is refused, and the handle still answers
    assert gpu_api.lib().gfs_orb_extract_batch(ext.h, ptrs, B, H, W, W - 1, 0, 0, gpu_api._p(kps), gpu_api._p(desc), ext.cap, gpu_api._p(n),
                                               gpu_api._p(mono)) == -1
    assert _same(ext.extract_batch(copies)[1], want[1])


@pytest.mark.parametrize("W,H", [(640, 480), (320, 240)])
def test_device_pointer_not_word_aligned(gpu_api, oracle, W, H):
    """Case j: gfs_orb_extract_batch_device with the image at byte offsets 1, 2 and 3 into a device buffer while the pitch (cols) is a
    multiple of 4: k_fast_cells and k_blur7 pick byte staging from (pitch & 3) == 0 && (base & 3) == 0.  Against offset 0 and the oracle."""
    B = 2
    imgs = [synth.noise_image(S.SEED + 50 + b, W, H) for b in range(B)]
    ext = gpu_api.ORBextractor(1000, S.SCALE, 8, S.INI_TH, S.MIN_TH, max_rows=H, max_cols=W, max_batch=B)
    orc = oracle.OrbOracle(1000, S.SCALE, 8, S.INI_TH, S.MIN_TH)
    hip = _Hip()
    try:
        base = None
        for off in (0, 1, 2, 3):
            host = np.zeros(B * H * W + 4, np.uint8)
            host[off:off + B * H * W] = np.stack(imgs).ravel()
            dev = hip.to_device(host)
            assert dev % 4 == 0
            ext.extract_batch_device(dev + off, B, H, W)
            res = _compare_batch(ext, orc, imgs)
            if base is None:
                base = res
            for b in range(B):
                assert _same(res[b], base[b]), f"case j: offset {off}, frame {b} differs from offset 0"
    finally:
        hip.free()


def _refused(ext, img, code, words):
    p = ext.last_paths()
    with pytest.raises(Exception) as e:
        ext(img)
    assert getattr(e.value, "code", None) == code and words in str(e.value), str(e.value)
    assert ext.last_paths() == p, "a refused call leaves the handle as it was"


def test_one_handle_across_sizes(gpu_api, oracle):
    """Case k: ensure_geometry rewrites every table of a used handle when the image size changes; the bookkeeping behind the host view
    (cands_packed, host_counts_valid, host_cands_valid, last_B) follows; a refused size changes nothing."""
    ext = gpu_api.ORBextractor(1000, S.SCALE, 8, S.INI_TH, S.MIN_TH, max_rows=640, max_cols=640, max_batch=3)
    orc = oracle.OrbOracle(1000, S.SCALE, 8, S.INI_TH, S.MIN_TH)
    frames = lambda w, h, B, s: [synth.noise_image(S.SEED + s + b, w, h) for b in range(B)]
    builds = lambda: ext.last_paths()["geometry_builds"]
    hip = _Hip()
    try:
        # 1. 640 x 480, B = 3
        imgs = frames(640, 480, 3, 60)
        _compare_batch(ext, orc, imgs, ext.extract_batch(imgs))
        assert builds() == 1
        # 2. 241 x 241, B = 1; candidates() twice in a row (the second answer comes from the host view the first one left)
        imgs = frames(241, 241, 1, 63)
        res = ext.extract_batch(imgs)
        first, again = ext.candidates(7), ext.candidates(7)
        assert all((a == b).all() for a, b in zip(first, again)) and len(first[0]) == len(orc_candidates(orc, imgs[0], 7)[0])
        _compare_batch(ext, orc, imgs, res)
        assert builds() == 2
        # 3. 480 x 640 (portrait), B = 2, through the device entry: candidates() BEFORE fetch() -- nothing of the call is on the host yet
        imgs = frames(480, 640, 2, 64)
        dev = hip.to_device(np.stack(imgs))
        ext.extract_batch_device(dev, 2, 640, 480)
        x, y, s = ext.candidates(0, b=1)
        xo, yo, so = orc_candidates(orc, imgs[1], 0)
        assert (x == xo).all() and (y == yo).all() and (s == so).all(), "case k: candidates() before fetch()"
        _compare_batch(ext, orc, imgs)
        assert builds() == 3 and ext.last_paths()["last_batch"] == 2
        # 4. 577 x 433, B = 1
        img = synth.noise_image(S.SEED + 66, 577, 433)
        prev = _compare_full(ext, orc, img)
        assert builds() == 4
        # 5. 320 x 240 needs kp_cap 1068 > 1056 + 8: refused; the previous call repeats with its bytes and no rebuild
        _refused(ext, synth.noise_image(S.SEED, 320, 240), S.ERR_CAPACITY, "needs more workspace than the handle reserved")
        assert _same(ext(img), prev) and builds() == 4
        # 6. 640 x 150: level 7 is smaller than a cell
        _refused(ext, synth.noise_image(S.SEED, 640, 150), S.ERR_UNSUPPORTED, "smaller than one FAST cell")
        assert _same(ext(img), prev) and builds() == 4
        # 7. 577 x 433 again: no rebuild
        assert _same(_compare_full(ext, orc, img), prev) and builds() == 4
        # 8. 640 x 480, B = 1
        _compare_full(ext, orc, synth.noise_image(S.SEED + 60, 640, 480))
        assert builds() == 5
        # beyond max_rows x max_cols
        _refused(ext, synth.noise_image(S.SEED, 641, 480), S.ERR_CAPACITY, "exceeds the handle's max")
        assert builds() == 5
    finally:
        hip.free()


def orc_candidates(orc, img, level):
    orc.extract(img)
    return orc.candidates(level)


def test_capacity_rule(gpu_api, oracle):
    """Case l: the default 640 x 480 handle refuses 320 x 240 (kp_cap 1068) and 640 x 300 (1100) with GFS_ERR_CAPACITY -- it holds
    1056 + 8 -- and goes on extracting 640 x 480; a handle created at 320 x 240 takes that image."""
    orc = oracle.OrbOracle(1000, S.SCALE, 8, S.INI_TH, S.MIN_TH)
    ext = gpu_api.ORBextractor(1000, S.SCALE, 8, S.INI_TH, S.MIN_TH)
    assert ext.cap == S.KP_CAP[(640, 480)] + 8
    small, wide = synth.noise_image(S.SEED, 320, 240), synth.noise_image(S.SEED, 640, 300)
    _refused(ext, small, S.ERR_CAPACITY, "image 320x240 needs more workspace than the handle reserved")  # before the first image
    _compare_full(ext, orc, synth.noise_image(S.SEED, 640, 480))
    _refused(ext, small, S.ERR_CAPACITY, "image 320x240 needs more workspace than the handle reserved")
    _refused(ext, wide, S.ERR_CAPACITY, "image 640x300 needs more workspace than the handle reserved")
    _compare_full(ext, orc, synth.noise_image(S.SEED + 1, 640, 480))
    assert ext.last_paths()["geometry_builds"] == 1
    own = gpu_api.ORBextractor(1000, S.SCALE, 8, S.INI_TH, S.MIN_TH, max_rows=240, max_cols=320)
    assert own.cap == S.KP_CAP[(320, 240)] + 8
    _compare_full(own, orc, small)
