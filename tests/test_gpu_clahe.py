"""GPU parity tests for CLAHE (MI355X; k_clahe_lut / k_clahe_interp through the C ABI): equalised bytes and look-up-table bytes
equal the sequential restatement (tests/host/clahe_restatement.cpp) with no tolerance -- histograms are
integer counts and the float blend has one fixed order -- and the pyramid built behind it equals the plain build fed the
restatement's image."""
import ctypes as C

import numpy as np
import pytest

import clahe_support as CS
from geoflowslam_amd import synth

pytestmark = pytest.mark.gpu

INVALID_ARG, CAPACITY = -1, -4


@pytest.fixture(scope="module")
def hip():
    from test_gpu_gms import _Hip
    h = _Hip()
    yield h
    h.free()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), [(tuple(int(v) for v in i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:4]])


@pytest.mark.parametrize("variant", CS.VARIANTS)
@pytest.mark.parametrize("size", CS.SIZES, ids=lambda s: "%dx%d" % s)
def test_case_list_equals_restatement(gpu_api, size, variant):
    W, H = size
    cl = gpu_api.Clahe(W, H, residual_variant=variant)
    want, want_luts = CS.expected(W, H, variant=variant)
    got = cl.apply(CS.image(W, H))
    _same(cl.luts(), want_luts, "luts")
    _same(got, want, "image")


@pytest.mark.parametrize("kw", [dict(clip_limit=0.0), dict(tiles=(4, 2)), dict(tiles=(16, 16))], ids=str)
@pytest.mark.parametrize("variant", CS.VARIANTS)
def test_clip_limit_and_tile_grids(gpu_api, kw, variant):
    W, H = 160, 120
    cl = gpu_api.Clahe(W, H, residual_variant=variant, **kw)
    want, want_luts = CS.expected(W, H, variant=variant, **kw)
    got = cl.apply(CS.image(W, H))
    _same(cl.luts(), want_luts, "luts")
    _same(got, want, "image")


@pytest.mark.parametrize("size", [(160, 120), (163, 117)], ids=lambda s: "%dx%d" % s)
def test_batch_stride_in_place_and_repeat(gpu_api, size):
    W, H = size
    imgs = [CS.image(W, H, seed) for seed in (0, 1, 2)]
    want = [CS.expected(W, H, seed) for seed in (0, 1, 2)]
    cl = gpu_api.Clahe(W, H, max_batch=3)
    plain = [cl.apply(im) for im in imgs]
    for f in range(3):
        _same(plain[f], want[f][0], ("plain", f))
    got = cl.apply(imgs)                                     # B = 3 distinct images in one call
    for f in range(3):
        _same(got[f], plain[f], ("batch", f))
        _same(cl.luts(f), want[f][1], ("batch luts", f))
    again = cl.apply(imgs)                                   # the same call twice
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    big = np.full((3, H, W + 13), 201, np.uint8)             # stride = width + 13, in and out
    big[:, :, :W] = imgs
    out = np.full((3, H, W + 13), 77, np.uint8)
    cl.apply([b[:, :W] for b in big], out=[o[:, :W] for o in out])
    for f in range(3):
        _same(out[f, :, :W], plain[f], ("stride", f))
    assert (out[:, :, W:] == 77).all()                       # the padding is not written
    views = [b[:, :W] for b in big]
    cl.apply(views, out=views)                               # in place
    for f in range(3):
        _same(big[f, :, :W], plain[f], ("in place", f))
    assert (big[:, :, W:] == 201).all()


def test_device_form_in_place_and_strided(gpu_api, hip):
    W, H, S = 163, 117, 163 + 13
    imgs = np.full((3, H, S), 9, np.uint8)
    imgs[:, :, :W] = [CS.image(W, H, seed) for seed in (0, 1, 2)]
    cl = gpu_api.Clahe(W, H, max_batch=3)
    d_in, d_out = hip.to_device(imgs), hip.to_device(np.zeros((3, H, W), np.uint8))
    cl.apply_device(d_in, W, H, S, 3, d_out, W)
    out = hip.to_host(d_out, (3, H, W), np.uint8)
    for f in range(3):
        _same(out[f], CS.expected(W, H, f)[0], ("device", f))
    st = hip.stream()
    cl.apply_device(d_in, W, H, S, 3, d_in, S, stream=st)    # in place, on the caller's stream
    back = hip.to_host(d_in, (3, H, S), np.uint8)
    _same(back[:, :, :W], out, "device in place")
    assert (back[:, :, W:] == 9).all()


@pytest.fixture(scope="module")
def pair():
    out = {}
    for W, H in ((160, 120), (163, 117)):
        i0, i1, flow = synth.klt_texture_pair(11, W, H, shift=(2.3, -1.4))
        # the texture squeezed into a narrow range, as a dim frame: CLAHE has something to do
        i0, i1 = (np.rint(100.0 + 0.25 * im.astype(np.float64)).clip(0, 255).astype(np.uint8) for im in (i0, i1))
        kps = np.stack(np.meshgrid(np.linspace(8, W - 9, 12), np.linspace(8, H - 9, 9)), -1).reshape(-1, 2).astype(np.float32)
        out[(W, H)] = (i0, i1, kps, CS.restate(i0)[0], CS.restate(i1)[0])
    return out


@pytest.mark.parametrize("size", [(160, 120), (163, 117)], ids=lambda s: "%dx%d" % s)
def test_pyramid_behind_clahe_equals_plain_build_of_restated_image(gpu_api, pair, size):
    W, H = size
    i0, i1, kps, e0, e1 = pair[size]
    assert (e0 != i0).mean() > 0.5
    trk = gpu_api.KltTracker(W, H, 21, max_batch=1, max_points=256)
    cl = gpu_api.Clahe(W, H)
    before = trk.buildOpticalFlowPyramid(i0).download()
    p0, q0 = trk.buildOpticalFlowPyramid(i0, clahe=cl, return_equalized=True)
    p1, q1 = trk.buildOpticalFlowPyramid(i1, clahe=cl, return_equalized=True)
    _same(q0, e0, "equalized_out 0")
    _same(q1, e1, "equalized_out 1")
    r0, r1 = trk.buildOpticalFlowPyramid(e0), trk.buildOpticalFlowPyramid(e1)
    for got, want in ((p0, r0), (p1, r1)):
        (gi, gd), (wi, wd) = got.download(), want.download()
        _same(gi, wi, "pyramid images")
        _same(gd, wd, "pyramid derivatives")
    a = trk.fbKltTracking(p0, p1, 3, 15.0, 0.5, kps, kps.copy())
    b = trk.fbKltTracking(r0, r1, 3, 15.0, 0.5, kps, kps.copy())
    assert a[2] == b[2] > 0 and np.array_equal(a[1], b[1]) and a[0].tobytes() == b[0].tobytes()
    # nothing existing moved: the tracker's plain build after a CLAHE build on the same handle
    after = trk.buildOpticalFlowPyramid(i0).download()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()


def test_device_pyramid_entry_with_and_without_destination(gpu_api, hip, pair):
    W, H = 163, 117
    i0, i1, _, e0, e1 = pair[(W, H)]
    S = W + 3
    src = np.zeros((2, H, S), np.uint8)
    src[:, :, :W] = [i0, i1]
    trk = gpu_api.KltTracker(W, H, 21, max_batch=2, max_points=16)
    cl = gpu_api.Clahe(W, H, max_batch=2)
    want = trk.buildOpticalFlowPyramid([e0, e1])
    wants = [want.download(f) for f in (0, 1)]
    d_src, d_eq = hip.to_device(src), hip.to_device(np.zeros((2, H, W + 5), np.uint8))
    pyr = gpu_api.KltPyramid(trk)
    trk.build_pyramid_clahe_device(cl, d_src, S, 2, pyr)     # dev_equalized = NULL: the image lives in the handle's scratch
    for f in (0, 1):
        gi, gd = pyr.download(f)
        _same(gi, wants[f][0], ("scratch images", f))
        _same(gd, wants[f][1], ("scratch derivatives", f))
    pyr2 = gpu_api.KltPyramid(trk)
    trk.build_pyramid_clahe_device(cl, d_src, S, 2, pyr2, d_equalized=d_eq, eq_stride=W + 5)
    eq = hip.to_host(d_eq, (2, H, W + 5), np.uint8)
    _same(eq[0, :, :W], e0, "dev_equalized 0")
    _same(eq[1, :, :W], e1, "dev_equalized 1")
    for f in (0, 1):
        _same(pyr2.download(f)[0], wants[f][0], ("given images", f))
    _same(hip.to_host(d_src, (2, H, S), np.uint8), src, "the source is left alone")


def test_refusals_leave_the_handle_usable(gpu_api, hip):
    A, L = gpu_api, gpu_api.lib()
    W, H = 160, 120
    img, (want, want_luts) = CS.image(W, H), CS.expected(W, H)
    cl = A.Clahe(W, H, max_batch=2)

    def still_fine():
        _same(cl.apply(img), want, "after a refusal")
        _same(cl.luts(), want_luts, "after a refusal")

    still_fine()
    out = np.empty_like(img)
    ip, op, null = (C.c_void_p * 1)(img.ctypes.data), (C.c_void_p * 1)(out.ctypes.data), (C.c_void_p * 1)(None)
    d_img = hip.to_device(img)
    ip3, op3 = (C.c_void_p * 3)(*[img.ctypes.data] * 3), (C.c_void_p * 3)(*[out.ctypes.data] * 3)
    calls = [
        (INVALID_ARG, lambda: L.gfs_clahe_apply(None, ip, W, H, W, 1, op, W)),
        (INVALID_ARG, lambda: L.gfs_clahe_apply(cl.h, None, W, H, W, 1, op, W)),
        (INVALID_ARG, lambda: L.gfs_clahe_apply(cl.h, ip, W, H, W, 1, None, W)),
        (INVALID_ARG, lambda: L.gfs_clahe_apply(cl.h, null, W, H, W, 1, op, W)),
        (INVALID_ARG, lambda: L.gfs_clahe_apply(cl.h, ip, W, H, W, 1, null, W)),
        (INVALID_ARG, lambda: L.gfs_clahe_apply(cl.h, ip, W, H, W - 1, 1, op, W)),
        (INVALID_ARG, lambda: L.gfs_clahe_apply(cl.h, ip, W, H, W, 1, op, W - 1)),
        (INVALID_ARG, lambda: L.gfs_clahe_apply(cl.h, ip, 0, H, W, 1, op, W)),
        (INVALID_ARG, lambda: L.gfs_clahe_apply(cl.h, ip, W, H, W, 0, op, W)),
        (CAPACITY, lambda: L.gfs_clahe_apply(cl.h, ip3, W, H, W, 3, op3, W)),
        (CAPACITY, lambda: L.gfs_clahe_apply(cl.h, ip, W + 1, H, W + 1, 1, op, W + 1)),
        (CAPACITY, lambda: L.gfs_clahe_apply(cl.h, ip, W, H + 1, W, 1, op, W)),
        (INVALID_ARG, lambda: L.gfs_clahe_apply_device(cl.h, None, W, H, W, 1, d_img, W, None)),
        (INVALID_ARG, lambda: L.gfs_clahe_apply_device(cl.h, d_img, W, H, W, 1, None, W, None)),
        (INVALID_ARG, lambda: L.gfs_clahe_apply_device(cl.h, d_img, W, H, W - 1, 1, d_img, W - 1, None)),
        (INVALID_ARG, lambda: L.gfs_clahe_apply_device(cl.h, d_img, W, H, W, 1, d_img, W + 4, None)),  # in place, other stride
        (CAPACITY, lambda: L.gfs_clahe_apply_device(cl.h, d_img, W, H, W, 3, d_img, W, None)),
        (INVALID_ARG, lambda: L.gfs_clahe_download_luts(cl.h, 0, None)),
        (INVALID_ARG, lambda: L.gfs_clahe_download_luts(cl.h, 1, out.ctypes.data)),  # the last call had one frame
    ]
    for k, (code, call) in enumerate(calls):
        assert call() == code, k
        still_fine()
    # creation: tiles out of range, unknown variant, image too large, NULL
    for kw, code in ((dict(tiles=(0, 8)), INVALID_ARG), (dict(tiles=(8, 17)), INVALID_ARG), (dict(residual_variant=2), INVALID_ARG),
                     (dict(max_width=8193), CAPACITY), (dict(max_batch=0), INVALID_ARG)):
        with pytest.raises(A.GfsError) as e:
            A.Clahe(**kw)
        assert e.value.code == code, kw
    cfg = A.ClaheConfig()
    L.gfs_clahe_default_config(C.byref(cfg))
    assert (cfg.clip_limit, cfg.tiles_x, cfg.tiles_y, cfg.residual_variant) == (3.0, 8, 8, A.CLAHE_RESIDUAL_STEPPED)
    assert L.gfs_clahe_create(0, W, H, 1, C.byref(cfg), None) == INVALID_ARG
    h = C.c_void_p()
    assert L.gfs_clahe_create(0, W, H, 1, None, C.byref(h)) == INVALID_ARG and not h

    # the pyramid entries: a CLAHE reserve below the tracker's image, a foreign pyramid, NULLs, batch above either reserve
    trk, other = A.KltTracker(W, H, 21, max_batch=1, max_points=16), A.KltTracker(W, H, 21, max_batch=1, max_points=16)
    pyr, foreign = A.KltPyramid(trk), A.KltPyramid(other)
    small = A.Clahe(W - 1, H)
    trk.buildOpticalFlowPyramid(img, pyramid=pyr, clahe=cl)
    good = pyr.download()
    ip2, op2 = (C.c_void_p * 2)(*[img.ctypes.data] * 2), (C.c_void_p * 2)(*[out.ctypes.data] * 2)
    calls = [
        (INVALID_ARG, lambda: L.gfs_klt_build_pyramid_clahe(trk.h, small.h, pyr.h, ip, W, 1, None, 0)),
        (INVALID_ARG, lambda: L.gfs_klt_build_pyramid_clahe(trk.h, cl.h, foreign.h, ip, W, 1, None, 0)),
        (INVALID_ARG, lambda: L.gfs_klt_build_pyramid_clahe(trk.h, None, pyr.h, ip, W, 1, None, 0)),
        (INVALID_ARG, lambda: L.gfs_klt_build_pyramid_clahe(trk.h, cl.h, pyr.h, null, W, 1, None, 0)),
        (INVALID_ARG, lambda: L.gfs_klt_build_pyramid_clahe(trk.h, cl.h, pyr.h, ip, W, 1, null, W)),
        (INVALID_ARG, lambda: L.gfs_klt_build_pyramid_clahe(trk.h, cl.h, pyr.h, ip, W - 1, 1, None, 0)),
        (INVALID_ARG, lambda: L.gfs_klt_build_pyramid_clahe(trk.h, cl.h, pyr.h, ip, W, 1, op, W - 1)),
        (CAPACITY, lambda: L.gfs_klt_build_pyramid_clahe(trk.h, cl.h, pyr.h, ip2, W, 2, op2, W)),
        (INVALID_ARG, lambda: L.gfs_klt_build_pyramid_clahe_device(trk.h, small.h, pyr.h, d_img, W, 1, None, 0, None)),
        (INVALID_ARG, lambda: L.gfs_klt_build_pyramid_clahe_device(trk.h, cl.h, foreign.h, d_img, W, 1, None, 0, None)),
        (INVALID_ARG, lambda: L.gfs_klt_build_pyramid_clahe_device(trk.h, cl.h, pyr.h, None, W, 1, None, 0, None)),
        (INVALID_ARG, lambda: L.gfs_klt_build_pyramid_clahe_device(trk.h, cl.h, pyr.h, d_img, W - 1, 1, None, 0, None)),
        (INVALID_ARG, lambda: L.gfs_klt_build_pyramid_clahe_device(trk.h, cl.h, pyr.h, d_img, W, 1, d_img, W + 4, None)),
        (CAPACITY, lambda: L.gfs_klt_build_pyramid_clahe_device(trk.h, cl.h, pyr.h, d_img, W, 2, None, 0, None)),
    ]
    for k, (code, call) in enumerate(calls):
        assert call() == code, k
        still_fine()
        again = pyr.download()
        assert again[0].tobytes() == good[0].tobytes() and again[1].tobytes() == good[1].tobytes(), k
    _same(hip.to_host(d_img, (H, W), np.uint8), img, "a refused in-place call wrote nothing")
