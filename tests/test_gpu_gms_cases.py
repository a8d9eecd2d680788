"""csrc/gms.hip on built cases (MI355X): ties for a row's maximum, key-points on and beyond the borders, index lists that are
no arange, frames of two sizes, match counts around the 256-thread stride and at the capacity, one heavily loaded cell, and
gfs_gms_inlier_mask with several problems in one call.  Every case is compared with the C++ oracle AND the numpy restatement
(gms_support.py; the two are compared with each other, and the cases checked for the edges they are meant to hit, on the CPU in
test_frame_gms_references.py).  Masks and counts are integers: array_equal, no tolerance."""
import numpy as np
import pytest

import gms_support as gs

pytestmark = pytest.mark.gpu

CAPACITY = -4  # GFS_ERR_CAPACITY (include/gfs_abi.h)
S = 8192  # key-points / matches per frame of the handle: the kernel's capacity


@pytest.fixture(scope="module")
def cases():
    return gs.all_cases()


@pytest.fixture(scope="module")
def expected(cases, oracle):
    """name -> (mask, n): the restatement's, after it has been found equal to the oracle's"""
    out = {}
    for name, c in cases.items():
        m, n = gs.gms_ref(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"])
        mo, no = oracle.gms_inlier_mask(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"])
        assert n == no and np.array_equal(m, mo), name
        out[name] = (m, n)
    return out


@pytest.fixture(scope="module")
def gm(gpu_api):
    return gpu_api.GmsMatcher(max_keypoints=S, max_batch=8)


def _problem(c):
    return c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"]


def _host(gm, cases, expected, name):
    m, n = gm.GetInlierMask(*_problem(cases[name]))
    assert n == expected[name][1] and np.array_equal(m, expected[name][0]), name
    return m


@pytest.mark.parametrize("name", ["tie", "tie_swapped"])
def test_tie_for_the_row_maximum(gm, cases, expected, name):
    """4(a): 111 : 111 votes in every left cell of a 3 x 3 block; VerifyCellPairs keeps the first maximum over ascending right
    index, so the matches into the lower right cell are the inliers, whichever half of the list they are."""
    m = _host(gm, cases, expected, name)
    winners = 0 if name == "tie_swapped" else 1
    assert int(m[winners::2].sum()) == 999 and int(m[1 - winners::2].sum()) == 0


@pytest.mark.parametrize("name", ["borders", "quirk", "quirk_minus2"])
def test_borders(gm, cases, expected, name):
    """4(b): x == width, negative coordinates, right cells below 0, at and beyond 400 and beyond a short; and the reference's
    comparison of an unpaired left cell (-1, or -2 below the threshold) with a right index of the same value"""
    m = _host(gm, cases, expected, name)
    if name == "quirk":
        assert m.tolist() == [True]
    if name == "quirk_minus2":
        assert m.tolist() == [False, False, True]


@pytest.mark.parametrize("kind", gs.INDEX_KINDS)
def test_index_lists_and_frame_sizes(gm, cases, expected, kind):
    """4(c): query lists that are a subset, a shuffle, with repeats; many matches onto one train point; two frame sizes"""
    _host(gm, cases, expected, "index_" + kind)


@pytest.mark.parametrize("name", [f"count_{n}" for n in gs.COUNTS] + ["one_cell"])
def test_match_counts(gm, cases, expected, name):
    """4(d): around the 256-thread stride, at the capacity of 8192, and 2048 matches out of one left cell"""
    _host(gm, cases, expected, name)


def test_host_batch(gpu_api, gm, cases, expected):
    """4(e): six problems in one gfs_gms_inlier_mask call, an empty one among them: each equals its own single call"""
    got = gm.GetInlierMaskBatch([_problem(cases[k]) for k in gs.HOST_BATCH])
    assert len(gs.HOST_BATCH) == 6 and len(got) == 6
    for k, (m, n) in zip(gs.HOST_BATCH, got):
        m1, n1 = gm.GetInlierMask(*_problem(cases[k]))
        assert n == n1 == expected[k][1] and np.array_equal(m, m1) and np.array_equal(m, expected[k][0]), k
    got = gm.GetInlierMaskBatch([_problem(cases[k]) for k in gs.HOST_BATCH[::-1]])  # other slots of the staging buffers
    for k, (m, n) in zip(gs.HOST_BATCH[::-1], got):
        assert n == expected[k][1] and np.array_equal(m, expected[k][0]), k
    with pytest.raises(gpu_api.GfsError) as e:
        gm.GetInlierMaskBatch([_problem(cases["quirk"])] * 9)
    assert e.value.code == CAPACITY


def test_device_entry_on_the_arange_cases(gm, cases, expected):
    """The cases whose matches are (i, train[i]) between frames of one size, as ONE batch through
    gfs_gms_inlier_mask_batch_device; nothing is written at and beyond a pair's match count."""
    from test_gpu_gms import _Hip
    names = [k for k, c in cases.items() if gs.is_arange(c) and c["size1"] == (gs.W, gs.H)]
    assert {"tie", "tie_swapped", "borders", "quirk", "quirk_minus2", "one_cell"} <= set(names)
    assert {f"count_{n}" for n in gs.COUNTS} <= set(names)
    hip = _Hip()
    try:
        for lo in range(0, len(names), 8):
            part = names[lo:lo + 8]
            B = len(part)
            kp1, kp2 = np.zeros((B, S), gs.KP_DTYPE), np.zeros((B, S), gs.KP_DTYPE)
            t = np.zeros((B, S), np.int32)
            n1, n2 = np.zeros(B, np.int32), np.zeros(B, np.int32)
            for b, k in enumerate(part):
                c = cases[k]
                n1[b], n2[b] = len(c["kp1"]), len(c["kp2"])
                kp1[b, :n1[b]], kp2[b, :n2[b]], t[b, :n1[b]] = c["kp1"], c["kp2"], c["t"]
            d_mask, d_cnt = hip.to_device(np.full((B, S), 0xA5, np.uint8)), hip.to_device(np.full(B + 8, -7, np.int32))
            gm.inlier_mask_batch_device(hip.to_device(kp1), hip.to_device(n1), hip.to_device(kp2), hip.to_device(n2), B, S,
                                        hip.to_device(t), gs.W, gs.H, d_mask, d_cnt)
            mask, cnt = hip.to_host(d_mask, (B, S), np.uint8), hip.to_host(d_cnt, B + 8, np.int32)
            assert (cnt[B:] == -7).all()
            for b, k in enumerate(part):
                m, n = expected[k]
                assert cnt[b] == n and np.array_equal(mask[b, :n1[b]], m.astype(np.uint8)), k
                assert (mask[b, n1[b]:] == 0xA5).all(), k
    finally:
        hip.free()
