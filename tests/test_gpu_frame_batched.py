"""csrc/frame.hip at batch sizes, ragged counts, edge values and through its refusals (MI355X): k_depth_to_cloud,
k_stereo_from_rgbd and k_depth_u16_to_f32 through the *_batch_device entries with B > 1, and the host entries' capacity and
resident-depth contracts.  Every expectation is the numpy restatement of frame_helpers_support.py (checked against the C++ oracle
and for its input conditions on the CPU, test_frame_gms_references.py); every comparison is on bit patterns.  Every output buffer
is filled with a sentinel pattern before the call, and everything the call may not write must still hold it afterwards."""
import ctypes as C
import functools

import numpy as np
import pytest

import frame_helpers_support as fs

pytestmark = pytest.mark.gpu

INVALID_ARG, CAPACITY = -1, -4  # GFS_ERR_* (include/gfs_abi.h)
GUARD = 64  # elements (points / values) of sentinel checked after the last slab


@pytest.fixture(scope="module")
def hip():
    from test_gpu_gms import _Hip
    h = _Hip()
    yield h
    h.free()


@pytest.fixture(scope="module")
def fr(gpu_api):
    return gpu_api.Frame(max_rows=240, max_cols=320, max_keypoints=1024)


def _holds_sentinel(a):
    return bool((fs.bits(a) == fs.SENTINEL).all())


@functools.lru_cache(maxsize=None)
def _cloud(name, B):
    depth, ds, K, _ = fs.cloud_batch(name, B)
    return depth, ds, tuple(float(k) for k in K), [fs.cloud_ref(depth[b], ds, *K) for b in range(B)]


def _run_cloud(fr, hip, depth, ds, K, stride_pts):
    B, rows, cols = depth.shape
    d_depth = hip.to_device(depth)
    d_out = hip.to_device(fs.sentinel((B * stride_pts + GUARD, 4)))
    d_cnt = hip.to_device(fs.sentinel(B + GUARD, np.int32))
    fr.depth_to_cloud_batch_device(d_depth, B, rows, cols, ds, *K, d_out, stride_pts, d_cnt)
    out = hip.to_host(d_out, (B * stride_pts + GUARD, 4), np.float32)
    cnt = hip.to_host(d_cnt, B + GUARD, np.int32)
    return out[:B * stride_pts].reshape(B, stride_pts, 4), out[B * stride_pts:], cnt[:B], cnt[B:]


def _check_cloud(slabs, guard, cnt, cnt_guard, refs, stride_pts):
    assert _holds_sentinel(guard) and _holds_sentinel(cnt_guard)
    assert cnt.tolist() == [len(r) for r in refs]  # the full count, also where it exceeds the slab
    for b, ref in enumerate(refs):
        n = min(len(ref), stride_pts)
        assert np.array_equal(fs.bits(slabs[b, :n]), fs.bits(ref[:n])), f"frame {b}"
        assert _holds_sentinel(slabs[b, n:]), f"frame {b}: written past its {n} points"


@pytest.mark.parametrize("B", fs.CLOUD_BATCHES)
@pytest.mark.parametrize("name", list(fs.CLOUD_SHAPES))
def test_cloud_batched(fr, hip, name, B):
    """3(a): a different depth map per frame, ragged counts (an empty frame, a full one, one whose points all come from the last
    1024-sample round), grid totals on and around one round."""
    depth, ds, K, refs = _cloud(name, B)
    stride_pts = max(len(r) for r in refs) + 5
    _check_cloud(*_run_cloud(fr, hip, depth, ds, K, stride_pts), refs, stride_pts)


@pytest.mark.parametrize("name,B", [("41x25", 5), ("53x37s3", 17), ("320x240s2", 5)])
def test_cloud_overflow(fr, hip, name, B):
    """3(b): a slab as large as the largest count, one point short of it, and of one point: counts[b] still reports every valid
    sample, the first min(count, stride_pts) points are right, and neither the next slab nor the guard is written."""
    depth, ds, K, refs = _cloud(name, B)
    most = max(len(r) for r in refs)
    assert most > 2
    for stride_pts in (most, most - 1, 1):
        _check_cloud(*_run_cloud(fr, hip, depth, ds, K, stride_pts), refs, stride_pts)


def test_cloud_host_entry_capacity(gpu_api, fr):
    """gfs_depth_to_cloud with room for one point less than there are: GFS_ERR_CAPACITY, *n the full count, buffer untouched."""
    depth, ds, K, refs = _cloud("53x37s3", 5)
    b = int(np.argmax([len(r) for r in refs]))
    ref, d = refs[b], np.ascontiguousarray(depth[b])
    out, n = fs.sentinel((len(ref) + 8, 4)), C.c_int(-7)
    args = (fr.h, C.c_void_p(d.ctypes.data), d.shape[0], d.shape[1], d.shape[1], ds, *K, C.c_void_p(out.ctypes.data))
    assert gpu_api.lib().gfs_depth_to_cloud(*args, len(ref) - 1, C.byref(n)) == CAPACITY
    assert n.value == len(ref) and _holds_sentinel(out)
    assert gpu_api.lib().gfs_depth_to_cloud(*args, len(ref), C.byref(n)) == 0  # exactly enough
    assert n.value == len(ref) and np.array_equal(fs.bits(out[:len(ref)]), fs.bits(ref)) and _holds_sentinel(out[len(ref):])


@pytest.mark.parametrize("which", ["dense", "strided"])
def test_cloud_special_depths(fr, hip, which):
    """3(c): NaN, the infinities, the zeros, negatives, 10 and its float neighbours, and subnormal depths on the samples (and off
    them, where they change nothing).  The expected cloud holds subnormal x / y / z: it is reproduced only while the kernels
    keep fp32 subnormals on input and output."""
    d, ds, K = fs.special_depth_case(which)
    K = tuple(float(k) for k in K)
    ref = fs.cloud_ref(d, ds, *K)
    assert (fs.is_subnormal(ref[:, 0]) | fs.is_subnormal(ref[:, 1])).sum() >= 8
    stride_pts = len(ref) + 3
    for B in (1, 3):
        _check_cloud(*_run_cloud(fr, hip, np.stack([d] * B), ds, K, stride_pts), [ref] * B, stride_pts)
    got = fr.ConvertDepthToPointCloud(d, ds, *K)
    assert got.shape == ref.shape and np.array_equal(fs.bits(got), fs.bits(ref))


# ----------------------------------------------------------------------------------------------------------------------- stereo
@functools.lru_cache(maxsize=None)
def _stereo(B, kp_stride):
    c = fs.stereo_case(B, kp_stride)
    return c, fs.stereo_case_ref(c, True), fs.stereo_case_ref(c, False)


@pytest.mark.parametrize("with_unx", [True, False])
@pytest.mark.parametrize("kp_stride", fs.STEREO_STRIDES)
@pytest.mark.parametrize("B", fs.STEREO_BATCHES)
def test_stereo_batched(fr, hip, B, kp_stride, with_unx):
    """3(d): ragged counts (0 and kp_stride among them), a separate undistorted x or none, coordinates in (-1, 0) that truncate
    to 0, special depths under the key-points (mvuRight = -inf where bf / d overflows).  The depth maps lie behind cols + 1
    elements of another value, so a coordinate rounded down instead of truncated reads something else, still inside the buffer."""
    c, ref_unx, ref_plain = _stereo(B, kp_stride)
    ref_ur, ref_vd = ref_unx if with_unx else ref_plain
    rows, cols = c["rows"], c["cols"]
    front = cols + 1
    d_depth = hip.to_device(np.concatenate([np.full(front, 5.0, np.float32), c["depth"].reshape(-1), np.full(front, 5.0, np.float32)]))
    d_kps, d_unx, d_cnt = hip.to_device(c["kps"]), hip.to_device(c["unx"]), hip.to_device(c["counts"])
    d_ur, d_vd = hip.to_device(fs.sentinel(B * kp_stride + GUARD)), hip.to_device(fs.sentinel(B * kp_stride + GUARD))
    fr.stereo_from_rgbd_batch_device(d_kps, d_unx if with_unx else None, d_cnt, B, kp_stride, d_depth + 4 * front, rows, cols,
                                     c["bf"], d_ur, d_vd)
    ur, vd = hip.to_host(d_ur, B * kp_stride + GUARD, np.float32), hip.to_host(d_vd, B * kp_stride + GUARD, np.float32)
    # (the expectation holds the sentinel at and beyond counts[b])
    assert np.array_equal(fs.bits(ur[:B * kp_stride]), fs.bits(ref_ur).reshape(-1))
    assert np.array_equal(fs.bits(vd[:B * kp_stride]), fs.bits(ref_vd).reshape(-1))
    assert _holds_sentinel(ur[B * kp_stride:]) and _holds_sentinel(vd[B * kp_stride:])


def _strided(depth):
    big = np.full((depth.shape[0] + 9, depth.shape[1] + 14), 3.25, np.float32)
    view = big[3:3 + depth.shape[0], 5:5 + depth.shape[1]]
    view[:] = depth
    assert not view.flags["C_CONTIGUOUS"] and view.strides[0] // 4 == depth.shape[1] + 14
    return view


def test_stereo_host_entries_undistorted_x_and_strided_depth(fr):
    """gfs_stereo_from_rgbd and gfs_frame_rgbd with a separate undistorted x and with a depth view whose rows are not adjacent"""
    c, ref_unx, ref_plain = _stereo(1, 1000)
    n = int(c["counts"][0])
    kps, unx, depth = c["kps"][0, :n], c["unx"][0, :n], c["depth"][0]
    K = tuple(float(k) for k in fs.intrinsics(*depth.shape))
    cloud = fs.cloud_ref(depth, 2, *K)
    for d in (depth, _strided(depth)):
        for u, (ref_ur, ref_vd) in ((unx, ref_unx), (None, ref_plain)):
            ur, vd = fr.ComputeStereoFromRGBD(kps, d, float(c["bf"]), kps_un_x=u)
            assert np.array_equal(fs.bits(ur), fs.bits(ref_ur)[0, :n]) and np.array_equal(fs.bits(vd), fs.bits(ref_vd)[0, :n])
            ur, vd, got, dev = fr.FrameRGBD(kps, d, float(c["bf"]), 2, *K, kps_un_x=u)
            assert np.array_equal(fs.bits(ur), fs.bits(ref_ur)[0, :n]) and np.array_equal(fs.bits(vd), fs.bits(ref_vd)[0, :n])
            assert dev[3] == len(cloud) and np.array_equal(fs.bits(got), fs.bits(cloud))
    got = fr.ConvertDepthToPointCloud(_strided(depth), 2, *K)
    assert np.array_equal(fs.bits(got), fs.bits(cloud))


# -------------------------------------------------------------------------------------------------------------------------- u16
@pytest.mark.parametrize("factor", fs.U16_FACTORS)
@pytest.mark.parametrize("shape", fs.U16_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_u16_conversion_tails(fr, hip, shape, factor):
    """3(e): sizes that are no multiple of the four elements a thread converts at once; nothing is written past the n-th"""
    raw = fs.u16_case(shape)
    n = raw.size
    d_raw = hip.to_device(np.concatenate([raw.reshape(-1), np.full(8, 12345, np.uint16)]))
    d_f = hip.to_device(fs.sentinel(n + GUARD))
    fr.depth_convert_u16_batch_device(d_raw, *shape, factor, d_f)
    got = hip.to_host(d_f, n + GUARD, np.float32)
    assert np.array_equal(fs.bits(got[:n]), fs.bits(fs.u16_ref(raw, factor)).reshape(-1))
    assert _holds_sentinel(got[n:])


def test_u16_conversion_refuses_misaligned_buffers(gpu_api, fr, hip):
    d_raw, d_f = hip.to_device(np.zeros(64, np.uint16)), hip.to_device(fs.sentinel(64))
    for src, dst in ((d_raw + 2, d_f), (d_raw, d_f + 4)):
        with pytest.raises(gpu_api.GfsError) as e:
            fr.depth_convert_u16_batch_device(src, 1, 3, 5, 0.001, dst)
        assert e.value.code == INVALID_ARG
    assert _holds_sentinel(hip.to_host(d_f, 64, np.float32))


# ------------------------------------------------------------------------------------------------------- resident depth map
def _refused(gpu_api, code, call, *a, **kw):
    with pytest.raises(gpu_api.GfsError) as e:
        call(*a, **kw)
    assert e.value.code == code


def test_frame_rgbd_resident_depth_state_machine(gpu_api):
    """3(f): depth = NULL is valid only after a gfs_frame_rgbd upload of the same rows x cols that nothing has overwritten since;
    a refused call leaves the handle usable."""
    c, ref_unx, _ = _stereo(1, 257)
    n = int(c["counts"][0])
    kps, unx, depth, bf = c["kps"][0, :n], c["unx"][0, :n], c["depth"][0], float(c["bf"])
    ur_ref, vd_ref = fs.bits(ref_unx[0])[0, :n], fs.bits(ref_unx[1])[0, :n]
    rows, cols = depth.shape
    K = tuple(float(k) for k in fs.intrinsics(rows, cols))
    cloud = fs.cloud_ref(depth, 1, *K)
    other = np.ascontiguousarray(depth[:rows - 2, :cols - 3])
    fr = gpu_api.Frame(max_rows=rows, max_cols=cols, max_keypoints=n)

    def resident(shape=(rows, cols), ds=0):
        return fr.FrameRGBD(kps, None, bf, ds, *K, kps_un_x=unx, shape=shape)

    def check_resident():
        ur, vd, got, dev = resident(ds=1)  # stereo coordinates and cloud from the map already on the device
        assert np.array_equal(fs.bits(ur), ur_ref) and np.array_equal(fs.bits(vd), vd_ref)
        assert dev[3] == len(cloud) and np.array_equal(fs.bits(got), fs.bits(cloud))

    _refused(gpu_api, INVALID_ARG, resident)  # a fresh handle
    ur, vd, got, dev = fr.FrameRGBD(kps, depth, bf, 1, *K, kps_un_x=unx)  # ... which a valid call then finds undisturbed
    assert np.array_equal(fs.bits(ur), ur_ref) and np.array_equal(fs.bits(vd), vd_ref) and np.array_equal(fs.bits(got), fs.bits(cloud))
    check_resident()
    fr.FrameRGBD(kps[:0], other, bf, 0, *K)  # an upload of another shape
    _refused(gpu_api, INVALID_ARG, resident)
    fr.FrameRGBD(kps[:0], depth, bf, 0, *K)
    _refused(gpu_api, INVALID_ARG, resident, shape=other.shape)
    check_resident()  # the refusals changed nothing
    fr.ConvertDepthToPointCloud(depth, 1, *K)  # overwrites the handle's depth buffer
    _refused(gpu_api, INVALID_ARG, resident)
    fr.FrameRGBD(kps[:0], depth, bf, 0, *K)
    check_resident()
    fr.ComputeStereoFromRGBD(kps, depth, bf)  # so does this
    _refused(gpu_api, INVALID_ARG, resident)
    fr.FrameRGBD(kps[:0], depth, bf, 0, *K)
    check_resident()
    # capacities of the handle and of the caller's cloud buffer
    tall = np.ones((rows + 1, cols), np.float32)
    _refused(gpu_api, INVALID_ARG, fr.FrameRGBD, kps, tall, bf, 1, *K)
    many = np.concatenate([kps, kps[:1]])
    _refused(gpu_api, INVALID_ARG, fr.FrameRGBD, many, depth, bf, 1, *K)
    out, nc = fs.sentinel((len(cloud), 4)), C.c_int(-7)
    ur, vd = np.zeros(n, np.float32), np.zeros(n, np.float32)
    args = (fr.h, C.c_void_p(kps.ctypes.data), None, n, C.c_void_p(depth.ctypes.data), rows, cols, cols, float(bf), 1, *K,
            C.c_void_p(ur.ctypes.data), C.c_void_p(vd.ctypes.data), C.c_void_p(out.ctypes.data))
    assert gpu_api.lib().gfs_frame_rgbd(*args, len(cloud) - 1, C.byref(nc), None, None, None) == CAPACITY
    assert nc.value == len(cloud) and _holds_sentinel(out)
    assert gpu_api.lib().gfs_frame_rgbd(*args, len(cloud), C.byref(nc), None, None, None) == 0
    assert nc.value == len(cloud) and np.array_equal(fs.bits(out), fs.bits(cloud))
    check_resident()
