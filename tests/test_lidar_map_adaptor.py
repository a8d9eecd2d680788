"""LidarMapping::viewer's loop body as adaptor code (geoflowslam_amd/host/gfs_adaptors.hpp: gfs_host::GatherLidarKeyFrames and
LidarLocalMapper) over plain-struct key-frames (tests/host/lidar_map_adaptor_test.cpp).  The CPU test checks the gather (list order,
bad key-frames and key-frames without a cloud skipped, empty clouds kept) and the map against the sequential restatement called on
the expected key-frames; the GPU test runs LidarLocalMapper::Update."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lidar_map_support as LMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(ROOT, "tests", "host", "_lidar_map_adaptor_test.so")


@pytest.fixture(scope="module")
def harness(api):
    src = os.path.join(ROOT, "tests", "host", "lidar_map_adaptor_test.cpp")
    deps = [src, os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp"), os.path.join(ROOT, "include", "gfs_abi.h")]
    if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
        libdir = os.path.join(ROOT, "geoflowslam_amd")
        tmp = _SO + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-o", tmp, src, "-L" + libdir, "-lgfs_hip", "-ldl",
                        "-lpthread", "-Wl,-rpath," + libdir], check=True)
        os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    L.lidar_map_adaptor_test.argtypes = [C.c_char_p, C.c_int] + [C.c_void_p] * 6 + [C.c_float] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    return L


def _run(L, w, bad, no_cloud, leaf, restated):
    k, n = len(w["q"]), len(w["cloud"])
    bad_a = np.array([i in bad for i in range(k)], np.uint8)
    has = np.array([i not in no_cloud for i in range(k)], np.uint8)
    q, t, cb, cloud = LMS._inputs(w)
    o = dict(sizes=np.zeros(2, np.int32), q=np.zeros((k, 4), np.float32), t=np.zeros((k, 3), np.float32), cb=np.zeros(k + 1, np.int32),
             cloud=np.zeros((max(n, 1), 3), np.float32), xyz=np.zeros((max(n, 1), 3), np.float32), info=np.zeros(6, np.int32))
    if restated:
        LMS.restatement()
    o["rc"] = L.lidar_map_adaptor_test(LMS._SO.encode() if restated else None, k, q.ctypes.data, t.ctypes.data, bad_a.ctypes.data,
                                       has.ctypes.data, cb.ctypes.data, cloud.ctypes.data, leaf,
                                       *[o[x].ctypes.data for x in ("sizes", "q", "t", "cb", "cloud")], o["xyz"].ctypes.data, n,
                                       o["info"].ctypes.data)
    return o


def _expected(w, bad, no_cloud):
    keep = [i for i in range(len(w["q"])) if i not in bad and i not in no_cloud]
    cb = w["cloud_begin"]
    clouds = [w["cloud"][cb[i]:cb[i + 1]] for i in keep]
    return dict(q=w["q"][keep], t=w["t"][keep], cloud=np.concatenate(clouds).reshape(-1, 3),
                cloud_begin=np.r_[0, np.cumsum([len(c) for c in clouds])].astype(np.int32))


CASES = [(60, 7, (), (), ()), (61, 7, (0, 4), (2,), (5,)), (62, 30, (3, 29), (0, 1, 17), (9, 10))]


def _check(o, w, bad, no_cloud, leaf):
    e = _expected(w, bad, no_cloud)
    k = len(e["q"])
    assert o["rc"] == 0
    assert list(o["sizes"]) == [k, len(e["cloud"])]
    assert np.array_equal(o["q"][:k], e["q"]) and np.array_equal(o["t"][:k], e["t"])  # list order, skipped key-frames left out
    assert np.array_equal(o["cb"][:k + 1], e["cloud_begin"]) and np.array_equal(o["cloud"][:len(e["cloud"])], e["cloud"])
    rc, pts, info = LMS.build(e, leaf)
    assert rc == 0 and LMS._info(o["info"]) == info
    assert LMS.same_bits(o["xyz"][:info["n_out"]], pts)


@pytest.mark.parametrize("seed,k,bad,no_cloud,empty", CASES)
def test_gather_and_map_against_restatement(harness, seed, k, bad, no_cloud, empty):
    w = LMS.window(seed, n_keyframes=k, n_cloud=300, empty=empty)
    assert all(w["cloud_begin"][i + 1] == w["cloud_begin"][i] for i in empty)
    _check(_run(harness, w, bad, no_cloud, 0.1, True), w, bad, no_cloud, 0.1)


def test_no_key_frame_left(harness):
    w = LMS.window(63, n_keyframes=2, n_cloud=100)
    o = _run(harness, w, (0,), (1,), 0.1, True)
    assert o["rc"] == LMS.INVALID_ARG and list(o["sizes"]) == [0, 0]  # a build over zero points is refused


@pytest.mark.gpu
@pytest.mark.parametrize("seed,k,bad,no_cloud,empty", CASES)
def test_local_mapper_update_on_gpu(harness, gpu_api, seed, k, bad, no_cloud, empty):
    w = LMS.window(seed, n_keyframes=k, n_cloud=300, empty=empty)
    _check(_run(harness, w, bad, no_cloud, 0.1, False), w, bad, no_cloud, 0.1)
