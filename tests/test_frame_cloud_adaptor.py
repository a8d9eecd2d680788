"""The Frame constructor's lidar-feature tail as adaptor code (geoflowslam_amd/host/gfs_adaptors.hpp: FrameCloudConfigFrom and
FrameCloudExtractor) over a plain stand-in for LidarParam (tests/host/frame_cloud_adaptor_test.cpp).  The CPU test checks the
configuration the adaptor derives and that the restatement run with it is the restatement of the same values; the GPU test runs
FrameCloudExtractor::Extract against the restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import frame_cloud_support as FCS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(ROOT, "tests", "host", "_frame_cloud_adaptor_test.so")
PARAMS = [(70.0, 9.0, 0.05, 0.05), (91.2, 8.0, 0.2, 0.1)]


@pytest.fixture(scope="module")
def harness(api):
    src = os.path.join(ROOT, "tests", "host", "frame_cloud_adaptor_test.cpp")
    deps = [src, os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp"), os.path.join(ROOT, "include", "gfs_abi.h")]
    if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
        libdir = os.path.join(ROOT, "geoflowslam_amd")
        tmp = _SO + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-o", tmp, src, "-L" + libdir, "-lgfs_hip", "-ldl",
                        "-lpthread", "-Wl,-rpath," + libdir], check=True)
        os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    d, f, vp = C.c_double, C.c_float, C.c_void_p
    L.fca_config.argtypes = [d, d, d, f, vp]
    L.fca_extract.argtypes = [d, d, d, f, vp, C.c_int, vp, vp, vp]
    return L


@pytest.mark.parametrize("params", PARAMS)
def test_adaptor_config(harness, params):
    out = np.zeros(5)
    harness.fca_config(*params, out.ctypes.data)
    assert out.tolist() == [params[0], params[1], params[2], float(np.float32(params[3])), 1e-9]
    cloud = FCS.grid_cloud(7, 40, 10)
    kw = dict(zip(("horizontal_angle", "max_distance", "local_map_resolution", "downsize_resolution"), out[:4].tolist()))
    a, b = FCS.restate(cloud, **kw), FCS.restate(cloud, **dict(zip(kw, params)))
    assert a["rc"] == 0 and a["info"] == b["info"] and all(FCS.same_bits(a[k], b[k]) for k in FCS.STAGES)


@pytest.mark.gpu
@pytest.mark.parametrize("params", PARAMS)
def test_adaptor_extract_gpu(gpu_api, harness, params):
    cloud = FCS.scene_cloud(5)
    n = len(cloud)
    oc, od, info = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(13, np.int32)
    assert harness.fca_extract(*params, cloud.ctypes.data, n, oc.ctypes.data, od.ctypes.data, info.ctypes.data) == 0
    ref = FCS.restate(cloud, **dict(zip(("horizontal_angle", "max_distance", "local_map_resolution", "downsize_resolution"), params)))
    I = dict(zip(FCS.INFO, (int(v) for v in info[:10])), passthrough=tuple(int(v) for v in info[10:]))
    assert I == ref["info"]
    assert FCS.same_bits(oc[:I["n_surf"] + I["n_edge"]], ref["cloud"]) and FCS.same_bits(od[:I["n_down"]], ref["down"])
    assert harness.fca_extract(*params, cloud.ctypes.data, 0, oc.ctypes.data, od.ctypes.data, info.ctypes.data) == -100  # a refusal throws
