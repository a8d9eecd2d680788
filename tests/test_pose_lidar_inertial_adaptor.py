"""gfs_host::PoseLidarVisualInertialOptimizationLastKeyFrame / ...LastFrame (geoflowslam_amd/host/gfs_adaptors.hpp) on mock types
(tests/host/pose_lidar_inertial_adaptor_test.cpp): what they add to the gather of the inertial adaptors -- the stored poses, the signed
time gap in key-frame mode, the cloud (a null one gives n_cloud = 0), the map handle -- and what they write back by reference.  The solve
is a recorder: no device, no restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import pose_inertial_support as S

ROOT = S.ROOT
_HOST = os.path.join(ROOT, "tests", "host")
_SRC = os.path.join(_HOST, "pose_lidar_inertial_adaptor_test.cpp")
_SO = os.path.join(_HOST, "_pose_lidar_inertial_adaptor_test.so")
KF, FR = S.KF, S.FR


def call(mode, N=9, cloud=None, t_frame=10.5, t_kf=10.0):
    L = S._build(_SO, _SRC, [_SRC, os.path.join(_HOST, "pose_inertial_adaptor_test.cpp"), os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp"),
                             os.path.join(ROOT, "include", "gfs_abi.h")])
    L.pose_lidar_inertial_adaptor_test.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    n_cloud = -1 if cloud is None else len(cloud)
    c = np.zeros((1, 3), np.float32) if cloud is None else np.ascontiguousarray(cloud, np.float32)
    seen, head, back = np.zeros((max(n_cloud, 1), 3), np.float32), np.zeros(10), np.zeros(6)
    assert L.pose_lidar_inertial_adaptor_test(mode, N, n_cloud, c.ctypes.data, t_frame, t_kf, seen.ctypes.data, head.ctypes.data, back.ctypes.data) == 0
    return seen, head, back


@pytest.mark.parametrize("mode", [KF, FR])
def test_gather_and_write_back(mode):
    cloud = np.random.default_rng(1).normal(size=(70, 3)).astype(np.float32)
    seen, head, back = call(mode, cloud=cloud)
    assert (seen == cloud).all()
    assert head.tolist() == [mode, 9, 70, 0.5 if mode == KF else 0.0, 1.0, 3.0, 1.0, 0.25, 1.0, 1.0]
    assert back.tolist() == [77, 31, 0.75, 42.0, 4, 1]  # the return value, nInliersLidar, residual, the new prior, mvbOutlier, the estimate


def test_the_time_gap_is_signed():
    assert call(KF, cloud=np.zeros((3, 3)), t_frame=10.0, t_kf=11.0)[1][3] == -1.0


@pytest.mark.parametrize("mode", [KF, FR])
def test_a_null_cloud_gives_no_points(mode):
    _, head, back = call(mode, cloud=None)
    assert head[2] == 0 and head[9] == 1 and back[0] == 77
    assert call(mode, cloud=np.zeros((0, 3)))[1][2] == 0
