"""gfs_host::PoseInertialOptimizationLastKeyFrame / ...LastFrame (geoflowslam_amd/host/gfs_adaptors.hpp) on mock types
(tests/host/pose_inertial_adaptor_test.cpp): the gather order and what it reads, the write-back, the new prior and the deletion of the
old one, the refusals.  The solve is a recorder: no device, no restatement."""
import ctypes as C
import os

import numpy as np
import pytest

import pose_inertial_support as S

ROOT = S.ROOT
_SRC = os.path.join(ROOT, "tests", "host", "pose_inertial_adaptor_test.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_pose_inertial_adaptor_test.so")
KF, FR = S.KF, S.FR


def harness():
    L = S._build(_SO, _SRC, [_SRC, os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp"), os.path.join(ROOT, "include", "gfs_abi.h")])
    i, vp = C.c_int, C.c_void_p
    L.pose_inertial_adaptor_test.argtypes = [i, i, i] + [vp] * 7 + [i] * 4 + [vp] * 9
    return L


def scene(seed, N=40):
    rng = np.random.default_rng(seed)
    has_mp = (rng.random(N) < 0.7).astype(np.uint8)
    has_mp[[0, N - 1]] = [0, 1]
    return dict(N=N, has_mp=has_mp, pos=rng.normal(size=(N, 3)).astype(np.float32), depth=rng.uniform(2, 18, N).astype(np.float32),
                kp=np.stack([rng.uniform(0, 640, N), rng.uniform(0, 480, N), rng.integers(0, 8, N)], 1).astype(np.float32),
                u_right=np.where(rng.random(N) < 0.3, -1.0, rng.uniform(0, 600, N)).astype(np.float32),
                sigma=(1.0 / 1.2 ** (2 * np.arange(8))).astype(np.float32), scripted=(rng.random(N) < 0.4).astype(np.uint8))


def call(sc, mode, kind=0, rec_init=0, f2f=0, f2m=0, n_rounds=4):
    N = sc["N"]
    o = dict(n=np.zeros(1, np.int32), xw=np.zeros((N, 3)), obs=np.zeros((N, 3)), w=np.zeros(N, np.float32), stereo=np.zeros(N, np.uint8),
             close=np.zeros(N, np.uint8), head=np.zeros(12), back=np.zeros(10), after=np.zeros(N, np.uint8))
    ins = [np.ascontiguousarray(sc[k]) for k in ("has_mp", "pos", "depth", "kp", "u_right", "sigma", "scripted")]
    rc = harness().pose_inertial_adaptor_test(mode, kind, N, *(a.ctypes.data for a in ins), rec_init, f2f, f2m, n_rounds, *(v.ctypes.data for v in o.values()))
    assert rc == 0
    return o


@pytest.mark.parametrize("mode", [KF, FR])
def test_gather_order_and_sources(mode):
    sc = scene(1)
    o = call(sc, mode, rec_init=1, n_rounds=3)
    idx = np.nonzero(sc["has_mp"])[0]
    n = int(o["n"][0])
    assert n == len(idx)
    assert (o["xw"][:n] == sc["pos"][idx].astype(np.float64)).all()
    assert (o["obs"][:n, :2] == sc["kp"][idx, :2].astype(np.float64)).all() and (o["obs"][:n, 2] == sc["u_right"][idx].astype(np.float64)).all()
    assert (o["w"][:n] == sc["sigma"][sc["kp"][idx, 2].astype(int)]).all()
    assert (o["stereo"][:n] == (sc["u_right"][idx] >= 0)).all() and (o["close"][:n] == (sc["depth"][idx] < np.float32(10))).all()
    mode_, rounds, rec, cur, other, dT, ig, ia, pH, fx, bf, refused = o["head"]
    assert (mode_, rounds, rec, cur, fx, bf, refused) == (mode, 3, 1, 3.0, 607.0, 45.0, 0)
    # the other end and the preintegration follow the mode; the random-walk information is mpImuPreintegrated's in both
    assert other == (2.0 if mode == FR else 11.0) and dT == np.float32(0.05 if mode == FR else 0.4)
    assert ig == np.float32(0.4) and ia == 2.0 * np.float32(0.4)
    assert pH == (9.0 if mode == FR else 0.0)


@pytest.mark.parametrize("mode", [KF, FR])
def test_write_back(mode):
    sc = scene(2)
    idx = np.nonzero(sc["has_mp"])[0]
    for f2f, f2m in ((0, 0), (1, 0), (0, 1), (1, 1)):
        o = call(sc, mode, f2f=f2f, f2m=f2m)
        ret, gf, gm, t0, t1, t2, n_written, H00, cmode, tally = o["back"]
        assert ret == 77 and (t0, t1, t2, n_written) == (5, 6, 7, 1)
        assert gf == (1.25 if f2f else -1) and gm == (1.25 if f2m else -1)
        want = np.ones(sc["N"], np.uint8)  # key-points without a map point keep what they had
        want[idx] = sc["scripted"][:len(idx)]
        assert (o["after"] == want).all()
        assert (H00, cmode) == (42.0, mode)  # the new prior is made from the returned H, in the call's mode
        # one solve; nothing leaks; in frame mode the previous frame's prior is deleted and cleared, in key-frame mode left alone
        assert tally == 1000 + (100 if mode == FR else 0)


@pytest.mark.parametrize("mode", [KF, FR])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_refusals(mode, kind):
    sc = scene(3)
    o = call(sc, mode, kind=kind)
    refused = kind in (1, 2) or mode == FR  # a missing prior only matters where it is read
    assert o["head"][11] == (1 if refused else 0)
    if refused:  # nothing was gathered, solved or written
        assert o["back"][0] == -1 and o["back"][6] == 0 and o["back"][7] == -1 and (o["after"] == 1).all() and o["back"][9] < 1000
    else:
        assert o["back"][0] == 77
