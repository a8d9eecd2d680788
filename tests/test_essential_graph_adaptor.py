"""CPU test of gfs_host::OptimizeEssentialGraph (geoflowslam_amd/host/gfs_adaptors.hpp) on mock KeyFrame / MapPoint / Map classes
(tests/host/essential_graph_adaptor_test.cpp, which describes the scenario) with the host restatement as the solve: the flattened
graph edge by edge -- creation order, the whole-key-frame and the single-edge `continue`s, the loop connection that pre-empts a
covisibility edge, the CorrectedSim3 / NonCorrectedSim3 mix, the accepted and the refused registration -- and the write-back of poses
and points.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_graph_support as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "essential_graph_adaptor_test.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_essential_graph_adaptor_test.so")
_DEPS = [_SRC, os.path.join(ROOT, "tests", "host", "pose_graph_restatement.cpp"), os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp"),
         os.path.join(ROOT, "geoflowslam_amd", "csrc", "sim3_dev.hpp"), os.path.join(ROOT, "include", "gfs_abi.h")]

IDS = [3, 5, 6, 8, 9, 11, 12, 14]
VERTEX_OF = {0: 0, 1: 1, 3: 2, 4: 3, 5: 4, 6: 5, 7: 6}  # key-frame index -> flat vertex (K2 is bad)
# (key-frame i, key-frame j, weight, measured on the corrected estimates?) in the order the reference makes the edges
EDGES = [(6, 0, 1, True), (7, 0, 1, True), (7, 1, 1, True),            # loop connections; K7 - K4 (weight 50) dropped
         (1, 0, 1, False),                                             # K1's parent
         (4, 3, 1, False), (4, 0, 1, False), ("icp", 4, 0, 3),         # K4: parent, loop edge, its registration; prev K2 has no vertex
         (5, 4, 1, False), (5, 1, 1, False), (5, 3, 1, False),  # K5: parent, loop edge K1 (registration refused; K2 skipped), covisible K3
         (6, 5, 1, False), (6, 4, 1, False), (6, 5, 1, False),         # K6: parent, covisible K4 (K0 already inserted), inertial
         (7, 6, 1, False), (7, 5, 1, False)]                           # K7: parent, covisible K5 (K1 already inserted)


@pytest.fixture(scope="module")
def harness(api):
    if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(p) for p in _DEPS):
        tmp = _SO + f".{os.getpid()}.tmp"
        libdir = os.path.dirname(api._LIB_PATH)
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", tmp, _SRC, "-L" + libdir,
                        "-lgfs_hip", "-Wl,-rpath," + libdir], check=True)
        os.replace(tmp, _SO)
    return C.CDLL(_SO)


def _run(L, fix_scale, use_icp):
    f64, f32, i32 = np.float64, np.float32, np.int32
    o = dict(kf_sim3=np.zeros((8, 8)), corrected=np.zeros((2, 8)), flat_n=np.zeros(3, i32), vq=np.zeros((8, 4)), vt=np.zeros((8, 3)),
             vs=np.zeros(8), vfixed=np.zeros(8, np.uint8), ei=np.zeros(32, i32), ej=np.zeros(32, i32), eq=np.zeros((32, 4)),
             et=np.zeros((32, 3)), es=np.zeros(32), ew=np.zeros(32), points=np.zeros((6, 3), f32), pref=np.zeros(6, i32),
             sol_q=np.zeros((8, 4)), sol_t=np.zeros((8, 3)), sol_s=np.zeros(8), sol_points=np.zeros((6, 3), f32),
             reg_calls=np.zeros((4, 18)), kf_out=np.zeros((8, 8), f32), mp_out=np.zeros((6, 5), f32), counts=np.zeros(5, i32),
             lambda_init=np.zeros(1, f64))
    L.essential_graph_adaptor_test.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * len(o)
    rc = L.essential_graph_adaptor_test(int(fix_scale), int(use_icp), *[v.ctypes.data for v in o.values()])
    assert rc == 0
    return o


@pytest.mark.parametrize("fix_scale,use_icp", [(True, False), (False, True)])
def test_flattening_and_write_back(harness, fix_scale, use_icp):
    o = _run(harness, fix_scale, use_icp)
    V, E, M = (int(v) for v in o["flat_n"])
    assert tuple(o["counts"]) == (1, int(fix_scale), 20, 2 if use_icp else 0, 1) and o["lambda_init"][0] == 1e-16
    # ---- vertices: every key-frame but the bad one, in GetAllKeyFrames order; the corrected estimates where there are any
    assert V == 7 and M == 6
    scw = o["kf_sim3"].copy()
    scw[6:8] = o["corrected"]
    flat_v = np.concatenate([o["vq"][:V], o["vt"][:V], o["vs"][:V, None]], 1)
    for k, v in VERTEX_OF.items():
        assert flat_v[v].tobytes() == scw[k].tobytes(), k
    assert list(o["vfixed"][:V]) == [1, 0, 0, 0, 0, 0, 0]
    assert (o["vs"][5:7] == (1.0 if fix_scale else 1.1)).all()
    # ---- edges, one by one; every measurement is Sjw * Swi in the arithmetic of csrc/sim3_dev.hpp, which numpy restates bit for bit
    want = [e for e in EDGES if use_icp or e[0] != "icp"]
    assert E == len(want)
    flat_e = np.concatenate([o["eq"][:E], o["et"][:E], o["es"][:E, None]], 1)
    for n, e in enumerate(want):
        if e[0] == "icp":
            _, i, j, w = e
            Sli = pg.sim3_mul(o["kf_sim3"][j:j + 1], pg.sim3_inverse(o["kf_sim3"][i:i + 1]))
            R = pg.quat_to_R(Sli[:, 0:4])
            meas = np.concatenate([pg.R_to_quat(R)[0], Sli[0, 4:7] / Sli[0, 7] + np.array([0.01, -0.02, 0.0]), [1.0]])
        else:
            i, j, w, corrected = e
            src = scw if corrected else o["kf_sim3"]
            meas = pg.sim3_mul(src[j:j + 1], pg.sim3_inverse(src[i:i + 1]))[0]
        assert (o["ei"][n], o["ej"][n], o["ew"][n]) == (VERTEX_OF[i], VERTEX_OF[j], w), (n, e)
        assert flat_e[n].tobytes() == meas.tobytes(), (n, e)
    # ---- the registrations: (target, source) = (pLKF, pKF) and the initial guess R(Sli), t / s
    if use_icp:
        assert [tuple(int(v) for v in c[:2]) for c in o["reg_calls"][:2]] == [(IDS[0], IDS[4]), (IDS[1], IDS[5])]
        Sli = pg.sim3_mul(o["kf_sim3"][0:1], pg.sim3_inverse(o["kf_sim3"][4:5]))
        T = o["reg_calls"][0, 2:].reshape(4, 4).T  # column-major
        assert T[:3, :3].tobytes() == pg.quat_to_R(Sli[:, 0:4]).reshape(3, 3).tobytes() and (T[:3, 3] == Sli[0, 4:7] / Sli[0, 7]).all()
        assert (T[3] == [0, 0, 0, 1]).all()
    # ---- the points' references: P1 is bad, P2 goes by mnCorrectedReference (K6), P3's key-frame has no vertex
    assert list(o["pref"]) == [VERTEX_OF[1], -1, VERTEX_OF[6], -1, VERTEX_OF[7], VERTEX_OF[5]]
    # ---- write-back: SetPose(q.cast<float>(), t.cast<float>() / s) for every vertex, the bad key-frame untouched
    for k in range(8):
        if k not in VERTEX_OF:
            assert o["kf_out"][k, 7] == 0
            continue
        v = VERTEX_OF[k]
        assert o["kf_out"][k, 7] == 1
        assert (o["kf_out"][k, 0:4] == o["sol_q"][v].astype(np.float32)).all()
        assert (o["kf_out"][k, 4:7] == o["sol_t"][v].astype(np.float32) / np.float32(o["sol_s"][v])).all()
    assert np.abs(o["sol_t"][:V] - o["vt"][:V]).max() > 1e-3  # the solve moved something
    # ... SetWorldPos and UpdateNormalAndDepth for every point that is not bad, with the solver's corrected position
    for m in range(6):
        calls = (0, 0) if m == 1 else (1, 1)
        assert tuple(o["mp_out"][m, 3:5]) == calls, m
        if m != 1:
            assert (o["mp_out"][m, 0:3] == o["sol_points"][m]).all()
    assert (o["sol_points"][3] == o["points"][3]).all() and (o["sol_points"][1] == o["points"][1]).all()
    # ... and the solver's points are the restatement's at the solver's own poses
    before = flat_v
    after = np.concatenate([o["sol_q"][:V], o["sol_t"][:V], o["sol_s"][:V, None]], 1)
    assert pg.correct_points(before, after, o["points"], o["pref"]).tobytes() == o["sol_points"].tobytes()
    assert (o["sol_points"][0] != o["points"][0]).any()


