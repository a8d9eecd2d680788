"""CPU tests of the LocalVisualLidarBA restatement (tests/host/lba_lidar_restatement.cpp) and of the new entry points' plumbing: without
lidar edges it is the LBA oracle bit for bit; its edges are GenerateLidarEdge's; its lidar gradient is the gradient of its robust
cost; the reference's gates (75 inliers, 50 points, fixed cameras, the fixed initial key-frame); the literals against the reference or
tests/golden/lba_lidar_constants.json; the new symbols are exported and refuse to run without a GPU.  No GPU."""
import json
import os
import re

import numpy as np
import pytest

import lba_lidar_support as LLS
import pose_lidar_support as PLS
from geoflowslam_amd import synth
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src/Optimizer.cc"
GOLDEN = os.path.join(ROOT, "tests", "golden", "lba_lidar_constants.json")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_without_lidar_is_the_oracle_bit_for_bit(seed):
    w = synth.lba_window(seed, n_free=6, n_fixed=2, n_points=300)
    r, _ = LLS.solve(w, lidar=False)
    ro = O.lba_solve(w)
    for k in ("pose_q", "pose_t", "points", "edge_chi2", "edge_depth_positive"):
        assert np.array_equal(r[k], ro[k]), k
    assert (r["iterations_run"], r["final_chi2"], r["final_lambda"]) == (ro["iterations_run"], ro["final_chi2"], ro["final_lambda"])
    L, Lo = LLS.linearize(w, lidar=False), O.lba_linearize(w)
    for k in ("Hpp", "Hll", "Hpl", "bp", "bl", "edge_chi2"):
        assert np.array_equal(L[k], Lo[k]), k
    assert L["chi2"] == Lo["chi2"]


def test_edges_are_generate_lidar_edge():
    w = LLS.window(3, n_free=3, n_fixed=1, n_cloud=120, lidar=[0, 1, 2])
    L = LLS.linearize(w)
    n = 0
    for i in range(3):
        q, t = w["pose_q"][i].astype(np.float32), w["pose_t"][i].astype(np.float32)
        cb = w["cloud_begin"]
        exp = []
        for k in range(cb[i], cb[i + 1]):
            keep, plane, s, _ = PLS.point_edge(w["map_xyz"], w["cloud"][k], q, t)
            if keep:
                exp.append((k - cb[i], plane, s))
        idx, pl, s = L["edges"][i]
        assert list(idx) == [e[0] for e in exp]
        assert all((pl[j].view(np.uint32) == exp[j][1].view(np.uint32)).all() and s[j] == exp[j][2] for j in range(len(exp)))
        n += len(exp)
    assert n > 100


def test_lidar_gradient_is_the_cost_gradient():
    """bp of a lidar-only window (no reprojection edge on the pose) against central differences of the robust lidar cost."""
    w = LLS.window(4, n_free=2, n_fixed=1, n_points=40, n_cloud=200, lidar=[0])
    keep = w["edge_pose"] != 0
    w2 = dict(w, edge_pose=w["edge_pose"][keep], edge_point=w["edge_point"][keep], edge_obs=w["edge_obs"][keep],
              edge_inv_sigma2=w["edge_inv_sigma2"][keep], edge_stereo=w["edge_stereo"][keep], n_edges=int(keep.sum()))
    L = LLS.linearize(w2)
    assert L["pose_lidar_edges"][0] > 50
    bp = L["bp"][0]
    # the edges are fixed at the stored pose; the cost at a moved pose: the restatement's chi2 minus the (unchanged) visual part
    idx, pl, s = L["edges"][0]
    cloud = w["cloud"][w["cloud_begin"][0]:w["cloud_begin"][1]].astype(np.float64)[idx]

    def cost(u):
        from scipy.spatial.transform import Rotation
        q, t = w["pose_q"][0], w["pose_t"][0]
        R = Rotation.from_quat(q).as_matrix()
        dR = Rotation.from_rotvec(u[:3]).as_matrix()
        Rn, tn = dR @ R, dR @ t + u[3:]
        pw = (cloud - tn) @ Rn  # Twc p = Rn^T (p - tn)
        e = s * ((pw * pl[:, :3]).sum(1) + pl[:, 3])
        c = 100.0 * e * e
        return np.where(c <= 1.0, c, 2 * np.sqrt(c) - 1).sum()

    h = 1e-6
    g = np.array([(cost(h * np.eye(6)[k]) - cost(-h * np.eye(6)[k])) / (2 * h) for k in range(6)])
    # g2o: b = -J^T W e, cost gradient = 2 J^T W e  ->  bp = -g / 2 (robust weights as in g2o's Huber linearisation)
    assert np.dot(bp, -g / 2) > 0.9 * np.linalg.norm(bp) * np.linalg.norm(g / 2)
    assert 0.5 < np.linalg.norm(bp) / np.linalg.norm(g / 2) < 2.0


def test_gates():
    base = dict(n_free=4, n_fixed=2, n_points=150, n_cloud=200, voxel=0.1)
    w = LLS.window(5, lidar=[0, 1, 2, 3], **base)
    w["matches_inliers"] = np.array([75, 76, 10, 10, 10, 10], np.int32)
    L = LLS.linearize(w)
    pe = L["pose_lidar_edges"]
    assert pe[0] > 0 and pe[1] == 0  # 75 inliers gets edges, 76 gets none
    assert pe[4] == 0 and pe[5] == 0  # fixed cameras never
    # 49 cloud points: none; 50 points: can get edges
    for n, expect in ((49, False), (50, True)):
        cb = w["cloud_begin"]
        cl = [w["cloud"][cb[i]:cb[i + 1]] for i in range(w["n_poses"])]
        cl[2] = cl[2][:n]
        w2 = dict(w, cloud=np.concatenate(cl), cloud_begin=np.r_[0, np.cumsum([len(c) for c in cl])].astype(np.int32))
        assert (LLS.linearize(w2)["pose_lidar_edges"][2] > 0) == expect, n
    # the fixed initial key-frame: its edges count in chi2, not in H / b
    wi = LLS.window(6, init_fixed=True, lidar=[0, 1], **base)
    wj = dict(wi, pose_local=wi["pose_local"].copy())
    wj["pose_local"][0] = 0
    Li, Lj = LLS.linearize(wi), LLS.linearize(wj)
    assert Li["pose_lidar_edges"][0] > 0 and Lj["pose_lidar_edges"][0] == 0
    assert Li["chi2"] > Lj["chi2"]
    wk = dict(wi, matches_inliers=wi["matches_inliers"].copy())
    wk["matches_inliers"][1] = 200
    wl = dict(wj, matches_inliers=wk["matches_inliers"])
    Lk, Ll = LLS.linearize(wk), LLS.linearize(wl)
    assert Lk["chi2"] > Ll["chi2"]
    for k in ("Hpp", "bp", "Hll", "bl", "Hpl"):  # pose 0 fixed: its edges reach chi2 only
        assert np.array_equal(Lk[k], Ll[k]), k


def test_weak_keyframe_ends_closer_with_lidar():
    w = LLS.window(7, n_free=4, n_fixed=2, n_points=200, n_cloud=400, lidar=[2])
    keep = ~((w["edge_pose"] == 2) & (np.arange(w["n_edges"]) % 4 != 0))  # key-frame 2 keeps a quarter of its observations
    w = dict(w, edge_pose=w["edge_pose"][keep], edge_point=w["edge_point"][keep], edge_obs=w["edge_obs"][keep],
             edge_inv_sigma2=w["edge_inv_sigma2"][keep], edge_stereo=w["edge_stereo"][keep], n_edges=int(keep.sum()))
    r, _ = LLS.solve(w)
    r0, _ = LLS.solve(w, lidar=False)
    assert r["pose_lidar_edges"][2] > 50
    err = lambda res: np.linalg.norm(res["pose_t"][2] - w["gt_t"][2])
    assert err(r) < err(r0)


def _reference_constants():
    src = open(REF).read()
    a = src.index("void Optimizer::LocalVisualLidarBA(")
    body = src[a:src.index("\n}\n", a)]
    g = src.index("vector<EdgeType*> Optimizer::GenerateLidarEdge(")
    gen = src[g:src.index("\n}\n", g)]
    return dict(max_inliers=int(re.search(r"mnMatchesInliers > (\d+)", body).group(1)),
                lidar_information=float(re.search(r"information\(0, 0\) = ([0-9.e]+);", body).group(1)),
                huber_delta_lidar=float(np.float32(np.sqrt(float(re.search(r"thHuberLidar = sqrt\(([0-9.]+)\)", body).group(1))))),
                min_cloud=int(re.search(r"mpPointCloudDownsampled->size\(\) < (\d+)\)", gen).group(1)))


def test_constants():
    golden = json.load(open(GOLDEN))
    if os.path.exists(REF):
        exp = _reference_constants()
        for k, v in exp.items():
            assert golden[k] == v, k
        body = open(REF).read()
        a = body.index("void Optimizer::LocalVisualLidarBA(")
        b = body[a:body.index("\n}\n", a)]
        assert b.index("GenerateLidarEdge") < b.index("vpEdgesStereo.push_back")  # lidar edges are added first
    c = LLS.constants()
    assert list(c) == [golden["max_inliers"], golden["lidar_information"], golden["huber_delta_lidar"], golden["min_cloud"],
                       1.0 if golden["edge_order"] == "lidar_first" else 0.0]
    lba = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "lba.hip")).read()
    assert int(re.search(r"kLbaLidarMaxInliers = (\d+);", lba).group(1)) == golden["max_inliers"]
    # the edge's information and Huber delta have one definition, pose_lidar.hip's, which lba.hip reads through lidar_assoc.hpp
    assert "gfs_lidar::edge_information()" in lba and "gfs_lidar::edge_huber_delta()" in lba
    pl = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "pose_lidar.hip")).read()
    assert int(re.search(r"kMinCloud = (\d+);", pl).group(1)) == golden["min_cloud"]
    assert float(re.search(r"kLidarInfo = ([0-9.e]+);", pl).group(1)) == golden["lidar_information"]
    assert float(re.search(r"kThHuberLidar = ([0-9.e]+);", pl).group(1)) == golden["huber_delta_lidar"]
    assert "double edge_information() { return kLidarInfo; }" in pl and "double edge_huber_delta() { return kThHuberLidar; }" in pl


def test_new_entry_points(api):
    L = api.lib()
    for s in ("gfs_lba_lidar_reserve", "gfs_lba_solve_lidar", "gfs_lba_solve_lidar_bool", "gfs_lba_linearize_lidar",
              "gfs_lba_fetch_lidar_edges"):
        assert hasattr(L, s), s
        assert s in api.ABI_SYMBOLS, s
    for m in ("LocalVisualLidarBA", "linearize_lidar", "fetch_lidar_edges"):
        assert callable(getattr(api.Optimizer, m, None)), m
    assert callable(getattr(synth, "lba_lidar_window", None))
    if api.device_count() == 0:
        with pytest.raises(api.GfsError):
            api.Optimizer(max_poses=8, max_points=64, max_edges=256)
        assert L.gfs_lba_lidar_reserve(None, 10) == -1
        assert L.gfs_lba_solve_lidar(None, None, None, None, None, None) == -1
