"""The lidar local-map build (LidarMapping::viewer, reference src/LidarMapping.cc:130-185) on the CPU: the sequential restatement
(tests/host/lidar_map_restatement.cpp) against an independent numpy statement of DESIGN.md section 11's rule, bit for bit; the
transform alone against numpy evaluated one operation at a time; the new symbols, the classes without a GPU, the reference's
literals.  No GPU."""
import glob
import json
import os
import re

import numpy as np
import pytest

import lidar_map_support as LMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
F = np.float32
INT32_MAX = 2147483647


# ------------------------------------------------------------------ the rule in numpy (written from DESIGN.md section 11)

def np_pose_matrix(q, t):
    """toMatrix4d(SE3f(q, t).inverse()): every operation a float32 numpy call, then widened."""
    c = np.array([-q[0], -q[1], -q[2], q[3]], F)
    n2 = F(c[0] * c[0])
    for k in (1, 2, 3):
        n2 = F(n2 + F(c[k] * c[k]))
    c = (c / np.sqrt(n2, dtype=F)).astype(F)
    x, y, z, w = c
    p = (np.asarray(t, F) * F(-1.0)).astype(F)
    v = np.array([x, y, z], F)

    def cross(a, b):
        return np.array([F(F(a[1] * b[2]) - F(a[2] * b[1])), F(F(a[2] * b[0]) - F(a[0] * b[2])), F(F(a[0] * b[1]) - F(a[1] * b[0]))], F)

    uv = cross(v, p)
    uv = (uv + uv).astype(F)
    tr = ((p + (w * uv).astype(F)).astype(F) + cross(v, uv)).astype(F)
    tx, ty, tz = F(F(2) * x), F(F(2) * y), F(F(2) * z)
    twx, twy, twz = F(tx * w), F(ty * w), F(tz * w)
    txx, txy, txz = F(tx * x), F(ty * x), F(tz * x)
    tyy, tyz, tzz = F(ty * y), F(tz * y), F(tz * z)
    one = F(1)
    R = np.array([[one - F(tyy + tzz), F(txy - twz), F(txz + twy)],
                  [F(txy + twz), one - F(txx + tzz), F(tyz - twx)],
                  [F(txz - twy), F(tyz + twx), one - F(txx + tyy)]], F)
    M = np.zeros((3, 4))
    M[:, :3] = R.astype(np.float64)
    M[:, 3] = tr.astype(np.float64)
    return M


def np_transform(w):
    out = []
    cb = w["cloud_begin"]
    for k in range(len(w["q"])):
        M = np_pose_matrix(w["q"][k], w["t"][k])
        c = np.asarray(w["cloud"][cb[k]:cb[k + 1]], F).astype(np.float64)
        o = np.zeros((len(c), 3), F)
        for r in range(3):
            a = np.multiply(M[r, 0], c[:, 0])
            b = np.multiply(M[r, 1], c[:, 1])
            s = np.add(a, b)
            s = np.add(s, np.multiply(M[r, 2], c[:, 2]))
            s = np.add(s, M[r, 3])
            o[:, r] = s.astype(F)
        out.append(o)
    return np.concatenate(out) if out else np.zeros((0, 3), F)


def np_voxel(xyz, leaf):
    """-> (status, points, info) with status 'ok' | 'invalid' | 'unsupported'."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    n = len(xyz)
    info = dict(n_in=n, n_out=0, passthrough=0, div=(0, 0, 0))
    leaf = F(leaf)
    if n < 1 or not np.isfinite(leaf) or not leaf > 0 or not np.isfinite(xyz).all() or not (np.abs(xyz) < F(1e6)).all():
        return "invalid", None, info
    with np.errstate(all="ignore"):
        inv = F(1.0) / leaf
        mn, mx = xyz.min(0), xyz.max(0)
        fd = ((mx - mn).astype(F) * inv).astype(F)
    cells, passthrough = 1, False
    for a in range(3):
        if not fd[a] < F(2147483648.0):
            passthrough = True
            break
        cells *= int(fd[a]) + 1  # Python integers: the product itself
        if cells > INT32_MAX:
            passthrough = True
            break
    if passthrough:
        info.update(n_out=n, passthrough=1)
        return "ok", xyz.copy(), info
    lo, hi = np.floor((mn * inv).astype(F)), np.floor((mx * inv).astype(F))
    if not ((np.abs(lo) < F(2147483648.0)).all() and (np.abs(hi) < F(2147483648.0)).all()):
        return "unsupported", None, info
    min_b = [int(v) for v in lo]
    div = [int(hi[a]) - min_b[a] + 1 for a in range(3)]
    if div[0] * div[1] * div[2] > INT32_MAX:
        return "unsupported", None, info
    info["div"] = tuple(div)
    ijk = (np.floor((xyz * inv).astype(F)) - np.array(min_b, F)).astype(F).astype(np.int64)
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    order = np.argsort(idx, kind="stable")  # ascending idx, ascending input index inside a voxel
    sidx = idx[order]
    head = np.flatnonzero(np.r_[True, sidx[1:] != sidx[:-1]])
    count = np.diff(np.r_[head, n])
    s = np.zeros((len(head), 3), F)
    for r in range(int(count.max())):  # the r-th point of every voxel that has one: one float32 addition each
        m = count > r
        s[m] = (s[m] + xyz[order[head[m] + r]]).astype(F)
    info["n_out"] = len(head)
    return "ok", (s / count.astype(F)[:, None]).astype(F), info


def np_build(w, leaf):
    n = int(w["cloud_begin"][-1])
    if n < 5:
        return "invalid", None, dict(n_in=n, n_out=0, passthrough=0, div=(0, 0, 0))
    st, pts, info = np_voxel(np_transform(w), leaf)
    if st == "ok" and info["n_out"] < 5:
        st, pts = "invalid", None
    return st, pts, info


_RC = {"ok": LMS.OK, "invalid": LMS.INVALID_ARG, "unsupported": LMS.UNSUPPORTED}


def _same(got, want):
    rc, pts, info = got
    st, npts, ninfo = want
    assert rc == _RC[st], (rc, st)
    assert info == ninfo, (info, ninfo)
    if st == "ok":
        assert LMS.same_bits(pts, npts)


# ------------------------------------------------------------------ 1. restatement == numpy statement

@pytest.mark.parametrize("seed,n_kf,leaf", LMS.WINDOWS, ids=[f"s{s}_k{k}_l{l}" for s, k, l in LMS.WINDOWS])
def test_windows_match_numpy(seed, n_kf, leaf):
    w = LMS.window(seed, n_keyframes=n_kf, scaled=bool(seed % 2))
    got, want = LMS.build(w, leaf), np_build(w, leaf)
    _same(got, want)
    assert got[2]["passthrough"] == 0 and 5 <= got[2]["n_out"] <= got[2]["n_in"]
    assert got[2]["n_out"] < got[2]["n_in"] or (leaf < 0.1 and n_kf < 7)  # the filter merges points


@pytest.mark.parametrize("case", LMS.constructed_clouds(), ids=[c[0] for c in LMS.constructed_clouds()])
def test_constructed_clouds_match_numpy(case):
    name, xyz, leaf = case
    got, want = LMS.voxel_filter(xyz, leaf), np_voxel(xyz, leaf)
    _same(got, want)
    info = got[2]
    if name == "passthrough":
        assert info["passthrough"] == 1 and info["n_out"] == len(xyz) and LMS.same_bits(got[1], xyz)
    else:
        assert info["passthrough"] == 0
    if name in ("one_voxel", "one_point", "one_point_negative_zero"):
        assert info["n_out"] == 1 and info["div"] == (1, 1, 1)
    if name == "duplicates":
        assert info["n_out"] < 300 + 1
    if name.startswith("multiples"):  # points on voxel faces on both sides of zero fall into the voxel above the face
        assert (xyz.min(0) < 0).all() and (xyz.max(0) > 0).all()


def test_empty_cloud_in_the_middle_of_the_list():
    w = LMS.window(40, n_keyframes=7, empty=(0, 3, 6))
    assert list(np.diff(w["cloud_begin"])[[0, 3, 6]]) == [0, 0, 0]
    _same(LMS.build(w, 0.1), np_build(w, 0.1))
    # the same clouds without the empty key-frames give the same map
    keep = [1, 2, 4, 5]
    cb = w["cloud_begin"]
    w2 = dict(q=w["q"][keep], t=w["t"][keep], cloud=w["cloud"],
              cloud_begin=np.r_[0, np.cumsum([cb[k + 1] - cb[k] for k in keep])].astype(np.int32))
    assert LMS.same_bits(LMS.build(w, 0.1)[1], LMS.build(w2, 0.1)[1])


def test_passthrough_window():
    w = LMS.window(41, n_keyframes=7)
    got = LMS.build(w, LMS.PASSTHROUGH_LEAF)
    _same(got, np_build(w, LMS.PASSTHROUGH_LEAF))
    assert got[2]["passthrough"] == 1 and got[2]["div"] == (0, 0, 0) and LMS.same_bits(got[1], LMS.transform(w))
    # one step coarser the filter still runs
    got = LMS.build(w, 0.004)
    _same(got, np_build(w, 0.004))
    assert got[2]["passthrough"] == 0


def test_refusals():
    xyz, leaf = LMS.overflow_pair()
    got = LMS.voxel_filter(xyz, leaf)
    _same(got, np_voxel(xyz, leaf))
    assert got[0] == LMS.UNSUPPORTED
    p = np.random.default_rng(3).uniform(-1, 1, (50, 3)).astype(F)
    for leaf in (0.0, -0.1, np.inf, np.nan):
        assert LMS.voxel_filter(p, leaf)[0] == LMS.INVALID_ARG and np_voxel(p, leaf)[0] == "invalid"
    for bad in (np.nan, np.inf, 1e6, -2e6):
        b = p.copy()
        b[17, 1] = bad
        assert LMS.voxel_filter(b, 0.1)[0] == LMS.INVALID_ARG and np_voxel(b, 0.1)[0] == "invalid"
    rc, _, info = LMS.voxel_filter(p, 0.1, cap=3)  # nothing is truncated
    assert rc == LMS.CAPACITY and info["n_out"] > 3
    w = LMS.window(42, n_keyframes=2)
    few = dict(q=w["q"], t=w["t"], cloud=w["cloud"][:4], cloud_begin=np.array([0, 2, 4], np.int32))
    assert LMS.build(few, 0.1)[0] == LMS.INVALID_ARG and np_build(few, 0.1)[0] == "invalid"
    one_voxel = dict(q=w["q"][:1], t=w["t"][:1], cloud=w["cloud"][:50], cloud_begin=np.array([0, 50], np.int32))
    got = LMS.build(one_voxel, 100.0)  # fewer than 5 map points
    _same(got, np_build(one_voxel, 100.0))
    assert got[0] == LMS.INVALID_ARG and got[2]["n_out"] < 5


# ------------------------------------------------------------------ 2. the transform alone

def test_transform_one_operation_at_a_time():
    total = 0
    for seed in range(6):
        w = LMS.window(50 + seed, n_keyframes=(1, 2, 7, 30)[seed % 4], scaled=seed != 0)
        norms = np.linalg.norm(w["q"].astype(np.float64), axis=1)
        if seed:
            assert (np.abs(norms - 1) > 1e-6).any()  # not exactly unit: the constructor's normalisation is exercised
        assert LMS.same_bits(LMS.transform(w), np_transform(w))
        total += len(w["cloud"])
    assert total >= 1000
    # the matrix itself
    rng = np.random.default_rng(7)
    for _ in range(200):
        q = rng.normal(size=4)
        q = (q / np.linalg.norm(q) * rng.uniform(0.9, 1.1)).astype(F)
        t = rng.uniform(-5, 5, 3).astype(F)
        M = np.zeros(12)
        LMS.restatement().lmr_pose_matrix(q.ctypes.data, t.ctypes.data, M.ctypes.data)
        assert (M.reshape(3, 4) == np_pose_matrix(q, t)).all()


# ------------------------------------------------------------------ 3. symbols, classes, constants

def test_new_symbols_exported(api):
    L = api.lib()
    for s in ("gfs_lidar_mapper_create", "gfs_lidar_mapper_destroy", "gfs_lidar_map_build", "gfs_lidar_map_fetch",
              "gfs_voxel_grid_filter", "gfs_test_lidar_map_grid"):
        assert hasattr(L, s), s
        assert s in api.ABI_SYMBOLS, s
    assert L.gfs_abi_version() == 1


def test_new_classes_raise_without_gpu(api):
    if api.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(api.GfsError):
        api.LidarMapper()
    with pytest.raises(api.GfsError):
        api.LidarMapper(1000, 4).voxel_filter(np.zeros((5, 3), F), 0.1)
    with pytest.raises(api.GfsError):
        api.LidarMap().fetch()


def test_constants_match_reference():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "lidar_map_constants.json")))
    assert golden["max_new_keyframes"] == 30 and golden["local_resolutions"] == [0.1, 0.2]
    assert set(golden["local_resolutions"]) <= set(LMS.LEAVES)  # the shipped resolutions are among the tested leaves
    if not os.path.exists(os.path.join(REF, "src", "LidarMapping.cc")):
        pytest.skip("the reference is not on this machine")
    src = open(os.path.join(REF, "src", "LidarMapping.cc")).read()
    a = src.index("void LidarMapping::insertKeyFrame(")
    body = src[a:src.index("\n}\n", a)]
    assert int(re.search(r"mlNewKeyFrames\.size\(\) > (\d+)\) mlNewKeyFrames\.pop_front", body).group(1)) == golden["max_new_keyframes"]
    vals = set()
    for y in glob.glob(os.path.join(REF, "**", "*.yaml"), recursive=True):
        for m in re.finditer(r"^LidarMapping\.LocalResolution:\s*([0-9.eE+-]+)", open(y, errors="ignore").read(), re.M):
            vals.add(float(m.group(1)))
    assert sorted(vals) == golden["local_resolutions"]
