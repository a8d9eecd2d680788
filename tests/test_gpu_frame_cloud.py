"""GPU tests of the frame cloud (reference src/Frame.cc:378-393 and src/LidarProcess.cc:20-204; gfs_frame_cloud_* in
include/gfs_abi.h): every case bit for bit against the sequential CPU restatement
(tests/host/frame_cloud_restatement.cpp) -- every stage through the test hook, both outputs, every info field -- plus the radius
filter against a count over all pairs, the angle guard's host path, the refusals and the handle's state."""
import ctypes as C

import numpy as np
import pytest

import frame_cloud_support as FCS

pytestmark = pytest.mark.gpu
F = np.float32
CAP = 20480


@pytest.fixture(scope="module")
def handles(gpu_api):
    """One handle per configuration, made on demand and closed with the module."""
    made = {}

    def get(max_points=CAP, **kw):
        key = (max_points,) + tuple(sorted(kw.items()))
        if key not in made:
            made[key] = gpu_api.FrameCloud(max_points=max_points, **kw)
        return made[key]

    yield get
    for h in made.values():
        h.close()


def _check(fc, cloud, **kw):
    """One call and its stages against the restatement; returns (device info, restatement)."""
    ref = FCS.restate(cloud, **kw)
    assert ref["rc"] == FCS.OK, ref["rc"]
    dc, dd, info = fc.extract(cloud)
    bad = FCS.compare(dc, dd, info, fc.stages(), ref)
    assert not bad, bad
    return info, ref


def _rc(api, fc, cloud, cap=None, cap_down=None):
    """The raw call -> (rc, cloud buffer, down buffer, info): the buffers are NaN-filled to show that a refusal leaves them alone."""
    p = FCS.xyzw(cloud)
    n = len(p)
    cap = n if cap is None else cap
    cap_down = n if cap_down is None else cap_down
    oc, od, info = np.full((max(cap, 1), 3), np.nan, F), np.full((max(cap_down, 1), 3), np.nan, F), api.FrameCloudInfo()
    rc = api.lib().gfs_frame_cloud_extract(fc.h, p.ctypes.data, n, oc.ctypes.data, cap, od.ctypes.data, cap_down, C.byref(info))
    return rc, oc, od, api.frame_cloud_info(info)


# ------------------------------------------------------------------ split

@pytest.mark.parametrize("case", FCS.split_cases(), ids=lambda c: c[0])
def test_split(handles, case):
    name, cloud, kw = case
    info, ref = _check(handles(**kw), cloud, **kw)
    assert info["host_scan_split"] == 0
    if name == "grid_8x32":
        assert info["n_scans"] == 7  # the last row is never emitted
    if name == "rows_20_21_22":
        assert [int(c) for c in ref["scans"][:, 1]] == [21, 22, 40]
    if name == "one_row":
        assert info["n_scans"] == 0 and info["n_down"] == 0 and info["n_surf"] == 0 and info["n_edge"] == 0
    if name == "drifting_rows":
        assert info["n_scans"] >= 10 and len(set(int(c) for c in ref["scans"][:, 1])) <= 3
    if name.startswith("pads"):
        assert [int(c) for c in ref["scans"][:, 2]] == [0, 1, 2, 3]


# ------------------------------------------------------------------ pick

@pytest.mark.parametrize("case", FCS.pick_cases(), ids=lambda c: c[0])
def test_pick(handles, case):
    name, cloud, kw = case
    info, ref = _check(handles(**kw), cloud, **kw)
    assert info["n_scans"] == 1
    if name == "flat_plane":
        assert info["n_edge_raw"] == 0
    if name == "many_corners":
        assert info["n_edge_raw"] == 10
    if name == "suppressed_neighbours":
        assert info["n_edge_raw"] == 2  # positions 50 and 80; 53 and 47 lie within +-5 of the stronger pick
        assert sorted(float(x) for x in ref["edge_raw"][:, 0]) == [-1.5 + 50 / 32, -1.5 + 80 / 32]
    if name == "candidates_1024":
        assert info["n_edge_raw"] + info["n_surf_raw"] == 1024


def test_mirrored_scan_has_ties():
    """The mirrored case does tie: its sorted values come in equal pairs, so the order is std::sort's and nothing else's."""
    name, cloud, kw = [c for c in FCS.pick_cases() if c[0] == "mirrored_ties"][0]
    ref = FCS.restate(cloud, **kw)
    s = ref["surf_raw"]
    mirrored = sum(1 for i in range(len(s) - 1) if s[i, 0] == -s[i + 1, 0] and s[i, 2] == s[i + 1, 2] and s[i, 0] != 0)
    assert mirrored >= 20, mirrored


def test_scan_of_1025_candidates_refused(gpu_api, handles):
    fc = handles()
    rc, oc, od, _ = _rc(gpu_api, fc, FCS.too_long_cloud())
    assert rc == FCS.CAPACITY and np.isnan(oc).all() and np.isnan(od).all()
    assert FCS.restate(FCS.too_long_cloud())["rc"] == FCS.CAPACITY


# ------------------------------------------------------------------ radius filter

@pytest.mark.parametrize("case", FCS.radius_cases(), ids=lambda c: c[0])
def test_radius_filter(handles, case):
    name, xyz, r, min_pts = case
    fc = handles(max_points=4096, local_map_resolution=r)
    got = fc.radius_filter(xyz, min_pts)
    assert FCS.same_bits(got, FCS.restated_radius(xyz, r, min_pts))
    assert FCS.same_bits(got, FCS.radius_all_pairs(xyz, r, min_pts))
    if name == "all_removed":
        assert len(got) == 0
    if name == "none_removed":
        assert len(got) == len(xyz)
    if name.startswith("lattice"):
        assert 0 < len(got) < len(xyz)


def test_radius_equality_inside_the_chain(handles):
    """local_map_resolution 0.0625 and scan points on the 0.0625 lattice: d2 == r * r occurs between the voxel centroids."""
    k = np.arange(64)
    parts = [np.stack([(k - 32) * 0.0625, np.full(64, v * 0.0625), np.full(64, 2.0)], 1) for v in range(-3, 4)]
    cloud = FCS.xyzw(np.concatenate(parts + [np.array([[0.0, 1.0, 2.0]])]).astype(F))
    kw = dict(local_map_resolution=0.0625, downsize_resolution=0.0625)
    info, ref = _check(handles(**kw), cloud, **kw)
    assert info["n_scans"] == 7 and info["n_surf_voxel"] == info["n_surf_raw"] > 0  # every lattice point is its own voxel


# ------------------------------------------------------------------ whole call

@pytest.mark.parametrize("seed", range(20))
def test_scene_cloud(handles, seed):
    kw = dict(local_map_resolution=(0.05, 0.2)[seed % 2], downsize_resolution=(0.05, 0.1)[(seed // 2) % 2])
    info, ref = _check(handles(**kw), FCS.scene_cloud(seed), **kw)
    assert info["host_scan_split"] == 0 and info["n_scans"] > 100 and info["n_down"] > 0


@pytest.mark.parametrize("seed", range(10))
def test_small_grid(handles, seed):
    kw = dict(local_map_resolution=(0.05, 0.2)[seed % 2], downsize_resolution=(0.05, 0.1)[(seed // 2) % 2])
    info, ref = _check(handles(**kw), FCS.scene_cloud(100 + seed, 40, 30), **kw)
    assert info["host_scan_split"] == 0 and info["n_scans"] > 20


def test_extract_device_matches_extract(gpu_api, handles):
    """The cloud gfs_frame_rgbd leaves on the device gives the bytes of extract on its host copy."""
    from geoflowslam_amd import synth
    fp = synth.frame_pair(3, 160, 120, 1)
    fr = gpu_api.Frame(max_rows=120, max_cols=160, max_keypoints=16)
    kps = np.zeros(0, gpu_api.KP_DTYPE)
    fx, fy, cx, cy = (float(F(v)) for v in synth.intrinsics(160, 120))
    _, _, host, (dc, dn, stride, n) = fr.FrameRGBD(kps, fp["depth0"], 40.0, 1, fx, fy, cx, cy)
    fc = handles()
    a = fc.extract(host)
    sa = fc.stages()
    b = fc.extract_device(dc, dn, cap=n, cap_down=n)
    sb = fc.stages()
    assert a[2] == b[2] and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert all(sa[k].tobytes() == sb[k].tobytes() for k in sa)
    assert not FCS.compare(b[0], b[1], b[2], sb, FCS.restate(host))
    fr.close()


# ------------------------------------------------------------------ guard

@pytest.mark.parametrize("which", ["grid_8x32", "scene", "pads_H70.0"])
def test_guard_forces_host_split(handles, which):
    cloud = FCS.scene_cloud(1) if which == "scene" else [c for c in FCS.split_cases() if c[0] == which][0][1]
    d = handles().extract(cloud)
    sd = handles().stages()
    fh = handles(angle_guard_deg=0.06)
    g = fh.extract(cloud)
    sg = fh.stages()
    assert d[2]["host_scan_split"] == 0 and g[2]["host_scan_split"] == 1
    assert dict(g[2], host_scan_split=0) == d[2]
    assert d[0].tobytes() == g[0].tobytes() and d[1].tobytes() == g[1].tobytes()
    assert all(sd[k].tobytes() == sg[k].tobytes() for k in sd)


# ------------------------------------------------------------------ refusals and state

def test_refusals(gpu_api, handles):
    api, fc = gpu_api, handles()
    good = FCS.scene_cloud(100, 40, 30)
    fresh = api.FrameCloud(max_points=CAP)
    want = fresh.extract(good)
    fresh.close()

    def still_fresh():
        got = fc.extract(good)
        assert got[2] == want[2] and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()

    def refused(rc_want, cloud, **kw):
        rc, oc, od, _ = _rc(api, fc, cloud, **kw)
        assert rc == rc_want, (rc, rc_want)
        assert np.isnan(oc).all() and np.isnan(od).all(), "a refusal wrote to an output"
        still_fresh()

    refused(FCS.INVALID_ARG, np.zeros((0, 4), F))
    for bad in (np.nan, np.inf, -np.inf, 2.0e6):
        c = good.copy()
        c[len(c) // 2, 1] = bad
        refused(FCS.INVALID_ARG, c)
        assert FCS.restate(c)["rc"] == FCS.INVALID_ARG
    c = good.copy()
    c[7, :3] = 0.0  # the curvature divides by the squared norm
    refused(FCS.INVALID_ARG, c)
    refused(FCS.CAPACITY, np.tile(good, (CAP // len(good) + 1, 1)))
    refused(FCS.CAPACITY, FCS.too_long_cloud())
    # too small output buffers, on a configuration whose outputs are not empty
    kw = dict(local_map_resolution=0.2, downsize_resolution=0.1)
    fk, big = handles(**kw), FCS.scene_cloud(1)
    ref = FCS.restate(big, **kw)
    assert len(ref["cloud"]) > 1 and len(ref["down"]) > 1
    for caps in (dict(cap=len(ref["cloud"]) - 1), dict(cap_down=len(ref["down"]) - 1)):
        rc, oc, od, info = _rc(api, fk, big, **caps)
        assert rc == FCS.CAPACITY and np.isnan(oc).all() and np.isnan(od).all()
        assert info == ref["info"]  # the sizes a caller needs to come back with
        _check(fk, big, **kw)
    cfg = api.FrameCloudConfig()
    for field, v in (("local_map_resolution", 0.0), ("local_map_resolution", -0.05), ("local_map_resolution", np.inf),
                     ("downsize_resolution", 0.0), ("downsize_resolution", np.nan)):
        api.lib().gfs_frame_cloud_default_config(C.byref(cfg))
        setattr(cfg, field, v)
        hdl = C.c_void_p()
        assert api.lib().gfs_frame_cloud_create(0, 1024, C.byref(cfg), C.byref(hdl)) == FCS.INVALID_ARG and not hdl.value


def test_unsupported_voxel_range(gpu_api):
    """Points 1290 leaves apart on every axis: PCL's int64 cell count passes (1290^3 <= INT32_MAX), its int arithmetic (1291^3) not."""
    k = np.arange(30)
    a = np.stack([0.9 + 1e-3 * k, np.full(30, 0.9), np.full(30, 0.9 + 1.0)], 1)
    b = np.stack([1290.1 + 1e-3 * k, np.full(30, 1290.1), np.full(30, 1290.1 + 1.0)], 1)
    cloud = FCS.xyzw(np.concatenate([a, b, [[0.0, -5.0, 1.0]]]).astype(F))
    kw = dict(local_map_resolution=2.0, downsize_resolution=1.0, horizontal_angle=300.0)
    ref = FCS.restate(cloud, **kw)
    fc = gpu_api.FrameCloud(max_points=1024, **kw)
    rc, oc, od, _ = _rc(gpu_api, fc, cloud)
    fc.close()
    assert ref["rc"] == FCS.UNSUPPORTED and rc == FCS.UNSUPPORTED and np.isnan(oc).all() and np.isnan(od).all()


def test_repeat_and_mixed_sizes(handles):
    fc = handles()
    big, small = FCS.scene_cloud(2), FCS.scene_cloud(102, 40, 30)
    first = fc.extract(big)
    for _ in range(2):
        again = fc.extract(big)
        assert again[2] == first[2] and again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes()
    _check(fc, small)
    _check(fc, big)
