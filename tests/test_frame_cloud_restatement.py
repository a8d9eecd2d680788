"""The frame cloud's sequential restatement (tests/host/frame_cloud_restatement.cpp) against an independent numpy statement of
DESIGN.md section 17, bit for bit, on the constructed clouds of frame_cloud_support and on small random grid clouds.  The numpy
statement sorts stably; where curvature values tie (the mirrored scan) the order is std::sort's, which numpy cannot know, so there the
comparison is on what no tie order changes in these cases (tied strong points lie more than 5 apart): the edge points and the surf
points as multisets."""
import math

import numpy as np
import pytest

import frame_cloud_support as FCS

F, D = np.float32, np.float64


def np_voxel(p, leaf):
    """DESIGN.md section 11 -> (points, passthrough)."""
    p = np.asarray(p, F).reshape(-1, 3)
    if len(p) == 0:
        return p, 0
    inv = F(1.0) / F(leaf)
    mn, mx = p.min(0), p.max(0)
    cells = 1
    for a in range(3):
        fd = F(mx[a] - mn[a]) * inv
        if not fd < F(2147483648.0):
            return p, 1
        cells *= int(fd) + 1
        if cells > 2147483647:
            return p, 1
    lo = np.floor(mn * inv).astype(np.int64)
    div = np.floor(mx * inv).astype(np.int64) - lo + 1
    ijk = (np.floor(p * inv) - lo.astype(F)).astype(np.int64)
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    order = np.argsort(idx, kind="stable")
    out = []
    j = 0
    while j < len(p):
        e = j
        s = np.zeros(3, F)
        while e < len(p) and idx[order[e]] == idx[order[j]]:
            s = (s + p[order[e]]).astype(F)
            e += 1
        out.append(s / F(e - j))
        j = e
    return np.array(out, F).reshape(-1, 3), 0


def np_frame_cloud(cloud, horizontal_angle=70.0, max_distance=9.0, local_map_resolution=0.05, downsize_resolution=0.05):
    p = np.asarray(cloud, F)[:, :3]
    n = len(p)
    deg = lambda a, b: math.atan2(float(a), float(b)) * 180 / math.pi
    scans, table = [], []
    last, count, cand = deg(p[0, 1], p[0, 2]), 0, 0
    for i in range(n):
        ang = deg(p[i, 1], p[i, 2])
        if abs(ang - last) > 0.05:
            if count > 20:
                first, end, pad, s = p[i - count], p[i - 1], 0, []
                if deg(first[0], first[2]) > -horizontal_angle / 2.0 + 5.0:
                    pad |= 1
                    s += [[first[0], first[1], F(max_distance)]] * 5
                s += p[i - count:i].tolist()
                if deg(end[0], end[2]) < horizontal_angle / 2.0 - 5.0:
                    pad |= 2
                    s += [[end[0], end[1], F(max_distance)]] * 5
                table.append([i - count, count, pad, cand])
                cand += len(s) - 10
                scans.append(np.array(s, F))
            count, last = 0, ang
        count += 1
    edge_raw, surf_raw, ties = [], [], False
    for s in scans:
        m = len(s)
        ids = np.arange(5, m - 5)
        diff = np.zeros((len(ids), 3), F)
        for k in (-5, -4, -3, -2, -1):
            diff = (diff + s[ids + k]).astype(F) if k > -5 else s[ids + k].copy()
        diff = (diff - (F(10) * s[ids]).astype(F)).astype(F)
        for k in (1, 2, 3, 4, 5):
            diff = (diff + s[ids + k]).astype(F)
        q = s[ids]
        pd = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]).astype(F) + q[:, 2] * q[:, 2]).astype(F).astype(D)
        d = diff.astype(D)
        val = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] / pd
        ties = ties or len(np.unique(val)) < len(val)
        order = np.argsort(val, kind="stable")
        picked, is_edge, picks = np.zeros(m, bool), np.zeros(m, bool), 0
        for i in order[::-1]:
            j = ids[i]
            if picked[j]:
                continue
            if val[i] <= 0.1:
                break
            picks += 1
            picked[j] = True
            if picks > 10:
                break
            is_edge[j] = True
            edge_raw.append(s[j])
            picked[j - 5:j + 6] = True
        surf_raw += [s[ids[i]] for i in order if not is_edge[ids[i]]]
    A = lambda l: np.array(l, F).reshape(-1, 3)
    out = dict(scans=np.array(table, np.int32).reshape(-1, 4), edge_raw=A(edge_raw), surf_raw=A(surf_raw), ties=ties)
    r = local_map_resolution
    out["edge_voxel"], p0 = np_voxel(out["edge_raw"], F(r / 4.0))
    out["surf_voxel"], p1 = np_voxel(out["surf_raw"], F(r / 2.0))
    out["edge"] = FCS.radius_all_pairs(out["edge_voxel"], r, 3)
    out["surf"] = FCS.radius_all_pairs(out["surf_voxel"], r, 14)
    out["cloud"] = np.concatenate([out["surf"], out["edge"]])
    out["down"], p2 = np_voxel(out["cloud"], F(downsize_resolution))
    out["passthrough"] = (p0, p1, p2)
    return out


def _compare(cloud, **kw):
    ref, me = FCS.restate(cloud, **kw), np_frame_cloud(cloud, **kw)
    assert ref["rc"] == FCS.OK
    assert ref["scans"].tobytes() == me["scans"].tobytes()
    if me["ties"]:
        canon = lambda a: sorted(map(tuple, np.asarray(a, F).view(np.uint32).tolist()))
        assert canon(ref["edge_raw"]) == canon(me["edge_raw"]) and canon(ref["surf_raw"]) == canon(me["surf_raw"])
        return ref, me
    for k in FCS.STAGES:
        assert FCS.same_bits(ref[k], me[k]), k
    assert ref["info"]["passthrough"] == me["passthrough"]
    assert [ref["info"]["n_" + k] for k in ("edge_raw", "surf_raw", "edge_voxel", "surf_voxel", "edge", "surf", "down")] == \
        [len(me[k]) for k in ("edge_raw", "surf_raw", "edge_voxel", "surf_voxel", "edge", "surf", "down")]
    return ref, me


@pytest.mark.parametrize("case", FCS.split_cases() + FCS.pick_cases(), ids=lambda c: c[0])
def test_constructed(case):
    name, cloud, kw = case
    ref, me = _compare(cloud, **kw)
    assert me["ties"] or name not in ("mirrored_ties", "flat_plane")  # (a plane's curvatures are rounding residue: many are equal)


@pytest.mark.parametrize("seed", range(5))
def test_random_grid(seed):
    cloud = FCS.grid_cloud(40 + seed, 36 + 3 * seed, 12, noise=0.02)
    kw = dict(local_map_resolution=(0.05, 0.2)[seed % 2], downsize_resolution=(0.05, 0.1)[seed % 2])
    ref, me = _compare(cloud, **kw)
    assert ref["info"]["n_scans"] == 11 and ref["info"]["n_edge_raw"] > 0


@pytest.mark.parametrize("case", FCS.radius_cases(), ids=lambda c: c[0])
def test_radius_rule(case):
    name, xyz, r, min_pts = case
    assert FCS.same_bits(FCS.restated_radius(xyz, r, min_pts), FCS.radius_all_pairs(xyz, r, min_pts))


def test_voxel_of_empty_cloud_is_empty():
    n, out, passthrough = FCS.restated_voxel(np.zeros((0, 3), F), 0.05)
    assert n == 0 and passthrough == 0


def test_refusals():
    good = FCS.grid_cloud(3, 32, 8)
    assert FCS.restate(np.zeros((0, 4), F))["rc"] == FCS.INVALID_ARG
    for bad in (np.nan, np.inf, 2.0e6):
        c = good.copy()
        c[5, 2] = bad
        assert FCS.restate(c)["rc"] == FCS.INVALID_ARG
    assert FCS.restate(good, local_map_resolution=0.0)["rc"] == FCS.INVALID_ARG
    assert FCS.restate(good, downsize_resolution=-1.0)["rc"] == FCS.INVALID_ARG
    assert FCS.restate(FCS.too_long_cloud())["rc"] == FCS.CAPACITY
