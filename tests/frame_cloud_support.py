"""Shared by the frame-cloud tests: builds and calls the sequential CPU restatement (tests/host/frame_cloud_restatement.cpp) and
makes the constructed clouds of DESIGN.md section 17's test list.  Not a test module."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from geoflowslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "frame_cloud_restatement.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_frame_cloud_restatement.so")
_L = None

OK, INVALID_ARG, CAPACITY, UNSUPPORTED = 0, -1, -4, -5
F = np.float32
STAGES = ("edge_raw", "surf_raw", "edge_voxel", "surf_voxel", "edge", "surf", "cloud", "down")
INFO = ("n_in", "n_scans", "n_edge_raw", "n_surf_raw", "n_edge_voxel", "n_surf_voxel", "n_edge", "n_surf", "n_down", "host_scan_split")
DEFAULTS = dict(horizontal_angle=70.0, max_distance=9.0, local_map_resolution=0.05, downsize_resolution=0.05)


def restatement():
    global _L
    if _L is None:
        if not os.path.exists(_SO) or os.path.getmtime(_SO) < os.path.getmtime(_SRC):
            tmp = _SO + f".{os.getpid()}.tmp"
            subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", tmp, _SRC], check=True)
            os.replace(tmp, _SO)
        L = C.CDLL(_SO)
        vp, i, d, f = C.c_void_p, C.c_int, C.c_double, C.c_float
        L.fcr_run.argtypes = [vp, i, d, d, d, f]
        L.fcr_count.argtypes = [i]
        L.fcr_points.argtypes = [i, vp]
        L.fcr_scans.argtypes = [vp]
        L.fcr_info.argtypes = [vp]
        L.fcr_voxel.argtypes = [vp, i, f, vp, vp]
        L.fcr_radius.argtypes = [vp, i, d, i, vp]
        _L = L
    return _L


def xyzw(points):
    """[n][3] or [n][4] -> contiguous float32 [n][4] (w = 1, as ConvertDepthToPointCloud writes it)."""
    p = np.asarray(points, F)
    p = p.reshape(-1, p.shape[-1] if p.ndim == 2 else 4)
    if p.shape[1] == 3:
        p = np.concatenate([p, np.ones((len(p), 1), F)], 1)
    return np.ascontiguousarray(p, F)


def config(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    return c


def restate(points, **kw):
    """The restatement of one cloud -> dict(rc, info, scans [n_scans][4], and every stage [n][3])."""
    L, c, p = restatement(), config(**kw), xyzw(points)
    rc = L.fcr_run(p.ctypes.data, len(p), c["horizontal_angle"], c["max_distance"], c["local_map_resolution"],
                   float(F(c["downsize_resolution"])))
    out = dict(rc=rc)
    info = np.zeros(13, np.int32)
    L.fcr_info(info.ctypes.data)
    out["info"] = dict(zip(INFO, (int(v) for v in info[:10])), passthrough=tuple(int(v) for v in info[10:]))
    scans = np.zeros((max(L.fcr_scan_count(), 1), 4), np.int32)
    L.fcr_scans(scans.ctypes.data)
    out["scans"] = scans[:L.fcr_scan_count()]
    for s, name in enumerate(STAGES):
        a = np.zeros((max(L.fcr_count(s), 1), 3), F)
        L.fcr_points(s, a.ctypes.data)
        out[name] = a[:L.fcr_count(s)]
    return out


def restated_radius(xyz, r, min_pts):
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    out = np.zeros((max(len(xyz), 1), 3), F)
    n = restatement().fcr_radius(xyz.ctypes.data, len(xyz), float(r), min_pts, out.ctypes.data)
    return out[:n].copy()


def restated_voxel(xyz, leaf):
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    out, p = np.zeros((max(len(xyz), 1), 3), F), C.c_int()
    n = restatement().fcr_voxel(xyz.ctypes.data, len(xyz), float(F(leaf)), out.ctypes.data, C.byref(p))
    return n, out[:max(n, 0)].copy(), p.value


def radius_all_pairs(xyz, r, min_pts):
    """The radius rule over all pairs in numpy: float d2 = (dx*dx + dy*dy) + dz*dz, (double)d2 <= r*r, self excluded."""
    p = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    d = p[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == F
    within = d2.astype(np.float64) <= float(r) * float(r)
    return p[(within.sum(1) - 1) >= min_pts]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ constructed clouds

def row(v_deg, h_deg, z):
    """One image row as the depth cloud has it: a constant y / z (up to float rounding), x / z = tan(h)."""
    h, z = np.asarray(h_deg, np.float64), np.asarray(z, np.float64) * np.ones(len(h_deg))
    return np.stack([z * np.tan(np.radians(h)), z * np.tan(np.radians(v_deg)), z], 1).astype(F)


def rows(specs, closing=True):
    """specs: [(v_deg, h_deg array, z array or scalar)] -> cloud; closing: one more point below, so that the last row is a scan
    (the run open at the end of the cloud is never emitted)."""
    parts = [row(*s) for s in specs]
    if closing:
        parts.append(row(specs[-1][0] + 1.0, [0.0], 2.0))
    return xyzw(np.concatenate(parts))


def grid_cloud(seed, width, height, fx=None, z0=2.0, noise=0.01, keep=None):
    """A width x height pinhole cloud in raster order (x = (u - cx) z / fx, y = (v - cy) z / fx), depth z0 + a slope + noise;
    keep [height][width] bool drops pixels (invalid depth)."""
    rng = np.random.default_rng(seed)
    fx = F(fx if fx is not None else width * 0.8)
    u, v = np.meshgrid(np.arange(width, dtype=F), np.arange(height, dtype=F))
    z = (z0 + 0.3 * u / width + 0.2 * v / height + noise * rng.standard_normal((height, width))).astype(F)
    z[:, width // 3] += F(0.4)  # a depth step: edge points
    x, y = (u - F(width / 2)) * z / fx, (v - F(height / 2)) * z / fx
    p = np.stack([x, y, z], -1).astype(F)
    if keep is not None:
        return xyzw(p[keep])
    return xyzw(p.reshape(-1, 3))


def split_cases():
    rng = np.random.default_rng(5)
    out = [("grid_8x32", grid_cloud(1, 32, 8), {})]
    h = lambda n, a=-10.0, b=10.0: np.linspace(a, b, n)
    zz = lambda n: 2.0 + 0.02 * rng.standard_normal(n)
    out.append(("rows_20_21_22", rows([(-2.0, h(20), zz(20)), (-1.0, h(21), zz(21)), (0.0, h(22), zz(22)), (1.0, h(40), zz(40))]), {}))
    keep = rng.uniform(size=(10, 48)) > 0.3
    keep[4, :] = False
    keep[6, 30:] = False  # a row of 30 valid pixels at most
    out.append(("invalid_pixels", grid_cloud(2, 48, 10, keep=keep), {}))
    out.append(("one_row", rows([(0.0, h(64), zz(64))], closing=False), {}))
    # y / z drifts by 0.0011 degrees a point: the breaks fall where the chain puts them, every ~46 points
    n = 600
    v = -0.3 + 0.0011 * np.arange(n)
    z = 2.0 + 0.02 * rng.standard_normal(n)
    hh = np.tile(np.linspace(-12.0, 12.0, 60), 10)
    p = np.stack([z * np.tan(np.radians(hh)), z * np.tan(np.radians(v)), z], 1)
    out.append(("drifting_rows", xyzw(p), {}))
    for H in (70.0, 91.2):
        t = H / 2.0 - 5.0
        specs = []
        for k, (a, b) in enumerate([(-t - 1.0, t + 1.0), (-t + 1.0, t + 1.0), (-t - 1.0, t - 1.0), (-t + 1.0, t - 1.0)]):
            specs.append((float(k), np.linspace(a, b, 70), zz(70)))
        out.append((f"pads_H{H}", rows(specs), dict(horizontal_angle=H)))
    return out


def _exact_row(z, x0=-1.0, dx=1.0 / 32):
    """A row at y = 0 (angle 0 exactly) with dyadic coordinates: every float sum of the curvature is exact."""
    z = np.asarray(z, np.float64)
    x = x0 + dx * np.arange(len(z))
    return np.stack([x, np.zeros(len(z)), z], 1).astype(F)


def _close(p):
    return xyzw(np.concatenate([p, row(1.0, [0.0], 2.0)]))


def pick_cases():
    out = []
    n = 120
    x = np.linspace(-1.4, 1.4, n)  # beyond +-30 degrees at z = 2: no pads, and a plane has no curvature
    out.append(("flat_plane", _close(np.stack([x, np.zeros(n), np.full(n, 2.0)], 1).astype(F)), {}))
    z = np.full(200, 2.0)
    z[10:190:13] += 0.5 + 0.01 * np.arange(len(z[10:190:13]))  # 14 separated corners, all strong
    out.append(("many_corners", _close(_exact_row(z, -3.125)), {}))
    z = np.full(100, 2.0)
    z[50] += 1.0
    z[53] += 0.5  # within +-5 of the stronger pick: suppressed
    z[47] += 0.375
    z[80] += 0.25
    out.append(("suppressed_neighbours", _close(_exact_row(z, -1.5)), {}))
    m = 81  # mirrored about its centre: x -> -x, z symmetric; exact sums, so the values tie in pairs
    k = np.arange(m) - m // 2
    z = 2.0 + np.abs(k) / 64.0
    z[[m // 2 - 20, m // 2 + 20]] += 0.5
    z[[m // 2 - 7, m // 2 + 7]] += 0.25
    out.append(("mirrored_ties", _close(np.stack([k / 64.0, np.zeros(m), z], 1).astype(F)), {}))
    rng = np.random.default_rng(9)
    z = 2.0 + rng.integers(0, 8, 1024) / 64.0  # both pads (|h| small): 1024 candidates
    out.append(("candidates_1024", _close(_exact_row(z, -0.5, 1.0 / 1024)), {}))
    return out


def too_long_cloud():
    rng = np.random.default_rng(10)
    return _close(_exact_row(2.0 + rng.integers(0, 8, 1025) / 64.0, -0.5, 1.0 / 1024))


def radius_cases():
    """[(name, xyz [n][3], r, min_pts)] for the radius filter on its own: <= 2000 points each."""
    rng = np.random.default_rng(21)
    out = []
    g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    lat = (g[rng.uniform(size=len(g)) > 0.45] * 0.0625).astype(F)  # d2 == r * r exactly between lattice neighbours
    out.append(("lattice_equal_r2", lat, 0.0625, 3))
    full = (g * 0.0625).astype(F)  # an inner point has 6 lattice neighbours at exactly r and 8 of the shifted lattice inside: 14
    out.append(("lattice_equal_r2_14", np.concatenate([full, full + F(0.03125)]), 0.0625, 14))
    p = rng.uniform(-0.4, 0.4, (500, 3)).astype(F)
    out.append(("duplicates", np.concatenate([p, p[::2], p[:100], p[:100]]), 0.05, 3))
    out.append(("all_removed", (rng.permutation(1000)[:, None] * np.array([0.2, 0.0, 0.1]) + rng.uniform(0, 0.01, (1000, 3))).astype(F), 0.05, 3))
    out.append(("none_removed", (F(100.0) + rng.uniform(0, 0.05, (800, 3))).astype(F), 0.1, 14))
    out.append(("far_and_negative", (rng.uniform(-0.08, 0.08, (1500, 3)) + [-5.0e3, 7.0e3, -0.01]).astype(F), 0.05, 14))
    return out


@functools.lru_cache(maxsize=None)
def scene_cloud(seed, width=160, height=120):
    """synth.frame_pair's first cloud at stride 1: ~ width * height points in raster order."""
    return xyzw(synth.frame_pair(seed, width, height, 1)["cloud0"])


def compare(dev_cloud, dev_down, dev_info, dev_stages, ref):
    """Every stage, both outputs and every info field against the restatement; returns the list of what differs."""
    bad = []
    if dev_info != ref["info"]:
        bad.append(("info", dev_info, ref["info"]))
    if dev_stages is not None:
        if dev_stages["scans"].tobytes() != ref["scans"].tobytes():
            bad.append("scans")
        for k in STAGES[:6]:
            if not same_bits(dev_stages[k], ref[k]):
                bad.append(k)
    if dev_cloud is not None and not same_bits(dev_cloud, ref["cloud"]):
        bad.append("cloud")
    if not same_bits(dev_down, ref["down"]):
        bad.append("down")
    return bad
