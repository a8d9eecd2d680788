"""Seeded synthetic RGB-D inputs for tests and bench (SURVEY.md §8(d) "Synthetic inputs").

A tiny analytic ray-caster: a room (floor + two walls) and a few axis-aligned boxes, textured with a
procedural multi-scale checker so that FAST corners exist at every pyramid level and so that two views
of the same scene are photo-consistent (ORB matches and GICP have a true answer).  Harness code only —
nothing here is part of the hot path.
"""
import numpy as np


def intrinsics(width, height):
    """fx=fy=607 for VGA, 910 for 720p (script/run_orbslam/RGBD-Inertial/config/g1_op_icp_lidar_indoor1.yaml:25-34)."""
    f = 607.0 * width / 640.0
    return f, f, (width - 1) / 2.0, (height - 1) / 2.0


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def random_motion(rng, trans=0.03, rot_deg=1.5):
    """SE(3) T_world_cam of the second view: t ~ U(-3,3) cm, r ~ U(-1.5,1.5) deg per axis."""
    T = np.eye(4)
    T[:3, :3] = _rot(*(np.deg2rad(rot_deg) * rng.uniform(-1, 1, 3)))
    T[:3, 3] = trans * rng.uniform(-1, 1, 3)
    return T


class Scene:
    def __init__(self, seed):
        rng = np.random.default_rng(seed)
        self.seed = int(seed)
        # planes: (normal, offset) with n.p = d ; camera looks along +z, y down
        self.planes = [
            (np.array([0.0, 1.0, 0.0]), 1.3 + 0.3 * rng.random()),   # floor (y = +h below the camera)
            (np.array([0.0, 0.0, 1.0]), 4.0 + 1.8 * rng.random()),   # front wall
            (np.array([1.0, 0.0, 0.0]), -(2.0 + 1.0 * rng.random())),  # left wall x = -a
        ]
        self.boxes = []
        for _ in range(5):
            c = np.array([rng.uniform(-1.5, 2.0), rng.uniform(0.2, 1.0), rng.uniform(1.5, 3.8)])
            h = np.array([rng.uniform(0.15, 0.5), rng.uniform(0.15, 0.5), rng.uniform(0.15, 0.4)])
            self.boxes.append((c - h, c + h))
        nsurf = 3 + 6 * 5
        self.freq = rng.uniform(2.5, 9.0, (nsurf, 3, 2)).astype(np.float32)
        self.phase = rng.uniform(0, 6.28, (nsurf, 3, 2)).astype(np.float32)
        self.amp = rng.uniform(15, 45, (nsurf, 3)).astype(np.float32)
        self.base = rng.uniform(70, 180, nsurf).astype(np.float32)

    def render(self, width, height, T_wc=None, noise_seed=0, depth_noise=0.002, invalid_frac=0.02):
        """-> gray u8 [H,W], depth f32 [H,W] (metres, 0 = invalid)."""
        fx, fy, cx, cy = intrinsics(width, height)
        T = np.eye(4) if T_wc is None else T_wc
        R, t = T[:3, :3].astype(np.float32), T[:3, 3].astype(np.float32)
        u, v = np.meshgrid(np.arange(width, dtype=np.float32), np.arange(height, dtype=np.float32))
        dc = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1).reshape(-1, 3)
        d = dc @ R.T
        o = t
        n = d.shape[0]
        best = np.full(n, np.inf, np.float32)
        sid = np.zeros(n, np.int32)
        uv = np.zeros((n, 2), np.float32)

        def consider(tt, mask, s, ucoord, vcoord):
            nonlocal best, sid, uv
            m = mask & (tt > 0.05) & (tt < best)
            best = np.where(m, tt, best)
            sid = np.where(m, s, sid)
            uv[m, 0] = ucoord[m]
            uv[m, 1] = vcoord[m]

        s = 0
        for nrm, off in self.planes:
            denom = d @ nrm.astype(np.float32)
            with np.errstate(divide="ignore", invalid="ignore"):
                tt = (off - o @ nrm.astype(np.float32)) / denom
            p = o + d * tt[:, None]
            ax = [i for i in range(3) if abs(nrm[i]) < 0.5]
            consider(tt, np.isfinite(tt), s, p[:, ax[0]], p[:, ax[1]])
            s += 1
        for lo, hi in self.boxes:
            lo = lo.astype(np.float32)
            hi = hi.astype(np.float32)
            for axis in range(3):
                for side, val in ((0, lo[axis]), (1, hi[axis])):
                    with np.errstate(divide="ignore", invalid="ignore"):
                        tt = (val - o[axis]) / d[:, axis]
                    p = o + d * tt[:, None]
                    oth = [i for i in range(3) if i != axis]
                    inside = (np.isfinite(tt) & (p[:, oth[0]] >= lo[oth[0]]) & (p[:, oth[0]] <= hi[oth[0]])
                              & (p[:, oth[1]] >= lo[oth[1]]) & (p[:, oth[1]] <= hi[oth[1]]))
                    consider(tt, inside, s, p[:, oth[0]], p[:, oth[1]])
                    s += 1
        hit = np.isfinite(best)
        f, ph, am = self.freq[sid], self.phase[sid], self.amp[sid]
        val = self.base[sid].copy()
        for k in range(3):
            val += am[:, k] * np.sign(np.sin(f[:, k, 0] * (2.0 ** k) * uv[:, 0] + ph[:, k, 0])
                                      * np.sin(f[:, k, 1] * (2.0 ** k) * uv[:, 1] + ph[:, k, 1]))
        rng = np.random.default_rng((self.seed * 7919 + noise_seed) & 0x7FFFFFFF)
        val = np.where(hit, val, 20.0) + rng.integers(-2, 3, n)
        gray = np.clip(np.rint(val), 0, 255).astype(np.uint8).reshape(height, width)
        z = (best * dc[:, 2]).astype(np.float32)  # depth along the optical axis (dc.z == 1)
        z = z + rng.normal(0, depth_noise, n).astype(np.float32)
        z = np.where(hit & (z > 0.3) & (z < 9.5), z, 0).astype(np.float32)
        z[rng.random(n) < invalid_frac] = 0
        return gray, z.reshape(height, width)


def depth_to_cloud(depth, stride, width=None, height=None):
    """Frame::ConvertDepthToPointCloud (reference src/Frame.cc:590-623): pixels on a stride grid with
    0 < d < 10 -> (x, y, z, 1) float32 in the camera frame. Returns [N,4] float32."""
    h, w = depth.shape
    fx, fy, cx, cy = intrinsics(w, h)
    vs, us = np.meshgrid(np.arange(0, h, stride), np.arange(0, w, stride), indexing="ij")
    d = depth[vs, us]
    m = (d > 0) & (d < 10)
    d = d[m].astype(np.float32)
    x = ((us[m].astype(np.float32) - np.float32(cx)) * d / np.float32(fx)).astype(np.float32)
    y = ((vs[m].astype(np.float32) - np.float32(cy)) * d / np.float32(fy)).astype(np.float32)
    return np.stack([x, y, d, np.ones_like(d)], -1).astype(np.float32)


def frame_pair(seed, width=640, height=480, stride=4):
    """-> dict(gray0, depth0, gray1, depth1, cloud0, cloud1, T_01) where T_01 maps frame-1 points into
    frame 0 (= T_target_source for GICP with target = previous frame, source = current frame,
    reference src/Tracking.cc:3375-3382)."""
    sc = Scene(seed)
    rng = np.random.default_rng(seed + 0x6F5)
    T1 = random_motion(rng)
    g0, d0 = sc.render(width, height, None, 0)
    g1, d1 = sc.render(width, height, T1, 1)
    return dict(gray0=g0, depth0=d0, gray1=g1, depth1=d1, cloud0=depth_to_cloud(d0, stride),
                cloud1=depth_to_cloud(d1, stride), T_01=T1)


def noise_image(seed, width, height):
    """Unstructured test image: smooth background + rectangles + noise (lots of corners)."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(60, 190) + 25 * np.sin(np.linspace(0, 6, width))[None, :] * np.cos(np.linspace(0, 4, height))[:, None]
    for _ in range(max(40, width * height // 800)):
        x0, y0 = rng.integers(0, width), rng.integers(0, height)
        w, h = rng.integers(4, 60), rng.integers(4, 60)
        img[y0:y0 + h, x0:x0 + w] += rng.uniform(30, 120) * rng.choice([-1, 1])
    img += rng.integers(-2, 3, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _quat_from_R(R):
    from scipy.spatial.transform import Rotation
    q = Rotation.from_matrix(R).as_quat()  # x, y, z, w
    return q if q[3] >= 0 else -q


def lba_window(seed, n_free=20, n_fixed=5, n_points=3000, mono_frac=0.1, outlier_frac=0.03):
    """Synthetic LocalBundleAdjustment window (BASELINE.json configs[4]): key-frames on a 2 m arc
    looking at `n_points` points in a 6x4x3 m box; every point is observed by every key-frame whose frustum contains it;
    RGB-D ("stereo", 3-D) edges, a fraction without depth (mono, 2-D); pixel noise sigma = sqrt(sigma2[octave]);
    3 % gross outliers (20 px); key-frame poses perturbed by 1 cm / 0.3 deg, points by 2 cm.
    Returns a dict of flat arrays matching gfs_lba_problem (include/gfs_abi.h) plus the ground truth."""
    rng = np.random.default_rng(seed)
    fx = fy = np.float64(np.float32(607.0))
    cx, cy = np.float64(np.float32(319.5)), np.float64(np.float32(239.5))
    bf = np.float64(np.float32(0.0745 * 607.0))
    n_poses = n_free + n_fixed
    pts = np.c_[rng.uniform(-3, 3, n_points), rng.uniform(-2, 2, n_points), rng.uniform(3.0, 6.0, n_points)]
    Rs, ts = [], []
    for i in range(n_poses):
        a = (i / max(n_poses - 1, 1) - 0.5) * 0.8  # arc angle
        c = np.array([2.0 * np.sin(a), 0.05 * rng.normal(), 2.0 - 2.0 * np.cos(a)])  # camera centre (world)
        Rwc = _rot(0.02 * rng.normal(), -a + 0.02 * rng.normal(), 0.02 * rng.normal())
        Rcw = Rwc.T
        Rs.append(Rcw)
        ts.append(-Rcw @ c)
    sigma2 = np.float64(np.float32(1.2) ** (2 * np.arange(8))).astype(np.float64)
    inv_sigma2 = np.float64(np.float32(1.0) / np.float32(1.2) ** (2 * np.arange(8)))
    e_pose, e_point, e_obs, e_is2, e_stereo = [], [], [], [], []
    for j in range(n_points):  # point-major edge order like the reference (src/Optimizer.cc:1816-1952)
        for i in range(n_poses):
            xc = Rs[i] @ pts[j] + ts[i]
            if xc[2] < 0.3:
                continue
            u, v = fx * xc[0] / xc[2] + cx, fy * xc[1] / xc[2] + cy
            if not (0 <= u < 640 and 0 <= v < 480):
                continue
            octv = int(rng.choice(8, p=np.array([217, 181, 151, 126, 105, 87, 73, 60]) / 1000.0))
            s = np.sqrt(sigma2[octv])
            noise = rng.normal(0, s, 3)
            if rng.random() < outlier_frac:
                noise[:2] += rng.choice([-1, 1], 2) * 20.0
            stereo = rng.random() >= mono_frac
            ur = u - bf / xc[2]
            e_pose.append(i)
            e_point.append(j)
            e_obs.append([np.float32(u + noise[0]), np.float32(v + noise[1]), np.float32(ur + noise[2]) if stereo else -1.0])
            e_is2.append(inv_sigma2[octv])
            e_stereo.append(1 if stereo else 0)
    fixed = np.zeros(n_poses, np.uint8)
    fixed[n_free:] = 1
    fixed[0] = 1 if n_fixed == 0 else fixed[0]
    q_gt = np.array([_quat_from_R(R) for R in Rs])
    t_gt = np.array(ts)
    q0, t0 = q_gt.copy(), t_gt.copy()
    for i in range(n_poses):
        if fixed[i]:
            continue
        dR = _rot(*(np.deg2rad(0.3) * rng.normal(size=3)))
        q0[i] = _quat_from_R(dR @ Rs[i])
        t0[i] = dR @ ts[i] + 0.01 * rng.normal(size=3)
    # the reference stores poses / points as float and widens them (src/Optimizer.cc:1692-1694, 1821)
    q0 = q0.astype(np.float32).astype(np.float64)
    t0 = t0.astype(np.float32).astype(np.float64)
    p0 = (pts + 0.02 * rng.normal(size=pts.shape)).astype(np.float32).astype(np.float64)
    return dict(n_poses=n_poses, n_points=n_points, n_edges=len(e_pose), pose_q=np.ascontiguousarray(q0),
                pose_t=np.ascontiguousarray(t0), pose_fixed=fixed, points=np.ascontiguousarray(p0),
                edge_pose=np.array(e_pose, np.int32), edge_point=np.array(e_point, np.int32),
                edge_obs=np.array(e_obs, np.float64), edge_inv_sigma2=np.array(e_is2, np.float64),
                edge_stereo=np.array(e_stereo, np.uint8), fx=fx, fy=fy, cx=cx, cy=cy, bf=bf,
                huber_mono=float(np.float32(np.sqrt(5.991))), huber_stereo=float(np.float32(np.sqrt(7.815))),
                iterations=10, gt_q=q_gt, gt_t=t_gt, gt_points=pts)


def gba_map(seed, n_keyframes, n_points, mono_frac=0.1, outlier_frac=0.03, step=0.5, fixed=()):
    """Synthetic map for GlobalBundleAdjustment: key-frames `step` metres apart along a corridor, looking sideways at `n_points`
    points on a band 3 - 6 m away, so that a point is seen only by the ten-odd key-frames whose frustum passes it and most pairs
    of key-frames share nothing (lba_window is fully covisible).  Key-frame 0 is fixed (pKF->mnId == pMap->GetInitKFid(),
    src/Optimizer.cc:121) plus the indices in `fixed`; RGB-D edges with a fraction `mono_frac` of mono ones, pixel noise, gross
    outliers, float-then-widened perturbed initial values: all as in lba_window.  Point-major edge order.  Every point has at
    least one observation.  Returns lba_window's dict."""
    rng = np.random.default_rng(seed)
    fx = fy = np.float64(np.float32(607.0))
    cx, cy = np.float64(np.float32(319.5)), np.float64(np.float32(239.5))
    bf = np.float64(np.float32(0.0745 * 607.0))
    length = step * max(n_keyframes - 1, 1)
    pts = np.c_[np.sort(rng.uniform(-1.0, length + 1.0, n_points)), rng.uniform(-1.5, 1.5, n_points), rng.uniform(3.0, 6.0, n_points)]
    Rs, ts = [], []
    for i in range(n_keyframes):
        c = np.array([step * i + 0.02 * rng.normal(), 0.05 * rng.normal(), 0.02 * rng.normal()])
        Rcw = _rot(0.02 * rng.normal(), 0.05 * rng.normal(), 0.02 * rng.normal()).T
        Rs.append(Rcw)
        ts.append(-Rcw @ c)
    sigma2 = np.float64(np.float32(1.2) ** (2 * np.arange(8))).astype(np.float64)
    inv_sigma2 = np.float64(np.float32(1.0) / np.float32(1.2) ** (2 * np.arange(8)))
    cols = dict(pose=[], point=[], obs=[], is2=[], stereo=[])
    for i in range(n_keyframes):  # the points within reach of key-frame i (pts is sorted by x)
        c_x = step * i
        j0, j1 = np.searchsorted(pts[:, 0], [c_x - 4.5, c_x + 4.5])
        xc = pts[j0:j1] @ Rs[i].T + ts[i]
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = fx * xc[:, 0] / xc[:, 2] + cx, fy * xc[:, 1] / xc[:, 2] + cy
        ok = np.nonzero((xc[:, 2] >= 0.3) & (u >= 0) & (u < 640) & (v >= 0) & (v < 480))[0]
        m = len(ok)
        octv = rng.choice(8, m, p=np.array([217, 181, 151, 126, 105, 87, 73, 60]) / 1000.0)
        noise = rng.normal(0, 1, (m, 3)) * np.sqrt(sigma2[octv])[:, None]
        out = rng.random(m) < outlier_frac
        noise[out, :2] += rng.choice([-1.0, 1.0], (int(out.sum()), 2)) * 20.0
        stereo = rng.random(m) >= mono_frac
        ur = u[ok] - bf / xc[ok, 2]
        obs = np.stack([np.float32(u[ok] + noise[:, 0]), np.float32(v[ok] + noise[:, 1]),
                        np.where(stereo, np.float32(ur + noise[:, 2]), np.float32(-1.0))], 1).astype(np.float64)
        cols["pose"].append(np.full(m, i, np.int32))
        cols["point"].append((j0 + ok).astype(np.int32))
        cols["obs"].append(obs)
        cols["is2"].append(inv_sigma2[octv])
        cols["stereo"].append(stereo.astype(np.uint8))
    e_pose, e_point = np.concatenate(cols["pose"]), np.concatenate(cols["point"])
    seen = np.zeros(n_points, bool)
    seen[e_point] = True
    new_id = np.cumsum(seen) - 1  # points nobody sees are left out (src/Optimizer.cc:263-268 drops them from the graph)
    order = np.argsort(e_point, kind="stable")  # point-major, key-frames ascending within a point
    e_pose, e_point = e_pose[order], new_id[e_point[order]].astype(np.int32)
    pts = pts[seen]
    fixed_flags = np.zeros(n_keyframes, np.uint8)
    fixed_flags[[0] + [int(k) for k in fixed]] = 1
    q_gt = np.array([_quat_from_R(R) for R in Rs])
    t_gt = np.array(ts)
    q0, t0 = q_gt.copy(), t_gt.copy()
    for i in range(n_keyframes):
        if fixed_flags[i]:
            continue
        dR = _rot(*(np.deg2rad(0.3) * rng.normal(size=3)))
        q0[i] = _quat_from_R(dR @ Rs[i])
        t0[i] = dR @ ts[i] + 0.01 * rng.normal(size=3)
    q0 = q0.astype(np.float32).astype(np.float64)
    t0 = t0.astype(np.float32).astype(np.float64)
    p0 = (pts + 0.02 * rng.normal(size=pts.shape)).astype(np.float32).astype(np.float64)
    return dict(n_poses=n_keyframes, n_points=len(pts), n_edges=len(e_pose), pose_q=np.ascontiguousarray(q0),
                pose_t=np.ascontiguousarray(t0), pose_fixed=fixed_flags, points=np.ascontiguousarray(p0),
                edge_pose=np.ascontiguousarray(e_pose), edge_point=np.ascontiguousarray(e_point),
                edge_obs=np.ascontiguousarray(np.concatenate(cols["obs"])[order]),
                edge_inv_sigma2=np.ascontiguousarray(np.concatenate(cols["is2"])[order]),
                edge_stereo=np.ascontiguousarray(np.concatenate(cols["stereo"])[order]), fx=fx, fy=fy, cx=cx, cy=cy, bf=bf,
                huber_mono=float(np.float32(np.sqrt(5.99))),  # thHuber2D = sqrt(5.99), not LocalBundleAdjustment's 5.991 (src/Optimizer.cc:126)
                huber_stereo=float(np.float32(np.sqrt(7.815))), iterations=10, gt_q=q_gt, gt_t=t_gt, gt_points=pts)


def pose_frame(seed, n_obs=300, mono_frac=0.15, outlier_frac=0.1, rot_deg=1.0, trans=0.03, outlier_px=25.0, noise_scale=1.0):
    """Synthetic Optimizer::PoseOptimization problem (reference src/Optimizer.cc:763-1098): one frame looking at `n_obs`
    map points in a 6x4x3 m box, RGB-D ("stereo", 3-D) observations with a fraction without depth (mono, 2-D), pixel noise
    sigma = sqrt(sigma2[octave]), `outlier_frac` gross outliers, initial pose off by ~rot_deg / ~trans metres.
    Returns the flat arrays of gfs_pose_problem (include/gfs_abi.h) plus the ground truth pose (q_gt, t_gt)."""
    rng = np.random.default_rng(seed)
    fx = fy = np.float64(np.float32(607.0))
    cx, cy = np.float64(np.float32(319.5)), np.float64(np.float32(239.5))
    bf = np.float64(np.float32(0.0745 * 607.0))
    Rcw = _rot(0.05 * rng.normal(), 0.2 * rng.normal(), 0.05 * rng.normal())
    tcw = np.array([0.3 * rng.normal(), 0.1 * rng.normal(), 0.2 * rng.normal()])
    sigma2 = np.float64(np.float32(1.2) ** (2 * np.arange(8)))
    inv_sigma2 = (np.float32(1.0) / np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
    xw, obs, w, st, is_out = [], [], [], [], []
    while len(xw) < n_obs:
        xc = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(1.0, 6.0)])
        u, v = fx * xc[0] / xc[2] + cx, fy * xc[1] / xc[2] + cy
        if not (0 <= u < 640 and 0 <= v < 480):
            continue
        octv = int(rng.choice(8, p=np.array([217, 181, 151, 126, 105, 87, 73, 60]) / 1000.0))
        noise = noise_scale * rng.normal(0, np.sqrt(sigma2[octv]), 3)
        out = rng.random() < outlier_frac
        if out:
            noise[:2] += rng.choice([-1, 1], 2) * outlier_px
        stereo = rng.random() >= mono_frac
        ur = u - bf / xc[2]
        xw.append((Rcw.T @ (xc - tcw)).astype(np.float32).astype(np.float64))  # MapPoint world positions are floats
        obs.append([np.float32(u + noise[0]), np.float32(v + noise[1]), np.float32(ur + noise[2]) if stereo else -1.0])
        w.append(inv_sigma2[octv])
        st.append(1 if stereo else 0)
        is_out.append(out)
    dR = _rot(*(np.deg2rad(rot_deg) * rng.normal(size=3)))
    q0 = _quat_from_R(dR @ Rcw).astype(np.float32).astype(np.float64)  # Sophus::SE3f pose widened to double
    t0 = (dR @ tcw + trans * rng.normal(size=3)).astype(np.float32).astype(np.float64)
    return dict(q=q0, t=t0, n_obs=n_obs, xw=np.array(xw), obs=np.array(obs, np.float64), inv_sigma2=np.array(w, np.float32),
                stereo=np.array(st, np.uint8), fx=fx, fy=fy, cx=cx, cy=cy, bf=bf, n_rounds=4, its=10,
                q_gt=_quat_from_R(Rcw), t_gt=tcw, is_outlier=np.array(is_out))


def sbp_pair(seed, n_points=900, n_extra_cur=250, motion=0.04, rot_deg=0.8, th=7.0, mono=False, desc_flip_bits=18,
             dup_frac=0.0, zero_obs_frac=0.0, preassigned_frac=0.0, n_levels=8, check_orientation=True):
    """Synthetic input of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (reference
    src/ORBmatcher.cc:1853-2063), flattened as gfs_sbp_problem (include/gfs_abi.h).

    `n_points` map points seen by the last frame; the current frame (pose = last pose composed with a small motion) sees
    most of them again (key-point = projection + sub-pixel noise, octave within +-1, descriptor = map-point descriptor with
    `desc_flip_bits` random bit flips, angle = last angle + small rotation) plus `n_extra_cur` unrelated key-points.
    dup_frac: fraction of map points duplicated (two map points competing for the same key-point -> the order-dependent
    skip of :1914-1915); zero_obs_frac: map points with Observations() == 0 (their assignment may be overwritten);
    preassigned_frac: current key-points that already hold a map point with observations."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    fx = fy = f32(607.0)
    cx, cy = f32(319.5), f32(239.5)
    bf = f32(0.0745 * 607.0)
    b = f32(0.0745)
    W, H = 640, 480
    min_x, max_x, min_y, max_y = f32(0), f32(W), f32(0), f32(H)
    scale = np.cumprod(np.r_[1.0, np.full(n_levels - 1, 1.2)]).astype(np.float32)
    Rlw = _rot(0.03 * rng.normal(), 0.2 * rng.normal(), 0.03 * rng.normal())
    tlw = np.array([0.2 * rng.normal(), 0.05 * rng.normal(), 0.1 * rng.normal()])
    dR = _rot(*(np.deg2rad(rot_deg) * rng.normal(size=3)))
    Rcw, tcw = dR @ Rlw, dR @ tlw + motion * rng.normal(size=3) + np.array([0, 0, -motion])
    kp_dtype = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                         ("octave", "<i4"), ("class_id", "<i4")])
    last_xw, last_desc, last_oct, last_ang, last_obs = [], [], [], [], []
    cur = []  # (x, y, octave, angle, u_right, desc)
    roll = np.deg2rad(rot_deg) * rng.normal()
    while len(last_xw) < n_points:
        xl = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(1.0, 7.0)])  # in the last camera
        ul, vl = fx * xl[0] / xl[2] + cx, fy * xl[1] / xl[2] + cy
        if not (0 <= ul < W and 0 <= vl < H):
            continue
        xw = (Rlw.T @ (xl - tlw)).astype(np.float32)
        octv = int(rng.choice(n_levels, p=np.array([217, 181, 151, 126, 105, 87, 73, 60][:n_levels]) / sum([217, 181, 151, 126, 105, 87, 73, 60][:n_levels])))
        ang = f32(rng.uniform(0, 360))
        desc = rng.integers(0, 256, 32, dtype=np.uint8)
        reps = 2 if rng.random() < dup_frac else 1
        for _ in range(reps):
            last_xw.append(xw + (0 if _ == 0 else rng.normal(0, 0.002, 3).astype(np.float32)))
            d = desc.copy()
            if _ > 0:
                flip = rng.choice(256, 6, replace=False)
                np.bitwise_xor.at(d, flip // 8, (1 << (flip % 8)).astype(np.uint8))
            last_desc.append(d)
            last_oct.append(octv)
            last_ang.append(ang)
            last_obs.append(0 if rng.random() < zero_obs_frac else 1)
        xc = Rcw @ xw.astype(np.float64) + tcw
        if xc[2] <= 0.2:
            continue
        uc, vc = fx * xc[0] / xc[2] + cx, fy * xc[1] / xc[2] + cy
        if not (0 <= uc < W and 0 <= vc < H) or rng.random() < 0.15:
            continue
        d = desc.copy()
        flip = rng.choice(256, int(rng.integers(0, desc_flip_bits + 1)), replace=False)
        np.bitwise_xor.at(d, flip // 8, (1 << (flip % 8)).astype(np.uint8))
        o2 = int(np.clip(octv + rng.integers(-1, 2), 0, n_levels - 1))
        a2 = f32((ang + np.rad2deg(roll) + rng.normal(0, 3.0)) % 360.0)
        if rng.random() < 0.06:
            a2 = f32(rng.uniform(0, 360))  # inconsistent rotation -> removed by the histogram check
        x2, y2 = f32(uc + rng.normal(0, 0.7)), f32(vc + rng.normal(0, 0.7))
        ur = f32(x2 - bf / xc[2] + rng.normal(0, 0.5)) if (not mono and rng.random() < 0.85) else f32(-1)
        cur.append((x2, y2, o2, a2, ur, d))
    for _ in range(n_extra_cur):
        cur.append((f32(rng.uniform(0, W)), f32(rng.uniform(0, H)), int(rng.integers(0, n_levels)), f32(rng.uniform(0, 360)),
                    f32(rng.uniform(1, W)) if rng.random() < 0.5 else f32(-1), rng.integers(0, 256, 32, dtype=np.uint8)))
    order = rng.permutation(len(cur))
    cur = [cur[i] for i in order]
    kps = np.zeros(len(cur), kp_dtype)
    kps["x"] = [c[0] for c in cur]
    kps["y"] = [c[1] for c in cur]
    kps["octave"] = [c[2] for c in cur]
    kps["angle"] = [c[3] for c in cur]
    kps["size"] = 31.0
    kps["class_id"] = -1
    return dict(last_xw=np.array(last_xw, np.float32)[:n_points], last_desc=np.array(last_desc, np.uint8)[:n_points],
                last_octave=np.array(last_oct, np.int32)[:n_points], last_angle=np.array(last_ang, np.float32)[:n_points],
                last_mp_has_obs=np.array(last_obs, np.uint8)[:n_points], cur_kps_un=kps,
                cur_u_right=np.array([c[4] for c in cur], np.float32), cur_desc=np.array([c[5] for c in cur], np.uint8).reshape(-1, 32),
                cur_has_mp_obs=(rng.random(len(cur)) < preassigned_frac).astype(np.uint8),
                Tcw_q=_quat_from_R(Rcw).astype(np.float32), Tcw_t=tcw.astype(np.float32),
                Tlw_q=_quat_from_R(Rlw).astype(np.float32), Tlw_t=tlw.astype(np.float32),
                fx=fx, fy=fy, cx=cx, cy=cy, bf=bf, b=b, min_x=min_x, max_x=max_x, min_y=min_y, max_y=max_y,
                grid_w_inv=f32(64) / (max_x - min_x), grid_h_inv=f32(48) / (max_y - min_y), scale_factors=scale,
                th=f32(th), mono=int(mono), check_orientation=int(check_orientation))


def sbp_map_frame(seed, th=1.0, nn_ratio=0.8, **kw):
    """Synthetic input of ORBmatcher::SearchByProjection(F, vpMapPoints, th, ...) (reference src/ORBmatcher.cc:43-206) as
    gfs_sbp_map_problem: the scene of sbp_pair with the projections Frame::isInFrustum would leave on the map points
    (mTrackProjX / Y / XR, predicted level, viewing cosine), in double like the float pipeline's inputs rounded to float."""
    p = sbp_pair(seed, **kw)
    rng = np.random.default_rng(seed + 7919)
    R = _rot_from_quat(p["Tcw_q"].astype(np.float64))
    xc = p["last_xw"].astype(np.float64) @ R.T + p["Tcw_t"].astype(np.float64)
    keep = (xc[:, 2] > 0.2)
    u = p["fx"] * xc[:, 0] / xc[:, 2] + p["cx"]
    v = p["fy"] * xc[:, 1] / xc[:, 2] + p["cy"]
    keep &= (u >= 0) & (u < 640) & (v >= 0) & (v < 480)
    ur = u - p["bf"] / xc[:, 2]
    view_cos = np.where(rng.random(len(u)) < 0.5, 0.9995, rng.uniform(0.5, 0.998, len(u))).astype(np.float32)
    return dict(mp_proj=np.stack([u, v, ur], 1)[keep].astype(np.float32), mp_level=p["last_octave"][keep],
                mp_view_cos=view_cos[keep], mp_desc=p["last_desc"][keep], mp_has_obs=p["last_mp_has_obs"][keep],
                cur_kps_un=p["cur_kps_un"], cur_u_right=p["cur_u_right"], cur_desc=p["cur_desc"], cur_has_mp_obs=p["cur_has_mp_obs"],
                min_x=p["min_x"], min_y=p["min_y"], grid_w_inv=p["grid_w_inv"], grid_h_inv=p["grid_h_inv"],
                scale_factors=p["scale_factors"], th=np.float32(th), nn_ratio=np.float32(nn_ratio))


def local_points_frame(seed, n_points=2000, n_cur=None, scale_factor=1.2, n_levels=8, th=1.0, nn_ratio=0.8, far_points=True,
                       th_far_points=6.0, view_cos_limit=0.5, share=0.5, **kw):
    """Synthetic input of Tracking::SearchLocalPoints from its second loop on (reference src/Tracking.cc:4312-4358), flattened as
    gfs_local_points_problem (include/gfs_abi.h): a frame pose, its key-points, and a list of `n_points` local map points with
    world position, normal and scale-invariance distances.

    About `share` of the list are the map points of sbp_pair's scene (same key-point and descriptor construction, so real matches
    exist); their normals mostly face the camera, their distance ranges put the predicted level at the octave they were seen at.  A
    few per cent each are bent away (viewing angle), too near, too far, or sit beyond the last / before the first pyramid level
    (the clamps of MapPoint::PredictScale).  The rest are laid out in the camera frame: behind it, off each of the four image
    sides, or in view without a key-point.  The list is shuffled, so the exits alternate along it.  One scene point that has a
    key-point in the frame (the anchor) is kept clean and its key-point is moved to index 0, so a frame with any key-point has a
    match.  n_cur: exact number of key-points (the scene's list cut or padded with unrelated ones); None = as the scene has them."""
    rng = np.random.default_rng(seed + 104729)
    f32 = np.float32
    n_scene = min(n_points, max(int(round(n_points * share)), 1)) if n_points > 0 else 0
    p = sbp_pair(seed, n_points=max(n_scene, 16), n_levels=n_levels, **kw)
    sf = float(scale_factor)
    scale = np.cumprod(np.r_[1.0, np.full(n_levels - 1, sf)]).astype(np.float32)
    R = _rot_from_quat(p["Tcw_q"].astype(np.float64)).astype(np.float32)
    t = p["Tcw_t"].astype(np.float32)
    Ow = (-(R.T.astype(np.float64) @ t.astype(np.float64))).astype(np.float32)
    R64, t64, Ow64 = R.astype(np.float64), t.astype(np.float64), Ow.astype(np.float64)
    fx, fy, cx, cy, bf = (float(p[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    W, H = float(p["max_x"]), float(p["max_y"])
    kps, cur_ur, cur_desc, cur_obs = p["cur_kps_un"].copy(), p["cur_u_right"].copy(), p["cur_desc"].copy(), p["cur_has_mp_obs"].copy()
    # the anchor: the first scene point whose key-point sits close to its projection, on a level the window accepts, not too deep
    anchor, anchor_kp = None, None
    if len(kps):
        bits = np.unpackbits(cur_desc, axis=1)
        for j in range(min(len(p["last_xw"]), 64)):
            xc = R64 @ p["last_xw"][j].astype(np.float64) + t64
            if not (0.3 < xc[2] and np.linalg.norm(xc) < 0.9 * th_far_points):
                continue
            u, v = fx * xc[0] / xc[2] + cx, fy * xc[1] / xc[2] + cy
            d = (bits != np.unpackbits(p["last_desc"][j])[None, :]).sum(1)
            i = int(np.argmin(d))
            o = int(p["last_octave"][j])
            if d[i] <= 24 and abs(kps["x"][i] - u) < 1.5 and abs(kps["y"][i] - v) < 1.5 and kps["octave"][i] in (o - 1, o) and \
                    (cur_ur[i] <= 0 or abs(cur_ur[i] - (u - bf / xc[2])) < 2.0) and not cur_obs[i]:
                anchor, anchor_kp = j, i
                break
    if anchor_kp is not None and anchor_kp != 0:
        for a in (kps, cur_ur, cur_desc, cur_obs):
            a[[0, anchor_kp]] = a[[anchor_kp, 0]]
    if n_cur is not None:
        if len(kps) >= n_cur:
            kps, cur_ur, cur_desc, cur_obs = kps[:n_cur], cur_ur[:n_cur], cur_desc[:n_cur], cur_obs[:n_cur]
        else:
            m = n_cur - len(kps)
            extra = np.zeros(m, kps.dtype)
            extra["x"], extra["y"] = rng.uniform(0, W, m), rng.uniform(0, H, m)
            extra["octave"], extra["angle"], extra["size"], extra["class_id"] = rng.integers(0, n_levels, m), rng.uniform(0, 360, m), 31.0, -1
            kps = np.concatenate([kps, extra])
            cur_ur = np.concatenate([cur_ur, np.where(rng.random(m) < 0.5, rng.uniform(1, W, m), -1).astype(np.float32)])
            cur_desc = np.concatenate([cur_desc.reshape(-1, 32), rng.integers(0, 256, (m, 32), dtype=np.uint8)])
            cur_obs = np.concatenate([cur_obs, np.zeros(m, np.uint8)])
    # scene points: the anchor first, then the others in scene order
    ids = ([anchor] if anchor is not None else []) + [j for j in range(len(p["last_xw"])) if j != anchor]
    ids = ids[:n_scene]
    xw, nrm, dmin, dmax, desc, obs = [], [], [], [], [], []

    def unit(v):
        return v / max(np.linalg.norm(v), 1e-12)

    def add(P, octv, d, o, kind):
        """kind: 0 clean, 1 bent away, 2 too far, 3 too near, 4 beyond the last level, 5 before the first level"""
        PO = P.astype(np.float64) - Ow64
        dist = np.linalg.norm(PO)
        side = unit(np.cross(PO, rng.normal(size=3)))
        if kind == 1:
            n = unit(0.3 * unit(PO) + side)                      # cos ~ 0.29
        elif rng.random() < 0.4:
            n = unit(PO)                                         # cos ~ 1: the narrow window of RadiusByViewingCos
        else:
            n = unit(unit(PO) + rng.uniform(0.1, 1.2) * side)    # cos 0.64 .. 0.995
        mx = dist * sf ** (octv - 0.5 + rng.uniform(-0.3, 0.3))
        if kind == 4:
            mx = dist * sf ** (n_levels - 1) * (1.0 + 0.5 * (sf - 1.0))
        if kind == 5:
            mx = dist * 0.85
        mn = mx / sf ** (n_levels - 1)
        if kind == 2:
            mx = dist / 1.5
            mn = mx / sf ** (n_levels - 1)
        if kind == 3:
            mn = dist * 1.5
        xw.append(P.astype(np.float32)); nrm.append(n.astype(np.float32)); dmin.append(f32(mn)); dmax.append(f32(mx))
        desc.append(d); obs.append(o)

    for q, j in enumerate(ids):
        kind = 0 if j == anchor else int(rng.choice(6, p=[0.74, 0.08, 0.05, 0.05, 0.04, 0.04]))
        add(p["last_xw"][j], int(p["last_octave"][j]), p["last_desc"][j], int(p["last_mp_has_obs"][j]), kind)
    for q in range(n_points - len(ids)):
        where = q % 6  # behind, left, right, above, below, in view
        z = rng.uniform(1.0, 7.0)
        u, v = rng.uniform(0, W), rng.uniform(0, H)
        if where == 0:
            z = -rng.uniform(0.2, 5.0)
        elif where == 1:
            u = -rng.uniform(0.5, 300)
        elif where == 2:
            u = W + rng.uniform(0.5, 300)
        elif where == 3:
            v = -rng.uniform(0.5, 300)
        elif where == 4:
            v = H + rng.uniform(0.5, 300)
        xc = np.array([(u - cx) / fx * abs(z), (v - cy) / fy * abs(z), z])
        P = R64.T @ (xc - t64)
        add(P, int(rng.integers(0, n_levels)), rng.integers(0, 256, 32, dtype=np.uint8), 1, 0)
    order = rng.permutation(n_points)
    take = lambda a, shape, dt: (np.array(a, dt).reshape(shape)[order] if n_points else np.zeros((0,) + shape[1:], dt))
    return dict(mp_xw=take(xw, (-1, 3), np.float32), mp_normal=take(nrm, (-1, 3), np.float32), mp_min_dist=take(dmin, (-1,), np.float32),
                mp_max_dist=take(dmax, (-1,), np.float32), mp_desc=take(desc, (-1, 32), np.uint8), mp_has_obs=take(obs, (-1,), np.uint8),
                Rcw=R.reshape(9), tcw=t, Ow=Ow, fx=p["fx"], fy=p["fy"], cx=p["cx"], cy=p["cy"], bf=p["bf"], min_x=p["min_x"],
                max_x=p["max_x"], min_y=p["min_y"], max_y=p["max_y"], grid_w_inv=p["grid_w_inv"], grid_h_inv=p["grid_h_inv"],
                scale_factors=scale, n_levels=n_levels, log_scale_factor=f32(np.log(f32(sf))), view_cos_limit=f32(view_cos_limit),
                far_points=int(bool(far_points)), th_far_points=f32(th_far_points), th=f32(th), nn_ratio=f32(nn_ratio),
                cur_kps_un=kps, cur_u_right=cur_ur, cur_desc=cur_desc.reshape(-1, 32), cur_has_mp_obs=cur_obs)


def fuse_problem(seed, n_points=1000, n_kp=1000, n_keyframes=1, scale_factor=1.2, n_levels=8, th=3.0, width=640, height=480):
    """Synthetic input of ORBmatcher::Fuse(pKF, vpMapPoints, th) (reference src/ORBmatcher.cc:1378-1548) for one list of `n_points` map
    points searched in `n_keyframes` key frames of `n_kp` key-points each, as gfs_fuse_search takes it (include/gfs_abi.h):
    -> dict(lists=[points dict], keyframes=[key-frame dict, ...]).

    The key frames are small motions of one pose.  Seven in ten points lie in front of all of them; each key frame sees most of
    those again (key-point = projection + noise growing with the level, some beyond the chi2 gates; octave = the predicted level or
    one below, a few two below or one above; descriptor = the point's with up to 18 bits flipped, a few unrelated; mvuRight
    present for most, a few exactly 0).  One in eight of these key-points has a twin a pixel or a cell away with the same
    descriptor (a Hamming tie).  Some points are bent away, too near or too far; the rest sit behind the cameras, off the image
    or in view without a key-point, so every exit of the loop is taken.  The list is shuffled."""
    rng = np.random.default_rng(seed + 15485863)
    f32 = np.float32
    fx = fy = f32(607.0)
    cx, cy = f32(width / 2 - 0.5), f32(height / 2 - 0.5)
    bf = f32(0.0745 * 607.0)
    sf = float(scale_factor)
    scale = np.cumprod(np.r_[1.0, np.full(n_levels - 1, sf)]).astype(np.float32)
    inv_sigma2 = (f32(1) / (scale * scale)).astype(np.float32)
    W, H = float(width), float(height)
    R0 = _rot(0.03 * rng.normal(), 0.2 * rng.normal(), 0.03 * rng.normal())
    t0 = np.array([0.2 * rng.normal(), 0.05 * rng.normal(), 0.1 * rng.normal()])
    poses = []
    for f in range(n_keyframes):
        dR = _rot(*(np.deg2rad(0.8) * rng.normal(size=3))) if f else np.eye(3)
        q = _quat_from_R(dR @ R0).astype(np.float32)
        t = (dR @ t0 + (0.04 * rng.normal(size=3) if f else 0)).astype(np.float32)
        Rq = _rot_from_quat(q.astype(np.float64))
        poses.append((q, t, Rq, t.astype(np.float64), (-(Rq.T @ t.astype(np.float64))).astype(np.float32)))
    R0q, t0q = poses[0][2], poses[0][3]
    Ow0 = poses[0][4].astype(np.float64)
    xw, nrm, dmin, dmax, desc, octs, scene = [], [], [], [], [], [], []

    def unit(v):
        return v / max(np.linalg.norm(v), 1e-12)

    for i in range(n_points):
        where = int(rng.choice(7, p=[0.7, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05]))  # in view; behind; left; right; above; below; in view
        z = rng.uniform(1.0, 7.0)
        u, v = rng.uniform(30, W - 30), rng.uniform(30, H - 30)
        if where == 1:
            z = -rng.uniform(0.2, 5.0)
        elif where == 2:
            u = -rng.uniform(0.5, 300)
        elif where == 3:
            u = W + rng.uniform(0.5, 300)
        elif where == 4:
            v = -rng.uniform(0.5, 300)
        elif where == 5:
            v = H + rng.uniform(0.5, 300)
        xc = np.array([(u - cx) / fx * abs(z), (v - cy) / fy * abs(z), z])
        P = (R0q.T @ (xc - t0q)).astype(np.float32)
        PO = P.astype(np.float64) - Ow0
        dist = np.linalg.norm(PO)
        kind = int(rng.choice(4, p=[0.82, 0.06, 0.06, 0.06])) if where == 0 else 0  # clean, bent away, too far, too near
        side = unit(np.cross(PO, rng.normal(size=3)))
        n = unit(0.3 * unit(PO) + side) if kind == 1 else unit(unit(PO) + rng.uniform(0.0, 1.2) * side)
        o = int(rng.integers(0, n_levels))
        mx = dist * sf ** (o - 0.5 + rng.uniform(-0.3, 0.3))
        mn = mx / sf ** (n_levels - 1)
        if kind == 2:
            mx = dist / 1.5
            mn = mx / sf ** (n_levels - 1)
        if kind == 3:
            mn = dist * 1.5
        xw.append(P); nrm.append(n.astype(np.float32)); dmin.append(f32(mn)); dmax.append(f32(mx)); octs.append(o)
        desc.append(rng.integers(0, 256, 32, dtype=np.uint8))
        scene.append(where == 0)
    order = rng.permutation(n_points)
    take = lambda a, shape, dt: (np.array(a, dt).reshape(shape)[order] if n_points else np.zeros((0,) + shape[1:], dt))
    pts = dict(mp_xw=take(xw, (-1, 3), np.float32), mp_normal=take(nrm, (-1, 3), np.float32), mp_min_dist=take(dmin, (-1,), np.float32),
               mp_max_dist=take(dmax, (-1,), np.float32), mp_desc=take(desc, (-1, 32), np.uint8))
    kp_dtype = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                         ("class_id", "<i4")])
    kfs = []
    for f, (q, t, Rq, tq, Ow) in enumerate(poses):
        cur = []  # (x, y, octave, u_right, desc)
        for i in range(n_points):
            if not scene[i] or rng.random() < 0.25:
                continue
            xc = Rq @ xw[i].astype(np.float64) + tq
            if xc[2] <= 0.2:
                continue
            uc, vc = fx * xc[0] / xc[2] + cx, fy * xc[1] / xc[2] + cy
            if not (0 <= uc < W and 0 <= vc < H):
                continue
            o = int(np.clip(octs[i] + rng.choice([0, -1, -2, 1], p=[0.5, 0.4, 0.05, 0.05]), 0, n_levels - 1))
            sig = (0.5 if rng.random() < 0.8 else 2.0) * float(scale[o])
            x2, y2 = f32(np.clip(uc + rng.normal(0, sig), 0, W - 1)), f32(np.clip(vc + rng.normal(0, sig), 0, H - 1))
            d = desc[i].copy()
            if rng.random() < 0.1:
                d = rng.integers(0, 256, 32, dtype=np.uint8)
            else:
                flip = rng.choice(256, int(rng.integers(0, 19)), replace=False)
                np.bitwise_xor.at(d, flip // 8, (1 << (flip % 8)).astype(np.uint8))
            r = rng.random()
            ur = f32(x2 - bf / xc[2] + rng.normal(0, sig)) if r < 0.8 else (f32(0) if r < 0.83 else f32(-1))
            cur.append((x2, y2, o, ur, d))
            if rng.random() < 0.125:  # a twin with the same descriptor: a pixel away, or in the next grid column
                dx = 1.0 if rng.random() < 0.5 else float(rng.choice([-1, 1])) * 0.6 * W / 64
                cur.append((f32(np.clip(x2 + dx, 0, W - 1)), y2, o, ur, d.copy()))
        order = rng.permutation(len(cur))
        cur = [cur[i] for i in order][:n_kp]
        while len(cur) < n_kp:
            cur.append((f32(rng.uniform(0, W)), f32(rng.uniform(0, H)), int(rng.integers(0, n_levels)),
                        f32(rng.uniform(1, W)) if rng.random() < 0.5 else f32(-1), rng.integers(0, 256, 32, dtype=np.uint8)))
        kps = np.zeros(len(cur), kp_dtype)
        kps["x"], kps["y"], kps["octave"] = [c[0] for c in cur], [c[1] for c in cur], [c[2] for c in cur]
        kps["size"], kps["class_id"] = 31.0, -1
        kfs.append(dict(Tcw_q=q, Tcw_t=t, Ow=Ow, fx=fx, fy=fy, cx=cx, cy=cy, bf=bf, min_x=f32(0), max_x=f32(W), min_y=f32(0), max_y=f32(H),
                        grid_w_inv=f32(64) / f32(W), grid_h_inv=f32(48) / f32(H), scale_factors=scale, inv_level_sigma2=inv_sigma2,
                        n_levels=n_levels, log_scale_factor=f32(np.log(f32(sf))), th=f32(th), kps_un=kps,
                        u_right=np.array([c[3] for c in cur], np.float32),
                        desc=np.array([c[4] for c in cur], np.uint8).reshape(-1, 32), list=0))
    return dict(lists=[pts], keyframes=kfs)


def sim3_search_problem(seed, mode, n_points=1000, n_kp=1000, n_problems=1, th=None, ratio_hamming=None, scale_factor=1.2, n_levels=8,
                        cluster_every=10, taken_frac=0.08, skip_frac=0.05, masks=True, width=640, height=480):
    """Synthetic input of the three Sim3 searches of loop closing (reference src/ORBmatcher.cc:1550-1654 mode 0, :432-529 mode 1,
    :531-636 mode 2) for one list of `n_points` map points searched in `n_problems` key frames of `n_kp` key-points each, as
    gfs_sim3_search takes it (include/gfs_abi.h): -> dict(lists=[points dict], problems=[problem dict, ...]).

    The scene is fuse_problem's (every exit of the loop is taken, Hamming ties included), the key frame's pose standing for the
    SE3 part of Scw.  On top of it one point in `cluster_every` heads a cluster: two to four other list entries become copies of
    it (same position, normal and distances, so the same projection in every key frame) whose descriptors differ from the head's in
    one to three bits, and every key frame gets two or three more key-points within a pixel and a half of the head's own key-point,
    on its octave, a few bits from the head's descriptor -- so the members of a cluster want the same key-points, and in the
    projection modes who comes first decides who gets which.  With `masks`, `taken_frac` of the key-points are taken at entry
    (kp_taken; projection modes only), a cluster's best key-point more often than others, and `skip_frac` of the points carry
    mp_skip.  th and ratio_hamming default to the call sites' values: 4 for Fuse; 3 and 1.5 for mode 1; 8 and 1.5 for mode 2."""
    mode = int(mode)
    th = {0: 4.0, 1: 3.0, 2: 8.0}[mode] if th is None else th
    ratio_hamming = 1.5 if ratio_hamming is None else ratio_hamming
    base = fuse_problem(seed, n_points=n_points, n_kp=n_kp, n_keyframes=n_problems, scale_factor=scale_factor, n_levels=n_levels, th=th,
                        width=width, height=height)
    rng = np.random.default_rng(seed + 32452843)
    pts = {k: np.array(v) for k, v in base["lists"][0].items()}
    kfs = [dict(kf, kps_un=kf["kps_un"].copy(), desc=kf["desc"].copy()) for kf in base["keyframes"]]

    def flipped(d, nbits):
        d = d.copy()
        b = rng.choice(256, nbits, replace=False)
        np.bitwise_xor.at(d, b // 8, (1 << (b % 8)).astype(np.uint8))
        return d

    heads = []
    if n_points >= 4 and cluster_every > 0:
        free = list(rng.permutation(n_points))
        for _ in range(max(1, n_points // cluster_every)):
            if len(free) < 5:
                break
            h = int(free.pop())
            members = [int(free.pop()) for _ in range(int(rng.integers(2, 5)))]
            for m in members:
                for k in ("mp_xw", "mp_normal", "mp_min_dist", "mp_max_dist"):
                    pts[k][m] = pts[k][h]
                pts["mp_desc"][m] = flipped(pts["mp_desc"][h], int(rng.integers(1, 4)))
            heads.append(h)
    problems = []
    for kf in kfs:
        n = len(kf["kps_un"])
        taken = (rng.random(n) < taken_frac).astype(np.uint8)
        if n >= 8 and heads:
            kbits = np.unpackbits(kf["desc"], axis=1)
            used = set()
            for h in heads:
                d = (kbits != np.unpackbits(pts["mp_desc"][h])[None, :]).sum(1)
                j = int(np.argmin(d))
                if d[j] > 18 or j in used:  # the head has no key-point of its own in this key frame
                    continue
                used.add(j)
                for _ in range(int(rng.integers(2, 4))):
                    e = int(rng.integers(0, n))
                    if e in used:
                        continue
                    used.add(e)
                    kf["kps_un"][e] = kf["kps_un"][j]
                    kf["kps_un"]["x"][e] = np.float32(np.clip(kf["kps_un"]["x"][j] + rng.uniform(-1.5, 1.5), 0, width - 1))
                    kf["kps_un"]["y"][e] = np.float32(np.clip(kf["kps_un"]["y"][j] + rng.uniform(-1.5, 1.5), 0, height - 1))
                    kf["desc"][e] = flipped(pts["mp_desc"][h], int(rng.integers(1, 9)))
                    taken[e] = 0
                taken[j] = rng.random() < 0.3
        p = {k: kf[k] for k in ("Tcw_q", "Tcw_t", "Ow", "fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "grid_w_inv", "grid_h_inv",
                                "scale_factors", "n_levels", "log_scale_factor", "kps_un", "desc", "list")}
        p.update(mode=mode, th=np.float32(th), ratio_hamming=np.float32(ratio_hamming),
                 kp_taken=taken if (masks and mode != 0) else None,
                 mp_skip=(rng.random(n_points) < skip_frac).astype(np.uint8) if masks else None)
        problems.append(p)
    return dict(lists=[pts], problems=problems)


def _rot_from_quat(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def klt_texture_pair(seed, width=640, height=480, shift=(3.3, -2.1), rot_deg=0.0, gain=1.0, noise=1):
    """Two views of one analytic texture: image 1 samples the texture at R(p - c) + c + shift, so a point p in image 0 is seen at
    p' = R^T(p - c - shift) + c ... in image 1 (returned as the callable `flow`).  -> (img0, img1, flow)."""
    rng = np.random.default_rng(seed)
    nwave = 24
    k = rng.uniform(0.02, 0.45, (nwave, 2)) * rng.choice([-1, 1], (nwave, 2))
    ph = rng.uniform(0, 6.28, nwave)
    amp = rng.uniform(6, 22, nwave)
    base = rng.uniform(90, 150)
    th = np.deg2rad(rot_deg)
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    c = np.array([width / 2.0, height / 2.0])

    def tex(x, y):
        v = np.full(x.shape, base)
        for i in range(nwave):
            v += amp[i] * np.sin(k[i, 0] * x + k[i, 1] * y + ph[i])
        return v

    u, v = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    img0 = tex(u, v)
    # image 1 pixel q shows the texture point R (q - c) + c + shift
    q = np.stack([u - c[0], v - c[1]], -1) @ R.T
    img1 = gain * tex(q[..., 0] + c[0] + shift[0], q[..., 1] + c[1] + shift[1])
    nrng = np.random.default_rng(seed + 17)
    if noise:
        img0 = img0 + nrng.integers(-noise, noise + 1, img0.shape)
        img1 = img1 + nrng.integers(-noise, noise + 1, img1.shape)

    def flow(p):
        """Position in image 1 of the texture point seen at p ([n, 2]) in image 0."""
        p = np.asarray(p, np.float64)
        return (p - c - np.asarray(shift)) @ R + c

    to_u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)
    return to_u8(img0), to_u8(img1), flow


def two_view_points(seed, n=400, outlier_frac=0.25, noise=0.3, width=640, height=480, trans=0.15, rot_deg=3.0):
    """Image points of n random 3-D points in two views related by a general motion (so that a fundamental matrix exists), pixel
    noise `noise`, a fraction replaced by gross mismatches.  -> (pts1 f32 [n, 2], pts2 f32 [n, 2], inlier bool [n], F_true [3, 3])."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = intrinsics(width, height)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    X = np.c_[rng.uniform(-2.5, 2.5, n), rng.uniform(-1.8, 1.8, n), rng.uniform(2.0, 7.0, n)]
    R = _rot(*np.deg2rad(rng.uniform(-rot_deg, rot_deg, 3)))
    t = rng.uniform(-trans, trans, 3)
    t[0] += trans  # never a pure rotation
    x1 = (K @ X.T).T
    x2 = (K @ (R @ X.T + t[:, None])).T
    p1 = x1[:, :2] / x1[:, 2:3] + rng.normal(0, noise, (n, 2))
    p2 = x2[:, :2] / x2[:, 2:3] + rng.normal(0, noise, (n, 2))
    out = rng.random(n) < outlier_frac
    p2[out] = np.c_[rng.uniform(0, width, out.sum()), rng.uniform(0, height, out.sum())]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return p1.astype(np.float32), p2.astype(np.float32), ~out, F / F[2, 2]


def cloud_pair(seed, width=160, height=120, trans=0.03, rot_deg=1.5):
    """Clouds only (no images): the depth maps are rendered at width x height and unprojected at stride 1, which gives the point
    density of a (4 width) x (4 height) depth image sampled at stride 4 (the intrinsics scale with the width) at 1/16 of the
    rendering cost.  -> (cloud0, cloud1, T_01)."""
    sc = Scene(seed)
    rng = np.random.default_rng(seed + 0x6F5)
    T1 = random_motion(rng, trans, rot_deg)
    d0 = sc.render(width, height, None, 0)[1]
    d1 = sc.render(width, height, T1, 1)[1]
    return depth_to_cloud(d0, 1), depth_to_cloud(d1, 1), T1


def voxel_average(xyz, res):
    """Mean of the points of every res-metre voxel (a stand-in for the PCL voxel filter that builds the local map), float32."""
    xyz = np.asarray(xyz, np.float64)
    keys = np.floor(xyz / res).astype(np.int64)
    _, inv = np.unique(keys, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv)
    out = np.stack([np.bincount(inv, xyz[:, k]) / cnt for k in range(3)], 1)
    return out.astype(np.float32)


def pose_lidar_frame(seed, n_obs=600, n_cloud=3000, n_keyframes=3, voxel=0.1, width=320, height=240, rot_deg=1.0, trans=0.03,
                     mono_frac=0.15, outlier_frac=0.1, outlier_px=25.0, n_iterations=3):
    """Synthetic Optimizer::PoseLidarVisualOptimization problem (reference src/Optimizer.cc:7698-8059) on a Scene: the local map is
    2-3 key-frame renders in world coordinates, voxel-averaged at `voxel` metres; the frame cloud is the current view in camera
    coordinates (about n_cloud points); the visual observations are those of pose_frame, consistent with the true pose; the initial
    pose (a Sophus::SE3f: float q, t) is the true one perturbed by ~rot_deg / ~trans metres.  Returns the fields of
    gfs_pose_lidar_problem (include/gfs_abi.h) plus map_xyz and the ground truth (q_gt, t_gt of Tcw)."""
    rng = np.random.default_rng(seed)
    sc = Scene(seed)
    T_wc = random_motion(rng, trans=0.05, rot_deg=2.0)
    pts = []
    for k in range(n_keyframes):
        T_kf = T_wc @ random_motion(rng, trans=0.15, rot_deg=4.0)
        _, d = sc.render(width, height, T_kf, 100 + k)
        c = depth_to_cloud(d, 2)[:, :3].astype(np.float64)
        pts.append(c @ T_kf[:3, :3].T + T_kf[:3, 3])
    map_xyz = voxel_average(np.concatenate(pts), voxel)
    _, d = sc.render(width, height, T_wc, 7)
    cloud = depth_to_cloud(d, 1)[:, :3]
    if len(cloud) > n_cloud:
        cloud = cloud[np.sort(rng.choice(len(cloud), n_cloud, replace=False))]
    Rcw, tcw = T_wc[:3, :3].T, -T_wc[:3, :3].T @ T_wc[:3, 3]
    fx = fy = np.float64(np.float32(607.0))
    cx, cy = np.float64(np.float32(319.5)), np.float64(np.float32(239.5))
    bf = np.float64(np.float32(0.0745 * 607.0))
    sigma2 = np.float64(np.float32(1.2) ** (2 * np.arange(8)))
    inv_sigma2 = (np.float32(1.0) / np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
    xw, obs, w, st = [], [], [], []
    while len(xw) < n_obs:
        xc = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(1.0, 6.0)])
        u, v = fx * xc[0] / xc[2] + cx, fy * xc[1] / xc[2] + cy
        if not (0 <= u < 640 and 0 <= v < 480):
            continue
        octv = int(rng.choice(8, p=np.array([217, 181, 151, 126, 105, 87, 73, 60]) / 1000.0))
        noise = rng.normal(0, np.sqrt(sigma2[octv]), 3)
        if rng.random() < outlier_frac:
            noise[:2] += rng.choice([-1, 1], 2) * outlier_px
        stereo = rng.random() >= mono_frac
        ur = u - bf / xc[2]
        xw.append((Rcw.T @ (xc - tcw)).astype(np.float32).astype(np.float64))
        obs.append([np.float32(u + noise[0]), np.float32(v + noise[1]), np.float32(ur + noise[2]) if stereo else -1.0])
        w.append(inv_sigma2[octv])
        st.append(1 if stereo else 0)
    dR = _rot(*(np.deg2rad(rot_deg) * rng.normal(size=3)))
    q0 = _quat_from_R(dR @ Rcw).astype(np.float32)
    t0 = (dR @ tcw + trans * rng.normal(size=3)).astype(np.float32)
    return dict(q=q0, t=t0, xw=np.array(xw).reshape(-1, 3), obs=np.array(obs, np.float64).reshape(-1, 3),
                inv_sigma2=np.array(w, np.float32), stereo=np.array(st, np.uint8), fx=fx, fy=fy, cx=cx, cy=cy, bf=bf,
                cloud=np.ascontiguousarray(cloud, np.float32), map_xyz=map_xyz, n_iterations=n_iterations,
                q_gt=_quat_from_R(Rcw), t_gt=tcw)


def lba_lidar_window(seed, n_free=20, n_fixed=5, n_points=3000, n_cloud=3000, voxel=0.04, width=160, height=120, n_map_kf=3,
                     lidar=None, init_fixed=False, short_cloud=(), empty_cloud=(), map_shift=None, **kw):
    """Synthetic Optimizer::LocalVisualLidarBA window (reference src/Optimizer.cc:1101-1587): an lba_window (poses 0 .. n_free - 1
    are lLocalKeyFrames, the rest fixed cameras) on a Scene, with each key-frame's downsampled cloud rendered from its TRUE pose
    (camera frame, about n_cloud points) and the local map voxel-averaged (`voxel` metres) from n_map_kf renders in world
    coordinates, as pose_lidar_frame builds it.
      lidar: local poses with mnMatchesInliers <= 75 (default: every other local pose, starting with 1); the others get 76 .. 300;
      init_fixed: pose 0 is also fixed (the map's initial key-frame: local, fixed, with lidar edges);
      short_cloud: poses whose cloud is cut to 49 points; empty_cloud: poses without a cloud;
      map_shift: a translation added to the map (far away: no point gets an edge).
    The stored poses stay float values (Sophus::SE3f).  Returns lba_window's dict plus pose_local, matches_inliers, cloud_begin,
    cloud and map_xyz."""
    w = lba_window(seed, n_free=n_free, n_fixed=n_fixed, n_points=n_points, **kw)
    n_poses = w["n_poses"]
    rng = np.random.default_rng(seed + 0x1DA)
    sc = Scene(seed)
    local = np.zeros(n_poses, np.uint8)
    local[:n_free] = 1
    if init_fixed:
        w["pose_fixed"] = w["pose_fixed"].copy()
        w["pose_fixed"][0] = 1
        w["pose_q"][0], w["pose_t"][0] = w["gt_q"][0].astype(np.float32), w["gt_t"][0].astype(np.float32)
    lidar = list(range(1, n_free, 2)) if lidar is None else list(lidar)
    inl = rng.integers(76, 300, n_poses).astype(np.int32)
    for i in lidar:
        inl[i] = rng.integers(20, 76)
    def T_wc(i):
        Rcw = _rot_from_quat(w["gt_q"][i])
        T = np.eye(4)
        T[:3, :3] = Rcw.T
        T[:3, 3] = -Rcw.T @ w["gt_t"][i]
        return T
    clouds = []
    for i in range(n_poses):
        if i in empty_cloud:
            clouds.append(np.zeros((0, 3), np.float32))
            continue
        _, d = sc.render(width, height, T_wc(i), 200 + i)
        c = depth_to_cloud(d, 1)[:, :3].astype(np.float32)
        m = 49 if i in short_cloud else n_cloud
        if len(c) > m:
            c = c[np.sort(rng.choice(len(c), m, replace=False))]
        clouds.append(np.ascontiguousarray(c, np.float32))
    pts = []
    for k in range(n_map_kf):
        T = T_wc(int(round(k * (n_poses - 1) / max(n_map_kf - 1, 1))))
        _, d = sc.render(2 * width, 2 * height, T, 300 + k)
        c = depth_to_cloud(d, 1)[:, :3].astype(np.float64)
        pts.append(c @ T[:3, :3].T + T[:3, 3])
    map_xyz = voxel_average(np.concatenate(pts), voxel)
    if map_shift is not None:
        map_xyz = (map_xyz + np.asarray(map_shift, np.float32)).astype(np.float32)
    w.update(pose_local=local, matches_inliers=inl, cloud_begin=np.r_[0, np.cumsum([len(c) for c in clouds])].astype(np.int32),
             cloud=np.ascontiguousarray(np.concatenate(clouds), np.float32).reshape(-1, 3), map_xyz=map_xyz)
    return w


def lidar_map_window(seed, n_keyframes=7, n_cloud=3000, width=160, height=120, trans=0.08, rot_deg=2.0, empty=(), around=None,
                     quat_scale=None):
    """Synthetic input of the lidar local-map build (LidarMapping::viewer, reference src/LidarMapping.cc:130-185): n_keyframes
    key-frames along a random walk through a Scene (starting at the camera-to-world pose `around`, default a small random one), each
    with its stored pose Tcw as a float quaternion (x, y, z, w) and translation, and its downsampled cloud rendered from that pose
    (camera frame, about n_cloud points).
      empty: key-frames whose cloud is empty;
      quat_scale: [n_keyframes] factors on the stored quaternions (not exactly unit: SE3f's constructor normalises).
    Returns q [K][4], t [K][3], clouds (list), cloud_begin [K + 1], cloud [n][3] (float32)."""
    rng = np.random.default_rng(seed + 0x71D)
    sc = Scene(seed)
    T = random_motion(rng, trans=0.05, rot_deg=2.0) if around is None else np.array(around, np.float64)
    q, t, clouds = [], [], []
    for k in range(n_keyframes):
        if k:
            T = T @ random_motion(rng, trans, rot_deg)
        Rcw, tcw = T[:3, :3].T, -T[:3, :3].T @ T[:3, 3]
        qk = _quat_from_R(Rcw).astype(np.float32)
        if quat_scale is not None:
            qk = (qk * np.float32(quat_scale[k])).astype(np.float32)
        q.append(qk)
        t.append(tcw.astype(np.float32))
        if k in empty:
            clouds.append(np.zeros((0, 3), np.float32))
            continue
        _, d = sc.render(width, height, T, 400 + k)
        c = depth_to_cloud(d, 1)[:, :3].astype(np.float32)
        if len(c) > n_cloud:
            c = c[np.sort(rng.choice(len(c), n_cloud, replace=False))]
        clouds.append(np.ascontiguousarray(c, np.float32))
    return dict(q=np.array(q, np.float32).reshape(-1, 4), t=np.array(t, np.float32).reshape(-1, 3), clouds=clouds,
                cloud_begin=np.r_[0, np.cumsum([len(c) for c in clouds])].astype(np.int32),
                cloud=np.ascontiguousarray(np.concatenate(clouds), np.float32).reshape(-1, 3))


def triangulation_problem(seed, n_kp=1000, n_neighbours=10, n_nodes=100, n_kp_neighbour=None, mono_frac=0.3, has_mp_frac=0.3,
                          node_perturb=0.1, noise_px=0.6, bad_depth_frac=0.0, scale_factor=1.2, n_levels=8, width=640, height=480,
                          only_stereo=False, coarse=False, check_orientation=False, inertial=False, far_points=False, th_far_points=6.0,
                          shuffle_lists=True):
    """One LocalMapping::CreateNewMapPoints problem (gfs_tri_problem; api.tri_structs): a current key frame and n_neighbours
    neighbours that see one shared scene of world points.  Per view: key-points with pixel noise, octaves that follow the depth,
    descriptors a few bits from their world point's (points of one vocabulary node share a family, so wrong pairs and equal
    distances occur), node ids shared through the world point with a share perturbed, a share of mono key-points and a share with
    has_mp set, baselines above mb, ep / F12 computed in float32 with the reference's expressions.  bad_depth_frac: stereo
    key-points whose depth is not positive (UnprojectStereo fails)."""
    from .api import KP_DTYPE
    rng = np.random.default_rng(seed)
    f32 = np.float32
    fx, fy, cx, cy = (f32(v) for v in intrinsics(width, height))
    mb = f32(0.0745)
    mbf = f32(mb * fx)
    n_nb_kp = n_kp if n_kp_neighbour is None else n_kp_neighbour
    n_world = max(int(1.4 * max(n_kp, n_nb_kp)), 8)
    ids = 3 * np.arange(max(n_nodes, 1)) + 1  # vocabulary node ids (not consecutive)
    w_node = rng.integers(0, max(n_nodes, 1), n_world)
    fam = rng.integers(0, 256, (max(n_nodes, 1), 32), dtype=np.uint8)
    bits = np.unpackbits(fam[w_node], axis=1)
    for i in range(n_world):
        bits[i, rng.choice(256, rng.integers(8, 22), replace=False)] ^= 1
    w_bits = bits
    w_angle = rng.uniform(0, 360, n_world)
    # the world points in front of the current camera (identity-ish), 0.8 .. 9 m
    z = rng.uniform(0.8, 9.0, n_world)
    w_xyz = np.stack([(rng.uniform(0, width, n_world) - cx) / fx * z, (rng.uniform(0, height, n_world) - cy) / fy * z, z], 1)
    scale = (f32(scale_factor) ** np.arange(n_levels)).astype(f32)
    sigma2 = (scale * scale).astype(f32)

    def view(n, T_wc, is_cur):
        R, t = T_wc[:3, :3].T, -T_wc[:3, :3].T @ T_wc[:3, 3]  # Tcw
        Tcw = np.concatenate([R, t[:, None]], 1).astype(f32)
        R32, t32 = Tcw[:, :3], Tcw[:, 3]
        Pc = w_xyz @ R.T + t
        u, v = fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy
        vis = np.nonzero((Pc[:, 2] > 0.3) & (u > 8) & (u < width - 8) & (v > 8) & (v < height - 8))[0]
        pick = rng.permutation(vis)[:n]
        kps_un, kps = np.zeros(n, KP_DTYPE), np.zeros(n, KP_DTYPE)
        m = len(pick)
        x = np.concatenate([u[pick] + noise_px * rng.standard_normal(m), rng.uniform(8, width - 8, n - m)])
        y = np.concatenate([v[pick] + noise_px * rng.standard_normal(m), rng.uniform(8, height - 8, n - m)])
        zz = np.concatenate([Pc[pick, 2], rng.uniform(0.8, 9.0, n - m)])
        oct_ = np.clip(np.round(np.log(zz / 1.2) / np.log(scale_factor)) + rng.integers(-1, 2, n), 0, n_levels - 1).astype(np.int32)
        kps_un["x"], kps_un["y"], kps_un["octave"] = x, y, oct_
        kps_un["angle"] = np.concatenate([(w_angle[pick] + 6 * rng.standard_normal(m)) % 360, rng.uniform(0, 360, n - m)])
        kps_un["size"] = 31 * scale[oct_]
        kps[:] = kps_un
        kps["x"], kps["y"] = kps_un["x"] + f32(0.25), kps_un["y"] - f32(0.125)  # (mvKeys: before undistortion)
        mono = rng.random(n) < mono_frac
        depth = (zz * (1 + 0.004 * rng.standard_normal(n))).astype(f32)
        u_right = (kps_un["x"] - mbf / depth).astype(f32)
        u_right[mono], depth[mono] = -1, -1
        if bad_depth_frac > 0:
            depth[(rng.random(n) < bad_depth_frac) & ~mono] = 0
        db = np.concatenate([w_bits[pick], rng.integers(0, 2, (n - m, 256), dtype=np.uint8)])
        flip = rng.random((n, 256)) < rng.uniform(0, 0.05, (n, 1))
        desc = np.packbits(db ^ flip.astype(np.uint8), axis=1)
        node = np.concatenate([w_node[pick], rng.integers(0, max(n_nodes, 1), n - m)])
        pert = rng.random(n) < node_perturb
        node[pert] = rng.integers(0, max(n_nodes, 1), int(pert.sum()))
        nid = ids[node] if n else np.zeros(0, np.int64)
        if n and n_nodes > 2:
            nid = np.where(node == rng.integers(0, n_nodes), nid + 1, nid)  # one node this view has under an id of its own
        order = rng.permutation(n)  # key-point indices differ from view to view
        kps_un, kps, u_right, depth, desc, nid = kps_un[order], kps[order], u_right[order], depth[order], desc[order], nid[order]
        node_id = np.unique(nid).astype(np.int32)
        lists = [np.nonzero(nid == k)[0] for k in node_id]
        if shuffle_lists:
            lists = [rng.permutation(l) for l in lists]
        node_start = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
        feat_idx = (np.concatenate(lists) if lists else np.zeros(0)).astype(np.int32)
        Ow = (-(R32.T @ t32)).astype(f32)
        return dict(Tcw=Tcw.reshape(-1), Ow=Ow, Rwc=np.ascontiguousarray(R32.T).reshape(-1), twc=Ow.copy(), fx=fx, fy=fy, cx=cx, cy=cy,
                    invfx=f32(1) / fx, invfy=f32(1) / fy, mbf=mbf, mb=mb, scale_factors=scale, level_sigma2=sigma2, n_levels=n_levels,
                    kps_un=kps_un, kps=kps, u_right=u_right, depth=depth, desc=desc,
                    has_mp=(rng.random(n) < has_mp_frac).astype(np.uint8), node_id=node_id, node_start=node_start, feat_idx=feat_idx)

    T0 = random_motion(rng, trans=0.05, rot_deg=2.0)
    cur = view(n_kp, T0, True)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)
    Kinv = np.linalg.inv(K.astype(np.float64)).astype(f32)
    R1, t1 = cur["Tcw"].reshape(3, 4)[:, :3], cur["Tcw"].reshape(3, 4)[:, 3]
    neighbours = []
    for i in range(n_neighbours):
        T = random_motion(rng, trans=0.0, rot_deg=4.0)
        d = rng.standard_normal(3)
        d[2] *= 0.3
        T[:3, 3] = T0[:3, 3] + d / np.linalg.norm(d) * rng.uniform(0.12, 0.5)  # baseline above mb
        nb = view(n_nb_kp, T, False)
        R2, t2 = nb["Tcw"].reshape(3, 4)[:, :3], nb["Tcw"].reshape(3, 4)[:, 3]
        C2 = (R2 @ cur["Ow"] + t2).astype(f32)
        nb["ep"] = np.array([fx * C2[0] / C2[2] + cx, fy * C2[1] / C2[2] + cy], f32)
        R12 = (R1 @ R2.T).astype(f32)
        t12 = (t1 - R12 @ t2).astype(f32)
        tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]], f32)
        nb["F12"] = (((Kinv.T @ tx).astype(f32) @ R12).astype(f32) @ Kinv).astype(f32).reshape(-1)
        neighbours.append(nb)
    return dict(cur=cur, neighbours=neighbours, only_stereo=only_stereo, coarse=coarse, check_orientation=check_orientation, inertial=inertial,
                far_points=far_points, th_far_points=f32(th_far_points), ratio_factor=f32(f32(1.5) * f32(scale_factor)))


def _flip_bits(rng, desc, n_bits):
    """Copies of the 32-byte descriptors with n_bits[i] distinct random bits of row i flipped."""
    bits = np.unpackbits(np.asarray(desc, np.uint8).reshape(-1, 32), axis=1)
    order = np.argsort(rng.random(bits.shape), axis=1)
    flip = np.zeros(bits.shape, bool)
    np.put_along_axis(flip, order, np.arange(256)[None, :] < np.asarray(n_bits)[:, None], axis=1)
    return np.packbits(bits ^ flip, axis=1)


def _bow_lists(rng, node_of, shuffle_lists):
    """A feature vector from the node id of every key-point: (node_id ascending, node_start, feat_idx)."""
    ids = np.unique(node_of)
    lists = []
    for v in ids:
        l = np.nonzero(node_of == v)[0]
        lists.append(rng.permutation(l) if shuffle_lists else l)
    start = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    feat = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
    return ids.astype(np.int32), start, feat


def bow_search_problem(seed, n_kp=1000, n_kf2=1, n_nodes=100, n_kp2=None, no_mp_frac=0.15, dup_frac=0.08, shuffle_lists=True,
                       one_sided_frac=0.1, max_flip_bits=70, wrong_node_frac=0.1, angle_outlier_frac=0.2, nn_ratio=0.9,
                       check_orientation=True):
    """Synthetic input of ORBmatcher::SearchByBoW(pKF1, pKF2, ...) (reference src/ORBmatcher.cc:936-1053) for one key frame 1 and
    n_kf2 key frames 2, as gfs_search_by_bow takes it (include/gfs_abi.h): dict(kf1, kf2 = [...], nn_ratio, check_orientation), a
    key frame being dict(angle, desc, has_mp, node_id, node_start, feat_idx).  The descriptors of a key frame 2 are copies of key
    frame 1's with 0..max_flip_bits bits flipped, so that the best distances land on both sides of TH_LOW and of the ratio.
      no_mp_frac      the share of key-points without a (good) map point, in every key frame
      dup_frac        the share of key-points whose descriptor is a copy of another one's of the same node (within a few bits in key
                      frame 1: two idx1 want one idx2; exact in key frame 2: equal best and second-best distances)
      shuffle_lists   the per-node lists in random order instead of ascending index order
      one_sided_frac  the share of a key frame's nodes whose id the other key frame does not have
      wrong_node_frac the share of key-points of a key frame 2 filed under another node than their source's
      angle_outlier_frac  the share of key-points of a key frame 2 whose angle is unrelated to their source's"""
    rng = np.random.default_rng(seed)
    n2 = n_kp if n_kp2 is None else n_kp2
    f32 = np.float32
    ids = np.sort(rng.choice(max(4 * n_nodes, 8), n_nodes, replace=False)).astype(np.int32) * 2  # even ids; private nodes get odd ones

    def duplicate(desc, node_of, flips):
        """dup_frac of the rows become copies of another row of their node with 0..flips bits flipped"""
        n = len(desc)
        for i in np.nonzero(rng.random(n) < dup_frac)[0]:
            same = np.nonzero(node_of == node_of[i])[0]
            src = int(same[rng.integers(len(same))])
            if src != i:
                desc[i] = _flip_bits(rng, desc[src:src + 1], [int(rng.integers(flips + 1))])[0]
        return desc

    def one_sided(node_of):
        """moves the key-points of one_sided_frac of the nodes to ids nobody else has"""
        for v in np.unique(node_of):
            if rng.random() < one_sided_frac:
                node_of[node_of == v] = v + 1
        return node_of

    node1 = ids[rng.integers(n_nodes, size=n_kp)] if n_kp else np.zeros(0, np.int32)
    desc1 = duplicate(rng.integers(0, 256, (n_kp, 32)).astype(np.uint8), node1, 3)
    ang1 = (rng.random(n_kp) * 360).astype(f32)
    nid, ns, fi = _bow_lists(rng, one_sided(node1.copy()), shuffle_lists)
    kf1 = dict(angle=ang1, desc=desc1, has_mp=(rng.random(n_kp) >= no_mp_frac).astype(np.uint8), node_id=nid, node_start=ns, feat_idx=fi)
    kf2 = []
    for _ in range(n_kf2):
        if n_kp == 0 or n2 == 0:
            src = np.zeros(n2, np.int64)
            desc2, node2, ang2 = rng.integers(0, 256, (n2, 32)).astype(np.uint8), ids[rng.integers(n_nodes, size=n2)], (rng.random(n2) * 360).astype(f32)
        else:
            src = rng.permutation(np.arange(n2) % n_kp)
            desc2 = _flip_bits(rng, desc1[src], rng.integers(0, max_flip_bits + 1, n2))
            node2 = node1[src].copy()
            wrong = rng.random(n2) < wrong_node_frac
            node2[wrong] = ids[rng.integers(n_nodes, size=int(wrong.sum()))]
            desc2 = duplicate(desc2, node2, 0)
            turn = f32(rng.random() * 360)
            ang2 = ((ang1[src] - turn + rng.normal(0, 4, n2)) % 360).astype(f32)
            out = rng.random(n2) < angle_outlier_frac
            ang2[out] = (rng.random(int(out.sum())) * 360).astype(f32)
        nid, ns, fi = _bow_lists(rng, one_sided(node2.copy()), shuffle_lists)
        kf2.append(dict(angle=ang2, desc=desc2, has_mp=(rng.random(n2) >= no_mp_frac).astype(np.uint8), node_id=nid, node_start=ns, feat_idx=fi))
    return dict(kf1=kf1, kf2=kf2, nn_ratio=f32(nn_ratio), check_orientation=bool(check_orientation))


def bow_vocabulary(seed, k=10, L=4, stop_frac=0.0, prune_frac=0.0, shuffle_children=False, level_flip_bits=(90, 60, 40, 28, 20, 14, 10, 8, 6, 4)):
    """A random vocabulary tree as gfs_bow_create takes it (gfs_bow_vocabulary in include/gfs_abi.h): dict(k, L, scoring = 0 (L1_NORM),
    weighting = 0 (TF_IDF), n_nodes, parent, child_start, children, desc [n_nodes, 32], weight, word_id).  Every inner node has k
    children; a child's descriptor is its parent's with about level_flip_bits[level - 1] bits flipped, so a feature near a leaf
    descends to it and siblings tie now and then.
      prune_frac        the share of the nodes of levels 1 .. L-1 that become leaves early (an irregular tree)
      shuffle_children  the node ids (all but the root's) and the word ids are random permutations: child ids are neither contiguous
                        nor ascending, as no text file can give them
      stop_frac         the share of the words with weight 0 (stopped); the others carry log(N / n_i)-like positive doubles"""
    rng = np.random.default_rng(seed + 49979687)
    parent, level_of, desc, leaf = [np.zeros(1, np.int64)], [np.zeros(1, np.int64)], [rng.integers(0, 256, (1, 32)).astype(np.uint8)], [np.zeros(1, bool)]
    inner, n = np.zeros(1, np.int64), 1  # the inner nodes of the level above, the nodes so far
    for lev in range(1, L + 1):
        m = len(inner) * k
        if m == 0:
            break
        par = np.repeat(inner, k)
        src = desc[0][par]
        flips = np.clip(rng.normal(level_flip_bits[lev - 1], 3, m).round().astype(np.int64), 0, 256)
        d = _flip_bits(rng, src, flips)
        is_leaf = np.ones(m, bool) if lev == L else rng.random(m) < prune_frac
        parent.append(par), level_of.append(np.full(m, lev)), desc.append(d), leaf.append(is_leaf)
        inner = n + np.nonzero(~is_leaf)[0]
        n += m
        desc = [np.concatenate(desc)]
    parent, desc, leaf = np.concatenate(parent), np.concatenate(desc), np.concatenate(leaf)
    n_words = int(leaf.sum())
    perm = np.arange(n)
    word_of_leaf = np.arange(n_words)
    if shuffle_children:
        perm[1:] = 1 + rng.permutation(n - 1)
        word_of_leaf = rng.permutation(n_words)
    counts = np.bincount(parent[1:], minlength=n)
    first = np.concatenate([[1], 1 + np.cumsum(counts)[:-1]])  # the first child of every node in the contiguous numbering
    cnt_new = np.zeros(n, np.int64)
    cnt_new[perm] = counts
    child_start = np.concatenate([[0], np.cumsum(cnt_new)])
    children = np.zeros(n - 1, np.int64)
    c = np.arange(1, n)
    children[child_start[perm[parent[c]]] + (c - first[parent[c]])] = perm[c]
    out_parent, out_desc, out_word, out_weight = np.zeros(n, np.int32), np.zeros((n, 32), np.uint8), np.full(n, -1, np.int32), np.zeros(n)
    out_parent[perm] = perm[parent]
    out_desc[perm] = desc
    N = 10000.0
    w = np.log(N / rng.integers(1, 5000, n_words))
    w[rng.random(n_words) < stop_frac] = 0.0
    leaves = np.nonzero(leaf)[0]
    out_word[perm[leaves]] = word_of_leaf
    out_weight[perm[leaves]] = w
    return dict(k=k, L=L, scoring=0, weighting=0, n_nodes=n, parent=out_parent, child_start=child_start.astype(np.int32),
                children=children.astype(np.int32), desc=out_desc, weight=out_weight, word_id=out_word)


def bow_features(seed, vocab, n, max_flip_bits=12, dup_frac=0.0):
    """n descriptors [n, 32] for gfs_bow_transform: leaf descriptors of `vocab` with 0..max_flip_bits bits flipped; dup_frac of them are
    exact copies of another feature, so that several features fall into one word."""
    rng = np.random.default_rng(seed + 15485863)
    leaves = np.nonzero(np.asarray(vocab["word_id"]) >= 0)[0]
    d = _flip_bits(rng, np.asarray(vocab["desc"], np.uint8)[leaves[rng.integers(len(leaves), size=n)]], rng.integers(0, max_flip_bits + 1, n)) \
        if n else np.zeros((0, 32), np.uint8)
    for i in np.nonzero(rng.random(n) < dup_frac)[0]:
        d[i] = d[int(rng.integers(n))]
    return np.ascontiguousarray(d, np.uint8)


def map_point_update_problem(seed, n_points=1000,obs_counts=(1, 20), n_keyframes=40, flip_bits=40, scale_factor=1.2, n_levels=8):
    """Synthetic input of MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:376-448,
    :468-532) for `n_points` map points, as gfs_map_points_update takes it (include/gfs_abi.h): a dict with the keys of
    gfs_map_points_problem.  obs_counts: the observations per point, an int, an inclusive (lo, hi) range or one count per point.

    Camera centres are drawn per key frame; a point's observations are key frames in ascending index (the pointer order of
    mObservations), distinct while there are enough.  A descriptor is the point's base pattern with 0..`flip_bits` random bits
    flipped, so rows tie in their median and the best row is rarely the first.  One observation in twelve is IN_NORMAL only (a bad
    key frame, or an index beyond mDescriptors.rows), one in thirty carries neither flag (leftIndex == -1), and every 17th point has
    no IN_DESC observation at all.  The reference key frame is one of the point's own observations."""
    rng = np.random.default_rng(seed + 32452843)
    if np.isscalar(obs_counts):
        counts = np.full(n_points, int(obs_counts), np.int64)
    elif isinstance(obs_counts, tuple) and len(obs_counts) == 2:
        counts = rng.integers(obs_counts[0], obs_counts[1] + 1, size=n_points)
    else:
        counts = np.asarray(obs_counts, np.int64)
        assert len(counts) == n_points
    obs_start = np.zeros(n_points + 1, np.int32)
    obs_start[1:] = np.cumsum(counts)
    n_obs = int(obs_start[-1])
    kf_Ow = (rng.normal(size=(n_keyframes, 3)) * [1.5, 0.3, 1.5]).astype(np.float32)
    pos = (rng.uniform([-4, -1.5, 2], [4, 1.5, 9], size=(n_points, 3))).astype(np.float32)
    scale = np.cumprod(np.r_[1.0, np.full(n_levels - 1, float(scale_factor))]).astype(np.float32)
    obs_kf = np.zeros(n_obs, np.int32)
    obs_desc = np.zeros((n_obs, 32), np.uint8)
    obs_flags = np.zeros(n_obs, np.uint8)
    ref_Ow = np.zeros((n_points, 3), np.float32)
    level_scale = np.ones(n_points, np.float32)
    for p in range(n_points):
        a, n = int(obs_start[p]), int(counts[p])
        kfs = np.sort(rng.choice(n_keyframes, size=n, replace=n > n_keyframes))
        obs_kf[a:a + n] = kfs
        base = np.unpackbits(rng.integers(0, 256, size=32, dtype=np.uint8))
        for i in range(n):
            bits = base.copy()
            k = int(rng.integers(0, flip_bits + 1))
            if k:
                bits[rng.choice(256, size=k, replace=False)] ^= 1
            obs_desc[a + i] = np.packbits(bits)
        r = rng.random(n)
        fl = np.where(r < 1 / 30, 0, np.where(r < 1 / 30 + 1 / 12, 1, 3)).astype(np.uint8)
        if p % 17 == 16:
            fl &= 1
        obs_flags[a:a + n] = fl
        ref_Ow[p] = kf_Ow[kfs[int(rng.integers(0, n))]] if n else kf_Ow[int(rng.integers(0, n_keyframes))]
        level_scale[p] = scale[int(rng.integers(0, n_levels))]
    return dict(obs_start=obs_start, obs_kf=obs_kf, obs_Ow=kf_Ow[obs_kf].reshape(-1, 3).copy(), obs_desc=obs_desc, obs_flags=obs_flags,
                pos=pos, ref_Ow=ref_Ow, level_scale=level_scale, max_scale=np.full(n_points, scale[-1], np.float32))


def clahe_image(seed, width, height):
    """A frame for the CLAHE tests: a low-contrast sinusoid under Gaussian noise of sigma 12 plus a nearly flat patch of 4 grey
    values.  The narrow histogram puts every tile of an 8 x 8 grid over the clip limit of 3.0 once tiles hold a few hundred pixels
    and the patch makes single bins exceed it many times over, so the redistributed excess takes many sizes (a residual below and
    above 128 both occur); a tile of one pixel clips nothing.  -> [height, width] u8."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    img = 118.0 + 22.0 * np.sin(0.11 * x + 0.3 * seed) * np.cos(0.07 * y + 0.2 * seed) + rng.normal(0.0, 12.0, (height, width))
    ph, pw, y0, x0 = max(height // 3, 1), max(width // 3, 1), height // 4, width // 2
    img[y0:y0 + ph, x0:x0 + pw] = 96 + rng.integers(0, 4, img[y0:y0 + ph, x0:x0 + pw].shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _quat_xyzw(R):
    """unit quaternion (x, y, z, w), w >= 0, of a rotation matrix"""
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-6:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:  # half a turn: the axis from the diagonal
        x, y, z = np.sqrt(np.maximum(0.0, (np.diag(R) + 1) / 2))
        q = np.array([x, np.copysign(y, R[0, 1]), np.copysign(z, R[0, 2]), 0.0])
    return q / np.linalg.norm(q)


def pose_graph(seed, n_keyframes, fix_scale=True, drift=0.05, loop=0, icp_edges=False, n_corrected=3, points_per_kf=20, radius=5.0):
    """Synthetic input of Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:2042-2413), flattened the way the adaptor
    flattens a map: a closed ring of `n_keyframes` key-frames (2 `radius` m across) whose odometry accumulated about `drift` radians
    of heading error and 2 % of scale error by the time the last key-frame sees key-frame `loop` again.  The current key-frame and its
    n_corrected - 1 predecessors are already corrected (CorrectedSim3: their estimates, with the loop's scale when fix_scale is
    off); every edge that touches them is measured on their drifted poses (NonCorrectedSim3), every other estimate is the drifted
    pose with scale 1.  Edges in the reference's order: the loop connections (:2147-2186), then per key-frame the spanning-tree edge
    to its predecessor, one older loop edge (with icp_edges followed by its ICP edge, information 3 I: :2266-2288), and the
    covisibility edge to the key-frame two back unless a loop connection already joins the pair.  Key-frame 0 is the map's init
    key-frame (fixed).  Map points sit in front of their reference key-frames' drifted poses; every 16th has no reference (-1).
    -> dict for api.EssentialGraphOptimizer.OptimizeEssentialGraph, plus true_R / true_t (world -> camera) and kind [E] (0 loop
    connection, 1 spanning tree, 2 loop edge, 3 ICP, 4 covisibility)."""
    rng = np.random.default_rng(seed)
    n = int(n_keyframes)
    assert n >= 6 and 0 <= loop < n - n_corrected - 2
    # world -> camera of the truth: centres on the ring, heading along it, a small wobble
    Rt, tt = [], []
    for k in range(n):
        a = 2 * np.pi * k / n
        Rwc = _rot(*(0.05 * rng.uniform(-1, 1, 3))) @ _rot(0, 0, a + np.pi / 2)
        c = np.array([radius * np.cos(a), radius * np.sin(a), 0.2 * rng.uniform(-1, 1)])
        Rt.append(Rwc.T)
        tt.append(-Rwc.T @ c)
    # the map's poses: the true relative motions with a heading bias, noise and a scale error, chained from key-frame 0
    Rd, td = [Rt[0]], [tt[0]]
    for k in range(1, n):
        Rrel, trel = Rt[k] @ Rt[k - 1].T, tt[k] - Rt[k] @ Rt[k - 1].T @ tt[k - 1]
        Rn = _rot(*(drift / n * np.array([0.2 * rng.normal(), 0.2 * rng.normal(), 1.0 + 0.3 * rng.normal()])))
        Rrel, trel = Rn @ Rrel, 1.02 * trel + 0.002 * rng.normal(size=3)
        Rd.append(Rrel @ Rd[k - 1])
        td.append(Rrel @ td[k - 1] + trel)

    def mul(a, b):  # Sim3 as (R, t, s): x -> s R x + t
        return a[0] @ b[0], a[2] * (a[0] @ b[1]) + a[1], a[2] * b[2]

    def inv(a):
        return a[0].T, -(a[0].T @ a[1]) / a[2], 1.0 / a[2]

    non_corrected = [(Rd[k], td[k], 1.0) for k in range(n)]
    cur = n - 1
    s_c = 1.0 if fix_scale else float(1.0 + 0.08 * rng.uniform(0.5, 1.0))
    cur_corr = (_rot(*(0.002 * rng.normal(size=3))) @ Rt[cur], s_c * (tt[cur] + 0.005 * rng.normal(size=3)), s_c)
    corrected = {k: mul(mul(non_corrected[k], inv(non_corrected[cur])), cur_corr) for k in range(n - n_corrected, n)}
    scw = [corrected.get(k, non_corrected[k]) for k in range(n)]
    drifted = lambda k: non_corrected[k]  # (NonCorrectedSim3 where there is one, else vScw: the same Sim3 here)

    edges = []  # (i, j, measurement, weight, kind)
    inserted = set()
    loop_connections = {cur: [loop, loop + 1], cur - 1: [loop]}
    for i in sorted(loop_connections):
        for j in loop_connections[i]:
            edges.append((i, j, mul(scw[j], inv(scw[i])), 1.0, 0))
            inserted.add((min(i, j), max(i, j)))
    old_i, old_l = n // 2, 1
    for i in range(n):
        Swi = inv(drifted(i))
        if i >= 1:
            edges.append((i, i - 1, mul(drifted(i - 1), Swi), 1.0, 1))
        if i == old_i and old_l < i - 2:
            Sli = mul(drifted(old_l), Swi)
            edges.append((i, old_l, Sli, 1.0, 2))
            if icp_edges:
                icp = (_rot(*(0.003 * rng.normal(size=3))) @ Sli[0], Sli[1] / Sli[2] + 0.01 * rng.normal(size=3), 1.0)
                edges.append((i, old_l, icp, 3.0, 3))
        if i >= 2 and (i - 2, i) not in inserted:
            edges.append((i, i - 2, mul(drifted(i - 2), Swi), 1.0, 4))

    pts, ref = [], []
    for k in range(n):
        p_cam = np.stack([rng.uniform(-1, 1, points_per_kf), rng.uniform(-0.5, 0.5, points_per_kf), rng.uniform(1, 4, points_per_kf)], 1)
        pts.append((p_cam - td[k]) @ Rd[k])  # Rd^T (p - t)
        ref.append(np.full(points_per_kf, k))
    pts, ref = np.concatenate(pts).astype(np.float32), np.concatenate(ref).astype(np.int32)
    ref[::16] = -1
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return dict(vertex_q=np.stack([_quat_xyzw(S[0]) for S in scw]), vertex_t=np.stack([S[1] for S in scw]),
                vertex_s=np.array([S[2] for S in scw]), vertex_fixed=fixed,
                edge_i=np.array([e[0] for e in edges], np.int32), edge_j=np.array([e[1] for e in edges], np.int32),
                edge_q=np.stack([_quat_xyzw(e[2][0]) for e in edges]), edge_t=np.stack([e[2][1] for e in edges]),
                edge_s=np.array([e[2][2] for e in edges]), edge_w=np.array([e[3] for e in edges]),
                fix_scale=bool(fix_scale), iterations=20, lambda_init=1e-16, points=pts, point_ref=ref,
                kind=np.array([e[4] for e in edges], np.int32), true_R=np.stack(Rt), true_t=np.stack(tt))


def sim3_opt_problem(seed, n_pairs=150, fix_scale=True, outlier_share=0.15, noise_px=0.7, th2=10.0, rot_deg=2.0, trans=0.05,
                     scale=None, estimate_rot_deg=0.5, estimate_trans=0.02, estimate_scale=0.01, outlier_px=40.0, n_levels=8,
                     scale_factor=1.2, width=640, height=480):
    """Synthetic input of Optimizer::OptimizeSim3 (reference src/Optimizer.cc:2797-3054), flattened the way the adaptor flattens two
    key frames: camera 1 and camera 2 see `n_pairs` common points, x1 = s R x2 + t with the true S12 = (R, t, s) (s = 1 with fix_scale
    unless `scale` is given, else a few percent off 1); x1c / x2c are the points in the two camera frames computed in float and cast
    to double as the reference does, the observations their projections plus noise_px of Gaussian noise, rounded to float like
    cv::KeyPoint, each at a random pyramid level with inv_sigma2 = scale_factor^(-2 level).  A share of the pairs are gross outliers
    (one observation moved by about outlier_px).  The estimate handed in is the truth perturbed by estimate_rot_deg / estimate_trans
    (and estimate_scale when the scale is free).  -> dict for api.Sim3Optimizer.OptimizeSim3, plus true_s12 [8] and outlier [n]."""
    rng = np.random.default_rng(seed)
    n = int(n_pairs)
    fx, fy, cx, cy = (float(np.float32(v)) for v in intrinsics(width, height))
    s_true = float(scale) if scale is not None else (1.0 if fix_scale else float(1.0 + 0.05 * rng.uniform(-1, 1)))
    R = _rot(*(np.deg2rad(rot_deg) * rng.uniform(-1, 1, 3)))
    t = trans * rng.uniform(-1, 1, 3)
    u, v, z = rng.uniform(20, width - 20, n), rng.uniform(20, height - 20, n), rng.uniform(1.0, 6.0, n)
    x2 = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1).astype(np.float32).reshape(n, 3)
    x1 = (s_true * (x2.astype(np.float64) @ R.T) + t).astype(np.float32).reshape(n, 3)
    x1c, x2c = x1.astype(np.float64), x2.astype(np.float64)

    def project(x):
        return np.stack([fx * x[:, 0] / x[:, 2] + cx, fy * x[:, 1] / x[:, 2] + cy], 1).reshape(n, 2)

    obs1, obs2 = project(x1c) + noise_px * rng.normal(size=(n, 2)), project(x2c) + noise_px * rng.normal(size=(n, 2))
    outlier = rng.random(n) < outlier_share
    side = rng.random(n) < 0.5
    kick = outlier_px * (1.0 + rng.random((n, 2))) * rng.choice([-1.0, 1.0], (n, 2))
    obs1[outlier & side] += kick[outlier & side]
    obs2[outlier & ~side] += kick[outlier & ~side]
    obs1, obs2 = obs1.astype(np.float32).astype(np.float64), obs2.astype(np.float32).astype(np.float64)
    sigma2 = (np.float32(scale_factor) ** np.arange(n_levels, dtype=np.float32)) ** 2
    inv_sigma2 = (np.float32(1.0) / sigma2).astype(np.float32)
    w1, w2 = inv_sigma2[rng.integers(0, n_levels, n)], inv_sigma2[rng.integers(0, n_levels, n)]
    Re = _rot(*(np.deg2rad(estimate_rot_deg) * rng.uniform(-1, 1, 3))) @ R
    te = t + estimate_trans * rng.uniform(-1, 1, 3)
    se = s_true if fix_scale else s_true * float(1.0 + estimate_scale * rng.uniform(-1, 1))
    return dict(s12=np.concatenate([_quat_xyzw(Re), te, [se]]), cam1=np.array([fx, fy, cx, cy]), cam2=np.array([fx, fy, cx, cy]),
                th2=float(np.float32(th2)), fix_scale=bool(fix_scale), x1c=x1c, x2c=x2c, obs1=obs1, obs2=obs2,
                inv_sigma2_1=np.ascontiguousarray(w1, np.float32), inv_sigma2_2=np.ascontiguousarray(w2, np.float32),
                true_s12=np.concatenate([_quat_xyzw(R), t, [s_true]]), outlier=outlier)


def sim3_ransac_iterations(n_pairs, probability=0.99, min_inliers=6, max_iterations=300):
    """Sim3Solver::SetRansacParameters (reference src/Sim3Solver.cc:119-143) evaluated directly: epsilon a float, the rest in double."""
    n, m = int(n_pairs), int(min_inliers)
    if m == n:
        return 1
    with np.errstate(all="ignore"):
        eps = np.float64(np.float32(m) / np.float32(n)) if n else np.float64(np.inf)
        v = np.ceil(np.log(1 - np.float64(probability)) / np.log(1 - eps ** 3))
    its = int(v) if np.isfinite(v) and abs(v) < 2 ** 31 else -2 ** 31  # x86-64's answer for a NaN or a value beyond int
    return max(1, min(its, int(max_iterations)))


def sim3_ransac_problem(seed, n_pairs=150, inlier_share=0.6, fix_scale=True, noise_px=0.5, min_inliers=15, n_iterations=None,
                        probability=0.99, max_iterations=300, rot_deg=25.0, trans=0.8, scale=None, n_levels=8, scale_factor=1.2,
                        width=640, height=480):
    """Synthetic input of Sim3Solver (reference src/Sim3Solver.cc), flattened as its constructor leaves it: two clouds of `n_pairs`
    points in the frames of camera 1 and camera 2, x1 = s R x2 + t with a known S12 = (R, t, s) (s = 1 with fix_scale unless `scale`
    is given) plus noise of about noise_px pixels at the point's depth; a share 1 - inlier_share of the pairs are outliers (x1 is
    another point of the frustum).  Each pair sits at a random pyramid level; its thresholds are mvnMaxError as the reference compares
    them, (float)(size_t)(9.210 * sigma2).  draws [n_iterations, 3]: r0 in [0, n-1], r1 in [0, n-2], r2 in [0, n-3], as
    DUtils::Random::RandomInt would return them; n_iterations defaults to SetRansacParameters(probability, min_inliers,
    max_iterations).  -> dict for api.Sim3RansacSolver.solve, plus true_R / true_t / true_s and outlier [n]."""
    rng = np.random.default_rng(seed)
    n = int(n_pairs)
    f32 = np.float32
    fx, fy, cx, cy = (float(f32(v)) for v in intrinsics(width, height))
    s_true = float(scale) if scale is not None else (1.0 if fix_scale else float(1.0 + 0.2 * rng.uniform(-1, 1)))
    R = _rot(*(np.deg2rad(rot_deg) * rng.uniform(-1, 1, 3)))
    t = trans * rng.uniform(-1, 1, 3)

    def frustum(k):
        u, v, z = rng.uniform(20, width - 20, k), rng.uniform(20, height - 20, k), rng.uniform(1.0, 6.0, k)
        return np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1).reshape(k, 3)

    x2 = frustum(n)
    x1 = s_true * (x2 @ R.T) + t
    x1 += noise_px / fx * np.abs(x1[:, 2:3]) * rng.normal(size=(n, 3))
    outlier = rng.random(n) >= inlier_share
    x1[outlier] = frustum(int(outlier.sum()))
    sigma2 = (f32(scale_factor) ** np.arange(n_levels, dtype=f32)) ** 2
    max_err = np.floor(9.210 * sigma2.astype(np.float64)).astype(f32)  # a vector<size_t> in the reference: truncated
    H = sim3_ransac_iterations(n, probability, min_inliers, max_iterations) if n_iterations is None else int(n_iterations)
    draws = np.zeros((H, 3), np.int32)
    if n >= 3:
        draws = np.stack([rng.integers(0, n - k, H) for k in range(3)], 1).astype(np.int32)
    return dict(x3d_c1=x1.astype(f32), x3d_c2=x2.astype(f32), max_err1=max_err[rng.integers(0, n_levels, n)],
                max_err2=max_err[rng.integers(0, n_levels, n)], cam1=np.array([fx, fy, cx, cy], f32), cam2=np.array([fx, fy, cx, cy], f32),
                fix_scale=bool(fix_scale), min_inliers=int(min_inliers), n_iterations=H, draws=draws, true_R=R, true_t=t, true_s=s_true,
                outlier=outlier)


def _exp_so3(w):
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + W
    return np.eye(3) + np.sin(th) / th * W + (1 - np.cos(th)) / th ** 2 * (W @ W)


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _spd(rng, diag, mix=0.05):
    """A dense symmetric positive definite matrix with the given eigenvalues, turned a little away from the axes."""
    n = len(diag)
    Q, _ = np.linalg.qr(np.eye(n) + mix * rng.normal(size=(n, n)))
    M = Q @ np.diag(np.asarray(diag, np.float64)) @ Q.T
    return (M + M.T) / 2


POSE_INERTIAL_LAST_KEYFRAME, POSE_INERTIAL_LAST_FRAME = 0, 1  # GFS_POSE_INERTIAL_* (include/gfs_abi.h)


def pose_inertial_problem(seed, mode, n_obs=300, outlier_share=0.15, stereo_share=0.85, preint_noise=1.0, inconsistent=False, n_rounds=4,
                          rec_init=False, dt=None, outlier_px=25.0, pose_error=1.0, depth=(1.0, 14.0), start=None):
    """Synthetic Optimizer::PoseInertialOptimizationLastKeyFrame (mode 0) / ...LastFrame (mode 1) problem (include/gfs_abi.h section 19):
    a body that turns and accelerates for `dt` seconds between the other end of the inertial edge (the last key frame, or the previous
    frame) and the current frame; a preintegration made from that motion with noise `preint_noise` times its covariance
    (`inconsistent`: off by several degrees and decimetres a second, so that chi2IMU > 15 -- the knob for the 1e-2 branch);
    `n_obs` map points seen from the true current pose, pixel noise by octave, `outlier_share` gross outliers (a share near 1 is
    the knob for few inliers), `stereo_share` with depth.  The current frame's estimate starts `pose_error` times a
    motion-model error away from the truth.  `start` (Rwb, twb, v, bg, ba): the true state of the other end, to chain problems.
    Returns the fields of gfs_pose_inertial_problem plus the truth."""
    rng = np.random.default_rng(seed)
    frame = mode == POSE_INERTIAL_LAST_FRAME
    dt = float(np.float32((0.05 if frame else 0.4) if dt is None else dt))
    g = np.array([0.0, 0.0, -float(np.float32(9.81))])
    fx = fy = np.float64(np.float32(607.0))
    cx, cy = np.float64(np.float32(319.5)), np.float64(np.float32(239.5))
    bf = np.float64(np.float32(0.0745 * 607.0))
    # camera <- body: the camera looks along the body's x, with a small mounting error; floats widened, as Sophus::SE3f mTcb is
    Rcb = _f32(np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]]) @ _rot(*(0.02 * rng.normal(size=3))))
    tcb = _f32(0.05 * rng.normal(size=3))
    Rbc, tbc = Rcb.T.copy(), _f32(-Rcb.T @ tcb)
    # the true motion
    Rwb1 = _rot(0.05 * rng.normal(), 0.05 * rng.normal(), rng.uniform(-np.pi, np.pi))
    p1, v1 = rng.uniform(-2, 2, 3), np.array([0.8, 0.1, 0.02]) * rng.normal(size=3)
    omega, acc = 0.4 * rng.normal(size=3), 0.8 * rng.normal(size=3)
    bg_true, ba_true = 0.002 * rng.normal(size=3), 0.02 * rng.normal(size=3)
    if start is not None:
        Rwb1, p1, v1, bg_true, ba_true = (np.asarray(start[k], np.float64) for k in ("Rwb", "twb", "v", "bg", "ba"))
        if "Rcb" in start:  # the same mounting along a chain
            Rcb, tcb = _f32(start["Rcb"]), _f32(start["tcb"])
            Rbc, tbc = Rcb.T.copy(), _f32(-Rcb.T @ tcb)
    Rwb2 = Rwb1 @ _exp_so3(omega * dt)
    v2, p2 = v1 + acc * dt, p1 + v1 * dt + 0.5 * acc * dt * dt
    # the preintegration: the ideal deltas, noise, plausible bias Jacobians, the bias it was integrated with
    sr, sv, sp = 1e-3 * np.sqrt(dt / 0.05), 4e-3 * np.sqrt(dt / 0.05), 1e-3 * np.sqrt(dt / 0.05)
    nr, nv, npos = preint_noise * sr * rng.normal(size=3), preint_noise * sv * rng.normal(size=3), preint_noise * sp * rng.normal(size=3)
    if inconsistent:
        nr, nv = nr + np.deg2rad(4.0) * rng.choice([-1, 1], 3), nv + 0.3 * rng.choice([-1, 1], 3)
    dR = Rwb1.T @ Rwb2 @ _exp_so3(nr)
    dV = Rwb1.T @ (v2 - v1 - g * dt) + nv
    dP = Rwb1.T @ (p2 - p1 - v1 * dt - 0.5 * g * dt * dt) + npos
    JRg = -dt * (np.eye(3) + 0.05 * rng.normal(size=(3, 3)))
    JVa = -dt * (np.eye(3) + 0.05 * rng.normal(size=(3, 3)))
    JPa = -0.5 * dt * dt * (np.eye(3) + 0.05 * rng.normal(size=(3, 3)))
    JVg, JPg = 0.3 * dt * dt * rng.normal(size=(3, 3)), 0.1 * dt ** 3 * rng.normal(size=(3, 3))
    pre_bg, pre_ba = (bg_true + 1e-4 * rng.normal(size=3)).astype(np.float32), (ba_true + 1e-3 * rng.normal(size=3)).astype(np.float32)
    info_inertial = _spd(rng, np.r_[np.full(3, sr ** -2), np.full(3, sv ** -2), np.full(3, sp ** -2)], 0.02)
    info_gyro_rw = _spd(rng, np.full(3, 1.0 / (1e-4 ** 2 * dt)), 0.02)
    info_acc_rw = _spd(rng, np.full(3, 1.0 / (1e-3 ** 2 * dt)), 0.02)

    def state(Rwb, p, v, bg, ba):  # as ImuCamPose(Frame*) leaves it: floats widened, the camera pose from the float pose
        Rwb, p = _f32(Rwb), _f32(p)
        Rcw = _f32(Rcb @ Rwb.T)
        tcw = _f32(Rcb @ (-Rwb.T @ p) + tcb)
        return dict(Rwb=Rwb, twb=p, Rcw=Rcw, tcw=tcw, v=_f32(v), bg=_f32(bg), ba=_f32(ba))

    e1 = 0.1 if frame else 0.0  # the previous frame's estimate is an optimised one; the key frame is fixed
    other = state(Rwb1 @ _exp_so3(e1 * 0.002 * rng.normal(size=3)), p1 + e1 * 0.005 * rng.normal(size=3), v1 + e1 * 0.01 * rng.normal(size=3),
                  bg_true + 1e-4 * rng.normal(size=3), ba_true + 1e-3 * rng.normal(size=3))
    cur = state(Rwb2 @ _exp_so3(pose_error * 0.008 * rng.normal(size=3)), p2 + pose_error * 0.02 * rng.normal(size=3),
                v2 + pose_error * 0.05 * rng.normal(size=3), other["bg"], other["ba"])
    prior_H = _spd(rng, np.r_[np.full(3, 2e4), np.full(3, 1e4), np.full(3, 4e2), np.full(3, 1e6), np.full(3, 1e4)], 0.02)
    # the map points, seen from the true current camera
    Rcw_t, tcw_t = Rcb @ Rwb2.T, Rcb @ (-Rwb2.T @ p2) + tcb
    sigma2 = np.float64(np.float32(1.2) ** (2 * np.arange(8)))
    inv_sigma2 = (np.float32(1.0) / np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
    xw, obs, w = np.zeros((n_obs, 3)), np.zeros((n_obs, 3)), np.zeros(n_obs, np.float32)
    st, close, is_out = np.zeros(n_obs, np.uint8), np.zeros(n_obs, np.uint8), np.zeros(n_obs, bool)
    k = 0
    while k < n_obs:
        z = rng.uniform(*depth)
        xc = np.array([rng.uniform(-0.5, 0.5) * z, rng.uniform(-0.38, 0.38) * z, z])
        u, v = fx * xc[0] / xc[2] + cx, fy * xc[1] / xc[2] + cy
        if not (0 <= u < 640 and 0 <= v < 480):
            continue
        octv = int(rng.choice(8, p=np.array([217, 181, 151, 126, 105, 87, 73, 60]) / 1000.0))
        noise = rng.normal(0, np.sqrt(sigma2[octv]), 3)
        is_out[k] = rng.random() < outlier_share
        if is_out[k]:
            noise[:2] += rng.choice([-1, 1], 2) * outlier_px
        st[k] = rng.random() < stereo_share
        xw[k] = _f32(Rcw_t.T @ (xc - tcw_t))
        obs[k] = [np.float32(u + noise[0]), np.float32(v + noise[1]), np.float32(u - bf / z + noise[2]) if st[k] else -1.0]
        w[k] = inv_sigma2[octv]
        close[k] = np.float32(z) < np.float32(10.0)
        k += 1
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(mode=int(mode), n_obs=int(n_obs), n_rounds=int(n_rounds), rec_init=int(bool(rec_init)), xw=xw, obs=obs, inv_sigma2=w, stereo=st,
                close=close, fx=fx, fy=fy, cx=cx, cy=cy, bf=bf, Rcb=Rcb, tcb=tcb, Rbc=Rbc, tbc=tbc, cur=cur, other=other,
                dR=f32(dR), dV=f32(dV), dP=f32(dP), JRg=f32(JRg), JVg=f32(JVg), JVa=f32(JVa), JPg=f32(JPg), JPa=f32(JPa), preint_bg=pre_bg,
                preint_ba=pre_ba, dT=np.float32(dt), info_inertial=info_inertial, info_gyro_rw=info_gyro_rw, info_acc_rw=info_acc_rw,
                prior_Rwb=other["Rwb"].copy(), prior_twb=other["twb"].copy(), prior_vwb=other["v"].copy(), prior_bg=other["bg"].copy(),
                prior_ba=other["ba"].copy(), prior_H=prior_H, is_outlier=is_out,
                truth=dict(Rwb=Rwb2, twb=p2, v=v2, bg=bg_true, ba=ba_true))


def pose_lidar_inertial_problem(seed, mode, n_obs=300, n_cloud=600, voxel=0.1, kf_time_gap=0.4, map_shift=0.0, start=None, n_keyframes=3,
                                width=320, height=240, prior_scale=1.0, **kw):
    """Synthetic Optimizer::PoseLidarVisualInertialOptimizationLastKeyFrame (mode 0) / ...LastFrame (mode 1) problem (include/gfs_abi.h
    section 21): a pose_inertial_problem (`kw` and `start` go to it) put on a Scene.  The frame cloud is the scene seen from the TRUE
    current camera, about `n_cloud` points in camera coordinates; the local map is `n_keyframes` renders from nearby poses carried
    into the problem's world and voxel-averaged at `voxel` metres, as pose_lidar_frame builds them, then moved by `map_shift` metres
    along every axis (a large shift: no point gets an edge).  `prior_scale` multiplies the previous frame's prior: 1e6 holds that frame
    still, so that in frame mode an `inconsistent` preintegration stays in the inertial edge (chi2IMU > 15).  Returns the fields of
    gfs_pose_lidar_inertial_problem plus map_xyz and the truth."""
    p = pose_inertial_problem(seed, mode, n_obs=n_obs, start=start, **kw)
    p["prior_H"] = p["prior_H"] * float(prior_scale)
    rng = np.random.default_rng(seed + 0x51D)
    sc = Scene(seed)
    Rwb, twb = p["truth"]["Rwb"], p["truth"]["twb"]
    Rcb, tcb = p["Rcb"], p["tcb"]
    T_wc = np.eye(4)  # world <- camera, at the truth
    T_wc[:3, :3] = (Rcb @ Rwb.T).T
    T_wc[:3, 3] = -T_wc[:3, :3] @ (Rcb @ (-Rwb.T @ twb) + tcb)
    S_c = random_motion(rng, trans=0.05, rot_deg=2.0)  # scene <- camera
    A = T_wc @ np.linalg.inv(S_c)  # world <- scene
    pts = []
    for k in range(n_keyframes):
        S_kf = S_c @ random_motion(rng, trans=0.15, rot_deg=4.0)
        _, d = sc.render(width, height, S_kf, 100 + k)
        c = depth_to_cloud(d, 2)[:, :3].astype(np.float64)
        c = c @ S_kf[:3, :3].T + S_kf[:3, 3]
        pts.append(c @ A[:3, :3].T + A[:3, 3])
    map_xyz = voxel_average(np.concatenate(pts), voxel) + np.float32(map_shift)
    cloud = np.zeros((0, 3), np.float32)
    if n_cloud > 0:
        _, d = sc.render(width, height, S_c, 7)
        cloud = depth_to_cloud(d, 1)[:, :3]
        assert len(cloud) >= n_cloud, (len(cloud), n_cloud)
        cloud = cloud[np.sort(rng.choice(len(cloud), n_cloud, replace=False))]
    cur = p["cur"]
    p.update(q=_quat_from_R(cur["Rcw"]).astype(np.float32), t=cur["tcw"].astype(np.float32), tcb_q=_quat_from_R(Rcb).astype(np.float32),
             tcb_t=tcb.astype(np.float32), kf_time_gap=float(kf_time_gap), cloud=np.ascontiguousarray(cloud, np.float32), map_xyz=map_xyz)
    return p


def lba_inertial_window(seed, n_opt=10, n_fixed=5, n_points=300, stereo_share=0.85, outlier_share=0.05, large=False, inconsistent=(),
                        single_mono_points=0, fixed_heavy_points=0, pose_error=1.0, point_error=1.0, obs_per_point=(3, 7), outlier_px=25.0,
                        dt=0.4, preint_noise=1.0, noise_scale=1.0, iterations=None, lambda_init=None):
    """Synthetic Optimizer::LocalInertialBA window (include/gfs_abi.h section 20): a body on a smooth trajectory (angular rate and
    acceleration drift slowly from one key-frame interval to the next) sampled every `dt` seconds; key frame 0 is the newest, key frame
    n_opt - 1 the oldest of the window, `prev` the fixed one in front of it, and `n_fixed` further fixed key frames stand near the
    start of the trajectory.  Each interval's preintegration is made from the true motion as pose_inertial_problem makes it, with
    noise `preint_noise` times its covariance; `inconsistent`: the edge sets whose preintegration is off by several degrees and
    decimetres a second.  `n_points` map points in front of the window, each observed from `obs_per_point` key frames in a random
    order (at least one of them in the window), `stereo_share` of the observations with depth, pixel noise by octave times
    `noise_scale`,
    `outlier_share` gross outliers.  Knobs for the degenerate cases: `single_mono_points` further points with ONE mono observation,
    `fixed_heavy_points` further points seen from one window key frame and otherwise only from fixed ones.  The window's estimates start
    `pose_error` times a motion-model error from the truth, the points `point_error` times 2 cm.  `large`: the bLarge settings
    (4 iterations, lambda 1e-2).  Returns the fields of gfs_lba_inertial_problem plus the truth and is_outlier per edge."""
    rng = np.random.default_rng(seed)
    N, F = int(n_opt), int(n_fixed)
    dt = float(np.float32(dt))
    g = np.array([0.0, 0.0, -float(np.float32(9.81))])
    fx = fy = np.float64(np.float32(607.0))
    cx, cy = np.float64(np.float32(319.5)), np.float64(np.float32(239.5))
    bf = np.float64(np.float32(0.0745 * 607.0))
    Rcb = _f32(np.array([[0.0, -1, 0], [0, 0, -1], [1, 0, 0]]) @ _rot(*(0.02 * rng.normal(size=3))))
    tcb = _f32(0.05 * rng.normal(size=3))
    Rbc, tbc = Rcb.T.copy(), _f32(-Rcb.T @ tcb)
    # the true trajectory at times 0 (prev) .. N (key frame 0)
    R = [_rot(0.05 * rng.normal(), 0.05 * rng.normal(), rng.uniform(-np.pi, np.pi))]
    p, v = [rng.uniform(-2, 2, 3)], [np.array([0.5, 0.1, 0.02]) * rng.normal(size=3)]
    omega, acc = 0.06 * rng.normal(size=3), 0.4 * rng.normal(size=3)  # slow turns: the window's key frames share their view
    bg_true, ba_true = 0.002 * rng.normal(size=3), 0.02 * rng.normal(size=3)
    steps = []
    for k in range(N):
        omega, acc = omega + 0.015 * rng.normal(size=3), acc + 0.08 * rng.normal(size=3)
        steps.append((omega.copy(), acc.copy()))
        R.append(R[k] @ _exp_so3(omega * dt))
        v.append(v[k] + acc * dt)
        p.append(p[k] + v[k] * dt + 0.5 * acc * dt * dt)

    def state(Rwb, pp, vv, bg, ba):
        Rwb, pp = _f32(Rwb), _f32(pp)
        return dict(Rwb=Rwb, twb=pp, Rcw=_f32(Rcb @ Rwb.T), tcw=_f32(Rcb @ (-Rwb.T @ pp) + tcb), v=_f32(vv), bg=_f32(bg), ba=_f32(ba))

    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    sr, sv, sp = 1e-3 * np.sqrt(dt / 0.05), 4e-3 * np.sqrt(dt / 0.05), 1e-3 * np.sqrt(dt / 0.05)
    inertial = [None] * N
    for k in range(N):  # the interval from time k to k + 1 is edge set N - 1 - k
        i = N - 1 - k
        nr, nv, npos = preint_noise * sr * rng.normal(size=3), preint_noise * sv * rng.normal(size=3), preint_noise * sp * rng.normal(size=3)
        if i in tuple(inconsistent):
            nr, nv = nr + np.deg2rad(4.0) * rng.choice([-1, 1], 3), nv + 0.3 * rng.choice([-1, 1], 3)
        JRg = -dt * (np.eye(3) + 0.05 * rng.normal(size=(3, 3)))
        JVa = -dt * (np.eye(3) + 0.05 * rng.normal(size=(3, 3)))
        JPa = -0.5 * dt * dt * (np.eye(3) + 0.05 * rng.normal(size=(3, 3)))
        JVg, JPg = 0.3 * dt * dt * rng.normal(size=(3, 3)), 0.1 * dt ** 3 * rng.normal(size=(3, 3))
        inertial[i] = dict(dR=f32(R[k].T @ R[k + 1] @ _exp_so3(nr)), dV=f32(R[k].T @ (v[k + 1] - v[k] - g * dt) + nv),
                           dP=f32(R[k].T @ (p[k + 1] - p[k] - v[k] * dt - 0.5 * g * dt * dt) + npos), JRg=f32(JRg), JVg=f32(JVg), JVa=f32(JVa),
                           JPg=f32(JPg), JPa=f32(JPa), preint_bg=(bg_true + 1e-4 * rng.normal(size=3)).astype(np.float32),
                           preint_ba=(ba_true + 1e-3 * rng.normal(size=3)).astype(np.float32), dT=np.float32(dt),
                           info_inertial=_spd(rng, np.r_[np.full(3, sr ** -2), np.full(3, sv ** -2), np.full(3, sp ** -2)], 0.02),
                           info_gyro_rw=_spd(rng, np.full(3, 1.0 / (1e-4 ** 2 * dt)), 0.02),
                           info_acc_rw=_spd(rng, np.full(3, 1.0 / (1e-3 ** 2 * dt)), 0.02))
    prev = state(R[0], p[0], v[0], bg_true + 1e-4 * rng.normal(size=3), ba_true + 1e-3 * rng.normal(size=3))
    truth, window = [], []
    for i in range(N):
        k = N - i
        truth.append(dict(Rwb=R[k], twb=p[k], v=v[k], bg=bg_true, ba=ba_true))
        window.append(state(R[k] @ _exp_so3(pose_error * 0.008 * rng.normal(size=3)), p[k] + pose_error * 0.02 * rng.normal(size=3),
                            v[k] + pose_error * 0.05 * rng.normal(size=3), prev["bg"] + 1e-5 * rng.normal(size=3),
                            prev["ba"] + 1e-4 * rng.normal(size=3)))
    # the other fixed key frames: earlier poses beside the start of the trajectory, looking the same way
    fixed_R, fixed_p = [], []
    for k in range(F):
        fixed_R.append(R[0] @ _exp_so3(0.05 * rng.normal(size=3)))
        fixed_p.append(p[0] + 0.3 * rng.normal(size=3))
    cams = []  # true camera poses by key-frame index: the window, prev, the fixed ones
    for i in range(N):
        cams.append((Rcb @ R[N - i].T, Rcb @ (-R[N - i].T @ p[N - i]) + tcb))
    cams.append((prev["Rcw"], prev["tcw"]))
    fixed_Rcw, fixed_tcw = np.zeros((F, 3, 3)), np.zeros((F, 3))
    for k in range(F):
        Rwb, pp = _f32(fixed_R[k]), _f32(fixed_p[k])
        fixed_Rcw[k], fixed_tcw[k] = _f32(Rcb @ Rwb.T), _f32(Rcb @ (-Rwb.T @ pp) + tcb)
        cams.append((fixed_Rcw[k], fixed_tcw[k]))
    K = N + 1 + F
    sigma2 = np.float64(np.float32(1.2) ** (2 * np.arange(8)))
    inv_sigma2 = (np.float32(1.0) / np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
    pts_true, pts, begin = [], [], [0]
    edge_kf, obs, w, st, close, is_out = [], [], [], [], [], []

    def observe(xw_true, kf, mono, outlier_ok=True):
        Rcw, tcw = cams[kf]
        xc = Rcw @ xw_true + tcw
        if xc[2] < 0.5:
            return False
        u, vv = fx * xc[0] / xc[2] + cx, fy * xc[1] / xc[2] + cy
        if not (0 <= u < 640 and 0 <= vv < 480):
            return False
        octv = int(rng.choice(8, p=np.array([217, 181, 151, 126, 105, 87, 73, 60]) / 1000.0))
        noise = noise_scale * rng.normal(0, np.sqrt(sigma2[octv]), 3)
        out = outlier_ok and rng.random() < outlier_share
        if out:
            noise[:2] += rng.choice([-1, 1], 2) * outlier_px
        stereo = (not mono) and rng.random() < stereo_share
        edge_kf.append(kf), w.append(inv_sigma2[octv]), st.append(stereo), is_out.append(out)
        obs.append([np.float32(u + noise[0]), np.float32(vv + noise[1]), np.float32(u - bf / xc[2] + noise[2]) if stereo else -1.0])
        return True

    kinds = ["normal"] * int(n_points) + ["single_mono"] * int(single_mono_points) + ["fixed_heavy"] * int(fixed_heavy_points)
    for kind in kinds:
        while True:
            home = int(rng.integers(0, N))
            z = rng.uniform(1.5, 14.0)
            xc = np.array([rng.uniform(-0.4, 0.4) * z, rng.uniform(-0.3, 0.3) * z, z])
            xw_true = _f32(cams[home][0].T @ (xc - cams[home][1]))
            n0 = len(edge_kf)
            if kind == "single_mono":
                order = [home]
            elif kind == "fixed_heavy":
                order = [home] + [N + int(k) for k in rng.permutation(F + 1)[:max(1, min(F + 1, 4))]]
                order = [order[k] for k in rng.permutation(len(order))]
            else:
                others = [k for k in rng.permutation(K) if k != home][:int(rng.integers(obs_per_point[0], obs_per_point[1] + 1)) - 1]
                order = [home] + [int(k) for k in others]
                order = [order[k] for k in rng.permutation(len(order))]
            for kf in order:
                observe(xw_true, kf, kind == "single_mono", kind == "normal")
            if home in edge_kf[n0:]:
                break
            del edge_kf[n0:], obs[n0:], w[n0:], st[n0:], is_out[n0:]
        zc = (cams[0][0] @ xw_true + cams[0][1])[2]
        close += [np.float32(zc) < np.float32(10.0)] * (len(edge_kf) - n0)
        pts_true.append(xw_true)
        pts.append(_f32(xw_true + point_error * 0.02 * rng.normal(size=3)))
        begin.append(len(edge_kf))
    n_pts = len(pts)
    return dict(n_opt=N, n_fixed=F, n_points=n_pts, n_edges=len(edge_kf), iterations=int((4 if large else 8) if iterations is None else iterations),
                n_cameras=1, lambda_init=float((1e-2 if large else 1e0) if lambda_init is None else lambda_init), fx=fx, fy=fy, cx=cx, cy=cy, bf=bf,
                Rcb=Rcb, tcb=tcb, Rbc=Rbc, tbc=tbc, window=window, window_imu=np.ones(N, np.uint8), prev=prev, fixed_Rcw=fixed_Rcw,
                fixed_tcw=fixed_tcw, inertial=inertial, points=np.array(pts, np.float64).reshape(n_pts, 3),
                point_edge_begin=np.array(begin, np.int32), edge_kf=np.array(edge_kf, np.int32), obs=np.array(obs, np.float64).reshape(-1, 3),
                inv_sigma2=np.array(w, np.float32), stereo=np.array(st, np.uint8), close=np.array(close, np.uint8),
                is_outlier=np.array(is_out, bool), large=bool(large), truth=dict(window=truth, points=np.array(pts_true).reshape(n_pts, 3)))
