"""Plain numpy restatements of the three frame helpers and the input builders shared by test_frame_gms_references.py (CPU: the
restatements against the C++ oracle, and the conditions every case must keep meeting) and test_gpu_frame_batched.py (device).

The restatements follow the reference line by line, one numpy operation per reference operation, all in float32:
  cloud_ref   Frame::ConvertDepthToPointCloud  src/Frame.cc:590-623    if (depth > 0.0 && depth < 10.0) (u - cx) * depth / fx
  stereo_ref  Frame::ComputeStereoFromRGBD     src/Frame.cc:1314-1332  imDepth.at<float>(v, u) with float v, u (truncation)
  u16_ref     imDepth.convertTo(CV_32F, f)     src/Tracking.cc:1622-1623
Everything is compared on bit patterns (bits()); there is no tolerance anywhere."""
import numpy as np

f32 = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
SENTINEL = 0xDEADBEEF  # bit pattern every output buffer is filled with before a call (as float32: -6.26e18, as int32: negative)
F10 = f32(10.0)
BELOW10, ABOVE10 = np.nextafter(F10, f32(0)), np.nextafter(F10, f32(20))
FLT_MIN = np.finfo(f32).tiny
# depth values the reference's two tests treat specially; the last five exercise fp32 subnormals (inputs and products)
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0, 10.0, BELOW10, ABOVE10, 1e-45, 1e-40, 3e-39, FLT_MIN, 1e-30], f32)
BF = f32(0.0745 * 607.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sentinel(shape, dtype=np.float32):
    return np.full(shape, SENTINEL, np.uint32).view(dtype)


def is_subnormal(a):
    a = np.abs(np.asarray(a, f32))
    return (a > 0) & (a < FLT_MIN)


def intrinsics(rows, cols):
    return f32(cols * 0.948 + 0.1), f32(cols * 0.951 + 0.2), f32(cols / 2 - 0.37), f32(rows / 2 + 0.21)


def cloud_ref(depth, ds, fx, fy, cx, cy):
    """-> [n, 4] float32 in push_back (raster) order"""
    depth = np.asarray(depth, f32)
    fx, fy, cx, cy = f32(fx), f32(fy), f32(cx), f32(cy)
    with np.errstate(all="ignore"):
        d = depth[::ds, ::ds]
        v, u = np.meshgrid(np.arange(0, depth.shape[0], ds), np.arange(0, depth.shape[1], ds), indexing="ij")
        ok = (d > 0.0) & (d < 10.0)
        d, u, v = d[ok], u[ok], v[ok]
        x = (u.astype(f32) - cx) * d / fx
        y = (v.astype(f32) - cy) * d / fy
        out = np.stack([x, y, d, np.ones_like(d)], 1).astype(f32)
    assert x.dtype == f32 and y.dtype == f32
    return out


def stereo_ref(kps, kps_un_x, depth, bf):
    """-> (mvuRight, mvDepth); kps_un_x None: the undistorted x is the key-point's own"""
    depth = np.asarray(depth, f32)
    with np.errstate(all="ignore"):
        iu, iv = kps["x"].astype(np.int32), kps["y"].astype(np.int32)
        d = depth[iv, iu]
        pos = d > 0
        xu = kps["x"] if kps_un_x is None else np.asarray(kps_un_x, f32)
        ur = np.where(pos, xu - f32(bf) / d, f32(-1))
        vd = np.where(pos, d, f32(-1))
    assert ur.dtype == f32 and vd.dtype == f32
    return ur, vd


def u16_ref(raw, factor):
    return raw.astype(f32) * f32(factor)


# ---------------------------------------------------------------------------------------------------------------- cloud cases
# name -> (cols, rows, ds); the grid totals sit on and around the 1024 samples one round of the kernel takes
CLOUD_SHAPES = {
    "32x32": (32, 32, 1),      # exactly 1024 samples
    "33x31": (33, 31, 1),      # 1023
    "41x25": (41, 25, 1),      # 1025: a second round of one sample
    "53x37s3": (53, 37, 3),    # the stride divides neither side
    "7x5s9": (7, 5, 9),        # one sample
    "1x1": (1, 1, 1),
    "1x40": (1, 40, 1),
    "320x240s2": (320, 240, 2),  # 19200 samples: 19 rounds of the carry
}
CLOUD_BATCHES = (2, 5, 17)
_KINDS = ("none", "all", "last_round", "random", "specials")


def grid_mask(rows, cols, ds):
    m = np.zeros((rows, cols), bool)
    m[::ds, ::ds] = True
    return m


def cloud_frame(kind, rows, cols, ds, rng):
    """One depth map.  Off the sample grid every kind holds a mix of valid depths and SPECIALS: they must change nothing."""
    on = grid_mask(rows, cols, ds)
    d = rng.uniform(0.3, 9.5, (rows, cols)).astype(f32)
    off_special = ~on & (rng.random((rows, cols)) < 0.3)
    d[off_special] = rng.choice(SPECIALS, int(off_special.sum()))
    g = d[::ds, ::ds].copy()
    total = g.size
    if kind == "none":
        g[:] = rng.choice(np.array([0.0, -0.0, -1.0, 10.0, ABOVE10, np.nan, np.inf], f32), g.shape)
    elif kind == "last_round":
        flat = g.reshape(-1)
        flat[:((total - 1) // 1024) * 1024] = 0
    elif kind == "random":
        g[rng.random(g.shape) < 0.35] = 0
    elif kind == "specials":
        flat = g.reshape(-1)
        k = max(1, min(total // 5, 200))
        flat[rng.choice(total, k, replace=False)] = np.resize(SPECIALS, k)
    d[::ds, ::ds] = g
    return d


def cloud_batch(name, B):
    """-> (depth [B, rows, cols], ds, (fx, fy, cx, cy), kinds).  Frame b is of kind _KINDS[b % 5]: a batch of 5 or 17 holds an
    empty frame, a full one and one whose valid samples all lie in the last 1024-sample round; a batch of 2 holds the first two."""
    cols, rows, ds = CLOUD_SHAPES[name]
    rng = np.random.default_rng(1000 + 31 * B + sorted(CLOUD_SHAPES).index(name))
    kinds = [_KINDS[b % len(_KINDS)] for b in range(B)]
    depth = np.stack([cloud_frame(k, rows, cols, ds, rng) for k in kinds])
    return depth, ds, intrinsics(rows, cols), kinds


def special_depth_case(which):
    """3(c): 200 special values scattered onto the samples of a 32 x 32 map ('dense', ds 1) / 60 onto the 18 x 13 samples of a
    53 x 37 map with ds 3 ('strided': specials off the grid too).  The intrinsics put the principal point on the map, so
    subnormal depths times a small (u - cx) stay subnormal and non-zero."""
    cols, rows, ds, k = (32, 32, 1, 200) if which == "dense" else (53, 37, 3, 60)
    rng = np.random.default_rng(77 if which == "dense" else 78)
    d = rng.uniform(0.3, 9.5, (rows, cols)).astype(f32)
    on = grid_mask(rows, cols, ds)
    off_special = ~on & (rng.random((rows, cols)) < 0.5)
    d[off_special] = rng.choice(SPECIALS, int(off_special.sum()))
    g = d[::ds, ::ds].copy()
    flat = g.reshape(-1)
    flat[rng.choice(flat.size, k, replace=False)] = np.resize(SPECIALS, k)  # every special at least k // 14 times
    d[::ds, ::ds] = g
    return d, ds, intrinsics(rows, cols)


# --------------------------------------------------------------------------------------------------------------- stereo cases
STEREO_BATCHES = (1, 4)
STEREO_STRIDES = (1, 255, 256, 257, 1000)
STEREO_ROWS, STEREO_COLS = 37, 53
# depths planted under key-points: <= 0, -0.0, NaN, +inf, subnormals (bf / d overflows: mvuRight = -inf), the largest finite
STEREO_SPECIALS = np.array([0.0, -0.0, -1.0, np.nan, np.inf, 1e-40, 1e-45, 3e-39, FLT_MIN, 1e-30], f32)


def stereo_counts(B, kp_stride):
    if B == 1:
        return np.array([max(1, 3 * kp_stride // 4)], np.int32)
    return np.resize(np.array([kp_stride, 0, max(1, kp_stride // 2), max(1, kp_stride - 1)], np.int32), B)


def stereo_case(B, kp_stride):
    """-> dict(depth [B, rows, cols], kps [B, kp_stride], unx [B, kp_stride], counts [B], bf).
    Every coordinate truncates into the image: fractional up to cols - 0.01 / rows - 0.01, and x, y in (-1, 0), which truncate
    to 0 where floor gives -1.  Entries at and beyond counts[b] hold in-image coordinates as well (nothing may come of them)."""
    rows, cols = STEREO_ROWS, STEREO_COLS
    rng = np.random.default_rng(500 + 7 * kp_stride + B)
    depth = rng.uniform(0.3, 12.0, (B, rows, cols)).astype(f32)
    depth[rng.random(depth.shape) < 0.15] = 0
    kps = np.zeros((B, kp_stride), KP_DTYPE)
    kps["x"] = rng.uniform(0, cols - 0.01, (B, kp_stride)).astype(f32)
    kps["y"] = rng.uniform(0, rows - 0.01, (B, kp_stride)).astype(f32)
    kps["x"] = np.minimum(kps["x"], f32(cols - 0.01))
    kps["y"] = np.minimum(kps["y"], f32(rows - 0.01))
    fixed = [(-0.5, -0.5), (cols - 0.01, rows - 0.01), (-0.999, 3.7), (5.2, -1e-3), (-1e-30, -0.25), (0.0, 0.0)]
    for b in range(B):
        for j, (x, y) in enumerate(fixed[:kp_stride]):
            kps["x"][b, j], kps["y"][b, j] = x, y
        neg = np.nonzero(rng.random(kp_stride) < 0.08)[0]
        neg = neg[neg >= len(fixed)]
        kps["x"][b, neg] = -rng.uniform(0.001, 0.999, len(neg)).astype(f32)
        neg = np.nonzero(rng.random(kp_stride) < 0.08)[0]
        neg = neg[neg >= len(fixed)]
        kps["y"][b, neg] = -rng.uniform(0.001, 0.999, len(neg)).astype(f32)
        for j, s in enumerate(STEREO_SPECIALS):  # plant the special depths under key-points len(fixed) + j
            i = len(fixed) + j
            if i < kp_stride:
                depth[b, int(kps["y"][b, i]), int(kps["x"][b, i])] = s
    kps["size"], kps["angle"], kps["octave"] = 31.0, 12.5, 1
    unx = (kps["x"] + rng.uniform(-3, 3, (B, kp_stride)).astype(f32)).astype(f32)
    unx[unx == kps["x"]] += f32(1)
    return dict(depth=depth, kps=kps, unx=unx, counts=stereo_counts(B, kp_stride), bf=BF, rows=rows, cols=cols)


def stereo_case_ref(case, with_unx):
    """-> (ur, vd) [B, kp_stride] as bit patterns, the sentinel at and beyond counts[b]"""
    B, S = case["kps"].shape
    ur, vd = sentinel((B, S)), sentinel((B, S))
    for b in range(B):
        n = int(case["counts"][b])
        ur[b, :n], vd[b, :n] = stereo_ref(case["kps"][b, :n], case["unx"][b, :n] if with_unx else None, case["depth"][b], case["bf"])
    return ur, vd


# ------------------------------------------------------------------------------------------------------------------ u16 cases
# n = B * rows * cols = 1, 3, 15, 63, 105, 1025, 2050, 4099: no multiple of 4, so every size ends in the scalar tail (of 1, 2 or 3
# elements); the first three sizes never reach the four-wide body, the last three span more than one workgroup of 1024 elements
U16_SHAPES = ((1, 1, 1), (3, 1, 1), (1, 3, 5), (1, 7, 9), (3, 5, 7), (1, 25, 41), (2, 25, 41), (1, 4099, 1))
U16_FACTORS = (1.0 / 5000.0, 0.001)


def u16_case(shape):
    rng = np.random.default_rng(int(np.prod(shape)))
    raw = rng.integers(0, 65536, shape, dtype=np.uint16)
    flat = raw.reshape(-1)
    flat[-1] = 65535
    if flat.size > 1:
        flat[0] = 0
    return raw
