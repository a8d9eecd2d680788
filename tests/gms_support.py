"""Plain numpy restatement of gms_matcher(...).GetInlierMask(mask, false, false) and the case builders shared by
test_frame_gms_references.py (CPU: restatement against the C++ oracle, and the conditions each case must keep meeting) and
test_gpu_gms_cases.py (device).  Masks are integers: every comparison is array_equal, there is no tolerance."""
import numpy as np

f32 = np.float32
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
W, H = 640, 480
CW, CH = W / 20, H / 20  # size of a grid cell of the default frame


def _nb9(idx):
    out = [-1] * 9
    ix, iy = idx % 20, idx // 20
    for yi in (-1, 0, 1):
        for xi in (-1, 0, 1):
            xx, yy = ix + xi, iy + yi
            if 0 <= xx < 20 and 0 <= yy < 20:
                out[xi + 4 + yi * 3] = xx + yy * 20
    return out


def gms_ref(kp1, size1, kp2, size2, q, t):
    """Thirdparty/GMS/include/gms_matcher.h of the reference: NormalizePoints (float / int), run(1) over the four shifted grids
    with AssignMatchPairs, VerifyCellPairs (rotation pattern 1, the identity) and the inlier marking, OR-ed together.
    A dense 400 x 400 vote matrix per grid; np.argmax takes the first maximum of a row, as the reference's `>` scan does.

    Indices outside the grids: a left index < 0 (x >= 20 or y >= 20 gives -1; a negative coordinate in row 0 gives < 0) or a
    right index < 0 casts no vote, as in the reference.  A right index >= 400 is skipped as well: the reference tests it
    (`rgidx >= mGridNumberRight`) before it touches the matrix.  A negative x in a row > 0 wraps into the previous row, as in the
    reference.  Marking: the reference compares mCellPairs[left] with the right index of EVERY match whose left index it can
    read, so a right index of -1 (-2) equals the -1 (-2) of a left cell without votes (below the threshold): an inlier.  For a
    left index < 0 the reference reads outside mCellPairs; like the oracle, that is taken as never equal.
    -> (mask bool [n_matches], n_inliers)"""
    q, t = np.asarray(q, np.int64), np.asarray(t, np.int64)
    n = len(q)
    mask = np.zeros(n, bool)
    if n == 0:
        return mask, 0
    x1, y1 = kp1["x"].astype(f32) / f32(size1[0]), kp1["y"].astype(f32) / f32(size1[1])
    x2, y2 = kp2["x"].astype(f32) / f32(size2[0]), kp2["y"].astype(f32) / f32(size2[1])
    lx, ly = x1[q] * f32(20), y1[q] * f32(20)  # pt.x * mGridSizeLeft.width: float * int -> float
    rx, ry = x2[t] * f32(20), y2[t] * f32(20)
    assert lx.dtype == f32 and rx.dtype == f32
    r = np.floor(rx).astype(np.int64) + np.floor(ry).astype(np.int64) * 20  # GetGridIndexRight: no range check
    for gtype in (1, 2, 3, 4):
        x = np.floor(lx) if gtype in (1, 3) else np.floor(lx.astype(np.float64) + 0.5)
        y = np.floor(ly) if gtype in (1, 2) else np.floor(ly.astype(np.float64) + 0.5)
        x, y = x.astype(np.int64), y.astype(np.int64)
        l = np.where((x >= 20) | (y >= 20), -1, x + y * 20)
        votes = (l >= 0) & (r >= 0) & (l < 400) & (r < 400)
        stats = np.zeros((400, 400), np.int64)
        np.add.at(stats, (l[votes], r[votes]), 1)
        npts = stats.sum(1)
        cell = np.full(400, -1, np.int64)
        for i in np.nonzero(npts)[0]:
            cell[i] = int(np.argmax(stats[i]))
            nl, nr = _nb9(int(i)), _nb9(int(cell[i]))
            score, thresh, numpair = 0, 0.0, 0
            for j in range(9):
                if nl[j] == -1 or nr[j] == -1:
                    continue
                score += int(stats[nl[j], nr[j]])
                thresh += float(npts[nl[j]])
                numpair += 1
            if score < 6 * np.sqrt(thresh / numpair):
                cell[i] = -2
        mask |= (l >= 0) & (cell[np.clip(l, 0, 399)] == r)
    return mask, int(mask.sum())


def grid_indices(kp1, size1, kp2, size2, q, t, gtype=1):
    """(left, right) cell index of every match for one shifted grid: what the conditions in the CPU file are stated in"""
    q, t = np.asarray(q, np.int64), np.asarray(t, np.int64)
    lx = (kp1["x"].astype(f32) / f32(size1[0]))[q] * f32(20)
    ly = (kp1["y"].astype(f32) / f32(size1[1]))[q] * f32(20)
    rx = (kp2["x"].astype(f32) / f32(size2[0]))[t] * f32(20)
    ry = (kp2["y"].astype(f32) / f32(size2[1]))[t] * f32(20)
    x = np.floor(lx) if gtype in (1, 3) else np.floor(lx.astype(np.float64) + 0.5)
    y = np.floor(ly) if gtype in (1, 2) else np.floor(ly.astype(np.float64) + 0.5)
    x, y = x.astype(np.int64), y.astype(np.int64)
    return np.where((x >= 20) | (y >= 20), -1, x + y * 20), np.floor(rx).astype(np.int64) + np.floor(ry).astype(np.int64) * 20


def _kps(x, y):
    kp = np.zeros(len(x), KP_DTYPE)
    kp["x"], kp["y"] = np.asarray(x, f32), np.asarray(y, f32)
    kp["size"], kp["octave"] = 31.0, 0
    return kp


def _case(kp1, kp2, q, t, size1=(W, H), size2=(W, H)):
    return dict(kp1=kp1, kp2=kp2, q=np.ascontiguousarray(q, np.int32), t=np.ascontiguousarray(t, np.int32), size1=size1, size2=size2)


def is_arange(c):
    """The device-resident entry takes match i = (i, train[i]) for every left key-point, both frames of one size"""
    return len(c["q"]) == len(c["kp1"]) and np.array_equal(c["q"], np.arange(len(c["q"]))) and c["size1"] == c["size2"] and len(c["kp2"]) > 0


def _in_cell(cx, cy, n, rng, lo=0.25, span=0.2):
    """n points in cell (cx, cy) of the default frame, at (c + lo .. c + lo + span) cells: with lo = 0.25 and span < 0.2 none of
    the four shifted grids (which round at c + 0.5) puts them anywhere but in cell c"""
    return (cx + lo + rng.uniform(0, span, n)) * CW, (cy + lo + rng.uniform(0, span, n)) * CH


# ------------------------------------------------------------------------------------------------------------------- 4(a) ties
TIE_BLOCK = [(cx, cy) for cy in (5, 6, 7) for cx in (5, 6, 7)]
TIE_PER_CELL = 222
TIE_OFFSETS = ((-3, 4), (6, 2))  # right-cell offset of the even / of the odd matches: the second has the LOWER cell index


def tie_case(swap=False, seed=1):
    """Every cell of a 3 x 3 block of left cells sends 111 matches to each of two right cells: a tie for the maximum of every row.
    Even matches go to offset (-3, +4), odd ones to (+6, +2), the lower index: the odd ones win.  swap=True exchanges the two."""
    rng = np.random.default_rng(seed)
    off_even, off_odd = TIE_OFFSETS[::-1] if swap else TIE_OFFSETS
    xs1, ys1, xs2, ys2 = [], [], [], []
    for cx, cy in TIE_BLOCK:
        x, y = _in_cell(cx, cy, TIE_PER_CELL, rng, 0.25, 0.19)
        k = np.arange(TIE_PER_CELL)
        ox = np.where(k % 2 == 0, off_even[0], off_odd[0])
        oy = np.where(k % 2 == 0, off_even[1], off_odd[1])
        xs1.append(x), ys1.append(y)
        xs2.append((cx + ox + 0.3 + rng.uniform(0, 0.4, TIE_PER_CELL)) * CW)
        ys2.append((cy + oy + 0.3 + rng.uniform(0, 0.4, TIE_PER_CELL)) * CH)
    kp1, kp2 = _kps(np.concatenate(xs1), np.concatenate(ys1)), _kps(np.concatenate(xs2), np.concatenate(ys2))
    n = len(kp1)  # 1998; match i of cell c is 222 c + k: even k <-> even i
    return _case(kp1, kp2, np.arange(n), np.arange(n))


# ---------------------------------------------------------------------------------------------------------------- 4(b) borders
def borders_case(seed=2):
    """3000 matches with coordinates from -5 to size + 5 on both sides: left x == width (cell index -1 for grid 1; 20 is also
    where grids 2 - 4 round the last half cell to), negative coordinates (wrap into the previous row / negative index), right
    points on y == height (r >= 400), far outside (|r| > 32767, beyond a short) and 40 % of the train indices random."""
    rng = np.random.default_rng(seed)
    n = 3000
    x1, y1 = rng.uniform(-5, W + 5, n), rng.uniform(-5, H + 5, n)
    x2, y2 = x1 + 9.0 + rng.normal(0, 0.5, n), y1 - 6.0 + rng.normal(0, 0.5, n)
    x1[:50] = W
    y1[50:80] = H
    y2[100:150] = H
    x2[150:170] = W
    y2[200:210], x2[210:220], y2[220:230] = 1e6, -1e6, -1e6
    x2[230:240], y2[230:240] = rng.uniform(-30, -0.5, 10), rng.uniform(0, 23, 10)  # r == -1 (row 0, column -1)
    t = np.arange(n)
    rnd = rng.random(n) < 0.4
    t[rnd] = rng.integers(0, n, int(rnd.sum()))
    return _case(_kps(x1, y1), _kps(x2, y2), np.arange(n), t)


def quirk_case():
    """One match, left (100, 100), right (-3, 5): the right index is -1 and the left cell has no valid vote, so the reference
    compares mCellPairs[l] == -1 with -1 and calls it an inlier."""
    return _case(_kps([100.0], [100.0]), _kps([-3.0], [5.0]), [0], [0])


def quirk_minus2_case():
    """The same comparison with -2: two matches vote cell 83 -> cell 50, too few for the threshold, so mCellPairs[83] = -2; a
    third match from cell 83 has the right index -2 (column -2 of row 0) and equals it: the only inlier."""
    return _case(_kps([100.0, 101.0, 102.0], [100.0, 101.0, 102.0]), _kps([330.0, 331.0, -40.0], [50.0, 51.0, 5.0]), [0, 1, 2], [0, 1, 2])


# ------------------------------------------------------------------------------------------------------------ 4(c) index lists
def _motion_scene(rng, n, size1=(W, H), size2=(W, H)):
    x1, y1 = rng.uniform(0, size1[0] - 0.01, n), rng.uniform(0, size1[1] - 0.01, n)
    sx, sy = size2[0] / size1[0], size2[1] / size1[1]
    x2 = np.clip((x1 + 7.0) * sx + rng.normal(0, 0.4, n), 0, size2[0] - 0.01)
    y2 = np.clip((y1 - 4.0) * sy + rng.normal(0, 0.4, n), 0, size2[1] - 0.01)
    return _kps(x1, y1), _kps(x2, y2)


def index_case(kind, seed=3):
    rng = np.random.default_rng(seed)
    n = 6000  # ~15 key-points a cell: enough for the neighbourhood score to pass where the motion is consistent
    size1, size2 = {"sizes_up": ((640, 480), (1280, 720)), "sizes_odd": ((577, 411), (640, 480))}.get(kind, ((W, H), (W, H)))
    kp1, kp2 = _motion_scene(rng, n, size1, size2)
    if kind == "subset":
        q = np.sort(rng.choice(n, 3500, replace=False))
    elif kind == "shuffle":
        q = rng.permutation(n)
    elif kind == "repeat":
        q = rng.integers(0, n, n)
    else:
        q = np.arange(n)
    t = q.copy()
    rnd = rng.random(len(q)) < 0.3
    t[rnd] = rng.integers(0, n, int(rnd.sum()))
    if kind == "one_train":
        t[::3] = 17  # a third of all matches land on one train point
    return _case(kp1, kp2, q, t, size1, size2)


INDEX_KINDS = ("subset", "shuffle", "repeat", "one_train", "sizes_up", "sizes_odd")


# -------------------------------------------------------------------------------------------------------------------- 4(d) counts
COUNTS = (1, 255, 256, 257, 8191, 8192)


def count_case(n, seed=4):
    """n matches (i, t[i]) over a square block of cells sized to hold ~16 of them a cell, 30 % of the train indices random"""
    rng = np.random.default_rng(seed + n)
    side = int(min(20, max(1, np.ceil(np.sqrt(n / 16)))))
    x1, y1 = rng.uniform(2 * CW, (2 + side) * CW - 0.01, n), rng.uniform(0, side * CH - 0.01, n)
    x1, y1 = np.minimum(x1, W - 0.01), np.minimum(y1, H - 0.01)
    x2, y2 = np.clip(x1 - 40.0 + rng.normal(0, 0.4, n), 0, W - 0.01), np.clip(y1 + 30.0 + rng.normal(0, 0.4, n), 0, H - 0.01)
    t = np.arange(n)
    rnd = rng.random(n) < 0.3
    t[rnd] = rng.integers(0, n, int(rnd.sum()))
    return _case(_kps(x1, y1), _kps(x2, y2), np.arange(n), t)


def one_cell_case(n=2048, seed=5):
    """All left points in one cell (for every shifted grid); 70 % of the right points in one cell, the rest anywhere"""
    rng = np.random.default_rng(seed)
    x1, y1 = _in_cell(6, 6, n, rng, 0.25, 0.19)
    x2, y2 = _in_cell(9, 4, n, rng, 0.05, 0.9)
    far = rng.random(n) < 0.3
    x2[far], y2[far] = rng.uniform(0, W - 0.01, int(far.sum())), rng.uniform(0, H - 0.01, int(far.sum()))
    return _case(_kps(x1, y1), _kps(x2, y2), np.arange(n), np.arange(n))


def empty_case():
    kp = _kps([10.0, 20.0], [10.0, 20.0])
    return _case(kp, kp.copy(), np.zeros(0, np.int32), np.zeros(0, np.int32))


def all_cases():
    """name -> case, every case of the GPU file (built once; nothing modifies them)"""
    c = {"tie": tie_case(False), "tie_swapped": tie_case(True), "borders": borders_case(), "quirk": quirk_case(), "quirk_minus2": quirk_minus2_case(),
         "one_cell": one_cell_case(), "empty": empty_case()}
    c.update({f"index_{k}": index_case(k) for k in INDEX_KINDS})
    c.update({f"count_{n}": count_case(n) for n in COUNTS})
    return c


HOST_BATCH = ("tie", "empty", "borders", "index_subset", "index_sizes_up", "count_257")
