"""CPU checks behind test_gpu_frame_batched.py and test_gpu_gms_cases.py: every case those files feed the device goes through
the numpy restatement (frame_helpers_support.py, gms_support.py) and through the C++ oracle, which must agree bit for bit; and
every case must still exercise the edge it was built for, so a builder that drifts fails here and not silently on the device."""
import numpy as np
import pytest

import frame_helpers_support as fs
import gms_support as gs

f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------ cloud
@pytest.mark.parametrize("name", list(fs.CLOUD_SHAPES))
def test_cloud_restatement_matches_oracle(oracle, name):
    cols, rows, ds = fs.CLOUD_SHAPES[name]
    for B in fs.CLOUD_BATCHES:
        depth, ds, K, kinds = fs.cloud_batch(name, B)
        assert depth.shape == (B, rows, cols) and depth.dtype == f32
        total = -(-rows // ds) * -(-cols // ds)
        counts = []
        for b in range(B):
            ref, orc = fs.cloud_ref(depth[b], ds, *K), oracle.depth_to_cloud(depth[b], ds, *K)
            assert ref.shape == orc.shape and np.array_equal(fs.bits(ref), fs.bits(orc))
            counts.append(len(ref))
            if kinds[b] == "none":
                assert len(ref) == 0
            if kinds[b] == "all":
                assert len(ref) == total
            if kinds[b] == "last_round":  # every valid sample at a raster position of the last 1024-sample round
                g = depth[b][::ds, ::ds].reshape(-1)
                first = np.nonzero((g > 0) & (g < 10))[0]
                assert len(first) > 0 and first[0] >= ((total - 1) // 1024) * 1024
        if B >= 5:
            assert {"none", "all", "last_round"} <= set(kinds) and len(set(counts)) >= min(3, total + 1)  # ragged counts
    assert {n: -(-fs.CLOUD_SHAPES[n][1] // fs.CLOUD_SHAPES[n][2]) * -(-fs.CLOUD_SHAPES[n][0] // fs.CLOUD_SHAPES[n][2])
            for n in ("32x32", "33x31", "41x25", "7x5s9", "320x240s2")} == {"32x32": 1024, "33x31": 1023, "41x25": 1025, "7x5s9": 1,
                                                                          "320x240s2": 19200}


@pytest.mark.parametrize("which", ["dense", "strided"])
def test_special_depths(oracle, which):
    """3(c): the special values reach the samples; the outputs hold subnormals (which only a kernel that keeps fp32 subnormals
    reproduces), the largest depth below 10 is kept and nothing at or above 10 is."""
    d, ds, K = fs.special_depth_case(which)
    on = d[::ds, ::ds]
    for s in fs.SPECIALS:
        assert (fs.bits(on) == fs.bits(f32(s))).any(), f"special depth {s!r} is on no sample"
    ref, orc = fs.cloud_ref(d, ds, *K), oracle.depth_to_cloud(d, ds, *K)
    assert ref.shape == orc.shape and np.array_equal(fs.bits(ref), fs.bits(orc))
    n_sub = int((fs.is_subnormal(ref[:, 0]) | fs.is_subnormal(ref[:, 1])).sum())
    assert n_sub >= 8, n_sub
    assert (ref[:, 2] == fs.BELOW10).any() and not (ref[:, 2] >= 10).any() and (ref[:, 2] > 0).all()
    assert fs.is_subnormal(ref[:, 2]).any() and (ref[:, 3] == 1).all()
    if ds > 1:  # off the grid the specials change nothing
        plain = d.copy()
        plain[~fs.grid_mask(*d.shape, ds)] = 1.0
        assert (~np.isfinite(d[~fs.grid_mask(*d.shape, ds)])).any()
        assert np.array_equal(fs.bits(fs.cloud_ref(plain, ds, *K)), fs.bits(ref))


# ----------------------------------------------------------------------------------------------------------------------- stereo
@pytest.mark.parametrize("B", fs.STEREO_BATCHES)
@pytest.mark.parametrize("kp_stride", fs.STEREO_STRIDES)
def test_stereo_restatement_matches_oracle(oracle, B, kp_stride):
    c = fs.stereo_case(B, kp_stride)
    rows, cols = c["rows"], c["cols"]
    x, y = c["kps"]["x"], c["kps"]["y"]
    assert (x > -1).all() and (x < cols).all() and (y > -1).all() and (y < rows).all()  # outside is undefined in the reference too
    assert (x.astype(np.int32) >= 0).all() and (y.astype(np.int32) >= 0).all()
    assert (c["unx"] != x).all()
    cnt = c["counts"]
    assert len(cnt) == B and (cnt >= 0).all() and (cnt <= kp_stride).all()
    if B > 1:
        assert 0 in cnt and kp_stride in cnt
    seen_ur, seen_d = [], []
    for with_unx in (True, False):
        for b in range(B):
            n = int(cnt[b])
            k, u = c["kps"][b, :n], (c["unx"][b, :n] if with_unx else None)
            ur, vd = fs.stereo_ref(k, u, c["depth"][b], c["bf"])
            uo, vo = oracle.stereo_from_rgbd(k, c["depth"][b], float(c["bf"]), u)
            assert np.array_equal(fs.bits(ur), fs.bits(uo)) and np.array_equal(fs.bits(vd), fs.bits(vo))
            seen_ur.append(ur)
            seen_d.append(c["depth"][b][k["y"].astype(np.int32), k["x"].astype(np.int32)])
    if kp_stride >= 255:
        ur, d = np.concatenate(seen_ur), np.concatenate(seen_d)
        neg = ((x > -1) & (x < 0)) | ((y > -1) & (y < 0))
        assert neg.sum() >= 8 and (np.floor(x[neg]) != x[neg].astype(np.int32)).any() and (np.floor(y[neg]) != y[neg].astype(np.int32)).any()
        assert (np.floor(x[(x > -1) & (x < 0)]) == -1).all()  # floor differs from the truncation wherever a coordinate is negative
        assert (d < 0).any() and (fs.bits(d) == fs.bits(f32(-0.0))).any() and np.isnan(d).any() and np.isposinf(d).any()
        assert fs.is_subnormal(d).any() and np.isneginf(ur).any()  # bf / subnormal overflows: mvuRight = -inf
        assert (ur == -1).any() and np.isfinite(ur).any()
        assert (x >= cols - 0.02).any() and (y >= rows - 0.02).any()


# -------------------------------------------------------------------------------------------------------------------------- u16
def test_u16_cases():
    sizes = [int(np.prod(s)) for s in fs.U16_SHAPES]
    assert sizes == [1, 3, 15, 63, 105, 1025, 2050, 4099] and all(n % 4 for n in sizes)
    for s in fs.U16_SHAPES:
        raw = fs.u16_case(s)
        assert raw.dtype == np.uint16 and raw.shape == s and 65535 in raw and (raw.size == 1 or 0 in raw)
        for factor in fs.U16_FACTORS:
            want = fs.u16_ref(raw, factor)
            assert want.dtype == f32
            # one rounding: the float32 product of two float32 values equals the rounded double product
            assert np.array_equal(fs.bits(want), fs.bits((raw.astype(np.float64) * float(f32(factor))).astype(f32)))


# -------------------------------------------------------------------------------------------------------------------------- GMS
@pytest.fixture(scope="module")
def gms_cases():
    return gs.all_cases()


@pytest.fixture(scope="module")
def gms_refs(gms_cases):
    return {k: gs.gms_ref(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"]) for k, c in gms_cases.items()}


def test_gms_restatement_matches_oracle(oracle, gms_cases, gms_refs):
    for name, c in gms_cases.items():
        m, n = gms_refs[name]
        mo, no = oracle.gms_inlier_mask(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"])
        assert n == no and np.array_equal(m, mo), name
        assert len(m) == len(c["q"])
        assert len(c["q"]) == 0 or (c["q"].min() >= 0 and c["q"].max() < len(c["kp1"]) and c["t"].min() >= 0 and c["t"].max() < len(c["kp2"]))
    assert all(k in gms_cases for k in gs.HOST_BATCH)


@pytest.mark.parametrize("swap", [False, True])
def test_gms_tie_block(gms_cases, gms_refs, swap):
    """4(a): in every grid every left cell of the block splits its 222 votes 111 : 111 between two right cells; the lower right
    index wins, whichever parity it was given."""
    name = "tie_swapped" if swap else "tie"
    c = gms_cases[name]
    m, n = gms_refs[name]
    assert len(m) == 9 * gs.TIE_PER_CELL
    for gtype in (1, 2, 3, 4):
        l, r = gs.grid_indices(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"], gtype)
        for j, (cx, cy) in enumerate(gs.TIE_BLOCK):
            sl = slice(j * gs.TIE_PER_CELL, (j + 1) * gs.TIE_PER_CELL)
            assert (l[sl] == cx + 20 * cy).all()  # no shifted grid splits a cell
            targets, votes = np.unique(r[sl], return_counts=True)
            assert len(targets) == 2 and votes.tolist() == [111, 111]
            lo_off = gs.TIE_OFFSETS[1]
            assert targets[0] == cx + lo_off[0] + 20 * (cy + lo_off[1])
            assert (r[sl][(0 if swap else 1)::2] == targets[0]).all()  # the parity that holds the lower index
    odd, even = int(m[1::2].sum()), int(m[0::2].sum())
    assert (odd, even) == ((0, 999) if swap else (999, 0)) and n == 999


def test_gms_border_and_list_conditions(gms_cases, gms_refs):
    c = gms_cases["borders"]
    m, n = gms_refs["borders"]
    assert len(m) == 3000 and 300 < n < 2700
    l1, r = gs.grid_indices(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"], 1)
    l4, _ = gs.grid_indices(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"], 4)
    x1, y1 = c["kp1"]["x"], c["kp1"]["y"]
    assert (x1 == gs.W).sum() >= 50 and (c["kp2"]["y"] == gs.H).sum() >= 50 and x1.min() < -4 and x1.max() > gs.W + 4
    assert (l1[:50] == -1).all() and (l1 < -1).any()  # x == width; negative coordinates in row 0
    assert ((x1 < 0) & (y1 >= gs.CH) & (y1 < gs.H) & (l1 >= 0)).any()  # negative x wraps into the previous row
    assert ((l1 >= 0) & (l4 == -1)).any()  # the shifted grids round the last half cell up to column / row 20
    assert (r >= 400).any() and (r > 32767).any() and (r < -32768).any() and (r == -1).any() and ((r < -1) & (r > -400)).any()
    assert not m[(r >= 400) | (r < -2)].any()
    # the quirk on its own
    cq = gms_cases["quirk"]
    lq, rq = gs.grid_indices(cq["kp1"], cq["size1"], cq["kp2"], cq["size2"], cq["q"], cq["t"], 1)
    assert lq.tolist() == [83] and rq.tolist() == [-1] and gms_refs["quirk"][0].tolist() == [True]
    cq = gms_cases["quirk_minus2"]
    lq, rq = gs.grid_indices(cq["kp1"], cq["size1"], cq["kp2"], cq["size2"], cq["q"], cq["t"], 1)
    assert lq.tolist() == [83, 83, 83] and rq.tolist() == [50, 50, -2] and gms_refs["quirk_minus2"][0].tolist() == [False, False, True]
    # index lists
    n1 = len(gms_cases["index_subset"]["kp1"])
    q = gms_cases["index_subset"]["q"]
    assert len(q) < n1 and len(np.unique(q)) == len(q) and not np.array_equal(q, np.arange(len(q)))
    q = gms_cases["index_shuffle"]["q"]
    assert np.array_equal(np.sort(q), np.arange(n1)) and not np.array_equal(q, np.arange(n1))
    q = gms_cases["index_repeat"]["q"]
    assert len(np.unique(q)) < len(q)
    assert (gms_cases["index_one_train"]["t"] == 17).sum() >= len(q) // 3
    assert (gms_cases["index_sizes_up"]["size1"], gms_cases["index_sizes_up"]["size2"]) == ((640, 480), (1280, 720))
    assert (gms_cases["index_sizes_odd"]["size1"], gms_cases["index_sizes_odd"]["size2"]) == ((577, 411), (640, 480))
    for k in gs.INDEX_KINDS:  # each list leaves a real filter: inliers and outliers both
        m, n = gms_refs["index_" + k]
        assert 0.2 * len(m) < n < 0.9 * len(m), (k, n, len(m))
    # counts
    assert [len(gms_cases[f"count_{k}"]["q"]) for k in gs.COUNTS] == [1, 255, 256, 257, 8191, 8192]
    for k in gs.COUNTS[1:]:
        m, n = gms_refs[f"count_{k}"]
        assert 0.2 * k < n < 0.9 * k, (k, n)
    c = gms_cases["one_cell"]
    for gtype in (1, 2, 3, 4):
        l, _ = gs.grid_indices(c["kp1"], c["size1"], c["kp2"], c["size2"], c["q"], c["t"], gtype)
        assert len(l) == 2048 and (l == 6 + 20 * 6).all()
    m, n = gms_refs["one_cell"]
    assert 0.5 * 2048 < n < 0.8 * 2048
    assert all(gs.is_arange(gms_cases[k]) for k in ("tie", "tie_swapped", "borders", "quirk", "quirk_minus2", "one_cell", "count_257", "count_8192"))
