"""CPU half of the ORB edge-geometry tests: on the oracle and the host hook gfs_test_orb_geometry alone (no GPU) it asserts, for every
row of tests/orb_geometry_support.py, the property the row is there for -- cell grids, nIni, quotas, which levels k_octree accepts, the
kp_cap numbers of the capacity rule -- and that the oracle has key points on every level of every row, so that the GPU comparison of
tests/test_gpu_orb_geometry.py has something to compare on each of them.  Each assertion names its row."""
import numpy as np
import pytest

import orb_geometry_support as S


@pytest.fixture(scope="module")
def geometry(api):
    return {c["key"]: api.orb_geometry(c["h"], c["w"], c["nf"], c["nl"], S.SCALE) for c in S.CASES}


@pytest.mark.parametrize("key", [c["key"] for c in S.CASES])
def test_row_has_the_geometry_it_is_there_for(api, geometry, key):
    c, g = S.CASE[key], geometry[key]
    lv = g["levels"]
    assert g["supported"] and len(lv) == c["nl"], key
    for l, L in enumerate(lv):  # what the hook reports is consistent with the reference's grid (src/ORBextractor.cc:778-786)
        assert L["n_cell_cols"] == (L["cols"] - 32) // 35 and L["n_cell_rows"] == (L["rows"] - 32) // 35, (key, l)
        assert L["w_cell"] == -(-(L["cols"] - 32) // L["n_cell_cols"]) and L["h_cell"] == -(-(L["rows"] - 32) // L["n_cell_rows"]), (key, l)
        assert L["n_ini"] == max(1, S.n_ini_raw(L["cols"] - 32, L["rows"] - 32)), (key, l)
        assert L["kp_cap"] == L["quota"] + 3 + 4 * L["n_ini"], (key, l)
        assert bool(L["octree_on_device"]) == (L["n_ini"] <= 4 and L["quota"] + 4 * L["n_ini"] + 8 <= S.OCT_MAX_NODES), (key, l)
    assert g["kp_cap"] == sum(L["kp_cap"] for L in lv), key
    assert bool(g["octree_on_device"]) == all(L["octree_on_device"] for L in lv) == (c["octree"] == "device"), f"row {key}: quadtree path"
    assert sum(L["quota"] for L in lv) == max(c["nf"], sum(L["quota"] for L in lv[:-1])), f"row {key}: quotas add up to the feature count"
    assert (g["pyr_strips"] == 0) == (c["nl"] == 1), f"row {key}: a pyramid kernel exactly when there is a level above 0"
    for l in c.get("one_cell_levels", ()):
        assert (lv[l]["n_cell_cols"], lv[l]["n_cell_rows"], lv[l]["n_cells"]) == (1, 1, 1), f"row {key}: level {l} is one cell"
    if "one_cell_levels" in c and c["nl"] > 2:
        assert all(lv[l]["n_cells"] > 1 for l in range(c["nl"]) if l not in c["one_cell_levels"]), f"row {key}: the other levels have more cells"
    if "top_level" in c:
        T = lv[-1]
        assert (T["cols"], T["rows"], T["max_cell_w"], T["max_cell_h"]) == c["top_level"], f"row {key}: top level"
        assert not api.orb_geometry(c["h"] - 4, c["w"] - 4, c["nf"], c["nl"], S.SCALE)["supported"], f"row {key}: 66 x 66 on top is refused"
    if "blur_tile_cols" in c:
        assert -(-c["w"] // 64) == c["blur_tile_cols"] and c["w"] - 64 == c["last_tile_w"], f"row {key}: blur tile columns"
        assert g["n_blur_tiles"] == c["blur_tile_cols"] * -(-c["h"] // 32), f"row {key}: blur tiles"
    if "widest_cell" in c:
        assert (lv[0]["max_cell_w"], lv[0]["max_cell_h"]) == c["widest_cell"], f"row {key}: the cell"
        assert all(lv[0]["max_cell_w"] >= L["max_cell_w"] for k in S.CASES for L in geometry[k["key"]]["levels"]), f"row {key}: widest cell"
        assert g["fast_lds_wave"] == max(geometry[k["key"]]["fast_lds_wave"] for k in S.CASES if k["group"] != "a"), \
            f"row {key}: largest fast_lds_wave next to the one-cell levels of group a"
    if "n_ini" in c:
        assert tuple(L["n_ini"] for L in lv) == c["n_ini"], f"row {key}: nIni"
    if c.get("raw_aspect_rounds_to_zero"):
        assert all(S.n_ini_raw(L["cols"] - 32, L["rows"] - 32) == 0 for L in lv), f"row {key}: round(width / height) is 0 before it is set to 1"
    if "quotas" in c:
        assert tuple(L["quota"] for L in lv) == c["quotas"], f"row {key}: quotas"
    if "quota0" in c:
        assert lv[0]["quota"] == c["quota0"], f"row {key}: level-0 quota"
    if "device_levels" in c:
        assert tuple(bool(L["octree_on_device"]) for L in lv) == c["device_levels"], f"row {key}: levels k_octree accepts"
    if "xtab_in_lds" in c:
        assert g["xtab_in_lds"] == c["xtab_in_lds"] and g["pyr_in_lds"] == 1, f"row {key}: x tables"


def test_d3400_is_the_last_count_on_the_device(api):
    """Row d3400: 738 + 4 + 8 = 750 <= 768 stays on the device; the feature count whose level-0 quota first passes 768 - 12 does not."""
    nf = 3400
    while api.orb_geometry(480, 640, nf, 8, S.SCALE)["octree_on_device"]:
        nf += 1
    q = api.orb_geometry(480, 640, nf, 8, S.SCALE)["levels"][0]["quota"]
    assert q == S.OCT_MAX_NODES - 12 + 1 and api.orb_geometry(480, 640, nf - 1, 8, S.SCALE)["levels"][0]["quota"] == S.OCT_MAX_NODES - 12


def test_capacity_rule_numbers(api):
    """Capacity rule (rows l and k of the GPU file): a handle holds kp_cap of its max size + 8; 1000 features on 8 levels need 1056 at
    640 x 480, 1068 at 320 x 240 (levels 5..7 are 129 x 96, 107 x 80, 89 x 67, nIni 2 each) and 1100 at 640 x 300."""
    for (w, h), cap in S.KP_CAP.items():
        assert api.orb_geometry(h, w, 1000, 8, S.SCALE)["kp_cap"] == cap, (w, h)
    lv = api.orb_geometry(240, 320, 1000, 8, S.SCALE)["levels"]
    assert [(L["cols"], L["rows"], L["n_ini"]) for L in lv[5:]] == [(129, 96, 2), (107, 80, 2), (89, 67, 2)]
    assert S.KP_CAP[(320, 240)] > S.KP_CAP[(640, 480)] + 8 and S.KP_CAP[(640, 300)] > S.KP_CAP[(640, 480)] + 8
    # row k: a 640 x 640 handle holds 1056 + 8 as well -- below what 320 x 240 needs; and 640 x 150 has a level smaller than a cell
    assert api.orb_geometry(640, 640, 1000, 8, S.SCALE)["kp_cap"] == 1056
    for w, h in ((640, 480), (241, 241), (480, 640), (577, 433)):
        assert api.orb_geometry(h, w, 1000, 8, S.SCALE)["kp_cap"] <= 1056 + 8, (w, h)
    assert not api.orb_geometry(150, 640, 1000, 8, S.SCALE)["supported"]


def test_hook_refuses_what_create_refuses(api):
    import ctypes as C
    I = api.OrbGeometryInfo()
    for rows, cols, nf, nl, sf in ((0, 640, 1000, 8, 1.2), (480, 640, 0, 8, 1.2), (480, 640, 1000, 0, 1.2), (480, 640, 1000, 17, 1.2),
                                   (480, 640, 1000, 8, 1.0)):
        assert api.lib().gfs_test_orb_geometry(rows, cols, nf, nl, sf, C.byref(I), None, 0) == -1
    assert api.lib().gfs_test_orb_geometry(480, 640, 1000, 8, 2.0, C.byref(I), None, 0) == S.ERR_UNSUPPORTED  # integer level ratio


@pytest.mark.parametrize("key", [c["key"] for c in S.CASES])
def test_oracle_has_key_points_on_every_level(oracle, geometry, key):
    c = S.CASE[key]
    orc = S.make_oracle(oracle, c)
    assert tuple(orc.tables()["feats"]) == tuple(L["quota"] for L in geometry[key]["levels"]), f"row {key}: the oracle's quotas"
    for rendered in (False, True) if c["rendered"] else (False,):
        m, k, d = orc.extract(S.image(c, rendered=rendered))
        counts = S.level_counts(orc, c["nl"])
        assert all(n >= 1 for n in counts) and sum(counts) == len(k) == len(d), f"row {key}: key points per level {counts}"
        assert all(orc.level_size(l) == (L["rows"], L["cols"]) for l, L in enumerate(geometry[key]["levels"])), f"row {key}: level sizes"
        if "kept_per_level" in c and not rendered:
            assert counts == [c["kept_per_level"]] * c["nl"], f"row {key}: the first sweep leaves 4 nodes whatever the quota"
        if not rendered:
            assert all(n <= L["kp_cap"] for n, L in zip(counts, geometry[key]["levels"])), f"row {key}: within the level's kp_cap"
    # the frames of the batches of group b (frames 0..8) have key points as well
    if c["group"] == "b" and c["w"] < 100:
        for i in range(1, 9):
            assert len(orc.extract(S.image(c, i))[1]) >= 1, f"row {key}: frame {i}"


def test_lapping_probes_sit_on_the_inclusive_bounds(oracle):
    """Case h: every computed lap has a key point exactly on an inclusive bound -- one integer off, at least one key point changes block."""
    L = S.LAP
    orc = oracle.OrbOracle(L["nf"], S.SCALE, L["nl"], S.INI_TH, S.MIN_TH)
    for rendered in (False, True):
        img = S.image(L, rendered=rendered)
        probes, exact = S.lap_probes(orc, img, L["nl"])
        n = len(orc.extract(img)[1])
        names = [p[0] for p in probes]
        assert len(probes) == 5, names
        m, k, _ = orc.extract(img, probes[0][1])
        assert m == 0 and len(k) == n, "case h: lap (-10, 1000) makes every key point stereo"
        if not rendered:
            assert n == 506 and exact, "case h: the noise image gives 506 key points, one of them with an integer x * scale"
        assert orc.extract(img, probes[1][1])[0] == n, "case h: an empty interval leaves every key point mono"
        for name, lap, others in probes[2:]:
            m = orc.extract(img, lap)[0]
            assert 0 < m < n or (m == 0 and n > 0), name
            for o in others:
                assert orc.extract(img, o)[0] > m, f"case h, {name}: lap {lap} against {o}"
