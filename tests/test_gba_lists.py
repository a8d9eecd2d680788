"""CPU tests of what GlobalBundleAdjustment builds on the host (no GPU): the structure lists of the Schur assembly
(csrc/gba_lists.hpp through gfs_test_gba_lists) against a brute-force statement, and the tile arithmetic of the tiled reduced
system (csrc/gba_tiles.hpp through gfs_test_gba_tile_layout) against Python integers."""
import numpy as np
import pytest

import gba_support as G


def _Fp(api):
    P = api.gba_panel_rows()
    assert P % 6 == 0 and P % 16 == 0 and P >= 48
    return P // 6


@pytest.mark.parametrize("index", range(9))
def test_structure_lists_against_brute_force(api, index):
    name, make = G.list_cases(_Fp(api))[index]
    w = make()
    L = api.gba_lists(w)
    ref = G.brute_force_lists(w)
    assert L["n_free"] == ref["F"], name
    assert np.array_equal(L["order"], ref["order"]), name
    # the set of listed blocks, in (i, j) order: every diagonal block and every pair with a common landmark
    want = sorted(ref["blocks"])
    assert [tuple(b) for b in L["blk_ij"].tolist()] == want, name
    assert L["blk_begin"][0] == 0 and L["blk_begin"][-1] == len(L["contrib"]) and (np.diff(L["blk_begin"]) >= 0).all(), name
    assert L["blk_begin"].dtype == np.int64 and L["pose_begin"].dtype == np.int64
    # every list's contents AND order: by landmark, then e1, then e2 (the brute force visits them so)
    for b, key in enumerate(want):
        got = [tuple(c) for c in L["contrib"][L["blk_begin"][b]:L["blk_begin"][b + 1]].tolist()]
        assert got == ref["blocks"][key], (name, key)
    for f in range(ref["F"]):
        assert L["pose_edges"][L["pose_begin"][f]:L["pose_begin"][f + 1]].tolist() == ref["pose"][f], (name, f)
    n_terms = sum(len(v) for v in ref["blocks"].values())
    print(f"{name}: F={ref['F']} blocks={len(want)} of {ref['F'] * (ref['F'] + 1) // 2} terms={n_terms}")
    if name == "duplicate-edges":  # both orders of two edges of one pose on one landmark, and each with itself
        diag = [c for k, v in ref["blocks"].items() if k[0] == k[1] for c in v]
        assert any(e1 != e2 for e1, e2 in diag) and all((e2, e1) in diag for e1, e2 in diag if e1 != e2)
    if name == "isolated-pose":
        lone = [i for i in range(ref["F"]) if all(k == (i, i) or i not in k for k in ref["blocks"])]
        assert lone, "no pose without a neighbour in this map"
    if name in ("all-fixed", "zero-points"):
        assert len(L["contrib"]) == 0 and len(L["blk_ij"]) == ref["F"]
    if name.startswith("F") and ref["F"] > 3:
        assert len(want) < ref["F"] * (ref["F"] + 1) // 2, "the map is fully covisible: it does not exercise sparsity"


def test_tile_and_offset_arithmetic(api):
    P = api.gba_panel_rows()
    for n in (0, 1, 6, P - 6, P, P + 6, 2 * P, 2 * P + 6, 6 * 485, 6 * 4000):
        T = -(-n // P)
        rng = np.random.default_rng(n)
        rows = {0, n - 1, P - 1, P, (T - 1) * P, n // 2} if n else set()
        cells = {(r, c) for r in rows if 0 <= r < n for c in (0, r, r // 2, (r // P) * P, max(r - 1, 0))}
        cells |= {(int(r), int(rng.integers(0, r + 1))) for r in rng.integers(0, max(n, 1), 20) if n}
        got0 = api.gba_tile_layout(n, 0, 0)
        assert got0["panels"] == T and got0["storage_bytes"] == T * (T + 1) // 2 * P * P * 8, n
        for r, c in cells:
            got = api.gba_tile_layout(n, r, c)
            ti, tj = r // P, c // P
            tile = ti * (ti + 1) // 2 + tj
            assert got["tile_index"] == tile and got["byte_offset"] == (tile * P * P + (r % P) * P + c % P) * 8, (n, r, c, got)
            assert got["byte_offset"] < got0["storage_bytes"]
    n = 6 * 4000  # where a 32-bit int of bytes overflows
    last = api.gba_tile_layout(n, n - 1, n - 1)
    assert last["byte_offset"] > 2 ** 31 and last["storage_bytes"] > 2 ** 31
    # distinct cells of the lower triangle never share storage
    n = 2 * P + 6
    seen = {api.gba_tile_layout(n, r, c)["byte_offset"] for r in range(0, n, 5) for c in range(0, r + 1, 7)}
    assert len(seen) == sum(len(range(0, r + 1, 7)) for r in range(0, n, 5))
