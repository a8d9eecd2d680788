"""CPU test of the essential graph's structure lists (geoflowslam_amd/csrc/eg_lists.hpp through gfs_test_essential_graph_lists)
against a brute-force dictionary: duplicates, both orientations, an edge between two fixed vertices, a free vertex without an edge, a
fixed vertex in the middle.  No GPU."""
import numpy as np
import pytest

from pose_graph_support import STRUCTURE_CASES

CASES = dict(STRUCTURE_CASES, no_free_vertex=([1, 1], [(0, 1)]), no_edge=([0, 0, 1], []))


def brute_force(fixed, edges):
    free = {}
    for v, f in enumerate(fixed):
        if not f:
            free[v] = len(free)
    blocks = {(f, f): [] for f in free.values()}
    for e, (i, j) in enumerate(edges):
        fi, fj = free.get(i, -1), free.get(j, -1)
        if fi >= 0:
            blocks[(fi, fi)].append(4 * e + 0)
        if fj >= 0:
            blocks[(fj, fj)].append(4 * e + 1)
        if fi >= 0 and fj >= 0:
            blocks.setdefault((max(fi, fj), min(fi, fj)), []).append(4 * e + (2 if fi > fj else 3))
    return free, blocks


@pytest.mark.parametrize("name", sorted(CASES))
def test_lists_against_brute_force(api, name):
    fixed, edges = CASES[name]
    ei, ej = [e[0] for e in edges], [e[1] for e in edges]
    L = api.essential_graph_lists(fixed, ei, ej)
    free, blocks = brute_force(fixed, edges)
    assert L["n_free"] == len(free)
    assert list(L["free_index"]) == [free.get(v, -1) for v in range(len(fixed))]
    keys = sorted(blocks)
    assert [tuple(b) for b in L["blk_ij"]] == keys  # (bi, bj) order, bi >= bj, every diagonal block
    assert all(bi >= bj for bi, bj in keys)
    assert L["blk_begin"][0] == 0 and L["blk_begin"][-1] == len(L["contrib"])
    for b, key in enumerate(keys):
        assert list(L["contrib"][L["blk_begin"][b]:L["blk_begin"][b + 1]]) == blocks[key], key  # edge order inside the block
    # every term of every edge with a free end exactly once
    n_terms = sum((fixed[i] == 0) + (fixed[j] == 0) + (fixed[i] == 0 and fixed[j] == 0) for i, j in edges)
    assert len(L["contrib"]) == n_terms == len(set(L["contrib"].tolist()))


def test_random_graphs_against_brute_force(api):
    rng = np.random.default_rng(0)
    for _ in range(20):
        V = int(rng.integers(2, 40))
        fixed = (rng.random(V) < 0.2).astype(np.uint8)
        E = int(rng.integers(0, 120))
        ei = rng.integers(0, V, E)
        ej = (ei + rng.integers(1, V, E)) % V
        L = api.essential_graph_lists(fixed, ei, ej)
        free, blocks = brute_force(list(fixed), list(zip(ei.tolist(), ej.tolist())))
        keys = sorted(blocks)
        assert [tuple(b) for b in L["blk_ij"]] == keys
        for b, key in enumerate(keys):
            assert list(L["contrib"][L["blk_begin"][b]:L["blk_begin"][b + 1]]) == blocks[key]


def test_refusals(api):
    L = api.lib()
    fixed, ei, ej, counts = np.zeros(3, np.uint8), np.array([0, 3], np.int32), np.array([1, 1], np.int32), np.zeros(3, np.int64)
    args = lambda i, j: (3, 2, fixed.ctypes.data, i.ctypes.data, j.ctypes.data, counts.ctypes.data, None, None, None, 0, None, 0)
    assert L.gfs_test_essential_graph_lists(*args(ei, ej)) == -1  # a vertex outside the graph
    ei[1] = 1
    assert L.gfs_test_essential_graph_lists(*args(ei, ej)) == -1  # an edge from a vertex to itself
