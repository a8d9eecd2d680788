"""The fast path of the voxel sort's leaf kernel (csrc/voxel_qsort.hpp k_voxel_qsort_leaf<unsigned>): a leaf range is radix-sorted
first, and only a range whose equal keys could change a voxel mean replays libstdc++'s introsort.  The hook
gfs_test_voxel_sort_paths tells on which path the ranges of the last sort ended, so every test also shows that it ran the code it is
about.  The permutation is compared with the oracle's quick_sort_omp, the voxel means bit for bit with the oracle's downsampling."""
import os
import subprocess
import sys

import numpy as np
import pytest

from geoflowslam_amd import synth
from test_voxel_tie_rule import LEAF, range_is_harmless, voxel_keys

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 19456
INVALID = np.uint64(0xFFFFFFFFFFFFFFFF)
SIZES = (2, 3, 16, 17, 63, 64, 65, 500, 1023, 1024, 1025, 2047, 5000, 19200)


def _pack(x, y, z):
    return (np.asarray(x).astype(np.uint64) | (np.asarray(y).astype(np.uint64) << np.uint64(21)) |
            (np.asarray(z).astype(np.uint64) << np.uint64(42)))


def _distinct_keys(rng, n, where):
    """n distinct voxel keys whose compacted form (x | y << bx | z << (bx + by), fields relative to the cloud's minimum) spans 31
    bits.  Element 0 alone carries the bits that set the widths of the other fields, so in every leaf range that does not hold it
    -- all but one of the ranges of the clouds of 1 024 points and more -- the keys differ only at the bottom (x), only at the top
    (z) or at both ends of the span: those ranges exercise the digit skipping.  A cloud below 1 024 points is one range that holds
    element 0: all 31 bits vary there, which is the four-pass case."""
    if where == "bottom":    # x: 16 bits, all the variation; y and z: one element sets their 7 + 8 bits
        x = rng.choice(1 << 16, n, replace=False)
        y, z = np.zeros(n, np.int64), np.zeros(n, np.int64)
        y[0], z[0] = 127, 255
    elif where == "top":     # z: 15 bits, all the variation; one element sets the 8 + 8 bits of x and y
        z = rng.choice(1 << 15, n, replace=False)
        x, y = np.zeros(n, np.int64), np.zeros(n, np.int64)
        x[0], y[0] = 255, 255
    else:                    # both ends: z (15 bits) and x (8 bits) vary, y (8 bits, set by one element) does not
        u = rng.choice(1 << 23, n, replace=False)
        x, z = u & 255, u >> 8
        y = np.zeros(n, np.int64)
        y[0] = 255
    return _pack(x + 1000, y + 2000, z + 3000)


def _arrange(rng, k, how):
    if how == "random":
        return k[rng.permutation(len(k))]
    s = np.sort(k)
    if how == "ascending":
        return s
    if how == "descending":
        return s[::-1].copy()
    teeth = 7  # sawtooth: seven ascending runs interleaved over the key range
    return np.concatenate([s[t::teeth] for t in range(teeth)])


def test_tie_free_ranges_are_the_references_permutation(gpu_api, oracle):
    rng = np.random.default_rng(31)
    reg = gpu_api.RegistrationGICP(max_points=CAP)
    for n in SIZES:
        for where in ("bottom", "top", "both"):
            for how in ("random", "ascending", "descending", "sawtooth"):
                k = _arrange(rng, _distinct_keys(rng, n, where), how)
                got = reg.voxel_sort_perm(k)
                paths = reg.voxel_sort_paths()
                want, _ = oracle.quick_sort_perm(k)
                assert np.array_equal(got, want), (n, where, how, int((got != want).sum()))
                assert paths["tie_free"] > 0 and paths["replica"] == 0 and paths["harmless"] == 0, (n, where, how, paths)
    for n in SIZES:  # the invalid key (all ones) once in a cloud: it is the largest key of the last range
        k = _arrange(rng, _distinct_keys(rng, n, "both"), "random")
        k[int(rng.integers(0, n))] = INVALID
        got = reg.voxel_sort_perm(k)
        paths = reg.voxel_sort_paths()
        want, _ = oracle.quick_sort_perm(k)
        assert np.array_equal(got, want), (n, "invalid", int((got != want).sum()))
        assert paths["tie_free"] > 0 and paths["replica"] == 0, (n, "invalid", paths)


def test_mixed_cloud_without_points_replays_only_the_tied_ranges(gpu_api, oracle):
    """19 200 keys, the low third with about 10 % of its keys doubled, the rest distinct; the hook sort has no point data, so every
    range with equal keys must come out in the reference's own order."""
    rng = np.random.default_rng(32)
    n = 19200
    v = rng.choice(1 << 22, n, replace=False)
    v.sort()
    low = n // 3
    dup = rng.choice(low - 1, low // 10, replace=False)
    v[dup + 1] = v[dup]
    v = v[rng.permutation(n)]
    k = _pack((v & 255) + 1000, ((v >> 8) & 127) + 2000, (v >> 15) + 3000)
    reg = gpu_api.RegistrationGICP(max_points=CAP)
    got = reg.voxel_sort_perm(k)
    paths = reg.voxel_sort_paths()
    want, _ = oracle.quick_sort_perm(k)
    assert np.array_equal(got, want), int((got != want).sum())
    assert paths["tie_free"] > 0 and paths["replica"] > 0 and paths["harmless"] == 0, paths


def _assert_means_are_the_oracles(reg, oracle, clouds):
    for which, cloud in enumerate(clouds):
        pts, _ = reg.preprocessed(0, which)
        po, _, _ = oracle.gicp_preprocess(cloud)
        assert len(pts) == len(po)
        ig = np.lexsort((pts[:, 2], pts[:, 1], pts[:, 0]))
        io = np.lexsort((po[:, 2], po[:, 1], po[:, 0]))
        assert (pts[ig].view(np.uint64) == po[io].view(np.uint64)).all(), ("voxel means differ", which)


@pytest.mark.parametrize("seed", [1000, 1300])
def test_voxel_means_of_bench_scenes_are_the_same_bits(gpu_api, oracle, seed):
    """Both clouds of two scenes of the benchmark: most ranges have harmless ties, and each scene has a voxel across a block cut."""
    fp = synth.frame_pair(seed, 640, 480, 4)
    reg = gpu_api.RegistrationGICP(max_points=CAP)
    reg.RegisterPointClouds(fp["cloud0"], fp["cloud1"])
    paths = reg.voxel_sort_paths()
    print("leaf paths, seed", seed, paths)
    _assert_means_are_the_oracles(reg, oracle, (fp["cloud0"], fp["cloud1"]))
    assert paths["harmless"] > 0 and paths["replica"] > 0, paths


def crafted_cloud(case):
    """2 100 points on a gently curved sheet, one point a voxel (50 voxels a row: the sorted order is row by row) except for one
    voxel at sorted position `first` that holds g points.  -> (cloud, first, g)"""
    first, g = {"a": (1022, 4), "b": (1020, 4), "c": (0, 2), "d": (500, 70), "plain": (0, 1)}[case]
    rng = np.random.default_rng(ord(case[0]))
    n = 2100
    nv = n - g + 1
    sizes = np.ones(nv, np.int64)
    sizes[first] = g
    v = np.repeat(np.arange(nv), sizes)
    ix, iy = v % 50, v // 50
    pts = np.ones((n, 4), np.float32)
    u = rng.uniform(0.1, 0.9, (n, 2))
    pts[:, 0] = ((ix + u[:, 0]) * LEAF).astype(np.float32)
    pts[:, 1] = ((iy + u[:, 1]) * LEAF).astype(np.float32)
    pts[:, 2] = (1.0 + 0.004 * np.sin(0.2 * ix) * np.cos(0.15 * iy) + 0.005).astype(np.float32)  # inside the voxel layer [1.0, 1.02)
    if case == "c":  # the tied voxel is (0, 0): 1e-9 beside 0.019
        pts[0, 0], pts[1, 0] = 1e-9, 0.019
    pts = pts[rng.permutation(n)]
    return pts, first, g


CRAFTED = {"a": "replica", "b": "harmless", "c": "replica", "d": "replica"}


def _numpy_says_harmless(oracle, cloud):
    keys = voxel_keys(cloud)
    perm, skeys = oracle.quick_sort_perm(keys)
    return range_is_harmless(skeys, 0, cloud[perm])  # one tied voxel: the range around it decides like the whole array does


@pytest.mark.parametrize("case", sorted(CRAFTED))
def test_crafted_voxels_take_the_stated_path(gpu_api, oracle, case):
    """(a) a voxel of 4 points across sorted position 1024: replica; (b) the same voxel ending at 1023: harmless; (c) 1e-9 beside
    0.019 in a tied voxel: the exponent window asks for the replica; (d) 70 points in a voxel: more than 64, replica."""
    cloud, first, g = crafted_cloud(case)
    plain, _, _ = crafted_cloud("plain")
    skeys = np.sort(voxel_keys(cloud))
    assert (skeys[first:first + g] == skeys[first]).all() and len(np.unique(skeys)) == len(cloud) - g + 1  # as crafted
    reg = gpu_api.RegistrationGICP(max_points=CAP)
    reg.RegisterPointClouds(cloud, plain)
    paths = reg.voxel_sort_paths()
    _assert_means_are_the_oracles(reg, oracle, (cloud, plain))
    want = dict(harmless=int(CRAFTED[case] == "harmless"), replica=int(CRAFTED[case] == "replica"))
    assert paths["tie_free"] > 0 and paths["harmless"] == want["harmless"] and paths["replica"] == want["replica"], (case, paths)
    assert _numpy_says_harmless(oracle, cloud) == (CRAFTED[case] == "harmless")
    assert _numpy_says_harmless(oracle, plain)


def collect_preprocessed(api):
    """Leaf paths, downsampled points and covariances of both clouds for the two bench scenes and the crafted clouds."""
    out = {}
    reg = api.RegistrationGICP(max_points=CAP)
    pairs = [("s%d" % s, synth.frame_pair(s, 640, 480, 4)) for s in (1000, 1300)]
    pairs = [(name, fp["cloud0"], fp["cloud1"]) for name, fp in pairs]
    pairs += [(c, crafted_cloud(c)[0], crafted_cloud("plain")[0]) for c in sorted(CRAFTED)]
    for name, a, b in pairs:
        reg.RegisterPointClouds(a, b)
        p = reg.voxel_sort_paths()
        out[name + "_paths"] = np.array([p["tie_free"], p["harmless"], p["replica"]])
        for which in (0, 1):
            pts, covs = reg.preprocessed(0, which)
            out["%s_p%d" % (name, which)] = pts
            out["%s_c%d" % (name, which)] = covs
    return out


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from geoflowslam_amd import api
from test_gpu_voxel_leaf_paths import collect_preprocessed
np.savez(sys.argv[2], **collect_preprocessed(api))
"""


def test_exact_ties_knob_gives_the_same_points_and_covariances(gpu_api, tmp_path):
    """GFS_GICP_VOXEL_TIES=exact (the reference's permutation in every range with equal keys) in a child process against the
    default in this one: downsampled points and covariances equal bit for bit, and no range called harmless under the knob."""
    assert os.environ.get("GFS_GICP_VOXEL_TIES") != "exact"
    default = collect_preprocessed(gpu_api)
    path = str(tmp_path / "exact.npz")
    cp = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=dict(os.environ, GFS_GICP_VOXEL_TIES="exact"),
                        capture_output=True, text=True, timeout=300)
    assert cp.returncode == 0, cp.stderr[-2000:]
    exact = dict(np.load(path))
    assert sorted(default) == sorted(exact)
    for key, d in default.items():
        e = exact[key]
        if key.endswith("_paths"):
            assert e[1] == 0 and e[2] == d[1] + d[2] and e[0] == d[0], (key, d, e)
            continue
        assert d.shape == e.shape and d.tobytes() == e.tobytes(), key
    assert sum(int(d[1]) for k, d in default.items() if k.endswith("_paths")) > 0
