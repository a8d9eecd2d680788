"""Pins the oracle against the REFERENCE'S OWN CODE where that code can be compiled here: small_gicp's util/sort_omp.hpp
(quick_sort_omp: the voxel sort of voxelgrid_sampling_omp, util/downsampling_omp.hpp:56) and ann/knn_result.hpp (KnnResult, the k-NN
result container of ann/kdtree.hpp:194-233) build from /root/reference without OpenCV / Eigen (oracle/ref_build.sh ->
oracle/_ref/libgfs_ref_small_gicp.so; every other hot-path source includes one of the two and is unbuildable in this image).
The reference runs its sort with OpenMP tasks on 4 threads (src/RegistrationGICP.cc:10); the tasks own disjoint ranges, so the
permutation does not depend on the thread count -- checked here with 1, 4 and 7 threads.

The reference library's results are recorded as SHA-256 digests in tests/golden/ref_small_gicp_results.json: the oracle is checked
against the record everywhere, and against the library itself (which must still produce the record) wherever oracle/_ref is built.
`PYTHONPATH=. python tests/test_oracle_ref.py` rewrites the record from the library."""
import hashlib
import json
import os

import numpy as np

from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_small_gicp_results.json")


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _recorded(section):
    return json.load(open(GOLDEN))[section]


def _voxel_keys(x, y, z):
    return (np.asarray(x, np.uint64) & 0x1FFFFF) | ((np.asarray(y, np.uint64) & 0x1FFFFF) << 21) | ((np.asarray(z, np.uint64) & 0x1FFFFF) << 42)


def sort_cases():
    rng = np.random.default_rng(11)
    cases = []
    for n in (0, 1, 2, 15, 16, 17, 100, 1023, 1024, 1025, 2047, 2048, 4097, 9000, 20000, 36864, 40000):
        for mode in range(6):
            if mode == 0:    # few distinct voxels: heavy ties
                x, y, z = rng.integers(0, 4, n), rng.integers(0, 3, n), rng.integers(0, 2, n)
            elif mode == 1:  # nearly all distinct
                x, y, z = rng.integers(0, 2000, n), rng.integers(0, 2000, n), rng.integers(0, 50, n)
            elif mode == 2:  # sorted, runs of equal keys (raster-ordered depth cloud)
                x, y, z = np.arange(n) // 3, np.zeros(n, np.int64), np.zeros(n, np.int64)
            elif mode == 3:  # reversed
                x, y, z = (n - np.arange(n)) // 2, np.ones(n, np.int64), np.ones(n, np.int64)
            elif mode == 4:  # all equal
                x, y, z = np.full(n, 7), np.full(n, 9), np.full(n, 11)
            else:            # organ pipe
                x, y, z = np.minimum(np.arange(n), n - np.arange(n)) // 2, np.zeros(n, np.int64), np.zeros(n, np.int64)
            k = _voxel_keys(np.asarray(x) + 1000, np.asarray(y) + 2000, np.asarray(z) + 3000)
            if mode in (0, 1) and n > 10:  # out-of-range points carry the all-ones key
                k[rng.integers(0, n, max(1, n // 50))] = np.uint64(0xFFFFFFFFFFFFFFFF)
            cases.append((f"n{n}-m{mode}", k))
    for n in (100, 700, 1000, 1023):  # McIlroy's adversary for std::sort: the heap-sort fallback of the leaves
        a = O.antiqsort_keys(n).astype(np.int64)
        for div in (1, 2, 3):
            cases.append((f"antiqsort{n}/{div}", _voxel_keys(a // div + 5, np.full(n, 3), np.full(n, 1))))
    return cases


def depth_cases():
    """The keys the path really sorts: voxel coordinates of the synthetic RGB-D clouds (raster order, 0.25 m / 0.1 m leaves)."""
    from geoflowslam_amd import synth
    cases = []
    for seed in (1, 2, 202):
        fp = synth.frame_pair(seed)
        for key in ("cloud0", "cloud1"):
            pts = np.asarray(fp[key], np.float64)[:, :3]
            for leaf in (0.25, 0.1):
                c = np.floor(pts / leaf).astype(np.int64) + (1 << 20)
                cases.append((f"{seed}/{key}/{leaf}", _voxel_keys(c[:, 0], c[:, 1], c[:, 2])))
    return cases


def knn_cases():
    rng = np.random.default_rng(3)
    cases = []
    for case in range(400):
        k = int(rng.choice([1, 2, 10, 11, 20]))
        n = int(rng.integers(0, 200))
        d = rng.uniform(0, 1, n)
        if n and case % 2:
            d = np.round(d * 8) / 8  # exact distance ties: the first pushed stays ahead (strict <)
        idx = rng.integers(0, 1 << 40, n).astype(np.uint64)
        cases.append((case, k, idx, d))
    return cases


def _ref_sort_digests(cases):
    return {name: _digest(*O.ref_quick_sort_perm(k, 4)) for name, k in cases}


def _ref_knn_digest():
    h = [O.knn_push_stream(k, idx, d, ref=True) for _, k, idx, d in knn_cases()]
    return _digest(*[np.array([n], np.int64) for n, _, _ in h], *[a for _, io, do in h for a in (io, do)])


def test_restated_quick_sort_omp_is_the_references_permutation():
    rec = _recorded("sort")
    for name, k in sort_cases():
        got, gk = O.quick_sort_perm(k)
        assert _digest(got, gk) == rec[name], name
        if O.ref_lib() is not None:
            want, wk = O.ref_quick_sort_perm(k, 4)
            assert np.array_equal(gk, wk) and np.array_equal(got, want), (name, int((got != want).sum()))
            for threads in (1, 7):
                other, _ = O.ref_quick_sort_perm(k, threads)
                assert np.array_equal(other, want), (name, threads)


def test_restated_quick_sort_omp_on_depth_camera_clouds():
    """The keys the path really sorts: voxel coordinates of the synthetic RGB-D clouds (raster order, 0.25 m / 0.1 m leaves)."""
    rec = _recorded("depth")
    for name, k in depth_cases():
        got, gk = O.quick_sort_perm(k)
        assert _digest(got, gk) == rec[name], name
        if O.ref_lib() is not None:
            want, _ = O.ref_quick_sort_perm(k, 4)
            assert np.array_equal(got, want), name


def test_restated_knn_result_is_the_references_container():
    got_all = []
    for case, k, idx, d in knn_cases():
        got = O.knn_push_stream(k, idx, d)
        got_all.append(got)
        if O.ref_lib() is not None:
            want = O.knn_push_stream(k, idx, d, ref=True)
            assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (case, k, len(idx))
            if k == 1:  # the static N = 1 specialisation (the correspondence search of gicp_factor.hpp:35-73)
                one = O.knn_push_stream(1, idx, d, ref=True, static_one=True)
                assert got[0] == one[0] and np.array_equal(got[1], one[1]) and np.array_equal(got[2], one[2])
    assert _digest(*[np.array([n], np.int64) for n, _, _ in got_all], *[a for _, io, do in got_all for a in (io, do)]) == _recorded("knn")
    if O.ref_lib() is not None:  # the library still produces the record
        assert _ref_knn_digest() == _recorded("knn")
        assert _ref_sort_digests(sort_cases()) == _recorded("sort") and _ref_sort_digests(depth_cases()) == _recorded("depth")


if __name__ == "__main__":
    assert O.ref_lib() is not None, "oracle/_ref not built (bash oracle/ref_build.sh)"
    with open(GOLDEN, "w") as f:
        json.dump(dict(sort=_ref_sort_digests(sort_cases()), depth=_ref_sort_digests(depth_cases()), knn=_ref_knn_digest()), f, indent=1)
        f.write("\n")
    print(f"wrote {GOLDEN}")
