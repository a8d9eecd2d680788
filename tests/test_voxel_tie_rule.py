"""The rule by which the voxel sort's leaf ranges (csrc/voxel_qsort.hpp: TieRule, k_voxel_qsort_leaf, k_voxel_qsort_heap) may leave
equal keys in position order instead of replaying libstdc++'s introsort: restated in numpy and checked on the CPU against what it
promises -- the voxel means of voxelgrid_sampling_omp (util/downsampling_omp.hpp:57-90: 1024-element blocks of the sorted array,
coordinates added up in double precision in sorted order) are the same doubles whichever order the ties of a passing range are in.
tests/test_gpu_voxel_leaf_paths.py checks the device's decisions against the same restatement."""
import numpy as np

LEAF = 0.02
BLOCK = 1024
OFFSET = 1 << 20


def voxel_keys(points):
    """(z, y, x) 21-bit voxel fields of float32 points at the 0.02 m leaf, packed as downsampling_omp.hpp:47-51 does."""
    c = np.floor(points[:, :3].astype(np.float64) * (1.0 / LEAF)).astype(np.int64) + OFFSET
    return (c[:, 0].astype(np.uint64) | (c[:, 1].astype(np.uint64) << np.uint64(21)) | (c[:, 2].astype(np.uint64) << np.uint64(42)))


def range_is_harmless(skeys, b, pts_sorted):
    """The device's predicate for the sorted range that starts at position b of the cloud's sorted array: skeys = its sorted keys,
    pts_sorted = the float32 points in that order.  True also for a range without equal keys."""
    n = len(skeys)
    head = np.ones(n, bool)
    head[1:] = skeys[1:] != skeys[:-1]
    starts = np.nonzero(head)[0]
    sizes = np.diff(np.append(starts, n))
    tied_groups = sizes > 1
    if not tied_groups.any():
        return True
    first = b + starts[tied_groups]
    g = sizes[tied_groups]
    if (g > 64).any() or ((first >> 10) != ((first + g - 1) >> 10)).any():
        return False
    tied = np.repeat(tied_groups, sizes)
    bits = pts_sorted[tied, :3].astype(np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    if (bits >= 0x7F800000).any():
        return False
    e = np.maximum(bits[bits != 0] >> np.uint32(23), 1).astype(np.int64)
    return len(e) == 0 or int(e.max() - e.min()) < 23


def voxel_means(skeys, pts_sorted):
    """voxelgrid_sampling_omp's block-wise sums over an already sorted cloud (no invalid keys): one mean per run of equal keys
    inside a 1024-element block, every run added up sequentially in double precision.  -> (keys, block, means[., 3]) in array order."""
    n = len(skeys)
    start = np.ones(n, bool)
    start[1:] = skeys[1:] != skeys[:-1]
    start[np.arange(0, n, BLOCK)] = True
    s = np.nonzero(start)[0]
    sizes = np.diff(np.append(s, n))
    p = pts_sorted[:, :3].astype(np.float64)
    acc = np.zeros((len(s), 3))
    for j in range(int(sizes.max())):  # sequential inside a run, all runs at once
        m = sizes > j
        acc[m] += p[s[m] + j]
    return skeys[s], s // BLOCK, acc / sizes[:, None].astype(np.float64)


def _random_cloud(rng):
    n = int(rng.integers(3000, 6001))
    tie_frac = rng.uniform(0.10, 0.40)
    big = rng.random() < 0.5  # some clouds hold groups above the 64-point limit
    sizes = []
    left = n
    tied_left = int(tie_frac * n)
    while left > 0:
        g = 1
        if tied_left > 1 and rng.random() < 0.15:
            g = int(min(left, tied_left, rng.integers(2, 81 if big else 9)))
            tied_left -= g
        sizes.append(g)
        left -= g
    nv = len(sizes)
    side = int(np.ceil(np.sqrt(nv))) + 1
    cells = rng.choice(side * side, nv, replace=False)
    ix, iy = cells % side - side // 2, cells // side - side // 2   # voxels on both sides of the origin
    iz = rng.integers(20, 60, nv)
    vox = np.repeat(np.stack([ix, iy, iz], 1), sizes, axis=0)
    pts = np.ones((n, 4), np.float32)
    pts[:, :3] = ((vox + rng.uniform(0.05, 0.95, (n, 3))) * LEAF).astype(np.float32)
    mode = rng.integers(0, 4)
    if mode == 1:    # coordinates next to zero inside the voxels that touch an axis plane: the exponent window
        near = (vox[:, 0] == 0) & (rng.random(n) < 0.3)
        pts[near, 0] = np.float32(1e-9) * rng.uniform(0.1, 1.0, int(near.sum())).astype(np.float32)
    elif mode == 2:  # exact zeros add exactly
        pts[(vox[:, 1] == 0) & (rng.random(n) < 0.3), 1] = 0.0
    pts = pts[rng.permutation(n)]
    assert (voxel_keys(pts) >> np.uint64(63) == 0).all()
    return pts


def test_harmless_ranges_give_the_same_means_in_any_tie_order(oracle):
    rng = np.random.default_rng(20240607)
    n_passing = n_failing = n_tied_passing = 0
    for _ in range(200):
        pts = _random_cloud(rng)
        keys = voxel_keys(pts)
        perm, skeys = oracle.quick_sort_perm(keys)
        n = len(keys)
        head = np.ones(n, bool)
        head[1:] = skeys[1:] != skeys[:-1]
        bounds = np.nonzero(head)[0]
        # ranges as the quicksort's leaves are: below 1024 elements, never cutting through a group of equal keys
        other = perm.copy()
        b = 0
        while b < n:
            e = min(n, b + int(rng.integers(200, 1024)))
            if e < n:
                cand = bounds[(bounds > b) & (bounds <= e)]
                e = int(cand[-1]) if len(cand) else int(np.append(bounds[bounds > b], n)[0])
            rk, rp = skeys[b:e], perm[b:e]
            if range_is_harmless(rk, b, pts[rp]):
                n_passing += 1
                n_tied_passing += int((rk[1:] == rk[:-1]).any())
                other[b:e] = rp[np.lexsort((rp, rk))]   # ties by position
            else:
                n_failing += 1
            b = e
        assert (keys[other] == skeys).all()
        k0, b0, m0 = voxel_means(skeys, pts[perm])
        k1, b1, m1 = voxel_means(skeys, pts[other])
        assert (k0 == k1).all() and (b0 == b1).all()
        assert (m0.view(np.uint64) == m1.view(np.uint64)).all(), "a range that passed the rule changed a voxel mean"
    # the draw must exercise both outcomes, and passing ranges with ties in them
    assert n_tied_passing > 100 and n_failing > 100, (n_passing, n_tied_passing, n_failing)


def test_the_restated_rule_on_hand_made_voxels():
    """Each of the four conditions on its own: the exponent window, the block cut, the group size."""
    pts = np.ones((2, 4), np.float32)
    pts[:, :3] = [[1e-9, 0.01, 0.01], [0.019, 0.011, 0.012]]
    keys = voxel_keys(pts)
    assert keys[0] == keys[1]
    assert not range_is_harmless(keys, 0, pts)               # exponents 2^-30 and 2^-6
    ok = np.ones((2, 4), np.float32)
    ok[:, :3] = [[0.011, 0.01, 0.01], [0.019, 0.011, 0.012]]
    assert range_is_harmless(voxel_keys(ok), 0, ok) and range_is_harmless(voxel_keys(ok), 1022, ok)
    assert not range_is_harmless(voxel_keys(ok), 1023, ok)  # positions 1023 and 1024: a block cut between them
    big = np.ones((65, 4), np.float32)
    big[:, :3] = 0.01
    assert not range_is_harmless(voxel_keys(big), 0, big) and range_is_harmless(voxel_keys(big[:64]), 0, big[:64])
