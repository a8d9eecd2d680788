"""The brute-force Hamming matcher (k_bf_hamming, csrc/match.hip: the distance as an i8 matrix product) against a numpy
brute force, index and distance equal, at every size where the kernel changes path: the 32-row accumulator blocks and their
two half-lanes, the 128-row tiles, the 64 queries of a wave and the 256 of a workgroup; ties across each of those boundaries
(the LOWEST train index wins, cv::batchDistance); distances 0 and 256; ragged batches with empty frames; and buffers whose
rows beyond the counts hold a descriptor that would win."""
import numpy as np
import pytest

from test_gpu_gms import _Hip

pytestmark = pytest.mark.gpu

SENTINEL = -7777
SIZES = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257]


def _ref(q, t):
    """np.unpackbits, xor, sum, argmin of dist * 2**20 + idx: smallest distance, lowest index among equals."""
    q, t = q.reshape(-1, 32), t.reshape(-1, 32)
    if len(t) == 0:
        return np.full(len(q), -1, np.int64), np.full(len(q), 0x7FFFFFFF, np.int64)
    qb, tb = np.unpackbits(q, axis=1), np.unpackbits(t, axis=1)
    idx, dist = np.zeros(len(q), np.int64), np.zeros(len(q), np.int64)
    for a in range(0, len(q), 64):
        d = (qb[a:a + 64, None, :] ^ tb[None, :, :]).sum(2, dtype=np.int64)
        key = d * 2 ** 20 + np.arange(len(t), dtype=np.int64)[None, :]
        j = key.argmin(1)
        idx[a:a + 64], dist[a:a + 64] = j, d[np.arange(len(j)), j]
    return idx, dist


def _match_batch(gpu_api, frames, stride):
    """One call of the batched device entry on B = len(frames) frames (q, t).  Every row of the two buffers beyond a frame's
    counts holds a copy of the frame's first query (a row that would win at distance 0); the outputs start as SENTINEL."""
    B = len(frames)
    qbuf, tbuf = np.zeros((B, stride, 32), np.uint8), np.zeros((B, stride, 32), np.uint8)
    for b, (q, t) in enumerate(frames):
        bait = q[0] if len(q) else np.full(32, 0x5A, np.uint8)
        qbuf[b], tbuf[b] = bait, bait
        qbuf[b, :len(q)], tbuf[b, :len(t)] = q, t
    hip = _Hip()
    try:
        d_q, d_t = hip.to_device(qbuf), hip.to_device(tbuf)
        d_nq = hip.to_device(np.array([len(q) for q, _ in frames], np.int32))
        d_nt = hip.to_device(np.array([len(t) for _, t in frames], np.int32))
        d_i, d_d = hip.to_device(np.full(B * stride, SENTINEL, np.int32)), hip.to_device(np.full(B * stride, SENTINEL, np.int32))
        mt = gpu_api.ORBmatcher(max_query=stride, max_train=stride, max_batch=B)
        mt.match_batch_device(d_q, d_nq, d_t, d_nt, B, stride, d_i, d_d, hip.stream())
        idx, dist = hip.to_host(d_i, (B, stride), np.int32), hip.to_host(d_d, (B, stride), np.int32)
        mt.close()
    finally:
        hip.free()
    return idx, dist


def _check(frames, idx, dist):
    for b, (q, t) in enumerate(frames):
        ri, rd = _ref(q, t)
        nq = len(q)
        assert np.array_equal(idx[b, :nq], ri) and np.array_equal(dist[b, :nq], rd), \
            f"frame {b} ({nq} x {len(t)}): {int((idx[b, :nq] != ri).sum())} indices, {int((dist[b, :nq] != rd).sum())} distances differ"
        assert (idx[b, nq:] == SENTINEL).all() and (dist[b, nq:] == SENTINEL).all(), f"frame {b}: wrote beyond nq = {nq}"


def _rand(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _flip(row, bits):
    out = row.copy()
    for k in bits:
        out[k // 8] ^= np.uint8(1 << (k % 8))
    return out


def _edge_pairs():
    n = len(SIZES)
    pairs = [(1, 1), (257, 1), (1, 257)]
    for i, s in enumerate(SIZES):
        pairs += [(s, s), (s, SIZES[n - 1 - i]), (s, SIZES[(i + 5) % n]), (s, SIZES[(i + 9) % n])]
    return sorted(set(pairs))


def test_tile_and_fragment_edges(gpu_api):
    """(nq, nt) over the block, wave, tile and workgroup sizes and their neighbours, every value on both sides, one call."""
    pairs = _edge_pairs()
    assert {a for a, _ in pairs} == set(SIZES) == {b for _, b in pairs} and {(1, 1), (257, 1), (1, 257)} <= set(pairs)
    rng = np.random.default_rng(11)
    frames = [(_rand(rng, a), _rand(rng, b)) for a, b in pairs]
    _check(frames, *_match_batch(gpu_api, frames, 300))


# a repeated row at indices on both sides of: the ends of the set; the half-lanes of an accumulator block (rows 3 | 4, 7 | 8);
# the 32-row blocks; the 128-row tiles; and rows a different wave would own if the waves split a tile's rows by 32 or by 64
TIE_SETS = [(0, 299), (3, 4), (7, 8), (31, 32), (63, 64), (95, 96), (127, 128), (128, 299), (159, 160), (255, 256), (256, 287),
            (5, 37, 69, 101, 133, 165, 197, 229, 261, 293), (299,), (131, 4), (260, 129, 30)]


@pytest.mark.parametrize("d", [0, 5])
def test_ties_take_the_lowest_index(gpu_api, d):
    """Query 0 lies at distance d from a row repeated across every boundary of the kernel while every other row is farther
    (random rows: about 128 +- 8): the answer is the lowest index of the repeated row, at distance d."""
    rng = np.random.default_rng(23 + d)
    frames = []
    for where in TIE_SETS:
        t, row = _rand(rng, 300), _rand(rng, 1)[0]
        t[list(where)] = row
        q = _rand(rng, 70)
        q[0] = q[33] = q[69] = _flip(row, range(17, 17 + 7 * d, 7))
        frames.append((q, t))
    idx, dist = _match_batch(gpu_api, frames, 320)
    for b, where in enumerate(TIE_SETS):
        for k in (0, 33, 69):
            assert (idx[b, k], dist[b, k]) == (min(where), d), (where, k, idx[b, k], dist[b, k])
    _check(frames, idx, dist)


def test_extremes(gpu_api):
    """All-zero against all-one descriptors (256 everywhere, index 0), both ways; a set against itself (0 at the own row,
    or at an earlier copy of it)."""
    rng = np.random.default_rng(5)
    zeros, ones = np.zeros((130, 32), np.uint8), np.full((257, 32), 255, np.uint8)
    same = _rand(rng, 200)
    same[150] = same[20]
    frames = [(zeros, ones), (ones, zeros), (same, same), (zeros, zeros[:33]), (ones[:1], ones)]
    idx, dist = _match_batch(gpu_api, frames, 288)
    assert (idx[0, :130] == 0).all() and (dist[0, :130] == 256).all() and (idx[1, :257] == 0).all() and (dist[1, :257] == 256).all()
    own = np.arange(200)
    own[150] = 20
    assert np.array_equal(idx[2, :200], own) and (dist[2, :200] == 0).all()
    assert (idx[3, :130] == 0).all() and (dist[3, :130] == 0).all() and (idx[4, 0], dist[4, 0]) == (0, 0)
    _check(frames, idx, dist)


def test_ragged_batch_and_rows_beyond_the_counts(gpu_api):
    """Five frames of different (nq, nt), one without queries and one without train rows, stride_rows above every count.
    The rows of both buffers beyond the counts repeat the frame's first query: matched, it would show as an index >= nt at
    distance 0.  Entries at or beyond nq keep the sentinel; the frame without train rows has -1 / 0x7fffffff."""
    rng = np.random.default_rng(41)
    shapes = [(100, 77), (0, 50), (40, 0), (257, 129), (1, 300)]
    frames = [(_rand(rng, a), _rand(rng, b)) for a, b in shapes]
    idx, dist = _match_batch(gpu_api, frames, 333)
    assert (idx[1] == SENTINEL).all() and (dist[1] == SENTINEL).all()
    assert (idx[2, :40] == -1).all() and (dist[2, :40] == 0x7FFFFFFF).all()
    for b, (a, n) in enumerate(shapes):
        if n:
            assert (idx[b, :a] >= 0).all() and (idx[b, :a] < n).all() and (dist[b, :a] > 0).all(), f"frame {b} matched a row beyond nt"
    _check(frames, idx, dist)


def test_one_full_frame_device_and_host_entry(gpu_api):
    """One frame of 1000 x 1003 (the bench's size: several tiles, a partial last tile and a partial last workgroup) through
    the batched device entry and through the host entry, which also keeps its early return for an empty set."""
    rng = np.random.default_rng(77)
    q, t = _rand(rng, 1000), _rand(rng, 1003)
    t[1002], t[640] = q[999], q[999]
    ri, rd = _ref(q, t)
    assert (ri[999], rd[999]) == (640, 0)
    idx, dist = _match_batch(gpu_api, [(q, t)], 1064)
    _check([(q, t)], idx, dist)
    mt = gpu_api.ORBmatcher(max_query=1100, max_train=1100)
    hi, hd = mt.match(q, t)
    assert np.array_equal(hi, ri) and np.array_equal(hd, rd)
    ei, ed = mt.match(q, t[:0])
    assert len(ei) == 0 and len(ed) == 0
    mt.close()
