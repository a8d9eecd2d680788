"""csrc/eig3_direct.hpp picks the columns of Eigen's closed-form 3 x 3 eigen-decomposition by selects; gicp.hip used to index private
arrays by i0, k and l.  tests/host/eig3_forms.cpp holds the indexed form as it stood next to the header, both
compiled for the host with -ffp-contract=off and both on the host's atan2, so the two can differ in structure only.  Every test here
requires all nine doubles of V to be bit-equal, and that the decisions it is about were really taken (the indexed form counts them).
No GPU."""
import ctypes as C
import functools
import itertools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "eig3_forms.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_eig3_forms.so")
_CSRC = os.path.join(ROOT, "geoflowslam_amd", "csrc")
HITS = ("i0=0", "i0=1", "i0=2", "diag_tie", "n0>n1", "n0==n1", "n0<n1", "scale==0", "identity", "d0>d1", "d0==d1", "d0<d1", "two_equal",
        "second_extract")
EPS = 2.220446049250313e-16


@functools.lru_cache(maxsize=None)
def forms():
    deps = [_SRC] + [os.path.join(_CSRC, f) for f in ("eig3_direct.hpp", "glibc_math.hpp", "glibc_tables.inc")]
    if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
        tmp = _SO + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-O2", "-std=c++17", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", tmp, _SRC], check=True)
        os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    vp = C.c_void_p
    L.ef_compare.argtypes = [vp, C.c_int64, vp, vp]
    L.ef_compare.restype = C.c_int64
    for f in (L.ef_indexed, L.ef_selects):
        f.argtypes, f.restype = [vp, vp], None
    return L


def compare(cov6):
    """-> {decision: count}; asserts bit equality of V on every row of cov6 [n, 6] = (xx, xy, xz, yy, yz, zz)."""
    cov6 = np.ascontiguousarray(cov6, np.float64).reshape(-1, 6)
    hits, first = np.zeros(16, np.int64), np.zeros(1, np.int64)
    bad = forms().ef_compare(cov6.ctypes.data, len(cov6), first.ctypes.data, hits.ctypes.data)
    assert bad == 0, (bad, len(cov6), int(first[0]), cov6[int(first[0])].tolist())
    return dict(zip(HITS, (int(h) for h in hits)))


def selects(cov6):
    V = np.zeros(9)
    c = np.ascontiguousarray(cov6, np.float64)
    forms().ef_selects(c.ctypes.data, V.ctypes.data)
    return V.reshape(3, 3).T  # columns = eigenvectors


def sym6(m):
    m = np.asarray(m, np.float64)
    return np.stack([m[..., 0, 0], m[..., 1, 0], m[..., 2, 0], m[..., 1, 1], m[..., 2, 1], m[..., 2, 2]], -1)


def neighbourhood_covariances(rng, n, k=10):
    """Covariances as knn_write_cov forms them (sums, mean = sum / k, (sum of products - mean * sum) / k) of k points around a centre
    within +-30 m, spread 1 mm .. 10 cm along each axis of a random frame."""
    centre = rng.uniform(-30, 30, (n, 1, 3))
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    sd = 10.0 ** rng.uniform(-3, -1, (n, 1, 3))
    p = centre + np.einsum("nkj,nij->nki", rng.normal(size=(n, k, 3)) * sd, q)
    sp = p.sum(1)
    mean = sp / k
    out = np.empty((n, 6))
    for o, (r, c) in enumerate(((0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2))):
        out[:, o] = ((p[:, :, r] * p[:, :, c]).sum(1) - mean[:, c] * sp[:, r]) / k
    return out


def test_a_million_neighbourhood_covariances():
    rng = np.random.default_rng(20240601)
    hits = {}
    for _ in range(4):
        for k, v in compare(neighbourhood_covariances(rng, 250_000)).items():
            hits[k] = hits.get(k, 0) + v
    print(hits)
    assert hits["i0=0"] + hits["i0=1"] + hits["i0=2"] >= 1_000_000
    for k in ("i0=0", "i0=1", "i0=2", "n0>n1", "n0<n1", "d0>d1", "d0<d1", "second_extract"):
        assert hits[k] > 10_000, (k, hits)


def test_the_selects_form_is_an_eigen_decomposition():
    """(so the two forms are not equal and wrong: V orthonormal, columns ascending, against numpy on well separated spectra)"""
    rng = np.random.default_rng(3)
    for c in neighbourhood_covariances(rng, 200):
        m = np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]])
        w, _ = np.linalg.eigh(m)
        if min(w[1] - w[0], w[2] - w[1]) < 1e-3 * w[2]:
            continue
        V = selects(c)
        assert np.abs(V.T @ V - np.eye(3)).max() < 1e-9
        assert np.abs(m @ V - V * w).max() < 1e-9 * w[2]


def _permuted(mats):
    """every matrix under the six relabellings of the axes"""
    mats = np.asarray(mats, np.float64).reshape(-1, 3, 3)
    return np.concatenate([mats[:, p][:, :, p] for p in map(list, itertools.permutations(range(3)))])


def test_every_i0_and_ties_of_the_absolute_diagonal():
    """tmp = s - ev I with two or three equal diagonal entries: the strict > keeps the first of them."""
    rng = np.random.default_rng(11)
    n = 4000
    p, q, r, t = (rng.uniform(-1, 1, n) for _ in range(4))
    z = np.zeros(n)
    two = np.array([[p, q, z], [q, p, z], [z, z, r]]).transpose(2, 0, 1)          # xx == yy
    two_b = np.array([[p, q, t], [q, p, t], [t, t, r]]).transpose(2, 0, 1)        # xx == yy, full
    three = np.array([[p, q, q], [q, p, q], [q, q, p]]).transpose(2, 0, 1)        # xx == yy == zz, eigenvalues p + 2q, p - q twice
    three_b = np.array([[p, q, t], [q, p, r], [t, r, p]]).transpose(2, 0, 1)      # xx == yy == zz, distinct eigenvalues
    diag = np.array([[p, z, z], [z, q, z], [z, z, r]]).transpose(2, 0, 1)
    hits = compare(sym6(_permuted(np.concatenate([two, two_b, three, three_b, diag]))))
    print(hits)
    for k in ("i0=0", "i0=1", "i0=2"):
        assert hits[k] > 1000, (k, hits)
    assert hits["diag_tie"] > 10_000, hits


def test_swap_and_equal_gaps():
    """sw true, sw false and d0 == d1: spectra (-1, t, 1) with t a few units of 2^-53 around 0, where d0 - d1 changes sign."""
    t = np.arange(-600, 601) * 2.0 ** -53
    n = len(t)
    z, one = np.zeros(n), np.ones(n)
    diag = np.array([[-one, z, z], [z, t, z], [z, z, one]]).transpose(2, 0, 1)
    offd = np.array([[t / 2, one, z], [one, t / 2, z], [z, z, t]]).transpose(2, 0, 1)  # eigenvalues t / 2 -+ 1, t
    scales = np.array([1.0, 3.0, 1e-4, 7e-6])[:, None, None, None]
    hits = compare(sym6(_permuted((np.concatenate([diag, offd])[None] * scales).reshape(-1, 3, 3))))
    print(hits)
    assert hits["d0>d1"] > 1000 and hits["d0<d1"] > 1000, hits
    assert hits["d0==d1"] > 0, hits


def test_two_equal_eigenvalues():
    """d0 <= 2 eps d1: the second vector comes from the first call's representative column, not from a second call."""
    rng = np.random.default_rng(5)
    n = 3000
    a, b = rng.uniform(0.1, 2, n), rng.uniform(2.5, 5, n)
    z = np.zeros(n)
    mats = [np.array([[a, z, z], [z, a, z], [z, z, b]]).transpose(2, 0, 1), np.array([[b, z, z], [z, a, z], [z, z, a]]).transpose(2, 0, 1)]
    # a I + c v v^T, v of small integers: the double eigenvalue survives the arithmetic in many of them
    v = rng.integers(-3, 4, (n, 3)).astype(np.float64)
    v[(v == 0).all(1)] = (1, 2, 2)
    mats.append(a[:, None, None] * np.eye(3) + np.einsum("ni,nj->nij", v, v) * rng.choice([-0.25, 0.5, 1.0], n)[:, None, None])
    hits = compare(sym6(_permuted(np.concatenate(mats))))
    print(hits)
    assert hits["two_equal"] > 10_000 and hits["d0>d1"] > 1000 and hits["d0<d1"] > 1000, hits


def test_multiples_of_the_identity_and_zero():
    c = np.array([0.0, -0.0, 1.0, -1.0, 1e-300, 1e300, 3.7e-5, EPS, 5e-324, 0.1])
    z = np.zeros_like(c)
    cov6 = np.stack([c, z, z, c, z, c], 1)
    hits = compare(cov6)
    print(hits)
    assert hits["identity"] == len(c), hits
    assert hits["scale==0"] >= 2, hits  # the two zeros (0.1 * 3 / 3 != 0.1: a multiple of the identity may leave a residue)
    # spectra one or two eps wide after scaling: on both sides of `ev[2] - ev[0] <= eps`
    k = np.arange(0, 40)
    near = np.stack([1 + 0 * k, 0 * k, 0 * k, 1 + k * EPS, 0 * k, 1 + 2 * k * EPS], 1).astype(np.float64)
    hits = compare(near)
    print(hits)
    assert hits["identity"] > 0, hits
    assert np.array_equal(selects(cov6[2]), np.eye(3))


def test_rank_one_and_rank_two():
    rng = np.random.default_rng(7)
    n = 20_000
    u, v = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    ui, vi = rng.integers(-4, 5, (n, 3)).astype(np.float64), rng.integers(-4, 5, (n, 3)).astype(np.float64)
    e = np.eye(3)
    r1 = [np.einsum("ni,nj->nij", w, w) for w in (u, ui, 1e-3 * u, np.repeat(e, 2, 0), np.array([[1.0, 1, 0], [1, 1, 1], [0, 1, -1]]))]
    r2 = [np.einsum("ni,nj->nij", a, a) + np.einsum("ni,nj->nij", b, b) for a, b in ((u, v), (ui, vi), (1e-2 * u, 1e-3 * v))]
    r2.append(np.array([np.diag(d) for d in ((1.0, 1, 0), (1, 0, 1), (0, 1, 1), (2, 1, 0), (0, 3, 1), (1, 0, 0.5))]))
    for what, mats in (("rank 1", r1), ("rank 2", r2)):
        hits = compare(sym6(np.concatenate(mats)))
        print(what, hits)
        assert hits["second_extract"] > 1000, (what, hits)
    assert compare(sym6(np.concatenate(r1)))["two_equal"] > 1000  # a plane of zeros: the two smallest coincide in many


def test_equal_cross_products():
    """n0 == n1: a matrix that is symmetric under the exchange of two axes gives the two cross products the same entries in another
    order; where the sums round alike the strict > takes the second."""
    rng = np.random.default_rng(13)
    n = 20_000
    p, q, r, t = (rng.integers(-8, 9, n).astype(np.float64) / 4 for _ in range(4))
    m = np.array([[p, q, q], [q, r, t], [q, t, r]]).transpose(2, 0, 1)
    mr = np.array([[p, q, q], [q, r, t], [q, t, r]]).transpose(2, 0, 1) * rng.uniform(0.5, 2, n)[:, None, None]
    hits = compare(sym6(_permuted(np.concatenate([m, mr]))))
    print(hits)
    assert hits["n0==n1"] > 100 and hits["n0>n1"] > 100 and hits["n0<n1"] > 100, hits


def test_non_finite_input_gives_the_same_bits():
    """(a cloud never holds them; the two forms must still agree, NaN for NaN)"""
    x = np.array([[np.nan, 0, 0, 1, 0, 1], [1, np.inf, 0, 1, 0, 1], [1, 0, 0, -np.inf, 0, 1], [np.inf, np.inf, np.inf, np.inf, np.inf, np.inf]])
    compare(x)
