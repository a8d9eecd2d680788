"""GPU half of the GICP geometry tests (MI355X): the neighbour searches of csrc/gicp.hip -- k_knn_cov, the r = 2 pass
k_knn_cov_far, the isolated-point pass k_knn_cov_far_wg, the 1-NN walk of k_gicp_linearize
-- on clouds that are NOT depth-camera rasters (tests/gicp_geometry_support.py), against brute-force numpy references that share
nothing with the kernels' cell grid or the oracle's KdTree, and with assertions on WHICH pass answered (gfs_gicp_knn_stats).
tests/test_gicp_geometry_reference.py pins the references and the caps used here on the CPU.

Bars: covariances |gpu - oracle| < 1e-9 (the stage bar of test_preprocess_stage_matches_oracle) and |gpu - reference_cov| <= 1e-9 +
d_or_cov on every point with a relative eigen-gap above 1e-3; ill-conditioned points by what the data defines (eigenvalues, the
normal minimises the neighbourhood's scatter); one linearisation within 100 x max(d_or_lin, 1e-14) of reference_linearize fed with
the GPU's own preprocessed clouds, inliers equal; full registrations by test_gpu_gicp._gicp_same."""
import functools
import os

import numpy as np
import pytest

import gicp_geometry_support as G

pytestmark = pytest.mark.gpu
SEED = G.SEEDS[0]
CAP = 8192  # raw points per cloud: the largest generator draws 6 000
LIN_NAMES = [n for n in G.NAMES if not (n.startswith("tiny_") and int(n[5:]) < 10)]  # clouds of >= 10 points


def _pack(out, key, r):
    out[key + "/T"], out[key + "/H"], out[key + "/b"] = r["T"], r["H"], r["b"]
    out[key + "/f"] = np.array([r["error"]])
    out[key + "/i"] = np.array([r["converged"], r["iterations"], r["num_inliers"], r["n_target_ds"], r["n_source_ds"]], np.int64)


def _unpack(d, key):
    i = d[key + "/i"]
    return dict(T=d[key + "/T"], H=d[key + "/H"], b=d[key + "/b"], error=float(d[key + "/f"][0]), converged=bool(i[0]), iterations=int(i[1]),
                num_inliers=int(i[2]), n_target_ds=int(i[3]), n_source_ds=int(i[4]))


def collect(api, names=G.NAMES, seed=SEED):
    """Everything the tests compare, from ONE fresh handle under the environment of the moment: per cloud the preprocessing of
    (c, c) and its pass counts; per pair (c, moved(c)) one linearisation at init_T (max_iterations = 1) with both preprocessed clouds,
    the full registration from init_T, and the registration of (c, nothing).  A flat dict of arrays."""
    reg = api.RegistrationGICP(max_points=CAP)
    out = {}
    for name in names:
        c = G.cloud(name, seed)
        reg.RegisterPointClouds(c, c)
        out[name + "/pts"], out[name + "/cov"] = reg.preprocessed(0, 0)
        out[name + "/stats"] = reg.knn_stats(0, 0)[0].astype(np.int64)
        src, init_T, _ = G.moved(c, seed)
        cfg = api.gicp_default_config()
        cfg.max_iterations = 1
        _pack(out, name + "/lin", reg.RegisterPointClouds(c, src, init_T, cfg))
        out[name + "/tpts"], out[name + "/tcov"] = reg.preprocessed(0, 0)
        out[name + "/spts"], out[name + "/scov"] = reg.preprocessed(0, 1)
        _pack(out, name + "/full", reg.RegisterPointClouds(c, src, init_T))
    _pack(out, "empty/full", reg.RegisterPointClouds(G.cloud(names[0], seed), np.zeros((0, 4), np.float32)))
    reg.close()
    return out


@pytest.fixture(scope="module")
def default(gpu_api):
    for k in ("GFS_GICP_KNN_EXACT", "GFS_GICP_COOP", "GFS_GICP_CELL"):
        assert k not in os.environ, k + " is set: these tests compare the knobs with the default"
    return collect(gpu_api)


def _to_oracle_order(f, pts, cov):
    """The GPU's covariances in the order of the oracle's points; the voxel means must be the oracle's bit for bit."""
    po = f["po"]
    assert len(pts) == len(po)
    ig, io = G.lexorder(pts), G.lexorder(po)
    assert (pts[ig] == po[io]).all(), "voxel means differ"
    out = np.zeros_like(cov)
    out[io] = cov[ig]
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", G.NAMES)
def test_covariances_match_brute_force(default, name):
    """(a) every point without an exact 10th/11th tie and with a defined plane normal: against the independent reference and the oracle."""
    f = G.facts(name, SEED)
    m = len(f["po"])
    cov = _to_oracle_order(f, default[name + "/pts"], default[name + "/cov"])
    assert int(f["tie"].sum()) <= 0  # the caps of the CPU module, again: no point is left out but these ...
    bad = int((f["gap"] <= G.GAP_MIN).sum())
    assert bad == m if name == "line" else bad <= 0.05 * m  # ... and these, which the next test takes
    if m < 5:
        assert (cov == np.eye(3)).all()  # fewer than 5 neighbours: identity, exactly
        return
    good = f["good"]
    d_ref = np.abs(cov - f["ref"]).reshape(m, -1).max(1)
    d_or = np.abs(cov - f["co"]).reshape(m, -1).max(1)
    print(f"{name}: m {m} compared {int(good.sum())} |gpu - reference| {d_ref[good].max() if good.any() else 0:.2e} "
          f"|gpu - oracle| {d_or[good].max() if good.any() else 0:.2e} d_or_cov {f['d_or_cov']:.2e}")
    assert f["d_or_cov"] <= 1e-9
    if good.any():
        w = int(np.argmax(np.where(good, d_ref, -1)))
        assert d_ref[good].max() <= 1e-9 + f["d_or_cov"], (name, w, d_ref[w], f["d10"][w], f["po"][w], default[name + "/stats"])
        w = int(np.argmax(np.where(good, d_or, -1)))
        assert d_or[good].max() < 1e-9, (name, w, d_or[w], f["d10"][w], f["po"][w], default[name + "/stats"])


@pytest.mark.parametrize("name", G.NAMES)
def test_every_covariance_is_a_plane_of_its_brute_force_neighbourhood(default, oracle, name):
    """(b) what the data defines even where the normal is not (the line, a few loners): symmetric, eigenvalues (1e-3, 1, 1), and the
    normal minimises the scatter S of the brute-force neighbourhood: n^T S n - l0 <= 1e-9 l2.  Held for EVERY point (a wrong
    neighbour set moves S).  The distance from closed_form_cov (same neighbours, the oracle's eigen arithmetic) is printed for the
    ill-conditioned points, next to the oracle's own: DESIGN.md section 2 has the figures."""
    f = G.facts(name, SEED)
    m = len(f["po"])
    cov = _to_oracle_order(f, default[name + "/pts"], default[name + "/cov"])
    if m < 5:
        assert (cov == np.eye(3)).all()
        return
    assert np.abs(cov - cov.transpose(0, 2, 1)).max() <= 1e-15  # (entries are at most 1: symmetric to the last bit or two)
    w, V = np.linalg.eigh(cov)
    assert np.abs(w - np.array([1e-3, 1.0, 1.0])).max() <= 1e-9, np.abs(w - np.array([1e-3, 1.0, 1.0])).max()
    S = G.scatter(f["po"], f["idx"])
    l = np.linalg.eigvalsh(S)
    n = V[:, :, 0]
    excess = np.einsum("ni,nij,nj->n", n, S, n) - l[:, 0]
    worst = int(np.argmax(excess / np.maximum(l[:, 2], 1e-300)))
    print(f"{name}: worst (n^T S n - l0) / l2 = {excess[worst] / l[worst, 2]:.2e} at point {worst} (gap {f['gap'][worst]:.1e})")
    assert (excess <= 1e-9 * l[:, 2]).all(), (name, worst, excess[worst], l[worst], f["d10"][worst])
    sel = np.nonzero(f["gap"] <= G.GAP_MIN)[0]
    if len(sel):
        cf = G.closed_form_cov(f["po"], f["idx"], oracle, sel)
        print(f"{name}: {len(sel)} ill-conditioned points: |gpu - closed_form_cov| {np.abs(cov[sel] - cf).max():.2e} "
              f"|oracle - closed_form_cov| {np.abs(f['co'][sel] - cf).max():.2e} |gpu - oracle| {np.abs(cov[sel] - f['co'][sel]).max():.2e}")


@pytest.mark.parametrize("name", G.NAMES)
def test_the_pass_that_answered(default, name):
    """(c) gfs_gicp_knn_stats = (m, deferred by k_knn_cov to the r = 2 pass, deferred by that to the isolated-point pass) against what
    the true k-th distances allow: k_knn_cov cannot certify beyond 1.5 cells, the r = 2 pass not beyond 2 (unless its cube covers
    the occupied box, which a cloud wider than 0.5 m excludes); and a k-th distance within one cell MUST be certified by k_knn_cov
    unless its keys cannot order the 10th and 11th candidate."""
    f = G.facts(name, SEED)
    pc = G.path_counts(f)
    m, to_r2, to_iso = (int(x) for x in default[name + "/stats"])
    print(f"{name}: m {m} (certified, r = 2, isolated) = ({m - to_r2}, {to_r2 - to_iso}, {to_iso}); brute force {pc}")
    assert m == pc["m"] and 0 <= to_iso <= to_r2 <= m
    if (f["extent"] > 0.5).any():
        assert to_r2 >= pc["must_r2"] and to_iso >= pc["must_isolated"]
    assert to_r2 <= pc["beyond_cell"] + pc["near_ties"]
    if name in ("wall_and_cell_faces", "dense_blob", "far_from_origin"):
        assert to_r2 == 0


def test_each_pass_owned_500_compared_points(default):
    """The sum over the clouds of what each pass answered AND test_covariances_match_brute_force compared."""
    own = np.zeros(3, np.int64)
    for name in G.NAMES:
        m, to_r2, to_iso = (int(x) for x in default[name + "/stats"])
        if m >= 5 and name != "line":
            own += [m - to_r2, to_r2 - to_iso, to_iso]
    print("compared points by pass (certified, r = 2, isolated):", own.tolist())
    assert own.min() >= 500


def test_exact_knob_defers_everything_and_gives_the_same_bits(gpu_api, default, monkeypatch):
    monkeypatch.setenv("GFS_GICP_KNN_EXACT", "1")
    reg = gpu_api.RegistrationGICP(max_points=CAP)
    for name in G.NAMES:
        c = G.cloud(name, SEED)
        reg.RegisterPointClouds(c, c)
        pts, cov = reg.preprocessed(0, 0)
        st = reg.knn_stats(0, 0)[0]
        assert int(st[1]) == int(st[0]) == len(pts), (name, st)
        assert np.array_equal(_bits(pts), _bits(default[name + "/pts"])), name
        assert np.array_equal(_bits(cov), _bits(default[name + "/cov"])), (name, int((cov != default[name + "/cov"]).any(axis=(1, 2)).sum()))


@pytest.mark.parametrize("name", [n for n in G.NAMES if not n.startswith("tiny_")] + ["tiny_12"])
def test_a_handle_no_larger_than_the_cloud_gives_the_same_bits(gpu_api, default, name):
    """The same cloud on a handle created for exactly its number of points (the library rounds the capacity up to 1 024).  Nothing may
    depend on spare capacity -- in a sparse cloud every point is deferred by k_knn_cov AND again by the r = 2 pass, so the two
    deferred lists together hold 2 m entries: in one buffer of P slots the second list overwrote unread entries of the first as soon
    as they held more than P together (sparse_uniform: 6 000 entries, P = 3 072; density_gradient: 7 982, P = 6 144), and the
    covariances of those queries came from other points' neighbourhoods.  GFS_GICP_KNN_EXACT=1 (everything deferred) showed it on the
    roomy handle of the other tests first."""
    c = G.cloud(name, SEED)
    reg = gpu_api.RegistrationGICP(max_points=len(c))
    reg.RegisterPointClouds(c, c)
    pts, cov = reg.preprocessed(0, 0)
    st = reg.knn_stats(0, 0)[0]
    assert np.array_equal(st, default[name + "/stats"]), (name, st, default[name + "/stats"])
    assert np.array_equal(_bits(pts), _bits(default[name + "/pts"])), name
    assert np.array_equal(_bits(cov), _bits(default[name + "/cov"])), (name, st, int((cov != default[name + "/cov"]).any(axis=(1, 2)).sum()))
    # ... and against the brute force directly, so that the statement does not rest on the roomy handle being right
    f = G.facts(name, SEED)
    cov = _to_oracle_order(f, pts, cov)
    good = f["good"]
    if good.any():
        assert np.abs(cov - f["ref"]).reshape(len(cov), -1).max(1)[good].max() <= 1e-9 + f["d_or_cov"], name


def _check_linearization(name, d, tag=""):
    """(d) for the results `d` of collect(): H, b, error of one linearisation against reference_linearize on d's own preprocessed clouds."""
    p = G.pair_facts(name, SEED)
    r = _unpack(d, name + "/lin")
    ref = G.reference_linearize(d[name + "/tpts"], d[name + "/tcov"], d[name + "/spts"], d[name + "/scov"], p["init_T"])
    assert ref["nn_ties"] == 0 and ref["at_gate"] == 0
    bar = 100 * max(p["d_or_lin"], 1e-14)
    dist = (G.rel(r["H"], ref["H"]), G.rel(r["b"], ref["b"]), abs(r["error"] - ref["error"]) / abs(ref["error"]))
    print(f"{name}{tag}: inliers {r['num_inliers']} of {r['n_source_ds']}; H {dist[0]:.2e} b {dist[1]:.2e} error {dist[2]:.2e}; "
          f"d_or_lin {p['d_or_lin']:.2e} bar {bar:.1e}")
    assert p["d_or_lin"] <= 1e-12
    assert r["num_inliers"] == ref["num_inliers"], (name, r["num_inliers"], ref["num_inliers"])
    assert r["num_inliers"] >= 0.5 * r["n_source_ds"]
    assert max(dist) <= bar, (name, dist, bar)
    ro = p["oracle1"]
    assert r["num_inliers"] == ro["num_inliers"] and r["iterations"] == ro["iterations"] and r["converged"] == ro["converged"]
    assert r["n_target_ds"] == ro["n_target_ds"] and r["n_source_ds"] == ro["n_source_ds"]
    return dist


@pytest.mark.parametrize("name", LIN_NAMES)
def test_one_linearization_matches_brute_force(default, name):
    _check_linearization(name, default)


@functools.lru_cache(maxsize=None)
def _oracle_full(name):
    from oracle import oracle as O
    c = G.cloud(name, SEED)
    src, init_T, _ = G.moved(c, SEED)
    return O.gicp_align(c, src, init_T)


def _check_full(name, d, tag=""):
    """(e) the criteria of tests/test_gpu_gicp.py, unchanged, and no tie allowance: these clouds have no ties."""
    from test_gpu_gicp import _gicp_same, _rel
    r, ro = _unpack(d, name + "/full"), _oracle_full(name)
    print(f"{name}{tag}: pose {_rel(r['T'], ro['T']):.2e} iterations {r['iterations']}/{ro['iterations']} inliers {r['num_inliers']}/{ro['num_inliers']}")
    assert _gicp_same(r, ro), (name, _rel(r["T"], ro["T"]), r, ro)


@pytest.mark.parametrize("name", G.NAMES)
def test_full_registration_matches_oracle(default, name):
    _check_full(name, default)


def test_one_batch_call_gives_the_bits_of_the_single_calls(gpu_api, default):
    """(f) all pairs, mixed sizes, the tiny ones and an empty source, as ONE gfs_gicp_align_batch_device call."""
    from test_gpu_gicp import _same
    from test_gpu_gms import _Hip
    names = list(G.NAMES) + ["empty"]
    B = len(names)
    c0, c1 = np.zeros((B, CAP, 4), np.float32), np.zeros((B, CAP, 4), np.float32)
    n0, n1 = np.zeros(B, np.int32), np.zeros(B, np.int32)
    T0 = np.stack([np.eye(4)] * B)
    for b, name in enumerate(names):
        c = G.cloud(G.NAMES[0] if name == "empty" else name, SEED)
        src, init_T, _ = G.moved(c, SEED)
        if name == "empty":
            src, init_T = src[:0], np.eye(4)
        c0[b, :len(c)], c1[b, :len(src)], n0[b], n1[b], T0[b] = c, src, len(c), len(src), init_T
    hip = _Hip()
    d = [hip.to_device(x) for x in (c0, n0, c1, n1)]
    reg = gpu_api.RegistrationGICP(max_points=CAP, max_batch=B)
    got = reg.align_batch_device(d[0], d[1], d[2], d[3], B, CAP, init_T=T0)
    for b, name in enumerate(names):
        assert _same(got[b], _unpack(default, name + "/full")), name
        if name != "empty":
            for which, key in ((0, "t"), (1, "s")):
                pts, cov = reg.preprocessed(b, which)
                assert np.array_equal(_bits(pts), _bits(default[name + "/" + key + "pts"])), (name, which)
                assert np.array_equal(_bits(cov), _bits(default[name + "/" + key + "cov"])), (name, which)
    hip.free()


def _same_results(a, b, keys):
    return all(np.array_equal(_bits(a[k]) if a[k].dtype == np.float64 else a[k], _bits(b[k]) if b[k].dtype == np.float64 else b[k]) for k in keys)


def test_per_handle_knobs_on_these_clouds(gpu_api, default, monkeypatch):
    """(f) GFS_GICP_COOP=0 promises the default's bits (test_cooperative_lm_kernel_gives_the_bits_of_the_launch_per_step_rounds): the
    same here, preprocessing included."""
    for knob, val in (("GFS_GICP_COOP", "0"),):
        monkeypatch.setenv(knob, val)
        got = collect(gpu_api)
        monkeypatch.delenv(knob)
        diff = [k for k in default if not _same_results(got, default, [k])]
        assert not diff, (knob, diff[:8])
