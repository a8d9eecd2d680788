"""gfs_create_new_map_points (k_tri_candidates + k_tri_resolve, geoflowslam_amd/csrc/triangulate.hip) on the MI355X against the
sequential CPU restatement (tests/host/triangulate_restatement.cpp): bit equality of match12, exit, x3d (as bits), point_stereo and
the counts, no tolerance."""
import numpy as np
import pytest

import triangulate_support as TS
from geoflowslam_amd import synth

pytestmark = pytest.mark.gpu

CAP, INV = -4, -1


@pytest.fixture(scope="module")
def matcher(gpu_api):
    m = gpu_api.ProjectionMatcher(max_last=64, max_cur=1024, max_batch=3)
    m.reserve_triangulation(5, 1 << 20)
    yield m
    m.close()


# key-points of the current key frame and of the neighbours: empty, one, around a wave, several tiles
SIZES = [(0, 64), (64, 0), (1, 1), (63, 65), (65, 63), (64, 64), (257, 1000), (1000, 257), (1000, 1000)]


@pytest.mark.parametrize("n_kp,n_kp_nb", SIZES)
def test_every_wave_and_tile_edge(matcher, n_kp, n_kp_nb):
    prob, want = TS.problem(n_kp, n_kp_nb)
    got = matcher.create_new_map_points(prob)
    TS.assert_equal(got, want, (n_kp, n_kp_nb))
    assert all(len(o["exit"]) == n_kp for o in got)
    if min(n_kp, n_kp_nb) >= 257:
        assert sum(o["n_created"] for o in got) > 0 and sum((np.bincount(o["exit"], minlength=12) > 0).sum() for o in got) >= 8


@pytest.mark.parametrize("n", [1, 64, 65, 300])
def test_a_single_node_holding_everything(matcher, n):
    """Node lists of 1, 64, 65 key-points on both sides (one tile, one more) and one node of 300 x 300 (chunks on both sides; an idx1
    sees idx2 taken in other chunks)."""
    prob, want = TS.problem(n, n, n_nodes=1)
    assert len(prob["cur"]["node_id"]) == 1 and all(len(nb["node_id"]) == 1 for nb in prob["neighbours"])
    TS.assert_equal(matcher.create_new_map_points(prob), want, ("single node", n))
    if n == 300:
        assert want[0]["n_matches"] > 64 and want[1]["n_matches"] > 0


@pytest.mark.parametrize("n_neighbours", [1, 2, 5])
def test_neighbours_in_order(matcher, n_neighbours):
    prob, want = TS.problem(400, 380, n_neighbours=n_neighbours, n_nodes=20)
    got = matcher.create_new_map_points(prob)
    TS.assert_equal(got, want, ("neighbours", n_neighbours))
    created = np.zeros(400, bool)
    for o in got:  # an idx1 created at one neighbour is matched at no later one
        assert not (created & (o["match12"] >= 0)).any()
        created |= o["exit"] == TS.CREATED
    assert created.any()


def test_three_problems_of_different_sizes_in_one_call(matcher):
    probs = [TS.problem(257, 1000)[0], TS.problem(64, 64, n_nodes=1)[0], TS.problem(400, 380, n_neighbours=5, n_nodes=20)[0]]
    got = matcher.create_new_map_points(probs)
    for b, p in enumerate(probs):
        TS.assert_equal(got[b], TS.restate(p), ("batch", b))
        TS.assert_equal(matcher.create_new_map_points(p), got[b], ("single call", b))


@pytest.mark.parametrize("flags", [dict(check_orientation=True), dict(check_orientation=False), dict(coarse=True), dict(only_stereo=True),
                                   dict(check_orientation=True, inertial=True, coarse=True)], ids=lambda f: "+".join(sorted(k for k in f if f[k])) or "plain")
def test_flags(matcher, flags):
    prob, want = TS.problem(500, 520, n_neighbours=3, n_nodes=25, **flags)
    got = matcher.create_new_map_points(prob)
    TS.assert_equal(got, want, flags)
    assert sum(o["n_created"] for o in got) > 0
    if flags.get("check_orientation"):
        off = TS.restate(dict(prob, check_orientation=False))
        assert any(a["n_matches"] < b["n_matches"] for a, b in zip(want, off))  # the histogram took matches away


def test_constructed_cases(matcher):
    for label, (prob, check) in TS.constructed().items():
        got = matcher.create_new_map_points(prob)
        assert check(got), (label, [(o["match12"].tolist(), o["exit"].tolist()) for o in got])
        TS.assert_equal(got, TS.restate(prob), label)


def _refused(gpu_api, m, probs, code):
    with pytest.raises(gpu_api.GfsError) as e:
        m.create_new_map_points(probs)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals_leave_the_handle_usable(gpu_api):
    """One above each reserve -> GFS_ERR_CAPACITY; each invalid argument -> GFS_ERR_INVALID_ARG.  Nothing is truncated, and after
    every refusal the previous call gives identical bytes.  A handle that never reserved refuses and is otherwise unchanged."""
    hdr = open(TS.os.path.join(TS.ROOT, "include", "gfs_abi.h")).read()
    assert "GFS_ERR_INVALID_ARG = -1," in hdr and "GFS_ERR_CAPACITY = -4," in hdr
    prob, want = TS.problem(400, 380, n_neighbours=2, n_nodes=20)
    pairs = gpu_api.tri_candidate_pairs(prob)
    m = gpu_api.ProjectionMatcher(max_last=64, max_cur=400, max_batch=2)
    before = gpu_api.ProjectionMatcher(max_last=64, max_cur=400, max_batch=2)
    m.reserve_triangulation(2, pairs)
    base = m.create_new_map_points([prob, prob])  # at every reserve exactly
    TS.assert_equal(base[0], want, "at the reserve")
    TS.assert_equal(base[1], want, "at the reserve")

    def again(what):
        got = m.create_new_map_points([prob, prob])
        for g in got:
            TS.assert_equal(g, base[0], what)

    _refused(gpu_api, m, [prob, prob, prob], CAP)                                          # three problems, max_batch = 2
    again("batch")
    _refused(gpu_api, m, dict(prob, neighbours=prob["neighbours"] + prob["neighbours"][:1]), CAP)  # three neighbours
    again("neighbours")
    wide = synth.triangulation_problem(5, n_kp=401, n_neighbours=1, n_nodes=20)
    _refused(gpu_api, m, wide, CAP)                                                        # 401 key-points, max_cur = 400
    _refused(gpu_api, m, dict(prob, neighbours=[prob["neighbours"][0], wide["neighbours"][0]]), CAP)
    again("key-points")
    m.reserve_triangulation(2, pairs - 1)
    _refused(gpu_api, m, prob, CAP)                                                        # one candidate pair above the reserve
    m.reserve_triangulation(2, pairs)
    again("candidate pairs")

    def cur_with(**kw):
        return dict(prob, cur=dict(prob["cur"], **kw))

    def nb_with(**kw):
        return dict(prob, neighbours=[prob["neighbours"][0], dict(prob["neighbours"][1], **kw)])

    _refused(gpu_api, m, cur_with(n_levels=17, scale_factors=np.ones(17, np.float32), level_sigma2=np.ones(17, np.float32)), INV)
    _refused(gpu_api, m, nb_with(n_levels=0), INV)
    again("levels")
    kps = prob["cur"]["kps_un"].copy()
    kps["octave"][7] = 8
    _refused(gpu_api, m, cur_with(kps_un=kps), INV)
    kps["octave"][7] = -1
    _refused(gpu_api, m, cur_with(kps_un=kps), INV)
    again("octave")
    feat = prob["neighbours"][1]["feat_idx"].copy()
    feat[3] = 380
    _refused(gpu_api, m, nb_with(feat_idx=feat), INV)                                      # a feature index outside [0, n_kp)
    feat[3] = -1
    _refused(gpu_api, m, nb_with(feat_idx=feat), INV)
    feat[3] = feat[4]
    _refused(gpu_api, m, nb_with(feat_idx=feat), INV)                                      # ... listed twice
    again("feature index")
    ids = prob["cur"]["node_id"].copy()
    ids[2] = ids[1]
    _refused(gpu_api, m, cur_with(node_id=ids), INV)                                       # node ids not strictly ascending
    again("node ids")
    for field in ("kps", "depth", "has_mp", "node_start", "feat_idx"):
        PP, RP, keep = gpu_api.tri_structs([prob])
        setattr(PP[0].neighbours[1].kf, field, None)
        assert gpu_api.lib().gfs_create_new_map_points(m.h, PP, 1, RP) == INV, field
    PP, RP, keep = gpu_api.tri_structs([prob])
    RP[0][1].x3d = None
    assert gpu_api.lib().gfs_create_new_map_points(m.h, PP, 1, RP) == INV
    again("NULL arrays")
    PP, RP, keep = gpu_api.tri_structs([prob])
    assert gpu_api.lib().gfs_create_new_map_points(before.h, PP, 1, RP) == CAP              # never reserved
    p = synth.sbp_pair(3, n_points=60, n_extra_cur=40)
    a, b = before.SearchByProjection(p), m.SearchByProjection(p)
    assert a[1] == b[1] and TS.same_bits(a[0], b[0])
    m.close()
    before.close()
