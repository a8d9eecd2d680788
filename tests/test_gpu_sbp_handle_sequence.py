"""One gfs_sbp handle with all three reserves made, its six kinds of call in a row (MI355X): the entry points of sbp.hip,
local_points.hip, fuse.hip and triangulate.hip share the handle's stream and lock, and gfs_search_local_points rewrites part of the
input block of gfs_search_by_projection*.  The sizes change from call to call (63, 64 and 65 map points and key-points, batches of 1
and 3), so the strides of the per-frame arrays (counts rounded up to 64: 64 or 128) and every offset behind them differ between
consecutive calls.  Every call's outputs are compared bit for bit with the CPU oracle or restatement its own test file uses."""
import numpy as np
import pytest

from geoflowslam_amd import synth

import bow_search_support as BS
import fuse_support as FS
import local_points_support as LPS
import sim3_search_support as SS
import triangulate_support as TS
from test_gpu_sbp_of import assert_of_equal, harness, of_case  # noqa: F401  (harness: the fixture that builds the adaptor's entry)

pytestmark = pytest.mark.gpu

_LAST = ("last_xw", "last_desc", "last_octave", "last_angle", "last_mp_has_obs")
_MAP = ("mp_proj", "mp_level", "mp_view_cos", "mp_desc", "mp_has_obs")
_CUR = ("cur_kps_un", "cur_u_right", "cur_desc", "cur_has_mp_obs")


def _cut(p, keys, n_points, n_cur):
    """the problem with exactly n_points map points and n_cur key-points (the first ones of the scene)"""
    assert len(p[keys[0]]) >= n_points and len(p["cur_kps_un"]) >= n_cur
    q = dict(p)
    for k in keys:
        q[k] = np.ascontiguousarray(p[k][:n_points])
    for k in _CUR:
        q[k] = np.ascontiguousarray(p[k][:n_cur])
    return q


def test_six_calls_with_changing_strides_on_one_handle(gpu_api, oracle):
    m = gpu_api.ProjectionMatcher(max_last=128, max_cur=128, max_batch=3)
    m.reserve_local(128)
    m.reserve_fuse(2, 128, 3)
    m.reserve_triangulation(2, 1 << 16)
    # 1. map search, batch of 3: strides 128 / 128
    frames = [_cut(synth.sbp_map_frame(70 + i, n_points=100, n_extra_cur=40, th=3.0), _MAP, n, c) for i, (n, c) in enumerate([(63, 65), (64, 63), (65, 64)])]
    for q, (cm, nm) in zip(frames, m.SearchByProjectionMap(frames)):
        cmo, nmo = oracle.search_by_projection_map(q)
        assert nm == nmo and np.array_equal(cm, cmo), "call 1"
    # 2. local points, one frame: strides 64 / 64 / 64 (headers and key-point arrays of the block above are rewritten)
    prob, want = LPS.frame(64, 63)
    LPS.assert_equal(m.search_local_points(prob), want, "call 2")
    # 3. fuse: two lists of 63 and 65 points in three key frames of 65, 64 and 63 key-points
    a, b = FS.problem(63, 65, n_keyframes=2)[0], FS.problem(65, 64, n_keyframes=1)[0]
    kfs = [dict(a["keyframes"][0], list=0), dict(b["keyframes"][0], list=1), _cut_kf(a["keyframes"][1], 63)]
    fuse = dict(lists=[a["lists"][0], b["lists"][0]], keyframes=kfs)
    FS.assert_equal(m.fuse_search(fuse["lists"], fuse["keyframes"]), FS.restate(fuse), "call 3")
    # 4. new map points: a key frame of 65 key-points against two neighbours of 63
    tri, tri_want = TS.problem(65, 63, n_neighbours=2)
    TS.assert_equal(m.create_new_map_points(tri), tri_want, "call 4")
    # 5. frame to frame, one pair: strides 128 / 64
    pair = _cut(synth.sbp_pair(80, n_points=65, n_extra_cur=40), _LAST, 65, 64)
    cm, nm = m.SearchByProjection(pair)
    cmo, nmo = oracle.search_by_projection(pair)
    assert nm == nmo and np.array_equal(cm, cmo), "call 5"
    # 6. local points again, batch of 3: strides 128 / 128 / 128
    cases = [(65, 65), (63, 64), (64, 63)]
    for c, got in zip(cases, m.search_local_points([LPS.frame(*c)[0] for c in cases])):
        LPS.assert_equal(got, LPS.frame(*c)[1], ("call 6", c))
    m.close()


def test_every_workspace_of_one_handle_with_changing_strides(gpu_api, oracle, harness):
    """The same handle with all FIVE reserves (local, fuse, tri, sim3, bow): the six calls above with the two Sim3 search forms,
    SearchByBoW and the optical-flow search between them, at 63 / 64 / 65 map points and key-points.  gfs_sim3_search and
    gfs_search_by_bow stage into blocks of their own on the handle's stream; the optical-flow search (SearchByProjectionWithOF, the
    adaptor around the KLT and F kernels) runs on handles and streams of its own between two calls of this one.  Every call against
    the restatement of its own test file, bit for bit."""
    m = gpu_api.ProjectionMatcher(max_last=128, max_cur=128, max_batch=3)
    m.reserve_local(128)
    m.reserve_fuse(2, 128, 3)
    m.reserve_triangulation(2, 1 << 16)
    m.reserve_sim3_search(2, 128, 3)
    m.reserve_bow(2, 4)

    def sim3(mode, n_mp, n_kp, what):
        prob, want, _ = SS.problem(mode, n_mp, n_kp)
        SS.assert_equal(m.sim3_search(prob["lists"], prob["problems"]), want, what)

    def bow(seed, n1, n2, what):
        prob, want = BS.problem(seed, n1, n2, n_kf2=2, n_nodes=3)
        BS.assert_equal(m.search_by_bow(prob), want, what)

    # 1. map search, batch of 3
    frames = [_cut(synth.sbp_map_frame(70 + i, n_points=100, n_extra_cur=40, th=3.0), _MAP, n, c) for i, (n, c) in enumerate([(63, 65), (64, 63), (65, 64)])]
    for q, (cm, nm) in zip(frames, m.SearchByProjectionMap(frames)):
        cmo, nmo = oracle.search_by_projection_map(q)
        assert nm == nmo and np.array_equal(cm, cmo), "call 1"
    sim3(SS.FUSE, 63, 65, "Sim3 Fuse after call 1")
    # 2. local points, one frame
    prob, want = LPS.frame(64, 63)
    LPS.assert_equal(m.search_local_points(prob), want, "call 2")
    bow(41, 65, 63, "SearchByBoW after call 2")
    # 3. fuse
    a, b = FS.problem(63, 65, n_keyframes=2)[0], FS.problem(65, 64, n_keyframes=1)[0]
    kfs = [dict(a["keyframes"][0], list=0), dict(b["keyframes"][0], list=1), _cut_kf(a["keyframes"][1], 63)]
    fuse = dict(lists=[a["lists"][0], b["lists"][0]], keyframes=kfs)
    FS.assert_equal(m.fuse_search(fuse["lists"], fuse["keyframes"]), FS.restate(fuse), "call 3")
    sim3(SS.SBP, 65, 64, "Sim3 SearchByProjection after call 3")
    # 4. new map points
    tri, tri_want = TS.problem(65, 63, n_neighbours=2)
    TS.assert_equal(m.create_new_map_points(tri), tri_want, "call 4")
    assert_of_equal(*of_case(harness, gpu_api, oracle, 3, n_last=65))  # the optical-flow search: 65 key points of the last frame
    sim3(SS.SBP_KFS, 64, 63, "Sim3 SearchByProjection (key frames) after call 4")
    # 5. frame to frame
    pair = _cut(synth.sbp_pair(80, n_points=65, n_extra_cur=40), _LAST, 65, 64)
    cm, nm = m.SearchByProjection(pair)
    cmo, nmo = oracle.search_by_projection(pair)
    assert nm == nmo and np.array_equal(cm, cmo), "call 5"
    bow(42, 63, 64, "SearchByBoW after call 5")
    # 6. local points again, batch of 3
    cases = [(65, 65), (63, 64), (64, 63)]
    for c, got in zip(cases, m.search_local_points([LPS.frame(*c)[0] for c in cases])):
        LPS.assert_equal(got, LPS.frame(*c)[1], ("call 6", c))
    sim3(SS.FUSE, 64, 64, "Sim3 Fuse after call 6")
    m.close()


def _cut_kf(kf, n_kp):
    """a fuse key frame with its first n_kp key-points"""
    assert len(kf["kps_un"]) >= n_kp
    return dict(kf, list=0, kps_un=np.ascontiguousarray(kf["kps_un"][:n_kp]), u_right=np.ascontiguousarray(kf["u_right"][:n_kp]),
                desc=np.ascontiguousarray(kf["desc"][:n_kp]))
