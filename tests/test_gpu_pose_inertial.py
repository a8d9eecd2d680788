"""gfs_pose_inertial_optimize on the device against the sequential restatement (tests/host/pose_inertial_restatement.cpp), byte for
byte: the estimates of both ends, the outlier flags, n_good, n_inliers, rounds_run, avg_reproj and every double of H."""
import ctypes as C
import threading

import numpy as np
import pytest

import pose_inertial_support as S
from geoflowslam_amd import api, synth

pytestmark = pytest.mark.gpu

KF, FR = S.KF, S.FR
CHUNK = 256      # kChunk of csrc/pose_inertial.hip: edges per pass of an ordered sum
IN_REGISTERS = 512  # a thread keeps its first two edges in registers; edges beyond go through global memory


@pytest.fixture(scope="module")
def opt():
    o = api.PoseInertialOptimizer(max_obs=640, max_batch=16)
    yield o
    o.close()


@pytest.fixture(scope="module")
def sweep_alone(opt):
    """Every sweep problem alone on the device, checked against the restatement once and shared."""
    out = {}
    for mode in (KF, FR):
        for k, p in enumerate(S.sweep(mode)):
            r = opt.optimize(p)
            S.assert_same(r, p, ("sweep", mode, k))
            out[(mode, k)] = r
    return out


@pytest.mark.parametrize("name", sorted(S.hand_built()))
def test_hand_built(opt, name):
    p = S.hand_built()[name]
    ref = S.assert_same(opt.optimize(p), p, name)
    if name.endswith("_behind"):
        assert ref["outlier"][5] == 1
    if name.endswith("_close_far"):
        assert ref["outlier"][3] == 0 and ref["outlier"][4] == 1
    if "_edges_" in name:
        assert ref["rounds_run"] == (1 if name in ("kf_edges_6", "fr_edges_5") else 4)
    if name.endswith("_no_obs"):
        assert ref["rounds_run"] == 1 and ref["n_good"] == 0 and np.isnan(ref["avg_reproj"])


SIZES = [0, 1, 6, 7, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1]


@pytest.mark.parametrize("mode", [KF, FR])
@pytest.mark.parametrize("kind", ["mono", "stereo", "mixed"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_chunks(opt, mode, kind, n):
    p = S.variant(synth.pose_inertial_problem(1000 + 7 * n + mode, mode, n_obs=n, stereo_share=0.6), kind)
    S.assert_same(opt.optimize(p), p, (mode, kind, n))


@pytest.mark.parametrize("mode", [KF, FR])
@pytest.mark.parametrize("n", [IN_REGISTERS - 1, IN_REGISTERS, IN_REGISTERS + 1, 600])
def test_sizes_beyond_the_register_edges(opt, mode, n):
    p = synth.pose_inertial_problem(2000 + n + mode, mode, n_obs=n, stereo_share=0.6)
    S.assert_same(opt.optimize(p), p, (mode, n))


@pytest.mark.parametrize("mode", [KF, FR])
@pytest.mark.parametrize("n_rounds", [1, 2, 3, 4])
def test_round_counts(opt, mode, n_rounds):
    p = synth.pose_inertial_problem(3000 + mode, mode, n_obs=220, n_rounds=n_rounds)
    ref = S.assert_same(opt.optimize(p), p, (mode, n_rounds))
    assert ref["rounds_run"] == n_rounds


def test_sweep_alone(sweep_alone):
    assert len(sweep_alone) == 80
    # the sweep does what it is for: outliers are found, the pose comes home
    for (mode, k), r in sweep_alone.items():
        p = S.sweep(mode)[k]
        assert r["n_inliers"] > 0.5 * p["n_obs"]
        assert np.abs(r["cur"]["twb"] - p["truth"]["twb"]).max() < np.abs(p["cur"]["twb"] - p["truth"]["twb"]).max() + 0.01


@pytest.mark.parametrize("B", [3, 16])
def test_batches_give_the_bytes_of_the_problems_alone(opt, sweep_alone, B):
    keys = sorted(sweep_alone)
    order = [keys[(37 * i) % len(keys)] for i in range(len(keys))]  # modes and sizes mixed within a batch
    for at in range(0, len(order), B):
        group = order[at:at + B]
        res = opt.optimize([S.sweep(m)[k] for m, k in group])
        for key, r in zip(group, res):
            assert S.result_bytes(r) == S.result_bytes(sweep_alone[key]), (B, key)


def test_chain_of_five_frames(opt):
    """The output of one call is a valid input of the next: each frame's prior is the previous solution's H, marginalised in numpy."""
    p = synth.pose_inertial_problem(300, FR, n_obs=200)
    for k in range(5):
        r = opt.optimize(p)
        S.assert_same(r, p, ("chain", k))
        assert np.linalg.eigvalsh(p["prior_H"]).min() > 0 and r["n_inliers"] > 100
        assert np.abs(r["cur"]["twb"] - p["truth"]["twb"]).max() < 0.02
        p = S.next_frame_problem(p, r, 301 + k)


def _expect(code, call):
    with pytest.raises(api.GfsError) as e:
        call()
    assert e.value.code == code and api.lib().gfs_last_error()


def test_refusals_leave_the_handle_usable(sweep_alone):
    GFS_ERR_INVALID_ARG, GFS_ERR_CAPACITY = -1, -4
    small = api.PoseInertialOptimizer(max_obs=400, max_batch=2)
    good = S.sweep(KF)[0]
    assert good["n_obs"] <= 400
    want = S.result_bytes(sweep_alone[(KF, 0)])

    def still_good():
        assert S.result_bytes(small.optimize(good)) == want

    still_good()
    _expect(GFS_ERR_CAPACITY, lambda: small.optimize([good, good, good]))
    still_good()
    _expect(GFS_ERR_CAPACITY, lambda: small.optimize([good, synth.pose_inertial_problem(5, FR, n_obs=401)]))
    still_good()
    for bad in (dict(good, n_rounds=0), dict(good, n_rounds=5), dict(good, mode=2), dict(good, mode=-1)):
        _expect(GFS_ERR_INVALID_ARG, lambda: small.optimize([good, bad]))
        still_good()
    for name in ("xw", "obs", "inv_sigma2", "stereo", "close", "outlier"):
        P, Sol, keep, n = api.pose_inertial_structs(good)
        if name == "outlier":
            Sol.outlier = None
        else:
            setattr(P, name, None)
        rc = api.lib().gfs_pose_inertial_optimize(small.h, C.byref(P), 1, C.byref(Sol))
        assert rc == GFS_ERR_INVALID_ARG, (name, rc)
        still_good()
    P, Sol, keep, n = api.pose_inertial_structs(good)
    P.n_obs = -1
    assert api.lib().gfs_pose_inertial_optimize(small.h, C.byref(P), 1, C.byref(Sol)) == GFS_ERR_INVALID_ARG
    still_good()
    small.close()


def test_two_handles_on_two_threads(sweep_alone):
    """Two handles, each with its own stream, driven from two threads at once: the bytes they give alone."""
    handles = [api.PoseInertialOptimizer(max_obs=640, max_batch=4) for _ in range(2)]
    jobs = [[(KF, k) for k in range(0, 12)], [(FR, k) for k in range(0, 12)]]
    got, errors = [dict(), dict()], []

    def work(i):
        try:
            for at in range(0, len(jobs[i]), 3):
                group = jobs[i][at:at + 3]
                for key, r in zip(group, handles[i].optimize([S.sweep(m)[k] for m, k in group])):
                    got[i][key] = S.result_bytes(r)
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for h in handles:
        h.close()
    assert not errors, errors
    for i in range(2):
        assert len(got[i]) == 12
        for key, b in got[i].items():
            assert b == S.result_bytes(sweep_alone[key]), key
