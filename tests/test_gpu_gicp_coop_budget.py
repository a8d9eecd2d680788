"""Partial grants of the cooperative GICP workgroup budget (MI355X).  k_gicp_lm_coop takes its workgroups from a process-wide budget
(csrc/gicp.hip CoopBudget); gicp_attempt asks for a workgroup per 256-point chunk of every pair (`want`), accepts anything down to
max(B, want / 2) (`least`) and launches what it got.  A handle that is alone always gets `want`: every workgroup then serves one chunk
and the chunk loop of the kernel runs once.  With part of the budget held by another handle's launch the grant is smaller and

  - a workgroup walks chunks g, g + Gp, ...;                         - the pairs' barriers count (episode + 1) * Gp arrivals;
  - workgroups beyond n_pairs * G or beyond a pair's chunks leave;   - below `least` the call runs the launch-per-step rounds.

The bits are promised to be those of the rounds whatever was granted.  Here the budget is held through the test hooks
(gfs_test_gicp_coop_hold / _release / _in_use, include/gfs_abi_test.h), so every grant is chosen, not raced for, and each case is
compared bit for bit with a handle created under GFS_GICP_COOP=0.  c = chunks of the source cloud after down-sampling, measured from
an un-held call.  (By the CPU oracle's counters the `far` start of test_gpu_gicp.py has no rejected trial on these scenes --
n_error_evals == n_linearize, as for every other start and scene tried while this file was written.  It is run as a long loop.)"""
import numpy as np
import pytest

from geoflowslam_amd import synth

from test_gpu_gicp import _gicp_same, _same

pytestmark = pytest.mark.gpu

SP = 20480  # 80 chunks a pair
FAR = np.eye(4)
FAR[:3, 3] = [0.08, -0.05, 0.06]


class _Rig:
    pass


@pytest.fixture(scope="module")
def rig(gpu_api):
    from test_gpu_gms import _Hip
    R = _Rig()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("GFS_GICP_COOP", "0")
        R.rounds = {20480: gpu_api.RegistrationGICP(max_points=20480), 5120: gpu_api.RegistrationGICP(max_points=5120)}
        R.roundsB = gpu_api.RegistrationGICP(max_points=SP, max_batch=3)
    R.coop = {20480: gpu_api.RegistrationGICP(max_points=20480), 5120: gpu_api.RegistrationGICP(max_points=5120)}
    R.coopB = gpu_api.RegistrationGICP(max_points=SP, max_batch=3)
    assert R.rounds[20480].coop_stats()["budget"] == 0 and R.roundsB.coop_stats()["budget"] == 0
    R.budget = R.coop[20480].coop_stats()["budget"]
    assert R.coop[5120].coop_stats()["budget"] == R.budget == R.coopB.coop_stats()["budget"]
    assert R.budget >= 240, R.budget  # three pairs of 80 chunks: the device entry's cases need it whole
    a, b, t = synth.frame_pair(300, 160, 120, stride=1), synth.frame_pair(301, 160, 120, stride=2), synth.frame_pair(303, 160, 120, stride=2)
    R.pair = {20480: (a["cloud0"], a["cloud1"]), 5120: (b["cloud0"], b["cloud1"])}
    R.tiny = (t["cloud0"], t["cloud1"][:7])
    R.empty = (t["cloud0"], t["cloud1"][:0])
    R.hip = _Hip()
    R.ref = {}  # what the rounds handles gave, once a call
    assert gpu_api.gicp_coop_in_use() == 0
    yield R
    assert gpu_api.gicp_coop_in_use() == 0, "a case left part of the budget held"
    R.hip.free()
    for h in list(R.rounds.values()) + list(R.coop.values()) + [R.roundsB, R.coopB]:
        h.close()


def _bits(a, b):
    return _same(a, b) and a["n_linearize"] == b["n_linearize"] and a["n_error_evals"] == b["n_error_evals"]


def _held(api, R, handle, got, least, call, what):
    """`call(handle)` while all of the budget but `got` workgroups is held -> (results, the handle's counters after the call).  The
    counters are asserted here: one more launch of `got` workgroups when got >= least, none below; never a workgroup that gave up."""
    before = handle.coop_stats()
    hold = R.budget - got
    assert api.gicp_coop_in_use() == 0
    handle.coop_hold(hold)
    try:
        out = call(handle)
        assert api.gicp_coop_in_use() == hold, (what, got)
    finally:
        handle.coop_release(hold)
    assert api.gicp_coop_in_use() == 0
    st = handle.coop_stats()
    print(f"{what}: budget {R.budget} held {hold} got {got} least {least} -> launches {before['launches']} -> {st['launches']}, "
          f"last_wgs {st['last_workgroups']}, failed {st['failed']}")
    assert not st["failed"], (what, got, st)  # a workgroup ran into kCoopSpinLimit: the barrier arithmetic is wrong
    if got >= least:
        assert st["launches"] == before["launches"] + 1 and st["last_workgroups"] == got, (what, got, before, st)
    else:
        assert st["launches"] == before["launches"], (what, got, before, st)
    return out, st


def _chunks(R, size):
    """c of the handle's pair from an un-held call (which is also the rounds handle's reference for it)"""
    key = ("pair", size)
    if key not in R.ref:
        R.ref[key] = R.rounds[size].RegisterPointClouds(*R.pair[size])
    return -(-R.ref[key]["n_source_ds"] // 256)


# (size, want, least, got as a number or in terms of c, the case makes a workgroup serve two chunks)
ONE_PAIR = [(20480, 80, 40, g, loops) for g, loops in ((79, False), ("c", False), ("c-1", True), (41, True), (40, True), (39, False))] + \
           [(5120, 20, 10, g, loops) for g, loops in ((19, False), (18, True), (10, True), (9, False))]


@pytest.mark.parametrize("size,want,least,got,loops", ONE_PAIR, ids=[f"{c[0]}-got{c[3]}" for c in ONE_PAIR])
def test_one_pair_under_a_partial_grant_gives_the_bits_of_the_rounds(gpu_api, rig, size, want, least, got, loops):
    """One pair on a handle of `want` chunks.  20480 points (c = 66 of 80): 79 and c leave workgroups over or give each chunk its
    own, c - 1 makes ONE workgroup serve two chunks, 41 and 40 make c - 41 / c - 40 do so, 39 is below `least` and runs the rounds.
    5120 points (c = 19 of 20): 19 the full grid, 18 one workgroup with two chunks, 10 nine with two and one with one, 9 refused."""
    c = _chunks(rig, size)
    print(f"size {size}: c = {c}")
    assert (40 < c - 1 and c < 79) if size == 20480 else (10 < c <= 19), c  # the scene still puts every case where its name says
    got = {"c": c, "c-1": c - 1}.get(got, got)
    r, st = _held(gpu_api, rig, rig.coop[size], got, least, lambda h: h.RegisterPointClouds(*rig.pair[size]), f"pair {size}")
    if loops:
        assert got >= least and c > st["last_workgroups"], (c, st)
    assert _bits(r, rig.ref[("pair", size)]), (size, got)


@pytest.mark.parametrize("third", ["tiny", "empty"])
@pytest.mark.parametrize("got", [239, 121, 120, 119])
def test_three_pairs_through_the_device_entry_under_a_partial_grant(gpu_api, rig, got, third):
    """B = 3 at stride 20480 (want 240, least 120): the stride-1 pair (66 chunks), the stride-2 pair (19) and a pair whose source has
    7 points (1 chunk) or none (0 chunks: Gp = 1, the scalar steps still run).  239 -> G = 79 and two workgroups beyond 3 G, 121 ->
    G = 40 and one beyond; 120 -> G = 40: pair 0 loops (Gp = 40 < 66), pair 1 has Gp = 19, pair 2 Gp = 1; 119 is refused."""
    R = rig
    pairs = [R.pair[20480], R.pair[5120], getattr(R, third)]
    key = ("dev", third)
    if key not in R.ref:
        def dev(which):
            c = np.zeros((3, SP, 4), np.float32)
            n = np.zeros(3, np.int32)
            for j, p in enumerate(pairs):
                c[j, :len(p[which])] = p[which]
                n[j] = len(p[which])
            return R.hip.to_device(c), R.hip.to_device(n)
        t, s = dev(0), dev(1)
        R.ref[key] = (t, s, R.roundsB.align_batch_device(t[0], t[1], s[0], s[1], 3, SP))
    t, s, want = R.ref[key]
    out, st = _held(gpu_api, R, R.coopB, got, 120, lambda h: h.align_batch_device(t[0], t[1], s[0], s[1], 3, SP), f"device entry ({third})")
    assert [w["n_source_ds"] for w in want][2] == (7 if third == "tiny" else 0) and -(-want[0]["n_source_ds"] // 256) > 40
    for j in range(3):
        assert _bits(out[j], want[j]), (got, third, j)


def test_a_far_start_and_the_streaming_entry_at_half_the_grid(gpu_api, rig):
    """On the 20480 handle at got = 40 (26 workgroups with two chunks): the `far` initial guess of test_gpu_gicp.py (six passes
    instead of three) and RegisterNext (the slots swapped: the source is the other parity)."""
    R = rig
    coop, rounds, (c0, c1) = R.coop[20480], R.rounds[20480], R.pair[20480]
    c = _chunks(R, 20480)
    want = rounds.RegisterPointClouds(c0, c1, FAR)
    r, st = _held(gpu_api, R, coop, 40, 40, lambda h: h.RegisterPointClouds(c0, c1, FAR), "far start")
    assert c > st["last_workgroups"] and _bits(r, want) and want["n_error_evals"] > R.ref[("pair", 20480)]["n_error_evals"]
    # the chain: (c0 <- c1) has just run on both handles; next (c1 <- c0)
    want = rounds.RegisterNext(c0)
    r, st = _held(gpu_api, R, coop, 40, 40, lambda h: h.RegisterNext(c0), "RegisterNext")
    assert -(-want["n_source_ds"] // 256) > st["last_workgroups"] and _bits(r, want)


def test_the_un_held_pair_meets_the_oracle(gpu_api, rig, oracle):
    """... and what all of the above are compared with is right: the un-held stride-2 pair against the CPU oracle."""
    before = rig.coop[5120].coop_stats()["launches"]
    r = rig.coop[5120].RegisterPointClouds(*rig.pair[5120])
    st = rig.coop[5120].coop_stats()
    assert st["launches"] == before + 1 and st["last_workgroups"] == 20 and not st["failed"]
    assert _chunks(rig, 5120) and _bits(r, rig.ref[("pair", 5120)])
    assert _gicp_same(r, oracle.gicp_align(*rig.pair[5120]))
