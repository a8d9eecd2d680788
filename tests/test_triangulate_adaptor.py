"""LocalMapping::CreateNewMapPoints as adaptor code (geoflowslam_amd/host/gfs_adaptors.hpp: gfs_host::CreateNewMapPoints,
tri_solve_host, MapPointCreator) over plain-struct KeyFrame / MapPoint / Atlas classes (tests/host/triangulate_adaptor_test.cpp).
The CPU tests run the adaptor with its host solve and compare the end state (the created points in creation order, their
observations, every key frame's map-point slots, the recent list) with a literal sequential loop that runs the restatement
neighbour by neighbour against the live state; the GPU test runs the same through MapPointCreator.  Also: the adaptor's host solve
against the restatement, array by array."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import triangulate_support as TS
from geoflowslam_amd import api as A
from geoflowslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(ROOT, "tests", "host", "_triangulate_adaptor_test.so")


@pytest.fixture(scope="module")
def harness(api):
    src = os.path.join(ROOT, "tests", "host", "triangulate_adaptor_test.cpp")
    deps = [src, os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp"), os.path.join(ROOT, "include", "gfs_abi.h"),
            os.path.join(ROOT, "geoflowslam_amd", "csrc", "triangulate_rule.hpp")]
    if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(d) for d in deps):
        libdir = os.path.join(ROOT, "geoflowslam_amd")
        tmp = _SO + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", tmp, src, "-L" + libdir,
                        "-lgfs_hip", "-ldl", "-lpthread", "-Wl,-rpath," + libdir], check=True)
        os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    L.tri_adaptor_test.argtypes = [C.c_char_p, C.POINTER(A.TriProblem), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.tri_host_solve.argtypes = [C.POINTER(A.TriProblem), C.c_int, C.POINTER(C.POINTER(A.TriResult))]
    TS.restatement()  # (builds the restatement the harness opens)
    return L


def _scene(seed, n_neighbours=4, **kw):
    return synth.triangulation_problem(50 + seed, n_kp=260, n_kp_neighbour=240, n_neighbours=n_neighbours, n_nodes=14, **kw)


def _run(L, prob, short_at=-1, stop_at=0, gpu=False, optical_flow=False):
    PP, RP, keep = A.tri_structs([prob])
    out = np.full(7, -9, np.int32)
    rc = L.tri_adaptor_test(TS._SO.encode(), PP, short_at, stop_at, int(gpu), int(optical_flow), out.ctypes.data)
    assert rc == 0, rc
    return dict(zip(("created", "created_sequential", "mismatches", "checks", "checks_sequential", "well_formed", "refused"), out.tolist()))


def _check(r, prob, upto=None, skip=()):
    """The adaptor's end state is the sequential loop's, and its count is the restatement's on the neighbours that were processed."""
    assert r["mismatches"] == 0 and r["created"] == r["created_sequential"] and r["checks"] == r["checks_sequential"], r
    assert r["well_formed"] == r["created"] and r["refused"] == 1, r
    nbs = [nb for i, nb in enumerate(prob["neighbours"]) if i not in skip]
    n = len(prob["neighbours"]) if upto is None else upto
    n_used = len([i for i in range(n) if i not in skip])
    want = TS.restate(dict(prob, neighbours=nbs))
    assert r["created"] == sum(o["n_created"] for o in want[:n_used]), (r, [o["n_created"] for o in want])
    return want


@pytest.mark.parametrize("seed", range(3))
def test_adaptor_end_state_equals_the_sequential_loop(harness, seed):
    prob = _scene(seed, far_points=seed == 1, inertial=seed == 2)
    r = _run(harness, prob, optical_flow=seed == 0)
    want = _check(r, prob)
    assert r["created"] > 20 and r["checks"] == 3 and all(o["n_created"] > 0 for o in want)


@pytest.mark.parametrize("stop_at,processed", [(1, 1), (3, 3)])
def test_stop_by_check_new_key_frames(harness, stop_at, processed):
    """check_new_key_frames says stop before neighbour 1 (after neighbour 0) and before neighbour 3 (after neighbour 2): the prefix
    that was replayed is exactly what the sequential loop had done by then."""
    prob = _scene(7, n_neighbours=5)
    r = _run(harness, prob, stop_at=stop_at)
    _check(r, prob, upto=processed)
    full = _run(harness, prob)
    assert r["checks"] == stop_at and 0 < r["created"] < full["created"]


def test_short_baseline_neighbour_in_the_middle(harness):
    """Neighbour 2 of 5 fails `baseline < pKF2->mb`: it is not uploaded, the others keep their order, and a stop is still counted per
    entry of the original list."""
    prob = _scene(9, n_neighbours=5)
    r = _run(harness, prob, short_at=2)
    _check(r, prob, skip=(2,))
    assert r["checks"] == 4
    s = _run(harness, prob, short_at=2, stop_at=3)  # stop before list entry 3: entries 0 and 1 were replayed, 2 was skipped
    _check(s, prob, upto=3, skip=(2,))
    assert s["created"] < r["created"]


@pytest.mark.parametrize("seed", range(4))
def test_host_solve_equals_restatement(harness, seed):
    probs = [TS.random_problem(8 * seed + k) for k in range(8)] + [p for p, _ in TS.constructed().values()]
    PP, RP, keep = A.tri_structs(probs)
    assert harness.tri_host_solve(PP, len(probs), RP) == 0
    got = A.tri_results(PP, RP, keep, len(probs))
    for g, p in zip(got, probs):
        TS.assert_equal(g, TS.restate(p), seed)


@pytest.mark.gpu
def test_adaptor_on_the_gpu(harness, gpu_api):
    prob = _scene(3, n_neighbours=5)
    r = _run(harness, prob, short_at=1, gpu=True)
    _check(r, prob, skip=(1,))
    assert r["created"] > 20
    s = _run(harness, prob, stop_at=2, gpu=True)
    _check(s, prob, upto=2)
