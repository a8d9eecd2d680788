"""MapPoint::ComputeDistinctiveDescriptors / UpdateNormalAndDepth as adaptor code (geoflowslam_amd/host/gfs_adaptors.hpp:
gfs_host::UpdateMapPoints, ProcessNewKeyFrame, the batched tail of SearchInNeighborsFuse, map_points_update_host, MapPointUpdater)
over plain-struct KeyFrame / MapPoint classes (tests/host/map_point_adaptor_test.cpp).  The CPU tests plug the sequential restatement
or the product's host rule in as the device call and compare the end state of every point (descriptor, normal, both distances,
what was written at all) with the reference's per-point loops; the GPU test runs the same through MapPointUpdater.  Also: the
host rule against the restatement on whole problems, and the same harness as a program of its own under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import pytest

import map_point_support as MS
from geoflowslam_amd import api as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "tests", "host", "map_point_adaptor_test.cpp")
_SO = os.path.join(ROOT, "tests", "host", "_map_point_adaptor_test.so")
_EXE = os.path.join(ROOT, "tests", "host", "_map_point_adaptor_asan")
_DEPS = [_SRC, os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp"), os.path.join(ROOT, "include", "gfs_abi.h"),
         os.path.join(ROOT, "geoflowslam_amd", "csrc", "map_point_rule.hpp"), os.path.join(ROOT, "geoflowslam_amd", "csrc", "fuse_rule.hpp")]


def _stale(out):
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in _DEPS)


@pytest.fixture(scope="module")
def harness(api):
    if _stale(_SO):
        libdir = os.path.join(ROOT, "geoflowslam_amd")
        tmp = _SO + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-o", tmp, _SRC, "-L" + libdir,
                        "-lgfs_hip", "-ldl", "-lpthread", "-Wl,-rpath," + libdir], check=True)
        os.replace(tmp, _SO)
    L = C.CDLL(_SO)
    L.map_point_adaptor_test.argtypes = [C.c_char_p, C.c_int, C.c_uint, C.POINTER(C.c_int), C.c_char_p, C.c_int]
    L.map_point_host_rule.argtypes = [C.POINTER(A.MapPointsProblem), C.POINTER(A.MapPointsResult)]
    return L


def _run(L, mode, seed):
    MS.restatement()
    msg, n = C.create_string_buffer(512), C.c_int(0)
    rc = L.map_point_adaptor_test(MS._SO.encode(), mode, seed, C.byref(n), msg, 512)
    assert rc == 0, (rc, msg.value.decode())
    assert n.value >= 40


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_adaptor_over_the_restatement(harness, seed):
    """UpdateMapPoints in both modes, ProcessNewKeyFrame and the SearchInNeighborsFuse tail end in the state of the per-point loops:
    a bad and a null key frame among the observations, an index beyond the descriptor rows, bad and null points, a point listed
    twice, a reference key frame that does not observe the point; a two-camera observation throws before anything is written."""
    _run(harness, 0, seed)


@pytest.mark.parametrize("seed", [1, 2])
def test_adaptor_over_the_host_rule(harness, seed):
    _run(harness, 1, seed)


@pytest.mark.parametrize("normals_only", [False, True])
def test_host_rule_gives_the_restatement_bits(harness, normals_only):
    probs = [MS.random_problem(seed) for seed in range(8)] + [MS.constructed()[0], MS.mixed()[0]]
    for i, prob in enumerate(probs):
        P, R, keep = A.map_points_structs(prob, normals_only)
        assert harness.map_point_host_rule(C.byref(P), C.byref(R)) == 0
        MS.assert_equal(A.map_points_results(P, keep), MS.restate(prob, normals_only), ("problem", i))


def test_harness_alone_under_sanitizers():
    """The same harness with its own main (the host rule, the adaptor over the mocks, the host call's refusals), built with
    -fsanitize=address,undefined and run as a program: it is never loaded into python."""
    if _stale(_EXE):
        tmp = _EXE + f".{os.getpid()}.tmp"
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-fno-omit-frame-pointer", "-DMP_STANDALONE", "-Wall", "-o", tmp, _SRC, "-ldl", "-lpthread"], check=True)
        os.replace(tmp, _EXE)
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([_EXE], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "map_point_adaptor_test: ok" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-2000:])


@pytest.mark.gpu
def test_adaptor_on_the_gpu(harness, gpu_api):
    """The same end states with MapPointUpdater as the solver (its reserve of 16 points has to grow)."""
    _run(harness, 2, 1)
