"""Maps shared by the GlobalBundleAdjustment tests: tests/test_gba_lists.py and tests/test_gba_oracle_inputs.py on the CPU,
tests/test_gpu_gba.py on the GPU.  P = api.gba_panel_rows() is the tile height of the reduced system and Fp = P // 6 the free poses
one tile holds: the shapes follow the constant.  Every map is synth.gba_map (key-frame 0 fixed), so F free poses are F + 1 key-frames.

FULL_SOLVES lists the maps the GPU solves completely against oracle.lba_solve.  A map may be in that list only if the oracle's own
answer does not hang on rounding: test_gba_oracle_inputs.py solves each of them and an edge-shuffled copy with the oracle and asks
for equal iteration counts and poses / points within 1e-7 -- a condition on the INPUTS; a map that misses it is replaced by another
seed, never excused.

STOP_MAP is a map whose Levenberg-Marquardt run rejects trials (lba_stop_support.perturb moves the free key-frames away from the
truth), for the scripted stop flag; the same conditions as lba_stop_support.check_window hold for it (asserted on the CPU)."""
import functools

import numpy as np

import lba_step_support as S
import lba_stop_support as ST
from geoflowslam_amd import synth

STEP = 1.0  # metres between key-frames: a point is seen by ~5 of them, so already 17 key-frames have pairs that share nothing


def gmap(F, n_points, seed, **kw):
    """gba_map with exactly F free poses"""
    fixed = tuple(kw.pop("fixed", ()))
    w = synth.gba_map(seed, F + 1 + len(fixed), n_points, step=kw.pop("step", STEP), fixed=fixed, **kw)
    assert int((w["pose_fixed"] == 0).sum()) == F
    return w


def size_cases(Fp):
    """(name, maker): free-pose counts around one, two and three tiles"""
    return [(f"F{F}", functools.partial(gmap, F, 60 + 8 * F, 500 + F)) for F in (1, 2, Fp, Fp + 1, 2 * Fp, 2 * Fp + 1)]


def structure_cases(Fp):
    F, N, s = Fp + 1, 200, 700
    base = lambda: gmap(F, N, s, fixed=(1,))  # noqa: E731  (two fixed key-frames: some landmarks have several fixed observers)
    return [("isolated-pose", lambda: S.isolated_pose(base())[0]),
            ("fixed-only-landmark", lambda: S.landmark_of_fixed_poses_only(base())[0]),
            ("single-mono-landmark", lambda: S.single_mono_landmark(base())[0]),
            ("all-mono", lambda: gmap(F, N, s + 1, mono_frac=1.0)),
            ("second-camera", lambda: S.with_second_camera_edges(base(), s)),
            ("shuffled-edges", lambda: S.shuffled_edges(base(), s)),
            ("fixed-in-the-middle", lambda: gmap(F, N, s + 2, fixed=(F // 2, F // 2 + 1, F)))]


def step_cases(Fp):
    return size_cases(Fp) + structure_cases(Fp)


def list_cases(Fp):
    """the maps of the structure-list test: 3, Fp + 1, 2 Fp + 1 free poses and the structural edge cases"""
    base = lambda: gmap(Fp + 1, 120, 800, fixed=(1,))  # noqa: E731
    return [("F3", lambda: gmap(3, 40, 801)), (f"F{Fp + 1}", lambda: gmap(Fp + 1, 150, 802)),
            (f"F{2 * Fp + 1}", lambda: gmap(2 * Fp + 1, 250, 803)),
            ("duplicate-edges", lambda: S.with_second_camera_edges(base(), 1)),
            ("shuffled-edges", lambda: S.shuffled_edges(base(), 2)),
            ("isolated-pose", lambda: S.isolated_pose(base())[0]),
            ("fixed-only-landmark", lambda: S.landmark_of_fixed_poses_only(base())[0]),
            ("all-fixed", lambda: S.all_poses_fixed(base())),
            ("zero-points", lambda: zero_points(base()))]


def zero_points(w):
    w = S.take_edges(w, np.zeros(0, np.int64))
    return dict(w, n_points=0, points=np.zeros((0, 3)))


# name -> (free poses as a function of Fp, points, seed, gba_map keywords, iterations, robust)
_FULL = {
    "Fp+1-robust": (lambda Fp: Fp + 1, 300, 900, {}, 10, True),
    "Fp+1-plain": (lambda Fp: Fp + 1, 300, 900, {}, 10, False),
    "2Fp+1-robust": (lambda Fp: 2 * Fp + 1, 400, 901, {}, 10, True),
    "2Fp+1-plain": (lambda Fp: 2 * Fp + 1, 400, 901, {}, 10, False),
    "mono-initial-map": (lambda Fp: 1, 150, 916, dict(mono_frac=1.0, step=0.5), 20, True),
}
FULL_SOLVES = tuple(_FULL)


@functools.lru_cache(maxsize=None)
def full_solve_map(name, Fp):
    """-> the problem dict as the oracle and the library get it (bRobust = false: infinite thresholds), shared: do not modify"""
    f, n_points, seed, kw, iterations, robust = _FULL[name]
    w = gmap(f(Fp), n_points, seed, **kw)
    w["iterations"] = iterations
    if not robust:
        w["huber_mono"] = w["huber_stereo"] = np.inf
    return w


STOP_PERTURB = (20, 1.5, 0)  # lba_stop_support.perturb: degrees, metres, metres (points)
STOP_SEED = 911


@functools.lru_cache(maxsize=None)
def stop_map(Fp):
    w = gmap(Fp + 1, 300, STOP_SEED)
    w["iterations"] = 10
    return ST.perturb(w, STOP_SEED, *STOP_PERTURB)


def gba_looks(trace, iterations):
    """The looks gfs_gba_solve makes in an unstopped run with this trial trace: lba_stop_support.looks_of_trace without the entry
    check -- BundleAdjustment has none, so GBA's look j is look j + 1 there."""
    return ST.looks_of_trace(trace, iterations)[1:]


# ------------------------------------------------------------------------------------------------ the lists, by brute force
def brute_force_lists(w):
    """The structure lists stated directly (numpy, no counting): -> dict(order, blocks {(i, j): [(e1, e2), ...]}, pose {f: [e, ...]})
    with edge ids in the stable landmark-major numbering."""
    fixed = np.asarray(w["pose_fixed"]) != 0
    free_index = np.where(~fixed, np.cumsum(~fixed) - 1, -1)
    F = int((~fixed).sum())
    order = np.argsort(np.asarray(w["edge_point"]), kind="stable")
    f_of = free_index[np.asarray(w["edge_pose"])[order]] if len(order) else np.zeros(0, np.int64)
    l_of = np.asarray(w["edge_point"])[order]
    blocks = {(i, i): [] for i in range(F)}
    for l in np.unique(l_of):
        es = np.nonzero((l_of == l) & (f_of >= 0))[0]
        for e1 in es:
            for e2 in es:
                i, j = int(f_of[e1]), int(f_of[e2])
                if j <= i:
                    blocks.setdefault((i, j), []).append((int(e1), int(e2)))
    pose = {f: [int(e) for e in np.nonzero(f_of == f)[0]] for f in range(F)}
    return dict(order=order, blocks=blocks, pose=pose, F=F)
