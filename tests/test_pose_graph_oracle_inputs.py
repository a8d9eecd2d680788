"""A condition on the INPUTS of the GPU's full-solve test (tests/test_gpu_pose_graph.py), checked on the CPU: g2o's rule (numeric
Jacobians with delta = 1e-9, a first lambda of 1e-16) defines its own answer only up to rounding noise, so a map is a fair test only
if that noise is far below the bar the GPU is held to.  For every map of pose_graph_support.MAPS the float64 and the long-double
restatement agree to 1e-6 in translation (metres; the rings are 10 m across) and in the quaternion components, and so does the float64
restatement of the same graph with its vertices relabelled (the edges keep their order).  A map that misses this is replaced by
another seed, never excused.  No GPU."""
import numpy as np
import pytest

import pose_graph_support as pg

BAR = 1e-6


@pytest.mark.parametrize("name", sorted(pg.MAPS))
def test_float64_and_long_double_agree(name):
    a, b = pg.map_solution(name, np.float64), pg.map_solution(name, np.longdouble)
    dq, dt, ds = pg.pose_difference(a["est"], b["est"].astype(np.float64))
    chi = abs(float(a["final_chi2"]) / float(b["final_chi2"]) - 1)
    moved = np.abs(a["est"][:, 4:7] - pg.PoseGraph(pg.map_problem(name)).est[:, 4:7]).max()
    print(f"{name}: float64 against long double: dq {dq:.1e} dt {dt:.1e} ds {ds:.1e} chi2 rel {chi:.1e}; iterations {a['iterations_run']} / "
          f"{b['iterations_run']}; the poses moved {moved:.3f} m")
    assert dq <= BAR and dt <= BAR
    assert moved > 0.01  # the optimisation had something to do


@pytest.mark.parametrize("name", sorted(pg.MAPS))
def test_relabelled_vertices_agree(name):
    p = pg.map_problem(name)
    perm = np.random.default_rng(5).permutation(len(p["vertex_s"]))
    r = pg.PoseGraph(pg.relabel(p, perm)).optimize(p["iterations"], p["lambda_init"])
    a = pg.map_solution(name)
    dq, dt, ds = pg.pose_difference(a["est"], r["est"][perm])
    print(f"{name}: relabelled: dq {dq:.1e} dt {dt:.1e} ds {ds:.1e}")
    assert dq <= BAR and dt <= BAR


def _verdicts(sol):
    """per iteration: the accept / reject sequence of its trials and the relative change of chi2 it ended with"""
    out = {}
    for it, accepted, before, trial in sol["trace"]:
        seq, first, last = out.get(it, ("", float(before), float(before)))
        out[it] = (seq + ("A" if accepted else "r"), first, float(trial) if accepted else last)
    return [(seq, abs(first - last) / first) for seq, first, last in (out[k] for k in sorted(out))]


def test_accept_reject_sequences_agree_until_the_noise_floor():
    """Up to the first iteration whose chi2 change is below 1e-9 relative the two precisions take the same decisions; after it they
    are rounding noise.  At least one map has rejected trials in that part: with a free scale the rule rejects its second step ten
    times in both precisions (sim3.h:199's B ~ sigma^-3 makes the residual far from linear), long before chi2 stops changing."""
    rejected_before_the_floor = []
    for name in sorted(pg.MAPS):
        va, vb = _verdicts(pg.map_solution(name, np.float64)), _verdicts(pg.map_solution(name, np.longdouble))
        n = 0
        while n < min(len(va), len(vb)) and min(va[n][1], vb[n][1]) >= 1e-9:
            n += 1
        # (an iteration in which every trial is rejected changes nothing: it counts when the one before it still moved chi2)
        upto = n
        while upto < min(len(va), len(vb)) and "A" not in va[upto][0] and "A" not in vb[upto][0]:
            upto += 1
        print(name, [v[0] for v in va], [v[0] for v in vb], "compared:", upto)
        assert [v[0] for v in va[:upto]] == [v[0] for v in vb[:upto]], name
        if any("r" in v[0] for v in va[:upto]):
            rejected_before_the_floor.append(name)
    print("maps with rejected trials before the floor:", rejected_before_the_floor)
    assert rejected_before_the_floor
