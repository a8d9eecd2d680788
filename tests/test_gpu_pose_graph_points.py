"""GPU test of the essential graph's point correction (gfs_essential_graph_correct_points: k_eg_correct_points alone): every map
point through correctedSwr.map(Srw.map(P)) of its reference vertex (reference src/Optimizer.cc:2387-2409), in double, cast to float.
No libm call is involved, so the device is bit-identical to the restatement: 10 000 points, among them points without a reference,
points on the fixed vertex (whose Sim3 does not change) and scales away from 1."""
import numpy as np
import pytest

import pose_graph_support as pg

pytestmark = pytest.mark.gpu


def test_correct_points_bitwise(gpu_api):
    rng = np.random.default_rng(11)
    V, M = 50, 10000
    u = np.concatenate([rng.normal(0, 1.0, (V, 3)), rng.uniform(-10, 10, (V, 3)), rng.uniform(-0.3, 0.3, (V, 1))], 1)
    before = pg.sim3_exp(u)[0]
    after = pg.sim3_mul(pg.sim3_exp(np.concatenate([rng.normal(0, 0.02, (V, 3)), rng.normal(0, 0.1, (V, 3)), rng.normal(0, 0.05, (V, 1))], 1))[0], before)
    after[0] = before[0]  # the fixed vertex
    pts = rng.uniform(-20, 20, (M, 3)).astype(np.float32)
    ref = rng.integers(-1, V, M).astype(np.int32)
    ref[:100] = 0
    ref[100:200] = -1
    opt = gpu_api.EssentialGraphOptimizer(max_vertices=64, max_edges=16, max_points=M)
    got = opt.correct_points(before, after, pts, ref)
    want = pg.correct_points(before, after, pts, ref)
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert (got[ref < 0] == pts[ref < 0]).all()
    assert np.abs(got[:100] - pts[:100]).max() <= 4e-6  # there and back in double: at most the last bit of a float at 20 m
    assert np.abs(got[ref > 0] - pts[ref > 0]).max() > 0.1
    assert np.abs(before[:, 7] - 1).max() > 0.1
    with pytest.raises(gpu_api.GfsError):
        opt.correct_points(before, after, pts, np.where(np.arange(M) == 5, V, ref))
    with pytest.raises(gpu_api.GfsError):
        opt.correct_points(before, after, np.zeros((M + 1, 3), np.float32), np.zeros(M + 1, np.int32))
    opt.close()
