"""The neighbourhood covariances of GICP's preprocessing are what they were before csrc/eig3_direct.hpp (MI355X): every one of the six
doubles a point that api.RegistrationGICP.preprocessed returns is bit-equal to tests/golden/knn_cov_parent.npz, recorded by
tools/record_knn_cov_parent.py with the library of the commit named in the fixture, where gicp.hip indexed private arrays by i0, k and
l.  Once on the default path (k_knn_cov, and k_knn_cov_far / k_knn_cov_far_wg for the queries it defers) and once under
GFS_GICP_KNN_EXACT=1 (every query through the two deferred kernels); single calls and one ragged batch of three clouds.  The clouds
are in tests/knn_cov_parent_support.py: those of the row-walk tests up to 1 200 points, two lattice planes, a line, seven points."""
import numpy as np
import pytest

import knn_cov_parent_support as S

pytestmark = pytest.mark.gpu
KEYS = S.NAMES + tuple("batch%d" % b for b in range(len(S.BATCH)))


@pytest.fixture(scope="module")
def recorded():
    return S.load()


@pytest.fixture(scope="module")
def runs(gpu_api, recorded):
    """Everything once, from the clouds as the fixture holds them."""
    from test_gpu_gms import _Hip
    hip = _Hip()
    out = S.run_all(gpu_api, recorded[0], hip)
    hip.free()
    return out


def test_the_fixture_holds_the_clouds_of_the_support_modules(recorded):
    clouds, golden, commit = recorded
    assert commit == "9651a99"
    for name in S.NAMES:
        assert clouds[name].dtype == np.float32 and len(clouds[name]) <= S.MAX_POINTS
        assert clouds[name].tobytes() == S.cloud(name).tobytes(), name
    assert set(golden) == {(p, k) for p in S.PATHS for k in KEYS}


@pytest.mark.parametrize("path", S.PATHS)
@pytest.mark.parametrize("key", KEYS)
def test_covariances_have_the_parents_bits(runs, recorded, path, key):
    got, want = runs[path, key], recorded[1][path, key]
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape, (path, key, got.shape, want.shape)
    diff = (got.view(np.uint64) != want.view(np.uint64)).any(1)
    print(f"{path} {key}: {len(got)} points, covariances that differ from the parent's {int(diff.sum())}")
    assert not diff.any(), (path, key, int(diff.sum()), np.nonzero(diff)[0][:8], got[diff][:2], want[diff][:2])
