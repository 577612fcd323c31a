"""GPU tests of the setup's dense coarse-matrix inverse (ricadi_dense_inverse_batch) against numpy.linalg.inv,
alone and in batches, for sizes around the 128-row blocks of the block Gauss-Jordan route and at the coarse size of
cfg2 (k ~ 1 800)."""
import numpy as np
import pytest

from optconpy_amd import _lib

pytestmark = pytest.mark.gpu


def _mats(k, nb, seed):
    """nb well-conditioned, non-symmetric k x k matrices (diagonally dominant: route 0 needs no pivoting)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((nb, k, k)) / np.sqrt(k)
    A += (2.0 + rng.random((nb, 1, 1))) * np.eye(k)
    return A


@pytest.mark.parametrize("k", [1, 17, 127, 128, 129, 300, 1800])
@pytest.mark.parametrize("nb", [1, 17, 24])
def test_dense_inverse_batch_against_numpy(k, nb):
    A = _mats(k, nb, 1000 * k + nb)
    with _lib.Context(0) as ctx:
        inv, route = ctx.dense_inverse_batch(A)
    assert route == 0
    ref = np.linalg.inv(A)
    for i in range(nb):
        err = np.linalg.norm(inv[i] - ref[i]) / np.linalg.norm(ref[i])
        assert err < 1e-12, (i, err)


def test_vanishing_leading_pivot_finishes_on_route_1():
    """A matrix whose leading entry is zero (invertible only with pivoting) sends the whole batch through the
    pivoted route; every matrix of it, the healthy ones included, comes back inverted."""
    k = 129
    A = _mats(k, 3, 7)
    A[1, 0, 0] = 0.0
    A[1, 0, 1:] = A[1, 0, 1:] + 1.0          # the first row stays independent
    with _lib.Context(0) as ctx:
        inv, route = ctx.dense_inverse_batch(A)
    assert route == 1
    for i in range(3):
        assert np.linalg.norm(A[i] @ inv[i] - np.eye(k)) < 1e-10
