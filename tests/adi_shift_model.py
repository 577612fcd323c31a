"""FP64 model of the automatic ADI shifts (``optconpy_amd.adi_shifts``, steps 1-2), in SciPy, for tests only.

Written from the recipe, on the oracle's saddle LU (``oracle.lin_alg_utils.SaddleLU``) instead of the device:

1. ``W0 = P^T W = cal E x`` with ``[[cal E, J^T], [J, 0]] [x; l] = [W; 0]``; ``warm_steps`` steps of the
   residual-form ADI at ``p0 = -sqrt(min * max |diag cal A / diag cal E|)`` on ``cal A - U V^T``
   (the oracle's ``solve_proj_lyap_stein``); orthonormal basis of ``[W0, Z_warm]`` (QR, SVD of R, at most 128
   directions down to 1e-10 relative).
2. ``H_A = Q^T (cal A - U V^T) Q``, ``H_E = Q^T cal E Q`` densely; candidates ``-|lambda|``.

Selection and admissibility are the product's own (``penzl_select``, ``admissible_order``): they are host code
on a handful of numbers and what the tests pin is the part in front of them.
"""
import numpy as np
import scipy.sparse as sps

from oracle import lin_alg_utils as olau, proj_ric_utils as opru
from optconpy_amd.adi_shifts import (BASIS_RTOL, MAX_BASIS, admissible_order, candidates, initial_shift,
                                     penzl_select)


def diag_ratio(calA, calE):
    da, de = sps.csr_matrix(calA).diagonal(), sps.csr_matrix(calE).diagonal()
    ok = (da != 0) & (de != 0)
    return np.abs(da[ok] / de[ok])


def model_basis(calA, calE, J, W, U=None, V=None, warm_steps=2):
    """Step 1: the orthonormal basis (NV x k) and p0."""
    calA, calE = sps.csr_matrix(calA), sps.csr_matrix(calE)
    W = np.asarray(W, dtype=float).reshape(calA.shape[0], -1)
    p0 = initial_shift(diag_ratio(calA, calE))
    x = olau.SaddleLU(calE, J).solve(W)[:calA.shape[0]]
    blocks = [calE @ x]
    if warm_steps > 0:
        r = opru.solve_proj_lyap_stein(amat=calA, mmat=calE, jmat=J, wmat=W, transposed=True,
                                       umat=U, vmat=None if V is None else np.asarray(V).T,
                                       adi_dict=dict(ms=[p0], adi_max_steps=warm_steps, adi_newZ_reltol=0.0))
        blocks.append(r["zfac"])
    Q, R = np.linalg.qr(np.hstack(blocks))
    Ur, s, _ = np.linalg.svd(R)
    keep = min(int(np.count_nonzero(s > BASIS_RTOL * s[0])), MAX_BASIS)
    return Q @ Ur[:, :keep], p0


def model_pencil(calA, calE, Q, U=None, V=None):
    """Step 2: the projected pencil, densely."""
    HA = Q.T @ (sps.csr_matrix(calA) @ Q)
    if U is not None:
        HA = HA - (Q.T @ U) @ (np.asarray(V).T @ Q)
    HE = Q.T @ (sps.csr_matrix(calE) @ Q)
    return HA, HE


def model_candidates(calA, calE, J, W, U=None, V=None, warm_steps=2):
    Q, _ = model_basis(calA, calE, J, W, U, V, warm_steps)
    return candidates(*model_pencil(calA, calE, Q, U, V))


def model_shifts(calA, calE, J, W, U=None, V=None, num=8, warm_steps=2):
    """The list ``auto_shifts`` would return on this operator (no fallback)."""
    return admissible_order(penzl_select(model_candidates(calA, calE, J, W, U, V, warm_steps), num))
