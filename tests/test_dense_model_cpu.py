"""The FP64 model of the dense step kernels (tests/dense_model.py) checks itself -- no GPU.

For every operation and every shape of tests/test_gpu_dense_step.py, plain float64 NumPy computing the same thing
lies inside the bound the GPU tests impose (so the bound is one a correct FP64 implementation meets), and one
mutation per operation -- the faults the GPU tests exist for -- violates it (so the tests can see them).
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import dense_model as dm


def _inside(got, ref, tolerance):
    r = dm.ratio(got, ref, tolerance)
    assert r <= 1.0, r
    return r


def _outside(got, ref, tolerance):
    r = dm.ratio(got, ref, tolerance)
    assert r > 1.0, r


# ------------------------------------------------------------------------------------------------ Gram / TN
@pytest.mark.parametrize("nv,c", dm.GRAM_CASES)
def test_gram_float64_inside_bound(nv, c):
    Z = dm.panel(1, nv, c)
    _inside(Z.T @ Z, dm.gram(Z), dm.tol(dm.gram_bound, Z))


def test_gram_mutations_are_caught():
    nv, c = 257, 33
    Z = dm.panel(1, nv, c)
    ref, t = dm.gram(Z), dm.tol(dm.gram_bound, Z)
    G = Z.T @ Z
    _inside(G, ref, t)
    _outside(Z[1:].T @ Z[1:], ref, t)                       # one row left out of the sum
    _outside(Z[:nv - nv % 4].T @ Z[:nv - nv % 4], ref, t)   # the row tail (nv % 4) dropped
    Gm = G.copy()
    Gm[16:32, 0:16] = 0.0                                   # the strictly upper tile (0, 1) not mirrored
    _outside(Gm, ref, t)
    _outside(G + Z[64:128].T @ Z[64:128], ref, t)           # one row slice added twice
    Gm = G.copy()
    Gm[5, 7] += 40 * dm.U * abs(Z[:, 5]) @ abs(Z[:, 7])     # a single entry off by 40 dot-product roundings
    assert dm.ratio(Gm, ref, t) < 1.0                       # ... is inside (nv = 257 terms) -- and by 400, outside
    Gm[5, 7] += 400 * dm.U * abs(Z[:, 5]) @ abs(Z[:, 7])
    _outside(Gm, ref, t)


def test_tn_float64_and_mutation():
    A, B = dm.panel(2, 1021, 129), dm.panel(3, 1021, 7)
    ref, t = dm.tn(A, B), dm.tol(dm.tn_bound, A, B)
    _inside(A.T @ B, ref, t)
    _outside(A[:1020].T @ B[:1020], ref, t)                 # last row dropped


# ------------------------------------------------------------------------------------------------ NN
@pytest.mark.parametrize("n,p,q", [(1, 1, 1), (15, 3, 31), (16, 4, 32), (17, 5, 33), (1021, 129, 7), (65, 513, 128)])
def test_nn_float64_inside_bound(n, p, q):
    A, C, Y = dm.panel(4, n, p), dm.panel(5, p, q), dm.panel(6, n, q)
    for alpha, beta in ((1.0, 0.0), (-1.0, 1.0), (0.7, -0.3)):
        got = alpha * (A @ C) + (beta * Y if beta != 0.0 else 0.0)
        _inside(got, dm.nn(A, C, alpha, beta, Y), dm.tol(dm.nn_bound, A, C, alpha, beta, Y))


def test_nn_beta_zero_ignores_nan_and_the_mutation_is_caught():
    A, C = dm.panel(4, 17, 5), dm.panel(5, 5, 33)
    Y = np.full((17, 33), np.nan)
    ref, t = dm.nn(A, C, 1.0, 0.0, Y), dm.tol(dm.nn_bound, A, C, 1.0, 0.0, Y)
    assert np.isfinite(np.asarray(ref, dtype=float)).all() and np.isfinite(t).all()
    _inside(A @ C, ref, t)
    _outside(A @ C + 0.0 * Y, ref, t)                       # beta applied although it is zero: NaN gets through
    _outside(A[:, :4] @ C[:4], ref, t)                      # the p % 4 tail dropped


# ------------------------------------------------------------------------------------------------ gain
@functools.lru_cache(maxsize=None)
def _gain_mt(nv, kind):
    return sps.identity(nv, format="csr") if kind == "identity" else dm.sparse_rows(nv, 5, seed=7)


@pytest.mark.parametrize("nv,nb,c", dm.GAIN_CASES)
def test_gain_float64_inside_bound(nv, nb, c):
    Z, B = dm.panel(8, nv, c), dm.panel(9, nv, nb)
    st = dm.gain_stages(Z, B)
    for kind in ("identity", "sparse"):
        MT = _gain_mt(nv, kind)
        _inside(-(MT @ (Z @ (Z.T @ B))), dm.gain(MT, Z, B, -1.0, st), dm.tol(dm.gain_bound, MT, Z, B, -1.0, stages=st))


def test_gain_mutations_are_caught():
    nv, nb, c = 65, 7, 31
    Z, B, MT = dm.panel(8, nv, c), dm.panel(9, nv, nb), _gain_mt(65, "sparse")
    ref, t = dm.gain(MT, Z, B), dm.tol(dm.gain_bound, MT, Z, B, 1.0)
    _inside(MT @ (Z @ (Z.T @ B)), ref, t)
    _outside(MT @ (Z[:, :c - 1] @ (Z[:, :c - 1].T @ B)), ref, t)        # the column tail (c % 4) cut short by one
    _outside(MT @ (Z @ (Z[:64].T @ B[:64])), ref, t)                    # the 65th row missing from Z^T B
    _outside(MT.T @ (Z @ (Z.T @ B)), ref, t)                            # the transposed sparse factor


# ------------------------------------------------------------------------------------------------ panel norms
@pytest.mark.parametrize("nrows,m", dm.NORMS_CASES)
def test_panel_norms_float64_inside_bound(nrows, m):
    W = dm.panel(10, nrows, m)
    (f, tr), (tf, ttr) = dm.panel_norms(W), dm.tol(dm.panel_norms_bound, W)
    G = W.T @ W
    _inside(np.sqrt(np.sum(G * G)), f, tf)
    _inside(np.trace(G), tr, ttr)


def test_panel_norms_mutations_are_caught():
    W = dm.panel(10, 257, 17)
    (f, tr), (tf, ttr) = dm.panel_norms(W), dm.tol(dm.panel_norms_bound, W)
    G = W[:256].T @ W[:256]                                 # the 257th row missing
    _outside(np.sqrt(np.sum(G * G)), f, tf)
    _outside(np.trace(G), tr, ttr)
    G = W.T @ W
    _outside(np.trace(G[:16, :16]), tr, ttr)                # the 17th column missing from the trace
    _outside(np.sqrt(np.sum(np.triu(G) ** 2)), f, tf)       # the strict lower triangle missing from the norm


# ------------------------------------------------------------------------------------------------ recombination
def _sweep_inputs(cfg1, nslot, G, m):
    pr = cfg1[0]
    E = pr.M.T.tocsr()
    coefz, coefw, pad = dm.sweep_tables(nslot, G, seed=11)
    Us = dm.panel(12, nslot, pr.NV, m)
    Us[pad] = 0.0                                           # padding slots travel as exact zeros
    W = dm.panel(13, pr.NV, m)
    return Us, coefz, coefw, E, W


def _recombine64(Us, coefz, coefw, E, W):
    G, m = coefz.shape[1], Us.shape[2]
    Z = np.concatenate([np.tensordot(coefz[:, j], Us, axes=(0, 0)) for j in range(G)], axis=1)
    Wn = W + E @ np.tensordot(coefw, Us, axes=(0, 0))
    bn = np.array([np.sum(Z[:, j * m:(j + 1) * m] ** 2) for j in range(G)])
    return Z, Wn, bn, bn.sum()


@pytest.mark.parametrize("nslot,G,m", dm.SWEEP_CASES)
def test_recombine_float64_inside_bound(cfg1, nslot, G, m):
    args = _sweep_inputs(cfg1, nslot, G, m)
    ref = dm.recombine(*args)
    t = dm.tol(dm.recombine_bound, *args, Z=ref[0])
    for got, r, tt in zip(_recombine64(*args), ref, t):
        _inside(got, r, tt)


def test_recombine_mutations_are_caught(cfg1):
    nslot, G, m = 5, 3, 33
    Us, coefz, coefw, E, W = _sweep_inputs(cfg1, nslot, G, m)
    ref = dm.recombine(Us, coefz, coefw, E, W)
    tZ, tW, tbn, ttot = dm.tol(dm.recombine_bound, Us, coefz, coefw, E, W, Z=ref[0])
    # one slot's coefficient taken from the neighbouring slot (block 1 and the W coefficients)
    live = [s for s in range(nslot) if coefz[s].any()]
    s0 = live[0]
    cz = coefz.copy()
    cz[s0, 1] = coefz[(s0 + 1) % nslot, 1] if coefz[(s0 + 1) % nslot, 1] != coefz[s0, 1] else coefz[s0, 1] + 1.0
    cw = coefw.copy()
    cw[s0] = coefw[(s0 + 1) % nslot]
    assert cw[s0] != coefw[s0]
    Z, Wn, bn, tot = _recombine64(Us, cz, cw, E, W)
    _outside(Z, ref[0], tZ)
    _outside(Wn, ref[1], tW)
    _outside(bn, ref[2], tbn)
    # one block norm missing the last nrows % 64 rows
    nv = Us.shape[1]
    Z, Wn, bn, tot = _recombine64(Us, coefz, coefw, E, W)
    _inside(bn, ref[2], tbn)
    bn2 = bn.copy()
    bn2[2] = np.sum(Z[:nv - nv % 64, 2 * m:3 * m] ** 2)
    _outside(bn2, ref[2], tbn)
    _outside(bn2.sum(), ref[3], ttot)
    # the remainder columns of the fused kernel (256 % m threads idle) left unwritten in one block
    Z2 = Z.copy()
    Z2[:, m + 256 % m:2 * m][0] = 0.0
    _outside(Z2, ref[0], tZ)
    # E applied to the pressure-padded panel stride instead of the velocity rows: W off by a row shift
    _outside(W + E @ np.roll(np.tensordot(coefw, Us, axes=(0, 0)), 1, axis=0), ref[1], tW)


# ------------------------------------------------------------------------------------------------ lincomb / apply_e
@pytest.mark.parametrize("nrows,m,nvec", dm.LINCOMB_CASES)
def test_lincomb_float64_inside_bound(nrows, m, nvec):
    P, coef = dm.panel(14, nvec, nrows, m), dm.panel(15, nvec)
    _inside(np.tensordot(coef, P, axes=(0, 0)), dm.lincomb(coef, P), dm.tol(dm.lincomb_bound, coef, P))


def test_lincomb_mutation_is_caught():
    P, coef = dm.panel(14, 17, 65, 7), dm.panel(15, 17)
    ref, t = dm.lincomb(coef, P), dm.tol(dm.lincomb_bound, coef, P)
    flat = np.concatenate([P.reshape(17, -1), np.zeros((17, 24))], axis=1).ravel()    # panels 24 doubles apart ...
    wrong = flat[:17 * 65 * 7].reshape(17, 65, 7)                                      # ... read as if contiguous
    _outside(np.tensordot(coef, wrong, axes=(0, 0)), ref, t)
    _outside(np.tensordot(coef[:16], P[:16], axes=(0, 0)), ref, t)                     # the last vector left out


@pytest.mark.parametrize("m", [1, 16, 33])
@pytest.mark.parametrize("coef", [1.0, -0.5])
def test_apply_e_float64_inside_bound(cfg1, m, coef):
    pr = cfg1[0]
    E = pr.M.T.tocsr()
    V, W = dm.panel(16, pr.NV, m), dm.panel(17, pr.NV, m)
    ref, t = dm.apply_e(E, V, W, coef), dm.tol(dm.apply_e_bound, E, V, W, coef)
    _inside(W + coef * (E @ V), ref, t)
    _outside(W + coef * (E.T @ np.roll(V, 1, axis=1)) if m > 1 else W - coef * (E @ V), ref, t)


# ------------------------------------------------------------------------------------------------ QR
@pytest.mark.parametrize("nv,c", [(1, 1), (33, 33), (255, 127), (257, 129), (2049, 33)])
def test_qr_posdiag_reproduces_z(nv, c):
    Z = dm.wellcond(nv, c, seed=3)
    Q, R = dm.qr_posdiag(Z)
    eps = float(np.finfo(dm.LD).eps)
    assert np.all(np.diag(R) > 0) and np.all(np.tril(R, -1) == 0)
    # Householder QR: backward stable, errors ~ c eps ||Z|| with a modest constant
    assert np.linalg.norm(np.asarray(Q @ R - dm.ld(Z), dtype=float)) <= 8 * c * eps * np.linalg.norm(Z)
    assert np.linalg.norm(np.asarray(Q.T @ Q - np.eye(c), dtype=float)) <= 8 * c * eps


def test_qr_posdiag_rank_deficient_column():
    Z = dm.wellcond(300, 7, seed=3)
    Z[:, 1] = Z[:, 0]
    Q, R = dm.qr_posdiag(Z)
    assert abs(float(R[1, 1])) <= 1e-17 * np.linalg.norm(Z)
    assert np.linalg.norm(np.asarray(Q @ R - dm.ld(Z), dtype=float)) <= 1e-17 * np.linalg.norm(Z)


def test_qr_r_distance_of_lapack_is_the_recorded_one():
    """The entrywise distance between LAPACK's Householder R (float64, row signs fixed) and the longdouble R, over
    all matrices of the GPU test: the GPU test allows QR_R_FACTOR times the recorded maximum."""
    worst = 0.0
    for nv, c in dm.QR_CASES:
        Z = dm.qr_matrix(nv, c)
        worst = max(worst, dm.r_distance(dm.fix_row_signs(np.linalg.qr(Z, mode="r")), dm.qr_reference_r(nv, c)))
    print("largest distance %.3e" % worst)
    # another LAPACK build sums in another order: the record must be of the right size, not the last digit
    assert dm.QR_R_DISTANCE / dm.QR_R_FACTOR <= worst <= dm.QR_R_FACTOR * dm.QR_R_DISTANCE, worst
