"""Checks of the FP64 cycle model (tests/precond_model.py) itself, without a GPU: exactness where the mathematics
says so, the relation of its folded and unfolded forms, and that its per-block metric catches the typical kernel
bugs with a margin over the tolerances the GPU parity tests use (tests/test_gpu_precond_parity.py)."""
import numpy as np
import pytest
import scipy.sparse as sps

from optconpy_amd import _lib
import precond_model as pm

SHIFTS = (-1.0, -40.0, -1500.0)


@pytest.fixture(scope="module")
def ops(cfg1):
    pr = cfg1[0]
    return (-pr.A - pr.Nc).T.tocsr(), pr.M.T.tocsr(), pr.J.tocsr()


def _smoothed(calA, Yv, omega=0.5):
    K0 = 0.5 * (calA + calA.T)
    Dinv = sps.diags(1.0 / K0.diagonal())
    return (Yv - omega * (Dinv @ (K0 @ Yv))).tocsr()


def _structure(calA, calE, J, one_block=False, smoothed=False, coarse=True):
    nv, np_ = calA.shape[0], J.shape[0]
    JJ = (abs(J) @ abs(J).T).tocsr()
    if one_block:
        vb, pb = np.zeros(nv, int), np.zeros(np_, int)
    else:
        vb = _lib.host_aggregate(abs(calA) + abs(calE), 32)[0]
        pb = _lib.host_aggregate(JJ, 32)[0]
    if not coarse:
        return pm.plain_structure(calA, calE, J, vb, pb)
    va = _lib.host_aggregate(abs(calE), 16)[0]
    pa = _lib.host_aggregate(JJ, 24)[0]
    P = None
    if smoothed:
        kcv = va.max() + 1
        Yv = sps.csr_matrix((np.ones(nv), (np.arange(nv), va)), shape=(nv, kcv))
        Pv = _smoothed(calA, Yv)
        Yp = sps.csr_matrix((np.ones(np_), (np.arange(np_), pa)), shape=(np_, pa.max() + 1))
        P = sps.block_diag([Pv, Yp]).tocsr()
    return pm.plain_structure(calA, calE, J, vb, pb, va, pa, P)


@pytest.mark.parametrize("coarse", ["none", "plain", "smoothed"])
def test_one_block_each_makes_simple_exact(ops, coarse):
    """One velocity block and one pressure block covering everything: Ahat = the velocity operator, Shat its exact
    Schur complement, so the SIMPLE sweep solves S z = rho exactly and P^-1 S = I to round-off whatever the coarse
    space (none, plain aggregates, smoothed aggregates) -- the coarse correction then cancels.  With smoothed
    aggregates that holds for the unfolded form z = Pe + SIMPLE(r - SPe); the folded form's (P - Y)_v e also passes
    through the pressure step -- its difference is checked in the next test."""
    calA, calE, J = ops
    st = _structure(calA, calE, J, one_block=True, smoothed=coarse == "smoothed", coarse=coarse != "none")
    model = pm.CycleModel(calA, calE, J, st)
    X = np.random.default_rng(1).standard_normal((calA.shape[0] + J.shape[0], 3))
    for p in SHIFTS:
        S = model.saddle(p, 1.0)
        Z = model.apply(p, 1.0, S @ X, folded=False if coarse == "smoothed" else None)
        assert np.linalg.norm(Z - X) / np.linalg.norm(X) < 1e-9, (coarse, p)


def test_folded_and_unfolded_forms_differ_by_the_simple_image_of_the_smoothing_term(ops):
    """The folded cycle adds (P - Y)_v e to the first sweep's output, which then passes through the pressure step:
    so once the unfolded form's prolongation P e is replaced by Y e + (P - Y) e, folded - unfolded =
    [-G Shat^-1 J ; Shat^-1 J] (P - Y)_v e.  With plain aggregation (P = Y) the two forms coincide."""
    calA, calE, J = ops
    nv = calA.shape[0]
    R = np.random.default_rng(2).standard_normal((nv + J.shape[0], 4))
    for smoothed in (False, True):
        st = _structure(calA, calE, J, smoothed=smoothed)
        model = pm.CycleModel(calA, calE, J, st)
        for p in SHIFTS:
            zf = model.apply(p, 1.0, R, folded=True)
            zu = model.apply(p, 1.0, R, folded=False)
            op = model.operands(p, 1.0)
            e = np.linalg.solve((model.P.T @ op["SP"]).toarray(), model.P.T @ R)
            d = op["PmY"] @ e
            dp = op["Sinv"] @ (J @ d)
            expect = np.vstack([-op["G"] @ dp, dp])
            scale = np.linalg.norm(zf)
            assert np.linalg.norm(zf - zu - expect) / scale < 1e-10, (smoothed, p)
            if not smoothed:
                assert np.linalg.norm(zf - zu) / scale < 1e-12, p
            else:
                assert np.linalg.norm(expect) / scale > 1e-3, p      # the term is there to be accounted for


def _last_partial_block(st):
    cnt = np.diff(st["bv_ptr"])
    part = np.nonzero(cnt < st["bs"])[0]
    assert part.size, "no partial velocity block"
    b = part[-1]
    return np.asarray(st["bv_rows"][st["bv_ptr"][b]:st["bv_ptr"][b + 1]])


@pytest.mark.parametrize("smoothed", [False, True])
def test_metric_catches_typical_kernel_bugs(ops, smoothed):
    """Synthetic bugs on a model output must exceed the tolerance its GPU test applies by at least 10x: two rows
    swapped inside one block, one block taken from another shift, the coarse term dropped in the last, partial block
    (FP64 form against the exact model and the BF16 form against the rounded one), and the FP16 rounding of the input
    ignored (against the rounded model)."""
    calA, calE, J = ops
    st = _structure(calA, calE, J, smoothed=smoothed)
    model = pm.CycleModel(calA, calE, J, st)
    R = np.random.default_rng(3).standard_normal((calA.shape[0] + J.shape[0], 16))
    hot = dict(h16=True, x32=True, mid32=True, b16=True)
    p, q = SHIFTS[0], SHIFTS[2]
    rows = _last_partial_block(st)
    blk = np.asarray(st["bv_rows"][st["bv_ptr"][3]:st["bv_ptr"][4]])
    for rounded, tol in ((None, pm.tol_fp64(model, p, 1.0)), (hot, pm.TOL_ROUNDED)):
        z = model.apply(p, 1.0, R, rounded=rounded)
        other = model.apply(q, 1.0, R, rounded=rounded)
        bugs = {}
        w = z.copy()
        w[blk[[0, 1]]] = w[blk[[1, 0]]]
        bugs["rows swapped"] = w
        w = z.copy()
        w[blk] = other[blk]
        bugs["block of another shift"] = w
        w = z.copy()
        e = model.P.T @ (pm.to_fp16(R) if rounded else R)
        e = (pm.to_fp32(model.operands(p, 1.0)["Einv"]) if rounded else model.operands(p, 1.0)["Einv"]) @ e
        w[rows] -= (model.Y @ e)[rows]
        bugs["coarse term dropped in the last partial block"] = w
        if rounded:
            bugs["FP16 input rounding ignored"] = model.apply(p, 1.0, R, rounded=dict(hot, h16=False))
        for name, w in bugs.items():
            err = pm.worst_block_error(w, z, st)
            assert err >= 10 * tol, (name, rounded is not None, err, tol)


def test_bf16_form_stays_within_the_exact_model_tolerance(ops):
    """The rounded model of the hot form against the exact model, per column: what the GPU test's BF16-level
    tolerance must admit (its margin is asserted here, on the CPU, for the cfg1 operator at three shifts)."""
    calA, calE, J = ops
    for smoothed in (False, True):
        st = _structure(calA, calE, J, smoothed=smoothed)
        model = pm.CycleModel(calA, calE, J, st)
        R = np.random.default_rng(4).standard_normal((calA.shape[0] + J.shape[0], 16))
        for p in SHIFTS:
            zr = model.apply(p, 1.0, R, rounded=dict(h16=True, x32=True, mid32=True, b16=True))
            ze = model.apply(p, 1.0, R)
            assert np.max(pm.column_errors(zr, ze)) < 0.5 * pm.TOL_BF16, (smoothed, p)
            assert np.max(pm.column_errors(zr, ze)) > 1e-2 * pm.TOL_BF16, (smoothed, p)   # the rounding is there


def test_rounding_helpers():
    x = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.0e38, 1.0 / 3.0])
    assert pm.to_bf16(x)[0] == 1.0                          # ties to even
    assert pm.to_bf16(x)[1] == 1.0 + 2.0 ** -6
    assert np.isfinite(pm.to_bf16(x)[2])                     # FP32's exponent range
    assert abs(pm.to_bf16(x)[3] - 1.0 / 3.0) <= 2.0 ** -9 / 3.0 * 2
    assert pm.to_fp16(np.array([1.0 + 2.0 ** -12]))[0] == 1.0
