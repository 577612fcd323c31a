"""CPU tests of LQG-balanced truncation: the host step of the library (``ricadi_host_lqg_balance``) against the NumPy
model, the model's own identities on the CPU oracle's factors, the header and the ctypes signatures of the new exports.

tests/test_gpu_lqgbt.py holds the device path to this model; these tests have to pass for that to mean anything.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lqgbt_model as lm
from optconpy_amd import _lib

EPS = lm.EPS


# ------------------------------------------------------------------------------------------- 1. the host export
def _check_host(S, tol, order, r_expected=None):
    """sigma to ``kc kf eps ||S||_2`` -- the SVD's rounding: a backward error of a modest multiple of eps ||S||_2 per
    sweep over the kc kf entries moves a singular value by no more (Weyl) --; the coefficient matrices through
    ``coefL^T S coefR = I_r`` to ``8 max(kc, kf) eps sigma_1 / sigma_r``: the entries are u_i^T S v_j / sqrt(sigma_i
    sigma_j), the singular vectors' orthogonality defect is of the order k eps, S scales it by sigma_1 and the two roots
    divide by at least sigma_r."""
    kc, kf = S.shape
    r, sig, cl, cr = _lib.host_lqg_balance(S, tol, order)
    rm_, sm_, clm, crm = lm.balance_svd(S, tol, order if order else None)
    nrm = np.linalg.norm(S, 2)
    err = np.abs(sig - sm_).max()
    print("S %d x %d: r %d (model %d), sigma error %.3e, bound %.3e" % (kc, kf, r, rm_, err, kc * kf * EPS * nrm))
    assert sig.shape == (min(kc, kf),) and np.all(np.diff(sig) <= 0)
    assert err <= kc * kf * EPS * nrm
    assert r == rm_ and (r_expected is None or r == r_expected)
    assert cl.shape == (kc, r) and cr.shape == (kf, r)
    defect = np.abs(cl.T @ S @ cr - np.eye(r)).max()
    bound = 8 * max(kc, kf) * EPS * sig[0] / sig[r - 1]
    print("   coefL^T S coefR - I: %.3e, bound %.3e" % (defect, bound))
    assert defect <= bound
    return r, sig, cl, cr


@pytest.mark.parametrize("shape", [(5, 37), (37, 5), (1, 1), (64, 64)])
def test_host_balance_random(shape):
    S = np.random.default_rng(shape[0] * 100 + shape[1]).standard_normal(shape)
    _check_host(S, 1e-12, 0, r_expected=min(shape))


def test_host_balance_rank_deficient():
    rng = np.random.default_rng(7)
    S = rng.standard_normal((10, 3)) @ rng.standard_normal((3, 12))
    r, sig, _, _ = _check_host(S, 1e-10, 0, r_expected=3)
    assert sig[3] <= 10 * 12 * EPS * np.linalg.norm(S, 2)


def test_host_balance_order_below_count():
    S = np.random.default_rng(11).standard_normal((20, 23))
    r, sig, cl, cr = _check_host(S, 1e-12, 4, r_expected=4)
    assert np.count_nonzero(sig > 1e-12 * sig[0]) == 20


def test_host_balance_error_returns():
    with pytest.raises(RuntimeError):
        _lib.host_lqg_balance(np.zeros((3, 4)))
    for bad in (np.nan, np.inf):
        S = np.ones((3, 4))
        S[1, 2] = bad
        with pytest.raises(ValueError):
            _lib.host_lqg_balance(S)
    with pytest.raises(ValueError):
        _lib.host_lqg_balance(np.ones((2, 2)), tol=1.0)
    with pytest.raises(ValueError):
        _lib.host_lqg_balance(np.ones((2, 2)), tol=-1e-3)


# ------------------------------------------------------------------------------------------- 2. the model's identities
@pytest.mark.parametrize("N", [4, 8])
def test_model_identities_on_oracle_factors(N):
    p = lm.problem(N)
    zc, zf = lm.oracle_factors(N)
    red = lm.balance(p["M"], p["A"], p["B"], p["C"], zc, zf, tol=1e-10)
    r, sig = red["order"], red["hsv"]
    ds = lm.Dense(p["M"], p["A"], p["J"], p["B"], p["C"])
    # T_l^T M T_r = I_r: the defect is the rounding of S (lm.identity_defect_bound's first factor) over sigma_r
    k, nv = max(zc.shape[1], zf.shape[1]), zc.shape[0]
    d_s = EPS * (nv * np.linalg.norm(np.abs(zc).T @ (abs(p["M"]) @ np.abs(zf))) + 8 * k * sig[0])
    defect = np.linalg.norm(red["er"] - np.eye(r))
    print("N %d: r %d, ||T_l^T M T_r - I||_F %.3e, bound %.3e" % (N, r, defect, 2 * d_s / sig[r - 1]))
    assert defect <= 2 * d_s / sig[r - 1]
    # the two reduced Riccati residuals
    # (lm.reduced_residual_check: against T^T R T with the computed identity defect, and in the issue's form)
    lm.assert_reduced_residuals(ds, red, zc, zf, "N %d" % N)
    # ... and the check is one that fails: a relative error of 1e-6 in A_r or in B_r is caught
    for key in ("ar", "br"):
        with pytest.raises(AssertionError):
            lm.assert_reduced_residuals(ds, dict(red, **{key: red[key] * (1 + 1e-6)}), zc, zf, "perturbed " + key)
    # truncation at the rounding level only: the closed loop of the dense projected plant with the controller
    full = lm.balance(p["M"], p["A"], p["B"], p["C"], zc, zf, tol=1e-14)
    ak, bk, ck = lm.controller(full)
    a = np.linalg.solve(ds.Mh, ds.Ah)
    b = np.linalg.solve(ds.Mh, ds.Bh)
    loop = np.block([[a, b @ ck], [bk @ ds.Ch, ak]])
    top = np.linalg.eigvals(loop).real.max()
    print("   order %d of %d: largest real part of the closed loop %.4f" % (full["order"], a.shape[0], top))
    assert top < 0.0


def test_dense_sigma_fixture_matches_recomputation():
    """The recorded dense-route values the GPU tests compare with (tests/golden/lqgbt_dense_sigma.npz) against a fresh
    run at N = 4, over the values above 1e-6 sigma_1 (both runs are the same LAPACK calls)."""
    for kind, route in (("riccati", lm.dense_route), ("lyapunov", lm.dense_lyap_route)):
        ref = route(4)[1]
        assert lm.sigma_distance(lm.dense_sigma(4, kind), ref) <= 1e-8


# ------------------------------------------------------------------------------------------- 3. header, ABI, ctypes
def test_header_exports_abi_and_signatures():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    hdr = open(os.path.join(root, "include", "ricadi.h")).read()
    for proto in (r"int ricadi_cross_gram_dev\(ricadi_ctx\* ctx, int n, int p, int q, const double\* dX, int ldx, "
                  r"const double\* dY, int ldy,\s+double\* dG\);",
                  r"int ricadi_project_pencil_twosided_dev\(ricadi_ctx\* ctx, const double\* dL, const double\* dRb, "
                  r"int r, double\* dHA,\s+double\* dHE\);",
                  r"int ricadi_lqg_balance_dev\(ricadi_ctx\* ctx, const double\* dZc, int kc, const double\* dZf, int kf, "
                  r"const double\* dB,\s+int nb, const double\* dCt, int nc, double tol, int order, int\* r_out, "
                  r"double\* sigma_out,\s+double\* dTl, double\* dTr, double\* Ar_out, double\* Er_out, double\* Br_out, "
                  r"double\* Cr_out\);",
                  r"int ricadi_host_lqg_balance\(int kc, int kf, const double\* S, double tol, int order, int\* r_out, "
                  r"double\* sigma_out,\s+double\* coefl_out, double\* coefr_out\);"):
        assert re.search(proto, hdr), proto
    assert "ABI 412" in hdr
    assert "cal A = A, cal E = M" in hdr                      # the orientation the device entry expects
    lib = _lib.load()
    assert lib.ricadi_version() == _lib.ABI_VERSION == 414
    ip, dp, vp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_void_p
    sig = {"ricadi_cross_gram_dev": [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int, vp],
           "ricadi_project_pencil_twosided_dev": [vp, vp, vp, C.c_int, vp, vp],
           "ricadi_lqg_balance_dev": [vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_double, C.c_int, ip, dp,
                                      vp, vp, dp, dp, dp, dp],
           "ricadi_host_lqg_balance": [C.c_int, C.c_int, dp, C.c_double, C.c_int, ip, dp, dp, dp]}
    for name, args in sig.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
        # as many parameters as the header declares
        decl = re.search(name + r"\(([^)]*)\)", hdr).group(1)
        assert len(decl.split(",")) == len(args), name


def test_python_entry_points_exist():
    import sadptprj_riclyap_adi.lqgbt as dropin
    from optconpy_amd import lqgbt
    assert dropin.balance_factors is lqgbt.balance_factors and dropin.lqgbt_reduce is lqgbt.lqgbt_reduce
    assert lqgbt.MAX_COLS == 1024 and lqgbt.MAX_ORDER == 128
    with pytest.raises(ValueError):
        lqgbt.lqgbt_reduce(ric_solver="other")
    with pytest.raises(ValueError):
        lqgbt.lqgbt_reduce(gramians="other")
