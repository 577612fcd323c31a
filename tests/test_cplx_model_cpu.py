"""CPU tests of the complex-shift path's model (tests/cplx_model.py) and of what the library answers without a GPU
(DESIGN.md section 3f).  The GPU tests (tests/test_gpu_cplx.py) compare the device with this model, so the model is
held to dense references and to its identities here."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import cplx_model as cm
import small_ops as so
from optconpy_amd import _lib

OMEGAS25 = np.logspace(-2.0, 4.0, 25)


# ------------------------------------------------------------------------------------------------ 1. the product
@pytest.mark.parametrize("name", ["fe3", "unsym", "e_outside"])
def test_model_product_against_dense(name):
    """The sparse complex product equals the dense ``(beta A + alpha E) x_v + J^T x_p``, ``J x_v`` within its own bound,
    and the bound is not vacuous (it is below 1e-12 of the result's scale)."""
    op = so.get(name)
    rng = np.random.default_rng(5)
    X = rng.standard_normal((op.n, 3)) + 1j * rng.standard_normal((op.n, 3))
    for alpha, beta in ((-0.1j, 1.0), (-30 + 30j, 1.0), (-1e3 - 300j, 0.5)):
        ref, bound = cm.product(op.ops, alpha, beta, X)
        dense = np.vstack([(beta * op.Ad + alpha * op.Ed) @ X[:op.nv] + op.Jd.T @ X[op.nv:], op.Jd @ X[:op.nv]])
        assert np.all(np.abs(ref - dense) <= bound), (name, alpha)
        assert bound.max() <= 1e-12 * np.abs(dense).max()


# ------------------------------------------------------------------------------------------------ 2. GMRES
def _proxy_inverse(op, alpha):
    """x -> S(proxy(alpha), 1)^-1 x applied to the real and the imaginary part: the exact real-shift preconditioner."""
    ap = cm.proxy(alpha)
    return lambda v: op.solve(ap, 1.0, v.real) + 1j * op.solve(ap, 1.0, v.imag)


@pytest.mark.parametrize("name", so.NAMES)
def test_model_gmres_converges_on_the_family(name):
    """Complex flexible GMRES(8) with the exact inverse at the proxy shift converges at the seven shifts inside 60
    cycles (measured: 36 iterations at most), to a true residual of 1e-10, and solves the system it was given."""
    op = so.get(name)
    rng = np.random.default_rng(11)
    b = np.concatenate([rng.standard_normal(op.nv) + 1j * rng.standard_normal(op.nv), np.zeros(op.np)])
    worst = 0
    for alpha in cm.SHIFTS7:
        S = cm.saddle_cplx(*op.ops, alpha, 1.0)
        x, its, cycles, ok = cm.fgmres(lambda v: S @ v, _proxy_inverse(op, alpha), b, restart=8, tol=1e-10,
                                       max_cycles=60)
        assert ok and cycles <= 60, (name, alpha, its)
        assert np.linalg.norm(S @ x - b) <= 1e-10 * np.linalg.norm(b)
        ref = np.linalg.solve(S.toarray(), b)
        assert np.linalg.norm(x - ref) <= 2 * np.linalg.cond(S.toarray()) * 1e-10 * np.linalg.norm(ref)
        worst = max(worst, its)
    print("%s: at most %d iterations over the seven shifts" % (name, worst))


def test_real_equivalent_form_needs_twice_the_iterations():
    """Why the Arnoldi kernels are complex: at N = 15, w = 100 the real-equivalent 2n x 2n system with real inner
    products needs more than twice the iterations of the complex one, same preconditioner (the exact inverse at the
    proxy shift on both parts), same tolerance, no restarts."""
    calA, calE, J = so.finite_element(15)
    nv, n = calA.shape[0], calA.shape[0] + J.shape[0]
    alpha = -100j
    S = cm.saddle_cplx(calA, calE, J, alpha, 1.0)
    lu = spla.splu(sps.csc_matrix(cm.saddle_cplx(calA, calE, J, cm.proxy(alpha), 1.0).real))
    rng = np.random.default_rng(3)
    b = np.concatenate([rng.standard_normal(nv) + 1j * rng.standard_normal(nv), np.zeros(n - nv)])
    _, it_c, _, ok_c = cm.fgmres(lambda v: S @ v, lambda v: lu.solve(v.real) + 1j * lu.solve(v.imag), b, restart=300,
                                 tol=1e-10, max_cycles=1)
    S2 = cm.real_equivalent(S)
    b2 = np.concatenate([b.real, b.imag])
    _, it_r, _, ok_r = cm.fgmres(lambda v: S2 @ v, lambda v: np.concatenate([lu.solve(v[:n]), lu.solve(v[n:])]), b2,
                                 restart=300, tol=1e-10, max_cycles=1)
    print("N = 15, w = 100: complex %d iterations, real-equivalent %d" % (it_c, it_r))
    assert ok_c and ok_r
    assert it_r > 2 * it_c


# ------------------------------------------------------------------------------------------------ 3. the proxy export
def test_host_proxy_export_equals_the_rule():
    rng = np.random.default_rng(2)
    alphas = list(cm.SHIFTS7) + [-2.0 ** e * 1j for e in (-3, 0, 7)] + \
        [-(2.0 ** (e + 0.5)) * (1 + 1e-12) * 1j for e in (-2, 3)] + \
        list(-rng.uniform(0, 1e3, 40) - 1j * rng.uniform(-1e4, 1e4, 40))
    for a in alphas:
        got = _lib.host_cplx_proxy(a)
        assert got == cm.proxy(a), a
        assert got < 0 and np.log2(-got) == np.round(np.log2(-got))
        assert 2 ** -0.5 <= abs(a) / -got <= 2 ** 0.5 * (1 + 1e-12)
    assert _lib.host_cplx_proxy(-1j * 2.0 ** 0.5 * 1.0001) == -2.0 and _lib.host_cplx_proxy(-1.4j) == -1.0
    for bad in (1.0 + 1j, 1e-300 + 0j, 0j, complex("nan"), complex(-1.0, np.inf), complex(-np.inf, 0.0)):
        with pytest.raises(ValueError):
            _lib.host_cplx_proxy(bad)
        with pytest.raises(ValueError):
            cm.proxy(bad)
    out = C.c_double(7.0)
    assert _lib.load().ricadi_host_cplx_proxy(-1.0, 0.0, None) == -1
    assert _lib.load().ricadi_host_cplx_proxy(1.0, 0.0, C.byref(out)) == -1 and out.value == 7.0


# ------------------------------------------------------------------------------------------------ 4. transfer functions
BT_NAMES = ["fe3", "nv65_np24", "unsym", "stiff_grid", "arrow200", "nv63_np0"]


@pytest.mark.parametrize("name", BT_NAMES)
def test_transfer_function_and_balanced_truncation_bound(name):
    """The transfer function through the saddle matrix at the shift -i w equals ``Ch (i w Eh - Ah)^-1 Bh`` on an
    orthonormal basis of ker J (measured agreement: 4e-15 relative; asserted: 1e-11, which a sign or orientation
    error misses by twelve orders), and square-root balanced truncation from dense Gramians at r = 3 and 6 stays under
    its bound ``max_w sigma_max(G - G_r) <= 2 sum_{i > r} sigma_i`` over 25 frequencies (measured ratios 0.29 .. 0.78).
    The error is not trivially zero: it exceeds 1e-3 of the bound."""
    op = so.get(name)
    B, Cm = op.B, op.W.T
    pj = cm.Projected(op.Ad, op.Ed, op.theta, B, Cm)
    full = []
    for w in OMEGAS25:
        Gs, Gp = cm.transfer_saddle(op.calA, op.calE, op.J, B, Cm, w), pj.transfer(w)
        assert np.linalg.norm(Gs - Gp) <= 1e-11 * np.linalg.norm(Gp), (name, w)
        full.append(Gp)
    for r in (3, 6):
        red = pj.balanced_truncation(r)
        assert np.linalg.norm(red["er"] - np.eye(r)) <= 1e-8
        err = max(cm.sigma_max(G - cm.reduced_transfer(red, w)) for G, w in zip(full, OMEGAS25))
        bound = 2.0 * red["hsv"][r:].sum()
        print("%s r %d: max error %.3e, bound %.3e, ratio %.3f" % (name, r, err, bound, err / bound))
        assert 1e-3 * bound <= err <= bound, (name, r, err, bound)


# ------------------------------------------------------------------------------------------------ 5. without a GPU
def test_device_exports_refuse_a_context_without_an_operator():
    """The library loads without a GPU, and the three device entries return RICADI_ESTATE for a missing context /
    operator before they look at anything else."""
    lib = _lib.load()
    one = (C.c_double * 1)(-1.0)
    assert lib.ricadi_shift_solve_cplx_batch_dev(None, 1, one, one, one, None, 0, 1, None, None, None) == -5
    assert lib.ricadi_op_apply_cplx_batch_dev(None, 1, one, one, one, None, 0, 1, None, 0, None, 0, None) == -5
    assert lib.ricadi_cplx_orth_dev(None, 1, 1, 1, None, 0, 0, None, None) == -5
    assert b"operator" in lib.ricadi_last_error()
