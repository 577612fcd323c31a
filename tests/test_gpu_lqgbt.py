"""GPU tests of LQG-balanced truncation (optconpy_amd/lqgbt.py, ricadi_lqg_balance_dev).

1. the cross-Gram kernel entry by entry against a longdouble ``X^T Y``, and bitwise twice;
2. the two-sided projected pencil against dense longdouble ``L^T (A Rb)`` / ``L^T (E Rb)`` on the tiny and irregular
   operators of tests/small_ops.py and the N = 4 finite-element operator, bitwise twice, and against K7 for L = Rb;
3. ``balance_factors`` on device-produced factors at N = 8 against the NumPy model on the same factors;
4. ``lqgbt_reduce`` end to end at N = 8 against the dense route, both Riccati solvers, and with the Lyapunov factors.

tests/test_lqgbt_cpu.py holds the model to its identities; it has to pass for these to mean anything.
"""
import numpy as np
import pytest

import lqgbt_model as lm
import small_ops as so
from optconpy_amd import _lib, backend, lqgbt
from optconpy_amd import problems as pb
from optconpy_amd import proj_ric_utils as pru

pytestmark = pytest.mark.gpu
U = 2.0 ** -53            # unit roundoff of FP64
LD = np.longdouble
# A sum of n products formed in ANY order, with or without fused multiply-adds, is within gamma_n sum |x_i y_i| of the
# exact one, gamma_n = n U / (1 - n U) <= 1.01 n U for n <= 2^40 (Higham, Accuracy and Stability, section 3.1); the
# longdouble reference (64-bit significand) adds n 2^-64 of the same sum, under 0.001 n U.
C_SUM = 1.02


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A test that leaves the device in an error state ends the run: nothing more is started on it."""
    yield
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:            # pragma: no cover - only after a device fault
        pytest.exit("device error after a test, stopping: %r" % (e,), returncode=3)


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def plain_ctx():
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


# ------------------------------------------------------------------------------------------- 1. the cross-Gram kernel
@pytest.mark.parametrize("p,q", [(1, 1), (5, 37), (33, 16), (130, 70)])
@pytest.mark.parametrize("n", [3, 61, 450, 1682])
def test_cross_gram_entry_by_entry(plain_ctx, n, p, q):
    """Row counts that are no multiple of 4 or of a slice (3, 61, 450, 1682), ragged 16- and 32-column tiles, p != q,
    leading dimensions above the widths with NaN in the padding (it must not be read).  Every entry of G is a sum of n
    products, so it lies within ``C_SUM n U (|X|^T |Y|)`` of the longdouble value (see C_SUM)."""
    rng = np.random.default_rng(1000 * n + 10 * p + q)
    ldx, ldy = p + 3, q + 5
    Xp, Yp = np.full((n, ldx), np.nan), np.full((n, ldy), np.nan)
    Xp[:, :p], Yp[:, :q] = rng.standard_normal((n, p)), rng.standard_normal((n, q))
    X, Y = Xp[:, :p], Yp[:, :q]
    ref = np.asarray(X.astype(LD).T @ Y.astype(LD))
    bound = C_SUM * n * U * (np.abs(X).T @ np.abs(Y))
    Xd, Yd = _dev(Xp), _dev(Yp)
    outs = []
    for _ in range(2):
        Gd = _dev(np.full((p + 1, q), np.nan))                       # one guard row behind G
        plain_ctx.cross_gram_dev(n, p, q, Xd.data_ptr(), ldx, Yd.data_ptr(), ldy, Gd.data_ptr())
        outs.append(_host(Gd))
    G = outs[0][:p]
    ratio = float(np.max(np.abs(G.astype(LD) - ref) / bound))
    print("n %d p %d q %d: largest error / bound %.3f" % (n, p, q, ratio))
    assert np.all(np.isfinite(G)) and ratio <= 1.0
    assert np.all(np.isnan(outs[0][p])), "guard row written"
    assert np.array_equal(outs[0][:p], outs[1][:p])


def test_cross_gram_argument_contract(plain_ctx):
    X = _dev(np.ones((8, 4)))
    G = _dev(np.zeros((4, 4)))
    for n, p, q, ldx, ldy in ((0, 4, 4, 4, 4), (8, 0, 4, 4, 4), (8, 4, 1025, 4, 1025), (8, 4, 4, 3, 4), (8, 4, 4, 4, 3)):
        with pytest.raises(ValueError):
            plain_ctx.cross_gram_dev(n, p, q, X.data_ptr(), ldx, X.data_ptr(), ldy, G.data_ptr())


# ------------------------------------------------------------------------------------------- 2. the two-sided pencil
RANKS = (1, 5, 16, 17, 128)


def _pencil_operator(name):
    if name == "fe4":
        calA, calE, J = so.finite_element(4)
        return calA, calE, J, calA.toarray(), calE.toarray(), {}
    op = so.get(name)
    return op.calA, op.calE, op.J, op.Ad, op.Ed, op.opts


@pytest.mark.parametrize("name", so.NAMES + ["fe4"])
def test_twosided_pencil_against_dense(name):
    """H_A = L^T (A Rb) and H_E = L^T (E Rb): an entry is a sum over the rows of at most nv products of an entry of L
    with a row sum of at most ``w`` products (w: the longest row of the pattern), accumulated chunk by chunk and then
    over at most nv / 16 workgroup partials: within ``C_SUM (w + 2 nv) U |L|^T |A| |Rb|`` of the longdouble value.
    Two runs bitwise equal; with L = Rb = Q (r <= nv, K7's own limit) the result is bitwise K7's: the same template,
    the same grid, the same order of every sum."""
    calA, calE, J, Ad, Ed, opts = _pencil_operator(name)
    nv = calA.shape[0]
    w = int(max(np.diff(calA.tocsr().indptr).max(), np.diff(calE.tocsr().indptr).max(), 1))
    with _lib.Context(0, **opts) as ctx:
        ctx.set_operator(calA, calE, J)
        for r in RANKS:
            rng = np.random.default_rng(7 * nv + r)
            L, Rb = rng.standard_normal((nv, r)), rng.standard_normal((nv, r))
            Ld, Rd = _dev(L), _dev(Rb)
            outs = []
            for _ in range(2):
                Hd = _dev(np.full((2, r, r), np.nan))
                ctx.project_pencil_twosided_dev(Ld.data_ptr(), Rd.data_ptr(), r, Hd[0].data_ptr(), Hd[1].data_ptr())
                outs.append(_host(Hd))
            assert np.array_equal(outs[0], outs[1]), (name, r)
            worst = 0.0
            for H, D in ((outs[0][0], Ad), (outs[0][1], Ed)):
                ref = np.asarray(L.astype(LD).T @ (D.astype(LD) @ Rb.astype(LD)))
                bound = C_SUM * (w + 2 * nv) * U * (np.abs(L).T @ (np.abs(D) @ np.abs(Rb))) + 1e-300
                worst = max(worst, float(np.max(np.abs(H.astype(LD) - ref) / bound)))
            assert np.all(np.isfinite(outs[0])) and worst <= 1.0, (name, r, worst)
            if r <= nv:
                Kd = _dev(np.full((2, r, r), np.nan))
                Hd = _dev(np.full((2, r, r), np.nan))
                ctx.project_pencil_dev(Rd.data_ptr(), r, Kd[0].data_ptr(), Kd[1].data_ptr())
                ctx.project_pencil_twosided_dev(Rd.data_ptr(), Rd.data_ptr(), r, Hd[0].data_ptr(), Hd[1].data_ptr())
                assert np.array_equal(_host(Kd), _host(Hd)), (name, r)          # the same arithmetic: bitwise K7's
            print("%s nv %d r %d: largest error / bound %.3f" % (name, nv, r, worst))


@pytest.mark.parametrize("name", ["nv1", "nv17_np16", "unsym", "arrow200", "fe4"])
def test_twosided_pencil_with_lowrank_term(name):
    """With a low-rank term set, cal A is A - U V^T (q = 3): H_A = L^T A Rb - (L^T U)(Rb^T V)^T, the two small factors
    from the cross-Gram kernel (sums of nv products) and their product a sum of q: the bound of the plain pencil plus
    ``C_SUM (2 nv + q) U (|L|^T |U|)(|Rb|^T |V|)^T``.  H_E is untouched; two runs bitwise equal; with L = Rb = Q the
    result is K7's (which forms Q^T U, Q^T V by its own dense form) to twice that bound."""
    calA, calE, J, Ad, Ed, opts = _pencil_operator(name)
    nv, q = calA.shape[0], 3
    w = int(max(np.diff(calA.tocsr().indptr).max(), np.diff(calE.tocsr().indptr).max(), 1))
    rng = np.random.default_rng(99 + nv)
    Um, Vm = rng.standard_normal((nv, q)), rng.standard_normal((nv, q))
    with _lib.Context(0, **opts) as ctx:
        ctx.set_operator(calA, calE, J)
        ctx.set_lowrank(Um, Vm)
        for r in RANKS:
            L, Rb = rng.standard_normal((nv, r)), rng.standard_normal((nv, r))
            Ld, Rd = _dev(L), _dev(Rb)

            def bound(Lm, D):
                plain = C_SUM * (w + 2 * nv) * U * (np.abs(Lm).T @ (np.abs(D) @ np.abs(Rb))) + 1e-300
                return plain, plain + C_SUM * (2 * nv + q) * U * ((np.abs(Lm).T @ np.abs(Um)) @ (np.abs(Rb).T @ np.abs(Vm)).T)

            outs = []
            for _ in range(2):
                Hd = _dev(np.full((2, r, r), np.nan))
                ctx.project_pencil_twosided_dev(Ld.data_ptr(), Rd.data_ptr(), r, Hd[0].data_ptr(), Hd[1].data_ptr())
                outs.append(_host(Hd))
            assert np.array_equal(outs[0], outs[1]), (name, r)
            Ll, Rl = L.astype(LD), Rb.astype(LD)
            ref_a = np.asarray(Ll.T @ (Ad.astype(LD) @ Rl) - (Ll.T @ Um.astype(LD)) @ (Rl.T @ Vm.astype(LD)).T)
            ref_e = np.asarray(Ll.T @ (Ed.astype(LD) @ Rl))
            worst = max(float(np.max(np.abs(outs[0][0].astype(LD) - ref_a) / bound(L, Ad)[1])),
                        float(np.max(np.abs(outs[0][1].astype(LD) - ref_e) / bound(L, Ed)[0])))
            print("%s nv %d r %d with U V^T: largest error / bound %.3f" % (name, nv, r, worst))
            assert np.all(np.isfinite(outs[0])) and worst <= 1.0, (name, r, worst)
            if r <= nv:
                Kd = _dev(np.full((2, r, r), np.nan))
                Hd = _dev(np.full((2, r, r), np.nan))
                ctx.project_pencil_dev(Rd.data_ptr(), r, Kd[0].data_ptr(), Kd[1].data_ptr())
                ctx.project_pencil_twosided_dev(Rd.data_ptr(), Rd.data_ptr(), r, Hd[0].data_ptr(), Hd[1].data_ptr())
                K7, H2 = _host(Kd), _host(Hd)
                assert np.all(np.abs(K7[0] - H2[0]) <= 2 * bound(Rb, Ad)[1]), (name, r)
                assert np.array_equal(K7[1], H2[1]), (name, r)


# ------------------------------------------------------------------------------------------- 3. balance_factors, N = 8
@pytest.fixture(scope="module")
def factors8():
    """The two Riccati factors of lm.problem(8) from the device's RADI (DeviceFactor) with their downloads."""
    p = lm.problem(8)
    d = dict(ms=p["ms"], radi_res_reltol=1e-12, device_resident=True)
    zc = pru.proj_alg_ric_radi(mmat=p["M"], amat=p["A"], jmat=p["J"], bmat=p["B"], wmat=p["C"].T, radi_dict=d)["zfac"]
    zf = pru.proj_alg_ric_radi(mmat=p["M"], amat=p["A"], jmat=p["J"], bmat=p["C"].T, wmat=p["B"], transposed=True,
                               radi_dict=d)["zfac"]
    return p, zc, zf, zc.numpy(), zf.numpy()


def _balance_bounds(p, zc, zf, mod):
    """Bounds on |device - model| for every output of the balancing step, from the cross-Gram bound.

    S: both the device's and the model's S = Zc^T (M Zf) lie within ``C_SUM (w + nv) U |Zc|^T |M| |Zf|`` of the exact one
    (sums of nv products of sums of at most w products), and each SVD has a backward error of at most ``8 k U sigma_1``
    (k = max(kc, kf)):  ||dS||_2 <= DELTA = 2 (C_SUM (w + nv) U || |Zc|^T |M| |Zf| ||_F + 8 k U sigma_1).
    sigma_i: within DELTA (Weyl).
    Singular vectors (up to a common sign of u_i and v_i): ||du_i||, ||dv_i|| <= 2 DELTA / (g_i - DELTA), g_i the
    distance of sigma_i to the other singular values and to zero (Wedin's sin-theta theorem, 2 sin(theta / 2) <=
    sqrt(2) sin(theta)).  Column i of T_l = Zc u_i sigma_i^-1/2 then moves by at most
        e_l[i] = ||Zc||_2 (||du_i|| + DELTA / (2 (sigma_i - DELTA)) + 2 (kc + 2) sqrt(kc) U) / sqrt(sigma_i - DELTA)
    -- the last term the rounding of the two products Zc coef_i, | |Zc| |_2 <= sqrt(kc) ||Zc||_2; this is where
    sigma_1 / sigma_r enters: DELTA is relative to sigma_1, the divisions are by gaps and values down to sigma_r --
    and likewise e_r[i].  An entry of a projected matrix t_l,i^T A t_r,j moves by at most
        e_l[i] ||A t_r,j|| + ||A^T t_l,i|| e_r[j] + e_l[i] ||A||_2 e_r[j] + C_SUM (w + 2 nv) U |t_l,i|^T |A| |t_r,j|,
    the last term the kernels' own rounding (tests 1 and 2); B_r and C_r the same with one basis.

    These are a-priori bounds and as wide as such bounds are: at N = 8, tol = 1e-6 the column bounds reach 3.5e-4 of
    the column's norm for the last columns and the bound of an entry of A_r reaches 57 where max |A_r| is 1198 (the
    errors measured on the device are about 1e-3 of the bounds).  A column whose gap is at most DELTA has no finite
    bound; the comparison asserts that there is none (all r columns are bounded for the cases run)."""
    M, A, B, C = p["M"], p["A"], p["B"], p["C"]
    nv, k = zc.shape[0], max(zc.shape[1], zf.shape[1])
    w = int(max(np.diff(M.indptr).max(), np.diff(A.indptr).max()))
    r, sig = mod["order"], mod["hsv"]
    abs_s = np.abs(zc).T @ (abs(M) @ np.abs(zf))
    delta = 2 * (C_SUM * (w + nv) * U * np.linalg.norm(abs_s) + 8 * k * U * sig[0])
    full = np.concatenate([sig, [0.0]])
    gap = np.array([np.min(np.abs(np.delete(full, i) - sig[i])) for i in range(r)])
    with np.errstate(divide="ignore", invalid="ignore"):
        dvec = np.where(gap > delta, 2 * delta / (gap - delta), np.inf)
        scale = np.where(sig[:r] > delta, 1.0 / np.sqrt(sig[:r] - delta), np.inf)
        dsq = np.where(sig[:r] > delta, delta / (2 * (sig[:r] - delta)), np.inf)
    tl, tr = mod["tl"], mod["tr"]
    e_l = np.linalg.norm(zc, 2) * scale * (dvec + dsq + 2 * (zc.shape[1] + 2) * U * np.sqrt(zc.shape[1]))
    e_r = np.linalg.norm(zf, 2) * scale * (dvec + dsq + 2 * (zf.shape[1] + 2) * U * np.sqrt(zf.shape[1]))

    def two(D):
        Dd = D.toarray()
        left, right = np.linalg.norm(Dd.T @ tl, axis=0), np.linalg.norm(Dd @ tr, axis=0)
        return e_l[:, None] * right[None, :] + left[:, None] * e_r[None, :] + \
            np.linalg.norm(Dd, 2) * e_l[:, None] * e_r[None, :] + \
            C_SUM * (w + 2 * nv) * U * (np.abs(tl).T @ (np.abs(Dd) @ np.abs(tr)))

    b_br = e_l[:, None] * np.linalg.norm(B, axis=0)[None, :] + C_SUM * nv * U * (np.abs(tl).T @ np.abs(B))
    b_cr = np.linalg.norm(C, axis=1)[:, None] * e_r[None, :] + C_SUM * nv * U * (np.abs(C) @ np.abs(tr))
    return dict(delta=delta, e_l=e_l, e_r=e_r, ar=two(A), er=two(M), br=b_br, cr=b_cr)


def _compare_with_model(p, zc, zf, out, tol, order):
    mod = lm.balance(p["M"], p["A"], p["B"], p["C"], zc, zf, tol=tol, order=order)
    bd = _balance_bounds(p, zc, zf, mod)
    r = mod["order"]
    # the truncation is decided away from the threshold, so the model's r is THE r
    assert np.all(np.abs(mod["hsv"] - tol * mod["hsv"][0]) > bd["delta"])
    assert out["order"] == r
    assert np.max(np.abs(out["hsv"] - mod["hsv"])) <= bd["delta"]
    tl, tr = np.asarray(out["tl"]), np.asarray(out["tr"])
    assert tl.shape == tr.shape == (zc.shape[0], r)
    # common sign of column i of T_l and T_r: the model's
    sgn = np.sign(np.sum(tl * mod["tl"], axis=0))
    sgn[sgn == 0] = 1.0
    ratios = dict(
        tl=np.max(np.linalg.norm(tl * sgn - mod["tl"], axis=0) / bd["e_l"]),
        tr=np.max(np.linalg.norm(tr * sgn - mod["tr"], axis=0) / bd["e_r"]),
        ar=np.max(np.abs(sgn[:, None] * out["ar"] * sgn[None, :] - mod["ar"]) / bd["ar"]),
        er=np.max(np.abs(sgn[:, None] * out["er"] * sgn[None, :] - mod["er"]) / bd["er"]),
        br=np.max(np.abs(sgn[:, None] * out["br"] - mod["br"]) / bd["br"]),
        cr=np.max(np.abs(out["cr"] * sgn[None, :] - mod["cr"]) / bd["cr"]))
    finite = int(np.count_nonzero(np.isfinite(bd["e_l"])))
    print("tol %g order %s: r %d, DELTA %.3e, |dsigma| %.3e, columns with a finite bound %d, error / bound: %s" %
          (tol, order, r, bd["delta"], np.max(np.abs(out["hsv"] - mod["hsv"])), finite,
           "  ".join("%s %.3g" % kv for kv in ratios.items())))
    assert finite == r, "a column without a finite bound would pass unchecked"
    assert all(np.isfinite(np.asarray(out[key])).all() for key in ("tl", "tr", "ar", "er", "br", "cr"))
    assert max(ratios.values()) <= 1.0, ratios
    # T_l^T M T_r = I_r, of the device's own bases, to the CPU test's bound
    d_s = bd["delta"] / 2
    defect = np.linalg.norm(tl.T @ (p["M"] @ tr) - np.eye(r))
    assert defect <= 2 * d_s / mod["hsv"][r - 1] and np.linalg.norm(out["er"] - np.eye(r)) <= 2 * d_s / mod["hsv"][r - 1]
    return mod


@pytest.mark.parametrize("tol,order", [(1e-6, None), (1e-3, None), (1e-6, 1), (1e-6, 7)])
def test_balance_factors_against_model(factors8, tol, order):
    """Every output against the NumPy model on the same factors (bounds: _balance_bounds), T_l^T M T_r = I_r; DeviceFactor
    and ndarray inputs give bitwise the same; the context's RADI settings are untouched.  (1e-3, None) is a ``tol`` that
    truncates well above the factors' own accuracy, (1e-6, 1) is ``order=1``."""
    p, zcd, zfd, zc, zf = factors8
    ctx = backend.context()
    before = lqgbt._context_settings(ctx)
    out = lqgbt.balance_factors(p["M"], p["A"], p["J"], zcd, zfd, p["B"], p["C"], tol=tol, order=order)
    assert isinstance(out["tl"], pru.DeviceFactor) and isinstance(out["tr"], pru.DeviceFactor)
    mod = _compare_with_model(p, zc, zf, out, tol, order)
    assert order is None or out["order"] == min(order, lm.truncation_order(mod["hsv"], tol))
    host = lqgbt.balance_factors(p["M"], p["A"], p["J"], zc, zf, p["B"], p["C"], tol=tol, order=order)
    assert isinstance(host["tl"], np.ndarray)
    for key in ("hsv", "tl", "tr", "ar", "er", "br", "cr"):
        assert np.array_equal(np.asarray(out[key]), np.asarray(host[key])), key
    assert lqgbt._context_settings(ctx) == before


def test_balance_factors_wide_factor_is_compressed(factors8):
    """A factor of more than 1024 columns goes through the library's compression first: [Zc, 0.5 Zc, ...] repeated to
    1100 columns has the Gramian (sum of the squared weights) Zc Zc^T, so sigma scales by that sum's root."""
    p, _, zfd, zc, zf = factors8
    reps = -(-1100 // zc.shape[1])
    wts = 0.5 ** np.arange(reps)
    wide = np.hstack([wt * zc for wt in wts])
    assert wide.shape[1] > lqgbt.MAX_COLS
    out = lqgbt.balance_factors(p["M"], p["A"], p["J"], wide, zfd, p["B"], p["C"], tol=1e-6)
    ref = lm.balance(p["M"], p["A"], p["B"], p["C"], zc, zf, tol=1e-6)["hsv"] * np.sqrt(np.sum(wts ** 2))
    # the compression drops singular values of the factor below 0.1 tol ||Z||_2: an error of that size relative to sigma_1
    assert lm.sigma_distance(out["hsv"], ref, floor=1e-4) <= 1e-3


def test_balance_factors_argument_contract(factors8):
    p, zcd, zfd, _, _ = factors8
    for order in (0, 129):
        with pytest.raises(ValueError):
            lqgbt.balance_factors(p["M"], p["A"], p["J"], zcd, zfd, p["B"], p["C"], order=order)
    with pytest.raises(ValueError):
        lqgbt.balance_factors(p["M"], p["A"], p["J"], zcd, zfd, p["B"], p["C"], tol=1.0)
    with pytest.raises(ValueError):
        lqgbt.balance_factors(p["M"], p["A"], p["J"], zcd, zfd, p["B"][:-1], p["C"])


# ------------------------------------------------------------------------------------------- 4. end to end, N = 8
def _end_to_end(kind, **kw):
    p = lm.problem(8)
    ctx = backend.context()
    before = lqgbt._context_settings(ctx)
    out = lqgbt.lqgbt_reduce(p["M"], p["A"], p["J"], p["B"], p["C"], tol=1e-10, return_factors=True, **kw)
    assert lqgbt._context_settings(ctx) == before
    dist = lm.sigma_distance(out["hsv"], lm.dense_sigma(8, kind))
    print("%s %s: r %d, kc %d, kf %d, sigma distance from the dense route %.3e (recorded CPU distance %.3e)" %
          (kind, kw, out["order"], out["zc"].shape[1], out["zf"].shape[1], dist, lm.SIGMA_DIST_N8))
    assert dist <= 10 * lm.SIGMA_DIST_N8
    return p, out


@pytest.mark.parametrize("solver,opts", [("radi", dict(ms="hamiltonian-sweep")),
                                         ("newtonadi", dict(pb.default_nwtn_adi_dict(), ms="from-problem"))])
def test_lqgbt_reduce_end_to_end(solver, opts):
    """sigma against the dense route within ten times the CPU-recorded distance (lm.SIGMA_DIST_N8; the margin covers the
    other shifts and stopping points of the device's solves); the reduced-residual checks of the CPU test
    (lm.reduced_residual_check) on the device's own factors; the controller's shapes."""
    if opts.get("ms") == "from-problem":
        opts = dict(opts, ms=lm.problem(8)["ms"])
    p, out = _end_to_end("riccati", ric_solver=solver, radi_dict=opts)
    zc, zf = out["zc"].numpy(), out["zf"].numpy()
    ds = lm.Dense(p["M"], p["A"], p["J"], p["B"], p["C"])
    lm.assert_reduced_residuals(ds, out, zc, zf, solver)
    r = out["order"]
    assert out["ak"].shape == (r, r) and out["bk"].shape == (r, p["C"].shape[0]) and out["ck"].shape == (p["B"].shape[1], r)
    ak, bk, ck = lm.controller(out)
    assert np.array_equal(out["ak"], ak) and np.array_equal(out["bk"], bk) and np.array_equal(out["ck"], ck)
    assert "zfac" not in out["info_c"] and "zfac" not in out["info_f"]


def test_lqgbt_reduce_lyapunov_gramians():
    """``gramians='lyapunov'``: the Hankel singular values against sqrt(eig(P M^T Q M)) from dense Lyapunov solves, by
    the same rule; no controller."""
    d = dict(pb.default_nwtn_adi_dict(), ms=lm.problem(8)["ms"])
    _, out = _end_to_end("lyapunov", gramians="lyapunov", radi_dict=d)
    assert "ak" not in out and "bk" not in out and "ck" not in out
