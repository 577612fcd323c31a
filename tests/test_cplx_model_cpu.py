"""CPU tests of the complex-shift path's model (tests/cplx_model.py) and of what the library answers without a GPU
(DESIGN.md section 3f).  The GPU tests (tests/test_gpu_cplx.py) compare the device with this model, so the model is
held to dense references and to its identities here.  Sections 6 and 7: the model of the GMRES cycle against
``np.linalg.qr`` / ``np.linalg.lstsq``, a float64 twin of every kernel of the cycle (same operation order) through the
cycles of tests/test_gpu_cplx_steps.py -- it has to stay inside HALF of every bound --, and six faults injected into the
twin, each of which has to break a bound at those shapes."""
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
    """The library loads without a GPU, and the three device entries and the four of the step probe return
    RICADI_ESTATE for a missing context / operator before they look at anything else."""
    lib = _lib.load()
    one = (C.c_double * 1)(-1.0)
    assert lib.ricadi_shift_solve_cplx_batch_dev(None, 1, one, one, one, None, 0, 1, None, None, None) == -5
    assert lib.ricadi_op_apply_cplx_batch_dev(None, 1, one, one, one, None, 0, 1, None, 0, None, 0, None) == -5
    assert lib.ricadi_cplx_orth_dev(None, 1, 1, 1, None, 0, 0, None, None) == -5
    assert b"operator" in lib.ricadi_last_error()
    assert lib.ricadi_cplx_probe_begin_dev(None, 1, 1, None, None) == -5
    assert lib.ricadi_cplx_probe_step_dev(None, 0, None, 1, None) == -5
    assert lib.ricadi_cplx_probe_close_dev(None, None, 1, None, None) == -5
    assert lib.ricadi_cplx_probe_read_dev(None, 0, 0, None, 0, None) == -5


# ------------------------------------------------------------------------------------------------ 6. the cycle's model
def _hessenberg(rng, k, scale=1.0):
    H = np.triu(rng.standard_normal((k + 1, k)) + 1j * rng.standard_normal((k + 1, k)), -1) * scale
    H[np.arange(1, k + 1), np.arange(k)] = np.abs(H[np.arange(1, k + 1), np.arange(k)])      # real subdiagonal
    return H + 3.0 * np.eye(k + 1, k)


@pytest.mark.parametrize("k", [1, 2, 7, 10])
def test_model_rotations_against_qr_and_lstsq(k):
    """The model's rotations triangularise the Hessenberg matrix as ``np.linalg.qr`` does -- R agrees up to a phase
    per row (the phases of Q's columns), ``R^H R = H^H H`` --, and its back substitution and residual norm are
    ``np.linalg.lstsq``'s minimiser and residual: ``|gv[k]|`` is the least-squares residual.  Tolerances: 200 eps of the
    quantity's scale (float64 references; condition numbers below 10)."""
    rng = np.random.default_rng(60 + k)
    H = _hessenberg(rng, k, 0.3)
    beta = 1.7
    y, rn, R, g = cm.hessenberg_ls(H, beta)
    R, y, g = R.astype(np.complex128), y.astype(np.complex128), g.astype(np.complex128)
    Rq = np.linalg.qr(H)[1]
    ph = (np.diag(R) / np.abs(np.diag(R))) / (np.diag(Rq) / np.abs(np.diag(Rq)))
    tol = 200 * cm.EPS
    assert np.max(np.abs(R - ph[:, None] * Rq)) <= tol * np.linalg.norm(H)
    assert np.allclose(np.tril(R, -1), 0.0)
    assert np.max(np.abs(R.conj().T @ R - H.conj().T @ H)) <= tol * np.linalg.norm(H) ** 2
    e1 = np.zeros(k + 1, dtype=np.complex128)
    e1[0] = beta
    yl = np.linalg.lstsq(H, e1, rcond=None)[0]
    assert np.linalg.cond(H) < 10
    assert np.max(np.abs(y - yl)) <= tol * np.linalg.norm(yl)
    assert abs(float(rn) - np.linalg.norm(e1 - H @ yl)) <= tol * beta
    assert abs(float(rn) - abs(g[k])) <= tol * beta and abs(np.linalg.norm(g) - beta) <= tol * beta


def test_model_exact_branches_and_vanished_pivot():
    """``r == 0``: c = 1, s = d = 0; ``|cur| == 0 < b``: c = 0, s = 1, d = b; general: G applied to (cur, b) gives
    (d, 0) with |d| = r.  A vanished pivot gives ``y_i = 0`` and the other unknowns are those of the remaining rows."""
    z = cm.hess_column([0.0, 0.0], [], [])
    assert (z["branch"], z["c"], z["s"], z["col"][0]) == ("zero", 1, 0, 0)
    b = cm.hess_column([0.0, 2.5], [], [])
    assert (b["branch"], b["c"], b["s"], b["col"][0]) == ("breakdown", 0, 1, 2.5)
    g = cm.hess_column([3.0 - 4.0j, 12.0], [], [])
    assert g["branch"] == "general" and abs(abs(g["col"][0]) - 13) <= 1e-17 and abs(g["rho"] - np.longdouble(13) / 5) <= 1e-17
    c, s, cur = g["c"], g["s"], np.clongdouble(3.0 - 4.0j)
    assert abs(c * cur + s * 12 - g["col"][0]) <= 1e-17 and abs(-np.conj(s) * cur + c * 12) <= 1e-17
    assert abs(c * c + abs(s) ** 2 - 1) <= 1e-18 and c.imag == 0
    # the second rotation of a breakdown column swaps the two leading coefficients
    sw = cm.hess_column([1.0 + 2.0j, 3.0 - 1.0j, 0.5], [0.0], [1.0])
    assert sw["col"][0] == 3.0 - 1.0j and abs(abs(sw["col"][1]) - np.hypot(abs(1 + 2j), 0.5)) <= 1e-15
    R = np.array([[2.0, 1.0j, 3.0], [0.0, 0.0, 1.0], [0.0, 0.0, 4.0j]])
    y = cm.back_substitute(R, np.array([1.0, 5.0, 8.0])).astype(np.complex128)
    assert y[1] == 0 and y[2] == 8.0 / 4.0j and abs(y[0] - (1.0 - 3.0 * y[2]) / 2.0) <= 1e-16
    assert cm.backsolve_ratio(R, np.array([1.0, 5.0, 8.0]), y) <= 1.0
    with pytest.raises(AssertionError):
        cm.backsolve_ratio(R, np.array([1.0, 5.0, 8.0]), y + np.array([0.0, 1.0, 0.0]))
    assert cm.gv_update(2.0j, 0.6, 0.8j) == (np.clongdouble(0.6) * 2.0j, -np.conj(np.clongdouble(0.8j)) * 2.0j)


# ------------------------------------------------------------------------------------------------ 7. the float64 twin
FAULTS = ("rot_conj", "gv_conj", "back_conj", "corr_sign", "dots_chunk", "tail48")


def _split(a):
    return np.ascontiguousarray(a.real), np.ascontiguousarray(a.imag)


def twin_dots(V, w, fault=None):
    """``v_j^H w`` per column as cplx_dots_kernel + cplx_reduce_kernel sum it: per 128-row block and row slot s the rows
    s, s + 16, ... one after the other, the slots of a wave pairwise twice, the four waves, then the blocks, the basis
    vectors in chunks of 32 (a chunk changes nothing in the arithmetic; the fault ``dots_chunk`` makes every chunk
    after the first read the first chunk's vectors).  V (nvec, n, mc), w (n, mc) complex; float64 products and sums."""
    nvec, n, mc = V.shape
    nblk = max(1, -(-n // 128))
    pad = nblk * 128 - n

    def tile(a):                                           # (.., n, mc) -> (.., nblk, 8, 16, mc): row = 128 b + 16 i + s
        a = np.concatenate([a, np.zeros(a.shape[:-2] + (pad, mc))], axis=-2)
        return a.reshape(a.shape[:-2] + (nblk, 8, 16, mc))

    if fault == "dots_chunk":
        V = V[np.where(np.arange(nvec) >= 32, np.arange(nvec) % 32, np.arange(nvec))]
    vr, vi = (tile(x) for x in _split(V))
    wr, wi = (tile(x) for x in _split(w))
    re = np.zeros((nvec, nblk, 16, mc))
    im = np.zeros((nvec, nblk, 16, mc))
    for i in range(8):
        re = (re + vi[:, :, i] * wi[:, i]) + vr[:, :, i] * wr[:, i]
        im = (im - vi[:, :, i] * wr[:, i]) + vr[:, :, i] * wi[:, i]
    out = []
    for acc in (re, im):
        acc = acc.reshape(nvec, nblk, 4, 2, 2, mc)                     # wave, pair, slot
        acc = acc[:, :, :, :, 0] + acc[:, :, :, :, 1]
        acc = acc[:, :, :, 0] + acc[:, :, :, 1]
        acc = ((acc[:, :, 0] + acc[:, :, 1]) + acc[:, :, 2]) + acc[:, :, 3]
        tot = np.zeros((nvec, mc))
        for b in range(nblk):
            tot = tot + acc[:, b]
        out.append(tot)
    return out[0] + 1j * out[1]


def twin_update(V, h, w, sign, nvec, fault=None):
    """``w += sign sum_{j < nvec} v_j h_j`` as cplx_update_kernel: the sum over j first, one addition to w."""
    ar, ai = np.zeros(w.shape), np.zeros(w.shape)
    flip = -1.0 if (fault == "corr_sign" and sign > 0) else 1.0
    for j in range(nvec):
        hr, hi = h[j].real, flip * h[j].imag
        ar = (ar + (-hi) * V[j].imag) + hr * V[j].real
        ai = (ai + hi * V[j].real) + hr * V[j].imag
    return (w.real + sign * ar) + 1j * (w.imag + sign * ai)


def twin_cgs2(V, w, fault=None):
    """One CGS2 step as cplx_orth issues it: (h (nvec + 1, mc), unit vector, nrm2, scale)."""
    nvec = V.shape[0]
    hs = []
    for _ in range(2):
        h = twin_dots(V, w, fault)
        w = twin_update(V, h, w, -1.0, nvec)
        hs.append(h)
    nrm2 = twin_dots(w[None], w).real[0]
    nn = np.sqrt(nrm2)
    scale = np.where(nn > 0, 1.0 / np.where(nn > 0, nn, 1.0), 0.0)
    h = np.concatenate([hs[0] + hs[1], nn[None].astype(np.complex128)])
    return h, (w.view(np.float64) * np.repeat(scale, 2)).view(np.complex128), nrm2, scale


def _cmul(a, b):
    return complex(a.real * b.real - a.imag * b.imag, a.real * b.imag + a.imag * b.real)


class Float64Twin:
    """The complex cycle in float64 with the kernels' operation order (plain NumPy and Python scalars) behind the
    interface cplx_model.check_cycle drives; ``fault``: one of FAULTS or None."""

    def __init__(self, n, restart, fault=None):
        assert fault is None or fault in FAULTS
        self.n, self.rs, self.fault = n, restart, fault

    def begin(self, R, bnorm):
        ng, n, mc = R.shape
        rs = self.rs
        nanc = lambda *s: np.full(s, np.nan + 1j * np.nan)               # noqa: E731
        nanr = lambda *s: np.full(s, np.nan)                             # noqa: E731
        self.ng, self.mc, self.bnorm = ng, mc, np.array(bnorm)
        self.a = dict(hout=nanc(ng, rs + 2, 8), Hm=nanc(ng, 8, rs, rs + 1), cs=nanr(ng, 8, rs), sn=nanc(ng, 8, rs),
                      gv=nanc(ng, 8, rs + 1), y=nanc(ng, rs, 8), scale=nanr(ng, 16), resid=nanr(ng, 8),
                      nrm2=np.zeros((ng, 16)))
        self.V = nanc(rs + 1, ng, n, mc)
        for g in range(ng):
            nrm2 = twin_dots(R[g][None], R[g]).real[0]
            nn, scale, resid = cm.cycle_start(nrm2, bnorm[g])
            self.a["nrm2"][g, 0:2 * mc:2] = nrm2
            self.a["gv"][g, :mc, 0] = nn
            self.a["scale"][g, 0:2 * mc:2] = self.a["scale"][g, 1:2 * mc:2] = scale
            self.a["resid"][g, :mc] = resid
            self.V[0, g] = (R[g].view(np.float64) * np.repeat(scale, 2)).view(np.complex128)

    def step(self, j, W, groups):
        a, mc = self.a, self.mc
        for g in groups:
            h, unit, nrm2, scale = twin_cgs2(self.V[:j + 1, g], W[g].copy())
            a["hout"][g, :j + 2], a["scale"][g] = 0.0, 0.0              # (whole rows of 16 lanes are written)
            a["hout"][g, :j + 2, :mc] = h
            a["nrm2"][g, 0:2 * mc:2] = nrm2
            a["scale"][g, 0:2 * mc:2] = a["scale"][g, 1:2 * mc:2] = scale
            self.V[j + 1, g] = unit
            for c in range(mc):
                self._hess(g, c, j, [complex(x) for x in h[:, c]])

    def _hess(self, g, c, j, hc):
        a = self.a
        cur = hc[0]
        for i in range(j):
            nxt, ci, si = hc[i + 1], float(a["cs"][g, c, i]), complex(a["sn"][g, c, i])
            sn_nxt = _cmul(si, nxt)
            sc_cur = _cmul(si if self.fault == "rot_conj" else si.conjugate(), cur)
            a["Hm"][g, c, j, i] = complex(ci * cur.real + sn_nxt.real, ci * cur.imag + sn_nxt.imag)
            cur = complex(ci * nxt.real - sc_cur.real, ci * nxt.imag - sc_cur.imag)
        b = hc[j + 1].real
        na = float(np.hypot(cur.real, cur.imag))
        r = float(np.hypot(na, b))
        if r == 0.0:
            cj, sj, d = 1.0, 0j, 0j
        elif na == 0.0:
            cj, sj, d = 0.0, 1.0 + 0j, complex(b)
        else:
            cj, f, e = na / r, b / (na * r), r / na
            sj, d = complex(cur.real * f, cur.imag * f), complex(cur.real * e, cur.imag * e)
        a["Hm"][g, c, j, j], a["Hm"][g, c, j, j + 1] = d, 0.0
        a["cs"][g, c, j], a["sn"][g, c, j] = cj, sj
        gj = complex(a["gv"][g, c, j])
        gn = _cmul(sj if self.fault == "gv_conj" else sj.conjugate(), gj)
        a["gv"][g, c, j + 1] = complex(-gn.real, -gn.imag)
        a["gv"][g, c, j] = complex(cj * gj.real, cj * gj.imag)
        bn = self.bnorm[g, c]
        a["resid"][g, c] = float(np.hypot(gn.real, gn.imag)) / bn if bn > 0.0 else 0.0

    def close(self, ks, Z, X):
        a, mc = self.a, self.mc
        for g in range(self.ng):
            k = ks[g]
            for c in range(mc):
                for i in range(k - 1, -1, -1):
                    s = complex(a["gv"][g, c, i])
                    for l in range(i + 1, k):
                        p = _cmul(complex(a["Hm"][g, c, l, i]), complex(a["y"][g, l, c]))
                        s = complex(s.real - p.real, s.imag - p.imag)
                    d = complex(a["Hm"][g, c, i, i])
                    dd = d.real * d.real + d.imag * d.imag
                    yi = 0j
                    if dd > 0.0:
                        q = _cmul(s, d if self.fault == "back_conj" else d.conjugate())
                        yi = complex(q.real / dd, q.imag / dd)
                    a["y"][g, i, c] = yi
            X[g] = twin_update(Z[:, g], a["y"][g, :, :mc], X[g], 1.0, k, self.fault)
        return X

    def read(self, what, slot=0):
        return self.V[slot].copy() if what == "V" else self.a[what].copy()


TWIN_WORST = {}


@pytest.mark.parametrize("case", cm.CYCLE_CASES, ids=[c["name"] for c in cm.CYCLE_CASES])
def test_float64_twin_meets_every_bound(case):
    """The twin through the cycles of the GPU tests, at their shapes: every quantity within HALF its bound (a ratio
    above 0.5 would say that the rounding count behind a constant is wrong), all structural checks of check_cycle."""
    rep = cm.run_case(Float64Twin(case["n"], case["restart"]), case)
    print("%s: error / bound %s" % (case["name"], {k: float("%.3g" % v) for k, v in rep.items()}))
    for k, v in rep.items():
        TWIN_WORST[k] = max(TWIN_WORST.get(k, 0.0), v)
    assert all(v <= 0.5 for v in rep.values()), {k: v for k, v in rep.items() if v > 0.5}
    assert set(rep) == set(cm.QUANTITIES) and len(rep.closes) == len(case["ks_list"])
    assert rep.branches == ({"general", "zero", "breakdown"} if case["breakdowns"] else {"general"})


@pytest.mark.parametrize("fault,quantity", [("rot_conj", "rotated column"), ("gv_conj", "gv"),
                                            ("back_conj", "back-solve residual"), ("corr_sign", "correction")])
def test_cycle_faults_break_a_bound(fault, quantity):
    """Each fault, injected into the twin, misses the bound of the quantity it spoils at n = 130, mc = 3 (and the twin
    without it does not: the case above)."""
    case = next(c for c in cm.CYCLE_CASES if c["name"] == "n130-mc3-restart10")
    rep = cm.run_case(Float64Twin(case["n"], case["restart"], fault), case)
    print("%s: %s error / bound %.3g" % (fault, quantity, rep[quantity]))
    assert rep[quantity] > 1.0 and not rep.ok()


@pytest.mark.parametrize("nvec", [33, 60])
def test_second_chunk_fault_breaks_the_coefficient_bound(nvec):
    """A dot pass whose second 32-vector chunk reads the first chunk's vectors misses ``cgs2_coef_bound`` at n = 61
    (the shape of the GPU test); the twin without the fault stays inside half of it."""
    n, mc = 61, 3
    rng = np.random.default_rng(70 + nvec)
    V = np.zeros((nvec, n, mc), dtype=np.complex128)
    for c in range(mc):
        V[:, :, c] = np.linalg.qr(rng.standard_normal((n, nvec)) + 1j * rng.standard_normal((n, nvec)))[0].T
    w = rng.standard_normal((n, mc)) + 1j * rng.standard_normal((n, mc))
    exact, bound = cm.cgs2_coef_bound(V, w)
    good = float(np.max(np.abs(twin_cgs2(V, w.copy())[0][:nvec] - exact) / bound))
    bad = float(np.max(np.abs(twin_cgs2(V, w.copy(), "dots_chunk")[0][:nvec] - exact) / bound))
    print("nvec %d: coefficients error / bound %.3g, with the chunk fault %.3g" % (nvec, good, bad))
    TWIN_WORST["CGS2 coefficients at nvec > 32"] = max(TWIN_WORST.get("CGS2 coefficients at nvec > 32", 0.0), good)
    assert good <= 0.5 and bad > 1.0


def twin_product(tiles, alpha, beta, X, fault=None):
    """``S(alpha, beta) X`` row by row, entry by entry in the saddle CSR order, with the kernels' two fused terms per
    entry (float64); the fault ``tail48`` drops the entries past 48 of a row."""
    rp, ci = tiles["s_rp"], tiles["s_ci"]
    re = alpha.real * tiles["src_e"] + beta * tiles["src_a"] + tiles["src_j"]
    im = alpha.imag * tiles["src_e"]
    Y = np.zeros((tiles["n"], X.shape[1]), dtype=np.complex128)
    for row in range(tiles["n"]):
        k1 = min(rp[row + 1], rp[row] + 48) if fault == "tail48" else rp[row + 1]
        ar, ai = np.zeros(X.shape[1]), np.zeros(X.shape[1])
        for k in range(rp[row], k1):
            x = X[ci[k]]
            ar = (ar + re[k] * x.real) - im[k] * x.imag
            ai = (ai + re[k] * x.imag) + im[k] * x.real
        Y[row] = ar + 1j * ai
    return Y


def test_product_twin_on_long_rows_and_the_dropped_tail():
    """On the long-row operator (tiled form, longest row 100, rows of exactly 48 and 49 entries) the float64 product
    stays inside half the product bound; without the entries past 48 of a row it misses it."""
    ops, rows = cm.long_row_operator()
    tiles = _lib.host_saddle_tiles(*ops)
    lens = np.diff(tiles["s_rp"])
    assert tiles["ms_ok"] and tiles["n"] == 1937 and lens.max() == 100 and 48 in lens and 49 in lens
    rng = np.random.default_rng(48)
    X = rng.standard_normal((1937, 2)) + 1j * rng.standard_normal((1937, 2))
    worst = {}
    for alpha, beta in ((-30 + 30j, 1.0), (-1e3 - 300j, 0.5)):
        ref, bound = cm.product(ops, alpha, beta, X)
        for fault in (None, "tail48"):
            err = np.abs(twin_product(tiles, alpha, beta, X, fault) - ref) / bound
            worst[fault] = max(worst.get(fault, 0.0), float(err.max()))
            if fault:
                # (only rows longer than 48 miss it; a row whose entries past 48 are stored zeros of J^T does not)
                bad = set(np.flatnonzero(err.max(axis=1) > 1.0))
                assert bad <= set(np.flatnonzero(lens > 48)) and {rows[2], rows[3]} <= bad, (alpha, bad)
    print("long rows: product error / bound %.3g, without the tails %.3g" % (worst[None], worst["tail48"]))
    TWIN_WORST["product on long rows"] = worst[None]
    assert worst[None] <= 0.5 and worst["tail48"] > 1.0


def test_float64_twin_summary():
    """(prints the largest error / bound per quantity over the twin's cases above: the CPU column of DESIGN.md 3f)"""
    assert TWIN_WORST, "the twin cases of this module did not run in this session"
    for k, v in TWIN_WORST.items():
        print("  %-32s %.3g" % (k, v))
