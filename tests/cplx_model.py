"""NumPy / SciPy FP64 model of the complex-shift path (ricadi_cplx.hip, solver_cplx.inl):

* the complex saddle product ``y = S(alpha, beta) x``, ``S(a, b) = [[b calA + a calE, J^T], [J, 0]]`` with complex
  ``alpha``, and the entrywise bound the device forms are held to (:func:`product`);
* one CGS2 step against an orthonormal complex basis and the bound on its coefficients (:func:`cgs2_step`,
  :func:`cgs2_coef_bound`);
* the restart cycle unit by unit in extended precision -- cycle start, one Hessenberg column through the rotations,
  the update of ``gv``, the residual estimate, the back substitution, the correction -- with their counted bounds, and
  the driver that holds a device (the step probe, or a float64 twin) to them (:func:`hess_column` ...,
  :func:`check_cycle`);
* right-preconditioned flexible GMRES(restart) with complex (or, on real input, real) inner products and a given
  preconditioner callable (:func:`fgmres`), and the real-equivalent 2n x 2n form (:func:`real_equivalent`);
* the proxy rule of the preconditioner's real shift (:func:`proxy`);
* the dense transfer function through the saddle matrix and through an orthonormal basis of ker J, and square-root
  balanced truncation from dense Gramians (:func:`transfer_saddle`, :func:`transfer_projected`, :func:`dense_bt`).

Product bound, per entry of an output, eps = 2^-52, k the stored length of the entry's saddle row:

    |y - ref| <= C (k + 2) eps ((|beta| |calA| + |alpha| |calE| + |J|-part) |x|),   C = C_CPLX = 4,

with moduli throughout.  It is ``saddle_model``'s bound with 4 in place of 2: forming the complex coefficient
``(beta vA + ar vE) + i (ai vE)`` costs two roundings on the real and one on the imaginary part, and a complex multiply
accumulated as two real fused terms per part is within ``sqrt(2) gamma_2`` of the exact product (Higham, Accuracy and
Stability, section 3.6) -- at most five roundings per term against the two of the real kernels' bound.  Derived, not
measured.
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sps

import saddle_model as sm

C_CPLX = 4.0
EPS = np.finfo(np.float64).eps

# the shifts the issue's CPU experiment used (all with Re alpha <= 0)
SHIFTS7 = (-0.1j, -1j, -30j, -1e3j, -1 - 1j, -30 + 30j, -1e3 - 300j)


# ------------------------------------------------------------------------------------------------ proxy rule
def proxy(alpha):
    """``-2^round(log2 |alpha|)`` (halves rounded up): the real shift the preconditioner is applied at."""
    a = complex(alpha)
    if not (np.isfinite(a.real) and np.isfinite(a.imag)) or a.real > 0 or a == 0:
        raise ValueError("a finite shift alpha != 0 with Re alpha <= 0 required")
    return -float(2.0 ** np.floor(np.log2(abs(a)) + 0.5))


# ------------------------------------------------------------------------------------------------ product
def saddle_cplx(calA, calE, J, alpha, beta=1.0):
    """S(alpha, beta) as a complex SciPy CSR."""
    vv = (beta * sps.csr_matrix(calA)).astype(np.complex128) + complex(alpha) * sps.csr_matrix(calE)
    if J.shape[0] == 0:
        return sps.csr_matrix(vv)
    Jc = sps.csr_matrix(J).astype(np.complex128)
    return sps.bmat([[vv, Jc.T], [Jc, None]], format="csr")


def product(ops, alpha, beta, X):
    """(ref, bound) of ``S(alpha, beta) X`` for a complex n x mc panel X."""
    calA, calE, J = ops
    ref = saddle_cplx(calA, calE, J, alpha, beta) @ X
    if J.shape[0] == 0:
        mag = (abs(beta) * abs(sps.csr_matrix(calA)) + abs(complex(alpha)) * abs(sps.csr_matrix(calE))) @ np.abs(X)
        k = np.diff((sm._pattern(calA) + sm._pattern(calE)).tocsr().indptr)[:, None].astype(np.float64)
    else:
        mag = sm.saddle_abs(calA, calE, J, abs(complex(alpha)), beta) @ np.abs(X)
        k = sm.row_lengths(calA, calE, J)[:, None].astype(np.float64)
    return ref, C_CPLX * (k + 2.0) * EPS * mag


def long_row_operator():
    """(ops, rows): the ``long100`` construction of tests/test_gpu_saddle_spmm.py (Taylor-Hood, N = 15, n = 1937) with
    a row of exactly 48 entries added -- saddle rows of 48, 49, 64 and 100 entries and a pressure row of 60.  The tiled
    product keeps 48 entries of a row in registers and streams the rest."""
    return sm.long_rows(sm.th_operators(15, 0.1), [48, 49, 64, 100], p_target=60)


# ------------------------------------------------------------------------------------------------ CGS2 step
def cgs2_step(V, w):
    """One CGS2 step, column by column: V (nvec, n, mc) complex with orthonormal columns per column index, w (n, mc).
    Returns (h, w_out): h (nvec + 1, mc) -- the summed coefficients ``v_j^H w`` of the two passes, then the norm of
    what is left (real) --, w_out the unit vector (zero where nothing is left)."""
    nvec, n, mc = V.shape
    w = np.array(w, dtype=np.complex128)
    h = np.zeros((nvec + 1, mc), dtype=np.complex128)
    for _ in range(2):
        hp = np.einsum("jnc,nc->jc", V.conj(), w)
        w = w - np.einsum("jnc,jc->nc", V, hp)
        h[:nvec] += hp
    nrm = np.linalg.norm(w, axis=0)
    h[nvec] = nrm
    return h, w * np.where(nrm > 0, 1.0 / np.where(nrm > 0, nrm, 1.0), 0.0)


def cgs2_coef_bound(V, w):
    """(exact, bound): the coefficients ``V^H w`` in extended precision and a bound on what a CGS2 step in FP64 returns
    as their sum, per coefficient.  With h1 = V^H w + e1 and w1 = w - V h1 + eu, the second pass gives
    h2 = V^H w - (V^H V) h1 + V^H eu + e2, so the sum is  V^H w + (I - V^H V) h1 + V^H eu + e2  (the first pass's own
    error cancels).  Terms: ``|e2_j| <= g(n) |v_j|^T |w1|``, ``||eu|| <= || g(nvec) (|w| + |V| |h|) ||``,
    ``||I - V^H V||_2 ||h||``, and two roundings of the sum; ``g(k) = C_CPLX (k + 2) eps`` as for the product."""
    nvec, n, mc = V.shape
    Vl, wl = V.astype(np.clongdouble), np.asarray(w).astype(np.clongdouble)
    exact = np.einsum("jnc,nc->jc", Vl.conj(), wl)
    w1 = np.asarray(wl - np.einsum("jnc,jc->nc", Vl, exact)).astype(np.complex128)
    hx = exact.astype(np.complex128)
    bound = np.zeros((nvec, mc))
    for c in range(mc):
        Vc = V[:, :, c].T                                            # n x nvec
        defect = np.linalg.norm(np.eye(nvec) - Vc.conj().T @ Vc, 2)
        eu = np.linalg.norm(C_CPLX * (nvec + 2) * EPS * (np.abs(w[:, c]) + np.abs(Vc) @ np.abs(hx[:, c])))
        e2 = C_CPLX * (n + 2) * EPS * (np.abs(Vc).T @ np.abs(w1[:, c]))
        bound[:, c] = e2 + eu + defect * np.linalg.norm(hx[:, c]) + 2 * EPS * np.abs(hx[:, c])
    return hx, bound


# ------------------------------------------------------------------------------------------------ the cycle, step by step
# The restart cycle of the complex flexible GMRES as the kernels of ricadi_cplx.hip run it (cplx_gmres_start_kernel,
# cplx_gmres_hess_kernel, cplx_gmres_backsolve_kernel, cplx_update_kernel with sign = +1), one function per unit, in
# np.clongdouble, for one complex column.  The inputs of a unit are the DEVICE's own stored arrays (the coefficient
# column hout, the earlier cs / sn / gv, the V slots), so a comparison sees the rounding of one unit only.
#
# Bounds, eps = 2^-52 (u = eps / 2 the unit roundoff), counted, not measured:
#
# * Rotated column, cs, sn (C1 = 4): entrywise ``C1 (j + 2) eps ||h_col||_2``.  Applying a stored rotation
#   ``G = [[c, s], [-conj(s), c]]`` (c real) to the pair (cur, nxt) costs per output one real-times-complex product
#   (u), one complex product (within sqrt(2) gamma_2 < 2.83 u of the exact one, Higham section 3.6) and one addition
#   (u): at most 3.83 u (|c| |cur| + |s| |nxt|) <= 2 eps ||(cur, nxt)||_2, and rotations keep the norm, so after i
#   rotations `cur` is within 2 i eps ||h_col|| and entry i of the column within 2 (i + 1) eps ||h_col||.  The new
#   rotation: na = hypot(cur) and r = hypot(na, b) are within one ulp each (eps, then 2 eps), c = na / r within
#   3.5 eps, s = cur b / (na r) within 4.5 eps, d = cur r / na within 4 eps r, r = ||h_col||.  d and s carry the PHASE
#   of cur, so the 2 j eps ||h_col|| of cur arrive multiplied by rho = r / na (d) and b / na <= rho (s): with
#   rho <= 2 -- which hess_column reports and the tests assert of their inputs -- everything stays below
#   (4 j + 4.5) eps ||h_col|| < C1 (j + 2) eps ||h_col||.  cs and sn are scale-free; the issue's form carries
#   ||h_col||_2, which is >= 1 in every column the tests build (asserted with rho).  The two exact branches
#   (r == 0; |cur| == 0 < b) are compared exactly.
# * gv: ``g[j] = c g[j]`` (u) and ``g[j + 1] = -conj(s) g[j]`` (2.83 u) from the device's own c, s, g[j]: within
#   1.5 eps |g[j]|, asserted as ``C1 (j + 2) eps |g[j]|``.  The residual estimate |g[j + 1]| / ||b|| adds one hypot
#   and one division (1.5 eps) and is asserted within the same bar, divided by ||b||, of the least-squares residual of
#   the Hessenberg system made of the device's coefficient columns (hessenberg_ls, in extended precision).
# * Back substitution (C2 = 4): ``|R y - g| <= C2 k eps (|R| |y| + |g|)`` componentwise -- the backward-error result
#   for substitution (Higham chapter 8) with the complex factor: row i subtracts k - i - 1 complex products (2.83 u
#   each, u per subtraction) and divides by d as  q = s conj(d),  dd = |d|^2 (3 u),  q / dd (u): 6.83 u on the pivot
#   term; in all at most (0.5 k + 3.5) eps <= C2 k eps for k >= 1.  No condition number enters.
# * Correction: ``C_CPLX (k + 2) eps (|Z| |y| + |x|)`` entrywise, as the product's bound (k complex fused terms, one
#   addition to x).
# * Cycle start: gv[0] = sqrt(nrm2), scale = 1 / gv[0], resid = gv[0] / ||b|| are one correctly rounded sqrt and one
#   division each: bitwise NumPy's.
C1 = 4.0
C2 = 4.0
RHO_MAX = 2.0
LD, CLD = np.longdouble, np.clongdouble


def cycle_start(nrm2, bnorm):
    """(gv0, scale, resid) in float64 from the squared norms and ||b|| (arrays of one shape): sqrt, 1 / x (0 for a
    vanished column), x / ||b|| (0 where b = 0)."""
    nrm2, bnorm = np.asarray(nrm2, dtype=np.float64), np.asarray(bnorm, dtype=np.float64)
    nn = np.sqrt(nrm2)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(nn > 0.0, 1.0 / nn, 0.0)
        resid = np.where(bnorm > 0.0, nn / bnorm, 0.0)
    return nn, scale, resid


def hess_column(h, cs, sn):
    """Column j of the Hessenberg matrix through the stored rotations 0 .. j - 1 and the new one.  h: j + 2 complex
    (rows 0 .. j the CGS2 coefficients, row j + 1 the norm, real >= 0); cs, sn: the j earlier rotations.  Returns a
    dict: ``col`` (j + 2 entries: the column of R, entry j the pivot d, entry j + 1 zero), ``c``, ``s``, ``branch``
    ("zero": r == 0, c = 1, s = d = 0; "breakdown": |cur| == 0 < b, c = 0, s = 1, d = b; "general"), ``norm``
    (||h||_2) and ``rho`` (r / |cur|; 1 in the exact branches)."""
    h = np.asarray(h).astype(CLD)
    j = len(cs)
    assert h.shape == (j + 2,) and len(sn) == j
    col = np.zeros(j + 2, dtype=CLD)
    cur = h[0]
    for i in range(j):
        c, s, nxt = LD(cs[i]), CLD(sn[i]), h[i + 1]
        col[i] = c * cur + s * nxt
        cur = c * nxt - np.conj(s) * cur
    b = LD(h[j + 1].real)
    na = LD(np.abs(cur))
    r = LD(np.hypot(na, b))
    if r == 0:
        branch, c, s, d, rho = "zero", LD(1), CLD(0), CLD(0), LD(1)
    elif na == 0:
        branch, c, s, d, rho = "breakdown", LD(0), CLD(1), CLD(b), LD(1)
    else:
        branch, c, s, d, rho = "general", na / r, cur * (b / (na * r)), cur * (r / na), r / na
    col[j] = d
    return dict(col=col, c=c, s=s, branch=branch, norm=LD(np.sqrt(np.sum(np.abs(h) ** 2))), rho=rho)


def gv_update(gj, c, s):
    """(g[j], g[j + 1]) after the rotation (c, s): ``c g_j`` and ``-conj(s) g_j``."""
    gj = CLD(gj)
    return LD(c) * gj, -np.conj(CLD(s)) * gj


def resid_estimate(gnext, bnorm):
    """``|g[j + 1]| / ||b||`` (0 where b = 0)."""
    return LD(np.abs(CLD(gnext))) / LD(bnorm) if bnorm > 0 else LD(0)


def back_substitute(R, g):
    """y with ``R y = g`` for the k x k upper triangular R; a vanished pivot gives ``y_i = 0``."""
    R, g = np.asarray(R).astype(CLD), np.asarray(g).astype(CLD)
    k = g.size
    y = np.zeros(k, dtype=CLD)
    for i in range(k - 1, -1, -1):
        acc = g[i] - np.sum(R[i, i + 1:] * y[i + 1:])
        y[i] = acc / R[i, i] if R[i, i] != 0 else 0
    return y


def backsolve_ratio(R, g, y):
    """Largest ``|R y - g| / (C2 k eps (|R| |y| + |g|))`` over the rows with a pivot (0 / 0 counts as 0); the rows
    whose pivot vanished must have ``y_i == 0`` (AssertionError otherwise)."""
    k = g.size
    Rl, gl, yl = np.asarray(R).astype(CLD), np.asarray(g).astype(CLD), np.asarray(y).astype(CLD)
    piv = np.diag(Rl) != 0
    assert np.all(yl[~piv] == 0), "a vanished pivot did not give y_i = 0"
    res = np.abs(Rl @ yl - gl)
    bound = C2 * k * EPS * (np.abs(Rl) @ np.abs(yl) + np.abs(gl))
    ratio = np.where(res == 0, 0.0, res / np.where(bound > 0, bound, np.finfo(np.float64).tiny))
    return float(np.max(ratio[piv])) if piv.any() else 0.0


def correction(x, Z, y):
    """(ref, bound) of ``x + sum_i Z_i y_i``: x (n,), Z (k, n), y (k,) complex."""
    xl, Zl, yl = np.asarray(x).astype(CLD), np.asarray(Z).astype(CLD), np.asarray(y).astype(CLD)
    k = yl.size
    ref = xl + Zl.T @ yl
    bound = C_CPLX * (k + 2) * EPS * (np.abs(Zl).T @ np.abs(yl) + np.abs(xl))
    return ref, bound.astype(np.float64)


def hessenberg_ls(Hbar, beta):
    """The least-squares problem ``min || beta e_1 - Hbar y ||`` of a (k + 1) x k upper Hessenberg matrix with a real,
    non-negative subdiagonal, through the model's own rotations in extended precision.  Returns (y, resnorm, R, g):
    the minimiser, the residual norm ``|g[k]|``, the k x k triangular factor and the rotated right-hand side."""
    Hbar = np.asarray(Hbar).astype(CLD)
    k = Hbar.shape[1]
    assert Hbar.shape[0] == k + 1
    R = np.zeros((k, k), dtype=CLD)
    g = np.zeros(k + 1, dtype=CLD)
    g[0] = beta
    cs, sn = [], []
    for j in range(k):
        out = hess_column(Hbar[:j + 2, j], cs, sn)
        R[:j + 1, j] = out["col"][:j + 1]
        cs.append(out["c"])
        sn.append(out["s"])
        g[j], g[j + 1] = gv_update(g[j], out["c"], out["s"])
    return back_substitute(R, g[:k]), LD(np.abs(g[k])), R, g


# ------------------------------------------------------------------------------------------------ the cycle, checked
# check_cycle drives a "device" -- the step probe of the library on the GPU (tests/test_gpu_cplx_steps.py) or the
# float64 twin of tests/test_cplx_model_cpu.py -- through one restart cycle and holds everything it wrote to the model.
# A device has  begin(R, bnorm), step(j, W, groups), close(ks, Z, X) -> X  and  read(what, slot=0)  with the arrays of
# Context.cplx_probe_read_dev: V (ng, n, mc), hout (ng, restart + 2, 8), Hm (ng, 8, restart, restart + 1) [column,
# row], cs / sn (ng, 8, restart), gv (ng, 8, restart + 1), y (ng, restart, 8), scale / nrm2 (ng, 16), resid (ng, 8).
STATE = ("hout", "Hm", "cs", "sn", "gv", "y", "scale", "resid", "nrm2")
QUANTITIES = ("start norms", "coefficients", "orthogonality", "reconstruction", "rotated column", "cs", "sn", "gv",
              "residual estimate", "back-solve residual", "correction")


def _crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.float64) if np.iscomplexobj(a) else a


def same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b), equal_nan=True)


def all_nan(a):
    return bool(np.all(np.isnan(_bits(a))))


class CycleReport(dict):
    """Largest error / bound per quantity of QUANTITIES, the rotation branches and close shapes reached."""

    def __init__(self):
        super().__init__()
        self.branches, self.closes = set(), []

    def put(self, key, value):
        value = float(value)
        self[key] = max(self.get(key, 0.0), value if np.isfinite(value) else np.inf)

    def cmp(self, key, got, ref, bound):
        """error / bound entrywise; an exact match passes whatever the bound (0 / 0)."""
        err = np.abs(np.asarray(got).astype(CLD) - np.asarray(ref).astype(CLD)).astype(np.float64)
        bound = np.asarray(bound, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        self.put(key, np.max(ratio) if ratio.size else 0.0)

    def ok(self):
        return all(v <= 1.0 for v in self.values())


def cycle_inputs(ng, n, mc, restart, seed, breakdowns=False):
    """Seeded inputs of a cycle: residual panels R (ng, n, mc), ||b|| (1.25 times the column norms of R), the noise
    panels of the steps (unit-norm columns on average), the Z panels and the iterate x0.  ``breakdowns`` (mc >= 3): in
    group 0 column 1 of R and of every noise panel is zero (with W = noise + 3 v the column stays zero: the r == 0
    branch) and column 2 of R lives on the first 64 rows, column 2 of the first noise panel on the rows from 64 on
    (``v_0^H w`` is an exact zero: the |cur| == 0 < b branch)."""
    rng = np.random.default_rng(seed)
    R = _crandn(rng, ng, n, mc)
    noise = _crandn(rng, restart, ng, n, mc) / np.sqrt(2 * n)
    Z = _crandn(rng, restart, ng, n, mc)
    x0 = _crandn(rng, ng, n, mc)
    if breakdowns:
        assert mc >= 3 and n > 64
        R[0, :, 1] = 0.0
        noise[:, 0, :, 1] = 0.0
        R[0, 64:, 2] = 0.0
        noise[0, 0, :64, 2] = 0.0
    bnorm = 1.25 * np.sqrt(np.einsum("gnc,gnc->gc", R.real, R.real) + np.einsum("gnc,gnc->gc", R.imag, R.imag))
    return dict(R=R, bnorm=bnorm, noise=noise, Z=Z, x0=x0, breakdowns=breakdowns)


def step_panel(inp, j, V):
    """``W_j = noise_j + 3 v_j`` (V: slots 0 .. j of the device, (j + 1, ng, n, mc)); in a breakdown cycle column 2 of
    group 0 takes ``3 v_0`` on top at j >= 1, so that its column keeps rho = r / |cur| <= 2 behind the rotation
    (c, s) = (0, 1), which swaps the two leading coefficients."""
    W = inp["noise"][j] + 3.0 * V[j]
    if inp["breakdowns"]:
        if j == 0:
            W[0, :, 2] = inp["noise"][0, 0, :, 2]          # v_0 lives on the first 64 rows: keep the product exact
        else:
            W[0, :, 2] += 3.0 * V[0, 0, :, 2]
    return W


def _case(n, mc, restart=10, steps=10, leave=None, ks_list=((10, 4, 10), (7, 4, 2)), breakdowns=False, opts=None):
    name = "n%d-mc%d-restart%d%s" % (n, mc, restart, "-breakdowns" if breakdowns else "")
    return dict(name=name, n=n, mc=mc, ng=3, restart=restart, steps=steps, leave={1: 3} if leave is None else leave,
                ks_list=ks_list, breakdowns=breakdowns, seed=1000 * n + mc, opts=dict(opts or {}))


# The cycles of tests/test_gpu_cplx_steps.py (and of the float64 twin): n = 61 is one partial 128-row block, 130 one full
# block plus two rows, 450 four blocks with a tail; gmres_restart = 10, group 1 leaves after step 3, the cycle end
# with k = (10, 4, 10) and again with k = (7, 4, 2); one case at the default restart (opts empty: the context's own);
# one short cycle with the two exact rotation branches.
DEFAULT_RESTART = 30
CYCLE_CASES = [_case(n, mc, opts=dict(gmres_restart=10)) for n in (61, 130, 450) for mc in (1, 3, 8)] + \
    [_case(450, 3, restart=DEFAULT_RESTART),
     _case(130, 3, steps=2, leave={}, ks_list=((2, 2, 2),), breakdowns=True, opts=dict(gmres_restart=10))]


def run_case(dev, case):
    inp = cycle_inputs(case["ng"], case["n"], case["mc"], case["restart"], case["seed"], case["breakdowns"])
    return check_cycle(dev, inp, case["restart"], case["steps"], case["leave"], case["ks_list"])


def _read_state(dev):
    return {k: dev.read(k) for k in STATE}


def _group_unchanged(before, after, g):
    return [k for k in before if not same_bits(before[k][g], after[k][g])]


def check_cycle(dev, inp, restart, steps, leave=None, ks_list=()):
    """One cycle on ``dev``: begin, ``steps`` Arnoldi steps (group g leaves the table after step ``leave[g]``), then
    one cycle end per entry of ``ks_list`` (each from the iterate x0).  Returns a CycleReport; structural violations
    (something written that should not be, a NaN where a value belongs, an inexact exact quantity) raise
    AssertionError at once."""
    R, bnorm = inp["R"], inp["bnorm"]
    ng, n, mc = R.shape
    leave = dict(leave or {})
    rep = CycleReport()
    tiny = np.finfo(np.float64).tiny
    # ---- begin
    dev.begin(R, bnorm)
    st = _read_state(dev)
    nrm2 = st["nrm2"][:, 0:2 * mc:2]
    exact = np.einsum("gnc->gc", np.abs(R.astype(CLD)) ** 2)
    rep.cmp("start norms", nrm2, exact, (n + 2) * EPS * exact.astype(np.float64))
    assert np.all(st["nrm2"][:, 1:2 * mc:2] == 0.0)
    nn, scale, resid = cycle_start(nrm2, bnorm)
    assert same_bits(st["gv"][:, :mc, 0], nn.astype(np.complex128)), "gv[0] is not sqrt(nrm2)"
    assert same_bits(st["scale"][:, 0:2 * mc:2], scale) and same_bits(st["scale"][:, 1:2 * mc:2], scale)
    assert same_bits(st["resid"][:, :mc], resid)
    V = [dev.read("V", 0)]
    assert same_bits(V[0], (R.view(np.float64) * np.repeat(scale, 2, axis=1)[:, None, :]).view(np.complex128))
    assert all_nan(st["gv"][:, :, 1:]) and all_nan(st["gv"][:, mc:]) and all_nan(st["scale"][:, 2 * mc:])
    assert all_nan(st["resid"][:, mc:])
    for k in ("hout", "Hm", "cs", "sn", "y"):
        assert all_nan(st[k]), k
    for slot in range(1, restart + 1):
        assert all_nan(dev.read("V", slot)), slot
    # ---- steps
    hbar = np.zeros((ng, mc, restart + 1, restart), dtype=CLD)
    for j in range(steps):
        on = [g for g in range(ng) if leave.get(g, restart) >= j]
        W = step_panel(inp, j, np.stack(V))
        dev.step(j, W, on)
        new = _read_state(dev)
        Vn = dev.read("V", j + 1)
        for g in range(ng):
            if g not in on:
                assert not _group_unchanged(st, new, g), (j, g, _group_unchanged(st, new, g))
                assert all_nan(Vn[g]), "a group that left the table got a basis vector"
                continue
            Vg = np.stack([v[g] for v in V])                         # (j + 1, n, mc)
            hx, hb = cgs2_coef_bound(Vg, W[g])
            h = new["hout"][g, :j + 2, :mc]
            # (the CGS2 step writes whole rows of 16 lanes: the lanes beyond the panel hold zeros, also in scale)
            assert np.all(np.isfinite(_bits(h))) and all_nan(new["hout"][g, j + 2:]) and \
                np.all(new["hout"][g, :j + 2, mc:] == 0.0) and np.all(new["scale"][g, 2 * mc:] == 0.0)
            assert np.all(h[j + 1].imag == 0.0) and np.all(h[j + 1].real >= 0.0)
            rep.cmp("coefficients", h[:j + 1], hx, hb)
            assert same_bits(np.sqrt(new["nrm2"][g, 0:2 * mc:2]), h[j + 1].real), "hout[j + 1] is not sqrt(nrm2)"
            _, sc, _ = cycle_start(new["nrm2"][g, 0:2 * mc:2], np.ones(mc))
            assert same_bits(new["scale"][g, 0:2 * mc:2], sc) and same_bits(new["scale"][g, 1:2 * mc:2], sc)
            assert np.all(np.isfinite(_bits(Vn[g])))
            for c in range(mc):
                hc = h[:, c]
                Vc = Vg[:, :, c].T
                wn = np.linalg.norm(W[g, :, c])
                if hc[j + 1].real > 0:
                    rep.put("orthogonality", np.linalg.norm(Vc.conj().T @ Vn[g, :, c]) / (8 * n * EPS))
                else:
                    assert np.all(Vn[g, :, c] == 0.0), "nothing left over, but the new vector is not zero"
                rec = W[g, :, c] - Vc @ hc[:j + 1] - hc[j + 1] * Vn[g, :, c]
                rep.put("reconstruction", np.linalg.norm(rec) / max(8 * (j + 3) * n * EPS * wn, tiny))
                # the Hessenberg column through the rotations
                out = hess_column(hc, st["cs"][g, c, :j], st["sn"][g, c, :j])
                rep.branches.add(out["branch"])
                bar = C1 * (j + 2) * EPS * float(out["norm"])
                col = new["Hm"][g, c, j]
                assert all_nan(col[j + 2:]) and col[j + 1] == 0.0
                if out["branch"] == "general":
                    assert out["rho"] <= RHO_MAX and out["norm"] >= 1, (j, g, c, out["rho"], out["norm"])
                    rep.cmp("rotated column", col[:j + 1], out["col"][:j + 1], bar)
                    rep.cmp("cs", new["cs"][g, c, j], out["c"], bar)
                    rep.cmp("sn", new["sn"][g, c, j], out["s"], bar)
                else:
                    rep.cmp("rotated column", col[:j], out["col"][:j], bar)
                    assert col[j] == complex(out["col"][j]) and new["cs"][g, c, j] == float(out["c"]) and \
                        new["sn"][g, c, j] == complex(out["s"]), (out["branch"], col[j], new["cs"][g, c, j])
                gj = st["gv"][g, c, j]
                g0, g1 = gv_update(gj, new["cs"][g, c, j], new["sn"][g, c, j])
                rep.cmp("gv", new["gv"][g, c, j:j + 2], [g0, g1], C1 * (j + 2) * EPS * abs(gj))
                # the estimate against the least-squares residual of the Hessenberg system of the device's columns
                hbar[g, c, :j + 2, j] = hc
                _, rn, _, _ = hessenberg_ls(hbar[g, c, :j + 2, :j + 1], nn[g, c])
                bn = bnorm[g, c]
                if bn > 0:
                    rep.cmp("residual estimate", new["resid"][g, c], rn / LD(bn), C1 * (j + 2) * EPS * abs(gj) / bn)
                else:
                    assert new["resid"][g, c] == 0.0
            # what the step did not write
            assert same_bits(st["y"][g], new["y"][g]) and all_nan(new["Hm"][g, :, j + 1:]) and \
                all_nan(new["cs"][g, :, j + 1:]) and all_nan(new["sn"][g, :, j + 1:]) and \
                all_nan(new["gv"][g, :, j + 2:]), (j, g)
            for k in ("Hm", "cs", "sn", "gv"):
                assert same_bits(st[k][g, :, :j], new[k][g, :, :j]) and all_nan(new[k][g, mc:]), (k, j, g)
            assert all_nan(new["resid"][g, mc:])
        for slot in range(j + 2, restart + 1):
            assert all_nan(dev.read("V", slot)), (j, slot)
        for slot in range(j + 1):
            assert same_bits(dev.read("V", slot), V[slot]), (j, slot)
        V.append(Vn)
        st = new
    # ---- cycle ends
    for ks in ks_list:
        nz = max(ks)
        X = dev.close(ks, inp["Z"][:nz], inp["x0"].copy())
        new = _read_state(dev)
        rep.closes.append(tuple(ks))
        for k in STATE:
            if k != "y":
                assert same_bits(st[k], new[k]), "the cycle end wrote %s" % k
        for g in range(ng):
            k = ks[g]
            assert same_bits(st["y"][g, k:], new["y"][g, k:]) and same_bits(st["y"][g, :, mc:], new["y"][g, :, mc:])
            y = new["y"][g, :k, :mc]
            assert np.all(np.isfinite(_bits(y))) and np.all(np.isfinite(_bits(X[g])))
            for c in range(mc):
                Rm = np.triu(st["Hm"][g, c, :k, :k].T)
                rep.put("back-solve residual", backsolve_ratio(Rm, st["gv"][g, c, :k], y[:, c]))
                ref, bound = correction(inp["x0"][g, :, c], inp["Z"][:k, g, :, c], y[:, c])
                rep.cmp("correction", X[g, :, c], ref, bound)
                if not np.any(y[:, c]):
                    assert same_bits(X[g, :, c], inp["x0"][g, :, c]), "y = 0 but x changed"
        st = new
    return rep


# ------------------------------------------------------------------------------------------------ flexible GMRES
def fgmres(apply_s, apply_pinv, b, restart=8, tol=1e-10, max_cycles=60):
    """Right-preconditioned flexible GMRES(restart) from zero for one right-hand side b; inner products are
    ``v^H w`` (complex on complex input, real on real input).  Returns (x, iterations, cycles, converged): converged on
    the TRUE relative residual, recomputed at every cycle start."""
    b = np.asarray(b)
    n = b.size
    x = np.zeros(n, dtype=b.dtype)
    bn = np.linalg.norm(b)
    if bn == 0:
        return x, 0, 0, True
    iters = 0
    for cyc in range(max_cycles + 1):
        r = b - apply_s(x)
        beta = np.linalg.norm(r)
        if beta <= tol * bn:
            return x, iters, cyc, True
        if cyc == max_cycles:
            break
        V = np.zeros((restart + 1, n), dtype=b.dtype)
        Z = np.zeros((restart, n), dtype=b.dtype)
        H = np.zeros((restart + 1, restart), dtype=b.dtype)
        V[0] = r / beta
        k = 0
        for j in range(restart):
            Z[j] = apply_pinv(V[j])
            w = apply_s(Z[j])
            for _ in range(2):
                hp = V[:j + 1].conj() @ w
                w = w - V[:j + 1].T @ hp
                H[:j + 1, j] += hp
            hn = np.linalg.norm(w)
            H[j + 1, j] = hn
            iters += 1
            k = j + 1
            e1 = np.zeros(k + 1, dtype=b.dtype)
            e1[0] = beta
            y, *_ = np.linalg.lstsq(H[:k + 1, :k], e1, rcond=None)
            if hn == 0 or np.linalg.norm(e1 - H[:k + 1, :k] @ y) <= tol * bn:
                break
            V[j + 1] = w / hn
        x = x + Z[:k].T @ y
    return x, iters, max_cycles, False


def real_equivalent(S):
    """The real 2n x 2n form [[Re S, -Im S], [Im S, Re S]] of a complex sparse matrix (acts on [Re x; Im x])."""
    S = sps.csr_matrix(S)
    return sps.bmat([[S.real, -S.imag], [S.imag, S.real]], format="csr")


# ------------------------------------------------------------------------------------------------ transfer functions
def transfer_saddle(calA, calE, J, B, C, omega):
    """``G(i w) = C V`` with ``S(-i w, 1) [V; L] = [-B; 0]``, (calA, calE) = (A, M): the route of ``freq_response``,
    through the dense saddle matrix."""
    S = saddle_cplx(calA, calE, J, -1j * omega, 1.0).toarray()
    nv = calA.shape[0]
    rhs = np.vstack([-np.asarray(B, dtype=np.complex128), np.zeros((J.shape[0], B.shape[1]))])
    lu = sla.lu_factor(S)
    X = sla.lu_solve(lu, rhs)
    X = X + sla.lu_solve(lu, rhs - S @ X)
    return np.asarray(C) @ X[:nv]


class Projected:
    """The system on an orthonormal basis Theta of ker J: ``Eh v' = Ah v + Bh u``, ``y = Ch v``."""

    def __init__(self, Ad, Ed, Theta, B, C):
        self.Th = Theta
        self.Ah, self.Eh = Theta.T @ Ad @ Theta, Theta.T @ Ed @ Theta
        self.Bh, self.Ch = Theta.T @ np.asarray(B), np.asarray(C) @ Theta

    def transfer(self, omega):
        """``Ch (i w Eh - Ah)^-1 Bh``."""
        return self.Ch @ np.linalg.solve(1j * omega * self.Eh - self.Ah, self.Bh.astype(np.complex128))

    def gramian_factors(self):
        """(Lq, Lp): ``Q = Lq Lq^T`` observability (``Ah^T Q Eh + Eh^T Q Ah + Ch^T Ch = 0``) and ``P = Lp Lp^T``
        reachability (``Ah P Eh^T + Eh P Ah^T + Bh Bh^T = 0``) Gramian, from LAPACK's Bartels-Stewart solver and a
        symmetric eigendecomposition (negative rounding-level eigenvalues clipped)."""
        a = np.linalg.solve(self.Eh, self.Ah)
        b = np.linalg.solve(self.Eh, self.Bh)
        P = sla.solve_continuous_lyapunov(a, -b @ b.T)
        Qt = sla.solve_continuous_lyapunov(a.T, -self.Ch.T @ self.Ch)          # Qt = Eh^T Q Eh
        Q = np.linalg.solve(self.Eh.T, np.linalg.solve(self.Eh.T, Qt.T).T)

        def root(X):
            lam, U = np.linalg.eigh(0.5 * (X + X.T))
            return U * np.sqrt(np.maximum(lam, 0.0))
        return root(Q), root(P)

    def balanced_truncation(self, r):
        """Square-root balanced truncation to order r: dict with hsv (all Hankel singular values) and the reduced
        ``ar``, ``er``, ``br``, ``cr`` -- the keys of ``lqgbt.balance_factors``."""
        Lq, Lp = self.gramian_factors()
        U, sig, Vt = np.linalg.svd(Lq.T @ self.Eh @ Lp)
        sq = 1.0 / np.sqrt(sig[:r])
        Tl, Tr = Lq @ (U[:, :r] * sq), Lp @ (Vt[:r].T * sq)
        return dict(hsv=sig, order=r, ar=Tl.T @ self.Ah @ Tr, er=Tl.T @ self.Eh @ Tr, br=Tl.T @ self.Bh,
                    cr=self.Ch @ Tr)


def reduced_transfer(red, omega):
    """``C_r (i w E_r - A_r)^-1 B_r`` of a reduced-model dict."""
    return red["cr"] @ np.linalg.solve(1j * omega * red["er"] - red["ar"], red["br"].astype(np.complex128))


def sigma_max(G):
    return float(np.linalg.norm(G, 2))
