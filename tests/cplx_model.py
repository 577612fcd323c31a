"""NumPy / SciPy FP64 model of the complex-shift path (ricadi_cplx.hip, solver_cplx.inl):

* the complex saddle product ``y = S(alpha, beta) x``, ``S(a, b) = [[b calA + a calE, J^T], [J, 0]]`` with complex
  ``alpha``, and the entrywise bound the device forms are held to (:func:`product`);
* one CGS2 step against an orthonormal complex basis and the bound on its coefficients (:func:`cgs2_step`,
  :func:`cgs2_coef_bound`);
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
