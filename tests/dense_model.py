"""Extended-precision model of the dense layer of an ADI step (ricadi_dense.hip, solver_dense.inl) and the
componentwise error bounds a correct FP64 implementation of each operation satisfies.

Plain NumPy / SciPy, no GPU and no project imports.  Every operation is computed in ``np.longdouble`` and comes
with a ``*_bound(..., u)`` function from the standard analysis of a dot product:

    |fl(x^T y) - x^T y| <= gamma_k |x|^T |y|,     gamma_k = k u / (1 - k u),

with ``k`` the number of summed terms plus the number of roundings applied to the sum afterwards; the bound holds
for EVERY order of summation (sequential, tree, partial sums added by atomics, FMA or not), which is what lets one
bound serve all launch forms of a kernel.  Compositions add the bounds of their stages, each stage applied to the
perturbed result of the one before.  Sums of non-negative terms (squared norms) get the relative bound gamma_k.

A test compares at ``tol = bound(U) + bound(U_REF)``: the first term is what the implementation under test may
be off by, the second what the model itself may be off by (``U_REF`` is the unit roundoff of ``longdouble``, so the
comparison stays valid on a host where ``longdouble`` is ``float64``).
"""
import functools

import numpy as np
import scipy.sparse as sps

LD = np.longdouble
U = 2.0 ** -53                                  # unit roundoff of FP64
U_REF = float(np.finfo(LD).eps) / 2.0           # ... of the model's arithmetic


def ld(a):
    return np.asarray(a, dtype=LD)


def gamma(k, u):
    ku = k * u
    assert ku < 0.5
    return ku / (1.0 - ku)


def tol(bound_fn, *args, **kw):
    """``bound(U) + bound(U_REF)``: the comparison tolerance (a tuple where the bound function returns one)."""
    a, b = bound_fn(*args, U, **kw), bound_fn(*args, U_REF, **kw)
    if isinstance(a, tuple):
        return tuple(np.asarray(x) + np.asarray(y) for x, y in zip(a, b))
    return np.asarray(a) + np.asarray(b)


def ratio(got, ref, tolerance):
    """Largest ``|got - ref| / tolerance`` (0/0 counts as 0; anything non-finite or off where the tolerance is 0
    gives inf): a result passes iff this is <= 1."""
    err = np.abs(ld(got) - ld(ref))
    t = ld(tolerance)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / t)
    r = np.where(np.isfinite(r), r, LD(np.inf))
    return float(np.max(r)) if r.size else 0.0


# The bound functions work on absolute values only, in float64: sums of non-negative terms, accurate to a relative
# gamma_n ~ 1e-13 of the bound itself, which no comparison can tell from the bound.
def fa(a):
    return np.abs(np.asarray(a, dtype=np.float64))


# ------------------------------------------------------------------------------------------------ products
def tn(A, B):
    """``A^T B``."""
    return ld(A).T @ ld(B)


def tn_bound(A, B, u):
    """``n`` summed products: ``gamma_n |A|^T |B|``."""
    return gamma(np.shape(A)[0], u) * (fa(A).T @ fa(B))


def gram(Z):
    return tn(Z, Z)


def gram_bound(Z, u):
    return tn_bound(Z, Z, u)


def nn(A, C, alpha=1.0, beta=0.0, Y=None):
    """``alpha A C + beta Y``; ``beta == 0`` ignores ``Y`` altogether (it may hold NaN)."""
    out = LD(alpha) * (ld(A) @ ld(C))
    if beta != 0.0:
        out = out + LD(beta) * ld(Y)
    return out


def nn_bound(A, C, alpha, beta, Y, u):
    """``p`` summed products, the multiplication by alpha and the final addition: ``(p + 2) u |alpha| |A||C|``, and
    ``u |beta Y|`` for the rounded product ``beta Y``."""
    p = np.shape(A)[1]
    b = gamma(p + 2, u) * abs(alpha) * (fa(A) @ fa(C))
    if beta != 0.0:
        b = b + u * abs(beta) * fa(Y)
    return b


class _Csr:
    """A sparse matrix: ``mul(X)`` = M X in longdouble, ``amul(X)`` = |M| |X| in float64, ``r`` = the largest number
    of stored entries in a row (the length of the longest dot product)."""

    def __init__(self, M):
        self.csr = sps.csr_matrix(M)
        M = sps.coo_matrix(self.csr)
        self.shape, self.row, self.col, self.val = M.shape, M.row, M.col, ld(M.data)
        self.r = int(np.bincount(M.row, minlength=1).max()) if M.nnz else 0
        self.abs = abs(self.csr).astype(np.float64)

    def mul(self, X):
        X = ld(X)
        out = np.zeros((self.shape[0], X.shape[1]), dtype=LD)
        np.add.at(out, self.row, self.val[:, None] * X[self.col])
        return out

    def amul(self, X):
        return self.abs @ fa(X)


# ------------------------------------------------------------------------------------------------ gain
def gain_stages(Z, B):
    """``(S, T) = (Z^T B, Z S)``: the two dense stages of the gain (shared by every MT and coef)."""
    S = tn(Z, B)
    return S, ld(Z) @ S


def gain(MT, Z, B, coef=1.0, stages=None):
    """``coef * MT (Z (Z^T B))``."""
    S, T = stages if stages is not None else gain_stages(Z, B)
    return LD(coef) * _Csr(MT).mul(T)


def gain_bound(MT, Z, B, coef, u, stages=None):
    """Three stages: S = Z^T B (nv terms), T = Z S (c terms + 2, as ``nn``), K = coef MT T (row entries of MT + the
    multiplication by alpha, the final addition and the one by coef); each on the perturbed result of the one before."""
    S, T = stages if stages is not None else gain_stages(Z, B)
    M = _Csr(MT)
    Za = fa(Z)
    c = Za.shape[1]
    bS = tn_bound(Z, B, u)
    bT = Za @ bS + gamma(c + 2, u) * (Za @ (fa(S) + bS))
    return abs(coef) * (M.amul(bT) + gamma(M.r + 3, u) * M.amul(fa(T) + bT))


# ------------------------------------------------------------------------------------------------ linear combinations
def lincomb(coef, panels):
    """``sum_i coef[i] panels[i]``  (panels: nvec x nrows x m)."""
    return np.tensordot(ld(coef), ld(panels), axes=(0, 0))


def lincomb_bound(coef, panels, u):
    """nvec summed products and the scaling by the sign: ``gamma_{nvec + 1} sum_i |coef[i]| |panel_i|``."""
    return gamma(len(coef) + 1, u) * np.tensordot(fa(coef), fa(panels), axes=(0, 0))


def apply_e(E, V, W, coef=1.0):
    """``W + coef E V``."""
    return ld(W) + LD(coef) * _Csr(E).mul(V)


def apply_e_bound(E, V, W, coef, u):
    """The row entries of E, the multiplication by coef and the addition of W; W takes that addition's rounding."""
    Em = _Csr(E)
    return gamma(Em.r + 2, u) * abs(coef) * Em.amul(V) + u * fa(W)


def _sumsq_bound(x, bx, u):
    """Bound on ``|fl(sum xhat^2) - sum x^2|`` for ``|xhat - x| <= bx``: the entries' own error carried through the
    squares, and ``gamma_{N + 1}`` relative for the sum of the N non-negative squares of the perturbed entries."""
    x = fa(x)
    carried = np.sum(bx * (2 * x + bx))
    return carried + gamma(x.size + 1, u) * (np.sum(x * x) + carried)


def recombine(Us, coefz, coefw, E, W):
    """One sweep's recombination: ``Z[:, j m:(j+1) m] = sum_s coefz[s, j] U_s``, ``W + E sum_s coefw[s] U_s``, the
    squared Frobenius norm of every block of Z and their total.  Us: nslot x nv x m."""
    Us, cz = ld(Us), ld(coefz)
    nslot, nv, m = Us.shape
    G = cz.shape[1]
    Z = np.concatenate([lincomb(cz[:, j], Us) for j in range(G)], axis=1)
    Wn = ld(W) + _Csr(E).mul(lincomb(coefw, Us))
    bn = np.array([np.sum(Z[:, j * m:(j + 1) * m] ** 2) for j in range(G)], dtype=LD)
    return Z, Wn, bn, np.sum(bn)


def recombine_bound(Us, coefz, coefw, E, W, u, Z=None):
    """Bounds for the four results of ``recombine`` (same order); ``Z``: its first result, if at hand."""
    nslot, nv, m = np.shape(Us)
    G = np.shape(coefz)[1]
    cz = np.asarray(coefz)
    bZ = np.concatenate([lincomb_bound(cz[:, j], Us, u) for j in range(G)], axis=1)
    Em = _Csr(E)
    t, bt = lincomb(coefw, Us), lincomb_bound(coefw, Us, u)
    # r summed products, the multiplication by alpha, the addition of W; W itself takes the rounding of that addition
    bW = Em.amul(bt) + gamma(Em.r + 2, u) * Em.amul(fa(t) + bt) + u * fa(W)
    if Z is None:
        Z = recombine(Us, coefz, coefw, E, W)[0]
    bbn = np.array([_sumsq_bound(Z[:, j * m:(j + 1) * m], bZ[:, j * m:(j + 1) * m], u) for j in range(G)])
    # the total sums the G block norms: G more additions of non-negative terms on top of each block's own bound
    btot = np.sum(bbn) + gamma(G, u) * float(np.sum(fa(Z) ** 2))
    return bZ, bW, bbn, btot


# ------------------------------------------------------------------------------------------------ norms of a panel
def panel_norms(W):
    """``(||W^T W||_F, ||W||_F^2)``."""
    G = gram(W)
    return np.sqrt(np.sum(G * G)), np.trace(G)


def panel_norms_bound(W, u):
    """``(bound of ||W^T W||_F, bound of ||W||_F^2)``.  The trace is a sum of nrows * m non-negative squares:
    relative.  The Frobenius norm of the Gram matrix carries the Gram bound through the m^2 squares, their sum and
    the square root (``|sqrt a - sqrt b| <= |a - b| / sqrt b``, and one rounding for the root)."""
    G, bG = fa(gram(W)), gram_bound(W, u)
    n, m = np.shape(W)
    btr = gamma(n * m + 1, u) * np.trace(G)
    f = np.sqrt(np.sum(G * G))
    bf = (_sumsq_bound(G, bG, u) / f if f > 0 else 0.0) + u * f
    return bf, btr


# ------------------------------------------------------------------------------------------------ QR
def qr_posdiag(Z, want_q=True):
    """Householder QR in longdouble: ``(Q, R)`` with Q n x c (None unless ``want_q``), R c x c upper triangular,
    ``diag(R) > 0``."""
    A = ld(Z).copy()
    n, c = A.shape
    assert n >= c
    V, tau = [], []
    for k in range(c):
        x = A[k:, k]
        nx = np.sqrt(np.sum(x * x))
        v = x.copy()
        alpha = x[0]
        beta = -nx if alpha >= 0 else nx
        if nx == 0:
            V.append(v)
            tau.append(LD(0))
            continue
        v[0] = alpha - beta
        t = LD(2) / np.sum(v * v)
        A[k:, k:] -= np.outer(t * v, v @ A[k:, k:])
        V.append(v)
        tau.append(t)
    R = np.triu(A[:c])
    s = np.where(np.diag(R) < 0, LD(-1), LD(1))
    if not want_q:
        return None, R * s[:, None]
    Q = np.zeros((n, c), dtype=LD)
    Q[:c] = np.eye(c, dtype=LD)
    for k in range(c - 1, -1, -1):
        Q[k:, k:] -= np.outer(tau[k] * V[k], V[k] @ Q[k:, k:])
    return Q * s, R * s[:, None]


def fix_row_signs(R):
    """R with every row's sign chosen so that its diagonal entry is >= 0."""
    R = np.asarray(R)
    s = np.where(np.diag(R) < 0, -1.0, 1.0).astype(R.dtype)
    return R * s[:, None]


def r_distance(R, Rref):
    """Largest entrywise difference of two triangular factors relative to ``||Rref||_F`` (= ``||Z||_F``)."""
    d = np.abs(ld(R) - ld(Rref))
    return float(np.max(d) / np.sqrt(np.sum(ld(Rref) ** 2)))


# ------------------------------------------------------------------------------------------------ test matrices
def panel(seed, *shape):
    """Standard normal entries; the seed is mixed with the shape so that no two shapes share a prefix."""
    return np.random.default_rng([seed, *shape]).standard_normal(shape)


def wellcond(nv, c, seed=0):
    """nv x c matrix with singular values spread over [1, 10]."""
    rng = np.random.default_rng([seed, nv, c])
    Qm, _ = np.linalg.qr(rng.standard_normal((nv, c)))
    Vm, _ = np.linalg.qr(rng.standard_normal((c, c)))
    return np.ascontiguousarray((Qm * np.linspace(1.0, 10.0, c)) @ Vm.T)


def sparse_rows(nv, per_row, seed=0):
    """Random nv x nv CSR matrix with ``min(per_row, nv)`` entries in every row."""
    rng = np.random.default_rng([seed, nv, per_row])
    k = min(per_row, nv)
    cols = np.concatenate([np.sort(rng.choice(nv, size=k, replace=False)) for _ in range(nv)])
    return sps.csr_matrix((rng.standard_normal(nv * k), cols, np.arange(0, nv * k + 1, k)), shape=(nv, nv))


def sweep_tables(nslot, G, seed=0):
    """Coefficient tables of a sweep as an all-gather leaves them: the rows of a random upper triangular G x G matrix
    dealt to ``nslot`` slots in a random order; slots beyond G (and, where there are none, two of the G slots) are
    padding: all-zero rows.  Returns ``(coefz (nslot x G), coefw (nslot), padding slot ids)``."""
    rng = np.random.default_rng([seed, nslot, G])
    Rm = np.triu(rng.standard_normal((G, G)))
    cw = rng.standard_normal(G)
    used = min(G, nslot)
    npad = nslot - used
    if npad < 2 and used > 2:          # no spare slot: two shifts' rows become padding
        drop = 2 - npad
        Rm[used - drop:used] = 0.0
        cw[used - drop:used] = 0.0
    slots = rng.permutation(nslot)
    coefz = np.zeros((nslot, G))
    coefw = np.zeros(nslot)
    coefz[slots[:used]] = Rm[:used]
    coefw[slots[:used]] = cw[:used]
    pad = [int(s) for s in range(nslot) if not coefz[s].any() and coefw[s] == 0.0]
    return coefz, coefw, pad


# ------------------------------------------------------------------------------------------------ shapes of the GPU tests
GRAM_C = (1, 15, 16, 17, 33, 64, 127, 128, 129, 320, 321, 385)
GRAM_NV = (1, 3, 63, 64, 65, 257, 1021)
GRAM_CASES = sorted({(1021, c) for c in GRAM_C} | {(nv, c) for nv in GRAM_NV for c in (17, 128, 321)})
GAIN_NB = (1, 7, 32, 33, 128)
GAIN_C = (1, 3, 5, 31, 64, 127, 128, 129, 512, 513)
GAIN_NV = (65, 1021)
GAIN_CASES = [(nv, nb, c) for nv in GAIN_NV for nb in GAIN_NB for c in GAIN_C]
NORMS_CASES = [(nrows, m) for nrows in (1, 63, 257, 1021) for m in (1, 16, 17, 127, 128)]
SWEEP_CASES = [(1, 1, 1), (4, 4, 7), (16, 16, 16), (5, 3, 33), (16, 2, 100), (8, 8, 128), (17, 4, 16), (4, 17, 8)]
LINCOMB_CASES = [(nrows, m, nvec) for nrows in (1, 65, 1021) for m in (1, 7, 16, 33, 128) for nvec in (1, 2, 17, 64)]
QR_C = (1, 31, 32, 33, 127, 128, 129, 257)
QR_CASES = [(nv, c) for c in QR_C for nv in sorted({c, 255, 256, 257, 2049}) if nv >= c]


def qr_matrix(nv, c):
    """The matrix of the block-QR case (nv, c)."""
    return wellcond(nv, c, seed=3)


@functools.lru_cache(maxsize=None)
def qr_reference_r(nv, c):
    return qr_posdiag(qr_matrix(nv, c), want_q=False)[1]


# r_distance between LAPACK's float64 Householder R (np.linalg.qr, row signs fixed) and qr_reference_r, largest over
# QR_CASES, as measured on the CPU (test_dense_model_cpu.py measures it again); the GPU factorisation -- CholQR2
# panels with re-orthogonalisation: as accurate as Householder on these matrices, but summing in another order --
# is allowed QR_R_FACTOR times that.
QR_R_DISTANCE = 9.3e-17
QR_R_FACTOR = 10.0


def sweep_fused(nslot, G, m):
    """Whether the recombination of these sizes runs in the fused kernel (ricadi_dense.hip: sweep_combine_ok)."""
    return nslot <= 16 and G <= 16 and m <= 128
