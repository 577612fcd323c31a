"""Model of RADI with shifts generated from the iteration itself ("residual Hamiltonian shifts": Benner, Bujanovic,
Kuerschner, Saak, Numer. Math. 2018, section 4.5): tests/radi_model.radi plus the selection rule, with
NumPy's eigenvalues and ``qr`` (the eigenvectors of the candidates are extended-precision null vectors: ``select``).

After a step the iteration holds the residual factor R, U (gain so far minus ``old``), B and the new block of Z.  With
Q an orthonormal basis of that block (k <= m columns, all in ker J, so the pressure drops out of every projection; from
the block's QR, leaving out the columns whose diagonal entry of R is below 3e-8 of the largest one: the ``dre`` call
forms have a W of 8 columns and rank 4, and so has every block of their Z)

    H_A = Q^T cal A Q,  H_E = Q^T cal E Q,  H_R = Q^T R,  H_U = Q^T U,  H_B = Q^T B
    A_c = H_A - H_U H_B^T,   At = H_E^-1 A_c,   Rt = H_E^-1 H_R
    Ham = [[At^T, -H_B H_B^T], [-Rt Rt^T, -At]]                                        (2k x 2k)

Candidates are the eigenvalues of Ham in the open left half plane, one of each conjugate pair (Im >= 0); the criterion of
a candidate with eigenvector x = [r; q] is ||q|| / ||x||; the next shift is -|lambda| of the candidate with the largest
criterion; the margin is the largest criterion over the second largest (inf with one candidate).  The caller's list is
the fallback (a counter of its own, cycling): no candidate, or a shift that is not finite and negative.
"""
import numpy as np

import dense_model as dm
import radi_model as rm

RANK_TOL = 3e-8       # RICADI_RADI_RANK_TOL: above the accuracy of the device's iterative solves, far below any independent column


def pack(Q, calA, calE, R, U, B):
    """H = Q^T [cal A Q | cal E Q | R | U | B], k x (2k + m + 2 nb): what the device's reduction kernel returns."""
    return Q.T @ np.hstack([calA @ Q, calE @ Q, R, U, B])


def keep_columns(Rq):
    """The columns of a block's QR that enter the basis: |R_ii| >= RANK_TOL max |R_jj|."""
    d = np.abs(np.diag(Rq))
    return d >= RANK_TOL * d.max()


def restrict(H, m, nb, keep):
    """The packed H of the basis Q[:, keep] from the packed H of Q (k = m): rows ``keep``, and columns ``keep`` of
    the two projected operators -- what the driver does on the host with the H it fetched."""
    k = H.shape[0]
    cols = np.concatenate([np.flatnonzero(keep), k + np.flatnonzero(keep), np.arange(2 * k, 2 * k + m + 2 * nb)])
    return np.ascontiguousarray(H[np.flatnonzero(keep)][:, cols])


def reduce(Q, calA, calE, RU, B):
    """The reduction kernel's result in longdouble: Q^T [cal A Q | cal E Q | R U | B]."""
    Q = dm.ld(Q)
    Y = np.hstack([dm._Csr(calA).mul(Q), dm._Csr(calE).mul(Q), dm.ld(RU), dm.ld(B)])
    return Q.T @ Y


def reduce_bounds(Q, calA, calE, RU, B, u):
    """Componentwise bound on what an implementation in arithmetic of unit roundoff u may differ by from the exact H;
    first order in u, by the lengths of the inner products as radi_model.update_bounds counts them.  An entry of the
    two projected operators is a sum over the nv rows of Q[r, i] times a row sum of at most r stored entries, r the
    longest row of the common pattern of cal A and cal E (the kernel walks that pattern for both, zeros included):
    gamma_{r + nv} |Q|^T (|cal A| |Q|) whatever the order of the sums.  An entry of the dense blocks is nv summed
    products: gamma_nv |Q|^T |.|."""
    nv = np.shape(Q)[0]
    A, E = dm._Csr(calA), dm._Csr(calE)
    r = dm._Csr(abs(A.csr) + abs(E.csr)).r
    aQ = dm.fa(Q)
    sparse = dm.gamma(r + nv, u) * (aQ.T @ np.hstack([A.amul(Q), E.amul(Q)]))
    dense = dm.gamma(nv, u) * (aQ.T @ np.hstack([dm.fa(RU), dm.fa(B)]))
    return np.hstack([sparse, dense])


def hamiltonian(k, m, nb, H):
    """Ham of the module docstring from the packed H."""
    H = np.asarray(H, dtype=float).reshape(k, 2 * k + m + 2 * nb)
    HA, HE = H[:, :k], H[:, k:2 * k]
    HR, HU, HB = H[:, 2 * k:2 * k + m], H[:, 2 * k + m:2 * k + m + nb], H[:, 2 * k + m + nb:]
    At = np.linalg.solve(HE, HA - HU @ HB.T)
    Rt = np.linalg.solve(HE, HR)
    return np.block([[At.T, -HB @ HB.T], [-Rt @ Rt.T, -At]])


def null_vector(M):
    """The null vector of a numerically singular square matrix: Gaussian elimination with complete pivoting in extended
    precision (complex longdouble), the last pivot taken as zero, back substitution."""
    A = np.array(M, dtype=np.clongdouble)
    n = A.shape[0]
    cols = np.arange(n)
    for c in range(n - 1):
        sub = np.abs(A[c:, c:])
        i, j = np.unravel_index(np.argmax(sub), sub.shape)
        i, j = i + c, j + c
        A[[c, i]] = A[[i, c]]
        A[:, [c, j]] = A[:, [j, c]]
        cols[[c, j]] = cols[[j, c]]
        if A[c, c] == 0:
            break
        A[c + 1:, c:] -= np.outer(A[c + 1:, c] / A[c, c], A[c, c:])
    y = np.zeros(n, dtype=np.clongdouble)
    y[n - 1] = 1
    for r in range(n - 2, -1, -1):
        y[r] = -(A[r, r + 1:] @ y[r + 1:]) / A[r, r] if A[r, r] != 0 else 0
    x = np.zeros(n, dtype=np.clongdouble)
    x[cols] = y
    return x


def select(k, m, nb, H):
    """(p, margin, eigenvalues of Ham, criterion values sorted descending): the rule on a packed H.  p = 0.0 without
    a candidate.  The eigenvalues are LAPACK's; the eigenvector of a candidate is the null vector of Ham - lambda I
    in extended precision, not LAPACK's: late in an iteration R~ R~^T is tiny against the other blocks of Ham, the lower
    half q of an eigenvector with it, and ``eig`` returns it to an ABSOLUTE accuracy of the rounding unit -- criterion
    values wrong by up to 2.8e-7 (relative) on the N = 8 test runs, against an eigendecomposition in 50 digits that
    the null vectors reproduce within 1e-14."""
    Ham = hamiltonian(k, m, nb, H)
    lam = np.linalg.eigvals(Ham)
    cands = [i for i in range(lam.size) if lam[i].real < 0 and lam[i].imag >= 0]      # (LAPACK pairs are exact conjugates)
    if not cands:
        return 0.0, np.inf, lam, np.zeros(0)
    HamL = np.asarray(Ham, dtype=np.longdouble)
    crit = []
    for i in cands:
        x = null_vector(HamL - np.clongdouble(lam[i]) * np.eye(2 * k, dtype=np.longdouble))
        crit.append(float(np.sqrt(np.sum(np.abs(x[k:]) ** 2) / np.sum(np.abs(x) ** 2))))
    crit = np.array(crit)
    order = np.argsort(-crit)
    best = cands[order[0]]
    margin = np.inf if len(cands) == 1 else crit[order[0]] / max(crit[order[1]], 1e-300)
    return -abs(lam[best]), margin, lam, crit[order]


def initial_shift(calA, calE):
    """optconpy_amd.adi_shifts.initial_shift of the operator's diagonal ratio, as the binding computes it."""
    from optconpy_amd import adi_shifts
    da, de = rm._dn(calA).diagonal(), rm._dn(calE).diagonal()
    ok = (da != 0) & (de != 0)
    return adi_shifts.initial_shift(np.abs(da[ok] / de[ok]))


def radi(calA, calE, J, B, W, fallback, old=None, max_steps=200, res_reltol=1e-10, record=None, refuse=(),
         record_full=None):
    """radi_model.radi with generated shifts: fallback[0] is the first shift, the list the fallback cycle.  Returns
    the dict of radi_model.radi plus ms (the shift of every step), margins (of every selection whose shift was used),
    fallbacks, kept (the basis size of every selection the driver makes: none after step max_steps).
    record (a list): every packed (k, m, nb, H) the run produces is appended.
    record_full (a list): (m, nb, H, Rq) with the packed H of ALL m columns of the block's Q (m x (3m + 2nb)) and the
    R of its QR -- what the device fetches; keep_columns, restrict and select turn it into the shift.
    refuse: the selection after each of these steps (1-based) counts as refused -- it is still made and recorded, and
    the next step takes the next entry of the list (ricadi_probe_radi_refuse)."""
    calA, calE, J = rm._dn(calA), rm._dn(calE), rm._dn(J)
    B, W = rm._dn(B), rm._dn(W)
    nv, m = W.shape
    nb = B.shape[1]
    R = rm.project(calE, J, W)
    U = np.zeros_like(B) if old is None else -rm._dn(old)
    rhs = np.linalg.norm(R.T @ R)
    blocks, hist, ms, margins, kept, stopped = [], [], [], [], [], "max_steps"
    refuse = set(int(v) for v in refuse)
    p, nfb, fallbacks = float(fallback[0]), 1, 0
    for j in range(max_steps):
        ms.append(p)
        V = rm.saddle_solve(calA - U @ B.T + p * calE, J, R)
        G = V.T @ B
        Y = np.eye(m) + G @ G.T
        L = np.linalg.cholesky(Y)
        blocks.append(np.sqrt(-2.0 * p) * np.linalg.solve(L, V.T).T)
        ET = calE @ ((-2.0 * p) * np.linalg.solve(Y, V.T).T)
        R = R + ET
        U = U + ET @ G
        hist.append(np.linalg.norm(R.T @ R) / rhs)
        if hist[-1] <= res_reltol:
            stopped = "res"
            break
        Q, Rq = np.linalg.qr(blocks[-1])
        keep = keep_columns(Rq)
        k = int(keep.sum())
        H = pack(Q[:, keep], calA, calE, R, U, B)
        if record is not None:
            record.append((k, m, nb, H.copy()))
        if record_full is not None:
            record_full.append((m, nb, pack(Q, calA, calE, R, U, B), Rq.copy()))
        if j + 1 < max_steps:
            kept.append(k)
        pn, margin, _, _ = select(k, m, nb, H)
        if not (np.isfinite(pn) and pn < 0.0) or (j + 1) in refuse:
            pn = float(fallback[nfb % len(fallback)])
            nfb += 1
            fallbacks += 1
        else:
            margins.append(margin)
        p = float(pn)
    Z = np.hstack(blocks)
    return dict(Z=Z, gain=U if old is None else U + rm._dn(old), res_hist=np.array(hist), steps=len(hist),
                stopped=stopped, rhs=rhs, ms=np.array(ms), margins=np.array(margins), fallbacks=fallbacks,
                kept=np.array(kept, dtype=int))


def random_instance(k, m, nb, seed):
    """A packed H with s.p.d. H_E and a stable closed loop H_A - H_U H_B^T (k x (2k + m + 2 nb)).  H_R is a tenth of
    the scale of the rest, as a residual factor that has fallen by an order of magnitude: with H_R as large as H_B a
    quarter of the instances of order 32 and 64 have their two best criterion values within 1 % of each other."""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((k, k))
    HE = M @ M.T / k + np.eye(k)
    S = rng.standard_normal((k, k))
    N = rng.standard_normal((k, k))
    # negative definite symmetric part: with s.p.d. H_E the pencil (A_c, H_E) is stable
    Ac = 0.5 * (S - S.T) - (N @ np.diag(np.logspace(-1, 1, k)) @ N.T) / k - 0.1 * np.eye(k)
    HR = 0.1 * rng.standard_normal((k, m))
    HU = 0.3 * rng.standard_normal((k, nb))
    HB = rng.standard_normal((k, nb))
    HA = Ac + HU @ HB.T
    return np.hstack([HA, HE, HR, HU, HB])
