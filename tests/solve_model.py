"""FP64 model of what the batched shift solve (solver_gmres.inl, gmres_core_any down to solve_batch) promises, written
from the mathematics and the documentation in include/ricadi.h, not from the code.

* ``closed_loop``: the operator  [[beta A + p E - U V^T, J^T], [J, 0]]  and its sparse LU.
* ``relres``: per-column relative residuals of a returned panel, evaluated in FP64 on the host.
* ``RecycleRing``: the recycled initial guess.  The context keeps the last ``depth`` shared right-hand sides; every
  shift keeps its solutions for the right-hand sides still in the ring; a solve of a set of shifts starts from
  ``x_g = sum_e Y_{g,e} C_e`` with ``C = argmin || b - [B_e] C ||_F`` over the entries e every shift of the call has
  a solution for -- and from zero when there is none.
* ``smw``: the Sherman-Morrison-Woodbury solution from the LU of the plain operator.

Allowance of a recycled guess against this model (``guess_allowance``): the library forms the normal equations, whose
solution carries  eps * kappa([B_e])^2  relative error where an orthogonal factorisation carries eps * kappa; with the
suite's usual factor for the length of the sums (``tol_fp64``: 1e3 * eps * cond) that is  1e3 * kappa^2 * 2^-53
relative to ||x_model||_F per group.
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sps
import scipy.sparse.linalg as spla

EPS = 2.0 ** -53
LU_TOL = 1e-8          # the suite's agreement of a GMRES solution with a sparse LU's


class DenseLU:
    """LAPACK LU with partial pivoting behind the interface of ``splu`` (``shape``, ``solve``)."""

    def __init__(self, S):
        self.shape = S.shape
        self._lu = sla.lu_factor(S.toarray() if sps.issparse(S) else np.asarray(S))

    def solve(self, B):
        return sla.lu_solve(self._lu, B)


def closed_loop(calA, calE, J, p, beta=1.0, U=None, V=None):
    """``(S, lu)``: the SciPy matrix S = [[beta calA + p calE - U V^T, J^T], [J, 0]] (CSC) and an LU of it with
    ``solve`` -- ``scipy.sparse.linalg.splu`` for the plain operator; with a low-rank term the NV x NV block is dense,
    where SuperLU takes 1.1 s per factorisation and 0.4 s per 16-column solve at NV = 1682 and LAPACK's LU of the
    same matrix 0.1 s and a few ms."""
    K = sps.csc_matrix(beta * calA + p * calE)
    lowrank = U is not None and np.asarray(U).shape[1] > 0
    if lowrank:
        K = sps.csc_matrix(K.toarray() - np.asarray(U) @ np.asarray(V).T)
    S = sps.bmat([[K, J.T], [J, None]], format="csc") if J is not None and J.shape[0] else K
    return S, (DenseLU(S) if lowrank else spla.splu(S))


def pad(B, n):
    """An NV x m right-hand side as an n x m panel (pressure rows zero)."""
    B = np.asarray(B, dtype=np.float64)
    if B.shape[0] == n:
        return B
    out = np.zeros((n, B.shape[1]))
    out[:B.shape[0]] = B
    return out


def relres(S, X, B):
    """||b_j - S x_j|| / ||b_j|| per column in FP64 (0 for a zero column of B)."""
    Bn = pad(B, S.shape[0])
    r = np.linalg.norm(Bn - S @ X, axis=0)
    bn = np.linalg.norm(Bn, axis=0)
    return np.where(bn > 0, r / np.where(bn > 0, bn, 1.0), 0.0)


def lu_solve(S, lu, B):
    """S^-1 [B; 0] from the sparse LU with one step of iterative refinement (the closed-loop matrix holds a dense
    NV x NV block; the first solution leaves up to 1e-12 there, the refined one a few 1e-14)."""
    Bn = pad(B, S.shape[0])
    X = lu.solve(Bn)
    return X + lu.solve(Bn - S @ X)


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def lstsq64(Bmat, b):
    """argmin ||b - Bmat C||_F by an orthogonal factorisation (LAPACK gelsd): minimum-norm where rank deficient."""
    return np.linalg.lstsq(Bmat, b, rcond=None)[0]


def guess_allowance(Bmat):
    """``(allowance, kappa)`` for "guess equals model" with the stored columns ``Bmat`` of full rank."""
    s = np.linalg.svd(Bmat, compute_uv=False)
    kappa = s[0] / s[-1]
    return 1e3 * kappa ** 2 * EPS, kappa


class RecycleRing:
    """The documented semantics of ``ricadi_set_recycle(depth)``, fed with the right-hand sides a test passed in and the
    solutions the solver returned."""

    def __init__(self, depth):
        self.depth = depth
        self.ring = []              # [(serial, B)], oldest first
        self.sol = {}               # shift -> {serial: Y}
        self.serial = 0

    def set_depth(self, depth):
        self.depth = depth

    def clear(self):
        self.ring = []
        self.sol = {}

    def store(self, shifts, b, Y):
        """A solve of ``shifts`` (hashable keys) with the shared right-hand side ``b`` returned the panels ``Y[g]``."""
        self.serial += 1
        self.ring.append((self.serial, np.array(b, dtype=np.float64)))
        for s, y in zip(shifts, Y):
            self.sol.setdefault(s, {})[self.serial] = np.array(y, dtype=np.float64)

    def entries(self, shifts):
        """The (serial, B) a solve of ``shifts`` may use: the last ``depth`` right-hand sides, as far as every shift
        has a solution for them."""
        live = self.ring[-self.depth:] if self.depth > 0 else []
        return [(k, B) for k, B in live if all(k in self.sol.get(s, {}) for s in shifts)]

    def guess(self, shifts, b):
        """``None`` (no guess) or a dict: ``X`` the guesses per shift, ``cols`` the stored columns used, ``B`` those
        columns side by side, ``C`` the coefficients."""
        ent = self.entries(shifts)
        if not ent:
            return None
        Bmat = np.hstack([B for _, B in ent])
        C = lstsq64(Bmat, np.asarray(b, dtype=np.float64))
        X = []
        for s in shifts:
            Ymat = np.hstack([self.sol[s][k] for k, _ in ent])
            X.append(Ymat @ C)
        return dict(X=X, cols=Bmat.shape[1], B=Bmat, C=C, serials=[k for k, _ in ent])


def normal_equations_guess(Bs, Ys, b, mirror=True):
    """The guess the way a float64 implementation of the library's method computes it: Gram matrix of the stored panels
    block by block (upper blocks computed, lower ones mirrored), scaled to unit diagonal, Cholesky.  ``Bs``: the stored
    right-hand sides, ``Ys[g]``: the matching solutions of shift g.  ``mirror=False`` leaves the blocks below the
    diagonal zero (a fault the CPU test injects)."""
    w = [B.shape[1] for B in Bs]
    off = np.concatenate([[0], np.cumsum(w)])
    h = off[-1]
    G = np.zeros((h, h))
    for i, Bi in enumerate(Bs):
        for j in range(i, len(Bs)):
            blk = Bi.T @ Bs[j]
            G[off[i]:off[i + 1], off[j]:off[j + 1]] = blk
            if mirror and j > i:
                G[off[j]:off[j + 1], off[i]:off[i + 1]] = blk.T
    rhs = np.vstack([Bi.T @ b for Bi in Bs])
    d = 1.0 / np.sqrt(np.diag(G))
    Gs = G * d[:, None] * d[None, :]
    C = d[:, None] * np.linalg.solve(Gs, d[:, None] * rhs)
    return [np.hstack(Yg) @ C for Yg in Ys]


def smw(lu_plain, U, V, b, n=None, tail=None):
    """Woodbury solution of (S - [U;0][V;0]^T) x = [b;0] from the LU of the plain S:
    x = y + Z (I - V^T Z)^-1 V^T y,  y = S^-1 b,  Z = S^-1 [U;0].  ``tail``: pressure rows of the augmented columns
    (a fault the CPU test injects; they are zero)."""
    nv, q = U.shape
    n = n or lu_plain.shape[0]
    y = lu_plain.solve(pad(b, n))
    Ua = pad(U, n).copy()
    if tail is not None:
        Ua[nv:] = tail
    Z = lu_plain.solve(Ua)
    cap = np.eye(q) - V.T @ Z[:nv]
    return y + Z @ np.linalg.solve(cap, V.T @ y[:nv]), Z, cap


def woodbury_w(Z, cap):
    """The cached W = S^-1 [U;0] (I - V^T S^-1 U)^-1."""
    return Z @ np.linalg.inv(cap)
