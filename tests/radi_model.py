"""Model of the low-rank RADI iteration for the projected Riccati equation (csrc/solver_radi.inl, ricadi_radi.hip)

    cal A X cal E^T + cal E X cal A^T - cal E X B B^T X cal E^T + W W^T = 0   on ker J,   X = Z Z^T,

in this repository's conventions (Benner, Bujanovic, Kuerschner, Saak, Numer. Math. 2018).  Plain NumPy: dense
saddle-point solves in FP64 for the whole iteration (:func:`radi`), ``np.longdouble`` for the dense update of one
step (:func:`update`) with the componentwise bounds a correct FP64 implementation satisfies (:func:`update_bounds`).

One step with the real shift p < 0, residual factor R (nv x m) and U = (gain so far) - old (nv x nb):

    [[cal A - U B^T + p cal E, J^T], [J, 0]] [V; L] = [R; 0]
    G = V^T B,   Y = I + G G^T = L L^T          (V unscaled; with Vs = sqrt(-2p) V it reads I + Gs Gs^T / (-2p))
    Z <- [Z, sqrt(-2p) V L^-T]
    T = (-2p) V Y^-1,   R <- R + cal E T,   U <- U + (cal E T) G

and the Riccati residual of Z Z^T is exactly R R^T.
"""
import numpy as np

import dense_model as dm

LD = np.longdouble


def _dn(a):
    return a.toarray() if hasattr(a, "toarray") else np.asarray(a, dtype=float)


def saddle_solve(A, J, rhs):
    """Velocity rows of the solution of [[A, J^T], [J, 0]] [x; l] = [rhs; 0] (dense LU)."""
    nv, npr = A.shape[0], J.shape[0]
    S = np.zeros((nv + npr, nv + npr))
    S[:nv, :nv] = A
    S[:nv, nv:] = J.T
    S[nv:, :nv] = J
    b = np.zeros((nv + npr, rhs.shape[1]))
    b[:nv] = rhs
    return np.linalg.solve(S, b)[:nv]


def project(calE, J, W):
    """P^T W as the library forms it: cal E x of the saddle solve with cal E."""
    return calE @ saddle_solve(calE, J, W)


def radi(calA, calE, J, B, W, shifts, old=None, max_steps=200, res_reltol=1e-10):
    """The iteration with dense saddle solves.  Returns a dict: Z (nv x steps m), gain = cal E X B (= U + old),
    res_hist (relative ||R_j^T R_j||_F after every step), steps, stopped ('res' / 'max_steps'), rhs
    (||R_0^T R_0||_F)."""
    calA, calE, J = _dn(calA), _dn(calE), _dn(J)
    B, W = _dn(B), _dn(W)
    nv, m = W.shape
    R = project(calE, J, W)
    U = np.zeros_like(B) if old is None else -_dn(old)
    rhs = np.linalg.norm(R.T @ R)
    blocks, hist, stopped = [], [], "max_steps"
    for j in range(max_steps):
        p = float(shifts[j % len(shifts)])
        V = saddle_solve(calA - U @ B.T + p * calE, J, R)
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
    Z = np.hstack(blocks)
    return dict(Z=Z, gain=U if old is None else U + _dn(old), res_hist=np.array(hist), steps=len(hist),
                stopped=stopped, rhs=rhs)


def dense_riccati_residuals(calA, calE, J, B, W, Z, m, old=None):
    """Relative Frobenius norm of the densely formed projected Riccati residual
    Pi (A_c X E^T + E X A_c^T - E X B B^T X E^T + W W^T) Pi^T,  Pi = I - J^T (J E^-1 J^T)^-1 J E^-1,  A_c = cal A + old B^T,
    of X = Z[:, :j m] Z[:, :j m]^T for every j >= 1, relative to ||Pi W W^T Pi^T||_F."""
    calA, calE, J, B, W = _dn(calA), _dn(calE), _dn(J), _dn(B), _dn(W)
    if old is not None:
        calA = calA + _dn(old) @ B.T
    EiJt = np.linalg.solve(calE, J.T)
    Pi = np.eye(calE.shape[0]) - J.T @ np.linalg.solve(J @ EiJt, np.linalg.solve(calE.T, J.T).T)
    Wp = Pi @ W
    rhs = np.linalg.norm(Wp @ Wp.T)
    out = []
    for j in range(1, Z.shape[1] // m + 1):
        Zj = Z[:, :j * m]
        AX = (calA @ Zj) @ (calE @ Zj).T
        K = calE @ (Zj @ (Zj.T @ B))
        out.append(np.linalg.norm(Pi @ (AX + AX.T - K @ K.T + W @ W.T) @ Pi.T) / rhs)
    return np.array(out)


# ---------------------------------------------------------------------------------------- one step's dense update
def update(p, V, B, RU, E):
    """The dense part of a step in longdouble.  V nv x m, B nv x nb, RU = [R | U] nv x (m + nb), E sparse.
    Returns G (m x nb), C = [sqrt(-2p) L^-T | (-2p) Y^-1 | (-2p) Y^-1 G] (m x (2m + nb)), the new [R | U] and the
    Z block sqrt(-2p) V L^-T."""
    p = LD(p)
    V, B, RU = dm.ld(V), dm.ld(B), dm.ld(RU)
    m = V.shape[1]
    G = V.T @ B
    Y = np.eye(m, dtype=LD) + G @ G.T
    L = _chol_ld(Y)
    Li = _lower_inv_ld(L)
    s2 = -2 * p
    C1 = np.sqrt(s2) * Li.T
    C2 = s2 * (Li.T @ Li)
    C = np.hstack([C1, C2, C2 @ G])
    EV = dm._Csr(E).mul(V)
    return G, C, RU + EV @ C[:, m:], V @ C1


def _chol_ld(Y):
    m = Y.shape[0]
    L = np.zeros_like(Y)
    for k in range(m):
        L[k, k] = np.sqrt(Y[k, k] - L[k, :k] @ L[k, :k])
        for i in range(k + 1, m):
            L[i, k] = (Y[i, k] - L[i, :k] @ L[k, :k]) / L[k, k]
    return L


def _lower_inv_ld(L):
    m = L.shape[0]
    X = np.zeros_like(L)
    for j in range(m):
        X[j, j] = 1 / L[j, j]
        for i in range(j + 1, m):
            X[i, j] = -(L[i, j:i] @ X[j:i, j]) / L[i, i]
    return X


def update_bounds(p, V, B, RU, E, u):
    """Componentwise bounds (G, C, new [R | U], Z block) on what an implementation in arithmetic of unit roundoff u
    may differ by from the exact result; first order in u.  Derivation, with gamma_k of dense_model, kappa = cond_2(Y)
    and the facts Y >= I (so ||Y^-1||_2 <= 1, ||L^-1||_2 <= 1) and |entry| <= 2-norm <= Frobenius norm:

      G      nv summed products: gamma_nv |V|^T |B| =: dG.
      Y      dY = |dG||G|^T + |G||dG|^T + gamma_{nb+2} |G||G|^T + u |Y|.
      L L^T  computed factor: Lh Lh^T = Yh + D1, |D1| <= gamma_{m+1} |L||L^T| (Higham, ASNA, Thm 10.3), so
             ||D1||_F <= gamma_{m+1} ||L||_F^2 = gamma_{m+1} trace(Y).
      L^-1   by substitution, column by column: L Xh = I + D2, |D2| <= gamma_m |L||Xh| (ASNA Thm 8.5), so
             ||D2||_F <= gamma_m ||L||_F ||L^-1||_F =: d2.
      C2     (-2p) Xh^T Xh, m summed products, the scaling: against Y^-1
             e2 = (-2p) [ gamma_{m+2} ||L^-1||_F^2 + 2 d2 ||Y^-1||_2 + ||Y^-1||_2^2 (||D1||_F + ||dY||_F) ].
      C1     sqrt(-2p) Xh^T.  The Cholesky factor moves with its matrix: ||dL||_F <= kappa ||L||_2 / sqrt(2) *
             (||D1||_F + ||dY||_F) / ||Y||_2 (ASNA Thm 10.8, first order), and L^-1 by ||L^-1||_2^2 ||dL||_F:
             e1 = sqrt(-2p) [ d2 ||L^-1||_2 + ||L^-1||_2^2 ||dL||_F ] + 2 u |C1|  (the scaling, the rounded root).
      C3     C2 G from the stored operands: e2 colsum|G| + |C2| dG + gamma_{m} |C2||G|.
      R, U   (E V) C: row of E (r entries), then m products, the addition:
             gamma_{r+m+2} (|E||V|) |C| + (|E||V|) dC + u |R U|.
      Z      V C1: gamma_m |V||C1| + |V| dC1.
    """
    p = float(p)
    s2 = -2.0 * p
    m, nb = np.shape(V)[1], np.shape(B)[1]
    nv = np.shape(V)[0]
    G, C, _, _ = update(p, V, B, RU, E)
    G64, C64 = np.asarray(G, dtype=np.float64), np.asarray(C, dtype=np.float64)
    aG = np.abs(G64)
    Y = np.eye(m) + G64 @ G64.T
    ev = np.linalg.eigvalsh(Y)
    kappa, ynorm = ev[-1] / ev[0], ev[-1]
    yinv2 = 1.0 / ev[0]
    linv2 = np.sqrt(yinv2)
    linvF2 = float(np.sum(1.0 / ev))              # ||L^-1||_F^2 = trace(Y^-1)
    LF2 = float(np.trace(Y))                      # ||L||_F^2
    dG = dm.gamma(nv, u) * (dm.fa(V).T @ dm.fa(B))
    dY = dG @ aG.T + aG @ dG.T + dm.gamma(nb + 2, u) * (aG @ aG.T) + u * np.abs(Y)
    dYF = float(np.linalg.norm(dY))
    D1F = dm.gamma(m + 1, u) * LF2
    d2 = dm.gamma(m, u) * np.sqrt(LF2 * linvF2)
    e2 = s2 * (dm.gamma(m + 2, u) * linvF2 + 2.0 * d2 * yinv2 + yinv2 ** 2 * (D1F + dYF))
    dL = kappa * np.sqrt(ynorm) / np.sqrt(2.0) * (D1F + dYF) / ynorm
    aC1, aC2 = np.abs(C64[:, :m]), np.abs(C64[:, m:2 * m])
    e1 = np.sqrt(s2) * (d2 * linv2 + linv2 ** 2 * dL) + 2.0 * u * aC1
    dC2 = np.full((m, m), e2)
    dC3 = dC2 @ aG + aC2 @ dG + dm.gamma(m, u) * (aC2 @ aG)
    dC = np.hstack([np.broadcast_to(e1, (m, m)), dC2, dC3])
    Ec = dm._Csr(E)
    aEV = Ec.amul(V)
    dRU = dm.gamma(Ec.r + m + 2, u) * (aEV @ np.abs(C64[:, m:])) + aEV @ dC[:, m:] + u * dm.fa(RU)
    dZ = dm.gamma(m, u) * (dm.fa(V) @ aC1) + dm.fa(V) @ dC[:, :m]
    return dG, dC, dRU, dZ


# ---------------------------------------------------------------------------------------- the small test problems
def call_forms(N, narrow=False):
    """The three call forms of the dense Riccati pin (tests/test_gpu_configs.py) at mesh size N, as a list of dicts:
    name, kw (keyword arguments of the pru call, without the options dict), calA / calE / J / B / W / old (the
    equation in the library's conventions), ms (the shift list).  narrow: the steady form with mw = 3, nb = 1."""
    from identities import dre_step_inputs
    from optconpy_amd import problems as pb
    from oracle import lin_alg_utils as olau
    forms = []
    pr = pb.ricc_problem(N, 0.2, NU=2, NY=2, alphau=1e-3)
    mct = olau.app_prj_via_sadpnt(amat=pr.M, jmat=pr.J, rhsv=pr.mc_mat.T, transposedprj=True)
    tb = olau.apply_invsqrt_fromright(pr.rmat, pr.b_mat, output="dense")
    trct = olau.apply_invsqrt_fromright(pr.y_masmat, mct, output="dense")
    if narrow:
        tb, trct = tb[:, :1], trct[:, :3]
    F = (-pr.A - pr.Nc).tocsr()
    forms.append(dict(name="narrow" if narrow else "steady", kw=dict(mmat=pr.M, amat=F, jmat=pr.J, bmat=tb, wmat=trct),
                      calA=F.T.tocsr(), calE=pr.M.T.tocsr(), J=pr.J, B=np.asarray(tb), W=np.asarray(trct), old=None,
                      ms=pb.logshifts(1.0, 2e3, 10)))
    if narrow:
        return forms
    pr = pb.ricc_problem(N, 0.2, NU=2, NY=2, alphau=1e-2)
    for with_old in (False, True):
        kw, p = dre_step_inputs(pr, tau=0.05, with_old=with_old)
        forms.append(dict(name="dre_old" if with_old else "dre", kw=kw, calA=p["ft"], calE=p["MT"], J=pr.J,
                          B=np.sqrt(p["tau"]) * np.asarray(p["tb"]), W=p["wmat"], old=kw.get("mtxoldb"),
                          ms=pb.logshifts(0.4, 60.0, 8)))
    return forms


def dense_are_of(form):
    """(X, cal E X B) of a call form from tests/identities.dense_projected_are."""
    from identities import dense_projected_are
    calA = _dn(form["calA"])
    if form["old"] is not None:
        calA = calA + _dn(form["old"]) @ form["B"].T
    X = dense_projected_are(calA, form["calE"], form["J"], form["B"], form["W"])
    return X, form["calE"] @ (X @ form["B"])
