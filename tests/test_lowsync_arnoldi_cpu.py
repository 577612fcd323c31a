"""NumPy model of the one-reduction (delayed CGS2) Arnoldi of the lockstep GMRES (ricadi_arnoldi.hip, K3L) against
the same flexible GMRES in its three-pass CGS2 form, on the cfg1 saddle operator with an incomplete-LU preconditioner.

One column, exactly the recurrence of the kernels: slot j holds the candidate u_j (projected once, scaled by 1/rho),
the dots give s = V^T u, alpha, t = V^T w, beta, ||w||^2, column j-1 of H~ is completed one iteration late with
p_{j-1} + rho_{j-1} [s; r_j], the host's convergence test reads the provisional estimate one iteration behind, the
last column of a cycle is completed by an end-of-cycle pass.  Storage of u / v in FP16 and of w in FP32 is emulated
on request; the arithmetic is FP64.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

TINY = 1e-300


def _q(x, dt):
    return x.astype(dt).astype(np.float64)


def _rot_apply(cs, sn, col, upto):
    col = col.copy()
    for i in range(upto):
        a, b = col[i], col[i + 1]
        col[i], col[i + 1] = cs[i] * a + sn[i] * b, -sn[i] * a + cs[i] * b
    return col


def _new_rot(a, b):
    d = np.hypot(a, b)
    return (a / d, b / d, d) if d > TINY else (1.0, 0.0, 0.0)


def gmres_model(S, P, b, tol, restart, form, basis_dt=np.float64, w_dt=np.float64, maxit=400, stop=True,
                relations=None):
    """Flexible right-preconditioned GMRES for one column; returns (x, iterations)."""
    n = b.size
    bn = np.linalg.norm(b)
    thr = 0.01 * tol * bn
    x = np.zeros(n)
    its = 0
    while True:
        r = b - S @ x
        beta = np.linalg.norm(r)
        if beta <= tol * bn or its >= maxit:
            return x, its
        V = np.zeros((n, restart + 1))
        Z = np.zeros((n, restart))
        Hraw = np.zeros((restart + 1, restart))     # H~ as completed (unrotated)
        R = np.zeros((restart + 1, restart))        # its rotated form
        cs, sn = np.zeros(restart), np.zeros(restart)
        g = np.zeros(restart + 1)
        g[0] = beta
        V[:, 0] = _q(r / beta, basis_dt)
        est = []
        pend = None                                  # (p_{j-1}, rho_{j-1}, g_{j-1})
        k = 0

        def complete(j, s, rr):
            # column j-1 of H~ from the pending column and the delayed correction of u_j
            p, rho, gj = pend
            sub = rho * rr
            dead = not (sub > TINY) or abs(gj) <= thr
            col = np.zeros(restart + 1)
            col[:j] = p + rho * s
            col[j] = 0.0 if dead else sub
            Hraw[:, j - 1] = col
            col = _rot_apply(cs, sn, col, j - 1)
            c, s_, d = _new_rot(col[j - 1], col[j])
            cs[j - 1], sn[j - 1] = c, s_
            col[j - 1], col[j] = (d if d > TINY else 1.0), 0.0
            R[:, j - 1] = col
            gj1 = g[j - 1]
            g[j], g[j - 1] = (-s_ * gj1, c * gj1) if d > TINY else (0.0, 0.0)
            return dead

        for j in range(restart):
            z = P(V[:, j])
            Z[:, j] = z
            w = _q(S @ z, w_dt)
            if form == "cgs2":
                h1 = V[:, :j + 1].T @ w
                w1 = w - V[:, :j + 1] @ h1
                h2 = V[:, :j + 1].T @ w1
                hn2 = w1 @ w1 - h2 @ h2
                hnext = np.sqrt(hn2) if hn2 > 0 else 0.0
                gj = g[j]
                if not (hnext > TINY) or abs(gj) <= thr:
                    hnext = 0.0
                col = np.zeros(restart + 1)
                col[:j + 1] = h1 + h2
                col[j + 1] = hnext
                Hraw[:, j] = col
                col = _rot_apply(cs, sn, col, j)
                c, s_, d = _new_rot(col[j], hnext)
                cs[j], sn[j] = c, s_
                col[j], col[j + 1] = (d if d > TINY else 1.0), 0.0
                R[:, j] = col
                g[j + 1], g[j] = (-s_ * gj, c * gj) if d > TINY else (0.0, 0.0)
                est.append(abs(g[j + 1]))
                scale = 1.0 / hnext if hnext > TINY else 0.0
                V[:, j + 1] = _q((w - V[:, :j + 1] @ (h1 + h2)) * scale, basis_dt)
            else:
                u = V[:, j]
                Vp = V[:, :j]
                s, t = Vp.T @ u, Vp.T @ w
                alpha, bet, ww = u @ u, u @ w, w @ w
                dead, rr = False, 1.0
                if j > 0:
                    r2 = alpha - s @ s
                    rr = np.sqrt(r2) if r2 > 0 else 0.0
                    dead = complete(j, s, rr)
                invr = 1.0 / rr if (not dead and rr > TINY) else 0.0
                hjj = (bet - s @ t) * invr
                rho2 = ww - t @ t - hjj * hjj
                rho = max(np.sqrt(rho2) if rho2 > 0 else 0.0, 1e-3 * np.sqrt(max(ww, 0.0)))
                if dead or not rho > TINY:
                    rho = 0.0
                hjj = 0.0 if dead else hjj
                p = np.zeros(j + 1) if dead else np.append(t, hjj)
                gj = g[j]
                pend = (p, rho, gj)
                # provisional estimate for column j (s' = 0, r' = 1)
                col = np.zeros(restart + 1)
                col[:j + 1] = p
                sub = 0.0 if (dead or abs(gj) <= thr) else rho
                col = _rot_apply(cs, sn, col, j)
                d = np.hypot(col[j], sub)
                est.append(abs(sub / d * gj) if d > TINY else 0.0)
                v = _q((u - Vp @ s) * invr, basis_dt)
                V[:, j] = v
                sig = 1.0 / rho if rho > 0 else 0.0
                V[:, j + 1] = _q((w - Vp @ t - v * hjj) * sig, basis_dt)
            its += 1
            k = j + 1
            # the host reads the previous iteration's estimate (one iteration of lag)
            if stop and j >= 1 and est[j - 1] <= tol * bn:
                break
            if its >= maxit:
                break
        if form != "cgs2":
            # end-of-cycle pass: completes column k-1 from u_k
            u = V[:, k]
            s = V[:, :k].T @ u
            r2 = u @ u - s @ s
            rr = np.sqrt(r2) if r2 > 0 else 0.0
            complete(k, s, rr)
            V[:, k] = (u - V[:, :k] @ s) / rr if rr > TINY else 0.0
        if relations is not None:
            relations.append((S @ Z[:, :k], V[:, :k + 1] @ Hraw[:k + 1, :k]))
        y = np.linalg.solve(np.triu(R[:k, :k]), g[:k])
        x = x + Z[:, :k] @ y


@pytest.fixture(scope="module")
def saddle(cfg1):
    pr = cfg1[0]
    calA = (-pr.A - pr.Nc).T.tocsr()
    MT = pr.M.T.tocsr()
    p = -30.0
    K = (calA + p * MT).tocsr()
    J = sp.csr_matrix(pr.J)
    S = sp.bmat([[K, J.T], [J, None]]).tocsr()
    Sp = sp.bmat([[K, J.T], [J, -1e-6 * sp.identity(pr.NP)]]).tocsc()
    ilu = spla.spilu(Sp, drop_tol=1e-3, fill_factor=8)
    rng = np.random.default_rng(7)
    b = np.zeros(pr.NV + pr.NP)
    b[:pr.NV] = rng.standard_normal(pr.NV)
    return S, ilu.solve, b


def _true_relres(S, b, x):
    return np.linalg.norm(b - S @ x) / np.linalg.norm(b)


def test_arnoldi_relation_holds_exactly_in_fp64(saddle):
    """With FP64 storage every completed column satisfies S z_j = V_{j+1} h~_j to rounding level, in both forms."""
    S, P, b = saddle
    for form in ("lowsync", "cgs2"):
        rel = []
        gmres_model(S, P, b, 1e-10, 30, form, relations=rel)
        for SZ, VH in rel:
            assert np.linalg.norm(SZ - VH) <= 1e-12 * np.linalg.norm(SZ), form


def test_iteration_counts_match_cgs2(saddle):
    """Tolerance 1e-10: the one-reduction form needs the CGS2 form's iterations within one (FP64 storage) and
    within two with the hot path's storage (FP16 basis, FP32 w); both reach the tolerance in the true residual."""
    S, P, b = saddle
    x1, i1 = gmres_model(S, P, b, 1e-10, 30, "lowsync")
    x2, i2 = gmres_model(S, P, b, 1e-10, 30, "cgs2")
    assert abs(i1 - i2) <= 1, (i1, i2)
    assert _true_relres(S, b, x1) <= 1e-10 and _true_relres(S, b, x2) <= 1e-10
    x1, i1 = gmres_model(S, P, b, 1e-10, 30, "lowsync", np.float16, np.float32)
    x2, i2 = gmres_model(S, P, b, 1e-10, 30, "cgs2", np.float16, np.float32)
    assert abs(i1 - i2) <= 2, (i1, i2)
    assert _true_relres(S, b, x1) <= 1e-10 and _true_relres(S, b, x2) <= 1e-10


def test_restart_cycle_boundaries(saddle):
    """Cycles of 3: every cycle ends in the end-of-cycle pass; the relation holds for each and the solve converges
    within a few iterations of CGS2."""
    S, P, b = saddle
    rel = []
    x1, i1 = gmres_model(S, P, b, 1e-10, 3, "lowsync", relations=rel)
    x2, i2 = gmres_model(S, P, b, 1e-10, 3, "cgs2")
    assert len(rel) >= 3
    for SZ, VH in rel:
        assert np.linalg.norm(SZ - VH) <= 1e-12 * np.linalg.norm(SZ)
    assert _true_relres(S, b, x1) <= 1e-10
    assert abs(i1 - i2) <= 3, (i1, i2)


def test_a_column_that_freezes_early(saddle):
    """A column kept iterating after it has converged (the lockstep batch waits for its slowest column) freezes:
    the column after the frozen one is inert, the solution keeps its accuracy; a zero right-hand side stays zero."""
    S, P, b = saddle
    x_ref, i_ref = gmres_model(S, P, b, 1e-10, 30, "lowsync")
    assert i_ref < 25
    x, its = gmres_model(S, P, b, 1e-10, 30, "lowsync", maxit=30, stop=False)
    assert its == 30
    assert np.all(np.isfinite(x))
    # the iterations after the freeze change nothing: one full cycle reaches the tolerance in the true residual
    assert _true_relres(S, b, x) <= 1e-10
    z, its0 = gmres_model(S, P, np.zeros_like(b), 1e-10, 30, "lowsync")
    assert its0 == 0 and not z.any()
