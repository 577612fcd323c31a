"""Dense FP64 model of the low-rank ADI's residual history and of its two stopping rules.

The recurrence of ``lyap_adi_dev`` (optconpy_amd/csrc/solver_adi.inl) for

    cal A X cal E^T + cal E X cal A^T + W W^T = 0   on ker J,

with every shift solve done exactly on an orthonormal basis ``Theta`` of ker J (``scipy.linalg.null_space``, as
``tests/identities.dense_projected_are``): ``S(p) [V; *] = [W; 0]`` is ``V = Theta (Theta^T (cal A + p cal E) Theta)^-1
Theta^T W``.  Nothing is shared with the library or with oracle/.

  step form    V_j = solve(p_j, W_{j-1});  W_j = W_{j-1} - 2 p_j cal E V_j;  Z <- [Z, sqrt(-2 p_j) V_j]
  history      h_j = ||W_j^T W_j||_F / ||W_0^T W_0||_F          (W_0 the right-hand side after the projection)
  newZ rule    r_j = ||Z_j||_F / ||[Z_1 .. Z_j]||_F < adi_newZ_reltol       (the reference's)
  res rule     h_j <= adi_res_reltol

  sweep form   G solves against the SAME W; after the first j blocks the residual factor is
               W + cal E sum_{i<=j} c_i U_i,  c = C_j^-1 1,  C_j the leading j x j block of C_ik = -1/(p_i + p_k):
               all prefix norms from ONE Gram matrix of [W, cal E U_1, .., cal E U_G].
"""
import numpy as np
import scipy.linalg as sla


def _dn(a):
    return a.toarray() if hasattr(a, "toarray") else np.asarray(a, dtype=float)


def cauchy_numpy(ps):
    """``(None, C^-1 1)`` of the Cauchy matrix ``C_ik = -1 / (p_i + p_k)``, by a dense solve."""
    ps = np.asarray(ps, dtype=float)
    C = -1.0 / (ps[:, None] + ps[None, :])
    return None, np.linalg.solve(C, np.ones(ps.size))


def gram_fro(W):
    return float(np.linalg.norm(W.T @ W))


class AdiResModel:
    def __init__(self, calA, calE, J):
        self.A, self.E = _dn(calA), _dn(calE)
        self.Th = sla.null_space(_dn(J))
        self.Ah = self.Th.T @ self.A @ self.Th
        self.Eh = self.Th.T @ self.E @ self.Th
        self._lu = {}

    def project(self, W):
        """``P^T W`` as the library forms it: one saddle solve with cal E, then cal E times the solution."""
        return self.E @ (self.Th @ np.linalg.solve(self.Eh, self.Th.T @ W))

    def solve(self, p, W):
        p = float(p)
        if p not in self._lu:
            self._lu[p] = sla.lu_factor(self.Ah + p * self.Eh)
        return self.Th @ sla.lu_solve(self._lu[p], self.Th.T @ W)

    def step_form(self, W0, shifts, steps):
        """``steps`` steps without any rule.  Returns dict(hist, rel_newZ, Z (list of blocks), W (list, W[j] after
        step j, W[0] = W0))."""
        W = np.array(W0, dtype=float)
        rhs = gram_fro(W)
        hist, rels, Z, Ws = [], [], [], [W.copy()]
        z2 = 0.0
        for j in range(steps):
            p = float(shifts[j % len(shifts)])
            V = self.solve(p, W)
            W = W - 2.0 * p * (self.E @ V)
            blk = np.sqrt(-2.0 * p) * V
            b2 = float(np.sum(blk * blk))
            z2 += b2
            Z.append(blk)
            Ws.append(W.copy())
            rels.append(np.sqrt(b2 / z2) if z2 > 0 else 0.0)
            hist.append(gram_fro(W) / rhs)
        return dict(hist=np.array(hist), rel_newZ=np.array(rels), Z=Z, W=Ws, rhs=rhs)

    def sweep_form_history(self, W0, shifts, G, steps, cauchy=cauchy_numpy):
        """Residual history of ``steps`` steps taken in sweeps of ``G`` shifts, every entry from the prefix formula
        on the Gram matrix of ``[W, cal E U_1, .., cal E U_G]``; ``cauchy(ps) -> (_, C^-1 1)``."""
        W = np.array(W0, dtype=float)
        m = W.shape[1]
        rhs = gram_fro(W)
        hist = []
        done = 0
        while done < steps:
            g = min(G, steps - done)
            ps = [float(shifts[(done + i) % len(shifts)]) for i in range(g)]
            T = [self.E @ self.solve(p, W) for p in ps]
            Pn = np.hstack([W] + T)
            Gm = Pn.T @ Pn
            for j in range(1, g + 1):
                c = np.asarray(cauchy(ps[:j])[1], dtype=float)
                d = np.kron(np.r_[1.0, c], np.eye(m))                # m x (j + 1) m: W_j = Pn[:, :(j + 1) m] d^T
                hist.append(float(np.linalg.norm(d @ Gm[:(j + 1) * m, :(j + 1) * m] @ d.T)) / rhs)
            c = np.asarray(cauchy(ps)[1], dtype=float)
            W = W + sum(ci * Ti for ci, Ti in zip(c, T))
            done += g
        return np.array(hist)


def stopping_step(rel_newZ, hist, newZ_reltol, res_reltol, max_steps=None):
    """(step, rule) at which the iteration with these two histories ends: the first step (1-based) where
    ``rel_newZ < newZ_reltol`` ('newZ') or, the rule being on, ``hist <= res_reltol`` ('res'); else
    ``(max_steps, 'max_steps')``.  Both firing at one step reports 'newZ', as the library does."""
    n = len(hist) if max_steps is None else min(max_steps, len(hist))
    for j in range(n):
        if rel_newZ[j] < newZ_reltol:
            return j + 1, "newZ"
        if res_reltol > 0.0 and hist[j] <= res_reltol:
            return j + 1, "res"
    return n, "max_steps"
