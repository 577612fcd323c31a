"""FP64 SciPy model of a child level's cycle with the coloured Vanka sweep, for the tests of that sweep.

Written from the mathematics, not from the kernels.  The level's operator is
``S(alpha, beta) = [[beta calA + alpha calE, J^T], [J, 0]]`` on ``nv + np`` unknowns.  The cycle is unfolded::

    z = Y e,   e = E^-1 Y^T r              (the level's own coarse correction: dense inverse of E = Y^T S Y, or the
                                            next level's cycle on E; plain aggregation Y)
    for each colour c, in order:
        rho = r - S z
        z[idx_b] += omega * Inv_b * rho[idx_b]      for every patch b of colour c,  Inv_b = S[idx_b, idx_b]^-1

All patches of a colour see the iterate as it stood before that colour.  The patches (64-wide records, -1 padded,
colour by colour) are what ``Context.precond_vanka`` or ``_lib.host_vanka_patches`` return; the pseudo-patches of the
lone velocity unknowns (the last ``lone_patches`` records) apply the diagonal of S on their unknowns only.

``rounded``: rounds only what the device stores reduced on this level -- the FP32 coarse inverse and the FP32 patch
inverses, where the level's operands are FP32-stored.

``VankaModel`` is a ``precond_model.CycleModel``: pass it as the ``child`` of the parent level's model.
"""
import numpy as np
import scipy.sparse as sps

import precond_model as pm


def galerkin_keep_pattern(Yp, J, Yv):
    """``Yp^T J Yv`` with every entry the pattern product yields kept, also where the values cancel to zero: a child
    level's J as the library forms it (it never drops a stored entry)."""
    G = sps.csr_matrix(Yp.T @ J @ Yv)
    pat = sps.csr_matrix(abs(sps.csr_matrix(Yp)).T @ abs(sps.csr_matrix(J)) @ abs(sps.csr_matrix(Yv)))
    pat.sum_duplicates()
    pat.sort_indices()
    out = pat.copy()
    out.data = np.asarray(G[pat.nonzero()]).ravel()
    return out


def child_operators(st, calA, calE, J):
    """Galerkin operators of the child level of a level with structure ``st`` (plain aggregation)."""
    nv, np_, kcv, kcp = st["nv"], st["np"], st["kcv"], st["kcp"]
    agg = np.asarray(st["aggof"])
    Yv = sps.csr_matrix((np.ones(nv), (np.arange(nv), agg[:nv])), shape=(nv, kcv))
    Yp = sps.csr_matrix((np.ones(np_), (np.arange(np_), agg[nv:] - kcv)), shape=(np_, kcp))
    return (Yv.T @ calA @ Yv).tocsr(), (Yv.T @ calE @ Yv).tocsr(), galerkin_keep_pattern(Yp, J, Yv)


class VankaModel(pm.CycleModel):
    """One child level with the coloured Vanka sweep; ``patches``: dict of ``host_vanka_patches``."""

    def __init__(self, calA, calE, J, structure, patches, omega=0.7, child=None):
        super().__init__(calA, calE, J, structure, child)
        self.omega = float(omega)
        self.patches = patches
        idx = np.asarray(patches["patch_idx"]).reshape(-1, 64)
        self.records = [row[row >= 0] for row in idx]
        self.colour_ptr = np.asarray(patches["colour_ptr"])
        self.first_lone = int(patches["pressure_patches"])

    @classmethod
    def from_context(cls, ctx, calA, calE, J, level=1, omega=0.7):
        """Model of level ``level`` (>= 1) of a device context and of the levels below it: a ``VankaModel`` where the
        level smooths with the Vanka sweep, else the plain ``CycleModel``."""
        st = ctx.precond_structure(level)
        child = None
        if st["child"]:
            child = cls.from_context(ctx, *child_operators(st, calA, calE, J), level=level + 1, omega=omega)
        vp = ctx.precond_vanka(level)
        if vp["pressure_patches"] == 0:
            return pm.CycleModel(calA, calE, J, st, child)
        return cls(calA, calE, J, st, vp, omega, child)

    def operands(self, alpha, beta):
        key = (alpha, beta)
        if key in self._cache:
            return self._cache[key]
        S = self.saddle(alpha, beta).tocsr()
        Sc = S.tocsc()
        invs, conds = [], [1.0]
        for b, idx in enumerate(self.records):
            Mb = Sc[:, idx][idx].toarray()
            if b >= self.first_lone:
                Mb = np.diag(np.diag(Mb))
            conds.append(np.linalg.cond(Mb))
            invs.append(np.linalg.inv(Mb))
        op = dict(S=S, inv=invs, cond_blocks=max(conds))
        if self.st["kc"] > 0:
            SP = (S @ self.Y).tocsr()
            op["SP"] = SP
            Ec = (self.Y.T @ SP).toarray()
            op["cond_coarse"] = np.linalg.cond(Ec)
            if self.child is None:
                op["Einv"] = np.linalg.inv(Ec)
        self._cache[key] = op
        return op

    def apply(self, alpha, beta, R, rounded=None, folded=None):
        R = np.asarray(R, dtype=np.float64)
        if R.ndim == 1:
            R = R[:, None]
        op = self.operands(alpha, beta)
        p32 = bool(rounded) and self.st.get("precond32", True)
        rnd = pm.to_fp32 if p32 else (lambda x: x)
        z = np.zeros_like(R)
        if self.st["kc"] > 0:
            rc = self.Y.T @ R
            if self.child is not None:
                e = self.child.apply(alpha, beta, rc, rounded=dict(precond32=True) if p32 else None)
            else:
                e = rnd(op["Einv"]) @ rc
            z = self.Y @ e
        for c in range(len(self.colour_ptr) - 1):
            rho = R - op["S"] @ z
            for b in range(self.colour_ptr[c], self.colour_ptr[c + 1]):
                idx = self.records[b]
                z[idx] += self.omega * (rnd(op["inv"][b]) @ rho[idx])
        return z


def gmres_right(S, precond, b, tol=1e-10, maxit=400):
    """Right-preconditioned full GMRES in FP64 (modified Gram-Schmidt, no restart); returns (x, iterations, relative
    residual of the Arnoldi recurrence)."""
    b = np.asarray(b, dtype=np.float64).ravel()
    bn = np.linalg.norm(b)
    V = [b / bn]
    Z = []
    H = np.zeros((maxit + 1, maxit))
    res = 1.0
    k = 0
    y = np.zeros(0)
    for k in range(1, maxit + 1):
        zk = np.asarray(precond(V[-1])).ravel()
        w = S @ zk
        for i, v in enumerate(V):
            H[i, k - 1] = v @ w
            w = w - H[i, k - 1] * v
        H[k, k - 1] = np.linalg.norm(w)
        Z.append(zk)
        V.append(w / H[k, k - 1])
        g = np.zeros(k + 1)
        g[0] = bn
        y, *_ = np.linalg.lstsq(H[:k + 1, :k], g, rcond=None)
        res = np.linalg.norm(H[:k + 1, :k] @ y - g) / bn
        if res <= tol:
            break
    x = np.column_stack(Z) @ y
    return x, k, res
