"""FP64 model of the preconditioner cycle, in SciPy, for the parity tests of the device cycle.

Written from the mathematics, not from the kernels.  The operator of a level is
``S(alpha, beta) = [[beta calA + alpha calE, J^T], [J, 0]]``; the structure of a level (block partitions,
aggregates, prolongation P) is what ``Context.precond_structure`` returns, or one built by hand with the same
keys.  Y is plain aggregation (one unit entry per dof, ``aggof``); P is Y or the smoothed prolongation.

Folded two-level cycle (coarse correction first, then one consistent SIMPLE block-Jacobi sweep)::

    e    = E^-1 P^T r                    E = P^T S P   (dense inverse; or the child level's cycle on E)
    rho  = r - S P e
    z_v1 = Ahat^-1 rho_v + (P - Y)_v e   Ahat = block diagonal of beta calA + alpha calE (velocity blocks)
    t    = J z_v1 - rho_p,  z_p = Shat^-1 t   Shat = block diagonal of J Ahat^-1 J^T (pressure blocks)
    z    = Y e + [z_v1 - Ahat^-1 J^T z_p ; z_p]

Unfolded cycle (no pressure rows, or no dense first-sweep operands; the device takes it with P = Y only):
``z = P e + SIMPLE(r - S P e)``; with
np = 0 SIMPLE is the velocity block sweep alone.  Without a coarse space the cycle is SIMPLE(r).

Where the device differs from the formulas above, the device decides; the model follows it:

* The Schur blocks are formed from the FP64 block inverses (never from their rounded copies), and the
  products ``Ahat_b^-1 D_b - T_b`` (D = S P, T = P - Y, velocity rows) and ``Ahat_b^-1 J^T[rows_b, .]`` are
  formed in FP64 from them as well; each is rounded once, where it is stored.
* The first sweep applies ``Ahat^-1 r_v - (Ahat^-1 D - T) e``: the residual's velocity rows are never formed.
* Where the last sweep has no dense rectangles (structure ``rect`` false) it applies the block inverse to
  ``(J^T z_p)`` formed in FP64; the rounded operand is then ``Ahat_b^-1`` itself.
* The child level is handed the restricted residual in FP64 and returns FP64; its operands are rounded as
  the level stores them (FP32 with FP32-stored operands), never to BF16, and it has no FP32 intermediate.
* The coarse inverse is the FP64 inverse rounded to FP32 where the operands are FP32-stored.
* The coarse part of z is added after the last rounding of the sweeps but before the FP32 output is rounded.

``rounded`` (dict, e.g. ``Context.decode_precond_form`` of the device's form word): rounds exactly what the
device stores reduced, where it rounds it -- the FP16 input (``h16``), the FP32 coarse inverse and block
operands (``precond32``), BF16 blocks (``b16``), the FP32 velocity intermediate (``mid32``), the FP32 output
(``x32``).  ``rounded=None``: exact FP64 arithmetic throughout.
"""
import numpy as np
import scipy.sparse as sps


# ---------------------------------------------------------------- rounding as the device stores
def to_fp16(x):
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def to_fp32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def to_bf16(x):
    """FP64 -> FP32 -> BF16, both round to nearest even (the setup's conversion kernel)."""
    u = np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32)).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _round_sparse(M, fn):
    M = M.tocsr(copy=True)
    M.data = fn(M.data)
    return M


# ---------------------------------------------------------------- structure helpers
def plain_structure(calA, calE, J, vblocks, pblocks, vagg=None, pagg=None, P=None, bs=32):
    """A structure dict from block labels (one label per dof) and aggregate labels; P defaults to Y."""
    nv = calA.shape[0]
    np_ = 0 if J is None else J.shape[0]

    def lists(lab):
        lab = np.asarray(lab)
        nb = int(lab.max()) + 1 if lab.size else 0
        order = np.argsort(lab, kind="stable").astype(np.int32)
        ptr = np.zeros(nb + 1, np.int32)
        np.add.at(ptr, lab + 1, 1)
        return np.cumsum(ptr).astype(np.int32), order, nb

    bv_ptr, bv_rows, nbv = lists(vblocks)
    bp_ptr, bp_rows, nbp = lists(pblocks) if np_ else (np.zeros(1, np.int32), np.zeros(0, np.int32), 0)
    st = dict(nv=nv, np=np_, nbv=nbv, nbp=nbp, bs=bs, bv_ptr=bv_ptr, bv_rows=bv_rows, bp_ptr=bp_ptr,
              bp_rows=bp_rows, child=False, rect=True, precond32=True)
    if vagg is None:
        st.update(kc=0, kcv=0, kcp=0, aggof=np.zeros(0, np.int32), P=None, smoothed=False, folded=False)
        return st
    kcv = int(np.max(vagg)) + 1
    kcp = int(np.max(pagg)) + 1 if np_ else 0
    aggof = np.concatenate([np.asarray(vagg), kcv + np.asarray(pagg if np_ else [], dtype=int)]).astype(np.int32)
    n = nv + np_
    Y = sps.csr_matrix((np.ones(n), (np.arange(n), aggof)), shape=(n, kcv + kcp))
    st.update(kc=kcv + kcp, kcv=kcv, kcp=kcp, aggof=aggof, P=Y if P is None else sps.csr_matrix(P),
              smoothed=P is not None, folded=np_ > 0)
    return st


# ---------------------------------------------------------------- the model
class CycleModel:
    """One level of the cycle; ``child``: the model of the next level (its operator is the Galerkin one)."""

    def __init__(self, calA, calE, J, structure, child=None):
        self.A = sps.csr_matrix(calA)
        self.E = sps.csr_matrix(calE)
        self.J = sps.csr_matrix(J) if J is not None and J.shape[0] > 0 else sps.csr_matrix((0, self.A.shape[0]))
        self.st = structure
        self.nv = self.A.shape[0]
        self.np = self.J.shape[0]
        self.n = self.nv + self.np
        self.child = child
        if structure["kc"] > 0:
            agg = np.asarray(structure["aggof"])
            self.Y = sps.csr_matrix((np.ones(self.n), (np.arange(self.n), agg)), shape=(self.n, structure["kc"]))
            self.P = sps.csr_matrix(structure["P"]) if structure["P"] is not None else self.Y
        self._cache = {}

    @classmethod
    def from_context(cls, ctx, calA, calE, J, level=0):
        """Model of a device context's cycle: the structure of every level from ``ctx.precond_structure``; a
        child level's operator is the parent's Galerkin operator with plain aggregation."""
        st = ctx.precond_structure(level)
        child = None
        if st["child"]:
            kcv = st["kcv"]
            agg = np.asarray(st["aggof"])
            Yv = sps.csr_matrix((np.ones(st["nv"]), (np.arange(st["nv"]), agg[:st["nv"]])), shape=(st["nv"], kcv))
            Yp = sps.csr_matrix((np.ones(st["np"]), (np.arange(st["np"]), agg[st["nv"]:] - kcv)),
                                shape=(st["np"], st["kcp"]))
            child = cls.from_context(ctx, Yv.T @ calA @ Yv, Yv.T @ calE @ Yv, Yp.T @ J @ Yv, level + 1)
        return cls(calA, calE, J, st, child)

    def levels(self):
        return 1 + (self.child.levels() if self.child else 0)

    def saddle(self, alpha, beta):
        K = (beta * self.A + alpha * self.E).tocsr()
        if self.np == 0:
            return K
        return sps.bmat([[K, self.J.T], [self.J, None]], format="csr")

    # -- per-shift operands, FP64 (as the setup forms them)
    def operands(self, alpha, beta):
        key = (alpha, beta)
        if key in self._cache:
            return self._cache[key]
        st, nv = self.st, self.nv
        K = (beta * self.A + alpha * self.E).tocsr()
        S = self.saddle(alpha, beta)
        conds = [1.0]
        rr, cc, vv = [], [], []
        for b in range(st["nbv"]):
            rows = np.asarray(st["bv_rows"][st["bv_ptr"][b]:st["bv_ptr"][b + 1]])
            Kb = K[rows][:, rows].toarray()
            Ib = np.linalg.inv(Kb)
            conds.append(np.linalg.cond(Kb))
            rr.append(np.repeat(rows, len(rows)))
            cc.append(np.tile(rows, len(rows)))
            vv.append(Ib.ravel())
        Ainv = sps.csr_matrix((np.concatenate(vv), (np.concatenate(rr), np.concatenate(cc))), shape=(nv, nv))
        op = dict(S=S, Ainv=Ainv, cond_blocks=max(conds))
        if self.np > 0:
            G = (Ainv @ self.J.T).tocsr()
            Sh = (self.J @ G).tocsr()
            rr, cc, vv, pc = [], [], [], [1.0]
            for b in range(st["nbp"]):
                rows = np.asarray(st["bp_rows"][st["bp_ptr"][b]:st["bp_ptr"][b + 1]])
                Sb = Sh[rows][:, rows].toarray()
                pc.append(np.linalg.cond(Sb))
                Ib = np.linalg.inv(Sb)
                rr.append(np.repeat(rows, len(rows)))
                cc.append(np.tile(rows, len(rows)))
                vv.append(Ib.ravel())
            op["Sinv"] = sps.csr_matrix((np.concatenate(vv), (np.concatenate(rr), np.concatenate(cc))),
                                        shape=(self.np, self.np))
            op["G"] = G
            op["cond_schur"] = max(pc)
        if st["kc"] > 0:
            SP = (S @ self.P).tocsr()
            op["SP"] = SP
            Ec = (self.P.T @ SP).toarray()
            op["cond_coarse"] = np.linalg.cond(Ec)
            if self.child is None:
                op["Einv"] = np.linalg.inv(Ec)
            if self.np > 0:
                T = (self.P - self.Y)[:nv].tocsr()
                op["W"] = (Ainv @ SP[:nv] - T).tocsr()      # Ahat^-1 D - T
                op["PmY"] = T
        self._cache[key] = op
        return op

    def conditioning(self, alpha, beta):
        """Largest condition number among the operands the cycle inverts, on every level: the factor by which
        the FP64 round-off of two independent implementations of this cycle may differ."""
        op = self.operands(alpha, beta)
        k = max(op["cond_blocks"], op.get("cond_schur", 1.0), op.get("cond_coarse", 1.0))
        if self.child is not None:
            k = max(k, self.child.conditioning(alpha, beta))
        return k

    def apply(self, alpha, beta, R, rounded=None, folded=None):
        """Z = P^-1 R (n x m).  ``rounded``: dict of the reduced storage in use (module docstring).
        ``folded``: force the folded (True) or unfolded (False) cycle; default: the structure's."""
        R = np.asarray(R, dtype=np.float64)
        if R.ndim == 1:
            R = R[:, None]
        rd = dict(rounded or {})
        st, nv = self.st, self.nv
        op = self.operands(alpha, beta)
        p32 = bool(rd) and st.get("precond32", True)
        blk = to_bf16 if rd.get("b16") else to_fp32 if p32 else None
        rnd = (lambda M: _round_sparse(M, blk)) if blk else (lambda M: M)
        mid = to_fp32 if rd.get("mid32") else (lambda x: x)
        if rd.get("h16"):
            R = to_fp16(R)
        kc = st["kc"]
        fold = (st["folded"] if folded is None else folded) and kc > 0 and self.np > 0
        z = np.zeros_like(R)
        if kc > 0:
            rc = self.P.T @ R
            if self.child is not None:
                # the child level: FP64 in and out, its own FP32 operands where the parent's are FP32-stored
                e = self.child.apply(alpha, beta, rc, rounded=dict(precond32=True) if p32 else None)
            else:
                Einv = to_fp32(op["Einv"]) if p32 else op["Einv"]
                e = Einv @ rc
            SPe = op["SP"] @ e
            Ye = (self.Y if fold else self.P) @ e      # the unfolded cycle prolongates with P itself
        else:
            SPe = Ye = e = 0.0
        Ainv = rnd(op["Ainv"])
        if fold:
            zv = mid(Ainv @ R[:nv] - rnd(op["W"]) @ e)
            rho_p = R[nv:] - SPe[nv:]
        else:
            rho = R - SPe
            zv = Ainv @ rho[:nv]
            rho_p = rho[nv:]
        if self.np > 0:
            t = self.J @ zv - rho_p
            zp = rnd(op["Sinv"]) @ t
            if st.get("rect", True):
                zv = zv - rnd(op["G"]) @ zp
            else:
                zv = zv - Ainv @ (self.J.T @ zp)
            z[:nv], z[nv:] = zv, zp
        else:
            z[:] = zv
        z = z + Ye
        if rd.get("x32"):
            z = to_fp32(z)
        return z


# ---------------------------------------------------------------- the comparison metric
def block_errors(Z, Zref, structure):
    """Per column, the largest relative error over the velocity and pressure blocks, ||D_b|| / ||Zref_b||.  A global
    norm would hide one wrong block.  A block whose reference nearly cancels is measured against 1e-3 of its share
    of the column, ||Zref|| sqrt(|b| / n), instead of its own norm."""
    Z = np.asarray(Z, dtype=np.float64).reshape(Zref.shape[0], -1)
    Zref = np.asarray(Zref, dtype=np.float64).reshape(Z.shape)
    nv = structure["nv"]
    col = np.linalg.norm(Zref, axis=0)
    worst = np.zeros(Z.shape[1])
    for ptr, rows, off in ((structure["bv_ptr"], structure["bv_rows"], 0),
                           (structure["bp_ptr"], structure["bp_rows"], nv)):
        for b in range(len(ptr) - 1):
            idx = off + np.asarray(rows[ptr[b]:ptr[b + 1]])
            d = np.linalg.norm(Z[idx] - Zref[idx], axis=0)
            ref = np.maximum(np.linalg.norm(Zref[idx], axis=0), 1e-3 * col * np.sqrt(len(idx) / Z.shape[0]))
            worst = np.maximum(worst, np.where(np.isfinite(d), d / np.maximum(ref, 1e-300), np.inf))
    return worst


def worst_block_error(Z, Zref, structure):
    return float(np.max(block_errors(Z, Zref, structure)))


# ---------------------------------------------------------------- tolerances of the parity tests
EPS64 = np.finfo(np.float64).eps
# Reduced forms against the rounded model: the same operands rounded at the same points, FP64 arithmetic on both
# sides -- what remains is FP64 round-off (amplified by the conditioning, tol_fp64) and the odd FP32 rounding of an
# intermediate that the two sides' FP64 values put on different sides of a rounding boundary (one FP32 ulp, 6e-8).
# 1e-5 is two orders of magnitude above that and two below the FP16 rounding of the input.
TOL_ROUNDED = 1e-5
# Reduced forms against the exact model, per COLUMN (column_errors): BF16 blocks carry 2^-9 relative rounding per
# entry, the FP16 input 2^-11; through the cycle that is ~1e-3 of a column at cfg1 (test_precond_model_cpu.py) and
# 1.5e-2 at N = 30, shift 1 (the rounded model there agrees with the device to TOL_ROUNDED per block).  Per
# block it is not a bound: where the coarse correction and the sweeps nearly cancel, a BF16-rounded cycle differs from
# the exact one by the block's own size -- the per-block check of the reduced forms is the one against the rounded
# model.
TOL_BF16 = 5e-2


def column_errors(Z, Zref):
    Z = np.asarray(Z, dtype=np.float64).reshape(Zref.shape[0], -1)
    return np.linalg.norm(Z - Zref, axis=0) / np.linalg.norm(Zref, axis=0)


def tol_fp64(model, alpha, beta):
    """FP64 forms against the exact model: round-off of two implementations of the same cycle, which differ by the
    condition numbers of what they invert (model.conditioning), with a factor 1e3 for the accumulation."""
    return max(1e-12, 1e3 * EPS64 * model.conditioning(alpha, beta))
