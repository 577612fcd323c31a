"""Tiny and irregular operators ``(calA, calE, J)`` with dense FP64 references, for the tests of the whole stack below
one tile (tests/test_small_ops_cpu.py, tests/test_gpu_small_ops.py).

The synthetic operators are seeded and built so that they are valid inputs by construction:

* ``calA = -(R R^T + I + 0.3 (Q - Q^T))`` with sparse random R, Q (about 3 entries per row): the symmetric part is
  negative definite, so the pencil ``(calA, calE)`` is stable on every subspace, and the matrix is not symmetric;
* ``calE`` symmetric positive definite: a positive diagonal (lumped), or ``0.2 G G^T + diag``;
* ``J`` with a strong entry ``(k, k)`` in row k (full row rank) and a few weak ones, scaled by 10: between the shifts
  -0.1 and -1e3 the velocity block grows from 1 to 1e3, and a constraint block of size 30 keeps the saddle matrix,
  and the coarse matrices the setup forms from it, near cond 1e4 at both ends.

The variants change the PATTERN (an unsymmetric calA, a calE outside calA's pattern, velocity rows no constraint
touches, a constraint touching every velocity unknown, an arrowhead row, constraints with disjoint supports, a grid
Laplacian for ``R R^T``: the one operator the setup smooths its prolongation for), not the construction.  ``FAMILY`` names every operator; ``get(name)`` returns it (cached) as a :class:`SmallOp`, which
also carries the references: the saddle matrix and its LU, the Leray projector, the projected generalised
eigenvalues, and the dense projected Lyapunov and Riccati solutions.  Everything is NumPy / SciPy FP64; the models
of the cycle, the product and the dense step are those of precond_model, saddle_model, dense_model and identities.
"""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sps

import identities
import precond_model as pm
import saddle_model as sm
from optconpy_amd import _lib, problems as pb

SHIFTS = (-0.1, -1.0, -30.0, -1e3)      # the shifts the caps are stated for; the tests use these and (1, 0)
SHIFTS16 = tuple(-np.logspace(-1.0, 3.0, 16))      # ... and these sixteen in the widest batched solve
COND_S_CAP = 1e7                        # cond S(p) over SHIFTS
COND_BLOCK_CAP = 1e8                    # block and Schur-block condition numbers of the cycle
NB, MW = 2, 3                           # columns of B and W in the iterations


# ------------------------------------------------------------------------------------------------ generator
def _sprand(rng, nrows, ncols, per_row, lo=-1.0, hi=1.0):
    """Sparse random matrix with ``min(per_row, ncols)`` entries in every row, uniform in [lo, hi)."""
    k = min(per_row, ncols)
    rows = np.repeat(np.arange(nrows), k)
    cols = np.concatenate([rng.choice(ncols, size=k, replace=False) for _ in range(nrows)]) if nrows else rows
    vals = rng.uniform(lo, hi, size=rows.size)
    return sps.csr_matrix((vals, (rows, cols)), shape=(nrows, ncols))


def synthetic(nv, np_, seed, lumped=False, e_outside=False, unsym=False, j_cols=None, dense_j_row=False,
              arrow=False, disjoint_j=False, grid=None, j_scale=10.0):
    """One synthetic operator as SciPy CSR ``(calA, calE, J)``.

    ``lumped``: calE is a positive diagonal.  ``e_outside``: G is drawn independently of R, so calE has entries
    outside calA's pattern (else G has R's pattern and calE stays inside R R^T).  ``unsym``: the skew pair
    ``Q - Q^T`` is replaced by one-sided entries of half the size (the pattern loses its symmetry; the symmetric
    part stays negative definite: at most 6 entries of 0.075 per row and column of ``I``'s share).  ``j_cols``:
    the constraints touch the first ``j_cols`` velocity unknowns only.  ``dense_j_row``: row 0 of J touches every
    velocity unknown.  ``arrow``: row and column 0 of calA are full (``[[2 + u.u, u^T], [u, I]]`` added to
    ``R R^T``; positive definite by its Schur complement).  ``disjoint_j``: row k of J lives on its own
    ``nv // np`` unknowns, so the graph of ``J J^T`` has no edge.  ``grid = (nx, ny)``: a stiffness-like calA
    (graph Laplacian of the grid in place of the random ``R R^T``, identity and skew part scaled by 0.2), which
    ``host_sa_criterion`` accepts: the one operator of the family with a smoothed prolongation."""
    rng = np.random.default_rng(seed)
    R = _sprand(rng, nv, nv, 3)
    Q = _sprand(rng, nv, nv, 3)
    eye = sps.identity(nv, format="csr")
    if unsym:
        skew = 0.5 * sps.triu(Q, 1) + 0.5 * sps.tril(_sprand(rng, nv, nv, 3), -1)
    else:
        skew = Q - Q.T
    if grid is not None:
        # stiffness-like: R is the edge-node incidence matrix of an nx x ny grid (R R^T its graph Laplacian), the
        # identity and the skew part are scaled down -- the operator the setup smooths its prolongation for
        nx, ny = grid
        assert nx * ny == nv
        node = np.arange(nv).reshape(nx, ny)
        ed = np.concatenate([np.stack([node[:-1].ravel(), node[1:].ravel()], 1),
                             np.stack([node[:, :-1].ravel(), node[:, 1:].ravel()], 1)])
        R = sps.csr_matrix((np.tile([1.0, -1.0], len(ed)), (ed.ravel(), np.repeat(np.arange(len(ed)), 2))),
                           shape=(nv, len(ed)))
        eye, skew = 0.2 * eye, 0.2 * skew
    core = R @ R.T + 0.3 * skew
    if arrow:
        u = np.zeros(nv)
        u[1:] = 0.1 * rng.uniform(0.5, 1.0, size=nv - 1) * rng.choice([-1.0, 1.0], size=nv - 1)
        head = sps.lil_matrix((nv, nv))
        head[0, :] = u
        head[:, 0] = u[:, None]
        head[0, 0] = 1.0 + u @ u
        core = core + head.tocsr()
    calA = (-(core + eye)).tocsr()
    dg = sps.diags(rng.uniform(0.5, 1.5, size=nv))
    if lumped:
        calE = dg.tocsr()
    else:
        if e_outside:
            G = _sprand(rng, nv, nv, 2)
        else:
            G = R.copy()
            G.data = rng.uniform(-1.0, 1.0, size=G.data.size)
        calE = (0.2 * (G @ G.T) + dg).tocsr()
    if np_ == 0:
        J = sps.csr_matrix((0, nv))
    elif disjoint_j:
        w = nv // np_
        rows = np.repeat(np.arange(np_), w)
        cols = np.arange(np_ * w)
        vals = rng.uniform(0.3, 0.8, size=cols.size) * rng.choice([-1.0, 1.0], size=cols.size)
        vals[::w] = rng.uniform(2.0, 3.0, size=np_)
        J = sps.csr_matrix((j_scale * vals, (rows, cols)), shape=(np_, nv))
    else:
        nc = nv if j_cols is None else j_cols
        weak = _sprand(rng, np_, nc, 2, -0.5, 0.5).tolil()
        for k in range(np_):
            weak[k, k] = rng.uniform(2.0, 3.0)
        if dense_j_row:
            weak[0, :] = rng.uniform(0.1, 0.4, size=nc) * rng.choice([-1.0, 1.0], size=nc)
            weak[0, 0] = 2.5
        J = j_scale * sps.csr_matrix(weak, shape=(np_, nc))
        if nc < nv:
            J = sps.hstack([J, sps.csr_matrix((np_, nv - nc))], format="csr")
    out = []
    for m in (calA, calE, J):
        m = sps.csr_matrix(m, dtype=np.float64)
        m.sum_duplicates()
        m.sort_indices()
        out.append(m)
    return tuple(out)


def finite_element(N):
    """``problems.ricc_problem(N, 0.05)`` in the orientation the solver receives it (as test_gpu_configs.py)."""
    pr = pb.ricc_problem(N, 0.05)
    return (-pr.A - pr.Nc).T.tocsr(), pr.M.T.tocsr(), pr.J.tocsr()


# name -> (builder, arguments, context options).  Tile edges: nv around the 16-row MFMA chunks, the 32-row SpMM
# blocks and the 16 / 32 / 64-row block-Jacobi blocks; np from {0, 1, nv - 1} and a value in between.
FAMILY = {
    "fe2": (finite_element, dict(N=2), {}),
    "fe3": (finite_element, dict(N=3), {}),
    "nv1": (synthetic, dict(nv=1, np_=0, seed=101), {}),
    "nv2_np0": (synthetic, dict(nv=2, np_=0, seed=102, lumped=True), {}),
    "nv2_np1": (synthetic, dict(nv=2, np_=1, seed=103), {}),
    "nv15_np0": (synthetic, dict(nv=15, np_=0, seed=104), {}),
    "nv16_np1": (synthetic, dict(nv=16, np_=1, seed=105), {}),
    "nv17_np16": (synthetic, dict(nv=17, np_=16, seed=106), {}),
    "nv31_np12": (synthetic, dict(nv=31, np_=12, seed=107), {}),
    "nv32_np31": (synthetic, dict(nv=32, np_=31, seed=108), {}),
    "nv33_np1": (synthetic, dict(nv=33, np_=1, seed=109), {}),
    "nv63_np0": (synthetic, dict(nv=63, np_=0, seed=110), {}),
    "nv65_np24": (synthetic, dict(nv=65, np_=24, seed=111), {}),
    "nv15_np14_b16": (synthetic, dict(nv=15, np_=14, seed=112), dict(bj_block=16)),
    "nv16_np7_b16": (synthetic, dict(nv=16, np_=7, seed=113), dict(bj_block=16)),
    "nv17_np1_b16": (synthetic, dict(nv=17, np_=1, seed=114), dict(bj_block=16)),
    "nv63_np62_b64": (synthetic, dict(nv=63, np_=62, seed=315), dict(bj_block=64)),
    "nv65_np20_b64": (synthetic, dict(nv=65, np_=20, seed=116), dict(bj_block=64)),
    "lumped": (synthetic, dict(nv=48, np_=15, seed=120, lumped=True), {}),
    "e_outside": (synthetic, dict(nv=44, np_=12, seed=121, e_outside=True), {}),
    "unsym": (synthetic, dict(nv=52, np_=17, seed=122, unsym=True), {}),
    "free_rows": (synthetic, dict(nv=56, np_=10, seed=123, j_cols=24), {}),
    "dense_j_row": (synthetic, dict(nv=41, np_=9, seed=124, dense_j_row=True), {}),
    "stiff_grid": (synthetic, dict(nv=54, np_=14, seed=128, grid=(9, 6)), {}),
    "arrow200": (synthetic, dict(nv=200, np_=40, seed=125, arrow=True), {}),
    "disjoint_5_2": (synthetic, dict(nv=5, np_=2, seed=126, disjoint_j=True, lumped=True), {}),
    "disjoint_12_4": (synthetic, dict(nv=12, np_=4, seed=127, disjoint_j=True, lumped=True), {}),
}
NAMES = list(FAMILY)


# ------------------------------------------------------------------------------------------------ references
class SmallOp:
    """One operator of the family with its dense copies and references (computed on first use)."""

    def __init__(self, name):
        fn, kw, opts = FAMILY[name]
        self.name, self.opts = name, dict(opts)
        self.calA, self.calE, self.J = fn(**kw)
        self.nv, self.np = self.calA.shape[0], self.J.shape[0]
        self.n = self.nv + self.np
        self.Ad, self.Ed, self.Jd = self.calA.toarray(), self.calE.toarray(), self.J.toarray()
        self._c = {}

    @property
    def ops(self):
        return self.calA, self.calE, self.J

    def _memo(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    # -- the saddle matrix
    def S(self, alpha, beta=1.0):
        """Dense ``[[beta calA + alpha calE, J^T], [J, 0]]``."""
        return self._memo(("S", alpha, beta), lambda: sm.saddle(self.calA, self.calE, self.J, alpha, beta).toarray())

    def lu(self, alpha, beta=1.0):
        return self._memo(("lu", alpha, beta), lambda: sla.lu_factor(self.S(alpha, beta)))

    def solve(self, alpha, beta, rhs):
        """``S(alpha, beta)^-1 rhs`` by the dense LU, one step of iterative refinement in FP64."""
        S, lu = self.S(alpha, beta), self.lu(alpha, beta)
        x = sla.lu_solve(lu, rhs)
        return x + sla.lu_solve(lu, rhs - S @ x)

    def cond_S(self, alpha, beta=1.0):
        return self._memo(("cond", alpha, beta), lambda: float(np.linalg.cond(self.S(alpha, beta))))

    # -- the divergence-free space
    @property
    def theta(self):
        """Orthonormal basis of ker J (nv x (nv - rank J))."""
        return self._memo("theta", lambda: sla.null_space(self.Jd) if self.np else np.eye(self.nv))

    @property
    def j_rank(self):
        return self._memo("rank", lambda: int(np.linalg.matrix_rank(self.Jd)) if self.np else 0)

    @property
    def leray(self):
        """``identities.leray_projector`` of ``(calE^T, J)``: P^T W is what the drivers make of W."""
        if self.np == 0:
            return np.eye(self.nv)
        return self._memo("leray", lambda: identities.leray_projector(sps.csr_matrix(self.calE.T), self.J))

    @property
    def pencil_eigs(self):
        """Generalised eigenvalues of the pencil projected onto ker J."""
        def f():
            Th = self.theta
            return sla.eigvals(Th.T @ self.Ad @ Th, Th.T @ self.Ed @ Th)
        return self._memo("eigs", f)

    @property
    def shifts(self):
        """Eight log-spaced ADI shifts over the moduli of the projected spectrum, a factor two beyond either end
        (distinct also where ker J has one dimension: the sweep form needs a regular Cauchy matrix)."""
        lam = np.abs(self.pencil_eigs)
        return pb.logshifts(0.5 * lam.min(), 2.0 * lam.max(), 8)

    # -- right-hand sides of the iterations
    @property
    def B(self):
        return self._memo("B", lambda: np.random.default_rng(7).standard_normal((self.nv, NB)))

    @property
    def W(self):
        return self._memo("W", lambda: np.random.default_rng(8).standard_normal((self.nv, MW)))

    @property
    def Z0(self):
        """A small initial iterate in ker J (two columns)."""
        return self._memo("Z0", lambda: 0.1 * self.theta @ (self.theta.T @
                                                            np.random.default_rng(9).standard_normal((self.nv, 2))))

    @property
    def oldB(self):
        """A gain-like ``nv x NB`` matrix, ``-calE Y Y^T B`` for a small random Y in ker J (as
        ``identities.dre_step_inputs`` builds one)."""
        def f():
            Y = 0.3 * self.theta @ (self.theta.T @ np.random.default_rng(10).standard_normal((self.nv, 3)))
            return -(self.Ed @ (Y @ (Y.T @ self.B)))
        return self._memo("oldB", f)

    # -- dense solutions
    def lyap(self, W=None):
        """X = Theta Xh Theta^T with ``calA X calE^T + calE X calA^T + W W^T = 0`` on ker J, by
        ``scipy.linalg.solve_continuous_lyapunov`` (Bartels-Stewart) on the projected pencil."""
        def f():
            Th = self.theta
            Ah, Eh = Th.T @ self.Ad @ Th, Th.T @ self.Ed @ Th
            Wh = np.linalg.solve(Eh, Th.T @ (self.W if W is None else W))
            a = np.linalg.solve(Eh, Ah)
            Xh = sla.solve_continuous_lyapunov(a, -(Wh @ Wh.T))
            Xh = 0.5 * (Xh + Xh.T)
            res = a @ Xh + Xh @ a.T + Wh @ Wh.T
            assert np.linalg.norm(res) <= 1e-12 * max(np.linalg.norm(Wh @ Wh.T), np.linalg.norm(a @ Xh))
            return Th @ Xh @ Th.T
        return f() if W is not None else self._memo("lyap", f)

    def are(self, old=False):
        """``identities.dense_projected_are`` of the operator (``old``: of ``calA + oldB B^T``)."""
        def f():
            Ad = self.Ad + self.oldB @ self.B.T if old else self.Ad
            return identities.dense_projected_are(Ad, self.Ed, self.Jd, self.B, self.W)
        return self._memo(("are", old), f)

    # -- the structure the host setup gives the cycle (no device needed)
    def host_structure(self):
        """The block partition of the one-level cycle as the setup forms it: velocity blocks by
        ``host_aggregate`` on the union pattern of calA and calE, pressure blocks on the pattern of ``J J^T``,
        both at the block size of the operator's options -- as a ``precond_model`` structure without a coarse
        space."""
        def f():
            bs = self.opts.get("bj_block", 32)
            vb, _ = _lib.host_aggregate((sm._pattern(self.calA) + sm._pattern(self.calE)).tocsr(), bs)
            if self.np:
                pb_, _ = _lib.host_aggregate(sm._pattern(sm._pattern(self.J) @ sm._pattern(self.J).T), bs)
            else:
                pb_ = np.zeros(0, np.int32)
            return pm.plain_structure(self.calA, self.calE, self.J, vb, pb_, bs=bs)
        return self._memo("hst", f)

    def block_conditioning(self, alpha, beta=1.0):
        """Largest block and Schur-block condition number of the cycle at ``(alpha, beta)`` on the host
        structure."""
        def f():
            op = pm.CycleModel(self.calA, self.calE, self.J, self.host_structure()).operands(alpha, beta)
            return float(max(op["cond_blocks"], op.get("cond_schur", 1.0)))
        return self._memo(("bcond", alpha, beta), f)


_OPS = {}


def get(name):
    if name not in _OPS:
        _OPS[name] = SmallOp(name)
    return _OPS[name]


# ------------------------------------------------------------------------------------------------ comparators
def rel(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300))


RES_TOL = 1e-10       # true relative residual of a shift solve, per column (the bar of test_gpu_parity.py)


def solve_errors(op, alpha, beta, X, R):
    """Per column of a shift solve ``S(alpha, beta) X = [R; 0]``: (true relative residual recomputed in FP64,
    relative forward error against the dense LU)."""
    S = op.S(alpha, beta)
    rhs = np.vstack([R, np.zeros((op.np, R.shape[1]))])
    bn = np.linalg.norm(rhs, axis=0)
    res = np.linalg.norm(S @ X - rhs, axis=0) / np.where(bn > 0, bn, 1.0)
    Xref = op.solve(alpha, beta, rhs)
    xn = np.linalg.norm(Xref, axis=0)
    fwd = np.linalg.norm(X - Xref, axis=0) / np.where(xn > 0, xn, 1.0)
    return res, fwd


def solve_ok(op, alpha, beta, X, R):
    """The assertions every shift solve is held to; returns (worst residual, worst forward error)."""
    assert np.all(np.isfinite(X)), (op.name, alpha, "not finite")
    res, fwd = solve_errors(op, alpha, beta, X, R)
    zero = np.linalg.norm(R, axis=0) == 0
    assert np.all(X[:, zero] == 0.0), (op.name, alpha, "a zero right-hand side gave a non-zero solution")
    assert res.max() <= RES_TOL, (op.name, alpha, "residual", res.max())
    bound = 2.0 * op.cond_S(alpha, beta) * RES_TOL
    assert fwd.max() <= bound, (op.name, alpha, "forward error", fwd.max(), bound)
    return float(res.max()), float(fwd.max())


def smoothing_omega(calA):
    """The damping the setup's rule gives the prolongation smoother ``I - omega D^-1 sym(calA)``: 0.5, scaled by
    ``2 / rho`` where ``rho = rho(D^-1 sym(calA))`` exceeds 2 -- rho from 20 steps of the power iteration, started
    from the values of the linear congruential generator ``s <- 1664525 s + 1013904223 (mod 2^32)``, s0 = 12345,
    mapped to ``(s >> 8) / 2^24 - 0.5`` (``smoothed_prolongation`` in ricadi_host.cpp; ``verbose`` prints rho and
    omega)."""
    A = sps.csr_matrix(calA)
    nv = A.shape[0]
    d = A.diagonal()
    K0 = (0.5 * (A + A.T)).tocsr()
    s, x = 12345, np.zeros(nv)
    for i in range(nv):
        s = (s * 1664525 + 1013904223) % 2 ** 32
        x[i] = (s >> 8) / 16777216.0 - 0.5
    rho = 0.0
    for _ in range(20):
        y = np.where(d != 0.0, (K0 @ x) / np.where(d != 0.0, d, 1.0), 0.0)
        nx, ny = np.linalg.norm(x), np.linalg.norm(y)
        rho = ny / nx if nx > 0 else 0.0
        x = y / ny if ny > 0 else 0.0 * y
    return 0.5 * (2.0 / rho if rho > 2.0 else 1.0)


def smoothed_prolongation(calA, st):
    """``(I - omega D^-1 sym(calA)) Y`` on the velocity rows and Y on the pressure rows, dense, for the aggregates
    of the structure ``st`` (rows with a zero diagonal keep their row of Y)."""
    A = sps.csr_matrix(calA)
    nv, n, kc = st["nv"], st["nv"] + st["np"], st["kc"]
    Y = np.zeros((n, kc))
    Y[np.arange(n), np.asarray(st["aggof"])] = 1.0
    d = A.diagonal()
    w = np.where(d != 0.0, smoothing_omega(A) / np.where(d != 0.0, d, 1.0), 0.0)
    P = Y.copy()
    P[:nv] -= w[:, None] * ((0.5 * (A + A.T)) @ Y[:nv])
    return P


def structure_problems(st):
    """What is wrong with a ``Context.precond_structure`` dict (empty list: nothing)."""
    bad = []
    nv, np_, bs = st["nv"], st["np"], st["bs"]
    for rows, ptr, cnt, what in ((st["bv_rows"], st["bv_ptr"], nv, "velocity"), (st["bp_rows"], st["bp_ptr"], np_,
                                                                               "pressure")):
        if sorted(np.asarray(rows).tolist()) != list(range(cnt)):
            bad.append("%s block rows are no permutation" % what)
        sizes = np.diff(np.asarray(ptr))
        if cnt and (ptr[0] != 0 or ptr[-1] != cnt or sizes.min() < 1):
            bad.append("%s block pointers do not cover the rows" % what)
        if sizes.size and sizes.max() > bs:
            bad.append("a %s block holds %d > %d rows" % (what, sizes.max(), bs))
    kc, kcv, kcp = st["kc"], st["kcv"], st["kcp"]
    if kc != kcv + kcp:
        bad.append("kc != kcv + kcp")
    if np_ > 0 and kcp > kcv:
        bad.append("kcp = %d > kcv = %d" % (kcp, kcv))
    if kc > 0:
        agg = np.asarray(st["aggof"])
        if agg.size != nv + np_:
            bad.append("aggof has the wrong length")
        else:
            if agg[:nv].min() < 0 or agg[:nv].max() >= kcv:
                bad.append("a velocity row lies outside [0, kcv)")
            if np_ and (agg[nv:].min() < kcv or agg[nv:].max() >= kc):
                bad.append("a pressure row lies outside [kcv, kc)")
            if np.bincount(np.clip(agg, 0, kc - 1), minlength=kc).min() < 1:
                bad.append("an aggregate is empty")
    return bad
