"""Dense FP64 model of the low-rank Lyapunov ADI with complex-conjugate shift pairs (DESIGN.md section 3g;
optconpy_amd/csrc/solver_adi_pairs.inl, the pair kernels of ricadi_cplx.hip).

The equation is ``A X E^T + E X A^T + W W^T = 0`` on ker J with ``A = calA - U V^T``.  A list entry is a negative real
shift (one step) or ONE complex number ``p = a + ib``, ``a < 0``, ``b != 0``, that stands for the pair ``(p, conj p)``:
the real-arithmetic pair step of Benner, Kuerschner and Saak (2013),

    S(p) [V; *] = [W; 0],   delta = a / b,   gam = 2 sqrt(-a),   V1 = Re V + delta Im V,
    Z <- [Z, gam V1, gam sqrt(delta^2 + 1) Im V],   W <- W - 4 a E V1,

two steps from one complex solve.  Every solve here is a dense solve with the saddle matrix
``S(p) = [[A + p E, J^T], [J, 0]]`` (``numpy.linalg.solve`` plus one step of refinement); the Woodbury form solves with
``calA`` and corrects, ``X = X_W + X_U (I - V^T X_U)^-1 V^T X_W``, as the driver does.  The stopping bookkeeping is the
driver's (adi_stop.h): a pair records its two blocks in order, both with the residual behind the pair, the rules are
read after the second block, and a pair is never split by ``max_steps``.  Nothing is shared with the library.

``blocks_twin`` is the float64 twin of ``adi_pair_blocks_kernel``: the same operations in the same order on the
packed solution groups, except that the kernel fuses ``Re x + delta Im x`` into one rounding.
"""
import numpy as np
import scipy.linalg as sla

EPS = np.finfo(np.float64).eps
MAX_MC = 8


def groups(width):
    """(ng, mc) of ``width`` real columns: ``ceil(width / 8)`` groups of ``ceil(width / ng)`` complex columns."""
    ng = -(-int(width) // MAX_MC)
    return ng, -(-int(width) // ng)


def pair_coefs(p):
    """(delta, gam, gam2) of the pair at ``p``, in the driver's order of operations."""
    a, b = float(np.real(p)), float(np.imag(p))
    delta = a / b
    gam = 2.0 * np.sqrt(-a)
    d2 = delta * delta
    return delta, gam, gam * np.sqrt(d2 + 1.0)


# ------------------------------------------------------------------------------------------------ the blocks kernel
def pack(Wm, U=None):
    """[W, U] (nv x m') as ``ng`` groups of ``mc`` complex columns (ng, nv, mc): zero imaginary parts, zero padding."""
    P = Wm if U is None else np.hstack([Wm, U])
    nv, mp = P.shape
    ng, mc = groups(mp)
    R = np.zeros((ng, nv, mc), dtype=complex)
    for j in range(mp):
        R[j // mc, :, j % mc] = P[:, j]
    return R


def unpack(X, m):
    """Columns 0 .. m of the step's panel from the groups X (ng, rows, mc)."""
    mc = X.shape[2]
    return np.stack([X[j // mc, :, j % mc] for j in range(m)], axis=1)


def blocks_twin(X, nv, m, p, fault=None):
    """Twin of the blocks kernel on the solution groups ``X`` (ng, n, mc) complex: returns
    ``(Z1, Z2, V1, norms2)`` -- the two scaled blocks and the unscaled ``V1`` (nv x m each) and the squared Frobenius
    norms of the two blocks.  ``fault`` injects one of the mistakes the tests must be able to see:
    ``'delta_sign'``, ``'no_sqrt'``, ``'last_row'`` (the last velocity row is not written: it stays NaN)."""
    delta, gam, gam2 = pair_coefs(p)
    if fault == "delta_sign":
        delta = -delta
    if fault == "no_sqrt":
        gam2 = gam
    x = unpack(X[:, :nv], m)
    re, im = np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag)
    V1 = re + delta * im
    Z1 = gam * V1
    Z2 = gam2 * im
    if fault == "last_row":
        V1[-1], Z1[-1], Z2[-1] = np.nan, np.nan, np.nan
    return Z1, Z2, V1, np.array([np.sum(Z1 * Z1), np.sum(Z2 * Z2)])


def blocks_bound(X, nv, m, p):
    """Entrywise bound of the scaled blocks against the twin, ``4 eps gam (|Re x| + |delta Im x|)``: the kernel's
    ``fma(delta, Im x, Re x)`` and the twin's two roundings differ by at most ``eps |delta Im x|``, the scaling adds
    ``eps`` relative, and the second block is formed by the same single product in both.  Without ``gam`` it bounds
    ``V1``."""
    delta, gam, _ = pair_coefs(p)
    x = unpack(X[:, :nv], m)
    b1 = 4.0 * EPS * (np.abs(x.real) + np.abs(delta * x.imag))
    return gam * b1, b1


# ------------------------------------------------------------------------------------------------ the Woodbury solve
# (m, q) of the pair-solve tests: no low-rank term with one, two and three groups and zero padding at (9, 0); one
# group; U straddling groups 0 and 1 with one padding column (mc = 6); U exactly group 1; U filling two groups and
# more; three groups of 8 with U behind W's last column in the last one; ng = 16, mc = 8, the widest batch
PAIR_SOLVE_SHAPES = ((1, 0), (8, 0), (9, 0), (24, 0), (1, 1), (3, 2), (5, 6), (8, 8), (2, 16), (17, 7), (120, 8))
WOODBURY_FAULTS = ("embed_sign", "group_of_m", "cap_shift", "straddle", "no_pressure")


def _abs2(z):
    """|Re z| + |Im z|: bounds the modulus and is what a real kernel on the real view sees."""
    return np.abs(np.real(z)) + np.abs(np.imag(z))


def _maps(m, q, fault=None):
    """Step column j -> (group, complex column), for the m + q columns.  ``group_of_m``: the map of ``groups(m)``
    wherever that place exists in the groups of ``m + q`` (elsewhere the right one)."""
    ng, mc = groups(m + q)
    right = [(j // mc, j % mc) for j in range(m + q)]
    if fault != "group_of_m":
        return right
    mcm = groups(m)[1]
    wrong = [(j // mcm, j % mcm) for j in range(m + q)]
    return [w if w[0] < ng and w[1] < mc else r for w, r in zip(wrong, right)]


def fault_applies(fault, m, q, n=None, nv=None):
    """Whether ``fault`` changes anything at this shape: every one needs ``q > 0``; ``group_of_m`` a column whose
    place differs, ``straddle`` columns of U in more than one group, ``no_pressure`` pressure rows."""
    if q == 0:
        return False
    ng, mc = groups(m + q)
    if fault == "group_of_m":
        return _maps(m, q, fault) != _maps(m, q)
    if fault == "straddle":
        return m // mc != (m + q - 1) // mc
    if fault == "no_pressure":
        return n is None or n > nv
    return True


def _smw_parts(Xraw, V, m, q, fault=None):
    """(t_W (q x m), cap (q x q), X_U (n x q)) of the first solve's groups."""
    nv = V.shape[0]
    at = _maps(m, q, fault)
    T = np.einsum("vk,gvc->gkc", V, Xraw[:, :nv])                   # V^T X per group, over the velocity rows
    tW = np.stack([T[g, :, cc] for g, cc in at[:m]], axis=1)
    u0 = m - 1 if fault == "cap_shift" else m
    right = _maps(m, q)
    src = at if fault != "cap_shift" else right
    tU = np.stack([T[src[u0 + l][0], :, src[u0 + l][1]] for l in range(q)], axis=1)
    XU = np.stack([Xraw[g, :, cc] for g, cc in at[m:m + q]], axis=1)
    if fault == "straddle":
        first = right[m][0]
        for l in range(q):
            if right[m + l][0] != first:
                XU[:, l] = 0.0
    return tW, np.eye(q) - tU, XU


def _correct(D, tW, cap, XU, m, q, nv, fault=None, solve=np.linalg.solve):
    y = solve(cap, tW)
    if fault == "embed_sign":
        corr = (XU.real @ y.real + XU.imag @ y.imag) + 1j * (XU.real @ y.imag + XU.imag @ y.real)
    else:
        corr = XU @ y
    if fault == "no_pressure":
        corr[nv:] = 0.0
    X = D.copy()
    for j, (g, cc) in enumerate(_maps(m, q, fault)[:m]):
        X[g, :, cc] += corr[:, j]
    return X, y


def woodbury_twin(Xraw, V, m, q, fault=None, Draw=None, solve=np.linalg.solve):
    """Float64 twin of ``PairSolve::capacitance()`` + ``woodbury()`` on the packed groups ``Xraw`` (ng, n, mc) complex
    of ``S(p)^-1 [W, U]``: with ``t = V^T X`` over the velocity rows, ``cap = I - t_U`` and ``y = cap^-1 t_W``,
    ``X_W <- X_W + X_U y`` over all n rows through the same group map; U's columns and the padding stay as they are.
    With ``Draw`` (the refinement's uncorrected groups, U's columns zero) the two-pass twin: ``X + (D_W + X_U cap^-1
    V^T D_W)`` with the first pass's ``cap`` and ``X_U``.  ``fault`` seeds one of ``WOODBURY_FAULTS`` or, on the
    two-pass twin, ``'refine_raw'`` (``D`` added uncorrected)."""
    if q == 0:
        return Xraw.copy()
    nv = V.shape[0]
    first = None if fault == "refine_raw" else fault
    tW, cap, XU = _smw_parts(Xraw, V, m, q, first)
    X, _ = _correct(Xraw, tW, cap, XU, m, q, nv, first, solve)
    if Draw is None:
        return X
    if fault == "refine_raw":
        return X + Draw
    tD, _, _ = _smw_parts(Draw, V, m, q, first)
    Dc, _ = _correct(Draw, tD, cap, XU, m, q, nv, first, solve)
    return X + Dc


def woodbury_bound(Xraw, V, m, q, Draw=None):
    """Entrywise bound (ng, n, mc) of a second evaluation of ``woodbury_twin`` against the first, both in float64 with
    any order of summation, counted from roundings (first order; ``u = eps``):

    * ``t = V^T X`` sums nv products per entry.  However the sum is ordered (the device adds slices with atomics), an
      evaluation is within ``(nv + 2) u |V|^T (|Re X| + |Im X|)`` of the exact product, two evaluations within twice
      that: ``dt``.
    * ``cap = I - t_U`` adds one rounding: ``dcap = dt_U + u |cap|``.  ``y = cap^-1 t_W`` then moves, column by column,
      by ``||cap^-1||_2 (||dt_W[:, j]||_2 + ||dcap||_F ||y_j||_2)``, and each of the two LU solves adds at most
      ``8 q u cond_2(cap) ||y_j||_2`` (the bar tests/test_pair_smw_cpu.py holds ``pair_lu`` to): ``dy_j``.
    * ``X_U y`` is a real product of inner length 2q: ``(2q + 2) u |X_U||y|`` per evaluation, plus
      ``||X_U[i, :]||_2 dy_j`` from the coefficients.
    * the final add rounds once per evaluation: ``u (|X_W| + |X_U||y|)``.

    A factor 1.25 covers the second-order terms, asserted small (``||cap^-1|| ||dcap|| <= 0.1``).  With ``Draw`` the
    same for the second pass (``cap`` and ``X_U`` are the first pass's, so ``dcap`` is charged again) plus the rounding
    of the sum of the two passes.  Entries of U's columns and of the padding are 0: they must not change."""
    ng, n, mc = Xraw.shape
    B = np.zeros((ng, n, mc))
    if q == 0:
        return B
    nv = V.shape[0]
    u = EPS
    at = _maps(m, q)
    tW, cap, XU = _smw_parts(Xraw, V, m, q)
    dT = 2.0 * (nv + 2) * u * np.einsum("vk,gvc->gkc", np.abs(V), _abs2(Xraw[:, :nv]))
    dtU = np.stack([dT[g, :, cc] for g, cc in at[m:m + q]], axis=1)
    dcap = np.linalg.norm(dtU) + u * np.linalg.norm(cap)
    inv = np.linalg.norm(np.linalg.inv(cap), 2)
    cond = np.linalg.cond(cap)
    assert inv * dcap <= 0.1, "the capacitance matrix is too ill-conditioned for a first-order bound"
    xu_row = np.linalg.norm(XU, axis=1)

    def one(D, tD):
        y = np.linalg.solve(cap, tD)
        dTD = 2.0 * (nv + 2) * u * np.einsum("vk,gvc->gkc", np.abs(V), _abs2(D[:, :nv]))
        dtW = np.stack([dTD[g, :, cc] for g, cc in at[:m]], axis=1)
        yn = np.linalg.norm(y, axis=0)
        dy = inv * (np.linalg.norm(dtW, axis=0) + dcap * yn) + 2.0 * 8.0 * q * u * cond * yn
        prod = _abs2(XU) @ _abs2(y)
        out = np.zeros((ng, n, mc))
        for j, (g, cc) in enumerate(at[:m]):
            out[g, :, cc] = 1.25 * (xu_row * dy[j] + 2.0 * (2 * q + 2) * u * prod[:, j]
                                    + 2.0 * u * (_abs2(D[g, :, cc]) + prod[:, j]))
        return out

    B = one(Xraw, tW)
    if Draw is not None:
        tD, _, _ = _smw_parts(Draw, V, m, q)
        B = B + one(Draw, tD) + 2.0 * u * _abs2(woodbury_twin(Xraw, V, m, q, Draw=Draw))
        for g, cc in at[m:]:
            B[g, :, cc] = 0.0
    return B


def amplification(model, p, W):
    """Per column j of W: ``||U||_F ||y_j|| / ||w_j||`` with ``y = cap^-1 V^T X_W`` at the shift ``p``.  The corrected
    residual is ``R_W + R_U y``, so this ratio multiplies the residuals of the solves with U's columns (relative to
    ``||U||_F``) in the residual of column j (relative to ``||w_j||``)."""
    m = W.shape[1]
    X = model._solve(model.saddle(model.A0, p), np.hstack([W, model.U]))[:model.nv]
    cap = np.eye(model.U.shape[1]) - model.V.T @ X[:, m:]
    y = np.linalg.solve(cap, model.V.T @ X[:, :m])
    wn = np.linalg.norm(W, axis=0)
    return np.linalg.norm(model.U) * np.linalg.norm(y, axis=0) / np.where(wn > 0, wn, 1.0)


def refinement_ladder(op, a, eta, deltas, q, seed):
    """Low-rank terms that bring the capacitance matrix of the pair solve close to singular, the construction of
    ``test_gpu_solve_branches.test_woodbury_refinement`` carried to the complex shift ``p = a (1 - i eta)``: with
    ``U, V = 0.1 standard_normal`` (nv x q), ``U2 = U inv(Re(V^T S(p)^-1 U)) (1 - delta)``, so that
    ``cap = I - V^T S(p)^-1 U2 = delta I - i Im(..) inv(Re(..)) (1 - delta)``.  Returns ``(p, [(delta, U2, V)])``;
    ``op`` is a ``small_ops.SmallOp``."""
    p = complex(a, -a * eta)
    mdl = PairsModel(*op.ops)
    rng = np.random.default_rng(seed)
    U = 0.1 * rng.standard_normal((op.nv, q))
    V = 0.1 * rng.standard_normal((op.nv, q))
    G = V.T @ mdl._solve(mdl.saddle(mdl.A0, p), U)[:op.nv]
    Ginv = np.linalg.inv(G.real)
    return p, [(float(d), U @ Ginv * (1.0 - d), V) for d in deltas]


# ------------------------------------------------------------------------------------------------ the iteration
class PairsModel:
    """The operator ``(calA - U V^T, calE, J)`` in dense form with the solves and references of the iteration."""

    def __init__(self, calA, calE, J, U=None, V=None):
        dn = lambda a: a.toarray() if hasattr(a, "toarray") else np.asarray(a, dtype=float)
        self.A0, self.E, self.J = dn(calA), dn(calE), dn(J)
        self.nv, self.np = self.A0.shape[0], self.J.shape[0]
        self.U = None if U is None else np.asarray(U, dtype=float)
        self.V = None if V is None else np.asarray(V, dtype=float)
        self.A = self.A0 if U is None else self.A0 - self.U @ self.V.T
        self.Th = sla.null_space(self.J) if self.np else np.eye(self.nv)

    def saddle(self, A, alpha, beta=1.0):
        n = self.nv + self.np
        S = np.zeros((n, n), dtype=complex if np.iscomplexobj(alpha) else float)
        S[:self.nv, :self.nv] = beta * A + alpha * self.E
        S[:self.nv, self.nv:] = self.J.T
        S[self.nv:, :self.nv] = self.J
        return S

    def _solve(self, S, R):
        rhs = np.zeros((S.shape[0], R.shape[1]), dtype=np.result_type(S, R))
        rhs[:self.nv] = R
        lu = sla.lu_factor(S)
        x = sla.lu_solve(lu, rhs)
        return x + sla.lu_solve(lu, rhs - S @ x)

    def project(self, W):
        """``P^T W`` as the drivers form it: one saddle solve with calE, then calE times the velocity part."""
        if self.np == 0:
            return np.array(W, dtype=float)
        return self.E @ self._solve(self.saddle(self.A0, 1.0, 0.0), W)[:self.nv]

    def solve(self, p, W, woodbury=False):
        """Velocity rows of ``(S(p) - [U; 0][V; 0]^T)^-1 [W; 0]``; ``woodbury``: through solves with ``calA`` and the
        capacitance matrix, as the driver; else one dense solve with the closed-loop matrix."""
        if self.U is None or not woodbury:
            return self._solve(self.saddle(self.A, p), W)[:self.nv]
        m = W.shape[1]
        X = self._solve(self.saddle(self.A0, p), np.hstack([W, self.U]))[:self.nv]
        XW, XU = X[:, :m], X[:, m:]
        cap = np.eye(self.U.shape[1]) - self.V.T @ XU
        return XW + XU @ np.linalg.solve(cap, self.V.T @ XW)

    def lyap(self, W):
        """Dense ``X = Theta Xh Theta^T`` of the projected equation with right-hand side factor ``W`` (Bartels-Stewart
        on the projected pencil, as ``small_ops.SmallOp.lyap``)."""
        Th = self.Th
        Ah, Eh = Th.T @ self.A @ Th, Th.T @ self.E @ Th
        Wh = np.linalg.solve(Eh, Th.T @ W)
        a = np.linalg.solve(Eh, Ah)
        Xh = sla.solve_continuous_lyapunov(a, -(Wh @ Wh.T))
        Xh = 0.5 * (Xh + Xh.T)
        res = a @ Xh + Xh @ a.T + Wh @ Wh.T
        assert np.linalg.norm(res) <= 1e-12 * max(np.linalg.norm(Wh @ Wh.T), np.linalg.norm(a @ Xh))
        return Th @ Xh @ Th.T

    def pencil_eigs(self):
        Th = self.Th
        return sla.eigvals(Th.T @ self.A @ Th, Th.T @ self.E @ Th)

    def projected_residual(self, Z, W0):
        """``Theta^T (A X E^T + E X A^T + W0 W0^T) Theta`` with ``X = Z Z^T``."""
        Th = self.Th
        L = (Th.T @ self.A @ Z) @ (Z.T @ self.E.T @ Th)
        Wh = Th.T @ W0
        return L + L.T + Wh @ Wh.T

    def run(self, entries, W, max_steps=300, newZ_reltol=0.0, res_reltol=0.0, project=True, woodbury=False):
        """The iteration over ``entries`` (floats and complex numbers, cycled) with the driver's stopping
        bookkeeping.  Returns dict: ``Z`` (nv x steps m), ``W0`` (the right-hand side after the projection), ``W`` (the
        final residual factor), ``steps``, ``pairs`` (pair entries visited), ``solves``, ``rel_newZ`` and ``hist`` (one
        entry per step; both entries of a pair hold the value behind the pair for ``hist``), ``rule``
        (``'newZ'``, ``'res'`` or ``'max_steps'``), ``last_is_pair`` (the last entry visited was a pair), ``amplification`` (with a low-rank term: per pair entry visited the
        largest ``amplification`` among the columns of the residual factor it solved for)."""
        Wj = self.project(W) if project else np.array(W, dtype=float)
        W0 = Wj.copy()
        rhs = float(np.linalg.norm(W0.T @ W0))
        blocks, rels, hist, amps = [], [], [], []
        z2, steps, pairs, solves, rule, e = 0.0, 0, 0, 0, "max_steps", 0
        last_is_pair = False

        def record(blk):
            nonlocal z2
            b2 = float(np.sum(blk * blk))
            z2 += b2
            blocks.append(blk)
            rels.append(np.sqrt(b2 / z2) if z2 > 0 else 0.0)
            return rels[-1] < newZ_reltol

        while steps < max_steps:
            p = entries[e % len(entries)]
            e += 1
            if isinstance(p, complex) and p.imag != 0.0:
                if steps + 2 > max_steps:
                    break
                delta, gam, gam2 = pair_coefs(p)
                if self.U is not None:
                    amps.append(float(np.max(amplification(self, p, Wj))))
                X = self.solve(p, Wj, woodbury)
                V1 = X.real + delta * X.imag
                Wj = Wj - 4.0 * p.real * (self.E @ V1)
                fired = record(gam * V1)
                fired = record(gam2 * X.imag) or fired
                h = float(np.linalg.norm(Wj.T @ Wj)) / rhs if rhs > 0 else 0.0
                hist += [h, h]
                steps += 2
                pairs += 1
                last_is_pair = True
            else:
                p = float(np.real(p))
                X = np.real(self.solve(p, Wj, woodbury))
                Wj = Wj - 2.0 * p * (self.E @ X)
                fired = record(np.sqrt(-2.0 * p) * X)
                h = float(np.linalg.norm(Wj.T @ Wj)) / rhs if rhs > 0 else 0.0
                hist.append(h)
                steps += 1
                last_is_pair = False
            solves += 1
            if fired:
                rule = "newZ"
                break
            if res_reltol > 0.0 and h <= res_reltol:
                rule = "res"
                break
        Z = np.hstack(blocks) if blocks else np.zeros((self.nv, 0))
        return dict(Z=Z, W0=W0, W=Wj, steps=steps, pairs=pairs, solves=solves, rel_newZ=np.array(rels),
                    hist=np.array(hist), rule=rule, last_is_pair=last_is_pair,
                    amplification=np.array(amps))


def pair_shifts(model, real_shifts):
    """The tests' shift recipe: of the projected-pencil eigenvalues of the operator as solved, the up to three with
    ``Im > 1e-6 |lambda|`` and the largest ``|Im / Re|`` (one entry per pair), then ``real_shifts[::3]``."""
    lam = model.pencil_eigs()
    lam = lam[np.isfinite(lam)]
    up = lam[(lam.imag > 1e-6 * np.abs(lam)) & (lam.real < 0)]
    up = up[np.argsort(-np.abs(up.imag / up.real), kind="stable")][:3]
    return [complex(z) for z in up] + [float(p) for p in list(real_shifts)[::3]]
