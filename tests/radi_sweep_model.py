"""Model of the SWEEP form of the low-rank RADI iteration (csrc/solver_radi.inl, ricadi_radi.hip):
G consecutive steps with pairwise distinct shifts p_1 .. p_G < 0 as G independent solves against the SAME panel, and a
small dense recombination.  Conventions are those of tests/radi_model.py.

At the start of a sweep the state is R_0 (nv x m), U_0 (nv x nb), cal A_0 = cal A - U_0 B^T:

    [[cal A_0 + p_g cal E, J^T], [J, 0]] [Vh_g; *] = [R_0; 0]                g = 1 .. G,   Vh = [Vh_1 .. Vh_G]
    S = cal E Vh,   Gh = Vh^T B (G m x nb),   Gamma = P^T P,  P = [R_0 | S]
    M_gh = -(I_m + Gh_g Gh_h^T) / (p_g + p_h)  =  L L^T                      (blocks in shift order)
    y = L^-1 (1_G (x) I_m),   h = L^-1 Gh,   T_j = L^-T[:, :j m]
    Z block = Vh T_k,   R_j = R_0 + S T_j y[:j m],   U_j = U_0 + S T_j h[:j m]
    ||R_j^T R_j||_F = ||c_j^T Gamma c_j||_F,   c_j = [I_m; T_j y[:j m]]

The first j m columns of Vh L^-T are the contribution of the first j sequential steps up to a rotation inside each
block (RADI = the Riccati subspace iterate on the rational Krylov block of the sweep-start closed loop), so Z Z^T, the
gain and the residual after every step equal the sequential iteration's in exact arithmetic.  For G = 1 it IS the
sequential step: M = (I + G G^T) / (-2p).

Plain NumPy: dense saddle solves in FP64 (:func:`radi_sweeps`), ``np.longdouble`` for the small matrices
(:func:`sweep_data`) and for the recombination with its componentwise bounds (:func:`combine`,
:func:`combine_bounds`).  ``python tests/radi_sweep_model.py`` writes tests/golden/radi_sweep_model.npz.
"""
import functools

import numpy as np

import dense_model as dm
import radi_model as rm

LD = np.longdouble
PIVOT = 1e-5           # RICADI_RADI_SWEEP_PIVOT: the smallest Cauchy pivot of an admitted sweep (study below)
MAX_K = 128            # G m of a sweep
MAX_GROUPS = 16        # RICADI_MAX_GROUPS


# ----------------------------------------------------------------------------------------------- the small matrices
def sweep_matrix(ps, Ghat, m):
    """M (G m x G m) in longdouble."""
    ps = dm.ld(np.asarray(ps, dtype=float))
    Gh = dm.ld(Ghat)
    G = len(ps)
    M = np.zeros((G * m, G * m), dtype=LD)
    I = np.eye(m, dtype=LD)
    for g in range(G):
        for h in range(G):
            M[g * m:(g + 1) * m, h * m:(h + 1) * m] = -(I + Gh[g * m:(g + 1) * m] @ Gh[h * m:(h + 1) * m].T) / (
                ps[g] + ps[h])
    return M


def sweep_data(ps, Ghat, Gamma, m, nb, res_reltol, rhs, steps_left):
    """Items 3-5 of the sweep in longdouble.  ps (G), Ghat (G m x nb), Gamma ((G + 1) m x (G + 1) m), rhs =
    ||R^T R||_F of the iteration's first residual factor.  Returns (k, res, Cf): k kept steps -- the first j whose
    relative residual is <= res_reltol, else min(G, steps_left) --, res the relative residuals after steps 1 .. k, and
    Cf = [T_k | T_k y[:k m] | T_k h[:k m]]  (G m x (k m + m + nb))."""
    G = len(ps)
    K = G * m
    Gh, Gam = dm.ld(Ghat).reshape(K, nb), dm.ld(Gamma)
    L = rm._chol_ld(sweep_matrix(ps, Gh, m))
    if not np.all(np.isfinite(np.asarray(L, dtype=float))):
        raise FloatingPointError("M has a pivot that is not positive and finite")
    Li = rm._lower_inv_ld(L)
    y = Li @ np.tile(np.eye(m, dtype=LD), (G, 1))
    h = Li @ Gh
    LiT = Li.T
    res, k = [], 0
    for j in range(1, min(G, steps_left) + 1):
        c = np.vstack([np.eye(m, dtype=LD), LiT[:, :j * m] @ y[:j * m]])
        res.append(float(np.sqrt(np.sum((c.T @ Gam @ c) ** 2)) / LD(rhs)))
        k = j
        if res[-1] <= res_reltol:
            break
    T = LiT[:, :k * m]
    Cf = np.hstack([T, T @ y[:k * m], T @ h[:k * m]])
    return k, np.array(res), Cf


def sweep_data_bounds(ps, Ghat, m, Cf, u):
    """Normwise first-order bound on the entries of Cf computed in arithmetic of unit roundoff u and rounded to FP64,
    against sweep_data's: the Cholesky factor and its inverse are backward stable (Higham, ASNA, Thm 10.3, 8.5), so
    every product of L^-1 with itself or with a matrix of entries <= max|Gh| moves by at most ~ n gamma_n cond_2(M)
    times its norm; the rounding to FP64 adds 2^-53 |Cf|."""
    M = np.asarray(sweep_matrix(ps, Ghat, m), dtype=float)
    ev = np.linalg.eigvalsh(M)
    n = M.shape[0]
    kappa = ev[-1] / ev[0]
    return dm.U * np.abs(Cf) + 4.0 * n * dm.gamma(n + 2, u) * kappa * float(np.max(np.abs(Cf)))


def sweep_res_bounds(ps, Ghat, Gamma, m, Cf, k, res, rhs, u):
    """Bound on the relative residual after step k as the host entry computes it: T_k y in arithmetic of unit
    roundoff u (its error as in sweep_data_bounds) and rounded to FP64, then with c = [I; T_k y] the quadratic form
    c^T Gamma c (nc summed products twice) and its Frobenius norm (m^2 summed squares, the root, the division) in
    FP64: first order, with U = 2^-53,
    (2 gamma_nc(U) + 2 U + 8 n gamma_{n+2}(u) cond_2(M)) || |c|^T |Gamma| |c| ||_F / rhs + gamma_{m^2+3}(U) res."""
    M = np.asarray(sweep_matrix(ps, Ghat, m), dtype=float)
    ev = np.linalg.eigvalsh(M)
    n, nc = M.shape[0], M.shape[0] + m
    c = np.vstack([np.eye(m), np.abs(np.asarray(Cf, dtype=float)[:, k * m:k * m + m])])
    q = float(np.linalg.norm(c.T @ np.abs(np.asarray(Gamma, dtype=float)) @ c))
    return ((2.0 * dm.gamma(nc, dm.U) + 2.0 * dm.U + 8.0 * n * dm.gamma(n + 2, u) * ev[-1] / ev[0]) * q / rhs +
            dm.gamma(m * m + 3, dm.U) * res)


def smallest_pivot(ps):
    """min_j prod_{k<j} ((p_j - p_k) / (p_j + p_k))^2 of a sweep's shifts (0 where two are equal): the pivots of the
    Cauchy matrix C_gh = -1 / (p_g + p_h) relative to its diagonal (ricadi::cauchy_data)."""
    ps = [LD(p) for p in ps]
    out = LD(1)
    for j in range(len(ps)):
        piv = LD(1)
        for k in range(j):
            q = (ps[j] - ps[k]) / (ps[j] + ps[k])
            piv *= q * q
        out = min(out, piv)
    return float(out)


def panel_groups(mw, nb):
    """Column groups the batched solve makes of an (mw + nb)-wide panel: sixteen-column groups above 32 columns."""
    return -(-(mw + nb) // 16) if mw + nb > 32 else 1


def sweep_width(shifts, mw, nb, want, max_steps, pivot=PIVOT):
    """The effective width (ricadi_host_radi_sweep_width): the largest G <= want, ns, 128 / mw, MAX_GROUPS / groups,
    max_steps, halved until every sweep of the cycled list has distinct shifts and a smallest pivot >= pivot."""
    ns = len(shifts)
    G = max(1, min(want, ns, MAX_K // mw, MAX_GROUPS // panel_groups(mw, nb), max_steps))
    while G >= 2:
        nsweep = ns // np.gcd(ns, G)
        if all(smallest_pivot([shifts[(s * G + i) % ns] for i in range(G)]) >= pivot for s in range(nsweep)):
            return G
        G //= 2
    return 1


# ------------------------------------------------------------------------------------------------ the iteration
def radi_sweeps(calA, calE, J, B, W, shifts, width, old=None, max_steps=200, res_reltol=1e-10, perturb=None,
                record=None):
    """The iteration in sweeps of `width` steps (the last one as many as max_steps leaves) with dense saddle solves.
    Returns the dict of radi_model.radi, and 'sweeps', 'solves'.  perturb = (relative size, seed): every solve is
    multiplied entrywise by 1 + size * N(0, 1).  record (a list): (ps, Ghat, Gamma, rhs, steps_left, k, res, Cf) of
    every sweep."""
    calA, calE, J = rm._dn(calA), rm._dn(calE), rm._dn(J)
    B, W = rm._dn(B), rm._dn(W)
    nv, m = W.shape
    nb = B.shape[1]
    R = rm.project(calE, J, W)
    U = np.zeros_like(B) if old is None else -rm._dn(old)
    rhs = np.linalg.norm(R.T @ R)
    rng = None if perturb is None else np.random.default_rng(perturb[1])
    blocks, hist, stopped, sweeps, solves = [], [], "max_steps", 0, 0
    while len(hist) < max_steps and stopped != "res":
        left = max_steps - len(hist)
        G = min(width, left)
        ps = [float(shifts[(len(hist) + g) % len(shifts)]) for g in range(G)]
        A0 = calA - U @ B.T
        Vs = []
        for p in ps:
            V = rm.saddle_solve(A0 + p * calE, J, R)
            if rng is not None:
                V = V * (1.0 + perturb[0] * rng.standard_normal(V.shape))
            Vs.append(V)
        Vh = np.hstack(Vs)
        S = calE @ Vh
        P = np.hstack([R, S])
        Ghat, Gamma = Vh.T @ B, P.T @ P
        k, res, Cf = sweep_data(ps, Ghat, Gamma, m, nb, res_reltol, rhs, left)
        if record is not None:
            record.append((np.array(ps), Ghat, Gamma, rhs, left, k, res, Cf))
        Cf = np.asarray(Cf, dtype=float)
        km = k * m
        blocks.append(Vh @ Cf[:, :km])
        R = R + S @ Cf[:, km:km + m]
        U = U + S @ Cf[:, km + m:]
        hist.extend(res.tolist())
        sweeps += 1
        solves += G
        if hist[-1] <= res_reltol:
            stopped = "res"
    Z = np.hstack(blocks)
    return dict(Z=Z, gain=U if old is None else U + rm._dn(old), res_hist=np.array(hist), steps=len(hist),
                stopped=stopped, rhs=rhs, sweeps=sweeps, solves=solves)


# ---------------------------------------------------------------------------------------------- the recombination
def combine(Vh, S, Cf, k, m, RU):
    """(Z block, new [R | U]) in longdouble: Vh Cf[:, :k m] and RU + S Cf[:, k m:]."""
    Vh, S, Cf, RU = dm.ld(Vh), dm.ld(S), dm.ld(Cf), dm.ld(RU)
    return Vh @ Cf[:, :k * m], RU + S @ Cf[:, k * m:]


def combine_bounds(Vh, S, Cf, k, m, RU, u):
    """Componentwise bounds on what an FP64 implementation of combine (operands as stored, K = G m summed products in
    any order, one addition into [R | U]) may differ by from the exact result; first order in u:
    Z: gamma_K |Vh||Cf|;   [R | U]: gamma_{K+1} |S||Cf| + u |RU|."""
    K = np.shape(Vh)[1]
    aC = dm.fa(Cf)
    dZ = dm.gamma(K, u) * (dm.fa(Vh) @ aC[:, :k * m])
    dRU = dm.gamma(K + 1, u) * (dm.fa(S) @ aC[:, k * m:]) + u * dm.fa(RU)
    return dZ, dRU


# ------------------------------------------------------------------------------------------------------ the fixture
GOLDEN = "radi_sweep_model.npz"
PERTURB, SEEDS = 1e-10, (1, 2, 3)                              # the device's gmres_tol; three seeds
STUDY_N = 8
STUDY_LISTS = tuple((ns, dec, il) for ns in (16, 32) for dec in (3, 4) for il in (False, True))
STUDY_WIDTHS = (2, 4, 8)
# ... and neighbour lists (ns, decades, width) chosen for their pivots: between the refused 4.0e-7 and the 1.1e-5 of the
# lists above, and just above 1e-5
STUDY_GAP = ((40, 4, 8), (48, 5, 8), (28, 3, 8), (32, 3.5, 8), (24, 3, 16), (48, 3, 4), (20, 3, 16), (28, 3.5, 8),
             (24, 3, 8), (40, 3, 4))
GAIN_BAR = 1e-7                                                # a tenth of the project's parity bar


def golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)


def study_shifts(ns, decades, interleave):
    from optconpy_amd import problems as pb
    return pb.logshifts(1.0, 10.0 ** decades, ns, interleave=interleave)


def cycle_pivot(shifts, G):
    """The smallest pivot of any sweep of the cycled list at width G."""
    ns = len(shifts)
    return min(smallest_pivot([shifts[(s * G + i) % ns] for i in range(G)]) for s in range(ns // np.gcd(ns, G)))


@functools.lru_cache(maxsize=None)
def forms(N):
    return tuple(rm.call_forms(N))


def widths_of(form):
    ns = len(form["ms"])
    return [w for w in (1, 2, 4, 8, 16) if w <= ns]


def relerr(a, b):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(np.asarray(b)))


def compare_runs(seq, swp):
    """Largest deviations of a sweep run from the sequential model: Z Z^T and the gain (relative, Frobenius), the
    residual history entry by entry (absolute: the entries are relative to ||R_0^T R_0|| already)."""
    n = min(len(seq["res_hist"]), len(swp["res_hist"]))
    return (relerr(swp["Z"] @ swp["Z"].T, seq["Z"] @ seq["Z"].T), relerr(swp["gain"], seq["gain"]),
            float(np.max(np.abs(seq["res_hist"][:n] - swp["res_hist"][:n]))))


def study_case(f, shifts, width, seed):
    """Gain error of the perturbed sweep run against the equally perturbed sequential run (width 1)."""
    kw = dict(old=f["old"], max_steps=2 * len(shifts), res_reltol=1e-10)
    seq = radi_sweeps(f["calA"], f["calE"], f["J"], f["B"], f["W"], shifts, 1, perturb=(PERTURB, seed), **kw)
    swp = radi_sweeps(f["calA"], f["calE"], f["J"], f["B"], f["W"], shifts, width, perturb=(PERTURB, seed), **kw)
    return relerr(swp["gain"], seq["gain"])


def make_golden():
    """tests/golden/radi_sweep_model.npz: 'dev_<N>_<form>' the largest deviations (Z Z^T, gain, history) of the sweep
    model from radi_model.radi over the widths of a form at res_reltol 1e-12; 'study' the admissibility table, one
    row per (ns, decades, interleaved, width) of STUDY_LISTS x STUDY_WIDTHS, then of STUDY_GAP: [ns, decades,
    interleaved, width, smallest pivot, gain error of seeds 1, 2, 3]; 'pivot' the bound taken from it: the smallest
    power of ten for which every admitted row keeps the gain within GAIN_BAR."""
    out = {}
    for N in (4, 8):
        for f in forms(N):
            seq = rm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], f["ms"], old=f["old"], res_reltol=1e-12)
            dev = np.zeros(3)
            for w in widths_of(f):
                swp = radi_sweeps(f["calA"], f["calE"], f["J"], f["B"], f["W"], f["ms"], w, old=f["old"],
                                  res_reltol=1e-12)
                assert swp["steps"] == seq["steps"], (N, f["name"], w, swp["steps"], seq["steps"])
                dev = np.maximum(dev, compare_runs(seq, swp))
            out["dev_%d_%s" % (N, f["name"])] = dev
            print("N = %d %-8s: %d steps, deviations ZZ^T %.2e gain %.2e history %.2e" % (
                (N, f["name"], seq["steps"]) + tuple(dev)))
    f = forms(STUDY_N)[0]
    rows = []
    for ns, dec, il in STUDY_LISTS:
        shifts = study_shifts(ns, dec, il)
        for w in STUDY_WIDTHS:
            errs = [study_case(f, shifts, w, seed) for seed in SEEDS]
            rows.append([ns, dec, int(il), w, cycle_pivot(shifts, w)] + errs)
            print("ns %2d decades %d interleaved %d width %d: pivot %.2e gain errors %s" % (
                ns, dec, il, w, rows[-1][4], " ".join("%.2e" % e for e in errs)))
    for ns, dec, w in STUDY_GAP:
        shifts = study_shifts(ns, dec, False)
        errs = [study_case(f, shifts, w, seed) for seed in SEEDS]
        rows.append([ns, dec, 0, w, cycle_pivot(shifts, w)] + errs)
        print("ns %2d decades %g neighbours width %d: pivot %.2e gain errors %s" % (
            ns, dec, w, rows[-1][4], " ".join("%.2e" % e for e in errs)))
    rows = np.array(rows)
    out["study"] = rows
    pivot = 1.0
    while pivot > 1e-12 and all(np.max(r[5:]) <= GAIN_BAR for r in rows if r[4] >= pivot / 10.0):
        pivot /= 10.0
    out["pivot"] = np.array(pivot)
    print("smallest power of ten that admits only cases within %.0e: %.0e" % (GAIN_BAR, pivot))
    np.savez(golden_path(), **out)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    make_golden()
