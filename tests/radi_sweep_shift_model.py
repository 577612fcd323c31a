"""Model of RADI sweeps whose shifts are generated from the iteration itself (``ms='hamiltonian-sweep'``,
ricadi_set_radi_sweep_shifts): the sweep form of tests/radi_sweep_model.py with a shift list per sweep,
chosen by the dominant rule of tests/radi_dominant_model.py from ALL blocks the sweep kept.

State at the end of a sweep that kept k blocks of m columns: [R | U], B and the kept group of Z.

    basis        Zg = the last min(k, 127 // m) kept blocks (c <= 127 columns),  Q Rq = Zg (thin QR),
                 S = dominant(Rq) (at most 32 left singular vectors, RANK_TOL), the basis is Q S;
                 H = Q^T [cal A Q | cal E Q | R | U | B]  (c x (2c + m + 2nb)), rotated to k' x (2k' + m + 2nb)
    candidates   radi_shift_model.select's: eigenvalues of Ham with Re < 0, one of each conjugate pair, criterion
                 ||q|| / ||x|| of the extended-precision null vector, shift -|lambda|; ordered by descending criterion,
                 on an exact tie the larger |lambda| first
    selection    walk the candidates in that order; accept p if it is finite and negative and
                 smallest_pivot(accepted + [p]) >= PIVOT; stop at G.  The next sweep solves the accepted shifts in
                 acceptance order
    cap          G = min(width, 128 // m, 16 // panel_groups(m, nb), steps left); no halving
    first sweep  one step with fallback[0]
    fallback     no admitted candidate (or a refused selection): ONE step with the next entry of the caller's list
                 (a counter of its own, starting at fallback[1], cycling)

At width 1 this is radi_dominant_model.radi: one block per sweep, the best candidate (a single shift always has
pivot 1).  ``python tests/radi_sweep_shift_model.py`` writes tests/golden/radi_sweep_shift_model.npz.
"""
import functools

import numpy as np

import radi_dominant_model as dmm
import radi_model as rm
import radi_shift_model as sm
import radi_sweep_model as swm

MAX_C = 127            # columns of the selection's group of Z (the device QR's and reduction's limit)


def cap_width(width, m, nb, steps_left):
    return max(1, min(width, swm.MAX_K // m, swm.MAX_GROUPS // swm.panel_groups(m, nb), steps_left))


def rotate(H, c, m, nb, S):
    """radi_dominant_model.rotate for a basis of c columns against an m-column residual: the packed H of Q S
    (k x (2k + m + 2nb)) from the packed H of Q (c x (2c + m + 2nb))."""
    H = np.asarray(H, dtype=float).reshape(c, 2 * c + m + 2 * nb)
    return np.ascontiguousarray(np.hstack([S.T @ H[:, :c] @ S, S.T @ H[:, c:2 * c] @ S, S.T @ H[:, 2 * c:]]))


def candidates(k, m, nb, H):
    """All candidates of radi_shift_model.select on a packed H, ordered: (shifts -|lambda|, criteria), descending
    criterion, on an exact tie the larger |lambda| first."""
    Ham = sm.hamiltonian(k, m, nb, H)
    lam = np.linalg.eigvals(Ham)
    cands = [i for i in range(lam.size) if lam[i].real < 0 and lam[i].imag >= 0]
    if not cands:
        return np.zeros(0), np.zeros(0)
    HamL = np.asarray(Ham, dtype=np.longdouble)
    crit = []
    for i in cands:
        x = sm.null_vector(HamL - np.clongdouble(lam[i]) * np.eye(2 * k, dtype=np.longdouble))
        crit.append(float(np.sqrt(np.sum(np.abs(x[k:]) ** 2) / np.sum(np.abs(x) ** 2))))
    mod = np.abs(lam[cands])
    order = sorted(range(len(cands)), key=lambda i: (-crit[i], -mod[i]))
    return -mod[order], np.array(crit)[order]


def greedy(ps, want, pivot=swm.PIVOT):
    """Indices of the candidates admitted, in acceptance order: finite, negative, and the smallest Cauchy pivot of
    the accepted list with the candidate appended stays >= pivot; at most `want`."""
    acc, idx = [], []
    for i, p in enumerate(ps):
        if len(acc) >= want:
            break
        if not (np.isfinite(p) and p < 0.0):
            continue
        if swm.smallest_pivot(acc + [float(p)]) >= pivot:
            acc.append(float(p))
            idx.append(i)
    return idx


def next_shifts(c, m, nb, H, Rq, want):
    """(admitted shifts in acceptance order, their criteria, k', all ordered candidates, all ordered criteria) of the
    rule on what a sweep has fetched: dominant -> rotate -> candidates -> greedy."""
    S = dmm.dominant(Rq)
    k = S.shape[1]
    ps, crit = candidates(k, m, nb, rotate(H, c, m, nb, S))
    idx = greedy(ps, want)
    return ps[idx], crit[idx], k, ps, crit


def radi(calA, calE, J, B, W, fallback, width, old=None, max_steps=200, res_reltol=1e-10, perturb=None, record=None,
         refuse=()):
    """The iteration.  Returns the dict of radi_dominant_model.radi plus 'sweeps', 'solves', 'widths' (solves of every
    sweep), 'kept_blocks' (steps kept by every sweep), 'basis_blocks' (blocks of Z in every selection's group).
    'kept': k' of every selection.  record (a list): (c, m, nb, H, Rq, want) of every selection.  perturb as in
    radi_dominant_model.radi.  refuse: the selection after a sweep whose last kept step (1-based) is listed counts as
    refused (ricadi_probe_radi_refuse)."""
    calA, calE, J = rm._dn(calA), rm._dn(calE), rm._dn(J)
    B, W = rm._dn(B), rm._dn(W)
    nv, m = W.shape
    nb = B.shape[1]
    R = rm.project(calE, J, W)
    U = np.zeros_like(B) if old is None else -rm._dn(old)
    rhs = np.linalg.norm(R.T @ R)
    rng = None if perturb is None else np.random.default_rng(perturb[1])
    refuse = set(int(v) for v in refuse)
    blocks, hist, ms, kept, widths, kblocks, bblocks = [], [], [], [], [], [], []
    stopped, solves, nfb, fallbacks = "max_steps", 0, 1, 0
    ps = [float(fallback[0])]
    while len(hist) < max_steps and stopped != "res":
        left = max_steps - len(hist)
        G = len(ps)
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
        k, res, Cf = swm.sweep_data(ps, Vh.T @ B, P.T @ P, m, nb, res_reltol, rhs, left)
        Cf = np.asarray(Cf, dtype=float)
        km = k * m
        blocks.append(Vh @ Cf[:, :km])
        R = R + S @ Cf[:, km:km + m]
        U = U + S @ Cf[:, km + m:]
        hist.extend(res.tolist())
        ms.extend(ps[:k])
        widths.append(G)
        kblocks.append(k)
        solves += G
        if hist[-1] <= res_reltol:
            stopped = "res"
            break
        if len(hist) >= max_steps:
            break
        nblk = min(k, MAX_C // m)
        Zg = blocks[-1][:, (k - nblk) * m:]
        c = nblk * m
        Q, Rq = np.linalg.qr(Zg)
        H = sm.pack(Q, calA, calE, R, U, B)
        want = cap_width(width, m, nb, max_steps - len(hist))
        if record is not None:
            record.append((c, m, nb, H.copy(), Rq.copy(), want))
        sel, _, kk, _, _ = next_shifts(c, m, nb, H, Rq, want)
        kept.append(kk)
        bblocks.append(nblk)
        if len(sel) == 0 or len(hist) in refuse:
            ps = [float(fallback[nfb % len(fallback)])]
            nfb += 1
            fallbacks += 1
        else:
            ps = [float(p) for p in sel]
    Z = np.hstack(blocks)
    return dict(Z=Z, gain=U if old is None else U + rm._dn(old), res_hist=np.array(hist), steps=len(hist),
                stopped=stopped, rhs=rhs, ms=np.array(ms), fallbacks=fallbacks, kept=np.array(kept, dtype=int),
                sweeps=len(widths), solves=solves, widths=np.array(widths, dtype=int),
                kept_blocks=np.array(kblocks, dtype=int), basis_blocks=np.array(bblocks, dtype=int))


# ---------------------------------------------------------------------------------------------------- the problems
@functools.lru_cache(maxsize=None)
def random_form(N, mw):
    """The steady form of radi_model.call_forms(N) with a random W of mw columns of equal size (G mw = 128 at mw = 16,
    width 8: the basis cannot hold all eight blocks)."""
    f = dict(rm.call_forms(N)[0])
    f["name"] = "random%d" % mw
    f["W"] = np.random.default_rng(11).standard_normal((f["calA"].shape[0], mw))
    f["kw"] = dict(f["kw"], wmat=f["W"])
    return f


@functools.lru_cache(maxsize=None)
def case_form(name, N):
    """A case of the table by name: 'steady' / 'dre' / 'dre_old' (radi_model.call_forms), 'wide33' / 'wide58'
    (radi_dominant_model.wide_form), 'random16'."""
    if name.startswith("wide"):
        return dmm.wide_form(N, int(name[4:]))
    if name.startswith("random"):
        return random_form(N, int(name[6:]))
    return [f for f in rm.call_forms(N) if f["name"] == name][0]


@functools.lru_cache(maxsize=None)
def run_case(name, N, width, res_reltol=1e-10, perturb=None, max_steps=200):
    """The model's run on a case (shared by the tests: treat as read-only), its selection records under 'record'."""
    f = case_form(name, N)
    rec = []
    out = radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], [sm.initial_shift(f["calA"], f["calE"])], width,
               old=f["old"], max_steps=max_steps, res_reltol=res_reltol, perturb=perturb, record=rec)
    out["record"] = rec
    return out


# ------------------------------------------------------------------------------------------------------ the fixture
GOLDEN = "radi_sweep_shift_model.npz"
PERTURB, SEEDS = 1e-10, (1, 2, 3)                              # the device's gmres_tol; three seeds
MOVE_BAR = 1e-4                                                # a case takes part in shift-by-shift comparisons below it
# (name, N, width) of the table in DESIGN.md 3d-4
TABLE = tuple((n, N, w) for N in (4, 8) for n in ("steady", "dre") for w in (2, 4, 8)) + (
    ("wide33", 8, 2), ("wide33", 8, 3), ("wide58", 8, 2), ("random16", 8, 4), ("random16", 8, 8))
# the cases that must take part (their shifts moved by at most 3.2e-6 in the study)
MUST_TAKE_PART = tuple(("steady", N, w) for N in (4, 8) for w in (2, 4, 8)) + (("wide33", 8, 2), ("wide33", 8, 3))


def key(name, N, width):
    return "%s_%d_w%d" % (name, N, width)


def golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)


def case_moves(name, N, width):
    """(largest relative move of a shift per seed, step counts equal per seed) when every solve is perturbed by
    PERTURB; a run whose widths differ from the unperturbed one's counts as a move of 1."""
    r = run_case(name, N, width)
    moves, same = [], []
    for seed in SEEDS:
        q = run_case(name, N, width, perturb=(PERTURB, seed))
        same.append(q["steps"] == r["steps"])
        if len(q["ms"]) != len(r["ms"]) or not np.array_equal(q["widths"], r["widths"]):
            moves.append(1.0)
            continue
        moves.append(float(np.max(np.abs(q["ms"] - r["ms"]) / np.abs(r["ms"]))))
    return np.array(moves), np.array(same)


def make_golden():
    """tests/golden/radi_sweep_shift_model.npz: per case of TABLE 'table_<key>' = [steps, sweeps, solves],
    'widths_<key>', 'kblocks_<key>', 'kept_<key>', 'ms_<key>', 'res_<key>' of the run at 1e-10, 'moves_<key>' the
    largest relative move of a shift per seed under the perturbation, 'same_<key>' whether the step count stayed;
    'participants' the keys whose moves stay below MOVE_BAR under all three seeds."""
    out, part = {}, []
    for name, N, w in TABLE:
        r = run_case(name, N, w)
        k = key(name, N, w)
        out["table_" + k] = np.array([r["steps"], r["sweeps"], r["solves"]])
        out["widths_" + k] = r["widths"]
        out["kblocks_" + k] = r["kept_blocks"]
        out["kept_" + k] = r["kept"]
        out["ms_" + k] = r["ms"]
        out["res_" + k] = r["res_hist"]
        moves, same = case_moves(name, N, w)
        out["moves_" + k] = moves
        out["same_" + k] = same
        if np.all(moves < MOVE_BAR):
            part.append(k)
        print("%-16s %2d steps / %d sweeps / %2d solves, widths %s, fallbacks %d, moves %s, steps kept %s" % (
            k, r["steps"], r["sweeps"], r["solves"], r["widths"].tolist(), r["fallbacks"],
            " ".join("%.1e" % v for v in moves), same.tolist()))
    out["participants"] = np.array(part)
    np.savez(golden_path(), **out)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    make_golden()
