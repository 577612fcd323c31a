"""Model of RADI with generated shifts on the DOMINANT basis (RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT; DESIGN.md
3d-2): tests/radi_shift_model.radi with one change.  With Q R the QR of the new block of Z, the basis of the selection
is Q S, S (m x k) the left singular vectors of R of its k = min(32, #{sigma_i >= RANK_TOL sigma_1}) largest singular
values (NumPy's ``svd``).  ``keep_columns`` / ``restrict`` of the column rule become ``dominant(Rq)`` -> S and
``rotate(H, m, nb, S)``; the selection itself (``radi_shift_model.select``) is the same.

Q S spans the dominant part of the block's range whatever the order of the block's columns, and the selection is of
order 2k <= 64 for a block of any width: the rule serves right-hand-side factors wider than 32 columns (the sweep's
W = [M^T Z_c, sqrt(tau) C~^T]), and the column rule's restriction "dependent columns last" does not apply to it.
"""
import functools

import numpy as np

import radi_model as rm
import radi_shift_model as sm

K_MAX = 32


def dominant(Rq):
    """S (m x k): the left singular vectors of the block's R of the k = min(32, #{sigma_i >= RANK_TOL sigma_1})
    largest singular values."""
    U, s, _ = np.linalg.svd(np.asarray(Rq, dtype=float))
    k = min(K_MAX, int(np.sum(s >= sm.RANK_TOL * s[0])))
    return U[:, :k]


def rotate(H, m, nb, S):
    """The packed H of the basis Q S (k x (2k + m + 2nb)) from the packed H of Q (m x (3m + 2nb)):
    [S^T H_A S | S^T H_E S | S^T (H_R, H_U, H_B)] -- what the driver does on the host with the H it fetched."""
    H = np.asarray(H, dtype=float).reshape(m, 3 * m + 2 * nb)
    return np.ascontiguousarray(np.hstack([S.T @ H[:, :m] @ S, S.T @ H[:, m:2 * m] @ S, S.T @ H[:, 2 * m:]]))


def next_shift(m, nb, H, Rq):
    """(p, margin, k) of the rule on what a step has fetched: dominant -> rotate -> select."""
    S = dominant(Rq)
    k = S.shape[1]
    p, margin, _, _ = sm.select(k, m, nb, rotate(H, m, nb, S))
    return p, margin, k


def radi(calA, calE, J, B, W, fallback, old=None, max_steps=200, res_reltol=1e-10, record_full=None, perturb=None):
    """radi_shift_model.radi on the dominant basis; the same returned dict.  record_full (a list): (m, nb, H, Rq) of
    every selection, H the packed m x (3m + 2nb) matrix of ALL columns of the block's Q -- what the device fetches.
    perturb = (relative size, seed): every solve V is multiplied entrywise by 1 + size * N(0, 1), the model of a
    device whose iterative solves stop at that relative accuracy."""
    calA, calE, J = rm._dn(calA), rm._dn(calE), rm._dn(J)
    B, W = rm._dn(B), rm._dn(W)
    nv, m = W.shape
    nb = B.shape[1]
    R = rm.project(calE, J, W)
    U = np.zeros_like(B) if old is None else -rm._dn(old)
    rhs = np.linalg.norm(R.T @ R)
    rng = None if perturb is None else np.random.default_rng(perturb[1])
    blocks, hist, ms, margins, kept, stopped = [], [], [], [], [], "max_steps"
    p, nfb, fallbacks = float(fallback[0]), 1, 0
    for j in range(max_steps):
        ms.append(p)
        V = rm.saddle_solve(calA - U @ B.T + p * calE, J, R)
        if rng is not None:
            V = V * (1.0 + perturb[0] * rng.standard_normal(V.shape))
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
        if j + 1 == max_steps:
            break
        Q, Rq = np.linalg.qr(blocks[-1])
        H = sm.pack(Q, calA, calE, R, U, B)
        if record_full is not None:
            record_full.append((m, nb, H.copy(), Rq.copy()))
        pn, margin, k = next_shift(m, nb, H, Rq)
        kept.append(k)
        if not (np.isfinite(pn) and pn < 0.0):
            pn = float(fallback[nfb % len(fallback)])
            nfb += 1
            fallbacks += 1
        else:
            margins.append(margin)
        p = float(pn)
    Z = np.hstack(blocks)
    return dict(Z=Z, gain=U if old is None else U + rm._dn(old), res_hist=np.array(hist), steps=len(hist),
                stopped=stopped, rhs=rhs, ms=np.array(ms), margins=np.array(margins), fallbacks=fallbacks,
                kept=np.array(kept, dtype=int))


# ------------------------------------------------------------------------------------------------- the wide problems
WIDE = ((4, 33), (4, 48), (8, 33), (8, 48), (8, 58))          # (N, mw) of the table in DESIGN.md 3d-2
STEPS = {(4, 33): 16, (4, 48): 16, (8, 33): 19, (8, 48): 18, (8, 58): 19}
STEPS_CYCLED = {(4, 33): 28, (4, 48): 29, (8, 33): 30, (8, 48): 30, (8, 58): 30}


def wide_w(nv, mw):
    """The wide right-hand-side factor of the tests: graded columns and eight of full size, as a sweep's
    W = [M^T Z_c, sqrt(tau) C~^T]."""
    W = np.random.default_rng(7).standard_normal((nv, mw))
    return W * np.concatenate([np.logspace(0, -4, mw - 8), np.ones(8)])


@functools.lru_cache(maxsize=None)
def wide_form(N, mw):
    """The steady form of radi_model.call_forms(N) with the wide W in place of its own."""
    f = dict(rm.call_forms(N)[0])
    f["name"] = "wide%d" % mw
    f["W"] = wide_w(f["calA"].shape[0], mw)
    f["kw"] = dict(f["kw"], wmat=f["W"])
    f["p0"] = sm.initial_shift(f["calA"], f["calE"])
    return f


@functools.lru_cache(maxsize=None)
def wide_run(N, mw, res_reltol=1e-10, perturb=None, max_steps=200):
    """The model's run on wide_form(N, mw) (shared by the tests: treat as read-only), with its record_full list
    under 'full'."""
    f = wide_form(N, mw)
    full = []
    out = radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], [f["p0"]], max_steps=max_steps, res_reltol=res_reltol,
               record_full=full, perturb=perturb)
    out["full"] = full
    return out


# ------------------------------------------------------------------------------------------------------ the fixture
GPU_CASES = ((4, 33), (4, 48), (8, 33), (8, 58))              # the whole solves of tests/test_gpu_radi_dominant.py
PERTURB, SEEDS = 1e-10, (1, 2, 3)                              # the device's gmres_tol; three seeds
GOLDEN = "radi_dominant_model.npz"


def golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", GOLDEN)


def make_golden():
    """tests/golden/radi_dominant_model.npz: per GPU case the model's shifts and residual history at 1e-10 and the
    largest relative move of a shift when every solve is perturbed by PERTURB, per seed (runs of the steps both have).
    ``python tests/radi_dominant_model.py`` writes it (about two minutes); tests/test_radi_dominant_cpu.py checks the
    stored shifts against the live model."""
    out = {}
    for N, mw in GPU_CASES:
        r = wide_run(N, mw)
        out["ms_%d_%d" % (N, mw)] = r["ms"]
        out["res_%d_%d" % (N, mw)] = r["res_hist"]
        moves = []
        for seed in SEEDS:
            q = wide_run(N, mw, perturb=(PERTURB, seed))
            k = min(len(q["ms"]), len(r["ms"]))
            moves.append(float(np.max(np.abs(q["ms"][:k] - r["ms"][:k]) / np.abs(r["ms"][:k]))))
            assert q["steps"] == r["steps"], (N, mw, seed, q["steps"], r["steps"])
        out["moves_%d_%d" % (N, mw)] = np.array(moves)
        print("N = %d mw = %d: %d steps, shifts move by %s under a relative perturbation of %.0e" % (
            N, mw, r["steps"], ", ".join("%.2e" % v for v in moves), PERTURB))
    np.savez(golden_path(), **out)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    make_golden()
