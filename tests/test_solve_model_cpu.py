"""The model of tests/solve_model.py has teeth (no GPU): at the shapes of tests/test_gpu_solve_branches.py a float64
normal-equations implementation of the recycled guess meets the allowance the GPU test grants, and one injected fault
each -- the ones the batched solve's bookkeeping could commit without the final answer showing it -- misses it by
more than a factor 100.  The two Woodbury faults are held against the closed-loop LU at the suite's 1e-8.
"""
import numpy as np
import pytest

import solve_model as sm

SHIFTS = (-1.0, -30.0, -1000.0)
M = 16


@pytest.fixture(scope="module")
def op(cfg1):
    pr = cfg1[0]
    calA = (-pr.A - pr.Nc).T.tocsr()
    calE = pr.M.T.tocsr()
    lus = {p: sm.closed_loop(calA, calE, pr.J, p) for p in SHIFTS}
    return pr, calA, calE, lus


@pytest.fixture(scope="module")
def history(op):
    """Five successive 16-column right-hand sides at depth 3 with the LU's solutions, and a sixth to guess for."""
    pr, _, _, lus = op
    rng = np.random.default_rng(40)
    Bs = [rng.standard_normal((pr.NV, M)) for _ in range(6)]
    Ys = [[lus[p][1].solve(sm.pad(B, pr.NV + pr.NP)) for B in Bs[:5]] for p in SHIFTS]
    ring = sm.RecycleRing(3)
    for e in range(5):
        ring.store(SHIFTS, Bs[e], [Ys[g][e] for g in range(3)])
    return Bs, Ys, ring


def _errs(X, model):
    return max(sm.rel(x, xm) for x, xm in zip(X, model["X"]))


def test_ring_semantics(history):
    Bs, Ys, ring = history
    g = ring.guess(SHIFTS, Bs[5])
    assert g["cols"] == 48 and g["serials"] == [3, 4, 5]          # the first two right-hand sides play no part
    assert ring.guess(SHIFTS + (-7.0,), Bs[5]) is None            # a shift without solutions: no guess
    assert ring.guess(SHIFTS[:1], Bs[5])["cols"] == 48            # a subset of the shifts
    # a stored right-hand side comes back as its stored solution
    g = ring.guess(SHIFTS, Bs[3])
    assert _errs([Ys[k][3] for k in range(3)], g) < 1e-12
    ring2 = sm.RecycleRing(3)
    assert ring2.guess(SHIFTS, Bs[0]) is None
    ring2.store(SHIFTS, Bs[0], [Ys[k][0] for k in range(3)])
    ring2.clear()
    assert ring2.guess(SHIFTS, Bs[0]) is None


def test_normal_equations_meet_the_allowance(history):
    Bs, Ys, ring = history
    g = ring.guess(SHIFTS, Bs[5])
    allow, kappa = sm.guess_allowance(g["B"])
    X = sm.normal_equations_guess(Bs[2:5], [Ys[k][2:5] for k in range(3)], Bs[5])
    err = _errs(X, g)
    print("kappa %.3g  error %.3g  allowance %.3g" % (kappa, err, allow))
    assert kappa < 2.0 and err <= allow


def test_mixed_widths_meet_the_allowance(op):
    """Widths 16, 5, 16 (21 stored columns before the third call)."""
    pr, _, _, lus = op
    rng = np.random.default_rng(41)
    Bs = [rng.standard_normal((pr.NV, w)) for w in (16, 5, 16)]
    Ys = [[lus[p][1].solve(sm.pad(B, pr.NV + pr.NP)) for B in Bs[:2]] for p in SHIFTS]
    ring = sm.RecycleRing(3)
    for e in range(2):
        ring.store(SHIFTS, Bs[e], [Ys[g][e] for g in range(3)])
    g = ring.guess(SHIFTS, Bs[2])
    assert g["cols"] == 21
    allow, _ = sm.guess_allowance(g["B"])
    assert _errs(sm.normal_equations_guess(Bs[:2], Ys, Bs[2]), g) <= allow
    # fault: the 5-column entry read with the leading dimension of a 16-column one
    flat = Bs[1].ravel()
    idx = (np.arange(pr.NV)[:, None] * 16 + np.arange(5)[None, :]) % flat.size
    bad = sm.normal_equations_guess([Bs[0], flat[idx]], Ys, Bs[2])
    assert _errs(bad, g) > 100 * allow


@pytest.mark.parametrize("fault", ["evicted_slot", "neighbour_rhs", "gram_not_mirrored"])
def test_guess_faults_miss_the_allowance(history, fault):
    Bs, Ys, ring = history
    g = ring.guess(SHIFTS, Bs[5])
    allow, _ = sm.guess_allowance(g["B"])
    B3, Y3 = Bs[2:5], [Ys[k][2:5] for k in range(3)]
    if fault == "evicted_slot":        # the right-hand side the fourth store evicted still sits in its slot
        X = sm.normal_equations_guess([Bs[0], Bs[3], Bs[4]], Y3, Bs[5])
    elif fault == "neighbour_rhs":     # solutions paired with the neighbouring right-hand side
        X = sm.normal_equations_guess(B3, [y[1:] + y[:1] for y in Y3], Bs[5])
    else:
        X = sm.normal_equations_guess(B3, Y3, Bs[5], mirror=False)
    err = _errs(X, g)
    print(fault, "error %.3g  allowance %.3g" % (err, allow))
    assert err > 100 * allow


@pytest.mark.parametrize("q", [1, 3, 8])
def test_woodbury_model_and_its_faults(op, q):
    pr, calA, calE, lus = op
    n = pr.NV + pr.NP
    rng = np.random.default_rng(42 + q)
    U = 0.1 * rng.standard_normal((pr.NV, q))
    V = 0.1 * rng.standard_normal((pr.NV, q))
    V2 = 0.1 * rng.standard_normal((pr.NV, q))
    b = rng.standard_normal((pr.NV, M))
    for p in SHIFTS:
        S2, lu2 = sm.closed_loop(calA, calE, pr.J, p, 1.0, U, V2)
        ref = sm.lu_solve(S2, lu2, b)
        assert sm.relres(S2, ref, b).max() <= 1e-10 / 100      # what the GPU test asks of its reference
        x, Z, cap = sm.smw(lus[p][1], U, V2, b)
        assert sm.rel(x, ref) < sm.LU_TOL
        # fault: W of the previous low-rank term (U, V) applied after V changed
        _, Zo, capo = sm.smw(lus[p][1], U, V, b)
        y = lus[p][1].solve(sm.pad(b, n))
        stale = y + sm.woodbury_w(Zo, capo) @ (V2.T @ y[:pr.NV])
        assert sm.rel(stale, ref) > 100 * sm.LU_TOL
        # fault: pressure rows of the augmented columns [b, U] not zeroed
        xt, _, _ = sm.smw(lus[p][1], U, V2, b, tail=rng.standard_normal((pr.NP, q)))
        assert sm.rel(xt, ref) > 100 * sm.LU_TOL


def test_refinement_construction_is_sound(op):
    """U2 = U T with T = (V^T S^-1 U)^-1 (1 - delta) makes the capacitance matrix delta I; the closed-loop LU's own
    residual stays a factor 100 below the loose tolerance 1e-8 for the deltas the GPU test uses."""
    pr, calA, calE, lus = op
    n, p, q = pr.NV + pr.NP, -30.0, 3
    rng = np.random.default_rng(50)
    U = 0.1 * rng.standard_normal((pr.NV, q))
    V = 0.1 * rng.standard_normal((pr.NV, q))
    b = rng.standard_normal((pr.NV, M))
    Z = lus[p][1].solve(sm.pad(U, n))
    for delta in (1e-1, 1e-2, 1e-3):
        U2 = U @ (np.linalg.inv(V.T @ Z[:pr.NV]) * (1.0 - delta))
        _, _, cap = sm.smw(lus[p][1], U2, V, b)
        assert np.abs(cap - delta * np.eye(q)).max() < 1e-9
        S2, lu2 = sm.closed_loop(calA, calE, pr.J, p, 1.0, U2, V)
        assert sm.relres(S2, sm.lu_solve(S2, lu2, b), b).max() <= 1e-8 / 100
