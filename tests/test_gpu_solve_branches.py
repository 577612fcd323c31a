"""GPU tests of the layer that strings the kernels into a batched shift solve (solver_gmres.inl, gmres_core_any down
to solve_batch): recycled initial guesses, Sherman-Morrison-Woodbury, storage escalation, the reported residual, the
wide-panel split.  Almost every branch of that layer is a safety net over the one before it, so "the solution agrees
with an LU" cannot see a defect in it.  Here every case asserts, from the context's branch trace
(``Context.solve_trace``), that the branch it is named for ran, and holds its result against the FP64 model of
tests/solve_model.py: the recycled guess (read through ``Context.recycle_guess_dev``) against the least-squares
combination it claims to be, Woodbury solutions against an LU of the closed-loop matrix, reported residuals against
residuals evaluated on the host.  ``test_counters_reached`` lists the coverage.

Operators: ``ricc_problem(15, 0.05)`` (cfg1's size, NV = 1682, NP = 255), ``ricc_problem(8, 0.1)`` (NV = 450, NP = 80)
where the size does not matter, ``ricc_problem(15, 0.005)`` for the escalation.  Solution buffers are pre-filled with
NaN.  Bounds: see ``solve_model.guess_allowance``; 1e-8 against an LU is the suite's; a residual evaluated a second
time may differ by rounding, hence 1.1 x gmres_tol -- with the reference's own residual asserted below gmres_tol / 100.
"""
import math

import numpy as np
import pytest

import solve_model as sm
from optconpy_amd import _lib, problems as pb

pytestmark = pytest.mark.gpu
SHIFTS = (-1.0, -30.0, -1000.0)
TOL = 1e-10            # the library's default gmres_tol
SEEN = set()           # trace counters that were nonzero when a context of this file was closed
RATIOS = {}            # family -> largest error / allowance
NOTES = {}


class Op:
    def __init__(self, N, nu):
        pr = pb.ricc_problem(N, nu)
        self.calA = (-pr.A - pr.Nc).T.tocsr()
        self.calE = pr.M.T.tocsr()
        self.J = pr.J
        self.NV, self.NP = pr.NV, pr.NP
        self.n = pr.NV + pr.NP
        self._plain = {}

    def plain(self, p):
        if p not in self._plain:
            self._plain[p] = sm.closed_loop(self.calA, self.calE, self.J, p)
        return self._plain[p]


@pytest.fixture(scope="module")
def big():
    return Op(15, 0.05)


@pytest.fixture(scope="module")
def small():
    return Op(8, 0.1)


@pytest.fixture(scope="module")
def hard():
    return Op(15, 0.005)


class Dev:
    """A context on an operator; panels go through torch tensors, solutions start as NaN."""

    def __init__(self, op, **opts):
        self.op = op
        self.ctx = _lib.Context(0, **opts)
        self.ctx.set_operator(op.calA, op.calE, op.J)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        SEEN.update(k for k, v in self.ctx.solve_trace().items() if v > 0)
        self.ctx.close()

    def trace(self):
        return self.ctx.solve_trace()

    def _buffers(self, ng, B):
        import torch
        Rd = torch.from_numpy(np.ascontiguousarray(B, dtype=np.float64)).cuda()
        Xd = torch.full((ng, self.op.n, B.shape[-1]), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()          # the library runs on its own stream
        return Rd, Xd

    def solve(self, ps, B, strict=True):
        """B: NV x m shared by the shifts ``ps``, or [len(ps)] x NV x m.  Returns (iters, relres, X)."""
        Rd, Xd = self._buffers(len(ps), B)
        stride = 0 if B.ndim == 2 else B.shape[1] * B.shape[2]
        its, rr = self.ctx.shift_solve_batch_dev(ps, [1.0] * len(ps), Rd.data_ptr(), stride, B.shape[-1],
                                                 Xd.data_ptr(), strict=strict)
        self.ctx.synchronize()
        return list(its), np.asarray(rr), Xd.cpu().numpy()

    def probe(self, ps, B):
        Rd, Xd = self._buffers(len(ps), B)
        rank = self.ctx.recycle_guess_dev(ps, [1.0] * len(ps), Rd.data_ptr(), B.shape[1], Xd.data_ptr())
        self.ctx.synchronize()
        return rank, Xd.cpu().numpy()


def _diff(t1, t0):
    return {k: t1[k] - t0[k] for k in t1}


def _ratio(family, r):
    RATIOS[family] = max(RATIOS.get(family, 0.0), float(r))


def _check_guess(X, model, tag, family="guess"):
    """The probe's guess against the model's, per group, relative to ||x_model||_F."""
    allow, kappa = sm.guess_allowance(model["B"])
    worst = max(sm.rel(X[g], model["X"][g]) for g in range(len(X)))
    print("[solve branches] %s: %d stored columns, kappa %.3g, error %.3g, allowance %.3g" %
          (tag, model["cols"], kappa, worst, allow))
    _ratio(family, worst / allow)
    assert worst <= allow, (tag, worst, allow)


def _check_solution(op, ps, B, X, tag, tol=TOL, lowrank=None, family="lu"):
    """Solutions against the LU of the (closed-loop) matrix at 1e-8, and their residual evaluated here."""
    for g, p in enumerate(ps):
        if lowrank is None:
            S, lu = op.plain(p)
        else:
            S, lu = sm.closed_loop(op.calA, op.calE, op.J, p, 1.0, *lowrank)
        Bg = B if B.ndim == 2 else B[g]
        ref = sm.lu_solve(S, lu, Bg)
        ref_res = sm.relres(S, ref, Bg).max()
        assert ref_res <= tol / 100, (tag, p, ref_res)              # the margin below cannot hide a miss
        err = sm.rel(X[g], ref)
        res = sm.relres(S, X[g], Bg).max()
        print("[solve branches] %s p=%g: vs LU %.3g, residual %.3g (reference's own %.3g)" % (tag, p, err, res, ref_res))
        _ratio(family, err / sm.LU_TOL)
        _ratio(family + "_residual", res / (1.1 * tol))
        assert err <= sm.LU_TOL, (tag, p, err)
        assert res <= 1.1 * tol, (tag, p, res)


# ------------------------------------------------------------------------------------------------ recycling
def test_ring_of_three_five_right_hand_sides(big):
    """Depth 3, five successive random 16-column right-hand sides, three shifts: before calls 2 .. 5 the guess is the
    model's, from 16, 32, 48, 48 stored columns on the side-by-side panel path at full rank; after the fifth store the
    first two right-hand sides play no part (the guess for the first is not its old solution)."""
    rng = np.random.default_rng(100)
    Bs = [rng.standard_normal((big.NV, 16)) for _ in range(5)]
    ring = sm.RecycleRing(3)
    Xs = []
    with Dev(big) as d:
        d.ctx.set_recycle(3)
        for k in range(5):
            if k:
                rank, Xg = d.probe(SHIFTS, Bs[k])
                t = d.trace()
                g = ring.guess(SHIFTS, Bs[k])
                want = (16, 32, 48, 48)[k - 1]
                assert (t["guess_cols"], g["cols"], rank, t["guess_rank"], t["guess_pan"]) == (want,) * 4 + (1,), (k, t)
                _check_guess(Xg, g, "ring of three, call %d" % (k + 1))
            t0 = d.trace()
            its, rr, X = d.solve(SHIFTS, Bs[k])
            dt = _diff(d.trace(), t0)
            assert (dt["solves"], dt["guess_tried"], dt["guess_used"], dt["stored"]) == (1, 1, int(k > 0), 1), dt
            assert rr.max() <= TOL
            ring.store(SHIFTS, Bs[k], X)
            Xs.append(X)
        rank, Xg = d.probe(SHIFTS, Bs[0])
        g = ring.guess(SHIFTS, Bs[0])
        assert g["serials"] == [3, 4, 5] and rank == 48
        _check_guess(Xg, g, "ring of three, evicted right-hand side")
        assert min(sm.rel(Xg[k], Xs[0][k]) for k in range(3)) > 0.5
        _check_solution(big, SHIFTS, Bs[4], Xs[4], "ring of three, fifth solve")


def test_mixed_widths(small):
    """Widths 16, 5, 16: the third call's guess combines 21 columns pair by pair; three more 16-column calls later the
    side-by-side panel (rebuilt at the width change, the 5-column entry evicted) is back and agrees with the model."""
    rng = np.random.default_rng(101)
    ring = sm.RecycleRing(3)
    with Dev(small) as d:
        d.ctx.set_recycle(3)
        seen = []
        for k, w in enumerate((16, 5, 16, 16, 16, 16, 16)):
            B = rng.standard_normal((small.NV, w))
            if k:
                rank, Xg = d.probe(SHIFTS, B)
                t = d.trace()
                g = ring.guess(SHIFTS, B)
                seen.append((t["guess_cols"], t["guess_pan"]))
                assert t["guess_cols"] == g["cols"] == rank
                _check_guess(Xg, g, "widths 16 5 16 ..., call %d" % (k + 1))
            its, rr, X = d.solve(SHIFTS, B)
            assert rr.max() <= TOL
            ring.store(SHIFTS, B, X)
        print("[solve branches] mixed widths (columns, panel path) before calls 2 ..:", seen)
        assert seen[1] == (21, 0), seen            # before the third call
        assert seen[-1] == (48, 1) and seen[-2] == (48, 1), seen


def test_stored_right_hand_side_comes_back(small):
    """b equal to a stored right-hand side: the guess is that stored solution, and the solve that follows has nothing
    to do."""
    rng = np.random.default_rng(102)
    Bs = [rng.standard_normal((small.NV, 16)) for _ in range(2)]
    ring = sm.RecycleRing(3)
    with Dev(small) as d:
        d.ctx.set_recycle(3)
        Xs = []
        for B in Bs:
            Xs.append(d.solve(SHIFTS, B)[2])
            ring.store(SHIFTS, B, Xs[-1])
        rank, Xg = d.probe(SHIFTS, Bs[0])
        assert rank == 32
        allow, _ = sm.guess_allowance(np.hstack(Bs))
        worst = max(sm.rel(Xg[g], Xs[0][g]) for g in range(3))
        _ratio("guess", worst / allow)
        assert worst <= allow, (worst, allow)
        its, rr, X = d.solve(SHIFTS, Bs[0])
        assert its == [0, 0, 0] and rr.max() <= TOL, (its, rr.max())
        assert max(sm.rel(X[g], Xs[0][g]) for g in range(3)) <= allow


def test_rank_deficient_ring(small):
    """A right-hand side stored twice: the Gram matrix is rank deficient, the guess still is the model's x (basic and
    minimum-norm coefficients differ; the two stored solutions agree to the solve tolerance, so x agrees to that)."""
    rng = np.random.default_rng(103)
    B = rng.standard_normal((small.NV, 16))
    ring = sm.RecycleRing(3)
    with Dev(small) as d:
        d.ctx.set_recycle(3)
        for _ in range(2):
            ring.store(SHIFTS, B, d.solve(SHIFTS, B)[2])
        rank, Xg = d.probe(SHIFTS, B)
        t = d.trace()
        print("[solve branches] right-hand side stored twice: rank %d of %d columns" % (rank, t["guess_cols"]))
        assert t["guess_cols"] == 32 and 0 < t["guess_rank"] < 32 and rank == t["guess_rank"], t
        g = ring.guess(SHIFTS, B)
        worst = max(sm.rel(Xg[k], g["X"][k]) for k in range(3))
        _ratio("guess_rank_deficient", worst / sm.LU_TOL)
        assert worst <= sm.LU_TOL, worst


def test_unknown_shift_subset_and_other_callers(small, monkeypatch):
    """Who gets a guess: not a batch with a shift no earlier call contained (the buffer stays NaN), a subset of the
    earlier shifts does; per-group right-hand sides and a low-rank term inside the Krylov operator neither try nor
    store.  The Woodbury route solves with the plain operator and does recycle (the ADI sweeps of a Newton step)."""
    rng = np.random.default_rng(104)
    Bs = [rng.standard_normal((small.NV, 16)) for _ in range(4)]
    ring = sm.RecycleRing(3)
    with Dev(small) as d:
        d.ctx.set_recycle(3)
        for B in Bs[:2]:
            ring.store(SHIFTS, B, d.solve(SHIFTS, B)[2])
        ps = (-1.0, -7.0, -30.0)
        rank, Xg = d.probe(ps, Bs[2])
        assert rank == 0 and np.isnan(Xg).all()
        t0 = d.trace()
        its, rr, X = d.solve(ps, Bs[2])
        dt = _diff(d.trace(), t0)
        assert dt["guess_tried"] == 1 and dt["guess_used"] == 0 and rr.max() <= TOL, dt
        ring.store(ps, Bs[2], X)
        # a subset of the first shifts, one group
        rank, Xg = d.probe((-30.0,), Bs[3])
        g = ring.guess((-30.0,), Bs[3])
        assert rank == g["cols"] == 48
        _check_guess(Xg, g, "one group of the earlier shifts")
        t0 = d.trace()
        its, rr, X = d.solve((-30.0,), Bs[3])
        assert _diff(d.trace(), t0)["guess_used"] == 1
        _check_solution(small, (-30.0,), Bs[3], X, "one group, recycled guess")
        # per-group right-hand sides
        t0 = d.trace()
        Bg = rng.standard_normal((3, small.NV, 16))
        its, rr, X = d.solve(SHIFTS, Bg)
        dt = _diff(d.trace(), t0)
        assert dt["guess_tried"] == 0 and dt["stored"] == 0 and dt["solves"] == 1, dt
        _check_solution(small, SHIFTS, Bg, X, "per-group right-hand sides")
        # shared, low-rank term through Woodbury: plain-operator solves of [b, U] (19 columns), recycled as such
        U = 0.1 * rng.standard_normal((small.NV, 3))
        V = 0.1 * rng.standard_normal((small.NV, 3))
        d.ctx.set_lowrank(U, V)
        t0 = d.trace()
        its, rr, X = d.solve(SHIFTS, Bs[3])
        dt = _diff(d.trace(), t0)
        assert dt["smw_setups"] == 1 and dt["guess_tried"] == 1 and dt["stored"] == 1, dt
        _check_solution(small, SHIFTS, Bs[3], X, "Woodbury with recycling", lowrank=(U, V), family="smw")
    # shared, low-rank term inside the operator
    monkeypatch.setenv("RICADI_SMW", "0")
    with Dev(small) as d:
        d.ctx.set_recycle(3)
        d.ctx.set_lowrank(U, V)
        t0 = d.trace()
        for B in Bs[:2]:
            its, rr, X = d.solve(SHIFTS, B)
        dt = _diff(d.trace(), t0)
        assert dt["guess_tried"] == 0 and dt["stored"] == 0 and dt["inop_lowrank"] == 2, dt
    monkeypatch.delenv("RICADI_SMW")


def test_new_operator_and_cleared_cache_forget(small):
    rng = np.random.default_rng(105)
    B = rng.standard_normal((small.NV, 16))
    with Dev(small) as d:
        d.ctx.set_recycle(3)
        d.solve(SHIFTS, B)
        assert d.probe(SHIFTS, B)[0] == 16
        d.ctx.set_operator(small.calA, small.calE, small.J)
        rank, Xg = d.probe(SHIFTS, B)
        assert rank == 0 and np.isnan(Xg).all()
        d.solve(SHIFTS, B)
        assert d.probe(SHIFTS, B)[0] == 16
        d.ctx.clear_cache()
        rank, Xg = d.probe(SHIFTS, B)
        assert rank == 0 and np.isnan(Xg).all()
        its, rr, X = d.solve(SHIFTS, B)
        assert min(its) > 0
        _check_solution(small, SHIFTS, B, X, "after clear_cache")
        assert d.probe(SHIFTS, B)[0] == 16


def test_depth_in_force_drops(small):
    """Five right-hand sides at depth 5, then depth 3 (an ADI followed by direct calls): the guess combines the
    last three right-hand sides, as ricadi_set_recycle documents, and keeps doing so while the ring turns over."""
    rng = np.random.default_rng(106)
    ring = sm.RecycleRing(5)
    with Dev(small) as d:
        d.ctx.set_recycle(5)
        for _ in range(5):
            B = rng.standard_normal((small.NV, 16))
            ring.store(SHIFTS, B, d.solve(SHIFTS, B)[2])
        d.ctx.set_recycle(3)
        ring.set_depth(3)
        for k in range(3):
            B = rng.standard_normal((small.NV, 16))
            rank, Xg = d.probe(SHIFTS, B)
            g = ring.guess(SHIFTS, B)
            assert rank == g["cols"] == 48, (k, rank)
            _check_guess(Xg, g, "depth 5 -> 3, call %d" % (k + 1))
            its, rr, X = d.solve(SHIFTS, B)
            assert rr.max() <= TOL
            ring.store(SHIFTS, B, X)


def test_wide_panel_with_guess(small):
    """m = 40: three column groups per shift, the last padded; with the second right-hand side equal to the first the
    guess is scattered into the groups and the solve has nothing to do."""
    rng = np.random.default_rng(107)
    B = rng.standard_normal((small.NV, 40))
    with Dev(small) as d:
        d.ctx.set_recycle(2)
        t0 = d.trace()
        its1, rr1, X1 = d.solve(SHIFTS, B)
        t1 = d.trace()
        its2, rr2, X2 = d.solve(SHIFTS, B)
        t2 = d.trace()
        assert _diff(t1, t0)["wide_passes"] == 1 and _diff(t2, t1)["wide_passes"] == 1
        assert t2["wide_groups_last"] == 9 and _diff(t2, t1)["wide_chunks"] == 1, t2
        assert _diff(t2, t1)["guess_used"] == 1 and t2["guess_cols"] == 40
        assert min(its1) > 0 and its2 == [0, 0, 0], (its1, its2)
        assert rr2.max() <= TOL
        allow, _ = sm.guess_allowance(B)
        worst = max(sm.rel(X2[g], X1[g]) for g in range(3))
        _ratio("guess", worst / allow)
        assert worst <= allow, (worst, allow)
        _check_solution(small, SHIFTS, B, X2, "wide panel, second solve")


def test_zero_column_and_zero_panel(small):
    rng = np.random.default_rng(108)
    Bs = [rng.standard_normal((small.NV, 16)) for _ in range(2)]
    for B in Bs:
        B[:, 3] = 0.0
    Z = np.zeros((small.NV, 16))
    with Dev(small) as d:
        its, rr, X = d.solve(SHIFTS, Z)                      # no recycling: from x = 0
        assert its == [0, 0, 0] and np.all(rr == 0.0) and np.all(X == 0.0)
        d.ctx.set_recycle(3)
        its, rr, X = d.solve(SHIFTS, Bs[0])
        assert np.all(X[:, :, 3] == 0.0) and np.all(rr[:, 3] == 0.0) and rr.max() <= TOL
        rank, Xg = d.probe(SHIFTS, Bs[1])
        assert rank > 0 and np.all(Xg[:, :, 3] == 0.0) and np.isfinite(Xg).all()
        its, rr, X = d.solve(SHIFTS, Bs[1])
        assert np.all(X[:, :, 3] == 0.0) and np.all(rr[:, 3] == 0.0)
        _check_solution(small, SHIFTS, Bs[1], X, "zero column")
        rank, Xg = d.probe(SHIFTS, Z)                        # the guess for b = 0 from a live ring
        assert np.all(Xg == 0.0)
        its, rr, X = d.solve(SHIFTS, Z)
        assert its == [0, 0, 0] and np.all(rr == 0.0) and np.all(X == 0.0)


# ------------------------------------------------------------------------------------------------- Woodbury
def _term_size(op, ps, B, lowrank):
    """max over shifts and columns of ||U V^T x_j|| / ||b_j|| for the closed-loop solutions x: what the Woodbury
    correction multiplies the error of the stored S^-1 U by, relative to the right-hand side."""
    U, V = lowrank
    worst = 0.0
    for g, p in enumerate(ps):
        S, lu = sm.closed_loop(op.calA, op.calE, op.J, p, 1.0, U, V)
        Bg = B if B.ndim == 2 else B[g]
        x = sm.lu_solve(S, lu, Bg)
        worst = max(worst, (np.linalg.norm(U @ (V.T @ x[:op.NV]), axis=0) / np.linalg.norm(Bg, axis=0)).max())
    return worst


@pytest.mark.parametrize("shared", [True, False], ids=["shared", "per_group"])
@pytest.mark.parametrize("q", [1, 3, 8])
def test_woodbury_cache(big, q, shared, monkeypatch):
    """U, V = 0.1 randn.  First call: W is set up (augmented panels [b, U], one for all groups or one per group);
    second call: the cache serves; after set_lowrank with another V: set up again, and the solutions are the new
    closed loop's.

    Measured on the MI355X: the closed-loop refinement runs in every one of these calls.  That is the design, not a
    defect of W: S^-1 U is known to gmres_tol relative to ||U||, and the correction multiplies that error by V^T x, so
    the closed-loop residual is  tol (1 + ||U V^T x|| / ||b||)  at best -- and at NV = 1682 a term of 0.1 randn has
    ||U V^T x|| / ||b|| between 3 and 26 (printed below).  A wrong W would leave a residual of order one, and refining
    that is solving the closed-loop system from zero; so in the cached calls the refinement's iterations (the total
    minus those of the same solve without the term) are held below those of that solve from zero, the same GMRES
    with the term inside the operator (RICADI_SMW=0), per group.  (Measured: 6 - 21 of 42 - 127 at q = 1 and 3, 23 - 71
    of 82 - 228 at q = 8.)  ``test_woodbury_weak_term`` is the case without refinement."""
    rng = np.random.default_rng(110 + q)
    U = 0.1 * rng.standard_normal((big.NV, q))
    V = 0.1 * rng.standard_normal((big.NV, q))
    V2 = 0.1 * rng.standard_normal((big.NV, q))
    shape = (big.NV, 16) if shared else (3, big.NV, 16)
    B1, B2 = rng.standard_normal(shape), rng.standard_normal(shape)
    tag = "Woodbury q=%d %s" % (q, "shared" if shared else "per group")
    with Dev(big) as d:
        plain = [d.solve(SHIFTS, B)[0] for B in (B1, B2)]
        d.ctx.set_lowrank(U, V)
        t0 = d.trace()
        its1, rr, X = d.solve(SHIFTS, B1)
        dt = _diff(d.trace(), t0)
        assert [dt[k] for k in ("solves", "smw_solves", "smw_setups", "smw_dup", "smw_bad", "inop_lowrank")] == \
            [1, 1, 1, 0, 0, 0], dt
        refined = [dt["smw_refined"]]
        assert rr.max() <= TOL
        _check_solution(big, SHIFTS, B1, X, tag + ", first", lowrank=(U, V), family="smw")
        t0 = d.trace()
        its2, rr, Xold = d.solve(SHIFTS, B2)
        dt = _diff(d.trace(), t0)
        assert (dt["smw_solves"], dt["smw_setups"], dt["smw_bad"]) == (1, 0, 0), dt
        refined.append(dt["smw_refined"])
        _check_solution(big, SHIFTS, B2, Xold, tag + ", cached", lowrank=(U, V), family="smw")
        d.ctx.set_lowrank(U, V2)
        t0 = d.trace()
        its3, rr, X = d.solve(SHIFTS, B2)
        dt = _diff(d.trace(), t0)
        assert (dt["smw_solves"], dt["smw_setups"], dt["smw_bad"]) == (1, 1, 0), dt
        refined.append(dt["smw_refined"])
        _check_solution(big, SHIFTS, B2, X, tag + ", new V", lowrank=(U, V2), family="smw")
        assert min(sm.rel(X[g], Xold[g]) for g in range(3)) > 1e4 * sm.LU_TOL
        t0 = d.trace()
        its4, rr, X = d.solve(SHIFTS, B1)
        dt = _diff(d.trace(), t0)
        assert (dt["smw_solves"], dt["smw_setups"], dt["smw_bad"]) == (1, 0, 0), dt
        refined.append(dt["smw_refined"])
        _check_solution(big, SHIFTS, B1, X, tag + ", new V cached", lowrank=(U, V2), family="smw")
    print("[solve branches] %s: ||U V^T x|| / ||b|| = %.3g; refined %s; iterations plain %s, with the term %s" %
          (tag, _term_size(big, SHIFTS, B2, (U, V)), refined, plain, [its1, its2, its3, its4]))
    NOTES.setdefault("Woodbury 0.1 randn, calls refined of 4", []).append(sum(refined))
    # from zero with the term inside the operator
    monkeypatch.setenv("RICADI_SMW", "0")
    with Dev(big) as d:
        d.ctx.set_lowrank(U, V)
        inop2 = d.solve(SHIFTS, B2)[0]
        d.ctx.set_lowrank(U, V2)
        inop4 = d.solve(SHIFTS, B1)[0]
    monkeypatch.delenv("RICADI_SMW")
    # the cached calls run the very plain solve of `plain` (same panels, same kernels), then the refinement
    for base, its, full in ((plain[1], its2, inop2), (plain[0], its4, inop4)):
        extra = [i - b for i, b in zip(its, base)]
        print("[solve branches] %s: refinement iterations %s, from zero inside the operator %s" % (tag, extra, full))
        _ratio("smw_refinement_iterations", max(e / f for e, f in zip(extra, full)))
        assert all(0 <= e < f for e, f in zip(extra, full)), (base, its, full)


def test_woodbury_weak_term(big):
    """A low-rank term that is small against the right-hand side (U, V = 1e-3 randn: ||U V^T x|| / ||b|| of order
    1e-2): setup, cached call and a new V all end without refinement -- a stale or wrong W would leave a closed-loop
    residual of that order, 1e8 times the tolerance, and be refined."""
    rng = np.random.default_rng(119)
    U = 1e-3 * rng.standard_normal((big.NV, 3))
    V = 1e-3 * rng.standard_normal((big.NV, 3))
    V2 = 1e-3 * rng.standard_normal((big.NV, 3))
    B1, B2 = rng.standard_normal((big.NV, 16)), rng.standard_normal((big.NV, 16))
    size = _term_size(big, SHIFTS, B2, (U, V))
    print("[solve branches] weak term: ||U V^T x|| / ||b|| = %.3g" % size)
    assert 1e-4 < size < 0.1
    with Dev(big) as d:
        d.ctx.set_lowrank(U, V)
        for k, (B, lr, setups) in enumerate(((B1, (U, V), 1), (B2, (U, V), 0), (B2, (U, V2), 1))):
            if k == 2:
                d.ctx.set_lowrank(U, V2)
            t0 = d.trace()
            its, rr, X = d.solve(SHIFTS, B)
            dt = _diff(d.trace(), t0)
            assert (dt["smw_solves"], dt["smw_setups"], dt["smw_refined"], dt["smw_bad"]) == (1, setups, 0, 0), (k, dt)
            assert rr.max() <= TOL
            _check_solution(big, SHIFTS, B, X, "weak term, call %d" % (k + 1), lowrank=lr, family="smw")


def test_woodbury_width_limit(small):
    """m + q = 128 takes the Woodbury route (augmented panels of 128 columns); m = 128 with q = 3 cannot and keeps
    the term inside the Krylov operator."""
    rng = np.random.default_rng(120)
    U = 0.1 * rng.standard_normal((small.NV, 3))
    V = 0.1 * rng.standard_normal((small.NV, 3))
    with Dev(small) as d:
        d.ctx.set_lowrank(U, V)
        for m, smw in ((125, 1), (128, 0)):
            B = rng.standard_normal((small.NV, m))
            t0 = d.trace()
            its, rr, X = d.solve(SHIFTS, B)
            dt = _diff(d.trace(), t0)
            assert (dt["smw_solves"], dt["smw_setups"], dt["inop_lowrank"]) == (smw, smw, 1 - smw), (m, dt)
            assert rr.max() <= TOL
            _check_solution(small, SHIFTS, B, X, "width limit m=%d" % m, lowrank=(U, V),
                            family="smw" if smw else "inop")


def test_lowrank_inside_the_operator(small, monkeypatch):
    rng = np.random.default_rng(121)
    U = 0.1 * rng.standard_normal((small.NV, 3))
    V = 0.1 * rng.standard_normal((small.NV, 3))
    B = rng.standard_normal((small.NV, 16))
    monkeypatch.setenv("RICADI_SMW", "0")
    with Dev(small) as d:
        d.ctx.set_lowrank(U, V)
        t0 = d.trace()
        its, rr, X = d.solve(SHIFTS, B)
        dt = _diff(d.trace(), t0)
        assert (dt["inop_lowrank"], dt["smw_solves"], dt["smw_setups"]) == (1, 0, 0), dt
        _check_solution(small, SHIFTS, B, X, "RICADI_SMW=0", lowrank=(U, V), family="inop")
    monkeypatch.delenv("RICADI_SMW")


def test_woodbury_refinement(big):
    """Capacitance matrix delta I (U2 = U T, T = (V^T S^-1 U)^-1 (1 - delta) from the plain LU): the Woodbury
    correction amplifies the solves' errors by 1 / delta, the verification pass sees it and one GMRES on the
    closed-loop operator repairs it.  Loose tolerance 1e-8: the closed-loop LU's own residual grows as 1 / delta and
    must stay a factor 100 below the tolerance.  Every run ends converged; the refinement must have run in one."""
    tol, p, q = 1e-8, -30.0, 3
    rng = np.random.default_rng(130)
    U = 0.1 * rng.standard_normal((big.NV, q))
    V = 0.1 * rng.standard_normal((big.NV, q))
    B = rng.standard_normal((big.NV, 16))
    S0, lu0 = big.plain(p)
    Zu = lu0.solve(sm.pad(U, big.n))
    reached = []
    for delta in (1e-1, 1e-2, 1e-3, 1e-4, 1e-5):
        if delta < 1e-3 and reached:
            break
        U2 = U @ (np.linalg.inv(V.T @ Zu[:big.NV]) * (1.0 - delta))
        S, lu = sm.closed_loop(big.calA, big.calE, big.J, p, 1.0, U2, V)
        if delta < 1e-3 and sm.relres(S, sm.lu_solve(S, lu, B), B).max() > tol / 100:
            break                                      # no room left for a reference
        with Dev(big, gmres_tol=tol) as d:
            d.ctx.set_lowrank(U2, V)
            t0 = d.trace()
            its, rr, X = d.solve((p,), B)
            dt = _diff(d.trace(), t0)
        print("[solve branches] refinement delta=%g: refined %d, bad %d, iterations %s, reported %.3g" %
              (delta, dt["smw_refined"], dt["smw_bad"], its, rr.max()))
        assert rr.max() <= tol * 1.0000001
        _check_solution(big, (p,), B, X, "refinement delta=%g" % delta, tol=tol, lowrank=(U2, V), family="smw_refined")
        if dt["smw_refined"]:
            reached.append(delta)
    NOTES["refinement reached at delta"] = reached
    assert reached, "the closed-loop refinement never ran"


def test_newton_step_takes_u_from_the_right_hand_side(cfg1):
    """Without mtxoldb the second Newton step's first sweep has U = K_k among its right-hand side's columns: no
    augmented columns (smw_dup)."""
    pr, tb, trct, ms = cfg1
    d = dict(pb.default_nwtn_adi_dict(), ms=ms, nwtn_max_steps=2, sweep_width=8)
    with _lib.Context(0) as ctx:
        ctx.set_operator((-pr.A - pr.Nc).T.tocsr(), pr.M.T.tocsr(), pr.J)
        Z, info = ctx.ric_newtonadi(ms, tb.toarray(), trct, _lib.adi_params(d))
        t = ctx.solve_trace()
        SEEN.update(k for k, v in t.items() if v > 0)
    print("[solve branches] Newton, two steps:", {k: v for k, v in t.items() if v})
    assert info["gmres_nonconverged"] == 0
    assert t["smw_dup"] >= 1 and t["smw_setups"] >= t["smw_dup"] and t["guess_used"] >= 1, t


# ---------------------------------------------------------------- escalation, non-convergence, cycle lengths
def test_escalation_leaves_the_other_groups_alone(hard):
    """[-1000, -1] on the hard operator with gmres_maxit = 200: the easy group converges at the default storage, the
    hard one is continued with wider storage; the easy group's panel is bitwise what the same call leaves with
    gmres_maxit at its default."""
    ps = (-1000.0, -1.0)
    B = np.random.default_rng(140).standard_normal((hard.NV, 16))
    with Dev(hard, gmres_maxit=200) as d:
        t0 = d.trace()
        its, rr, X = d.solve(ps, B)
        dt = _diff(d.trace(), t0)
    with Dev(hard) as d:
        its0, rr0, X0 = d.solve(ps, B)
        dt0 = d.trace()
    print("[solve branches] escalation: iterations %s (gmres_maxit 200), %s (default); groups continued %d + %d" %
          (its, its0, dt["esc1_groups"], dt["esc2_groups"]))
    NOTES["escalation iterations (maxit 200 / default)"] = (its, its0)
    print("[solve branches] escalation: stalled %d, at gmres_maxit %d (gmres_maxit 200); %d, %d, continued %d + %d "
          "(default)" % (dt["stalled_groups"], dt["maxit_groups"], dt0["stalled_groups"], dt0["maxit_groups"],
                         dt0["esc1_groups"], dt0["esc2_groups"]))
    assert dt["esc1_groups"] + dt["esc2_groups"] >= 1 and dt["maxit_groups"] >= 1, dt
    assert its[0] <= 200 < its[1], its
    assert rr.max() <= TOL and rr0.max() <= TOL
    _check_solution(hard, ps, B, X, "escalation")
    assert dt0["esc1_groups"] + dt0["esc2_groups"] == 0 and its0[0] == its[0], (dt0, its0)
    assert np.array_equal(X[0], X0[0]), np.abs(X[0] - X0[0]).max()


def test_seven_iterations_per_storage_level(big):
    """gmres_maxit = 7: a group that does not converge has run exactly 7 iterations at each of the three storage
    levels, the reported residuals (of order 1e-2) are those of the returned X."""
    B = np.random.default_rng(141).standard_normal((big.NV, 16))
    with Dev(big, gmres_maxit=7) as d:
        t0 = d.trace()
        its, rr, X = d.solve(SHIFTS, B, strict=False)
        dt = _diff(d.trace(), t0)
    print("[solve branches] gmres_maxit 7: iterations %s, worst reported residual %s" % (its, rr.max(axis=1)))
    print("[solve branches] gmres_maxit 7: groups at gmres_maxit %d, continued %d + %d" %
          (dt["maxit_groups"], dt["esc1_groups"], dt["esc2_groups"]))
    assert np.isfinite(X).all()
    unconverged = [g for g in range(3) if rr[g].max() > TOL]
    assert unconverged and all(its[g] == 21 for g in unconverged), its
    assert dt["maxit_groups"] >= 3 * len(unconverged) and dt["esc1_groups"] >= len(unconverged) \
        and dt["esc2_groups"] >= len(unconverged), dt
    for g, p in enumerate(SHIFTS):
        ref = sm.relres(big.plain(p)[0], X[g], B)
        dev = np.abs(rr[g] - ref) / ref
        _ratio("reported_residual", dev.max() / 1e-6)
        assert dev.max() <= 1e-6, (p, dev.max())


def test_cycle_lengths(big):
    B = np.random.default_rng(142).standard_normal((big.NV, 16))
    with Dev(big) as d:
        its, rr, X = d.solve(SHIFTS, B)
        t = d.trace()
    print("[solve branches] cycles: default restart %s iterations, %d cycles, longest %d" %
          (its, t["cycles"], t["cycle_len_max"]))
    assert t["cycle_len_max"] in (10, 15, 23, 30) and 0 < t["cycle_len_last"] <= t["cycle_len_max"], t
    assert t["cycles"] * t["cycle_len_max"] >= max(its)
    with Dev(big, gmres_restart=6) as d:
        its, rr, X = d.solve(SHIFTS, B)
        t = d.trace()
    print("[solve branches] cycles: restart 6 %s iterations, %d cycles" % (its, t["cycles"]))
    assert t["cycle_len_max"] == 6 and t["cycle_len_last"] == 6
    assert t["cycles"] >= math.ceil(max(its) / 6)
    assert rr.max() <= TOL
    _check_solution(big, SHIFTS, B, X, "restart 6")


def test_counters_reached():
    """Runs last in this file: every counter of the trace advanced in some case above.  smw_bad (capacitance matrix
    not inverted, or the plain solve unconverged) and stalled_groups (three full-length cycles without gain) need an
    operator that provokes them; they are listed, not asserted."""
    if not SEEN:
        pytest.skip("run with the rest of this file")
    exempt = {"smw_bad", "stalled_groups"}
    print("[solve branches] reached:", sorted(SEEN))
    print("[solve branches] not reached:", sorted(set(_lib.Context.TRACE) - SEEN))
    print("[solve branches] largest error / allowance:", {k: "%.3g" % v for k, v in sorted(RATIOS.items())})
    print("[solve branches] notes:", NOTES)
    assert set(_lib.Context.TRACE) - exempt <= SEEN, sorted(set(_lib.Context.TRACE) - exempt - SEEN)
