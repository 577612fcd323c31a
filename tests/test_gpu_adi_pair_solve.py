"""GPU tests of the complex solve of one pair entry, step by step (``struct PairSolve`` of
solver_adi_pairs.inl through ``ricadi_adi_pair_solve_dev``): the pack kernel bitwise, the Sherman-Morrison-Woodbury
correction against its float64 twin on the device's own uncorrected groups, the solution against the closed-loop LU,
the report, and the refinement branch on a ladder of nearly singular capacitance matrices.  Every check prints
``[pair solve] operator | check | measured | bound`` before it asserts.

tests/test_adi_pairs_cpu.py shows that the twin's bound holds a second float64 evaluation and is broken by every seeded
fault, and that the ladder makes the refinement due; tests/test_pair_smw_cpu.py holds the host arithmetic to NumPy.
"""
import numpy as np
import pytest
import scipy.sparse as sps

import adi_pairs_model as apm
import small_ops as so
from optconpy_amd import _lib
from test_adi_pairs_cpu import (KERNEL_P, LADDER_M, LADDER_OPS, LADDER_Q, LADDER_TOL, ladder_of,
                                ladder_rhs, model_of)

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
TOL = 1e-10                      # gmres_tol of the contexts here (the default, set explicitly)
OPS = ("unsym", "nv33_np1", "nv65_np24", "fe3")
WIDE_OPS = ("fe3", "unsym")
WIDE = 24                        # m + q from which a shape counts as wide
GUARD = 64                       # complex entries of NaN on either side of the packed groups
CTX = _lib.Context


def _say(name, check, value, bound):
    ok = bool(np.isfinite(value)) and value <= bound
    print("[pair solve] %s | %s | %.3e | %.3e%s" % (name, check, value, bound, "" if ok else "  MISS"))
    return ok


def _dev(a, dtype=np.float64):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A test that leaves the device in an error state ends the run: nothing more is started on it."""
    yield
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:            # pragma: no cover - only after a device fault
        pytest.exit("device error after a test, stopping: %r" % (e,), returncode=3)


def _context(op, tol=TOL):
    ctx = _lib.Context(0, **dict(op.opts, gmres_tol=tol))
    ctx.set_operator(*op.ops)
    return ctx


def _lowrank(nv, q, seed):
    rng = np.random.default_rng(seed)
    return 0.1 * rng.standard_normal((nv, q)), 0.1 * rng.standard_normal((nv, q))


def _probe(ctx, op, p, W, q, mask=7):
    """One call of the entry with NaN-filled outputs: (report, rhs (ng, nv, mc), raw, D, X (ng, n, mc each), the guard
    entries around the packed groups, W as it is on the device afterwards)."""
    m = W.shape[1]
    ng, mc = apm.groups(m + q)
    nan = np.nan + 1j * np.nan
    Wd = _dev(W)
    rhs = _dev(np.full(ng * op.nv * mc + 2 * GUARD, nan), np.complex128)
    raw = _dev(np.full((2, ng, op.n, mc), nan), np.complex128)
    X = _dev(np.full((ng, op.n, mc), nan), np.complex128)
    rep = ctx.adi_pair_solve_dev(p, Wd.data_ptr(), m, mask, raw.data_ptr(), X.data_ptr(),
                                 rhs.data_ptr() + 16 * GUARD)
    rhs, raw = _host(rhs), _host(raw)
    guards = np.concatenate([rhs[:GUARD], rhs[-GUARD:]])
    return rep, rhs[GUARD:-GUARD].reshape(ng, op.nv, mc), raw[0], raw[1], _host(X), guards, _host(Wd)


def _bits(a):
    return np.ascontiguousarray(a).view(np.float64)


def _closed_loop(op, p, U, V):
    mdl = apm.PairsModel(*op.ops, U=U, V=V)
    return mdl, mdl.saddle(mdl.A, p)


def _solution_checks(who, op, p, W, U, V, X, rep, tol, miss):
    """The final groups against the closed-loop LU and the report against the host's residual."""
    m, q = W.shape[1], 0 if U is None else U.shape[1]
    mdl, S = _closed_loop(op, p, U, V)
    rhs = np.zeros((op.n, m), dtype=complex)
    rhs[:op.nv] = W
    xref = mdl._solve(S, W)
    wn = np.linalg.norm(W, axis=0)
    live = wn > 0
    own = float(np.max(np.linalg.norm(S @ xref - rhs, axis=0)[live] / wn[live]))
    assert _say(who, "reference residual", own, tol / 100)
    x = apm.unpack(X, m)
    res = np.linalg.norm(S @ x - rhs, axis=0)
    rr = np.where(live, res / np.where(live, wn, 1.0), 0.0)
    bar = 1.1 * (10.0 if q else 1.0) * tol
    if not _say(who, "true residual", float(rr.max()), bar):
        miss.append((who, "residual", float(rr.max())))
    xn = np.linalg.norm(xref, axis=0)
    fwd = float(np.max(np.linalg.norm(x - xref, axis=0)[live] / xn[live]))
    if not _say(who, "forward error", fwd, 2.0 * np.linalg.cond(S) * bar):
        miss.append((who, "forward", fwd))
    # the report
    assert (rep["ng"], rep["mc"]) == apm.groups(m + q)
    assert rep["refined"] == (rep["worst_before"] > 10.0 * tol), rep
    assert rep["converged"] == (rep["worst_after"] <= 10.0 * tol), rep
    assert rep["iters"] >= 1 and (rep["refined"] or rep["worst_before"] == rep["worst_after"])
    nnz = int(np.count_nonzero(mdl.saddle(mdl.A0, p), axis=1).max())
    floor = 8.0 * EPS * (nnz + q + 2) * float(np.max(np.linalg.norm(np.abs(S) @ np.abs(x), axis=0)[live] / wn[live]))
    gap = abs(rep["worst_after"] - float(rr.max()))
    if not _say(who, "reported residual - host's", gap, 0.1 * float(rr.max()) + floor):
        miss.append((who, "reported", gap))
    assert np.isnan(rep["min_pivot_rel"]) if q == 0 else 0.0 < rep["min_pivot_rel"] <= 1.0
    return rr


def _twin_check(who, V, m, q, raw, X, miss, D=None, tag="correction / bound"):
    """dX against the twin on the device's own uncorrected groups; U's columns and the padding bitwise unchanged."""
    ng, n, mc = raw.shape
    twin = apm.woodbury_twin(raw, V, m, q, Draw=D)
    bound = apm.woodbury_bound(raw, V, m, q, Draw=D)
    wcols = bound > 0
    assert wcols.sum() == m * n
    ratio = float(np.max(np.abs(X - twin)[wcols] / bound[wcols]))
    if not _say(who, tag, ratio, 1.0):
        miss.append((who, tag, ratio))
    assert np.array_equal(_bits(X[~wcols]), _bits(raw[~wcols])), "a column of U or of the padding was changed"
    return ratio


def _shifts(name):
    op, mdl, ms = model_of(name, False)
    out = [KERNEL_P[0], KERNEL_P[1]]
    if ms and isinstance(ms[0], complex):
        out.append(ms[0])
    return out


CASES = [(name, m, q) for name in OPS for (m, q) in apm.PAIR_SOLVE_SHAPES if m + q < WIDE or name in WIDE_OPS]
CASES += [("nv1", m, q) for (m, q) in apm.PAIR_SOLVE_SHAPES if m <= 1]


@pytest.mark.parametrize("name,m,q", CASES)
def test_one_pair_solve_step_by_step(name, m, q):
    """Pack bitwise with NaN neighbours; with q > 0 the correction within ``woodbury_bound`` of the twin on the
    device's own ``dRaw`` over all n rows (wherever no refinement ran); the solution against the closed-loop LU --
    true residual at most ``1.1 * 10 tol`` (q > 0) or ``1.1 tol`` (q = 0), forward error within ``2 cond(S_cl)`` times
    that; the report."""
    op = so.get(name)
    rng = np.random.default_rng(1000 * m + q)
    W = rng.standard_normal((op.nv, m))
    U, V = _lowrank(op.nv, q, 50 + q) if q else (None, None)
    miss, worst = [], 0.0
    with _context(op) as ctx:
        if q:
            ctx.set_lowrank(U, V)
        for p in _shifts(name):
            who = "%s m %d q %d p %s" % (name, m, q, p)
            rep, rhs, raw, D, X, guards, Wback = _probe(ctx, op, p, W, q)
            print("[pair solve] %s | report %s" % (who, rep))
            assert np.array_equal(_bits(rhs), _bits(apm.pack(W, U))), "the packed groups differ"
            assert np.all(np.isnan(_bits(guards))), "the pack kernel wrote beside the groups"
            assert np.array_equal(Wback, W)
            assert np.all(np.isfinite(_bits(X)))
            if q:
                assert np.all(np.isfinite(_bits(raw)))
                assert rep["refined"] or np.all(np.isnan(_bits(D)))
                if not rep["refined"]:
                    worst = max(worst, _twin_check(who, V, m, q, raw, X, miss))
            else:
                assert np.all(np.isnan(_bits(raw))), "dRaw is written only with a low-rank term"
            _solution_checks(who, op, p, W, U, V, X, rep, TOL, miss)
            assert rep["converged"]
    print("[pair solve] %s m %d q %d | largest correction / bound over the shifts | %.3e | 1" % (name, m, q, worst))
    assert not miss, miss


@pytest.mark.parametrize("q", [0, 2])
def test_a_zero_column_of_w(q):
    """A zero column of W gives an exactly zero solution column over all n rows; its 0 / 0 is not a miss."""
    op = so.get("fe3")
    W = np.random.default_rng(9).standard_normal((op.nv, 3))
    W[:, 1] = 0.0
    U, V = _lowrank(op.nv, q, 52) if q else (None, None)
    miss = []
    with _context(op) as ctx:
        if q:
            ctx.set_lowrank(U, V)
        rep, rhs, raw, D, X, guards, _ = _probe(ctx, op, KERNEL_P[0], W, q)
    x = apm.unpack(X, 3)
    assert np.all(x[:, 1] == 0.0) and np.all(x[:, 0] != 0.0)
    assert rep["converged"] and np.isfinite(rep["worst_after"]) and not rep["refined"]
    _solution_checks("fe3 zero column q %d" % q, op, KERNEL_P[0], W, U, V, X, rep, TOL, miss)
    assert not miss, miss


@pytest.mark.parametrize("name", LADDER_OPS)
def test_the_refinement_branch(name):
    """The ladder of tests/adi_pairs_model.refinement_ladder at gmres_tol = 1e-8: converged and correct at every rung;
    at delta = 1e-3 the refinement ran, and the two-pass twin holds on the device's ``dRaw`` and the refinement's
    uncorrected ``D`` (an uncorrected add would be far outside)."""
    op, p, rungs = ladder_of(name)
    miss = []
    for delta, U2, V in rungs:
        for m in LADDER_M:
            W = ladder_rhs(op, m)
            who = "%s ladder delta %g m %d" % (name, delta, m)
            with _context(op, LADDER_TOL) as ctx:
                ctx.set_lowrank(U2, V)
                rep, rhs, raw, D, X, guards, _ = _probe(ctx, op, p, W, LADDER_Q)
            print("[pair solve] %s | refined %d worst_before %.3e worst_after %.3e iterations %d min pivot %.2e" %
                  (who, rep["refined"], rep["worst_before"], rep["worst_after"], rep["iters"], rep["min_pivot_rel"]))
            _solution_checks(who, op, p, W, U2, V, X, rep, LADDER_TOL, miss)
            assert rep["converged"], rep
            if rep["refined"]:
                assert np.all(np.isfinite(_bits(D)))
                ng, mc = apm.groups(m + LADDER_Q)
                ucols = [(j // mc, j % mc) for j in range(m, ng * mc)]
                assert all(np.all(D[g, :, cc] == 0.0) for g, cc in ucols), "U's columns of the refinement are not zero"
                _twin_check(who, V, m, LADDER_Q, raw, X, miss, D=D, tag="two-pass correction / bound")
                bad = apm.woodbury_twin(raw, V, m, LADDER_Q, fault="refine_raw", Draw=D)
                bound = apm.woodbury_bound(raw, V, m, LADDER_Q, Draw=D)
                assert np.max(np.abs(bad - X)[bound > 0] / bound[bound > 0]) > 1.0, "an uncorrected D would pass"
            else:
                _twin_check(who, V, m, LADDER_Q, raw, X, miss)
            if delta == 1e-3:
                assert rep["refined"], "the refinement did not run: worst_before %.3e" % rep["worst_before"]
    assert not miss, miss


def test_pack_alone_on_the_kernel_operators():
    """The pack kernel by itself (what_mask 1 + 8: no solve) on nv = 1, 2 and across workgroup edges, every shape of
    the table: bitwise ``apm.pack``, NaN neighbours untouched, the other outputs untouched."""
    for name in ("nv1", "nv2_np1", "nv31_np12", "arrow200"):
        op = so.get(name)
        with _context(op) as ctx:
            for m, q in apm.PAIR_SOLVE_SHAPES:
                W = np.random.default_rng(m + q).standard_normal((op.nv, m))
                U, V = _lowrank(op.nv, q, 3) if q else (None, None)
                ctx.set_lowrank(U, V)
                rep, rhs, raw, D, X, guards, Wback = _probe(ctx, op, -1 + 2j, W, q, mask=1 + 8)
                assert np.array_equal(_bits(rhs), _bits(apm.pack(W, U))), (name, m, q)
                assert np.all(np.isnan(_bits(guards))) and np.array_equal(Wback, W)
                assert np.all(np.isnan(_bits(raw))) and np.all(np.isnan(_bits(X)))
                assert (rep["ng"], rep["mc"], rep["iters"]) == apm.groups(m + q) + (0,)


def test_refusals_leave_the_outputs_untouched():
    op = so.get("fe3")
    W = np.random.default_rng(1).standard_normal((op.nv, 127))
    with _context(op) as ctx:
        for kw in (dict(p=1 + 1j), dict(p=-1 + 0j), dict(p=complex(-1, np.inf)), dict(m=0), dict(mask=16),
                   dict(m=127, q=2), dict(rhs_off=8)):
            a = dict(p=-1 + 1j, m=3, mask=7, q=0, rhs_off=0)
            a.update(kw)
            if a["q"]:
                ctx.set_lowrank(*_lowrank(op.nv, a["q"], 4))
            Wd = _dev(W)
            outs = [_dev(np.full(4 * 16 * op.n * 8, np.nan)) for _ in range(3)]
            with pytest.raises(ValueError, match="ricadi"):
                ctx.adi_pair_solve_dev(a["p"], Wd.data_ptr(), a["m"], a["mask"], outs[0].data_ptr(),
                                       outs[1].data_ptr(), outs[2].data_ptr() + a["rhs_off"])
            assert ctx.pair_solve_report is None
            assert all(np.all(np.isnan(_host(o))) for o in outs)
            ctx.set_lowrank(None, None)
        with pytest.raises(ValueError, match="ricadi"):
            ctx.adi_pair_solve_dev(-1 + 1j, None, 3, 0)
        rep = ctx.adi_pair_solve_dev(-1 + 1j, _dev(W[:, :3]).data_ptr(), 3, 0)  # no output asked for: report alone
        assert rep["converged"] and rep["worst_after"] <= TOL
    with CTX(0) as ctx:
        with pytest.raises(RuntimeError, match="operator"):
            ctx.adi_pair_solve_dev(-1 + 1j, _dev(W).data_ptr(), 3, 0)


def test_a_call_after_a_probe_call_is_a_fresh_contexts(monkeypatch):
    """``lyap_adi`` after a probe call returns bitwise what a fresh context returns -- a real list on a plain
    context, a pair list on a context with a low-rank term -- and ``adi_pair_info`` keeps the last ``lyap_adi`` call's
    values over a probe call (recycling off, as in
    test_gpu_adi_pairs.test_real_calls_around_a_pair_call_are_a_fresh_contexts)."""
    monkeypatch.setenv("RICADI_RECYCLE", "0")
    op, mdl, ms = model_of("fe3", True)
    prm = _lib.adi_params(dict(adi_max_steps=300, adi_newZ_reltol=1e-12))
    W9 = np.random.default_rng(4).standard_normal((op.nv, 9))
    for lst, lowrank in ((op.shifts, None), (ms, (-op.oldB, op.B))):
        q = 0 if lowrank is None else 2
        with _context(op) as ctx:
            ctx.set_recycle(0)
            if lowrank:
                ctx.set_lowrank(*lowrank)
            fresh = ctx.lyap_adi(lst, op.W, prm)
        with _context(op) as ctx:
            ctx.set_recycle(0)
            if lowrank:
                ctx.set_lowrank(*lowrank)
            _probe(ctx, op, ms[0], W9, q)
            Z, info = ctx.lyap_adi(lst, op.W, prm)
            assert np.array_equal(Z, fresh[0]) and info == fresh[1]
            before = ctx.adi_pair_info()
            _probe(ctx, op, KERNEL_P[2], W9, q)
            assert ctx.adi_pair_info() == before == info.get("pair_info", [0, 0, 0, 0])


def test_a_singular_capacitance_matrix_leaves_the_context_usable(monkeypatch):
    """The rotation block ``calA = -I_2, calE = I_2``, no constraints, ``U = [[-2, -2], [2, -2]]``, ``V = I_2`` at
    ``p = -1 - 2i``: ``cap = I - (calA + p calE)^-1 U`` is exactly singular in exact arithmetic.  Either outcome is
    taken -- the 'numerically singular' error or a report that is not converged --; a healthy call behind it succeeds
    and is bitwise a fresh context's."""
    monkeypatch.setenv("RICADI_RECYCLE", "0")
    ops = (sps.csr_matrix(-np.eye(2)), sps.csr_matrix(np.eye(2)), sps.csr_matrix((0, 2)))
    U, V = np.array([[-2.0, -2.0], [2.0, -2.0]]), np.eye(2)
    p = -1 - 2j
    cap = np.eye(2) - V.T @ np.linalg.solve(-np.eye(2) + p * np.eye(2), U)
    assert np.linalg.svd(cap, compute_uv=False)[-1] <= 4 * EPS
    W = np.array([[1.0], [0.5]])
    prm = _lib.adi_params(dict(adi_max_steps=6, adi_newZ_reltol=0.0))

    def healthy(ctx):
        ctx.set_lowrank(None, None)
        return ctx.lyap_adi([-1 + 2j], W, prm)

    with CTX(0, gmres_tol=TOL) as ctx:
        ctx.set_operator(*ops)
        ctx.set_recycle(0)
        fresh = healthy(ctx)
    with CTX(0, gmres_tol=TOL) as ctx:
        ctx.set_operator(*ops)
        ctx.set_recycle(0)
        ctx.set_lowrank(U, V)
        Wd = _dev(W)
        X = _dev(np.full((1, 2, 3), np.nan + 0j), np.complex128)
        try:
            rep = ctx.adi_pair_solve_dev(p, Wd.data_ptr(), 1, 4, None, X.data_ptr())
            outcome = "a report: converged %d, worst_after %.3e, min pivot %.3e" % (
                rep["converged"], rep["worst_after"], rep["min_pivot_rel"])
            assert not rep["converged"], rep
        except RuntimeError as e:
            assert "numerically singular" in str(e)
            rep = ctx.pair_solve_report
            assert rep is not None and (rep["ng"], rep["mc"]) == (1, 3) and rep["min_pivot_rel"] < 1e-13
            outcome = "the 'numerically singular' error, min pivot %.3e" % rep["min_pivot_rel"]
        print("[pair solve] rotation block | singular capacitance matrix | outcome: %s" % outcome)
        Z, info = healthy(ctx)
    assert np.array_equal(Z, fresh[0]) and info == fresh[1]
