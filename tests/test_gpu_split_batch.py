"""GPU tests of the lockstep GMRES batch run as two half-batches on two streams (the default) against the same batch
on one stream (RICADI_SPLIT=0, read when a context is created).  Every kernel of the iteration sums a group in an
order that does not depend on which other groups share its launch, so the two must agree bit for bit: the same
iterations per group and the same solutions.
"""
import numpy as np
import pytest

from optconpy_amd import _lib, problems as pb

pytestmark = pytest.mark.gpu
FORMS = ("split", "one")


def _operator(pr):
    return (-pr.A - pr.Nc).T.tocsr(), pr.M.T.tocsr()


def _solve(pr, monkeypatch, form, R, ps, lowrank=None, env=(), **opts):
    import torch
    calA, MT = _operator(pr)
    for k, v in env:
        monkeypatch.setenv(k, v)
    if form == "one":
        monkeypatch.setenv("RICADI_SPLIT", "0")
    else:
        monkeypatch.delenv("RICADI_SPLIT", raising=False)
    m = R.shape[1]
    with _lib.Context(0, **opts) as ctx:
        ctx.set_operator(calA, MT, pr.J)
        if lowrank is not None:
            ctx.set_lowrank(*lowrank)
        Rd = torch.from_numpy(np.ascontiguousarray(R)).cuda()
        Xd = torch.empty((len(ps), pr.NV + pr.NP, m), dtype=torch.float64, device="cuda")
        its, rr = ctx.shift_solve_batch_dev(ps, [1.0] * len(ps), Rd.data_ptr(), 0, m, Xd.data_ptr())
        ctx.synchronize()
        X = Xd.cpu().numpy()
    monkeypatch.delenv("RICADI_SPLIT", raising=False)
    for k, _ in env:
        monkeypatch.delenv(k, raising=False)
    return list(its), np.asarray(rr), X


def _check(pr, monkeypatch, R, ps, bitwise=True, **kw):
    out = {f: _solve(pr, monkeypatch, f, R, ps, **kw) for f in FORMS}
    its_s, rr_s, X_s = out["split"]
    its_o, rr_o, X_o = out["one"]
    assert rr_s.max() <= 1e-10, rr_s.max()
    assert its_s == its_o, (its_s, its_o)
    if bitwise:
        assert np.array_equal(X_s, X_o), np.abs(X_s - X_o).max()
        assert np.array_equal(rr_s, rr_o)
    else:
        d = np.linalg.norm(X_s - X_o) / np.linalg.norm(X_o)
        assert d < 1e-8, d
    return out


@pytest.fixture(scope="module")
def cfg2_problem():
    return pb.ricc_problem(58, 0.05, NU=4, NY=4, alphau=1e-2)


def test_sixteen_groups_cfg1(cfg1, monkeypatch):
    """A full batch of 16 shifts at cfg1 size."""
    pr = cfg1[0]
    R = np.random.default_rng(1).standard_normal((pr.NV, 16))
    _check(pr, monkeypatch, R, list(pb.logshifts(1.0, 3e3, 16)))


def test_sixteen_groups_cfg2(cfg2_problem, monkeypatch):
    """A full batch of 16 shifts at cfg2 size (the benchmark's): the hot iteration form on both streams."""
    pr = cfg2_problem
    R = np.random.default_rng(2).standard_normal((pr.NV, 16))
    _check(pr, monkeypatch, R, list(pb.logshifts(1.0, 3e3, 16)))


@pytest.mark.parametrize("ps", [[-0.5, -3e4, -0.7, -4e4, -1.0, -5e4, -1.4, -6e4, -2.0, -7e4, -2.8, -8e4, -4.0, -9e4,
                                 -5.6, -1e5],
                                [-0.5, -3e4, -1.0, -5e4, -2.0, -8e4]])
def test_non_contiguous_active_groups(cfg1, monkeypatch, ps):
    """Large shifts converge early and leave the even group ids as the active ones: eight of sixteen (still two
    halves), and three of six (one stream)."""
    pr = cfg1[0]
    R = np.random.default_rng(3).standard_normal((pr.NV, 16))
    _check(pr, monkeypatch, R, ps)


def test_groups_leave_mid_cycle(cfg1, monkeypatch):
    """Shifts decades apart converge at very different iteration counts: groups leave the tables of both halves in
    the middle of a restart cycle, the second stream is joined back mid-cycle when fewer than eight are left, and
    short cycles (restart 6) end many times."""
    pr = cfg1[0]
    R = np.random.default_rng(4).standard_normal((pr.NV, 16))
    _check(pr, monkeypatch, R, [-0.5, -20.0, -800.0, -3e4, -7.0, -150.0, -1.5, -60.0, -2500.0, -9e3],
           gmres_restart=6)


def test_wide_panel(cfg1, monkeypatch):
    """A 40-column panel: three 16-column groups per shift (the last padded), nine groups split across the halves."""
    pr = cfg1[0]
    R = np.random.default_rng(5).standard_normal((pr.NV, 40))
    _check(pr, monkeypatch, R, [-5.0, -90.0, -1200.0])


@pytest.mark.parametrize("smw", ["1", "0"])
def test_lowrank(cfg1, monkeypatch, smw):
    """Operator with a low-rank term: through Sherman-Morrison-Woodbury (plain-operator GMRES, split) and with the
    term inside the Krylov operator (RICADI_SMW=0: one stream either way).  The iterations agree exactly, the solutions
    to rounding only: the coefficients V^T x (inside the operator with RICADI_SMW=0; of the correction x += W V^T x and
    the capacitance matrix otherwise) come from gemm_tn, which adds its partial tiles with FP64 atomics in an order that
    differs from run to run, split or not (measured: 6e-10 and 1.7e-7 at most in entries of size 40)."""
    pr = cfg1[0]
    rng = np.random.default_rng(6)
    U = 0.1 * rng.standard_normal((pr.NV, 3))
    V = 0.1 * rng.standard_normal((pr.NV, 3))
    R = rng.standard_normal((pr.NV, 16))
    _check(pr, monkeypatch, R, [-2.0, -60.0, -900.0, -4e3], bitwise=False, lowrank=(U, V),
           env=(("RICADI_SMW", smw),))


def test_one_group(cfg1, monkeypatch):
    """One shift: one stream either way."""
    pr = cfg1[0]
    R = np.random.default_rng(7).standard_normal((pr.NV, 16))
    _check(pr, monkeypatch, R, [-30.0])


def test_iteration_timer_classes(cfg1):
    """Timer classes iter / iter_split: finite, positive wall time per iteration for several group counts."""
    pr = cfg1[0]
    calA, MT = _operator(pr)
    ps = list(pb.logshifts(1.0, 3e3, 16))
    with _lib.Context(0) as ctx:
        ctx.set_operator(calA, MT, pr.J)
        for ng in (1, 2, 5, 16):
            for name in ("iter", "iter_split"):
                t = ctx.time_kernel_dev(name, ps[:ng], [1.0] * ng, 16, nvec=3, reps=3)
                assert np.isfinite(t) and t > 0.0, (name, ng, t)
