"""GPU tests of the one-reduction (delayed CGS2) Arnoldi of the lockstep GMRES's hot path (16-column panels, FP16
basis, FP32 operator output) against the three-pass CGS2 form it replaces (RICADI_ARNOLDI=cgs2, read when a context
is created).  Both forms solve the same cfg1 systems through the C-ABI; the sparse LU (SuperLU) is the reference and
the FP64 true residual the judge.
"""
import numpy as np
import pytest

from optconpy_amd import _lib
from oracle import lin_alg_utils as olau

pytestmark = pytest.mark.gpu
FORMS = ("lowsync", "cgs2")


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _solve(cfg1, monkeypatch, form, R, ps, **opts):
    import torch
    pr = cfg1[0]
    calA = (-pr.A - pr.Nc).T.tocsr()
    MT = pr.M.T.tocsr()
    if form == "cgs2":
        monkeypatch.setenv("RICADI_ARNOLDI", "cgs2")
    else:
        monkeypatch.delenv("RICADI_ARNOLDI", raising=False)
    m = R.shape[1]
    with _lib.Context(0, **opts) as ctx:
        ctx.set_operator(calA, MT, pr.J)
        Rd = torch.from_numpy(np.ascontiguousarray(R)).cuda()
        Xd = torch.empty((len(ps), pr.NV + pr.NP, m), dtype=torch.float64, device="cuda")
        its, rr = ctx.shift_solve_batch_dev(ps, [1.0] * len(ps), Rd.data_ptr(), 0, m, Xd.data_ptr())
        ctx.synchronize()
        X = Xd.cpu().numpy()
        w32 = ctx.setup_info()["fp32_operator_output"]
    monkeypatch.delenv("RICADI_ARNOLDI", raising=False)
    return np.asarray(its, dtype=float), np.asarray(rr), X, w32


def _check(cfg1, monkeypatch, R, ps, iter_slack=2, **opts):
    pr = cfg1[0]
    calA = (-pr.A - pr.Nc).T.tocsr()
    MT = pr.M.T.tocsr()
    out = {f: _solve(cfg1, monkeypatch, f, R, ps, **opts) for f in FORMS}
    for f in FORMS:
        its, rr, X, w32 = out[f]
        assert rr.max() <= 1e-10, (f, rr.max())
        for g, p in enumerate(ps):
            ref = olau.SaddleLU(calA + p * MT, pr.J).solve(R)
            assert rel(X[g][:pr.NV], ref[:pr.NV]) < 1e-8, (f, g)
    assert np.abs(out["lowsync"][0] - out["cgs2"][0]).max() <= iter_slack, (out["lowsync"][0], out["cgs2"][0])
    return out


def test_forms_agree_on_a_sixteen_column_panel(cfg1, monkeypatch):
    """Three shifts of a 16-column panel: the hot form is taken (FP32 operator output) and both Arnoldi forms meet
    the tolerance, match the sparse LU and need the same iterations within two."""
    rng = np.random.default_rng(16)
    R = rng.standard_normal((cfg1[0].NV, 16))
    out = _check(cfg1, monkeypatch, R, [-1.0, -40.0, -1500.0])
    assert out["lowsync"][3] == 1


def test_zero_column_stays_inert(cfg1, monkeypatch):
    """A zero right-hand side column is frozen from the first iteration: its solution stays exactly zero."""
    rng = np.random.default_rng(17)
    R = rng.standard_normal((cfg1[0].NV, 16))
    R[:, 7] = 0.0
    out = _check(cfg1, monkeypatch, R, [-3.0, -300.0])
    for f in FORMS:
        assert np.abs(out[f][2][:, :, 7]).max() == 0.0, f


def test_shifts_far_apart_leave_the_table_mid_cycle(cfg1, monkeypatch):
    """Shifts four decades apart converge at very different iteration counts: groups leave the lockstep table in
    the middle of a restart cycle, and the end-of-cycle pass completes their last column."""
    rng = np.random.default_rng(18)
    R = rng.standard_normal((cfg1[0].NV, 16))
    _check(cfg1, monkeypatch, R, [-0.5, -20.0, -800.0, -3e4])


def test_short_restart_cycles(cfg1, monkeypatch):
    """gmres_restart = 6 forces many restart cycles, each ending in the end-of-cycle pass."""
    rng = np.random.default_rng(19)
    R = rng.standard_normal((cfg1[0].NV, 16))
    _check(cfg1, monkeypatch, R, [-2.0, -200.0], iter_slack=4, gmres_restart=6)


def test_forty_column_panel_as_padded_groups(cfg1, monkeypatch):
    """A 40-column panel is solved as three 16-column groups per shift, the last one padded with zero columns."""
    rng = np.random.default_rng(40)
    R = rng.standard_normal((cfg1[0].NV, 40))
    _check(cfg1, monkeypatch, R, [-5.0, -90.0])


def test_timer_classes_of_both_forms(cfg1, monkeypatch):
    """Kernel-timer classes 5-7 (dots, update_dots, update) return a finite, positive time under both forms at the
    hot width (16) and a generic one (5)."""
    pr = cfg1[0]
    calA = (-pr.A - pr.Nc).T.tocsr()
    MT = pr.M.T.tocsr()
    ps = [-2.0, -30.0, -400.0]
    for form in FORMS:
        if form == "cgs2":
            monkeypatch.setenv("RICADI_ARNOLDI", "cgs2")
        else:
            monkeypatch.delenv("RICADI_ARNOLDI", raising=False)
        with _lib.Context(0) as ctx:
            ctx.set_operator(calA, MT, pr.J)
            for m in (16, 5):
                for nvec in (1, 3, 30):
                    for name in ("dots", "update_dots", "update"):
                        t = ctx.time_kernel_dev(name, ps, [1.0] * len(ps), m, nvec=nvec, reps=2)
                        assert np.isfinite(t) and t > 0.0, (form, name, m, nvec, t)
    monkeypatch.delenv("RICADI_ARNOLDI", raising=False)
