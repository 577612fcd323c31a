"""The sweep form of RADI without a GPU: the NumPy model (tests/radi_sweep_model.py) against the
sequential model (tests/radi_model.radi), the library's host entries ``ricadi_host_radi_sweep`` /
``ricadi_host_radi_sweep_width`` against the model in longdouble, and the admissibility study behind
``RICADI_RADI_SWEEP_PIVOT``.  The model is the yardstick of tests/test_gpu_radi_sweep.py."""
import functools
import os
import re

import numpy as np
import pytest

import dense_model as dm
import radi_model as rm
import radi_sweep_model as swm
from optconpy_amd import _lib, problems as pb

U_HOST = dm.U_REF                   # the host entry computes in long double
GOLD = np.load(swm.golden_path())


@functools.lru_cache(maxsize=None)
def runs(N):
    """Per call form at mesh size N: (form, sequential run, {width: (sweep run, its recorded sweeps)}) at 1e-12.
    Shared by the tests: read-only."""
    out = []
    for f in swm.forms(N):
        seq = rm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], f["ms"], old=f["old"], res_reltol=1e-12)
        per = {}
        for w in swm.widths_of(f):
            rec = []
            per[w] = (swm.radi_sweeps(f["calA"], f["calE"], f["J"], f["B"], f["W"], f["ms"], w, old=f["old"],
                                      res_reltol=1e-12, record=rec), rec)
        out.append((f, seq, per))
    return out


# ------------------------------------------------------------------------------- 1. the model against radi_model.radi
@pytest.mark.parametrize("N", [4, 8])
def test_sweep_model_is_the_sequential_iteration(N):
    """Same step count, Z Z^T, gain and history entry by entry, for every power-of-two width the list allows (also
    widths the pivot rule would refuse: the solves are exact here).  The bars are ten times the deviations
    make_golden measured (1e-15 for Z Z^T and the gain, 1e-13 .. 2e-12 for the history)."""
    for f, seq, per in runs(N):
        assert sorted(per) == [w for w in (1, 2, 4, 8, 16) if w <= len(f["ms"])] and len(per) >= 4
        bar = 10.0 * GOLD["dev_%d_%s" % (N, f["name"])]
        for w, (swp, rec) in per.items():
            assert swp["steps"] == seq["steps"] and swp["stopped"] == seq["stopped"] == "res", (f["name"], w)
            assert len(swp["res_hist"]) == swp["steps"] and swp["Z"].shape == seq["Z"].shape
            assert swp["solves"] == sum(len(r[0]) for r in rec) and swp["sweeps"] == len(rec)
            assert swp["steps"] <= swp["solves"] <= swp["steps"] + w - 1
            dev = swm.compare_runs(seq, swp)
            print("N = %d %-8s width %2d: ZZ^T %.2e gain %.2e history %.2e" % ((N, f["name"], w) + dev))
            assert all(d <= b for d, b in zip(dev, bar)), (f["name"], w, dev, bar)
    assert runs(N)[1][0]["W"].shape[1] == 8 and np.linalg.matrix_rank(runs(N)[1][0]["W"]) == 4      # dre: rank 4
    assert runs(N)[2][0]["old"] is not None


def test_sweep_model_prefix_and_width_one():
    """The first j blocks of a sweep are j sequential steps (a run cut by max_steps inside a sweep), and width 1
    is the sequential step itself."""
    f = swm.forms(4)[0]
    a = (f["calA"], f["calE"], f["J"], f["B"], f["W"], f["ms"])
    seq = rm.radi(*a, max_steps=5, res_reltol=0.0)
    for w in (1, 8):
        swp = swm.radi_sweeps(*a, w, max_steps=5, res_reltol=0.0)
        assert swp["steps"] == 5 and swp["solves"] == 5
        assert max(swm.compare_runs(seq, swp)[:2]) < 1e-13


# ----------------------------------------------------------------------- 2. the host entry against sweep_data
def check_host(ps, Ghat, Gamma, m, nb, tol, rhs, left):
    k, res, Cf = swm.sweep_data(ps, Ghat, Gamma, m, nb, tol, rhs, left)
    hk, hres, hCf = _lib.host_radi_sweep(ps, m, nb, Ghat, Gamma, rhs, tol, left)
    assert hk == k and hres.shape == res.shape and hCf.shape == Cf.shape == (len(ps) * m, k * m + m + nb)
    Cf64 = np.asarray(Cf, dtype=float)
    rc = dm.ratio(hCf, Cf, swm.sweep_data_bounds(ps, Ghat, m, Cf64, U_HOST))
    assert rc <= 1.0, rc
    # the residual of every step from the model's Cf of that step
    worst = 0.0
    for j in range(1, k + 1):
        kj, rj, Cfj = (k, res, Cf) if j == k else swm.sweep_data(ps, Ghat, Gamma, m, nb, 0.0, rhs, j)
        assert kj == j and abs(rj[-1] - res[j - 1]) <= 1e-15 * res[j - 1] + 1e-300
        b = swm.sweep_res_bounds(ps, Ghat, Gamma, m, Cfj, j, res[j - 1], rhs, U_HOST)
        worst = max(worst, abs(hres[j - 1] - res[j - 1]) / b)
    assert worst <= 1.0, worst
    return k, rc, worst


def test_host_sweep_matches_the_longdouble_model():
    """(ps, Ghat, Gamma) of every sweep of every model run at N = 4 and N = 8, width 1 included."""
    n, worst = 0, (0.0, 0.0)
    for N in (4, 8):
        for f, _, per in runs(N):
            m, nb = f["W"].shape[1], f["B"].shape[1]
            for w, (_, rec) in per.items():
                for ps, Ghat, Gamma, rhs, left, k, _, _ in rec:
                    hk, rc, rr = check_host(ps, Ghat, Gamma, m, nb, 1e-12, rhs, left)
                    assert hk == k
                    worst = (max(worst[0], rc), max(worst[1], rr))
                    n += 1
    print("%d sweeps: Cf error / bound %.2e, residual error / bound %.2e" % ((n,) + worst))
    assert n == sum(len(rec) for N in (4, 8) for _, _, per in runs(N) for _, rec in per.values()) and n >= 250


def test_host_sweep_stop_cases_and_breakdown():
    f, _, per = runs(4)[0]
    m, nb = f["W"].shape[1], f["B"].shape[1]
    ps, Ghat, Gamma, rhs, left, k, res, _ = per[8][1][0]
    assert k == 8 and left > 8
    # stop by the residual inside the sweep: a tolerance between the residuals of steps 3 and 4
    assert res[3] < res[2]
    assert check_host(ps, Ghat, Gamma, m, nb, np.sqrt(res[2] * res[3]), rhs, left)[0] == 4
    # ... by the steps that are left
    assert check_host(ps, Ghat, Gamma, m, nb, 1e-12, rhs, 3)[0] == 3
    # one step: the sequential step's coefficients
    k1, r1, Cf1 = _lib.host_radi_sweep(ps[:1], m, nb, Ghat[:m], Gamma[:2 * m, :2 * m], rhs, 1e-12, 5)
    Y = np.eye(m) + Ghat[:m] @ Ghat[:m].T
    assert k1 == 1 and np.allclose(Cf1[:, m:2 * m], -2.0 * ps[0] * np.linalg.inv(Y), rtol=1e-13, atol=0)
    assert np.allclose(Cf1[:, :m] @ Cf1[:, :m].T, Cf1[:, m:2 * m], rtol=1e-13, atol=1e-300)
    bad = Ghat.copy()
    bad[3, 0] = np.nan
    with pytest.raises(RuntimeError):
        _lib.host_radi_sweep(ps, m, nb, bad, Gamma, rhs, 1e-12, left)
    with pytest.raises(ValueError):
        _lib.host_radi_sweep([-1.0, -1.0], m, nb, Ghat[:2 * m], Gamma[:3 * m, :3 * m], rhs, 1e-12, left)
    with pytest.raises(ValueError):
        _lib.host_radi_sweep(ps, m, nb, Ghat, Gamma, rhs, 1e-12, 0)


def test_host_sweep_at_the_widest_shape():
    """G m = 128: against the model, and the time of the long double arithmetic (printed)."""
    import time
    rng = np.random.default_rng(3)
    g, m, nb = 8, 16, 8
    ps = pb.logshifts(1.0, 1e3, 8)
    Ghat = rng.standard_normal((g * m, nb))
    P = rng.standard_normal((400, (g + 1) * m))
    Gamma = P.T @ P
    rhs = np.linalg.norm(Gamma[:m, :m])
    k, rc, rr = check_host(ps, Ghat, Gamma, m, nb, 0.0, rhs, 100)
    t0 = time.perf_counter()
    for _ in range(5):
        _lib.host_radi_sweep(ps, m, nb, Ghat, Gamma, rhs, 0.0, 100)
    print("G m = 128: k = %d, Cf error / bound %.2e, residual error / bound %.2e, %.2f ms per call" % (
        k, rc, rr, 1e3 * (time.perf_counter() - t0) / 5))
    assert k == 8


# ----------------------------------------------------------------------------------------- 3. the effective width
def test_host_sweep_width():
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "ricadi.h")).read()
    assert float(re.search(r"#define RICADI_RADI_SWEEP_PIVOT (\S+)", hdr).group(1)) == swm.PIVOT and abs(float(GOLD["pivot"]) - swm.PIVOT) < 1e-9 * swm.PIVOT
    wide = pb.logshifts(1.0, 1e4, 16)                       # 16 well separated shifts
    W = _lib.host_radi_sweep_width
    assert swm.cycle_pivot(wide, 16) >= swm.PIVOT
    assert W(wide, 2, 2, 16, 200) == 16 and W(wide, 2, 2, 8, 200) == 8 and W(wide, 2, 2, 1, 200) == 1
    assert W(wide[:5], 2, 2, 16, 200) == 5                  # ns
    assert W(wide, 16, 8, 16, 200) == 8 and W(wide, 17, 8, 16, 200) == 7 and W(wide, 65, 8, 16, 200) == 1   # 128 / mw
    assert W(wide, 58, 4, 16, 200) == 2 and W(wide, 30, 10, 16, 200) == 4 and W(wide, 22, 10, 16, 200) == 5   # 128 / mw
    # the column groups of the (mw + nb)-wide panel, where THEY decide: one group up to 32 columns, sixteen-column
    # groups above; G groups <= 16
    assert swm.panel_groups(20, 12) == 1 and swm.panel_groups(20, 13) == 3 and swm.panel_groups(17, 64) == 6
    assert W(wide, 20, 12, 16, 200) == 6                    # 32 columns: one group, 128 / 20 = 6 decides
    assert W(wide, 20, 13, 16, 200) == 5                    # 33 columns: three groups, 16 / 3 = 5 < 6
    assert W(wide, 20, 20, 16, 200) == 5                    # 40 columns: three groups
    assert W(wide, 17, 64, 16, 200) == 2                    # 81 columns: six groups, 16 / 6 = 2 < 128 / 17 = 7
    assert W(wide, 8, 8, 16, 200) == 16 and W(wide, 8, 25, 16, 200) == 5        # 16 columns: one group; 33: three
    assert W(wide, 2, 47, 16, 200) == 4 and W(wide, 2, 48, 16, 200) == 4 and W(wide, 2, 63, 16, 200) == 3   # 49, 50: four; 65: five
    assert W(wide, 2, 2, 16, 3) == 3                        # max_steps
    assert W([-1.0, -2.0, -1.0, -3.0], 2, 2, 4, 200) == 2 and W([-1.0, -1.0, -2.0, -2.0], 2, 2, 4, 200) == 1
    assert W([-2.0], 2, 2, 4, 200) == 1
    for args in ((wide, 2, 2, 0, 200), (wide, 2, 2, 17, 200), (wide, 2, 2, 4, 0), ([1.0, -1.0], 2, 2, 2, 200),
                 (wide, 100, 64, 2, 200)):
        with pytest.raises(ValueError):
            W(*args)
    # the 32-neighbour list over three decades: halved to what the pivot rule says, as the model does
    nb32 = pb.logshifts(1.0, 1e3, 32)
    piv = {w: swm.cycle_pivot(nb32, w) for w in (2, 4, 8, 16)}
    want = max(w for w in (2, 4, 8, 16) if piv[w] >= swm.PIVOT)
    assert piv[16] < swm.PIVOT <= piv[4] and W(nb32, 2, 2, 16, 200) == want
    for lst in (nb32, pb.logshifts(1.0, 1e4, 32), pb.logshifts(1.0, 1e3, 32, interleave=True), wide, [-1.0, -1.5, -9.0]):
        for want_w in (1, 2, 3, 6, 8, 16):
            for mw, nb, ms in ((2, 2, 200), (16, 8, 200), (58, 4, 200), (2, 2, 5), (20, 12, 200), (20, 13, 200),
                               (20, 20, 200), (17, 64, 200), (8, 8, 200), (2, 63, 200)):
                assert W(lst, mw, nb, want_w, ms) == swm.sweep_width(lst, mw, nb, want_w, ms)


# ------------------------------------------------------------------------------------ 4. the admissibility study
def test_admissibility_study_reproduces():
    """The table behind RICADI_RADI_SWEEP_PIVOT (tests/golden/radi_sweep_model.npz): the pivots of
    every row live, the rule that takes the bound from the table, and three rows of gain errors live (one seed): the
    refused sweep, the admitted one with the smallest pivot and a well separated one."""
    rows = GOLD["study"]
    assert rows.shape == (len(swm.STUDY_LISTS) * len(swm.STUDY_WIDTHS) + len(swm.STUDY_GAP), 5 + len(swm.SEEDS))
    gap = [r for r in rows if 4.0e-7 < r[4] < 1.1e-5]
    assert len(gap) >= 6 and sum(1 for r in gap if r[4] < swm.PIVOT) >= 4       # the bound is bracketed from both sides
    for r in rows:
        sh = swm.study_shifts(int(r[0]), float(r[1]), bool(r[2]))
        assert abs(swm.cycle_pivot(sh, int(r[3])) - r[4]) <= 1e-12 * r[4]
    admitted = rows[rows[:, 4] >= swm.PIVOT]
    refused = rows[rows[:, 4] < swm.PIVOT]
    assert np.max(admitted[:, 5:]) <= swm.GAIN_BAR and len(refused) >= 1
    assert np.max(rows[rows[:, 4] >= swm.PIVOT / 10.0][:, 5:]) > swm.GAIN_BAR       # a tenth of it admits too much
    f = swm.forms(swm.STUDY_N)[0]
    live = [refused[np.argmin(refused[:, 4])], admitted[np.argmin(admitted[:, 4])], admitted[np.argmax(admitted[:, 4])]]
    for r in live:
        sh = swm.study_shifts(int(r[0]), float(r[1]), bool(r[2]))
        e = swm.study_case(f, sh, int(r[3]), swm.SEEDS[0])
        print("ns %d decades %g interleaved %d width %d pivot %.2e: gain error %.2e (stored %.2e)" % (
            r[0], r[1], r[2], r[3], r[4], e, r[5]))
        assert 0.5 * r[5] <= e <= 2.0 * r[5]
        assert (e <= swm.GAIN_BAR) == (r[4] >= swm.PIVOT)
