"""RADI with generated shifts on the dominant basis (RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT), on the
CPU:

1. the NumPy model (tests/radi_dominant_model.py) against SciPy's dense Riccati solver on ker J -- the four call forms
   and the wide right-hand-side factors (33 .. 58 columns) --, its step counts against the table of DESIGN.md 3d-2 and
   against the cycled list's, and on the ``dre`` forms (8 columns, rank 4) against the column rule's shifts;
2. the library's host entry ``ricadi_host_radi_next_shift_dominant`` (one-sided Jacobi SVD of R, rotation of H, the
   same selection) against the model's ``dominant`` -> ``rotate`` -> ``select`` on every (H, R) the wide runs record;
3. a rank-deficient block whose dependent columns are NOT last: the basis spans the block's range all the same;
4. the refusals and the argument contract.

No GPU is needed: the entry is host code.
"""
import numpy as np
import pytest

import radi_dominant_model as dmm
import radi_model as rm
import radi_shift_model as sm
from optconpy_amd import _lib

BAR = 1e-12           # relative, X and cal E X B (the bar of test_radi_shift_cpu.test_model_reproduces_dense_are)
SHIFT_BAR = 1e-12     # relative, the entry's shift against the model's (the column rule reaches 5e-15 on its pairs;
#                       the room is for the conditioning of the singular subspace: sigma_33 / sigma_32 up to 0.83)


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def small_forms(N):
    return rm.call_forms(N) + rm.call_forms(N, narrow=True)


def run_form(f, tol, **kw):
    p0 = sm.initial_shift(f["calA"], f["calE"])
    return dmm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], [p0], old=f["old"], max_steps=200, res_reltol=tol,
                    **kw)


# ---------------------------------------------------------------------------------------------------- 1. the model
@pytest.mark.parametrize("N", [4, 8])
def test_model_reproduces_dense_are_on_the_call_forms(N):
    fs = small_forms(N)
    assert [f["name"] for f in fs] == ["steady", "dre", "dre_old", "narrow"]
    for f in fs:
        t = run_form(f, 1e-16)
        X, K = rm.dense_are_of(f)
        ex, ek = rel(t["Z"] @ t["Z"].T, X), rel(t["gain"], K)
        print("N = %d %-8s steps %3d fallbacks %d  rel X %.2e  rel K %.2e" % (N, f["name"], t["steps"], t["fallbacks"],
                                                                             ex, ek))
        assert t["stopped"] == "res", f["name"]
        assert ex < BAR and ek < BAR, (f["name"], ex, ek)


@pytest.mark.parametrize("N,mw", dmm.WIDE)
def test_model_reproduces_dense_are_on_the_wide_factors(N, mw):
    f = dmm.wide_form(N, mw)
    t = dmm.wide_run(N, mw, 1e-16)
    X, K = rm.dense_are_of(f)
    ex, ek = rel(t["Z"] @ t["Z"].T, X), rel(t["gain"], K)
    print("N = %d mw = %d steps %3d fallbacks %d  rel X %.2e  rel K %.2e" % (N, mw, t["steps"], t["fallbacks"], ex, ek))
    assert t["stopped"] == "res"
    assert ex < BAR and ek < BAR, (ex, ek)


@pytest.mark.parametrize("N,mw", dmm.WIDE)
def test_model_step_counts_on_the_wide_factors(N, mw):
    """The table of DESIGN.md 3d-2: steps at 1e-10 with the dominant basis, no fallbacks, 32 directions kept in every
    selection, and no more steps than the form's cycled list needs."""
    f, g = dmm.wide_form(N, mw), dmm.wide_run(N, mw)
    cy = rm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], f["ms"], max_steps=200, res_reltol=1e-10)
    print("N = %d mw = %d steps %d (cycled list %d) fallbacks %d smallest margin %.6f" % (
        N, mw, g["steps"], cy["steps"], g["fallbacks"], g["margins"].min()))
    assert g["stopped"] == "res" and cy["stopped"] == "res"
    assert g["steps"] == dmm.STEPS[N, mw] and cy["steps"] == dmm.STEPS_CYCLED[N, mw]
    assert g["steps"] <= cy["steps"]
    assert g["fallbacks"] == 0 and np.all(g["kept"] == 32) and len(g["kept"]) == g["steps"] - 1
    assert np.all(g["ms"] < 0) and len(g["ms"]) == g["steps"]


@pytest.mark.parametrize("N", [4, 8])
def test_model_gives_the_column_rules_shifts_on_the_dre_forms(N):
    """W of 8 columns and rank 4, the dependent columns last: the column rule's basis spans the block's range, the
    dominant rule keeps the same 4 directions in another basis, and the selection does not depend on the basis."""
    for f in rm.call_forms(N)[1:]:
        p0 = sm.initial_shift(f["calA"], f["calE"])
        col = sm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], [p0], old=f["old"], max_steps=200,
                      res_reltol=1e-10)
        dom = run_form(f, 1e-10)
        err = np.max(np.abs(dom["ms"] - col["ms"]) / np.abs(col["ms"]))
        print("N = %d %-8s steps %d / %d, shifts within %.2e" % (N, f["name"], dom["steps"], col["steps"], err))
        assert dom["steps"] == col["steps"] == {4: 13, 8: 16}[N]
        assert np.all(dom["kept"] == 4) and dom["fallbacks"] == 0
        assert err <= 1e-12, err


# ------------------------------------------------------------------------------- 2. the host entry against the model
def test_host_entry_on_the_wide_runs():
    total, worst_all = 0, 0.0
    for N, mw in dmm.WIDE:
        worst = 0.0
        for m, nb, H, Rq in dmm.wide_run(N, mw)["full"]:
            assert m == mw and H.shape == (m, 3 * m + 2 * nb) and Rq.shape == (m, m)
            p_ref, margin, k = dmm.next_shift(m, nb, H, Rq)
            p, mg, kept, refusal = _lib.host_radi_next_shift(m, nb, H, Rq, dominant=True)
            assert refusal is None and kept == k == 32, (refusal, kept, k)
            assert p < 0 and p_ref < 0
            worst = max(worst, abs(p - p_ref) / abs(p_ref))
            total += 1
        print("N = %d mw = %d: shifts within %.2e" % (N, mw, worst))
        worst_all = max(worst_all, worst)
    assert total >= 80
    assert worst_all <= SHIFT_BAR, worst_all


def test_host_entry_is_the_column_rule_on_a_full_rank_narrow_block():
    """Every (H, R) of the N = 8 steady and narrow runs of the column rule: all columns kept by either rule, the same
    subspace, the same shift."""
    for f in (rm.call_forms(8)[0], rm.call_forms(8, narrow=True)[0]):
        full = []
        sm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], [sm.initial_shift(f["calA"], f["calE"])], old=f["old"],
                max_steps=200, res_reltol=1e-10, record_full=full)
        assert len(full) >= 12
        for m, nb, H, Rq in full:
            pc, _, kc, rc = _lib.host_radi_next_shift(m, nb, H, Rq)
            pd, _, kd, rd = _lib.host_radi_next_shift(m, nb, H, Rq, dominant=True)
            assert rc is None and rd is None and kc == kd == m
            assert abs(pc - pd) <= SHIFT_BAR * abs(pc), (pc, pd)


# ------------------------------------------------------------------ 3. dependent columns anywhere in the block
def _dense_instance(nv, m, nb, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((nv, nv))
    calE = M @ M.T / nv + np.eye(nv)
    S = rng.standard_normal((nv, nv))
    N = rng.standard_normal((nv, nv))
    calA = 0.5 * (S - S.T) - N @ N.T / nv - 0.1 * np.eye(nv)
    return calA, calE, rng.standard_normal((nv, nb)), 0.1 * rng.standard_normal((nv, m)), np.zeros((nv, nb))


def test_host_entry_spans_the_range_of_an_interleaved_rank_deficient_block():
    """6 columns, rank 3, the duplicates interleaved (the block of test_radi_shift_cpu's column-rule test, where the
    kept columns of Q do NOT span the block's range).  The dominant basis does: the shift is the one the selection
    gives on an orthonormal basis of the three independent columns themselves."""
    nv, m, nb = 30, 6, 2
    calA, calE, B, R, U = _dense_instance(nv, m, nb, seed=7)
    Z3 = np.random.default_rng(8).standard_normal((nv, 3))
    blk = Z3[:, [0, 0, 1, 2, 1, 2]] * np.array([1.0, -2.0, 1.0, 1.0, 0.5, 3.0])
    Q, Rq = np.linalg.qr(blk)
    assert sm.keep_columns(Rq).tolist() == [True, False, True, True, False, False]
    H = sm.pack(Q, calA, calE, R, U, B)
    p_ref, margin, k = dmm.next_shift(m, nb, H, Rq)
    p, mg, kept, refusal = _lib.host_radi_next_shift(m, nb, H, Rq, dominant=True)
    assert refusal is None and kept == k == 3
    assert abs(p - p_ref) <= SHIFT_BAR * abs(p_ref), (p, p_ref)
    # the block's range itself
    Q3 = np.linalg.qr(Z3)[0]
    p_range = sm.select(3, m, nb, sm.pack(Q3, calA, calE, R, U, B))[0]
    # the column rule on the same block reads another subspace
    p_col = _lib.host_radi_next_shift(m, nb, H, Rq)[0]
    print("interleaved block: dominant %.15g, range %.15g, column rule %.15g" % (p, p_range, p_col))
    assert abs(p - p_range) <= 1e-10 * abs(p_range), (p, p_range)
    # whatever order the columns come in
    perm = [3, 5, 0, 4, 1, 2]
    Qp, Rp = np.linalg.qr(blk[:, perm])
    pp, _, kp, rp = _lib.host_radi_next_shift(m, nb, sm.pack(Qp, calA, calE, R, U, B), Rp, dominant=True)
    assert rp is None and kp == 3 and abs(pp - p_range) <= 1e-10 * abs(p_range)


def test_host_entry_keeps_at_most_32_and_counts_by_singular_values():
    m, nb = 40, 2
    rng = np.random.default_rng(5)
    H = sm.random_instance(m, m, nb, seed=11)
    for sig, want in ((np.ones(m), 32), (np.r_[np.ones(5), 1e-9 * np.ones(m - 5)], 5),
                      (np.r_[4.0, 1.3e-7, 1.1e-7, np.ones(3), np.zeros(m - 6)], 5)):
        U1, U2 = np.linalg.qr(rng.standard_normal((m, m)))[0], np.linalg.qr(rng.standard_normal((m, m)))[0]
        Rq = np.triu(np.linalg.qr((U1 * sig) @ U2.T)[1])
        assert _lib.host_radi_next_shift(m, nb, H, Rq, dominant=True)[2] == want
        assert dmm.dominant(Rq).shape[1] == want


# --------------------------------------------------------------------------------------- 4. refusals and contract
def test_host_entry_refusals():
    H = sm.random_instance(2, 2, 1, seed=1)
    I2 = np.eye(2)
    p, mg, kept, refusal = _lib.host_radi_next_shift(2, 1, H, I2, dominant=True)
    assert refusal is None and kept == 2 and p < 0
    assert abs(p - sm.select(2, 2, 1, H)[0]) <= SHIFT_BAR * abs(p)
    for bad in (np.nan, np.inf, -np.inf):
        for i, j in ((0, 0), (1, 1), (0, 1)):               # every entry of R is looked at
            Rn = I2.copy()
            Rn[i, j] = bad
            assert _lib.host_radi_next_shift(2, 1, H, Rn, dominant=True) == (None, None, 0, "r_not_finite")
    assert _lib.host_radi_next_shift(2, 1, H, np.zeros((2, 2)), dominant=True) == (None, None, 0, "r_zero")
    # a nilpotent R has a zero diagonal and rank one: it is not refused here
    assert _lib.host_radi_next_shift(2, 1, H, np.array([[0.0, 5.0], [0.0, 0.0]]), dominant=True)[2:] == (1, None)
    H0 = np.array([[0.0, 1.0, 0.7, 0.0, 0.0]])             # no eigenvalue in the open left half plane
    assert _lib.host_radi_next_shift(1, 1, H0, np.array([[1.0]]), dominant=True) == (None, None, 1, "no_shift")
    Hs = H.copy()
    Hs[:, 2:4] = np.array([[1.0, 2.0], [2.0, 4.0]])        # singular H_E
    assert _lib.host_radi_next_shift(2, 1, Hs, I2, dominant=True) == (None, None, 2, "breakdown")
    Hn = H.copy()
    Hn[1, 0] = np.nan
    assert _lib.host_radi_next_shift(2, 1, Hn, I2, dominant=True) == (None, None, 2, "breakdown")


def test_host_entry_argument_errors():
    for m, nb in [(0, 1), (128, 1), (2, 65), (2, 0)]:
        with pytest.raises(ValueError):
            _lib.host_radi_next_shift(m, nb, np.zeros(max(m, 1) * (3 * max(m, 0) + 2 * max(nb, 0))),
                                      np.zeros(max(m, 1) ** 2), dominant=True)
    H = sm.random_instance(2, 2, 1, seed=1)
    with pytest.raises(ValueError):
        _lib.host_radi_next_shift(2, 1, H[:, :-1], np.eye(2), dominant=True)
    # m = 127 is served
    m, nb = 127, 1
    p, _, kept, refusal = _lib.host_radi_next_shift(m, nb, sm.random_instance(m, m, nb, seed=2), np.eye(m),
                                                    dominant=True)
    assert refusal is None and kept == 32 and p < 0


# ------------------------------------------------------------------------------- 5. the fixture and the sweep's keyword
def test_fixture_holds_the_models_shifts():
    """tests/golden/radi_dominant_model.npz (the GPU tests' reference) against the live model."""
    g = np.load(dmm.golden_path())
    for N, mw in dmm.GPU_CASES:
        r = dmm.wide_run(N, mw)
        ms = g["ms_%d_%d" % (N, mw)]
        assert len(ms) == r["steps"] == dmm.STEPS[N, mw]
        assert np.max(np.abs(ms - r["ms"]) / np.abs(r["ms"])) <= 1e-9          # (NumPy builds differ in the last bits)
        assert np.max(np.abs(g["res_%d_%d" % (N, mw)] - r["res_hist"]) / r["res_hist"]) <= 1e-6
        assert g["moves_%d_%d" % (N, mw)].shape == (3,)


def test_sweep_refuses_radi_without_a_radi_solver():
    """The oracle's pru has no proj_alg_ric_radi: ValueError before anything is computed; so has another name."""
    import test_dae_ric as td
    from optconpy_amd.dae_ric import MemoryStore, solve_flow_daeric
    from oracle import lin_alg_utils as olau, proj_ric_utils as opru
    pr, kw, tmesh = td._setup(Nts=1)
    store = MemoryStore()
    with pytest.raises(ValueError, match="proj_alg_ric_radi"):
        solve_flow_daeric(store=store, pru=opru, lau=olau, ric_solver="radi", **kw)
    with pytest.raises(ValueError, match="ric_solver"):
        solve_flow_daeric(store=store, pru=opru, lau=olau, ric_solver="adi", **kw)
    assert len(store) == 0
