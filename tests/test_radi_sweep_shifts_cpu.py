"""RADI sweeps with generated shifts (``ms='hamiltonian-sweep'``, ricadi_set_radi_sweep_shifts) without
a GPU:

1. the NumPy model (tests/radi_sweep_shift_model.py) against SciPy's dense Riccati solver on ker J;
2. its step / sweep / width table against the fixture and against the table of DESIGN.md 3d-4;
3. the model at width 1 against tests/radi_dominant_model.radi, shift by shift;
4. the stability study's participants and moves against the fixture;
5. the host entry ``ricadi_host_radi_sweep_shifts`` against the model's dominant -> rotate -> ordered candidates ->
   greedy selection on every (H, Rq) the model runs record;
6. its refusals and special cases;
7. the header's exports, the ABI version and the ctypes mirror.

The model is the yardstick of tests/test_gpu_radi_sweep_shifts.py.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import radi_dominant_model as dmm
import radi_model as rm
import radi_shift_model as sm
import radi_sweep_model as swm
import radi_sweep_shift_model as ssm
from optconpy_amd import _lib

BAR = 1e-12           # relative, X and cal E X B (the bar of test_radi_model_cpu.py)
SHIFT_BAR = 1e-12     # relative, the entry's shifts against the model's (the bar of DESIGN.md 3d-2)
TIE = 1e-9            # two criteria closer than this (relative) may come out in either order
GOLD = np.load(ssm.golden_path())

# (steps, sweeps) of DESIGN.md 3d-4's table, per (case, N, width)
DESIGN_TABLE = {
    ("steady", 4, 2): (13, 7), ("steady", 4, 4): (13, 5), ("steady", 4, 8): (13, 4),
    ("dre", 4, 2): (12, 7), ("dre", 4, 4): (12, 5), ("dre", 4, 8): (12, 4),
    ("steady", 8, 2): (19, 10), ("steady", 8, 4): (20, 6), ("steady", 8, 8): (18, 4),
    ("dre", 8, 2): (18, 10), ("dre", 8, 4): (17, 6), ("dre", 8, 8): (17, 4),
    ("wide33", 8, 2): (19, 10), ("wide33", 8, 3): (18, 7), ("wide58", 8, 2): (20, 11),
    ("random16", 8, 4): (18, 6), ("random16", 8, 8): (18, 4),
}
# steps of the cycled list and of one generated shift per step, per (case, N)
CYCLED = {("steady", 4): 26, ("dre", 4): 17, ("steady", 8): 29, ("dre", 8): 24, ("wide33", 8): 30, ("wide58", 8): 30}
ONE_PER_STEP = {("steady", 4): 15, ("dre", 4): 13, ("steady", 8): 19, ("dre", 8): 16, ("wide33", 8): 19,
                ("wide58", 8): 19, ("random16", 8): 18}


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


# ---------------------------------------------------------------------------------------------------- 1. the model
@pytest.mark.parametrize("N", [4, 8])
def test_model_reproduces_dense_are(N):
    fs = rm.call_forms(N) + rm.call_forms(N, narrow=True)
    assert [f["name"] for f in fs] == ["steady", "dre", "dre_old", "narrow"]
    for f in fs:
        X, K = rm.dense_are_of(f)
        p0 = sm.initial_shift(f["calA"], f["calE"])
        for w in (2, 4, 8):
            t = ssm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], [p0], w, old=f["old"], max_steps=200,
                         res_reltol=1e-16)
            ex, ek = rel(t["Z"] @ t["Z"].T, X), rel(t["gain"], K)
            print("N = %d %-8s width %d: steps %3d sweeps %2d widths %s fallbacks %d  rel X %.2e  rel K %.2e" % (
                N, f["name"], w, t["steps"], t["sweeps"], t["widths"].tolist(), t["fallbacks"], ex, ek))
            assert t["stopped"] == "res", (f["name"], w)
            assert ex < BAR and ek < BAR, (f["name"], w, ex, ek)
            assert t["widths"][0] == 1 and t["widths"].max() <= w and t["solves"] == t["widths"].sum()
            assert len(t["ms"]) == t["steps"] == t["kept_blocks"].sum()


# ---------------------------------------------------------------------------------------------------- 2. the table
def test_model_table():
    """Steps, sweeps, solves, widths, kept blocks and basis sizes of every case equal the fixture's; steps and sweeps
    equal the table of DESIGN.md 3d-4; the claims made of the table hold."""
    assert set(ssm.TABLE) == set(DESIGN_TABLE)
    for name, N, w in ssm.TABLE:
        r, k = ssm.run_case(name, N, w), ssm.key(name, N, w)
        print("%-16s %2d steps / %2d sweeps / %2d solves, widths %s" % (k, r["steps"], r["sweeps"], r["solves"],
                                                                      r["widths"].tolist()))
        assert r["stopped"] == "res" and r["fallbacks"] == 0
        assert [r["steps"], r["sweeps"], r["solves"]] == GOLD["table_" + k].tolist(), k
        assert (r["steps"], r["sweeps"]) == DESIGN_TABLE[name, N, w], k
        assert r["widths"].tolist() == GOLD["widths_" + k].tolist()
        assert r["kept_blocks"].tolist() == GOLD["kblocks_" + k].tolist()
        assert r["kept"].tolist() == GOLD["kept_" + k].tolist()
        # the first sweep is the start shift alone; the cap; solves exceed the steps by at most 4; the step count
        # stays that of one generated shift per step within 3 and below the cycled list's
        f = ssm.case_form(name, N)
        cap = ssm.cap_width(w, f["W"].shape[1], f["B"].shape[1], 200)
        assert r["widths"][0] == 1 and r["widths"].max() <= cap
        assert 0 <= r["solves"] - r["steps"] <= 4
        assert abs(r["steps"] - ONE_PER_STEP[name, N]) <= 3
        if (name, N) in CYCLED:
            assert r["steps"] <= CYCLED[name, N]
        assert np.all(r["ms"] < 0) and len(r["ms"]) == r["steps"]
        if k in GOLD["participants"]:
            assert np.max(np.abs(r["ms"] - GOLD["ms_" + k]) / np.abs(r["ms"])) <= 1e-9     # (NumPy builds differ in the last bits)
            assert np.max(np.abs(r["res_hist"] - GOLD["res_" + k]) / r["res_hist"]) <= 1e-5
    # the caps of the wide factors, and the basis of the 16-column W: 7 of 8 blocks
    assert ssm.cap_width(8, 33, 4, 200) == 3 and ssm.cap_width(8, 58, 4, 200) == 2 and ssm.cap_width(8, 16, 4, 200) == 8
    r = ssm.run_case("random16", 8, 8)
    assert r["kept_blocks"].max() == 8 and r["basis_blocks"].max() == 7
    assert all(rec[0] == min(kb, 7) * 16 for rec, kb in zip(r["record"], r["kept_blocks"]))


# -------------------------------------------------------------------------------------------------- 3. width one
@pytest.mark.parametrize("N", [4, 8])
def test_model_at_width_one_is_the_dominant_model(N):
    for f in rm.call_forms(N):
        p0 = sm.initial_shift(f["calA"], f["calE"])
        a = dmm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], [p0], old=f["old"], res_reltol=1e-10)
        b = ssm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], [p0], 1, old=f["old"], res_reltol=1e-10)
        assert a["steps"] == b["steps"] == b["sweeps"] == b["solves"] and np.all(b["widths"] == 1)
        assert a["kept"].tolist() == b["kept"].tolist() and a["fallbacks"] == b["fallbacks"] == 0
        err = np.max(np.abs(a["ms"] - b["ms"]) / np.abs(a["ms"]))
        print("N = %d %-8s: %d steps, shifts within %.2e" % (N, f["name"], a["steps"], err))
        assert err <= 1e-9, err


# ---------------------------------------------------------------------------------------------- 4. the stability study
def test_stability_study_participants():
    """A case takes part in shift-by-shift comparisons if its shifts move by less than MOVE_BAR under all three seeds;
    the steady and the 33-column cases must; the step counts do not move in any case."""
    part = set(GOLD["participants"].tolist())
    for name, N, w in ssm.TABLE:
        k = ssm.key(name, N, w)
        moves = GOLD["moves_" + k]
        assert moves.shape == (3,) and GOLD["same_" + k].all(), k
        assert (k in part) == bool(np.all(moves < ssm.MOVE_BAR)), (k, moves)
    for c in ssm.MUST_TAKE_PART:
        assert ssm.key(*c) in part, c
        assert GOLD["moves_" + ssm.key(*c)].max() < 3.25e-6          # (3.2e-6 to two digits: steady N = 8 width 8, wide33 width 3)
    # the tie flips of the rank-4 blocks
    for c in (("dre", 4, 4), ("dre", 8, 2), ("dre", 8, 4), ("dre", 4, 8)):
        assert ssm.key(*c) not in part and GOLD["moves_" + ssm.key(*c)].max() >= 7e-3


@pytest.mark.parametrize("case", [("steady", 4, 2), ("steady", 4, 4), ("steady", 4, 8), ("dre", 4, 4), ("steady", 8, 8)])
def test_stability_study_moves_against_the_fixture(case):
    """The live study on the cheap cases: the same participation, moves of the fixture's size."""
    k = ssm.key(*case)
    moves, same = ssm.case_moves(*case)
    print("%s: moves %s (fixture %s)" % (k, moves, GOLD["moves_" + k]))
    assert same.all()
    assert bool(np.all(moves < ssm.MOVE_BAR)) == (k in GOLD["participants"])
    if k in GOLD["participants"]:
        assert np.all(moves <= 2.0 * GOLD["moves_" + k] + 1e-9) and np.all(GOLD["moves_" + k] <= 2.0 * moves + 1e-9)


# ------------------------------------------------------------------------------- 5. the host entry against the model
def near_tie(crit, idx, want):
    """Whether the criteria at the admitted boundary -- the last admitted candidate and the next one in the order, where
    the count `want` ended the walk -- are within TIE of each other: which of the two is admitted is then open to
    rounding.  (Ties inside the admitted list are NOT excluded: the entry has to reproduce their order.)"""
    if len(idx) < want or idx[-1] + 1 >= len(crit):
        return False
    a, b = crit[idx[-1]], crit[idx[-1] + 1]
    return bool(abs(a - b) <= TIE * abs(a))


def test_host_entry_on_the_model_runs():
    total, excluded, worst = 0, 0, 0.0
    for name, N, w in ssm.TABLE:
        for c, m, nb, H, Rq, want in ssm.run_case(name, N, w)["record"]:
            assert H.shape == (c, 2 * c + m + 2 * nb) and Rq.shape == (c, c) and c % m == 0 and c <= 127
            sel, crit_sel, k, ps_all, crit_all = ssm.next_shifts(c, m, nb, H, Rq, want)
            idx = ssm.greedy(ps_all, want)
            total += 1
            if near_tie(crit_all, idx, want):
                excluded += 1
                continue
            ps, crit, kept, refusal = _lib.host_radi_sweep_shifts(c, m, nb, H, Rq, want)
            assert refusal is None and kept == k, (name, N, w, refusal, kept, k)
            assert len(ps) == len(sel) >= 1, (name, N, w, ps, sel)
            worst = max(worst, float(np.max(np.abs(ps - sel) / np.abs(sel))))
            assert np.max(np.abs(crit - crit_sel)) <= 1e-9
            assert swm.smallest_pivot(ps) >= swm.PIVOT
    print("%d selections, %d excluded for a near tie, shifts within %.2e" % (total, excluded, worst))
    assert total >= 80
    assert excluded <= 0.05 * total, (excluded, total)
    assert worst <= SHIFT_BAR, worst


def test_host_entry_with_one_shift_is_the_dominant_entry():
    """want = 1 on the block of one step (c = m): the shift of ricadi_host_radi_next_shift_dominant, bit for bit."""
    n = 0
    for N, mw in ((4, 33), (8, 58)):
        for m, nb, H, Rq in dmm.wide_run(N, mw)["full"]:
            p, _, kept, refusal = _lib.host_radi_next_shift(m, nb, H, Rq, dominant=True)
            ps, crit, kept2, refusal2 = _lib.host_radi_sweep_shifts(m, m, nb, H, Rq, 1)
            assert refusal is None and refusal2 is None and kept == kept2 == 32
            assert ps.tolist() == [p]
            n += 1
    assert n >= 30


# -------------------------------------------------------------------------------------- 6. refusals, special cases
def diag_instance(a, r, nb=1):
    """Packed H (k x (2k + 1 + 2nb)) with H_E = I, H_U = H_B = 0, H_A = diag(a), H_R = r (k x 1): the left-half-plane
    eigenvalues of Ham are the entries of a."""
    k = len(a)
    return np.hstack([np.diag(a), np.eye(k), np.reshape(r, (k, 1)), np.zeros((k, 2 * nb))])


def test_pivot_rule_rejects_the_second_best_candidate():
    a, r = np.array([-1.0, -1.001, -5.0]), np.array([3.0, 2.0, 1.0])
    H = diag_instance(a, r)
    ps_all, crit_all = ssm.candidates(3, 1, 1, H)
    assert np.allclose(ps_all, a, rtol=1e-12) and np.all(np.diff(crit_all) < -1e-3)      # ordered as a, no ties
    assert swm.smallest_pivot([-1.0, -1.001]) < swm.PIVOT <= swm.smallest_pivot([-1.0, -5.0])
    assert ssm.greedy(ps_all, 2) == [0, 2] and ssm.greedy(ps_all, 3) == [0, 2] and ssm.greedy(ps_all, 1) == [0]
    for want, expect in ((1, [0]), (2, [0, 2]), (3, [0, 2]), (16, [0, 2])):
        ps, crit, kept, refusal = _lib.host_radi_sweep_shifts(3, 1, 1, H, np.eye(3), want)
        assert refusal is None and kept == 3
        assert np.allclose(ps, ps_all[expect], rtol=1e-12, atol=0) and np.allclose(crit, crit_all[expect], rtol=1e-9)
    # acceptance order is criterion order, not shift order
    H2 = diag_instance(a[::-1].copy(), r)
    p2, c2 = ssm.candidates(3, 1, 1, H2)
    assert np.all(np.diff(c2) < -1e-3) and not np.all(np.diff(p2) < 0) and not np.all(np.diff(p2) > 0)
    ps, _, _, _ = _lib.host_radi_sweep_shifts(3, 1, 1, H2, np.eye(3), 3)
    assert np.allclose(ps, p2[ssm.greedy(p2, 3)], rtol=1e-12, atol=0) and len(ps) == 2


def test_exact_tie_takes_the_larger_modulus_first():
    """Two decoupled copies of one direction with the residual scaled so that the criteria are EQUAL: H_A = diag(a, 4a),
    H_E = I, H_R = diag(r, 2r) scales Ham's second copy by exactly 4 (a power of two: no rounding)."""
    H = np.hstack([np.diag([-1.5, -6.0]), np.eye(2), np.diag([0.25, 0.5]), np.zeros((2, 2))])
    ps_all, crit_all = ssm.candidates(2, 2, 1, H)
    assert crit_all[0] == crit_all[1] and ps_all.tolist() == [-6.0, -1.5]
    ps, crit, _, refusal = _lib.host_radi_sweep_shifts(2, 2, 1, H, np.eye(2), 2)
    assert refusal is None and ps.tolist() == [-6.0, -1.5] and crit[0] == crit[1]


def test_basis_of_one_column_and_refusals():
    H = diag_instance(np.array([-2.0]), np.array([1.0]))
    ps, crit, kept, refusal = _lib.host_radi_sweep_shifts(1, 1, 1, H, np.array([[4.0]]), 8)
    assert refusal is None and kept == 1 and ps.tolist() == [-2.0] and len(crit) == 1
    # a group of two columns against a residual of one: c != m
    H2 = diag_instance(np.array([-2.0, -7.0]), np.array([1.0, 0.5]))
    ps, _, kept, refusal = _lib.host_radi_sweep_shifts(2, 1, 1, H2, np.eye(2), 8)
    assert refusal is None and kept == 2 and np.allclose(ps, [-2.0, -7.0], rtol=1e-13)
    # a dependent column of the group leaves the basis
    ps, _, kept, refusal = _lib.host_radi_sweep_shifts(2, 1, 1, H2, np.array([[1.0, 0.0], [0.0, 1e-9]]), 8)
    assert refusal is None and kept == 1 and np.allclose(ps, [-2.0], rtol=1e-13)
    empty = (0, 0)
    for bad in (np.nan, np.inf):
        Rn = np.eye(2)
        Rn[0, 1] = bad
        out = _lib.host_radi_sweep_shifts(2, 1, 1, H2, Rn, 8)
        assert (len(out[0]), len(out[1])) == empty and out[2:] == (0, "r_not_finite")
    out = _lib.host_radi_sweep_shifts(2, 1, 1, H2, np.zeros((2, 2)), 8)
    assert (len(out[0]), len(out[1])) == empty and out[2:] == (0, "r_zero")
    H0 = np.array([[0.0, 1.0, 0.7, 0.0, 0.0]])              # no eigenvalue in the open left half plane
    assert _lib.host_radi_sweep_shifts(1, 1, 1, H0, np.array([[1.0]]), 8)[2:] == (1, "no_shift")
    Hs = H2.copy()
    Hs[:, 2:4] = np.array([[1.0, 2.0], [2.0, 4.0]])         # singular H_E
    assert _lib.host_radi_sweep_shifts(2, 1, 1, Hs, np.eye(2), 8)[2:] == (2, "breakdown")
    for c, m, nb, want in [(0, 1, 1, 1), (128, 1, 1, 1), (1, 0, 1, 1), (1, 128, 1, 1), (1, 1, 0, 1), (1, 1, 65, 1),
                           (1, 1, 1, 0), (1, 1, 1, 17)]:
        with pytest.raises(ValueError):
            _lib.host_radi_sweep_shifts(c, m, nb, np.zeros(max(c, 1) * (2 * max(c, 0) + max(m, 0) + 2 * max(nb, 0))),
                                        np.zeros(max(c, 1) ** 2), want)
    with pytest.raises(ValueError):
        _lib.host_radi_sweep_shifts(2, 1, 1, H2[:, :-1], np.eye(2), 2)


# ------------------------------------------------------------------------------------------- 7. header, ABI, ctypes
def test_header_exports_abi_and_signatures():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    hdr = open(os.path.join(root, "include", "ricadi.h")).read()
    for proto in (r"int ricadi_set_radi_sweep_shifts\(ricadi_ctx\* ctx, int on\);",
                  r"int ricadi_radi_sweep_widths\(ricadi_ctx\* ctx, int\* out, int cap, int\* n_out\);",
                  r"int ricadi_radi_reduce_group_dev\(ricadi_ctx\* ctx, const double\* dQ, int c, const double\* dRU, "
                  r"int m, const double\* dB,\s+int nb, double\* dH_out\);",
                  r"int ricadi_host_radi_sweep_shifts\(int c, int m, int nb, const double\* H, const double\* R, int want, "
                  r"double\* ps_out,\s+double\* crit_out, int\* n_out, int\* kept_out\);"):
        assert re.search(proto, hdr), proto
    assert "ABI 412" in hdr
    assert float(re.search(r"#define RICADI_RADI_SWEEP_PIVOT (\S+)", hdr).group(1)) == swm.PIVOT
    assert float(re.search(r"#define RICADI_RADI_RANK_TOL (\S+)", hdr).group(1)) == sm.RANK_TOL
    lib = _lib.load()
    assert lib.ricadi_version() == _lib.ABI_VERSION == 414
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    sig = {"ricadi_set_radi_sweep_shifts": [C.c_void_p, C.c_int],
           "ricadi_radi_sweep_widths": [C.c_void_p, None, C.c_int, ip],
           "ricadi_radi_reduce_group_dev": [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                            C.c_void_p],
           "ricadi_host_radi_sweep_shifts": [C.c_int, C.c_int, C.c_int, None, None, C.c_int, None, None, ip, ip]}
    for name, args in sig.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(args), name
        for got, want in zip(fn.argtypes, args):
            assert want is None or got is want, (name, got, want)
    for name in ("set_radi_sweep_shifts", "radi_sweep_widths", "radi_reduce_group_dev"):
        assert callable(getattr(_lib.Context, name))
    assert callable(_lib.host_radi_sweep_shifts)
