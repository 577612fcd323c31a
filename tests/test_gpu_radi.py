"""GPU tests of the low-rank RADI solver (ricadi_radi.hip, csrc/solver_radi.inl, pru.proj_alg_ric_radi).

1. the dense part of a step (ricadi_radi_update_dev) entry by entry against the longdouble model of
   tests/radi_model.py, at ``bound(2^-53) + bound(u_longdouble)`` with the bounds derived there;
2. the whole solve against SciPy's dense Riccati solver on ker J for the three call forms of the dense pin;
3. the residual history against the NumPy model's;
4. stopping and statistics;  5. nothing left behind in the context;  6. the argument contract.

tests/test_radi_model_cpu.py holds the model itself to the dense solver; it has to pass for these to mean anything.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spsla

import dense_model as dm
import radi_model as rm
from optconpy_amd import _lib, backend

pytestmark = pytest.mark.gpu
K_TOL = 1e-6          # the project's parity bar
# Largest relative deviation of the device's residual history from the model's over the entries above 1e-6 (N = 8,
# steady form) as measured on the MI355X; the test asserts ten times that (the margin covers the inexact
# solves' dependence on iteration counts).
HIST_MEASURED = 3.636e-10


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


_forms, _models, _dense = {}, {}, {}


def forms(N):
    if N not in _forms:
        _forms[N] = rm.call_forms(N)
    return _forms[N]


def model(N, i, tol):
    """The NumPy model's run of call form i at mesh size N (computed once per tolerance)."""
    key = (N, i, tol)
    if key not in _models:
        f = forms(N)[i]
        _models[key] = rm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], f["ms"], old=f["old"], max_steps=200,
                               res_reltol=tol)
    return _models[key]


def dense(N, i):
    if (N, i) not in _dense:
        _dense[(N, i)] = rm.dense_are_of(forms(N)[i])
    return _dense[(N, i)]


@pytest.fixture(scope="module")
def ctx4():
    """Context with the operator of the steady form at N = 4 (nv = 98: no multiple of 16, 32 or 64)."""
    f = forms(4)[0]
    ctx = _lib.Context(0)
    ctx.set_operator(f["calA"], f["calE"], f["J"])
    yield ctx, f
    ctx.close()


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------- 1. the update step
SHAPES = [(1, 1), (3, 2), (4, 4), (16, 4), (17, 3), (64, 64)]


def _update_inputs(nv, n, m, nb, p, wide_v):
    """V in a panel of n rows (pressure rows NaN: they must not be read) and width ldv, B scaled so that
    ||G G^T||_2 = 4 (Y = I + G G^T between I and 5 I: cond(Y) <= 5), the panel [R | U]."""
    rng = np.random.default_rng(1000 * m + nb)
    ldv = m + nb if wide_v else m
    Vp = np.full((n, ldv), np.nan)
    Vp[:nv] = rng.standard_normal((nv, ldv))
    V = np.ascontiguousarray(Vp[:nv, :m])
    B = rng.standard_normal((nv, nb))
    G0 = V.T @ B
    B *= np.sqrt(4.0 / np.linalg.norm(G0 @ G0.T, 2))
    RU = rng.standard_normal((nv, m + nb))
    return Vp, ldv, V, B, RU


@pytest.mark.parametrize("p", [-1.0, -2e3])
@pytest.mark.parametrize("m,nb", SHAPES)
def test_update_step_entry_by_entry(ctx4, m, nb, p):
    """G componentwise, C, the new [R | U] and the Z block against the longdouble model; guard entries; the same
    call twice bitwise.  (4, 4) runs with V inside the solve's panel of width m + nb, (17, 3) with the Z block at
    column 5 of a buffer of width 2m + 7."""
    ctx, f = ctx4
    nv, n = ctx.nv, ctx.n
    Vp, ldv, V, B, RU = _update_inputs(nv, n, m, nb, p, wide_v=(m, nb) == (4, 4))
    zoff, ldz = (5, 2 * m + 7) if (m, nb) == (17, 3) else (0, m)
    G, Cm, RUn, Zb = rm.update(p, V, B, RU, f["calE"])
    Y = np.eye(m) + np.asarray(G @ G.T, dtype=float)
    assert np.linalg.cond(Y) <= 10.0
    tG, tC, tRU, tZ = dm.tol(rm.update_bounds, p, V, B, RU, f["calE"])
    Vd, Bd = _dev(Vp), _dev(B)
    outs = []
    for _ in range(2):
        RUd = _dev(np.stack([RU, RU]))          # the second panel is a guard
        Zd = _dev(np.full((nv, ldz), np.nan))
        Gd, Cd = _dev(np.full((m, nb), np.nan)), _dev(np.full((m, 2 * m + nb), np.nan))
        ctx.radi_update_dev(p, Vd.data_ptr(), ldv, m, Bd.data_ptr(), nb, RUd.data_ptr(), Zd.data_ptr(), ldz, zoff,
                            Gd.data_ptr(), Cd.data_ptr())
        outs.append([_host(t) for t in (Gd, Cd, RUd, Zd)])
    Gh, Ch, RUh, Zh = outs[0]
    ratios = dict(G=dm.ratio(Gh, G, tG), C=dm.ratio(Ch, Cm, tC), RU=dm.ratio(RUh[0], RUn, tRU),
                  Z=dm.ratio(Zh[:, zoff:zoff + m], Zb, tZ))
    print("m %d nb %d p %g: error / bound " % (m, nb, p) + "  ".join("%s %.3g" % kv for kv in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    assert np.array_equal(RUh[1], RU)                                   # the untouched panel
    guard = np.ones(ldz, dtype=bool)
    guard[zoff:zoff + m] = False
    assert np.all(np.isnan(Zh[:, guard])) and not np.any(np.isnan(Zh[:, ~guard]))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b, equal_nan=True)                      # bitwise: fixed summation order
    # without dC_out the same update
    RUd, Zd, Gd = _dev(RU), _dev(np.full((nv, ldz), np.nan)), _dev(np.zeros((m, nb)))
    ctx.radi_update_dev(p, Vd.data_ptr(), ldv, m, Bd.data_ptr(), nb, RUd.data_ptr(), Zd.data_ptr(), ldz, zoff,
                        Gd.data_ptr(), None)
    assert np.array_equal(_host(RUd), RUh[0]) and np.array_equal(_host(Zd), Zh, equal_nan=True)


# ------------------------------------------------------------------------------------------- 2. the whole solve
@pytest.mark.parametrize("N", [4, 8])
def test_radi_vs_dense_are_three_call_forms(N):
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    backend.reset()
    try:
        for i, f in enumerate(forms(N)):
            X, K = dense(N, i)
            d = dict(ms=f["ms"], radi_res_reltol=1e-12, radi_max_steps=200)
            out = pru.proj_alg_ric_radi(radi_dict=d, **f["kw"])
            Z = out["zfac"]
            mod = model(N, i, 1e-12)
            print("N = %d %-8s steps %d (model %d)  rel X %.2e  rel K %.2e  gmres its %d" % (
                N, f["name"], out["radi_steps"], mod["steps"], rel(Z @ Z.T, X), rel(out["gain"], K),
                out["gmres_iters"]))
            assert rel(Z @ Z.T, X) < 1e-6, f["name"]
            assert rel(out["gain"], K) < K_TOL, f["name"]
            # the gain from the factor: cal E Z Z^T B (what get_mTzzTtb forms), plus nothing else
            assert rel(pru.get_mTzzTtb(f["calE"], Z, f["B"]), out["gain"]) < 1e-8, f["name"]
            assert out["gmres_nonconverged"] == 0
            assert out["stop_rule"] == _lib.RICADI_STOP_RES
            assert out["radi_steps"] <= mod["steps"] + 2, (out["radi_steps"], mod["steps"])
            assert out["shift_solves"] == out["radi_steps"] == len(out["res_hist"])
            if i == 0:
                dev = pru.proj_alg_ric_radi(radi_dict=dict(d, device_resident=True), **f["kw"])
                assert isinstance(dev["zfac"], pru.DeviceFactor)
                assert rel(dev["gain"], out["gain"]) < 1e-10
                Zd = np.asarray(dev["zfac"])
                assert rel(Zd @ Zd.T, X) < 1e-6
    finally:
        backend.reset()


# ------------------------------------------------------------------------------------------- 3. the history
def test_history_against_the_model():
    """N = 8, steady form: the device's relative residual after every step against the model's, over the entries
    above 1e-6.  Measured on the MI355X: see HIST_MEASURED; asserted at ten times that."""
    f = forms(8)[0]
    mod = model(8, 0, 1e-12)
    with _lib.Context(0) as ctx:
        ctx.set_operator(f["calA"], f["calE"], f["J"])
        _, _, info = ctx.ric_radi(f["ms"], f["B"], f["W"], max_steps=200, res_reltol=1e-12)
        hist = ctx.adi_res_history()
    k = min(len(hist), len(mod["res_hist"]))
    big = mod["res_hist"][:k] > 1e-6
    assert big.sum() >= 8
    dev = float(np.max(np.abs(hist[:k][big] - mod["res_hist"][:k][big]) / mod["res_hist"][:k][big]))
    print("history against the model: largest relative deviation %.3e over %d entries (%d steps, model %d)"
          % (dev, big.sum(), len(hist), mod["steps"]))
    assert HIST_MEASURED is not None, "no measurement recorded"
    assert dev <= 10.0 * HIST_MEASURED


# ------------------------------------------------------------------------------------------- 4. stopping, statistics
def test_max_steps_stops_and_counts(ctx4):
    ctx, f = ctx4
    mw = f["W"].shape[1]
    Z, K, info = ctx.ric_radi(f["ms"], f["B"], f["W"], max_steps=5, res_reltol=1e-12, compress_cols=10 * mw)
    hist = ctx.adi_res_history()
    assert info["radi_steps"] == 5 and info["stop_rule"] == "max_steps"
    assert len(hist) == 5 and np.all(np.diff(hist) < 0) and hist[-1] == info["res_rel"]
    assert info["shift_solves"] == 5
    assert Z.shape == (ctx.nv, 5 * mw) and info["cols"] == 5 * mw
    # the residual rule ends it where the history first crosses
    # (the solves are iterative: their last bits, and with them the history's, differ from run to run)
    assert hist[1] > 1.01 * hist[2]
    Z2, K2, info2 = ctx.ric_radi(f["ms"], f["B"], f["W"], max_steps=5, res_reltol=1.01 * hist[2])
    assert info2["radi_steps"] == 3 and info2["stop_rule"] == "res"
    assert rel(Z2 @ Z2.T, Z[:, :3 * mw] @ Z[:, :3 * mw].T) < 1e-8


# ------------------------------------------------------------------------------------------- 5. nothing left behind
def _lu_solve(f, p, R):
    nv, npr = f["calE"].shape[0], f["J"].shape[0]
    S = sps.bmat([[f["calA"] + p * f["calE"], f["J"].T], [f["J"], None]], format="csc")
    return spsla.splu(S).solve(np.vstack([R, np.zeros((npr, R.shape[1]))]))


def test_nothing_left_behind(ctx4):
    """A plain shift solve before and after a RADI call agrees with SciPy's sparse LU; no Sherman-Morrison-Woodbury
    solve and no in-operator low-rank term for the later one; the recycling depth of direct calls as before."""
    ctx, f = ctx4
    R = np.random.default_rng(3).standard_normal((ctx.nv, 4))
    ref = _lu_solve(f, -7.0, R)
    ctx.set_recycle(2)
    try:
        X0, _, _ = ctx.shift_solve(-7.0, 1.0, R)
        assert rel(X0, ref) < 1e-8
        t0 = ctx.solve_trace()
        _, _, info = ctx.ric_radi(f["ms"], f["B"], f["W"], max_steps=6, res_reltol=1e-12)
        t1 = ctx.solve_trace()
        assert t1["solves"] - t0["solves"] == 6 + 1          # the steps and the projection
        assert t1["smw_solves"] - t0["smw_solves"] == 5      # the first step's U is zero: plain operator
        assert t1["smw_dup"] - t0["smw_dup"] == 5            # S^-1 U from the panel's own columns, every time
        assert t1["guess_tried"] == t0["guess_tried"] and t1["stored"] == t0["stored"]      # recycling off inside
        X1, _, _ = ctx.shift_solve(-7.0, 1.0, R)
        t2 = ctx.solve_trace()
        assert rel(X1, ref) < 1e-8
        assert t2["smw_solves"] == t1["smw_solves"] and t2["inop_lowrank"] == t1["inop_lowrank"]
        assert t2["guess_tried"] == t1["guess_tried"] + 1 and t2["stored"] == t1["stored"] + 1     # depth as before
    finally:
        ctx.set_recycle(0)


# ------------------------------------------------------------------------------------------- 6. contract
def test_contract(ctx4):
    ctx, f = ctx4
    B, W, ms = f["B"], f["W"], np.asarray(f["ms"], dtype=float)
    nv = ctx.nv
    t0 = ctx.solve_trace()["solves"]
    wide = np.zeros((nv, 65))
    bad = [
        dict(B=wide),                                   # nb > 64
        dict(W=np.zeros((nv, 125))),                    # mw + nb > 128
        dict(max_steps=0),
        dict(shifts=np.zeros(0)),
        dict(shifts=np.array([-1.0, 0.0])),
        dict(shifts=np.array([-1.0, 2.0])),
    ]
    for kw in bad:
        a = dict(shifts=ms, B=B, W=W, max_steps=5)
        a.update(kw)
        with pytest.raises(ValueError):
            ctx.ric_radi(a["shifts"], a["B"], a["W"], max_steps=a["max_steps"])
    # Z_out too small for max_steps * mw columns
    Bc, Wc = np.ascontiguousarray(B), np.ascontiguousarray(W)
    Z = np.zeros((nv, 5 * W.shape[1] - 1))
    stats, cc = np.zeros(8), C.c_int(0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = ctx._lib.ricadi_ric_radi(ctx._h, dp(ms), ms.size, dp(Bc), Bc.shape[1], dp(Wc), Wc.shape[1], None, 5, 1e-10, 0,
                                  1, 0, dp(Z), Z.shape[1], C.byref(cc), None, dp(stats))
    assert rc == -1
    assert ctx.solve_trace()["solves"] == t0            # nothing was launched
    # a context with an exchange set: nothing is sharded here
    ident = C.create_string_buffer(128)
    assert ctx._lib.ricadi_rccl_unique_id(ident, 128) == 0
    _lib._chk(ctx._lib.ricadi_set_exchange_rccl(ctx._h, 0, 1, ident, None, 8 * ctx.n * 16 * 8 + 4096 * 2))
    try:
        rc = ctx._lib.ricadi_ric_radi(ctx._h, dp(ms), ms.size, dp(Bc), Bc.shape[1], dp(Wc), Wc.shape[1], None, 5,
                                      1e-10, 0, 1, 0, None, 0, C.byref(cc), None, dp(stats))
        assert rc == -5 and b"shard" in ctx._lib.ricadi_last_error()
        assert ctx.solve_trace()["solves"] == t0
    finally:
        _lib._chk(ctx._lib.ricadi_set_exchange(ctx._h, 0, 1, None, None, None, None, 0))
    Z, K, info = ctx.ric_radi(ms, B, W, max_steps=3)
    assert info["radi_steps"] == 3
