"""GPU tests of RADI with shifts generated from the iteration (ricadi_set_radi_shifts).

1. the reduction kernel (ricadi_radi_reduce_dev) entry by entry against a longdouble product, exact on small integers,
   bitwise equal on a second call;
2. the whole solve in HAMILTONIAN mode against SciPy's dense Riccati solver on ker J, three call forms, and its step
   count against the same call with the form's cycled list;
3. the shift of every step and the step count against the NumPy model (tests/radi_shift_model.py);
4. the per-shift cache: nothing left behind, the same bits on a second call and in CYCLE mode afterwards;
5. the argument contract.

tests/test_radi_shift_cpu.py holds the model and the host selection; it has to pass for these to mean anything.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

import dense_model as dm
import radi_model as rm
import radi_shift_model as sm
from optconpy_amd import _lib, adi_shifts, backend

pytestmark = pytest.mark.gpu
K_TOL = 1e-6          # the bars of tests/test_gpu_radi.py for the cycled list
X_TOL = 1e-6
# Largest relative deviation of the device's shifts from the model's (N = 8, steady form, radi_res_reltol = 1e-10) as
# measured on the MI355X; the test asserts ten times that and that the bound stays below 1e-3 (the
# margin covers the inexact solves' dependence on iteration counts; a flipped selection is an O(1) difference).
SHIFT_MEASURED = 4.507e-10


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


_forms, _models = {}, {}


def forms(N):
    if N not in _forms:
        _forms[N] = rm.call_forms(N)
    return _forms[N]


def model(N, i, tol):
    """The generated-shift model's run of call form i at mesh size N (computed once per tolerance)."""
    key = (N, i, tol)
    if key not in _models:
        f = forms(N)[i]
        p0 = sm.initial_shift(f["calA"], f["calE"])
        _models[key] = sm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], [p0], old=f["old"], max_steps=200,
                               res_reltol=tol)
    return _models[key]


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module", params=[4, 8])
def ctx_op(request):
    """Context with the operator of the steady form (nv = 98 / 450: no multiple of 16 or 64)."""
    f = forms(request.param)[0]
    ctx = _lib.Context(0)
    ctx.set_operator(f["calA"], f["calE"], f["J"])
    yield ctx, f
    ctx.close()


@pytest.fixture(scope="module")
def ctx8():
    f = forms(8)[0]
    ctx = _lib.Context(0)
    ctx.set_operator(f["calA"], f["calE"], f["J"])
    yield ctx, f
    ctx.close()


# ------------------------------------------------------------------------------------------- 1. the reduction kernel
SHAPES = [(1, 1, 1), (3, 3, 1), (4, 4, 2), (8, 8, 2), (32, 32, 64)]


def _reduce(ctx, Q, RU, B):
    k, m, nb = Q.shape[1], RU.shape[1] - B.shape[1], B.shape[1]
    Qd, RUd, Bd = _dev(Q), _dev(RU), _dev(B)
    Hd = _dev(np.full((k + 1, 2 * k + m + 2 * nb), np.nan))          # one guard row
    ctx.radi_reduce_dev(Qd.data_ptr(), k, RUd.data_ptr(), m, Bd.data_ptr(), nb, Hd.data_ptr())
    H = _host(Hd)
    assert np.all(np.isnan(H[k])) and not np.any(np.isnan(H[:k]))
    return H[:k]


@pytest.mark.parametrize("k,m,nb", SHAPES)
def test_reduce_entry_by_entry(ctx_op, k, m, nb):
    ctx, f = ctx_op
    nv = ctx.nv
    rng = np.random.default_rng(100 * k + nb)
    Q = rng.standard_normal((nv, k))
    RU, B = rng.standard_normal((nv, m + nb)), rng.standard_normal((nv, nb))
    ref = sm.reduce(Q, f["calA"], f["calE"], RU, B)
    tol = dm.tol(sm.reduce_bounds, Q, f["calA"], f["calE"], RU, B)
    H = _reduce(ctx, Q, RU, B)
    ratio = dm.ratio(H, ref, tol)
    print("nv %d k %d m %d nb %d: error / bound %.3g" % (nv, k, m, nb, ratio))
    assert ratio <= 1.0
    assert np.array_equal(_reduce(ctx, Q, RU, B), H)                   # bitwise: fixed summation order
    # the dense blocks of small integers are exact (the operator's values are not integers)
    Qi = rng.integers(-3, 4, (nv, k)).astype(float)
    RUi, Bi = rng.integers(-3, 4, (nv, m + nb)).astype(float), rng.integers(-3, 4, (nv, nb)).astype(float)
    Hi = _reduce(ctx, Qi, RUi, Bi)
    assert np.array_equal(Hi[:, 2 * k:], Qi.T @ np.hstack([RUi, Bi]))


def test_reduce_exact_on_small_integers():
    """An operator with small integer values on the pattern of the N = 4 operator: every entry of H is exact."""
    f = forms(4)[0]
    rng = np.random.default_rng(7)

    def ints(M):
        M = sps.csr_matrix(M).copy()
        M.data = rng.integers(-4, 5, M.nnz).astype(float)
        return M

    A, E = ints(f["calA"]), ints(f["calE"])
    with _lib.Context(0) as ctx:
        ctx.set_operator(A, E, f["J"])
        nv = ctx.nv
        for k, m, nb in [(3, 3, 1), (32, 32, 64)]:
            Q = rng.integers(-3, 4, (nv, k)).astype(float)
            RU, B = rng.integers(-3, 4, (nv, m + nb)).astype(float), rng.integers(-3, 4, (nv, nb)).astype(float)
            ref = Q.T @ np.hstack([A @ Q, E @ Q, RU, B])
            assert np.array_equal(_reduce(ctx, Q, RU, B), ref)


# ------------------------------------------------------------------------------------------- 2. the whole solve
@pytest.mark.parametrize("N", [4, 8])
def test_hamiltonian_vs_dense_are_three_call_forms(N):
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    backend.reset()
    try:
        for i, f in enumerate(forms(N)):
            X, K = rm.dense_are_of(f)
            d = dict(ms="hamiltonian", radi_res_reltol=1e-12, radi_max_steps=200)
            out = pru.proj_alg_ric_radi(radi_dict=d, **f["kw"])
            cyc = pru.proj_alg_ric_radi(radi_dict=dict(d, ms=f["ms"]), **f["kw"])
            Z = out["zfac"]
            print("N = %d %-8s steps %d (cycled list %d, model %d)  fallbacks %d  rel X %.2e  rel K %.2e  gmres its %d"
                  % (N, f["name"], out["radi_steps"], cyc["radi_steps"], model(N, i, 1e-12)["steps"],
                     out["shift_fallbacks"], rel(Z @ Z.T, X), rel(out["gain"], K), out["gmres_iters"]))
            assert rel(Z @ Z.T, X) < X_TOL, f["name"]
            assert rel(out["gain"], K) < K_TOL, f["name"]
            assert out["gmres_nonconverged"] == 0
            assert out["stop_rule"] == _lib.RICADI_STOP_RES
            assert out["radi_steps"] <= cyc["radi_steps"], (f["name"], out["radi_steps"], cyc["radi_steps"])
            assert len(out["ms"]) == out["radi_steps"] == out["shift_solves"] and np.all(np.asarray(out["ms"]) < 0)
            assert "ms" not in cyc and "shift_fallbacks" not in cyc
    finally:
        backend.reset()


# ------------------------------------------------------------------------------------------- 3. against the model
def _ham_run(ctx, f, tol=1e-10, max_steps=200, ms=None):
    """One HAMILTONIAN call on a context (the mode is restored): (K, info, shift history, fallbacks)."""
    p0 = adi_shifts.initial_shift(ctx.diag_ratio)
    before = ctx.set_radi_shifts("hamiltonian")
    try:
        _, K, info = ctx.ric_radi([p0] if ms is None else ms, f["B"], f["W"], max_steps=max_steps, res_reltol=tol)
    finally:
        ctx.set_radi_shifts(before)
    return K, info, ctx.radi_shift_history(), ctx.radi_shift_fallbacks()


def test_shift_history_and_step_count_against_the_model(ctx8):
    """N = 8, steady form, 1e-10: every step's shift against the model's (whose smallest margin there is 1.06) and
    the step count, give or take one."""
    ctx, f = ctx8
    mod = model(8, 0, 1e-10)
    assert mod["margins"].min() >= 1.06 and mod["fallbacks"] == 0
    K, info, hist, nfb = _ham_run(ctx, f)
    k = min(len(hist), len(mod["ms"]))
    dev = float(np.max(np.abs(hist[:k] - mod["ms"][:k]) / np.abs(mod["ms"][:k])))
    print("shifts against the model: largest relative deviation %.3e over %d steps (device %d steps, model %d), "
          "fallbacks %d" % (dev, k, len(hist), mod["steps"], nfb))
    assert info["radi_steps"] == len(hist) and info["stop_rule"] == "res"
    assert nfb == 0
    assert abs(info["radi_steps"] - mod["steps"]) <= 1
    assert SHIFT_MEASURED is not None, "no measurement recorded"
    assert 10.0 * SHIFT_MEASURED < 1e-3
    assert dev <= 10.0 * SHIFT_MEASURED


# ------------------------------------------------------------------------------------------- 4. the cache
def test_cache_holds_nothing_new_and_the_bits_repeat(ctx8):
    ctx, f = ctx8
    p0 = adi_shifts.initial_shift(ctx.diag_ratio)
    _, Kc, infoc = ctx.ric_radi(f["ms"], f["B"], f["W"], max_steps=200, res_reltol=1e-10)       # CYCLE mode
    hc = ctx.radi_shift_history()
    assert np.array_equal(hc, [f["ms"][j % len(f["ms"])] for j in range(infoc["radi_steps"])])
    assert ctx.radi_shift_fallbacks() == 0
    n0 = ctx.cache_entries()
    K1, info1, h1, fb1 = _ham_run(ctx, f)
    n1 = ctx.cache_entries()
    print("cache entries: %d before, %d after %d steps with generated shifts" % (n0, n1, info1["radi_steps"]))
    assert len(set(h1)) == len(h1) > 5                   # all distinct: each one was set up
    assert n1 <= n0 + 1                                  # the list has one entry
    K2, info2, h2, fb2 = _ham_run(ctx, f)
    assert ctx.cache_entries() == n1
    assert np.array_equal(K2, K1) and np.array_equal(h2, h1) and fb2 == fb1 == 0
    # a list of three: the first entry starts, nothing else of it is used while shifts can be generated
    K3, info3, h3, _ = _ham_run(ctx, f, ms=[p0, -3.0, -70.0])
    assert np.array_equal(K3, K1) and ctx.cache_entries() == n1
    # a call that ends early leaves nothing either
    _ham_run(ctx, f, max_steps=3)
    assert ctx.cache_entries() == n1
    # CYCLE mode afterwards: the bits it gave before
    _, Kc2, infoc2 = ctx.ric_radi(f["ms"], f["B"], f["W"], max_steps=200, res_reltol=1e-10)
    assert np.array_equal(Kc2, Kc) and infoc2["radi_steps"] == infoc["radi_steps"]
    assert np.array_equal(ctx.radi_shift_history(), hc)
    assert ctx.cache_entries() == n1


# ------------------------------------------------------------------------------------------- 5. contract
def test_contract():
    f = forms(4)[0]
    B, W, ms = np.ascontiguousarray(f["B"]), np.ascontiguousarray(f["W"]), np.asarray(f["ms"], dtype=float)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    with _lib.Context(0) as ctx:
        ctx.set_operator(f["calA"], f["calE"], f["J"])
        nv = ctx.nv
        n, nfb = C.c_int(0), C.c_int(0)
        assert ctx._lib.ricadi_radi_shift_history(ctx._h, None, 0, C.byref(n)) == -5        # before any RADI call
        assert ctx._lib.ricadi_radi_shift_fallbacks(ctx._h, C.byref(nfb)) == -5
        assert ctx._lib.ricadi_set_radi_shifts(ctx._h, 2) == -1
        ctx.set_radi_shifts("hamiltonian")
        t0 = ctx.solve_trace()["solves"]
        stats, cc = np.zeros(8), C.c_int(0)
        W33 = np.zeros((nv, 33))
        rc = ctx._lib.ricadi_ric_radi(ctx._h, dp(ms), ms.size, dp(B), B.shape[1], dp(W33), 33, None, 5, 1e-10, 0, 1, 0,
                                      None, 0, C.byref(cc), None, dp(stats))
        assert rc == -1 and b"mw <= 32" in ctx._lib.ricadi_last_error()
        assert ctx.solve_trace()["solves"] == t0                                            # nothing was launched
        # a context with an exchange set: nothing is sharded here
        ident = C.create_string_buffer(128)
        assert ctx._lib.ricadi_rccl_unique_id(ident, 128) == 0
        _lib._chk(ctx._lib.ricadi_set_exchange_rccl(ctx._h, 0, 1, ident, None, 8 * ctx.n * 16 * 8 + 4096 * 2))
        try:
            rc = ctx._lib.ricadi_ric_radi(ctx._h, dp(ms), ms.size, dp(B), B.shape[1], dp(W), W.shape[1], None, 5,
                                          1e-10, 0, 1, 0, None, 0, C.byref(cc), None, dp(stats))
            assert rc == -5 and b"shard" in ctx._lib.ricadi_last_error()
            assert ctx.solve_trace()["solves"] == t0
        finally:
            _lib._chk(ctx._lib.ricadi_set_exchange(ctx._h, 0, 1, None, None, None, None, 0))
        # in CYCLE mode the same width is served
        ctx.set_radi_shifts("cycle")
        rc = ctx._lib.ricadi_ric_radi(ctx._h, dp(ms), ms.size, dp(B), B.shape[1], dp(np.ascontiguousarray(
            np.hstack([W] * 9)[:, :33])), 33, None, 1, 1e-10, 0, 1, 0, None, 0, C.byref(cc), None, dp(stats))
        assert rc == 0
        assert ctx.radi_shift_history().tolist() == [ms[0]]


def test_pru_returns_the_shifts_and_restores_the_mode():
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    backend.reset()
    try:
        f = forms(4)[0]
        out = pru.proj_alg_ric_radi(radi_dict=dict(ms="hamiltonian", radi_res_reltol=1e-8), **f["kw"])
        ctx = backend.context_for(f["calA"], f["calE"], f["J"])
        assert out["ms"][0] == adi_shifts.initial_shift(ctx.diag_ratio)
        assert len(out["ms"]) == out["radi_steps"] and out["shift_fallbacks"] == 0
        fb = pru.proj_alg_ric_radi(radi_dict=dict(ms="hamiltonian", ms_fallback=[-5.0, -50.0], radi_res_reltol=1e-8),
                                   **f["kw"])
        assert fb["ms"][0] == -5.0 and fb["stop_rule"] == _lib.RICADI_STOP_RES
        with pytest.raises(ValueError):
            pru.proj_alg_ric_radi(radi_dict=dict(ms="hamiltonian", ms_fallback=[-5.0, 1.0]), **f["kw"])
        with pytest.raises(ValueError):                                  # 33 columns: refused, and the mode restored
            pru.proj_alg_ric_radi(radi_dict=dict(ms="hamiltonian"), **dict(f["kw"], wmat=np.ones((ctx.nv, 33))))
        cyc = pru.proj_alg_ric_radi(radi_dict=dict(ms=f["ms"], radi_max_steps=12, radi_res_reltol=1e-30), **f["kw"])
        assert np.array_equal(ctx.radi_shift_history(), [f["ms"][j % len(f["ms"])] for j in range(12)])
        assert cyc["radi_steps"] == 12
    finally:
        backend.reset()
