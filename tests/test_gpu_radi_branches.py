"""GPU tests of the branches of the RADI driver (ric_radi_run, solver_radi.inl) that a converged X and K
cannot see -- the iteration converges to them with any negative shifts:

a. the shift of every step, the kept basis sizes and the step count against the NumPy model (tests/radi_shift_model.py),
   every call form: full rank, rank-deficient W (the dre forms: 8 columns, rank 4 -- the flag word of the block's
   CholQR2, the Householder QR and a second reduction, the ``keep`` subset), mw = 3;
b. forced fallbacks (ricadi_probe_radi_refuse): the fallback cycle's own counter, list shifts set up in the middle of
   the call, a generated shift after a fallback, what the per-shift cache holds afterwards, the same bits again;
c. recompression inside the call, also of a factor wider than it is tall;
d. HAMILTONIAN mode at mw = 17 and 32 (the driver's CholQR2 step had run at 4 and 8 columns only);
e. the breakdown flag of the factorisation kernel, at the probe (no non-finite data goes through a whole solve).

The problems are the N = 4 and N = 8 call forms (nv = 98 and 450): the smallest with a deficient W and a level hierarchy.
tests/test_radi_shift_cpu.py holds the model and the host selection; it has to pass for these to mean anything.
"""
import numpy as np
import pytest

import radi_model as rm
import radi_shift_model as sm
from optconpy_amd import _lib

pytestmark = pytest.mark.gpu
K_TOL = 1e-6          # the bars of tests/test_gpu_radi.py
X_TOL = 1e-6
PAIR_TOL = 1e-8       # two runs of the same iteration (test_gpu_radi.test_max_steps_stops_and_counts)
TOL = 1e-10           # res_reltol of every run here
MARGIN_MIN = 1.02     # smallest margin of a model run whose shifts are compared: the selection is well determined
# Largest relative deviation of the device's shifts from the model's per (N, form) at res_reltol = 1e-10, as measured on
# the MI355X; the tests assert ten times that and that the bound stays below 1e-3 (the margin covers
# the inexact solves' dependence on iteration counts; a flipped selection is an O(1) difference).
SHIFT_MEASURED = {
    (8, "steady"): 4.507e-10,
    (8, "dre"): 5.236e-11,
    (8, "dre_old"): 3.126e-10,
    (8, "narrow"): 1.322e-09,
    (4, "steady"): 3.905e-10,
    (4, "dre"): 4.775e-11,
    (4, "dre_old"): 3.837e-10,
}
KEPT = {"steady": 4, "narrow": 3, "dre": 4, "dre_old": 4}      # of 4, 3, 8, 8 columns
REFUSE = (2, 3, 6)


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def shift_bound(key):
    assert SHIFT_MEASURED[key] is not None, "no measurement recorded for %s" % (key,)
    bound = 10.0 * SHIFT_MEASURED[key]
    assert bound < 1e-3
    return bound


def shift_dev(a, b):
    """Largest relative deviation of the shifts a from b over the steps both have."""
    k = min(len(a), len(b))
    return float(np.max(np.abs(np.asarray(a[:k]) - np.asarray(b[:k])) / np.abs(b[:k])))


_forms, _models, _dense, _ctxs = {}, {}, {}, {}


def form(N, name):
    if N not in _forms:
        _forms[N] = {f["name"]: f for f in rm.call_forms(N) + rm.call_forms(N, narrow=True)}
    return _forms[N][name]


def p0_of(f):
    return sm.initial_shift(f["calA"], f["calE"])


def fallback_list(f):
    return [p0_of(f)] + [float(v) for v in f["ms"][:3]]


def model(N, name, fallback=None, refuse=(), W=None, max_steps=200):
    """The generated-shift model's run (computed once)."""
    f = form(N, name)
    fb = [p0_of(f)] if fallback is None else list(fallback)
    key = (N, name, tuple(fb), tuple(refuse), None if W is None else W.shape[1], max_steps)
    if key not in _models:
        _models[key] = sm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"] if W is None else W, fb, old=f["old"],
                               max_steps=max_steps, res_reltol=TOL, refuse=refuse)
    return _models[key]


def dense(N, name, W=None):
    """(X, cal E X B) of the dense solver for the form, or for the form with another W (computed once)."""
    key = (N, name, None if W is None else W.shape[1])
    if key not in _dense:
        f = form(N, name)
        _dense[key] = rm.dense_are_of(f if W is None else dict(f, W=W))
    return _dense[key]


def wide_w(N, mw):
    """mw random columns, seeded, scaled to ||W||_F of the steady form."""
    f = form(N, "steady")
    W = np.random.default_rng(1000 * N + mw).standard_normal((f["W"].shape[0], mw))
    return W * (np.linalg.norm(f["W"]) / np.linalg.norm(W))


@pytest.fixture(scope="module")
def ctx_of():
    """Contexts by (N, operator): the steady and narrow forms share one operator, the two dre forms the other."""
    def get(N, name):
        key = (N, "dre" if name.startswith("dre") else "steady")
        if key not in _ctxs:
            f = form(N, name)
            ctx = _lib.Context(0)
            ctx.set_operator(f["calA"], f["calE"], f["J"])
            _ctxs[key] = ctx
        return _ctxs[key]
    yield get
    for ctx in _ctxs.values():
        ctx.close()
    _ctxs.clear()


def run(ctx, f, shifts=None, mode="hamiltonian", W=None, max_steps=200, compress_cols=0):
    """One RADI call (the mode is restored): dict(Z, K, info, ms, fallbacks, kept, qr_repeats, recompressions, res)."""
    before = ctx.set_radi_shifts(mode)
    try:
        Z, K, info = ctx.ric_radi([p0_of(f)] if shifts is None else shifts, f["B"], f["W"] if W is None else W,
                                  oldB=f["old"], max_steps=max_steps, res_reltol=TOL, compress_cols=compress_cols)
    finally:
        ctx.set_radi_shifts(before)
    out = dict(Z=Z, K=K, info=info, ms=ctx.radi_shift_history(), fallbacks=ctx.radi_shift_fallbacks(),
               kept=ctx.probe_radi_kept(), res=np.asarray(ctx.adi_res_history()))
    out.update(ctx.probe_radi_counters())
    assert info["radi_steps"] == len(out["ms"]) == len(out["res"])
    return out


def check_solution(r, XK, what):
    X, K = XK
    ex, ek = rel(r["Z"] @ r["Z"].T, X), rel(r["K"], K)
    print("%s: rel X %.2e  rel K %.2e  gmres nonconverged %d" % (what, ex, ek, r["info"]["gmres_nonconverged"]))
    assert ex < X_TOL and ek < K_TOL, (what, ex, ek)
    assert r["info"]["gmres_nonconverged"] == 0
    assert r["info"]["stop_rule"] == "res"


# ------------------------------------------------------------------------- a. every step's shift against the model
@pytest.mark.parametrize("N,name", sorted(SHIFT_MEASURED, key=lambda k: (-k[0], k[1])))
def test_shifts_kept_and_steps_against_the_model(ctx_of, N, name):
    """Model steps 19 / 16 / 16 / 18 (N = 8: steady, dre, dre_old, narrow) and 13 / 13 (N = 4: dre, dre_old); smallest
    margins 1.062 / 1.030 / 1.026 / 1.120 and 1.227 / 1.234, N = 4 steady 1.037.  (N = 4 narrow, 1.008, is left out:
    its selection is not determined well enough to be compared.)"""
    f, mod = form(N, name), model(N, name)
    assert mod["margins"].min() >= MARGIN_MIN and mod["fallbacks"] == 0 and mod["stopped"] == "res"
    assert np.all(mod["kept"] == KEPT[name]) and len(mod["kept"]) == mod["steps"] - 1
    r = run(ctx_of(N, name), f)
    dev = shift_dev(r["ms"], mod["ms"])
    print("N = %d %-8s shifts against the model: largest relative deviation %.3e (device %d steps, model %d; smallest "
          "model margin %.3f), fallbacks %d, kept %s of %d, qr_repeats %d of %d selections" % (
              N, name, dev, len(r["ms"]), mod["steps"], mod["margins"].min(), r["fallbacks"],
              sorted(set(r["kept"].tolist())), f["W"].shape[1], r["qr_repeats"], len(r["kept"])))
    assert r["info"]["stop_rule"] == "res"
    assert abs(r["info"]["radi_steps"] - mod["steps"]) <= 1
    assert r["fallbacks"] == 0
    n = min(len(r["kept"]), len(mod["kept"]))
    assert len(r["kept"]) == r["info"]["radi_steps"] - 1             # one selection after every step but the last
    assert np.array_equal(r["kept"][:n], mod["kept"][:n]) and np.all(r["kept"] == KEPT[name])
    if name.startswith("dre"):
        # the deficiency puts the normalised pivot of the Gram matrix far below 1e-12 (the dependent columns are at
        # 1e-13 ... 4e-10 of the largest diagonal entry of R): the block's QR is repeated by Householder TSQR
        assert r["qr_repeats"] >= 1
    assert r["recompressions"] == 0
    assert dev <= shift_bound((N, name)), (dev, SHIFT_MEASURED[(N, name)])


# ----------------------------------------------------------------------------------------- b. forced fallbacks
@pytest.mark.parametrize("name", ["steady", "dre_old"])
def test_forced_fallbacks(name):
    """N = 8, refused selections after steps 2, 3 and 6, list [p0] + ms[:3].  Model: 21 and 19 steps, 3 fallbacks,
    smallest margin 1.048 / 1.049."""
    N = 8
    f = form(N, name)
    fb = fallback_list(f)
    mod = model(N, name, fallback=fb, refuse=REFUSE)
    assert mod["fallbacks"] == 3 and mod["margins"].min() >= MARGIN_MIN and mod["stopped"] == "res"
    assert (mod["ms"][2], mod["ms"][3], mod["ms"][6]) == (fb[1], fb[2], fb[3])
    with _lib.Context(0) as plain, _lib.Context(0) as ctx:
        for c in (plain, ctx):
            c.set_operator(f["calA"], f["calE"], f["J"])
        # a context that never has a refuse list: the same calls but for the refusals
        free = run(plain, f, shifts=fb)
        assert free["fallbacks"] == 0
        # what one shift adds to the cache (an entry per level): a shift of the form's list that the fallbacks do
        # not reach, in a CYCLE call of one step
        warm = run(ctx, f, shifts=fb)
        assert np.array_equal(warm["K"], free["K"]) and np.array_equal(warm["ms"], free["ms"])
        na = ctx.cache_entries()
        run(ctx, f, shifts=[float(f["ms"][3])], mode="cycle", max_steps=1)
        per_shift = ctx.cache_entries() - na
        assert per_shift >= 1
        n0 = ctx.cache_entries()
        ctx.probe_radi_refuse(REFUSE)
        r = run(ctx, f, shifts=fb)
        n1 = ctx.cache_entries()
        dev = shift_dev(r["ms"], mod["ms"])
        print("N = %d %-8s refused after %s: %d steps (model %d), fallbacks %d, shifts within %.3e of the model's, "
              "qr_repeats %d, cache entries %d -> %d (%d per shift)" % (
                  N, name, REFUSE, len(r["ms"]), mod["steps"], r["fallbacks"], dev, r["qr_repeats"], n0, n1, per_shift))
        assert r["fallbacks"] == 3
        assert (r["ms"][2], r["ms"][3], r["ms"][6]) == (fb[1], fb[2], fb[3])         # bitwise: entries 1, 2, 3
        assert abs(len(r["ms"]) - mod["steps"]) <= 1
        assert dev <= shift_bound((N, name)), (dev, SHIFT_MEASURED[(N, name)])
        assert np.all(r["kept"] == KEPT[name]) and len(r["kept"]) == len(r["ms"]) - 1    # refused ones were made too
        check_solution(r, dense(N, name), "N = %d %s with fallbacks" % (N, name))
        # the list entries that were used and not yet cached, and no more: fb[0] was there, the generated shifts that
        # follow a fallback leave nothing
        assert n1 == n0 + 3 * per_shift
        # the same call again: the same shifts and bits, nothing new in the cache
        r2 = run(ctx, f, shifts=fb)
        assert np.array_equal(r2["ms"], r["ms"]) and np.array_equal(r2["K"], r["K"]) and r2["fallbacks"] == 3
        assert ctx.cache_entries() == n1
        # cleared: the bits of the context that never had a list
        ctx.probe_radi_refuse(())
        r3 = run(ctx, f, shifts=fb)
        assert r3["fallbacks"] == 0 and ctx.cache_entries() == n1
        assert np.array_equal(r3["ms"], free["ms"]) and np.array_equal(r3["K"], free["K"])


def test_fallback_with_a_list_of_one(ctx_of):
    """N = 4, steady form, list [p0], refused after step 2: step 3 runs with p0 again and the cache is what it was.  A
    refusal listed at step == max_steps changes nothing: no selection is made there."""
    f = form(4, "steady")
    ctx = ctx_of(4, "steady")
    p0 = p0_of(f)
    free = run(ctx, f)
    n0 = ctx.cache_entries()
    try:
        ctx.probe_radi_refuse([2])
        r = run(ctx, f)
        print("N = 4 steady, list of one, refused after 2: %d steps (%d without), fallbacks %d" % (
            len(r["ms"]), len(free["ms"]), r["fallbacks"]))
        assert r["fallbacks"] == 1 and r["ms"][2] == p0 == r["ms"][0]
        assert r["ms"][1] == free["ms"][1] and r["ms"][2] != free["ms"][2]
        assert ctx.cache_entries() == n0
        check_solution(r, dense(4, "steady"), "N = 4 steady, list of one")
        ctx.probe_radi_refuse(())
        short = run(ctx, f, max_steps=5)
        ctx.probe_radi_refuse([5])
        last = run(ctx, f, max_steps=5)
        assert short["fallbacks"] == last["fallbacks"] == 0 and len(last["kept"]) == 4
        assert last["info"]["stop_rule"] == "max_steps"
        assert np.array_equal(last["ms"], free["ms"][:5]) and np.array_equal(last["ms"], short["ms"])
        assert np.array_equal(last["K"], short["K"])
    finally:
        ctx.probe_radi_refuse(())
    again = run(ctx, f)
    assert np.array_equal(again["ms"], free["ms"]) and np.array_equal(again["K"], free["K"])
    assert ctx.cache_entries() == n0


# ---------------------------------------------------------------------------- c. recompression inside the call
@pytest.mark.parametrize("case", ["cycle_m4", "ham_dre_m8", "ham_w32"])
def test_recompression_inside_the_call(ctx_of, case):
    """The factor is recompressed whenever compress_cols columns have been added since the last time; the iteration
    itself does not read Z (the block's QR is taken before), so the shifts, the residuals and K must not change, and
    Z Z^T only by the truncation.  ham_w32: 128 columns on 98 rows when it is first compressed."""
    max_steps = 60
    if case == "cycle_m4":
        name, mode, W, cc, shifts = "steady", "cycle", None, 8, form(4, "steady")["ms"]
    elif case == "ham_dre_m8":
        name, mode, W, cc, shifts = "dre", "hamiltonian", None, 16, None
    else:
        name, mode, W, cc, shifts = "steady", "hamiltonian", wide_w(4, 32), 128, None
    f = form(4, name)
    ctx = ctx_of(4, name)
    mw = f["W"].shape[1] if W is None else W.shape[1]
    ref = run(ctx, f, shifts=shifts, mode=mode, W=W, max_steps=max_steps, compress_cols=max_steps * mw + 1)
    r = run(ctx, f, shifts=shifts, mode=mode, W=W, max_steps=max_steps, compress_cols=cc)
    zz, zz0 = r["Z"] @ r["Z"].T, ref["Z"] @ ref["Z"].T
    print("%s: %d steps, recompressions %d, columns %d (uncompressed %d, %d rows), K within %.2e and Z Z^T within %.2e "
          "of the uncompressed run, fallbacks %d" % (case, len(r["ms"]), r["recompressions"], r["info"]["cols"],
                                                       ref["info"]["cols"], ctx.nv, rel(r["K"], ref["K"]),
                                                       rel(zz, zz0), r["fallbacks"]))
    assert ref["recompressions"] == 0 and ref["info"]["cols"] == len(ref["ms"]) * mw
    assert r["recompressions"] >= 2
    assert r["info"]["cols"] < ref["info"]["cols"] and r["Z"].shape[1] == r["info"]["cols"]
    if case == "ham_w32":
        assert 4 * mw > ctx.nv                         # wider than tall at the first recompression
    XK = dense(4, name, W)
    check_solution(ref, XK, case + " uncompressed")
    check_solution(r, XK, case)
    assert rel(r["K"], ref["K"]) < PAIR_TOL and rel(zz, zz0) < PAIR_TOL
    assert np.all(np.diff(r["res"]) < 0)
    assert len(r["ms"]) == len(ref["ms"])
    if mode == "hamiltonian":
        assert r["fallbacks"] == ref["fallbacks"] == 0
        assert shift_dev(r["ms"], ref["ms"]) <= shift_bound((4, name))
        assert np.array_equal(r["kept"], ref["kept"])
    else:
        assert np.array_equal(r["ms"], ref["ms"])


# ------------------------------------------------------------------------------------------------- d. widths
@pytest.mark.parametrize("N", [4, 8])
@pytest.mark.parametrize("mw", [17, 32])
def test_hamiltonian_widths(ctx_of, N, mw):
    """W of 17 and 32 random columns on the steady operator (model: 15 / 15 steps at N = 4, 19 / 18 at N = 8, no
    fallbacks; its margins go down to 1.004, so its shifts are not compared): the CholQR2 step of the driver at an odd width and at its limit."""
    f = form(N, "steady")
    ctx = ctx_of(N, "steady")
    W = wide_w(N, mw)
    r = run(ctx, f, W=W)
    cyc = run(ctx, f, shifts=f["ms"], mode="cycle", W=W)
    print("N = %d mw = %d: %d steps (cycled list %d), fallbacks %d, kept %s, qr_repeats %d" % (
        N, mw, len(r["ms"]), len(cyc["ms"]), r["fallbacks"], sorted(set(r["kept"].tolist())), r["qr_repeats"]))
    check_solution(r, dense(N, "steady", W), "N = %d mw = %d" % (N, mw))
    assert cyc["info"]["stop_rule"] == "res"
    assert len(r["ms"]) <= len(cyc["ms"])
    assert np.all(r["kept"] == mw) and len(r["kept"]) == len(r["ms"]) - 1
    assert np.all(r["ms"] < 0)


# ----------------------------------------------------------------------------- e. the breakdown flag, at the probe
def test_breakdown_flag_at_the_probe(ctx_of):
    """One NaN in B makes G = V^T B, and with it a pivot of I + G G^T, not finite: RICADI_EBREAKDOWN with the
    breakdown message, and the next call with clean inputs gives the bits it gave before."""
    import torch
    ctx = ctx_of(4, "steady")
    nv, m, nb, p = ctx.nv, 5, 3, -2.0
    rng = np.random.default_rng(11)
    V, B, RU = rng.standard_normal((nv, m)), 0.1 * rng.standard_normal((nv, nb)), rng.standard_normal((nv, m + nb))

    def dev(a):
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
        torch.cuda.synchronize()
        return t

    def call(Bh):
        Vd, Bd, RUd = dev(V), dev(Bh), dev(RU)
        Zd, Gd, Cd = dev(np.zeros((nv, m))), dev(np.zeros((m, nb))), dev(np.zeros((m, 2 * m + nb)))
        ctx.radi_update_dev(p, Vd.data_ptr(), m, m, Bd.data_ptr(), nb, RUd.data_ptr(), Zd.data_ptr(), m, 0,
                            Gd.data_ptr(), Cd.data_ptr())
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (Gd, Cd, RUd, Zd)]

    good = call(B)
    assert all(np.all(np.isfinite(a)) for a in good)
    Bn = B.copy()
    Bn[nv // 2, 1] = np.nan
    with pytest.raises(RuntimeError, match=r"error -4.*pivot that is not positive and finite"):
        call(Bn)
    again = call(B)
    for a, b in zip(good, again):
        assert np.array_equal(a, b)
