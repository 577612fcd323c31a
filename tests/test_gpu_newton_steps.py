"""The Newton-Kleinman driver (csrc/solver_newton.inl) step by step on the MI355X, against the dense FP64 model of
tests/newton_model.py:

a. the update norm (``ricadi_diff_zzt_fnorm_dev``) against the longdouble reference, shape by shape;
b. the argument contract of the new entry, of the two reporters and of the Newton entries' step limits;
c. the per-step history against the model's, with prefix runs that assert the premise of the bound;
d. the three stop rules;  e. a start from an iterate;  f. the sweep form and a recompression inside the ADI.

tests/test_newton_model_cpu.py holds the model to the dense solver and the allowance to NumPy's own distance from the
reference; it has to pass for these to mean anything.
"""
import ctypes as C

import numpy as np
import pytest

import newton_model as nm
import radi_model as rm
from optconpy_amd import _lib

pytestmark = pytest.mark.gpu
K_TOL = nm.K_TOL          # the project's parity bar (tests/test_gpu_small_ops.py, tests/test_gpu_radi.py)


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
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


# --------------------------------------------------------------------------------------------- a. the update norm
@pytest.fixture(scope="module")
def dims():
    """One dimension-only context for all shapes (ricadi_set_dims per shape)."""
    ctx = _lib.Context(0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("nv,k1,k0", nm.upd_shapes())
def test_update_norm_against_the_reference(dims, nv, k1, k0):
    """upd and x1 within UPD_FACTOR * UPD_DISTANCE * u (||Z1||_F^2 + ||Z0||_F^2) of the longdouble reference, for
    every kind of Z0 the shape has; inputs bitwise unchanged; a second call within the allowance of the first."""
    ctx = dims
    ctx.set_dims(nv)
    worst = 0.0
    for kind, Z1, Z0 in nm.upd_cases(nv, k1, k0):
        ref = nm.upd_reference(Z1, Z0)
        allow = nm.allowance(Z1, Z0)
        d1 = _dev(Z1)
        d0 = None if Z0 is None else _dev(Z0)
        p0 = None if d0 is None else d0.data_ptr()
        got = ctx.diff_zzt_fnorm_dev(d1.data_ptr(), k1, p0, k0)
        again = ctx.diff_zzt_fnorm_dev(d1.data_ptr(), k1, p0, k0)
        only_upd = ctx.diff_zzt_fnorm_dev(d1.data_ptr(), k1, p0, k0, want=(True, False))
        only_x1 = ctx.diff_zzt_fnorm_dev(d1.data_ptr(), k1, p0, k0, want=(False, True))
        eu, ex = abs(got[0] - ref[0]) / allow, abs(got[1] - ref[1]) / allow
        worst = max(worst, eu, ex)
        print("nv %4d k1 %3d k0 %3d %-12s upd %.6e (ref %.6e) error / allowance %.3f | x1 %.6e error / allowance %.3f"
              % (nv, k1, k0, kind, got[0], ref[0], eu, got[1], ex))
        assert np.array_equal(_host(d1), Z1) and (d0 is None or np.array_equal(_host(d0), Z0))
        assert np.isfinite(got[0]) and np.isfinite(got[1])          # the outputs were NaN before the call
        assert eu <= 1.0 and ex <= 1.0, (kind, eu, ex)
        assert abs(again[0] - got[0]) <= allow and abs(again[1] - got[1]) <= allow
        assert abs(only_upd[0] - got[0]) <= allow and np.isnan(only_upd[1])
        assert abs(only_x1[1] - got[1]) <= allow and np.isnan(only_x1[0])
    print("nv %4d k1 %3d k0 %3d: largest error / allowance %.3f" % (nv, k1, k0, worst))


# --------------------------------------------------------------------------------------------- b. the contract
def _raw_diff(ctx, p1, k1, p0, k0):
    upd, x1 = C.c_double(np.nan), C.c_double(np.nan)
    rc = ctx._lib.ricadi_diff_zzt_fnorm_dev(ctx._h, p1, k1, p0, k0, C.byref(upd), C.byref(x1))
    return rc, upd.value, x1.value


def test_update_norm_refusals(dims):
    ctx = dims
    fresh = _lib.Context(0)
    try:
        z = _dev(np.ones((5, 3)))
        rc, u, x = _raw_diff(fresh, z.data_ptr(), 3, None, 0)
        assert rc == -5 and np.isnan(u) and np.isnan(x)                     # RICADI_ESTATE: no dimensions
    finally:
        fresh.close()
    ctx.set_dims(5)
    p = z.data_ptr()
    lim = _lib.MAX_UPD_COLS
    assert lim == nm.UPD_WIDTH_LIMIT
    for args in ((p, 0, None, 0), (p, -1, p, 3), (p, 3, p, -1), (None, 3, None, 0), (p, 3, None, 2),
                 (p, lim, p, 1), (p, 1, p, lim), (p, lim + 1, None, 0), (p, 2 ** 31 - 1, p, 2 ** 31 - 1)):
        rc, u, x = _raw_diff(ctx, *args)
        assert rc == -1 and np.isnan(u) and np.isnan(x), args                # RICADI_EINVAL, outputs untouched
    with pytest.raises(ValueError):
        ctx.diff_zzt_fnorm_dev(p, 0, None, 0)
    # a NULL second panel with k0 = 0 and a pointer with k0 = 0 are both the one-factor call
    a = ctx.diff_zzt_fnorm_dev(p, 3, None, 0)
    b = ctx.diff_zzt_fnorm_dev(p, 3, p, 0)
    assert a[0] == a[1] and abs(a[0] - b[0]) <= nm.allowance(np.ones((5, 3)))
    assert abs(a[0] - 15.0) <= nm.allowance(np.ones((5, 3)))                # ||1 1^T||_F of a 5 x 3 panel of ones


_forms = {}


def forms(N):
    if N not in _forms:
        _forms[N] = rm.call_forms(N)
    return _forms[N]


_cases = {}


def case(N, i, G):
    """The model's run of a history case: live at N = 4, from the fixture at N = 8."""
    key = (N, i, G)
    if key not in _cases:
        _cases[key] = nm.live_case(N, i, G) if N == 4 else nm.unpack(np.load(nm.GOLDEN), nm.case_key(N, i, G))
    return _cases[key]


@pytest.fixture(scope="module")
def ctxs():
    """Contexts per (N, form), made on demand and closed with the module."""
    made = {}

    def get(N, i):
        if (N, i) not in made:
            f = forms(N)[i]
            ctx = _lib.Context(0)
            ctx.set_operator(f["calA"], f["calE"], f["J"])
            made[(N, i)] = ctx
        return made[(N, i)]
    yield get
    for ctx in made.values():
        ctx.close()


def _params(cs, G=1, **over):
    d = dict(adi_max_steps=nm.ADI_MAX_STEPS, adi_newZ_reltol=cs["newZ_reltol"], nwtn_max_steps=6,
             nwtn_upd_reltol=cs["nwtn_upd_reltol"], nwtn_upd_abstol=0.0, sweep_width=G)
    d.update(over)
    return _lib.adi_params(d)


def _run(ctx, f, prm, Z0=None, **kw):
    return ctx.ric_newtonadi(f["ms"], f["B"], f["W"], prm, Z0=Z0, oldB=f["old"], **kw)


def test_newton_refuses_step_limits_below_one(ctxs):
    """One good call, then nwtn_max_steps = 0 and adi_max_steps = 0 through both entries: RICADI_EINVAL, and the
    factor, the Newton history and the ADI's residual history are bitwise what they were."""
    import torch
    ctx, f, cs = ctxs(4, 0), forms(4)[0], case(4, 0, 1)
    fresh = _lib.Context(0)
    try:
        fresh.set_operator(f["calA"], f["calE"], f["J"])
        for bad in (dict(nwtn_max_steps=0), dict(adi_max_steps=0)):          # refused on a context without a factor too
            with pytest.raises(ValueError):
                _run(fresh, f, _params(cs, **bad))
        with pytest.raises(RuntimeError):
            fresh.newton_history()                                           # RICADI_ESTATE: no Newton call yet
    finally:
        fresh.close()
    ctx.set_adi_res_history(True)
    try:
        _run(ctx, f, _params(cs, nwtn_max_steps=2))
        before = (ctx.factor_get(), ctx.newton_history(), ctx.adi_res_history(), ctx.newton_stopped_by(),
                  ctx.adi_stopped_by())
        assert before[1].shape == (2, 6) and before[2].size > 0
        Bt, Wt = _dev(f["B"]), _dev(f["W"])
        for bad in (dict(nwtn_max_steps=0), dict(adi_max_steps=0), dict(nwtn_max_steps=-3)):
            with pytest.raises(ValueError):
                _run(ctx, f, _params(cs, **bad))
            with pytest.raises(ValueError):
                ctx.ric_newtonadi_dev(f["ms"], Bt, Wt, _params(cs, **bad))
            after = (ctx.factor_get(), ctx.newton_history(), ctx.adi_res_history(), ctx.newton_stopped_by(),
                     ctx.adi_stopped_by())
            assert all(np.array_equal(a, b) for a, b in zip(before[:3], after[:3])) and before[3:] == after[3:], bad
        torch.cuda.synchronize()
    finally:
        ctx.set_adi_res_history(False)


def test_history_cap_and_forgetting(ctxs):
    """cap below the step count fills cap rows and reports the full count; ricadi_clear_cache keeps the reporters,
    a replaced operator forgets them."""
    ctx, f, cs = ctxs(4, 1), forms(4)[1], case(4, 1, 1)
    _, plain = _run(ctx, f, _params(cs))
    assert "upd_hist" not in plain and "nwtn_stopped_by" not in plain
    [float(v) for v in plain.values() if not isinstance(v, str)]       # numbers and strings only, as callers rely on
    _, info = _run(ctx, f, _params(cs), upd_hist=True)
    full = ctx.newton_history()
    n = len(cs["steps"])
    assert full.shape == (n, 6) and n >= 2
    part, count = ctx.newton_history(cap=1)
    assert count == n and part.shape == (1, 6) and np.array_equal(part[0], full[0])
    none, count = ctx.newton_history(cap=0)
    assert count == n and none.shape == (0, 6)
    more, count = ctx.newton_history(cap=n + 3)
    assert count == n and np.array_equal(more, full)
    # the raw entry leaves the rows beyond cap alone
    buf = np.full((n, 6), -7.0)
    cnt = C.c_int(0)
    assert ctx._lib.ricadi_newton_history(ctx._h, _lib._d(buf), 1, C.byref(cnt)) == 0
    assert cnt.value == n and np.array_equal(buf[0], full[0]) and np.all(buf[1:] == -7.0)
    assert np.array_equal(info["upd_hist"], full) and info["nwtn_stopped_by"] == ctx.newton_stopped_by()
    ctx.clear_cache()
    assert np.array_equal(ctx.newton_history(), full) and ctx.newton_stopped_by() == "reltol"
    ctx.set_operator(f["calA"], f["calE"], f["J"])
    with pytest.raises(RuntimeError):
        ctx.newton_history()
    with pytest.raises(RuntimeError):
        ctx.newton_stopped_by()


# --------------------------------------------------------------------------------------------- c. the history
def _bar_against(Z, step):
    """||Z Z^T - X_model||_F / ||X_model||_F and the bar it is held to: K_TOL less the error the kept iterate was
    truncated with (the triangle inequality then gives K_TOL against the model's own iterate)."""
    return nm.upd_float64_qr(np.asarray(Z), step["Z"])[0] / step["x1"], K_TOL - step["trunc"]


def _check_history(name, hist, steps, nv, first_has_iterate=False, recompressed=False):
    """Rows of a device history against the model's steps (the bound of c)."""
    assert hist.shape == (len(steps), 6), (hist.shape, len(steps))
    for k, (row, s) in enumerate(zip(hist, steps)):
        upd, upd_rel, adi, raw, kept, x1 = row
        print("%s step %d: ADI steps %d (model %d), columns %d -> %d, x1 %.9e (model %.9e), upd %.6e (model %.6e), "
              "upd_rel %.3e (model %.3e), |upd - model| / (2 K_TOL x1) %.3e"
              % (name, k + 1, adi, s["adi_steps"], raw, kept, x1, s["x1"], upd, s["upd"], upd_rel, s["upd_rel"],
                 abs(upd - s["upd"]) / (2 * K_TOL * s["x1"])))
        assert adi == s["adi_steps"]
        if recompressed:
            assert raw < adi * s["width"]
        else:
            assert raw == adi * s["width"]
        assert 1 <= kept <= min(raw, nv)
        assert abs(x1 - s["x1"]) <= 1e-8 * s["x1"]
        assert abs(upd - s["upd"]) <= 2 * K_TOL * s["x1"]
        assert upd_rel == upd / x1


@pytest.mark.parametrize("N,i,G", [c for c in nm.HISTORY_CASES if c[2] == 1])
def test_history_against_the_model(ctxs, N, i, G):
    """Step form.  The bound on upd is the triangle inequality over two iterates that each meet K_TOL against the
    model's; the prefix runs (nwtn_max_steps = k) assert that premise for every k."""
    ctx, f, cs = ctxs(N, i), forms(N)[i], case(N, i, G)
    name, steps = nm.case_key(N, i, G), cs["steps"]
    last = len(steps)
    for k in range(1, last):
        Z, info = _run(ctx, f, _params(cs, nwtn_max_steps=k))
        err, bar = _bar_against(Z, steps[k - 1])
        print("%s prefix %d: ||Z Z^T - X_model|| / ||X_model|| %.3e (bar %.3e)" % (name, k, err, bar))
        assert info["nwtn_steps"] == k and ctx.newton_stopped_by() == "max_steps"
        assert ctx.newton_history().shape == (k, 6)
        assert err <= bar
    Z, info = _run(ctx, f, _params(cs))
    hist = ctx.newton_history()
    _check_history(name, hist, steps, ctx.nv)
    err, bar = _bar_against(Z, steps[-1])
    print("%s whole call: %d steps, stopped by %s, ||Z Z^T - X_model|| / ||X_model|| %.3e (bar %.3e)"
          % (name, info["nwtn_steps"], ctx.newton_stopped_by(), err, bar))
    assert err <= bar
    assert info["nwtn_steps"] == last and ctx.newton_stopped_by() == "reltol"
    assert info["upd_abs"] == hist[-1, 0] and info["upd_rel"] == hist[-1, 1]
    assert info["adi_steps"] == int(hist[:, 2].sum()) and info["cols"] == int(hist[-1, 4])
    assert info["gmres_nonconverged"] == 0


# --------------------------------------------------------------------------------------------- d. the stop rules
@pytest.fixture(scope="module")
def free5():
    """The model's five steps on the N = 4 steady form with the case's ADI tolerance and no Newton tolerance."""
    cs = case(4, 0, 1)
    run = nm.newton(forms(4)[0], newZ_reltol=cs["newZ_reltol"], nwtn_max_steps=5, nwtn_upd_reltol=0.0,
                    nwtn_upd_abstol=0.0)
    assert [s["adi_steps"] for s in run["steps"][:3]] == [s["adi_steps"] for s in cs["steps"]]
    return run["steps"]


@pytest.mark.parametrize("rule", ["abstol", "reltol"])
def test_stop_rule_tolerances(ctxs, free5, rule):
    """The tolerance at the geometric middle of the model's values at steps 2 and 3, the other one 0: three steps."""
    ctx, f, cs = ctxs(4, 0), forms(4)[0], case(4, 0, 1)
    key = "upd" if rule == "abstol" else "upd_rel"
    tol = float(np.sqrt(free5[1][key] * free5[2][key]))
    assert free5[1][key] >= 10 * tol and free5[2][key] * 10 <= tol
    over = dict(nwtn_upd_abstol=tol, nwtn_upd_reltol=0.0) if rule == "abstol" else dict(nwtn_upd_reltol=tol)
    _, info = _run(ctx, f, _params(cs, **over))
    hist = ctx.newton_history()
    print("%s %.3e: %d steps, stopped by %s, last row %s" % (rule, tol, info["nwtn_steps"], ctx.newton_stopped_by(),
                                                              hist[-1]))
    assert info["nwtn_steps"] == 3 and hist.shape == (3, 6) and ctx.newton_stopped_by() == rule
    col = 0 if rule == "abstol" else 1
    assert hist[1, col] >= tol > hist[2, col]


def test_stop_rule_both_fire_reports_abstol(ctxs, free5):
    ctx, f, cs = ctxs(4, 0), forms(4)[0], case(4, 0, 1)
    ta = float(np.sqrt(free5[1]["upd"] * free5[2]["upd"]))
    tr = float(np.sqrt(free5[1]["upd_rel"] * free5[2]["upd_rel"]))
    _, info = _run(ctx, f, _params(cs, nwtn_upd_abstol=ta, nwtn_upd_reltol=tr))
    hist = ctx.newton_history()
    assert info["nwtn_steps"] == 3 and hist[2, 0] < ta and hist[2, 1] < tr and ctx.newton_stopped_by() == "abstol"


def test_stop_rule_max_steps(ctxs, free5):
    ctx, f, cs = ctxs(4, 0), forms(4)[0], case(4, 0, 1)
    _, info = _run(ctx, f, _params(cs, nwtn_max_steps=2, nwtn_upd_reltol=0.0, nwtn_upd_abstol=0.0))
    assert info["nwtn_steps"] == 2 and ctx.newton_history().shape == (2, 6) and ctx.newton_stopped_by() == "max_steps"
    _check_history("max_steps = 2", ctx.newton_history(), free5[:2], ctx.nv)


def test_extra_steps_do_not_drift(ctxs, free5):
    """Both tolerances 0, five steps: from the step where the model's relative update is below K_TOL the device's
    is at most 2 K_TOL, and the last factor still meets K_TOL against the dense solution."""
    ctx, f, cs = ctxs(4, 0), forms(4)[0], case(4, 0, 1)
    Z, info = _run(ctx, f, _params(cs, nwtn_max_steps=5, nwtn_upd_reltol=0.0, nwtn_upd_abstol=0.0))
    hist = ctx.newton_history()
    assert info["nwtn_steps"] == 5 and hist.shape == (5, 6) and ctx.newton_stopped_by() == "max_steps"
    small = [k for k, s in enumerate(free5) if s["upd_rel"] < K_TOL]
    assert small and small[0] == 2 and small == list(range(2, 5))
    for k in range(5):
        print("step %d: device upd_rel %.3e, model %.3e, ADI steps %d (model %d)"
              % (k + 1, hist[k, 1], free5[k]["upd_rel"], hist[k, 2], free5[k]["adi_steps"]))
    assert np.all(hist[2:, 1] <= 2 * K_TOL)
    _check_history("five steps", hist[:3], free5[:3], ctx.nv)
    X, _ = rm.dense_are_of(f)
    err = np.linalg.norm(Z @ Z.T - X) / np.linalg.norm(X)
    print("after five steps: Z Z^T against the dense solution %.3e" % err)
    assert err <= K_TOL


# --------------------------------------------------------------------------------------------- e. from an iterate
@pytest.mark.parametrize("i", [0, 2])
def test_start_from_an_iterate(ctxs, i):
    """Z0 = the factor of a one-step run: the rows of the history are rows 2.. of the plain run's, within the bound
    of c, with one step less (i = 2: with the old gain of the 'dre_old' form)."""
    ctx, f, cs = ctxs(4, i), forms(4)[i], case(4, i, 1)
    assert (f["old"] is not None) == (i == 2)
    steps = cs["steps"]
    Z1, _ = _run(ctx, f, _params(cs, nwtn_max_steps=1))
    Z1 = np.array(Z1)
    _, plain = _run(ctx, f, _params(cs))
    hp = ctx.newton_history()
    _, info = _run(ctx, f, _params(cs), Z0=Z1)
    h = ctx.newton_history()
    assert info["nwtn_steps"] == plain["nwtn_steps"] - 1 == len(steps) - 1 and ctx.newton_stopped_by() == "reltol"
    _check_history(nm.case_key(4, i, 1) + " from Z_1", h, steps[1:], ctx.nv)
    for a, b, s in zip(h, hp[1:], steps[1:]):
        assert a[2] == b[2] and a[3] == b[3]
        assert abs(a[0] - b[0]) <= 2 * K_TOL * s["x1"] and abs(a[5] - b[5]) <= 1e-8 * s["x1"]


# --------------------------------------------------------------------------------------------- f. sweeps, recompression
def test_sweep_form_history(ctxs):
    """N = 8, sweep_width = 4: the ADI step counts are those adi_sweep_model.sweep_schedule predicts."""
    (N, i, G), = [c for c in nm.HISTORY_CASES if c[2] > 1]
    ctx, f, cs = ctxs(N, i), forms(N)[i], case(N, i, G)
    Z, info = _run(ctx, f, _params(cs, G=G))
    hist = ctx.newton_history()
    _check_history(nm.case_key(N, i, G), hist, cs["steps"], ctx.nv)
    assert info["adi_sweeps"] >= int(np.ceil(hist[:, 2] / G).sum()) and ctx.newton_stopped_by() == "reltol"
    err, bar = _bar_against(Z, cs["steps"][-1])
    print("sweep form: ||Z Z^T - X_model|| / ||X_model|| %.3e (bar %.3e)" % (err, bar))
    assert err <= bar


def test_recompression_inside_the_adi(ctxs):
    """compress_cols = 64 on the N = 4 steady form: the ADI recompresses its factor inside every Newton step (the
    raw-column entry is below steps x width) and the history is still the model's."""
    ctx, f, cs = ctxs(4, 0), forms(4)[0], case(4, 0, 1)
    Z, info = _run(ctx, f, _params(cs, compress_cols=64))
    hist = ctx.newton_history()
    _check_history("compress_cols 64", hist, cs["steps"], ctx.nv, recompressed=True)
    err, bar = _bar_against(Z, cs["steps"][-1])
    assert err <= bar and ctx.newton_stopped_by() == "reltol"
