"""GPU tests of the sweep form of RADI (ricadi_radi.hip, csrc/solver_radi.inl,
``radi_dict['sweep_width']`` of pru.proj_alg_ric_radi).

1. the recombination kernel (ricadi_radi_sweep_combine_dev) entry by entry against the longdouble model of
   tests/radi_sweep_model.py;
2. the whole solve at widths 2, 4, 8 against SciPy's dense Riccati solver and against the sequential device run;
3. the solves really are batched (counters), and a sweep cut by the residual keeps a prefix;
4. the batch at its limits (G m = 128; a 62-column panel);
5. contract and hygiene;  6. a two-step DRE sweep through solve_flow_daeric.

tests/test_radi_sweep_cpu.py holds the model and the host entries; it has to pass for these to mean anything.
"""
import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spsla

import dense_model as dm
import radi_dominant_model as rdm
import radi_model as rm
import radi_sweep_model as swm
from optconpy_amd import _lib, backend, problems as pb

pytestmark = pytest.mark.gpu
K_TOL = 1e-6          # the project's parity bar (tests/test_gpu_radi.py)
# Measured on the MI355X over the whole solves below (widths 2, 4, 8; the three call forms at N = 4 and 8; the four
# limit cases): the largest relative deviation of the residual history from the SEQUENTIAL DEVICE run's over the
# entries above 1e-6, and the largest relative deviation of the gain from that run's.  The tests assert ten times
# these; the gain bar is never looser than 1e-7.  Both runs solve to gmres_tol = 1e-10, so deviations of that order
# are the solves', not the recombination's.
HIST_MEASURED = 9.956e-08
GAIN_MEASURED = 4.515e-09
# ... and of the DRE sweep's gains and w against the same call at width 1
DRE_MEASURED = 6.864e-10


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def gain_bar():
    assert GAIN_MEASURED is not None, "no measurement recorded"
    return min(10.0 * GAIN_MEASURED, 1e-7)


def hist_bar():
    assert HIST_MEASURED is not None, "no measurement recorded"
    return 10.0 * HIST_MEASURED


_dense = {}


def dense(N, i):
    if (N, i) not in _dense:
        _dense[(N, i)] = rm.dense_are_of(swm.forms(N)[i])
    return _dense[(N, i)]


def _ctx(N):
    f = swm.forms(N)[0]
    ctx = _lib.Context(0)
    ctx.set_operator(f["calA"], f["calE"], f["J"])
    return ctx, f


@pytest.fixture(scope="module")
def ctx4():
    ctx, f = _ctx(4)
    yield ctx, f
    ctx.close()


@pytest.fixture(scope="module")
def ctx8():
    ctx, f = _ctx(8)
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


# ------------------------------------------------------------------------------------------- 1. the recombination
SHAPES = [(2, 1, 1, 2), (3, 5, 2, 2), (8, 16, 8, 8), (8, 16, 8, 5), (2, 58, 4, 2), (2, 64, 64, 1)]      # (G, m, nb, k)


def _combine_inputs(nv, n, G, m, nb, k, wide_v, integer):
    """The G solution panels inside panels of n rows (pressure rows NaN: they must not be read) of width ldv, S, a
    DENSE coefficient matrix (also the rows the driver's Cf has zero), the panel [R | U]."""
    rng = np.random.default_rng(100000 * G + 1000 * m + 10 * nb + k)
    draw = (lambda *s: rng.integers(-3, 4, size=s).astype(float)) if integer else (lambda *s: rng.standard_normal(s))
    ldv = m + nb if wide_v else m
    Vp = np.full((G, n, ldv), np.nan)
    Vp[:, :nv] = draw(G, nv, ldv)
    Vh = np.hstack([Vp[g, :nv, :m] for g in range(G)])
    return Vp, ldv, Vh, draw(nv, G * m), draw(G * m, k * m + m + nb), draw(nv, m + nb)


def _run_combine(ctx, G, m, nb, k, Vp, ldv, S, Cf, RU, zoff, ldz):
    nv, n = ctx.nv, ctx.n
    Vd, Sd, Cd = _dev(Vp), _dev(S), _dev(Cf)
    RUd = _dev(np.stack([RU, RU]))              # the second panel is a guard
    Zd = _dev(np.full((nv, ldz), np.nan))
    ctx.radi_sweep_combine_dev(G, Vd.data_ptr(), n * ldv, ldv, m, Sd.data_ptr(), Cd.data_ptr(), k, nb,
                               RUd.data_ptr(), Zd.data_ptr(), ldz, zoff)
    return _host(RUd), _host(Zd)


@pytest.mark.parametrize("wide_v", [False, True])
@pytest.mark.parametrize("G,m,nb,k", SHAPES)
@pytest.mark.parametrize("N", [4, 8])
def test_combine_entry_by_entry(ctx4, ctx8, N, G, m, nb, k, wide_v):
    """Z block and the new [R | U] against the longdouble model at bound(2^-53) + bound(u_longdouble); columns of Z
    outside the block and a guard panel untouched; the same call twice bitwise; small-integer inputs exactly.
    NV = 98 and 450 (both leave a ragged last 16-row chunk); both leading dimensions of the solution panels."""
    ctx, _ = ctx4 if N == 4 else ctx8
    nv, n, km = ctx.nv, ctx.n, k * m
    assert nv == (98 if N == 4 else 450) and nv % 16 != 0
    zoff, ldz = (5, km + 12) if wide_v else (0, km)
    Vp, ldv, Vh, S, Cf, RU = _combine_inputs(nv, n, G, m, nb, k, wide_v, False)
    Zb, RUn = swm.combine(Vh, S, Cf, k, m, RU)
    tZ, tRU = dm.tol(swm.combine_bounds, Vh, S, Cf, k, m, RU)
    RUh, Zh = _run_combine(ctx, G, m, nb, k, Vp, ldv, S, Cf, RU, zoff, ldz)
    ratios = dict(Z=dm.ratio(Zh[:, zoff:zoff + km], Zb, tZ), RU=dm.ratio(RUh[0], RUn, tRU))
    print("N %d G %d m %d nb %d k %d ldv %d: error / bound " % (N, G, m, nb, k, ldv) +
          "  ".join("%s %.3g" % kv for kv in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    assert np.array_equal(RUh[1], RU)
    guard = np.ones(ldz, dtype=bool)
    guard[zoff:zoff + km] = False
    assert np.all(np.isnan(Zh[:, guard])) and not np.any(np.isnan(Zh[:, ~guard]))
    RU2, Z2 = _run_combine(ctx, G, m, nb, k, Vp, ldv, S, Cf, RU, zoff, ldz)
    assert np.array_equal(RU2, RUh) and np.array_equal(Z2, Zh, equal_nan=True)          # bitwise
    # small integers: every product and sum is exact in FP64
    Vp, ldv, Vh, S, Cf, RU = _combine_inputs(nv, n, G, m, nb, k, wide_v, True)
    RUh, Zh = _run_combine(ctx, G, m, nb, k, Vp, ldv, S, Cf, RU, zoff, ldz)
    assert np.array_equal(Zh[:, zoff:zoff + km], Vh @ Cf[:, :km]) and np.array_equal(RUh[0], RU + S @ Cf[:, km:])


def test_combine_contract(ctx4):
    ctx, _ = ctx4
    nv, n = ctx.nv, ctx.n
    V, S, Cf, RU, Z = _dev(np.zeros((2, n, 4))), _dev(np.zeros((nv, 8))), _dev(np.zeros((8, 16))), \
        _dev(np.zeros((nv, 8))), _dev(np.zeros((nv, 8)))
    ok = dict(G=2, vstride=n * 4, ldv=4, m=4, k=2, nb=4, ldz=8, zoff=0)
    for kw in (dict(G=0), dict(G=17), dict(m=65), dict(k=0), dict(k=3), dict(nb=0), dict(nb=65), dict(ldv=3),
               dict(ldz=7), dict(zoff=1), dict(vstride=nv * 4 - 1)):
        a = dict(ok, **kw)
        with pytest.raises(ValueError):
            ctx.radi_sweep_combine_dev(a["G"], V.data_ptr(), a["vstride"], a["ldv"], a["m"], S.data_ptr(),
                                       Cf.data_ptr(), a["k"], a["nb"], RU.data_ptr(), Z.data_ptr(), a["ldz"], a["zoff"])


# ------------------------------------------------------------------------------------------- 2. the whole solve
def _against_sequential(name, seq, out, width, want_width):
    """The bars of a sweep run against the sequential device run; returns (history deviation, gain deviation)."""
    k = min(len(out["res_hist"]), len(seq["res_hist"]))
    big = seq["res_hist"][:k] > 1e-6
    hd = float(np.max(np.abs(out["res_hist"][:k][big] - seq["res_hist"][:k][big]) / seq["res_hist"][:k][big]))
    gd = rel(out["gain"], seq["gain"])
    print("%-14s width %d: steps %d (sequential %d) solves %d  history %.3e over %d entries  gain %.3e" % (
        name, width, out["radi_steps"], seq["radi_steps"], out["shift_solves"], hd, big.sum(), gd))
    assert big.sum() >= 5, name
    assert out["sweep_width"] == want_width and seq["sweep_width"] == 1 and seq["sweeps"] == 0, name
    assert abs(out["radi_steps"] - seq["radi_steps"]) <= 1, (name, out["radi_steps"], seq["radi_steps"])
    assert len(out["res_hist"]) == out["radi_steps"], name
    assert out["radi_steps"] <= out["shift_solves"] <= out["radi_steps"] + want_width - 1, name
    assert out["sweeps"] == -(-out["shift_solves"] // want_width), name
    assert out["gmres_nonconverged"] == 0 and seq["gmres_nonconverged"] == 0, name
    assert out["stop_rule"] == seq["stop_rule"], name
    return hd, gd


@pytest.mark.parametrize("i", [0, 1, 2])
@pytest.mark.parametrize("N", [4, 8])
def test_sweeps_vs_dense_are_and_sequential(N, i):
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    f = swm.forms(N)[i]
    X, K = dense(N, i)
    mw, nb = f["W"].shape[1], f["B"].shape[1]
    backend.reset()
    try:
        d = dict(ms=f["ms"], radi_res_reltol=1e-12, radi_max_steps=200)
        seq = pru.proj_alg_ric_radi(radi_dict=d, **f["kw"])
        worst = []
        for w in (2, 4, 8):
            eff = _lib.host_radi_sweep_width(f["ms"], mw, nb, w, 200)
            assert eff == w                       # every width is admitted for these lists
            out = pru.proj_alg_ric_radi(radi_dict=dict(d, sweep_width=w), **f["kw"])
            Z = out["zfac"]
            ex, ek = rel(Z @ Z.T, X), rel(out["gain"], K)
            print("N = %d %-8s width %d: rel X %.2e  rel K %.2e" % (N, f["name"], w, ex, ek))
            assert ex < 1e-6 and ek < K_TOL, (f["name"], w, ex, ek)
            assert Z.shape[1] == out["radi_steps"] * mw and out["stop_rule"] == _lib.RICADI_STOP_RES
            worst.append(_against_sequential("N%d %s" % (N, f["name"]), seq, out, w, eff))
        hd, gd = max(h for h, _ in worst), max(g for _, g in worst)
        assert gd <= gain_bar() and hd <= hist_bar(), (hd, gd)
    finally:
        backend.reset()


# ------------------------------------------------------------------------------------------- 3. really batched
def test_sweeps_batch_the_solves(ctx4):
    """Fails without the feature: eight steps at width 4 are TWO calls of the batched solve, not eight."""
    ctx, f = ctx4
    mw = f["W"].shape[1]
    assert ctx.set_radi_sweep_width(4) == 1
    try:
        t0 = ctx.solve_trace()
        Z, K, info = ctx.ric_radi(f["ms"], f["B"], f["W"], max_steps=8, res_reltol=1e-14)
        t1 = ctx.solve_trace()
        hist = ctx.adi_res_history()
        assert t1["solves"] - t0["solves"] == 2 + 1          # two sweeps and the projection
        assert t1["smw_dup"] - t0["smw_dup"] == 1            # the first sweep's U is zero: plain operator
        assert ctx.radi_sweep_info() == dict(width=4, sweeps=2, solves=8)
        assert info["shift_solves"] == 8 and info["radi_steps"] == 8 and info["stop_rule"] == "max_steps"
        assert Z.shape == (ctx.nv, 8 * mw) and len(hist) == 8 and np.all(np.diff(hist) < 0)
        assert np.array_equal(ctx.radi_shift_history(), np.asarray(f["ms"][:8]))
        # the residual rule inside the first sweep: three blocks kept, four solves issued
        assert hist[1] > 1.01 * hist[2]
        Z2, K2, info2 = ctx.ric_radi(f["ms"], f["B"], f["W"], max_steps=8, res_reltol=1.01 * hist[2])
        assert info2["radi_steps"] == 3 and info2["stop_rule"] == "res" and info2["shift_solves"] == 4
        assert ctx.radi_sweep_info() == dict(width=4, sweeps=1, solves=4)
        assert Z2.shape == (ctx.nv, 3 * mw) and len(ctx.adi_res_history()) == 3
        assert np.array_equal(ctx.radi_shift_history(), np.asarray(f["ms"][:3]))
        assert rel(Z2 @ Z2.T, Z[:, :3 * mw] @ Z[:, :3 * mw].T) < 1e-8
        # a sweep cut by max_steps: 4 + 2
        _, _, info3 = ctx.ric_radi(f["ms"], f["B"], f["W"], max_steps=6, res_reltol=1e-14)
        assert info3["radi_steps"] == 6 and info3["shift_solves"] == 6
        assert ctx.radi_sweep_info() == dict(width=4, sweeps=2, solves=6)
    finally:
        ctx.set_radi_sweep_width(1)


# ------------------------------------------------------------------------------------------- 4. the limits
@pytest.mark.parametrize("case", ["gm128", "wide62", "groups16", "groups12"])
def test_batch_at_its_limits(ctx8, case):
    """mw = 16, nb = 8, G = 8: G m = 128, the widest coefficient matrix (W and B standard normals: the ten shifts of the
    list do not bring that equation to 1e-12, so both runs make the same 40 steps, five full sweeps); mw = 58, nb = 4,
    G = 2: a 62-column panel, four sixteen-column groups per shift, to the residual rule.  The batch at SIXTEEN
    groups: mw = nb = 8 at width 16 on a 16-shift list (G m = 128, one 16-column group per shift), 32 steps; and twelve
    groups of a split panel: mw = 30, nb = 10 at width 4 (three groups per shift), 24 steps.  Against the sequential
    device run."""
    ctx, f = ctx8
    rng = np.random.default_rng(11)
    if case == "gm128":
        W, B, want, steps = rng.standard_normal((ctx.nv, 16)), rng.standard_normal((ctx.nv, 8)), 8, 40
    elif case == "wide62":
        W, B, want, steps = rdm.wide_w(ctx.nv, 58), f["B"], 2, 200
    elif case == "groups16":
        W, B, want, steps = rng.standard_normal((ctx.nv, 8)), rng.standard_normal((ctx.nv, 8)), 16, 32
    else:
        W, B, want, steps = rdm.wide_w(ctx.nv, 30), rng.standard_normal((ctx.nv, 10)), 4, 24
    ms = pb.logshifts(1.0, 1e4, 16) if case == "groups16" else f["ms"]
    mw, nb = W.shape[1], B.shape[1]
    assert _lib.host_radi_sweep_width(ms, mw, nb, 16, 200) == want
    assert want * swm.panel_groups(mw, nb) == dict(gm128=8, wide62=8, groups16=16, groups12=12)[case]
    runs = {}
    for w in (1, 16):
        ctx.set_radi_sweep_width(w)
        try:
            Z, K, info = ctx.ric_radi(ms, B, W, max_steps=steps, res_reltol=1e-12, fetch=False)
        finally:
            ctx.set_radi_sweep_width(1)
        swi = ctx.radi_sweep_info()
        assert info["stop_rule"] == ("res" if case == "wide62" else "max_steps")
        runs[w] = dict(info, gain=K, res_hist=ctx.adi_res_history(), sweep_width=swi["width"], sweeps=swi["sweeps"],
                       stop_rule=ctx.STOP_RULES.index(info["stop_rule"]))
    hd, gd = _against_sequential(case, runs[1], runs[16], 16, want)
    assert gd <= gain_bar() and hd <= hist_bar(), (hd, gd)


# ------------------------------------------------------------------------------------------- 5. contract, hygiene
def _lu_solve(f, p, R):
    npr = f["J"].shape[0]
    S = sps.bmat([[f["calA"] + p * f["calE"], f["J"].T], [f["J"], None]], format="csc")
    return spsla.splu(S).solve(np.vstack([R, np.zeros((npr, R.shape[1]))]))


def test_contract_and_hygiene(ctx4):
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    ctx, f = ctx4
    for w in (0, 17):
        with pytest.raises(ValueError):
            ctx.set_radi_sweep_width(w)
    # width 1 gives the bits of a context that never saw the setting
    with _lib.Context(0) as fresh:
        fresh.set_operator(f["calA"], f["calE"], f["J"])
        _, Kf, _ = fresh.ric_radi(f["ms"], f["B"], f["W"], max_steps=6, res_reltol=1e-14)
    ctx.set_radi_sweep_width(4)
    ctx.set_radi_sweep_width(1)
    _, K1, _ = ctx.ric_radi(f["ms"], f["B"], f["W"], max_steps=6, res_reltol=1e-14)
    assert ctx.radi_sweep_info() == dict(width=1, sweeps=0, solves=6)
    # (the solves are iterative and start from zero on either context: same operator, same bits)
    assert np.array_equal(K1, Kf)
    # a generated-shift mode with width > 1: refused before anything is launched
    ctx.set_radi_sweep_width(4)
    ctx.set_radi_shifts("hamiltonian")
    try:
        t0 = ctx.solve_trace()["solves"]
        with pytest.raises(ValueError):
            ctx.ric_radi(f["ms"], f["B"], f["W"], max_steps=6)
        assert ctx.solve_trace()["solves"] == t0
    finally:
        ctx.set_radi_shifts("cycle")
        ctx.set_radi_sweep_width(1)
    # a one-element list: effective width 1
    ctx.set_radi_sweep_width(4)
    try:
        _, _, info = ctx.ric_radi(f["ms"][:1], f["B"], f["W"], max_steps=3, res_reltol=1e-14)
        assert ctx.radi_sweep_info() == dict(width=1, sweeps=0, solves=3) and info["radi_steps"] == 3
        # nothing left behind after a sweep run (tests/test_gpu_radi.py::test_nothing_left_behind)
        R = np.random.default_rng(3).standard_normal((ctx.nv, 4))
        ref = _lu_solve(f, -7.0, R)
        ctx.set_recycle(2)
        try:
            X0, _, _ = ctx.shift_solve(-7.0, 1.0, R)
            assert rel(X0, ref) < 1e-8
            t0 = ctx.solve_trace()
            _, _, info = ctx.ric_radi(f["ms"], f["B"], f["W"], max_steps=8, res_reltol=1e-14)
            t1 = ctx.solve_trace()
            assert ctx.radi_sweep_info()["sweeps"] == 2
            assert t1["guess_tried"] == t0["guess_tried"] and t1["stored"] == t0["stored"]      # recycling off inside
            X1, _, _ = ctx.shift_solve(-7.0, 1.0, R)
            t2 = ctx.solve_trace()
            assert rel(X1, ref) < 1e-8
            assert t2["smw_solves"] == t1["smw_solves"] and t2["inop_lowrank"] == t1["inop_lowrank"]
            assert t2["guess_tried"] == t1["guess_tried"] + 1 and t2["stored"] == t1["stored"] + 1
        finally:
            ctx.set_recycle(0)
    finally:
        ctx.set_radi_sweep_width(1)
    # pru: the setting is restored after a failing call, and after a good one
    backend.reset()
    try:
        with pytest.raises(ValueError):
            pru.proj_alg_ric_radi(radi_dict=dict(ms="hamiltonian", sweep_width=4, radi_max_steps=4), **f["kw"])
        pctx = backend.context()
        assert pctx.set_radi_sweep_width(1) == 1 and pctx.set_radi_shifts("cycle") == _lib.RICADI_RADI_SHIFTS_CYCLE
        with pytest.raises(ValueError):
            pru.proj_alg_ric_radi(radi_dict=dict(ms=f["ms"], sweep_width=17), **f["kw"])
        out = pru.proj_alg_ric_radi(radi_dict=dict(ms=f["ms"], radi_max_steps=4), **f["kw"])
        assert out["sweep_width"] == 1 and out["sweeps"] == 0 and out["shift_solves"] == 4
        out = pru.proj_alg_ric_radi(radi_dict=dict(ms=f["ms"], radi_max_steps=4, sweep_width=4), **f["kw"])
        assert out["sweep_width"] == 4 and out["sweeps"] == 1 and out["shift_solves"] == 4
        out = pru.proj_alg_ric_radi(radi_dict=dict(ms=f["ms"], radi_max_steps=4), **f["kw"])
        assert out["sweep_width"] == 1 and out["sweeps"] == 0
        assert backend.context().set_radi_sweep_width(4) == 1
        # the default MEANS width 1, also on a context someone set wider; that setting is as before afterwards
        out = pru.proj_alg_ric_radi(radi_dict=dict(ms=f["ms"], radi_max_steps=4), **f["kw"])
        assert out["sweep_width"] == 1 and out["sweeps"] == 0
        assert backend.context().set_radi_sweep_width(1) == 4
    finally:
        backend.reset()


# ------------------------------------------------------------------------------------------- 6. the DRE sweep
class _Recording:
    """pru with the sweep widths of its RADI calls recorded."""

    def __init__(self, pru):
        self._pru, self.widths, self.sweeps = pru, [], []

    def __getattr__(self, name):
        return getattr(self._pru, name)

    def proj_alg_ric_radi(self, **kw):
        out = self._pru.proj_alg_ric_radi(**kw)
        self.widths.append(out["sweep_width"])
        self.sweeps.append(out["sweeps"])
        return out


def test_two_step_dre_sweep_with_radi_sweeps():
    """N = 8, two time steps through solve_flow_daeric with ``ric_solver='radi'`` and a list of shifts: gains and w of
    every time at width 4 against the same call at width 1."""
    from optconpy_amd import problems as pb, proj_ric_utils as pru
    from optconpy_amd.dae_ric import MemoryStore, solve_flow_daeric
    from test_dae_ric import _setup
    backend.reset()
    try:
        pr, kw, tmesh = _setup(N=8, Nts=2)
        d = dict(ms=pb.logshifts(0.4, 60.0, 8), radi_res_reltol=1e-12, radi_max_steps=200)
        s1, s4 = MemoryStore(), MemoryStore()
        r1, r4 = _Recording(pru), _Recording(pru)
        f1 = solve_flow_daeric(store=s1, pru=r1, ric_solver="radi", radi_dict=d, **kw)
        f4 = solve_flow_daeric(store=s4, pru=r4, ric_solver="radi", radi_dict=dict(d, sweep_width=4), **kw)
        print("widths", r1.widths, r4.widths, "sweeps", r4.sweeps)
        assert len(r4.widths) == len(r1.widths) == 2 and set(r1.widths) == {1}
        assert all(2 <= w <= 4 for w in r4.widths) and all(s >= 1 for s in r4.sweeps)
        worst = 0.0
        for t in tmesh:
            ek = rel(s4.load(f4[t]["mtxtb"]), s1.load(f1[t]["mtxtb"]))
            ew = rel(s4.load(f4[t]["w"]), s1.load(f1[t]["w"]))
            print("t = %.3f: gain %.3e  w %.3e" % (t, ek, ew))
            worst = max(worst, ek, ew)
        assert DRE_MEASURED is not None, "no measurement recorded"
        assert worst <= min(10.0 * DRE_MEASURED, 1e-7), worst
    finally:
        backend.reset()
