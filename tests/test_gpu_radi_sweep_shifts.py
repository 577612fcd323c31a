"""GPU tests of RADI sweeps with generated shifts (``ms='hamiltonian-sweep'``, ricadi_set_radi_sweep_shifts; DESIGN.md
3d-4).

1. the reduction for a group of 33 .. 127 columns of Z against an m-column residual (ricadi_radi_reduce_group_dev) entry
   by entry against a longdouble product, exact on small integers, bitwise equal on a second call, and the bits of the
   existing entries where the group is one of their shapes;
2. whole solves of the call forms at widths 2, 4, 8 against SciPy's dense Riccati solver;
3. the cases of the model's stability study that take part: step count, sweep widths, basis sizes and every shift
   against the model (tests/golden/radi_sweep_shift_model.npz, written by tests/radi_sweep_shift_model.py);
4. width 1 with the setting on: the bits of ``'hamiltonian-dominant'``;
5. wide factors (33 columns at width 3, 58 at width 2);  6. the 128-column limit (16 columns at width 8);
7. forced fallbacks, and the borrowed per-shift entries a sequential call shares with a sweep;
8. a run stopped by the residual inside a sweep;  9. the contract;  10. the two-step DRE sweep.

tests/test_radi_sweep_shifts_cpu.py holds the model and the host entry; it has to pass for these to mean anything.
"""
import numpy as np
import pytest
import scipy.sparse as sps

import dense_model as dm
import radi_model as rm
import radi_shift_model as sm
import radi_sweep_shift_model as ssm
from optconpy_amd import _lib, backend

pytestmark = pytest.mark.gpu
K_TOL = 1e-6          # the project's bar (tests/test_gpu_radi.py)
X_TOL = 1e-6
TOL = 1e-10           # res_reltol of the runs compared with the model: the tolerance of its table and shifts
# Largest relative deviation of the device's shifts from the model's per participating case of the stability study, as
# measured on the MI355X at res_reltol = 1e-10; the tests assert ten times the case's value, never more than 1e-3 (a
# flipped selection moved shifts by >= 7e-3 in the study).
SHIFT_MEASURED = {
    "steady_4_w2": 1.529e-09,
    "steady_4_w4": 1.846e-07,
    "steady_4_w8": 1.435e-08,
    "dre_4_w2": 3.186e-09,
    "steady_8_w2": 2.199e-08,
    "steady_8_w4": 3.424e-07,
    "steady_8_w8": 1.083e-06,
    "dre_8_w8": 2.561e-07,
    "wide33_8_w2": 1.280e-07,
    "wide33_8_w3": 1.334e-06,
    "wide58_8_w2": 1.470e-08,
    "random16_8_w4": 1.002e-05,
    "random16_8_w8": 1.080e-06,
}
GOLD = np.load(ssm.golden_path())
PARTICIPANTS = [c for c in ssm.TABLE if ssm.key(*c) in set(GOLD["participants"].tolist())]


def shift_bar(key):
    assert SHIFT_MEASURED[key] is not None, "no measurement recorded for " + key
    bar = 10.0 * SHIFT_MEASURED[key]
    assert bar <= 1e-3
    return bar


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


_ctxs = {}


@pytest.fixture(scope="module")
def ctx_of():
    """Contexts by (N, operator): 'steady' (nv = 98 / 450: no multiple of 16 or 64) or 'dre'."""
    def get(N, op="steady"):
        if (N, op) not in _ctxs:
            f = rm.call_forms(N)[0 if op == "steady" else 1]
            ctx = _lib.Context(0)
            ctx.set_operator(f["calA"], f["calE"], f["J"])
            _ctxs[N, op] = ctx
        return _ctxs[N, op]
    yield get
    for ctx in _ctxs.values():
        ctx.close()
    _ctxs.clear()


# ---------------------------------------------------------------------------------------- 1. the group's reduction
# (c, m, nb): tile edges at 32 / 16 / 64, c no multiple of 16, m + 2nb across a dense-tile edge
SHAPES = [(33, 1, 1), (34, 17, 2), (47, 4, 64), (64, 8, 8), (99, 33, 4), (112, 16, 8), (116, 58, 4), (127, 1, 1)]


def _reduce(ctx, Q, RU, B, entry="group"):
    c, nb = Q.shape[1], B.shape[1]
    m = RU.shape[1] - nb
    Qd, RUd, Bd = _dev(Q), _dev(RU), _dev(B)
    Hd = _dev(np.full((c + 1, 2 * c + m + 2 * nb), np.nan))          # one guard row
    fn = dict(group=ctx.radi_reduce_group_dev, narrow=ctx.radi_reduce_dev, wide=ctx.radi_reduce_wide_dev)[entry]
    fn(Qd.data_ptr(), c, RUd.data_ptr(), m, Bd.data_ptr(), nb, Hd.data_ptr())
    H = _host(Hd)
    assert np.all(np.isnan(H[c])) and not np.any(np.isnan(H[:c]))
    return H[:c]


def _basis(rng, nv, c):
    """A random orthonormal Q where nv allows one (c <= nv); else random columns of that size (at nv = 98 a basis of
    99 .. 127 columns cannot be orthonormal, and the kernel does not need it to be)."""
    Q = rng.standard_normal((nv, c))
    return np.linalg.qr(Q)[0] if c <= nv else Q / np.sqrt(nv)


@pytest.mark.parametrize("N", [4, 8])
@pytest.mark.parametrize("c,m,nb", SHAPES)
def test_reduce_group_entry_by_entry(ctx_of, N, c, m, nb):
    """Every entry within radi_shift_model.reduce_bounds at u = 2^-53 of the longdouble product."""
    ctx, f = ctx_of(N), rm.call_forms(N)[0]
    nv = ctx.nv
    rng = np.random.default_rng(1000 * c + 10 * m + nb)
    Q = _basis(rng, nv, c)
    RU, B = rng.standard_normal((nv, m + nb)), rng.standard_normal((nv, nb))
    ref = sm.reduce(Q, f["calA"], f["calE"], RU, B)
    tol = dm.tol(sm.reduce_bounds, Q, f["calA"], f["calE"], RU, B)
    H = _reduce(ctx, Q, RU, B)
    ratio = dm.ratio(H, ref, tol)
    print("nv %d c %d m %d nb %d: error / bound %.3g" % (nv, c, m, nb, ratio))
    assert ratio <= 1.0
    assert np.array_equal(_reduce(ctx, Q, RU, B), H)                   # bitwise: fixed summation order


def test_reduce_group_exact_on_small_integers_and_the_existing_entries_bits(ctx_of):
    """An operator with small integer values on the pattern of the N = 4 operator: every entry of H is exact.  A group
    that is a shape of an existing entry runs that entry's kernel: the same bits."""
    f = rm.call_forms(4)[0]
    rng = np.random.default_rng(7)

    def ints(M):
        M = sps.csr_matrix(M).copy()
        M.data = rng.integers(-4, 5, M.nnz).astype(float)
        return M

    A, E = ints(f["calA"]), ints(f["calE"])
    with _lib.Context(0) as ctx:
        ctx.set_operator(A, E, f["J"])
        nv = ctx.nv
        for c, m, nb in SHAPES:
            Q = rng.integers(-3, 4, (nv, c)).astype(float)
            RU, B = rng.integers(-3, 4, (nv, m + nb)).astype(float), rng.integers(-3, 4, (nv, nb)).astype(float)
            ref = Q.T @ np.hstack([A @ Q, E @ Q, RU, B])
            assert np.array_equal(_reduce(ctx, Q, RU, B), ref), (c, m, nb)
        # shapes the entry refuses (before anything is launched): a wide residual on the narrow kernel, the limits
        d = _dev(np.zeros(4)).data_ptr()
        for c, m, nb in ((32, 33, 1), (0, 1, 1), (128, 1, 1), (40, 128, 1), (40, 0, 1), (40, 4, 65), (40, 4, 0)):
            with pytest.raises(ValueError):
                ctx.radi_reduce_group_dev(d, c, d, m, d, nb, d)
    for N in (4, 8):
        ctx = ctx_of(N)
        nv = ctx.nv
        for (c, m, nb), entry in (((32, 4, 4), "narrow"), ((64, 64, 8), "wide")):
            Q = _basis(rng, nv, c)
            RU, B = rng.standard_normal((nv, m + nb)), rng.standard_normal((nv, nb))
            assert np.array_equal(_reduce(ctx, Q, RU, B), _reduce(ctx, Q, RU, B, entry)), (N, c, m, nb)


# ------------------------------------------------------------------------------------------------ the whole solves
def run(ctx, f, width, fallback=None, max_steps=200, tol=TOL, sweep_shifts=True, mode="hamiltonian-dominant",
        compress_cols=0):
    """One RADI call with generated sweep shifts (mode, setting and width are restored): dict(Z, K, info, ms, fallbacks,
    kept, res, widths, swi)."""
    fb = [sm.initial_shift(f["calA"], f["calE"])] if fallback is None else list(fallback)
    mode_before = ctx.set_radi_shifts(mode)
    set_before = ctx.set_radi_sweep_shifts(sweep_shifts)
    width_before = ctx.set_radi_sweep_width(width)
    try:
        Z, K, info = ctx.ric_radi(fb, f["B"], f["W"], oldB=f["old"], max_steps=max_steps, res_reltol=tol,
                                  compress_cols=compress_cols)
    finally:
        ctx.set_radi_sweep_width(width_before)
        ctx.set_radi_sweep_shifts(set_before)
        ctx.set_radi_shifts(mode_before)
    out = dict(Z=Z, K=K, info=info, ms=ctx.radi_shift_history(), fallbacks=ctx.radi_shift_fallbacks(),
               kept=ctx.probe_radi_kept(), res=np.asarray(ctx.adi_res_history()), widths=ctx.radi_sweep_widths(),
               swi=ctx.radi_sweep_info())
    out.update(ctx.probe_radi_counters())
    assert info["radi_steps"] == len(out["ms"]) == len(out["res"])
    assert out["swi"]["solves"] == info["shift_solves"] and out["swi"]["sweeps"] == len(out["widths"])
    assert len(out["widths"]) == 0 or out["widths"].sum() == info["shift_solves"]
    return out


_dense, _cycled, _runs = {}, {}, {}


def dense_of(name, N):
    if (name, N) not in _dense:
        _dense[name, N] = rm.dense_are_of(ssm.case_form(name, N))
    return _dense[name, N]


def cycled_steps(name, N, tol):
    """Steps of the form's cycled list in the model (tests/radi_model.radi)."""
    if (name, N, tol) not in _cycled:
        f = ssm.case_form(name, N)
        _cycled[name, N, tol] = rm.radi(f["calA"], f["calE"], f["J"], f["B"], f["W"], f["ms"], old=f["old"],
                                        res_reltol=tol)["steps"]
    return _cycled[name, N, tol]


def case_run(ctx_of, name, N, w):
    """The device's run of a case of the model's table at 1e-10 (run once, shared: read-only)."""
    if (name, N, w) not in _runs:
        _runs[name, N, w] = run(ctx_of(N, "dre" if name.startswith("dre") else "steady"), ssm.case_form(name, N), w)
    return _runs[name, N, w]


def check_solution(r, name, N, what):
    X, K = dense_of(name, N)
    ex, ek = rel(r["Z"] @ r["Z"].T, X), rel(r["K"], K)
    print("%s: %d steps in %d sweeps %s, %d solves, fallbacks %d, kept %s, qr_repeats %d, rel X %.2e rel K %.2e" % (
        what, len(r["ms"]), len(r["widths"]), r["widths"].tolist(), r["info"]["shift_solves"], r["fallbacks"],
        sorted(set(r["kept"].tolist())), r["qr_repeats"], ex, ek))
    assert r["info"]["stop_rule"] == "res" and r["info"]["gmres_nonconverged"] == 0
    assert ex < X_TOL and ek < K_TOL, (what, ex, ek)


# ---------------------------------------------------------------------------------------------- 2. the call forms
@pytest.mark.parametrize("name", ["steady", "dre", "dre_old"])
@pytest.mark.parametrize("N", [4, 8])
def test_call_forms_against_the_dense_solver(ctx_of, N, name):
    f = ssm.case_form(name, N)
    ctx = ctx_of(N, "steady" if name == "steady" else "dre")
    mw, nb = f["W"].shape[1], f["B"].shape[1]
    for w in (2, 4, 8):
        r = run(ctx, f, w, tol=1e-12)
        check_solution(r, name, N, "N = %d %-8s width %d" % (N, name, w))
        assert r["fallbacks"] == 0
        assert r["widths"][0] == 1 and r["widths"].max() <= w == r["swi"]["width"]
        assert len(r["kept"]) == len(r["widths"]) - 1                    # one selection per sweep but the last
        assert r["Z"].shape[1] == len(r["ms"]) * mw
        assert len(r["ms"]) <= cycled_steps(name, N, 1e-12), (len(r["ms"]), cycled_steps(name, N, 1e-12))
        assert 0 <= r["info"]["shift_solves"] - len(r["ms"]) < w


# ------------------------------------------------------------------------------------------- 3. against the model
@pytest.mark.parametrize("name,N,w", PARTICIPANTS)
def test_participating_cases_against_the_model(ctx_of, name, N, w):
    """Step count, sweep widths and basis sizes equal the model's; every shift within ten times the largest deviation
    measured on the MI355X for the case (SHIFT_MEASURED), at most 1e-3."""
    k = ssm.key(name, N, w)
    assert GOLD["moves_" + k].max() < ssm.MOVE_BAR
    r = case_run(ctx_of, name, N, w)
    ms = GOLD["ms_" + k]
    n = min(len(ms), len(r["ms"]))
    d = float(np.max(np.abs(r["ms"][:n] - ms[:n]) / np.abs(ms[:n])))
    print("%s: %d steps (model %d), widths %s (model %s), kept %s, shifts within %.3e of the model's (its own move by "
          "%.1e)" % (k, len(r["ms"]), len(ms), r["widths"].tolist(), GOLD["widths_" + k].tolist(), r["kept"].tolist(),
                     d, GOLD["moves_" + k].max()))
    assert len(r["ms"]) == len(ms) == GOLD["table_" + k][0]
    assert r["widths"].tolist() == GOLD["widths_" + k].tolist()
    assert r["kept"].tolist() == GOLD["kept_" + k].tolist()
    assert r["fallbacks"] == 0 and r["info"]["shift_solves"] == GOLD["table_" + k][2]
    assert d <= shift_bar(k), (d, SHIFT_MEASURED[k])


def test_every_required_case_takes_part():
    assert set(ssm.MUST_TAKE_PART) <= set(PARTICIPANTS) and set(ssm.key(*c) for c in PARTICIPANTS) == set(SHIFT_MEASURED)


# -------------------------------------------------------------------------------------------------- 4. width one
@pytest.mark.parametrize("N,name", [(4, "steady"), (8, "dre_old")])
def test_width_one_is_the_dominant_mode(ctx_of, N, name):
    f = ssm.case_form(name, N)
    ctx = ctx_of(N, "steady" if name == "steady" else "dre")
    a = run(ctx, f, 1, sweep_shifts=False)
    b = run(ctx, f, 1, sweep_shifts=True)
    assert np.array_equal(a["K"], b["K"]) and np.array_equal(a["ms"], b["ms"]) and np.array_equal(a["Z"], b["Z"])
    assert a["kept"].tolist() == b["kept"].tolist() and len(b["widths"]) == 0
    assert b["swi"] == dict(width=1, sweeps=0, solves=len(b["ms"]))


# ------------------------------------------------------------------------------------ 5. wide factors, 6. G mw = 128
@pytest.mark.parametrize("name,w,cap", [("wide33", 3, 3), ("wide33", 8, 3), ("wide58", 2, 2), ("wide58", 8, 2)])
def test_wide_factors(ctx_of, name, w, cap):
    """33 columns at width 3 and 58 at width 2 (the caps 128 / mw: a wider request runs the same sweeps and bits): the
    model's steps, X and K against the dense solver."""
    r = case_run(ctx_of, name, 8, cap)
    if w != cap:
        r2 = run(ctx_of(8), ssm.case_form(name, 8), w)
        assert r2["swi"]["width"] == cap and np.array_equal(r2["K"], r["K"]) and np.array_equal(r2["ms"], r["ms"])
        return
    check_solution(r, name, 8, "N = 8 %s width %d" % (name, w))
    k = ssm.key(name, 8, w)
    assert r["swi"]["width"] == cap and r["widths"].max() == cap
    assert len(r["ms"]) == GOLD["table_" + k][0] and r["widths"].tolist() == GOLD["widths_" + k].tolist()
    assert np.all(r["kept"] == 32) and r["fallbacks"] == 0


def test_the_128_column_limit(ctx_of):
    """mw = 16 at width 8: G mw = 128, the group of the selection holds 7 of the 8 blocks a full sweep keeps (112
    columns).  Converges; the widths -- and, in the test above, the shifts -- are the model's, whose basis is cut so."""
    mod = ssm.run_case("random16", 8, 8)
    assert mod["kept_blocks"].max() == 8 and mod["basis_blocks"].max() == 7 and max(rec[0] for rec in mod["record"]) == 112
    r = case_run(ctx_of, "random16", 8, 8)
    check_solution(r, "random16", 8, "N = 8 random16 width 8")
    assert r["swi"]["width"] == 8 and r["widths"].max() == 8
    assert r["widths"].tolist() == mod["widths"].tolist() and len(r["ms"]) == mod["steps"]


# ------------------------------------------------------------------------------------------ 7. forced fallbacks
def test_forced_fallbacks():
    """N = 8 steady at width 4, list [p0] + ms[:3]: the selection after the sweep that ends at step 5, and after the
    second sweep behind it, count as refused.  The sweeps that follow are ONE step with list entries 1 and 2."""
    f = ssm.case_form("steady", 8)
    fb = [sm.initial_shift(f["calA"], f["calE"])] + [float(v) for v in f["ms"][:3]]
    with _lib.Context(0) as ctx:
        ctx.set_operator(f["calA"], f["calE"], f["J"])
        free = run(ctx, f, 4, fallback=fb)
        assert free["fallbacks"] == 0 and free["widths"].tolist()[:2] == [1, 4]
        # what one shift adds to the cache (an entry per level): a listed shift the fallbacks do not reach
        na = ctx.cache_entries()
        run(ctx, f, 1, fallback=[fb[3]], mode="cycle", sweep_shifts=False, max_steps=1)
        per_shift = ctx.cache_entries() - na
        assert per_shift >= 1
        n0 = ctx.cache_entries()
        try:
            ctx.probe_radi_refuse([5])
            one = run(ctx, f, 4, fallback=fb)
            assert one["fallbacks"] == 1 and one["widths"].tolist()[:3] == [1, 4, 1] and one["ms"][5] == fb[1]
            ends = np.cumsum(one["widths"])
            E = int(ends[3])                                     # the sweep behind the fallback step ends here
            assert E > 6 and len(one["widths"]) > 5
            ctx.probe_radi_refuse([5, E])
            n0 = ctx.cache_entries()                             # (fb[1] is in the cache now)
            r = run(ctx, f, 4, fallback=fb)
            n1 = ctx.cache_entries()
            print("refused after steps 5 and %d: widths %s, fallbacks %d, cache entries %d -> %d (%d per shift)" % (
                E, r["widths"].tolist(), r["fallbacks"], n0, n1, per_shift))
            assert r["fallbacks"] == 2
            assert r["widths"].tolist()[:5] == one["widths"].tolist()[:4] + [1]
            assert r["ms"][5] == fb[1] and r["ms"][E] == fb[2]                     # bitwise: entries 1, 2
            assert np.array_equal(r["ms"][:E], one["ms"][:E])
            assert len(r["kept"]) == len(r["widths"]) - 1                        # the refused selections were made too
            check_solution(r, "steady", 8, "N = 8 steady width 4 with fallbacks")
            assert n1 == n0 + per_shift                          # fb[2], and no generated shift
            r2 = run(ctx, f, 4, fallback=fb)
            assert np.array_equal(r2["ms"], r["ms"]) and np.array_equal(r2["K"], r["K"]) and r2["fallbacks"] == 2
            assert ctx.cache_entries() == n1
        finally:
            ctx.probe_radi_refuse(())
        r3 = run(ctx, f, 4, fallback=fb)
        assert r3["fallbacks"] == 0 and np.array_equal(r3["ms"], free["ms"]) and np.array_equal(r3["K"], free["K"])
        assert ctx.cache_entries() == n1


def test_sequential_and_sweep_calls_share_their_borrowed_entries():
    """A sequential call with generated shifts borrows the first of the per-shift entries a generated sweep borrows.
    N = 8 steady on one context: sequential DOMINANT, sweeps of 4, and both once more -- each repeat gives the bits of
    its first run, whichever form rebuilt the shared entry in between, and the cache holds what the first call left.
    (No recompression inside the calls: a recompressed factor's bits are those of the GEMM's atomics.)"""
    f = ssm.case_form("steady", 8)
    nocomp = 200 * f["W"].shape[1] + 1
    with _lib.Context(0) as ctx:
        ctx.set_operator(f["calA"], f["calE"], f["J"])
        assert ctx.nv == 450
        runs, entries = [], []
        for width in (1, 4, 1, 4):
            runs.append(run(ctx, f, width, sweep_shifts=width > 1, compress_cols=nocomp))
            entries.append(ctx.cache_entries())
        print("steps %s, sweep widths %s, cache entries %s" % ([len(r["ms"]) for r in runs],
                                                               [r["widths"].tolist() for r in runs], entries))
        assert len(runs[0]["widths"]) == 0 and runs[1]["widths"].max() > 1 and runs[1]["swi"]["width"] == 4
        for first, again in ((0, 2), (1, 3)):
            for k in ("K", "ms", "res"):
                assert np.array_equal(runs[again][k], runs[first][k]), (first, again, k)
            assert runs[again]["recompressions"] == runs[first]["recompressions"] == 0
        assert entries[1:] == entries[:1] * 3


# ------------------------------------------------------------------------- 8. the residual rule inside a sweep
def test_residual_rule_inside_a_sweep(ctx_of):
    f, ctx = ssm.case_form("steady", 4), ctx_of(4)
    full = case_run(ctx_of, "steady", 4, 8)
    assert full["widths"].tolist()[:3] == [1, 2, 6]
    hist = full["res"]
    assert hist[4] > 1.01 * hist[5]
    r = run(ctx, f, 8, tol=1.01 * hist[5])                      # stops at step 6: the third block of the third sweep
    G, k = int(r["widths"][-1]), len(r["ms"]) - int(r["widths"][:-1].sum())
    print("stopped inside a sweep: widths %s, %d steps, %d solves" % (r["widths"].tolist(), len(r["ms"]),
                                                                    r["info"]["shift_solves"]))
    assert r["info"]["stop_rule"] == "res" and len(r["ms"]) == 6 and r["widths"].tolist() == [1, 2, 6]
    assert (G, k) == (6, 3) and r["info"]["shift_solves"] - r["info"]["radi_steps"] == G - k
    assert r["Z"].shape[1] == 6 * f["W"].shape[1] and len(r["kept"]) == 2       # no selection after the stop
    assert np.array_equal(r["ms"], full["ms"][:6])
    assert rel(r["Z"] @ r["Z"].T, full["Z"][:, :r["Z"].shape[1]] @ full["Z"][:, :r["Z"].shape[1]].T) < 1e-8
    # a sweep cut by max_steps: 1 + 2 + 2 of the 6 generated
    c = run(ctx, f, 8, max_steps=5, tol=1e-14)
    assert c["widths"].tolist() == [1, 2, 2] and c["info"]["stop_rule"] == "max_steps" and len(c["ms"]) == 5
    assert np.array_equal(c["ms"], full["ms"][:5]) and len(c["kept"]) == 2


# ---------------------------------------------------------------------------------------------------- 9. contract
def test_contract(ctx_of):
    from optconpy_amd import proj_ric_utils as pru
    f, ctx = ssm.case_form("steady", 4), ctx_of(4)
    lib, h = ctx._lib, ctx._h
    # the setters: values, returns, what stays refused
    assert lib.ricadi_set_radi_sweep_shifts(h, 2) == -1 and lib.ricadi_set_radi_sweep_shifts(h, -1) == -1
    assert lib.ricadi_set_radi_sweep_shifts(h, 1) == 0 and lib.ricadi_set_radi_sweep_shifts(h, 0) == 1
    assert lib.ricadi_set_radi_shift_mode(h, 3) == -1
    assert ctx.set_radi_sweep_shifts(True) is False and ctx.set_radi_sweep_shifts(False) is True
    # the setting with mode 0 or 1: refused before anything is launched, at any width
    for mode in ("cycle", "hamiltonian"):
        for w in (1, 4):
            t0 = ctx.solve_trace()["solves"]
            with pytest.raises(ValueError):
                run(ctx, f, w, fallback=f["ms"], mode=mode)
            assert ctx.solve_trace()["solves"] == t0
    # the setting off: a generated mode at width 4 is refused as before
    for mode in ("hamiltonian", "hamiltonian-dominant"):
        t0 = ctx.solve_trace()["solves"]
        with pytest.raises(ValueError):
            run(ctx, f, 4, mode=mode, sweep_shifts=False)
        assert ctx.solve_trace()["solves"] == t0
    # CYCLE-mode sweeps: the bits do not depend on the setting having been toggled
    a = run(ctx, f, 4, fallback=f["ms"], mode="cycle", sweep_shifts=False, max_steps=8, tol=1e-14)
    ctx.set_radi_sweep_shifts(True)
    ctx.set_radi_sweep_shifts(False)
    b = run(ctx, f, 4, fallback=f["ms"], mode="cycle", sweep_shifts=False, max_steps=8, tol=1e-14)
    assert np.array_equal(a["K"], b["K"]) and np.array_equal(a["Z"], b["Z"]) and a["widths"].tolist() == [4, 4]
    # pru: mode, setting and width are restored after a failing call and after a good one
    backend.reset()
    try:
        def settings():
            c = backend.context()
            s = (c.set_radi_shifts("cycle"), c.set_radi_sweep_shifts(False), c.set_radi_sweep_width(1))
            return s
        good = dict(ms="hamiltonian-sweep", radi_res_reltol=TOL)
        out = pru.proj_alg_ric_radi(radi_dict=good, **f["kw"])
        assert settings() == (_lib.RICADI_RADI_SHIFTS_CYCLE, False, 1)
        assert out["sweep_width"] == 8 and out["sweeps"] == len(out["sweep_widths"]) and out["shift_fallbacks"] == 0
        assert out["sweep_widths"][0] == 1 and sum(out["sweep_widths"]) == out["shift_solves"]
        assert len(out["ms"]) == out["radi_steps"] and out["stop_rule"] == _lib.RICADI_STOP_RES
        X, K = dense_of("steady", 4)
        assert rel(out["gain"], K) < K_TOL and rel(out["zfac"] @ out["zfac"].T, X) < X_TOL
        for bad in (dict(good, sweep_width=17), dict(good, sweep_width=0)):
            with pytest.raises(ValueError):
                pru.proj_alg_ric_radi(radi_dict=bad, **f["kw"])
            assert settings() == (_lib.RICADI_RADI_SHIFTS_CYCLE, False, 1)
        wide = dict(f["kw"], wmat=np.ones((f["W"].shape[0], 127)))             # mw + nb > 128: refused inside the call
        with pytest.raises(ValueError):
            pru.proj_alg_ric_radi(radi_dict=good, **wide)
        assert settings() == (_lib.RICADI_RADI_SHIFTS_CYCLE, False, 1)
        with pytest.raises(ValueError):                                        # the other generated modes still refuse
            pru.proj_alg_ric_radi(radi_dict=dict(ms="hamiltonian", sweep_width=4), **f["kw"])
        # ms_fallback, and a width of its own
        fb = [sm.initial_shift(f["calA"], f["calE"])] + [float(v) for v in f["ms"][:2]]
        out2 = pru.proj_alg_ric_radi(radi_dict=dict(good, ms_fallback=fb, sweep_width=2), **f["kw"])
        assert out2["sweep_width"] == 2 and max(out2["sweep_widths"]) == 2 and out2["ms"][0] == fb[0]
        assert "sweep_widths" not in pru.proj_alg_ric_radi(radi_dict=dict(ms="hamiltonian-dominant"), **f["kw"])
    finally:
        backend.reset()


def test_exchange_context_is_refused():
    """A context with an exchange set keeps returning RICADI_ESTATE before anything is launched, with the setting on."""
    import ctypes as C
    f = ssm.case_form("steady", 4)
    with _lib.Context(0) as ctx:
        ctx.set_operator(f["calA"], f["calE"], f["J"])
        ms = np.ascontiguousarray([sm.initial_shift(f["calA"], f["calE"])])
        B, W = np.ascontiguousarray(f["B"]), np.ascontiguousarray(f["W"])
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        stats, cc = np.zeros(8), C.c_int(0)
        ctx.set_radi_shifts("hamiltonian-dominant")
        ctx.set_radi_sweep_shifts(True)
        ctx.set_radi_sweep_width(4)
        t0 = ctx.solve_trace()["solves"]
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
        Z, K, info = ctx.ric_radi(ms, B, W, max_steps=5)
        assert info["radi_steps"] == 5 and ctx.radi_sweep_widths().tolist() == [1, 2, 2]


# --------------------------------------------------------------------------------------------- 10. the DRE sweep
def test_two_step_dre_sweep():
    """The problem and the bar of test_dae_ric.test_two_step_sweep_gpu_vs_dense_riccati_solver, every step's Riccati
    equation by RADI in sweeps of generated shifts."""
    from identities import dense_dre_sweep_gains
    from optconpy_amd import proj_ric_utils as pru
    from optconpy_amd.dae_ric import MemoryStore, solve_flow_daeric
    from test_dae_ric import _pin_setup

    class Recording:
        def __init__(self):
            self.outs = []

        def __getattr__(self, name):
            return getattr(pru, name)

        def proj_alg_ric_radi(self, **kw):
            out = pru.proj_alg_ric_radi(**kw)
            self.outs.append((kw["wmat"].shape[1], kw["bmat"].shape[1], out["sweep_width"], list(out["sweep_widths"]),
                              out["radi_steps"], out["shift_fallbacks"]))
            return out

    backend.reset()
    try:
        pr, kw, tmesh = _pin_setup()
        dense = dense_dre_sweep_gains(pr, kw, tmesh)
        store, rec = MemoryStore(), Recording()
        fb = solve_flow_daeric(store=store, pru=rec, ric_solver="radi",
                               radi_dict=dict(ms="hamiltonian-sweep", sweep_width=4, radi_res_reltol=1e-13,
                                              radi_max_steps=120), **kw)
        print("(mw, nb, cap, sweep widths, steps, fallbacks) per time step:", rec.outs)
        assert len(rec.outs) == len(tmesh) - 1
        for mw, nb, cap, widths, steps, nfb in rec.outs:
            assert cap == ssm.cap_width(4, mw, nb, 120) and nfb == 0
            # (a W of more than 64 columns has the cap 128 // mw = 1: the sequential form, no sweeps)
            assert (widths == []) if cap == 1 else (widths[0] == 1 and max(widths) <= cap)
        assert any(max(o[3]) > 1 for o in rec.outs)
        for t in tmesh:
            K = store.load(fb[t]["mtxtb"])
            e = np.linalg.norm(K - dense[t]) / np.linalg.norm(dense[t])
            print("t = %.3f: gain against the dense solver %.2e" % (t, e))
            assert e <= 1e-6, t
    finally:
        backend.reset()
