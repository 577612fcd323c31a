"""Every launch form of the saddle product K1 against the FP64 SciPy product (tests/saddle_model.py).

``Context.op_apply_batch_dev`` runs ``saddle_spmm`` as the lockstep GMRES iteration does -- groups with their own
(alpha, beta), active tables, the FP32-stored input (X32) and FP32 output panel (Y32), the residual form, the low-rank
epilogue -- and reports the kernel form that ran (``k1_variant``: 0 CSR, 1 tiled, 2 tiled multi-shift, +4 FP32 input).
Every element is held to the bound of ``saddle_model`` (C = 2: |y - ref| <= 2 (k + 2) eps |S| |x|, plus one FP32 ulp
for Y32), the reference computed on fl32(X) under X32.  Groups the call does not name, and the gaps between panels,
must keep the NaN they were filled with.  Each test asserts the variant it is named for (``_expected_variant`` mirrors
the launcher's choice from the exported tile format); ``test_variants_reached`` runs last and checks the coverage.

Operators: cfg1 (N = 15), N = 58 (>= 900 row blocks: the multi-shift kernel walks 16 groups in one workgroup), and
long-row variants of cfg1 (``saddle_model.long_rows``): rows of 49, 64, 100 entries and a pressure row of 60
(multi-shift tiles), rows up to 250 entries (max_cols > 192: second pass of the 16-byte tile fill), a row of 400
(max_cols > 320: CSR at m = 16, still tiled at m = 1).
"""
import os

import numpy as np
import pytest

from optconpy_amd import _lib
import saddle_model as sm

pytestmark = pytest.mark.gpu

M_ALL = [1, 5, 15, 16, 17, 32, 33, 48, 128]
X32, Y32, LOWRANK, RESIDUAL = (_lib.Context.OA_X32, _lib.Context.OA_Y32, _lib.Context.OA_LOWRANK,
                               _lib.Context.OA_RESIDUAL)
REACHED = dict(variants=set(), y32=set(), long_tile_row=False, f4_pass2=False)
WORST = {}


def _shifts(G):
    """Distinct shifts, a DRE-style beta != 1 in every third group (group 0 first), groups 1 and 2 equal."""
    al = list(-np.logspace(0.0, 3.0, G))
    be = [0.37 if g % 3 == 0 else 1.0 for g in range(G)]
    if G >= 3:
        al[2], be[2] = al[1], be[1]
    return al, be


def _build(name):
    base = sm.th_operators(15, 0.1)
    if name == "cfg1":
        return base
    if name == "n58":
        return sm.th_operators(58, 0.05)
    if name == "long100":
        return sm.long_rows(base, [49, 64, 100], p_target=60)[0]
    if name == "long250":
        return sm.long_rows(base, [49, 64, 100, 170, 250])[0]
    if name == "long400":
        return sm.long_rows(base, [400])[0]
    raise KeyError(name)


@pytest.fixture(scope="module")
def env():
    """(ops, tiles, context) per (operator, RICADI_MS_SPMM setting); the switch is read when the context is made."""
    ops, ctxs = {}, {}

    def get(name, ms=None):
        if name not in ops:
            o = _build(name)
            ops[name] = (o, _lib.host_saddle_tiles(*o))
        key = (name, ms)
        if key not in ctxs:
            old = os.environ.get("RICADI_MS_SPMM")
            if ms is None:
                os.environ.pop("RICADI_MS_SPMM", None)
            else:
                os.environ["RICADI_MS_SPMM"] = ms
            try:
                ctx = _lib.Context(0)
            finally:
                if old is None:
                    os.environ.pop("RICADI_MS_SPMM", None)
                else:
                    os.environ["RICADI_MS_SPMM"] = old
            ctx.set_operator(*ops[name][0])
            ctxs[key] = ctx
        return ops[name][0], ops[name][1], ctxs[key]
    yield get
    for ctx in ctxs.values():
        ctx.close()


def _expected_variant(t, m, nact, flags, ms, lowrank):
    """k1_variant the launcher picks (solver_precond.inl: saddle_tiled, ms_pays, spmm_blocked_ms_ok); None: the
    entry must refuse the combination."""
    fits = t["sb_ok"] and t["max_cols"] * m * 8 + 16 <= 40 * 1024
    pays = ms != "0" and t["ms_ok"] and (ms == "2" or (nact >= 4 and t["nnz"] * 10.0 * nact > 200e6))
    ms_ok = pays and m <= 16 and t["max_cols"] <= 160 and t["n"] * m * 8 < 2 ** 31
    if flags & X32:
        if not fits or flags & RESIDUAL or lowrank:
            return None
        return (2 if ms_ok else 1) + 4
    if flags & Y32:
        return None
    return 2 if (fits and ms_ok and not lowrank) else 1 if fits else 0


def _run(env, name, m, G=3, flags=0, ms=None, active=None, x_stride=None, y_stride=None, alpha=1.0, beta_r=0.0,
         r_stride=None, lowrank=None, seed=0, expect=-1):
    """One call, checked element by element; returns the variant."""
    import torch
    ops, t, ctx = env(name, ms)
    n = t["n"]
    nm = n * m
    xs, ys = x_stride or nm, y_stride or nm
    al, be = _shifts(G)
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((G, xs))
    Xd = torch.from_numpy(X.ravel()).cuda()
    Yd = torch.full((G * ys,), float("nan"), dtype=torch.float64, device="cuda")
    R = Rd = None
    rs = 0
    if flags & RESIDUAL:
        rs = r_stride or nm
        R = rng.standard_normal((G, rs))
        Rd = torch.from_numpy(R.ravel()).cuda()
    if lowrank:
        U = rng.standard_normal((t["nv"], lowrank))
        V = rng.standard_normal((t["nv"], lowrank)) / np.sqrt(t["nv"])
        ctx.set_lowrank(U, V)
    nact = G if active is None else len(active)
    want = _expected_variant(t, m, nact, flags, ms, bool(lowrank))
    if expect != -1:
        assert want == expect, (name, m, flags, ms, want, expect)
    try:
        if want is None:
            with pytest.raises(ValueError):       # RICADI_EINVAL
                ctx.op_apply_batch_dev(al, be, Xd.data_ptr(), xs, m, Yd.data_ptr(), ys, active=active, flags=flags,
                                       alpha=alpha, r_ptr=None if Rd is None else Rd.data_ptr(), r_stride=rs,
                                       beta_r=beta_r)
            assert torch.isnan(Yd).all().item(), "a refused call wrote its output"
            return None
        var = ctx.op_apply_batch_dev(al, be, Xd.data_ptr(), xs, m, Yd.data_ptr(), ys, active=active, flags=flags,
                                     alpha=alpha, r_ptr=None if Rd is None else Rd.data_ptr(), r_stride=rs,
                                     beta_r=beta_r)
        torch.cuda.synchronize()
    finally:
        if lowrank:
            ctx.set_lowrank(None, None)
    assert var == want, (name, m, flags, ms, var, want)
    Y = Yd.cpu().numpy().reshape(G, ys)
    groups = list(range(G)) if active is None else list(active)
    nv = t["nv"]
    y32 = bool(flags & Y32)
    for g in range(G):
        if g not in groups:
            assert np.all(np.isnan(Y[g])), ("group not named was written", g)
            continue
        assert np.all(np.isnan(Y[g, nm:])), ("gap behind the panel was written", g)
        Xg = X[g, :nm].reshape(n, m)
        if flags & X32:
            Xg = Xg.astype(np.float32).astype(np.float64)
        Rg = None if R is None else R[g, :nm].reshape(n, m)
        ref, bound = sm.reference(ops, al[g], be[g], Xg, alpha=alpha, R=Rg, beta_r=beta_r,
                                  lowrank=(U, V) if lowrank else None)
        e = sm.excess(Y[g, :nm].reshape(n, m), ref, bound, y32)
        for part, rows in (("velocity", slice(0, nv)), ("pressure", slice(nv, n))):
            key = (var, "y32" if y32 else "y64", part)
            WORST[key] = max(WORST.get(key, 0.0), float(np.max(e[rows])))
        assert np.all(e <= 1.0), (name, m, flags, ms, g, float(np.max(e)),
                                  np.unravel_index(int(np.argmax(e)), e.shape))
    REACHED["variants"].add(var)
    if y32:
        REACHED["y32"].add(var)
    lens = np.diff(t["rp2"], axis=1)
    if var in (1, 2, 5, 6) and lens.max() > 48:
        REACHED["long_tile_row"] = True
    if var == 5 and m == 16 and t["max_cols"] > 192 and xs % 4 == 0:
        REACHED["f4_pass2"] = True
    return var


@pytest.mark.parametrize("m", M_ALL)
@pytest.mark.parametrize("G", [1, 3])
def test_per_group_fp64(env, m, G):
    """cfg1, FP64 in and out, one workgroup per (row block, group): tiled where the tiles fit the LDS, else CSR."""
    _run(env, "cfg1", m, G=G, seed=m)


@pytest.mark.parametrize("m", M_ALL)
@pytest.mark.parametrize("flags", [X32, X32 | Y32], ids=["x32", "x32_y32"])
def test_per_group_fp32_input(env, m, flags):
    """cfg1, FP32-stored input (and FP32 output panel): variant 5 where the tiles fit, refused elsewhere."""
    _run(env, "cfg1", m, G=3, flags=flags, seed=100 + m)


@pytest.mark.parametrize("m", [1, 5, 16, 17])
@pytest.mark.parametrize("flags", [0, X32, X32 | Y32], ids=["x64", "x32", "x32_y32"])
@pytest.mark.parametrize("G,active", [(1, None), (3, None), (16, None), (16, [1, 4, 7]), (16, list(range(0, 16, 2)))],
                         ids=["G1", "G3", "G16", "G16_147", "G16_even"])
def test_multi_shift_forced(env, m, flags, G, active):
    """cfg1 with RICADI_MS_SPMM=2: the multi-shift kernel for m <= 16 (variants 2 and 6; grid.y splits the groups,
    with several groups per workgroup at G = 16), the per-group kernel above."""
    v = _run(env, "cfg1", m, G=G, flags=flags, ms="2", active=active, seed=G * 7 + m)
    assert (v & 3) == (2 if m <= 16 else 1), v


@pytest.mark.parametrize("flags", [0, X32 | Y32], ids=["x64", "x32_y32"])
def test_multi_shift_off(env, flags):
    """RICADI_MS_SPMM=0: per-group tiles whatever the group count."""
    v = _run(env, "cfg1", 16, G=16, flags=flags, ms="0", seed=5)
    assert (v & 3) == 1, v


@pytest.mark.parametrize("ms", [None, "2"], ids=["default", "ms_forced"])
@pytest.mark.parametrize("flags", [0, X32, X32 | Y32], ids=["x64", "x32", "x32_y32"])
@pytest.mark.parametrize("active", [None, [1, 4, 7]], ids=["all", "147"])
def test_n58(env, ms, flags, active):
    """N = 58, 16 groups: at >= 900 row blocks the multi-shift kernel keeps grid.y = 1, so one workgroup walks every
    active group through its double-buffered tile."""
    _, t, _ = env("n58", ms)
    assert t["nblk"] >= 900, t["nblk"]
    v = _run(env, "n58", 16, G=16, flags=flags, ms=ms, active=active, seed=58)
    if ms == "2":
        assert (v & 3) == 2, v


@pytest.mark.parametrize("ms,m", [("0", 5), ("0", 16), ("0", 17), ("2", 5), ("2", 16), ("2", 17), (None, 48)])
@pytest.mark.parametrize("G,active", [(3, None), (16, list(range(0, 16, 2)))], ids=["G3", "G16_even"])
def test_residual_form(env, ms, m, G, active):
    """The restart residual: y = r - S x (alpha = -1, beta_r = 1), FP64, r with its own stride; per-group tiles,
    multi-shift tiles (m <= 16 forced) and CSR (m = 48)."""
    n = env("cfg1", ms)[1]["n"]
    v = _run(env, "cfg1", m, G=G, flags=RESIDUAL, ms=ms, active=active, alpha=-1.0, beta_r=1.0,
             r_stride=n * m + 3, y_stride=n * m + 5, seed=300 + m)
    assert v == (2 if ms == "2" and m <= 16 else 1 if m <= 32 else 0), v


@pytest.mark.parametrize("q", [1, 8])
def test_lowrank_epilogue(env, q):
    """- U (V^T x_v) in the tile kernel's epilogue, m = 17, three groups."""
    v = _run(env, "cfg1", 17, G=3, flags=LOWRANK, lowrank=q, seed=q)
    assert v == 1, v


@pytest.mark.parametrize("ms", [None, "2"], ids=["default", "ms_forced"])
@pytest.mark.parametrize("m", [1, 16, 17])
@pytest.mark.parametrize("flags", [0, X32 | Y32], ids=["x64", "x32_y32"])
def test_long_rows_multi_shift_tiles(env, ms, m, flags):
    """Rows of 49, 64, 100 entries and a pressure row of 60 (max_cols <= 152): the streamed part past 48 entries in
    the per-group and in the multi-shift kernel."""
    _, t, _ = env("long100", ms)
    assert int(np.max(np.diff(t["rp2"], axis=1))) == 100 and t["ms_ok"]
    _run(env, "long100", m, G=3, flags=flags, ms=ms, seed=m)


@pytest.mark.parametrize("m", [1, 16])
@pytest.mark.parametrize("flags", [0, X32, X32 | Y32], ids=["x64", "x32", "x32_y32"])
def test_long_rows_wide_tiles(env, m, flags):
    """Rows up to 250 entries: max_cols > 192, so the 16-byte tile fill of the FP32 input takes a second pass."""
    _, t, _ = env("long250")
    assert 192 < t["max_cols"] <= 319, t["max_cols"]
    v = _run(env, "long250", m, G=3, flags=flags, seed=250 + m)
    assert (v & 3) == 1, v


@pytest.mark.parametrize("m,flags,variant", [(16, 0, 0), (16, X32, None), (1, 0, 1), (1, X32 | Y32, 5)])
def test_row_of_400(env, m, flags, variant):
    """A row of 400 entries: max_cols > 320, so 16-column panels go to the CSR kernel (and the FP32 forms are
    refused there) while one-column panels stay tiled."""
    _, t, _ = env("long400")
    assert t["max_cols"] > 320, t["max_cols"]
    _run(env, "long400", m, G=3, flags=flags, seed=400 + m, expect=variant)


@pytest.mark.parametrize("name,ms", [("cfg1", None), ("cfg1", "2"), ("long250", None)])
@pytest.mark.parametrize("flags", [X32, X32 | Y32], ids=["x32", "x32_y32"])
def test_fp32_input_unaligned_groups(env, name, ms, flags):
    """x_stride = 16 n + 2: the FP32 group bases are not 16-byte aligned, so the launchers must take the one-column
    tile fill instead of the 16-byte one."""
    n = env(name, ms)[1]["n"]
    v = _run(env, name, 16, G=3, flags=flags, ms=ms, x_stride=16 * n + 2, y_stride=16 * n + 4, seed=2)
    assert v == (6 if ms == "2" else 5), v


def test_refused_combinations(env):
    """FP32 output without FP32 input, FP32 input with the residual term: RICADI_EINVAL, nothing written."""
    _run(env, "cfg1", 16, flags=Y32)
    _run(env, "cfg1", 16, flags=X32 | RESIDUAL, alpha=-1.0, beta_r=1.0)


def test_variants_reached():
    """Runs last in this file: what the tests above reached together."""
    if not REACHED["variants"]:
        pytest.skip("run with the rest of this file")
    print("[saddle spmm] reached:", {k: sorted(v) if isinstance(v, set) else v for k, v in REACHED.items()})
    for key in sorted(WORST):
        print("[saddle spmm] variant %d %s %s rows: worst error / bound %.3f" % (key + (WORST[key],)))
    assert {0, 1, 2, 5, 6} <= REACHED["variants"], REACHED
    assert {5, 6} <= REACHED["y32"], REACHED
    assert REACHED["long_tile_row"] and REACHED["f4_pass2"], REACHED
