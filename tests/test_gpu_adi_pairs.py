"""GPU tests of the Lyapunov ADI with complex-conjugate shift pairs (ricadi_lyap_adi_cplx,
solver_adi_pairs.inl, the pair kernels of ricadi_cplx.hip) against the dense model of tests/adi_pairs_model.py and the
dense Lyapunov solutions of tests/small_ops.py.  Every check prints ``[adi pairs] operator | check | measured | bound``
before it asserts.

tests/test_adi_pairs_cpu.py holds the model to its references and shows that the comparisons of the blocks kernel can
fail; it has to pass for these to mean anything.
"""
import ctypes as C

import numpy as np
import pytest

import adi_pairs_model as apm
import small_ops as so
from optconpy_amd import _lib
from optconpy_amd import proj_ric_utils as pru
from test_adi_pairs_cpu import (FIRST_BLOCK_TOL, KERNEL_M, KERNEL_NV, KERNEL_P, LOWRANK, PLAIN, first_block_list, model_of,
                                steps_pinned)

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
LYAP_TOL = 1e-8          # Z Z^T against the dense Lyapunov solution: the bar of test_gpu_small_ops.py
HIST_TOL = 2.05e-9       # residual history of the step form against the model, entries above 1e-6
TIGHT = dict(adi_max_steps=300, adi_newZ_reltol=1e-12)
KERNEL_OPS = ("nv1", "nv2_np1", "nv31_np12", "nv33_np1", "arrow200")     # nv = KERNEL_NV, constraints on four of them


def _say(name, check, value, bound):
    ok = bool(np.isfinite(value)) and value <= bound
    print("[adi pairs] %s | %s | %.3e | %.3e%s" % (name, check, value, bound, "" if ok else "  MISS"))
    return ok


def _dev(a, dtype=np.float64):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")
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


def _context(op):
    ctx = _lib.Context(0, **op.opts)
    ctx.set_operator(*op.ops)
    return ctx


def _pairs_visited(ms, steps):
    """Pair entries among the entries of the cycled list that ``steps`` steps visit."""
    done, pairs, e = 0, 0, 0
    while done < steps:
        pair = isinstance(ms[e % len(ms)], complex)
        done += 2 if pair else 1
        pairs += int(pair)
        e += 1
    assert done == steps
    return pairs


# ------------------------------------------------------------------------------------------------ the blocks kernel
@pytest.mark.parametrize("name", KERNEL_OPS)
def test_blocks_kernel_entry_by_entry(name):
    """``ricadi_adi_pair_blocks_dev`` on the device's own X against the float64 twin: nv = 1, 2, one below and one
    above the rows of a workgroup, several workgroups with a tail; m = 1 .. 24 (one to three groups, partial last
    group); zc = 0 and 3 with ldz = zc + 2m + 5; four shifts.  The pressure rows of X are NaN and must not be read, Z
    and V1 start as NaN and stay NaN outside the two blocks; entries within ``4 eps gam (|Re x| + |delta Im x|)`` (V1:
    without gam), norms within ``(nv m + 4) eps`` relative and bitwise equal on a second call."""
    op = so.get(name)
    assert op.nv in KERNEL_NV
    miss = []
    with _context(op) as ctx:
        nv, n = op.nv, op.n
        for m in KERNEL_M:
            ng, mc = apm.groups(m)
            assert (ng, mc) == _lib.adi_pair_groups(m)
            for zc in (0, 3):
                ldz = zc + 2 * m + 5
                for p in KERNEL_P:
                    rng = np.random.default_rng(1000 * nv + 10 * m + zc)
                    X = rng.standard_normal((ng, n, mc)) + 1j * rng.standard_normal((ng, n, mc))
                    X[:, nv:] = np.nan + 1j * np.nan
                    Xd = _dev(X, np.complex128)
                    outs = []
                    for _ in range(2):
                        Zd, V1d = _dev(np.full((nv, ldz), np.nan)), _dev(np.full((nv, m), np.nan))
                        n2 = ctx.adi_pair_blocks_dev(ng, mc, m, p, Xd.data_ptr(), Zd.data_ptr(), ldz, zc, V1d.data_ptr())
                        outs.append((_host(Zd), _host(V1d), n2))
                    Z, V1, n2 = outs[0]
                    assert np.array_equal(outs[1][2], n2), "norms not bitwise repeatable"
                    assert np.array_equal(outs[1][0], Z, equal_nan=True) and np.array_equal(outs[1][1], V1)
                    Xh = _host(Xd)
                    assert np.array_equal(Xh.view(np.float64), X.view(np.float64), equal_nan=True), "X was written"
                    T1, T2, TV, tn2 = apm.blocks_twin(Xh, nv, m, p)
                    bz, bv = apm.blocks_bound(Xh, nv, m, p)
                    outside = np.ones(ldz, dtype=bool)
                    outside[zc:zc + 2 * m] = False
                    assert np.all(np.isnan(Z[:, outside])), "Z was written outside the two blocks"
                    blk = Z[:, zc:zc + 2 * m]
                    assert np.all(np.isfinite(blk)) and np.all(np.isfinite(V1)), "a pressure row was read"
                    tiny = np.finfo(float).tiny
                    worst = max(float(np.max(np.abs(blk[:, :m] - T1) / np.maximum(bz, tiny))),
                                float(np.max(np.abs(blk[:, m:] - T2) / np.maximum(bz, tiny))),
                                float(np.max(np.abs(V1 - TV) / np.maximum(bv, tiny))))
                    nerr = float(np.max(np.abs(n2 - tn2) / tn2))
                    tag = "m %d zc %d p %s" % (m, zc, p)
                    if not _say(name, tag + ": entry error / bound", worst, 1.0):
                        miss.append((tag, worst))
                    if not _say(name, tag + ": norms", nerr, (nv * m + 4) * EPS):
                        miss.append((tag, nerr))
        # refusals of the entry: outputs untouched
        Zd, V1d = _dev(np.full((nv, 9), np.nan)), _dev(np.full((nv, 2), np.nan))
        Xd = _dev(np.zeros((1, n, 2)), np.complex128)
        for kw in (dict(m=3), dict(p=1 + 1j), dict(p=-1 + 0j), dict(ldz=3), dict(mc=9), dict(ng=17)):
            a = dict(ng=1, mc=2, m=2, p=-1 + 1j, ldz=9)
            a.update(kw)
            with pytest.raises(ValueError, match="ricadi"):
                ctx.adi_pair_blocks_dev(a["ng"], a["mc"], a["m"], a["p"], Xd.data_ptr(), Zd.data_ptr(), a["ldz"], 0,
                                        V1d.data_ptr())
        assert np.all(np.isnan(_host(Zd))) and np.all(np.isnan(_host(V1d)))
    assert not miss, miss


# ------------------------------------------------------------------------------------------------ the driver
def _driver_case(name, lowrank, W=None, tag=""):
    op, mdl, ms = model_of(name, lowrank)
    W = op.W if W is None else W
    m = W.shape[1]
    ref = mdl.run(ms, W, max_steps=300, newZ_reltol=1e-12, woodbury=lowrank)
    X = mdl.lyap(W)
    with _context(op) as ctx:
        if lowrank:
            ctx.set_lowrank(-op.oldB, op.B)
        Z, info = ctx.lyap_adi(ms, W, _lib.adi_params(TIGHT))
    who = "%s%s%s" % (name, " lowrank" if lowrank else "", tag)
    print("[adi pairs] %s | steps %d (model %d) solves %d pair_info %s stopped by %s" %
          (who, info["adi_steps"], ref["steps"], info["shift_solves"], info.get("pair_info"), info["adi_stopped_by"]))
    ok = _say(who, "Z Z^T vs dense", so.rel(Z @ Z.T, X), LYAP_TOL)
    assert ok
    # the model's step count exactly where its stopping step is a factor 2 clear of the tolerance on both sides
    pinned = steps_pinned(ref, TIGHT["adi_newZ_reltol"])
    print("[adi pairs] %s | step count held to the model's %s" % (who, "exactly" if pinned else "+- 2"))
    assert abs(info["adi_steps"] - ref["steps"]) <= (0 if pinned else 2), (info["adi_steps"], ref["steps"])
    assert info["cols"] == info["adi_steps"] * m == Z.shape[1]
    assert info["gmres_nonconverged"] == 0
    if any(isinstance(p, complex) for p in ms):
        pairs = _pairs_visited(ms, info["adi_steps"])
        assert info["pair_info"][0] == pairs and info["pair_info"][3] == 0
        assert info["shift_solves"] == info["adi_steps"] - pairs
        assert info["pair_info"][1] >= pairs
        if lowrank:
            # no refinement pass where the model's amplification stays at or below 8 along its own run (9 is where a
            # column could reach 10 gmres_tol; tests/test_adi_pairs_cpu.py asserts it for every LOWRANK operator)
            amp = float(ref["amplification"].max())
            print("[adi pairs] %s | largest model amplification %.2f, refinement passes %d" %
                  (who, amp, info["pair_info"][2]))
            if amp <= 8.0:
                assert info["pair_info"][2] == 0, info["pair_info"]
        else:
            assert info["pair_info"][2] == 0
    else:
        assert "pair_info" not in info and info["shift_solves"] == info["adi_steps"]
    return info


@pytest.mark.parametrize("name", PLAIN)
def test_driver_against_dense(name):
    """The CPU test's operators and lists through ``Context.lyap_adi``: ``Z Z^T`` to LYAP_TOL, the model's step count
    +- 2, ``cols = steps m``, ``pair_info[0]`` the pair entries visited."""
    _driver_case(name, False)


@pytest.mark.parametrize("name", LOWRANK)
def test_driver_against_dense_with_a_lowrank_term(name):
    """The same with ``calA + oldB B^T``: Sherman-Morrison-Woodbury around the complex solve."""
    _driver_case(name, True)


@pytest.mark.parametrize("m", [3, 9, 17])
def test_driver_panel_widths(m):
    """One, two and three groups of complex columns on fe3, with and without the low-rank term."""
    op = so.get("fe3")
    W = np.random.default_rng(80 + m).standard_normal((op.nv, m))
    _driver_case("fe3", False, W, " m %d" % m)
    _driver_case("fe3", True, W, " m %d" % m)


# ------------------------------------------------------------------------------------------------ stopping
def test_stopping_and_history():
    """An odd ``adi_max_steps`` with a pair due last ends one step short with rule MAX_STEPS; the history has one entry
    per step, equal within a pair, and agrees with the model's to the step-form bound."""
    op, mdl, ms = model_of("fe3", False)
    pair = ms[0]
    with _context(op) as ctx:
        ctx.set_adi_res_history(True)
        Z, info = ctx.lyap_adi([pair], op.W, _lib.adi_params(dict(adi_max_steps=5, adi_newZ_reltol=0.0)))
        assert (info["adi_steps"], info["cols"], info["shift_solves"]) == (4, 4 * op.W.shape[1], 2)
        assert info["adi_stopped_by"] == "max_steps" and info["pair_info"][0] == 2
        assert ctx.adi_res_history().size == 4
        lst = [pair, -1.0, ms[1]]
        Z, info = ctx.lyap_adi(lst, op.W, _lib.adi_params(dict(adi_max_steps=20, adi_newZ_reltol=0.0)))
        h = ctx.adi_res_history()
        ref = mdl.run(lst, op.W, max_steps=20)
        assert info["adi_steps"] == ref["steps"] == 20 and h.size == 20
        for k in range(0, 20, 5):
            assert h[k] == h[k + 1] and h[k + 3] == h[k + 4] and h[k + 1] != h[k + 2]
        big = ref["hist"] > 1e-6
        assert big.any()
        assert _say("fe3", "residual history vs model", float(np.max(np.abs(h[big] - ref["hist"][big]) / ref["hist"][big])),
                    HIST_TOL)
        # the residual rule ends the iteration behind a pair, with both of its blocks kept
        prm = _lib.adi_params(dict(adi_max_steps=300, adi_newZ_reltol=0.0, adi_res_reltol=1e-6))
        Z, info = ctx.lyap_adi(ms, op.W, prm)
        ref = mdl.run(ms, op.W, max_steps=300, res_reltol=1e-6)
        assert info["adi_stopped_by"] == "res" and ref["rule"] == "res"
        assert abs(info["adi_steps"] - ref["steps"]) <= 2 and info["cols"] == info["adi_steps"] * op.W.shape[1]
        assert ctx.adi_res_history()[-1] <= 1e-6


def test_a_rule_that_fires_on_a_pairs_first_block_keeps_both_blocks():
    """fe3, the first recipe pair with its imaginary part times 20, ``adi_newZ_reltol = 0.266``: the model's relative
    block norms are 1.0, 0.99 and 0.101, 0.701 (tests/test_adi_pairs_cpu.py), so the rule fires on the second pair's
    first block and not on its second.  The run ends with rule newZ behind that pair, both of its blocks in Z."""
    op, mdl, lst = first_block_list()
    m = op.W.shape[1]
    with _context(op) as ctx:
        Z, info = ctx.lyap_adi(lst, op.W, _lib.adi_params(dict(adi_max_steps=300, adi_newZ_reltol=FIRST_BLOCK_TOL)))
    with _context(op) as ctx:
        Z4, info4 = ctx.lyap_adi(lst, op.W, _lib.adi_params(dict(adi_max_steps=4, adi_newZ_reltol=0.0)))
    print("[adi pairs] fe3 | first-block rule | steps %d cols %d pair_info %s stopped by %s" %
          (info["adi_steps"], info["cols"], info["pair_info"], info["adi_stopped_by"]))
    assert info["adi_stopped_by"] == "newZ" and info["adi_steps"] == 4 and info["cols"] == 4 * m == Z.shape[1]
    assert info["pair_info"][0] == 2
    assert info4["adi_stopped_by"] == "max_steps" and info4["cols"] == 4 * m
    assert np.array_equal(Z, Z4[:, :4 * m])
    assert np.all(np.any(Z[:, 2 * m:] != 0.0, axis=0)), "a block of the second pair is missing"


def test_recompression_inside_the_iteration():
    """``compress_cols`` works as in the real step form: fewer columns, the same ``Z Z^T``."""
    op, mdl, ms = model_of("fe3", False)
    with _context(op) as ctx:
        Z, info = ctx.lyap_adi(ms, op.W, _lib.adi_params(dict(TIGHT, compress_cols=24)))
    assert info["cols"] < info["adi_steps"] * op.W.shape[1] and info["cols"] == Z.shape[1]
    assert _say("fe3", "Z Z^T vs dense, compress_cols 24", so.rel(Z @ Z.T, op.lyap()), LYAP_TOL)


# ------------------------------------------------------------------------------------------------ unchanged paths
@pytest.mark.parametrize("width", [1, 4])
def test_real_list_is_bitwise_ricadi_lyap_adi(width):
    """A list without pairs through ``ricadi_lyap_adi_cplx`` is ``ricadi_lyap_adi``, step and sweep form (a fresh
    context each)."""
    op = so.get("fe3")
    prm = _lib.adi_params(dict(TIGHT, sweep_width=width))
    with _context(op) as ctx:
        Z0, info0 = ctx.lyap_adi(op.shifts, op.W, prm)
    with _context(op) as ctx:
        Z1, stats, cols = ctx.lyap_adi_cplx(op.shifts, np.zeros(len(op.shifts)), op.W, prm)
        assert ctx.adi_pair_info() == [0, 0, 0, 0]
    assert cols == info0["cols"] and int(stats[0]) == info0["adi_steps"] and int(stats[3]) == info0["shift_solves"]
    assert np.array_equal(Z0, Z1)


def test_real_calls_around_a_pair_call_are_a_fresh_contexts(monkeypatch):
    """On one context a real ``lyap_adi`` before and after a pair call returns bitwise what a fresh context returns:
    the pair step's workspaces, the proxies' cache entries and the grown GMRES workspace change nothing a real call
    computes.  Recycling is off, as in ``test_gpu_cplx.test_real_path_unchanged``: with it, any second call on one
    operator starts its solves from the first call's stored solutions (the ring outlives a call) and differs in the
    last bits from a fresh context's, whether a pair call lies between them or not."""
    monkeypatch.setenv("RICADI_RECYCLE", "0")
    op, mdl, ms = model_of("fe3", False)
    prm = _lib.adi_params(TIGHT)
    with _context(op) as ctx:
        ctx.set_recycle(0)
        fresh, finfo = ctx.lyap_adi(op.shifts, op.W, prm)
    with _context(op) as ctx:
        ctx.set_recycle(0)
        before, _ = ctx.lyap_adi(op.shifts, op.W, prm)
        before = before.copy()
        ctx.lyap_adi(ms, op.W, prm)
        assert ctx.adi_pair_info()[0] > 0
        after, ainfo = ctx.lyap_adi(op.shifts, op.W, prm)
    assert np.array_equal(before, fresh) and np.array_equal(after, fresh)
    assert ainfo["adi_steps"] == finfo["adi_steps"] and "pair_info" not in ainfo


def test_complex_batch_solve_still_refuses_a_lowrank_term():
    op = so.get("unsym")
    rng = np.random.default_rng(5)
    with _context(op) as ctx:
        R = _dev(rng.standard_normal((op.nv, 3)) + 1j * rng.standard_normal((op.nv, 3)), np.complex128)
        ctx.set_lowrank(-op.oldB, op.B)
        with pytest.raises(ValueError, match="low-rank"):
            ctx.shift_solve_cplx_batch_dev([-1 + 1j], R)
        # ... while the pair step takes it
        Z, info = ctx.lyap_adi([-1 + 1j], op.W, _lib.adi_params(dict(adi_max_steps=2, adi_newZ_reltol=0.0)))
        assert info["adi_steps"] == 2 and info["pair_info"][0] == 1


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    """RICADI_EINVAL with a message: ``re >= 0``, NaN, ``m + q > 128``, a complex entry on a context with a forced
    exchange; the context stays usable."""
    op = so.get("fe3")
    prm = _lib.adi_params(dict(adi_max_steps=4, adi_newZ_reltol=0.0))
    with _context(op) as ctx:
        for re_, im_ in (([-1.0, 0.0], [1.0, 1.0]), ([-1.0, 2.0], [1.0, 0.0]), ([-1.0, np.nan], [1.0, 0.0]),
                         ([-1.0, -2.0], [1.0, np.nan]), ([-1.0, -np.inf], [1.0, 0.0])):
            with pytest.raises(ValueError, match="ADI shifts must be finite with a negative real part"):
                ctx.lyap_adi_cplx(re_, im_, op.W, prm)
        ctx.set_lowrank(-op.oldB, op.B)
        wide = np.random.default_rng(2).standard_normal((op.nv, 127))
        with pytest.raises(ValueError, match="at most 128"):
            ctx.lyap_adi([-1 + 1j], wide, prm)
        ctx.set_lowrank(None, None)
        ident = C.create_string_buffer(128)
        assert ctx._lib.ricadi_rccl_unique_id(ident, 128) == 0
        _lib._chk(ctx._lib.ricadi_set_exchange_rccl(ctx._h, 0, 1, ident, None, 8 * ctx.n * 16 * 8 + 4096 * 2))
        with pytest.raises(ValueError, match="exchange"):
            ctx.lyap_adi([-1 + 1j], op.W, prm)
        _lib._chk(ctx._lib.ricadi_set_exchange(ctx._h, 0, 1, None, None, None, None, 0))
        Z, info = ctx.lyap_adi([-1 + 1j], op.W, prm)
        assert info["adi_steps"] == 4 and np.all(np.isfinite(Z))


# ------------------------------------------------------------------------------------------------ the drop-in
def test_dropin_takes_complex_lists_and_auto_complex():
    """``solve_proj_lyap_stein`` with a complex list (``umat`` / ``vmat`` included) and with ``ms='auto-complex'`` on
    fe3: ``out['ms']``, ``out['pair_info']``, LYAP_TOL; ``ms='auto'`` returns what it returned before."""
    op, mdl, ms = model_of("fe3", False)
    kw = dict(amat=op.calA, mmat=op.calE, jmat=op.J, wmat=op.W, transposed=True)
    X = op.lyap()
    auto0 = pru.solve_proj_lyap_stein(adi_dict=dict(TIGHT, ms="auto"), **kw)
    lst = [ms[0], ms[0].conjugate()] + ms[1:]
    out = pru.solve_proj_lyap_stein(adi_dict=dict(TIGHT, ms=lst), **kw)
    assert out["ms"] == ms and out["pair_info"][0] >= 1
    assert _say("fe3", "drop-in, complex list", so.rel(out["zfac"] @ out["zfac"].T, X), LYAP_TOL)
    opl, mdll, msl = model_of("fe3", True)
    outl = pru.solve_proj_lyap_stein(adi_dict=dict(TIGHT, ms=msl), umat=-op.oldB, vmat=op.B.T, **kw)
    assert outl["pair_info"][0] >= 1
    assert _say("fe3", "drop-in, complex list, umat / vmat", so.rel(outl["zfac"] @ outl["zfac"].T, mdll.lyap(op.W)),
                LYAP_TOL)
    outc = pru.solve_proj_lyap_stein(adi_dict=dict(TIGHT, ms="auto-complex"), **kw)
    assert any(isinstance(p, complex) for p in outc["ms"]) and outc["pair_info"][0] >= 1
    assert sum(2 if isinstance(p, complex) else 1 for p in outc["ms"]) <= 8
    assert _say("fe3", "drop-in, auto-complex", so.rel(outc["zfac"] @ outc["zfac"].T, X), LYAP_TOL)
    auto1 = pru.solve_proj_lyap_stein(adi_dict=dict(TIGHT, ms="auto"), **kw)
    # (the same list up to the last bits: the projected pencil itself is summed in a fixed order -- ricadi_project.hip
    # has no atomics, test_gpu_adi_shifts.py asserts it bitwise --, but the Gram matrices of ctx.qr behind the basis it
    # is projected on come from gemm_tn, which adds its slices with atomics in an order that varies from call to
    # call, and the recycling ring starts the second call's solves from the first call's solutions: eps-level changes
    # of a pencil of order <= 128, far below the 1e-8 asked here)
    assert len(auto1["ms"]) == len(auto0["ms"]) and all(type(p) is float for p in auto1["ms"])
    assert np.allclose(auto1["ms"], auto0["ms"], rtol=1e-8, atol=0.0) and "pair_info" not in auto1
    assert abs(auto1["adi_steps"] - auto0["adi_steps"]) <= 1
    assert _say("fe3", "drop-in, auto", so.rel(auto1["zfac"] @ auto1["zfac"].T, X), LYAP_TOL)
    # the Riccati iterations keep refusing complex entries
    for fn, key in ((pru.proj_alg_ric_newtonadi, "nwtn_adi_dict"), (pru.proj_alg_ric_radi, "radi_dict")):
        with pytest.raises(ValueError, match="ADI shifts must be negative real numbers"):
            fn(mmat=op.calE, amat=op.calA, jmat=op.J, bmat=op.B, wmat=op.W, transposed=True, **{key: dict(ms=[-1 + 1j])})
