"""The whole stack on tiny and irregular operators (tests/small_ops.py) against dense FP64 references.

Every other GPU test takes its operator from a Taylor-Hood mesh with NV >= 98.  Here NV runs from 1 to 65 around
the tile sizes of the kernels (16-row MFMA chunks, 32-row SpMM blocks, 16 / 32 / 64-row block-Jacobi blocks), the
constraint count from 0 to NV - 1, and the patterns are irregular: every workgroup is a tail workgroup, coarse spaces
have 2 - 3 unknowns or none, pressure blocks one row.  One context per operator serves all its tests; each check
prints ``[small ops] operator | check | measured | bound`` before it asserts, and a test reports all its misses.

References: the dense saddle matrix and its LU, the dense projected Lyapunov and Riccati solutions (small_ops), the
cycle, product and dense-step models of precond_model, saddle_model and dense_model.  tests/test_small_ops_cpu.py
shows that the family meets the caps these bounds rest on and that every comparator used here can fail.

Contract refusals (the only inputs an entry may refuse here, asserted as ``ValueError`` with untouched outputs):
``ricadi_qr`` with more columns than rows (c <= NV, include/ricadi.h).  ``compress``, ``recompress``, ``gain`` and
``lyap_res_norm`` take c > NV.
"""
import contextlib
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sps

import dense_model as dm
import precond_model as pm
import saddle_model as sm
import small_ops as so
from optconpy_amd import _lib, adi_shifts

pytestmark = pytest.mark.gpu

K_TOL = 1e-6            # gain against the dense Riccati solution (the project's parity bar)
LYAP_TOL = 1e-8         # Z Z^T against the dense Lyapunov solution (test_reference_unit_test_through_dropin)
TIGHT = dict(adi_max_steps=300, adi_newZ_reltol=1e-12, nwtn_max_steps=30, nwtn_upd_reltol=1e-11,
             nwtn_upd_abstol=1e-14)      # test_hip_newton_adi_vs_dense_are_three_call_forms
CYCLE_PAIRS = [(-0.1, 1.0), (-30.0, 1.0), (-1e3, 1.0), (1.0, 0.0)]


def _say(name, check, value, bound, note=""):
    """Print one measurement beside its bound; True if it holds."""
    ok = bool(np.isfinite(value)) and value <= bound
    print("[small ops] %s | %s | %.3e | %.3e | %s%s" % (name, check, value, bound, note, "" if ok else "  MISS"))
    return ok


def _check(miss, name, check, value, bound, note=""):
    if not _say(name, check, value, bound, note):
        miss.append(check)


@contextlib.contextmanager
def _no_ricadi_warning():
    """The library's non-convergence warning (``_lib._warn_nonconverged``) becomes an error inside this block."""
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="ricadi")
        yield


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _nan(*shape):
    import torch
    t = torch.full(shape, float("nan"), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ contexts
@pytest.fixture(scope="module", params=so.NAMES)
def dev(request):
    """(operator, its context): one context per operator for the whole module (pytest runs the tests operator by
    operator), closed before the next one is made."""
    op = so.get(request.param)
    ctx = _lib.Context(0, **op.opts)
    ctx.set_operator(*op.ops)
    yield op, ctx
    ctx.close()


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A test that leaves the device in an error state ends the run: nothing more is started on it."""
    yield
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:            # pragma: no cover - only after a device fault
        pytest.exit("device error after a test, stopping: %r" % (e,), returncode=3)


class _Env:
    """Environment switches of the library for the life of one context (read when the operator is set)."""

    def __init__(self, **env):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------------ structure
def test_structure(dev):
    """Every level of the hierarchy: block lists are permutations with at most ``bs`` rows per block, aggregates
    lie in their ranges and none is empty, ``kcp <= kcv``; the level-0 plan is the host's; P is plain aggregation
    or, where ``smoothed`` is reported, ``(I - omega D^-1 sym(calA)) Y`` on the velocity rows to 1e-14."""
    op, ctx = dev
    miss = []
    plan = _lib.host_plan_levels(*op.ops, **op.opts)
    level = 0
    while True:
        try:
            st = ctx.precond_structure(level)
        except ValueError:
            break
        bad = so.structure_problems(st)
        print("[small ops] %s | structure level %d | nv %d np %d blocks %d+%d of %d, kcv %d kcp %d, smoothed %s, "
              "child %s | %s" % (op.name, level, st["nv"], st["np"], st["nbv"], st["nbp"], st["bs"], st["kcv"],
                                 st["kcp"], st["smoothed"], st["child"], bad or "ok"))
        miss += ["level %d: %s" % (level, b) for b in bad]
        if level == 0:
            assert (st["nv"], st["np"]) == (op.nv, op.np)
            assert st["bs"] == op.opts.get("bj_block", 32)
            assert (st["kcv"], st["kcp"], st["smoothed"]) == (plan["kcv"], plan["kcp"], plan["smoothed"]), (st, plan)
        if st["kc"] > 0:
            P = st["P"].toarray()
            if st["smoothed"]:
                assert level == 0
                ref = so.smoothed_prolongation(op.calA, st)
                assert np.abs(ref.sum(axis=1)[:op.nv] - 1.0).max() > 1e-3      # the reference is not plain Y
            else:
                ref = np.zeros_like(P)
                ref[np.arange(P.shape[0]), st["aggof"]] = 1.0
            if not _say(op.name, "P level %d max abs diff" % level, np.abs(P - ref).max(), 1e-14):
                miss.append("level %d: P" % level)
        if not st["child"]:
            break
        level += 1
    assert level < 6
    assert not miss, miss


# ------------------------------------------------------------------------------------------------ SpMM
def _integer_twin(op, seed=0):
    """Operator with the patterns of ``op`` and small integer values (diagonally dominant, calE symmetric), and
    its dense saddle matrix as a function of integer (alpha, beta)."""
    rng = np.random.default_rng([seed, op.nv, op.np])

    def ints(pattern):
        m = sps.csr_matrix(pattern, dtype=np.float64, copy=True)
        m.data = rng.choice([-2.0, -1.0, 1.0, 2.0], size=m.data.size)
        return m

    A = ints(op.calA)
    A = (A - sps.diags(A.diagonal()) - sps.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 1.0)).tocsr()
    T = sps.triu(ints(op.calE), 1)
    E = (T + T.T).tocsr()
    E = (E + sps.diags(np.asarray(abs(E).sum(axis=1)).ravel() + 1.0)).tocsr()
    J = ints(op.J)
    for m in (A, E, J):
        m.sort_indices()
    assert sm._pattern(A).nnz >= op.nv and abs(sm._pattern(J) - sm._pattern(op.J)).nnz == 0
    return A, E, J


@pytest.fixture(scope="module")
def twin(dev):
    """(integer operator, its context) of the current operator."""
    op, _ = dev
    ops = _integer_twin(op)
    ctx = _lib.Context(0, **op.opts)
    ctx.set_operator(*ops)
    yield ops, ctx
    ctx.close()


def _batch_product(ctx, n, al, be, X, m):
    """``op_apply_batch_dev`` on G panels; returns (Y (G x n x m), variant)."""
    G = len(al)
    Xd, Yd = _dev(X), _nan(G, n, m)
    var = ctx.op_apply_batch_dev(al, be, Xd.data_ptr(), n * m, m, Yd.data_ptr(), n * m)
    ctx.synchronize()
    return _host(Yd), var


def _spmm_checks(op, ctx, iops, ictx, m):
    from test_gpu_saddle_spmm import _expected_variant
    n = op.n
    t = _lib.host_saddle_tiles(*op.ops, **op.opts)
    rng = np.random.default_rng([m, n])
    miss, variants = [], set()
    for G in (1, 3):
        al = [-0.1, -30.0, -1e3] if G == 3 else [-30.0]
        be = [1.0, 0.37, 1.0][:G]
        X = rng.standard_normal((G, n, m))
        Y, var = _batch_product(ctx, n, al, be, X, m)
        want = _expected_variant(t, m, G, 0, None, False)
        assert var == want, (op.name, m, G, var, want)
        variants.add(var)
        for g in range(G):
            ref, bound = sm.reference(op.ops, al[g], be[g], X[g])
            _check(miss, op.name, "op_apply_batch m=%d G=%d g=%d error/bound" % (m, G, g),
                   float(np.max(sm.excess(Y[g], ref, bound))), 1.0, "variant %d" % var)
            Yh = ctx.spmm(al[g], be[g], X[g])
            _check(miss, op.name, "spmm m=%d G=%d shift %g error/bound" % (m, G, al[g]),
                   float(np.max(sm.excess(Yh, ref, bound))), 1.0)
    # integers: every product and sum is exact in FP64, whatever the order
    Xi = rng.integers(-4, 5, size=(3, n, m)).astype(np.float64)
    ali, bei = [-3.0, -2.0, 1.0], [2.0, 1.0, 0.0]      # beta A + alpha E stays diagonally dominant
    Yi, _ = _batch_product(ictx, n, ali, bei, Xi, m)
    for g in range(3):
        ref = sm.saddle(*iops, ali[g], bei[g]) @ Xi[g]
        d = max(np.abs(Yi[g] - ref).max(), np.abs(ictx.spmm(ali[g], bei[g], Xi[g]) - ref).max())
        _check(miss, op.name, "integer product m=%d (%g, %g) max abs diff" % (m, ali[g], bei[g]), d, 0.0)
    assert not miss, miss
    return variants


@pytest.mark.parametrize("m", [1, 16, 17])
def test_spmm(dev, twin, m):
    """``ctx.spmm`` and ``op_apply_batch_dev`` (G = 1, 3) against ``S @ X`` at the bound of saddle_model, the kernel
    form the launcher is expected to pick, and exact equality on integer operators and panels."""
    op, ctx = dev
    _spmm_checks(op, ctx, *twin, m)


def test_spmm_long_row_takes_the_csr_kernel():
    """The arrowhead operator's row of 201 columns is a tile of its own: it fits the tile kernel's LDS budget up to
    25 columns of the panel, so m = 16 and 17 above run tiled; at m = 32 the CSR kernel serves (variant 0)."""
    op = so.get("arrow200")
    iops = _integer_twin(op)
    with _lib.Context(0) as ctx, _lib.Context(0) as ictx:
        ctx.set_operator(*op.ops)
        ictx.set_operator(*iops)
        assert _spmm_checks(op, ctx, iops, ictx, 32) == {0}


# ------------------------------------------------------------------------------------------------ cycle
def _cycle_checks(op, ctx, label):
    """``precond_apply_batch_dev`` (m = 1, 5, 16; four (alpha, beta) pairs in one batch) and ``precond_apply``
    against the model of the context's own structure, per block (``block_errors``): where nothing is stored
    reduced, the exact model at ``tol_fp64``; else the rounded model (``rounded`` = the form the call reports) at
    ``TOL_ROUNDED``.  Returns (misses, forms that ran exact)."""
    model = pm.CycleModel.from_context(ctx, *op.ops)
    st = model.st
    miss, exact = [], []
    al, be = [a for a, _ in CYCLE_PAIRS], [b for _, b in CYCLE_PAIRS]
    G = len(al)
    t64 = {ab: pm.tol_fp64(model, *ab) for ab in CYCLE_PAIRS}
    ops_ = [model.operands(*ab) for ab in CYCLE_PAIRS]
    _check(miss, op.name, "%s block and Schur-block conditioning" % label,
           max(max(o["cond_blocks"], o.get("cond_schur", 1.0)) for o in ops_), so.COND_BLOCK_CAP,
           "with the coarse matrices %.1e, levels %d" % (max(model.conditioning(*ab) for ab in CYCLE_PAIRS),
                                                         model.levels()))
    _check(miss, op.name, "%s tol_fp64" % label, max(t64.values()), pm.TOL_ROUNDED)

    def compare(what, Z, R, ab, form):
        reduced = any(form[k] for k in ("h16", "x32", "mid32", "b16", "precond32"))
        if not reduced:
            exact.append(what)
        assert np.all(np.isfinite(Z)), (op.name, label, what, ab)
        ref = model.apply(ab[0], ab[1], R, rounded=form if reduced else None)
        _check(miss, op.name, "%s cycle %s (%g, %g) worst block error" % (label, what, ab[0], ab[1]),
               pm.worst_block_error(Z, ref, st), pm.TOL_ROUNDED if reduced else t64[ab],
               "%s model, form %s" % ("rounded" if reduced else "exact",
                                      sorted(k for k, v in form.items() if v is True)))

    for m in (1, 5, 16):
        R = np.random.default_rng([7, m, op.n]).standard_normal((G, op.n, m))
        Rd, Zd = _dev(R), _nan(G, op.n, m)
        form = ctx.precond_apply_batch_dev(al, be, Rd.data_ptr(), op.n * m, m, Zd.data_ptr())
        ctx.synchronize()
        Z = _host(Zd)
        form["precond32"] = st["precond32"]
        for g, ab in enumerate(CYCLE_PAIRS):
            compare("batch m=%d" % m, Z[g], R[g], ab, form)
    R = np.random.default_rng([8, op.n]).standard_normal((op.n, 5))
    host_form = dict(h16=False, x32=False, mid32=False, b16=False, precond32=st["precond32"])
    for ab in CYCLE_PAIRS:
        compare("host m=5", ctx.precond_apply(ab[0], ab[1], R), R, ab, host_form)
    return miss, exact


def test_cycle_default_form(dev):
    op, ctx = dev
    miss, _ = _cycle_checks(op, ctx, "default")
    assert not miss, miss


def test_cycle_fp64_form(dev):
    """The same under ``RICADI_PRECOND64=1`` (a context of its own: the switch is read when the context is made);
    the host entry then stores nothing reduced and is held to ``tol_fp64`` against the exact model."""
    op, _ = dev
    with _Env(RICADI_PRECOND64="1"):
        with _lib.Context(0, **op.opts) as ctx:
            ctx.set_operator(*op.ops)
            miss, exact = _cycle_checks(op, ctx, "fp64")
    assert "host m=5" in exact, exact
    assert not miss, miss


# ------------------------------------------------------------------------------------------------ solves
def _rhs(op, m, seed):
    R = np.random.default_rng([seed, m, op.nv]).standard_normal((op.nv, m))
    if m >= 5:
        R[:, 2] = 0.0          # a zero right-hand side inside a panel
    return R


def _solve_check(miss, op, what, a, b, X, R, its):
    """Print the figures of one solve, then hold it to ``small_ops.solve_ok``."""
    res, fwd = so.solve_errors(op, a, b, X, R)
    print("[small ops] %s | %s (%g, %g) | residual %.3e (bound %.0e), forward error %.3e (bound %.3e) | "
          "iterations %s, n = %d" % (op.name, what, a, b, res.max(), so.RES_TOL, fwd.max(),
                                     2.0 * op.cond_S(a, b) * so.RES_TOL, its, op.n))
    try:
        so.solve_ok(op, a, b, X, R)
    except AssertionError as e:
        miss.append("%s (%g, %g): %s" % (what, a, b, e))


@pytest.mark.parametrize("m", [1, 5, 17])
def test_shift_solve(dev, m):
    """``shift_solve`` against the dense LU at every shift of the family and at (1, 0): true residual <= 1e-10 per
    column, forward error <= 2 cond(S) 1e-10, finite, no non-convergence warning, a zero column stays zero."""
    op, ctx = dev
    R = _rhs(op, m, 1)
    miss = []
    with _no_ricadi_warning():
        for a, b in [(p, 1.0) for p in so.SHIFTS] + [(1.0, 0.0)]:
            X, its, _ = ctx.shift_solve(a, b, R)
            _solve_check(miss, op, "shift_solve m=%d" % m, a, b, X, R, its)
        if m == 1:
            Rz = np.zeros((op.nv, 1))
            X, its, _ = ctx.shift_solve(-1.0, 1.0, Rz)
            _solve_check(miss, op, "shift_solve zero rhs", -1.0, 1.0, X, Rz, its)
    assert not miss, miss


@pytest.mark.parametrize("m", [1, 5, 17])
@pytest.mark.parametrize("G", [1, 3, 16])
def test_shift_solve_batch(dev, G, m):
    """``shift_solve_batch_dev`` with 1, 3 (a right-hand side per shift) and 16 shifts (one shared), every shift held
    to the same assertions."""
    op, ctx = dev
    shifts = {1: [-30.0], 3: [-0.1, -30.0, -1e3], 16: list(so.SHIFTS16)}[G]
    shared = G == 16
    Rs = [_rhs(op, m, 2 + (0 if shared else g)) for g in range(G)]
    Rd = _dev(Rs[0] if shared else np.stack(Rs))
    Xd = _nan(G, op.n, m)
    with _no_ricadi_warning():
        its, _ = ctx.shift_solve_batch_dev(shifts, [1.0] * G, Rd.data_ptr(), 0 if shared else op.nv * m, m,
                                           Xd.data_ptr())
    ctx.synchronize()
    X = _host(Xd)
    miss = []
    for g, p in enumerate(shifts):
        _solve_check(miss, op, "shift_solve_batch G=%d m=%d" % (G, m), p, 1.0, X[g], Rs[g], its[g])
    assert not miss, miss


# ------------------------------------------------------------------------------------------------ projected pencil
@pytest.mark.parametrize("lowrank", [False, True], ids=["plain", "lowrank"])
def test_project_pencil(dev, twin, lowrank):
    """``project_pencil`` for k = 1, min(nv, 16), min(nv, 17), with and without a low-rank term (q = 3): exact on
    integers, bitwise repeatable, and on the real operator within the componentwise bound of a sum of
    ``nv + rowlen (+ nv + q)`` products."""
    op, ctx = dev
    iops, ictx = twin
    nv = op.nv
    miss = []
    rng = np.random.default_rng([3, nv])
    ks = sorted({1, min(nv, 16), min(nv, 17)})
    tag = "lowrank" if lowrank else "plain"
    U = V = Ui = Vi = None
    if lowrank:
        U, V = 0.1 * rng.standard_normal((nv, 3)), rng.standard_normal((nv, 3))
        Ui, Vi = (rng.integers(-2, 3, size=(nv, 3)).astype(np.float64) for _ in range(2))
        ctx.set_lowrank(U, V)
        ictx.set_lowrank(Ui, Vi)
    try:
        for k in ks:
            Qi = rng.integers(-3, 4, size=(nv, k)).astype(np.float64)
            HA, HE = ictx.project_pencil(Qi)
            Ad, Ed = iops[0].toarray(), iops[1].toarray()
            if lowrank:
                Ad = Ad - Ui @ Vi.T
            d = max(np.abs(HA - Qi.T @ Ad @ Qi).max(), np.abs(HE - Qi.T @ Ed @ Qi).max())
            _check(miss, op.name, "project_pencil %s integers k=%d max abs diff" % (tag, k), d, 0.0)
            Q = rng.standard_normal((nv, k))
            HA, HE = ctx.project_pencil(Q)
            HA2, HE2 = ctx.project_pencil(Q)
            assert np.array_equal(HA, HA2) and np.array_equal(HE, HE2), (op.name, k, "not repeatable")
            u = dm.U
            rowlen = int(np.diff(op.calA.indptr).max() + np.diff(op.calE.indptr).max())
            bA = dm.gamma(nv + rowlen + 2, u) * (np.abs(Q).T @ np.abs(op.Ad) @ np.abs(Q))
            refA = Q.T @ op.Ad @ Q
            if lowrank:
                bA = bA + dm.gamma(2 * nv + 3 + 2, u) * ((np.abs(Q).T @ np.abs(U)) @ (np.abs(V).T @ np.abs(Q)))
                refA = refA - (Q.T @ U) @ (V.T @ Q)
            bE = dm.gamma(nv + rowlen + 2, u) * (np.abs(Q).T @ np.abs(op.Ed) @ np.abs(Q))
            r = max(dm.ratio(HA, refA, 2.0 * bA), dm.ratio(HE, Q.T @ op.Ed @ Q, 2.0 * bE))
            _check(miss, op.name, "project_pencil %s k=%d error/bound" % (tag, k), float(r), 1.0)
    finally:
        if lowrank:
            ctx.set_lowrank(None, None)
            ictx.set_lowrank(None, None)
    assert not miss, miss


# ------------------------------------------------------------------------------------------------ dense step
@pytest.fixture(scope="module")
def dims_ctx():
    made = {}

    def get(nv):
        if nv not in made:
            made[nv] = _lib.Context(0)
            made[nv].set_dims(nv)
        return made[nv]

    yield get
    for ctx in made.values():
        ctx.close()


DENSE_CASES = [(nv, c) for nv in (1, 15, 33) for c in sorted({1, nv, nv + 3})]


@pytest.mark.parametrize("nv,c", DENSE_CASES)
def test_dense_step_below_one_tile(dims_ctx, nv, c):
    """``qr``, ``compress``, ``recompress`` and ``gain`` on a dimension-only context with the assertions of
    test_gpu_dense_step.py (QR residual 1e-13, orthogonality 1e-12, ``Zc Zc^T`` to 2e-14, the gain at its
    componentwise bound); ``qr`` refuses c > nv by contract and must leave its outputs alone."""
    ctx = dims_ctx(nv)
    name = "set_dims(%d)" % nv
    Z = dm.panel(31, nv, c)
    X = Z @ Z.T
    miss = []
    if c <= nv:
        Q, R = ctx.qr(Z)
        assert np.all(np.tril(R, -1) == 0)
        _check(miss, name, "qr c=%d residual" % c, np.linalg.norm(Q @ R - Z) / np.linalg.norm(Z), 1e-13)
        _check(miss, name, "qr c=%d orthogonality" % c, np.linalg.norm(Q.T @ Q - np.eye(c)), 1e-12)
    else:
        with pytest.raises(ValueError):
            ctx.qr(Z)
        Qs, Rs = np.full((nv, c), 7.0), np.full((c, c), 7.0)
        rc = ctx._lib.ricadi_qr(ctx._h, _lib._d(Z), c, _lib._d(Qs), _lib._d(Rs))
        assert rc == -1 and np.all(Qs == 7.0) and np.all(Rs == 7.0), "a refused call wrote its outputs"
    Zc, sv = ctx.compress(Z)
    assert Zc.shape == (nv, min(c, nv)) and np.all(np.isfinite(Zc))
    _check(miss, name, "compress c=%d Zc Zc^T" % c, so.rel(Zc @ Zc.T, X), 2e-14)
    s_ref = np.linalg.svd(Z, compute_uv=False)
    # include/ricadi.h: the QR route resolves singular values to eps s_1 (here 33 eps, times 10), the Gram route, which
    # serves c > nv, to sqrt(eps) s_1 = 1.5e-8 of the largest
    _check(miss, name, "compress c=%d singular values" % c, so.rel(sv[:s_ref.size], s_ref),
           1e-7 if c > nv else 1e-13)
    Zr = ctx.recompress(Z)
    assert 1 <= Zr.shape[1] <= min(c, nv) and np.all(np.isfinite(Zr))
    _check(miss, name, "recompress c=%d Zc Zc^T" % c, so.rel(Zr @ Zr.T, X), 2e-14)
    B = dm.panel(32, nv, so.NB)
    st = dm.gain_stages(Z, B)
    for kind, MT in (("identity", sps.identity(nv, format="csr")), ("sparse", dm.sparse_rows(nv, 5, seed=7))):
        K = ctx.gain(B, Z=Z, MT=MT)
        r = dm.ratio(K, dm.gain(MT, Z, B, 1.0, st), dm.tol(dm.gain_bound, MT, Z, B, 1.0, stages=st))
        _check(miss, name, "gain %s c=%d error/bound" % (kind, c), float(r), 1.0)
    assert not miss, miss


def test_lyap_res_norm(dev):
    """``lyap_res_norm`` (the squared norm) on the operator's own context for c = 1, nv, nv + 3 against the dense
    ``||P^T (calA X calE^T + calE X calA^T + W W^T) P||_F^2``, rtol 1e-7 as test_gpu_dense_step.py."""
    op, ctx = dev
    P = op.leray
    miss = []
    for c in sorted({1, op.nv, op.nv + 3}):
        Z = dm.panel(33, op.nv, c)
        X = Z @ Z.T
        R = op.Ad @ X @ op.Ed.T + op.Ed @ X @ op.Ad.T + op.W @ op.W.T
        ref = np.linalg.norm(P.T @ R @ P) ** 2
        got = ctx.lyap_res_norm(Z, op.W)
        assert ref > 0
        _check(miss, op.name, "lyap_res_norm c=%d relative difference" % c, abs(got - ref) / ref, 1e-7)
    assert not miss, miss


# ------------------------------------------------------------------------------------------------ iterations
def _lyap_check(op, ctx, label, shifts, sweep_width):
    prm = _lib.adi_params(dict(TIGHT, sweep_width=sweep_width))
    with _no_ricadi_warning():
        Z, info = ctx.lyap_adi(shifts, op.W, prm)
    assert np.all(np.isfinite(Z))
    return _say(op.name, "lyap_adi %s Z Z^T vs dense" % label, so.rel(Z @ Z.T, op.lyap()), LYAP_TOL,
                "%d steps, %d columns (nv = %d), %d shift solves, %d GMRES iterations, stopped by %s" % (
                    info["adi_steps"], info["cols"], op.nv, info["shift_solves"], info["gmres_iters"],
                    info["adi_stopped_by"]))


def test_lyap_adi(dev):
    """Step form and sweeps of four shifts: ``Z Z^T`` against the dense projected Lyapunov solution."""
    op, ctx = dev
    miss = [label for label, sw in (("step form", 1), ("sweep_width=4", 4))
            if not _lyap_check(op, ctx, label, op.shifts, sw)]
    assert not miss, miss


def test_lyap_adi_auto_shifts(dev):
    """``ms='auto'``: ``adi_shifts.auto_shifts`` on an operator whose Krylov basis cannot reach its usual width
    (nv < 128: at most nv directions, and fewer rows than ``[W0, Z_warm]`` has columns where nv < 9), then the ADI
    with those shifts to the same bar."""
    op, ctx = dev
    with _no_ricadi_warning():
        ms = adi_shifts.auto_shifts(ctx, op.W)
    print("[small ops] %s | auto_shifts | %s | %s" % (op.name, ["%.3g" % p for p in ms], ms.info))
    assert len(ms) >= 1 and all(p < 0 and np.isfinite(p) for p in ms) and len(set(ms)) == len(ms)
    assert not ms.info["fallback"] and 1 <= ms.info["basis_dim"] <= op.nv
    assert _lyap_check(op, ctx, "auto shifts", list(ms), 1)


@pytest.mark.parametrize("form", ["plain", "z0_oldB"])
def test_ric_newtonadi(dev, form):
    """Newton-ADI from zero, and from ``Z0`` with ``oldB``: the gain ``calE X B`` against
    ``identities.dense_projected_are`` (of ``calA + oldB B^T`` in the second form)."""
    op, ctx = dev
    prm = _lib.adi_params(dict(TIGHT))
    Z0, old = (None, None) if form == "plain" else (op.Z0, op.oldB)
    with _no_ricadi_warning():
        Z, info = ctx.ric_newtonadi(op.shifts, op.B, op.W, prm, Z0=Z0, oldB=old)
    K = ctx.gain(op.B)
    X = op.are(old=old is not None)
    assert np.all(np.isfinite(Z)) and np.all(np.isfinite(K))
    _say(op.name, "ric_newtonadi %s Z Z^T vs dense" % form, so.rel(Z @ Z.T, X), K_TOL)
    assert _say(op.name, "ric_newtonadi %s gain vs dense" % form, so.rel(K, op.Ed @ X @ op.B), K_TOL,
                "%d Newton steps, %d ADI steps, %d columns (nv = %d), %d shift solves, %d GMRES iterations" % (
                    info["nwtn_steps"], info["adi_steps"], info["cols"], op.nv, info["shift_solves"],
                    info["gmres_iters"]))
    assert so.rel(Z @ Z.T, X) <= K_TOL


@pytest.mark.parametrize("mode", ["cycle", "hamiltonian"])
def test_ric_radi(dev, mode):
    """RADI with the cycled list and with the shifts it generates itself (the list's first entry starts, the list
    is the fallback): the gain against ``identities.dense_projected_are``.  Three columns per step: the factor
    outgrows nv on the smallest operators."""
    op, ctx = dev
    before = ctx.set_radi_shifts(mode)
    try:
        with _no_ricadi_warning():
            Z, K, info = ctx.ric_radi(op.shifts, op.B, op.W, max_steps=200, res_reltol=1e-12)
    finally:
        ctx.set_radi_shifts(before)
    X = op.are()
    assert np.all(np.isfinite(Z)) and np.all(np.isfinite(K))
    _say(op.name, "ric_radi %s Z Z^T vs dense" % mode, so.rel(Z @ Z.T, X), K_TOL)
    assert _say(op.name, "ric_radi %s gain vs dense" % mode, so.rel(K, op.Ed @ X @ op.B), K_TOL,
                "%d steps, %d columns (nv = %d), residual %.1e, stopped by %s, %d GMRES iterations, %d fallbacks" % (
                    info["radi_steps"], info["cols"], op.nv, info["res_rel"], info["stop_rule"], info["gmres_iters"],
                    ctx.radi_shift_fallbacks()))
    assert so.rel(Z @ Z.T, X) <= K_TOL
