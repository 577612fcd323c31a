"""GPU tests of the complex-shift path (ricadi_cplx.hip, solver_cplx.inl, lqgbt.freq_response)
against the FP64 model of tests/cplx_model.py and dense complex references, on the tiny and irregular operators of
tests/small_ops.py, the N = 4 finite-element operator and -- for one full-width launch of the tiled product -- cfg2's
operator (N = 58).  The product also runs on the operators that reach what the family does not: rows longer than the 48
entries a tile row keeps in registers (tiled form), the two sides of ``max_cols <= 160``, a CSR case without constraints
and several groups per ``grid.y`` slot; the CGS2 entry on more than one chunk of 32 basis vectors, on a column with
nothing left over and on a narrow call after a wide one.  The GMRES cycle's own kernels have
tests/test_gpu_cplx_steps.py.  Every check prints ``[cplx] operator | check | measured | bound`` before it asserts.

tests/test_cplx_model_cpu.py holds the model to its references; it has to pass for these to mean anything.
"""

import numpy as np
import pytest

import cplx_model as cm
import small_ops as so
from optconpy_amd import _lib, backend, lqgbt
from optconpy_amd import problems as pb

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
RES_TOL = so.RES_TOL
SHIFTS3 = (-0.1j, -30 + 30j, -1e3 - 300j)
SHIFTS16 = tuple(-1j * np.logspace(-1.0, 3.0, 16))


def _say(name, check, value, bound):
    ok = bool(np.isfinite(value)) and value <= bound
    print("[cplx] %s | %s | %.3e | %.3e%s" % (name, check, value, bound, "" if ok else "  MISS"))
    return ok


def _cdev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.complex128)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A test that leaves the device in an error state ends the run: nothing more is started on it."""
    yield
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:            # pragma: no cover - only after a device fault
        pytest.exit("device error after a test, stopping: %r" % (e,), returncode=3)


class _Fe4:
    """The N = 4 finite-element operator with the attributes of a SmallOp the product test uses."""
    name, opts = "fe4", {}

    def __init__(self):
        self.calA, self.calE, self.J = so.finite_element(4)
        self.ops = (self.calA, self.calE, self.J)
        self.nv, self.np = self.calA.shape[0], self.J.shape[0]
        self.n = self.nv + self.np


def _operator(name):
    return _Fe4() if name == "fe4" else so.get(name)


@pytest.fixture(scope="module", params=so.NAMES)
def dev(request):
    """(operator, its context): one context per operator of the small family for the whole module, closed before the
    next one is made."""
    op = so.get(request.param)
    ctx = _lib.Context(0, **op.opts)
    ctx.set_operator(*op.ops)
    yield op, ctx
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. the product
def _product_case(op, ctx, mc, ng, active, seed):
    """One call of the complex product on padded panels; returns (worst error / bound, variant)."""
    rng = np.random.default_rng(seed)
    rows = op.n + 3                                    # group stride above n * mc
    alphas = [SHIFTS3[g % 3] for g in range(ng)]
    betas = [1.0, 0.5, 1.0, 2.0, 1.0][:ng]
    act = list(range(ng)) if active is None else active
    X = np.full((ng, rows, mc), np.nan + 1j * np.nan)
    for g in act:
        X[g, :op.n] = _crandn(rng, op.n, mc)
    Xd = _cdev(X)
    outs, variants = [], []
    for _ in range(2):
        Yd = _cdev(np.full((ng, rows, mc), np.nan + 1j * np.nan))
        _, var = ctx.op_apply_cplx_batch_dev(alphas, Xd, betas=betas, Y_t=Yd, active=active)
        outs.append(_host(Yd))
        variants.append(var)
    Y = outs[0]
    assert np.array_equal(outs[0].view(np.float64), outs[1].view(np.float64), equal_nan=True), "not bitwise repeatable"
    assert variants[0] == variants[1]
    worst = 0.0
    for g in range(ng):
        if g not in act:
            assert np.all(np.isnan(Y[g].real)) and np.all(np.isnan(Y[g].imag)), "an inactive group was written"
            continue
        assert np.all(np.isnan(Y[g, op.n:].real)), "rows behind the panel were written"
        ref, bound = cm.product(op.ops, alphas[g], betas[g], X[g, :op.n])
        assert np.all(np.isfinite(Y[g, :op.n].view(np.float64)))
        worst = max(worst, float(np.max(np.abs(Y[g, :op.n] - ref) / np.maximum(bound, np.finfo(float).tiny))))
    return worst, variants[0]


def _product_checks(op, ctx):
    """Every entry within ``4 (k + 2) eps (|beta| |A| + |alpha| |E| + |J|) |x|`` of the model (cplx_model's derivation),
    mc in {1, 3, 8}, one group and five groups with two inactive, group strides above the panel, NaN behind the panels
    and in the inactive groups (neither is written); bitwise equal on a second call; the form that ran is the tiled
    one exactly where the host setup builds the multi-shift tiles."""
    want = 1 if _lib.host_saddle_tiles(*op.ops, **op.opts)["ms_ok"] else 2
    miss = []
    for mc in (1, 3, 8):
        for ng, active in ((1, None), (5, [0, 2, 4])):
            worst, var = _product_case(op, ctx, mc, ng, active, seed=100 * mc + ng)
            if not _say(op.name, "product mc %d ng %d form %d: error / bound" % (mc, ng, var), worst, 1.0):
                miss.append((mc, ng, worst))
            assert var == want, (op.name, var, want)
    assert not miss, miss


def test_product_entry_by_entry(dev):
    """The product on every operator of the small family (the checks: _product_checks)."""
    _product_checks(*dev)


def test_product_entry_by_entry_fe4():
    """... and on the N = 4 finite-element operator."""
    op = _Fe4()
    with _lib.Context(0) as ctx:
        ctx.set_operator(*op.ops)
        _product_checks(op, ctx)


def test_both_product_forms_occur():
    """The family exercises both forms: some operator has the multi-shift tiles (tiled form) and some has not (CSR)."""
    forms = {name: _lib.host_saddle_tiles(*_operator(name).ops, **_operator(name).opts)["ms_ok"]
             for name in so.NAMES + ["fe4"]}
    print("[cplx] tiled:", sorted(k for k, v in forms.items() if v), "| CSR:", sorted(k for k, v in forms.items() if not v))
    assert any(forms.values()) and not all(forms.values())


def test_product_full_width_at_cfg2():
    """N = 58 (cfg2's operator): ng = 16, mc = 8 in one launch reaches the tiled form at full width, entry by entry
    within the bound and bitwise repeatable."""
    calA, calE, J = so.finite_element(58)
    n = calA.shape[0] + J.shape[0]
    rng = np.random.default_rng(58)
    alphas = list(SHIFTS16)
    X = _crandn(rng, 16, n, 8)
    with _lib.Context(0) as ctx:
        ctx.set_operator(calA, calE, J)
        Xd = _cdev(X)
        Y1, var = ctx.op_apply_cplx_batch_dev(alphas, Xd)
        Y2, _ = ctx.op_apply_cplx_batch_dev(alphas, Xd)
        Y1, Y2 = _host(Y1), _host(Y2)
    assert var == 1
    assert np.array_equal(Y1.view(np.float64), Y2.view(np.float64))
    worst = 0.0
    for g in (0, 7, 15):
        ref, bound = cm.product((calA, calE, J), alphas[g], 1.0, X[g])
        worst = max(worst, float(np.max(np.abs(Y1[g] - ref) / bound)))
    assert _say("fe58", "tiled product ng 16 mc 8: error / bound", worst, 1.0)


class _Op:
    """(calA, calE, J) with the attributes of a SmallOp that _product_checks uses."""

    def __init__(self, name, ops, **opts):
        self.name, self.ops, self.opts = name, ops, opts
        self.nv, self.np = ops[0].shape[0], ops[2].shape[0]
        self.n = self.nv + self.np


def _tile_row_lengths(tiles):
    return np.diff(tiles["rp2"], axis=1).ravel()


def test_product_long_rows_on_the_tiled_form():
    """The streamed tail of the tiled product (entries from the 49th of a row on), which no operator of the small
    family reaches (their longest tile row has 45 entries; the arrowhead operator takes the CSR form): the ``long100``
    operator of test_gpu_saddle_spmm.py with a 48 added -- rows of exactly 48 (registers only), 49 (one streamed
    entry), 64 and 100 entries and a pressure row of 60, tiled form."""
    ops, rows = cm.long_row_operator()
    op = _Op("long100+48", ops)
    tiles = _lib.host_saddle_tiles(*ops)
    lens = _tile_row_lengths(tiles)
    print("[cplx] %s | n %d, widened rows %s, longest tile rows %s, max_cols %d" %
          (op.name, op.n, rows, sorted(lens)[-5:], tiles["max_cols"]))
    assert tiles["ms_ok"] and op.n == 1937 and lens.max() == 100 and np.sum(lens == 48) >= 1 and np.sum(lens == 49) >= 1
    with _lib.Context(0) as ctx:
        ctx.set_operator(*ops)
        _product_checks(op, ctx)


@pytest.mark.parametrize("nv,seed,tiled", [(160, 860, True), (161, 861, False)])
def test_product_at_the_max_cols_boundary(nv, seed, tiled):
    """The two sides of the rule ``max_cols <= 160`` of the tiled form: the arrowhead operator with 160 unknowns has
    one row of 160 entries and row blocks of 160 columns (tiled, 112 streamed entries in one row); with 161 it takes
    the CSR form -- the one CSR case without constraints (np = 0)."""
    op = _Op("arrow%d" % nv, so.synthetic(nv=nv, np_=0, seed=seed, arrow=True, lumped=True))
    tiles = _lib.host_saddle_tiles(*op.ops)
    assert tiles["max_cols"] == nv and tiles["ms_ok"] == tiled and _tile_row_lengths(tiles).max() == nv and op.np == 0
    with _lib.Context(0) as ctx:
        ctx.set_operator(*op.ops)
        _product_checks(op, ctx)


@pytest.mark.parametrize("active", [list(range(0, 16, 2)), None], ids=["every-second-group", "all-groups"])
def test_product_several_groups_per_slot(active):
    """nv65_np24 (tiled, 4 row blocks), ng = 16, mc = 8, every active group compared entry by entry.  The tiled launch
    splits the active groups over at most 8 ``grid.y`` slots: the eight groups 0, 2, .. 14 get a slot each, gathered
    through the group table; all sixteen give every slot two groups, which reuse the one LDS tile between the two
    barriers."""
    op = so.get("nv65_np24")
    rng = np.random.default_rng(160)
    alphas, betas = list(SHIFTS16), list(1.0 + 0.125 * np.arange(16))
    act = list(range(16)) if active is None else active
    X = np.full((16, op.n, 8), np.nan + 1j * np.nan)
    X[act] = _crandn(rng, len(act), op.n, 8)
    assert _lib.host_saddle_tiles(*op.ops, **op.opts)["ms_ok"]
    with _lib.Context(0, **op.opts) as ctx:
        ctx.set_operator(*op.ops)
        Xd = _cdev(X)
        outs = []
        for _ in range(2):
            Yd = _cdev(np.full(X.shape, np.nan + 1j * np.nan))
            _, var = ctx.op_apply_cplx_batch_dev(alphas, Xd, betas=betas, Y_t=Yd, active=active)
            outs.append(_host(Yd))
            assert var == 1
    Y = outs[0]
    assert np.array_equal(outs[0].view(np.float64), outs[1].view(np.float64), equal_nan=True), "not bitwise repeatable"
    worst = 0.0
    for g in range(16):
        if g not in act:
            assert np.all(np.isnan(Y[g].view(np.float64))), "an inactive group was written"
            continue
        ref, bound = cm.product(op.ops, alphas[g], betas[g], X[g])
        assert np.all(np.isfinite(Y[g].view(np.float64)))
        worst = max(worst, float(np.max(np.abs(Y[g] - ref) / np.maximum(bound, np.finfo(float).tiny))))
    assert _say(op.name, "product ng 16 mc 8, %d active groups: error / bound" % len(act), worst, 1.0)


# ------------------------------------------------------------------------------------------------ 7. the CGS2 step
@pytest.fixture(scope="module", params=[3, 61, 450, 1937])
def orth_ctx(request):
    """A context whose operator has n rows (no constraints): the CGS2 entry works on panels of the resident n."""
    n = request.param
    calA, calE, J = so.synthetic(nv=n, np_=0, seed=700 + n, lumped=True)
    ctx = _lib.Context(0)
    ctx.set_operator(calA, calE, J)
    yield n, ctx
    ctx.close()


@pytest.mark.parametrize("ng", [1, 3])
@pytest.mark.parametrize("mc", [1, 8])
@pytest.mark.parametrize("nvec", [1, 2, 9, 31, 32, 33, 70])
def test_cgs2_step(orth_ctx, nvec, mc, ng):
    """One CGS2 step against an orthonormal basis (NumPy QR, per group and column): the new vector is orthogonal to the
    basis to ``8 n eps``, ``w_in = V h + h_last w_out`` to ``8 (nvec + 2) n eps ||w_in||``, the coefficients within the
    model's bound of ``V^H w`` (cplx_model.cgs2_coef_bound), bitwise twice.  Where nvec >= n (n = 3, nvec = 9) an
    orthonormal basis that leaves something over has at most n - 1 vectors: that many are used (n = 61 runs 31, 32,
    33 and 60).  The dot pass walks the basis in chunks of 32: 31 and 32 fill one chunk, 33 and 70 start a second and
    a third one (a partial one each), which reuse the LDS staging of the first."""
    n, ctx = orth_ctx
    nv_ = min(nvec, n - 1)
    rng = np.random.default_rng(1000 * n + 100 * nvec + 10 * mc + ng)
    V = np.zeros((nv_, ng, n, mc), dtype=np.complex128)
    for g in range(ng):
        for c in range(mc):
            Q, _ = np.linalg.qr(_crandn(rng, n, nv_))
            V[:, g, :, c] = Q.T
    W = _crandn(rng, ng, n, mc)
    Vd = _cdev(V)
    outs = []
    for _ in range(2):
        Wd = _cdev(W)
        H = ctx.cplx_orth_dev(Vd, Wd)
        outs.append((_host(H), _host(Wd)))
    assert np.array_equal(outs[0][0].view(np.float64), outs[1][0].view(np.float64))
    assert np.array_equal(outs[0][1].view(np.float64), outs[1][1].view(np.float64))
    H, Wo = outs[0]
    assert np.all(np.isfinite(H.view(np.float64))) and np.all(np.isfinite(Wo.view(np.float64)))
    worst = dict(orth=0.0, recon=0.0, coef=0.0)
    for g in range(ng):
        Vg = V[:, g]
        exact, bound = cm.cgs2_coef_bound(Vg, W[g])
        worst["coef"] = max(worst["coef"], float(np.max(np.abs(H[g, :nv_] - exact) / bound)))
        assert np.all(H[g, nv_].imag == 0.0) and np.all(H[g, nv_].real > 0.0)
        for c in range(mc):
            Vc = Vg[:, :, c].T
            worst["orth"] = max(worst["orth"], float(np.linalg.norm(Vc.conj().T @ Wo[g, :, c]) / (8 * n * EPS)))
            rec = W[g, :, c] - Vc @ H[g, :nv_, c] - H[g, nv_, c] * Wo[g, :, c]
            worst["recon"] = max(worst["recon"], float(np.linalg.norm(rec) /
                                                       (8 * (nv_ + 2) * n * EPS * np.linalg.norm(W[g, :, c]))))
    ok = [_say("n %d" % n, "cgs2 nvec %d mc %d ng %d: %s / bound" % (nv_, mc, ng, k), v, 1.0) for k, v in worst.items()]
    assert all(ok), worst


def _orth_basis(rng, nvec, ng, n, mc):
    V = np.zeros((nvec, ng, n, mc), dtype=np.complex128)
    for g in range(ng):
        for c in range(mc):
            V[:, g, :, c] = np.linalg.qr(_crandn(rng, n, nvec))[0].T
    return V


def test_cgs2_nothing_left(orth_ctx):
    """A column with nothing left over goes through the CGS2 entry: column 0 of group 0 is zero -- its coefficients
    and ``h_last`` are exactly zero and the returned vector is exactly zero, not NaN --, column 1 of group 1 lies in
    the span of the basis up to rounding (``W = V c``): its coefficients are within the model's bound of ``c``,
    ``h_last`` is at rounding level (``8 (nvec + 2) n eps ||w||``; no bar on the direction of what is left), and every
    returned value of either case is finite.  The other columns are ordinary and meet the bars of test_cgs2_step."""
    n, ctx = orth_ctx
    nvec, ng, mc = min(9, n - 1), 2, 3
    rng = np.random.default_rng(5000 + n)
    V = _orth_basis(rng, nvec, ng, n, mc)
    W = _crandn(rng, ng, n, mc)
    W[0, :, 0] = 0.0
    coef = _crandn(rng, nvec)
    W[1, :, 1] = V[:, 1, :, 1].T @ coef
    Wd = _cdev(W)
    H = _host(ctx.cplx_orth_dev(_cdev(V), Wd))
    Wo = _host(Wd)
    assert np.all(np.isfinite(H.view(np.float64))) and np.all(np.isfinite(Wo.view(np.float64)))
    assert np.all(H[0, :, 0] == 0.0) and np.all(Wo[0, :, 0] == 0.0), "a zero column did not come back as zeros"
    assert np.all(H[:, nvec].imag == 0.0) and np.all(H[:, nvec].real >= 0.0)
    worst = 0.0
    for g in range(ng):
        exact, bound = cm.cgs2_coef_bound(V[:, g], W[g])
        err = np.abs(H[g, :nvec] - exact)
        worst = max(worst, float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(bound, np.finfo(float).tiny)))))
    ok = _say("n %d" % n, "cgs2 zero / in-span columns: coef / bound", worst, 1.0)
    wn = float(np.linalg.norm(W[1, :, 1]))
    ok &= _say("n %d" % n, "cgs2 in-span column: h_last", float(H[1, nvec, 1].real), 8 * (nvec + 2) * n * EPS * wn)
    for g, c in ((0, 1), (0, 2), (1, 0), (1, 2)):
        Vc = V[:, g, :, c].T
        ok &= _say("n %d" % n, "cgs2 ordinary column (%d, %d): orth / bound" % (g, c),
                   float(np.linalg.norm(Vc.conj().T @ Wo[g, :, c]) / (8 * n * EPS)), 1.0)
        assert H[g, nvec, c].real > 0.0
    assert ok


def test_cgs2_narrow_call_after_a_wide_one():
    """The workspaces only grow: after a call with nvec = 40 the row stride of the coefficient arrays (41 rows) is
    larger than the 3 rows a call with nvec = 2 fills.  The narrow call's result on that context is bitwise the
    result on a fresh context."""
    n, ng, mc = 61, 3, 8
    rng = np.random.default_rng(4002)
    V40, V2 = _orth_basis(rng, 40, ng, n, mc), _orth_basis(rng, 2, ng, n, mc)
    W40, W2 = _crandn(rng, ng, n, mc), _crandn(rng, ng, n, mc)
    ops = so.synthetic(nv=n, np_=0, seed=700 + n, lumped=True)

    def narrow(wide_first):
        with _lib.Context(0) as ctx:
            ctx.set_operator(*ops)
            if wide_first:
                assert np.all(np.isfinite(_host(ctx.cplx_orth_dev(_cdev(V40), _cdev(W40))).view(np.float64)))
            Wd = _cdev(W2)
            H = _host(ctx.cplx_orth_dev(_cdev(V2), Wd))
            return H, _host(Wd)

    (H1, W1), (H0, W0) = narrow(True), narrow(False)
    assert np.all(np.isfinite(H0.view(np.float64))) and np.all(H0[:, 2].real > 0.0)
    assert np.array_equal(H1.view(np.float64), H0.view(np.float64)), "coefficients differ after a wide call"
    assert np.array_equal(W1.view(np.float64), W0.view(np.float64)), "unit vectors differ after a wide call"


# ------------------------------------------------------------------------------------------------ 8. the solve
def _dense_cplx(op, alpha):
    S = cm.saddle_cplx(*op.ops, alpha, 1.0).toarray()
    return S, float(np.linalg.cond(S))


def _solve_ok(op, alpha, X, R, label):
    """small_ops.solve_ok carried to a complex shift; returns the messages of what it missed."""
    S, cond = _dense_cplx(op, alpha)
    rhs = np.vstack([R, np.zeros((op.np, R.shape[1]))])
    miss = []
    if not np.all(np.isfinite(X.view(np.float64))):
        return ["%s: not finite" % label]
    zero = np.linalg.norm(R, axis=0) == 0
    if not np.all(X[:, zero] == 0.0):
        miss.append("%s: a zero right-hand side gave a non-zero solution" % label)
    bn = np.linalg.norm(rhs, axis=0)
    res = float(np.max(np.linalg.norm(S @ X - rhs, axis=0) / np.where(bn > 0, bn, 1.0)))
    Xref = np.linalg.solve(S, rhs)
    Xref = Xref + np.linalg.solve(S, rhs - S @ Xref)
    xn = np.linalg.norm(Xref, axis=0)
    fwd = float(np.max(np.linalg.norm(X - Xref, axis=0) / np.where(xn > 0, xn, 1.0)))
    if not _say(op.name, "%s residual" % label, res, RES_TOL):
        miss.append("%s: residual %.3e" % (label, res))
    if not _say(op.name, "%s forward error" % label, fwd, 2.0 * cond * RES_TOL):
        miss.append("%s: forward error %.3e" % (label, fwd))
    return miss


def _rhs3(op, ng, seed):
    """Random complex right-hand sides (ng, nv, 3) with the middle column zero."""
    R = _crandn(np.random.default_rng(seed), ng, op.nv, 3)
    R[:, :, 1] = 0.0
    return R


def test_solve_seven_shifts(dev):
    """The seven shifts of the CPU experiment in one batch, mc = 3, a right-hand side per group with one zero column:
    finite, zero column in gives zero column out, true residual <= 1e-10, forward error against the dense complex LU
    <= 2 cond(S(alpha, 1)) 1e-10; the residuals the entry reports are the true ones."""
    op, ctx = dev
    R = _rhs3(op, 7, 21)
    X, its, rr = ctx.shift_solve_cplx_batch_dev(cm.SHIFTS7, _cdev(R))
    X = _host(X)
    print("[cplx] %s | iterations %s | reported residual %.3e" % (op.name, its, rr.max()))
    miss = []
    for g, alpha in enumerate(cm.SHIFTS7):
        miss += _solve_ok(op, alpha, X[g], R[g], "alpha %s" % (alpha,))
    assert rr.shape == (7, 3) and rr.max() <= RES_TOL and np.all(rr[:, 1] == 0.0)
    assert not miss, miss


def test_solve_sixteen_shifts_one_rhs(dev):
    """Sixteen distinct shifts -i logspace(-1, 3, 16) sharing one right-hand side (r_stride = 0), the widest batch."""
    op, ctx = dev
    R = _rhs3(op, 1, 22)[0]
    X, its, rr = ctx.shift_solve_cplx_batch_dev(SHIFTS16, _cdev(R))
    X = _host(X)
    print("[cplx] %s | iterations %s | reported residual %.3e" % (op.name, its, rr.max()))
    miss = []
    for g, alpha in enumerate(SHIFTS16):
        miss += _solve_ok(op, alpha, X[g], R, "w %.3g" % abs(alpha))
    assert not miss, miss


def test_solve_restarts():
    """``gmres_restart = 8`` on nv65_np24: cycles end and restart -- some group needs more than 8 iterations -- and the
    solutions meet the same bars."""
    op = so.get("nv65_np24")
    R = _rhs3(op, 7, 23)
    with _lib.Context(0, gmres_restart=8, **op.opts) as ctx:
        ctx.set_operator(*op.ops)
        X, its, rr = ctx.shift_solve_cplx_batch_dev(cm.SHIFTS7, _cdev(R))
        X = _host(X)
    print("[cplx] nv65_np24 restart 8 | iterations %s" % (its,))
    assert max(its) > 8
    miss = []
    for g, alpha in enumerate(cm.SHIFTS7):
        miss += _solve_ok(op, alpha, X[g], R[g], "restart 8, alpha %s" % (alpha,))
    assert not miss, miss


# ------------------------------------------------------------------------------------------------ 9. conjugation
def test_conjugation(dev):
    """The solution at conj(alpha) with conj(R) is the conjugate, within the two solves' forward-error bounds."""
    op, ctx = dev
    R = _rhs3(op, 1, 24)[0]
    alpha = -30 + 30j
    X1, _, _ = ctx.shift_solve_cplx_batch_dev([alpha], _cdev(R))
    X2, _, _ = ctx.shift_solve_cplx_batch_dev([np.conj(alpha)], _cdev(np.conj(R)))
    X1, X2 = _host(X1)[0], _host(X2)[0]
    _, cond = _dense_cplx(op, alpha)
    nz = [0, 2]
    dist = float(np.max(np.linalg.norm(X2[:, nz] - np.conj(X1[:, nz]), axis=0) / np.linalg.norm(X1[:, nz], axis=0)))
    assert _say(op.name, "conjugate solve distance", dist, 4.0 * cond * RES_TOL)


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals_leave_the_context_usable():
    """``Re alpha > 0``, ``alpha = 0``, mc = 9, ng = 17 and a low-rank term are refused with ValueError by the solve and
    the product; after each refusal the product gives bitwise what it gave before."""
    import torch
    op = so.get("unsym")
    rng = np.random.default_rng(31)
    with _lib.Context(0, **op.opts) as ctx:
        ctx.set_operator(*op.ops)
        Xd = _cdev(_crandn(rng, 1, op.n, 3))
        before = _host(ctx.op_apply_cplx_batch_dev([-1j], Xd)[0])

        def still_fine():
            assert np.array_equal(_host(ctx.op_apply_cplx_batch_dev([-1j], Xd)[0]).view(np.float64),
                                  before.view(np.float64))

        R3, R9 = _cdev(_crandn(rng, op.nv, 3)), _cdev(_crandn(rng, op.nv, 9))
        for alphas, R in (([1.0 - 1j], R3), ([0j], R3), ([-1j], R9), ([-1j * (g + 1) for g in range(17)], R3)):
            with pytest.raises(ValueError):
                ctx.shift_solve_cplx_batch_dev(alphas, R)
            still_fine()
        for alphas, X in (([1e-9 + 5j], Xd), ([0j], Xd), ([-1j], _cdev(_crandn(rng, 1, op.n, 9))),
                          ([-1j] * 17, _cdev(_crandn(rng, 17, op.n, 1)))):
            with pytest.raises(ValueError):
                ctx.op_apply_cplx_batch_dev(alphas, X)
            still_fine()
        ctx.set_lowrank(rng.standard_normal((op.nv, 2)), rng.standard_normal((op.nv, 2)))
        with pytest.raises(ValueError):
            ctx.shift_solve_cplx_batch_dev([-1j], R3)
        with pytest.raises(ValueError):
            ctx.op_apply_cplx_batch_dev([-1j], Xd)
        ctx.set_lowrank(None, None)
        still_fine()
        X, _, rr = ctx.shift_solve_cplx_batch_dev([-1j], R3)
        assert rr.max() <= RES_TOL and torch.isfinite(torch.view_as_real(X)).all()


# ------------------------------------------------------------------------------------------------ 11. the real path
def test_real_path_unchanged(monkeypatch):
    """On one context a real batched solve before and after a complex solve returns bitwise the same X (recycling
    off): the complex workspaces and the proxies' cache entries change nothing a real call computes."""
    import torch
    monkeypatch.setenv("RICADI_RECYCLE", "0")
    op = so.get("stiff_grid")
    rng = np.random.default_rng(41)
    al, be = np.array(so.SHIFTS), np.ones(len(so.SHIFTS))
    Rr = torch.from_numpy(rng.standard_normal((op.nv, 4))).to("cuda:0")
    with _lib.Context(0, **op.opts) as ctx:
        ctx.set_operator(*op.ops)
        ctx.set_recycle(0)

        def real_solve():
            X = torch.full((al.size, op.n, 4), float("nan"), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            ctx.shift_solve_batch_dev(al, be, Rr.data_ptr(), 0, 4, X.data_ptr())
            return _host(X)

        first = real_solve()
        _, _, rr = ctx.shift_solve_cplx_batch_dev(SHIFTS16, _cdev(_crandn(rng, op.nv, 8)))
        assert rr.max() <= RES_TOL
        second = real_solve()
    assert np.all(np.isfinite(first)) and np.array_equal(first, second)


# ------------------------------------------------------------------------------------------------ 12. freq_response
OMEGAS20 = np.logspace(-1.0, 3.0, 20)


def _dense_response(op, B, Cm, w):
    """(G, bound): the dense transfer function and the entrywise bound ``2 cond 1e-10 ||C|| ||V||`` of the device's."""
    S, cond = _dense_cplx(op, -1j * w)
    rhs = np.vstack([-B.astype(np.complex128), np.zeros((op.np, B.shape[1]))])
    V = np.linalg.solve(S, rhs)
    V = (V + np.linalg.solve(S, rhs - S @ V))[:op.nv]
    return Cm @ V, 2.0 * cond * RES_TOL * np.linalg.norm(Cm, 2) * np.linalg.norm(V)


@pytest.mark.parametrize("name", ["fe3", "unsym", "stiff_grid"])
def test_freq_response_against_dense(name):
    """Twenty frequencies -- more than one batch, a ragged last one -- entrywise within ``2 cond 1e-10 ||C|| ||V||`` of
    the dense transfer function; ``info`` reports converged solves; bad frequencies are refused."""
    op = so.get(name)
    B, Cm = op.B, op.W.T
    backend.reset()
    G, d = lqgbt.freq_response(op.calE, op.calA, op.J, B, Cm, OMEGAS20, info=True)
    assert G.shape == (20, Cm.shape[0], B.shape[1]) and G.dtype == np.complex128
    assert d["iters"].shape == (20,) and d["iters"].min() >= 1 and d["relres"].max() <= RES_TOL
    worst = 0.0
    for k, w in enumerate(OMEGAS20):
        ref, bound = _dense_response(op, B, Cm, w)
        worst = max(worst, float(np.max(np.abs(G[k] - ref)) / bound))
    assert _say(name, "freq_response: error / bound", worst, 1.0)
    print("[cplx] %s | iterations per frequency %s" % (name, d["iters"].tolist()))
    for bad in ([1.0, 0.0], [-1.0], [np.inf], [np.nan], []):
        with pytest.raises(ValueError):
            lqgbt.freq_response(op.calE, op.calA, op.J, B, Cm, bad)
    backend.reset()


# ------------------------------------------------------------------------------------------------ 13. reduction_error
@pytest.mark.parametrize("name", ["nv65_np24", "arrow200"])
def test_reduction_error_end_to_end(name):
    """Balanced truncation to order 3 from the device's Lyapunov factors, then ``reduction_error``: ``err`` equals the
    curve of the dense full transfer function with the same reduced matrices within the solves' bound, and
    ``hinf_lower <= 2 sum_{i > 3} hsv_i`` with hsv as the device returned it (the dense route leaves >= 22 % slack on
    these two operators)."""
    from oracle import lin_alg_utils as olau
    op = so.get(name)
    M, A, J = op.calE, op.calA, op.J
    B = np.ascontiguousarray(olau.app_prj_via_sadpnt(amat=M, jmat=J, rhsv=op.B, transposedprj=True))
    Ct = np.ascontiguousarray(olau.app_prj_via_sadpnt(amat=M, jmat=J, rhsv=op.W, transposedprj=True))
    Cm = np.ascontiguousarray(Ct.T)
    backend.reset()
    d = dict(pb.default_nwtn_adi_dict(), ms=op.shifts, adi_max_steps=300, adi_newZ_reltol=1e-12)
    red = lqgbt.lqgbt_reduce(M, A, J, B, Cm, radi_dict=d, gramians="lyapunov", order=3)
    assert red["order"] == 3
    om = np.logspace(-2.0, 4.0, 13)
    out = lqgbt.reduction_error(M, A, J, B, Cm, red, om)
    assert np.array_equal(out["omegas"], om) and out["err"].shape == out["full"].shape == (13,)
    Gr = lqgbt.reduced_freq_response(red, om)
    worst = 0.0
    for k, w in enumerate(om):
        ref, bound = _dense_response(op, B, Cm, w)
        bound *= np.sqrt(ref.size)                       # entrywise bound -> bound of the 2-norm of the difference
        worst = max(worst, abs(out["err"][k] - np.linalg.norm(ref - Gr[k], 2)) / bound,
                    abs(out["full"][k] - np.linalg.norm(ref, 2)) / bound)
    assert _say(name, "reduction_error: |err - model curve| / bound", worst, 1.0)
    tail = 2.0 * float(np.sum(red["hsv"][3:]))
    assert out["hinf_lower"] == out["err"].max()
    assert _say(name, "hinf_lower against 2 sum hsv_i, i > 3", out["hinf_lower"], tail)
    assert out["hinf_lower"] >= 1e-3 * tail
    backend.reset()
