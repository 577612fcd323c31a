"""A context that changes operators against a fresh one, bit for bit.

The product runs on ONE process-wide context (``backend.context_for`` / ``backend.context_dims``) whose operator is
replaced several times per time step of the DRE sweep, between the two Riccati solves of ``lqgbt_reduce`` and from one
benchmark configuration to the next.  Here a veteran context runs the whole battery of tests/context_battery.py on one
operator after another; at every position a fresh context with the same options runs the same battery, and the two
are compared (one test per position and battery section, the veteran advancing in order):

* an output must be bitwise equal (``np.array_equal``; integers, strings and histories equal) -- the solves are
  iterative and start from zero on either context: same operator, same bits -- unless ``CONTROL_TABLE`` names it AND
  the cause named there applies to the operator and the run (``allowed``);
* an output the table allows to differ (its bits depend on the order of FP64 atomics) must, on the veteran, meet the
  bound against the dense FP64 reference that tests/test_gpu_small_ops.py applies to a fresh
  context (``context_battery.BOUNDS``: the comparators of small_ops.py, ``RES_TOL``, ``LYAP_TOL``, ``K_TOL``).  No new
  tolerance.

``test_control`` runs the battery on two fresh contexts and fails if anything outside the table differs between them,
so the table cannot hide a defect of the reuse: it is fixed by the control, not by the sequences.

Every line ``[context reuse] ...`` printed before an assertion is a measurement (profiles/context_reuse_gpu.md).
"""
import time

import numpy as np
import pytest
import scipy.sparse as sps

import context_battery as cb
import small_ops as so
from optconpy_amd import _lib
from test_gpu_small_ops import LYAP_TOL, TIGHT, _stop_after_a_device_error  # noqa: F401 - the fixture is autouse

pytestmark = pytest.mark.gpu

_ATOMICS = ("gemm_tn_kernel adds the partial tiles of its row slices with FP64 atomics; with three or more slices the "
            "sum depends on their order")
_RECOMPRESSED = ("the factor is recompressed (compress_pchol_exec: H = R R^T is a gemm_tn product over the factor's "
                 "columns, hundreds of rows, so several slices on every operator): " + _ATOMICS)
_ROWS = ("a gemm_tn product of panels with nv rows -- launch_gemm_tn_b cuts thin products into slices of 64 rows, so "
         "three or more slices from 129 rows on: " + _ATOMICS)


def _always(op, out):
    return True


def _rows129(op, out):
    return op.nv >= 129


# output -> (why two fresh contexts need not agree on its bits, where that cause applies).  The unconditional entries
# are what the control shows: the outputs of ric_newtonadi, which recompresses its factor after every Newton step,
# differ between two fresh contexts, on one control operator or on both (profiles/context_reuse_gpu.md); its trace
# counts the solves of the second step, which starts from the recompressed iterate.  The other entries are read from
# the code and apply only where their cause does: on an operator with fewer than 129 velocity rows, and for a RADI call
# that did not recompress, these outputs must be bitwise like everything else.  Nothing of spmm / precond_apply / plain
# shift_solve / ric_radi may be named (tests/test_context_reuse_cpu.py checks the table).
CONTROL_TABLE = {
    "ric_newtonadi.Z": ("after every Newton step " + _RECOMPRESSED, _always),
    "ric_newtonadi.gain": ("the gain of a recompressed factor: " + _RECOMPRESSED, _always),
    "ric_newtonadi.info": ("the second step starts from the recompressed first iterate: " + _RECOMPRESSED, _always),
    "ric_newtonadi.trace": ("solves of the second step, which starts from the recompressed iterate: " + _RECOMPRESSED,
                            _always),
    "radi_default.Z": ("where the factor outgrows 512 columns " + _RECOMPRESSED, cb.radi_default_recompressed),
    "shift_solve.recycle.X16": ("the normal equations of the recycled initial guess are " + _ROWS, _rows129),
    "shift_solve.recycle.X5": ("the normal equations of the recycled initial guess are " + _ROWS, _rows129),
    "shift_solve.recycle.its": ("an iteration more or less from another guess, whose normal equations are " + _ROWS,
                                _rows129),
    "shift_solve.recycle.relres": ("the residual of an iterate that started from the recycled guess, whose normal "
                                   "equations are " + _ROWS, _rows129),
    "lyap_adi.sweep.Z": ("the sweep-form ADI starts its solves from recycled guesses (depth 5), whose normal equations "
                         "are " + _ROWS, _rows129),
    "lyap_adi.sweep.info": ("iteration counts and norms of such an ADI: the guess's normal equations are " + _ROWS,
                            _rows129),
    "lyap_adi.sweep.res_hist": ("residuals of such an ADI's iterates: the guess's normal equations are " + _ROWS,
                                _rows129),
    "shift_solve.recycle.trace": ("restart cycles follow the iteration counts of solves that start from the recycled "
                                  "guess, whose normal equations are " + _ROWS, _rows129),
    "lyap_adi.sweep.trace": ("restart cycles follow the iteration counts of such an ADI: the guess's normal equations "
                             "are " + _ROWS, _rows129),
    "resident.gain": ("Z^T B of the gain is " + _ROWS, _rows129),
}
# A context whose operator was NOT replaced keeps its ring of recycled right-hand sides (so does ricadi_clear_cache,
# which keeps the ring's slots): the recycled solves start from other guesses than a fresh context's -- more stored
# panels, other slots -- and cannot have its bits.  The refusal tests allow exactly these outputs to differ, at their
# dense bounds; the sequences do not.
RING_KEPT = ("shift_solve.recycle.X16", "shift_solve.recycle.X5", "shift_solve.recycle.its",
             "shift_solve.recycle.relres", "shift_solve.recycle.trace", "lyap_adi.sweep.Z", "lyap_adi.sweep.info",
             "lyap_adi.sweep.res_hist", "lyap_adi.sweep.trace")


def _say(*a):
    print("[context reuse]", *a)


# ------------------------------------------------------------------------------------------------ fresh side
_FRESH = {}


def _okey(opts):
    return tuple(sorted(opts.items()))


def _dims_battery(ctx, nv, cols):
    """``compress`` of a seeded random nv x cols factor on a dimension-only context."""
    Z = np.random.default_rng([5, nv, cols]).standard_normal((nv, cols))
    Zc, sv = ctx.compress(Z)
    return {"compress.Zc": Zc, "compress.sv": sv}


def _sections(key):
    """The steps a position is run in: the battery's sections, or the one ``compress`` of a dimension-only position."""
    return ("dims",) if isinstance(key, tuple) else cb.SECTIONS


def _run_section(ctx, key, sec):
    if isinstance(key, tuple):
        return _dims_battery(ctx, key[1], key[2])
    return cb.run(ctx, cb.get_op(key), seed=0, sections=(sec,))


def _set_position(ctx, key):
    if isinstance(key, tuple):
        ctx.set_dims(key[1])
    else:
        ctx.set_operator(*cb.get_op(key).ops)


class Fresh:
    """ONE new context with these options at this position, run section by section on demand (in order) and closed
    after the last one; its outputs are computed once per (options, position) of the module, shared, never modified."""

    def __init__(self, opts, key):
        self.opts, self.key, self.ctx, self.out = opts, key, None, {}

    def section(self, sec):
        for s in _sections(self.key):
            if s not in self.out:
                if self.ctx is None:
                    self.ctx = _lib.Context(0, **self.opts)
                    _set_position(self.ctx, self.key)
                self.out[s] = _run_section(self.ctx, self.key, s)
            if s == sec:
                break
        if len(self.out) == len(_sections(self.key)):
            self.close()
        return self.out[sec]

    def whole(self):
        out = {}
        for s in _sections(self.key):
            out.update(self.section(s))
        return out

    def close(self):
        if self.ctx is not None:
            self.ctx.close()
            self.ctx = None


def fresh(opts, key):
    k = (_okey(opts), key)
    if k not in _FRESH:
        _FRESH[k] = Fresh(opts, key)
    return _FRESH[k]


@pytest.fixture(scope="module", autouse=True)
def _close_fresh_contexts():
    yield
    for f in _FRESH.values():
        f.close()


def allowed(k, op, out, also=()):
    """Whether output ``k`` may differ in its bits from a fresh context's here: named in the control table and its
    cause applies to this operator and this run, or named in ``also`` (the refusal tests' ring)."""
    return k in also or (k in CONTROL_TABLE and CONTROL_TABLE[k][1](op, out))


def compare(label, key, veteran, reference, reporters=None, also=()):
    """The comparison rule of the module docstring; prints the measurement, then asserts.  ``reporters``: what the
    ``rep0.*`` outputs are compared with instead (see ``_after_refusal``); ``also``: further outputs that may differ
    at their dense bounds."""
    if reporters is not None:
        reference = dict(reference, **reporters)
    diff = cb.differing(veteran, reference)
    worst, miss, outside = 0.0, [], list(diff)
    if not isinstance(key, tuple):
        op = cb.get_op(key)
        inp = cb.inputs(op, 0)
        outside = [k for k in diff if not allowed(k, op, veteran, also)]
        for k in diff:
            if k not in outside:
                try:
                    worst = max(worst, cb.BOUNDS[k](op, veteran, inp))
                except AssertionError as e:
                    miss.append("%s: %s" % (k, e))
    _say("%s | %s | bitwise %d of %d | not bitwise: %s | worst reference-bound ratio %.3e" % (
        label, key, len(veteran) - len(diff), len(veteran), diff or "-", worst))
    assert not outside, ("not bitwise equal to a fresh context, and not allowed to differ here", label, key, outside)
    assert not miss, (label, key, miss)


# ------------------------------------------------------------------------------------------------ control
@pytest.mark.parametrize("key", ["nv33_np1", "lumped", ("dims", 50, 24), ("dims", 33, 24)], ids=str)
def test_control(key):
    """Two fresh contexts, the same battery: what differs must be named in the control table (and the four families
    spmm, precond_apply, plain shift_solve and ric_radi must not be: they have to be bitwise)."""
    a, b = fresh({}, key).whole(), Fresh({}, key).whole()
    diff = cb.differing(a, b)
    _say("control | %s | bitwise %d of %d | not bitwise: %s" % (key, len(a) - len(diff), len(a), diff or "-"))
    assert not [k for k in CONTROL_TABLE if k.startswith(cb.BITWISE_FAMILIES)]
    if isinstance(key, tuple):
        assert not diff, diff
        return
    op, inp = cb.get_op(key), cb.inputs(cb.get_op(key), 0)
    assert not [k for k in diff if not allowed(k, op, a)], diff
    # both contexts' outputs meet the reference bounds of everything the table names (its entries are checkable,
    # whether or not this run happened to differ in them)
    for k in CONTROL_TABLE:
        cb.BOUNDS[k](op, a, inp)
        cb.BOUNDS[k](op, b, inp)


# ------------------------------------------------------------------------------------------------ sequences
def _facts(ctx, key, opts):
    if isinstance(key, tuple):
        return dict(dims=True, nv=ctx.nv, np=ctx.np_)
    op = cb.get_op(key)
    si, st = ctx.setup_info(), ctx.precond_structure(0)
    t = _lib.host_saddle_tiles(*op.ops, **opts)
    return dict(dims=False, nv=si["nv"], np=si["np"], levels=si["levels"], kc=si["kc"], bs=si["bs"],
                folded=st["folded"], rect=st["rect"], smoothed=st["smoothed"], child=st["child"],
                sb_ok=t["sb_ok"], ms_ok=t["ms_ok"], child_smoother=si["child_smoother"],
                vanka_patches=si["vanka_patches"])


class Veteran:
    """One context for a whole sequence; ``advance(step)`` sets the operator of every position and runs every section
    up to ``step`` in order (a test selected alone still sees the veteran its step is about)."""

    def __init__(self, name):
        self.name = name
        self.opts, self.keys = cb.SEQUENCES[name]
        self.steps = [(pos, sec) for pos, key in enumerate(self.keys) for sec in _sections(key)]
        self.ctx = _lib.Context(0, **self.opts)
        self.done, self.failed, self.facts, self.outs = 0, None, [], []

    def advance(self, step):
        while self.done <= step:
            pos, sec = self.steps[self.done]
            key = self.keys[pos]
            try:
                if sec == _sections(key)[0]:
                    _set_position(self.ctx, key)
                    self.facts.append(_facts(self.ctx, key, self.opts))
                self.outs.append(_run_section(self.ctx, key, sec))
            except BaseException as e:
                self.failed = "position %d (%s), section %s raised %r" % (pos, key, sec, e)
                raise
            self.done += 1
        return self.outs[step]


@pytest.fixture(scope="module")
def veterans():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Veteran(name)
        return made[name]

    yield get
    for v in made.values():
        v.ctx.close()


def _flips_grow(f):
    """nv grows strictly, np goes 0 -> > 0, the multi-shift tile format goes on -> off (arrow200's long row), the coarse
    space goes away (arrow200: none); the ADI's W has three columns on every operator: the ring and the side-by-side
    panel of the recycled right-hand sides are rebuilt at the same width for more rows."""
    nv = [x["nv"] for x in f]
    assert nv == sorted(set(nv)) and f[0]["np"] == 0 and all(x["np"] > 0 for x in f[1:])
    assert {x["ms_ok"] for x in f} == {True, False} and {x["kc"] > 0 for x in f} == {True, False}


def _flips_shrink(f):
    """nv shrinks strictly down to one row, np goes > 0 -> 0, multi-shift tiles off -> on, no coarse space -> one:
    buffers, workspaces and block lists sized for a larger operator serve a smaller one."""
    nv = [x["nv"] for x in f]
    assert nv == sorted(set(nv), reverse=True) and nv[-1] == 1 and f[-1]["np"] == 0 and all(x["np"] > 0 for x in f[:-1])
    assert {x["ms_ok"] for x in f} == {True, False} and {x["kc"] > 0 for x in f} == {True, False}


def _flips_pressure(f):
    """Pressure rows on -> off -> on: the folded cycle and its operands (``tp``, ``ps_meta``, the rectangular last
    sweep behind ``gt_ok``) are used, left unused with their device arrays in place, and used again."""
    assert [x["np"] > 0 for x in f] == [True, False, True]
    assert [x["folded"] for x in f] == [True, False, True], [x["folded"] for x in f]


def _flips_values(f):
    """The same sizes and patterns with other values: the per-shift cache is keyed by (alpha, beta) alone, so an
    inverse that survived the replacement would be applied to the wrong matrix.  Plain -> smoothed aggregation on the
    way (stiff_grid)."""
    assert len({(x["nv"], x["np"]) for x in f[:3]}) == 1 and len({(x["nv"], x["np"]) for x in f[3:]}) == 1
    assert [x["smoothed"] for x in f] == [False, False, False, True, True]


def _flips_hierarchy(f):
    """A child level comes, goes and comes back (setup_info levels 3 -> 2 -> 3)."""
    assert [x["levels"] for x in f] == [3, 2, 3] and [x["child"] for x in f] == [True, False, True]


def _flips_hierarchy_vanka(f):
    """The same with the coloured Vanka sweep on the child level: its patch records come, go and come back."""
    _flips_hierarchy(f)
    assert [x["child_smoother"] for x in f] == [1, 0, 1]           # (setup_info reports the smoother in use)
    assert [x["vanka_patches"] > 0 for x in f] == [True, False, True], [x["vanka_patches"] for x in f]


def _flips_dims(f):
    """Operator -> dimensions only -> operator -> dimensions only (of the operator's own nv: ``context_dims`` would
    not even call set_dims, the test does) -> a larger operator."""
    assert [x["dims"] for x in f] == [False, True, False, True, False]
    assert [x["nv"] for x in f] == [33, 50, 33, 33, 65]


def _flips_block(bs):
    def check(f):
        nv = [x["nv"] for x in f]
        assert all(x["bs"] == bs for x in f) and nv[0] < nv[1] > nv[2]
        assert {x["kc"] > 0 for x in f} == {True, False}
    check.__doc__ = """Block size %d: small -> large -> small, with and without a coarse space.""" % bs
    return check


FLIPS = {"grow": _flips_grow, "shrink": _flips_shrink, "pressure": _flips_pressure, "values": _flips_values,
         "hierarchy": _flips_hierarchy, "hierarchy_vanka": _flips_hierarchy_vanka, "dims": _flips_dims,
         "block16": _flips_block(16), "block64": _flips_block(64)}
def _steps(name):
    return [(pos, sec) for pos, key in enumerate(cb.SEQUENCES[name][1]) for sec in _sections(key)]


STEPS = [(name, i) for name in cb.SEQUENCES for i in range(len(_steps(name)))]


def _step_id(name, i):
    pos, sec = _steps(name)[i]
    key = cb.SEQUENCES[name][1][pos]
    return "%s-%d-%s-%s" % (name, pos, key if isinstance(key, str) else "set_dims%d" % key[1], sec)


@pytest.mark.parametrize("name,step", STEPS, ids=[_step_id(n, i) for n, i in STEPS])
def test_sequence(veterans, name, step):
    """One section of the battery (``context_battery.SECTIONS``; a dimension-only position has one step, its
    ``compress``) at one position of a sequence (``context_battery.SEQUENCES``; what each is after: the docstrings of
    the ``_flips_*`` functions above, asserted from setup_info / precond_structure / host_saddle_tiles at the last
    step): the veteran's outputs against a fresh context's."""
    v = veterans(name)
    if v.failed:
        pytest.skip("an earlier step of this sequence raised: " + v.failed)
    t0 = time.time()
    pos, sec = v.steps[step]
    key = v.keys[pos]
    out = v.advance(step)
    if isinstance(key, tuple):
        # a dimension-only context has no operator: what needs one refuses
        with pytest.raises(RuntimeError, match="set the operator first"):
            v.ctx.set_lowrank(None, None)
    compare("%s %d %s" % (name, pos, sec), key, out, fresh(v.opts, key).section(sec))
    if step == len(v.steps) - 1:
        _say("%s | facts %s" % (name, v.facts))
        FLIPS[name](v.facts)
    _say("%s | position %d %s | %.2f s" % (name, pos, sec, time.time() - t0))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.fixture(scope="module")
def refused():
    """(operator, a veteran that has run the battery once on nv33_np1)."""
    op = so.get("nv33_np1")
    ctx = _lib.Context(0)
    ctx.set_operator(*op.ops)
    cb.run(ctx, op, seed=0)
    yield op, ctx
    ctx.close()


def _after_refusal(label, op, ctx, reporters):
    """The battery after a refused call against a fresh context's.

    Two deliberate deviations from "equal to a fresh context", both for a context whose operator was NOT replaced
    (``reporters`` given):

    * the reporters before any solve (``rep0.*``) are compared with what they said right before the refused call, not
      with a fresh context's: a refused call must not change what the last successful one left, and a fresh context has
      no last call;
    * the ring of recycled right-hand sides is not forgotten either, so the outputs of ``RING_KEPT`` start from other
      guesses than a fresh context's and are held to their dense bounds instead of its bits.  ``ricadi_clear_cache``
      behaves the same way: it keeps the ring's slots, which then refill in another order than a growing ring
      (include/ricadi.h at ``ricadi_clear_cache``).

    After a refusal that ends in a replacement (``reporters`` None) neither applies: everything as a fresh context."""
    compare("refusal: " + label, op.name, cb.run(ctx, op, seed=0), fresh({}, op.name).whole(), reporters=reporters,
            also=RING_KEPT if reporters is not None else ())


def test_refused_positive_shift(refused):
    op, ctx = refused
    rep = cb.reporters(ctx, op)
    with pytest.raises(ValueError):
        ctx.lyap_adi([1.0], op.W, _lib.adi_params(dict(TIGHT)))
    _after_refusal("lyap_adi with a positive shift", op, ctx, rep)


def test_refused_wrong_row_count(refused):
    op, ctx = refused
    rep = cb.reporters(ctx, op)
    with pytest.raises(ValueError):
        ctx.spmm(-1.0, 1.0, np.ones((op.n + 1, 4)))
    _after_refusal("spmm with a wrong row count", op, ctx, rep)


def test_refused_generated_shifts_at_width_4(refused):
    op, ctx = refused
    rep = cb.reporters(ctx, op)
    ctx.set_radi_sweep_width(4)
    ctx.set_radi_shifts("hamiltonian")
    try:
        t0 = ctx.solve_trace()["solves"]
        with pytest.raises(ValueError):
            ctx.ric_radi(op.shifts, op.B, op.W, max_steps=6)
        assert ctx.solve_trace()["solves"] == t0
    finally:
        ctx.set_radi_shifts("cycle")
        ctx.set_radi_sweep_width(1)
    _after_refusal("ric_radi with generated shifts at width 4", op, ctx, rep)


def test_refused_operator_leaves_the_old_one_intact(refused):
    """``set_operator`` with a column index of J out of range is refused during validation: the old operator, its
    cache and its factor answer as before, bitwise."""
    op, ctx = refused
    rep = cb.reporters(ctx, op)
    R = np.random.default_rng(41).standard_normal((op.nv, 5))
    X = np.random.default_rng(42).standard_normal((op.n, 5))

    def answers():
        return (ctx.spmm(-30.0, 0.5, X), ctx.precond_apply(-30.0, 0.5, X), ctx.shift_solve(-30.0, 1.0, R)[0],
                ctx.factor_get(), ctx.cache_entries(), ctx.adi_stopped_by(), ctx.radi_shift_history())

    before = answers()
    a, e, j = (_lib.as_csr(m) for m in op.ops)
    jci = j[1].copy()
    jci[-1] = op.nv                                       # one past the last velocity column
    rc = ctx._lib.ricadi_set_operator(ctx._h, op.nv, op.np, _lib._i(a[0]), _lib._i(a[1]), _lib._d(a[2]), _lib._i(e[0]),
                                      _lib._i(e[1]), _lib._d(e[2]), _lib._i(j[0]), _lib._i(jci), _lib._d(j[2]))
    assert rc != 0 and "J: column index out of range" in ctx._lib.ricadi_last_error().decode()
    assert all(cb.same(x, y) for x, y in zip(before, answers())), "the refused replacement changed the old operator"
    _after_refusal("set_operator with a column of J out of range", op, ctx, rep)


def test_refused_setup_then_a_good_operator(refused):
    """An operator whose setup is refused -- one velocity row of calA and calE zeroed: "singular block-Jacobi block"
    when the first shift is set up (a flag word and an exception), unless the host setup refuses it first -- and then
    the good operator again."""
    op, ctx = refused
    D = sps.diags(np.where(np.arange(op.nv) == 7, 0.0, 1.0))
    bad = ((D @ op.calA).tocsr(), (D @ op.calE).tocsr(), op.J)
    with pytest.raises((RuntimeError, ValueError)) as ei:
        ctx.set_operator(*bad)
        ctx.shift_solve(-1.0, 1.0, np.ones((op.nv, 2)))
    _say("refused setup | %r" % (ei.value,))
    ctx.set_operator(*op.ops)
    _after_refusal("a solve on an operator with a singular block", op, ctx, None)      # (replaced: as a fresh one)


# ------------------------------------------------------------------------------------------------ the product's door
def test_the_products_door():
    """``pru.solve_proj_lyap_stein`` on fe2, fe3, fe2, fe3 through ``backend.context_for`` (one process-wide context,
    the operator replaced before every call) against the same four calls with ``backend.reset()`` before each, by the
    comparison rule: nothing of a step-form ADI is in the control table, so the factor and every number of the call's
    info must be bitwise; ``Z Z^T`` is also held to ``LYAP_TOL`` against the dense solution."""
    import sadptprj_riclyap_adi.proj_ric_utils as pru
    from optconpy_amd import backend

    def call(op):
        d = dict(TIGHT, ms=op.shifts)
        return pru.solve_proj_lyap_stein(amat=sps.csr_matrix(op.calA.T), mmat=sps.csr_matrix(op.calE.T), jmat=op.J,
                                         wmat=op.W, adi_dict=d)

    ops = [so.get(k) for k in ("fe2", "fe3", "fe2", "fe3")]
    backend.reset()
    try:
        vet = [call(op) for op in ops]
        ref = []
        for op in ops:
            backend.reset()
            ref.append(call(op))
    finally:
        backend.reset()
    for i, (op, v, r) in enumerate(zip(ops, vet, ref)):
        Z = np.asarray(v["zfac"])
        bitwise = cb.same(Z, np.asarray(r["zfac"])) and all(cb.same(v[k], r[k]) for k in v if k != "zfac")
        err = so.rel(Z @ Z.T, op.lyap())
        _say("door | call %d (%s) | bitwise %s | Z Z^T vs dense %.3e (bound %.0e) | %d steps, stopped by %s" % (
            i, op.name, bitwise, err, LYAP_TOL, v["adi_steps"], v["adi_stopped_by"]))
        assert sorted(v) == sorted(r)
        assert bitwise, (i, op.name, [k for k in v if k != "zfac" and not cb.same(v[k], r[k])])
        assert v["gmres_nonconverged"] == 0 and v["adi_stopped_by"] == r["adi_stopped_by"]
        assert err <= LYAP_TOL, (i, op.name, err)
