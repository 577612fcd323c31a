"""One fixed battery of calls on a context, for the tests of a context that changes operators
(tests/test_gpu_context_reuse.py, tests/test_context_reuse_cpu.py).

``run(ctx, op, seed)`` takes a context that has ``op`` (a :class:`small_ops.SmallOp`, or a :class:`CustomOp`) set and
returns a flat dict of named outputs -- NumPy arrays, integers and strings -- in the order of ``names()``.  Every input
is generated from ``seed`` and the operator's sizes; the shifts are ``small_ops.SHIFTS`` and ``op.shifts``.  No entry is
skipped for any operator of the family: tests/test_gpu_small_ops.py runs every one of these calls on every operator,
np = 0 and nv = 1 included, and the battery follows it.

Order: the reporters before any solve; ``spmm`` and ``precond_apply``; ``shift_solve`` plain, recycled and with a
low-rank term; ``lyap_adi`` in step and sweep form and two Newton steps of ``ric_newtonadi``; ``ric_radi`` in four
settings; ``gain``, ``lyap_res_norm`` and ``factor_get`` of the resident factor; one more ``ric_radi`` at the default
recompression.  After each driver: its info dict, its
histories and the delta of the cumulative ``solve_trace`` counters across the call.  The battery has five sections
(``SECTIONS``: direct calls, the two ADIs, Newton, RADI with the resident factor, the default RADI);
``run(..., sections=...)`` runs some
of them, so that a test can take one section at a time and stay short.

Left out: the ``RICADI_SMW=0`` form of the low-rank solve.  The switch is read when a context is created
(``read_switches``), so it cannot be reached on a live context.

``BOUNDS`` holds, per output that need not be bitwise repeatable, the check against the dense FP64 reference that
tests/test_gpu_small_ops.py applies to a fresh context (its comparators and bars, imported).
"""
import numpy as np

import small_ops as so
from optconpy_amd import _lib

# the bars of tests/test_gpu_small_ops.py, where they are stated (imported, not copied)
from test_gpu_small_ops import K_TOL, LYAP_TOL, TIGHT

PAIRS = ((-1.0, 1.0), (-30.0, 0.5))           # (alpha, beta) of the products and the cycle
# cumulative slots of Context.solve_trace (the other slots describe the most recent event or a maximum over the
# context's life, which a veteran context legitimately carries over)
TRACE_CUMULATIVE = ("solves", "guess_tried", "guess_used", "stored", "smw_solves", "smw_setups", "smw_dup", "smw_bad",
                    "smw_refined", "inop_lowrank", "esc1_groups", "esc2_groups", "wide_passes", "wide_chunks", "cycles",
                    "stalled_groups", "maxit_groups")
RADI_FORMS = ("cycle", "hamiltonian", "sweep4", "sweep_shifts")
BITWISE_FAMILIES = ("spmm.", "precond_apply.", "shift_solve.plain.", "ric_radi.")


class CustomOp(so.SmallOp):
    """A :class:`small_ops.SmallOp` of matrices that are not in ``small_ops.FAMILY`` (a transpose, a scaled copy, a
    finite-element operator of another size), with the same references."""

    def __init__(self, name, calA, calE, J, opts=None):
        self.name, self.opts = name, dict(opts or {})
        self.calA, self.calE, self.J = (m.tocsr() for m in (calA, calE, J))
        for m in (self.calA, self.calE, self.J):
            m.sum_duplicates()
            m.sort_indices()
        self.nv, self.np = self.calA.shape[0], self.J.shape[0]
        self.n = self.nv + self.np
        self.Ad, self.Ed, self.Jd = self.calA.toarray(), self.calE.toarray(), self.J.toarray()
        self._c = {}


def newton2_reference(op):
    """The iterate two Newton-Kleinman steps from X = 0 give for the projected Riccati equation of ``identities.
    dense_projected_are`` when each step's Lyapunov equation is solved by the ADI the call runs: X1 is the Lyapunov
    solution ``op.lyap()`` (the first ADI stops on its tolerance of 1e-12 on every operator); with
    ``K = calE X1 B``, X2 is the dense ADI iterate after ``TIGHT['adi_max_steps']`` steps, ``op.shifts`` cycled, for
    ``(calA - K B^T) X calE^T + calE X (calA - K B^T)^T + [W, K] [W, K]^T = 0`` on ker J -- in the standard form
    ``a X + X a^T + w w^T = 0`` of the projected pencil: ``V_1 = sqrt(-2 p_1) (a + p_1)^-1 w``,
    ``V_j = sqrt(p_j / p_{j-1}) (I - (p_j + p_{j-1}) (a + p_j)^-1) V_{j-1}``, ``X = sum V_j V_j^T`` (dense LU solves,
    FP64).  Where the second ADI converges this is the Bartels-Stewart solution to 1e-11; where it does not -- the
    finite-element operators, with these eight shifts -- it is the truncated iterate the call actually computes (the
    CPU oracle's two-step iterate agrees with it to 4e-12 on fe2, fe3, fe6, nv33_np1 and nv65_np24)."""
    def f():
        K = op.Ed @ op.lyap() @ op.B
        Th = op.theta
        Eh = Th.T @ op.Ed @ Th
        a = np.linalg.solve(Eh, Th.T @ (op.Ad - K @ op.B.T) @ Th)
        w = np.linalg.solve(Eh, Th.T @ np.hstack([op.W, K]))
        eye, X, V = np.eye(a.shape[0]), np.zeros_like(a), None
        ps = [float(p) for p in op.shifts]
        for j in range(TIGHT["adi_max_steps"]):
            p, q = ps[j % len(ps)], ps[(j - 1) % len(ps)]
            if V is None:
                V = np.sqrt(-2.0 * p) * np.linalg.solve(a + p * eye, w)
            else:
                V = np.sqrt(p / q) * (V - (p + q) * np.linalg.solve(a + p * eye, V))
            X += V @ V.T
        return Th @ (0.5 * (X + X.T)) @ Th.T
    return op._memo("newton2", f)


# ------------------------------------------------------------------------------------------------ operators, sequences
_CUSTOM = {}


def get_op(key):
    """An operator of ``small_ops.FAMILY`` by name, or one of the derived ones: ``unsym_T`` (``unsym`` with calA and
    calE transposed, the same J: the pair of operators ``lqgbt_reduce`` alternates between), ``stiff_grid_x3``
    (``stiff_grid`` with calA scaled by 3: same pattern, same shifts' cache keys, other values) and ``fe6``
    (``ricc_problem(6, 0.05)``: the smallest of the family that gets a child level, at ``coarse_max=16``)."""
    if key in so.FAMILY:
        return so.get(key)
    if key not in _CUSTOM:
        if key == "unsym_T":
            b = so.get("unsym")
            _CUSTOM[key] = CustomOp(key, b.calA.T, b.calE.T, b.J)
        elif key == "stiff_grid_x3":
            b = so.get("stiff_grid")
            _CUSTOM[key] = CustomOp(key, 3.0 * b.calA, b.calE, b.J)
        elif key == "fe6":
            _CUSTOM[key] = CustomOp(key, *so.finite_element(6))
        else:
            raise KeyError(key)
    return _CUSTOM[key]


HIERARCHY = dict(hierarchy=1, coarse_max=16)    # fe6: 242 + 48 -> a child level of 18 + 2; fe3: a dense coarse problem
# name -> (context options, positions); a position is an operator's key or ("dims", nv, columns of the factor)
SEQUENCES = {
    "grow": ({}, ["nv15_np0", "nv33_np1", "nv65_np24", "arrow200"]),
    "shrink": ({}, ["arrow200", "nv65_np24", "nv17_np16", "nv2_np1", "nv1"]),
    "pressure": ({}, ["lumped", "nv63_np0", "lumped"]),
    "values": ({}, ["unsym", "unsym_T", "unsym", "stiff_grid", "stiff_grid_x3"]),
    "hierarchy": (dict(HIERARCHY), ["fe6", "fe3", "fe6"]),
    "hierarchy_vanka": (dict(HIERARCHY, child_smoother=1), ["fe6", "fe3", "fe6"]),
    "dims": ({}, ["nv33_np1", ("dims", 50, 24), "nv33_np1", ("dims", 33, 24), "nv65_np24"]),
    "block16": (dict(bj_block=16), ["nv15_np14_b16", "nv17_np1_b16", "nv16_np7_b16"]),
    "block64": (dict(bj_block=64), ["nv63_np62_b64", "nv65_np20_b64", "nv63_np62_b64"]),
}


def host_facts(key, opts):
    """What the host entries say about a position (no device): sizes, the tile format's flags, the hierarchy."""
    if isinstance(key, tuple):
        return dict(dims=True, nv=key[1], np=0)
    op = get_op(key)
    t = _lib.host_saddle_tiles(*op.ops, **opts)
    plan = _lib.host_plan_levels(*op.ops, **opts)
    hier = _lib.host_plan_hierarchy(*op.ops, **opts)
    return dict(dims=False, nv=op.nv, np=op.np, sb_ok=t["sb_ok"], ms_ok=t["ms_ok"], smoothed=plan["smoothed"],
                kc=plan["kc"], levels=len(hier) + 1 if plan["kc"] > 0 else 1,
                nbv=len(op.host_structure()["bv_ptr"]) - 1)


# ------------------------------------------------------------------------------------------------ inputs
def inputs(op, seed):
    """Every random input of the battery (a dict of arrays), from ``seed`` and the operator's sizes."""
    rng = np.random.default_rng([seed, op.nv, op.np])
    d = {}
    for m in (5, 16):
        d["X%d" % m] = rng.standard_normal((op.n, m))
        d["R%d" % m] = rng.standard_normal((op.nv, m))
    d["rec"] = [rng.standard_normal((op.nv, 16)) for _ in range(3)] + [rng.standard_normal((op.nv, 5))]
    d["U"], d["V"] = 0.1 * rng.standard_normal((op.nv, 3)), rng.standard_normal((op.nv, 3))
    return d


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


def _trace(ctx):
    t = ctx.solve_trace()
    return np.array([t[k] for k in TRACE_CUMULATIVE], dtype=np.int64)


def _info(info):
    """(numbers of an info dict in key order, its strings in key order)."""
    keys = sorted(info)
    num = np.array([float(info[k]) for k in keys if not isinstance(info[k], str)])
    txt = "|".join("%s=%s" % (k, info[k]) for k in keys if isinstance(info[k], str))
    return num, txt


def _reporter(fn):
    """The value of a reporter; an exception is recorded as its type and message."""
    try:
        v = fn()
    except Exception as e:                                   # noqa: BLE001 - recorded, compared between contexts
        return "%s: %s" % (type(e).__name__, e)
    if isinstance(v, dict):
        return "|".join("%s=%s" % (k, v[k]) for k in sorted(v))
    return v


SECTIONS = ("direct", "adi", "newton", "radi", "radi_default")     # the battery's sections, in order


def names(sections=SECTIONS):
    """The names of the battery's outputs, in order (no device needed)."""
    out = []
    if "direct" in sections:
        out += ["rep0.setup_info", "rep0.cache_entries", "rep0.adi_res_history", "rep0.adi_stopped_by",
                "rep0.newton_history", "rep0.newton_stopped_by", "rep0.radi_shift_history", "rep0.radi_sweep_info", "rep0.radi_sweep_widths", "rep0.recycle_guess_rank"]
        for m in (5, 16):
            out += ["spmm.m%d" % m, "precond_apply.m%d" % m]
        for m in (16, 5):
            out += ["shift_solve.plain.m%d.%s" % (m, k) for k in ("X", "its", "relres")]
        out += ["shift_solve.recycle.%s" % k for k in ("X16", "X5", "its", "relres", "trace")]
        out += ["shift_solve.lowrank.%s" % k for k in ("X", "its", "relres", "trace")]
    if "adi" in sections:
        for form in ("step", "sweep"):
            out += ["lyap_adi.%s.%s" % (form, k) for k in ("Z", "info", "stopped_by", "res_hist", "trace")]
    if "newton" in sections:
        out += ["ric_newtonadi.%s" % k for k in ("Z", "gain", "info", "stopped_by", "trace")]
    if "radi" in sections:
        for form in RADI_FORMS:
            out += ["ric_radi.%s.%s" % (form, k) for k in ("Z", "K", "info", "stop_rule", "shift_hist", "fallbacks",
                                                            "sweep_info", "sweep_widths", "trace")]
        out += ["resident.gain", "resident.lyap_res_norm", "resident.factor"]
    if "radi_default" in sections:
        out += ["radi_default.%s" % k for k in ("Z", "K", "info", "stop_rule", "trace")]
    return out


def reporters(ctx, op, inp=None):
    """What the reporters say right now (the ``rep0.*`` outputs): ``setup_info``, ``cache_entries``, the ADI's, the
    Newton driver's and RADI's "of the last call" entries, and the rank of the recycled guess for a 16-column panel at depth 0 (0
    expected).  An exception is recorded as its type and message."""
    inp = inputs(op, 0) if inp is None else inp
    G = len(so.SHIFTS)
    out = {}
    out["rep0.setup_info"] = _reporter(ctx.setup_info)
    out["rep0.cache_entries"] = _reporter(ctx.cache_entries)
    out["rep0.adi_res_history"] = _reporter(ctx.adi_res_history)
    out["rep0.adi_stopped_by"] = _reporter(ctx.adi_stopped_by)
    out["rep0.newton_history"] = _reporter(ctx.newton_history)
    out["rep0.newton_stopped_by"] = _reporter(ctx.newton_stopped_by)
    out["rep0.radi_shift_history"] = _reporter(ctx.radi_shift_history)
    out["rep0.radi_sweep_info"] = _reporter(ctx.radi_sweep_info)
    out["rep0.radi_sweep_widths"] = _reporter(ctx.radi_sweep_widths)
    Rd, Xd = _dev(inp["R16"]), _nan(G, op.n, 16)
    out["rep0.recycle_guess_rank"] = _reporter(
        lambda: ctx.recycle_guess_dev(so.SHIFTS, [1.0] * G, Rd.data_ptr(), 16, Xd.data_ptr()))
    return out


# ------------------------------------------------------------------------------------------------ the battery
def run(ctx, op, seed=0, sections=SECTIONS):
    """The battery, or the named sections of it (a test may run one section at a time: the calls a context sees are the
    same, in the same order, as long as the sections of an operator are run in order)."""
    assert (ctx.nv, ctx.np_) == (op.nv, op.np), "the context does not hold this operator"
    inp = inputs(op, seed)
    out = {}
    for sec in SECTIONS:
        if sec in sections:
            _SECTION[sec](ctx, op, inp, out)
    assert list(out) == names(sections), "names() and run() disagree"
    return out


def _direct(ctx, op, inp, out):
    G = len(so.SHIFTS)
    ones = [1.0] * G

    # -- the reporters before any solve
    out.update(reporters(ctx, op, inp))

    # -- products and the cycle
    for m in (5, 16):
        out["spmm.m%d" % m] = np.stack([ctx.spmm(a, b, inp["X%d" % m]) for a, b in PAIRS])
        out["precond_apply.m%d" % m] = np.stack([ctx.precond_apply(a, b, inp["X%d" % m]) for a, b in PAIRS])

    # -- shift solves: plain
    for m in (16, 5):
        res = [ctx.shift_solve(p, 1.0, inp["R%d" % m]) for p in so.SHIFTS]
        out["shift_solve.plain.m%d.X" % m] = np.stack([r[0] for r in res])
        out["shift_solve.plain.m%d.its" % m] = np.array([r[1] for r in res])
        out["shift_solve.plain.m%d.relres" % m] = np.stack([r[2] for r in res])

    # -- recycled: three shared right-hand sides of width 16 (the second and third start from a guess), then one of
    # width 5 (the width change invalidates the side-by-side panel)
    t0 = _trace(ctx)
    ctx.set_recycle(3)
    try:
        xs, its, rrs = [], [], []
        for R in inp["rec"]:
            m = R.shape[1]
            Rd, Xd = _dev(R), _nan(G, op.n, m)
            it, rr = ctx.shift_solve_batch_dev(so.SHIFTS, ones, Rd.data_ptr(), 0, m, Xd.data_ptr())
            ctx.synchronize()
            xs.append(_host(Xd))
            its.append(list(it))
            rrs.append(rr.ravel())
    finally:
        ctx.set_recycle(0)
    out["shift_solve.recycle.X16"] = np.stack(xs[:3])
    out["shift_solve.recycle.X5"] = xs[3]
    out["shift_solve.recycle.its"] = np.array(its)
    out["shift_solve.recycle.relres"] = np.concatenate(rrs)
    out["shift_solve.recycle.trace"] = _trace(ctx) - t0

    # -- with a low-rank term of width 3 (Woodbury)
    t0 = _trace(ctx)
    ctx.set_lowrank(inp["U"], inp["V"])
    try:
        res = [ctx.shift_solve(p, 1.0, inp["R5"]) for p in so.SHIFTS]
    finally:
        ctx.set_lowrank(None, None)
    out["shift_solve.lowrank.X"] = np.stack([r[0] for r in res])
    out["shift_solve.lowrank.its"] = np.array([r[1] for r in res])
    out["shift_solve.lowrank.relres"] = np.stack([r[2] for r in res])
    out["shift_solve.lowrank.trace"] = _trace(ctx) - t0


def _adi(ctx, op, inp, out):
    # -- Lyapunov ADI: step form (default recycling) and sweeps of four shifts, residual history on
    ctx.set_adi_res_history(True)
    try:
        for form, width in (("step", 1), ("sweep", 4)):
            t0 = _trace(ctx)
            Z, info = ctx.lyap_adi(op.shifts, op.W, _lib.adi_params(dict(TIGHT, sweep_width=width)))
            out["lyap_adi.%s.Z" % form] = np.array(Z)
            out["lyap_adi.%s.info" % form], out["lyap_adi.%s.stopped_by" % form] = _info(info)
            out["lyap_adi.%s.res_hist" % form] = ctx.adi_res_history()
            out["lyap_adi.%s.trace" % form] = _trace(ctx) - t0
    finally:
        ctx.set_adi_res_history(False)


def _newton(ctx, op, inp, out):
    # -- two Newton steps
    t0 = _trace(ctx)
    Z, info = ctx.ric_newtonadi(op.shifts, op.B, op.W, _lib.adi_params(dict(TIGHT, nwtn_max_steps=2)))
    out["ric_newtonadi.Z"] = np.array(Z)
    out["ric_newtonadi.gain"] = ctx.gain(op.B)
    out["ric_newtonadi.info"], out["ric_newtonadi.stopped_by"] = _info(info)
    out["ric_newtonadi.trace"] = _trace(ctx) - t0


def _radi(ctx, op, inp, out):
    # -- RADI: the cycled list, generated shifts, sweeps of four, sweeps with generated shifts; settings restored
    for form in RADI_FORMS:
        mode = {"cycle": "cycle", "hamiltonian": "hamiltonian", "sweep4": "cycle",
                "sweep_shifts": "hamiltonian-dominant"}[form]
        m0 = ctx.set_radi_shifts(mode)
        w0 = ctx.set_radi_sweep_width(4 if form in ("sweep4", "sweep_shifts") else 1)
        s0 = ctx.set_radi_sweep_shifts(form == "sweep_shifts")
        t0 = _trace(ctx)
        try:
            # (no recompression inside the call -- the default starts one every 512 columns, and a recompressed
            # factor's bits are those of gemm_tn_kernel's atomics: the family ric_radi has to be bitwise)
            Z, K, info = ctx.ric_radi(op.shifts, op.B, op.W, max_steps=200, res_reltol=1e-12,
                                      compress_cols=200 * so.MW + 1)
        finally:
            ctx.set_radi_sweep_shifts(s0)
            ctx.set_radi_sweep_width(w0)
            ctx.set_radi_shifts(m0)
        key = "ric_radi.%s." % form
        out[key + "Z"], out[key + "K"] = np.array(Z), K
        out[key + "info"], out[key + "stop_rule"] = _info(info)
        out[key + "shift_hist"] = ctx.radi_shift_history()
        out[key + "fallbacks"] = ctx.radi_shift_fallbacks()
        out[key + "sweep_info"] = _reporter(ctx.radi_sweep_info)
        out[key + "sweep_widths"] = ctx.radi_sweep_widths()
        out[key + "trace"] = _trace(ctx) - t0

    # -- the resident factor (of the last RADI call)
    Zr = ctx.factor_get()
    out["resident.gain"] = ctx.gain(op.B)
    out["resident.lyap_res_norm"] = float(ctx.lyap_res_norm(Zr, op.W))
    out["resident.factor"] = Zr


def _radi_default(ctx, op, inp, out):
    # -- the product's default RADI: a recompression every 512 columns (reached where the cycled list needs more than
    # 170 steps: the finite-element operators), on the pools and the auxiliary resources a replacement left
    t0 = _trace(ctx)
    Z, K, info = ctx.ric_radi(op.shifts, op.B, op.W, max_steps=400, res_reltol=1e-12)
    out["radi_default.Z"], out["radi_default.K"] = np.array(Z), K
    out["radi_default.info"], out["radi_default.stop_rule"] = _info(info)
    out["radi_default.trace"] = _trace(ctx) - t0


_SECTION = {"direct": _direct, "adi": _adi, "newton": _newton, "radi": _radi, "radi_default": _radi_default}


# ------------------------------------------------------------------------------------------------ comparison
def same(a, b):
    """Bitwise equality of two outputs (arrays: shape and every element, NaN equal to NaN)."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))
    return type(a) is type(b) and a == b


def differing(a, b):
    """Names of the outputs of two battery runs that are not bitwise equal."""
    assert list(a) == list(b)
    return [k for k in a if not same(a[k], b[k])]


def _solves_ok(op, X, Rs):
    """``small_ops.solve_ok`` for every shift of SHIFTS on panels X (right-hand side x shift x n x m)."""
    ratio = 0.0
    for k, R in enumerate(Rs):
        for g, p in enumerate(so.SHIFTS):
            res, _ = so.solve_ok(op, p, 1.0, X[k][g], R)
            ratio = max(ratio, res / so.RES_TOL)
    return ratio


def _bar(value, bound, what):
    assert np.isfinite(value) and value <= bound, (what, value, bound)
    return float(value / bound)


def _lyap(form):
    def check(op, out, inp):
        Z = out["lyap_adi.%s.Z" % form]
        return _bar(so.rel(Z @ Z.T, op.lyap()), LYAP_TOL, "lyap_adi %s Z Z^T vs dense" % form)
    return check


def _converged(prefix):
    """A driver's counters have no dense reference: what test_gpu_small_ops.py asks of them is that no solve missed
    its tolerance (its ``_no_ricadi_warning``): ``gmres_nonconverged == 0``."""
    def check(op, out, inp):
        num = out[prefix + ".info"]
        keys = _INFO_KEYS[prefix.split(".")[0]]
        assert num.shape == (len(keys),), (prefix, num)
        assert num[keys.index("gmres_nonconverged")] == 0, (prefix, "a shift solve missed its tolerance")
        return 0.0
    return check


_INFO_KEYS = {
    "lyap_adi": sorted(["adi_steps", "adi_rel_newZ", "gmres_iters", "shift_solves", "res_fro", "cols",
                        "gmres_nonconverged", "gmres_worst_relres", "storage_escalations"]),
    "ric_newtonadi": sorted(["nwtn_steps", "upd_abs", "upd_rel", "adi_steps", "gmres_iters", "shift_solves", "cols",
                             "gmres_nonconverged", "gmres_worst_relres", "lyap_res_fro", "lyap_rhs_fro",
                             "storage_escalations", "adi_sweeps"]),
}


def _newton_z(op, out, inp):
    Z = out["ric_newtonadi.Z"]
    assert np.all(np.isfinite(Z))
    return _bar(so.rel(Z @ Z.T, newton2_reference(op)), K_TOL, "ric_newtonadi (two steps) Z Z^T vs dense")


def _newton_gain(op, out, inp):
    assert np.all(np.isfinite(out["ric_newtonadi.gain"]))
    return _bar(so.rel(out["ric_newtonadi.gain"], op.Ed @ newton2_reference(op) @ op.B), K_TOL,
                "ric_newtonadi (two steps) gain vs dense")


def _resident_gain(op, out, inp):
    return _bar(so.rel(out["resident.gain"], op.Ed @ op.are() @ op.B), K_TOL, "gain of the resident factor vs dense")


def _radi_default_z(op, out, inp):
    Z = out["radi_default.Z"]
    return _bar(so.rel(Z @ Z.T, op.are()), K_TOL, "ric_radi (default recompression) Z Z^T vs dense")


def _radi_default_k(op, out, inp):
    return _bar(so.rel(out["radi_default.K"], op.Ed @ op.are() @ op.B), K_TOL,
                "ric_radi (default recompression) gain vs dense")


def radi_default_recompressed(op, out):
    """Whether the default RADI call of this battery run outgrew 512 columns (and so recompressed its factor)."""
    steps = int(out["radi_default.info"][sorted(_RADI_INFO_KEYS).index("radi_steps")])
    return steps * so.MW >= 512


_RADI_INFO_KEYS = ("radi_steps", "res_rel", "rhs_fro", "gmres_iters", "shift_solves", "cols", "gmres_nonconverged",
                   "gmres_worst_relres", "storage_escalations")


def _recycle_x16(op, out, inp):
    return _solves_ok(op, out["shift_solve.recycle.X16"], inp["rec"][:3])


def _recycle_x5(op, out, inp):
    return _solves_ok(op, [out["shift_solve.recycle.X5"]], inp["rec"][3:])


def _recycle_relres(op, out, inp):
    # the true relative residual the solve itself reports, at the bar every shift solve is held to
    return _bar(out["shift_solve.recycle.relres"].max(), so.RES_TOL, "reported residual of the recycled solves")


def _recycle_its(op, out, inp):
    its = out["shift_solve.recycle.its"]
    assert its.shape == (4, len(so.SHIFTS)) and its.min() >= 0, its      # (convergence: _recycle_x16 / _recycle_x5)
    return 0.0


def _res_hist(form):
    def check(op, out, inp):
        h = out["lyap_adi.%s.res_hist" % form]
        steps = int(out["lyap_adi.%s.info" % form][_INFO_KEYS["lyap_adi"].index("adi_steps")])
        assert h.shape == (steps,) and np.all(np.isfinite(h)) and np.all(h >= 0), (form, h.shape, steps)
        return 0.0
    return check


def _trace_nonneg(name):
    def check(op, out, inp):
        t = out[name]
        assert t.shape == (len(TRACE_CUMULATIVE),) and t.min() >= 0, (name, t)
        for k in ("stalled_groups", "maxit_groups"):
            assert t[TRACE_CUMULATIVE.index(k)] == 0, (name, k, "a solve missed its tolerance")
        return 0.0
    return check


# output -> its check against the dense FP64 reference (returns the measured value as a fraction of its bound).  Only
# outputs named in the control table of tests/test_gpu_context_reuse.py are ever checked through this.
BOUNDS = {
    "shift_solve.recycle.X16": _recycle_x16,
    "shift_solve.recycle.X5": _recycle_x5,
    "shift_solve.recycle.its": _recycle_its,
    "shift_solve.recycle.relres": _recycle_relres,
    "shift_solve.recycle.trace": _trace_nonneg("shift_solve.recycle.trace"),
    "lyap_adi.step.Z": _lyap("step"),
    "lyap_adi.step.info": _converged("lyap_adi.step"),
    "lyap_adi.step.res_hist": _res_hist("step"),
    "lyap_adi.step.trace": _trace_nonneg("lyap_adi.step.trace"),
    "lyap_adi.sweep.Z": _lyap("sweep"),
    "lyap_adi.sweep.info": _converged("lyap_adi.sweep"),
    "lyap_adi.sweep.res_hist": _res_hist("sweep"),
    "lyap_adi.sweep.trace": _trace_nonneg("lyap_adi.sweep.trace"),
    "ric_newtonadi.Z": _newton_z,
    "ric_newtonadi.gain": _newton_gain,
    "ric_newtonadi.info": _converged("ric_newtonadi"),
    "ric_newtonadi.trace": _trace_nonneg("ric_newtonadi.trace"),
    "resident.gain": _resident_gain,
    "radi_default.Z": _radi_default_z,
    "radi_default.K": _radi_default_k,
}
