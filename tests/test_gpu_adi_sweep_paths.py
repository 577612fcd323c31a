"""What the sweep-form ADI driver (``SweepAdi``, optconpy_amd/csrc/solver_adi.inl) does between its kernels and its
stopping policy, on the MI355X at a size where a failure can be traced: N = 8 (NV = 450, n = 530, m = 4), every run a
``ctx.lyap_adi`` of at most 64 steps held to the dense model (``tests/adi_res_model.py``) and to the schedule
``tests/adi_sweep_model.py`` predicts from it.

  1. windows that are not one of the cycle's: a sweep cut by ``AdiStop::cut`` after which the iteration goes on
     (cases A - D of adi_sweep_model.CASES; B wraps round the list and runs a full-width misaligned window, C drops a
     block on a misaligned window) and a window the pivot bound refuses, which runs narrowed (case E: an error before
     ``adi_window_width``);
  2. aligned sweeps that wrap round the list, the last one partial, no rule;
  3. the in-flight recompression (``AsyncRecompress``): one round after every sweep and after every second one, against
     the same run without, and together with a cut and a misaligned window;
  4. an odd panel width (m = 7) through the splice, the factor held within its rows;
  5. the Newton driver with a small ``compress_cols``.

The premises -- schedules, tolerances in the middle of their intervals, margins >= 1.1, the rank band of 3 -- are
asserted without a GPU in tests/test_adi_sweep_model_cpu.py.  Case A under the residual rule is not run: no tolerance
gives it a misaligned window of two or more shifts (see there)."""
import numpy as np
import pytest

from optconpy_amd import _lib, backend, problems as pb
from oracle import lin_alg_utils as olau, proj_ric_utils as opru

from adi_res_model import AdiResModel
import adi_sweep_model as sw
from test_gpu_adi_res import HIST_BOUND

pytestmark = pytest.mark.gpu
K_TOL = 1e-6          # the bar of tests/test_gpu_configs.py::test_hip_newton_adi_vs_dense_are_three_call_forms
ZZT_TOL = 1e-7        # the sweep form against the oracle (tests/test_gpu_parity.py, sweep_width = 4)
M = 4


class Shared:
    """Problem, model and the step-form references (computed once per list, read only); one context for the runs
    that need no fresh one."""

    def __init__(self):
        self.pr, self.F, self.W = sw.problem_n8()
        pr = self.pr
        assert (pr.NV, pr.NV + pr.J.shape[0], self.W.shape[1]) == (450, 530, M)
        self.mdl = AdiResModel(self.F.T, pr.M.T, pr.J)
        self.W0 = self.mdl.project(self.W)
        self._ref = {}
        self.ctx = self.fresh()

    def fresh(self):
        ctx = _lib.Context(0)
        ctx.set_operator(self.F.T.tocsr(), self.pr.M.T.tocsr(), self.pr.J)
        return ctx

    def ref(self, lst):
        if lst not in self._ref:
            ms = pb.logshifts(*lst)
            r = self.mdl.step_form(self.W0, ms, sw.STEPS)
            r["Z"] = np.hstack(r["Z"])
            self._ref[lst] = (ms, r)
        return self._ref[lst]


@pytest.fixture(scope="module")
def S():
    s = Shared()
    yield s
    s.ctx.close()
    backend.reset()


def zzt_dev(Z, ref, steps):
    """||Z Z^T - Z_m Z_m^T||_F / ||Z_m^T Z_m||_F against the model's first `steps` blocks."""
    Zm = ref["Z"][:, :steps * M]
    return np.linalg.norm(Z @ Z.T - Zm @ Zm.T) / np.linalg.norm(Zm.T @ Zm)


def run_and_check(S, label, lst, G, want, ctx=None, history=True, residual=True, **d):
    """One ``lyap_adi`` in sweeps of G against the model's schedule `want` (adi_sweep_model.sweep_schedule) and the
    model's factor, final residual and history (`history` / `residual`: whether these two are held to HIST_BOUND[16]
    -- relative for the model's entries above 1e-6, of 1e-6 below -- or only printed).  Prints every measured figure
    before it asserts."""
    ms, ref = S.ref(lst)
    ctx = S.ctx if ctx is None else ctx
    ctx.set_adi_res_history(history)
    prm = _lib.adi_params(dict(dict(adi_max_steps=sw.STEPS, adi_newZ_reltol=0.0), ms=ms, sweep_width=G, **d))
    Z, info = ctx.lyap_adi(ms, S.W, prm)
    h = ctx.adi_res_history()
    ctx.set_adi_res_history(False)
    steps = want["steps"]
    e_z = zzt_dev(Z, ref, steps) if info["adi_steps"] == steps else np.inf
    last = ref["hist"][steps - 1]
    e_res = abs(info["res_fro"] / ref["rhs"] - last) / max(last, 1e-6)
    n = min(len(h), steps)
    big = ref["hist"][:n] > 1e-6
    dev = np.abs(h[:n] - ref["hist"][:n]) / ref["hist"][:n]
    e_h = dev[big].max() if history and big.any() else 0.0
    print("%s: steps %d (model %d), stopped by %s (%s), solves %d (%d), cols %d; Z Z^T off the model's by %.3e; "
          "res_fro / rhs %.6e (model %.6e, deviation %.3e of max(model, 1e-6)); history: %d entries, %d above 1e-6, "
          "largest relative deviation there %.3e (all: %.3e); model margin %.3f, sweeps %s"
          % (label, info["adi_steps"], steps, info["adi_stopped_by"], want["rule"], info["shift_solves"],
             want["solves"], info["cols"], e_z, info["res_fro"] / ref["rhs"], last, e_res, len(h), int(big.sum()), e_h,
             dev.max() if n else 0.0, want["margin"], want["sweeps"]))
    assert info["gmres_nonconverged"] == 0
    assert (info["adi_steps"], info["adi_stopped_by"], info["shift_solves"]) == (steps, want["rule"], want["solves"])
    if not d.get("compress_cols"):
        assert info["cols"] == Z.shape[1] == steps * M
    assert e_z <= ZZT_TOL
    assert e_res <= HIST_BOUND[16] or not residual
    if history:
        assert len(h) == steps and e_h <= HIST_BOUND[16]
    else:
        assert len(h) == 0
    return Z, info, h


# ------------------------------------------------------------------- 1. windows that are not one of the cycle's
@pytest.mark.parametrize("name", sorted(sw.CASES))
def test_cut_and_misaligned_windows(S, name):
    """The model's schedule under the reference's rule at the tolerance in the middle of the interval that gives it
    (margins 1.445 / 1.550 / 1.294 / 1.164 / 1.313): the device ends after the model's step, by the model's rule, with
    the model's number of solves -- which counts the sweeps' widths, so a window cut or narrowed otherwise shows --,
    steps * m columns, the model's Z Z^T, final residual and history.

    A - D: no window has a pivot below the 6.1e-4 at which HIST_BOUND[16] was measured.  E runs windows with pivots of
    3.2e-5 .. 1.5e-4 (the recombination amplifies the solves' errors like pivot^-1/2, and W is advanced through the
    same Cauchy data), so that figure does not cover it: E is run without a history and held on the decisions and the
    factor; its final residual is printed."""
    c = sw.CASES[name]
    ms, ref = S.ref(c["ms"])
    tol = sw.tolerance_interval(ref, ms, c["G"], c["schedule"])[2]
    want = sw.sweep_schedule(ref["rel_newZ"], ref["hist"], ms, c["G"], newZ_reltol=tol)
    assert want["sweeps"] == c["schedule"] and want["margin"] >= 1.1
    run_and_check(S, "case " + name, c["ms"], c["G"], want, history=name != "E", residual=name != "E",
                  adi_newZ_reltol=tol)


# ------------------------------------------------------------------------------------- 2. wrap-round, no rule
@pytest.mark.parametrize("name,n", [("B", 30), ("B", 40), ("D", 30), ("D", 40)])
def test_wrapped_cycle_windows_and_partial_last_sweep(S, name, n):
    """Both tolerances 0: the cycle's windows all the way (B: 3 windows of 4 over 6 shifts, the one at 4 takes shifts
    4, 5, 0, 1; D: 3 windows of 8 over 12), the last sweep partial for adi_max_steps = 30."""
    c = sw.CASES[name]
    ms, ref = S.ref(c["ms"])
    want = sw.sweep_schedule(ref["rel_newZ"], ref["hist"], ms, c["G"], max_steps=n)
    assert want["steps"] == n and want["margin"] == np.inf
    run_and_check(S, "%s, %d steps, no rule" % (name, n), c["ms"], c["G"], want, adi_max_steps=n)


# ------------------------------------------------------------------------------- 3. in-flight recompression
LIST16 = sw.CASES["C"]["ms"]


@pytest.fixture(scope="module")
def plain64(S):
    """64 steps in sweeps of 16 without recompression, on a context of its own."""
    ms, ref = S.ref(LIST16)
    want = sw.sweep_schedule(ref["rel_newZ"], ref["hist"], ms, 16)
    ctx = S.fresh()
    try:
        return run_and_check(S, "64 steps, compress_cols 0", LIST16, 16, want, ctx=ctx, adi_res_reltol=1e-300)
    finally:
        ctx.close()


@pytest.mark.parametrize("cc", [64, 65, 128])
def test_inflight_recompression_against_the_same_run_without(S, plain64, cc):
    """compress_cols = 64: a round after each of the first three sweeps (the helper thread compresses the prefix on
    the second stream while the next sweep appends behind it; finish() splices [compressed prefix | tail]); 65 and 128:
    one round, after the second sweep.  Same decisions as without; the history bitwise equal (Z is an input of nothing
    in it; each run on a fresh context, so both start from the same empty recycling store); Z Z^T the model's.

    The column count proves that the rounds ran and where the tail sits: with 64, the last splice leaves [prefix of
    the first 192 columns, compressed three times | 64], so cols - 64 is a numerical rank of those 192 columns -- the
    device truncates at 3e-8 relative (kInternalRelThresh), between the model's ranks at 1e-6 and 1e-9 (72 and 99);
    with 65 / 128 it is [first 128 columns compressed | 128]."""
    ms, ref = S.ref(LIST16)
    Z0, i0, h0 = plain64
    want = sw.sweep_schedule(ref["rel_newZ"], ref["hist"], ms, 16, m=M, compress_cols=cc)
    assert want["rounds"] == ([0, 1, 2] if cc == 64 else [1])
    ctx = S.fresh()
    try:
        Z, info, h = run_and_check(S, "64 steps, compress_cols %d" % cc, LIST16, 16, want, ctx=ctx, compress_cols=cc,
                                   adi_res_reltol=1e-300)
    finally:
        ctx.close()
    assert (info["adi_steps"], info["shift_solves"], info["adi_stopped_by"]) == \
        (i0["adi_steps"], i0["shift_solves"], i0["adi_stopped_by"])
    same = h.tobytes() == h0.tobytes()
    print("compress_cols %d: history bitwise equal to the run without: %s (largest difference %.3e); cols %d"
          % (cc, same, np.abs(h - h0).max(), info["cols"]))
    assert same
    pre = 192 if cc == 64 else 128
    lo, hi = (sw.numerical_rank(ref["Z"][:, :pre], t) for t in (1e-6, 1e-9))
    print("compress_cols %d: cols - %d = %d, model's ranks of the first %d columns at 1e-6 / 1e-9: %d / %d"
          % (cc, 256 - pre, info["cols"] - (256 - pre), pre, lo, hi))
    assert info["cols"] == Z.shape[1] and lo <= info["cols"] - (256 - pre) <= hi


def test_cut_misaligned_window_and_splice_in_one_run(S):
    """Case C with compress_cols = 32: rounds start behind the first and the second sweep (the one-shift sweep behind
    the cut adds 4 columns: none there), and the second is spliced in behind the misaligned window that drops a block:
    [first 32 blocks compressed | 1 + 7 blocks].  The decisions are case C's."""
    c = sw.CASES["C"]
    ms, ref = S.ref(c["ms"])
    tol = sw.tolerance_interval(ref, ms, 16, c["schedule"])[2]
    want = sw.sweep_schedule(ref["rel_newZ"], ref["hist"], ms, 16, newZ_reltol=tol, m=M, compress_cols=32)
    assert want["sweeps"] == c["schedule"] and want["rounds"] == [0, 1] and (want["steps"], want["solves"]) == (40, 41)
    Z, info, h = run_and_check(S, "case C, compress_cols 32", c["ms"], 16, want, adi_newZ_reltol=tol, compress_cols=32)
    lo, hi = (sw.numerical_rank(ref["Z"][:, :32 * M], t) for t in (1e-6, 1e-9))
    print("case C, compress_cols 32: cols - 32 = %d, model's ranks of the first 128 columns at 1e-6 / 1e-9: %d / %d"
          % (info["cols"] - 8 * M, lo, hi))
    assert info["cols"] == Z.shape[1] and lo <= info["cols"] - 8 * M <= hi


# ------------------------------------------------------------------------------- 4. more columns than rows
def test_odd_panel_width_through_the_splice_stays_within_the_rows():
    """The N = 8 Stokes pencil of test_gpu_parity.test_odd_panel_widths_through_adi_and_batched_solve (the regression
    for a factor with more columns than rows), m = 7 -- no multiple of 4 --, 12 shifts in sweeps of 4, a round behind
    every third sweep (28 columns each): the factor stays within its 450 rows, is the oracle's, and the iteration takes
    the steps of the run without recompression."""
    sm = pb.stokes_system(8, nu=1.0)
    Mm, A, J, NV = sm["M"], sm["A"], sm["J"], sm["NV"]
    F = (-Mm - 0.1 * A).tocsr()
    m = 7
    W = np.random.default_rng(m).standard_normal((NV, m))
    ms = pb.logshifts(2.0, 8e3, 12)
    d = dict(adi_max_steps=150, adi_newZ_reltol=1e-11, ms=ms, sweep_width=4)
    Zo = opru.solve_proj_lyap_stein(amat=F, mmat=Mm, jmat=J, wmat=W, adi_dict=d)["zfac"]
    ctx = _lib.Context(0)
    try:
        ctx.set_operator(F.T.tocsr(), Mm.T.tocsr(), J)
        Z1, i1 = ctx.lyap_adi(ms, W, _lib.adi_params(d))
        Z2, i2 = ctx.lyap_adi(ms, W, _lib.adi_params(dict(d, compress_cols=64)))
    finally:
        ctx.close()
    scale = np.linalg.norm(Zo.T @ Zo)
    e1, e2 = (opru.comp_diff_zzt_fnorm(Z, Zo) / scale for Z in (Z1, Z2))
    print("Stokes N = 8, m = 7: %d steps / %d columns without recompression, %d steps / %d columns with "
          "compress_cols = 64 (NV = %d); Z Z^T off the oracle's by %.3e / %.3e"
          % (i1["adi_steps"], i1["cols"], i2["adi_steps"], i2["cols"], NV, e1, e2))
    assert i1["cols"] == i1["adi_steps"] * m
    assert i2["cols"] == Z2.shape[1] <= NV
    assert e2 <= ZZT_TOL
    assert i2["adi_steps"] == i1["adi_steps"] and i2["adi_stopped_by"] == i1["adi_stopped_by"]


# ------------------------------------------------------------------------------------------------ 5. Newton
def test_newton_with_a_round_after_every_sweep():
    """The steady call of test_gpu_configs.test_hip_newton_adi_vs_dense_are_three_call_forms at N = 8 in sweeps of 8
    (10 shifts: 5 cycle windows that wrap) with compress_cols = 64: from the second Newton step on the panel is
    m = 4 wide, a round after every sweep.  Against scipy's dense Riccati solution, and the Newton steps of the run
    with the driver's own compress_cols (512)."""
    from identities import dense_projected_are
    tight = dict(adi_max_steps=300, adi_newZ_reltol=1e-12, nwtn_max_steps=30, nwtn_upd_reltol=1e-11,
                 nwtn_upd_abstol=1e-14)
    pr = pb.ricc_problem(8, 0.2, NU=2, NY=2, alphau=1e-3)
    mct = olau.app_prj_via_sadpnt(amat=pr.M, jmat=pr.J, rhsv=pr.mc_mat.T, transposedprj=True)
    tb = olau.apply_invsqrt_fromright(pr.rmat, pr.b_mat, output="dense")
    trct = olau.apply_invsqrt_fromright(pr.y_masmat, mct, output="dense")
    F = (-pr.A - pr.Nc).tocsr()
    X = dense_projected_are(F.T, pr.M.T, pr.J, tb, trct)
    ms = pb.logshifts(1.0, 2e3, 10)
    d = dict(tight, ms=ms, sweep_width=8)
    ctx = _lib.Context(0)
    try:
        ctx.set_operator(F.T.tocsr(), pr.M.T.tocsr(), pr.J)
        Z0, i0 = ctx.ric_newtonadi(ms, tb, trct, _lib.adi_params(d))
        Z, info = ctx.ric_newtonadi(ms, tb, trct, _lib.adi_params(dict(d, compress_cols=64)))
    finally:
        ctx.close()
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    e_x, e_k = rel(Z @ Z.T, X), rel(pr.M.T @ (Z @ (Z.T @ tb)), pr.M.T @ (X @ tb))
    print("Newton, compress_cols 64: %d Newton steps (%d with the default), %d ADI steps (%d), %d sweeps (%d), "
          "%d columns (%d); Z Z^T off the dense solution by %.3e, K by %.3e"
          % (info["nwtn_steps"], i0["nwtn_steps"], info["adi_steps"], i0["adi_steps"], info["adi_sweeps"],
             i0["adi_sweeps"], info["cols"], i0["cols"], e_x, e_k))
    assert info["adi_sweeps"] > 0 and info["gmres_nonconverged"] == 0
    assert e_x < 1e-6 and e_k < K_TOL
    assert info["nwtn_steps"] == i0["nwtn_steps"]
