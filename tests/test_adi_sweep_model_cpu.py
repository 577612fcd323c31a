"""The schedule model of the sweep-form ADI (``tests/adi_sweep_model.py``) on the host: against the stopping policy
``adi_stop.h`` played by the probe of ``tests/test_adi_stop_cpu.py``, against ``ricadi_host_adi_window_width`` (the
narrowing of a window that ``cauchy_data`` refuses), and the premises of ``tests/test_gpu_adi_sweep_paths.py``: the
schedules of its cases, recomputed from the dense model on the N = 8 problem.  CPU only.

Recomputed table (model on ``pb.ricc_problem(8, 0.05, NU=2, NY=2)``: NV = 450, n = 530, m = 4; reference's rule, the
tolerance in the geometric middle of the interval that gives the schedule; adi_max_steps = 64):

  case  shifts                   G   interval of adi_newZ_reltol    tolerance   steps / solves  margin
  A     logshifts(1, 1e3, 8)     8   1.0169e-3 .. 2.1246e-3         1.4699e-3   22 / 22         1.445
  B     logshifts(1, 300, 6)     4   1.8505e-3 .. 4.4441e-3         2.8677e-3   18 / 18         1.550
  C     logshifts(1, 1e3, 16)    16  4.3067e-6 .. 7.2067e-6         5.5711e-6   40 / 41         1.294
  D     logshifts(1, 1e3, 12)    8   5.8256e-5 .. 7.8972e-5         6.7828e-5   32 / 32         1.164
  E     logshifts(.5, 1e2, 16)   16  6.9945e-6 .. 1.2050e-5         9.1805e-6   64 / 64         1.313

A - D are the schedules and margins of the issue that asked for these tests; E is a real input whose windows (34, 16)
and (42, 16) are refused by the pivot bound.  Under the RESIDUAL rule no tolerance gives case A's list a misaligned
window of two or more shifts: the model's residual falls at every step, so behind a cut every later prediction is at
or below the tolerance too and the run goes on one shift at a time
(test_residual_rule_on_case_a_never_widens_again) -- the GPU file therefore has no such run."""
import numpy as np
import pytest

from optconpy_amd import _lib, problems as pb

from adi_res_model import AdiResModel, stopping_step
import adi_sweep_model as sw
from test_adi_stop_cpu import probe, rel_of, gap_tol          # noqa: F401  (probe: the fixture, imported not copied)

TABLE = {"A": (22, 22, 1.445), "B": (18, 18, 1.550), "C": (40, 41, 1.294), "D": (32, 32, 1.164), "E": (64, 64, 1.313)}
LISTS16 = [(1.0, 1e3, 16), (1.0, 1e2, 16), (1.0, 3e3, 16)]


@pytest.fixture(scope="module")
def refs():
    """name -> (shifts, step form of the model over sw.STEPS steps), computed once, read only."""
    pr, F, W = sw.problem_n8()
    assert (pr.NV, pr.NV + pr.J.shape[0], W.shape[1]) == (450, 530, 4)
    mdl = AdiResModel(F.T, pr.M.T, pr.J)
    assert mdl.Th.shape[1] == 370
    W0 = mdl.project(W)
    out = {}
    for name, c in sw.CASES.items():
        ms = pb.logshifts(*c["ms"])
        out[name] = (ms, mdl.step_form(W0, ms, sw.STEPS))
    return out


def _b2_res(ref):
    b2 = np.array([float(np.sum(z * z)) for z in ref["Z"]])
    assert np.allclose(rel_of(b2), ref["rel_newZ"], rtol=1e-12)
    return b2, ref["hist"] * ref["rhs"]


# ------------------------------------------------------------------------------------ 1. model against policy code
@pytest.mark.parametrize("name", sorted(sw.CASES))
def test_model_schedule_equals_the_policy_codes(probe, refs, name):
    """adi_stop.h through the probe (cut, reveal, stop or go on; it knows nothing of pivots) against the model with
    the pivot rule off: the same (g, kept) per sweep, step and rule -- the case's own tolerance, tolerances in gaps of
    the residual history inside the first, second and third pass, both rules together, and neither."""
    ms, ref = refs[name]
    c = sw.CASES[name]
    b2, res = _b2_res(ref)
    ns, G = len(ms), c["G"]
    tz = sw.tolerance_interval(ref, ms, G, c["schedule"])[2]
    settings = [(tz, 0.0), (0.0, 0.0)]
    for first in (2, ns + 2, 2 * ns + 2):
        k, tr = gap_tol(ref["hist"][:sw.STEPS - 8], first)
        settings += [(0.0, tr), (tz, tr)]
    for newz, rtol in settings:
        want = sw.sweep_schedule(ref["rel_newZ"], ref["hist"], ms, G, newZ_reltol=newz, res_reltol=rtol,
                                 pivot_rule="none")
        assert want["margin"] >= 1.001, (name, newz, rtol, want["margin"])     # (the probe's b2 is rounded anew)
        sweeps, steps, rule = probe(ns, G, b2, res, newz, rtol, rhs=ref["rhs"])
        assert sweeps == [(g, kept) for _, g, kept in want["sweeps"]], (name, newz, rtol)
        assert (steps, rule) == (want["steps"], want["rule"]) == stopping_step(ref["rel_newZ"], ref["hist"], newz, rtol)
        assert want["asked"] == [g for _, g, _ in want["sweeps"]]


# --------------------------------------------------------------------------------- 2. premises of the GPU tests
@pytest.mark.parametrize("name", sorted(sw.CASES))
def test_cases_have_the_listed_schedules_with_margin(refs, name):
    ms, ref = refs[name]
    c = sw.CASES[name]
    lo, hi, tol, margin = sw.tolerance_interval(ref, ms, c["G"], c["schedule"])
    out = sw.sweep_schedule(ref["rel_newZ"], ref["hist"], ms, c["G"], newZ_reltol=tol)
    print("case %s: adi_newZ_reltol in (%.4e, %.4e), middle %.4e, margin %.3f, steps %d, solves %d, asked %s"
          % (name, lo, hi, tol, margin, out["steps"], out["solves"], out["asked"]))
    steps, solves, table_margin = TABLE[name]
    assert out["sweeps"] == c["schedule"] and (out["steps"], out["solves"]) == (steps, solves)
    assert out["rule"] == ("max_steps" if name == "E" else "newZ")
    assert margin >= 1.1 and abs(margin - table_margin) < 0.01
    assert np.isclose(margin, np.sqrt(hi / lo))               # every compared quantity is an end of some interval
    # what each case is there for
    mis = [(f, g, k) for f, g, k in out["sweeps"] if f % c["G"]]
    assert mis and any(g >= 2 for _, g, _ in mis)             # a misaligned window of more than one shift runs
    assert all(sw.admissible(ms, f, g) for f, g, _ in out["sweeps"])
    if name == "B":
        assert len(sw.aligned_windows(6, 4)) == 3 and (13, 4, 4) in out["sweeps"]
    if name == "C":
        assert out["sweeps"][-1] == (33, 8, 7)                # a block dropped on a misaligned window
    if name == "E":
        assert out["asked"] == [16, 16, 1, 1, 16, 16, 14] and out["sweeps"][4:6] == [(34, 8, 8), (42, 8, 8)]
        assert not sw.admissible(ms, 34, 16) and not sw.admissible(ms, 42, 16)
        with pytest.raises(sw.WindowRefused):
            sw.sweep_schedule(ref["rel_newZ"], ref["hist"], ms, 16, newZ_reltol=tol, pivot_rule="throw")
    else:
        assert out["asked"] == [g for _, g, _ in out["sweeps"]]          # nothing narrowed: the parent's sweeps
        # no window of these runs has a smaller pivot than the aligned sweep of logshifts(1, 1e3, 16)
        assert min(sw.window_pivot(ms, f, g) for f, g, _ in out["sweeps"]) >= 6.0e-4


def _breakpoints(seq, ns):
    vals = set(float(v) for v in seq)
    for k in range(ns, len(seq)):
        a, b = seq[k], seq[k - ns]
        if a > 0.0 and b > a:
            vals.add(float(a * (a / b)))
    vals = np.array(sorted(vals))
    return np.sqrt(vals[:-1] * vals[1:])


def test_residual_rule_on_case_a_never_widens_again(refs):
    """Every tolerance between two neighbouring compared quantities: where a run stopped by the residual rule leaves
    the aligned cycle, it goes on one shift at a time."""
    ms, ref = refs["A"]
    seen = 0
    for tol in _breakpoints(ref["hist"], len(ms)):
        out = sw.sweep_schedule(ref["rel_newZ"], ref["hist"], ms, 8, res_reltol=tol)
        mis = [(f, g, k) for f, g, k in out["sweeps"] if f % 8]
        seen += bool(mis)
        assert all(g == 1 for _, g, _ in mis), (tol, out["sweeps"])
    assert seen >= 10


def test_wrap_round_runs_without_a_rule(refs):
    """Neither rule: aligned sweeps all the way, the last one partial where G does not divide adi_max_steps; B's cycle
    wraps round the list."""
    for name in ("B", "D"):
        ms, ref = refs[name]
        G = sw.CASES[name]["G"]
        for n in (30, 40):
            out = sw.sweep_schedule(ref["rel_newZ"], ref["hist"], ms, G, max_steps=n)
            assert (out["steps"], out["rule"], out["solves"], out["margin"]) == (n, "max_steps", n, np.inf)
            full = [(k * G, G, G) for k in range(n // G)]
            assert out["sweeps"] == full + ([(n - n % G, n % G, n % G)] if n % G else [])
        assert out["asked"] == [g for _, g, _ in out["sweeps"]]
    ms = refs["B"][0]
    order = [tuple(int(np.flatnonzero(np.asarray(ms) == p)[0]) for p in sw.window(ms, f, g))
             for f, g in sw.aligned_windows(6, 4)]
    assert order == [(0, 1, 2, 3), (4, 5, 0, 1), (2, 3, 4, 5)]


def test_recompression_rounds_and_rank_band(refs):
    """The rounds of the in-flight recompression: with compress_cols <= G m after every full sweep that is not the
    last, with 2 G m after every second; and the band the column count of the compress_cols = 64 run must lie in."""
    ms, ref = refs["C"]
    for cc, rounds in ((64, [0, 1, 2]), (65, [1]), (128, [1]), (0, [])):
        out = sw.sweep_schedule(ref["rel_newZ"], ref["hist"], ms, 16, m=4, compress_cols=cc)
        assert out["steps"] == 64 and out["rounds"] == rounds, (cc, out["rounds"])
    # case C with compress_cols = 32: a round behind every sweep but the last, the cut one-shift sweep included
    tol = sw.tolerance_interval(ref, ms, 16, sw.CASES["C"]["schedule"])[2]
    out = sw.sweep_schedule(ref["rel_newZ"], ref["hist"], ms, 16, newZ_reltol=tol, m=4, compress_cols=32)
    assert out["sweeps"] == sw.CASES["C"]["schedule"] and out["rounds"] == [0, 1]
    Z = np.hstack(ref["Z"])
    lo, mid, hi = (sw.numerical_rank(Z[:, :192], t) for t in (1e-6, 3e-8, 1e-9))
    print("numerical rank of the first 192 columns at 1e-6 / 3e-8 / 1e-9 relative: %d / %d / %d" % (lo, mid, hi))
    assert (lo, hi) == (72, 99) and lo < mid < hi


# ------------------------------------------------------------------- 3. host entry against the model's pivots
def test_host_window_width_against_the_models_pivots():
    lists = [pb.logshifts(*l) for l in LISTS16] + [pb.logshifts(*c["ms"]) for c in sw.CASES.values()]
    for ms in lists:
        ns = len(ms)
        G = min(16, ns)
        for f, g in sw.aligned_windows(ns, G):
            assert sw.admissible(ms, f, g) and _lib.host_adi_window_width(ms, f, g) == g
        for first in range(2 * ns):
            for g in range(1, G + 1):
                w = _lib.host_adi_window_width(ms, first, g)
                assert w == sw.run_width(ms, first, g), (first, g)
                assert sw.admissible(ms, first, w)
                _lib.host_cauchy(sw.window(ms, first, w))                     # cauchy_data itself takes it
                if w < g:
                    # the width before it in the halving g, g // 2, .. (2 w for a power of two) is refused
                    chain = [g >> i for i in range(5) if g >> i > w]
                    assert chain[-1] // 2 == w and not sw.admissible(ms, first, chain[-1])
                    with pytest.raises(RuntimeError):
                        _lib.host_cauchy(sw.window(ms, first, chain[-1]))
            assert _lib.host_adi_window_width(ms, first, 1) == 1
    # the two windows of the study: smallest pivot over all windows, narrowed to 8
    for lst, first, aligned, worst in (((1.0, 1e3, 16), 9, 6.10e-4, 5.72e-7), ((1.0, 1e2, 16), 8, 4.78e-6, 1.74e-10)):
        ms = pb.logshifts(*lst)
        assert np.isclose(sw.window_pivot(ms, 0, 16), aligned, rtol=5e-3)
        assert np.isclose(sw.window_pivot(ms, first, 16), worst, rtol=5e-3)
        assert np.isclose(sw.worst_window(ms, 16)[0], worst, rtol=5e-3)
        assert _lib.host_adi_window_width(ms, first, 16) == 8
        assert sw.admissible(ms, first, 8) and not sw.admissible(ms, first, 16)
    ms = pb.logshifts(1.0, 3e3, 16)                                           # the benchmark's list: nothing narrowed
    assert np.isclose(sw.worst_window(ms, 16)[0], 6.40e-6, rtol=5e-3)
    assert all(_lib.host_adi_window_width(ms, f, 16) == 16 for f in range(16))


def test_host_window_width_on_an_unsorted_list():
    """The interleaved 32-shift list (a permutation of a log-spaced one): both aligned sweeps of 16 pass, the window
    rotated by 8 does not (pivot 3.2e-7) and runs 8 wide."""
    ms = pb.logshifts(1.0, 3e3, 32, interleave=True)
    assert sorted(ms, reverse=True) == list(pb.logshifts(1.0, 3e3, 32)) and list(ms) != sorted(ms, reverse=True)
    for f, g in sw.aligned_windows(32, 16):
        assert sw.window_pivot(ms, f, g) > 1e-3 and _lib.host_adi_window_width(ms, f, g) == 16
    assert 1e-7 < sw.window_pivot(ms, 8, 16) < 1e-6
    assert _lib.host_adi_window_width(ms, 8, 16) == 8 == sw.run_width(ms, 8, 16)
    for first in range(32):
        assert _lib.host_adi_window_width(ms, first, 16) == sw.run_width(ms, first, 16)


def test_host_window_width_refuses_bad_arguments():
    ms = pb.logshifts(1.0, 1e3, 8)
    for first, g in ((-1, 4), (0, 0), (0, 9), (0, 17)):
        with pytest.raises(ValueError):
            _lib.host_adi_window_width(ms, first, g)
    with pytest.raises(ValueError):
        _lib.host_adi_window_width([-1.0, 2.0], 0, 2)
    # equal shifts inside the window: cauchy_data refuses, the width falls to what has distinct shifts
    assert _lib.host_adi_window_width([-1.0, -1.0, -5.0, -30.0], 0, 4) == 1
    assert _lib.host_adi_window_width([-1.0, -1.0, -5.0, -30.0], 1, 3) == 3


# ------------------------------------------------------------------------------------- 4. a synthetic history
def dipped(ns, steps, dip_pos):
    """In the style of test_adi_stop_cpu.synthetic: geometric decay per cycle position (squared block norms fall by
    0.3 per visit, residuals by 0.2), and ONE dip -- the second visit of position `dip_pos` is 1e-3 of its place in
    the sequence -- so that the extrapolation to its third visit is far too small: a mispredicted cut."""
    k = np.arange(steps)
    pos, visit = k % ns, k // ns
    frac = (pos + 0.5) / ns
    b2 = 4.0 ** (-frac) * 0.3 ** visit
    res = 0.5 * 3.0 ** (-frac) * 0.2 ** visit
    b2[ns + dip_pos] *= 1e-3
    return b2, res


def test_a_cut_that_leaves_the_refused_window(probe):
    """logshifts(1, 1e3, 16), G = 16, adi_max_steps = 57.  The dip at step 24 makes `cut` end the third sweep with
    step 41's block, which does not stop: steps = 41 = 9 mod 16 with 16 more to go, the window whose pivot is 5.7e-7.
    The policy (probe) asks for 16 there; before the narrowing that was the throw; now it runs 8 + 8, and the run
    ends where stopping_step says."""
    ms = pb.logshifts(1.0, 1e3, 16)
    b2, res = dipped(16, 57, 8)
    rel = rel_of(b2)
    pred = rel[24] * (rel[24] / rel[8])
    tol = float(np.sqrt(pred * rel[24]))
    assert pred * 4.0 < tol < rel[24] / 4.0 and rel[24] < np.delete(rel, 24).min()
    want = stopping_step(rel, res, tol, 0.0)
    assert want == (57, "max_steps")
    sweeps, steps, rule = probe(16, 16, b2, res, tol, 0.0)
    assert sweeps == [(16, 16), (16, 16), (9, 9), (16, 16)] and (steps, rule) == want
    none = sw.sweep_schedule(rel, res, ms, 16, newZ_reltol=tol, pivot_rule="none")
    assert [(g, k) for _, g, k in none["sweeps"]] == sweeps
    with pytest.raises(sw.WindowRefused, match=r"window \(41, 16\)"):
        sw.sweep_schedule(rel, res, ms, 16, newZ_reltol=tol, pivot_rule="throw")
    out = sw.sweep_schedule(rel, res, ms, 16, newZ_reltol=tol)
    assert out["sweeps"] == [(0, 16, 16), (16, 16, 16), (32, 9, 9), (41, 8, 8), (49, 8, 8)]
    assert out["asked"] == [16, 16, 9, 16, 8] and out["margin"] >= 4.0
    assert (out["steps"], out["rule"]) == want and out["solves"] == 57
    # the library's own decision at these windows
    assert _lib.host_adi_window_width(ms, 41, 16) == 8 and _lib.host_adi_window_width(ms, 49, 8) == 8
    assert _lib.host_adi_window_width(ms, 32, 9) == 9
    with pytest.raises(RuntimeError):
        _lib.host_cauchy(sw.window(ms, 41, 16))
