"""The stopping policy of the native ADI drivers (``optconpy_amd/csrc/adi_stop.h``: ``AdiStop::cut`` and
``AdiStop::record``) on the host, against ``adi_res_model.stopping_step`` -- the model the Python driver and the GPU
tests are held to.  A probe that includes nothing but that header plays the sweep driver's loop: ``cut``, reveal
``g_now`` blocks through ``record``, stop or go on.  The per-step sequences ``b2[k]`` (squared norm of the block) and
``res[k]`` (``||W_k^T W_k||_F``) are those of the sequential iteration, which are the sweep form's too: block j of a
sweep is the block the sequential iteration appends.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from optconpy_amd import problems as pb
from oracle import lin_alg_utils as olau

from adi_res_model import AdiResModel, stopping_step

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = {0: "max_steps", 1: "newZ", 2: "res"}

PROBE = r"""
#include <cstdio>
#include <vector>
#include "adi_stop.h"
// stdin: ns G adi_max_steps newZ_reltol res_reltol res_wanted res_rhs, then b2[0..max), then res[0..max);
// res_wanted < 0: the residual is wanted by the tolerance alone and record() is never given one
int main() {
  int ns, G, max_steps, wanted;
  double newz, rtol, rhs;
  if (scanf("%d %d %d %la %la %d %la", &ns, &G, &max_steps, &newz, &rtol, &wanted, &rhs) != 7) return 2;
  std::vector<double> b2(max_steps), res(max_steps);
  for (double& x : b2) if (scanf("%la", &x) != 1) return 2;
  for (double& x : res) if (scanf("%la", &x) != 1) return 2;
  ricadi::AdiStop stop(ns, newz, rtol, max_steps, wanted > 0);
  stop.res_rhs = rhs;
  if (G > ns) G = ns;
  int steps = 0, rule = ricadi::AdiStop::kMaxSteps;
  for (;;) {
    const int g_now = stop.cut(steps, G);
    if (g_now < 1) break;
    int kept = g_now;
    bool stopped = false;
    for (int j = 0; j < g_now && !stopped; ++j) {
      const ricadi::AdiStop::Verdict v = stop.record(steps + j, b2[steps + j], stop.res_on && wanted >= 0 ? &res[steps + j] : nullptr);
      if (v.rule != ricadi::AdiStop::kMaxSteps) {
        kept = j + 1;
        stopped = true;
        rule = v.rule;
      }
    }
    steps += kept;
    printf("sweep %d %d\n", g_now, kept);
    if (stopped || steps >= max_steps) break;
  }
  printf("end %d %d\n", steps, rule);
  return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("adi_stop")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "optconpy_amd", "csrc"),
                           str(src), "-o", str(exe)])

    def run(ns, G, b2, res, newz, rtol, wanted=None, rhs=1.0):
        """-> (list of (g_now, kept) per sweep, steps, rule name)"""
        wanted = rtol > 0.0 if wanted is None else wanted
        words = [str(ns), str(G), str(len(b2)), float(newz).hex(), float(rtol).hex(), str(int(wanted)),
                 float(rhs).hex()] + [float(x).hex() for x in b2] + [float(x).hex() for x in res]
        out = subprocess.run([str(exe)], input=" ".join(words), stdout=subprocess.PIPE, text=True, check=True).stdout
        lines = [l.split() for l in out.splitlines()]
        assert lines[-1][0] == "end" and all(l[0] == "sweep" for l in lines[:-1])
        return [(int(l[1]), int(l[2])) for l in lines[:-1]], int(lines[-1][1]), RULES[int(lines[-1][2])]
    return run


def rel_of(b2):
    """Relative block norms of the model (adi_res_model.AdiResModel.step_form)."""
    return np.sqrt(np.asarray(b2) / np.cumsum(b2))


def synthetic(ns, steps, wobble):
    """Geometric decay per cycle position, another ratio at every position, times a deterministic +-20 % wobble:
    (b2, res), res_rhs = 1.  The squared block norms fall by 0.03 .. 0.15 per visit (their relative norms by a factor
    2.6 .. 6), the residuals by 0.1 .. 0.4."""
    k = np.arange(steps)
    pos, visit = k % ns, k // ns
    frac = (pos + 0.5) / ns
    w_b = 1.0 + wobble * 0.2 * np.sin(1.7 * k + 0.3)
    w_r = 1.0 + wobble * 0.2 * np.cos(2.3 * k + 1.1)
    b2 = 4.0 ** (-frac) * (0.03 + 0.12 * ((7 * pos + 3) % ns + 0.5) / ns) ** visit * w_b
    res = 0.5 * 3.0 ** (-frac) * (0.1 + 0.3 * ((5 * pos + 1) % ns + 0.5) / ns) ** visit * w_r
    return b2, res


def gap_tol(seq, first):
    """(k, tol): smallest 0-based k >= first whose entry lies a factor >= 2 below every earlier one, and the
    tolerance in the middle of that gap, tol = sqrt(min(seq[:k]) seq[k]): entry k is the first at or below tol, with
    a factor sqrt(2) to spare on either side, so that rounding in the probe cannot move the step.  (For a falling
    sequence this is tests/test_gpu_adi_res.py::_gap_step: a gap between consecutive entries.  With another decay
    rate at every cycle position the sequences here do not fall monotonically.)"""
    for k in range(max(first, 1), len(seq)):
        low = seq[:k].min()
        if low / seq[k] >= 2.0:
            return k, float(np.sqrt(low * seq[k]))
    raise AssertionError("no gap of a factor 2 from entry %d on" % first)


def check(probe, ns, G, b2, res, newz, rtol, wanted=None, rhs=1.0):
    """Agreement with the model, and the cuts never change the answer.  Returns the sweeps."""
    sweeps, steps, rule = probe(ns, G, b2, res, newz, rtol, wanted, rhs)
    want = stopping_step(rel_of(b2), np.asarray(res) / rhs, newz, rtol)
    assert (steps, rule) == want, (ns, G, newz, rtol, sweeps)
    assert sum(kept for _, kept in sweeps) == steps
    before = 0
    for g_now, kept in sweeps:
        assert 1 <= kept <= g_now <= min(G, ns, len(b2) - before), (sweeps, before)
        before += kept
    assert all(kept == g_now for g_now, kept in sweeps[:-1])        # only the sweep that stops is truncated
    return sweeps


def rule_settings(b2, res, first):
    """(newZ_reltol, res_reltol) with only the first rule on, only the second, both with either firing first, and
    neither -- each tolerance in a gap at or behind entry `first`."""
    rel = rel_of(b2)
    kz, tz = gap_tol(rel, first)
    kr, tr = gap_tol(res, first)
    kz2, tz2 = gap_tol(rel, kr + 1)           # the reference's rule behind the residual rule's step, and the reverse
    kr2, tr2 = gap_tol(res, kz + 1)
    assert kz2 > kr and kr2 > kz
    return [(tz, 0.0), (0.0, tr), (tz2, tr), (tz, tr2), (0.0, 0.0)]


@pytest.mark.parametrize("ns", [1, 3, 16])
@pytest.mark.parametrize("G", [1, 2, 8, 16])
def test_agreement_with_the_model_on_synthetic_histories(probe, ns, G):
    steps = 10 * ns if ns < 16 else 80
    b2, res = synthetic(ns, steps, wobble=1.0)
    for first in (2, 2 * ns + 1):             # inside the first pass over the cycle; behind two full passes
        for newz, rtol in rule_settings(b2, res, first):
            check(probe, ns, G, b2, res, newz, rtol)
    # neither rule, the residual evaluated all the same (history on request): adi_max_steps, max_steps
    sweeps, n, rule = probe(ns, G, b2, res, 0.0, 0.0, wanted=True)
    assert (n, rule) == (steps, "max_steps") and all(g == min(G, ns) for g, _ in sweeps[:-1])


@pytest.fixture(scope="module")
def real_pair():
    """b2, res and ||W_0^T W_0||_F of the model's step form on the N = 15 problem of tests/test_gpu_adi_res.py (16
    shifts over three decades, 32 steps)."""
    pr = pb.ricc_problem(15, 0.05, NU=2, NY=2)
    F = (-pr.A - pr.Nc).tocsr()
    mct = olau.app_prj_via_sadpnt(amat=pr.M, jmat=pr.J, rhsv=pr.mc_mat.T, transposedprj=True)
    W = olau.apply_invsqrt_fromright(pr.y_masmat, mct, output="dense")
    mdl = AdiResModel(F.T, pr.M.T, pr.J)
    ref = mdl.step_form(mdl.project(W), pb.logshifts(1.0, 1e3, 16), 32)
    b2 = np.array([float(np.sum(z * z)) for z in ref["Z"]])
    assert np.allclose(rel_of(b2), ref["rel_newZ"], rtol=1e-12)
    return b2, ref["hist"] * ref["rhs"], ref["rhs"]


@pytest.mark.parametrize("G", [1, 2, 8, 16])
def test_agreement_with_the_model_on_a_real_history(probe, real_pair, G):
    b2, res, rhs = real_pair
    hist = res / rhs
    for first in (4, 18):                     # inside the first sweep of 16 and inside the second
        k, tol = gap_tol(hist, first)
        check(probe, 16, G, b2, res, 0.0, tol, rhs=rhs)
        kz, tz = gap_tol(rel_of(b2), first)
        check(probe, 16, G, b2, res, tz, 0.0, rhs=rhs)
        check(probe, 16, G, b2, res, tz, tol, rhs=rhs)
    check(probe, 16, G, b2, res, 0.0, 0.0, rhs=rhs)


@pytest.mark.parametrize("ns,G", [(1, 1), (3, 2), (3, 3), (16, 8), (16, 16)])
def test_the_cut_is_exact_for_exactly_geometric_decay(probe, ns, G):
    """No wobble, and the stopping step behind two full passes over the cycle: the prediction is then the value itself
    (up to rounding, far inside the gap), the last sweep is cut at the stopping step and no solve behind it is spent:
    kept == g_now.  This is the property that saves solves, not a correctness requirement -- a wrong prediction costs
    solves or one more sweep, never the answer (check())."""
    steps = 10 * ns if ns < 16 else 80
    b2, res = synthetic(ns, steps, wobble=0.0)
    for newz, rtol in rule_settings(b2, res, 2 * ns + 1)[:4]:
        sweeps = check(probe, ns, G, b2, res, newz, rtol)
        assert sweeps[-1][0] == sweeps[-1][1], (newz, rtol, sweeps)


def test_ties_and_precedence(probe):
    """Powers of two, so that every quotient and root below is exact.  b2 = 3, 1: the second block's relative norm is
    sqrt(1/4) = 1/2.  res = 1/2, 1/8 with res_rhs = 1."""
    b2, res = [3.0, 1.0, 2.0 ** -40], [0.5, 0.125, 2.0 ** -30]
    assert rel_of(b2)[1] == 0.5
    # a relative block norm EQUAL to adi_newZ_reltol does not stop (<): the third block does
    assert probe(1, 1, b2, res, 0.5, 0.0)[1:] == (3, "newZ")
    assert probe(1, 1, b2, res, 0.5000000000000001, 0.0)[1:] == (2, "newZ")
    # a relative residual EQUAL to adi_res_reltol stops (<=), by 'res'
    assert probe(1, 1, b2, res, 0.0, 0.125)[1:] == (2, "res")
    assert probe(1, 1, b2, res, 0.0, 0.12499999999999999)[1:] == (3, "res")
    # both fire at step 2: the reference's rule is reported
    assert probe(1, 1, b2, res, 0.75, 0.125)[1:] == (2, "newZ")
    # the same inside one sweep of three distinct shifts
    assert probe(3, 3, b2, res, 0.5, 0.125) == ([(3, 2)], 2, "res")
    assert probe(3, 3, b2, res, 0.75, 0.125) == ([(3, 2)], 2, "newZ")
    for case in ((0.5, 0.0), (0.0, 0.125), (0.75, 0.125)):
        assert probe(1, 1, b2, res, *case)[1:] == stopping_step(rel_of(b2), res, *case)


def test_without_a_residual_the_residual_rule_never_fires(probe):
    """Residual not evaluated (record() without one): residuals far below any tolerance change nothing, the run ends
    by the reference's rule or at adi_max_steps."""
    b2, _ = synthetic(3, 30, wobble=1.0)
    dead = np.zeros(30)
    k, tz = gap_tol(rel_of(b2), 4)
    for G in (1, 3):
        assert probe(3, G, b2, dead, tz, 0.0, wanted=False)[1:] == (k + 1, "newZ")
        assert probe(3, G, b2, dead, 0.0, 0.0, wanted=False)[1:] == (30, "max_steps")
    # ... and evaluated but the rule off (history on request): still never 'res'
    assert probe(3, 3, b2, dead, 0.0, 0.0, wanted=True)[1:] == (30, "max_steps")
    # ... and the rule on but record() given no residual
    assert probe(3, 3, b2, dead, 0.0, 1e-3, wanted=-1)[1:] == (30, "max_steps")
    assert probe(3, 3, b2, dead, 0.0, 1e-3, wanted=True)[1:] == (1, "res")
