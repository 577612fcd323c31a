// adi_stop.h -- the stopping policy of the low-rank ADI drivers (solver_adi.inl): the two rules, what they remember,
// and the prediction that cuts a sweep.  Host arithmetic on the C++ standard library alone, so that a test can
// compile it by itself (tests/test_adi_stop_cpu.py).  Every comparison against a tolerance is in this file.
#pragma once

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace ricadi {

struct AdiStop {
  // the values of RICADI_STOP_* (include/ricadi.h; asserted where the drivers include both)
  enum Rule { kMaxSteps = 0, kNewZ = 1, kRes = 2 };
  struct Verdict {
    double rel;      // ||Z_j||_F / ||[Z_1 .. Z_j]||_F
    double res;      // ||W_j^T W_j||_F / ||W_0^T W_0||_F (0 without a residual)
    int rule;        // the rule that ends the iteration at this block; kMaxSteps: none does
  };

  const int ns;                     // length of the shift cycle
  const double adi_newZ_reltol;     // the reference's rule: rel < adi_newZ_reltol
  const double adi_res_reltol;      // the residual rule: res <= adi_res_reltol (0: off)
  const int adi_max_steps;
  const bool res_on;                // the residual is evaluated at all (the rule, or the history alone)
  double znorm2 = 0.0;              // ||[Z_1 .. Z_j]||_F^2
  double res_rhs = -1.0;            // ||W_0^T W_0||_F, set by the driver from its first Gram matrix
  // value at the last (h1) and the last but one (h2) visit of every position of the shift cycle
  std::vector<double> rel_h1, rel_h2, res_h1, res_h2;

  AdiStop(int ns_, double newZ_reltol, double res_reltol, int max_steps, bool res_wanted)
      : ns(ns_), adi_newZ_reltol(newZ_reltol), adi_res_reltol(res_reltol), adi_max_steps(max_steps),
        res_on(res_wanted || res_reltol > 0.0), rel_h1(ns_, 0.0), rel_h2(ns_, 0.0), res_h1(res_on ? ns_ : 0, 0.0),
        res_h2(res_on ? ns_ : 0, 0.0) {}

  // Width of the sweep that starts after `steps` steps, at most G.  Block j of a sweep is the block the step-by-step
  // iteration appends at that step, so the rules below end both forms after the same step; so that the solves behind
  // the stopping step are not spent in vain, the last two passes over the shift cycle predict that step (per cycle
  // position: same shift, geometric decay) and the sweep is cut there -- on the block norms, then, up to the width
  // that left, on the residuals.  A wrong prediction costs solves or a sweep, never the answer.
  int cut(int steps, int G) const {
    int g_now = G;
    if (adi_newZ_reltol > 0.0)
      for (int g = 0; g < g_now; ++g)
        if (predicted(rel_h1, rel_h2, (steps + g) % ns) < adi_newZ_reltol) {
          g_now = g + 1;
          break;
        }
    if (adi_res_reltol > 0.0)
      for (int g = 0; g < g_now; ++g)
        if (predicted(res_h1, res_h2, (steps + g) % ns) <= adi_res_reltol) {
          g_now = g + 1;
          break;
        }
    return std::min(g_now, adi_max_steps - steps);
  }

  // The block that step `step_index` (0-based) reveals: b2 its squared Frobenius norm, res_abs the ||W^T W||_F behind
  // it (null: not evaluated).  The reference's rule comes first; a step at which both fire reports it.
  Verdict record(int step_index, double b2, const double* res_abs) {
    const int pos = step_index % ns;
    znorm2 += b2;
    Verdict v{znorm2 > 0.0 ? std::sqrt(b2 / znorm2) : 0.0, 0.0, kMaxSteps};
    rel_h2[pos] = rel_h1[pos];
    rel_h1[pos] = v.rel;
    if (v.rel < adi_newZ_reltol) v.rule = kNewZ;
    if (res_on && res_abs) {
      v.res = res_rhs > 0.0 ? *res_abs / res_rhs : 0.0;
      res_h2[pos] = res_h1[pos];
      res_h1[pos] = v.res;
      if (v.rule == kMaxSteps && adi_res_reltol > 0.0 && v.res <= adi_res_reltol) v.rule = kRes;
    }
    return v;
  }

 private:
  // geometric extrapolation of the last two visits; +inf where they do not decay
  static double predicted(const std::vector<double>& h1, const std::vector<double>& h2, int pos) {
    if (h1[pos] > 0.0 && h2[pos] > h1[pos]) return h1[pos] * (h1[pos] / h2[pos]);
    return std::numeric_limits<double>::infinity();
  }
};

}  // namespace ricadi
