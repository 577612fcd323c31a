// pair_smw.h -- the host arithmetic of the pair step's complex solve (solver_adi_pairs.inl, struct PairSolve; DESIGN.md
// section 3g): the scalars of a pair step, the grouping of its m + q columns, the map from a step column to its place
// in the groups, the q x q capacitance matrix of the Sherman-Morrison-Woodbury correction with its LU, and the real
// embedding of the complex coefficients.  Host arithmetic on the C++ standard library alone, so that a test can
// compile it by itself (tests/test_pair_smw_cpu.py).
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstddef>
#include <utility>
#include <vector>

namespace ricadi {

using cdbl = std::complex<double>;

// LU with partial pivoting of the q x q matrix `a` (row-major) in place; false: a pivot below 1e-13 max |a_ij|.
// min_pivot_rel (optional): the smallest pivot modulus met, over max |a_ij| (0 for a zero matrix).
inline bool pair_lu(std::vector<cdbl>& a, std::vector<int>& piv, int q, double* min_pivot_rel = nullptr) {
  double scale = 0.0;
  for (const cdbl& v : a) scale = std::max(scale, std::abs(v));
  piv.assign(q, 0);
  double low = INFINITY;
  if (min_pivot_rel) *min_pivot_rel = 0.0;
  for (int k = 0; k < q; ++k) {
    int pk = k;
    for (int i = k + 1; i < q; ++i)
      if (std::abs(a[(size_t)i * q + k]) > std::abs(a[(size_t)pk * q + k])) pk = i;
    piv[k] = pk;
    if (pk != k)
      for (int j = 0; j < q; ++j) std::swap(a[(size_t)k * q + j], a[(size_t)pk * q + j]);
    const cdbl d = a[(size_t)k * q + k];
    if (scale > 0.0) low = std::min(low, std::abs(d) / scale);
    if (min_pivot_rel) *min_pivot_rel = scale > 0.0 ? low : 0.0;
    if (!(std::abs(d) >= 1e-13 * scale) || scale == 0.0) return false;
    for (int i = k + 1; i < q; ++i) {
      const cdbl f = a[(size_t)i * q + k] / d;
      a[(size_t)i * q + k] = f;
      for (int j = k + 1; j < q; ++j) a[(size_t)i * q + j] -= f * a[(size_t)k * q + j];
    }
  }
  return true;
}
// y (q x w, row-major) <- a^-1 y with the factors of pair_lu
inline void pair_lu_solve(const std::vector<cdbl>& a, const std::vector<int>& piv, int q, std::vector<cdbl>& y, int w) {
  for (int k = 0; k < q; ++k)
    if (piv[k] != k)
      for (int j = 0; j < w; ++j) std::swap(y[(size_t)k * w + j], y[(size_t)piv[k] * w + j]);
  for (int k = 0; k < q; ++k)
    for (int i = k + 1; i < q; ++i)
      for (int j = 0; j < w; ++j) y[(size_t)i * w + j] -= a[(size_t)i * q + k] * y[(size_t)k * w + j];
  for (int k = q - 1; k >= 0; --k)
    for (int j = 0; j < w; ++j) {
      cdbl sacc = y[(size_t)k * w + j];
      for (int l = k + 1; l < q; ++l) sacc -= a[(size_t)k * q + l] * y[(size_t)l * w + j];
      y[(size_t)k * w + j] = sacc / a[(size_t)k * q + k];
    }
}

// The scalars of a pair step
struct PairCoefs {
  double delta, gam, gam2;
  PairCoefs(double a, double b) {
    delta = a / b;
    gam = 2.0 * std::sqrt(-a);
    const double d2 = delta * delta;
    gam2 = gam * std::sqrt(d2 + 1.0);
  }
};

// The mp = m + q real columns of a step -- W and, behind it, U -- travel as ng groups of mc complex columns: step
// column j is complex column j % mc of group j / mc; the columns behind mp in the last group are padding.
struct PairGroups {
  int ng, mc;
  explicit PairGroups(int mp) : ng((mp + 7) / 8), mc((mp + ng - 1) / ng) {}
  int group_of(int j) const { return j / mc; }
  int col_of(int j) const { return j % mc; }
  int m2() const { return 2 * mc; }
  // step columns [j0, j1) of U (step columns m .. mp) that group g holds; empty where j0 >= j1
  std::pair<int, int> u_range(int g, int m, int mp) const { return {std::max(m, g * mc), std::min(mp, (g + 1) * mc)}; }
  // columns of W in group g: the first c0 of its mc
  int w_cols(int g, int m) const { return std::min(mc, std::max(0, m - g * mc)); }
};

// (V^T D)[k][step column j] from ht, the q x 2 mc real products of the ng groups (row k of group g at (g q + k) 2 mc,
// complex column cc at 2 cc)
inline cdbl pair_t_at(const double* ht, const PairGroups& pg, int q, int k, int j) {
  const double* t = ht + ((size_t)pg.group_of(j) * q + k) * pg.m2() + 2 * pg.col_of(j);
  return cdbl(t[0], t[1]);
}

// cap (q x q, row-major) <- I - V^T X_U: X_U are the step columns m .. m + q
inline void pair_capacitance(const double* ht, const PairGroups& pg, int m, int q, std::vector<cdbl>& cap) {
  cap.assign((size_t)q * q, cdbl(0.0, 0.0));
  for (int k = 0; k < q; ++k)
    for (int l = 0; l < q; ++l) cap[(size_t)k * q + l] = (k == l ? 1.0 : 0.0) - pair_t_at(ht, pg, q, k, m + l);
}

// y (q x m, row-major) <- V^T D_W: the step columns 0 .. m
inline void pair_vtw(const double* ht, const PairGroups& pg, int m, int q, std::vector<cdbl>& y) {
  y.assign((size_t)q * m, cdbl(0.0, 0.0));
  for (int k = 0; k < q; ++k)
    for (int j = 0; j < m; ++j) y[(size_t)k * m + j] = pair_t_at(ht, pg, q, k, j);
}

// complex y (q x m) as the real 2q x 2mc matrix of every group, [[re, im], [-im, re]] per entry: the real view of X_U
// (n x 2q) times group g's matrix is the real view of X_U y in that group's columns.  Columns at or behind m are zero.
inline void pair_embed(const std::vector<cdbl>& y, const PairGroups& pg, int m, int q, std::vector<double>& hm) {
  const int m2 = pg.m2();
  hm.assign((size_t)pg.ng * 2 * q * m2, 0.0);
  for (int k = 0; k < q; ++k)
    for (int j = 0; j < m; ++j) {
      const cdbl v = y[(size_t)k * m + j];
      double* g0 = hm.data() + (size_t)pg.group_of(j) * 2 * q * m2 + 2 * pg.col_of(j);
      g0[(size_t)(2 * k) * m2] = v.real();
      g0[(size_t)(2 * k) * m2 + 1] = v.imag();
      g0[(size_t)(2 * k + 1) * m2] = -v.imag();
      g0[(size_t)(2 * k + 1) * m2 + 1] = v.real();
    }
}

}  // namespace ricadi
