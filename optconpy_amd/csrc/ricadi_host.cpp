// ricadi_host.cpp -- host-side setup logic of libricadi_hip.so (no device code).
//
// Builds, once per operator and per level of the hierarchy, everything of the
// preconditioner that does not depend on the ADI shift (build_setup, a list of
// phases): the unified saddle-point sparsity pattern, the block-Jacobi
// partitions (greedy graph aggregation), the dense diagonal blocks of cal A and
// cal E, the aggregation coarse space chosen by the hierarchy rule and its
// Galerkin matrices -- dense, or sparse for a child level.  The per-shift parts
// are linear combinations formed on the device.
// Nothing here follows reference code: the reference solves these systems with
// SuperLU.
#include <array>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <stdexcept>

#include "ricadi_internal.h"

namespace ricadi {

HostCsr make_csr(int nrows, int ncols, const int32_t* rp, const int32_t* ci, const double* v) {
  HostCsr a;
  a.nrows = nrows;
  a.ncols = ncols;
  a.rp.assign(rp, rp + nrows + 1);
  const int nnz = rp[nrows];
  a.ci.assign(ci, ci + nnz);
  a.v.assign(v, v + nnz);
  sort_rows(a);
  return a;
}

void sort_rows(HostCsr& a) {
  std::vector<std::pair<int, double>> tmp;
  for (int i = 0; i < a.nrows; ++i) {
    const int b = a.rp[i], e = a.rp[i + 1];
    bool sorted = true;
    for (int k = b + 1; k < e; ++k)
      if (a.ci[k] < a.ci[k - 1]) { sorted = false; break; }
    if (sorted) continue;
    tmp.clear();
    for (int k = b; k < e; ++k) tmp.emplace_back(a.ci[k], a.v[k]);
    std::sort(tmp.begin(), tmp.end(),
              [](const std::pair<int, double>& x, const std::pair<int, double>& y) {
                return x.first < y.first;
              });
    for (int k = b; k < e; ++k) {
      a.ci[k] = tmp[k - b].first;
      a.v[k] = tmp[k - b].second;
    }
  }
}

// Counts the cnt keys key[k] in [0, nb) into ptr (ptr[b] .. ptr[b + 1] becomes the range of key b) and returns the
// start of every range: scattering entry k to pos[key[k]]++ in entry order is the counting sort, stable in the entry
// index, that the transposes and the row lists of a partition are.
static std::vector<int> bucket_starts(int nb, const int* key, size_t cnt, std::vector<int>& ptr) {
  ptr.assign(nb + 1, 0);
  for (size_t k = 0; k < cnt; ++k) ptr[key[k] + 1]++;
  for (int b = 0; b < nb; ++b) ptr[b + 1] += ptr[b];
  return std::vector<int>(ptr.begin(), ptr.end() - 1);
}

// t = a^T for CSR arrays of nrows rows and ncols columns (entries of a row of t in the order of a's rows)
static void transpose_arrays(int nrows, int ncols, const std::vector<int>& rp, const std::vector<int>& ci,
                             const std::vector<double>& v, std::vector<int>& t_rp, std::vector<int>& t_ci,
                             std::vector<double>& t_v) {
  std::vector<int> pos = bucket_starts(ncols, ci.data(), ci.size(), t_rp);
  t_ci.resize(ci.size());
  t_v.resize(ci.size());
  for (int i = 0; i < nrows; ++i)
    for (int k = rp[i]; k < rp[i + 1]; ++k) {
      const int d = pos[ci[k]]++;
      t_ci[d] = i;
      t_v[d] = v[k];
    }
}

HostCsr transpose(const HostCsr& a) {
  HostCsr t;
  t.nrows = a.ncols;
  t.ncols = a.nrows;
  transpose_arrays(a.nrows, a.ncols, a.rp, a.ci, a.v, t.rp, t.ci, t.v);
  return t;
}

// Greedy BFS aggregation: grow a block from each still-free seed until it holds
// bsize rows.  Deterministic (seeds in index order, neighbours in CSR order).
int aggregate(int n, const int* rp, const int* ci, int bsize, int* blk) {
  if (bsize < 1) bsize = 1;
  std::fill(blk, blk + n, -1);
  std::vector<int> members;
  members.reserve(bsize);
  int nb = 0;
  for (int seed = 0; seed < n; ++seed) {
    if (blk[seed] >= 0) continue;
    members.clear();
    members.push_back(seed);
    blk[seed] = nb;
    size_t head = 0;
    while (head < members.size() && (int)members.size() < bsize) {
      const int u = members[head++];
      for (int k = rp[u]; k < rp[u + 1] && (int)members.size() < bsize; ++k) {
        const int v = ci[k];
        if (v >= 0 && v < n && blk[v] < 0) {
          blk[v] = nb;
          members.push_back(v);
        }
      }
    }
    ++nb;
  }
  return nb;
}

static void lists_from_blocks(int n, const int* blk, int nb, std::vector<int>& ptr, std::vector<int>& rows) {
  std::vector<int> pos = bucket_starts(nb, blk, (size_t)n, ptr);
  rows.resize(n);
  for (int i = 0; i < n; ++i) rows[pos[blk[i]]++] = i;
}

// Rows of a sparse matrix accumulated through a marker array: the first touch of a column in the current row appends
// an entry (0.0 in each of the nval value arrays that share the pattern), so a row lists its columns in first-touch
// order; slot() returns the entry to add to.
struct RowAccumulator {
  std::vector<int> where;
  std::vector<int>& ci;
  std::vector<double>* val[3];
  int nval, r0 = 0;
  RowAccumulator(int ncols, std::vector<int>& ci_, std::vector<double>* v0, std::vector<double>* v1 = nullptr,
                 std::vector<double>* v2 = nullptr)
      : where(ncols, -1), ci(ci_), val{v0, v1, v2}, nval(v2 ? 3 : v1 ? 2 : 1) {}
  void begin_row() { r0 = (int)ci.size(); }
  int slot(int col) {
    int at = where[col];
    if (at < r0) {              // not seen in this row yet
      at = (int)ci.size();
      where[col] = at;
      ci.push_back(col);
      for (int q = 0; q < nval; ++q) val[q]->push_back(0.0);
    }
    return at;
  }
};

// Galerkin product R^T M C for aggregation maps: entry (i, j) of M goes to (rowmap[i], colmap[j]).
// rows_ptr / rows_list: the fine rows of every coarse row.
static HostCsr galerkin(const HostCsr& M, int nrow_c, const int* rows_ptr, const int* rows_list, int row_off,
                        const int* colmap, int ncol_c) {
  HostCsr out;
  out.nrows = nrow_c;
  out.ncols = ncol_c;
  out.rp.assign(1, 0);
  RowAccumulator acc(ncol_c, out.ci, &out.v);
  for (int a = 0; a < nrow_c; ++a) {
    acc.begin_row();
    for (int q = rows_ptr[a]; q < rows_ptr[a + 1]; ++q) {
      const int i = rows_list[q] - row_off;
      for (int k = M.rp[i]; k < M.rp[i + 1]; ++k) {
        const int at = acc.slot(colmap[M.ci[k]]);
        out.v[at] += M.v[k];
      }
    }
    out.rp.push_back((int)out.ci.size());
  }
  sort_rows(out);
  return out;
}

// Is smoothing the velocity aggregates with a Jacobi step on sym(A) appropriate for this operator?
//  - only for a stiffness-like A -- constants nearly in the kernel of its symmetric part: row sums small against
//    the diagonal (NSE operator 0.01-0.06, DRE operator at n = 3e4 0.03; a mass matrix 1.6).  Smoothing the
//    aggregates with a mass-like matrix makes the cycle WORSE (numpy mirror, [[M, J^T],[J, 0]]: 54 -> 122
//    iterations at omega = 0.5, no convergence at 0.67);
//  - and only while the symmetric part dominates: the smoother says nothing about a convection-dominated operator.
//    gamma = sum |skew part| / sum |off-diagonal symmetric part| (~ 1.2 x the cell Peclet number): measured
//    slowest-shift iterations with / without smoothing at gamma = 0.10: 73 / 100, 0.23: 59 / 67, 0.52: 82 / 106 and
//    93 / 106, but 1.07: 120 / 107, 2.0: 262 / 217 and 291 / 226.
// rs / gamma return the two ratios (gamma = -1 when the first test already failed).
bool sa_criterion(const HostCsr& A, double& rs_out, double& gamma_out) {
  const int nv = A.nrows;
  double srs = 0.0, sdg = 0.0;
  std::vector<double> colsum(nv, 0.0);
  for (int i = 0; i < nv; ++i)
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) colsum[A.ci[k]] += A.v[k];
  for (int i = 0; i < nv; ++i) {
    double rsum = 0.0, dg = 0.0;
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) {
      rsum += A.v[k];
      if (A.ci[k] == i) dg += A.v[k];
    }
    srs += std::fabs(0.5 * (rsum + colsum[i]));
    sdg += std::fabs(dg);
  }
  rs_out = sdg > 0.0 ? srs / sdg : -1.0;
  gamma_out = -1.0;
  if (!(sdg > 0.0) || srs > 0.15 * sdg) return false;
  const HostCsr At0 = transpose(A);
  std::vector<double> w1(nv, 0.0), w2(nv, 0.0);
  double sk = 0.0, sy = 0.0;
  for (int i = 0; i < nv; ++i) {
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) w1[A.ci[k]] += 0.5 * A.v[k];
    for (int k = At0.rp[i]; k < At0.rp[i + 1]; ++k) w2[At0.ci[k]] += 0.5 * At0.v[k];
    auto visit = [&](int j) {
      if (w1[j] == 0.0 && w2[j] == 0.0) return;
      sk += std::fabs(w1[j] - w2[j]);
      if (j != i) sy += std::fabs(w1[j] + w2[j]);
      w1[j] = w2[j] = 0.0;
    };
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) visit(A.ci[k]);
    for (int k = At0.rp[i]; k < At0.rp[i + 1]; ++k) visit(At0.ci[k]);
  }
  gamma_out = sy > 0.0 ? sk / sy : 1e30;
  return gamma_out <= 0.7;
}

int root_levels(const ricadi_opts& o) {
  // (a context that may use L levels has at most L - 1 grids: the dense coarse problem counts)
  return o.hierarchy == 1 ? RICADI_MAX_HIERARCHY_LEVELS + 1 : std::max(2, o.max_levels);
}
ricadi_opts child_opts(const ricadi_opts& o, bool parent_is_child) {
  ricadi_opts c = o;
  // aggregates of the child level (in units of ITS dofs = this level's aggregates): pairs of velocity aggregates,
  // single pressure aggregates; its own dense inverse may be an eighth larger than the cap (pairs do not always
  // pair up) -- once for the whole chain of a fine hierarchy
  c.agg_v = 2;
  c.agg_p = 1;
  if (!(o.hierarchy == 1 && parent_is_child)) c.coarse_max = o.coarse_max + o.coarse_max / 8;
  return c;
}
int child_levels(const ricadi_opts& o, int levels) { return o.hierarchy == 1 ? levels - 1 : 2; }

// ---- build_setup: one phase per job -------------------------------------------------------------------------------
// What the hierarchy rule decides for a level
struct Aggregates {
  std::vector<int> va, pa;   // aggregate of every velocity / pressure row
  int kv = 0, kp = 0;        // how many there are
  int av = 0, ap = 0;        // the aggregate sizes the rule ended with
  bool multilevel = false;   // the coarse problem goes to a child level
};
// What more than one phase reads and no caller sees (the pressure blocks' map is read by its own phase only)
struct SetupWork {
  std::vector<int> vv_rp, vv_ci;   // velocity-velocity pattern (union of A and E), for the graph work
  std::vector<int> pp_rp, pp_ci;   // pressure graph: pattern of J J^T
  std::vector<int> blk, local;     // block-Jacobi block of a velocity row and the row's position in it
};

// Owns s_rp, s_ci, s_srcA, s_srcE, s_srcJ, dA, dE (and w.vv_*): the unified saddle pattern with its three value sources.
// dA / dE take the LAST stored entry (i, i) of a row; the smoothed prolongation SUMS the entries (i, i) of A (its dg).
// The two differ only for a CSR with duplicate columns, which make_csr sorts but does not merge.
static void saddle_pattern(const HostCsr& A, const HostCsr& E, const HostCsr& J, const HostCsr& JT, HostSetup& hs,
                           SetupWork& w) {
  const int nv = hs.nv, np = hs.np;
  hs.s_rp.assign(hs.n + 1, 0);
  hs.dA.assign(nv, 0.0);
  hs.dE.assign(nv, 0.0);
  w.vv_rp.assign(nv + 1, 0);
  for (int i = 0; i < nv; ++i) {
    int a = A.rp[i], ae = A.rp[i + 1], e = E.rp[i], ee = E.rp[i + 1];
    while (a < ae || e < ee) {
      const int ca = a < ae ? A.ci[a] : INT32_MAX;
      const int ce = e < ee ? E.ci[e] : INT32_MAX;
      const int c = std::min(ca, ce);
      double va = 0.0, ve = 0.0;
      if (ca == c) va = A.v[a++];
      if (ce == c) ve = E.v[e++];
      hs.s_ci.push_back(c);
      hs.s_srcA.push_back(va);
      hs.s_srcE.push_back(ve);
      hs.s_srcJ.push_back(0.0);
      w.vv_ci.push_back(c);
      if (c == i) {
        hs.dA[i] = va;
        hs.dE[i] = ve;
      }
    }
    w.vv_rp[i + 1] = (int)w.vv_ci.size();
    for (int k = JT.rp[i]; k < JT.rp[i + 1]; ++k) {
      hs.s_ci.push_back(nv + JT.ci[k]);
      hs.s_srcA.push_back(0.0);
      hs.s_srcE.push_back(0.0);
      hs.s_srcJ.push_back(JT.v[k]);
    }
    hs.s_rp[i + 1] = (int)hs.s_ci.size();
  }
  for (int k = 0; k < np; ++k) {
    for (int q = J.rp[k]; q < J.rp[k + 1]; ++q) {
      hs.s_ci.push_back(J.ci[q]);
      hs.s_srcA.push_back(0.0);
      hs.s_srcE.push_back(0.0);
      hs.s_srcJ.push_back(J.v[q]);
    }
    hs.s_rp[nv + k + 1] = (int)hs.s_ci.size();
  }
}

// Owns bs, nbv, bv_ptr, bv_rows, bv_A, bv_E (and w.blk, w.local): the block-Jacobi partition of the velocity block
static void velocity_blocks(const HostCsr& A, const HostCsr& E, const ricadi_opts& o, HostSetup& hs, SetupWork& w) {
  const int nv = hs.nv;
  const int bs = (o.bj_block <= 16) ? 16 : (o.bj_block <= 32 ? 32 : 64);
  hs.bs = bs;
  w.blk.resize(nv);
  hs.nbv = aggregate(nv, w.vv_rp.data(), w.vv_ci.data(), bs, w.blk.data());
  lists_from_blocks(nv, w.blk.data(), hs.nbv, hs.bv_ptr, hs.bv_rows);
  w.local.resize(nv);
  for (int b = 0; b < hs.nbv; ++b)
    for (int k = hs.bv_ptr[b]; k < hs.bv_ptr[b + 1]; ++k) w.local[hs.bv_rows[k]] = k - hs.bv_ptr[b];
  hs.bv_A.assign((size_t)hs.nbv * bs * bs, 0.0);
  hs.bv_E.assign((size_t)hs.nbv * bs * bs, 0.0);
  for (int i = 0; i < nv; ++i) {
    const int b = w.blk[i];
    double* Ba = hs.bv_A.data() + (size_t)b * bs * bs + (size_t)w.local[i] * bs;
    double* Be = hs.bv_E.data() + (size_t)b * bs * bs + (size_t)w.local[i] * bs;
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k)
      if (w.blk[A.ci[k]] == b) Ba[w.local[A.ci[k]]] += A.v[k];
    for (int k = E.rp[i]; k < E.rp[i + 1]; ++k)
      if (w.blk[E.ci[k]] == b) Be[w.local[E.ci[k]]] += E.v[k];
  }
}

// Owns nbp, bp_ptr, bp_rows (and w.pp_*): the pressure graph (pattern of J J^T) and its block partition
static void pressure_blocks(const HostCsr& J, const HostCsr& JT, HostSetup& hs, SetupWork& w) {
  const int np = hs.np;
  w.pp_rp.assign(np + 1, 0);
  std::vector<int> mark(np, -1);
  for (int k = 0; k < np; ++k) {
    for (int q = J.rp[k]; q < J.rp[k + 1]; ++q) {
      const int j = J.ci[q];
      for (int t = JT.rp[j]; t < JT.rp[j + 1]; ++t) {
        const int k2 = JT.ci[t];
        if (mark[k2] != k) {
          mark[k2] = k;
          w.pp_ci.push_back(k2);
        }
      }
    }
    std::sort(w.pp_ci.begin() + w.pp_rp[k], w.pp_ci.end());
    w.pp_rp[k + 1] = (int)w.pp_ci.size();
  }
  std::vector<int> pblk(std::max(np, 1));
  hs.nbp = np > 0 ? aggregate(np, w.pp_rp.data(), w.pp_ci.data(), hs.bs, pblk.data()) : 0;
  lists_from_blocks(np, pblk.data(), hs.nbp, hs.bp_ptr, hs.bp_rows);
}

// Owns jd_ptr, jd_vblk, jd_val: the dense J sub-blocks of the consistent SIMPLE Schur complement.
// S_bb = sum_beta J_{b,beta} Ahat_beta^-1 J_{b,beta}^T needs, per pressure block b,
// the bs x bs slices of J against every velocity block beta it touches.  J does
// not depend on the shift, so the slices are extracted once.
static void schur_j_blocks(const HostCsr& J, HostSetup& hs, const SetupWork& w) {
  const int bs = hs.bs;
  hs.jd_ptr.assign(1, 0);
  std::vector<int> slot(std::max(hs.nbv, 1), -1), touched;
  for (int b = 0; b < hs.nbp; ++b) {
    touched.clear();
    const size_t base = hs.jd_vblk.size();
    for (int q = hs.bp_ptr[b]; q < hs.bp_ptr[b + 1]; ++q) {
      const int k = hs.bp_rows[q], il = q - hs.bp_ptr[b];
      for (int e = J.rp[k]; e < J.rp[k + 1]; ++e) {
        const int j = J.ci[e], vb = w.blk[j];
        if (slot[vb] < 0) {
          slot[vb] = (int)touched.size();
          touched.push_back(vb);
          hs.jd_vblk.push_back(vb);
          hs.jd_val.resize(hs.jd_val.size() + (size_t)bs * bs, 0.0);
        }
        hs.jd_val[(base + slot[vb]) * (size_t)bs * bs + (size_t)il * bs + w.local[j]] += J.v[e];
      }
    }
    for (int vb : touched) slot[vb] = -1;
    hs.jd_ptr.push_back((int)hs.jd_vblk.size());
  }
}

// Owns sb_*: the row blocks and the tile format of the LDS-tiled SpMM.
// Rows are visited aggregate by aggregate (compact mesh patches) and packed
// greedily into blocks of <= kSbMaxRows rows whose set of distinct columns stays
// within kSbMaxCols, so that the x tile of a block fits the LDS budget.
constexpr int kSbMaxRows = 32, kSbMaxCols = 152;   // 152 x 16 x 8 B tiles: 8 workgroups per CU fit the 160 KB LDS
static void saddle_tiles(HostSetup& hs) {
  const int nv = hs.nv, np = hs.np, n = hs.n;
  std::vector<int> order;
  order.reserve(n);
  for (int q = 0; q < nv; ++q) order.push_back(hs.bv_rows[q]);
  for (int q = 0; q < np; ++q) order.push_back(nv + hs.bp_rows[q]);
  hs.sb_rowptr.assign(1, 0);
  hs.sb_rp.assign(1, 0);
  hs.sb_cptr.assign(1, 0);
  std::vector<int> stamp(n, -1), pos(n, -1), cols, brows;
  int bid = 0;
  size_t at = 0;
  while (at < order.size()) {
    cols.clear();
    brows.clear();
    // a velocity block never continues into the pressure rows
    const bool vel = order[at] < nv;
    while (at < order.size() && (int)brows.size() < kSbMaxRows && (order[at] < nv) == vel) {
      const int row = order[at];
      int fresh = 0;
      for (int k = hs.s_rp[row]; k < hs.s_rp[row + 1]; ++k)
        if (stamp[hs.s_ci[k]] != bid) ++fresh;
      if (!brows.empty() && (int)cols.size() + fresh > kSbMaxCols) break;
      for (int k = hs.s_rp[row]; k < hs.s_rp[row + 1]; ++k) {
        const int c = hs.s_ci[k];
        if (stamp[c] != bid) {
          stamp[c] = bid;
          cols.push_back(c);
        }
      }
      brows.push_back(row);
      ++at;
    }
    std::sort(cols.begin(), cols.end());
    for (size_t j = 0; j < cols.size(); ++j) pos[cols[j]] = (int)j;
    // Rows of similar length next to each other: a wave of the kernel steps through the 16-entry chunks of FOUR
    // consecutive local rows together (DPP broadcasts need all lanes), i.e. through the LONGEST of the four;
    // sorted by (half-)chunk count the four rows of a wave-pass need the same number of steps almost everywhere
    // (P2 vertex / edge-midpoint rows differ by a factor two in their entry counts).
    std::stable_sort(brows.begin(), brows.end(), [&](int a, int b) {
      return (hs.s_rp[a + 1] - hs.s_rp[a] + 7) / 8 > (hs.s_rp[b + 1] - hs.s_rp[b] + 7) / 8;   // half chunks
    });
    const size_t nnz0 = hs.sb_perm.size();
    // Entry order within a row: the kernel's 32-lane halves pair the local rows (2j, 2j+1), and
    // their two ds_read_b64 of a step (16 columns = 128 B each) are conflict free iff the two tile
    // rows have opposite parity (LDS bank = (byte / 4) mod 64).  Even local rows therefore list
    // their even tile rows first, odd local rows their odd ones: the parities differ wherever both
    // rows are in their first or both in their second part.
    int ql = 0;
    for (int row : brows) {
      for (int pass = 0; pass < 2; ++pass)
        for (int k = hs.s_rp[row]; k < hs.s_rp[row + 1]; ++k) {
          const int l = pos[hs.s_ci[k]];
          const bool first = (l & 1) == (ql & 1);
          if (first != (pass == 0)) continue;
          hs.sb_perm.push_back(k);
          hs.sb_lidx.push_back((uint16_t)l);
        }
      hs.sb_rows.push_back(row);
      hs.sb_rp.push_back((int)hs.sb_perm.size());
      ++ql;
    }
    for (int c : cols) hs.sb_cols.push_back(c);
    hs.sb_cptr.push_back((int)hs.sb_cols.size());
    hs.sb_rowptr.push_back((int)hs.sb_rows.size());
    hs.sb_max_cols = std::max(hs.sb_max_cols, (int)cols.size());
    hs.sb_max_nnz = std::max(hs.sb_max_nnz, (int)(hs.sb_perm.size() - nnz0));
    ++bid;
  }
  hs.sb_nblk = bid;
}

// The hierarchy rule: the aggregates of this level and whether its coarse problem goes to a child level.  stiff: the
// operator is one the smoothed prolongation is made for (sa_criterion).  Writes no HostSetup field.
static Aggregates hierarchy_rule(const HostCsr& E, const ricadi_opts& o, int bs, int nv, int np, const SetupWork& w,
                                 int max_levels, bool stiff) {
  // graph for velocity aggregates: pattern of cal E if it is a genuine
  // (mass-like) matrix -- keeps the components apart -- else the union pattern
  const bool e_graph = E.nnz() > (size_t)(2 * nv);
  // Without a mass-like cal E (lau.solve_sadpnt_smw hands over ONE matrix) the aggregates follow the union
  // pattern and mix the velocity components; a child level built on those stagnates (measured at n = 1e5:
  // relres 0.9 after 3000 iterations, two levels: 169) -- stay with two levels then.
  if (!e_graph) max_levels = 2;
  const int* g_rp = e_graph ? E.rp.data() : w.vv_rp.data();
  const int* g_ci = e_graph ? E.ci.data() : w.vv_ci.data();
  int av = std::max(1, o.agg_v), ap = std::max(1, o.agg_p);
  const bool fine = o.hierarchy == 1;
  Aggregates g;
  g.va.resize(nv);
  g.pa.resize(std::max(np, 1));
  int kv = 0, kp = 0;
  for (int attempt = 0; attempt < 16; ++attempt) {
    // The coarse pressure aggregates must not coincide with the Schur
    // block-Jacobi blocks (same graph, same greedy rule, same size): with
    // identical partitions the multiplicative two-level cycle stagnates
    // (measured: N=40, ap == bs == 32 stalls at 1e-2, ap in {16,24,48,64}
    // converges in 137-182 iterations).
    if (ap == bs) ap = ap + ap / 2;
    kv = aggregate(nv, g_rp, g_ci, av, g.va.data());
    kp = np > 0 ? aggregate(np, w.pp_rp.data(), w.pp_ci.data(), ap, g.pa.data()) : 0;
    // Dense inverse of this level's coarse matrix whenever it fits coarse_max.  (Rounds 2-3 handed the coarse problem
    // to a child level from HALF of coarse_max on -- the per-shift inversion grows with k^3 and the child's matrix is
    // half as large -- tuned on the one-solve-per-shift cycle: cfg3, k 3 046 -> 1 658, 72 -> 79 iterations, 188 -> 160 ms
    // per 32-shift cycle.  The workload the library exists for solves every shift many times per setup: the cfg3
    // Newton step -- 200 ADI steps over 32 shifts -- takes 955 ms with the dense inverse against 1 003 ms with the
    // child level (round 4, same-call A/B), so the dense inverse wins wherever it fits.)
    // For a stiffness-dominated operator the child level is a poor stand-in at the small shifts (measured at n = 2e5,
    // nu = 0.05, shift 1, same aggregates (36, 54), k = 5 415: child 229 iterations, dense inverse 175, dense inverse
    // with the smoothed prolongation 118 -- and the smoothed coarse operator handed to a child: 150 at these aggregates
    // but 572 against 214 at (81, 121), so smoothing stays a two-level affair).  Such operators keep two levels up to
    // 1.5 x coarse_max and grow their aggregates up to (121, 182) for it: n = 5e5, (81, 121), k = 5 969: 181 -> 132
    // iterations per shift-solve, 9.99 -> 8.86 s per pass over 128 shifts with the per-shift inversions inside.  A
    // convection-dominated or mass-like operator (criterion false) is served as well by the child as by the inverse
    // (n = 1e5, nu = 0.0025: 182 vs 153 iterations at shift 1, equal from shift 50 on, 219 vs 381 ms per 16 shifts).
    // A chain of pairwise velocity coarsening over single pressure aggregates runs out of velocity unknowns: from the
    // fourth child on k_v falls below k_p and the coarse saddle matrix [[K, B^T], [B, 0]] is singular (B: k_p x k_v
    // cannot have full row rank; met at n = 5e5, "coarse matrix singular").  A level of the fine hierarchy therefore
    // coarsens its pressure further until its velocity aggregates outnumber the pressure aggregates by a quarter.
    if (fine && np > 0 && 4L * kv < 5L * kp && ap < np) {
      ap += std::max(1, ap / 2);
      continue;
    }
    // The default hierarchy needs k_p <= k_v for the same reason (a tiny operator, or pressure rows with disjoint
    // supports: few velocity aggregates under many pressure components).  No operator whose coarse matrix could be
    // inverted so far has k_p > k_v, so this changes no structure that worked.
    if (!fine && np > 0 && kp > kv && ap < np) {
      ap += std::max(1, ap / 2);
      continue;
    }
    const int direct_max = std::max(16, stiff && !fine ? o.coarse_max + o.coarse_max / 2 : o.coarse_max);
    if (kv + kp <= direct_max) break;
    if (fine) {
      // The fine hierarchy (ricadi_opts::hierarchy = 1): the aggregates stay as they are and the coarse problem goes
      // to a child, level after level, whatever the operator (the mirror's count hardly moves with the mesh at fine
      // aggregates).  Only a level that can have no child -- the last one the chain allows, or
      // an operator without pressure or without a mass-like cal E -- grows its aggregates until its inverse fits (by
      // 1.5 and at least one: a child starts from (2, 1)).
      if (max_levels > 2 && np > 0) {
        g.multilevel = true;
        break;
      }
      av += std::max(1, av / 2);
      ap += std::max(1, ap / 2);
      continue;
    }
    const bool grow_first = stiff && av + av / 2 <= 128;
    // A third level, only where it can be GENTLE: the coarse problem of these aggregates goes to a
    // child level whose own aggregates are pairs of velocity aggregates and single pressure aggregates
    // (so that the child's two-level cycle is a near-exact solve).  Coarsening the child harder makes
    // its cycle -- one multiplicative coarse correction + one SIMPLE sweep, not a contraction -- too
    // poor a stand-in for the coarse solve: GMRES stagnates (measured at n = 5e5 with every tried
    // pair of level-2 aggregate sizes).  Larger problems therefore still grow the
    // aggregates of THIS level, but only until the gentle child fits (in steps of 1.5, not 2).
    if (max_levels > 2 && np > 0 && !grow_first && 0.55 * kv + kp <= std::max(16, o.coarse_max)) {
      g.multilevel = true;
      break;
    }
    if (max_levels > 2 && np > 0) {
      av += av / 2;
      ap += ap / 2;
      continue;
    }
    av *= 2;
    ap *= 2;
  }
  // Pressure aggregates never join components of the graph of J J^T: where more components than velocity aggregates
  // are left, no aggregate size gives a regular coarse matrix, and the level goes without a coarse space (kv = kp = 0).
  if (np > 0 && kp > kv) {
    kv = kp = 0;
    g.multilevel = false;
  }
  g.kv = kv;
  g.kp = kp;
  g.av = av;
  g.ap = ap;
  return g;
}

// Owns kc, kcv, kcp, agg_v, agg_p, multilevel, aggof, agg_ptr, agg_rows: the coarse space the rule chose
static void coarse_space(const Aggregates& g, HostSetup& hs) {
  hs.kcv = g.kv;
  hs.kcp = g.kp;
  hs.kc = g.kv + g.kp;
  hs.agg_v = g.av;
  hs.agg_p = g.ap;
  hs.multilevel = g.multilevel;
  hs.aggof.resize(hs.n);
  for (int i = 0; i < hs.nv; ++i) hs.aggof[i] = g.va[i];
  for (int k = 0; k < hs.np; ++k) hs.aggof[hs.nv + k] = g.kv + g.pa[k];
  lists_from_blocks(hs.n, hs.aggof.data(), hs.kc, hs.agg_ptr, hs.agg_rows);
}

// rho(D^-1 K0), K0 = (A + A^T) / 2, D = dg: 20 steps of the power iteration from a fixed pseudo-random start
static double jacobi_radius(const HostCsr& A, const HostCsr& At, const std::vector<double>& dg) {
  const int nv = A.nrows;
  std::vector<double> x(nv), y(nv);
  unsigned sd = 12345u;
  for (int i = 0; i < nv; ++i) {
    sd = sd * 1664525u + 1013904223u;
    x[i] = (double)(sd >> 8) / 16777216.0 - 0.5;
  }
  double rho = 0.0;
  for (int it = 0; it < 20; ++it) {
    double nx = 0.0, ny = 0.0;
    for (int i = 0; i < nv; ++i) {
      double t = 0.0;
      for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) t += A.v[k] * x[A.ci[k]];
      for (int k = At.rp[i]; k < At.rp[i + 1]; ++k) t += At.v[k] * x[At.ci[k]];
      y[i] = dg[i] != 0.0 ? 0.5 * t / dg[i] : 0.0;
      nx += x[i] * x[i];
      ny += y[i] * y[i];
    }
    rho = nx > 0.0 ? std::sqrt(ny / nx) : 0.0;
    const double sc = ny > 0.0 ? 1.0 / std::sqrt(ny) : 0.0;
    for (int i = 0; i < nv; ++i) x[i] = y[i] * sc;
  }
  return rho;
}

// Owns sa, p_*, pd_*, pt_*: the prolongation P by rows -- plain aggregation (sa = false, arrays empty), or smoothed on
// the velocity rows -- with P - Y and P^T.  sa_rs / sa_gamma: the ratios of sa_criterion, for the verbose line.
static void smoothed_prolongation(const HostCsr& A, const ricadi_opts& o, double sa_omega, bool stiff, double sa_rs,
                                  double sa_gamma, HostSetup& hs, const Aggregates& g) {
  const int nv = hs.nv, np = hs.np, kv = g.kv;
  hs.sa = sa_omega > 0.0 && !hs.multilevel && np > 0 && kv > 0;
  if (hs.sa) {
    hs.sa = stiff;
    if (o.verbose)
      fprintf(stderr, "[ricadi] smoothed aggregation %s: row sums / diagonal of sym(cal A) = %.3f, skew / symmetric "
              "off-diagonal mass %.3f\n", hs.sa ? "on" : "off", sa_rs, sa_gamma);
  }
  if (!hs.sa) return;
  const HostCsr At = transpose(A);
  std::vector<double> dg(nv, 0.0);   // the SUM of the stored entries (i, i) of a row: D of the smoother and of rho
  for (int i = 0; i < nv; ++i)
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k)
      if (A.ci[k] == i) dg[i] += A.v[k];
  // damping relative to the spectral radius of D^-1 K0 (power iteration): the prolongation smoother
  // I - omega D^-1 K0 must not amplify -- a mass-like cal A (lau.app_prj_via_sadpnt hands the mass matrix over
  // as the operator) has rho ~ 4 for P2 elements, and omega = 0.67 made GMRES fail there
  const double rho = jacobi_radius(A, At, dg);
  if (rho > 2.0) sa_omega *= 2.0 / rho;
  if (o.verbose) fprintf(stderr, "[ricadi] smoothed aggregation: rho(D^-1 K0) ~ %.2f, omega %.3f\n", rho, sa_omega);
  hs.p_rp.assign(1, 0);
  hs.pd_rp.assign(1, 0);
  RowAccumulator acc(hs.kc, hs.p_ci, &hs.p_v);
  for (int i = 0; i < nv; ++i) {
    acc.begin_row();
    auto add = [&](int a, double w) {
      const int at = acc.slot(a);
      hs.p_v[at] += w;
    };
    add(g.va[i], 1.0);
    const double d = dg[i];
    if (d != 0.0) {
      const double sc = -0.5 * sa_omega / d;         // K0 = (A + A^T) / 2
      for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) add(g.va[A.ci[k]], sc * A.v[k]);
      for (int k = At.rp[i]; k < At.rp[i + 1]; ++k) add(g.va[At.ci[k]], sc * At.v[k]);
    }
    hs.p_rp.push_back((int)hs.p_ci.size());
    for (int k = acc.r0; k < (int)hs.p_ci.size(); ++k) {
      hs.pd_ci.push_back(hs.p_ci[k]);
      hs.pd_v.push_back(hs.p_v[k] - (hs.p_ci[k] == g.va[i] ? 1.0 : 0.0));
    }
    hs.pd_rp.push_back((int)hs.pd_ci.size());
  }
  for (int k = 0; k < np; ++k) {
    hs.p_ci.push_back(kv + g.pa[k]);
    hs.p_v.push_back(1.0);
    hs.p_rp.push_back((int)hs.p_ci.size());
  }
  transpose_arrays(hs.n, hs.kc, hs.p_rp, hs.p_ci, hs.p_v, hs.pt_rp, hs.pt_ci, hs.pt_v);
}

// the entries of row j of P (plain aggregation: the single (aggof[j], 1))
static int prolongation_row(const HostSetup& hs, int j, const int*& ci, const double*& v) {
  static const double one = 1.0;
  if (hs.sa) {
    ci = hs.p_ci.data() + hs.p_rp[j];
    v = hs.p_v.data() + hs.p_rp[j];
    return hs.p_rp[j + 1] - hs.p_rp[j];
  }
  ci = hs.aggof.data() + j;
  v = &one;
  return 1;
}

// Owns l1A, l1E, l1J (a level with a child: its Galerkin matrices) or E0, EM, EJ (dense P^T A P, P^T E P and the
// coarse J with its transpose)
static void coarse_matrices(const HostCsr& A, const HostCsr& E, const HostCsr& J, HostSetup& hs, const Aggregates& g) {
  const int nv = hs.nv, np = hs.np, kv = g.kv, kp = g.kp, kc = hs.kc;
  if (hs.multilevel) {
    hs.l1A = galerkin(A, kv, hs.agg_ptr.data(), hs.agg_rows.data(), 0, g.va.data(), kv);
    hs.l1E = galerkin(E, kv, hs.agg_ptr.data(), hs.agg_rows.data(), 0, g.va.data(), kv);
    hs.l1J = galerkin(J, kp, hs.agg_ptr.data() + kv, hs.agg_rows.data(), nv, g.va.data(), kv);
    return;
  }
  hs.E0.assign((size_t)kc * kc, 0.0);
  hs.EM.assign((size_t)kc * kc, 0.0);
  hs.EJ.assign((size_t)kc * kc, 0.0);
  for (int i = 0; i < nv; ++i) {
    const int *ri, *cj;
    const double *rw, *cw;
    const int nri = prolongation_row(hs, i, ri, rw);
    for (int k = A.rp[i]; k < A.rp[i + 1]; ++k) {
      const int ncj = prolongation_row(hs, A.ci[k], cj, cw);
      for (int a = 0; a < nri; ++a)
        for (int b = 0; b < ncj; ++b) hs.E0[(size_t)ri[a] * kc + cj[b]] += rw[a] * A.v[k] * cw[b];
    }
    for (int k = E.rp[i]; k < E.rp[i + 1]; ++k) {
      const int ncj = prolongation_row(hs, E.ci[k], cj, cw);
      for (int a = 0; a < nri; ++a)
        for (int b = 0; b < ncj; ++b) hs.EM[(size_t)ri[a] * kc + cj[b]] += rw[a] * E.v[k] * cw[b];
    }
  }
  for (int k = 0; k < np; ++k)
    for (int q = J.rp[k]; q < J.rp[k + 1]; ++q) {
      const int cp = kv + g.pa[k];
      const int* cj;
      const double* cw;
      const int ncj = prolongation_row(hs, J.ci[q], cj, cw);
      for (int b = 0; b < ncj; ++b) {
        hs.EJ[(size_t)cp * kc + cj[b]] += J.v[q] * cw[b];
        hs.EJ[(size_t)cj[b] * kc + cp] += J.v[q] * cw[b];
      }
    }
}

// Owns sy_rp, sy_ci, sy_A, sy_E, sy_J: the prolongated operator S*Y (n x kc, sparse).
// Row i of the unified saddle pattern with its columns mapped to their aggregates and
// duplicates merged (a row touches ~6 aggregates instead of ~28 columns).  The
// residual after the coarse correction, r - S (Y e), is then one short-row CSR SpMM
// over the L2-resident coarse vector instead of a full saddle SpMM.
static void prolongated_operator(HostSetup& hs) {
  hs.sy_rp.assign(1, 0);
  RowAccumulator acc(hs.kc, hs.sy_ci, &hs.sy_A, &hs.sy_E, &hs.sy_J);
  for (int i = 0; i < hs.n; ++i) {
    acc.begin_row();
    for (int k = hs.s_rp[i]; k < hs.s_rp[i + 1]; ++k) {
      const int* cj;
      const double* cw;
      const int ncj = prolongation_row(hs, hs.s_ci[k], cj, cw);
      for (int b = 0; b < ncj; ++b) {
        const int at = acc.slot(cj[b]);
        hs.sy_A[at] += hs.s_srcA[k] * cw[b];
        hs.sy_E[at] += hs.s_srcE[k] * cw[b];
        hs.sy_J[at] += hs.s_srcJ[k] * cw[b];
      }
    }
    hs.sy_rp.push_back((int)hs.sy_ci.size());
  }
}

// Owns syb_*: S*Y in the tile format of the LDS-tiled SpMM, on the SAME row blocks as S: per block
// the distinct aggregates its rows touch (the LDS tile of coarse-vector rows) and per
// entry the 16-bit tile row; values are gathered through sy_perm.
static void prolongated_tiles(HostSetup& hs) {
  hs.syb_rp.assign(1, 0);
  hs.syb_cptr.assign(1, 0);
  std::vector<int> pos(hs.kc, -1), cols;
  for (int b = 0; b < hs.sb_nblk; ++b) {
    cols.clear();
    for (int q = hs.sb_rowptr[b]; q < hs.sb_rowptr[b + 1]; ++q) {
      const int row = hs.sb_rows[q];
      for (int k = hs.sy_rp[row]; k < hs.sy_rp[row + 1]; ++k)
        if (pos[hs.sy_ci[k]] < 0) {
          pos[hs.sy_ci[k]] = 0;
          cols.push_back(hs.sy_ci[k]);
        }
    }
    std::sort(cols.begin(), cols.end());
    for (size_t j = 0; j < cols.size(); ++j) pos[cols[j]] = (int)j;
    for (int q = hs.sb_rowptr[b]; q < hs.sb_rowptr[b + 1]; ++q) {
      const int row = hs.sb_rows[q];
      for (int k = hs.sy_rp[row]; k < hs.sy_rp[row + 1]; ++k) {
        hs.syb_perm.push_back(k);
        hs.syb_lidx.push_back((uint16_t)pos[hs.sy_ci[k]]);
      }
      hs.syb_rp.push_back((int)hs.syb_perm.size());
    }
    for (int c : cols) {
      hs.syb_cols.push_back(c);
      pos[c] = -1;
    }
    hs.syb_cptr.push_back((int)hs.syb_cols.size());
    hs.syb_max_cols = std::max(hs.syb_max_cols, (int)cols.size());
  }
}

HostSetup build_setup(const HostCsr& A, const HostCsr& E, const HostCsr& J, const HostCsr& JT, const ricadi_opts& o,
                      int max_levels, double sa_omega) {
  HostSetup hs;
  SetupWork w;
  hs.nv = A.nrows;
  hs.np = J.nrows;
  hs.n = hs.nv + hs.np;
  saddle_pattern(A, E, J, JT, hs, w);
  velocity_blocks(A, E, o, hs, w);
  pressure_blocks(J, JT, hs, w);
  schur_j_blocks(J, hs, w);
  saddle_tiles(hs);
  if (!o.use_coarse) {   // no coarse space: kc = 0, one empty aggregate list
    hs.agg_ptr.assign(1, 0);
    hs.aggof.assign(hs.n, 0);
    return hs;
  }
  // Is this an operator the smoothed prolongation is made for (stiffness-like, symmetric part dominant)?
  double sa_rs = -1.0, sa_gamma = -1.0;
  const bool stiff = sa_omega > 0.0 && hs.np > 0 && sa_criterion(A, sa_rs, sa_gamma);
  const Aggregates g = hierarchy_rule(E, o, hs.bs, hs.nv, hs.np, w, max_levels, stiff);
  if (g.kv + g.kp == 0) {   // the rule found no regular coarse space: as without use_coarse
    hs.agg_ptr.assign(1, 0);
    hs.aggof.assign(hs.n, 0);
    return hs;
  }
  coarse_space(g, hs);
  smoothed_prolongation(A, o, sa_omega, stiff, sa_rs, sa_gamma, hs, g);
  coarse_matrices(A, E, J, hs, g);
  prolongated_operator(hs);
  prolongated_tiles(hs);
  return hs;
}

// Cauchy data of one shift-parallel ADI sweep:
//   C_ij = -1/(p_i + p_j)  (s.p.d. for distinct negative real shifts),
//   C = R^T R;  rinv = R^-1 (upper, row-major);  cinv1 = C^-1 * ones.
// Owner rank of every shift of the list (see ricadi_host_deal in include/ricadi.h).
int deal_shifts(const double* shifts, int ns, int world, int32_t* owner) {
  double lmin = 1e300, lmax = -1e300;
  for (int i = 0; i < ns; ++i) {
    if (!(shifts[i] < 0.0)) return RICADI_EINVAL;
    const double l = std::log(-shifts[i]);
    lmin = std::min(lmin, l);
    lmax = std::max(lmax, l);
  }
  // predicted GMRES iterations (relative): slowest at the smallest |p| (cfg2: ~110 at p = -1,
  // ~30-45 over the upper half of a 1 ... 3e3 list)
  std::vector<double> it(ns);
  for (int i = 0; i < ns; ++i) {
    const double t = lmax > lmin ? (std::log(-shifts[i]) - lmin) / (lmax - lmin) : 1.0;
    it[i] = 1.0 + 2.5 * (1.0 - t) * (1.0 - t);
  }
  std::vector<int> order(ns);
  for (int i = 0; i < ns; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return it[a] > it[b]; });
  const double a = 3.2, b = 1.0;   // latency floor : per-group slope of a lockstep iteration
  std::vector<double> mx(world, 0.0), sm(world, 0.0);
  std::vector<int> cnt(world, 0);
  const int cap = (ns + world - 1) / world + 1;   // keeps the per-rank batch (and the exchange slots) small
  for (int k = 0; k < ns; ++k) {
    const int i = order[k];
    int best = -1;
    double bt = 0.0;
    for (int r = 0; r < world; ++r) {
      if (cnt[r] >= cap) continue;
      const double t = a * std::max(mx[r], it[i]) + b * (sm[r] + it[i]);
      if (best < 0 || t < bt - 1e-12) {
        best = r;
        bt = t;
      }
    }
    owner[i] = best;
    mx[best] = std::max(mx[best], it[i]);
    sm[best] += it[i];
    ++cnt[best];
  }
  return RICADI_OK;
}

// Least squares through the normal equations with a rank-revealing (diagonally pivoted)
// Cholesky factorisation:  Y = argmin || b - B Y ||_F  given  Ghh = B^T B (h x h) and
// Ghb = B^T b (h x m), both row-major.  Columns of B whose pivot falls below rtol * the largest
// diagonal entry are left out (their rows of Y are zero).  Returns the rank used.
int gram_lstsq(int h, int m, const double* Ghh, const double* Ghb, double rtol, double* Y) {
  std::vector<double> L((size_t)h * h, 0.0), d(h);
  std::vector<int> piv(h);
  double dmax = 0.0;
  for (int i = 0; i < h; ++i) {
    d[i] = Ghh[(size_t)i * h + i];
    piv[i] = i;
    dmax = std::max(dmax, d[i]);
  }
  for (size_t i = 0; i < (size_t)h * m; ++i) Y[i] = 0.0;
  if (!(dmax > 0.0)) return 0;
  int r = 0;
  for (; r < h; ++r) {
    int best = r;
    for (int i = r + 1; i < h; ++i)
      if (d[piv[i]] > d[piv[best]]) best = i;
    if (!(d[piv[best]] > rtol * dmax)) break;
    std::swap(piv[r], piv[best]);
    const int pr = piv[r];
    const double lrr = std::sqrt(d[pr]);
    L[(size_t)pr * h + r] = lrr;
    for (int i = r + 1; i < h; ++i) {
      const int pi = piv[i];
      double sum = Ghh[(size_t)pi * h + pr];
      for (int k = 0; k < r; ++k) sum -= L[(size_t)pi * h + k] * L[(size_t)pr * h + k];
      const double l = sum / lrr;
      L[(size_t)pi * h + r] = l;
      d[pi] -= l * l;
    }
  }
  // L (rows piv[0..r), r columns) L^T Y_P = Ghb_P
  std::vector<double> t((size_t)r);
  for (int c = 0; c < m; ++c) {
    for (int i = 0; i < r; ++i) {
      double sum = Ghb[(size_t)piv[i] * m + c];
      for (int k = 0; k < i; ++k) sum -= L[(size_t)piv[i] * h + k] * t[k];
      t[i] = sum / L[(size_t)piv[i] * h + i];
    }
    for (int i = r - 1; i >= 0; --i) {
      double sum = t[i];
      for (int k = i + 1; k < r; ++k) sum -= L[(size_t)piv[k] * h + i] * t[k];
      t[i] = sum / L[(size_t)piv[i] * h + i];
    }
    for (int i = 0; i < r; ++i) Y[(size_t)piv[i] * m + c] = t[i];
  }
  return r;
}

int gram_lstsq_scaled(int h, int m, std::vector<double>& Ghh, std::vector<double>& Ghb, double rtol,
                      std::vector<double>& Y) {
  std::vector<double> sc(h);
  for (int i = 0; i < h; ++i) {
    const double d = Ghh[(size_t)i * h + i];
    sc[i] = d > 0.0 ? 1.0 / std::sqrt(d) : 0.0;
  }
  for (int i = 0; i < h; ++i) {
    for (int j = 0; j < h; ++j) Ghh[(size_t)i * h + j] *= sc[i] * sc[j];
    for (int j = 0; j < m; ++j) Ghb[(size_t)i * m + j] *= sc[i];
  }
  Y.assign((size_t)h * m, 0.0);
  const int r = gram_lstsq(h, m, Ghh.data(), Ghb.data(), rtol, Y.data());
  for (int i = 0; i < h; ++i)
    for (int j = 0; j < m; ++j) Y[(size_t)i * m + j] *= sc[i];
  return r;
}

// Cauchy data of an ADI sweep, C_ij = -1 / (p_i + p_j) = R^T R:  rinv = R^-1 (g x g, row major, upper
// triangular) and cinv1 = C^-1 1 -- in CLOSED FORM, not by a numerical Cholesky factorisation.  Column j of R^-1
// holds the partial-fraction coefficients of the rational function of ADI step j,
//   f_j(s) = sqrt(-2 p_j) / (s + p_j) * prod_{k<j} (s - p_k) / (s + p_k) = sum_{i<=j} c_ij / (s + p_i),
//   c_ij = sqrt(-2 p_j) prod_{k<j} (-p_i - p_k) / ( [i<j] (p_j - p_i) prod_{k<j, k!=i} (p_k - p_i) ),
// and C^-1 1 those of the residual's  prod_k (s - p_k) / (s + p_k) = 1 + sum_i d_i / (s + p_i),
//   d_i = -2 p_i prod_{k!=i} (p_i + p_k) / (p_i - p_k):
// products of sums and differences of the shifts, each entry accurate to a few ulp however ill conditioned C is.
// (Round 1-3 factorised C numerically: the 16 x 16 matrix of 16 NEIGHBOURS of a 32-shift list has condition 4e13,
// its computed R^-1 was wrong by 1e-6 relative, and the gain of the cfg3 Newton iteration came out 1.3e-5 off the
// oracle's -- whatever the GMRES tolerance -- while 16 shifts spread over the same range, cfg2, agreed to 1e-10.)
// Admissible sweeps: the recombination still amplifies the ERRORS OF THE SOLVES by ~ cond(R), so a sweep whose
// smallest pivot R_jj^2 / C_jj = prod_{k<j} ((p_j - p_k) / (p_j + p_k))^2 falls below 1e-6 (cond(R) >~ 1e5; cfg2:
// 2e-3) is refused: the drivers then halve the sweep width.
int cauchy_data(const double* shifts, int g, double* rinv, double* cinv1) {
  if (g < 1) return RICADI_EINVAL;
  typedef long double ld;
  std::vector<ld> p(g);
  for (int i = 0; i < g; ++i) {
    p[i] = (ld)shifts[i];
    if (!(shifts[i] < 0.0)) return RICADI_EINVAL;
    for (int k = 0; k < i; ++k)
      if (shifts[k] == shifts[i]) return RICADI_EBREAKDOWN;
  }
  for (int j = 0; j < g; ++j) {
    ld piv = 1.0L;
    for (int k = 0; k < j; ++k) {
      const ld q = (p[j] - p[k]) / (p[j] + p[k]);
      piv *= q * q;
    }
    if (!(piv > 1e-6L)) return RICADI_EBREAKDOWN;
  }
  for (int i = 0; i < g; ++i)
    for (int j = 0; j < g; ++j) rinv[(size_t)i * g + j] = 0.0;
  for (int j = 0; j < g; ++j)
    for (int i = 0; i <= j; ++i) {
      ld num = sqrtl(-2.0L * p[j]), den = 1.0L;
      for (int k = 0; k < j; ++k) num *= (-p[i] - p[k]);
      if (i < j) den *= (p[j] - p[i]);
      for (int k = 0; k < j; ++k)
        if (k != i) den *= (p[k] - p[i]);
      rinv[(size_t)i * g + j] = (double)(num / den);
    }
  for (int i = 0; i < g; ++i) {
    ld v = -2.0L * p[i];
    for (int k = 0; k < g; ++k)
      if (k != i) v *= (p[i] + p[k]) / (p[i] - p[k]);
    cinv1[i] = (double)v;
  }
  return RICADI_OK;
}

// The width that runs for the window of g shifts behind step `first` of the cycled list: g, halved until cauchy_data
// takes the leading shifts of the window (one shift is always taken).  What the sweep form of the ADI does with a
// window that is not one of its cycle's (a sweep cut by the stopping prediction, and every sweep behind it).
int adi_window_width(const double* shifts, int ns, int first, int g) {
  std::vector<double> ps(g), rinv((size_t)g * g), cinv1(g);
  for (; g >= 2; g /= 2) {
    for (int i = 0; i < g; ++i) ps[i] = shifts[(first + i) % ns];
    if (cauchy_data(ps.data(), g, rinv.data(), cinv1.data()) == RICADI_OK) break;
  }
  return std::max(g, 1);
}

// ---- device records of the preconditioner (uploaded by ricadi_set_operator) ---------------------------------------
// Sorted distinct columns that the rows of every velocity block touch in the CSR matrix (rp, ci): the lists one after
// the other in cols, block b's at [ptr[b], ptr[b + 1]); returns the length of the longest list.
static int block_columns(const HostSetup& hs, const std::vector<int>& rp, const std::vector<int>& ci,
                         std::vector<int>& ptr, std::vector<int>& cols) {
  ptr.assign(hs.nbv + 1, 0);
  cols.clear();
  int kmax = 0;
  std::vector<int> tmp;
  for (int b = 0; b < hs.nbv; ++b) {
    tmp.clear();
    for (int q = hs.bv_ptr[b]; q < hs.bv_ptr[b + 1]; ++q)
      for (int k = rp[hs.bv_rows[q]]; k < rp[hs.bv_rows[q] + 1]; ++k) tmp.push_back(ci[k]);
    std::sort(tmp.begin(), tmp.end());
    tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
    cols.insert(cols.end(), tmp.begin(), tmp.end());
    ptr[b + 1] = (int)cols.size();
    kmax = std::max(kmax, (int)tmp.size());
  }
  return kmax;
}

// Dense bs x ks slice per velocity block of the CSR matrix (rp, ci, v) over the block's column list (ptr, cols of
// block_columns): out[(b bs + row of the block) ks + position of the column in the list] += value.
static std::vector<double> block_slices(const HostSetup& hs, const std::vector<int>& rp, const std::vector<int>& ci,
                                        const std::vector<double>& v, const std::vector<int>& ptr,
                                        const std::vector<int>& cols, int ks) {
  std::vector<double> out((size_t)hs.nbv * hs.bs * ks, 0.0);
  for (int b = 0; b < hs.nbv; ++b) {
    const int* cb = cols.data() + ptr[b];
    const int nc = ptr[b + 1] - ptr[b];
    for (int q = hs.bv_ptr[b]; q < hs.bv_ptr[b + 1]; ++q) {
      const int row = hs.bv_rows[q], il = q - hs.bv_ptr[b];
      for (int k = rp[row]; k < rp[row + 1]; ++k) {
        const int* f = std::lower_bound(cb, cb + nc, ci[k]);
        if (f == cb + nc || *f != ci[k]) throw std::runtime_error("dense block slice: column outside the block's list");
        out[((size_t)b * hs.bs + il) * ks + (int)(f - cb)] += v[k];
      }
    }
  }
  return out;
}

HostSetup build_setup_checked(const HostCsr& A, const HostCsr& E, const HostCsr& J, const HostCsr& JT,
                              const ricadi_opts& o, int max_levels, double sa_omega) {
  HostSetup hs = build_setup(A, E, J, JT, o, max_levels, sa_omega);
  if (!hs.sa) return hs;
  // the folded first sweep takes per-block dense slices of S*P of at most 64 columns
  std::vector<int> ptr, cols;
  const int kmax = block_columns(hs, hs.sy_rp, hs.sy_ci, ptr, cols);
  if (kmax > 64 || !block_apply2_ok(hs.bs, 64)) {
    if (o.verbose)
      fprintf(stderr, "[ricadi] smoothed aggregation off: a velocity block touches %d coarse columns\n", kmax);
    return build_setup(A, E, J, JT, o, max_levels, 0.0);
  }
  return hs;
}

// Multi-shift operands of a CSR matrix with three value sources (a, e, j) in the tile order perm; ncol_v: columns
// below it are velocity columns
static void ms_arrays(const HostSetup& hs, const std::vector<int>& rp, const std::vector<int>& ci,
                      const std::vector<double>& a, const std::vector<double>& e, const std::vector<double>& j,
                      const std::vector<int>& perm, const std::vector<uint16_t>& lidx, int ncol_v,
                      std::vector<double>& aj, std::vector<double>& ee, std::vector<uint16_t>& lm) {
  const size_t nnz = perm.size();
  std::vector<int> rowof(ci.size());
  for (int i = 0; i + 1 < (int)rp.size(); ++i)
    for (int k = rp[i]; k < rp[i + 1]; ++k) rowof[k] = i;
  aj.resize(nnz);
  ee.resize(nnz);
  lm.resize(nnz);
  for (size_t kb = 0; kb < nnz; ++kb) {
    const int k = perm[kb];
    aj[kb] = a[k] + j[k];
    ee[kb] = e[k];
    const bool vv = rowof[k] < hs.nv && ci[k] < ncol_v;
    lm[kb] = (uint16_t)(lidx[kb] | (vv ? 0x8000 : 0));
  }
}

// Row block b of a tile format: its row pointers padded to 33 (rp2) and its column list to mc entries (cols2)
static void pad_tile_block(const std::vector<int>& rowptr, const std::vector<int>& rp, const std::vector<int>& cptr,
                           const std::vector<int>& colsrc, int b, int mc, std::vector<int>& rp2,
                           std::vector<int>& cols2) {
  const int q0 = rowptr[b], nr = rowptr[b + 1] - q0;
  for (int q = 0; q <= 32; ++q) rp2[(size_t)b * 33 + q] = rp[q0 + std::min(q, nr)];
  const int c0 = cptr[b], nc = cptr[b + 1] - c0;
  for (int k = 0; k < nc; ++k) cols2[(size_t)b * mc + k] = colsrc[c0 + k];
}

PrecondRecords build_records(const HostSetup& hs, const HostCsr& J, const HostCsr& JT, bool sweep_meta,
                             bool ms_spmm) {
  PrecondRecords r;
  const int np = hs.np;
  // rectangular last sweep: pressure dofs touched by every velocity block, dense J^T slices
  if (np > 0 && hs.nbv > 0) {
    std::vector<int> ptr, cols;
    const int kmax = block_columns(hs, JT.rp, JT.ci, ptr, cols);
    const int ks = kmax <= 32 ? 32 : (kmax <= 64 ? 64 : (kmax <= 128 ? 128 : 0));
    if (ks > 0 && block_apply_rect_ok(hs.bs, ks)) {
      r.jtd = block_slices(hs, JT.rp, JT.ci, JT.v, ptr, cols, ks);
      r.gt_ptr = std::move(ptr);
      r.gt_cols = std::move(cols);
      r.gt_ks = ks;
      r.gt_kmax = kmax;
      r.gt_ok = true;
    }
  }
  // records of the fused pressure step (pressure_step_kernel): one load per (block, row) instead of the chain
  // block list -> row index -> row pointers
  r.ps_meta.assign((size_t)std::max(hs.nbp, 0) * 32 * PSREC_WIDTH, 0);
  const bool with_sy = hs.kc > 0 && (int)hs.sy_rp.size() == hs.n + 1;
  for (int b = 0; b < hs.nbp; ++b)
    for (int il = 0; il < 32; ++il) {
      int* mt = &r.ps_meta[((size_t)b * 32 + il) * PSREC_WIDTH];
      const int cnt = hs.bp_ptr[b + 1] - hs.bp_ptr[b];
      if (il >= cnt || cnt > 32) {
        mt[PSREC_ROW] = -1;
        continue;
      }
      const int prow = hs.bp_rows[hs.bp_ptr[b] + il];
      mt[PSREC_ROW] = prow;
      mt[PSREC_J0] = J.rp[prow];
      mt[PSREC_J1] = J.rp[prow + 1];
      mt[PSREC_SY0] = with_sy ? hs.sy_rp[hs.nv + prow] : 0;
      mt[PSREC_SY1] = with_sy ? hs.sy_rp[hs.nv + prow + 1] : 0;
      // (the kernel clamps its index loads to the row's last entry: an empty row must not point behind the arrays)
      if (mt[PSREC_J1] == mt[PSREC_J0]) mt[PSREC_J0] = mt[PSREC_J1] = 0;
      if (mt[PSREC_SY1] == mt[PSREC_SY0]) mt[PSREC_SY0] = mt[PSREC_SY1] = 0;
    }
  // dense slices of S*Y per velocity block (first sweep with the coarse residual folded in)
  if (hs.kc > 0 && np > 0 && hs.nbv > 0 && !hs.sy_rp.empty()) {
    std::vector<int> ptr, cols;
    const int kmax = block_columns(hs, hs.sy_rp, hs.sy_ci, ptr, cols);
    const int ks = kmax <= 32 ? 32 : (kmax <= 64 ? 64 : 0);
    if (ks > 0 && block_apply2_ok(hs.bs, ks)) {
      r.dA = block_slices(hs, hs.sy_rp, hs.sy_ci, hs.sy_A, ptr, cols, ks);
      r.dE = block_slices(hs, hs.sy_rp, hs.sy_ci, hs.sy_E, ptr, cols, ks);
      r.dJ = block_slices(hs, hs.sy_rp, hs.sy_ci, hs.sy_J, ptr, cols, ks);
      // (P - Y)[row, :]: its columns are among those of (S P)[row, :] (S has a diagonal)
      if (hs.sa) r.dT = block_slices(hs, hs.pd_rp, hs.pd_ci, hs.pd_v, ptr, cols, ks);
      r.cy_ptr = std::move(ptr);
      r.cy_cols = std::move(cols);
      r.ady_ks = ks;
      r.ady_ok = true;
    }
  }
  // fixed-stride records of the velocity sweeps (block_rect32_kernel, block_two32_kernel; SweepRecs)
  if (sweep_meta && hs.bs == 32 && hs.nbv > 0 && (r.gt_ok || r.ady_ok)) {
    const int kr = r.gt_ok ? r.gt_ks : 0, k2 = r.ady_ok ? r.ady_ks : 0;
    const int stride = swrec_stride(kr, k2);
    std::vector<int> meta((size_t)hs.nbv * stride, 0);
    bool ok = true;
    for (int b = 0; b < hs.nbv && ok; ++b) {
      int* mt = &meta[(size_t)b * stride];
      const int b0 = hs.bv_ptr[b], nb = hs.bv_ptr[b + 1] - b0;
      if (nb > 32 || nb <= 0) { ok = false; break; }
      mt[SWREC_NB] = nb;
      for (int i = 0; i < 32; ++i) {
        const int row = hs.bv_rows[b0 + std::min(i, nb - 1)];
        mt[SWREC_ROWS + i] = row;
        mt[SWREC_AGG + i] = hs.kc > 0 ? hs.aggof[row] : 0;
      }
      if (r.gt_ok) {
        const int i0 = r.gt_ptr[b], ni = r.gt_ptr[b + 1] - i0;
        mt[SWREC_NI_RECT] = ni;
        for (int i = 0; i < kr; ++i) mt[SWREC_IN + i] = ni > 0 ? r.gt_cols[i0 + std::min(i, ni - 1)] : 0;
      }
      if (r.ady_ok) {
        const int i0 = r.cy_ptr[b], ni = r.cy_ptr[b + 1] - i0;
        mt[SWREC_NI_TWO] = ni;
        for (int i = 0; i < k2; ++i) mt[SWREC_IN + kr + i] = ni > 0 ? r.cy_cols[i0 + std::min(i, ni - 1)] : 0;
      }
    }
    if (ok) {
      r.sw_meta = std::move(meta);
      r.sw_stride = stride;
      r.sw_in_rect = SWREC_IN;
      r.sw_in_two = SWREC_IN + kr;
    }
  }
  // tile formats padded to fixed strides: rows2 [nblk][32], rp2 [nblk][33], cols2 [nblk][max cols], colsm2 = cols2
  // through the aggregate map
  const int nb = hs.sb_nblk;
  r.syb_ok = hs.kc > 0 && nb > 0 && hs.syb_max_cols > 0;
  if (r.syb_ok) {
    const int mc = hs.syb_max_cols;
    r.syb_rp2.assign((size_t)nb * 33, 0);
    r.syb_cols2.assign((size_t)nb * mc, -1);
    for (int b = 0; b < nb; ++b)
      pad_tile_block(hs.sb_rowptr, hs.syb_rp, hs.syb_cptr, hs.syb_cols, b, mc, r.syb_rp2, r.syb_cols2);
  }
  {
    const int mc = std::max(hs.sb_max_cols, 1);
    r.sb_rows2.assign((size_t)nb * 32, -1);
    r.sb_rp2.assign((size_t)nb * 33, 0);
    r.sb_cols2.assign((size_t)nb * mc, -1);
    r.sb_colsm2.assign((size_t)nb * mc, -1);
    for (int b = 0; b < nb; ++b) {
      const int q0 = hs.sb_rowptr[b], nr = hs.sb_rowptr[b + 1] - q0;
      for (int q = 0; q < nr; ++q) r.sb_rows2[(size_t)b * 32 + q] = hs.sb_rows[q0 + q];
      pad_tile_block(hs.sb_rowptr, hs.sb_rp, hs.sb_cptr, hs.sb_cols, b, mc, r.sb_rp2, r.sb_cols2);
      for (int k = hs.sb_cptr[b]; k < hs.sb_cptr[b + 1]; ++k)
        r.sb_colsm2[(size_t)b * mc + (k - hs.sb_cptr[b])] = hs.kc > 0 ? hs.aggof[hs.sb_cols[k]] : -1;
    }
  }
  r.sb_ok = nb > 0 && hs.sb_max_cols < 65536;
  // multi-shift operands: those of the saddle operator whenever its tiles are narrow enough, those of S*Y only when
  // the multi-shift kernel is switched on as well
  r.ms_ok = r.sb_ok && hs.sb_max_cols <= 160;
  if (r.ms_ok)
    ms_arrays(hs, hs.s_rp, hs.s_ci, hs.s_srcA, hs.s_srcE, hs.s_srcJ, hs.sb_perm, hs.sb_lidx, hs.nv, r.sbAJ, r.sbE,
              r.sb_lidx_ms);
  if (r.syb_ok && hs.syb_max_cols <= 160 && r.ms_ok && ms_spmm)
    ms_arrays(hs, hs.sy_rp, hs.sy_ci, hs.sy_A, hs.sy_E, hs.sy_J, hs.syb_perm, hs.syb_lidx, hs.kcv, r.sybAJ, r.sybE,
              r.syb_lidx_ms);
  r.sy_chunk = (hs.sy_ci.size() <= (size_t)10 * std::max(hs.n, 1)) ? 8 : 16;
  return r;
}

// ---- coloured Vanka sweep: patches and colours ----------------------------------------
VankaPatches vanka_patches(int nv, const HostCsr& J) {
  VankaPatches vp;
  const int np = J.nrows;
  vp.npress = np;
  std::vector<std::vector<int>> pat(np);
  std::vector<char> held(nv, 0);
  for (int i = 0; i < np; ++i) {
    std::vector<int> ks;
    for (int k = J.rp[i]; k < J.rp[i + 1]; ++k) ks.push_back(k);
    // duplicates of a column (none in a canonical CSR) count once: the first
    std::sort(ks.begin(), ks.end(), [&](int a, int b) { return J.ci[a] != J.ci[b] ? J.ci[a] < J.ci[b] : a < b; });
    ks.erase(std::unique(ks.begin(), ks.end(), [&](int a, int b) { return J.ci[a] == J.ci[b]; }), ks.end());
    if ((int)ks.size() > VANKA_K - 1) {
      // the size cap: the VANKA_K - 1 entries of largest |J_iv|, ties to the lower index
      std::stable_sort(ks.begin(), ks.end(), [&](int a, int b) { return std::fabs(J.v[a]) > std::fabs(J.v[b]); });
      vp.dropped += (int)ks.size() - (VANKA_K - 1);
      ks.resize(VANKA_K - 1);
    }
    std::vector<int>& p = pat[i];
    for (int k : ks) p.push_back(J.ci[k]);
    std::sort(p.begin(), p.end());
    for (int v : p) held[v] = 1;
    p.push_back(nv + i);
    vp.largest = std::max(vp.largest, (int)p.size());
  }
  // first-fit colouring in patch order: per unknown the colours of the patches that hold it so far
  std::vector<std::vector<int>> used(nv);
  std::vector<int> colour(np, 0), mark;
  int ncol = 0;
  for (int i = 0; i < np; ++i) {
    mark.assign(ncol + 1, 0);
    for (size_t q = 0; q + 1 < pat[i].size(); ++q)
      for (int c : used[pat[i][q]]) mark[c] = 1;
    int c = 0;
    while (mark[c]) ++c;
    colour[i] = c;
    ncol = std::max(ncol, c + 1);
    for (size_t q = 0; q + 1 < pat[i].size(); ++q) used[pat[i][q]].push_back(c);
  }
  std::vector<int> lone;
  for (int v = 0; v < nv; ++v)
    if (!held[v]) lone.push_back(v);
  vp.nlone = (int)lone.size();
  vp.nlone_patches = (vp.nlone + VANKA_K - 1) / VANKA_K;
  vp.ncolours = ncol + (vp.nlone_patches > 0 ? 1 : 0);
  vp.npatches = np + vp.nlone_patches;
  vp.colour_ptr.assign(vp.ncolours + 1, 0);
  for (int i = 0; i < np; ++i) ++vp.colour_ptr[colour[i] + 1];
  if (vp.nlone_patches > 0) vp.colour_ptr[vp.ncolours] = vp.nlone_patches;
  for (int c = 0; c < vp.ncolours; ++c) vp.colour_ptr[c + 1] += vp.colour_ptr[c];
  vp.idx.assign((size_t)vp.npatches * VANKA_K, -1);
  std::vector<int> at(vp.colour_ptr.begin(), vp.colour_ptr.end() - 1);
  for (int i = 0; i < np; ++i) std::copy(pat[i].begin(), pat[i].end(), vp.idx.begin() + (size_t)at[colour[i]]++ * VANKA_K);
  for (int q = 0; q < vp.nlone; ++q) vp.idx[(size_t)np * VANKA_K + q] = lone[q];
  return vp;
}

// ---- RADI: the next shift from the projected residual Hamiltonian ---------------------------
// The library links no LAPACK and rocSOLVER has no non-symmetric eigensolver: a small dense solver for real matrices of
// order <= 64 -- balancing (scaling by powers of two), Householder reduction to Hessenberg form, Francis' double-shift
// QR iteration for the eigenvalues (the classical hqr scheme), and per wanted eigenvalue the null vector of
// Ham - lambda I by complex Gaussian elimination with complete pivoting.

// scaling part of the Parlett-Reinsch balancing: a similarity by a diagonal of powers of two (exact)
static void balance_scale(int n, std::vector<double>& a) {
  bool done = false;
  while (!done) {
    done = true;
    for (int i = 0; i < n; ++i) {
      double r = 0.0, c = 0.0;
      for (int j = 0; j < n; ++j)
        if (j != i) {
          c += std::fabs(a[(size_t)j * n + i]);
          r += std::fabs(a[(size_t)i * n + j]);
        }
      if (c == 0.0 || r == 0.0 || !std::isfinite(c) || !std::isfinite(r)) continue;
      double g = r / 2.0, f = 1.0;
      const double s = c + r;
      while (c < g) {
        f *= 2.0;
        c *= 4.0;
      }
      g = r * 2.0;
      while (c > g) {
        f /= 2.0;
        c /= 4.0;
      }
      if ((c + r) / f < 0.95 * s) {
        done = false;
        g = 1.0 / f;
        for (int j = 0; j < n; ++j) a[(size_t)i * n + j] *= g;
        for (int j = 0; j < n; ++j) a[(size_t)j * n + i] *= f;
      }
    }
  }
}

// Householder reduction to upper Hessenberg form in place (the transformations are not kept)
static void hessenberg(int n, std::vector<double>& a) {
  std::vector<double> v(n);
  for (int j = 0; j + 2 < n; ++j) {
    double nrm2 = 0.0;
    for (int i = j + 1; i < n; ++i) nrm2 += a[(size_t)i * n + j] * a[(size_t)i * n + j];
    if (nrm2 == 0.0) continue;
    const double x0 = a[(size_t)(j + 1) * n + j];
    const double alpha = -std::copysign(std::sqrt(nrm2), x0);
    for (int i = j + 1; i < n; ++i) v[i] = a[(size_t)i * n + j];
    v[j + 1] -= alpha;
    double vv = 0.0;
    for (int i = j + 1; i < n; ++i) vv += v[i] * v[i];
    if (vv == 0.0) continue;
    const double beta = 2.0 / vv;
    for (int c = j; c < n; ++c) {          // from the left: rows j + 1 ..
      double s = 0.0;
      for (int i = j + 1; i < n; ++i) s += v[i] * a[(size_t)i * n + c];
      s *= beta;
      for (int i = j + 1; i < n; ++i) a[(size_t)i * n + c] -= s * v[i];
    }
    for (int r = 0; r < n; ++r) {          // from the right: columns j + 1 ..
      double s = 0.0;
      for (int i = j + 1; i < n; ++i) s += a[(size_t)r * n + i] * v[i];
      s *= beta;
      for (int i = j + 1; i < n; ++i) a[(size_t)r * n + i] -= s * v[i];
    }
    a[(size_t)(j + 1) * n + j] = alpha;
    for (int i = j + 2; i < n; ++i) a[(size_t)i * n + j] = 0.0;
  }
}

// Eigenvalues of an upper Hessenberg matrix (destroyed) by the double-shift QR iteration; conjugate pairs come out as
// exact conjugates, real eigenvalues with wi = 0.  false: 60 iterations on one eigenvalue did not converge.
// patient: the second attempt radi_shift_select makes on a fresh copy where the first has failed (Hamiltonians of order
// 64 from wide blocks: met on the N = 8 model runs of tests/radi_dominant_model.py) -- an exceptional shift every ten
// iterations and up to 300 of them; the first attempt and its results are as they always were.
static bool hqr_eigenvalues(int n, std::vector<double>& h, double* wr, double* wi, bool patient = false) {
  const double eps = 2.220446049250313e-16;
  auto A = [&](int i, int j) -> double& { return h[(size_t)i * n + j]; };
  double anorm = 0.0;
  for (int i = 0; i < n; ++i)
    for (int j = std::max(i - 1, 0); j < n; ++j) anorm += std::fabs(A(i, j));
  if (!std::isfinite(anorm)) return false;
  int nn = n - 1;
  double t = 0.0, p = 0.0, q = 0.0, r = 0.0, s, x, y, z, w;
  while (nn >= 0) {
    int its = 0, l;
    do {
      for (l = nn; l >= 1; --l) {
        s = std::fabs(A(l - 1, l - 1)) + std::fabs(A(l, l));
        if (s == 0.0) s = anorm;
        if (std::fabs(A(l, l - 1)) <= eps * s) {
          A(l, l - 1) = 0.0;
          break;
        }
      }
      x = A(nn, nn);
      if (l == nn) {                       // one root
        wr[nn] = x + t;
        wi[nn--] = 0.0;
      } else {
        y = A(nn - 1, nn - 1);
        w = A(nn, nn - 1) * A(nn - 1, nn);
        if (l == nn - 1) {                 // two roots
          p = 0.5 * (y - x);
          q = p * p + w;
          z = std::sqrt(std::fabs(q));
          x += t;
          if (q >= 0.0) {
            z = p + std::copysign(z, p);
            wr[nn - 1] = wr[nn] = x + z;
            if (z != 0.0) wr[nn] = x - w / z;
            wi[nn - 1] = wi[nn] = 0.0;
          } else {
            wr[nn - 1] = wr[nn] = x + p;
            wi[nn - 1] = z;
            wi[nn] = -z;
          }
          nn -= 2;
        } else {
          if (its == (patient ? 300 : 60)) return false;
          if (its == 10 || its == 20 || (patient && its > 20 && its % 10 == 0)) {    // exceptional shift
            t += x;
            for (int i = 0; i <= nn; ++i) A(i, i) -= x;
            s = std::fabs(A(nn, nn - 1)) + std::fabs(A(nn - 1, nn - 2));
            y = x = 0.75 * s;
            w = -0.4375 * s * s;
          }
          ++its;
          int m;
          for (m = nn - 2; m >= l; --m) {  // two consecutive small subdiagonal entries
            z = A(m, m);
            r = x - z;
            s = y - z;
            p = (r * s - w) / A(m + 1, m) + A(m, m + 1);
            q = A(m + 1, m + 1) - z - r - s;
            r = A(m + 2, m + 1);
            s = std::fabs(p) + std::fabs(q) + std::fabs(r);
            if (s != 0.0) {
              p /= s;
              q /= s;
              r /= s;
            }
            if (m == l) break;
            const double u = std::fabs(A(m, m - 1)) * (std::fabs(q) + std::fabs(r));
            const double v = std::fabs(p) * (std::fabs(A(m - 1, m - 1)) + std::fabs(z) + std::fabs(A(m + 1, m + 1)));
            if (u <= eps * v) break;
          }
          for (int i = m + 2; i <= nn; ++i) {
            A(i, i - 2) = 0.0;
            if (i != m + 2) A(i, i - 3) = 0.0;
          }
          for (int k = m; k <= nn - 1; ++k) {   // the double QR step on rows l .. nn, columns m .. nn
            if (k != m) {
              p = A(k, k - 1);
              q = A(k + 1, k - 1);
              r = k != nn - 1 ? A(k + 2, k - 1) : 0.0;
              if ((x = std::fabs(p) + std::fabs(q) + std::fabs(r)) != 0.0) {
                p /= x;
                q /= x;
                r /= x;
              }
            }
            s = std::copysign(std::sqrt(p * p + q * q + r * r), p);
            if (s == 0.0) continue;
            if (k == m) {
              if (l != m) A(k, k - 1) = -A(k, k - 1);
            } else {
              A(k, k - 1) = -s * x;
            }
            p += s;
            x = p / s;
            y = q / s;
            z = r / s;
            q /= p;
            r /= p;
            for (int j = k; j <= nn; ++j) {
              p = A(k, j) + q * A(k + 1, j);
              if (k != nn - 1) {
                p += r * A(k + 2, j);
                A(k + 2, j) -= p * z;
              }
              A(k + 1, j) -= p * y;
              A(k, j) -= p * x;
            }
            const int mmin = nn < k + 3 ? nn : k + 3;
            for (int i = l; i <= mmin; ++i) {
              p = x * A(i, k) + y * A(i, k + 1);
              if (k != nn - 1) {
                p += z * A(i, k + 2);
                A(i, k + 2) -= p * r;
              }
              A(i, k + 1) -= p * q;
              A(i, k) -= p;
            }
          }
        }
      }
    } while (l < nn - 1);
  }
  return true;
}

// Null vector of M = Ham - lambda I (n x n, complex): Gaussian elimination with complete pivoting; the last pivot is
// the one that vanishes, its unknown is set to 1 and the rest follows by back substitution.
static void null_vector(int n, const std::vector<double>& ham, std::complex<double> lambda,
                        std::vector<std::complex<double>>& x) {
  typedef std::complex<double> cd;
  std::vector<cd> M((size_t)n * n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) M[(size_t)i * n + j] = cd(ham[(size_t)i * n + j], 0.0) - (i == j ? lambda : cd(0.0, 0.0));
  std::vector<int> cp(n);
  std::iota(cp.begin(), cp.end(), 0);
  int rank = n - 1;
  for (int k = 0; k < n - 1; ++k) {
    int pi = k, pj = k;
    double best = -1.0;
    for (int i = k; i < n; ++i)
      for (int j = k; j < n; ++j) {
        const double v = std::norm(M[(size_t)i * n + j]);
        if (v > best) {
          best = v;
          pi = i;
          pj = j;
        }
      }
    if (!(best > 0.0)) {                   // the rest is exactly zero: more than one free unknown, take the first
      rank = k;
      break;
    }
    if (pi != k)
      for (int j = 0; j < n; ++j) std::swap(M[(size_t)k * n + j], M[(size_t)pi * n + j]);
    if (pj != k) {
      for (int i = 0; i < n; ++i) std::swap(M[(size_t)i * n + k], M[(size_t)i * n + pj]);
      std::swap(cp[k], cp[pj]);
    }
    const cd piv = M[(size_t)k * n + k];
    for (int i = k + 1; i < n; ++i) {
      const cd f = M[(size_t)i * n + k] / piv;
      if (f == cd(0.0, 0.0)) continue;
      for (int j = k + 1; j < n; ++j) M[(size_t)i * n + j] -= f * M[(size_t)k * n + j];
    }
  }
  std::vector<cd> y(n, cd(0.0, 0.0));
  y[rank] = cd(1.0, 0.0);
  for (int i = rank - 1; i >= 0; --i) {
    cd s(0.0, 0.0);
    for (int j = i + 1; j <= rank; ++j) s += M[(size_t)i * n + j] * y[j];
    y[i] = -s / M[(size_t)i * n + i];
  }
  x.assign(n, cd(0.0, 0.0));
  for (int i = 0; i < n; ++i) x[cp[i]] = y[i];
}

// Ham (2k x 2k, row-major) from H = Q^T [cal A Q | cal E Q | R | U | B] (k x (2k + m + 2nb)):
//   A_c = H_A - H_U H_B^T,  At = H_E^-1 A_c,  Rt = H_E^-1 H_R,  Ham = [[At^T, -H_B H_B^T], [-Rt Rt^T, -At]].
// false: H_E is singular to working precision (LU with partial pivoting) or an entry is not finite.
static bool radi_hamiltonian(int k, int m, int nb, const double* H, std::vector<double>& ham) {
  const int ldh = 2 * k + m + 2 * nb, w = k + m;
  const double *HA = H, *HE = H + k, *HR = H + 2 * k, *HU = H + 2 * k + m, *HB = H + 2 * k + m + nb;
  for (int i = 0; i < k * ldh; ++i)
    if (!std::isfinite(H[i])) return false;
  std::vector<double> E((size_t)k * k), X((size_t)k * w);       // X = [A_c | H_R], then H_E^-1 of it
  double emax = 0.0;
  for (int i = 0; i < k; ++i) {
    for (int j = 0; j < k; ++j) {
      E[(size_t)i * k + j] = HE[(size_t)i * ldh + j];
      emax = std::max(emax, std::fabs(E[(size_t)i * k + j]));
      double s = HA[(size_t)i * ldh + j];
      for (int c = 0; c < nb; ++c) s -= HU[(size_t)i * ldh + c] * HB[(size_t)j * ldh + c];
      X[(size_t)i * w + j] = s;
    }
    for (int j = 0; j < m; ++j) X[(size_t)i * w + k + j] = HR[(size_t)i * ldh + j];
  }
  for (int c = 0; c < k; ++c) {
    int pr = c;
    for (int i = c + 1; i < k; ++i)
      if (std::fabs(E[(size_t)i * k + c]) > std::fabs(E[(size_t)pr * k + c])) pr = i;
    if (!(std::fabs(E[(size_t)pr * k + c]) > 1e-14 * emax)) return false;
    if (pr != c) {
      for (int j = 0; j < k; ++j) std::swap(E[(size_t)c * k + j], E[(size_t)pr * k + j]);
      for (int j = 0; j < w; ++j) std::swap(X[(size_t)c * w + j], X[(size_t)pr * w + j]);
    }
    const double piv = E[(size_t)c * k + c];
    for (int i = c + 1; i < k; ++i) {
      const double f = E[(size_t)i * k + c] / piv;
      if (f == 0.0) continue;
      for (int j = c + 1; j < k; ++j) E[(size_t)i * k + j] -= f * E[(size_t)c * k + j];
      for (int j = 0; j < w; ++j) X[(size_t)i * w + j] -= f * X[(size_t)c * w + j];
    }
  }
  for (int i = k - 1; i >= 0; --i)
    for (int j = 0; j < w; ++j) {
      double s = X[(size_t)i * w + j];
      for (int c = i + 1; c < k; ++c) s -= E[(size_t)i * k + c] * X[(size_t)c * w + j];
      X[(size_t)i * w + j] = s / E[(size_t)i * k + i];
    }
  const int n = 2 * k;
  ham.assign((size_t)n * n, 0.0);
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) {
      ham[(size_t)i * n + j] = X[(size_t)j * w + i];
      ham[(size_t)(k + i) * n + k + j] = -X[(size_t)i * w + j];
      double sb = 0.0, sr = 0.0;
      for (int c = 0; c < nb; ++c) sb += HB[(size_t)i * ldh + c] * HB[(size_t)j * ldh + c];
      for (int c = 0; c < m; ++c) sr += X[(size_t)i * w + k + c] * X[(size_t)j * w + k + c];
      ham[(size_t)i * n + k + j] = -sb;
      ham[(size_t)(k + i) * n + j] = -sr;
    }
  for (double v : ham)
    if (!std::isfinite(v)) return false;
  return true;
}

// The rule: candidates are the eigenvalues of Ham in the open left half plane, one of each conjugate pair (Im >= 0);
// criterion ||q|| / ||x|| of the eigenvector x = [r; q]; the shift of a candidate is -|lambda|.  cands: (shift,
// criterion) of every candidate in the order of the eigenvalues.  wr / wi (2k each, may be NULL): all eigenvalues.
static int radi_shift_candidates(int k, int m, int nb, const double* H, double* wr_out, double* wi_out,
                                 std::vector<std::pair<double, double>>& cands) {
  std::vector<double> ham;
  if (!radi_hamiltonian(k, m, nb, H, ham)) {
    set_error("ricadi_host_radi_shift: H_E is singular or H holds a value that is not finite");
    return RICADI_EBREAKDOWN;
  }
  const int n = 2 * k;
  std::vector<double> h = ham, wr(n), wi(n);
  balance_scale(n, h);
  hessenberg(n, h);
  bool converged = hqr_eigenvalues(n, h, wr.data(), wi.data());
  if (!converged) {
    h = ham;
    balance_scale(n, h);
    hessenberg(n, h);
    converged = hqr_eigenvalues(n, h, wr.data(), wi.data(), true);
  }
  if (!converged) {
    set_error("ricadi_host_radi_shift: the QR iteration did not converge");
    return RICADI_EBREAKDOWN;
  }
  if (wr_out) std::copy(wr.begin(), wr.end(), wr_out);
  if (wi_out) std::copy(wi.begin(), wi.end(), wi_out);
  cands.clear();
  std::vector<std::complex<double>> x;
  for (int i = 0; i < n; ++i) {
    if (!(wr[i] < 0.0) || wi[i] < 0.0) continue;
    null_vector(n, ham, std::complex<double>(wr[i], wi[i]), x);
    double nq = 0.0, nx = 0.0;
    for (int j = 0; j < n; ++j) {
      const double v = std::norm(x[j]);
      nx += v;
      if (j >= k) nq += v;
    }
    cands.emplace_back(-std::hypot(wr[i], wi[i]), nx > 0.0 ? std::sqrt(nq / nx) : 0.0);
  }
  return RICADI_OK;
}

// p = the shift of the candidate with the largest criterion (the first of equal ones), margin = largest / second
// largest (+inf with one candidate), p = 0 without a candidate.
int radi_shift_select(int k, int m, int nb, const double* H, double* p_out, double* margin_out, double* wr_out,
                      double* wi_out) {
  std::vector<std::pair<double, double>> cands;
  const int rc = radi_shift_candidates(k, m, nb, H, wr_out, wi_out, cands);
  if (rc != RICADI_OK) return rc;
  double best = -1.0, second = -1.0, pbest = 0.0;
  for (const auto& cd : cands) {
    const double crit = cd.second;
    if (crit > best) {
      second = best;
      best = crit;
      pbest = cd.first;
    } else if (crit > second) {
      second = crit;
    }
  }
  const int ncand = (int)cands.size();
  *p_out = ncand ? pbest : 0.0;
  if (margin_out)
    *margin_out = ncand >= 2 && second > 0.0 ? best / second : std::numeric_limits<double>::infinity();
  return RICADI_OK;
}

// The next shift from what a step of the RADI driver has fetched: H = Q^T [cal A Q | cal E Q | R | U | B]
// for all m columns of the block's Q (m x (3m + 2nb)), R of its QR (m x m).  The basis of the selection is the columns
// of Q whose diagonal entry of R is at least RICADI_RADI_RANK_TOL of the largest one (a W of deficient rank -- the DRE
// forms of the test problems: 8 columns, rank 4 -- makes every block of Z as deficient, and the other columns of Q are
// then arbitrary directions): the rows of H of those columns, and their columns in the two projected operators.  The
// tolerance is not rounding level: the block's columns come from iterative solves, and columns that depend on their
// predecessors do so only to the solves' accuracy (ricadi.h).
// 0: *p_out / *margin_out hold the shift and its margin.  A RICADI_RADI_REFUSED_* value: the driver falls back to the
// caller's list -- an entry of R that is not finite, R = 0, a breakdown of the selection, no candidate or a shift that
// is not finite and negative.  *kept_out (may be NULL): the size of the basis, 0 where R itself is refused.
int radi_next_shift(int m, int nb, const double* hH, const double* hR, double* p_out, double* margin_out,
                    int* kept_out) {
  const int hw = 3 * m + 2 * nb;
  if (kept_out) *kept_out = 0;
  double dmax = 0.0;
  for (int i = 0; i < m; ++i) {
    const double d = std::fabs(hR[(size_t)i * m + i]);
    if (!(d <= std::numeric_limits<double>::max())) return RICADI_RADI_REFUSED_R_NOT_FINITE;
    dmax = std::max(dmax, d);
  }
  if (dmax == 0.0) return RICADI_RADI_REFUSED_R_ZERO;
  std::vector<int> keep;
  for (int i = 0; i < m; ++i)
    if (std::fabs(hR[(size_t)i * m + i]) >= RICADI_RADI_RANK_TOL * dmax) keep.push_back(i);
  const int k = (int)keep.size(), kw = 2 * k + m + 2 * nb;
  if (kept_out) *kept_out = k;
  std::vector<double> Hk((size_t)k * kw);
  for (int a = 0; a < k; ++a) {
    const double* row = hH + (size_t)keep[a] * hw;
    double* out = Hk.data() + (size_t)a * kw;
    for (int b = 0; b < k; ++b) {
      out[b] = row[keep[b]];
      out[k + b] = row[m + keep[b]];
    }
    std::copy(row + 2 * m, row + hw, out + 2 * k);
  }
  double p = 0.0, margin = 0.0;
  if (radi_shift_select(k, m, nb, Hk.data(), &p, &margin, nullptr, nullptr) != RICADI_OK)
    return RICADI_RADI_REFUSED_BREAKDOWN;
  if (!(p < 0.0) || !(p >= -std::numeric_limits<double>::max())) return RICADI_RADI_REFUSED_NO_SHIFT;
  *p_out = p;
  if (margin_out) *margin_out = margin;
  return 0;
}

// Singular values and left singular vectors of R (m x m, row-major) by one-sided (Hestenes) Jacobi: plane rotations
// from the right make the columns of A = R mutually orthogonal, A V = U Sigma; their norms are the singular values,
// the normalised columns the left singular vectors.  The method works on R itself -- an eigensolver on R R^T would
// square the condition and lose every singular value below 1e-8 of the largest, where RICADI_RADI_RANK_TOL cuts.
// Sweeps over all pairs in a fixed order until no pair's cosine exceeds 1e-15 sqrt(m), the rounding error of the
// cosine itself (at most 60 sweeps).  A: the rotated
// matrix, COLUMN by column (A[j m + i] = entry (i, j)); sig: the column norms.
// jacobi_rotate_columns is the iteration for `cols` columns of length `rows`; V (optional, cols x cols, column by column,
// the identity on entry) takes the same rotations, so that A_in V = A_out.  Returns whether a sweep without a rotation
// was reached (false: the 60 sweeps ran out and the columns may not be orthogonal to the tolerance).
static bool jacobi_rotate_columns(int rows, int cols, std::vector<double>& A, double* V) {
  const int m = rows;
  const double tol = 1e-15 * std::sqrt((double)m);
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < cols - 1; ++p)
      for (int q = p + 1; q < cols; ++q) {
        double* ap = A.data() + (size_t)p * m;
        double* aq = A.data() + (size_t)q * m;
        double a = 0.0, b = 0.0, g = 0.0;
        for (int i = 0; i < m; ++i) {
          a += ap[i] * ap[i];
          b += aq[i] * aq[i];
          g += ap[i] * aq[i];
        }
        if (g == 0.0 || !(std::fabs(g) > tol * std::sqrt(a) * std::sqrt(b))) continue;
        rotated = true;
        const double zeta = (b - a) / (2.0 * g);
        const double t = std::copysign(1.0, zeta) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t;
        for (int i = 0; i < m; ++i) {
          const double x = ap[i], y = aq[i];
          ap[i] = cs * x - sn * y;
          aq[i] = sn * x + cs * y;
        }
        if (V) {
          double* vp = V + (size_t)p * cols;
          double* vq = V + (size_t)q * cols;
          for (int i = 0; i < cols; ++i) {
            const double x = vp[i], y = vq[i];
            vp[i] = cs * x - sn * y;
            vq[i] = sn * x + cs * y;
          }
        }
      }
    if (!rotated) return true;
  }
  return false;
}
static void column_norms(int rows, int cols, const std::vector<double>& A, std::vector<double>& sig) {
  sig.resize(cols);
  for (int j = 0; j < cols; ++j) {
    double s = 0.0;
    for (int i = 0; i < rows; ++i) s += A[(size_t)j * rows + i] * A[(size_t)j * rows + i];
    sig[j] = std::sqrt(s);
  }
}
static void jacobi_left_svd(int m, const double* R, std::vector<double>& A, std::vector<double>& sig) {
  A.resize((size_t)m * m);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) A[(size_t)j * m + i] = R[(size_t)i * m + j];
  (void)jacobi_rotate_columns(m, m, A, nullptr);       // (the shift selection takes what 60 sweeps give, as before)
  column_norms(m, m, A, sig);
}

// ---- square-root balancing of two low-rank factors (ricadi_host_lqg_balance) -----------------
// S = Zc^T M Zf (kc x kf, row-major) = U Sigma V^T by the Jacobi iteration above on the SHORTER side's columns (S when
// kc >= kf, else S^T), the rotations accumulated for the other side's vectors.  r = #{sigma_i > tol sigma_1}, at most
// `order` (order <= 0: no cap).  sig_out: all min(kc, kf) values, descending.  coefL (kc x r) = U_r Sigma_r^-1/2 and
// coefR (kf x r) = V_r Sigma_r^-1/2, row-major with leading dimension r, so that coefL^T S coefR = I_r; the caller's
// buffers hold kc (kf) times min(kc, kf, order) doubles.  RICADI_ENOCONV (nothing written but *r_out = 0) if the
// iteration has not converged in its 60 sweeps.
int lqg_balance(int kc, int kf, const double* S, double tol, int order, int* r_out, double* sig_out, double* coefL,
                double* coefR) {
  *r_out = 0;
  bool nonzero = false;
  for (size_t i = 0; i < (size_t)kc * kf; ++i) {
    if (!(std::fabs(S[i]) <= std::numeric_limits<double>::max())) return RICADI_EINVAL;
    nonzero = nonzero || S[i] != 0.0;
  }
  if (!nonzero) return RICADI_EBREAKDOWN;
  const bool tall = kc >= kf;                    // rotate the columns of S itself
  const int rows = tall ? kc : kf, cols = tall ? kf : kc;
  std::vector<double> A((size_t)rows * cols), W((size_t)cols * cols, 0.0), sig;
  for (int j = 0; j < cols; ++j) {
    W[(size_t)j * cols + j] = 1.0;
    for (int i = 0; i < rows; ++i) A[(size_t)j * rows + i] = tall ? S[(size_t)i * kf + j] : S[(size_t)j * kf + i];
  }
  if (!jacobi_rotate_columns(rows, cols, A, W.data())) return RICADI_ENOCONV;
  column_norms(rows, cols, A, sig);
  std::vector<int> idx(cols);
  std::iota(idx.begin(), idx.end(), 0);
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return sig[a] > sig[b]; });
  const double smax = sig[idx[0]];
  if (!(smax > 0.0) || !(smax <= std::numeric_limits<double>::max())) return RICADI_EBREAKDOWN;
  for (int a = 0; a < cols; ++a) sig_out[a] = sig[idx[a]];
  int r = 0;
  while (r < cols && (order <= 0 || r < order) && sig[idx[r]] > tol * smax) ++r;
  *r_out = r;
  // the long vectors (columns of A over their norms) belong to the side that was rotated, the accumulated ones to the other
  double* longc = tall ? coefL : coefR;
  double* shortc = tall ? coefR : coefL;
  for (int a = 0; a < r; ++a) {
    const int j = idx[a];
    const double sg = sig[j], sq = 1.0 / std::sqrt(sg);
    for (int i = 0; i < rows; ++i) longc[(size_t)i * r + a] = A[(size_t)j * rows + i] / sg * sq;
    for (int i = 0; i < cols; ++i) shortc[(size_t)i * r + a] = W[(size_t)j * cols + i] * sq;
  }
  return RICADI_OK;
}

// radi_next_shift with the basis Q S in place of a choice of columns of Q (RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT;
// DESIGN.md 3d-2): S (m x k) holds the left singular vectors of R of its k = min(32, #{sigma_i >= RICADI_RADI_RANK_TOL
// sigma_1}) largest singular values, so Q S spans the dominant part of the block's range whatever the order of its
// columns, and a block of up to 127 columns leaves a selection of order 2k <= 64.  The packed matrix handed to
// radi_shift_select is  [S^T H_A S | S^T H_E S | S^T (H_R, H_U, H_B)]  (k x (2k + m + 2nb)).
// Return values and *kept_out as radi_next_shift; here EVERY entry of R is looked at, not only its diagonal.
// The basis Q S of a group of c columns against an m-column residual (c = m: the block of one step; c != m: the kept
// blocks of a sweep): hH is c x (2c + m + 2nb), hR c x c; Hk the rotated k x (2k + m + 2nb).
static int radi_dominant_rotate(int c, int m, int nb, const double* hH, const double* hR, std::vector<double>& Hk,
                                int* k_out) {
  const int hw = 2 * c + m + 2 * nb;
  *k_out = 0;
  for (int i = 0; i < c * c; ++i)
    if (!(std::fabs(hR[i]) <= std::numeric_limits<double>::max())) return RICADI_RADI_REFUSED_R_NOT_FINITE;
  std::vector<double> A, sig;
  jacobi_left_svd(c, hR, A, sig);
  std::vector<int> order(c);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sig[a] > sig[b]; });
  const double smax = sig[order[0]];
  if (!(smax <= std::numeric_limits<double>::max())) return RICADI_RADI_REFUSED_R_NOT_FINITE;
  if (smax == 0.0) return RICADI_RADI_REFUSED_R_ZERO;
  int k = 0;
  while (k < c && k < 32 && sig[order[k]] >= RICADI_RADI_RANK_TOL * smax) ++k;
  *k_out = k;
  // S by columns: S[a] = column order[a] of A over its norm
  std::vector<double> S((size_t)k * c);
  for (int a = 0; a < k; ++a)
    for (int i = 0; i < c; ++i) S[(size_t)a * c + i] = A[(size_t)order[a] * c + i] / sig[order[a]];
  // T = S^T H (k x hw), then the two projected operators once more from the right
  const int kw = 2 * k + m + 2 * nb;
  std::vector<double> T((size_t)k * hw, 0.0);
  Hk.assign((size_t)k * kw, 0.0);
  for (int a = 0; a < k; ++a)
    for (int i = 0; i < c; ++i) {
      const double s = S[(size_t)a * c + i];
      const double* row = hH + (size_t)i * hw;
      double* out = T.data() + (size_t)a * hw;
      for (int j = 0; j < hw; ++j) out[j] += s * row[j];
    }
  for (int a = 0; a < k; ++a) {
    const double* t = T.data() + (size_t)a * hw;
    double* out = Hk.data() + (size_t)a * kw;
    for (int b = 0; b < k; ++b) {
      double sa = 0.0, se = 0.0;
      for (int j = 0; j < c; ++j) {
        sa += t[j] * S[(size_t)b * c + j];
        se += t[c + j] * S[(size_t)b * c + j];
      }
      out[b] = sa;
      out[k + b] = se;
    }
    std::copy(t + 2 * c, t + hw, out + 2 * k);
  }
  return 0;
}

int radi_next_shift_dominant(int m, int nb, const double* hH, const double* hR, double* p_out, double* margin_out,
                             int* kept_out) {
  std::vector<double> Hk;
  int k = 0;
  const int refused = radi_dominant_rotate(m, m, nb, hH, hR, Hk, &k);
  if (kept_out) *kept_out = k;
  if (refused) return refused;
  double p = 0.0, margin = 0.0;
  if (radi_shift_select(k, m, nb, Hk.data(), &p, &margin, nullptr, nullptr) != RICADI_OK)
    return RICADI_RADI_REFUSED_BREAKDOWN;
  if (!(p < 0.0) || !(p >= -std::numeric_limits<double>::max())) return RICADI_RADI_REFUSED_NO_SHIFT;
  *p_out = p;
  if (margin_out) *margin_out = margin;
  return 0;
}

static long double radi_sweep_pivot(const double* ps, int g);

// The shifts of the NEXT SWEEP from what a sweep has fetched (ricadi_set_radi_sweep_shifts): the
// dominant rule on the group of c columns of Z the sweep kept (hH c x (2c + m + 2nb), hR c x c), all candidates ordered
// by descending criterion (on an exact tie the larger |lambda| first), and of those up to `want`, greedily: a candidate
// is admitted if it is finite and negative and the smallest Cauchy pivot of the admitted list with it appended
// (cauchy_data's pivots, in acceptance order) stays >= RICADI_RADI_SWEEP_PIVOT.  ps_out / crit_out (want each): the
// admitted shifts in acceptance order and their criteria, *n_out their number.  Returns 0, or a RICADI_RADI_REFUSED_*
// value (NO_SHIFT where no candidate is admitted; *n_out = 0 then).  want = 1 is radi_next_shift_dominant's shift.
int radi_next_shifts_dominant(int c, int m, int nb, const double* hH, const double* hR, int want, double* ps_out,
                              double* crit_out, int* n_out, int* kept_out) {
  *n_out = 0;
  std::vector<double> Hk;
  int k = 0;
  const int refused = radi_dominant_rotate(c, m, nb, hH, hR, Hk, &k);
  if (kept_out) *kept_out = k;
  if (refused) return refused;
  std::vector<std::pair<double, double>> cands;
  if (radi_shift_candidates(k, m, nb, Hk.data(), nullptr, nullptr, cands) != RICADI_OK)
    return RICADI_RADI_REFUSED_BREAKDOWN;
  std::stable_sort(cands.begin(), cands.end(), [](const std::pair<double, double>& a, const std::pair<double, double>& b) {
    return a.second > b.second || (a.second == b.second && a.first < b.first);
  });
  std::vector<double> acc;
  for (const auto& cd : cands) {
    if ((int)acc.size() >= want) break;
    const double p = cd.first;
    if (!(p < 0.0) || !(p >= -std::numeric_limits<double>::max())) continue;
    acc.push_back(p);
    if (radi_sweep_pivot(acc.data(), (int)acc.size()) >= (long double)RICADI_RADI_SWEEP_PIVOT) {
      ps_out[acc.size() - 1] = p;
      if (crit_out) crit_out[acc.size() - 1] = cd.second;
    } else {
      acc.pop_back();
    }
  }
  *n_out = (int)acc.size();
  return acc.empty() ? RICADI_RADI_REFUSED_NO_SHIFT : 0;
}

// ---- the sweep form of RADI (solver_radi.inl) ------------------------------------------------
// What the host does between the one fetch of a sweep and the recombination kernel.  With the g shifts p, Gh = Vh^T B
// (g m x nb) and Gamma = P^T P, P = [R_0 | cal E Vh]:
//   M_gh = -(I_m + Gh_g Gh_h^T) / (p_g + p_h) = L L^T,  y = L^-1 (1_g (x) I_m),  h = L^-1 Gh,  T_j = L^-T[:, :j m],
//   res_j = ||c_j^T Gamma c_j||_F / rhs,  c_j = [I_m; T_j y[:j m]],   Cf = [T_k | T_k y[:k m] | T_k h[:k m]].
// T_j y[:j m] and T_j h[:j m] grow by the rows of block j from one step to the next, so the whole history costs one
// pass over L^-1.  Arithmetic: long double for M, its factor, L^-1 and the coefficients.  M inherits the conditioning of the sweep's Cauchy matrix (cond(M) up to
// ~1 / RICADI_RADI_SWEEP_PIVOT^2 and more when Gh is large), and FP64 would lose that many digits of Cf before the
// kernel ever uses it; with 11 more bits the factorisation's error stays below the rounding of Cf to FP64 for every
// admitted sweep.  The quadratic forms of the history run in FP64: their input Gamma is an FP64 Gram matrix.  At
// g m = 128 that leaves ~1e6 long double multiply-adds per sweep of 8 solves (DESIGN.md 3d-3 has the measured time).
int radi_sweep(int g, int m, int nb, const double* shifts, const double* Ghat, const double* Gamma, double rhs,
               double res_reltol, int steps_left, int* k_out, double* res_out, double* Cf_out) {
  typedef long double ld;
  const int K = g * m, nc = K + m;
  std::vector<ld> L((size_t)K * K, 0.0L), Li((size_t)K * K, 0.0L);
  for (int a = 0; a < g; ++a)
    for (int b = 0; b <= a; ++b) {
      const ld den = -((ld)shifts[a] + (ld)shifts[b]);
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
          ld s = i == j ? 1.0L : 0.0L;
          const double *gi = Ghat + (size_t)(a * m + i) * nb, *gj = Ghat + (size_t)(b * m + j) * nb;
          for (int t = 0; t < nb; ++t) s += (ld)gi[t] * (ld)gj[t];
          L[(size_t)(a * m + i) * K + b * m + j] = s / den;
        }
    }
  // Cholesky factor in the lower triangle, row by row
  for (int i = 0; i < K; ++i) {
    for (int j = 0; j <= i; ++j) {
      ld s = L[(size_t)i * K + j];
      for (int t = 0; t < j; ++t) s -= L[(size_t)i * K + t] * L[(size_t)j * K + t];
      if (j < i) {
        L[(size_t)i * K + j] = s / L[(size_t)j * K + j];
      } else {
        if (!(s > 0.0L) || !(s <= (ld)std::numeric_limits<double>::max())) return RICADI_EBREAKDOWN;
        L[(size_t)i * K + i] = sqrtl(s);
      }
    }
    for (int j = i + 1; j < K; ++j) L[(size_t)i * K + j] = 0.0L;
  }
  // L^-1 by forward substitution, row by row (row i of L X = I: unit-stride updates with the rows above, t ascending)
  for (int i = 0; i < K; ++i) {
    ld* xi = &Li[(size_t)i * K];
    for (int t = 0; t < i; ++t) {
      const ld l = L[(size_t)i * K + t];
      const ld* xt = &Li[(size_t)t * K];
      for (int j = 0; j <= t; ++j) xi[j] -= l * xt[j];
    }
    const ld d = L[(size_t)i * K + i];
    for (int j = 0; j < i; ++j) xi[j] /= d;
    xi[i] = 1.0L / d;
  }
  std::vector<ld> y((size_t)K * m, 0.0L), h((size_t)K * nb, 0.0L), ty((size_t)K * m, 0.0L), th((size_t)K * nb, 0.0L);
  for (int i = 0; i < K; ++i) {
    for (int t = 0; t <= i; ++t) y[(size_t)i * m + t % m] += Li[(size_t)i * K + t];
    for (int t = 0; t <= i; ++t)
      for (int b = 0; b < nb; ++b) h[(size_t)i * nb + b] += Li[(size_t)i * K + t] * (ld)Ghat[(size_t)t * nb + b];
  }
  const int jmax = std::min(g, steps_left);
  // the quadratic form in FP64: Gamma is an FP64 Gram matrix, off by 2^-53 |P|^T |P| already, and c is rounded once
  std::vector<double> gc((size_t)nc * m), tyd((size_t)K * m, 0.0);
  int k = 0;
  for (int j = 1; j <= jmax; ++j) {
    // rows of block j of L^-1 enter T_j y and T_j h (L^-T[i, r] = L^-1[r, i], zero for i > r)
    for (int r = (j - 1) * m; r < j * m; ++r)
      for (int i = 0; i <= r; ++i) {
        const ld l = Li[(size_t)r * K + i];
        for (int a = 0; a < m; ++a) ty[(size_t)i * m + a] += l * y[(size_t)r * m + a];
        for (int b = 0; b < nb; ++b) th[(size_t)i * nb + b] += l * h[(size_t)r * nb + b];
      }
    // c = [I_m; ty] has rows below (j + 1) m only
    const int nr = (j + 1) * m;
    for (int i = 0; i < j * m; ++i)
      for (int a = 0; a < m; ++a) tyd[(size_t)i * m + a] = (double)ty[(size_t)i * m + a];
    for (int i = 0; i < nr; ++i) {
      double* gi = &gc[(size_t)i * m];
      for (int a = 0; a < m; ++a) gi[a] = Gamma[(size_t)i * nc + a];
      for (int t = m; t < nr; ++t) {
        const double gam = Gamma[(size_t)i * nc + t];
        for (int a = 0; a < m; ++a) gi[a] += gam * tyd[(size_t)(t - m) * m + a];
      }
    }
    double f = 0.0;
    for (int a = 0; a < m; ++a)
      for (int b = 0; b < m; ++b) {
        double s = gc[(size_t)a * m + b];
        for (int t = m; t < nr; ++t) s += tyd[(size_t)(t - m) * m + a] * gc[(size_t)t * m + b];
        f += s * s;
      }
    const double res = rhs > 0.0 ? std::sqrt(f) / rhs : 0.0;
    res_out[j - 1] = res;
    k = j;
    if (res <= res_reltol) break;
  }
  *k_out = k;                       // (ty / th hold the sums of the first k blocks)
  const int km = k * m, ldc = km + m + nb;
  for (int i = 0; i < K; ++i) {
    double* row = Cf_out + (size_t)i * ldc;
    for (int c = 0; c < km; ++c) row[c] = c >= i ? (double)Li[(size_t)c * K + i] : 0.0;
    for (int a = 0; a < m; ++a) row[km + a] = (double)ty[(size_t)i * m + a];
    for (int b = 0; b < nb; ++b) row[km + m + b] = (double)th[(size_t)i * nb + b];
  }
  return RICADI_OK;
}

// min_j prod_{k<j} ((p_j - p_k) / (p_j + p_k))^2 of a sweep's shifts: cauchy_data's pivots (0 where two are equal)
static long double radi_sweep_pivot(const double* ps, int g) {
  long double out = 1.0L;
  for (int j = 0; j < g; ++j) {
    long double piv = 1.0L;
    for (int k = 0; k < j; ++k) {
      const long double q = ((long double)ps[j] - (long double)ps[k]) / ((long double)ps[j] + (long double)ps[k]);
      piv *= q * q;
    }
    out = std::min(out, piv);
  }
  return out;
}

int radi_sweep_groups(int mw, int nb) { return mw + nb > 32 ? (mw + nb + 15) / 16 : 1; }
// The widest sweep the kernels and the batched solve take at these panel widths
int radi_sweep_cap(int mw, int nb) {
  return std::min(RICADI_RADI_SWEEP_MAX_K / mw, RICADI_MAX_GROUPS / radi_sweep_groups(mw, nb));
}

// The effective sweep width of a cycled list (1: the sequential form).  Host arithmetic only.
int radi_sweep_width(const double* shifts, int ns, int mw, int nb, int want, int max_steps) {
  int G = std::min(std::min(want, ns), radi_sweep_cap(mw, nb));
  G = std::max(1, std::min(G, max_steps));
  std::vector<double> ps;
  for (; G >= 2; G /= 2) {
    const int nsweep = ns / std::gcd(ns, G);
    bool ok = true;
    for (int s = 0; s < nsweep && ok; ++s) {
      ps.resize(G);
      for (int i = 0; i < G; ++i) ps[i] = shifts[((size_t)s * G + i) % ns];
      ok = radi_sweep_pivot(ps.data(), G) >= (long double)RICADI_RADI_SWEEP_PIVOT;
    }
    if (ok) return G;
  }
  return 1;
}

}  // namespace ricadi

extern "C" {

int ricadi_host_radi_sweep(int g, int m, int nb, const double* shifts, const double* Ghat, const double* Gamma,
                           double rhs, double res_reltol, int steps_left, int* k_out, double* res_out,
                           double* Cf_out) {
  if (g < 1 || g > RICADI_MAX_GROUPS || m < 1 || g * m > RICADI_RADI_SWEEP_MAX_K || nb < 1 || nb > 64 || steps_left < 1 ||
      !shifts || !Ghat || !Gamma || !k_out || !res_out || !Cf_out) {
    ricadi::set_error("ricadi_host_radi_sweep: bad argument (1 <= g <= 16, g m <= 128, 1 <= nb <= 64, steps_left >= 1)");
    return RICADI_EINVAL;
  }
  for (int i = 0; i < g; ++i) {
    bool ok = shifts[i] < 0.0;
    for (int j = 0; j < i; ++j) ok = ok && shifts[i] != shifts[j];
    if (!ok) {
      ricadi::set_error("ricadi_host_radi_sweep: the shifts of a sweep must be negative and pairwise distinct");
      return RICADI_EINVAL;
    }
  }
  try {
    const int rc = ricadi::radi_sweep(g, m, nb, shifts, Ghat, Gamma, rhs, res_reltol, steps_left, k_out, res_out, Cf_out);
    if (rc == RICADI_EBREAKDOWN)
      ricadi::set_error("RADI sweep: M has a pivot that is not positive and finite (NaN / Inf in a shift solve)");
    return rc;
  } catch (const std::exception&) {
    ricadi::set_error("ricadi_host_radi_sweep: exception");
    return RICADI_EHIP;
  }
}

int ricadi_host_radi_sweep_width(const double* shifts, int ns, int mw, int nb, int want, int max_steps,
                                 int* width_out) {
  if (!shifts || !width_out || ns < 1 || mw < 1 || nb < 1 || nb > 64 || mw + nb > RICADI_MAX_M || want < 1 ||
      want > RICADI_MAX_GROUPS || max_steps < 1) {
    ricadi::set_error("ricadi_host_radi_sweep_width: bad argument");
    return RICADI_EINVAL;
  }
  for (int i = 0; i < ns; ++i)
    if (!(shifts[i] < 0.0)) {
      ricadi::set_error("ricadi_host_radi_sweep_width: RADI shifts must be negative");
      return RICADI_EINVAL;
    }
  try {
    *width_out = ricadi::radi_sweep_width(shifts, ns, mw, nb, want, max_steps);
  } catch (const std::exception&) {
    ricadi::set_error("ricadi_host_radi_sweep_width: exception");
    return RICADI_EHIP;
  }
  return RICADI_OK;
}

static int radi_shift_entry(int k, int m, int nb, const double* H, double* p_out, double* margin_out, double* wr,
                            double* wi) {
  if (k < 1 || k > 32 || m < 1 || m > 32 || nb < 1 || nb > 64 || !H || !p_out) {
    ricadi::set_error("ricadi_host_radi_shift: bad argument (1 <= k, m <= 32, 1 <= nb <= 64)");
    return RICADI_EINVAL;
  }
  try {
    return ricadi::radi_shift_select(k, m, nb, H, p_out, margin_out, wr, wi);
  } catch (const std::exception&) {
    ricadi::set_error("ricadi_host_radi_shift: exception");
    return RICADI_EHIP;
  }
}

int ricadi_host_radi_shift(int k, int m, int nb, const double* H, double* p_out, double* margin_out) {
  return radi_shift_entry(k, m, nb, H, p_out, margin_out, nullptr, nullptr);
}

int ricadi_host_radi_shift_eigs(int k, int m, int nb, const double* H, double* p_out, double* margin_out,
                                double* wr_out, double* wi_out) {
  return radi_shift_entry(k, m, nb, H, p_out, margin_out, wr_out, wi_out);
}

int ricadi_host_radi_next_shift(int m, int nb, const double* H, const double* R, double* p_out, double* margin_out,
                                int* kept_out) {
  if (m < 1 || m > 32 || nb < 1 || nb > 64 || !H || !R || !p_out) {
    ricadi::set_error("ricadi_host_radi_next_shift: bad argument (1 <= m <= 32, 1 <= nb <= 64)");
    return RICADI_EINVAL;
  }
  try {
    return ricadi::radi_next_shift(m, nb, H, R, p_out, margin_out, kept_out);
  } catch (const std::exception&) {
    ricadi::set_error("ricadi_host_radi_next_shift: exception");
    return RICADI_EHIP;
  }
}

int ricadi_host_radi_next_shift_dominant(int m, int nb, const double* H, const double* R, double* p_out,
                                         double* margin_out, int* kept_out) {
  if (m < 1 || m > 127 || nb < 1 || nb > 64 || !H || !R || !p_out) {
    ricadi::set_error("ricadi_host_radi_next_shift_dominant: bad argument (1 <= m <= 127, 1 <= nb <= 64)");
    return RICADI_EINVAL;
  }
  try {
    return ricadi::radi_next_shift_dominant(m, nb, H, R, p_out, margin_out, kept_out);
  } catch (const std::exception&) {
    ricadi::set_error("ricadi_host_radi_next_shift_dominant: exception");
    return RICADI_EHIP;
  }
}

int ricadi_host_radi_sweep_shifts(int c, int m, int nb, const double* H, const double* R, int want, double* ps_out,
                                  double* crit_out, int* n_out, int* kept_out) {
  if (c < 1 || c > 127 || m < 1 || m > 127 || nb < 1 || nb > 64 || want < 1 || want > RICADI_MAX_GROUPS || !H || !R ||
      !ps_out || !n_out) {
    ricadi::set_error("ricadi_host_radi_sweep_shifts: bad argument (1 <= c, m <= 127, 1 <= nb <= 64, 1 <= want <= 16)");
    return RICADI_EINVAL;
  }
  try {
    return ricadi::radi_next_shifts_dominant(c, m, nb, H, R, want, ps_out, crit_out, n_out, kept_out);
  } catch (const std::exception&) {
    ricadi::set_error("ricadi_host_radi_sweep_shifts: exception");
    return RICADI_EHIP;
  }
}

int ricadi_host_lqg_balance(int kc, int kf, const double* S, double tol, int order, int* r_out, double* sigma_out,
                            double* coefl_out, double* coefr_out) {
  if (kc < 1 || kf < 1 || !S || !(tol >= 0.0 && tol < 1.0) || !r_out || !sigma_out || !coefl_out || !coefr_out) {
    ricadi::set_error("ricadi_host_lqg_balance: bad argument (kc, kf >= 1, 0 <= tol < 1)");
    return RICADI_EINVAL;
  }
  try {
    const int rc = ricadi::lqg_balance(kc, kf, S, tol, order, r_out, sigma_out, coefl_out, coefr_out);
    if (rc == RICADI_EINVAL) ricadi::set_error("ricadi_host_lqg_balance: S has an entry that is not finite");
    if (rc == RICADI_EBREAKDOWN) ricadi::set_error("ricadi_host_lqg_balance: S is zero");
    if (rc == RICADI_ENOCONV) ricadi::set_error("ricadi_host_lqg_balance: the Jacobi SVD did not converge in 60 sweeps");
    return rc;
  } catch (const std::exception&) {
    ricadi::set_error("ricadi_host_lqg_balance: exception");
    return RICADI_EHIP;
  }
}

int ricadi_host_vanka_patches(int nv, int np, const int32_t* j_rp, const int32_t* j_ci, const double* j_v,
                              int32_t* sizes_out, int32_t* colour_ptr, int32_t* patch_idx) {
  if (nv < 1 || np < 0 || !sizes_out || (np > 0 && (!j_rp || !j_ci || !j_v))) {
    ricadi::set_error("ricadi_host_vanka_patches: bad argument");
    return RICADI_EINVAL;
  }
  try {
    const int32_t zero = 0;
    const double dzero = 0.0;
    const ricadi::HostCsr J = np > 0 ? ricadi::make_csr(np, nv, j_rp, j_ci, j_v) : ricadi::make_csr(0, nv, &zero, &zero, &dzero);
    for (size_t k = 0; k < J.nnz(); ++k)
      if (J.ci[k] < 0 || J.ci[k] >= nv) {
        ricadi::set_error("ricadi_host_vanka_patches: column index out of range");
        return RICADI_EINVAL;
      }
    const ricadi::VankaPatches vp = ricadi::vanka_patches(nv, J);
    const int32_t sz[8] = {vp.ncolours, vp.npatches, vp.npress, vp.largest, vp.dropped, vp.nlone, vp.nlone_patches, 0};
    std::copy(sz, sz + 8, sizes_out);
    if (colour_ptr) std::copy(vp.colour_ptr.begin(), vp.colour_ptr.end(), colour_ptr);
    if (patch_idx) std::copy(vp.idx.begin(), vp.idx.end(), patch_idx);
  } catch (...) {
    ricadi::set_error("ricadi_host_vanka_patches: exception");
    return RICADI_EINVAL;
  }
  return RICADI_OK;
}

int ricadi_host_aggregate(int n, const int32_t* rowptr, const int32_t* col, int bsize,
                          int32_t* blk_out) {
  if (n < 0 || !rowptr || !col || !blk_out) {
    ricadi::set_error("ricadi_host_aggregate: bad argument");
    return RICADI_EINVAL;
  }
  return ricadi::aggregate(n, rowptr, col, bsize, blk_out);
}

int ricadi_host_sa_criterion(int nv, const int32_t* a_rp, const int32_t* a_ci, const double* a_v, double* rowsum_ratio_out,
                             double* skew_ratio_out, int* on_out) {
  if (nv < 1 || !a_rp || !a_ci || !a_v || !on_out) {
    ricadi::set_error("ricadi_host_sa_criterion: bad argument");
    return RICADI_EINVAL;
  }
  try {
    const ricadi::HostCsr A = ricadi::make_csr(nv, nv, a_rp, a_ci, a_v);
    double rs = -1.0, g = -1.0;
    *on_out = ricadi::sa_criterion(A, rs, g) ? 1 : 0;
    if (rowsum_ratio_out) *rowsum_ratio_out = rs;
    if (skew_ratio_out) *skew_ratio_out = g;
  } catch (...) {
    ricadi::set_error("ricadi_host_sa_criterion: exception");
    return RICADI_EINVAL;
  }
  return RICADI_OK;
}

// The operator of the three planning / tile entries below, and their common default for the smoothing weight
struct HostOperator {
  ricadi::HostCsr A, E, J, JT;
};
static double default_sa_omega(int np, const ricadi_opts& o) { return (np == 0 || o.bj_block != 32) ? 0.0 : 0.5; }

// Their argument check (rest_ok: what an entry requires beyond the operator) and the operator itself -- J empty
// without pressure; column ranges are not checked.  false: the error is set and names the entry.
static bool host_operator(const char* entry, int nv, int np, const int32_t* a_rp, const int32_t* a_ci,
                          const double* a_v, const int32_t* e_rp, const int32_t* e_ci, const double* e_v,
                          const int32_t* j_rp, const int32_t* j_ci, const double* j_v, bool rest_ok, HostOperator& op) {
  if (nv < 1 || np < 0 || !a_rp || !a_ci || !a_v || !e_rp || !e_ci || !e_v || (np > 0 && (!j_rp || !j_ci || !j_v)) ||
      !rest_ok) {
    ricadi::set_error(std::string(entry) + ": bad argument");
    return false;
  }
  const int32_t zero = 0;
  op.A = ricadi::make_csr(nv, nv, a_rp, a_ci, a_v);
  op.E = ricadi::make_csr(nv, nv, e_rp, e_ci, e_v);
  op.J = np > 0 ? ricadi::make_csr(np, nv, j_rp, j_ci, j_v) : ricadi::make_csr(0, nv, &zero, &zero, a_v);
  op.JT = ricadi::transpose(op.J);
  return true;
}

int ricadi_host_plan_levels(int nv, int np, const int32_t* a_rp, const int32_t* a_ci, const double* a_v,
                            const int32_t* e_rp, const int32_t* e_ci, const double* e_v, const int32_t* j_rp,
                            const int32_t* j_ci, const double* j_v, const ricadi_opts* opts, int32_t* out) {
  try {
    HostOperator op;
    if (!host_operator("ricadi_host_plan_levels", nv, np, a_rp, a_ci, a_v, e_rp, e_ci, e_v, j_rp, j_ci, j_v,
                       opts && out, op))
      return RICADI_EINVAL;
    const ricadi::HostSetup hs = ricadi::build_setup(op.A, op.E, op.J, op.JT, *opts, std::max(2, opts->max_levels),
                                                     default_sa_omega(np, *opts));
    out[0] = hs.kc == 0 ? 1 : hs.multilevel ? 3 : 2;
    out[1] = hs.kc;
    out[2] = hs.kcv;
    out[3] = hs.kcp;
    out[4] = hs.sa ? 1 : 0;
  } catch (...) {
    ricadi::set_error("ricadi_host_plan_levels: exception");
    return RICADI_EINVAL;
  }
  return RICADI_OK;
}

// One level of ricadi_host_plan_hierarchy and, through its Galerkin matrices, the levels below it: what
// ricadi_set_operator does, without the device
static void plan_level(const ricadi::HostCsr& A, const ricadi::HostCsr& E, const ricadi::HostCsr& J,
                       const ricadi::HostCsr& JT, const ricadi_opts& o, int levels, bool is_child,
                       std::vector<std::array<int32_t, 9>>& rows) {
  const ricadi::HostSetup hs =
      ricadi::build_setup_checked(A, E, J, JT, o, levels, is_child ? 0.0 : default_sa_omega(J.nrows, o));
  rows.push_back({hs.nv, hs.np, hs.kcv, hs.kcp, hs.agg_v, hs.agg_p, hs.multilevel ? 1 : 0,
                  hs.multilevel ? 0 : hs.kc, hs.sa ? 1 : 0});
  if (hs.multilevel)
    plan_level(hs.l1A, hs.l1E, hs.l1J, ricadi::transpose(hs.l1J), ricadi::child_opts(o, is_child),
               ricadi::child_levels(o, levels), true, rows);
}

int ricadi_host_plan_hierarchy(int nv, int np, const int32_t* a_rp, const int32_t* a_ci, const double* a_v,
                               const int32_t* e_rp, const int32_t* e_ci, const double* e_v, const int32_t* j_rp,
                               const int32_t* j_ci, const double* j_v, const ricadi_opts* opts, int32_t* nlevels_out,
                               int32_t* levels_out, int32_t* smoothed_out) {
  try {
    HostOperator op;
    if (!host_operator("ricadi_host_plan_hierarchy", nv, np, a_rp, a_ci, a_v, e_rp, e_ci, e_v, j_rp, j_ci, j_v,
                       opts && nlevels_out && levels_out && (opts->hierarchy == 0 || opts->hierarchy == 1), op))
      return RICADI_EINVAL;
    std::vector<std::array<int32_t, 9>> rows;
    plan_level(op.A, op.E, op.J, op.JT, *opts, ricadi::root_levels(*opts), false, rows);
    if ((int)rows.size() > RICADI_MAX_HIERARCHY_LEVELS) throw std::runtime_error("more levels than the rule allows");
    *nlevels_out = (int32_t)rows.size();
    std::fill(levels_out, levels_out + 8 * RICADI_MAX_HIERARCHY_LEVELS, 0);
    if (smoothed_out) std::fill(smoothed_out, smoothed_out + RICADI_MAX_HIERARCHY_LEVELS, 0);
    for (size_t l = 0; l < rows.size(); ++l) {
      std::copy(rows[l].begin(), rows[l].begin() + 8, levels_out + 8 * l);
      if (smoothed_out) smoothed_out[l] = rows[l][8];
    }
  } catch (...) {
    ricadi::set_error("ricadi_host_plan_hierarchy: exception");
    return RICADI_EINVAL;
  }
  return RICADI_OK;
}

int ricadi_host_saddle_tiles(int nv, int np, const int32_t* a_rp, const int32_t* a_ci, const double* a_v,
                             const int32_t* e_rp, const int32_t* e_ci, const double* e_v, const int32_t* j_rp,
                             const int32_t* j_ci, const double* j_v, const ricadi_opts* opts, int32_t* sizes_out,
                             int32_t* rows2, int32_t* rp2, int32_t* cols2, uint16_t* lidx, uint16_t* lidx_ms,
                             double* vAJ, double* vE, int32_t* perm, int32_t* s_rp, int32_t* s_ci, double* s_src) {
  try {
    HostOperator op;
    if (!host_operator("ricadi_host_saddle_tiles", nv, np, a_rp, a_ci, a_v, e_rp, e_ci, e_v, j_rp, j_ci, j_v,
                       opts && sizes_out, op))
      return RICADI_EINVAL;
    const ricadi::HostSetup hs = ricadi::build_setup_checked(
        op.A, op.E, op.J, op.JT, *opts, std::max(2, opts->max_levels), default_sa_omega(np, *opts));
    const ricadi::PrecondRecords r = ricadi::build_records(hs, op.J, op.JT, false, true);
    const int nb = hs.sb_nblk, mc = std::max(hs.sb_max_cols, 1);
    const size_t nnz = hs.s_ci.size();
    const int32_t sz[8] = {hs.n, nb, hs.sb_max_cols, hs.sb_max_nnz, (int32_t)nnz, r.sb_ok ? 1 : 0, r.ms_ok ? 1 : 0,
                           hs.nv};
    std::copy(sz, sz + 8, sizes_out);
    auto out = [](auto* dst, const auto& src, size_t cnt) {
      if (dst) std::copy(src.begin(), src.begin() + cnt, dst);
    };
    out(rows2, r.sb_rows2, (size_t)nb * 32);
    out(rp2, r.sb_rp2, (size_t)nb * 33);
    out(cols2, r.sb_cols2, (size_t)nb * mc);
    out(lidx, hs.sb_lidx, nnz);
    out(perm, hs.sb_perm, nnz);
    out(s_rp, hs.s_rp, (size_t)hs.n + 1);
    out(s_ci, hs.s_ci, nnz);
    if (s_src) {
      out(s_src, hs.s_srcA, nnz);
      out(s_src + nnz, hs.s_srcE, nnz);
      out(s_src + 2 * nnz, hs.s_srcJ, nnz);
    }
    if (r.ms_ok) {
      out(lidx_ms, r.sb_lidx_ms, nnz);
      out(vAJ, r.sbAJ, nnz);
      out(vE, r.sbE, nnz);
    }
  } catch (...) {
    ricadi::set_error("ricadi_host_saddle_tiles: exception");
    return RICADI_EINVAL;
  }
  return RICADI_OK;
}

int ricadi_host_deal(const double* shifts, int ns, int world, int32_t* owner_out) {
  if (!shifts || !owner_out || ns < 1 || world < 1) {
    ricadi::set_error("ricadi_host_deal: bad argument");
    return RICADI_EINVAL;
  }
  return ricadi::deal_shifts(shifts, ns, world, owner_out);
}

int ricadi_host_cauchy(const double* shifts, int g, double* rinv_out, double* cinv1_out) {
  if (!shifts || !rinv_out || !cinv1_out) {
    ricadi::set_error("ricadi_host_cauchy: bad argument");
    return RICADI_EINVAL;
  }
  int rc = ricadi::cauchy_data(shifts, g, rinv_out, cinv1_out);
  if (rc == RICADI_EBREAKDOWN)
    ricadi::set_error("ricadi_host_cauchy: Cauchy matrix not positive definite "
                      "(shifts must be distinct, negative and few)");
  return rc;
}

int ricadi_host_adi_window_width(const double* shifts, int ns, int first, int g, int* width_out) {
  if (!shifts || !width_out || ns < 1 || first < 0 || g < 1 || g > RICADI_MAX_GROUPS || g > ns) {
    ricadi::set_error("ricadi_host_adi_window_width: bad argument (first >= 0, 1 <= g <= min(ns, 16))");
    return RICADI_EINVAL;
  }
  for (int i = 0; i < ns; ++i)
    if (!(shifts[i] < 0.0)) {
      ricadi::set_error("ricadi_host_adi_window_width: ADI shifts must be negative");
      return RICADI_EINVAL;
    }
  *width_out = ricadi::adi_window_width(shifts, ns, first, g);
  return RICADI_OK;
}

int ricadi_host_cplx_proxy(double ar, double ai, double* alpha_pre_out) {
  if (!alpha_pre_out || !ricadi::cplx_shift_ok(ar, ai)) {
    ricadi::set_error("ricadi_host_cplx_proxy: a finite shift alpha != 0 with Re alpha <= 0 required");
    return RICADI_EINVAL;
  }
  *alpha_pre_out = ricadi::cplx_proxy(ar, ai);
  return RICADI_OK;
}

}  // extern "C"
