// solver_adi_pairs.inl -- low-rank Lyapunov ADI whose shift list holds complex-conjugate pairs:
// the real-arithmetic pair step of Benner, Kuerschner and Saak (2013) in the step form, the Woodbury form of its complex
// solve, and their entry points.  Part of ricadi_solver.hip (one translation unit; included there last).
//
// A list entry is a negative real shift -- one step, adi_real_step of solver_adi.inl -- or one complex number
// p = a + ib (a < 0, b != 0) that stands for the pair (p, conj p): ONE complex solve S(p) [V; *] = [W; 0] through
// cplx_solve gives both steps,
//   V1 = Re V + delta Im V,   Z <- [Z, gam V1, gam sqrt(delta^2 + 1) Im V],   W <- W - 4a E V1
// (gam = 2 sqrt(-a), delta = a / b), with a real residual factor behind the pair and none inside it.

#include <complex>
#include <cstdint>

#include "pair_smw.h"              // the host arithmetic of PairSolve: grouping, index map, capacitance LU, embedding

namespace {

// The complex solve of a pair step on the operator of the context, low-rank term included:
//   (S(p) - [U; 0] [V; 0]^T) [X; *] = [W; 0]
// for the m columns of W, packed with U (q > 0) into ng groups of mc complex columns.  With q > 0 the batch solves
// [X_W, X_U] = S(p)^-1 [W, U] and X = X_W + X_U (I - V^T X_U)^-1 V^T X_W (Sherman-Morrison-Woodbury): V^T X is the real
// gemm_tn on the real view, the q x q complex capacitance matrix is factorised on the host, the correction is the real
// gemm_nn with the complex q x m coefficients embedded as a real 2q x 2m matrix.  The true residual of the corrected
// columns -- complex product plus low-rank term -- decides on ONE refinement pass (a column above 10 gmres_tol).
struct PairSolve {
  ricadi_ctx* const c;
  const int m, q, mp;
  const PairGroups pg;            // the grouping of the mp columns and the index map (pair_smw.h)
  const int ng, mc, m2, n, nv;
  const size_t gs, gsr;           // group strides of the solution panels (n rows) and of the packed right-hand sides (nv)
  const GroupTab all;
  CplxCoefs cf{};
  std::vector<double> ht, hm, h16, bn2;
  std::vector<cdbl> cap, y;
  std::vector<int> piv;
  bool converged = true;          // of the last solve: every column of W met its bar
  double worst = 0.0;             // ... the largest true relative residual
  int iters = 0;                  // ... lockstep iterations (the slowest group's), refinement included
  // for ricadi_adi_pair_solve_dev (the driver reads none of them): whether the refinement pass ran, the largest
  // residual before it (`worst` is the one after it), the smallest pivot of the capacitance LU over max |cap_ij|, and
  // where to copy the groups as first solved -- ng gs doubles, the refinement's uncorrected D behind them
  bool refined = false;
  double worst_before = 0.0, min_pivot_rel = NAN;
  double* raw_out = nullptr;

  PairSolve(ricadi_ctx* ctx, int m_)
      : c(ctx), m(m_), q(std::max(ctx->q, 0)), mp(m_ + q), pg(mp), ng(pg.ng), mc(pg.mc), m2(2 * mc),
        n(ctx->n), nv(ctx->nv), gs((size_t)ctx->n * m2), gsr((size_t)ctx->nv * m2), all(all_groups(ng)) {
    c->pair_rhs.ensure(gsr * ng);
    c->pair_x.ensure(gs * ng);
    if (q > 0) {
      c->pair_rhs2.ensure(gs * ng);
      c->pair_d.ensure(gs * ng);
      c->pair_xu.ensure((size_t)n * 2 * q);
      c->pair_t.ensure((size_t)ng * q * m2);
      c->pair_m.ensure((size_t)ng * 2 * q * m2);
    }
  }

  // ht <- V^T D of the groups of D (q x m2 each, on the real view), on the host
  void vt(const double* D) {
    hipStream_t st = c->st;
    const size_t cnt = (size_t)ng * q * m2;
    HIPCHK(hipMemsetAsync(c->pair_t.p, 0, sizeof(double) * cnt, st));
    launch_gemm_tn_b(st, all, nv, q, m2, c->V.p, q, D, m2, gs, c->pair_t.p, m2, (size_t)q * m2);
    ht.resize(cnt);
    HIPCHK(hipMemcpyAsync(ht.data(), c->pair_t.p, sizeof(double) * cnt, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }

  // capacitance I - V^T X_U from the solutions in pair_x, factorised; X_U as one complex panel (n x q) in pair_xu
  void capacitance() {
    hipStream_t st = c->st;
    vt(c->pair_x.p);
    pair_capacitance(ht.data(), pg, m, q, cap);
    if (!pair_lu(cap, piv, q, &min_pivot_rel))
      throw HipError{"ADI pair step: the capacitance matrix I - V^T S(p)^-1 U of the low-rank term is numerically singular"};
    for (int g = 0; g < ng; ++g) {
      const auto [j0, j1] = pg.u_range(g, m, mp);
      if (j0 < j1)
        launch_copy_cols(st, n, 2 * (j1 - j0), c->pair_x.p + g * gs, m2, 2 * (j0 - g * mc), c->pair_xu.p, 2 * q,
                         2 * (j0 - m), 1.0);
    }
  }

  // D_W <- D_W + X_U (I - V^T X_U)^-1 V^T D_W on the groups of D
  void woodbury(double* D) {
    hipStream_t st = c->st;
    vt(D);
    pair_vtw(ht.data(), pg, m, q, y);
    pair_lu_solve(cap, piv, q, y, m);
    pair_embed(y, pg, m, q, hm);     // complex y (q x m) as the real 2q x m2 matrix of every group
    HIPCHK(hipMemcpyAsync(c->pair_m.p, hm.data(), sizeof(double) * hm.size(), hipMemcpyHostToDevice, st));
    launch_gemm_nn_bp(st, all, n, 2 * q, m2, same_ptr((const double*)c->pair_xu.p), 2 * q, c->pair_m.p, m2,
                      (size_t)2 * q * m2, D, m2, gs, 1.0, 1.0);
    HIPCHK(hipStreamSynchronize(st));     // hm is reused
  }

  // squared column norms of the groups of `panel` (rows x m2, stride gsp) into h16 (16 per group, column cc at 2 cc)
  void norms2(const double* panel, int rows, size_t gsp) {
    hipStream_t st = c->st;
    ricadi_ctx::CplxWork& k = c->cw;
    launch_cplx_dots(st, all, rows, m2, 0, 1, nullptr, 0, 0, panel, gsp, k.partial.p, k.nvec + 1, k.nrm2.p, 16);
    h16.resize((size_t)ng * 16);
    HIPCHK(hipMemcpyAsync(h16.data(), k.nrm2.p, sizeof(double) * ng * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }

  // cw.r <- [W; 0] - (S(p) - U V^T) X on all groups; returns the largest relative residual among the columns of W
  double residual() {
    hipStream_t st = c->st;
    ricadi_ctx::CplxWork& k = c->cw;
    cplx_product(c, all, cf, m2, c->pair_x.p, gs, k.r.p, gs);
    launch_cplx_axpby(st, all, gsr, m2, -1.0, k.r.p, gs, 1.0, nullptr, c->pair_rhs.p, gsr, k.r.p, gs);
    if (n > nv)
      launch_cplx_axpby(st, all, gs - gsr, m2, -1.0, k.r.p + gsr, gs, 0.0, nullptr, nullptr, 0, k.r.p + gsr, gs);
    vt(c->pair_x.p);
    launch_gemm_nn_bp(st, all, nv, q, m2, same_ptr((const double*)c->U.p), q, c->pair_t.p, m2, (size_t)q * m2, k.r.p,
                      m2, gs, 1.0, 1.0);
    norms2(k.r.p, n, gs);
    double w = 0.0;
    for (int j = 0; j < m; ++j) {
      const size_t at = (size_t)pg.group_of(j) * 16 + 2 * pg.col_of(j);
      const double b2 = bn2[at], r2 = h16[at];
      const double rr = b2 > 0.0 ? std::sqrt(r2 / b2) : 0.0;
      w = std::isfinite(rr) ? std::max(w, rr) : INFINITY;
    }
    return w;
  }

  // pair_x <- the solution groups at p = a + ib for the residual factor dW (nv x m)
  void solve(double a, double b, const double* dW) {
    hipStream_t st = c->st;
    const double tol = c->opts.gmres_tol;
    for (int g = 0; g < ng; ++g) {
      cf.ar[g] = a;
      cf.ai[g] = b;
      cf.beta[g] = 1.0;
    }
    launch_adi_pair_pack(st, nv, m, q, ng, mc, dW, q > 0 ? c->U.p : nullptr, c->pair_rhs.p, gsr);
    const CplxResult r = cplx_solve(c, ng, cf, c->pair_rhs.p, gsr, mc, c->pair_x.p);
    iters = *std::max_element(r.iters.begin(), r.iters.end());
    refined = false;
    if (q == 0) {
      converged = r.converged;
      worst = 0.0;
      for (int j = 0; j < m; ++j) worst = std::max(worst, r.relres[(size_t)pg.group_of(j) * mc + pg.col_of(j)]);
      worst_before = worst;
      return;
    }
    if (raw_out) HIPCHK(hipMemcpyAsync(raw_out, c->pair_x.p, sizeof(double) * gs * ng, hipMemcpyDeviceToDevice, st));
    norms2(c->pair_rhs.p, nv, gsr);
    bn2 = h16;
    capacitance();
    woodbury(c->pair_x.p);
    worst = worst_before = residual();
    if (worst > 10.0 * tol) {
      refined = true;
      // one pass on the residual equation: S(p) D = r for the columns of W (those of U are zeroed), corrected alike
      ++c->pair_info[2];
      ricadi_ctx::CplxWork& k = c->cw;
      // The right-hand side is the whole residual, pressure rows included: J (X_W + X_U y) carries the solves'
      // pressure residuals times the same y as the velocity rows do, and a pass on the velocity rows alone leaves
      // that share where it is.
      HIPCHK(hipMemcpyAsync(c->pair_rhs2.p, k.r.p, sizeof(double) * gs * ng, hipMemcpyDeviceToDevice, st));
      for (int g = 0; g < ng; ++g) {
        const int c0 = pg.w_cols(g, m);
        if (c0 < mc)
          HIPCHK(hipMemset2DAsync(c->pair_rhs2.p + g * gs + 2 * c0, sizeof(double) * m2, 0,
                                  sizeof(double) * 2 * (mc - c0), n, st));
      }
      CplxResult r2;
      {
        Restore<double> keep_tol(c->opts.gmres_tol);
        c->opts.gmres_tol = std::min(0.5, std::max(1e-14, 0.5 * tol / worst));
        r2 = cplx_solve(c, ng, cf, c->pair_rhs2.p, gs, mc, c->pair_d.p, n);
      }
      iters += *std::max_element(r2.iters.begin(), r2.iters.end());
      if (raw_out)
        HIPCHK(hipMemcpyAsync(raw_out + gs * ng, c->pair_d.p, sizeof(double) * gs * ng, hipMemcpyDeviceToDevice, st));
      woodbury(c->pair_d.p);
      launch_cplx_axpby(st, all, gs, m2, 1.0, c->pair_x.p, gs, 1.0, nullptr, c->pair_d.p, gs, c->pair_x.p, gs);
      worst = residual();
    }
    converged = worst <= 10.0 * tol;
  }
};

// The step-form driver for a list with pair entries: (sre[e], sim[e]) is a real shift where sim[e] == 0, else a pair.
// Conventions as lyap_adi_dev: dW (nv x m) is overwritten by the final residual factor, the blocks go to c->Z from
// column c->zc on.  AdiStop counts the list in steps (two per pair): a pair records its two blocks in order, both with
// the residual behind the pair, and the rules are read after the second one -- a pair is never split, neither by a rule
// that fires on its first block nor by adi_max_steps (one step left before a pair ends the iteration there).
AdiStats lyap_adi_pairs_dev(ricadi_ctx* c, const double* sre, const double* sim, int ne, double* dW, int m,
                            const ricadi_adi_params& prm) {
  AdiStats stt;
  Restore<int> keep_rec(c->rec_depth);
  c->rec_depth = std::max(c->rec_user_depth, adi_recycle_depth(c));
  c->adi_res_hist.clear();
  c->adi_stop_rule = RICADI_STOP_MAX_STEPS;
  c->adi_ran = true;
  hipStream_t st = c->st;
  int ns = 0;
  for (int e = 0; e < ne; ++e) ns += sim[e] != 0.0 ? 2 : 1;
  ensure_work(c, m);
  // per-shift data up front, as lyap_adi_dev: the real shifts and the proxies of the pairs in one batched factorisation
  std::vector<double> first;
  for (int e = 0, reach = 0; e < ne && reach < prm.adi_max_steps; ++e) {
    const double p = sim[e] != 0.0 ? cplx_proxy(sre[e], sim[e]) : sre[e];
    if (std::find(first.begin(), first.end(), p) == first.end()) first.push_back(p);
    reach += sim[e] != 0.0 ? 2 : 1;
  }
  setup_and_project(c, first.data(), (int)first.size(), prm.project_w != 0, dW, m);
  const long it0 = c->total_iters;
  int zc_last = c->zc;
  AdiStop stop(ns, prm.adi_newZ_reltol, prm.adi_res_reltol, prm.adi_max_steps, adi_res_wanted(c, prm));
  const int mm = m * m;
  double* hg = stop.res_on ? adi_res_begin(c, dW, m) : nullptr;
  PairSolve ps(c, m);
  c->sweep_t.ensure((size_t)c->nv * m);
  c->pair_part.ensure((size_t)2 * adi_pair_num_blocks(c->nv));
  c->pair_nrm.ensure(2);
  auto residual_of_step = [&]() {
    if (stop.res_rhs < 0.0) stop.res_rhs = gram_block_fro(hg, m, m, 0);
    return gram_block_fro(hg + mm, m, m, 0);
  };
  int steps = 0;
  for (int e = 0; steps < prm.adi_max_steps; e = (e + 1) % ne) {
    const double a = sre[e], b = sim[e];
    int rule = RICADI_STOP_MAX_STEPS;
    if (b == 0.0) {
      double n2 = 0.0, wf = 0.0;
      GmresResult r = adi_real_step(c, a, dW, m, hg, n2);
      if (!r.converged) {
        stt.nonconverged++;
        stt.worst_relres = std::max(stt.worst_relres, r.max_relres);
      }
      if (stop.res_on) wf = residual_of_step();
      const AdiStop::Verdict v = stop.record(steps, n2, stop.res_on ? &wf : nullptr);
      if (stop.res_on) c->adi_res_hist.push_back(v.res);
      c->zc += m;
      steps += 1;
      stt.rel = v.rel;
      rule = v.rule;
      if (prm.verbose)
        fprintf(stderr, "[ricadi] ADI step %3d: shift %10.3e rel new Z %9.3e gmres its %d\n", steps, a, stt.rel, r.iters);
    } else {
      if (steps + 2 > prm.adi_max_steps) break;      // a pair is never split
      ps.solve(a, b, dW);
      ++c->pair_info[0];
      c->pair_info[1] += ps.iters;
      if (!ps.converged) {
        ++c->pair_info[3];
        stt.nonconverged++;
        stt.worst_relres = std::max(stt.worst_relres, ps.worst);
        if (prm.verbose)
          fprintf(stderr, "[ricadi] ADI pair at %g%+gi: the complex solve stopped at relres %.2e\n", a, b, ps.worst);
      }
      const PairCoefs pc(a, b);
      launch_adi_pair_blocks(st, c->nv, m, ps.mc, pc.delta, pc.gam, pc.gam2, c->pair_x.p, ps.gs, c->Z.p, c->zld, c->zc,
                             c->sweep_t.p, c->pair_part.p, c->pair_nrm.p);
      // W <- W - 4a E V1
      launch_spmm(st, c->nv, c->E.rp.p, c->E.ci.p, c->E.v.p, c->sweep_t.p, m, nullptr, dW, m, dW, m, -4.0 * a, 1.0,
                  nullptr, m);
      HIPCHK(hipMemcpyAsync(c->h_resid, c->pair_nrm.p, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
      if (hg) adi_res_fetch(c, dW, m, hg);
      HIPCHK(hipStreamSynchronize(st));
      const double n2a = c->h_resid[0], n2b = c->h_resid[1];
      double wf = 0.0;
      if (stop.res_on) wf = residual_of_step();
      const AdiStop::Verdict v1 = stop.record(steps, n2a, stop.res_on ? &wf : nullptr);
      const AdiStop::Verdict v2 = stop.record(steps + 1, n2b, stop.res_on ? &wf : nullptr);
      if (stop.res_on) {
        c->adi_res_hist.push_back(v1.res);
        c->adi_res_hist.push_back(v2.res);
      }
      c->zc += 2 * m;
      steps += 2;
      stt.rel = v2.rel;
      // the reference's rule comes first, on whichever block it fired
      rule = (v1.rule == RICADI_STOP_NEWZ || v2.rule == RICADI_STOP_NEWZ) ? RICADI_STOP_NEWZ : v2.rule;
      if (prm.verbose)
        fprintf(stderr, "[ricadi] ADI steps %3d, %3d: pair %10.3e%+.3ei rel new Z %9.3e, %9.3e complex gmres its %d\n",
                steps - 1, steps, a, b, v1.rel, v2.rel, ps.iters);
    }
    stt.shift_solves++;
    stt.steps = steps;
    if (rule != RICADI_STOP_MAX_STEPS) {
      c->adi_stop_rule = rule;
      break;
    }
    if (prm.compress_cols > 0 && c->zc - zc_last >= prm.compress_cols) {
      factor_recompress(c);
      zc_last = c->zc;
    }
  }
  stt.gmres_iters = c->total_iters - it0;
  gram_norms(c, dW, c->nv, m, &stt.res_fro, nullptr);
  return stt;
}

}  // namespace

extern "C" {

int ricadi_lyap_adi_cplx(ricadi_ctx* c, const double* shifts_re, const double* shifts_im, int ns, const double* W, int m,
                         const ricadi_adi_params* prm, double* Z_out, int* c_out, double* stats_out) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(shifts_re && shifts_im && ns > 0 && W && prm, RICADI_EINVAL, "bad argument");
  bool pairs = false;
  for (int i = 0; i < ns; ++i) {
    REQUIRE(std::isfinite(shifts_re[i]) && std::isfinite(shifts_im[i]) && shifts_re[i] < 0.0, RICADI_EINVAL,
            "ADI shifts must be finite with a negative real part");
    pairs = pairs || shifts_im[i] != 0.0;
  }
  REQUIRE(prm->adi_max_steps > 0, RICADI_EINVAL, "adi_max_steps must be positive");
  std::fill(c->pair_info, c->pair_info + 4, (int64_t)0);
  // a real list is ricadi_lyap_adi's, sweep form included
  if (!pairs) return ricadi_lyap_adi(c, shifts_re, ns, W, m, prm, Z_out, c_out, stats_out);
  REQUIRE(!sharded(c), RICADI_EINVAL, "complex shift pairs are not taken on a context with an exchange (ricadi_set_exchange)");
  REQUIRE(m + std::max(c->q, 0) <= RICADI_MAX_M, RICADI_EINVAL,
          "complex shift pairs: panel width plus low-rank width must be at most 128");
  return lyap_adi_entry(c, W, m, prm, Z_out, c_out, stats_out,
                        [&](double* dW) { return lyap_adi_pairs_dev(c, shifts_re, shifts_im, ns, dW, m, *prm); });
}

int ricadi_adi_pair_blocks_dev(ricadi_ctx* c, int ng, int mc, int m, double ar, double ai, const double* dX, double* dZ,
                               int ldz, int zc, double* dV1, double* norms2_out) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(ng >= 1 && ng <= RICADI_MAX_GROUPS, RICADI_EINVAL, "1 <= ng <= 16 required");
  REQUIRE(mc >= 1 && mc <= 8, RICADI_EINVAL, "complex panels have 1 <= mc <= 8 columns");
  REQUIRE(m >= 1 && m <= ng * mc, RICADI_EINVAL, "1 <= m <= ng * mc required");
  REQUIRE(std::isfinite(ar) && std::isfinite(ai) && ar < 0.0 && ai != 0.0, RICADI_EINVAL,
          "a pair needs a finite shift with Re < 0 and Im != 0");
  REQUIRE(dX && dZ && dV1 && norms2_out, RICADI_EINVAL, "NULL argument");
  REQUIRE(((uintptr_t)dX & 15) == 0, RICADI_EINVAL, "dX must be 16-byte aligned");
  REQUIRE(zc >= 0 && ldz >= zc + 2 * m, RICADI_EINVAL, "ldz >= zc + 2 m required");
  API_BEGIN_ON(c)
  const PairCoefs pc(ar, ai);
  c->pair_part.ensure((size_t)2 * adi_pair_num_blocks(c->nv));
  c->pair_nrm.ensure(2);
  launch_adi_pair_blocks(c->st, c->nv, m, mc, pc.delta, pc.gam, pc.gam2, dX, (size_t)c->n * 2 * mc, dZ, ldz, zc, dV1,
                         c->pair_part.p, c->pair_nrm.p);
  HIPCHK(hipMemcpyAsync(norms2_out, c->pair_nrm.p, sizeof(double) * 2, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

int ricadi_adi_pair_solve_dev(ricadi_ctx* c, double ar, double ai, const double* dW, int m, int what_mask, double* dRaw,
                              double* dX, double* dRhs, double* report) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(std::isfinite(ar) && std::isfinite(ai) && ar < 0.0 && ai != 0.0, RICADI_EINVAL,
          "a pair needs a finite shift with Re < 0 and Im != 0");
  REQUIRE(dW && report, RICADI_EINVAL, "NULL argument");
  REQUIRE(m >= 1 && m + std::max(c->q, 0) <= RICADI_MAX_M, RICADI_EINVAL,
          "pair solve: m >= 1 and panel width plus low-rank width at most 128 required");
  REQUIRE(what_mask >= 0 && what_mask < 16, RICADI_EINVAL, "what_mask has four bits");
  REQUIRE(!(what_mask & 1) || (dRhs && ((uintptr_t)dRhs & 15) == 0), RICADI_EINVAL, "dRhs must be 16-byte aligned");
  REQUIRE(!(what_mask & 2) || dRaw, RICADI_EINVAL, "NULL dRaw");
  REQUIRE(!(what_mask & 4) || dX, RICADI_EINVAL, "NULL dX");
  REQUIRE(!sharded(c), RICADI_EINVAL, "complex shift pairs are not taken on a context with an exchange (ricadi_set_exchange)");
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  int64_t keep_info[4];
  std::copy(c->pair_info, c->pair_info + 4, keep_info);
  ensure_work(c, m);
  PairSolve ps(c, m);
  std::fill(report, report + 8, 0.0);
  report[0] = ps.ng;
  report[1] = ps.mc;
  report[7] = NAN;
  // the pack kernel straight into the caller's groups: what it writes beside them shows there
  if (what_mask & 1)
    launch_adi_pair_pack(st, ps.nv, m, ps.q, ps.ng, ps.mc, dW, ps.q > 0 ? c->U.p : nullptr, dRhs, ps.gsr);
  if (!(what_mask & 8)) {
    const double proxy = cplx_proxy(ar, ai);
    setup_and_project(c, &proxy, 1, false, nullptr, m);
    if ((what_mask & 2) && ps.q > 0) ps.raw_out = dRaw;
    try {
      ps.solve(ar, ai, dW);
    } catch (...) {
      std::copy(keep_info, keep_info + 4, c->pair_info);
      report[2] = ps.iters;
      report[7] = ps.min_pivot_rel;
      (void)hipStreamSynchronize(st);
      throw;
    }
    std::copy(keep_info, keep_info + 4, c->pair_info);
    report[2] = ps.iters;
    report[3] = ps.refined ? 1.0 : 0.0;
    report[4] = ps.worst_before;
    report[5] = ps.worst;
    report[6] = ps.converged ? 1.0 : 0.0;
    report[7] = ps.min_pivot_rel;
    if (what_mask & 4)
      HIPCHK(hipMemcpyAsync(dX, c->pair_x.p, sizeof(double) * ps.gs * ps.ng, hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  API_END
}

int ricadi_adi_pair_info(ricadi_ctx* c, int64_t out[4]) {
  REQUIRE(c && out, RICADI_EINVAL, "NULL argument");
  std::copy(c->pair_info, c->pair_info + 4, out);
  return RICADI_OK;
}

}  // extern "C"
