// solver_cplx.inl -- saddle systems at complex shifts: the complex product, the CGS2 step and the
// right-preconditioned flexible GMRES that runs all groups of a batch in lockstep, and their entry points.
// Part of ricadi_solver.hip (one translation unit; included there last).
//
// Everything complex lives here and in ricadi_cplx.hip; the real preconditioner cycle is used as it is, on the real
// view of a panel (width 2 mc) at the real proxy shift of every group.

namespace {

// the table of the listed group ids
GroupTab cplx_table(const std::vector<int>& ids) {
  GroupTab t{};
  t.ng = (int)ids.size();
  for (int i = 0; i < t.ng; ++i) t.gid[i] = ids[i];
  return t;
}

// Workspaces for ng groups of 16 real columns and nvec basis vectors per CGS2 step; basis: also the Krylov vectors and
// the Z_j of a solve with the context's restart length.  Buffers only grow.
void cplx_ensure_work(ricadi_ctx* c, int ng, int nvec, bool basis) {
  ricadi_ctx::CplxWork& k = c->cw;
  k.groups = std::max(k.groups, ng);
  k.nvec = std::max(k.nvec, nvec);
  k.n = c->n;
  const size_t G = (size_t)k.groups, gs = (size_t)c->n * 16, rows = (size_t)k.nvec + 1;
  k.w.ensure(G * gs);
  k.r.ensure(G * gs);
  k.b.ensure(G * gs);
  k.partial.ensure(G * cplx_num_blocks(c->n) * rows * 16);
  k.h1.ensure(G * rows * 16);
  k.h2.ensure(G * rows * 16);
  k.hout.ensure(G * rows * 16);
  k.nrm2.ensure(G * 16);
  k.scale.ensure(G * 16);
  k.bnorm.ensure(G * 8);
  k.resid.ensure(G * 8);
  if (basis) {
    const size_t rs = (size_t)c->opts.gmres_restart;
    k.basis = true;
    k.V.ensure((rs + 1) * G * gs);
    k.Zb.ensure(rs * G * gs);
    k.Hm.ensure(G * 8 * rs * (rs + 1) * 2);
    k.cs.ensure(G * 8 * rs);
    k.sn.ensure(G * 8 * rs * 2);
    k.gv.ensure(G * 8 * (rs + 1) * 2);
    k.y.ensure(G * rs * 16);
  }
}

CplxCoefs cplx_coefs(int ng, const double* ars, const double* ais, const double* betas) {
  CplxCoefs cf{};
  for (int g = 0; g < ng; ++g) {
    cf.ar[g] = ars[g];
    cf.ai[g] = ais[g];
    cf.beta[g] = betas[g];
  }
  return cf;
}

// y_g = S(alpha_g, beta_g) x_g for the groups of tab: the tiled form where the operator has the multi-shift tiles,
// the CSR form for every other operator.  Returns the form (1 tiled, 2 CSR).
int cplx_product(ricadi_ctx* c, const GroupTab& tab, const CplxCoefs& cf, int m2, const double* x, size_t gsx, double* y,
                 size_t gsy) {
  const bool tiled = c->ms_ok && saddle_tiled(c, 16) && cplx_spmm_tiled_ok(c->sb_max_cols, (size_t)c->n);
  if (tiled)
    launch_cplx_spmm_tiled(c->st, tab, cf, c->sb_nblk, c->sb_rows2.p, c->sb_rp2.p, c->sb_cols2.p, c->sb_lidx_ms.p,
                           c->sbAJ.p, c->sbE.p, x, gsx, y, gsy, m2, c->sb_max_cols);
  else
    launch_cplx_spmm_csr(c->st, tab, cf, c->n, c->s_rp.p, c->s_ci.p, c->srcA.p, c->srcE.p, c->srcJ.p, x, gsx, y, gsy, m2);
  return tiled ? 1 : 2;
}

// One CGS2 step: w against the nvec basis panels (two passes, coefficients added), its norm, the unit vector into
// `unit` (which may be w).  Leaves the coefficient column in cw.hout (rows of 16, group stride (ldp) * 16).
void cplx_orth(ricadi_ctx* c, const GroupTab& tab, int m2, int nvec, const double* V, size_t vstride, size_t gsv,
               double* w, size_t gsw, int ldp, double* unit, size_t gsu) {
  ricadi_ctx::CplxWork& k = c->cw;
  hipStream_t st = c->st;
  const size_t gsh = (size_t)ldp * 16;
  const GroupInts nv = same_int(nvec);
  double* const pass[2] = {k.h1.p, k.h2.p};
  for (double* h : pass) {
    launch_cplx_dots(st, tab, c->n, m2, nvec, 0, V, vstride, gsv, w, gsw, k.partial.p, ldp, h, gsh);
    launch_cplx_update(st, tab, nv, c->n, m2, V, vstride, gsv, h, gsh, -1.0, w, gsw);
  }
  launch_cplx_dots(st, tab, c->n, m2, 0, 1, nullptr, 0, 0, w, gsw, k.partial.p, ldp, k.nrm2.p, 16);
  launch_cplx_orth_finish(st, tab, nvec, k.h1.p, k.h2.p, k.nrm2.p, gsh, k.hout.p, k.scale.p);
  launch_cplx_axpby(st, tab, (size_t)c->n * m2, m2, 0.0, nullptr, 0, 1.0, k.scale.p, w, gsw, unit, gsu);
}

// The proxy shifts of a batch, their per-shift data (groups with the same proxy share one entry) and the real batch
// of width 2 mc the preconditioner cycle runs on
struct CplxPrecond {
  std::vector<ShiftData*> sds;
  Batch bt;
  CycleForm pf;
  CplxPrecond(ricadi_ctx* c, int ng, const CplxCoefs& cf, int m2) : sds(ng) {
    std::vector<double> ua, ub;
    std::vector<int> slot(ng);
    for (int g = 0; g < ng; ++g) {
      const double ap = cplx_proxy(cf.ar[g], cf.ai[g]);
      int s = 0;
      while (s < (int)ua.size() && !(ua[s] == ap && ub[s] == cf.beta[g])) ++s;
      if (s == (int)ua.size()) {
        ua.push_back(ap);
        ub.push_back(cf.beta[g]);
      }
      slot[g] = s;
    }
    std::vector<ShiftData*> us(ua.size());
    get_shifts(c, ua.data(), ub.data(), (int)ua.size(), us.data());
    for (int g = 0; g < ng; ++g) sds[g] = us[slot[g]];
    ensure_work(c, m2, ng, 0);         // the cycle's own panels (coarse residual, pressure part, ...)
    bt = make_batch(c, sds.data(), ng, m2);
    pf = cycle_form(c, m2, bt.blocks16, bt.gs, false, false);
  }
};

struct CplxResult {
  std::vector<int> iters;
  std::vector<double> relres;   // ng x mc, true residuals
  bool converged = true;
};

// S(alpha_g, beta_g) X_g = [R_g; 0] for ng groups in lockstep: flexible GMRES(restart) from zero, Z_j kept in FP64.
CplxResult cplx_solve(ricadi_ctx* c, int ng, const CplxCoefs& cf, const double* dR, size_t gsr, int mc, double* dX) {
  hipStream_t st = c->st;
  const int m2 = 2 * mc, n = c->n, restart = c->opts.gmres_restart, maxit = c->opts.gmres_maxit;
  const double tol = c->opts.gmres_tol;
  const size_t gs = (size_t)n * m2, vstride = gs * ng;
  CplxPrecond pc(c, ng, cf, m2);
  cplx_ensure_work(c, ng, restart + 1, true);
  ricadi_ctx::CplxWork& k = c->cw;
  const int ldp = k.nvec + 1;
  const size_t gsh = (size_t)ldp * 16;
  const GroupTab all = all_groups(ng);
  // b_g = [R_g; 0], x_g = 0, r_g = b_g
  HIPCHK(hipMemsetAsync(k.b.p, 0, sizeof(double) * gs * ng, st));
  for (int g = 0; g < ng; ++g)
    HIPCHK(hipMemcpyAsync(k.b.p + g * gs, dR + g * gsr, sizeof(double) * c->nv * m2, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemsetAsync(dX, 0, sizeof(double) * gs * ng, st));
  HIPCHK(hipMemcpyAsync(k.r.p, k.b.p, sizeof(double) * gs * ng, hipMemcpyDeviceToDevice, st));
  std::vector<double> h16((size_t)ng * 16), h8((size_t)ng * 8), bn((size_t)ng * 8, 0.0);
  auto norms = [&](const GroupTab& tab, const double* panel) {
    launch_cplx_dots(st, tab, n, m2, 0, 1, nullptr, 0, 0, panel, gs, k.partial.p, ldp, k.nrm2.p, 16);
    HIPCHK(hipMemcpyAsync(h16.data(), k.nrm2.p, sizeof(double) * ng * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  };
  norms(all, k.b.p);
  for (int g = 0; g < ng; ++g)
    for (int col = 0; col < mc; ++col) bn[g * 8 + col] = std::sqrt(h16[g * 16 + 2 * col]);
  HIPCHK(hipMemcpyAsync(k.bnorm.p, bn.data(), sizeof(double) * ng * 8, hipMemcpyHostToDevice, st));

  CplxResult res;
  res.iters.assign(ng, 0);
  res.relres.assign((size_t)ng * mc, 0.0);
  std::vector<int> act(ng);
  std::iota(act.begin(), act.end(), 0);
  bool first = true;
  while (true) {
    GroupTab tab = cplx_table(act);
    if (!first) {   // the true residual r = b - S x of the groups still iterating
      cplx_product(c, tab, cf, m2, dX, gs, k.r.p, gs);
      launch_cplx_axpby(st, tab, gs, m2, -1.0, k.r.p, gs, 1.0, nullptr, k.b.p, gs, k.r.p, gs);
    }
    first = false;
    norms(tab, k.r.p);
    std::vector<int> keep;
    for (int g : act) {
      double worst = 0.0;
      for (int col = 0; col < mc; ++col) {
        const double b0 = bn[g * 8 + col];
        const double rr = b0 > 0.0 ? std::sqrt(h16[g * 16 + 2 * col]) / b0 : 0.0;
        res.relres[(size_t)g * mc + col] = rr;
        worst = std::isfinite(rr) ? std::max(worst, rr) : INFINITY;
      }
      if (!(worst <= tol)) {
        if (res.iters[g] < maxit) keep.push_back(g);
        else res.converged = false;
      }
    }
    act = keep;
    if (act.empty()) break;
    tab = cplx_table(act);
    // cycle start: v_0 = r / ||r||
    launch_cplx_gmres_start(st, tab, mc, restart, k.nrm2.p, k.bnorm.p, k.gv.p, k.scale.p, k.resid.p);
    launch_cplx_axpby(st, tab, gs, m2, 0.0, nullptr, 0, 1.0, k.scale.p, k.r.p, gs, k.V.p, gs);
    std::vector<int> cyc = act;
    GroupInts ks = same_int(0);
    for (int j = 0; j < restart && !cyc.empty(); ++j) {
      const GroupTab ct = cplx_table(cyc);
      double* vj = k.V.p + (size_t)j * vstride;
      double* zj = k.Zb.p + (size_t)j * vstride;
      pc.bt.tab = ct;
      precond_apply(c, pc.bt, pc.pf, CycleIO{vj, gs, nullptr, zj, nullptr, 0});
      cplx_product(c, ct, cf, m2, zj, gs, k.w.p, gs);
      cplx_orth(c, ct, m2, j + 1, k.V.p, vstride, gs, k.w.p, gs, ldp, k.V.p + (size_t)(j + 1) * vstride, gs);
      launch_cplx_gmres_hess(st, ct, mc, j, restart, k.hout.p, gsh, k.Hm.p, k.cs.p, k.sn.p, k.gv.p, k.bnorm.p, k.resid.p);
      HIPCHK(hipMemcpyAsync(h8.data(), k.resid.p, sizeof(double) * ng * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      std::vector<int> on;
      for (int g : cyc) {
        ++res.iters[g];
        ks.v[g] = j + 1;
        bool conv = true;
        for (int col = 0; col < mc; ++col) conv = conv && h8[g * 8 + col] <= tol;
        if (!conv && res.iters[g] < maxit) on.push_back(g);
      }
      cyc = on;
    }
    // cycle end: R y = g, x += Z y
    launch_cplx_gmres_backsolve(st, tab, ks, mc, restart, k.Hm.p, k.gv.p, k.y.p, (size_t)restart * 16);
    launch_cplx_update(st, tab, ks, n, m2, k.Zb.p, vstride, gs, k.y.p, (size_t)restart * 16, 1.0, dX, gs);
  }
  HIPCHK(hipStreamSynchronize(st));
  c->total_solves += ng;
  for (int g = 0; g < ng; ++g) c->total_iters += res.iters[g];
  return res;
}

}  // namespace

extern "C" {

// what every complex entry checks first (in front of the try: it returns)
static int cplx_check(const ricadi_ctx* c, int ng, int mc, const double* ars, const double* ais, const double* betas) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(ng >= 1 && ng <= RICADI_MAX_GROUPS, RICADI_EINVAL, "1 <= ng <= 16 required");
  REQUIRE(mc >= 1 && mc <= 8, RICADI_EINVAL, "complex panels have 1 <= mc <= 8 columns");
  REQUIRE(ars && ais && betas, RICADI_EINVAL, "NULL argument");
  for (int g = 0; g < ng; ++g)
    REQUIRE(cplx_shift_ok(ars[g], ais[g]) && std::isfinite(betas[g]), RICADI_EINVAL,
            "complex shift: finite, alpha != 0 and Re alpha <= 0 required");
  REQUIRE(c->q == 0, RICADI_EINVAL, "the complex path takes no low-rank term (ricadi_set_lowrank with q = 0 first)");
  return RICADI_OK;
}

int ricadi_shift_solve_cplx_batch_dev(ricadi_ctx* c, int ng, const double* alphas_re, const double* alphas_im,
                                      const double* betas, const double* dR, int64_t r_stride, int mc, double* dX,
                                      int* iters_out, double* relres_out) {
  if (int rc = cplx_check(c, ng, mc, alphas_re, alphas_im, betas)) return rc;
  REQUIRE(dR && dX, RICADI_EINVAL, "NULL argument");
  REQUIRE(r_stride == 0 || r_stride >= (int64_t)c->nv * mc, RICADI_EINVAL, "bad r_stride");
  bool ok = true;
  API_BEGIN_ON(c)
  const CplxResult r = cplx_solve(c, ng, cplx_coefs(ng, alphas_re, alphas_im, betas), dR, (size_t)r_stride * 2, mc, dX);
  if (iters_out) std::copy(r.iters.begin(), r.iters.end(), iters_out);
  if (relres_out) std::copy(r.relres.begin(), r.relres.end(), relres_out);
  ok = r.converged;
  if (!ok) ricadi::set_error("complex shift solve: a group stopped at gmres_maxit");
  API_END_STATUS(ok ? RICADI_OK : RICADI_ENOCONV)
}

int ricadi_op_apply_cplx_batch_dev(ricadi_ctx* c, int ng, const double* alphas_re, const double* alphas_im,
                                   const double* betas, const double* dX, int64_t x_stride, int mc, const int32_t* active,
                                   int nactive, double* dY, int64_t y_stride, int* variant_out) {
  if (int rc = cplx_check(c, ng, mc, alphas_re, alphas_im, betas)) return rc;
  REQUIRE(dX && dY, RICADI_EINVAL, "NULL argument");
  const int64_t nm = (int64_t)c->n * mc;
  REQUIRE(x_stride >= nm && y_stride >= nm, RICADI_EINVAL, "bad x_stride / y_stride");
  std::vector<int> ids;
  if (int rc = active_ids(active, nactive, ng, ids)) return rc;
  API_BEGIN_ON(c)
  const GroupTab tab = active ? cplx_table(ids) : all_groups(ng);
  const int variant = cplx_product(c, tab, cplx_coefs(ng, alphas_re, alphas_im, betas), 2 * mc, dX, (size_t)x_stride * 2,
                                   dY, (size_t)y_stride * 2);
  HIPCHK(hipStreamSynchronize(c->st));
  if (variant_out) *variant_out = variant;
  API_END
}

int ricadi_cplx_orth_dev(ricadi_ctx* c, int ng, int mc, int nvec, const double* dV, int64_t v_stride, int64_t g_stride,
                         double* dW, double* dH) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(ng >= 1 && ng <= RICADI_MAX_GROUPS, RICADI_EINVAL, "1 <= ng <= 16 required");
  REQUIRE(mc >= 1 && mc <= 8, RICADI_EINVAL, "complex panels have 1 <= mc <= 8 columns");
  REQUIRE(nvec >= 1 && nvec <= 400, RICADI_EINVAL, "1 <= nvec <= 400 required");
  REQUIRE(dV && dW && dH, RICADI_EINVAL, "NULL argument");
  const int64_t nm = (int64_t)c->n * mc;
  REQUIRE(g_stride >= nm && v_stride >= nm, RICADI_EINVAL, "bad v_stride / g_stride");
  API_BEGIN_ON(c)
  const int m2 = 2 * mc;
  cplx_ensure_work(c, ng, nvec, false);
  const int ldp = c->cw.nvec + 1;
  const GroupTab all = all_groups(ng);
  cplx_orth(c, all, m2, nvec, dV, (size_t)v_stride * 2, (size_t)g_stride * 2, dW, (size_t)nm * 2, ldp, dW,
            (size_t)nm * 2);
  for (int g = 0; g < ng; ++g)
    HIPCHK(hipMemcpy2DAsync(dH + (size_t)g * (nvec + 1) * m2, sizeof(double) * m2, c->cw.hout.p + (size_t)g * ldp * 16,
                            sizeof(double) * 16, sizeof(double) * m2, nvec + 1, hipMemcpyDeviceToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

}  // extern "C"
