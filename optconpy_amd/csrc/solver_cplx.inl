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

// The sizes and strides of a restart cycle of ng groups of mc complex columns on the context's workspace (after
// cplx_ensure_work): what the solve and the step probe hand to the three cycle functions below
struct CplxCycle {
  int mc, m2, n, restart, ldp;
  size_t gs, vstride, gsh, gsy;
};
CplxCycle cplx_cycle(const ricadi_ctx* c, int ng, int mc) {
  CplxCycle cy{};
  cy.mc = mc;
  cy.m2 = 2 * mc;
  cy.n = c->n;
  cy.restart = c->opts.gmres_restart;
  cy.ldp = c->cw.nvec + 1;
  cy.gs = (size_t)c->n * cy.m2;
  cy.vstride = cy.gs * ng;
  cy.gsh = (size_t)cy.ldp * 16;
  cy.gsy = (size_t)cy.restart * 16;
  return cy;
}

// cycle start from the squared residual norms in cw.nrm2: gv[0], scale, resid; v_0 = r / ||r|| into V slot 0
void cplx_cycle_start_launches(ricadi_ctx* c, const CplxCycle& cy, const GroupTab& tab) {
  ricadi_ctx::CplxWork& k = c->cw;
  launch_cplx_gmres_start(c->st, tab, cy.mc, cy.restart, k.nrm2.p, k.bnorm.p, k.gv.p, k.scale.p, k.resid.p);
  launch_cplx_axpby(c->st, tab, cy.gs, cy.m2, 0.0, nullptr, 0, 1.0, k.scale.p, k.r.p, cy.gs, k.V.p, cy.gs);
}

// Arnoldi step j after the product (w = S P^-1 v_j in cw.w): CGS2 against V[0 .. j] into V[j + 1], column j of the
// Hessenberg matrix through the rotations, the residual estimate into cw.resid
void cplx_arnoldi_launches(ricadi_ctx* c, const CplxCycle& cy, const GroupTab& ct, int j) {
  ricadi_ctx::CplxWork& k = c->cw;
  cplx_orth(c, ct, cy.m2, j + 1, k.V.p, cy.vstride, cy.gs, k.w.p, cy.gs, cy.ldp, k.V.p + (size_t)(j + 1) * cy.vstride,
            cy.gs);
  launch_cplx_gmres_hess(c->st, ct, cy.mc, j, cy.restart, k.hout.p, cy.gsh, k.Hm.p, k.cs.p, k.sn.p, k.gv.p, k.bnorm.p,
                         k.resid.p);
}

// cycle end: R y = g with the first ks[g] columns, x += Z y
void cplx_cycle_end_launches(ricadi_ctx* c, const CplxCycle& cy, const GroupTab& tab, const GroupInts& ks, double* dX) {
  ricadi_ctx::CplxWork& k = c->cw;
  launch_cplx_gmres_backsolve(c->st, tab, ks, cy.mc, cy.restart, k.Hm.p, k.gv.p, k.y.p, cy.gsy);
  launch_cplx_update(c->st, tab, ks, cy.n, cy.m2, k.Zb.p, cy.vstride, cy.gs, k.y.p, cy.gsy, 1.0, dX, cy.gs);
}

// S(alpha_g, beta_g) X_g = [R_g; 0] for ng groups in lockstep: flexible GMRES(restart) from zero, Z_j kept in FP64.
// R_g has rhs_rows rows (default: the nv velocity rows; n for a right-hand side with a pressure part, as the residual
// equation of the pair step's refinement has).
CplxResult cplx_solve(ricadi_ctx* c, int ng, const CplxCoefs& cf, const double* dR, size_t gsr, int mc, double* dX,
                      int rhs_rows = -1) {
  hipStream_t st = c->st;
  const int m2 = 2 * mc, n = c->n, restart = c->opts.gmres_restart, maxit = c->opts.gmres_maxit;
  const double tol = c->opts.gmres_tol;
  const size_t rows = rhs_rows < 0 ? (size_t)c->nv : (size_t)rhs_rows;
  CplxPrecond pc(c, ng, cf, m2);
  cplx_ensure_work(c, ng, restart + 1, true);
  c->cprobe = ricadi_ctx::CplxProbe();   // the workspace of a probe cycle in flight is the solve's now
  ricadi_ctx::CplxWork& k = c->cw;
  const CplxCycle cy = cplx_cycle(c, ng, mc);
  const int ldp = cy.ldp;
  const size_t gs = cy.gs, vstride = cy.vstride;
  const GroupTab all = all_groups(ng);
  // b_g = [R_g; 0], x_g = 0, r_g = b_g
  HIPCHK(hipMemsetAsync(k.b.p, 0, sizeof(double) * gs * ng, st));
  for (int g = 0; g < ng; ++g)
    HIPCHK(hipMemcpyAsync(k.b.p + g * gs, dR + g * gsr, sizeof(double) * rows * m2, hipMemcpyDeviceToDevice, st));
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
    cplx_cycle_start_launches(c, cy, tab);
    std::vector<int> cyc = act;
    GroupInts ks = same_int(0);
    for (int j = 0; j < restart && !cyc.empty(); ++j) {
      const GroupTab ct = cplx_table(cyc);
      double* vj = k.V.p + (size_t)j * vstride;
      double* zj = k.Zb.p + (size_t)j * vstride;
      pc.bt.tab = ct;
      precond_apply(c, pc.bt, pc.pf, CycleIO{vj, gs, nullptr, zj, nullptr, 0});
      cplx_product(c, ct, cf, m2, zj, gs, k.w.p, gs);
      cplx_arnoldi_launches(c, cy, ct, j);
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
    cplx_cycle_end_launches(c, cy, tab, ks, dX);
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
  c->cprobe = ricadi_ctx::CplxProbe();   // (the step writes the coefficient arrays of a probe cycle in flight)
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

// ---- step probe of the complex cycle (tests) --------------------------------------------------------------------
// The units cplx_solve is made of -- cplx_cycle_start_launches, cplx_arnoldi_launches, cplx_cycle_end_launches -- one
// call each on the solver's own workspace with the strides of a solve (cplx_cycle).  Neither the preconditioner nor
// the operator runs: the caller supplies w.  Synchronous.
static bool cplx_probe_live(const ricadi_ctx* c) {
  const ricadi_ctx::CplxProbe& p = c->cprobe;
  return p.ng > 0 && c->cw.basis && p.work == c->cw.V.p && p.restart == c->opts.gmres_restart && c->cw.n == c->n;
}

int ricadi_cplx_probe_begin_dev(ricadi_ctx* c, int ng, int mc, const double* dR, const double* bnorm) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(ng >= 1 && ng <= RICADI_MAX_GROUPS, RICADI_EINVAL, "1 <= ng <= 16 required");
  REQUIRE(mc >= 1 && mc <= 8, RICADI_EINVAL, "complex panels have 1 <= mc <= 8 columns");
  REQUIRE(dR && bnorm, RICADI_EINVAL, "NULL argument");
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  c->cprobe = ricadi_ctx::CplxProbe();
  const int restart = c->opts.gmres_restart;
  cplx_ensure_work(c, ng, restart + 1, true);
  ricadi_ctx::CplxWork& k = c->cw;
  const CplxCycle cy = cplx_cycle(c, ng, mc);
  const size_t G = (size_t)ng, rs = (size_t)restart;
  // whatever a step does not write reads back as NaN (all bits set)
  auto nan_fill = [&](DArr<double>& a, size_t count) { HIPCHK(hipMemsetAsync(a.p, 0xFF, sizeof(double) * count, st)); };
  nan_fill(k.V, (rs + 1) * cy.vstride);
  nan_fill(k.Hm, G * 8 * rs * (rs + 1) * 2);
  nan_fill(k.cs, G * 8 * rs);
  nan_fill(k.sn, G * 8 * rs * 2);
  nan_fill(k.gv, G * 8 * (rs + 1) * 2);
  nan_fill(k.y, G * cy.gsy);
  nan_fill(k.scale, G * 16);
  nan_fill(k.resid, G * 8);
  nan_fill(k.hout, G * cy.gsh);
  HIPCHK(hipMemcpyAsync(k.r.p, dR, sizeof(double) * cy.vstride, hipMemcpyDeviceToDevice, st));
  std::vector<double> bn(G * 8, 0.0);
  for (int g = 0; g < ng; ++g) std::copy(bnorm + (size_t)g * mc, bnorm + (size_t)(g + 1) * mc, bn.begin() + g * 8);
  HIPCHK(hipMemcpyAsync(k.bnorm.p, bn.data(), sizeof(double) * bn.size(), hipMemcpyHostToDevice, st));
  const GroupTab all = all_groups(ng);
  launch_cplx_dots(st, all, cy.n, cy.m2, 0, 1, nullptr, 0, 0, k.r.p, cy.gs, k.partial.p, cy.ldp, k.nrm2.p, 16);
  cplx_cycle_start_launches(c, cy, all);
  HIPCHK(hipStreamSynchronize(st));
  c->cprobe.ng = ng;
  c->cprobe.mc = mc;
  c->cprobe.restart = restart;
  c->cprobe.kdone.assign(ng, 0);
  c->cprobe.work = k.V.p;
  API_END
}

int ricadi_cplx_probe_step_dev(ricadi_ctx* c, int j, const double* dW, int nact, const int* groups) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(cplx_probe_live(c), RICADI_EINVAL, "no probe cycle: call ricadi_cplx_probe_begin_dev first");
  REQUIRE(j >= 0 && j < c->opts.gmres_restart, RICADI_EINVAL, "0 <= j < gmres_restart required");
  REQUIRE(dW && groups && nact >= 1 && nact <= c->cprobe.ng, RICADI_EINVAL, "bad argument");
  for (int i = 0; i < nact; ++i)
    REQUIRE(groups[i] >= 0 && groups[i] < c->cprobe.ng && std::find(groups, groups + i, groups[i]) == groups + i,
            RICADI_EINVAL, "distinct group ids in 0 .. ng-1 required");
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  const CplxCycle cy = cplx_cycle(c, c->cprobe.ng, c->cprobe.mc);
  for (int i = 0; i < nact; ++i) {
    const size_t off = (size_t)groups[i] * cy.gs;
    HIPCHK(hipMemcpyAsync(c->cw.w.p + off, dW + off, sizeof(double) * cy.gs, hipMemcpyDeviceToDevice, st));
  }
  cplx_arnoldi_launches(c, cy, cplx_table(std::vector<int>(groups, groups + nact)), j);
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < nact; ++i) c->cprobe.kdone[groups[i]] = j + 1;
  API_END
}

int ricadi_cplx_probe_close_dev(ricadi_ctx* c, const int* ks, int nz, const double* dZ, double* dX) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(cplx_probe_live(c), RICADI_EINVAL, "no probe cycle: call ricadi_cplx_probe_begin_dev first");
  REQUIRE(ks && dZ && dX && nz >= 1 && nz <= c->opts.gmres_restart, RICADI_EINVAL, "bad argument");
  for (int g = 0; g < c->cprobe.ng; ++g)
    REQUIRE(ks[g] >= 0 && ks[g] <= nz && ks[g] <= c->cprobe.kdone[g], RICADI_EINVAL,
            "0 <= k_g <= min(nz, steps run for the group) required");
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  const CplxCycle cy = cplx_cycle(c, c->cprobe.ng, c->cprobe.mc);
  GroupInts kk = same_int(0);
  for (int g = 0; g < c->cprobe.ng; ++g) kk.v[g] = ks[g];
  HIPCHK(hipMemcpyAsync(c->cw.Zb.p, dZ, sizeof(double) * (size_t)nz * cy.vstride, hipMemcpyDeviceToDevice, st));
  cplx_cycle_end_launches(c, cy, all_groups(c->cprobe.ng), kk, dX);
  HIPCHK(hipStreamSynchronize(st));
  API_END
}

int ricadi_cplx_probe_read_dev(ricadi_ctx* c, int what, int slot, double* dOut, int64_t cap, int64_t* count) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(cplx_probe_live(c), RICADI_EINVAL, "no probe cycle: call ricadi_cplx_probe_begin_dev first");
  REQUIRE(dOut && count && cap >= 0, RICADI_EINVAL, "bad argument");
  REQUIRE(what >= RICADI_CPROBE_V && what <= RICADI_CPROBE_NRM2, RICADI_EINVAL, "unknown probe quantity");
  REQUIRE(what != RICADI_CPROBE_V || (slot >= 0 && slot <= c->opts.gmres_restart), RICADI_EINVAL,
          "0 <= slot <= gmres_restart required");
  API_BEGIN_ON(c)
  const ricadi_ctx::CplxWork& k = c->cw;
  const CplxCycle cy = cplx_cycle(c, c->cprobe.ng, c->cprobe.mc);
  const size_t G = (size_t)c->cprobe.ng, rs = (size_t)cy.restart;
  const double* src = nullptr;
  size_t cnt = 0;
  switch (what) {
    case RICADI_CPROBE_V: src = k.V.p + (size_t)slot * cy.vstride, cnt = cy.vstride; break;
    case RICADI_CPROBE_HOUT: src = k.hout.p, cnt = G * (rs + 2) * 16; break;
    case RICADI_CPROBE_HM: src = k.Hm.p, cnt = G * 8 * rs * (rs + 1) * 2; break;
    case RICADI_CPROBE_CS: src = k.cs.p, cnt = G * 8 * rs; break;
    case RICADI_CPROBE_SN: src = k.sn.p, cnt = G * 8 * rs * 2; break;
    case RICADI_CPROBE_GV: src = k.gv.p, cnt = G * 8 * (rs + 1) * 2; break;
    case RICADI_CPROBE_Y: src = k.y.p, cnt = G * cy.gsy; break;
    case RICADI_CPROBE_SCALE: src = k.scale.p, cnt = G * 16; break;
    case RICADI_CPROBE_RESID: src = k.resid.p, cnt = G * 8; break;
    default: src = k.nrm2.p, cnt = G * 16; break;
  }
  *count = (int64_t)cnt;
  if ((int64_t)cnt > cap) throw HipError{"output buffer too small"};
  if (what == RICADI_CPROBE_HOUT)   // rows 0 .. gmres_restart + 1 of every group (the group stride is the workspace's)
    HIPCHK(hipMemcpy2DAsync(dOut, sizeof(double) * (rs + 2) * 16, src, sizeof(double) * cy.gsh,
                            sizeof(double) * (rs + 2) * 16, G, hipMemcpyDeviceToDevice, c->st));
  else
    HIPCHK(hipMemcpyAsync(dOut, src, sizeof(double) * cnt, hipMemcpyDeviceToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

}  // extern "C"
