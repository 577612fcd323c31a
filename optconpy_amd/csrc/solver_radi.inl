// solver_radi.inl -- low-rank RADI iteration for the projected Riccati equation (pru.proj_alg_ric_radi).
// Part of ricadi_solver.hip (one translation unit; included there in order).

// A driver that installs its own low-rank term in the context (Newton-Kleinman: (K_k - old) B^T; RADI: U_j B^T): whatever
// way it is left -- also by an exception -- no stale term may stay behind for later ricadi_lyap_adi /
// ricadi_shift_solve calls.
struct LowRankReset {
  ricadi_ctx* c;
  ~LowRankReset() {
    c->q = 0;
    ++c->lr_epoch;
  }
};

struct RadiStats {
  int steps = 0;
  double res = 0.0, rhs = 0.0;      // last relative residual, ||R_0^T R_0||_F
  long gmres_iters = 0, shift_solves = 0, nonconverged = 0, escalations = 0;
  double worst_relres = 0.0;
  bool breakdown = false;           // the factorisation kernel met a pivot that is not positive and finite
};

// The dense part of one step on device operands: G = V^T B, the coefficient matrix C, the fused update of [R | U]
// and the block of Z (ricadi_radi.hip).  dG (m x nb), dC (m x (2m + nb)), dPart (radi_vtb_partial_len) and the flag
// word are the caller's; the word is cleared here and raised by the factorisation kernel.
static void radi_dense_step(ricadi_ctx* c, double p, const double* dV, int ldv, int m, const double* dB, int nb,
                            double* dRU, double* dZ, int zld, int zc, double* dG, double* dC, double* dPart,
                            int* dflag) {
  hipStream_t st = c->st;
  HIPCHK(hipMemsetAsync(dflag, 0, sizeof(int), st));
  launch_radi_vtb(st, c->nv, m, nb, dV, ldv, dB, dPart, dG);
  launch_radi_factor(st, m, nb, p, dG, dC, dflag);
  launch_radi_update(st, c->nv, m, nb, c->E.rp.p, c->E.ci.p, c->E.v.p, dV, ldv, dC, dRU, dZ, zld, zc);
}

// RADI on DEVICE operands (row-major, their own width as leading dimension): dB nv x nb, dW nv x mw, dOld nv x nb or
// NULL.  Step j with the shift p of the cycle:
//   [[cal A - U B^T + p cal E, J^T], [J, 0]] [V; *] = [R; 0]   -- solve_batch with c->U = U, c->V = B; [R | U] is ONE
//       panel, so that S^-1 U comes out of the same solve (lr_ucol); while U is identically zero (first step without
//       `old`) the m columns of R alone are solved on the plain operator;
//   G = V^T B,  Y = I + G G^T = L L^T,  Z <- [Z, sqrt(-2p) V L^-T],  T = (-2p) V Y^-1,  R <- R + cal E T,
//   U <- U + (cal E T) G;
//   res_j = ||R^T R||_F / ||R_0^T R_0||_F  (the Riccati residual of Z Z^T is exactly R R^T): the one host
//       synchronisation the driver adds per step.
// The factor is left in the context (c->Z, c->zc); the gain cal E X B = U + old goes to dK_out (nv x nb, may be NULL).
// Recycling of solved right-hand sides is off inside (the panel width changes after the first step; the ring's
// assumptions have not been checked for that).
static RadiStats ric_radi_run(ricadi_ctx* c, const double* shifts, int ns, const double* dB, int nb, const double* dW,
                              int mw, const double* dOld, int max_steps, double res_reltol, int compress_cols,
                              bool project_w, bool verbose, double* dK_out) {
  RadiStats stt;
  hipStream_t st = c->st;
  const int nv = c->nv, m = mw, mp = mw + nb, mm = mw * mw;
  LowRankReset lowrank_reset{c};
  Restore<int> keep_rec(c->rec_depth);
  c->rec_depth = 0;
  c->q = 0;
  ++c->lr_epoch;
  c->adi_res_hist.clear();
  c->adi_stop_rule = RICADI_STOP_MAX_STEPS;
  c->adi_ran = true;
  if (compress_cols <= 0) compress_cols = 512;       // as the Newton driver
  ensure_work(c, mp, 1, nb);
  TArr<double> dWm(c->pool, (size_t)nv * m), dRU(c->pool, (size_t)nv * mp), dG(c->pool, (size_t)m * nb),
      dC(c->pool, (size_t)m * (2 * m + nb)), dPart(c->pool, radi_vtb_partial_len(nv, m, nb));
  // W is projected in place: private copy
  HIPCHK(hipMemcpyAsync(dWm.p, dW, sizeof(double) * nv * m, hipMemcpyDeviceToDevice, st));
  // per-shift data of the whole cycle (and of the projection) up front, as lyap_adi_dev
  setup_and_project(c, shifts, std::min(ns, max_steps), project_w, dWm.p, m);
  // the panel [R | U]: R = P^T W, U = -old
  launch_copy_cols(st, nv, m, dWm.p, m, 0, dRU.p, mp, 0, 1.0);
  if (dOld) launch_copy_cols(st, nv, nb, dOld, nb, 0, dRU.p, mp, m, -1.0);
  else HIPCHK(hipMemset2DAsync(dRU.p + m, sizeof(double) * mp, 0, sizeof(double) * nb, nv, st));
  bool uzero = dOld == nullptr;
  c->U.ensure((size_t)nv * nb);
  c->V.ensure((size_t)nv * nb);
  HIPCHK(hipMemcpyAsync(c->V.p, dB, sizeof(double) * nv * nb, hipMemcpyDeviceToDevice, st));
  factor_reserve(c, max_steps * m);
  const long it0 = c->total_iters, esc0 = c->escalations;
  int zc_last = 0;
  // ||R_j^T R_j||: the fixed-order Gram kernel on the R columns of the panel; ||R_0^T R_0|| is launched here and
  // fetched with the first step's
  c->res_part.ensure(gram_fixed_partial_len(nv, m));
  c->res_gram.ensure((size_t)2 * mm);
  double* hg = res_host(c, (size_t)2 * mm + 1);
  int* hflag = reinterpret_cast<int*>(hg + 2 * mm);
  int* dflag = c->flag.p + 3;
  launch_gram_fixed(st, nv, m, dRU.p, mp, c->res_part.p, c->res_gram.p);
  c->res_launches += 2;
  for (int step = 1; step <= max_steps; ++step) {
    const double p = shifts[(step - 1) % ns];
    ShiftData* sd = get_shift(c, p, 1.0);
    GmresResult r;
    int ldv = m;
    if (uzero) {
      c->q = 0;
      launch_copy_cols(st, nv, m, dRU.p, mp, 0, c->bvec.p, m, 0, 1.0);
      if (c->np > 0) HIPCHK(hipMemsetAsync(c->bvec.p + (size_t)nv * m, 0, sizeof(double) * (size_t)c->np * m, st));
      r = gmres_solve(c, sd, c->bvec.p, c->xs.p, m, false, nullptr);
    } else {
      c->q = nb;
      ++c->lr_epoch;
      launch_copy_cols(st, nv, nb, dRU.p, mp, m, c->U.p, nb, 0, 1.0);
      c->lr_ucol = m;
      load_rhs(c, dRU.p, mp, c->bvec.p);
      r = gmres_solve(c, sd, c->bvec.p, c->xs.p, mp, true, nullptr);
      c->lr_ucol = -1;
      ldv = mp;
    }
    if (!r.converged) {
      stt.nonconverged++;
      stt.worst_relres = std::max(stt.worst_relres, r.max_relres);
      if (verbose)
        fprintf(stderr, "[ricadi] RADI step %d shift %g: GMRES stopped at relres %.2e after %d its\n", step, p,
                r.max_relres, r.iters);
    }
    stt.shift_solves++;
    radi_dense_step(c, p, c->xs.p, ldv, m, dB, nb, dRU.p, c->Z.p, c->zld, c->zc, dG.p, dC.p, dPart.p, dflag);
    uzero = false;
    launch_gram_fixed(st, nv, m, dRU.p, mp, c->res_part.p, c->res_gram.p + mm);
    c->res_launches += 2;
    HIPCHK(hipMemcpyAsync(hg, c->res_gram.p, sizeof(double) * 2 * mm, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hflag, dflag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (*hflag != 0) {
      stt.breakdown = true;
      break;
    }
    if (step == 1) stt.rhs = gram_block_fro(hg, m, m, 0);
    const double wf = gram_block_fro(hg + mm, m, m, 0);
    stt.res = stt.rhs > 0.0 ? wf / stt.rhs : 0.0;
    c->zc += m;
    stt.steps = step;
    c->adi_res_hist.push_back(stt.res);
    if (verbose)
      fprintf(stderr, "[ricadi] RADI step %3d: shift %10.3e rel residual %9.3e gmres its %d\n", step, p, stt.res, r.iters);
    if (stt.res <= res_reltol) {
      c->adi_stop_rule = RICADI_STOP_RES;
      break;
    }
    if (step < max_steps && c->zc - zc_last >= compress_cols) {
      factor_recompress(c);
      zc_last = c->zc;
    }
  }
  stt.gmres_iters = c->total_iters - it0;
  stt.escalations = c->escalations - esc0;
  if (dK_out && !stt.breakdown) {
    launch_copy_cols(st, nv, nb, dRU.p, mp, m, dK_out, nb, 0, 1.0);
    if (dOld) launch_axpby(st, (size_t)nv * nb, 1.0, dOld, 1.0, dK_out);
  }
  HIPCHK(hipStreamSynchronize(st));
  return stt;
}
