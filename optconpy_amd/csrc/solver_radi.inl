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

// The per-shift entry of a GENERATED shift (RICADI_RADI_SHIFTS_HAMILTONIAN): c->cache is an unbounded map keyed by the
// shift, and thirty distinct shifts per call would each leave their per-shift data behind (the dense coarse inverse
// alone is about 40 MB at cfg2).  Instead every level lends its one ricadi_ctx::radi_sd to its map under the shift's
// key, marked stale -- so that setup_issue rebuilds it in the buffers it already has and resets smw_epoch and the
// `rec` serials, as for any stale entry -- and takes it back before the next shift, at the end of the call and when
// the call is left by an exception.  A level whose map already holds the key (a shift of the caller's list) is left
// alone.
struct OwnedShift {
  ricadi_ctx* c;
  std::pair<double, double> key{0.0, 0.0};
  std::vector<ricadi_ctx*> lent;
  explicit OwnedShift(ricadi_ctx* ctx) : c(ctx) {}
  OwnedShift(const OwnedShift&) = delete;
  OwnedShift& operator=(const OwnedShift&) = delete;
  void lend(double p) {
    take_back();
    key = std::make_pair(p, 1.0);
    for (ricadi_ctx* l = c; l; l = l->child.get()) {
      if (l->cache.count(key)) continue;
      if (!l->radi_sd) l->radi_sd.reset(new ShiftData);
      l->radi_sd->valid = false;
      l->radi_sd->last_iters = -1;
      l->radi_sd->sub = nullptr;
      lent.push_back(l);              // (before the emplace: if that throws, take_back finds nothing to take)
      l->cache.emplace(key, std::move(l->radi_sd));
    }
  }
  void take_back() {
    for (ricadi_ctx* l : lent) {
      auto it = l->cache.find(key);
      if (it == l->cache.end()) continue;
      l->radi_sd = std::move(it->second);
      l->cache.erase(it);
    }
    lent.clear();
  }
  ~OwnedShift() { take_back(); }
};

// The same for the up to RICADI_MAX_GROUPS generated shifts of one SWEEP (ricadi_set_radi_sweep_shifts; DESIGN.md
// 3d-4): solve g of the sweep borrows entry g of the level's ricadi_ctx::radi_sdv (ricadi_ctx::radi_sd stays with the
// sequential modes).  take_back() before a sweep that takes an entry of the caller's list: that one enters the cache
// as any listed shift does.
struct OwnedShifts {
  ricadi_ctx* c;
  std::vector<std::pair<std::pair<double, double>, std::pair<ricadi_ctx*, int>>> lent;      // key, (level, slot)
  explicit OwnedShifts(ricadi_ctx* ctx) : c(ctx) {}
  OwnedShifts(const OwnedShifts&) = delete;
  OwnedShifts& operator=(const OwnedShifts&) = delete;
  void lend(const double* ps, int G) {
    take_back();
    for (int g = 0; g < G; ++g) {
      const auto key = std::make_pair(ps[g], 1.0);
      for (ricadi_ctx* l = c; l; l = l->child.get()) {
        if (l->cache.count(key)) continue;
        if ((int)l->radi_sdv.size() <= g) l->radi_sdv.resize(g + 1);
        if (!l->radi_sdv[g]) l->radi_sdv[g].reset(new ShiftData);
        l->radi_sdv[g]->valid = false;
        l->radi_sdv[g]->last_iters = -1;
        l->radi_sdv[g]->sub = nullptr;
        lent.push_back(std::make_pair(key, std::make_pair(l, g)));      // (before the emplace, as OwnedShift)
        l->cache.emplace(key, std::move(l->radi_sdv[g]));
      }
    }
  }
  void take_back() {
    for (const auto& e : lent) {
      ricadi_ctx* l = e.second.first;
      auto it = l->cache.find(e.first);
      if (it == l->cache.end()) continue;
      l->radi_sdv[e.second.second] = std::move(it->second);
      l->cache.erase(it);
    }
    lent.clear();
  }
  ~OwnedShifts() { take_back(); }
};

// Scratch of the shift selection (HAMILTONIAN mode), sized once per call
struct RadiShiftWork {
  TArr<double> Q, Q1, G, T, Rq, H, part, gpart;
  explicit RadiShiftWork(ricadi_ctx* c)
      : Q(c->pool), Q1(c->pool), G(c->pool), T(c->pool), Rq(c->pool), H(c->pool), part(c->pool), gpart(c->pool) {}
  // cq: the columns of the basis -- m for the block of one step; for the group of a sweep the largest
  // multiple of m the selection may meet: the partial buffers then hold any multiple of m up to it
  void alloc(ricadi_ctx* c, int cq, int m, int nb) {
    const int nv = c->nv;
    Q.alloc((size_t)nv * cq);
    Q1.alloc((size_t)nv * cq);
    G.alloc((size_t)cq * cq);
    T.alloc((size_t)4 * 128 * 128);
    Rq.alloc((size_t)cq * cq);
    H.alloc((size_t)cq * (2 * cq + m + 2 * nb));
    size_t np = 0, ng = 0;
    for (int k = cq; k >= m; k -= m) {
      np = std::max(np, radi_reduce_partial_len(nv, k, m, nb));
      ng = std::max(ng, gram_fixed_partial_len(nv, k));
    }
    part.alloc(np);
    gpart.alloc(ng);
  }
};

// Q R = the new block of Z (nv x cq at dZblk, leading dimension ldz, read where it lies; cq = m for the block of one
// step, a multiple of m for the group of blocks a sweep kept) and the reduced matrices
// H = Q^T [cal A Q | cal E Q | R | U | B] (ricadi_radi.hip; cq x (2cq + m + 2nb)), all on the stream, no host
// synchronisation.  The QR is the
// CholQR2 panel step of block_qr_dev on its kernels (cholqr_wide, the MFMA GEMM for Q), with the two Gram matrices from
// the fixed-order Gram kernel instead of the atomically accumulated GEMM: the same inputs give bitwise the same Q, R
// and H.  *qrflag (device) is raised when a Gram matrix is not positive definite to working precision; the caller then
// repeats the QR with block_qr_dev (Householder TSQR).
static void radi_shift_issue(ricadi_ctx* c, RadiShiftWork& w, const double* dZblk, int ldz, int cq, int m,
                             const double* dRU, const double* dB, int nb, int* qrflag) {
  hipStream_t st = c->st;
  const int nv = c->nv;
  double *T1 = w.T.p, *R1 = T1 + 16384, *T2 = R1 + 16384, *R2 = T2 + 16384;
  HIPCHK(hipMemsetAsync(qrflag, 0, sizeof(int), st));
  launch_gram_fixed(st, nv, cq, dZblk, ldz, w.gpart.p, w.G.p);
  launch_cholqr_wide(st, cq, w.G.p, cq, T1, R1, qrflag);
  launch_gemm_nn(st, nv, cq, cq, dZblk, ldz, T1, 128, w.Q1.p, cq, 1.0, 0.0);
  launch_gram_fixed(st, nv, cq, w.Q1.p, cq, w.gpart.p, w.G.p);
  launch_cholqr_wide(st, cq, w.G.p, cq, T2, R2, qrflag);
  launch_gemm_nn(st, nv, cq, cq, w.Q1.p, cq, T2, 128, w.Q.p, cq, 1.0, 0.0);
  launch_gemm_nn(st, cq, cq, cq, R2, 128, R1, 128, w.Rq.p, cq, 1.0, 0.0);        // R = R_2 R_1
  launch_radi_reduce(st, nv, cq, m, nb, c->s_rp.p, c->s_ci.p, c->srcA.p, c->srcE.p, w.Q.p, dRU, dB, w.part.p, w.H.p);
}

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

// The SWEEP form of the iteration (effective width Gw > 1; the formulas at
// ricadi_set_radi_sweep_width): the loop of ric_radi_run below with G <= Gw steps per pass.
//   1. ONE solve_batch with the G shifts against the panel [R_0 | U_0] (gsb = 0, c->q = nb, lr_ucol = m: the `dup`
//      path, S^-1 U out of the same solve for every shift; while U is identically zero the m columns of R, plain);
//   2. P = [R_0 | cal E Vh] (launch_sweep_resid_panel on the compacted solution panels), Gamma = P^T P
//      (launch_gram_fixed), Gh_g = Vh_g^T B (launch_radi_vtb per shift): fixed summation orders;
//   3. the sweep's host synchronisation: Gamma and Gh;
//   4. ricadi::radi_sweep: the steps kept, the residual after each, the coefficient matrix Cf;
//   5. Cf uploaded;  6. launch_radi_sweep_combine: the kept blocks of Z, [R | U] advanced to R_k, U_k.
// CYCLE mode (gen = false): sweep s takes the next G = min(Gw, steps left) entries of the cycled list.
// GENERATED shifts (gen = true: ricadi_set_radi_sweep_shifts with RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT; DESIGN.md
// 3d-4): the first sweep is ONE step with shifts[0]; after the stop test of a sweep that does not end the iteration
//   7. the CholQR2 of the group of Z the sweep kept (its last min(k, 127 / m) blocks, read where they lie in c->Z,
//      BEFORE any recompression) and the reduction H = Q^T [cal A Q | cal E Q | R | U | B] (radi_shift_issue at
//      c = blocks * m columns), H, R and the QR's flag fetched: the sweep's SECOND host synchronisation (block_qr_dev
//      and the reduction once more where the flag is raised);
//   8. ricadi::radi_next_shifts_dominant: up to min(Gw, steps left) shifts for the next sweep, in acceptance order.
// A refused selection (or one after a step ricadi_probe_radi_refuse lists) makes the next sweep ONE step with the next
// entry of `shifts` (a counter of its own from shifts[1], cycling).  Generated shifts borrow their per-shift entries
// (OwnedShifts); entries of the list enter the cache.
// hbuf: pinned, nc^2 + K nb + K (K + m + nb) doubles (nc = K + m, K = Gw m), and with gen cq (2 cq + m + 2 nb) + cq^2
// + 1 more (cq = min(Gw, 127 / m) m).
static void radi_run_sweeps(ricadi_ctx* c, RadiStats& stt, const double* shifts, int ns, int Gw, bool gen,
                            const double* dB, int nb, int m, double* dRU, bool uzero, int max_steps, double res_reltol,
                            int compress_cols, bool verbose, double* hbuf) {
  hipStream_t st = c->st;
  const int nv = c->nv, n = c->n, mp = m + nb, Kw = Gw * m, ncw = Kw + m;
  TArr<double> dR0(c->pool, (size_t)nv * m), dVc(c->pool, (size_t)nv * Kw), dP(c->pool, (size_t)nv * ncw),
      dGh(c->pool, (size_t)Kw * nb), dGam(c->pool, (size_t)ncw * ncw), dCf(c->pool, (size_t)Kw * (Kw + mp)),
      dPart(c->pool, radi_vtb_partial_len(nv, m, nb));
  c->res_part.ensure(gram_fixed_partial_len(nv, ncw));
  c->sweep_u.ensure((size_t)n * mp * Gw);
  double *hGam = hbuf, *hGh = hGam + (size_t)ncw * ncw, *hCf = hGh + (size_t)Kw * nb;
  // generated shifts: the group's scratch, the fetched H, R and flag behind the sweep's own host buffers
  const int cqw = std::min(Gw, 127 / m) * m;
  double *hH = gen ? hCf + (size_t)Kw * (Kw + mp) : nullptr, *hR = gen ? hH + (size_t)cqw * (2 * cqw + m + 2 * nb) : nullptr;
  int* hqr = gen ? reinterpret_cast<int*>(hR + (size_t)cqw * cqw) : nullptr;
  int* qrflag = c->flag.p + 1;              // (block_qr_dev's word: the fallback QR reuses it)
  RadiShiftWork sw(c);
  OwnedShifts owned(c);
  if (gen) sw.alloc(c, cqw, m, nb);
  std::vector<double> ps(Gw), be(Gw, 1.0), resv(Gw), psn(Gw), crit(Gw);
  std::vector<ShiftData*> sds(Gw);
  std::vector<GmresResult> res(Gw);
  int zc_last = 0, sweeps = 0;
  int Gnext = 1, nfb = 1;                   // gen: the solves of the next sweep (its shifts in ps), the list's counter
  bool listed = true;                       // gen: the next sweep takes an entry of the caller's list
  if (gen) ps[0] = shifts[0];
  // RICADI_TIMING: setup, solve, reductions + fetch, host, combine, QR + reduction, selection
  double tph[7] = {0, 0, 0, 0, 0, 0, 0};
  Tick tk;
  auto lap = [&](int i) {
    if (c->sw.timing) {
      (void)hipStreamSynchronize(st);
      tph[i] += tk.lap();
    }
  };
  while (stt.steps < max_steps) {
    const int left = max_steps - stt.steps, G = gen ? Gnext : std::min(Gw, left), K = G * m, nc = K + m;
    if (!gen)
      for (int g = 0; g < G; ++g) ps[g] = shifts[(stt.steps + g) % ns];
    if (c->sw.timing) tk.lap();
    if (gen) {
      if (listed) owned.take_back();
      else owned.lend(ps.data(), G);
    }
    get_shifts(c, ps.data(), be.data(), G, sds.data());
    lap(0);
    double* x = c->sweep_u.p;
    int ldv = m;
    if (uzero) {
      c->q = 0;
      launch_copy_cols(st, nv, m, dRU, mp, 0, c->bvec.p, m, 0, 1.0);
      if (c->np > 0) HIPCHK(hipMemsetAsync(c->bvec.p + (size_t)nv * m, 0, sizeof(double) * (size_t)c->np * m, st));
      solve_batch(c, sds.data(), G, c->bvec.p, 0, x, m, false, nullptr, res.data());
    } else {
      c->q = nb;
      ++c->lr_epoch;
      launch_copy_cols(st, nv, nb, dRU, mp, m, c->U.p, nb, 0, 1.0);
      c->lr_ucol = m;
      load_rhs(c, dRU, mp, c->bvec.p);
      solve_batch(c, sds.data(), G, c->bvec.p, 0, x, mp, true, nullptr, res.data());
      c->lr_ucol = -1;
      ldv = mp;
    }
    const size_t vstride = (size_t)n * ldv;
    int its = 0;
    for (int g = 0; g < G; ++g) {
      its = std::max(its, res[g].iters);
      if (res[g].converged) continue;
      stt.nonconverged++;
      stt.worst_relres = std::max(stt.worst_relres, res[g].max_relres);
      if (verbose)
        fprintf(stderr, "[ricadi] RADI sweep %d shift %g: GMRES stopped at relres %.2e after %d its\n", sweeps + 1,
                ps[g], res[g].max_relres, res[g].iters);
    }
    stt.shift_solves += G;
    c->radi_sweep_widths.push_back(G);
    lap(1);
    // the reductions: P = [R_0 | cal E Vh], its Gram matrix, Gh
    launch_copy_cols(st, nv, m, dRU, mp, 0, dR0.p, m, 0, 1.0);
    const double* vb = x;
    size_t vs = vstride;
    if (ldv != m) {
      for (int g = 0; g < G; ++g) launch_copy_cols(st, nv, m, x + g * vstride, ldv, 0, dVc.p + (size_t)g * nv * m, m, 0, 1.0);
      vb = dVc.p;
      vs = (size_t)nv * m;
    }
    launch_sweep_resid_panel(st, nv, m, G, c->E.rp.p, c->E.ci.p, c->E.v.p, dR0.p, vb, vs, dP.p);
    c->res_part.ensure(gram_fixed_partial_len(nv, nc));       // (a narrower sweep slices the rows differently)
    launch_gram_fixed(st, nv, nc, dP.p, nc, c->res_part.p, dGam.p);
    for (int g = 0; g < G; ++g)
      launch_radi_vtb(st, nv, m, nb, x + g * vstride, ldv, dB, dPart.p, dGh.p + (size_t)g * m * nb);
    c->res_launches += 3 + 2 * G;
    HIPCHK(hipMemcpyAsync(hGam, dGam.p, sizeof(double) * nc * nc, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hGh, dGh.p, sizeof(double) * K * nb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (c->sw.timing) tph[2] += tk.lap();
    if (sweeps == 0) stt.rhs = gram_block_fro(hGam, nc, m, 0);
    int k = 0;
    const int rc = ricadi::radi_sweep(G, m, nb, ps.data(), hGh, hGam, stt.rhs, res_reltol, left, &k, resv.data(), hCf);
    if (c->sw.timing) tph[3] += tk.lap();
    if (rc != RICADI_OK) {
      c->radi_shift_hist.push_back(ps[0]);
      stt.breakdown = true;
      break;
    }
    const int km = k * m;
    HIPCHK(hipMemcpyAsync(dCf.p, hCf, sizeof(double) * K * (km + mp), hipMemcpyHostToDevice, st));
    launch_radi_sweep_combine(st, nv, G, m, nb, k, x, vstride, ldv, dP.p + m, nc, dCf.p, dRU, c->Z.p, c->zld, c->zc);
    uzero = false;
    ++sweeps;
    c->zc += km;
    for (int j = 0; j < k; ++j) {
      c->radi_shift_hist.push_back(ps[j]);
      c->adi_res_hist.push_back(resv[j]);
      if (verbose)
        fprintf(stderr, "[ricadi] RADI step %3d: shift %10.3e%s rel residual %9.3e (sweep %d of %d solves, gmres its %d)\n",
                stt.steps + j + 1, ps[j], !gen ? "" : sweeps == 1 ? " (first)" : listed ? " (fallback)" : " (generated)",
                resv[j], sweeps, G, its);
    }
    stt.steps += k;
    stt.res = resv[k - 1];
    lap(4);
    if (stt.res <= res_reltol) {
      c->adi_stop_rule = RICADI_STOP_RES;
      break;
    }
    if (gen && stt.steps < max_steps) {
      // the group of Z the sweep kept, where it lies in the factor: its QR, the reduction, the second synchronisation
      const int cq = std::min(k, 127 / m) * m, hw = 2 * cq + m + 2 * nb;
      const double* dZg = c->Z.p + (c->zc - cq);
      auto fetch = [&] {
        HIPCHK(hipMemcpyAsync(hH, sw.H.p, sizeof(double) * cq * hw, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hR, sw.Rq.p, sizeof(double) * cq * cq, hipMemcpyDeviceToHost, st));
      };
      radi_shift_issue(c, sw, dZg, c->zld, cq, m, dRU, dB, nb, qrflag);
      fetch();
      HIPCHK(hipMemcpyAsync(hqr, qrflag, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (*hqr != 0) {
        // the group's Gram matrix is not positive definite to working precision: Householder TSQR, and H once more
        block_qr_dev(c, dZg, c->zld, nv, cq, sw.Q.p, sw.Rq.p);
        launch_radi_reduce(st, nv, cq, m, nb, c->s_rp.p, c->s_ci.p, c->srcA.p, c->srcE.p, sw.Q.p, dRU, dB, sw.part.p,
                           sw.H.p);
        fetch();
        HIPCHK(hipStreamSynchronize(st));
        ++c->radi_qr_repeats;
      }
      if (c->sw.timing) tph[5] += tk.lap();
      const int want = std::min(Gw, max_steps - stt.steps);
      int kept = 0, nsel = 0;
      listed = ricadi::radi_next_shifts_dominant(cq, m, nb, hH, hR, want, psn.data(), crit.data(), &nsel, &kept) != 0 ||
               std::find(c->radi_refuse.begin(), c->radi_refuse.end(), stt.steps) != c->radi_refuse.end();
      c->radi_kept_hist.push_back(kept);
      if (listed) {
        ps[0] = shifts[nfb++ % ns];
        Gnext = 1;
        ++c->radi_fallbacks;
      } else {
        std::copy(psn.begin(), psn.begin() + nsel, ps.begin());
        Gnext = nsel;
      }
      if (c->sw.timing) tph[6] += tk.lap();
    }
    if (stt.steps < max_steps && c->zc - zc_last >= compress_cols) {
      factor_recompress(c);
      ++c->radi_recompressions;
      zc_last = c->zc;
    }
  }
  c->radi_sweep_info[1] = sweeps;
  if (c->sw.timing) {
    fprintf(stderr, "[ricadi timing] RADI %d steps in %d sweeps of width %d: per-shift setup %.1f ms, solve %.1f, reductions + fetch %.1f, host %.1f, combine %.1f",
            stt.steps, sweeps, Gw, 1e3 * tph[0], 1e3 * tph[1], 1e3 * tph[2], 1e3 * tph[3], 1e3 * tph[4]);
    if (gen) fprintf(stderr, ", QR + reduction %.1f, host selection %.1f", 1e3 * tph[5], 1e3 * tph[6]);
    fprintf(stderr, "\n");
  }
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
// Shifts: RICADI_RADI_SHIFTS_CYCLE cycles through `shifts`.  RICADI_RADI_SHIFTS_HAMILTONIAN (mw <= 32; with
// ..._DOMINANT any mw, the host's ricadi::radi_next_shift_dominant in place of radi_next_shift) starts with
// shifts[0] and generates every later shift from the iteration: right after the residual Gram launch the QR of the new
// block of Z and the reduction kernel are issued -- speculatively, once too often at the end --, H and R are fetched
// with the Gram matrix and the flag words in the step's ONE synchronisation, and the host selects the shift after the
// stop test (ricadi::radi_next_shift, ricadi_host.cpp); `shifts` is the fallback cycle, with a counter of its own.
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
  // the sweep form: CYCLE mode at the width the list allows; generated shifts (ricadi_set_radi_sweep_shifts, the
  // entries admit it with the DOMINANT mode only) at the cap -- no halving, the selection admits
  // shifts sweep by sweep; at 1 the sequential form below, mode 2 as it is without the setting
  const bool gensweep = c->radi_sweep_shifts != 0 && c->radi_shift_mode == RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT;
  const int Gw = c->radi_sweep_width <= 1 ? 1
                 : gensweep ? std::max(1, std::min(std::min(c->radi_sweep_width, max_steps),
                                                    std::min(RICADI_RADI_SWEEP_MAX_K / mw,
                                                             RICADI_MAX_GROUPS / ricadi::radi_sweep_groups(mw, nb))))
                 : c->radi_shift_mode == RICADI_RADI_SHIFTS_CYCLE
                     ? ricadi::radi_sweep_width(shifts, ns, mw, nb, c->radi_sweep_width, max_steps)
                     : 1;
  c->radi_sweep_info[0] = Gw;
  c->radi_sweep_info[1] = c->radi_sweep_info[2] = 0;
  c->radi_sweep_widths.clear();
  ensure_work(c, mp, Gw, nb);
  TArr<double> dWm(c->pool, (size_t)nv * m), dRU(c->pool, (size_t)nv * mp), dG(c->pool, (size_t)m * nb),
      dC(c->pool, (size_t)m * (2 * m + nb)), dPart(c->pool, radi_vtb_partial_len(nv, m, nb));
  // W is projected in place: private copy
  HIPCHK(hipMemcpyAsync(dWm.p, dW, sizeof(double) * nv * m, hipMemcpyDeviceToDevice, st));
  const bool dominant = c->radi_shift_mode == RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT;      // (mw <= 127)
  const bool ham = dominant || c->radi_shift_mode == RICADI_RADI_SHIFTS_HAMILTONIAN;
  const int hw = 3 * m + 2 * nb;                      // columns of H
  c->radi_shift_hist.clear();
  c->radi_fallbacks = 0;
  c->radi_kept_hist.clear();
  c->radi_qr_repeats = 0;
  c->radi_recompressions = 0;
  c->radi_ran = true;
  // per-shift data of the whole cycle (and of the projection) up front, as lyap_adi_dev; with generated shifts the
  // first shift only
  setup_and_project(c, shifts, ham ? 1 : std::min(ns, max_steps), project_w, dWm.p, m);
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
  const size_t cqw = (size_t)std::min(Gw, 127 / m) * m;       // columns of a generated sweep's selection group
  const size_t hsweep = Gw > 1 ? (size_t)(Gw + 1) * m * (Gw + 1) * m + (size_t)Gw * m * nb + (size_t)Gw * m * (Gw * m + mp) +
                                     (gensweep ? cqw * (2 * cqw + m + 2 * nb) + cqw * cqw + 1 : 0)
                               : 0;
  double* hg = res_host(c, std::max((size_t)2 * mm + 1 + (ham ? (size_t)m * hw + mm : 0), hsweep));
  int* hflag = reinterpret_cast<int*>(hg + 2 * mm);          // [0] the factorisation's flag, [1] the QR's
  double *hH = hg + 2 * mm + 1, *hR = hH + (size_t)m * hw;
  int* dflag = c->flag.p + 3;
  int* qrflag = c->flag.p + 1;                               // (block_qr_dev's word: the fallback QR reuses it)
  hflag[1] = 0;
  RadiShiftWork sw(c);
  if (ham && Gw == 1) sw.alloc(c, m, m, nb);
  OwnedShift owned(c);
  double p_next = shifts[0], margin = 0.0;
  bool fell_back = false;
  int nfb = 1;                                               // the fallback cycle's own counter
  double tph[4] = {0, 0, 0, 0};                              // RICADI_TIMING: setup, solve + dense step, QR + reduction, selection
  Tick tk;
  auto lap = [&](int i) {
    if (c->sw.timing) {
      (void)hipStreamSynchronize(st);
      tph[i] += tk.lap();
    }
  };
  if (Gw > 1) {
    radi_run_sweeps(c, stt, shifts, ns, Gw, gensweep, dB, nb, m, dRU.p, uzero, max_steps, res_reltol, compress_cols,
                    verbose, hg);
    max_steps = 0;                                           // (the loop below is the sequential form)
  } else {
    launch_gram_fixed(st, nv, m, dRU.p, mp, c->res_part.p, c->res_gram.p);
    c->res_launches += 2;
  }
  for (int step = 1; step <= max_steps; ++step) {
    const double p = ham ? p_next : shifts[(step - 1) % ns];
    c->radi_shift_hist.push_back(p);
    if (c->sw.timing) tk.lap();
    if (ham && step > 1) {
      if (fell_back) owned.take_back();
      else owned.lend(p);
    }
    ShiftData* sd = get_shift(c, p, 1.0);
    lap(0);
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
    lap(1);
    const double* dZblk = c->Z.p + c->zc;
    if (ham) {
      radi_shift_issue(c, sw, dZblk, c->zld, m, m, dRU.p, dB, nb, qrflag);
      HIPCHK(hipMemcpyAsync(hH, sw.H.p, sizeof(double) * m * hw, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(hR, sw.Rq.p, sizeof(double) * mm, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(hflag + 1, qrflag, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipMemcpyAsync(hg, c->res_gram.p, sizeof(double) * 2 * mm, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hflag, dflag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (c->sw.timing) tph[2] += tk.lap();
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
    if (verbose) {
      if (ham)
        fprintf(stderr, "[ricadi] RADI step %3d: shift %10.3e (%s, margin %.3f) rel residual %9.3e gmres its %d\n", step,
                p, step == 1 ? "first" : fell_back ? "fallback" : "generated", step == 1 || fell_back ? 0.0 : margin,
                stt.res, r.iters);
      else
        fprintf(stderr, "[ricadi] RADI step %3d: shift %10.3e rel residual %9.3e gmres its %d\n", step, p, stt.res,
                r.iters);
    }
    if (stt.res <= res_reltol) {
      c->adi_stop_rule = RICADI_STOP_RES;
      break;
    }
    if (ham && step < max_steps) {
      if (hflag[1] != 0) {
        // the block's Gram matrix is not positive definite to working precision: Householder TSQR, and H once more
        block_qr_dev(c, dZblk, c->zld, nv, m, sw.Q.p, sw.Rq.p);
        launch_radi_reduce(st, nv, m, m, nb, c->s_rp.p, c->s_ci.p, c->srcA.p, c->srcE.p, sw.Q.p, dRU.p, dB, sw.part.p,
                           sw.H.p);
        HIPCHK(hipMemcpyAsync(hH, sw.H.p, sizeof(double) * m * hw, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hR, sw.Rq.p, sizeof(double) * mm, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        ++c->radi_qr_repeats;
      }
      int kept = 0;
      fell_back = (dominant ? ricadi::radi_next_shift_dominant(m, nb, hH, hR, &p_next, &margin, &kept)
                            : ricadi::radi_next_shift(m, nb, hH, hR, &p_next, &margin, &kept)) != 0 ||
                  std::find(c->radi_refuse.begin(), c->radi_refuse.end(), step) != c->radi_refuse.end();
      c->radi_kept_hist.push_back(kept);
      if (fell_back) {
        p_next = shifts[nfb++ % ns];
        ++c->radi_fallbacks;
      }
      if (c->sw.timing) tph[3] += tk.lap();
    }
    if (step < max_steps && c->zc - zc_last >= compress_cols) {
      factor_recompress(c);
      ++c->radi_recompressions;
      zc_last = c->zc;
    }
  }
  stt.gmres_iters = c->total_iters - it0;
  stt.escalations = c->escalations - esc0;
  c->radi_sweep_info[2] = (int)stt.shift_solves;
  if (c->sw.timing && Gw == 1)
    fprintf(stderr, "[ricadi timing] RADI %d steps (%s shifts): per-shift setup %.1f ms, solve + dense step %.1f, QR + reduction %.1f, host selection %.1f\n",
            stt.steps, ham ? "generated" : "cycled", 1e3 * tph[0], 1e3 * tph[1], 1e3 * tph[2], 1e3 * tph[3]);
  if (dK_out && !stt.breakdown) {
    launch_copy_cols(st, nv, nb, dRU.p, mp, m, dK_out, nb, 0, 1.0);
    if (dOld) launch_axpby(st, (size_t)nv * nb, 1.0, dOld, 1.0, dK_out);
  }
  HIPCHK(hipStreamSynchronize(st));
  return stt;
}
