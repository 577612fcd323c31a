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

// The per-shift entries of GENERATED shifts (RICADI_RADI_SHIFTS_HAMILTONIAN[_DOMINANT]; the up to RICADI_MAX_GROUPS
// of one sweep with ricadi_set_radi_sweep_shifts): c->cache is an unbounded map keyed by the shift, and
// thirty distinct shifts per call would each leave their per-shift data behind (the dense coarse inverse alone is about
// 40 MB at cfg2).  Instead every level lends entry g of its ricadi_ctx::radi_sdv to its map under the key of shift g
// -- a sequential step lends entry 0: lend(&p, 1) --, marked stale -- so that setup_issue rebuilds it in the buffers it
// already has and resets smw_epoch and the `rec` serials, as for any stale entry -- and takes it back before the next
// shifts, at the end of the call and when the call is left by an exception.  A level whose map already holds the key
// (a shift of the caller's list) is left alone.  take_back() before a solve that takes an entry of the caller's list:
// that one enters the cache as any listed shift does.
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
        lent.push_back(std::make_pair(key, std::make_pair(l, g)));      // (before the emplace: should that throw)
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

// The pinned host buffer of one call (res_host), laid out in this ONE place: what a pass fetches and what it uploads.
// At sweep width Gw (K = Gw m, nc = K + m): Gam nc x nc, Gh K x nb, Cf K x (K + m + nb); with a selection (gen) H
// cq x (2 cq + m + 2 nb) and R cq x cq of its widest group (cq = min(Gw, 127 / m) m); last the flag words ([0] the
// factorisation's, [1] the selection QR's).  The sequential form is the shape Gw = 1: its two m x m Gram matrices lie
// in Gam, its selection has cq = m.
struct RadiHostBuf {
  size_t count;                     // doubles in all
  double *Gam, *Gh, *Cf, *H, *R;
  int* flags;
  RadiHostBuf(ricadi_ctx* c, int Gw, int m, int nb, bool gen) {
    const size_t K = (size_t)Gw * m, nc = K + m, cq = gen ? (size_t)std::min(Gw, 127 / m) * m : 0;
    const size_t sizes[5] = {nc * nc, K * nb, K * (K + m + nb), cq * (2 * cq + m + 2 * nb), cq * cq};
    count = 1;
    for (size_t s : sizes) count += s;
    Gam = res_host(c, count);
    Gh = Gam + sizes[0];
    Cf = Gh + sizes[1];
    H = Cf + sizes[2];
    R = H + sizes[3];
    flags = reinterpret_cast<int*>(R + sizes[4]);
    flags[0] = flags[1] = 0;
  }
};

// The solve's hint that U is columns [lr_ucol, lr_ucol + q) of its right-hand side holds for ONE solve: no exit
// between setting it and that solve -- also not an exception -- leaves it behind
struct UcolHintReset {
  ricadi_ctx* c;
  ~UcolHintReset() { c->lr_ucol = -1; }
};

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
//
// One call is prepare(), run_steps() or run_sweeps(), finish() (ric_radi_run below).  The two loops are lists of the
// phases; a decision both forms make is ONE member function, and the members are what the phases share.  The guards
// are members, so every exit runs them.
struct RadiRun {
  ricadi_ctx* const c;
  const double *const shifts, *const dB, *const dOld;
  const int ns, nb, m, mp, nv, max_steps;
  const double res_reltol;
  const int compress_cols;
  const bool verbose;
  const hipStream_t st;
  const bool dominant, ham, gen;    // (dominant: mw <= 127)  gen: the sweep form generates its shifts
  const int Gw;                     // the sweep width in force; 1: the sequential form
  RadiStats stt;
  LowRankReset lowrank_reset;
  Restore<int> keep_rec;
  TArr<double> dWm, dRU, dPart;     // W projected in place: private copy; the panel [R | U]; radi_vtb's partials
  RadiShiftWork sw;
  OwnedShifts owned;
  RadiHostBuf h;
  int* const dflag;
  int* const qrflag;                // (block_qr_dev's word: the fallback QR reuses it)
  bool uzero;                       // U is identically zero
  bool listed = true;               // generated shifts: the pass in hand takes an entry of the caller's list
  int nfb = 1, zc_last = 0;         // the fallback list's own counter; the factor's columns at the last recompression
  long it0 = 0, esc0 = 0;
  // RICADI_TIMING.  Steps: setup, solve + dense step, QR + reduction, selection.  Sweeps: setup, solve, reductions +
  // fetch, host, combine, QR + reduction, selection
  double tph[7] = {0, 0, 0, 0, 0, 0, 0};
  Tick tk;
  // the sweep form: its scratch, the shifts of the sweep in hand (ps; gen: of the next one as soon as they are chosen),
  // what its solves returned, and what one phase leaves for the next
  TArr<double> dR0, dVc, dP, dGh, dGam, dCf;
  std::vector<double> ps, be, resv, psn, crit;
  std::vector<ShiftData*> sds;
  std::vector<GmresResult> res;
  int sweeps = 0, G = 0, k = 0, ldv = 0, its = 0;

  RadiRun(ricadi_ctx* ctx, const double* shifts_, int ns_, const double* dB_, int nb_, int mw, const double* dOld_,
          int max_steps_, double res_reltol_, int compress_cols_, bool verbose_)
      : c(ctx), shifts(shifts_), dB(dB_), dOld(dOld_), ns(ns_), nb(nb_), m(mw), mp(mw + nb_), nv(ctx->nv),
        max_steps(max_steps_), res_reltol(res_reltol_), compress_cols(compress_cols_ <= 0 ? 512 : compress_cols_),
        verbose(verbose_), st(ctx->st), dominant(ctx->radi_shift_mode == RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT),
        ham(dominant || ctx->radi_shift_mode == RICADI_RADI_SHIFTS_HAMILTONIAN),
        gen(ctx->radi_sweep_shifts != 0 && dominant), Gw(width_in_force()), lowrank_reset{ctx},
        keep_rec(ctx->rec_depth), dWm(ctx->pool), dRU(ctx->pool), dPart(ctx->pool), sw(ctx), owned(ctx),
        h(ctx, Gw, mw, nb_, Gw > 1 ? gen : ham), dflag(ctx->flag.p + 3), qrflag(ctx->flag.p + 1),
        uzero(dOld_ == nullptr), dR0(ctx->pool), dVc(ctx->pool), dP(ctx->pool), dGh(ctx->pool), dGam(ctx->pool),
        dCf(ctx->pool) {}

  // the sweep form: CYCLE mode at the width the list allows; generated shifts (ricadi_set_radi_sweep_shifts, the
  // entries admit it with the DOMINANT mode only) at the cap -- no halving, the selection admits
  // shifts sweep by sweep; at 1 the sequential form, mode 2 as it is without the setting
  int width_in_force() const {
    const int want = c->radi_sweep_width;
    if (want <= 1) return 1;
    if (gen) return std::max(1, std::min(std::min(want, max_steps), ricadi::radi_sweep_cap(m, nb)));
    if (c->radi_shift_mode != RICADI_RADI_SHIFTS_CYCLE) return 1;
    return ricadi::radi_sweep_width(shifts, ns, m, nb, want, max_steps);
  }

  void lap(int i) {
    if (c->sw.timing) {
      (void)hipStreamSynchronize(st);
      tph[i] += tk.lap();
    }
  }

  // the context's "last call" state cleared, the workspaces sized, the first shifts set up, W projected, the panel
  // [R | U] = [P^T W | -old] and V = B in place, the factor empty
  void prepare(const double* dW, bool project_w) {
    c->rec_depth = 0;
    c->q = 0;
    ++c->lr_epoch;
    c->adi_res_hist.clear();
    c->adi_stop_rule = RICADI_STOP_MAX_STEPS;
    c->adi_ran = true;
    c->radi_sweep_info[0] = Gw;
    c->radi_sweep_info[1] = c->radi_sweep_info[2] = 0;
    c->radi_sweep_widths.clear();
    ensure_work(c, mp, Gw, nb);
    dWm.alloc((size_t)nv * m);
    dRU.alloc((size_t)nv * mp);
    dPart.alloc(radi_vtb_partial_len(nv, m, nb));
    HIPCHK(hipMemcpyAsync(dWm.p, dW, sizeof(double) * nv * m, hipMemcpyDeviceToDevice, st));
    c->radi_shift_hist.clear();
    c->radi_fallbacks = 0;
    c->radi_kept_hist.clear();
    c->radi_qr_repeats = 0;
    c->radi_recompressions = 0;
    c->radi_ran = true;
    // per-shift data of the whole cycle (and of the projection) up front, as lyap_adi_dev; with generated shifts the
    // first shift only
    setup_and_project(c, shifts, ham ? 1 : std::min(ns, max_steps), project_w, dWm.p, m);
    launch_copy_cols(st, nv, m, dWm.p, m, 0, dRU.p, mp, 0, 1.0);
    if (dOld) launch_copy_cols(st, nv, nb, dOld, nb, 0, dRU.p, mp, m, -1.0);
    else HIPCHK(hipMemset2DAsync(dRU.p + m, sizeof(double) * mp, 0, sizeof(double) * nb, nv, st));
    c->U.ensure((size_t)nv * nb);
    c->V.ensure((size_t)nv * nb);
    HIPCHK(hipMemcpyAsync(c->V.p, dB, sizeof(double) * nv * nb, hipMemcpyDeviceToDevice, st));
    factor_reserve(c, max_steps * m);
    it0 = c->total_iters;
    esc0 = c->escalations;
  }

  // Per-shift entries for the G shifts at p: generated shifts borrow theirs; before an entry of the caller's list
  // what was lent goes back, and that entry enters the cache as any listed shift does.
  void entries_for(const double* p, int g, bool from_list) {
    if (from_list) owned.take_back();
    else owned.lend(p, g);
  }

  // The context and the right-hand side made ready for a solve against the panel, and the solve: solve(width, lowrank)
  // reads c->bvec.  While U is identically zero the m columns of R, plain; else [R | U] with c->U = U, c->q = nb and
  // lr_ucol = m -- the `dup` path: S^-1 U out of the same solve.  Returns the leading dimension of the solutions.
  template <class F>
  int solve_panel(F&& solve) {
    if (uzero) {
      c->q = 0;
      launch_copy_cols(st, nv, m, dRU.p, mp, 0, c->bvec.p, m, 0, 1.0);
      if (c->np > 0) HIPCHK(hipMemsetAsync(c->bvec.p + (size_t)nv * m, 0, sizeof(double) * (size_t)c->np * m, st));
      solve(m, false);
      return m;
    }
    c->q = nb;
    ++c->lr_epoch;
    launch_copy_cols(st, nv, nb, dRU.p, mp, m, c->U.p, nb, 0, 1.0);
    UcolHintReset hint_reset{c};
    c->lr_ucol = m;
    load_rhs(c, dRU.p, mp, c->bvec.p);
    solve(mp, true);
    return mp;
  }

  // a solve's outcome into the statistics; unit and idx name the pass in the verbose line ("step" 3, "sweep" 2)
  void record(const GmresResult& r, const char* unit, int idx, double p) {
    stt.shift_solves++;
    if (r.converged) return;
    stt.nonconverged++;
    stt.worst_relres = std::max(stt.worst_relres, r.max_relres);
    if (verbose)
      fprintf(stderr, "[ricadi] RADI %s %d shift %g: GMRES stopped at relres %.2e after %d its\n", unit, idx, p,
              r.max_relres, r.iters);
  }

  // H and R of a selection over cq columns on their way to the host
  void fetch_selection(int cq) {
    HIPCHK(hipMemcpyAsync(h.H, sw.H.p, sizeof(double) * cq * (2 * cq + m + 2 * nb), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h.R, sw.Rq.p, sizeof(double) * cq * cq, hipMemcpyDeviceToHost, st));
  }
  // the selection's CholQR2 of the cq columns of Z at dZg and its reduction issued; H, R and the QR's flag follow.  The
  // caller synchronises.
  void issue_selection(const double* dZg, int cq) {
    radi_shift_issue(c, sw, dZg, c->zld, cq, m, dRU.p, dB, nb, qrflag);
    fetch_selection(cq);
    HIPCHK(hipMemcpyAsync(h.flags + 1, qrflag, sizeof(int), hipMemcpyDeviceToHost, st));
  }
  // the Gram matrix of those columns was not positive definite to working precision: Householder TSQR, and H once more
  void repeat_selection_if_flagged(const double* dZg, int cq) {
    if (h.flags[1] == 0) return;
    block_qr_dev(c, dZg, c->zld, nv, cq, sw.Q.p, sw.Rq.p);
    launch_radi_reduce(st, nv, cq, m, nb, c->s_rp.p, c->s_ci.p, c->srcA.p, c->srcE.p, sw.Q.p, dRU.p, dB, sw.part.p,
                       sw.H.p);
    fetch_selection(cq);
    HIPCHK(hipStreamSynchronize(st));
    ++c->radi_qr_repeats;
  }

  // Generated or fallback, after a selection that returned rc with a basis of `kept`: refused by the host or by the
  // probe's list (ricadi_probe_radi_refuse, after this many steps), the next shift is the next entry of `shifts` -- a
  // counter of its own from shifts[1], cycling -- into *p.  Returns whether it fell back.
  bool fall_back(int rc, int kept, double* p) {
    const bool fb = rc != 0 || std::find(c->radi_refuse.begin(), c->radi_refuse.end(), stt.steps) != c->radi_refuse.end();
    c->radi_kept_hist.push_back(kept);
    if (fb) {
      *p = shifts[nfb++ % ns];
      ++c->radi_fallbacks;
    }
    return fb;
  }

  bool stopped() {
    if (stt.res > res_reltol) return false;
    c->adi_stop_rule = RICADI_STOP_RES;
    return true;
  }

  void recompress_if_due() {
    if (stt.steps >= max_steps || c->zc - zc_last < compress_cols) return;
    factor_recompress(c);
    ++c->radi_recompressions;
    zc_last = c->zc;
  }

  // The SEQUENTIAL form.  Shifts: RICADI_RADI_SHIFTS_CYCLE cycles through `shifts`.  RICADI_RADI_SHIFTS_HAMILTONIAN
  // (mw <= 32; with ..._DOMINANT any mw, the host's ricadi::radi_next_shift_dominant in place of radi_next_shift)
  // starts with shifts[0] and generates every later shift from the iteration: right after the residual Gram launch
  // the QR of the new block of Z and the reduction kernel are issued -- speculatively, once too often at the end --, H
  // and R are fetched with the Gram matrix and the flag words in the step's ONE synchronisation, and the host selects
  // the shift after the stop test (ricadi::radi_next_shift, ricadi_host.cpp); `shifts` is the fallback cycle.
  void run_steps() {
    const int mm = m * m;
    TArr<double> dG(c->pool, (size_t)m * nb), dC(c->pool, (size_t)m * (2 * m + nb));
    // ||R_j^T R_j||: the fixed-order Gram kernel on the R columns of the panel; ||R_0^T R_0|| is launched here and
    // fetched with the first step's
    c->res_part.ensure(gram_fixed_partial_len(nv, m));
    c->res_gram.ensure((size_t)2 * mm);
    if (ham) sw.alloc(c, m, m, nb);
    launch_gram_fixed(st, nv, m, dRU.p, mp, c->res_part.p, c->res_gram.p);
    c->res_launches += 2;
    double p = shifts[0], margin = 0.0;
    for (int step = 1; step <= max_steps; ++step) {
      if (!ham) p = shifts[(step - 1) % ns];
      c->radi_shift_hist.push_back(p);
      if (c->sw.timing) tk.lap();
      if (ham) entries_for(&p, 1, listed);
      ShiftData* sd = get_shift(c, p, 1.0);
      lap(0);
      GmresResult r;
      const int ld = solve_panel([&](int w, bool lr) { r = gmres_solve(c, sd, c->bvec.p, c->xs.p, w, lr, nullptr); });
      record(r, "step", step, p);
      radi_dense_step(c, p, c->xs.p, ld, m, dB, nb, dRU.p, c->Z.p, c->zld, c->zc, dG.p, dC.p, dPart.p, dflag);
      uzero = false;
      launch_gram_fixed(st, nv, m, dRU.p, mp, c->res_part.p, c->res_gram.p + mm);
      c->res_launches += 2;
      lap(1);
      const double* dZblk = c->Z.p + c->zc;
      if (ham) issue_selection(dZblk, m);
      HIPCHK(hipMemcpyAsync(h.Gam, c->res_gram.p, sizeof(double) * 2 * mm, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(h.flags, dflag, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (c->sw.timing) tph[2] += tk.lap();
      if (h.flags[0] != 0) {
        stt.breakdown = true;
        break;
      }
      if (step == 1) stt.rhs = gram_block_fro(h.Gam, m, m, 0);
      const double wf = gram_block_fro(h.Gam + mm, m, m, 0);
      stt.res = stt.rhs > 0.0 ? wf / stt.rhs : 0.0;
      c->zc += m;
      stt.steps = step;
      c->adi_res_hist.push_back(stt.res);
      if (verbose) {
        if (ham)
          fprintf(stderr, "[ricadi] RADI step %3d: shift %10.3e (%s, margin %.3f) rel residual %9.3e gmres its %d\n", step,
                  p, step == 1 ? "first" : listed ? "fallback" : "generated", listed ? 0.0 : margin, stt.res, r.iters);
        else
          fprintf(stderr, "[ricadi] RADI step %3d: shift %10.3e rel residual %9.3e gmres its %d\n", step, p, stt.res,
                  r.iters);
      }
      if (stopped()) break;
      if (ham && step < max_steps) {
        repeat_selection_if_flagged(dZblk, m);
        int kept = 0;
        listed = fall_back(dominant ? ricadi::radi_next_shift_dominant(m, nb, h.H, h.R, &p, &margin, &kept)
                                    : ricadi::radi_next_shift(m, nb, h.H, h.R, &p, &margin, &kept),
                           kept, &p);
        if (c->sw.timing) tph[3] += tk.lap();
      }
      recompress_if_due();
    }
    if (c->sw.timing)
      fprintf(stderr, "[ricadi timing] RADI %d steps (%s shifts): per-shift setup %.1f ms, solve + dense step %.1f, QR + reduction %.1f, host selection %.1f\n",
              stt.steps, ham ? "generated" : "cycled", 1e3 * tph[0], 1e3 * tph[1], 1e3 * tph[2], 1e3 * tph[3]);
  }

  // The SWEEP form (effective width Gw > 1; the formulas at ricadi_set_radi_sweep_width): the loop of
  // run_steps with G <= Gw steps per pass.
  //   1. ONE solve_batch with the G shifts against the panel [R_0 | U_0] (gsb = 0; solve_panel);
  //   2. P = [R_0 | cal E Vh] (launch_sweep_resid_panel on the compacted solution panels), Gamma = P^T P
  //      (launch_gram_fixed), Gh_g = Vh_g^T B (launch_radi_vtb per shift): fixed summation orders;
  //   3. the sweep's host synchronisation: Gamma and Gh (sweep_reduce);
  //   4. ricadi::radi_sweep: the steps kept, the residual after each, the coefficient matrix Cf (sweep_host);
  //   5. Cf uploaded;  6. launch_radi_sweep_combine: the kept blocks of Z, [R | U] advanced to R_k, U_k (sweep_combine).
  // CYCLE mode (gen false): sweep s takes the next G = min(Gw, steps left) entries of the cycled list.
  // GENERATED shifts (gen: ricadi_set_radi_sweep_shifts with RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT):
  // the first sweep is ONE step with shifts[0]; after the stop test of a sweep that does not end the iteration
  // select_sweep chooses the next sweep's shifts, or ONE step with the list's next entry.
  void run_sweeps() {
    const int Kw = Gw * m, ncw = Kw + m;
    dR0.alloc((size_t)nv * m);
    dVc.alloc((size_t)nv * Kw);
    dP.alloc((size_t)nv * ncw);
    dGh.alloc((size_t)Kw * nb);
    dGam.alloc((size_t)ncw * ncw);
    dCf.alloc((size_t)Kw * (Kw + mp));
    c->res_part.ensure(gram_fixed_partial_len(nv, ncw));
    c->sweep_u.ensure((size_t)c->n * mp * Gw);
    // generated shifts: the scratch of the widest group a selection may meet
    if (gen) sw.alloc(c, std::min(Gw, 127 / m) * m, m, nb);
    ps.resize(Gw);
    be.assign(Gw, 1.0);
    resv.resize(Gw);
    psn.resize(Gw);
    crit.resize(Gw);
    sds.resize(Gw);
    res.resize(Gw);
    int Gnext = 1;                  // gen: the solves of the next sweep
    ps[0] = shifts[0];
    while (stt.steps < max_steps) {
      const int left = max_steps - stt.steps;
      G = gen ? Gnext : std::min(Gw, left);
      if (!gen)
        for (int g = 0; g < G; ++g) ps[g] = shifts[(stt.steps + g) % ns];
      if (c->sw.timing) tk.lap();
      if (gen) entries_for(ps.data(), G, listed);
      get_shifts(c, ps.data(), be.data(), G, sds.data());
      lap(0);
      ldv = solve_panel([&](int w, bool lr) {
        solve_batch(c, sds.data(), G, c->bvec.p, 0, c->sweep_u.p, w, lr, nullptr, res.data());
      });
      its = 0;
      for (int g = 0; g < G; ++g) {
        its = std::max(its, res[g].iters);
        record(res[g], "sweep", sweeps + 1, ps[g]);
      }
      c->radi_sweep_widths.push_back(G);
      lap(1);
      sweep_reduce();
      if (c->sw.timing) tph[2] += tk.lap();
      if (!sweep_host(left)) break;
      sweep_combine();
      lap(4);
      if (stopped()) break;
      if (gen && stt.steps < max_steps) Gnext = select_sweep();
      recompress_if_due();
    }
    c->radi_sweep_info[1] = sweeps;
    if (c->sw.timing) {
      fprintf(stderr, "[ricadi timing] RADI %d steps in %d sweeps of width %d: per-shift setup %.1f ms, solve %.1f, reductions + fetch %.1f, host %.1f, combine %.1f",
              stt.steps, sweeps, Gw, 1e3 * tph[0], 1e3 * tph[1], 1e3 * tph[2], 1e3 * tph[3], 1e3 * tph[4]);
      if (gen) fprintf(stderr, ", QR + reduction %.1f, host selection %.1f", 1e3 * tph[5], 1e3 * tph[6]);
      fprintf(stderr, "\n");
    }
  }

  // 2., 3.: the reductions of the sweep's G solutions (c->sweep_u, leading dimension ldv) and their fetch
  void sweep_reduce() {
    const int K = G * m, nc = K + m;
    const double* x = c->sweep_u.p;
    const size_t vstride = (size_t)c->n * ldv;
    launch_copy_cols(st, nv, m, dRU.p, mp, 0, dR0.p, m, 0, 1.0);
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
    HIPCHK(hipMemcpyAsync(h.Gam, dGam.p, sizeof(double) * nc * nc, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h.Gh, dGh.p, sizeof(double) * K * nb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }

  // 4.: k, resv and Cf from what was fetched; false: breakdown, the iteration ends
  bool sweep_host(int left) {
    if (sweeps == 0) stt.rhs = gram_block_fro(h.Gam, G * m + m, m, 0);
    k = 0;
    const int rc = ricadi::radi_sweep(G, m, nb, ps.data(), h.Gh, h.Gam, stt.rhs, res_reltol, left, &k, resv.data(), h.Cf);
    if (c->sw.timing) tph[3] += tk.lap();
    if (rc == RICADI_OK) return true;
    c->radi_shift_hist.push_back(ps[0]);
    stt.breakdown = true;
    return false;
  }

  // 5., 6.: the k kept steps into the factor, the panel and the histories
  void sweep_combine() {
    const int K = G * m, km = k * m;
    HIPCHK(hipMemcpyAsync(dCf.p, h.Cf, sizeof(double) * K * (km + mp), hipMemcpyHostToDevice, st));
    launch_radi_sweep_combine(st, nv, G, m, nb, k, c->sweep_u.p, (size_t)c->n * ldv, ldv, dP.p + m, K + m, dCf.p, dRU.p,
                              c->Z.p, c->zld, c->zc);
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
  }

  // 7. the CholQR2 of the group of Z the sweep kept (its last min(k, 127 / m) blocks, read where they lie in c->Z,
  //    BEFORE any recompression) and the reduction H = Q^T [cal A Q | cal E Q | R | U | B], H, R and the QR's flag
  //    fetched: the sweep's SECOND host synchronisation (the Householder repeat where the flag is raised);
  // 8. ricadi::radi_next_shifts_dominant: up to min(Gw, steps left) shifts for the next sweep into ps, in acceptance
  //    order.  A refused selection makes the next sweep ONE step with the list's next entry (fall_back).
  // Returns the solves of the next sweep.
  int select_sweep() {
    const int cq = std::min(k, 127 / m) * m;
    const double* dZg = c->Z.p + (c->zc - cq);
    issue_selection(dZg, cq);
    HIPCHK(hipStreamSynchronize(st));
    repeat_selection_if_flagged(dZg, cq);
    if (c->sw.timing) tph[5] += tk.lap();
    int kept = 0, nsel = 0;
    listed = fall_back(ricadi::radi_next_shifts_dominant(cq, m, nb, h.H, h.R, std::min(Gw, max_steps - stt.steps),
                                                         psn.data(), crit.data(), &nsel, &kept),
                       kept, &ps[0]);
    if (!listed) std::copy(psn.begin(), psn.begin() + nsel, ps.begin());
    if (c->sw.timing) tph[6] += tk.lap();
    return listed ? 1 : nsel;
  }

  // the statistics closed, the gain U + old out
  RadiStats finish(double* dK_out) {
    stt.gmres_iters = c->total_iters - it0;
    stt.escalations = c->escalations - esc0;
    c->radi_sweep_info[2] = (int)stt.shift_solves;
    if (dK_out && !stt.breakdown) {
      launch_copy_cols(st, nv, nb, dRU.p, mp, m, dK_out, nb, 0, 1.0);
      if (dOld) launch_axpby(st, (size_t)nv * nb, 1.0, dOld, 1.0, dK_out);
    }
    HIPCHK(hipStreamSynchronize(st));
    return stt;
  }
};

static RadiStats ric_radi_run(ricadi_ctx* c, const double* shifts, int ns, const double* dB, int nb, const double* dW,
                              int mw, const double* dOld, int max_steps, double res_reltol, int compress_cols,
                              bool project_w, bool verbose, double* dK_out) {
  RadiRun run(c, shifts, ns, dB, nb, mw, dOld, max_steps, res_reltol, compress_cols, verbose);
  run.prepare(dW, project_w);
  if (run.Gw > 1) run.run_sweeps();
  else run.run_steps();
  return run.finish(dK_out);
}
