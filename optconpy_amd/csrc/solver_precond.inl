// solver_precond.inl -- batches of panels; the saddle operator and the multilevel preconditioner on device panels.
// Part of ricadi_solver.hip (one translation unit; included there in order).

// ---- batches -----------------------------------------------------------------------
// The shifts of one batched solve: per group id the shift-dependent operands, and
// the table of groups a launch works on (ricadi_internal.h).  All workspace
// buffers are group-major with the strides below.
// A per-shift block operand of the preconditioner as stored: its pointer table in every precision (null where a shift
// has no copy in it)
struct BlockOperand {
  GroupPtrs d = {};
  GroupPtrsF f = {};
  GroupPtrsH h = {};    // BF16
  void set(int g, const double* pd, const float* pf, const uint16_t* ph = nullptr) {
    d.p[g] = pd;
    f.p[g] = pf;
    h.p[g] = ph;
  }
};
static GroupTab all_groups(int G) {
  GroupTab t{};
  t.ng = G;
  for (int g = 0; g < G; ++g) t.gid[g] = g;
  return t;
}
struct Batch {
  int G = 0;                 // groups in the solve (ids 0 .. G-1)
  int m = 0;                 // panel width of every group
  GroupTab tab;              // groups the next launches act on
  double alpha[RICADI_MAX_GROUPS], beta[RICADI_MAX_GROUPS];   // shift of every group id
  GroupPtrs sval = {}, svalb = {}, syval = {}, syvalb = {};
  BlockOperand bvinv, bpinv, gtm, adym;       // blocks of the sweeps
  BlockOperand einv;                          // the last level's dense inverse (no BF16 copy)
  BlockOperand vkinv;                         // patch inverses of the coloured Vanka sweep (a child level's batch)
  bool blocks16 = false;                      // every group of the batch has the BF16 copies of the sweeps' blocks
  size_t gs = 0, gsp = 0, gsc = 0, gsq = 0;   // strides: n*m, np*m, kc*m, q*m
  std::shared_ptr<Batch> sub;                 // the same groups on the child level
  hipStream_t st = nullptr;                   // stream of every launch for the batch (make_batch: the context's)
  // groups active in the whole lockstep solve when this batch is one half of it (gmres_core's split): the choice of
  // the multi-shift kernels follows the whole solve, so both halves launch what one stream would; 0: tab.ng
  int ng_solve = 0;
  int ms_groups() const { return ng_solve > 0 ? ng_solve : tab.ng; }

  void all() { tab = all_groups(G); }
  void only(int g) {
    tab.ng = 1;
    tab.gid[0] = g;
  }
  void set(const std::vector<int>& ids) {
    tab.ng = (int)ids.size();
    for (int i = 0; i < tab.ng; ++i) tab.gid[i] = ids[i];
  }
};

static Batch make_batch(ricadi_ctx* c, ShiftData* const* sds, int G, int m) {
  Batch bt;
  bt.G = G;
  bt.m = m;
  bt.tab = GroupTab{};
  bt.blocks16 = c->sw.blocks16 && G > 0;
  for (int g = 0; g < RICADI_MAX_GROUPS; ++g) bt.alpha[g] = bt.beta[g] = 0.0;
  for (int g = 0; g < G; ++g) {
    const ShiftData& s = *sds[g];
    bt.alpha[g] = s.alpha;
    bt.beta[g] = s.beta;
    bt.sval.p[g] = s.sval.p;
    bt.svalb.p[g] = s.svalb.p;
    bt.syval.p[g] = s.syval.p;
    bt.syvalb.p[g] = s.syvalb.p;
    bt.bvinv.set(g, s.bvinv.p, s.bvinvf.p, s.bvinvh.p);
    bt.bpinv.set(g, s.bpinv.p, s.bpinvf.p, s.bpinvh.p);
    bt.gtm.set(g, s.gtm.p, s.gtmf.p, s.gtmh.p);
    bt.adym.set(g, s.adym.p, s.adymf.p, s.adymh.p);
    bt.einv.set(g, s.einv.p, s.einvf.p);
    bt.vkinv.set(g, s.vkinv.p, s.vkinvf.p);
    if (!s.bvinvh.p || !s.bpinvh.p || !s.gtmh.p || !s.adymh.p) bt.blocks16 = false;
  }
  bt.gs = (size_t)c->n * m;
  bt.gsp = (size_t)c->np * m;
  bt.gsc = (size_t)c->kc * m;
  bt.gsq = (size_t)std::max(c->q, 1) * m;
  bt.st = c->st;
  bt.all();
  if (c->child) {
    ShiftData* subs[RICADI_MAX_GROUPS];
    for (int g = 0; g < G; ++g) subs[g] = sds[g]->sub;
    bt.sub = std::make_shared<Batch>(make_batch(c->child.get(), subs, G, m));
  }
  return bt;
}
static Batch make_batch(ricadi_ctx* c, ShiftData* sd, int m) { return make_batch(c, &sd, 1, m); }

// Multi-shift tile kernel or one workgroup per (row block, group)?  The multi-shift kernel
// reads the matrix once for all groups (26 -> 18 B per non-zero in total instead of 10 B per
// group) but walks the groups of a row block one after the other at 4 waves per SIMD; it
// pays where the per-shift value arrays of the active groups no longer fit the caches
// (measured: n = 5e5, 16 groups: 1.53 -> 1.25 ms per launch; n = 3e4: 83 -> 87 us).
static bool ms_pays(const ricadi_ctx* c, int ng, size_t nnz) {
  if (!c->sw.ms_spmm || !c->ms_ok) return false;
  if (c->sw.ms_force) return true;
  // per-shift value arrays of the active groups near or beyond the 256 MB infinity cache (measured with the FP32
  // operator input that follows this switch: cfg3, 227 MB: 197 -> 205 shift-solves/s; cfg2, 136 MB: 1.4 % slower)
  return ng >= 4 && (double)nnz * 10.0 * ng > 200e6;
}

// ---- operator and preconditioner on device panels ---------------------------------
// y = beta_r * r + alpha * S x on the saddle operator (optionally through the
// prolongation map): LDS-tiled kernel when the block tiles fit, else the CSR one.
// gsx / gsy / gsr: group strides of x, y, r.
// The LDS-tiled kernels serve panels of width m (else the CSR kernel runs)
static bool saddle_tiled(const ricadi_ctx* c, int m) {
  return c->sb_ok &&
         spmm_blocked_lds_bytes(m, c->sb_max_cols) <= (size_t)40 * 1024;
}
// x32 (optional): FP32 copy of x with the same leading dimension and group stride; the tiled kernels read it
// instead of x (plain products only: no residual term, no low-rank epilogue, no prolongation map)
static void saddle_spmm(ricadi_ctx* c, const Batch& bt, const double* x, size_t gsx,
                        const int* xmap, double* y, size_t gsy, const double* r, size_t gsr,
                        double alpha, double beta_r, const LowRankArgs& lr = LowRankArgs(),
                        const float* x32 = nullptr, float* y32 = nullptr) {
  const int m = bt.m;
  const bool fits = saddle_tiled(c, m);
  const bool has_lr = lr.q > 0 && lr.nrows > 0;
  if (x32 && fits && !r && !xmap && !has_lr) {
    const bool ms = ms_pays(c, bt.ms_groups(), c->snnz) && spmm_blocked_ms_ok(m, c->sb_max_cols, (size_t)c->n);
    c->k1_variant = (ms ? 2 : 1) + 4;
    if (ms)
      launch_spmm_blocked_ms_x32(bt.st, bt.tab, bt.alpha, bt.beta, c->sb_nblk, c->sb_rows2.p, c->sb_rp2.p,
                                 c->sb_cols2.p, c->sb_lidx_ms.p, c->sbAJ.p, c->sbE.p, x32, m, gsx, y, m, gsy, alpha,
                                 m, c->sb_max_cols, y32);
    else
      launch_spmm_blocked_x32(bt.st, bt.tab, c->sb_nblk, c->sb_rows2.p, c->sb_rp2.p, c->sb_cols2.p, c->sb_lidx.p,
                              bt.svalb, x32, m, gsx, y, m, gsy, alpha, m, c->sb_max_cols, y32);
    return;
  }
  if (y32) throw HipError{"FP32 operator output asked for outside the FP32-input tile kernels"};
  const bool ms = fits && ms_pays(c, bt.ms_groups(), c->snnz) && !xmap && !has_lr &&
                  spmm_blocked_ms_ok(m, c->sb_max_cols, (size_t)c->n);
  if (!xmap) c->k1_variant = ms ? 2 : fits ? 1 : 0;
  if (ms)
    launch_spmm_blocked_ms(bt.st, bt.tab, bt.alpha, bt.beta, c->sb_nblk, c->sb_rows2.p, c->sb_rp2.p,
                           c->sb_cols2.p, c->sb_lidx_ms.p, c->sbAJ.p, c->sbE.p, x, m, gsx, y, m, gsy,
                           r, m, gsr, alpha, beta_r, m, c->sb_max_cols);
  else if (fits)
    launch_spmm_blocked_b(bt.st, bt.tab, c->sb_nblk, c->sb_rows2.p, c->sb_rp2.p,
                          xmap ? c->sb_colsm2.p : c->sb_cols2.p, c->sb_lidx.p, bt.svalb, x, m, gsx, y,
                          m, gsy, r, m, gsr, alpha, beta_r, m, c->sb_max_cols, lr);
  else
    launch_spmm_b(bt.st, bt.tab, c->n, c->s_rp.p, c->s_ci.p, bt.sval, x, m, gsx, xmap, y, m, gsy, r,
                  m, gsr, alpha, beta_r, m, lr);
}

// y = S(alpha,beta) x for every active group (n x m panels, ld = m, group stride gsx /
// bt.gs); optional low-rank  - U V^T x_v  (U, V shared by the groups)
// y32 (optional, with x32 only): the product goes to this FP32 panel (stride bt.gs) and y is not written
// the low-rank term - U V^T x of the active groups (none without set_lowrank): the coefficients V^T x first; the
// product with U rides in the SpMM's epilogue
static LowRankArgs lowrank_args(ricadi_ctx* c, const Batch& bt, const double* x, size_t gsx) {
  LowRankArgs lr;
  if (c->q <= 0) return lr;
  HIPCHK(hipMemsetAsync(c->lrc.p, 0, sizeof(double) * bt.gsq * bt.G, bt.st));
  launch_gemm_tn_b(bt.st, bt.tab, c->nv, c->q, bt.m, c->V.p, c->q, x, bt.m, gsx, c->lrc.p, bt.m, bt.gsq);
  lr.U = c->U.p;
  lr.c = c->lrc.p;
  lr.gsc = bt.gsq;
  lr.q = c->q;
  lr.nrows = c->nv;
  return lr;
}
static void op_apply(ricadi_ctx* c, const Batch& bt, const double* x, size_t gsx, double* y,
                     bool lowrank, const float* x32 = nullptr, float* y32 = nullptr) {
  const LowRankArgs lr = lowrank ? lowrank_args(c, bt, x, gsx) : LowRankArgs();
  saddle_spmm(c, bt, x, gsx, nullptr, y, bt.gs, nullptr, 0, 1.0, 0.0, lr, x32, y32);
}
// fn(tables ...) with the tables of the operands ops in the precision a stage reads its blocks in: the level's (FP32,
// or FP64 with RICADI_PRECOND64=1); H: a stage whose launcher also takes BF16 blocks reads those where the cycle form
// puts it on them (b16)
template <bool H = false, class Fn, class... Op>
static void with_stored(const ricadi_ctx* c, bool b16, Fn&& fn, const Op&... ops) {
  if constexpr (H) {
    if (b16) return fn(ops.h...);
  }
  if (c->precond32) fn(ops.f...);
  else fn(ops.d...);
}
// ---- kernels of the preconditioner that ricadi_time_kernel_dev also launches on their own
// block-Jacobi sweep over the velocity (or pressure) blocks:  out[rows_b] (-)= inv_b in[rows_b]  (+ epilogue pa / cin)
static void block_sweep(ricadi_ctx* c, const Batch& bt, bool pressure, const double* in, size_t gsi, double* out,
                        int subtract, const ProlongArgs& pa = ProlongArgs(), const CsrInArgs& cin = CsrInArgs()) {
  const int nb = pressure ? c->nbp : c->nbv, m = bt.m;
  const int* bptr = pressure ? c->bp_ptr.p : c->bv_ptr.p;
  const int* rows = pressure ? c->bp_rows.p : c->bv_rows.p;
  // Plain panel input, 32 x 32 blocks, a latency-bound launch (few waves: the Schur sweep of cfg2 has 110 blocks x 16
  // groups): the rectangle kernel with the block's own rows as its input list -- its loads are issued in groups, the
  // plain kernel's index -> gather pairs are a chain of dependent round trips.  With many waves the rectangle kernel's
  // 152 VGPRs cost more than its grouped loads gain (velocity-sized sweep at cfg2: 43 vs 33 us).
  const bool as_rect = !cin.rp && c->bs == 32 && (long)nb * bt.tab.ng <= 8192;
  with_stored(c, false, [&](const auto& inv) {
    if (as_rect)
      launch_block_apply_rect_b(bt.st, bt.tab, 32, 32, nb, bptr, rows, bptr, rows, inv, in, m, gsi, out, m, bt.gs, m,
                                subtract, pa);
    else
      launch_block_apply_b(bt.st, bt.tab, c->bs, nb, bptr, rows, inv, in, m, gsi, out, m, bt.gs, m, subtract, pa, cin);
  }, pressure ? bt.bpinv : bt.bvinv);
}
// r2 = r - (S Y) ec through the tile kernels (c->syb_ok): the multi-shift one where it pays
static bool sy_tiled_ms(const ricadi_ctx* c, const Batch& bt) {
  return ms_pays(c, bt.ms_groups(), c->snnz) && spmm_blocked_ms_ok(bt.m, c->syb_max_cols, (size_t)c->kc);
}
static void sy_residual_tiled(ricadi_ctx* c, const Batch& bt, const double* r, size_t gsr) {
  const int m = bt.m;
  if (sy_tiled_ms(c, bt))
    launch_spmm_blocked_ms(bt.st, bt.tab, bt.alpha, bt.beta, c->sb_nblk, c->sb_rows2.p, c->syb_rp2.p, c->syb_cols2.p,
                           c->syb_lidx_ms.p, c->sybAJ.p, c->sybE.p, c->ec.p, m, bt.gsc, c->r2.p, m, bt.gs, r, m, gsr,
                           -1.0, 1.0, m, c->syb_max_cols);
  else
    launch_spmm_blocked_b(bt.st, bt.tab, c->sb_nblk, c->sb_rows2.p, c->syb_rp2.p, c->syb_cols2.p, c->syb_lidx.p,
                          bt.syvalb, c->ec.p, m, bt.gsc, c->r2.p, m, bt.gs, r, m, gsr, -1.0, 1.0, m, c->syb_max_cols);
}
// rc = Y^T r (smoothed aggregation: P^T r) by the 16-lanes-per-row CSR kernel
static void restrict_csr(ricadi_ctx* c, const Batch& bt, const double* r, size_t gsr) {
  const int* rrp = c->sa ? c->pt_rp.p : c->agg_ptr.p;
  const int* rci = c->sa ? c->pt_ci.p : c->agg_rows.p;
  const GroupPtrs rvals = same_ptr(c->sa ? (const double*)c->pt_v.p : c->ones.p);
  launch_spmm_b(bt.st, bt.tab, c->kc, rrp, rci, rvals, r, bt.m, gsr, nullptr, c->rc.p, bt.m, bt.gsc, nullptr, 0, 0,
                1.0, 0.0, bt.m);
}

// ---- the preconditioner cycle ------------------------------------------------------
// z = P^-1 r for every active group: multiplicative two-level, coarse correction first, then one consistent SIMPLE
// block-Jacobi sweep on the updated residual.
// What one application launches, stage by stage: decided by cycle_form alone (gmres_core once per solve, beside its
// IterationForm; ricadi_precond_apply_batch_dev, the kernel timers and setup_info ask it too).
struct CycleForm {
  // rc = Y^T r (P^T r): one wave per row (rc k-blocked for CO_DENSE_KB), 16-lane CSR on the FP16 / FP64 input
  enum Restriction { RS_NONE, RS_ROWWAVE, RS_CSR16, RS_CSR64 } restriction = RS_NONE;
  // ec = E^-1 rc: one cycle of the child level, or the last level's dense inverse (k-blocked pipelined, or tiled)
  enum Coarse { CO_NONE, CO_CHILD, CO_DENSE_KB, CO_DENSE } coarse = CO_NONE;
  // r2 = r - (S Y) ec before the sweeps: its pressure rows (folded cycle, split pressure step) or all of it (unfolded)
  enum SyResidual { SY_NONE, SY_PROWS, SY_FULL } sy = SY_NONE;
  // first velocity sweep: plain on r2; two-term with the coarse residual folded in, by the generic kernel or the
  // record-driven one (pipe: on BF16 blocks, its second segment's loads in flight behind the first segment's MFMAs)
  enum First { FS_PLAIN, FS_TWO_TERM, FS_TWO32, FS_TWO32_PIPE, FS_NONE } first = FS_PLAIN;
  // pressure step: one launch (K2p) on BF16 / FP32-or-FP64 blocks, or J product and Schur sweep on their own
  enum Pressure { PS_NONE, PS_FUSED16, PS_FUSED, PS_SPLIT } pressure = PS_NONE;
  // last velocity sweep: dense rectangles by the record-driven / the generic kernel, or the J^T product formed row by
  // row
  enum Last { LS_NONE, LS_RECT32, LS_RECT, LS_CSR_IN } last = LS_NONE;
  bool h16 = false;     // the input is read from the FP16-stored vector
  bool x32 = false;     // only the FP32 copy of z is wanted (the operator reads it)
  bool mid32 = false;   // the velocity part between the sweeps as an FP32 panel
  bool b16 = false;     // BF16-stored per-shift blocks: read by the pressure step and the record-driven sweeps
  bool folded = false;  // the coarse residual is formed inside the first sweep and the pressure step
  // a child level's coloured Vanka sweep in place of the SIMPLE sweeps: z = Y ec, then per colour the residual of the
  // level's operator and the patch kernel (pc_vanka); first = FS_NONE, no pressure step, no last sweep
  bool vanka = false;
  int two_ks = 0, rect_ks = 0;   // padded widths of the two-term sweep's second block / of the rectangles (0: none)
  // the sweeps that read BF16 blocks (a record-driven kernel runs on the level's FP32 / FP64 blocks as well)
  bool first16() const { return b16 && (first == FS_TWO32 || first == FS_TWO32_PIPE); }
  bool last16() const { return b16 && last == LS_RECT32; }
  // the form word of include/ricadi.h (restriction: its value is the 2-bit code; first and last: 1 = on BF16 blocks,
  // 2 = on FP32 / FP64 blocks by either kernel)
  unsigned word() const {
    unsigned w = (h16 ? RICADI_PCF_H16 : 0) | (x32 ? RICADI_PCF_X32 : 0) | (mid32 ? RICADI_PCF_MID32 : 0) |
                 (b16 ? RICADI_PCF_B16 : 0) | (folded ? RICADI_PCF_FOLDED : 0) | (vanka ? RICADI_PCF_VANKA : 0);
    w |= (unsigned)restriction << RICADI_PCF_RESTRICT_SHIFT;
    w |= (last == LS_NONE ? 0u : last == LS_CSR_IN ? 3u : last16() ? 1u : 2u) << RICADI_PCF_LAST_SHIFT;
    if (coarse != CO_NONE) w |= (coarse == CO_CHILD ? 1u : 2u) << RICADI_PCF_COARSE_SHIFT;
    w |= (first == FS_NONE ? 0u : first == FS_PLAIN ? 3u : first16() ? 1u : 2u) << RICADI_PCF_FIRST_SHIFT;
    if (pressure != PS_NONE) w |= pressure == PS_SPLIT ? RICADI_PCF_PSPLIT : RICADI_PCF_PFUSED;
    return w | (unsigned)two_ks << RICADI_PCF_TWO_KS_SHIFT | (unsigned)rect_ks << RICADI_PCF_RECT_KS_SHIFT;
  }
};
// The cycle of level c on panels of width m.  blocks16: every group of the batch has BF16 blocks; gsr: group stride
// of the input; out32: only the FP32 copy of z is wanted; in16: the input is the FP16-stored vector (read where the
// cycle folds, on up to 16 columns).  The sweeps' operand precision is the level's (c->precond32).
static CycleForm cycle_form(const ricadi_ctx* c, int m, bool blocks16, size_t gsr, bool out32, bool in16) {
  CycleForm f;
  const size_t gs = (size_t)c->n * m;
  if (c->vanka) {
    // the unfolded cycle with the Vanka sweep: restriction and coarse apply as ever, everything after them in pc_vanka
    f.vanka = true;
    f.x32 = out32;
    f.first = f.FS_NONE;
    if (c->kc > 0) {
      const bool rowwave = m == 16 && c->sw.rowwave && spmm_rowwave_pays(c->kc, (size_t)c->n);
      f.restriction = rowwave ? f.RS_ROWWAVE : f.RS_CSR64;
      f.coarse = c->child ? f.CO_CHILD : c->sw.coarse_pipe && c->precond32 && rowwave ? f.CO_DENSE_KB : f.CO_DENSE;
    }
    return f;
  }
  // the pressure step -- pressure rows of r - (S Y) e, J product, Schur sweep -- as ONE launch for 16-column panels
  const bool fusedp = c->np > 0 && m == 16 && c->bs == 32;
  f.folded = c->kc > 0 && c->ady_ok && c->np > 0;
  f.h16 = in16 && f.folded && m <= 16;
  f.x32 = out32;
  // The velocity part between the three sweeps (first sweep -> pressure step's J product -> last sweep) as an FP32
  // panel: where only the FP32 copy of z is wanted anyway (the operator reads Z_j as stored), the first sweep writes
  // the velocity rows of z32 itself, the pressure step gathers 64-B instead of 128-B rows and the last sweep updates
  // them in place.  Rounding the intermediate to FP32 perturbs the (flexible) preconditioner by what its FP32
  // inverses and the FP32-stored Z_j already do.
  f.mid32 = c->sw.mid32 && out32 && fusedp && f.folded && c->gt_ok && c->precond32;
  // ... and on BF16-stored blocks where every shift of the batch has them (record-driven sweeps only)
  const bool recs = c->sw_stride > 0;   // the level has the sweeps' fixed-stride records
  f.b16 = f.mid32 && blocks16 && recs && c->bs == 32;
  if (c->kc > 0) {
    const bool rowwave = m == 16 && c->sw.rowwave && spmm_rowwave_pays(c->kc, c->sa ? c->pt_ci.n : (size_t)c->n);
    f.restriction = rowwave ? f.RS_ROWWAVE : f.h16 ? f.RS_CSR16 : f.RS_CSR64;
    // only where the dense inverse reads rc: a child level takes it as its row-major input
    f.coarse = c->child ? f.CO_CHILD : c->sw.coarse_pipe && c->precond32 && rowwave ? f.CO_DENSE_KB : f.CO_DENSE;
    f.sy = !f.folded ? f.SY_FULL : fusedp ? f.SY_NONE : f.SY_PROWS;
  }
  if (f.folded) {
    f.two_ks = c->ady_ks;
    // (the sweep adds no coarse part: the last sweep does)
    f.first = !block_two32_ok(c->bs, m, c->ady_ks, recs, false, gs, gsr, (size_t)c->kc * m) ? f.FS_TWO_TERM
              : f.b16 && c->sw.coarse_pipe ? f.FS_TWO32_PIPE : f.FS_TWO32;
  }
  if (c->np > 0) {
    f.pressure = !fusedp ? f.PS_SPLIT : f.b16 ? f.PS_FUSED16 : f.PS_FUSED;
    f.rect_ks = c->gt_ok ? c->gt_ks : 0;
    f.last = !c->gt_ok ? f.LS_CSR_IN
             : block_rect32_ok(c->bs, m, c->gt_ks, recs, (size_t)c->np * m, gs, f.mid32, out32) ? f.LS_RECT32
                                                                                                : f.LS_RECT;
  }
  return f;
}
// Does the GMRES iteration hand the preconditioner the FP16-stored vector (else: the FP64 copy)?
static bool precond_reads_h16(const ricadi_ctx* c, int m) { return cycle_form(c, m, false, 0, false, c->basis16).h16; }

// The panels of one application: input r (group stride gsr), or exactly where the form has h16 the same vector as
// stored in FP16 (r16, same stride; r is then not touched); output z (stride bt.gs) and its optional FP32 copy z32
// (stride gs32), written by the sweeps that write z last.
struct CycleIO {
  const double* r = nullptr;
  size_t gsr = 0;
  const _Float16* r16 = nullptr;
  double* z = nullptr;
  float* z32 = nullptr;
  size_t gs32 = 0;
};
// the coarse correction Y ec, added to the velocity rows by the sweep that writes them last
static ProlongArgs prolongation(const ricadi_ctx* c, const Batch& bt) {
  ProlongArgs pa;
  if (c->kc > 0) {
    pa.aggof = c->aggof.p;
    pa.ec = c->ec.p;
    pa.gse = bt.gsc;
  }
  return pa;
}
// the fixed-stride records of the velocity sweeps (of a level that has them: the form says so) with the input list at
// in_off
static SweepRecs sweep_records(const ricadi_ctx* c, int in_off) {
  return SweepRecs{c->sw_meta.p, c->sw_stride, in_off};
}
static void precond_apply(ricadi_ctx* c, const Batch& bt, const CycleForm& f, const CycleIO& io);

// The stages in the order of the cycle and of the timer classes pc_restrict .. pc_rect (Context.TK 10 - 16).  A stage
// the form does not have launches nothing.
static void pc_restrict(ricadi_ctx* c, const Batch& bt, const CycleForm& f, const CycleIO& io) {
  const int* rrp = c->sa ? c->pt_rp.p : c->agg_ptr.p;
  const int* rci = c->sa ? c->pt_ci.p : c->agg_rows.p;
  const GroupPtrs rvals = same_ptr(c->sa ? (const double*)c->pt_v.p : c->ones.p);
  if (f.restriction == f.RS_ROWWAVE)
    launch_spmm_rowwave(bt.st, bt.tab, c->kc, rrp, rci, rvals, io.r16 ? nullptr : io.r, io.r16, io.gsr, c->rc.p,
                        bt.gsc, bt.m, f.coarse == f.CO_DENSE_KB);
  else if (f.restriction == f.RS_CSR16)
    launch_spmm_h(bt.st, bt.tab, c->kc, rrp, rci, rvals, nullptr, io.r16, bt.m, io.gsr, c->rc.p, bt.m, bt.gsc,
                  nullptr, 0, 0, 1.0, 0.0, bt.m, 16);
  else if (f.restriction == f.RS_CSR64)
    restrict_csr(c, bt, io.r, io.gsr);
}
static void pc_coarse(ricadi_ctx* c, const Batch& bt, const CycleForm& f, const CycleIO&) {
  if (f.coarse == f.CO_CHILD) {
    // coarse problem by one cycle of the child level's preconditioner (a fixed linear operator)
    ricadi_ctx* ch = c->child.get();
    Batch cb = *bt.sub;
    cb.tab = bt.tab;
    cb.st = bt.st;
    cb.ng_solve = bt.ng_solve;
    precond_apply(ch, cb, cycle_form(ch, cb.m, cb.blocks16, bt.gsc, false, false),
                  CycleIO{c->rc.p, bt.gsc, nullptr, c->ec.p});
  } else if (f.coarse == f.CO_DENSE_KB) {
    launch_dense_apply_kb(bt.st, bt.tab, c->kc, bt.einv.f, c->rc.p, c->ec.p);
  } else if (f.coarse == f.CO_DENSE) {
    with_stored(c, false, [&](const auto& einv) {
      launch_dense_apply_b(bt.st, bt.tab, c->kc, bt.m, einv, c->rc.p, c->ec.p);
    }, bt.einv);
  }
}
static void pc_sy_prows(ricadi_ctx* c, const Batch& bt, const CycleForm& f, const CycleIO& io) {
  hipStream_t st = bt.st;
  const int nv = c->nv, m = bt.m;
  if (f.sy == f.SY_PROWS) {
    // only the PRESSURE rows of r - (S Y) ec are formed (short CSR product over np rows); the
    // velocity rows ride inside the first velocity sweep (block_apply2_kernel)
    if (io.r16)
      launch_spmm_h(st, bt.tab, c->np, c->sy_rp.p + nv, c->sy_ci.p, bt.syval, c->ec.p, nullptr, m, bt.gsc,
                    c->r2.p + (size_t)nv * m, m, bt.gs, io.r16 + (size_t)nv * m, m, io.gsr, -1.0, 1.0, m, c->sy_chunk);
    else
      launch_spmm_b(st, bt.tab, c->np, c->sy_rp.p + nv, c->sy_ci.p, bt.syval, c->ec.p, m, bt.gsc, nullptr,
                    c->r2.p + (size_t)nv * m, m, bt.gs, io.r + (size_t)nv * m, m, io.gsr, -1.0, 1.0, m, LowRankArgs(),
                    c->sy_chunk);
  } else if (f.sy == f.SY_FULL) {
    // Residual after the coarse correction, r2 = r - (S Y) ec, with the prolongated
    // operator (short rows over the L2-resident coarse vector) -- not a full saddle SpMM
    // through the prolongation map.  (Forming the velocity rows of r2 inside the first
    // velocity sweep instead, like the J^T product below, was measured slower: 249 vs
    // 257 shift-solves/s -- 8 rows x 7.6 dependent gathers per lane.)
    // Tile form: the aggregates a row block touches (a few dozen coarse rows) go to LDS once.
    if (c->syb_ok && (sy_tiled_ms(c, bt) || spmm_blocked_lds_bytes(m, c->syb_max_cols) <= (size_t)40 * 1024))
      sy_residual_tiled(c, bt, io.r, io.gsr);
    else
      launch_spmm_b(st, bt.tab, c->n, c->sy_rp.p, c->sy_ci.p, bt.syval, c->ec.p, m, bt.gsc, nullptr, c->r2.p, m,
                    bt.gs, io.r, m, io.gsr, -1.0, 1.0, m, LowRankArgs(), c->sy_chunk);
  }
}
static void pc_two_term(ricadi_ctx* c, const Batch& bt, const CycleForm& f, const CycleIO& io) {
  const int m = bt.m;
  if (f.first == f.FS_NONE) return;
  if (f.first == f.FS_PLAIN) {
    // on r2 (on r without a coarse level); without pressure rows this sweep writes z last
    const bool r2 = c->kc > 0;
    block_sweep(c, bt, false, r2 ? c->r2.p : io.r, r2 ? bt.gs : io.gsr, io.z, 0,
                c->np == 0 ? prolongation(c, bt) : ProlongArgs());
    return;
  }
  // z_v = Ahat^-1 r_v - (Ahat^-1 D) ec : first velocity sweep on the corrected residual without
  // ever writing it
  Seg2 s1, s2;
  s1.kstride = c->bs;
  s1.in = io.r16 ? nullptr : io.r;
  s1.in16 = io.r16;
  s1.gs = io.gsr;
  s2.iptr = c->cy_ptr.p;
  s2.irows = c->cy_cols.p;
  s2.kstride = c->ady_ks;
  s2.in = c->ec.p;
  s2.gs = bt.gsc;
  ProlongArgs pa;
  if (f.mid32) {
    pa.out32 = io.z32;
    pa.gs32 = io.gs32;
    pa.only32 = 1;
  }
  if (f.first == f.FS_TWO_TERM)
    with_stored(c, false, [&](const auto& m1, const auto& m2) {
      launch_block_apply2_b(bt.st, bt.tab, c->bs, c->nbv, c->bv_ptr.p, c->bv_rows.p, m1, s1, m2, s2, io.z, m, bt.gs, m,
                            pa);
    }, bt.bvinv, bt.adym);
  else
    with_stored<true>(c, f.first16(), [&](const auto& m1, const auto& m2) {
      launch_block_two32(bt.st, bt.tab, c->nbv, sweep_records(c, c->sw_in_two), m1, s1, m2, s2, io.z, bt.gs, pa,
                         f.first == f.FS_TWO32_PIPE);
    }, bt.bvinv, bt.adym);
}
// t = J z_v - r_p (r_p of r2, or of r without a coarse level)
static void pc_jprod(ricadi_ctx* c, const Batch& bt, const CycleForm& f, const CycleIO& io) {
  if (f.pressure != f.PS_SPLIT) return;
  const int m = bt.m;
  const bool r2 = c->kc > 0;
  launch_spmm_b(bt.st, bt.tab, c->np, c->J.rp.p, c->J.ci.p, same_ptr(c->J.v.p), io.z, m, bt.gs, nullptr, c->tp.p, m,
                bt.gsp, (r2 ? c->r2.p : io.r) + (size_t)c->nv * m, m, r2 ? bt.gs : io.gsr, 1.0, -1.0, m);
}
static void pc_schur(ricadi_ctx* c, const Batch& bt, const CycleForm& f, const CycleIO& io) {
  if (f.pressure == f.PS_NONE) return;
  const int nv = c->nv, m = bt.m;
  const size_t off = (size_t)nv * m;
  double* zp = io.z + off;
  // Fused variant: the pressure sweep writes z_p already WITH its coarse part and keeps
  // the plain z_p (the operand of the J^T product below) in tp -- in place: a wave
  // reads its block's rows of tp before it writes them, blocks are disjoint.
  ProlongArgs pa;
  pa.out2 = c->tp.p;
  pa.gs2 = bt.gsp;
  if (io.z32) {
    pa.out32 = io.z32 + off;
    pa.gs32 = io.gs32;
    pa.only32 = f.x32 && c->gt_ok;   // the rectangle sweep below completes the FP32 copy
  }
  if (c->kc > 0) {
    pa.aggof = c->aggof.p + nv;
    pa.ec = c->ec.p;
    pa.gse = bt.gsc;
  }
  if (f.pressure == f.PS_SPLIT) {
    block_sweep(c, bt, true, c->tp.p, bt.gsp, zp, 0, pa);
    return;
  }
  // r_p: of the folded cycle the input vector itself (FP64 or FP16-stored) with the coarse term formed in
  // the kernel; else the pressure rows of the corrected residual r2 (of r without a coarse level)
  const bool sy = f.folded, r2 = !sy && c->kc > 0;
  const double* rp64 = io.r16 ? nullptr : (r2 ? c->r2.p : io.r) + off;
  const _Float16* rp16 = io.r16 ? io.r16 + off : nullptr;
  const size_t gsrp = r2 ? bt.gs : io.gsr;
  // z_v: the FP32 panel where the first sweep left that (mid32; BF16 blocks come with it), else the rows of z
  with_stored<true>(c, f.pressure == f.PS_FUSED16, [&](const auto& inv) {
    launch_pressure_step_b(bt.st, bt.tab, c->nbp, c->ps_meta.p, inv, c->J.ci.p, c->J.v.p, io.z, bt.gs, sy, c->sy_ci.p,
                           bt.syval, c->ec.p, bt.gsc, rp64, rp16, gsrp, zp, bt.gs, pa, f.mid32 ? io.z32 : nullptr,
                           io.gs32);
  }, bt.bpinv);
}
// z_v -= Ahat^-1 (J^T z_p): the same block-Jacobi inverse as in the Schur blocks; the
// J^T product is formed inside the sweep, row by row as the blocks gather them
// (z_p is small and L2 resident), instead of through an intermediate panel.  It adds the coarse correction Y ec
// to the velocity rows of z (the pressure rows already carry theirs).
static void pc_rect(ricadi_ctx* c, const Batch& bt, const CycleForm& f, const CycleIO& io) {
  if (f.last == f.LS_NONE) return;
  const int m = bt.m;
  ProlongArgs pa = prolongation(c, bt);
  if (f.last == f.LS_CSR_IN) {
    // blocks that touch too many pressure dofs for the dense rectangles: the J^T product formed row by row inside
    // the sweep (CsrInArgs)
    CsrInArgs cin;
    cin.rp = c->JT.rp.p;
    cin.ci = c->JT.ci.p;
    cin.v = same_ptr(c->JT.v.p);
    cin.src = c->tp.p;
    cin.gss = bt.gsp;
    block_sweep(c, bt, false, nullptr, 0, io.z, 1, pa, cin);
    return;
  }
  // z_v -= G z_p with the per-shift blocks G_b = Ahat_b^-1 J^T[rows_b, pcols_b] formed at setup
  pa.out32 = io.z32;
  pa.gs32 = io.gs32;
  pa.only32 = f.x32;
  pa.old32 = f.mid32 ? 1 : 0;
  if (f.last == f.LS_RECT32)
    with_stored<true>(c, f.last16(), [&](const auto& g) {
      launch_block_rect32(bt.st, bt.tab, c->gt_ks, c->nbv, sweep_records(c, c->sw_in_rect), g, c->tp.p, bt.gsp, io.z,
                          bt.gs, 1, pa);
    }, bt.gtm);
  else
    with_stored(c, false, [&](const auto& g) {
      launch_block_apply_rect_b(bt.st, bt.tab, c->bs, c->gt_ks, c->nbv, c->bv_ptr.p, c->bv_rows.p, c->gt_ptr.p,
                                c->gt_cols.p, g, c->tp.p, m, bt.gsp, io.z, m, bt.gs, m, 1, pa);
    }, bt.gtm);
}
// The coloured Vanka sweep of a child level (CycleForm::vanka), colour after colour on the iterate as it stood
// before the colour:  rho = r - S z (the level's saddle product in its residual form, tiled or CSR as the level
// chooses), then z[idx_b] += omega Inv_b rho[idx_b] for every patch b of the colour -- two launches per colour.
// (One in-place kernel that forms its own residual rows would race: a patch reads columns of z that another patch
// of the same colour writes.)
static void vanka_colours(ricadi_ctx* c, const Batch& bt, const CycleIO& io) {
  const double omega = c->opts.child_damping;
  for (int col = 0; col < c->vk.ncolours; ++col) {
    const int p0 = c->vk.colour_ptr[col], cnt = c->vk.colour_ptr[col + 1] - p0;
    saddle_spmm(c, bt, io.z, bt.gs, nullptr, c->r2.p, bt.gs, io.r, io.gsr, -1.0, 1.0);
    with_stored(c, false, [&](const auto& inv) {
      launch_vanka_patch(bt.st, bt.tab, p0, cnt, c->vk_idx.p, inv, c->r2.p, bt.gs, io.z, bt.gs, bt.m, omega);
    }, bt.vkinv);
  }
}
static void pc_vanka(ricadi_ctx* c, const Batch& bt, const CycleForm& f, const CycleIO& io) {
  if (!f.vanka) return;
  // z = Y ec: the sweep adds to it (plain aggregation on a child level)
  launch_prolong_plain(bt.st, bt.tab, c->n, bt.m, c->kc > 0 ? c->aggof.p : nullptr, c->ec.p, bt.gsc, io.z, bt.gs);
  vanka_colours(c, bt, io);
}
using CycleStage = void (*)(ricadi_ctx*, const Batch&, const CycleForm&, const CycleIO&);
static const CycleStage cycle_stages[] = {pc_restrict, pc_coarse, pc_sy_prows, pc_two_term,
                                          pc_jprod,    pc_schur,  pc_rect,     pc_vanka};

// what an application of the cycle, or of one of its stages, does first
static void cycle_begin(ricadi_ctx* c, const CycleForm& f, const CycleIO& io) {
  c->mid32_last = f.mid32 ? 1 : 0;
  if (c->sa && !f.folded) throw HipError{"smoothed aggregation needs the folded preconditioner cycle"};
  if (!io.r16 != !f.h16) throw HipError{"FP16-stored input where the cycle form does not read it, or none"};
}
static void precond_apply(ricadi_ctx* c, const Batch& bt, const CycleForm& f, const CycleIO& io) {
  cycle_begin(c, f, io);
  for (CycleStage stage : cycle_stages) stage(c, bt, f, io);
  if (io.z32 && f.last != f.LS_RECT32 && f.last != f.LS_RECT)   // (the rectangle sweeps write z32 themselves)
    for (int i = 0; i < bt.tab.ng; ++i)
      launch_to_f32(bt.st, c->n, bt.m, io.z + (size_t)bt.tab.gid[i] * bt.gs, bt.m,
                    io.z32 + (size_t)bt.tab.gid[i] * io.gs32, bt.m);
}

static void op_apply(ricadi_ctx* c, ShiftData* sd, const double* x, double* y, int m, bool lowrank) {
  const Batch bt = make_batch(c, sd, m);
  op_apply(c, bt, x, bt.gs, y, lowrank);
}
static void precond_apply(ricadi_ctx* c, ShiftData* sd, const double* r, double* z, int m) {
  const Batch bt = make_batch(c, sd, m);
  precond_apply(c, bt, cycle_form(c, m, bt.blocks16, bt.gs, false, false), CycleIO{r, bt.gs, nullptr, z});
}

static void col_norms2(ricadi_ctx* c, const double* w, int nrows, int m, double* out) {
  launch_cols_dots(c->st, nrows, m, 0, nullptr, 0, w, 1, c->partial.p, out);
}

