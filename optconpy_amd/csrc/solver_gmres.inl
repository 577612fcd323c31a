// solver_gmres.inl -- lockstep batched GMRES, wide panels as column groups, recycled guesses, storage safety net, Sherman-Morrison-Woodbury.
// Part of ricadi_solver.hip (one translation unit; included there in order).

// ---- batched panel GMRES --------------------------------------------------------------
// Solves S(shift_g) x_g = b_g for the m columns of every group's n x m panel:
// one Arnoldi process per column, all groups in lockstep inside ONE sequence of
// launches (grid.z = active groups).  At n ~ 3e4 a single panel leaves most of
// the chip idle and the launch path dominates; batching the shifts of a sweep
// fills it.  Right preconditioning, CGS2 (on the hot path in its one-reduction,
// delayed form: DESIGN.md 3a), per-column Givens QR.  A group whose columns have
// all converged leaves the active table; its correction is formed at the end of
// the restart cycle from the basis vectors it had by then.
//   b: group stride gsb (0 = one right-hand side shared by all groups);
//   x: group stride n*m, overwritten.
struct GmresResult {
  int iters = 0;
  bool converged = false;
  bool stalled = false;       // gave up before gmres_maxit: three full-length cycles in a row gained < 30 %
  double max_relres = 0.0;
};

// What one lockstep GMRES iteration launches: the single place that decides it (gmres_core and the kernel
// timers of solver_capi.inl both ask here).
struct IterationForm {
  bool b16 = false, b32 = false;   // Krylov basis stored in FP16 / FP32 (neither: FP64)
  bool h16 = false;     // the preconditioner reads the current vector from the FP16 basis; its FP64 copy is not written
  bool keepw = false;   // w is not rewritten between the two Gram-Schmidt passes: the final update subtracts
                        // V (h1 + h2) from the original w
  bool fuseh = false;   // last Arnoldi pass and Hessenberg update in ONE launch (K3h)
  bool x32 = false;     // the operator reads the FP32-stored Z_j
  bool w32 = false;     // ... and writes w = S z_j as an FP32 panel, which the three Arnoldi passes read
  bool lowsync = false; // one-reduction (delayed CGS2) Arnoldi: dots, reduction, update per iteration (three launches,
                        // not five), three more at the end of a cycle
};
static IterationForm iteration_form(const ricadi_ctx* c, int m, int G, bool lowrank) {
  const int restart = c->opts.gmres_restart;
  IterationForm f;
  f.b16 = c->basis16;
  f.b32 = c->basis32 && !f.b16;
  f.h16 = precond_reads_h16(c, m);
  f.keepw = update_dots_keeps_w(m, f.b16, restart);
  f.fuseh = c->sw.fuseh && update_hess_fused_ok(m, f.b16);   // (RICADI_FUSEH=0: the separate Hessenberg kernel)
  // FP32 operator input for a batch of G groups: always with the multi-shift kernel; with one workgroup per (row
  // block, group) the FP32 input by itself measured 1.4 % slower at cfg2 in round 3, but it is what lets the cycle
  // keep its velocity part in FP32 and its blocks in BF16 (round 4), which more than pays for it (RICADI_X32=0: only
  // with the multi-shift kernel; there the launches are bandwidth bound: cfg5 K1 1252 -> 1150 us per launch, cycle
  // +2 %).  Not with the low-rank term.
  f.x32 = saddle_tiled(c, m) && (c->sw.x32_always || ms_pays(c, G, c->snnz)) && !(lowrank && c->q > 0);
  // the tile kernels with FP32 input write the FP32 panel, the three 16-column passes on the FP16-stored basis read
  // it (RICADI_W32=0: FP64 panel)
  f.w32 = f.x32 && c->sw.w32 && m == 16 && f.b16 && f.fuseh && f.keepw && arnoldi16_w32_ok(restart);
  // ... and there the one-reduction Arnoldi (RICADI_ARNOLDI=cgs2: the three passes)
  f.lowsync = f.w32 && f.h16 && c->sw.lowsync && arnoldi16_lowsync_ok(restart);
  return f;
}
// fn(basis) with the Krylov basis as stored: _Float16*, float* or double*
template <class Fn>
static void with_basis(ricadi_ctx* c, const IterationForm& f, Fn&& fn) {
  if (f.b16) fn(reinterpret_cast<_Float16*>(c->basisf.p));
  else if (f.b32) fn(c->basisf.p);
  else fn(c->basis.p);
}

// fn(w) with the operator's output panel as stored: float* (f.w32) or double*
template <class Fn>
static void with_panel(ricadi_ctx* c, const IterationForm& f, Fn&& fn) {
  if (f.w32) fn(c->wv32.p);
  else fn(c->wv.p);
}

// The Arnoldi passes of iteration nvec - 1 on the workspace panels (w = S z_j in wv / wv32, coefficients in h1 / h2),
// for the groups of bt.tab.  Strides as in gmres_core.
struct ArnoldiStrides {
  size_t nm, vs, gsh, gspart, h2buf;
  ArnoldiStrides(const ricadi_ctx* c, const Batch& bt)
      : nm(bt.gs), vs(bt.gs * bt.G), gsh((size_t)(c->opts.gmres_restart + 2) * bt.m),
        gspart((size_t)dots_num_blocks(c->n) * (c->opts.gmres_restart + 2) * bt.m),
        h2buf((size_t)(c->opts.gmres_restart + 2) * c->wcols) {}
};
// column norms squared of a panel (group stride gsw) for the groups of bt.tab: out[g * m + j]
static void panel_norms2(ricadi_ctx* c, const Batch& bt, const double* w, size_t gsw, double* out) {
  launch_cols_dots_b(bt.st, bt.tab, c->n, bt.m, 0, (const double*)nullptr, 0, 0, w, gsw, 1, c->partial.p,
                     ArnoldiStrides(c, bt).gspart, out, (size_t)bt.m);
}
// first pass: h1 = V^T w
static void arnoldi_dots(ricadi_ctx* c, const IterationForm& f, const Batch& bt, int nvec) {
  const ArnoldiStrides s(c, bt);
  with_basis(c, f, [&](auto* V) {
    with_panel(c, f, [&](auto* w) {
      launch_cols_dots_b(bt.st, bt.tab, c->n, bt.m, nvec, V, s.vs, s.nm, w, s.nm, 0, c->partial.p, s.gspart, c->h1.p,
                         s.gsh);
    });
  });
}
// first update fused with the dot products of the second pass: w -= V h1, h2 = V^T w (and ||w||^2)
static void arnoldi_update_dots(ricadi_ctx* c, const IterationForm& f, const Batch& bt, int nvec) {
  const ArnoldiStrides s(c, bt);
  with_basis(c, f, [&](auto* V) {
    with_panel(c, f, [&](auto* w) {
      launch_cols_update_dots_b(bt.st, bt.tab, c->n, bt.m, nvec, V, s.vs, s.nm, c->h1.p, s.gsh, w, s.nm, f.keepw,
                                c->partial.p, s.gspart, c->h2.p, s.gsh);
    });
  });
}
// last update: v_{j+1} = scale (w - V h2), stored in the basis (fuseh: with the Hessenberg / Givens update of
// iteration j = nvec - 1 in the same launch; the residual estimates also go to host_resid)
static void arnoldi_update(ricadi_ctx* c, const IterationForm& f, const Batch& bt, int nvec, double* host_resid) {
  const ArnoldiStrides s(c, bt);
  const int j = nvec - 1, m = bt.m;
  const size_t resbuf = (size_t)c->wcols;                    // doubles between the two residual-estimate buffers
  double* vcur = f.h16 ? nullptr : c->vcur.p;
  if (f.fuseh) {
    _Float16* Vh = reinterpret_cast<_Float16*>(c->basisf.p);
    with_panel(c, f, [&](auto* w) {
      launch_cols_update16_hess_b(bt.st, bt.tab, c->n, nvec, Vh, s.vs, s.nm, c->h1.p, c->h2.p, s.gsh, f.keepw ? 1 : 0,
                                  w, s.nm, vcur, s.nm, Vh + (size_t)nvec * s.vs, s.nm, j, c->opts.gmres_restart, c->H.p,
                                  c->cs.p, c->sn.p, c->g.p, c->resid.p + (size_t)(j & 1) * resbuf,
                                  c->resid.p + (size_t)((j + 1) & 1) * resbuf, c->bnorm2.p, c->opts.gmres_tol,
                                  host_resid);
    });
    return;
  }
  const double* h = f.keepw ? c->h2.p + s.h2buf : c->h2.p;
  with_basis(c, f, [&](auto* V) {
    if constexpr (std::is_same<std::remove_pointer_t<decltype(V)>, double>::value)
      launch_cols_update_b(bt.st, bt.tab, c->n, m, nvec, V, s.vs, s.nm, h, s.gsh, -1.0, c->wv.p, s.nm, c->scale.p,
                           V + (size_t)nvec * s.vs, s.nm);
    else
      launch_cols_update_b(bt.st, bt.tab, c->n, m, nvec, V, s.vs, s.nm, h, s.gsh, -1.0, c->wv.p, s.nm, c->scale.p,
                           vcur, s.nm, V + (size_t)nvec * s.vs, s.nm);
  });
}

// One-reduction Arnoldi (f.lowsync).  dots of iteration j (end_of_cycle: without w, j = k_g per group, and the
// completion of column k_g - 1), update of iteration j (completes column j-1, provisional residual estimate of
// column j into host_resid, v_j into slot j, the next candidate u_{j+1} into slot j+1).
static void arnoldi_lowsync_dots(ricadi_ctx* c, const Batch& bt, const GroupInts& js, bool end_of_cycle) {
  const ArnoldiStrides s(c, bt);
  const int restart = c->opts.gmres_restart;
  launch_arnoldi16_lowsync_dots(bt.st, bt.tab, js, c->n, reinterpret_cast<_Float16*>(c->basisf.p), s.vs, s.nm,
                                end_of_cycle ? nullptr : c->wv32.p, s.nm, c->ls_partial.p,
                                lowsync_partial_stride(c->n, restart), c->ls_coef.p, lowsync_coef_stride(restart));
  if (end_of_cycle)
    launch_arnoldi16_lowsync_close(bt.st, bt.tab, js, c->ls_coef.p, lowsync_coef_stride(restart), restart, c->H.p,
                                   c->cs.p, c->sn.p, c->g.p, c->bnorm2.p, c->opts.gmres_tol);
}
static void arnoldi_lowsync_update(ricadi_ctx* c, const Batch& bt, int j, double* host_resid) {
  const ArnoldiStrides s(c, bt);
  const int restart = c->opts.gmres_restart;
  launch_arnoldi16_lowsync_update(bt.st, bt.tab, c->n, j, reinterpret_cast<_Float16*>(c->basisf.p), s.vs, s.nm,
                                  c->wv32.p, s.nm, c->ls_coef.p, lowsync_coef_stride(restart), restart, c->H.p,
                                  c->cs.p, c->sn.p, c->g.p, c->bnorm2.p, c->opts.gmres_tol,
                                  c->resid.p + (size_t)(j & 1) * c->wcols, host_resid);
}

// The Arnoldi phase of lockstep iteration j on w = S z_j (in wv / wv32, as f says) for the groups of bt.tab
// (iteration_launches and the step probe of solver_capi.inl): column j of the Hessenberg matrix, its rotation, the
// residual estimates (also to host_resid, may be null) and the next Krylov vector.
static void arnoldi_launches(ricadi_ctx* c, const IterationForm& f, const Batch& bt, int j, double* host_resid) {
  if (f.lowsync) {
    // slot j holds the candidate u_j the preconditioner read; v_j replaces it, u_{j+1} goes to slot j + 1
    arnoldi_lowsync_dots(c, bt, same_int(j), false);
    arnoldi_lowsync_update(c, bt, j, host_resid);
  } else {
    const int restart = c->opts.gmres_restart;
    arnoldi_dots(c, f, bt, j + 1);
    arnoldi_update_dots(c, f, bt, j + 1);
    if (!f.fuseh)
      launch_gmres_hess_b(bt.st, bt.tab, bt.m, j, restart, c->h1.p, c->h2.p, c->H.p, c->cs.p, c->sn.p, c->g.p,
                          c->scale.p, c->resid.p, c->bnorm2.p, c->opts.gmres_tol, host_resid,
                          f.keepw ? c->h2.p + (size_t)(restart + 2) * c->wcols : nullptr);
    arnoldi_update(c, f, bt, j + 1, host_resid);
  }
}

// Start of a restart cycle for the groups of bt.tab, from their residual panels in wv: norms, g = [||r||, 0 ..],
// scale = 1 / ||r||, then -- after decide(), which may narrow bt.tab from the norms (false: no group goes on, nothing
// more is launched) -- the first Krylov vector, the scaled residual, into slot 0 (LockstepSolve::begin_cycle and
// the probe).
template <class Decide>
static bool cycle_start_launches(ricadi_ctx* c, const IterationForm& f, Batch& bt, Decide&& decide) {
  const size_t nm = bt.gs;
  panel_norms2(c, bt, c->wv.p, nm, c->nrm2.p);
  launch_gmres_start_b(bt.st, bt.tab, bt.m, c->opts.gmres_restart, c->nrm2.p, c->g.p, c->scale.p, c->resid.p);
  if (!decide()) return false;
  with_basis(c, f, [&](auto* V) {
    if constexpr (std::is_same<std::remove_pointer_t<decltype(V)>, double>::value)
      launch_colscale_b(bt.st, bt.tab, c->n, bt.m, c->scale.p, c->wv.p, nm, 0.0, V, nm);
    else
      launch_colscale_b(bt.st, bt.tab, c->n, bt.m, c->scale.p, c->wv.p, nm, 0.0, c->vcur.p, nm, V, nm);
  });
  return true;
}

// End of a restart cycle for the groups of bt.tab: x_g += Z_g y_g with the kk.v[g] preconditioned vectors group g
// built, R y = g per column (one launch each for all groups, k_g by value; end_cycle and the probe).
static void cycle_end_launches(ricadi_ctx* c, const IterationForm& f, const Batch& bt, const GroupInts& kk, double* x) {
  const int restart = c->opts.gmres_restart;
  const size_t nm = bt.gs, vs = nm * bt.G;
  // one-reduction form: the last column of every group still waits for the correction of its candidate u_{k_g}
  if (f.lowsync) arnoldi_lowsync_dots(c, bt, kk, true);
  launch_gmres_backsolve_b(bt.st, bt.tab, bt.m, kk, restart, c->H.p, c->g.p, c->yv.p);
  launch_cols_update_bk(bt.st, bt.tab, c->n, bt.m, kk, c->zbasisf.p, vs, nm, c->yv.p, (size_t)restart * bt.m, x, nm, x,
                        nm);
}

// The launches of lockstep iteration j for the groups of bt.tab, on bt.st (gmres_core and the kernel timers):
// preconditioner, operator, Arnoldi.  Residual estimates of the iteration also go to host_resid (may be null).
static void iteration_launches(ricadi_ctx* c, const IterationForm& f, const CycleForm& pf, const Batch& bt, int j,
                               bool lowrank, double* host_resid) {
  const size_t nm = bt.gs, vs = nm * bt.G;
  const double* vj = (f.b32 || f.b16) ? c->vcur.p : c->basis.p + (size_t)j * vs;
  _Float16* Vh = reinterpret_cast<_Float16*>(c->basisf.p);   // FP16 storage shares the FP32 buffer
  // flexible form: Z_j = P^-1 v_j is kept (FP32), the cycle's correction is x += Z y -- no
  // preconditioner application at the cycle end, and P may differ from step to step
  // ... and the operator reads that stored FP32 copy (half the bytes of the x gathers; S Z_j = V H then
  // holds for exactly the vectors the correction uses), so the sweeps need not store the FP64 z at all
  float* zj = c->zbasisf.p + (size_t)j * vs;
  precond_apply(c, bt, pf, CycleIO{vj, nm, f.h16 ? Vh + (size_t)j * vs : nullptr, c->zv.p, zj, nm});
  op_apply(c, bt, c->zv.p, nm, c->wv.p, lowrank, f.x32 ? zj : nullptr, f.w32 ? c->wv32.p : nullptr);
  arnoldi_launches(c, f, bt, j, host_resid);
}

// ---- two half-batches on two streams ----------------------------------------------------
// The groups of a lockstep batch are independent Arnoldi processes and every buffer the iteration writes is indexed
// by group id, so the batch can go through the same launch sequence as two halves on two streams: the GPU then runs
// a VALU / LDS / gather bound launch of one half (saddle SpMM, restriction, pressure step) beside an FP64-MFMA bound
// one of the other (coarse apply, first sweep), and each half's launch boundaries hide behind the other's kernels
// (DESIGN.md 6a).  Every kernel sums a group in an order that does not depend on the other groups of its launch, so
// the split changes no bit of the results.  The second stream (non-blocking) lives in the context.
// Fewer live groups than this run on one stream: halves of 1 - 2 groups are latency-bound chains whose launches
// measured slower side by side than as one table (cfg2: 4 groups +10 %, 2 groups +25 % per iteration; 8 groups -8 %).
constexpr int kSplitMinGroups = 8;
static hipStream_t half_stream(ricadi_ctx* c) {
  if (!c->st_half) {
    HIPCHK(hipStreamCreateWithFlags(&c->st_half, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) HIPCHK(hipEventCreateWithFlags(&c->ev_res_half[i], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  }
  return c->st_half;
}
// Does the lockstep solve of G groups run as two halves?  Not with a child level (the child's cycle has not been
// audited for scratch shared across groups), not with the low-rank operator term (its coefficient panel lrc is cleared
// for all groups at once and summed with atomics), and only where it was measured to pay: up to n = 2e5 (cfg2, n = 3e4:
// -9 % per 16-group iteration; cfg3, n = 5e4: -5 % per step; cfg5, n = 5e5: +1.1 .. +1.8 % per iteration at 4 - 16
// groups, where every launch already fills the chip).
static bool split_halves(const ricadi_ctx* c, int G, bool lowrank) {
  return c->sw.split && G >= kSplitMinGroups && !c->child && !(lowrank && c->q > 0) && c->n <= 200000;
}
// The halves of the active groups: alternating positions in the order of the groups' iteration counts in their
// previous solve (slowest first; every ADI sweep repeats the same shifts), else in the caller's order (a sorted shift
// list: neighbours need similar counts).  Either way each half gets a mix of slow and fast shifts, and the two slowest
// land in different halves.
static void split_groups(ShiftData* const* sds, const std::vector<int>& act, std::vector<int> (&half)[2]) {
  std::vector<int> ord = act;
  bool known = true;
  for (int g : act) known = known && sds[g]->last_iters >= 0;
  if (known)
    std::stable_sort(ord.begin(), ord.end(),
                     [&](int a, int b) { return sds[a]->last_iters > sds[b]->last_iters; });
  half[0].clear();
  half[1].clear();
  for (size_t i = 0; i < ord.size(); ++i) half[i & 1].push_back(ord[i]);
  // group ids in increasing order within a half, as in the one-stream table
  std::sort(half[0].begin(), half[0].end());
  std::sort(half[1].begin(), half[1].end());
}
namespace {   // (file-local types: no symbols of theirs leave the library)
// The schedule of the two halves (gmres_core and the split-iteration timer): half h on bh[h].st -- half 0 on the
// context's stream -- with the lag event pair lag_events(h).  The caller fills half[] (split_groups, or lists of its
// own), forks, sets the tables for the groups that are live, issues iterations and joins; between a join and the next
// fork everything runs on the context's stream.  With enabled == false (split_halves said no) nothing of the second
// stream is created or touched.
struct HalfSchedule {
  ricadi_ctx* c;
  const bool enabled;
  std::vector<int> half[2];    // group ids of the halves
  Batch bh[2];                 // the solve's batch on the stream of half h, table: the live groups of the half
  bool forked = false;

  HalfSchedule(ricadi_ctx* ctx, const Batch& bt, bool enable) : c(ctx), enabled(enable), bh{bt, bt} {
    if (enabled) bh[1].st = half_stream(c);
  }
  hipEvent_t* lag_events(int h) const { return h == 1 && enabled ? c->ev_res_half : c->ev_res; }
  // two halves for this many groups?
  bool pays(size_t ngroups) const { return enabled && ngroups >= (size_t)kSplitMinGroups; }
  // the second stream starts behind what the context's stream has been given so far
  void fork() {
    HIPCHK(hipEventRecord(c->ev_fork, bh[0].st));
    HIPCHK(hipStreamWaitEvent(bh[1].st, c->ev_fork, 0));
    forked = true;
  }
  // tables of the halves: their groups that are in `live`; the multi-shift kernels' choice follows the groups of
  // the whole solve
  void set_live(const std::vector<int>& live) {
    for (int h = 0; h < 2; ++h) {
      std::vector<int> lh;
      for (int g : half[h])
        if (std::find(live.begin(), live.end(), g) != live.end()) lh.push_back(g);
      bh[h].set(lh);
      bh[h].ng_solve = (int)live.size();
    }
  }
  // iteration j on both halves; lag >= 0: that event of each half's pair is recorded behind the half's launches
  void issue(const IterationForm& f, const CycleForm& pf, int j, bool lowrank, double* host_resid, int lag = -1) {
    for (int h = 0; h < 2; ++h) {
      if (bh[h].tab.ng > 0) iteration_launches(c, f, pf, bh[h], j, lowrank, host_resid);
      if (lag >= 0) HIPCHK(hipEventRecord(lag_events(h)[lag], bh[h].st));
    }
  }
  // the context's stream goes on behind what the second stream has been given (no-op unless forked)
  void join() {
    if (!forked) return;
    HIPCHK(hipEventRecord(c->ev_join, bh[1].st));
    HIPCHK(hipStreamWaitEvent(bh[0].st, c->ev_join, 0));
    forked = false;
  }
};

// The lockstep solve as restart cycles (gmres_core drives the phases):  begin_cycle -- true residual of the iterates,
// who converged / hit maxit / stalled, the next cycle's length, first Krylov vector of the groups that go on;
// iterate_cycle -- up to cyc lockstep iterations, the host looking at the residual estimates one iteration late;
// end_cycle -- x += Z y.
struct LockstepSolve {
  ricadi_ctx* const c;
  ShiftData* const* const sds;
  const int G, m;
  const double* const b;
  const size_t gsb;
  double* const x;
  const bool lowrank, allow_stall;
  GmresResult* const res;
  const std::vector<int>* const only;
  const hipStream_t st;
  const int restart, maxit;
  const double tol;
  Batch bt;
  const size_t nm, vs;           // one panel; one Krylov vector of all groups
  const int GM;
  const IterationForm f;
  const CycleForm pf;
  HalfSchedule halves;
  // pinned host slots: [0] true residuals, [1] right-hand side norms, [2], [3] the iterations' residual estimates
  double* const hb;
  const size_t slot = (size_t)RICADI_MAX_M * RICADI_MAX_GROUPS;
  std::vector<double> bn;        // ||b|| per column
  std::vector<double> rstart;    // residual per column at the start of the previous cycle
  std::vector<int> act;          // groups of the current cycle
  std::vector<int> live;         // ... of them, still iterating
  GroupInts kk;                  // Krylov vectors group g built in the current cycle (by value to the cycle's close)
  std::vector<int> nstall;       // full-length cycles in a row that gained < 30 % on some column of group g
  bool first;                    // the iterates are zero: the first residual is b
  // Cycle length: short cycles keep the Krylov basis (the dominant HBM traffic of an
  // iteration: three passes over it) small; a cycle that gains less than a factor 10
  // on some column lengthens the following ones, up to gmres_restart.
  int cyc;
  Tick tick;

  // (after ensure_work, which decides the storage of the basis)
  LockstepSolve(ricadi_ctx* ctx, ShiftData* const* sds_, int G_, const double* b_, size_t gsb_, double* x_, int m_,
                bool lowrank_, GmresResult* res_, bool have_x0, const std::vector<int>* only_, bool allow_stall_)
      : c(ctx), sds(sds_), G(G_), m(m_), b(b_), gsb(gsb_), x(x_), lowrank(lowrank_), allow_stall(allow_stall_),
        res(res_), only(only_), st(ctx->st), restart(ctx->opts.gmres_restart), maxit(ctx->opts.gmres_maxit),
        tol(ctx->opts.gmres_tol), bt(make_batch(ctx, sds_, G_, m_)), nm(bt.gs), vs(nm * G_), GM(G_ * m_),
        f(iteration_form(ctx, m_, G_, lowrank_)), pf(cycle_form(ctx, m_, bt.blocks16, nm, f.x32, f.h16)),
        halves(ctx, bt, split_halves(ctx, G_, lowrank_)), hb(ctx->h_resid), bn(GM), rstart(GM, 0.0), nstall(G_, 0), first(!have_x0), cyc(std::min(restart, 10)) {
    c->w32_last = f.w32 ? 1 : 0;
    for (int g = 0; g < G; ++g) res[g] = GmresResult();
    if (only) act = *only;
    else
      for (int g = 0; g < G; ++g) act.push_back(g);
  }

  void lap(double& acc) {
    if (c->sw.timing) {
      (void)hipStreamSynchronize(st);
      if (halves.enabled) (void)hipStreamSynchronize(halves.bh[1].st);
      acc += tick.lap();
    }
  }

  // norms of the right-hand sides: host (bn) and device (bnorm2, not squared, for the Hessenberg kernels); x = 0
  // without an initial guess
  void rhs_norms() {
    bt.all();
    panel_norms2(c, bt, b, gsb, c->bnorm2.p);
    HIPCHK(hipMemcpyAsync(hb + slot, c->bnorm2.p, sizeof(double) * GM, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int j = 0; j < GM; ++j) bn[j] = std::sqrt(std::max(hb[slot + j], 0.0));
    HIPCHK(hipMemcpyAsync(c->bnorm2.p, bn.data(), sizeof(double) * GM, hipMemcpyHostToDevice, st));
    if (first) HIPCHK(hipMemsetAsync(x, 0, sizeof(double) * vs, st));
    tick = Tick();
  }

  // all columns of group g at the tolerance in the residuals r?  (records the group's worst relative residual)
  bool group_converged(const double* r, int g) {
    double worst = 0.0;
    bool ok = true;
    for (int j = g * m; j < (g + 1) * m; ++j) {
      const double rel = bn[j] > 0.0 ? r[j] / bn[j] : 0.0;
      worst = std::max(worst, rel);
      if (!(r[j] <= tol * bn[j])) ok = false;
    }
    res[g].max_relres = worst;
    return ok;
  }

  // The decision at a cycle start, from the true residuals r of the groups of act (host): a group is done when it
  // has converged, has used maxit iterations, or -- allow_stall -- three full-length cycles in a row gained less
  // than 30 % on one of its columns.  Returns the groups that go on; a column that gained less than a factor 10
  // lengthens the cycles from here on.  Launches nothing.
  std::vector<int> next_active(const double* r) {
    std::vector<int> next;
    bool slow = false;
    for (int g : act) {
      if (group_converged(r, g)) {
        res[g].converged = true;
      } else if (res[g].iters < maxit) {
        bool flat = false;
        for (int j = g * m; j < (g + 1) * m; ++j) {
          if (rstart[j] > 0.0 && r[j] > tol * bn[j] && r[j] > 0.1 * rstart[j]) slow = true;
          if (rstart[j] > 0.0 && r[j] > tol * bn[j] && r[j] > 0.7 * rstart[j]) flat = true;
          rstart[j] = r[j];
        }
        nstall[g] = (flat && cyc >= restart) ? nstall[g] + 1 : 0;
        if (allow_stall && nstall[g] >= 3) {
          res[g].stalled = true;
          ++c->trace.stalled_groups;
        } else {
          next.push_back(g);
        }
      } else {
        ++c->trace.maxit_groups;
      }
    }
    if (slow) cyc = std::min(restart, cyc + (cyc + 1) / 2);
    return next;
  }

  // r = b - S x of the groups of bt.tab into wv (the first time without an initial guess: r = b, all groups)
  void residual() {
    if (first) {
      if (gsb == nm) {
        HIPCHK(hipMemcpyAsync(c->wv.p, b, sizeof(double) * vs, hipMemcpyDeviceToDevice, st));
      } else {
        for (int g = 0; g < G; ++g)
          HIPCHK(hipMemcpyAsync(c->wv.p + (size_t)g * nm, b + (size_t)g * gsb, sizeof(double) * nm,
                                hipMemcpyDeviceToDevice, st));
      }
    } else if (lowrank && c->q > 0) {
      op_apply(c, bt, x, nm, c->wv.p, lowrank);
      launch_axpby_b(st, bt.tab, nm, 1.0, b, gsb, -1.0, c->wv.p, nm);
    } else {
      // r = b - S x in one launch (the residual form of the SpMM)
      saddle_spmm(c, bt, x, nm, nullptr, c->wv.p, nm, b, gsb, -1.0, 1.0);
    }
    first = false;
  }

  // false: no group goes on
  bool begin_cycle() {
    if (act.empty()) return false;
    lap(c->t_iter);
    bt.set(act);
    residual();
    // who goes on is decided on the host from the residual norms; their first Krylov vector: the scaled residual
    const bool go = cycle_start_launches(c, f, bt, [&] {
      HIPCHK(hipMemcpyAsync(hb, c->resid.p, sizeof(double) * GM, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      act = next_active(hb);
      bt.set(act);
      return !act.empty();
    });
    if (!go) return false;
    live = act;
    kk = same_int(0);
    ++c->trace.cycles;
    c->trace.cycle_len_last = cyc;
    c->trace.cycle_len_max = std::max<int64_t>(c->trace.cycle_len_max, cyc);
    return true;
  }

  void iterate_cycle() {
    // one cycle schedule for both halves; the second stream starts behind what the first has issued so far, and is
    // joined back as soon as too few groups are left for two halves
    const bool two = halves.pays(act.size());
    if (two) {
      split_groups(sds, act, halves.half);
      halves.fork();
    }
    lap(c->t_cyc);
    for (int j = 0; j < cyc && !live.empty(); ++j) {
      // The residual estimates also go straight to a pinned host slot behind a lag event; the host looks at the
      // PREVIOUS iteration's slot, so it never drains the streams (at most one surplus Arnoldi step per group).
      double* cur = hb + 2 * slot + (size_t)(j & 1) * slot;
      if (!halves.pays(live.size())) halves.join();
      if (halves.forked) {
        halves.set_live(live);
        halves.issue(f, pf, j, lowrank, cur, j & 1);
      } else {
        bt.set(live);
        iteration_launches(c, f, pf, bt, j, lowrank, cur);
        HIPCHK(hipEventRecord(c->ev_res[j & 1], st));
      }
      for (int g : live) {
        ++res[g].iters;
        kk.v[g] = j + 1;
      }
      // who iterates on: not at maxit, and -- by the estimates of iteration j - 1, which have arrived behind their
      // lag events -- not converged
      std::vector<int> still;
      if (j >= 1) {
        HIPCHK(hipEventSynchronize(c->ev_res[(j - 1) & 1]));
        // (the second half's: recorded up to the join; done since)
        if (two) HIPCHK(hipEventSynchronize(halves.lag_events(1)[(j - 1) & 1]));
        const double* prev = hb + 2 * slot + (size_t)((j - 1) & 1) * slot;
        for (int g : live)
          if (!group_converged(prev, g) && res[g].iters < maxit) still.push_back(g);
      } else {
        for (int g : live)
          if (res[g].iters < maxit) still.push_back(g);
      }
      live.swap(still);
    }
    // the second stream's iterations are complete before the corrections (and before anything after the solve)
    halves.join();
    lap(c->t_iter);
  }

  // corrections: x_g += Z_g y_g with the k_g preconditioned vectors group g built
  // (one launch each for all groups of the cycle, k_g per group by value)
  void end_cycle() {
    bt.set(act);
    cycle_end_launches(c, f, bt, kk, x);
    lap(c->t_cyc);
  }

  void finish() {
    lap(c->t_cyc);
    for (int g = 0; g < G; ++g)
      if (!only || std::find(only->begin(), only->end(), g) != only->end()) sds[g]->last_iters = res[g].iters;
  }
};

}  // namespace

// have_x0: x holds an initial guess (else it is zeroed);  only: the groups to iterate on (NULL = all; the
// panels of the other groups are not touched);  allow_stall: a group whose full-length restart cycles no
// longer gain is given up early (the caller repeats it with wider storage).
static void gmres_core(ricadi_ctx* c, ShiftData* const* sds, int G, const double* b, size_t gsb, double* x,
                       int m, bool lowrank, GmresResult* res, bool have_x0, const std::vector<int>* only,
                       bool allow_stall) {
  ensure_work(c, m, G, 0);
  LockstepSolve s(c, sds, G, b, gsb, x, m, lowrank, res, have_x0, only, allow_stall);
  s.rhs_norms();
  while (s.begin_cycle()) {
    s.iterate_cycle();
    s.end_cycle();
  }
  s.finish();
}

// ---- wide panels as sixteen-column groups -------------------------------------------------------
// The columns of a panel are independent Arnoldi processes (per-column Givens), so an n x m panel with
// m > 32 -- the time-varying Riccati loop's [M^T Z_c, sqrt(tau) C~^T, K_k] of up to comprz_maxc + NY' + NU
// columns, solve_dae_ric.py:149 of the reference -- is solved as groups of 16 columns of the SAME shift in
// the lockstep batch: every kernel tuned for the 16-column case (LDS-tiled SpMM, 16-byte Arnoldi kernels,
// fused pressure step, FP16 vector input) then carries the iteration instead of the generic-width ones.
// The shifts of the call are walked in chunks of floor(RICADI_MAX_GROUPS / groups per shift); the column
// groups are scattered into / gathered from group-major panels (pad columns are zero: a zero column is
// inert in every kernel of the iteration).  RICADI_WIDE_SPLIT=0 keeps the wide panels whole.
static void gmres_core_any(ricadi_ctx* c, ShiftData* const* sds, int G, const double* b, size_t gsb, double* x,
                           int m, bool lowrank, GmresResult* res, bool have_x0, const std::vector<int>* only,
                           bool allow_stall) {
  const int W0 = wide_split_width(c, m);
  if (!W0) {
    gmres_core(c, sds, G, b, gsb, x, m, lowrank, res, have_x0, only, allow_stall);
    return;
  }
  hipStream_t st = c->st;
  const int n = c->n;
  const size_t nm = (size_t)n * m;
  std::vector<int> todo;
  if (only) todo = *only;
  else
    for (int g = 0; g < G; ++g) todo.push_back(g);
  for (int g = 0; g < G; ++g) res[g] = GmresResult();
  for (int s : todo) res[s].converged = true;
  // (ensure_work of the caller reserved a full chunk; growing the workspace here would free the buffer b lives in)
  if (c->wcols < W0 * RICADI_MAX_GROUPS) throw HipError{"workspace not sized for the column groups of a wide panel"};
  c->split_b.ensure((size_t)n * W0 * RICADI_MAX_GROUPS);
  c->split_x.ensure((size_t)n * W0 * RICADI_MAX_GROUPS);
  // columns [col0, col0 + ncols) of every panel as groups of W columns
  auto run_pass = [&](int col0, int ncols, int W) {
    const int ncg = (ncols + W - 1) / W;
    const int per = std::max(1, RICADI_MAX_GROUPS / ncg);
    const size_t nmw = (size_t)n * W;
    // chunks of equal size (16 shifts, 3 per chunk: 3 3 3 3 2 2 rather than 3 3 3 3 3 1); the caller's order is
    // kept: neighbouring shifts of a sorted list need similar iteration counts, which is what a lockstep batch wants
    const int nchunk = ((int)todo.size() + per - 1) / per;
    ++c->trace.wide_passes;
    c->trace.wide_chunks += nchunk;
    size_t at = 0;
    for (int ch = 0; ch < nchunk; ++ch) {
      const int cnt = ((int)todo.size() - (int)at + (nchunk - ch) - 1) / (nchunk - ch);
      const int Gv = cnt * ncg;
      std::vector<ShiftData*> vsds(Gv);
      c->trace.wide_groups_last = Gv;
      if (ncg * W != ncols) {
        HIPCHK(hipMemsetAsync(c->split_b.p, 0, sizeof(double) * nmw * Gv, st));
        if (have_x0) HIPCHK(hipMemsetAsync(c->split_x.p, 0, sizeof(double) * nmw * Gv, st));
      }
      for (int k = 0; k < cnt; ++k) {
        const int s = todo[at + k];
        for (int cg = 0; cg < ncg; ++cg) {
          const int v = k * ncg + cg, w = std::min(W, ncols - cg * W), sc = col0 + cg * W;
          vsds[v] = sds[s];
          launch_copy_cols(st, n, w, b + (size_t)s * gsb, m, sc, c->split_b.p + (size_t)v * nmw, W, 0, 1.0);
          if (have_x0)
            launch_copy_cols(st, n, w, x + (size_t)s * nm, m, sc, c->split_x.p + (size_t)v * nmw, W, 0, 1.0);
        }
      }
      std::vector<GmresResult> vres(Gv);
      gmres_core(c, vsds.data(), Gv, c->split_b.p, nmw, c->split_x.p, W, lowrank, vres.data(), have_x0, nullptr,
                 allow_stall);
      for (int k = 0; k < cnt; ++k) {
        const int s = todo[at + k];
        GmresResult& r = res[s];
        for (int cg = 0; cg < ncg; ++cg) {
          const int v = k * ncg + cg, w = std::min(W, ncols - cg * W);
          launch_copy_cols(st, n, w, c->split_x.p + (size_t)v * nmw, W, 0, x + (size_t)s * nm, m, col0 + cg * W, 1.0);
          r.iters = std::max(r.iters, vres[v].iters);
          r.converged = r.converged && vres[v].converged;
          r.stalled = r.stalled || vres[v].stalled;
          r.max_relres = std::max(r.max_relres, vres[v].max_relres);
        }
      }
      at += cnt;
    }
  };
  // (a remainder of up to 8 columns -- m = 66 = 4 x 16 + 2 -- as one more batch of 8-column groups over all
  // shifts instead of a fifth sixteen-column group per shift was measured at n = 1e5: 2172 vs 2176 ms per pass
  // over 64 shifts; the sweeps of an 8-column batch cost what those of a 16-column one do -- the block inverses
  // they read are as many bytes as the panels)
  run_pass(0, m, W0);
}

// ---- recycled right-hand sides (ricadi_set_recycle) ---------------------------------------------
// Initial guesses  x_g = sum_e Y_{g,e} C_e  from the stored pairs (B_e, Y_{g,e}),  S_g Y_{g,e} = B_e, with
// C = argmin || b - [B_e] C ||_F  (normal equations on the matrix cores, rank-revealing Cholesky on the
// host).  b: the right-hand side shared by the groups (n x m, pressure rows zero).  Returns false when no
// stored panel is common to all groups (x is not touched then).
static bool recycle_guess(ricadi_ctx* c, ShiftData* const* sds, int G, const double* b, int m, double* x) {
  ++c->trace.guess_tried;
  c->trace.guess_cols = c->trace.guess_rank = c->trace.guess_pan = 0;
  std::vector<const ricadi_ctx::RecB*> ent;
  // the ring keeps its size when the depth in force drops (an ADI at depth 5, then direct calls at depth 3): only the
  // newest rec_depth right-hand sides take part, as ricadi_set_recycle documents
  long oldest = 0;
  {
    std::vector<long> ser;
    for (auto& e : c->rec_ring)
      if (e && e->serial >= 0 && e->rows == c->nv) ser.push_back(e->serial);
    std::sort(ser.begin(), ser.end());
    if ((int)ser.size() > c->rec_depth && c->rec_depth > 0) oldest = ser[ser.size() - (size_t)c->rec_depth];
  }
  for (auto& e : c->rec_ring) {
    if (!e || e->serial < oldest || e->rows != c->nv) continue;
    bool all = true;
    for (int g = 0; g < G && all; ++g) {
      bool has = false;
      for (auto& y : sds[g]->rec)
        if (y && y->serial == e->serial && y->w == e->w) has = true;
      all = has;
    }
    if (all) ent.push_back(e.get());
  }
  if (ent.empty()) return false;
  int h = 0;
  for (auto* e : ent) h += e->w;
  hipStream_t st = c->st;
  const int nv = c->nv, n = c->n, hw = h + m;
  TArr<double> Gd(c->pool), Yd(c->pool, (size_t)h * m);
  std::vector<double> Ghh((size_t)h * h), Ghb((size_t)h * m), Y;
  int r0 = 0;
  // slot of every entry in the side-by-side panel (all of the panel's width, ring of at most 8 slots)
  std::vector<int> slot_of(ent.size(), -1);
  bool pan = c->rec_pan_w == m && c->rec_pan.p && c->rec_ring.size() <= 8;
  for (size_t i = 0; i < ent.size() && pan; ++i) {
    for (size_t si = 0; si < c->rec_ring.size(); ++si)
      if (c->rec_ring[si].get() == ent[i]) slot_of[i] = (int)si;
    pan = slot_of[i] >= 0 && ent[i]->w == m;
  }
  if (pan) {
    // Gram matrix of ALL slots and their products with b in two launches; the live entries are picked on the host
    const int H = 8 * m, Hw = H + m;
    Gd.alloc((size_t)H * Hw);
    HIPCHK(hipMemsetAsync(Gd.p, 0, sizeof(double) * H * Hw, st));
    launch_gemm_tn(st, nv, H, H, c->rec_pan.p, H, c->rec_pan.p, H, Gd.p, Hw);
    launch_gemm_tn(st, nv, H, m, c->rec_pan.p, H, b, m, Gd.p + H, Hw);
    std::vector<double> Gh((size_t)H * Hw);
    HIPCHK(hipMemcpyAsync(Gh.data(), Gd.p, sizeof(double) * Gh.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t ei = 0; ei < ent.size(); ++ei)
      for (int a = 0; a < m; ++a) {
        const int i = (int)ei * m + a, gi = slot_of[ei] * m + a;
        for (size_t ej = 0; ej < ent.size(); ++ej)
          for (int bcol = 0; bcol < m; ++bcol)
            Ghh[(size_t)i * h + ej * m + bcol] = Gh[(size_t)gi * Hw + slot_of[ej] * m + bcol];
        for (int j = 0; j < m; ++j) Ghb[(size_t)i * m + j] = Gh[(size_t)gi * Hw + H + j];
      }
  } else {
    Gd.alloc((size_t)h * hw);
    HIPCHK(hipMemsetAsync(Gd.p, 0, sizeof(double) * h * hw, st));
    for (size_t i = 0; i < ent.size(); ++i) {
      int c0 = r0;
      for (size_t j = i; j < ent.size(); ++j) {
        launch_gemm_tn(st, nv, ent[i]->w, ent[j]->w, ent[i]->b.p, ent[i]->w, ent[j]->b.p, ent[j]->w,
                       Gd.p + (size_t)r0 * hw + c0, hw);
        c0 += ent[j]->w;
      }
      launch_gemm_tn(st, nv, ent[i]->w, m, ent[i]->b.p, ent[i]->w, b, m, Gd.p + (size_t)r0 * hw + h, hw);
      r0 += ent[i]->w;
    }
    std::vector<double> Gh((size_t)h * hw);
    HIPCHK(hipMemcpyAsync(Gh.data(), Gd.p, sizeof(double) * Gh.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < h; ++i) {
      for (int j = 0; j < h; ++j) Ghh[(size_t)i * h + j] = j >= i ? Gh[(size_t)i * hw + j] : Gh[(size_t)j * hw + i];
      for (int j = 0; j < m; ++j) Ghb[(size_t)i * m + j] = Gh[(size_t)i * hw + h + j];
    }
  }
  // the diagonal blocks come from a symmetric kernel, the off-diagonal ones were computed above the
  // diagonal only: the mirror image is exact
  const int rank = gram_lstsq_scaled(h, m, Ghh, Ghb, 1e-11, Y);
  c->trace.guess_cols = h;
  c->trace.guess_rank = rank;
  c->trace.guess_pan = pan ? 1 : 0;
  if (rank == 0) return false;
  HIPCHK(hipMemcpyAsync(Yd.p, Y.data(), sizeof(double) * h * m, hipMemcpyHostToDevice, st));
  const GroupTab all = all_groups(G);
  r0 = 0;
  for (size_t i = 0; i < ent.size(); ++i) {
    GroupPtrs A = same_ptr((const double*)nullptr);
    for (int g = 0; g < G; ++g)
      for (auto& y : sds[g]->rec)
        if (y && y->serial == ent[i]->serial && y->w == ent[i]->w) A.p[g] = y->y.p;
    launch_gemm_nn_bp(st, all, n, ent[i]->w, m, A, ent[i]->w, Yd.p + (size_t)r0 * m, m, 0, x, m, (size_t)n * m,
                      1.0, i == 0 ? 0.0 : 1.0);
    r0 += ent[i]->w;
  }
  HIPCHK(hipStreamSynchronize(st));   // Y is a stack object
  if (c->opts.verbose > 1) fprintf(stderr, "[ricadi] recycled guess from %d stored columns (rank %d)\n", h, rank);
  ++c->trace.guess_used;
  return true;
}

static void recycle_store(ricadi_ctx* c, ShiftData* const* sds, int G, const double* b, int m, const double* x) {
  hipStream_t st = c->st;
  const int depth = c->rec_depth;
  ++c->trace.stored;
  ricadi_ctx::RecB* slot = nullptr;
  if ((int)c->rec_ring.size() < depth) {
    c->rec_ring.emplace_back(new ricadi_ctx::RecB);
    slot = c->rec_ring.back().get();
  } else {
    for (auto& e : c->rec_ring)
      if (!slot || e->serial < slot->serial) slot = e.get();
  }
  slot->serial = ++c->rec_serial;
  slot->w = m;
  slot->rows = c->nv;
  slot->b.ensure((size_t)c->nv * m);
  HIPCHK(hipMemcpyAsync(slot->b.p, b, sizeof(double) * c->nv * m, hipMemcpyDeviceToDevice, st));
  {
    // side-by-side copy (slots of another width invalidate the panel: recycle_guess then takes the pairwise path)
    int si = 0;
    for (; si < (int)c->rec_ring.size(); ++si)
      if (c->rec_ring[si].get() == slot) break;
    if (c->rec_pan_w != m || c->rec_pan.n < (size_t)c->nv * 8 * m) {
      c->rec_pan.ensure((size_t)c->nv * 8 * m);
      HIPCHK(hipMemsetAsync(c->rec_pan.p, 0, sizeof(double) * (size_t)c->nv * 8 * m, st));
      c->rec_pan_w = m;
      for (auto& e : c->rec_ring)
        if (e.get() != slot && e->serial >= 0 && e->w == m && e->rows == c->nv)
          launch_copy_cols(st, c->nv, m, e->b.p, m, 0, c->rec_pan.p, 8 * m, (int)(&e - &c->rec_ring[0]) * m, 1.0);
    }
    if (si < 8) launch_copy_cols(st, c->nv, m, b, m, 0, c->rec_pan.p, 8 * m, si * m, 1.0);
  }
  auto live = [&](long serial) {
    for (auto& e : c->rec_ring)
      if (e->serial == serial) return true;
    return false;
  };
  const size_t nm = (size_t)c->n * m;
  for (int g = 0; g < G; ++g) {
    ShiftData::RecY* y = nullptr;
    for (auto& r : sds[g]->rec)
      if (!live(r->serial)) y = r.get();          // a solution whose right-hand side has left the ring
    if (!y && (int)sds[g]->rec.size() < depth) {
      sds[g]->rec.emplace_back(new ShiftData::RecY);
      y = sds[g]->rec.back().get();
    }
    if (!y)
      for (auto& r : sds[g]->rec)
        if (!y || r->serial < y->serial) y = r.get();
    y->serial = slot->serial;
    y->w = m;
    y->y.ensure(nm);
    HIPCHK(hipMemcpyAsync(y->y.p, x + (size_t)g * nm, sizeof(double) * nm, hipMemcpyDeviceToDevice, st));
  }
}

// Storage of the Krylov basis / the preconditioner inverses for the solves inside the scope:
//   level 1: FP32-stored basis, FP64 inverses;  level 2: FP64-stored basis, FP64 inverses
// (level 0 = the context's defaults: FP16 / FP32 basis by size, FP32 inverses).  All levels of a
// multilevel preconditioner follow.  The arithmetic is FP64 at every level.
struct StorageScope {
  ricadi_ctx* c;
  bool b16, b32;
  std::vector<bool> p32;
  StorageScope(ricadi_ctx* ctx, int level) : c(ctx), b16(ctx->basis16), b32(ctx->basis32) {
    for (ricadi_ctx* l = c; l; l = l->child.get()) {
      p32.push_back(l->precond32);
      l->precond32 = false;
    }
    c->basis16 = false;
    if (level >= 2) {
      c->basis32 = false;
      c->basis.ensure((size_t)(c->wrestart + 1) * c->n * c->wcols);
    }
  }
  ~StorageScope() {
    size_t i = 0;
    for (ricadi_ctx* l = c; l; l = l->child.get()) l->precond32 = p32[i++];
    c->basis16 = b16;
    c->basis32 = b32;
  }
};
static int storage_level(const ricadi_ctx* c) {
  if (!c->precond32 && !c->basis32) return 2;
  if (!c->precond32 && !c->basis16) return 1;
  return 0;
}

// Relative true residuals ||b - (S - U V^T) x|| / ||b|| per column (G*m values, host);
// the residual panels are left in c->wv.
static void true_relres(ricadi_ctx* c, ShiftData* const* sds, int G, const double* b, size_t gsb,
                        const double* x, int m, bool lowrank, double* out) {
  hipStream_t st = c->st;
  Batch bt = make_batch(c, sds, G, m);
  const size_t nm = bt.gs;
  const int GM = G * m;
  double* hb = c->h_resid;
  op_apply(c, bt, x, nm, c->wv.p, lowrank);
  launch_axpby_b(st, bt.tab, nm, 1.0, b, gsb, -1.0, c->wv.p, nm);
  panel_norms2(c, bt, c->wv.p, nm, c->nrm2.p);
  panel_norms2(c, bt, b, gsb, c->bnorm2.p);
  HIPCHK(hipMemcpyAsync(hb, c->nrm2.p, sizeof(double) * GM, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hb + GM, c->bnorm2.p, sizeof(double) * GM, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int j = 0; j < GM; ++j)
    out[j] = hb[GM + j] > 0.0 ? std::sqrt(std::max(hb[j], 0.0) / hb[GM + j]) : 0.0;
}

// The batched solve as the drivers call it: recycled initial guess (shared right-hand side, plain
// operator), the lockstep GMRES, the storage safety net -- a group that stops at gmres_maxit or
// stagnates is continued from its iterate with the FP32- and then the FP64-stored basis and FP64
// preconditioner inverses (counted in c->escalations) -- true residuals on request.
static void gmres_solve_batch(ricadi_ctx* c, ShiftData* const* sds, int G, const double* b,
                              size_t gsb, double* x, int m, bool lowrank, double* relres_host,
                              GmresResult* res) {
  hipStream_t st = c->st;
  const bool plain = !(lowrank && c->q > 0);
  const bool shared = (gsb == 0 || G == 1) && plain && c->rec_depth > 0;
  Tick tkg;
  const bool guess = shared && recycle_guess(c, sds, G, b, m, x);
  if (c->sw.timing) {
    (void)hipStreamSynchronize(st);
    c->t_guess += tkg.lap();
  }
  const int lvl0 = storage_level(c);
  gmres_core_any(c, sds, G, b, gsb, x, m, lowrank, res, guess, nullptr, lvl0 < 2);
  std::vector<int> bad;
  for (int g = 0; g < G; ++g)
    if (!res[g].converged) bad.push_back(g);
  for (int level = lvl0 + 1; level <= 2 && !bad.empty(); ++level) {
    StorageScope wide(c, level);
    std::vector<GmresResult> r2(G);
    gmres_core_any(c, sds, G, b, gsb, x, m, lowrank, r2.data(), true, &bad, level < 2);
    c->escalations += (long)bad.size();
    (level == 1 ? c->trace.esc1_groups : c->trace.esc2_groups) += (int64_t)bad.size();
    std::vector<int> still;
    for (int g : bad) {
      if (c->opts.verbose)
        fprintf(stderr, "[ricadi] shift (%g, %g): %s after %d iterations at relres %.2e -> storage level %d: %d more, %.2e\n",
                sds[g]->alpha, sds[g]->beta, res[g].stalled ? "stagnation" : "gmres_maxit", res[g].iters,
                res[g].max_relres, level, r2[g].iters, r2[g].max_relres);
      res[g].iters += r2[g].iters;
      res[g].converged = r2[g].converged;
      res[g].stalled = r2[g].stalled;
      res[g].max_relres = r2[g].max_relres;
      if (!r2[g].converged) still.push_back(g);
    }
    bad.swap(still);
  }
  if (relres_host) true_relres(c, sds, G, b, gsb, x, m, lowrank, relres_host);
  if (shared) recycle_store(c, sds, G, b, m, x);
  for (int g = 0; g < G; ++g) c->total_iters += res[g].iters;
  c->total_solves += G;
}

// In-place inverse of a small dense matrix on the host (Gauss-Jordan, partial pivoting).
static bool host_invert(std::vector<double>& a, int q) {
  std::vector<double> inv((size_t)q * q, 0.0);
  for (int i = 0; i < q; ++i) inv[(size_t)i * q + i] = 1.0;
  double amax = 0.0;
  for (double v : a) amax = std::max(amax, std::fabs(v));
  for (int k = 0; k < q; ++k) {
    int p = k;
    for (int i = k + 1; i < q; ++i)
      if (std::fabs(a[(size_t)i * q + k]) > std::fabs(a[(size_t)p * q + k])) p = i;
    const double piv = a[(size_t)p * q + k];
    if (!(std::fabs(piv) > 1e-12 * amax)) return false;
    if (p != k)
      for (int j = 0; j < q; ++j) {
        std::swap(a[(size_t)k * q + j], a[(size_t)p * q + j]);
        std::swap(inv[(size_t)k * q + j], inv[(size_t)p * q + j]);
      }
    for (int j = 0; j < q; ++j) {
      a[(size_t)k * q + j] /= piv;
      inv[(size_t)k * q + j] /= piv;
    }
    for (int i = 0; i < q; ++i) {
      if (i == k) continue;
      const double f = a[(size_t)i * q + k];
      if (f == 0.0) continue;
      for (int j = 0; j < q; ++j) {
        a[(size_t)i * q + j] -= f * a[(size_t)k * q + j];
        inv[(size_t)i * q + j] -= f * inv[(size_t)k * q + j];
      }
    }
  }
  a.swap(inv);
  return true;
}

// Batched solve with the low-rank term  (S_g - U V^T) x_g = b_g.
//
// Default: Sherman-Morrison-Woodbury, as the reference's lau.solve_sadpnt_smw does --
// GMRES runs on the plain saddle operator (no thin GEMMs inside the iteration), and
//   x = y + W (V^T y),   y = S^-1 b,   W = S^-1 [U;0] (I - V^T S^-1 U)^-1 .
// W_g is cached per shift and low-rank term; a batch that meets a shift without it
// solves the augmented panels [b_g, U] (m + q columns) once.  The closed-loop residual
// is then verified in FP64; columns above the tolerance (ill-conditioned capacitance
// matrix) are refined by one GMRES on the closed-loop operator itself.
static void solve_batch(ricadi_ctx* c, ShiftData* const* sds, int G, const double* b, size_t gsb,
                        double* x, int m, bool lowrank, double* relres_host, GmresResult* res) {
  const int q = c->q;
  ++c->trace.solves;
  if (!lowrank || q <= 0 || !c->sw.smw || m + q > RICADI_MAX_M) {
    if (lowrank && q > 0) ++c->trace.inop_lowrank;
    gmres_solve_batch(c, sds, G, b, gsb, x, m, lowrank && q > 0, relres_host, res);
    return;
  }
  hipStream_t st = c->st;
  const int n = c->n, nv = c->nv, np = c->np;
  const size_t nm = (size_t)n * m;
  const double tol = c->opts.gmres_tol;
  bool need = false;
  for (int g = 0; g < G; ++g) need = need || sds[g]->smw_epoch != c->lr_epoch;
  const GroupTab all = all_groups(G);
  bool bad = false;
  // U = columns [ucol, ucol + q) of the (shared) right-hand side: S^-1 U is part of the plain solution,
  // no augmented columns needed (first sweep of a Newton step without mtxoldb: rhs = [W, K_k], U = K_k)
  const int ucol = c->lr_ucol;
  c->lr_ucol = -1;             // the hint holds for one solve
  const bool dup = need && (gsb == 0 || G == 1) && ucol >= 0 && ucol + q <= m;
  ++c->trace.smw_solves;
  if (need) {
    ++c->trace.smw_setups;
    if (dup) ++c->trace.smw_dup;
    const int ma = dup ? m : m + q;
    const size_t nma = (size_t)n * ma;
    double* xa;
    int xoff;     // column of S^-1 U inside the solution panels xa (leading dimension ma)
    if (dup) {
      gmres_solve_batch(c, sds, G, b, gsb, x, m, false, nullptr, res);
      xa = x;
      xoff = ucol;
    } else {
      // augmented panels [b_g, U]; one panel for all groups when they share b
      const int nra = gsb == 0 ? 1 : G;
      c->smw_rhs.ensure(nma * nra);
      c->smw_x.ensure(nma * G);
      double* ra = c->smw_rhs.p;
      xa = c->smw_x.p;
      xoff = m;
      for (int g = 0; g < nra; ++g) {
        launch_copy_cols(st, n, m, b + (size_t)g * gsb, m, 0, ra + g * nma, ma, 0, 1.0);
        launch_copy_cols(st, nv, q, c->U.p, q, 0, ra + g * nma, ma, m, 1.0);
        if (np > 0)
          HIPCHK(hipMemset2DAsync(ra + g * nma + (size_t)nv * ma + m, sizeof(double) * ma, 0,
                                  sizeof(double) * q, np, st));
      }
      gmres_solve_batch(c, sds, G, ra, gsb == 0 ? 0 : nma, xa, ma, false, nullptr, res);
    }
    // capacitance matrices I - V^T (S^-1 U)
    c->smw_cap.ensure((size_t)G * q * q);
    HIPCHK(hipMemsetAsync(c->smw_cap.p, 0, sizeof(double) * G * q * q, st));
    launch_gemm_tn_b(st, all, nv, q, q, c->V.p, q, xa + xoff, ma, nma, c->smw_cap.p, q, (size_t)q * q);
    std::vector<double> caps((size_t)G * q * q);
    HIPCHK(hipMemcpyAsync(caps.data(), c->smw_cap.p, sizeof(double) * caps.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int g = 0; g < G && !bad; ++g) {
      std::vector<double> cap((size_t)q * q);
      for (int i = 0; i < q; ++i)
        for (int j = 0; j < q; ++j)
          cap[(size_t)i * q + j] = (i == j ? 1.0 : 0.0) - caps[(size_t)g * q * q + (size_t)i * q + j];
      if (!host_invert(cap, q) || !res[g].converged) bad = true;
      std::copy(cap.begin(), cap.end(), caps.begin() + (size_t)g * q * q);
    }
    if (bad) ++c->trace.smw_bad;
    if (!dup)
      for (int g = 0; g < G; ++g)
        launch_copy_cols(st, n, m, xa + g * nma, ma, 0, x + g * nm, m, 0, 1.0);
    if (!bad) {
      HIPCHK(hipMemcpyAsync(c->smw_cap.p, caps.data(), sizeof(double) * caps.size(), hipMemcpyHostToDevice, st));
      for (int g = 0; g < G; ++g) {
        ShiftData* sd = sds[g];
        if (sd->smw_w.n != (size_t)n * q) sd->smw_w.alloc((size_t)n * q);
        launch_gemm_nn(st, n, q, q, xa + g * nma + xoff, ma, c->smw_cap.p + (size_t)g * q * q, q,
                       sd->smw_w.p, q, 1.0, 0.0);
        sd->smw_epoch = c->lr_epoch;
      }
      HIPCHK(hipStreamSynchronize(st));   // caps is a stack object
    }
  } else {
    gmres_solve_batch(c, sds, G, b, gsb, x, m, false, nullptr, res);
  }
  const size_t gsq = (size_t)q * m;
  if (!bad) {
    // x_g += W_g (V^T x_g)
    GroupPtrs W = same_ptr((const double*)nullptr);
    for (int g = 0; g < G; ++g) W.p[g] = sds[g]->smw_w.p;
    HIPCHK(hipMemsetAsync(c->lrc.p, 0, sizeof(double) * gsq * G, st));
    launch_gemm_tn_b(st, all, nv, q, m, c->V.p, q, x, m, nm, c->lrc.p, m, gsq);
    launch_gemm_nn_bp(st, all, n, q, m, W, q, c->lrc.p, m, gsq, x, m, nm, 1.0, 1.0);
  }
  // verification on the closed-loop operator, refinement where needed
  std::vector<double> rr((size_t)G * m);
  true_relres(c, sds, G, b, gsb, x, m, true, rr.data());
  bool ok = true;
  for (double v : rr) ok = ok && v <= tol;
  if (!ok) {
    ++c->trace.smw_refined;
    c->smw_rhs.ensure(nm * G);
    c->smw_x.ensure(nm * G);
    HIPCHK(hipMemcpyAsync(c->smw_rhs.p, c->wv.p, sizeof(double) * nm * G, hipMemcpyDeviceToDevice, st));
    std::vector<GmresResult> r2(G);
    // residual equation on the closed-loop operator; its tolerance is relative to ||r||
    double worst = 0.0;
    for (double v : rr) worst = std::max(worst, v);
    {
      Restore<double> keep_tol(c->opts.gmres_tol);
      c->opts.gmres_tol = std::min(0.5, std::max(1e-14, 0.5 * tol / worst));
      gmres_solve_batch(c, sds, G, c->smw_rhs.p, nm, c->smw_x.p, m, true, nullptr, r2.data());
    }
    launch_axpby_b(st, all, nm, 1.0, c->smw_x.p, nm, 1.0, x, nm);
    for (int g = 0; g < G; ++g) res[g].iters += r2[g].iters;
    true_relres(c, sds, G, b, gsb, x, m, true, rr.data());
  }
  for (int g = 0; g < G; ++g) {
    double w = 0.0;
    for (int j = 0; j < m; ++j) w = std::max(w, rr[(size_t)g * m + j]);
    res[g].max_relres = w;
    res[g].converged = w <= tol * 1.0000001;
  }
  if (relres_host) std::copy(rr.begin(), rr.end(), relres_host);
}

static GmresResult gmres_solve(ricadi_ctx* c, ShiftData* sd, const double* b, double* x, int m,
                               bool lowrank, double* relres_host) {
  GmresResult r;
  solve_batch(c, &sd, 1, b, (size_t)c->n * m, x, m, lowrank, relres_host, &r);
  return r;
}

// rhs panel (n x m) from an NV x m device block (pressure rows zero)
static void load_rhs(ricadi_ctx* c, const double* dR, int m, double* b) {
  HIPCHK(hipMemcpyAsync(b, dR, sizeof(double) * (size_t)c->nv * m, hipMemcpyDeviceToDevice, c->st));
  if (c->np > 0)
    HIPCHK(hipMemsetAsync(b + (size_t)c->nv * m, 0, sizeof(double) * (size_t)c->np * m, c->st));
}
