// solver_setup.inl -- per-shift setup: workspaces, coarse inverses (block Gauss-Jordan / pivoted rocSOLVER), block inverses, Schur blocks.
// Part of ricadi_solver.hip (one translation unit; included there in order).


// Width of the column groups a wide panel is solved in (0: the panel stays whole); see gmres_core_any.
static int wide_split_width(const ricadi_ctx* c, int m) {
  return (c->sw.wide_split && m > 32) ? 16 : 0;
}

// Workspace for batches of up to `groups` panels of width m (group-major: every
// buffer holds one slab per group; basis is vector-major, i.e. Krylov vector j of
// all groups is contiguous).
// `extra` columns per group are reserved on top of m (default: the low-rank width, for
// the augmented Sherman-Morrison-Woodbury solves) so that a nested, wider solve never
// reallocates buffers the caller has already filled.
static void ensure_work(ricadi_ctx* c, int m, int groups = 1, int extra = -1) {
  const int restart = c->opts.gmres_restart;
  if (extra < 0) extra = std::max(c->q, 0);
  if (c->child) {
    c->child->opts.gmres_restart = std::min(c->opts.gmres_restart, 4);   // its Krylov buffers are not used
    ensure_work(c->child.get(), m, groups, extra);
  }
  // every buffer scales with the total number of columns (m + extra) * groups
  int want = (m + extra) * groups;
  // a wide panel is solved as chunks of up to RICADI_MAX_GROUPS sixteen-column groups: the buffers must hold a
  // full chunk already NOW -- the caller's right-hand side lives in them (c->bvec) when the solve starts
  if (wide_split_width(c, m + extra)) want = std::max(want, 16 * RICADI_MAX_GROUPS);
  if (want <= c->wcols && restart == c->wrestart) return;
  const size_t gm = (size_t)std::max(want, c->wcols);
  const size_t nm = (size_t)c->n * gm;
  // Krylov basis: stored in FP16 by default (FP32 with RICADI_BASIS32, FP64 with
  // RICADI_BASIS64); ALL arithmetic stays FP64 -- the three passes over the basis per
  // iteration are the largest share of the HBM traffic.  The current vector is also
  // kept in FP64 (vcur, holding the same rounded values) for the operator /
  // preconditioner application, so the Arnoldi relation holds exactly for the stored
  // vectors; what the storage precision limits is the residual reduction one restart
  // cycle can deliver (~1e-3 for FP16, cycles gain ~1e-2), and every cycle starts from
  // the true FP64 residual.  Unit vectors of dimension n have entries ~ n^-1/2: FP16
  // (normal range from 6e-5) is used up to n = 2^21, FP32 beyond.
  c->basis32 = !c->sw.basis64;
  c->basis16 = basis16_default(c);
  if (c->basis32) {
    c->basisf.alloc((size_t)(restart + 1) * nm);
    c->vcur.alloc(nm);
    c->basis.release();
  } else {
    c->basis.alloc((size_t)(restart + 1) * nm);
    c->basisf.release();
  }
  c->zbasisf.alloc((size_t)restart * nm);      // flexible GMRES: Z_j = P^-1 v_j kept (FP32), x += Z y at the cycle end
  c->wv.alloc(nm);
  c->wv32.alloc(nm);
  c->zv.alloc(nm);
  c->r2.alloc(nm);
  c->xs.alloc(nm);
  c->bvec.alloc(nm);
  c->pw1.alloc(nm);
  c->pw2.alloc(nm);
  c->tp.alloc((size_t)std::max(c->np, 1) * gm);
  c->rc.alloc((size_t)std::max(c->kc, 1) * gm);
  c->ec.alloc((size_t)std::max(c->kc, 1) * gm);
  c->partial.alloc((size_t)dots_num_blocks(c->n) * (restart + 2) * gm);
  c->h1.alloc((size_t)(restart + 2) * gm);
  c->ls_partial.alloc((gm + 15) / 16 * lowsync_partial_stride(c->n, restart));
  c->ls_coef.alloc((gm + 15) / 16 * lowsync_coef_stride(restart));
  c->h2.alloc((size_t)2 * (restart + 2) * gm);      // two buffers (atomic dot passes alternate between them)
  c->H.alloc(gm * (restart + 1) * restart);
  c->cs.alloc(gm * restart);
  c->sn.alloc(gm * restart);
  c->g.alloc(gm * (restart + 1));
  c->scale.alloc(gm);
  c->resid.alloc(2 * gm);          // two buffers (the fused update + Hessenberg launch alternates between them)
  c->yv.alloc((size_t)restart * gm);
  c->bnorm2.alloc(gm);
  c->nrm2.alloc(gm);
  c->lrc.alloc((size_t)64 * gm + 64);
  if (!c->h_resid) {
    HIPCHK(hipHostMalloc((void**)&c->h_resid,
                         sizeof(double) * 4 * RICADI_MAX_M * RICADI_MAX_GROUPS));
    for (int i = 0; i < 2; ++i) HIPCHK(hipEventCreateWithFlags(&c->ev_res[i], hipEventDisableTiming));
  }
  c->wcols = (int)gm;
  c->wrestart = restart;
}

// ---- per-shift setup ---------------------------------------------------------
static Exec main_exec(ricadi_ctx* c);
static void get_shifts(ricadi_ctx* c, const double* alphas, const double* betas, int ng, ShiftData** out);

template <class T>
static void stable_alloc(DArr<T>& a, size_t n) {
  if (a.n != n) a.alloc(n);
}

// In-place inverses of nb (<= gj_max_batch()) dense k x k matrices (row-major, device pointers in hmats) by
// block Gauss-Jordan elimination without pivoting: per 128-row block three small kernels and two batched
// rocBLAS GEMMs (ricadi_precond.hip).  A diagonal block with a vanishing pivot raises *gjflag (the matrices are
// garbage then; the caller assembles them again and takes the pivoted rocSOLVER route).  No host
// synchronisation: the pointer arrays go up from hptrs (pinned, read by the copy when the stream reaches it) to
// dptrs; the caller has sized the gj_* panels for the batch.
static void gj_invert_batched(ricadi_ctx* c, const Exec& ex, int* gjflag, double* const* hmats, int nb, int k,
                              double** hptrs, double** dptrs) {
  hipStream_t st = ex.st;
  const int NB = gj_block();
  const size_t pan = (size_t)k * NB;
  for (int i = 0; i < nb; ++i) {
    hptrs[i] = hmats[i];
    hptrs[nb + i] = c->gj_cb.p + pan * i;
    hptrs[2 * nb + i] = c->gj_rp.p + pan * i;
    hptrs[3 * nb + i] = c->gj_rb.p + pan * i;
    hptrs[4 * nb + i] = c->gj_d.p + (size_t)NB * NB * i;
  }
  HIPCHK(hipMemcpyAsync(dptrs, hptrs, sizeof(double*) * 5 * nb, hipMemcpyHostToDevice, st));
  double* const* dA = dptrs;
  double* const* dCb = dA + nb;
  double* const* dRp = dA + 2 * nb;
  double* const* dRb = dA + 3 * nb;
  double* const* dD = dA + 4 * nb;
  const double one = 1.0, zero = 0.0, mone = -1.0;
  for (int k0 = 0; k0 < k; k0 += NB) {
    const int nbe = std::min(NB, k - k0);
    launch_gj_prep(st, nb, hmats, k, k0, nbe, c->gj_cb.p, c->gj_rp.p, c->gj_d.p);
    launch_gj_diag(st, nb, c->gj_d.p, nbe, gjflag);
    // row-major Rb = D^-1 Rp  ==  column-major Rb^T = Rp^T (D^-1)^T
    RBCHK(rocblas_dgemm_batched(ex.rb, rocblas_operation_none, rocblas_operation_none, k, nbe, nbe, &one,
                                (const double* const*)dRp, k, (const double* const*)dD, NB, &zero, dRb, k, nb));
    // row-major A -= Cb Rb  ==  column-major A^T -= Rb^T Cb^T
    RBCHK(rocblas_dgemm_batched(ex.rb, rocblas_operation_none, rocblas_operation_none, k, k, nbe, &mone,
                                (const double* const*)dRb, k, (const double* const*)dCb, NB, &one, dA, k, nb));
    launch_gj_rows(st, nb, hmats, k, k0, nbe, c->gj_rb.p);
  }
}

// The gj_* panels and pointer arrays for a batch of nb matrices of size k.  Growing them may synchronise the device:
// setup_issue calls this before its first launch.  The pinned pointer buffer holds a full batch from the start.
static void gj_reserve(ricadi_ctx* c, int nb, int k) {
  const int NB = gj_block(), chunk = std::min(gj_max_batch(), nb);
  const size_t pan = (size_t)k * NB;
  c->gj_cb.ensure(pan * chunk);
  c->gj_rp.ensure(pan * chunk);
  c->gj_rb.ensure(pan * chunk);
  c->gj_d.ensure((size_t)NB * NB * chunk);
  c->gj_ptrs.ensure((size_t)5 * nb);
  if (c->gj_hcap < (size_t)5 * nb) {
    if (c->gj_hptrs) {
      HIPCHK(hipDeviceSynchronize());      // an earlier upload may still read the old buffer
      HIPCHK(hipHostFree(c->gj_hptrs));
      c->gj_hptrs = nullptr;
    }
    const size_t cap = (size_t)5 * std::max(nb, gj_max_batch());
    HIPCHK(hipHostMalloc((void**)&c->gj_hptrs, sizeof(double*) * cap));
    c->gj_hcap = cap;
  }
}

// Issue half of the route-0 inverses of all matrices in hp (chunks of gj_max_batch() in stream order on ex); the
// verdict is in ex.flag[2] once ex.st has got there (invert_dense_finish).  The gj_* panels and pointer arrays are
// shared by every Exec: a setup issued on one must be finished before another is issued.
static void invert_dense_issue(ricadi_ctx* c, const Exec& ex, const std::vector<double*>& hp, int k) {
  const int nb = (int)hp.size();
  gj_reserve(c, nb, k);
  HIPCHK(hipMemsetAsync(ex.flag + 2, 0, sizeof(int), ex.st));
  for (int i0 = 0; i0 < nb; i0 += gj_max_batch())
    gj_invert_batched(c, ex, ex.flag + 2, hp.data() + i0, std::min(gj_max_batch(), nb - i0), k,
                      c->gj_hptrs + 5 * i0, c->gj_ptrs.p + 5 * i0);
}

// Finish half: ex.st must have been synchronised.  A vanishing pivot in any matrix sends ALL of them through
// route 1 on the main stream (`reassemble` restores what route 0 has overwritten).  Returns the route.
template <class F>
static int invert_dense_finish(ricadi_ctx* c, const Exec& ex, const std::vector<double*>& hp, int k,
                               std::vector<int>& info, F&& reassemble) {
  hipStream_t st = c->st;
  const int nb = (int)hp.size();
  int flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, ex.flag + 2, sizeof(int), hipMemcpyDeviceToHost, ex.st));
  HIPCHK(hipStreamSynchronize(ex.st));
  if (flag == 0) {
    std::fill(info.begin(), info.end(), 0);
    return 0;
  }
  reassemble();
  // row-major E == column-major E^T; inv(E^T) column-major == inv(E) row-major
  c->ipiv.ensure((size_t)k * nb);
  c->info.ensure(nb);
  c->eptrs.ensure(nb);
  HIPCHK(hipMemcpyAsync(c->eptrs.p, hp.data(), sizeof(double*) * nb, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));   // hp may be a stack object of the caller
  RBCHK(rocsolver_dgetrf_batched(c->rb, k, k, c->eptrs.p, k, c->ipiv.p, k, c->info.p, nb));
  RBCHK(rocsolver_dgetri_batched(c->rb, k, c->eptrs.p, k, c->ipiv.p, k, c->info.p, nb));
  HIPCHK(hipMemcpyAsync(info.data(), c->info.p, sizeof(int) * nb, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return 1;
}

// In-place inverses of nb dense k x k matrices (row major, device pointers in hp): the coarse matrices of a setup.
// Route 0: block Gauss-Jordan WITHOUT pivoting on batched GEMMs (gj_invert_batched) -- with the velocity
// aggregates ordered before the pressure aggregates that is block elimination of the coarse saddle matrix: the
// velocity block has a definite symmetric part for ADI shifts (and is s.p.d. for the projection), the Schur
// complement -B Av^-1 B^T inherits it.  A pivot that vanishes relative to its block's scale sends ALL matrices of
// the call through route 1: rocSOLVER's getrf / getri with partial pivoting (its unpivoted routines, the step in
// between until round 3, only notice an EXACTLY zero pivot -- a pivot of 1e-14 of the block's scale passed and left
// a garbage inverse).  `reassemble` restores the matrices the first route has overwritten.  info (nb entries):
// rocSOLVER's status.  Returns the route.
template <class F>
static int invert_dense_batch(ricadi_ctx* c, const std::vector<double*>& hp, int k, std::vector<int>& info,
                              F&& reassemble) {
  const Exec ex = main_exec(c);
  invert_dense_issue(c, ex, hp, k);
  HIPCHK(hipStreamSynchronize(ex.st));
  return invert_dense_finish(c, ex, hp, k, info, reassemble);
}

// A per-shift setup between its two halves: setup_issue puts every launch on `ex` without synchronising the
// host, setup_finish waits for them, checks the flags, takes the pivoted coarse route if needed and marks the data
// valid.  An exception in between (the caller's own work) leaves the job to its destructor, which drains ex.st
// before the half-built data can be built again elsewhere.
struct SetupJob {
  Exec ex;
  std::vector<ShiftData*> todo;
  std::vector<double*> hp;      // the coarse matrices of todo (route 0 in flight on ex)
  Tick tks;
  double tph[6] = {0, 0, 0, 0, 0, 0};
  bool open = false;
  SetupJob() = default;
  SetupJob(const SetupJob&) = delete;
  SetupJob& operator=(const SetupJob&) = delete;
  ~SetupJob() {
    if (open) (void)hipStreamSynchronize(ex.st);
  }
};

// Issue half of the per-shift data for the given (alpha, beta) pairs; whatever is missing is built for all of
// them together: the element-wise / block kernels per shift, the dense coarse inverses in ONE batched block
// Gauss-Jordan elimination (its launches then serve all shifts of a sweep at once).  With ex on the auxiliary
// stream the work waits for what the main stream has issued so far.
static void setup_issue(ricadi_ctx* c, const Exec& ex, const double* alphas, const double* betas, int ng,
                        ShiftData** out, SetupJob& job) {
  hipStream_t st = ex.st;
  job.ex = ex;
  std::vector<ShiftData*>& todo = job.todo;
  todo.clear();
  for (int g = 0; g < ng; ++g) {
    auto key = std::make_pair(alphas[g], betas[g]);
    auto it = c->cache.find(key);
    if (it == c->cache.end()) it = c->cache.emplace(key, std::unique_ptr<ShiftData>(new ShiftData)).first;
    ShiftData* sd = it->second.get();
    out[g] = sd;
    if (sd->valid || std::find(todo.begin(), todo.end(), sd) != todo.end()) continue;
    sd->alpha = alphas[g];
    sd->beta = betas[g];
    sd->smw_epoch = -1;
    for (auto& r : sd->rec) r->serial = -1;     // stale, but the buffers stay (a hipFree / hipMalloc pair per panel
                                                // cost 13 ms per setup of 17 shifts)
    todo.push_back(sd);
  }
  if (todo.empty()) return;
  job.open = true;
  job.tks = Tick();
  double* tph = job.tph;
  Tick& tks = job.tks;
  auto lapS = [&](int i) {
    if (c->sw.timing) {
      (void)hipStreamSynchronize(st);
      tph[i] += tks.lap();
    }
  };
  const size_t bsz = (size_t)c->bs * c->bs;
  const int k = c->kc;
  const int kd = c->child ? 0 : c->kc;   // size of the dense coarse inverse (none with a child level)
  const bool copies16 = c->sw.blocks16 && c->sw_stride > 0 && c->gt_ok && c->ady_ok && k > 0 && c->nbp > 0;
  // Every buffer first, then the launches: an allocation may wait for the device (hipFree inside a growing
  // DArr does), and the projection solve would then wait for the work already issued here.
  for (ShiftData* sd : todo) {
    stable_alloc(sd->sval, c->snnz);
    if (c->sb_ok) stable_alloc(sd->svalb, c->snnz);
    stable_alloc(sd->bvinv, (size_t)c->nbv * bsz);
    if (c->nbp > 0) stable_alloc(sd->bpinv, (size_t)c->nbp * bsz);
    if (c->gt_ok) stable_alloc(sd->gtm, (size_t)c->nbv * c->bs * c->gt_ks);
    if (c->ady_ok && k > 0) stable_alloc(sd->adym, (size_t)c->nbv * c->bs * c->ady_ks);
    if (kd > 0) stable_alloc(sd->einv, (size_t)k * k);
    if (k > 0) {
      stable_alloc(sd->syval, c->synnz);
      if (c->syb_ok) stable_alloc(sd->syvalb, c->synnz);
    }
    if (c->vanka) {
      const size_t vn = (size_t)c->vk.npatches * VANKA_K * VANKA_K;
      stable_alloc(sd->vkinv, vn);      // (the FP64 originals stay, like einv: a solve repeated with FP64 operands reads them)
      if (c->precond32) stable_alloc(sd->vkinvf, vn);
    }
    if (c->precond32) {
      stable_alloc(sd->bvinvf, sd->bvinv.n);
      if (c->nbp > 0) stable_alloc(sd->bpinvf, sd->bpinv.n);
      if (c->gt_ok) stable_alloc(sd->gtmf, sd->gtm.n);
      if (c->ady_ok && k > 0) stable_alloc(sd->adymf, sd->adym.n);
      if (copies16) {
        stable_alloc(sd->bvinvh, sd->bvinv.n);
        stable_alloc(sd->bpinvh, sd->bpinv.n);
        stable_alloc(sd->gtmh, sd->gtm.n);
        stable_alloc(sd->adymh, sd->adym.n);
      }
    }
  }
  if (kd > 0) gj_reserve(c, (int)todo.size(), k);
  if (st != c->st) {
    HIPCHK(hipEventRecord(c->ev_z, c->st));
    HIPCHK(hipStreamWaitEvent(st, c->ev_z, 0));
  }
  HIPCHK(hipMemsetAsync(ex.flag, 0, sizeof(int), st));
  if (c->child) {
    std::vector<double> al(todo.size()), be(todo.size());
    std::vector<ShiftData*> subs(todo.size(), nullptr);
    for (size_t i = 0; i < todo.size(); ++i) {
      al[i] = todo[i]->alpha;
      be[i] = todo[i]->beta;
    }
    get_shifts(c->child.get(), al.data(), be.data(), (int)todo.size(), subs.data());
    for (size_t i = 0; i < todo.size(); ++i) todo[i]->sub = subs[i];
  }
  lapS(0);
  for (ShiftData* sd : todo) {
    const double alpha = sd->alpha, beta = sd->beta;
    launch_assemble_shift(st, (int)c->snnz, c->srcA.p, c->srcE.p, c->srcJ.p, alpha, beta,
                          sd->sval.p);
    if (c->sb_ok) launch_gather_vals(st, (int)c->snnz, c->sb_perm.p, sd->sval.p, sd->svalb.p);
    launch_block_combine(st, (size_t)c->nbv * bsz, c->bvA.p, c->bvE.p, alpha, beta, sd->bvinv.p);
    if (kd > 0) launch_combine3(st, (size_t)k * k, c->E0.p, c->EM.p, c->EJ.p, alpha, beta, sd->einv.p);
    if (k > 0) {
      launch_assemble_shift(st, (int)c->synnz, c->sy_A.p, c->sy_E.p, c->sy_J.p, alpha, beta,
                            sd->syval.p);
      if (c->syb_ok) launch_gather_vals(st, (int)c->synnz, c->syb_perm.p, sd->syval.p, sd->syvalb.p);
    }
  }
  lapS(1);
  // block inversions and Schur blocks: one launch each for all shifts (<= 16 per call)
  for (size_t t0 = 0; t0 < todo.size(); t0 += RICADI_MAX_GROUPS) {
    const int cnt = (int)std::min<size_t>(RICADI_MAX_GROUPS, todo.size() - t0);
    GroupPtrs pv = same_ptr((const double*)nullptr), pp = pv;
    for (int i = 0; i < cnt; ++i) {
      pv.p[i] = todo[t0 + i]->bvinv.p;
      pp.p[i] = todo[t0 + i]->bpinv.p;
    }
    launch_block_invert(st, cnt, c->nbv, c->bs, c->bv_ptr.p, pv, ex.flag);
    if (c->gt_ok) {
      GroupPtrs pg = same_ptr((const double*)nullptr);
      for (int i = 0; i < cnt; ++i) pg.p[i] = todo[t0 + i]->gtm.p;
      launch_gt_blocks(st, cnt, c->nbv, c->bs, c->gt_ks, c->gt_jtd.p, pv, pg);
    }
    if (c->ady_ok && k > 0) {
      GroupPtrs pa_ = same_ptr((const double*)nullptr);
      double al[RICADI_MAX_GROUPS], be[RICADI_MAX_GROUPS];
      for (int i = 0; i < cnt; ++i) {
        pa_.p[i] = todo[t0 + i]->adym.p;
        al[i] = todo[t0 + i]->alpha;
        be[i] = todo[t0 + i]->beta;
      }
      launch_ady_blocks(st, cnt, c->nbv, c->bs, c->ady_ks, c->cy_dA.p, c->cy_dE.p, c->cy_dJ.p,
                        c->sa ? c->cy_dT.p : nullptr, al, be, pv, pa_);
    }
    if (c->nbp > 0) {
      launch_schur_blocks_bj(st, cnt, c->nbp, c->bs, c->bp_ptr.p, c->jd_ptr.p, c->jd_vblk.p,
                             c->jd_val.p, pv, pp);
      launch_block_invert(st, cnt, c->nbp, c->bs, c->bp_ptr.p, pp, ex.flag);
    }
  }
  lapS(2);
  if (kd > 0) {
    job.hp.resize(todo.size());
    for (size_t i = 0; i < todo.size(); ++i) job.hp[i] = todo[i]->einv.p;
    invert_dense_issue(c, ex, job.hp, k);
  }
  lapS(3);
  if (c->precond32) {
    // the FP32 / BF16 copies of everything but the coarse inverses (those may still take route 1)
    const int bs2 = c->bs * c->bs;
    for (ShiftData* sd : todo) {
      launch_to_f32(st, c->nbv, bs2, sd->bvinv.p, bs2, sd->bvinvf.p, bs2);
      if (c->nbp > 0) {
        launch_to_f32(st, c->nbp, bs2, sd->bpinv.p, bs2, sd->bpinvf.p, bs2);
      }
      if (c->gt_ok) {
        const int gsz = c->bs * c->gt_ks;
        launch_to_f32(st, c->nbv, gsz, sd->gtm.p, gsz, sd->gtmf.p, gsz);
      }
      if (c->ady_ok && k > 0) {
        const int gsz = c->bs * c->ady_ks;
        launch_to_f32(st, c->nbv, gsz, sd->adym.p, gsz, sd->adymf.p, gsz);
      }
      if (copies16) {
        // BF16 copies for the record-driven sweeps (all four or none: the cycle switches as a whole)
        launch_to_bf16(st, sd->bvinv.n, sd->bvinv.p, sd->bvinvh.p);
        launch_to_bf16(st, sd->bpinv.n, sd->bpinv.p, sd->bpinvh.p);
        launch_to_bf16(st, sd->gtm.n, sd->gtm.p, sd->gtmh.p);
        launch_to_bf16(st, sd->adym.n, sd->adym.p, sd->adymh.p);
      }
    }
  }
  lapS(4);
}

// The patch inverses of the coloured Vanka sweep for the shifts of a setup (a child level; called from setup_finish,
// when the level's assembled values sd->sval are complete and the route-0 panels of the coarse inverses are free
// again): gather S[idx, idx] of every (shift, patch), invert the whole batch with the coarse matrices' routine
// (block Gauss-Jordan, pivoted rocSOLVER route for all of them where a pivot vanishes), store as the level stores
// its operands (in place in FP64; the FP32 copies beside them where the level's operands are FP32-stored).
static void vanka_setup(ricadi_ctx* c, const Exec& ex, const std::vector<ShiftData*>& todo) {
  hipStream_t st = ex.st;
  const size_t np_ = (size_t)c->vk.npatches, kk = (size_t)VANKA_K * VANKA_K;
  if (np_ == 0 || todo.empty()) return;
  std::vector<double*> base(todo.size());
  for (size_t i = 0; i < todo.size(); ++i) base[i] = todo[i]->vkinv.p;
  auto gather = [&] {
    for (size_t t0 = 0; t0 < todo.size(); t0 += RICADI_MAX_GROUPS) {
      const int cnt = (int)std::min<size_t>(RICADI_MAX_GROUPS, todo.size() - t0);
      GroupPtrs sv = same_ptr((const double*)nullptr);
      for (int i = 0; i < cnt; ++i) sv.p[i] = todo[t0 + i]->sval.p;
      launch_vanka_gather(st, cnt, (int)np_, c->vk.npress, c->vk_idx.p, c->s_rp.p, c->s_ci.p, sv, base.data() + t0);
    }
  };
  gather();
  std::vector<double*> hp(todo.size() * np_);
  for (size_t i = 0; i < todo.size(); ++i)
    for (size_t b = 0; b < np_; ++b) hp[i * np_ + b] = base[i] + kk * b;
  std::vector<int> info(hp.size(), 0);
  invert_dense_issue(c, ex, hp, VANKA_K);
  HIPCHK(hipStreamSynchronize(st));
  invert_dense_finish(c, ex, hp, VANKA_K, info, gather);
  for (int v : info)
    if (v != 0) throw HipError{"Vanka patch matrix singular (getrf/getri info " + std::to_string(v) + ")"};
  if (c->precond32) {
    for (size_t i = 0; i < todo.size(); ++i)
      launch_to_f32(c->st, (int)np_, (int)kk, base[i], (int)kk, todo[i]->vkinvf.p, (int)kk);
    HIPCHK(hipStreamSynchronize(c->st));
  }
}

// Finish half: waits for the issued work, reports a singular block or coarse matrix (same errors as ever), takes
// the pivoted route for the whole batch where a coarse pivot vanished, makes the FP32 copies of the coarse
// inverses on the main stream and marks the data valid.
static void setup_finish(ricadi_ctx* c, SetupJob& job) {
  if (!job.open) return;
  hipStream_t st = c->st;
  const Exec& ex = job.ex;
  const std::vector<ShiftData*>& todo = job.todo;
  double* tph = job.tph;
  HIPCHK(hipStreamSynchronize(ex.st));
  job.open = false;
  Tick tf;                       // (RICADI_TIMING: the issued phases were timed in setup_issue)
  const int k = c->kc;
  const int kd = c->child ? 0 : c->kc;
  const int nb = (int)todo.size();
  std::vector<int> info(nb, 0);
  if (kd > 0) {
    c->coarse_route = invert_dense_finish(c, ex, job.hp, k, info, [&] {
      for (ShiftData* sd : todo)
        launch_combine3(st, (size_t)k * k, c->E0.p, c->EM.p, c->EJ.p, sd->alpha, sd->beta, sd->einv.p);
    });
  }
  tph[3] += tf.lap();
  int flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, ex.flag, sizeof(int), hipMemcpyDeviceToHost, ex.st));
  HIPCHK(hipStreamSynchronize(ex.st));
  for (int i = 0; i < nb; ++i)
    if (info[i] != 0)
      throw HipError{"coarse matrix singular (getrf/getri info " + std::to_string(info[i]) + ")"};
  if (flag) throw HipError{"singular block-Jacobi block"};
  if (c->precond32 && kd > 0) {
    for (ShiftData* sd : todo) {
      const size_t kp = (size_t)(k + 15) / 16;
      if (sd->einvf.n != kp * kp * 256) sd->einvf.alloc(kp * kp * 256);
      launch_to_f32_tiled(st, k, sd->einv.p, sd->einvf.p);
    }
    HIPCHK(hipStreamSynchronize(st));
  }
  if (c->vanka) vanka_setup(c, ex, todo);
  tph[4] += tf.lap();
  if (c->sw.timing && !c->borrowed)
    fprintf(stderr, "[ricadi timing] setup of %d shifts: child %.1f ms, per-shift assembly %.1f, block inverses + Schur blocks %.1f, coarse inverses %.1f, FP32 copies %.1f\n",
            (int)todo.size(), 1e3 * tph[0], 1e3 * tph[1], 1e3 * tph[2], 1e3 * tph[3], 1e3 * tph[4]);
  for (ShiftData* sd : todo) sd->valid = true;
}

// Per-shift data for the given (alpha, beta) pairs, built on the main stream (both halves at once).
static void get_shifts(ricadi_ctx* c, const double* alphas, const double* betas, int ng, ShiftData** out) {
  SetupJob job;
  setup_issue(c, main_exec(c), alphas, betas, ng, out, job);
  setup_finish(c, job);
}

static ShiftData* get_shift(ricadi_ctx* c, double alpha, double beta) {
  ShiftData* sd = nullptr;
  get_shifts(c, &alpha, &beta, 1, &sd);
  return sd;
}

