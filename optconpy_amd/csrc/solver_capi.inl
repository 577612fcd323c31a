// solver_capi.inl -- the C-ABI of include/ricadi.h: the guard macros and the helpers its three files share, then the
// product's entry points (the test probes are in solver_capi_probe.inl, the benchmark's timers in
// solver_capi_timing.inl).
// Part of ricadi_solver.hip (one translation unit; included there in order).

// =====================================================================================
//                                      C  A B I
// =====================================================================================
#define API_BEGIN try {
// ... of every entry that touches the device: on the context's device, whichever the calling thread had current (host
// worker threads start on device 0)
#define API_BEGIN_ON(c) API_BEGIN HIPCHK(hipSetDevice((c)->dev));
// ... returning `status` where nothing was thrown
#define API_END_STATUS(status)                                    \
  }                                                               \
  catch (const ricadi::HipError& e) {                             \
    ricadi::set_error(e.msg);                                     \
    return RICADI_EHIP;                                           \
  }                                                               \
  catch (const std::exception& e) {                               \
    ricadi::set_error(e.what());                                  \
    return RICADI_EHIP;                                           \
  }                                                               \
  catch (...) {                                                   \
    ricadi::set_error("unknown C++ exception");                   \
    return RICADI_EHIP;                                           \
  }                                                               \
  return (status);
#define API_END API_END_STATUS(RICADI_OK)

#define REQUIRE(cond, code, msg)     \
  do {                               \
    if (!(cond)) {                   \
      ricadi::set_error(msg);        \
      return code;                   \
    }                                \
  } while (0)

// ---- argument checks (in front of the try: they return) ------------------------------------------------------------
static int check_panel(const ricadi_ctx* c, int m) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(m >= 1 && m <= RICADI_MAX_M, RICADI_EINVAL, "panel width must be in [1, 128]");
  return RICADI_OK;
}

// columns of one batch: what a slot of the pinned residual buffer holds (ensure_work)
constexpr int kMaxBatchCols = 2048;
static_assert(RICADI_MAX_GROUPS * RICADI_MAX_M <= kMaxBatchCols, "a full batch of the widest panels fits");

// check_panel, and ng groups of such panels (ng*m <= 2048 follows: the static_assert above)
static int check_batch(const ricadi_ctx* c, int ng, int m) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(ng >= 1 && ng <= RICADI_MAX_GROUPS, RICADI_EINVAL, "1 <= ng <= 16 and ng*m <= 2048 required");
  return RICADI_OK;
}

// host Z with cz columns, else the resident factor: is there one?
static int check_factor(const ricadi_ctx* c, const double* Z, int cz) {
  if (Z) REQUIRE(cz > 0, RICADI_EINVAL, "bad column count");
  else REQUIRE(c->zc > 0, RICADI_ESTATE, "no device-resident factor");
  return RICADI_OK;
}

// ---- shared set-up ---------------------------------------------------------------------------------------------------
// What a batched entry sets up before it launches: the shift records, the workspace, the batch (all groups active)
// and, on request, the iteration form and the cycle form the lockstep GMRES decides for such a batch.
struct BatchSetup {
  // kNoWork: the workspace is left as it is; kWorkPlain: ensure_work without room for low-rank columns; kWorkLowRank:
  // with room for the context's low-rank width (the solves)
  enum Work { kNoWork, kWorkPlain, kWorkLowRank };
  enum Forms { kNoForms, kIteration, kCycle };   // kCycle: both
  std::vector<ShiftData*> sds;
  Batch bt;
  IterationForm f;
  CycleForm pf;
  // in_stride: group stride of the cycle's FP64 input (0: the batch's own, n*m); where the cycle reads the FP16-stored
  // vector instead, that one has the batch's stride
  BatchSetup(ricadi_ctx* c, int ng, const double* alphas, const double* betas, int m, Work work, Forms forms = kNoForms,
             size_t in_stride = 0)
      : sds(ng) {
    get_shifts(c, alphas, betas, ng, sds.data());
    if (work == kWorkPlain) ensure_work(c, m, ng, 0);
    if (work == kWorkLowRank) ensure_work(c, m, ng);
    bt = make_batch(c, sds.data(), ng, m);
    if (forms != kNoForms) f = iteration_form(c, m, ng, false);
    if (forms == kCycle) pf = cycle_form(c, m, bt.blocks16, f.h16 || !in_stride ? bt.gs : in_stride, f.x32, f.h16);
  }
};

// The factor an entry works on: the host Z with cz columns, staged on the device here, else the resident one
// (check_factor has passed)
struct FactorArg {
  DArr<double> stage;
  const double* p;
  int cz, ld;
  FactorArg(ricadi_ctx* c, const double* Z, int cz_host) : p(c->Z.p), cz(c->zc), ld(c->zld) {
    if (!Z) return;
    stage.alloc((size_t)c->nv * cz_host);
    HIPCHK(hipMemcpyAsync(stage.p, Z, sizeof(double) * c->nv * cz_host, hipMemcpyHostToDevice, c->st));
    p = stage.p;
    cz = ld = cz_host;
  }
};

// The resident factor (nv x zc, zc > 0) packed into the host array Z_out; synchronous
static void factor_download(ricadi_ctx* c, double* Z_out) {
  HIPCHK(hipMemcpy2DAsync(Z_out, sizeof(double) * c->zc, c->Z.p, sizeof(double) * c->zld, sizeof(double) * c->zc, c->nv,
                          hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
}

extern "C" {

const char* ricadi_last_error(void) { return ricadi::g_err.c_str(); }
int ricadi_version(void) { return 414; }
int ricadi_sizeof_opts(void) { return (int)sizeof(ricadi_opts); }
int ricadi_sizeof_adi_params(void) { return (int)sizeof(ricadi_adi_params); }
// field types in declaration order (d = double, i = int); keep in step with include/ricadi.h
const char* ricadi_struct_signature(void) { return "ricadi_opts:diiiiiiiiiiiid;ricadi_adi_params:iddiddiiii"; }

void ricadi_default_opts(ricadi_opts* o) {
  if (!o) return;
  o->gmres_tol = 1e-10;
  o->gmres_restart = 30;
  o->gmres_maxit = 3000;
  o->bj_block = 32;
  o->agg_v = 16;
  o->agg_p = 24;
  o->coarse_max = 4096;
  o->use_coarse = 1;
  o->max_levels = 3;
  o->verbose = 0;
  o->compress_qr = 1;
  o->hierarchy = 0;
  o->child_smoother = 0;
  o->child_damping = 0.7;
}

void ricadi_default_adi_params(ricadi_adi_params* p) {
  if (!p) return;
  // /root/reference/optcont_main.py:122-131
  p->adi_max_steps = 200;
  p->adi_newZ_reltol = 1e-8;
  p->nwtn_max_steps = 16;
  p->nwtn_upd_reltol = 5e-8;
  p->nwtn_upd_abstol = 1e-7;
  p->project_w = 1;
  p->verbose = 0;
  p->compress_cols = 0;
  p->sweep_width = 1;
  p->adi_res_reltol = 0.0;
}

// The only reading of the library's switches (ricadi_ctx::sw); RICADI_RECYCLE and RICADI_INJECT_SWEEP_FAILURE are
// read per call instead (solver_adi.inl)
static Switches read_switches() {
  auto set = [](const char* name) { return getenv(name) != nullptr; };
  auto off = [](const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '0';
  };
  Switches s;
  s.precond64 = set("RICADI_PRECOND64");
  s.basis64 = set("RICADI_BASIS64");
  s.basis32 = set("RICADI_BASIS32");
  s.timing = set("RICADI_TIMING");
  s.debug_sweeps = set("RICADI_DEBUG_SWEEPS");
  s.smw = !off("RICADI_SMW");
  s.wide_split = !(getenv("RICADI_WIDE_SPLIT") && atoi(getenv("RICADI_WIDE_SPLIT")) == 0);
  if (const char* e = getenv("RICADI_SA")) s.sa_omega = atof(e);
  s.sweep_meta = !off("RICADI_SWEEP_META");
  s.ms_spmm = !off("RICADI_MS_SPMM");
  s.ms_force = getenv("RICADI_MS_SPMM") && getenv("RICADI_MS_SPMM")[0] == '2';
  s.w32 = !off("RICADI_W32");
  s.x32_always = !off("RICADI_X32");
  s.blocks16 = !off("RICADI_BLOCKS16");
  s.rowwave = !off("RICADI_ROWWAVE");
  s.mid32 = !off("RICADI_MID32");
  s.coarse_pipe = !off("RICADI_COARSE_PIPE");
  if (const char* e = getenv("RICADI_ARNOLDI")) s.lowsync = strcmp(e, "cgs2") != 0;
  s.fuseh = !off("RICADI_FUSEH");
  s.split = !off("RICADI_SPLIT");
  s.setup_overlap = !off("RICADI_SETUP_OVERLAP");
  return s;
}

int ricadi_create(int device_id, ricadi_ctx** out) {
  REQUIRE(out, RICADI_EINVAL, "ricadi_create: ctx is NULL");
  *out = nullptr;
  API_BEGIN
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (ndev <= 0) throw ricadi::HipError{"no HIP device visible (this library has no CPU fallback)"};
  if (device_id < 0 || device_id >= ndev) throw ricadi::HipError{"bad device id"};
  HIPCHK(hipSetDevice(device_id));
  std::unique_ptr<ricadi_ctx> c(new ricadi_ctx);
  c->dev = device_id;
  ricadi_default_opts(&c->opts);
  c->sw = read_switches();
  c->precond32 = !c->sw.precond64;
  HIPCHK(hipStreamCreate(&c->st));
  RBCHK(rocblas_create_handle(&c->rb));
  RBCHK(rocblas_set_stream(c->rb, c->st));
  c->flag.alloc(4);
  c->info.alloc(4);
  *out = c.release();
  API_END
}

int ricadi_destroy(ricadi_ctx* ctx) {
  if (!ctx) return RICADI_OK;
  API_BEGIN
  (void)hipSetDevice(ctx->dev);
  (void)hipStreamSynchronize(ctx->st);
  delete ctx;
  API_END
}

int ricadi_set_opts(ricadi_ctx* c, const ricadi_opts* o) {
  REQUIRE(c && o, RICADI_EINVAL, "ricadi_set_opts: NULL argument");
  REQUIRE(o->gmres_restart >= 2 && o->gmres_restart <= 400, RICADI_EINVAL, "gmres_restart out of range");
  REQUIRE(o->gmres_tol > 0 && o->gmres_maxit > 0, RICADI_EINVAL, "bad gmres_tol / gmres_maxit");
  REQUIRE(o->hierarchy == 0 || o->hierarchy == 1, RICADI_EINVAL, "hierarchy must be 0 or 1");
  REQUIRE(o->child_smoother == 0 || o->child_smoother == 1, RICADI_EINVAL, "child_smoother must be 0 or 1");
  REQUIRE(o->child_damping > 0 && o->child_damping <= 2, RICADI_EINVAL, "child_damping out of range");
  const bool structural = c->has_op && (o->bj_block != c->opts.bj_block || o->agg_v != c->opts.agg_v ||
                                        o->agg_p != c->opts.agg_p || o->coarse_max != c->opts.coarse_max ||
                                        o->max_levels != c->opts.max_levels ||
                                        o->use_coarse != c->opts.use_coarse ||
                                        o->hierarchy != c->opts.hierarchy ||
                                        o->child_smoother != c->opts.child_smoother ||
                                        o->child_damping != c->opts.child_damping);
  REQUIRE(!structural, RICADI_ESTATE, "preconditioner options must be set before ricadi_set_operator");
  c->opts = *o;
  return RICADI_OK;
}

void* ricadi_stream(ricadi_ctx* c) { return c ? (void*)c->st : nullptr; }

int ricadi_synchronize(ricadi_ctx* c) {
  REQUIRE(c, RICADI_EINVAL, "NULL ctx");
  API_BEGIN_ON(c)
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

// Everything a context holds that is tied to the resident operator or left by calls on it ("what a context
// remembers"): ricadi_set_operator -- the child level's included -- and ricadi_set_dims forget through this one
// helper, so they cannot differ in what they forget.  Workspaces and scratch keep their capacity; settings (recycle
// depth, RADI modes, the probe's refuse list, the exchange, the options) and the cumulative counters (solve trace,
// total_iters, exchange count) stay.  Leaves has_op false: the caller says what the context describes next.
static void forget_operator(ricadi_ctx* c) {
  c->has_op = false;
  c->cache.clear();
  c->radi_sdv.clear();
  c->child.reset();
  c->q = 0;
  c->zc = 0;
  c->wcols = 0;                // workspaces depend on n
  c->cw.groups = c->cw.nvec = c->cw.n = 0;   // ... the complex ones too
  c->cw.basis = false;
  // the ring goes, slots and all: recycle_guess lists its entries in slot order, so a ring that kept its (invalid)
  // slots would fill them in another order than a fresh context's growing ring, and the normal equations of the same
  // guess would come out permuted -- other rounding, other bits (found by tests/test_gpu_context_reuse.py)
  c->rec_ring.clear();
  c->rec_pan_w = 0;
  c->lr_ucol = -1;
  // "of the last call": a reporter asked now answers as a fresh context's does
  c->adi_ran = false;
  c->adi_res_hist.clear();
  c->adi_stop_rule = 0;
  c->newton_ran = false;
  c->newton_hist.clear();
  c->newton_stop_rule = 0;
  c->radi_ran = false;
  c->radi_shift_hist.clear();
  c->radi_fallbacks = 0;
  c->radi_kept_hist.clear();
  c->radi_qr_repeats = c->radi_recompressions = 0;
  c->radi_sweep_info[0] = 1;
  c->radi_sweep_info[1] = c->radi_sweep_info[2] = 0;
  c->radi_sweep_widths.clear();
  c->w32_last = c->mid32_last = -1;
  c->k1_variant = -1;
  c->coarse_route = -1;
  c->probe = ricadi_ctx::ArnoldiProbe();
  c->cprobe = ricadi_ctx::CplxProbe();
}

int ricadi_set_operator(ricadi_ctx* c, int nv, int np, const int32_t* a_rp, const int32_t* a_ci,
                        const double* a_v, const int32_t* e_rp, const int32_t* e_ci,
                        const double* e_v, const int32_t* j_rp, const int32_t* j_ci,
                        const double* j_v) {
  REQUIRE(c, RICADI_EINVAL, "NULL ctx");
  REQUIRE(nv > 0 && np >= 0, RICADI_EINVAL, "bad sizes");
  REQUIRE(a_rp && e_rp, RICADI_EINVAL, "NULL matrix");
  REQUIRE((a_ci && a_v) || a_rp[nv] == 0, RICADI_EINVAL, "NULL matrix arrays");
  REQUIRE((e_ci && e_v) || e_rp[nv] == 0, RICADI_EINVAL, "NULL matrix arrays");
  REQUIRE(np == 0 || (j_rp && j_ci && j_v), RICADI_EINVAL, "NULL J");
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  HostCsr A = make_csr(nv, nv, a_rp, a_ci, a_v);
  HostCsr E = make_csr(nv, nv, e_rp, e_ci, e_v);
  HostCsr J;
  if (np > 0) {
    J = make_csr(np, nv, j_rp, j_ci, j_v);
  } else {
    J.nrows = 0;
    J.ncols = nv;
    J.rp.assign(1, 0);
  }
  for (size_t k = 0; k < A.nnz(); ++k)
    if (A.ci[k] < 0 || A.ci[k] >= nv) throw ricadi::HipError{"A: column index out of range"};
  for (size_t k = 0; k < E.nnz(); ++k)
    if (E.ci[k] < 0 || E.ci[k] >= nv) throw ricadi::HipError{"E: column index out of range"};
  for (size_t k = 0; k < J.nnz(); ++k)
    if (J.ci[k] < 0 || J.ci[k] >= nv) throw ricadi::HipError{"J: column index out of range"};
  // everything shift independent, on the host
  if (!c->borrowed) c->levels = root_levels(c->opts);
  // smoothed aggregation of the velocity prolongation: two-level setups, folded preconditioner cycle only
  const double sa_omega = (c->borrowed || np == 0 || c->opts.bj_block != 32) ? 0.0 : c->sw.sa_omega;
  const HostCsr JT = transpose(J);
  const HostSetup hs = build_setup_checked(A, E, J, JT, c->opts, c->levels, sa_omega);
  const PrecondRecords pr = build_records(hs, J, JT, c->sw.sweep_meta, c->sw.ms_spmm);
  // validation ends here: what follows replaces the resident operator.  has_op is false from this first mutation to
  // the last statement, and the sizes are zero until the upload sets them, so a replacement that fails half way leaves
  // a context that refuses every call ("set the operator first") instead of one that describes the old operator
  // without its child level and its cache
  forget_operator(c);
  c->nv = c->np = c->n = 0;
  // the child level (same stream and rocBLAS handle) takes the coarse problem
  if (hs.multilevel) {
    std::unique_ptr<ricadi_ctx> ch(new ricadi_ctx);
    ch->dev = c->dev;
    ch->st = c->st;
    ch->rb = c->rb;
    ch->borrowed = true;
    // options and depth of the child level (ricadi_host.cpp; ricadi_host_plan_hierarchy walks the same chain): its
    // aggregates are pairs and double until its dense inverse fits, or -- the fine hierarchy -- stay pairs with a
    // child of its own below
    ch->opts = child_opts(c->opts, c->borrowed);
    ch->levels = child_levels(c->opts, c->levels);
    ch->sw = c->sw;
    ch->sw.timing = false;              // the parent times the child's setup as one phase
    ch->precond32 = c->precond32;
    ch->flag.alloc(4);
    ch->info.alloc(4);
    const int rc = ricadi_set_operator(ch.get(), hs.kcv, hs.kcp, hs.l1A.rp.data(), hs.l1A.ci.data(), hs.l1A.v.data(),
                                       hs.l1E.rp.data(), hs.l1E.ci.data(), hs.l1E.v.data(), hs.l1J.rp.data(),
                                       hs.l1J.ci.data(), hs.l1J.v.data());
    if (rc != RICADI_OK) throw ricadi::HipError{std::string("child level: ") + ricadi_last_error()};
    c->child = std::move(ch);
  }
  // upload
  c->nv = nv;
  c->np = np;
  c->n = nv + np;
  c->bs = hs.bs;
  c->nbv = hs.nbv;
  c->nbp = hs.nbp;
  c->kc = hs.kc;
  c->agg_v = hs.agg_v;
  c->agg_p = hs.agg_p;
  c->sa = hs.sa;
  c->snnz = hs.s_ci.size();
  c->s_rp.upload(hs.s_rp, st);
  c->s_ci.upload(hs.s_ci, st);
  c->srcA.upload(hs.s_srcA, st);
  c->srcE.upload(hs.s_srcE, st);
  c->srcJ.upload(hs.s_srcJ, st);
  c->A.upload(A, st);
  c->E.upload(E, st);
  c->J.upload(J, st);
  c->JT.upload(JT, st);
  // a child level's coloured Vanka sweep: patches and colours from its J (shift independent)
  c->vanka = c->borrowed && c->opts.child_smoother == 1 && np > 0;
  c->vk = c->vanka ? vanka_patches(nv, J) : VankaPatches();
  c->vk_idx.upload(c->vk.idx, st);
  c->gt_ok = pr.gt_ok;
  c->gt_ks = pr.gt_ks;
  c->gt_ptr.upload(pr.gt_ptr, st);
  c->gt_cols.upload(pr.gt_cols, st);
  c->gt_jtd.upload(pr.jtd, st);
  c->bv_ptr.upload(hs.bv_ptr, st);
  c->bv_rows.upload(hs.bv_rows, st);
  c->bp_ptr.upload(hs.bp_ptr, st);
  c->bp_rows.upload(hs.bp_rows, st);
  c->bvA.upload(hs.bv_A, st);
  c->bvE.upload(hs.bv_E, st);
  c->jd_ptr.upload(hs.jd_ptr, st);
  c->jd_vblk.upload(hs.jd_vblk, st);
  c->jd_val.upload(hs.jd_val, st);
  c->agg_ptr.upload(hs.agg_ptr, st);
  c->agg_rows.upload(hs.agg_rows, st);
  c->aggof.upload(hs.aggof, st);
  c->pt_rp.upload(hs.pt_rp, st);
  c->pt_ci.upload(hs.pt_ci, st);
  c->pt_v.upload(hs.pt_v, st);
  c->synnz = hs.sy_ci.size();
  c->sy_chunk = pr.sy_chunk;
  c->sy_rp.upload(hs.sy_rp, st);
  c->sy_ci.upload(hs.sy_ci, st);
  c->ps_meta.upload(pr.ps_meta, st);
  c->sy_A.upload(hs.sy_A, st);
  c->sy_E.upload(hs.sy_E, st);
  c->sy_J.upload(hs.sy_J, st);
  c->ady_ok = pr.ady_ok;
  c->ady_ks = pr.ady_ks;
  c->cy_ptr.upload(pr.cy_ptr, st);
  c->cy_cols.upload(pr.cy_cols, st);
  c->cy_dA.upload(pr.dA, st);
  c->cy_dE.upload(pr.dE, st);
  c->cy_dJ.upload(pr.dJ, st);
  c->cy_dT.upload(pr.dT, st);
  c->sw_meta.upload(pr.sw_meta, st);
  c->sw_stride = pr.sw_stride;
  c->sw_in_rect = pr.sw_in_rect;
  c->sw_in_two = pr.sw_in_two;
  c->syb_ok = pr.syb_ok;
  c->syb_max_cols = hs.syb_max_cols;
  if (c->syb_ok) {
    c->syb_rp2.upload(pr.syb_rp2, st);
    c->syb_cols2.upload(pr.syb_cols2, st);
    c->syb_perm.upload(hs.syb_perm, st);
    c->syb_lidx.upload(hs.syb_lidx, st);
  }
  c->E0.upload(hs.E0, st);
  c->EM.upload(hs.EM, st);
  c->EJ.upload(hs.EJ, st);
  c->ones.upload(std::vector<double>((size_t)c->n, 1.0), st);
  c->sb_nblk = hs.sb_nblk;
  c->sb_max_cols = hs.sb_max_cols;
  c->sb_max_nnz = hs.sb_max_nnz;
  c->sb_rows2.upload(pr.sb_rows2, st);
  c->sb_rp2.upload(pr.sb_rp2, st);
  c->sb_cols2.upload(pr.sb_cols2, st);
  c->sb_colsm2.upload(pr.sb_colsm2, st);
  c->sb_perm.upload(hs.sb_perm, st);
  c->sb_lidx.upload(hs.sb_lidx, st);
  c->sb_ok = pr.sb_ok;
  c->ms_ok = pr.ms_ok;
  c->sbAJ.upload(pr.sbAJ, st);
  c->sbE.upload(pr.sbE, st);
  c->sb_lidx_ms.upload(pr.sb_lidx_ms, st);
  c->sybAJ.upload(pr.sybAJ, st);
  c->sybE.upload(pr.sybE, st);
  c->syb_lidx_ms.upload(pr.syb_lidx_ms, st);
  HIPCHK(hipStreamSynchronize(st));
  if (c->opts.verbose) {
    if (pr.gt_ok)
      fprintf(stderr, "[ricadi] last velocity sweep in rectangular form: <= %d pressure dofs per block (slice width %d)\n",
              pr.gt_kmax, pr.gt_ks);
    fprintf(stderr, "[ricadi] prolongated operator S*Y: %.1f entries per row\n", (double)c->synnz / std::max(c->n, 1));
    fprintf(stderr, "[ricadi] operator nv=%d np=%d nnz(S)=%zu | BJ blocks %d+%d (bs=%d) | coarse %d (%d+%d) | "
            "SpMM row blocks %d (max %d distinct cols, %d nnz; mean %.0f cols)\n",
            nv, np, c->snnz, c->nbv, c->nbp, c->bs, c->kc, hs.kcv, hs.kcp, hs.sb_nblk,
            hs.sb_max_cols, hs.sb_max_nnz, hs.sb_nblk ? (double)hs.sb_cols.size() / hs.sb_nblk : 0.0);
  }
  c->has_op = true;
  API_END
}

int ricadi_clear_cache(ricadi_ctx* c) {
  REQUIRE(c, RICADI_EINVAL, "NULL ctx");
  API_BEGIN_ON(c)
  HIPCHK(hipStreamSynchronize(c->st));
  for (ricadi_ctx* l = c; l; l = l->child.get())
    for (auto& kv : l->cache) {
      kv.second->valid = false;   // buffers stay
      for (auto& r : kv.second->rec) r->serial = -1;
    }
  for (auto& e : c->rec_ring) e->serial = -1;
  API_END
}

int ricadi_set_recycle(ricadi_ctx* c, int depth) {
  REQUIRE(c && depth >= 0 && depth <= 8, RICADI_EINVAL, "recycling depth must be in [0, 8]");
  c->rec_user_depth = c->rec_depth = depth;
  return RICADI_OK;
}

// the exchange state of a context back to "none" (a communicator the library created is destroyed)
static void exchange_reset(ricadi_ctx* c) {
  if (c->xcomm && c->xcomm_owned) (void)ncclCommDestroy(c->xcomm);
  c->xcomm = nullptr;
  c->xcomm_owned = false;
  c->xforce = false;
  c->xsend_own.release();
  c->xrecv_own.release();
  c->xrank = 0;
  c->xworld = 1;
  c->xfn = nullptr;
  c->xuser = nullptr;
  c->xsend = c->xrecv = nullptr;
  c->xcap = 0;
}

int ricadi_set_exchange(ricadi_ctx* c, int rank, int world, ricadi_allgather_fn fn, void* user,
                        void* send_dev, void* recv_dev, int64_t send_capacity) {
  REQUIRE(c, RICADI_EINVAL, "NULL ctx");
  API_BEGIN_ON(c)
  exchange_reset(c);
  if (world <= 1 || !fn) return RICADI_OK;
  REQUIRE(rank >= 0 && rank < world && world <= 64, RICADI_EINVAL, "bad rank / world size");
  REQUIRE(send_dev && recv_dev && send_capacity >= 2 * RICADI_XCTL, RICADI_EINVAL, "exchange buffers missing or too small");
  c->xrank = rank;
  c->xworld = world;
  c->xfn = fn;
  c->xuser = user;
  c->xsend = static_cast<double*>(send_dev);
  c->xrecv = static_cast<double*>(recv_dev);
  c->xcap = (size_t)send_capacity;
  API_END
}

int ricadi_rccl_unique_id(void* id_out, int bytes) {
  REQUIRE(id_out && bytes >= (int)sizeof(ncclUniqueId), RICADI_EINVAL, "id buffer of at least 128 bytes required");
  ncclUniqueId id;
  const ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) {
    ricadi::set_error(std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    return RICADI_EHIP;
  }
  std::memcpy(id_out, &id, sizeof(id));
  return RICADI_OK;
}

int ricadi_set_exchange_rccl(ricadi_ctx* c, int rank, int world, const void* unique_id, void* comm,
                             int64_t send_capacity) {
  REQUIRE(c, RICADI_EINVAL, "NULL ctx");
  REQUIRE(world >= 1 && world <= 64 && rank >= 0 && rank < world, RICADI_EINVAL, "bad rank / world size");
  const bool resize = !unique_id && !comm;      // keep the communicator, new buffer sizes
  REQUIRE(!resize || (c->xcomm && c->xrank == rank && c->xworld == world), RICADI_EINVAL,
          "a unique id (ricadi_rccl_unique_id) or a communicator is required");
  REQUIRE(send_capacity >= 2 * RICADI_XCTL, RICADI_EINVAL, "send_capacity too small");
  API_BEGIN_ON(c)
  if (resize) {
    HIPCHK(hipStreamSynchronize(c->st));
  } else if (comm) {
    exchange_reset(c);
    c->xcomm = static_cast<ncclComm_t>(comm);
  } else {
    exchange_reset(c);
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof(id));
    const ncclResult_t r = ncclCommInitRank(&c->xcomm, world, id, rank);
    if (r != ncclSuccess) {
      c->xcomm = nullptr;
      throw HipError{std::string("ncclCommInitRank: ") + ncclGetErrorString(r)};
    }
    c->xcomm_owned = true;
  }
  const size_t cap = ((size_t)send_capacity + 7) / 8;
  c->xsend_own.alloc(cap);
  c->xrecv_own.alloc(cap * world);
  HIPCHK(hipMemsetAsync(c->xsend_own.p, 0, cap * sizeof(double), c->st));
  HIPCHK(hipMemsetAsync(c->xrecv_own.p, 0, cap * world * sizeof(double), c->st));
  c->xrank = rank;
  c->xworld = world;
  c->xforce = world == 1;
  c->xsend = c->xsend_own.p;
  c->xrecv = c->xrecv_own.p;
  c->xcap = cap * sizeof(double);
  API_END
}

int ricadi_exchange_count(ricadi_ctx* c, int64_t* count_out) {
  REQUIRE(c && count_out, RICADI_EINVAL, "NULL argument");
  *count_out = (int64_t)c->xcount;
  return RICADI_OK;
}

int ricadi_set_dims(ricadi_ctx* c, int nv) {
  REQUIRE(c && nv > 0, RICADI_EINVAL, "bad argument");
  forget_operator(c);
  c->nv = nv;
  c->np = 0;
  c->n = nv;
  return RICADI_OK;
}

int ricadi_set_lowrank(ricadi_ctx* c, const double* U, const double* V, int q) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(q >= 0 && q <= 64, RICADI_EINVAL, "low-rank width must be in [0, 64]");
  REQUIRE(q == 0 || (U && V), RICADI_EINVAL, "NULL low-rank factor");
  API_BEGIN_ON(c)
  c->q = q;
  ++c->lr_epoch;
  if (q > 0) {
    const size_t cnt = (size_t)c->nv * q;
    c->U.ensure(cnt);
    c->V.ensure(cnt);
    HIPCHK(hipMemcpyAsync(c->U.p, U, cnt * sizeof(double), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipMemcpyAsync(c->V.p, V, cnt * sizeof(double), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  }
  API_END
}

int ricadi_spmm_dev(ricadi_ctx* c, double alpha, double beta, const double* dX, int m, double* dY) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(dX && dY, RICADI_EINVAL, "NULL panel");
  API_BEGIN_ON(c)
  ShiftData* sd = get_shift(c, alpha, beta);
  ensure_work(c, m);
  op_apply(c, sd, dX, dY, m, true);
  API_END
}

int ricadi_spmm(ricadi_ctx* c, double alpha, double beta, const double* X, int m, double* Y) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(X && Y, RICADI_EINVAL, "NULL panel");
  API_BEGIN_ON(c)
  const size_t nm = (size_t)c->n * m;
  ShiftData* sd = get_shift(c, alpha, beta);
  ensure_work(c, m);
  HIPCHK(hipMemcpyAsync(c->pw1.p, X, nm * sizeof(double), hipMemcpyHostToDevice, c->st));
  op_apply(c, sd, c->pw1.p, c->pw2.p, m, true);
  HIPCHK(hipMemcpyAsync(Y, c->pw2.p, nm * sizeof(double), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

int ricadi_precond_apply(ricadi_ctx* c, double alpha, double beta, const double* R, int m, double* Z) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(R && Z, RICADI_EINVAL, "NULL panel");
  API_BEGIN_ON(c)
  const size_t nm = (size_t)c->n * m;
  ShiftData* sd = get_shift(c, alpha, beta);
  ensure_work(c, m);
  HIPCHK(hipMemcpyAsync(c->pw1.p, R, nm * sizeof(double), hipMemcpyHostToDevice, c->st));
  precond_apply(c, sd, c->pw1.p, c->pw2.p, m);
  HIPCHK(hipMemcpyAsync(Z, c->pw2.p, nm * sizeof(double), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

static int solve_status(bool converged) {
  if (!converged) ricadi::set_error("GMRES did not reach the tolerance");
  return converged ? RICADI_OK : RICADI_ENOCONV;
}

int ricadi_shift_solve_dev(ricadi_ctx* c, double alpha, double beta, const double* dR, int m,
                           double* dX, int* iters_out, double* relres_out) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(dR && dX, RICADI_EINVAL, "NULL panel");
  int status = RICADI_OK;
  API_BEGIN_ON(c)
  ShiftData* sd = get_shift(c, alpha, beta);
  ensure_work(c, m);
  load_rhs(c, dR, m, c->bvec.p);
  GmresResult r = gmres_solve(c, sd, c->bvec.p, dX, m, true, relres_out);
  if (iters_out) *iters_out = r.iters;
  status = solve_status(r.converged);
  API_END_STATUS(status)
}

int ricadi_shift_solve_batch_dev(ricadi_ctx* c, int ng, const double* alphas, const double* betas,
                                 const double* dR, int64_t r_stride, int m, double* dX,
                                 int* iters_out, double* relres_out) {
  if (int rc = check_batch(c, ng, m)) return rc;
  REQUIRE(dR && dX && alphas && betas, RICADI_EINVAL, "NULL argument");
  REQUIRE(r_stride == 0 || r_stride >= (int64_t)c->nv * m, RICADI_EINVAL, "bad r_stride");
  int status = RICADI_OK;
  API_BEGIN_ON(c)
  BatchSetup s(c, ng, alphas, betas, m, BatchSetup::kWorkLowRank);
  const size_t nm = (size_t)c->n * m;
  const int nload = r_stride == 0 ? 1 : ng;
  for (int g = 0; g < nload; ++g) load_rhs(c, dR + (size_t)g * r_stride, m, c->bvec.p + (size_t)g * nm);
  std::vector<GmresResult> res(ng);
  solve_batch(c, s.sds.data(), ng, c->bvec.p, r_stride == 0 ? 0 : nm, dX, m, true, relres_out,
              res.data());
  for (int g = 0; g < ng; ++g) {
    if (iters_out) iters_out[g] = res[g].iters;
    if (!res[g].converged) status = solve_status(false);
  }
  API_END_STATUS(status)
}

int ricadi_recycle_guess_dev(ricadi_ctx* c, int ng, const double* alphas, const double* betas, const double* dR, int m,
                             double* dX, int* rank_out) {
  if (int rc = check_batch(c, ng, m)) return rc;
  REQUIRE(dR && dX && alphas && betas && rank_out, RICADI_EINVAL, "NULL argument");
  *rank_out = 0;
  API_BEGIN_ON(c)
  BatchSetup s(c, ng, alphas, betas, m, BatchSetup::kWorkLowRank);
  load_rhs(c, dR, m, c->bvec.p);
  if (c->rec_depth > 0 && recycle_guess(c, s.sds.data(), ng, c->bvec.p, m, dX)) *rank_out = (int)c->trace.guess_rank;
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

int ricadi_shift_solve(ricadi_ctx* c, double alpha, double beta, const double* R, const double* Rp,
                       int m, double* X_out, int* iters_out, double* relres_out) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(R && X_out, RICADI_EINVAL, "NULL panel");
  int status = RICADI_OK;
  API_BEGIN_ON(c)
  const size_t nm = (size_t)c->n * m, nvm = (size_t)c->nv * m;
  ShiftData* sd = get_shift(c, alpha, beta);
  ensure_work(c, m);
  HIPCHK(hipMemcpyAsync(c->bvec.p, R, nvm * sizeof(double), hipMemcpyHostToDevice, c->st));
  if (c->np > 0) {
    if (Rp)
      HIPCHK(hipMemcpyAsync(c->bvec.p + nvm, Rp, (nm - nvm) * sizeof(double), hipMemcpyHostToDevice, c->st));
    else
      HIPCHK(hipMemsetAsync(c->bvec.p + nvm, 0, (nm - nvm) * sizeof(double), c->st));
  }
  GmresResult r = gmres_solve(c, sd, c->bvec.p, c->xs.p, m, true, relres_out);
  HIPCHK(hipMemcpyAsync(X_out, c->xs.p, nm * sizeof(double), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  if (iters_out) *iters_out = r.iters;
  status = solve_status(r.converged);
  API_END_STATUS(status)
}

int ricadi_apply_e_dev(ricadi_ctx* c, double coef, const double* dV, int m, double* dW) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(dV && dW, RICADI_EINVAL, "NULL panel");
  API_BEGIN_ON(c)
  launch_spmm(c->st, c->nv, c->E.rp.p, c->E.ci.p, c->E.v.p, dV, m, nullptr, dW, m, dW, m, coef, 1.0,
              nullptr, m);
  API_END
}

int ricadi_lincomb_dev(ricadi_ctx* c, int nrows, int m, int nvec, const double* dBasis,
                       int64_t stride, const double* coef, double* dOut) {
  REQUIRE(c && dBasis && coef && dOut, RICADI_EINVAL, "NULL argument");
  REQUIRE(nrows > 0 && m >= 1 && m <= RICADI_MAX_M && nvec >= 1 && nvec <= 64, RICADI_EINVAL,
          "bad sizes");
  API_BEGIN_ON(c)
  std::vector<double> h((size_t)nvec * m);
  for (int i = 0; i < nvec; ++i)
    for (int j = 0; j < m; ++j) h[(size_t)i * m + j] = coef[i];
  c->scratch.ensure((size_t)nvec * m + 64);
  HIPCHK(hipMemcpyAsync(c->scratch.p, h.data(), sizeof(double) * nvec * m, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  launch_cols_update(c->st, nrows, m, nvec, dBasis, (size_t)stride, c->scratch.p, 1.0, nullptr, nullptr,
                     dOut);
  API_END
}

int ricadi_sweep_recombine_slots_dev(ricadi_ctx* c, int nslot, int G, const double* dU, int m,
                                     const double* coefz, const double* coefw, double* dZ, double* dW,
                                     double* n2_out, double* block_n2_out) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(dU && coefz && coefw && dZ && dW && n2_out, RICADI_EINVAL, "NULL argument");
  REQUIRE(G >= 1 && G <= 64 && nslot >= 1 && nslot <= 128 && G * m <= 2048, RICADI_EINVAL,
          "1 <= G <= 64, 1 <= nslot <= 128 and G*m <= 2048 required");
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  const int nv = c->nv;
  const size_t nvm = (size_t)nv * m;
  ensure_work(c, m, std::min(G, RICADI_MAX_GROUPS));
  c->sweep_t.ensure(nvm);
  c->sweep_coef.ensure((size_t)(G + 1) * nslot * m);
  c->nrm2.ensure((size_t)G * m);
  // coefficient rows replicated over the m columns: G columns of coefz, then coefw
  std::vector<double> coef((size_t)(G + 1) * nslot * m);
  for (int j = 0; j <= G; ++j)
    for (int i = 0; i < nslot; ++i) {
      const double v = j < G ? coefz[(size_t)i * G + j] : coefw[i];
      for (int cc = 0; cc < m; ++cc) coef[((size_t)j * nslot + i) * m + cc] = v;
    }
  HIPCHK(hipMemcpyAsync(c->sweep_coef.p, coef.data(), sizeof(double) * coef.size(),
                        hipMemcpyHostToDevice, st));
  // Z-block j = sum_i coefz[i][j] U_i  (columns j*m .. of dZ, leading dimension G*m): the ADI driver's own
  // recombination (fused kernel up to 16 slots and 16 blocks, per block beyond)
  sweep_blocks(c, dU, nvm, nslot, G, m, c->sweep_coef.p, dZ, G * m, 0, c->nrm2.p);
  // W += E (sum_i coefw[i] U_i)
  launch_cols_update(st, nv, m, nslot, dU, nvm, c->sweep_coef.p + (size_t)G * nslot * m, 1.0, nullptr,
                     nullptr, c->sweep_t.p);
  launch_spmm(st, nv, c->E.rp.p, c->E.ci.p, c->E.v.p, c->sweep_t.p, m, nullptr, dW, m, dW, m, 1.0, 1.0,
              nullptr, m);
  std::vector<double> nr((size_t)G * m);
  HIPCHK(hipMemcpyAsync(nr.data(), c->nrm2.p, sizeof(double) * G * m, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));   // also keeps `coef` alive until its upload has run
  double n2 = 0.0;
  for (double v : nr) n2 += v;
  *n2_out = n2;
  if (block_n2_out)
    for (int j = 0; j < G; ++j) {
      double b2 = 0.0;
      for (int cc = 0; cc < m; ++cc) b2 += nr[(size_t)j * m + cc];
      block_n2_out[j] = b2;
    }
  API_END
}

int ricadi_sweep_recombine_dev(ricadi_ctx* c, int G, const double* dU, int m, const double* rinv,
                               const double* cinv1, double* dZ, double* dW, double* n2_out) {
  return ricadi_sweep_recombine_slots_dev(c, G, G, dU, m, rinv, cinv1, dZ, dW, n2_out, nullptr);
}

int ricadi_gain_dev(ricadi_ctx* c, double coef, const double* dZ, int cz, int ldz, const double* dB,
                    int nb, double* dK) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(dZ && dB && dK && cz > 0 && ldz >= cz && nb >= 1 && nb <= RICADI_MAX_M, RICADI_EINVAL,
          "bad argument");
  API_BEGIN_ON(c)
  gain_dev(c, c->E, dZ, cz, ldz, dB, nb, dK);
  if (coef != 1.0) launch_axpby(c->st, (size_t)c->nv * nb, coef, dK, 0.0, dK);
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

int ricadi_panel_norms_dev(ricadi_ctx* c, const double* dW, int nrows, int m, double* gram_fro,
                           double* nrm2) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(dW && nrows > 0, RICADI_EINVAL, "bad panel");
  API_BEGIN_ON(c)
  gram_norms(c, dW, nrows, m, gram_fro, nrm2);
  API_END
}

int ricadi_qr(ricadi_ctx* c, const double* Z, int cz, double* Q_out, double* R_out) {
  REQUIRE(c && c->nv > 0, RICADI_ESTATE, "set the operator (or the dimensions) first");
  REQUIRE(Z && R_out && cz > 0 && cz <= c->nv, RICADI_EINVAL, "bad argument");
  API_BEGIN_ON(c)
  const int nv = c->nv;
  DArr<double> dZ, dQ, dR;
  dZ.alloc((size_t)nv * cz);
  dQ.alloc((size_t)nv * cz);
  dR.alloc((size_t)cz * cz);
  HIPCHK(hipMemcpyAsync(dZ.p, Z, sizeof(double) * nv * cz, hipMemcpyHostToDevice, c->st));
  block_qr_dev(c, dZ.p, cz, nv, cz, dQ.p, dR.p);
  HIPCHK(hipMemcpyAsync(R_out, dR.p, sizeof(double) * cz * cz, hipMemcpyDeviceToHost, c->st));
  if (Q_out) HIPCHK(hipMemcpyAsync(Q_out, dQ.p, sizeof(double) * nv * cz, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

// The Newton loop's update norm on device panels (diff_zzt_fnorm as ric_newtonadi_run calls it), for tests
int ricadi_diff_zzt_fnorm_dev(ricadi_ctx* c, const double* dZ1, int k1, const double* dZ0, int k0, double* upd_out,
                              double* x1_out) {
  REQUIRE(c && c->nv > 0, RICADI_ESTATE, "set the operator (or the dimensions) first");
  REQUIRE(k1 >= 1 && k0 >= 0, RICADI_EINVAL, "k1 >= 1 and k0 >= 0 required");
  REQUIRE(dZ1 && (dZ0 || k0 == 0), RICADI_EINVAL, "NULL panel");
  REQUIRE(k0 <= RICADI_MAX_UPD_COLS && k1 <= RICADI_MAX_UPD_COLS - k0, RICADI_EINVAL,
          "k1 + k0 <= RICADI_MAX_UPD_COLS (4096) required");
  API_BEGIN_ON(c)
  double x1 = 0.0;
  const double upd = diff_zzt_fnorm(c, dZ1, k1, k0 > 0 ? dZ0 : nullptr, k0, &x1);
  if (upd_out) *upd_out = upd;
  if (x1_out) *x1_out = x1;
  API_END
}

// H_A = Q^T (cal A - U V^T) Q, H_E = Q^T cal E Q on device panels; the low-rank term through the dense form of
// the same kernel (Q^T U, Q^T V), so H is bitwise reproducible with it as well
static void project_pencil_dev(ricadi_ctx* c, const double* dQ, int k, double* dHA, double* dHE) {
  const int nv = c->nv, q = c->q;
  size_t cnt = project_part_count(nv, k, k);
  if (q > 0) cnt = std::max(cnt, project_part_count(nv, k, q));
  TArr<double> part(c->pool, cnt);
  launch_project_pencil(c->st, nv, k, c->s_rp.p, c->s_ci.p, c->srcA.p, c->srcE.p, dQ, nullptr, nullptr, 0, part.p,
                        dHA, dHE);
  if (q > 0) {
    TArr<double> qu(c->pool, (size_t)k * q), qv(c->pool, (size_t)k * q);
    launch_project_pencil(c->st, nv, k, nullptr, nullptr, nullptr, nullptr, dQ, c->U.p, c->V.p, q, part.p, qu.p,
                          qv.p);
    launch_project_lowrank(c->st, k, q, qu.p, qv.p, dHA);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->st));
}

int ricadi_project_pencil_dev(ricadi_ctx* c, const double* dQ, int k, double* dHA, double* dHE) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(dQ && dHA && dHE && k >= 1 && k <= RICADI_MAX_M && k <= c->nv, RICADI_EINVAL, "bad argument");
  API_BEGIN_ON(c)
  project_pencil_dev(c, dQ, k, dHA, dHE);
  API_END
}

int ricadi_project_pencil(ricadi_ctx* c, const double* Q, int k, double* HA, double* HE) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(Q && HA && HE && k >= 1 && k <= RICADI_MAX_M && k <= c->nv, RICADI_EINVAL, "bad argument");
  API_BEGIN_ON(c)
  const size_t nq = (size_t)c->nv * k, nh = (size_t)k * k;
  TArr<double> dQ(c->pool, nq), dH(c->pool, 2 * nh);
  HIPCHK(hipMemcpyAsync(dQ.p, Q, sizeof(double) * nq, hipMemcpyHostToDevice, c->st));
  project_pencil_dev(c, dQ.p, k, dH.p, dH.p + nh);
  HIPCHK(hipMemcpyAsync(HA, dH.p, sizeof(double) * nh, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(HE, dH.p + nh, sizeof(double) * nh, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

// ---- balanced truncation from two factors ----
// G = X^T Y on device panels, fixed summation order
static void cross_gram_dev(ricadi_ctx* c, int n, int p, int q, const double* dX, int ldx, const double* dY, int ldy,
                           double* dG) {
  TArr<double> part(c->pool, cross_gram_partial_len(n, p, q));
  launch_cross_gram(c->st, n, p, q, dX, ldx, dY, ldy, part.p, dG);
  HIPCHK(hipGetLastError());
}

int ricadi_cross_gram_dev(ricadi_ctx* c, int n, int p, int q, const double* dX, int ldx, const double* dY, int ldy,
                          double* dG) {
  REQUIRE(c && dX && dY && dG, RICADI_EINVAL, "NULL argument");
  REQUIRE(n >= 1 && p >= 1 && p <= 1024 && q >= 1 && q <= 1024 && ldx >= p && ldy >= q, RICADI_EINVAL,
          "n >= 1, 1 <= p, q <= 1024, ldx >= p and ldy >= q required");
  API_BEGIN_ON(c)
  cross_gram_dev(c, n, p, q, dX, ldx, dY, ldy, dG);
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

// H_A = L^T (cal A - U V^T) Rb, H_E = L^T cal E Rb on device panels; the low-rank term through two cross-Gram matrices
static void project_pencil_twosided_dev(ricadi_ctx* c, const double* dL, const double* dRb, int r, double* dHA,
                                        double* dHE) {
  const int nv = c->nv, q = c->q;
  TArr<double> part(c->pool, project_part_count(nv, r, r));
  launch_project_pencil_twosided(c->st, nv, r, c->s_rp.p, c->s_ci.p, c->srcA.p, c->srcE.p, dL, dRb, part.p, dHA, dHE);
  if (q > 0) {
    TArr<double> lu(c->pool, (size_t)r * q), rv(c->pool, (size_t)r * q);
    cross_gram_dev(c, nv, r, q, dL, r, c->U.p, q, lu.p);
    cross_gram_dev(c, nv, r, q, dRb, r, c->V.p, q, rv.p);
    launch_project_lowrank(c->st, r, q, lu.p, rv.p, dHA);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->st));
}

int ricadi_project_pencil_twosided_dev(ricadi_ctx* c, const double* dL, const double* dRb, int r, double* dHA,
                                       double* dHE) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(dL && dRb && dHA && dHE && r >= 1 && r <= RICADI_MAX_M, RICADI_EINVAL, "bad argument (1 <= r <= 128)");
  REQUIRE(c->q <= 1024, RICADI_EINVAL, "the low-rank term of the context has more than 1024 columns");
  API_BEGIN_ON(c)
  project_pencil_twosided_dev(c, dL, dRb, r, dHA, dHE);
  API_END
}

int ricadi_lqg_balance_dev(ricadi_ctx* c, const double* dZc, int kc, const double* dZf, int kf, const double* dB, int nb,
                           const double* dCt, int nc, double tol, int order, int* r_out, double* sigma_out, double* dTl,
                           double* dTr, double* Ar_out, double* Er_out, double* Br_out, double* Cr_out) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(dZc && dZf && dB && dCt && r_out && sigma_out && dTl && dTr && Ar_out && Er_out && Br_out && Cr_out,
          RICADI_EINVAL, "NULL argument");
  REQUIRE(kc >= 1 && kc <= 1024 && kf >= 1 && kf <= 1024 && nb >= 1 && nb <= 1024 && nc >= 1 && nc <= 1024,
          RICADI_EINVAL, "1 <= kc, kf, nb, nc <= 1024 required");
  REQUIRE(tol >= 0.0 && tol < 1.0, RICADI_EINVAL, "0 <= tol < 1 required");
  REQUIRE(c->q <= 1024, RICADI_EINVAL, "the low-rank term of the context has more than 1024 columns");
  *r_out = 0;
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  const int nv = c->nv;
  const int rcap = std::min(std::min(kc, kf), std::min(order > 0 ? order : RICADI_MAX_M, std::min(RICADI_MAX_M, nv)));
  // S = Zc^T (cal E Zf): the product in panels of at most RICADI_MAX_M columns, then one cross-Gram matrix
  TArr<double> EZ(c->pool, (size_t)nv * kf), dS(c->pool, (size_t)kc * kf);
  for (int c0 = 0; c0 < kf; c0 += RICADI_MAX_M) {
    const int w = std::min(RICADI_MAX_M, kf - c0);
    launch_spmm(st, nv, c->E.rp.p, c->E.ci.p, c->E.v.p, dZf + c0, kf, nullptr, EZ.p + c0, kf, nullptr, 0, 1.0, 0.0,
                nullptr, w);
  }
  cross_gram_dev(c, nv, kc, kf, dZc, kc, EZ.p, kf, dS.p);
  std::vector<double> S((size_t)kc * kf), cl((size_t)kc * rcap), cr((size_t)kf * rcap);
  HIPCHK(hipMemcpyAsync(S.data(), dS.p, sizeof(double) * S.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  int r = 0;
  const int rc = lqg_balance(kc, kf, S.data(), tol, rcap, &r, sigma_out, cl.data(), cr.data());
  if (rc == RICADI_ENOCONV) throw ricadi::HipError{"ricadi_lqg_balance_dev: the Jacobi SVD of Zc^T cal E Zf did not converge"};
  if (rc != RICADI_OK) throw ricadi::HipError{"ricadi_lqg_balance_dev: Zc^T cal E Zf is zero or not finite"};
  *r_out = r;
  // T_l = Zc (U_r Sigma_r^-1/2), T_r = Zf (V_r Sigma_r^-1/2)
  TArr<double> dcl(c->pool, (size_t)kc * r), dcr(c->pool, (size_t)kf * r);
  HIPCHK(hipMemcpyAsync(dcl.p, cl.data(), sizeof(double) * kc * r, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dcr.p, cr.data(), sizeof(double) * kf * r, hipMemcpyHostToDevice, st));
  launch_gemm_nn(st, nv, kc, r, dZc, kc, dcl.p, r, dTl, r, 1.0, 0.0);
  launch_gemm_nn(st, nv, kf, r, dZf, kf, dcr.p, r, dTr, r, 1.0, 0.0);
  // the reduced model: [A_r | E_r | B_r | C_r^T]
  const size_t rr = (size_t)r * r;
  TArr<double> dH(c->pool, 2 * rr + (size_t)r * (nb + nc));
  project_pencil_twosided_dev(c, dTl, dTr, r, dH.p, dH.p + rr);
  cross_gram_dev(c, nv, r, nb, dTl, r, dB, nb, dH.p + 2 * rr);
  cross_gram_dev(c, nv, r, nc, dTr, r, dCt, nc, dH.p + 2 * rr + (size_t)r * nb);
  std::vector<double> crt((size_t)r * nc);
  HIPCHK(hipMemcpyAsync(Ar_out, dH.p, sizeof(double) * rr, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(Er_out, dH.p + rr, sizeof(double) * rr, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(Br_out, dH.p + 2 * rr, sizeof(double) * r * nb, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(crt.data(), dH.p + 2 * rr + (size_t)r * nb, sizeof(double) * r * nc, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < nc; ++i)
    for (int a = 0; a < r; ++a) Cr_out[(size_t)i * r + a] = crt[(size_t)a * nc + i];
  API_END
}

// What ricadi_lyap_adi and ricadi_lyap_adi_cplx share behind their argument checks: the factor reserved, W uploaded,
// `run(dW)` -- the driver, which returns its AdiStats --, the outputs.
static int lyap_adi_entry(ricadi_ctx* c, const double* W, int m, const ricadi_adi_params* prm, double* Z_out, int* c_out,
                          double* stats_out, const std::function<AdiStats(double*)>& run) {
  API_BEGIN_ON(c)
  ensure_work(c, m);
  const long esc0 = c->escalations;
  factor_reserve(c, prm->adi_max_steps * m);
  DArr<double> dW;
  dW.alloc((size_t)c->nv * m);
  HIPCHK(hipMemcpyAsync(dW.p, W, sizeof(double) * c->nv * m, hipMemcpyHostToDevice, c->st));
  if (c->sw.timing) c->t_setup = c->t_solve = c->t_recomb = c->t_compress = c->t_proj = c->t_cyc = c->t_iter = c->t_guess = 0;
  Tick tka;
  AdiStats s = run(dW.p);
  if (c->sw.timing) {
    (void)hipStreamSynchronize(c->st);
    fprintf(stderr, "[ricadi timing] lyap_adi: total %.1f ms = setup %.1f + projection %.1f + solves %.1f (Arnoldi iterations %.1f, "
            "restart-cycle bookkeeping %.1f, recycled guesses %.1f) + recombination %.1f + recompression %.1f (+ rest)\n",
            1e3 * tka.lap(), 1e3 * c->t_setup, 1e3 * c->t_proj, 1e3 * c->t_solve, 1e3 * c->t_iter, 1e3 * c->t_cyc,
            1e3 * c->t_guess, 1e3 * c->t_recomb, 1e3 * c->t_compress);
  }
  if (c_out) *c_out = c->zc;
  if (Z_out && c->zc > 0) factor_download(c, Z_out);
  if (stats_out) {
    stats_out[0] = s.steps;
    stats_out[1] = s.rel;
    stats_out[2] = (double)s.gmres_iters;
    stats_out[3] = (double)s.shift_solves;
    stats_out[4] = s.res_fro;
    stats_out[5] = (double)s.nonconverged;
    stats_out[6] = s.worst_relres;
    stats_out[7] = (double)(c->escalations - esc0);
  }
  API_END
}

int ricadi_lyap_adi(ricadi_ctx* c, const double* shifts, int ns, const double* W, int m,
                    const ricadi_adi_params* prm, double* Z_out, int* c_out, double* stats_out) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(shifts && ns > 0 && W && prm, RICADI_EINVAL, "bad argument");
  for (int i = 0; i < ns; ++i) REQUIRE(shifts[i] < 0.0, RICADI_EINVAL, "ADI shifts must be negative");
  REQUIRE(prm->adi_max_steps > 0, RICADI_EINVAL, "adi_max_steps must be positive");
  return lyap_adi_entry(c, W, m, prm, Z_out, c_out, stats_out,
                        [&](double* dW) { return lyap_adi_dev(c, shifts, ns, dW, m, *prm); });
}

int ricadi_adi_res_history(ricadi_ctx* c, double* out, int cap, int* n_out) {
  REQUIRE(c && n_out && cap >= 0 && (out || cap == 0), RICADI_EINVAL, "bad argument");
  REQUIRE(c->adi_ran, RICADI_ESTATE, "no ADI iteration has run on this context");
  const int n = (int)c->adi_res_hist.size();
  *n_out = n;
  for (int i = 0; i < std::min(n, cap); ++i) out[i] = c->adi_res_hist[i];
  return RICADI_OK;
}
int ricadi_set_adi_res_history(ricadi_ctx* c, int on) {
  REQUIRE(c, RICADI_EINVAL, "NULL context");
  c->adi_res_record = on != 0;
  return RICADI_OK;
}
int ricadi_adi_res_launches(ricadi_ctx* c, int64_t* n_out) {
  REQUIRE(c && n_out, RICADI_EINVAL, "NULL argument");
  *n_out = (int64_t)c->res_launches;
  return RICADI_OK;
}
int ricadi_adi_stop_rule(ricadi_ctx* c, int* rule_out) {
  REQUIRE(c && rule_out, RICADI_EINVAL, "NULL argument");
  REQUIRE(c->adi_ran, RICADI_ESTATE, "no ADI iteration has run on this context");
  *rule_out = c->adi_stop_rule;
  return RICADI_OK;
}

int ricadi_newton_history(ricadi_ctx* c, double* out, int cap, int* n_out) {
  REQUIRE(c && n_out && cap >= 0 && (out || cap == 0), RICADI_EINVAL, "bad argument");
  REQUIRE(c->newton_ran, RICADI_ESTATE, "no Newton iteration has run on this context");
  const int n = (int)(c->newton_hist.size() / 6);
  *n_out = n;
  for (int i = 0; i < 6 * std::min(n, cap); ++i) out[i] = c->newton_hist[i];
  return RICADI_OK;
}
int ricadi_newton_stop_rule(ricadi_ctx* c, int* rule_out) {
  REQUIRE(c && rule_out, RICADI_EINVAL, "NULL argument");
  REQUIRE(c->newton_ran, RICADI_ESTATE, "no Newton iteration has run on this context");
  *rule_out = c->newton_stop_rule;
  return RICADI_OK;
}

// the checks both Newton entries make before anything is launched
static int check_newton(const ricadi_ctx* c, const double* shifts, int ns, const void* B, int nb, const void* W, int mw,
                        const void* Z0, int c0, const ricadi_adi_params* prm) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(shifts && ns > 0 && B && W && prm, RICADI_EINVAL, "bad argument");
  REQUIRE(nb >= 1 && nb <= 64 && mw >= 1 && mw + nb <= RICADI_MAX_M, RICADI_EINVAL, "bad widths");
  REQUIRE(c0 == 0 || Z0, RICADI_EINVAL, "Z0 is NULL");
  // a loop that never runs would answer with the factor an earlier call left in the context
  REQUIRE(prm->nwtn_max_steps >= 1, RICADI_EINVAL, "nwtn_max_steps must be positive");
  REQUIRE(prm->adi_max_steps >= 1, RICADI_EINVAL, "adi_max_steps must be positive");
  for (int i = 0; i < ns; ++i) REQUIRE(shifts[i] < 0.0, RICADI_EINVAL, "ADI shifts must be negative");
  return RICADI_OK;
}

int ricadi_ric_newtonadi(ricadi_ctx* c, const double* shifts, int ns, const double* B, int nb,
                         const double* W, int mw, const double* Z0, int c0, const double* oldB,
                         const ricadi_adi_params* prm, double* Z_out, int zcap, int* c_out,
                         double* stats_out) {
  if (int rc = check_newton(c, shifts, ns, B, nb, W, mw, Z0, c0, prm)) return rc;
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  const int nv = c->nv;
  TArr<double> dB(c->pool, (size_t)nv * nb), dWm(c->pool, (size_t)nv * mw), dOld(c->pool), dZ0(c->pool);
  HIPCHK(hipMemcpyAsync(dB.p, B, sizeof(double) * nv * nb, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dWm.p, W, sizeof(double) * nv * mw, hipMemcpyHostToDevice, st));
  if (oldB) {
    dOld.alloc((size_t)nv * nb);
    HIPCHK(hipMemcpyAsync(dOld.p, oldB, sizeof(double) * nv * nb, hipMemcpyHostToDevice, st));
  }
  if (c0 > 0) {
    dZ0.alloc((size_t)nv * c0);
    HIPCHK(hipMemcpyAsync(dZ0.p, Z0, sizeof(double) * nv * c0, hipMemcpyHostToDevice, st));
  }
  ric_newtonadi_run(c, shifts, ns, dB.p, nb, dWm.p, mw, dZ0.p, c0, oldB ? dOld.p : nullptr, prm, stats_out);
  if (c_out) *c_out = c->zc;
  if (Z_out && c->zc > 0) {
    if (c->zc > zcap) throw ricadi::HipError{"Z_out capacity too small"};
    factor_download(c, Z_out);
  }
  API_END
}

// The same with every panel ALREADY ON THE DEVICE (no PCIe traffic inside the call): dB, dW, dZ0, dOldB are device
// pointers (row-major, leading dimension = width; dZ0 / dOldB may be NULL with c0 = 0).  The new iterate stays in
// the context's factor: ricadi_factor_cols, ricadi_factor_get (host) / ricadi_factor_get_dev (device).
int ricadi_ric_newtonadi_dev(ricadi_ctx* c, const double* shifts, int ns, const double* dB, int nb,
                             const double* dW, int mw, const double* dZ0, int c0, const double* dOldB,
                             const ricadi_adi_params* prm, int* c_out, double* stats_out) {
  if (int rc = check_newton(c, shifts, ns, dB, nb, dW, mw, dZ0, c0, prm)) return rc;
  API_BEGIN_ON(c)
  ric_newtonadi_run(c, shifts, ns, dB, nb, dW, mw, dZ0, c0, dOldB, prm, stats_out);
  if (c_out) *c_out = c->zc;
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

// ---- RADI (solver_radi.inl) ----
// the checks both entries make before anything is launched
static int check_radi(const ricadi_ctx* c, const double* shifts, int ns, const void* B, int nb, const void* W, int mw,
                      int max_steps) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(ns >= 1 && shifts && B && W, RICADI_EINVAL, "bad argument");
  REQUIRE(nb >= 1 && nb <= 64 && mw >= 1 && mw + nb <= RICADI_MAX_M, RICADI_EINVAL, "bad widths");
  REQUIRE(max_steps >= 1, RICADI_EINVAL, "max_steps must be positive");
  for (int i = 0; i < ns; ++i) REQUIRE(shifts[i] < 0.0, RICADI_EINVAL, "RADI shifts must be negative");
  REQUIRE(!sharded(c), RICADI_ESTATE, "ricadi_ric_radi does not shard: clear the exchange of this context first");
  REQUIRE(c->radi_shift_mode != RICADI_RADI_SHIFTS_HAMILTONIAN || mw <= 32, RICADI_EINVAL,
          "RICADI_RADI_SHIFTS_HAMILTONIAN needs mw <= 32");
  // (RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT: mw <= 127 and nb <= 64, which every mode needs and the lines above check)
  REQUIRE(c->radi_sweep_shifts || c->radi_sweep_width == 1 || c->radi_shift_mode == RICADI_RADI_SHIFTS_CYCLE, RICADI_EINVAL,
          "a RADI sweep width above 1 needs RICADI_RADI_SHIFTS_CYCLE: generated shifts are one at a time");
  REQUIRE(!c->radi_sweep_shifts || c->radi_shift_mode == RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT, RICADI_EINVAL,
          "ricadi_set_radi_sweep_shifts needs RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT");
  return RICADI_OK;
}
static void radi_stats_out(const RadiStats& s, double* stats_out) {
  if (!stats_out) return;
  stats_out[0] = s.steps;
  stats_out[1] = s.res;
  stats_out[2] = s.rhs;
  stats_out[3] = (double)s.gmres_iters;
  stats_out[4] = (double)s.shift_solves;
  stats_out[5] = (double)s.nonconverged;
  stats_out[6] = s.worst_relres;
  stats_out[7] = (double)s.escalations;
}
#define RADI_BREAKDOWN_MSG "RADI: I + G G^T has a pivot that is not positive and finite (NaN / Inf in a shift solve)"

int ricadi_ric_radi(ricadi_ctx* c, const double* shifts, int ns, const double* B, int nb, const double* W, int mw,
                    const double* oldB, int max_steps, double res_reltol, int compress_cols, int project_w,
                    int verbose, double* Z_out, int zcap, int* c_out, double* K_out, double* stats_out) {
  if (int rc = check_radi(c, shifts, ns, B, nb, W, mw, max_steps)) return rc;
  REQUIRE(!Z_out || (long)zcap >= (long)max_steps * mw, RICADI_EINVAL, "Z_out capacity below max_steps * mw");
  bool breakdown = false;
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  const int nv = c->nv;
  TArr<double> dB(c->pool, (size_t)nv * nb), dWm(c->pool, (size_t)nv * mw), dOld(c->pool), dK(c->pool);
  HIPCHK(hipMemcpyAsync(dB.p, B, sizeof(double) * nv * nb, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dWm.p, W, sizeof(double) * nv * mw, hipMemcpyHostToDevice, st));
  if (oldB) {
    dOld.alloc((size_t)nv * nb);
    HIPCHK(hipMemcpyAsync(dOld.p, oldB, sizeof(double) * nv * nb, hipMemcpyHostToDevice, st));
  }
  if (K_out) dK.alloc((size_t)nv * nb);
  const RadiStats s = ric_radi_run(c, shifts, ns, dB.p, nb, dWm.p, mw, oldB ? dOld.p : nullptr, max_steps, res_reltol,
                                   compress_cols, project_w != 0, verbose != 0, dK.p);
  radi_stats_out(s, stats_out);
  breakdown = s.breakdown;
  if (c_out) *c_out = c->zc;
  if (!breakdown) {
    if (K_out) HIPCHK(hipMemcpyAsync(K_out, dK.p, sizeof(double) * nv * nb, hipMemcpyDeviceToHost, st));
    if (Z_out && c->zc > 0) factor_download(c, Z_out);
    HIPCHK(hipStreamSynchronize(st));
  }
  API_END_STATUS(breakdown ? (ricadi::set_error(RADI_BREAKDOWN_MSG), RICADI_EBREAKDOWN) : RICADI_OK)
}

int ricadi_ric_radi_dev(ricadi_ctx* c, const double* shifts, int ns, const double* dB, int nb, const double* dW, int mw,
                        const double* dOldB, int max_steps, double res_reltol, int compress_cols, int project_w,
                        int verbose, int* c_out, double* dK_out, double* stats_out) {
  if (int rc = check_radi(c, shifts, ns, dB, nb, dW, mw, max_steps)) return rc;
  bool breakdown = false;
  API_BEGIN_ON(c)
  const RadiStats s = ric_radi_run(c, shifts, ns, dB, nb, dW, mw, dOldB, max_steps, res_reltol, compress_cols,
                                   project_w != 0, verbose != 0, dK_out);
  radi_stats_out(s, stats_out);
  breakdown = s.breakdown;
  if (c_out) *c_out = c->zc;
  API_END_STATUS(breakdown ? (ricadi::set_error(RADI_BREAKDOWN_MSG), RICADI_EBREAKDOWN) : RICADI_OK)
}

int ricadi_set_radi_shifts(ricadi_ctx* c, int mode) {
  REQUIRE(c && (mode == RICADI_RADI_SHIFTS_CYCLE || mode == RICADI_RADI_SHIFTS_HAMILTONIAN), RICADI_EINVAL,
          "mode must be RICADI_RADI_SHIFTS_CYCLE or RICADI_RADI_SHIFTS_HAMILTONIAN");
  c->radi_shift_mode = mode;
  return RICADI_OK;
}
// the same setting with the modes added since ABI 410; ricadi_set_radi_shifts keeps the two modes and the refusals
// it had
int ricadi_set_radi_shift_mode(ricadi_ctx* c, int mode) {
  REQUIRE(c && (mode == RICADI_RADI_SHIFTS_CYCLE || mode == RICADI_RADI_SHIFTS_HAMILTONIAN ||
                mode == RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT),
          RICADI_EINVAL,
          "mode must be RICADI_RADI_SHIFTS_CYCLE, RICADI_RADI_SHIFTS_HAMILTONIAN or "
          "RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT");
  c->radi_shift_mode = mode;
  return RICADI_OK;
}
int ricadi_set_radi_sweep_width(ricadi_ctx* c, int width) {
  REQUIRE(c && width >= 1 && width <= RICADI_MAX_GROUPS, RICADI_EINVAL, "1 <= width <= 16 required");
  c->radi_sweep_width = width;
  return RICADI_OK;
}
// sweeps whose shifts the iteration generates (solver_radi.inl): returns the previous value
int ricadi_set_radi_sweep_shifts(ricadi_ctx* c, int on) {
  REQUIRE(c && (on == 0 || on == 1), RICADI_EINVAL, "on must be 0 or 1");
  const int before = c->radi_sweep_shifts;
  c->radi_sweep_shifts = on;
  return before;
}
int ricadi_radi_sweep_widths(ricadi_ctx* c, int* out, int cap, int* n_out) {
  REQUIRE(c && n_out && cap >= 0 && (out || cap == 0), RICADI_EINVAL, "bad argument");
  REQUIRE(c->radi_ran, RICADI_ESTATE, "no RADI iteration has run on this context");
  const int n = (int)c->radi_sweep_widths.size();
  *n_out = n;
  for (int i = 0; i < std::min(n, cap); ++i) out[i] = c->radi_sweep_widths[i];
  return RICADI_OK;
}
int ricadi_radi_sweep_info(ricadi_ctx* c, int* out) {
  REQUIRE(c && out, RICADI_EINVAL, "NULL argument");
  REQUIRE(c->radi_ran, RICADI_ESTATE, "no RADI iteration has run on this context");
  for (int i = 0; i < 3; ++i) out[i] = c->radi_sweep_info[i];
  return RICADI_OK;
}
int ricadi_radi_shift_history(ricadi_ctx* c, double* out, int cap, int* n_out) {
  REQUIRE(c && n_out && cap >= 0 && (out || cap == 0), RICADI_EINVAL, "bad argument");
  REQUIRE(c->radi_ran, RICADI_ESTATE, "no RADI iteration has run on this context");
  const int n = (int)c->radi_shift_hist.size();
  *n_out = n;
  for (int i = 0; i < std::min(n, cap); ++i) out[i] = c->radi_shift_hist[i];
  return RICADI_OK;
}
int ricadi_radi_shift_fallbacks(ricadi_ctx* c, int* n_out) {
  REQUIRE(c && n_out, RICADI_EINVAL, "NULL argument");
  REQUIRE(c->radi_ran, RICADI_ESTATE, "no RADI iteration has run on this context");
  *n_out = c->radi_fallbacks;
  return RICADI_OK;
}

// Copy of the device-resident factor into a DEVICE buffer (nv x cz row-major, ld cz; cz = ricadi_factor_cols)
int ricadi_factor_get_dev(ricadi_ctx* c, double* dZ_out, int cz) {
  REQUIRE(c && dZ_out, RICADI_EINVAL, "NULL argument");
  REQUIRE(cz == c->zc && cz > 0, RICADI_EINVAL, "column count differs from the resident factor");
  API_BEGIN_ON(c)
  launch_copy_cols(c->st, c->nv, cz, c->Z.p, c->zld, 0, dZ_out, cz, 0, 1.0);
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

int ricadi_compress(ricadi_ctx* c, const double* Z, int cz, double thresh, int kmax, double* Zc_out,
                    int* k_out, double* sv_out) {
  REQUIRE(c && c->nv > 0, RICADI_ESTATE, "set the operator (or the dimensions) first");
  REQUIRE(Zc_out && k_out, RICADI_EINVAL, "NULL output");
  if (int rc = check_factor(c, Z, cz)) return rc;
  API_BEGIN_ON(c)
  const FactorArg z(c, Z, cz);
  cz = z.cz;
  DArr<double> out;
  out.alloc((size_t)c->nv * cz);
  std::vector<double> sv;
  // the reference's route -- thin QR, then SVD of R ("QR ... SVD", optcont_main.py:133-134) -- up to 1024 columns
  // (the factors the Newton iteration returns are recompressed to a few hundred); raw factors beyond that take the
  // Gram route (singular values resolved to sqrt(eps) sigma_1 instead of eps sigma_1): an O(n c^2) block QR with
  // re-orthogonalisation of thousands of columns costs seconds
  const bool qr_route = c->opts.compress_qr != 0 && cz <= 1024;
  int k = compress_dev(c, z.p, cz, z.ld, thresh, kmax, false, out.p, &sv, qr_route);
  *k_out = k;
  if (k > 0) {
    HIPCHK(hipMemcpyAsync(Zc_out, out.p, sizeof(double) * c->nv * k, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  }
  if (sv_out) std::memcpy(sv_out, sv.data(), sizeof(double) * std::min<size_t>(sv.size(), (size_t)std::min(cz, c->nv)));
  API_END
}

int ricadi_recompress(ricadi_ctx* c, const double* Z, int cz, double rel, double* Zc_out, int* k_out) {
  REQUIRE(c && c->nv > 0, RICADI_ESTATE, "set the operator (or the dimensions) first");
  REQUIRE(Z && Zc_out && k_out && cz > 0, RICADI_EINVAL, "NULL argument or bad column count");
  API_BEGIN_ON(c)
  DArr<double> tmp, out;
  tmp.alloc((size_t)c->nv * cz);
  out.alloc((size_t)c->nv * cz);
  HIPCHK(hipMemcpyAsync(tmp.p, Z, sizeof(double) * c->nv * cz, hipMemcpyHostToDevice, c->st));
  const int k = recompress_exec(c, main_exec(c), tmp.p, cz, cz, rel > 0.0 ? rel : kInternalRelThresh, out.p);
  *k_out = k;
  if (k > 0) {
    HIPCHK(hipMemcpyAsync(Zc_out, out.p, sizeof(double) * c->nv * k, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  }
  API_END
}

int ricadi_gain(ricadi_ctx* c, const int32_t* mt_rp, const int32_t* mt_ci, const double* mt_v,
                const double* Z, int cz, const double* B, int nb, double* K_out) {
  REQUIRE(c && c->nv > 0, RICADI_ESTATE, "set the operator (or the dimensions) first");
  REQUIRE(mt_rp || c->has_op, RICADI_ESTATE, "no cal E in the context: pass mt_* explicitly");
  REQUIRE(B && K_out && nb >= 1 && nb <= RICADI_MAX_M, RICADI_EINVAL, "bad argument");
  if (int rc = check_factor(c, Z, cz)) return rc;
  API_BEGIN_ON(c)
  const int nv = c->nv;
  const FactorArg z(c, Z, cz);
  DArr<double> dB, dK;
  dB.alloc((size_t)nv * nb);
  dK.alloc((size_t)nv * nb);
  HIPCHK(hipMemcpyAsync(dB.p, B, sizeof(double) * nv * nb, hipMemcpyHostToDevice, c->st));
  if (mt_rp) {
    HostCsr Mt = make_csr(nv, nv, mt_rp, mt_ci, mt_v);
    DevCsr dMt;
    dMt.upload(Mt, c->st);
    gain_dev(c, dMt, z.p, z.cz, z.ld, dB.p, nb, dK.p);
  } else {
    gain_dev(c, c->E, z.p, z.cz, z.ld, dB.p, nb, dK.p);
  }
  HIPCHK(hipMemcpyAsync(K_out, dK.p, sizeof(double) * nv * nb, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

int ricadi_lyap_res_norm(ricadi_ctx* c, const double* Z, int cz, const double* W, int m,
                         double* res2_out) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(Z && W && res2_out && cz > 0 && m > 0, RICADI_EINVAL, "bad argument");
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  const int nv = c->nv, wtot = 2 * cz + m;
  DArr<double> dZ, S, chunk, G;
  dZ.alloc((size_t)nv * cz);
  S.alloc((size_t)nv * wtot);       // [cal A_eff Z, cal E Z, W], ld = wtot
  HIPCHK(hipMemcpyAsync(dZ.p, Z, sizeof(double) * nv * cz, hipMemcpyHostToDevice, st));
  {
    DArr<double> dWh;
    dWh.alloc((size_t)nv * m);
    HIPCHK(hipMemcpyAsync(dWh.p, W, sizeof(double) * nv * m, hipMemcpyHostToDevice, st));
    launch_copy_cols(st, nv, m, dWh.p, m, 0, S.p, wtot, 2 * cz, 1.0);
    HIPCHK(hipStreamSynchronize(st));
  }
  // cal A Z and cal E Z in column chunks of <= 64
  const int CH = 64;
  chunk.alloc((size_t)c->n * CH * 2);
  double* in = chunk.p;
  double* out = chunk.p + (size_t)c->n * CH;
  for (int c0 = 0; c0 < cz; c0 += CH) {
    const int w = std::min(CH, cz - c0);
    launch_copy_cols(st, nv, w, dZ.p, cz, c0, in, w, 0, 1.0);
    launch_spmm(st, nv, c->A.rp.p, c->A.ci.p, c->A.v.p, in, w, nullptr, out, w, nullptr, 0, 1.0, 0.0, nullptr, w);
    if (c->q > 0) {
      c->scratch.ensure((size_t)c->q * w + 64);
      HIPCHK(hipMemsetAsync(c->scratch.p, 0, sizeof(double) * c->q * w, st));
      launch_gemm_tn(st, nv, c->q, w, c->V.p, c->q, in, w, c->scratch.p, w);
      launch_gemm_nn(st, nv, c->q, w, c->U.p, c->q, c->scratch.p, w, out, w, -1.0, 1.0);
    }
    launch_copy_cols(st, nv, w, out, w, 0, S.p, wtot, c0, 1.0);
    launch_spmm(st, nv, c->E.rp.p, c->E.ci.p, c->E.v.p, in, w, nullptr, out, w, nullptr, 0, 1.0, 0.0, nullptr, w);
    launch_copy_cols(st, nv, w, out, w, 0, S.p, wtot, cz + c0, 1.0);
  }
  // project every column: P^T s
  Restore<int> keep_q(c->q);
  for (int c0 = 0; c0 < wtot; c0 += CH) {
    const int w = std::min(CH, wtot - c0);
    launch_copy_cols(st, nv, w, S.p, wtot, c0, in, w, 0, 1.0);
    project_panel(c, in, w);
    launch_copy_cols(st, nv, w, in, w, 0, S.p, wtot, c0, 1.0);
  }
  G.alloc((size_t)wtot * wtot);
  HIPCHK(hipMemsetAsync(G.p, 0, sizeof(double) * wtot * wtot, st));
  launch_gemm_tn(st, nv, wtot, wtot, S.p, wtot, S.p, wtot, G.p, wtot);
  std::vector<double> Gh((size_t)wtot * wtot);
  HIPCHK(hipMemcpyAsync(Gh.data(), G.p, sizeof(double) * wtot * wtot, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  // residual = U S U^T with U = [G, H, Wp], S swaps the first two blocks;
  // ||.||_F^2 = trace(S Gram S Gram)
  auto perm = [&](int i) { return i < cz ? i + cz : (i < 2 * cz ? i - cz : i); };
  double tr = 0.0;
  for (int i = 0; i < wtot; ++i)
    for (int j = 0; j < wtot; ++j)
      tr += Gh[(size_t)perm(i) * wtot + j] * Gh[(size_t)perm(j) * wtot + i];
  *res2_out = tr;
  API_END
}

int ricadi_factor_cols(ricadi_ctx* c, int* c_out) {
  REQUIRE(c && c_out, RICADI_EINVAL, "NULL argument");
  *c_out = c->zc;
  return RICADI_OK;
}

int ricadi_factor_get(ricadi_ctx* c, double* Z_out, int cz) {
  REQUIRE(c && Z_out, RICADI_EINVAL, "NULL argument");
  REQUIRE(cz == c->zc && cz > 0, RICADI_EINVAL, "column count does not match the device factor");
  API_BEGIN_ON(c)
  factor_download(c, Z_out);
  API_END
}

int ricadi_factor_set(ricadi_ctx* c, const double* Z, int cz) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(Z && cz > 0, RICADI_EINVAL, "bad argument");
  API_BEGIN_ON(c)
  factor_reserve(c, cz);
  HIPCHK(hipMemcpyAsync(c->Z.p, Z, sizeof(double) * c->nv * cz, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  c->zc = cz;
  API_END
}

}  // extern "C"
