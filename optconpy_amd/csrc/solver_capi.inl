// solver_capi.inl -- the C-ABI of include/ricadi.h.
// Part of ricadi_solver.hip (one translation unit; included there in order).

// =====================================================================================
//                                      C  A B I
// =====================================================================================
#define API_BEGIN try {
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

// Milliseconds per call of fn() over reps calls on stream st, timed with HIP events (destroyed on every path)
template <class Fn>
static double timed_ms(hipStream_t st, int reps, Fn&& fn) {
  struct Events {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events() {
      for (hipEvent_t x : e)
        if (x) (void)hipEventDestroy(x);
    }
  } ev;
  HIPCHK(hipEventCreate(&ev.e[0]));
  HIPCHK(hipEventCreate(&ev.e[1]));
  HIPCHK(hipEventRecord(ev.e[0], st));
  for (int i = 0; i < reps; ++i) fn();
  HIPCHK(hipEventRecord(ev.e[1], st));
  HIPCHK(hipEventSynchronize(ev.e[1]));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
  return (double)ms / reps;
}

// The first level from c downwards for which is(level) holds (NULL: none); lb, the batch of c on entry, becomes the
// batch of that level with the same group table.
template <class Pred>
static ricadi_ctx* walk_levels(ricadi_ctx* c, Batch& lb, Pred&& is) {
  const GroupTab tab = lb.tab;
  ricadi_ctx* lc = c;
  for (; lc && !is(lc); lc = lc->child.get()) {
    if (!lc->child) continue;
    Batch t = *lb.sub;
    t.tab = tab;
    lb = t;
  }
  return lc;
}

extern "C" {

const char* ricadi_last_error(void) { return ricadi::g_err.c_str(); }
int ricadi_version(void) { return 406; }
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
  API_BEGIN
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
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
  API_BEGIN
  HIPCHK(hipSetDevice(c->dev));
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
  HostSetup hs;
  build_setup_checked(A, E, J, c->opts, hs, c->levels, sa_omega);
  const HostCsr JT = transpose(J);
  const PrecondRecords pr = build_records(hs, J, JT, c->sw.sweep_meta, c->sw.ms_spmm);
  // the child level (same stream and rocBLAS handle) takes the coarse problem
  c->cache.clear();
  c->child.reset();
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
  c->q = 0;
  c->wcols = 0;  // workspaces depend on n
  c->zc = 0;
  c->has_op = true;
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
  API_END
}

int ricadi_clear_cache(ricadi_ctx* c) {
  REQUIRE(c, RICADI_EINVAL, "NULL ctx");
  API_BEGIN
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
  API_BEGIN
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
  API_BEGIN
  HIPCHK(hipSetDevice(c->dev));
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
  c->cache.clear();
  for (auto& e : c->rec_ring) e->serial = -1;
  c->has_op = false;
  c->nv = nv;
  c->np = 0;
  c->n = nv;
  c->q = 0;
  c->zc = 0;
  c->wcols = 0;
  return RICADI_OK;
}

int ricadi_set_lowrank(ricadi_ctx* c, const double* U, const double* V, int q) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(q >= 0 && q <= 64, RICADI_EINVAL, "low-rank width must be in [0, 64]");
  REQUIRE(q == 0 || (U && V), RICADI_EINVAL, "NULL low-rank factor");
  API_BEGIN
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

static int check_panel(ricadi_ctx* c, int m) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  (void)hipSetDevice(c->dev);   // host worker threads start on device 0
  REQUIRE(m >= 1 && m <= RICADI_MAX_M, RICADI_EINVAL, "panel width must be in [1, 128]");
  return RICADI_OK;
}

int ricadi_spmm_dev(ricadi_ctx* c, double alpha, double beta, const double* dX, int m, double* dY) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(dX && dY, RICADI_EINVAL, "NULL panel");
  API_BEGIN
  ShiftData* sd = get_shift(c, alpha, beta);
  ensure_work(c, m);
  op_apply(c, sd, dX, dY, m, true);
  API_END
}

int ricadi_spmm(ricadi_ctx* c, double alpha, double beta, const double* X, int m, double* Y) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(X && Y, RICADI_EINVAL, "NULL panel");
  API_BEGIN
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
  API_BEGIN
  const size_t nm = (size_t)c->n * m;
  ShiftData* sd = get_shift(c, alpha, beta);
  ensure_work(c, m);
  HIPCHK(hipMemcpyAsync(c->pw1.p, R, nm * sizeof(double), hipMemcpyHostToDevice, c->st));
  precond_apply(c, sd, c->pw1.p, c->pw2.p, m);
  HIPCHK(hipMemcpyAsync(Z, c->pw2.p, nm * sizeof(double), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

// The group ids of active[0 .. nactive) into ids, validated (active == NULL: all groups, ids stays empty)
static int active_ids(const int32_t* active, int nactive, int ng, std::vector<int>& ids) {
  if (!active) return RICADI_OK;
  for (int i = 0; i < nactive; ++i) {
    REQUIRE(active[i] >= 0 && active[i] < ng && std::find(ids.begin(), ids.end(), active[i]) == ids.end(),
            RICADI_EINVAL, "active: distinct group ids in [0, ng) required");
    ids.push_back(active[i]);
  }
  REQUIRE(!ids.empty(), RICADI_EINVAL, "no active group");
  return RICADI_OK;
}

int ricadi_precond_apply_batch_dev(ricadi_ctx* c, int ng, const double* alphas, const double* betas,
                                   const double* dR, int64_t r_stride, int m, const int32_t* active, int nactive,
                                   double* dZ, int* form_out) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(dR && dZ && alphas && betas, RICADI_EINVAL, "NULL argument");
  REQUIRE(ng >= 1 && ng <= RICADI_MAX_GROUPS && (size_t)ng * m <= 2048, RICADI_EINVAL,
          "1 <= ng <= 16 and ng*m <= 2048 required");
  REQUIRE(r_stride >= (int64_t)c->n * m, RICADI_EINVAL, "bad r_stride");
  std::vector<int> ids;
  if (int rc = active_ids(active, nactive, ng, ids)) return rc;
  API_BEGIN
  hipStream_t st = c->st;
  std::vector<ShiftData*> sds(ng);
  get_shifts(c, alphas, betas, ng, sds.data());
  ensure_work(c, m, ng, 0);
  Batch bt = make_batch(c, sds.data(), ng, m);
  if (active) bt.set(ids);
  else bt.all();
  const size_t nm = bt.gs, vs = nm * ng;
  // the form gmres_core applies the preconditioner in (same question, same answer)
  const IterationForm f = iteration_form(c, m, ng, false);
  // input: the FP64 panel, or the FP16-stored Krylov vector (basis slot 0, rounded by the kernel that stores the
  // basis) beside an FP64 panel of NaN -- the iteration does not write that copy then
  const double* r = dR;
  size_t gsr = (size_t)r_stride;
  _Float16* r16 = nullptr;
  std::vector<double> ones((size_t)ng * m, 1.0);
  if (f.h16) {
    r16 = reinterpret_cast<_Float16*>(c->basisf.p);
    HIPCHK(hipMemcpyAsync(c->scale.p, ones.data(), sizeof(double) * ones.size(), hipMemcpyHostToDevice, st));
    launch_colscale_b(st, bt.tab, c->n, m, c->scale.p, dR, gsr, 0.0, c->pw2.p, nm, r16, nm);
    HIPCHK(hipMemsetAsync(c->pw1.p, 0xFF, sizeof(double) * vs, st));
    r = c->pw1.p;
    gsr = nm;
  }
  // output: z straight into dZ, or -- where the operator reads the FP32-stored Z_j -- that panel (slot 0 of the
  // Z_j store) with the FP64 panel it must not need filled with NaN
  float* z32 = c->zbasisf.p;
  double* z = dZ;
  if (f.x32) {
    HIPCHK(hipMemsetAsync(c->zv.p, 0xFF, sizeof(double) * vs, st));
    HIPCHK(hipMemsetAsync(z32, 0xFF, sizeof(float) * vs, st));
    z = c->zv.p;
  }
  const CycleForm pf = cycle_form(c, m, bt.blocks16, gsr, f.x32, f.h16);
  precond_apply(c, bt, pf, CycleIO{r, gsr, r16, z, z32, nm});
  if (f.x32) {
    std::vector<float> h32(nm);
    std::vector<double> h64(nm);
    for (int i = 0; i < bt.tab.ng; ++i) {
      const size_t g = (size_t)bt.tab.gid[i];
      HIPCHK(hipMemcpyAsync(h32.data(), z32 + g * nm, sizeof(float) * nm, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      for (size_t k = 0; k < nm; ++k) h64[k] = h32[k];
      HIPCHK(hipMemcpyAsync(dZ + g * nm, h64.data(), sizeof(double) * nm, hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
    }
  }
  HIPCHK(hipStreamSynchronize(st));
  if (form_out) *form_out = (int)pf.word();
  API_END
}

int ricadi_op_apply_batch_dev(ricadi_ctx* c, int ng, const double* alphas, const double* betas, const double* dX,
                              int64_t x_stride, int m, const int32_t* active, int nactive, int flags, double alpha,
                              const double* dR, int64_t r_stride, double beta_r, double* dY, int64_t y_stride,
                              int* variant_out) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(dX && dY && alphas && betas, RICADI_EINVAL, "NULL argument");
  REQUIRE(ng >= 1 && ng <= RICADI_MAX_GROUPS && (size_t)ng * m <= 2048, RICADI_EINVAL,
          "1 <= ng <= 16 and ng*m <= 2048 required");
  REQUIRE((flags & ~(RICADI_OA_X32 | RICADI_OA_Y32 | RICADI_OA_LOWRANK | RICADI_OA_RESIDUAL)) == 0, RICADI_EINVAL,
          "unknown flag");
  const int64_t nm = (int64_t)c->n * m;
  REQUIRE(x_stride >= nm && y_stride >= nm, RICADI_EINVAL, "bad x_stride / y_stride");
  const bool res = flags & RICADI_OA_RESIDUAL, x32 = flags & RICADI_OA_X32, y32 = flags & RICADI_OA_Y32;
  const bool lowrank = (flags & RICADI_OA_LOWRANK) && c->q > 0;
  REQUIRE(!res || (dR && r_stride >= nm), RICADI_EINVAL, "residual form: r and r_stride >= n*m required");
  // the FP32 operand forms exist in the tile kernels' plain product only (saddle_spmm)
  REQUIRE(!x32 || (saddle_tiled(c, m) && !res && !lowrank), RICADI_EINVAL,
          "FP32 input: only the plain product where the tiles fit");
  REQUIRE(!y32 || x32, RICADI_EINVAL, "FP32 output: with the FP32 input only");
  std::vector<int> ids;
  if (int rc = active_ids(active, nactive, ng, ids)) return rc;
  API_BEGIN
  hipStream_t st = c->st;
  std::vector<ShiftData*> sds(ng);
  get_shifts(c, alphas, betas, ng, sds.data());
  ensure_work(c, m, ng, 0);
  Batch bt = make_batch(c, sds.data(), ng, m);
  if (active) bt.set(ids);
  else bt.all();
  // FP32 copies of x / y with the caller's group strides (as the iteration stores Z_j and w)
  DArr<float> xf, yf;
  if (x32) {
    xf.alloc((size_t)x_stride * ng);
    for (int i = 0; i < bt.tab.ng; ++i) {
      const size_t g = (size_t)bt.tab.gid[i];
      launch_to_f32(st, c->n, m, dX + g * x_stride, m, xf.p + g * x_stride, m);
    }
  }
  if (y32) yf.alloc((size_t)y_stride * ng);
  const LowRankArgs lr = lowrank ? lowrank_args(c, bt, dX, (size_t)x_stride) : LowRankArgs();
  saddle_spmm(c, bt, dX, (size_t)x_stride, nullptr, dY, (size_t)y_stride, res ? dR : nullptr,
              res ? (size_t)r_stride : 0, alpha, res ? beta_r : 0.0, lr, xf.p, yf.p);
  if (y32) {
    std::vector<float> h32((size_t)nm);
    std::vector<double> h64((size_t)nm);
    for (int i = 0; i < bt.tab.ng; ++i) {
      const size_t g = (size_t)bt.tab.gid[i];
      HIPCHK(hipMemcpyAsync(h32.data(), yf.p + g * y_stride, sizeof(float) * nm, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      for (int64_t k = 0; k < nm; ++k) h64[k] = h32[k];
      HIPCHK(hipMemcpyAsync(dY + g * y_stride, h64.data(), sizeof(double) * nm, hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
    }
  }
  HIPCHK(hipStreamSynchronize(st));
  if (variant_out) *variant_out = c->k1_variant;
  API_END
}

int ricadi_precond_structure(ricadi_ctx* c, int level, int32_t* sizes_out, int32_t* bv_ptr, int32_t* bv_rows,
                             int32_t* bp_ptr, int32_t* bp_rows, int32_t* aggof, int32_t* p_rp, int32_t* p_ci,
                             double* p_v) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(sizes_out && level >= 0, RICADI_EINVAL, "bad argument");
  const ricadi_ctx* l = c;
  for (int i = 0; i < level && l; ++i) l = l->child.get();
  REQUIRE(l, RICADI_EINVAL, "no such level");
  API_BEGIN
  (void)hipSetDevice(c->dev);
  hipStream_t st = c->st;
  const int n = l->n, kc = l->kc;
  auto down = [&](auto* dst, const auto& src, size_t cnt) {
    if (dst && cnt) HIPCHK(hipMemcpyAsync(dst, src.p, sizeof(*dst) * cnt, hipMemcpyDeviceToHost, st));
  };
  // dof -> coarse index (velocity aggregates first), and P^T by rows where the prolongation is smoothed
  std::vector<int32_t> agg(kc > 0 ? n : 0), ptrp, ptci;
  std::vector<double> ptv;
  down(agg.data(), l->aggof, agg.size());
  if (l->sa) {
    ptrp.resize(kc + 1);
    ptci.resize(l->pt_ci.n);
    ptv.resize(l->pt_v.n);
    down(ptrp.data(), l->pt_rp, ptrp.size());
    down(ptci.data(), l->pt_ci, ptci.size());
    down(ptv.data(), l->pt_v, ptv.size());
  }
  HIPCHK(hipStreamSynchronize(st));
  int kcv = 0;
  for (int i = 0; i < l->nv && kc > 0; ++i) kcv = std::max(kcv, agg[i] + 1);
  const int nnzp = kc <= 0 ? 0 : l->sa ? (int)ptci.size() : n;
  const bool folds = cycle_form(l, 16, false, 0, false, false).folded;   // (whatever the panel width)
  const int32_t sz[16] = {l->nv, l->np, l->nbv, l->nbp, l->bs, kc, kcv, kc - kcv, l->sa ? 1 : 0, nnzp,
                          l->child ? 1 : 0, folds ? 1 : 0, l->gt_ok ? 1 : 0, l->precond32 ? 1 : 0, l->agg_v, l->agg_p};
  std::copy(sz, sz + 16, sizes_out);
  down(bv_ptr, l->bv_ptr, (size_t)l->nbv + 1);
  down(bv_rows, l->bv_rows, (size_t)l->nv);
  down(bp_ptr, l->bp_ptr, l->nbp > 0 ? (size_t)l->nbp + 1 : 0);
  down(bp_rows, l->bp_rows, (size_t)l->np);
  if (aggof) std::copy(agg.begin(), agg.end(), aggof);
  if (kc > 0 && (p_rp || p_ci || p_v)) {
    // P by rows: P^T transposed, or one unit entry per row (plain aggregation)
    std::vector<int32_t> rp(n + 1, 0), ci(nnzp);
    std::vector<double> v(nnzp, 1.0);
    if (l->sa) {
      for (int32_t j : ptci) ++rp[j + 1];
      for (int i = 0; i < n; ++i) rp[i + 1] += rp[i];
      std::vector<int32_t> at(rp.begin(), rp.end() - 1);
      for (int a = 0; a < kc; ++a)
        for (int k = ptrp[a]; k < ptrp[a + 1]; ++k) {
          ci[at[ptci[k]]] = a;
          v[at[ptci[k]]++] = ptv[k];
        }
    } else {
      for (int i = 0; i < n; ++i) {
        rp[i + 1] = i + 1;
        ci[i] = agg[i];
      }
    }
    if (p_rp) std::copy(rp.begin(), rp.end(), p_rp);
    if (p_ci) std::copy(ci.begin(), ci.end(), p_ci);
    if (p_v) std::copy(v.begin(), v.end(), p_v);
  }
  HIPCHK(hipStreamSynchronize(st));
  API_END
}

int ricadi_precond_vanka(ricadi_ctx* c, int level, int32_t* sizes_out, int32_t* colour_ptr, int32_t* patch_idx) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(sizes_out && level >= 0, RICADI_EINVAL, "bad argument");
  const ricadi_ctx* l = c;
  for (int i = 0; i < level && l; ++i) l = l->child.get();
  REQUIRE(l, RICADI_EINVAL, "no such level");
  API_BEGIN
  (void)hipSetDevice(c->dev);
  const VankaPatches& vp = l->vk;
  const int32_t sz[8] = {vp.ncolours, vp.npatches, l->vanka ? vp.npress : 0, vp.largest, vp.dropped, vp.nlone,
                         vp.nlone_patches, 0};
  std::copy(sz, sz + 8, sizes_out);
  if (colour_ptr) std::copy(vp.colour_ptr.begin(), vp.colour_ptr.end(), colour_ptr);
  // the records as the device holds them
  if (patch_idx && l->vk_idx.n) {
    HIPCHK(hipMemcpyAsync(patch_idx, l->vk_idx.p, sizeof(int32_t) * l->vk_idx.n, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  }
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
  API_BEGIN
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
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(dR && dX && alphas && betas, RICADI_EINVAL, "NULL argument");
  REQUIRE(ng >= 1 && ng <= RICADI_MAX_GROUPS && (size_t)ng * m <= 2048, RICADI_EINVAL,
          "1 <= ng <= 16 and ng*m <= 2048 required");
  REQUIRE(r_stride == 0 || r_stride >= (int64_t)c->nv * m, RICADI_EINVAL, "bad r_stride");
  int status = RICADI_OK;
  API_BEGIN
  std::vector<ShiftData*> sds(ng);
  get_shifts(c, alphas, betas, ng, sds.data());
  ensure_work(c, m, ng);
  const size_t nm = (size_t)c->n * m;
  const int nload = r_stride == 0 ? 1 : ng;
  for (int g = 0; g < nload; ++g) load_rhs(c, dR + (size_t)g * r_stride, m, c->bvec.p + (size_t)g * nm);
  std::vector<GmresResult> res(ng);
  solve_batch(c, sds.data(), ng, c->bvec.p, r_stride == 0 ? 0 : nm, dX, m, true, relres_out,
              res.data());
  for (int g = 0; g < ng; ++g) {
    if (iters_out) iters_out[g] = res[g].iters;
    if (!res[g].converged) status = solve_status(false);
  }
  API_END_STATUS(status)
}

int ricadi_recycle_guess_dev(ricadi_ctx* c, int ng, const double* alphas, const double* betas, const double* dR, int m,
                             double* dX, int* rank_out) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(dR && dX && alphas && betas && rank_out, RICADI_EINVAL, "NULL argument");
  REQUIRE(ng >= 1 && ng <= RICADI_MAX_GROUPS && (size_t)ng * m <= 2048, RICADI_EINVAL,
          "1 <= ng <= 16 and ng*m <= 2048 required");
  *rank_out = 0;
  API_BEGIN
  std::vector<ShiftData*> sds(ng);
  get_shifts(c, alphas, betas, ng, sds.data());
  ensure_work(c, m, ng);
  load_rhs(c, dR, m, c->bvec.p);
  if (c->rec_depth > 0 && recycle_guess(c, sds.data(), ng, c->bvec.p, m, dX)) *rank_out = (int)c->trace.guess_rank;
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

int ricadi_solve_trace(ricadi_ctx* c, int64_t* out, int nout) {
  REQUIRE(c && out && nout >= 0, RICADI_EINVAL, "bad argument");
  const ricadi_ctx::SolveTrace& t = c->trace;
  const int64_t v[RICADI_TRACE_SLOTS] = {
      t.solves,      t.guess_tried, t.guess_used,       t.guess_cols,     t.guess_rank,     t.guess_pan,
      t.stored,      t.smw_solves,  t.smw_setups,       t.smw_dup,        t.smw_bad,        t.smw_refined,
      t.inop_lowrank, t.esc1_groups, t.esc2_groups,     t.wide_passes,    t.wide_chunks,    t.wide_groups_last,
      t.cycles,      t.cycle_len_last, t.cycle_len_max, t.stalled_groups, t.maxit_groups};
  std::copy(v, v + std::min(nout, (int)RICADI_TRACE_SLOTS), out);
  return RICADI_OK;
}

int ricadi_shift_solve(ricadi_ctx* c, double alpha, double beta, const double* R, const double* Rp,
                       int m, double* X_out, int* iters_out, double* relres_out) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(R && X_out, RICADI_EINVAL, "NULL panel");
  int status = RICADI_OK;
  API_BEGIN
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
  API_BEGIN
  launch_spmm(c->st, c->nv, c->E.rp.p, c->E.ci.p, c->E.v.p, dV, m, nullptr, dW, m, dW, m, coef, 1.0,
              nullptr, m);
  API_END
}

int ricadi_lincomb_dev(ricadi_ctx* c, int nrows, int m, int nvec, const double* dBasis,
                       int64_t stride, const double* coef, double* dOut) {
  REQUIRE(c && dBasis && coef && dOut, RICADI_EINVAL, "NULL argument");
  REQUIRE(nrows > 0 && m >= 1 && m <= RICADI_MAX_M && nvec >= 1 && nvec <= 64, RICADI_EINVAL,
          "bad sizes");
  API_BEGIN
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
  API_BEGIN
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
  API_BEGIN
  gain_dev(c, c->E, dZ, cz, ldz, dB, nb, dK);
  if (coef != 1.0) launch_axpby(c->st, (size_t)c->nv * nb, coef, dK, 0.0, dK);
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

int ricadi_panel_norms_dev(ricadi_ctx* c, const double* dW, int nrows, int m, double* gram_fro,
                           double* nrm2) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(dW && nrows > 0, RICADI_EINVAL, "bad panel");
  API_BEGIN
  gram_norms(c, dW, nrows, m, gram_fro, nrm2);
  API_END
}

int ricadi_time_spmm_dev(ricadi_ctx* c, double alpha, double beta, const double* dX, int m,
                         double* dY, int reps, double* ms_per_launch) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(dX && dY && reps > 0 && ms_per_launch, RICADI_EINVAL, "bad argument");
  API_BEGIN
  ShiftData* sd = get_shift(c, alpha, beta);
  // plain assembled-CSR saddle SpMM only (no low-rank term): the roofline kernel
  const Batch bt = make_batch(c, sd, m);
  *ms_per_launch =
      timed_ms(c->st, reps, [&] { saddle_spmm(c, bt, dX, bt.gs, nullptr, dY, bt.gs, nullptr, 0, 1.0, 0.0); });
  API_END
}

int ricadi_time_spmm_batch_dev(ricadi_ctx* c, int ng, const double* alphas, const double* betas,
                               const double* dX, int m, double* dY, int reps, double* ms_per_launch) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(dX && dY && alphas && betas && reps > 0 && ms_per_launch, RICADI_EINVAL, "bad argument");
  REQUIRE(ng >= 1 && ng <= RICADI_MAX_GROUPS, RICADI_EINVAL, "1 <= ng <= 16 required");
  API_BEGIN
  std::vector<ShiftData*> sds(ng);
  get_shifts(c, alphas, betas, ng, sds.data());
  const Batch bt = make_batch(c, sds.data(), ng, m);
  // the saddle SpMM exactly as the batched GMRES launches it (no low-rank term; on the FP32-stored vector
  // when the iteration does so, and into an FP32 panel when its Arnoldi passes read one: dY is then left alone).
  // The basis storage is the one the solver's workspace will have (no workspace may exist yet).
  Restore<bool> keep16(c->basis16);
  c->basis16 = basis16_default(c);
  const IterationForm f = iteration_form(c, m, ng, false);
  DArr<float> x32, y32;
  if (f.x32) {
    x32.alloc(bt.gs * ng);
    for (int g = 0; g < ng; ++g)
      launch_to_f32(c->st, c->n, m, dX + (size_t)g * bt.gs, m, x32.p + (size_t)g * bt.gs, m);
  }
  if (f.w32) y32.alloc(bt.gs * ng);
  c->w32_last = f.w32 ? 1 : 0;
  auto spmm = [&] { op_apply(c, bt, dX, bt.gs, dY, false, x32.p, y32.p); };
  spmm();   // warm-up
  *ms_per_launch = timed_ms(c->st, reps, spmm);
  API_END
}

// One launch (or launch pair: the dot kernels come with their partial-sum reduction) of a
// hot-path kernel class exactly as the batched GMRES issues it, timed with HIP events on
// the context stream.  Operands are the solver's own workspace buffers, filled with finite
// values; results are discarded.
int ricadi_time_kernel_dev(ricadi_ctx* c, int which, int ng, const double* alphas, const double* betas,
                           int m, int nvec, int reps, double* ms_per_launch) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(alphas && betas && reps > 0 && ms_per_launch, RICADI_EINVAL, "bad argument");
  REQUIRE(ng >= 1 && ng <= RICADI_MAX_GROUPS && (size_t)ng * m <= 2048, RICADI_EINVAL,
          "1 <= ng <= 16 and ng*m <= 2048 required");
  REQUIRE(nvec >= 1 && nvec <= c->opts.gmres_restart, RICADI_EINVAL, "1 <= nvec <= gmres_restart required");
  API_BEGIN
  hipStream_t st = c->st;
  std::vector<ShiftData*> sds(ng);
  get_shifts(c, alphas, betas, ng, sds.data());
  ensure_work(c, m, ng, 0);
  Batch bt = make_batch(c, sds.data(), ng, m);
  const int restart = c->opts.gmres_restart;
  const size_t nm = bt.gs, vs = nm * ng;
  const size_t gsh = (size_t)(restart + 2) * m;
  // finite fill: byte 0x3C -> 1.5e-18 (FP64), 1.06 (FP16), 0.0115 (FP32)
  HIPCHK(hipMemsetAsync(c->wv.p, 0x3C, sizeof(double) * vs, st));
  HIPCHK(hipMemsetAsync(c->zv.p, 0x3C, sizeof(double) * vs, st));
  if (c->zbasisf.p) HIPCHK(hipMemsetAsync(c->zbasisf.p, 0x3C, sizeof(float) * vs, st));
  HIPCHK(hipMemsetAsync(c->r2.p, 0x3C, sizeof(double) * vs, st));
  HIPCHK(hipMemsetAsync(c->h1.p, 0x3C, sizeof(double) * gsh * ng, st));
  HIPCHK(hipMemsetAsync(c->h2.p, 0x3C, sizeof(double) * gsh * ng, st));
  HIPCHK(hipMemsetAsync(c->scale.p, 0x3C, sizeof(double) * (size_t)ng * m, st));
  HIPCHK(hipMemsetAsync(c->resid.p, 0x3C, sizeof(double) * 2 * c->wcols, st));
  HIPCHK(hipMemsetAsync(c->bnorm2.p, 0x3C, sizeof(double) * (size_t)ng * m, st));
  HIPCHK(hipMemsetAsync(c->g.p, 0x3C, sizeof(double) * (size_t)ng * m * (restart + 1), st));
  HIPCHK(hipMemsetAsync(c->cs.p, 0x3C, sizeof(double) * (size_t)ng * m * restart, st));
  HIPCHK(hipMemsetAsync(c->sn.p, 0x3C, sizeof(double) * (size_t)ng * m * restart, st));
  HIPCHK(hipMemsetAsync(c->ls_coef.p, 0x3C, sizeof(double) * c->ls_coef.n, st));
  if (c->kc > 0) {
    HIPCHK(hipMemsetAsync(c->rc.p, 0x3C, sizeof(double) * bt.gsc * ng, st));
    HIPCHK(hipMemsetAsync(c->ec.p, 0x3C, sizeof(double) * bt.gsc * ng, st));
  }
  if (c->np > 0) HIPCHK(hipMemsetAsync(c->tp.p, 0x3C, sizeof(double) * bt.gsp * ng, st));
  const IterationForm f = iteration_form(c, m, ng, false);
  const size_t basis_bytes = (size_t)(nvec + 1) * vs * (f.b16 ? 2 : f.b32 ? 4 : 8);
  if (c->basis32) {
    HIPCHK(hipMemsetAsync(c->basisf.p, 0x3C, basis_bytes, st));
    HIPCHK(hipMemsetAsync(c->vcur.p, 0x3C, sizeof(double) * vs, st));
  } else {
    HIPCHK(hipMemsetAsync(c->basis.p, 0x3C, basis_bytes, st));
  }
  const _Float16* Vh = f.h16 ? reinterpret_cast<_Float16*>(c->basisf.p) : nullptr;
  // the operator's output and the Arnoldi passes on the FP32 panel where the iteration uses it
  c->w32_last = f.w32 ? 1 : 0;
  // the preconditioner cycle on the workspace panels, in the form gmres_core decides
  const CycleForm pf = cycle_form(c, m, bt.blocks16, nm, f.x32, f.h16);
  const CycleIO io{c->wv.p, nm, Vh, c->zv.p, c->zbasisf.p, nm};
  auto launch = [&]() {
    switch (which) {
      case 0:
        op_apply(c, bt, c->zv.p, nm, c->wv.p, false, f.x32 ? c->zbasisf.p : nullptr, f.w32 ? c->wv32.p : nullptr);
        break;
      case 1:
        block_sweep(c, bt, false, c->r2.p, nm, c->zv.p, 0);
        break;
      case 2:
        if (c->nbp <= 0) throw HipError{"no pressure block"};
        block_sweep(c, bt, true, c->tp.p, bt.gsp, c->zv.p + (size_t)c->nv * m, 0);
        break;
      case 3:
        if (c->kc <= 0) throw HipError{"no coarse level"};
        {
          // the dense inverse lives on the last level
          Batch lb = bt;
          ricadi_ctx* lc = walk_levels(c, lb, [](const ricadi_ctx* l) { return !l->child; });
          pc_coarse(lc, lb, cycle_form(lc, m, lb.blocks16, 0, false, false), CycleIO());
        }
        break;
      case 4:
        if (!c->syb_ok) throw HipError{"no tiled S*Y"};
        sy_residual_tiled(c, bt, c->wv.p, nm);
        break;
      // one-reduction form: 5 = its dots (with the reduction), 6 = the end-of-cycle pass, 7 = its update (iteration
      // nvec - 1)
      case 5:
        if (f.lowsync) arnoldi_lowsync_dots(c, bt, same_int(nvec - 1), false);
        else arnoldi_dots(c, f, bt, nvec);
        break;
      case 6:
        if (f.lowsync) arnoldi_lowsync_dots(c, bt, same_int(nvec), true);
        else arnoldi_update_dots(c, f, bt, nvec);
        break;
      case 7:
        if (f.lowsync) arnoldi_lowsync_update(c, bt, nvec - 1, nullptr);
        else arnoldi_update(c, f, bt, nvec, nullptr);
        break;
      case 8:
        precond_apply(c, bt, pf, io);
        break;
      case 9:
        if (c->kc <= 0) throw HipError{"no coarse level"};
        restrict_csr(c, bt, c->wv.p, nm);
        break;
      case 10: case 11: case 12: case 13: case 14: case 15: case 16:
        // ONE stage of the preconditioner application, the function precond_apply itself calls
        cycle_begin(c, pf, io);
        cycle_stages[which - 10](c, bt, pf, io);
        break;
      case RICADI_TK_PC_VANKA: {
        // the Vanka sweep lives on a child level: all its colours on that level's panels, as pc_vanka issues them
        Batch lb = bt;
        ricadi_ctx* lc = walk_levels(c, lb, [](const ricadi_ctx* l) { return l->vanka; });
        if (!lc) throw HipError{"no coarse level with a Vanka sweep"};
        vanka_colours(lc, lb, CycleIO{lc->wv.p, lb.gs, nullptr, lc->zv.p});
        break;
      }
      case RICADI_TK_ITER: case RICADI_TK_ITER_SPLIT:
        break;   // (below)
      default:
        throw HipError{"unknown kernel class"};
    }
  };
  if (which == RICADI_TK_ITER || which == RICADI_TK_ITER_SPLIT) {
    // reps hot iterations j = nvec - 1 (no convergence logic): all groups on the context stream, or the even and the
    // odd group ids as two halves on two streams, forked from it and joined back to it once around all reps
    const bool two = which == RICADI_TK_ITER_SPLIT && ng >= 2;
    HalfSchedule halves(c, bt, two);
    if (two) {
      std::vector<int> all;
      for (int g = 0; g < ng; ++g) {
        halves.half[g & 1].push_back(g);
        all.push_back(g);
      }
      halves.set_live(all);
    }
    auto iters = [&](int k) {
      if (two) halves.fork();
      for (int i = 0; i < k; ++i) {
        if (two) halves.issue(f, pf, nvec - 1, false, nullptr);
        else iteration_launches(c, f, pf, bt, nvec - 1, false, nullptr);
      }
      halves.join();
    };
    iters(1);   // warm-up
    *ms_per_launch = timed_ms(st, 1, [&] { iters(reps); }) / reps;
  } else {
    launch();   // warm-up (code object load, caches)
    *ms_per_launch = timed_ms(st, reps, launch);
  }
  API_END
}

// ---- step probe of the Arnoldi phase (tests) -------------------------------------------------------------------
// The units the lockstep GMRES is made of -- cycle_start_launches, arnoldi_launches, cycle_end_launches of
// solver_gmres.inl -- one call each on the solver's own workspace, with the batch, the iteration form and the cycle
// form decided as for a solve, and the workspace read back in FP64.  The preconditioner and the operator are not run:
// the caller supplies w.  Synchronous.
namespace {
struct ProbeSetup {
  std::vector<ShiftData*> sds;
  Batch bt;
  IterationForm f;
  CycleForm pf;
  ProbeSetup(ricadi_ctx* c, int ng, const double* alphas, const double* betas, int m) : sds(ng) {
    get_shifts(c, alphas, betas, ng, sds.data());
    ensure_work(c, m, ng, 0);
    bt = make_batch(c, sds.data(), ng, m);
    f = iteration_form(c, m, ng, false);
    pf = cycle_form(c, m, bt.blocks16, bt.gs, f.x32, f.h16);
    c->w32_last = f.w32 ? 1 : 0;
  }
  // the batch of the last begin (step, close, read)
  explicit ProbeSetup(ricadi_ctx* c)
      : ProbeSetup(c, c->probe.ng, c->probe.alpha.data(), c->probe.beta.data(), c->probe.m) {}
};
// begin has run and the workspace it filled is still the context's
bool probe_live(const ricadi_ctx* c) {
  return c->probe.ng > 0 && c->probe.work == c->wv.p && c->wrestart == c->opts.gmres_restart;
}
double half_bits_to_double(uint16_t h) {
  const int e = (h >> 10) & 31, f = h & 1023;
  double v = e == 0 ? std::ldexp((double)f, -24) : e == 31 ? (f ? NAN : INFINITY) : std::ldexp(1024.0 + f, e - 25);
  return (h & 0x8000) ? -v : v;
}
// count stored values of `bytes` bytes each (2: FP16, 4: FP32, 8: FP64) at src, as FP64 at dst (both device)
void probe_widen(ricadi_ctx* c, const void* src, int bytes, size_t count, double* dst) {
  if (bytes == 8) {
    HIPCHK(hipMemcpyAsync(dst, src, sizeof(double) * count, hipMemcpyDeviceToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
    return;
  }
  std::vector<unsigned char> raw(count * bytes);
  std::vector<double> wide(count);
  HIPCHK(hipMemcpyAsync(raw.data(), src, raw.size(), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  for (size_t i = 0; i < count; ++i) {
    if (bytes == 2) {
      uint16_t h;
      std::memcpy(&h, raw.data() + 2 * i, 2);
      wide[i] = half_bits_to_double(h);
    } else {
      float x;
      std::memcpy(&x, raw.data() + 4 * i, 4);
      wide[i] = (double)x;
    }
  }
  HIPCHK(hipMemcpyAsync(dst, wide.data(), sizeof(double) * count, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
}
}  // namespace

int ricadi_arnoldi_probe_begin_dev(ricadi_ctx* c, int ng, const double* alphas, const double* betas, int m,
                                   const double* dR, const double* dBnorm) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(alphas && betas && dR && dBnorm, RICADI_EINVAL, "bad argument");
  REQUIRE(ng >= 1 && ng <= RICADI_MAX_GROUPS && (size_t)ng * m <= 2048, RICADI_EINVAL,
          "1 <= ng <= 16 and ng*m <= 2048 required");
  API_BEGIN
  hipStream_t st = c->st;
  c->probe = ricadi_ctx::ArnoldiProbe();
  ProbeSetup p(c, ng, alphas, betas, m);
  const int restart = c->opts.gmres_restart;
  const size_t vs = p.bt.gs * ng, gm = (size_t)ng * m, gsh = (size_t)(restart + 2) * c->wcols;
  // whatever a step does not write reads back as NaN (all bits set, in every storage type)
  if (c->basis32) HIPCHK(hipMemsetAsync(c->basisf.p, 0xFF, (size_t)(restart + 1) * vs * (p.f.b16 ? 2 : 4), st));
  else HIPCHK(hipMemsetAsync(c->basis.p, 0xFF, sizeof(double) * (restart + 1) * vs, st));
  HIPCHK(hipMemsetAsync(c->h1.p, 0xFF, sizeof(double) * gsh, st));
  HIPCHK(hipMemsetAsync(c->h2.p, 0xFF, sizeof(double) * 2 * gsh, st));
  HIPCHK(hipMemsetAsync(c->H.p, 0xFF, sizeof(double) * gm * (restart + 1) * restart, st));
  HIPCHK(hipMemsetAsync(c->cs.p, 0xFF, sizeof(double) * gm * restart, st));
  HIPCHK(hipMemsetAsync(c->sn.p, 0xFF, sizeof(double) * gm * restart, st));
  HIPCHK(hipMemsetAsync(c->yv.p, 0xFF, sizeof(double) * gm * restart, st));
  HIPCHK(hipMemsetAsync(c->resid.p, 0xFF, sizeof(double) * 2 * c->wcols, st));
  HIPCHK(hipMemsetAsync(c->ls_coef.p, 0xFF, sizeof(double) * c->ls_coef.n, st));
  HIPCHK(hipMemcpyAsync(c->wv.p, dR, sizeof(double) * vs, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(c->bnorm2.p, dBnorm, sizeof(double) * gm, hipMemcpyDeviceToDevice, st));
  p.bt.all();
  cycle_start_launches(c, p.f, p.bt, [] { return true; });
  HIPCHK(hipStreamSynchronize(st));
  c->probe.ng = ng;
  c->probe.m = m;
  c->probe.alpha.assign(alphas, alphas + ng);
  c->probe.beta.assign(betas, betas + ng);
  c->probe.kdone.assign(ng, 0);
  c->probe.work = c->wv.p;
  API_END
}

int ricadi_arnoldi_probe_step_dev(ricadi_ctx* c, int j, const double* dW, int nact, const int* groups) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(probe_live(c), RICADI_EINVAL, "no probe cycle: call ricadi_arnoldi_probe_begin_dev first");
  REQUIRE(j >= 0 && j < c->opts.gmres_restart, RICADI_EINVAL, "0 <= j < gmres_restart required");
  REQUIRE(dW && groups && nact >= 1 && nact <= c->probe.ng, RICADI_EINVAL, "bad argument");
  for (int i = 0; i < nact; ++i)
    REQUIRE(groups[i] >= 0 && groups[i] < c->probe.ng, RICADI_EINVAL, "group id outside 0 .. ng-1");
  (void)hipSetDevice(c->dev);
  API_BEGIN
  hipStream_t st = c->st;
  ProbeSetup p(c);
  const int m = c->probe.m;
  const size_t nm = p.bt.gs;
  p.bt.set(std::vector<int>(groups, groups + nact));
  // w as the iteration reads it
  for (int i = 0; i < nact; ++i) {
    const size_t off = (size_t)groups[i] * nm;
    if (p.f.w32) launch_to_f32(st, c->n, m, dW + off, m, c->wv32.p + off, m);
    else HIPCHK(hipMemcpyAsync(c->wv.p + off, dW + off, sizeof(double) * nm, hipMemcpyDeviceToDevice, st));
  }
  const size_t slot = (size_t)RICADI_MAX_M * RICADI_MAX_GROUPS;
  arnoldi_launches(c, p.f, p.bt, j, c->h_resid + 2 * slot + (size_t)(j & 1) * slot);
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < nact; ++i) c->probe.kdone[groups[i]] = j + 1;
  API_END
}

int ricadi_arnoldi_probe_close_dev(ricadi_ctx* c, const int* ks, int nz, const float* dZ, double* dX) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(probe_live(c), RICADI_EINVAL, "no probe cycle: call ricadi_arnoldi_probe_begin_dev first");
  REQUIRE(ks && dZ && dX && nz >= 1 && nz <= c->opts.gmres_restart, RICADI_EINVAL, "bad argument");
  for (int g = 0; g < c->probe.ng; ++g)
    REQUIRE(ks[g] >= 0 && ks[g] <= nz && ks[g] <= c->probe.kdone[g], RICADI_EINVAL,
            "0 <= k_g <= min(nz, steps run for the group) required");
  (void)hipSetDevice(c->dev);
  API_BEGIN
  hipStream_t st = c->st;
  ProbeSetup p(c);
  GroupInts kk = same_int(0);
  for (int g = 0; g < c->probe.ng; ++g) kk.v[g] = ks[g];
  HIPCHK(hipMemcpyAsync(c->zbasisf.p, dZ, sizeof(float) * (size_t)nz * p.bt.gs * c->probe.ng, hipMemcpyDeviceToDevice,
                        st));
  p.bt.all();
  cycle_end_launches(c, p.f, p.bt, kk, dX);
  HIPCHK(hipStreamSynchronize(st));
  API_END
}

int ricadi_arnoldi_probe_read_dev(ricadi_ctx* c, int what, int slot, double* dOut, int64_t cap, int64_t* count) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(probe_live(c), RICADI_EINVAL, "no probe cycle: call ricadi_arnoldi_probe_begin_dev first");
  REQUIRE(dOut && count && cap >= 0, RICADI_EINVAL, "bad argument");
  const int restart = c->opts.gmres_restart, ng = c->probe.ng, m = c->probe.m;
  REQUIRE(what != RICADI_PROBE_BASIS || (slot >= 0 && slot <= restart), RICADI_EINVAL,
          "0 <= slot <= gmres_restart required");
  (void)hipSetDevice(c->dev);
  API_BEGIN
  ProbeSetup p(c);
  const IterationForm& f = p.f;
  const size_t gm = (size_t)ng * m, vs = p.bt.gs * ng, h2buf = (size_t)(restart + 2) * c->wcols;
  const void* src = nullptr;
  int bytes = 8;
  size_t cnt = 0;
  switch (what) {
    case RICADI_PROBE_BASIS:
      bytes = f.b16 ? 2 : f.b32 ? 4 : 8;
      src = c->basis32 ? (const char*)c->basisf.p + (size_t)slot * vs * bytes : (const char*)(c->basis.p + (size_t)slot * vs);
      cnt = vs;
      break;
    case RICADI_PROBE_W: src = c->wv.p, cnt = vs; break;
    case RICADI_PROBE_W32: src = c->wv32.p, bytes = 4, cnt = vs; break;
    case RICADI_PROBE_VCUR:
      if (!c->basis32) throw HipError{"no FP64 copy of the current vector with the FP64-stored basis"};
      src = c->vcur.p, cnt = vs;
      break;
    case RICADI_PROBE_H1: src = c->h1.p, cnt = (size_t)(restart + 2) * gm; break;
    case RICADI_PROBE_H2: src = c->h2.p, cnt = (size_t)(restart + 2) * gm; break;
    case RICADI_PROBE_HSUM: src = c->h2.p + h2buf, cnt = (size_t)(restart + 2) * gm; break;
    case RICADI_PROBE_H: src = c->H.p, cnt = gm * (restart + 1) * restart; break;
    case RICADI_PROBE_CS: src = c->cs.p, cnt = gm * restart; break;
    case RICADI_PROBE_SN: src = c->sn.p, cnt = gm * restart; break;
    case RICADI_PROBE_G: src = c->g.p, cnt = gm * (restart + 1); break;
    case RICADI_PROBE_SCALE: src = c->scale.p, cnt = gm; break;
    case RICADI_PROBE_RESID0: src = c->resid.p, cnt = gm; break;
    case RICADI_PROBE_RESID1: src = c->resid.p + c->wcols, cnt = gm; break;
    case RICADI_PROBE_Y: src = c->yv.p, cnt = gm * restart; break;
    case RICADI_PROBE_NRM2: src = c->nrm2.p, cnt = gm; break;
    case RICADI_PROBE_LS_COEF:
      if (!f.lowsync) throw HipError{"not the one-reduction form"};
      src = c->ls_coef.p, cnt = (size_t)ng * lowsync_coef_stride(restart);
      break;
    case RICADI_PROBE_FORM: cnt = 8; break;
    default: throw HipError{"unknown probe quantity"};
  }
  *count = (int64_t)cnt;
  if ((int64_t)cnt > cap) throw HipError{"output buffer too small"};
  if (what == RICADI_PROBE_FORM) {
    const double bits[8] = {(double)f.b16,   (double)f.b32, (double)f.h16, (double)f.keepw,
                            (double)f.fuseh, (double)f.x32, (double)f.w32, (double)f.lowsync};
    HIPCHK(hipMemcpyAsync(dOut, bits, sizeof(bits), hipMemcpyHostToDevice, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  } else {
    probe_widen(c, src, bytes, cnt, dOut);
  }
  API_END
}

int ricadi_qr(ricadi_ctx* c, const double* Z, int cz, double* Q_out, double* R_out) {
  REQUIRE(c && c->nv > 0, RICADI_ESTATE, "set the operator (or the dimensions) first");
  REQUIRE(Z && R_out && cz > 0 && cz <= c->nv, RICADI_EINVAL, "bad argument");
  API_BEGIN
  (void)hipSetDevice(c->dev);
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
  API_BEGIN
  (void)hipSetDevice(c->dev);
  project_pencil_dev(c, dQ, k, dHA, dHE);
  API_END
}

int ricadi_project_pencil(ricadi_ctx* c, const double* Q, int k, double* HA, double* HE) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(Q && HA && HE && k >= 1 && k <= RICADI_MAX_M && k <= c->nv, RICADI_EINVAL, "bad argument");
  API_BEGIN
  (void)hipSetDevice(c->dev);
  const size_t nq = (size_t)c->nv * k, nh = (size_t)k * k;
  TArr<double> dQ(c->pool, nq), dH(c->pool, 2 * nh);
  HIPCHK(hipMemcpyAsync(dQ.p, Q, sizeof(double) * nq, hipMemcpyHostToDevice, c->st));
  project_pencil_dev(c, dQ.p, k, dH.p, dH.p + nh);
  HIPCHK(hipMemcpyAsync(HA, dH.p, sizeof(double) * nh, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipMemcpyAsync(HE, dH.p + nh, sizeof(double) * nh, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

int ricadi_setup_info(ricadi_ctx* c, int* out, int nout) {
  REQUIRE(c && out && nout >= 8, RICADI_EINVAL, "bad argument");
  out[0] = c->nv;
  out[1] = c->np;
  out[2] = c->nbv;
  out[3] = c->nbp;
  out[4] = c->bs;
  out[5] = c->kc;
  out[6] = c->sb_nblk;
  out[7] = c->sb_max_cols;
  for (int i = 8; i < nout; ++i) out[i] = 0;
  // [8]: levels in use; [9]: size of the dense inverse on the last level
  int lv = c->kc > 0 ? 2 : 1;
  const ricadi_ctx* lc = c;
  for (; lc->child; lc = lc->child.get()) ++lv;
  if (nout > 8) out[8] = lv;
  if (nout > 9) out[9] = lc->kc;
  // [10]: 1 if the iteration reads the current vector from the FP16 basis (no FP64 copy written), 16-column panels
  if (nout > 10) out[10] = (c->has_op && cycle_form(c, 16, false, 0, false, basis16_default(c)).h16) ? 1 : 0;
  // [11], [12]: padded widths of the dense rectangles of the last / first velocity sweep (0: sweep not in that form);
  // [13]: pressure dofs per Schur block list entry count (np), [14]: nnz(J), [15]: nnz of the pressure rows of S*Y
  if (nout > 11) out[11] = c->gt_ok ? c->gt_ks : 0;
  if (nout > 12) out[12] = (c->ady_ok && c->kc > 0) ? c->ady_ks : 0;
  if (nout > 13) out[13] = c->np;
  if (nout > 14) out[14] = (int)c->J.ci.n;
  if (nout > 15) out[15] = c->kc > 0 && c->np > 0 ? (int)(c->synnz) : 0;
  // [16]: entries of the restriction (rows of P^T with smoothed aggregation; else one per dof)
  if (nout > 16) out[16] = c->kc > 0 ? (c->sa ? (int)c->pt_ci.n : c->n) : 0;
  // [17]: route of the last batch of dense coarse inverses on the last level (0 block Gauss-Jordan, 1 rocSOLVER with
  // partial pivoting; -1 none yet); [18]: kernel of the last saddle SpMM launch (0 CSR, 1 LDS-tiled per
  // group, 2 LDS-tiled multi-shift, +4: FP32 x input; -1 none yet)
  if (nout > 17) out[17] = lc->coarse_route;
  if (nout > 18) out[18] = c->k1_variant;
  // [19]: the last preconditioner application kept the velocity part between its sweeps as an FP32 panel (1) or as
  // an FP64 panel (0); -1 none yet
  if (nout > 19) out[19] = c->mid32_last;
  // [20]: the operator launch of the last iteration / timing call wrote w as an FP32 panel (1) or FP64 (0); -1 none yet
  if (nout > 20) out[20] = c->w32_last;
  // [21] .. [26]: the coloured Vanka sweep of the first child level that has one: in use, colours, patches (one per
  // pressure unknown of that level), largest patch, entries of J dropped by the size cap, lone pseudo-patches
  const ricadi_ctx* vc = c->child.get();
  while (vc && !vc->vanka) vc = vc->child.get();
  if (vc) {
    const int v[6] = {1, vc->vk.ncolours, vc->vk.npress, vc->vk.largest, vc->vk.dropped, vc->vk.nlone_patches};
    for (int i = 0; i < 6; ++i)
      if (nout > 21 + i) out[21 + i] = v[i];
  }
  // [27] .. [29]: the hierarchy rule in force, its levels as ricadi_host_plan_hierarchy counts them (grids with a
  // sweep of their own), the dense inverse of the last one
  if (nout > 27) out[27] = c->opts.hierarchy;
  if (nout > 28) out[28] = lv - (c->kc > 0 ? 1 : 0);
  if (nout > 29) out[29] = lc->kc;
  return RICADI_OK;
}

int ricadi_dense_inverse_batch(ricadi_ctx* c, int k, int nb, double* A, int* route_out) {
  REQUIRE(c && A && k >= 1 && nb >= 1 && nb <= 4 * RICADI_MAX_GROUPS, RICADI_EINVAL, "bad argument");
  API_BEGIN
  hipStream_t st = c->st;
  const size_t kk = (size_t)k * k;
  DArr<double> dA, dA0;
  dA.alloc(kk * nb);
  dA0.alloc(kk * nb);
  HIPCHK(hipMemcpyAsync(dA.p, A, sizeof(double) * kk * nb, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dA0.p, dA.p, sizeof(double) * kk * nb, hipMemcpyDeviceToDevice, st));
  std::vector<double*> hp(nb);
  for (int i = 0; i < nb; ++i) hp[i] = dA.p + kk * i;
  std::vector<int> info(nb, 0);
  const int route = invert_dense_batch(c, hp, k, info, [&] {
    HIPCHK(hipMemcpyAsync(dA.p, dA0.p, sizeof(double) * kk * nb, hipMemcpyDeviceToDevice, st));
  });
  if (route_out) *route_out = route;
  for (int i = 0; i < nb; ++i)
    if (info[i] != 0) throw HipError{"matrix " + std::to_string(i) + " singular (getrf/getri info " + std::to_string(info[i]) + ")"};
  HIPCHK(hipMemcpyAsync(A, dA.p, sizeof(double) * kk * nb, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  API_END
}

int ricadi_time_qr_dev(ricadi_ctx* c, const double* dZ, int cz, int reps, double* ms_per_call) {
  REQUIRE(c && c->nv > 0 && dZ && cz > 0 && cz <= c->nv && reps > 0 && ms_per_call, RICADI_EINVAL,
          "bad argument");
  API_BEGIN
  (void)hipSetDevice(c->dev);
  DArr<double> Q, R;
  Q.alloc((size_t)c->nv * cz);
  R.alloc((size_t)cz * cz);
  *ms_per_call = timed_ms(c->st, reps, [&] { block_qr_dev(c, dZ, cz, c->nv, cz, Q.p, R.p); });
  API_END
}

int ricadi_time_gram_dev(ricadi_ctx* c, const double* dZ, int cz, double* dG, int reps,
                         double* ms_per_launch) {
  REQUIRE(c && c->nv > 0 && dZ && dG && cz > 0 && reps > 0 && ms_per_launch, RICADI_EINVAL,
          "bad argument");
  API_BEGIN
  (void)hipSetDevice(c->dev);
  HIPCHK(hipMemsetAsync(dG, 0, sizeof(double) * cz * cz, c->st));
  *ms_per_launch = timed_ms(c->st, reps, [&] { launch_gemm_tn(c->st, c->nv, cz, cz, dZ, cz, dZ, cz, dG, cz); });
  API_END
}

int ricadi_lyap_adi(ricadi_ctx* c, const double* shifts, int ns, const double* W, int m,
                    const ricadi_adi_params* prm, double* Z_out, int* c_out, double* stats_out) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(shifts && ns > 0 && W && prm, RICADI_EINVAL, "bad argument");
  for (int i = 0; i < ns; ++i) REQUIRE(shifts[i] < 0.0, RICADI_EINVAL, "ADI shifts must be negative");
  REQUIRE(prm->adi_max_steps > 0, RICADI_EINVAL, "adi_max_steps must be positive");
  API_BEGIN
  ensure_work(c, m);
  const long esc0 = c->escalations;
  factor_reserve(c, prm->adi_max_steps * m);
  DArr<double> dW;
  dW.alloc((size_t)c->nv * m);
  HIPCHK(hipMemcpyAsync(dW.p, W, sizeof(double) * c->nv * m, hipMemcpyHostToDevice, c->st));
  if (c->sw.timing) c->t_setup = c->t_solve = c->t_recomb = c->t_compress = c->t_proj = c->t_cyc = c->t_iter = c->t_guess = 0;
  Tick tka;
  AdiStats s = lyap_adi_dev(c, shifts, ns, dW.p, m, *prm);
  if (c->sw.timing) {
    (void)hipStreamSynchronize(c->st);
    fprintf(stderr, "[ricadi timing] lyap_adi: total %.1f ms = setup %.1f + projection %.1f + solves %.1f (Arnoldi iterations %.1f, "
            "restart-cycle bookkeeping %.1f, recycled guesses %.1f) + recombination %.1f + recompression %.1f (+ rest)\n",
            1e3 * tka.lap(), 1e3 * c->t_setup, 1e3 * c->t_proj, 1e3 * c->t_solve, 1e3 * c->t_iter, 1e3 * c->t_cyc,
            1e3 * c->t_guess, 1e3 * c->t_recomb, 1e3 * c->t_compress);
  }
  if (c_out) *c_out = c->zc;
  if (Z_out && c->zc > 0) {
    HIPCHK(hipMemcpy2DAsync(Z_out, sizeof(double) * c->zc, c->Z.p, sizeof(double) * c->zld,
                            sizeof(double) * c->zc, c->nv, hipMemcpyDeviceToHost, c->st));
    HIPCHK(hipStreamSynchronize(c->st));
  }
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

}  // extern "C"

extern "C" {

int ricadi_ric_newtonadi(ricadi_ctx* c, const double* shifts, int ns, const double* B, int nb,
                         const double* W, int mw, const double* Z0, int c0, const double* oldB,
                         const ricadi_adi_params* prm, double* Z_out, int zcap, int* c_out,
                         double* stats_out) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(shifts && ns > 0 && B && W && prm, RICADI_EINVAL, "bad argument");
  REQUIRE(nb >= 1 && nb <= 64 && mw >= 1 && mw + nb <= RICADI_MAX_M, RICADI_EINVAL, "bad widths");
  REQUIRE(c0 == 0 || Z0, RICADI_EINVAL, "Z0 is NULL");
  for (int i = 0; i < ns; ++i) REQUIRE(shifts[i] < 0.0, RICADI_EINVAL, "ADI shifts must be negative");
  API_BEGIN
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
    HIPCHK(hipMemcpy2DAsync(Z_out, sizeof(double) * c->zc, c->Z.p, sizeof(double) * c->zld,
                            sizeof(double) * c->zc, nv, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  API_END
}

// The same with every panel ALREADY ON THE DEVICE (no PCIe traffic inside the call): dB, dW, dZ0, dOldB are device
// pointers (row-major, leading dimension = width; dZ0 / dOldB may be NULL with c0 = 0).  The new iterate stays in
// the context's factor: ricadi_factor_cols, ricadi_factor_get (host) / ricadi_factor_get_dev (device).
int ricadi_ric_newtonadi_dev(ricadi_ctx* c, const double* shifts, int ns, const double* dB, int nb,
                             const double* dW, int mw, const double* dZ0, int c0, const double* dOldB,
                             const ricadi_adi_params* prm, int* c_out, double* stats_out) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(shifts && ns > 0 && dB && dW && prm, RICADI_EINVAL, "bad argument");
  REQUIRE(nb >= 1 && nb <= 64 && mw >= 1 && mw + nb <= RICADI_MAX_M, RICADI_EINVAL, "bad widths");
  REQUIRE(c0 == 0 || dZ0, RICADI_EINVAL, "Z0 is NULL");
  for (int i = 0; i < ns; ++i) REQUIRE(shifts[i] < 0.0, RICADI_EINVAL, "ADI shifts must be negative");
  API_BEGIN
  ric_newtonadi_run(c, shifts, ns, dB, nb, dW, mw, dZ0, c0, dOldB, prm, stats_out);
  if (c_out) *c_out = c->zc;
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

// Copy of the device-resident factor into a DEVICE buffer (nv x cz row-major, ld cz; cz = ricadi_factor_cols)
int ricadi_factor_get_dev(ricadi_ctx* c, double* dZ_out, int cz) {
  REQUIRE(c && dZ_out, RICADI_EINVAL, "NULL argument");
  REQUIRE(cz == c->zc && cz > 0, RICADI_EINVAL, "column count differs from the resident factor");
  API_BEGIN
  launch_copy_cols(c->st, c->nv, cz, c->Z.p, c->zld, 0, dZ_out, cz, 0, 1.0);
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

int ricadi_compress(ricadi_ctx* c, const double* Z, int cz, double thresh, int kmax, double* Zc_out,
                    int* k_out, double* sv_out) {
  REQUIRE(c && c->nv > 0, RICADI_ESTATE, "set the operator (or the dimensions) first");
  REQUIRE(Zc_out && k_out, RICADI_EINVAL, "NULL output");
  API_BEGIN
  const double* dZ;
  int ld;
  DArr<double> tmp, out;
  if (Z) {
    REQUIRE(cz > 0, RICADI_EINVAL, "bad column count");
    tmp.alloc((size_t)c->nv * cz);
    HIPCHK(hipMemcpyAsync(tmp.p, Z, sizeof(double) * c->nv * cz, hipMemcpyHostToDevice, c->st));
    dZ = tmp.p;
    ld = cz;
  } else {
    REQUIRE(c->zc > 0, RICADI_ESTATE, "no device-resident factor");
    dZ = c->Z.p;
    cz = c->zc;
    ld = c->zld;
  }
  out.alloc((size_t)c->nv * cz);
  std::vector<double> sv;
  // the reference's route -- thin QR, then SVD of R ("QR ... SVD", optcont_main.py:133-134) -- up to 1024 columns
  // (the factors the Newton iteration returns are recompressed to a few hundred); raw factors beyond that take the
  // Gram route (singular values resolved to sqrt(eps) sigma_1 instead of eps sigma_1): an O(n c^2) block QR with
  // re-orthogonalisation of thousands of columns costs seconds
  const bool qr_route = c->opts.compress_qr != 0 && cz <= 1024;
  int k = compress_dev(c, dZ, cz, ld, thresh, kmax, false, out.p, &sv, qr_route);
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
  API_BEGIN
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
  API_BEGIN
  const int nv = c->nv;
  DArr<double> dZ, dB, dK;
  const double* z;
  int ld;
  if (Z) {
    REQUIRE(cz > 0, RICADI_EINVAL, "bad column count");
    dZ.alloc((size_t)nv * cz);
    HIPCHK(hipMemcpyAsync(dZ.p, Z, sizeof(double) * nv * cz, hipMemcpyHostToDevice, c->st));
    z = dZ.p;
    ld = cz;
  } else {
    REQUIRE(c->zc > 0, RICADI_ESTATE, "no device-resident factor");
    z = c->Z.p;
    cz = c->zc;
    ld = c->zld;
  }
  dB.alloc((size_t)nv * nb);
  dK.alloc((size_t)nv * nb);
  HIPCHK(hipMemcpyAsync(dB.p, B, sizeof(double) * nv * nb, hipMemcpyHostToDevice, c->st));
  if (mt_rp) {
    HostCsr Mt = make_csr(nv, nv, mt_rp, mt_ci, mt_v);
    DevCsr dMt;
    dMt.upload(Mt, c->st);
    gain_dev(c, dMt, z, cz, ld, dB.p, nb, dK.p);
  } else {
    gain_dev(c, c->E, z, cz, ld, dB.p, nb, dK.p);
  }
  HIPCHK(hipMemcpyAsync(K_out, dK.p, sizeof(double) * nv * nb, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

int ricadi_lyap_res_norm(ricadi_ctx* c, const double* Z, int cz, const double* W, int m,
                         double* res2_out) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(Z && W && res2_out && cz > 0 && m > 0, RICADI_EINVAL, "bad argument");
  API_BEGIN
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
  API_BEGIN
  HIPCHK(hipMemcpy2DAsync(Z_out, sizeof(double) * cz, c->Z.p, sizeof(double) * c->zld,
                          sizeof(double) * cz, c->nv, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

int ricadi_factor_set(ricadi_ctx* c, const double* Z, int cz) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(Z && cz > 0, RICADI_EINVAL, "bad argument");
  API_BEGIN
  factor_reserve(c, cz);
  HIPCHK(hipMemcpyAsync(c->Z.p, Z, sizeof(double) * c->nv * cz, hipMemcpyHostToDevice, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  c->zc = cz;
  API_END
}

}  // extern "C"

