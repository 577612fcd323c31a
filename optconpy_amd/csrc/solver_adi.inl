// solver_adi.inl -- setup prefetch, projection; low-rank ADI in step and sweep form, rank-sharded sweeps (exchange).
// Part of ricadi_solver.hip (one translation unit; included there in order).

// ---- low-rank ADI (device resident) -------------------------------------------------
struct AdiStats {
  int steps = 0;
  double rel = 0.0;
  long gmres_iters = 0;
  long shift_solves = 0;
  double res_fro = 0.0;
  long nonconverged = 0;      // shift-solves that hit gmres_maxit above the tolerance
  double worst_relres = 0.0;
  int sweeps = 0;             // sweep form: batched sweeps run (= all-gathers when sharded)
};

// The last RICADI_XCTL bytes of the send buffer (and the last world * RICADI_XCTL of the receive buffer) are kept
// for the small control messages (decisions, statistics), so that they never touch panels in flight.
#define RICADI_XCTL 4096
static size_t exchange_panel_capacity(const ricadi_ctx* c) { return c->xcap > RICADI_XCTL ? c->xcap - RICADI_XCTL : 0; }
static void require_exchange_capacity(const ricadi_ctx* c, size_t bytes) {
  if (bytes > exchange_panel_capacity(c))
    throw HipError{"exchange buffer too small: " + std::to_string(bytes + RICADI_XCTL) + " bytes per rank needed, " +
                   std::to_string(c->xcap) + " given to ricadi_set_exchange"};
}
// All-gather of `count` doubles per rank through the host's collective (ricadi_set_exchange): the ranks' first
// `count` doubles of `send` arrive rank-major in `recv`.  The context stream is drained first (callback) or the
// collective is ordered on it (RCCL).
static void exchange_at(ricadi_ctx* c, double* send, double* recv, size_t count) {
  ++c->xcount;
  if (c->xcomm) {
    // RCCL: stream ordered behind the solves that filled `send`, ahead of the recombination that reads `recv`
    const ncclResult_t r = ncclAllGather(send, recv, count, ncclDouble, c->xcomm, c->st);
    if (r != ncclSuccess) throw HipError{std::string("ncclAllGather: ") + ncclGetErrorString(r)};
    return;
  }
  HIPCHK(hipStreamSynchronize(c->st));
  const int rc = c->xfn(c->xuser, send, recv, (int64_t)(count * sizeof(double)));
  if (rc != 0) throw HipError{"the all-gather callback of ricadi_set_exchange failed (" + std::to_string(rc) + ")"};
}
// ... of the panels: c->xsend to c->xrecv
static void exchange(ricadi_ctx* c, size_t count) {
  require_exchange_capacity(c, count * sizeof(double));
  exchange_at(c, c->xsend, c->xrecv, count);
}
static double* ctl_send(ricadi_ctx* c) { return c->xsend + exchange_panel_capacity(c) / sizeof(double); }
static double* ctl_recv(ricadi_ctx* c) {
  return c->xrecv + (size_t)c->xworld * exchange_panel_capacity(c) / sizeof(double);
}
static bool sharded(const ricadi_ctx* c) { return (c->xworld > 1 || c->xforce) && (c->xfn != nullptr || c->xcomm != nullptr); }

// Per-shift data of the ADI shifts an iteration is about to use -- and of the projection
// operator (alpha, beta) = (1, 0) when `with_projection` -- built in ONE setup pass: the
// coarse matrices of all of them go through the same batched factorisation (a matrix set
// up alone costs ~8x its share of a batch of 16).
static void prefetch_setup(ricadi_ctx* c, const double* shifts, int nuse, bool with_projection) {
  std::vector<double> al, be;
  if (with_projection && c->np > 0) {
    al.push_back(1.0);
    be.push_back(0.0);
  }
  for (int i = 0; i < nuse; ++i) {
    al.push_back(shifts[i]);
    be.push_back(1.0);
  }
  if (al.empty()) return;
  std::vector<ShiftData*> sds(al.size());
  get_shifts(c, al.data(), be.data(), (int)al.size(), sds.data());
}

// W (NV x m, device, in place) <- P^T W  through one saddle solve with cal E
static void project_panel(ricadi_ctx* c, double* dW, int m) {
  if (c->np == 0) return;
  ShiftData* sd = get_shift(c, 1.0, 0.0);
  ensure_work(c, m);
  load_rhs(c, dW, m, c->bvec.p);
  GmresResult r = gmres_solve(c, sd, c->bvec.p, c->xs.p, m, false, nullptr);
  if (!r.converged) throw HipError{"projection solve did not converge"};
  launch_spmm(c->st, c->nv, c->E.rp.p, c->E.ci.p, c->E.v.p, c->xs.p, m, nullptr, dW, m, nullptr, 0,
              1.0, 0.0, nullptr, m);
}

// Per-shift setup beside the projection solve.  The serial order (prefetch_setup, then project_panel) sets up the
// ADI shifts and the projection operator (alpha, beta) = (1, 0) in one batch and then solves.  The overlapped order:
//   1. the projection operator alone on the main stream (get_shift: issued and finished),
//   2. the setup of the ADI shifts issued on the auxiliary stream (this function),
//   3. the projection solve on the main stream (the caller: project_panel),
//   4. setup_finish (the caller).
// Returns false -- nothing done, the caller keeps the serial order -- without a projection, with a child level
// (its setup runs on the parent's stream), when sharded (a rank's setup failure must reach the other ranks through
// the sweep's status words, which the serial order reports from one place) and with RICADI_SETUP_OVERLAP=0.
// Scratch that both streams touch between 2 and 4:
//   * gj_cb / gj_rp / gj_rb / gj_d / gj_ptrs / gj_hptrs: used by setups only, and 1 is finished before 2 is issued;
//   * flag words: the auxiliary Exec has its own (flag2); the solve uses none of c->flag;
//   * pools: the setup takes nothing from a pool (ShiftData owns its buffers); the solve uses c->pool on the main
//     stream only;
//   * rc / ec and the rest of the GMRES workspace: not touched by the setup; ensure_work has sized them before;
//   * ipiv / info / eptrs (pivoted route): used by setup_finish only, after the auxiliary stream has drained;
//   * st2 / rb2 / ev_z: shared with the asynchronous recompression, which runs inside the sweeps, after 4.
static bool setup_overlap_begin(ricadi_ctx* c, const double* shifts, int nuse, bool project, SetupJob& job) {
  if (!project || c->np == 0 || c->child || sharded(c) || !c->sw.setup_overlap) return false;
  get_shift(c, 1.0, 0.0);
  std::vector<double> be(nuse, 1.0);
  std::vector<ShiftData*> sds(nuse);
  setup_issue(c, aux_exec(c), shifts, be.data(), nuse, sds.data(), job);
  return true;
}
// body(); with `fail` given, what it throws is recorded there instead
template <class F>
static void run_guarded(std::string* fail, F&& body) {
  if (!fail) {
    body();
    return;
  }
  try {
    body();
  } catch (const HipError& e) {
    *fail = e.msg;
  } catch (const std::exception& e) {
    *fail = e.what();
  }
}
// What every driver does before its first shift solve: the per-shift setup of `shifts` and, with `project`, dW (NV x m)
// <- P^T dW -- in the overlapped order where setup_overlap_begin takes it, else prefetch_setup; project_panel;
// setup_finish.  `after_setup` runs between the setup and the projection (the drivers' timers).  With `fail` given
// (rank-sharded sweeps) a failure of the serial setup or of the projection is recorded there instead of thrown, and
// the projection is skipped once it is set.
static void setup_and_project(ricadi_ctx* c, const double* shifts, int nuse, bool project, double* dW, int m,
                              std::string* fail = nullptr, const std::function<void()>& after_setup = nullptr) {
  SetupJob sjob;
  if (!setup_overlap_begin(c, shifts, nuse, project, sjob))
    run_guarded(fail, [&] { prefetch_setup(c, shifts, nuse, project); });
  if (after_setup) after_setup();
  if (project && (!fail || fail->empty())) run_guarded(fail, [&] { project_panel(c, dW, m); });
  setup_finish(c, sjob);          // (overlapped order only: the projection's time then includes the wait for the setup)
}

// Control message: v[0..n) of every rank arrive rank-major in ctl_recv (queued; the caller fetches and waits)
static void ctl_allgather(ricadi_ctx* c, const double* v, int n) {
  if ((size_t)n * sizeof(double) > RICADI_XCTL) throw HipError{"control message too long"};
  HIPCHK(hipMemcpyAsync(ctl_send(c), v, sizeof(double) * n, hipMemcpyHostToDevice, c->st));
  exchange_at(c, ctl_send(c), ctl_recv(c), (size_t)n);
}
// v[0..n) <- rank 0's values (decisions must not differ between the ranks: the norms they rest on come
// from kernels with atomic accumulation).  One tiny all-gather.
static void values_of_rank0(ricadi_ctx* c, double* v, int n) {
  if (!sharded(c)) return;
  ctl_allgather(c, v, n);
  HIPCHK(hipMemcpyAsync(v, ctl_recv(c), sizeof(double) * n, hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
}
// v[0..nsum) <- sum over the ranks, v[nsum..nsum+nmax) <- maximum over the ranks (statistics)
static void reduce_over_ranks(ricadi_ctx* c, double* v, int nsum, int nmax) {
  if (!sharded(c)) return;
  const int n = nsum + nmax;
  ctl_allgather(c, v, n);
  std::vector<double> all((size_t)n * c->xworld);
  HIPCHK(hipMemcpyAsync(all.data(), ctl_recv(c), sizeof(double) * all.size(), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  for (int i = 0; i < n; ++i) {
    double t = all[i];
    for (int r = 1; r < c->xworld; ++r) {
      const double o = all[(size_t)r * n + i];
      t = i < nsum ? t + o : std::max(t, o);
    }
    v[i] = t;
  }
}

// The Z blocks of one sweep and their squared column norms: block j = sum_s coef[j][s] U_s (U_s = ubase + s * ustride,
// the first NV rows of each; coef the replicated device table coef[(j nslot + s) m + c]) into columns
// zc0 + j m .. of Z (leading dimension zld), norms2[j m + c] its squared column norms.  All blocks in the two
// launches of the fused kernel (sums in a fixed order) where it takes the sizes -- nslot <= 16 and G <= 16 --,
// else block by block through c->sweep_t.  Returns whether the fused kernel ran.  The caller has sized
// c->sweep_t (NV x m), the GMRES workspace for width m (the per-block norms use its partials) and norms2 (G m).
static bool sweep_blocks(ricadi_ctx* c, const double* ubase, size_t ustride, int nslot, int G, int m,
                         const double* coef, double* Z, int zld, int zc0, double* norms2) {
  hipStream_t st = c->st;
  const int nv = c->nv;
  const bool combined = sweep_combine_ok(m, nslot, G);
  if (combined) {
    // all blocks and their norms in two launches (K4s)
    c->sweep_part.ensure(sweep_combine_partial_len(nv, m, G));
    launch_sweep_combine(st, nv, m, nslot, G, ubase, ustride, coef, Z, zld, zc0, c->sweep_part.p, norms2);
  } else {
    for (int j = 0; j < G; ++j) {
      launch_cols_update(st, nv, m, nslot, ubase, ustride, coef + (size_t)j * nslot * m, 1.0, nullptr, nullptr,
                         c->sweep_t.p);
      launch_copy_cols(st, nv, m, c->sweep_t.p, m, 0, Z, zld, zc0 + j * m, 1.0);
      col_norms2(c, c->sweep_t.p, nv, m, norms2 + (size_t)j * m);
    }
  }
  return combined;
}

// Residual rule (adi_res_reltol; ricadi.h): whether the residual of every step is evaluated at all
static bool adi_res_wanted(const ricadi_ctx* c, const ricadi_adi_params& prm) {
  return prm.adi_res_reltol > 0.0 || c->adi_res_record;
}
// pinned host buffer the Gram matrix of the residual rule is fetched into (a copy to pageable memory would make the
// host wait by itself, ahead of the synchronisation that fetches the block norms)
static double* res_host(ricadi_ctx* c, size_t count) {
  if (count > c->h_res_cap) {
    if (c->h_res) (void)hipHostFree(c->h_res);
    c->h_res = nullptr;
    c->h_res_cap = 0;
    HIPCHK(hipHostMalloc((void**)&c->h_res, sizeof(double) * count, hipHostMallocDefault));
    c->h_res_cap = count;
  }
  return c->h_res;
}
// ||V^T V||_F of V = sum_x d[x] P_blk[x] from the Gram matrix Gm (nc x nc) of the panel P, whose column block b is
// columns b m .. b m + m: V^T V = sum_xy d[x] d[y] Gm[blk[x], blk[y]].  Plain loops in a fixed order.
static double gram_combination_fro(const double* Gm, int nc, int m, const int* blk, const double* d, int cnt) {
  double f = 0.0;
  for (int a = 0; a < m; ++a)
    for (int b = 0; b < m; ++b) {
      double s = 0.0;
      for (int x = 0; x < cnt; ++x) {
        double t = 0.0;
        for (int y = 0; y < cnt; ++y) t += d[y] * Gm[((size_t)blk[x] * m + a) * nc + (size_t)blk[y] * m + b];
        s += d[x] * t;
      }
      f += s * s;
    }
  return std::sqrt(f);
}

// ... of the single block `blk`
static double gram_block_fro(const double* Gm, int nc, int m, int blk) {
  const double one = 1.0;
  return gram_combination_fro(Gm, nc, m, &blk, &one, 1);
}

static_assert(AdiStop::kMaxSteps == RICADI_STOP_MAX_STEPS && AdiStop::kNewZ == RICADI_STOP_NEWZ &&
                  AdiStop::kRes == RICADI_STOP_RES, "AdiStop::Rule restates RICADI_STOP_*");

// The shifts of one sweep with their Cauchy data: R^-1 (g x g, C_ij = -1/(p_i+p_j) = R^T R) and C^-1 1
struct CauchySet {
  std::vector<double> ps, rinv, cinv1;
  // <- the g shifts behind step `first` of the cycle; false: their Cauchy matrix is numerically singular
  bool fill(const double* shifts, int ns, int first, int g) {
    ps.resize(g);
    for (int i = 0; i < g; ++i) ps[i] = shifts[(first + i) % ns];
    rinv.assign((size_t)g * g, 0.0);
    cinv1.assign(g, 0.0);
    return cauchy_data(ps.data(), g, rinv.data(), cinv1.data()) == RICADI_OK;
  }
};
// out <- C_k^-1 1 of the leading k shifts of a sweep (R^-1 of the leading block is the leading block of R^-1)
static void cauchy_cinv_prefix(const double* ps, int k, std::vector<double>& out) {
  std::vector<double> rdummy((size_t)k * k, 0.0);
  out.assign(k, 0.0);
  if (cauchy_data(ps, k, rdummy.data(), out.data()) != RICADI_OK)
    throw HipError{"Cauchy matrix of a truncated ADI sweep is numerically singular"};
}

// The sweep width G this shift list allows (0: none, the caller keeps the step form) and, in `cycle`, the Cauchy data
// of every sweep until the shift pattern repeats.  A numerically singular Cauchy matrix (the shifts of a sweep too
// many / too close: 16 consecutive entries of a 128-shift list over 3.5 decades) halves the width until every sweep
// of the cycle is admissible -- as shift_parallel.py does.  Host arithmetic only: nothing is launched or allocated.
static int admissible_width(const double* shifts, int ns, int m, const ricadi_adi_params& prm,
                            std::vector<CauchySet>& cycle) {
  int G = std::min(std::min(prm.sweep_width, ns), RICADI_MAX_GROUPS);
  while (G >= 2 && (prm.adi_max_steps < G || G * m > 2048)) G /= 2;
  if (G < 2) return 0;
  for (int i = 0; i < ns; ++i)
    for (int j = i + 1; j < ns; ++j)
      if (shifts[i] == shifts[j]) return 0;     // sweeps need distinct shifts
  for (; G >= 2; G /= 2) {
    cycle.assign(ns / std::gcd(ns, G), CauchySet());
    bool ok = true;
    for (size_t sw = 0; sw < cycle.size() && ok; ++sw) ok = cycle[sw].fill(shifts, ns, (int)sw * G, G);
    if (ok) return G;
  }
  return 0;
}

// Sweep form of the ADI: G consecutive steps with distinct shifts are G
// independent solves against the SAME residual factor,
//   S(p_g) [U_g; *] = [W; 0],
// recombined with the G x G Cauchy matrix C_ij = -1/(p_i+p_j) = R^T R:
//   Z-block = U (R^-1 (x) I),   W <- W + E U ((C^-1 1) (x) I)
// -- identical to the G sequential steps up to a rotation of the block's columns (Z Z^T and the gain are the same).
// The G solves go through ONE batched lockstep GMRES, which is what fills the GPU at n ~ 3e4.  Column block j of
// U R^-1 lies in span{U_1..U_j}: it IS the block the step-by-step iteration appends at step j (up to its sign), so
// the stopping rules (AdiStop) are applied block by block, the blocks behind the stopping step are dropped, and the
// iteration ends after the same step as the sequential one.  Any run of consecutive, distinct shifts is a valid
// sweep; where AdiStop::cut shortens one, its Cauchy data -- and those of the misaligned sweeps behind it -- are computed
// on the spot, for a window narrowed until cauchy_data takes it (cauchy_of).
//
// Shift-parallel form (ricadi_set_exchange): every rank owns a fixed subset of the shift list -- fixed, because the
// per-shift setup, the Sherman-Morrison-Woodbury panels and the recycled solutions live with the owner -- and solves
// only its shifts of a sweep; one all-gather per sweep.  A failure in the OWNER-LOCAL work of a rank (per-shift
// setup: a singular block; its solves) must not leave the other ranks waiting in that all-gather: it is recorded in
// `fail` (guarded), the rank still takes part in the exchange -- with zero panels and its status word set --, and
// all ranks throw together once the words have gone round.  The words ride in the pressure rows of each rank's first
// solution panel (the recombination reads velocity rows only), so a sweep costs ONE collective.
//
// One sweep is the phases of run(), in that order; the members below them are what one phase leaves for the next.
struct SweepAdi {
  ricadi_ctx* const c;
  const double* const shifts;
  double* const dW;
  const ricadi_adi_params& prm;
  AdiStats& stt;
  const std::vector<CauchySet>& cycle;
  const hipStream_t st;
  const bool shard, words_fit;      // words_fit: the status words ride in the pressure rows
  const int ns, m, G, nv, world, rank;
  const size_t nm;
  std::vector<int32_t> owner;
  std::string fail;
  Tick tk;
  AdiStop stop;
  AsyncRecompress job;
  long it0 = 0;
  int zc_last = 0, steps = 0, sw = 0;
  std::vector<double> be, coef, hn, cpre, dpre;
  std::vector<int> bpre;
  std::vector<ShiftData*> sds;
  std::vector<GmresResult> res;
  CauchySet var;                    // Cauchy data of a sweep that is not one of the cycle's
  // the sweep in hand: its width and the blocks of it that stay; its Cauchy data; where solution g sits in the
  // buffer the recombination reads and this rank's g; this rank's solutions and all of them, slot-major
  int Gs = 0, kept = 0, per_rank = 0, nslot = 0, nmine = 0, nc = 0;
  bool stopped = false;
  const CauchySet* cs = nullptr;
  std::vector<int> slot_of, mine;
  double* usolve = nullptr;
  const double* ubase = nullptr;
  const double* hg = nullptr;       // residual rule: Gram matrix (nc x nc) of [W, E U_1, .., E U_nslot], pinned host
  double words[2] = {0.0, 0.0};     // this rank's status word (a member: the upload may outlive gather())

  // (after admissible_width: from here on device state is touched)
  SweepAdi(ricadi_ctx* ctx, const double* shifts_, int ns_, double* dW_, int m_, const ricadi_adi_params& prm_,
           AdiStats& stt_, int G_, const std::vector<CauchySet>& cycle_)
      : c(ctx), shifts(shifts_), dW(dW_), prm(prm_), stt(stt_), cycle(cycle_), st(ctx->st), shard(sharded(ctx)),
        words_fit((size_t)ctx->np * m_ >= 2), ns(ns_), m(m_), G(G_), nv(ctx->nv), world(shard ? ctx->xworld : 1),
        rank(shard ? ctx->xrank : 0), nm((size_t)ctx->n * m_), owner(ns_, 0),
        stop(ns_, prm_.adi_newZ_reltol, prm_.adi_res_reltol, prm_.adi_max_steps, adi_res_wanted(ctx, prm_)), job(ctx),
        be(G_, 1.0), sds(G_), res(G_) {
    if (shard && deal_shifts(shifts, ns, world, owner.data()) != RICADI_OK) throw HipError{"bad shift list"};
    ensure_work(c, m, G);
    tk = Tick();
  }

  void lap(double& acc) {
    if (c->sw.timing) {
      (void)hipStreamSynchronize(st);
      acc += tk.lap();
    }
  }
  // owner-local work: when sharded its failure is recorded in `fail` instead of thrown
  template <class F>
  void guarded(F&& body) { run_guarded(shard ? &fail : nullptr, body); }
  // row j of the coefficient table <- col[i * stride], i < cnt, replicated over the m columns, in buffer order
  void fill_row(int j, const double* col, int stride, int cnt) {
    for (int i = 0; i < cnt; ++i)
      for (int cidx = 0; cidx < m; ++cidx) coef[((size_t)j * nslot + slot_of[i]) * m + cidx] = col[(size_t)i * stride];
  }

  // this rank's shifts of the first pass set up, W projected (replicated: every rank sets the projection operator up)
  void prepare() {
    std::vector<double> own;
    for (int i = 0; i < std::min(ns, prm.adi_max_steps); ++i)
      if (owner[i] == rank) own.push_back(shifts[i]);
    setup_and_project(c, own.data(), (int)own.size(), prm.project_w != 0, dW, m, shard ? &fail : nullptr,
                      [&] { lap(c->t_setup); });
    lap(c->t_proj);
    it0 = c->total_iters;
    if (!shard) c->sweep_u.ensure(nm * G);
    c->sweep_t.ensure((size_t)nv * m);
    zc_last = c->zc;
  }

  // Cauchy data of the window of g shifts behind step `first`: an aligned full sweep is one of the cycle's; any other
  // window (a cut sweep and every sweep behind it) gets its data on the spot, narrowed -- g is updated -- where
  // cauchy_data refuses it (adi_window_width: halved down to one shift, which is always taken).  Host arithmetic on
  // the replicated shift list: every rank narrows alike.
  const CauchySet& cauchy_of(int first, int& g) {
    if (g == G && first % G == 0) return cycle[(first / G) % cycle.size()];
    g = adi_window_width(shifts, ns, first, g);
    if (!var.fill(shifts, ns, first, g)) throw HipError{"Cauchy matrix of a single-shift ADI sweep refused: bad shift"};
    return var;
  }

  // who solves what, and where solution g sits in the buffer the recombination reads
  void deal() {
    slot_of.assign(Gs, 0);
    mine.clear();
    // (not sharded: one rank that owns every shift)
    std::vector<int> cnt(world, 0);
    for (int g = 0; g < Gs; ++g) {
      const int r = owner[(steps + g) % ns];
      slot_of[g] = cnt[r]++;                       // index among its owner's items, completed below
      if (r == rank) mine.push_back(g);
    }
    per_rank = *std::max_element(cnt.begin(), cnt.end());
    for (int g = 0; g < Gs; ++g) slot_of[g] += owner[(steps + g) % ns] * per_rank;
    nslot = world * per_rank;
    nmine = (int)mine.size();
    nc = (nslot + 1) * m;
  }

  // this rank's solves of the sweep, all against the same W, in one lockstep batch
  void solve_share() {
    std::vector<double> psm(nmine);
    for (int k = 0; k < nmine; ++k) psm[k] = cs->ps[mine[k]];
    if (nmine && fail.empty()) guarded([&] { get_shifts(c, psm.data(), be.data(), nmine, sds.data()); });
    lap(c->t_setup);
    usolve = shard ? c->xsend : c->sweep_u.p;
    if (shard) {
      require_exchange_capacity(c, (size_t)per_rank * nm * sizeof(double));
      // padding slots travel as zeros (their coefficients are zero, but 0 * NaN is not)
      if (nmine < per_rank)
        HIPCHK(hipMemsetAsync(c->xsend + (size_t)nmine * nm, 0, sizeof(double) * nm * (per_rank - nmine), st));
    }
    if (nmine && fail.empty())
      guarded([&] {
        // test hook (tests/test_gpu_round4.py): this rank's share of sweep k fails
        if (const char* inj = shard ? getenv("RICADI_INJECT_SWEEP_FAILURE") : nullptr)
          if (atoi(inj) == sw) throw HipError{"injected failure in sweep " + std::to_string(sw)};
        load_rhs(c, dW, m, c->bvec.p);
        solve_batch(c, sds.data(), nmine, c->bvec.p, 0, usolve, m, true, nullptr, res.data());
      });
    c->lr_ucol = -1;            // only the first solve of a Newton step has U among its rhs columns
    lap(c->t_solve);
    if (fail.empty()) {
      for (int k = 0; k < nmine; ++k)
        if (!res[k].converged) {
          stt.nonconverged++;
          stt.worst_relres = std::max(stt.worst_relres, res[k].max_relres);
        }
      stt.shift_solves += nmine;
    }
  }

  // sharded: the sweep's one all-gather, this rank's status word with its panels
  void gather() {
    ubase = usolve;
    if (!shard) return;
    words[0] = fail.empty() ? 0.0 : 1.0;
    if (!fail.empty()) HIPCHK(hipMemsetAsync(c->xsend, 0, sizeof(double) * nm * per_rank, st));
    if (words_fit) {
      HIPCHK(hipMemcpyAsync(c->xsend + (size_t)nv * m, words, sizeof(words), hipMemcpyHostToDevice, st));
    } else {
      // no pressure rows to carry the words: a control message of their own
      double any = words[0];
      reduce_over_ranks(c, &any, 0, 1);
      if (any != 0.0) throw HipError{fail.empty() ? "another rank failed in its share of an ADI sweep" : fail};
    }
    exchange(c, (size_t)per_rank * nm);
    ubase = c->xrecv;
  }

  // Z <- [Z, U R^-1]: block j = sum_i rinv[i][j] U_i, with its squared norm; with the residual rule the Gram matrix
  // of [W, E U_1, .., E U_nslot] (launch_sweep_resid_panel, launch_gram_fixed: fixed summation order, so every rank
  // gets the same bits from the same gathered panels and decides alone).  One wait for all that the decisions need.
  void recombine() {
    // coefficient rows in buffer order: Gs columns of R^-1, then (advance_w) C^-1 1
    coef.assign((size_t)(Gs + 1) * nslot * m, 0.0);
    for (int j = 0; j < Gs; ++j) fill_row(j, cs->rinv.data() + j, Gs, Gs);
    c->sweep_coef.ensure(coef.size());
    HIPCHK(hipMemcpyAsync(c->sweep_coef.p, coef.data(), sizeof(double) * (size_t)Gs * nslot * m,
                          hipMemcpyHostToDevice, st));
    const bool combined = sweep_blocks(c, ubase, nm, nslot, Gs, m, c->sweep_coef.p, c->Z.p, c->zld, c->zc, c->nrm2.p);
    hn.resize((size_t)Gs * m);
    HIPCHK(hipMemcpyAsync(hn.data(), c->nrm2.p, sizeof(double) * Gs * m, hipMemcpyDeviceToHost, st));
    if (stop.res_on) {
      c->res_pan.ensure((size_t)nv * nc);
      c->res_part.ensure(gram_fixed_partial_len(nv, nc));
      c->res_gram.ensure((size_t)nc * nc);
      launch_sweep_resid_panel(st, nv, m, nslot, c->E.rp.p, c->E.ci.p, c->E.v.p, dW, ubase, nm, c->res_pan.p);
      launch_gram_fixed(st, nv, nc, c->res_pan.p, nc, c->res_part.p, c->res_gram.p);
      c->res_launches += 3;
      double* hgw = res_host(c, (size_t)nc * nc);
      hg = hgw;
      HIPCHK(hipMemcpyAsync(hgw, c->res_gram.p, sizeof(double) * nc * nc, hipMemcpyDeviceToHost, st));
    }
    std::vector<double> rwords;
    if (shard && words_fit) {
      // the ranks' status words, one strided copy out of the gathered buffer
      rwords.assign((size_t)2 * world, 0.0);
      HIPCHK(hipMemcpy2DAsync(rwords.data(), sizeof(double) * 2, c->xrecv + (size_t)nv * m,
                              sizeof(double) * nm * per_rank, sizeof(double) * 2, world, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (int r = 0; r < (int)rwords.size() / 2; ++r)
      if (rwords[(size_t)2 * r] != 0.0)
        throw HipError{r == rank && !fail.empty() ? fail
                                                  : "rank " + std::to_string(r) + " failed in its share of an ADI sweep"};
    // The block norms steer the stopping decisions, which must not differ between the ranks.  The fused
    // recombination sums in a fixed order (sweep_combine_kernel): every rank gets the same bits from the same
    // gathered panels and decides alone.  The per-block fallback hands round rank 0's values.
    if (!combined)
      for (int o = 0; o < Gs * m; o += RICADI_XCTL / 8)
        values_of_rank0(c, hn.data() + o, std::min(RICADI_XCTL / 8, Gs * m - o));
    // ||W_0^T W_0|| is the leading block of the first sweep's matrix
    if (stop.res_on && stop.res_rhs < 0.0) stop.res_rhs = gram_block_fro(hg, nc, m, 0);
  }

  // ||W_j^T W_j||_F of the residual factor after the first j + 1 blocks, W + sum_{i <= j} (C_{j+1}^-1 1)_i E U_i
  double prefix_residual(int j) {
    const double* cj = cs->cinv1.data();
    if (j + 1 < Gs) {
      cauchy_cinv_prefix(cs->ps.data(), j + 1, cpre);
      cj = cpre.data();
    }
    bpre.assign(j + 2, 0);
    dpre.assign(j + 2, 1.0);
    for (int i = 0; i <= j; ++i) {
      bpre[i + 1] = 1 + slot_of[i];
      dpre[i + 1] = cj[i];
    }
    return gram_combination_fro(hg, nc, m, bpre.data(), dpre.data(), j + 2);
  }

  // the rules, block by block; the blocks behind the stopping step are dropped
  void decide() {
    kept = Gs;
    stopped = false;
    for (int j = 0; j < Gs && !stopped; ++j) {
      double b2 = 0.0;
      for (int cc = 0; cc < m; ++cc) b2 += hn[(size_t)j * m + cc];
      const double wf = stop.res_on ? prefix_residual(j) : 0.0;
      const AdiStop::Verdict v = stop.record(steps + j, b2, stop.res_on ? &wf : nullptr);
      stt.rel = v.rel;
      if (stop.res_on) c->adi_res_hist.push_back(v.res);
      if (v.rule != RICADI_STOP_MAX_STEPS) {
        kept = j + 1;
        stopped = true;
        c->adi_stop_rule = v.rule;
      }
    }
  }

  // W <- W + E (U C^-1 1) over the blocks that are KEPT: every U_g was solved against the same W, so the first
  // `kept` solutions are the sweep of the first `kept` shifts, whose Cauchy data differ only in C^-1 1 -- W stays
  // the residual factor of the truncated Z, and ||W^T W|| the residual norm that is reported
  void advance_w() {
    const double* cw = cs->cinv1.data();
    if (kept < Gs) {
      cauchy_cinv_prefix(cs->ps.data(), kept, cpre);
      cw = cpre.data();
    }
    fill_row(Gs, cw, 1, kept);
    double* crow = c->sweep_coef.p + (size_t)Gs * nslot * m;
    HIPCHK(hipMemcpyAsync(crow, coef.data() + (size_t)Gs * nslot * m, sizeof(double) * (size_t)nslot * m,
                          hipMemcpyHostToDevice, st));
    launch_cols_update(st, nv, m, nslot, ubase, nm, crow, 1.0, nullptr, nullptr, c->sweep_t.p);
    launch_spmm(st, nv, c->E.rp.p, c->E.ci.p, c->E.v.p, c->sweep_t.p, m, nullptr, dW, m, dW, m, 1.0,
                1.0, nullptr, m);
    HIPCHK(hipStreamSynchronize(st));     // `coef` is reused by the next sweep
    c->zc += kept * m;
    steps += kept;
    stt.steps = steps;
    stt.sweeps = sw + 1;
    lap(c->t_recomb);
    const bool dbg = c->sw.debug_sweeps;
    if (!prm.verbose && !dbg) return;
    int its = 0;
    for (int k = 0; k < nmine; ++k) its = std::max(its, res[k].iters);
    if (dbg) {
      double wf = 0.0;
      gram_norms(c, dW, c->nv, m, &wf, nullptr);
      fprintf(stderr, "[ricadi rank %d] sweep %d: Gs %d kept %d per_rank %d nmine %d  ||W^T W|| %.6e  znorm2 %.6e  its", rank, sw + 1,
              Gs, kept, per_rank, nmine, wf, stop.znorm2);
      for (int k = 0; k < nmine; ++k) fprintf(stderr, " %d", res[k].iters);
      fprintf(stderr, "\n");
    }
    fprintf(stderr, "[ricadi] ADI sweep %3d (steps %d..%d): rel new Z %9.3e, gmres its <= %d%s\n",
            sw + 1, steps - kept + 1, steps, stt.rel, its, shard ? " (this rank)" : "");
  }

  void finish() {
    job.finish();
    lap(c->t_compress);
    stt.gmres_iters = c->total_iters - it0;
    if (shard) {
      // a rank has only seen its own solves
      double v[4] = {(double)stt.gmres_iters, (double)stt.shift_solves, (double)stt.nonconverged, stt.worst_relres};
      reduce_over_ranks(c, v, 3, 1);
      stt.gmres_iters = (long)(v[0] + 0.5);
      stt.shift_solves = (long)(v[1] + 0.5);
      stt.nonconverged = (long)(v[2] + 0.5);
      stt.worst_relres = v[3];
    }
    gram_norms(c, dW, c->nv, m, &stt.res_fro, nullptr);
  }

  void run() {
    prepare();
    for (;; ++sw) {
      Gs = stop.cut(steps, G);
      if (Gs < 1) break;
      cs = &cauchy_of(steps, Gs);
      deal();
      solve_share();
      gather();
      recombine();
      decide();
      advance_w();
      if (stopped || steps >= prm.adi_max_steps) break;
      if (prm.compress_cols > 0 && c->zc - zc_last >= prm.compress_cols) {
        // splice in what the helper finished during the last sweeps, hand it the next prefix
        job.finish();
        job.start();
        zc_last = c->zc;
        lap(c->t_compress);
      }
    }
    finish();
  }
};

// Returns false (nothing done) if the shift list does not allow sweeps.
static bool lyap_adi_sweeps_dev(ricadi_ctx* c, const double* shifts, int ns, double* dW, int m,
                                const ricadi_adi_params& prm, AdiStats& stt) {
  std::vector<CauchySet> cycle;
  const int G = admissible_width(shifts, ns, m, prm, cycle);
  if (G < 2) return false;
  SweepAdi(c, shifts, ns, dW, m, prm, stt, G, cycle).run();
  return true;
}

// Depth of the recycling ring inside the ADI drivers (RICADI_RECYCLE=d; 0 switches it off)
// (cfg2, same-call A/B: depth 0 / 2 / 3 / 5 / 8 -> 63.1 / 56.3 / 55.3 / 53.4 / 52.7 iterations per solve,
// 436.7 / 405.9 / 405.9 / 401.9 / 409.8 ms per step.)  Every stored pair costs n x m doubles per shift:
// 5 where that is small, 3 beyond n = 2e5 (cfg5: 128 shifts x 3 x 64 MB).
static int adi_recycle_depth(const ricadi_ctx* c) {
  const char* e = getenv("RICADI_RECYCLE");     // read per call: tests toggle it
  return e ? std::max(0, std::min(8, atoi(e))) : (c->n <= 200000 ? 5 : 3);
}

// What the step form fetches for the residual rule: res_gram holds W^T W before and after a step (2 m^2 doubles), `hg`
// is its pinned host copy.  Launches ||W_0^T W_0|| of the iteration; it is fetched in the first step's synchronisation.
static double* adi_res_begin(ricadi_ctx* c, const double* dW, int m) {
  c->res_part.ensure(gram_fixed_partial_len(c->nv, m));
  c->res_gram.ensure((size_t)2 * m * m);
  double* hg = res_host(c, (size_t)2 * m * m);
  launch_gram_fixed(c->st, c->nv, m, dW, m, c->res_part.p, c->res_gram.p);
  c->res_launches += 2;
  return hg;
}
// ... W^T W behind a step into the second half, both halves to `hg` (queued: the step's synchronisation fetches them)
static void adi_res_fetch(ricadi_ctx* c, const double* dW, int m, double* hg) {
  const int mm = m * m;
  launch_gram_fixed(c->st, c->nv, m, dW, m, c->res_part.p, c->res_gram.p + mm);
  c->res_launches += 2;
  HIPCHK(hipMemcpyAsync(hg, c->res_gram.p, sizeof(double) * 2 * mm, hipMemcpyDeviceToHost, c->st));
}

// One step at the real shift p: S(p) [V; *] = [W; 0], W <- W - 2 p E V, Z <- [Z, sqrt(-2p) V] at column c->zc (which the
// caller advances).  n2: the block's squared Frobenius norm; with `hg` the Gram matrices of adi_res_fetch are in it when
// the step returns (one synchronisation for both).
static GmresResult adi_real_step(ricadi_ctx* c, double p, double* dW, int m, double* hg, double& n2) {
  hipStream_t st = c->st;
  ShiftData* sd = get_shift(c, p, 1.0);
  load_rhs(c, dW, m, c->bvec.p);
  GmresResult r = gmres_solve(c, sd, c->bvec.p, c->xs.p, m, true, nullptr);
  // W <- W - 2 p E V
  launch_spmm(st, c->nv, c->E.rp.p, c->E.ci.p, c->E.v.p, c->xs.p, m, nullptr, dW, m, dW, m,
              -2.0 * p, 1.0, nullptr, m);
  // Z <- [Z, sqrt(-2p) V]
  launch_copy_cols(st, c->nv, m, c->xs.p, m, 0, c->Z.p, c->zld, c->zc, std::sqrt(-2.0 * p));
  col_norms2(c, c->xs.p, c->nv, m, c->nrm2.p);
  HIPCHK(hipMemcpyAsync(c->h_resid, c->nrm2.p, sizeof(double) * m, hipMemcpyDeviceToHost, st));
  if (hg) adi_res_fetch(c, dW, m, hg);
  HIPCHK(hipStreamSynchronize(st));
  n2 = 0.0;
  for (int j = 0; j < m; ++j) n2 += c->h_resid[j];
  n2 *= -2.0 * p;
  return r;
}

// Step form: one shift solve per step, S(p) [V; *] = [W; 0], then W <- W - 2 p E V and Z <- [Z, sqrt(-2p) V].
// dW: NV x m device panel (overwritten by the final residual factor); the blocks are appended to c->Z (ld = c->zld)
// starting at column c->zc.  Tries the sweep form first where sweep_width asks for it.  Both rules of AdiStop end the
// iteration; what it reports goes to c->adi_res_hist / c->adi_stop_rule.  On a sharded context every rank runs this
// form on its own solves and, with the residual evaluated, rank 0's verdict is handed round every step.
static AdiStats lyap_adi_dev(ricadi_ctx* c, const double* shifts, int ns, double* dW, int m,
                             const ricadi_adi_params& prm) {
  AdiStats stt;
  Restore<int> keep_rec(c->rec_depth);
  c->rec_depth = std::max(c->rec_user_depth, adi_recycle_depth(c));
  c->adi_res_hist.clear();
  c->adi_stop_rule = RICADI_STOP_MAX_STEPS;
  c->adi_ran = true;
  if (prm.sweep_width > 1 && lyap_adi_sweeps_dev(c, shifts, ns, dW, m, prm, stt)) return stt;
  stt = AdiStats();
  ensure_work(c, m);
  // per-shift data of the whole shift cycle (and of the projection) up front: the coarse
  // inverses then come out of one batched factorisation instead of one at a time
  setup_and_project(c, shifts, std::min(ns, prm.adi_max_steps), prm.project_w != 0, dW, m);
  const long it0 = c->total_iters;
  int zc_last = c->zc;
  // Residual rule: W^T W after every step (fixed-order Gram kernel), fetched with the block norms.  ||W_0^T W_0||
  // is launched here and fetched in the first step's synchronisation.
  AdiStop stop(ns, prm.adi_newZ_reltol, prm.adi_res_reltol, prm.adi_max_steps, adi_res_wanted(c, prm));
  const int mm = m * m;
  double* hg = stop.res_on ? adi_res_begin(c, dW, m) : nullptr;
  for (int step = 1; step <= prm.adi_max_steps; ++step) {
    const double p = shifts[(step - 1) % ns];
    double n2 = 0.0, wf = 0.0;
    GmresResult r = adi_real_step(c, p, dW, m, hg, n2);
    if (!r.converged) {
      stt.nonconverged++;
      stt.worst_relres = std::max(stt.worst_relres, r.max_relres);
      if (prm.verbose)
        fprintf(stderr, "[ricadi] ADI step %d shift %g: GMRES stopped at relres %.2e after %d its\n",
                step, p, r.max_relres, r.iters);
    }
    stt.shift_solves++;
    if (stop.res_on) {
      if (stop.res_rhs < 0.0) stop.res_rhs = gram_block_fro(hg, m, m, 0);
      wf = gram_block_fro(hg + mm, m, m, 0);
    }
    AdiStop::Verdict v = stop.record(step - 1, n2, stop.res_on ? &wf : nullptr);
    c->zc += m;
    stt.steps = step;
    stt.rel = v.rel;
    if (prm.verbose)
      fprintf(stderr, "[ricadi] ADI step %3d: shift %10.3e rel new Z %9.3e gmres its %d\n", step,
              p, stt.rel, r.iters);
    if (stop.res_on) {
      // (sharded: every rank runs this form on its own solves, whose last bits differ; rank 0's residual and the
      // rule it found go round, so that the ranks report the same history and end together)
      double dec[2] = {v.res, (double)v.rule};
      values_of_rank0(c, dec, 2);
      v.rule = (int)dec[1];
      c->adi_res_hist.push_back(dec[0]);
    }
    if (v.rule != RICADI_STOP_MAX_STEPS) {
      c->adi_stop_rule = v.rule;
      break;
    }
    if (prm.compress_cols > 0 && c->zc - zc_last >= prm.compress_cols) {
      factor_recompress(c);
      zc_last = c->zc;
    }
  }
  stt.gmres_iters = c->total_iters - it0;
  gram_norms(c, dW, c->nv, m, &stt.res_fro, nullptr);
  return stt;
}

static void factor_reserve(ricadi_ctx* c, int ld) {
  if ((size_t)c->nv * ld > c->Z.n) c->Z.alloc((size_t)c->nv * ld);
  c->zld = ld;
  c->zc = 0;
}

