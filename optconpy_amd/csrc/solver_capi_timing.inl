// solver_capi_timing.inl -- the C-ABI of include/ricadi.h: the benchmark's timers (launches of the solver's own kernels
// on its own workspace, timed with HIP events).
// Part of ricadi_solver.hip (one translation unit; included there in order).

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

int ricadi_time_spmm_dev(ricadi_ctx* c, double alpha, double beta, const double* dX, int m,
                         double* dY, int reps, double* ms_per_launch) {
  if (int rc = check_panel(c, m)) return rc;
  REQUIRE(dX && dY && reps > 0 && ms_per_launch, RICADI_EINVAL, "bad argument");
  API_BEGIN_ON(c)
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
  API_BEGIN_ON(c)
  // the saddle SpMM exactly as the batched GMRES launches it (no low-rank term; on the FP32-stored vector
  // when the iteration does so, and into an FP32 panel when its Arnoldi passes read one: dY is then left alone).
  // The basis storage is the one the solver's workspace will have (no workspace may exist yet).
  Restore<bool> keep16(c->basis16);
  c->basis16 = basis16_default(c);
  const BatchSetup s(c, ng, alphas, betas, m, BatchSetup::kNoWork, BatchSetup::kIteration);
  const Batch& bt = s.bt;
  const IterationForm& f = s.f;
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
  if (int rc = check_batch(c, ng, m)) return rc;
  REQUIRE(alphas && betas && reps > 0 && ms_per_launch, RICADI_EINVAL, "bad argument");
  REQUIRE(nvec >= 1 && nvec <= c->opts.gmres_restart, RICADI_EINVAL, "1 <= nvec <= gmres_restart required");
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  // the iteration form, and the preconditioner cycle on the workspace panels in the form gmres_core decides
  BatchSetup s(c, ng, alphas, betas, m, BatchSetup::kWorkPlain, BatchSetup::kCycle);
  Batch& bt = s.bt;
  const IterationForm& f = s.f;
  const CycleForm& pf = s.pf;
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
  const CycleIO io{c->wv.p, nm, Vh, c->zv.p, c->zbasisf.p, nm};
  auto launch = [&]() {
    switch (which) {
      case RICADI_TK_SPMM:
        op_apply(c, bt, c->zv.p, nm, c->wv.p, false, f.x32 ? c->zbasisf.p : nullptr, f.w32 ? c->wv32.p : nullptr);
        break;
      case RICADI_TK_BLOCK_V:
        block_sweep(c, bt, false, c->r2.p, nm, c->zv.p, 0);
        break;
      case RICADI_TK_BLOCK_P:
        if (c->nbp <= 0) throw HipError{"no pressure block"};
        block_sweep(c, bt, true, c->tp.p, bt.gsp, c->zv.p + (size_t)c->nv * m, 0);
        break;
      case RICADI_TK_COARSE:
        if (c->kc <= 0) throw HipError{"no coarse level"};
        {
          // the dense inverse lives on the last level
          Batch lb = bt;
          ricadi_ctx* lc = walk_levels(c, lb, [](const ricadi_ctx* l) { return !l->child; });
          pc_coarse(lc, lb, cycle_form(lc, m, lb.blocks16, 0, false, false), CycleIO());
        }
        break;
      case RICADI_TK_SPMM_SY:
        if (!c->syb_ok) throw HipError{"no tiled S*Y"};
        sy_residual_tiled(c, bt, c->wv.p, nm);
        break;
      // one-reduction form: 5 = its dots (with the reduction), 6 = the end-of-cycle pass, 7 = its update (iteration
      // nvec - 1)
      case RICADI_TK_DOTS:
        if (f.lowsync) arnoldi_lowsync_dots(c, bt, same_int(nvec - 1), false);
        else arnoldi_dots(c, f, bt, nvec);
        break;
      case RICADI_TK_UPDATE_DOTS:
        if (f.lowsync) arnoldi_lowsync_dots(c, bt, same_int(nvec), true);
        else arnoldi_update_dots(c, f, bt, nvec);
        break;
      case RICADI_TK_UPDATE:
        if (f.lowsync) arnoldi_lowsync_update(c, bt, nvec - 1, nullptr);
        else arnoldi_update(c, f, bt, nvec, nullptr);
        break;
      case RICADI_TK_PRECOND:
        precond_apply(c, bt, pf, io);
        break;
      case RICADI_TK_RESTRICT:
        if (c->kc <= 0) throw HipError{"no coarse level"};
        restrict_csr(c, bt, c->wv.p, nm);
        break;
      case RICADI_TK_PC_STAGE0 + 0: case RICADI_TK_PC_STAGE0 + 1: case RICADI_TK_PC_STAGE0 + 2:
      case RICADI_TK_PC_STAGE0 + 3: case RICADI_TK_PC_STAGE0 + 4: case RICADI_TK_PC_STAGE0 + 5:
      case RICADI_TK_PC_STAGE0 + 6:
        // ONE stage of the preconditioner application, the function precond_apply itself calls
        cycle_begin(c, pf, io);
        cycle_stages[which - RICADI_TK_PC_STAGE0](c, bt, pf, io);
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

int ricadi_time_qr_dev(ricadi_ctx* c, const double* dZ, int cz, int reps, double* ms_per_call) {
  REQUIRE(c && c->nv > 0 && dZ && cz > 0 && cz <= c->nv && reps > 0 && ms_per_call, RICADI_EINVAL,
          "bad argument");
  API_BEGIN_ON(c)
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
  API_BEGIN_ON(c)
  HIPCHK(hipMemsetAsync(dG, 0, sizeof(double) * cz * cz, c->st));
  *ms_per_launch = timed_ms(c->st, reps, [&] { launch_gemm_tn(c->st, c->nv, cz, cz, dZ, cz, dZ, cz, dG, cz); });
  API_END
}

}  // extern "C"
