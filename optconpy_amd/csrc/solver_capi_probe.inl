// solver_capi_probe.inl -- the C-ABI of include/ricadi.h: the entry points written for the tests (single stages of the
// solver on its own workspace, its structure, its counters).
// Part of ricadi_solver.hip (one translation unit; included there in order).

namespace {
// The batch, the iteration form and the cycle form of a probe cycle, decided as for a solve
BatchSetup probe_setup(ricadi_ctx* c, int ng, const double* alphas, const double* betas, int m) {
  BatchSetup p(c, ng, alphas, betas, m, BatchSetup::kWorkPlain, BatchSetup::kCycle);
  c->w32_last = p.f.w32 ? 1 : 0;
  return p;
}
// ... of the last begin (step, close, read)
BatchSetup probe_setup(ricadi_ctx* c) {
  return probe_setup(c, c->probe.ng, c->probe.alpha.data(), c->probe.beta.data(), c->probe.m);
}
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

extern "C" {

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
  if (int rc = check_batch(c, ng, m)) return rc;
  REQUIRE(dR && dZ && alphas && betas, RICADI_EINVAL, "NULL argument");
  REQUIRE(r_stride >= (int64_t)c->n * m, RICADI_EINVAL, "bad r_stride");
  std::vector<int> ids;
  if (int rc = active_ids(active, nactive, ng, ids)) return rc;
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  // the forms gmres_core applies the preconditioner in (same question, same answer)
  BatchSetup s(c, ng, alphas, betas, m, BatchSetup::kWorkPlain, BatchSetup::kCycle, (size_t)r_stride);
  Batch& bt = s.bt;
  const IterationForm& f = s.f;
  const CycleForm& pf = s.pf;
  if (active) bt.set(ids);
  const size_t nm = bt.gs, vs = nm * ng;
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
  precond_apply(c, bt, pf, CycleIO{r, gsr, r16, z, z32, nm});
  if (f.x32)
    for (int i = 0; i < bt.tab.ng; ++i) {
      const size_t g = (size_t)bt.tab.gid[i];
      probe_widen(c, z32 + g * nm, 4, nm, dZ + g * nm);
    }
  HIPCHK(hipStreamSynchronize(st));
  if (form_out) *form_out = (int)pf.word();
  API_END
}

int ricadi_op_apply_batch_dev(ricadi_ctx* c, int ng, const double* alphas, const double* betas, const double* dX,
                              int64_t x_stride, int m, const int32_t* active, int nactive, int flags, double alpha,
                              const double* dR, int64_t r_stride, double beta_r, double* dY, int64_t y_stride,
                              int* variant_out) {
  if (int rc = check_batch(c, ng, m)) return rc;
  REQUIRE(dX && dY && alphas && betas, RICADI_EINVAL, "NULL argument");
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
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  BatchSetup s(c, ng, alphas, betas, m, BatchSetup::kWorkPlain);
  Batch& bt = s.bt;
  if (active) bt.set(ids);
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
  if (y32)
    for (int i = 0; i < bt.tab.ng; ++i) {
      const size_t g = (size_t)bt.tab.gid[i];
      probe_widen(c, yf.p + g * y_stride, 4, (size_t)nm, dY + g * y_stride);
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
  API_BEGIN_ON(c)
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
  API_BEGIN_ON(c)
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

// ---- step probe of the Arnoldi phase (tests) -------------------------------------------------------------------
// The units the lockstep GMRES is made of -- cycle_start_launches, arnoldi_launches, cycle_end_launches of
// solver_gmres.inl -- one call each on the solver's own workspace, with the batch, the iteration form and the cycle
// form decided as for a solve, and the workspace read back in FP64.  The preconditioner and the operator are not run:
// the caller supplies w.  Synchronous.
int ricadi_arnoldi_probe_begin_dev(ricadi_ctx* c, int ng, const double* alphas, const double* betas, int m,
                                   const double* dR, const double* dBnorm) {
  if (int rc = check_batch(c, ng, m)) return rc;
  REQUIRE(alphas && betas && dR && dBnorm, RICADI_EINVAL, "bad argument");
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  c->probe = ricadi_ctx::ArnoldiProbe();
  BatchSetup p = probe_setup(c, ng, alphas, betas, m);
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
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  BatchSetup p = probe_setup(c);
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
  API_BEGIN_ON(c)
  hipStream_t st = c->st;
  BatchSetup p = probe_setup(c);
  GroupInts kk = same_int(0);
  for (int g = 0; g < c->probe.ng; ++g) kk.v[g] = ks[g];
  HIPCHK(hipMemcpyAsync(c->zbasisf.p, dZ, sizeof(float) * (size_t)nz * p.bt.gs * c->probe.ng, hipMemcpyDeviceToDevice,
                        st));
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
  API_BEGIN_ON(c)
  BatchSetup p = probe_setup(c);
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
  API_BEGIN_ON(c)
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

// the dense part of one RADI step (radi_dense_step), synchronous
int ricadi_radi_update_dev(ricadi_ctx* c, double p, const double* dV, int ldv, int m, const double* dB, int nb,
                           double* dRU, double* dZblk, int ldz, int zoff, double* dG_out, double* dC_out) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(dV && dB && dRU && dZblk && dG_out, RICADI_EINVAL, "NULL argument");
  REQUIRE(m >= 1 && m <= 127 && nb >= 1 && nb <= 64 && p < 0.0, RICADI_EINVAL, "1 <= m <= 127, 1 <= nb <= 64, p < 0 required");
  REQUIRE(ldv >= m && zoff >= 0 && ldz >= zoff + m, RICADI_EINVAL, "bad leading dimension");
  int flag = 0;
  API_BEGIN_ON(c)
  TArr<double> dC(c->pool), dPart(c->pool, radi_vtb_partial_len(c->nv, m, nb));
  if (!dC_out) dC.alloc((size_t)m * (2 * m + nb));
  int* dflag = c->flag.p + 3;
  radi_dense_step(c, p, dV, ldv, m, dB, nb, dRU, dZblk, ldz, zoff, dG_out, dC_out ? dC_out : dC.p, dPart.p, dflag);
  HIPCHK(hipMemcpyAsync(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost, c->st));
  HIPCHK(hipStreamSynchronize(c->st));
  API_END_STATUS(flag ? (ricadi::set_error(RADI_BREAKDOWN_MSG), RICADI_EBREAKDOWN) : RICADI_OK)
}

// the recombination of a RADI sweep (launch_radi_sweep_combine), synchronous
int ricadi_radi_sweep_combine_dev(ricadi_ctx* c, int G, const double* dV, int64_t vstride, int ldv, int m,
                                  const double* dS, const double* dCf, int k, int nb, double* dRU, double* dZblk,
                                  int ldz, int zoff) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(dV && dS && dCf && dRU && dZblk, RICADI_EINVAL, "NULL argument");
  REQUIRE(G >= 1 && G <= RICADI_MAX_GROUPS && m >= 1 && G * m <= RICADI_RADI_SWEEP_MAX_K && k >= 1 && k <= G && nb >= 1 &&
              nb <= 64,
          RICADI_EINVAL, "1 <= G <= 16, G m <= 128, 1 <= k <= G, 1 <= nb <= 64 required");
  REQUIRE(ldv >= m && zoff >= 0 && ldz >= zoff + k * m && (G == 1 || vstride >= (int64_t)c->nv * ldv), RICADI_EINVAL,
          "bad leading dimension or stride");
  API_BEGIN_ON(c)
  launch_radi_sweep_combine(c->st, c->nv, G, m, nb, k, dV, (size_t)vstride, ldv, dS, G * m, dCf, dRU, dZblk, ldz, zoff);
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

// the reduced matrices of the shift selection (launch_radi_reduce), synchronous
int ricadi_radi_reduce_dev(ricadi_ctx* c, const double* dQ, int k, const double* dRU, int m, const double* dB, int nb,
                           double* dH_out) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(dQ && dRU && dB && dH_out, RICADI_EINVAL, "NULL argument");
  REQUIRE(k >= 1 && k <= 32 && m >= 1 && m <= 32 && nb >= 1 && nb <= 64, RICADI_EINVAL,
          "1 <= k <= 32, 1 <= m <= 32, 1 <= nb <= 64 required");
  API_BEGIN_ON(c)
  TArr<double> part(c->pool, radi_reduce_partial_len(c->nv, k, m, nb));
  launch_radi_reduce(c->st, c->nv, k, m, nb, c->s_rp.p, c->s_ci.p, c->srcA.p, c->srcE.p, dQ, dRU, dB, part.p, dH_out);
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

// the same on the wide kernel (launch_radi_reduce above 32 columns), synchronous
int ricadi_radi_reduce_wide_dev(ricadi_ctx* c, const double* dQ, int k, const double* dRU, int m, const double* dB,
                                int nb, double* dH_out) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(dQ && dRU && dB && dH_out, RICADI_EINVAL, "NULL argument");
  REQUIRE(k == m && m >= 33 && m <= 127 && nb >= 1 && nb <= 64, RICADI_EINVAL,
          "k = m, 33 <= m <= 127, 1 <= nb <= 64 required");
  API_BEGIN_ON(c)
  TArr<double> part(c->pool, radi_reduce_partial_len(c->nv, k, m, nb));
  launch_radi_reduce(c->st, c->nv, k, m, nb, c->s_rp.p, c->s_ci.p, c->srcA.p, c->srcE.p, dQ, dRU, dB, part.p, dH_out);
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

// the same for the group of blocks a sweep kept: c columns of Q against an m-column residual
int ricadi_radi_reduce_group_dev(ricadi_ctx* c, const double* dQ, int cq, const double* dRU, int m, const double* dB,
                                 int nb, double* dH_out) {
  REQUIRE(c && c->has_op, RICADI_ESTATE, "set the operator first");
  REQUIRE(dQ && dRU && dB && dH_out, RICADI_EINVAL, "NULL argument");
  REQUIRE(cq >= 1 && cq <= 127 && m >= 1 && m <= 127 && nb >= 1 && nb <= 64 && (cq > 32 || m <= 32) &&
              2 * cq + m + 2 * nb <= 509,
          RICADI_EINVAL, "1 <= c, m <= 127 (m <= 32 where c <= 32), 1 <= nb <= 64, 2c + m + 2nb <= 509 required");
  API_BEGIN_ON(c)
  TArr<double> part(c->pool, radi_reduce_partial_len(c->nv, cq, m, nb));
  launch_radi_reduce(c->st, c->nv, cq, m, nb, c->s_rp.p, c->s_ci.p, c->srcA.p, c->srcE.p, dQ, dRU, dB, part.p, dH_out);
  HIPCHK(hipStreamSynchronize(c->st));
  API_END
}

int ricadi_probe_cache_entries(ricadi_ctx* c, int* n_out) {
  REQUIRE(c && n_out, RICADI_EINVAL, "NULL argument");
  size_t n = 0;
  for (const ricadi_ctx* l = c; l; l = l->child.get()) n += l->cache.size();
  *n_out = (int)n;
  return RICADI_OK;
}

// branches of the RADI driver (ric_radi_run): the steps after which the selection counts as refused, and what the
// last call counted
int ricadi_probe_radi_refuse(ricadi_ctx* c, const int* steps, int n) {
  REQUIRE(c && n >= 0 && (steps || n == 0), RICADI_EINVAL, "bad argument");
  for (int i = 0; i < n; ++i) REQUIRE(steps[i] >= 1, RICADI_EINVAL, "steps are counted from 1");
  c->radi_refuse.assign(steps, steps + n);
  return RICADI_OK;
}
int ricadi_probe_radi_counters(ricadi_ctx* c, int* out) {
  REQUIRE(c && out, RICADI_EINVAL, "NULL argument");
  REQUIRE(c->radi_ran, RICADI_ESTATE, "no RADI iteration has run on this context");
  out[0] = c->radi_qr_repeats;
  out[1] = c->radi_recompressions;
  return RICADI_OK;
}
int ricadi_probe_radi_kept(ricadi_ctx* c, int* out, int cap, int* n_out) {
  REQUIRE(c && n_out && cap >= 0 && (out || cap == 0), RICADI_EINVAL, "bad argument");
  REQUIRE(c->radi_ran, RICADI_ESTATE, "no RADI iteration has run on this context");
  const int n = (int)c->radi_kept_hist.size();
  *n_out = n;
  for (int i = 0; i < std::min(n, cap); ++i) out[i] = c->radi_kept_hist[i];
  return RICADI_OK;
}

}  // extern "C"
