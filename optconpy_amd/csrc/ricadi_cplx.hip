// ricadi_cplx.hip -- kernels of the complex-shift path: the saddle product
//     y = S(ar + i ai, beta) x,   S(alpha, beta) = [[beta A + alpha E, J^T], [J, 0]],
// on complex panels, and the Arnoldi kernels of the complex flexible GMRES on an FP64-stored basis.
//
// A complex panel of mc columns is the real row-major panel of m2 = 2 mc columns with the real parts in the even
// columns; m2 <= 16, so a panel row is one 16-lane row group as in the real kernels.  Lane g of a row group owns real
// column g -- the real part of complex column g >> 1 for even g, the imaginary part for odd g -- and reads its partner
// column g ^ 1 of the same row.  Every sum runs in a fixed order and nothing is accumulated with atomics: the same
// inputs give bitwise the same outputs.
#include "ricadi_device.h"

namespace ricadi {

// ---------------------------------------------------------------------------
// K1c, CSR form: one 16-lane row group per saddle row, the row's entries one after the other.  Per entry the complex
// coefficient is (beta vA + ar vE + vJ) + i (ai vE) from the three value sources of the unified saddle pattern (vJ
// and the pair (vA, vE) have disjoint supports); lane g adds  re * x[g] -/+ im * x[g ^ 1].
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cplx_spmm_csr_kernel(int nrows, const int* __restrict__ rp,
                                                            const int* __restrict__ ci, const double* __restrict__ vA,
                                                            const double* __restrict__ vE, const double* __restrict__ vJ,
                                                            GroupTab gt, CplxCoefs cf, const double* __restrict__ x,
                                                            size_t gsx, double* __restrict__ y, size_t gsy, int m2) {
  const int row = blockIdx.x * 16 + (threadIdx.x >> 4), g = threadIdx.x & 15;
  if (row >= nrows || g >= m2) return;
  const int grp = gt.gid[blockIdx.z];
  const double ar = cf.ar[grp], ai = cf.ai[grp], be = cf.beta[grp];
  const double sg = (g & 1) ? 1.0 : -1.0;
  const double* __restrict__ xg = x + (size_t)grp * gsx;
  double acc = 0.0;
  const int k1 = rp[row + 1];
  for (int k = rp[row]; k < k1; ++k) {
    const double e = vE[k];
    const double re = fma(ar, e, be * vA[k]) + vJ[k], im = sg * (ai * e);
    const size_t o = (size_t)ci[k] * m2;
    acc = fma(re, xg[o + g], acc);
    acc = fma(im, xg[o + (g ^ 1)], acc);
  }
  y[(size_t)grp * gsy + (size_t)row * m2 + g] = acc;
}

void launch_cplx_spmm_csr(hipStream_t st, const GroupTab& gt, const CplxCoefs& cf, int nrows, const int* rp,
                          const int* ci, const double* vA, const double* vE, const double* vJ, const double* x,
                          size_t gsx, double* y, size_t gsy, int m2) {
  if (nrows <= 0 || gt.ng <= 0) return;
  hipLaunchKernelGGL(cplx_spmm_csr_kernel, dim3((nrows + 15) / 16, 1, gt.ng), dim3(256), 0, st, nrows, rp, ci, vA, vE,
                     vJ, gt, cf, x, gsx, y, gsy, m2);
}

// ---------------------------------------------------------------------------
// K1c, tiled form, on the tile format of the multi-shift kernel (spmm_blocked_ms_kernel): one workgroup per 32-row
// block serves all active groups.  The block's slice of vAJ / vE and its 16-bit local indices (velocity-velocity flag
// in bit 15) are loaded into registers once -- lane g of a row group holds entries g, 16 + g, 32 + g of its row --, the
// groups are then walked one after the other: the x rows of the block's column list go to ONE LDS tile of max_cols x 16
// doubles (half the real kernel's two), and every entry is broadcast inside its row group and multiplied with the
// lane's own column and with its partner column of the same tile row.  Rows longer than 48 entries stream the rest.
// grid.y splits the active groups as in the real kernel.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cplx_spmm_tiled_kernel(const int* __restrict__ rows2, const int* __restrict__ rp2,
                                                              const int* __restrict__ cols2,
                                                              const uint16_t* __restrict__ lidx, GroupTab gt,
                                                              CplxCoefs cf, const double* __restrict__ vAJ,
                                                              const double* __restrict__ vE, const double* __restrict__ x,
                                                              size_t gsx, double* __restrict__ y, size_t gsy, int m2,
                                                              int max_cols) {
  extern __shared__ double tile[];   // max_cols x 16
  const int b = blockIdx.x;
  const int g = threadIdx.x & 15, gq = threadIdx.x >> 4;
  const int* __restrict__ bcols = cols2 + (size_t)b * max_cols;
  constexpr int NR = 2, NCH = 3;
  int ka[NR], kb[NR], grow[NR];
  double mAJ[NR][NCH], mE[NR][NCH];
  int myl[NR][NCH];
#pragma unroll
  for (int rr = 0; rr < NR; ++rr) {
    const int q = gq + 16 * rr;
    ka[rr] = rp2[b * 33 + q];
    kb[rr] = rp2[b * 33 + q + 1];
    grow[rr] = rows2[b * 32 + q];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int k = ka[rr] + ch * 16 + g;
      const bool ok = k < kb[rr];
      mAJ[rr][ch] = ok ? vAJ[k] : 0.0;
      mE[rr][ch] = ok ? vE[k] : 0.0;
      myl[rr][ch] = ok ? (int)lidx[k] : 0;
    }
  }
  const bool on = g < m2;
  const double sg = (g & 1) ? 1.0 : -1.0;
  for (int gi = blockIdx.y; gi < gt.ng; gi += gridDim.y) {
    const int grp = gt.gid[gi];
    const double ar = cf.ar[grp], ai = cf.ai[grp], be = cf.beta[grp];
    const double* __restrict__ xg = x + (size_t)grp * gsx;
    __syncthreads();                   // everybody is done with the previous group's tile
    for (int j = gq; j < max_cols; j += 16) {
      const int c = bcols[j];
      tile[j * 16 + g] = (c >= 0 && on) ? xg[(size_t)c * m2 + g] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < NR; ++rr) {
      const int len = kb[rr] - ka[rr];   // uniform in the row group
      double acc = 0.0;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const int cnt = min(16, len - ch * 16);
        if (cnt > 0) {
          const int l = myl[rr][ch];
          const double re_l = fma(ar, mE[rr][ch], ((l & 0x8000) ? be : 1.0) * mAJ[rr][ch]);
          const double im_l = ai * mE[rr][ch];
          const int slot_l = (l & 0x7fff) * 16;
          for (int t = 0; t < cnt; ++t) {
            const double re = __shfl(re_l, t, 16), im = sg * __shfl(im_l, t, 16);
            const int sl = __shfl(slot_l, t, 16);
            acc = fma(re, tile[sl + g], acc);
            acc = fma(im, tile[sl + (g ^ 1)], acc);
          }
        }
      }
      for (int k = ka[rr] + NCH * 16; k < kb[rr]; ++k) {
        const int l = (int)lidx[k];
        const double e = vE[k];
        const double re = fma(ar, e, ((l & 0x8000) ? be : 1.0) * vAJ[k]), im = sg * (ai * e);
        const int sl = (l & 0x7fff) * 16;
        acc = fma(re, tile[sl + g], acc);
        acc = fma(im, tile[sl + (g ^ 1)], acc);
      }
      if (grow[rr] >= 0 && on) y[(size_t)grp * gsy + (size_t)grow[rr] * m2 + g] = acc;
    }
  }
}

bool cplx_spmm_tiled_ok(int max_cols, size_t panel_rows) {
  return max_cols >= 1 && max_cols <= 160 && panel_rows * 16 * 8 < ((size_t)1 << 31);
}
void launch_cplx_spmm_tiled(hipStream_t st, const GroupTab& gt, const CplxCoefs& cf, int nblk, const int* rows2,
                            const int* rp2, const int* cols2, const uint16_t* lidx, const double* vAJ, const double* vE,
                            const double* x, size_t gsx, double* y, size_t gsy, int m2, int max_cols) {
  if (nblk <= 0 || gt.ng <= 0) return;
  int ysplit = 1;
  while (ysplit < gt.ng && (long)nblk * ysplit < 900 && ysplit < 8) ysplit *= 2;
  const size_t lds = (size_t)max_cols * 16 * sizeof(double);
  hipLaunchKernelGGL(cplx_spmm_tiled_kernel, dim3(nblk, std::min(ysplit, gt.ng), 1), dim3(256), lds, st, rows2, rp2,
                     cols2, lidx, gt, cf, vAJ, vE, x, gsx, y, gsy, m2, max_cols);
}

// ---------------------------------------------------------------------------
// K3c: the Arnoldi passes.  A workgroup of 256 threads (16 row slots x 16 lanes) owns CX_ROWS = 128 consecutive rows,
// eight per thread, held in registers across the basis vectors.
// ---------------------------------------------------------------------------
constexpr int CX_ROWS = 128, CX_RPT = 8, CX_JCH = 32;
int cplx_num_blocks(int nrows) { return std::max(1, (nrows + CX_ROWS - 1) / CX_ROWS); }

// partial[grp][blk][j][16] = this workgroup's share of  v_j^H w  (j < nvec; even lane: real part, odd lane: imaginary
// part) and, with want_self, of ||w||^2 per complex column at j = nvec (even lane; the odd one holds 0).  Inside a
// workgroup the row slots are summed by two butterfly steps and the four waves in wave order.
__global__ __launch_bounds__(256) void cplx_dots_kernel(GroupTab gt, int n, int m2, int nvec, int want_self,
                                                        const double* __restrict__ V, size_t vstride, size_t gsv,
                                                        const double* __restrict__ w, size_t gsw,
                                                        double* __restrict__ partial, int ldp) {
  __shared__ double sm[CX_JCH][4][16];
  const int grp = gt.gid[blockIdx.z];
  const int g = threadIdx.x & 15, s = threadIdx.x >> 4, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.x * CX_ROWS;
  const bool on = g < m2, odd = g & 1;
  const double* __restrict__ wg = w + (size_t)grp * gsw;
  double wo[CX_RPT], wp[CX_RPT];
#pragma unroll
  for (int i = 0; i < CX_RPT; ++i) {
    const int row = r0 + s + 16 * i;
    const bool ok = on && row < n;
    wo[i] = ok ? wg[(size_t)row * m2 + g] : 0.0;
    wp[i] = ok ? wg[(size_t)row * m2 + (g ^ 1)] : 0.0;
  }
  const int ntot = nvec + (want_self ? 1 : 0);
  double* __restrict__ pout = partial + ((size_t)grp * gridDim.x + blockIdx.x) * ldp * 16;
  for (int j0 = 0; j0 < ntot; j0 += CX_JCH) {
    const int jn = min(CX_JCH, ntot - j0);
    for (int jj = 0; jj < jn; ++jj) {
      const int j = j0 + jj;
      double acc = 0.0;
      if (j < nvec) {
        const double* __restrict__ vj = V + (size_t)j * vstride + (size_t)grp * gsv;
#pragma unroll
        for (int i = 0; i < CX_RPT; ++i) {
          const int row = r0 + s + 16 * i;
          if (on && row < n) {
            const double vo = vj[(size_t)row * m2 + g], vp = vj[(size_t)row * m2 + (g ^ 1)];
            // even: v_re w_re + v_im w_im;  odd (own = imaginary part): v_re w_im - v_im w_re
            acc = odd ? fma(vp, wo[i], fma(-vo, wp[i], acc)) : fma(vo, wo[i], fma(vp, wp[i], acc));
          }
        }
      } else if (!odd) {
#pragma unroll
        for (int i = 0; i < CX_RPT; ++i) acc = fma(wo[i], wo[i], fma(wp[i], wp[i], acc));
      }
      acc += __shfl_xor(acc, 16, 64);
      acc += __shfl_xor(acc, 32, 64);
      if ((threadIdx.x & 63) < 16) sm[jj][wave][g] = acc;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < jn * 16; idx += 256) {
      const int jj = idx >> 4, gg = idx & 15;
      pout[(size_t)(j0 + jj) * 16 + gg] = ((sm[jj][0][gg] + sm[jj][1][gg]) + sm[jj][2][gg]) + sm[jj][3][gg];
    }
    __syncthreads();
  }
}

// out[grp][idx] = sum over the row blocks, in block order, of partial[grp][blk][idx]  (idx < cnt * 16)
__global__ __launch_bounds__(256) void cplx_reduce_kernel(GroupTab gt, int nblk, int cnt, int ldp,
                                                          const double* __restrict__ partial, double* __restrict__ out,
                                                          size_t gso) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= cnt * 16) return;
  const int grp = gt.gid[blockIdx.z];
  const double* __restrict__ p = partial + (size_t)grp * nblk * ldp * 16 + idx;
  double sum = 0.0;
  for (int b = 0; b < nblk; ++b) sum += p[(size_t)b * ldp * 16];
  out[(size_t)grp * gso + idx] = sum;
}

void launch_cplx_dots(hipStream_t st, const GroupTab& gt, int n, int m2, int nvec, int want_self, const double* V,
                      size_t vstride, size_t gsv, const double* w, size_t gsw, double* partial, int ldp, double* out,
                      size_t gso) {
  const int cnt = nvec + (want_self ? 1 : 0);
  if (gt.ng <= 0 || cnt <= 0) return;
  const int nblk = cplx_num_blocks(n);
  hipLaunchKernelGGL(cplx_dots_kernel, dim3(nblk, 1, gt.ng), dim3(256), 0, st, gt, n, m2, nvec, want_self, V, vstride,
                     gsv, w, gsw, partial, ldp);
  hipLaunchKernelGGL(cplx_reduce_kernel, dim3((cnt * 16 + 255) / 256, 1, gt.ng), dim3(256), 0, st, gt, nblk, cnt, ldp,
                     partial, out, gso);
}

// w += sign * sum_{j < nvec[grp]} v_j h_j  with complex coefficients h (per group: row j holds 16 doubles, complex
// column c at 2c, 2c + 1): the projection step of CGS2 (sign = -1) and the correction x += Z y (sign = +1)
__global__ __launch_bounds__(256) void cplx_update_kernel(GroupTab gt, GroupInts nvecs, int n, int m2,
                                                          const double* __restrict__ V, size_t vstride, size_t gsv,
                                                          const double* __restrict__ h, size_t gsh, double sign,
                                                          double* __restrict__ w, size_t gsw) {
  const int grp = gt.gid[blockIdx.z];
  const int g = threadIdx.x & 15, s = threadIdx.x >> 4;
  if (g >= m2) return;
  const int r0 = blockIdx.x * CX_ROWS, nvec = nvecs.v[grp];
  const double sg = (g & 1) ? 1.0 : -1.0;
  const double* __restrict__ hg = h + (size_t)grp * gsh;
  double acc[CX_RPT];
#pragma unroll
  for (int i = 0; i < CX_RPT; ++i) acc[i] = 0.0;
  for (int j = 0; j < nvec; ++j) {
    const double hr = hg[j * 16 + (g & ~1)], hi = sg * hg[j * 16 + (g | 1)];
    const double* __restrict__ vj = V + (size_t)j * vstride + (size_t)grp * gsv;
#pragma unroll
    for (int i = 0; i < CX_RPT; ++i) {
      const int row = r0 + s + 16 * i;
      if (row < n) acc[i] = fma(hr, vj[(size_t)row * m2 + g], fma(hi, vj[(size_t)row * m2 + (g ^ 1)], acc[i]));
    }
  }
  double* __restrict__ wg = w + (size_t)grp * gsw;
#pragma unroll
  for (int i = 0; i < CX_RPT; ++i) {
    const int row = r0 + s + 16 * i;
    if (row < n) wg[(size_t)row * m2 + g] += sign * acc[i];
  }
}
void launch_cplx_update(hipStream_t st, const GroupTab& gt, const GroupInts& nvecs, int n, int m2, const double* V,
                        size_t vstride, size_t gsv, const double* h, size_t gsh, double sign, double* w, size_t gsw) {
  if (gt.ng <= 0) return;
  hipLaunchKernelGGL(cplx_update_kernel, dim3(cplx_num_blocks(n), 1, gt.ng), dim3(256), 0, st, gt, nvecs, n, m2, V,
                     vstride, gsv, h, gsh, sign, w, gsw);
}

// out = a * in + b * scale[grp][column] * other   elementwise on the real view (other == NULL: the first term only;
// scale == NULL: 1).  Serves the normalisation (a = 0, other = w, scale), the residual b - S x (a = -1, b = 1) and
// the copy of a panel.  `out` may be `in` or `other` (no __restrict__ on the panels).
__global__ __launch_bounds__(256) void cplx_axpby_kernel(GroupTab gt, size_t count, int m2, double a, const double* in,
                                                         size_t gsi, double b, const double* __restrict__ scale,
                                                         const double* other, size_t gso_, double* out, size_t gsout) {
  const int grp = gt.gid[blockIdx.z];
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) {
    double v = a != 0.0 ? a * in[(size_t)grp * gsi + i] : 0.0;
    if (other) v += b * (scale ? scale[grp * 16 + (int)(i % m2)] : 1.0) * other[(size_t)grp * gso_ + i];
    out[(size_t)grp * gsout + i] = v;
  }
}
void launch_cplx_axpby(hipStream_t st, const GroupTab& gt, size_t count, int m2, double a, const double* in, size_t gsi,
                       double b, const double* scale, const double* other, size_t gso, double* out, size_t gsout) {
  if (gt.ng <= 0 || count == 0) return;
  const int grid = (int)std::min<size_t>((count + 255) / 256, 2048);
  hipLaunchKernelGGL(cplx_axpby_kernel, dim3(grid, 1, gt.ng), dim3(256), 0, st, gt, count, m2, a, in, gsi, b, scale,
                     other, gso, out, gsout);
}

// The end of a CGS2 step: hout[j] = h1[j] + h2[j] (j < nvec), hout[nvec] = (||w||, 0) from the squared norms, and the
// factor 1 / ||w|| (0 for a vanished column) in both slots of the column's pair
__global__ __launch_bounds__(256) void cplx_orth_finish_kernel(GroupTab gt, int nvec, const double* __restrict__ h1,
                                                               const double* __restrict__ h2,
                                                               const double* __restrict__ nrm2, size_t gsh,
                                                               double* __restrict__ hout, double* __restrict__ scale) {
  const int grp = gt.gid[blockIdx.x];
  const size_t o = (size_t)grp * gsh;
  for (int idx = threadIdx.x; idx < nvec * 16; idx += 256) hout[o + idx] = h1[o + idx] + h2[o + idx];
  if (threadIdx.x < 16) {
    const double nn = sqrt(nrm2[grp * 16 + (threadIdx.x & ~1)]);
    hout[o + (size_t)nvec * 16 + threadIdx.x] = (threadIdx.x & 1) ? 0.0 : nn;
    scale[grp * 16 + threadIdx.x] = nn > 0.0 ? 1.0 / nn : 0.0;
  }
}
void launch_cplx_orth_finish(hipStream_t st, const GroupTab& gt, int nvec, const double* h1, const double* h2,
                             const double* nrm2, size_t gsh, double* hout, double* scale) {
  if (gt.ng <= 0) return;
  hipLaunchKernelGGL(cplx_orth_finish_kernel, dim3(gt.ng), dim3(256), 0, st, gt, nvec, h1, h2, nrm2, gsh, hout, scale);
}

// ---------------------------------------------------------------------------
// K3c, the small stages: one wave per group, lane c < mc owns complex column c.
// Storage per (group, column): Hm restart x (restart + 1) complex (column j of R, entries 0 .. j + 1), cs restart
// reals, sn restart complex, gv (restart + 1) complex; rotations G = [[c, s], [-conj(s), c]] with c real.
// ---------------------------------------------------------------------------
struct cd {
  double re, im;
};
__device__ __forceinline__ cd cmul(cd a, cd b) { return cd{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cd cconj(cd a) { return cd{a.re, -a.im}; }

// cycle start: gv[0] = ||r||, scale = 1 / ||r|| (0 for a vanished column), resid = ||r|| / ||b|| (0 where b = 0)
__global__ __launch_bounds__(64) void cplx_gmres_start_kernel(GroupTab gt, int mc, int restart,
                                                              const double* __restrict__ nrm2,
                                                              const double* __restrict__ bnorm, double* __restrict__ gv,
                                                              double* __restrict__ scale, double* __restrict__ resid) {
  const int grp = gt.gid[blockIdx.x], c = threadIdx.x;
  if (c >= mc) return;
  const double nn = sqrt(nrm2[grp * 16 + 2 * c]), bn = bnorm[grp * 8 + c];
  double* gc = gv + ((size_t)grp * 8 + c) * (restart + 1) * 2;
  gc[0] = nn;
  gc[1] = 0.0;
  scale[grp * 16 + 2 * c] = scale[grp * 16 + 2 * c + 1] = nn > 0.0 ? 1.0 / nn : 0.0;
  resid[grp * 8 + c] = bn > 0.0 ? nn / bn : 0.0;
}
void launch_cplx_gmres_start(hipStream_t st, const GroupTab& gt, int mc, int restart, const double* nrm2,
                             const double* bnorm, double* gv, double* scale, double* resid) {
  if (gt.ng <= 0) return;
  hipLaunchKernelGGL(cplx_gmres_start_kernel, dim3(gt.ng), dim3(64), 0, st, gt, mc, restart, nrm2, bnorm, gv, scale,
                     resid);
}

// column j of the Hessenberg matrix (hcol: rows 0 .. j complex, row j + 1 the norm) through the rotations 0 .. j - 1,
// then the new rotation; resid = |gv[j + 1]| / ||b||
__global__ __launch_bounds__(64) void cplx_gmres_hess_kernel(GroupTab gt, int mc, int j, int restart,
                                                             const double* __restrict__ hcol, size_t gsh,
                                                             double* __restrict__ Hm, double* __restrict__ cs,
                                                             double* __restrict__ sn, double* __restrict__ gv,
                                                             const double* __restrict__ bnorm,
                                                             double* __restrict__ resid) {
  const int grp = gt.gid[blockIdx.x], c = threadIdx.x;
  if (c >= mc) return;
  const size_t gc = (size_t)grp * 8 + c;
  const double* hc = hcol + (size_t)grp * gsh + 2 * c;
  double* Hj = Hm + (gc * restart + j) * (size_t)(restart + 1) * 2;
  double* csc = cs + gc * restart;
  double* snc = sn + gc * restart * 2;
  double* g = gv + gc * (restart + 1) * 2;
  cd cur{hc[0], hc[1]};
  for (int i = 0; i < j; ++i) {
    const cd nxt{hc[(i + 1) * 16], hc[(i + 1) * 16 + 1]};
    const double ci = csc[i];
    const cd si{snc[2 * i], snc[2 * i + 1]};
    const cd sn_nxt = cmul(si, nxt), sc_cur = cmul(cconj(si), cur);
    Hj[2 * i] = ci * cur.re + sn_nxt.re;
    Hj[2 * i + 1] = ci * cur.im + sn_nxt.im;
    cur = cd{ci * nxt.re - sc_cur.re, ci * nxt.im - sc_cur.im};
  }
  const double b = hc[(j + 1) * 16];   // real, >= 0
  const double na = hypot(cur.re, cur.im), r = hypot(na, b);
  double cj;
  cd sj, d;
  if (r == 0.0) {
    cj = 1.0;
    sj = cd{0.0, 0.0};
    d = cd{0.0, 0.0};
  } else if (na == 0.0) {
    cj = 0.0;
    sj = cd{1.0, 0.0};
    d = cd{b, 0.0};
  } else {
    cj = na / r;
    const double f = b / (na * r);
    sj = cd{cur.re * f, cur.im * f};
    const double e = r / na;
    d = cd{cur.re * e, cur.im * e};
  }
  Hj[2 * j] = d.re;
  Hj[2 * j + 1] = d.im;
  Hj[2 * (j + 1)] = 0.0;
  Hj[2 * (j + 1) + 1] = 0.0;
  csc[j] = cj;
  snc[2 * j] = sj.re;
  snc[2 * j + 1] = sj.im;
  const cd gj{g[2 * j], g[2 * j + 1]};
  const cd gn = cmul(cconj(sj), gj);
  g[2 * (j + 1)] = -gn.re;
  g[2 * (j + 1) + 1] = -gn.im;
  g[2 * j] = cj * gj.re;
  g[2 * j + 1] = cj * gj.im;
  const double bn = bnorm[gc];
  resid[gc] = bn > 0.0 ? hypot(gn.re, gn.im) / bn : 0.0;
}
void launch_cplx_gmres_hess(hipStream_t st, const GroupTab& gt, int mc, int j, int restart, const double* hcol,
                            size_t gsh, double* Hm, double* cs, double* sn, double* gv, const double* bnorm,
                            double* resid) {
  if (gt.ng <= 0) return;
  hipLaunchKernelGGL(cplx_gmres_hess_kernel, dim3(gt.ng), dim3(64), 0, st, gt, mc, j, restart, hcol, gsh, Hm, cs, sn, gv,
                     bnorm, resid);
}

// R y = g for the first ks[grp] columns; y per group: row i holds 16 doubles (complex column c at 2c, 2c + 1).  A
// vanished pivot (a column whose right-hand side is zero, or an exact breakdown) gives y_i = 0.
__global__ __launch_bounds__(64) void cplx_gmres_backsolve_kernel(GroupTab gt, GroupInts ks, int mc, int restart,
                                                                  const double* __restrict__ Hm,
                                                                  const double* __restrict__ gv, double* __restrict__ y,
                                                                  size_t gsy) {
  const int grp = gt.gid[blockIdx.x], c = threadIdx.x;
  if (c >= mc) return;
  const int k = ks.v[grp];
  const size_t gc = (size_t)grp * 8 + c;
  const double* Hc = Hm + gc * restart * (size_t)(restart + 1) * 2;
  const double* g = gv + gc * (restart + 1) * 2;
  double* yc = y + (size_t)grp * gsy + 2 * c;
  for (int i = k - 1; i >= 0; --i) {
    cd sacc{g[2 * i], g[2 * i + 1]};
    for (int l = i + 1; l < k; ++l) {
      const double* Hl = Hc + (size_t)l * (restart + 1) * 2;
      const cd p = cmul(cd{Hl[2 * i], Hl[2 * i + 1]}, cd{yc[l * 16], yc[l * 16 + 1]});
      sacc.re -= p.re;
      sacc.im -= p.im;
    }
    const double* Hi = Hc + (size_t)i * (restart + 1) * 2;
    const cd d{Hi[2 * i], Hi[2 * i + 1]};
    const double dd = d.re * d.re + d.im * d.im;
    cd yi{0.0, 0.0};
    if (dd > 0.0) {
      const cd q = cmul(sacc, cconj(d));
      yi = cd{q.re / dd, q.im / dd};
    }
    yc[i * 16] = yi.re;
    yc[i * 16 + 1] = yi.im;
  }
}
void launch_cplx_gmres_backsolve(hipStream_t st, const GroupTab& gt, const GroupInts& ks, int mc, int restart,
                                 const double* Hm, const double* gv, double* y, size_t gsy) {
  if (gt.ng <= 0) return;
  hipLaunchKernelGGL(cplx_gmres_backsolve_kernel, dim3(gt.ng), dim3(64), 0, st, gt, ks, mc, restart, Hm, gv, y, gsy);
}

// ---------------------------------------------------------------------------
// K6c: the streaming kernels of the complex-conjugate pair step of the Lyapunov ADI.  The m'
// real columns of a step -- the residual factor W and, with a low-rank term, U beside it -- travel as ng groups of mc
// complex columns: real column j is complex column j % mc of group j / mc.
// ---------------------------------------------------------------------------
constexpr int PAIR_ROWS = 32;   // rows per workgroup of both kernels
int adi_pair_rows() { return PAIR_ROWS; }
int adi_pair_num_blocks(int nv) { return std::max(1, (nv + PAIR_ROWS - 1) / PAIR_ROWS); }

// R_g (nv x mc complex, group stride gsr doubles) <- columns g mc .. of [W (nv x m), U (nv x q)]: imaginary parts zero,
// columns behind m + q zero.  One 16-byte store per complex entry.
__global__ __launch_bounds__(256) void adi_pair_pack_kernel(int nv, int m, int q, int ng, int mc,
                                                            const double* __restrict__ W, const double* __restrict__ U,
                                                            double* __restrict__ R, size_t gsr) {
  const int wide = ng * mc;
  const size_t total = (size_t)nv * wide;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const size_t row = idx / wide;
    const int j = (int)(idx % wide), grp = j / mc, cc = j % mc;
    double v = 0.0;
    if (j < m) v = W[row * m + j];
    else if (j < m + q) v = U[row * q + (j - m)];
    *reinterpret_cast<double2*>(R + (size_t)grp * gsr + (row * mc + cc) * 2) = make_double2(v, 0.0);
  }
}
void launch_adi_pair_pack(hipStream_t st, int nv, int m, int q, int ng, int mc, const double* W, const double* U,
                          double* R, size_t gsr) {
  if (nv <= 0 || ng <= 0) return;
  const size_t total = (size_t)nv * ng * mc;
  const int grid = (int)std::min<size_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(adi_pair_pack_kernel, dim3(grid), dim3(256), 0, st, nv, m, q, ng, mc, W, U, R, gsr);
}

// The two real blocks of a pair step from the solution groups X_g (rows x mc complex, group stride gsx doubles; the
// first nv rows are read, the pressure rows behind them never): per velocity row and column j < m, with x = X[row][j],
//   v1 = Re x + delta Im x,   Z[row][zc + j] = gam v1,   Z[row][zc + m + j] = gam2 Im x,   V1[row][j] = v1
// (gam = 2 sqrt(-a), gam2 = gam sqrt(delta^2 + 1), delta = a / b).  A workgroup owns PAIR_ROWS rows; thread t takes the
// entries t, t + 256, .. of its tile in row-major order (one 16-byte load each) and sums the squares of what it wrote;
// the 256 sums are added pairwise in LDS in a fixed tree, partial[2 blk], partial[2 blk + 1] are the workgroup's shares
// of the two squared Frobenius norms.
__global__ __launch_bounds__(256) void adi_pair_blocks_kernel(int nv, int m, int mc, double delta, double gam,
                                                              double gam2, const double* __restrict__ X, size_t gsx,
                                                              double* __restrict__ Z, int zld, int zc,
                                                              double* __restrict__ V1, double* __restrict__ partial) {
  __shared__ double s1[256], s2[256];
  const int r0 = blockIdx.x * PAIR_ROWS, m2 = 2 * mc;
  const int rows = min(PAIR_ROWS, nv - r0);
  double a1 = 0.0, a2 = 0.0;
  for (int idx = threadIdx.x; idx < rows * m; idx += 256) {
    const size_t row = (size_t)(r0 + idx / m);
    const int j = idx % m, grp = j / mc, cc = j % mc;
    const double2 x = *reinterpret_cast<const double2*>(X + (size_t)grp * gsx + row * m2 + 2 * cc);
    const double v1 = fma(delta, x.y, x.x);
    const double z1 = gam * v1, z2 = gam2 * x.y;
    Z[row * zld + zc + j] = z1;
    Z[row * zld + zc + m + j] = z2;
    V1[row * m + j] = v1;
    a1 = fma(z1, z1, a1);
    a2 = fma(z2, z2, a2);
  }
  s1[threadIdx.x] = a1;
  s2[threadIdx.x] = a2;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) {
      s1[threadIdx.x] += s1[threadIdx.x + w];
      s2[threadIdx.x] += s2[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = s1[0];
    partial[2 * blockIdx.x + 1] = s2[0];
  }
}
// out[k] = sum over the workgroups, in workgroup order, of partial[2 blk + k]  (k < 2; the pattern of cplx_reduce_kernel)
__global__ __launch_bounds__(64) void adi_pair_reduce_kernel(int nblk, const double* __restrict__ partial,
                                                             double* __restrict__ out) {
  if (threadIdx.x >= 2) return;
  double sum = 0.0;
  for (int b = 0; b < nblk; ++b) sum += partial[2 * b + threadIdx.x];
  out[threadIdx.x] = sum;
}
void launch_adi_pair_blocks(hipStream_t st, int nv, int m, int mc, double delta, double gam, double gam2,
                            const double* X, size_t gsx, double* Z, int zld, int zc, double* V1, double* partial,
                            double* norms2) {
  if (nv <= 0 || m <= 0) return;
  const int nblk = adi_pair_num_blocks(nv);
  hipLaunchKernelGGL(adi_pair_blocks_kernel, dim3(nblk), dim3(256), 0, st, nv, m, mc, delta, gam, gam2, X, gsx, Z, zld,
                     zc, V1, partial);
  hipLaunchKernelGGL(adi_pair_reduce_kernel, dim3(1), dim3(64), 0, st, nblk, partial, norms2);
}

}  // namespace ricadi
