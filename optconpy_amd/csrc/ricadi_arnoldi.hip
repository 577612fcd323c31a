// ricadi_arnoldi.hip -- K3: the Arnoldi passes of the lockstep GMRES on a low-precision-stored Krylov basis
// (dots, update+dots, update + Hessenberg) and the small per-column GMRES kernels.
//
//
// Everything here is new code: the reference (/root/reference) has no native or
// GPU source at all; the kernels implement the list
// K1..K6 of SURVEY.md section 8(a).
//
// Layout rules shared by all kernels
//   * dense panels are row-major n x m, one row = m contiguous doubles
//     (m = 16 -> one 128-B line per row: an indexed row gather is a full line);
//   * a wavefront (64 lanes) is split into 16-lane groups; a group owns one
//     matrix row and its lanes own the panel columns g, g+16, ...;
//   * reductions over rows are two-stage (per-workgroup partials, then a small
//     reduce kernel), so results are bitwise reproducible run to run.
#include <stdexcept>

#include "ricadi_device.h"

namespace ricadi {

// ---------------------------------------------------------------------------
// K3: per-column Krylov orthogonalisation.
//
// cols_dots: partial[blk][i][c] = sum_{r in chunk} V_i[r,c] * w[r,c]  for
// i < nvec (vector nvec, if want_self, is w itself -> ||w||^2 per column).
// The w chunk is staged in LDS once and re-used against every basis panel
// (the "LDS-staged Krylov panel"); a thread owns one (i, c) output, the 16
// lanes of a group read one contiguous row of V_i, so no cross-lane reduction
// is needed at all.  A second kernel sums the partials over workgroups.
// ---------------------------------------------------------------------------
constexpr int DOT_ROWS = 64;

// the dot phase on a staged chunk: wl holds nr rows of m doubles (the chunk starts at element `base` of every basis
// vector); pout[i * m + c], i < nvec (and row nvec = the chunk's own column norms squared, if want_self)
template <class BT>
__device__ __forceinline__ void chunk_dots(const BT* __restrict__ basis, size_t vstride, size_t base, int nr, int m,
                                           int nvec, int want_self, const double* wl, double* __restrict__ pout) {
  const int nout = (nvec + (want_self ? 1 : 0)) * m;
  for (int o = threadIdx.x; o < nout; o += blockDim.x) {
    const int i = o / m, c = o - i * m;
    double s0 = 0.0, s1 = 0.0;
    int r = 0;
    if (i < nvec) {
      const BT* v = basis + (size_t)i * vstride + base + c;
      double s2 = 0.0, s3 = 0.0;
      for (; r + 3 < nr; r += 4) {       // four independent row loads in flight
        const double v0 = (double)v[(size_t)r * m], v1 = (double)v[(size_t)(r + 1) * m];
        const double v2 = (double)v[(size_t)(r + 2) * m], v3 = (double)v[(size_t)(r + 3) * m];
        s0 = fma(v0, wl[r * m + c], s0);
        s1 = fma(v1, wl[(r + 1) * m + c], s1);
        s2 = fma(v2, wl[(r + 2) * m + c], s2);
        s3 = fma(v3, wl[(r + 3) * m + c], s3);
      }
      for (; r < nr; ++r) s0 = fma((double)v[(size_t)r * m], wl[r * m + c], s0);
      s0 += s2;
      s1 += s3;
    } else {
      for (; r < nr; ++r) s0 = fma(wl[r * m + c], wl[r * m + c], s0);
    }
    pout[o] = s0 + s1;
  }
}
template <class BT>
__global__ __launch_bounds__(256) void cols_dots_kernel(
    GroupTab gt, int nrows, int m, int nvec, const BT* __restrict__ basis, size_t vstride, size_t gsb,
    const double* __restrict__ w, size_t gsw, int want_self, double* __restrict__ partial, size_t gsp) {
  extern __shared__ double wl[];  // DOT_ROWS x m
  const int grp = gt.gid[blockIdx.z];
  basis += (size_t)grp * gsb;
  w += (size_t)grp * gsw;
  partial += (size_t)grp * gsp;
  const int r0 = blockIdx.x * DOT_ROWS;
  const int nr = min(DOT_ROWS, nrows - r0);
  for (int e = threadIdx.x; e < nr * m; e += blockDim.x) wl[e] = w[(size_t)r0 * m + e];
  __syncthreads();
  const int nout = (nvec + (want_self ? 1 : 0)) * m;
  chunk_dots(basis, vstride, (size_t)r0 * m, nr, m, nvec, want_self, wl, partial + (size_t)blockIdx.x * nout);
}

// out[o] (+)= sum_b partial[b][o].  256 threads = 16 outputs x 16 block-slices:
// the 16 lanes of a group read 16 consecutive outputs of one partial row (one
// 128-B line), the 16 groups stride over the workgroups; LDS tree at the end.
__global__ __launch_bounds__(256) void reduce_partials_kernel(GroupTab gt, int nblk, int nout,
                                                              const double* __restrict__ partial,
                                                              size_t gsp, double* __restrict__ out,
                                                              size_t gso, int accumulate) {
  __shared__ double red[16][17];
  const int grp = gt.gid[blockIdx.z];
  partial += (size_t)grp * gsp;
  out += (size_t)grp * gso;
  const int oo = threadIdx.x & 15, bsl = threadIdx.x >> 4;
  const int o = blockIdx.x * 16 + oo;
  double s0 = 0.0, s1 = 0.0;
  if (o < nout) {
    // eight loads in flight per thread (two left the kernel waiting on ~15 dependent round trips: 6.6 us)
    int b = bsl;
    double t[8];
    for (; b + 112 < nblk; b += 128) {
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = partial[(size_t)(b + 16 * u) * nout + o];
      s0 += (t[0] + t[2]) + (t[4] + t[6]);
      s1 += (t[1] + t[3]) + (t[5] + t[7]);
    }
    for (; b + 16 < nblk; b += 32) {
      s0 += partial[(size_t)b * nout + o];
      s1 += partial[(size_t)(b + 16) * nout + o];
    }
    if (b < nblk) s0 += partial[(size_t)b * nout + o];
  }
  red[bsl][oo] = s0 + s1;
  __syncthreads();
  if (bsl == 0 && o < nout) {
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < 16; ++t) s += red[t][oo];
    out[o] = accumulate ? out[o] + s : s;
  }
}

int dots_num_blocks(int nrows) { return (nrows + DOT_ROWS - 1) / DOT_ROWS; }

// ---------------------------------------------------------------------------
// K3, FP16-stored basis with panels of M = 8 * NOCT columns (NOCT = 2, 16 columns: the hot case; 1, 3, 4: the
// projection solve, the augmented Sherman-Morrison-Woodbury sweep [b, U] of the Newton step and wider panels): the
// same three Arnoldi passes with 16-byte (8 x FP16) basis loads.  The generic kernels above read 2 bytes per lane
// and load, which is fine while the launches are latency bound (n ~ 3e4) and leaves them at 0.34-0.46 of the HBM
// roofline at n = 5e5.
//   dots: lane = (row slice s = lane & 15, (vector, column octet) pair) -- the 16 lanes of a DPP row hold the 16 row
//   slices of ONE pair, each lane runs over rows s, s+16, s+32, s+48 of the 64-row chunk with its 4 loads in flight,
//   and the row sum is 4 DPP exchanges.
// ---------------------------------------------------------------------------
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));

template <int CTRL>
__device__ __forceinline__ double dpp_xchg(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
// sum over the 16 lanes of a DPP row, result in every lane
__device__ __forceinline__ double dpp_row_sum(double v) {
  v += dpp_xchg<0xB1>(v);    // quad_perm [1,0,3,2]
  v += dpp_xchg<0x4E>(v);    // quad_perm [2,3,0,1]
  v += dpp_xchg<0x141>(v);   // row_half_mirror
  v += dpp_xchg<0x140>(v);   // row_mirror
  return v;
}

// LDS row stride of a staged chunk: M + 2 doubles (16 columns: 18 doubles, 144 B) -- with M the lanes of a DPP row
// (rows s, s+1, ... 128 B apart) fall on two banks sets and every read is an 8-way conflict
constexpr int WLS = 18;
// dot products of the chunk held in wl (DOT_ROWS rows of M doubles, stride M + 2; rows >= nr zeroed) against the
// basis vectors [0, nvec) and, if want_self, against itself (output row nvec)
template <int NOCT>
__device__ __forceinline__ void chunk_dots8x(const _Float16* __restrict__ basis, size_t vstride, int r0, int nr,
                                             int nvec, int want_self, const double* wl, double* __restrict__ pout) {
  constexpr int M = 8 * NOCT, WS = M + 2;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = lane & 15, pr = lane >> 4;
  const int ntot = nvec + (want_self ? 1 : 0);
  const int npairs = ntot * NOCT;
  for (int pq0 = 0; pq0 < npairs; pq0 += 16) {
    const int pq = pq0 + 4 * wave + pr;
    const int i = pq / NOCT, o = pq - i * NOCT;
    double acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = 0.0;
    if (i < nvec) {
      const _Float16* v = basis + (size_t)i * vstride + (size_t)r0 * M + o * 8;
      half8_t x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = s + 16 * k;
        if (row < nr) x[k] = *reinterpret_cast<const half8_t*>(v + (size_t)row * M);
        else x[k] = (half8_t)(_Float16)0;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double* wr = wl + (s + 16 * k) * WS + o * 8;
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = fma((double)x[k][t], wr[t], acc[t]);
      }
    } else if (i == nvec && want_self) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double* wr = wl + (s + 16 * k) * WS + o * 8;
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = fma(wr[t], wr[t], acc[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = dpp_row_sum(acc[t]);
    if (s == 0 && i < ntot) {
      double2* op = reinterpret_cast<double2*>(pout + (size_t)i * M + o * 8);
      op[0] = make_double2(acc[0], acc[1]);
      op[1] = make_double2(acc[2], acc[3]);
      op[2] = make_double2(acc[4], acc[5]);
      op[3] = make_double2(acc[6], acc[7]);
    }
  }
}

// WT: storage type of the panel w.  float: the operator's output of the hot path is an FP32 panel -- the basis it is
// orthogonalised against is FP16-stored, so its rounding of 6e-8 is far inside what the iteration already carries;
// the arithmetic stays FP64.  Its chunk is staged with all loads issued before the first conversion.
template <int NOCT, class WT>
__global__ __launch_bounds__(256) void cols_dots8x_kernel(
    GroupTab gt, int nrows, int nvec, const _Float16* __restrict__ basis, size_t vstride, size_t gsb,
    const WT* __restrict__ w, size_t gsw, int want_self, double* __restrict__ partial, size_t gsp) {
  constexpr int M = 8 * NOCT, WS = M + 2, M2 = M / 2;     // a thread stages two-column pieces, M2 per row
  __shared__ __attribute__((aligned(16))) double wl[DOT_ROWS * WS];
  const int grp = gt.gid[blockIdx.z];
  basis += (size_t)grp * gsb;
  w += (size_t)grp * gsw;
  partial += (size_t)grp * gsp;
  const int r0 = blockIdx.x * DOT_ROWS;
  const int nr = min(DOT_ROWS, nrows - r0);
  auto piece = [&](int e) {
    const int row = e / M2;
    return reinterpret_cast<double2*>(wl + row * WS + 2 * (e - row * M2));
  };
  if constexpr (sizeof(WT) == 4) {
    constexpr int NL = DOT_ROWS * M2 / 256;
    const float2* src = reinterpret_cast<const float2*>(w + (size_t)r0 * M);
    float2 raw[NL];
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const int e = threadIdx.x + 256 * k;
      raw[k] = src[e < nr * M2 ? e : 0];
    }
#pragma unroll
    for (int k = 0; k < NL; ++k) {
      const int e = threadIdx.x + 256 * k;
      *piece(e) = e < nr * M2 ? make_double2((double)raw[k].x, (double)raw[k].y) : make_double2(0.0, 0.0);
    }
  } else {
    const double2* src = reinterpret_cast<const double2*>(w + (size_t)r0 * M);
    for (int e = threadIdx.x; e < DOT_ROWS * M2; e += 256) *piece(e) = e < nr * M2 ? src[e] : make_double2(0.0, 0.0);
  }
  __syncthreads();
  const int nout = (nvec + (want_self ? 1 : 0)) * M;
  chunk_dots8x<NOCT>(basis, vstride, r0, nr, nvec, want_self, wl, partial + (size_t)blockIdx.x * nout);
}

// w' = w - V h (written back), then the dots of w' against V and itself (chunk_dots8x; the basis chunk
// is cache resident by then, so the LDS side decides: with unpadded rows this phase was 2x slower)
// STORE = false: w' is only staged in LDS for the dots, the panel w keeps the vector BEFORE the first projection (the
// final update then subtracts the basis with the SUM of both passes' coefficients: one 8-byte store per element less)
template <int NOCT, bool STORE, class WT>
__global__ __launch_bounds__(256) void cols_update_dots8x_kernel(
    GroupTab gt, int nrows, int nvec, const _Float16* __restrict__ basis, size_t vstride, size_t gsb,
    const double* __restrict__ h, size_t gsh, WT* __restrict__ w, size_t gsw,
    double* __restrict__ partial, size_t gsp) {
  constexpr int M = 8 * NOCT, WS = M + 2;
  extern __shared__ __attribute__((aligned(16))) double sm8x[];
  double* wl = sm8x;                       // DOT_ROWS rows, stride WS
  double* hl = sm8x + DOT_ROWS * WS;       // nvec x M
  const int grp = gt.gid[blockIdx.z];
  basis += (size_t)grp * gsb;
  h += (size_t)grp * gsh;
  w += (size_t)grp * gsw;
  partial += (size_t)grp * gsp;
  const int r0 = blockIdx.x * DOT_ROWS;
  const int nr = min(DOT_ROWS, nrows - r0);
  for (int e = threadIdx.x; e < nvec * M; e += 256) hl[e] = h[e];
  __syncthreads();
  {
    // update: a thread owns the elements tid, tid + 256, ... of the chunk (for M = 8, 16, 32 all in one column);
    // per pair of basis vectors its two-byte loads are issued together and the coefficients come from LDS once.
    // (The 16-byte form with the vectors split over lane pairs was slower at every basis size: 1.69 vs 1.02 ms at
    // n = 5e5, 16 columns, 7 vectors.)
    const size_t base = (size_t)r0 * M;
    constexpr int NE = DOT_ROWS * M / 256;           // 2 * NOCT
    int e[NE], c[NE];
    bool ok[NE];
    double sacc[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) {
      e[k] = threadIdx.x + 256 * k;
      c[k] = e[k] % M;
      ok[k] = e[k] < nr * M;
      sacc[k] = 0.0;
    }
    int i = 0;
    for (; i + 1 < nvec; i += 2) {
      _Float16 b0[NE], b1[NE];
      const _Float16* v0 = basis + (size_t)i * vstride + base;
      const _Float16* v1 = v0 + vstride;
#pragma unroll
      for (int k = 0; k < NE; ++k) {
        b0[k] = v0[ok[k] ? e[k] : 0];               // unconditional loads (row 0 of the chunk is always valid)
        b1[k] = v1[ok[k] ? e[k] : 0];
      }
      const double* h0 = hl + i * M;
      const double* h1 = h0 + M;
#pragma unroll
      for (int k = 0; k < NE; ++k) sacc[k] = fma(h1[c[k]], (double)b1[k], fma(h0[c[k]], (double)b0[k], sacc[k]));
    }
    if (i < nvec) {
      _Float16 b0[NE];
      const _Float16* v0 = basis + (size_t)i * vstride + base;
#pragma unroll
      for (int k = 0; k < NE; ++k) b0[k] = v0[ok[k] ? e[k] : 0];
      const double* h0 = hl + i * M;
#pragma unroll
      for (int k = 0; k < NE; ++k) sacc[k] = fma(h0[c[k]], (double)b0[k], sacc[k]);
    }
    WT wv[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) wv[k] = w[base + (ok[k] ? e[k] : 0)];
#pragma unroll
    for (int k = 0; k < NE; ++k) {
      const double v = ok[k] ? (double)wv[k] - sacc[k] : 0.0;
      if (STORE && ok[k]) w[base + e[k]] = (WT)v;
      wl[(e[k] / M) * WS + c[k]] = v;
    }
  }
  __syncthreads();
  chunk_dots8x<NOCT>(basis, vstride, r0, nr, nvec, 1, wl, partial + (size_t)blockIdx.x * (nvec + 1) * M);
}

// a[t] += sum_{i < nvec} hc[i * ldh + t] * V_i[t], t < 8: the eight FP16 columns at v of nvec vectors vstride apart
// (hc: the coefficients of those columns, rows of ldh doubles); 16-byte loads, four vectors in flight
__device__ __forceinline__ void accum_octet(const _Float16* v, size_t vstride, int nvec, const double* hc,
                                            int ldh, double (&a)[8]) {
  int i = 0;
  for (; i + 3 < nvec; i += 4) {
    half8_t x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const half8_t*>(v + (size_t)(i + u) * vstride);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < 8; ++t) a[t] = fma(hc[(i + u) * ldh + t], (double)x[u][t], a[t]);
  }
  for (; i < nvec; ++i) {
    const half8_t x = *reinterpret_cast<const half8_t*>(v + (size_t)i * vstride);
#pragma unroll
    for (int t = 0; t < 8; ++t) a[t] = fma(hc[i * ldh + t], (double)x[t], a[t]);
  }
}

// out = scale * (w + sign * V h), stored in FP16 (outf) and, rounded identically, in FP64 (out):
// thread = (row, column half), 16-byte basis loads, four vectors in flight
__global__ __launch_bounds__(256) void cols_update16_kernel(
    GroupTab gt, size_t nhalf, GroupInts nvecs, const _Float16* __restrict__ basis, size_t vstride, size_t gsb,
    const double* __restrict__ h, size_t gsh, double sign, const double* __restrict__ w, size_t gsw,
    const double* __restrict__ scale, double* __restrict__ out, size_t gso, _Float16* __restrict__ outf,
    size_t gsf, int m) {
  extern __shared__ double hl[];           // nvec x m  (m = 8, 16, 24 or 32 columns)
  const int noct = m >> 3;
  const int grp = gt.gid[blockIdx.z];
  const int nvec = nvecs.v[grp];
  basis += (size_t)grp * gsb;
  h += (size_t)grp * gsh;
  if (w) w += (size_t)grp * gsw;
  if (scale) scale += (size_t)grp * m;
  if (out) out += (size_t)grp * gso;
  if (outf) outf += (size_t)grp * gsf;
  for (int e = threadIdx.x; e < nvec * m; e += 256) hl[e] = h[e];
  __syncthreads();
  for (size_t idx = blockIdx.x * (size_t)256 + threadIdx.x; idx < nhalf; idx += (size_t)gridDim.x * 256) {
    const size_t e = idx * 8;
    const int c0 = (int)(idx % (size_t)noct) * 8;
    double a[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) a[t] = 0.0;
    accum_octet(basis + e, vstride, nvec, hl + c0, m, a);
    if (w) {
      const double2* wp = reinterpret_cast<const double2*>(w + e);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double2 ww = wp[t];
        a[2 * t] = ww.x + sign * a[2 * t];
        a[2 * t + 1] = ww.y + sign * a[2 * t + 1];
      }
    } else {
#pragma unroll
      for (int t = 0; t < 8; ++t) a[t] *= sign;
    }
    if (scale) {
#pragma unroll
      for (int t = 0; t < 8; ++t) a[t] *= scale[c0 + t];
    }
    if (outf) {
      half8_t f;
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        f[t] = (_Float16)a[t];
        a[t] = (double)f[t];
      }
      *reinterpret_cast<half8_t*>(outf + e) = f;
    }
    if (out) {
      double2* op = reinterpret_cast<double2*>(out + e);
#pragma unroll
      for (int t = 0; t < 4; ++t) op[t] = make_double2(a[2 * t], a[2 * t + 1]);
    }
  }
}
// Same update for an FP32-stored basis (the Z_j of the flexible GMRES: the correction x += Z y at the end of a
// restart cycle): thread = 4 consecutive elements, 16-byte loads, four vectors in flight.  No stored copy.
__global__ __launch_bounds__(256) void cols_update_f4_kernel(
    GroupTab gt, size_t nquad, GroupInts nvecs, const float* __restrict__ basis, size_t vstride, size_t gsb,
    const double* __restrict__ h, size_t gsh, double sign, const double* __restrict__ w, size_t gsw,
    const double* __restrict__ scale, double* __restrict__ out, size_t gso, int m) {
  extern __shared__ double hl[];           // nvec x m
  const int grp = gt.gid[blockIdx.z];
  const int nvec = nvecs.v[grp];
  basis += (size_t)grp * gsb;
  h += (size_t)grp * gsh;
  if (w) w += (size_t)grp * gsw;
  if (scale) scale += (size_t)grp * m;
  out += (size_t)grp * gso;
  for (int e = threadIdx.x; e < nvec * m; e += 256) hl[e] = h[e];
  __syncthreads();
  for (size_t idx = blockIdx.x * (size_t)256 + threadIdx.x; idx < nquad; idx += (size_t)gridDim.x * 256) {
    const size_t e = idx * 4;
    const int c0 = (int)(e % (size_t)m);
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    const float* v = basis + e;
    int i = 0;
    for (; i + 3 < nvec; i += 4) {
      float4 x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const float4*>(v + (size_t)(i + u) * vstride);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double* hh = hl + (i + u) * m + c0;
        a[0] = fma(hh[0], (double)x[u].x, a[0]);
        a[1] = fma(hh[1], (double)x[u].y, a[1]);
        a[2] = fma(hh[2], (double)x[u].z, a[2]);
        a[3] = fma(hh[3], (double)x[u].w, a[3]);
      }
    }
    for (; i < nvec; ++i) {
      const float4 x = *reinterpret_cast<const float4*>(v + (size_t)i * vstride);
      const double* hh = hl + i * m + c0;
      a[0] = fma(hh[0], (double)x.x, a[0]);
      a[1] = fma(hh[1], (double)x.y, a[1]);
      a[2] = fma(hh[2], (double)x.z, a[2]);
      a[3] = fma(hh[3], (double)x.w, a[3]);
    }
    if (w) {
      const double2* wp = reinterpret_cast<const double2*>(w + e);
      const double2 w0 = wp[0], w1 = wp[1];
      a[0] = w0.x + sign * a[0];
      a[1] = w0.y + sign * a[1];
      a[2] = w1.x + sign * a[2];
      a[3] = w1.y + sign * a[3];
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) a[t] *= sign;
    }
    if (scale) {
#pragma unroll
      for (int t = 0; t < 4; ++t) a[t] *= scale[c0 + t];
    }
    double2* op = reinterpret_cast<double2*>(out + e);
    op[0] = make_double2(a[0], a[1]);
    op[1] = make_double2(a[2], a[3]);
  }
}
// ---- launch helpers shared by the dot launchers ----
static void reduce_partials(hipStream_t st, const GroupTab& gt, int nblk, int nout, const double* partial, size_t gsp,
                            double* out, size_t gso) {
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((nout + 15) / 16, 1, gt.ng), dim3(256), 0, st, gt, nblk, nout,
                     partial, gsp, out, gso, 0);
}
constexpr size_t kLdsLimit = 48 * 1024;
// LDS bytes of cols_update_dots8x_kernel: the staged chunk and nvec rows of coefficients
static size_t update_dots_lds_bytes(int m, int nvec) { return (size_t)(DOT_ROWS * (m + 2) + nvec * m) * sizeof(double); }
// fn(integral constant NOCT) for the panel widths the 8x kernels serve; false: another width
template <class Fn>
static bool with_noct(int m, Fn&& fn) {
  switch (m) {
    case 8: fn(std::integral_constant<int, 1>()); return true;
    case 16: fn(std::integral_constant<int, 2>()); return true;
    case 24: fn(std::integral_constant<int, 3>()); return true;
    case 32: fn(std::integral_constant<int, 4>()); return true;
    default: return false;
  }
}
// The FP32 panel exists only on the hot path (iteration_form: FP16 basis, 16 columns, w kept): anything else is a
// dispatch error, never a quiet detour through a generic kernel.
template <class BT, class WT>
static void require_panel_form(int m, bool keep_w) {
  if (std::is_same<WT, float>::value && !(std::is_same<BT, _Float16>::value && m == 16 && keep_w))
    throw std::logic_error("FP32 panel w: only with the FP16-stored basis, 16 columns and w kept");
}

template <class BT, class WT>
void launch_cols_dots_b(hipStream_t st, const GroupTab& gt, int nrows, int m, int nvec,
                        const BT* basis, size_t vstride, size_t gsb, const WT* w, size_t gsw,
                        int want_self, double* partial, size_t gsp, double* out, size_t gso) {
  require_panel_form<BT, WT>(m, true);
  const int nblk = dots_num_blocks(nrows);
  const int nout = (nvec + (want_self ? 1 : 0)) * m;
  if (nout == 0 || gt.ng <= 0) return;
  const dim3 grid(nblk, 1, gt.ng);
  bool done = false;
  if constexpr (std::is_same<BT, _Float16>::value)
    done = with_noct(m, [&](auto noct) {
      constexpr int NOCT = decltype(noct)::value;
      if constexpr (NOCT == 2 || std::is_same<WT, double>::value)
        hipLaunchKernelGGL((cols_dots8x_kernel<NOCT, WT>), grid, dim3(256), 0, st, gt, nrows, nvec, basis, vstride, gsb,
                           w, gsw, want_self, partial, gsp);
    });
  if constexpr (std::is_same<WT, double>::value)
    if (!done)
      hipLaunchKernelGGL(cols_dots_kernel<BT>, grid, dim3(256), DOT_ROWS * m * sizeof(double), st, gt, nrows, m, nvec,
                         basis, vstride, gsb, w, gsw, want_self, partial, gsp);
  reduce_partials(st, gt, nblk, nout, partial, gsp, out, gso);
}
void launch_cols_dots(hipStream_t st, int nrows, int m, int nvec, const double* basis,
                      size_t vstride, const double* w, int want_self, double* partial,
                      double* out) {
  launch_cols_dots_b(st, single_group(), nrows, m, nvec, basis, vstride, 0, w, 0, want_self, partial,
                     0, out, 0);
}

// Fused CGS2 middle step: for a chunk of DOT_ROWS rows
//   w'[r,c] = w[r,c] - sum_i h[i,c] V_i[r,c]          (first Gram-Schmidt update, written back)
//   partial[blk][i,c] = sum_r V_i[r,c] w'[r,c],  i <= nvec  (row nvec = ||w'||^2)
// The dot products of the second pass are row-local, so the block computes them
// right after its slice of w' -- the basis slice it has just read is still in
// L1/L2 -- which saves one launch and one pass over the Krylov basis per
// iteration compared with separate update and dots kernels.
template <class BT>
__global__ __launch_bounds__(256) void cols_update_dots_kernel(
    GroupTab gt, int nrows, int m, int nvec, const BT* __restrict__ basis, size_t vstride,
    size_t gsb, const double* __restrict__ h, size_t gsh, double* __restrict__ w, size_t gsw,
    double* __restrict__ partial, size_t gsp) {
  extern __shared__ double wl[];  // DOT_ROWS x m
  const int grp = gt.gid[blockIdx.z];
  basis += (size_t)grp * gsb;
  h += (size_t)grp * gsh;
  w += (size_t)grp * gsw;
  partial += (size_t)grp * gsp;
  const int r0 = blockIdx.x * DOT_ROWS;
  const int nr = min(DOT_ROWS, nrows - r0);
  const size_t base = (size_t)r0 * m;
  for (int e = threadIdx.x; e < nr * m; e += blockDim.x) {
    const int c = e % m;
    double s0 = 0.0, s1 = 0.0;
    int i = 0;
    for (; i + 1 < nvec; i += 2) {
      s0 = fma(h[i * m + c], (double)basis[(size_t)i * vstride + base + e], s0);
      s1 = fma(h[(i + 1) * m + c], (double)basis[(size_t)(i + 1) * vstride + base + e], s1);
    }
    if (i < nvec) s0 = fma(h[i * m + c], (double)basis[(size_t)i * vstride + base + e], s0);
    const double v = w[base + e] - (s0 + s1);
    wl[e] = v;
    w[base + e] = v;
  }
  __syncthreads();
  chunk_dots(basis, vstride, base, nr, m, nvec, 1, wl, partial + (size_t)blockIdx.x * (nvec + 1) * m);
}
// Can the 16-column FP16 launch leave w untouched (keep_w; see cols_update_dots8x_kernel)?
bool update_dots_keeps_w(int m, bool fp16_basis, int nvec_max) {
  return fp16_basis && m == 16 && update_dots_lds_bytes(16, nvec_max) <= kLdsLimit;
}
bool arnoldi16_w32_ok(int nvec_max) { return update_dots_lds_bytes(16, nvec_max) <= kLdsLimit; }
template <class BT, class WT>
void launch_cols_update_dots_b(hipStream_t st, const GroupTab& gt, int nrows, int m, int nvec,
                               const BT* basis, size_t vstride, size_t gsb, const double* h,
                               size_t gsh, WT* w, size_t gsw, bool keep_w, double* partial, size_t gsp,
                               double* out, size_t gso) {
  require_panel_form<BT, WT>(m, keep_w);
  if (gt.ng <= 0) return;
  const int nblk = dots_num_blocks(nrows);
  const int nout = (nvec + 1) * m;
  const dim3 grid(nblk, 1, gt.ng);
  const size_t lds = update_dots_lds_bytes(m, nvec);
  bool done = false;
  if constexpr (std::is_same<BT, _Float16>::value)
    done = lds <= kLdsLimit && with_noct(m, [&](auto noct) {
      constexpr int NOCT = decltype(noct)::value;
      // (w is kept at 16 columns only: update_dots_keeps_w)
      if constexpr (NOCT == 2) {
        if (keep_w) {
          hipLaunchKernelGGL((cols_update_dots8x_kernel<2, false, WT>), grid, dim3(256), lds, st, gt, nrows, nvec, basis,
                             vstride, gsb, h, gsh, w, gsw, partial, gsp);
          return;
        }
      }
      if constexpr (std::is_same<WT, double>::value)
        hipLaunchKernelGGL((cols_update_dots8x_kernel<NOCT, true, WT>), grid, dim3(256), lds, st, gt, nrows, nvec, basis,
                           vstride, gsb, h, gsh, w, gsw, partial, gsp);
    });
  if (!done) {
    if constexpr (std::is_same<WT, double>::value)
      hipLaunchKernelGGL(cols_update_dots_kernel<BT>, grid, dim3(256), DOT_ROWS * m * sizeof(double), st, gt, nrows, m,
                         nvec, basis, vstride, gsb, h, gsh, w, gsw, partial, gsp);
    else
      throw std::logic_error("FP32 panel w: the coefficients do not fit the update-and-dots kernel's LDS");
  }
  reduce_partials(st, gt, nblk, nout, partial, gsp, out, gso);
}

// out[r,c] = scale[c] * ( w[r,c] + sign * sum_{i<nvec} h[i*m+c] * V_i[r,c] )
// (scale may be NULL = 1; w may be NULL = 0).  Streams nvec panels once.
// outf (optional): the result as stored in the basis (BT: the stored Krylov vector); out then
// holds the same rounded values, so the vector the next operator application
// sees IS the stored one.
template <class BT>
__global__ __launch_bounds__(256) void cols_update_kernel(
    GroupTab gt, size_t nelem, int m, GroupInts nvecs, const BT* __restrict__ basis, size_t vstride,
    size_t gsb, const double* __restrict__ h, size_t gsh, double sign,
    const double* __restrict__ w, size_t gsw, const double* __restrict__ scale,
    double* __restrict__ out, size_t gso, BT* __restrict__ outf, size_t gsf) {
  const int grp = gt.gid[blockIdx.z];
  const int nvec = nvecs.v[grp];
  basis += (size_t)grp * gsb;
  h += (size_t)grp * gsh;
  if (w) w += (size_t)grp * gsw;
  if (scale) scale += (size_t)grp * m;
  if (out) out += (size_t)grp * gso;
  if (outf) outf += (size_t)grp * gsf;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < nelem;
       e += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % m);
    double s0 = 0.0, s1 = 0.0;
    int i = 0;
    for (; i + 1 < nvec; i += 2) {
      s0 = fma(h[i * m + c], (double)basis[(size_t)i * vstride + e], s0);
      s1 = fma(h[(i + 1) * m + c], (double)basis[(size_t)(i + 1) * vstride + e], s1);
    }
    if (i < nvec) s0 = fma(h[i * m + c], (double)basis[(size_t)i * vstride + e], s0);
    double v = (w ? w[e] : 0.0) + sign * (s0 + s1);
    if (scale) v *= scale[c];
    if (outf) {
      const BT f = (BT)v;
      outf[e] = f;
      v = (double)f;
    }
    if (out) out[e] = v;
  }
}
template <class BT>
static void cols_update_impl(hipStream_t st, const GroupTab& gt, int nrows, int m,
                             const GroupInts& nvec, const BT* basis, size_t vstride, size_t gsb,
                             const double* h, size_t gsh,
                             double sign, const double* w, size_t gsw, const double* scale,
                             double* out, size_t gso, BT* outf, size_t gsf) {
  size_t nelem = (size_t)nrows * m;
  if (!nelem || gt.ng <= 0) return;
  if constexpr (std::is_same<BT, _Float16>::value) {
    int nmax = 0;
    for (int i = 0; i < gt.ng; ++i) nmax = std::max(nmax, nvec.v[gt.gid[i]]);
    if ((m & 7) == 0 && m <= 32 && (size_t)nmax * m * sizeof(double) <= kLdsLimit) {
      const size_t nhalf = (size_t)nrows * (m / 8);       // 8-column pieces
      const int grid16 = (int)std::min<size_t>((nhalf + 255) / 256, 8192);
      hipLaunchKernelGGL(cols_update16_kernel, dim3(grid16, 1, gt.ng), dim3(256),
                         (size_t)std::max(nmax, 1) * m * sizeof(double), st, gt, nhalf, nvec, basis, vstride, gsb,
                         h, gsh, sign, w, gsw, scale, out, gso, outf, gsf, m);
      return;
    }
  }
  if constexpr (std::is_same<BT, float>::value) {
    int nmax = 0;
    for (int i = 0; i < gt.ng; ++i) nmax = std::max(nmax, nvec.v[gt.gid[i]]);
    if ((m & 3) == 0 && !outf && out && (size_t)nmax * m * sizeof(double) <= kLdsLimit) {
      const size_t nquad = nelem / 4;
      const int gridq = (int)std::min<size_t>((nquad + 255) / 256, 8192);
      hipLaunchKernelGGL(cols_update_f4_kernel, dim3(gridq, 1, gt.ng), dim3(256),
                         (size_t)std::max(nmax, 1) * m * sizeof(double), st, gt, nquad, nvec, basis, vstride, gsb, h,
                         gsh, sign, w, gsw, scale, out, gso, m);
      return;
    }
  }
  int grid = (int)std::min<size_t>((nelem + 255) / 256, 8192);
  hipLaunchKernelGGL(cols_update_kernel<BT>, dim3(grid, 1, gt.ng), dim3(256), 0, st, gt, nelem, m,
                     nvec, basis, vstride, gsb, h, gsh, sign, w, gsw, scale, out, gso, outf, gsf);
}
template <class BT>
void launch_cols_update_b(hipStream_t st, const GroupTab& gt, int nrows, int m, int nvec,
                          const BT* basis, size_t vstride, size_t gsb, const double* h,
                          size_t gsh, double sign, const double* w, size_t gsw, const double* scale,
                          double* out, size_t gso, BT* outf, size_t gsf) {
  cols_update_impl(st, gt, nrows, m, same_int(nvec), basis, vstride, gsb, h, gsh, sign, w, gsw, scale,
                   out, gso, outf, gsf);
}
// correction step of a restart cycle: group g combines its first nvec.v[g] vectors
// acc (optional): out = acc + sum; acc may be `out` itself (every thread reads its elements before it writes them)
template <class BT>
void launch_cols_update_bk(hipStream_t st, const GroupTab& gt, int nrows, int m, const GroupInts& nvec,
                           const BT* basis, size_t vstride, size_t gsb, const double* h, size_t gsh,
                           double* out, size_t gso, const double* acc, size_t gsa) {
  cols_update_impl(st, gt, nrows, m, nvec, basis, vstride, gsb, h, gsh, 1.0, acc, gsa,
                   (const double*)nullptr, out, gso, (BT*)nullptr, 0);
}
void launch_cols_update(hipStream_t st, int nrows, int m, int nvec, const double* basis,
                        size_t vstride, const double* h, double sign, const double* w,
                        const double* scale, double* out) {
  launch_cols_update_b(st, single_group(), nrows, m, nvec, basis, vstride, 0, h, 0, sign, w, 0, scale,
                       out, 0);
}
// the Krylov basis stored in FP64, FP32 or FP16 (the arithmetic is FP64 throughout)
// ... and the panel w in FP64 or FP32 (FP32: hot path only, require_panel_form)
#define RICADI_PANEL_LAUNCHERS(BT, WT)                                                                                \
  template void launch_cols_dots_b(hipStream_t, const GroupTab&, int, int, int, const BT*, size_t, size_t, const WT*, \
                                   size_t, int, double*, size_t, double*, size_t);                                    \
  template void launch_cols_update_dots_b(hipStream_t, const GroupTab&, int, int, int, const BT*, size_t, size_t,      \
                                          const double*, size_t, WT*, size_t, bool, double*, size_t, double*, size_t);
#define RICADI_BASIS_LAUNCHERS(BT)                                                                                    \
  RICADI_PANEL_LAUNCHERS(BT, double)                                                                                  \
  RICADI_PANEL_LAUNCHERS(BT, float)                                                                                   \
  template void launch_cols_update_b(hipStream_t, const GroupTab&, int, int, int, const BT*, size_t, size_t,           \
                                     const double*, size_t, double, const double*, size_t, const double*, double*,    \
                                     size_t, BT*, size_t);                                                            \
  template void launch_cols_update_bk(hipStream_t, const GroupTab&, int, int, const GroupInts&, const BT*, size_t,     \
                                      size_t, const double*, size_t, double*, size_t, const double*, size_t);
RICADI_BASIS_LAUNCHERS(double)
RICADI_BASIS_LAUNCHERS(float)
RICADI_BASIS_LAUNCHERS(_Float16)
#undef RICADI_BASIS_LAUNCHERS
#undef RICADI_PANEL_LAUNCHERS

// ---------------------------------------------------------------------------
// GMRES small per-column kernels (one thread per panel column).
//   state layout (all device, per column c):
//     H   [c][j][i]   (restart+1) x restart upper Hessenberg -> R after rotations
//     cs,sn [c][i],  g [c][i]
// hess_update: consumes h1 (pass 1), h2 (pass 2 incl. ||w'||^2 as last row),
// applies the stored rotations, creates the new one, writes scale = 1/h_{j+1,j}
// (0 on breakdown / frozen column) and the residual estimate |g_{j+1}|.
// ---------------------------------------------------------------------------
constexpr double kTiny = 1e-300;
// frozen column (already converged: |g_j| at or below thr; or exact breakdown: no sub-diagonal): it is kept inert
__device__ __forceinline__ bool column_frozen(double sub, double gabs, double thr) {
  return !(sub > kTiny) || gabs <= thr;
}
// The new rotation of column j of one panel column: from `cur` (the diagonal entry after the stored rotations) and
// the sub-diagonal `sub` it writes cs[j], sn[j], the rotated Hc[j], Hc[j + 1] and g[j], g[j + 1] (gj: g[j] before);
// returns the residual estimate |g[j + 1]|.
__device__ __forceinline__ double givens_tail(double cur, double sub, double gj, int j, double* Hc, double* cs,
                                              double* sn, double* g) {
  const double d = hypot(cur, sub);
  double cj = 1.0, sj = 0.0;
  if (d > kTiny) {
    cj = cur / d;
    sj = sub / d;
  }
  cs[j] = cj;
  sn[j] = sj;
  Hc[j] = (d > kTiny) ? d : 1.0;           // keep R non-singular for frozen columns
  Hc[j + 1] = 0.0;
  g[j + 1] = (d > kTiny) ? -sj * gj : 0.0;
  g[j] = (d > kTiny) ? cj * gj : 0.0;
  return (d > kTiny) ? fabs(sj * gj) : 0.0;
}

// One 64-lane workgroup per panel column: the lanes stage h1+h2, cs, sn in LDS
// with independent loads (and reduce ||h2||^2 with shuffles); lane 0 then runs
// the sequential rotation chain out of LDS instead of a chain of dependent
// global loads.
__global__ __launch_bounds__(64) void gmres_hess_kernel(
    GroupTab gt, int m, int j, int restart, const double* __restrict__ h1,
    const double* __restrict__ h2, double* __restrict__ H, double* __restrict__ cs,
    double* __restrict__ sn, double* __restrict__ g, double* __restrict__ scale,
    double* __restrict__ resid, const double* __restrict__ bnorm, double tol,
    double* __restrict__ host_resid, double* __restrict__ hsum) {
  extern __shared__ double sh[];       // hcol[restart+2], csl[restart], snl[restart]
  if (host_resid) host_resid += (size_t)gt.gid[blockIdx.z] * m;
  {
    // group-major state: every array holds one slab per group
    const size_t grp = (size_t)gt.gid[blockIdx.z];
    h1 += grp * (restart + 2) * m;
    h2 += grp * (restart + 2) * m;
    if (hsum) hsum += grp * (restart + 2) * m;
    H += grp * m * (restart + 1) * restart;
    cs += grp * m * restart;
    sn += grp * m * restart;
    g += grp * m * (restart + 1);
    scale += grp * m;
    resid += grp * m;
    bnorm += grp * m;
  }
  double* hcol = sh;
  double* csl = sh + restart + 2;
  double* snl = csl + restart;
  const int c = blockIdx.x;
  const int lane = threadIdx.x;
  double* Hc = H + (size_t)c * (restart + 1) * restart + (size_t)j * (restart + 1);
  double* csc = cs + (size_t)c * restart;
  double* snc = sn + (size_t)c * restart;
  double* gc = g + (size_t)c * (restart + 1);
  const int nv = j + 1;
  double part = 0.0;
  for (int i = lane; i < nv; i += 64) {
    const double b = h2[i * m + c];
    part += b * b;
    hcol[i] = h1[i * m + c] + b;
    if (hsum) hsum[i * m + c] = hcol[i];       // coefficients of BOTH passes, for an update that starts from the unprojected w
  }
  for (int i = lane; i < j; i += 64) {
    csl[i] = csc[i];
    snl[i] = snc[i];
  }
  for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
  __syncthreads();
  if (lane != 0) return;
  const double h2sq = part;
  const double ww = h2[nv * m + c];  // ||w'||^2 before the second projection
  const double gj = gc[j];
  double hn2 = ww - h2sq;
  double hnext = hn2 > 0.0 ? sqrt(hn2) : 0.0;
  if (column_frozen(hnext, fabs(gj), 0.01 * tol * bnorm[c])) hnext = 0.0;
  double cur = hcol[0];
  for (int i = 0; i < j; ++i) {
    const double nxt = hcol[i + 1];
    const double t = csl[i] * cur + snl[i] * nxt;
    const double u = -snl[i] * cur + csl[i] * nxt;
    Hc[i] = t;
    cur = u;
  }
  const double rnew = givens_tail(cur, hnext, gj, j, Hc, csc, snc, gc);
  scale[c] = (hnext > kTiny) ? 1.0 / hnext : 0.0;
  resid[c] = rnew;
  // pinned host copy for the (lagged) convergence check: saves a D2H copy per iteration
  if (host_resid) host_resid[c] = rnew;
}
void launch_gmres_hess_b(hipStream_t st, const GroupTab& gt, int m, int j, int restart,
                         const double* h1, const double* h2, double* H, double* cs, double* sn,
                         double* g, double* scale, double* resid, const double* bnorm, double tol,
                         double* host_resid, double* hsum) {
  if (gt.ng <= 0) return;
  hipLaunchKernelGGL(gmres_hess_kernel, dim3(m, 1, gt.ng), dim3(64),
                     (3 * restart + 4) * sizeof(double), st, gt, m, j, restart, h1, h2, H, cs, sn, g,
                     scale, resid, bnorm, tol, host_resid, hsum);
}

// y[i*m + c] solves R y = g for the k x k triangle of column c.  One wave per (column, group): lane l first
// fetches column-entries R[i][l] = Hc[l][i] of all rows i <= l (independent loads, all in flight), then the k steps of
// the back substitution run out of LDS with a wave reduction each (one thread per column walking the triangle with
// dependent global loads took 31 us per call).
__global__ __launch_bounds__(64) void gmres_backsolve_kernel(GroupTab gt, int m, GroupInts ks, int restart,
                                                             const double* __restrict__ H,
                                                             const double* __restrict__ g,
                                                             double* __restrict__ y) {
  extern __shared__ double sm[];          // k rows of 64: sm[i * 64 + l] = R[i][l];  then ys[64]
  const int c = blockIdx.x, lane = threadIdx.x;
  const int k = ks.v[gt.gid[blockIdx.z]];
  if (k <= 0) return;
  {
    const size_t grp = (size_t)gt.gid[blockIdx.z];
    H += grp * m * (restart + 1) * restart;
    g += grp * m * (restart + 1);
    y += grp * restart * m;
  }
  const double* Hc = H + (size_t)c * (restart + 1) * restart;
  const double* gc = g + (size_t)c * (restart + 1);
  double* ys = sm + (size_t)k * 64;
  for (int i = 0; i < k; ++i)
    sm[i * 64 + lane] = (lane < k && lane >= i) ? Hc[(size_t)lane * (restart + 1) + i] : 0.0;
  ys[lane] = 0.0;
  __syncthreads();
  for (int i = k - 1; i >= 0; --i) {
    double part = (lane > i && lane < k) ? sm[i * 64 + lane] * ys[lane] : 0.0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
    if (lane == i) ys[i] = (gc[i] - part) / sm[i * 64 + i];
    __syncthreads();
  }
  if (lane < k) y[lane * m + c] = ys[lane];
}
// the same, one thread per column (cycles longer than a wave: gmres_restart > 63)
__global__ void gmres_backsolve_seq_kernel(GroupTab gt, int m, GroupInts ks, int restart,
                                           const double* __restrict__ H, const double* __restrict__ g,
                                           double* __restrict__ y) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m) return;
  const int k = ks.v[gt.gid[blockIdx.z]];
  {
    const size_t grp = (size_t)gt.gid[blockIdx.z];
    H += grp * m * (restart + 1) * restart;
    g += grp * m * (restart + 1);
    y += grp * restart * m;
  }
  const double* Hc = H + (size_t)c * (restart + 1) * restart;
  const double* gc = g + (size_t)c * (restart + 1);
  for (int i = k - 1; i >= 0; --i) {
    double s = gc[i];
    for (int l = i + 1; l < k; ++l) s -= Hc[(size_t)l * (restart + 1) + i] * y[l * m + c];
    y[i * m + c] = s / Hc[(size_t)i * (restart + 1) + i];
  }
}
void launch_gmres_backsolve_b(hipStream_t st, const GroupTab& gt, int m, const GroupInts& k,
                              int restart, const double* H, const double* g, double* y) {
  if (gt.ng <= 0) return;
  if (restart > 63) {   // (the wave form holds one row per lane)
    hipLaunchKernelGGL(gmres_backsolve_seq_kernel, dim3((m + 63) / 64, 1, gt.ng), dim3(64), 0, st, gt, m, k, restart,
                       H, g, y);
    return;
  }
  hipLaunchKernelGGL(gmres_backsolve_kernel, dim3(m, 1, gt.ng), dim3(64), (size_t)(restart + 1) * 64 * sizeof(double),
                     st, gt, m, k, restart, H, g, y);
}

// start of a cycle: beta[c] = sqrt(nrm2[c]); g = [beta, 0...]; scale = 1/beta
__global__ void gmres_start_kernel(GroupTab gt, int m, int restart,
                                   const double* __restrict__ nrm2, double* __restrict__ g,
                                   double* __restrict__ scale, double* __restrict__ resid) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m) return;
  {
    const size_t grp = (size_t)gt.gid[blockIdx.z];
    nrm2 += grp * m;
    g += grp * m * (restart + 1);
    scale += grp * m;
    resid += grp * m;
  }
  const double b = sqrt(fmax(nrm2[c], 0.0));
  double* gc = g + (size_t)c * (restart + 1);
  for (int i = 0; i <= restart; ++i) gc[i] = 0.0;
  gc[0] = b;
  scale[c] = b > 1e-300 ? 1.0 / b : 0.0;
  resid[c] = b;
}
void launch_gmres_start_b(hipStream_t st, const GroupTab& gt, int m, int restart,
                          const double* nrm2, double* g, double* scale, double* resid) {
  if (gt.ng <= 0) return;
  hipLaunchKernelGGL(gmres_start_kernel, dim3((m + 63) / 64, 1, gt.ng), dim3(64), 0, st, gt, m,
                     restart, nrm2, g, scale, resid);
}

// ---------------------------------------------------------------------------
// K3h: the last Arnoldi pass of the hot path (FP16-stored basis, 16 columns) WITH the Hessenberg / Givens update
// in the same launch -- one dependent launch per iteration less.  Every workgroup derives the normalisation
// 1 / h_{j+1,j} of its 16 columns itself from the (already reduced) Gram-Schmidt coefficients,
//     h_{j+1,j}^2 = ||w'||^2 - sum_i h2_i^2,   frozen columns (converged, or exact breakdown) -> 0,
// so nothing it needs comes from another workgroup of the launch; workgroup 0 of every group ALSO does what
// gmres_hess_kernel did (column of H through the stored rotations, new rotation, g, residual estimate into
// pinned host memory).  The residual estimates are double buffered (resid_in read by everybody, resid_out
// written by workgroup 0): a value that decides "frozen" must not change under the other workgroups' feet.
//   use_sum = 1: w is the vector BEFORE the first projection, coefficients h1 + h2 (cols_update_dots8x_kernel<2, false, .>);
//   use_sum = 0: w has been projected once, coefficients h2.
// ---------------------------------------------------------------------------
// (launch bounds: eight waves per SIMD, what the kernel has always run at -- left alone the allocator lands one VGPR
// above the 64 that takes)
template <class WT>
__global__ __launch_bounds__(256, 8) void cols_update16_hess_kernel(
    GroupTab gt, size_t nhalf, int nvec, const _Float16* __restrict__ basis, size_t vstride, size_t gsb,
    const double* __restrict__ h1, const double* __restrict__ h2, size_t gsh, int use_sum,
    const WT* __restrict__ w, size_t gsw, double* __restrict__ out, size_t gso, _Float16* __restrict__ outf,
    size_t gsf, int j, int restart, double* __restrict__ H, double* __restrict__ cs, double* __restrict__ sn,
    double* __restrict__ g, const double* __restrict__ resid_in, double* __restrict__ resid_out,
    const double* __restrict__ bnorm, double tol, double* __restrict__ host_resid) {
  extern __shared__ double hl[];           // nvec x 16 coefficients, then 16 scales
  const int m = 16;
  const int grp = gt.gid[blockIdx.z];
  basis += (size_t)grp * gsb;
  h1 += (size_t)grp * gsh;
  h2 += (size_t)grp * gsh;
  w += (size_t)grp * gsw;
  if (out) out += (size_t)grp * gso;
  outf += (size_t)grp * gsf;
  double* scl = hl + nvec * m;
  for (int e = threadIdx.x; e < nvec * m; e += 256) hl[e] = use_sum ? h1[e] + h2[e] : h2[e];
  double hnext = 0.0;
  if (threadIdx.x < m) {
    const int c = threadIdx.x;
    double h2sq = 0.0;
    for (int i = 0; i < nvec; ++i) {
      const double b = h2[i * m + c];
      h2sq = fma(b, b, h2sq);
    }
    const double hn2 = h2[nvec * m + c] - h2sq;          // ||w'||^2 before the second projection, minus it
    hnext = hn2 > 0.0 ? sqrt(hn2) : 0.0;
    const double rprev = resid_in[(size_t)grp * m + c];  // |g_j|
    if (column_frozen(hnext, rprev, 0.01 * tol * bnorm[(size_t)grp * m + c])) hnext = 0.0;
    scl[c] = hnext > kTiny ? 1.0 / hnext : 0.0;
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x < m) {
    // the Hessenberg column of this iteration (what gmres_hess_kernel did), one lane per panel column
    const int c = threadIdx.x;
    const size_t gq = (size_t)grp;
    double* Hc = H + gq * m * (restart + 1) * restart + (size_t)c * (restart + 1) * restart + (size_t)j * (restart + 1);
    double* csc = cs + gq * m * restart + (size_t)c * restart;
    double* snc = sn + gq * m * restart + (size_t)c * restart;
    double* gc = g + gq * m * (restart + 1) + (size_t)c * (restart + 1);
    const double gj = gc[j];
    double cur = h1[c] + h2[c];
    for (int i = 0; i < j; ++i) {
      const double nxt = h1[(i + 1) * m + c] + h2[(i + 1) * m + c];
      const double t = csc[i] * cur + snc[i] * nxt;
      const double u = -snc[i] * cur + csc[i] * nxt;
      Hc[i] = t;
      cur = u;
    }
    const double rnew = givens_tail(cur, hnext, gj, j, Hc, csc, snc, gc);
    resid_out[gq * m + c] = rnew;
    if (host_resid) host_resid[gq * m + c] = rnew;
  }
  for (size_t idx = blockIdx.x * (size_t)256 + threadIdx.x; idx < nhalf; idx += (size_t)gridDim.x * 256) {
    const size_t e = idx * 8;
    const int c0 = (int)(idx & 1) * 8;
    double a[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) a[t] = 0.0;
    accum_octet(basis + e, vstride, nvec, hl + c0, m, a);
    if constexpr (sizeof(WT) == 4) {
      const float4* wp = reinterpret_cast<const float4*>(w + e);
      const float4 w0 = wp[0], w1 = wp[1];
      const float wf[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
      for (int t = 0; t < 8; ++t) a[t] = ((double)wf[t] - a[t]) * scl[c0 + t];
    } else {
      const double2* wp = reinterpret_cast<const double2*>(w + e);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double2 ww = wp[t];
        a[2 * t] = (ww.x - a[2 * t]) * scl[c0 + 2 * t];
        a[2 * t + 1] = (ww.y - a[2 * t + 1]) * scl[c0 + 2 * t + 1];
      }
    }
    half8_t f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      f[t] = (_Float16)a[t];
      a[t] = (double)f[t];
    }
    *reinterpret_cast<half8_t*>(outf + e) = f;
    if (out) {
      double2* op = reinterpret_cast<double2*>(out + e);
#pragma unroll
      for (int t = 0; t < 4; ++t) op[t] = make_double2(a[2 * t], a[2 * t + 1]);
    }
  }
}
bool update_hess_fused_ok(int m, bool fp16_basis) { return fp16_basis && m == 16; }
template <class WT>
void launch_cols_update16_hess_b(hipStream_t st, const GroupTab& gt, int nrows, int nvec, const _Float16* basis,
                                 size_t vstride, size_t gsb, const double* h1, const double* h2, size_t gsh, int use_sum,
                                 const WT* w, size_t gsw, double* out, size_t gso, _Float16* outf, size_t gsf, int j,
                                 int restart, double* H, double* cs, double* sn, double* g, const double* resid_in,
                                 double* resid_out, const double* bnorm, double tol, double* host_resid) {
  if (gt.ng <= 0) return;
  const size_t nhalf = (size_t)nrows * 2;
  const int grid = (int)std::min<size_t>((nhalf + 255) / 256, 8192);
  hipLaunchKernelGGL(cols_update16_hess_kernel<WT>, dim3(grid, 1, gt.ng), dim3(256),
                     (size_t)(nvec * 16 + 16) * sizeof(double), st, gt, nhalf, nvec, basis, vstride, gsb, h1, h2, gsh,
                     use_sum, w, gsw, out, gso, outf, gsf, j, restart, H, cs, sn, g, resid_in, resid_out, bnorm, tol,
                     host_resid);
}
// the panel w in FP64 or FP32
#define RICADI_UPDATE16_HESS(WT)                                                                                      \
  template void launch_cols_update16_hess_b(hipStream_t, const GroupTab&, int, int, const _Float16*, size_t, size_t,  \
                                            const double*, const double*, size_t, int, const WT*, size_t, double*,    \
                                            size_t, _Float16*, size_t, int, int, double*, double*, double*, double*,  \
                                            const double*, double*, const double*, double, double*);
RICADI_UPDATE16_HESS(double)
RICADI_UPDATE16_HESS(float)
#undef RICADI_UPDATE16_HESS

// ---------------------------------------------------------------------------
// K3L: the Arnoldi of the hot path (FP16-stored basis, 16 columns, FP32 panel w) in its one-reduction form: delayed
// classical Gram-Schmidt run twice (DCGS2; Swirydowicz et al. 2020, Bielich et al. 2022), three launches per
// iteration (dots, the partial-sum reduction, update) instead of five.  Per column, at iteration j:
//   * V_{j-1} = [v_0 .. v_{j-1}] is orthonormal and final; slot j of the basis holds the candidate u_j, projected
//     ONCE and scaled by a norm estimate 1 / rho_{j-1}; the preconditioner and the operator have made w = S P^-1 u_j;
//   * dots (arnoldi16_lowsync_dots_kernel + reduce_partials_kernel): ONE pass over V_{j-1}, u_j and w gives
//     s = V^T u_j, alpha = u_j^T u_j, t = V^T w, beta = u_j^T w and ||w||^2;
//   * update (arnoldi16_lowsync_update_kernel): every workgroup derives from those sums
//       r_j = sqrt(alpha - ||s||^2)            (the delayed re-orthogonalisation: u_j = V s + r_j v_j),
//       h_jj = (beta - s^T t) / r_j,  rho_j^2 = ||w||^2 - ||t||^2 - h_jj^2,
//     and streams V_{j-1}, u_j and w once, writing v_j = (u_j - V s) / r_j into slot j (in place: row-local) and
//     u_{j+1} = (w - V t - v_j h_jj) / rho_j into slot j+1.  Its workgroup 0 also completes column j-1 of H~,
//     p_{j-1} + rho_{j-1} [s; r_j], applies the stored and the new Givens rotation, updates g, keeps the pending
//     column p_j = [t; h_jj] and rho_j for the next iteration (two buffers by the parity of j: the other workgroups
//     read the previous one), and writes a PROVISIONAL residual estimate for column j (s' = 0, r' = 1 on a copy of the
//     rotations) to the device and pinned host slots -- the host keeps its one-iteration lag; H~ and g only ever
//     hold completed columns.
// rho_j only sets the FP16 storage scale of u_{j+1}: whatever value is used, w = [V, v_j] p_j + rho_j u_{j+1} holds,
// and u_{j+1} = V s' + r' v_{j+1} is measured exactly by the next reduction -- cancellation in the Pythagorean estimate
// cannot corrupt H~, only mis-scale the stored vector, so its range is guarded (floor 1e-3 ||w||, where the estimate
// is at the level of the FP16 basis' own loss of orthogonality).  The last column of a cycle is completed by a dots
// pass without w and arnoldi16_lowsync_close_kernel (each group with its own k_g), so the back substitution only
// sees completed columns.  Frozen columns (|g| <= 0.01 tol ||b|| before the column's rotation, or breakdown) get a
// zero sub-diagonal as in gmres_hess_kernel; the column after a frozen one is made inert (v, u, coefficients zero).
// (An in-launch reduction by the last-arriving workgroup was tried first: with one agent-scope release per
// workgroup over 16 x 468 workgroups the dots launch took 244 us at cfg2, with 48 workgroups per group 62 us.)
// ---------------------------------------------------------------------------
size_t lowsync_partial_stride(int nrows, int restart) { return (size_t)dots_num_blocks(nrows) * 2 * (restart + 2) * 16; }
// per group: the reduced sums [slot][s|t][16] (2 (restart + 2) rows), then two pending columns (p, rho, g before
// the column's rotation: restart + 3 rows each)
size_t lowsync_coef_stride(int restart) { return (size_t)(4 * restart + 10) * 16; }
bool arnoldi16_lowsync_ok(int restart) { return (size_t)((restart + 2) * 32 + 48) * sizeof(double) <= 48 * 1024; }

struct LsPend {
  double *p, *rho, *gj;
  __device__ LsPend(double* coef, int restart, int par)
      : p(coef + 2 * (restart + 2) * 16 + (size_t)par * (restart + 3) * 16), rho(p + (restart + 1) * 16), gj(rho + 16) {}
};

// partial[blk][o], o < ldp: the sums of one 64-row chunk per workgroup for slots V_0 .. V_{j-1}, u_j, w (j = js[group];
// HAS_W = false: the end-of-cycle pass, no w).  u_j and w are staged in LDS once (FP64, rows of stride WLS); lane =
// (row slice sl, column half, slot) as in chunk_dots8x<2>: the 16 lanes of a DPP row hold the 16 row slices of ONE
// (slot, half), and one load of a basis row feeds both sums.  (With u_j and w loaded into registers by every slot's
// lanes instead -- eight times the cache traffic -- the launch took 37 us at cfg2 against 23 us.)
template <bool HAS_W>
__global__ __launch_bounds__(256) void arnoldi16_lowsync_dots_kernel(
    GroupTab gt, GroupInts js, int nrows, int ldp, const _Float16* __restrict__ basis, size_t vstride, size_t gsb,
    const float* __restrict__ w, size_t gsw, double* __restrict__ partial, size_t gsp) {
  __shared__ __attribute__((aligned(16))) double lds[2 * DOT_ROWS * WLS];
  double* ul = lds;
  double* wl = lds + DOT_ROWS * WLS;
  const int grp = gt.gid[blockIdx.z];
  const int j = js.v[grp];
  const int nslot = j + 2;
  basis += (size_t)grp * gsb;
  if (HAS_W) w += (size_t)grp * gsw;
  double* prow = partial + (size_t)grp * gsp + (size_t)blockIdx.x * ldp;
  if (j <= 0 && !HAS_W) return;
  const _Float16* u = basis + (size_t)j * vstride;
  const int r0 = blockIdx.x * DOT_ROWS, nr = min(DOT_ROWS, nrows - r0);
  if (threadIdx.x < DOT_ROWS * 2) {
    const int row = threadIdx.x >> 1, hf = threadIdx.x & 1;
    half8_t x = (half8_t)(_Float16)0;
    if (row < nr) x = *reinterpret_cast<const half8_t*>(u + (size_t)(r0 + row) * 16 + hf * 8);
    double2* d = reinterpret_cast<double2*>(ul + row * WLS + hf * 8);
#pragma unroll
    for (int t = 0; t < 4; ++t) d[t] = make_double2((double)x[2 * t], (double)x[2 * t + 1]);
  }
  {
    const int row = threadIdx.x >> 2, q = threadIdx.x & 3;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (HAS_W && row < nr) x = *reinterpret_cast<const float4*>(w + (size_t)(r0 + row) * 16 + q * 4);
    double2* d = reinterpret_cast<double2*>(wl + row * WLS + q * 4);
    d[0] = make_double2((double)x.x, (double)x.y);
    d[1] = make_double2((double)x.z, (double)x.w);
  }
  for (int e = nslot * 32 + threadIdx.x; e < ldp; e += 256) prow[e] = 0.0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sl = lane & 15, half = (lane >> 4) & 1, vsub = lane >> 5;
  for (int i0 = 0; i0 < nslot; i0 += 8) {
    const int i = i0 + 2 * wave + vsub;
    double as[8], at[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) as[t] = at[t] = 0.0;
    if (i < j) {
      const _Float16* v = basis + (size_t)i * vstride + (size_t)r0 * 16 + half * 8;
      half8_t x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int row = sl + 16 * k;
        if (row < nr) x[k] = *reinterpret_cast<const half8_t*>(v + (size_t)row * 16);
        else x[k] = (half8_t)(_Float16)0;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double* ur = ul + (sl + 16 * k) * WLS + half * 8;
        const double* wr = wl + (sl + 16 * k) * WLS + half * 8;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          const double xv = (double)x[k][t];
          as[t] = fma(xv, ur[t], as[t]);
          at[t] = fma(xv, wr[t], at[t]);
        }
      }
    } else if (i == j) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double* ur = ul + (sl + 16 * k) * WLS + half * 8;
        const double* wr = wl + (sl + 16 * k) * WLS + half * 8;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          as[t] = fma(ur[t], ur[t], as[t]);
          at[t] = fma(ur[t], wr[t], at[t]);
        }
      }
    } else if (i == j + 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double* wr = wl + (sl + 16 * k) * WLS + half * 8;
#pragma unroll
        for (int t = 0; t < 8; ++t) as[t] = fma(wr[t], wr[t], as[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      as[t] = dpp_row_sum(as[t]);
      at[t] = dpp_row_sum(at[t]);
    }
    if (sl == 0 && i < nslot) {
      double2* o = reinterpret_cast<double2*>(prow + (size_t)i * 32 + half * 8);
      double2* o2 = reinterpret_cast<double2*>(prow + (size_t)i * 32 + 16 + half * 8);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        o[t] = make_double2(as[2 * t], as[2 * t + 1]);
        o2[t] = make_double2(at[2 * t], at[2 * t + 1]);
      }
    }
  }
}

// Column c of group grp, from the reduced sums: completes column j-1 of H~ (when `complete`), returns the update's
// coefficients.  Every caller derives the same values from the same inputs.
struct LsCoefs {
  double invr, hjj, sig;
  bool dead;
};
__device__ LsCoefs ls_column(const double* sums, int j, int c, int restart, double* coef, double thr, bool complete,
                             bool with_w, double* Hcol, double* csc, double* snc, double* gc, double* resid_out,
                             double* host_resid) {
  const double tiny = 1e-300;
  auto S = [&](int i) { return sums[i * 32 + c]; };
  auto T = [&](int i) { return sums[i * 32 + 16 + c]; };
  double r = 1.0;                           // v_0 = u_0 (the cycle start normalised it)
  bool dead = false;                        // column j-1 frozen or broken down: column j is inert
  if (j > 0) {
    const LsPend pp(coef, restart, (j - 1) & 1);
    double ssq = 0.0;
    for (int i = 0; i < j; ++i) ssq = fma(S(i), S(i), ssq);
    const double r2 = S(j) - ssq;
    r = r2 > 0.0 ? sqrt(r2) : 0.0;
    const double rho = pp.rho[c], gj = pp.gj[c];
    double sub = rho * r;
    dead = column_frozen(sub, fabs(gj), thr);
    if (complete) {
      // column j-1:  p_{j-1} + rho_{j-1} [s; r]
      if (dead) sub = 0.0;
      double* Hc = Hcol + (size_t)(j - 1) * (restart + 1);
      double cur = fma(rho, S(0), pp.p[c]);
      for (int i = 0; i + 1 < j; ++i) {
        const double nxt = fma(rho, S(i + 1), pp.p[(i + 1) * 16 + c]);
        Hc[i] = csc[i] * cur + snc[i] * nxt;
        cur = -snc[i] * cur + csc[i] * nxt;
      }
      (void)givens_tail(cur, sub, gj, j - 1, Hc, csc, snc, gc);
    }
  }
  LsCoefs o{0.0, 0.0, 0.0, dead};
  if (!with_w) return o;
  o.invr = (!dead && r > tiny) ? 1.0 / r : 0.0;
  double st = 0.0, tsq = 0.0;
  for (int i = 0; i < j; ++i) {
    st = fma(S(i), T(i), st);
    tsq = fma(T(i), T(i), tsq);
  }
  const double hjj = (T(j) - st) * o.invr;
  const double ww = S(j + 1);
  const double wn = sqrt(fmax(ww, 0.0));
  const double rho2 = ww - tsq - hjj * hjj;
  double rho = fmax(rho2 > 0.0 ? sqrt(rho2) : 0.0, 1e-3 * wn);
  if (dead || !(rho > tiny)) rho = 0.0;
  o.hjj = dead ? 0.0 : hjj;
  o.sig = rho > 0.0 ? 1.0 / rho : 0.0;
  if (complete) {
    // pending column j, and the provisional residual estimate after it (s' = 0, r' = 1) on a copy of the rotations
    const LsPend pn(coef, restart, j & 1);
    for (int i = 0; i < j; ++i) pn.p[i * 16 + c] = dead ? 0.0 : T(i);
    pn.p[j * 16 + c] = o.hjj;
    pn.rho[c] = rho;
    const double gj = gc[j];
    pn.gj[c] = gj;
    const double sub = (dead || fabs(gj) <= thr) ? 0.0 : rho;
    double cur = dead ? 0.0 : (j > 0 ? T(0) : o.hjj);
    for (int i = 0; i < j; ++i) {
      const double nxt = dead ? 0.0 : (i + 1 < j ? T(i + 1) : o.hjj);
      cur = -snc[i] * cur + csc[i] * nxt;
    }
    const double d = hypot(cur, sub);
    const double rnew = (d > tiny) ? fabs(sub / d * gj) : 0.0;
    resid_out[c] = rnew;
    if (host_resid) host_resid[c] = rnew;
  }
  return o;
}

__global__ __launch_bounds__(256) void arnoldi16_lowsync_update_kernel(
    GroupTab gt, size_t nhalf, int j, _Float16* __restrict__ basis, size_t vstride, size_t gsb,
    const float* __restrict__ w, size_t gsw, double* __restrict__ coef, size_t gsc, int restart,
    double* __restrict__ H, double* __restrict__ cs, double* __restrict__ sn, double* __restrict__ g,
    const double* __restrict__ bnorm, double tol, double* __restrict__ resid_out, double* __restrict__ host_resid) {
  extern __shared__ double cl[];           // the reduced sums [slot][s|t][16] (slots 0 .. j+1), then invr, hjj, sig
  const int m = 16;
  const int grp = gt.gid[blockIdx.z];
  basis += (size_t)grp * gsb;
  w += (size_t)grp * gsw;
  coef += (size_t)grp * gsc;
  const int nsum = (j + 2) * 32;
  double* sums = cl;
  double* il = cl + nsum;                  // invr, hjj, sig: 16 each
  for (int e = threadIdx.x; e < nsum; e += 256) sums[e] = coef[e];
  __syncthreads();
  if (threadIdx.x < m) {
    const int c = threadIdx.x;
    const size_t gq = (size_t)grp;
    const bool w0 = blockIdx.x == 0;
    const LsCoefs k = ls_column(sums, j, c, restart, coef, 0.01 * tol * bnorm[gq * m + c], w0, true,
                                H + gq * m * (restart + 1) * restart + (size_t)c * (restart + 1) * restart,
                                cs + gq * m * restart + (size_t)c * restart, sn + gq * m * restart + (size_t)c * restart,
                                g + gq * m * (restart + 1) + (size_t)c * (restart + 1), resid_out + gq * m,
                                host_resid ? host_resid + gq * m : nullptr);
    il[c] = k.invr;
    il[m + c] = k.hjj;
    il[2 * m + c] = k.sig;
  }
  __syncthreads();
  _Float16* uj = basis + (size_t)j * vstride;
  _Float16* un = uj + vstride;
  for (size_t idx = blockIdx.x * (size_t)256 + threadIdx.x; idx < nhalf; idx += (size_t)gridDim.x * 256) {
    const size_t e = idx * 8;
    const int c0 = (int)(idx & 1) * 8;
    double as[8], at[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) as[t] = at[t] = 0.0;
    const _Float16* v = basis + e;
    int i = 0;
    for (; i + 3 < j; i += 4) {
      half8_t x[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) x[q] = *reinterpret_cast<const half8_t*>(v + (size_t)(i + q) * vstride);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < 8; ++t) {
          as[t] = fma(sums[(i + q) * 32 + c0 + t], (double)x[q][t], as[t]);
          at[t] = fma(sums[(i + q) * 32 + 16 + c0 + t], (double)x[q][t], at[t]);
        }
    }
    for (; i < j; ++i) {
      const half8_t x = *reinterpret_cast<const half8_t*>(v + (size_t)i * vstride);
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        as[t] = fma(sums[i * 32 + c0 + t], (double)x[t], as[t]);
        at[t] = fma(sums[i * 32 + 16 + c0 + t], (double)x[t], at[t]);
      }
    }
    const half8_t uu = *reinterpret_cast<const half8_t*>(uj + e);
    const float4* wp = reinterpret_cast<const float4*>(w + e);
    const float4 w0 = wp[0], w1 = wp[1];
    const float wf[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    half8_t fv, fu;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      fv[t] = (_Float16)(((double)uu[t] - as[t]) * il[c0 + t]);
      // the stored (rounded) v_j: w = [V, v_j] p_j + rho_j u_{j+1} holds for the vectors as stored
      fu[t] = (_Float16)(((double)wf[t] - at[t] - (double)fv[t] * il[m + c0 + t]) * il[2 * m + c0 + t]);
    }
    *reinterpret_cast<half8_t*>(uj + e) = fv;
    *reinterpret_cast<half8_t*>(un + e) = fu;
  }
}

// end of a cycle: completes column k_g - 1 of every group from the sums of the dots pass without w
__global__ __launch_bounds__(64) void arnoldi16_lowsync_close_kernel(
    GroupTab gt, GroupInts ks, double* __restrict__ coef, size_t gsc, int restart, double* __restrict__ H,
    double* __restrict__ cs, double* __restrict__ sn, double* __restrict__ g, const double* __restrict__ bnorm,
    double tol) {
  const int m = 16;
  const int grp = gt.gid[blockIdx.z];
  const int k = ks.v[grp];
  const int c = threadIdx.x;
  if (k <= 0 || c >= m) return;
  const size_t gq = (size_t)grp;
  coef += gq * gsc;
  (void)ls_column(coef, k, c, restart, coef, 0.01 * tol * bnorm[gq * m + c], true, false,
                  H + gq * m * (restart + 1) * restart + (size_t)c * (restart + 1) * restart,
                  cs + gq * m * restart + (size_t)c * restart, sn + gq * m * restart + (size_t)c * restart,
                  g + gq * m * (restart + 1) + (size_t)c * (restart + 1), nullptr, nullptr);
}

void launch_arnoldi16_lowsync_dots(hipStream_t st, const GroupTab& gt, const GroupInts& js, int nrows,
                                   const _Float16* basis, size_t vstride, size_t gsb, const float* w32, size_t gsw,
                                   double* partial, size_t gsp, double* coef, size_t gsc) {
  if (gt.ng <= 0) return;
  int jmax = 0;
  for (int z = 0; z < gt.ng; ++z) jmax = std::max(jmax, js.v[gt.gid[z]]);
  const int nblk = dots_num_blocks(nrows), ldp = (jmax + 2) * 32;
  if (w32)
    hipLaunchKernelGGL(arnoldi16_lowsync_dots_kernel<true>, dim3(nblk, 1, gt.ng), dim3(256), 0, st, gt, js, nrows, ldp,
                       basis, vstride, gsb, w32, gsw, partial, gsp);
  else
    hipLaunchKernelGGL(arnoldi16_lowsync_dots_kernel<false>, dim3(nblk, 1, gt.ng), dim3(256), 0, st, gt, js, nrows,
                       ldp, basis, vstride, gsb, w32, gsw, partial, gsp);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((ldp + 15) / 16, 1, gt.ng), dim3(256), 0, st, gt, nblk, ldp, partial,
                     gsp, coef, gsc, 0);
}
void launch_arnoldi16_lowsync_update(hipStream_t st, const GroupTab& gt, int nrows, int j, _Float16* basis,
                                     size_t vstride, size_t gsb, const float* w32, size_t gsw, double* coef,
                                     size_t gsc, int restart, double* H, double* cs, double* sn, double* g,
                                     const double* bnorm, double tol, double* resid_out, double* host_resid) {
  if (gt.ng <= 0) return;
  const size_t nhalf = (size_t)nrows * 2;
  const int grid = (int)std::min<size_t>((nhalf + 255) / 256, 8192);
  hipLaunchKernelGGL(arnoldi16_lowsync_update_kernel, dim3(grid, 1, gt.ng), dim3(256),
                     (size_t)((j + 2) * 32 + 48) * sizeof(double), st, gt, nhalf, j, basis, vstride, gsb, w32, gsw, coef,
                     gsc, restart, H, cs, sn, g, bnorm, tol, resid_out, host_resid);
}
void launch_arnoldi16_lowsync_close(hipStream_t st, const GroupTab& gt, const GroupInts& ks, double* coef, size_t gsc,
                                    int restart, double* H, double* cs, double* sn, double* g, const double* bnorm,
                                    double tol) {
  if (gt.ng <= 0) return;
  hipLaunchKernelGGL(arnoldi16_lowsync_close_kernel, dim3(1, 1, gt.ng), dim3(64), 0, st, gt, ks, coef, gsc, restart, H,
                     cs, sn, g, bnorm, tol);
}

}  // namespace ricadi
