// ricadi_radi.hip -- the dense part of a RADI step (solver_radi.inl).
//
// After the shift solve  [[cal A - U B^T + p cal E, J^T], [J, 0]] [V; *] = [R; 0]  a step needs
//   G = V^T B (m x nb),   Y = I + G G^T = L L^T,
//   Z <- [Z, sqrt(-2p) V L^-T],   T = (-2p) V Y^-1,   R <- R + cal E T,   U <- U + (cal E T) G.
// Three kernels:
//   radi_vtb_kernel / radi_vtb_reduce_kernel   G, a tall-skinny product: one partial per row slice, the slices summed
//                                              in slice order;
//   radi_factor_kernel                         one workgroup: Y, its Cholesky factor, L^-1 and the coefficient matrix
//                                              C = [sqrt(-2p) L^-T | (-2p) Y^-1 | (-2p) Y^-1 G]  (m x (2m + nb));
//   radi_update_kernel                         one pass over the rows of cal E: (cal E V)_row and V_row times C, added
//                                              into the panel [R | U] and written as the new block of Z.
// With shifts generated from the iteration (ricadi_set_radi_shifts) a step also needs
//   radi_reduce_kernel                         H = Q^T [cal A Q | cal E Q | R | U | B] for an orthonormal basis Q of the
//                                              new block of Z: one pass over the rows of cal A and cal E, one partial
//                                              per row slice, the slices summed by radi_vtb_reduce_kernel;
//   radi_reduce_wide_kernel<GROUP>             the same for blocks of 33 .. 127 columns: the
//                                              output tiled over workgroups, on the FP64 matrix cores.
// The sweep form (G steps as one lockstep batch of solves) replaces the last two by
//   radi_sweep_combine_kernel                  Z block = Vh Cf[:, :k m], [R | U] += (cal E Vh) Cf[:, k m:] for the dense
//                                              coefficient matrix the host makes of the sweep's small matrices, on the
//                                              FP64 matrix cores.
// FP64 throughout, no atomics, every sum in a fixed order: the same inputs give bitwise the same outputs.
#include "ricadi_internal.h"
#include "ricadi_device.h"

namespace ricadi {

// ---- G = V^T B ------------------------------------------------------------------------------------------------------
// part[s][i nb + j] = sum over the rows of slice s, in row order, of V[r, i] B[r, j]
__global__ __launch_bounds__(256) void radi_vtb_kernel(int n, int m, int nb, const double* __restrict__ V, int ldv,
                                                       const double* __restrict__ B, int rows_per_slice,
                                                       double* __restrict__ part) {
  const int r0 = blockIdx.x * rows_per_slice, r1 = min(n, r0 + rows_per_slice);
  const int mn = m * nb;
  for (int e = threadIdx.x; e < mn; e += 256) {
    const int i = e / nb, j = e - i * nb;
    double s = 0.0;
    for (int r = r0; r < r1; ++r) s = fma(V[(size_t)r * ldv + i], B[(size_t)r * nb + j], s);
    part[(size_t)blockIdx.x * mn + e] = s;
  }
}
__global__ __launch_bounds__(256) void radi_vtb_reduce_kernel(int slices, int mn, const double* __restrict__ part,
                                                              double* __restrict__ G) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= mn) return;
  double s = 0.0;
  for (int w = 0; w < slices; ++w) s += part[(size_t)w * mn + e];
  G[e] = s;
}
// row slices: 64 rows or more each, at most 1024 of them
static int radi_vtb_slices(int n, int& rows_per_slice) {
  const int want = std::max(1, std::min((n + 63) / 64, 1024));
  rows_per_slice = (n + want - 1) / want;
  return (n + rows_per_slice - 1) / rows_per_slice;
}
size_t radi_vtb_partial_len(int n, int m, int nb) {
  int rps = 0;
  return (size_t)radi_vtb_slices(std::max(n, 1), rps) * m * nb;
}
void launch_radi_vtb(hipStream_t st, int n, int m, int nb, const double* V, int ldv, const double* B, double* partial,
                     double* G) {
  int rps = 0;
  const int slices = radi_vtb_slices(n, rps);
  hipLaunchKernelGGL(radi_vtb_kernel, dim3(slices), dim3(256), 0, st, n, m, nb, V, ldv, B, rps, partial);
  hipLaunchKernelGGL(radi_vtb_reduce_kernel, dim3((m * nb + 255) / 256), dim3(256), 0, st, slices, m * nb, partial, G);
}

// ---- Y = I + G G^T, its factor, the coefficient matrix -----------------------------------------------------------------
// One workgroup; A (LDS, m rows of ld = (m + 1) | 1 doubles -- odd, so that a column walk touches every bank) holds
//   the lower triangle of Y, then L in its place;
//   X = L^-1 beside it: X[i][j] (i >= j) at A[j][i + 1] -- row j behind its diagonal, i.e. L^-T by rows;
//   the lower triangle of (-2p) Y^-1 over L once X is complete.
// A pivot that is not positive and finite raises *flag (Y >= I for finite G: it means NaN / Inf in the solve); C is
// left unwritten then.
__global__ __launch_bounds__(256) void radi_factor_kernel(int m, int nb, double p, const double* __restrict__ G,
                                                          double* __restrict__ C, int* __restrict__ flag) {
  extern __shared__ double A[];
  __shared__ int bad;
  const int tid = threadIdx.x;
  const int ld = (m + 1) | 1, ldc = 2 * m + nb;
  if (tid == 0) bad = 0;
  for (int e = tid; e < m * m; e += 256) {
    const int i = e / m, j = e - i * m;
    if (j > i) continue;
    double s = 0.0;
    for (int k = 0; k < nb; ++k) s = fma(G[i * nb + k], G[j * nb + k], s);
    A[i * ld + j] = i == j ? 1.0 + s : s;
  }
  __syncthreads();
  // right-looking Cholesky, column by column
  for (int k = 0; k < m; ++k) {
    if (tid == 0) {
      const double d = A[k * ld + k];
      if (d > 0.0 && d <= 1.7976931348623157e308) A[k * ld + k] = sqrt(d);
      else bad = 1;
    }
    __syncthreads();
    if (bad) break;          // (uniform: the next write of `bad` is behind this iteration's last barrier)
    const double dk = A[k * ld + k];
    for (int i = k + 1 + tid; i < m; i += 256) A[i * ld + k] /= dk;
    __syncthreads();
    const int t = m - k - 1;
    for (int e = tid; e < t * t; e += 256) {
      const int a = e / t, b = e - a * t;
      if (b <= a) A[(k + 1 + a) * ld + k + 1 + b] -= A[(k + 1 + a) * ld + k] * A[(k + 1 + b) * ld + k];
    }
    __syncthreads();
  }
  if (bad) {
    if (tid == 0) *flag = 1;
    return;
  }
  // X = L^-1 by forward substitution, thread j its column j
  if (tid < m) {
    const int j = tid;
    double* xr = A + j * ld + 1;          // xr[i] = X[i][j]
    xr[j] = 1.0 / A[j * ld + j];
    for (int i = j + 1; i < m; ++i) {
      double s = 0.0;
      for (int k = j; k < i; ++k) s = fma(A[i * ld + k], xr[k], s);
      xr[i] = -s / A[i * ld + i];
    }
  }
  __syncthreads();
  const double s2 = -2.0 * p, s1 = sqrt(s2);
  // C1 = sqrt(-2p) L^-T; lower triangle of C2 = (-2p) X^T X (kept in LDS over L, written to both halves of C)
  for (int e = tid; e < m * m; e += 256) {
    const int a = e / m, b = e - a * m;
    C[a * ldc + b] = b >= a ? s1 * A[a * ld + b + 1] : 0.0;
    if (b > a) continue;
    double s = 0.0;
    for (int k = a; k < m; ++k) s = fma(A[a * ld + k + 1], A[b * ld + k + 1], s);
    s *= s2;
    C[a * ldc + m + b] = s;
    C[b * ldc + m + a] = s;
    A[a * ld + b] = s;          // (over L, which nothing reads any more; X lies behind the diagonal of its row)
  }
  __syncthreads();
  // C3 = C2 G
  for (int e = tid; e < m * nb; e += 256) {
    const int a = e / nb, j = e - a * nb;
    double s = 0.0;
    for (int b = 0; b < m; ++b) s = fma(b <= a ? A[a * ld + b] : A[b * ld + a], G[b * nb + j], s);
    C[a * ldc + 2 * m + j] = s;
  }
}
void launch_radi_factor(hipStream_t st, int m, int nb, double p, const double* G, double* C, int* flag) {
  const int ld = (m + 1) | 1;
  const size_t lds = sizeof(double) * (size_t)m * ld;
  static bool attr_set = false;
  if (lds > 65536 && !attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(radi_factor_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * 127 * 129));   // m = 127
    attr_set = true;
  }
  hipLaunchKernelGGL(radi_factor_kernel, dim3(1), dim3(256), lds, st, m, nb, p, G, C, flag);
}

// ---- the fused update ------------------------------------------------------------------------------------------------
// A workgroup owns RADI_RB rows: it gathers (cal E V)_row and V_row into LDS once, then walks C in column tiles of
// RADI_CT (C at the widest shape, 127 x 318 doubles, does not fit in LDS): columns [0, m) of C give the Z block from
// V_row, columns [m, 2m + nb) are added into [R | U] from (cal E V)_row.  LDS: (2 RADI_RB + RADI_CT) m doubles <= 64 KB
// for m <= 127.
constexpr int RADI_RB = 16, RADI_CT = 32;
__global__ __launch_bounds__(256) void radi_update_kernel(int nv, int m, int nb, const int* __restrict__ rp,
                                                          const int* __restrict__ ci, const double* __restrict__ ev,
                                                          const double* __restrict__ V, int ldv,
                                                          const double* __restrict__ C, double* __restrict__ RU,
                                                          double* __restrict__ Z, int zld, int zc) {
  extern __shared__ double sh[];
  double* vs = sh;                         // RADI_RB x m: the rows of V
  double* es = sh + RADI_RB * m;           // RADI_RB x m: the rows of cal E V
  double* ct = es + RADI_RB * m;           // m x RADI_CT: a column tile of C
  const int tid = threadIdx.x;
  const int row0 = blockIdx.x * RADI_RB, nr = min(RADI_RB, nv - row0);
  const int ldc = 2 * m + nb, ldp = m + nb;
  for (int e = tid; e < RADI_RB * m; e += 256) {
    const int r = e / m, c = e - r * m;
    double v = 0.0, s = 0.0;
    if (r < nr) {
      const int row = row0 + r;
      v = V[(size_t)row * ldv + c];
      for (int q = rp[row]; q < rp[row + 1]; ++q) s = fma(ev[q], V[(size_t)ci[q] * ldv + c], s);
    }
    vs[e] = v;
    es[e] = s;
  }
  for (int j0 = 0; j0 < ldc; j0 += RADI_CT) {
    const int w = min(RADI_CT, ldc - j0);
    __syncthreads();
    for (int e = tid; e < m * RADI_CT; e += 256) {
      const int c = e / RADI_CT, j = e - c * RADI_CT;
      ct[e] = j < w ? C[(size_t)c * ldc + j0 + j] : 0.0;
    }
    __syncthreads();
    for (int e = tid; e < RADI_RB * RADI_CT; e += 256) {
      const int r = e / RADI_CT, j = e - r * RADI_CT;
      if (r >= nr || j >= w) continue;
      const int jg = j0 + j;
      const double* a = (jg < m ? vs : es) + r * m;
      double s = 0.0;
      for (int c = 0; c < m; ++c) s = fma(a[c], ct[c * RADI_CT + j], s);
      const size_t row = (size_t)(row0 + r);
      if (jg < m) Z[row * zld + zc + jg] = s;
      else RU[row * ldp + jg - m] += s;
    }
  }
}
void launch_radi_update(hipStream_t st, int nv, int m, int nb, const int* rp, const int* ci, const double* ev,
                        const double* V, int ldv, const double* C, double* RU, double* Z, int zld, int zc) {
  if (nv <= 0) return;
  const size_t lds = sizeof(double) * (size_t)(2 * RADI_RB + RADI_CT) * m;
  hipLaunchKernelGGL(radi_update_kernel, dim3((nv + RADI_RB - 1) / RADI_RB), dim3(256), lds, st, nv, m, nb, rp, ci, ev,
                     V, ldv, C, RU, Z, zld, zc);
}

// ---- the recombination of a sweep ---------------------------------------------------------
// Z[:, zc : zc + k m] = Vh Cf[:, :k m]  and  [R | U] += S Cf[:, k m:]  in one pass over the velocity rows: Vh = the G
// solution panels side by side (panel g at V + g vstride, leading dimension ldv, its first m columns), S = cal E Vh
// (nv x K, K = G m <= 128, leading dimension lds), Cf K x (k m + m + nb) row-major -- the dense generalisation of
// launch_sweep_combine, whose coefficient is (G x G) (x) I_m.
// grid = (chunks of 64 rows, column tiles of RADI_SCT = 64 output columns): the first ceil(k m / 64) tiles are columns
// of the Z block (A operand: rows of Vh), the others columns of [R | U] (A operand: rows of S).  A wave owns 16 rows
// and the tile's four 16-column fragments: v_mfma_f64_16x16x4_f64 with gemm_nn's fragment maps (lane l holds
// A[row l & 15][k l >> 4], B[k l >> 4][col l & 15], D[row (l >> 4) + 4 reg][col l & 15]), K / 4 instructions per
// fragment, k ascending.  Cf's columns are tiled over workgroups and its B fragments are read where they lie: the
// whole matrix is at most 128 x 208 doubles, every wave of a tile reads the same 64 KB of it and it stays in L2 / the
// vector L1; an LDS stage would save a fourth of that traffic and cost a barrier per tile.  The rows of Vh / S are read
// once per column tile (at most four tiles).  No atomics, no reduction across waves: bitwise reproducible.
// The A fragments are strided loads: the sixteen lanes of a k-step read sixteen different rows at stride ldv / lds,
// 32 contiguous bytes (four k) of each, and every column tile reads the row block again.  At K <= 128 and 0.06 ms per
// sweep (n = 3e4) that is not what a sweep waits for; if K or nv grow, staging the 64 x K row block in LDS once per
// workgroup (coalesced row reads, shared by the column tiles) is the lever.
constexpr int RADI_SCT = 64;
__global__ __launch_bounds__(256) void radi_sweep_combine_kernel(int nv, int G, int m, int nb, int k,
                                                                 const double* __restrict__ V, size_t vstride, int ldv,
                                                                 const double* __restrict__ S, int lds,
                                                                 const double* __restrict__ Cf,
                                                                 double* __restrict__ RU, double* __restrict__ Z,
                                                                 int zld, int zc) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, lk = lane >> 4;
  const int K = G * m, km = k * m, ldp = m + nb, ldc = km + ldp;
  const int nzt = (km + RADI_SCT - 1) / RADI_SCT;
  const bool zt = (int)blockIdx.y < nzt;
  const int j0 = RADI_SCT * (zt ? (int)blockIdx.y : (int)blockIdx.y - nzt);    // first column inside Z block / [R | U]
  const int ncol = zt ? km : ldp, coff = zt ? 0 : km;                          // columns there; their offset in Cf
  const int row0 = (blockIdx.x * 4 + wave) * 16;
  if (row0 >= nv) return;
  const int arow = row0 + lc;
  const bool aok = arow < nv;
  d4 acc[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) acc[b] = (d4){0.0, 0.0, 0.0, 0.0};
  int g = lk / m, c = lk - g * m;                                              // kk = g m + c
  for (int kk0 = 0; kk0 < K; kk0 += 4) {
    const int kk = kk0 + lk;
    const bool kok = kk < K;
    double af = 0.0;
    if (aok && kok) af = zt ? V[(size_t)g * vstride + (size_t)arow * ldv + c] : S[(size_t)arow * lds + kk];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int col = j0 + 16 * b + lc;
      const double bf = (kok && col < ncol) ? Cf[(size_t)kk * ldc + coff + col] : 0.0;
      acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf, acc[b], 0, 0, 0);
    }
    c += 4;
    while (c >= m) {
      c -= m;
      ++g;
    }
  }
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int row = row0 + lk + 4 * e, col = j0 + 16 * b + lc;
      if (row >= nv || col >= ncol) continue;
      if (zt) Z[(size_t)row * zld + zc + col] = acc[b][e];
      else RU[(size_t)row * ldp + col] += acc[b][e];
    }
}
void launch_radi_sweep_combine(hipStream_t st, int nv, int G, int m, int nb, int k, const double* V, size_t vstride,
                               int ldv, const double* S, int lds, const double* Cf, double* RU, double* Z, int zld,
                               int zc) {
  if (nv <= 0) return;
  const int tiles = (k * m + RADI_SCT - 1) / RADI_SCT + (m + nb + RADI_SCT - 1) / RADI_SCT;
  hipLaunchKernelGGL(radi_sweep_combine_kernel, dim3((nv + 63) / 64, tiles), dim3(256), 0, st, nv, G, m, nb, k, V,
                     vstride, ldv, S, lds, Cf, RU, Z, zld, zc);
}

// ---- the reduced matrices of the shift selection ------------------------------------------------------------------
// H = Q^T [cal A Q | cal E Q | R | U | B]  (k x W, W = 2k + m + 2nb, row-major; k = m <= 32, nb <= 64) in one pass over
// the velocity rows of the saddle pattern (rp / ci, columns below nv only) with its two value sources vA / vE.
// A workgroup owns a slice of rows (a multiple of RADI_HB) and walks it in chunks of RADI_HB rows.  Per chunk it
//   1. gathers the Q rows the chunk's sparse rows name and forms (cal A Q)_row and (cal E Q)_row, copies the rows of
//      [R | U] and B beside them -- the row Y_r of W entries -- and its own rows of Q, all into LDS;
//   2. adds Q_r^T Y_r into registers: thread = (sub, column j) holds H[0 .. k)[j] of the rows r = sub (mod nsub) of
//      every chunk, nsub = min(256 / W, RADI_HB), in row order.
// At the end the nsub partial sums of a column are added in sub order through LDS, and radi_vtb_reduce_kernel adds the
// slices in slice order: no atomics, every sum in a fixed order.
// LDS (doubles): RADI_HB (ldy + ldq) + (nsub > 1 ? k W : 0), ldy = W | 1, ldq = k | 1 (odd: the gather phase writes
// and the sum phase reads along rows, a later column walk would touch every bank); nsub > 1 means W <= 128, so at most
// 16 * (129 + 33) + 32 * 128 doubles = 53 KB, and 16 * (225 + 33) = 33 KB for the widest W = 224.
constexpr int RADI_HB = 16, RADI_HK = 32;
__global__ __launch_bounds__(256) void radi_reduce_kernel(int nv, int k, int m, int nb, int rows_per_slice, int nsub,
                                                          const int* __restrict__ rp, const int* __restrict__ ci,
                                                          const double* __restrict__ vA,
                                                          const double* __restrict__ vE,
                                                          const double* __restrict__ Q,
                                                          const double* __restrict__ RU,
                                                          const double* __restrict__ B, double* __restrict__ part) {
  extern __shared__ double sh[];
  const int W = 2 * k + m + 2 * nb, ldy = W | 1, ldq = k | 1, ldp = m + nb;
  double* ys = sh;                          // RADI_HB x ldy
  double* qs = ys + RADI_HB * ldy;          // RADI_HB x ldq
  double* red = qs + RADI_HB * ldq;         // k x W (nsub > 1 only)
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * rows_per_slice, r1 = min(nv, r0 + rows_per_slice);
  const bool summing = tid < nsub * W;
  const int sub = summing ? tid / W : 0, j = summing ? tid - sub * W : 0;
  double acc[RADI_HK];
#pragma unroll
  for (int i = 0; i < RADI_HK; ++i) acc[i] = 0.0;
  for (int row0 = r0; row0 < r1; row0 += RADI_HB) {
    const int nr = min(RADI_HB, r1 - row0);
    for (int e = tid; e < RADI_HB * k; e += 256) {
      const int r = e / k, c = e - r * k;
      double a = 0.0, s = 0.0, q = 0.0;
      if (r < nr) {
        const int row = row0 + r;
        q = Q[(size_t)row * k + c];
        const int p1 = rp[row + 1];
#pragma unroll 4
        for (int p = rp[row]; p < p1; ++p) {
          const int col = ci[p];
          const double qv = col < nv ? Q[(size_t)col * k + c] : 0.0;      // (beyond nv: the J^T part of the saddle row)
          a = fma(vA[p], qv, a);
          s = fma(vE[p], qv, s);
        }
      }
      ys[r * ldy + c] = a;
      ys[r * ldy + k + c] = s;
      qs[r * ldq + c] = q;
    }
    for (int e = tid; e < RADI_HB * ldp; e += 256) {
      const int r = e / ldp, c = e - r * ldp;
      ys[r * ldy + 2 * k + c] = r < nr ? RU[(size_t)(row0 + r) * ldp + c] : 0.0;
    }
    for (int e = tid; e < RADI_HB * nb; e += 256) {
      const int r = e / nb, c = e - r * nb;
      ys[r * ldy + 2 * k + ldp + c] = r < nr ? B[(size_t)(row0 + r) * nb + c] : 0.0;
    }
    __syncthreads();
    if (summing) {
      for (int r = sub; r < nr; r += nsub) {
        const double y = ys[r * ldy + j];
        const double* qr = qs + r * ldq;
#pragma unroll
        for (int i = 0; i < RADI_HK; ++i)
          if (i < k) acc[i] = fma(qr[i], y, acc[i]);
      }
    }
    __syncthreads();
  }
  double* out = part + (size_t)blockIdx.x * k * W;
  if (nsub == 1) {
    if (summing) {
#pragma unroll
      for (int i = 0; i < RADI_HK; ++i)
        if (i < k) out[i * W + j] = acc[i];
    }
    return;
  }
  for (int s = 0; s < nsub; ++s) {          // the sub-sums of a column, in sub order
    if (summing && sub == s) {
#pragma unroll
      for (int i = 0; i < RADI_HK; ++i)
        if (i < k) red[i * W + j] = s == 0 ? acc[i] : red[i * W + j] + acc[i];
    }
    __syncthreads();
  }
  for (int e = tid; e < k * W; e += 256) out[e] = red[e];
}
// row slices: 64 rows or more each (a multiple of RADI_HB), at most 1024 of them
static int radi_reduce_slices(int n, int& rows_per_slice) {
  const int want = std::max(1, std::min((n + 63) / 64, 1024));
  rows_per_slice = RADI_HB * (((n + want - 1) / want + RADI_HB - 1) / RADI_HB);
  return (n + rows_per_slice - 1) / rows_per_slice;
}
// ---- the same for a wide block: 33 <= k = m <= 127, W = 3m + 2nb <= 509 ---------------------------------------------
// k W <= 64 643 outputs are too many for per-thread accumulators, so the output is tiled over workgroups:
// grid = (row slices, column tiles).  A column tile holds RADI_WCT = 64 columns of Y = [cal A Q | cal E Q | R | U | B]
// and all k rows of H:
//   tile t < ngt = ceil(k / 32) ("gather tile"):  columns [32t, 32t + 32) of cal A Q AND of cal E Q, so that one walk
//       over a sparse row and ONE gather of Q serve both, as in the narrow kernel; every entry of the two products is
//       formed once -- no gather is repeated across tiles, only the row's index / value stream is read by each of
//       the ngt gather tiles (2 at m = 58, 4 at m = 127);
//   tile t >= ngt ("dense tile"):  columns [64 (t - ngt), ..) of [R | U | B]: plain copies, no gather.
// Per chunk of RADI_WB = 16 rows a workgroup puts its own rows of Q (16 x k, zero-padded to a multiple of 16 columns)
// and the tile's rows of Y (16 x 64) into LDS; wave w owns the tile's columns [16w, 16w + 16) and all ceil(k / 16) <= 8
// row tiles of H: Q_chunk^T Y_chunk on v_mfma_f64_16x16x4_f64, four instructions of depth 4 per row tile and chunk,
// the chunks of the slice in row order.  One partial per row slice, the slices summed in slice order by
// radi_vtb_reduce_kernel: no atomics, every sum in a fixed order.
// LDS (static): 16 x 144 + 16 x 80 doubles = 28 KB (leading dimensions = 16 mod 32 doubles: the four rows a wave
// reads at once fall into different banks).
// GROUP: the basis is a GROUP of c = k columns of Z against a residual of m != k columns
// (W = 2k + m + 2nb <= 509): the same tiles, chunks and summation order, the dense tiles cover m + 2nb columns.  The
// instantiation without it is the kernel of a single wide block (m_arg unused), its code and bits as before.
constexpr int RADI_WB = 16, RADI_WCT = 64, RADI_WLQ = 144, RADI_WLY = 80;
template <bool GROUP>
__global__ __launch_bounds__(256) void radi_reduce_wide_kernel(int nv, int k, int m_arg, int nb, int rows_per_slice,
                                                               const int* __restrict__ rp, const int* __restrict__ ci,
                                                               const double* __restrict__ vA,
                                                               const double* __restrict__ vE,
                                                               const double* __restrict__ Q,
                                                               const double* __restrict__ RU,
                                                               const double* __restrict__ B,
                                                               double* __restrict__ part) {
  __shared__ double qs[RADI_WB * RADI_WLQ];
  __shared__ double ys[RADI_WB * RADI_WLY];
  const int m = GROUP ? m_arg : k;
  const int W = 2 * k + m + 2 * nb, ldp = m + nb, ndense = ldp + nb;
  const int ngt = (k + 31) / 32, nrt = (k + 15) / 16, kp = 16 * nrt;
  const int t = blockIdx.y;
  const bool gather = t < ngt;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lc = lane & 15, lk = lane >> 4;
  const int r0 = blockIdx.x * rows_per_slice, r1 = min(nv, r0 + rows_per_slice);
  d4 acc[8];
#pragma unroll
  for (int a = 0; a < 8; ++a) acc[a] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int row0 = r0; row0 < r1; row0 += RADI_WB) {
    const int nr = min(RADI_WB, r1 - row0);
    for (int e = tid; e < RADI_WB * kp; e += 256) {
      const int r = e / kp, c = e - r * kp;
      qs[r * RADI_WLQ + c] = (r < nr && c < k) ? Q[(size_t)(row0 + r) * k + c] : 0.0;
    }
    if (gather) {
      for (int e = tid; e < RADI_WB * 32; e += 256) {
        const int r = e >> 5, j = e & 31, c = 32 * t + j;
        double a = 0.0, s = 0.0;
        if (r < nr && c < k) {
          const int row = row0 + r;
          const int p1 = rp[row + 1];
#pragma unroll 4
          for (int p = rp[row]; p < p1; ++p) {
            const int col = ci[p];
            const double qv = col < nv ? Q[(size_t)col * k + c] : 0.0;      // (beyond nv: the J^T part of the saddle row)
            a = fma(vA[p], qv, a);
            s = fma(vE[p], qv, s);
          }
        }
        ys[r * RADI_WLY + j] = a;
        ys[r * RADI_WLY + 32 + j] = s;
      }
    } else {
      for (int e = tid; e < RADI_WB * RADI_WCT; e += 256) {
        const int r = e >> 6, j = e & 63, c = RADI_WCT * (t - ngt) + j;
        double v = 0.0;
        if (r < nr) {
          if (c < ldp) v = RU[(size_t)(row0 + r) * ldp + c];
          else if (c < ndense) v = B[(size_t)(row0 + r) * nb + c - ldp];
        }
        ys[r * RADI_WLY + j] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int r = 4 * ks + lk;
      const double bf = ys[r * RADI_WLY + 16 * wave + lc];
#pragma unroll
      for (int a = 0; a < 8; ++a)
        if (a < nrt) acc[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(qs[r * RADI_WLQ + 16 * a + lc], bf, acc[a], 0, 0, 0);
    }
    __syncthreads();
  }
  // the wave's column jl of the tile -> column of H (-1: padding)
  const int jl = 16 * wave + lc;
  int col = -1;
  if (gather) {
    const int c = 32 * t + (jl & 31);
    if (c < k) col = jl < 32 ? c : k + c;
  } else {
    const int c = RADI_WCT * (t - ngt) + jl;
    if (c < ndense) col = 2 * k + c;
  }
  if (col < 0) return;
  double* out = part + (size_t)blockIdx.x * k * W;
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = 16 * a + lk + 4 * e;
      if (a < nrt && i < k) out[(size_t)i * W + col] = acc[a][e];
    }
}
// row slices of the wide kernel: 64 rows or more each (a multiple of RADI_WB), at most 1024 of them, the partials
// kept below 64 MB
static int radi_reduce_wide_slices(int n, int k, int W, int& rows_per_slice) {
  const int cap = std::max(1, (int)(((size_t)64 << 20) / (sizeof(double) * (size_t)k * W)));
  const int want = std::max(1, std::min(std::min((n + 63) / 64, 1024), cap));
  rows_per_slice = RADI_WB * (((n + want - 1) / want + RADI_WB - 1) / RADI_WB);
  return (n + rows_per_slice - 1) / rows_per_slice;
}
size_t radi_reduce_partial_len(int nv, int k, int m, int nb) {
  int rps = 0;
  const int W = 2 * k + m + 2 * nb;
  if (k > RADI_HK) return (size_t)radi_reduce_wide_slices(std::max(nv, 1), k, W, rps) * k * W;
  return (size_t)radi_reduce_slices(std::max(nv, 1), rps) * k * W;
}
static void launch_radi_reduce_wide(hipStream_t st, int nv, int k, int m, int nb, const int* rp, const int* ci,
                                    const double* vA, const double* vE, const double* Q, const double* RU,
                                    const double* B, double* partial, double* H) {
  const int W = 2 * k + m + 2 * nb;
  int rps = 0;
  const int slices = radi_reduce_wide_slices(nv, k, W, rps);
  const int tiles = (k + 31) / 32 + (m + 2 * nb + RADI_WCT - 1) / RADI_WCT;
  if (m == k)
    hipLaunchKernelGGL(radi_reduce_wide_kernel<false>, dim3(slices, tiles), dim3(256), 0, st, nv, k, m, nb, rps, rp, ci,
                       vA, vE, Q, RU, B, partial);
  else
    hipLaunchKernelGGL(radi_reduce_wide_kernel<true>, dim3(slices, tiles), dim3(256), 0, st, nv, k, m, nb, rps, rp, ci,
                       vA, vE, Q, RU, B, partial);
  hipLaunchKernelGGL(radi_vtb_reduce_kernel, dim3((k * W + 255) / 256), dim3(256), 0, st, slices, k * W, partial, H);
}
void launch_radi_reduce(hipStream_t st, int nv, int k, int m, int nb, const int* rp, const int* ci, const double* vA,
                        const double* vE, const double* Q, const double* RU, const double* B, double* partial,
                        double* H) {
  if (nv <= 0) return;
  if (k > RADI_HK) {          // (k = m: a wide block; k != m: the group of a sweep, W <= 509: the callers check)
    launch_radi_reduce_wide(st, nv, k, m, nb, rp, ci, vA, vE, Q, RU, B, partial, H);
    return;
  }
  const int W = 2 * k + m + 2 * nb;
  const int nsub = std::max(1, std::min(256 / W, RADI_HB));
  int rps = 0;
  const int slices = radi_reduce_slices(nv, rps);
  const size_t lds = sizeof(double) * ((size_t)RADI_HB * ((W | 1) + (k | 1)) + (nsub > 1 ? (size_t)k * W : 0));
  hipLaunchKernelGGL(radi_reduce_kernel, dim3(slices), dim3(256), lds, st, nv, k, m, nb, rps, nsub, rp, ci, vA, vE, Q,
                     RU, B, partial);
  hipLaunchKernelGGL(radi_vtb_reduce_kernel, dim3((k * W + 255) / 256), dim3(256), 0, st, slices, k * W, partial, H);
}

}  // namespace ricadi
