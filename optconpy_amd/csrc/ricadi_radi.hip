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
// FP64 throughout, no atomics, every sum in a fixed order: the same inputs give bitwise the same outputs.
#include "ricadi_internal.h"

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

}  // namespace ricadi
