// ricadi_project.hip -- K7: the pencil of the operator projected onto a dense basis,
//   H_A = Q^T cal A Q,  H_E = Q^T cal E Q   (Q: NV x k row-major, k <= 128),
// for the Ritz values behind the automatic ADI shifts (optconpy_amd/adi_shifts.py).
//
// One pass over the velocity rows of the saddle pattern (s_rp / s_ci, columns below NV only) with the two
// value sources srcA / srcE: pattern and indices are read once for both products.  A workgroup owns a
// contiguous range of rows and one 16-column slice of the products; per 16-row chunk it forms
// (cal A Q)[rows, slice] and (cal E Q)[rows, slice] in LDS from gathered Q rows, then multiplies by its own
// contiguous Q rows on v_mfma_f64_16x16x4_f64.  The result is a k x k partial per workgroup; a second kernel
// sums the partials in workgroup order.  No atomics: the same inputs give bitwise the same H.
//
// The two-sided form (TWOSIDED) multiplies the products formed from a right basis by the rows of a second, left basis:
// L^T cal A Rb and L^T cal E Rb, the reduced pencil of a balanced truncation.
//
// The dense form of the same kernel (Y = two dense NV x q panels instead of the two sparse products) gives
// Q^T U and Q^T V of the low-rank term, so H_A - (Q^T U)(V^T Q) is reproducible as well.
#include "ricadi_device.h"

namespace ricadi {

// v_mfma_f64_16x16x4_f64: lane l holds A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15];
// D[row = (l>>4) + 4*reg][col = l&15].
//
// part: [gridDim.x][2][kp][np2], kp = 16 * ceil(k / 16), np2 = 16 * gridDim.y; every entry is written.
// TWOSIDED (the Petrov-Galerkin form, L^T cal A Q and L^T cal E Q): the workgroup's own rows come from the left basis L
// (NV x k as Q), the gathered rows from Q as before; without it L is not read and the arithmetic is the one-basis one.
template <bool DENSE, bool TWOSIDED>
__global__ __launch_bounds__(256) void project_pencil_kernel(int nv, int k, int n2, int rows_per_wg,
                                                             const int* __restrict__ rp, const int* __restrict__ ci,
                                                             const double* __restrict__ vA,
                                                             const double* __restrict__ vE,
                                                             const double* __restrict__ Q,
                                                             const double* __restrict__ L,
                                                             const double* __restrict__ U,
                                                             const double* __restrict__ V,
                                                             double* __restrict__ part) {
  __shared__ double sA[16][17];
  __shared__ double sE[16][17];
  const int kt = (k + 15) >> 4;
  const int kp = 16 * kt;
  const int np2 = 16 * gridDim.y;
  const int j0 = 16 * blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lc = lane & 15, lk = lane >> 4;
  const int rr = threadIdx.x >> 4, jj = threadIdx.x & 15;   // the (row, column) of the chunk this thread forms
  const int rbeg = blockIdx.x * rows_per_wg;
  const int rend = min(nv, rbeg + rows_per_wg);
  d4 accA[2], accE[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    accA[t] = (d4){0.0, 0.0, 0.0, 0.0};
    accE[t] = (d4){0.0, 0.0, 0.0, 0.0};
  }
  const int col = j0 + jj;
  const double* __restrict__ own = TWOSIDED ? L : Q;
  for (int r0 = rbeg; r0 < rend; r0 += 16) {
    const int row = r0 + rr;
    double a = 0.0, e = 0.0;
    if (row < rend && col < n2) {
      if (DENSE) {
        a = U[(size_t)row * n2 + col];
        e = V[(size_t)row * n2 + col];
      } else {
        for (int p = rp[row]; p < rp[row + 1]; ++p) {
          const int c = ci[p];
          if (c >= nv) continue;                   // J^T part of the saddle row
          const double qv = Q[(size_t)c * k + col];
          a = fma(vA[p], qv, a);
          e = fma(vE[p], qv, e);
        }
      }
    }
    sA[rr][jj] = a;
    sE[rr][jj] = e;
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int rk = r0 + 4 * s + lk;
      const double bA = sA[4 * s + lk][lc], bE = sE[4 * s + lk][lc];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int i = 16 * (wave + 4 * t) + lc;
        if (wave + 4 * t < kt) {
          const double aq = (rk < rend && i < k) ? own[(size_t)rk * k + i] : 0.0;
          accA[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(aq, bA, accA[t], 0, 0, 0);
          accE[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(aq, bE, accE[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  double* pA = part + (size_t)blockIdx.x * 2 * kp * np2;
  double* pE = pA + (size_t)kp * np2;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (wave + 4 * t >= kt) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t o = (size_t)(16 * (wave + 4 * t) + lk + 4 * r) * np2 + j0 + lc;
      pA[o] = accA[t][r];
      pE[o] = accE[t][r];
    }
  }
}

// HA / HE (k x n2, row-major) = sum of the nwg partials, in workgroup order
__global__ void project_reduce_kernel(int nwg, int k, int n2, int kp, int np2, const double* __restrict__ part,
                                      double* __restrict__ HA, double* __restrict__ HE) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 2 * k * n2) return;
  const int mat = idx / (k * n2), ij = idx % (k * n2);
  const int i = ij / n2, j = ij % n2;
  const double* p = part + (size_t)mat * kp * np2 + (size_t)i * np2 + j;
  double s = 0.0;
  for (int w = 0; w < nwg; ++w) s += p[(size_t)w * 2 * kp * np2];
  (mat ? HE : HA)[ij] = s;
}

// HA (k x k) -= QU QV^T, QU = Q^T U and QV = Q^T V (k x q); fixed summation order
__global__ void project_lowrank_kernel(int k, int q, const double* __restrict__ QU, const double* __restrict__ QV,
                                       double* __restrict__ HA) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= k * k) return;
  const int i = idx / k, j = idx % k;
  double s = 0.0;
  for (int l = 0; l < q; ++l) s = fma(QU[(size_t)i * q + l], QV[(size_t)j * q + l], s);
  HA[idx] -= s;
}

// Workgroups over the rows: enough to fill the chip with the column slices, partials kept to ~4 * kt MB
static int project_grid(int nv, int ncol_tiles, int& rows_per_wg) {
  const int chunks = (nv + 15) / 16;
  const int nwg = std::max(1, std::min(chunks, 1024 / ncol_tiles));
  rows_per_wg = 16 * ((chunks + nwg - 1) / nwg);
  return (nv + rows_per_wg - 1) / rows_per_wg;
}

size_t project_part_count(int nv, int k, int n2) {
  int rpw = 0;
  const int ct = (n2 + 15) / 16;
  const int nwg = project_grid(nv, ct, rpw);
  return (size_t)nwg * 2 * (16 * ((k + 15) / 16)) * (16 * ct);
}

void launch_project_pencil(hipStream_t st, int nv, int k, const int* rp, const int* ci, const double* vA,
                           const double* vE, const double* Q, const double* U, const double* V, int q,
                           double* part, double* HA, double* HE) {
  const bool dense = U != nullptr;
  const int n2 = dense ? q : k;
  const int ct = (n2 + 15) / 16;
  int rpw = 0;
  const int nwg = project_grid(nv, ct, rpw);
  if (dense)
    hipLaunchKernelGGL((project_pencil_kernel<true, false>), dim3(nwg, ct), dim3(256), 0, st, nv, k, n2, rpw, rp, ci,
                       vA, vE, Q, Q, U, V, part);
  else
    hipLaunchKernelGGL((project_pencil_kernel<false, false>), dim3(nwg, ct), dim3(256), 0, st, nv, k, n2, rpw, rp, ci,
                       vA, vE, Q, Q, U, V, part);
  const int tot = 2 * k * n2;
  hipLaunchKernelGGL(project_reduce_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, nwg, k, n2,
                     16 * ((k + 15) / 16), 16 * ct, part, HA, HE);
}

// H_A = L^T cal A Rb, H_E = L^T cal E Rb (r x r): the same pass, grid and partial layout with both bases
void launch_project_pencil_twosided(hipStream_t st, int nv, int r, const int* rp, const int* ci, const double* vA,
                                    const double* vE, const double* L, const double* Rb, double* part, double* HA,
                                    double* HE) {
  const int ct = (r + 15) / 16;
  int rpw = 0;
  const int nwg = project_grid(nv, ct, rpw);
  hipLaunchKernelGGL((project_pencil_kernel<false, true>), dim3(nwg, ct), dim3(256), 0, st, nv, r, r, rpw, rp, ci, vA,
                     vE, Rb, L, nullptr, nullptr, part);
  const int tot = 2 * r * r;
  hipLaunchKernelGGL(project_reduce_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, nwg, r, r, 16 * ct, 16 * ct,
                     part, HA, HE);
}

void launch_project_lowrank(hipStream_t st, int k, int q, const double* QU, const double* QV, double* HA) {
  hipLaunchKernelGGL(project_lowrank_kernel, dim3((k * k + 255) / 256), dim3(256), 0, st, k, q, QU, QV, HA);
}

}  // namespace ricadi
