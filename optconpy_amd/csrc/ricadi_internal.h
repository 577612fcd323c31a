// ricadi_internal.h -- shared declarations of libricadi_hip.so (not installed).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ricadi.h"

#define RICADI_MAX_M 128
#define RICADI_MAX_GROUPS 16

namespace ricadi {

// ---- host-side CSR helper --------------------------------------------------
struct HostCsr {
  int nrows = 0, ncols = 0;
  std::vector<int> rp, ci;
  std::vector<double> v;
  size_t nnz() const { return ci.size(); }
};
HostCsr make_csr(int nrows, int ncols, const int32_t* rp, const int32_t* ci, const double* v);
HostCsr transpose(const HostCsr& a);
void sort_rows(HostCsr& a);

int aggregate(int n, const int* rp, const int* ci, int bsize, int* blk);

// Patches and colours of the coloured Vanka sweep of a level, from its J alone (ricadi_host_vanka_patches of
// include/ricadi.h states the rule).  idx: VANKA_K indices per patch, -1 padded, colour by colour.
constexpr int VANKA_K = 64;
struct VankaPatches {
  int ncolours = 0, npatches = 0, npress = 0, largest = 0, dropped = 0, nlone = 0, nlone_patches = 0;
  std::vector<int> colour_ptr, idx;
};
VankaPatches vanka_patches(int nv, const HostCsr& J);

// Host-built description of the saddle operator and of the fixed (shift independent) parts of one level of the
// preconditioner.
struct HostSetup {
  int nv = 0, np = 0, n = 0;
  // unified saddle pattern, three value sources
  std::vector<int> s_rp, s_ci;
  std::vector<double> s_srcA, s_srcE, s_srcJ;
  // diagonals of A and E
  std::vector<double> dA, dE;
  // block-Jacobi, velocity block
  int bs = 32;
  int nbv = 0;
  std::vector<int> bv_ptr, bv_rows;
  std::vector<double> bv_A, bv_E;  // nbv x bs x bs
  // block-Jacobi, Schur complement
  int nbp = 0;
  std::vector<int> bp_ptr, bp_rows;  // rows are pressure-local (0..np)
  // dense bs x bs blocks of J for every (pressure block, coupled velocity block) pair:
  // row = pressure dof local to its block, column = velocity dof local to its block
  std::vector<int> jd_ptr, jd_vblk;
  std::vector<double> jd_val;
  // LDS-tiled SpMM: rows grouped in blocks of <= 32 (visited block-Jacobi aggregate by
  // aggregate = compact mesh patches); per block the distinct columns and
  // 16-bit local column indices; arrays in block order
  int sb_nblk = 0, sb_max_cols = 0, sb_max_nnz = 0;
  std::vector<int> sb_rowptr, sb_rows, sb_rp, sb_cptr, sb_cols, sb_perm;
  std::vector<uint16_t> sb_lidx;
  // coarse level
  int kc = 0, kcv = 0, kcp = 0;
  int agg_v = 0, agg_p = 0;            // aggregate sizes the hierarchy rule ended with
  std::vector<int> agg_ptr, agg_rows;  // aggregates over all n dofs
  std::vector<int> aggof;              // n -> coarse index
  std::vector<double> E0, EM, EJ;      // kc x kc dense
  // Multilevel: the coarse saddle problem is NOT inverted densely (kc > coarse_max with the base
  // aggregate sizes); its Galerkin matrices Yv^T A Yv, Yv^T E Yv, Yp^T J Yv go to a child level.
  bool multilevel = false;
  HostCsr l1A, l1E, l1J;
  // Smoothed aggregation (round 3; two-level setups only): the velocity part of the prolongation is
  //   P_v = (I - omega D^-1 K0) Y_v,  K0 = sym(cal A), D = diag(K0)
  // -- shift independent, so that P^T S(p) P and S(p) P stay linear in (alpha, beta).  p_*: P by rows (all n rows;
  // pressure rows are the piecewise-constant ones), pt_*: P^T by rows (the restriction), pd_*: P - Y on the
  // velocity rows (its action on the coarse vector is folded into the first velocity sweep).  With sa == false
  // P = Y and these arrays are empty.
  bool sa = false;
  std::vector<int> p_rp, p_ci, pt_rp, pt_ci, pd_rp, pd_ci;
  std::vector<double> p_v, pt_v, pd_v;
  // S * Y: CSR over (row, aggregate) with the three value sources of the saddle pattern
  std::vector<int> sy_rp, sy_ci;
  std::vector<double> sy_A, sy_E, sy_J;
  // ... and in tile format on the row blocks of the saddle operator
  int syb_max_cols = 0;
  std::vector<int> syb_rp, syb_cptr, syb_cols, syb_perm;
  std::vector<uint16_t> syb_lidx;
};
// JT = transpose(J): the caller computes it once per level (build_records and the upload need it too)
HostSetup build_setup(const HostCsr& A, const HostCsr& E, const HostCsr& J, const HostCsr& JT, const ricadi_opts& o,
                      int max_levels, double sa_omega);
// build_setup, rebuilt without smoothed aggregation when the smoothed prolongation does not fit the folded first
// sweep (a velocity block touching more than 64 coarse columns)
HostSetup build_setup_checked(const HostCsr& A, const HostCsr& E, const HostCsr& J, const HostCsr& JT,
                              const ricadi_opts& o, int max_levels, double sa_omega);

// The hierarchy below a level, shared by ricadi_set_operator and ricadi_host_plan_hierarchy: the levels the top
// context may use (build_setup's max_levels: 2 = no child), and the options and levels of the child of a level with
// options o that may use `levels` (parent_is_child: that level is a child itself).
int root_levels(const ricadi_opts& o);
ricadi_opts child_opts(const ricadi_opts& o, bool parent_is_child);
int child_levels(const ricadi_opts& o, int levels);

// ---- device records of the preconditioner ------------------------------------------
// Fixed-stride record of a 32-row velocity block (ricadi_ctx::sw_meta, SweepRecs::meta): a header of
// SWREC_ROWS words {nb, ni of the rectangle sweep, ni of the two-term sweep, 0}, then the block's rows [32], the
// aggregate of every row [32], the input rows of the rectangle sweep [kr] and of the two-term sweep [k2]; every list
// is padded with its last entry.  kr / k2: padded slice widths of the two sweeps (0: sweep not in that form).
constexpr int SWREC_NB = 0, SWREC_NI_RECT = 1, SWREC_NI_TWO = 2;
constexpr int SWREC_ROWS = 4;
constexpr int SWREC_AGG = SWREC_ROWS + 32;
constexpr int SWREC_IN = SWREC_AGG + 32;
constexpr int swrec_stride(int kr, int k2) { return SWREC_IN + kr + k2; }
// Record of one (Schur block, row of the block) of the fused pressure step (ricadi_ctx::ps_meta), PSREC_WIDTH words:
// {pressure-local row or -1, J row range [j0, j1), (S Y) pressure-row range [sy0, sy1)}; an empty range is [0, 0)
constexpr int PSREC_ROW = 0, PSREC_J0 = 1, PSREC_J1 = 2, PSREC_SY0 = 3, PSREC_SY1 = 4, PSREC_WIDTH = 5;

// Everything the preconditioner uploads beyond the HostSetup arrays themselves, derived on the host from the setup,
// J and J^T.  sweep_meta: build the fixed-stride sweep records (RICADI_SWEEP_META); ms_spmm: the multi-shift value
// arrays of S*Y (RICADI_MS_SPMM; those of the saddle operator are built whenever its tiles allow them).
struct PrecondRecords {
  // last velocity sweep in rectangular form: per velocity block the pressure dofs its rows touch (gt_ptr / gt_cols)
  // and the dense bs x gt_ks slices of J^T over them; gt_kmax = longest list
  bool gt_ok = false;
  int gt_ks = 0, gt_kmax = 0;
  std::vector<int> gt_ptr, gt_cols;
  std::vector<double> jtd;
  // first velocity sweep with the coarse residual folded in: per velocity block the coarse columns its S*Y rows
  // touch and the dense bs x ady_ks slices of the three value sources (dT: of P - Y, smoothed aggregation only)
  bool ady_ok = false;
  int ady_ks = 0;
  std::vector<int> cy_ptr, cy_cols;
  std::vector<double> dA, dE, dJ, dT;
  std::vector<int> ps_meta;                    // PSREC_WIDTH words per (Schur block, row)
  std::vector<int> sw_meta;                    // swrec_stride words per velocity block; empty: sw_stride = 0
  int sw_stride = 0, sw_in_rect = 0, sw_in_two = 0;
  // tile format of the saddle operator padded to fixed strides (see spmm_blocked_kernel)
  bool sb_ok = false;
  std::vector<int> sb_rows2, sb_rp2, sb_cols2, sb_colsm2;
  // ... and of S*Y
  bool syb_ok = false;
  std::vector<int> syb_rp2, syb_cols2;
  // multi-shift kernel operands in tile order: AJ = A part + J part (disjoint supports), E, and the local index with
  // the velocity-velocity flag in bit 15; ms_ok: those of the saddle operator were built
  bool ms_ok = false;
  std::vector<double> sbAJ, sbE, sybAJ, sybE;
  std::vector<uint16_t> sb_lidx_ms, syb_lidx_ms;
  int sy_chunk = 16;                           // row chunk of the S*Y CSR kernel: 8 when its rows are short
};
PrecondRecords build_records(const HostSetup& hs, const HostCsr& J, const HostCsr& JT, bool sweep_meta,
                             bool ms_spmm);
bool sa_criterion(const HostCsr& A, double& rs_out, double& gamma_out);
int cauchy_data(const double* shifts, int g, double* rinv, double* cinv1);
int adi_window_width(const double* shifts, int ns, int first, int g);
int deal_shifts(const double* shifts, int ns, int world, int32_t* owner);
int gram_lstsq(int h, int m, const double* Ghh, const double* Ghb, double rtol, double* Y);
// the same on the column-normalised problem (unit diagonal), solution scaled back; Ghh / Ghb are overwritten
int gram_lstsq_scaled(int h, int m, std::vector<double>& Ghh, std::vector<double>& Ghb, double rtol,
                      std::vector<double>& Y);

// ---- batches of panels ------------------------------------------------------------
// A *batch* is a set of up to RICADI_MAX_GROUPS panels (one per ADI shift of a
// sweep), stored group-major: panel g of a buffer starts g * (group stride)
// doubles behind panel 0.  Batched launches add the ACTIVE groups as grid.z:
// block z works on group gid[z], so groups whose solve has converged simply
// drop out of the table while their data stay where they are.  Shift-dependent
// operands (matrix values, block inverses, coarse inverse) come as one pointer
// per group id.  Both tables travel by value in the kernel arguments.
struct GroupTab {
  int ng;
  int gid[RICADI_MAX_GROUPS];
};
template <class T>
struct GroupPtrsT {
  const T* p[RICADI_MAX_GROUPS];
};
typedef GroupPtrsT<double> GroupPtrs;
typedef GroupPtrsT<float> GroupPtrsF;   // FP32-stored preconditioner operands
typedef GroupPtrsT<uint16_t> GroupPtrsH;   // BF16-stored block operands of the sweeps (bit patterns; round 4)
struct GroupInts {            // one small integer per group id (by value)
  int v[RICADI_MAX_GROUPS];
};
inline GroupInts same_int(int k) {
  GroupInts g;
  for (int i = 0; i < RICADI_MAX_GROUPS; ++i) g.v[i] = k;
  return g;
}
inline GroupTab single_group() {
  GroupTab t{};
  t.ng = 1;
  return t;
}
template <class T>
inline GroupPtrsT<T> same_ptr(const T* q) {
  GroupPtrsT<T> g;
  for (int i = 0; i < RICADI_MAX_GROUPS; ++i) g.p[i] = q;
  return g;
}

// The epilogue of a block-Jacobi sweep.  Coarse-level prolongation fused into it: every row the sweep
// writes gets  + ec[aggof[row], :]  (ec: kc x m per group, stride gse); and the copies of the result.
struct ProlongArgs {
  const int* aggof = nullptr;
  const double* ec = nullptr;
  size_t gse = 0;
  double* out2 = nullptr;   // if set: the sweep's result before the coarse part is added
  size_t gs2 = 0;
  float* out32 = nullptr;   // if set: FP32 copy of what the sweep writes (flexible GMRES keeps Z_j = P^-1 v_j)
  size_t gs32 = 0;
  int only32 = 0;           // with out32: the FP64 result is not stored (the operator reads the FP32 copy)
  int old32 = 0;            // rectangle sweep: the rows it updates are read from out32 (FP32 intermediate of the cycle)
};
// The fixed-stride records of the 32-row velocity blocks (ricadi_ctx::sw_meta; layout: SWREC_* above), for the two
// record-driven sweeps.  With them a wave has every index after ONE load round (block pointers -> row lists ->
// aggregate map were three dependent ones).  in_off: offset of the launched sweep's input list in a record (SWREC_IN
// for the rectangle sweep, SWREC_IN + kr for the two-term one).
struct SweepRecs {
  const int* meta = nullptr;
  int stride = 0, in_off = 0;
};

// Low-rank term fused into an SpMM epilogue:  y[row, :] -= U[row, :] * c  for
// row < nrows, with c = V^T x (q x m per group, stride gsc) reduced beforehand.
struct LowRankArgs {
  const double* U = nullptr;
  const double* c = nullptr;
  size_t gsc = 0;
  int q = 0, nrows = 0;
};

// Input of a block-Jacobi sweep produced on the fly:
//   in[row, :] = base[row, :] + scale * (C * src)[row, :]
// with a CSR matrix C (rows = the sweep's rows; values per group), a panel src (group
// stride gss, same leading dimension as `in` would have) and an optional panel base
// (group stride gsb; NULL = 0).  Saves writing and re-reading the intermediate panel:
// the J^T product of the SIMPLE sweep (base = NULL, scale = 1) and the residual after
// the coarse correction r - (S Y) e (base = r, scale = -1).
struct CsrInArgs {
  const int* rp = nullptr;
  const int* ci = nullptr;
  GroupPtrs v = {};
  const double* src = nullptr;
  size_t gss = 0;
  const double* base = nullptr;
  size_t gsb = 0;
  double scale = 1.0;
};

// One input segment of the two-term block sweep (block_apply2_kernel):
//   iptr == NULL: the block's own rows; moff == NULL: matrix of block b at b * BS * kstride;
//   kstride == 0: row stride = the block's input count.
struct Seg2 {
  const int* iptr = nullptr;
  const int* irows = nullptr;
  const int* moff = nullptr;
  int kstride = 0;
  const double* in = nullptr;
  size_t gs = 0;
  const _Float16* in16 = nullptr;   // segment 1 only: read the input rows from an FP16 panel instead of `in`
};

// y = A x for a CSR matrix with LONG rows (the restriction: one row per aggregate), one wave per row
// (spmm_rowwave_kernel); x FP64 or FP16-stored (x16), panels of m = 16 columns (leading dimension 16), group strides
// gsx / gsy.  spmm_rowwave_pays: rows long enough on average (>= 32 entries) for it to beat the 16-lane-per-row kernel.
// kb: y (the coarse residual) in the k-blocked layout of rckb_index, for launch_dense_apply_kb.
bool spmm_rowwave_pays(int nrows, size_t nnz);
void launch_spmm_rowwave(hipStream_t st, const GroupTab& gt, int nrows, const int* rp, const int* ci,
                         const GroupPtrs& vals, const double* x, const _Float16* x16, size_t gsx, double* y, size_t gsy,
                         int m, bool kb = false);
// The k x 16 coarse residual in the k-blocked layout: the rows below k4 = k & ~3 in groups of four, entry (j, c) at
// ((j >> 2) * 16 + c) * 4 + (j & 3), so that the four values a lane of the coarse apply feeds to four MFMAs are 32
// contiguous bytes; the last k - k4 rows row-major where they always are.  Same k * 16 doubles.
__host__ __device__ inline size_t rckb_index(int j, int c, int k) {
  return j < (k & ~3) ? ((size_t)(j >> 2) * 16 + c) * 4 + (j & 3) : (size_t)j * 16 + c;
}

// ---- kernel launchers (ricadi_spmm.hip, ricadi_arnoldi.hip, ricadi_precond.hip, ricadi_dense.hip, ricadi_radi.hip) -----
// The *_b launchers are the batched forms (GroupTab + group strides `gs*`, in
// doubles); the plain ones run a single panel.
void launch_spmm_h(hipStream_t st, const GroupTab& gt, int nrows, const int* rp, const int* ci,
                   const GroupPtrs& vals, const double* x, const _Float16* x16, int ldx, size_t gsx, double* y, int ldy,
                   size_t gsy, const _Float16* r16, int ldr, size_t gsr, double alpha, double beta_r, int m, int chunk);
void launch_spmm_b(hipStream_t st, const GroupTab& gt, int nrows, const int* rp, const int* ci,
                   const GroupPtrs& vals, const double* x, int ldx, size_t gsx, const int* xmap,
                   double* y, int ldy, size_t gsy, const double* r, int ldr, size_t gsr,
                   double alpha, double beta_r, int m, const LowRankArgs& lr = LowRankArgs(),
                   int chunk = 16);   // chunk = 8: matrices with short rows (<= ~10 entries)
void launch_spmm_blocked_b(hipStream_t st, const GroupTab& gt, int nblk, const int* rows2,
                           const int* rp2, const int* cols2, const uint16_t* lidx,
                           const GroupPtrs& vals, const double* x, int ldx, size_t gsx, double* y,
                           int ldy, size_t gsy, const double* r, int ldr, size_t gsr, double alpha,
                           double beta_r, int m, int max_cols,
                           const LowRankArgs& lr = LowRankArgs());
// multi-shift form: one read of the value arrays (tile order; vAJ = A part + J part, vE) for
// all active groups; lidx carries the velocity-velocity flag in bit 15; alphas / betas:
// RICADI_MAX_GROUPS coefficients indexed by group id
bool spmm_blocked_ms_ok(int m, int max_cols, size_t panel_rows);
// FP32 input panel: with m == 16 the kernel fills its tile with 16-byte loads and addresses x rows as 16 packed floats
// -- the panel must be packed (ldx == 16, 16-byte aligned); the one caller (saddle_spmm) passes ldx = m
void launch_spmm_blocked_x32(hipStream_t st, const GroupTab& gt, int nblk, const int* rows2, const int* rp2,
                             const int* cols2, const uint16_t* lidx, const GroupPtrs& vals, const float* x, int ldx,
                             size_t gsx, double* y, int ldy, size_t gsy, double alpha, int m, int max_cols, float* y32 = nullptr);
void launch_spmm_blocked_ms_x32(hipStream_t st, const GroupTab& gt, const double* alphas, const double* betas,
                                int nblk, const int* rows2, const int* rp2, const int* cols2, const uint16_t* lidx,
                                const double* vAJ, const double* vE, const float* x, int ldx, size_t gsx, double* y,
                                int ldy, size_t gsy, double alpha, int m, int max_cols, float* y32 = nullptr);
void launch_spmm_blocked_ms(hipStream_t st, const GroupTab& gt, const double* alphas, const double* betas,
                            int nblk, const int* rows2, const int* rp2, const int* cols2,
                            const uint16_t* lidx, const double* vAJ, const double* vE,
                            const double* x, int ldx, size_t gsx, double* y, int ldy, size_t gsy,
                            const double* r, int ldr, size_t gsr, double alpha, double beta_r, int m,
                            int max_cols);
void launch_axpby_b(hipStream_t st, const GroupTab& gt, size_t n, double a, const double* x,
                    size_t gsx, double b, double* y, size_t gsy);
void launch_colscale_b(hipStream_t st, const GroupTab& gt, size_t nrows, int m, const double* a,
                       const double* x, size_t gsx, double b, double* y, size_t gsy,
                       float* yf = nullptr, size_t gsf = 0);
void launch_colscale_b(hipStream_t st, const GroupTab& gt, size_t nrows, int m, const double* a,
                       const double* x, size_t gsx, double b, double* y, size_t gsy, _Float16* yf,
                       size_t gsf);
// Arnoldi passes on the Krylov basis stored as BT = double, float or _Float16 (the arithmetic is FP64 throughout).
// The panel w is stored as WT = double, or float: the operator's FP32 output on the hot path, admitted exactly where
// iteration_form admits it (FP16 basis, 16 columns, keep_w, arnoldi16_w32_ok); any other use throws.
template <class BT, class WT>
void launch_cols_dots_b(hipStream_t st, const GroupTab& gt, int nrows, int m, int nvec,
                        const BT* basis, size_t vstride, size_t gsb, const WT* w, size_t gsw,
                        int want_self, double* partial, size_t gsp, double* out, size_t gso);
// keep_w (FP16 basis, 16 columns, update_dots_keeps_w): w is left as it was BEFORE the first projection (no store per
// element); the Hessenberg kernel then writes h1 + h2 to `hsum` and the final update uses those on w
template <class BT, class WT>
void launch_cols_update_dots_b(hipStream_t st, const GroupTab& gt, int nrows, int m, int nvec,
                               const BT* basis, size_t vstride, size_t gsb, const double* h,
                               size_t gsh, WT* w, size_t gsw, bool keep_w, double* partial, size_t gsp,
                               double* out, size_t gso);
template <class BT>
void launch_cols_update_b(hipStream_t st, const GroupTab& gt, int nrows, int m, int nvec,
                          const BT* basis, size_t vstride, size_t gsb, const double* h,
                          size_t gsh, double sign, const double* w, size_t gsw, const double* scale,
                          double* out, size_t gso, BT* outf = nullptr, size_t gsf = 0);
template <class BT>
void launch_cols_update_bk(hipStream_t st, const GroupTab& gt, int nrows, int m, const GroupInts& nvec,
                           const BT* basis, size_t vstride, size_t gsb, const double* h, size_t gsh,
                           double* out, size_t gso, const double* acc = nullptr, size_t gsa = 0);
void launch_gmres_hess_b(hipStream_t st, const GroupTab& gt, int m, int j, int restart,
                         const double* h1, const double* h2, double* H, double* cs, double* sn,
                         double* g, double* scale, double* resid, const double* bnorm, double tol,
                         double* host_resid = nullptr, double* hsum = nullptr);
bool update_dots_keeps_w(int m, bool fp16_basis, int nvec_max);
bool arnoldi16_w32_ok(int nvec_max);   // do the coefficients of nvec_max vectors fit beside the FP32 panel's chunk?
void launch_gmres_backsolve_b(hipStream_t st, const GroupTab& gt, int m, const GroupInts& k,
                              int restart, const double* H, const double* g, double* y);
void launch_gmres_start_b(hipStream_t st, const GroupTab& gt, int m, int restart,
                          const double* nrm2, double* g, double* scale, double* resid);
// The generic preconditioner sweeps take their operands stored in FP64 (T = double: GroupPtrs) or FP32 (T = float:
// GroupPtrsF).
template <class T>
void launch_block_apply_b(hipStream_t st, const GroupTab& gt, int bs, int nblocks, const int* bptr,
                          const int* rows, const GroupPtrsT<T>& inv, const double* in, int ldi,
                          size_t gsi, double* out, int ldo, size_t gso, int m, int subtract,
                          const ProlongArgs& pa = ProlongArgs(), const CsrInArgs& ci = CsrInArgs());
void launch_dense_apply_b(hipStream_t st, const GroupTab& gt, int k, int m, const GroupPtrs& Einv,
                          const double* rc, double* ec);
// FP32-stored inverses: tile-major (launch_to_f32_tiled)
void launch_dense_apply_b(hipStream_t st, const GroupTab& gt, int k, int m, const GroupPtrsF& Einv,
                          const double* rc, double* ec);
// The same product on the FP32 tile-major inverse for m = 16 with rc in the k-blocked layout (rckb_index); ec
// row-major as above.
void launch_dense_apply_kb(hipStream_t st, const GroupTab& gt, int k, const GroupPtrsF& Einv, const double* rc,
                           double* ec);
// rectangular block sweep  out[rows_b] (-)= mats[b] (bs x ks) * in[irows_b]  (+ fused prolongation)
bool block_apply_rect_ok(int bs, int ks);
template <class T>
void launch_block_apply_rect_b(hipStream_t st, const GroupTab& gt, int bs, int ks, int nblocks,
                               const int* bptr, const int* rows, const int* iptr, const int* irows,
                               const GroupPtrsT<T>& mats, const double* in, int ldi, size_t gsi, double* out,
                               int ldo, size_t gso, int m, int subtract, const ProlongArgs& pa);
// out[rows_b] = M1_b in1[rows_b] - M2_b in2[list2_b]  (+ fused prolongation / plain copy via pa);
// segment 1: the block's own rows, bs x bs matrices; segment 2: list + bs x kstride (32 | 64) matrices
bool block_apply2_ok(int bs, int k2);
template <class T>
void launch_block_apply2_b(hipStream_t st, const GroupTab& gt, int bs, int nblocks, const int* bptr,
                           const int* rows, const GroupPtrsT<T>& m1, const Seg2& s1, const GroupPtrsT<T>& m2,
                           const Seg2& s2, double* out, int ldo, size_t gso, int m, const ProlongArgs& pa);
// per shift:  out[b] = Ainv[b] * (alpha dE[b] + beta dA[b] + dJ[b])   (dense slices of S*Y, bs x ks)
void launch_ady_blocks(hipStream_t st, int nshift, int nblocks, int bs, int ks, const double* dA,
                       const double* dE, const double* dJ, const double* dT, const double* alphas,
                       const double* betas, const GroupPtrs& ainv, const GroupPtrs& out);
void launch_gt_blocks(hipStream_t st, int nshift, int nblocks, int bs, int ks, const double* jtd,
                      const GroupPtrs& ainv, const GroupPtrs& out);
void launch_to_f32(hipStream_t st, int nrows, int ncols, const double* src, int lds_, float* dst,
                   int ldd);
void launch_to_f32_tiled(hipStream_t st, int k, const double* src, float* dst);
void launch_gemm_tn_b(hipStream_t st, const GroupTab& gt, int n, int p, int q, const double* A,
                      int lda, const double* B, int ldb, size_t gsB, double* C, int ldc, size_t gsC);
// A given per group (A[g] is n x p, leading dimension lda)
void launch_gemm_nn_bp(hipStream_t st, const GroupTab& gt, int n, int p, int q, const GroupPtrs& A,
                       int lda, const double* C, int ldc, size_t gsC, double* Y, int ldy, size_t gsY,
                       double alpha, double beta);
void launch_spmm(hipStream_t st, int nrows, const int* rp, const int* ci, const double* val,
                 const double* x, int ldx, const int* xmap, double* y, int ldy, const double* r,
                 int ldr, double alpha, double beta_r, const double* rowscale, int m);
size_t spmm_blocked_lds_bytes(int m, int max_cols);
void launch_gather_vals(hipStream_t st, int nnz, const int* perm, const double* src, double* dst);
void launch_assemble_shift(hipStream_t st, int nnz, const double* srcA, const double* srcE,
                           const double* srcJ, double alpha, double beta, double* out);
void launch_axpby(hipStream_t st, size_t n, double a, const double* x, double b, double* y);
void launch_copy_cols(hipStream_t st, int nrows, int w, const double* src, int lds_, int sc0,
                      double* dst, int ldd, int dc0, double scale);
int dots_num_blocks(int nrows);
void launch_cols_dots(hipStream_t st, int nrows, int m, int nvec, const double* basis,
                      size_t vstride, const double* w, int want_self, double* partial,
                      double* out);
void launch_cols_update(hipStream_t st, int nrows, int m, int nvec, const double* basis,
                        size_t vstride, const double* h, double sign, const double* w,
                        const double* scale, double* out);
// setup kernels for up to RICADI_MAX_GROUPS shifts per launch (blockIdx.y = shift)
void launch_schur_blocks_bj(hipStream_t st, int nshift, int nblocks, int bs, const int* bptr,
                            const int* jd_ptr, const int* jd_vblk, const double* jd_val,
                            const GroupPtrs& bvinv, const GroupPtrs& blocks);
void launch_block_invert(hipStream_t st, int nshift, int nblocks, int bs, const int* bptr,
                         const GroupPtrs& blocks, int* flag);
void launch_block_combine(hipStream_t st, size_t n, const double* Ba, const double* Be,
                          double alpha, double beta, double* out);
void launch_gemm_tn(hipStream_t st, int n, int p, int q, const double* A, int lda, const double* B,
                    int ldb, double* C, int ldc);
void launch_gemm_nn(hipStream_t st, int n, int p, int q, const double* A, int lda, const double* C,
                    int ldc, double* Y, int ldy, double alpha, double beta);
int tsqr_num_blocks(int nrows);
void launch_tsqr_local(hipStream_t st, int nrows, int w, const double* A, int lda, double* Qloc,
                       double* Rstack);
void launch_tsqr_apply(hipStream_t st, int nrows, int w, const double* Qloc, const double* G,
                       double* Qout, int ldq);
void launch_cholqr_small(hipStream_t st, int w, const double* G, const double* Rprev, double* T,
                         double* R, int* flag);
void launch_cholqr_wide(hipStream_t st, int w, const double* G, int ldg, double* T, double* R, int* flag);
void launch_select_evecs(hipStream_t st, int c, int k, const double* evec, double* sel);
void launch_transpose_sign(hipStream_t st, int k, int k1, double sneg, const double* in, double* out);
// batched block Gauss-Jordan inverse of the coarse matrices (ricadi_precond.hip); nb <= RICADI_MAX_GROUPS matrices
int gj_block();
int gj_max_batch();
void launch_gj_prep(hipStream_t st, int nb, double* const* mats, int k, int k0, int nbe, double* Cb, double* Rp,
                    double* D);
void launch_gj_diag(hipStream_t st, int nb, double* D, int nbe, int* flag);
void launch_gj_rows(hipStream_t st, int nb, double* const* mats, int k, int k0, int nbe, const double* Rb);
void launch_combine3(hipStream_t st, size_t n, const double* a0, const double* a1,
                     const double* a2, double alpha, double beta, double* out);
// K7: projected pencil H_A = Q^T cal A Q, H_E = Q^T cal E Q (ricadi_project.hip).  With U != NULL the dense form:
// HA = Q^T U, HE = Q^T V (k x q).  part: project_part_count(nv, k, k or q) doubles of scratch.
size_t project_part_count(int nv, int k, int n2);
void launch_project_pencil(hipStream_t st, int nv, int k, const int* rp, const int* ci, const double* vA,
                           const double* vE, const double* Q, const double* U, const double* V, int q,
                           double* part, double* HA, double* HE);
void launch_project_lowrank(hipStream_t st, int k, int q, const double* QU, const double* QV, double* HA);
// the two-sided form: HA = L^T cal A Rb, HE = L^T cal E Rb (r x r; L, Rb: NV x r row-major, r <= 128);
// part: project_part_count(nv, r, r) doubles
void launch_project_pencil_twosided(hipStream_t st, int nv, int r, const int* rp, const int* ci, const double* vA,
                                    const double* vE, const double* L, const double* Rb, double* part, double* HA,
                                    double* HE);

// coloured Vanka sweep of a child level (ricadi_precond.hip): the patch matrices S[idx, idx] of up to RICADI_MAX_GROUPS
// shifts per launch (mats[i]: npatches x 64 x 64 of shift i; patches from first_lone on: diagonal only); one colour
// z[idx_b] += omega Inv_b rho[idx_b] over the patches [p0, p0 + count); z = Y ec (aggof == nullptr: z = 0)
void launch_vanka_gather(hipStream_t st, int nshift, int npatches, int first_lone, const int* idx, const int* s_rp,
                         const int* s_ci, const GroupPtrs& sval, double* const* mats);
template <class T>
void launch_vanka_patch(hipStream_t st, const GroupTab& gt, int p0, int count, const int* idx, const GroupPtrsT<T>& invs,
                        const double* rho, size_t gsr, double* z, size_t gsz, int m, double omega);
void launch_prolong_plain(hipStream_t st, const GroupTab& gt, int n, int m, const int* aggof, const double* ec,
                          size_t gse, double* z, size_t gsz);
// dst (BF16 bit patterns, round to nearest even) = src (FP64), n entries
void launch_to_bf16(hipStream_t st, size_t n, const double* src, uint16_t* dst);
// The two velocity sweeps of the hot shape driven by the fixed-stride records (block_two32_kernel, block_rect32_kernel):
// same contracts as launch_block_apply2_b / launch_block_apply_rect_b on packed 16-column panels (leading dimension
// 16), for blocks stored as T = double, float or uint16_t (BF16).  Each takes exactly what its predicate admits:
// 32-row blocks, m == 16, a padded width ks (s2.kstride) of 32 or 64, records (recs), group strides whose byte offsets
// fit 32 bits; the rectangles an FP32 intermediate (old32) only with its panel (out32); the two-term sweep no fused
// prolongation (prolong: pa.aggof set).
// pipe (BF16 blocks only): the second segment's loads in flight behind the first segment's MFMAs
bool block_two32_ok(int bs, int m, int ks, bool recs, bool prolong, size_t gso, size_t gs1, size_t gs2);
template <class T>
void launch_block_two32(hipStream_t st, const GroupTab& gt, int nblocks, const SweepRecs& rec, const GroupPtrsT<T>& m1,
                        const Seg2& s1, const GroupPtrsT<T>& m2, const Seg2& s2, double* out, size_t gso,
                        const ProlongArgs& pa, bool pipe = false);
bool block_rect32_ok(int bs, int m, int ks, bool recs, size_t gsi, size_t gso, bool old32, bool out32);
template <class T>
void launch_block_rect32(hipStream_t st, const GroupTab& gt, int ks, int nblocks, const SweepRecs& rec,
                         const GroupPtrsT<T>& mats, const double* in, size_t gsi, double* out, size_t gso, int subtract,
                         const ProlongArgs& pa);

// K2p: the pressure step of the SIMPLE cycle fused into one launch (m = 16, 32 x 32 Schur blocks):
//   out[rows_b] = inv_b (J z + (S Y)_p ec - r_p)[rows_b]  with the epilogue options of the Schur sweep (pa).
// meta: per (block, row of the block) one PSREC_WIDTH-word record (layout: PSREC_* above; ricadi_ctx::ps_meta);
// with_sy = false: no coarse term; z is the n x 16 panel whose
// velocity rows are read, rp_ / rp16 the pressure rows of the residual (FP64 or FP16-stored), out the pressure rows of z.
// zv32 (optional, group stride gsz32): the velocity rows as the FP32 panel the first sweep left (64-B row gathers).
// T = double, float or uint16_t (BF16-stored inverses).
template <class T>
void launch_pressure_step_b(hipStream_t st, const GroupTab& gt, int nblocks, const int* meta,
                            const GroupPtrsT<T>& inv, const int* jci, const double* jv, const double* z,
                            size_t gsz, bool with_sy, const int* syci, const GroupPtrs& syv, const double* ec, size_t gse,
                            const double* rp_, const _Float16* rp16, size_t gsr, double* out, size_t gso,
                            const ProlongArgs& pa, const float* zv32 = nullptr, size_t gsz32 = 0);

// K3h: last Arnoldi pass + Hessenberg / Givens update in one launch (FP16 basis, m = 16; the panel w in FP64 or FP32)
bool update_hess_fused_ok(int m, bool fp16_basis);
template <class WT>
void launch_cols_update16_hess_b(hipStream_t st, const GroupTab& gt, int nrows, int nvec, const _Float16* basis,
                                 size_t vstride, size_t gsb, const double* h1, const double* h2, size_t gsh, int use_sum,
                                 const WT* w, size_t gsw, double* out, size_t gso, _Float16* outf, size_t gsf, int j,
                                 int restart, double* H, double* cs, double* sn, double* g, const double* resid_in,
                                 double* resid_out, const double* bnorm, double tol, double* host_resid);

// K3L: the one-reduction (delayed CGS2) Arnoldi of the same hot path (ricadi_arnoldi.hip).  dots: one pass over V,
// the candidate u_j (slot j) and w, reduced into the group's coefficient block (w32 = NULL: the end-of-cycle pass,
// j = k_g per group); update: derives the coefficients from those sums, completes column j-1 of H~ (workgroup 0),
// writes the provisional residual estimate of column j, v_j into slot j (in place) and the next candidate u_{j+1}
// into slot j+1; close: completes column k_g - 1 after the end-of-cycle dots pass.
bool arnoldi16_lowsync_ok(int restart);
size_t lowsync_partial_stride(int nrows, int restart);   // doubles per group of the partial-sum buffer
size_t lowsync_coef_stride(int restart);                 // doubles per group of the coefficient buffer
void launch_arnoldi16_lowsync_dots(hipStream_t st, const GroupTab& gt, const GroupInts& js, int nrows,
                                   const _Float16* basis, size_t vstride, size_t gsb, const float* w32, size_t gsw,
                                   double* partial, size_t gsp, double* coef, size_t gsc);
void launch_arnoldi16_lowsync_update(hipStream_t st, const GroupTab& gt, int nrows, int j, _Float16* basis,
                                     size_t vstride, size_t gsb, const float* w32, size_t gsw, double* coef,
                                     size_t gsc, int restart, double* H, double* cs, double* sn, double* g,
                                     const double* bnorm, double tol, double* resid_out, double* host_resid);
void launch_arnoldi16_lowsync_close(hipStream_t st, const GroupTab& gt, const GroupInts& ks, double* coef, size_t gsc,
                                    int restart, double* H, double* cs, double* sn, double* g, const double* bnorm,
                                    double tol);

// K5c: pivoted Cholesky of a (possibly augmented) symmetric matrix, 8 / 16 / 32 pivots per launch pair --
// the eigensolver-free recompression (ricadi_dense.hip).  State lives on the device so that the host can
// issue all blocks without a read-back: once `stop` is set the remaining launches return at once.
struct PcholState {
  double d0;     // first pivot (scale of the tolerance)
  int rank;      // rows of the factor written so far
  int stop;      // 1: tolerance / row limit reached
  int nblk;      // rows written by the last panel launch
  int pad;
};
int pchol_block(int nc);          // pivots per panel launch for nc columns (0: nc too large)
void launch_pchol_panel(hipStream_t st, const double* A, int ld, int nr, int nc, double tol, int kmax,
                        PcholState* stt, double* Rout, int ldr, int* done);
void launch_pchol_trail(hipStream_t st, double* A, int ld, int nr, int nc, const PcholState* stt,
                        const double* Rall, int ldr);
void launch_transpose(hipStream_t st, int rows, int cols, const double* in, int ldi, double* out, int ldo);

// K4s: all Z blocks of an ADI sweep + their squared column norms in two launches
bool sweep_combine_ok(int m, int nslot, int G);
size_t sweep_combine_partial_len(int nrows, int m, int G);
void launch_sweep_combine(hipStream_t st, int nrows, int m, int nslot, int G, const double* U, size_t ustride,
                          const double* coef, double* Z, int zld, int zc0, double* partial, double* norms2);

// K4r: the panel P = [W, E U_1, ..., E U_nslot] of an ADI sweep (nrows x (nslot + 1) m) in one launch, and the Gram
// matrix G = P^T P (nc x nc, ld nc) of a row-major panel with every sum in a fixed order (two launches; `partial`:
// gram_fixed_partial_len doubles): the same panel gives bitwise the same G
void launch_sweep_resid_panel(hipStream_t st, int nrows, int m, int nslot, const int* rp, const int* ci,
                              const double* ev, const double* W, const double* U, size_t ustride, double* P);
size_t gram_fixed_partial_len(int n, int nc);
void launch_gram_fixed(hipStream_t st, int n, int nc, const double* P, int ldp, double* partial, double* G);
// K4x: the cross-Gram matrix G = X^T Y (p x q, ld q) of two row-major panels (n x p, ld ldx; n x q, ld ldy;
// p, q <= 1024), the same scheme with every tile block written (`partial`: cross_gram_partial_len doubles)
size_t cross_gram_partial_len(int n, int p, int q);
void launch_cross_gram(hipStream_t st, int n, int p, int q, const double* X, int ldx, const double* Y, int ldy,
                       double* partial, double* G);

// K6: the dense part of a RADI step (ricadi_radi.hip).  vtb: G (m x nb) = V^T B of V (n rows, leading dimension ldv)
// and B (n x nb), sums in a fixed order (`partial`: radi_vtb_partial_len doubles).  factor: one workgroup, m <= 127,
// nb <= 64: Y = I + G G^T = L L^T and C = [sqrt(-2p) L^-T | (-2p) Y^-1 | (-2p) Y^-1 G] (m x (2m + nb)); *flag raised on
// a pivot that is not positive and finite.  update: [R | U] (nv x (m + nb), in place) += (cal E V) C[:, m:], columns
// [zc, zc + m) of Z (leading dimension zld) = V C[:, :m]; V is read on its first nv rows.
size_t radi_vtb_partial_len(int n, int m, int nb);
void launch_radi_vtb(hipStream_t st, int n, int m, int nb, const double* V, int ldv, const double* B, double* partial,
                     double* G);
void launch_radi_factor(hipStream_t st, int m, int nb, double p, const double* G, double* C, int* flag);
void launch_radi_update(hipStream_t st, int nv, int m, int nb, const int* rp, const int* ci, const double* ev,
                        const double* V, int ldv, const double* C, double* RU, double* Z, int zld, int zc);
// reduce: H (k x (2k + m + 2nb), row-major) = Q^T [cal A Q | cal E Q | R | U | B] for the shift selection: Q nv x k
// (ld k), RU = [R | U] nv x (m + nb), B nv x nb; rp / ci / vA / vE the saddle pattern with its two value sources (rows
// and columns below nv); 1 <= nb <= 64; sums in a fixed order (`partial`: radi_reduce_partial_len).  1 <= k, m <= 32:
// radi_reduce_kernel; 33 <= k <= 127: radi_reduce_wide_kernel (output tiles on the FP64 matrix cores), k = m a wide
// block, k != m (1 <= m <= 127, 2k + m + 2nb <= 509) the group of blocks a sweep kept.
size_t radi_reduce_partial_len(int nv, int k, int m, int nb);
void launch_radi_reduce(hipStream_t st, int nv, int k, int m, int nb, const int* rp, const int* ci, const double* vA,
                        const double* vE, const double* Q, const double* RU, const double* B, double* partial,
                        double* H);
// The shift selection on the host (ricadi_host.cpp; ricadi_host_radi_shift): RICADI_OK / RICADI_EBREAKDOWN.  wr_out /
// wi_out (2k each, may be NULL): all eigenvalues of the Hamiltonian.
int radi_shift_select(int k, int m, int nb, const double* H, double* p_out, double* margin_out, double* wr_out,
                      double* wi_out);
// The driver's use of it (ricadi_host.cpp; ricadi_host_radi_next_shift): the basis of the selection from the diagonal
// of the block's R (m x m), H (m x (3m + 2nb)) restricted to it, radi_shift_select.  0 or a RICADI_RADI_REFUSED_*
// value; *kept_out (may be NULL): the size of the basis.
int radi_next_shift(int m, int nb, const double* H, const double* R, double* p_out, double* margin_out, int* kept_out);
// The same with the dominant left singular directions of R as the basis (m <= 127, at most 32 kept;
// ricadi_host_radi_next_shift_dominant).
int radi_next_shift_dominant(int m, int nb, const double* H, const double* R, double* p_out, double* margin_out,
                             int* kept_out);
// The shifts of the next sweep (ricadi_host_radi_sweep_shifts): the dominant rule on a group of c
// columns (H c x (2c + m + 2nb), R c x c), the candidates ordered by criterion, up to `want` admitted greedily under the
// sweep's pivot bound.  0 or a RICADI_RADI_REFUSED_* value.
int radi_next_shifts_dominant(int c, int m, int nb, const double* H, const double* R, int want, double* ps_out,
                              double* crit_out, int* n_out, int* kept_out);
// Square-root balancing of two factors (ricadi_host_lqg_balance): S (kc x kf) = U Sigma V^T by
// the host Jacobi iteration, r = #{sigma_i > tol sigma_1} capped by order (<= 0: no cap), sig_out the min(kc, kf) values,
// coefL = U_r Sigma_r^-1/2 (kc x r), coefR = V_r Sigma_r^-1/2 (kf x r), leading dimension r.  RICADI_OK, RICADI_EINVAL
// (an entry that is not finite), RICADI_EBREAKDOWN (S = 0) or RICADI_ENOCONV (60 sweeps without convergence).
int lqg_balance(int kc, int kf, const double* S, double tol, int order, int* r_out, double* sig_out, double* coefL,
                double* coefR);
// The sweep form of RADI.  Host (ricadi_host.cpp; ricadi_host_radi_sweep / _sweep_width): the kept
// steps, the residual after each and the coefficient matrix Cf (g m x (k m + m + nb)) from what a sweep has fetched;
// the effective width of a cycled list; the column groups the batched solve makes of an (mw + nb)-wide panel; the
// widest sweep those groups and the kernels' RICADI_RADI_SWEEP_MAX_K columns allow.
int radi_sweep(int g, int m, int nb, const double* shifts, const double* Ghat, const double* Gamma, double rhs,
               double res_reltol, int steps_left, int* k_out, double* res_out, double* Cf_out);
int radi_sweep_width(const double* shifts, int ns, int mw, int nb, int want, int max_steps);
int radi_sweep_groups(int mw, int nb);
int radi_sweep_cap(int mw, int nb);
// Device (ricadi_radi.hip): Z[:, zc : zc + k m] = Vh Cf[:, :k m], [R | U] += S Cf[:, k m:]; Vh's panel g at
// V + g vstride (leading dimension ldv, m columns used), S nv x G m with leading dimension lds.
void launch_radi_sweep_combine(hipStream_t st, int nv, int G, int m, int nb, int k, const double* V, size_t vstride,
                               int ldv, const double* S, int lds, const double* Cf, double* RU, double* Z, int zld,
                               int zc);

// K1c / K3c: the complex-shift path (ricadi_cplx.hip).  A complex panel of mc <= 8 columns is
// the real row-major panel of m2 = 2 mc columns (real parts in the even columns, leading dimension m2); group strides
// are in doubles.  Coefficient rows (h, y, the partial sums) hold 16 doubles whatever m2: complex column c at 2c, 2c + 1.
// A shift the complex path takes: finite, not zero, real part <= 0.  Its real proxy shift, at which the (real)
// preconditioner is applied: -2^round(log2 |alpha|), halves rounded up -- the frequencies of a sweep share few setups.
inline bool cplx_shift_ok(double ar, double ai) {
  return std::isfinite(ar) && std::isfinite(ai) && ar <= 0.0 && (ar != 0.0 || ai != 0.0);
}
inline double cplx_proxy(double ar, double ai) {
  return -std::ldexp(1.0, (int)std::floor(std::log2(std::hypot(ar, ai)) + 0.5));
}
struct CplxCoefs {            // alpha_g = ar + i ai and beta_g per group id (by value)
  double ar[RICADI_MAX_GROUPS], ai[RICADI_MAX_GROUPS], beta[RICADI_MAX_GROUPS];
};
// y_g = S(alpha_g, beta_g) x_g: CSR form on the unified saddle pattern with its three value sources; tiled form on the
// multi-shift tile format (lidx with the velocity-velocity flag in bit 15, vAJ, vE; max_cols <= 160)
void launch_cplx_spmm_csr(hipStream_t st, const GroupTab& gt, const CplxCoefs& cf, int nrows, const int* rp,
                          const int* ci, const double* vA, const double* vE, const double* vJ, const double* x,
                          size_t gsx, double* y, size_t gsy, int m2);
bool cplx_spmm_tiled_ok(int max_cols, size_t panel_rows);
void launch_cplx_spmm_tiled(hipStream_t st, const GroupTab& gt, const CplxCoefs& cf, int nblk, const int* rows2,
                            const int* rp2, const int* cols2, const uint16_t* lidx, const double* vAJ, const double* vE,
                            const double* x, size_t gsx, double* y, size_t gsy, int m2, int max_cols);
// out[g][j] = v_j^H w (j < nvec; basis vector j of group g at V + j vstride + g gsv) and, with want_self, ||w||^2 per
// column at row nvec; partial: groups x cplx_num_blocks(n) x ldp x 16 doubles (ldp >= nvec + want_self), summed in block
// order by a second launch; out: rows of 16, group stride gso
int cplx_num_blocks(int nrows);
void launch_cplx_dots(hipStream_t st, const GroupTab& gt, int n, int m2, int nvec, int want_self, const double* V,
                      size_t vstride, size_t gsv, const double* w, size_t gsw, double* partial, int ldp, double* out,
                      size_t gso);
// w_g += sign sum_{j < nvecs[g]} v_j h_j
void launch_cplx_update(hipStream_t st, const GroupTab& gt, const GroupInts& nvecs, int n, int m2, const double* V,
                        size_t vstride, size_t gsv, const double* h, size_t gsh, double sign, double* w, size_t gsw);
// out = a in + b scale[g][column] other on `count` doubles per group (other == NULL: a in; scale == NULL: 1; a == 0:
// `in` is not read)
void launch_cplx_axpby(hipStream_t st, const GroupTab& gt, size_t count, int m2, double a, const double* in, size_t gsi,
                       double b, const double* scale, const double* other, size_t gso, double* out, size_t gsout);
// hout = h1 + h2 (nvec rows), row nvec = (||w||, 0) from nrm2 (16 per group), scale (16 per group) = 1 / ||w|| or 0
void launch_cplx_orth_finish(hipStream_t st, const GroupTab& gt, int nvec, const double* h1, const double* h2,
                             const double* nrm2, size_t gsh, double* hout, double* scale);
// the small stages of the complex GMRES, one wave per group; per (group, column) slots of 8 columns per group:
// Hm restart x (restart + 1) complex, cs restart, sn restart complex, gv (restart + 1) complex, bnorm / resid 8 per group
void launch_cplx_gmres_start(hipStream_t st, const GroupTab& gt, int mc, int restart, const double* nrm2,
                             const double* bnorm, double* gv, double* scale, double* resid);
void launch_cplx_gmres_hess(hipStream_t st, const GroupTab& gt, int mc, int j, int restart, const double* hcol,
                            size_t gsh, double* Hm, double* cs, double* sn, double* gv, const double* bnorm,
                            double* resid);
void launch_cplx_gmres_backsolve(hipStream_t st, const GroupTab& gt, const GroupInts& ks, int mc, int restart,
                                 const double* Hm, const double* gv, double* y, size_t gsy);

// K6c: the pair step of the Lyapunov ADI (ricadi_cplx.hip).  Real column j of a step's panel is
// complex column j % mc of group j / mc.  pack: R_g <- [W, U] with zero imaginary parts and zero padding columns
// (U == NULL with q = 0).  blocks: Z[:, zc .. zc + 2m) <- [gam V1, gam2 Im X], V1 = Re X + delta Im X (nv x m,
// contiguous), norms2[0..2) the squared Frobenius norms of the two blocks; partial: 2 adi_pair_num_blocks(nv) doubles.
int adi_pair_rows();
int adi_pair_num_blocks(int nv);
void launch_adi_pair_pack(hipStream_t st, int nv, int m, int q, int ng, int mc, const double* W, const double* U,
                          double* R, size_t gsr);
void launch_adi_pair_blocks(hipStream_t st, int nv, int m, int mc, double delta, double gam, double gam2,
                            const double* X, size_t gsx, double* Z, int zld, int zc, double* V1, double* partial,
                            double* norms2);

void set_error(const std::string& msg);

}  // namespace ricadi
