/* ricadi.h -- C-ABI of libricadi_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the low-rank Newton-ADI hot path that optconpy reaches
 * through `import sadptprj_riclyap_adi.{proj_ric_utils,lin_alg_utils}`
 * (/root/reference/optcont_main.py:13-14, /root/reference/solve_dae_ric.py:3-4).
 * Every entry point below names the reference-side call it stands behind.
 *
 * Conventions
 *  - plain C types only; all matrices FP64, all indices int32;
 *  - sparse matrices are CSR (rowptr[nrows+1], col[nnz], val[nnz]), sorted or not;
 *  - dense panels are ROW-MAJOR, `ld` = number of columns unless stated
 *    (a C-order numpy array of shape (n, m) is passed as is);
 *  - the caller owns every host buffer; the library copies in / out and keeps
 *    device state only inside the opaque context;
 *  - every function returns 0 on success or a negative RICADI_E* code;
 *    ricadi_last_error() gives the message.  Non-convergence of ADI/Newton is
 *    not an error (the reference just stops at *_max_steps); iteration counts
 *    and histories come back through the stats arrays;
 *  - a context is bound to one GPU and one HIP stream and is NOT thread safe.
 *
 * The operator handled by a context is the saddle-point matrix
 *
 *      S(alpha, beta) = [ beta*A + alpha*E - U*Vt    Jt ]
 *                       [ J                           0  ]
 *
 * with A ("cal A"), E ("cal E") NV x NV, J NP x NV, and an optional low-rank
 * term U (NV x q), Vt (q x NV).  An ADI shift p is (alpha, beta) = (p, 1); the
 * Leray projection uses (1, 0).
 */
#ifndef RICADI_H
#define RICADI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RICADI_OK 0
#define RICADI_EINVAL (-1)    /* bad argument                               */
#define RICADI_EHIP (-2)      /* HIP / rocSOLVER runtime error              */
#define RICADI_ENOCONV (-3)   /* inner Krylov solve missed its tolerance    */
#define RICADI_EBREAKDOWN (-4)/* singular block / coarse matrix             */
#define RICADI_ESTATE (-5)    /* call order violated (operator not set ...) */

typedef struct ricadi_ctx ricadi_ctx;

/* most levels of a hierarchy under ricadi_opts::hierarchy = 1 (a level: a grid with its own sweep; the dense inverse
 * of the last level's coarse problem is not counted) */
#define RICADI_MAX_HIERARCHY_LEVELS 6

/* Options of the inner solver (block-Jacobi + coarse-level preconditioned
 * GMRES).  Zero-initialise and call ricadi_default_opts() first.            */
typedef struct ricadi_opts {
  double gmres_tol;      /* relative residual per column (default 1e-10, the
                            unit of work of SURVEY.md section 8d)            */
  int gmres_restart;     /* max Krylov vectors per cycle (default 30); cycles
                            start at 10 vectors and grow to this whenever a
                            cycle gains less than a factor 10 on some column */
  int gmres_maxit;       /* max iterations per solve (default 3000)         */
  int bj_block;          /* block-Jacobi block size, <= 64 (default 32)     */
  int agg_v;             /* velocity aggregate size of the coarse level     */
  int agg_p;             /* pressure aggregate size of the coarse level     */
  int coarse_max;        /* cap on coarse dimension (default 4096); a stiffness-dominated operator
                            (ricadi_host_sa_criterion true) may use 1.5 x this for its dense inverse:
                            see max_levels and ricadi_host_plan_levels        */
  int use_coarse;        /* 0: one-level block-Jacobi only                  */
  int max_levels;        /* 2: two-level method only.  3 (default): where the coarse problem of the
                            aggregates exceeds coarse_max, it is handed to a child level (the same
                            preconditioner on its Galerkin matrices, aggregates = pairs of velocity
                            aggregates + single pressure aggregates, dense inverse <= coarse_max*9/8)
                            instead of growing the aggregates until a dense inverse fits; the
                            aggregates then only grow (x1.5 per step) until that gentle child fits:
                            0.55 k_v + k_p <= coarse_max (n ~ 1e5 keeps agg_v / agg_p).  A harder-
                            coarsened child makes GMRES stagnate.  Operators the
                            smoothed prolongation applies to keep TWO levels instead, up to k <= 1.5
                            coarse_max, and grow their aggregates up to (121, 182) for it: at their small
                            shifts the child is a poor stand-in for the inverse (n = 2e5: 229 vs 118
                            iterations), and the smoothed coarse operator does not go with a child.
                            Under either rule a level keeps k_p <= k_v (else its coarse saddle matrix is
                            singular): it coarsens its pressure aggregates further for that, and where they
                            cannot join -- they never cross components of the graph of J J^T -- the level
                            goes without a coarse space, as with use_coarse = 0                          */
  int verbose;
  int compress_qr;       /* ricadi_compress: 1 (default) = thin block QR + SVD of R, the reference's
                            "QR ... SVD" (singular values resolved to eps*s_1), for factors of up to
                            1024 columns -- wider ones take the Gram route;  0 = always Gram matrix +
                            eigendecomposition (resolves singular values down to sqrt(eps)*s_1)      */
  int hierarchy;         /* rule of the multilevel hierarchy.  0 (default): the rule of max_levels above.  1 ("fine"):
                            level 0 keeps agg_v / agg_p and never grows them; where its coarse problem exceeds
                            coarse_max it goes to a child level (pairs of velocity aggregates, single pressure
                            aggregates, dense inverse <= coarse_max*9/8), which hands ITS coarse problem to a child
                            in the same way -- at most RICADI_MAX_HIERARCHY_LEVELS levels, one V-cycle visit per
                            level, the last one holds the dense inverse; only if that many levels do not reach the
                            cap does the LAST level grow its aggregates (x1.5 per step); a level whose velocity aggregates
                            would not outnumber its pressure aggregates by a quarter coarsens its pressure further
                            (else the coarse saddle matrix of a deep chain is singular).  Every level with a child
                            uses plain aggregation; the two-level rule for stiffness-dominated operators
                            (ricadi_host_sa_criterion) is not applied; max_levels is ignored.
                            ricadi_host_plan_hierarchy returns the levels.  Set before ricadi_set_operator       */
  int child_smoother;    /* smoother of a child level of the multilevel preconditioner (a hierarchy without a
                            child level ignores it): 0 (default) one SIMPLE block sweep; 1 one coloured Vanka
                            sweep -- per child pressure unknown the patch of itself and the velocity unknowns
                            its row of J touches (at most 64 unknowns), local saddle systems inverted per
                            shift, patches that share no unknown applied together, colour after colour on the
                            updated residual.  Set before ricadi_set_operator                              */
  double child_damping;  /* damping omega of the Vanka sweep (default 0.7); the SIMPLE sweep ignores it.  Set
                            before ricadi_set_operator                                                      */
} ricadi_opts;

/* Parameters of the ADI / Newton loops; same meaning as the keys of the
 * reference's `nwtn_adi_dict` (/root/reference/optcont_main.py:122-131).    */
typedef struct ricadi_adi_params {
  int adi_max_steps;
  double adi_newZ_reltol;
  double adi_res_reltol; /* 0 (default): off.  > 0: second stopping rule of the ADI, on the relative projected
                            Lyapunov residual -- the iteration ends after the first step j with
                            ||W_j^T W_j||_F <= adi_res_reltol * ||W_0^T W_0||_F, W_j the residual factor
                            after step j and W_0 the right-hand side after the optional projection.  The
                            sweep form applies the rule block by block and ends after the same step as
                            the step form as long as the residual has not fallen by more than about
                            eight orders of magnitude within the sweep; below that its value inside the
                            sweep is rounding noise and the tolerance is met in the next sweep (up to
                            sweep_width - 1 steps later).  adi_newZ_reltol keeps working: the
                            rule that fires first ends the iteration (adi_newZ_reltol = 0 switches the
                            reference's rule off).  The residual history is recorded: ricadi_adi_res_history */
  int nwtn_max_steps;
  double nwtn_upd_reltol;
  double nwtn_upd_abstol;
  int project_w;         /* project the rhs factor first (default 1)        */
  int verbose;
  int compress_cols;     /* > 0: recompress the device factor whenever it has
                            grown by this many columns (truncation at
                            sqrt(eps)*sigma_1, i.e. exact to rounding in Z Z^T).
                            0: ricadi_lyap_adi keeps the raw ADI columns like
                            the reference; ricadi_ric_newtonadi uses 512.      */
  int sweep_width;       /* 1 (default): ADI steps one at a time, as the reference.
                            G > 1: sweep form -- G consecutive steps (distinct
                            shifts) are solved together in one batched GMRES and
                            recombined with their Cauchy matrix; same Z Z^T, the
                            stopping rule is applied every G steps.  Falls back to
                            1 when the shift list has repeats, fewer than G
                            entries or an ill-conditioned Cauchy matrix.  G <= 16;
                            the drop-in's proj_alg_ric_newtonadi and the benchmark
                            use 16 (the whole shift cycle of cfg2 in one sweep).  */
} ricadi_adi_params;

const char* ricadi_last_error(void);
int ricadi_version(void);
/* sizeof(ricadi_opts) / sizeof(ricadi_adi_params) as THIS build of the library sees
 * them.  A binding whose mirror of the structs has another size must refuse to load:
 * the library reads every field of the structs it is handed, so a shorter mirror makes
 * it read past the caller's buffer (optconpy_amd/_lib.py checks this at load time). */
int ricadi_sizeof_opts(void);
int ricadi_sizeof_adi_params(void);
/* Field types of the two structs in declaration order, d = double, i = int:
 * "ricadi_opts:<types>;ricadi_adi_params:<types>" -- sizes alone cannot see a
 * trailing int that hides in the tail padding.                                   */
const char* ricadi_struct_signature(void);
void ricadi_default_opts(ricadi_opts* o);
void ricadi_default_adi_params(ricadi_adi_params* p);

/* ---- context ---------------------------------------------------------- */
int ricadi_create(int device_id, ricadi_ctx** ctx);
int ricadi_destroy(ricadi_ctx* ctx);
int ricadi_set_opts(ricadi_ctx* ctx, const ricadi_opts* o);
/* HIP stream all work of this context is enqueued on (as a void*).          */
void* ricadi_stream(ricadi_ctx* ctx);
int ricadi_synchronize(ricadi_ctx* ctx);

/* ---- operator ---------------------------------------------------------
 * Replaces the (amat, mmat, jmat) arguments of
 * pru.solve_proj_lyap_stein / pru.proj_alg_ric_newtonadi
 * (/root/reference/tests/test_units_compfacres_compress.py:62-64,
 *  /root/reference/optcont_main.py:488-492, solve_dae_ric.py:152-159) and of
 * lau.solve_sadpnt_smw (/root/reference/solve_dae_ric.py:192-194).
 * A = cal A, E = cal E already in the orientation they are applied in
 * (the Python shim resolves `transposed`).
 *
 * Replacing an operator.  A context may be given one operator after another,
 * of any size, constraint count and hierarchy depth:
 *  - A replacement forgets everything tied to the resident operator: the
 *    per-shift cache (child levels included), the child level, the low-rank
 *    term (q = 0), the resident factor, the workspace sizes, the recycled
 *    right-hand sides and their solutions, and everything a reporter says "of
 *    the last call" (ADI residual history and stop rule, Newton history and
 *    stop rule, RADI shift history,
 *    fallbacks, sweep info and widths, the probes' last-call counters, the
 *    kernel forms of ricadi_setup_info): asked right after the call, a
 *    reporter answers as a fresh context's does.
 *  - A replacement keeps the settings (options, ricadi_set_recycle, the RADI
 *    shift mode, sweep width and sweep shifts, ricadi_set_adi_res_history, the
 *    probe's refuse list, the exchange) and the counters documented as
 *    cumulative (ricadi_solve_trace, the iteration totals,
 *    ricadi_exchange_count).  Device buffers keep their capacity.
 *  - The solves are iterative and start from zero: after a replacement the
 *    context computes what a fresh context with the same options computes.
 *  - A replacement refused during validation leaves the old operator intact:
 *    NULL arrays, bad sizes, a column index out of range, a refusal of the
 *    host setup.  The old operator, its cache and its factor answer as before.
 *  - A replacement that fails after it began leaves no operator: every call
 *    that needs one refuses with "set the operator first" until
 *    ricadi_set_operator or ricadi_set_dims succeeds.                        */
int ricadi_set_operator(ricadi_ctx* ctx, int nv, int np,
                        const int32_t* a_rowptr, const int32_t* a_col, const double* a_val,
                        const int32_t* e_rowptr, const int32_t* e_col, const double* e_val,
                        const int32_t* j_rowptr, const int32_t* j_col, const double* j_val);

/* Drop the per-shift data (assembled values, block inverses, coarse inverse)
 * cached for every (alpha, beta) used so far; they are rebuilt on demand.
 * ricadi_clear_cache forgets the per-shift data and the recycled right-hand
 * sides, on every level; it keeps the operator, the child level, the low-rank
 * term, the resident factor, the settings and every reporter's last answer.
 * It also keeps the slots of the ring of recycled right-hand sides (emptied):
 * they refill in another order than a new context's growing ring, so recycled
 * initial guesses after it may differ from a new context's in the last bits.   */
int ricadi_clear_cache(ricadi_ctx* ctx);

/* Dimension-only context (no operator): enough for ricadi_compress and for
 * ricadi_gain with an explicit `mt_*` matrix, which need NV only.
 * ricadi_set_dims forgets exactly what ricadi_set_operator forgets (one helper
 * serves both) and keeps what it keeps; the context then has no operator until
 * the next ricadi_set_operator.                                              */
int ricadi_set_dims(ricadi_ctx* ctx, int nv);

/* Low-rank term  - U * Vt ;  U is NV x q row-major, V is NV x q row-major
 * (i.e. Vt = V^T).  q = 0 removes it.  Stands behind the umat / vmat
 * arguments of lau.solve_sadpnt_smw (/root/reference/solve_dae_ric.py:192-194,
 * optcont_main.py:510-514).                                                 */
int ricadi_set_lowrank(ricadi_ctx* ctx, const double* U, const double* V, int q);

/* ---- K1: saddle-point SpMM (testable kernel) --------------------------
 * Y = S(alpha, beta) * X for an n x m panel, n = NV + NP (host buffers).    */
int ricadi_spmm(ricadi_ctx* ctx, double alpha, double beta,
                const double* X, int m, double* Y);

/* Preconditioner alone: Z = P(alpha,beta)^-1 * R  (n x m), for tests.       */
int ricadi_precond_apply(ricadi_ctx* ctx, double alpha, double beta,
                         const double* R, int m, double* Z);

/* Preconditioner as the lockstep GMRES iteration applies it, for tests (device panels).  ng shifts
 * (alphas[g], betas[g]); R_g = dR + g*r_stride (n x m, r_stride >= n*m); Z_g = dZ + g*n*m (FP64).  The form
 * is the iteration's for a batch of ng panels of width m: where it hands the preconditioner the FP16-stored
 * Krylov vector, R is rounded to FP16 into that storage and the FP64 panel handed along holds NaN; where the
 * operator reads the FP32-stored Z_j, Z is that FP32 panel (widened).  active (may be NULL = all): the nactive
 * distinct group ids the application acts on; the other panels of dZ are not written.  form_out (may be NULL):
 * the branch each stage took, RICADI_PCF_* bits below.  ng*m <= 2048.  No reference counterpart.            */
#define RICADI_PCF_H16 (1 << 0)          /* input read from the FP16-stored vector                            */
#define RICADI_PCF_X32 (1 << 1)          /* output: the FP32 panel only (the operator reads it)               */
#define RICADI_PCF_MID32 (1 << 2)        /* velocity part between the sweeps as an FP32 panel                 */
#define RICADI_PCF_B16 (1 << 3)          /* BF16-stored per-shift blocks                                      */
#define RICADI_PCF_RESTRICT_SHIFT 4      /* 2 bits: restriction 1 one wave per row, 2 FP16 CSR, 3 FP64 CSR   */
#define RICADI_PCF_COARSE_SHIFT 6        /* 2 bits: coarse problem 1 child level's cycle, 2 dense inverse     */
#define RICADI_PCF_PFUSED (1 << 8)       /* pressure step in one launch                                       */
#define RICADI_PCF_PSPLIT (1 << 9)       /* pressure step in three launches                                   */
#define RICADI_PCF_FIRST_SHIFT 10        /* 2 bits: first velocity sweep 1 record-driven two-term on BF16 blocks,
                                            2 two-term on FP32- or FP64-stored blocks (record-driven kernel where
                                            the level has records and the shape admits it, generic kernel
                                            otherwise), 3 plain block sweep                                   */
#define RICADI_PCF_LAST_SHIFT 12         /* 2 bits: last velocity sweep 1 record-driven rectangle on BF16 blocks,
                                            2 rectangle on FP32- or FP64-stored blocks (record-driven or generic
                                            kernel, as above), 3 J^T product formed row by row (CSR in)       */
#define RICADI_PCF_FOLDED (1 << 14)      /* folded cycle (coarse residual inside the first sweep)             */
#define RICADI_PCF_VANKA (1 << 15)       /* a child level's cycle with the coloured Vanka sweep: coarse correction,
                                            then per colour the residual and the patch kernel (no SIMPLE sweeps:
                                            first / last sweep and pressure step read 0)                       */
#define RICADI_PCF_TWO_KS_SHIFT 16       /* 8 bits: padded width of the two-term sweep's second block (0: none) */
#define RICADI_PCF_RECT_KS_SHIFT 24      /* 8 bits: padded width of the rectangle sweep's blocks (0: none)    */
int ricadi_precond_apply_batch_dev(ricadi_ctx* ctx, int ng, const double* alphas, const double* betas,
                                   const double* dR, int64_t r_stride, int m, const int32_t* active,
                                   int nactive, double* dZ, int* form_out);

/* The saddle product y_g = beta_r r_g + alpha S(alphas[g], betas[g]) x_g as the lockstep GMRES launches it
 * (the operator product of the iteration and the restart residual), for tests: a batch of ng panels of width m,
 * x_g = dX + g*x_stride, y_g = dY + g*y_stride, r_g = dR + g*r_stride (device FP64, row-major, ld m; every stride
 * >= n*m).  active (may be NULL = all ng): the group ids to apply it to; the other panels of dY are not written.
 * flags: RICADI_OA_X32 the input is rounded to FP32 on the device first (as the iteration stores Z_j);
 * RICADI_OA_Y32 the product goes to an FP32 panel, returned widened in dY; RICADI_OA_LOWRANK the term - U V^T x_v
 * of ricadi_set_lowrank; RICADI_OA_RESIDUAL the term beta_r r_g (else dR is ignored).  The FP32 forms exist for
 * the plain product where the tiles of the operator fit (else RICADI_EINVAL).  variant_out (may be NULL): the
 * kernel form that ran, as ricadi_setup_info's k1_variant. */
#define RICADI_OA_X32 1
#define RICADI_OA_Y32 2
#define RICADI_OA_LOWRANK 4
#define RICADI_OA_RESIDUAL 8
int ricadi_op_apply_batch_dev(ricadi_ctx* ctx, int ng, const double* alphas, const double* betas, const double* dX,
                              int64_t x_stride, int m, const int32_t* active, int nactive, int flags, double alpha,
                              const double* dR, int64_t r_stride, double beta_r, double* dY, int64_t y_stride,
                              int* variant_out);

/* Structure of the preconditioner cycle of level `level` (0: this context, 1: its child level, ...), for
 * tests.  sizes_out[16] = [nv, np, nbv, nbp, bs, kc, kcv, kcp, smoothed aggregation, nnz(P), has a child level,
 * folded cycle, rectangle last sweep, FP32-stored operands, 0, 0].  Call with the arrays NULL for the sizes,
 * then again with bv_ptr[nbv+1], bv_rows[nv], bp_ptr[nbp+1], bp_rows[np], aggof[n] (dof -> coarse index),
 * p_rp[n+1], p_ci[nnz(P)], p_v[nnz(P)] (the prolongation P, CSR over all n rows); any of them may be NULL. */
int ricadi_precond_structure(ricadi_ctx* ctx, int level, int32_t* sizes_out, int32_t* bv_ptr, int32_t* bv_rows,
                             int32_t* bp_ptr, int32_t* bp_rows, int32_t* aggof, int32_t* p_rp, int32_t* p_ci,
                             double* p_v);

/* The patches of the coloured Vanka sweep of level `level` (>= 1: a child level) as the device uses them, for
 * tests; sizes_out and the records as ricadi_host_vanka_patches returns them (all sizes 0 where the level has no
 * Vanka sweep).  Call with the arrays NULL for the sizes, then again with colour_ptr[colours + 1] and
 * patch_idx[64 * patches]; either may be NULL.                                                                   */
int ricadi_precond_vanka(ricadi_ctx* ctx, int level, int32_t* sizes_out, int32_t* colour_ptr, int32_t* patch_idx);

/* ---- one shift-solve ---------------------------------------------------
 * Solve S(alpha,beta) [V; L] = [R; Rp] for an NV x m panel R (Rp may be
 * NULL = 0).  X_out is n x m (velocity rows first).  iters_out[1],
 * relres_out[m] may be NULL.  This is the unit of the `shift-solves/s`
 * metric; stands behind lau.solve_sadpnt_smw.                              */
int ricadi_shift_solve(ricadi_ctx* ctx, double alpha, double beta,
                       const double* R, const double* Rp, int m,
                       double* X_out, int* iters_out, double* relres_out);

/* ---- a2: low-rank ADI for the projected Lyapunov equation -------------
 * pru.solve_proj_lyap_stein (/root/reference/tests/test_units_compfacres_compress.py:62-64).
 * W is NV x m.  Z_out must hold NV x (adi_max_steps*m) doubles, row-major
 * with ld = *c_out on return (columns are packed).  Z_out may be NULL: the
 * factor then stays on the device (see ricadi_factor_*).
 * stats_out (may be NULL, else >= 8 doubles) receives [steps, rel_newZ,
 * total_gmres_iters, shift_solves, ||W_end^T W_end||_F, shift-solves that
 * missed the GMRES tolerance, their worst relative residual, solves repeated
 * with wider storage].                                                      */
int ricadi_lyap_adi(ricadi_ctx* ctx, const double* shifts, int nshifts,
                    const double* W, int m, const ricadi_adi_params* prm,
                    double* Z_out, int* c_out, double* stats_out);

/* Relative projected Lyapunov residual ||W_j^T W_j||_F / ||W_0^T W_0||_F after every ADI step of the most recent
 * Lyapunov solve of the context (ricadi_lyap_adi; for ricadi_ric_newtonadi(_dev) the solve of the last Newton
 * step): entry j-1 belongs to step j.  *n_out = number of steps recorded; at most `cap` entries are copied to
 * `out` (may be NULL with cap = 0).  The history is recorded when adi_res_reltol > 0 or after
 * ricadi_set_adi_res_history(ctx, 1); otherwise nothing is computed for it and *n_out = 0.  RICADI_ESTATE before
 * any ADI call.  No reference counterpart.
 * After ricadi_ric_radi(_dev) it is that call's history instead: the relative projected RICCATI residual
 * ||R_j^T R_j||_F / ||R_0^T R_0||_F after every RADI step -- always recorded there, the quantity is free.        */
int ricadi_adi_res_history(ricadi_ctx* ctx, double* out, int cap, int* n_out);
/* on != 0: record the residual history also while adi_res_reltol = 0 (no rule is added by it).                 */
int ricadi_set_adi_res_history(ricadi_ctx* ctx, int on);
/* The rule that ended the most recent Lyapunov solve of the context (as above).  Every slot of the two stats
 * arrays is taken -- slot 7 of ricadi_lyap_adi's is the count of solves repeated with wider storage --, so the
 * value has a call of its own instead of a slot.  RICADI_ESTATE before any ADI call.  After ricadi_ric_radi(_dev):
 * the rule that ended that call, RICADI_STOP_RES (res_reltol) or RICADI_STOP_MAX_STEPS (max_steps).             */
#define RICADI_STOP_MAX_STEPS 0          /* adi_max_steps reached                                               */
#define RICADI_STOP_NEWZ 1               /* relative norm of the new block below adi_newZ_reltol                */
#define RICADI_STOP_RES 2                /* relative residual at or below adi_res_reltol                        */
int ricadi_adi_stop_rule(ricadi_ctx* ctx, int* rule_out);
/* Kernel launches the residual rule has added since the context was created (three per sweep, two per step and two
 * for the right-hand side of the step form; 0 while neither the rule nor the history is on), for tests.          */
int ricadi_adi_res_launches(ricadi_ctx* ctx, int64_t* n_out);

/* ---- low-rank ADI with complex-conjugate shift pairs (exports added under the same ABI number) --
 * ricadi_lyap_adi_cplx:  ricadi_lyap_adi -- same conventions for W, Z_out, c_out, stats_out -- for a list whose entry i
 *   is the real shift shifts_re[i] where shifts_im[i] == 0 and else the PAIR (p, conj p), p = shifts_re[i] + i
 *   shifts_im[i].  A pair is the real-arithmetic step of Benner, Kuerschner and Saak (2013): one complex solve, two real
 *   blocks of Z, a real residual factor behind it.  It counts as two steps (stats_out[0], adi_max_steps, the residual
 *   history: both entries of a pair hold the residual behind the pair) and as one shift solve (stats_out[3]); it is
 *   never split -- with one step left before adi_max_steps and a pair due the iteration ends one step short with
 *   RICADI_STOP_MAX_STEPS, and the rules are read after a pair's second block.  A low-rank term of the context is
 *   applied around the complex solve (Sherman-Morrison-Woodbury; a numerically singular capacitance matrix is an error).
 *   Step form only: with a pair in the list prm->sweep_width is not used (the Cauchy recombination of the sweep form is
 *   real).  With every shifts_im[i] == 0 the call IS ricadi_lyap_adi(ctx, shifts_re, ...), sweep form included.
 *   RICADI_EINVAL: a shift that is not finite or has shifts_re[i] >= 0; with a pair in the list also m + q > 128 (q the
 *   width of the low-rank term) and a context with an exchange (ricadi_set_exchange: sharded, or a forced one).
 * ricadi_adi_pair_blocks_dev:  the blocks kernel of the pair step alone, for tests.  dX: ng groups of n x mc complex
 *   solutions (device, 16-byte aligned, group stride n mc complex; n = NV + NP, only the first NV rows of a group are
 *   read), real column j < m of the step in complex column j % mc of group j / mc.  With delta = ar / ai, gam = 2
 *   sqrt(-ar):  V1 = Re X + delta Im X  to dV1 (NV x m, contiguous),  gam V1  to columns zc .. zc + m of dZ (leading
 *   dimension ldz >= zc + 2 m),  gam sqrt(delta^2 + 1) Im X  to the m columns behind; norms2_out[2] (host): the squared
 *   Frobenius norms of the two blocks, summed in a fixed order.
 * ricadi_adi_pair_info:  of the last ricadi_lyap_adi_cplx call: [pair entries solved, lockstep iterations of their
 *   complex GMRES (per solve the slowest group's, refinement included), Woodbury refinement passes, complex solves
 *   that missed their tolerance].  All zero after a call without pairs.
 * ricadi_adi_pair_solve_dev (ABI 414, for tests):  the complex solve of ONE pair entry at p = ar + i ai, as the driver
 *   runs it on the context's operator and low-rank term (width q): the proxy shift's setup, [W, U] packed into ng groups
 *   of mc complex columns ((ng, mc) of m + q columns), the lockstep solve, with q > 0 the Sherman-Morrison-Woodbury
 *   correction and -- a column's true residual above 10 gmres_tol -- its one refinement pass.  No projection of W, no
 *   blocks kernel, no update of W or Z, no stopping bookkeeping; ricadi_adi_pair_info keeps what it held.  dW: NV x m
 *   (device, read only).  what_mask: 1  dRhs (ng groups of NV x mc complex, 16-byte aligned) <- the packed right-hand
 *   sides, written by the pack kernel itself;  2  dRaw (2 ng groups of n x mc complex, n = NV + NP) <- with q > 0 the
 *   groups as first solved, before any correction, and behind them, where the refinement ran, its uncorrected D;
 *   4  dX (ng groups of n x mc complex) <- the final groups;  8  stop behind the pack (no solve).  A pointer whose bit
 *   is not set may be NULL.  report[8] (host): ng, mc, lockstep iterations, refinement ran (0 / 1), the largest true
 *   relative residual of W's columns before the refinement, the same after it (equal where it did not run), converged
 *   (0 / 1: after <= 10 gmres_tol with q > 0, every column at gmres_tol with q = 0), the smallest pivot modulus of the
 *   capacitance LU over max |cap_ij| (NaN with q = 0).  RICADI_EINVAL as ricadi_adi_pair_blocks_dev, m + q > 128, an
 *   exchange: the outputs stay untouched.  A numerically singular capacitance matrix is RICADI_EHIP with report[0 .. 2]
 *   and report[7] filled.                                                                                          */
int ricadi_lyap_adi_cplx(ricadi_ctx* ctx, const double* shifts_re, const double* shifts_im, int nshifts,
                         const double* W, int m, const ricadi_adi_params* prm, double* Z_out, int* c_out,
                         double* stats_out);
int ricadi_adi_pair_blocks_dev(ricadi_ctx* ctx, int ng, int mc, int m, double ar, double ai, const double* dX,
                               double* dZ, int ldz, int zc, double* dV1, double* norms2_out);
int ricadi_adi_pair_info(ricadi_ctx* ctx, int64_t out[4]);
int ricadi_adi_pair_solve_dev(ricadi_ctx* ctx, double ar, double ai, const double* dW, int m, int what_mask,
                              double* dRaw, double* dX, double* dRhs, double* report);

/* ---- a1: Newton-Kleinman ADI for the projected Riccati equation -------
 * pru.proj_alg_ric_newtonadi (/root/reference/optcont_main.py:488-492,
 * /root/reference/solve_dae_ric.py:152-159).  B is NV x nb dense, W NV x mw,
 * Z0 NV x c0 (or NULL), oldB NV x nb (mtxoldb, or NULL).  Z_out capacity
 * NV x zcap doubles (zcap >= adi_max_steps*(mw+nb)); may be NULL.
 * stats_out (>= 12 doubles): [newton_steps, last_upd_abs, last_upd_rel,
 * total_adi_steps, total_gmres_iters, shift_solves, shift-solves that missed
 * the GMRES tolerance, their worst relative residual, ||W_end^T W_end||_F of the
 * last Lyapunov solve (its projected residual norm: `check_lyap_res`,
 * /root/reference/optcont_main.py:130), ||W_0^T W_0||_F of its right-hand side,
 * solves repeated with wider storage, batched ADI sweeps run (sweep form)].     */
int ricadi_ric_newtonadi(ricadi_ctx* ctx, const double* shifts, int nshifts,
                         const double* B, int nb, const double* W, int mw,
                         const double* Z0, int c0, const double* oldB,
                         const ricadi_adi_params* prm,
                         double* Z_out, int zcap, int* c_out, double* stats_out);

/* ---- a3: column compression -------------------------------------------
 * pru.compress_Zsvd (/root/reference/optcont_main.py:498-499,
 * solve_dae_ric.py:162-163).  Keeps singular values > thresh (thresh < 0:
 * no threshold) and at most kmax (kmax <= 0: no cap).  Z == NULL compresses
 * the factor left on the device by the last ADI / Newton call.  Zc_out is
 * NV x *k_out row-major; sv_out (may be NULL) receives min(c, NV) singular
 * values.                                                                  */
int ricadi_compress(ricadi_ctx* ctx, const double* Z, int c, double thresh, int kmax,
                    double* Zc_out, int* k_out, double* sv_out);

/* The recompression the ADI / Newton drivers apply to their own factor while it grows (no counterpart
 * in the reference, which compresses once through pru.compress_Zsvd,
 * /root/reference/solve_dae_ric.py:161-165): Zc with Zc Zc^T = Z Z^T up to rel^2 ||Z Z^T||, by a pivoted
 * Cholesky factorisation of the Gram matrix and an orthonormalisation of its factor's rows -- no
 * eigensolver, no singular values.  Exposed for tests and timing; `rel` <= 0 takes the drivers' own
 * level (3e-8).  Zc_out must hold NV x c doubles; *k_out columns are written (row-major, ld = *k_out).  */
int ricadi_recompress(ricadi_ctx* ctx, const double* Z, int c, double rel, double* Zc_out, int* k_out);

/* ---- a4: factored product  E * (Z * (Z^T * B)) -------------------------
 * pru.get_mTzzTtb(MT, Z, tb) (/root/reference/optcont_main.py:505-506,
 * solve_dae_ric.py:101,183,189); the feedback gain is its negative.
 * `mt_*` is the CSR of the matrix applied from the left (NV x NV); NULL uses
 * cal E of the context.  Z == NULL uses the device-resident factor.         */
int ricadi_gain(ricadi_ctx* ctx,
                const int32_t* mt_rowptr, const int32_t* mt_col, const double* mt_val,
                const double* Z, int c, const double* B, int nb, double* K_out);

/* ---- a5: squared projected Lyapunov residual norm from factors ---------
 * pru.comp_proj_lyap_res_norm(Z, F, M, W, J)
 * (/root/reference/tests/test_units_compfacres_compress.py:82,104).
 * Uses the context operator: cal A = F^T, cal E = M^T, low-rank term.      */
int ricadi_lyap_res_norm(ricadi_ctx* ctx, const double* Z, int c,
                         const double* W, int m, double* res2_out);

/* ---- device-resident factor -------------------------------------------- */
int ricadi_factor_cols(ricadi_ctx* ctx, int* c_out);
int ricadi_factor_get(ricadi_ctx* ctx, double* Z_out, int c);
int ricadi_factor_set(ricadi_ctx* ctx, const double* Z, int c);
/* ... into a DEVICE buffer (NV x c row-major, ld = c; c = ricadi_factor_cols) */
int ricadi_factor_get_dev(ricadi_ctx* ctx, double* dZ_out, int c);

/* a1 with every panel ALREADY IN HBM (no PCIe traffic inside the call; the reference's callers hand numpy
 * arrays over, /root/reference/solve_dae_ric.py:152-159 -- this is the same call for a host side that keeps
 * its panels on the device between calls, e.g. one backward time step after the other): dB NV x nb, dW NV x mw,
 * dZ0 NV x c0 (NULL with c0 = 0), dOldB NV x nb or NULL, all row-major with leading dimension = width.
 * The new iterate stays in the context's factor (ricadi_factor_cols / _get / _get_dev).
 * stats_out as ricadi_ric_newtonadi.                                                                        */
int ricadi_ric_newtonadi_dev(ricadi_ctx* ctx, const double* shifts, int nshifts,
                             const double* dB, int nb, const double* dW, int mw,
                             const double* dZ0, int c0, const double* dOldB,
                             const ricadi_adi_params* prm, int* c_out, double* stats_out);
/* Both entries of a1 return RICADI_EINVAL before anything is launched for nwtn_max_steps < 1 and adi_max_steps < 1
 * (ABI 413; a loop that never ran used to answer with the factor an earlier call had left in the context), as for
 * bad widths, a NULL panel and a shift >= 0.  After a refused call the resident factor, the histories and every
 * other reporter answer as before it.
 *
 * ricadi_newton_history (ABI 413): one row of six doubles per Newton step of the most recent ricadi_ric_newtonadi(_dev)
 * call of the context, row k-1 for step k:
 *   [upd_abs = ||Z_k Z_k^T - Z_{k-1} Z_{k-1}^T||_F, upd_rel = upd_abs / ||Z_k Z_k^T||_F, ADI steps of the step,
 *    columns of the raw ADI factor before the step's recompression, columns kept, ||Z_k Z_k^T||_F].
 * *n_out = number of steps; at most `cap` ROWS (6 * cap doubles) are copied to `out` (may be NULL with cap = 0).
 * Always recorded (six doubles per step); on a sharded context after rank 0's decision has gone round, so every
 * rank holds rank 0's row.  The last row's first two entries are stats_out[1] and stats_out[2] of the call.
 * RICADI_ESTATE before any Newton call.
 * ricadi_newton_stop_rule: the rule that ended that call.  Where both tolerances are met at one step it reports
 * RICADI_NEWTON_STOP_ABSTOL, the first test of `upd_abs < nwtn_upd_abstol || upd_rel < nwtn_upd_reltol`.        */
#define RICADI_NEWTON_STOP_MAX_STEPS 0   /* nwtn_max_steps reached                                              */
#define RICADI_NEWTON_STOP_ABSTOL 1      /* update norm below nwtn_upd_abstol                                   */
#define RICADI_NEWTON_STOP_RELTOL 2      /* relative update norm below nwtn_upd_reltol                          */
int ricadi_newton_history(ricadi_ctx* ctx, double* out, int cap, int* n_out);
int ricadi_newton_stop_rule(ricadi_ctx* ctx, int* rule_out);

/* ---- a1r: low-rank RADI for the projected Riccati equation (Benner, Bujanovic, Kuerschner, Saak, Numer. Math.
 * 2018; pru.proj_alg_ric_radi; no reference counterpart) -------------------------------------------------------
 * The same equation as a1, cal A X cal E^T + cal E X cal A^T - cal E X B B^T X cal E^T + W W^T = 0 on ker J
 * (with oldB: cal A + oldB B^T in place of cal A), solved directly for X = Z Z^T: one saddle-point shift solve with
 * the current closed loop per step, no outer iteration, no initial iterate.  With R_0 = P^T W (project_w != 0;
 * else W is taken as projected), U_0 = -oldB (or 0), step j with the real shift p < 0 of the cycle is
 *   [[cal A - U B^T + p cal E, J^T], [J, 0]] [V; *] = [R; 0],   G = V^T B,   Y = I + G G^T = L L^T,
 *   Z <- [Z, sqrt(-2p) V L^-T],   T = (-2p) V Y^-1,   R <- R + cal E T,   U <- U + (cal E T) G.
 * The Riccati residual of Z Z^T is exactly R R^T: the call stops with RICADI_STOP_RES once
 * ||R_j^T R_j||_F / ||R_0^T R_0||_F <= res_reltol, else with RICADI_STOP_MAX_STEPS after max_steps
 * (ricadi_adi_stop_rule; the history: ricadi_adi_res_history).  The factor grows by mw columns per step and is
 * recompressed whenever it has grown by compress_cols columns (<= 0: 512); it stays in the context
 * (ricadi_factor_cols / _get / _get_dev).  Shift solves that miss the GMRES tolerance are counted, not fatal.
 * B NV x nb, W NV x mw, oldB NV x nb or NULL; 1 <= nb <= 64, mw >= 1, mw + nb <= 128.  Z_out (may be NULL): NV x zcap
 * doubles, zcap >= max_steps * mw.  K_out (may be NULL): the gain cal E X B = U + oldB, NV x nb.
 * stats_out (>= 8 doubles): [steps, last relative residual, ||R_0^T R_0||_F, total GMRES iterations, shift solves,
 * solves that missed the tolerance, their worst relative residual, solves repeated with wider storage].
 * RICADI_EINVAL, before anything is launched, for bad widths, max_steps < 1, nshifts < 1, a shift >= 0 and
 * zcap < max_steps * mw with Z_out given; RICADI_ESTATE on a context with an exchange set (nothing is sharded here);
 * RICADI_EBREAKDOWN when Y has a pivot that is not positive and finite (NaN / Inf in a solve).
 * Recycling of solved right-hand sides (ricadi_set_recycle) is off inside the call and as before after it.
 * With a sweep width above 1 (ricadi_set_radi_sweep_width below; ABI 411; default 1) and RICADI_RADI_SHIFTS_CYCLE, up to
 * that many consecutive steps are solved in ONE lockstep batch against the same panel and recombined: the same steps,
 * history, stopping rule and gain; stats_out[4] then counts every solve issued.                                     */
int ricadi_ric_radi(ricadi_ctx* ctx, const double* shifts, int nshifts, const double* B, int nb, const double* W,
                    int mw, const double* oldB, int max_steps, double res_reltol, int compress_cols, int project_w,
                    int verbose, double* Z_out, int zcap, int* c_out, double* K_out, double* stats_out);
/* a1r with every panel ALREADY IN HBM (row-major, leading dimension = width; dOldB and dK_out may be NULL); the
 * factor stays in the context.                                                                                  */
int ricadi_ric_radi_dev(ricadi_ctx* ctx, const double* shifts, int nshifts, const double* dB, int nb,
                        const double* dW, int mw, const double* dOldB, int max_steps, double res_reltol,
                        int compress_cols, int project_w, int verbose, int* c_out, double* dK_out,
                        double* stats_out);
/* Where ricadi_ric_radi(_dev) takes its shifts from; a context setting like ricadi_set_recycle, default CYCLE.
 *   RICADI_RADI_SHIFTS_CYCLE        the caller's list, cycled.
 *   RICADI_RADI_SHIFTS_HAMILTONIAN  shifts[0] for the first step; every later shift is generated from the state of the
 *     iteration ("residual Hamiltonian shifts", section 4.5 of the RADI paper): with Q an orthonormal
 *     basis of the new block of Z (k <= mw columns, all in ker J: the columns of the block's QR whose diagonal entry
 *     of R is at least RICADI_RADI_RANK_TOL = 3e-8 of the largest one),
 *       H_A = Q^T cal A Q, H_E = Q^T cal E Q, H_R = Q^T R, H_U = Q^T U, H_B = Q^T B,
 *       A_c = H_A - H_U H_B^T,  At = H_E^-1 A_c,  Rt = H_E^-1 H_R,
 *       Ham = [[At^T, -H_B H_B^T], [-Rt Rt^T, -At]]   (2k x 2k),
 *     the candidates are the eigenvalues of Ham with negative real part, one of each conjugate pair; the next shift is
 *     p = -|lambda| of the candidate whose eigenvector x = [r; q] has the largest ||q|| / ||x||.  The list is the
 *     fallback (a counter of its own, cycling, starting at shifts[1]): no candidate, a shift that is not finite and
 *     negative, or a breakdown of the selection (ricadi_host_radi_shift).
 *     Requires mw <= 32 (else ricadi_ric_radi(_dev) return RICADI_EINVAL before anything is launched).  Only shifts[0]
 *     is set up in advance; a generated shift's per-shift data are rebuilt in ONE entry the context owns and never
 *     enter the per-shift cache: after the call the cache holds what it held before plus the entries of the list that
 *     were used.
 *   RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT  the same rule on another basis: with Q R the QR of the
 *     new block, the basis is Q S, S (mw x k) the left singular vectors of R of its k = min(32, #{sigma_i >=
 *     RICADI_RADI_RANK_TOL sigma_1}) largest singular values -- the dominant part of the block's range, whatever the
 *     order of its columns.  The selection stays of order 2k <= 64 for any width: accepted for 1 <= mw <= 127,
 *     nb <= 64 (and mw + nb <= 128), RADI's own limits.  Everything else -- first shift, fallback list, cache -- as HAMILTONIAN.
 * ricadi_set_radi_shifts takes CYCLE and HAMILTONIAN and returns RICADI_EINVAL for every other value, as it did before
 * the third mode existed (callers and tests rely on that refusal); ricadi_set_radi_shift_mode (ABI 410) is the same
 * setting and takes all three, RICADI_EINVAL for another value.                                                      */
#define RICADI_RADI_SHIFTS_CYCLE 0
#define RICADI_RADI_SHIFTS_HAMILTONIAN 1
#define RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT 2
int ricadi_set_radi_shifts(ricadi_ctx* ctx, int mode);
int ricadi_set_radi_shift_mode(ricadi_ctx* ctx, int mode);
/* The shift of every step of the most recent ricadi_ric_radi(_dev) call of the context, in either mode: *n_out = steps
 * started (one more than the steps completed when the call ended by a breakdown); at most `cap` entries are copied to
 * `out` (may be NULL with cap = 0).  RICADI_ESTATE before any RADI call.                                             */
int ricadi_radi_shift_history(ricadi_ctx* ctx, double* out, int cap, int* n_out);
/* How many of those shifts were fallbacks to the caller's list (HAMILTONIAN mode; 0 in CYCLE mode).  RICADI_ESTATE
 * before any RADI call.  (Every slot of stats_out is taken, so these values have calls of their own.)               */
int ricadi_radi_shift_fallbacks(ricadi_ctx* ctx, int* n_out);
/* The reduced matrices of the shift selection on device operands, for tests:
 *   dH_out (k x (2k + m + 2nb), row-major) = Q^T [cal A Q | cal E Q | R | U | B]
 * with dQ NV x k (leading dimension k, any columns), dRU = [R | U] NV x (m + nb), dB NV x nb.  One pass over the rows of
 * cal A and cal E; every sum runs in a fixed order: the same call gives bitwise the same dH_out.
 * 1 <= k <= 32, 1 <= m <= 32, 1 <= nb <= 64 (the driver calls it with k = m).                                         */
int ricadi_radi_reduce_dev(ricadi_ctx* ctx, const double* dQ, int k, const double* dRU, int m, const double* dB,
                           int nb, double* dH_out);
/* The same for a wide block, on the kernel RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT uses above 32 columns: k = m,
 * 33 <= m <= 127, 1 <= nb <= 64; dH_out m x (3m + 2nb).  Bitwise the same on a second call.                          */
int ricadi_radi_reduce_wide_dev(ricadi_ctx* ctx, const double* dQ, int k, const double* dRU, int m, const double* dB,
                                int nb, double* dH_out);
/* Entries of the per-shift cache, summed over the levels of the preconditioner hierarchy, for tests.               */
int ricadi_probe_cache_entries(ricadi_ctx* ctx, int* n_out);
/* Branches of the RADI driver, for tests.
 * ricadi_probe_radi_refuse: under RICADI_RADI_SHIFTS_HAMILTONIAN the selection made after each of the n listed steps
 *   (1-based) counts as refused: it still runs and is recorded, and the step that follows takes the next entry of the
 *   caller's list.  The list stays in the context until it is replaced or cleared (n = 0; steps may then be NULL);
 *   empty by default.  RICADI_EINVAL for n < 0, n > 0 without steps, or a step below 1.
 * ricadi_probe_radi_counters, of the most recent ricadi_ric_radi(_dev) call: out[0] how often the block's CholQR2 raised
 *   its flag (normalised pivot below 1e-12) and the QR and the reduction were repeated with the Householder QR, out[1]
 *   how often the factor was recompressed inside the call.
 * ricadi_probe_radi_kept, of the most recent call: the size of the basis (columns of the block's Q kept) of every
 *   selection made, in order; *n_out their number, at most `cap` copied to `out` (may be NULL with cap = 0).
 * The last two return RICADI_ESTATE before any RADI call.                                                            */
int ricadi_probe_radi_refuse(ricadi_ctx* ctx, const int* steps, int n);
int ricadi_probe_radi_counters(ricadi_ctx* ctx, int* out);
int ricadi_probe_radi_kept(ricadi_ctx* ctx, int* out, int cap, int* n_out);
/* The dense part of ONE RADI step on device operands, for tests: dV (its first NV rows, leading dimension ldv >= m),
 * dB NV x nb, dRU = [R | U] NV x (m + nb) updated in place, the new block of Z written to columns [zoff, zoff + m)
 * of dZblk (leading dimension ldz >= zoff + m); dG_out m x nb; dC_out m x (2m + nb) (may be NULL):
 * [sqrt(-2p) L^-T | (-2p) Y^-1 | (-2p) Y^-1 G].  1 <= m <= 127, 1 <= nb <= 64, p < 0.  All sums run in a fixed
 * order: the same call gives bitwise the same outputs.  RICADI_EBREAKDOWN as above.                              */
int ricadi_radi_update_dev(ricadi_ctx* ctx, double p, const double* dV, int ldv, int m, const double* dB, int nb,
                           double* dRU, double* dZblk, int ldz, int zoff, double* dG_out, double* dC_out);
/* The SWEEP form of a1r (ABI 411): with RICADI_RADI_SHIFTS_CYCLE and a width G > 1, G consecutive
 * steps with pairwise distinct shifts p_1 .. p_G run as G solves against the SAME panel [R_0 | U_0] in ONE lockstep
 * batch (cal A_0 = cal A - U_0 B^T the closed loop at the start of the sweep),
 *   [[cal A_0 + p_g cal E, J^T], [J, 0]] [Vh_g; *] = [R_0; 0],   Vh = [Vh_1 .. Vh_G],   S = cal E Vh,   Gh = Vh^T B,
 *   M_gh = -(I + Gh_g Gh_h^T) / (p_g + p_h) = L L^T,   y = L^-1 (1_G (x) I),   h = L^-1 Gh,   T_j = L^-T[:, :j mw],
 *   Z <- [Z, Vh T_k],   R <- R_0 + S T_k y[:k mw],   U <- U_0 + S T_k h[:k mw],
 * which equals the G sequential steps block by block up to a rotation inside each block (Z Z^T, the gain and the
 * residual after every step are the same in exact arithmetic; G = 1 is the step above).  The residual after every
 * step of the sweep comes from ONE fetch of Gh and of the Gram matrix of [R_0 | S]; the sweep keeps k blocks, k the
 * first step whose residual is <= res_reltol, else as many as max_steps leaves, and drops the blocks behind it: steps,
 * history, stopping rule and ricadi_radi_shift_history mean what they mean at width 1, while the count of shift solves
 * (stats_out[4]) counts every solve issued and may exceed the steps by up to G - 1.
 * ricadi_set_radi_sweep_width: a context setting like ricadi_set_radi_shift_mode, default 1 (the sequential form,
 * bitwise as before); RICADI_EINVAL for width < 1 or > 16.  The width that runs is ricadi_host_radi_sweep_width's.
 * With width > 1 and a generated-shift mode ricadi_ric_radi(_dev) return RICADI_EINVAL before anything is launched
 * (unless ricadi_set_radi_sweep_shifts below is on).
 * ricadi_radi_sweep_info, of the most recent ricadi_ric_radi(_dev) call: out[0] the effective width, out[1] sweeps
 * run (0 at width 1), out[2] solves issued.  RICADI_ESTATE before any RADI call.                                  */
#define RICADI_RADI_SWEEP_PIVOT 1e-5       /* smallest relative Cauchy pivot of an admitted sweep   */
#define RICADI_RADI_SWEEP_MAX_K 128        /* G mw of a sweep                                                        */
int ricadi_set_radi_sweep_width(ricadi_ctx* ctx, int width);
int ricadi_radi_sweep_info(ricadi_ctx* ctx, int* out);
/* Sweeps whose shifts are GENERATED from the iteration (ABI 412): a context setting, default 0.
 * ricadi_set_radi_sweep_shifts(ctx, on) returns the previous value (0 / 1), RICADI_EINVAL (-1) for another `on`.
 * With it on, ricadi_ric_radi(_dev) require RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT (else RICADI_EINVAL before anything
 * is launched) and accept a sweep width above 1 with it.  At width 1 the call is the DOMINANT mode itself, bit for bit.
 * Above 1:
 *   cap      G = min(width, 128 / mw, 16 / column groups of the panel, max_steps); no halving.
 *   first    sweep: ONE step with shifts[0].
 *   basis    after a sweep that kept k blocks and did not end the iteration: Zg = the last min(k, 127 / mw) kept blocks
 *            (c <= 127 columns), Q Rq = Zg, S the dominant <= 32 left singular vectors of Rq (RICADI_RADI_RANK_TOL), the
 *            basis Q S; H = Q^T [cal A Q | cal E Q | R | U | B] is c x (2c + mw + 2nb).
 *   select   the candidates of the HAMILTONIAN rule on that basis, ALL of them, ordered by descending criterion (on an
 *            exact tie the larger |lambda| first); walking them in that order a candidate is admitted if it is finite
 *            and negative and the smallest Cauchy pivot prod_{k<j} ((p_j - p_k) / (p_j + p_k))^2 of the admitted list
 *            with it appended stays >= RICADI_RADI_SWEEP_PIVOT; up to min(G, steps left).  The next sweep solves the
 *            admitted shifts in acceptance order (it may be narrower than G).
 *   fallback a refused selection (RICADI_RADI_REFUSED_*, none admitted): the next sweep is ONE step with the next entry
 *            of the list (a counter of its own from shifts[1], cycling), counted in ricadi_radi_shift_fallbacks.
 * Two host synchronisations per sweep (the second is skipped when the sweep ended the iteration).  The cache holds
 * after the call what it held before plus the entries of the list that were used.  ricadi_probe_radi_refuse: a sweep
 * whose last kept step is listed counts as refused.  ricadi_probe_radi_kept: one entry per selection.
 * ricadi_radi_sweep_info: out[0] the cap G, out[1] sweeps, out[2] solves issued.
 * ricadi_radi_sweep_widths, of the most recent ricadi_ric_radi(_dev) call in a sweep form: the solves of every sweep in
 * order; *n_out their number (0 after a sequential call), at most `cap` copied to `out` (may be NULL with cap = 0).
 * RICADI_ESTATE before any RADI call.                                                                              */
int ricadi_set_radi_sweep_shifts(ricadi_ctx* ctx, int on);
int ricadi_radi_sweep_widths(ricadi_ctx* ctx, int* out, int cap, int* n_out);
/* The reduction for such a group on device operands, for tests: dH_out (c x (2c + m + 2nb)) with dQ NV x c; any
 * 1 <= c <= 127 with 1 <= m <= 127 (m <= 32 where c <= 32), 2c + m + 2nb <= 509.  c <= 32 and c = m run the kernels
 * of ricadi_radi_reduce_dev / _wide_dev (the same bits); 33 <= c, m != c the group form of the wide kernel: FP64
 * matrix cores, no atomics, a fixed summation order -- bitwise the same on a second call.                          */
int ricadi_radi_reduce_group_dev(ricadi_ctx* ctx, const double* dQ, int c, const double* dRU, int m, const double* dB,
                                 int nb, double* dH_out);
/* The recombination of a sweep on device operands, for tests: the G solution panels lie at dV + g vstride (their
 * first NV rows, leading dimension ldv >= m, the first m columns are used), dS = cal E Vh NV x G m, dCf the
 * coefficient matrix G m x (k m + m + nb) of ricadi_host_radi_sweep.  Writes columns [zoff, zoff + k m) of dZblk
 * (leading dimension ldz) = Vh Cf[:, :k m] and adds S Cf[:, k m:] into dRU = [R | U] NV x (m + nb).
 * 1 <= G <= 16, G m <= 128, 1 <= k <= G, 1 <= nb <= 64.  FP64 matrix cores, no atomics, every sum in ascending
 * order: the same call gives bitwise the same outputs.                                                            */
int ricadi_radi_sweep_combine_dev(ricadi_ctx* ctx, int G, const double* dV, int64_t vstride, int ldv, int m,
                                  const double* dS, const double* dCf, int k, int nb, double* dRU, double* dZblk,
                                  int ldz, int zoff);

/* ---- device-pointer level (multi-GPU orchestration, benchmarks) --------
 * Same operations on buffers that already live in HBM (e.g. torch tensors'
 * data_ptr()); nothing is copied to or from the host.                      */
int ricadi_spmm_dev(ricadi_ctx* ctx, double alpha, double beta,
                    const double* dX, int m, double* dY);
int ricadi_shift_solve_dev(ricadi_ctx* ctx, double alpha, double beta,
                           const double* dR, int m, double* dX,
                           int* iters_out, double* relres_out);
/* The shifts of one ADI sweep in ONE batched solve: for g < ng solve
 *   S(alphas[g], betas[g]) X_g = [R_g; 0]
 * with R_g = dR + g*r_stride (NV x m each; r_stride in doubles, 0 = the same
 * right-hand side for every shift, the shift-parallel sweep) and X_g =
 * dX + g*n*m (n x m each).  All groups advance in lockstep inside one launch
 * sequence (grid.z = groups still iterating), which fills the chip where a
 * single n ~ 3e4 panel cannot.  ng <= 16, ng*m <= 2048.  iters_out: ng ints,
 * relres_out: ng*m doubles (either may be NULL).  Returns RICADI_ENOCONV if a
 * group stopped at gmres_maxit.  Counterpart of the per-shift factorise-and-
 * solve work inside pru.solve_proj_lyap_stein / pru.proj_alg_ric_newtonadi (the package
 * body is not in /root/reference; call sites: /root/reference/solve_dae_ric.py:152-159,
 * /root/reference/optcont_main.py:488-492,
 * /root/reference/tests/test_units_compfacres_compress.py:62-64).                */
int ricadi_shift_solve_batch_dev(ricadi_ctx* ctx, int ng, const double* alphas,
                                 const double* betas, const double* dR,
                                 int64_t r_stride, int m, double* dX,
                                 int* iters_out, double* relres_out);
/* ---- saddle systems at COMPLEX shifts (exports added under ABI 412) ----------------------
 * alpha = ar + i ai with ar <= 0 and alpha != 0, beta real: RICADI_EINVAL for ar > 0, alpha = 0 or a value that is not
 * finite (the preconditioner has never been applied at a non-negative shift).  A complex panel of mc columns is a
 * row-major array of complex doubles (real part first): the same memory as a real row-major panel of 2 mc columns with
 * the real parts in the even columns.  1 <= mc <= 8; strides are counted in complex elements; all pointers but the
 * shifts and the *_out arrays are device pointers.  A low-rank term set on the context (ricadi_set_lowrank, q > 0) is
 * REFUSED with RICADI_EINVAL in this version: remove it first.  Every sum runs in a fixed order, no atomics: the same
 * call gives bitwise the same result.
 * ricadi_shift_solve_cplx_batch_dev:  S(alphas_re[g] + i alphas_im[g], betas[g]) X_g = [R_g; 0] for g < ng <= 16,
 *   R_g = dR + g r_stride (NV x mc; r_stride 0 = one right-hand side for all groups, else >= NV mc), X_g = dX + g n mc
 *   (n x mc).  Right-preconditioned flexible GMRES with complex inner products, all groups in lockstep, from zero, with
 *   the context's gmres_restart / gmres_tol / gmres_maxit; the preconditioner is the real cycle applied to the real and
 *   the imaginary part at the real proxy shift of ricadi_host_cplx_proxy.  iters_out[ng], relres_out[ng mc] (the true
 *   relative residuals, recomputed with the complex product) may be NULL.  RICADI_ENOCONV as the real entry.
 * ricadi_op_apply_cplx_batch_dev:  the product alone, y_g = S(alpha_g, beta_g) x_g, for tests; x_g = dX + g x_stride,
 *   y_g = dY + g y_stride (strides >= n mc); active / nactive as ricadi_op_apply_batch_dev; variant_out (may be NULL):
 *   1 the tiled form (operators with the multi-shift tiles), 2 the CSR form (every other operator).
 * ricadi_cplx_orth_dev:  one CGS2 step of the complex Arnoldi kernels, for tests: w_g = dW + g n mc (n x mc, n = NV +
 *   NP of the resident operator) against the nvec basis panels v_{j,g} = dV + j v_stride + g g_stride (1 <= nvec <= 400);
 *   dH + g (nvec + 1) mc receives (nvec + 1) x mc complex: the summed coefficients v_j^H w of the two passes, then the
 *   norm of what is left; w is overwritten by the unit vector (zero where nothing is left).
 * ricadi_host_cplx_proxy:  the proxy shift -2^round(log2 |alpha|) (host only, no context).                        */
int ricadi_shift_solve_cplx_batch_dev(ricadi_ctx* ctx, int ng, const double* alphas_re, const double* alphas_im,
                                      const double* betas, const double* dR, int64_t r_stride, int mc, double* dX,
                                      int* iters_out, double* relres_out);
int ricadi_op_apply_cplx_batch_dev(ricadi_ctx* ctx, int ng, const double* alphas_re, const double* alphas_im,
                                   const double* betas, const double* dX, int64_t x_stride, int mc,
                                   const int32_t* active, int nactive, double* dY, int64_t y_stride, int* variant_out);
int ricadi_cplx_orth_dev(ricadi_ctx* ctx, int ng, int mc, int nvec, const double* dV, int64_t v_stride,
                         int64_t g_stride, double* dW, double* dH);
int ricadi_host_cplx_proxy(double ar, double ai, double* alpha_pre_out);
/* Step probe of the complex cycle (tests; exports added under ABI 412): the units the restart cycle of
 * ricadi_shift_solve_cplx_batch_dev is made of, one call each, on the solver's own workspace and with the strides of
 * a solve of ng groups of mc complex columns -- without the preconditioner and the operator: the caller supplies
 * w = S P^-1 v_j.  Complex panels [ng][n][mc] (n = NV + NP) are device pointers; every call is synchronous.
 *   begin: sizes the workspace as a solve does, fills V, Hm, cs, sn, gv, y, scale, resid and hout with 0xFF bytes
 *          (what no later call writes reads back as NaN), computes the squared norms of the residual panels dR and
 *          runs the cycle start (gv[0], scale, resid, v_0 into V slot 0) for all ng groups.  bnorm: HOST array
 *          [ng][mc], ||b|| per column.
 *   step:  the Arnoldi phase of iteration j (0 <= j < gmres_restart) on the panels dW for the nact groups listed in
 *          `groups` (host; distinct ids in 0 .. ng-1): CGS2 against V[0 .. j] into V[j + 1], then column j of the
 *          Hessenberg matrix, its rotation, gv and resid.  The CGS2 step also leaves ||w'||^2 in nrm2 and 1 / ||w'||
 *          in scale.  The other groups are not touched.
 *   close: the cycle end for all groups, group g with its first ks[g] vectors (host; 0 <= ks[g] <= min(nz, steps run
 *          for g)): R y = g, then dX += Z y with the nz FP64 panels dZ [nz][ng][n][mc] (copied into the solver's Z
 *          storage) on the caller's panels dX [ng][n][mc].
 *   read:  one workspace array (RICADI_CPROBE_*) into dOut (capacity cap doubles; *count: doubles written), `slot`:
 *          the Krylov vector for RICADI_CPROBE_V, ignored otherwise.
 * RICADI_EINVAL before anything is launched for j, ng, mc, a group id, ks, nz, `what` or a slot out of range, and for
 * step / close / read without a begin on the current workspace (a complex solve, a ricadi_cplx_orth_dev call or a new
 * operator ends the probe cycle).  A later solve on the context is bitwise what it is on a fresh context.          */
#define RICADI_CPROBE_V 0      /* Krylov vector `slot`, [ng][n][mc] complex                                        */
#define RICADI_CPROBE_HOUT 1   /* coefficient column of the last CGS2 step, [ng][gmres_restart + 2][8] complex     */
#define RICADI_CPROBE_HM 2     /* [ng][8][gmres_restart][gmres_restart + 1] complex: column j of R, entries 0 .. j + 1 */
#define RICADI_CPROBE_CS 3     /* [ng][8][gmres_restart] real                                                      */
#define RICADI_CPROBE_SN 4     /* [ng][8][gmres_restart] complex                                                   */
#define RICADI_CPROBE_GV 5     /* [ng][8][gmres_restart + 1] complex                                               */
#define RICADI_CPROBE_Y 6      /* [ng][gmres_restart][8] complex                                                   */
#define RICADI_CPROBE_SCALE 7  /* [ng][16] real: the factor of a complex column in both slots of its pair          */
#define RICADI_CPROBE_RESID 8  /* [ng][8] real                                                                     */
#define RICADI_CPROBE_NRM2 9   /* [ng][16] real: squared norm of complex column c at 2 c, 0 at 2 c + 1             */
int ricadi_cplx_probe_begin_dev(ricadi_ctx* ctx, int ng, int mc, const double* dR, const double* bnorm);
int ricadi_cplx_probe_step_dev(ricadi_ctx* ctx, int j, const double* dW, int nact, const int* groups);
int ricadi_cplx_probe_close_dev(ricadi_ctx* ctx, const int* ks, int nz, const double* dZ, double* dX);
int ricadi_cplx_probe_read_dev(ricadi_ctx* ctx, int what, int slot, double* dOut, int64_t cap, int64_t* count);

/* dW (NV x m) += coef * E * dV (first NV rows of an n x m or NV x m panel) */
int ricadi_apply_e_dev(ricadi_ctx* ctx, double coef, const double* dV, int m, double* dW);
/* dOut (nrows x m) = sum_i coef[i] * panel_i, panel_i = dBasis + i*stride
 * (stride in doubles); coef is a host array.  Used by the shift-parallel
 * Cauchy recombination.                              */
int ricadi_lincomb_dev(ricadi_ctx* ctx, int nrows, int m, int nvec, const double* dBasis,
                       int64_t stride, const double* coef, double* dOut);
/* Cauchy recombination of one ADI sweep on the device:
 * dU holds the G solutions U_i (G x NV x m, contiguous, NV rows each); with
 * rinv = R^-1 (G x G row-major, C = R^T R) and cinv1 = C^-1 1 (host arrays from
 * ricadi_host_cauchy):  dZ (NV x G*m, row-major) = U (R^-1 (x) I_m),
 * dW (NV x m) += E U ((C^-1 1) (x) I_m),  *n2_out = ||dZ||_F^2.                */
int ricadi_sweep_recombine_dev(ricadi_ctx* ctx, int G, const double* dU, int m,
                               const double* rinv, const double* cinv1,
                               double* dZ, double* dW, double* n2_out);
/* The same with the solutions in an arbitrary order and with unused slots, as an all-gather
 * of per-rank blocks delivers them: dU holds nslot panels (nslot x NV x m, contiguous);
 * coefz (nslot x G, row-major) and coefw (nslot) are the rows of R^-1 and the entries of
 * C^-1 1 of the shift each slot carries (zero rows for padding slots and for slots that
 * belong to another column part):  dZ (NV x G*m) = sum_i coefz[i][:] (x) U_i,
 * dW (NV x m) += E sum_i coefw[i] U_i.  The data are consumed where the collective put
 * them; only the small coefficient table is permuted.  block_n2_out (G doubles, may be
 * NULL): squared Frobenius norm of every column block of dZ -- with coefz the rows of the
 * upper triangular R^-1 these are the blocks of the step-by-step iteration, which is what
 * the reference's stopping rule looks at.  Up to 16 slots and 16 blocks the blocks and
 * their norms come from the ADI driver's fused kernel (sums in a fixed order: the same
 * inputs give bitwise the same norms); wider calls are served block by block.          */
int ricadi_sweep_recombine_slots_dev(ricadi_ctx* ctx, int nslot, int G, const double* dU, int m,
                                     const double* coefz, const double* coefw,
                                     double* dZ, double* dW, double* n2_out, double* block_n2_out);
/* dK (NV x nb) = coef * E * (Z * (Z^T B)) for a device-resident factor dZ
 * (NV x c, row-major with leading dimension ldz) and dB (NV x nb).          */
int ricadi_gain_dev(ricadi_ctx* ctx, double coef, const double* dZ, int c, int ldz,
                    const double* dB, int nb, double* dK);
/* Frobenius norms of the m columns' Gram matrix: out = ||W^T W||_F, and the
 * squared F-norm of the panel in nrm2 (both may be NULL).                  */
int ricadi_panel_norms_dev(ricadi_ctx* ctx, const double* dW, int nrows, int m,
                           double* gram_fro, double* nrm2);
/* Average duration (ms) of the last timed kernel class, measured with HIP
 * events on the context stream: which = 0 SpMM.                            */
int ricadi_time_spmm_dev(ricadi_ctx* ctx, double alpha, double beta, const double* dX,
                         int m, double* dY, int reps, double* ms_per_launch);
/* The same for the batched launch of the hot path: ng panels (dX + g*n*m ->
 * dY + g*n*m), shift g = (alphas[g], betas[g]); one launch covers all of them. */
int ricadi_time_spmm_batch_dev(ricadi_ctx* ctx, int ng, const double* alphas,
                               const double* betas, const double* dX, int m,
                               double* dY, int reps, double* ms_per_launch);

/* One launch of a hot-path kernel class exactly as the batched GMRES issues it (ng groups,
 * panel width m, nvec Krylov vectors for the Arnoldi classes), on the solver's own
 * workspace buffers; average over `reps` launches, HIP events on the context stream.
 * Behind the per-kernel roofline objects of bench.py.  No reference counterpart.      */
#define RICADI_TK_SPMM 0          /* tile SpMM of the saddle operator                     */
#define RICADI_TK_BLOCK_V 1       /* block-Jacobi sweep, velocity blocks                  */
#define RICADI_TK_BLOCK_P 2       /* block-Jacobi sweep, Schur (pressure) blocks          */
#define RICADI_TK_COARSE 3        /* dense coarse apply                                   */
#define RICADI_TK_SPMM_SY 4       /* tile SpMM of the prolongated operator S*Y            */
#define RICADI_TK_DOTS 5          /* cols_dots + reduce_partials                          */
#define RICADI_TK_UPDATE_DOTS 6   /* cols_update_dots + reduce_partials                   */
#define RICADI_TK_UPDATE 7        /* cols_update (writes the new Krylov vector)           */
#define RICADI_TK_PRECOND 8       /* the whole preconditioner application (all launches)  */
#define RICADI_TK_RESTRICT 9      /* restriction Y^T r (CSR SpMM with unit values)        */
/* 10 + k: stage k of the preconditioner application ALONE, issued by the solver's own code path (so the
 * kernel and its template instance are the ones the iteration launches at this size):
 * 0 restriction, 1 coarse apply (dense inverse or child cycle), 2 pressure rows of r - (S Y) e,
 * 3 first velocity sweep (two-term block sweep with the coarse residual folded in), 4 J product,
 * 5 Schur-complement sweep, 6 last velocity sweep (rectangle sweep with prolongation)             */
#define RICADI_TK_PC_STAGE0 10
/* One hot lockstep GMRES iteration (preconditioner, operator, Arnoldi passes of iteration nvec - 1; no convergence
 * logic), averaged over `reps` iterations issued back to back: ITER all ng groups on the context stream, ITER_SPLIT
 * the even and the odd group ids as two half-batches on two streams, forked from the context stream before the
 * first iteration and joined back to it after the last (the solver's split, RICADI_SPLIT).  Result: wall time per
 * iteration from HIP events.                                                                                     */
#define RICADI_TK_ITER 17
#define RICADI_TK_ITER_SPLIT 18
/* The coloured Vanka sweep of the first child level that has one (ricadi_opts::child_smoother = 1): all its colours,
 * 2 launches each (residual of the child's operator, patch kernel), without the child's coarse correction.
 * RICADI_EHIP ("no coarse level with a Vanka sweep") where no level has one.                                                                  */
#define RICADI_TK_PC_VANKA 19
int ricadi_time_kernel_dev(ricadi_ctx* ctx, int which, int ng, const double* alphas,
                           const double* betas, int m, int nvec, int reps,
                           double* ms_per_launch);

/* Step probe of the lockstep GMRES (tests): the units the solver's restart cycle is made of, one call each, on the
 * solver's own workspace and with the batch, iteration form and kernel choice of a solve of ng groups of width m --
 * without the preconditioner and the operator: the caller supplies w = S P^-1 v_j.  All pointers are device
 * pointers unless noted; every call is synchronous.  Group-major panels [ng][n][m], n = NV + NP.
 *   begin: the cycle start (norms of the residual panels dR, g, scale, first Krylov vector into slot 0) for all ng
 *          groups; dBnorm [ng][m]: ||b|| per column, as the frozen-column rule reads it.  What no later call writes
 *          reads back as NaN.
 *   step:  the Arnoldi phase of iteration j (0 <= j < gmres_restart) on the panels dW, for the nact groups listed in
 *          `groups` (host; ids in 0 .. ng-1); the panels of the other groups are not touched.
 *   close: the cycle end for all groups, group g with its first ks[g] vectors (host; 0 <= ks[g] <= steps run for g):
 *          one-reduction form: completion of column ks[g] - 1; R y = g; dX += Z y with the nz FP32 slots
 *          dZ [nz][ng][n][m] (copied into the solver's Z storage).
 *   read:  a workspace array as FP64 into dOut (capacity cap doubles; *count: doubles written).  `slot`: Krylov
 *          vector for RICADI_PROBE_BASIS, ignored otherwise.
 * RICADI_EINVAL before anything is launched for j, ng, m, a group id or a slot out of range, and for step / close /
 * read without a begin on the current workspace.                                                                 */
#define RICADI_PROBE_BASIS 0    /* Krylov vector `slot`, [ng][n][m], converted from its stored type                */
#define RICADI_PROBE_W 1        /* the FP64 panel w, [ng][n][m]                                                    */
#define RICADI_PROBE_W32 2      /* the FP32 panel w                                                                */
#define RICADI_PROBE_VCUR 3     /* FP64 copy of the newest Krylov vector (FP16 / FP32 basis)                       */
#define RICADI_PROBE_H1 4       /* first-pass coefficients, [ng][gmres_restart + 2][m]                             */
#define RICADI_PROBE_H2 5       /* second pass; row j + 1: ||w'||^2                                                */
#define RICADI_PROBE_HSUM 6     /* h1 + h2 as the separate Hessenberg kernel leaves it for an update from w        */
#define RICADI_PROBE_H 7        /* [ng][m][gmres_restart][gmres_restart + 1]: column j of R, entries 0 .. j + 1    */
#define RICADI_PROBE_CS 8       /* [ng][m][gmres_restart]                                                          */
#define RICADI_PROBE_SN 9
#define RICADI_PROBE_G 10       /* [ng][m][gmres_restart + 1]                                                      */
#define RICADI_PROBE_SCALE 11   /* [ng][m]                                                                         */
#define RICADI_PROBE_RESID0 12  /* residual estimates, buffer 0 and 1, [ng][m] each                                */
#define RICADI_PROBE_RESID1 13
#define RICADI_PROBE_Y 14       /* [ng][gmres_restart][m]                                                          */
#define RICADI_PROBE_NRM2 15    /* squared norms of the cycle start, [ng][m]                                       */
#define RICADI_PROBE_LS_COEF 16 /* one-reduction form, per group: sums [gmres_restart + 2][s|t][16], then two pending
                                 * columns of gmres_restart + 3 rows of 16 (p, rho, g before the rotation)          */
#define RICADI_PROBE_FORM 17    /* 8 values 0 / 1: FP16 basis, FP32 basis, preconditioner reads FP16, w kept, fused
                                 * Hessenberg, FP32 operator input, FP32 panel w, one-reduction form               */
int ricadi_arnoldi_probe_begin_dev(ricadi_ctx* ctx, int ng, const double* alphas, const double* betas, int m,
                                   const double* dR, const double* dBnorm);
int ricadi_arnoldi_probe_step_dev(ricadi_ctx* ctx, int j, const double* dW, int nact, const int* groups);
int ricadi_arnoldi_probe_close_dev(ricadi_ctx* ctx, const int* ks, int nz, const float* dZ, double* dX);
int ricadi_arnoldi_probe_read_dev(ricadi_ctx* ctx, int what, int slot, double* dOut, int64_t cap,
                                  int64_t* count);

/* K5: thin QR factorisation Z = Q R of an NV x c host matrix (c <= NV) by block
 * Gram-Schmidt with re-orthogonalisation over 32-column panels, each panel
 * factorised by a Householder TSQR tree.  R_out: c x c row-major upper triangular;
 * Q_out: NV x c or NULL.  The "QR" of the reference's compress_Zsvd comment
 * (/root/reference/optcont_main.py:133-134) and of the Newton update norm.      */
int ricadi_qr(ricadi_ctx* ctx, const double* Z, int c, double* Q_out, double* R_out);

/* The Newton-Kleinman loop's update norm, called as the loop calls it (ABI 413, for tests):
 *   *upd_out = ||Z1 Z1^T - Z0 Z0^T||_F,   *x1_out = ||Z1 Z1^T||_F
 * from R of the block QR of [Z1, Z0] (no panel of which holds columns of both factors) as ||R S R^T||_F,
 * S = diag(I_k1, -I_k0) -- the Gram matrices of the factors are never formed, so an update 1e-10 below x1 keeps
 * about four digits.  dZ1 NV x k1 and dZ0 NV x k0 are DEVICE panels, row-major with leading dimension = width and
 * only read; dZ0 may be NULL with k0 = 0; either output may be NULL.  k1 + k0 may exceed NV (two full-rank iterates
 * of a small operator): the NV x NV matrix [Z1, Z0] S [Z1, Z0]^T is then the smaller one and is formed as it stands,
 * to the same accuracy -- block Gram-Schmidt has nothing left to orthogonalise against once the columns have used up
 * the NV dimensions.
 * A dimension-only context (ricadi_set_dims) is enough.
 * Width limit: k1 + k0 <= RICADI_MAX_UPD_COLS.  The block QR itself has no fixed bound -- its kernels walk the
 * columns in panels of at most 128 and their grids grow with the width in 32- or 64-column tiles, far below the
 * grid limits; the scratch pool serves any size the device can allocate -- so the bound is the workspace: five
 * (k1 + k0)^2 arrays of doubles (R, its two transposes and the product on the device, the product again on the
 * host), 0.67 GB at 4096 columns, beside two NV x (k1 + k0) panels.
 * RICADI_EINVAL before anything is launched, outputs untouched: k1 < 1, k0 < 0, a NULL panel with a positive width,
 * k1 + k0 above the limit.  RICADI_ESTATE on a context without dimensions.                                        */
#define RICADI_MAX_UPD_COLS 4096
int ricadi_diff_zzt_fnorm_dev(ricadi_ctx* ctx, const double* dZ1, int k1, const double* dZ0, int k0,
                              double* upd_out, double* x1_out);

/* K7: the pencil of the operator projected onto a dense basis (the Ritz values behind ms='auto'):
 * HA = Q^T (cal A - U V^T) Q,  HE = Q^T cal E Q  (k x k row-major; the low-rank term if one is set).
 * Q: NV x k row-major, 1 <= k <= 128, any columns (orthonormal ones for Ritz values).  One pass over the
 * velocity rows of the operator; per-workgroup partials summed in a fixed order, so the same inputs give
 * bitwise the same HA / HE.  Host buffers; the _dev form takes device pointers.  No reference counterpart. */
int ricadi_project_pencil(ricadi_ctx* ctx, const double* Q, int k, double* HA, double* HE);
int ricadi_project_pencil_dev(ricadi_ctx* ctx, const double* dQ, int k, double* dHA, double* dHE);

/* ---- balanced truncation from two low-rank factors (exports added under ABI 412) ----
 * ricadi_cross_gram_dev: G = X^T Y (p x q row-major, leading dimension q) of two row-major DEVICE panels, X n x p with
 *   leading dimension ldx >= p, Y n x q with ldy >= q, 1 <= p, q <= 1024; dG a device buffer of p q doubles.  A 32 x 32
 *   tile per wave on the FP64 matrix cores, row slices summed in a fixed order and no atomics: the same inputs give
 *   bitwise the same G.  Needs a context, not an operator.
 * ricadi_project_pencil_twosided_dev: the Petrov-Galerkin form of K7,
 *   HA = L^T (cal A - U V^T) Rb,  HE = L^T cal E Rb  (r x r row-major),
 *   for a left basis L and a right basis Rb (NV x r row-major device panels, 1 <= r <= 128): one pass over the velocity
 *   rows of the operator, rows gathered from Rb and multiplied by the workgroup's own rows of L; partials summed in
 *   workgroup order, bitwise reproducible.  With L = Rb = Q it is ricadi_project_pencil_dev's pencil.
 * ricadi_lqg_balance_dev: square-root balancing of two factors on the RESIDENT operator, which must be set in the
 *   orientation cal A = A, cal E = M of the system M v' = A v + J^T p + B u, y = C v -- the one the filter equation's
 *   solve (transposed=True) leaves resident.  dZc (NV x kc, X = Zc Zc^T the regulator / observability factor) and dZf
 *   (NV x kf, Y = Zf Zf^T the filter / reachability factor), dB (NV x nb) and dCt = C^T (NV x nc) are device panels with
 *   leading dimension = width, 1 <= kc, kf, nb, nc <= 1024.  S = Zc^T cal E Zf = U Sigma V^T (host Jacobi SVD),
 *   r = #{sigma_i > tol sigma_1} capped by order (order <= 0: no cap), by 128, kc, kf and NV; 0 <= tol < 1.
 *   T_l = Zc U_r Sigma_r^-1/2 -> dTl, T_r = Zf V_r Sigma_r^-1/2 -> dTr (device, NV x r, leading dimension r; buffers of
 *   NV rcap doubles, rcap the cap above), so that T_l^T cal E T_r = I_r;  *r_out = r;  sigma_out (host, min(kc, kf)
 *   doubles): all singular values, descending -- the LQG characteristic values when the factors solve the two Riccati
 *   equations, the Hankel singular values when they solve the two Lyapunov equations.  Host outputs, row-major with the
 *   leading dimension of their width:  Ar_out = T_l^T cal A T_r and Er_out = T_l^T cal E T_r (r x r; buffers rcap^2),
 *   Br_out = T_l^T B (r x nb; rcap nb), Cr_out = C T_r (nc x r; nc rcap).  A low-rank term of the context is part of
 *   cal A (at most 1024 columns).  RICADI_EHIP with a message when S is zero or not finite or its SVD did not converge.
 * ricadi_host_lqg_balance: the host step alone (no GPU, no context): S kc x kf row-major; outputs r, sigma_out
 *   (min(kc, kf)), coefl_out = U_r Sigma_r^-1/2 (kc x r) and coefr_out = V_r Sigma_r^-1/2 (kf x r), leading dimension r,
 *   in buffers of kc (kf) times min(kc, kf, order) doubles: coefl^T S coefr = I_r.  RICADI_EINVAL for a bad argument or
 *   an entry of S that is not finite, RICADI_EBREAKDOWN for S = 0, RICADI_ENOCONV if the Jacobi iteration has not
 *   converged in its 60 sweeps (nothing is written then).                                                   */
int ricadi_cross_gram_dev(ricadi_ctx* ctx, int n, int p, int q, const double* dX, int ldx, const double* dY, int ldy,
                          double* dG);
int ricadi_project_pencil_twosided_dev(ricadi_ctx* ctx, const double* dL, const double* dRb, int r, double* dHA,
                                       double* dHE);
int ricadi_lqg_balance_dev(ricadi_ctx* ctx, const double* dZc, int kc, const double* dZf, int kf, const double* dB,
                           int nb, const double* dCt, int nc, double tol, int order, int* r_out, double* sigma_out,
                           double* dTl, double* dTr, double* Ar_out, double* Er_out, double* Br_out, double* Cr_out);
int ricadi_host_lqg_balance(int kc, int kf, const double* S, double tol, int order, int* r_out, double* sigma_out,
                            double* coefl_out, double* coefr_out);

/* Structure of the preconditioner the context built for its operator:
 * out = [NV, NP, velocity blocks, Schur blocks, block size, coarse dimension,
 *        SpMM row blocks, max distinct columns per row block,
 *        preconditioner levels in use, dimension of the dense inverse on the last level,
 *        1 if the GMRES iteration hands the preconditioner the FP16-stored vector,
 *        padded width of the dense rectangles of the last velocity sweep (0: not in that form),
 *        the same for the first (two-term) velocity sweep, NP, nnz(J), nnz(S*Y)];
 *        entries of the restriction,
 *        route the last batch of dense coarse inverses took (0 block Gauss-Jordan without pivoting, 1 rocSOLVER
 *        with partial pivoting; -1 none yet),
 *        kernel of the last saddle SpMM launch (0 CSR, 1 LDS-tiled per group, 2 LDS-tiled multi-shift; +4 with
 *        FP32 x input; -1 none yet),
 *        1 if the last preconditioner application kept the velocity part between its sweeps as an FP32 panel
 *        (first sweep -> pressure step -> last sweep), 0 for an FP64 panel; -1 none yet,
 *        1 if the operator launch of the last iteration (or timing call) wrote w = S z as an FP32 panel for the
 *        Arnoldi passes, 0 for FP64; -1 none yet,
 *        [21] 1 if a child level smooths with the coloured Vanka sweep (0: SIMPLE sweep or no child level), and of
 *        the first such level [22] its colours (the lone colour included), [23] its patches (one per pressure unknown of the
 *        level), [24] its largest patch, [25] the entries of J the size cap of 64 unknowns dropped, [26] its lone
 *        pseudo-patches,
 *        [27] ricadi_opts::hierarchy in force, [28] the levels of the hierarchy as ricadi_host_plan_hierarchy counts
 *        them (grids with a sweep of their own: entry 8 counts the dense coarse problem as one level more), [29] the
 *        dimension of the dense inverse of the last level (entry 9 again; 0 without a coarse space)];
 * nout >= 8; entries beyond nout are not written.                                   */
int ricadi_setup_info(ricadi_ctx* ctx, int* out, int nout);

/* In-place inverses of nb dense k x k matrices (row major, back to back in A, host memory) by the routine the
 * setup uses for the coarse matrices of a batch of shifts: block Gauss-Jordan without pivoting, and -- when a
 * pivot vanishes relative to the scale of its diagonal block -- rocSOLVER's getrf / getri with partial
 * pivoting for the whole batch.  *route_out: the route that finished (as in ricadi_setup_info).  Exported for
 * tests (the production operators never leave route 0).  No reference counterpart (its LU is SuperLU's). */
int ricadi_dense_inverse_batch(ricadi_ctx* ctx, int k, int nb, double* A, int* route_out);

/* Average duration (ms) of the thin QR of a device-resident NV x c factor (the device
 * part of ricadi_qr: Householder TSQR panels inside a block Gram-Schmidt on the MFMA
 * GEMMs), HIP events on the context stream: the TSQR MFMA-utilisation figure.          */
int ricadi_time_qr_dev(ricadi_ctx* ctx, const double* dZ, int c, int reps, double* ms_per_call);

/* Average duration (ms) of the FP64-MFMA Gram kernel G = Z^T Z (the 2*NV*c^2 flop
 * part of ricadi_compress) for a device-resident NV x c factor, HIP events on the
 * context stream.  dG must hold c*c doubles.                                   */
int ricadi_time_gram_dev(ricadi_ctx* ctx, const double* dZ, int c, double* dG, int reps,
                         double* ms_per_launch);

/* ---- recycling of solved right-hand sides -------------------------------
 * depth > 0: every batched solve whose groups share ONE right-hand side panel (the sweeps
 * of the ADI) starts from the least-squares combination of the last `depth` panels it has
 * already solved for the same shifts -- x0_g = sum_e Y_{g,e} C_e with C = argmin ||b - B C||_F
 * over the stored right-hand sides B -- instead of from zero, and stores its own (b, y_g)
 * afterwards.  The residual factors of consecutive ADI sweeps span nearly the same space
 * (cfg2: ||b - B C|| / ||b|| = 5e-2 ... 7e-4 per column from the fourth sweep on), which
 * saves that many digits of every later solve; the tolerance stays relative to ||b||.
 * The ADI / Newton drivers switch it on for their own sweeps (depth 5, 3 beyond n = 2e5;
 * RICADI_RECYCLE=d overrides, 0 = off); this call sets the depth for direct ricadi_shift_solve*_dev calls
 * (default 0, so that repeated identical solves measure what they seem to measure).
 * ricadi_clear_cache() drops the stored panels.  No reference counterpart (SuperLU is direct). */
int ricadi_set_recycle(ricadi_ctx* ctx, int depth);

/* Test hook: the recycled initial guess a batched solve of these ng shifts with the shared right-hand side dR
 * (NV x m, device) would start from, and nothing else -- no solve, nothing stored.  dX: ng panels of n x m (device);
 * they receive the guesses, or stay untouched with *rank_out = 0 where there is no guess (depth 0, no stored panel
 * common to all shifts, Gram matrix of rank 0).  *rank_out: numerical rank of the stored columns' Gram matrix.
 * Of the counters of ricadi_solve_trace it moves the guess_* ones only.                                          */
int ricadi_recycle_guess_dev(ricadi_ctx* ctx, int ng, const double* alphas, const double* betas, const double* dR,
                             int m, double* dX, int* rank_out);

/* ---- trace of the branches the batched shift solve took (tests) ----------
 * Host counters of the context, bumped where the decision is taken; no kernel, launch or synchronisation depends
 * on them.  Copies min(nout, RICADI_TRACE_SLOTS) values into out and returns RICADI_OK.  All are cumulative over
 * the context's life (take differences), except the *_last / guess_{cols,rank,pan} slots -- values of the most recent
 * event -- and cycle_len_max, the largest so far.  Slots:
 *    0 solves           calls of the batched solve (every ricadi_shift_solve* call, every sweep of the drivers)
 *    1 guess_tried      a recycled guess was asked for          2 guess_used   ... and used
 *    3 guess_cols       stored columns the last guess combined  4 guess_rank   rank of their Gram matrix
 *    5 guess_pan        1: normal equations from the side-by-side panel, 0: pair by pair
 *    6 stored           right-hand side / solution pairs stored
 *    7 smw_solves       solves by Sherman-Morrison-Woodbury     8 smw_setups   ... that built W for some shift
 *    9 smw_dup          ... with S^-1 U taken from the right-hand side's own columns (Newton driver)
 *   10 smw_bad          capacitance matrix not inverted or plain solve unconverged
 *   11 smw_refined      closed-loop residual above the tolerance: one more GMRES on the closed-loop operator
 *   12 inop_lowrank     solves with the low-rank term inside the Krylov operator (RICADI_SMW=0, m + q > 128)
 *   13 esc1_groups, 14 esc2_groups    groups continued at storage level 1 / 2
 *   15 wide_passes, 16 wide_chunks, 17 wide_groups_last   wide panels as sixteen-column groups: passes, lockstep
 *                       batches, column groups of the last batch
 *   18 cycles           restart cycles started                 19 cycle_len_last, 20 cycle_len_max   their length
 *   21 stalled_groups   groups given up for stagnation         22 maxit_groups   groups stopped at gmres_maxit     */
#define RICADI_TRACE_SLOTS 23
int ricadi_solve_trace(ricadi_ctx* ctx, int64_t* out, int nout);

/* ---- shift-parallel sweeps across processes (one process per GPU) -------
 * The ADI sweeps of ricadi_lyap_adi / ricadi_ric_newtonadi (sweep_width > 1) shard by shift:
 * every rank owns a fixed subset of the shift list (ricadi_host_deal), sets up and solves only
 * its own shifts of a sweep in one batched solve, and the solution panels are exchanged by ONE
 * all-gather per sweep; recombination, recompression, update norm and gain are replicated.  The
 * stopping decisions inside a sweep are taken by every rank on its own from the gathered panels (the
 * block norms are summed in a fixed order, so the ranks see the same bits); a rank whose own setup or
 * solves fail still takes part in the all-gather with a status word set, and all ranks return the error
 * together.  Two transports: RCCL inside the library (ricadi_set_exchange_rccl, below), or -- this call --
 * a collective the host supplies as a callback on two device buffers it owns (the Python binding uses it
 * for gloo groups: CPU tests and the one-GPU rehearsal):
 *   fn(user, send_dev, recv_dev, bytes_per_rank) must place rank r's first bytes_per_rank bytes
 *   of send_dev at recv_dev + r * bytes_per_rank on EVERY rank and return 0 once the data are
 *   visible to work enqueued afterwards on any stream (the library has synchronised its own
 *   stream before the call).
 * send_dev holds send_capacity bytes, recv_dev world * send_capacity; the last 4096 bytes of send_dev
 * (and the last world * 4096 of recv_dev) carry the small control messages, so fn is also called with
 * pointers INSIDE the two buffers and must honour them.  world = 1 (or fn NULL) removes the exchange.  All ranks must make the same sequence of solver calls with the same
 * arguments.  SURVEY.md section 8e; the reference has nothing distributed
 * (/root/reference/solve_dae_ric.py:122 and optcont_main.py:577 are sequential loops).      */
typedef int (*ricadi_allgather_fn)(void* user, const void* send_dev, void* recv_dev,
                                   int64_t bytes_per_rank);
int ricadi_set_exchange(ricadi_ctx* ctx, int rank, int world, ricadi_allgather_fn fn, void* user,
                        void* send_dev, void* recv_dev, int64_t send_capacity);

/* The same sharding with the collective INSIDE the library: RCCL's ncclAllGather (double, count = n * m per
 * solution panel and rank) enqueued on the context's stream between the solves and the recombination -- no host
 * synchronisation, no callback (section 5: the blocks exchanged are the V_i of
 * /root/reference/solve_dae_ric.py:152-159, the reference itself has nothing distributed).
 *   ricadi_rccl_unique_id: 128 bytes from ncclGetUniqueId; rank 0 calls it and hands the bytes to the other
 *     ranks by whatever means the host has (the Python binding: torch.distributed.broadcast_object_list).
 *   ricadi_set_exchange_rccl: joins the communicator of `world` ranks identified by unique_id
 *     (ncclCommInitRank, collective over the ranks; destroyed with the context) -- or, with comm != NULL, uses an
 *     ncclComm_t the caller created (not destroyed by the library).  The library allocates its own send buffer
 *     of send_capacity bytes and receive buffer of world * send_capacity bytes (capacity needed:
 *     max panels per rank and sweep * n * m * 8 + 4096).  world = 1 is allowed and still runs the exchange
 *     path (one rank: the transport test).  unique_id = comm = NULL on a context that already holds a
 *     communicator of the same rank / world keeps it and only re-sizes the buffers.
 *     Replaces a callback set by ricadi_set_exchange and vice versa;
 *     ricadi_set_exchange(ctx, 0, 1, NULL, ...) removes either.
 *   ricadi_exchange_count: collectives the context has issued so far, control messages included (a sweep
 *     costs exactly one; a Newton step one more for the update-norm decision, an ADI call one for statistics). */
int ricadi_rccl_unique_id(void* id_out, int bytes);
int ricadi_set_exchange_rccl(ricadi_ctx* ctx, int rank, int world, const void* unique_id, void* comm,
                             int64_t send_capacity);
int ricadi_exchange_count(ricadi_ctx* ctx, int64_t* count_out);

/* ---- host-side logic exported for CPU tests ---------------------------- */
/* Owner rank of every entry of an ADI shift list under `world` ranks: longest-processing-time
 * dealing on the lockstep cost model  T(rank) = a max_g it_g + b sum_g it_g  (a / b = 3.2: the
 * latency floor and the per-group slope of one lockstep iteration) with
 * predicted iteration counts it(p) that fall with |p| (the small shifts are the slow solves).
 * Deterministic in (shifts, world): every rank computes the same table.  Returns 0 or <0.   */
int ricadi_host_deal(const double* shifts, int nshifts, int world, int32_t* owner_out);
/* Whether the setup smooths the velocity aggregates of the two-level preconditioner for the operator cal A (CSR,
 * NV x NV):  *on_out = 1 iff the row sums of sym(cal A) stay below 0.15 of its diagonal (stiffness-like, not
 * mass-like) and sum |skew part| / sum |off-diagonal symmetric part| <= 0.7 (not convection dominated).  The two
 * ratios are returned (skew ratio -1 when the first test failed).  Host only; no GPU needed.                       */
int ricadi_host_sa_criterion(int nv, const int32_t* a_rowptr, const int32_t* a_col, const double* a_val,
                             double* rowsum_ratio_out, double* skew_ratio_out, int* on_out);
/* The preconditioner hierarchy ricadi_set_operator would choose for (cal A, cal E, J) with these options, computed on
 * the host (before the device-side fallbacks):  out[5] = { levels (1: block-Jacobi only, 2: dense coarse inverse,
 * 3: child level), coarse dimension k, its velocity / pressure parts, smoothed prolongation (0/1) }.  A stiffness-
 * dominated operator (ricadi_host_sa_criterion) keeps two levels up to k <= 1.5 coarse_max and grows its aggregates
 * up to (121, 182) for it; any other goes to a child level as soon as the gentle child fits coarse_max.             */
int ricadi_host_plan_levels(int nv, int np, const int32_t* a_rowptr, const int32_t* a_col, const double* a_val,
                            const int32_t* e_rowptr, const int32_t* e_col, const double* e_val,
                            const int32_t* j_rowptr, const int32_t* j_col, const double* j_val,
                            const ricadi_opts* opts, int32_t* out);
/* The whole hierarchy ricadi_set_operator would build for (cal A, cal E, J) with these options, level by level, on the
 * host: the same rule and the same child options as the setup, with the switch RICADI_SA at its default.  A level is
 * a grid with a sweep of its own; level l + 1 works on the aggregates of level l (plain aggregation, Galerkin
 * matrices), the last level inverts its coarse matrix densely.  *nlevels_out = number of levels (at most
 * RICADI_MAX_HIERARCHY_LEVELS; ricadi_host_plan_levels' out[0] counts the dense coarse problem as one more where
 * there is a coarse space).  levels_out: 8 entries per level, RICADI_MAX_HIERARCHY_LEVELS * 8 in all,
 *   [nv, np, kv, kp, agg_v, agg_p, has_child, dense_dim]
 * -- the level's size, its velocity / pressure aggregates, the aggregate sizes it ended with (the caller's on level 0
 * under hierarchy = 1; (2, 1) on a child unless it is the last level and had to grow them), whether its coarse problem
 * goes to a child, and kv + kp where it is inverted densely (0 on every level with a child).  smoothed_out (may be
 * NULL): per level 1 where its prolongation is smoothed.  Deterministic; no GPU needed.                             */
int ricadi_host_plan_hierarchy(int nv, int np, const int32_t* a_rowptr, const int32_t* a_col, const double* a_val,
                               const int32_t* e_rowptr, const int32_t* e_col, const double* e_val,
                               const int32_t* j_rowptr, const int32_t* j_col, const double* j_val,
                               const ricadi_opts* opts, int32_t* nlevels_out, int32_t* levels_out,
                               int32_t* smoothed_out);
/* The row-block tile format of the saddle SpMM that ricadi_set_operator would build (host only), for tests.
 * sizes_out[8] = [n, nblk, max_cols, max_nnz, nnz(S), tiles usable, multi-shift form built, nv].  Call with
 * the arrays NULL for the sizes, then again with rows2[nblk*32] (global row per local row, -1 = none),
 * rp2[nblk*33] (entry range per local row, in tile order), cols2[nblk*max(max_cols,1)] (global column per tile
 * slot, -1 = none), lidx[nnz] (tile slot per entry), perm[nnz] (index of the entry in the saddle CSR), the
 * saddle CSR s_rp[n+1], s_ci[nnz] and its value sources s_src[3*nnz] (cal A, cal E, J / J^T parts, one array
 * after the other); with the multi-shift form also lidx_ms[nnz] (tile slot | 0x8000 for velocity-velocity
 * entries), vAJ[nnz] (cal A + J part) and vE[nnz] (cal E part), in tile order.  Any array may be NULL.  */
int ricadi_host_saddle_tiles(int nv, int np, const int32_t* a_rowptr, const int32_t* a_col, const double* a_val,
                             const int32_t* e_rowptr, const int32_t* e_col, const double* e_val,
                             const int32_t* j_rowptr, const int32_t* j_col, const double* j_val,
                             const ricadi_opts* opts, int32_t* sizes_out, int32_t* rows2, int32_t* rp2,
                             int32_t* cols2, uint16_t* lidx, uint16_t* lidx_ms, double* vAJ, double* vE,
                             int32_t* perm, int32_t* s_rp, int32_t* s_ci, double* s_src);
/* The patches and colours of the coloured Vanka sweep for a level with nv velocity and np pressure unknowns, from
 * its J (CSR, np x nv) alone; host only, deterministic.  One patch per pressure unknown i: the velocity unknowns
 * with a stored entry in row i of J (ascending), then nv + i.  A record is 64 int32, -1 padded; a row with more
 * than 63 entries keeps the 63 of largest |J_iv| (ties: the lower index) and the rest are counted as dropped.
 * Colours: first fit in patch order; two patches share a colour only if they share no unknown.  Velocity
 * unknowns in no patch ("lone") are packed in ascending order, 64 at a time, into pseudo-patches that form one
 * last colour; the sweep applies the diagonal of the velocity block to them.  Patches are listed colour by
 * colour, inside a colour by pressure unknown.
 * sizes_out[8] = [colours (the lone colour included), patches (pseudo-patches included), pressure patches (= np),
 * largest patch (unknowns), entries of J dropped by the size cap, lone velocity unknowns, lone pseudo-patches,
 * 0].  Call with the arrays NULL for the sizes, then again with colour_ptr[colours + 1] (first patch of every
 * colour) and patch_idx[64 * patches]; either may be NULL.                                                       */
int ricadi_host_vanka_patches(int nv, int np, const int32_t* j_rowptr, const int32_t* j_col, const double* j_val,
                              int32_t* sizes_out, int32_t* colour_ptr, int32_t* patch_idx);
/* Greedy BFS aggregation of the graph of a CSR pattern into blocks of at
 * most bsize rows; blk_out[n]; returns the number of blocks (or <0).        */
int ricadi_host_aggregate(int n, const int32_t* rowptr, const int32_t* col,
                          int bsize, int32_t* blk_out);
/* Cauchy recombination data for a sweep of g distinct real negative shifts
 * (SURVEY.md section 8e):  C_ij = -1/(p_i+p_j) = R^T R (upper R);
 * rinv_out = R^-1 (g x g row-major), cinv1_out = C^-1 * ones (g), both in closed form (partial
 * fractions of the ADI steps' rational functions: accurate to a few ulp per entry whatever the
 * condition of C).  RICADI_EBREAKDOWN for repeated shifts and for sweeps whose recombination would
 * amplify the solves' errors by more than ~1e5 (smallest relative pivot of C below 1e-6: shifts too
 * many / too close); the drivers then halve the sweep width.                                    */
int ricadi_host_cauchy(const double* shifts, int g, double* rinv_out, double* cinv1_out);
/* The width the sweep form of ricadi_lyap_adi runs for a window of its shift cycle that is not one of the aligned
 * full sweeps (a sweep cut by the stopping prediction, and every sweep behind such a cut): the window is the g
 * entries first .. first + g - 1 of the cycled list of ns shifts, and *width_out is g halved until ricadi_host_cauchy
 * takes the leading *width_out of them -- one shift is always taken, so the iteration goes on with a narrower sweep
 * where the window's Cauchy matrix is refused.  Host only, no GPU needed; export added under ABI 412.
 * RICADI_EINVAL unless first >= 0, 1 <= g <= min(ns, 16) and every shift is negative.                              */
int ricadi_host_adi_window_width(const double* shifts, int ns, int first, int g, int* width_out);
/* The next RADI shift under RICADI_RADI_SHIFTS_HAMILTONIAN from the reduced matrices
 * H = Q^T [cal A Q | cal E Q | R | U | B] (k x (2k + m + 2nb), row-major; ricadi_radi_reduce_dev), by the rule stated
 * at ricadi_set_radi_shifts.  Host only, no GPU needed.  The library links no LAPACK: the eigenvalues of the real
 * 2k x 2k matrix Ham come from a balancing by powers of two, a Householder reduction to Hessenberg form and the
 * double-shift QR iteration; the eigenvector of a candidate is the null vector of Ham - lambda I by complex Gaussian
 * elimination with complete pivoting.  *p_out: the shift (negative), or 0 when Ham has no eigenvalue with negative real
 * part.  *margin_out (may be NULL): the largest criterion value over the second largest, +inf with one candidate.
 * RICADI_EINVAL unless 1 <= k <= 32, 1 <= m <= 32, 1 <= nb <= 64; RICADI_EBREAKDOWN when H_E is singular (LU pivot
 * below 1e-14 of its largest entry), H holds a value that is not finite, or the QR iteration does not converge.       */
int ricadi_host_radi_shift(int k, int m, int nb, const double* H, double* p_out, double* margin_out);
/* The same, and all 2k eigenvalues of Ham (real and imaginary parts, in no particular order), for tests.             */
int ricadi_host_radi_shift_eigs(int k, int m, int nb, const double* H, double* p_out, double* margin_out,
                                double* wr_out, double* wi_out);
/* What the RADI driver does with what a step has fetched: H = Q^T [cal A Q | cal E Q | R | U | B] for ALL m columns of
 * the block's Q (m x (3m + 2nb), row-major) and R of the block's QR (m x m, row-major).  The basis of the selection is
 * the columns i of Q with |R_ii| >= RICADI_RADI_RANK_TOL max_j |R_jj|; H is restricted to their rows, and to their columns in its
 * first two blocks, and handed to ricadi_host_radi_shift.  (The QR is unpivoted: the kept columns of Q span the block's
 * range when the dependent columns come last, as in a W = [independent | combinations])  Host only,
 * no GPU needed.  *kept_out (may be NULL): the
 * size of the basis (0 where R itself is refused).  Returns 0 with *p_out (negative) and *margin_out (may be NULL)
 * set, or -- not an error, the driver then takes the next entry of the caller's list and the outputs but *kept_out
 * are left alone -- one of the values below.  RICADI_EINVAL unless 1 <= m <= 32, 1 <= nb <= 64.                       */
/* The rank tolerance: the columns of a block are solutions of shift solves of relative accuracy gmres_tol (default
 * 1e-10), so columns that depend on their predecessors exactly -- a W of deficient rank -- have |R_ii| at that
 * accuracy times the solves' conditioning, not at rounding level (measured 1e-13 ... 4e-10 of the largest entry on the
 * dre test forms; the independent columns of every test problem are above 7e-4).  3e-8 is the level of the internal
 * recompressions: a direction below it changes Z Z^T by less than the rounding unit.                              */
#define RICADI_RADI_RANK_TOL 3e-8
#define RICADI_RADI_REFUSED_R_NOT_FINITE 1   /* a diagonal entry of R is not finite                                */
#define RICADI_RADI_REFUSED_R_ZERO 2         /* the diagonal of R is zero                                          */
#define RICADI_RADI_REFUSED_BREAKDOWN 3      /* ricadi_host_radi_shift returned RICADI_EBREAKDOWN                  */
#define RICADI_RADI_REFUSED_NO_SHIFT 4       /* no candidate, or a shift that is not finite and negative          */
int ricadi_host_radi_next_shift(int m, int nb, const double* H, const double* R, double* p_out, double* margin_out,
                                int* kept_out);
/* The same under RICADI_RADI_SHIFTS_HAMILTONIAN_DOMINANT: the basis is Q S, S (m x k) the left singular vectors of R
 * of its k = min(32, #{sigma_i >= RICADI_RADI_RANK_TOL sigma_1}) largest singular values, from a one-sided Jacobi
 * iteration on R itself (singular values resolved far below the tolerance; nothing squares the condition).  H is
 * turned into [S^T H_A S | S^T H_E S | S^T (H_R, H_U, H_B)] (k x (2k + m + 2nb)) and handed to the same selection.
 * *kept_out = k.  The refusals are the four values above, with EVERY entry of R looked at in place of its diagonal
 * (R = 0: no singular value is positive).  RICADI_EINVAL unless 1 <= m <= 127, 1 <= nb <= 64.                         */
int ricadi_host_radi_next_shift_dominant(int m, int nb, const double* H, const double* R, double* p_out,
                                         double* margin_out, int* kept_out);
/* What the host does between the one fetch of a RADI sweep and its recombination (the formulas at
 * ricadi_set_radi_sweep_width).  Host only, no GPU needed; long double inside.
 * ricadi_host_radi_sweep: g shifts (negative, pairwise distinct), Ghat g m x nb, Gamma (g + 1) m x (g + 1) m the Gram
 *   matrix of [R_0 | S], rhs = ||R^T R||_F of the iteration's first residual factor (<= 0: every residual reads 0),
 *   steps_left >= 1.  *k_out = the steps kept: the first j whose relative residual is <= res_reltol, else
 *   min(g, steps_left); res_out (>= g doubles) the relative residuals after steps 1 .. k; Cf_out (>= g m (g m + m + nb)
 *   doubles) = [T_k | T_k y[:k m] | T_k h[:k m]], row-major g m x (k m + m + nb), leading dimension k m + m + nb.
 *   1 <= g <= 16, g m <= RICADI_RADI_SWEEP_MAX_K, 1 <= nb <= 64.  RICADI_EBREAKDOWN if a pivot of M is not positive
 *   and finite.
 * ricadi_host_radi_sweep_width: the effective width for a cycled list of ns shifts: the largest G <= want with G <= ns,
 *   G mw <= RICADI_RADI_SWEEP_MAX_K, G times the column groups of an (mw + nb)-wide panel in the batched solve (one up
 *   to 32 columns, ceil((mw + nb) / 16) above) <= 16 and G <= max_steps; then halved until every sweep of the cycle
 *   -- sweep s takes entries s G .. s G + G - 1 of the cycled list -- has pairwise distinct shifts and a smallest pivot
 *   prod_{k<j} ((p_j - p_k) / (p_j + p_k))^2 >= RICADI_RADI_SWEEP_PIVOT.  1: the sequential form.  A prefix of an
 *   admissible sweep is admissible.  1 <= want <= 16.                                                               */
int ricadi_host_radi_sweep(int g, int m, int nb, const double* shifts, const double* Ghat, const double* Gamma,
                           double rhs, double res_reltol, int steps_left, int* k_out, double* res_out,
                           double* Cf_out);
/* The shifts of the next sweep under ricadi_set_radi_sweep_shifts (the rule there) from what a sweep
 * has fetched: H (c x (2c + m + 2nb)) and R (c x c) of the group's QR.  ps_out / crit_out (>= want each; crit_out may
 * be NULL): the admitted shifts in acceptance order and their criteria; *n_out their number; *kept_out (may be NULL)
 * the size of the basis.  Returns 0, or one of the RICADI_RADI_REFUSED_* values with *n_out = 0 (NO_SHIFT: no candidate
 * was admitted).  want = 1 gives ricadi_host_radi_next_shift_dominant's shift (c = m).  RICADI_EINVAL unless
 * 1 <= c, m <= 127, 1 <= nb <= 64, 1 <= want <= 16.  Host only.                                                     */
int ricadi_host_radi_sweep_shifts(int c, int m, int nb, const double* H, const double* R, int want, double* ps_out,
                                  double* crit_out, int* n_out, int* kept_out);
int ricadi_host_radi_sweep_width(const double* shifts, int ns, int mw, int nb, int want, int max_steps,
                                 int* width_out);

#ifdef __cplusplus
}
#endif
#endif /* RICADI_H */
