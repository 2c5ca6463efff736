/*
 * sip_lqr_amd.h -- C ABI of the MI355X (gfx950) batched regularized-LQR /
 * Riccati solver.  This is the drop-in boundary for the Newton-KKT linear
 * solve of joaospinto/sip_optimal_control: every entry point names the
 * reference interface it replaces (paths relative to the reference tree).
 *
 * The reference solves ONE problem per `LQR` object on the host
 * (sip_optimal_control/lqr.hpp:66-200).  This library solves `batch`
 * independent problems of one shape (uniform-dimension chain: the topology
 * of Topology::set_chain, lqr.cpp:32-40, and of Dimensions::set_uniform,
 * lqr.cpp:77-88) per call, on the GPU, with device-resident inputs and
 * outputs.  There is no CPU fallback: every compute entry point fails with
 * SIP_LQR_ERR_HIP / SIP_LQR_ERR_UNSUPPORTED rather than compute on the host.
 *
 * Plain C, plain pointers and sizes, no C++/torch types.  All device
 * pointers are ordinary HIP device pointers; `stream` is a hipStream_t
 * passed as void* (NULL = the default stream).  The caller owns every byte
 * (as in the reference: lqr.hpp:136-186, "mem_assign"/"num_bytes").
 * Device buffers must be 16-byte aligned (hipMalloc and every framework
 * allocator are; the LDS-DMA kernels return SIP_LQR_ERR_HIP otherwise).
 * The compute entry points only enqueue kernels on `stream` -- no host
 * synchronisation, no allocation, no memset / memcpy nodes -- so a loop of
 * them can be captured in a hipGraph and replayed on any stream, the first
 * call on a plan included: everything a plan needs on the device is uploaded
 * by its *_plan_create (the one exception is a plan latched INVALID at
 * creation, which reports through a synchronous copy).
 * Devices: a plan belongs to the HIP device ordinal it was created with.  Every
 * compute entry point makes that device current for the duration of the call
 * and restores the caller's current device before it returns, so `stream`
 * must be a stream of the plan's device (NULL = that device's default stream)
 * and the buffers must live on it (or be peer-accessible).  *_plan_create
 * leaves the caller's current device untouched as well.  A chain plan
 * created on a host without any HIP device serves the host-side entry points
 * only (sizes, pack / unpack, kernel name); its compute entry points return
 * SIP_LQR_ERR_HIP.
 *
 * ------------------------------------------------------------------------
 * Packed chain layout (device and host-staging buffers; scalar = double for
 * SIP_LQR_F64, float for SIP_LQR_F32).  All blocks are column-major and
 * compact (ld = rows), exactly as the reference maps them
 * (Eigen::Map<MatrixXd>(ptr, rows, cols), e.g. lqr.cpp:654-687).  Problems
 * are stored one after the other (problem-major); inside a problem, stages
 * i = 0..T follow each other; node i is the parent of edge i, node i+1 its
 * child:
 *
 *   mats  [batch][ for i in 0..T :  Q_i (n*n) | delta_i (n)          "node"
 *                    and, if i < T: A_i (n*n) | B_i (n*m) |
 *                                   M_i (n*m) | R_i (m*m) ]          "edge"
 *   vecs  [batch][ for i in 0..T :  q_i (n) | c_i (n)   , if i<T: r_i (m) ]
 *   sol   [batch][ for i in 0..T :  x_i (n) | y_i (n)   , if i<T: u_i (m) ]
 *   gains [batch][ for i in 0..T-1: K_i (m*n) | k_i (m) ]
 *   status[batch]  int32, FactorStatus codes below
 *
 * mats holds what LQR::factor() reads (LQR::Input::{Q,M,R,A,B,delta},
 * lqr.hpp:77-85; patched in by helpers.cpp:362-367), vecs what LQR::solve()
 * additionally reads ({q,r,c}, helpers.cpp:814-816), sol what it writes
 * (LQR::Output::{x,u,y}, lqr.hpp:91-94), gains the feedback terms
 * LQR::Workspace::{K,k} (lqr.hpp:112,118).
 * ------------------------------------------------------------------------
 */
#ifndef SIP_LQR_AMD_H
#define SIP_LQR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-problem factor status: the values of LQR::FactorStatus,
 * sip_optimal_control/lqr.hpp:68-74. */
enum {
  SIP_LQR_SUCCESS = 0,
  SIP_LQR_INVALID_DELTA = 1,
  SIP_LQR_F_FACTORIZATION_FAILURE = 2,
  SIP_LQR_G_FACTORIZATION_FAILURE = 3,
  SIP_LQR_INVALID_TOPOLOGY = 4
};

/* API-level return codes (the reference has no error channel besides
 * FactorStatus; these report misuse of this library). */
enum {
  SIP_LQR_OK = 0,
  SIP_LQR_ERR_INVALID_ARGUMENT = -1,
  SIP_LQR_ERR_UNSUPPORTED = -2, /* shape/dtype has no HIP kernel */
  SIP_LQR_ERR_HIP = -3,         /* a HIP runtime call failed   */
  SIP_LQR_ERR_ALLOC = -4
};

enum { SIP_LQR_F64 = 0, SIP_LQR_F32 = 1 };
/* Layout of `mats` (see "Packed chain layout" above):
 *   FULL       Q (n x n) and R (m x m) as full column-major squares, as LQR::Input holds them;
 *   SYMMETRIC  Q and R as their lower triangles packed by columns (column c: rows c .. n-1): n (n + 1) / 2 and
 *              m (m + 1) / 2 scalars.  The reference reads both triangles of a Q it takes to be symmetric
 *              (`V = Q`, lqr.cpp:658) and only the lower one of R (Eigen::LLT of G, lqr.cpp:697 -- G's strictly
 *              upper part comes from R + (B^T W) B there, the kernels here use the symmetric counterpart), so the
 *              upper triangles are redundant bytes of a bandwidth-bound sweep: 576 of the 7 840 B a problem-stage
 *              moves at n = 12, m = 4.  Everything else ([Q | delta] then [A | B | M | R] per stage) is unchanged. */
enum { SIP_LQR_LAYOUT_FULL = 0, SIP_LQR_LAYOUT_SYMMETRIC = 1 };

typedef struct sip_lqr_plan sip_lqr_plan;
/* Threading: like the reference (no globals; distinct LQR + Workspace pairs are independent, a
 * shared Workspace is not thread-safe), distinct plans may be used concurrently; one plan (and the
 * device buffers handed to it) serves one host thread / one stream at a time. */

/* Replaces: LQR::LQR(const Input&, Workspace&) + compile_topology()
 * (lqr.cpp:635-643) for `batch` problems of horizon T (= num_edges), state
 * dimension n, control dimension m, on HIP device `device`.  The chain
 * topology is compiled here once, like the reference caches its traversal
 * (lqr.cpp:641,646).  Every (dtype, n >= 1, m >= 1) is served: hot shapes by a
 * dedicated fused kernel, everything else by the general engine (one
 * wavefront per problem, see sip_lqr_kernel_name()). */
int sip_lqr_plan_create(int dtype, int64_t batch, int T, int n, int m,
                        int device, sip_lqr_plan **plan);
/* The same with a layout of `mats` other than FULL.  SIP_LQR_LAYOUT_SYMMETRIC: fp64 shapes with a symmetric-packed
 * fused kernel (sip_lqr_kernel_name() carries "sym": LDS-staged kernels with even n and m whose blocks stay whole
 * 16-byte pieces, the reference's n = 12, m = 4 benchmark shape among them); SIP_LQR_ERR_UNSUPPORTED otherwise.
 * sip_lqr_mats_len / _bytes, sip_lqr_split_mats_len, sip_lqr_pack_problem and every compute entry point follow the
 * plan's layout (sip_lqr_factor_solve_split: [Q | delta | M | R] with Q, R packed; what the Newton-KKT step's
 * condensation then writes); the one-sweep sip_lqr_solve_multi is FULL-layout only (a SYMMETRIC plan goes column by
 * column). */
int sip_lqr_plan_create_layout(int dtype, int64_t batch, int T, int n, int m, int device, int layout,
                               sip_lqr_plan **plan);
int sip_lqr_plan_layout(const sip_lqr_plan *plan);

void sip_lqr_plan_destroy(sip_lqr_plan *plan);

/* Opt-in (on = 1), on a plan whose kernel is chain_factor_solve_mt16 (exact (32,4) and (32,8) in fp32 and fp64; in
 * fp64 also the embeddings of 16 < n < 32 / other m <= 8 -- an fp32 plan of such a shape runs on the general engine and
 * the call changes nothing on it; likewise the rows for 12 and 16 controls and their embeddings on a plan that took
 * sip_lqr_plan_set_wide_controls BEFORE this call; not with SIP_LQR_SPLIT=general): sip_lqr_factor runs the backward
 * matrix sweep alone and keeps the factor state (W per node, K, -G^-1 per edge, the statuses), sip_lqr_solve a
 * vector-only sweep + rollout against it, sip_lqr_solve_multi up to 16 columns per sweep on the matrix cores.
 * sip_lqr_kernel_name gains the suffix " + chain_factor_mt16 + chain_solve_mt16"; sip_lqr_workspace_bytes does not
 * shrink; on the exact shapes sip_lqr_solve_multi_workspace_bytes becomes > 0 (g | k per node and column), on embedded
 * shapes it stays 0 and sip_lqr_solve_multi runs the new single-column solve per column.  sip_lqr_factor_solve is
 * unaffected.  The factor sweep scales F = I + D^1/2 V D^1/2 to a unit diagonal before it factors it; the fused
 * sweep does so in fp64 only: K from sip_lqr_factor on an opt-in plan agrees with K from sip_lqr_factor_solve on the
 * same plan to rounding (in fp32 it is the more accurate one on badly scaled problems), NOT bitwise.  sip_lqr_solve and
 * sip_lqr_solve_multi leave `sol` of a problem whose factorization failed untouched, on exact and embedded shapes.
 * The same call on a plan on which sip_lqr_plan_set_fused_f32 took effect BEFORE it (every row of that kernel; not with
 * SIP_LQR_SPLIT=general): sip_lqr_factor runs chain_factor_qf32, the backward matrix sweep alone, and keeps S = F^-1 per
 * node, K, the LDL factor of G per edge and the statuses; sip_lqr_solve runs chain_solve_cols_qf32 on one column against
 * that state (it reads A, B and delta of `mats`, not the cost) and leaves K | k in `gains`; sip_lqr_solve_multi carries
 * up to 8 columns per sweep.  sip_lqr_kernel_name gains the suffix " + chain_factor_qf32 + chain_solve_qf32";
 * sip_lqr_workspace_bytes does not change; sip_lqr_solve_multi_workspace_bytes(plan, c) becomes
 * batch * 4 * (T + 1) * min(c, 8) * (2 n + m) (g | h | k per node and column).  sip_lqr_factor_solve is unaffected,
 * bitwise.  sip_lqr_solve and sip_lqr_solve_multi leave `sol` of a problem whose factorization failed untouched.  In
 * the other call order (this call first, then sip_lqr_plan_set_fused_f32) nothing changes here and the plan is the
 * fused-fp32-only plan.
 * Call once, right after plan creation (after sip_lqr_plan_set_fused_f32 where both are wanted), before any size is
 * read.  Other plans: SIP_LQR_OK, nothing changes.
 * on = 0: nothing changes.  SIP_LQR_ERR_INVALID_ARGUMENT: NULL plan, or a second call with on = 1. */
int sip_lqr_plan_set_separate_sweeps(sip_lqr_plan *plan, int on);
int sip_lqr_has_separate_sweeps(const sip_lqr_plan *plan); /* 1 after a successful opt-in that took effect */

/* Opt-in (on = 1), on an fp32 FULL-layout plan that runs on the general engine and whose (n, m) has a row in the table
 * of the fused fp32 kernel chain_factor_solve_qf32 (csrc/chain_qf32.hpp: n <= 15, m <= 8; rows: n in {4, 6, 8, 12} x
 * m in {1, 2, 3, 4}, and (1, 1), (5, 3), (9, 2), (15, 8)): the plan takes that kernel -- one fused launch, four
 * problems per wavefront, the arithmetic of the fp64 kernels on `float` -- instead of the general engine's factor and
 * solve launches.  sip_lqr_kernel_name becomes "chain_factor_solve_qf32<n,m,direct>/f32"; sip_lqr_workspace_bytes
 * becomes the larger of the fused and the general layout (it does not shrink); the per-problem lengths are unchanged.
 * sip_lqr_factor, sip_lqr_solve and sip_lqr_solve_multi re-run the full sweep (factor on a zero right-hand side,
 * solve_multi column by column, sip_lqr_solve_multi_workspace_bytes stays 0), unless SIP_LQR_SPLIT=general keeps them
 * on the general engine; sip_lqr_solve then computes bitwise what sip_lqr_factor_solve computes.
 * sip_lqr_plan_set_separate_sweeps AFTER this call gives the three split calls sweeps of their own (one factorisation
 * for a factor followed by any number of solves; see there).  Statuses are exact;
 * sol and gains of a problem whose status != SUCCESS are unspecified, as for every fused kernel.
 * Call once, right after plan creation, before any size is read.  fp64 plans, fp32 plans whose shape has no row
 * (n = 16 and n = 32 among them), plans created under SIP_LQR_VARIANT=general, and on = 0: SIP_LQR_OK, nothing
 * changes.  SIP_LQR_ERR_INVALID_ARGUMENT: NULL plan, or a second call with on = 1 after one that took effect. */
int sip_lqr_plan_set_fused_f32(sip_lqr_plan *plan, int on);
int sip_lqr_has_fused_f32(const sip_lqr_plan *plan); /* 1 after an opt-in that took effect */

/* Opt-in (on = 1), on a FULL-layout plan that runs on the general engine, was not created under
 * SIP_LQR_VARIANT=general and has 9 <= m <= 16, n <= 32: the plan takes the n = 32 matrix-core kernel
 * chain_factor_solve_mt16 in its instantiations for 12 and 16 controls (csrc/chain_mt16_wide.hip; one problem per
 * wavefront, one fused launch) instead of the general engine's factor and solve launches.
 *   n = 32, m in {12, 16}, either dtype: the exact row; sip_lqr_kernel_name becomes
 *     "chain_factor_solve_mt16<32,12,mfma16x16x4>/f64" (or <32,16,...>, or /f32).
 *   any other fp64 shape in range (n <= 16 included), unless SIP_LQR_PAD=0: embedded in the row with the least M >= m
 *     by a device-side repack before and after the sweep (extra states and controls decouple exactly); the name
 *     gains " embedding (n,m)".
 *   an fp32 shape without an exact row: nothing changes, as for the m <= 8 rows of this kernel.
 * sip_lqr_workspace_bytes becomes the larger of the fused and the general layout (it does not shrink); the per-problem
 * lengths are unchanged.  sip_lqr_factor, sip_lqr_solve and sip_lqr_solve_multi re-run the fused sweep (factor on a
 * zero right-hand side, solve_multi column by column), unless SIP_LQR_SPLIT=general keeps them on the general engine;
 * sip_lqr_plan_set_separate_sweeps AFTER this call gives them sweeps of their own exactly as on the m <= 8 rows (up to
 * 16 columns per sweep on the exact rows, the single-column solve per column on embedded shapes; see there).  These
 * instantiations scale F = I + D^1/2 V D^1/2 to a unit diagonal before they factor it in both precisions.  Statuses are
 * exact; sol and gains of a problem whose status != SUCCESS are unspecified, as for every fused kernel.  A (n <= 16)
 * problem embedded in 32 x 32 tiles pays for the whole tile: measure before opting in at small n (README).
 * Call once, right after plan creation, before any size is read and before sip_lqr_plan_set_separate_sweeps.  Plans
 * the call does not apply to, and on = 0: SIP_LQR_OK, nothing changes.  SIP_LQR_ERR_INVALID_ARGUMENT: NULL plan, or a
 * second call with on = 1 after one that took effect. */
int sip_lqr_plan_set_wide_controls(sip_lqr_plan *plan, int on);
int sip_lqr_has_wide_controls(const sip_lqr_plan *plan); /* 1 after an opt-in that took effect */

/* Sizes, in bytes, of the whole-batch buffers.  Replace
 * LQR::Workspace::num_bytes / LQR::Output::num_bytes (lqr.hpp:104-106,
 * 146-186); size_t, not int (the reference's int overflows at batch
 * scale). */
size_t sip_lqr_mats_bytes(const sip_lqr_plan *plan);
size_t sip_lqr_vecs_bytes(const sip_lqr_plan *plan);
size_t sip_lqr_sol_bytes(const sip_lqr_plan *plan);
size_t sip_lqr_gains_bytes(const sip_lqr_plan *plan);
size_t sip_lqr_status_bytes(const sip_lqr_plan *plan);
size_t sip_lqr_workspace_bytes(const sip_lqr_plan *plan);
/* Problems per call and bytes per scalar (8: SIP_LQR_F64, 4: SIP_LQR_F32) of a plan. */
int64_t sip_lqr_plan_batch(const sip_lqr_plan *plan);
size_t sip_lqr_scalar_bytes(const sip_lqr_plan *plan);
/* Per-problem lengths in scalars (packed chain layout above). */
size_t sip_lqr_mats_len(const sip_lqr_plan *plan);
size_t sip_lqr_vecs_len(const sip_lqr_plan *plan);
size_t sip_lqr_gains_len(const sip_lqr_plan *plan);

/* Host-side layout conversion between the reference's per-stage pointer
 * tables (LQR::Input, lqr.hpp:76-85: double** indexed by node or edge; the
 * blocks are always double, as in the reference) and the packed chain
 * layout of problem `p` inside host staging buffers of mats_bytes /
 * vecs_bytes / sol_bytes.  For SIP_LQR_F32 plans the values are rounded to
 * float on the way in and widened on the way out. */
int sip_lqr_pack_problem(const sip_lqr_plan *plan, int64_t p,
                         double *const *Q, double *const *M, double *const *R,
                         double *const *q, double *const *r, double *const *A,
                         double *const *B, double *const *c,
                         double *const *delta, void *mats_host,
                         void *vecs_host);
int sip_lqr_unpack_solution(const sip_lqr_plan *plan, int64_t p,
                            const void *sol_host, double *const *x,
                            double *const *u, double *const *y);
int sip_lqr_unpack_gains(const sip_lqr_plan *plan, int64_t p,
                         const void *gains_host, double *const *K,
                         double *const *k);

/* Replaces: the loop body of BM_LQRFactorSolve
 * (benchmarks/lqr_benchmark.cpp:653-663) = LQR::factor_with_status()
 * (lqr.cpp:645-731) followed by LQR::solve() (lqr.cpp:735-871), for every
 * problem of the batch, as one fused launch.  Writes status[p]; sol/gains of
 * a problem whose status != SUCCESS are unspecified (the reference's solve()
 * after a failed factor is undefined, lqr.cpp:735).  d_workspace:
 * sip_lqr_workspace_bytes() of device scratch holding the per-node factor
 * state the forward rollout needs (the role of LQR::Workspace::{W,V,
 * F_factor,v,...}, lqr.hpp:110-119). Asynchronous on `stream`. */
int sip_lqr_factor_solve(const sip_lqr_plan *plan, const void *d_mats,
                         const void *d_vecs, void *d_sol, void *d_gains,
                         int32_t *d_status, void *d_workspace, void *stream);

/* The same fused sweep with the dynamics Jacobians read in place.  Replaces: the copy of ddyn_dx /
 * ddyn_du into LQR::Input::A / B (helpers.cpp:365-366) followed by the loop body above -- the
 * Newton-KKT step (sip_kkt_factor_solve) hands the Riccati sweep the Jacobians where the model
 * callback left them instead of copying them into `mats`.
 *   d_mats: per problem sip_lqr_split_mats_len() scalars: node blocks [Q | delta] as in the packed
 *           chain layout, edge blocks [M | R] (no A, B);
 *   d_ab  : stage i of problem p: A (n x n, column-major) then B (n x m, column-major) at
 *           d_ab + (p * ab_problem_stride + i * ab_stage_stride) scalars.
 * d_mats, d_vecs, d_gains, d_workspace 16-byte aligned; d_ab and its strides any (8-byte aligned scalars: a stage's
 * A | B is a whole number of 16-byte pieces and is copied exactly from sources that are only 8-byte aligned);
 * 3 * ab_problem_stride * 8 + (n*n + n*m) * 8 < 2^32 bytes (the four
 * problems of a wavefront are addressed by 32-bit offsets; SIP_LQR_ERR_INVALID_ARGUMENT beyond: that is
 * a problem stride of up to ~178 M scalars).  Available (sip_lqr_has_split() == 1) for fp64 plans whose fused
 * kernel is an LDS-staged one (n <= 15, m <= 8) and whose A | B block is a whole number of 16-byte pieces
 * (n (n + m) even: 88 of those 120 shapes, the reference's Newton-KKT benchmark grid among them; with n (n + m)
 * odd the blocks of every other stage would start on an odd 8-byte offset); SIP_LQR_ERR_UNSUPPORTED otherwise.
 * Everything else as sip_lqr_factor_solve. */
int sip_lqr_has_split(const sip_lqr_plan *plan);
int64_t sip_lqr_split_mats_len(const sip_lqr_plan *plan);
int sip_lqr_factor_solve_split(const sip_lqr_plan *plan, const void *d_mats, const void *d_ab,
                               int64_t ab_problem_stride, int64_t ab_stage_stride, const void *d_vecs, void *d_sol,
                               void *d_gains, int32_t *d_status, void *d_workspace, void *stream);

/* Replaces: LQR::factor_with_status() alone (lqr.cpp:645-731; called by
 * CallbackProvider::factor, helpers.cpp:368).  Leaves the factor state in
 * d_workspace and the K part of d_gains for later sip_lqr_solve() calls.
 * Shapes with a fused kernel run its backward sweep alone (fp64: plus the LDL
 * factors of the G matrices for the vector-only solve mode); other shapes run
 * on the general engine, whose work arena holds the reference's factor state.
 * sol of a problem whose status != SUCCESS is unspecified. */
int sip_lqr_factor(const sip_lqr_plan *plan, const void *d_mats, void *d_gains,
                   int32_t *d_status, void *d_workspace, void *stream);

/* Replaces: LQR::solve(Output&) alone (lqr.cpp:735-871; called by
 * CallbackProvider::solve, helpers.cpp:826) against the factor state of the
 * last sip_lqr_factor() on the same workspace; may be called repeatedly with
 * new right-hand sides (tests/lqr_test.cpp:431-450).  d_gains: the buffer that
 * sip_lqr_factor() filled (K is read, the k part is written).  Shapes with a
 * fused fp64 kernel run the affine sweep alone (vectors distributed over the
 * lanes, no matrix work) followed by the rollout.  Fills sol. */
int sip_lqr_solve(const sip_lqr_plan *plan, const void *d_mats,
                  const void *d_vecs, void *d_sol, void *d_gains,
                  void *d_workspace, void *stream);

/* Replaces: the multi-right-hand-side block of solve_stagewise_kkt_matrix
 * (helpers.cpp:521-665: LQR::solve generalised from one right-hand side to
 * num_rhs columns, reading LQR::Workspace directly; the caller is the theta
 * Schur complement, helpers.cpp:387) against the factor state of the last
 * sip_lqr_factor() on the same workspace.  d_vecs_cols / d_sol_cols: num_rhs
 * arrays of sip_lqr_vecs_bytes() each, one after the other (column c at
 * c * sip_lqr_vecs_bytes()).  Shapes with a multi-rhs kernel (every fp64 shape
 * n <= 16, m <= 8) carry up to 8 columns through ONE backward / forward sweep,
 * fetching every matrix operand of a stage once; plans with the separate sweeps
 * carry 8 (fp32, n <= 15) or 16 (n = 32) columns per launch;
 * d_col_workspace: sip_lqr_solve_multi_workspace_bytes() of device scratch
 * (per-column g, h, k of the rollout).  Other shapes run sip_lqr_solve() per
 * column (workspace bytes 0, d_col_workspace may be NULL).  The k part of
 * d_gains is unspecified afterwards. */
size_t sip_lqr_solve_multi_workspace_bytes(const sip_lqr_plan *plan, int num_rhs);
int sip_lqr_solve_multi(const sip_lqr_plan *plan, const void *d_mats,
                        const void *d_vecs_cols, void *d_sol_cols, int num_rhs,
                        void *d_gains, void *d_workspace, void *d_col_workspace,
                        void *stream);

/* The residual of the KKT system the chain entry points solve, evaluated in fp64 on the device (no counterpart in the
 * reference, whose callers form it on the host), in the vecs layout -- slot q_i, slot c_i, slot r_i:
 *   rho_q[i] = Q_i x_i - y_i + q_i  (+ M_i u_i + A_i^T y_{i+1}                if i < T)
 *   rho_c[0] = -x_0 - delta_0 o y_0 + c_0
 *   rho_c[i] = A_{i-1} x_{i-1} + B_{i-1} u_{i-1} - x_i - delta_i o y_i + c_i     (i >= 1)
 *   rho_r[i] = M_i^T x_i + R_i u_i + B_i^T y_{i+1} + r_i                       (i < T)
 * so that a solve whose right-hand side is rho returns the correction d with K (z + d) + b = 0.  Every plan has it
 * (every dtype, shape, layout and opt-in: it reads `mats` in the plan's layout and nothing of the workspace).  Every
 * product and sum is fp64 (fused multiply-adds); fp32 mats are widened on load; Q and R are taken symmetric.
 *   wide = 0: d_vecs and d_sol are in the plan's dtype; wide = 1: they are doubles, with the same per-problem lengths
 *             (on an SIP_LQR_F64 plan the two are the same thing);
 *   d_res   : batch * sip_lqr_vecs_len() doubles, or NULL when only the norms are wanted;
 *   d_norm  : batch doubles, d_norm[p] = max |rho| over problem p (NaN if an entry is).
 * Kernels only, asynchronous on `stream`.  SIP_LQR_ERR_INVALID_ARGUMENT, before any HIP call: a NULL plan, d_mats,
 * d_vecs, d_sol or d_norm, or a `wide` that is neither 0 nor 1. */
int sip_lqr_residual(const sip_lqr_plan *plan, const void *d_mats, const void *d_vecs, const void *d_sol, int wide,
                     double *d_res, double *d_norm, void *stream);

/* Iterative refinement in fp64 around the plan's own solve, against the factor state of the last sip_lqr_factor() on
 * d_workspace (the contract of sip_lqr_solve; d_gains is the buffer that call filled).  d_vecs64 (the right-hand
 * side) and d_sol64 (the iterate, read and written) are doubles with the per-problem lengths of vecs / sol, whatever
 * the plan's dtype.  `iterations` (1 .. 32) rounds of
 *   rho / s_p in the plan's dtype, s_p the power of two with s_p <= max |rho| < 2 s_p over problem p (1 when that
 *             norm is 0 or not finite): exact, and the correction solve stays in range however small rho has become;
 *   sip_lqr_solve on it (the plan's kernel, opt-ins included);
 *   sol64 += s_p * d, summed in fp64, skipped where d_status[p] != SIP_LQR_SUCCESS (d_status: the statuses the factor
 *             call wrote, or NULL: nothing is skipped);
 * then one more residual.  from_zero = 1: the iterate is zero-filled first, so round 1 is the plan's ordinary solve and
 * every later round a refinement step; from_zero = 0: d_sol64 holds the starting iterate.
 *   d_norms : (iterations + 1) * batch doubles; d_norms[j * batch + p] is max |rho| of problem p before round j + 1,
 *             the last row that of the result;
 *   d_refine_workspace: sip_lqr_refine_workspace_bytes() of device scratch =
 *             2 * up(batch * sip_lqr_vecs_len() * sip_lqr_scalar_bytes()) + up(batch * 8), up() rounding up to a
 *             multiple of 256: rho / s and d in the plan's dtype, then s.
 * The k part of d_gains is unspecified afterwards (as for sip_lqr_solve_multi); K is untouched.  Kernels only,
 * asynchronous on `stream`.  SIP_LQR_ERR_INVALID_ARGUMENT, before any HIP call: a NULL plan, d_mats, d_vecs64,
 * d_sol64, d_workspace, d_refine_workspace or d_norms (d_gains when T > 0), iterations outside 1 .. 32, from_zero
 * neither 0 nor 1. */
size_t sip_lqr_refine_workspace_bytes(const sip_lqr_plan *plan);
int sip_lqr_refine(const sip_lqr_plan *plan, const void *d_mats, const double *d_vecs64, double *d_sol64,
                   int iterations, int from_zero, void *d_gains, void *d_workspace, void *d_refine_workspace,
                   const int32_t *d_status, double *d_norms, void *stream);

/* sip_lqr_residual for several right-hand sides and iterates against one d_mats, the columns laid out as for
 * sip_lqr_solve_multi: column c of d_vecs_cols, d_sol_cols and d_res_cols is a whole-batch array at
 * c * batch * sip_lqr_vecs_len() scalars.  One launch stages a stage's blocks once and carries
 * sip_lqr_residual_multi_columns() columns through them (1 .. 8, by the shape and dtype of the plan, for a d_mats
 * that is 16-byte aligned; 0 for a NULL plan); the columns go in groups of that many, one launch per group.  Column c
 * is bit for bit what sip_lqr_residual computes on that column.  Formulas, `wide`, the dtype rules and "every plan has
 * it" are those of sip_lqr_residual.
 *   d_res_cols: num_rhs * batch * sip_lqr_vecs_len() doubles, or NULL when only the norms are wanted;
 *   d_norms   : num_rhs * batch doubles, d_norms[c * batch + p] = max |rho| over problem p in column c.
 * num_rhs = 0 launches nothing.  Kernels only, asynchronous on `stream`.  SIP_LQR_ERR_INVALID_ARGUMENT, before any HIP
 * call: a NULL plan, d_mats or d_norms, num_rhs < 0, num_rhs > 0 with a NULL d_vecs_cols or d_sol_cols, or a `wide`
 * that is neither 0 nor 1. */
int sip_lqr_residual_multi_columns(const sip_lqr_plan *plan);
int sip_lqr_residual_multi(const sip_lqr_plan *plan, const void *d_mats, const void *d_vecs_cols,
                           const void *d_sol_cols, int num_rhs, int wide, double *d_res_cols, double *d_norms,
                           void *stream);

/* sip_lqr_refine for several right-hand sides: the contract of sip_lqr_refine per column, the columns of d_vecs64_cols
 * and d_sol64_cols laid out as above (doubles).  `iterations` (1 .. 32) rounds of
 *   the scaled residual of all columns (sip_lqr_residual_multi's kernel), rho / s_{p,c} in the plan's dtype with one
 *             power of two per problem AND column, never one shared by the columns of a problem;
 *   sip_lqr_solve_multi on all num_rhs columns (whatever the plan runs: column sweeps, opt-ins, embedding, or column
 *             by column on the general engine);
 *   sol64[c][p] += s_{p,c} * d[c][p], skipped in every column where d_status[p] != SIP_LQR_SUCCESS (d_status: per
 *             problem, the statuses the factor call wrote, or NULL: nothing is skipped);
 * then one more residual of all columns.  from_zero as for sip_lqr_refine.
 *   d_norms : (iterations + 1) * num_rhs * batch doubles; d_norms[(j * num_rhs + c) * batch + p] is max |rho| of
 *             problem p in column c before round j + 1, the last row that of the result;
 *   d_col_workspace: sip_lqr_solve_multi_workspace_bytes(plan, num_rhs) of device scratch; may be NULL where that is 0;
 *   d_refine_workspace: sip_lqr_refine_multi_workspace_bytes(plan, num_rhs) of device scratch =
 *             2 * up(num_rhs * batch * sip_lqr_vecs_len() * sip_lqr_scalar_bytes()) + up(num_rhs * batch * 8), up()
 *             rounding up to a multiple of 256: rho / s, then d, both [num_rhs][batch][vecs_len] in the plan's dtype
 *             (sip_lqr_solve_multi's column arrays as they stand), then s[c][p]; 0 for a NULL plan or num_rhs < 1.
 * num_rhs = 0 launches nothing.  The k part of d_gains is unspecified afterwards; K is untouched.  Kernels only, no
 * allocation and no synchronisation, asynchronous on `stream`.  SIP_LQR_ERR_INVALID_ARGUMENT, before any HIP call:
 * what sip_lqr_refine rejects, num_rhs < 0, or a NULL d_col_workspace where its bytes are not 0. */
size_t sip_lqr_refine_multi_workspace_bytes(const sip_lqr_plan *plan, int num_rhs);
int sip_lqr_refine_multi(const sip_lqr_plan *plan, const void *d_mats, const double *d_vecs64_cols,
                         double *d_sol64_cols, int num_rhs, int iterations, int from_zero, void *d_gains,
                         void *d_workspace, void *d_col_workspace, void *d_refine_workspace,
                         const int32_t *d_status, double *d_norms, void *stream);

/* Gradients of a scalar loss L(z) through the solve (no counterpart in the reference).  The chain entry points solve
 * K z + b = 0 with z = (x, u, y), b = (q, r, c) and K symmetric (the formulas at sip_lqr_residual).  With g = dL/dz in
 * the sol layout, the adjoint lambda solves K lambda + g = 0 -- the plan's own solve with g as the right-hand side --
 * and dL/dvecs = lambda as it stands (slot q_i <-> x_i, slot c_i <-> y_i, slot r_i <-> u_i).  dL/dmats is a sum of
 * outer products of lambda = (lx_i, ly_i, lu_i) and z = (x_i, y_i, u_i), block by block, in the plan's layout:
 *   Q_i, FULL       1/2 (lx_i x_i^T + x_i lx_i^T), written to the whole square
 *   Q_i, SYMMETRIC  packed entry (r, c): lx_r x_c + lx_c x_r for r > c, lx_r x_r for r = c
 *   R_i             the same two rules with lu_i, u_i
 *   delta_i         -ly_i o y_i
 *   A_i             ly_{i+1} x_i^T + y_{i+1} lx_i^T
 *   B_i             ly_{i+1} u_i^T + y_{i+1} lu_i^T
 *   M_i             lx_i u_i^T + x_i lu_i^T
 * Q and R are taken symmetric everywhere in this library: the FULL rule is the gradient over symmetric perturbations
 * (dL = <G, dQ> for symmetric dQ), the SYMMETRIC rule the derivative with respect to the packed parameter, and the two
 * agree: <G_full, dQ> = sum over the packed entries of g_rc dQ_rc.
 *
 * sip_lqr_vjp_mats is the kernel alone: d_grad_mats (batch * sip_lqr_mats_len() scalars) from d_sol (z) and d_adj
 * (lambda).  Every plan has it (every dtype, shape, layout and opt-in: it reads nothing of `mats` and nothing of the
 * workspace).  Products and sums are fp64 (fused multiply-adds), fp32 inputs are widened on load, the result is
 * rounded once to the output scalar.
 *   wide = 0: d_sol, d_adj and d_grad_mats are in the plan's dtype; wide = 1: all three are doubles, with the same
 *             per-problem lengths (on an SIP_LQR_F64 plan the two are the same thing);
 *   d_status: NULL, or the statuses the factor call wrote: a problem whose status != SIP_LQR_SUCCESS gets an all-zero
 *             gradient, and its d_sol and d_adj (unspecified, possibly NaN) are not read.
 * Every scalar of d_grad_mats is written exactly once; d_grad_mats need only be aligned to its scalar.  Kernels only,
 * no allocation and no synchronisation, asynchronous on `stream`.  SIP_LQR_ERR_INVALID_ARGUMENT, before any HIP call:
 * a NULL plan, d_sol, d_adj or d_grad_mats, or a `wide` that is neither 0 nor 1.
 *
 * sip_lqr_vjp is the whole backward pass in the plan's dtype, against the factor state of the last sip_lqr_factor() on
 * d_workspace (the contract of sip_lqr_solve; d_gains is the buffer that call filled): sip_lqr_solve with d_grad_sol
 * (g) as the right-hand side into d_grad_vecs (lambda = dL/dvecs), then the kernel above on d_sol and d_grad_vecs.
 *   d_grad_mats: may be NULL: only lambda is wanted and the kernel is not launched;
 *   d_status   : NULL, or the statuses the factor call wrote: a failed problem ends with all-zero grad_vecs and
 *                all-zero grad_mats, whatever its solve left there.
 * The k part of d_gains is unspecified afterwards (as for sip_lqr_refine); K is untouched.  The gains K | k are not
 * differentiated: a loss that reads them gets no gradient from here.  sip_lqr_factor_solve alone does not leave the
 * state this call needs on every plan: call sip_lqr_factor first, as for sip_lqr_solve.  No second derivative is
 * offered.  SIP_LQR_ERR_INVALID_ARGUMENT, before any HIP call: a NULL plan, d_mats, d_sol, d_grad_sol, d_workspace or
 * d_grad_vecs (d_gains when T > 0). */
int sip_lqr_vjp_mats(const sip_lqr_plan *plan, const void *d_sol, const void *d_adj, int wide,
                     const int32_t *d_status, void *d_grad_mats, void *stream);
int sip_lqr_vjp(const sip_lqr_plan *plan, const void *d_mats, const void *d_sol, const void *d_grad_sol,
                void *d_gains, void *d_workspace, const int32_t *d_status, void *d_grad_vecs, void *d_grad_mats,
                void *stream);

/* The gradient for several right-hand sides against one d_mats: the caller solved K z_c + b_c = 0 for num_rhs columns
 * (sip_lqr_solve_multi) and the loss reads all the z_c, so dL/dmats = sum over c of G(lambda_c, z_c), G the outer
 * products above.  The columns are laid out as for sip_lqr_solve_multi: column c of d_sol_cols, d_adj_cols,
 * d_grad_sol_cols and d_grad_vecs_cols is a whole-batch array at c * batch * sip_lqr_vecs_len() scalars.  d_grad_mats
 * is ONE array of batch * sip_lqr_mats_len() scalars: the sum over the columns.
 *
 * sip_lqr_vjp_mats_multi is the kernel alone (`wide`, d_status and "every plan has it" as for sip_lqr_vjp_mats).  One
 * launch carries sip_lqr_vjp_multi_columns() columns (8, or fewer where 8 columns of one stage of z and lambda do not
 * fit 64 KiB of LDS; 0 for a NULL plan): it reads every column once and writes d_grad_mats once.  An entry is summed
 * in fp64 in ascending column order -- column 0 by the expression of sip_lqr_vjp_mats, every further column by two
 * fused multiply-adds onto the running sum -- and rounded once to the output scalar, so num_rhs = 1 gives the bits of
 * sip_lqr_vjp_mats.  More columns go in groups of that many, one launch per group.  The accumulate rule: the first
 * group never reads d_grad_mats; every later group reads the scalar the groups before left there, undoes the factor
 * 1, 1/2 or -1/2 exactly, continues the same chain of fused multiply-adds from it and stores again.  With double
 * output the result therefore does not depend on the grouping (barring underflow); with float output every group
 * boundary costs one rounding to float.  num_rhs = 0 writes an all-zero d_grad_mats (the empty sum).  A problem whose
 * status != SIP_LQR_SUCCESS gets an all-zero gradient from the first group and is left alone by the later ones; its
 * columns (unspecified, possibly NaN) are not read.  Every scalar of d_grad_mats is written exactly once per group;
 * d_grad_mats need only be aligned to its scalar.  SIP_LQR_VJP_MULTI_COLUMNS=<1..8> (a measuring aid, read per call)
 * caps the columns of a group.
 *
 * sip_lqr_vjp_multi is the whole backward pass in the plan's dtype against the factor state of the last
 * sip_lqr_factor() on d_workspace, in this order: sip_lqr_solve_multi with the d_grad_sol_cols (g_c) as right-hand
 * sides into d_grad_vecs_cols (lambda_c = dL/dvecs_c); where d_status is given, all-zero lambda_c of every failed
 * problem in every column; then the kernel above on d_sol_cols and d_grad_vecs_cols, unless d_grad_mats is NULL (only
 * the lambda_c are wanted).
 *   d_col_workspace: sip_lqr_solve_multi_workspace_bytes(plan, num_rhs) of device scratch; may be NULL where that is 0.
 * What sip_lqr_vjp says about sip_lqr_factor, the k part of d_gains, the gains and second derivatives holds here too.
 *
 * Both: kernels only, no allocation and no synchronisation, asynchronous on `stream`, safe under stream capture.
 * SIP_LQR_ERR_INVALID_ARGUMENT, before any HIP call: a NULL plan, num_rhs < 0, num_rhs > 0 with a NULL column array
 * (d_sol_cols, d_adj_cols, d_grad_sol_cols); sip_lqr_vjp_mats_multi: a NULL d_grad_mats, a `wide` that is neither 0
 * nor 1; sip_lqr_vjp_multi: a NULL d_mats, d_workspace or d_grad_vecs_cols (d_gains when T > 0), a NULL
 * d_col_workspace where its bytes are not 0. */
int sip_lqr_vjp_multi_columns(const sip_lqr_plan *plan);
int sip_lqr_vjp_mats_multi(const sip_lqr_plan *plan, const void *d_sol_cols, const void *d_adj_cols, int num_rhs,
                           int wide, const int32_t *d_status, void *d_grad_mats, void *stream);
int sip_lqr_vjp_multi(const sip_lqr_plan *plan, const void *d_mats, const void *d_sol_cols,
                      const void *d_grad_sol_cols, int num_rhs, void *d_gains, void *d_workspace,
                      void *d_col_workspace, const int32_t *d_status, void *d_grad_vecs_cols, void *d_grad_mats,
                      void *stream);

/* ------------------------------------------------------------------------
 * General trees / per-node dimensions (the full Topology + Dimensions model
 * of lqr.hpp:5-64): the path behind the drop-in C++ `LQR` adapter
 * (include/sip_optimal_control_amd/lqr_dropin.hpp).  `batch` instances of ONE
 * topology and dimension table, each with its own data; fp64; state and
 * control dimensions >= 0 (0 allowed, tests/variable_dimensions_test.cpp:
 * 316-336).
 *
 * Arenas (scalars = double, offsets from sip_lqr_tree_offset()):
 *   input  [batch][ node blocks: Q (n*n) | q (n) | c (n) | delta (n) ;
 *                   edge blocks: A (nc*np) | B (nc*m) | M (np*m) | R (m*m) | r (m) ]
 *   work   [batch][ edge blocks: W (max_n^2) | K (m*np) | G_factor (m*m) | k (m) ;
 *                   node blocks: V (n*n) | F_factor (n*n) | sqrt_delta (n) |
 *                                sqrt_delta_inv (n) | v (n) ; scratch ]
 *                  -- the fields of LQR::Workspace (lqr.hpp:110-127), same
 *                     meaning, so their consumers (helpers.cpp:521-665) can be
 *                     served from a copy of it
 *   output [batch][ node blocks: x (n) | y (n) ; edge blocks: u (m) ]
 * ------------------------------------------------------------------------ */
typedef struct sip_lqr_tree_plan sip_lqr_tree_plan;

/* Host-side topology compilation.  Replaces: compile_topology_data
 * (lqr.cpp:563-631): validates the edge list, builds the CSR children lists
 * (stable in edge index), DFS preorder (lowest edge index first) and the
 * reversed-preorder "postorder".  Output arrays are caller-owned with the sizes
 * of LQR::Workspace (lqr.hpp:129-135): child_offsets[N+1], child_edges[E],
 * edge_parents_out[E], edge_children_out[E], preorder[N], postorder[N],
 * node_marks[N].  Returns a FactorStatus (SUCCESS or INVALID_TOPOLOGY). */
int sip_lqr_compile_topology(int num_edges, int root, const int *edge_parents,
                             const int *edge_children, int *child_offsets,
                             int *child_edges, int *edge_parents_out,
                             int *edge_children_out, int *preorder,
                             int *postorder, int *node_marks);

/* Replaces: LQR::LQR + compile_topology (lqr.cpp:635-643) for `batch`
 * instances.  An invalid topology still yields a plan; its status is latched
 * (lqr.cpp:646-648) and returned by every sip_lqr_tree_factor(). */
int sip_lqr_tree_plan_create(int64_t batch, int num_edges, int root,
                             const int *edge_parents, const int *edge_children,
                             const int *state_dims, const int *control_dims,
                             int device, sip_lqr_tree_plan **plan);
void sip_lqr_tree_plan_destroy(sip_lqr_tree_plan *plan);
int sip_lqr_tree_topology_status(const sip_lqr_tree_plan *plan);
/* Compiled traversal (host copies, valid when the topology is valid):
 * which = 0 child_offsets[N+1], 1 child_edges[E], 2 preorder[N], 3 postorder[N] */
const int *sip_lqr_tree_topology_array(const sip_lqr_tree_plan *plan, int which);

/* Per-problem arena lengths in doubles. */
size_t sip_lqr_tree_input_len(const sip_lqr_tree_plan *plan);
size_t sip_lqr_tree_work_len(const sip_lqr_tree_plan *plan);
size_t sip_lqr_tree_output_len(const sip_lqr_tree_plan *plan);
/* Offset (in doubles, inside one problem) of a block: arena 0 = input,
 * 1 = work, 2 = output; kind 0 = node block, 1 = edge block; index = node or
 * edge id.  Returns (size_t)-1 on a bad argument. */
size_t sip_lqr_tree_offset(const sip_lqr_tree_plan *plan, int arena, int kind,
                           int index);

/* Replaces: LQR::factor_with_status() (lqr.cpp:645-731) for every instance:
 * reads Q, M, R, A, B, delta from d_input, writes the factor state to d_work
 * and FactorStatus codes to d_status[batch].  Asynchronous on `stream`. */
int sip_lqr_tree_factor(const sip_lqr_tree_plan *plan, const double *d_input,
                        double *d_work, int32_t *d_status, void *stream);
/* Replaces: LQR::solve(Output&) (lqr.cpp:735-871): reads q, r, c (and A, B,
 * delta) from d_input and the factor state from d_work, writes x, u, y to
 * d_output and k, v to d_work.  Instances whose d_status != SUCCESS are
 * skipped.  May be called repeatedly after one factor. */
int sip_lqr_tree_solve(const sip_lqr_tree_plan *plan, const double *d_input,
                       double *d_work, double *d_output,
                       const int32_t *d_status, void *stream);

/* Replaces: factor_with_status() + solve() (the loop body of BM_LQRVariableFactorSolve,
 * benchmarks/lqr_benchmark.cpp:716-744) for every instance, as one fused sweep: trees whose state
 * dimensions are <= 15 and control dimensions <= 8 run on a padded size class of the
 * broadcast-FMA kernels (csrc/tree_qw16.hpp; sip_lqr_tree_kernel_name() tells), anything else on the
 * general engine (factor, then solve).  Fills d_output (x, y, u), d_status and, of d_work, the
 * K and k fields of every edge (d_work may be NULL on the fused path: no gains wanted); the other
 * LQR::Workspace fields of d_work are only filled by sip_lqr_tree_factor().  d_scratch:
 * sip_lqr_tree_fused_scratch_bytes() bytes of device scratch (0: general engine, may be NULL). */
size_t sip_lqr_tree_fused_scratch_bytes(const sip_lqr_tree_plan *plan);
int sip_lqr_tree_factor_solve(const sip_lqr_tree_plan *plan, const double *d_input,
                              double *d_work, double *d_output, int32_t *d_status,
                              void *d_scratch, void *stream);
/* The same fused sweep, leaving in d_work (required) EVERY factor-state field of LQR::Workspace that
 * sip_lqr_tree_factor() leaves there (lqr.hpp:109-135: W, K, G_factor, k per edge; V, F_factor, sqrt_delta,
 * sqrt_delta_inv, v per node -- read by helpers.cpp:521-665), same arena layout: what the drop-in LQR class needs to
 * run on the fused kernels by default.  G_factor / F_factor: the lower triangle holds Eigen's L, the entries above
 * the diagonal their pre-factor values (Eigen::LLT factors in place, lqr.cpp:505, 697).  A second instantiation of
 * the kernel, so sip_lqr_tree_factor_solve() keeps its register budget. */
int sip_lqr_tree_factor_solve_workspace(const sip_lqr_tree_plan *plan, const double *d_input,
                                        double *d_work, double *d_output, int32_t *d_status,
                                        void *d_scratch, void *stream);
const char *sip_lqr_tree_kernel_name(const sip_lqr_tree_plan *plan);

/* The two halves of the fused sweep, as the reference calls them (CallbackProvider::factor / ::solve,
 * helpers.cpp:368, 826): exactly the data contracts of sip_lqr_tree_factor() / sip_lqr_tree_solve() on the
 * size-class kernels.  sip_lqr_tree_factor_fused() reads Q, M, R, A, B, delta (never q, r, c), writes W, K, G_factor
 * per edge and V, F_factor, sqrt_delta, sqrt_delta_inv per node to d_work (same layout and conventions as
 * sip_lqr_tree_factor_solve_workspace()) and the statuses to d_status (first failing node / edge in postorder, G
 * before delta before F at a node); it does not touch an output arena.  sip_lqr_tree_solve_fused() reads q, c, r
 * (and A, B, delta) from d_input and the factor state from d_work, writes x, y, u to d_output and v per node, k per
 * edge to d_work -- nothing else of d_work; instances whose d_status != SUCCESS are skipped, their outputs untouched.
 * May be called repeatedly after one factor.  A factor from sip_lqr_tree_factor(),
 * sip_lqr_tree_factor_solve_workspace() or sip_lqr_tree_factor_fused() serves sip_lqr_tree_solve(),
 * sip_lqr_tree_solve_fused() and sip_lqr_tree_solve_multi() alike.  d_scratch: sip_lqr_tree_fused_scratch_bytes()
 * bytes (0: general engine, may be NULL).  Trees beyond the size classes and plans created with
 * SIP_LQR_TREE=general run sip_lqr_tree_factor() / sip_lqr_tree_solve() themselves.  A latched invalid topology:
 * sip_lqr_tree_factor_fused() reports it as sip_lqr_tree_factor() does, sip_lqr_tree_solve_fused() returns
 * SIP_LQR_ERR_INVALID_ARGUMENT, as it does for a missing pointer, before any HIP call.  Both only enqueue kernels
 * on `stream` (no synchronisation, allocation or copy): graph-capturable.  sip_lqr_tree_split_kernel_name():
 * "tree_factor_qw16<N,M>/f64 + tree_solve_qw16<N,M>/f64" (the FACTOR_ONLY instantiation of tree_qw16.hpp and the
 * SINGLE one of tree_mrhs_qw16.hpp) or "tree_generic/f64"; "" for NULL. */
int sip_lqr_tree_factor_fused(const sip_lqr_tree_plan *plan, const double *d_input, double *d_work,
                              int32_t *d_status, void *d_scratch, void *stream);
int sip_lqr_tree_solve_fused(const sip_lqr_tree_plan *plan, const double *d_input, double *d_work,
                             double *d_output, const int32_t *d_status, void *d_scratch, void *stream);
const char *sip_lqr_tree_split_kernel_name(const sip_lqr_tree_plan *plan);

/* Replaces: the multi-right-hand-side block of solve_stagewise_kkt_matrix (helpers.cpp:414-747, its LQR part
 * :521-665: LQR::solve with GEMM in place of GEMV, reading LQR::Workspace directly; the caller is the theta Schur
 * complement K^-1 J_theta, helpers.cpp:387) on any tree, for num_rhs >= 1 columns against ONE factorization.
 *   right-hand sides: per problem and column sip_lqr_tree_rhs_len() doubles, node blocks q (n) | c (n), edge
 *                     blocks r (m) at sip_lqr_tree_rhs_offset(kind 0 = node / 1 = edge, index) -- the output
 *                     arena's layout; column c of problem b at (c * batch + b) * sip_lqr_tree_rhs_len();
 *   outputs         : per problem and column the output arena (x | y per node, u per edge), column c of problem b
 *                     at (c * batch + b) * sip_lqr_tree_output_len().
 * Reads A, B and delta from d_input (its q, r, c are ignored) and the factor state from d_work (W, G_factor, K per
 * edge; V, F_factor, sqrt_delta, sqrt_delta_inv per node), as sip_lqr_tree_factor() or
 * sip_lqr_tree_factor_solve_workspace() leave it.  d_work is only read: the per-column v and k (and g, h) go to
 * d_scratch, sip_lqr_tree_solve_multi_scratch_bytes(num_rhs) bytes of device scratch.  Instances whose
 * d_status != SUCCESS are skipped and their output columns left untouched.  Trees that fit a size class of the
 * fused kernels (state dimensions <= 15, control dimensions <= 8) carry up to 8 columns per wavefront through one
 * backward / forward sweep (csrc/tree_mrhs_qw16.hpp), fetching every matrix operand of a step once; anything else
 * (and plans created with SIP_LQR_TREE=general) runs the general engine column by column
 * (sip_lqr_tree_multi_kernel_name() tells).  num_rhs < 1, a missing pointer or a latched invalid topology:
 * SIP_LQR_ERR_INVALID_ARGUMENT before any HIP call.  Asynchronous on `stream`, kernels only. */
size_t sip_lqr_tree_rhs_len(const sip_lqr_tree_plan *plan);
size_t sip_lqr_tree_rhs_offset(const sip_lqr_tree_plan *plan, int kind, int index); /* (size_t)-1 if bad */
size_t sip_lqr_tree_solve_multi_scratch_bytes(const sip_lqr_tree_plan *plan, int num_rhs);
int sip_lqr_tree_solve_multi(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_work,
                             const double *d_rhs_cols, double *d_out_cols, int num_rhs,
                             const int32_t *d_status, void *d_scratch, void *stream);
const char *sip_lqr_tree_multi_kernel_name(const sip_lqr_tree_plan *plan);

/* The residual of the KKT system the tree entry points solve, evaluated in fp64 on the device (no counterpart in the
 * reference, whose callers form it on the host; the system is the one of tests/lqr_test.cpp:859-929), for any valid
 * tree plan -- either engine, dimensions of 0 and a single node included:
 *   rho_q[i]        = Q_i x_i - y_i + q_i + sum over the child edges e of i, in child_edges order, of
 *                     (M_e u_e + A_e^T y_child(e))
 *   rho_c[root]     = -x_root - delta_root o y_root + c_root
 *   rho_c[child(e)] = A_e x_parent(e) + B_e u_e - x_child - delta_child o y_child + c_child
 *   rho_r[e]        = M_e^T x_parent(e) + R_e u_e + B_e^T y_child + r_e
 * in the layout of a right-hand side of sip_lqr_tree_solve_multi (sip_lqr_tree_rhs_len / _offset: rho_q | rho_c where
 * x | y are, rho_r where u is), so that a solve whose right-hand side is rho returns the correction d with
 * K (z + d) + b = 0.  Every entry is summed in fp64 as a head + tail pair -- each product's rounding error kept by one
 * fused multiply-add, each sum's by an error-free transformation -- and rounded once at the end, so it is as accurate
 * as a sum in twice the working precision: what a refinement round can gain is bounded by what the residual resolves.
 * Q and R are taken symmetric from their lower triangles; the sum over the children of a node has one order, so two
 * launches give the same bits.
 *   d_input : the input arena (its A, B, M, R, Q, delta; q, c, r too when d_rhs is NULL);
 *   d_rhs   : NULL, or batch * sip_lqr_tree_rhs_len() doubles: q, c, r of every problem, one column;
 *   d_output: x, y, u in the output arena's layout (only read);
 *   d_res   : batch * sip_lqr_tree_rhs_len() doubles, or NULL when only the norms are wanted;
 *   d_norm  : batch doubles, d_norm[p] = max |rho| over problem p (NaN if an entry is).
 * Nothing of the work arena is read.  sip_lqr_tree_residual_kernel_name(): "tree_residual<staged>/f64" (the matrices
 * of a node and of an edge go through LDS) or "tree_residual<direct>/f64" (the largest of them exceeds a wavefront's
 * share of LDS: read in place), decided per plan; a d_input that is not 16-byte aligned is read in place whatever
 * the name says.  "" for NULL.  Kernels only, asynchronous on `stream`.  SIP_LQR_ERR_INVALID_ARGUMENT, before any HIP
 * call: a NULL plan or d_norm, a NULL d_input or d_output whose arena is not empty, a latched invalid topology. */
const char *sip_lqr_tree_residual_kernel_name(const sip_lqr_tree_plan *plan);
int sip_lqr_tree_residual(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_rhs,
                          const double *d_output, double *d_res, double *d_norm, void *stream);

/* Iterative refinement in fp64 around the plan's own solve, against the factor state in d_work (left by
 * sip_lqr_tree_factor(), sip_lqr_tree_factor_fused() or sip_lqr_tree_factor_solve_workspace(); only read).  d_output
 * is the iterate, read and written.  `iterations` (1 .. 32) rounds of
 *   rho / s_p, s_p the power of two with s_p <= max |rho| < 2 s_p over problem p (1 when that norm is 0 or not
 *             finite): exact, and the correction solve stays in range however small rho has become;
 *   sip_lqr_tree_solve_multi on it with one column (the fused size-class kernel or the general engine, as the plan
 *             dispatches);
 *   d_output += s_p * d, summed in fp64, skipped where d_status[p] != SIP_LQR_SUCCESS (d_status: the statuses the
 *             factor call wrote; required, as the solve skips those problems too);
 * then one more residual.  from_zero = 1: the iterate is zero-filled first, so round 1 is the plan's ordinary solve and
 * every later round a refinement step; from_zero = 0: d_output holds the starting iterate.  d_rhs: as for
 * sip_lqr_tree_residual().
 *   d_norms : (iterations + 1) * batch doubles; d_norms[j * batch + p] is max |rho| of problem p before round j + 1,
 *             the last row that of the result;
 *   d_refine_workspace: sip_lqr_tree_refine_workspace_bytes() of device scratch =
 *             2 * up(batch * sip_lqr_tree_rhs_len() * 8) + up(batch * 8) +
 *             up(sip_lqr_tree_solve_multi_scratch_bytes(plan, 1)), up() rounding up to a multiple of 256:
 *             rho / s, d, s, then the scratch of the one-column solve (0 for NULL or a latched invalid topology).
 * Kernels only, asynchronous on `stream`.  SIP_LQR_ERR_INVALID_ARGUMENT, before any HIP call: a NULL plan, d_work,
 * d_status, d_refine_workspace or d_norms, a NULL d_input or d_output whose arena is not empty, iterations outside
 * 1 .. 32, from_zero neither 0 nor 1, a latched invalid topology. */
size_t sip_lqr_tree_refine_workspace_bytes(const sip_lqr_tree_plan *plan);
int sip_lqr_tree_refine(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_work,
                        const double *d_rhs, double *d_output, int iterations, int from_zero,
                        const int32_t *d_status, void *d_refine_workspace, double *d_norms, void *stream);

/* sip_lqr_tree_residual for several right-hand sides and iterates against one d_input, the columns laid out as for
 * sip_lqr_tree_solve_multi: column c of d_rhs_cols, d_out_cols and d_res_cols is a whole-batch array at
 * c * batch * sip_lqr_tree_rhs_len() scalars.  One launch handles the matrices of a node or an edge once and carries
 * sip_lqr_tree_residual_multi_columns() columns through them (1 .. 8, by the topology and dimensions of the plan, for
 * a d_input that is 16-byte aligned; 0 for a NULL plan or a latched invalid topology); the columns go in groups of
 * that many, one launch per group, a group of one column on the kernel of sip_lqr_tree_residual.  Column c is bit for
 * bit what sip_lqr_tree_residual computes on that column.
 *   d_rhs_cols: NULL (q, c, r of d_input for every column), or num_rhs * batch * sip_lqr_tree_rhs_len() doubles;
 *   d_out_cols: num_rhs * batch * sip_lqr_tree_rhs_len() doubles, x, y, u of every column (only read);
 *   d_res_cols: num_rhs * batch * sip_lqr_tree_rhs_len() doubles, or NULL when only the norms are wanted;
 *   d_norms   : num_rhs * batch doubles, d_norms[c * batch + p] = max |rho| over problem p in column c.
 * sip_lqr_tree_residual_multi_kernel_name(): "tree_residual_cols<staged,NC>/f64" or "tree_residual_cols<direct,NC>/f64",
 * NC the columns of a full group, for an aligned d_input (one that is not is read in place); "" for NULL or a latched
 * invalid topology.  num_rhs = 0 launches nothing.  Kernels only, asynchronous on `stream`.
 * SIP_LQR_ERR_INVALID_ARGUMENT, before any HIP call: what sip_lqr_tree_residual rejects, num_rhs < 0, or num_rhs > 0
 * with a NULL d_out_cols whose arena is not empty. */
int sip_lqr_tree_residual_multi_columns(const sip_lqr_tree_plan *plan);
const char *sip_lqr_tree_residual_multi_kernel_name(const sip_lqr_tree_plan *plan);
int sip_lqr_tree_residual_multi(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_rhs_cols,
                                const double *d_out_cols, int num_rhs, double *d_res_cols, double *d_norms,
                                void *stream);

/* sip_lqr_tree_refine for several right-hand sides: the contract of sip_lqr_tree_refine per column, the columns of
 * d_rhs_cols and d_out_cols laid out as above.  `iterations` (1 .. 32) rounds of
 *   the scaled residual of all columns (sip_lqr_tree_residual_multi's kernel), rho / s_{p,c} with one power of two
 *             per problem AND column, never one shared by the columns of a problem;
 *   one sip_lqr_tree_solve_multi on all num_rhs columns;
 *   d_out_cols[c][p] += s_{p,c} * d[c][p], skipped in every column of a problem where d_status[p] != SIP_LQR_SUCCESS;
 * then one more residual of all columns.  from_zero as for sip_lqr_tree_refine.
 *   d_norms : (iterations + 1) * num_rhs * batch doubles; d_norms[(j * num_rhs + c) * batch + p] is max |rho| of
 *             problem p in column c before round j + 1, the last row that of the result;
 *   d_refine_workspace: sip_lqr_tree_refine_multi_workspace_bytes(plan, num_rhs) of device scratch =
 *             2 * up(num_rhs * batch * sip_lqr_tree_rhs_len() * 8) + up(num_rhs * batch * 8) +
 *             up(sip_lqr_tree_solve_multi_scratch_bytes(plan, num_rhs)), up() rounding up to a multiple of 256:
 *             rho / s, then d, both [num_rhs][batch][rhs_len] (sip_lqr_tree_solve_multi's column arrays as they
 *             stand), then s[c][p], then the solve's scratch; 0 for NULL, a latched invalid topology or num_rhs < 1.
 * num_rhs = 0 launches nothing.  Kernels only, no allocation and no synchronisation, asynchronous on `stream`.
 * SIP_LQR_ERR_INVALID_ARGUMENT, before any HIP call: what sip_lqr_tree_refine rejects, num_rhs < 0, or num_rhs > 0
 * with a NULL d_out_cols whose arena is not empty. */
size_t sip_lqr_tree_refine_multi_workspace_bytes(const sip_lqr_tree_plan *plan, int num_rhs);
int sip_lqr_tree_refine_multi(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_work,
                              const double *d_rhs_cols, double *d_out_cols, int num_rhs, int iterations, int from_zero,
                              const int32_t *d_status, void *d_refine_workspace, double *d_norms, void *stream);

/* Gradients of a scalar loss L(z) through the tree solve (no counterpart in the reference; the tree twin of
 * sip_lqr_vjp).  The tree entry points solve K z + b = 0 with z = (x_i, y_i per node; u_e per edge),
 * b = (q_i, c_i; r_e) and K symmetric (its rows are the rho_* formulas at sip_lqr_tree_residual).  With g = dL/dz in the
 * output arena's layout, the adjoint lambda solves K lambda + g = 0 -- sip_lqr_tree_solve_multi with one column and g
 * as the right-hand side -- and dL/db = lambda as it stands (slot q_i <-> x_i, slot c_i <-> y_i, slot r_e <-> u_e);
 * dL/dK = lambda z^T.  The gradient with respect to the input arena is an array in the input arena's own layout,
 * sip_lqr_tree_input_len() doubles per problem (node blocks Q | q | c | delta, edge blocks A | B | M | R | r, matrices
 * column-major), from lambda = (lx_i, ly_i; lu_e) and z; for node i, and edge e with parent p and child c:
 *   Q_i (n x n)    (r, col)  1/2 (lx_i[r] x_i[col] + x_i[r] lx_i[col]), written to the whole square
 *   q_i, c_i       j         lx_i[j], ly_i[j]
 *   delta_i        j         -ly_i[j] y_i[j]
 *   A_e (nc x np)  (r, col)  ly_c[r] x_p[col] + y_c[r] lx_p[col]
 *   B_e (nc x m)   (r, col)  ly_c[r] u_e[col] + y_c[r] lu_e[col]
 *   M_e (np x m)   (r, col)  lx_p[r] u_e[col] + x_p[r] lu_e[col]
 *   R_e (m x m)    (r, col)  1/2 (lu_e[r] u_e[col] + u_e[r] lu_e[col])
 *   r_e            j         lu_e[j]
 * Q and R follow the chain's FULL rule: the gradient over symmetric perturbations, dL = <G, dQ> for symmetric dQ.
 * The gains K | k and the other fields of the work arena are not differentiated: a loss that reads them gets no
 * gradient from here.  Gradients through sip_kkt_* are not offered.  No second derivative is offered.
 *
 * sip_lqr_tree_vjp_input is the kernel alone: d_grad_input (batch * sip_lqr_tree_input_len() doubles) from d_output
 * (z) and d_adj (lambda), both batch * sip_lqr_tree_output_len() doubles.  Every valid plan has it, on either engine,
 * dimensions of 0, a single node and no edges included: it reads nothing of the input or work arenas, only a table the
 * plan built when it was created (8 bytes per input-arena scalar on the device, freed with the plan).  An entry is
 * fma(lambda[ia], z[ib], z[ia] * lambda[ib]) in fp64 times 1, 1/2 or -1/2, or a copy of lambda.
 *   d_status: NULL, or the statuses the factor call wrote: a problem whose status != SIP_LQR_SUCCESS gets an all-zero
 *             gradient, and its d_output and d_adj (unspecified, possibly NaN) are not read.
 * Every scalar of d_grad_input is written exactly once and nothing else is; d_grad_input need only be aligned to 8
 * bytes; no atomics: two launches give the same bits.  An empty input arena launches nothing.
 * sip_lqr_tree_vjp_kernel_name(): "tree_vjp<staged>/f64" (z and lambda of a problem go through LDS) or
 * "tree_vjp<direct>/f64" (16 * sip_lqr_tree_output_len() bytes exceed 64 KiB: read in place), decided per plan; "" for
 * NULL or a latched invalid topology.  Kernels only, no allocation, copy or synchronisation, asynchronous on `stream`.
 * SIP_LQR_ERR_INVALID_ARGUMENT, before any HIP call: a NULL plan, a latched invalid topology, a NULL d_output, d_adj
 * or d_grad_input whose arena is not empty.
 *
 * sip_lqr_tree_vjp is the whole backward pass against the factor state in d_work (left by sip_lqr_tree_factor(),
 * sip_lqr_tree_factor_fused() or sip_lqr_tree_factor_solve_workspace(); only read), on the fused size-class kernels
 * and on the general engine alike: sip_lqr_tree_solve_multi with one column and d_grad_output (g) as the right-hand
 * side into d_adj (lambda = dL/d(q, c, r)); d_adj of every problem whose status != SIP_LQR_SUCCESS zeroed (the solve
 * leaves those untouched); then the kernel above on d_output and d_adj.
 *   d_status    : required: the statuses the factor call wrote; a failed problem ends with all-zero d_adj and
 *                 all-zero d_grad_input;
 *   d_grad_input: may be NULL: only lambda is wanted, the kernel is not launched and d_output is not needed;
 *   d_scratch   : sip_lqr_tree_vjp_scratch_bytes(plan) = sip_lqr_tree_solve_multi_scratch_bytes(plan, 1) of device
 *                 scratch.
 * Kernels only, no allocation, copy or synchronisation, asynchronous on `stream`.  SIP_LQR_ERR_INVALID_ARGUMENT,
 * before any HIP call: a NULL plan, a latched invalid topology, a NULL d_status, d_work or d_scratch, a NULL d_input,
 * d_grad_output or d_adj whose arena is not empty, a NULL d_output with d_grad_input given. */
const char *sip_lqr_tree_vjp_kernel_name(const sip_lqr_tree_plan *plan);
int sip_lqr_tree_vjp_input(const sip_lqr_tree_plan *plan, const double *d_output, const double *d_adj,
                           const int32_t *d_status, double *d_grad_input, void *stream);
size_t sip_lqr_tree_vjp_scratch_bytes(const sip_lqr_tree_plan *plan);
int sip_lqr_tree_vjp(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_work,
                     const double *d_output, const double *d_grad_output, const int32_t *d_status, double *d_adj,
                     double *d_grad_input, void *d_scratch, void *stream);

/* Gradients through sip_lqr_tree_solve_multi: several columns against ONE input arena, and one gradient (the tree twin
 * of sip_lqr_vjp_multi).  Column c solves K z_c + b_c = 0 with the caller's right-hand side b_c; a loss that reads
 * every z_c has dL/d(A, B, M, R, Q, delta) = sum over c of the table above on (lambda_c, z_c), with lambda_c the adjoint
 * of column c, and dL/db_c = lambda_c.  Columns are laid out as for sip_lqr_tree_solve_multi: column c at
 * c * batch * sip_lqr_tree_output_len() doubles; there is one d_grad_input of batch * sip_lqr_tree_input_len() doubles.
 *
 * sip_lqr_tree_vjp_input_multi is the kernel alone.  An entry of a matrix block or of delta is, over the columns in
 * ascending order and in fp64, fma(lambda_0[ia], z_0[ib], z_0[ia] * lambda_0[ib]) for the first column and
 * acc = fma(lambda_c[ia], z_c[ib], fma(z_c[ia], lambda_c[ib], acc)) for every further one, then times 1, 1/2 or -1/2
 * (exact) and one store.  THE q, c AND r SLOTS OF d_grad_input ARE WRITTEN +0.0: sip_lqr_tree_solve_multi ignores the
 * arena's q, c, r (its right-hand sides are the columns), so the true gradient there is zero, and dL/db_c is lambda_c
 * itself, which the caller holds as d_adj_cols.  One column therefore gives the bits of sip_lqr_tree_vjp_input on
 * every other entry and +0.0 on these.  One launch carries sip_lqr_tree_vjp_multi_columns() columns: min(8, what 160 KiB
 * of LDS hold at 16 * sip_lqr_tree_output_len() bytes per column; the kernel's limit of dynamic LDS is raised where a
 * group needs more than 64 KiB), or 8 read in place where not even one column fits 64 KiB; more columns go in further
 * launches, which read the scalar already in d_grad_input, undo its factor exactly and chain
 * their columns onto it, so the result does not depend on the grouping (barring underflow in the halving).
 * SIP_LQR_TREE_VJP_MULTI_COLUMNS=<1..8> caps the columns of a launch and SIP_LQR_TREE_VJP_COLS_SHAPE=<wavefronts>,
 * <entries per run>[,<KiB of LDS, 0: read in place>] replaces the launch shape: measuring aids, read per call.
 *   num_rhs : >= 0; 0 writes an all-zero gradient and reads no column;
 *   d_status: NULL, or the statuses the factor call wrote: a problem whose status != SIP_LQR_SUCCESS gets an all-zero
 *             gradient, and its columns (unspecified, possibly NaN) are not read.
 * Every scalar of d_grad_input is written exactly once per launch and nothing else is; d_grad_input need only be
 * aligned to 8 bytes; no atomics: two calls give the same bits.  An empty input arena launches nothing.
 * sip_lqr_tree_vjp_multi_columns(): 0 for NULL or a latched invalid topology.  sip_lqr_tree_vjp_multi_kernel_name():
 * "tree_vjp_cols<staged,NC>/f64" or "tree_vjp_cols<direct,NC>/f64" with NC the columns of a full launch; "" for NULL
 * or a latched invalid topology.  Kernels only, no allocation, copy or synchronisation, asynchronous on `stream`, safe
 * under stream capture.  SIP_LQR_ERR_INVALID_ARGUMENT, before any HIP call: a NULL plan, a latched invalid topology,
 * num_rhs < 0, num_rhs > 0 with a NULL d_out_cols or d_adj_cols whose arena is not empty, a NULL d_grad_input.
 *
 * sip_lqr_tree_vjp_multi is the whole backward pass against the factor state in d_work (left by any of the three
 * factor entry points; only read), on the fused size-class kernels and on the general engine alike: one
 * sip_lqr_tree_solve_multi with the columns d_grad_out_cols (g_c = dL/dz_c) as right-hand sides into d_adj_cols
 * (lambda_c = dL/db_c); every column of d_adj_cols zeroed where status != SIP_LQR_SUCCESS (the solve leaves those
 * untouched); then the kernel above on d_out_cols and d_adj_cols.
 *   d_status    : required; a failed problem ends with all-zero d_adj_cols and an all-zero d_grad_input;
 *   d_grad_input: may be NULL: only the lambda_c are wanted, the kernel is not launched and d_out_cols is not needed;
 *   d_scratch   : sip_lqr_tree_vjp_multi_scratch_bytes(plan, num_rhs) =
 *                 sip_lqr_tree_solve_multi_scratch_bytes(plan, num_rhs) of device scratch (required even where that
 *                 is 0);
 *   num_rhs     : >= 0; 0 solves nothing and writes an all-zero d_grad_input.
 * Kernels only, no allocation, copy or synchronisation, asynchronous on `stream`, safe under stream capture.
 * SIP_LQR_ERR_INVALID_ARGUMENT, before any HIP call: a NULL plan, a latched invalid topology, num_rhs < 0, a NULL
 * d_status, d_work or d_scratch, a NULL d_input whose arena is not empty, num_rhs > 0 with a NULL d_grad_out_cols or
 * d_adj_cols whose arena is not empty, a NULL d_out_cols with d_grad_input given (and num_rhs > 0). */
int sip_lqr_tree_vjp_multi_columns(const sip_lqr_tree_plan *plan);
const char *sip_lqr_tree_vjp_multi_kernel_name(const sip_lqr_tree_plan *plan);
int sip_lqr_tree_vjp_input_multi(const sip_lqr_tree_plan *plan, const double *d_out_cols, const double *d_adj_cols,
                                 int num_rhs, const int32_t *d_status, double *d_grad_input, void *stream);
size_t sip_lqr_tree_vjp_multi_scratch_bytes(const sip_lqr_tree_plan *plan, int num_rhs);
int sip_lqr_tree_vjp_multi(const sip_lqr_tree_plan *plan, const double *d_input, const double *d_work,
                           const double *d_out_cols, const double *d_grad_out_cols, int num_rhs,
                           const int32_t *d_status, double *d_adj_cols, double *d_grad_input, void *d_scratch,
                           void *stream);

/* Name of the kernel variant the plan dispatches to (static string). */
const char *sip_lqr_kernel_name(const sip_lqr_plan *plan);

/* Library version string. */
const char *sip_lqr_version(void);

#ifdef __cplusplus
}
#endif
#endif
