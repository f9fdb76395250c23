/*
 * mtg.h -- C ABI of the MI355X batched minimum-derivative polynomial
 * optimizer (libmav_trajectory_generation.so).  Plain C types only: pointers, sizes, status codes.
 *
 * The reference (magrimm/mav_trajectory_generation_cmake) has no FFI; its
 * boundary is the C++ template class PolynomialOptimization<N>
 * (mav_trajectory_generation/include/mav_trajectory_generation/
 * polynomial_optimization_linear.h:45-269).  Each entry point below states
 * which reference interface it replaces.  The C++ drop-in headers at the
 * reference's include paths (include/mav_trajectory_generation/ headers, namespace
 * mav_trajectory_generation) are written on top of this ABI, and
 * INTEGRATION.md shows the bindings (C++, CMake, ctypes) a maintainer adds.
 *
 * Rules: the library never aborts and never throws; calls return MTG_OK or a
 * negative MTG_ERR_*.  All buffers are caller-owned and never retained after
 * a call returns (with MTG_FLAG_ASYNC: until the stream is synchronized).
 * One mtg_ctx serialises its calls; different contexts are thread-safe.
 *
 * Data layout (all FP64, row-major, B = batch, V = K + 1 vertices,
 * h = N / 2 derivatives 0..h-1 per vertex, D dimensions):
 *   values   [B][V][h][D]  value of derivative k at vertex v, dimension d
 *                          (read only where the derivative is fixed)
 *   fixed_mask [B][V]      uint8, bit k set => derivative k of vertex v is
 *                          fixed (Vertex::addConstraint, vertex.h:58-64);
 *                          bits >= h are dropped with a warning status, as
 *                          setupFromVertices does (lin_impl:74-95)
 *   times    [B][K]        segment times, must be > 0 (lin_impl:287)
 *   coeffs   [B][K][D][N]  polynomial coefficients, increasing powers
 *                          (polynomial_optimization_linear.h:42-44)
 *   free_out [B][D][V*h]   optional: getFreeConstraints() values
 *                          (polynomial_optimization_linear.h:180-184) in the
 *                          reference order (sorted by vertex, then derivative)
 *   n_free_out [B]         optional: getNumberFreeConstraints()
 *   cost_out [B]           optional: computeCost() = 0.5 sum c^T Q c
 *                          (lin_impl:114-130)
 *   status   [B]           optional: per-trajectory MTG_TRAJ_* bits
 * ("lin_impl" = .../impl/polynomial_optimization_linear_impl.h)
 */
#ifndef MTG_H_
#define MTG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTG_ABI_VERSION 5   /* 2: + mtg_soft_constraint_cost_batch, mtg_host_soft_constraint_cost_batch
                               3: + mtg_collision_time_gradient_batch, mtg_host_collision_time_gradient_batch
                               4: + mtg_objective_batch, mtg_host_objective_batch, mtg_host_objective_bounds_batch
                               5: + mtg_objective_time_batch, mtg_host_objective_time_batch,
                                    mtg_host_objective_time_bounds_batch
                               5, additive: + mtg_evaluate_at_batch, mtg_host_evaluate_at_batch,
                                    mtg_evaluate_at_path
                               5, additive: + mtg_solve_linear_ragged_batch, mtg_host_solve_linear_ragged_batch,
                                    mtg_solve_ragged_plan
                               5, additive: + mtg_evaluate_at_ragged_batch, mtg_evaluate_at_ragged_path,
                                    mtg_host_evaluate_at_ragged_batch, mtg_min_max_magnitude_ragged_batch,
                                    mtg_host_min_max_magnitude_ragged_batch
                               5, additive: + mtg_segment_min_max_magnitude_batch, mtg_segment_min_max_axis_batch,
                                    mtg_host_segment_min_max_magnitude_batch, mtg_host_segment_min_max_axis_batch
                               5, additive: + mtg_evaluate_range_ragged_batch, mtg_evaluate_range_ragged_batch_full
                               5, additive: + mtg_coefficients_from_vertices_ragged_batch,
                                    mtg_vertex_derivatives_ragged_batch, mtg_vertex_ragged_tile,
                                    mtg_collision_cost_ragged_batch, mtg_host_vertex_derivatives_batch,
                                    mtg_host_vertex_derivatives_ragged_batch,
                                    mtg_host_coefficients_from_vertices_ragged_batch,
                                    mtg_host_collision_cost_ragged_batch */

/* Call-level return codes. */
#define MTG_OK 0
#define MTG_ERR_INVALID_ARGUMENT (-1)
#define MTG_ERR_UNSUPPORTED_N (-2)     /* N must be even, 2 <= N <= 12 (polynomial.h:46) */
#define MTG_ERR_BAD_DERIVATIVE (-3)    /* 0 <= r <= N/2-1 (lin_impl:50-55) */
#define MTG_ERR_SIZE_MISMATCH (-4)     /* K < 1, D < 1, B < 0 (lin_impl:66-67, :279-281) */
#define MTG_ERR_HIP (-5)               /* HIP runtime error, see mtg_last_error() */
#define MTG_ERR_NO_DEVICE (-6)
#define MTG_ERR_OUT_OF_MEMORY (-7)
#define MTG_ERR_TOO_LARGE (-8)         /* per-trajectory working set exceeds LDS */

/* Per-trajectory status bits (status[b]). */
#define MTG_TRAJ_OK 0
#define MTG_TRAJ_BAD_TIME 1            /* some T <= 0 or not finite (CHECK_GT lin_impl:287) */
#define MTG_TRAJ_NOT_SPD 2             /* non-positive pivot in R_pp (reference: undetected, lin_impl:355-368),
                                          or some 0 < T < DBL_EPSILON, where the reference's A(T) is
                                          singular (baseCoeffsWithTime, polynomial.h:225) */
#define MTG_TRAJ_ROW_TOO_SHORT 4        /* mtg_objective[_time]_batch with MTG_FLAG_DEVICE_PTRS: x_stride is shorter than
                                          this trajectory's row (a host-pointer call returns
                                          MTG_ERR_INVALID_ARGUMENT instead); its x is not read */
#define MTG_TRAJ_WARN_DROPPED 256      /* constraint of order > N/2-1 ignored (LOG(WARNING) lin_impl:84-87) */
#define MTG_TRAJ_ERROR_MASK 255

/* Flags. */
#define MTG_FLAG_DEVICE_PTRS 1u        /* all array arguments are device pointers on the ctx device */
#define MTG_FLAG_ASYNC 2u              /* do not synchronize the stream before returning */
#define MTG_FLAG_SPLIT_KERNELS 4u      /* two-kernel path: assembly kernel + block-Cholesky kernel */
#define MTG_FLAG_GENERAL_KERNEL 8u     /* diagnostics: always use the general LDS-resident fused kernel
                                          (default: see mtg_solve_kernel) */
/* Deprecated (ABI 1 names kept so round-3 callers still compile): 16u and 32u selected the
 * lane-per-chain and interior-waypoint lane kernels, retired in round 4 (measured slower than the
 * default everywhere).  The bits are reserved and ignored: a call that sets them runs
 * the default kernel, and mtg_solve_kernel never returns MTG_KERNEL_LANE or MTG_KERNEL_IP. */
#define MTG_FLAG_LANE_KERNEL 16u       /* deprecated, ignored */
#define MTG_FLAG_IP_KERNEL 32u         /* deprecated, ignored */

#define MTG_FLAG_DL_KERNEL 64u         /* the dimension-lane kernel where it applies (N = 10 with K = 10,
                                          N = 12 with K = 20; D <= 4, r >= 1; one lane per (chain,
                                          dimension)).  The reference generators' pattern takes its pattern
                                          pass, any other mask with every position fixed its general-mask
                                          pass, and a trajectory with a free position the general fused
                                          kernel's block function inside it (with that kernel's bits):
                                          DESIGN.md 3.2c.  The default for those shapes at every batch size */
#define MTG_FLAG_COLUMN_KERNEL 128u    /* the register column kernel wherever it applies, also where the
                                          default for the batch size is the dimension-lane kernel (A/B) */
#define MTG_DL_MIN_BATCH 1             /* Deprecated (round 3: 2048; kept as 1 for callers that test it).
                                          Since round 4 the dimension-lane kernel is the
                                          default at every batch size where it applies, so a trajectory's
                                          result never depends on the size of the call or on the other
                                          trajectories in it (it was faster at every size) */

/* Solve kernels (mtg_solve_kernel): which one mtg_solve_linear_batch runs for a shape.  (1 and 5,
   MTG_KERNEL_LANE and MTG_KERNEL_IP, named the kernels retired in round 4: deprecated, never returned.) */
#define MTG_KERNEL_LANE 1              /* deprecated */
#define MTG_KERNEL_IP 5                /* deprecated */
#define MTG_KERNEL_COLUMN 2            /* default: register column kernel, a lane per column of G_v /
                                          per dimension, twisted (K <= 12, N = 12 up to K = 20) */
#define MTG_KERNEL_GENERAL 3           /* general LDS-resident fused kernel (any K) */
#define MTG_KERNEL_SPLIT 4             /* assembly kernel + block-Cholesky kernel */
#define MTG_KERNEL_DL 6                /* one lane per (chain, dimension) (MTG_FLAG_DL_KERNEL) */
#define MTG_KERNEL_DLX 7               /* the same for chains of other lengths (N = 6 / 8 / 10 / 12, D <= 4,
                                          r >= 1, where neither the DL nor the column kernel applies: e.g. the
                                          reference benchmark's K = 50 / 100), plus the general kernel's
                                          block function for trajectories whose interior vertices do not
                                          fix exactly their position */

typedef struct mtg_ctx mtg_ctx;

/* Version / diagnostics. */
int mtg_abi_version(void);
/* The solve kernel (MTG_KERNEL_*) mtg_solve_linear_batch runs for this shape and these flags, or a
   negative MTG_ERR_* for a shape it rejects.  No device work. */
int mtg_solve_kernel(int N, int D, int K, int derivative_to_optimize, unsigned flags);
/* The same for a batch of B trajectories (or trajectory x candidate pairs).  Since round 4 the answer
   does not depend on B (kept for round-3 callers). */
int mtg_solve_kernel_batch(int N, int D, int K, int derivative_to_optimize, int64_t B, unsigned flags);
const char* mtg_status_string(int code);
const char* mtg_last_error(mtg_ctx* ctx);

/* Devices and contexts.  A context owns a HIP stream on one device plus
 * staging buffers for host-pointer calls. */
int mtg_device_count(int* count);
int mtg_create(int device, mtg_ctx** out_ctx);
int mtg_destroy(mtg_ctx* ctx);
/* Launch on an external hipStream_t (e.g. torch's current stream).  NULL
 * selects the HIP null (default) stream; mtg_reset_stream restores the
 * context's own stream. */
int mtg_set_stream(mtg_ctx* ctx, void* hip_stream);
int mtg_reset_stream(mtg_ctx* ctx);
void* mtg_get_stream(mtg_ctx* ctx);
int mtg_synchronize(mtg_ctx* ctx);

/* Batched setupFromVertices + solveLinear.  Replaces, per trajectory,
 *   PolynomialOptimization<N>(D)                 lin_impl:33-44
 *   setupFromVertices(vertices, times, r)        lin_impl:47-99
 *     updateSegmentTimes                         lin_impl:276-295
 *     setupConstraintReorderingMatrix            lin_impl:172-250
 *   solveLinear()                                lin_impl:329-369
 *     constructR + SparseQR + per-dim solve      lin_impl:298-365
 *     updateSegmentsFromCompactConstraints       lin_impl:253-273
 *   getSegments / getFreeConstraints / computeCost.
 * One call solves B independent problems of identical shape (N, D, K, r);
 * masks and values may differ per trajectory. */
int mtg_solve_linear_batch(mtg_ctx* ctx, int N, int D, int K, int derivative_to_optimize,
                           int64_t batch, const double* values, const uint8_t* fixed_mask,
                           const double* times, double* coeffs, double* free_out,
                           int32_t* n_free_out, double* cost_out, int32_t* status,
                           unsigned flags);

/* mtg_solve_linear_batch for a batch whose trajectories have different segment counts (ragged K):
 * PolynomialOptimization<N> takes any number of vertices per instance, and a planner's candidate
 * paths have a different waypoint count each.  One call, no bucketing by the caller.
 *
 * Layout (CSR, no padding).  K_b = seg_count[b], V_b = K_b + 1; vo[b] = sum_{j<b} V_j and
 * so[b] = sum_{j<b} K_j, both 64-bit.  Trajectory b owns
 *   values     [vo[b] .. vo[b] + V_b][h][D]
 *   fixed_mask [vo[b] .. vo[b] + V_b]
 *   times      [so[b] .. so[b] + K_b]
 *   coeffs     [so[b] .. so[b] + K_b][D][N]
 *   free_out   the block [D][V_b h] at double offset D h vo[b]; entries >= n_free are +0.0
 *   n_free_out[b], cost_out[b], status[b]
 * Each block is exactly what mtg_solve_linear_batch reads or writes for one trajectory of K_b
 * segments, so a run of consecutive trajectories with equal K is a valid uniform array for every
 * uniform-K entry point.  The nullable outputs are those of the uniform call.
 * seg_count [B] is shape metadata, like K in the uniform call: a HOST array also with
 * MTG_FLAG_DEVICE_PTRS, read during the call and not kept.
 *
 * Semantics: for every b, every output byte equals what
 * mtg_solve_linear_batch(ctx, N, D, K_b, r, 1, ...that trajectory's blocks..., flags) writes, the
 * status bits and whatever the coefficients hold under an error bit included.  flags pass to every
 * group unchanged (MTG_FLAG_GENERAL_KERNEL, _DL_KERNEL, _COLUMN_KERNEL, _SPLIT_KERNELS; _DEVICE_PTRS
 * and _ASYNC with their usual meaning); the kernel for K_b is mtg_solve_kernel(N, D, K_b, r, flags).
 *
 * The plan (host code, mtg_solve_ragged_plan reports it).  A group is all trajectories with one K.
 * A group whose members are consecutive in the batch (one run) is solved in place: the uniform
 * launcher runs on slices of the caller's arrays and nothing is copied.  Every other group is
 * gathered: one kernel copies its inputs into packed uniform arrays owned by the context, the
 * uniform launcher runs there, and one kernel copies the outputs to their CSR positions.  Groups are
 * launched in ascending K on the context's stream with no host synchronisation in between.  A caller
 * who sorts the batch by K gets every group in place (zero copies).  In-place slices are 8-byte
 * aligned for the doubles and byte aligned for the mask whatever the arrays' own alignment; coeffs
 * slices keep the alignment of coeffs modulo 16 (K D N is even).  The solve kernels need no more
 * (DESIGN.md 3.14).
 * Host-pointer calls stage the CSR arrays whole and run the same path (no chunked pipeline).
 * mtg_last_kernel_ms spans the call's first to its last kernel.  Two MTG_FLAG_ASYNC calls on one
 * context may follow each other without a synchronisation between them.
 *
 * Errors, all before any device work: those of the uniform call on N, D, r and batch;
 * MTG_ERR_INVALID_ARGUMENT for seg_count == NULL with batch > 0; MTG_ERR_SIZE_MISMATCH for any
 * seg_count[b] < 1; the code of mtg_solve_kernel if it rejects some K that is present
 * (MTG_ERR_TOO_LARGE).  batch == 0: MTG_OK. */
int mtg_solve_linear_ragged_batch(mtg_ctx* ctx, int N, int D, int derivative_to_optimize, int64_t batch,
                                  const int32_t* seg_count, const double* values, const uint8_t* fixed_mask,
                                  const double* times, double* coeffs, double* free_out, int32_t* n_free_out,
                                  double* cost_out, int32_t* status, unsigned flags);
/* The plan of that call for these segment counts, with its call-level errors: *n_groups distinct K,
 * *n_in_place trajectories in groups solved in place (== batch for a batch sorted by K),
 * *total_segments = sum K_b (any pointer may be NULL).  No context, no device work. */
int mtg_solve_ragged_plan(int N, int D, int derivative_to_optimize, int64_t batch, const int32_t* seg_count,
                          unsigned flags, int64_t* n_groups, int64_t* n_in_place, int64_t* total_segments);

/* Contiguous shard `shard` (0 <= shard < n_shards) of a batch of `batch` independent problems:
 * [*begin, *end) = [g ceil(B/G), min(B, (g+1) ceil(B/G))).  The partition that
 * mtg_solve_linear_batch_multi, bench.py's ranks and the Python layer use.  No device work. */
int mtg_shard_range(int64_t batch, int n_shards, int shard, int64_t* begin, int64_t* end);

/* mtg_solve_linear_batch over several contexts, normally one per device (mtg_create(g, ...)), in one
 * call: the batch is cut into n_ctxs contiguous shards (mtg_shard_range) and shard g is solved by
 * ctxs[g] on its own host thread (the calling thread takes shard 0), each with its own staging /
 * chunk pipeline, writing its disjoint slice of the outputs.  Trajectories are independent, so there
 * is no collective.  This replaces a caller's loop of single solves over a whole batch
 * (src/polynomial_timing_evaluation.cpp:119-126) with one call that uses every GPU of the node.
 * Host arrays only (MTG_FLAG_DEVICE_PTRS and MTG_FLAG_ASYNC are rejected: device arrays live on one
 * device); the call returns when every shard has landed.  Results are bit-identical to one
 * mtg_solve_linear_batch over the whole batch.  On failure the first failing shard's code is
 * returned and mtg_last_error(ctxs[0]) names the shard.  Distinct contexts run concurrently; a
 * context listed twice serialises its shards. */
int mtg_solve_linear_batch_multi(mtg_ctx* const* ctxs, int n_ctxs, int N, int D, int K, int derivative_to_optimize,
                                 int64_t batch, const double* values, const uint8_t* fixed_mask,
                                 const double* times, double* coeffs, double* free_out, int32_t* n_free_out,
                                 double* cost_out, int32_t* status, unsigned flags);

/* Diagnostics: the next mtg_solve_linear_batch on ctx (also as one shard of a multi-device solve)
 * returns `code` (a negative MTG_ERR_*) without touching any array, as a failing device would --
 * for testing how a caller or mtg_solve_linear_batch_multi propagates a shard's failure. */
int mtg_debug_fail_next_solve(mtg_ctx* ctx, int code);

/* Batched Trajectory::evaluateRange (src/trajectory.cpp:68-128) over solved
 * trajectories, with the reference's sequential time accumulation (acc += dt)
 * reproduced exactly.  coeffs [B][K][D][N], times [B][K].  Sample counts are
 * ragged: first call with out == NULL to get counts[B] (samples per
 * trajectory); then pass the same counts (read), offsets[B] (exclusive prefix
 * sum of counts, in samples) and out [sum(counts)][D] (+ optional
 * sample_times [sum]).
 * t_start/t_end/dt are shared by the whole batch; derivative selects the
 * derivative order evaluated (Polynomial::evaluate, polynomial.h:138-151). */
int mtg_evaluate_range_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch,
                             const double* coeffs, const double* times, double t_start,
                             double t_end, double dt, int derivative, int64_t* counts,
                             const int64_t* offsets, double* out, double* sample_times,
                             unsigned flags);

/* Batched Trajectory::evaluateRange in ONE call (the samples' total is not known in advance):
 * counts[B] (samples per trajectory), offsets[B] (exclusive prefix sum of counts, in samples),
 * *total (the sum) and the samples out [total][D] (+ sample_times [total], nullable) -- all computed
 * on the device with no host round trip between them (the clock kernel also counts and scans; the
 * sample kernel adds the block offsets).  `capacity` is the number of sample rows out (and
 * sample_times) can hold.  If *total exceeds it, no sample is written and the call returns
 * MTG_ERR_TOO_LARGE after counts, offsets and *total are filled (retry with capacity = *total); with
 * MTG_FLAG_DEVICE_PTRS | MTG_FLAG_ASYNC the caller checks *total itself.  A safe capacity per
 * trajectory is min(t_end, sum T_i) / dt + 2 (samples are taken while the accumulated time is below
 * t_end and inside the trajectory), summed over the batch, with a little slack for the rounding of
 * the accumulated clock.  With MTG_FLAG_DEVICE_PTRS every array (and total) is a device pointer;
 * otherwise all are host pointers (the call then reads the total back once to size its staging). */
int mtg_evaluate_range_batch_full(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* coeffs,
                                  const double* times, double t_start, double t_end, double dt, int derivative,
                                  int64_t* counts, int64_t* offsets, int64_t* total, double* out,
                                  double* sample_times, int64_t capacity, unsigned flags);

/* mtg_evaluate_range_batch and mtg_evaluate_range_batch_full for a batch whose trajectories have
 * different segment counts, in the CSR layout of mtg_solve_linear_ragged_batch
 * (so[b] = sum_{j<b} seg_count[j], 64-bit):
 *   coeffs [so[b] .. so[b] + K_b][D][N], times [so[b] .. so[b] + K_b]   (as the ragged solve writes them)
 *   seg_count [B]: a HOST array also with MTG_FLAG_DEVICE_PTRS, read during the call and not kept
 *   counts, offsets, total, out, sample_times, capacity, the two-call protocol (out == NULL gives
 *   counts) and the one-call protocol: exactly those of the uniform entries
 *   t_start, t_end and dt are shared by the batch
 * Promise: counts[b], every byte of trajectory b's sample rows and every byte of its sample times equal
 * what mtg_evaluate_range_batch writes for that trajectory alone with K = K_b, whatever the order or
 * the composition of the batch -- the reference's accumulated clock and unfused Horner, bit for bit.
 * The CSR indirection is in the kernels: the segment offsets [B + 1] are computed on
 * the host and uploaded (8 (B + 1) bytes); no coefficient and no time is copied on the device.  A
 * host-pointer call stages the CSR arrays whole.  Two MTG_FLAG_ASYNC ragged calls of any kind on one
 * context, with different seg_count, may follow each other without a synchronisation between them.
 * The clock kernels take 32 trajectories per wave, whose times are one contiguous slice of `times`.
 * One rule, from seg_count alone, says where they read them: staged in LDS iff
 *   max over the blocks b0 = 0, 32, 64, ... of sum_{b0 <= b < min(b0 + 32, B)} K_b  <=  32 * 256,
 * otherwise from global memory.  For a full block of equal K this is the uniform call's rule K <= 256;
 * a staged trajectory may itself have K_b > 256.  The choice does not change a bit of the result.
 * The sample kernels (a block per trajectory) are picked, and their LDS sized, by the uniform call's
 * rule at K_max = max K_b.
 * Errors, all before any device work: those of the uniform calls on N, D, batch, derivative, dt and
 * capacity; MTG_ERR_INVALID_ARGUMENT for seg_count == NULL with batch > 0 (and for the required arrays,
 * as in the uniform calls); MTG_ERR_SIZE_MISMATCH for any seg_count[b] < 1.  When the sample kernels'
 * LDS at K_max does not fit (N = 10, D = 3: K_max > 250), a call that writes samples returns the
 * non-zero result of the uniform call at K = K_max (MTG_ERR_HIP, "invalid argument" in
 * mtg_last_error) and writes nothing; the count call (out == NULL) still succeeds, and the context
 * serves the next call.  batch == 0: MTG_OK (the one-call form sets *total = 0 when total is given).
 * A short capacity in the one-call form returns MTG_ERR_TOO_LARGE with counts, offsets and *total
 * filled and no sample written, as in the uniform call. */
int mtg_evaluate_range_ragged_batch(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count,
                                    const double* coeffs, const double* times, double t_start, double t_end,
                                    double dt, int derivative, int64_t* counts, const int64_t* offsets, double* out,
                                    double* sample_times, unsigned flags);
int mtg_evaluate_range_ragged_batch_full(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count,
                                         const double* coeffs, const double* times, double t_start, double t_end,
                                         double dt, int derivative, int64_t* counts, int64_t* offsets, int64_t* total,
                                         double* out, double* sample_times, int64_t capacity, unsigned flags);

/* Batched Trajectory::evaluate (src/trajectory.cpp:41-66) at caller-given query times, several
 * derivative orders from one pass over the coefficients (Polynomial::evaluate(t, VectorXd*),
 * polynomial.h:120-134, each order as polynomial.h:138-151).  The output shape is known in advance:
 * no counts, no offsets, no prefix sum.
 *   coeffs [B][K][D][N] (as the solve writes them), times [B][K]
 *   t_query: the time of trajectory b's query m is t_query[b * t_stride + m]; t_stride == 0 is one
 *            row of M times shared by the whole batch, otherwise t_stride >= M
 *   out [B][M][n_derivatives][D]: orders derivative_begin .. derivative_begin + n_derivatives - 1
 *   in_range_out [B][M] (nullable), status [B] (nullable: MTG_TRAJ_BAD_TIME)
 * Per trajectory b and query time t:
 *   segment    acc = 0; for i = 0 .. K-1: acc = fl(acc + T_i), stop at the first i with acc > t
 *              (sequential FP64 adds, trajectory.cpp:42-57).
 *   beyond     t > acc after the loop (+inf included): the row is all +0.0 and in_range = 0
 *              (trajectory.cpp:58-61; no message is printed).
 *   the end    the loop ran out and t > acc is false (t equals the accumulated total): the reference
 *              indexes one past the last segment; the last segment is used (i = K-1), in_range = 1.
 *   NaN        a NaN t gives a NaN row and in_range = 0.
 *   otherwise  in_range = 1, also for t < 0 (-inf included): the first segment is evaluated at a
 *              negative local time, as the reference does.
 *   local time tl = fl(t - fl(acc - T_i)), acc the value after adding T_i (trajectory.cpp:63-65);
 *              not simplified.
 *   value      order k >= N: +0.0.  Otherwise r = fl(base(k, N-1) c[N-1]); for j = N-2 .. k:
 *              r = fl(r tl), r = fl(r + fl(base(k, j) c[j])), base(k, j) = j!/(j-k)!
 *              (polynomial.h:138-151).  Multiply and add are separate roundings: no FMA, on the
 *              device or on the host, so both give the reference's bits.
 *   bad times  a trajectory with some T_i <= 0 or not finite: MTG_TRAJ_BAD_TIME, all its rows NaN
 *              and its in_range 0.
 * Errors: MTG_ERR_UNSUPPORTED_N; MTG_ERR_SIZE_MISMATCH (K < 1, D < 1, batch < 0, M < 0);
 * MTG_ERR_BAD_DERIVATIVE (derivative_begin < 0, n_derivatives outside 1..N);
 * MTG_ERR_INVALID_ARGUMENT (NULL ctx; t_stride < 0 or 0 < t_stride < M; coeffs, times, t_query or
 * out NULL with batch * M > 0); MTG_ERR_TOO_LARGE (a 64-thread block's rows exceed LDS:
 * n_derivatives * D > 128).  batch == 0 or M == 0: MTG_OK, nothing written.
 * Two kernels, picked from the shape alone (mtg_evaluate_at_path): a query's bits
 * depend neither on the kernel nor on the call it is part of. */
#define MTG_EVALUATE_AT_LANE 1         /* a lane per (trajectory, query): few queries per trajectory */
#define MTG_EVALUATE_AT_STAGED 2       /* a block per (trajectory, chunk of queries), coefficients in LDS */
int mtg_evaluate_at_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* coeffs,
                          const double* times, const double* t_query, int64_t t_stride, int64_t M,
                          int derivative_begin, int n_derivatives, double* out, uint8_t* in_range_out,
                          int32_t* status, unsigned flags);
/* The kernel (MTG_EVALUATE_AT_*) mtg_evaluate_at_batch runs for this shape -- staged iff
 * M >= max(32, K) and the staged block fits LDS -- or a negative MTG_ERR_*.  No device work. */
int mtg_evaluate_at_path(int N, int D, int K, int64_t M, int n_derivatives);

/* mtg_evaluate_at_batch for a batch whose trajectories have different segment counts, in the CSR
 * layout of mtg_solve_linear_ragged_batch (so[b] = sum_{j<b} seg_count[j], 64-bit):
 *   coeffs [so[b] .. so[b] + K_b][D][N], times [so[b] .. so[b] + K_b]   (as the ragged solve writes them)
 *   t_query, out [B][M][n_derivatives][D], in_range_out [B][M], status [B]: as in the uniform call
 *   seg_count [B]: a HOST array also with MTG_FLAG_DEVICE_PTRS, read during the call and not kept
 * Semantics: per trajectory and query exactly the text of mtg_evaluate_at_batch with K = K_b -- the
 * segment search, the beyond / end / NaN / negative-time rules, the unfused Horner, MTG_TRAJ_BAD_TIME
 * giving NaN rows -- so every output byte of trajectory b equals what mtg_evaluate_at_batch writes for
 * that trajectory alone, whatever the order of the batch.
 * The CSR indirection is in the kernels: the segment offsets [B + 1] are computed on
 * the host and uploaded (8 (B + 1) bytes), no coefficient is copied.  The mapping is
 * mtg_evaluate_at_ragged_path(N, D, max K_b, M, n_derivatives): one rule, from the shape alone.
 * Flags as in the uniform call; a host-pointer call stages the CSR arrays whole.  Two MTG_FLAG_ASYNC
 * ragged calls of any kind on one context, with different seg_count, may follow each other without a
 * synchronisation between them.
 * Errors, all before any device work: those of mtg_evaluate_at_batch on N, D, batch, M, t_stride and
 * the derivative arguments; MTG_ERR_INVALID_ARGUMENT for seg_count == NULL with batch > 0;
 * MTG_ERR_SIZE_MISMATCH for any seg_count[b] < 1.  batch == 0 or M == 0: MTG_OK, nothing written. */
int mtg_evaluate_at_ragged_batch(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count,
                                 const double* coeffs, const double* times, const double* t_query, int64_t t_stride,
                                 int64_t M, int derivative_begin, int n_derivatives, double* out,
                                 uint8_t* in_range_out, int32_t* status, unsigned flags);
/* The kernel (MTG_EVALUATE_AT_*) mtg_evaluate_at_ragged_batch runs for a batch whose largest segment
 * count is K_max: mtg_evaluate_at_path(N, D, K_max, M, n_derivatives).  No device work. */
int mtg_evaluate_at_ragged_path(int N, int D, int K_max, int64_t M, int n_derivatives);

/* Batched segment-time sweep (the nonlinear time-allocation objective,
 * polynomial_optimization_nonlinear_impl.h:765-832 via updateSegmentTimes +
 * solveLinear + computeCost): for each trajectory b and candidate c the
 * times are scale[c] * times[b][:] and the result is the optimal cost
 * J(b, c) (computeCost()).  cost_out [B][C]. */
int mtg_time_sweep_batch(mtg_ctx* ctx, int N, int D, int K, int derivative_to_optimize,
                         int64_t batch, const double* values, const uint8_t* fixed_mask,
                         const double* times, int n_candidates, const double* scales,
                         double* cost_out, int32_t* status, unsigned flags);

/* Cost (and gradient) of FIXED vertex derivatives at candidate segment times: the reference's
 * getCostAndGradientDerivative (polynomial_optimization_nonlinear_impl.h:1452-1520) evaluated at
 * perturbed times, as its numerical time gradient does (getCostAndGradientTime :2153-2238):
 *   J(b, c) = sum_dims d^T R(T_c) d   (no 1/2, unlike computeCost)
 *   grad(b, c, dim) = 2 (R(T_c) d)_free   (free derivatives in the reference (vertex, derivative)
 *                                          order; only with fixed_mask, entries >= n_free left 0)
 * with T_c[i] = times[b][i] * scales[c][i].  vertex_values [B][V][h][D] holds ALL derivatives of
 * every vertex (fixed values and the solved free ones, e.g. from free_out); fixed_mask [B][V] is
 * needed only for the gradient.  cost_out [B][C]; grad_out [B][C][D][V*h] (nullable). */
int mtg_cost_at_times_batch(mtg_ctx* ctx, int N, int D, int K, int derivative_to_optimize,
                            int64_t batch, const double* vertex_values, const uint8_t* fixed_mask,
                            const double* times, int n_candidates, const double* scales,
                            double* cost_out, double* grad_out, unsigned flags);

/* Segment-time sweep of the fixed-derivative cost with its time Jacobian (BASELINE config 5, the
 * matrix-core path).  Replaces, per trajectory b and candidate allocation c,
 *   updateSegmentTimes(T_c) + getCostAndGradientDerivative(NULL)      nl_impl:1452-1520
 * and the J_d part of getCostAndGradientTime's per-segment gradient    nl_impl:2153-2238
 * (dJd_dt; the collision, soft-constraint and w_* weighting terms are not part of this path; J_c is
 * mtg_collision_cost_batch and J_sc is mtg_soft_constraint_cost_batch):
 *   cost_out[b][c]      = sum_dims d^T R(T_c) d                 (as mtg_cost_at_times_batch)
 *   jac_out[b][c][i]    = dJ/dT_i at T_c                        (nullable)
 * with T_c[i] = times[b][i] * scales[c][i] and d = vertex_values[b] (ALL derivatives of every
 * vertex, fixed and solved free ones).  increment_time == 0 gives the exact derivative;
 * increment_time > 0 gives the reference's central difference
 *   (J(T_i + dt) - J(T_i - dt)) / (2 dt), both perturbed times 0.1 when T_i <= 0.1
 * (nl_impl:2180-2223; the reference default is increment_time = 0.1,
 * polynomial_optimization_nonlinear.h:67); NaN where T_i - dt <= 0 (the reference CHECK-fails).
 * Works for any n_candidates >= 1; per-call LDS limits the shape (MTG_ERR_TOO_LARGE). */
int mtg_time_jacobian_batch(mtg_ctx* ctx, int N, int D, int K, int derivative_to_optimize,
                            int64_t batch, const double* vertex_values, const double* times,
                            int n_candidates, const double* scales, double increment_time,
                            double* cost_out, double* jac_out, unsigned flags);

/* Coefficients from ALL vertex derivatives (fixed and free), nothing solved: per trajectory the
 * reference's setFreeConstraints (polynomial_optimization_linear.h:185-186) followed by
 * updateSegmentsFromCompactConstraints (lin_impl:253-273), c_i = A(T_i)^-1 [x_i; x_{i+1}].
 * vertex_values [B][V][h][D], times [B][K] (> 0) -> coeffs [B][K][D][N].
 * Shape limit: a block stages whole trajectories in LDS, 8 * ((K+1)*h*D + K + K*D*N) bytes each, and
 * needs room for two of them in 48 KiB; otherwise MTG_ERR_TOO_LARGE (nothing is written).  At D = 3 that
 * is K <= 66 for N = 10 and K <= 55 for N = 12: the long chains (K = 100) are outside this entry
 * (mtg_host_coefficients_from_vertices_batch has no such limit). */
int mtg_coefficients_from_vertices_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch,
                                         const double* vertex_values, const double* times, double* coeffs,
                                         unsigned flags);

/* Vertex derivatives of solved trajectories: the reference's M^+ A p
 * (polynomial_optimization_nonlinear_impl.h:162-180, computeInitialSolutionWithoutPositionConstraints;
 * getA / getMpinv, polynomial_optimization_linear.h:209-214): derivative k < h of every segment end,
 * averaged over the two segment ends meeting at an interior vertex.
 * coeffs [B][K][D][N], times [B][K] -> vertex_values [B][V][h][D].
 * Shape limit: that of mtg_coefficients_from_vertices_batch (two trajectories of
 * 8 * ((K+1)*h*D + K + K*D*N) bytes in 48 KiB of LDS, else MTG_ERR_TOO_LARGE; D = 3: K <= 66 for N = 10,
 * K <= 55 for N = 12), so the long chains (K = 100) are outside this entry too. */
int mtg_vertex_derivatives_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* coeffs,
                                 const double* times, double* vertex_values, unsigned flags);

/* The two maps for a batch whose trajectories have different segment counts, on the CSR layout of
 * mtg_solve_linear_ragged_batch: K_b = seg_count[b] >= 1, V_b = K_b + 1, so[b] = sum_{j<b} K_j,
 * vo[b] = so[b] + b (both 64-bit).  seg_count [B] is a host array, also with MTG_FLAG_DEVICE_PTRS.
 *   mtg_coefficients_from_vertices_ragged_batch  (setFreeConstraints,
 *       polynomial_optimization_linear.h:185-186, + updateSegmentsFromCompactConstraints, lin_impl:253-273)
 *       vertex_values [vo[b] .. vo[b]+V_b][h][D], times [so[b] .. so[b]+K_b] -> coeffs [so[b] .. so[b]+K_b][D][N]
 *   mtg_vertex_derivatives_ragged_batch  (M^+ A p, nl_impl:162-180)
 *       coeffs, times as above -> vertex_values: the mean of the two segment ends at an interior vertex,
 *       the single end at the first or last vertex of its trajectory.
 * Every output byte of trajectory b equals what the uniform entry writes for that trajectory alone,
 * where the uniform entry accepts that K.  There is no limit on K: a block owns a fixed tile of
 * mtg_vertex_ragged_tile(N, D) consecutive packed segments, whatever trajectory borders fall inside
 * it, so its LDS use depends on N and D only and a K = 100 chain goes through.  MTG_ERR_TOO_LARGE only
 * where not even one segment's arrays fit the staging (a D in the hundreds).
 * Errors, all raised before any device work: those of the uniform calls on N, D and batch;
 * MTG_ERR_INVALID_ARGUMENT for seg_count == NULL with batch > 0; MTG_ERR_SIZE_MISMATCH for a
 * seg_count[b] < 1.  batch == 0 returns MTG_OK.  Flags: MTG_FLAG_DEVICE_PTRS, MTG_FLAG_ASYNC; two
 * MTG_FLAG_ASYNC ragged calls of any kind may follow each other on one context. */
int mtg_coefficients_from_vertices_ragged_batch(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count,
                                                const double* vertex_values, const double* times, double* coeffs,
                                                unsigned flags);
int mtg_vertex_derivatives_ragged_batch(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count,
                                        const double* coeffs, const double* times, double* vertex_values,
                                        unsigned flags);
/* Packed segments per block of the two entries above (> 0), or MTG_ERR_UNSUPPORTED_N,
 * MTG_ERR_SIZE_MISMATCH (D < 1), MTG_ERR_TOO_LARGE.  For tests and tools. */
int mtg_vertex_ragged_tile(int N, int D);

/* Extremum of a trajectory (the reference's Extremum, extremum.h): segment-local time, value and
 * segment index. */
typedef struct mtg_extremum {
  double time;
  double value;
  int32_t segment;
  int32_t reserved;
} mtg_extremum;

/* Minimum and maximum magnitude of derivative `derivative` (0 <= derivative <= N-2) over each
 * whole trajectory: Trajectory::computeMinMaxMagnitude (src/trajectory.cpp:181-218) with the
 * dimensions in dimension_mask (bit d = dimension d; 0 = all).  Per segment the candidates are
 * t = 0, t = T and the real roots in [0, T] of sum_d conv(p_d^(k), p_d^(k+1)) (one dimension: of
 * p^(k+1)), src/segment.cpp:82-196.  coeffs [B][K][D][N], times [B][K]; minimum / maximum [B]
 * (either may be NULL).  Roots are isolated on 256 samples per segment and refined to a few ulp
 * (the reference uses Jenkins-Traub, src/rpoly.cpp); see DESIGN.md. */
int mtg_min_max_magnitude_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* coeffs,
                                const double* times, int derivative, uint32_t dimension_mask,
                                mtg_extremum* minimum, mtg_extremum* maximum, unsigned flags);

/* mtg_min_max_magnitude_batch for a batch whose trajectories have different segment counts, in the
 * CSR layout of mtg_solve_linear_ragged_batch: coeffs [so[b] .. so[b] + K_b][D][N],
 * times [so[b] .. so[b] + K_b], minimum / maximum [B] (either may be NULL); seg_count [B] is a HOST
 * array also with MTG_FLAG_DEVICE_PTRS.  Every output byte of trajectory b equals what
 * mtg_min_max_magnitude_batch writes for that trajectory alone.
 * The extrema kernel's rounding order depends on the block geometry its launcher derives from K, so
 * this entry follows the ragged solve: the same host-side plan; a K-group that is one
 * run of the batch goes through the uniform launcher in place, on slices of the caller's arrays; the
 * coefficients and times of every other group are gathered into packed arrays by one kernel, the
 * uniform launcher runs there, and one kernel moves the results to minimum[b] / maximum[b].  One
 * launch per group in ascending K, one stream, no host synchronisation in between; a batch sorted by
 * K copies nothing.
 * Errors, all before any device work: those of the uniform call on N, D, batch, derivative and
 * dimension_mask; MTG_ERR_INVALID_ARGUMENT for seg_count == NULL with batch > 0;
 * MTG_ERR_SIZE_MISMATCH for any seg_count[b] < 1; MTG_ERR_TOO_LARGE for any seg_count[b] > 256.
 * batch == 0: MTG_OK. */
int mtg_min_max_magnitude_ragged_batch(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count,
                                       const double* coeffs, const double* times, int derivative,
                                       uint32_t dimension_mask, mtg_extremum* minimum, mtg_extremum* maximum,
                                       unsigned flags);

/* Per-segment extrema on a time window, with the candidate list: the layer under
 * Trajectory::computeMinMaxMagnitude.  A call has no trajectory structure -- coeffs [S][D][N],
 * times [S] -- so a uniform batch (S = B K) and a CSR-packed ragged batch (S = sum K_b) are the same
 * call: no plan, no gather, no indirection.  A segment's outputs depend only on that segment's inputs,
 * not on S or on its index.
 *
 * mtg_segment_min_max_magnitude_batch: Segment::computeMinMaxMagnitudeCandidates followed by
 * selectMinMaxMagnitudeFromCandidates (src/segment.cpp:82-196) on [t_start, t_end].  The candidates
 * are t_start, t_end, then the real roots in the window of sum_{d in mask} conv(p_d^(k), p_d^(k+1))
 * (one selected dimension: of p^(k+1)); the quantity is sqrt(sum_d p_d^(k)(t)^2); the first candidate
 * in that order wins ties (std::max / std::min keep their first argument, segment.cpp:177-194).
 * minimum / maximum [S], candidate_times [S][candidate_capacity], candidate_count [S].
 *
 * mtg_segment_min_max_axis_batch: Polynomial::computeMinMax (src/polynomial.cpp:97-138) for every
 * (segment, dimension): the candidates are t_start, t_end and the real roots in the window of
 * p_d^(k+1); the quantity is the SIGNED p_d^(k)(t); the comparisons are strict, so the first candidate
 * wins ties (polynomial.cpp:126-136).  minimum / maximum [S][D], candidate_times
 * [S][D][candidate_capacity], candidate_count [S][D].
 *
 * Common to both:
 *   windows [S][2] = t_start, t_end, segment-local; NULL: [0, times[s]] (times may be NULL when windows
 *     is given: it is not read).  The window is not clamped to [0, T]; the reference does not clamp it.
 *   mtg_extremum.time is segment-local; .segment is 0, as Extremum(t, v, 0) leaves it.
 *   Roots: the project's search, not Jenkins-Traub -- sign changes (and exact zeros) of the root
 *     polynomial on the 257 samples t_start + s h, h = (t_end - t_start) / 256, the last sample t_end
 *     itself, each bracket refined by the safeguarded Newton-bisection.  A root pair closer than h with
 *     no sign change between samples is not isolated.  On [0, T] the per-segment
 *     extremes are the values mtg_min_max_magnitude_batch reduces over a trajectory, bit for bit.
 *   candidate_times lists t_start, t_end, then the isolated roots in ascending order; a root that
 *     coincides with an end is listed as well.  candidate_count is the true count also when it exceeds
 *     candidate_capacity; only the first candidate_capacity times are written and the rest of a row is
 *     +0.0.  When every coefficient of the root polynomial is exactly zero (an axis held constant) the
 *     list is the two ends and the count 2 (the reference's root finder returns no roots for the zero
 *     polynomial, rpoly.cpp:62-65), while the min / max search stays the shared code's, which sees a
 *     zero at every sample.
 *   status [S]: MTG_TRAJ_BAD_TIME when the window is not finite, when t_start > t_end (the reference
 *     returns false), or when there is no window and times[s] is not positive and finite.  Every floating
 *     output of such a segment is NaN (its candidate rows included) and its counts are 0.
 *   Every output pointer is nullable, and requesting one output never changes the bits of another.
 * Errors: N, D, derivative (0 .. N-2) and dimension_mask (0 = all; a bit >= D: MTG_ERR_INVALID_ARGUMENT)
 * as in mtg_min_max_magnitude_batch; MTG_ERR_SIZE_MISMATCH for n_segments < 0;
 * MTG_ERR_INVALID_ARGUMENT for candidate_times with candidate_capacity < 2 and for a NULL ctx, coeffs,
 * or times and windows both NULL with n_segments > 0.  n_segments == 0: MTG_OK.  MTG_FLAG_DEVICE_PTRS
 * and MTG_FLAG_ASYNC as in the collision entries; a host-pointer call stages its arrays once. */
int mtg_segment_min_max_magnitude_batch(mtg_ctx* ctx, int N, int D, int64_t n_segments, const double* coeffs,
                                        const double* times, const double* windows, int derivative,
                                        uint32_t dimension_mask, mtg_extremum* minimum, mtg_extremum* maximum,
                                        double* candidate_times, int32_t* candidate_count, int candidate_capacity,
                                        int32_t* status, unsigned flags);
int mtg_segment_min_max_axis_batch(mtg_ctx* ctx, int N, int D, int64_t n_segments, const double* coeffs,
                                   const double* times, const double* windows, int derivative, mtg_extremum* minimum,
                                   mtg_extremum* maximum, double* candidate_times, int32_t* candidate_count,
                                   int candidate_capacity, int32_t* status, unsigned flags);

/* ---- Collision term of the nonlinear objective (kOptimizeFreeConstraintsAndCollision[AndTime]).
 *
 * The map.  The reference reads distances through esdf / sdf_tools, which are not part of its tree;
 * this ABI takes a dense grid of signed distances instead:
 *   cell of p            i = floor((p - origin) / resolution) per axis
 *   centre of cell i     origin + (i + 0.5) * resolution
 *   nearest-cell lookup  distance[cell of p], or oob_distance when an index is outside the grid
 *                        (stands for getDistanceInMetricUnits / Get)
 *   continuous lookup    getDistanceSDF (nl_impl:1846-1904): the eight cells at index +-1 on every
 *                        axis around the cell of p (a stencil two cells wide, getNeighborsSDF
 *                        :1808-1843), their centres as corner positions, combined by triLerp exactly
 *                        as written (:2436-2464); the nearest-cell value when a corner cell is
 *                        outside the grid. */
typedef struct mtg_sdf_grid {
  const float* distance;   /* [nx][ny][nz], z fastest; host or device pointer as the call's flags say */
  int32_t nx, ny, nz;
  double origin[3];        /* metric position of the low corner of cell (0,0,0) */
  double resolution;       /* cell edge, > 0 */
  double oob_distance;     /* value returned for a cell outside the grid */
} mtg_sdf_grid;

/* The reference's optimization_parameters_ fields the collision term reads. */
typedef struct mtg_collision_params {
  double coll_check_time_increment;  /* dt of the sample clock, > 0 */
  double map_resolution;             /* arc-length gate, bounds margin and finite-difference increment,
                                        >= 0; separate from grid.resolution */
  double epsilon;                    /* width of the quadratic band of the potential */
  double robot_radius;
  double coll_pot_multiplier;
  double min_bound[3], max_bound[3];
  int32_t use_continuous_distance;   /* use_continous_distance: the continuous lookup inside the bounds */
  int32_t reserved;
} mtg_collision_params;

/* Batched getCostAndGradientCollision (nl_impl:1523-1709) with getCostAndGradientPotentialESDF
 * (:1713-1806), getDistanceSDF and getCostPotential (:2319-2343), restated exactly.  D must be 3 and
 * N one of 6, 8, 10, 12; any K >= 1.  Per trajectory, with time_sum = -1, dist_sum = 0:
 *   for each segment i: for (t = 0; t < T_i; t += dt)      (the accumulated clock, not j * dt)
 *     position and velocity of the three axes at t;
 *     time_sum < 0: time_sum = 0, prev_pos = pos, next sample;
 *     time_sum += dt, dist_sum += |pos - prev_pos|, prev_pos = pos;
 *     dist_sum < map_resolution: next sample;
 *     c, grad c = potential and its central differences at pos (increment map_resolution);
 *     J += c |vel| time_sum;  the gradient below only if |vel| > 1e-6;  dist_sum = time_sum = 0
 *   after the segment: time_sum += -dt + (T_i - t)   (t: the first clock value not below T_i; this
 *     can leave time_sum in (-dt, 0], and the next sample then takes the first-entry branch again)
 * Potential of d = distance - robot_radius: d <= 0: coll_pot_multiplier (-d) + epsilon / 2 and the
 * trajectory's collision flag is set; d <= epsilon: (d - epsilon)^2 / (2 epsilon); else 0.  The
 * continuous lookup is used when use_continuous_distance is set and every axis of pos lies in
 * [min_bound + map_resolution, max_bound - map_resolution], the nearest-cell lookup otherwise.
 * Gradient (paper eq. 14, nl_impl:1671-1687): a sample of segment i adds, per axis k, to that
 * segment's coefficient-space vector
 *   |vel| time_sum (grad c)_k [t^n] + time_sum c vel_k / |vel| [n t^(n-1)],   n = 0 .. N-1,
 * and the reference's product with L_pp is A(T_i)^-T applied to it, top half to vertex i, bottom
 * half to vertex i + 1 (summed at an interior vertex), free derivatives in the reference's
 * (vertex, derivative) order: the packing of mtg_cost_at_times_batch's grad_out, so the two add.
 * map_resolution == 0 divides by zero in the central differences, as in the reference (NaN gradient).
 *
 * vertex_values [B][V][h][D] holds ALL derivatives; the coefficients are formed from them as
 * mtg_coefficients_from_vertices_batch does.  fixed_mask [B][V] is needed only for grad_out.
 * cost_out [B]; grad_out [B][D][V*h] (nullable; entries >= n_free are 0); collision_out [B]
 * (nullable); n_evaluated_out [B] (nullable): samples that reached the potential; status [B]
 * (nullable).  A trajectory with a T_i that is not positive and finite, or with more than 2^24 clock
 * samples in a segment (T_i / dt), gets MTG_TRAJ_BAD_TIME, a NaN cost and a zero gradient.
 * MTG_ERR_INVALID_ARGUMENT: D != 3, dt <= 0, map_resolution < 0, grid resolution <= 0, a grid
 * dimension < 1.  With MTG_FLAG_DEVICE_PTRS grid->distance is a device pointer too (grid and params
 * themselves are always host structs, read during the call); a host-pointer call stages the grid
 * once per call.  Results do not depend on the trajectory's place in the batch or on the batch. */
int mtg_collision_cost_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* vertex_values,
                             const uint8_t* fixed_mask, const double* times, const mtg_sdf_grid* grid,
                             const mtg_collision_params* params, double* cost_out, double* grad_out,
                             uint8_t* collision_out, int32_t* n_evaluated_out, int32_t* status, unsigned flags);

/* Host (CPU) path of mtg_collision_cost_batch, no context and no GPU needed: the loop above in
 * scalar C++ in the reference's order, on the calling thread(s).  The C++ drop-in uses it for single
 * trajectories.  All host pointers; threads <= 0: mtg_host_default_threads(). */
int mtg_host_collision_cost_batch(int N, int D, int K, int64_t batch, const double* vertex_values,
                                  const uint8_t* fixed_mask, const double* times, const mtg_sdf_grid* grid,
                                  const mtg_collision_params* params, double* cost_out, double* grad_out,
                                  uint8_t* collision_out, int32_t* n_evaluated_out, int32_t* status, int threads);

/* getCostAndGradientCollision (nl_impl:1523-1709) for a batch whose trajectories have different
 * segment counts: J_c, its gradient and the is_collision flag of every candidate in one call, on the
 * CSR layout of mtg_solve_linear_ragged_batch (K_b = seg_count[b] >= 1, V_b = K_b + 1,
 * so[b] = sum_{j<b} K_j, vo[b] = so[b] + b; seg_count [B] is a host array, also with
 * MTG_FLAG_DEVICE_PTRS).  vertex_values [vo[b] .. vo[b]+V_b][h][3] and fixed_mask [vo[b] ..] are
 * indexed at vo[b], times at so[b]; cost_out, collision_out, n_evaluated_out and status are [B];
 * grad_out is the block [3][V_b h] at double offset 3 h vo[b] -- the layout of the ragged solve's
 * free_out, so the two add -- and is zeroed by the call.  Semantics, nullable outputs, per-trajectory
 * status, flags and grid staging are those of mtg_collision_cost_batch, and every output byte of
 * trajectory b equals what that entry writes for the trajectory alone.
 * One launch of B one-wave blocks whose LDS is sized for the largest K_b: MTG_ERR_TOO_LARGE, before
 * any device work, when that exceeds 64 KiB (N = 10: K_max > 172).  A batch holding one long chain
 * therefore runs its short trajectories at the long chain's occupancy.
 * Errors: those of mtg_collision_cost_batch (D != 3, dt <= 0, ...); MTG_ERR_INVALID_ARGUMENT for
 * seg_count == NULL with batch > 0; MTG_ERR_SIZE_MISMATCH for a seg_count[b] < 1.  batch == 0 returns
 * MTG_OK.  Two MTG_FLAG_ASYNC ragged calls of any kind may follow each other on one context. */
int mtg_collision_cost_ragged_batch(mtg_ctx* ctx, int N, int D, int64_t batch, const int32_t* seg_count,
                                    const double* vertex_values, const uint8_t* fixed_mask, const double* times,
                                    const mtg_sdf_grid* grid, const mtg_collision_params* params, double* cost_out,
                                    double* grad_out, uint8_t* collision_out, int32_t* n_evaluated_out, int32_t* status,
                                    unsigned flags);

/* Host (CPU) path of mtg_collision_cost_ragged_batch: the per-trajectory code of
 * mtg_host_collision_cost_batch on each trajectory's blocks of the CSR arrays, threaded over
 * trajectories; a trajectory's bytes are those of that entry with batch 1. */
int mtg_host_collision_cost_ragged_batch(int N, int D, int64_t batch, const int32_t* seg_count,
                                         const double* vertex_values, const uint8_t* fixed_mask, const double* times,
                                         const mtg_sdf_grid* grid, const mtg_collision_params* params, double* cost_out,
                                         double* grad_out, uint8_t* collision_out, int32_t* n_evaluated_out,
                                         int32_t* status, int threads);

/* Segment-time gradient of the collision cost: the dJc_dt part of getCostAndGradientTime
 * (nl_impl:2155-2243), the central difference of J_c in each segment time, restated as the reference
 * is written.  D must be 3, N one of 6, 8, 10, 12, K >= 1 up to the LDS limit below.
 *
 * The stale L_.  getCostAndGradientTime perturbs a segment time with updateSegmentTimes, which
 * rebuilds cost_matrices_ and inverse_mapping_matrices_ but does NOT recompute L_: that member is
 * assigned only at the top of the objective (:1197-1200) and in the optimize* set-ups.
 * getCostAndGradientCollision forms its coefficients as L_ * d (:1558) and reads its loop bounds from
 * getSegmentTimes (:1563).  So the perturbed evaluations walk the UNPERTURBED polynomials to a
 * perturbed end time -- which is why this gradient cannot be composed from mtg_collision_cost_batch
 * (it re-forms the coefficients from the times it is given).  Per trajectory:
 *   c_i = A(T_i)^-1 [x_i; x_{i+1}] from `times`, exactly the coefficients of mtg_collision_cost_batch;
 *   for each segment n and side s (0 = smaller, evaluated first; 1 = bigger) the times T' are
 *     T'[i] = T[i] for i != n;  T'[n] = 0.1 on BOTH sides if T[n] <= 0.1 (the reference's literal 0.1,
 *     whatever increment_time is), else T[n] - increment_time (s = 0), T[n] + increment_time (s = 1);
 *   J_c(n, s) = the loop documented at mtg_collision_cost_batch with those coefficients, the clock
 *     bound t < T'[i] and the end-of-segment correction time_sum += -dt + (T'[i] - t); the bigger
 *     side evaluates segment n's polynomial past T[n];
 *   grad_t[n] = (J_c(n, 1) - J_c(n, 0)) / (2 increment_time).
 * T[n] <= 0.1 makes the two walks identical and grad_t[n] exactly +0.0.  T[n] > 0.1 with
 * T[n] - increment_time <= 0: the reference CHECK-fails in updateSegmentTimes; grad_t[n] and both side
 * costs are NaN and both side counts 0, for that n only (the rule of mtg_time_jacobian_batch).
 * MTG_TRAJ_BAD_TIME: some T[i] is not positive and finite, or a perturbed time of some segment has
 * more than 2^24 clock samples ((T[i] + increment_time) / dt, and 0.1 / dt where T[i] <= 0.1); then
 * every output of the trajectory is NaN and its counts are 0.
 * MTG_ERR_INVALID_ARGUMENT: increment_time not > 0 and finite (a deviation: the reference would
 * divide by zero), and the argument errors of mtg_collision_cost_batch.
 *
 * vertex_values [B][V][h][3] (ALL derivatives), times [B][K]; grad_t_out [B][K]; side_cost_out
 * [B][K][2] (nullable): J_c(n, s); side_evaluated_out [B][K][2] (nullable): the samples of that walk
 * that reached the potential; status [B] (nullable).  Flags and grid staging as
 * mtg_collision_cost_batch (MTG_FLAG_DEVICE_PTRS, MTG_FLAG_ASYNC).  The nullable outputs do not change
 * grad_t_out's bits, and results do not depend on the trajectory's place in the batch or on the batch.
 *
 * segments_walked_out [B] (nullable, device call only) is a diagnostic of how the kernel avoids 2K
 * complete walks.  It first walks the unperturbed trajectory once (not counted) and records, at the
 * entry of every segment m, the loop state (time_sum, dist_sum) and the cost and sample count of the
 * segments before and from m.  The walk of (n, s) starts from the recorded entry of segment n (the
 * segments before n are untouched), walks segment n to T'[n] and continues with n+1, n+2, ...  At the
 * entry of each segment m >= n+2 -- where prev_pos is the last sample of the unperturbed segment m-1
 * in both walks -- it compares its (time_sum, dist_sum) BIT FOR BIT with the recorded pair: if both
 * are equal the rest of the walk is the unperturbed one, the recorded sums from m on are added and the
 * walk stops, having walked m - n segments; if they are never equal it walks to the end (K - n
 * segments).  segments_walked_out[b] is the sum of those counts over the 2K perturbations (0 for a
 * perturbation under the NaN rule and for a BAD_TIME trajectory): a function of the inputs alone.
 * When every perturbation rejoins at n+2 it is 4K - 2.
 * MTG_ERR_TOO_LARGE: the device call keeps one trajectory (vertex values, coefficients, records) in
 * 64 KiB of LDS: K <= 204 (N = 6), 166 (8), 140 (10), 121 (12).  The host path has no such limit.
 * Not covered: the variant that re-forms the coefficients at the perturbed times (what a recomputed
 * L_ would give); no semantics is invented for it here. */
int mtg_collision_time_gradient_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* vertex_values,
                                      const double* times, const mtg_sdf_grid* grid, const mtg_collision_params* params,
                                      double increment_time, double* grad_t_out, double* side_cost_out,
                                      int32_t* side_evaluated_out, int32_t* segments_walked_out, int32_t* status,
                                      unsigned flags);

/* Host (CPU) path of mtg_collision_time_gradient_batch, no context and no GPU needed: the reference
 * written literally, 2K complete walks per trajectory in the reference's order, in scalar C++ on the
 * calling thread(s).  The C++ drop-in uses it for single trajectories.  All host pointers;
 * threads <= 0: mtg_host_default_threads(). */
int mtg_host_collision_time_gradient_batch(int N, int D, int K, int64_t batch, const double* vertex_values,
                                           const double* times, const mtg_sdf_grid* grid,
                                           const mtg_collision_params* params, double increment_time,
                                           double* grad_t_out, double* side_cost_out, int32_t* side_evaluated_out,
                                           int32_t* status, int threads);

/* ---- Soft-constraint term of the nonlinear objective (use_soft_constraints, the reference's default,
 * polynomial_optimization_nonlinear.h:57): the magnitude limits added with
 * addMaximumMagnitudeConstraint, as a cost. */
typedef struct mtg_soft_constraint_params {
  int32_t n_constraints;      /* 1 .. 8 (inequality_constraints_, addMaximumMagnitudeConstraint) */
  int32_t derivative[8];      /* 0 .. min(4, N-2): POSITION .. SNAP, the reference's switch nl_impl:2356-2386 */
  double  limit[8];           /* ConstraintData::value, > 0 */
  double  weight;             /* soft_constraint_weight (reference default 100) */
  double  maximum_cost;       /* reference default 1e12 */
  double  increment;          /* the reference's map_resolution: finite-difference step */
} mtg_soft_constraint_params;

/* Batched getCostAndGradientSoftConstraints (nl_impl:2025-2091) with
 * evaluateMaximumMagnitudeAsSoftConstraint (:2396-2425) and
 * PolynomialOptimization::computeMaximumOfMagnitude (lin_impl:470-503), restated.  1 <= D <= 4, N one
 * of 6, 8, 10, 12, K >= 1 up to the LDS limit below.  Per trajectory:
 *   cost = sum_c min(maximum_cost, exp(weight * (max_c - limit_c) / limit_c))    (in constraint order)
 *   max_c = computeMaximumOfMagnitude<derivative_c>: the candidates are, per segment in order, t = 0
 *     and then the real roots in [0, T_i] of sum_d conv(p_d^(k), p_d^(k+1)) (D = 1: of p^(k+1)), and
 *     after the last segment t = T_K.  A candidate replaces the best so far only when strictly larger
 *     (the first one wins ties).  Interior segment ends are NOT candidates -- the difference from
 *     Trajectory::computeMinMaxMagnitude / mtg_min_max_magnitude_batch.  Roots are isolated and refined
 *     exactly as there (256 samples per segment, safeguarded Newton).
 *   grad[d][n] = (cost(x + increment e_{d,n}) - cost(x - increment e_{d,n})) / (2 increment) for
 *     dimension d and free index n (the reference's central difference, left side evaluated first);
 *     increment == 0 divides 0 by 0, as in the reference (a NaN gradient, a finite cost).
 * vertex_values [B][V][h][D] holds ALL derivatives; the coefficients are formed from them as
 * mtg_coefficients_from_vertices_batch does.  fixed_mask [B][V] is needed only for grad_out.
 * cost_out [B]; grad_out [B][D][V*h] (nullable; free derivatives in the reference's (vertex,
 * derivative) order, entries >= n_free are 0: the packing of mtg_cost_at_times_batch and
 * mtg_collision_cost_batch, so the three terms add); maxima_out [B][n_constraints] (nullable): the
 * unperturbed trajectory's optimization_info_.maxima; status [B] (nullable).  grad_out == NULL skips
 * the gradient and leaves the cost's bits unchanged.  A trajectory with a T_i that is not positive and
 * finite gets MTG_TRAJ_BAD_TIME, a NaN cost (and NaN maxima) and a zero gradient.
 * MTG_ERR_INVALID_ARGUMENT: D outside 1..4; N not in {6, 8, 10, 12}; n_constraints outside 1..8; a
 * derivative outside 0..min(4, N-2) or a limit that is not > 0 (a deviation: the reference returns a
 * zero violation for a derivative its switch does not know).  params is a host struct, read during
 * the call.  Results do not depend on the trajectory's place in the batch or on the batch.
 * MTG_ERR_TOO_LARGE: the device call keeps one trajectory (vertex values, coefficients, per-segment
 * maxima) and at least eight search areas in 64 KiB of LDS, which bounds K -- with two constraints
 * K <= 189 (N = 6), 148 (8), 120 (10), 100 (12) at D = 3; 92 at N = 10, D = 4; 264 at N = 10, D = 1;
 * eight constraints: K <= 79 at N = 10, D = 3 -- unlike mtg_min_max_magnitude_batch, which streams
 * segments and takes K <= 256.  The host path has no such limit.
 * Not covered: the soft-constraint part of getCostAndGradientTime (nl_impl:2199-2226).  As read,
 * updateSegmentTimes does not rebuild segments_, so the reference's dJsc_dt differences two equal
 * numbers; no semantics is invented for it here. */
int mtg_soft_constraint_cost_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* vertex_values,
                                   const uint8_t* fixed_mask, const double* times,
                                   const mtg_soft_constraint_params* params, double* cost_out, double* grad_out,
                                   mtg_extremum* maxima_out, int32_t* status, unsigned flags);

/* Host (CPU) path of mtg_soft_constraint_cost_batch, no context and no GPU needed: the reference's
 * loop written literally -- for every (dimension, free index, side) ALL coefficients are re-formed and
 * ALL segments searched.  All host pointers; threads <= 0: mtg_host_default_threads(). */
int mtg_host_soft_constraint_cost_batch(int N, int D, int K, int64_t batch, const double* vertex_values,
                                        const uint8_t* fixed_mask, const double* times,
                                        const mtg_soft_constraint_params* params, double* cost_out,
                                        double* grad_out, mtg_extremum* maxima_out, int32_t* status, int threads);

/* ---- The nonlinear objective in the optimiser's variables: what nlopt calls once per iteration in
 * PolynomialOptimizationNonLinear<N> (nl_impl:909-1449), one cost and one gradient per trajectory,
 * composed on the device from the five entry points above. */
#define MTG_OBJECTIVE_FREE_CONSTRAINTS 0                        /* objectiveFunctionFreeConstraints, nl_impl:909-1000 */
#define MTG_OBJECTIVE_FREE_CONSTRAINTS_AND_COLLISION 1          /* ...AndCollision, nl_impl:1003-1156 */
#define MTG_OBJECTIVE_FREE_CONSTRAINTS_AND_COLLISION_AND_TIME 2 /* ...AndCollisionAndTime, nl_impl:1159-1449 */
/* The two gradient-free objectives (objectiveFunctionTime, objectiveFunctionTimeAndConstraints) are
 * values of mtg_objective_time_params.objective (mtg_objective_time_batch, below); mtg_objective_batch
 * rejects them with MTG_ERR_INVALID_ARGUMENT.  Not covered anywhere: the reference's numerical-gradient
 * switches, bits of mtg_objective_params.reserved (any non-zero `reserved` is rejected). */
#define MTG_OBJECTIVE_TIME 3                                    /* objectiveFunctionTime, nl_impl:765-832 */
#define MTG_OBJECTIVE_TIME_AND_CONSTRAINTS 4                    /* ...TimeAndConstraints, nl_impl:835-906 */
#define MTG_OBJECTIVE_USE_NUMERIC_GRAD 1                        /* use_numeric_grad: not covered */
#define MTG_OBJECTIVE_SIMPLE_NUMGRAD_TIME 2                     /* is_simple_numgrad_time: not covered */
#define MTG_OBJECTIVE_SIMPLE_NUMGRAD_CONSTRAINTS 4              /* is_simple_numgrad_constraints: not covered */

typedef struct mtg_objective_params {
  int32_t objective;                /* MTG_OBJECTIVE_* */
  int32_t derivative_to_optimize;
  double  w_d, w_c, w_t, w_sc;      /* reference defaults 0.1, 10, 1, 1 */
  double  increment_time;           /* reference default 0.1; used by objective 2 only */
  int32_t use_soft_constraints;     /* reference default true */
  int32_t is_collision_safe;        /* objective 2 only */
  int32_t is_coll_raise_first_iter; /* objective 2 only */
  int32_t reserved;                 /* must be 0 (see the not-covered switches above) */
  double  add_coll_raise;
} mtg_objective_params;

/* optimization_info_ + total_cost_iter0_ + is_iter0_ of one problem; all-zero bytes = a fresh optimisation */
typedef struct mtg_objective_state {
  double  total_cost_iter0;
  double  cost_trajectory, cost_collision, cost_time, cost_soft_constraints;
  int32_t n_iterations;
  int32_t iter0_done;
} mtg_objective_state;

/* The unweighted parts, exactly as the component entry points return them (also for a trajectory
 * with an error status: the NaN rule below applies to the objective's own outputs only).  Every
 * pointer is nullable; a gradient part is filled only when grad_out is given and the objective uses it. */
typedef struct mtg_objective_parts {
  double *J_d, *J_c, *J_sc, *J_t;       /* [B] */
  double *dJd_dt, *dJc_dt;              /* [B][K]       (objective 2) */
  double *grad_d, *grad_c, *grad_sc;    /* [B][D][V*h], the packing of mtg_cost_at_times_batch */
} mtg_objective_parts;

/* One evaluation of the objective per trajectory.  values / fixed_mask are the problem as
 * mtg_solve_linear_batch reads it; row b of x [B][x_stride] is the vector nlopt sees:
 *   objective 2: the K segment times first (objectives 0 and 1 have none and read `times` [B][K];
 *                objective 2 takes times == NULL),
 *   then D blocks of n_free[b] free derivatives in the reference's (vertex, derivative) order;
 *   n_free[b] = the derivatives below h that fixed_mask[b] does not fix (bit 7 and bits >= h are
 *   ignored); it may differ between trajectories and may be 0.
 * x_stride must be at least the longest row (else MTG_ERR_INVALID_ARGUMENT; with MTG_FLAG_DEVICE_PTRS
 * the mask is not read on the host: x_stride < (objective 2: K) + D V h is then checked per trajectory on
 * the device and reported as MTG_TRAJ_ROW_TOO_SHORT, an error bit like the others).  Entries of x past a row's
 * length are not read; entries of grad_out [B][x_stride] past it are written as +0.0.
 *
 * Semantics.  Every product and every sum below rounds on its own and is evaluated left to right.
 *   vertex_values = the fixed values from `values`, the free ones from x (setFreeConstraints); T = the
 *     times (objective 2: from x).
 *   J_d, grad_d   = mtg_cost_at_times_batch with one candidate and scales of 1.
 *   J_c, grad_c, is_collision = mtg_collision_cost_batch.
 *   J_sc, grad_sc = mtg_soft_constraint_cost_batch; both 0 when use_soft_constraints is off.
 * Objective 0: cost = J_d + J_sc (unweighted, as the reference's TODO leaves it); grad = grad_d (the
 *   reference does not add grad_sc there).  State: n_iterations++, cost_trajectory = J_d,
 *   cost_soft_constraints = J_sc, nothing else.
 * Objective 1: ct = w_d J_d, cc = w_c J_c, cs = w_sc J_sc; cost = (ct + cc) + cs;
 *   grad = (w_d grad_d + w_c grad_c) + w_sc grad_sc.  State: n_iterations++, the three costs; if
 *   !iter0_done: total_cost_iter0 = cost, iter0_done = 1.  There is no raise.
 * Objective 2: J_t = T_0 + T_1 + ... (sequential, computeTotalTrajectoryTime);
 *   grad_t[n] = ((w_d dJd_dt[n] + w_c dJc_dt[n]) + w_sc * 0.0) + w_t, with dJd_dt from
 *   mtg_time_jacobian_batch (one candidate, scales of 1, increment_time) and dJc_dt from
 *   mtg_collision_time_gradient_batch; the soft-constraint time term is the reference's exact zero (see
 *   mtg_soft_constraint_cost_batch).  The free-derivative gradient is that of objective 1.
 *   ct, cc, cs as above, ctime = w_t J_t, total = ((ct + cc) + ctime) + cs.
 *   If is_collision_safe and is_collision, the cost may be raised:
 *     with is_coll_raise_first_iter: if total < state.total_cost_iter0 then
 *       cc = (state.total_cost_iter0 - (total - cc)) + add_coll_raise;
 *     otherwise the same with last = ((state.cost_trajectory + state.cost_collision) + state.cost_time)
 *       + state.cost_soft_constraints in place of total_cost_iter0.
 *   cost = ((ct + cc) + ctime) + cs with the possibly raised cc.  State: n_iterations++, the four
 *   costs; if !iter0_done: total_cost_iter0 = cost, iter0_done = 1 (after the raise, as the reference
 *   orders it).  The gradient is not touched by the raise.
 * state == NULL behaves as an all-zero state that is thrown away.
 * weighted_costs_out [B][4] = trajectory, collision (after the raise), time, soft constraints as the
 *   state receives them (objective 0: J_d, 0, 0, J_sc; objective 1: time = 0).
 * grad_out == NULL is the reference's gradient.empty() branch: no gradient work is launched (no grad_*,
 *   no dJ*_dt) and the bits of cost_out, weighted_costs_out, collision_out and state do not change.
 *
 * Shapes and argument errors are those of the entry points used: objectives 1 and 2 need D = 3 and N in
 * {6, 8, 10, 12} and take the smaller of the components' LDS limits on K (MTG_ERR_TOO_LARGE);
 * objective 0 takes 1 <= D <= 4.  grid / collision are NULL for objective 0, soft is NULL iff
 * !use_soft_constraints; the param structs are host structs read during the call.
 * status [B] (nullable) is the OR of the components' statuses (the bits of mtg_solve_linear_batch) and
 * of MTG_TRAJ_BAD_TIME where a time is not positive and finite (a time <= 0 in x is such a case).  For a
 * trajectory with an error bit every floating output of its row is NaN (the padding of grad_out stays
 * +0.0), collision_out is 0 and its state is left as it was.
 *
 * Device call: an unpack kernel, the component kernels and a combine kernel on the context's stream,
 * no host synchronisation between them; intermediates live in a context-owned workspace
 * (DESIGN.md).  MTG_FLAG_DEVICE_PTRS (every array, parts' pointers and grid->distance included) and
 * MTG_FLAG_ASYNC as in the collision entries; a host-pointer call stages inputs and the requested
 * outputs once each. */
int mtg_objective_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* values,
                        const uint8_t* fixed_mask, const double* times, const double* x, int64_t x_stride,
                        const mtg_objective_params* params, const mtg_sdf_grid* grid,
                        const mtg_collision_params* collision, const mtg_soft_constraint_params* soft,
                        double* cost_out, double* grad_out, double* weighted_costs_out, uint8_t* collision_out,
                        mtg_objective_state* state, const mtg_objective_parts* parts, int32_t* status, unsigned flags);

/* Host (CPU) path of mtg_objective_batch, no context and no GPU needed: composed of
 * mtg_host_collision_cost_batch, mtg_host_soft_constraint_cost_batch,
 * mtg_host_collision_time_gradient_batch and a host evaluation of the derivative term:
 * J_d = sum_dims sum_segments e^T H(T_i) e with H as mtg_host_segment_matrices returns it,
 * grad_d = 2 (R d)_free, dJd_dt by the reference's central difference of J_d with the rules of
 * mtg_time_jacobian_batch (0 where T_i <= 0.1, NaN where T_i - increment_time <= 0).  The combination
 * is the same code as the device's.  All host pointers; threads <= 0: mtg_host_default_threads(). */
int mtg_host_objective_batch(int N, int D, int K, int64_t batch, const double* values, const uint8_t* fixed_mask,
                             const double* times, const double* x, int64_t x_stride,
                             const mtg_objective_params* params, const mtg_sdf_grid* grid,
                             const mtg_collision_params* collision, const mtg_soft_constraint_params* soft,
                             double* cost_out, double* grad_out, double* weighted_costs_out, uint8_t* collision_out,
                             mtg_objective_state* state, const mtg_objective_parts* parts, int32_t* status,
                             int threads);

/* Bounds and initial step of the optimiser's variables (host only), restated literally, index arithmetic
 * included: setFreeEndpointDerivativeHardConstraints (nl_impl:2518-2564) and the time bounds and
 * initial step of nl_impl:646-692.  x [B][x_stride] in the layout of mtg_objective_batch, with the K
 * times first when with_times is set.  Per trajectory, with nf = n_free[b] and r = derivative_to_optimize:
 *   times: lower 0.1, upper +inf;  every free derivative: -inf / +inf, then
 *   for k < D, n < K - 1:
 *     start = k nf + n r              (solve_with_position_constraint)
 *     start = k nf + n (r + 1), lower[start] = min_bound[k], upper[start] = max_bound[k]   (otherwise)
 *     for each constraint c: idx = start + derivative_c - 1 (with position constraint; unsigned, so
 *       derivative 0 wraps) or start + derivative_c; lower[idx] = -|limit_c|, upper[idx] = |limit_c|
 *   initial_step = initial_stepsize_rel * |x|.
 * An index the reference's .at() would throw on (>= D nf) gives MTG_ERR_INVALID_ARGUMENT.
 * constraints may be NULL (none; only n_constraints, derivative and limit are read); min_bound /
 * max_bound [D] are read only without the position constraint.  lower, upper, initial_step
 * [B][x_stride] (each nullable); entries past a row's length are +0.0. */
int mtg_host_objective_bounds_batch(int N, int D, int K, int64_t batch, const uint8_t* fixed_mask, int with_times,
                                    const double* x, int64_t x_stride, int derivative_to_optimize,
                                    int solve_with_position_constraint,
                                    const mtg_soft_constraint_params* constraints, const double* min_bound,
                                    const double* max_bound, double initial_stepsize_rel, double* lower,
                                    double* upper, double* initial_step);

/* ---- The two gradient-free objectives in the segment times: objectiveFunctionTime (nl_impl:765-832,
 * kOptimizeTime, reached through optimizeTime()) and objectiveFunctionTimeAndConstraints
 * (nl_impl:835-906, kOptimizeFreeConstraintsAndTime: the default `objective` of
 * NonlinearOptimizationParameters, polynomial_optimization_nonlinear.h:60).  The reference CHECKs
 * gradient.empty() in both (:768, :838), so there is no gradient argument. */
typedef struct mtg_objective_time_params {
  int32_t objective;               /* MTG_OBJECTIVE_TIME or MTG_OBJECTIVE_TIME_AND_CONSTRAINTS; others: INVALID_ARGUMENT */
  int32_t derivative_to_optimize;
  double  time_penalty;            /* reference default 500 */
  double  w_c;                     /* objective 3 only; the collision term exists iff w_c > 0 (nl_impl:789) */
  int32_t use_soft_constraints;
  int32_t reserved;                /* must be 0 */
} mtg_objective_time_params;

/* One evaluation of objectiveFunctionTime (objective 3) or objectiveFunctionTimeAndConstraints
 * (objective 4) per trajectory.  values / fixed_mask are the problem as mtg_solve_linear_batch reads
 * it; row b of x [B][x_stride] is the vector nlopt sees:
 *   objective 3: the K segment times, and nothing else;
 *   objective 4: the K times, then D blocks of n_free[b] free derivatives in the layout of
 *                mtg_objective_batch objective 2.
 * x_stride must be at least the longest row (else MTG_ERR_INVALID_ARGUMENT; with MTG_FLAG_DEVICE_PTRS
 * the check is made per trajectory on the device and reported as MTG_TRAJ_ROW_TOO_SHORT, an error bit
 * like the others); entries of x past a row's length are not read.
 *
 * Semantics.  Every product and every sum below rounds on its own and is evaluated left to right.
 * T = the times from x.
 * Objective 3 (nl_impl:765-832):
 *   ct, the free derivatives and the coefficients = cost_out, free_out and coeffs of
 *     mtg_solve_linear_batch(values, fixed_mask, T, flags = 0) (updateSegmentTimes + solveLinear +
 *     computeCost, :779-782): the bytes of the default kernel for the shape, whichever it is.
 *   J_t = T_0 + T_1 + ... (sequential, computeTotalTrajectoryTime); ctime = (J_t * J_t) * time_penalty (:784-785).
 *   vertex_values = the fixed entries from `values`, the free ones from the solve (setFreeConstraints' layout).
 *   cs = the cost of mtg_soft_constraint_cost_batch(vertex_values, T, constraints) when
 *     use_soft_constraints is set, else 0 (:795-801).  cs is unweighted: the reference applies no w_sc here.
 *   cc = w_c * J_c when w_c > 0, else 0 (:787-793).  J_c is the loop documented at
 *     mtg_collision_cost_batch with its clock bounds and end-of-segment correction taken from T, and its
 *     coefficients c_i = A(Tc_i)^-1 [x_i; x_{i+1}] with Tc = coeff_times[b] [B][K]: optimizeTime forms L_
 *     once from the initial times (:259-264) and objectiveFunctionTime never refreshes it, while
 *     getCostAndGradientCollision takes its coefficients as L_ * d (:1558) and its loop bounds from
 *     getSegmentTimes (:1563) -- the stale L_ documented at mtg_collision_time_gradient_batch.
 *     coeff_times is required when w_c > 0.  No semantics is invented for a refreshed L_: a caller who
 *     wants one passes coeff_times equal to the times in x.
 *   cost = ((ct + cc) + ctime) + cs (:831).  State (:817-829): n_iterations++, the four costs; if
 *     !iter0_done: total_cost_iter0 = cost, iter0_done = 1.
 * Objective 4 (nl_impl:835-906):
 *   vertex_values = the fixed entries from `values`, the free ones from x (setFreeConstraints, :871).
 *   ct = 0.5 * J_d with J_d from mtg_cost_at_times_batch (one candidate, scales of 1): the reference's
 *     computeCost() after updateSegmentTimes + setFreeConstraints (:870-873).  The halving is exact, so
 *     ct's bits are defined by that entry point.
 *   ctime and cs as in objective 3 (:877-886).  There is no collision term: grid, collision and
 *     coeff_times must be NULL, and w_c is not read.
 *   cost = (ct + ctime) + cs (:905).  State (:899-903): n_iterations++, cost_trajectory, cost_time and
 *     cost_soft_constraints; cost_collision, total_cost_iter0 and iter0_done are left as they were.
 * state == NULL behaves as an all-zero state that is thrown away.
 * Outputs of both objectives (cost_out [B] is required, every other output is nullable, and requesting
 * one does not change the bits of cost_out or state):
 *   weighted_costs_out [B][4] = ct, cc (or 0), ctime, cs.
 *   collision_out [B]: the collision flag of J_c's walk (0 without a collision term).
 *   maxima_out [B][n_constraints] = the maxima of mtg_soft_constraint_cost_batch;
 *   constraint_values_out [B][n_constraints], entry c = maxima[c].value - limit[c]: what
 *     evaluateMaximumMagnitudeConstraint returns to nlopt for a hard inequality constraint
 *     (nl_impl:2346-2392).  Both are available whether or not use_soft_constraints is set: with it off and
 *     either requested, the maxima search runs and its cost is discarded.  `constraints` may be NULL only
 *     if use_soft_constraints is off and neither is requested.
 *   free_out [B][D][V*h] (entries >= n_free are 0) and coeffs_out [B][K][D][N] describe the trajectory at
 *     x: objective 3: the solve's own outputs; objective 4: the free part of x, and the coefficients of
 *     mtg_coefficients_from_vertices_batch(vertex_values, T).
 *   parts (nullable): J_d (objective 4 only), J_c, J_sc and J_t are filled as the components return
 *     them; its gradient fields (dJd_dt, dJc_dt, grad_d, grad_c, grad_sc) must be NULL.
 *
 * Shapes and errors.  w_c > 0 (objective 3) requires D = 3, N in {6, 8, 10, 12} and non-NULL grid,
 * collision and coeff_times; otherwise 1 <= D <= 4 and those three must be NULL.  The soft-constraint
 * search needs N in {6, 8, 10, 12}.  K is limited by the smaller LDS limit of the components used
 * (MTG_ERR_TOO_LARGE).  MTG_ERR_INVALID_ARGUMENT: an objective other than 3 or 4, reserved != 0, a
 * missing or an extra grid / collision / coeff_times, a non-NULL gradient field of parts.
 * status [B] (nullable) is the OR of the solve's bits (objective 3: MTG_TRAJ_BAD_TIME, MTG_TRAJ_NOT_SPD,
 * MTG_TRAJ_WARN_DROPPED) and of the components' bits; a time in x or an entry of coeff_times that is
 * not positive and finite gives MTG_TRAJ_BAD_TIME.  For a trajectory with an error bit every floating
 * output of its row is NaN (maxima: time and value NaN, segment 0), collision_out is 0 and its state
 * is left as it was: the rule of mtg_objective_batch.  The parts are exempt, as there.
 *
 * Device call: one stream, no host synchronisation between the kernels; intermediates live in the
 * context-owned workspace.  Objective 3: times-unpack | solve | assemble | [soft
 * constraints] | [collision with coefficient times] | combine; objective 4: unpack | cost | [soft
 * constraints] | [coefficients] | combine.  MTG_FLAG_DEVICE_PTRS and MTG_FLAG_ASYNC as in
 * mtg_objective_batch.  Results do not depend on the trajectory's place in the batch or on the batch. */
int mtg_objective_time_batch(mtg_ctx* ctx, int N, int D, int K, int64_t batch, const double* values,
                             const uint8_t* fixed_mask, const double* x, int64_t x_stride,
                             const mtg_objective_time_params* params, const double* coeff_times,
                             const mtg_sdf_grid* grid, const mtg_collision_params* collision,
                             const mtg_soft_constraint_params* constraints, double* cost_out,
                             double* weighted_costs_out, uint8_t* collision_out, double* constraint_values_out,
                             mtg_extremum* maxima_out, double* free_out, double* coeffs_out,
                             mtg_objective_state* state, const mtg_objective_parts* parts, int32_t* status,
                             unsigned flags);

/* Host (CPU) path of mtg_objective_time_batch, no context and no GPU needed: composed of
 * mtg_host_solve_linear_batch (objective 3), mtg_host_soft_constraint_cost_batch, the host collision
 * loop of mtg_host_collision_cost_batch with the coefficients formed at coeff_times, the host J_d of
 * mtg_host_objective_batch (objective 4) and mtg_host_coefficients_from_vertices_batch; the
 * combination is the same code as the device's.  All host pointers; threads <= 0:
 * mtg_host_default_threads(). */
int mtg_host_objective_time_batch(int N, int D, int K, int64_t batch, const double* values,
                                  const uint8_t* fixed_mask, const double* x, int64_t x_stride,
                                  const mtg_objective_time_params* params, const double* coeff_times,
                                  const mtg_sdf_grid* grid, const mtg_collision_params* collision,
                                  const mtg_soft_constraint_params* constraints, double* cost_out,
                                  double* weighted_costs_out, uint8_t* collision_out, double* constraint_values_out,
                                  mtg_extremum* maxima_out, double* free_out, double* coeffs_out,
                                  mtg_objective_state* state, const mtg_objective_parts* parts, int32_t* status,
                                  int threads);

/* Bounds and initial step of the two set-ups (host only), restated literally.  x [B][x_stride] in the
 * layout of mtg_objective_time_batch, `objective` as in mtg_objective_time_params.
 *   MTG_OBJECTIVE_TIME (optimizeTime, nl_impl:248-256 and :273-276), for each of the K times t:
 *     initial_step = initial_stepsize_rel * t, lower = 0.1, upper = t * 2.
 *   MTG_OBJECTIVE_TIME_AND_CONSTRAINTS (optimizeTimeAndFreeConstraints, nl_impl:551-562), for every
 *     entry of the row: initial_step = initial_stepsize_rel * |x|, lower = -|x| * 2, upper = |x| * 2;
 *     then lower = 0.1 for the K times.
 * fixed_mask [B][V] gives the rows' lengths (objective 4; not read for objective 3).  lower, upper,
 * initial_step [B][x_stride] (each nullable); entries past a row's length are +0.0, as in
 * mtg_host_objective_bounds_batch.  MTG_ERR_INVALID_ARGUMENT: another objective, x_stride shorter than
 * a row. */
int mtg_host_objective_time_bounds_batch(int N, int D, int K, int64_t batch, const uint8_t* fixed_mask,
                                         int objective, const double* x, int64_t x_stride,
                                         double initial_stepsize_rel, double* lower, double* upper,
                                         double* initial_step);

/* Timing of the most recent kernel launch(es) of this context on its stream
 * (hipEvent pair around the solve kernel), in milliseconds. */
int mtg_last_kernel_ms(mtg_ctx* ctx, float* ms);
/* Keep a HIP event pair per launch for the last `ring` launches (ring >= 0;
 * the default is 1; 0 records no events).  Single-kernel calls carry the pair in
 * the kernel's dispatch packet.  mtg_kernel_times synchronizes on the newest event and
 * writes up to n durations (ms, oldest first) of the launches still in the
 * ring; *n_out receives the count. */
int mtg_enable_timing(mtg_ctx* ctx, int ring);
int mtg_kernel_times(mtg_ctx* ctx, float* ms, int n, int* n_out);

/* Host (CPU) path of mtg_solve_linear_batch, no context and no GPU needed: the same algorithm
 * as the HIP kernels (exact tables, symmetric pinning, block LDL^T Thomas), in scalar C++ on the
 * calling thread(s).  For one problem it is the lowest-latency path (a GPU round trip costs more
 * than the solve itself): the C++ drop-in PolynomialOptimization<N>::solveLinear uses it by
 * default (BASELINE config 1), replacing the reference's CPU solveLinear (lin_impl:329-369).
 * Same arrays and per-trajectory status as mtg_solve_linear_batch, all host pointers;
 * threads <= 0: mtg_host_default_threads(). */
int mtg_host_solve_linear_batch(int N, int D, int K, int derivative_to_optimize, int64_t batch,
                                const double* values, const uint8_t* fixed_mask, const double* times,
                                double* coeffs, double* free_out, int32_t* n_free_out, double* cost_out,
                                int32_t* status, int threads);

/* Host (CPU) path of mtg_solve_linear_ragged_batch, no context and no GPU needed: the same CSR
 * arrays (all host pointers) and the same plan offsets; every trajectory is solved on its own blocks
 * by the code behind mtg_host_solve_linear_batch, so its outputs are the bytes that call writes for
 * a batch of one.  Threaded over trajectories; threads <= 0: mtg_host_default_threads().  The
 * call-level errors of the device call except MTG_ERR_TOO_LARGE (the host solver has no size limit). */
int mtg_host_solve_linear_ragged_batch(int N, int D, int derivative_to_optimize, int64_t batch,
                                       const int32_t* seg_count, const double* values, const uint8_t* fixed_mask,
                                       const double* times, double* coeffs, double* free_out, int32_t* n_free_out,
                                       double* cost_out, int32_t* status, int threads);

/* The worker count the host paths (mtg_host_*) use when called with threads <= 0: the CPUs this
 * process may run on -- its affinity mask, capped by the cgroup CPU quota -- not every CPU of the
 * machine.  (The reference's host code is single-threaded; there is no reference counterpart.) */
int mtg_host_default_threads(void);

/* Host (CPU) path of mtg_min_max_magnitude_batch, no context and no GPU needed: the same candidates,
 * root isolation and tie rules as the HIP kernel, on the calling thread(s).  The reference computes
 * Trajectory::computeMinMaxMagnitude on the CPU (src/trajectory.cpp:181-218); the C++ drop-in uses
 * this for its single trajectories unless ExecutionPolicy::kDevice.  All host pointers; threads <= 0:
 * mtg_host_default_threads(). */
int mtg_host_min_max_magnitude_batch(int N, int D, int K, int64_t batch, const double* coeffs, const double* times,
                                     int derivative, uint32_t dimension_mask, mtg_extremum* minimum,
                                     mtg_extremum* maximum, int threads);

/* Host (CPU) path of mtg_evaluate_at_batch, no context and no GPU needed: the definition there
 * followed literally in scalar code (the linear scan of trajectory.cpp:42-57, not a binary search),
 * threaded over trajectories.  The same bits as the kernels; the C++ drop-in's evaluateAt<N> uses it
 * unless ExecutionPolicy::kDevice.  All host pointers; the argument errors of mtg_evaluate_at_batch
 * (no MTG_ERR_TOO_LARGE); threads <= 0: mtg_host_default_threads(). */
int mtg_host_evaluate_at_batch(int N, int D, int K, int64_t batch, const double* coeffs, const double* times,
                               const double* t_query, int64_t t_stride, int64_t M, int derivative_begin,
                               int n_derivatives, double* out, uint8_t* in_range_out, int32_t* status, int threads);

/* Host (CPU) paths of mtg_evaluate_at_ragged_batch and mtg_min_max_magnitude_ragged_batch, no context
 * and no GPU needed: the scalar code behind the two host entries above on each trajectory's blocks of
 * the CSR arrays, so a trajectory's outputs are the bytes those entries write for it alone.  Threaded
 * over trajectories; threads <= 0: mtg_host_default_threads().  All host pointers; the call-level
 * errors of the device calls except MTG_ERR_TOO_LARGE. */
int mtg_host_evaluate_at_ragged_batch(int N, int D, int64_t batch, const int32_t* seg_count, const double* coeffs,
                                      const double* times, const double* t_query, int64_t t_stride, int64_t M,
                                      int derivative_begin, int n_derivatives, double* out, uint8_t* in_range_out,
                                      int32_t* status, int threads);
int mtg_host_min_max_magnitude_ragged_batch(int N, int D, int64_t batch, const int32_t* seg_count,
                                            const double* coeffs, const double* times, int derivative,
                                            uint32_t dimension_mask, mtg_extremum* minimum, mtg_extremum* maximum,
                                            int threads);

/* Host (CPU) paths of mtg_segment_min_max_magnitude_batch and mtg_segment_min_max_axis_batch, no
 * context and no GPU needed: the same samples, refinement, candidate order and tie rules in scalar
 * code (the search mtg_host_min_max_magnitude_batch runs per segment, on the window), threaded over
 * segments.  The C++ drop-in's Polynomial::computeMinMax* and Segment::computeMinMaxMagnitude* use
 * them.  All host pointers; the argument errors of the device calls; threads <= 0:
 * mtg_host_default_threads(). */
int mtg_host_segment_min_max_magnitude_batch(int N, int D, int64_t n_segments, const double* coeffs,
                                             const double* times, const double* windows, int derivative,
                                             uint32_t dimension_mask, mtg_extremum* minimum, mtg_extremum* maximum,
                                             double* candidate_times, int32_t* candidate_count,
                                             int candidate_capacity, int32_t* status, int threads);
int mtg_host_segment_min_max_axis_batch(int N, int D, int64_t n_segments, const double* coeffs, const double* times,
                                        const double* windows, int derivative, mtg_extremum* minimum,
                                        mtg_extremum* maximum, double* candidate_times, int32_t* candidate_count,
                                        int candidate_capacity, int32_t* status, int threads);

/* ---- Host utilities (no GPU): the reference's synthetic-input generators,
 * bit-exact with libstdc++ <random>, packed straight into the ABI layout.
 * Trajectory b of a batch uses seed (seed0 + b).  values [B][V][h][D],
 * fixed_mask [B][V]; derivatives above N/2-1 set the WARN_DROPPED bit in the
 * returned mask (bit 7) and are otherwise ignored, as setupFromVertices does. */
/* createRandomVertices (src/vertex.cpp:27-79) + estimateSegmentTimes (:162-178) */
int mtg_host_random_vertices_batch(int N, int D, int K, int max_derivative, const double* pos_min,
                                   const double* pos_max, uint32_t seed0, int64_t batch,
                                   double v_max, double a_max, double magic_fabian_constant,
                                   double* values, uint8_t* fixed_mask, double* times,
                                   int threads);
/* createRandomVerticesPath (src/polynomial_timing_evaluation.cpp:34-91) +
 * estimateSegmentTimes(v_max, a_max, magic) as timeEval does (:93-112) */
int mtg_host_random_vertices_path_batch(int N, int D, int K, double average_distance,
                                        int max_derivative, uint32_t seed0, int64_t batch,
                                        double v_max, double a_max, double magic_fabian_constant,
                                        double* values, uint8_t* fixed_mask, double* times,
                                        int threads);

/* estimateSegmentTimes (src/vertex.cpp:162-178) on explicit positions [n_vertices][D]:
 * times[i] = 2 d / v_max (1 + magic v_max / a_max exp(-2 d / v_max)), d = |p_{i+1} - p_i| with
 * Eigen's norm reduction order.  times [n_vertices - 1]. */
int mtg_host_estimate_segment_times(int n_vertices, int D, const double* positions, double v_max, double a_max,
                                    double magic_fabian_constant, double* times);

/* Per-segment matrices of PolynomialOptimization<N> at segment time T (> 0), N x N row-major, any
 * pointer may be NULL:
 *   A      setupMappingMatrix (lin_impl:102-111)
 *   A_inv  A(T)^-1 (invertMappingMatrix, lin_impl:133-169), from the exact A(1)^-1 table:
 *          diag(T^-j) A(1)^-1 S(T), S = diag(T^(slot mod N/2))
 *   Q      computeQuadraticCostJacobian(derivative_to_optimize, T) (lin_impl:574-589)
 *   H      A^-T Q A^-1 (constructR's per-segment block, lin_impl:305-308), from the exact table:
 *          T^(1-2r) S Htilde S
 * They back getA / getAInverse / getR of the C++ drop-in. */
int mtg_host_segment_matrices(int N, int derivative_to_optimize, double T, double* A, double* A_inv, double* Q,
                              double* H);

/* Host form of mtg_coefficients_from_vertices_batch (setFreeConstraints +
 * updateSegmentsFromCompactConstraints, lin_impl:253-273) for the C++ drop-in's single problems:
 * vertex_values [B][V][h][D] (all derivatives), times [B][K] -> coeffs [B][K][D][N]. */
int mtg_host_coefficients_from_vertices_batch(int N, int D, int K, int64_t batch, const double* vertex_values,
                                              const double* times, double* coeffs, int threads);

/* Host form of mtg_vertex_derivatives_batch (M^+ A p, nl_impl:162-180) in scalar C++: the end
 * derivatives of every segment by Horner with the base coefficients j!/(j-k)! (polynomial.h:120-151),
 * the mean of the two ends that meet at an interior vertex.  coeffs [B][K][D][N], times [B][K] ->
 * vertex_values [B][V][h][D]; any K.  threads <= 0: mtg_host_default_threads(). */
int mtg_host_vertex_derivatives_batch(int N, int D, int K, int64_t batch, const double* coeffs, const double* times,
                                      double* vertex_values, int threads);

/* Host forms of the two CSR maps (mtg_vertex_derivatives_ragged_batch,
 * mtg_coefficients_from_vertices_ragged_batch): the uniform host code on each trajectory's blocks,
 * threaded over trajectories; a trajectory's bytes are those of the uniform host entry with batch 1.
 * The errors on N, D, batch and seg_count are the device entries'. */
int mtg_host_vertex_derivatives_ragged_batch(int N, int D, int64_t batch, const int32_t* seg_count,
                                             const double* coeffs, const double* times, double* vertex_values,
                                             int threads);
int mtg_host_coefficients_from_vertices_ragged_batch(int N, int D, int64_t batch, const int32_t* seg_count,
                                                     const double* vertex_values, const double* times, double* coeffs,
                                                     int threads);

#ifdef __cplusplus
}
#endif
#endif /* MTG_H_ */
