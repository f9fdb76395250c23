// Internal declarations shared by the kernels (mtg_kernels.hip) and the C ABI
// (mtg_capi.hip).  Not installed; the public surface is include/mtg.h.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mtg.h"
#include "mtg_objective_common.h"

namespace mtg {

// Timing events for the next kernel launch, set by the C ABI around a timed call: launch_kernel()
// records them in the kernel's own dispatch packet (hipExtLaunchKernelGGL) instead of as two
// separate marker packets in the stream.
struct PendingEvents {
  hipEvent_t start = nullptr, stop = nullptr;
  bool used = false;
};
PendingEvents& pending_events();  // per host thread

template <typename F, typename... Args>
inline void launch_kernel(F kernel, const dim3& grid, const dim3& block, uint32_t lds, hipStream_t stream,
                          Args... args) {
  PendingEvents& pe = pending_events();
  if (pe.start && !pe.used) {
    pe.used = true;
    hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, pe.start, pe.stop, 0u, args...);
  } else {
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
  }
}

// Arguments of one batched solve launch.  Pointers are device pointers.
struct SolveArgs {
  const double* values;   // [B][V][h][D]
  const uint8_t* mask;    // [B][V]
  const double* times;    // [B][K]
  double* coeffs;         // [B][K][D][N]
  double* free_out;       // [B][D][V*h]  (nullable)
  int32_t* n_free_out;    // [B]          (nullable)
  double* cost_out;       // [B]          (nullable)
  int32_t* status;        // [B]          (nullable)
  const double* scales;   // time-sweep candidate scales [C] (nullable: plain solve)
  int64_t B;              // trajectories (or trajectory x candidate pairs for the sweep)
  int K, D, r;
  int n_cand;             // candidates per trajectory for the sweep (1 for a plain solve)
  int gi;                 // register column kernel: G in LDS for the interior-waypoint body (set by
                          // launch_solve_reg, mtg_solve_reg.inc reg_gi_doubles)
  double* work;           // long-chain dimension-lane kernel: its workspace (dlx_workspace_bytes)
  int64_t work_bytes;
};

// Lanes per trajectory and LDS bytes per workgroup for a shape; returns false
// when the per-trajectory working set cannot fit in LDS.
bool solve_geometry(int N, int D, int K, int* lanes_per_traj, size_t* lds_bytes, int* traj_per_block);

// Launch the fused solve on `stream` with the kernel solve_kernel() picks: the register column
// kernel (mtg_solve_reg.hip) where reg_geometry allows it (K <= 12, or N = 12 with K <= 20), else
// the general LDS-resident kernel (mtg_kernels.hip); the dimension-lane kernel (mtg_solve_dl.hip)
// where dl_geometry allows it; MTG_FLAG_GENERAL_KERNEL the general kernel.
// B: the batch (trajectories, or trajectory x candidate pairs; < 0: unknown).  The choice does not
// depend on it (since round 4: the DL kernel at every size where it applies).
int solve_kernel(int N, int D, int K, unsigned flags, int r = -1, int64_t B = -1);  // MTG_KERNEL_*
hipError_t launch_solve(int N, const SolveArgs& a, hipStream_t stream, unsigned flags = 0);
bool reg_geometry(int N, int D, int K, int* lanes_per_traj, size_t* lds_bytes);
hipError_t launch_solve_reg(int N, const SolveArgs& a, hipStream_t stream);
// dimension-lane kernel of the interior-waypoint pattern (mtg_solve_dl.hip: ends fix every
// derivative, interior vertices exactly their position): one lane per (chain, dimension)
bool dl_geometry(int N, int D, int K, int r);
hipError_t launch_solve_dl(int N, const SolveArgs& a, hipStream_t stream);
// the same recurrence for chains of any length (mtg_solve_dlx.hip), where neither the DL kernel nor
// the column kernel applies; its workspace (a.work) holds dlx_workspace_bytes for the launch's batch
bool dlx_geometry(int N, int D, int K, int r);
size_t dlx_workspace_bytes(int N, int D, int K, int64_t B);
hipError_t launch_solve_dlx(int N, const SolveArgs& a, hipStream_t stream);

// Two-kernel path (MTG_FLAG_SPLIT_KERNELS): assembly into the block-tridiagonal
// workspace, then the block-Cholesky solve + recovery.
size_t split_workspace_bytes(int N, int D, int K, int64_t B);
hipError_t launch_solve_split(int N, const SolveArgs& a, void* workspace, hipStream_t stream);

// The copy kernels of the ragged solve (mtg_ragged.hip).  One record per gathered trajectory, record j
// for the j-th trajectory of the packed arrays: vertex offsets in the caller's CSR arrays and in the
// packed ones (the segment offsets are src_v - b and dst_v - j), the batch index and K.
struct RaggedRec {
  int64_t src_v, dst_v, b;
  int32_t K, reserved;
};
struct RaggedCopyArgs {
  const RaggedRec* recs;  // [n]
  int64_t n;
  int hD, DN;             // (N / 2) D and D N
  // the caller's CSR arrays (gather reads the first three, scatter writes the others; nullable outputs)
  const double* values;
  const uint8_t* mask;
  const double* times;
  double *coeffs, *free, *cost;
  int32_t *n_free, *status;
  // the packed arrays (gather writes the first three, scatter reads the others)
  double* p_values;
  uint8_t* p_mask;
  double* p_times;
  const double *p_coeffs, *p_free, *p_cost;
  const int32_t *p_n_free, *p_status;
};
hipError_t launch_ragged_gather(const RaggedCopyArgs& a, hipStream_t stream);
hipError_t launch_ragged_scatter(const RaggedCopyArgs& a, hipStream_t stream);
// The copy kernels of the ragged min / max magnitude, driven by the same records: coeffs and times of
// the gathered trajectories into packed arrays (a wave per trajectory, as launch_ragged_gather), and
// their extremes from the packed arrays to minimum[b] / maximum[b] (nullable pairs; a lane each).
struct RaggedCoeffArgs {
  const RaggedRec* recs;  // [n]
  int64_t n;
  int DN;                 // D N
  const double *coeffs, *times;                 // the caller's CSR arrays
  double *p_coeffs, *p_times;                   // the packed arrays
  mtg_extremum *p_minimum, *p_maximum;          // [n] (the group launches write them, the scatter reads them)
  mtg_extremum *minimum, *maximum;              // [B]
};
hipError_t launch_ragged_gather_coeffs(const RaggedCoeffArgs& a, hipStream_t stream);
hipError_t launch_ragged_scatter_extrema(const RaggedCoeffArgs& a, hipStream_t stream);

// cost / gradient of fixed vertex derivatives at candidate times (mtg_cost.hip)
size_t cost_lds_bytes(int N, int D, int K);
hipError_t launch_cost_at_times(int N, int r, const double* values, const uint8_t* mask, const double* times,
                                const double* scales, double* cost, double* grad, int64_t B, int K, int D, int C,
                                hipStream_t stream);

// collision cost / gradient over a signed distance field (mtg_collision.hip); `distance` is the
// device copy of grid.distance.  coeff_times [B][K] (nullable, cost only: hipErrorInvalidValue with
// grad): the coefficients are formed at these times while the walk reads `times` (the stale L_ of
// objectiveFunctionTime, mtg.h); an entry that is not positive and finite gives MTG_TRAJ_BAD_TIME.
// nullptr launches the kernels of mtg_collision_cost_batch, unchanged.
size_t collision_lds_bytes(int N, int K);
hipError_t launch_collision_cost(int N, const double* values, const uint8_t* mask, const double* times,
                                 const mtg_sdf_grid& grid, const float* distance, const mtg_collision_params& p,
                                 double* cost, double* grad, uint8_t* collision, int32_t* n_evaluated, int32_t* status,
                                 int64_t B, int K, hipStream_t stream, const double* coeff_times = nullptr);

// the same for a CSR batch (mtg_collision_ragged.hip): trajectory b's segments are seg_off[b] ..
// seg_off[b + 1] of times [sum K], its vertices the rows seg_off[b] + b .. of values [sum K + B][h][3] and
// mask [sum K + B], its gradient block [3][V_b h] at double offset 3 h (seg_off[b] + b); seg_off [B + 1]
// is a device array.  One launch whose LDS is collision_lds_bytes(N, K_max), K_max the largest K_b.
hipError_t launch_collision_cost_ragged(int N, int K_max, int64_t B, const int64_t* seg_off, const double* values,
                                        const uint8_t* mask, const double* times, const mtg_sdf_grid& grid,
                                        const float* distance, const mtg_collision_params& p, double* cost,
                                        double* grad, uint8_t* collision, int32_t* n_evaluated, int32_t* status,
                                        hipStream_t stream);

// segment-time gradient of the collision cost (mtg_collision_time.hip); `distance` is the device copy
// of grid.distance
size_t collision_time_lds_bytes(int N, int K);
hipError_t launch_collision_time_gradient(int N, const double* values, const double* times, const mtg_sdf_grid& grid,
                                          const float* distance, const mtg_collision_params& p, double increment_time,
                                          double* grad_t, double* side_cost, int32_t* side_evaluated, int32_t* walked,
                                          int32_t* status, int64_t B, int K, hipStream_t stream);

// soft-constraint cost / gradient of the magnitude limits (mtg_soft_constraint.hip): threads per block
// for a shape (0: the trajectory's working set exceeds LDS) and the block's LDS bytes
int soft_constraint_threads(int N, int D, int K, int C);
size_t soft_constraint_lds_bytes(int N, int D, int K, int C, int threads);
hipError_t launch_soft_constraint_cost(int N, const double* values, const uint8_t* mask, const double* times,
                                       const mtg_soft_constraint_params& params, double* cost, double* grad,
                                       mtg_extremum* maxima, int32_t* status, int64_t B, int K, int D,
                                       hipStream_t stream);

// segment-time cost sweep + time Jacobian on the matrix cores (mtg_jacobian.hip)
size_t time_jacobian_lds_bytes(int N, int D, int K, int C);
hipError_t launch_time_jacobian(int N, int r, const double* values, const double* times, const double* scales,
                                double* cost, double* jac, double delta, int64_t B, int K, int D, int C,
                                hipStream_t stream);

// the objective in the optimiser's variables (mtg_objective.hip): the unpack and combine kernels around
// the component launchers above.  All pointers are device pointers.
struct ObjectiveUnpackArgs {
  const double* x;         // [B][x_stride]
  const double* values;    // [B][V][h][D]
  const uint8_t* mask;     // [B][V]
  const double* times_in;  // [B][K], or nullptr: the times lead the rows of x (objective 2)
  double* vertex_values;   // [B][V][h][D]
  double* times;           // [B][K]
  int32_t* n_free;         // [B]
  int32_t* status;         // [B]: MTG_TRAJ_BAD_TIME, MTG_TRAJ_ROW_TOO_SHORT
  double* ones;            // [K]: the scales of 1
  int64_t B, x_stride;
  int K, V, h, D;
};
struct ObjectiveCombineArgs {
  const double *J_d, *J_c, *J_sc;              // [B] (J_c, J_sc nullable: 0)
  const double *grad_d, *grad_c, *grad_sc;     // [B][D][V*h] (grad_c, grad_sc nullable: 0)
  const double *dJd_dt, *dJc_dt, *times;       // [B][K]
  const uint8_t* collision;                    // [B] (nullable: 0)
  const int32_t *n_free, *st_unpack, *st_collision, *st_soft, *st_collision_time;  // [B] (st_* nullable)
  double *cost_out, *grad_out, *weighted, *J_t_out;
  uint8_t* collision_out;
  mtg_objective_state* state;
  int32_t* status;
  int64_t B, x_stride;
  int K, V, h, D;
  ObjectiveRule rule;
};
hipError_t launch_objective_unpack(const ObjectiveUnpackArgs& a, hipStream_t stream);
hipError_t launch_objective_combine(const ObjectiveCombineArgs& a, hipStream_t stream);

// the kernels of mtg_objective_time_batch (mtg_objective.hip) that the component launchers do not
// provide.  All pointers are device pointers.
struct ObjectiveTimesUnpackArgs {  // objective 3: x -> times, the bad-time and row-too-short status
  const double* x;  // [B][x_stride]
  double* times;    // [B][K]; 1.0 for a row that does not fit x_stride (its x is not read)
  int32_t* status;  // [B]
  int64_t B, x_stride;
  int K;
};
struct ObjectiveAssembleArgs {  // objective 3: values, fixed_mask and the solve's free_out -> vertex_values
  const double* values;   // [B][V][h][D]
  const uint8_t* mask;    // [B][V]
  const double* free;     // [B][D][V*h]
  double* vertex_values;  // [B][V][h][D]
  int64_t B;
  int V, h, D;
};
struct ObjectiveTimeCombineArgs {
  const double* cost_traj;     // [B]: the solve's cost (objective 3) or J_d (objective 4)
  const double *J_c, *J_sc;    // [B] (nullable: 0)
  const double* times;         // [B][K]
  const uint8_t* collision;    // [B] (nullable: 0)
  const int32_t *st_unpack, *st_solve, *st_soft, *st_collision;  // [B] (all but st_unpack nullable)
  const mtg_extremum* maxima;  // [B][C] as the soft-constraint kernel wrote them (nullable; may be maxima_out)
  const double* x;             // [B][x_stride] and
  const int32_t* n_free;       // [B]: objective 4's free_out (nullable otherwise)
  double limit[8];
  int C;
  double *cost_out, *weighted, *J_t_out, *constraint_values, *free_out, *coeffs_out;  // (all but cost_out nullable)
  mtg_extremum* maxima_out;
  uint8_t* collision_out;
  mtg_objective_state* state;
  int32_t* status;
  int64_t B, x_stride;
  int K, V, h, D, N;
  ObjectiveTimeRule rule;
};
hipError_t launch_objective_times_unpack(const ObjectiveTimesUnpackArgs& a, hipStream_t stream);
hipError_t launch_objective_assemble(const ObjectiveAssembleArgs& a, hipStream_t stream);
hipError_t launch_objective_time_combine(const ObjectiveTimeCombineArgs& a, hipStream_t stream);

// vertex derivatives <-> coefficients (mtg_vertex.hip)
bool vertex_map_fits(int N, int D, int K);
hipError_t launch_vertex_map(bool to_coeffs, int N, const double* in, const double* times, double* out, int64_t B,
                             int K, int D, hipStream_t stream);

// the same for a CSR batch (mtg_vertex_ragged.hip): coeffs [S][D][N], times [S], values [S + B][h][D]
// with S = seg_off[B] segments in all; a block owns vertex_ragged_tile(N, D) consecutive packed
// segments (0: a single segment's arrays exceed the LDS staging), whatever K the trajectories have
int vertex_ragged_tile(int N, int D);
hipError_t launch_vertex_map_ragged(bool to_coeffs, int N, const double* in, const double* times,
                                    const int64_t* seg_off, double* out, int64_t B, int64_t S, int D,
                                    hipStream_t stream);

// min / max magnitude of a derivative over trajectories (mtg_extrema.hip)
hipError_t launch_min_max_magnitude(int N, const double* coeffs, const double* times, int64_t B, int K, int D,
                                    int derivative, unsigned dims, mtg_extremum* mn, mtg_extremum* mx,
                                    hipStream_t stream);

// min / max per segment (magnitude) or per (segment, dimension) (axis: signed value) on a window, with
// the candidate list (mtg_segment_extrema.hip).  coeffs [S][D][N], times [S] (nullable with windows),
// windows [S][2] (nullable: [0, times[s]]); mn / mx [S] or [S][D], cand [..][cap], count, status [S]:
// every output nullable
hipError_t launch_segment_extrema(bool axis, int N, const double* coeffs, const double* times, const double* windows,
                                  int64_t S, int D, int derivative, unsigned dims, mtg_extremum* mn, mtg_extremum* mx,
                                  double* cand, int32_t* count, int cap, int32_t* status, hipStream_t stream);

// Trajectory::evaluate at caller-given times (mtg_evaluate_at.hip).  evaluate_at_plan is the one rule
// that picks the mapping (path: MTG_EVALUATE_AT_LANE or MTG_EVALUATE_AT_STAGED) and the block's
// threads and LDS bytes from the shape alone; false: a block's rows do not fit in LDS.
struct EvalAtPlan {
  int path, threads;
  size_t lds;
};
bool evaluate_at_plan(int N, int D, int K, int64_t M, int n_derivatives, EvalAtPlan* plan);
hipError_t launch_evaluate_at(int N, int D, int K, int64_t B, const double* coeffs, const double* times,
                              const double* t_query, int64_t t_stride, int64_t M, int derivative_begin,
                              int n_derivatives, double* out, uint8_t* in_range, int32_t* status, hipStream_t stream);

// the same for a CSR batch (mtg_evaluate_at_ragged.hip): trajectory b's segments are
// seg_off[b] .. seg_off[b + 1] of coeffs [sum K][D][N] and times [sum K]; seg_off [B + 1] is a device
// array; the plan is evaluate_at_plan at K_max, the largest segment count of the batch
hipError_t launch_evaluate_at_ragged(int N, int D, int K_max, int64_t B, const int64_t* seg_off, const double* coeffs,
                                     const double* times, const double* t_query, int64_t t_stride, int64_t M,
                                     int derivative_begin, int n_derivatives, double* out, uint8_t* in_range,
                                     int32_t* status, hipStream_t stream);

// evaluateRange
hipError_t launch_eval_count(int N, int D, int K, int64_t B, const double* times, double t_start,
                             double t_end, double dt, int64_t* counts, hipStream_t stream);
// run-table workspace of launch_eval_range (bytes; *cap = runs stored per trajectory)
size_t eval_workspace_bytes(int K, int64_t B, int* cap);
// Samples of every trajectory (one block each).  Without runs_ready the run table is built first
// (eval_runs_kernel); with runs_ready, launch_eval_runs_counts already built it together with the
// counts and the two-level offsets: offsets then holds the in-block prefix and the kernel writes the
// final offsets to offsets_out.  A trajectory whose samples would end past `capacity` samples is
// not written, and none is when the device-side `total` (nullable) exceeds it.
hipError_t launch_eval_range(int N, int D, int K, int64_t B, const double* coeffs,
                             const double* times, double t_start, double t_end, double dt,
                             int derivative, const int64_t* counts, const int64_t* offsets, double* out,
                             double* sample_times, void* ws, int cap, hipStream_t stream, bool runs_ready = false,
                             int64_t* offsets_out = nullptr, int64_t capacity = INT64_MAX,
                             const int64_t* total = nullptr);
// The one-call evaluateRange's first two kernels: the run table plus counts[B] and the in-block
// offsets (eval_runs_kernel), then the block offsets and the grand total (eval_scan_kernel); all
// device-side, no host round trip.  Workspace: eval_full_workspace_bytes.
size_t eval_full_workspace_bytes(int K, int64_t B, int* cap);
hipError_t launch_eval_runs_counts(int K, int64_t B, const double* times, double t_start, double t_end, double dt,
                                   int64_t* counts, int64_t* offsets, void* ws, int cap, int64_t* total,
                                   hipStream_t stream);
// eval_scan_kernel alone (mtg_eval.hip): nb block totals in bsum, scanned in place, and the grand total
void launch_eval_scan(int64_t nb, int64_t* bsum, int64_t* total, hipStream_t stream);

// evaluateRange on a CSR batch (mtg_eval_ragged.hip): the same three launches, with trajectory b's
// segments at seg_off[b] .. seg_off[b + 1] of coeffs [sum K][D][N] and times [sum K].  The workspace
// is that of the uniform launches (it does not depend on K).
struct EvalRagged {
  const int64_t* seg_off;  // [B + 1], a device array
  int K_max;               // the largest K_b: it sizes the sample kernels' LDS and picks among them
  int64_t clock_slice;     // eval_ragged_clock_slice of the (host) offsets
};
// The clock kernels' staging rule: the most segments of any 32-trajectory block, from the host copy of
// seg_off; the times are staged in LDS when that is at most 32 * 256, else read from global memory.
int64_t eval_ragged_clock_slice(const int64_t* seg_off, int64_t B);
bool eval_ragged_clock_staged(int64_t clock_slice);
// hipErrorInvalidValue when the sample kernels' LDS at K segments does not fit (launch_eval_range's
// error at that K), without launching anything
hipError_t eval_range_lds_check(int N, int D, int K);
hipError_t launch_eval_count_ragged(const EvalRagged& r, int64_t B, const double* times, double t_start, double t_end,
                                    double dt, int64_t* counts, hipStream_t stream);
hipError_t launch_eval_runs_counts_ragged(const EvalRagged& r, int64_t B, const double* times, double t_start,
                                          double t_end, double dt, int64_t* counts, int64_t* offsets, void* ws, int cap,
                                          int64_t* total, hipStream_t stream);
hipError_t launch_eval_range_ragged(int N, int D, const EvalRagged& r, int64_t B, const double* coeffs,
                                    const double* times, double t_start, double t_end, double dt, int derivative,
                                    const int64_t* counts, const int64_t* offsets, double* out, double* sample_times,
                                    void* ws, int cap, hipStream_t stream, bool runs_ready = false,
                                    int64_t* offsets_out = nullptr, int64_t capacity = INT64_MAX,
                                    const int64_t* total = nullptr);

}  // namespace mtg
