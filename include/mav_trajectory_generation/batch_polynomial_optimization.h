// batch_polynomial_optimization.h -- BatchPolynomialOptimization<N>: B independent problems of one
// shape (N, D, K, r) per call, on the GPU.  This is the throughput API the library exists for
// (BASELINE configs 2-5); the reference has no batched form -- its callers loop over
// PolynomialOptimization<N> (src/polynomial_timing_evaluation.cpp:119-126).
//
// Arrays are in the C ABI layout (include/mtg.h): values [B][K+1][N/2][D], mask [B][K+1] (bit k:
// derivative k fixed), times [B][K], coeffs [B][K][D][N].  Pass MTG_FLAG_DEVICE_PTRS to hand over
// device pointers (inputs already in HBM); host pointers are staged by the library.
// solveRagged takes problems of different segment counts in one call (CSR arrays, include/mtg.h
// mtg_solve_linear_ragged_batch), and evaluateAtRagged / minMaxMagnitudeRagged / evaluateRangeRagged /
// vertexDerivativesRagged / coefficientsFromVerticesRagged / collisionCostRagged
// consume its coefficients in the same layout: the entries here that are not tied to the object's K.
//
// Several devices: construct with a device list (e.g. allDevices()).  A host-array solve() is then
// one mtg_solve_linear_batch_multi call: contiguous shards of the batch, one host thread and one
// context per device, no collective; bit-identical to a one-device solve.  Device-
// pointer calls and the other entry points run on the first device.
#ifndef MAV_TRAJECTORY_GENERATION_BATCH_POLYNOMIAL_OPTIMIZATION_H_
#define MAV_TRAJECTORY_GENERATION_BATCH_POLYNOMIAL_OPTIMIZATION_H_

#include <cstdint>
#include <vector>

#include "mav_trajectory_generation/runtime.h"
#include "mav_trajectory_generation/vertex.h"

namespace mav_trajectory_generation {

// Pack one Vertex::Vector into the ABI layout: values [V][h][D] (fixed derivatives), mask [V];
// orders >= h are dropped with a warning and flagged in bit 7 (the solver then reports
// MTG_TRAJ_WARN_DROPPED), as setupFromVertices does (lin_impl:74-95).
inline void packVertices(const Vertex::Vector& vertices, int N, int D, double* values, uint8_t* mask) {
  const int h = N / 2;
  const int V = (int)vertices.size();
  for (size_t i = 0; i < (size_t)V * h * D; ++i) values[i] = 0.0;
  for (int v = 0; v < V; ++v) {
    if (vertices[v].D() != D) fail(MTG_ERR_SIZE_MISMATCH, "vertex dimension mismatch");
    unsigned m = 0;
    for (auto it = vertices[v].cBegin(); it != vertices[v].cEnd(); ++it) {
      const int k = it->first;
      if (k < 0) continue;
      if (k >= h) {
        m |= 0x80u;
        continue;
      }
      m |= 1u << k;
      for (int d = 0; d < D; ++d) values[((size_t)v * h + k) * D + d] = it->second[d];
    }
    mask[v] = (uint8_t)m;
  }
}

template <int _N = 10>
class BatchPolynomialOptimization {
  static_assert(_N % 2 == 0 && _N >= 2 && _N <= 12, "N must be even and in [2, 12]");

 public:
  enum { N = _N };
  BatchPolynomialOptimization(int dimension, int segments, int derivative_to_optimize, int device = 0)
      : BatchPolynomialOptimization(dimension, segments, derivative_to_optimize, std::vector<int>{device}) {}
  BatchPolynomialOptimization(int dimension, int segments, int derivative_to_optimize, const std::vector<int>& devices)
      : D_(dimension), K_(segments), r_(derivative_to_optimize) {
    if (devices.empty()) fail(MTG_ERR_INVALID_ARGUMENT, "BatchPolynomialOptimization: no device");
    for (int device : devices) {
      mtg_ctx* c = nullptr;
      const int rc = mtg_create(device, &c);
      if (rc != MTG_OK) {
        for (mtg_ctx* o : ctxs_) mtg_destroy(o);
        ctxs_.clear();
        check(rc, nullptr, "mtg_create");
      }
      ctxs_.push_back(c);
    }
    ctx_ = ctxs_.front();
  }
  ~BatchPolynomialOptimization() {
    for (mtg_ctx* c : ctxs_) mtg_destroy(c);
  }
  // every visible device: 0 .. mtg_device_count() - 1
  static std::vector<int> allDevices() {
    int n = 0;
    check(mtg_device_count(&n), nullptr, "mtg_device_count");
    std::vector<int> d(n);
    for (int i = 0; i < n; ++i) d[i] = i;
    return d;
  }
  int numDevices() const { return (int)ctxs_.size(); }
  BatchPolynomialOptimization(const BatchPolynomialOptimization&) = delete;
  BatchPolynomialOptimization& operator=(const BatchPolynomialOptimization&) = delete;

  int dimension() const { return D_; }
  int segments() const { return K_; }
  int derivativeToOptimize() const { return r_; }
  mtg_ctx* context() const { return ctx_; }

  // setupFromVertices + solveLinear + getSegments / computeCost per problem (mtg_solve_linear_batch)
  void solve(int64_t batch, const double* values, const uint8_t* mask, const double* times, double* coeffs,
             double* cost = nullptr, int32_t* status = nullptr, unsigned flags = 0, double* free_out = nullptr,
             int32_t* n_free = nullptr) {
    if (ctxs_.size() > 1 && !(flags & (MTG_FLAG_DEVICE_PTRS | MTG_FLAG_ASYNC))) {
      check(mtg_solve_linear_batch_multi(ctxs_.data(), (int)ctxs_.size(), N, D_, K_, r_, batch, values, mask, times,
                                         coeffs, free_out, n_free, cost, status, flags),
            ctx_, "mtg_solve_linear_batch_multi");
      return;
    }
    check(mtg_solve_linear_batch(ctx_, N, D_, K_, r_, batch, values, mask, times, coeffs, free_out, n_free, cost,
                                 status, flags),
          ctx_, "mtg_solve_linear_batch");
  }
  // Problems given as Vertex lists (one per problem, all with K + 1 vertices) and segment times.
  void solve(const std::vector<Vertex::Vector>& problems, const std::vector<std::vector<double>>& times,
             std::vector<double>* coeffs, std::vector<double>* cost = nullptr, std::vector<int32_t>* status = nullptr) {
    const int64_t B = (int64_t)problems.size();
    const int V = K_ + 1, h = N / 2;
    if ((int64_t)times.size() != B) fail(MTG_ERR_SIZE_MISMATCH, "one segment-time vector per problem");
    std::vector<double> vals((size_t)B * V * h * D_), t((size_t)B * K_);
    std::vector<uint8_t> mask((size_t)B * V);
    for (int64_t b = 0; b < B; ++b) {
      if ((int)problems[b].size() != V || (int)times[b].size() != K_)
        fail(MTG_ERR_SIZE_MISMATCH, "every problem needs K + 1 vertices and K segment times");
      packVertices(problems[b], N, D_, vals.data() + (size_t)b * V * h * D_, mask.data() + (size_t)b * V);
      for (int i = 0; i < K_; ++i) t[(size_t)b * K_ + i] = times[b][i];
    }
    check_notnull(coeffs, "coeffs")->assign((size_t)B * K_ * D_ * N, 0.0);
    if (cost) cost->assign((size_t)B, 0.0);
    if (status) status->assign((size_t)B, 0);
    solve(B, vals.data(), mask.data(), t.data(), coeffs->data(), cost ? cost->data() : nullptr,
          status ? status->data() : nullptr);
  }
  // The same for problems of different segment counts (mtg_solve_linear_ragged_batch): seg_count [batch]
  // is a host array also with MTG_FLAG_DEVICE_PTRS, the other arrays are the CSR arrays of include/mtg.h
  // (trajectory b at vertex offset sum_{j<b} (K_j + 1) and segment offset sum_{j<b} K_j).  The object's
  // `segments` is not used; runs on the first device.
  void solveRagged(int64_t batch, const int32_t* seg_count, const double* values, const uint8_t* mask,
                   const double* times, double* coeffs, double* cost = nullptr, int32_t* status = nullptr,
                   unsigned flags = 0, double* free_out = nullptr, int32_t* n_free = nullptr) {
    check(mtg_solve_linear_ragged_batch(ctx_, N, D_, r_, batch, seg_count, values, mask, times, coeffs, free_out,
                                        n_free, cost, status, flags),
          ctx_, "mtg_solve_linear_ragged_batch");
  }
  // Problems given as Vertex lists of any length >= 2 each, with their segment times.  coeffs receives
  // [sum K][D][N]; problem b's segments start at (*segment_offsets)[b] (B + 1 entries, the last the total).
  void solveRagged(const std::vector<Vertex::Vector>& problems, const std::vector<std::vector<double>>& times,
                   std::vector<double>* coeffs, std::vector<int64_t>* segment_offsets = nullptr,
                   std::vector<double>* cost = nullptr, std::vector<int32_t>* status = nullptr) {
    const int64_t B = (int64_t)problems.size();
    const int h = N / 2;
    if ((int64_t)times.size() != B) fail(MTG_ERR_SIZE_MISMATCH, "one segment-time vector per problem");
    std::vector<int32_t> seg((size_t)B);
    std::vector<int64_t> so((size_t)B + 1, 0);
    for (int64_t b = 0; b < B; ++b) {
      if (problems[b].size() < 2 || times[b].size() + 1 != problems[b].size())
        fail(MTG_ERR_SIZE_MISMATCH, "every problem needs V >= 2 vertices and V - 1 segment times");
      seg[b] = (int32_t)times[b].size();
      so[b + 1] = so[b] + seg[b];
    }
    const size_t totS = (size_t)so[B], totV = totS + (size_t)B;
    std::vector<double> vals(totV * h * D_), t(totS);
    std::vector<uint8_t> mask(totV);
    for (int64_t b = 0; b < B; ++b) {
      const size_t v0 = (size_t)(so[b] + b);
      packVertices(problems[b], N, D_, vals.data() + v0 * h * D_, mask.data() + v0);
      for (int i = 0; i < seg[b]; ++i) t[(size_t)so[b] + i] = times[b][i];
    }
    check_notnull(coeffs, "coeffs")->assign(totS * D_ * N, 0.0);
    if (cost) cost->assign((size_t)B, 0.0);
    if (status) status->assign((size_t)B, 0);
    solveRagged(B, seg.data(), vals.data(), mask.data(), t.data(), coeffs->data(), cost ? cost->data() : nullptr,
                status ? status->data() : nullptr);
    if (segment_offsets) *segment_offsets = so;
  }
  // time-allocation sweep: optimal cost at scale[c] * times (mtg_time_sweep_batch)
  void timeSweep(int64_t batch, const double* values, const uint8_t* mask, const double* times, int n_candidates,
                 const double* scales, double* cost, int32_t* status = nullptr, unsigned flags = 0) {
    check(mtg_time_sweep_batch(ctx_, N, D_, K_, r_, batch, values, mask, times, n_candidates, scales, cost, status,
                               flags),
          ctx_, "mtg_time_sweep_batch");
  }
  // config 5: cost sweep + segment-time Jacobian on the matrix cores (mtg_time_jacobian_batch)
  void timeJacobian(int64_t batch, const double* vertex_values, const double* times, int n_candidates,
                    const double* scales, double* cost, double* jac, double increment_time = 0.0,
                    unsigned flags = 0) {
    check(mtg_time_jacobian_batch(ctx_, N, D_, K_, r_, batch, vertex_values, times, n_candidates, scales,
                                  increment_time, cost, jac, flags),
          ctx_, "mtg_time_jacobian_batch");
  }
  // cost (and gradient) of fixed vertex derivatives at candidate times (mtg_cost_at_times_batch)
  void costAtTimes(int64_t batch, const double* vertex_values, const uint8_t* mask, const double* times,
                   int n_candidates, const double* scales, double* cost, double* grad = nullptr, unsigned flags = 0) {
    check(mtg_cost_at_times_batch(ctx_, N, D_, K_, r_, batch, vertex_values, mask, times, n_candidates, scales, cost,
                                  grad, flags),
          ctx_, "mtg_cost_at_times_batch");
  }
  // collision cost (and gradient, packed as costAtTimes' grad) over a signed distance field
  // (mtg_collision_cost_batch: getCostAndGradientCollision, nl_impl:1523-1709); D must be 3
  void collisionCost(int64_t batch, const double* vertex_values, const uint8_t* mask, const double* times,
                     const mtg_sdf_grid& grid, const mtg_collision_params& params, double* cost, double* grad = nullptr,
                     uint8_t* is_collision = nullptr, int32_t* n_evaluated = nullptr, int32_t* status = nullptr,
                     unsigned flags = 0) {
    check(mtg_collision_cost_batch(ctx_, N, D_, K_, batch, vertex_values, mask, times, &grid, &params, cost, grad,
                                   is_collision, n_evaluated, status, flags),
          ctx_, "mtg_collision_cost_batch");
  }
  // segment-time gradient of the collision cost, grad_t [B][K] (mtg_collision_time_gradient_batch: the
  // dJc_dt part of getCostAndGradientTime, nl_impl:2155-2243); D must be 3
  void collisionTimeGradient(int64_t batch, const double* vertex_values, const double* times, const mtg_sdf_grid& grid,
                             const mtg_collision_params& params, double* grad_t, double increment_time = 0.1,
                             double* side_cost = nullptr, int32_t* side_evaluated = nullptr,
                             int32_t* segments_walked = nullptr, int32_t* status = nullptr, unsigned flags = 0) {
    check(mtg_collision_time_gradient_batch(ctx_, N, D_, K_, batch, vertex_values, times, &grid, &params,
                                            increment_time, grad_t, side_cost, side_evaluated, segments_walked, status,
                                            flags),
          ctx_, "mtg_collision_time_gradient_batch");
  }
  // The complete getCostAndGradientTime (nl_impl:2155-2243) of host arrays: J_t [B] = sum_i T_i and
  // grad_t [B][K] = (w_d dJd_dt + w_c dJc_dt) + w_t, composed of timeJacobian (one candidate, scales of
  // 1, the same increment_time) and collisionTimeGradient; the reference's default weights are 0.1, 10,
  // 1.  Its w_sc dJsc_dt is 0 by its own code (updateSegmentTimes does not rebuild the segments the
  // soft-constraint term reads) and is left out.  djd_dt / djc_dt [B][K] (nullable) receive the parts.
  void timeGradient(int64_t batch, const double* vertex_values, const double* times, const mtg_sdf_grid& grid,
                    const mtg_collision_params& params, double w_d, double w_c, double w_t, double* J_t, double* grad_t,
                    double increment_time = 0.1, double* djd_dt = nullptr, double* djc_dt = nullptr,
                    int32_t* status = nullptr) {
    const size_t n = (size_t)batch * K_;
    std::vector<double> ones((size_t)K_, 1.0), cost((size_t)batch), jd(n), jc(n);
    timeJacobian(batch, vertex_values, times, 1, ones.data(), cost.data(), jd.data(), increment_time);
    collisionTimeGradient(batch, vertex_values, times, grid, params, jc.data(), increment_time, nullptr, nullptr, nullptr,
                          status);
    for (int64_t b = 0; b < batch; ++b) {
      double sum = 0.0;
      for (int i = 0; i < K_; ++i) sum += times[(size_t)b * K_ + i];
      if (J_t) J_t[b] = sum;
    }
    for (size_t i = 0; i < n; ++i) {
      grad_t[i] = (w_d * jd[i] + w_c * jc[i]) + w_t;
      if (djd_dt) djd_dt[i] = jd[i];
      if (djc_dt) djc_dt[i] = jc[i];
    }
  }
  // soft-constraint cost of the magnitude limits (and gradient, packed as costAtTimes' grad)
  // (mtg_soft_constraint_cost_batch: getCostAndGradientSoftConstraints, nl_impl:2025-2091); D <= 4
  void softConstraintCost(int64_t batch, const double* vertex_values, const uint8_t* mask, const double* times,
                          const mtg_soft_constraint_params& params, double* cost, double* grad = nullptr,
                          mtg_extremum* maxima = nullptr, int32_t* status = nullptr, unsigned flags = 0) {
    check(mtg_soft_constraint_cost_batch(ctx_, N, D_, K_, batch, vertex_values, mask, times, &params, cost, grad,
                                         maxima, status, flags),
          ctx_, "mtg_soft_constraint_cost_batch");
  }
  // The reference's nonlinear objective in the optimiser's variables, one cost and one gradient per
  // trajectory (mtg_objective_batch: objectiveFunctionFreeConstraints[AndCollision[AndTime]],
  // nl_impl:909-1449).  x [B][x_stride]: (objective 2: the K times, then) D blocks of n_free[b] free
  // derivatives; params.derivative_to_optimize is set to this object's.  grid / collision NULL for
  // objective 0, soft NULL iff !params.use_soft_constraints, times NULL for objective 2.
  void objective(int64_t batch, const double* values, const uint8_t* mask, const double* times, const double* x,
                 int64_t x_stride, mtg_objective_params params, const mtg_sdf_grid* grid,
                 const mtg_collision_params* collision, const mtg_soft_constraint_params* soft, double* cost,
                 double* grad = nullptr, double* weighted_costs = nullptr, uint8_t* is_collision = nullptr,
                 mtg_objective_state* state = nullptr, const mtg_objective_parts* parts = nullptr,
                 int32_t* status = nullptr, unsigned flags = 0) {
    params.derivative_to_optimize = r_;
    check(mtg_objective_batch(ctx_, N, D_, K_, batch, values, mask, times, x, x_stride, &params, grid, collision, soft,
                              cost, grad, weighted_costs, is_collision, state, parts, status, flags),
          ctx_, "mtg_objective_batch");
  }
  // The two gradient-free objectives in the segment times, one cost per trajectory
  // (mtg_objective_time_batch: objectiveFunctionTime, nl_impl:765-832, and
  // objectiveFunctionTimeAndConstraints, :835-906).  x [B][x_stride]: the K times (objective 4: then D
  // blocks of n_free[b] free derivatives); params.derivative_to_optimize is set to this object's.
  // coeff_times / grid / collision iff objective 3 with w_c > 0; constraints NULL only with the soft
  // constraints off and neither constraint_values nor maxima requested.
  void objectiveTime(int64_t batch, const double* values, const uint8_t* mask, const double* x, int64_t x_stride,
                     mtg_objective_time_params params, const double* coeff_times, const mtg_sdf_grid* grid,
                     const mtg_collision_params* collision, const mtg_soft_constraint_params* constraints, double* cost,
                     double* weighted_costs = nullptr, uint8_t* is_collision = nullptr,
                     double* constraint_values = nullptr, mtg_extremum* maxima = nullptr, double* free = nullptr,
                     double* coeffs = nullptr, mtg_objective_state* state = nullptr,
                     const mtg_objective_parts* parts = nullptr, int32_t* status = nullptr, unsigned flags = 0) {
    params.derivative_to_optimize = r_;
    check(mtg_objective_time_batch(ctx_, N, D_, K_, batch, values, mask, x, x_stride, &params, coeff_times, grid,
                                   collision, constraints, cost, weighted_costs, is_collision, constraint_values, maxima,
                                   free, coeffs, state, parts, status, flags),
          ctx_, "mtg_objective_time_batch");
  }
  void coefficientsFromVertices(int64_t batch, const double* vertex_values, const double* times, double* coeffs,
                                unsigned flags = 0) {
    check(mtg_coefficients_from_vertices_batch(ctx_, N, D_, K_, batch, vertex_values, times, coeffs, flags), ctx_,
          "mtg_coefficients_from_vertices_batch");
  }
  void vertexDerivatives(int64_t batch, const double* coeffs, const double* times, double* vertex_values,
                         unsigned flags = 0) {
    check(mtg_vertex_derivatives_batch(ctx_, N, D_, K_, batch, coeffs, times, vertex_values, flags), ctx_,
          "mtg_vertex_derivatives_batch");
  }
  void minMaxMagnitude(int64_t batch, const double* coeffs, const double* times, int derivative,
                       uint32_t dimension_mask, mtg_extremum* minimum, mtg_extremum* maximum, unsigned flags = 0) {
    check(mtg_min_max_magnitude_batch(ctx_, N, D_, K_, batch, coeffs, times, derivative, dimension_mask, minimum,
                                      maximum, flags),
          ctx_, "mtg_min_max_magnitude_batch");
  }
  // Trajectory::evaluateRange over the batch (mtg_evaluate_range_batch): counts [B]; then samples
  // [sum counts][D] (+ sampling times) at offsets (exclusive prefix sum of counts).
  void evaluateRangeCounts(int64_t batch, const double* times, double t_start, double t_end, double dt,
                           int64_t* counts, unsigned flags = 0) {
    check(mtg_evaluate_range_batch(ctx_, N, D_, K_, batch, nullptr, times, t_start, t_end, dt, 0, counts, nullptr,
                                   nullptr, nullptr, flags),
          ctx_, "mtg_evaluate_range_batch(count)");
  }
  void evaluateRange(int64_t batch, const double* coeffs, const double* times, double t_start, double t_end,
                     double dt, int derivative, int64_t* counts, const int64_t* offsets, double* out,
                     double* sampling_times = nullptr, unsigned flags = 0) {
    check(mtg_evaluate_range_batch(ctx_, N, D_, K_, batch, coeffs, times, t_start, t_end, dt, derivative, counts,
                                   offsets, out, sampling_times, flags),
          ctx_, "mtg_evaluate_range_batch");
  }
  // Trajectory::evaluate of every trajectory at its own query times (mtg_evaluate_at_batch): the time of
  // trajectory b's query m is t_query[b * t_stride + m] (t_stride 0: one row of M times for the whole
  // batch); out [B][M][n_derivatives][D] holds orders derivative_begin .. derivative_begin +
  // n_derivatives - 1, in_range [B][M] whether the time lies inside the trajectory.
  void evaluateAt(int64_t batch, const double* coeffs, const double* times, const double* t_query, int64_t t_stride,
                  int64_t M, int derivative_begin, int n_derivatives, double* out, uint8_t* in_range = nullptr,
                  int32_t* status = nullptr, unsigned flags = 0) {
    check(mtg_evaluate_at_batch(ctx_, N, D_, K_, batch, coeffs, times, t_query, t_stride, M, derivative_begin,
                                n_derivatives, out, in_range, status, flags),
          ctx_, "mtg_evaluate_at_batch");
  }
  // evaluateAt and minMaxMagnitude for trajectories of different segment counts
  // (mtg_evaluate_at_ragged_batch, mtg_min_max_magnitude_ragged_batch): coeffs [sum K][D][N] and times
  // [sum K] are the CSR arrays solveRagged writes and takes, seg_count [batch] a host array also with
  // MTG_FLAG_DEVICE_PTRS; the other arguments are those of the uniform members.  Every trajectory's
  // outputs are the bytes the uniform member gives for it alone.  The object's `segments` is not used.
  void evaluateAtRagged(int64_t batch, const int32_t* seg_count, const double* coeffs, const double* times,
                        const double* t_query, int64_t t_stride, int64_t M, int derivative_begin, int n_derivatives,
                        double* out, uint8_t* in_range = nullptr, int32_t* status = nullptr, unsigned flags = 0) {
    check(mtg_evaluate_at_ragged_batch(ctx_, N, D_, batch, seg_count, coeffs, times, t_query, t_stride, M,
                                       derivative_begin, n_derivatives, out, in_range, status, flags),
          ctx_, "mtg_evaluate_at_ragged_batch");
  }
  void minMaxMagnitudeRagged(int64_t batch, const int32_t* seg_count, const double* coeffs, const double* times,
                             int derivative, uint32_t dimension_mask, mtg_extremum* minimum, mtg_extremum* maximum,
                             unsigned flags = 0) {
    check(mtg_min_max_magnitude_ragged_batch(ctx_, N, D_, batch, seg_count, coeffs, times, derivative, dimension_mask,
                                             minimum, maximum, flags),
          ctx_, "mtg_min_max_magnitude_ragged_batch");
  }
  // evaluateRangeCounts and evaluateRange for trajectories of different segment counts
  // (mtg_evaluate_range_ragged_batch), on the same CSR arrays: counts [batch]; then the samples
  // [sum counts][D] (+ sampling times) at offsets.  Every trajectory's count, samples and sampling times
  // are the bytes the uniform members give for it alone.
  void evaluateRangeRaggedCounts(int64_t batch, const int32_t* seg_count, const double* times, double t_start,
                                 double t_end, double dt, int64_t* counts, unsigned flags = 0) {
    check(mtg_evaluate_range_ragged_batch(ctx_, N, D_, batch, seg_count, nullptr, times, t_start, t_end, dt, 0, counts,
                                          nullptr, nullptr, nullptr, flags),
          ctx_, "mtg_evaluate_range_ragged_batch(count)");
  }
  void evaluateRangeRagged(int64_t batch, const int32_t* seg_count, const double* coeffs, const double* times,
                           double t_start, double t_end, double dt, int derivative, int64_t* counts,
                           const int64_t* offsets, double* out, double* sampling_times = nullptr, unsigned flags = 0) {
    check(mtg_evaluate_range_ragged_batch(ctx_, N, D_, batch, seg_count, coeffs, times, t_start, t_end, dt, derivative,
                                          counts, offsets, out, sampling_times, flags),
          ctx_, "mtg_evaluate_range_ragged_batch");
  }

  // The two vertex <-> coefficient maps and the collision cost for trajectories of different segment
  // counts (mtg_vertex_derivatives_ragged_batch, mtg_coefficients_from_vertices_ragged_batch,
  // mtg_collision_cost_ragged_batch) on the same CSR arrays: vertex_values [sum K + batch][h][D] and mask
  // [sum K + batch] hold trajectory b's V_b rows at so[b] + b, grad is its block [3][V_b h] at double
  // offset 3 h (so[b] + b) (solveRagged's free layout), cost / is_collision / n_evaluated / status are
  // [batch].  Every trajectory's outputs are the bytes the uniform member gives for it alone; the maps
  // have no limit on K.  The object's `segments` is not used.
  void vertexDerivativesRagged(int64_t batch, const int32_t* seg_count, const double* coeffs, const double* times,
                               double* vertex_values, unsigned flags = 0) {
    check(mtg_vertex_derivatives_ragged_batch(ctx_, N, D_, batch, seg_count, coeffs, times, vertex_values, flags), ctx_,
          "mtg_vertex_derivatives_ragged_batch");
  }
  void coefficientsFromVerticesRagged(int64_t batch, const int32_t* seg_count, const double* vertex_values,
                                      const double* times, double* coeffs, unsigned flags = 0) {
    check(mtg_coefficients_from_vertices_ragged_batch(ctx_, N, D_, batch, seg_count, vertex_values, times, coeffs,
                                                      flags),
          ctx_, "mtg_coefficients_from_vertices_ragged_batch");
  }
  void collisionCostRagged(int64_t batch, const int32_t* seg_count, const double* vertex_values, const uint8_t* mask,
                           const double* times, const mtg_sdf_grid& grid, const mtg_collision_params& params,
                           double* cost, double* grad = nullptr, uint8_t* is_collision = nullptr,
                           int32_t* n_evaluated = nullptr, int32_t* status = nullptr, unsigned flags = 0) {
    check(mtg_collision_cost_ragged_batch(ctx_, N, D_, batch, seg_count, vertex_values, mask, times, &grid, &params,
                                          cost, grad, is_collision, n_evaluated, status, flags),
          ctx_, "mtg_collision_cost_ragged_batch");
  }

 private:
  int D_, K_, r_;
  std::vector<mtg_ctx*> ctxs_;
  mtg_ctx* ctx_ = nullptr;
};

// getCostAndGradientCollision for trajectories of N coefficients and K segments in three dimensions,
// without a BatchPolynomialOptimization object: on the library's host path
// (mtg_host_collision_cost_batch) unless the execution policy is kDevice, as the single-problem
// calls of PolynomialOptimization<N> (runtime.h).  Host pointers.
template <int N>
inline void collisionCost(int K, int64_t batch, const double* vertex_values, const uint8_t* mask, const double* times,
                          const mtg_sdf_grid& grid, const mtg_collision_params& params, double* cost,
                          double* grad = nullptr, uint8_t* is_collision = nullptr, int32_t* n_evaluated = nullptr,
                          int32_t* status = nullptr) {
  if (singleOnDevice()) {
    mtg_ctx* ctx = defaultContext();
    check(mtg_collision_cost_batch(ctx, N, 3, K, batch, vertex_values, mask, times, &grid, &params, cost, grad,
                                   is_collision, n_evaluated, status, 0),
          ctx, "mtg_collision_cost_batch");
  } else {
    check(mtg_host_collision_cost_batch(N, 3, K, batch, vertex_values, mask, times, &grid, &params, cost, grad,
                                        is_collision, n_evaluated, status, 1),
          nullptr, "mtg_host_collision_cost_batch");
  }
}

// The collision part dJc_dt of getCostAndGradientTime (mtg_collision_time_gradient_batch) without a
// BatchPolynomialOptimization object: on the library's host path
// (mtg_host_collision_time_gradient_batch, which has no segments_walked diagnostic) unless the
// execution policy is kDevice, as collisionCost.  Host pointers.
template <int N>
inline void collisionTimeGradient(int K, int64_t batch, const double* vertex_values, const double* times,
                                  const mtg_sdf_grid& grid, const mtg_collision_params& params, double* grad_t,
                                  double increment_time = 0.1, double* side_cost = nullptr,
                                  int32_t* side_evaluated = nullptr, int32_t* status = nullptr) {
  if (singleOnDevice()) {
    mtg_ctx* ctx = defaultContext();
    check(mtg_collision_time_gradient_batch(ctx, N, 3, K, batch, vertex_values, times, &grid, &params, increment_time,
                                            grad_t, side_cost, side_evaluated, nullptr, status, 0),
          ctx, "mtg_collision_time_gradient_batch");
  } else {
    check(mtg_host_collision_time_gradient_batch(N, 3, K, batch, vertex_values, times, &grid, &params, increment_time,
                                                 grad_t, side_cost, side_evaluated, status, 1),
          nullptr, "mtg_host_collision_time_gradient_batch");
  }
}

// getCostAndGradientSoftConstraints for trajectories of N coefficients, K segments and D dimensions,
// without a BatchPolynomialOptimization object: on the library's host path
// (mtg_host_soft_constraint_cost_batch) unless the execution policy is kDevice, as collisionCost.
// Host pointers.
template <int N>
inline void softConstraintCost(int D, int K, int64_t batch, const double* vertex_values, const uint8_t* mask,
                               const double* times, const mtg_soft_constraint_params& params, double* cost,
                               double* grad = nullptr, mtg_extremum* maxima = nullptr, int32_t* status = nullptr) {
  if (singleOnDevice()) {
    mtg_ctx* ctx = defaultContext();
    check(mtg_soft_constraint_cost_batch(ctx, N, D, K, batch, vertex_values, mask, times, &params, cost, grad, maxima,
                                         status, 0),
          ctx, "mtg_soft_constraint_cost_batch");
  } else {
    check(mtg_host_soft_constraint_cost_batch(N, D, K, batch, vertex_values, mask, times, &params, cost, grad, maxima,
                                              status, 1),
          nullptr, "mtg_host_soft_constraint_cost_batch");
  }
}

// The nonlinear objective in the optimiser's variables (mtg_objective_batch) for trajectories of N
// coefficients, K segments and D dimensions, without a BatchPolynomialOptimization object: on the
// library's host path (mtg_host_objective_batch) unless the execution policy is kDevice, as
// collisionCost.  Host pointers.
template <int N>
inline void objective(int D, int K, int64_t batch, const double* values, const uint8_t* mask, const double* times,
                      const double* x, int64_t x_stride, const mtg_objective_params& params, const mtg_sdf_grid* grid,
                      const mtg_collision_params* collision, const mtg_soft_constraint_params* soft, double* cost,
                      double* grad = nullptr, double* weighted_costs = nullptr, uint8_t* is_collision = nullptr,
                      mtg_objective_state* state = nullptr, const mtg_objective_parts* parts = nullptr,
                      int32_t* status = nullptr) {
  if (singleOnDevice()) {
    mtg_ctx* ctx = defaultContext();
    check(mtg_objective_batch(ctx, N, D, K, batch, values, mask, times, x, x_stride, &params, grid, collision, soft, cost,
                              grad, weighted_costs, is_collision, state, parts, status, 0),
          ctx, "mtg_objective_batch");
  } else {
    check(mtg_host_objective_batch(N, D, K, batch, values, mask, times, x, x_stride, &params, grid, collision, soft, cost,
                                   grad, weighted_costs, is_collision, state, parts, status, 1),
          nullptr, "mtg_host_objective_batch");
  }
}

// objectiveFunctionTime / objectiveFunctionTimeAndConstraints (mtg_objective_time_batch) for
// trajectories of N coefficients, K segments and D dimensions, without a BatchPolynomialOptimization
// object: on the library's host path (mtg_host_objective_time_batch) unless the execution policy is
// kDevice, as objective.  Host pointers.
template <int N>
inline void objectiveTime(int D, int K, int64_t batch, const double* values, const uint8_t* mask, const double* x,
                          int64_t x_stride, const mtg_objective_time_params& params, const double* coeff_times,
                          const mtg_sdf_grid* grid, const mtg_collision_params* collision,
                          const mtg_soft_constraint_params* constraints, double* cost, double* weighted_costs = nullptr,
                          uint8_t* is_collision = nullptr, double* constraint_values = nullptr,
                          mtg_extremum* maxima = nullptr, double* free = nullptr, double* coeffs = nullptr,
                          mtg_objective_state* state = nullptr, const mtg_objective_parts* parts = nullptr,
                          int32_t* status = nullptr) {
  if (singleOnDevice()) {
    mtg_ctx* ctx = defaultContext();
    check(mtg_objective_time_batch(ctx, N, D, K, batch, values, mask, x, x_stride, &params, coeff_times, grid, collision,
                                   constraints, cost, weighted_costs, is_collision, constraint_values, maxima, free,
                                   coeffs, state, parts, status, 0),
          ctx, "mtg_objective_time_batch");
  } else {
    check(mtg_host_objective_time_batch(N, D, K, batch, values, mask, x, x_stride, &params, coeff_times, grid, collision,
                                        constraints, cost, weighted_costs, is_collision, constraint_values, maxima, free,
                                        coeffs, state, parts, status, 1),
          nullptr, "mtg_host_objective_time_batch");
  }
}

// Trajectory::evaluate for trajectories of N coefficients, K segments and D dimensions at their own
// query times (mtg_evaluate_at_batch), without a BatchPolynomialOptimization object: on the library's
// host path (mtg_host_evaluate_at_batch) unless the execution policy is kDevice, as collisionCost.
// The same bits as Trajectory::evaluate called in a loop.  Host pointers.
template <int N>
inline void evaluateAt(int D, int K, int64_t batch, const double* coeffs, const double* times, const double* t_query,
                       int64_t t_stride, int64_t M, int derivative_begin, int n_derivatives, double* out,
                       uint8_t* in_range = nullptr, int32_t* status = nullptr) {
  if (singleOnDevice()) {
    mtg_ctx* ctx = defaultContext();
    check(mtg_evaluate_at_batch(ctx, N, D, K, batch, coeffs, times, t_query, t_stride, M, derivative_begin,
                                n_derivatives, out, in_range, status, 0),
          ctx, "mtg_evaluate_at_batch");
  } else {
    check(mtg_host_evaluate_at_batch(N, D, K, batch, coeffs, times, t_query, t_stride, M, derivative_begin,
                                     n_derivatives, out, in_range, status, 1),
          nullptr, "mtg_host_evaluate_at_batch");
  }
}

// Per-segment extrema on a window with the candidate list (mtg_segment_min_max_magnitude_batch,
// mtg_segment_min_max_axis_batch), without a BatchPolynomialOptimization object: coeffs
// [n_segments][D][N] and times [n_segments] carry no trajectory structure, so a uniform batch and the
// CSR arrays of a ragged one are both valid.  On the library's host paths unless the execution policy
// is kDevice, as evaluateAt.  Host pointers; every output is nullable.
template <int N>
inline void segmentMinMaxMagnitude(int D, int64_t n_segments, const double* coeffs, const double* times,
                                   const double* windows, int derivative, uint32_t dimension_mask,
                                   mtg_extremum* minimum, mtg_extremum* maximum, double* candidate_times = nullptr,
                                   int32_t* candidate_count = nullptr, int candidate_capacity = 0,
                                   int32_t* status = nullptr) {
  if (singleOnDevice()) {
    mtg_ctx* ctx = defaultContext();
    check(mtg_segment_min_max_magnitude_batch(ctx, N, D, n_segments, coeffs, times, windows, derivative, dimension_mask,
                                              minimum, maximum, candidate_times, candidate_count, candidate_capacity,
                                              status, 0),
          ctx, "mtg_segment_min_max_magnitude_batch");
  } else {
    check(mtg_host_segment_min_max_magnitude_batch(N, D, n_segments, coeffs, times, windows, derivative, dimension_mask,
                                                   minimum, maximum, candidate_times, candidate_count,
                                                   candidate_capacity, status, 1),
          nullptr, "mtg_host_segment_min_max_magnitude_batch");
  }
}

template <int N>
inline void segmentMinMaxAxis(int D, int64_t n_segments, const double* coeffs, const double* times,
                              const double* windows, int derivative, mtg_extremum* minimum, mtg_extremum* maximum,
                              double* candidate_times = nullptr, int32_t* candidate_count = nullptr,
                              int candidate_capacity = 0, int32_t* status = nullptr) {
  if (singleOnDevice()) {
    mtg_ctx* ctx = defaultContext();
    check(mtg_segment_min_max_axis_batch(ctx, N, D, n_segments, coeffs, times, windows, derivative, minimum, maximum,
                                         candidate_times, candidate_count, candidate_capacity, status, 0),
          ctx, "mtg_segment_min_max_axis_batch");
  } else {
    check(mtg_host_segment_min_max_axis_batch(N, D, n_segments, coeffs, times, windows, derivative, minimum, maximum,
                                              candidate_times, candidate_count, candidate_capacity, status, 1),
          nullptr, "mtg_host_segment_min_max_axis_batch");
  }
}

// evaluateAt<N> and Trajectory::computeMinMaxMagnitude for trajectories of different segment counts in
// the CSR layout (coeffs [sum K][D][N], times [sum K], seg_count [batch]), without a
// BatchPolynomialOptimization object: on the library's host paths unless the execution policy is
// kDevice, as evaluateAt.  Host pointers.
template <int N>
inline void evaluateAtRagged(int D, int64_t batch, const int32_t* seg_count, const double* coeffs, const double* times,
                             const double* t_query, int64_t t_stride, int64_t M, int derivative_begin,
                             int n_derivatives, double* out, uint8_t* in_range = nullptr, int32_t* status = nullptr) {
  if (singleOnDevice()) {
    mtg_ctx* ctx = defaultContext();
    check(mtg_evaluate_at_ragged_batch(ctx, N, D, batch, seg_count, coeffs, times, t_query, t_stride, M,
                                       derivative_begin, n_derivatives, out, in_range, status, 0),
          ctx, "mtg_evaluate_at_ragged_batch");
  } else {
    check(mtg_host_evaluate_at_ragged_batch(N, D, batch, seg_count, coeffs, times, t_query, t_stride, M,
                                            derivative_begin, n_derivatives, out, in_range, status, 1),
          nullptr, "mtg_host_evaluate_at_ragged_batch");
  }
}

template <int N>
inline void minMaxMagnitudeRagged(int D, int64_t batch, const int32_t* seg_count, const double* coeffs,
                                  const double* times, int derivative, uint32_t dimension_mask, mtg_extremum* minimum,
                                  mtg_extremum* maximum) {
  if (singleOnDevice()) {
    mtg_ctx* ctx = defaultContext();
    check(mtg_min_max_magnitude_ragged_batch(ctx, N, D, batch, seg_count, coeffs, times, derivative, dimension_mask,
                                             minimum, maximum, 0),
          ctx, "mtg_min_max_magnitude_ragged_batch");
  } else {
    check(mtg_host_min_max_magnitude_ragged_batch(N, D, batch, seg_count, coeffs, times, derivative, dimension_mask,
                                                  minimum, maximum, 1),
          nullptr, "mtg_host_min_max_magnitude_ragged_batch");
  }
}

// vertexDerivatives, coefficientsFromVertices and collisionCost<N> for trajectories of different segment
// counts in the CSR layout (vertex_values [sum K + batch][h][D], mask [sum K + batch], coeffs
// [sum K][D][N], times [sum K], seg_count [batch]; grad: trajectory b's block [3][V_b h] at double offset
// 3 h (so[b] + b)), without a BatchPolynomialOptimization object: on the library's host paths unless the
// execution policy is kDevice, as collisionCost.  Host pointers.
template <int N>
inline void vertexDerivativesRagged(int D, int64_t batch, const int32_t* seg_count, const double* coeffs,
                                    const double* times, double* vertex_values) {
  if (singleOnDevice()) {
    mtg_ctx* ctx = defaultContext();
    check(mtg_vertex_derivatives_ragged_batch(ctx, N, D, batch, seg_count, coeffs, times, vertex_values, 0), ctx,
          "mtg_vertex_derivatives_ragged_batch");
  } else {
    check(mtg_host_vertex_derivatives_ragged_batch(N, D, batch, seg_count, coeffs, times, vertex_values, 1), nullptr,
          "mtg_host_vertex_derivatives_ragged_batch");
  }
}

template <int N>
inline void coefficientsFromVerticesRagged(int D, int64_t batch, const int32_t* seg_count, const double* vertex_values,
                                           const double* times, double* coeffs) {
  if (singleOnDevice()) {
    mtg_ctx* ctx = defaultContext();
    check(mtg_coefficients_from_vertices_ragged_batch(ctx, N, D, batch, seg_count, vertex_values, times, coeffs, 0), ctx,
          "mtg_coefficients_from_vertices_ragged_batch");
  } else {
    check(mtg_host_coefficients_from_vertices_ragged_batch(N, D, batch, seg_count, vertex_values, times, coeffs, 1),
          nullptr, "mtg_host_coefficients_from_vertices_ragged_batch");
  }
}

template <int N>
inline void collisionCostRagged(int64_t batch, const int32_t* seg_count, const double* vertex_values,
                                const uint8_t* mask, const double* times, const mtg_sdf_grid& grid,
                                const mtg_collision_params& params, double* cost, double* grad = nullptr,
                                uint8_t* is_collision = nullptr, int32_t* n_evaluated = nullptr,
                                int32_t* status = nullptr) {
  if (singleOnDevice()) {
    mtg_ctx* ctx = defaultContext();
    check(mtg_collision_cost_ragged_batch(ctx, N, 3, batch, seg_count, vertex_values, mask, times, &grid, &params, cost,
                                          grad, is_collision, n_evaluated, status, 0),
          ctx, "mtg_collision_cost_ragged_batch");
  } else {
    check(mtg_host_collision_cost_ragged_batch(N, 3, batch, seg_count, vertex_values, mask, times, &grid, &params, cost,
                                               grad, is_collision, n_evaluated, status, 1),
          nullptr, "mtg_host_collision_cost_ragged_batch");
  }
}

}  // namespace mav_trajectory_generation

#endif  // MAV_TRAJECTORY_GENERATION_BATCH_POLYNOMIAL_OPTIMIZATION_H_
