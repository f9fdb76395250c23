// mtg_evaluate_at_ragged.hip -- batched Trajectory::evaluate at caller-given query times for a batch
// whose trajectories have different segment counts (mtg_evaluate_at_ragged_batch, include/mtg.h;
// DESIGN.md 3.15).  The kernels are those of mtg_evaluate_at.inc with the CSR indirection: a
// trajectory's coefficients and times are read where they lie, nothing is copied.  A unit of its own,
// so that mtg_evaluate_at.hip holds the uniform kernels and nothing else.
#include "mtg_evaluate_at.inc"

namespace mtg {

// K_max: the largest segment count of the batch (it picks the mapping and sizes the staged block's
// LDS: evaluate_at_plan(N, D, K_max, M, n_derivatives)); seg_off [B + 1] on the device.
hipError_t launch_evaluate_at_ragged(int N, int D, int K_max, int64_t B, const int64_t* seg_off, const double* coeffs,
                                     const double* times, const double* t_query, int64_t t_stride, int64_t M,
                                     int derivative_begin, int n_derivatives, double* out, uint8_t* in_range,
                                     int32_t* status, hipStream_t stream) {
  EvalAtRaggedArgs a{};
  a.seg_off = seg_off;
  return launch_at<true>(N, D, K_max, B, coeffs, times, t_query, t_stride, M, derivative_begin, n_derivatives, out,
                         in_range, status, a, stream);
}

}  // namespace mtg
