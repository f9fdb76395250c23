// mtg_evaluate_at.hip -- batched Trajectory::evaluate (src/trajectory.cpp:41-66) at caller-given
// query times for a batch of one segment count K.  The definition is in include/mtg.h
// (mtg_evaluate_at_batch); DESIGN.md 3.13.  The kernels are mtg_evaluate_at.inc, instantiated here for
// uniform K (the CSR form is mtg_evaluate_at_ragged.hip); this file keeps the rule that picks the
// mapping.
#include "mtg_evaluate_at.inc"

namespace mtg {

// The one rule that picks the mapping.  Staged when a block's queries repay staging the whole
// trajectory: M >= max(32, K) -- per query the staged mapping reads K D N / min(M, chunk)
// coefficients and the lane mapping D N, so staging reads less from M = K on, and below 32 queries
// a staged block would leave most of its first wave idle -- and the staged block's LDS fits;
// otherwise a lane per query.  The block shrinks (256, 128, 64 threads) until its LDS fits.
bool evaluate_at_plan(int N, int D, int K, int64_t M, int nd, EvalAtPlan* p) {
  const int64_t W = (int64_t)nd * D;
  if (W > (int64_t)(kAtMaxLds / 8 / 64)) return false;  // a 64-thread block's rows do not fit
  if (M >= 32 && M >= K) {
    int T = M <= 64 ? 64 : (M <= 128 ? 128 : kAtMaxThreads);
    const size_t fixed = sizeof(double) * ((size_t)K * D * N + 2 * (size_t)K + 1);
    while (T > 64 && fixed + sizeof(double) * T * W > kAtMaxLds) T >>= 1;
    if (fixed + sizeof(double) * T * W <= kAtMaxLds) {
      *p = EvalAtPlan{MTG_EVALUATE_AT_STAGED, T, fixed + sizeof(double) * T * W};
      return true;
    }
  }
  int T = kAtMaxThreads;
  while (T > 64 && sizeof(double) * T * W > kAtMaxLds) T >>= 1;
  *p = EvalAtPlan{MTG_EVALUATE_AT_LANE, T, sizeof(double) * T * (size_t)W};
  return true;
}

hipError_t launch_evaluate_at(int N, int D, int K, int64_t B, const double* coeffs, const double* times,
                              const double* t_query, int64_t t_stride, int64_t M, int derivative_begin,
                              int n_derivatives, double* out, uint8_t* in_range, int32_t* status, hipStream_t stream) {
  return launch_at<false>(N, D, K, B, coeffs, times, t_query, t_stride, M, derivative_begin, n_derivatives, out,
                          in_range, status, EvalAtArgs{}, stream);
}

}  // namespace mtg
