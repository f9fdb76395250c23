// mtg_eval_ragged.hip -- batched Trajectory::evaluateRange for a batch whose trajectories have
// different segment counts (mtg_evaluate_range_ragged_batch, mtg_evaluate_range_ragged_batch_full,
// include/mtg.h).  The kernels are those of mtg_eval.inc with the CSR indirection: a
// trajectory's coefficients and times are read where they lie, nothing is copied.  A unit of its own,
// so that mtg_eval.hip holds the uniform kernels and nothing else.
#include "mtg_eval.inc"

namespace mtg {

// The one rule for the clock kernels' segment times, from the segment offsets alone: the largest number
// of segments any 32-trajectory block of the clock kernels holds.  The launch stages the times in LDS
// when that is at most 32 * 256 doubles -- the uniform launch's budget at its limit K = 256, and for
// equal K_b and a full block the uniform rule K <= 256 -- and its dynamic LDS is that many doubles;
// otherwise every lane pair reads its times from global memory.
int64_t eval_ragged_clock_slice(const int64_t* seg_off, int64_t B) {
  int64_t m = 0;
  for (int64_t b0 = 0; b0 < B; b0 += kPairTraj) {
    const int64_t b1 = B - b0 < kPairTraj ? B : b0 + kPairTraj;
    m = seg_off[b1] - seg_off[b0] > m ? seg_off[b1] - seg_off[b0] : m;
  }
  return m;
}

bool eval_ragged_clock_staged(int64_t clock_slice) { return clock_slice <= (int64_t)kPairTraj * kClockLdsK; }

hipError_t eval_range_lds_check(int N, int D, int K) {
  return eval_range_lds(N, D, K) > 64 * 1024 ? hipErrorInvalidValue : hipSuccess;
}

namespace {
ClockStage clock_stage(const EvalRagged& r) {
  const bool lds = eval_ragged_clock_staged(r.clock_slice);
  return ClockStage{lds, lds ? (uint32_t)(sizeof(double) * r.clock_slice) : 0u};
}
}  // namespace

hipError_t launch_eval_count_ragged(const EvalRagged& r, int64_t B, const double* times, double t_start, double t_end,
                                    double dt, int64_t* counts, hipStream_t stream) {
  return eval_count_launch<true>(r.seg_off, clock_stage(r), B, times, t_start, t_end, dt, counts, stream);
}

hipError_t launch_eval_runs_counts_ragged(const EvalRagged& r, int64_t B, const double* times, double t_start,
                                          double t_end, double dt, int64_t* counts, int64_t* offsets, void* ws, int cap,
                                          int64_t* total, hipStream_t stream) {
  return eval_runs_counts_launch<true>(r.seg_off, clock_stage(r), B, times, t_start, t_end, dt, counts, offsets, ws,
                                       cap, total, stream);
}

hipError_t launch_eval_range_ragged(int N, int D, const EvalRagged& r, int64_t B, const double* coeffs,
                                    const double* times, double t_start, double t_end, double dt, int derivative,
                                    const int64_t* counts, const int64_t* offsets, double* out, double* sample_times,
                                    void* ws, int cap, hipStream_t stream, bool runs_ready, int64_t* offsets_out,
                                    int64_t capacity, const int64_t* total) {
  return eval_range_launch<true>(N, D, r.K_max, r.seg_off, clock_stage(r), B, coeffs, times, t_start, t_end, dt,
                                 derivative, counts, offsets, out, sample_times, ws, cap, stream, runs_ready,
                                 offsets_out, capacity, total);
}

}  // namespace mtg
