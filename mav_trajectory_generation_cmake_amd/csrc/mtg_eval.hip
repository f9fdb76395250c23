// mtg_eval.hip -- batched Trajectory::evaluateRange (src/trajectory.cpp:68-128) for a batch of one
// segment count K (mtg_evaluate_range_batch, mtg_evaluate_range_batch_full).  The kernels and their
// launchers are mtg_eval.inc, instantiated here for uniform K (the CSR form is mtg_eval_ragged.hip);
// this file keeps what does not depend on K: the scan of the block totals and the workspace sizes.
#include "mtg_eval.inc"

namespace mtg {

// Second level of the offsets: one block scans the per-block totals in place (exclusive) and writes
// the grand total.  nb = ceil(B / kPairTraj) entries (one per 32-trajectory block of the clock
// kernel); each thread takes a contiguous chunk.
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void eval_scan_kernel(int64_t nb, int64_t* bsum, int64_t* total) {
  __shared__ int64_t part[kScanThreads];
  const int t = threadIdx.x;
  const int64_t per = (nb + kScanThreads - 1) / kScanThreads;
  const int64_t i0 = (int64_t)t * per < nb ? (int64_t)t * per : nb, i1 = i0 + per < nb ? i0 + per : nb;
  int64_t s = 0;
  for (int64_t i = i0; i < i1; ++i) s += bsum[i];
  part[t] = s;
  __syncthreads();
  for (int m = 1; m < kScanThreads; m <<= 1) {  // inclusive scan of the chunk sums
    const int64_t o = t >= m ? part[t - m] : 0;
    __syncthreads();
    part[t] += o;
    __syncthreads();
  }
  int64_t run = part[t] - s;  // exclusive prefix of this chunk
  for (int64_t i = i0; i < i1; ++i) {
    const int64_t v = bsum[i];
    bsum[i] = run;
    run += v;
  }
  if (t == kScanThreads - 1) *total = part[t];
}

void launch_eval_scan(int64_t nb, int64_t* bsum, int64_t* total, hipStream_t stream) {
  hipLaunchKernelGGL(eval_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, nb, bsum, total);
}

hipError_t launch_eval_count(int N, int D, int K, int64_t B, const double* times, double t_start,
                             double t_end, double dt, int64_t* counts, hipStream_t stream) {
  (void)N;
  (void)D;
  return eval_count_launch<false>(K, clock_stage_uniform(K), B, times, t_start, t_end, dt, counts, stream);
}

size_t eval_workspace_bytes(int K, int64_t B, int* cap) {
  // up to 256 runs per trajectory (config 2 has ~100-130: at 128 some trajectories overflowed to
  // the slow path, 0.793 -> 0.785 ms at 1e4), fewer for huge batches: the table is only written as
  // far as each trajectory's runs go and is capped at 2 GB; a trajectory with more runs than the
  // table holds continues on its eval wave's lane 0
  (void)K;
  int c = 256;
  while (c > 8 && (double)B * (c * sizeof(RunRec) + sizeof(RunHead)) > 2.0e9) c /= 2;
  *cap = c;
  return (size_t)B * (sizeof(RunHead) + (size_t)c * sizeof(RunRec));
}

size_t eval_full_workspace_bytes(int K, int64_t B, int* cap) {
  // the run table, then the per-block totals and the grand total
  return eval_workspace_bytes(K, B, cap) + sizeof(int64_t) * (size_t)((B + kPairTraj - 1) / kPairTraj + 1);
}

hipError_t launch_eval_runs_counts(int K, int64_t B, const double* times, double t_start, double t_end, double dt,
                                   int64_t* counts, int64_t* offsets, void* ws, int cap, int64_t* total,
                                   hipStream_t stream) {
  return eval_runs_counts_launch<false>(K, clock_stage_uniform(K), B, times, t_start, t_end, dt, counts, offsets, ws,
                                        cap, total, stream);
}

hipError_t launch_eval_range(int N, int D, int K, int64_t B, const double* coeffs, const double* times,
                             double t_start, double t_end, double dt, int derivative, const int64_t* counts,
                             const int64_t* offsets, double* out, double* sample_times, void* ws, int cap,
                             hipStream_t stream, bool runs_ready, int64_t* offsets_out, int64_t capacity,
                             const int64_t* total) {
  return eval_range_launch<false>(N, D, K, K, clock_stage_uniform(K), B, coeffs, times, t_start, t_end, dt, derivative,
                                  counts, offsets, out, sample_times, ws, cap, stream, runs_ready, offsets_out,
                                  capacity, total);
}

}  // namespace mtg
