// mtg_collision.hip -- batched collision cost and gradient over a signed distance field
// (mtg_collision_cost_batch): the uniform-K instantiations of mtg_collision.inc -- the two kernels of
// mtg_collision_cost_batch and the stale-L_ one of mtg_objective_time_batch -- and nothing else
// (the CSR form is mtg_collision_ragged.hip).
#include "mtg_collision.inc"

namespace mtg {

size_t collision_lds_bytes(int N, int K) { return sizeof(double) * collision_lds_doubles(N, K); }

hipError_t launch_collision_cost(int N, const double* values, const uint8_t* mask, const double* times,
                                 const mtg_sdf_grid& grid, const float* distance, const mtg_collision_params& p,
                                 double* cost, double* grad, uint8_t* collision, int32_t* n_evaluated, int32_t* status,
                                 int64_t B, int K, hipStream_t stream, const double* coeff_times) {
  CollisionArgs a;
  collision_fill_args<false>(a, values, mask, times, grid, distance, p, cost, grad, collision, n_evaluated, status, B, K);
  a.coeff_times = coeff_times;
  return launch_collision<false>(N, a, grad != nullptr, stream);
}

}  // namespace mtg
