// mtg_collision_ragged.hip -- collision cost, gradient and flag for a batch whose trajectories have
// different segment counts (mtg_collision_cost_ragged_batch, include/mtg.h).  The
// kernel is that of mtg_collision.inc with the CSR indirection: one wave per trajectory, which reads
// its vertices, mask and times where they lie.  A unit of its own, so that mtg_collision.hip holds
// the uniform kernels and nothing else.
#include "mtg_collision.inc"

namespace mtg {

// K_max: the largest segment count of the batch (it sizes the launch's LDS: collision_lds_bytes(N,
// K_max)); seg_off [B + 1] on the device.  One launch of B one-wave blocks.
hipError_t launch_collision_cost_ragged(int N, int K_max, int64_t B, const int64_t* seg_off, const double* values,
                                        const uint8_t* mask, const double* times, const mtg_sdf_grid& grid,
                                        const float* distance, const mtg_collision_params& p, double* cost,
                                        double* grad, uint8_t* collision, int32_t* n_evaluated, int32_t* status,
                                        hipStream_t stream) {
  CollisionRaggedArgs a;
  collision_fill_args<true>(a, values, mask, times, grid, distance, p, cost, grad, collision, n_evaluated, status, B,
                            K_max);
  a.seg_off = seg_off;
  return launch_collision<true>(N, a, grad != nullptr, stream);
}

}  // namespace mtg
