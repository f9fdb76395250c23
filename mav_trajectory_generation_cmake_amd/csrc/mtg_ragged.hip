// mtg_ragged.hip -- the copy kernels of the ragged entries: the two of the ragged solve
// (mtg_solve_linear_ragged_batch) and the two of the ragged min / max magnitude
// (mtg_min_max_magnitude_ragged_batch).  A ragged batch keeps trajectories of different segment counts K in CSR arrays;
// the groups whose members are not consecutive are gathered into packed uniform arrays, solved by the
// existing kernels, and scattered back:
//
// * ragged_gather_kernel: values, fixed_mask and times of every gathered trajectory, from the caller's
//   CSR arrays into the packed arrays;
// * ragged_scatter_kernel: coeffs, free_out, n_free_out, cost_out and status (those requested) of
//   every gathered trajectory, from the packed arrays to their CSR positions;
// * ragged_gather_coeffs_kernel: coeffs and times of every gathered trajectory into packed arrays, for
//   the entries that consume solved coefficients;
// * ragged_scatter_extrema_kernel: the gathered trajectories' minimum and maximum to minimum[b] and
//   maximum[b] (a lane per trajectory: one 24-byte struct each).
//
// One launch each for all gathered groups, driven by one record per gathered trajectory (RaggedRec).
// A wave owns a trajectory and its lanes stride over the trajectory's doubles, so a wave instruction
// reads and writes one contiguous run (config 2: 165 value and 10 time doubles in, 300 coefficient
// doubles out).  A run moves as 16-byte pieces where source and destination are both 16-byte aligned
// (the CSR offsets only guarantee 8), as doubles otherwise; a piece's loads are all issued before its
// stores.  Plain vector loads and stores; nothing here computes.
#include <hip/hip_runtime.h>

#include "mtg_internal.h"

namespace mtg {

namespace {

constexpr int kRaggedThreads = 256;  // four waves, one trajectory each
constexpr int kWave = 64;

typedef double rg_dvec2 __attribute__((ext_vector_type(2)));

// dst[i] = src[i], i < n, by one wave; U pieces per lane in flight
template <int U>
__device__ __forceinline__ void wave_copy(const double* __restrict__ src, double* __restrict__ dst, int n, int lane) {
  const bool al16 = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
  if (al16) {
    const rg_dvec2* s2 = reinterpret_cast<const rg_dvec2*>(src);
    rg_dvec2* d2 = reinterpret_cast<rg_dvec2*>(dst);
    const int n2 = n >> 1;
    for (int base = 0; base < n2; base += U * kWave) {
      rg_dvec2 r[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = base + u * kWave + lane;
        if (i < n2) r[u] = s2[i];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = base + u * kWave + lane;
        if (i < n2) d2[i] = r[u];
      }
    }
    if ((n & 1) && lane == 0) dst[n - 1] = src[n - 1];
  } else {
    for (int base = 0; base < n; base += U * kWave) {
      double r[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = base + u * kWave + lane;
        if (i < n) r[u] = src[i];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = base + u * kWave + lane;
        if (i < n) dst[i] = r[u];
      }
    }
  }
}

__global__ __launch_bounds__(kRaggedThreads) void ragged_gather_kernel(RaggedCopyArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t j = (int64_t)blockIdx.x * (kRaggedThreads / kWave) + (threadIdx.x >> 6);
  if (j >= a.n) return;
  const RaggedRec rec = a.recs[j];
  const int K = rec.K, V = K + 1;
  const int64_t src_s = rec.src_v - rec.b, dst_s = rec.dst_v - j;  // so = vo - index
  // the two small arrays first: their loads are in flight while the values are requested
  const uint8_t* ms = a.mask + rec.src_v;
  uint8_t* md = a.p_mask + rec.dst_v;
  for (int i = lane; i < V; i += kWave) md[i] = ms[i];
  wave_copy<1>(a.times + src_s, a.p_times + dst_s, K, lane);
  wave_copy<2>(a.values + rec.src_v * a.hD, a.p_values + rec.dst_v * a.hD, V * a.hD, lane);
}

__global__ __launch_bounds__(kRaggedThreads) void ragged_scatter_kernel(RaggedCopyArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t j = (int64_t)blockIdx.x * (kRaggedThreads / kWave) + (threadIdx.x >> 6);
  if (j >= a.n) return;
  const RaggedRec rec = a.recs[j];
  const int K = rec.K, V = K + 1;
  const int64_t src_s = rec.src_v - rec.b, dst_s = rec.dst_v - j;
  if (lane == 0) {
    if (a.n_free) a.n_free[rec.b] = a.p_n_free[j];
    if (a.cost) a.cost[rec.b] = a.p_cost[j];
    if (a.status) a.status[rec.b] = a.p_status[j];
  }
  if (a.free) wave_copy<2>(a.p_free + rec.dst_v * a.hD, a.free + rec.src_v * a.hD, V * a.hD, lane);
  if (a.coeffs) wave_copy<4>(a.p_coeffs + dst_s * a.DN, a.coeffs + src_s * a.DN, K * a.DN, lane);
}

__global__ __launch_bounds__(kRaggedThreads) void ragged_gather_coeffs_kernel(RaggedCoeffArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t j = (int64_t)blockIdx.x * (kRaggedThreads / kWave) + (threadIdx.x >> 6);
  if (j >= a.n) return;
  const RaggedRec rec = a.recs[j];
  const int K = rec.K;
  const int64_t src_s = rec.src_v - rec.b, dst_s = rec.dst_v - j;
  wave_copy<1>(a.times + src_s, a.p_times + dst_s, K, lane);
  wave_copy<4>(a.coeffs + src_s * a.DN, a.p_coeffs + dst_s * a.DN, K * a.DN, lane);
}

__global__ __launch_bounds__(kRaggedThreads) void ragged_scatter_extrema_kernel(RaggedCoeffArgs a) {
  const int64_t j = (int64_t)blockIdx.x * kRaggedThreads + threadIdx.x;
  if (j >= a.n) return;
  const int64_t b = a.recs[j].b;
  if (a.minimum) a.minimum[b] = a.p_minimum[j];
  if (a.maximum) a.maximum[b] = a.p_maximum[j];
}

template <class Args>
hipError_t launch_copy(void (*kernel)(Args), const Args& a, hipStream_t stream, int per = kRaggedThreads / kWave) {
  if (a.n <= 0) return hipSuccess;
  const int64_t blocks = (a.n + per - 1) / per;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  launch_kernel(kernel, dim3((unsigned)blocks), dim3(kRaggedThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_ragged_gather(const RaggedCopyArgs& a, hipStream_t stream) {
  return launch_copy(ragged_gather_kernel, a, stream);
}

hipError_t launch_ragged_scatter(const RaggedCopyArgs& a, hipStream_t stream) {
  return launch_copy(ragged_scatter_kernel, a, stream);
}

hipError_t launch_ragged_gather_coeffs(const RaggedCoeffArgs& a, hipStream_t stream) {
  return launch_copy(ragged_gather_coeffs_kernel, a, stream);
}

hipError_t launch_ragged_scatter_extrema(const RaggedCoeffArgs& a, hipStream_t stream) {
  return launch_copy(ragged_scatter_extrema_kernel, a, stream, kRaggedThreads);
}

}  // namespace mtg
