// mtg_vertex.hip -- the two maps between a trajectory's vertex derivatives and its coefficients,
// batched:
//
// * coefficients_from_vertices: c_i = A(T_i)^-1 [x_i; x_{i+1}] per (segment, dimension), the
//   reference's updateSegmentsFromCompactConstraints (lin_impl:253-273) after
//   setFreeConstraints (polynomial_optimization_linear.h:185-186) -- every vertex derivative
//   (fixed and free) is given, nothing is solved.  Same arithmetic as the solve kernels'
//   epilogue: A(T)^-1 = diag(T^-j) A(1)^-1 S(T) from the exact-rational A(1)^-1 table, with the
//   segment's start position subtracted first (only c_0 changes; no cancellation of p_i
//   against p_{i+1} in c_j, j >= h).  The per-(segment, dimension) part is mtg_vertex_common.h,
//   shared with mtg_soft_constraint.hip.
// * vertex_derivatives: the reference's M^+ A p (nl_impl:162-180, used by
//   computeInitialSolutionWithoutPositionConstraints): the end derivatives A_i c_i of every
//   segment, mapped to the (vertex, derivative) unknowns by the pseudo-inverse of the 0/1
//   reordering matrix M (lin_impl:172-250), i.e. the mean of the two segment ends that meet at an
//   interior vertex and the single end at the first / last vertex.  The per-(vertex, derivative,
//   dimension) part is mtg_vertex_common.h too, shared with mtg_vertex_ragged.hip.
//
// Both are HBM-bound streams.  A block of 256 threads owns TB consecutive trajectories: it
// stages their input (contiguous in HBM) into LDS with coalesced loads, computes one item per
// thread out of LDS, writes the results into LDS and stores them as one contiguous run.
#include "mtg_vertex_common.h"

namespace mtg {

namespace {

// vertex values [TB][V][H][D] -> coefficients [TB][K][D][N]
template <int N>
__global__ __launch_bounds__(kVtxThreads) void coefficients_from_vertices_kernel(const double* __restrict__ values,
                                                                                 const double* __restrict__ times,
                                                                                 double* __restrict__ coeffs,
                                                                                 int64_t B, int K, int D, int TB) {
  constexpr int H = N / 2;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int V = K + 1, xsz = V * H * D, csz = K * D * N;
  const int64_t b0 = (int64_t)blockIdx.x * TB;
  const int nb = (int)(B - b0 < TB ? B - b0 : TB);
  double* xv = lds;                // [nb][V][H][D]
  double* tl = xv + TB * xsz;      // [nb][K]
  double* co = tl + TB * K;        // [nb][K][D][N] (TB * K even: 16-B aligned when TB even)
  const int tid = threadIdx.x;
  stage_copy<8>(values + b0 * xsz, xv, nb * xsz, tid);
  stage_copy<2>(times + b0 * K, tl, nb * K, tid);
  __syncthreads();
  for (int it = tid; it < nb * K * D; it += kVtxThreads) {
    const int bl = it / (K * D), rem = it - bl * (K * D), i = rem / D, d = rem - i * D;
    const double T = tl[bl * K + i];
    const double* x = xv + bl * xsz;
    coefficients_from_ends<N>([&](int e, int k) { return x[((i + e) * H + k) * D + d]; }, T, co + (size_t)it * N);
  }
  __syncthreads();
  double* dst = coeffs + b0 * csz;
  for (int e = tid; e < nb * csz; e += kVtxThreads) dst[e] = co[e];
}

// coefficients [TB][K][D][N] -> vertex values [TB][V][H][D]
template <int N>
__global__ __launch_bounds__(kVtxThreads) void vertex_derivatives_kernel(const double* __restrict__ coeffs,
                                                                         const double* __restrict__ times,
                                                                         double* __restrict__ values, int64_t B,
                                                                         int K, int D, int TB) {
  constexpr int H = N / 2;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int V = K + 1, xsz = V * H * D, csz = K * D * N;
  const int64_t b0 = (int64_t)blockIdx.x * TB;
  const int nb = (int)(B - b0 < TB ? B - b0 : TB);
  double* co = lds;                // [nb][K][D][N]
  double* tl = co + TB * csz;      // [nb][K]
  double* xv = tl + TB * K;        // [nb][V][H][D]
  const int tid = threadIdx.x;
  stage_copy<8>(coeffs + b0 * csz, co, nb * csz, tid);
  stage_copy<2>(times + b0 * K, tl, nb * K, tid);
  __syncthreads();
  // item (trajectory, vertex, derivative, dimension) in output order
  for (int it = tid; it < nb * xsz; it += kVtxThreads) {
    const int bl = it / xsz, rem = it - bl * xsz;
    const int v = rem / (H * D), r2 = rem - v * (H * D), k = r2 / D, d = r2 - k * D;
    xv[it] = vertex_derivative_from_ends<N>(
        v < K, v > 0, k, [&](int j) { return co[((bl * K + v) * D + d) * N + j]; },
        [&](int j) { return (co + ((bl * K + v - 1) * D + d) * N)[j]; }, [&]() { return tl[bl * K + v - 1]; });
  }
  __syncthreads();
  double* dst = values + b0 * xsz;
  for (int e = tid; e < nb * xsz; e += kVtxThreads) dst[e] = xv[e];
}

int traj_per_block(int N, int D, int K) {
  const int H = N / 2, V = K + 1;
  const size_t per = sizeof(double) * ((size_t)V * H * D + K + (size_t)K * D * N);
  int tb = (int)(48 * 1024 / per);
  if (tb > 16) tb = 16;
  return tb & ~1;  // even: the LDS regions stay 16-B aligned
}

template <int N>
hipError_t launch_vertex_n(bool to_coeffs, const double* in, const double* times, double* out, int64_t B, int K,
                           int D, hipStream_t stream) {
  const int tb = traj_per_block(N, D, K);
  if (tb < 2) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  const int H = N / 2, V = K + 1;
  const size_t lds = sizeof(double) * (size_t)tb * ((size_t)V * H * D + K + (size_t)K * D * N);
  const dim3 grid((unsigned)((B + tb - 1) / tb)), block(kVtxThreads);
  if (to_coeffs)
    launch_kernel((coefficients_from_vertices_kernel<N>), grid, block, lds, stream, in, times, out, B, K, D, tb);
  else
    launch_kernel((vertex_derivatives_kernel<N>), grid, block, lds, stream, in, times, out, B, K, D, tb);
  return hipGetLastError();
}

}  // namespace

bool vertex_map_fits(int N, int D, int K) { return traj_per_block(N, D, K) >= 2; }

hipError_t launch_vertex_map(bool to_coeffs, int N, const double* in, const double* times, double* out, int64_t B,
                             int K, int D, hipStream_t stream) {
  switch (N) {
    case 2: return launch_vertex_n<2>(to_coeffs, in, times, out, B, K, D, stream);
    case 4: return launch_vertex_n<4>(to_coeffs, in, times, out, B, K, D, stream);
    case 6: return launch_vertex_n<6>(to_coeffs, in, times, out, B, K, D, stream);
    case 8: return launch_vertex_n<8>(to_coeffs, in, times, out, B, K, D, stream);
    case 10: return launch_vertex_n<10>(to_coeffs, in, times, out, B, K, D, stream);
    case 12: return launch_vertex_n<12>(to_coeffs, in, times, out, B, K, D, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mtg
