// mtg_vertex_ragged.hip -- the two maps between vertex derivatives and coefficients for a batch whose
// trajectories have different segment counts (mtg_coefficients_from_vertices_ragged_batch,
// mtg_vertex_derivatives_ragged_batch, include/mtg.h).
//
// The CSR arrays are contiguous over the whole batch -- coeffs [sum K][D][N], times [sum K],
// vertex_values [sum K + B][h][D] -- and both maps are per-segment / per-vertex arithmetic with no
// reduction over a trajectory.  So a block of 256 threads owns a fixed tile of TS consecutive *packed
// segments*, whatever trajectory borders fall inside it, and LDS use depends on TS, N and D only: a
// chain of any K goes through.  A segment g of trajectory b has its two vertices at rows g + b and
// g + b + 1; the block finds b by a binary search of seg_off [B + 1] (a device array), stages its
// contiguous input run with coalesced loads (stage_copy), computes one item per thread out of LDS with
// the per-item functions of mtg_vertex_common.h -- the ones the uniform kernels call, hence the same
// bits -- and stores one contiguous output run.
//
// * coefficients: the tile's ns segments need vertex rows (g0 + b_first) .. (g_last + b_last + 1), at
//   most 2 TS (a tile of K = 1 trajectories); the output run is the tile's ns D N coefficients.
// * derivatives: the block writes the start vertex of each of its segments and, where a segment is the
//   last of its trajectory, the trajectory's last vertex: the rows (g0 + b_first) .. (g_last + b_last
//   [+ 1]), contiguous, at most 2 TS, and every row of the batch exactly once.  An interior start
//   vertex needs the end of the segment before it: one halo segment before the tile.
#include "mtg_internal.h"
#include "mtg_vertex_common.h"

namespace mtg {

namespace {

constexpr int kVtxRaggedMaxTile = 32;
constexpr size_t kVtxRaggedMaxLds = 48 * 1024;

__host__ __device__ inline size_t vertex_ragged_lds(int N, int D, int ts) {
  const int H = N / 2;
  return sizeof(double) * ((size_t)(ts + 1) * D * N + (ts + 1) + (size_t)(2 * ts + 1) * H * D) +
         sizeof(int) * (size_t)(2 * ts + 2);
}

// the largest b in [lo, hi] with seg_off[b] + (rows ? b : 0) <= x
__device__ __forceinline__ int64_t last_not_above(const int64_t* __restrict__ seg_off, int64_t lo, int64_t hi,
                                                  int64_t x, bool rows) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo + 1) / 2;
    if (seg_off[mid] + (rows ? mid : 0) <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// vertex values [sum K + B][H][D] -> coefficients [sum K][D][N]
template <int N>
__global__ __launch_bounds__(kVtxThreads) void coefficients_from_vertices_ragged_kernel(
    const double* __restrict__ values, const double* __restrict__ times, const int64_t* __restrict__ seg_off,
    double* __restrict__ coeffs, int64_t B, int64_t S, int D, int TS) {
  constexpr int H = N / 2;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t g0 = (int64_t)blockIdx.x * TS;
  const int ns = (int)(S - g0 < TS ? S - g0 : TS);
  double* xv = lds;                            // [<= 2 TS + 1][H][D]
  double* tl = xv + (2 * TS + 1) * H * D;      // [ns]
  double* co = tl + TS + 1;                    // [ns][D][N]
  int* sb = (int*)(co + (TS + 1) * D * N);     // [ns] the segment's trajectory, relative to the tile's first
  const int tid = threadIdx.x;
  const int64_t b_first = last_not_above(seg_off, 0, B - 1, g0, false);
  const int64_t b_last = last_not_above(seg_off, b_first, B - 1, g0 + ns - 1, false);
  const int64_t vr0 = g0 + b_first;
  const int nrows = (int)(g0 + ns - 1 + b_last + 1 - vr0) + 1;
  if (tid < ns) sb[tid] = (int)(last_not_above(seg_off, b_first, b_last, g0 + tid, false) - b_first);
  stage_copy<8>(values + vr0 * (H * D), xv, nrows * H * D, tid);
  stage_copy<2>(times + g0, tl, ns, tid);
  __syncthreads();
  for (int it = tid; it < ns * D; it += kVtxThreads) {
    const int sl = it / D, d = it - sl * D;
    const int lr = sl + sb[sl];  // (g + b) - vr0
    const double T = tl[sl];
    coefficients_from_ends<N>([&](int e, int k) { return xv[((lr + e) * H + k) * D + d]; }, T, co + (size_t)it * N);
  }
  __syncthreads();
  double* dst = coeffs + g0 * (D * N);
  for (int e = tid; e < ns * D * N; e += kVtxThreads) dst[e] = co[e];
}

// coefficients [sum K][D][N] -> vertex values [sum K + B][H][D]
template <int N>
__global__ __launch_bounds__(kVtxThreads) void vertex_derivatives_ragged_kernel(
    const double* __restrict__ coeffs, const double* __restrict__ times, const int64_t* __restrict__ seg_off,
    double* __restrict__ values, int64_t B, int64_t S, int D, int TS) {
  constexpr int H = N / 2;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t g0 = (int64_t)blockIdx.x * TS;
  const int ns = (int)(S - g0 < TS ? S - g0 : TS);
  const int halo = g0 > 0 ? 1 : 0;             // the segment before the tile
  const int64_t gs0 = g0 - halo;
  double* co = lds;                            // [halo + ns][D][N]
  double* tl = co + (TS + 1) * D * N;          // [halo + ns]
  double* xv = tl + TS + 1;                    // [<= 2 TS + 1][H][D]
  int* ri = (int*)(xv + (2 * TS + 1) * H * D);  // [rows] (local start segment << 2) | at_end << 1 | at_start
  const int tid = threadIdx.x;
  const int64_t g_last = g0 + ns - 1;
  const int64_t b_first = last_not_above(seg_off, 0, B - 1, g0, false);
  const int64_t b_last = last_not_above(seg_off, b_first, B - 1, g_last, false);
  const int64_t vr0 = g0 + b_first;
  const int nrows = (int)(g_last + b_last + (g_last == seg_off[b_last + 1] - 1 ? 1 : 0) - vr0) + 1;
  if (tid < nrows) {
    const int64_t r = vr0 + tid;
    const int64_t b = last_not_above(seg_off, b_first, b_last, r, true);
    const int64_t s0 = seg_off[b], s1 = seg_off[b + 1];
    const int64_t v = r - (s0 + b);            // the vertex within its trajectory, 0 .. K_b
    const int lseg = (int)(s0 + v - gs0);      // its start segment in co (one past the staged run when v == K_b)
    ri[tid] = (lseg << 2) | (v > 0 ? 2 : 0) | (v < s1 - s0 ? 1 : 0);
  }
  stage_copy<8>(coeffs + gs0 * (D * N), co, (halo + ns) * D * N, tid);
  stage_copy<2>(times + gs0, tl, halo + ns, tid);
  __syncthreads();
  // item (vertex row, derivative, dimension) in output order
  for (int it = tid; it < nrows * H * D; it += kVtxThreads) {
    const int lr = it / (H * D), r2 = it - lr * (H * D), k = r2 / D, d = r2 - k * D;
    const int info = ri[lr], lseg = info >> 2;
    xv[it] = vertex_derivative_from_ends<N>(
        (info & 1) != 0, (info & 2) != 0, k, [&](int j) { return co[(lseg * D + d) * N + j]; },
        [&](int j) { return (co + ((lseg - 1) * D + d) * N)[j]; }, [&]() { return tl[lseg - 1]; });
  }
  __syncthreads();
  double* dst = values + vr0 * (H * D);
  for (int e = tid; e < nrows * H * D; e += kVtxThreads) dst[e] = xv[e];
}

template <int N>
hipError_t launch_vertex_ragged_n(bool to_coeffs, const double* in, const double* times, const int64_t* seg_off,
                                  double* out, int64_t B, int64_t S, int D, hipStream_t stream) {
  const int ts = vertex_ragged_tile(N, D);
  if (ts < 1) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  const int64_t blocks = (S + ts - 1) / ts;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  const size_t lds = vertex_ragged_lds(N, D, ts);
  const dim3 grid((unsigned)blocks), block(kVtxThreads);
  if (to_coeffs)
    launch_kernel((coefficients_from_vertices_ragged_kernel<N>), grid, block, (uint32_t)lds, stream, in, times, seg_off,
                  out, B, S, D, ts);
  else
    launch_kernel((vertex_derivatives_ragged_kernel<N>), grid, block, (uint32_t)lds, stream, in, times, seg_off, out, B,
                  S, D, ts);
  return hipGetLastError();
}

}  // namespace

int vertex_ragged_tile(int N, int D) {
  int ts = kVtxRaggedMaxTile;
  while (ts > 0 && vertex_ragged_lds(N, D, ts) > kVtxRaggedMaxLds) --ts;
  return ts;
}

hipError_t launch_vertex_map_ragged(bool to_coeffs, int N, const double* in, const double* times,
                                    const int64_t* seg_off, double* out, int64_t B, int64_t S, int D,
                                    hipStream_t stream) {
  switch (N) {
    case 2: return launch_vertex_ragged_n<2>(to_coeffs, in, times, seg_off, out, B, S, D, stream);
    case 4: return launch_vertex_ragged_n<4>(to_coeffs, in, times, seg_off, out, B, S, D, stream);
    case 6: return launch_vertex_ragged_n<6>(to_coeffs, in, times, seg_off, out, B, S, D, stream);
    case 8: return launch_vertex_ragged_n<8>(to_coeffs, in, times, seg_off, out, B, S, D, stream);
    case 10: return launch_vertex_ragged_n<10>(to_coeffs, in, times, seg_off, out, B, S, D, stream);
    case 12: return launch_vertex_ragged_n<12>(to_coeffs, in, times, seg_off, out, B, S, D, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mtg
