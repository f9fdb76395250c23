// mtg_evaluate_at.inc -- the two kernels of batched Trajectory::evaluate (src/trajectory.cpp:41-66) at
// caller-given query times, several derivative orders per pass over the coefficients
// (Polynomial::evaluate, polynomial.h:120-151), and their launcher.  Included by mtg_evaluate_at.hip
// (uniform K: mtg_evaluate_at_batch, DESIGN.md 3.13) and by mtg_evaluate_at_ragged.hip (CSR batches:
// mtg_evaluate_at_ragged_batch, DESIGN.md 3.15); each unit instantiates one value of the Ragged flag.
//
// Two mappings, picked by evaluate_at_plan from the shape alone (never from the batch or the data):
//   staged  a block per (trajectory, chunk of queries): the trajectory's K D N coefficients, its K + 1
//           prefix sums and its K times are staged in LDS once (lane 0 runs the serial prefix while
//           the other lanes copy), then one query per lane: a binary search of the LDS prefix and
//           n_derivatives D Horner chains.
//   lane    a lane per (trajectory, query): the lane walks its trajectory's times in global memory
//           (the reference's linear scan) and reads only its segment's D N contiguous coefficients.
// Both call eval_row with the same operands, so a query's bits do not depend on the mapping.  Both
// stage a block's rows in LDS and write them as one contiguous run of the output (store_run).
//
// Ragged: trajectory b's segments start at seg_off[b] in coeffs and times and it has
// K_b = seg_off[b + 1] - seg_off[b] of them, where the uniform kernels have b K and K.  Nothing else
// differs -- the same eval_row operands, the same rows, the same stores (out, in_range and status do
// not depend on K) -- so a trajectory's bytes are those of the uniform call with K = K_b.
#include <float.h>

#include <type_traits>

#include "mtg_internal.h"

namespace mtg {

namespace {

constexpr size_t kAtMaxLds = 64 * 1024;
constexpr int kAtMaxThreads = 256;
constexpr int kAtPasses = 4;                 // staged: queries per block = threads x kAtPasses
constexpr int64_t kAtMaxBlocks = 1 << 22;    // blocks per launch (grid x block stays below 2^32)

typedef double dvec2 __attribute__((ext_vector_type(2)));

// Polynomial::base_coefficients_(k, j) = j!/(j-k)! (src/polynomial.cpp:140-155), 0 for j < k; exact
// in a double (at most 11!).  Row k is read with a wave-uniform k: scalar loads.
struct BaseTable {
  double v[12][12];
};
constexpr BaseTable make_base_table() {
  BaseTable t{};
  for (int k = 0; k < 12; ++k)
    for (int j = 0; j < 12; ++j) {
      double b = j < k ? 0.0 : 1.0;
      for (int i = j - k + 1; j >= k && i <= j; ++i) b *= (double)i;
      t.v[k][j] = b;
    }
  return t;
}
__constant__ BaseTable c_at_base = make_base_table();

struct EvalAtArgs {
  const double* coeffs;   // [B][K][D][N]
  const double* times;    // [B][K]
  const double* t_query;  // [B][t_stride] (t_stride 0: [M], shared)
  double* out;            // [B][M][nd][D]
  uint8_t* in_range;      // [B][M] (nullable)
  int32_t* status;        // [B] (nullable)
  int64_t B, M, t_stride;
  int64_t chunks;         // staged: blocks per trajectory
  int D, K, k0, nd;
};
// ragged: coeffs [sum K][D][N], times [sum K]; K is the largest K_b (it sized the staged block's LDS)
struct EvalAtRaggedArgs : EvalAtArgs {
  const int64_t* seg_off;  // [B + 1]
};
template <bool Ragged>
using AtArgs = std::conditional_t<Ragged, EvalAtRaggedArgs, EvalAtArgs>;

__device__ __forceinline__ bool bad_time(double T) { return !(T > 0.0 && T <= DBL_MAX); }

// One row [nd][D]: order k0 + q of every dimension at local time tl, from the segment's coefficients
// c [D][N].  Multiply, then add, each rounded (polynomial.h:138-151): no FMA.
template <int N>
__device__ __forceinline__ void eval_row(const double* c, double tl, int D, int k0, int nd, double* row) {
#pragma clang fp contract(off)
  for (int d = 0; d < D; ++d) {
    double cc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) cc[j] = c[d * N + j];
    for (int q = 0; q < nd; ++q) {
      const int k = k0 + q;
      double r = 0.0;
      if (k < N) {
        const double* bs = c_at_base.v[k];
        r = bs[N - 1] * cc[N - 1];
#pragma unroll
        for (int j = N - 2; j >= 0; --j) {
          if (j >= k) {
            r = r * tl;
            r = r + bs[j] * cc[j];
          }
        }
      }
      row[q * D + d] = r;
    }
  }
}

__device__ __forceinline__ void fill_row(double* row, int W, double v) {
  for (int i = 0; i < W; ++i) row[i] = v;
}

// n doubles of LDS to a contiguous run of global memory: 16-B pieces from the first 16-B aligned
// address, an 8-B head and tail where the run does not start or end on one.  Plain stores.
__device__ __forceinline__ void store_run(double* dst, const double* ob, int n, int tid, int T) {
  int head = (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1);
  head = head < n ? head : n;
  if (tid == 0 && head) dst[0] = ob[0];
  const int n2 = (n - head) >> 1;
  dvec2* d2 = reinterpret_cast<dvec2*>(dst + head);
  for (int i = tid; i < n2; i += T) d2[i] = dvec2{ob[head + 2 * i], ob[head + 2 * i + 1]};
  if (tid == 0 && ((n - head) & 1)) dst[n - 1] = ob[n - 1];
}

template <int N, bool Ragged>
__global__ __launch_bounds__(kAtMaxThreads) void evaluate_at_staged_kernel(AtArgs<Ragged> a, int64_t block0) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double at_lds[];
  __shared__ int s_bad;
  const int T = blockDim.x, tid = threadIdx.x;
  const int D = a.D, W = a.nd * a.D;
  const int64_t blk = block0 + blockIdx.x;
  const int64_t b = blk / a.chunks, ch = blk - b * a.chunks;
  // ragged: the trajectory's first segment in coeffs and times, and its own segment count
  [[maybe_unused]] int64_t s0 = 0;
  int K;
  if constexpr (Ragged) {
    s0 = a.seg_off[b];
    K = (int)(a.seg_off[b + 1] - s0);
  } else {
    K = a.K;
  }
  double* ob = at_lds;        // [T][W] (first: 16-B aligned)
  double* cf = ob + T * W;    // [K][D][N]
  double* pre = cf + K * D * N;  // [K + 1]
  double* tm = pre + K + 1;      // [K]
  const double* cb;
  if constexpr (Ragged) cb = a.coeffs + s0 * D * N;
  else cb = a.coeffs + b * (int64_t)K * D * N;
  if (tid == 0) {
    const double* tb;
    if constexpr (Ragged) tb = a.times + s0;
    else tb = a.times + b * K;
    double acc = 0.0;
    bool bad = false;
    pre[0] = 0.0;
    for (int i = 0; i < K; ++i) {
      const double Ti = tb[i];
      bad = bad || bad_time(Ti);
      acc = acc + Ti;
      pre[i + 1] = acc;
      tm[i] = Ti;
    }
    s_bad = bad;
    if (ch == 0 && a.status) a.status[b] = bad ? MTG_TRAJ_BAD_TIME : MTG_TRAJ_OK;
  } else {
    for (int i = tid - 1; i < K * D * N; i += T - 1) cf[i] = cb[i];
  }
  __syncthreads();
  const bool bad = s_bad != 0;
  const double* tq = a.t_query + b * a.t_stride;
  for (int p = 0; p < kAtPasses; ++p) {
    const int64_t m0 = (ch * kAtPasses + p) * T;
    if (m0 >= a.M) break;
    const int cnt = (int)(a.M - m0 < T ? a.M - m0 : T);
    if (tid < cnt) {
      const double t = tq[m0 + tid];
      // first i with pre[i + 1] > t (the prefix is non-decreasing for valid times); K: none
      int lo = 0, hi = K;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (pre[mid + 1] > t) hi = mid;
        else lo = mid + 1;
      }
      bool beyond = false;
      if (lo == K) {
        beyond = t > pre[K];
        lo = K - 1;  // t equal to the total (or NaN): the last segment
      }
      double* row = ob + tid * W;
      const bool nan = bad || t != t;
      if (nan) fill_row(row, W, __builtin_nan(""));
      else if (beyond) fill_row(row, W, 0.0);
      else eval_row<N>(cf + lo * D * N, t - (pre[lo + 1] - tm[lo]), D, a.k0, a.nd, row);
      if (a.in_range) a.in_range[b * a.M + m0 + tid] = !(nan || beyond);
    }
    __syncthreads();
    store_run(a.out + (b * a.M + m0) * W, ob, cnt * W, tid, T);
    __syncthreads();
  }
}

template <int N, bool Ragged>
__global__ __launch_bounds__(kAtMaxThreads) void evaluate_at_lane_kernel(AtArgs<Ragged> a, int64_t block0) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double at_lds[];
  const int T = blockDim.x, tid = threadIdx.x;
  const int D = a.D, W = a.nd * a.D;
  const int64_t q0 = (block0 + blockIdx.x) * T, total = a.B * a.M;
  const int cnt = (int)(total - q0 < T ? total - q0 : T);  // (the grid's tail)
  double* ob = at_lds;  // [T][W]
  if (tid < cnt) {
    const int64_t q = q0 + tid, b = q / a.M, m = q - b * a.M;
    const double t = a.t_query[b * a.t_stride + m];
    int K;
    int64_t s0;  // the trajectory's first segment in coeffs and times
    if constexpr (Ragged) {
      s0 = a.seg_off[b];
      K = (int)(a.seg_off[b + 1] - s0);
    } else {
      K = a.K;
      s0 = b * K;
    }
    const double* tb = a.times + s0;
    // trajectory.cpp:42-57: the first i whose accumulated end time exceeds t; the walk goes on to
    // the end for the bad-time check
    double acc = 0.0, acc_i = 0.0, T_i = 0.0;
    int seg = -1;
    bool bad = false;
    for (int i = 0; i < K; ++i) {
      const double Ti = tb[i];
      bad = bad || bad_time(Ti);
      acc = acc + Ti;
      if (seg < 0 && acc > t) {
        seg = i;
        acc_i = acc;
        T_i = Ti;
      }
    }
    bool beyond = false;
    if (seg < 0) {
      beyond = t > acc;
      seg = K - 1;
      acc_i = acc;
      T_i = tb[K - 1];
    }
    double* row = ob + tid * W;
    const bool nan = bad || t != t;
    if (nan) fill_row(row, W, __builtin_nan(""));
    else if (beyond) fill_row(row, W, 0.0);
    else eval_row<N>(a.coeffs + (s0 + seg) * (int64_t)D * N, t - (acc_i - T_i), D, a.k0, a.nd, row);
    if (a.in_range) a.in_range[q] = !(nan || beyond);
    if (m == 0 && a.status) a.status[b] = bad ? MTG_TRAJ_BAD_TIME : MTG_TRAJ_OK;
  }
  __syncthreads();
  store_run(a.out + q0 * W, ob, cnt * W, tid, T);
}

template <int N, bool Ragged>
hipError_t launch_at_n(const EvalAtPlan& p, const AtArgs<Ragged>& a, hipStream_t stream) {
  const int64_t blocks =
      p.path == MTG_EVALUATE_AT_STAGED ? a.B * a.chunks : (a.B * a.M + p.threads - 1) / p.threads;
  for (int64_t b0 = 0; b0 < blocks; b0 += kAtMaxBlocks) {
    const dim3 grid((unsigned)(blocks - b0 < kAtMaxBlocks ? blocks - b0 : kAtMaxBlocks)), block(p.threads);
    if (p.path == MTG_EVALUATE_AT_STAGED)
      launch_kernel(evaluate_at_staged_kernel<N, Ragged>, grid, block, (uint32_t)p.lds, stream, a, b0);
    else
      launch_kernel(evaluate_at_lane_kernel<N, Ragged>, grid, block, (uint32_t)p.lds, stream, a, b0);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// the plan for (K, M) -- K is the largest K_b of a ragged batch -- and the launch for this N
template <bool Ragged>
hipError_t launch_at(int N, int D, int K, int64_t B, const double* coeffs, const double* times, const double* t_query,
                     int64_t t_stride, int64_t M, int derivative_begin, int n_derivatives, double* out,
                     uint8_t* in_range, int32_t* status, AtArgs<Ragged> a, hipStream_t stream) {
  if (B == 0 || M == 0) return hipSuccess;
  EvalAtPlan p;
  if (!evaluate_at_plan(N, D, K, M, n_derivatives, &p)) return hipErrorInvalidValue;
  a.coeffs = coeffs;
  a.times = times;
  a.t_query = t_query;
  a.out = out;
  a.in_range = in_range;
  a.status = status;
  a.B = B;
  a.M = M;
  a.t_stride = t_stride;
  const int64_t chunk = (int64_t)p.threads * kAtPasses;
  a.chunks = (M + chunk - 1) / chunk;
  a.D = D;
  a.K = K;
  a.k0 = derivative_begin;
  a.nd = n_derivatives;
  switch (N) {
    case 2: return launch_at_n<2, Ragged>(p, a, stream);
    case 4: return launch_at_n<4, Ragged>(p, a, stream);
    case 6: return launch_at_n<6, Ragged>(p, a, stream);
    case 8: return launch_at_n<8, Ragged>(p, a, stream);
    case 10: return launch_at_n<10, Ragged>(p, a, stream);
    case 12: return launch_at_n<12, Ragged>(p, a, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

}  // namespace mtg
