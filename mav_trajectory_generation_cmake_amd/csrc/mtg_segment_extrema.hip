// mtg_segment_extrema.hip -- per-segment extrema on a time window, with the candidate list:
// mtg_segment_min_max_magnitude_batch (Segment::computeMinMaxMagnitudeCandidates +
// selectMinMaxMagnitudeFromCandidates, src/segment.cpp:82-196) and mtg_segment_min_max_axis_batch
// (Polynomial::computeMinMax per (segment, dimension), src/polynomial.cpp:57-138).
//
// A grid over work items, not over trajectories: an item is a segment (magnitude entry) or a
// (segment, dimension) pair (axis entry), and a group of 8 consecutive lanes of one wave owns it.  A
// wave holds 8 items, a block 32; there is no reduction across groups and no __syncthreads, so a
// uniform batch [B K] and a CSR-packed ragged batch [sum K_b] are the same launch.  The per-segment
// search is mtg_extrema_common.h with L = 8 -- the staging of q, q1, the forming of f, the scan, the
// refinement and the group reduction are the text mtg_extrema.hip runs at K <= 64, so on [0, T] the
// per-segment extremes here are the bits that kernel reduces over a trajectory.  The axis entry is the
// header's one-dimension path (f = p_d^(k+1)) with the signed Horner value as the quantity.
//
// The candidate list.  The scan hands its mask to CandidateSink::begin before it refines anything:
// each lane counts its bits, an 8-lane inclusive prefix by shuffles gives every lane its write offset
// (lane index and interval order are already ascending), lane 0 writes the two ends and the count and
// the lanes clear the row's tail; put() then stores each root as it is refined.  An exact zero of f at
// t_start is a candidate the scan never tests (lane 0 lists it first); a zero polynomial has no roots
// (rpoly.cpp:62-65): its list is the two ends, while the search itself stays the shared code's.
// Outputs are write-once and small: plain vector stores.
#include "mtg_extrema_common.h"

namespace mtg {

namespace {

constexpr int kSegL = 8;            // lanes per item
constexpr int kSegThreads = 256;    // 4 waves, 32 items per block
constexpr int kSegGroups = kSegThreads / kSegL;

// waves per SIMD the register budget is built for: the uniform kernel's (mtg_extrema.hip)
template <int N>
constexpr int segment_extrema_waves() { return N <= 10 ? 5 : 1; }

struct CandidateSink {
  double* row;      // this item's [cap] times, or nullptr
  int32_t* count;   // this item's count, or nullptr
  int cap, lane;
  bool want, zero_f, start_root;  // start_root: lane 0 only, f(t_start) == 0
  double t0, t1;
  int idx;  // next write position of this lane

  __device__ __forceinline__ void begin(uint64_t pend) {
    if (!want) return;
    const int c = zero_f ? 0 : __builtin_popcountll(pend) + (start_root ? 1 : 0);
    int incl = c;
#pragma unroll
    for (int m = 1; m < kSegL; m <<= 1) {
      const int v = __shfl_up(incl, m, kSegL);
      if (lane >= m) incl += v;
    }
    const int total = __shfl(incl, kSegL - 1, kSegL);
    idx = 2 + incl - c;
    if (lane == 0) {
      if (count) *count = 2 + total;
      if (row) row[0] = t0, row[1] = t1;
    }
    if (row)
      for (int e = 2 + total + lane; e < cap; e += kSegL) row[e] = 0.0;
    if (start_root && !zero_f) put(t0, 0);
  }
  __device__ __forceinline__ void put(double t, int) {
    if (!want || zero_f) return;
    if (row && idx < cap) row[idx] = t;
    ++idx;
  }
};

template <int N, bool AXIS>
__global__ __launch_bounds__(kSegThreads) __attribute__((amdgpu_waves_per_eu(segment_extrema_waves<N>()))) void segment_extrema_kernel(
    const double* __restrict__ coeffs, const double* __restrict__ times, const double* __restrict__ windows,
    int64_t n_items, int D, int k, unsigned dims_all, int qd, mtg_extremum* __restrict__ out_min,
    mtg_extremum* __restrict__ out_max, double* __restrict__ cand, int32_t* __restrict__ count, int cap,
    int32_t* __restrict__ status) {
  constexpr int L = kSegL;
  constexpr int LF = 2 * N - 2;
  static_assert(kExtremaSamples / L <= 64, "one candidate mask per lane (CandidateSink::begin runs once)");
  extern __shared__ __attribute__((aligned(16))) double xlds[];
  const int tid = threadIdx.x;
  const int lane = tid % L, grp = tid / L;
  const int64_t item = (int64_t)blockIdx.x * kSegGroups + grp;
  const bool active = item < n_items;
  const int64_t it = active ? item : 0;
  const int64_t seg = AXIS ? it / D : it;
  const int axis = AXIS ? (int)(it - seg * D) : 0;
  const unsigned dims = AXIS ? 1u << axis : dims_all;
  const int ndim = AXIS ? 1 : __builtin_popcount(dims);
  const int nd = N - k;
  const int GS = extrema_group_doubles(N, qd);
  double* gf = xlds + (size_t)grp * GS;  // this group's f, then q, then the padded q1
  double* gq = gf + 2 * N;
  double* gq1 = gq + qd * N;

  double t0 = 0.0, t1;
  bool ok;
  if (windows) {
    t0 = windows[2 * seg], t1 = windows[2 * seg + 1];
    ok = fabs(t0) <= DBL_MAX && fabs(t1) <= DBL_MAX && t0 <= t1;
  } else {
    t1 = times[seg];
    ok = t1 > 0.0 && t1 <= DBL_MAX;
  }
  const double* cs = coeffs + (seg * D) * N;
  double f[LF];
  extrema_form_f<N, L>(gf, gq, gq1, qd, dims, ndim, k, lane, true, [&](int d, int j) { return cs[d * N + j]; }, f);

  double* row = cand ? cand + item * cap : nullptr;
  Ext lo{0.0, DBL_MAX, 0x7fffffff}, hi{0.0, -DBL_MAX, 0x7fffffff};
  if (active && ok) {
    bool zero_f = true;
#pragma unroll
    for (int j = 0; j < LF; ++j) zero_f = zero_f && f[j] == 0.0;
    CandidateSink sink{row,   count ? count + item : nullptr,        cap, lane, cand != nullptr || count != nullptr,
                       zero_f, lane == 0 && horner<LF>(f, t0) == 0.0, t0,  t1,   0};
    if constexpr (AXIS) {
      auto val = [&](double t) {  // the signed p_d^(k)(t) from the staged q
        double acc = 0.0;
#pragma unroll
        for (int j = N - 1; j >= 0; --j) acc = acc * t + gq[j];
        return acc;
      };
      extrema_scan_on<N, L, true>(f, t0, t1, lane, 1, val, sink, lo, hi);
    } else {
      const bool staged = ndim <= qd;  // q of every selected dimension is in LDS
      auto mag = [&](double t) {       // (the text of mtg_extrema.hip's)
        double s = 0.0;
        if (staged) {
          s = extrema_sumsq_staged<N>(gq, ndim, t);
        } else {
          for (int d = 0; d < D; ++d) {
            if (!((dims >> d) & 1u)) continue;
            double qv[N];
#pragma unroll
            for (int j = 0; j < N; ++j) qv[j] = j < nd ? cs[d * N + j + k] * c_ff.v[j + k][k] : 0.0;
            double acc = 0.0;
#pragma unroll
            for (int j = N - 1; j >= 0; --j) acc = acc * t + qv[j];
            s += acc * acc;
          }
        }
        return sqrt(s);
      };
      extrema_scan_on<N, L, true>(f, t0, t1, lane, 1, mag, sink, lo, hi);
    }
  }
  extrema_group_reduce<L>(lo, hi);
  if (!active) return;
  if (ok) {
    if (lane == 0) {
      if (out_min) out_min[item] = mtg_extremum{lo.t, lo.v, 0, 0};
      if (out_max) out_max[item] = mtg_extremum{hi.t, hi.v, 0, 0};
    }
  } else {  // MTG_TRAJ_BAD_TIME: every floating output NaN, the count 0
    const double nan = __builtin_nan("");
    if (lane == 0) {
      if (out_min) out_min[item] = mtg_extremum{nan, nan, 0, 0};
      if (out_max) out_max[item] = mtg_extremum{nan, nan, 0, 0};
      if (count) count[item] = 0;
    }
    if (row)
      for (int e = lane; e < cap; e += L) row[e] = nan;
  }
  if (status && lane == 0 && axis == 0) status[seg] = ok ? MTG_TRAJ_OK : MTG_TRAJ_BAD_TIME;
}

template <int N, bool AXIS>
hipError_t launch_segment_extrema_n(const double* coeffs, const double* times, const double* windows, int64_t S, int D,
                                    int k, unsigned dims, mtg_extremum* mn, mtg_extremum* mx, double* cand,
                                    int32_t* count, int cap, int32_t* status, hipStream_t stream) {
  const int ndim = AXIS ? 1 : __builtin_popcount(dims);
  const int qd = ndim < kExtremaQD ? ndim : kExtremaQD;
  const size_t lds = sizeof(double) * (size_t)kSegGroups * extrema_group_doubles(N, qd);
  if (lds > kMaxLdsPerBlock) return hipErrorInvalidValue;
  const int64_t n_items = AXIS ? S * D : S;
  const int64_t blocks = (n_items + kSegGroups - 1) / kSegGroups;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  launch_kernel((segment_extrema_kernel<N, AXIS>), dim3((unsigned)blocks), dim3(kSegThreads), (uint32_t)lds, stream,
                coeffs, times, windows, n_items, D, k, dims, qd, mn, mx, cand, count, cap, status);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_segment_extrema(bool axis, int N, const double* coeffs, const double* times, const double* windows,
                                  int64_t S, int D, int derivative, unsigned dims, mtg_extremum* mn, mtg_extremum* mx,
                                  double* cand, int32_t* count, int cap, int32_t* status, hipStream_t stream) {
  if (S == 0) return hipSuccess;
#define MTG_SEG_CASE(n)                                                                                              \
  case n:                                                                                                            \
    return axis ? launch_segment_extrema_n<n, true>(coeffs, times, windows, S, D, derivative, dims, mn, mx, cand,   \
                                                    count, cap, status, stream)                                      \
                : launch_segment_extrema_n<n, false>(coeffs, times, windows, S, D, derivative, dims, mn, mx, cand,  \
                                                     count, cap, status, stream)
  switch (N) {
    MTG_SEG_CASE(2);
    MTG_SEG_CASE(4);
    MTG_SEG_CASE(6);
    MTG_SEG_CASE(8);
    MTG_SEG_CASE(10);
    MTG_SEG_CASE(12);
    default: return hipErrorInvalidValue;
  }
#undef MTG_SEG_CASE
}

}  // namespace mtg
