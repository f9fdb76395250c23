// mtg_extrema.hip -- minimum and maximum magnitude of a derivative over whole trajectories
// (mtg_min_max_magnitude_batch): the reference's Trajectory::computeMinMaxMagnitude
// (src/trajectory.cpp:181-218) over Segment::computeMinMaxMagnitudeCandidates /
// selectMinMaxMagnitudeFromCandidates (src/segment.cpp:82-196).
//
// Reference: per segment the candidate times are t = 0, t = T and the real roots in [0, T] of
//   sum_{d in dims} conv(p_d^(k), p_d^(k+1))      (the derivative of |p^(k)|^2 / 2; one selected
//                                                   dimension: the roots of p^(k+1) alone)
// found by Jenkins-Traub (src/rpoly.cpp) with |imag| <= DBL_EPSILON as "real"; the magnitude
// sqrt(sum p_d^(k)(t)^2) is evaluated at every candidate and the segment minimum / maximum taken,
// then the trajectory's (strict comparisons: the first segment wins ties).
//
// Here: a group of L lanes per (trajectory, segment) (L = 8 lanes of one wave for K <= 64; the
// block holds whole trajectories).  The real roots in [0, T] are isolated by the sign changes of the
// root polynomial f on kExtremaSamples + 1 uniform samples -- lane l of the group evaluates f on its
// own run of kExtremaSamples / L sample intervals -- and refined by safeguarded Newton-bisection until
// f is within its rounding error of 0.  The reference's own test checks its candidates the same way, against sampled extrema
// (test/test_polynomial_optimization.cpp:447-487).  A root pair closer than T / kExtremaSamples (no
// sign change between samples) is not isolated; at such a pair |p^(k)| is flat to second order, so
// the extreme values move by O((T/S)^2) relative.
//
// Work layout (latency, not arithmetic, set the cost of the direct versions):
// * the group stages the derivative coefficients q_d = p_d^(k), q1_d = p_d^(k+1) of up to QD selected
//   dimensions in LDS with one batch of loads (QD = 4 unless the block's LDS would not fit), forms
//   f = sum_d conv(q_d, q1_d) there, each lane its share of the coefficients, and evaluates the
//   magnitude at the candidates from the staged q_d (more than QD dimensions: from global memory);
// * the scan only sets bits -- sample intervals with a sign change, samples where f is exactly 0,
//   the end points -- and one loop then takes each lane's candidates lowest bit first, refining the
//   brackets: a wave runs the refinement once per candidate a lane holds (~1), and the Newton
//   iteration, the magnitude and the candidate comparison exist once in the code;
// * the Newton step takes f and f' from one Horner pass.
// Candidates carry their position in the sequential order (t = 0, t = T, then the roots by sample
// index), and the group's minimum and maximum are reduced across lanes with that order as the
// tie-break: the same candidate wins as in a sequential scan (std::max / std::min keep the earlier
// candidate on ties).
// The per-segment part (staging, forming f, the scan, the refinement, the magnitude, the group's
// reduction) is mtg_extrema_common.h, shared with mtg_soft_constraint.hip; this file keeps the
// kernel around it: the block's geometry and the trajectory's scan over its segments.
#include "mtg_extrema_common.h"

namespace mtg {

constexpr int kExtremaMaxThreads = 512;

namespace {

// L lanes per (trajectory, segment); tpb whole trajectories per block; qd dimensions staged per
// pass.  LDS per group (extrema_group_doubles): f [2N]; q [qd][N]; q1 with zero pads,
// [Z q1_0 Z q1_1 ... q1_{qd-1} Z] (N doubles each), so that the convolution reads q1[n - a] at a
// fixed offset from n for every a, without bounds selects; then the groups' extremes.
// Waves per SIMD the register budget is built for: at N <= 10 five (96 VGPRs, ~14 spilled: config 2,
// L = 8, 0.104 -> 0.089 ms against four without spills); N = 12 spills ~40 at five, so the compiler's
// own choice.
template <int N>
constexpr int extrema_waves() { return N <= 10 ? 5 : 1; }

template <int N, int L>
__global__ __launch_bounds__(kExtremaMaxThreads) __attribute__((amdgpu_waves_per_eu(extrema_waves<N>()))) void min_max_magnitude_kernel(
    const double* __restrict__ coeffs, const double* __restrict__ times, int64_t B, int K, int D, int k,
    unsigned dims, int tpb, int qd, mtg_extremum* __restrict__ out_min, mtg_extremum* __restrict__ out_max) {
  constexpr int LF = 2 * N - 2;  // root polynomial length bound (conv of N and N-1 terms)
  extern __shared__ __attribute__((aligned(16))) double xlds[];
  const int tid = threadIdx.x;
  const int lane = tid % L, grp = tid / L;  // the group of L lanes owns one (trajectory, segment)
  const int ngrp = tpb * K;                 // groups of the block
  const int bl = grp / K, i = grp - bl * K;
  const int64_t b = (int64_t)blockIdx.x * tpb + bl;
  const bool active = grp < ngrp && b < B;
  const int nd = N - k;  // p^(k) coefficient count
  const int ndim = __builtin_popcount(dims);
  const int GS = extrema_group_doubles(N, qd);
  Ext* smin = reinterpret_cast<Ext*>(xlds + (size_t)ngrp * GS);
  Ext* smax = smin + ngrp;
  const int g = grp < ngrp ? grp : 0;
  double* gf = xlds + (size_t)g * GS;  // this group's f, then q, then the padded q1
  double* gq = gf + 2 * N;
  double* gq1 = gq + qd * N;  // q1_c starts at gq1 + (2c + 1) N

  Ext lo{0.0, DBL_MAX, 0x7fffffff}, hi{0.0, -DBL_MAX, 0x7fffffff};
  const int64_t bb = active ? b : 0;
  const int ii = active ? i : 0;
  const double T = times[bb * K + ii];
  const double* cs = coeffs + ((bb * K + ii) * D) * N;
  double f[LF];
  extrema_form_f<N, L>(gf, gq, gq1, qd, dims, ndim, k, lane, grp < ngrp, [&](int d, int j) { return cs[d * N + j]; }, f);

  if (active) {
    const bool staged = ndim <= qd;  // q of every selected dimension is in LDS
    auto mag = [&](double t) {
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
    extrema_scan<N, L>(f, T, lane, 1, mag, lo, hi);  // t = T right after t = 0 (polynomial.cpp:38-39)
  }
  extrema_group_reduce<L>(lo, hi);
  if (lane == 0 && grp < ngrp) smin[grp] = lo, smax[grp] = hi;
  __syncthreads();
  if (active && i == 0 && lane == 0) {  // trajectory's segments in order; strict: the first segment wins ties
    Ext m = smin[grp], M = smax[grp];
    int im = 0, iM = 0;
    for (int q = 1; q < K; ++q) {
      const Ext a = smin[grp + q], c = smax[grp + q];
      if (a.v < m.v) m = a, im = q;
      if (c.v > M.v) M = c, iM = q;
    }
    if (out_min) out_min[b] = mtg_extremum{m.t, m.v, im, 0};
    if (out_max) out_max[b] = mtg_extremum{M.t, M.v, iM, 0};
  }
}

// lanes per segment and trajectories per block: 8 lanes while a trajectory fits a block (K <= 64),
// then fewer; the trajectories per block that keep the block's waves fullest (K = 10: 8 lanes, 4
// trajectories, 320 threads = 5 full waves).  (Config 2, same box: 16 lanes 0.130 ms, 8 lanes 0.104,
// 4 lanes 0.106 -- fewer lanes share the per-segment work of forming f over fewer waves, more
// lanes scan fewer samples each.)
void extrema_geometry(int K, int* lanes, int* tpb, int* threads) {
  int L = 8;
  while (L > 1 && K * L > kExtremaMaxThreads) L >>= 1;
  int best_t = 1;
  double best_u = 0.0;
  for (int t = 1; t * K * L <= kExtremaMaxThreads; ++t) {
    const int th = (t * K * L + 63) / 64 * 64;
    const double u = (double)(t * K * L) / th;
    if (u > best_u + 1e-9) best_u = u, best_t = t;
  }
  *lanes = L;
  *tpb = best_t;
  *threads = (best_t * K * L + 63) / 64 * 64;
}

template <int N, int L>
hipError_t launch_extrema_nl(const double* coeffs, const double* times, int64_t B, int K, int D, int k, unsigned dims,
                             int tpb, int threads, mtg_extremum* mn, mtg_extremum* mx, hipStream_t stream) {
  // dimensions staged per pass: as many as the selection needs (at most 4) while the block's LDS
  // stays within kMaxLdsPerBlock, at least 1
  const int ndim = __builtin_popcount(dims);
  auto bytes = [&](int qd) {
    return sizeof(double) * (size_t)tpb * K * extrema_group_doubles(N, qd) + 2 * sizeof(Ext) * (size_t)tpb * K;
  };
  int qd = ndim < kExtremaQD ? ndim : kExtremaQD;
  while (qd > 1 && bytes(qd) > kMaxLdsPerBlock) --qd;
  const size_t lds = bytes(qd);
  if (lds > kMaxLdsHard) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((B + tpb - 1) / tpb)), block(threads);
  launch_kernel((min_max_magnitude_kernel<N, L>), grid, block, (uint32_t)lds, stream, coeffs, times, B, K, D, k, dims,
                tpb, qd, mn, mx);
  return hipGetLastError();
}

template <int N>
hipError_t launch_extrema_n(const double* coeffs, const double* times, int64_t B, int K, int D, int k, unsigned dims,
                            mtg_extremum* mn, mtg_extremum* mx, hipStream_t stream) {
  int L, tpb, threads;
  extrema_geometry(K, &L, &tpb, &threads);
  switch (L) {
    case 16: return launch_extrema_nl<N, 16>(coeffs, times, B, K, D, k, dims, tpb, threads, mn, mx, stream);
    case 8: return launch_extrema_nl<N, 8>(coeffs, times, B, K, D, k, dims, tpb, threads, mn, mx, stream);
    case 4: return launch_extrema_nl<N, 4>(coeffs, times, B, K, D, k, dims, tpb, threads, mn, mx, stream);
    case 2: return launch_extrema_nl<N, 2>(coeffs, times, B, K, D, k, dims, tpb, threads, mn, mx, stream);
    default: return launch_extrema_nl<N, 1>(coeffs, times, B, K, D, k, dims, tpb, threads, mn, mx, stream);
  }
}

}  // namespace

hipError_t launch_min_max_magnitude(int N, const double* coeffs, const double* times, int64_t B, int K, int D,
                                    int derivative, unsigned dims, mtg_extremum* mn, mtg_extremum* mx,
                                    hipStream_t stream) {
  if (K < 1 || K > 256) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  switch (N) {
    case 2: return launch_extrema_n<2>(coeffs, times, B, K, D, derivative, dims, mn, mx, stream);
    case 4: return launch_extrema_n<4>(coeffs, times, B, K, D, derivative, dims, mn, mx, stream);
    case 6: return launch_extrema_n<6>(coeffs, times, B, K, D, derivative, dims, mn, mx, stream);
    case 8: return launch_extrema_n<8>(coeffs, times, B, K, D, derivative, dims, mn, mx, stream);
    case 10: return launch_extrema_n<10>(coeffs, times, B, K, D, derivative, dims, mn, mx, stream);
    case 12: return launch_extrema_n<12>(coeffs, times, B, K, D, derivative, dims, mn, mx, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mtg
