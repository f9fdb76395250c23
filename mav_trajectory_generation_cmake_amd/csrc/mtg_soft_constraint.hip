// mtg_soft_constraint.hip -- soft-constraint term of the nonlinear objective
// (mtg_soft_constraint_cost_batch): the reference's getCostAndGradientSoftConstraints
// (polynomial_optimization_nonlinear_impl.h:2025-2091) over evaluateMaximumMagnitudeAsSoftConstraint
// (:2396-2425) and PolynomialOptimization::computeMaximumOfMagnitude (lin_impl:470-503).
//
// Reference: J_sc = sum_c min(maximum_cost, exp(weight (max_c - limit_c) / limit_c)), max_c the
// maximum of |p^(k_c)| over the candidates t = 0 and the roots of every segment, then t = T of the
// last one.  The gradient is a central difference over every free derivative of every dimension; each
// side sets the free constraints, re-forms every segment and searches every segment again.
//
// Here: one block per trajectory, groups of 8 lanes per segment search (mtg_extrema_common.h, the
// search of mtg_extrema.hip), one launch.
// * The block stages the vertex values and times in LDS and forms the coefficients there
//   (mtg_vertex_common.h, the code of mtg_vertex.hip's coefficients_from_vertices_kernel).
// * Phase A: a group per (constraint, segment) searches the unperturbed segment; the segments' maxima
//   go to LDS, and per constraint the prefix maxima pre[i] = max over segments < i and the suffix maxima
//   suf[i] = max over segments >= i.  maxima_out is the sequential scan of the segments (a later
//   segment replaces an earlier one only when strictly larger); the cost is summed in constraint order.
// * Phase B (only with grad_out): perturbing the free derivative (vertex v, order k) of dimension d
//   changes the coefficients of segments v - 1 and v only, and only in dimension d.  A group per
//   (free index, dimension) re-forms those two polynomials from the perturbed vertex values, searches
//   the one or two touched segments (the other dimensions are read from the unperturbed coefficients)
//   and takes max(pre[first touched], touched maxima, suf[last touched + 1]): the trajectory maximum
//   the full re-evaluation finds, because every other segment's coefficients -- hence its maximum, to
//   the bit -- are unchanged.  The group sums the constraints' costs of the left and the right side in
//   constraint order and writes (right - left) / (2 increment): no atomics, a fixed order, and nothing
//   that depends on the trajectory's place in the batch.
//   The last segment carries the t = T candidate; vertex 0 and vertex K touch one segment.
#include "mtg_extrema_common.h"
#include "mtg_vertex_common.h"

namespace mtg {

constexpr int kSoftLanes = 8;  // lanes per segment search (mtg_extrema.hip: the fastest at K = 10)
// Waves per SIMD the register budget is built for: four at N <= 10 (the block's LDS allows four blocks
// of four waves per CU), the compiler's own choice at N = 12, which would spill heavily at four
// (measurements: DESIGN.md 3.9).
template <int N>
constexpr int soft_waves() { return N <= 10 ? 4 : 1; }

struct SoftParams {
  int C;
  int derivative[8];
  double limit[8];
  double weight, maximum_cost, increment;
};

// LDS doubles of the block apart from the groups' search areas: vertex values, times, coefficients,
// prefix / suffix maxima, the segments' maxima, the constraints (8 limits, 8 derivatives) and the
// free-index table (ints, counted in doubles)
__host__ __device__ constexpr int soft_fixed_doubles(int N, int D, int K, int C) {
  return (K + 1) * (N / 2) * D + K + K * D * N + 2 * C * (K + 1) + 3 * C * K + 12 + ((K + 1) * (N / 2) + 2) / 2 + 1;
}
__host__ __device__ constexpr int soft_group_doubles(int N, int D) { return extrema_group_doubles(N, D) + 2 * N; }

namespace {

// min(maximum_cost, exp(weight (max - limit) / limit)) as the reference writes it (nl_impl:2410-2416)
__device__ __forceinline__ double soft_term(const SoftParams& p, double limit, double mx) {
  const double abs_violation = mx - limit;
  const double relative_violation = abs_violation / limit;
  const double e = exp(relative_violation * p.weight);
  return e < p.maximum_cost ? e : p.maximum_cost;
}

template <int N>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(soft_waves<N>()))) void soft_constraint_kernel(const double* __restrict__ values,
                                                              const uint8_t* __restrict__ mask,
                                                              const double* __restrict__ times, SoftParams p,
                                                              double* __restrict__ cost, double* __restrict__ grad,
                                                              mtg_extremum* __restrict__ maxima,
                                                              int32_t* __restrict__ status, int K, int D) {
  constexpr int H = N / 2, L = kSoftLanes, LF = 2 * N - 2;
  extern __shared__ __attribute__((aligned(16))) double slds[];
  const int V = K + 1, xsz = V * H * D, C = p.C, VH = V * H;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid % L, grp = tid / L, ngrp = nthr / L;
  const int64_t b = blockIdx.x;
  double* xv = slds;                  // [V][H][D]
  double* tl = xv + xsz;              // [K]
  double* co = tl + K;                // [K][D][N]
  double* pre = co + K * D * N;       // [C][K + 1]
  double* suf = pre + C * (K + 1);    // [C][K + 1]
  double* seg = suf + C * (K + 1);    // [C][K] x (t, v, ord): the segments' maxima
  double* lim = seg + 3 * C * K;      // [8] the constraints' limits and, as ints, [8] their derivatives:
  int* kd = reinterpret_cast<int*>(lim + 8);  // indexed per lane, so in LDS and not in the argument registers
  int* fidx = kd + 8;                 // [0] = n_free, then the free slots v * H + k
  double* garea = slds + soft_fixed_doubles(N, D, K, C) + (size_t)grp * soft_group_doubles(N, D);
  double* gf = garea;  // this group's f, then q, then the padded q1 (extrema_group_doubles(N, D))
  double* gq = gf + 2 * N;
  double* gq1 = gq + D * N;
  double* pc = garea + extrema_group_doubles(N, D);  // perturbed coefficients of segments v - 1, v: [2][N]

  for (int e = tid; e < xsz; e += nthr) xv[e] = values[b * xsz + e];
  for (int e = tid; e < K; e += nthr) tl[e] = times[b * K + e];
  if (tid == 0) {
#pragma unroll
    for (int c = 0; c < 8; ++c) lim[c] = p.limit[c], kd[c] = p.derivative[c];
    int n = 0;
    if (grad) {
      const unsigned hm = (1u << H) - 1u;
      for (int v = 0; v < V; ++v) {
        const unsigned mv = mask[b * V + v] & hm;
        for (int k = 0; k < H; ++k)
          if (!((mv >> k) & 1u)) fidx[1 + n++] = v * H + k;
      }
    }
    fidx[0] = n;
  }
  __syncthreads();
  bool bad = false;
  for (int i = 0; i < K; ++i) bad |= !(tl[i] > 0.0 && tl[i] <= DBL_MAX);
  const int nfree = fidx[0];
  if (grad) {  // entries >= n_free are 0; so is every entry of a trajectory with a bad time
    double* g = grad + b * (int64_t)D * VH;
    for (int e = tid; e < D * VH; e += nthr)
      if (bad || e % VH >= nfree) g[e] = 0.0;
  }
  if (bad) {
    if (tid == 0) {
      cost[b] = __builtin_nan("");
      if (status) status[b] = MTG_TRAJ_BAD_TIME;
    }
    if (maxima && tid < C) maxima[b * C + tid] = mtg_extremum{__builtin_nan(""), __builtin_nan(""), 0, 0};
    return;
  }
  for (int it = tid; it < K * D; it += nthr) {
    const int i = it / D, d = it - i * D;
    coefficients_from_ends<N>([&](int e, int k) { return xv[((i + e) * H + k) * D + d]; }, tl[i], co + it * N);
  }
  __syncthreads();

  const unsigned dims = (1u << D) - 1u;
  // the maximum of derivative k over segment i, with dimension pd read from pcs instead of co (pd < 0:
  // none); every lane of the group returns it.  Lanes of a group without a segment run along.
  auto search = [&](int i, int k, int pd, const double* pcs, bool active) {
    const int ii = active ? i : 0;
    const double T = active ? tl[ii] : 0.0;
    const double* cs = co + ii * D * N;
    double f[LF];
    extrema_form_f<N, L>(gf, gq, gq1, D, dims, D, k, lane, true,
                         [&](int d, int j) { return d == pd ? pcs[j] : cs[d * N + j]; }, f);
    Ext lo{0.0, DBL_MAX, 0x7fffffff}, hi{0.0, -DBL_MAX, 0x7fffffff};
    if (active)  // t = T only after the last segment, behind its roots (lin_impl:494-499)
      extrema_scan<N, L>(f, T, lane, ii == K - 1 ? 0x7ffffffe : -1,
                         [&](double t) { return sqrt(extrema_sumsq_staged<N>(gq, D, t)); }, lo, hi);
    extrema_group_reduce<L>(lo, hi);
    return hi;
  };

  // ---- phase A: the unperturbed segments
  for (int it0 = 0; it0 < C * K; it0 += ngrp) {
    const int it = it0 + grp;
    const bool own = it < C * K;
    const int c = own ? it / K : 0, i = own ? it - c * K : 0;
    const Ext hi = search(i, kd[c], -1, co, own);
    if (own && lane == 0) seg[3 * it] = hi.t, seg[3 * it + 1] = hi.v, seg[3 * it + 2] = (double)hi.ord;
  }
  __syncthreads();
  if (tid < C) {
    const int c = tid;
    const double* sc = seg + 3 * c * K;
    mtg_extremum best{0.0, 0.0, 0, 0};  // Extremum(): time 0, value 0, segment 0
    double m = 0.0;
    for (int i = 0; i < K; ++i) {
      pre[c * (K + 1) + i] = m;
      const double v = sc[3 * i + 1];
      if (v > best.value) best = mtg_extremum{sc[3 * i], v, i, 0};
      if (v > m) m = v;
    }
    pre[c * (K + 1) + K] = m;
    m = 0.0;
    suf[c * (K + 1) + K] = 0.0;
    for (int i = K - 1; i >= 0; --i) {
      const double v = sc[3 * i + 1];
      if (v > m) m = v;
      suf[c * (K + 1) + i] = m;
    }
    if (maxima) maxima[b * C + c] = best;
  }
  __syncthreads();
  if (tid == 0) {
    double J = 0.0;
    for (int c = 0; c < C; ++c) J += soft_term(p, lim[c], suf[c * (K + 1)]);
    cost[b] = J;
    if (status) status[b] = MTG_TRAJ_OK;
  }
  if (!grad) return;

  // ---- phase B: a group per (dimension, free index); both sides, every constraint, <= 2 segments
  const int pairs = nfree * D;
  for (int p0 = 0; p0 < pairs; p0 += ngrp) {
    const int pair = p0 + grp;
    const bool own = pair < pairs;
    const int d = own ? pair / nfree : 0, n = own ? pair - d * nfree : 0;
    const int slot = own ? fidx[1 + n] : 0;
    const int v = slot / H, k = slot - v * H;
    const bool has0 = own && v > 0, has1 = own && v < K;  // segments v - 1 and v
    const int i0 = has0 ? v - 1 : 0, i1 = has1 ? v : 0;
    const int first = has0 ? v - 1 : v, last = has1 ? v : v - 1;  // the touched segments
    // one search per step: step = (side, constraint, which touched segment); left side (x - increment)
    // first, as the reference, the constraints in order
    double side_cost[2] = {0.0, 0.0};
    double m = 0.0;
    for (int step = 0; step < 4 * C; ++step) {
      const int side = step / (2 * C), c = (step >> 1) % C, s = step & 1;
      if (step % (2 * C) == 0) {  // a new side: re-form the two touched polynomials of dimension d
        const double delta = side == 0 ? -p.increment : p.increment;
        lds_fence();  // (the previous search's reads of pc)
        if (lane < 2) {  // lane 0: segment v - 1 (its end is vertex v), lane 1: segment v (its start is)
          const int i = lane == 0 ? i0 : i1;
          const bool has = lane == 0 ? has0 : has1;
          coefficients_from_ends<N>(
              [&](int e, int q) {
                const double xq = xv[((i + e) * H + q) * D + d];
                return has && i + e == v && q == k ? xq + delta : xq;
              },
              tl[i], pc + lane * N);
        }
        lds_fence();
      }
      if (s == 0) {  // the untouched segments' maximum
        m = 0.0;
        if (own) {
          const double a = pre[c * (K + 1) + first], z = suf[c * (K + 1) + last + 1];
          m = a > z ? a : z;
        }
      }
      const bool has = s == 0 ? has0 : has1;
      const Ext hs = search(s == 0 ? i0 : i1, kd[c], d, pc + s * N, has);
      if (has && hs.v > m) m = hs.v;
      if (s == 1) side_cost[side] += soft_term(p, lim[c], m);
    }
    if (own && lane == 0) grad[(b * D + d) * (int64_t)VH + n] = (side_cost[1] - side_cost[0]) / (2.0 * p.increment);
  }
}

template <int N>
hipError_t launch_soft_n(const double* values, const uint8_t* mask, const double* times, const SoftParams& p,
                         double* cost, double* grad, mtg_extremum* maxima, int32_t* status, int64_t B, int K, int D,
                         hipStream_t stream) {
  const int threads = soft_constraint_threads(N, D, K, p.C);
  if (threads == 0) return hipErrorInvalidValue;
  const size_t lds = soft_constraint_lds_bytes(N, D, K, p.C, threads);
  launch_kernel((soft_constraint_kernel<N>), dim3((unsigned)B), dim3(threads), (uint32_t)lds, stream, values, mask,
                times, p, cost, grad, maxima, status, K, D);
  return hipGetLastError();
}

}  // namespace

size_t soft_constraint_lds_bytes(int N, int D, int K, int C, int threads) {
  return sizeof(double) *
         ((size_t)soft_fixed_doubles(N, D, K, C) + (size_t)(threads / kSoftLanes) * soft_group_doubles(N, D));
}

// threads per block: 256 (32 searches in flight) while the block's LDS stays within 64 KiB, else 128
// or 64 (fewer search areas); 0: the trajectory does not fit
int soft_constraint_threads(int N, int D, int K, int C) {
  for (int t = 256; t >= 64; t >>= 1)
    if (soft_constraint_lds_bytes(N, D, K, C, t) <= kMaxLdsPerBlock) return t;
  return 0;
}

hipError_t launch_soft_constraint_cost(int N, const double* values, const uint8_t* mask, const double* times,
                                       const mtg_soft_constraint_params& params, double* cost, double* grad,
                                       mtg_extremum* maxima, int32_t* status, int64_t B, int K, int D,
                                       hipStream_t stream) {
  if (B == 0) return hipSuccess;
  if (B > 0x7fffffff) return hipErrorInvalidValue;
  SoftParams p{};
  p.C = params.n_constraints;
  for (int c = 0; c < p.C; ++c) p.derivative[c] = params.derivative[c], p.limit[c] = params.limit[c];
  p.weight = params.weight;
  p.maximum_cost = params.maximum_cost;
  p.increment = params.increment;
  switch (N) {
    case 6: return launch_soft_n<6>(values, mask, times, p, cost, grad, maxima, status, B, K, D, stream);
    case 8: return launch_soft_n<8>(values, mask, times, p, cost, grad, maxima, status, B, K, D, stream);
    case 10: return launch_soft_n<10>(values, mask, times, p, cost, grad, maxima, status, B, K, D, stream);
    case 12: return launch_soft_n<12>(values, mask, times, p, cost, grad, maxima, status, B, K, D, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mtg
