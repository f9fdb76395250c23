// mtg_extrema_common.h -- the per-segment extremum search shared by the kernels that need it:
// mtg_extrema.hip (mtg_min_max_magnitude_batch), mtg_soft_constraint.hip
// (mtg_soft_constraint_cost_batch) and mtg_segment_extrema.hip (mtg_segment_min_max_*_batch).  One copy of: the staging of q_d = p_d^(k), q1_d = p_d^(k+1) in a
// group's LDS, the forming of the root polynomial f = sum_d conv(q_d, q1_d), the scan of f on
// kExtremaSamples + 1 samples, the safeguarded Newton refinement, the magnitude at a candidate and the
// group's reduction.  The algorithm and its layout are described in mtg_extrema.hip.
//
// A group of L consecutive lanes of one wave owns one segment.  The callers differ in where the
// segment's coefficients come from (`coef(d, j)`: global memory there, LDS here) and in the candidate
// set (`end_ord`: the position of t = T in the sequential candidate order, or < 0 when t = T is no
// candidate of this segment).
#pragma once

#include "mtg_device.h"

namespace mtg {

constexpr int kExtremaSamples = 256;
constexpr int kExtremaQD = 4;  // dimensions staged per pass (at most)
#ifndef MTG_EXTREMA_CS
#define MTG_EXTREMA_CS 16
#endif

// falling factorials j!/(j-k)!, j, k < 12 (exact in FP64)
struct FallingTable {
  double v[12][12];
};
constexpr FallingTable make_falling_table() {
  FallingTable t{};
  for (int j = 0; j < 12; ++j)
    for (int k = 0; k < 12; ++k) {
      double f = 1.0;
      for (int q = 0; q < k; ++q) f *= (double)(j - q);
      t.v[j][k] = k > j ? 0.0 : f;
    }
  return t;
}
static __constant__ FallingTable c_ff = make_falling_table();

// LDS doubles of one group: f, then q_d of qd dimensions, then their q1_d with zero pads
__host__ __device__ constexpr int extrema_group_doubles(int N, int qd) { return 2 * N + qd * N + (2 * qd + 1) * N; }

namespace {

struct Ext {
  double t, v;
  int ord;  // position in the sequential candidate order (tie-break)
};

// Horner over the whole zero-padded array: leading zero coefficients leave acc exactly 0, so the
// value is the same as over the first len terms, without a select per term
template <int L>
__device__ __forceinline__ double horner(const double (&c)[L], double t) {
  double acc = 0.0;
#pragma unroll
  for (int j = L - 1; j >= 0; --j) acc = acc * t + c[j];
  return acc;
}

// a beats b as the maximum (larger value; on a tie the earlier candidate)
__device__ __forceinline__ bool better_max(const Ext& a, const Ext& b) { return a.v > b.v || (a.v == b.v && a.ord < b.ord); }
__device__ __forceinline__ bool better_min(const Ext& a, const Ext& b) { return a.v < b.v || (a.v == b.v && a.ord < b.ord); }

__device__ __forceinline__ Ext shfl_xor(const Ext& e, int m, int width) {
  return Ext{__shfl_xor(e.t, m, width), __shfl_xor(e.v, m, width), __shfl_xor(e.ord, m, width)};
}

// safeguarded Newton-bisection on [ta, tb] (a sign change of f, f(ta) = fa, f(tb) = fb) from the
// secant point, until f(x) is within its rounding error of 0; f and f' from one Horner pass (as
// mtg_host_extrema_common.h)
template <int LF>
__device__ __forceinline__ double refine(const double (&f)[LF], double ta, double tb, double fa, double fb) {
  double a0 = ta, b0 = tb, fa0 = fa, x = ta - fa * ((tb - ta) / (fb - fa));
  if (!(x > ta && x < tb)) x = 0.5 * (ta + tb);
  for (int it = 0; it < 60; ++it) {
    double fx = 0.0, dfx = 0.0, ga = 0.0;  // ga: sum |f_j| |x|^j, the scale of f(x)'s rounding error
    const double ax = fabs(x);
#pragma unroll
    for (int j = LF - 1; j >= 0; --j) {
      dfx = dfx * x + fx;
      fx = fx * x + f[j];
      ga = ga * ax + fabs(f[j]);
    }
    // f(x) indistinguishable from 0 (below its own evaluation error): converged.  Without this the
    // Newton steps wander by the rounding noise and only the bisection bound ends them (~45 steps).
    if (fabs(fx) <= (2.0 * LF * DBL_EPSILON) * ga) break;
    if ((fx < 0.0) == (fa0 < 0.0)) a0 = x, fa0 = fx;
    else b0 = x;
    double xn = x - fx * __builtin_amdgcn_rcp(dfx);  // (a Newton step: an approximate reciprocal will do)
    if (!(xn > a0 && xn < b0)) xn = 0.5 * (a0 + b0);
    if (b0 - a0 <= 4.0 * DBL_EPSILON * fmax(fabs(a0), fabs(b0)) || xn == x) {
      x = xn;
      break;
    }
    x = xn;
  }
  return x;
}

// refine() for the windowed scan, whose sample times are t0 + s h.  In the [0, T] scan ta = (s - 1) h is
// a product, and the compiler contracts it into tb - ta and ta + tb above (one rounding, not two); the
// windowed scan hands in the same two FMAs, written out, so that on [0, T] both scans start every
// refinement from the same point and return the same bits.  (A copy, not a shared body: refine() above
// must keep compiling to the text the trajectory kernels have always had.)
template <int LF>
__device__ __forceinline__ double refine_from(const double (&f)[LF], double ta, double tb, double fa, double fb,
                                              double width, double sum) {
  double a0 = ta, b0 = tb, fa0 = fa, x = ta - fa * (width / (fb - fa));
  if (!(x > ta && x < tb)) x = 0.5 * sum;
  for (int it = 0; it < 60; ++it) {
    double fx = 0.0, dfx = 0.0, ga = 0.0;  // ga: sum |f_j| |x|^j, the scale of f(x)'s rounding error
    const double ax = fabs(x);
#pragma unroll
    for (int j = LF - 1; j >= 0; --j) {
      dfx = dfx * x + fx;
      fx = fx * x + f[j];
      ga = ga * ax + fabs(f[j]);
    }
    // f(x) indistinguishable from 0 (below its own evaluation error): converged.  Without this the
    // Newton steps wander by the rounding noise and only the bisection bound ends them (~45 steps).
    if (fabs(fx) <= (2.0 * LF * DBL_EPSILON) * ga) break;
    if ((fx < 0.0) == (fa0 < 0.0)) a0 = x, fa0 = fx;
    else b0 = x;
    double xn = x - fx * __builtin_amdgcn_rcp(dfx);  // (a Newton step: an approximate reciprocal will do)
    if (!(xn > a0 && xn < b0)) xn = 0.5 * (a0 + b0);
    if (b0 - a0 <= 4.0 * DBL_EPSILON * fmax(fabs(a0), fabs(b0)) || xn == x) {
      x = xn;
      break;
    }
    x = xn;
  }
  return x;
}

// index of the m-th selected dimension (m-th set bit of dims)
__device__ __forceinline__ int sel_dim(unsigned dims, int m) {
  for (int r = 0; r < m; ++r) dims &= dims - 1u;
  return __builtin_ctz(dims);
}

// Stages q, q1 of the selected dimensions (qd at a time) in the group's LDS and forms the root
// polynomial f of derivative k there; every lane of the group returns with f in registers.
// LDS of the group (extrema_group_doubles): gf = f [2N]; gq = q [qd][N]; gq1 = q1 with zero pads,
// [Z q1_0 Z q1_1 ... q1_{qd-1} Z] (N doubles each), so that the convolution reads q1[n - a] at a
// fixed offset from n for every a, without bounds selects.  coef(d, j) is coefficient j of the
// segment's polynomial in dimension d; `own`: the group owns its LDS (other groups' lanes run along
// and store nothing).  After the call gq holds q of the dimensions of the last pass.
template <int N, int L, class Coef>
__device__ __forceinline__ void extrema_form_f(double* gf, double* gq, double* gq1, int qd, unsigned dims, int ndim,
                                               int k, int lane, bool own, Coef coef, double (&f)[2 * N - 2]) {
  constexpr int LF = 2 * N - 2;         // root polynomial length bound (conv of N and N-1 terms)
  constexpr int UF = (LF + L - 1) / L;  // f coefficients per lane
  constexpr int UE0 = (2 * N * kExtremaQD + L - 1) / L;
  constexpr int UE = UE0 < 8 ? UE0 : 8;  // staged entries per lane and round of loads
  if (own)  // the zero pads (never overwritten)
    for (int e = lane; e < (qd + 1) * N; e += L) gq1[(e / N) * 2 * N + e % N] = 0.0;
  // ---- stage q, q1 of qd selected dimensions at a time; lane l forms f[n], n = l, l + L, ...
  double facc[UF];
#pragma unroll
  for (int u = 0; u < UF; ++u) facc[u] = 0.0;
  for (int m0 = 0; m0 < ndim; m0 += qd) {
    const int nc = ndim - m0 < qd ? ndim - m0 : qd;
    for (int e0 = 0; e0 < 2 * N * qd; e0 += UE * L) {  // (one round for L >= 8)
      double sv[UE];
      int se[UE];
#pragma unroll
      for (int u = 0; u < UE; ++u) {  // one batch of loads: entry e = (c, j): q (j < N) or q1 (j >= N)
        const int e = e0 + lane + u * L;
        const int c = e / (2 * N), j = e - c * (2 * N);
        double v = 0.0;
        if (c < nc) {
          const int d = sel_dim(dims, m0 + c);
          const int jj = j < N ? j : j - N, kk = j < N ? k : k + 1;
          if (jj + kk < N) v = coef(d, jj + kk) * c_ff.v[jj + kk][kk];
        }
        sv[u] = v;
        se[u] = e < 2 * N * qd ? (j < N ? c * N + j : qd * N + (2 * c + 1) * N + (j - N)) : -1;
      }
#pragma unroll
      for (int u = 0; u < UE; ++u)
        if (se[u] >= 0 && own) gq[se[u]] = sv[u];
    }
    lds_fence();  // (the group is L consecutive lanes of one wave)
#pragma unroll
    for (int u = 0; u < UF; ++u) {
      const int n = lane + u * L;
      if (n >= LF) continue;
      if (ndim == 1) {  // one dimension: the roots of p^(k+1) (segment.cpp:124-130); (n >= N: a pad)
        facc[u] = gq1[N + n];
      } else {  // convolve(d, dd) (polynomial.h convolve), summed over dimensions
        double t = 0.0;
        for (int c = 0; c < nc; ++c) {
          const double* q1n = gq1 + (2 * c + 1) * N + n;  // q1_c[n - a] = q1n[-a] (pads: 0)
#pragma unroll
          for (int a = 0; a < N; ++a) t += gq[c * N + a] * q1n[-a];
        }
        facc[u] += t;
      }
    }
    if (m0 + qd < ndim) lds_fence();  // (read before the next pass overwrites q, q1)
  }
#pragma unroll
  for (int u = 0; u < UF; ++u) {
    const int n = lane + u * L;
    if (n < LF && own) gf[n] = facc[u];
  }
  lds_fence();
#pragma unroll
  for (int j = 0; j < LF; ++j) f[j] = gf[j];
}

// squared magnitude sum_c q_c(t)^2 of the ndim dimensions staged in gq
template <int N>
__device__ __forceinline__ double extrema_sumsq_staged(const double* gq, int ndim, double t) {
  double s = 0.0;
  for (int c = 0; c < ndim; ++c) {
    double acc = 0.0;
#pragma unroll
    for (int j = N - 1; j >= 0; --j) acc = acc * t + gq[c * N + j];
    s += acc * acc;
  }
  return s;
}

// The candidates a scan finds go to a sink: begin(pend) once per candidate mask, after the scan has
// set its bits (bit q: a candidate in sample interval q of the lane's run) and before the first is
// refined, then put(t, ord) per candidate in ascending order.  The kernels that only need the extremes
// pass this one, which compiles to nothing.
struct ExtremaNoSink {
  __device__ __forceinline__ void begin(uint64_t) const {}
  __device__ __forceinline__ void put(double, int) const {}
};

// This lane's share of the segment's candidates on [t0, T] (W: a window with its own start; !W: t0 is
// not read and the scan runs on [0, T], the text the trajectory kernels have always compiled): lane l
// scans its run of kExtremaSamples / L sample intervals; lane 0 takes t = t0 (order 0) and lane L - 1
// takes t = T with order end_ord (end_ord < 0: t = T is not a candidate).  The samples are t0 + s h,
// h = (T - t0) / kExtremaSamples, the last one T itself.  A root found in sample interval s has order
// 2 + s.  The scan only sets bits; one loop then takes each lane's candidates lowest bit first (a
// wave runs the refinement once per candidate a lane holds).  Contract: the caller invokes this only
// for lanes that own a segment (inside its `if (active)`), and with every such lane of the wave at
// this call together -- the candidate loop ends on a wave ballot, which counts the executing lanes
// only, so lanes that skipped the call are not waited for and lanes inside it leave it together.
// lo / hi: the lane's best candidates so far, updated.
template <int N, int L, bool W, class Mag, class Sink>
__device__ __forceinline__ void extrema_scan_on(const double (&f)[2 * N - 2], double t0, double T, int lane,
                                                int end_ord, Mag mag, Sink& sink, Ext& lo, Ext& hi) {
  constexpr int LF = 2 * N - 2;
  constexpr int SPL = kExtremaSamples / L;  // sample intervals per lane
  constexpr int CH = SPL < 64 ? SPL : 64;   // sample intervals per candidate mask (one bit each)
  constexpr int CS = CH < MTG_EXTREMA_CS ? CH : MTG_EXTREMA_CS;  // sample intervals per unrolled scan step
  const double h = W ? (T - t0) / kExtremaSamples : T / kExtremaSamples;
  auto at = [&](int s) { return W ? t0 + s * h : s * h; };  // sample s < kExtremaSamples
  const int s0 = lane * SPL;
  double fa = horner<LF>(f, at(s0));
  // the end points t = t0 (lane 0) and t = T (lane L - 1), in one pass of the wave.
  // (An exact zero of f at t = t0 or t = T is the same candidate with a later order: never chosen.)
  if (lane == 0 || (lane == L - 1 && end_ord >= 0)) {
    const double te = lane == 0 ? (W ? t0 : 0.0) : T;
    const Ext e{te, mag(te), lane == 0 ? 0 : end_ord};
    lo = hi = e;
  }
  for (int ch = 0; ch < SPL / CH; ++ch) {  // (one mask for L >= 4)
    const int sc = s0 + ch * CH;  // this mask's samples sc + 1 .. sc + CH
    uint64_t pend = 0;
#pragma nounroll
    for (int q0 = 0; q0 < CH; q0 += CS) {
#pragma unroll
      for (int q = 0; q < CS; ++q) {
        const int s = sc + 1 + q0 + q;
        const double tb = s == kExtremaSamples ? T : at(s);
        const double fb = horner<LF>(f, tb);
        const bool hit = fb == 0.0 || (fa < 0.0 && fb > 0.0) || (fa > 0.0 && fb < 0.0);
        pend |= hit ? 1ull << (q0 + q) : 0ull;
        fa = fb;
      }
    }
    sink.begin(pend);
    // the candidates, lowest bit first, one per lane per round
    while (__builtin_amdgcn_ballot_w64(pend != 0) != 0) {
      if (pend != 0) {
        const int q = __builtin_ctzll(pend);
        pend &= pend - 1;
        const int s = sc + 1 + q;
        const double tb = s == kExtremaSamples ? T : at(s);
        const double tl = at(s - 1);
        const double fl = horner<LF>(f, tl), fb = horner<LF>(f, tb);
        double t;
        if constexpr (W) {  // tb - tl and tl + tb as the [0, T] scan forms them: (s - 1) h enters unrounded
          const double sh = (double)(s - 1);
          t = fb == 0.0 ? tb : refine_from<LF>(f, tl, tb, fl, fb, __builtin_fma(-sh, h, tb - t0), __builtin_fma(sh, h, t0 + tb));
        } else {
          t = fb == 0.0 ? tb : refine<LF>(f, tl, tb, fl, fb);
        }
        const Ext e{t, mag(t), 2 + s};
        if (better_max(e, hi)) hi = e;
        if (better_min(e, lo)) lo = e;
        sink.put(e.t, e.ord);
      }
    }
  }
}

// the scan on [0, T] with no sink: the trajectory kernels' call
template <int N, int L, class Mag>
__device__ __forceinline__ void extrema_scan(const double (&f)[2 * N - 2], double T, int lane, int end_ord, Mag mag,
                                             Ext& lo, Ext& hi) {
  ExtremaNoSink none;
  extrema_scan_on<N, L, false>(f, 0.0, T, lane, end_ord, mag, none, lo, hi);
}

// the group's extremes in every lane of the group (lanes of one group are consecutive lanes of one
// wave); ties go to the earlier candidate
template <int L>
__device__ __forceinline__ void extrema_group_reduce(Ext& lo, Ext& hi) {
#pragma unroll
  for (int m = L / 2; m >= 1; m >>= 1) {
    const Ext a = shfl_xor(lo, m, L), c = shfl_xor(hi, m, L);
    if (better_min(a, lo)) lo = a;
    if (better_max(c, hi)) hi = c;
  }
}

}  // namespace

}  // namespace mtg
