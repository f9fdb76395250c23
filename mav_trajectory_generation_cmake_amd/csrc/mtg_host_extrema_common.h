// mtg_host_extrema_common.h -- the host paths' search of one segment for the extremes of a
// derivative's magnitude, shared by mtg_host_extrema.cpp (Trajectory::computeMinMaxMagnitude, and the
// per-segment entries on a window with their candidate lists) and
// mtg_host_soft_constraint.cpp (PolynomialOptimization::computeMaximumOfMagnitude).  Same algorithm
// as the HIP kernels (mtg_extrema_common.h): the real roots in [0, T] of
// sum_d conv(p_d^(k), p_d^(k+1)) (one dimension: of p^(k+1)), isolated by sign changes on 256 uniform
// samples and refined by safeguarded Newton-bisection; the magnitude at each candidate; a candidate
// replaces the best so far only when it is strictly better, so the first one wins ties.
// Plain C++ (no HIP).
#pragma once

#include <cfloat>
#include <cmath>

namespace mtg {

constexpr int kHostExtremaSamples = 256;

struct HostExt {
  double t, v;
};

// The two candidate sets of the reference.
enum class SegmentCandidates {
  kBothEnds,   // t = 0, t = T, then the roots (Segment::computeMinMaxMagnitudeCandidates via
               // polynomial.cpp:38-39): Trajectory::computeMinMaxMagnitude
  kStartOnly,  // t = 0, then the roots; t = T is no candidate of the segment
               // (computeMaximumOfMagnitude, lin_impl:478-492: the caller adds the last segment's end)
};

inline double host_falling(int j, int n) {  // falling factorial j! / (j - n)!
  double f = 1.0;
  for (int q = 0; q < n; ++q) f *= (double)(j - q);
  return f;
}

inline double host_horner(const double* c, int len, double t) {
  double acc = 0.0;
  for (int j = len - 1; j >= 0; --j) acc = acc * t + c[j];
  return acc;
}

// magnitude of derivative k of the selected dimensions at t; cs [D][N]
inline double host_segment_magnitude(int N, int D, const double* cs, int k, unsigned dims, double t) {
  const int nd = N - k;
  double s = 0.0;
  for (int d = 0; d < D; ++d) {
    if (!((dims >> d) & 1u)) continue;
    double acc = 0.0;
    for (int j = nd - 1; j >= 0; --j) acc = acc * t + cs[d * N + j + k] * host_falling(j + k, k);
    s += acc * acc;
  }
  return std::sqrt(s);
}

// signed value of derivative k of dimension d at t (Polynomial::computeMinMax's quantity); cs [D][N]
inline double host_segment_axis_value(int N, const double* cs, int d, int k, double t) {
  double acc = 0.0;
  for (int j = N - k - 1; j >= 0; --j) acc = acc * t + cs[d * N + j + k] * host_falling(j + k, k);
  return acc;
}

// One segment on [t0, T] (W: a window with its own start; !W: t0 is not read and the search runs on
// [0, T], the arithmetic the trajectory entries have always had): cs [D][N], derivative k, dimensions
// dims.  f, q, q1: work arrays of 2N, N, N doubles; on return f holds the root polynomial and the
// result is its length.  value(t): the quantity whose extremes are sought; sink(t): called for every
// root found (an exact zero at t0 included), in ascending order.  lo / hi: the minimum and maximum
// over the candidates.
template <bool W, class Value, class Sink>
inline int host_segment_extrema_on(int N, int D, const double* cs, double t0, double T, int k, unsigned dims,
                                   SegmentCandidates candidates, double* f, double* q, double* q1, Value value,
                                   Sink sink, HostExt* lo_out, HostExt* hi_out) {
  const int nd = N - k, ndd = N - k - 1;
  const int ndim = __builtin_popcount(dims);
  for (int j = 0; j < 2 * N; ++j) f[j] = 0.0;
  int lf = 0;
  for (int d = 0; d < D; ++d) {
    if (!((dims >> d) & 1u)) continue;
    for (int j = 0; j < N; ++j) {
      q[j] = j < nd ? cs[d * N + j + k] * host_falling(j + k, k) : 0.0;
      q1[j] = j < ndd ? cs[d * N + j + k + 1] * host_falling(j + k + 1, k + 1) : 0.0;
    }
    if (ndim == 1) {  // one dimension: the roots of p^(k+1) (segment.cpp:124-130)
      for (int j = 0; j < ndd; ++j) f[j] = q1[j];
      lf = ndd;
    } else {  // convolve(d, dd) summed over the dimensions
      for (int a = 0; a < nd; ++a)
        for (int c = 0; c < ndd; ++c) f[a + c] += q[a] * q1[c];
      lf = nd + ndd - 1;
    }
  }
  HostExt lo{0.0, DBL_MAX}, hi{0.0, -DBL_MAX};
  auto consider = [&](double t) {
    const double v = value(t);
    if (v > hi.v) hi = HostExt{t, v};
    if (v < lo.v) lo = HostExt{t, v};
  };
  const double ts = W ? t0 : 0.0;
  consider(ts);  // the end point(s) first, then the roots in order
  if (candidates == SegmentCandidates::kBothEnds) consider(T);
  const double h = W ? (T - t0) / kHostExtremaSamples : T / kHostExtremaSamples;
  double ta = ts, fa = host_horner(f, lf, ts);
  if (fa == 0.0) {
    sink(ts);
    consider(ts);
  }
  for (int s = 1; s <= kHostExtremaSamples; ++s) {
    const double tb = s == kHostExtremaSamples ? T : (W ? t0 + s * h : s * h);
    const double fb = host_horner(f, lf, tb);
    if (fb == 0.0) {
      sink(tb);
      consider(tb);
    } else if ((fa < 0.0 && fb > 0.0) || (fa > 0.0 && fb < 0.0)) {
      double a0 = ta, b0 = tb, fa0 = fa, x = ta - fa * ((tb - ta) / (fb - fa));  // from the secant point
      if (!(x > ta && x < tb)) x = 0.5 * (ta + tb);
      for (int it = 0; it < 60; ++it) {
        double fx = 0.0, dfx = 0.0, ga = 0.0;  // f and f' in one Horner pass; ga: f(x)'s error scale
        const double ax = std::fabs(x);
        for (int j = lf - 1; j >= 0; --j) {
          dfx = dfx * x + fx;
          fx = fx * x + f[j];
          ga = ga * ax + std::fabs(f[j]);
        }
        if (std::fabs(fx) <= (2.0 * (2 * N - 2) * DBL_EPSILON) * ga) break;  // within rounding of 0
        if ((fx < 0.0) == (fa0 < 0.0)) a0 = x, fa0 = fx;
        else b0 = x;
        double xn = x - fx / dfx;
        if (!(xn > a0 && xn < b0)) xn = 0.5 * (a0 + b0);
        if (b0 - a0 <= 4.0 * DBL_EPSILON * std::fmax(std::fabs(a0), std::fabs(b0)) || xn == x) {
          x = xn;
          break;
        }
        x = xn;
      }
      sink(x);
      consider(x);
    }
    ta = tb;
    fa = fb;
  }
  *lo_out = lo;
  *hi_out = hi;
  return lf;
}

// The trajectory entries' search: [0, T], the magnitude, no candidate list.
inline void host_segment_extrema(int N, int D, const double* cs, double T, int k, unsigned dims,
                                 SegmentCandidates candidates, double* f, double* q, double* q1, HostExt* lo_out,
                                 HostExt* hi_out) {
  host_segment_extrema_on<false>(
      N, D, cs, 0.0, T, k, dims, candidates, f, q, q1,
      [&](double t) { return host_segment_magnitude(N, D, cs, k, dims, t); }, [](double) {}, lo_out, hi_out);
}

}  // namespace mtg
