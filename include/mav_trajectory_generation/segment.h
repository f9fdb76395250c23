// segment.h -- Segment: a time and one Polynomial per dimension (reference segment.h:37-131,
// src/segment.cpp:27-58).
//
// computeMinMaxMagnitudeCandidate{Times,s} / selectMinMaxMagnitudeFromCandidates are one segment of
// mtg_segment_min_max_magnitude_batch (host or GPU, ExecutionPolicy): the library's root search on
// the window, not Jenkins-Traub (src/rpoly.cpp, not ported).
#ifndef MAV_TRAJECTORY_GENERATION_SEGMENT_H_
#define MAV_TRAJECTORY_GENERATION_SEGMENT_H_

#include <cmath>
#include <cstdint>
#include <limits>
#include <ostream>
#include <vector>

#include "mav_trajectory_generation/extremum.h"
#include "mav_trajectory_generation/motion_defines.h"
#include "mav_trajectory_generation/polynomial.h"

namespace mav_trajectory_generation {

constexpr double kNumNSecPerSec = 1.0e9;
constexpr double kNumSecPerNsec = 1.0e-9;

class Segment {
 public:
  typedef std::vector<Segment> Vector;

  Segment(int N, int D) : time_(0.0), N_(N), D_(D) { polynomials_.resize(D_, Polynomial(N_)); }
  Segment(const Segment& segment) = default;
  Segment& operator=(const Segment& segment) = default;

  bool operator==(const Segment& rhs) const {  // src/segment.cpp:27-40
    if (D_ != rhs.D_ || time_ != rhs.time_) return false;
    for (int i = 0; i < D_; ++i)
      if (polynomials_[i] != rhs.polynomials_[i]) return false;
    return true;
  }
  bool operator!=(const Segment& rhs) const { return !operator==(rhs); }

  int D() const { return D_; }
  int N() const { return N_; }
  double getTime() const { return time_; }
  uint64_t getTimeNSec() const { return static_cast<uint64_t>(kNumNSecPerSec * time_); }
  void setTime(double time_sec) { time_ = time_sec; }
  void setTimeNSec(uint64_t time_ns) { time_ = time_ns * kNumSecPerNsec; }

  Polynomial& operator[](size_t idx) {
    if (idx >= (size_t)D_) fail(MTG_ERR_INVALID_ARGUMENT, "Segment: dimension index out of range");
    return polynomials_[idx];
  }
  const Polynomial& operator[](size_t idx) const {
    if (idx >= (size_t)D_) fail(MTG_ERR_INVALID_ARGUMENT, "Segment: dimension index out of range");
    return polynomials_[idx];
  }
  const Polynomial::Vector& getPolynomialsRef() const { return polynomials_; }

  // src/segment.cpp:51-58
  VectorXd evaluate(double t, int derivative_order = derivative_order::POSITION) const {
    VectorXd result(D_);
    for (int d = 0; d < D_; ++d) result[d] = polynomials_[d].evaluate(t, derivative_order);
    return result;
  }

  // Candidate times for the extremes of the derivative's magnitude over `dimensions` on
  // [t_start, t_end]: t_start, t_end, then the real roots in the window of
  // sum_d conv(p_d^(k), p_d^(k+1)) (one dimension: of p^(k+1)), ascending (src/segment.cpp:82-131).
  // One segment of mtg_segment_min_max_magnitude_batch: on the library's host path unless
  // ExecutionPolicy::kDevice, as Trajectory::computeMinMaxMagnitude.  false: no dimensions, a dimension
  // out of range, a derivative outside 0 .. N-2, t_start > t_end or a window that is not finite.
  // (The reference's function falls off its end without a return on success, segment.cpp:131, which
  // is undefined behaviour; its callers read true.  This one returns true.)
  bool computeMinMaxMagnitudeCandidateTimes(int derivative, double t_start, double t_end,
                                            const std::vector<int>& dimensions,
                                            std::vector<double>* candidate_times) const {
    check_notnull(candidate_times, "candidate_times");
    candidate_times->clear();
    if (dimensions.empty()) {
      warn("No dimensions specified.");
      return false;
    }
    uint32_t mask = 0;
    for (int d : dimensions) {
      if (d < 0 || d >= D_ || d >= 32) {
        warn("Specified dimensions are out of bounds.");
        return false;
      }
      mask |= 1u << d;
    }
    if (derivative < 0 || derivative > N_ - 2) {
      warn("derivative has to be in [0, N - 2].");
      return false;
    }
    std::vector<double> coeffs((size_t)D_ * N_);
    for (int d = 0; d < D_; ++d) {
      const VectorXd c = polynomials_[d].getCoefficients();
      for (int j = 0; j < N_; ++j) coeffs[(size_t)d * N_ + j] = c[j];
    }
    const double window[2] = {t_start, t_end};
    constexpr int kCap = 2 + 257;  // the ends, and at most one root per sample interval plus one at t_start
    double times[kCap];
    int32_t count = 0, status = 0;
    if (singleOnDevice()) {
      mtg_ctx* ctx = defaultContext();
      check(mtg_segment_min_max_magnitude_batch(ctx, N_, D_, 1, coeffs.data(), nullptr, window, derivative, mask, nullptr,
                                                nullptr, times, &count, kCap, &status, 0),
            ctx, "mtg_segment_min_max_magnitude_batch");
    } else {
      check(mtg_host_segment_min_max_magnitude_batch(N_, D_, 1, coeffs.data(), nullptr, window, derivative, mask, nullptr,
                                                     nullptr, times, &count, kCap, &status, 1),
            nullptr, "mtg_host_segment_min_max_magnitude_batch");
    }
    if (status != MTG_TRAJ_OK) {
      warn(t_start > t_end ? "t_start is greater than t_end." : "the window is not finite.");
      return false;
    }
    candidate_times->assign(times, times + (count < kCap ? count : kCap));
    return true;
  }

  // The candidate times with the magnitude at each, as Extremum(t, magnitude, 0)
  // (src/segment.cpp:133-156).  Like the reference, this returns true whatever the times' search
  // returned; the list is then empty.
  bool computeMinMaxMagnitudeCandidates(int derivative, double t_start, double t_end,
                                        const std::vector<int>& dimensions, std::vector<Extremum>* candidates) const {
    check_notnull(candidates, "candidates");
    std::vector<double> candidate_times;
    computeMinMaxMagnitudeCandidateTimes(derivative, t_start, t_end, dimensions, &candidate_times);
    candidates->resize(candidate_times.size());
    for (size_t i = 0; i < candidate_times.size(); ++i)
      (*candidates)[i] = Extremum(candidate_times[i], magnitudeAt(candidate_times[i], derivative, dimensions), 0);
    return true;
  }

  // Minimum and maximum among the candidates inside [t_start, t_end], then t_start and t_end
  // themselves (src/segment.cpp:158-197).  std::max / std::min keep their first argument on a tie,
  // so the earliest candidate wins.  false: t_start > t_end.
  bool selectMinMaxMagnitudeFromCandidates(double t_start, double t_end, int derivative,
                                           const std::vector<int>& dimensions,
                                           const std::vector<Extremum>& candidates, Extremum* minimum,
                                           Extremum* maximum) const {
    check_notnull(minimum, "minimum");
    check_notnull(maximum, "maximum");
    if (t_start > t_end) {
      warn("t_start is greater than t_end.");
      return false;
    }
    minimum->value = std::numeric_limits<double>::max();
    maximum->value = std::numeric_limits<double>::lowest();
    auto take = [&](const Extremum& c) {
      if (*maximum < c) *maximum = c;
      if (c < *minimum) *minimum = c;
    };
    for (const Extremum& c : candidates)
      if (!(c.time < t_start || c.time > t_end)) take(c);
    take(Extremum(t_start, magnitudeAt(t_start, derivative, dimensions), 0));
    take(Extremum(t_end, magnitudeAt(t_end, derivative, dimensions), 0));
    return true;
  }

 protected:
  // sqrt(sum_{d in dimensions} p_d^(derivative)(t)^2), summed in the order given
  double magnitudeAt(double t, int derivative, const std::vector<int>& dimensions) const {
    double s = 0.0;
    for (int d : dimensions) {
      const double v = (*this)[(size_t)d].evaluate(t, derivative);
      s += v * v;
    }
    return std::sqrt(s);
  }

  Polynomial::Vector polynomials_;
  double time_;

 private:
  int N_;
  int D_;
};

// printSegment (src/segment.cpp:60-80): time, then each dimension's coefficients.
inline void printSegment(std::ostream& stream, const Segment& s, int derivative) {
  stream << "t: " << s.getTime() << std::endl;
  stream << " coefficients for " << positionDerivativeToString(derivative) << ": " << std::endl;
  for (int i = 0; i < s.D(); ++i) {
    stream << "dim " << i << ": " << std::endl;
    const VectorXd c = s[i].getCoefficients(derivative);
    for (int j = 0; j < (int)c.size(); ++j) stream << (j ? " " : "") << c[j];
    stream << std::endl;
  }
}

inline std::ostream& operator<<(std::ostream& stream, const Segment& s) {
  printSegment(stream, s, derivative_order::POSITION);
  return stream;
}

inline std::ostream& operator<<(std::ostream& stream, const std::vector<Segment>& segments) {
  for (const Segment& s : segments) stream << s << std::endl;
  return stream;
}

}  // namespace mav_trajectory_generation

#endif  // MAV_TRAJECTORY_GENERATION_SEGMENT_H_
