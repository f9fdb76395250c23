// mtg_collision_common.h -- the per-position part of the collision term, shared by the HIP kernel
// (mtg_collision.hip) and the host path (mtg_host_collision.cpp): the map lookup that stands for the
// reference's esdf / sdf_tools calls, getDistanceSDF with lerp / triLerp (nl_impl:1846-1904,
// :2436-2464), getCostPotential (:2319-2343) and getCostAndGradientPotentialESDF (:1713-1806).
// Plain C++; every function is a literal restatement, operation order included.
#pragma once

#include <stdint.h>

#include "mtg.h"

#if defined(__HIPCC__)
#define MTG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MTG_HD inline
#endif

namespace mtg {

// A segment with more clock samples than this (T / dt) is reported as MTG_TRAJ_BAD_TIME: the clock
// t += dt must advance (dt above half an ulp of T), and a single wave must finish.
constexpr double kCollisionMaxSegmentSamples = 16777216.0;  // 2^24

// ---- the segment-time perturbation of getCostAndGradientTime (nl_impl:2180-2223), shared by
// mtg_collision_time.hip and mtg_host_collision_time.cpp
constexpr double kCollisionTimeClamp = 0.1;  // the reference's literal: T_n <= 0.1 gives 0.1 on both sides

// the perturbed time of segment n: side 0 = smaller (evaluated first), 1 = bigger
MTG_HD double collision_time_perturbed(double T, double inc, int side) {
  if (T <= kCollisionTimeClamp) return kCollisionTimeClamp;
  return side ? T + inc : T - inc;
}

// MTG_TRAJ_BAD_TIME of the time gradient: T not positive and finite, or a perturbed time of this
// segment (T + inc, or the clamp value) with more than kCollisionMaxSegmentSamples clock samples
MTG_HD bool collision_time_bad(double T, double inc, double dt) {
  if (!(T > 0.0 && T <= 1.7976931348623157e308)) return true;
  if (!((T + inc) / dt <= kCollisionMaxSegmentSamples)) return true;
  return T <= kCollisionTimeClamp && !(kCollisionTimeClamp / dt <= kCollisionMaxSegmentSamples);
}

struct CollisionMap {  // mtg_sdf_grid by value
  const float* distance;
  int nx, ny, nz;
  double origin[3];
  double resolution;
  double oob;
};

struct CollisionPot {  // the mtg_collision_params fields the potential reads
  double increment;    // map_resolution: bounds margin and finite-difference step
  double epsilon, robot_radius, multiplier;
  double lo[3], hi[3];
  int continuous;
};

// Cell of p: floor((p - origin) / resolution) per axis; false (indices 0) when outside the grid
// or not a number.
MTG_HD bool collision_cell(const CollisionMap& m, const double (&p)[3], int (&c)[3]) {
  const double fx = __builtin_floor((p[0] - m.origin[0]) / m.resolution);
  const double fy = __builtin_floor((p[1] - m.origin[1]) / m.resolution);
  const double fz = __builtin_floor((p[2] - m.origin[2]) / m.resolution);
  const bool in = fx >= 0.0 && fx < (double)m.nx && fy >= 0.0 && fy < (double)m.ny && fz >= 0.0 && fz < (double)m.nz;
  c[0] = in ? (int)fx : 0;
  c[1] = in ? (int)fy : 0;
  c[2] = in ? (int)fz : 0;
  return in;
}

MTG_HD double collision_map_at(const CollisionMap& m, int ix, int iy, int iz) {
  return (double)m.distance[((int64_t)ix * m.ny + iy) * m.nz + iz];
}

// lerp (nl_impl:2436-2439) with its two weights formed once per axis: the same quotients the
// reference forms in each of its calls
MTG_HD void collision_lerp_weights(double x, double x1, double x2, double& w0, double& w1) {
  w0 = (x2 - x) / (x2 - x1);
  w1 = (x - x1) / (x2 - x1);
}

// Distance at p: the nearest-cell value (getDistanceInMetricUnits / Get), or with `continuous`
// getDistanceSDF's stencil over the eight cells at index +-1 around the cell of p, falling back to
// the nearest cell when a corner is outside the grid (nl_impl:1861-1876).
MTG_HD double collision_distance(const CollisionMap& m, const double (&p)[3], bool continuous) {
  int c[3];
  if (!collision_cell(m, p, c)) return m.oob;
  const bool corners = c[0] >= 1 && c[0] <= m.nx - 2 && c[1] >= 1 && c[1] <= m.ny - 2 && c[2] >= 1 && c[2] <= m.nz - 2;
  if (!continuous || !corners) return collision_map_at(m, c[0], c[1], c[2]);
  double w0[3], w1[3];
  for (int k = 0; k < 3; ++k) {
    const double x1 = m.origin[k] + ((double)(c[k] - 1) + 0.5) * m.resolution;
    const double x2 = m.origin[k] + ((double)(c[k] + 1) + 0.5) * m.resolution;
    collision_lerp_weights(p[k], x1, x2, w0[k], w1[k]);
  }
  const double q000 = collision_map_at(m, c[0] - 1, c[1] - 1, c[2] - 1), q001 = collision_map_at(m, c[0] - 1, c[1] - 1, c[2] + 1);
  const double q010 = collision_map_at(m, c[0] - 1, c[1] + 1, c[2] - 1), q011 = collision_map_at(m, c[0] - 1, c[1] + 1, c[2] + 1);
  const double q100 = collision_map_at(m, c[0] + 1, c[1] - 1, c[2] - 1), q101 = collision_map_at(m, c[0] + 1, c[1] - 1, c[2] + 1);
  const double q110 = collision_map_at(m, c[0] + 1, c[1] + 1, c[2] - 1), q111 = collision_map_at(m, c[0] + 1, c[1] + 1, c[2] + 1);
  // triLerp (nl_impl:2451-2464), its pairing kept as written: the y step joins x00 with x01 and
  // x10 with x11
  const double x00 = w0[0] * q000 + w1[0] * q100;
  const double x10 = w0[0] * q010 + w1[0] * q110;
  const double x01 = w0[0] * q001 + w1[0] * q101;
  const double x11 = w0[0] * q011 + w1[0] * q111;
  const double r0 = w0[1] * x00 + w1[1] * x01;
  const double r1 = w0[1] * x10 + w1[1] * x11;
  return w0[2] * r0 + w1[2] * r1;
}

// getCostPotential (nl_impl:2319-2343)
MTG_HD double collision_potential(const CollisionPot& q, double distance, bool& is_collision) {
  is_collision = false;
  const double d = distance - q.robot_radius;
  if (d <= 0.0) {
    is_collision = true;
    return q.multiplier * (-d) + 0.5 * q.epsilon;
  }
  if (d <= q.epsilon) {
    const double e = d - q.epsilon;
    return 0.5 * 1.0 / q.epsilon * e * e;
  }
  return 0.0;
}

// getCostAndGradientPotentialESDF (nl_impl:1713-1806): the potential at p and, with grad, its
// central differences over +-increment per axis; the distance rule of all seven lookups is decided
// by the bounds test of the unshifted p.
MTG_HD double collision_potential_at(const CollisionMap& m, const CollisionPot& q, const double (&p)[3], bool want_grad,
                                     double (&grad)[3], bool& is_collision) {
  const double inc = q.increment;
  const bool valid = !(p[0] < q.lo[0] + inc || p[0] > q.hi[0] - inc || p[1] < q.lo[1] + inc || p[1] > q.hi[1] - inc ||
                       p[2] < q.lo[2] + inc || p[2] > q.hi[2] - inc);
  const bool continuous = valid && q.continuous;
  const double c = collision_potential(q, collision_distance(m, p, continuous), is_collision);
  if (want_grad) {
    for (int k = 0; k < 3; ++k) {
      double pl[3] = {p[0], p[1], p[2]}, pr[3] = {p[0], p[1], p[2]};
      pl[k] = p[k] - inc;
      pr[k] = p[k] + inc;
      bool cl, cr;
      const double left = collision_potential(q, collision_distance(m, pl, continuous), cl);
      const double right = collision_potential(q, collision_distance(m, pr, continuous), cr);
      grad[k] = (right - left) / (2.0 * inc);
    }
  }
  return c;
}

#if !defined(__HIPCC__)
// mtg_host_collision_cost_batch (mtg_host_collision.cpp) with the coefficients formed at coeff_times
// [B][K] while the loop reads `times`: the stale L_ of objectiveFunctionTime (mtg.h,
// mtg_objective_time_batch).  Cost only.  coeff_times == nullptr is the exported function; an entry
// that is not positive and finite gives MTG_TRAJ_BAD_TIME.
int host_collision_cost_coeff_times(int N, int D, int K, int64_t batch, const double* vertex_values,
                                    const double* times, const double* coeff_times, const mtg_sdf_grid* grid,
                                    const mtg_collision_params* params, double* cost_out, uint8_t* collision_out,
                                    int32_t* n_evaluated_out, int32_t* status, int threads);
#endif

}  // namespace mtg
