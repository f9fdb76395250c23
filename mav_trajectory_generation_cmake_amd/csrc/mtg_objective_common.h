// mtg_objective_common.h -- the parts of mtg_objective_batch that the HIP kernels (mtg_objective.hip)
// and the host path (mtg_host_objective.cpp) share: where a free derivative sits in the optimiser's
// vector, and the weighting / raise / state rules of the reference's objective functions
// (nl_impl:909-1449), restated in the order include/mtg.h writes them.  Plain C++.  Every product
// and sum must round on its own: the host build has -ffp-contract=off, the device functions carry
// the pragma (hipcc contracts a * b + c into an FMA by default).
#pragma once

#include <stdint.h>

#include "mtg.h"

#if defined(__HIPCC__)
#define MTG_OBJ_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MTG_OBJ_HD inline
#endif

namespace mtg {

// free derivatives (below h) of a trajectory: bit 7 and bits >= h of the mask are ignored
MTG_OBJ_HD int objective_n_free(const uint8_t* mask, int V, int h) {
  const unsigned hm = (1u << h) - 1u;
  int n = 0;
  for (int v = 0; v < V; ++v) n += __builtin_popcount(~(unsigned)mask[v] & hm);
  return n;
}

// index of the free slot (v, k) among the free slots in (vertex, derivative) order
MTG_OBJ_HD int objective_free_index(const uint8_t* mask, int v, int k, int h) {
  const unsigned hm = (1u << h) - 1u;
  int n = 0;
  for (int u = 0; u < v; ++u) n += __builtin_popcount(~(unsigned)mask[u] & hm);
  return n + __builtin_popcount(~(unsigned)mask[v] & ((1u << k) - 1u));
}

// the weights and switches of mtg_objective_params the combination reads, by value
struct ObjectiveRule {
  int objective;
  double w_d, w_c, w_t, w_sc;
  int is_collision_safe, is_coll_raise_first_iter;
  double add_coll_raise;
};

MTG_OBJ_HD double objective_nan() { return __builtin_nan(""); }

// cost, weighted costs [4] and the new state of one trajectory (mtg.h, "Semantics"); `in` is the
// state before the call (all zero for state == NULL).
MTG_OBJ_HD double objective_combine_cost(const ObjectiveRule& p, double J_d, double J_c, double J_sc, double J_t,
                                         bool is_collision, const mtg_objective_state& in, mtg_objective_state* out,
                                         double* weighted) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  mtg_objective_state s = in;
  double cost, ct, cc = 0.0, ctime = 0.0, cs;
  if (p.objective == MTG_OBJECTIVE_FREE_CONSTRAINTS) {
    ct = J_d;
    cs = J_sc;
    cost = J_d + J_sc;
    s.n_iterations++;
    s.cost_trajectory = ct;
    s.cost_soft_constraints = cs;
  } else if (p.objective == MTG_OBJECTIVE_FREE_CONSTRAINTS_AND_COLLISION) {
    ct = p.w_d * J_d;
    cc = p.w_c * J_c;
    cs = p.w_sc * J_sc;
    cost = (ct + cc) + cs;
    s.n_iterations++;
    s.cost_trajectory = ct;
    s.cost_collision = cc;
    s.cost_soft_constraints = cs;
    if (!s.iter0_done) {
      s.total_cost_iter0 = cost;
      s.iter0_done = 1;
    }
  } else {
    ct = p.w_d * J_d;
    cc = p.w_c * J_c;
    cs = p.w_sc * J_sc;
    ctime = p.w_t * J_t;
    const double total = ((ct + cc) + ctime) + cs;
    if (p.is_collision_safe && is_collision) {
      if (p.is_coll_raise_first_iter) {
        if (total < in.total_cost_iter0) cc = (in.total_cost_iter0 - (total - cc)) + p.add_coll_raise;
      } else {
        const double last = ((in.cost_trajectory + in.cost_collision) + in.cost_time) + in.cost_soft_constraints;
        if (total < last) cc = (last - (total - cc)) + p.add_coll_raise;
      }
    }
    cost = ((ct + cc) + ctime) + cs;
    s.n_iterations++;
    s.cost_trajectory = ct;
    s.cost_collision = cc;
    s.cost_time = ctime;
    s.cost_soft_constraints = cs;
    if (!s.iter0_done) {
      s.total_cost_iter0 = cost;
      s.iter0_done = 1;
    }
  }
  weighted[0] = ct;
  weighted[1] = cc;
  weighted[2] = ctime;
  weighted[3] = cs;
  *out = s;
  return cost;
}

// one entry of the free-derivative gradient
MTG_OBJ_HD double objective_combine_grad(const ObjectiveRule& p, double g_d, double g_c, double g_sc) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (p.objective == MTG_OBJECTIVE_FREE_CONSTRAINTS) return g_d;
  return (p.w_d * g_d + p.w_c * g_c) + p.w_sc * g_sc;
}

// one entry of the time gradient (objective 2); the soft-constraint term is the reference's exact zero
MTG_OBJ_HD double objective_combine_grad_time(const ObjectiveRule& p, double dJd_dt, double dJc_dt) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return ((p.w_d * dJd_dt + p.w_c * dJc_dt) + p.w_sc * 0.0) + p.w_t;
}

// computeTotalTrajectoryTime: the sequential sum
MTG_OBJ_HD double objective_total_time(const double* T, int K) {
  double s = 0.0;
  for (int i = 0; i < K; ++i) s += T[i];
  return s;
}

// a segment time the reference would CHECK-fail on
MTG_OBJ_HD bool objective_time_bad(double T) { return !(T > 0.0 && T <= 1.7976931348623157e308); }

// the fields of mtg_objective_time_params the combination of mtg_objective_time_batch reads, by value
struct ObjectiveTimeRule {
  int objective;
  double time_penalty, w_c;
};

// cost, weighted costs [4] and the new state of one trajectory for objectiveFunctionTime (cost_traj: the
// solve's cost) and objectiveFunctionTimeAndConstraints (cost_traj: J_d, halved here), mtg.h
// "Semantics" of mtg_objective_time_batch; J_sc is 0 with the soft constraints off.
MTG_OBJ_HD double objective_time_combine_cost(const ObjectiveTimeRule& p, double cost_traj, double J_c, double J_sc,
                                              double J_t, const mtg_objective_state& in, mtg_objective_state* out,
                                              double* weighted) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  mtg_objective_state s = in;
  const double ctime = (J_t * J_t) * p.time_penalty;
  const double cs = J_sc;
  double cost, ct, cc = 0.0;
  if (p.objective == MTG_OBJECTIVE_TIME) {
    ct = cost_traj;
    if (p.w_c > 0.0) cc = p.w_c * J_c;
    cost = ((ct + cc) + ctime) + cs;
    s.n_iterations++;
    s.cost_trajectory = ct;
    s.cost_collision = cc;
    s.cost_time = ctime;
    s.cost_soft_constraints = cs;
    if (!s.iter0_done) {
      s.total_cost_iter0 = cost;
      s.iter0_done = 1;
    }
  } else {
    ct = 0.5 * cost_traj;
    cost = (ct + ctime) + cs;
    s.n_iterations++;
    s.cost_trajectory = ct;
    s.cost_time = ctime;
    s.cost_soft_constraints = cs;
  }
  weighted[0] = ct;
  weighted[1] = cc;
  weighted[2] = ctime;
  weighted[3] = cs;
  *out = s;
  return cost;
}

}  // namespace mtg
