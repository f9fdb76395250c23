// mtg_host_objective.cpp -- host (CPU) path of mtg_objective_batch: the reference's objective
// functions in the optimiser's variables (polynomial_optimization_nonlinear_impl.h:909-1449), composed
// of the library's host paths of the collision, soft-constraint and collision-time terms and a host
// evaluation of the derivative term (getCostAndGradientDerivative :1452-1520 and the J_d part of
// getCostAndGradientTime :2155-2243); the weighting, raise and state rules are
// mtg_objective_common.h, shared with the kernels.  Also mtg_host_objective_bounds_batch
// (setFreeEndpointDerivativeHardConstraints :2518-2564, the time bounds and initial step :646-692).
// And mtg_host_objective_time_batch, the two gradient-free objectives in the segment times
// (objectiveFunctionTime :765-832, objectiveFunctionTimeAndConstraints :835-906) composed of the host
// solve, the host soft-constraint path, the host collision loop with coefficient times and the same
// derivative term, with mtg_host_objective_time_bounds_batch (:248-276, :551-562).
// Plain C++ (no HIP).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
#include <thread>
#include <vector>

#include "mtg.h"
#include "mtg_collision_common.h"
#include "mtg_host_threads.h"
#include "mtg_objective_common.h"

namespace {

// sum over dimensions and segments of e^T H(T_i) e, e = [x_i; x_{i+1}], with H from
// mtg_host_segment_matrices; for r >= 1 the positions are taken relative to x_i[0] first (H annihilates
// a common position offset, as in mtg_cost.hip).  Rd (nullable) [V][h][D] receives R d.
double derivative_cost(int N, int D, int K, int r, const double* vv, const double* T, double* Rd) {
  const int h = N / 2;
  double Hm[12 * 12], e[12], y[12];
  if (Rd)
    for (int i = 0; i < (K + 1) * h * D; ++i) Rd[i] = 0.0;
  double J = 0.0;
  for (int i = 0; i < K; ++i) {
    if (mtg_host_segment_matrices(N, r, T[i], nullptr, nullptr, nullptr, Hm) != MTG_OK)
      return std::numeric_limits<double>::quiet_NaN();
    for (int d = 0; d < D; ++d) {
      for (int q = 0; q < h; ++q) {
        e[q] = vv[((size_t)i * h + q) * D + d];
        e[h + q] = vv[((size_t)(i + 1) * h + q) * D + d];
      }
      if (r >= 1) {
        e[h] -= e[0];
        e[0] = 0.0;
      }
      double seg = 0.0;
      for (int a = 0; a < N; ++a) {
        double s = 0.0;
        for (int b = 0; b < N; ++b) s += Hm[a * N + b] * e[b];
        y[a] = s;
        seg += e[a] * s;
      }
      J += seg;
      if (Rd)
        for (int q = 0; q < h; ++q) {
          Rd[((size_t)i * h + q) * D + d] += y[q];
          Rd[((size_t)(i + 1) * h + q) * D + d] += y[h + q];
        }
    }
  }
  return J;
}

struct Work {
  std::vector<double> Rd, tp;
};

// J_d, grad_d [D][V*h] (nullable; the free entries, the rest untouched) and dJd_dt [K] (nullable) of
// one trajectory
void derivative_term(int N, int D, int K, int r, const double* vv, const uint8_t* mask, const double* T, double inc,
                     double* J_d, double* grad_d, double* dJd_dt, Work& w) {
  const int h = N / 2, V = K + 1;
  w.Rd.resize((size_t)V * h * D);
  *J_d = derivative_cost(N, D, K, r, vv, T, grad_d ? w.Rd.data() : nullptr);
  if (grad_d) {
    for (int d = 0; d < D; ++d) {
      int idx = 0;
      for (int v = 0; v < V; ++v)
        for (int q = 0; q < h; ++q)
          if (!((mask[v] >> q) & 1u)) grad_d[(size_t)d * V * h + idx++] = 2.0 * w.Rd[((size_t)v * h + q) * D + d];
    }
  }
  if (dJd_dt) {  // the reference's central difference: two full costs per segment, the smaller side first
    w.tp.assign(T, T + K);
    for (int n = 0; n < K; ++n) {
      if (T[n] <= 0.1) {
        dJd_dt[n] = 0.0;  // both perturbed times are 0.1 (nl_impl:2182, :2201)
      } else if (!(T[n] - inc > 0.0)) {
        dJd_dt[n] = std::numeric_limits<double>::quiet_NaN();  // the reference CHECK-fails
      } else {
        w.tp[n] = T[n] - inc;
        const double Jm = derivative_cost(N, D, K, r, vv, w.tp.data(), nullptr);
        w.tp[n] = T[n] + inc;
        const double Jp = derivative_cost(N, D, K, r, vv, w.tp.data(), nullptr);
        w.tp[n] = T[n];
        dJd_dt[n] = (Jp - Jm) / (2.0 * inc);
      }
    }
  }
}

}  // namespace

extern "C" int mtg_host_objective_batch(int N, int D, int K, int64_t batch, const double* values,
                                        const uint8_t* fixed_mask, const double* times, const double* x,
                                        int64_t x_stride, const mtg_objective_params* params, const mtg_sdf_grid* grid,
                                        const mtg_collision_params* collision, const mtg_soft_constraint_params* soft,
                                        double* cost_out, double* grad_out, double* weighted_costs_out,
                                        uint8_t* collision_out, mtg_objective_state* state,
                                        const mtg_objective_parts* parts, int32_t* status, int threads) {
  if (!params) return MTG_ERR_INVALID_ARGUMENT;
  const int obj = params->objective;
  if (obj < MTG_OBJECTIVE_FREE_CONSTRAINTS || obj > MTG_OBJECTIVE_FREE_CONSTRAINTS_AND_COLLISION_AND_TIME)
    return MTG_ERR_INVALID_ARGUMENT;
  if (params->reserved != 0) return MTG_ERR_INVALID_ARGUMENT;
  const bool with_coll = obj != MTG_OBJECTIVE_FREE_CONSTRAINTS;
  const bool with_time = obj == MTG_OBJECTIVE_FREE_CONSTRAINTS_AND_COLLISION_AND_TIME;
  const bool with_soft = params->use_soft_constraints != 0;
  const bool with_grad = grad_out != nullptr;
  const int r = params->derivative_to_optimize;
  if (N < 2 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  const int h = N / 2, V = K + 1;
  if (r < 0 || r > h - 1) return MTG_ERR_BAD_DERIVATIVE;
  if (K < 1 || D < 1 || batch < 0) return MTG_ERR_SIZE_MISMATCH;
  if (with_coll) {
    if (N < 6) return MTG_ERR_UNSUPPORTED_N;
    if (D != 3 || !grid || !collision) return MTG_ERR_INVALID_ARGUMENT;
    if (with_time && !(params->increment_time > 0.0 && params->increment_time <= DBL_MAX)) return MTG_ERR_INVALID_ARGUMENT;
  } else if (D > 4) {
    return MTG_ERR_INVALID_ARGUMENT;
  }
  if (with_soft != (soft != nullptr)) return MTG_ERR_INVALID_ARGUMENT;
  if (x_stride < 0) return MTG_ERR_INVALID_ARGUMENT;
  if (batch == 0) return MTG_OK;
  if (!values || !fixed_mask || !cost_out || !x || (!with_time && !times)) return MTG_ERR_INVALID_ARGUMENT;
  const int nt = with_time ? K : 0;
  const size_t nB = (size_t)batch, per = (size_t)V * h * D, gper = (size_t)D * V * h;
  std::vector<int32_t> n_free(nB);
  for (int64_t b = 0; b < batch; ++b) {
    n_free[b] = mtg::objective_n_free(fixed_mask + b * V, V, h);
    if (x_stride < nt + (int64_t)D * n_free[b]) return MTG_ERR_INVALID_ARGUMENT;
  }

  // ---- unpack: setFreeConstraints and the times
  std::vector<double> vv(nB * per), T(nB * K);
  std::vector<int32_t> st(nB, 0), st_c(nB, 0), st_s(nB, 0), st_t(nB, 0);
  for (int64_t b = 0; b < batch; ++b) {
    const uint8_t* mask = fixed_mask + b * V;
    const double* xr = x + b * x_stride;
    for (int v = 0; v < V; ++v)
      for (int k = 0; k < h; ++k)
        for (int d = 0; d < D; ++d) {
          const size_t e = ((size_t)v * h + k) * D + d;
          vv[b * per + e] = ((mask[v] >> k) & 1u) ? values[b * per + e]
                                                  : xr[nt + (int64_t)d * n_free[b] + mtg::objective_free_index(mask, v, k, h)];
        }
    for (int i = 0; i < K; ++i) {
      T[b * K + i] = with_time ? xr[i] : times[b * K + i];
      if (mtg::objective_time_bad(T[b * K + i])) st[b] |= MTG_TRAJ_BAD_TIME;
    }
  }

  // ---- the parts
  std::vector<double> J_d(nB), J_c(nB, 0.0), J_sc(nB, 0.0), g_d(with_grad ? nB * gper : 0, 0.0),
      g_c(with_grad && with_coll ? nB * gper : 0, 0.0), g_sc(with_grad && with_coll && with_soft ? nB * gper : 0, 0.0),
      jd(with_grad && with_time ? nB * K : 0), jc(with_grad && with_time ? nB * K : 0);
  std::vector<uint8_t> coll(nB, 0);
  int rc = MTG_OK;
  if (with_coll)
    rc = mtg_host_collision_cost_batch(N, D, K, batch, vv.data(), fixed_mask, T.data(), grid, collision, J_c.data(),
                                       with_grad ? g_c.data() : nullptr, coll.data(), nullptr, st_c.data(), threads);
  if (rc == MTG_OK && with_soft)
    rc = mtg_host_soft_constraint_cost_batch(N, D, K, batch, vv.data(), fixed_mask, T.data(), soft, J_sc.data(),
                                             with_grad && with_coll ? g_sc.data() : nullptr, nullptr, st_s.data(), threads);
  if (rc == MTG_OK && with_time && with_grad)
    rc = mtg_host_collision_time_gradient_batch(N, D, K, batch, vv.data(), T.data(), grid, collision,
                                                params->increment_time, jc.data(), nullptr, nullptr, st_t.data(), threads);
  if (rc != MTG_OK) return rc;
  mtg::run_threads(batch, threads, [&](int64_t b0, int64_t b1) {
    Work w;
    for (int64_t b = b0; b < b1; ++b) {
      if (st[b] & MTG_TRAJ_BAD_TIME) {
        J_d[b] = std::numeric_limits<double>::quiet_NaN();
        if (with_grad && with_time)
          for (int i = 0; i < K; ++i) jd[b * K + i] = std::numeric_limits<double>::quiet_NaN();
        continue;
      }
      derivative_term(N, D, K, r, vv.data() + b * per, fixed_mask + b * V, T.data() + b * K, params->increment_time,
                      &J_d[b], with_grad ? g_d.data() + b * gper : nullptr,
                      with_grad && with_time ? jd.data() + b * K : nullptr, w);
    }
  });

  // ---- combine (the rules of mtg_objective_common.h, as the combine kernel applies them)
  const mtg::ObjectiveRule rule{obj, params->w_d, params->w_c, params->w_t, params->w_sc, params->is_collision_safe,
                                params->is_coll_raise_first_iter, params->add_coll_raise};
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> J_t(nB, 0.0);
  for (int64_t b = 0; b < batch; ++b) {
    const int stb = st[b] | st_c[b] | st_s[b] | st_t[b];
    const bool err = (stb & MTG_TRAJ_ERROR_MASK) != 0;
    const int nf = n_free[b];
    if (status) status[b] = stb;
    if (with_time) J_t[b] = mtg::objective_total_time(T.data() + b * K, K);
    if (with_grad) {
      double* g = grad_out + b * x_stride;
      for (int64_t j = 0; j < x_stride; ++j) {
        double val = 0.0;
        if (j < nt + (int64_t)D * nf) {
          if (err) {
            val = nan;
          } else if (j < nt) {
            val = mtg::objective_combine_grad_time(rule, jd[b * K + j], jc[b * K + j]);
          } else {
            const int jj = (int)(j - nt), d = jj / nf, i = jj - d * nf;
            const size_t o = b * gper + (size_t)d * V * h + i;
            val = mtg::objective_combine_grad(rule, g_d[o], with_coll ? g_c[o] : 0.0, with_coll && with_soft ? g_sc[o] : 0.0);
          }
        }
        g[j] = val;
      }
    }
    if (err) {
      cost_out[b] = nan;
      if (weighted_costs_out)
        for (int q = 0; q < 4; ++q) weighted_costs_out[4 * b + q] = nan;
      if (collision_out) collision_out[b] = 0;
      continue;
    }
    mtg_objective_state in = {};
    if (state) in = state[b];
    mtg_objective_state out;
    double w4[4];
    cost_out[b] = mtg::objective_combine_cost(rule, J_d[b], J_c[b], J_sc[b], J_t[b], coll[b] != 0, in, &out, w4);
    if (weighted_costs_out)
      for (int q = 0; q < 4; ++q) weighted_costs_out[4 * b + q] = w4[q];
    if (collision_out) collision_out[b] = coll[b] ? 1 : 0;
    if (state) state[b] = out;
  }
  if (parts) {
    auto put = [](double* dst, const std::vector<double>& src, bool have) {
      if (dst && have && !src.empty()) std::copy(src.begin(), src.end(), dst);
    };
    put(parts->J_d, J_d, true);
    put(parts->J_c, J_c, with_coll);
    put(parts->J_sc, J_sc, with_soft);
    put(parts->J_t, J_t, true);
    put(parts->dJd_dt, jd, true);
    put(parts->dJc_dt, jc, true);
    put(parts->grad_d, g_d, true);
    put(parts->grad_c, g_c, true);
    put(parts->grad_sc, g_sc, true);
  }
  return MTG_OK;
}

extern "C" int mtg_host_objective_bounds_batch(int N, int D, int K, int64_t batch, const uint8_t* fixed_mask,
                                               int with_times, const double* x, int64_t x_stride,
                                               int derivative_to_optimize, int solve_with_position_constraint,
                                               const mtg_soft_constraint_params* constraints, const double* min_bound,
                                               const double* max_bound, double initial_stepsize_rel, double* lower,
                                               double* upper, double* initial_step) {
  if (N < 2 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  const int h = N / 2, V = K + 1, r = derivative_to_optimize;
  if (r < 0 || r > h - 1) return MTG_ERR_BAD_DERIVATIVE;
  if (K < 1 || D < 1 || batch < 0) return MTG_ERR_SIZE_MISMATCH;
  if (x_stride < 0 || (constraints && (constraints->n_constraints < 0 || constraints->n_constraints > 8)))
    return MTG_ERR_INVALID_ARGUMENT;
  if (batch == 0) return MTG_OK;
  if (!fixed_mask || (initial_step && !x) || (!solve_with_position_constraint && (!min_bound || !max_bound)))
    return MTG_ERR_INVALID_ARGUMENT;
  const int nt = with_times ? K : 0;
  const int C = constraints ? constraints->n_constraints : 0;
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> lo, up;
  for (int64_t b = 0; b < batch; ++b) {
    const size_t nf = (size_t)mtg::objective_n_free(fixed_mask + b * V, V, h);
    const size_t n_all = (size_t)D * nf;
    if ((int64_t)(nt + n_all) > x_stride) return MTG_ERR_INVALID_ARGUMENT;
    lo.assign(n_all, -inf);
    up.assign(n_all, inf);
    // setFreeEndpointDerivativeHardConstraints, index arithmetic as written (unsigned int)
    for (int k = 0; k < D; ++k) {
      for (int n = 0; n < K - 1; ++n) {
        unsigned int start_idx = 0;
        if (solve_with_position_constraint) {
          start_idx = (unsigned int)(k * nf + (size_t)n * r);
        } else {
          start_idx = (unsigned int)(k * nf + (size_t)n * (r + 1));
          if (start_idx >= n_all) return MTG_ERR_INVALID_ARGUMENT;  // .at() throws
          lo[start_idx] = min_bound[k];
          up[start_idx] = max_bound[k];
        }
        for (int c = 0; c < C; ++c) {
          unsigned int deriv_idx = 0;
          if (solve_with_position_constraint) {
            deriv_idx = (unsigned int)constraints->derivative[c] - 1u;
          } else {
            deriv_idx = (unsigned int)constraints->derivative[c];
          }
          const unsigned int idx = start_idx + deriv_idx;
          if (idx >= n_all) return MTG_ERR_INVALID_ARGUMENT;  // .at() throws
          lo[idx] = -std::abs(constraints->limit[c]);
          up[idx] = std::abs(constraints->limit[c]);
        }
      }
    }
    for (int64_t j = 0; j < x_stride; ++j) {
      const bool in_row = j < (int64_t)(nt + n_all);
      if (lower) lower[b * x_stride + j] = !in_row ? 0.0 : j < nt ? 0.1 : lo[j - nt];
      if (upper) upper[b * x_stride + j] = !in_row ? 0.0 : j < nt ? inf : up[j - nt];
      if (initial_step) initial_step[b * x_stride + j] = in_row ? initial_stepsize_rel * std::abs(x[b * x_stride + j]) : 0.0;
    }
  }
  return MTG_OK;
}

// ---- mtg_objective_time_batch on the host: objectiveFunctionTime (nl_impl:765-832) and
// objectiveFunctionTimeAndConstraints (:835-906), in the launch order of the device call.
extern "C" int mtg_host_objective_time_batch(int N, int D, int K, int64_t batch, const double* values,
                                             const uint8_t* fixed_mask, const double* x, int64_t x_stride,
                                             const mtg_objective_time_params* params, const double* coeff_times,
                                             const mtg_sdf_grid* grid, const mtg_collision_params* collision,
                                             const mtg_soft_constraint_params* constraints, double* cost_out,
                                             double* weighted_costs_out, uint8_t* collision_out,
                                             double* constraint_values_out, mtg_extremum* maxima_out, double* free_out,
                                             double* coeffs_out, mtg_objective_state* state,
                                             const mtg_objective_parts* parts, int32_t* status, int threads) {
  if (!params) return MTG_ERR_INVALID_ARGUMENT;
  const int obj = params->objective;
  if (obj != MTG_OBJECTIVE_TIME && obj != MTG_OBJECTIVE_TIME_AND_CONSTRAINTS) return MTG_ERR_INVALID_ARGUMENT;
  if (params->reserved != 0) return MTG_ERR_INVALID_ARGUMENT;
  const bool solve = obj == MTG_OBJECTIVE_TIME;
  const bool with_coll = solve && params->w_c > 0.0;
  const bool with_soft = params->use_soft_constraints != 0;
  const bool with_max = with_soft || constraint_values_out || maxima_out;
  const int r = params->derivative_to_optimize;
  if (N < 2 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  const int h = N / 2, V = K + 1;
  if (r < 0 || r > h - 1) return MTG_ERR_BAD_DERIVATIVE;
  if (K < 1 || D < 1 || batch < 0) return MTG_ERR_SIZE_MISMATCH;
  if (with_coll) {
    if (N < 6) return MTG_ERR_UNSUPPORTED_N;
    if (D != 3 || !grid || !collision || !coeff_times) return MTG_ERR_INVALID_ARGUMENT;
  } else if (D > 4 || grid || collision || coeff_times) {
    return MTG_ERR_INVALID_ARGUMENT;
  }
  if (with_max && (!constraints || N < 6)) return MTG_ERR_INVALID_ARGUMENT;
  if (parts && (parts->dJd_dt || parts->dJc_dt || parts->grad_d || parts->grad_c || parts->grad_sc))
    return MTG_ERR_INVALID_ARGUMENT;
  if (x_stride < 0) return MTG_ERR_INVALID_ARGUMENT;
  if (batch == 0) return MTG_OK;
  if (!values || !fixed_mask || !cost_out || !x) return MTG_ERR_INVALID_ARGUMENT;
  const size_t nB = (size_t)batch, per = (size_t)V * h * D, gper = (size_t)D * V * h, cper = (size_t)K * D * N;
  std::vector<int32_t> n_free(nB);
  for (int64_t b = 0; b < batch; ++b) {
    n_free[b] = mtg::objective_n_free(fixed_mask + b * V, V, h);
    if (x_stride < K + (solve ? 0 : (int64_t)D * n_free[b])) return MTG_ERR_INVALID_ARGUMENT;
  }
  const int C = with_max ? constraints->n_constraints : 0;

  // ---- the times, and the trajectory at x
  std::vector<double> T(nB * K), vv(nB * per), ct(nB), fr(solve ? nB * gper : 0), co((solve || coeffs_out) ? nB * cper : 0);
  std::vector<int32_t> st(nB, 0), st_v(nB, 0), st_c(nB, 0), st_s(nB, 0);
  for (int64_t b = 0; b < batch; ++b)
    for (int i = 0; i < K; ++i) {
      T[b * K + i] = x[b * x_stride + i];
      if (mtg::objective_time_bad(T[b * K + i])) st[b] |= MTG_TRAJ_BAD_TIME;
    }
  int rc = MTG_OK;
  if (solve) {
    rc = mtg_host_solve_linear_batch(N, D, K, r, batch, values, fixed_mask, T.data(), co.data(), fr.data(), nullptr,
                                     ct.data(), st_v.data(), threads);
    if (rc != MTG_OK) return rc;
  }
  for (int64_t b = 0; b < batch; ++b) {
    const uint8_t* mask = fixed_mask + b * V;
    for (int v = 0; v < V; ++v)
      for (int k = 0; k < h; ++k)
        for (int d = 0; d < D; ++d) {
          const size_t e = ((size_t)v * h + k) * D + d;
          const int fi = mtg::objective_free_index(mask, v, k, h);
          vv[b * per + e] = ((mask[v] >> k) & 1u) ? values[b * per + e]
                            : solve               ? fr[b * gper + (size_t)d * V * h + fi]
                                                  : x[b * x_stride + K + (int64_t)d * n_free[b] + fi];
        }
  }

  // ---- the parts
  std::vector<double> J_c(nB, 0.0), J_sc(nB, 0.0), J_t(nB, 0.0);
  std::vector<uint8_t> coll(nB, 0);
  std::vector<mtg_extremum> mx((size_t)nB * C);
  if (!solve) {
    mtg::run_threads(batch, threads, [&](int64_t b0, int64_t b1) {
      for (int64_t b = b0; b < b1; ++b)
        ct[b] = (st[b] & MTG_TRAJ_BAD_TIME) ? std::numeric_limits<double>::quiet_NaN()
                                            : derivative_cost(N, D, K, r, vv.data() + b * per, T.data() + b * K, nullptr);
    });
    if (coeffs_out) rc = mtg_host_coefficients_from_vertices_batch(N, D, K, batch, vv.data(), T.data(), co.data(), threads);
  }
  if (rc == MTG_OK && with_max)
    rc = mtg_host_soft_constraint_cost_batch(N, D, K, batch, vv.data(), nullptr, T.data(), constraints, J_sc.data(),
                                             nullptr, mx.data(), st_s.data(), threads);
  if (rc == MTG_OK && with_coll)
    rc = mtg::host_collision_cost_coeff_times(N, D, K, batch, vv.data(), T.data(), coeff_times, grid, collision,
                                              J_c.data(), coll.data(), nullptr, st_c.data(), threads);
  if (rc != MTG_OK) return rc;

  // ---- combine (the rule of mtg_objective_common.h, as the combine kernel applies it)
  const mtg::ObjectiveTimeRule rule{obj, params->time_penalty, params->w_c};
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int64_t b = 0; b < batch; ++b) {
    const int stb = st[b] | st_v[b] | st_s[b] | st_c[b];
    const bool err = (stb & MTG_TRAJ_ERROR_MASK) != 0;
    const int nf = n_free[b];
    if (status) status[b] = stb;
    J_t[b] = mtg::objective_total_time(T.data() + b * K, K);
    if (free_out)
      for (size_t j = 0; j < gper; ++j) {
        const size_t d = j / ((size_t)V * h), i = j % ((size_t)V * h);
        free_out[b * gper + j] = err     ? nan
                                 : solve ? fr[b * gper + j]
                                         : ((int)i < nf ? x[b * x_stride + K + (int64_t)d * nf + (int64_t)i] : 0.0);
      }
    if (coeffs_out)
      for (size_t j = 0; j < cper; ++j) coeffs_out[b * cper + j] = err ? nan : co[b * cper + j];
    for (int c = 0; c < C; ++c) {
      if (constraint_values_out)
        constraint_values_out[b * C + c] = err ? nan : mx[b * C + c].value - constraints->limit[c];
      if (maxima_out) maxima_out[b * C + c] = err ? mtg_extremum{nan, nan, 0, 0} : mx[b * C + c];
    }
    if (err) {
      cost_out[b] = nan;
      if (weighted_costs_out)
        for (int q = 0; q < 4; ++q) weighted_costs_out[4 * b + q] = nan;
      if (collision_out) collision_out[b] = 0;
      continue;
    }
    mtg_objective_state in = {};
    if (state) in = state[b];
    mtg_objective_state out;
    double w4[4];
    cost_out[b] = mtg::objective_time_combine_cost(rule, ct[b], J_c[b], with_soft ? J_sc[b] : 0.0, J_t[b], in, &out, w4);
    if (weighted_costs_out)
      for (int q = 0; q < 4; ++q) weighted_costs_out[4 * b + q] = w4[q];
    if (collision_out) collision_out[b] = coll[b] ? 1 : 0;
    if (state) state[b] = out;
  }
  if (parts) {
    auto put = [](double* dst, const std::vector<double>& src, bool have) {
      if (dst && have) std::copy(src.begin(), src.end(), dst);
    };
    put(parts->J_d, ct, !solve);
    put(parts->J_c, J_c, with_coll);
    put(parts->J_sc, J_sc, with_max);
    put(parts->J_t, J_t, true);
  }
  return MTG_OK;
}

extern "C" int mtg_host_objective_time_bounds_batch(int N, int D, int K, int64_t batch, const uint8_t* fixed_mask,
                                                    int objective, const double* x, int64_t x_stride,
                                                    double initial_stepsize_rel, double* lower, double* upper,
                                                    double* initial_step) {
  if (N < 2 || N > 12 || (N % 2)) return MTG_ERR_UNSUPPORTED_N;
  const int h = N / 2, V = K + 1;
  if (K < 1 || D < 1 || batch < 0) return MTG_ERR_SIZE_MISMATCH;
  const bool times_only = objective == MTG_OBJECTIVE_TIME;
  if ((!times_only && objective != MTG_OBJECTIVE_TIME_AND_CONSTRAINTS) || x_stride < 0) return MTG_ERR_INVALID_ARGUMENT;
  if (batch == 0) return MTG_OK;
  if (!x || (!times_only && !fixed_mask)) return MTG_ERR_INVALID_ARGUMENT;
  for (int64_t b = 0; b < batch; ++b) {
    const int64_t len = K + (times_only ? 0 : (int64_t)D * mtg::objective_n_free(fixed_mask + b * V, V, h));
    if (len > x_stride) return MTG_ERR_INVALID_ARGUMENT;
    for (int64_t j = 0; j < x_stride; ++j) {
      const double xv = x[b * x_stride + j];
      double lo = 0.0, up = 0.0, step = 0.0;
      if (j < len && times_only) {  // nl_impl:248-256, :273-276
        step = initial_stepsize_rel * xv;
        up = xv * 2.0;
        lo = 0.1;
      } else if (j < len) {  // nl_impl:551-562
        const double abs_x = std::abs(xv);
        step = initial_stepsize_rel * abs_x;
        lo = -abs_x * 2;
        up = abs_x * 2;
        if (j < K) lo = 0.1;
      }
      if (lower) lower[b * x_stride + j] = lo;
      if (upper) upper[b * x_stride + j] = up;
      if (initial_step) initial_step[b * x_stride + j] = step;
    }
  }
  return MTG_OK;
}
