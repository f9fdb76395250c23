// mtg_objective.hip -- the two kernels that go around the component launchers in
// mtg_objective_batch (include/mtg.h): the reference's objective functions in the optimiser's
// variables (polynomial_optimization_nonlinear_impl.h:909-1449).
//
//   objective_unpack_kernel   x, values, fixed_mask -> vertex_values [B][V][h][D] (setFreeConstraints),
//                             times [B][K], n_free [B], the bad-time status, and the scales of 1 the
//                             cost / Jacobian launchers take.  One thread per vertex value.
//   objective_combine_kernel  the parts -> cost, grad in x's layout, weighted costs, collision flag,
//                             state, status, with the NaN rule.  One thread per gradient entry; the
//                             thread of column 0 also writes the row's scalars.
//
// and the three of mtg_objective_time_batch (objectiveFunctionTime[AndConstraints], nl_impl:765-906):
//
//   objective_times_unpack_kernel  objective 3: x -> times [B][K], the bad-time / row-too-short status.
//   objective_assemble_kernel      objective 3: values, fixed_mask, the solve's free_out -> vertex_values.
//                                  One thread per vertex value.
//   objective_time_combine_kernel  the parts -> cost, weighted costs, collision flag, state, status, the
//                                  hard-constraint values, objective 4's free_out, with the NaN rule.
//                                  (objective 4 starts with objective_unpack_kernel.)
//
// All are plain streaming kernels: consecutive threads write consecutive addresses, no LDS, no
// atomics, no scratch, any B (the grid's tail is masked).  The weighted sums must round product by
// product (mtg.h): mtg_objective_common.h carries "#pragma clang fp contract(off)" in each rule.
#include "mtg_internal.h"
#include "mtg_objective_common.h"

namespace mtg {

namespace {

constexpr int kObjThreads = 256;

__global__ __launch_bounds__(kObjThreads) void objective_unpack_kernel(ObjectiveUnpackArgs a) {
  const int64_t per = (int64_t)a.V * a.h * a.D;
  const int64_t gid = (int64_t)blockIdx.x * kObjThreads + threadIdx.x;
  if (gid >= a.B * per) return;
  const int64_t b = gid / per;
  const int e = (int)(gid - b * per);
  const int v = e / (a.h * a.D), k = (e / a.D) % a.h, d = e % a.D;
  const uint8_t* mask = a.mask + b * a.V;
  const double* xr = a.x + b * a.x_stride;
  const int nt = a.times_in ? 0 : a.K;  // objective 2: the K times lead the row
  const int nf = objective_n_free(mask, a.V, a.h);
  // a row that does not fit x_stride is not read at all: the components then see zeros and times of 1
  // (finite work), and the combine kernel turns the trajectory's outputs into NaN by its status
  const bool fits = nt + (int64_t)a.D * nf <= a.x_stride;
  double val;
  if ((mask[v] >> k) & 1u) {
    val = a.values[gid];
  } else {
    val = fits ? xr[nt + (int64_t)d * nf + objective_free_index(mask, v, k, a.h)] : 0.0;
  }
  a.vertex_values[gid] = val;
  if (e < a.K) a.times[b * a.K + e] = a.times_in ? a.times_in[b * a.K + e] : (fits ? xr[e] : 1.0);
  if (e == 0) {
    a.n_free[b] = nf;
    bool bad = false;
    if (a.times_in || fits)
      for (int i = 0; i < a.K; ++i) bad |= objective_time_bad(a.times_in ? a.times_in[b * a.K + i] : xr[i]);
    a.status[b] = (bad ? MTG_TRAJ_BAD_TIME : MTG_TRAJ_OK) | (fits ? 0 : MTG_TRAJ_ROW_TOO_SHORT);
  }
  if (gid < a.K) a.ones[gid] = 1.0;
}

__global__ __launch_bounds__(kObjThreads) void objective_combine_kernel(ObjectiveCombineArgs a) {
  const int64_t W = a.grad_out ? (a.x_stride > 0 ? a.x_stride : 1) : 1;
  const int64_t gid = (int64_t)blockIdx.x * kObjThreads + threadIdx.x;
  if (gid >= a.B * W) return;
  const int64_t b = gid / W;
  const int64_t j = gid - b * W;
  int st = a.st_unpack[b];
  if (a.st_collision) st |= a.st_collision[b];
  if (a.st_soft) st |= a.st_soft[b];
  if (a.st_collision_time) st |= a.st_collision_time[b];
  const bool err = (st & MTG_TRAJ_ERROR_MASK) != 0;
  const int nf = a.n_free[b];
  const int nt = a.rule.objective == MTG_OBJECTIVE_FREE_CONSTRAINTS_AND_COLLISION_AND_TIME ? a.K : 0;

  if (a.grad_out && j < a.x_stride) {
    double g = 0.0;  // the padding past the row
    if (j < nt + (int64_t)a.D * nf) {
      if (err) {
        g = objective_nan();
      } else if (j < nt) {
        g = objective_combine_grad_time(a.rule, a.dJd_dt[b * a.K + j], a.dJc_dt[b * a.K + j]);
      } else {
        const int jj = (int)(j - nt), d = jj / nf, i = jj - d * nf;
        const int64_t o = (b * a.D + d) * (int64_t)(a.V * a.h) + i;
        g = objective_combine_grad(a.rule, a.grad_d[o], a.grad_c ? a.grad_c[o] : 0.0, a.grad_sc ? a.grad_sc[o] : 0.0);
      }
    }
    a.grad_out[b * a.x_stride + j] = g;
  }
  if (j != 0) return;

  if (a.status) a.status[b] = st;
  const double J_t = nt ? objective_total_time(a.times + b * a.K, a.K) : 0.0;
  if (a.J_t_out) a.J_t_out[b] = J_t;
  if (err) {
    a.cost_out[b] = objective_nan();
    if (a.weighted)
      for (int q = 0; q < 4; ++q) a.weighted[4 * b + q] = objective_nan();
    if (a.collision_out) a.collision_out[b] = 0;
    return;  // the state is left as it was
  }
  mtg_objective_state in = {};
  if (a.state) in = a.state[b];
  mtg_objective_state out;
  double w[4];
  const bool coll = a.collision ? a.collision[b] != 0 : false;
  a.cost_out[b] = objective_combine_cost(a.rule, a.J_d[b], a.J_c ? a.J_c[b] : 0.0, a.J_sc ? a.J_sc[b] : 0.0, J_t, coll, in,
                                         &out, w);
  if (a.weighted)
    for (int q = 0; q < 4; ++q) a.weighted[4 * b + q] = w[q];
  if (a.collision_out) a.collision_out[b] = coll ? 1 : 0;
  if (a.state) a.state[b] = out;
}

// ---- mtg_objective_time_batch (objectiveFunctionTime[AndConstraints], nl_impl:765-906)

// objective 3: x holds the K times and nothing else.  One thread per time; the thread of time 0 also
// writes the row's status.
__global__ __launch_bounds__(kObjThreads) void objective_times_unpack_kernel(ObjectiveTimesUnpackArgs a) {
  const int64_t gid = (int64_t)blockIdx.x * kObjThreads + threadIdx.x;
  if (gid >= a.B * a.K) return;
  const int64_t b = gid / a.K;
  const int i = (int)(gid - b * a.K);
  const bool fits = a.K <= a.x_stride;  // (a row that does not fit is not read: times of 1, finite work)
  const double* xr = a.x + b * a.x_stride;
  a.times[gid] = fits ? xr[i] : 1.0;
  if (i == 0) {
    bool bad = false;
    if (fits)
      for (int q = 0; q < a.K; ++q) bad |= objective_time_bad(xr[q]);
    a.status[b] = (bad ? MTG_TRAJ_BAD_TIME : MTG_TRAJ_OK) | (fits ? 0 : MTG_TRAJ_ROW_TOO_SHORT);
  }
}

// objective 3: the fixed entries from `values`, the free ones from the solve's free_out
// (setFreeConstraints' layout).  One thread per vertex value.
__global__ __launch_bounds__(kObjThreads) void objective_assemble_kernel(ObjectiveAssembleArgs a) {
  const int64_t per = (int64_t)a.V * a.h * a.D;
  const int64_t gid = (int64_t)blockIdx.x * kObjThreads + threadIdx.x;
  if (gid >= a.B * per) return;
  const int64_t b = gid / per;
  const int e = (int)(gid - b * per);
  const int v = e / (a.h * a.D), k = (e / a.D) % a.h, d = e % a.D;
  const uint8_t* mask = a.mask + b * a.V;
  double val;
  if ((mask[v] >> k) & 1u) {
    val = a.values[gid];
  } else {
    val = a.free[(b * a.D + d) * (int64_t)(a.V * a.h) + objective_free_index(mask, v, k, a.h)];
  }
  a.vertex_values[gid] = val;
}

// threads per trajectory of the combine-time kernel: the widest of the row outputs it writes
__host__ __device__ inline int64_t objective_time_width(const ObjectiveTimeCombineArgs& a) {
  int64_t W = 1;
  if (a.free_out && (int64_t)a.D * a.V * a.h > W) W = (int64_t)a.D * a.V * a.h;
  if (a.coeffs_out && (int64_t)a.K * a.D * a.N > W) W = (int64_t)a.K * a.D * a.N;
  if ((a.constraint_values || a.maxima_out) && a.C > W) W = a.C;
  return W;
}

// The parts -> cost, weighted costs, collision flag, state, status, the hard-constraint values and
// objective 4's free_out, with the NaN rule.  Thread (b, j) handles entry j of the trajectory's row
// outputs; the thread of entry 0 also writes its scalars.
__global__ __launch_bounds__(kObjThreads) void objective_time_combine_kernel(ObjectiveTimeCombineArgs a) {
  const int64_t W = objective_time_width(a);
  const int64_t gid = (int64_t)blockIdx.x * kObjThreads + threadIdx.x;
  if (gid >= a.B * W) return;
  const int64_t b = gid / W;
  const int64_t j = gid - b * W;
  int st = a.st_unpack[b];
  if (a.st_solve) st |= a.st_solve[b];
  if (a.st_soft) st |= a.st_soft[b];
  if (a.st_collision) st |= a.st_collision[b];
  const bool err = (st & MTG_TRAJ_ERROR_MASK) != 0;
  const int Vh = a.V * a.h;

  if (a.free_out && j < (int64_t)a.D * Vh) {
    double* f = a.free_out + b * (int64_t)a.D * Vh + j;
    if (err) {
      *f = objective_nan();
    } else if (a.rule.objective == MTG_OBJECTIVE_TIME_AND_CONSTRAINTS) {  // the free part of x
      const int nf = a.n_free[b], d = (int)(j / Vh), i = (int)(j - (int64_t)d * Vh);
      *f = i < nf ? a.x[b * a.x_stride + a.K + (int64_t)d * nf + i] : 0.0;
    }
  }
  if (a.coeffs_out && err && j < (int64_t)a.K * a.D * a.N) a.coeffs_out[b * (int64_t)a.K * a.D * a.N + j] = objective_nan();
  if (j < a.C) {
    if (a.constraint_values)
      a.constraint_values[b * a.C + j] = err ? objective_nan() : a.maxima[b * a.C + j].value - a.limit[j];
    if (a.maxima_out && err) a.maxima_out[b * a.C + j] = mtg_extremum{objective_nan(), objective_nan(), 0, 0};
  }
  if (j != 0) return;

  if (a.status) a.status[b] = st;
  const double J_t = objective_total_time(a.times + b * a.K, a.K);
  if (a.J_t_out) a.J_t_out[b] = J_t;
  if (err) {
    a.cost_out[b] = objective_nan();
    if (a.weighted)
      for (int q = 0; q < 4; ++q) a.weighted[4 * b + q] = objective_nan();
    if (a.collision_out) a.collision_out[b] = 0;
    return;  // the state is left as it was
  }
  mtg_objective_state in = {};
  if (a.state) in = a.state[b];
  mtg_objective_state out;
  double w[4];
  a.cost_out[b] = objective_time_combine_cost(a.rule, a.cost_traj[b], a.J_c ? a.J_c[b] : 0.0, a.J_sc ? a.J_sc[b] : 0.0,
                                              J_t, in, &out, w);
  if (a.weighted)
    for (int q = 0; q < 4; ++q) a.weighted[4 * b + q] = w[q];
  if (a.collision_out) a.collision_out[b] = (a.collision && a.collision[b]) ? 1 : 0;
  if (a.state) a.state[b] = out;
}

}  // namespace

hipError_t launch_objective_times_unpack(const ObjectiveTimesUnpackArgs& a, hipStream_t stream) {
  const int64_t total = a.B * a.K;
  if (total == 0) return hipSuccess;
  launch_kernel(objective_times_unpack_kernel, dim3((unsigned)((total + kObjThreads - 1) / kObjThreads)),
                dim3(kObjThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_objective_assemble(const ObjectiveAssembleArgs& a, hipStream_t stream) {
  const int64_t total = a.B * (int64_t)a.V * a.h * a.D;
  if (total == 0) return hipSuccess;
  launch_kernel(objective_assemble_kernel, dim3((unsigned)((total + kObjThreads - 1) / kObjThreads)), dim3(kObjThreads),
                0, stream, a);
  return hipGetLastError();
}

hipError_t launch_objective_time_combine(const ObjectiveTimeCombineArgs& a, hipStream_t stream) {
  const int64_t total = a.B * objective_time_width(a);
  if (total == 0) return hipSuccess;
  launch_kernel(objective_time_combine_kernel, dim3((unsigned)((total + kObjThreads - 1) / kObjThreads)),
                dim3(kObjThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_objective_unpack(const ObjectiveUnpackArgs& a, hipStream_t stream) {
  const int64_t total = a.B * (int64_t)a.V * a.h * a.D;
  if (total == 0) return hipSuccess;
  launch_kernel(objective_unpack_kernel, dim3((unsigned)((total + kObjThreads - 1) / kObjThreads)), dim3(kObjThreads), 0,
                stream, a);
  return hipGetLastError();
}

hipError_t launch_objective_combine(const ObjectiveCombineArgs& a, hipStream_t stream) {
  const int64_t W = a.grad_out ? (a.x_stride > 0 ? a.x_stride : 1) : 1;
  const int64_t total = a.B * W;
  if (total == 0) return hipSuccess;
  launch_kernel(objective_combine_kernel, dim3((unsigned)((total + kObjThreads - 1) / kObjThreads)), dim3(kObjThreads), 0,
                stream, a);
  return hipGetLastError();
}

}  // namespace mtg
