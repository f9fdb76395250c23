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
// Both are plain streaming kernels: consecutive threads write consecutive addresses, no LDS, no
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

}  // namespace

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
