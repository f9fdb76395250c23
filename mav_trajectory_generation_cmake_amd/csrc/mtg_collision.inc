// mtg_collision.inc -- the kernel of the batched collision cost and gradient over a signed distance
// field and its launcher: the reference's getCostAndGradientCollision
// (polynomial_optimization_nonlinear_impl.h:1523-1709), semantics in include/mtg.h.  Included by
// mtg_collision.hip (uniform K: mtg_collision_cost_batch, DESIGN.md 3.8) and by mtg_collision_ragged.hip
// (CSR batches: mtg_collision_cost_ragged_batch, DESIGN.md 3.18); each unit instantiates one value of
// the Ragged flag.
//
// Mapping: one wave per trajectory.  LDS holds the trajectory's vertex values, segment times and
// coefficients [K][3][N] (formed as coefficients_from_vertices_kernel forms them), plus one chunk of
// 64 samples: positions and step lengths.  A segment is walked in chunks of 64 clock samples:
//   1. every lane runs the chunk's 64 clock additions t += dt (the accumulated clock cannot be
//      formed in parallel bit-exactly; 64 dependent adds are small against step 4) and keeps the
//      value of its own sample;
//   2. lane s evaluates position and velocity of sample s (Horner out of LDS) and the step length
//      to the sample before it (the previous chunk's last position is carried in LDS);
//   3. every lane runs the gate recurrence (time_sum, dist_sum, the first-entry branch) over the
//      chunk's step lengths and keeps the decision and time_sum of its own sample; the state is
//      carried across chunks and segments in registers (wave-uniform);
//   4. the lanes whose sample passed the gate do the seven map lookups, the potential, the cost
//      term and, with the gradient, add their two terms to a per-lane copy of the segment's three
//      N-vectors (registers).
// At the end of a segment the per-lane vectors are summed over the wave by a fixed butterfly and
// replace the segment's coefficients in LDS (no longer needed); the cost partial sums are reduced
// the same way at the end.  No atomics: a trajectory's result depends on nothing but its own data.
// Last, A(T_i)^-T per (segment, axis) column and the free-order packing, as cost_at_times_kernel.
// With coefficient times (mtg_objective_time_batch's stale L_) a third instantiation forms the
// coefficients at those times and walks to `times`; the two kernels of mtg_collision_cost_batch are
// the instantiations without it, untouched.
//
// Ragged: trajectory b's segments start at so = seg_off[b] in times, its vertices at so + b in values
// and mask, its gradient block [3][V_b h] at double offset 3 h (so + b), and it has
// K_b = seg_off[b + 1] - so segments, where the uniform kernels have b K, b V and K.  The block lays
// its LDS out for its own K_b (the launch sizes it for the largest).  Nothing else differs, so a
// trajectory's bytes are those of the uniform call with K = K_b.
#include <type_traits>

#include "mtg_collision_common.h"
#include "mtg_device.h"

namespace mtg {

struct CollisionArgs {
  const double* values;  // [B][V][h][3] all derivatives
  const uint8_t* mask;   // [B][V] (gradient only)
  const double* times;   // [B][K]
  const double* coeff_times;  // [B][K] (nullable): the coefficients' times where they differ from the walk's
  CollisionMap map;
  CollisionPot pot;
  double dt;
  double* cost;          // [B]
  double* grad;          // [B][3][V*h] (nullable, zeroed by the caller)
  uint8_t* collision;    // [B] (nullable)
  int32_t* n_evaluated;  // [B] (nullable)
  int32_t* status;       // [B] (nullable)
  int64_t B;
  int K;
};
// ragged: values [sum K + B][h][3], mask [sum K + B], times [sum K], grad [3 h (sum K + B)]; K is the
// largest K_b (it sized the launch's LDS)
struct CollisionRaggedArgs : CollisionArgs {
  const int64_t* seg_off;  // [B + 1]
};
template <bool Ragged>
using CollArgs = std::conditional_t<Ragged, CollisionRaggedArgs, CollisionArgs>;

namespace {

constexpr int kChunk = 64;         // samples per chunk = lanes
constexpr int kPosStride = 65;     // slot 0: the sample before the chunk

// sum over the wave in a fixed order; every lane gets the total
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// STALE: the coefficients are formed at a.coeff_times, the walk reads a.times (cost only)
template <int N, bool GRAD, bool STALE = false, bool Ragged = false>
__global__ __launch_bounds__(64) void collision_kernel(CollArgs<Ragged> a) {
  static_assert(!(Ragged && STALE), "the ragged kernels have no stale-L_ form");
  constexpr int H = N / 2;
  constexpr unsigned HM = (1u << H) - 1u;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  // ragged: the trajectory's first segment in times, and its own segment count
  [[maybe_unused]] int64_t s0 = 0;
  int K;
  if constexpr (Ragged) {
    s0 = a.seg_off[b];
    K = (int)(a.seg_off[b + 1] - s0);
  } else {
    K = a.K;
  }
  const int V = K + 1;
  const int cols = K * 3;
  double* co = lds;                        // [K][3][N] coefficients, then the segment's gradient vector
  double* tl = co + cols * N;              // [K]
  double* xv = tl + K;                     // [V][H][3]
  double* ps = xv + V * H * 3;             // [3][kPosStride] positions of the chunk
  double* st = ps + 3 * kPosStride;        // [kChunk] step lengths
  const double* vals;
  if constexpr (Ragged) vals = a.values + (s0 + b) * (int64_t)(H * 3);
  else vals = a.values + b * (int64_t)V * H * 3;
  for (int i = lane; i < V * H * 3; i += 64) xv[i] = vals[i];
  bool bad = false;
  for (int i = lane; i < K; i += 64) {
    double T;
    if constexpr (Ragged) T = a.times[s0 + i];
    else T = a.times[b * K + i];
    tl[i] = T;
    bad |= !(T > 0.0 && T <= DBL_MAX) || !(T / a.dt <= kCollisionMaxSegmentSamples);
    if (STALE) {
      const double Tc = a.coeff_times[b * K + i];
      bad |= !(Tc > 0.0 && Tc <= DBL_MAX);
    }
  }
  if (lane < 3) ps[lane * kPosStride] = 0.0;
  __syncthreads();
  if (__any(bad)) {  // not positive / not finite / too long for the clock: no loop is entered
    if (lane == 0) {
      a.cost[b] = __builtin_nan("");
      if (a.collision) a.collision[b] = 0;
      if (a.n_evaluated) a.n_evaluated[b] = 0;
      if (a.status) a.status[b] = MTG_TRAJ_BAD_TIME;
    }
    return;
  }

  // ---- coefficients c_i = A(T_i)^-1 [x_i; x_{i+1}] (coefficients_from_vertices_kernel's arithmetic)
  cdouble* Ai1 = (cdouble*)(c_a1inv + MTG_A1INV_OFF(N));
  for (int j = lane; j < cols; j += 64) {
    const int i = j / 3, d = j - i * 3;
    const double T = STALE ? a.coeff_times[b * K + i] : tl[i];
    double s[H];
    s[0] = 1.0;
#pragma unroll
    for (int k = 1; k < H; ++k) s[k] = s[k - 1] * T;
    double sh[N];
#pragma unroll
    for (int k = 0; k < H; ++k) {
      sh[k] = s[k] * xv[(i * H + k) * 3 + d];
      sh[H + k] = s[k] * xv[((i + 1) * H + k) * 3 + d];
    }
    const double p0 = sh[0];
    sh[0] = 0.0;
    sh[H] -= p0;
    const double tinv = rcp(T);
    double tp = 1.0;
    double* out = co + j * N;
#pragma unroll
    for (int jj = 0; jj < N; ++jj) {
      double acc;
      if (jj < H) {
        acc = (jj == 0) ? p0 : Ai1[jj * N + jj] * sh[jj];
      } else {
        acc = 0.0;
#pragma unroll
        for (int q = 1; q < N; ++q) acc += Ai1[jj * N + q] * sh[q];
      }
      out[jj] = acc * tp;
      tp *= tinv;
    }
  }
  __syncthreads();

  // ---- the sample loop
  const double dt = a.dt, gate = a.pot.increment;
  double time_sum = -1.0, dist_sum = 0.0;  // wave-uniform
  double J = 0.0;                          // per lane
  int evaluated = 0;
  bool collided = false;
  for (int i = 0; i < K; ++i) {
    const double T = tl[i];
    double acc[3][N];
    if (GRAD) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int n = 0; n < N; ++n) acc[k][n] = 0.0;
    }
    double t = 0.0, t_end = 0.0;
    bool done = false;
    while (!done) {  // one chunk of kChunk clock samples; wave-uniform
      // 1. the clock
      double myt = 0.0;
      for (int s = 0; s < kChunk; ++s) {
        myt = (s == lane) ? t : myt;
        t += dt;
        if (!done && !(t < T)) {
          t_end = t;
          done = true;
        }
      }
      const bool valid = myt < T;
      const int nvalid = __popcll(__ballot(valid));  // the valid samples are lanes 0 .. nvalid-1
      // 2. position, velocity, step length
      double pos[3], vel[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double* c = co + (i * 3 + k) * N;
        double p = c[N - 1], v = (double)(N - 1) * c[N - 1];
#pragma unroll
        for (int n = N - 2; n >= 0; --n) p = p * myt + c[n];
#pragma unroll
        for (int n = N - 2; n >= 1; --n) v = v * myt + (double)n * c[n];
        pos[k] = p;
        vel[k] = v;
        ps[k * kPosStride + lane + 1] = p;
      }
      __syncthreads();
      {
        const double dx = pos[0] - ps[lane], dy = pos[1] - ps[kPosStride + lane], dz = pos[2] - ps[2 * kPosStride + lane];
        st[lane] = __builtin_sqrt(dx * dx + dy * dy + dz * dz);
      }
      __syncthreads();
      // 3. the gate recurrence
      bool mine = false;
      double myts = 0.0;
      for (int s = 0; s < nvalid; ++s) {
        bool eval = false;
        double ts = 0.0;
        if (time_sum < 0) {
          time_sum = 0.0;
        } else {
          time_sum += dt;
          dist_sum += st[s];
          if (!(dist_sum < gate)) {
            eval = true;
            ts = time_sum;
            dist_sum = 0.0;
            time_sum = 0.0;
          }
        }
        if (s == lane) {
          mine = eval;
          myts = ts;
        }
      }
      if (lane < 3) ps[lane * kPosStride] = ps[lane * kPosStride + nvalid];  // carried to the next chunk
      __syncthreads();
      // 4. the gated samples
      if (valid && mine) {
        double gc[3] = {0.0, 0.0, 0.0};
        bool pc;
        const double c = collision_potential_at(a.map, a.pot, pos, GRAD, gc, pc);
        collided |= pc;
        ++evaluated;
        const double vn = __builtin_sqrt(vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]);
        J += c * vn * myts;
        if (GRAD && vn > 1e-6) {
          const double tc = myts * c;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double ga = vn * myts * gc[k], gb = tc * vel[k] / vn;
            double tp = 1.0, tm = 0.0;
#pragma unroll
            for (int n = 0; n < N; ++n) {
              acc[k][n] += ga * tp + gb * ((double)n * tm);
              tm = tp;
              tp *= myt;
            }
          }
        }
      }
    }
    time_sum += -dt + (T - t_end);
    if (GRAD) {
      // the segment's three N-vectors: fixed-order sum over the lanes, into the coefficients' place
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int n = 0; n < N; ++n) {
          const double tot = wave_sum(acc[k][n]);
          if (lane == 0) co[(i * 3 + k) * N + n] = tot;
        }
    }
  }
  const double Jt = wave_sum(J);
  const int ne = __popcll(__ballot(collided));
  int et = evaluated;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) et += __shfl_xor(et, o, 64);
  if (lane == 0) {
    a.cost[b] = Jt;
    if (a.collision) a.collision[b] = ne ? 1 : 0;
    if (a.n_evaluated) a.n_evaluated[b] = et;
    if (a.status) a.status[b] = MTG_TRAJ_OK;
  }
  if (!GRAD) return;
  __syncthreads();

  // ---- L_pp^T: A(T_i)^-T = S(T) A(1)^-T diag(T^-j) per (segment, axis) column, in place
  for (int j = lane; j < cols; j += 64) {
    const int i = j / 3;
    const double T = tl[i];
    double s[H];
    s[0] = 1.0;
#pragma unroll
    for (int k = 1; k < H; ++k) s[k] = s[k - 1] * T;
    const double tinv = rcp(T);
    double u[N];
    double tp = 1.0;
#pragma unroll
    for (int jj = 0; jj < N; ++jj) {
      u[jj] = co[j * N + jj] * tp;
      tp *= tinv;
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
      double y = 0.0;
#pragma unroll
      for (int jj = 0; jj < N; ++jj) y += Ai1[jj * N + q] * u[jj];
      co[j * N + q] = s[q % H] * y;
    }
  }
  __syncthreads();
  // vertex v collects the top rows of segment v and the bottom rows of segment v-1; free order
  if (lane < 3) {
    const uint8_t* msk;
    double* g;
    if constexpr (Ragged) {
      msk = a.mask + (s0 + b);
      g = a.grad + (s0 + b) * (int64_t)(3 * H) + lane * (int64_t)(V * H);
    } else {
      msk = a.mask + b * V;
      g = a.grad + (b * 3 + lane) * (int64_t)(V * H);
    }
    int idx = 0;
    for (int v = 0; v <= K; ++v) {
      const unsigned mv = msk[v] & HM;
      for (int q = 0; q < H; ++q) {
        if ((mv >> q) & 1u) continue;
        const double bot = v > 0 ? co[((v - 1) * 3 + lane) * N + H + q] : 0.0;
        const double top = v < K ? co[(v * 3 + lane) * N + q] : 0.0;
        g[idx++] = bot + top;
      }
    }
  }
}

// a.K sizes the LDS: K, or the largest K_b of a ragged batch
template <int N, bool Ragged>
hipError_t launch_collision_n(const CollArgs<Ragged>& a, bool grad, hipStream_t stream) {
  const size_t lds = collision_lds_bytes(N, a.K);
  if (lds > kMaxLdsPerBlock) return hipErrorInvalidValue;
  if (a.B == 0) return hipSuccess;
  if (a.coeff_times && grad) return hipErrorInvalidValue;  // (the stale-L_ gradient is not built)
  if constexpr (Ragged) {
    if (a.coeff_times) return hipErrorInvalidValue;
    if (grad) launch_kernel((collision_kernel<N, true, false, true>), dim3((unsigned)a.B), dim3(64), lds, stream, a);
    else launch_kernel((collision_kernel<N, false, false, true>), dim3((unsigned)a.B), dim3(64), lds, stream, a);
  } else {
    if (a.coeff_times) launch_kernel((collision_kernel<N, false, true>), dim3((unsigned)a.B), dim3(64), lds, stream, a);
    else if (grad) launch_kernel((collision_kernel<N, true>), dim3((unsigned)a.B), dim3(64), lds, stream, a);
    else launch_kernel((collision_kernel<N, false>), dim3((unsigned)a.B), dim3(64), lds, stream, a);
  }
  return hipGetLastError();
}

// the map, the potential and the outputs, which the two forms share
template <bool Ragged>
void collision_fill_args(CollArgs<Ragged>& a, const double* values, const uint8_t* mask, const double* times,
                         const mtg_sdf_grid& grid, const float* distance, const mtg_collision_params& p, double* cost,
                         double* grad, uint8_t* collision, int32_t* n_evaluated, int32_t* status, int64_t B, int K) {
  a.values = values;
  a.mask = mask;
  a.times = times;
  a.coeff_times = nullptr;
  a.map = CollisionMap{distance, grid.nx, grid.ny, grid.nz, {grid.origin[0], grid.origin[1], grid.origin[2]},
                       grid.resolution, grid.oob_distance};
  a.pot = CollisionPot{p.map_resolution, p.epsilon, p.robot_radius, p.coll_pot_multiplier,
                       {p.min_bound[0], p.min_bound[1], p.min_bound[2]},
                       {p.max_bound[0], p.max_bound[1], p.max_bound[2]}, p.use_continuous_distance ? 1 : 0};
  a.dt = p.coll_check_time_increment;
  a.cost = cost;
  a.grad = grad;
  a.collision = collision;
  a.n_evaluated = n_evaluated;
  a.status = status;
  a.B = B;
  a.K = K;
}

template <bool Ragged>
hipError_t launch_collision(int N, const CollArgs<Ragged>& a, bool grad, hipStream_t stream) {
  switch (N) {
    case 6: return launch_collision_n<6, Ragged>(a, grad, stream);
    case 8: return launch_collision_n<8, Ragged>(a, grad, stream);
    case 10: return launch_collision_n<10, Ragged>(a, grad, stream);
    case 12: return launch_collision_n<12, Ragged>(a, grad, stream);
    default: return hipErrorInvalidValue;
  }
}

// LDS bytes of a trajectory of K segments (collision_lds_bytes, defined in mtg_collision.hip)
inline size_t collision_lds_doubles(int N, int K) {
  const int H = N / 2;
  return (size_t)K * 3 * N + K + (size_t)(K + 1) * H * 3 + 3 * kPosStride + kChunk;
}

}  // namespace

}  // namespace mtg
