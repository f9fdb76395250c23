// mtg_collision_time.hip -- batched segment-time gradient of the collision cost
// (mtg_collision_time_gradient_batch): the dJc_dt part of the reference's getCostAndGradientTime
// (polynomial_optimization_nonlinear_impl.h:2155-2243), semantics in include/mtg.h.
//
// Mapping: one block of kWaves waves per trajectory, one launch.  LDS holds the trajectory's vertex
// values, segment times and coefficients [K][3][N] (formed from the UNPERTURBED times, exactly as
// mtg_collision.hip forms them) and the records below.  A "walk" is the reference's sample loop over
// consecutive segments, done by one wave in chunks of 64 clock samples:
//   1. every lane runs the chunk's clock additions t += dt (the accumulated clock cannot be formed in
//      parallel bit-exactly) up to the first value not below the segment's end, and keeps the value
//      of its own sample;
//   2. lane s evaluates position and velocity of sample s (Horner out of LDS) and the step length to
//      the sample before it (lane s-1 by a lane shift; lane 0 takes the carried last position);
//   3. every lane runs the gate recurrence (time_sum, dist_sum, the first-entry branch) over the
//      chunk's step lengths, read lane by lane, and keeps the decision and time_sum of its sample;
//   4. the lanes whose sample passed the gate do the map lookup, the potential and the cost term.
// No LDS is written inside a walk, so the waves of a block need no barrier while they walk.
//
// Round -1: wave 0 walks the unperturbed trajectory and records, per segment m, the state at its
// entry (time_sum, dist_sum, prev_pos), the segment's cost sum and sample count, and from those the
// prefix sums (segments before m) and suffix sums (segments m .. K-1), all in fixed order.
// Rounds 0 ..: perturbation p = 2 n + side goes to wave p mod kWaves.  Its walk restarts from the
// recorded entry of segment n, walks segment n to the perturbed end and goes on through n+1, n+2, ...
// At the entry of a segment m >= n+2 (prev_pos is then the last sample of the unperturbed segment
// m-1 in both walks) it compares (time_sum, dist_sum) bit for bit with the record: equal means the
// rest of the walk is the unperturbed one, so it adds the recorded suffix and stops.  The same code
// instance does every walk, so equal inputs give equal bits.  No atomics; every sum has a fixed order.
#include "mtg_collision_common.h"
#include "mtg_device.h"

namespace mtg {

namespace {

// Waves per block.  A trajectory's bits do not depend on it (each walk is done by one wave, whichever);
// it trades the latency of one trajectory (more waves share the 2K walks) against the waves that idle
// during round -1.  A/B: scripts/variant_lib.sh with -DMTG_COLLISION_TIME_WAVES=n.
#ifndef MTG_COLLISION_TIME_WAVES
#define MTG_COLLISION_TIME_WAVES 2
#endif
constexpr int kWaves = MTG_COLLISION_TIME_WAVES;
constexpr int kThreads = 64 * kWaves;

struct CollisionTimeArgs {
  const double* values;     // [B][V][h][3] all derivatives
  const double* times;      // [B][K]
  CollisionMap map;
  CollisionPot pot;
  double dt, inc;
  double* grad_t;           // [B][K]
  double* side_cost;        // [B][K][2] (nullable)
  int32_t* side_evaluated;  // [B][K][2] (nullable)
  int32_t* walked;          // [B] (nullable)
  int32_t* status;          // [B] (nullable)
  int K;
};

// sums over the wave in a fixed order; every lane gets the total
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the value lane l holds (l wave-uniform)
__device__ __forceinline__ double read_lane(double v, int l) {
  const long long x = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)x, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(x >> 32), l);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// a wave-uniform condition as a scalar branch
__device__ __forceinline__ bool uniform(bool c) { return __builtin_amdgcn_readfirstlane((int)c) != 0; }

__device__ __forceinline__ bool same_bits(double a, double b) {
  return __double_as_longlong(a) == __double_as_longlong(b);
}

template <int N>
__global__ __launch_bounds__(kThreads) void collision_time_kernel(CollisionTimeArgs a) {
  constexpr int H = N / 2;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = a.K, V = K + 1;
  const int cols = K * 3;
  double* co = lds;                      // [K][3][N] coefficients at the unperturbed times
  double* tl = co + cols * N;            // [K]
  double* xv = tl + K;                   // [V][H][3]
  double* e_ts = xv + V * H * 3;         // [K] time_sum at the entry of segment m, unperturbed walk
  double* e_ds = e_ts + K;               // [K] dist_sum
  double* e_pp = e_ds + K;               // [K][3] prev_pos
  double* pre = e_pp + 3 * K;            // [K+1] cost of the segments before m
  double* suf = pre + (K + 1);           // [K+1] cost of the segments m .. K-1
  double* sc = suf + (K + 1);            // [K][2] side costs
  int* pre_e = (int*)(sc + 2 * K);       // [K+1] evaluated samples before m
  int* suf_e = pre_e + (K + 1);          // [K+1] from m on
  int* se = suf_e + (K + 1);             // [K][2] side counts
  int* wk = se + 2 * K;                  // [K][2] segments walked
  const double* vals = a.values + b * (int64_t)V * H * 3;
  for (int i = tid; i < V * H * 3; i += kThreads) xv[i] = vals[i];
  for (int i = tid; i < K; i += kThreads) tl[i] = a.times[b * K + i];
  __syncthreads();
  const double dt = a.dt, inc = a.inc, gate = a.pot.increment;
  bool bad = false;
  for (int i = lane; i < K; i += 64) bad |= collision_time_bad(tl[i], inc, dt);
  if (__any(bad)) {  // the same answer in every wave: no loop is entered
    const double nan = __builtin_nan("");
    for (int n = tid; n < K; n += kThreads) {
      a.grad_t[b * K + n] = nan;
      if (a.side_cost) a.side_cost[(b * K + n) * 2] = a.side_cost[(b * K + n) * 2 + 1] = nan;
      if (a.side_evaluated) a.side_evaluated[(b * K + n) * 2] = a.side_evaluated[(b * K + n) * 2 + 1] = 0;
    }
    if (tid == 0) {
      if (a.walked) a.walked[b] = 0;
      if (a.status) a.status[b] = MTG_TRAJ_BAD_TIME;
    }
    return;
  }

  // ---- coefficients c_i = A(T_i)^-1 [x_i; x_{i+1}] (coefficients_from_vertices_kernel's arithmetic)
  cdouble* Ai1 = (cdouble*)(c_a1inv + MTG_A1INV_OFF(N));
  for (int j = tid; j < cols; j += kThreads) {
    const int i = j / 3, d = j - i * 3;
    const double T = tl[i];
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

  // ---- the walks: round -1 the unperturbed one (wave 0), then the 2K perturbed ones
  const int rounds = (2 * K + kWaves - 1) / kWaves;
  for (int r = -1; r < rounds; ++r) {
    if (r == 0) __syncthreads();  // the records of round -1
    const bool record = r < 0;
    const int p = record ? 0 : r * kWaves + wave;
    const int n = p >> 1, side = p & 1;
    bool active = record ? wave == 0 : p < 2 * K;
    double Tp = 0.0;
    if (active && !record) {
      const double Tn = tl[n];
      Tp = collision_time_perturbed(Tn, inc, side);
      if (!(Tn <= kCollisionTimeClamp) && !(Tn - inc > 0.0)) {  // the reference CHECK-fails here
        if (lane == 0) {
          sc[p] = __builtin_nan("");
          se[p] = 0;
          wk[p] = 0;
        }
        active = false;
      }
    }
    if (!uniform(active)) continue;
    double time_sum = -1.0, dist_sum = 0.0, prev0 = 0.0, prev1 = 0.0, prev2 = 0.0;  // wave-uniform
    if (!record) {
      time_sum = e_ts[n];
      dist_sum = e_ds[n];
      prev0 = e_pp[n * 3];
      prev1 = e_pp[n * 3 + 1];
      prev2 = e_pp[n * 3 + 2];
    }
    double J = 0.0;     // per lane
    int evaluated = 0;  // per lane
    int m = n;
    for (; m < K; ++m) {
      if (record) {
        if (lane == 0) {
          e_ts[m] = time_sum;
          e_ds[m] = dist_sum;
          e_pp[m * 3] = prev0;
          e_pp[m * 3 + 1] = prev1;
          e_pp[m * 3 + 2] = prev2;
        }
      } else if (m >= n + 2 && uniform(same_bits(time_sum, e_ts[m]) && same_bits(dist_sum, e_ds[m]))) {
        break;  // rejoined the unperturbed walk
      }
      const double T = (!record && m == n) ? Tp : tl[m];
      const double* cm = co + m * 3 * N;
      double t = 0.0, t_end = 0.0;
      bool done = false;
      while (!done) {  // one chunk of up to 64 clock samples; wave-uniform
        // 1. the clock
        double myt = 0.0;
        int nvalid = 0;
        for (int s = 0; s < 64; ++s) {
          myt = (s == lane) ? t : myt;
          t += dt;
          nvalid = s + 1;
          if (uniform(!(t < T))) {
            t_end = t;
            done = true;
            break;
          }
        }
        const bool valid = lane < nvalid;
        // 2. position, velocity, step length.  (The compiler barrier keeps the 3 N coefficient loads and
        // their products inside the chunk: hoisted out of the chunk loop they cost 100 VGPRs and a
        // wave per SIMD, for nothing where a segment is one chunk.)
        asm volatile("" ::: "memory");
        double pos[3], vel[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double* c = cm + k * N;
          double q = c[N - 1], v = (double)(N - 1) * c[N - 1];
#pragma unroll
          for (int i = N - 2; i >= 0; --i) q = q * myt + c[i];
#pragma unroll
          for (int i = N - 2; i >= 1; --i) v = v * myt + (double)i * c[i];
          pos[k] = q;
          vel[k] = v;
        }
        double step;
        {
          const double u0 = __shfl_up(pos[0], 1, 64), u1 = __shfl_up(pos[1], 1, 64), u2 = __shfl_up(pos[2], 1, 64);
          const double dx = pos[0] - (lane == 0 ? prev0 : u0), dy = pos[1] - (lane == 0 ? prev1 : u1),
                       dz = pos[2] - (lane == 0 ? prev2 : u2);
          step = __builtin_sqrt(dx * dx + dy * dy + dz * dz);
        }
        // 3. the gate recurrence
        bool mine = false;
        double myts = 0.0;
        for (int s = 0; s < nvalid; ++s) {
          const double d = read_lane(step, s);
          bool eval = false;
          double ts = 0.0;
          if (time_sum < 0) {
            time_sum = 0.0;
          } else {
            time_sum += dt;
            dist_sum += d;
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
        prev0 = read_lane(pos[0], nvalid - 1);  // carried to the next chunk / segment
        prev1 = read_lane(pos[1], nvalid - 1);
        prev2 = read_lane(pos[2], nvalid - 1);
        // 4. the gated samples
        if (valid && mine) {
          double gc[3];
          bool pc;
          const double c = collision_potential_at(a.map, a.pot, pos, false, gc, pc);
          ++evaluated;
          const double vn = __builtin_sqrt(vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]);
          J += c * vn * myts;
        }
      }
      time_sum += -dt + (T - t_end);
      if (record) {  // the segment's own sums
        const double Jm = wave_sum(J);
        const int em = wave_sum(evaluated);
        if (lane == 0) {
          suf[m] = Jm;
          suf_e[m] = em;
        }
        J = 0.0;
        evaluated = 0;
      }
    }
    if (record) {
      if (lane == 0) {  // prefix and suffix sums, in place, fixed order
        double pj = 0.0;
        int pe = 0;
        for (int i = 0; i < K; ++i) {
          pre[i] = pj;
          pre_e[i] = pe;
          pj += suf[i];
          pe += suf_e[i];
        }
        pre[K] = pj;
        pre_e[K] = pe;
        suf[K] = 0.0;
        suf_e[K] = 0;
        for (int i = K - 1; i >= 0; --i) {
          suf[i] += suf[i + 1];
          suf_e[i] += suf_e[i + 1];
        }
      }
    } else {
      const double Jt = wave_sum(J);
      const int et = wave_sum(evaluated);
      if (lane == 0) {
        sc[p] = (pre[n] + Jt) + suf[m];
        se[p] = pre_e[n] + et + suf_e[m];
        wk[p] = m - n;
      }
    }
  }
  __syncthreads();
  for (int n = tid; n < K; n += kThreads) {
    const double j0 = sc[2 * n], j1 = sc[2 * n + 1];
    a.grad_t[b * K + n] = (j1 - j0) / (2.0 * inc);
    if (a.side_cost) {
      a.side_cost[(b * K + n) * 2] = j0;
      a.side_cost[(b * K + n) * 2 + 1] = j1;
    }
    if (a.side_evaluated) {
      a.side_evaluated[(b * K + n) * 2] = se[2 * n];
      a.side_evaluated[(b * K + n) * 2 + 1] = se[2 * n + 1];
    }
  }
  if (tid == 0) {
    if (a.walked) {
      int w = 0;
      for (int q = 0; q < 2 * K; ++q) w += wk[q];
      a.walked[b] = w;
    }
    if (a.status) a.status[b] = MTG_TRAJ_OK;
  }
}

template <int N>
hipError_t launch_collision_time_n(const CollisionTimeArgs& a, int64_t B, hipStream_t stream) {
  const size_t lds = collision_time_lds_bytes(N, a.K);
  if (lds > kMaxLdsPerBlock) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  launch_kernel((collision_time_kernel<N>), dim3((unsigned)B), dim3(kThreads), lds, stream, a);
  return hipGetLastError();
}

}  // namespace

size_t collision_time_lds_bytes(int N, int K) {
  const int H = N / 2;
  const size_t doubles = (size_t)K * 3 * N + K + (size_t)(K + 1) * H * 3 + 5 * (size_t)K + 2 * (size_t)(K + 1) + 2 * (size_t)K;
  const size_t ints = 2 * (size_t)(K + 1) + 4 * (size_t)K;
  return sizeof(double) * doubles + sizeof(int) * ints;
}

hipError_t launch_collision_time_gradient(int N, const double* values, const double* times, const mtg_sdf_grid& grid,
                                          const float* distance, const mtg_collision_params& p, double increment_time,
                                          double* grad_t, double* side_cost, int32_t* side_evaluated, int32_t* walked,
                                          int32_t* status, int64_t B, int K, hipStream_t stream) {
  CollisionTimeArgs a;
  a.values = values;
  a.times = times;
  a.map = CollisionMap{distance, grid.nx, grid.ny, grid.nz, {grid.origin[0], grid.origin[1], grid.origin[2]},
                       grid.resolution, grid.oob_distance};
  a.pot = CollisionPot{p.map_resolution, p.epsilon, p.robot_radius, p.coll_pot_multiplier,
                       {p.min_bound[0], p.min_bound[1], p.min_bound[2]},
                       {p.max_bound[0], p.max_bound[1], p.max_bound[2]}, p.use_continuous_distance ? 1 : 0};
  a.dt = p.coll_check_time_increment;
  a.inc = increment_time;
  a.grad_t = grad_t;
  a.side_cost = side_cost;
  a.side_evaluated = side_evaluated;
  a.walked = walked;
  a.status = status;
  a.K = K;
  switch (N) {
    case 6: return launch_collision_time_n<6>(a, B, stream);
    case 8: return launch_collision_time_n<8>(a, B, stream);
    case 10: return launch_collision_time_n<10>(a, B, stream);
    case 12: return launch_collision_time_n<12>(a, B, stream);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace mtg
