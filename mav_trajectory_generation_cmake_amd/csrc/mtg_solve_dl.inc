// mtg_solve_dl.inc -- the batched solve with one lane per (elimination chain, dimension): the
// "dimension-lane" (DL) kernel (included by mtg_solve_dl_n*_d*.hip, one translation unit per (N, D)).
// DESIGN.md 3.2c.
//
// The reference generators' pattern (createRandomVertices / createRandomVerticesPath,
// src/vertex.cpp:27-79, src/polynomial_timing_evaluation.cpp:34-91): both end vertices fix
// derivatives 0..PE (PE = min(4, N/2 - 1)) and each interior vertex fixes exactly its position.  The
// unknowns are derivatives 1..F (F = N/2 - 1) of the interior vertices (and PE+1..F of the end
// vertices), R_pp (lin_impl:298-326) is block tridiagonal with F x F blocks, and it depends on the
// segment times only -- it is the same matrix for every dimension.  Chain A eliminates vertices 0,
// 1, ... up to the meeting vertex m = K/2, chain B the time-reversed trajectory from vertex K down,
// the two Schur halves are summed at m; the backward sweep keeps the LDL^T factors of each vertex
// and re-forms the coupling from the table, with the epilogue fused (segment J's coefficients as
// soon as both its end vertices are final).
//
// A chain takes D lanes, one per dimension: each runs the time-only recurrence and its own
// dimension's right-hand side.  A wave holds 64 / (2 D) trajectories (D = 3: 10, 60 lanes).  The
// recurrence runs in a per-vertex SCALED basis (DlChain) in which the table blocks are constants and
// every time dependence is a power of T_{J-1} / T_J.  The factors are written once per chain to LDS
// (the backward sweep of all D lanes reads them as broadcasts); z' stays in registers.  Inputs are
// gathered straight from HBM into registers and the coefficient runs are written through buffer
// resources with precomputed per-lane offsets.
//
// A wave's trajectories take one of four passes, chosen from each trajectory's own masks (so its
// bits never depend on its wave-mates): the pattern pass above; the ends pass (interior vertices fix
// exactly their position, the end vertices any derivatives with the position -- e.g. the reference's
// 2_vertices_rand / ConstraintPacking masks, ends fixed to ACCELERATION or JERK); the general-mask
// pass (every position fixed, any other derivative); and, for a free position somewhere, the general
// kernel's block function (dl_fallback), four trajectories at a time.
#pragma once
#include "mtg_fused.inc"  // solve_fused_block (the waves of other patterns)

namespace mtg {

typedef __attribute__((address_space(3))) double dl_lds_double;  // (keeps LDS reads ds_read, not flat)

// Table reads in the forward step, the backward step and the coefficient rows are compile-time
// constants: each entry is materialised into an SGPR pair by two s_mov_b32 where it is used (no LDS
// instruction, no latency to wait for).  The cost rows (only when cost_out is asked for) read the LDS
// copy: their ~55 further constants would spill the SGPRs into VGPR lanes.
static __device__ constexpr double k_dl_htilde[MTG_HTILDE_SIZE] = {MTG_HTILDE_VALUES};
static __device__ constexpr double k_dl_a1inv[MTG_A1INV_SIZE] = {MTG_A1INV_VALUES};

// The sweeps are unrolled with a scheduling barrier between steps: the shift register and the
// carried factors are statically indexed (no register copies), and the barrier keeps the scheduler
// from interleaving steps, which is what blew the register budget of the first unrolled version.
#define MTG_DL_STEP_BARRIER() __builtin_amdgcn_sched_barrier(0)

// The pattern the kernel serves: both end vertices fix derivatives 0..PE and nothing above, every
// interior vertex exactly its position -- the reference generators' (createRandomVertices /
// createRandomVerticesPath with max_derivative 4, src/vertex.cpp:27-79,
// src/polynomial_timing_evaluation.cpp:34-91): PE = min(4, N/2 - 1).  With PE < N/2 - 1 (N = 12,
// config 4) the end vertices keep F - PE free derivatives: vertex 0 of each chain is then a step of
// its own (J0 = 0), whose matrix is a constant block of TL~.
template <int N, int KMAX, int D>
struct DlShape {
  static constexpr int H = N / 2, F = H - 1, KC = KMAX / 2, KS = KC - 1;
  static constexpr int PE = F < 4 ? F : 4, NF0 = F - PE;  // fixed / free derivatives (above the position) at the ends
  static constexpr int J0 = NF0 > 0 ? 0 : 1;              // the first chain vertex with unknowns
  static constexpr int NL = F * (F - 1) / 2;  // strictly lower entries of an F x F unit L
  static constexpr int FS = NL + F;           // one stored vertex's factors: L, then 1 / pivots
  static constexpr int TPW = kBlock / (2 * D);  // trajectories per wave, at most
  // Long chains (config 4: KC = 10) run one wave per SIMD (RR): z' of every chain vertex stays in
  // registers (the compiler parks the vertices not in use in AGPRs) and the segment times are parked
  // once per chain, not per lane, so a wave needs ~38 KB of LDS and four fit a CU -- 1e4 trajectories
  // in one round (with z' in LDS a wave needed 70 KB: two per CU, two rounds).  Short chains
  // (config 2 / 3) run two waves per SIMD, which the 125000-trajectory shards need to hide memory
  // latency.
  static constexpr bool RR = KC > 5;
  static constexpr int WAVES = RR ? 1 : 2;  // waves per SIMD the register budget is built for (no spill)
  // Short chains keep their positions and segment times in registers (PREG: the unrolled sweeps index
  // them statically), so the forward sweep starts when its first vertex's inputs have landed, not
  // after the whole batch of loads -- the load phase overlaps the sweep.  Long chains park them in
  // LDS: positions per lane ([KC+1][kBlock]), times per chain ([KC][2 TPW]).  (The general-mask pass
  // parks them in every shape: its extra live state would not fit the registers otherwise.)
  static constexpr bool PREG = !RR;
  static constexpr int PARK = (KC + 1) * kBlock + KC * 2 * TPW;
  // LDS doubles: factors [TPW][2][FSTR] (vertex J of a chain at J FS; the pattern pass with J0 = 1 leaves
  // the last FS unused),
  // row staging [kBlock][N], parked inputs [PARK][kBlock], reductions [kBlock] (+ as many ints), then
  // Htilde + A(1)^-1 (only launches with cost_out ask for it)
  // Staging rows of N + SPAD doubles: a ds_write_b128 is serviced 8 lanes at a time on 32 banks, so
  // the row stride in 16-B units must be odd for a lane's row to start on its own banks (N = 10: 5,
  // no pad; N = 12: 6 -> 7, one 16-B pad per row; else lanes l and l + 4 conflict).
  static constexpr int SPAD = (N / 2) % 2 == 0 ? 2 : 0, SROW = N + SPAD;
  // A chain's factors take an odd number of 16-B units (FSTR = 2 mod 4 doubles): the backward sweep's
  // reads of one entry by all chains of a wave then hit distinct banks (ds_read_b128: 16-lane groups,
  // (a/4) mod 64, chain c at 4 (FSTR / 2) c), and the 16-B alignment the wide LDS accesses need is
  // kept.  (Config 2's pattern pass used 4 FS = 40 doubles, 20 units: every fourth chain shared a bank.)
  static constexpr int FSTR = KC * FS + ((6 - (KC * FS) % 4) % 4);
  static_assert(FSTR % 4 == 2, "odd 16-B units per chain");
  static constexpr int FAC_OFF = 0, STG_OFF = FAC_OFF + TPW * 2 * FSTR,
                       PARK_OFF = STG_OFF + kBlock * SROW, RED_OFF = PARK_OFF + PARK,
                       TAB_OFF = RED_OFF + kBlock + kBlock / 2;
  static constexpr int LDS_DOUBLES_NOTAB = TAB_OFF, LDS_DOUBLES = TAB_OFF + 2 * N * N;
  static constexpr int N_FREE(int K) { return 2 * NF0 + (K - 1) * F; }
  static constexpr bool OK = N >= 6 && N <= 12 && KMAX >= 4 && KMAX % 2 == 0 && D >= 1 && D <= 4;
};

// NOT_SPD for a segment time whose unscaled system leaves the double range: the other kernels work
// in the unscaled basis, where the pivots of S_v scale like T^e, e = 3-2R .. 2H-1-2R, and report
// NOT_SPD when they under- or overflow; the scaled basis here would not, so the time is checked
// directly (T^e normal and finite for both end exponents, by the binary exponent of T).
template <int N, int R>
__device__ __forceinline__ int dl_scale_bits(double T) {
  constexpr int ea = 3 - 2 * R, eb = N - 1 - 2 * R;
  const int x = __builtin_amdgcn_frexp_exp(T) - 1;  // floor(log2 T) for normal T
  const int xa = x * ea, xb = x * eb;
  return (xa <= -1022 || xa >= 1023 || xb <= -1022 || xb >= 1023) ? MTG_TRAJ_NOT_SPD : 0;
}

// x^e for e in [E0, E1] from x and xi = 1/x: each power one multiplication of two lower ones
// (depth log2 |e|), so no power costs a reciprocal.
template <int E0, int E1>
struct DlPow {
  static constexpr int NP = E1 > 0 ? E1 : 0, NM = E0 < 0 ? -E0 : 0;
  double pp[NP + 1], pm[NM + 1];
  __device__ __forceinline__ DlPow(double x, double xi) {
    pp[0] = 1.0;
    pm[0] = 1.0;
    if constexpr (NP >= 1) pp[1] = x;
    if constexpr (NM >= 1) pm[1] = xi;
#pragma unroll
    for (int k = 2; k <= NP; ++k) pp[k] = pp[k >> 1] * pp[k - (k >> 1)];
#pragma unroll
    for (int k = 2; k <= NM; ++k) pm[k] = pm[k >> 1] * pm[k - (k >> 1)];
  }
  __device__ __forceinline__ double operator()(int e) const { return e >= 0 ? pp[e] : pm[-e]; }
};

// One elimination chain (chain A: vertices 0, 1, ..., KC; chain B: the time-reversed trajectory) of
// one dimension, in a SCALED basis.  The unknowns at chain vertex J are X_J[a] (derivative a + 1,
// a < F); segment J (vertices J, J+1) has time T_J and, with s_J = diag(T_J^(a+1)) and
// sc_J = T_J^(1-2R), the blocks of H_J = sc S Htilde S are TL_J = sc s TL~ s, TR_J = sc s TR~ s,
// BR_J = sc s BR~ s (TL~ = Htilde[1..F][1..F], BR~ = Htilde[H+1..][H+1..], BL~ = TR~^T =
// Htilde[H+1..][1..F]).  Row block J of R_pp is divided by D_L,J = sc_J s_J and the unknowns are
// Y_J = D_R,J X_J with D_R,J = s_J.  Then, with rho = T_{J-1} / T_J:
//   D_L,J^-1 TL_J D_R,J^-1 = TL~,  D_L,J^-1 BR_{J-1} D_R,J^-1 = rho^(a+b+3-2R) BR~,
//   D_L,J^-1 BL_{J-1} D_R,J-1^-1 = rho^(a+2-2R) BL~,  D_L,J-1^-1 TR_{J-1} D_R,J^-1 = BL~^T rho^(b+1),
// so the block LDL^T recurrence becomes
//   S'_J = TL~ + rho^(a+b+3-2R) P_J,   P_J = BR~ - W^T diag(1/d) W,   W = L_{J-1}^-1 BL~^T,
// where BL~^T, BR~, TL~ are compile-time constants and every time-dependent factor is a power of
// rho: the per-step work that depends on the segment times is a handful of multiplications instead
// of scaling each of the ~50 matrix entries it touches.  (S'_J is symmetric; it is congruent to the
// unscaled S_J up to the positive factor sc_J, so it is SPD exactly when S_J is.)  The right-hand
// side and the back substitution:
//   rhs'_J = -(rho^(a+2-2R) (hp dpp + BL~ z'_{J-1}) + hn dpn),   z'_J = S'_J^-1 rhs'_J,
//   Y_J = z'_J - S'_J^-1 BL~^T (rho_{J+1}^(b+1) Y_{J+1}),
// with hp = Htilde[H+a+1][H], hn = Htilde[a+1][H] and positions relative to each segment's start
// (translation invariance, r >= 1).  The segment's scaled end values, which the coefficients and the
// cost are formed from, are then Y_J (start) and rho_{J+1}^(b+1) Y_{J+1} (end): no further scaling.
// The two chains meet at vertex KC in the UNSCALED basis (each chain's half T^(a+b+3-2R) P and
// T^(a+2-2R) rhs', T = T_{KC-1}), summed through a lane shuffle and factored identically in both
// chains, so x_KC is bit-identical in them (up to the sign of odd derivatives).
//
// G (general masks, "GDL"): every vertex fixes its position, any other derivative is fixed or free
// (pinm(J) bit a: derivative a + 1 fixed at chain vertex J) -- every other mask the reference's API
// allows except a free position.  The same recurrence with runtime pinning (symmetric pinning, as in
// the other kernels): pinned rows and columns of S'_J are zeroed with 1 / pivot 0 (factor_pins), so
// the Schur product and the back substitution skip them; pinned entries of z'_J carry the scaled
// fixed values Yf_J = T_J^(a+1) f_J, so BL~ z'_{J-1} couples the previous vertex's fixed values; and
// the right-hand side of a free row gets the fixed values of its own vertex, (TL~ + rho^(a+k+3-2R) BR~)
// Yf_J, and of the next one, BL~^T T_J^(b+1) f_{J+1}.  The back substitution leaves the next vertex's
// pinned entries out of BL~^T v.  Vertex 0 is always a step of its own (J0 = 0).  Checked in numpy
// against the oracle before the kernel was written (scripts/gdl_emulate.py: 2e-10 on config-2 shapes).
//
// EP (the ends pass): the pattern's recurrence with the end vertex's pins known at run time (pm0,
// derivatives 1..F; the position is fixed) and every interior vertex fixing exactly its position.
// Chain vertex 0 is a step of its own (J0 = 0, fvertex0): S'_0 = TL~ with the pinned rows and columns
// pinned (factor_pins), so vertex 1's Schur product and the backward solve at vertex 0 skip them; the
// interior steps are the pattern's.  (With the generators' pins it is the long-chain pattern pass
// exactly, bit for bit: the masked terms it adds are exact zeros.)
//
// ST (status): the chain keeps what the status is made of -- the smallest pivot (pivot_min in the
// factorisations' dependent chain) and, for long chains, the parked times' status bits.  A launch that
// asks for no status, cost or n_free (DlHot, launch_dl_nrk) runs ST = false: the same f64 operations
// on the solution's path, none of the checks.
enum DlMode : int { kDlPattern = 0, kDlEnds = 1, kDlGeneral = 2 };
template <int N, int R, int KMAX, int D, int MODE = kDlPattern, bool ST = true>
struct DlChain {
  using SH = DlShape<N, KMAX, D>;
  static constexpr bool G = MODE == kDlGeneral, EP = MODE == kDlEnds;
  static constexpr int H = SH::H, F = SH::F, KC = SH::KC, KS = SH::KS, NL = SH::NL, FS = SH::FS;
  static constexpr int PE = SH::PE, J0 = (G || EP) ? 0 : SH::J0;
  static constexpr int NN = N, RR_ = R, KM = KMAX, DD = D;
  static constexpr bool GG = G, EE = EP, SS = ST;
  static constexpr unsigned FM = (1u << F) - 1u;
  static constexpr bool RR = SH::RR;
  static constexpr int TOP = KS - 1;
  static constexpr int E0 = 2 - 2 * R, E1 = 2 * H - 1 - 2 * R;  // the powers of rho (and T) used
  static constexpr int li(int i, int k) { return i * (i - 1) / 2 + k; }  // (i, k), i > k, in L

  const dl_lds_double* ht;  // Htilde(N, R), row-major N x N (LDS copy, read as broadcasts)
  const dl_lds_double* a1;  // A(1)^-1 (LDS copy)
  double* park;      // this lane's parked positions: vertex j at park[j kBlock]
  double* tpark;     // its chain's parked times: segment j at tpark[j tstride]
  static constexpr int tstride = 2 * SH::TPW;
  static constexpr bool PR = SH::PREG && !G;  // positions and times in registers (else parked in LDS)
  double Pr[PR ? KC + 1 : 1], Tr[PR ? KC : 1];
  // Long chains' pattern pass (FR): the forward sweep reads its positions and times from registers as
  // their loads land, and parks each in LDS (for the backward sweep) once the step that first uses it
  // has run -- so the sweep starts on its first vertex's inputs instead of after the whole batch of
  // loads and a barrier (the load phase of config 4 is ~4 us of HBM traffic).  The times' status
  // bits are taken as they are parked.
  static constexpr bool FR = SH::RR && !G;
  // (forward() parks P_1 and T_0 after vertex 0's own step: a chain whose vertex 0 has none, J0 = 1,
  // would leave them unparked)
  static_assert(!FR || J0 == 0, "the register-input forward sweep needs vertex 0 as a step of its own");
  double Pf[FR ? KC + 1 : 1], Tf[FR ? KC : 1];
  bool twr;       // FR: this lane parks its chain's times
  int tbits = 0;  // FR: the parked times' status bits
  uint64_t fmask;    // chain B: the sign bit, applied to odd derivatives
  double E0s[F];     // z'_0: the end vertex's derivatives 1..F (chain coordinates), scaled by T_0^(a+1);
                     // its free ones (a >= PE; EP: not in pm0) forward-substituted
  unsigned pm0 = 0;  // EP: the end vertex's pins (bit a: derivative a + 1 fixed)
  int nf0a = 0;      // EP: chain A's end vertex's free derivatives (free_out offsets)
  // z'_J of the stored chain vertices as a shift register: the forward sweep shifts down and writes
  // the new vertex at TOP (which holds z'_0 before the first step), the backward sweep reads TOP and
  // shifts up.  (The sweeps are unrolled, with a scheduling barrier between steps.)
  double Zs[KS > 0 ? KS : 1][F];
  double Y[F];       // the current vertex of the backward sweep, scaled (D_R of its own segment)
  double Tn, tin;    // the time whose powers scale Y (T_{J+1} in the backward sweep) and its inverse
  double* fac;       // this chain's factors in LDS: vertex J (J0..KC-1) at fac[(J - J0) FS]
  bool wr;           // this lane writes the chain's factors
  double pmin = DBL_MAX;
  double cacc = 0.0;
  // G: the chain vertices' pins, this lane's vertex values (buffer resource, vertex 0's offset and
  // the stride between chain vertices, bytes), and the free-value counts (this chain's vertices
  // 0..KC-1; the trajectory's total)
  uint64_t pins;  // bit J F + a: derivative a + 1 fixed at chain vertex J (one register pair)
  double gf[G ? F : 1];  // the next forward step's fixed-value term (gfix)
  __amdgpu_buffer_rsrc_t rvals;
  int vo, vs;
  int csum, ftot;

  // Htilde(N, R)[r][c] (the LDS copy: Ht, the cost rows; compile-time constants: Hc) and A(1)^-1[r][c]
  __device__ __forceinline__ double Ht(int r, int c) const { return ht[r * N + c]; }
  __device__ __forceinline__ double A1(int r, int c) const {
    return k_dl_a1inv[MTG_A1INV_OFF(N) + r * N + c];
  }
  __device__ __forceinline__ double Hc(int r, int c) const {
    return k_dl_htilde[MTG_HTILDE_OFF(N, R) + r * N + c];
  }
  __device__ __forceinline__ double TLc(int a, int b) const { return Hc(a + 1, b + 1); }
  __device__ __forceinline__ double BRc(int a, int b) const { return Hc(H + a + 1, H + b + 1); }
  __device__ __forceinline__ double BLc(int a, int k) const { return Hc(H + a + 1, k + 1); }
  __device__ __forceinline__ double hp(int a) const { return Hc(H + a + 1, H); }
  __device__ __forceinline__ double hn(int a) const { return Hc(a + 1, H); }
  __device__ __forceinline__ double Pj(int j) const { return PR ? Pr[j] : park[j * kBlock]; }
  __device__ __forceinline__ double Tj(int j) const { return PR ? Tr[j] : tpark[j * tstride]; }
  // the forward sweep's view (FR: the registers)
  __device__ __forceinline__ double PjF(int j) const { return FR ? Pf[j] : Pj(j); }
  __device__ __forceinline__ double TjF(int j) const { return FR ? Tf[j] : Tj(j); }
  // FR, after forward step J (the first to use them): park P_{J+1} and T_J for the backward sweep
  __device__ __forceinline__ void park_fwd(int J) {
    if constexpr (FR) {
      park[(J + 1) * kBlock] = Pf[J + 1];
      if (twr) tpark[J * tstride] = Tf[J];
      if constexpr (ST) {
        tbits |= time_bits(Tf[J]) | dl_scale_bits<N, R>(Tf[J]);
        asm volatile("" : "+v"(tbits));  // (taken here, not kept live to the end of the sweep)
      }
    }
  }
  // Every step reads the same table entries: without this the compiler hoists the entries all
  // steps use out of the sweep and keeps them live in registers.  Each step re-reads them.
  __device__ __forceinline__ void fresh_tables() {
    asm volatile("" : "+s"(ht));
    asm volatile("" : "+s"(a1));
  }

  __device__ __forceinline__ double fl(double v, int k) const {
    return (k & 1) ? __builtin_bit_cast(double, __builtin_bit_cast(uint64_t, v) ^ fmask) : v;
  }
  // z'_{J-1} for the forward step at J: the shift register's TOP
  __device__ __forceinline__ double zprev(int J, int k) const { return Zs[TOP][k]; }

  // G: whether derivative a + 1 is fixed at chain vertex J; its fixed value (chain coordinates,
  // unscaled; 0 where it is free), loaded from the vertex values (L2: the positions' lines)
  // (EP: only chain vertex 0 has pins)
  __device__ __forceinline__ unsigned pinm(int J) const {
    return G ? (unsigned)(pins >> (J * F)) & FM : (EP && J == 0 ? pm0 : 0u);
  }
  __device__ __forceinline__ bool pinned(int J, int a) const {
    return G ? ((pins >> (J * F + a)) & 1u) != 0 : (EP && J == 0 && ((pm0 >> a) & 1u) != 0);
  }
  // (The offset is laundered so that each call is a load of its own: merged, the loads of a vertex's
  // values by several steps would keep them live from the first step to the last.)
  __device__ __forceinline__ double fxv(int J, int a) const {
    int off = vo + J * vs + (a + 1) * D * 8;
    asm volatile("" : "+v"(off));
    const double x = fl(__builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rvals, off, 0, 0)), a + 1);
    return pinned(J, a) ? x : 0.0;
  }
  // G: free derivatives at chain vertex J; where vertex J's free values start in free_out
  __device__ __forceinline__ int nfv(int J) const { return F - __builtin_popcount(pinm(J)); }
  __device__ __forceinline__ int free_off(bool chB, int J) const {
    int s = 0;  // chain A: sum over J' < J; chain B: over J' <= J (vertices K .. K - J)
#pragma unroll
    for (int q = 0; q < KC; ++q) s += (chB ? q <= J : q < J) ? nfv(q) : 0;
    return chB ? ftot - s : s;
  }

  // LDL^T of the lower triangle of S in place (unit L below the diagonal), dinv = 1 / pivots.  P0 > 0:
  // rows / columns 0..P0-1 are pinned (identity, nothing eliminated): L zero there and dinv 0, so a
  // later Schur product or back substitution through these factors skips them.
  template <int P0 = 0>
  __device__ __forceinline__ void factor(double (&S)[F][F], double (&dinv)[F]) {
    double dg[F];
#pragma unroll
    for (int j = 0; j < P0; ++j) {
      dinv[j] = 0.0;
      dg[j] = 0.0;
#pragma unroll
      for (int i = j + 1; i < F; ++i) S[i][j] = 0.0;
    }
#pragma unroll
    for (int j = P0; j < F; ++j) {
      double w[F];
      double dj = S[j][j];
#pragma unroll
      for (int k = P0; k < j; ++k) {
        w[k] = S[j][k] * dg[k];
        dj -= S[j][k] * w[k];
      }
      if constexpr (ST) {
        pmin = pivot_min(pmin, dj);
        // (long chains: materialised here -- left to the compiler, every pivot of the sweep stayed live
        // until the status was reduced at the end, 50 doubles at config 4, spilled to AGPRs and scratch;
        // 29.3 -> 28.2 us.  Short chains are faster without it: 10.8 vs 11.1 us at config 2.)
        if (RR) asm volatile("" : "+v"(pmin));
      }
      const double inv = rcp(dj);
      dg[j] = dj;
      dinv[j] = inv;
#pragma unroll
      for (int i = j + 1; i < F; ++i) {
        double t = S[i][j];
#pragma unroll
        for (int k = P0; k < j; ++k) t -= S[i][k] * w[k];
        S[i][j] = t * inv;
      }
    }
  }
  // G: factor() with the rows / columns in pm pinned: zeroed, unit diagonal (so no pivot of them is
  // 0 or NaN), 1 / pivot 0 -- a later Schur product or back substitution skips them.  (Their unit
  // pivots enter pmin, which only tests for a pivot <= 0 or not finite.)
  __device__ __forceinline__ void factor_pins(double (&S)[F][F], double (&dinv)[F], unsigned pm) {
#pragma unroll
    for (int a = 0; a < F; ++a) {
      const bool pa = (pm >> a) & 1u;
#pragma unroll
      for (int b = 0; b < a; ++b) S[a][b] = (pa || ((pm >> b) & 1u)) ? 0.0 : S[a][b];
      S[a][a] = pa ? 1.0 : S[a][a];
    }
    factor(S, dinv);
#pragma unroll
    for (int a = 0; a < F; ++a) dinv[a] = ((pm >> a) & 1u) ? 0.0 : dinv[a];
  }

  // y <- S^-1 y with S = L diag(1/dinv) L^T, L given by element (i, k) = l(i, k)
  template <typename LF>
  __device__ __forceinline__ static void solve(LF l, const double (&dinv)[F], double (&y)[F]) {
#pragma unroll
    for (int i = 1; i < F; ++i)
#pragma unroll
      for (int k = 0; k < i; ++k) y[i] -= l(i, k) * y[k];
#pragma unroll
    for (int i = F - 1; i >= 0; --i) {
      double t = y[i] * dinv[i];
#pragma unroll
      for (int k = i + 1; k < F; ++k) t -= l(k, i) * y[k];
      y[i] = t;
    }
  }

  // One forward step at chain vertex J (FIRST: J == 1, the previous vertex fully pinned, P = BR~;
  // MERGE: J == KC, the meeting vertex: segment J-1 only, summed with the partner lane's half in the
  // unscaled basis).  Lp, Dp: the previous vertex's factors; Tp, tip: T_{J-1} and 1 / T_{J-1}, on
  // return (not MERGE) T_J and 1 / T_J.  Leaves the factors of S' (S for MERGE) in S, dinv and z' (x
  // for MERGE) in rhs.
  template <bool MERGE, bool FIRST>
  __device__ __forceinline__ void fstep(int J, int partner, const double (&Lp)[NL > 0 ? NL : 1],
                                        const double (&Dp)[F], double& Tp, double& tip, double (&S)[F][F],
                                        double (&dinv)[F], double (&rhs)[F]) {
    fresh_tables();
    // P = BR~ - W^T diag(Dp) W, W = Lp^-1 BL~^T (lower triangle)
    double Pm[F][F];
    if constexpr (FIRST) {
#pragma unroll
      for (int a = 0; a < F; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) Pm[a][b] = BRc(a, b);
    } else {
      double W[F][F], U[F][F];
#pragma unroll
      for (int k = 0; k < F; ++k)
#pragma unroll
        for (int a = 0; a < F; ++a) {
          double w = BLc(a, k);
#pragma unroll
          for (int q = 0; q < k; ++q) w -= Lp[li(k, q)] * W[q][a];
          W[k][a] = w;
          U[k][a] = Dp[k] * w;
        }
#pragma unroll
      for (int a = 0; a < F; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) {
          double p = BRc(a, b);
#pragma unroll
          for (int k = 0; k < F; ++k) p -= W[k][a] * U[k][b];
          Pm[a][b] = p;
        }
    }
    // this dimension's coupling to the previous vertex: qv = hp dpp + BL~ z'_{J-1}
    const double pj = PjF(J);
    const double dpp = pj - PjF(J - 1);
    double qv[F];
#pragma unroll
    for (int a = 0; a < F; ++a) {
      double q = hp(a) * dpp;
#pragma unroll
      for (int k = 0; k < F; ++k) q += BLc(a, k) * zprev(J, k);
      qv[a] = q;
    }
    if constexpr (MERGE) {  // this chain's half, unscaled: T^(a+b+3-2R) P and -T^(a+2-2R) qv, T = T_{J-1}
      const DlPow<E0, E1> pw(Tp, tip);
#pragma unroll
      for (int a = 0; a < F; ++a) {
#pragma unroll
        for (int b = 0; b <= a; ++b) S[a][b] = pw(a + b + 3 - 2 * R) * Pm[a][b];
        rhs[a] = -(pw(a + 2 - 2 * R) * qv[a]);
        if constexpr (G) rhs[a] = pinned(J, a) ? 0.0 : rhs[a] - gf[a];  // (gfix: this half's fixed values)
      }
      // the partner's half, in this chain's coordinates: (-1)^(a+b), (-1)^(a+1)
#pragma unroll
      for (int a = 0; a < F; ++a) {
#pragma unroll
        for (int b = 0; b <= a; ++b) {
          const double o = __shfl(S[a][b], partner);
          S[a][b] = ((a + b) & 1) ? S[a][b] - o : S[a][b] + o;
        }
        const double o = __shfl(rhs[a], partner);
        rhs[a] = ((a + 1) & 1) ? rhs[a] - o : rhs[a] + o;
      }
    } else {
      const double Tc = TjF(J), tic = rcp(Tc);
      const DlPow<E0, E1> pw(Tp * tic, Tc * tip);  // rho = T_{J-1} / T_J and 1 / rho
      const double dpn = PjF(J + 1) - pj;
#pragma unroll
      for (int a = 0; a < F; ++a) {
#pragma unroll
        for (int b = 0; b <= a; ++b) S[a][b] = TLc(a, b) + pw(a + b + 3 - 2 * R) * Pm[a][b];
        rhs[a] = -(pw(a + 2 - 2 * R) * qv[a] + hn(a) * dpn);
      }
      if constexpr (G) {  // (gfix: the fixed values' couplings)
#pragma unroll
        for (int a = 0; a < F; ++a) rhs[a] = pinned(J, a) ? 0.0 : rhs[a] - gf[a];
      }
      Tp = Tc;
      tip = tic;
    }
    if constexpr (G) {
      factor_pins(S, dinv, pinm(J));
    } else {
      factor(S, dinv);
    }
    auto l = [&](int i, int k) { return S[i][k]; };
    solve(l, dinv, rhs);  // (G: pinned entries come out 0)
  }

  // G: the fixed values' part of step Jn's right-hand side (before the step: its Schur product needs
  // the registers), scaled like the step's rows, rho = T_{Jn-1} / T_Jn:
  //   previous vertex  rho^(a+2-2R) BL~ Yf_{Jn-1}            (Yf_J = T_J^(k+1) f_J)
  //   own vertex       (TL~ + rho^(a+k+3-2R) BR~) Yf_Jn
  //   next vertex      BL~^T T_Jn^(b+1) f_{Jn+1}
  // and for the meeting vertex (Jn = KC) this chain's half, unscaled (T = T_{KC-1}):
  //   T^(a+2-2R) BL~ Yf_{KC-1} + T^(a+k+3-2R) BR~ f_KC.
  // The sweeps then keep 0 in the pinned entries of z'; the backward rounds put the fixed values in.
  __device__ __forceinline__ void gfix(int Jn) {
    fresh_tables();
    double fp[F], fo[F], fn[F];
#pragma unroll
    for (int a = 0; a < F; ++a) {
      fp[a] = fxv(Jn - 1, a);
      fo[a] = fxv(Jn, a);
      fn[a] = Jn < KC ? fxv(Jn + 1, a) : 0.0;
    }
    const double Tp = Tj(Jn - 1);
    {
      double t = Tp;
#pragma unroll
      for (int a = 0; a < F; ++a) {
        fp[a] *= t;
        t *= Tp;
      }
    }
    if (Jn < KC) {
      const double Tc = Tj(Jn), tic = rcp(Tc);
      const DlPow<E0, E1> pw(Tp * tic, Tc * rcp(Tp));
      double t = Tc;
#pragma unroll
      for (int a = 0; a < F; ++a) {
        fo[a] *= t;
        fn[a] *= t;
        t *= Tc;
      }
#pragma unroll
      for (int a = 0; a < F; ++a) {
        double q = 0.0, o = 0.0;
#pragma unroll
        for (int k = 0; k < F; ++k) {
          q += BLc(a, k) * fp[k];
          o += (TLc(a, k) + pw(a + k + 3 - 2 * R) * BRc(a, k)) * fo[k] + BLc(k, a) * fn[k];
        }
        gf[a] = pw(a + 2 - 2 * R) * q + o;
      }
    } else {
      const DlPow<E0, E1> pw(Tp, rcp(Tp));
#pragma unroll
      for (int a = 0; a < F; ++a) {
        double q = 0.0, o = 0.0;
#pragma unroll
        for (int k = 0; k < F; ++k) {
          q += BLc(a, k) * fp[k];
          o += (pw(a + k + 3 - 2 * R) * BRc(a, k)) * fo[k];
        }
        gf[a] = pw(a + 2 - 2 * R) * q + o;
      }
    }
    // (computed here: otherwise the compiler sinks the arithmetic into the step that uses gf, and the
    // fixed values it loaded are held through that step's Schur product)
#pragma unroll
    for (int a = 0; a < F; ++a) asm volatile("" : "+v"(gf[a]));
  }

  // Forward step at an interior chain vertex J < KC: factors to Lp / Dp (and to LDS for the backward
  // sweep), z'_J into the shift register
  template <bool FIRST>
  __device__ __forceinline__ void fvertex(int J, int partner, double (&Lp)[NL > 0 ? NL : 1], double (&Dp)[F],
                                          double& Tp, double& tip) {
    double S[F][F], dinv[F], rhs[F];
    fstep<false, FIRST>(J, partner, Lp, Dp, Tp, tip, S, dinv, rhs);
    store_vertex(J, S, dinv, rhs, Lp, Dp);
  }

  // The factors of vertex J into Lp / Dp (the next step's) and, by one lane of the chain, to LDS for
  // the backward sweep; z'_J into the shift register or its LDS slot
  __device__ __forceinline__ void store_vertex(int J, const double (&S)[F][F], const double (&dinv)[F],
                                               const double (&rhs)[F], double (&Lp)[NL > 0 ? NL : 1],
                                               double (&Dp)[F]) {
#pragma unroll
    for (int i = 1; i < F; ++i)
#pragma unroll
      for (int k = 0; k < i; ++k) Lp[li(i, k)] = S[i][k];
    if (J >= 1) {
#pragma unroll
      for (int q = 0; q + 1 < KS; ++q)
#pragma unroll
        for (int k = 0; k < F; ++k) Zs[q][k] = Zs[q + 1][k];
    }
#pragma unroll
    for (int i = 0; i < F; ++i) Zs[TOP][i] = rhs[i];  // (J = 0: z'_0 with its free part solved)
#pragma unroll
    for (int i = 0; i < F; ++i) Dp[i] = dinv[i];
    if (wr) {
      double* fv = fac + (J - J0) * FS;
#pragma unroll
      for (int k = 0; k < NL; ++k) fv[k] = Lp[k];
#pragma unroll
      for (int i = 0; i < F; ++i) fv[NL + i] = Dp[i];
    }
  }

  // Chain vertex 0 when it keeps free derivatives (J0 == 0): S'_0 = TL~ on them (segment 0 alone),
  // the fixed ones pinned (the pattern: derivatives 1..PE; EP: pm0); rhs'_0 = -(TL~ z'_fixed + hn dpn).
  // Its factors and z'_0 feed vertex 1 like any other vertex's.
  __device__ __forceinline__ void fvertex0(double (&Lp)[NL > 0 ? NL : 1], double (&Dp)[F]) {
    fresh_tables();
    double S[F][F], dinv[F], rhs[F];
    const double dpn = PjF(1) - PjF(0);
#pragma unroll
    for (int a = 0; a < F; ++a) {
#pragma unroll
      for (int b = 0; b <= a; ++b) S[a][b] = EP || (a >= PE && b >= PE) ? TLc(a, b) : (a == b ? 1.0 : 0.0);
      double q = hn(a) * dpn;
#pragma unroll
      for (int k = 0; k < (EP ? F : PE); ++k) q += TLc(a, k) * E0s[k];  // (EP: E0s is 0 where free)
      rhs[a] = (EP ? !pinned(0, a) : a >= PE) ? -q : 0.0;
    }
    if constexpr (EP) {
      factor_pins(S, dinv, pm0);
    } else {
      factor<PE>(S, dinv);
    }
    auto l = [&](int i, int k) { return S[i][k]; };
    solve(l, dinv, rhs);
#pragma unroll
    for (int a = 0; a < F; ++a) E0s[a] = (EP ? !pinned(0, a) : a >= PE) ? rhs[a] : E0s[a];
#pragma unroll
    for (int a = 0; a < F; ++a) rhs[a] = E0s[a];
    store_vertex(0, S, dinv, rhs, Lp, Dp);
  }

  // G: chain vertex 0 (any pins): S'_0 = TL~ (segment 0 alone), rhs'_0 = -(hn dpn + TL~ Yf_0 +
  // BL~^T T_0^(b+1) f_1); z'_0 with its pinned entries 0.
  __device__ __forceinline__ void gvertex0(double (&Lp)[NL > 0 ? NL : 1], double (&Dp)[F]) {
    fresh_tables();
    double y0[F], n1[F];
#pragma unroll
    for (int a = 0; a < F; ++a) {
      y0[a] = fxv(0, a);
      n1[a] = fxv(1, a);
    }
    const double T0 = Tj(0);
    {
      double t = T0;
#pragma unroll
      for (int a = 0; a < F; ++a) {
        y0[a] *= t;
        n1[a] *= t;
        t *= T0;
      }
    }
    double S[F][F], dinv[F], rhs[F];
    const double dpn = Pj(1) - Pj(0);
#pragma unroll
    for (int a = 0; a < F; ++a) {
#pragma unroll
      for (int b = 0; b <= a; ++b) S[a][b] = TLc(a, b);
      double q = hn(a) * dpn;
#pragma unroll
      for (int k = 0; k < F; ++k) q += TLc(a, k) * y0[k] + BLc(k, a) * n1[k];
      rhs[a] = pinned(0, a) ? 0.0 : -q;
    }
    factor_pins(S, dinv, pinm(0));
    auto l = [&](int i, int k) { return S[i][k]; };
    solve(l, dinv, rhs);  // (pinned entries 0; ZPIN: the fixed values)
#pragma unroll
    for (int a = 0; a < F; ++a) {
      E0s[a] = rhs[a];
      rhs[a] = E0s[a];
    }
    store_vertex(0, S, dinv, rhs, Lp, Dp);
  }

  // E: the end vertex's fixed derivatives 1..PE (chain coordinates).  On return Y = x_KC, UNSCALED
  // (the meeting vertex's free values; scale_meeting() then scales it for the backward sweep).
  __device__ __forceinline__ void forward(int partner, const double (&E)[F]) {
    double Lp[NL > 0 ? NL : 1], Dp[F];  // the previous vertex's factors (unused before vertex 1)
#pragma unroll
    for (int k = 0; k < (NL > 0 ? NL : 1); ++k) Lp[k] = 0.0;
#pragma unroll
    for (int k = 0; k < F; ++k) Dp[k] = 0.0;
    double Tp = TjF(0), tip = rcp(Tp);
    if constexpr (!G) {  // z'_0 = T_0^(a+1) E (the free ones, a >= PE or not in pm0, solved by fvertex0)
      double t = Tp;
#pragma unroll
      for (int a = 0; a < F; ++a) {
        E0s[a] = (EP ? pinned(0, a) : a < PE) ? t * E[a] : 0.0;
        t *= Tp;
      }
    }
#pragma unroll
    for (int q = 0; q < KS; ++q)
#pragma unroll
      for (int k = 0; k < F; ++k) Zs[q][k] = q == TOP && !G ? E0s[k] : 0.0;
    if constexpr (G) {
      gvertex0(Lp, Dp);
      MTG_DL_STEP_BARRIER();
      gfix(1);
      MTG_DL_STEP_BARRIER();
      fvertex<false>(1, partner, Lp, Dp, Tp, tip);
    } else if constexpr (J0 == 0) {
      fvertex0(Lp, Dp);
      park_fwd(0);
      MTG_DL_STEP_BARRIER();
      fvertex<false>(1, partner, Lp, Dp, Tp, tip);
      park_fwd(1);
    } else {
      fvertex<true>(1, partner, Lp, Dp, Tp, tip);
      park_fwd(1);
    }
#pragma unroll
    for (int J = 2; J < KC; ++J) {
      MTG_DL_STEP_BARRIER();
      if constexpr (G) {
        gfix(J);
        MTG_DL_STEP_BARRIER();
      }
      fvertex<false>(J, partner, Lp, Dp, Tp, tip);
      park_fwd(J);
    }
    MTG_DL_STEP_BARRIER();
    if constexpr (G) {
      gfix(KC);
      MTG_DL_STEP_BARRIER();
    }
    double S[F][F], dinv[F], rhs[F];
    fstep<true, false>(KC, partner, Lp, Dp, Tp, tip, S, dinv, rhs);
#pragma unroll
    for (int i = 0; i < F; ++i) Y[i] = G && pinned(KC, i) ? fxv(KC, i) : rhs[i];  // (G: the fixed values)
    Tn = Tp;  // T_{KC-1}: the meeting vertex is scaled with its chain's last segment
    tin = tip;
  }
  __device__ __forceinline__ void scale_meeting() {
    double t = Tn;
#pragma unroll
    for (int a = 0; a < F; ++a) {
      Y[a] *= t;
      t *= Tn;
    }
  }

  // Segment J of the chain, both ends final: the coefficients of the original segment (chain B:
  // reversed, odd derivatives negated back) into occ[0..N), and its cost share.  ys, ye: the scaled
  // end values T^(a+1) x^(a+1) at chain vertices J and J+1; tinv = 1 / T_J.
  //   c = diag(T^-j) A(1)^-1 sh + p e_0,  sh = [0, ys; p1 - p, ye] in the original direction,
  // the top h rows exact (c_j = x_j / j!), the cost 0.5 sc sh^T Htilde sh (mtg_solve_reg.inc).
  __device__ __forceinline__ void segment_row(bool chB, bool want_cost, int J, double tinv, const double (&ys)[F],
                                              const double (&ye)[F], double (&occ)[N]) {
    fresh_tables();
    double sh[N];
    const double pa = Pj(J), pb = Pj(J + 1);
    const double p0 = chB ? pb : pa;
    sh[0] = 0.0;
    sh[H] = chB ? pa - pb : pb - pa;
#pragma unroll
    for (int a = 0; a < F; ++a) {
      sh[a + 1] = chB ? fl(ye[a], a + 1) : ys[a];
      sh[H + a + 1] = chB ? fl(ys[a], a + 1) : ye[a];
    }
    double tp[N];  // tinv^j
    tp[0] = 1.0;
    tp[1] = tinv;
#pragma unroll
    for (int j = 2; j < N; ++j) tp[j] = tp[j >> 1] * tp[j - (j >> 1)];
    occ[0] = p0;
#pragma unroll
    for (int j = 1; j < H; ++j) occ[j] = (A1(j, j) * sh[j]) * tp[j];
#pragma unroll
    for (int j = H; j < N; ++j) {
      double acc = 0.0;
#pragma unroll
      for (int q = 1; q < N; ++q) acc += A1(j, q) * sh[q];
      occ[j] = acc * tp[j];
    }
    if (want_cost) {  // 0.5 sc sh^T Htilde sh (translation-invariant, r >= 1), sc = tinv^(2R-1)
      double q = 0.0;
#pragma unroll
      for (int p = 0; p < N; ++p) {
        double row = 0.5 * Ht(p, p) * sh[p];
#pragma unroll
        for (int t = p + 1; t < N; ++t) row += Ht(p, t) * sh[t];
        q += sh[p] * row;
      }
      cacc += tp[2 * R - 1] * q;
    }
  }

  // y = z'_J - S'_J^-1 BL~^T v (J >= J0), v = rho_{J+1}^(b+1) Y_{J+1}; reads the factors of vertex J.
  // (At J = 0 the pinned derivatives come out as their fixed values: their 1 / pivots are 0.)
  __device__ __forceinline__ void bstep(int J, const double (&v)[F], double (&y)[F]) {
    fresh_tables();
    const double* fv = fac + (J - J0) * FS;
    double Lf[NL > 0 ? NL : 1], Df[F];
#pragma unroll
    for (int k = 0; k < NL; ++k) Lf[k] = fv[k];
#pragma unroll
    for (int i = 0; i < F; ++i) Df[i] = fv[NL + i];
    double tt[F];
#pragma unroll
    for (int a = 0; a < F; ++a) {
      double acc = 0.0;
#pragma unroll
      for (int b = 0; b < F; ++b) acc += BLc(b, a) * v[b];
      tt[a] = acc;
    }
    auto l = [&](int i, int k) { return Lf[li(i, k)]; };
    solve(l, Df, tt);
    if (J == 0) {
#pragma unroll
      for (int i = 0; i < F; ++i) y[i] = E0s[i] - tt[i];
    } else {
#pragma unroll
      for (int i = 0; i < F; ++i) y[i] = Zs[TOP][i] - tt[i];
#pragma unroll
      for (int q = KS - 1; q >= 1; --q)
#pragma unroll
        for (int k = 0; k < F; ++k) Zs[q][k] = Zs[q - 1][k];
    }
  }
};

// (buf_rsrc, mtg_device.h: the kernel's loads and stores address buffer resources with 32-bit
// per-lane byte offsets; an offset past the resource drops a store without a branch)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t dl_rsrc(const void* base, uint32_t bytes) { return buf_rsrc(base, bytes); }
typedef u32x4 dl_u32x4;
typedef u32x2 dl_u32x2;

// Bit q * 2D .. q * 2D + 2D - 1 of a wave ballot: the lanes of the wave's trajectory q
template <int D>
__device__ __forceinline__ bool dl_traj_any(uint64_t ballot, int q) {
  constexpr uint64_t LM = 2 * D >= 64 ? ~0ull : (1ull << (2 * D)) - 1ull;
  return q * 2 * D < 64 && ((ballot >> (q * 2 * D)) & LM) != 0;
}

// The coefficient stores' cache policy for outputs that stay in the Infinity Cache: sc1 (the
// buffer-store cache-policy bit 4 on gfx950).  Measured (same box, interleaved, profiles/r06/): config
// 2 (24 MB of coefficients) 10.9 -> 10.0 us, config 4 (57.6 MB) 27.8 -> 24.3 us; the config-3 shard
// (300 MB) 93 -> 131 us.  Against the batch (r06_sc1): the short chains gain up to 48 MB of output
// (2e4 trajectories), break even at 72 MB and lose from 96 MB; the long chains (config 4's, which
// write more slowly) gain at every size measured, up to 173 MB -- so sc1 below a per-shape output
// size (dl_store_sc1, host side).  (nt and sc0 nt: slower at every size.)
constexpr int kDlSc1 = 16;

// The wave's coefficient stores.  Each backward round, every lane's row (chain ch, dimension d of
// trajectory t: segment J of chain A or K-1-J of chain B) is staged in LDS at stg[lane SROW]; the
// runs (t, ch) of D N doubles are then contiguous in HBM (and in LDS up to the row pads).  A lane writes pieces
// e = lane + u kBlock (16 B; 8 B when the output is only 8-B aligned) of the staged runs: piece e of
// round J goes to byte off[u] + J dlt[u] of the wave's output region -- the same run offset every
// round, only the segment moves -- so the division into runs is done once.  A piece past the wave's
// trajectories, or of a trajectory that breaks the pattern (its outputs come from the fallback),
// gets an offset past the region: the buffer store drops it.
template <int N, int KMAX, int D, int AL16>
struct DlStore {
  static constexpr int DN = D * N, PW = AL16 ? 2 : 1, PPR = DN / PW;
  static constexpr int POL = AL16 == 2 ? kDlSc1 : 0;  // the stores' cache policy
  static constexpr int NU = (DlShape<N, KMAX, D>::TPW * 2 * PPR + kBlock - 1) / kBlock;
  static constexpr int kOOB = 0x40000000;
  static_assert(NU * kBlock * PW <= kBlock * N, "the staged pieces a lane reads lie in the staging area");
  // staged position (in pieces) of piece e: runs are contiguous rows of N doubles, each followed by
  // the row pad (DlShape::SPAD)
  static constexpr int SP = DlShape<N, KMAX, D>::SPAD / PW, RP = N / PW;
  static __device__ __forceinline__ int staged(int e) { return SP ? e + (e / RP) * SP : e; }
  static_assert(DN % PW == 0, "whole 16-B pieces per run");
  int off[NU], dlt[NU];
  __device__ __forceinline__ void init(int lane, int nvt, uint64_t badl) {
    const int lim = nvt * 2 * PPR;
    // the wave's trajectories that break the pattern, one bit each (wave-uniform; none, normally)
    uint32_t badq = 0;
    if (badl != 0) {
#pragma unroll
      for (int q = 0; q < DlShape<N, KMAX, D>::TPW; ++q) badq |= dl_traj_any<D>(badl, q) ? 1u << q : 0u;
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int e = lane + u * kBlock;
      const int run = e / PPR, o = e - run * PPR, q = run >> 1;
      const bool rv = run & 1;
      const bool ok = e < lim && !((badq >> (q & 31)) & 1u);
      off[u] = ok ? (q * KMAX * DN + o * PW + (rv ? (KMAX - 1) * DN : 0)) * 8 : kOOB;
      dlt[u] = ok ? (rv ? -DN * 8 : DN * 8) : 0;
    }
  }
};

// The outputs of a pass, as the pass takes them: the pattern pass's from the kernel's hot header
// (DlHot) and, only where the launch asks for an optional one, from the arguments behind it.
struct DlOuts {
  double* coeffs;
  double* free_out;
  double* cost_out;
  int32_t* status;
  int32_t* n_free_out;
};

// One backward round: y_J (bstep, or z'_0 at J = 0), segment J's coefficients staged in LDS and
// written as the wave's runs (chain A's segment J and chain B's K-1-J of each trajectory), the free
// values of chain vertex J, then y_J becomes the next round's Y.  own: this lane's trajectory is
// valid and follows the pattern (its outputs are this kernel's to write).  FIRSTB: J == KC-1, whose
// end vertex (the meeting vertex) is scaled with T_{KC-1} itself (rho = 1).
template <typename DC, int AL16, bool FIRSTB = false>
__device__ __forceinline__ void dl_round(DC& c, const DlOuts& a, int J, int lane, int ch, int d, bool own, int64_t pb,
                                         double* stg, const DlStore<DC::NN, DC::KM, DC::DD, AL16>& sm,
                                         __amdgpu_buffer_rsrc_t out) {
  constexpr int N = DC::NN, KMAX = DC::KM, D = DC::DD;
  constexpr int H = N / 2, F = H - 1, K = KMAX, V = K + 1;
  const double T = c.Tj(J), tinv = rcp(T);
  double v[F];  // segment J's scaled end values at chain vertex J+1: (T_J / T_{J+1})^(b+1) Y_{J+1}
  if constexpr (FIRSTB) {
#pragma unroll
    for (int b = 0; b < F; ++b) v[b] = c.Y[b];
  } else {
    const double rho = T * c.tin;
    double rp = rho;
#pragma unroll
    for (int b = 0; b < F; ++b) {
      v[b] = rp * c.Y[b];
      rp *= rho;
    }
  }
  using SH = DlShape<N, KMAX, D>;
  double y[F];
  if (FIRSTB || J >= DC::J0) {
    if constexpr (DC::GG) {  // the next vertex's pinned entries are not unknowns: out of BL~^T v
      double vb[F];
#pragma unroll
      for (int b = 0; b < F; ++b) vb[b] = c.pinned(J + 1, b) ? 0.0 : v[b];
      c.bstep(J, vb, y);
    } else {
      c.bstep(J, v, y);
    }
  } else {
#pragma unroll
    for (int k = 0; k < F; ++k) y[k] = c.E0s[k];
  }
  if constexpr (DC::GG) {  // the vertex's pinned entries: its fixed values, scaled Yf_J = T_J^(k+1) f_J
    double tp = T;
#pragma unroll
    for (int k = 0; k < F; ++k) {
      y[k] = c.pinned(J, k) ? tp * c.fxv(J, k) : y[k];
      tp *= T;
    }
  }
  double occ[N];
  c.segment_row(ch != 0, DC::SS && a.cost_out != nullptr, J, tinv, y, v, occ);
  if (DC::GG && a.free_out && own) {
    // chain vertex J's free values in the reference's (vertex, derivative) order, at the offset of
    // its vertex among all vertices' free values
    double* fo = a.free_out + (pb * D + d) * ((int64_t)V * H) + c.free_off(ch != 0, J);
    const unsigned fr = ~c.pinm(J) & DC::FM;
    double tp = tinv;
#pragma unroll
    for (int k = 0; k < F; ++k) {
      const double x = y[k] * tp;  // unscaled: X_J = T_J^-(k+1) Y_J
      if ((fr >> k) & 1u) fo[__builtin_popcount(fr & ((1u << k) - 1u))] = ch ? c.fl(x, k + 1) : x;
      tp *= tinv;
    }
  } else if (DC::EE && a.free_out && own) {
    // the end vertex's free derivatives (not in pm0), then F per interior vertex: chain A's end vertex
    // has nf0a of them
    const int vx = ch ? K - J : J;
    double* fo = a.free_out + (pb * D + d) * ((int64_t)V * H) + (vx == 0 ? 0 : c.nf0a + (vx - 1) * F);
    const unsigned fr = ~c.pinm(J) & DC::FM;
    double tp = tinv;
#pragma unroll
    for (int k = 0; k < F; ++k) {
      const double x = y[k] * tp;  // unscaled: X_J = T_J^-(k+1) Y_J
      if ((fr >> k) & 1u) fo[__builtin_popcount(fr & ((1u << k) - 1u))] = ch ? c.fl(x, k + 1) : x;
      tp *= tinv;
    }
  } else if ((J >= 1 || SH::NF0 > 0) && a.free_out && own) {
    // chain vertex J's free values in the reference's (vertex, derivative) order: the end vertex's
    // NF0 (derivatives PE+1..F), then F per interior vertex
    const int vx = ch ? K - J : J;
    double* fo = a.free_out + (pb * D + d) * ((int64_t)V * H) +
                 (vx == 0 ? 0 : (vx == K ? SH::NF0 + (K - 1) * F : SH::NF0 + (vx - 1) * F)) - (J == 0 ? SH::PE : 0);
    double tp = tinv;
#pragma unroll
    for (int k = 0; k < F; ++k) {
      const double x = y[k] * tp;  // unscaled: X_J = T_J^-(k+1) Y_J
      if (J >= 1 || k >= SH::PE) fo[k] = ch ? c.fl(x, k + 1) : x;
      tp *= tinv;
    }
  }
#pragma unroll
  for (int k = 0; k < F; ++k) c.Y[k] = y[k];
  c.Tn = T;
  c.tin = tinv;
  if (!a.coeffs) return;
  dvec2* o2 = reinterpret_cast<dvec2*>(stg + lane * SH::SROW);
#pragma unroll
  for (int j = 0; j < N / 2; ++j) o2[j] = dvec2{occ[2 * j], occ[2 * j + 1]};
  lds_fence();
  // every staged read of the round is issued before the first store: one LDS latency per round
  constexpr int NU = DlStore<N, KMAX, D, AL16>::NU;
  // (the cache policy is an immediate of the instruction: SC1, a template parameter -- a run-time
  // branch between the two forms changed the long-chain ends pass's register allocation enough to
  // break it, round 6: see DESIGN 3.2c)
  constexpr int kAux = DlStore<N, KMAX, D, AL16>::POL;
  if constexpr (AL16) {
    dvec2 w[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) w[u] = reinterpret_cast<const dvec2*>(stg)[DlStore<N, KMAX, D, AL16>::staged(lane + u * kBlock)];
#pragma unroll
    for (int u = 0; u < NU; ++u)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(dl_u32x4, w[u]), out, sm.off[u] + J * sm.dlt[u], 0, kAux);
  } else {
    double w[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) w[u] = stg[DlStore<N, KMAX, D, AL16>::staged(lane + u * kBlock)];
#pragma unroll
    for (int u = 0; u < NU; ++u)
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(dl_u32x2, w[u]), out, sm.off[u] + J * sm.dlt[u], 0, kAux);
  }
  lds_fence();  // (this round's reads before the next round's rows)
}

// Trajectories whose masks are not the pattern run the general kernel's block function
// (solve_fused_slots, mtg_fused.inc) after the wave's DL pass, kDlFallbackTraj at a time (16 lanes
// each): slot s of a pass takes the wave's (pass kDlFallbackTraj + s)-th such trajectory.  A slot's
// arithmetic is independent of the other slots, so every trajectory gets the same bits whatever its
// wave-mates are: the DL kernel's if it follows the pattern, the general kernel's if not.  Its
// register demand (~180 VGPRs) is below the DL path's, so, inlined, it does not raise the kernel's
// allocation.
constexpr int kDlFallbackLgLog2 = 4, kDlFallbackTraj = kBlock >> kDlFallbackLgLog2;
template <int N, int R, int D>
__device__ __forceinline__ void dl_fallback(const SolveArgs& a, int64_t pair0, int nvt, uint64_t badl, double* lds) {
  uint32_t badq = 0;  // the wave's trajectories of other patterns, one bit each (wave-uniform)
  for (int q = 0; q < nvt; ++q) badq |= dl_traj_any<D>(badl, q) ? 1u << q : 0u;
  const int nb = __builtin_popcount(badq);
  const int slot = threadIdx.x >> kDlFallbackLgLog2;
  for (int base = 0; base < nb; base += kDlFallbackTraj) {
    const int k = base + slot;  // this slot's trajectory: the k-th set bit of badq
    uint32_t m = badq;
    for (int i = 0; i < k && m; ++i) m &= m - 1u;
    const bool valid = k < nb;
    const int q = valid ? __builtin_ctz(m) : 0;
    solve_fused_slots<N, R>(a, kDlFallbackLgLog2, pair0 + q, valid, lds);
    __syncthreads();
  }
}

// The kernel's only parameter: the hot header, then the full arguments.
//
// DlHot is everything a plain solve's pattern pass reads, in the kernarg segment's first 64 bytes, so
// the wave's head is one s_load_dwordx16 and one wait before its input loads leave -- the fields used
// to span two lines, the second read only after the first had been waited for and branched on.  What
// is uniform over the launch is worked out once on the host (dl_fill_hot): the byte sizes of a full
// wave's regions (a wave's base is blockIdx.x times one of them, a 32 x 32 -> 64-bit product), the
// last wave's place and trajectory count instead of B, and the plain-solve decision instead of n_cand
// and scales.  The time sweep (not kDlPlain) takes B, n_cand and scales from the arguments behind the
// header, in a branch of its own: its 64-bit divisions stay off the plain path.
//
// The passes other than the pattern's re-read the parameter from the kernarg segment (dl_args): a
// reference to the kernel's parameter would make the kernel copy it to the stack and read its fields
// from there in the pattern pass too, and values shared with the pattern pass would be kept live
// (SGPRs spilled to VGPR lanes) through it.  As the kernel's single explicit parameter it sits at
// offset 0 of the kernarg segment, so the pointer below is its address.
enum DlHotFlags : uint32_t {
  kDlPlain = 1u,     // n_cand == 1 and no scales: pair p is trajectory p, times unscaled
  kDlCoeffs = 2u,    // coeffs != null
  kDlOptional = 4u,  // any of free_out, n_free_out, cost_out, status asked for
};
struct DlHot {
  const double* values;
  const uint8_t* mask;
  const double* times;
  double* coeffs;
  uint32_t vbytes, mbytes, tbytes, obytes;  // bytes of tpw trajectories' values, masks, times, coefficients
  int32_t tpw;                              // trajectories per wave (<= DlShape::TPW)
  uint32_t flags;                           // DlHotFlags
  uint32_t last_block;                      // the launch's last wave ...
  int32_t last_nvt;                         // ... and its trajectories (pairs), 1..tpw
};
static_assert(sizeof(DlHot) == 64, "the hot header is one 64-byte line");
struct DlKernArgs {
  DlHot h;
  SolveArgs a;
};
static_assert(offsetof(DlKernArgs, h) == 0, "the hot header leads the kernarg segment");
__device__ __forceinline__ const DlKernArgs& dl_args() {
  return *reinterpret_cast<const DlKernArgs*>((uintptr_t)__builtin_amdgcn_kernarg_segment_ptr());
}
// The hot header as one 64-byte scalar load, materialised whole: left to the compiler, the fields are
// loaded in pieces where each is first used, each piece with a wait of its own.
__device__ __forceinline__ DlHot dl_hot() {
  typedef uint32_t dl_u32x16 __attribute__((ext_vector_type(16)));
  dl_u32x16 v = *(const __attribute__((address_space(4))) dl_u32x16*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(v));
  return __builtin_bit_cast(DlHot, v);
}

// The header of a launch of B pairs in waves of tpw (host; restated in tests/test_dl_header.py).
// False if a wave's region would not fit 32 bits (no shape the kernel is built for comes near).
inline bool dl_fill_hot(int N, int K, int D, int tpw, const SolveArgs& a, DlHot* h) {
  const int64_t V = K + 1, H = N / 2;
  const int64_t vb = tpw * V * H * D * 8, mb = tpw * V, tb = (int64_t)tpw * K * 8, ob = (int64_t)tpw * K * D * N * 8;
  if (a.B < 1 || tpw < 1 || vb > INT32_MAX || ob > INT32_MAX) return false;
  const int64_t blocks = (a.B + tpw - 1) / tpw;
  if (blocks > UINT32_MAX) return false;
  h->values = a.values;
  h->mask = a.mask;
  h->times = a.times;
  h->coeffs = a.coeffs;
  h->vbytes = (uint32_t)vb;
  h->mbytes = (uint32_t)mb;
  h->tbytes = (uint32_t)tb;
  h->obytes = (uint32_t)ob;
  h->tpw = tpw;
  h->flags = (a.n_cand == 1 && !a.scales ? kDlPlain : 0u) | (a.coeffs ? kDlCoeffs : 0u) |
             (a.free_out || a.n_free_out || a.cost_out || a.status ? kDlOptional : 0u);
  h->last_block = (uint32_t)(blocks - 1);
  h->last_nvt = (int32_t)(a.B - (blocks - 1) * tpw);
  return true;
}

// The wave's and this lane's place in the batch, and the buffer resources of the wave's inputs (one
// trajectory per 2 D lanes: lane t 2D + ch D + d is trajectory t, chain ch, dimension d).
template <int N, int KMAX, int D>
struct DlWave {
  using SH = DlShape<N, KMAX, D>;
  static constexpr int H = N / 2, K = KMAX, V = K + 1;
  int lane, t, r2, ch, d, tq, partner, nvt, trl;
  bool valid;
  int64_t pair0, pb;
  double tscale;
  __amdgpu_buffer_rsrc_t rv, rt, rm;
  const char* obase;           // the wave's coefficients (the values where none are asked for: never stored to)
  int vo, vs, to, ts, mo, ms;  // this lane's first vertex / time / mask and the strides of its chain (bytes)
  // h: the hot header (dl_hot); a: the full arguments behind it (read by a time sweep only)
  __device__ __forceinline__ DlWave(const DlHot& h, const SolveArgs& a, int lane_id) {
    const int tpw = h.tpw;
    lane = lane_id;
    t = lane / (2 * D);
    r2 = lane - t * (2 * D);
    ch = r2 >= D ? 1 : 0;
    d = r2 - ch * D;
    tq = t < SH::TPW ? t : 0;
    partner = ch ? lane - D : lane + D;
    const uint32_t bid = blockIdx.x;
    nvt = bid == h.last_block ? h.last_nvt : tpw;  // the wave's trajectories
    pair0 = (int64_t)((uint64_t)bid * (uint32_t)tpw);
    valid = t < nvt;
    pb = valid ? pair0 + t : pair0;
    obase = (h.flags & kDlCoeffs) ? reinterpret_cast<const char*>(h.coeffs) + (uint64_t)bid * h.obytes
                                  : reinterpret_cast<const char*>(h.values);
    // the wave's problems as buffer resources from its first one on, addressed with 32-bit lane offsets
    if (__builtin_expect((h.flags & kDlPlain) != 0u, 1)) {
      trl = valid ? t : 0;
      rv = dl_rsrc(reinterpret_cast<const char*>(h.values) + (uint64_t)bid * h.vbytes, (uint32_t)(nvt * (V * H * D * 8)));
      rt = dl_rsrc(reinterpret_cast<const char*>(h.times) + (uint64_t)bid * h.tbytes, (uint32_t)(nvt * (K * 8)));
      rm = dl_rsrc(h.mask + (uint64_t)bid * h.mbytes, (uint32_t)(nvt * V));
      tscale = 1.0;
    } else {  // a time sweep: pair pb solves trajectory pb / n_cand with its times scaled
      const int64_t nc = a.n_cand;
      const int64_t tr0 = pair0 / nc;
      trl = (int)(pb / nc - tr0);
      const int64_t ntr = (a.B + nc - 1) / nc;
      const int ntw = (int)(ntr - tr0 < SH::TPW ? ntr - tr0 : SH::TPW);
      rv = dl_rsrc(a.values + tr0 * (V * H * D), (uint32_t)(ntw * V * H * D * 8));
      rt = dl_rsrc(a.times + tr0 * K, (uint32_t)(ntw * K * 8));
      rm = dl_rsrc(a.mask + tr0 * V, (uint32_t)(ntw * V));
      tscale = a.scales ? a.scales[pb % nc] : 1.0;
    }
    // (chain B walks the vertices backwards)
    vo = (trl * (V * H * D) + (ch ? K * H * D : 0) + d) * 8;
    vs = ch ? -(H * D * 8) : H * D * 8;
    to = (trl * K + (ch ? K - 1 : 0)) * 8;
    ts = ch ? -8 : 8;
    mo = trl * V + (ch ? K : 0);
    ms = ch ? -1 : 1;
  }
  // the wave's coefficient runs ([nvt][K][D][N])
  __device__ __forceinline__ __amdgpu_buffer_rsrc_t out() const { return dl_rsrc(obase, (uint32_t)(nvt * (K * D * N * 8))); }
  __device__ __forceinline__ unsigned mask(int j) const { return __builtin_amdgcn_raw_buffer_load_b8(rm, mo + j * ms, 0, 0); }
  __device__ __forceinline__ double time(int j, double sc) const {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rt, to + j * ts, 0, 0)) * sc;
  }
  __device__ __forceinline__ double value(int j, int k) const {
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rv, vo + j * vs + k * D * 8, 0, 0));
  }
};

// A pass's outputs from the full arguments (the cold passes; the pattern pass of a launch that asks
// for an optional output)
__device__ __forceinline__ DlOuts dl_outs(const SolveArgs& a) {
  return DlOuts{a.coeffs, a.free_out, a.cost_out, a.status, a.n_free_out};
}

// Status bits of the chain's segment times (time_bits, dl_scale_bits), materialised where they are
// taken: computed after the sweeps (where the status is reduced), the compiler kept the times live
// through them and, in the long-chain mode, spilled them to scratch.
template <int N, int R, int KC>
__device__ __forceinline__ int dl_time_bits(const double (&Tc)[KC]) {
  int st = 0;
#pragma unroll
  for (int j = 0; j < KC; ++j) st |= time_bits(Tc[j]) | dl_scale_bits<N, R>(Tc[j]);
  asm volatile("" : "+v"(st));
  return st;
}

// One DL pass over the wave (cc: a DlChain of the pattern, ends or general-mask mode): forward
// sweep, meeting vertex, backward sweep with the epilogue fused, per-trajectory status / cost /
// n_free.  mine: this lane's trajectory is the pass's; the others' store pieces are dropped and their
// other outputs guarded.  st: status bits found before the pass (the segment times' --
// dl_time_bits -- and dropped orders).  E: the end vertex's derivatives 1..F (the pattern and ends
// passes; chain coordinates).  tph: the debug build's phase stamps.
template <typename CC, int AL16, typename W>
__device__ __forceinline__ void dl_run_pass(CC& cc, const DlOuts& a, const W& w, const double (&E)[CC::F], bool mine,
                                            int st, double* lds, uint64_t* tph) {
  constexpr int N = CC::NN, R = CC::RR_, KMAX = CC::KM, D = CC::DD;
  using SH = DlShape<N, KMAX, D>;
  constexpr int H = N / 2, F = SH::F, KC = SH::KC;
  constexpr int K = KMAX, V = K + 1;
#ifdef MTG_PHASE_TIMING
#define MTG_DL_PSTAMP(k) tph[k] = __builtin_amdgcn_s_memrealtime()
#else
#define MTG_DL_PSTAMP(k) (void)tph
#endif
  const int lane = w.lane, ch = w.ch, d = w.d;
  const int64_t pb = w.pb;
  cc.forward(w.partner, E);
  MTG_DL_PSTAMP(2);
  // (times in registers: their status bits here, after the sweep -- taken before it, they would make
  // the sweep wait for the last segment time's load, where it now starts on the first vertex's)
  if constexpr (CC::SS && CC::PR) st |= dl_time_bits<N, R, KC>(cc.Tr);
  if constexpr (CC::SS && CC::FR) st |= cc.tbits;
  if (a.free_out && mine && ch == 0) {  // the meeting vertex, free values unscaled
    double* fo = a.free_out + (pb * D + d) * ((int64_t)V * H);
    if constexpr (CC::GG) {
      const unsigned fr = ~cc.pinm(KC) & CC::FM;
#pragma unroll
      for (int k = 0; k < F; ++k)
        if ((fr >> k) & 1u) fo[cc.csum + __builtin_popcount(fr & ((1u << k) - 1u))] = cc.Y[k];
    } else {  // (interior: (KC - 1) F slots before it, after the end vertex's free ones)
      const int o0 = CC::EE ? cc.nf0a : SH::NF0;
#pragma unroll
      for (int k = 0; k < F; ++k) fo[o0 + (KC - 1) * F + k] = cc.Y[k];
    }
  }
  cc.scale_meeting();
  __syncthreads();  // the factors (written by one lane per chain) before the backward sweep

  // ---- backward sweep with the epilogue fused, J = KC-1 .. 0 (dl_round)
  double* stg = lds + SH::STG_OFF;
  DlStore<N, KMAX, D, AL16> sm;
  sm.init(lane, w.nvt, __builtin_amdgcn_ballot_w64(!mine));
  const __amdgpu_buffer_rsrc_t ro = w.out();
  dl_round<CC, AL16, true>(cc, a, KC - 1, lane, ch, d, mine, pb, stg, sm, ro);
#pragma unroll
  for (int J = KC - 2; J >= 1; --J) {
    MTG_DL_STEP_BARRIER();
    dl_round<CC, AL16>(cc, a, J, lane, ch, d, mine, pb, stg, sm, ro);
  }
  MTG_DL_STEP_BARRIER();
  dl_round<CC, AL16>(cc, a, 0, lane, ch, d, mine, pb, stg, sm, ro);
  MTG_DL_PSTAMP(3);

  // ---- per trajectory: status (both chains, all dimensions) and the cost (sum over its 2 D lanes)
  // (ST = false: the launch asked for none of them)
  if constexpr (CC::SS) {
    if (!(cc.pmin > 0.0 && cc.pmin <= DBL_MAX)) st |= MTG_TRAJ_NOT_SPD;
    if (a.status || a.cost_out) {
      double* red = lds + SH::RED_OFF;
      int* redi = reinterpret_cast<int*>(red + kBlock);
      __syncthreads();
      red[lane] = cc.cacc;
      redi[lane] = st;
      __syncthreads();
      if (w.r2 == 0 && mine) {
        double cost = 0.0;
        int s = 0;
#pragma unroll
        for (int q = 0; q < 2 * D; ++q) cost += red[lane + q], s |= redi[lane + q];
        if (a.cost_out) a.cost_out[pb] = cost;
        if (a.status) a.status[pb] = s;
      }
    }
    if (w.r2 == 0 && mine && a.n_free_out) {
      if constexpr (CC::GG || CC::EE) {
        a.n_free_out[pb] = cc.ftot;
      } else {
        a.n_free_out[pb] = SH::N_FREE(K);
      }
    }
  }
#ifdef MTG_PHASE_TIMING
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the wave's stores have left)
  MTG_DL_PSTAMP(4);
  if (a.free_out && lane == 0) {  // [start, loads, forward, backward, drained, hw_id, xcc_id]
    double* fo = a.free_out + w.pair0 * D * ((int64_t)V * H);
    for (int k = 0; k < 5; ++k) fo[k] = (double)tph[k];
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    fo[5] = (double)hw;
    fo[6] = (double)xcc;
  }
#endif
#undef MTG_DL_PSTAMP
}

// The chain's LDS places (factors, parked inputs, tables) and its lane's role, as every pass sets them
template <typename CC, typename W>
__device__ __forceinline__ void dl_place(CC& c, const W& w, int tpw, double* lds) {
  using SH = DlShape<CC::NN, CC::KM, CC::DD>;
  c.fmask = w.ch ? 0x8000000000000000ull : 0ull;
  c.fac = lds + SH::FAC_OFF + (w.tq * 2 + w.ch) * SH::FSTR;
  c.wr = w.d == 0 && w.t < tpw;
  c.park = lds + SH::PARK_OFF + w.lane;
  c.tpark = lds + SH::PARK_OFF + (CC::KC + 1) * kBlock + w.tq * 2 + w.ch;  // (per chain)
  c.ht = (const dl_lds_double*)(lds + SH::TAB_OFF);
  c.a1 = (const dl_lds_double*)(lds + SH::TAB_OFF + CC::NN * CC::NN);
}

// The pattern's and the ends pass's inputs into the chain: positions and times in registers (PREG),
// or held for the forward sweep (FR), which parks them as it goes (vertex 0's position here).
template <typename CC>
__device__ __forceinline__ void dl_take_inputs(CC& c, const double (&P)[CC::KC + 1], const double (&Tc)[CC::KC], int d,
                                               int t) {
  using SH = DlShape<CC::NN, CC::KM, CC::DD>;
  constexpr int KC = CC::KC;
  if constexpr (CC::PR) {
#pragma unroll
    for (int j = 0; j <= KC; ++j) c.Pr[j] = P[j];
#pragma unroll
    for (int j = 0; j < KC; ++j) c.Tr[j] = Tc[j];
  } else {
    static_assert(CC::FR, "the pattern and ends passes keep their inputs in registers");
#pragma unroll
    for (int j = 0; j <= KC; ++j) c.Pf[j] = P[j];
#pragma unroll
    for (int j = 0; j < KC; ++j) c.Tf[j] = Tc[j];
    c.twr = d == 0 && t < SH::TPW;
    c.park[0] = P[0];  // (the others as the forward sweep takes them: park_fwd)
  }
}

// The ends pass (DlChain<..., kDlEnds>) for the wave's trajectories with eown set: interior vertices
// fix exactly their position, the end vertices their position and any of derivatives 1..F (orders
// above N/2 - 1 dropped with WARN_DROPPED, lin_impl:74-95).  It re-reads its inputs (from L2, with a
// laundered lane id) instead of taking them from the pattern pass, so nothing stays live across that
// pass; in a cold branch, so the register allocator puts any spills here, not in the pattern pass.
template <int N, int R, int KMAX, int D, int AL16, bool ST>
__device__ __forceinline__ void dl_ends_pass(bool eown) {
  const DlKernArgs& ka = dl_args();
  const DlOuts a = dl_outs(ka.a);
  const DlHot h = dl_hot();
  const int tpw = h.tpw;
#ifdef MTG_PHASE_TIMING  // (debug build: this pass's stamps, written like the pattern pass's)
  uint64_t tph[6];
  tph[0] = __builtin_amdgcn_s_memrealtime();
#else
  uint64_t* tph = nullptr;
#endif
  using SH = DlShape<N, KMAX, D>;
  using EC= DlChain<N, R, KMAX, D, kDlEnds, ST>;
  constexpr int H = N / 2, F = SH::F, KC = SH::KC;
  constexpr unsigned HM = (1u << H) - 1u;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  int lane_id = threadIdx.x;
  asm volatile("" : "+v"(lane_id));
  const DlWave<N, KMAX, D> w(h, ka.a, lane_id);
  EC c;
  dl_place(c, w, tpw, lds);
  const unsigned m0 = w.mask(0);
  double Tc[KC], P[KC + 1], E[F];
  Tc[0] = w.time(0, w.tscale);
#pragma unroll
  for (int k = 0; k < F; ++k) E[k] = c.fl(w.value(0, k + 1), k + 1);
#pragma unroll
  for (int j = 0; j <= KC; ++j) {
    P[j] = w.value(j, 0);
    if (j + 1 < KC) Tc[j + 1] = w.time(j + 1, w.tscale);
  }
  c.pm0 = (m0 >> 1) & EC::FM;
  const int nf0 = F - __builtin_popcount(c.pm0), nfp = __shfl(nf0, w.partner);
  c.nf0a = w.ch ? nfp : nf0;
  c.ftot = nf0 + nfp + (KMAX - 1) * F;
  dl_take_inputs(c, P, Tc, w.d, w.t);
#ifdef MTG_PHASE_TIMING
  tph[1] = __builtin_amdgcn_s_memrealtime();
#endif
  dl_run_pass<EC, AL16>(c, a, w, E, eown, (m0 & ~HM) ? MTG_TRAJ_WARN_DROPPED : 0, lds, tph);
}

// The general-mask pass (DlChain<..., kDlGeneral>) for the wave's trajectories with gown set: every
// position fixed, any other derivative at any vertex.  Like the ends pass it re-reads its inputs and
// runs in a cold branch (it needs more registers than the pattern pass, and its spills go here).
template <int N, int R, int KMAX, int D, int AL16, bool ST>
__device__ __forceinline__ void dl_general_pass(bool gown) {
  const DlKernArgs& ka = dl_args();
  const DlOuts a = dl_outs(ka.a);
  const DlHot h = dl_hot();
  const int tpw = h.tpw;
#ifdef MTG_PHASE_TIMING  // (debug build: this pass's stamps, written like the pattern pass's)
  uint64_t tph[6];
  tph[0] = __builtin_amdgcn_s_memrealtime();
#else
  uint64_t* tph = nullptr;
#endif
  using SH = DlShape<N, KMAX, D>;
  using DG= DlChain<N, R, KMAX, D, kDlGeneral, ST>;
  constexpr int H = N / 2, F = SH::F, KC = SH::KC;
  constexpr unsigned HM = (1u << H) - 1u;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  // (the lane id laundered: everything the pass derives from it, and its loads, are its own -- shared
  // with the kernel's, they would stay live through the pattern pass)
  int lane_id = threadIdx.x;
  asm volatile("" : "+v"(lane_id));
  const DlWave<N, KMAX, D> w(h, ka.a, lane_id);
  DG g;
  dl_place(g, w, tpw, lds);
  g.rvals = w.rv;
  g.vo = w.vo;
  g.vs = w.vs;
  // positions (per lane) and segment times (per chain) parked in LDS, the pins packed
  double P[KC + 1], Tc[KC];
  unsigned mk[KC + 1];
#pragma unroll
  for (int j = 0; j <= KC; ++j) {
    mk[j] = w.mask(j);
    P[j] = w.value(j, 0);
    if (j < KC) Tc[j] = w.time(j, w.tscale);
  }
  int dropped = 0;
  g.pins = 0;
#pragma unroll
  for (int j = 0; j <= KC; ++j) {
    g.pins |= (uint64_t)((mk[j] >> 1) & DG::FM) << (j * F);
    dropped |= mk[j] & ~HM;
    g.park[j * kBlock] = P[j];
  }
  if (w.d == 0 && w.t < SH::TPW) {
#pragma unroll
    for (int j = 0; j < KC; ++j) g.tpark[j * g.tstride] = Tc[j];
  }
  int st0 = 0;
  if constexpr (ST) st0 = dl_time_bits<N, R, KC>(Tc) | (dropped ? MTG_TRAJ_WARN_DROPPED : 0);
  int cs = 0;
#pragma unroll
  for (int j = 0; j < KC; ++j) cs += g.nfv(j);
  g.csum = cs;
  g.ftot = cs + __shfl(cs, w.partner) + g.nfv(KC);
  __syncthreads();  // (the parked times)
#ifdef MTG_PHASE_TIMING
  tph[1] = __builtin_amdgcn_s_memrealtime();
#endif
  double E[F];
#pragma unroll
  for (int k = 0; k < F; ++k) E[k] = 0.0;
  dl_run_pass<DG, AL16>(g, a, w, E, gown, st0, lds, tph);
}

// AL16: the coefficient output is 8-B aligned only (0), 16-B aligned (1), 16-B aligned and written
// with the sc1 cache policy (2: kDlSc1, dl_store_sc1).  A wave's trajectories go through up to four
// passes, each taking the trajectories of its masks (the others' outputs are dropped or guarded):
// the pattern's DL pass, the ends pass (interior vertices exactly their position, any end pins), the
// general-mask DL pass (every vertex fixes its position), and the general kernel's block function
// for the rest (a free position somewhere).  Which pass a trajectory takes depends on its own masks
// only.
// ST: the launch asks for status, cost or n_free (true), or for none of them (false: every pass runs
// without the checks and the reduction that produce them -- DlChain).
template <int N, int R, int KMAX, int D, int AL16, bool ST>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(DlShape<N, KMAX, D>::WAVES))) void solve_dl_kernel(
    DlKernArgs ka) {  // (the single parameter: dl_args)
  using SH = DlShape<N, KMAX, D>;
  using DC = DlChain<N, R, KMAX, D, kDlPattern, ST>;
  constexpr int F = SH::F, KC = SH::KC;
  constexpr unsigned EM = (1u << (SH::PE + 1)) - 1u;  // the end vertices' mask
  const DlHot h = dl_hot();
  const int tpw = h.tpw;
  // the pattern pass's outputs: the coefficients from the header, the optional ones read only where
  // the header says one is asked for
  DlOuts a{h.coeffs, nullptr, nullptr, nullptr, nullptr};
  if (h.flags & kDlOptional) {
    // (the address laundered inside the branch: a plain kernarg load would be hoisted out of it)
    typedef const __attribute__((address_space(4))) char* dl_kptr;  // (constant address space: scalar loads)
    auto fa = (const __attribute__((address_space(4))) SolveArgs*)((dl_kptr)__builtin_amdgcn_kernarg_segment_ptr() +
                                                                   offsetof(DlKernArgs, a));
    asm volatile("" : "+s"(fa));
    a.free_out = fa->free_out;
    if constexpr (ST) {
      a.cost_out = fa->cost_out;
      a.status = fa->status;
      a.n_free_out = fa->n_free_out;
    }
  }
  extern __shared__ __attribute__((aligned(16))) double lds[];
#ifdef MTG_PHASE_TIMING  // (debug build: s_memrealtime stamps per wave, written over the first free values)
  uint64_t tph[6];
  tph[0] = __builtin_amdgcn_s_memrealtime();
#else
  uint64_t* tph = nullptr;
#endif
  const DlWave<N, KMAX, D> w(h, ka.a, threadIdx.x);
  const int t = w.t, d = w.d;

  DC c;
  dl_place(c, w, tpw, lds);
  // ---- one batch of loads, all issued before any is used (one HBM latency): the chain's masks,
  // segment times, vertex positions and end derivatives.  (The masks first, then in the order the
  // forward sweep uses them: loads return in order, so with PREG each step waits only for its own
  // vertex's inputs.)
  unsigned mk[KC + 1];
  double Tc[KC], P[KC + 1], E[F];
#pragma unroll
  for (int j = 0; j <= KC; ++j) mk[j] = w.mask(j);
  Tc[0] = w.time(0, w.tscale);
#pragma unroll
  for (int k = 0; k < F; ++k) E[k] = k < SH::PE ? c.fl(w.value(0, k + 1), k + 1) : 0.0;
#pragma unroll
  for (int j = 0; j <= KC; ++j) {
    P[j] = w.value(j, 0);
    if (j + 1 < KC) Tc[j + 1] = w.time(j + 1, w.tscale);
  }
  // Which pass a trajectory takes, from its masks (bitwise, so the mask loads are not serialised by
  // short-circuiting; a lane sees its chain's vertices, a trajectory is the OR of its 2 D lanes):
  // the pattern (derivatives 0..PE fixed at both ends, exactly the position in between) -> the DL
  // pass; otherwise the end positions fixed and exactly the position in between -> the ends pass;
  // otherwise every position fixed -> the general-mask pass; otherwise the fallback.
  unsigned bad = mk[0] ^ EM, ebad = ~mk[0] & 1u, xpos = 0u;
#pragma unroll
  for (int j = 1; j <= KC; ++j) {
    bad |= mk[j] ^ 1u;
    ebad |= mk[j] ^ 1u;
  }
#pragma unroll
  for (int j = 0; j <= KC; ++j) xpos |= ~mk[j] & 1u;
  const uint64_t badl = __builtin_amdgcn_ballot_w64(bad != 0u), el = __builtin_amdgcn_ballot_w64(ebad != 0u),
                 xl = __builtin_amdgcn_ballot_w64(xpos != 0u);
  const bool pbad = dl_traj_any<D>(badl, t), ebt = dl_traj_any<D>(el, t), xbad = dl_traj_any<D>(xl, t);
  const bool own = w.valid && !pbad, eown = w.valid && pbad && !ebt, gown = w.valid && ebt && !xbad,
             fown = w.valid && xbad;

  if (a.cost_out) {  // the tables (LDS copies: the cost rows read Htilde from there)
    constexpr int UH = (N * N + kBlock - 1) / kBlock;
    const double* hg = c_htilde + MTG_HTILDE_OFF(N, R);
    const double* ag = c_a1inv + MTG_A1INV_OFF(N);
    double hv[UH], av[UH];
#pragma unroll
    for (int u = 0; u < UH; ++u) {
      const int i = w.lane + u * kBlock;
      hv[u] = hg[i < N * N ? i : N * N - 1];
      av[u] = ag[i < N * N ? i : N * N - 1];
    }
#pragma unroll
    for (int u = 0; u < UH; ++u) {
      const int i = w.lane + u * kBlock;
      lds[SH::TAB_OFF + (i < N * N ? i : N * N - 1)] = hv[u];
      lds[SH::TAB_OFF + N * N + (i < N * N ? i : N * N - 1)] = av[u];
    }
  }
  if (__builtin_amdgcn_ballot_w64(own) != 0) {
    dl_take_inputs(c, P, Tc, d, t);
    if (a.cost_out) __syncthreads();  // (the tables)
#ifdef MTG_PHASE_TIMING
    tph[1] = __builtin_amdgcn_s_memrealtime();  // (PREG: nothing waited for the loads yet)
#endif
    dl_run_pass<DC, AL16>(c, a, w, E, own, 0, lds, tph);
  }
  // (cold for the register allocator: their spills go to these passes, not to the pattern's)
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(eown) != 0, 0)) {
    __syncthreads();  // (the table copies; the pattern pass's LDS use before this pass's)
    dl_ends_pass<N, R, KMAX, D, AL16, ST>(eown);
  }
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(gown) != 0, 0)) {
    __syncthreads();  // (the table copies; the previous passes' LDS use before this pass's)
    dl_general_pass<N, R, KMAX, D, AL16, ST>(gown);
  }
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(fown) != 0, 0)) {  // a free position somewhere: the general kernel's block
    __syncthreads();
    dl_fallback<N, R, D>(dl_args().a, w.pair0, w.nvt, __builtin_amdgcn_ballot_w64(fown), lds);
  }
}
// The chain lengths the kernel is built for (per N): config 2/3's and config 4's
__host__ __device__ constexpr int dl_kmax(int N) { return N == 10 ? 10 : (N == 12 ? 20 : 0); }
template <int N, int D>
__host__ __device__ constexpr size_t dl_lds_bytes(bool cost = true) {
  constexpr int KMAX = dl_kmax(N) > 0 ? dl_kmax(N) : 4;
  const size_t dl = sizeof(double) * (size_t)(cost ? DlShape<N, KMAX, D>::LDS_DOUBLES : DlShape<N, KMAX, D>::LDS_DOUBLES_NOTAB);
  const size_t fb = sizeof(double) * (size_t)kDlFallbackTraj * slot_doubles(N / 2, D, KMAX, 1 << kDlFallbackLgLog2);
  return dl > fb ? dl : fb;
}

// The coefficient stores' cache policy for a launch writing `bytes` of coefficients (kDlSc1): sc1
// up to 64 MB for the short chains, 192 MB for the long ones (RR).  MTG_DL_STORE_SC1=0 / 1 forces it
// (A/B runs); read once per process.
inline bool dl_store_sc1(size_t bytes, bool long_chains) {
  static const int force = [] {
    const char* v = getenv("MTG_DL_STORE_SC1");
    return v && (v[0] == '0' || v[0] == '1') ? v[0] - '0' : -1;
  }();
  return force >= 0 ? force == 1 : bytes <= ((size_t)(long_chains ? 192 : 64) << 20);
}

// Whether a launch that asks for no status, cost or n_free runs the status-free instantiation
// (ST = false).  It is the shorter wave: where the launch lasts as long as one wave it gains (same box,
// interleaved, profiles/dl_hot_header_ab.json: config 2 9.63 -> 9.49 us, config 4 23.48 -> 22.50 us),
// but the HBM-bound config-3 shard (300 MB of coefficients, two waves per SIMD) ran 1 % slower with
// it in five pairs of five (medians 92.3 -> 93.3 us).  So, like the sc1 store policy (dl_store_sc1), it is
// chosen below the output size at which the launch turns HBM-bound -- the same bounds; the sizes
// between the two measured regimes are not measured.  MTG_DL_STATUS=1 keeps the checks always, =0
// drops them whenever nothing asks for them (A/B runs); read once per process.
inline bool dl_status_free(size_t bytes, bool long_chains) {
  static const int force = [] {
    const char* v = getenv("MTG_DL_STATUS");
    return v && (v[0] == '0' || v[0] == '1') ? v[0] - '0' : -1;
  }();
  return force >= 0 ? force == 0 : bytes <= ((size_t)(long_chains ? 192 : 64) << 20);
}

template <int N, int R, int KMAX, int D, int AL16, bool ST>
static hipError_t launch_dl_inst(const DlKernArgs& ka, unsigned blocks, size_t lds, hipStream_t stream) {
  if (lds > kMaxLdsPerBlock) {  // (long chains keep z' in LDS: beyond the default dynamic limit)
    const hipError_t e = hipFuncSetAttribute((const void*)solve_dl_kernel<N, R, KMAX, D, AL16, ST>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  launch_kernel((solve_dl_kernel<N, R, KMAX, D, AL16, ST>), dim3(blocks), dim3(kBlock), lds, stream, ka);
  return hipGetLastError();
}

template <int N, int R, int KMAX, int D>
static hipError_t launch_dl_nrk(const SolveArgs& a, hipStream_t stream) {
  if constexpr (!DlShape<N, KMAX, D>::OK || R < 1) {
    return hipErrorInvalidValue;
  } else {
    if (a.K != KMAX) return hipErrorInvalidValue;
    const size_t lds = dl_lds_bytes<N, D>(a.cost_out != nullptr);
    const int tpw = DlShape<N, KMAX, D>::TPW;
    const size_t out_bytes = (size_t)a.B * KMAX * D * N * sizeof(double);
    const bool sc1 = dl_store_sc1(out_bytes, DlShape<N, KMAX, D>::RR);
    if (a.B == 0) return hipSuccess;
    const bool al16 = !(reinterpret_cast<uintptr_t>(a.coeffs) & 15u);
    const int al = al16 ? (sc1 ? 2 : 1) : 0;
    DlKernArgs ka;
    if (!dl_fill_hot(N, KMAX, D, tpw, a, &ka.h)) return hipErrorInvalidValue;
    ka.a = a;
    const unsigned blocks = ka.h.last_block + 1u;
    // the status-free instantiation only when nothing it leaves out is asked for (free_out alone
    // needs none of the checks), and where it is the faster one (dl_status_free)
    const bool st = a.status || a.cost_out || a.n_free_out || !dl_status_free(out_bytes, DlShape<N, KMAX, D>::RR);
    if (st) {
      if (al == 2) return launch_dl_inst<N, R, KMAX, D, 2, true>(ka, blocks, lds, stream);
      if (al == 1) return launch_dl_inst<N, R, KMAX, D, 1, true>(ka, blocks, lds, stream);
      return launch_dl_inst<N, R, KMAX, D, 0, true>(ka, blocks, lds, stream);
    }
    if (al == 2) return launch_dl_inst<N, R, KMAX, D, 2, false>(ka, blocks, lds, stream);
    if (al == 1) return launch_dl_inst<N, R, KMAX, D, 1, false>(ka, blocks, lds, stream);
    return launch_dl_inst<N, R, KMAX, D, 0, false>(ka, blocks, lds, stream);
  }
}

template <int N, int R, int D>
static hipError_t launch_dl_nrd(const SolveArgs& a, hipStream_t stream) {
  if constexpr (dl_kmax(N) > 0) {
    if (a.K == dl_kmax(N)) return launch_dl_nrk<N, R, dl_kmax(N), D>(a, stream);
  }
  return hipErrorInvalidValue;
}

template <int N, int D>
static hipError_t launch_dl_nd(const SolveArgs& a, hipStream_t stream) {
  switch (a.r) {
    case 1: if constexpr (N / 2 > 1) return launch_dl_nrd<N, 1, D>(a, stream); break;
    case 2: if constexpr (N / 2 > 2) return launch_dl_nrd<N, 2, D>(a, stream); break;
    case 3: if constexpr (N / 2 > 3) return launch_dl_nrd<N, 3, D>(a, stream); break;
    case 4: if constexpr (N / 2 > 4) return launch_dl_nrd<N, 4, D>(a, stream); break;
    case 5: if constexpr (N / 2 > 5) return launch_dl_nrd<N, 5, D>(a, stream); break;
    default: break;
  }
  return hipErrorInvalidValue;
}

#define MTG_DL_LAUNCHER(NN, DD)                                                          \
  hipError_t launch_solve_dl_n##NN##_d##DD(const SolveArgs& a, hipStream_t stream) {     \
    return launch_dl_nd<NN, DD>(a, stream);                                              \
  }

}  // namespace mtg
