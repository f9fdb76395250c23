// mtg_solve_dl.hip -- dispatch of the dimension-lane kernel (mtg_solve_dl.inc; one translation unit
// per (N, D) in mtg_solve_dl_n*_d*.hip).
#include "mtg_solve_dl.inc"  // (templates only: no kernel is instantiated in this unit)

namespace mtg {

#define MTG_DL_DECL(NN, DD) hipError_t launch_solve_dl_n##NN##_d##DD(const SolveArgs&, hipStream_t);
MTG_DL_DECL(10, 1) MTG_DL_DECL(10, 2) MTG_DL_DECL(10, 3) MTG_DL_DECL(10, 4)
MTG_DL_DECL(12, 1) MTG_DL_DECL(12, 2) MTG_DL_DECL(12, 3) MTG_DL_DECL(12, 4)
#undef MTG_DL_DECL

// Shapes the kernel serves: N = 10 with K = 10 (configs 2, 3) and N = 12 with K = 20 (config 4),
// D <= 4, r >= 1 (translation-relative positions); its LDS (and the general kernel's block function's,
// for the trajectories of other patterns) within a CU's 160 KB.
bool dl_geometry(int N, int D, int K, int r) {
  if (D < 1 || D > 4 || r < 1 || r > N / 2 - 1 || K != dl_kmax(N) || K == 0) return false;
  size_t lds = 0;
#define MTG_DL_LDS(NN, DD) \
  if (N == NN && D == DD) lds = dl_lds_bytes<NN, DD>();
  MTG_DL_LDS(10, 1) MTG_DL_LDS(10, 2) MTG_DL_LDS(10, 3) MTG_DL_LDS(10, 4)
  MTG_DL_LDS(12, 1) MTG_DL_LDS(12, 2) MTG_DL_LDS(12, 3) MTG_DL_LDS(12, 4)
#undef MTG_DL_LDS
  return lds > 0 && lds <= kMaxLdsHard;
}

hipError_t launch_solve_dl(int N, const SolveArgs& a, hipStream_t stream) {
  if (!dl_geometry(N, a.D, a.K, a.r)) return hipErrorInvalidValue;
#define MTG_DL_CASE(NN, DD) \
  if (N == NN && a.D == DD) return launch_solve_dl_n##NN##_d##DD(a, stream);
  MTG_DL_CASE(10, 1) MTG_DL_CASE(10, 2) MTG_DL_CASE(10, 3) MTG_DL_CASE(10, 4)
  MTG_DL_CASE(12, 1) MTG_DL_CASE(12, 2) MTG_DL_CASE(12, 3) MTG_DL_CASE(12, 4)
#undef MTG_DL_CASE
  return hipErrorInvalidValue;
}

}  // namespace mtg

// The hot header (DlHot, 64 bytes into `out`) the launcher fills for a launch of these arguments: a
// host-only hook for the tests (tests/test_dl_header.py), not part of the C ABI (include/mtg.h).
// Returns 0, or -1 where the DL kernel does not serve the shape.
extern "C" int mtgtest_dl_hot_header(int N, int D, int K, int r, const void* values, const void* mask, const void* times,
                                     void* coeffs, const void* scales, int64_t B, int n_cand, int any_optional,
                                     void* out) {
  using namespace mtg;
  if (!dl_geometry(N, D, K, r) || B < 1) return -1;
  SolveArgs a{};
  a.values = static_cast<const double*>(values);
  a.mask = static_cast<const uint8_t*>(mask);
  a.times = static_cast<const double*>(times);
  a.coeffs = static_cast<double*>(coeffs);
  a.scales = static_cast<const double*>(scales);
  static int32_t dummy_status;  // (the fill only tests the optional outputs against null)
  a.status = any_optional ? &dummy_status : nullptr;
  a.B = B;
  a.K = K;
  a.D = D;
  a.r = r;
  a.n_cand = n_cand;
  const int tpw = kBlock / (2 * D);  // DlShape::TPW
  DlHot h;
  if (!dl_fill_hot(N, K, D, tpw, a, &h)) return -1;
  *static_cast<DlHot*>(out) = h;  // (the caller's buffer: 64 bytes, 8-byte aligned)
  return 0;
}
