// The plan of a ragged solve (mtg_solve_linear_ragged_batch, mtg_host_solve_linear_ragged_batch,
// mtg_solve_ragged_plan): CSR offsets of the batch and its groups.  Host code only, no device work.
// Plain C++ (no HIP): the host sources are also built on their own.
//
// Trajectory b has K_b = seg_count[b] segments and V_b = K_b + 1 vertices; vo[b] = sum_{j<b} V_j and
// so[b] = sum_{j<b} K_j = vo[b] - b.  A group is all trajectories with one K.  A group whose members
// are consecutive in the batch is solved in place, on slices of the caller's arrays; every other group
// is gathered into packed arrays.  The gathered trajectories, ordered by (K, position in the batch),
// form a CSR batch of their own (`members`, with vertex offsets pvo): each gathered group is a run of
// it, so the packed arrays of a group are a slice of one packed array per kind.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "mtg.h"

namespace mtg {

struct RaggedGroup {
  int K;
  int64_t count;
  int64_t first;    // in place: the batch index of the first member; gathered: the index into members
  bool in_place;
};

struct RaggedPlan {
  std::vector<int64_t> vo;        // [B + 1] vertex offsets (so[b] = vo[b] - b)
  std::vector<RaggedGroup> groups;  // ascending K
  std::vector<int64_t> members;   // gathered trajectories, group after group, each in batch order
  std::vector<int64_t> pvo;       // [members + 1] vertex offsets of the packed arrays
  int64_t n_in_place = 0;
  int64_t so(int64_t b) const { return vo[(size_t)b] - b; }
  int64_t pso(int64_t j) const { return pvo[(size_t)j] - j; }
  int64_t total_vertices() const { return vo.back(); }
  int64_t total_segments() const { return vo.back() - (int64_t)(vo.size() - 1); }
};

// MTG_OK, or MTG_ERR_SIZE_MISMATCH for a seg_count below 1 (nothing else is checked here)
inline int ragged_plan(int64_t batch, const int32_t* seg_count, RaggedPlan* plan) {
  RaggedPlan& p = *plan;
  p = RaggedPlan{};
  p.vo.assign((size_t)batch + 1, 0);
  for (int64_t b = 0; b < batch; ++b) {
    if (seg_count[b] < 1) return MTG_ERR_SIZE_MISMATCH;
    p.vo[(size_t)b + 1] = p.vo[(size_t)b] + seg_count[b] + 1;
  }
  // the distinct K, ascending; per K its count and the first and last member
  std::vector<int32_t> ks(seg_count, seg_count + batch);
  std::sort(ks.begin(), ks.end());
  ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
  const size_t G = ks.size();
  std::vector<int64_t> count(G, 0), first(G, 0), last(G, 0);
  std::vector<int32_t> group_of((size_t)batch);
  for (int64_t b = 0; b < batch; ++b) {
    const size_t g = (size_t)(std::lower_bound(ks.begin(), ks.end(), seg_count[b]) - ks.begin());
    group_of[(size_t)b] = (int32_t)g;
    if (count[g]++ == 0) first[g] = b;
    last[g] = b;
  }
  std::vector<int64_t> fill(G, 0);
  int64_t n_gathered = 0;
  p.groups.resize(G);
  for (size_t g = 0; g < G; ++g) {
    RaggedGroup& gr = p.groups[g];
    gr.K = ks[g];
    gr.count = count[g];
    gr.in_place = last[g] - first[g] + 1 == count[g];
    gr.first = gr.in_place ? first[g] : n_gathered;
    fill[g] = gr.first;
    if (gr.in_place) p.n_in_place += gr.count;
    else n_gathered += gr.count;
  }
  p.members.resize((size_t)n_gathered);
  for (int64_t b = 0; b < batch; ++b) {
    const size_t g = (size_t)group_of[(size_t)b];
    if (!p.groups[g].in_place) p.members[(size_t)fill[g]++] = b;
  }
  p.pvo.assign((size_t)n_gathered + 1, 0);
  for (int64_t j = 0; j < n_gathered; ++j)
    p.pvo[(size_t)j + 1] = p.pvo[(size_t)j] + seg_count[p.members[(size_t)j]] + 1;
  return MTG_OK;
}

}  // namespace mtg
