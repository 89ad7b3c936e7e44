// ovl_plan.h -- the search's batch arithmetic as plain host code (standard library only, so
// tests/ovl_plan_check.cpp runs it without a GPU): which reads are query reads and how many
// windows they have, the "as many as fit a budget, at least one" cut, and a chain launch's
// unit count, live list and buffer capacities.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace ovl {

// Which reads a search takes as queries (Process_Overlaps.C:108-114) and their windows.
struct QueryRule {
  const uint32_t *len = nullptr;   // read lengths, entry 0 is read first_iid
  const uint32_t *lib = nullptr;   // library IDs (-H / -R filters); null: every read in library 0
  uint32_t first_iid = 1;
  int32_t min_olap_len = 0;        // --minlength
  uint32_t k = 0;
  uint32_t lib_lo = 0, lib_hi = UINT32_MAX;

  // a ref read: in a wanted library (-R, :108) and at least --minlength long (:114); these are
  // what ovl_stats.ref_reads counts
  bool is_ref(uint32_t iid) const {
    const uint32_t r = iid - first_iid;
    const uint32_t l = lib ? lib[r] : 0;
    return l >= lib_lo && l <= lib_hi && (int64_t)len[r] >= (int64_t)min_olap_len;
  }
  // k-mer windows of a ref read in one orientation (a query unit); 0: the read gives no unit
  uint64_t windows(uint32_t iid) const {
    const uint32_t L = len[iid - first_iid];
    return is_ref(iid) && L >= k ? (uint64_t)(L - k + 1) : 0;
  }
  // f(iid, is_ref, windows) for every read of [bgn, end]; `a >= bgn` ends the loop when end is
  // UINT32_MAX and a wraps
  template <typename F>
  void each(uint32_t bgn, uint32_t end, F &&f) const {
    for (uint32_t a = bgn; a <= end && a >= bgn; a++) f(a, is_ref(a), windows(a));
  }
};

// The end of the longest run weights[from, to) with to <= n whose sum stays within budget --
// but at least one item, so that an item larger than the budget is still taken, alone.
// An empty range returns from.  *sum (optional) receives the run's sum.
template <typename W>
inline uint32_t take_within(const W &weights, uint32_t from, uint32_t n, uint64_t budget,
                            uint64_t *sum = nullptr) {
  uint32_t to = from;
  uint64_t s = 0;
  while (to < n && (s + (uint64_t)weights[to] <= budget || to == from)) s += (uint64_t)weights[to++];
  if (sum) *sum = s;
  return to;
}

// nodes <= hits; a wave claims node_block nodes at a time for at most 64 lanes per claim, so a
// block wastes < 64 / 4096 of itself, and each wave ends holding one block
inline uint64_t chain_pool_for(uint64_t hits, uint32_t chain_waves, uint32_t node_block) {
  return hits + hits / 32 + (uint64_t)(chain_waves + 2) * node_block + 8;
}

// One chain launch over a probed batch: its units, the ones with hits, the capacities.
struct ChainPlan {
  uint32_t nc = 0;               // the batch's first nc units are chained
  uint64_t hsum = 0;             // their seed hits
  // only units with hits are chained: a unit without one adds no pair, node, counter or
  // flag, yet its wave would read every window's record (a full-size configs[4] search
  // against a super-batch of ~2 % of the reads: about half its units)
  std::vector<uint32_t> live;    // {i < nc : uh[i] > 0}
  uint64_t pool_cap = 0, pairs_cap = 0, pnodes_cap = 0;
  uint64_t win_budget = 0;       // the next probe batch's windows
  bool all_live() const { return live.size() == nc; }
};

// The batch's units [0, nb) with uh[i] seed hits and windows [rbase[i], rbase[i + 1]) are cut to
// the hit budget (probe results stay valid for the prefix).  The next probe's window budget
// adapts to the hits-per-window ratio seen, so that a batch's probe results are all consumed
// (units beyond the hit budget would otherwise be re-probed).  Every value a chain launch needs
// comes from one call: after a budget change, plan again and use all of the new plan.
inline ChainPlan plan_chain(const uint32_t *uh, uint32_t nb, const uint64_t *rbase,
                            uint64_t hit_budget, uint64_t per_unit, uint32_t chain_waves,
                            uint32_t node_block, uint64_t win_cap) {
  ChainPlan P;
  P.nc = take_within(uh, 0, nb, hit_budget, &P.hsum);
  const double ratio = (double)P.hsum / (double)std::max<uint64_t>(1, rbase[P.nc]);
  const double wb = (double)hit_budget / std::max(ratio, 1e-3) * 1.05;
  P.win_budget = (uint64_t)std::min(std::max(wb, 16.0 * (1 << 20)), (double)win_cap);
  P.live.reserve(P.nc);
  for (uint32_t i = 0; i < P.nc; i++)
    if (uh[i]) P.live.push_back(i);
  P.pool_cap = chain_pool_for(P.hsum, chain_waves, node_block);
  P.pairs_cap = std::min<uint64_t>(P.hsum + 1, (uint64_t)P.nc * per_unit + 1024);
  P.pnodes_cap = P.hsum + 1;
  return P;
}

}  // namespace ovl
