// ovl_plan.h -- the search's and the driver's arithmetic as plain host code (standard library
// only, so tests/ovl_plan_check.cpp runs it without a GPU): which reads are query reads and
// which are hashed, and how many windows they have; the "as many as fit a budget, at least
// one" cut; a chain launch's unit count, live list and buffer capacities; and what the
// OverlapDriver job, the hash-batch builder, the index build and the sorted query windows
// decide from lengths and counts alone (batch ends, cuts, packing, orders, layouts, shapes).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
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
// win_floor: the fewest windows the next probe batch is given (below win_cap); the tests'
// window-budget knob lowers it to 1.
static const uint64_t WIN_FLOOR = 16ull << 20;
inline ChainPlan plan_chain(const uint32_t *uh, uint32_t nb, const uint64_t *rbase,
                            uint64_t hit_budget, uint64_t per_unit, uint32_t chain_waves,
                            uint32_t node_block, uint64_t win_cap, uint64_t win_floor = WIN_FLOOR) {
  ChainPlan P;
  P.nc = take_within(uh, 0, nb, hit_budget, &P.hsum);
  const double ratio = (double)P.hsum / (double)std::max<uint64_t>(1, rbase[P.nc]);
  const double wb = (double)hit_budget / std::max(ratio, 1e-3) * 1.05;
  P.win_budget = (uint64_t)std::min(std::max(wb, (double)win_floor), (double)win_cap);
  P.live.reserve(P.nc);
  for (uint32_t i = 0; i < P.nc; i++)
    if (uh[i]) P.live.push_back(i);
  P.pool_cap = chain_pool_for(P.hsum, chain_waves, node_block);
  P.pairs_cap = std::min<uint64_t>(P.hsum + 1, (uint64_t)P.nc * per_unit + 1024);
  P.pnodes_cap = P.hsum + 1;
  return P;
}

// ---- the hash side ------------------------------------------------------------------------

// Which reads a hash batch loads (Build_Hash_Index.C:495-523): the query rule's test with -H's
// libraries [min_lib_hash, max_lib_hash] in lib_lo / lib_hi.  each() calls
// f(iid, loadable, windows).
struct HashRule : QueryRule {
  bool loadable(uint32_t iid) const { return is_ref(iid); }
};

inline uint64_t hash_windows(const HashRule &H, uint32_t bgn, uint32_t end) {
  uint64_t w = 0;
  H.each(bgn, end, [&](uint32_t, bool, uint64_t win) { w += win; });
  return w;
}

using IidRange = std::pair<uint32_t, uint32_t>;    // reads first..second, inclusive

inline uint32_t ceil_log2(uint64_t x) {
  uint32_t b = 0;
  while ((1ull << b) < x) b++;
  return b;
}

// Process_Overlaps' block schedule (overlapInCore.C:249-269, Process_Overlaps.C:86-171):
// blocks of perThread reads from bgnRefID on, each searched only while it starts below
// endRefID -- the reads before endRefID always, endRefID itself unless a block starts on it.
struct RefSchedule {
  bool any = false;              // bgn < end: there are ref reads at all
  uint32_t last = 0;             // the last searched ref read
};
inline RefSchedule ref_schedule(uint32_t bgn_ref, uint32_t end_ref, uint32_t num_threads) {
  RefSchedule S;
  if (bgn_ref < end_ref) {
    const uint32_t T = std::max<uint32_t>(num_threads, 1);
    const uint32_t per = 1 + (end_ref - bgn_ref) / T / 8;
    S.last = ((end_ref - bgn_ref) % per == 0) ? end_ref - 1 : end_ref;
    S.any = true;
  }
  return S;
}

static const uint32_t ENTRIES_PER_BUCKET = 21;     // overlapInCore.H:102

// hash_entry_limit (Build_Hash_Index.C:489): the table-load stop, from --hashload and --hashbits
inline uint64_t hash_entry_limit(double max_hash_load, uint32_t hash_mask_bits) {
  return (uint64_t)(max_hash_load * (double)(1ull << hash_mask_bits) * (double)ENTRIES_PER_BUCKET);
}

// Build_Hash_Index.C:495-523 -- the allocation pass counts every loadable read up to endID
// (len + 1 each); the reference asserts when that exceeds the data limit by more than one
// maximal read
inline uint64_t hash_alloc_bases(const HashRule &H, uint32_t bgn, uint32_t end) {
  uint64_t n = 0;
  H.each(bgn, end, [&](uint32_t a, bool loadable, uint64_t) {
    if (loadable) n += H.len[a - H.first_iid] + 1;
  });
  return n;
}
inline bool hash_alloc_refused(uint64_t alloc_bases, uint64_t max_hash_data_len, uint64_t max_readlen) {
  return alloc_bases >= max_hash_data_len + max_readlen;
}

// Build_Hash_Index.C:525-541 -- before each read the loading loop requires String_Ct <
// Max_Hash_Strings and total_len < Max_Hash_Data_Len.  String_Ct counts every ID (skipped
// reads too); total_len grows by len + 1 per loaded read.  bgn <= end.
struct HashStop {
  uint32_t e = 0;                // the batch's last read by strings and bases
  uint64_t total = 0;            // bases loaded (len + 1 per loadable read)
  uint64_t windows = 0;          // windows of bgn..e
};
inline HashStop hash_stop(const HashRule &H, uint32_t bgn, uint32_t end, uint64_t max_hash_strings,
                          uint64_t max_hash_data_len) {
  HashStop S;
  S.e = end;
  for (uint32_t id = bgn;; id++) {
    if (H.loadable(id)) S.total += H.len[id - H.first_iid] + 1;
    S.windows += H.windows(id);
    if (id == end) break;
    if ((uint64_t)(id + 1 - bgn) >= max_hash_strings || S.total >= max_hash_data_len) {
      S.e = id;
      break;
    }
  }
  return S;
}

// When the table load may cut a batch, its first build covers a prefix of about twice the
// limit's windows (a read's new k-mers are at most its windows, so the cut lies past the
// limit's windows; typical reads bring 0.3-0.7 new k-mers per window).  Consecutive batches of
// one job cut at about the same number of windows, so after the first cut (hint: its windows)
// the prefix is the previous cut's windows + 1/8.  A prefix the load does not stop inside is
// doubled.
inline uint64_t first_build_target(uint64_t windows, uint64_t entry_limit, uint64_t hint) {
  const uint64_t want = hint ? hint + hint / 8 : 2 * entry_limit;
  return std::min<uint64_t>(windows, std::max<uint64_t>(want, 1u << 20));
}
inline uint64_t doubled_build_target(uint64_t windows, uint64_t built) {
  return std::min<uint64_t>(windows, 2 * built);
}
// the last read of the longest prefix of bgn..e within `target` windows, at least one read
inline uint32_t prefix_end(const HashRule &H, uint32_t bgn, uint32_t e, uint64_t target) {
  struct {
    const HashRule &H;
    uint32_t bgn;
    uint64_t operator[](uint32_t i) const { return H.windows(bgn + i); }
  } win{H, bgn};
  return bgn + take_within(win, 0, e - bgn + 1, target) - 1;
}

// Hash_Entries grows by the k-mers a read brings that no earlier read of the batch holds
// (first[i] of read bgn + i); the load stops the batch at the first read where it reaches the
// limit.  Returns that read's index, or nr when the limit is not reached.
inline uint32_t load_cut(const uint32_t *first, uint32_t nr, uint64_t entry_limit) {
  uint64_t entries = 0;
  for (uint32_t i = 0; i < nr; i++) {
    entries += first[i];
    if (entries >= entry_limit) return i;
  }
  return nr;
}

// Consecutive batches (bw: their windows) joined into super-batches of up to cap windows; a
// batch past the cap stands alone.
struct SuperBatches {
  std::vector<IidRange> sbs;
  uint64_t max_windows = 0;      // the largest one's windows
};
inline SuperBatches pack_super_batches(const std::vector<IidRange> &bat,
                                       const std::vector<uint64_t> &bw, uint64_t cap) {
  SuperBatches S;
  uint64_t w = 0;
  for (size_t i = 0; i < bat.size(); i++) {
    if (!S.sbs.empty() && w + bw[i] <= cap) {
      S.sbs.back().second = bat[i].second;
      w += bw[i];
    } else {
      S.sbs.push_back(bat[i]);
      w = bw[i];
    }
    S.max_windows = std::max(S.max_windows, w);
  }
  return S;
}

// searches of a query chunk starting at read qlo: a query meets only hashed reads with larger
// IDs (Find_Overlaps.C:328), so the super-batches whose last read lies past qlo
inline uint64_t searches_of(const std::vector<IidRange> &sbs, uint32_t qlo) {
  uint64_t n = 0;
  for (const auto &sb : sbs) n += qlo < sb.second ? 1 : 0;
  return n;
}
// (chunk, super-batch), the super-batches of every other chunk in reverse order: a chunk then
// starts with the index its predecessor ended on when both reach the last super-batch
inline std::vector<std::pair<size_t, size_t>> search_order(const std::vector<IidRange> &qchunks,
                                                           const std::vector<IidRange> &sbs) {
  std::vector<std::pair<size_t, size_t>> plan;
  for (size_t qi = 0; qi < qchunks.size(); qi++)
    for (size_t i = 0; i < sbs.size(); i++) {
      const size_t si = (qi & 1) ? sbs.size() - 1 - i : i;
      if (qchunks[qi].first < sbs[si].second) plan.push_back({qi, si});
    }
  return plan;
}

// The ref range bgn..end cut into consecutive chunks of at most wcap query windows (both
// orientations: 2 x windows per read), at least one read each.  *max_windows is raised to the
// largest chunk's windows.
inline std::vector<IidRange> cut_query_chunks(const QueryRule &Q, uint32_t bgn, uint32_t end,
                                              uint64_t wcap, uint64_t *max_windows) {
  std::vector<IidRange> out;
  uint32_t lo = bgn;
  uint64_t w = 0;
  Q.each(bgn, end, [&](uint32_t a, bool, uint64_t win) {
    const uint64_t add = 2 * win;
    if (w + add > wcap && a > lo) {
      out.push_back({lo, a - 1});
      *max_windows = std::max(*max_windows, w);
      lo = a;
      w = 0;
    }
    w += add;
  });
  if (end >= bgn) out.push_back({lo, end});
  *max_windows = std::max(*max_windows, w);
  return out;
}

// ---- the sorted query windows' layout -------------------------------------------------------
struct SqRun {
  uint32_t u0, u1;               // the run's units [u0, u1)
  uint64_t e0, n;                // its windows: entries [e0, e0 + n) of key / wid
  uint64_t wb0, ub0;             // offsets of its unit bases (n units + 1) and 512-window blocks
};
struct SqLayout {
  std::vector<SqRun> runs;       // consecutive units, <= run_size windows each (one unit at least)
  std::vector<uint64_t> wb;      // per unit + one per run: run-local first window
  std::vector<uint32_t> ublk;    // per run and 512-window block: the run-local unit its first window is in
  uint64_t total = 0, maxrun = 0;
};
inline SqLayout sq_layout(const std::vector<uint64_t> &uwin, uint64_t run_size) {
  SqLayout L;
  const uint32_t nu = (uint32_t)uwin.size();
  for (uint32_t u = 0; u < nu;) {
    SqRun R;
    R.u0 = u;
    R.e0 = L.total;
    R.u1 = u = take_within(uwin, u, nu, run_size, &R.n);
    R.wb0 = L.wb.size();
    uint64_t acc = 0;
    for (uint32_t x = R.u0; x < R.u1; x++) { L.wb.push_back(acc); acc += uwin[x]; }
    L.wb.push_back(acc);
    R.ub0 = L.ublk.size();
    uint32_t x = 0;
    for (uint64_t w = 0; w < R.n; w += 512) {
      while (L.wb[R.wb0 + x + 1] <= w) x++;
      L.ublk.push_back(x);
    }
    L.total += R.n;
    L.maxrun = std::max(L.maxrun, R.n);
    L.runs.push_back(R);
  }
  return L;
}

// ---- the index's shapes -----------------------------------------------------------------------
// From the record bound P (every window of the batch's reads + the skip k-mers): 2^cb coarse
// buckets of ~2048, 2^fb fine buckets of ~128 in each, and the per-wave sort buffer: twice the
// mean fine bucket, a power of 2, 64..1024 records.
struct IndexShape {
  uint32_t cb = 0, fb = 0, nfine = 0, cap = 0;
  uint64_t per_cb = 0;
};
inline IndexShape index_shape(uint64_t P) {
  IndexShape S;
  S.cb = std::min<uint32_t>(12, std::max<uint32_t>(4, ceil_log2(P / 2048 + 1)));
  S.per_cb = (P >> S.cb) + 1;
  S.fb = std::min<uint32_t>(11, ceil_log2((S.per_cb + 127) / 128));
  const uint32_t nfb = 1u << S.fb;
  S.nfine = (1u << S.cb) * nfb;
  const uint64_t mean = S.per_cb / nfb + 1;
  S.cap = 64;
  while (S.cap < 2 * mean && S.cap < 1024) S.cap <<= 1;
  return S;
}

#ifndef OVL_SLICE_Q
#define OVL_SLICE_Q 8
#endif
// The table: one slice per fine bucket, built by one wave in LDS (k_table).
// Slots per slice >= OVL_SLICE_Q / 4 x the largest fine bucket's distinct k-mers (and always
// more than it, so every probe sequence meets an empty slot).  2x: a denser table (1.25x /
// 1.5x: 16 -> 8 GB at 50k x 10 kb) builds 1.5 ms faster but lengthens the probe sequences,
// +2.7 ms in k_probe.  Slices sized to their OWN bucket (2 x distinct + 1, ~6 GB) were
// measured in round 3 too: k_probe 12.4 -> 22.2 ms per launch, since the per-slice
// {base, size} lookup is a second dependent random access per window
// (profiles/r03d_bench_perslice.json); not kept.  dense (ovl_ctx::dense_tables): 1x.
// The filter: ~8 bits per indexed window (>= distinct k-mers) in every fine bucket's region, a
// power of two of 64-bit words, at most 64: ~130 MB for a batch of canu's --hashbits 23
// --hashload 0.75.
// LDS per wave: its slice and, with the filter, its fine bucket's filter region.  A slice
// whose wave does not fit 64 KB with the filter is built without it (the filter is only a
// shortcut in front of the table); without it, it is refused.
struct TableShape {
  uint32_t slice_bits = 0, tab_bits = 0;
  uint32_t bloom_w = 0;          // the filter's word exponent as requested (allocated even if dropped)
  bool bloom = false;            // the filter is built
  bool refused = false;          // the slice alone passes 64 KB
  uint32_t wpb = 0;              // k_table: waves per block
  size_t lds = 0;                // ... and its LDS bytes
};
inline TableShape table_shape(const IndexShape &X, uint32_t max_distinct, bool dense,
                              uint64_t records, bool bloom) {
  TableShape T;
  const uint64_t maxd = std::max<uint32_t>(max_distinct, 1);
  const uint64_t slice_q = dense ? 4 : OVL_SLICE_Q;
  T.slice_bits = std::max<uint32_t>(1, ceil_log2(slice_q * maxd / 4 + 1));
  T.tab_bits = X.cb + X.fb + T.slice_bits;
  if (bloom) {
    const uint64_t words = (8ull * records + 64ull * X.nfine - 1) / (64ull * X.nfine);
    while (T.bloom_w < 6 && (1ull << T.bloom_w) < words) T.bloom_w++;
  }
  const uint64_t slice = 16ull << T.slice_bits;
  T.bloom = bloom && slice + (8ull << T.bloom_w) <= 65536;
  const uint64_t per_wave = slice + (T.bloom ? 8ull << T.bloom_w : 0ull);
  T.refused = per_wave > 65536;
  T.wpb = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(4, 65536ull / per_wave));
  T.lds = (size_t)T.wpb * per_wave;
  return T;
}

}  // namespace ovl
