// ovl_plan_check: canu_amd/csrc/ovl_plan.h (the search's and the driver's arithmetic) against
// hand-computed values.  A program of its own, built with AddressSanitizer and UBSan by
// tests/test_host.py; prints "ovl_plan_check ok" and exits 0 when every check holds.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../canu_amd/csrc/ovl_plan.h"

using namespace ovl;

static int g_bad = 0;
#define CHECK(x)                                                         \
  do {                                                                   \
    if (!(x)) {                                                          \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x);              \
      g_bad++;                                                           \
    }                                                                    \
  } while (0)

static void check_take_within() {
  uint64_t sum = 99;
  // a first item larger than the budget is still taken, alone
  const std::vector<uint64_t> big{10, 1, 1};
  CHECK(take_within(big, 0, 3, 5, &sum) == 1 && sum == 10);
  CHECK(take_within(big, 1, 3, 5, &sum) == 3 && sum == 2);
  // an exact fit includes the item, one over excludes it
  const std::vector<uint64_t> w{3, 4, 5};
  CHECK(take_within(w, 0, 3, 7, &sum) == 2 && sum == 7);
  CHECK(take_within(w, 0, 3, 6, &sum) == 1 && sum == 3);
  CHECK(take_within(w, 0, 3, 12, &sum) == 3 && sum == 12);
  // 32-bit weights whose sum passes 2^32: 2 x 0xFFFFFFFF = 8589934590 <= 2^33 < 3 x 0xFFFFFFFF
  const uint32_t m[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  CHECK(take_within(m, 0, 3, 1ull << 33, &sum) == 2 && sum == 8589934590ull);
  CHECK(take_within(m, 0, 3, 12884901885ull, &sum) == 3 && sum == 12884901885ull);
  CHECK(take_within(m, 0, 3, 12884901884ull, &sum) == 2);
  // an empty range returns from
  CHECK(take_within(w, 2, 2, 100, &sum) == 2 && sum == 0);
  CHECK(take_within(w, 3, 3, 100) == 3);
}

static void check_query_rule() {
  //                        id: 10   11  12   13  14  15
  const uint32_t len[6] = {100, 15, 30, 500, 18, 18};
  const uint32_t lib[6] = {1, 1, 2, 1, 3, 1};
  QueryRule Q;
  Q.len = len;
  Q.lib = lib;
  Q.first_iid = 10;
  Q.min_olap_len = 16;
  Q.k = 22;
  Q.lib_lo = 1;
  Q.lib_hi = 2;
  CHECK(Q.is_ref(10) && Q.windows(10) == 79);      // 100 - 22 + 1
  CHECK(!Q.is_ref(11) && Q.windows(11) == 0);      // shorter than --minlength
  CHECK(Q.is_ref(12) && Q.windows(12) == 9);
  CHECK(Q.is_ref(13) && Q.windows(13) == 479);
  CHECK(!Q.is_ref(14) && Q.windows(14) == 0);      // library 3, outside [1, 2]: neither
  CHECK(Q.is_ref(15) && Q.windows(15) == 0);       // min_olap_len <= L < k: a ref read, no unit
  uint64_t refs = 0, visited = 0;
  std::vector<uint32_t> unit_ids;
  std::vector<uint64_t> unit_win;
  Q.each(10, 15, [&](uint32_t a, bool ref, uint64_t w) {
    visited++;
    refs += ref;
    if (w) { unit_ids.push_back(a); unit_win.push_back(w); }
  });
  CHECK(visited == 6 && refs == 4);
  CHECK((unit_ids == std::vector<uint32_t>{10, 12, 13}));
  CHECK((unit_win == std::vector<uint64_t>{79, 9, 479}));
  // a sub-range, and an empty one (end < bgn)
  refs = 0;
  Q.each(11, 12, [&](uint32_t, bool ref, uint64_t) { refs += ref; });
  CHECK(refs == 1);
  visited = 0;
  Q.each(13, 12, [&](uint32_t, bool, uint64_t) { visited++; });
  CHECK(visited == 0);
  // a null library array means library 0
  Q.lib = nullptr;
  CHECK(!Q.is_ref(10) && Q.windows(10) == 0);      // library 0 is outside [1, 2]
  Q.lib_lo = 0;
  Q.lib_hi = 0;
  CHECK(Q.is_ref(10) && Q.windows(10) == 79);
  CHECK(Q.is_ref(14) && Q.windows(14) == 0);
  refs = 0;
  Q.each(10, 15, [&](uint32_t, bool ref, uint64_t) { refs += ref; });
  CHECK(refs == 5);
  // end = UINT32_MAX terminates: the last three read IDs
  const uint32_t len3[3] = {40, 40, 41};
  QueryRule T;
  T.len = len3;
  T.first_iid = UINT32_MAX - 2;
  T.k = 22;
  visited = 0;
  uint64_t wsum = 0;
  T.each(UINT32_MAX - 2, UINT32_MAX, [&](uint32_t, bool, uint64_t w) { visited++; wsum += w; });
  CHECK(visited == 3 && wsum == 19 + 19 + 20);
}

static bool live_is_exact(const ChainPlan &P, const uint32_t *uh) {
  std::vector<uint32_t> want;
  for (uint32_t i = 0; i < P.nc; i++)
    if (uh[i] > 0) want.push_back(i);
  for (uint32_t i : P.live)
    if (i >= P.nc) return false;
  return P.live == want;
}

static void check_plan_chain() {
  // case A: 100 windows per unit; per_unit 2, 4 chain waves, node blocks of 16
  const uint32_t uh[8] = {5, 0, 7, 0, 0, 9, 3, 0};
  uint64_t rbase[9];
  for (int i = 0; i <= 8; i++) rbase[i] = 100ull * i;
  ChainPlan A = plan_chain(uh, 8, rbase, 24, 2, 4, 16, 1ull << 30);
  CHECK(A.nc == 8 && A.hsum == 24);
  CHECK((A.live == std::vector<uint32_t>{0, 2, 5, 6}) && live_is_exact(A, uh) && !A.all_live());
  CHECK(A.pnodes_cap == 25);
  CHECK(A.pairs_cap == 25);                        // min(24 + 1, 8 * 2 + 1024)
  CHECK(A.pool_cap == 24 + 0 + 6 * 16 + 8);
  CHECK(A.win_budget == 16ull << 20);              // 24 / (24 / 800) * 1.05 = 840: the floor
  // the budget halved, as the out-of-memory retry does: 5 + 0 + 7 + 0 + 0 = 12, then 9 is over
  ChainPlan H = plan_chain(uh, 8, rbase, A.hsum / 2, 2, 4, 16, 1ull << 30);
  CHECK(H.nc == 5 && H.nc < A.nc && H.hsum == 12);
  CHECK((H.live == std::vector<uint32_t>{0, 2}) && live_is_exact(H, uh));
  CHECK(H.pnodes_cap == H.hsum + 1);
  CHECK(H.pairs_cap == std::min<uint64_t>(H.hsum + 1, (uint64_t)H.nc * 2 + 1024));
  CHECK(H.pairs_cap == 13 && H.pool_cap == 12 + 0 + 96 + 8);
  // the per-unit side of pairs_cap, and hits / 32 in the pool
  const uint32_t many[2] = {4000, 4000};
  ChainPlan D = plan_chain(many, 2, rbase, 10000, 1, 4, 16, 1ull << 30);
  CHECK(D.nc == 2 && D.hsum == 8000 && D.all_live());
  CHECK(D.pairs_cap == 2 * 1 + 1024 && D.pnodes_cap == 8001 && D.pool_cap == 8000 + 250 + 96 + 8);
  // the window budget: 1e9 / (8000 / 200) * 1.05 = 26.25 M, and the cap
  D = plan_chain(many, 2, rbase, 1000000000, 1, 4, 16, 1ull << 30);
  CHECK(D.win_budget == 26250000);
  D = plan_chain(many, 2, rbase, 1000000000, 1, 4, 16, 20ull << 20);
  CHECK(D.win_budget == 20ull << 20);
  // the floor as a parameter, at 1 (the tests' window-budget knob): 10000 / (8000 / 200) * 1.05
  // = 262.5 windows, far below 16 M; a cap below that still binds; nothing else moves
  ChainPlan F = plan_chain(many, 2, rbase, 10000, 1, 4, 16, 1ull << 30, 1);
  CHECK(F.win_budget == 262);
  CHECK(F.nc == 2 && F.hsum == 8000 && F.all_live() && F.pairs_cap == 1026 && F.pnodes_cap == 8001);
  F = plan_chain(many, 2, rbase, 10000, 1, 4, 16, 100, 1);
  CHECK(F.win_budget == 100);
  F = plan_chain(many, 2, rbase, 1, 1, 4, 16, 100, 1);            // 1 / 40 * 1.05 < 1: the floor
  CHECK(F.nc == 1 && F.win_budget == 1);
  F = plan_chain(uh, 8, rbase, 24, 2, 4, 16, 1ull << 30, 1);      // case A: 840, give or take
  CHECK(F.win_budget >= 839 && F.win_budget <= 840 && F.win_budget <= (1ull << 30));
  // the default floor: the values as before (case A's 16 M, D's 26.25 M), named or left out
  CHECK(WIN_FLOOR == 16ull << 20);
  F = plan_chain(many, 2, rbase, 10000, 1, 4, 16, 1ull << 30);
  CHECK(F.win_budget == 16ull << 20);
  F = plan_chain(many, 2, rbase, 10000, 1, 4, 16, 1ull << 30, WIN_FLOOR);
  CHECK(F.win_budget == 16ull << 20);
  F = plan_chain(many, 2, rbase, 1000000000, 1, 4, 16, 1ull << 30, WIN_FLOOR);
  CHECK(F.win_budget == 26250000);
  F = plan_chain(many, 2, rbase, 10000, 1, 4, 16, 1ull << 20);    // a cap below the floor wins
  CHECK(F.win_budget == 1ull << 20);
  // case B: no hits at all
  const uint32_t zero[4] = {0, 0, 0, 0};
  ChainPlan B = plan_chain(zero, 4, rbase, 10, 2, 4, 16, 1ull << 30);
  CHECK(B.nc == 4 && B.live.empty() && B.hsum == 0 && !B.all_live());
  // case C: a single unit over the budget
  const uint32_t over[2] = {100, 1};
  ChainPlan C = plan_chain(over, 2, rbase, 10, 2, 4, 16, 1ull << 30);
  CHECK(C.nc == 1 && C.hsum == 100 && (C.live == std::vector<uint32_t>{0}) && C.all_live());
}

static void check_hash_rule() {
  // check_query_rule's table, read as hash reads: -H 1-2
  //                        id: 10   11  12   13  14  15
  const uint32_t len[6] = {100, 15, 30, 500, 18, 18};
  const uint32_t lib[6] = {1, 1, 2, 1, 3, 1};
  HashRule H;
  H.len = len;
  H.lib = lib;
  H.first_iid = 10;
  H.min_olap_len = 16;
  H.k = 22;
  H.lib_lo = 1;
  H.lib_hi = 2;
  CHECK(H.loadable(10) && H.windows(10) == 79);
  CHECK(!H.loadable(11) && H.windows(11) == 0);    // shorter than --minlength
  CHECK(H.loadable(12) && H.windows(12) == 9);
  CHECK(H.loadable(13) && H.windows(13) == 479);
  CHECK(!H.loadable(14) && H.windows(14) == 0);    // library 3
  CHECK(H.loadable(15) && H.windows(15) == 0);     // loaded (a string, 19 bases), no k-mer
  uint64_t visited = 0, loaded = 0, wsum = 0;
  H.each(10, 15, [&](uint32_t, bool l, uint64_t w) { visited++; loaded += l; wsum += w; });
  CHECK(visited == 6 && loaded == 4 && wsum == 79 + 9 + 479);
  CHECK(hash_windows(H, 10, 15) == 567 && hash_windows(H, 11, 12) == 9 && hash_windows(H, 13, 12) == 0);
  CHECK(hash_alloc_bases(H, 10, 15) == 101 + 31 + 501 + 19);
  // the :523 refusal: at exactly the limit + one maximal read, not one below
  CHECK(hash_alloc_refused(652, 152, 500) && !hash_alloc_refused(651, 152, 500));
  // a null library array means library 0
  H.lib = nullptr;
  CHECK(!H.loadable(10) && hash_windows(H, 10, 15) == 0 && hash_alloc_bases(H, 10, 15) == 0);
  H.lib_lo = 0;
  H.lib_hi = UINT32_MAX;
  CHECK(H.loadable(14) && hash_windows(H, 10, 15) == 567);
  CHECK(hash_alloc_bases(H, 10, 15) == 652 + 19);
  // end = UINT32_MAX terminates
  const uint32_t len3[3] = {40, 40, 41};
  HashRule T;
  T.len = len3;
  T.first_iid = UINT32_MAX - 2;
  T.k = 22;
  visited = 0;
  T.each(UINT32_MAX - 2, UINT32_MAX, [&](uint32_t, bool, uint64_t) { visited++; });
  CHECK(visited == 3 && hash_windows(T, UINT32_MAX - 2, UINT32_MAX) == 19 + 19 + 20);
  CHECK(hash_alloc_bases(T, UINT32_MAX - 1, UINT32_MAX) == 41 + 42);
}

static void check_ref_schedule() {
  // 18 reads, T 1: per = 1 + 18 / 1 / 8 = 3, 18 % 3 == 0: a block starts on 19, not searched
  RefSchedule S = ref_schedule(1, 19, 1);
  CHECK(S.any && S.last == 18);
  // 16 reads: per = 3, 16 % 3 = 1: the last block starts on 16 and reaches 17
  S = ref_schedule(1, 17, 1);
  CHECK(S.any && S.last == 17);
  // T = 0 counts as one thread
  S = ref_schedule(1, 19, 0);
  CHECK(S.any && S.last == 18);
  // 40 reads, T 2: per = 1 + 40 / 2 / 8 = 3, 40 % 3 = 1
  S = ref_schedule(1, 41, 2);
  CHECK(S.any && S.last == 41);
  // T 4: per = 1 + 18 / 4 / 8 = 1: every range is whole blocks
  S = ref_schedule(1, 19, 4);
  CHECK(S.any && S.last == 18);
  // bgn == end and bgn > end: no ref read
  CHECK(!ref_schedule(5, 5, 1).any && !ref_schedule(6, 5, 8).any);
}

static void check_hash_stop() {
  // 0.6 x 2^22 x 21 = 52848230.4; 0.75 x 2^23 x 21 exactly
  CHECK(hash_entry_limit(0.6, 22) == 52848230ull);
  CHECK(hash_entry_limit(0.75, 23) == 132120576ull);
  //                     id:  1   2   3    4   5   6      read 3 is shorter than --minlength
  const uint32_t len[6] = {100, 50, 10, 200, 80, 60};
  HashRule H;
  H.len = len;
  H.first_iid = 1;
  H.min_olap_len = 16;
  H.k = 22;                                        // windows 79 29 0 179 59 39
  // strings bind first: three IDs, the skipped read 3 among them
  HashStop S = hash_stop(H, 1, 6, 3, 10000);
  CHECK(S.e == 3 && S.total == 101 + 51 && S.windows == 108);
  // bases bind first: 152 reached with read 2; at 153 reads 3 (nothing) and 4 are loaded too
  S = hash_stop(H, 1, 6, 100, 152);
  CHECK(S.e == 2 && S.total == 152 && S.windows == 108);
  S = hash_stop(H, 1, 6, 100, 153);
  CHECK(S.e == 4 && S.total == 353 && S.windows == 287);
  // neither: the whole range
  S = hash_stop(H, 1, 6, 100, 10000);
  CHECK(S.e == 6 && S.total == 495 && S.windows == 385);
  // the range's end comes before the string test of its last read
  S = hash_stop(H, 1, 6, 6, 10000);
  CHECK(S.e == 6 && S.windows == 385);
  S = hash_stop(H, 1, 6, 5, 10000);
  CHECK(S.e == 5 && S.total == 434 && S.windows == 346);
  S = hash_stop(H, 4, 4, 1, 1);
  CHECK(S.e == 4 && S.total == 201 && S.windows == 179);

  // the first build's prefix
  CHECK(first_build_target(10000000, 1000000, 0) == 2000000);
  CHECK(first_build_target(10000000, 100, 0) == 1048576);            // the 2^20 floor
  CHECK(first_build_target(500, 100, 0) == 500);                     // the batch itself
  CHECK(first_build_target(10000000, 1000000, 8000000) == 9000000);  // hint + hint / 8
  CHECK(first_build_target(10000000, 1000000, 16) == 1048576);
  CHECK(doubled_build_target(10000000, 3000000) == 6000000);
  CHECK(doubled_build_target(10000000, 6000000) == 10000000);
  CHECK(prefix_end(H, 1, 6, 108) == 3);            // 79 + 29, and read 3 adds nothing
  CHECK(prefix_end(H, 1, 6, 107) == 1);
  CHECK(prefix_end(H, 1, 6, 10) == 1);             // a first read larger than the target, alone
  CHECK(prefix_end(H, 4, 6, 100) == 4);
  CHECK(prefix_end(H, 1, 6, 385) == 6 && prefix_end(H, 1, 6, 1000) == 6);
  CHECK(prefix_end(H, 1, 6, 384) == 5);

  // the load cut over first-occurrence counts
  const uint32_t first[4] = {5, 0, 7, 3};
  CHECK(load_cut(first, 4, 5) == 0);               // hit on the first read
  CHECK(load_cut(first, 4, 6) == 2);
  CHECK(load_cut(first, 4, 15) == 3);              // hit on the last
  CHECK(load_cut(first, 4, 16) == 4);              // not reached
  CHECK(load_cut(first, 0, 1) == 0);
  CHECK(hash_windows(H, 1, 1 + load_cut(first, 4, 15)) == 287);   // the cut range's windows
}

using Ranges = std::vector<IidRange>;

static void check_super_batches() {
  // cap 60: 30 + 30 joined; 100 stands alone; 20 + 20 joined behind it
  const Ranges bat{{1, 10}, {11, 20}, {21, 30}, {31, 40}, {41, 50}};
  SuperBatches S = pack_super_batches(bat, {30, 30, 100, 20, 20}, 60);
  CHECK((S.sbs == Ranges{{1, 20}, {21, 30}, {31, 50}}) && S.max_windows == 100);
  S = pack_super_batches(bat, {30, 30, 100, 20, 20}, 59);
  CHECK((S.sbs == Ranges{{1, 10}, {11, 20}, {21, 30}, {31, 50}}) && S.max_windows == 100);
  S = pack_super_batches(bat, {30, 30, 100, 20, 20}, 1000);
  CHECK((S.sbs == Ranges{{1, 50}}) && S.max_windows == 200);
  S = pack_super_batches({}, {}, 60);
  CHECK(S.sbs.empty() && S.max_windows == 0);

  // 3 chunks x 4 super-batches; the second chunk starts past the first two super-batches
  const Ranges sbs{{1, 100}, {101, 200}, {201, 300}, {301, 400}};
  const Ranges chunks{{1, 150}, {250, 320}, {321, 399}};
  CHECK(searches_of(sbs, 1) == 4 && searches_of(sbs, 250) == 2 && searches_of(sbs, 321) == 1);
  CHECK(searches_of(sbs, 399) == 1 && searches_of(sbs, 400) == 0);
  const std::vector<std::pair<size_t, size_t>> want{{0, 0}, {0, 1}, {0, 2}, {0, 3},
                                                    {1, 3}, {1, 2},          // reversed
                                                    {2, 3}};
  CHECK(search_order(chunks, sbs) == want);
  CHECK(search_order({}, sbs).empty() && search_order(chunks, {}).empty());
}

static void check_query_chunks() {
  //                        id: 10   11  12   13  14  15     2 x windows: 158 0 18 958 0 0
  const uint32_t len[6] = {100, 15, 30, 500, 18, 18};
  QueryRule Q;
  Q.len = len;
  Q.first_iid = 10;
  Q.min_olap_len = 16;
  Q.k = 22;
  uint64_t mx = 0;
  // 158 + 0 + 18 fit 200, read 13 does not; behind it every read finds the chunk over the cap
  CHECK((cut_query_chunks(Q, 10, 15, 200, &mx) == Ranges{{10, 12}, {13, 13}, {14, 15}}) && mx == 958);
  // a cap smaller than one read: every read with windows alone
  mx = 0;
  CHECK((cut_query_chunks(Q, 10, 15, 1, &mx) ==
         Ranges{{10, 10}, {11, 11}, {12, 12}, {13, 13}, {14, 15}}) && mx == 958);
  mx = 0;
  CHECK((cut_query_chunks(Q, 10, 15, 10000, &mx) == Ranges{{10, 15}}) && mx == 1134);
  // the largest chunk is only ever raised
  mx = 2000;
  CHECK(cut_query_chunks(Q, 12, 13, 10000, &mx).size() == 1 && mx == 2000);
  mx = 7;
  CHECK(cut_query_chunks(Q, 13, 12, 200, &mx).empty() && mx == 7);
}

static void check_sq_layout() {
  // runs of <= 1024 windows: 512 + 300 + 212 fill the first exactly; unit 0 ends on the edge
  // of the first 512-window block, so block 1 starts in unit 1
  const SqLayout L = sq_layout({512, 300, 212, 600, 100}, 1024);
  CHECK(L.runs.size() == 2 && L.total == 1724 && L.maxrun == 1024);
  const SqRun &A = L.runs[0], &B = L.runs[1];
  CHECK(A.u0 == 0 && A.u1 == 3 && A.e0 == 0 && A.n == 1024 && A.wb0 == 0 && A.ub0 == 0);
  CHECK(B.u0 == 3 && B.u1 == 5 && B.e0 == 1024 && B.n == 700 && B.wb0 == 4 && B.ub0 == 2);
  CHECK((L.wb == std::vector<uint64_t>{0, 512, 812, 1024, 0, 600, 700}));
  CHECK((L.ublk == std::vector<uint32_t>{0, 1, 0, 0}));
  // a unit larger than a run is a run of its own; no units, no runs
  const SqLayout M = sq_layout({2000, 10}, 1024);
  CHECK(M.runs.size() == 2 && M.runs[0].n == 2000 && M.runs[1].e0 == 2000 && M.maxrun == 2000);
  CHECK((M.ublk == std::vector<uint32_t>{0, 0, 0, 0, 0}) && M.runs[1].ub0 == 4);
  CHECK(sq_layout({}, 1024).runs.empty());
}

static void check_index_shapes() {
  CHECK(ceil_log2(0) == 0 && ceil_log2(1) == 0 && ceil_log2(2) == 1 && ceil_log2(3) == 2);
  CHECK(ceil_log2(4096) == 12 && ceil_log2(4097) == 13);
  IndexShape X = index_shape(0);
  CHECK(X.cb == 4 && X.per_cb == 1 && X.fb == 0 && X.nfine == 16 && X.cap == 64);
  // 2048: cb = max(4, log2(2)); per_cb 129; 2 fine buckets of mean 65: cap 256 >= 130
  X = index_shape(2048);
  CHECK(X.cb == 4 && X.per_cb == 129 && X.fb == 1 && X.nfine == 32 && X.cap == 256);
  // the largest count build_index takes: both exponents and the sort capacity at their caps
  const IndexShape Z = index_shape(0xFFFFFFEFull);
  CHECK(Z.cb == 12 && Z.per_cb == 1048576 && Z.fb == 11 && Z.nfine == 8388608 && Z.cap == 1024);

  // tables over the P = 2048 shape (cb + fb = 5, 32 fine buckets)
  // 2 x 100 + 1 = 201 slots -> 2^8, 4 KB per wave, 4 waves per block
  TableShape T = table_shape(X, 100, false, 2000, false);
  CHECK(T.slice_bits == 8 && T.tab_bits == 13 && !T.bloom && !T.refused && T.wpb == 4 && T.lds == 16384);
  // dense: 100 + 1 slots -> 2^7
  T = table_shape(X, 100, true, 2000, false);
  CHECK(T.slice_bits == 7 && T.tab_bits == 12 && !T.refused && T.wpb == 4 && T.lds == 8192);
  // the filter: (8 x 2000 + 2047) / 2048 = 8 words per bucket -> 2^3, 64 B beside the slice
  T = table_shape(X, 100, false, 2000, true);
  CHECK(T.bloom && T.bloom_w == 3 && T.slice_bits == 8 && T.wpb == 4 && T.lds == 4 * (4096 + 64));
  T = table_shape(X, 100, false, 100000, true);    // 391 words: capped at 2^6
  CHECK(T.bloom && T.bloom_w == 6 && T.lds == 4 * (4096 + 512));
  // 2 x 1023 + 1 = 2047 slots -> 2^11 = 32 KB: filter kept, one wave per block
  T = table_shape(X, 1023, false, 2000, true);
  CHECK(T.slice_bits == 11 && T.bloom && !T.refused && T.wpb == 1 && T.lds == 32768 + 64);
  // 2 x 2047 + 1 = 4095 -> 2^12 = 64 KB: the slice fills the wave's LDS, the filter is dropped
  T = table_shape(X, 2047, false, 2000, true);
  CHECK(T.slice_bits == 12 && !T.bloom && T.bloom_w == 3 && !T.refused && T.wpb == 1 && T.lds == 65536);
  T = table_shape(X, 2047, false, 2000, false);
  CHECK(T.slice_bits == 12 && !T.bloom && !T.refused && T.lds == 65536);
  // 2 x 2048 + 1 = 4097 -> 2^13: refused, with or without the filter; dense it still fits
  CHECK(table_shape(X, 2048, false, 2000, false).refused && table_shape(X, 2048, false, 2000, true).refused);
  T = table_shape(X, 2048, true, 2000, false);
  CHECK(T.slice_bits == 12 && !T.refused);
  // no k-mer at all counts as one: 3 slots -> 2^2, dense 2 -> 2^1
  CHECK(table_shape(X, 0, false, 0, false).slice_bits == 2 && table_shape(X, 0, true, 0, false).slice_bits == 1);
  CHECK(table_shape(Z, 100, false, 2000, false).tab_bits == 12 + 11 + 8);
}

int main() {
  check_take_within();
  check_query_rule();
  check_plan_chain();
  check_hash_rule();
  check_ref_schedule();
  check_hash_stop();
  check_super_batches();
  check_query_chunks();
  check_sq_layout();
  check_index_shapes();
  if (g_bad) return 1;
  printf("ovl_plan_check ok\n");
  return 0;
}
