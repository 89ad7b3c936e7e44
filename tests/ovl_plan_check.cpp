// ovl_plan_check: canu_amd/csrc/ovl_plan.h (the search's batch arithmetic) against
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
  // case B: no hits at all
  const uint32_t zero[4] = {0, 0, 0, 0};
  ChainPlan B = plan_chain(zero, 4, rbase, 10, 2, 4, 16, 1ull << 30);
  CHECK(B.nc == 4 && B.live.empty() && B.hsum == 0 && !B.all_live());
  // case C: a single unit over the budget
  const uint32_t over[2] = {100, 1};
  ChainPlan C = plan_chain(over, 2, rbase, 10, 2, 4, 16, 1ull << 30);
  CHECK(C.nc == 1 && C.hsum == 100 && (C.live == std::vector<uint32_t>{0}) && C.all_live());
}

int main() {
  check_take_within();
  check_query_rule();
  check_plan_chain();
  if (g_bad) return 1;
  printf("ovl_plan_check ok\n");
  return 0;
}
