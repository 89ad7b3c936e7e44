// ped_host.h -- the host side of Prefix_Edit_Dist that overlapInCore (ovl_api.hip), findErrors
// (fe.hip) and correctOverlaps (co.hip) share: Edit_Match_Limit and the size of a wave's row
// log.  Plain C++, no HIP.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace ped {

constexpr uint32_t AS_MAX_READLEN = (1u << 21) - 1;

// Binomial_Bound.C:47
inline int binomial_bound(int e, double p, int start) {
  const double bound = 1e-4, thold = 3.62;
  const double q = 1.0 - p;
  if (start < e) start = e;
  for (int n = start; n < (int)AS_MAX_READLEN; n++) {
    if (n <= 35) {
      double sum = 0.0, p_pow = 1.0, q_pow = pow(q, n);
      int bin = 1, ct = 0;
      for (int k = 0; k < e && 1.0 - sum > bound; k++) {
        const double x = bin * p_pow * q_pow;
        sum += x;
        // the reference's int product overflows from n = 30 on (145422675 * 16); its tables
        // are what a product that wraps leaves, so wrap in unsigned arithmetic, where that is
        // defined
        bin = (int)((uint32_t)bin * (uint32_t)(n - ct));
        bin /= ++ct;
        p_pow *= p;
        q_pow /= q;
      }
      if (1.0 - sum > bound) return n;
    } else {
      const double z = (e - 0.5 - n * p) / sqrt(n * p * q);
      if (z <= thold) return n;
      double sum = 0.0, mu_pow = 1.0, fact = 1.0;
      const double pc = exp(-n * p);
      for (int k = 0; k < e; k++) {
        sum += mu_pow * pc / fact;
        mu_pow *= n * p;
        fact *= k + 1;
      }
      if (1.0 - sum > bound) return n;
    }
  }
  return AS_MAX_READLEN;
}

// Initialize_Match_Limit (Binomial_Bound.C:116) as prefixEditDistance.C:40-116,
// findErrors.C:472-474 and correctOverlaps.C:131-133 call it: entries [0, upto] of the table for
// max_errors; what lies at or beyond max_errors stays 0.
inline void init_match_limit(std::vector<int32_t> &ml, double erate, int32_t max_errors,
                             int32_t upto) {
  ml.assign((size_t)upto + 1, 0);
  int32_t e = 0, s = 1;
  const int32_t l = std::min<int32_t>(max_errors, 2000);
  while (e <= 1 && e <= upto) ml[e++] = 0;
  while (e < l && e <= upto) {
    s = binomial_bound(e - 1, erate, s);
    ml[e] = s - 1;
    e++;
  }
  if (e > upto) return;
  const double sl = 0.982064188397525 / erate + 0.067835741959926;   // AS_MAX_READLEN_BITS 21
  double vl = ml[e - 1] + sl;
  while (e < max_errors && e <= upto) {
    ml[e] = (int32_t)ceil(vl);
    vl += sl;
    e++;
  }
}

// A wave's row log, in values.  Row e is at most 2e + 1 wide, so (limit + 1)^2 values hold every
// row of an alignment with `limit` errors; a launch starts with per_error values per error and
// the overlaps that outgrow that run again with the worst case of the largest among them.
constexpr uint64_t ROW_LOG_MAX = 0x7fff0000ull;   // offsets into the log are 32-bit

inline uint64_t row_log_rows(int32_t limit) { return ((uint64_t)limit + 1) * ((uint64_t)limit + 1); }
inline uint64_t row_log_worst(int32_t limit) { return row_log_rows(limit) + 64; }
inline uint64_t row_log_first(int per_error, int32_t limit) {
  return std::min<uint64_t>((uint64_t)per_error * limit + 64, row_log_worst(limit));
}
// the log for the overlaps that overflowed log_cap, or 0 if log_cap was their worst case already
inline uint64_t row_log_regrown(uint64_t log_cap, int32_t next_limit) {
  return log_cap >= row_log_rows(next_limit) ? 0 : row_log_worst(next_limit);
}

// What findErrors (fe.hip) and correctOverlaps (co.hip) launch the wave aligner with.
constexpr int WAVES_PER_BLOCK = 4;
constexpr uint64_t SCRATCH_BUDGET = 16ull << 30;      // row logs of one launch, bytes
// the bits of a per-overlap outcome that mean the same in both; each stage has more of its own
enum : uint32_t { F_OVERFLOW = 4, F_GENERIC = 8, F_INTERNAL = 16, F_STAGED = 32 };

struct LaunchSize {
  bool ok;                   // false: the log is beyond ROW_LOG_MAX and nothing was sized
  uint64_t per_wave;         // ints of a wave's scratch: log, meta, stack, delta, the stage's own
  uint64_t nwaves;           // waves that own scratch
  uint32_t blocks;
  uint64_t scratch_bytes;
};

// 64 VGPRs and 4 KB of LDS per wave: eight waves per SIMD fit, if their row logs fit the budget;
// no more waves (and logs) than overlaps, and one wave always.  `extra` ints follow the delta.
inline LaunchSize launch_size(uint64_t log_cap, int32_t limit, uint64_t extra, uint64_t todo,
                              int n_cu, int waves_per_block = WAVES_PER_BLOCK,
                              uint64_t budget = SCRATCH_BUDGET) {
  LaunchSize L{};
  if (log_cap > ROW_LOG_MAX) return L;
  L.ok = true;
  L.per_wave = log_cap + 3ull * (limit + 2) + 2ull * (limit + 4) + extra + 8;
  const uint64_t fit = std::max<uint64_t>(1, budget / (L.per_wave * 4));
  L.nwaves = std::min<uint64_t>({todo, (uint64_t)n_cu * 8 * waves_per_block, fit});
  L.blocks = (uint32_t)((L.nwaves + waves_per_block - 1) / waves_per_block);
  L.scratch_bytes = L.per_wave * L.nwaves * 4;
  return L;
}

}  // namespace ped
