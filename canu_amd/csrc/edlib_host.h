// edlib_host.h -- the arithmetic of edlib_wave.h's aligner that overlapPair (pair.hip),
// falconsense (fs.hip) and alignGFA (gfa.hip) share: the shape of a pass, obtainAlignment's leaf
// rule and the size of a wave's scratch.  Plain C++, no HIP; the constexpr functions are the
// kernels' as well.
#pragma once

#include <cstdint>

namespace edw {

constexpr uint32_t AS_MAX_READLEN = (1u << 21) - 1;
constexpr int WAVES_PER_BLOCK = 4;
constexpr int STRIPE_ROWS = 4096;                     // 64 lanes x 64 rows
constexpr int LDS_COLUMNS = 16384;                    // stripe-boundary row kept in LDS
constexpr int LDS_WORDS = LDS_COLUMNS / 16;           // 2 bits per column
constexpr int STACK_DEPTH = 40;                       // the target halves at every level

// A stripe's boundary row of a wave in global memory, in words: none while the longest target
// fits the row in LDS.
inline uint64_t grow_words(uint32_t max_target) {
  return max_target > (uint32_t)LDS_COLUMNS ? ((uint64_t)max_target + 15) / 16 : 0;
}

// obtainAlignment (edlib.C:1193): a span of qn rows and tn columns is traced back directly when
// Pv, Mv and the score of every block column (20 bytes) and 8 bytes more per column stay under
// leaf_bytes, else it is split.
constexpr bool is_leaf(int qn, int tn, long long leaf_bytes) {
  return 20ll * ((qn + 63) >> 6) * tn + 8ll * tn < leaf_bytes;
}

// block columns of the largest leaf
constexpr int leaf_entries(long long leaf_bytes) { return (int)(leaf_bytes / 20 + 1); }

struct PathSize {            // a wave's path scratch, from the longest query and target
  uint32_t leaf_entries;     // Pv, Mv and score of a leaf's block columns
  uint32_t max_blocks;       // Pv, Mv and score of a split's last column, twice: left, right
  uint64_t ops_bytes;        // a leaf's operations
  uint64_t grow_words;
};

inline PathSize path_size(uint32_t max_query, uint32_t max_target, long long leaf_bytes) {
  PathSize Z;
  Z.leaf_entries = (uint32_t)leaf_entries(leaf_bytes);
  Z.max_blocks = (max_query + 63) / 64 + 1;
  Z.ops_bytes = ((uint64_t)max_query + max_target + 64 + 15) & ~15ull;
  Z.grow_words = grow_words(max_target);
  return Z;
}

}  // namespace edw
