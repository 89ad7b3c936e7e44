// mhap_common.h -- what the kernels of the MHAP stage and its host code share: the constants and
// the records that cross between them (plain C++), and under hipcc the strand view and the wave
// helpers of the kernels.
#pragma once

#include <cstdint>

#include "mhap_hash.h"

namespace mh {

constexpr int64_t LMAX = 0x7FFFFFFFFFFFFFFFll;
constexpr int OCAP = 4096;        // ordered-sketch keys collected per strand (LDS)
constexpr int NBIN = 4096;        // radix-select bins (12-bit digits)
constexpr int TSLOTS = 2048;      // candidate table slots per wave
constexpr int TSHIFT = 21;        // 32 - log2(TSLOTS)
constexpr int RKW = 8;            // distinct k-mers per thread per round in k_mh_minhash
constexpr int RKK = 16;           // positions per thread in k_mh_keys

struct Cand {
  uint32_t q, t, cnt, pad;        // query read, stored strand (2 r + rc), shared entries
};

struct RecDev {
  uint32_t a, b;                  // reads (0-based in the context)
  uint32_t o, cnt;                // b strand, first-stage count
  uint32_t inter, n, raw, pad;    // Jaccard numerator / denominator, edges count
  int32_t a1, a2, a_len, b1, b2, b_len;
};

struct BloomDev {
  const uint64_t *words;        // null: keep every k-mer
  uint64_t bit_size;            // 64 x words
  int32_t k;                    // hash functions
};

// The -f table (FrequencyCounts.fractionCounts): open addressing on the 64-bit key.
struct FreqSlot {
  uint64_t key;
  double sidf;                    // scaledIdf of the k-mer (weighting mode 1)
  uint32_t used, pad;
};

enum { W_ONE = 0, W_TFIDF = 1, W_COUNT = 2 };

// one hash function's minimum so far: the exact draw, the k-mer's first position
// (FP_NONE: none yet) and the value stored (a key half)
struct BestOut {
  int64_t val;
  uint32_t fp;
  uint32_t v;
};

// A best draw of one hash function: its high word decides almost every comparison; the
// exact value is recomputed from (state, w) -- the k-mer's chain before the function's w
// draws -- only when two candidates tie on the high word (w = 0: state is the value).
struct BestRec {
  int32_t hi;
  uint32_t fp;                    // first position of the k-mer (0xFFFFFFFF: none yet)
  uint32_t v;                     // the value stored: the key's low / high 32 bits
  int32_t w;
  uint64_t state;
};

constexpr uint32_t FP_NONE = 0xFFFFFFFFu;

#ifdef __HIPCC__
// Utils$Translate (Utils.rc): the complement of an upper-case IUPAC byte, 0 for the rest
__constant__ uint8_t c_comp[256];

// One strand of a read as the jar sees it: the forward string, or Utils.rc of it
struct Strand {
  const uint8_t *s;
  int32_t L;
  int32_t rc;
  __device__ __forceinline__ uint64_t ch(int32_t p) const {
    return rc ? (uint64_t)c_comp[upper_byte(s[L - 1 - p])] : (uint64_t)upper_byte(s[p]);
  }
};

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t popc64(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }

__device__ __forceinline__ int32_t wave_sum_i32(int32_t v) {
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
  return v;
}
__device__ __forceinline__ int32_t wave_min_i32(int32_t v) {
  for (int s = 32; s > 0; s >>= 1) { const int32_t t = __shfl_xor(v, s); v = t < v ? t : v; }
  return v;
}
__device__ __forceinline__ int32_t wave_max_i32(int32_t v) {
  for (int s = 32; s > 0; s >>= 1) { const int32_t t = __shfl_xor(v, s); v = t > v ? t : v; }
  return v;
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
  for (int s = 32; s > 0; s >>= 1) { const uint32_t t = __shfl_xor(v, s); v = t < v ? t : v; }
  return v;
}

// signed 64-bit minimum over the wave, result uniform: DPP row shifts within 16-lane rows,
// then the row broadcasts (lanes whose source is outside the row read LMAX)
template <int CTRL, int RM>
__device__ __forceinline__ int64_t dpp_i64(int64_t v) {
  const int lo = __builtin_amdgcn_update_dpp((int)0xFFFFFFFF, (int)(uint32_t)v, CTRL, RM, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp((int)0x7FFFFFFF, (int)(uint32_t)((uint64_t)v >> 32),
                                             CTRL, RM, 0xf, false);
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
__device__ __forceinline__ int64_t wave_min_i64(int64_t v) {
  int64_t t;
  t = dpp_i64<0x111, 0xf>(v); v = t < v ? t : v;
  t = dpp_i64<0x112, 0xf>(v); v = t < v ? t : v;
  t = dpp_i64<0x114, 0xf>(v); v = t < v ? t : v;
  t = dpp_i64<0x118, 0xf>(v); v = t < v ? t : v;
  t = dpp_i64<0x142, 0xa>(v); v = t < v ? t : v;
  t = dpp_i64<0x143, 0xc>(v); v = t < v ? t : v;
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, 63);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)((uint64_t)v >> 32), 63);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
#endif  // __HIPCC__

}  // namespace mh
