// mhap_hash.h -- the hashes of the MHAP stage that its kernels and its host code share, and the
// complement map of Utils.rc.  Plain C++: no HIP header; MHAP_HD is __host__ __device__ under hipcc
// and nothing but inline without it.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define MHAP_HD __device__ __host__ __forceinline__
#else
#define MHAP_HD inline
#endif

namespace mh {

// Utils$Translate (Utils.rc): the complement of an upper-case IUPAC byte, 0 for the rest
struct CompMap {
  uint8_t to[256];
};
constexpr CompMap make_comp_map() {
  CompMap m{};
  const char from[] = "ABCDGHKMNRSTVWY", to[] = "TVGHCDMKNYSABWR";
  for (int i = 0; from[i]; i++) m.to[(uint8_t)from[i]] = (uint8_t)to[i];
  return m;
}
constexpr CompMap COMP_MAP = make_comp_map();

MHAP_HD uint32_t upper_byte(uint32_t b) {
  return (b >= 'a' && b <= 'z') ? b - 32u : b;
}

MHAP_HD uint64_t rotl64(uint64_t x, int r) {
  return (x << r) | (x >> (64 - r));
}

MHAP_HD uint64_t fmix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33;
  k *= 0xC4CEB9FE1A85EC53ull;
  k ^= k >> 33;
  return k;
}

// Guava Hashing.murmur3_128(0).hashUnencodedChars(kmer).asLong(): MurmurHash3_x64_128 of
// the chars as little-endian UTF-16, first 8 bytes (h1)  (HashUtils.computeSequenceHashesLong
// @0-108; oracle mhap_jar.murmur3_128_h1)
template <class CH>
MHAP_HD uint64_t murmur128_h1(CH ch, int32_t k) {
  const uint64_t c1 = 0x87C37B91114253D5ull, c2 = 0x4CF5AD432745937Full;
  uint64_t h1 = 0, h2 = 0;
  const int32_t nb = k >> 3;
  int32_t q = 0;
  for (int32_t b = 0; b < nb; b++, q += 8) {
    uint64_t k1 = ch(q) | (ch(q + 1) << 16) | (ch(q + 2) << 32) | (ch(q + 3) << 48);
    uint64_t k2 = ch(q + 4) | (ch(q + 5) << 16) | (ch(q + 6) << 32) | (ch(q + 7) << 48);
    k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
    h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52DCE729;
    k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
    h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495AB5;
  }
  const int32_t t = k - 8 * nb;
  if (t > 4) {
    uint64_t k2 = 0;
    for (int32_t j = 0; j < t - 4; j++) k2 |= ch(q + 4 + j) << (16 * j);
    k2 *= c2; k2 = rotl64(k2, 33); k2 *= c1; h2 ^= k2;
  }
  if (t > 0) {
    uint64_t k1 = 0;
    for (int32_t j = 0; j < (t < 4 ? t : 4); j++) k1 |= ch(q + j) << (16 * j);
    k1 *= c1; k1 = rotl64(k1, 31); k1 *= c2; h1 ^= k1;
  }
  h1 ^= (uint64_t)(2 * k);
  h2 ^= (uint64_t)(2 * k);
  h1 += h2;
  h2 += h1;
  h1 = fmix64(h1);
  h2 = fmix64(h2);
  return h1 + h2;
}

// --supress-noise 1: the jar's bundled Guava 19.0 BloomFilter (MURMUR128_MITZ_64) over the
// -f file's keys (FrequencyCounts.<init> @189-207, lambda$1 @162-185; keepKmer @0-21).  The
// Long funnel hashes the key's 8 little-endian bytes with murmur3_128(0); bit i of a key is
// (h1 + i * h2 & Long.MAX_VALUE) % bitSize (BloomFilterStrategies$2.put / mightContain;
// oracle mhap_jar.GuavaBloom)
MHAP_HD void murmur128_u64(uint64_t key, uint64_t &h1, uint64_t &h2) {
  const uint64_t c1 = 0x87C37B91114253D5ull, c2 = 0x4CF5AD432745937Full;
  uint64_t k1 = key * c1;
  k1 = rotl64(k1, 31);
  k1 *= c2;
  h1 = k1 ^ 8u;                                   // one 8-byte tail, length 8
  h2 = 8u;
  h1 += h2;
  h2 += h1;
  h1 = fmix64(h1);
  h2 = fmix64(h2);
  h1 += h2;
  h2 += h1;
}

MHAP_HD bool bloom_has(const uint64_t *words, uint64_t bit_size,
                                                   int32_t k, uint64_t key) {
  uint64_t h1, h2;
  murmur128_u64(key, h1, h2);
  uint64_t c = h1;
  for (int32_t i = 0; i < k; i++, c += h2) {
    const uint64_t b = (c & 0x7FFFFFFFFFFFFFFFull) % bit_size;
    if (!((words[b >> 6] >> (b & 63)) & 1ull)) return false;
  }
  return true;
}

// the slot of a key in the -f table (open addressing, FreqSlot)
MHAP_HD uint64_t slot_hash(uint64_t key) {
  return fmix64(key ^ 0x9E3779B97F4A7C15ull);
}

}  // namespace mh
