// mhap_host.h -- the host arithmetic of the MHAP stage as plain functions (standard library only,
// so tests/mhap_host_check.cpp runs it without a GPU): argument checks, the acceptance bits, the
// Guava Bloom plan and the -f table, the weighting mode, the strands in use and the MinHash batch
// plan, the index / compare launch sizes, and the order and text of the records.  Values in,
// values or vectors out; the extern "C" functions of mhap.hip call them between their HIP calls.
#pragma once

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/canu_mhap.h"
#include "mhap_common.h"

namespace mhap_host {

using namespace mh;

// ---- argument checks: the message of a refusal (ERR_BAD_PARAM), empty when there is none ----
inline std::string check_params(const mhap_params *p) {
  if (!p) return "null params";
  if (p->k < 1 || p->k > 32 || p->ordered_k < 1 || p->ordered_k > 32)
    return "k-mer sizes must be 1..32";
  if (p->num_hashes < 1 || p->num_hashes > 1024) return "num_hashes must be 1..1024";
  if (p->ordered_sketch < 1 || p->ordered_sketch > 2048)   // k_mh_compare LDS: 3 x 8 S + 1 KB
    return "ordered_sketch must be 1..2048";
  if (p->min_matches < 1) return "min_matches must be >= 1";
  if (!(p->max_shift >= -1.0)) return "--max-shift must be >= -1";
  if (p->min_store < 0) return "--min-store-length must be >= 0";
  return "";
}

inline std::string check_weighting(const mhap_weighting *w) {
  if (!w) return "null weighting";
  if (!(w->repeat_idf_scale >= 1.0)) return "The minimum repeat idf scale must be >=1.0.";
  if (w->supress_noise < 0 || w->supress_noise > 2)            // FrequencyCounts.<init> @10-50
    return "Unknown removeUnique option " + std::to_string(w->supress_noise) + ".";
  return "";
}

// reads bgn..end (inclusive IDs) lie inside the loaded reads first_iid .. first_iid + nreads - 1
inline bool range_loaded(uint32_t bgn, uint32_t end, uint32_t first_iid, uint32_t nreads) {
  return !(bgn < first_iid || end >= first_iid + nreads || bgn > end);
}

// ---- second-stage acceptance ------------------------------------------------------------------
// the jar's score of a Jaccard value (BottomOverlapSketch.jaccardToIdentity @0-25)
inline double jaccard_identity(double J, int kk) {
  if (!(J > 0.0)) return 0.0;
  const double d = (-1.0 / (double)kk) * log(2.0 * J / (1.0 + J));
  return exp(-d);
}

// computeKBottomSketchJaccard's J = inter / n (0 when n = 0)
inline double jaccard_of(uint32_t inter, uint32_t n) {
  return n == 0 ? 0.0 : (double)inter / (double)n;
}

// bit n (S + 1) + i: identity(i / n) >= threshold, for 1 <= n <= S, i <= n; the identity is
// computed here, on the host, exactly as the oracle does
inline std::vector<uint32_t> accept_bits(uint32_t S, int kk, double threshold) {
  const size_t nbits = (size_t)(S + 1) * (S + 1);
  std::vector<uint32_t> bits((nbits + 31) / 32, 0);
  for (uint32_t n = 1; n <= S; n++)
    for (uint32_t i = 0; i <= n; i++)
      if (jaccard_identity(jaccard_of(i, n), kk) >= threshold) {
        const size_t b = (size_t)n * (S + 1) + i;
        bits[b >> 5] |= 1u << (b & 31);
      }
  return bits;
}

// identity 0 (n = 0) >= threshold
inline uint32_t pass_empty(int kk, double threshold) {
  return jaccard_identity(0.0, kk) >= threshold ? 1u : 0u;
}

// ---- the -f table (FrequencyCounts) -------------------------------------------------------------
// Guava BloomFilter.create(funnel, expected (0 -> 1), 1e-5): optimalNumOfBits,
// optimalNumOfHashFunctions, BitArray of ceil(bits / 64) longs.  words = 0: a filter of 0 bits,
// which the caller refuses.
struct BloomPlan {
  size_t words = 0;
  uint64_t bits = 0;              // 64 x words
  int32_t k = 0;                  // hash functions
};

inline BloomPlan bloom_plan(uint64_t expected) {
  const int64_t ne = expected ? (int64_t)expected : 1;
  const int64_t bits = (int64_t)((double)(-ne) * log(1e-5) / (log(2.0) * log(2.0)));
  const double hk = (double)bits / (double)ne * log(2.0);
  const double fk = floor(hk);
  BloomPlan B;
  B.k = std::max<int32_t>(1, (int32_t)((int64_t)fk + (hk - fk >= 0.5 ? 1 : 0)));
  B.words = (size_t)((bits + 63) / 64);
  B.bits = 64ull * B.words;
  return B;
}

// a k-mer's key: the hash of the smaller of it and Utils.rc of it (reverse, upper case,
// complement; String.compareTo is memcmp's order), of the k-mer itself without do_rc
inline uint64_t canonical_key(const uint8_t *km, uint32_t k, bool do_rc) {
  uint8_t rk[32];
  const uint8_t *use = km;
  if (do_rc) {
    for (uint32_t t = 0; t < k; t++) rk[t] = COMP_MAP.to[upper_byte(km[k - 1 - t])];
    if (memcmp(rk, km, k) < 0) use = rk;
  }
  return murmur128_h1([&](int32_t q) { return (uint64_t)use[q]; }, (int32_t)k);
}

struct FreqTable {
  std::vector<FreqSlot> slots;    // open addressing at load <= 1/2 (slot_hash, linear probes)
  uint64_t mask = 0;
  std::vector<uint64_t> bloom;    // the filter's words (empty without a plan)
};

// FrequencyCounts.<init> @0-429 and its lambda$1 (oracle mhap_jar.FrequencyCounts): n k-mers of
// k <= 32 bytes back to back with their fractions, in file order.  bloom (--supress-noise 1):
// every line's key enters the filter, whatever its fraction (lambda$1 @162-185).
inline FreqTable freq_table(const char *kmers, const double *fractions, uint64_t n, uint32_t k,
                            bool do_rc, const mhap_weighting &w, const BloomPlan *bloom) {
  FreqTable T;
  if (bloom) T.bloom.assign(bloom->words, 0ull);
  const double offset = (w.repeat_weight >= 0.0 && w.repeat_weight < 1.0) ? w.repeat_weight : 0.0;
  const double cutoff = w.filter_threshold, range = w.repeat_idf_scale;
  // key -> fraction, file order, a later line of the same key replacing an earlier one
  std::vector<std::pair<uint64_t, double>> kv;
  double max_value = -INFINITY;
  for (uint64_t i = 0; i < n; i++) {
    const double f = fractions[i];
    if (!(f >= cutoff) && !bloom) continue;
    const uint64_t key = canonical_key((const uint8_t *)kmers + i * k, k, do_rc);
    if (bloom) {
      uint64_t h1, h2;
      murmur128_u64(key, h1, h2);
      uint64_t x = h1;
      for (int32_t j = 0; j < bloom->k; j++, x += h2) {
        const uint64_t b = (x & 0x7FFFFFFFFFFFFFFFull) % bloom->bits;
        T.bloom[b >> 6] |= 1ull << (b & 63);
      }
    }
    if (!(f >= cutoff)) continue;
    max_value = std::max(max_value, f);
    kv.emplace_back(key, f);
  }
  const auto idf = [&](double x) { return log(max_value / x - offset); };
  const double min_idf = idf(max_value), max_idf = idf(cutoff);
  const double scale = (max_idf - min_idf) / (range - 1.0);
  uint64_t slots = 16;
  while (slots < 2 * kv.size() + 1) slots <<= 1;
  T.slots.assign(slots, FreqSlot{0, 0.0, 0, 0});
  T.mask = slots - 1;
  for (const auto &e : kv) {
    uint64_t h = slot_hash(e.first) & T.mask;
    while (T.slots[h].used && T.slots[h].key != e.first) h = (h + 1) & T.mask;
    T.slots[h].key = e.first;
    T.slots[h].used = 1;
    T.slots[h].sidf = 1.0 + (idf(e.second) - min_idf) / scale;     // scaledIdf @31-94
  }
  return T;
}

// ---- weighting ----------------------------------------------------------------------------------
// W_ONE (repeat_weight < 0), W_TFIDF (a -f table and repeat_weight < 1), else W_COUNT
inline int weighting_mode(double repeat_weight, bool has_table) {
  return repeat_weight < 0.0 ? W_ONE : (has_table && repeat_weight < 1.0) ? W_TFIDF : W_COUNT;
}

// The weight of a k-mer seen once in its strand and not in the -f table -- nearly all of a
// sketch's k-mers -- whose draws k_mh_bitslice takes
inline int32_t bitslice_weight(int mode, double repeat_idf_scale) {
  if (mode != W_TFIDF) return 1;                    // W_ONE: 1 (not popular); W_COUNT: count
  const double x = repeat_idf_scale;                // tf(1) x scaledIdf of an absent k-mer
  const double f = floor(x);
  const int64_t w = (int64_t)f + (x - f >= 0.5 ? 1 : 0);   // Math.round
  return (int32_t)std::min<int64_t>(std::max<int64_t>(w, 1), 0x7FFFFFFF);
}

// ---- sketching ----------------------------------------------------------------------------------
// the shortest read that is used: --min-olap-length, and at least a k-mer
inline int32_t min_use(int32_t min_olap, uint32_t k) { return std::max<int32_t>(min_olap, (int32_t)k); }

// The strands (2 r + rc) of reads r0 .. r0 + nr - 1 that get a MinHash sketch, in order; returns
// the number of reads used.  len: the context's read lengths.
inline uint64_t strands_in_use(const uint32_t *len, uint32_t r0, uint32_t nr, int32_t min_olap,
                               uint32_t k, uint32_t ordered_k, bool no_rc,
                               std::vector<uint32_t> &sids) {
  const int32_t mu = min_use(min_olap, k);
  uint64_t used = 0;
  sids.clear();
  for (uint32_t i = 0; i < nr; i++) {
    const uint32_t r = r0 + i;
    const int64_t L = len[r];
    if (L < mu || L < (int64_t)ordered_k) continue;
    used++;
    sids.push_back(2 * r);
    if (!no_rc) sids.push_back(2 * r + 1);
  }
  return used;
}

// One launch of the MinHash kernels: strands sids[a, b), strand a + i's k-mers at koff[i]
// (b - a + 1 entries), tot of them.
struct SketchBatch {
  size_t a = 0, b = 0;
  std::vector<uint64_t> koff;
  uint64_t tot = 0;
};

constexpr uint64_t KEY_BUDGET = 1ull << 29;       // k-mers per batch
constexpr size_t BATCH_STRANDS = 1u << 20;        // strands per batch

// Batches of at most key_budget k-mers and max_strands strands, in order; a batch always takes
// at least one strand, even one that exceeds the budget alone.  A read shorter than k adds 0.
inline std::vector<SketchBatch> sketch_batches(const std::vector<uint32_t> &sids,
                                               const uint32_t *len, int32_t k,
                                               uint64_t key_budget, size_t max_strands) {
  std::vector<SketchBatch> out;
  for (size_t a = 0; a < sids.size();) {
    SketchBatch B;
    B.a = a;
    size_t b = a;
    while (b < sids.size() && b - a < max_strands) {
      const int64_t np = (int64_t)len[sids[b] >> 1] - k + 1;
      const uint64_t add = np > 0 ? (uint64_t)np : 0;
      if (B.tot + add > key_budget && b > a) break;
      B.koff.push_back(B.tot);
      B.tot += add;
      b++;
    }
    B.koff.push_back(B.tot);
    B.b = b;
    out.push_back(std::move(B));
    a = b;
  }
  return out;
}

// ---- index and compare --------------------------------------------------------------------------
// the index's keys are j << 32 | value with j <= H: the radix sort's last bit
inline int index_end_bit(int32_t H) {
  int end_bit = 32;
  while ((1ll << (end_bit - 32)) <= H) end_bit++;
  return end_bit;
}

// candidates the first stage has room for: at first, and after a launch that counted `count`
inline size_t cand_cap_initial(uint32_t nq) { return std::max<size_t>((size_t)nq * 64, 1u << 16); }
inline size_t cand_cap_grown(uint32_t count) { return (size_t)count + (count >> 2) + 1024; }
constexpr size_t CAND_CAP_MAX = 0xFFFFFFF0ull;

inline size_t rec_cap(uint32_t ncand) { return std::max<size_t>(ncand, 1024); }

// k_mh_compare: one wave per block, the blocks stride over the candidates
inline uint32_t compare_blocks(uint32_t ncand) { return std::min<uint32_t>(ncand, 256u * 64u); }

// dynamic LDS: k_mh_candidates' [4][TSLOTS] keys and counts; k_mh_compare's A, B, groups [S]
// (u64) and histogram; k_mh_minhash's [4][H] BestRec; k_mh_bitslice's [H] BestOut
inline size_t candidates_lds() { return 2 * 4 * TSLOTS * sizeof(uint32_t); }
inline size_t compare_lds(int32_t S) { return 3 * 8 * (size_t)S + 1024; }
inline size_t minhash_lds(uint32_t H) { return sizeof(BestRec) * 4 * H; }
inline size_t bitslice_lds(int32_t H) { return sizeof(BestOut) * H; }

// ---- records ------------------------------------------------------------------------------------
// mhap_fetch's order: (a, b, o)
inline void sort_records(std::vector<RecDev> &h) {
  std::sort(h.begin(), h.end(), [](const RecDev &x, const RecDev &y) {
    return x.a != y.a ? x.a < y.a : x.b != y.b ? x.b < y.b : x.o < y.o;
  });
}

inline mhap_record to_record(const RecDev &r, uint32_t first_iid, int ordered_k) {
  const double score = jaccard_identity(jaccard_of(r.inter, r.n), ordered_k);
  return mhap_record{first_iid + r.a, first_iid + r.b, 1.0 - std::min(score, 1.0),
                     (double)r.raw, r.a1, r.a2, r.a_len, r.o, r.b1, r.b2, r.b_len, r.cnt};
}

// Java's String.format("%.6f", x): the shortest decimal that reads back as x
// (FloatingDecimal), rounded half-up to 6 places (FormattedFloatingDecimal.applyPrecision)
inline std::string java_fixed6(double x) {
  char buf[64];
  auto res = std::to_chars(buf, buf + sizeof buf, x, std::chars_format::scientific);
  *res.ptr = 0;
  // d.ddddde[+-]xx -> digits, exponent
  std::string mant(buf, strchr(buf, 'e'));
  const int ex = atoi(strchr(buf, 'e') + 1);
  bool neg = false;
  if (!mant.empty() && mant[0] == '-') { neg = true; mant.erase(0, 1); }
  std::string dig;
  for (char ch : mant)
    if (ch != '.') dig += ch;
  // value = 0.dig * 10^(ex + 1); keep integer part + 6 decimals
  const int ip = ex + 1;                         // digits before the point
  std::string intpart, frac;
  if (ip <= 0) {
    intpart = "0";
    frac = std::string(-ip, '0') + dig;
  } else {
    if ((int)dig.size() < ip) dig += std::string(ip - dig.size(), '0');
    intpart = dig.substr(0, ip);
    frac = dig.substr(ip);
  }
  if (frac.size() < 7) frac += std::string(7 - frac.size(), '0');
  const bool up = frac[6] >= '5';
  std::string num = intpart + frac.substr(0, 6);
  if (up) {
    int i = (int)num.size() - 1;
    while (i >= 0 && num[i] == '9') num[i--] = '0';
    if (i >= 0) num[i]++;
    else num.insert(num.begin(), '1');
  }
  std::string s = num.substr(0, num.size() - 6) + "." + num.substr(num.size() - 6);
  return neg ? "-" + s : s;
}

// MatchResult.toString's line into buf[cap]: snprintf's return value
inline int format_line(const mhap_record &x, uint32_t hash_base, uint32_t num_hash,
                       uint32_t query_base, char *buf, size_t cap) {
  // mhapConvert.C:122-123: a_iid = W0 + (query_base - 1) - num_hash, b_iid = W1 + hash_base - 1
  const uint64_t w0 = (uint64_t)x.a_iid - (query_base - 1) + num_hash;
  const uint64_t w1 = (uint64_t)x.b_iid - (hash_base - 1);
  return snprintf(buf, cap, "%llu %llu %s %s 0 %d %d %d %u %d %d %d", (unsigned long long)w0,
                  (unsigned long long)w1, java_fixed6(x.erate).c_str(), java_fixed6(x.raw).c_str(),
                  x.a_bgn, x.a_end, x.a_len, x.b_rc, x.b_bgn, x.b_end, x.b_len);
}

}  // namespace mhap_host
