// mhap_host_check -- prints what canu_amd/csrc/mhap_host.h computes, for tests/test_mhap_host.py.
// A program of its own (g++, AddressSanitizer and UBSan): no HIP, no GPU, never loaded into Python.
//   mhap_host_check <what> <arguments...>       (table: "kmer fraction" lines on stdin)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../canu_amd/csrc/mhap_host.h"

using namespace mhap_host;

static uint64_t bits_of(double x) {
  uint64_t u;
  memcpy(&u, &x, 8);
  return u;
}

// the probe of the kernels' table_find, with the slot hash the host inserted by
static bool table_has(const FreqTable &T, uint64_t key) {
  for (uint64_t h = mh::slot_hash(key) & T.mask;; h = (h + 1) & T.mask) {
    if (!T.slots[h].used) return false;
    if (T.slots[h].key == key) return true;
  }
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string what = argv[1];
  const auto I = [&](int i) { return atoll(argv[i]); };
  const auto D = [&](int i) { return strtod(argv[i], nullptr); };

  if (what == "bloom") {                       // expected... -> words bits k
    for (int i = 2; i < argc; i++) {
      const BloomPlan B = bloom_plan((uint64_t)I(i));
      printf("%zu %" PRIu64 " %d\n", B.words, B.bits, B.k);
    }
  } else if (what == "table") {                // k do_rc repeat_weight scale cutoff noise expected
    if (argc != 9) return 2;
    const uint32_t k = (uint32_t)I(2);
    mhap_weighting w{D(4), D(5), D(6), 0, (int32_t)I(7)};
    std::string kmers, km;
    std::vector<double> fr;
    std::string f;
    while (std::cin >> km >> f) {
      if (km.size() != k) return 2;
      kmers += km;
      fr.push_back(strtod(f.c_str(), nullptr));
    }
    const bool bloom = w.supress_noise == 1;
    const BloomPlan plan = bloom ? bloom_plan((uint64_t)I(8)) : BloomPlan{};
    const FreqTable T = freq_table(kmers.data(), fr.data(), fr.size(), k, I(3) != 0, w,
                                   bloom ? &plan : nullptr);
    printf("slots %zu %" PRIu64 "\n", T.slots.size(), T.mask);
    for (const mh::FreqSlot &s : T.slots)
      if (s.used)
        printf("key %016" PRIx64 " %016" PRIx64 " %d\n", s.key, bits_of(s.sidf),
               (int)table_has(T, s.key));
    printf("bloom %zu %" PRIu64 " %d\n", T.bloom.size(), plan.bits, plan.k);
    for (uint64_t x : T.bloom) printf("word %016" PRIx64 "\n", x);
  } else if (what == "key") {                  // do_rc kmer... -> key
    for (int i = 3; i < argc; i++)
      printf("%016" PRIx64 "\n",
             canonical_key((const uint8_t *)argv[i], (uint32_t)strlen(argv[i]), I(2) != 0));
  } else if (what == "accept") {               // S kk threshold -> pass_empty, then the words
    const std::vector<uint32_t> bits = accept_bits((uint32_t)I(2), (int)I(3), D(4));
    printf("%u\n", pass_empty((int)I(3), D(4)));
    for (uint32_t x : bits) printf("%08x\n", x);
  } else if (what == "weight") {               // (repeat_weight has_table scale)... -> mode bs_w
    for (int i = 2; i + 2 < argc; i += 3) {
      const int mode = weighting_mode(D(i), I(i + 1) != 0);
      printf("%d %d\n", mode, bitslice_weight(mode, D(i + 2)));
    }
  } else if (what == "strands") {              // k ordered_k min_olap no_rc r0 nr len...
    std::vector<uint32_t> len, sids;
    for (int i = 8; i < argc; i++) len.push_back((uint32_t)I(i));
    const uint64_t used = strands_in_use(len.data(), (uint32_t)I(6), (uint32_t)I(7), (int32_t)I(4),
                                         (uint32_t)I(2), (uint32_t)I(3), I(5) != 0, sids);
    printf("%" PRIu64 " %d", used, min_use((int32_t)I(4), (uint32_t)I(2)));
    for (uint32_t s : sids) printf(" %u", s);
    printf("\n");
  } else if (what == "batches") {              // k budget max_strands len... (sids: 2 r, 2 r + 1)
    std::vector<uint32_t> len, sids;
    for (int i = 5; i < argc; i++) len.push_back((uint32_t)I(i));
    for (uint32_t r = 0; r < len.size(); r++) sids.push_back(2 * r + (r & 1));
    for (const SketchBatch &B :
         sketch_batches(sids, len.data(), (int32_t)I(2), (uint64_t)I(3), (size_t)I(4))) {
      printf("%zu %zu %" PRIu64, B.a, B.b, B.tot);
      for (uint64_t o : B.koff) printf(" %" PRIu64, o);
      printf("\n");
    }
  } else if (what == "sizes") {                // end_bit H | initial nq | grown n | blocks n | ...
    for (int i = 2; i + 1 < argc; i += 2) {
      const std::string f = argv[i];
      const int64_t v = I(i + 1);
      if (f == "end_bit") printf("%d\n", index_end_bit((int32_t)v));
      else if (f == "initial") printf("%zu\n", cand_cap_initial((uint32_t)v));
      else if (f == "grown") printf("%zu\n", cand_cap_grown((uint32_t)v));
      else if (f == "rec") printf("%zu\n", rec_cap((uint32_t)v));
      else if (f == "blocks") printf("%u\n", compare_blocks((uint32_t)v));
      else if (f == "compare_lds") printf("%zu\n", compare_lds((int32_t)v));
      else if (f == "minhash_lds") printf("%zu\n", minhash_lds((uint32_t)v));
      else if (f == "bitslice_lds") printf("%zu\n", bitslice_lds((int32_t)v));
      else if (f == "candidates_lds") printf("%zu\n", candidates_lds());
      else return 2;
    }
  } else if (what == "fixed6") {
    for (int i = 2; i < argc; i++) printf("%s\n", java_fixed6(D(i)).c_str());
  } else if (what == "fetch") {                // first_iid kk (a b o inter n)... -> sorted records
    std::vector<mh::RecDev> h;
    for (int i = 4; i + 4 < argc; i += 5) {
      mh::RecDev r{};
      r.a = (uint32_t)I(i); r.b = (uint32_t)I(i + 1); r.o = (uint32_t)I(i + 2);
      r.inter = (uint32_t)I(i + 3); r.n = (uint32_t)I(i + 4);
      r.raw = r.inter; r.a1 = 1; r.a2 = 2; r.a_len = 3; r.b1 = 4; r.b2 = 5; r.b_len = 6; r.cnt = 9;
      h.push_back(r);
    }
    sort_records(h);
    char line[256];
    for (const mh::RecDev &r : h) {
      const mhap_record x = to_record(r, (uint32_t)I(2), (int)I(3));
      const int n = format_line(x, 1, 0, 1, line, sizeof line);
      printf("%u %u %u %016" PRIx64 " %u %d|%s\n", x.a_iid, x.b_iid, x.b_rc, bits_of(x.erate),
             x.count, n, line);
    }
  } else if (what == "range") {                // first_iid nreads (bgn end)...
    for (int i = 4; i + 1 < argc; i += 2)
      printf("%d\n", (int)range_loaded((uint32_t)I(i), (uint32_t)I(i + 1), (uint32_t)I(2),
                                       (uint32_t)I(3)));
  } else if (what == "params") {               // k H min_matches S kk max_shift min_store
    mhap_params p{};
    p.k = (uint32_t)I(2); p.num_hashes = (uint32_t)I(3); p.min_matches = (uint32_t)I(4);
    p.ordered_sketch = (uint32_t)I(5); p.ordered_k = (uint32_t)I(6);
    p.max_shift = D(7); p.min_store = (int32_t)I(8);
    printf("%s\n", check_params(&p).c_str());
  } else if (what == "weighting") {            // scale noise
    mhap_weighting w{0.9, D(2), 1e-5, 0, (int32_t)I(3)};
    printf("%s\n%s\n", check_weighting(&w).c_str(), check_weighting(nullptr).c_str());
  } else {
    return 2;
  }
  return 0;
}
