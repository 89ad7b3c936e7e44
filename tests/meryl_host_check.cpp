// Stand-alone check of canu_amd/csrc/meryl_host.h (no HIP, no Python): built with
// -fsanitize=address,undefined by tests/test_meryl_cpu.py and run directly.  Writes a
// database of fixture size, reopens it, writes both texts, and feeds the reader damaged files.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../canu_amd/csrc/meryl_host.h"

static int failures = 0;
#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) { fprintf(stderr, "FAILED %s:%d %s\n", __FILE__, __LINE__, #x); failures++; } \
  } while (0)

static std::string slurp(const std::string &p) {
  std::string s;
  FILE *f = fopen(p.c_str(), "rb");
  if (!f) return s;
  char b[4096];
  size_t n;
  while ((n = fread(b, 1, sizeof b, f)) > 0) s.append(b, n);
  fclose(f);
  return s;
}

static void spit(const std::string &p, const std::string &s) {
  FILE *f = fopen(p.c_str(), "wb");
  if (f) { fwrite(s.data(), 1, s.size(), f); fclose(f); }
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <scratch dir>\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  merhost::MerDb db;
  db.k = 16;
  // 13,000 distinct mers with counts 1..40 (only counts >= 2 are kept), ascending
  uint64_t key = 0x12345, x = 88172645463325252ull;
  std::vector<uint64_t> h(64, 0);
  for (int i = 0; i < 13000; i++) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    key += 1 + (x % 300000);
    uint32_t c = (x >> 20) % 5 ? 1 : 2 + (uint32_t)((x >> 30) % 39);
    h[c]++;
    if (c >= db.low_count) { db.mers.push_back(key & 0xFFFFFFFFull); db.counts.push_back(c); }
  }
  for (uint64_t c = 1; c < h.size(); c++)
    if (h[c]) db.hist.push_back({c, h[c]});
  merhost::finish_totals(db);
  CHECK(db.distinct == 13000);

  std::string err;
  const std::string p = dir + "/db";
  CHECK(merhost::save(db, p, err));
  merhost::MerDb back;
  CHECK(merhost::open(p, back, err));
  CHECK(back.k == db.k && back.total == db.total && back.distinct == db.distinct &&
        back.unique == db.unique && back.largest == db.largest);
  CHECK(back.mers == db.mers && back.counts == db.counts && back.hist == db.hist);

  // the texts of the reopened database equal the original's
  for (int which = 0; which < 2; which++) {
    const merhost::MerDb &d = which ? back : db;
    std::string tag = which ? "b" : "a";
    FILE *r = fopen((dir + "/rows" + tag).c_str(), "w"), *i = fopen((dir + "/info" + tag).c_str(), "w"),
         *t = fopen((dir + "/dt" + tag).c_str(), "w");
    CHECK(r && i && t);
    if (!(r && i && t)) return 1;
    merhost::write_histogram(d, r, i);
    merhost::write_threshold(d, 5, t);
    fclose(r); fclose(i); fclose(t);
  }
  CHECK(slurp(dir + "/rowsa") == slurp(dir + "/rowsb") && !slurp(dir + "/rowsa").empty());
  CHECK(slurp(dir + "/infoa") == slurp(dir + "/infob"));
  CHECK(slurp(dir + "/dta") == slurp(dir + "/dtb") && slurp(dir + "/dta")[0] == '>');
  char s[40];
  merhost::mer_to_string(0x1B, 4, s);             // 00 01 10 11
  CHECK(std::string(s) == "ACGT");
  merhost::mer_to_string(~0ull, 32, s);
  CHECK(std::string(s) == std::string(32, 'T'));

  // damaged files are refused, not read past
  const std::string idx = slurp(p + ".mcidx"), dat = slurp(p + ".mcdat");
  const std::string q = dir + "/bad";
  for (size_t cut : {(size_t)0, (size_t)7, (size_t)30, idx.size() / 2, idx.size() - 1}) {
    spit(q + ".mcidx", idx.substr(0, cut));
    spit(q + ".mcdat", dat);
    CHECK(!merhost::open(q, back, err));
  }
  for (size_t cut : {(size_t)0, (size_t)9, (size_t)40, dat.size() / 2, dat.size() - 1}) {
    spit(q + ".mcidx", idx);
    spit(q + ".mcdat", dat.substr(0, cut));
    CHECK(!merhost::open(q, back, err));
  }
  std::string m = idx;
  m[0] = 'X';
  spit(q + ".mcidx", m);
  spit(q + ".mcdat", dat);
  CHECK(!merhost::open(q, back, err));
  m = idx;
  m[56] = (char)0xFF; m[57] = (char)0xFF; m[62] = (char)0x7F;   // a huge kept count
  spit(q + ".mcidx", m);
  CHECK(!merhost::open(q, back, err));
  m = idx;
  m[64] = (char)0xFF; m[71] = (char)0x7F;                        // a huge histogram length
  spit(q + ".mcidx", m);
  CHECK(!merhost::open(q, back, err));
  CHECK(!merhost::open(dir + "/absent", back, err));
  if (failures) return 1;
  puts("meryl_host_check ok");
  return 0;
}
