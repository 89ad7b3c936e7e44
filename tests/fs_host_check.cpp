// fs_host_check.cpp -- a program of its own for the host code of falconsense, built with
// -fsanitize=address,undefined and run directly by tests/test_fs_cpu.py:
//
//   fs_host_check DIR NAME...
//
// For every NAME, DIR holds NAME.tig and NAME.dat (a corStore's two files) and NAME.expect (the
// layouts and children decoded by tests/fs_restate.py: uint32 n, n x {tig_id, layout_len,
// first_child, n_children}, uint32 m, m x {ident, reverse, min, max, askip, bskip}).  Checked:
// tgs_reader.h reads the store as decoded; it refuses the two files cut at every record
// boundary and with damaged counts; and the FASTA writer breaks lines at 60 columns.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../canu_amd/csrc/fs_fasta.h"
#include "../canu_amd/csrc/tgs_reader.h"

static int failures = 0;

#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);          \
      fprintf(stderr, "\n");                 \
      failures++;                            \
    }                                        \
  } while (0)

static bool refused(const std::vector<uint8_t> &tig, const std::vector<uint8_t> &dat) {
  tgs::Store s;
  std::string err;
  const bool ok = s.parse(tig.data(), tig.size(), dat.data(), dat.size(), err);
  return !ok && !err.empty();
}

static void put32(std::vector<uint8_t> &v, size_t at, uint32_t x) { memcpy(v.data() + at, &x, 4); }
static uint32_t get32(const std::vector<uint8_t> &v, size_t at) { return tgs::get<uint32_t>(v.data() + at); }

static void check_store(const std::string &dir, const std::string &name) {
  std::vector<uint8_t> tig, dat, exp;
  std::string err;
  if (!tgs::slurp(dir + "/" + name + ".tig", tig, err) || !tgs::slurp(dir + "/" + name + ".dat", dat, err) ||
      !tgs::slurp(dir + "/" + name + ".expect", exp, err)) {
    CHECK(false, "%s", err.c_str());
    return;
  }
  tgs::Store s;
  CHECK(s.parse(tig.data(), tig.size(), dat.data(), dat.size(), err), "%s: %s", name.c_str(), err.c_str());
  // the decoded layouts: every tig that is not deleted, in ID order
  const uint32_t n = get32(exp, 0);
  size_t at = 4, k = 0;
  std::vector<size_t> boundaries;
  for (const tgs::Tig &t : s.tigs) {
    if (t.deleted) continue;
    CHECK(k < n, "%s: more tigs than expected", name.c_str());
    if (k >= n) break;
    CHECK(get32(exp, at) == t.tig_id && get32(exp, at + 4) == t.layout_len &&
          get32(exp, at + 8) == t.first_child && get32(exp, at + 12) == t.n_children,
          "%s: tig %u differs", name.c_str(), t.tig_id);
    at += 16;
    k++;
  }
  CHECK(k == n, "%s: %zu tigs, expected %u", name.c_str(), k, n);
  const uint32_t m = get32(exp, at);
  at += 4;
  CHECK(m == s.children.size(), "%s: %zu children, expected %u", name.c_str(), s.children.size(), m);
  for (uint32_t c = 0; c < m && c < s.children.size(); c++, at += 24) {
    const tgs::Child &ch = s.children[c];
    CHECK(get32(exp, at) == ch.ident && get32(exp, at + 4) == ch.reverse &&
          (int32_t)get32(exp, at + 8) == ch.min && (int32_t)get32(exp, at + 12) == ch.max &&
          (int32_t)get32(exp, at + 16) == ch.askip && (int32_t)get32(exp, at + 20) == ch.bskip,
          "%s: child %u differs", name.c_str(), c);
  }

  // the index cut at every entry boundary (and inside the header)
  for (size_t cut : {(size_t)0, (size_t)4, (size_t)19}) {
    std::vector<uint8_t> t2(tig.begin(), tig.begin() + cut);
    CHECK(refused(t2, dat), "%s: index of %zu bytes accepted", name.c_str(), cut);
  }
  for (size_t e = 0; e < s.tigs.size(); e++) {
    std::vector<uint8_t> t2(tig.begin(), tig.begin() + tgs::HEADER_BYTES + e * tgs::ENTRY_BYTES);
    CHECK(refused(t2, dat), "%s: index cut before entry %zu accepted", name.c_str(), e);
  }
  // the data file cut at every record boundary: before a record, after its tag, after its
  // header, after each child
  for (size_t e = 0; e < s.tigs.size(); e++) {
    if (s.tigs[e].deleted) continue;
    const uint64_t word = tgs::get<uint64_t>(tig.data() + tgs::HEADER_BYTES + e * tgs::ENTRY_BYTES + tgs::RECORD_BYTES);
    const size_t off = (size_t)(word >> 24);
    std::vector<size_t> cuts = {off, off + 4, off + 4 + tgs::RECORD_BYTES};
    for (uint32_t c = 1; c <= s.tigs[e].n_children; c++)
      cuts.push_back(off + 4 + tgs::RECORD_BYTES + c * tgs::POSITION_BYTES);
    for (size_t cut : cuts) {
      if (cut >= dat.size()) continue;              // the whole file
      std::vector<uint8_t> d2(dat.begin(), dat.begin() + cut);
      CHECK(refused(tig, d2), "%s: data file cut at %zu (tig %zu) accepted", name.c_str(), cut, e);
    }
    // damaged counts: the children of this tig, in the data file only, then in both
    const size_t nch_dat = off + 4 + 36, nch_idx = tgs::HEADER_BYTES + e * tgs::ENTRY_BYTES + 36;
    for (uint32_t delta : {1u, 1000000u}) {
      std::vector<uint8_t> d2 = dat, t2 = tig;
      put32(d2, nch_dat, get32(dat, nch_dat) + delta);
      CHECK(refused(tig, d2), "%s: tig %zu with %u more children in the data file accepted", name.c_str(), e, delta);
      put32(t2, nch_idx, get32(tig, nch_idx) + delta);
      CHECK(refused(t2, d2), "%s: tig %zu with %u more children accepted", name.c_str(), e, delta);
    }
  }
  // damaged header counts
  for (int d : {-1, 1}) {
    std::vector<uint8_t> t2 = tig;
    put32(t2, 16, get32(tig, 16) + (uint32_t)d);
    CHECK(refused(t2, dat), "%s: index with %d entries more accepted", name.c_str(), d);
    t2 = tig;
    put32(t2, 8, get32(tig, 8) + (uint32_t)d);
    CHECK(refused(t2, dat), "%s: index with total %d off accepted", name.c_str(), d);
  }
  std::vector<uint8_t> t2 = tig;
  put32(t2, 0, 0x12345678);
  CHECK(refused(t2, dat), "%s: wrong magic accepted", name.c_str());
  t2 = tig;
  put32(t2, 4, 2);
  CHECK(refused(t2, dat), "%s: version 2 accepted", name.c_str());
}

static void check_fasta() {
  for (size_t len : {(size_t)59, (size_t)60, (size_t)61, (size_t)120, (size_t)0}) {
    std::vector<uint8_t> s(len);
    for (size_t i = 0; i < len; i++) s[i] = (uint8_t)"ACGT"[i & 3];
    std::string out;
    fs_fasta_record(out, 7, 2, s.data(), len);
    std::string want = ">read7_2\n";
    for (size_t i = 0; i < len; i += 60) want += std::string((const char *)s.data() + i, std::min<size_t>(60, len - i)) + "\n";
    CHECK(out == want, "FASTA record of %zu bases:\n%s", len, out.c_str());
    size_t lines = 0;
    for (char c : out) lines += c == '\n';
    CHECK(lines == 1 + (len + 59) / 60, "FASTA record of %zu bases has %zu lines", len, lines);
  }
  // pieces: split at lower case, strictly longer than the minimum
  std::string cns = std::string(500, 'A') + "c" + std::string(501, 'G') + "acgt" + std::string(3, 'T');
  std::string out, log;
  const uint32_t k = fs_fasta_pieces(out, &log, 3, (const uint8_t *)cns.data(), cns.size(), 500);
  CHECK(k == 1, "%u pieces, expected 1", k);
  CHECK(log == "Generated read 3_0 of length 501.\n", "log: %s", log.c_str());
  CHECK(out.rfind(">read3_0\n", 0) == 0, "header: %s", out.substr(0, 12).c_str());
}

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s DIR NAME...\n", argv[0]);
    return 2;
  }
  for (int i = 2; i < argc; i++) check_store(argv[1], argv[i]);
  check_fasta();
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("fs_host_check: %d store(s) ok\n", argc - 2);
  return 0;
}
