// pair_host_check.cpp -- the .ovb reader (canu_amd/csrc/ovb_reader.h) as a program of its
// own, so that it can run under AddressSanitizer / UBSan (tests/test_pair_cpu.py):
//
//   pair_host_check read <file.ovb> <out.bin>   records as ovl_record bytes; exit 2 + message
//                                               on a malformed file
//   pair_host_check selfcheck <dir>             write with the project's writer (several
//                                               blocks), read back, compare; hand-made streams
//                                               with every snappy element kind; bad streams
//   pair_host_check damage <file.ovb> <dir>     the file truncated at every length and with
//                                               bytes overwritten: each variant must read or
//                                               fail cleanly
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../canu_amd/csrc/ovb_reader.h"
#include "../canu_amd/csrc/ovl_ovb.h"

static int die(const std::string &m) {
  fprintf(stderr, "pair_host_check: %s\n", m.c_str());
  return 1;
}

static bool spit(const std::string &path, const std::vector<uint8_t> &b) {
  FILE *F = fopen(path.c_str(), "wb");
  if (!F) return false;
  bool ok = b.empty() || fwrite(b.data(), 1, b.size(), F) == b.size();
  return fclose(F) == 0 && ok;
}

static bool slurp(const std::string &path, std::vector<uint8_t> &b) {
  FILE *F = fopen(path.c_str(), "rb");
  if (!F) return false;
  b.clear();
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, F)) > 0) b.insert(b.end(), buf, buf + n);
  fclose(F);
  return true;
}

static std::vector<uint8_t> frame(const std::vector<uint8_t> &stream) {
  std::vector<uint8_t> f(8);
  uint64_t cl = stream.size();
  memcpy(f.data(), &cl, 8);
  f.insert(f.end(), stream.begin(), stream.end());
  return f;
}

static bool same(const ovl_record &x, const ovl_record &y) {
  return x.a_iid == y.a_iid && x.b_iid == y.b_iid && x.dat[0] == y.dat[0] && x.dat[1] == y.dat[1];
}

static int selfcheck(const std::string &dir) {
  std::string err;
  std::vector<ovl_record> got;
  // 1. the writer's files, empty, one record, several blocks
  for (uint64_t n : {0ull, 1ull, 43680ull, 100001ull}) {
    std::vector<ovl_record> recs(n);
    uint64_t x = 88172645463325252ull + n;
    for (auto &r : recs) {
      x ^= x << 13; x ^= x >> 7; x ^= x << 17;
      r.a_iid = (uint32_t)(x % 5000) + 1;
      r.b_iid = (uint32_t)((x >> 20) % 5000) + 1;
      r.dat[0] = x * 0x9E3779B97F4A7C15ull;
      r.dat[1] = x * 0xC2B2AE3D27D4EB4Full;
    }
    const std::string p = dir + "/w" + std::to_string(n) + ".ovb";
    if (ovl::write_ovb_file(recs.data(), n, p.c_str(), false) != 0) return die("write " + p);
    if (!ovb::read_ovb_file(p.c_str(), got, err)) return die("read " + p + ": " + err);
    if (got.size() != n) return die("count of " + p);
    for (uint64_t i = 0; i < n; i++)
      if (!same(got[i], recs[i])) return die("record " + std::to_string(i) + " of " + p);
  }
  // 2. one block of two records made of a literal and the three copy kinds
  //    record 0: words 1 2 3 4 5 6; record 1 repeats it
  std::vector<uint8_t> s = {48};                                  // 48 bytes
  s.push_back((4 - 1) << 2);                                      // literal, 4 bytes: word 1
  for (uint8_t b : {1, 0, 0, 0}) s.push_back(b);
  s.push_back((20 - 1) << 2);                                     // literal, words 2..6
  for (uint32_t w = 2; w <= 6; w++) for (int i = 0; i < 4; i++) s.push_back(i ? 0 : (uint8_t)w);
  s.push_back(1 | ((8 - 4) << 2) | (0 << 5)); s.push_back(24);    // copy-1: 8 bytes from 24 back
  s.push_back(2 | ((8 - 1) << 2)); s.push_back(24); s.push_back(0);   // copy-2: 8 bytes
  s.push_back(3 | ((8 - 1) << 2)); s.push_back(24); s.push_back(0); s.push_back(0); s.push_back(0);
  std::string p = dir + "/copies.ovb";
  if (!spit(p, frame(s))) return die("write " + p);
  if (!ovb::read_ovb_file(p.c_str(), got, err)) return die("copies: " + err);
  if (got.size() != 2 || !same(got[0], got[1]) || got[0].a_iid != 1 || got[0].b_iid != 2 ||
      got[0].dat[0] != ((3ull << 32) | 4) || got[0].dat[1] != ((5ull << 32) | 6))
    return die("copies: wrong records");
  // an overlapping copy (run-length): 24 bytes = literal of 1 byte, copy of 23 from 1 back
  s = {24, 0 << 2, 7, 2 | ((23 - 1) << 2), 1, 0};
  p = dir + "/rle.ovb";
  if (!spit(p, frame(s))) return die("write " + p);
  if (!ovb::read_ovb_file(p.c_str(), got, err) || got.size() != 1 || got[0].a_iid != 0x07070707u)
    return die("rle: " + err);
  // 3. streams that must be refused
  const std::vector<std::vector<uint8_t>> bad = {
      {},                                   // no length
      {0x80},                               // length unfinished
      {0xff, 0xff, 0xff, 0xff, 0xff, 0x01}, // length beyond 32 bits
      {0xff, 0xff, 0xff, 0x7f},             // length beyond a buffer
      {24, (24 - 1) << 2, 1, 2, 3},         // literal past the block
      {24, 61 << 2, 0xff},                  // literal length bytes past the block
      {4, (8 - 1) << 2, 1, 2, 3, 4, 5, 6, 7, 8},   // literal past the stated length
      {24, 2 | (7 << 2), 1, 0},             // copy with nothing before it
      {24, 0, 9, 2 | (7 << 2), 0, 0},       // copy offset 0
      {24, 0, 9, 1 | (7 << 2)},             // copy offset missing
      {24, 0, 9, 3 | (7 << 2), 1, 0},       // 4-byte offset cut short
      {24, 0, 9},                           // shorter than stated
      {8, (8 - 1) << 2, 1, 2, 3, 4, 5, 6, 7, 8},   // no whole record
  };
  for (size_t i = 0; i < bad.size(); i++) {
    p = dir + "/bad" + std::to_string(i) + ".ovb";
    if (!spit(p, frame(bad[i]))) return die("write " + p);
    err.clear();
    if (ovb::read_ovb_file(p.c_str(), got, err)) return die("bad stream " + std::to_string(i) + " was read");
    if (err.empty() || !got.empty()) return die("bad stream " + std::to_string(i) + ": no message");
  }
  // the frame itself: a length cut short, a length beyond the file
  std::vector<uint8_t> f = {1, 2, 3};
  p = dir + "/frame0.ovb";
  if (!spit(p, f) || ovb::read_ovb_file(p.c_str(), got, err)) return die("short frame was read");
  f = frame({24, 0, 9});
  f[1] = 0x10;
  p = dir + "/frame1.ovb";
  if (!spit(p, f) || ovb::read_ovb_file(p.c_str(), got, err)) return die("long frame was read");
  if (ovb::read_ovb_file((dir + "/absent.ovb").c_str(), got, err)) return die("absent file was read");
  printf("pair_host_check ok\n");
  return 0;
}

static int damage(const std::string &file, const std::string &dir) {
  std::vector<uint8_t> b;
  if (!slurp(file, b)) return die("can't read " + file);
  std::vector<ovl_record> want, got;
  std::string err;
  if (!ovb::read_ovb_file(file.c_str(), want, err)) return die(file + ": " + err);
  const std::string p = dir + "/damaged.ovb";
  size_t failed = 0, cases = 0;
  const size_t step = b.size() > 4096 ? b.size() / 997 + 1 : 1;
  for (size_t len = 0; len < b.size(); len += step) {           // truncations
    if (!spit(p, std::vector<uint8_t>(b.begin(), b.begin() + len))) return die("write " + p);
    cases++;
    if (!ovb::read_ovb_file(p.c_str(), got, err)) {
      failed++;
      if (err.empty()) return die("truncated file: no message");
    } else {                                                    // cut between two blocks
      if (got.size() >= want.size()) return die("truncated file gave every record");
      for (size_t i = 0; i < got.size(); i++)
        if (!same(got[i], want[i])) return die("truncated file gave other records");
    }
  }
  uint64_t x = 2463534242ull;
  for (int i = 0; i < 600; i++) {                                // overwritten bytes
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    std::vector<uint8_t> c = b;
    const size_t at = i < 64 ? (size_t)i % c.size() : (size_t)(x % c.size());
    c[at] = (uint8_t)(x >> 32);
    if (i % 3 == 0) c[(at + 1) % c.size()] = 0xff;
    if (!spit(p, c)) return die("write " + p);
    cases++;
    if (!ovb::read_ovb_file(p.c_str(), got, err)) {
      failed++;
      if (err.empty()) return die("damaged file: no message");
    }
  }
  printf("pair_host_check ok: %zu records, %zu damaged files, %zu refused\n", want.size(), cases,
         failed);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 4 && !strcmp(argv[1], "read")) {
    std::vector<ovl_record> recs;
    std::string err;
    if (!ovb::read_ovb_file(argv[2], recs, err)) {
      fprintf(stderr, "error: %s\n", err.c_str());
      return 2;
    }
    FILE *F = fopen(argv[3], "wb");
    if (!F) return die("can't write the output");
    static_assert(sizeof(ovl_record) == 24, "ovl_record is 24 bytes");
    if (!recs.empty() && fwrite(recs.data(), 24, recs.size(), F) != recs.size()) return die("write");
    return fclose(F) == 0 ? 0 : 1;
  }
  if (argc == 3 && !strcmp(argv[1], "selfcheck")) return selfcheck(argv[2]);
  if (argc == 4 && !strcmp(argv[1], "damage")) return damage(argv[2], argv[3]);
  return die("usage: read FILE OUT | selfcheck DIR | damage FILE DIR");
}
