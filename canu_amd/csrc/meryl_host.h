// meryl_host.h -- the host-only half of libcanu_meryl.so: the counted database in memory,
// its files (prefix.mcdat / prefix.mcidx, a format of this project), and the two texts of
// the reference's dump modes.  No HIP here: meryl.hip, bin/meryl and the stand-alone
// sanitizer program (tests/meryl_host_check.cpp) all include this header.
//
// prefix.mcidx  "CAMERIDX" u32 abi u32 k u32 canonical u32 low_count
//               u64 total u64 distinct u64 unique u64 largest u64 kept u64 nhist
//               nhist x (u64 count, u64 distinct mers with that count), ascending count
//               "XDIREMAC"
// prefix.mcdat  "CAMERDAT" u32 abi u32 k u64 kept
//               kept x u64 mer (ascending), kept x u32 count
//               "TADREMAC"
// All little endian.  Not the reference's bit-packed database: only its texts are matched.
#ifndef CANU_MERYL_HOST_H
#define CANU_MERYL_HOST_H

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace merhost {

constexpr uint32_t kDbAbi = 1;

struct MerDb {
  uint32_t k = 0;
  uint32_t canonical = 1;
  uint32_t low_count = 2;
  uint64_t total = 0, distinct = 0, unique = 0, largest = 0;
  std::vector<std::pair<uint64_t, uint64_t>> hist;   // (count, distinct mers), ascending
  std::vector<uint64_t> mers;                        // count >= low_count, ascending
  std::vector<uint32_t> counts;
};

// Totals from the sparse histogram (meryl keeps them in the index: libmeryl.C:404-433).
inline void finish_totals(MerDb &db) {
  db.total = db.distinct = db.unique = db.largest = 0;
  for (auto &h : db.hist) {
    db.total += h.first * h.second;
    db.distinct += h.second;
    if (h.first == 1) db.unique = h.second;
    if (h.first > db.largest) db.largest = h.first;
  }
}

inline void mer_to_string(uint64_t mer, uint32_t k, char *out) {
  for (uint32_t i = 0; i < k; i++) out[i] = "ACGT"[(mer >> (2 * (k - 1 - i))) & 3];
  out[k] = 0;
}

// meryl -Dh (plotHistogram, meryl-dump.C:125-155): rows to `rows`, the four lines to `info`.
inline void write_histogram(const MerDb &db, FILE *rows, FILE *info) {
  if (info) {
    fprintf(info, "Found %llu mers.\n", (unsigned long long)db.total);
    fprintf(info, "Found %llu distinct mers.\n", (unsigned long long)db.distinct);
    fprintf(info, "Found %llu unique mers.\n", (unsigned long long)db.unique);
    fprintf(info, "Largest mercount is %llu.\n", (unsigned long long)db.largest);
  }
  if (!rows) return;
  uint64_t distinct = 0, total = 0;
  for (auto &h : db.hist) {
    if (h.first == 0 || h.second == 0) continue;
    distinct += h.second;
    total += h.second * h.first;
    fprintf(rows, "%u\t%llu\t%.4f\t%.4f\n", (unsigned)h.first, (unsigned long long)h.second,
            distinct / (double)db.distinct, total / (double)db.total);
  }
}

// meryl -Dt -n min_count (dumpThreshold, meryl-dump.C:55-68).
inline void write_threshold(const MerDb &db, uint64_t min_count, FILE *out) {
  char s[40];
  for (size_t i = 0; i < db.mers.size(); i++)
    if (db.counts[i] >= min_count) {
      mer_to_string(db.mers[i], db.k, s);
      fprintf(out, ">%llu\n%s\n", (unsigned long long)db.counts[i], s);
    }
}

namespace detail {
inline bool put(FILE *f, const void *p, size_t n) { return n == 0 || fwrite(p, 1, n, f) == n; }
inline bool get(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
template <class T> bool put(FILE *f, T v) { return put(f, &v, sizeof v); }
template <class T> bool get(FILE *f, T &v) { return get(f, &v, sizeof v); }
inline long file_size(FILE *f) {
  long at = ftell(f);
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, at, SEEK_SET);
  return n;
}
}  // namespace detail

inline bool save(const MerDb &db, const std::string &prefix, std::string &err) {
  using namespace detail;
  std::string ip = prefix + ".mcidx", dp = prefix + ".mcdat";
  FILE *f = fopen(ip.c_str(), "wb");
  if (!f) { err = "cannot write " + ip; return false; }
  bool ok = put(f, "CAMERIDX", 8) && put(f, kDbAbi) && put(f, db.k) && put(f, db.canonical) &&
            put(f, db.low_count) && put(f, db.total) && put(f, db.distinct) &&
            put(f, db.unique) && put(f, db.largest) && put(f, (uint64_t)db.mers.size()) &&
            put(f, (uint64_t)db.hist.size());
  for (auto &h : db.hist) ok = ok && put(f, h.first) && put(f, h.second);
  ok = ok && put(f, "XDIREMAC", 8);
  ok = (fclose(f) == 0) && ok;
  if (!ok) { err = "short write to " + ip; return false; }
  f = fopen(dp.c_str(), "wb");
  if (!f) { err = "cannot write " + dp; return false; }
  ok = put(f, "CAMERDAT", 8) && put(f, kDbAbi) && put(f, db.k) &&
       put(f, (uint64_t)db.mers.size()) &&
       put(f, db.mers.data(), db.mers.size() * sizeof(uint64_t)) &&
       put(f, db.counts.data(), db.counts.size() * sizeof(uint32_t)) &&
       put(f, "TADREMAC", 8);
  ok = (fclose(f) == 0) && ok;
  if (!ok) { err = "short write to " + dp; return false; }
  return true;
}

inline bool open(const std::string &prefix, MerDb &db, std::string &err) {
  using namespace detail;
  std::string ip = prefix + ".mcidx", dp = prefix + ".mcdat";
  char magic[8];
  uint32_t abi = 0, k2 = 0;
  uint64_t kept = 0, kept2 = 0, nhist = 0;
  FILE *f = fopen(ip.c_str(), "rb");
  if (!f) { err = "cannot read " + ip; return false; }
  long size = detail::file_size(f);
  bool ok = get(f, magic, 8);
  if (!ok || memcmp(magic, "CAMERIDX", 8) != 0) {
    fclose(f);
    err = ip + ": not a canu_amd meryl index (the reference's databases are not readable)";
    return false;
  }
  ok = get(f, abi) && get(f, db.k) && get(f, db.canonical) && get(f, db.low_count) &&
       get(f, db.total) && get(f, db.distinct) && get(f, db.unique) && get(f, db.largest) &&
       get(f, kept) && get(f, nhist);
  if (ok && abi != kDbAbi) {
    fclose(f);
    err = ip + ": database ABI " + std::to_string(abi) + ", this build reads " +
          std::to_string(kDbAbi);
    return false;
  }
  // sizes are checked against the file before anything is allocated from them
  if (!ok || db.k < 1 || db.k > 32 || nhist > (uint64_t)size / 16 ||
      (uint64_t)size != 80 + nhist * 16) {
    fclose(f);
    err = ip + ": truncated or corrupt";
    return false;
  }
  db.hist.resize(nhist);
  for (auto &h : db.hist) ok = ok && get(f, h.first) && get(f, h.second);
  ok = ok && get(f, magic, 8) && memcmp(magic, "XDIREMAC", 8) == 0;
  fclose(f);
  if (!ok) { err = ip + ": truncated or corrupt"; return false; }

  f = fopen(dp.c_str(), "rb");
  if (!f) { err = "cannot read " + dp; return false; }
  size = detail::file_size(f);
  ok = get(f, magic, 8);
  if (!ok || memcmp(magic, "CAMERDAT", 8) != 0) {
    fclose(f);
    err = dp + ": not a canu_amd meryl database (the reference's databases are not readable)";
    return false;
  }
  ok = get(f, abi) && get(f, k2) && get(f, kept2);
  if (!ok || abi != kDbAbi || k2 != db.k || kept2 != kept || kept > (uint64_t)size / 12 ||
      (uint64_t)size != 32 + kept * 12) {
    fclose(f);
    err = dp + ": truncated, corrupt or not the partner of " + ip;
    return false;
  }
  db.mers.resize(kept);
  db.counts.resize(kept);
  ok = get(f, db.mers.data(), kept * sizeof(uint64_t)) &&
       get(f, db.counts.data(), kept * sizeof(uint32_t)) && get(f, magic, 8) &&
       memcmp(magic, "TADREMAC", 8) == 0;
  fclose(f);
  if (!ok) { err = dp + ": truncated or corrupt"; return false; }
  return true;
}

}  // namespace merhost
#endif
