// tgs_reader.h -- a read-only reader of canu's corStore (a tgStore, src/stores/tgStore.C and
// tgTig.C) as generateCorrectionLayouts writes it: version 1, two files.
//
//   seqDB.v001.tig   uint32 magic 'MASR', version 1, total, indexLen, n; then n tgStoreEntry:
//                    a tgTigRecord (48 bytes) and one word -- unused:12 flushNeeded:1
//                    isDeleted:1 svID:10 fileOffset:40
//   seqDB.v001.dat   at fileOffset: "TIGR", the tgTigRecord again, gappedLen bases and gappedLen
//                    quality values, childrenLen tgPosition (44 bytes), childDeltasLen int32
//
// Only what falconsense reads is kept: per tig its ID, the layout length, and of every child the
// ident, the orientation, min / max and the two skips.  Gapped bases and deltas are stepped
// over.  Every length and offset is checked against the two file sizes; a store that does not
// add up is refused with a message (the programs exit with status 1 on it).  Host only.
#ifndef CANU_TGS_READER_H
#define CANU_TGS_READER_H

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace tgs {

constexpr uint32_t MASR_MAGIC = 0x5253414d;
constexpr size_t RECORD_BYTES = 48, ENTRY_BYTES = 56, POSITION_BYTES = 44, HEADER_BYTES = 20;

struct Child {
  uint32_t ident, reverse;
  int32_t min, max, askip, bskip;
};

struct Tig {
  uint32_t tig_id = 0, layout_len = 0;
  bool deleted = true;
  uint64_t first_child = 0;
  uint32_t n_children = 0;
};

inline bool slurp(const std::string &path, std::vector<uint8_t> &out, std::string &err) {
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) { err = "can't open '" + path + "'"; return false; }
  out.clear();
  uint8_t buf[1 << 16];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  const bool bad = ferror(f) != 0;
  fclose(f);
  if (bad) { err = "can't read '" + path + "'"; return false; }
  return true;
}

template <class T> inline T get(const uint8_t *p) {
  T v;
  memcpy(&v, p, sizeof v);
  return v;
}

class Store {
 public:
  std::vector<Tig> tigs;          // by tig ID, 0 .. n-1
  std::vector<Child> children;

  bool open(const std::string &path, std::string &err) {
    std::vector<uint8_t> tig, dat;
    if (!slurp(path + "/seqDB.v001.tig", tig, err) || !slurp(path + "/seqDB.v001.dat", dat, err))
      return false;
    return parse(tig.data(), tig.size(), dat.data(), dat.size(), err);
  }

  bool parse(const uint8_t *tig, size_t tig_bytes, const uint8_t *dat, size_t dat_bytes,
             std::string &err) {
    tigs.clear();
    children.clear();
    if (tig_bytes < HEADER_BYTES) { err = "tig index of " + std::to_string(tig_bytes) + " bytes has no header"; return false; }
    if (get<uint32_t>(tig) != MASR_MAGIC) { err = "tig index: magic number mismatch"; return false; }
    if (get<uint32_t>(tig + 4) != 1) { err = "tig index: version " + std::to_string(get<uint32_t>(tig + 4)) + ", expected 1"; return false; }
    const uint32_t total = get<uint32_t>(tig + 8), n = get<uint32_t>(tig + 16);
    if (total != n || (uint64_t)n * ENTRY_BYTES + HEADER_BYTES != tig_bytes) {
      err = "tig index: " + std::to_string(n) + " entries (total " + std::to_string(total) +
            ") do not make " + std::to_string(tig_bytes) + " bytes";
      return false;
    }
    tigs.resize(n);
    std::vector<std::pair<uint64_t, uint64_t>> extent;     // of every record in the data file
    for (uint32_t k = 0; k < n; k++) {
      const uint8_t *e = tig + HEADER_BYTES + (size_t)k * ENTRY_BYTES;
      const uint64_t word = get<uint64_t>(e + RECORD_BYTES);
      Tig &t = tigs[k];
      t.tig_id = k;
      t.deleted = (word >> 13) & 1;
      if (t.deleted) continue;
      if (((word >> 14) & 1023) != 1) { err = "tig " + std::to_string(k) + " is of version " + std::to_string((word >> 14) & 1023); return false; }
      const uint64_t off = word >> 24;
      const std::string who = "tig " + std::to_string(k);
      if (off > dat_bytes || dat_bytes - off < 4 + RECORD_BYTES) { err = who + ": record at " + std::to_string(off) + " past the data file"; return false; }
      const uint8_t *r = dat + off;
      if (memcmp(r, "TIGR", 4) != 0) { err = who + ": no tig record at " + std::to_string(off); return false; }
      r += 4;
      if (get<uint32_t>(r) != k) { err = who + ": the record is of tig " + std::to_string(get<uint32_t>(r)); return false; }
      t.layout_len = get<uint32_t>(r + 28);
      const uint64_t gapped = get<uint32_t>(r + 32), nch = get<uint32_t>(r + 36), ndelta = get<uint32_t>(r + 40);
      if (nch != get<uint32_t>(e + 36)) { err = who + ": " + std::to_string(nch) + " children in the data file, " + std::to_string(get<uint32_t>(e + 36)) + " in the index"; return false; }
      const uint64_t need = 2 * gapped + nch * POSITION_BYTES + ndelta * 4;
      const uint64_t have = dat_bytes - off - 4 - RECORD_BYTES;
      if (need > have) { err = who + ": " + std::to_string(need) + " bytes of bases, children and deltas, " + std::to_string(have) + " left in the data file"; return false; }
      extent.push_back({off, off + 4 + RECORD_BYTES + need});
      const uint8_t *p = r + RECORD_BYTES + 2 * gapped;
      t.first_child = children.size();
      t.n_children = (uint32_t)nch;
      for (uint64_t c = 0; c < nch; c++, p += POSITION_BYTES) {
        Child ch;
        ch.ident = get<uint32_t>(p);
        ch.reverse = (get<uint32_t>(p + 4) >> 3) & 1;
        ch.askip = get<int32_t>(p + 20);
        ch.bskip = get<int32_t>(p + 24);
        ch.min = get<int32_t>(p + 28);
        ch.max = get<int32_t>(p + 32);
        children.push_back(ch);
      }
    }
    std::sort(extent.begin(), extent.end());
    for (size_t i = 1; i < extent.size(); i++)
      if (extent[i - 1].second > extent[i].first) {
        err = "the record at " + std::to_string(extent[i - 1].first) + " runs into the one at " +
              std::to_string(extent[i].first);
        return false;
      }
    return true;
  }
};

}  // namespace tgs

#endif
