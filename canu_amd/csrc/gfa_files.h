// gfa_files.h -- the files of canu_amd/bin/alignGFA, byte-compatible with the reference's
// src/gfa/gfa.C and bed.C: the GFA and BED readers (lines split at spaces and tabs, the LN:i:
// lookup, the name-to-ID rule, gfaLink::alignmentLength) and writers, and a reader of the bases
// of a tgStore at any version (src/stores/tgStore.C, tgTig.C) with the checks tgs_reader.h makes:
//
//   seqDB.v<V>.tig   uint32 magic 'MASR', version 1, total, indexLen, n; then n tgStoreEntry: a
//                    tgTigRecord (48 bytes) and one word -- unused:12 flushNeeded:1 isDeleted:1
//                    svID:10 fileOffset:40.  Version V, or the nearest one below that exists.
//   seqDB.v<svID>.dat  at fileOffset: "TIGR", the tgTigRecord again, gappedLen bases, gappedLen
//                    quality values, children, deltas
//
// A tig's sequence is its gapped consensus without the '-' (tgTig::buildUngapped); an entry that
// is deleted or of version 0 has none.  A file that does not add up is refused with a message;
// a line with too few fields, which the reference reads through a null pointer, likewise.
// Host only.
#ifndef CANU_GFA_FILES_H
#define CANU_GFA_FILES_H

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "tgs_reader.h"

namespace gfa_files {

inline std::vector<std::string> split_words(const std::string &line) {
  std::vector<std::string> w;
  size_t i = 0;
  while (i < line.size()) {
    while (i < line.size() && (line[i] == ' ' || line[i] == '\t')) i++;
    size_t j = i;
    while (j < line.size() && line[j] != ' ' && line[j] != '\t') j++;
    if (j > i) w.push_back(line.substr(i, j - i));
    i = j;
  }
  return w;
}

inline std::vector<std::string> split_lines(const std::string &text) {
  std::vector<std::string> out;
  size_t i = 0;
  while (i < text.size()) {
    size_t j = text.find('\n', i);
    if (j == std::string::npos) j = text.size();
    if (j > i) out.push_back(text.substr(i, j - i));
    i = j + 1;
  }
  return out;
}

// nameToCanuID: 'tig', 'utg' or 'ctg' and a number; anything else is UINT32_MAX
inline uint32_t name_to_id(const std::string &name) {
  if (name.size() >= 3 && (!name.compare(0, 3, "tig") || !name.compare(0, 3, "utg") ||
                           !name.compare(0, 3, "ctg")))
    return (uint32_t)strtoll(name.c_str() + 3, nullptr, 10);
  return UINT32_MAX;
}

// findGFAtokenI for "LN:i:"
inline bool find_length(const std::string &features, uint32_t &value) {
  const char *p = strstr(features.c_str(), "LN:i:");
  if (!p) return false;
  p += 5;
  if (*p == ':') p++;
  value = (uint32_t)strtoll(p, nullptr, 10);
  return true;
}

struct Sequence {
  std::string name, sequence, features;
  uint32_t id = UINT32_MAX, length = 0;
};

struct Link {
  std::string a_name, b_name, cigar;
  bool a_fwd = false, b_fwd = false, has_cigar = true;
  uint32_t a_id = UINT32_MAX, b_id = UINT32_MAX;
};

struct Gfa {
  std::string header;
  std::vector<Sequence> sequences;
  std::vector<Link> links;
};

inline bool parse_gfa(const std::string &text, Gfa &g, std::string &err) {
  g = Gfa{};
  for (const std::string &line : split_lines(text)) {
    if (line.size() < 2 || line[1] != '\t') { err = "misformed file; second letter must be tab in line '" + line + "'"; return false; }
    const std::vector<std::string> w = split_words(line);
    if (line[0] == 'H') {
      g.header = line.substr(2);
    } else if (line[0] == 'S') {
      if (w.size() < 4) { err = "S line with " + std::to_string(w.size()) + " fields: '" + line + "'"; return false; }
      Sequence s;
      s.name = w[1]; s.sequence = w[2]; s.features = w[3];
      find_length(s.features, s.length);
      s.id = name_to_id(s.name);
      g.sequences.push_back(s);
    } else if (line[0] == 'L') {
      if (w.size() < 6) { err = "L line with " + std::to_string(w.size()) + " fields: '" + line + "'"; return false; }
      Link l;
      l.a_name = w[1]; l.a_fwd = w[2][0] == '+';
      l.b_name = w[3]; l.b_fwd = w[4][0] == '+';
      l.cigar = w[5];
      l.a_id = name_to_id(l.a_name);
      l.b_id = name_to_id(l.b_name);
      g.links.push_back(l);
    } else {
      err = "unrecognized line '" + line + "'";
      return false;
    }
  }
  return true;
}

// gfaLink::alignmentLength; the warnings it prints are appended to `warn`
inline void alignment_length(const std::string &cigar, int32_t &query_len, int32_t &refce_len,
                             int32_t &align_len, std::string &warn) {
  refce_len = query_len = align_len = 0;
  const char *cp = cigar.c_str();
  if (*cp == '*' || *cp == 0) return;
  do {
    char *end;
    const int64_t val = strtoll(cp, &end, 10);
    cp = end;
    const char code = *cp;
    if (code) cp++;
    char buf[64];
    switch (code) {
      case 'M': case '=': case 'X': refce_len += val; query_len += val; align_len += val; break;
      case 'I': query_len += val; align_len += val; break;
      case 'D': refce_len += val; align_len += val; break;
      case 'N': refce_len += val;  // fall through
      case 'S': case 'H': case 'P':
        snprintf(buf, sizeof buf, "warning - unsupported CIGAR code '%c' in '", code);
        warn += buf + cigar + "'\n";
        break;
      default:
        snprintf(buf, sizeof buf, "unknown CIGAR code '%c' in '", code);
        warn += buf + cigar + "'\n";
        break;
    }
  } while (*cp != 0);
}

inline std::string save_gfa(const Gfa &g) {
  std::string out = "H\t" + g.header + "\n";
  char buf[32];
  for (const Sequence &s : g.sequences) {
    snprintf(buf, sizeof buf, "%u", s.length);
    out += "S\t" + s.name + "\t" + (s.sequence.empty() ? "*" : s.sequence) + "\tLN:i:" + buf + "\n";
  }
  for (const Link &l : g.links)
    out += "L\t" + l.a_name + "\t" + (l.a_fwd ? "+" : "-") + "\t" + l.b_name + "\t" +
           (l.b_fwd ? "+" : "-") + "\t" + (l.has_cigar ? l.cigar : "*") + "\n";
  return out;
}

struct Record {
  std::string a_name, b_name;
  uint32_t a_id = UINT32_MAX, b_id = UINT32_MAX, score = 0;
  int32_t bgn = 0, end = 0;
  bool b_fwd = false;
};

inline bool parse_bed(const std::string &text, std::vector<Record> &recs, std::string &err) {
  recs.clear();
  for (const std::string &line : split_lines(text)) {
    const std::vector<std::string> w = split_words(line);
    if (w.size() < 6) { err = "BED line with " + std::to_string(w.size()) + " fields: '" + line + "'"; return false; }
    Record r;
    r.a_name = w[0];
    r.bgn = (int32_t)strtoll(w[1].c_str(), nullptr, 10);
    r.end = (int32_t)strtoll(w[2].c_str(), nullptr, 10);
    r.b_name = w[3];
    r.score = (uint32_t)strtoll(w[4].c_str(), nullptr, 10);
    r.b_fwd = w[5][0] == '+';
    r.a_id = name_to_id(r.a_name);
    r.b_id = name_to_id(r.b_name);
    recs.push_back(r);
  }
  return true;
}

inline std::string save_bed(const std::vector<Record> &recs) {
  std::string out;
  char buf[64];
  for (const Record &r : recs) {
    snprintf(buf, sizeof buf, "\t%d\t%d\t", r.bgn, r.end);
    out += r.a_name + buf + r.b_name;
    snprintf(buf, sizeof buf, "\t%u\t%c\n", r.score, r.b_fwd ? '+' : '-');
    out += buf;
  }
  return out;
}

// ------------------------------------------------------------------ the tig store

// The data file of a store version: its bytes, or nullptr where there is none.
using DataFile = std::function<const std::vector<uint8_t> *(uint32_t)>;

// The ungapped bases of every tig of an index (empty: deleted, or never written).
inline bool parse_tig_bases(const uint8_t *tig, size_t tig_bytes, const DataFile &data,
                            std::vector<std::string> &out, std::string &err) {
  using namespace tgs;
  out.clear();
  if (tig_bytes < HEADER_BYTES) { err = "tig index of " + std::to_string(tig_bytes) + " bytes has no header"; return false; }
  if (get<uint32_t>(tig) != MASR_MAGIC) { err = "tig index: magic number mismatch"; return false; }
  if (get<uint32_t>(tig + 4) != 1) { err = "tig index: version " + std::to_string(get<uint32_t>(tig + 4)) + ", expected 1"; return false; }
  const uint32_t total = get<uint32_t>(tig + 8), n = get<uint32_t>(tig + 16);
  if (total != n || (uint64_t)n * ENTRY_BYTES + HEADER_BYTES != tig_bytes) {
    err = "tig index: " + std::to_string(n) + " entries (total " + std::to_string(total) +
          ") do not make " + std::to_string(tig_bytes) + " bytes";
    return false;
  }
  out.resize(n);
  for (uint32_t k = 0; k < n; k++) {
    const uint8_t *e = tig + HEADER_BYTES + (size_t)k * ENTRY_BYTES;
    const uint64_t word = get<uint64_t>(e + RECORD_BYTES);
    const uint32_t sv = (uint32_t)((word >> 14) & 1023);
    if (((word >> 13) & 1) || sv == 0) continue;
    const std::string who = "tig " + std::to_string(k);
    const std::vector<uint8_t> *dat = data(sv);
    if (!dat) { err = who + ": no data file of version " + std::to_string(sv); return false; }
    const uint64_t off = word >> 24, dat_bytes = dat->size();
    if (off > dat_bytes || dat_bytes - off < 4 + RECORD_BYTES) { err = who + ": record at " + std::to_string(off) + " past the data file"; return false; }
    const uint8_t *r = dat->data() + off;
    if (memcmp(r, "TIGR", 4) != 0) { err = who + ": no tig record at " + std::to_string(off); return false; }
    r += 4;
    if (get<uint32_t>(r) != k) { err = who + ": the record is of tig " + std::to_string(get<uint32_t>(r)); return false; }
    const uint64_t gapped = get<uint32_t>(r + 32), nch = get<uint32_t>(r + 36), ndelta = get<uint32_t>(r + 40);
    if (gapped != get<uint32_t>(e + 32)) { err = who + ": " + std::to_string(gapped) + " gapped bases in the data file, " + std::to_string(get<uint32_t>(e + 32)) + " in the index"; return false; }
    const uint64_t need = 2 * gapped + nch * POSITION_BYTES + ndelta * 4;
    const uint64_t have = dat_bytes - off - 4 - RECORD_BYTES;
    if (need > have) { err = who + ": " + std::to_string(need) + " bytes of bases, children and deltas, " + std::to_string(have) + " left in the data file"; return false; }
    const uint8_t *b = r + RECORD_BYTES;
    std::string &s = out[k];
    s.reserve(gapped);
    for (uint64_t i = 0; i < gapped; i++)
      if (b[i] != '-') s.push_back((char)b[i]);
  }
  return true;
}

inline bool file_exists(const std::string &path) {
  FILE *f = fopen(path.c_str(), "rb");
  if (f) fclose(f);
  return f != nullptr;
}

// tgStore(path, version) for reading: the index of `version`, or of the nearest version below
// that has one, and the data files its entries name.
inline bool load_tig_bases(const std::string &path, uint32_t version, std::vector<std::string> &out,
                           std::string &err) {
  char name[64];
  uint32_t v = version > 1023 ? 1023 : version;
  for (; v > 0; v--) {
    snprintf(name, sizeof name, "/seqDB.v%03u.tig", v);
    if (file_exists(path + name)) break;
  }
  if (v == 0) { err = "failed to find any tigs in store '" + path + "'"; return false; }
  std::vector<uint8_t> tig;
  if (!tgs::slurp(path + name, tig, err)) return false;
  std::map<uint32_t, std::vector<uint8_t>> files;
  std::map<uint32_t, bool> missing;
  const DataFile data = [&](uint32_t sv) -> const std::vector<uint8_t> * {
    if (missing.count(sv)) return nullptr;
    auto it = files.find(sv);
    if (it != files.end()) return &it->second;
    char dn[64];
    snprintf(dn, sizeof dn, "/seqDB.v%03u.dat", sv);
    std::string e;
    std::vector<uint8_t> bytes;
    if (!tgs::slurp(path + dn, bytes, e)) { missing[sv] = true; return nullptr; }
    return &(files[sv] = std::move(bytes));
  };
  return parse_tig_bases(tig.data(), tig.size(), data, out, err);
}

}  // namespace gfa_files

#endif
