// tr_files.h -- what canu_amd/bin/trimReads reads and writes beside the two stores (host C++17,
// no dependency): its command line, the gkpStore's `libraries` file, the clear range file
// (src/overlapBasedTrimming/clearRangeFile.H), the log and the stats text (trimReads.C:245,
// 382-435, 469-504).  tests/tr_host_check.cpp runs all of it under the sanitizers.
#ifndef CANU_TR_FILES_H
#define CANU_TR_FILES_H

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/canu_tr.h"

namespace trf {

struct Job {
  const char *gkp = nullptr, *ovl = nullptr, *clear = nullptr, *out = nullptr;
  uint32_t id_min = 1, id_max = UINT32_MAX;
  tr_params P;
};

// AS_UTL_decodeRange: "a" or "a-b".
inline void decode_range(const char *s, uint32_t &lo, uint32_t &hi) {
  char *e = nullptr;
  lo = hi = (uint32_t)strtoull(s, &e, 10);
  if (e && *e == '-') hi = (uint32_t)strtoull(e + 1, nullptr, 10);
}

// trimReads.C:145-218.  False with a one-line message: an unknown option, an option without its
// value, one of -Ci / -Cm / -l (not supported: canu never passes them, the reference's usage
// calls them unsupported and its asserts can fire with them), or no -G / -O / -Co / -o (without
// -Co the reference dereferences NULL).
inline bool parse_args(int argc, const char *const *argv, Job &J, std::string &err) {
  tr_params &P = J.P;
  P.erate = 0.015;
  P.min_read_length = 64;
  P.min_evidence_overlap = 40;
  P.min_evidence_coverage = 1;
  for (int arg = 1; arg < argc; arg++) {
    const char *a = argv[arg];
    const bool known = !strcmp(a, "-G") || !strcmp(a, "-O") || !strcmp(a, "-Co") || !strcmp(a, "-o") ||
                       !strcmp(a, "-e") || !strcmp(a, "-minlength") || !strcmp(a, "-ol") ||
                       !strcmp(a, "-oc") || !strcmp(a, "-t");
    if (!strcmp(a, "-Ci") || !strcmp(a, "-Cm") || !strcmp(a, "-l")) {
      err = std::string("option ") + a + " is not supported";
      return false;
    }
    if (!known) { err = std::string("unknown option '") + a + "'"; return false; }
    if (arg + 1 >= argc) { err = std::string("option ") + a + " needs a value"; return false; }
    const char *v = argv[++arg];
    if (!strcmp(a, "-G")) J.gkp = v;
    else if (!strcmp(a, "-O")) J.ovl = v;
    else if (!strcmp(a, "-Co")) J.clear = v;
    else if (!strcmp(a, "-o")) J.out = v;
    else if (!strcmp(a, "-e")) P.erate = atof(v);
    else if (!strcmp(a, "-minlength")) P.min_read_length = (uint32_t)atoi(v);
    else if (!strcmp(a, "-ol")) P.min_evidence_overlap = (uint32_t)atoi(v);
    else if (!strcmp(a, "-oc")) P.min_evidence_coverage = (uint32_t)atoi(v);
    else decode_range(v, J.id_min, J.id_max);
  }
  if (!J.gkp) { err = "no gatekeeper store (-G) given"; return false; }
  if (!J.ovl) { err = "no overlap store (-O) given"; return false; }
  if (!J.clear) { err = "no output clear range file (-Co) given"; return false; }
  if (!J.out) { err = "no output prefix (-o) given"; return false; }
  return true;
}

// <gkpStore>/libraries: gkLibrary[numLibraries + 1] of 168 bytes (128 of name, ten uint32);
// _finalTrim is the fifth uint32 (gkStore.H:168-181).  -> finalTrim of library 0 .. num_libraries.
inline bool parse_libraries(const std::vector<uint8_t> &raw, uint32_t num_libraries,
                            std::vector<uint32_t> &final_trim, std::string &err) {
  const size_t rec = 168, at = 128 + 4 * 4;
  if (raw.size() < rec * ((size_t)num_libraries + 1)) {
    err = "the libraries file is " + std::to_string(raw.size()) + " bytes, " +
          std::to_string(num_libraries) + " libraries need " + std::to_string(rec * ((size_t)num_libraries + 1));
    return false;
  }
  final_trim.assign(num_libraries + 1, 0);
  for (uint32_t l = 0; l <= num_libraries; l++) memcpy(&final_trim[l], raw.data() + rec * l + at, 4);
  return true;
}

inline bool read_file(const std::string &path, std::vector<uint8_t> &raw) {
  FILE *F = fopen(path.c_str(), "rb");
  if (!F) return false;
  raw.clear();
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, F)) > 0) raw.insert(raw.end(), buf, buf + n);
  fclose(F);
  return true;
}

// A clear range file: uint32 numReads, bgn[numReads + 1], end[numReads + 1].
inline bool parse_clear(const std::vector<uint8_t> &raw, uint32_t num_reads, std::vector<uint32_t> &bgn,
                        std::vector<uint32_t> &end, std::string &err) {
  if (raw.size() < 4) { err = "a clear range file of " + std::to_string(raw.size()) + " bytes has no read count"; return false; }
  uint32_t n;
  memcpy(&n, raw.data(), 4);
  if (n != num_reads) {
    err = "a clear range file for " + std::to_string(n) + " reads, the store has " + std::to_string(num_reads);
    return false;
  }
  if (raw.size() != 4 + 8 * ((size_t)n + 1)) {
    err = "a clear range file of " + std::to_string(raw.size()) + " bytes does not hold its " + std::to_string(n) + " reads";
    return false;
  }
  bgn.resize((size_t)n + 1);
  end.resize((size_t)n + 1);
  memcpy(bgn.data(), raw.data() + 4, 4 * ((size_t)n + 1));
  memcpy(end.data(), raw.data() + 4 + 4 * ((size_t)n + 1), 4 * ((size_t)n + 1));
  return true;
}

// The -Co file after the run: 0 .. length for a read left alone, UINT32_MAX twice for a deleted
// one; entry 0 is what an existing file held there, else 0.
inline std::vector<uint8_t> clear_bytes(uint32_t num_reads, const uint32_t *lengths, const tr_result &R,
                                        uint32_t bgn0, uint32_t end0) {
  std::vector<uint32_t> v(1 + 2 * ((size_t)num_reads + 1));
  uint32_t *bgn = v.data() + 1, *end = bgn + num_reads + 1;
  v[0] = num_reads;
  bgn[0] = bgn0;
  end[0] = end0;
  for (uint32_t i = 0; i < num_reads; i++) {
    const uint8_t st = R.status[i];
    const bool gone = st == TR_NOV || st == TR_DEL, mod = st == TR_MOD;
    bgn[i + 1] = gone ? UINT32_MAX : mod ? R.bgn[i] : 0;
    end[i + 1] = gone ? UINT32_MAX : mod ? R.end[i] : lengths[i];
  }
  std::vector<uint8_t> out(v.size() * 4);
  memcpy(out.data(), v.data(), out.size());
  return out;
}

inline std::string log_text(uint32_t id_min, uint32_t id_max, const uint32_t *lengths, const tr_result &R) {
  std::string out = "id\tinitL\tinitR\tfinalL\tfinalR\tmessage (DEL=deleted NOC=no change MOD=modified)\n";
  static const char *tag[] = {"", "NOV", "DEL", "NOC", "MOD"};
  char line[256];
  for (uint32_t id = id_min; id <= id_max && id >= 1; id++) {
    const uint32_t i = id - 1;
    const uint8_t st = R.status[i] <= TR_MOD ? R.status[i] : 0;
    int n = snprintf(line, sizeof line, "%u\t%u\t%u\t%u\t%u\t%s", id, 0u, lengths[i], R.bgn[i], R.end[i], tag[st]);
    if (st != TR_NOV) {
      if (R.flags[i] & TR_FLAG_NO_HQ)
        n += snprintf(line + n, sizeof line - n, "\tno high quality overlaps");
      else
        n += snprintf(line + n, sizeof line - n, "\tskipped %u overlaps; used %u overlaps", R.n_skipped[i], R.n_used[i]);
    }
    out.append(line, (size_t)n);
    out += '\n';
  }
  return out;
}

inline uint32_t encode_evalue(double q) { return q < 0.4095 ? (uint32_t)(10000.0 * q + 0.5) : 4095u; }

inline std::string stats_text(const tr_params &P, const tr_stats &S) {
  std::string out;
  char line[256];
  auto put = [&](int n) { out.append(line, (size_t)n); };
  auto row = [&](const tr_count &c, const char *what) {
    put(snprintf(line, sizeof line, "%6u reads %12llu bases (%s)\n", (unsigned)c.reads, (unsigned long long)c.bases, what));
  };
  out += "PARAMETERS:\n----------\n";
  put(snprintf(line, sizeof line, "%7u    (reads trimmed below this many bases are deleted)\n", P.min_read_length));
  put(snprintf(line, sizeof line, "%7.4f    (use overlaps at or below this fraction error)\n", encode_evalue(P.erate) / 10000.0));
  put(snprintf(line, sizeof line, "%7u    (break region if overlap is less than this long, for 'largest covered' algorithm)\n", P.min_evidence_overlap));
  put(snprintf(line, sizeof line, "%7u    (break region if overlap coverage is less than this many read%s, for 'largest covered' algorithm)\n",
               P.min_evidence_coverage, P.min_evidence_coverage == 1 ? "" : "s"));
  out += "\nINPUT READS:\n-----------\n";
  row(S.reads_in, "reads processed");
  row(S.deleted_in, "reads not processed, previously deleted");
  row(S.no_trim_in, "reads not processed, in a library where trimming isn't allowed");
  out += "\nOUTPUT READS:\n------------\n";
  row(S.reads_out, "trimmed reads output");
  row(S.no_change_out, "reads with no change, kept as is");
  row(S.no_ovl_out, "reads with no overlaps, deleted");
  row(S.deleted_out, "reads with short trimmed length, deleted");
  out += "\nTRIMMING DETAILS:\n----------------\n";
  row(S.trim5, "bases trimmed from the 5' end of a read");
  row(S.trim3, "bases trimmed from the 3' end of a read");
  return out;
}

inline bool write_file(const std::string &path, const void *data, size_t n) {
  FILE *F = fopen(path.c_str(), "wb");
  if (!F) return false;
  const bool ok = (n == 0 || fwrite(data, 1, n, F) == n);
  return (fclose(F) == 0) && ok;
}

}  // namespace trf

#endif
