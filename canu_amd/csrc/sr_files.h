// sr_files.h -- what canu_amd/bin/splitReads reads and writes beside the two stores (host C++17,
// no dependency): its command line (splitReads.C:120-180), the three switches of the gkpStore's
// `libraries` file, the clear range files (through tr_files.h's reader) and the stats text
// (splitReads.C:409-445).  tests/sr_host_check.cpp runs all of it under the sanitizers.
#ifndef CANU_SR_FILES_H
#define CANU_SR_FILES_H

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/canu_sr.h"
#include "tr_files.h"

namespace srf {

using trf::parse_clear;
using trf::read_file;
using trf::write_file;

struct Job {
  const char *gkp = nullptr, *ovl = nullptr, *clear_in = nullptr, *clear = nullptr, *out = nullptr;
  uint32_t id_min = 0, id_max = UINT32_MAX;
  sr_params P;
};

// False with a one-line message: an unknown option, an option without its value, a negative -e,
// or no -G / -O / -Co / -o (without -Co the reference dereferences NULL).  No -Ci leaves clear_in
// null: every read starts at 0 .. length (the reference crashes in strcpy(NULL) there).
inline bool parse_args(int argc, const char *const *argv, Job &J, std::string &err) {
  sr_params &P = J.P;
  P.erate = 0.015;
  P.min_read_length = 64;
  for (int arg = 1; arg < argc; arg++) {
    const char *a = argv[arg];
    const bool known = !strcmp(a, "-G") || !strcmp(a, "-O") || !strcmp(a, "-Ci") || !strcmp(a, "-Co") ||
                       !strcmp(a, "-o") || !strcmp(a, "-e") || !strcmp(a, "-minlength") || !strcmp(a, "-t");
    if (!known) { err = std::string("unknown option '") + a + "'"; return false; }
    if (arg + 1 >= argc) { err = std::string("option ") + a + " needs a value"; return false; }
    const char *v = argv[++arg];
    if (!strcmp(a, "-G")) J.gkp = v;
    else if (!strcmp(a, "-O")) J.ovl = v;
    else if (!strcmp(a, "-Ci")) J.clear_in = v;
    else if (!strcmp(a, "-Co")) J.clear = v;
    else if (!strcmp(a, "-o")) J.out = v;
    else if (!strcmp(a, "-e")) P.erate = atof(v);
    else if (!strcmp(a, "-minlength")) P.min_read_length = (uint32_t)atoi(v);
    else trf::decode_range(v, J.id_min, J.id_max);
  }
  if (P.erate < 0.0) { err = "error rate (-e) too small; must be 'fraction error' and above 0.0"; return false; }
  if (!J.gkp) { err = "no gatekeeper store (-G) given"; return false; }
  if (!J.ovl) { err = "no overlap store (-O) given"; return false; }
  if (!J.clear) { err = "no output clear range file (-Co) given"; return false; }
  if (!J.out) { err = "no output prefix (-o) given"; return false; }
  return true;
}

// <gkpStore>/libraries: gkLibrary[numLibraries + 1] of 168 bytes (128 of name, ten uint32);
// _removeSpurReads, _removeChimericReads and _checkForSubReads are the seventh to ninth uint32
// (gkStore.H:168-196).  -> SR_LIB_* of library 0 .. num_libraries.
inline bool parse_libraries(const std::vector<uint8_t> &raw, uint32_t num_libraries,
                            std::vector<uint8_t> &flags, std::string &err) {
  const size_t rec = 168, at = 128 + 4 * 6;
  if (raw.size() < rec * ((size_t)num_libraries + 1)) {
    err = "the libraries file is " + std::to_string(raw.size()) + " bytes, " +
          std::to_string(num_libraries) + " libraries need " + std::to_string(rec * ((size_t)num_libraries + 1));
    return false;
  }
  flags.assign((size_t)num_libraries + 1, 0);
  for (uint32_t l = 0; l <= num_libraries; l++) {
    uint32_t sw[3];
    memcpy(sw, raw.data() + rec * l + at, sizeof sw);
    flags[l] = (uint8_t)(((sw[0] || sw[1] || sw[2]) ? SR_LIB_ELIGIBLE : 0) | (sw[2] ? SR_LIB_SUBREADS : 0));
  }
  return true;
}

// The -Co file after the run: the input range, the trimmed one, or UINT32_MAX twice for a read
// deleted here; cb / ce the input clear ranges (entry i for read i + 1), entry 0 the -Ci file's.
inline std::vector<uint8_t> clear_bytes(uint32_t num_reads, const uint32_t *cb, const uint32_t *ce,
                                        const sr_result &R, uint32_t bgn0, uint32_t end0) {
  std::vector<uint32_t> v(1 + 2 * ((size_t)num_reads + 1));
  uint32_t *bgn = v.data() + 1, *end = bgn + num_reads + 1;
  v[0] = num_reads;
  bgn[0] = bgn0;
  end[0] = end0;
  for (uint32_t i = 0; i < num_reads; i++) {
    const uint8_t st = R.status[i];
    bgn[i + 1] = st == SR_DELETED_OUT ? UINT32_MAX : st == SR_TRIMMED ? R.bgn[i] : cb[i];
    end[i + 1] = st == SR_DELETED_OUT ? UINT32_MAX : st == SR_TRIMMED ? R.end[i] : ce[i];
  }
  std::vector<uint8_t> out(v.size() * 4);
  memcpy(out.data(), v.data(), out.size());
  return out;
}

inline std::string stats_text(const sr_params &P, const sr_stats &S) {
  std::string out;
  char line[256];
  auto put = [&](int n) { out.append(line, (size_t)n); };
  auto row = [&](const sr_count &c, const char *what, const char *unit = "bases") {
    put(snprintf(line, sizeof line, "%6u reads %12llu %s (%s)\n", (unsigned)c.reads, (unsigned long long)c.bases, unit, what));
  };
  out += "PARAMETERS:\n----------\n";
  put(snprintf(line, sizeof line, "%7u    (reads trimmed below this many bases are deleted)\n", P.min_read_length));
  put(snprintf(line, sizeof line, "%7.4f    (use overlaps at or below this fraction error)\n", P.erate));
  out += "INPUT READS:\n-----------\n";
  row(S.reads_in, "reads processed");
  row(S.deleted_in, "reads not processed, previously deleted");
  row(S.no_trim_in, "reads not processed, in a library where trimming isn't allowed");
  out += "\nPROCESSED:\n--------\n";
  row(S.no_overlaps, "no overlaps");
  row(S.no_coverage, "no coverage after adjusting for trimming done already");
  row(S.proc_chimera, "processed for chimera");
  row(S.proc_spur, "processed for spur");
  row(S.proc_subread, "processed for subreads");
  out += "\nREADS WITH SIGNALS:\n------------------\n";
  row(S.reads_bad_spur5, "number of 5' spur signal", "signals");
  row(S.reads_bad_spur3, "number of 3' spur signal", "signals");
  row(S.reads_bad_chimera, "number of chimera signal", "signals");
  row(S.reads_bad_subread, "number of subread signal", "signals");
  out += "\nSIGNALS:\n-------\n";
  row(S.bases_bad_spur5, "size of 5' spur signal");
  row(S.bases_bad_spur3, "size of 3' spur signal");
  row(S.bases_bad_chimera, "size of chimera signal");
  row(S.bases_bad_subread, "size of subread signal");
  out += "\nTRIMMING:\n--------\n";
  row(S.trimmed5, "trimmed from the 5' end of the read");
  row(S.trimmed3, "trimmed from the 3' end of the read");
  return out;
}

// detectSubReads' ERROR lines, in record order.
inline std::string error_lines(const ovl_record *recs, uint64_t n, const uint8_t *fate) {
  std::string out;
  char line[128];
  for (uint64_t i = 0; i < n; i++) {
    if (fate[i] == SR_FATE_MANY)
      out.append(line, (size_t)snprintf(line, sizeof line, "ERROR: more overlaps than expected for pair %u %u.\n",
                                        recs[i].a_iid, recs[i].b_iid));
    else if (fate[i] == SR_FATE_SAME_ORIENT)
      out.append(line, (size_t)snprintf(line, sizeof line, "ERROR: same orient duplicate overlaps for pair %u %u\n",
                                        recs[i].a_iid, recs[i].b_iid));
  }
  return out;
}

}  // namespace srf

#endif
