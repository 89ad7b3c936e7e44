// pair_main.cpp -- canu_amd/bin/overlapPair: the command line canu's mhap.sh runs after
// mhapConvert (OverlapMhap.pm:522-537), over libcanu_pair.so.
//
//   overlapPair -G asm.gkpStore -O results/N.mhap.ovb -o results/N.WORKING.ovb
//               [-partial] -len L -erate E -memory M -t T [-invert] [-b id] [-e id]
//
// Options as overlapPair.C:690-729.  -memory and -t are accepted and ignored (the reads named
// by the file are device resident; the device schedules the work); -b / -e only restrict an
// ovStore input, which is refused: canu passes files.  The output is the .ovb and the
// "<base>.counts" file ovFile(..., ovFileFullWrite) leaves, and reportFinal's lines on stderr.
#include <sys/stat.h>

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/canu_pair.h"
#include "gkp_store.h"
#include "ovb_reader.h"
#include "ovl_ovb.h"

static int usage(const char *argv0) {
  fprintf(stderr, "usage: %s ...\n", argv0);
  fprintf(stderr, "  -G gkpStore     Mandatory, path to gkpStore\n");
  fprintf(stderr, "  -O ovlFile      overlaps to realign (an .ovb file; an ovStore is not supported)\n");
  fprintf(stderr, "  -o ovlFile      output .ovb\n");
  fprintf(stderr, "  -erate e        Overlaps are computed at 'e' fraction error\n");
  fprintf(stderr, "  -len l          Minimum overlap length, 1 or more\n");
  fprintf(stderr, "  -partial        Overlaps are 'overlapInCore -G' partial overlaps\n");
  fprintf(stderr, "  -memory m       accepted, ignored\n");
  fprintf(stderr, "  -t n            accepted, ignored\n");
  fprintf(stderr, "  -invert         Invert the overlap A <-> B before aligning\n");
  return 1;
}

int main(int argc, char **argv) {
  const char *gkp_name = nullptr, *ovl_name = nullptr, *out_name = nullptr;
  pair_params P;
  pair_params_init(&P);
  P.min_overlap_length = 0;                      // the reference's default; refused below
  int err = 0;
  for (int arg = 1; arg < argc; arg++) {
    const char *a = argv[arg];
    auto value = [&]() -> const char * {
      if (arg + 1 >= argc) { err++; return "0"; }
      return argv[++arg];
    };
    if (!strcmp(a, "-G")) gkp_name = value();
    else if (!strcmp(a, "-O")) ovl_name = value();
    else if (!strcmp(a, "-o")) out_name = value();
    else if (!strcmp(a, "-b") || !strcmp(a, "-e") || !strcmp(a, "-t") || !strcmp(a, "-memory"))
      value();                                   // taken and not used
    else if (!strcmp(a, "-erate")) P.max_erate = atof(value());
    else if (!strcmp(a, "-len")) P.min_overlap_length = (uint32_t)atoi(value());
    else if (!strcmp(a, "-partial")) P.partial = 1;
    else if (!strcmp(a, "-invert")) P.invert = 1;
    else err++;
  }
  if (!gkp_name || !ovl_name || !out_name) err++;
  if (err) return usage(argv[0]);
  if (P.min_overlap_length == 0) {
    fprintf(stderr, "%s: -len 0 (or no -len) is not supported: the reference hands its aligner "
                    "empty spans there.  Give -len 1 or more, as canu does.\n", argv[0]);
    return 1;
  }
  struct stat sb;
  if (stat(ovl_name, &sb) == 0 && S_ISDIR(sb.st_mode)) {
    fprintf(stderr, "%s: '%s' is a directory: ovStore input is not supported, give the .ovb "
                    "file.\n", argv[0], ovl_name);
    return 1;
  }

  std::string msg;
  gkp::Store store;
  if (!store.open(gkp_name, msg)) {
    fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
    return 1;
  }
  fprintf(stderr, "Reading overlaps from file '%s' and writing to '%s'\n", ovl_name, out_name);
  std::vector<ovl_record> recs;
  if (!ovb::read_ovb_file(ovl_name, recs, msg)) {
    fprintf(stderr, "%s: '%s': %s\n", argv[0], ovl_name, msg.c_str());
    return 1;
  }
  fprintf(stderr, "Loaded %zu overlaps.\n", recs.size());

  // the reads the file names (overlapReadCache::loadReads), as one ID range whose other
  // reads are empty
  uint32_t lo = UINT32_MAX, hi = 0;
  for (const ovl_record &r : recs) {
    for (uint32_t id : {r.a_iid, r.b_iid}) {
      if (id == 0 || id > store.num_reads()) {
        fprintf(stderr, "%s: an overlap names read %u; the store has reads 1..%u\n", argv[0], id,
                store.num_reads());
        return 1;
      }
      lo = id < lo ? id : lo;
      hi = id > hi ? id : hi;
    }
  }
  pair_ctx *ctx = nullptr;
  if (pair_ctx_create(&P, 0, &ctx) != PAIR_OK) {
    fprintf(stderr, "%s: %s\n", argv[0], pair_last_error());
    return 1;
  }
  if (!recs.empty()) {
    const uint32_t n = hi - lo + 1;
    std::vector<uint8_t> named(n, 0);
    for (const ovl_record &r : recs) named[r.a_iid - lo] = named[r.b_iid - lo] = 1;
    std::vector<uint32_t> lens(n, 0);
    std::vector<uint64_t> offs(n, 0);
    std::string bases, seq, qlt;
    for (uint32_t i = 0; i < n; i++) {
      offs[i] = bases.size();
      if (!named[i]) continue;
      if (!store.load(lo + i, seq, qlt, msg)) {
        fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
        return 1;
      }
      lens[i] = (uint32_t)seq.size();
      bases += seq;
    }
    if (pair_load_reads(ctx, lo, n, (const uint8_t *)bases.data(), offs.data(), lens.data()) !=
        PAIR_OK) {
      fprintf(stderr, "%s: %s\n", argv[0], pair_last_error());
      return 1;
    }
    if (pair_realign(ctx, recs.data(), recs.size(), recs.data()) != PAIR_OK) {
      fprintf(stderr, "%s: %s\n", argv[0], pair_last_error());
      return 1;
    }
  }
  pair_stats S;
  pair_get_stats(ctx, &S);
  pair_ctx_destroy(ctx);

  if (ovl::write_ovb_file(recs.data(), recs.size(), out_name, true) != 0) {
    fprintf(stderr, "%s: can't write '%s': %s\n", argv[0], out_name, strerror(errno));
    return 1;
  }

  // alignStats::reportFinal (overlapPair.C:138-153)
  const unsigned long np = S.n_passed, nf = S.n_failed;
  fprintf(stderr, "\n");
  fprintf(stderr, " -- %lu overlaps processed.\n", np + nf);
  fprintf(stderr, " -- %lu skipped.\n", (unsigned long)S.n_skipped);
  fprintf(stderr, " -- %lu failed %lu passed (%.4f%%).\n", nf, np, 100.0 * np / (np + nf));
  fprintf(stderr, " --\n");
  fprintf(stderr, " -- %lu failed initial alignment, allowing A to extend\n", (unsigned long)S.n_fail_ext_a);
  fprintf(stderr, " -- %lu failed initial alignment, allowing B to extend\n", (unsigned long)S.n_fail_ext_b);
  fprintf(stderr, " -- %lu failed initial alignment\n", (unsigned long)S.n_fail_ext);
  fprintf(stderr, " --\n");
  fprintf(stderr, " -- %lu partial overlaps (of any quality)\n", (unsigned long)S.n_partial);
  fprintf(stderr, " -- %lu dovetail overlaps (before extensions, of any quality)\n", (unsigned long)S.n_dovetail);
  fprintf(stderr, " --\n");
  fprintf(stderr, " -- %lu/%lu A read dovetail extensions\n", (unsigned long)S.n_ext5a, (unsigned long)S.n_ext3a);
  fprintf(stderr, " -- %lu/%lu B read dovetail extensions\n", (unsigned long)S.n_ext5b, (unsigned long)S.n_ext3b);
  fprintf(stderr, " -- %.3f ms in k_pair, %lu DP cells\n", S.ms_kernel, (unsigned long)S.dp_cells);
  return 0;
}
