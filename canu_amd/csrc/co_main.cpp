// co_main.cpp -- canu_amd/bin/correctOverlaps: the command line canu's oea.sh runs
// (OverlapErrorAdjustment.pm:509-517), over libcanu_co.so.
//
//   correctOverlaps -G asm.gkpStore -O asm.ovlStore -R bgn end -e erate -l minlen
//                   -c red.red -o N.oea [-t T]
//
// Options as correctOverlaps.C:52-121.  -l and -t are accepted and change nothing (they are
// parsed and never used there either).  CANU_CO_DEVICE picks the GPU.  Only the reads of the
// range and the B reads its overlaps name are loaded.  The output is the .oea file and, on
// stderr, the reference's "Corrected" line and its nine counters (CANU_CO_VERBOSE adds the
// kernel times).
//
// A store with an `evalues` file is refused: the reference would read the overlaps' evalues
// from it, and canu never runs this step on such a store.  A range with no overlaps writes a
// header with n = 0 (the reference indexes olaps[-1] there, correctOverlaps-Redo_Olaps.C:279).
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/canu_co.h"
#include "co_files.h"
#include "gkp_store.h"
#include "ovs_reader.h"

static int usage(const char *argv0) {
  fprintf(stderr, "usage: %s -G gkpStore -O ovlStore -R bgnID endID -c file.red -o file.oea [options]\n", argv0);
  fprintf(stderr, "  -e erate   error rate of the overlaps (0.06)\n");
  fprintf(stderr, "  -l n, -t n accepted, ignored\n");
  return 1;
}

int main(int argc, char **argv) {
  const char *gkp_name = nullptr, *ovl_name = nullptr, *red_name = nullptr, *out_name = nullptr;
  uint32_t bgn = 0, end = UINT32_MAX;
  co_params P;
  co_params_init(&P);
  int err = 0;
  for (int arg = 1; arg < argc; arg++) {
    const char *a = argv[arg];
    auto value = [&]() -> const char * {
      if (arg + 1 >= argc) { err++; return "0"; }
      return argv[++arg];
    };
    if (!strcmp(a, "-G")) gkp_name = value();
    else if (!strcmp(a, "-O")) ovl_name = value();
    else if (!strcmp(a, "-c")) red_name = value();
    else if (!strcmp(a, "-o")) out_name = value();
    else if (!strcmp(a, "-R")) { bgn = (uint32_t)atoi(value()); end = (uint32_t)atoi(value()); }
    else if (!strcmp(a, "-e")) P.error_rate = atof(value());
    else if (!strcmp(a, "-l")) value();
    else if (!strcmp(a, "-t")) value();
    else { fprintf(stderr, "Unknown option '%s'\n", a); err++; }
  }
  if (!gkp_name) { fprintf(stderr, "ERROR: no input gatekeeper store (-G) supplied.\n"); err++; }
  if (!ovl_name) { fprintf(stderr, "ERROR: no input overlap store (-O) supplied.\n"); err++; }
  if (!red_name) { fprintf(stderr, "ERROR: no input read corrections file (-c) supplied.\n"); err++; }
  if (!out_name) { fprintf(stderr, "ERROR: no output erates file (-o) supplied.\n"); err++; }
  if (err) return usage(argv[0]);

  std::string msg;
  gkp::Store gkp;
  if (!gkp.open(gkp_name, msg)) {
    fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
    return 1;
  }
  if (bgn < 1) bgn = 1;                                         // correctOverlaps.C:146-150
  if (gkp.num_reads() < end) end = gkp.num_reads();
  if (bgn > end) {
    fprintf(stderr, "%s: no reads in the range %u-%u (the store has %u)\n", argv[0], bgn, end,
            gkp.num_reads());
    return 1;
  }
  {
    uint64_t sz = 0;
    if (ovs::file_size(std::string(ovl_name) + "/evalues", sz)) {
      fprintf(stderr, "%s: '%s' has an evalues file: its overlaps' error rates were adjusted "
              "already, and this step runs on a store without one\n", argv[0], ovl_name);
      return 1;
    }
  }
  ovs::Store store;
  std::vector<ovl_record> recs;
  if (!store.open(ovl_name, msg) || !store.read_range(bgn, end, recs, msg)) {
    fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
    return 1;
  }
  std::vector<fe_correction> red;
  if (!cofiles::read_red(red_name, red, msg)) {
    fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
    return 1;
  }
  fprintf(stderr, "Reading %zu corrections from '%s'.\n", red.size(), red_name);
  fprintf(stderr, "Read_Olaps()--  Loaded %zu overlaps.\n", recs.size());

  cofiles::Oea out;
  out.bgn_id = bgn;
  out.end_id = end;
  if (recs.empty()) {
    if (!cofiles::write_oea(out_name, out, msg)) {
      fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
      return 1;
    }
    fprintf(stderr, "No overlaps in the range %u-%u: '%s' holds none.\n\nBye.\n", bgn, end, out_name);
    return 0;
  }

  // the reads of the range and the B reads, as one ID range whose other reads are empty
  uint32_t lo = bgn, hi = end;
  for (const ovl_record &r : recs) {
    if (r.b_iid == 0 || r.b_iid > gkp.num_reads()) {
      fprintf(stderr, "%s: an overlap names read %u; the store has reads 1..%u\n", argv[0], r.b_iid,
              gkp.num_reads());
      return 1;
    }
    lo = r.b_iid < lo ? r.b_iid : lo;
    hi = r.b_iid > hi ? r.b_iid : hi;
  }
  const uint32_t n = hi - lo + 1;
  std::vector<uint8_t> named(n, 0);
  for (uint32_t i = bgn; i <= end; i++) named[i - lo] = 1;
  for (const ovl_record &r : recs) named[r.b_iid - lo] = 1;
  std::vector<uint32_t> lens(n, 0);
  std::vector<uint64_t> offs(n, 0);
  std::string bases, seq, qlt;
  for (uint32_t i = 0; i < n; i++) {
    offs[i] = bases.size();
    if (!named[i]) continue;
    if (!gkp.load(lo + i, seq, qlt, msg)) {
      fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
      return 1;
    }
    lens[i] = (uint32_t)seq.size();
    bases += seq;
  }

  int device = 0;
  if (const char *d = getenv("CANU_CO_DEVICE")) device = atoi(d);
  co_ctx *ctx = nullptr;
  out.evalues.resize(recs.size());
  if (co_ctx_create(&P, device, &ctx) != CO_OK ||
      co_load_reads(ctx, lo, n, (const uint8_t *)bases.data(), offs.data(), lens.data()) != CO_OK ||
      co_set_corrections(ctx, red.data(), red.size()) != CO_OK ||
      co_correct_overlaps(ctx, bgn, end, recs.data(), recs.size(), out.evalues.data()) != CO_OK ||
      co_write_oea(ctx, out_name) != CO_OK) {
    fprintf(stderr, "%s: %s\n", argv[0], co_last_error());
    co_ctx_destroy(ctx);
    return 1;
  }
  co_stats S;
  co_get_stats(ctx, &S);
  co_ctx_destroy(ctx);

  typedef unsigned long long ull;
  fprintf(stderr, "Corrected %llu bases with %llu substitutions, %llu deletions and %llu insertions.\n",
          (ull)S.corrected_bases, (ull)S.substitutions, (ull)S.deletions, (ull)S.insertions);
  fprintf(stderr, "Olaps Fwd %llu\n", (ull)S.olaps_fwd);          // correctOverlaps-Redo_Olaps.C:543-552
  fprintf(stderr, "Olaps Rev %llu\n", (ull)S.olaps_rev);
  fprintf(stderr, "Total:  %llu\n", (ull)S.total);
  fprintf(stderr, "Failed: %llu (both)\n", (ull)S.failed_both);
  fprintf(stderr, "Failed: %llu (either)\n", (ull)S.failed_either);
  fprintf(stderr, "Failed: %llu (match to end)\n", (ull)S.failed_end);
  fprintf(stderr, "Failed: %llu (negative length)\n", (ull)S.failed_length);
  fprintf(stderr, "rhaFail %llu rhaPass %llu\n", (ull)S.rha_fail, (ull)S.rha_pass);
  if (getenv("CANU_CO_VERBOSE"))
    fprintf(stderr, " -- %.3f ms in k_co_correct, %.3f ms in k_co_align, %llu rows, %llu re-run(s)\n",
            S.ms_correct, S.ms_align, (ull)S.rows, (ull)S.regrows);
  fprintf(stderr, "\nBye.\n");
  return 0;
}
