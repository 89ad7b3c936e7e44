// fe_main.cpp -- canu_amd/bin/findErrors: the command line canu's red.sh runs
// (OverlapErrorAdjustment.pm:194-202), over libcanu_fe.so.
//
//   findErrors -G asm.gkpStore -O asm.ovlStore -R bgn end -e erate -l minlen -o N.red -t T
//              [-d degree] [-k kmerlen] [-p] [-V votelen] [-x excludelen]
//
// Options as findErrors.C:381-425.  -t and -l are accepted and change nothing (-l is parsed and
// never used there either).  CANU_FE_DEVICE picks the GPU.  Only the reads of the range and the
// B reads its overlaps name are loaded.  The output is the .red file and the reference's two
// "Passed overlaps" / "Failed overlaps" lines on stderr (CANU_FE_VERBOSE adds the overlap count
// and the kernel times).  A range with no overlaps writes its
// IDENT records (the reference reads olaps[0] of an empty list there, findErrors.C:281).
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/canu_fe.h"
#include "gkp_store.h"
#include "ovs_reader.h"

static int usage(const char *argv0) {
  fprintf(stderr, "usage: %s -G gkpStore -O ovlStore -R bgnID endID -o file.red [options]\n", argv0);
  fprintf(stderr, "  -e erate   error rate of the overlaps (0.06)\n");
  fprintf(stderr, "  -d n       set keep flag on end of reads with less than this many overlaps (2)\n");
  fprintf(stderr, "  -k n       minimum exact-match region to prevent change (9)\n");
  fprintf(stderr, "  -p         don't use haplotype counts to correct\n");
  fprintf(stderr, "  -V n       number of exact match bases around an error to vote to change (9)\n");
  fprintf(stderr, "  -x n       length of end of exact match to exclude in preventing change (3)\n");
  fprintf(stderr, "  -l n, -t n accepted, ignored\n");
  return 1;
}

int main(int argc, char **argv) {
  const char *gkp_name = nullptr, *ovl_name = nullptr, *out_name = nullptr;
  uint32_t bgn = 0, end = UINT32_MAX;
  int threads = 4;
  fe_params P;
  fe_params_init(&P);
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
    else if (!strcmp(a, "-R")) { bgn = (uint32_t)atoi(value()); end = (uint32_t)atoi(value()); }
    else if (!strcmp(a, "-e")) P.error_rate = atof(value());
    else if (!strcmp(a, "-l")) value();
    else if (!strcmp(a, "-t")) threads = atoi(value());
    else if (!strcmp(a, "-d")) P.degree_threshold = (int32_t)strtol(value(), nullptr, 10);
    else if (!strcmp(a, "-k")) P.kmer_len = (int32_t)strtol(value(), nullptr, 10);
    else if (!strcmp(a, "-p")) P.use_haplo_ct = 0;
    else if (!strcmp(a, "-V")) P.vote_qualify_len = (int32_t)strtol(value(), nullptr, 10);
    else if (!strcmp(a, "-x")) P.end_exclude_len = (int32_t)strtol(value(), nullptr, 10);
    else { fprintf(stderr, "Unknown option '%s'\n", a); err++; }
  }
  if (!gkp_name) { fprintf(stderr, "ERROR: no gatekeeper store (-G) supplied.\n"); err++; }
  if (!ovl_name) { fprintf(stderr, "ERROR: no overlap store (-O) supplied.\n"); err++; }
  if (!out_name) { fprintf(stderr, "ERROR: no output file (-o) supplied.\n"); err++; }
  if (threads == 0) { fprintf(stderr, "ERROR: number of compute threads (-t) must be larger than zero.\n"); err++; }
  if (err) return usage(argv[0]);

  std::string msg;
  gkp::Store gkp;
  if (!gkp.open(gkp_name, msg)) {
    fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
    return 1;
  }
  if (bgn < 1) bgn = 1;                                         // findErrors.C:483-487
  if (gkp.num_reads() < end) end = gkp.num_reads();
  if (bgn > end) {
    fprintf(stderr, "%s: no reads in the range %u-%u (the store has %u)\n", argv[0], bgn, end,
            gkp.num_reads());
    return 1;
  }
  ovs::Store store;
  std::vector<ovl_record> recs;
  if (!store.open(ovl_name, msg) || !store.read_range(bgn, end, recs, msg)) {
    fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
    return 1;
  }
  const bool verbose = getenv("CANU_FE_VERBOSE") != nullptr;
  if (verbose) fprintf(stderr, "Read_Olaps()-- loaded %zu overlaps.\n", recs.size());

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
  if (const char *d = getenv("CANU_FE_DEVICE")) device = atoi(d);
  fe_ctx *ctx = nullptr;
  uint64_t ncor = 0;
  if (fe_ctx_create(&P, device, &ctx) != FE_OK ||
      fe_load_reads(ctx, lo, n, (const uint8_t *)bases.data(), offs.data(), lens.data()) != FE_OK ||
      fe_find_errors(ctx, bgn, end, recs.data(), recs.size(), &ncor) != FE_OK ||
      fe_write_red(ctx, out_name) != FE_OK) {
    fprintf(stderr, "%s: %s\n", argv[0], fe_last_error());
    fe_ctx_destroy(ctx);
    return 1;
  }
  fe_stats S;
  fe_get_stats(ctx, &S);
  fe_ctx_destroy(ctx);

  const unsigned long np = S.n_passed, nf = S.n_failed;            // findErrors.C:503-505
  fprintf(stderr, "\n");
  fprintf(stderr, "Passed overlaps = %10lu %8.4f%%\n", np, 100.0 * np / (nf + np));
  fprintf(stderr, "Failed overlaps = %10lu %8.4f%%\n", nf, 100.0 * nf / (nf + np));
  if (verbose)
    fprintf(stderr, " -- %.3f ms in k_fe_align, %.3f ms in k_fe_decide, %lu rows, %lu re-run(s)\n",
          S.ms_align, S.ms_decide, (unsigned long)S.rows, (unsigned long)S.regrows);
  fprintf(stderr, "\nBye.\n");
  return 0;
}
