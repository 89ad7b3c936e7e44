// sr_main.cpp -- canu_amd/bin/splitReads: the command line canu's trimming stage runs after
// trimReads (OverlapBasedTrimming.pm:128-196), over libcanu_sr.so.
//
//   splitReads -G asm.gkpStore -O asm.ovlStore -Ci asm.1.trimReads.clear
//              -Co asm.2.splitReads.clear -e erate -minlength l -o asm.2.splitReads [-t bgn-end]
//
// Options as splitReads.C:120-152.  CANU_SR_DEVICE picks the GPU.  Each library's switches come
// from the gkpStore's `libraries` file.  The outputs are the clear range file, <o>.log (empty, as
// the reference's), <o>.stats, and on stderr the reference's "Processing from ID" line and
// detectSubReads' ERROR lines (CANU_SR_VERBOSE adds the kernel times).  Two deliberate
// differences: no -Co is a usage error (the reference dereferences NULL), and no -Ci starts every
// read at 0 .. length (the reference crashes in strcpy(NULL)).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/canu_sr.h"
#include "gkp_store.h"
#include "ovs_reader.h"
#include "sr_files.h"

static int usage(const char *argv0, const std::string &why) {
  fprintf(stderr, "%s: %s\n", argv0, why.c_str());
  fprintf(stderr, "usage: %s -G gkpStore -O ovlStore -Ci input.clearFile -Co output.clearFile -o outputPrefix\n", argv0);
  fprintf(stderr, "  -t bgn-end     limit processing to only reads from bgn to end (inclusive)\n");
  fprintf(stderr, "  -e erate       printed in the statistics (0.015); no overlap is filtered by it\n");
  fprintf(stderr, "  -minlength l   reads trimmed below this many bases are deleted (64)\n");
  return 1;
}

int main(int argc, char **argv) {
  srf::Job J;
  std::string msg;
  if (!srf::parse_args(argc, argv, J, msg)) {
    if (msg.compare(0, 14, "unknown option") == 0) {      // one line, as splitReads.C:148
      fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
      return 1;
    }
    return usage(argv[0], msg);
  }

  gkp::Store gkp;
  if (!gkp.open(J.gkp, msg)) {
    fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
    return 1;
  }
  const uint32_t n = gkp.num_reads();
  std::vector<uint8_t> raw, lib_of;
  if (!srf::read_file(std::string(J.gkp) + "/libraries", raw) ||
      !srf::parse_libraries(raw, gkp.num_libraries(), lib_of, msg)) {
    fprintf(stderr, "%s: '%s/libraries': %s\n", argv[0], J.gkp, msg.empty() ? "can't open" : msg.c_str());
    return 1;
  }
  std::vector<uint32_t> lens(n);
  std::vector<uint8_t> lib_flags(n);
  for (uint32_t id = 1; id <= n; id++) {
    lens[id - 1] = gkp.length(id);
    const uint32_t lib = gkp.library(id);
    lib_flags[id - 1] = lib <= gkp.num_libraries() ? lib_of[lib] : 0;
  }

  // an existing -Co file is loaded, reset and overwritten from -Ci (splitReads.C:185-195): only
  // that it is one for this store matters
  std::vector<uint32_t> ob, oe, cb, ce;
  if (srf::read_file(J.clear, raw) && !srf::parse_clear(raw, n, ob, oe, msg)) {
    fprintf(stderr, "%s: '%s': %s\n", argv[0], J.clear, msg.c_str());
    return 1;
  }
  uint32_t bgn0 = 0, end0 = 0;
  if (J.clear_in) {
    if (!srf::read_file(J.clear_in, raw)) {
      fprintf(stderr, "%s: can't open '%s'\n", argv[0], J.clear_in);
      return 1;
    }
    if (!srf::parse_clear(raw, n, cb, ce, msg)) {
      fprintf(stderr, "%s: '%s': %s\n", argv[0], J.clear_in, msg.c_str());
      return 1;
    }
    bgn0 = cb[0];
    end0 = ce[0];
  }

  uint32_t id_min = J.id_min < 1 ? 1 : J.id_min, id_max = J.id_max > n ? n : J.id_max;
  fprintf(stderr, "Processing from ID %u to %u out of %u reads, using errorRate = %.2f\n", id_min, id_max, n,
          J.P.erate);

  ovs::Store store;
  std::vector<ovl_record> recs;
  if (!store.open(J.ovl, msg) || (id_min <= id_max && !store.read_range(id_min, id_max, recs, msg))) {
    fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
    return 1;
  }

  std::vector<uint32_t> bgn(n), end(n), nadj(n), nreg(n);
  std::vector<uint8_t> status(n), fate(recs.size());
  std::vector<sr_region> regions(recs.size() / 2 + 1);
  std::vector<uint64_t> region_off((size_t)n + 1);
  sr_result R{bgn.data(), end.data(), status.data(), nadj.data(), nreg.data(), fate.data(),
              regions.data(), regions.size(), region_off.data()};
  int device = 0;
  if (const char *d = getenv("CANU_SR_DEVICE")) device = atoi(d);
  sr_ctx *ctx = nullptr;
  sr_stats S;
  const uint32_t *in_b = J.clear_in ? cb.data() + 1 : nullptr, *in_e = J.clear_in ? ce.data() + 1 : nullptr;
  if (sr_ctx_create(&J.P, device, &ctx) != SR_OK ||
      sr_split_reads(ctx, n, lens.data(), lib_flags.data(), in_b, in_e, recs.data(), recs.size(), 0, id_min,
                     id_max, &R) != SR_OK ||
      sr_get_stats(ctx, &S) != SR_OK) {
    fprintf(stderr, "%s: %s\n", argv[0], sr_last_error());
    sr_ctx_destroy(ctx);
    return 1;
  }
  sr_ctx_destroy(ctx);
  const std::string errs = srf::error_lines(recs.data(), recs.size(), fate.data());
  fwrite(errs.data(), 1, errs.size(), stderr);
  if (getenv("CANU_SR_VERBOSE"))
    fprintf(stderr, " -- %llu overlaps; %llu reads by a wave (%.3f ms), %llu large (%.3f ms), %.3f ms in the record pass; %llu bad regions\n",
            (unsigned long long)S.n_overlaps, (unsigned long long)S.n_wave_reads, S.ms_wave,
            (unsigned long long)S.n_large_reads, S.ms_large, S.ms_records, (unsigned long long)S.n_regions);

  if (!J.clear_in) {                                      // 0 .. length
    cb.assign((size_t)n + 1, 0);
    ce.assign((size_t)n + 1, 0);
    for (uint32_t i = 0; i < n; i++) ce[i + 1] = lens[i];
  }
  const std::vector<uint8_t> clr = srf::clear_bytes(n, cb.data() + 1, ce.data() + 1, R, bgn0, end0);
  const std::string sta = srf::stats_text(J.P, S);
  const std::string pre = J.out;
  if (!srf::write_file(J.clear, clr.data(), clr.size()) || !srf::write_file(pre + ".log", "", 0) ||
      !srf::write_file(pre + ".stats", sta.data(), sta.size())) {
    fprintf(stderr, "%s: can't write the outputs of '%s'\n", argv[0], J.out);
    return 1;
  }
  return 0;
}
