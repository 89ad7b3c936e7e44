// tr_main.cpp -- canu_amd/bin/trimReads: the command line canu's trimming stage runs
// (OverlapBasedTrimming.pm:57-120), over libcanu_tr.so.
//
//   trimReads -G asm.gkpStore -O asm.ovlStore -Co asm.1.trimReads.clear -e erate
//             -minlength l -ol l -oc c -o asm.1.trimReads [-t bgn-end]
//
// Options as trimReads.C:145-189.  -Ci, -Cm and -l are refused (tr_files.h).  CANU_TR_DEVICE picks
// the GPU.  Each library's finalTrim comes from the gkpStore's `libraries` file.  The outputs are
// the clear range file, <o>.log, <o>.stats and the reference's "Processing from ID" line on
// stderr (CANU_TR_VERBOSE adds the kernel times).  The reference's nine .dat / .gp plot files and
// its gnuplot runs are not produced: canu reads the .clear and the .stats only.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/canu_tr.h"
#include "gkp_store.h"
#include "ovs_reader.h"
#include "tr_files.h"

static int usage(const char *argv0, const std::string &why) {
  fprintf(stderr, "%s: %s\n", argv0, why.c_str());
  fprintf(stderr, "usage: %s -G gkpStore -O ovlStore -Co output.clearFile -o outputPrefix\n", argv0);
  fprintf(stderr, "  -t bgn-end     limit processing to only reads from bgn to end (inclusive)\n");
  fprintf(stderr, "  -e erate       ignore overlaps with more than 'erate' percent error (0.015)\n");
  fprintf(stderr, "  -ol l          the minimum evidence overlap length (40)\n");
  fprintf(stderr, "  -oc c          the minimum evidence overlap coverage (1)\n");
  fprintf(stderr, "  -minlength l   reads trimmed below this many bases are deleted (64)\n");
  return 1;
}

int main(int argc, char **argv) {
  trf::Job J;
  std::string msg;
  if (!trf::parse_args(argc, argv, J, msg)) return usage(argv[0], msg);

  gkp::Store gkp;
  if (!gkp.open(J.gkp, msg)) {
    fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
    return 1;
  }
  const uint32_t n = gkp.num_reads();
  std::vector<uint8_t> raw;
  std::vector<uint32_t> final_trim;
  if (!trf::read_file(std::string(J.gkp) + "/libraries", raw) ||
      !trf::parse_libraries(raw, gkp.num_libraries(), final_trim, msg)) {
    fprintf(stderr, "%s: '%s/libraries': %s\n", argv[0], J.gkp, msg.empty() ? "can't open" : msg.c_str());
    return 1;
  }
  std::vector<uint32_t> lens(n);
  std::vector<uint8_t> rules(n);
  for (uint32_t id = 1; id <= n; id++) {
    lens[id - 1] = gkp.length(id);
    const uint32_t lib = gkp.library(id);
    rules[id - 1] = lib <= gkp.num_libraries() && final_trim[lib] < 256 ? (uint8_t)final_trim[lib] : 0;
  }

  // an existing clear range file is loaded and reset (trimReads.C:225-230): entry 0 stays
  uint32_t bgn0 = 0, end0 = 0;
  if (trf::read_file(J.clear, raw)) {
    std::vector<uint32_t> ob, oe;
    if (!trf::parse_clear(raw, n, ob, oe, msg)) {
      fprintf(stderr, "%s: '%s': %s\n", argv[0], J.clear, msg.c_str());
      return 1;
    }
    bgn0 = ob[0];
    end0 = oe[0];
  }

  uint32_t id_min = J.id_min < 1 ? 1 : J.id_min, id_max = J.id_max > n ? n : J.id_max;
  fprintf(stderr, "Processing from ID %u to %u out of %u reads.\n", id_min, id_max, n);

  ovs::Store store;
  std::vector<ovl_record> recs;
  if (!store.open(J.ovl, msg) || (id_min <= id_max && !store.read_range(id_min, id_max, recs, msg))) {
    fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
    return 1;
  }

  std::vector<uint32_t> bgn(n), end(n), nskip(n), nused(n);
  std::vector<uint8_t> status(n), flags(n);
  tr_result R{bgn.data(), end.data(), status.data(), flags.data(), nskip.data(), nused.data()};
  int device = 0;
  if (const char *d = getenv("CANU_TR_DEVICE")) device = atoi(d);
  tr_ctx *ctx = nullptr;
  tr_stats S;
  if (tr_ctx_create(&J.P, device, &ctx) != TR_OK ||
      tr_trim_reads(ctx, n, lens.data(), rules.data(), recs.data(), recs.size(), 0, id_min, id_max, &R) != TR_OK ||
      tr_get_stats(ctx, &S) != TR_OK) {
    fprintf(stderr, "%s: %s\n", argv[0], tr_last_error());
    tr_ctx_destroy(ctx);
    return 1;
  }
  tr_ctx_destroy(ctx);
  for (uint32_t i = 0; i < n; i++)
    if (flags[i] & TR_FLAG_RESET) fprintf(stderr, "iid = %u\n", i + 1);      // bestEdge.C:396
  if (getenv("CANU_TR_VERBOSE"))
    fprintf(stderr, " -- %llu overlaps; %llu reads by a wave (%.3f ms), %llu large (%.3f ms), %.3f ms in the record pass\n",
            (unsigned long long)S.n_overlaps, (unsigned long long)S.n_wave_reads, S.ms_wave,
            (unsigned long long)S.n_large_reads, S.ms_large, S.ms_segment);

  const std::vector<uint8_t> clr = trf::clear_bytes(n, lens.data(), R, bgn0, end0);
  const std::string log = trf::log_text(id_min, id_max, lens.data(), R), sta = trf::stats_text(J.P, S);
  const std::string pre = J.out;
  if (!trf::write_file(J.clear, clr.data(), clr.size()) ||
      !trf::write_file(pre + ".log", log.data(), log.size()) ||
      !trf::write_file(pre + ".stats", sta.data(), sta.size())) {
    fprintf(stderr, "%s: can't write the outputs of '%s'\n", argv[0], J.out);
    return 1;
  }
  return 0;
}
