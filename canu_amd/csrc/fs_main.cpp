// fs_main.cpp -- canu_amd/bin/falconsense: the command line canu's correctReads.sh runs
// (CorrectReads.pm:503-512), over libcanu_fs.so.
//
//   falconsense -G asm.gkpStore -C asm.corStore -b bgn -e end [-r readlist] [-t T] [-p prefix]
//               -cc minCoverage -cl minLength -ci minIdentity  > corrected.fasta
//
// Options as falconsense.C:229-270, its three habits included: -ci goes through atoi (canu's
// 0.x is 0); the tigs processed are bgn <= id < end with end clamped to the number of reads, so
// read `end` itself is left out; -r keeps the listed IDs of [bgn, end].  -t and -p are accepted
// and change nothing.  CANU_FS_DEVICE picks the GPU.  Only the reads the selected tigs name are
// loaded.  The corrected reads go to stdout, the "Processing read" and "Generated read" lines
// to stderr (CANU_FS_VERBOSE adds the kernel times).
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../include/canu_fs.h"
#include "fs_fasta.h"
#include "gkp_store.h"
#include "tgs_reader.h"

static int usage(const char *argv0) {
  fprintf(stderr, "usage: %s -G gkpStore -C corStore [-b bgnID] [-e endID] [-r readlist] [options]\n", argv0);
  fprintf(stderr, "  -cc coverage   minimum consensus coverage to output corrected base (4)\n");
  fprintf(stderr, "  -cl length     minimum length of corrected region (500)\n");
  fprintf(stderr, "  -ci identity   minimum identity of an aligned evidence read (an integer)\n");
  fprintf(stderr, "  -t n, -p name  accepted, ignored\n");
  return 1;
}

int main(int argc, char **argv) {
  const char *gkp_name = nullptr, *cor_name = nullptr, *list_name = nullptr;
  uint32_t id_min = 0, id_max = UINT32_MAX;
  fs_params P;
  fs_params_init(&P);
  int err = 0;
  for (int arg = 1; arg < argc; arg++) {
    const char *a = argv[arg];
    auto value = [&]() -> const char * {
      if (arg + 1 >= argc) { err++; return "0"; }
      return argv[++arg];
    };
    if (!strcmp(a, "-G")) gkp_name = value();
    else if (!strcmp(a, "-C")) cor_name = value();
    else if (!strcmp(a, "-p")) value();
    else if (!strcmp(a, "-t")) value();
    else if (!strcmp(a, "-b")) id_min = (uint32_t)atoi(value());
    else if (!strcmp(a, "-e")) id_max = (uint32_t)atoi(value());
    else if (!strcmp(a, "-r")) list_name = value();
    else if (!strcmp(a, "-cc")) P.min_coverage = (uint32_t)atoi(value());
    else if (!strcmp(a, "-cl")) P.min_output_length = (uint32_t)atoi(value());
    else if (!strcmp(a, "-ci")) P.min_identity = atoi(value());        // atoi, as there
    else { fprintf(stderr, "ERROR: unknown option '%s'\n", a); err++; }
  }
  if (!gkp_name) { fprintf(stderr, "ERROR: no gkpStore input (-G) supplied.\n"); err++; }
  if (!cor_name) { fprintf(stderr, "ERROR: no corStore input (-C) supplied.\n"); err++; }
  if (err) return usage(argv[0]);

  std::string msg;
  gkp::Store gkp;
  if (!gkp.open(gkp_name, msg)) {
    fprintf(stderr, "%s: %s\n", argv[0], msg.c_str());
    return 1;
  }
  tgs::Store cor;
  if (!cor.open(cor_name, msg)) {
    fprintf(stderr, "%s: '%s': %s\n", argv[0], cor_name, msg.c_str());
    return 1;
  }
  const uint32_t num_reads = gkp.num_reads();
  if (num_reads < id_max) id_max = num_reads;                          // falconsense.C:314-315
  std::set<uint32_t> read_list;
  if (list_name) {                                                     // loadReadList, :59-83
    FILE *R = fopen(list_name, "r");
    if (!R) {
      fprintf(stderr, "Failed to open '%s' for reading: %s\n", list_name, strerror(errno));
      return 1;
    }
    char line[1024];
    while (fgets(line, sizeof line, R)) {
      const uint32_t id = (uint32_t)strtoul(line, nullptr, 10);
      if (id_min <= id && id <= id_max) read_list.insert(id);
    }
    fclose(R);
  }

  std::vector<fs_layout> layouts;
  std::vector<fs_child> children;
  std::vector<uint32_t> layout_len;
  uint32_t lo = UINT32_MAX, hi = 0;
  auto name = [&](uint32_t id) -> bool {
    if (id == 0 || id > num_reads) {
      fprintf(stderr, "%s: a layout names read %u; the store has reads 1..%u\n", argv[0], id, num_reads);
      return false;
    }
    lo = id < lo ? id : lo;
    hi = id > hi ? id : hi;
    return true;
  };
  for (uint32_t ii = id_min; ii < id_max; ii++) {
    if (!read_list.empty() && !read_list.count(ii)) continue;
    if (ii >= cor.tigs.size() || cor.tigs[ii].deleted) {
      fprintf(stderr, "%s: '%s' has no tig %u\n", argv[0], cor_name, ii);
      return 1;
    }
    const tgs::Tig &t = cor.tigs[ii];
    if (!name(ii)) return 1;
    fs_layout l{ii, (uint32_t)children.size(), t.n_children};
    for (uint32_t k = 0; k < t.n_children; k++) {
      const tgs::Child &c = cor.children[t.first_child + k];
      if (!name(c.ident)) return 1;
      children.push_back(fs_child{c.ident, c.reverse, c.min, c.max, c.askip, c.bskip});
    }
    layouts.push_back(l);
    layout_len.push_back(t.layout_len);
  }
  if (layouts.empty()) return 0;

  // the reads the tigs name, as one ID range whose other reads are empty
  const uint32_t n = hi - lo + 1;
  std::vector<uint8_t> named(n, 0);
  for (const fs_layout &l : layouts) named[l.tig_id - lo] = 1;
  for (const fs_child &c : children) named[c.ident - lo] = 1;
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
  if (const char *d = getenv("CANU_FS_DEVICE")) device = atoi(d);
  fs_ctx *ctx = nullptr;
  uint64_t nl = 0, nb = 0;
  if (fs_ctx_create(&P, device, &ctx) != FS_OK ||
      fs_load_reads(ctx, lo, n, (const uint8_t *)bases.data(), offs.data(), lens.data()) != FS_OK ||
      fs_consensus(ctx, layouts.data(), layouts.size(), children.data(), children.size()) != FS_OK ||
      fs_result_size(ctx, &nl, &nb) != FS_OK) {
    fprintf(stderr, "%s: %s\n", argv[0], fs_last_error());
    fs_ctx_destroy(ctx);
    return 1;
  }
  std::vector<uint8_t> cns(nb ? nb : 1);
  std::vector<uint64_t> off(nl + 1);
  fs_fetch(ctx, cns.data(), off.data(), nullptr);
  fs_stats S;
  fs_get_stats(ctx, &S);
  fs_ctx_destroy(ctx);

  std::string out, log;
  for (size_t i = 0; i < layouts.size(); i++) {
    out.clear();
    log.clear();
    fprintf(stderr, "Processing read %u of length %u with %u evidence reads.\n", layouts[i].tig_id,
            layout_len[i], layouts[i].n_children);
    fs_fasta_pieces(out, &log, layouts[i].tig_id, cns.data() + off[i], off[i + 1] - off[i],
                    P.min_output_length);
    fputs(log.c_str(), stderr);
    if (!out.empty() && fwrite(out.data(), 1, out.size(), stdout) != out.size()) {
      fprintf(stderr, "%s: short write to stdout\n", argv[0]);
      return 1;
    }
  }
  if (getenv("CANU_FS_VERBOSE"))
    fprintf(stderr, " -- %.3f ms locate, %.3f ms path, %.3f ms sort, %.3f ms consensus, %llu cells\n",
            S.ms_locate, S.ms_path, S.ms_sort, S.ms_consensus, (unsigned long long)S.dp_cells);
  return fflush(stdout) == 0 ? 0 : 1;
}
