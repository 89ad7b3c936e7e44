// canu_amd/bin/meryl -- the three meryl command lines of canu's 0-mercounts stage
// (src/pipelines/canu/Meryl.pm:434-455, :634, :698), over libcanu_meryl.so:
//
//   meryl -B -C -L 2 -v -m K -threads T -memory M -s <gkpStore | reads.fasta> -o PREFIX
//   meryl -Dh -s PREFIX            histogram rows on stdout, the four info lines on stderr
//   meryl -Dt -n THRESH -s PREFIX  ">count\nMER\n" on stdout
//
// The two dump modes are host only (meryl_host.h); the count needs a gfx950 device
// (CANU_MERYL_DEVICE picks it).  Every other meryl mode is refused.
#include <sys/stat.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "canu_meryl.h"
#include "gkp_store.h"
#include "meryl_host.h"

namespace {

void usage(const char *me) {
  fprintf(stderr,
          "usage: %s -B [-C] [-L low] -m merSize -s <gkpStore|fasta> -o prefix\n"
          "          [-v] [-threads T] [-memory MB]\n"
          "       %s -Dh -s prefix\n"
          "       %s -Dt -n threshold -s prefix\n"
          "  -B           count the mers of every read (1..N, full sequence) on the GPU\n"
          "  -C           canonical mers\n"
          "  -L low       keep mers with at least this count in the database (default 2)\n"
          "  -memory MB   may only LOWER the HBM the per-pass buffers take (the count then runs\n"
          "               more passes); it never raises it above what the device has free\n"
          "  -threads, -v accepted, no effect\n"
          "  -Dh, -Dt     host only.  prefix.mcdat / prefix.mcidx are this program's own\n"
          "               format, not interchangeable with the reference meryl's.\n"
          "  CANU_MERYL_DEVICE=<n> picks the GPU (default 0).\n",
          me, me, me);
}

int refuse(const char *me, const std::string &what) {
  fprintf(stderr, "%s: %s\n", me, what.c_str());
  return 1;
}

bool is_dir(const std::string &p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

struct Reads {
  std::string bases;
  std::vector<uint64_t> offsets;
  std::vector<uint32_t> lengths;
  void add(const std::string &s) {
    offsets.push_back(bases.size());
    lengths.push_back((uint32_t)s.size());
    bases += s;
  }
};

bool load_store(const std::string &path, Reads &R, std::string &err) {
  gkp::Store st;
  if (!st.open(path, err)) return false;
  std::string seq, qlt;
  for (uint32_t id = 1; id <= st.num_reads(); id++) {   // every read, full sequence
    if (!st.load(id, seq, qlt, err)) return false;
    R.add(seq);
  }
  return true;
}

bool load_fasta(const std::string &path, Reads &R, std::string &err) {
  FILE *f = fopen(path.c_str(), "r");
  if (!f) { err = "can't open '" + path + "'"; return false; }
  std::string cur, line;
  bool have = false;
  char buf[1 << 16];
  auto take = [&]() {
    if (line.empty()) return;
    if (line[0] == '>') {
      if (have) R.add(cur);
      cur.clear();
      have = true;
    } else if (have) {
      for (char c : line)
        if (c > ' ') cur += c;
    }
    line.clear();
  };
  while (fgets(buf, sizeof buf, f)) {
    size_t n = strlen(buf);
    bool eol = n && buf[n - 1] == '\n';
    line.append(buf, eol ? n - 1 : n);
    if (eol) take();
  }
  take();
  if (have) R.add(cur);
  fclose(f);
  return true;
}

}  // namespace

int main(int argc, char **argv) {
  const char *me = argv[0];
  bool build = false, canonical = false, dump_h = false, dump_t = false;
  uint32_t k = 0, low = 2;
  uint64_t thresh = 0, memory_mb = 0;
  bool have_n = false;
  std::string src, out;
  for (int a = 1; a < argc; a++) {
    std::string o = argv[a];
    auto val = [&]() -> const char * {
      if (a + 1 >= argc) { fprintf(stderr, "%s: %s needs a value\n", me, o.c_str()); exit(1); }
      return argv[++a];
    };
    if (o == "-B") build = true;
    else if (o == "-C") canonical = true;
    else if (o == "-v") {}
    else if (o == "-L") low = (uint32_t)strtoul(val(), nullptr, 10);
    else if (o == "-m") k = (uint32_t)strtoul(val(), nullptr, 10);
    else if (o == "-threads") (void)val();
    else if (o == "-memory") memory_mb = strtoull(val(), nullptr, 10);
    else if (o == "-s") src = val();
    else if (o == "-o") out = val();
    else if (o == "-Dh") dump_h = true;
    else if (o == "-Dt") dump_t = true;
    else if (o == "-n") { thresh = strtoull(val(), nullptr, 10); have_n = true; }
    else if (o == "-h" || o == "--help") { usage(me); return 0; }
    else {
      usage(me);
      return refuse(me, "'" + o + "' is not supported: this meryl does only the count (-B) and "
                        "the two dumps (-Dh, -Dt) canu's 0-mercounts stage runs");
    }
  }
  if ((int)build + (int)dump_h + (int)dump_t != 1) {
    usage(me);
    return refuse(me, "exactly one of -B, -Dh, -Dt");
  }
  if (src.empty()) return refuse(me, "no input (-s)");

  if (dump_h || dump_t) {
    if (dump_t && !have_n) return refuse(me, "-Dt needs -n threshold");
    merhost::MerDb db;
    std::string err;
    if (!merhost::open(src, db, err)) return refuse(me, err);
    // the reference's build keeps every mer whatever its -L; this database does not
    if (dump_t && thresh < db.low_count)
      fprintf(stderr,
              "%s: warning: -n %llu is below the -L %u this database was counted with: mers with "
              "a count below %u are not in it (count with -L 1 to dump them)\n",
              me, (unsigned long long)thresh, db.low_count, db.low_count);
    if (dump_h) merhost::write_histogram(db, stdout, stderr);
    else merhost::write_threshold(db, thresh, stdout);
    return fflush(stdout) == 0 ? 0 : 1;
  }

  if (k < 1 || k > 32) return refuse(me, "-m merSize must be 1..32");
  if (out.empty()) return refuse(me, "no output prefix (-o)");
  if (low < 1) low = 1;
  Reads R;
  std::string err;
  if (!(is_dir(src) ? load_store(src, R, err) : load_fasta(src, R, err))) return refuse(me, err);

  mer_params P;
  mer_params_init(&P);
  P.kmer_len = k;
  P.canonical = canonical ? 1 : 0;
  P.low_count = low;
  if (memory_mb) {
    P.hbm_budget_bytes = memory_mb << 20;
    if (P.hbm_budget_bytes < MER_MIN_BUDGET_BYTES) P.hbm_budget_bytes = MER_MIN_BUDGET_BYTES;
  }
  const char *dev = getenv("CANU_MERYL_DEVICE");
  mer_ctx *ctx = nullptr;
  int rc = mer_ctx_create(&P, dev ? atoi(dev) : 0, &ctx);
  if (!rc) rc = mer_load_reads(ctx, (uint32_t)R.lengths.size(), (const uint8_t *)R.bases.data(),
                               R.offsets.data(), R.lengths.data());
  if (!rc) rc = mer_count(ctx);
  if (!rc) rc = mer_save(ctx, out.c_str());
  if (rc) {
    fprintf(stderr, "%s: %s\n", me, mer_last_error());
    mer_ctx_destroy(ctx);
    return 1;
  }
  mer_stats S;
  mer_get_stats(ctx, &S);
  fprintf(stderr, "Found %llu mers, %llu distinct, %llu unique; %llu kept at -L %u.\n",
          (unsigned long long)S.total_mers, (unsigned long long)S.distinct_mers,
          (unsigned long long)S.unique_mers, (unsigned long long)S.kept_mers, low);
  fprintf(stderr, "%llu passes, %.1f ms on the device (plan %.1f, partition %.1f, sort %.1f).\n",
          (unsigned long long)S.passes, S.ms_total, S.ms_plan, S.ms_partition, S.ms_sort);
  mer_ctx_destroy(ctx);
  return 0;
}
