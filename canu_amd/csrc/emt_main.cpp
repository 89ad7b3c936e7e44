// canu_amd/bin/estimate-mer-threshold -h FILE [-c COV]: the threshold behind canu's default
// `auto` (the reference's src/meryl/estimate-mer-threshold.C, histogram-file input only).
// One integer on stdout, the reference's progress text on stderr.  Host only.
//
// The arithmetic is the reference's: histogram entries and counts are 32-bit, and every
// product of the two wraps in 32 bits before it is added to a 64-bit sum.  canu_amd/meryl.py
// (estimate_threshold) is the same computation in Python; the tests hold both to the golden
// outputs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct Hist {
  std::vector<uint32_t> v;     // far longer than len, zero beyond it, as the reference's array
  uint32_t len = 0;            // largest count in the file + 1
  uint32_t at(uint64_t i) const { return i < v.size() ? v[i] : 0; }
};

bool load(const char *path, Hist &H) {
  FILE *f = fopen(path, "r");
  if (!f) return false;
  H.v.assign(1u << 20, 0);
  char line[1024];
  uint32_t top = 0;
  while (fgets(line, sizeof line, f)) {
    char *e = line;
    uint32_t h = (uint32_t)strtoull(e, &e, 10);
    uint32_t c = (uint32_t)strtoull(e, &e, 10);
    if (h >= H.v.size()) H.v.resize((size_t)h + 1 + (1u << 20), 0);
    H.v[h] = c;
    if (h > top) top = h;
  }
  fclose(f);
  H.len = top + 1;
  return true;
}

uint32_t guess_coverage(const Hist &H) {
  uint32_t i = 2;
  while (i < H.len && H.at(i - 1) > H.at(i)) i++;
  uint32_t best = i - 1;
  for (; i < H.len; i++)
    if (H.at(best) < H.at(i)) best = i;
  fprintf(stderr, "Guessed X coverage is %u\n", best);
  return best;
}

void report(uint32_t max_count, const Hist &H, uint64_t distinct, uint64_t total,
            uint64_t useful_distinct, uint64_t useful_all) {
  fprintf(stderr,
          "Set maxCount to %u (%u kmers), which will cover %.2f%% of distinct mers and %.2f%% "
          "of all mers.\n",
          max_count, H.at(max_count), 100.0 * distinct / useful_distinct,
          100.0 * total / useful_all);
}

}  // namespace

int main(int argc, char **argv) {
  const char *hist_path = nullptr;
  double coverage = 0;
  int err = 0;
  for (int a = 1; a < argc; a++) {
    if (!strcmp(argv[a], "-h") && a + 1 < argc) hist_path = argv[++a];
    else if (!strcmp(argv[a], "-c") && a + 1 < argc) coverage = atof(argv[++a]);
    else if (!strcmp(argv[a], "-m")) {
      fprintf(stderr, "%s: -m (a meryl database) is not supported; use -h histogram\n", argv[0]);
      return 1;
    } else {
      fprintf(stderr, "unknown option '%s'\n", argv[a]);
      err++;
    }
  }
  if (!hist_path || err) {
    fprintf(stderr, "usage: %s [-c coverage] -h histogram\n", argv[0]);
    fprintf(stderr, "  -h histogram    histogram from meryl -Dh\n");
    fprintf(stderr, "  -c coverage     expected coverage of reads\n");
    return 1;
  }
  Hist H;
  if (!load(hist_path, H)) {
    fprintf(stderr, "%s: cannot read '%s'\n", argv[0], hist_path);
    return 1;
  }
  const uint32_t n = H.len;
  uint64_t n_distinct = 0, n_total = 0;
  const uint64_t n_unique = H.at(1);
  for (uint32_t h = 0; h < n; h++) {
    n_distinct += H.at(h);
    n_total += (uint32_t)(H.at(h) * h);
  }
  fprintf(stderr, "RAW MER COUNTS:\n");
  fprintf(stderr, "  distinct: %12llu (different kmer sequences)\n", (unsigned long long)n_distinct);
  fprintf(stderr, "  unique:   %12llu (single-copy kmers)\n", (unsigned long long)n_unique);
  fprintf(stderr, "  total:    %12llu (kmers in sequences)\n", (unsigned long long)n_total);
  fprintf(stderr, "\n");
  const double guessed = coverage > 0 ? coverage : (double)guess_coverage(H);

  const uint64_t useful_distinct = n_distinct - n_unique, useful_all = n_total - n_unique;
  uint64_t distinct = 0, total = 0;
  uint32_t max_count = 0, ext_count = 0, kk = 2;
  // first limit: nearly all distinct mers, or two thirds of all mers at a high count
  for (; kk < n; kk++) {
    distinct += H.at(kk);
    total += (uint32_t)(H.at(kk) * kk);
    if (distinct / (double)useful_distinct > 0.9975 ||
        (total / (double)useful_all > 0.6667 && kk > 50 * guessed)) {
      max_count = kk;
      break;
    }
  }
  report(max_count, H, distinct, total, useful_distinct, useful_all);

  // mean mers per count in a window around it, then slide the window to the first gap
  uint32_t lo = max_count < 27 ? 2 : max_count - 25;
  uint32_t hi = max_count + 26 > n ? n : max_count + 26;
  uint64_t avg = 0, tot = 0;
  for (uint32_t i = lo; i < hi; i++) {
    uint32_t p = i * H.at(i);
    avg += p;
    tot += p;
  }
  const uint32_t span = hi - lo;
  if (span == 0) {
    fprintf(stderr, "%s: histogram too short to estimate a threshold\n", argv[0]);
    return 1;
  }
  avg /= span;
  fprintf(stderr, "Average number of kmers between count %u and %u is %llu\n", lo, hi,
          (unsigned long long)avg);
  while (hi < n && tot != 0) {
    tot -= (uint32_t)(lo * H.at(lo));
    tot += (uint32_t)(hi * H.at(hi));
    lo++;
    hi++;
  }
  uint32_t limit;
  if (tot > 0) {
    limit = n;
    fprintf(stderr, "No break in kmer coverage found.\n");
  } else {
    limit = lo;
    fprintf(stderr, "Found break in kmer coverage at %d\n", (int)limit);
  }
  // extend to a tenfold jump, or to 90 % of the sequence at sufficient coverage
  for (; kk < limit; kk++) {
    if (avg * 10 < (uint32_t)(kk * H.at(kk))) break;
    if ((double)total / useful_all >= 0.9 && kk > 50 * guessed) break;
    distinct += H.at(kk);
    total += (uint32_t)(H.at(kk) * kk);
    if (H.at(kk) > 0) ext_count = kk;
  }
  if (ext_count > 0) max_count = ext_count;
  report(max_count, H, distinct, total, useful_distinct, useful_all);
  printf("%u\n", max_count);
  return 0;
}
