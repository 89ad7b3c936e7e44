// tr_host_check.cpp -- the host code of canu_amd/bin/trimReads (canu_amd/csrc/tr_files.h) run by
// itself, so that it can be built with -fsanitize=address,undefined: the argument parser, the
// clear range file reader and writer, the log and stats formatters and the libraries reader.
//
//   tr_host_check <dir>
//
// <dir> holds what tests/test_tr_cpu.py wrote from one fixture: args.txt (the fixture's options,
// one per line), lengths.bin, bgn.bin, end.bin, n_skipped.bin, n_used.bin (uint32 per read),
// status.bin, flags.bin (uint8 per read), counters.bin (nine pairs of uint64), range.bin (id_min,
// id_max), the reference's want.clear, want.log, want.stats, and optionally libraries with
// final_trim.bin (uint32 per library, from library 0).  Exit status 0: everything equal and every
// damaged input refused.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../canu_amd/csrc/tr_files.h"

static int failures = 0;

static void expect(bool ok, const char *what) {
  if (!ok) {
    fprintf(stderr, "FAIL: %s\n", what);
    failures++;
  }
}

template <class T>
static std::vector<T> load(const std::string &path) {
  std::vector<uint8_t> raw;
  if (!trf::read_file(path, raw)) {
    fprintf(stderr, "FAIL: can't read %s\n", path.c_str());
    failures++;
  }
  std::vector<T> v(raw.size() / sizeof(T));
  if (!v.empty()) memcpy(v.data(), raw.data(), v.size() * sizeof(T));
  return v;
}

static bool parses(std::vector<std::string> words, trf::Job &J, std::string &err) {
  std::vector<const char *> argv{"trimReads"};
  for (const std::string &w : words) argv.push_back(w.c_str());
  J = trf::Job();
  return trf::parse_args((int)argv.size(), argv.data(), J, err);
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <dir>\n", argv[0]);
    return 2;
  }
  const std::string d = std::string(argv[1]) + "/";

  // ---- the argument parser
  std::vector<uint8_t> raw = load<uint8_t>(d + "args.txt");
  std::vector<std::string> opts;
  std::string cur;
  for (uint8_t c : raw) {
    if (c == '\n') { if (!cur.empty()) opts.push_back(cur); cur.clear(); }
    else cur += (char)c;
  }
  if (!cur.empty()) opts.push_back(cur);
  std::vector<std::string> full{"-G", "g", "-O", "o", "-Co", "c", "-o", "p"};
  full.insert(full.end(), opts.begin(), opts.end());
  trf::Job J, X;
  std::string err;
  expect(parses(full, J, err), "canu's command line parses");
  for (const char *bad : {"-Ci", "-Cm", "-l"}) {
    std::vector<std::string> w = full;
    w.push_back(bad);
    w.push_back("x");
    expect(!parses(w, X, err) && err.find("not supported") != std::string::npos, "-Ci / -Cm / -l are refused");
  }
  {
    std::vector<std::string> w(full.begin(), full.begin() + 4);
    w.insert(w.end(), full.begin() + 6, full.end());
    expect(!parses(w, X, err) && err.find("-Co") != std::string::npos, "a missing -Co is refused");
    w = full;
    w.push_back("-t");
    expect(!parses(w, X, err), "an option without its value is refused");
    w.back() = "-bogus";
    expect(!parses(w, X, err), "an unknown option is refused");
    w = full;
    w.push_back("-t");
    w.push_back("7");
    expect(parses(w, X, err) && X.id_min == 7 && X.id_max == 7, "-t with one number");
    w.back() = "3-9";
    expect(parses(w, X, err) && X.id_min == 3 && X.id_max == 9, "-t with a range");
  }

  // ---- the three outputs
  std::vector<uint32_t> lens = load<uint32_t>(d + "lengths.bin"), bgn = load<uint32_t>(d + "bgn.bin"),
                        end = load<uint32_t>(d + "end.bin"), nskip = load<uint32_t>(d + "n_skipped.bin"),
                        nused = load<uint32_t>(d + "n_used.bin"), range = load<uint32_t>(d + "range.bin");
  std::vector<uint8_t> status = load<uint8_t>(d + "status.bin"), flags = load<uint8_t>(d + "flags.bin");
  std::vector<uint64_t> cnt = load<uint64_t>(d + "counters.bin");
  const uint32_t n = (uint32_t)lens.size();
  expect(bgn.size() == n && end.size() == n && nskip.size() == n && nused.size() == n && status.size() == n &&
             flags.size() == n && cnt.size() == 18 && range.size() == 2,
         "the inputs have one entry per read");
  if (failures) return 1;
  tr_result R{bgn.data(), end.data(), status.data(), flags.data(), nskip.data(), nused.data()};
  tr_stats S{};
  tr_count *c[9] = {&S.reads_in, &S.deleted_in, &S.no_trim_in, &S.reads_out, &S.no_ovl_out,
                    &S.deleted_out, &S.no_change_out, &S.trim5, &S.trim3};
  for (int k = 0; k < 9; k++) *c[k] = tr_count{cnt[2 * k], cnt[2 * k + 1]};
  const std::vector<uint8_t> want_clear = load<uint8_t>(d + "want.clear"), want_log = load<uint8_t>(d + "want.log"),
                             want_stats = load<uint8_t>(d + "want.stats");
  const std::vector<uint8_t> clr = trf::clear_bytes(n, lens.data(), R, 0, 0);
  expect(clr == want_clear, "the clear range file equals the reference's");
  const std::string log = trf::log_text(range[0], range[1], lens.data(), R);
  expect(log == std::string(want_log.begin(), want_log.end()), "the log equals the reference's");
  const std::string sta = trf::stats_text(J.P, S);
  expect(sta == std::string(want_stats.begin(), want_stats.end()), "the stats equal the reference's");

  // ---- the clear range file, whole and damaged
  std::vector<uint32_t> cb, ce;
  expect(trf::parse_clear(clr, n, cb, ce, err) && cb.size() == (size_t)n + 1 && ce.size() == (size_t)n + 1,
         "a whole clear range file loads");
  bool same = true;
  for (uint32_t i = 0; i < n && same; i++) {
    const bool gone = status[i] == TR_NOV || status[i] == TR_DEL;
    same = gone ? (cb[i + 1] == UINT32_MAX && ce[i + 1] == UINT32_MAX) : ce[i + 1] >= cb[i + 1];
  }
  expect(same, "what was written is what is read");
  const std::vector<uint8_t> again = trf::clear_bytes(n, lens.data(), R, 5, 6);
  expect(trf::parse_clear(again, n, cb, ce, err) && cb[0] == 5 && ce[0] == 6, "entry 0 is kept");
  std::vector<uint8_t> bad(clr.begin(), clr.end() - 4);
  expect(!trf::parse_clear(bad, n, cb, ce, err), "a short clear range file is refused");
  bad.assign(clr.begin(), clr.begin() + 3);
  expect(!trf::parse_clear(bad, n, cb, ce, err), "a clear range file without a count is refused");
  bad.clear();
  expect(!trf::parse_clear(bad, n, cb, ce, err), "an empty clear range file is refused");
  bad = clr;
  bad.push_back(0);
  expect(!trf::parse_clear(bad, n, cb, ce, err), "a clear range file of odd length is refused");
  expect(!trf::parse_clear(clr, n + 1, cb, ce, err), "a clear range file of another store is refused");
  bad = clr;
  bad[0] ^= 1;
  expect(!trf::parse_clear(bad, n, cb, ce, err), "a wrong read count is refused");
  bad = clr;
  memset(bad.data(), 0xFF, 4);                          // a count whose size overflows 32 bits
  expect(!trf::parse_clear(bad, UINT32_MAX, cb, ce, err), "a huge read count is refused");

  // ---- the libraries file
  std::vector<uint8_t> libs;
  if (trf::read_file(d + "libraries", libs)) {
    const std::vector<uint32_t> want = load<uint32_t>(d + "final_trim.bin");
    std::vector<uint32_t> ft;
    expect(trf::parse_libraries(libs, (uint32_t)want.size() - 1, ft, err) && ft == want, "finalTrim of every library");
    expect(!trf::parse_libraries(libs, (uint32_t)want.size() + 40, ft, err), "a short libraries file is refused");
    libs.resize(100);
    expect(!trf::parse_libraries(libs, 0, ft, err), "a libraries file below one record is refused");
  }

  if (failures == 0) printf("tr_host_check: ok\n");
  return failures ? 1 : 0;
}
