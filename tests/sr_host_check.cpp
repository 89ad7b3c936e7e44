// sr_host_check.cpp -- the host code of canu_amd/bin/splitReads (canu_amd/csrc/sr_files.h) run by
// itself, so that it can be built with -fsanitize=address,undefined: the argument parser, the
// clear range file writer (and tr_files.h's reader), the stats formatter, the ERROR lines and the
// libraries reader.
//
//   sr_host_check <dir>
//
// <dir> holds what tests/test_sr_cpu.py wrote from one fixture: args.txt (the fixture's options,
// one per line), lengths.bin, bgn.bin, end.bin, clear_bgn.bin, clear_end.bin (uint32 per read),
// status.bin (uint8 per read), records.bin (ovl_record), fate.bin (uint8 per record),
// counters.bin (twenty pairs of uint64), entry0.bin (two uint32), the reference's want.clear,
// want.stats and want.errors (its stderr after the first line), and optionally libraries with
// lib_flags.bin (uint8 per library, from library 0).  Exit status 0: everything equal and every
// damaged input refused.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../canu_amd/csrc/sr_files.h"

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
  if (!srf::read_file(path, raw)) {
    fprintf(stderr, "FAIL: can't read %s\n", path.c_str());
    failures++;
  }
  std::vector<T> v(raw.size() / sizeof(T));
  if (!v.empty()) memcpy(v.data(), raw.data(), v.size() * sizeof(T));
  return v;
}

static bool parses(std::vector<std::string> words, srf::Job &J, std::string &err) {
  std::vector<const char *> argv{"splitReads"};
  for (const std::string &w : words) argv.push_back(w.c_str());
  J = srf::Job();
  return srf::parse_args((int)argv.size(), argv.data(), J, err);
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
  srf::Job J, X;
  std::string err;
  expect(parses(full, J, err) && J.clear_in == nullptr, "canu's command line parses, -Ci is optional");
  {
    std::vector<std::string> w = full;
    w.push_back("-Ci");
    w.push_back("in.clear");
    expect(parses(w, X, err) && X.clear_in && std::string(X.clear_in) == "in.clear", "-Ci is taken");
    w.assign(full.begin(), full.begin() + 4);
    w.insert(w.end(), full.begin() + 6, full.end());
    expect(!parses(w, X, err) && err.find("-Co") != std::string::npos, "a missing -Co is refused");
    w.assign(full.begin() + 2, full.end());
    expect(!parses(w, X, err) && err.find("-G") != std::string::npos, "a missing -G is refused");
    w = full;
    w.push_back("-t");
    expect(!parses(w, X, err), "an option without its value is refused");
    w.back() = "-bogus";
    expect(!parses(w, X, err) && err.find("unknown option") == 0, "an unknown option is refused");
    for (const char *gone : {"-ol", "-oc", "-Cm", "-l"}) {
      w = full;
      w.push_back(gone);
      w.push_back("1");
      expect(!parses(w, X, err), "trimReads' options are not splitReads'");
    }
    w = full;
    w.push_back("-e");
    w.push_back("-0.5");
    expect(!parses(w, X, err), "a negative -e is refused");
    w = full;
    w.push_back("-t");
    w.push_back("7");
    expect(parses(w, X, err) && X.id_min == 7 && X.id_max == 7, "-t with one number");
    w.back() = "3-9";
    expect(parses(w, X, err) && X.id_min == 3 && X.id_max == 9, "-t with a range");
  }

  // ---- the outputs
  std::vector<uint32_t> lens = load<uint32_t>(d + "lengths.bin"), bgn = load<uint32_t>(d + "bgn.bin"),
                        end = load<uint32_t>(d + "end.bin"), cb = load<uint32_t>(d + "clear_bgn.bin"),
                        ce = load<uint32_t>(d + "clear_end.bin"), entry0 = load<uint32_t>(d + "entry0.bin");
  std::vector<uint8_t> status = load<uint8_t>(d + "status.bin"), fate = load<uint8_t>(d + "fate.bin");
  std::vector<ovl_record> recs = load<ovl_record>(d + "records.bin");
  std::vector<uint64_t> cnt = load<uint64_t>(d + "counters.bin");
  const uint32_t n = (uint32_t)lens.size();
  expect(bgn.size() == n && end.size() == n && cb.size() == n && ce.size() == n && status.size() == n &&
             fate.size() == recs.size() && cnt.size() == 40 && entry0.size() == 2,
         "the inputs have one entry per read and per record");
  if (failures) return 1;
  sr_result R{};
  R.bgn = bgn.data();
  R.end = end.data();
  R.status = status.data();
  R.fate = fate.data();
  sr_stats S{};
  sr_count *c[20] = {&S.reads_in, &S.deleted_in, &S.no_trim_in, &S.no_overlaps, &S.no_coverage,
                     &S.proc_chimera, &S.proc_spur, &S.proc_subread, &S.reads_bad_spur5, &S.reads_bad_spur3,
                     &S.reads_bad_chimera, &S.reads_bad_subread, &S.bases_bad_spur5, &S.bases_bad_spur3,
                     &S.bases_bad_chimera, &S.bases_bad_subread, &S.trimmed5, &S.trimmed3, &S.no_change,
                     &S.deleted_out};
  for (int k = 0; k < 20; k++) *c[k] = sr_count{cnt[2 * k], cnt[2 * k + 1]};
  const std::vector<uint8_t> want_clear = load<uint8_t>(d + "want.clear"), want_stats = load<uint8_t>(d + "want.stats"),
                             want_errors = load<uint8_t>(d + "want.errors");
  const std::vector<uint8_t> clr = srf::clear_bytes(n, cb.data(), ce.data(), R, entry0[0], entry0[1]);
  expect(clr == want_clear, "the clear range file equals the reference's");
  const std::string sta = srf::stats_text(J.P, S);
  expect(sta == std::string(want_stats.begin(), want_stats.end()), "the stats equal the reference's");
  const std::string errs = srf::error_lines(recs.data(), recs.size(), fate.data());
  expect(errs == std::string(want_errors.begin(), want_errors.end()), "the ERROR lines equal the reference's");
  expect(srf::error_lines(nullptr, 0, nullptr).empty(), "no records, no lines");

  // ---- the clear range file, whole and damaged
  std::vector<uint32_t> ib, ie;
  expect(srf::parse_clear(clr, n, ib, ie, err) && ib.size() == (size_t)n + 1 && ie.size() == (size_t)n + 1 &&
             ib[0] == entry0[0] && ie[0] == entry0[1],
         "a whole clear range file loads, entry 0 kept");
  bool same = true;
  for (uint32_t i = 0; i < n && same; i++)
    same = status[i] == SR_DELETED_OUT ? (ib[i + 1] == UINT32_MAX && ie[i + 1] == UINT32_MAX)
                                       : status[i] == SR_TRIMMED ? (ib[i + 1] == bgn[i] && ie[i + 1] == end[i])
                                                                 : (ib[i + 1] == cb[i] && ie[i + 1] == ce[i]);
  expect(same, "what was written is what is read");
  std::vector<uint8_t> bad(clr.begin(), clr.end() - 4);
  expect(!srf::parse_clear(bad, n, ib, ie, err), "a short clear range file is refused");
  bad.assign(clr.begin(), clr.begin() + 3);
  expect(!srf::parse_clear(bad, n, ib, ie, err), "a clear range file without a count is refused");
  bad.clear();
  expect(!srf::parse_clear(bad, n, ib, ie, err), "an empty clear range file is refused");
  bad = clr;
  bad.push_back(0);
  expect(!srf::parse_clear(bad, n, ib, ie, err), "a clear range file of odd length is refused");
  expect(!srf::parse_clear(clr, n + 1, ib, ie, err), "a clear range file of another store is refused");
  bad = clr;
  memset(bad.data(), 0xFF, 4);                          // a count whose size overflows 32 bits
  expect(!srf::parse_clear(bad, UINT32_MAX, ib, ie, err), "a huge read count is refused");

  // ---- the libraries file
  std::vector<uint8_t> libs;
  if (srf::read_file(d + "libraries", libs)) {
    const std::vector<uint8_t> want = load<uint8_t>(d + "lib_flags.bin");
    std::vector<uint8_t> lf;
    expect(srf::parse_libraries(libs, (uint32_t)want.size() - 1, lf, err) && lf == want, "the switches of every library");
    expect(!srf::parse_libraries(libs, (uint32_t)want.size() + 40, lf, err), "a short libraries file is refused");
    libs.resize(100);
    expect(!srf::parse_libraries(libs, 0, lf, err), "a libraries file below one record is refused");
    libs.clear();
    expect(!srf::parse_libraries(libs, 0, lf, err), "an empty libraries file is refused");
  }

  if (failures == 0) printf("sr_host_check: ok\n");
  return failures ? 1 : 0;
}
