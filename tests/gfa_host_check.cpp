// gfa_host_check.cpp -- a stand-alone check of alignGFA's host code (canu_amd/csrc/gfa_files.h,
// gfa_host.h), built with the address and undefined-behaviour sanitizers and run by
// tests/test_gfa_cpu.py on a directory it fills from the fixtures:
//
//   gfa_host_check DIR      DIR/cases.txt, one case a line:
//     gfa FILE | bed FILE                     parse, write again: the bytes of FILE
//     badgfa FILE | badbed FILE               must be refused
//     cigar CIGAR Q R A                       gfaLink::alignmentLength
//     store DIR VERSION FILE                  the tigs of the store: FILE's lines
//     damage DIR VERSION                      the store cut at and around every record boundary,
//                                             with damaged counts: refused, or read in bounds
//     link ALEN BLEN AA BA AL MAXEDIT ABGN_B BEND_B ABGN_A     checkLink's arithmetic
//     window ALEN BLEN BGN END ABGN AEND MAXEDIT                checkRecord_align's window
//     relax MAXEDIT NEXT                                        maxEdit *= 1.2
//     score NBGN NEND BLEN DIST ALIGNLEN SCORE
//     ratio DIST ALIGNLEN TEXT                                  %.4f
// It prints one line per failure and exits with their number.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../canu_amd/csrc/gfa_files.h"
#include "../canu_amd/csrc/gfa_host.h"

static int failures = 0;

static void fail(const std::string &what) {
  printf("FAIL %s\n", what.c_str());
  failures++;
}

static std::string slurp_text(const std::string &path) {
  std::vector<uint8_t> raw;
  std::string err;
  if (!tgs::slurp(path, raw, err)) { fail("cannot read " + path); return ""; }
  return std::string(raw.begin(), raw.end());
}

static void damage(const std::string &dir, uint32_t version) {
  char name[64];
  snprintf(name, sizeof name, "/seqDB.v%03u.tig", version);
  std::vector<uint8_t> tig, dat;
  std::string err;
  if (!tgs::slurp(dir + name, tig, err)) { fail(err); return; }
  snprintf(name, sizeof name, "/seqDB.v%03u.dat", version);
  if (!tgs::slurp(dir + name, dat, err)) { fail(err); return; }
  std::vector<std::string> whole, got;
  std::vector<uint8_t> d = dat;
  const gfa_files::DataFile data = [&](uint32_t) { return &d; };
  if (!gfa_files::parse_tig_bases(tig.data(), tig.size(), data, whole, err)) { fail("whole store: " + err); return; }
  // the record boundaries, from the index
  std::vector<uint64_t> cuts;
  const uint32_t n = tgs::get<uint32_t>(tig.data() + 16);
  for (uint32_t k = 0; k < n; k++) {
    const uint64_t word = tgs::get<uint64_t>(tig.data() + tgs::HEADER_BYTES + (size_t)k * tgs::ENTRY_BYTES + tgs::RECORD_BYTES);
    if (!((word >> 13) & 1)) cuts.push_back(word >> 24);
  }
  for (uint64_t c : cuts)
    for (int64_t delta : {-1, 0, 1, 4, 51, 52, 53}) {
      const int64_t at = (int64_t)c + delta;
      if (at < 0 || at >= (int64_t)dat.size()) continue;
      d.assign(dat.begin(), dat.begin() + at);
      if (gfa_files::parse_tig_bases(tig.data(), tig.size(), data, got, err))
        fail("a data file cut at " + std::to_string(at) + " was read");
    }
  // damaged counts: the gapped length, the children and the deltas of every record, in the data
  // file alone and in both files
  for (uint64_t c : cuts)
    for (int field : {32, 36, 40})
      for (uint32_t v : {0x7fffffffu, 0xffffffffu, 0x00ffffffu}) {
        d = dat;
        memcpy(d.data() + c + 4 + field, &v, 4);
        if (gfa_files::parse_tig_bases(tig.data(), tig.size(), data, got, err) && got != whole && field == 32)
          fail("a damaged gapped length was read");
      }
  d = dat;
  for (uint32_t v : {0u, n + 1, 0xffffffffu}) {                  // the number of entries
    std::vector<uint8_t> t = tig;
    memcpy(t.data() + 16, &v, 4);
    if (gfa_files::parse_tig_bases(t.data(), t.size(), data, got, err)) fail("a damaged entry count was read");
  }
  for (size_t len : {(size_t)0, (size_t)19, tig.size() - 1, tig.size() - 56})
    if (len < tig.size() && gfa_files::parse_tig_bases(tig.data(), len, data, got, err))
      fail("an index of " + std::to_string(len) + " bytes was read");
  std::vector<uint8_t> t = tig;
  t[0] ^= 1;
  if (gfa_files::parse_tig_bases(t.data(), t.size(), data, got, err)) fail("a damaged magic number was read");
}

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s DIR\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  std::ifstream cases(dir + "/cases.txt");
  if (!cases) { fprintf(stderr, "no %s/cases.txt\n", dir.c_str()); return 2; }
  std::string line;
  int ncases = 0;
  while (std::getline(cases, line)) {
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    if (kind.empty()) continue;
    ncases++;
    std::string err;
    if (kind == "gfa" || kind == "badgfa") {
      std::string f;
      in >> f;
      const std::string text = slurp_text(dir + "/" + f);
      gfa_files::Gfa g;
      const bool ok = gfa_files::parse_gfa(text, g, err);
      if (kind == "badgfa") { if (ok) fail(line + ": read"); continue; }
      if (!ok) { fail(line + ": " + err); continue; }
      if (gfa_files::save_gfa(g) != text) fail(line + ": written differently");
      for (const gfa_files::Link &l : g.links) {
        int32_t q, r, a;
        std::string warn;
        gfa_files::alignment_length(l.cigar, q, r, a, warn);
      }
    } else if (kind == "bed" || kind == "badbed") {
      std::string f;
      in >> f;
      const std::string text = slurp_text(dir + "/" + f);
      std::vector<gfa_files::Record> recs;
      const bool ok = gfa_files::parse_bed(text, recs, err);
      if (kind == "badbed") { if (ok) fail(line + ": read"); continue; }
      if (!ok) { fail(line + ": " + err); continue; }
      if (gfa_files::save_bed(recs) != text) fail(line + ": written differently");
    } else if (kind == "cigar") {
      std::string cg, warn;
      int32_t q, r, a, wq, wr, wa;
      in >> cg >> wq >> wr >> wa;
      gfa_files::alignment_length(cg, q, r, a, warn);
      if (q != wq || r != wr || a != wa) fail(line);
    } else if (kind == "store") {
      std::string d, f;
      uint32_t v;
      in >> d >> v >> f;
      std::vector<std::string> tigs;
      if (!gfa_files::load_tig_bases(dir + "/" + d, v, tigs, err)) { fail(line + ": " + err); continue; }
      std::string all;
      for (const std::string &t : tigs) all += t + "\n";
      if (all != slurp_text(dir + "/" + f)) fail(line + ": other bases");
    } else if (kind == "damage") {
      std::string d;
      uint32_t v;
      in >> d >> v;
      damage(dir + "/" + d, v);
    } else if (kind == "link") {
      int32_t alen, blen, aa, ba, al, me, abgn_b, bend_b, abgn_a;
      in >> alen >> blen >> aa >> ba >> al >> me >> abgn_b >> bend_b >> abgn_a;
      if (gfa_host::link_max_edit(al) != me || gfa_host::link_abgn_b(alen, aa) != abgn_b ||
          gfa_host::link_bend_b(blen, ba) != bend_b || gfa_host::link_abgn_a(alen, aa) != abgn_a)
        fail(line);
    } else if (kind == "window") {
      int32_t alen, blen, bgn, end, abgn, aend, me;
      in >> alen >> blen >> bgn >> end >> abgn >> aend >> me;
      int32_t b = bgn, e = end;
      gfa_host::rec_window(alen, blen, gfa_host::rec_step(blen), b, e);
      if (b != abgn || e != aend || gfa_host::rec_max_edit(blen) != me) fail(line);
    } else if (kind == "relax") {
      int32_t me, next;
      in >> me >> next;
      if (gfa_host::rec_relax(me) != next) fail(line);
    } else if (kind == "score") {
      int32_t nbgn, nend, blen, dist, al, sc;
      in >> nbgn >> nend >> blen >> dist >> al >> sc;
      if (gfa_host::rec_align_len(nbgn, nend, blen, dist) != al || gfa_host::rec_score(dist, al) != sc)
        fail(line);
    } else if (kind == "ratio") {
      int32_t dist, al;
      std::string text;
      in >> dist >> al >> text;
      char buf[32];
      snprintf(buf, sizeof buf, "%.4f", gfa_host::link_ratio(dist, al));
      if (text != buf) fail(line);
    } else {
      fail("unknown case: " + line);
    }
  }
  printf("%d cases, %d failures\n", ncases, failures);
  return failures > 255 ? 255 : failures;
}
