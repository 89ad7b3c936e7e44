// gfa_host.h -- the arithmetic alignGFA does in doubles (src/gfa/alignGFA.C), in plain C++ with
// the reference's types, for gfa.hip's host side and for tests/gfa_host_check.cpp.  Nothing of it
// runs on the device: a device double would be free to contract or reorder.
#ifndef CANU_GFA_HOST_H
#define CANU_GFA_HOST_H

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace gfa_host {

// checkLink (:198-238)
inline int32_t link_max_edit(int32_t align_len) { return (int32_t)ceil(align_len * 0.12); }
inline int32_t link_abgn_b(int32_t a_len, int32_t a_align) { return std::max(a_len - a_align, 0); }
inline int32_t link_bend_b(int32_t b_len, int32_t b_align) {
  return std::min(b_len, (int32_t)(1.10 * b_align));
}
inline int32_t link_abgn_a(int32_t a_len, int32_t a_align) {
  return std::max(a_len - (int32_t)(1.10 * a_align), 0);
}

// checkRecord_align (:336-340)
inline int32_t rec_max_edit(int32_t b_len) { return (int32_t)ceil(b_len * 0.03); }
inline int32_t rec_step(int32_t b_len) { return (int32_t)ceil(b_len * 0.15); }
inline void rec_window(int32_t a_len, int32_t b_len, int32_t step, int32_t &abgn, int32_t &aend) {
  aend = std::min(aend + 2 * step, a_len);
  abgn = std::max(aend - b_len - 2 * step, 0);
}
// :435-443: `maxEdit *= 1.2` is an int32 times a double, converted back
inline bool rec_can_relax(int32_t abgn, int32_t aend, int32_t b_len, int32_t max_edit) {
  return (aend - abgn < 4 * b_len) && (max_edit < b_len * 0.25);
}
inline int32_t rec_relax(int32_t max_edit) { return (int32_t)(max_edit * 1.2); }
// :382-383
inline int32_t rec_align_len(int32_t nbgn, int32_t nend, int32_t b_len, int32_t dist) {
  return ((nend - nbgn) + b_len + dist) / 2;
}
inline int32_t rec_score(int32_t dist, int32_t align_len) {
  return 1000 - (int32_t)(1000.0 * dist / align_len);
}
// :406-407: the alignment touches no edge of the window, or the edge is the contig's
inline bool rec_accept(int32_t abgn, int32_t aend, int32_t nbgn, int32_t nend, int32_t a_len) {
  return ((abgn < nbgn) || (abgn == 0)) && ((nend < aend) || (aend == a_len));
}
// checkLink's last -V line (:300)
inline double link_ratio(int32_t dist, int32_t align_len) { return (double)dist / align_len; }

}  // namespace gfa_host

#endif
