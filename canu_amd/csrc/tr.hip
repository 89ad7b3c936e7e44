// tr.hip -- libcanu_tr.so: canu's trimReads on gfx950 (include/canu_tr.h).
//
//   k_tr_segment   one thread per overlap record: checks it (IDs in order, a_bgn < a_end) and
//                  writes its end points and whether -e skips it (8 bytes for the 24 read)
//   k_tr_offsets   one thread per read: where the read's overlaps start (a binary search; the
//                  records are sorted by a_iid)
//   k_tr_wave      one wave per read, reads in descending order of overlap count, everything in
//                  LDS: the used overlaps' end-point keys (position, open before close) and
//                  (lo, hi) keys are sorted by a bitonic network; the depth list is a prefix
//                  sum of +1 / -1 over the end points; the merge of intervalList::merge is a
//                  prefix maximum of hi; the two-pointer intersection is two binary searches
//                  per merged interval; the first strictly longest interval is a wave maximum.
//                  Rule 2 then runs bestEdge's point loops, one point after the other, lanes
//                  over the overlaps.
//   k_tr_large_keys, hipcub's segmented radix sort, k_tr_large
//                  the same for a read with more than TR_WAVE_CAP overlaps, its lists in device
//                  memory, each sized from the read's overlap count.
//
// intervalList::computeDepth is not a plain depth list: where closes follow opens at one
// position it can fold the piece it just opened back into the one before and then lower that
// piece's count (tests/tr_restate.py, IntervalList.depth_of).  That changes which pieces reach
// -oc only with -oc >= 2 and an open and a close at one position; the sweep looks for exactly
// that and lane 0 then walks the sorted events as the reference does.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/canu_tr.h"
#include "capi_common.h"

#define TR_WAVE_CAP 512u      // overlaps of a read k_tr_wave holds in LDS (a power of two)
#define AS_MAX_READLEN ((1u << 21) - 1)
#define AS_MAX_EVALUE 4095u

namespace {

using capi::fail;

CAPI_SAME_CODES(TR);

enum { E_BAD_ID = 1, E_UNSORTED = 2, E_BAD_SPAN = 4 };
enum { F_OK = 1, F_RESET = 2, F_LITERAL = 4 };           // k_tr_wave's flags of a read

struct DevParams {
  uint32_t ev_max, min_overlap, min_coverage;
};

// ------------------------------------------------------------------------------ the records

__global__ __launch_bounds__(256) void k_tr_segment(const ovl_record *__restrict__ rec, uint64_t n,
                                                    const uint32_t *__restrict__ lengths,
                                                    uint32_t num_reads, uint32_t ev_max,
                                                    uint2 *__restrict__ span, int *__restrict__ err,
                                                    unsigned long long *__restrict__ where) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t a = rec[i].a_iid;
  const uint64_t w0 = rec[i].dat[0];
  int e = 0;
  if (a == 0 || a > num_reads) e |= E_BAD_ID;
  if (i > 0 && rec[i - 1].a_iid > a) e |= E_UNSORTED;
  uint32_t bgn = 0, end = 0;
  if (!(e & E_BAD_ID)) {
    const uint32_t len = lengths[a - 1];
    const uint32_t h5 = (uint32_t)(w0 & AS_MAX_READLEN), h3 = (uint32_t)((w0 >> 21) & AS_MAX_READLEN);
    if ((uint64_t)h5 + h3 >= len) e |= E_BAD_SPAN;     // a_bgn >= a_end, or a_end wraps
    bgn = h5;
    end = len - h3;
  }
  const uint32_t skip = ((uint32_t)(w0 >> 42) & AS_MAX_EVALUE) > ev_max;
  span[i] = make_uint2(bgn, (end << 1) | skip);
  if (e) {
    atomicOr(err, e);
    atomicMin(where, (unsigned long long)i);
  }
}

// off[r], r = 0 .. num_reads + 1: the first record whose a_iid is >= r.
__global__ __launch_bounds__(256) void k_tr_offsets(const ovl_record *__restrict__ rec, uint64_t n,
                                                    uint32_t num_reads, uint64_t *__restrict__ off) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r > num_reads + 1) return;
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (rec[mid].a_iid < r) lo = mid + 1; else hi = mid;
  }
  off[r] = lo;
}

// ------------------------------------------------------------------------------ wave helpers

__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1; }

template <class T>
__device__ __forceinline__ T wave_incl_add(T v, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}

__device__ __forceinline__ uint32_t wave_incl_max(uint32_t v, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = __shfl_up(v, o);
    if (lane >= o) v = max(v, u);
  }
  return v;
}

template <class T>
__device__ __forceinline__ T wave_max(T v) {
  for (int o = 32; o > 0; o >>= 1) {
    const T u = __shfl_xor(v, o);
    v = u > v ? u : v;
  }
  return v;
}

__device__ __forceinline__ uint32_t pow2_at_least(uint32_t n) {
  uint32_t m = 1;
  while (m < n) m <<= 1;
  return m;
}

// Ascending bitonic sort of a[0 .. m), m a power of two, by the 64 threads of the block.
template <class T>
__device__ void bitonic_sort(T *a, uint32_t m, int lane) {
  for (uint32_t k = 2; k <= m; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = lane; t < (m >> 1); t += 64) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const T x = a[i], y = a[l];
        if ((x > y) == ((i & k) == 0)) {
          a[i] = y;
          a[l] = x;
        }
      }
      __syncthreads();
    }
}

// The lists of one read.  k_tr_wave points them into LDS, k_tr_large into device memory.
struct Lists {
  uint32_t *ev;     // 2 n end-point keys (position << 1 | close), sorted; later every overlap's
                    // (bgn << 32 | end) for bestEdge, as uint64
  uint64_t *iv;     // n (lo << 32 | hi) keys, sorted; then the merged intervals; later the trim
                    // points of bestEdge where t5 / t3 are null
  uint32_t *idlo, *idhi;   // the depth runs
  uint64_t *stack;  // the literal depth walk's pieces (lo << 32 | ct); null: packed into ev
  uint32_t *t5, *t3;       // bestEdge's trim points, a power of two of room; null: in iv
};

// intervalList::computeDepth and the ID loop of largestCovered as the reference walks them, by
// one lane.  Pieces are (lo, ct); a piece's hi is the next one's lo.
template <bool LARGE>
__device__ uint32_t depth_runs_literal(const Lists &L, uint32_t nev, uint32_t min_cov) {
  auto put = [&](uint32_t k, uint32_t lo, uint32_t ct) {
    if (LARGE) L.stack[k] = ((uint64_t)lo << 32) | ct; else L.ev[k] = (lo << 11) | ct;
  };
  auto lo_of = [&](uint32_t k) { return LARGE ? (uint32_t)(L.stack[k] >> 32) : L.ev[k] >> 11; };
  auto ct_of = [&](uint32_t k) { return LARGE ? (uint32_t)L.stack[k] : L.ev[k] & 2047u; };
  uint32_t key = L.ev[0];
  uint32_t prev_pos = key >> 1, top = 0, top_lo = prev_pos, top_hi = prev_pos, top_ct = 1;
  for (uint32_t i = 1; i < nev; i++) {
    key = L.ev[i];                                     // read before piece i can be written
    const uint32_t pos = key >> 1;
    top_hi = pos;
    const uint32_t nct = (key & 1) ? top_ct - 1 : top_ct + 1;
    if (prev_pos != pos && top_lo != top_hi) {
      put(top, top_lo, top_ct);
      top++;
      top_lo = pos;
    }
    top_hi = pos;
    top_ct = nct;
    if (top > 1 && ct_of(top - 1) == top_ct) {         // the piece before ends where this begins
      top--;
      top_lo = lo_of(top);
    }
    prev_pos = pos;
  }
  put(top, top_lo, top_ct);                            // its lo closes the piece before it
  uint32_t nid = 0, ib = 0, ie = 0;
  for (uint32_t k = 0; k < top; k++) {
    const uint32_t lo = lo_of(k), hi = lo_of(k + 1), ct = ct_of(k);
    if (ct < min_cov) {
      if (ie > ib) { L.idlo[nid] = ib; L.idhi[nid] = ie; nid++; }
      ib = ie = 0;
    } else if (ib == 0 && ie == 0) {
      ib = lo; ie = hi;
    } else if (ie == lo) {
      ie = hi;
    } else {
      if (ie > ib) { L.idlo[nid] = ib; L.idhi[nid] = ie; nid++; }
      ib = lo; ie = hi;
    }
  }
  if (ie > ib) { L.idlo[nid] = ib; L.idhi[nid] = ie; nid++; }
  return nid;
}

// The maximal runs of depth >= min_cov over the sorted end points -> idlo / idhi; *literal is
// set where the reference's list can differ from the true depth.
__device__ uint32_t depth_runs(const Lists &L, uint32_t nev, uint32_t min_cov, int lane, bool *literal) {
  int depth = 0;
  bool carry_good = false, touch = false;
  uint32_t nstart = 0, nend = 0;
  for (uint32_t c = 0; c < nev; c += 64) {
    const uint32_t i = c + lane;
    const bool valid = i < nev;
    const uint32_t k = valid ? L.ev[i] : 0, kn = i + 1 < nev ? L.ev[i + 1] : 0xFFFFFFFFu;
    const int d = depth + wave_incl_add<int>(valid ? ((k & 1) ? -1 : 1) : 0, lane);
    const bool piece_end = valid && (kn >> 1) != (k >> 1);
    const bool good = piece_end && d >= (int)min_cov;
    touch |= valid && !(k & 1) && i + 1 < nev && (kn & 1) && (kn >> 1) == (k >> 1);
    const uint64_t pmask = __ballot(piece_end), gmask = __ballot(good);
    const uint64_t below = pmask & lanes_below(lane);
    const bool prev_good = below ? ((gmask >> (63 - __clzll(below))) & 1) : carry_good;
    const bool start = good && !prev_good, stop = piece_end && !good && prev_good;
    const uint64_t smask = __ballot(start), emask = __ballot(stop);
    if (start) L.idlo[nstart + __popcll(smask & lanes_below(lane))] = k >> 1;
    if (stop) L.idhi[nend + __popcll(emask & lanes_below(lane))] = k >> 1;
    nstart += __popcll(smask);
    nend += __popcll(emask);
    if (pmask) carry_good = (gmask >> (63 - __clzll(pmask))) & 1;
    depth = __shfl(d, 63);
  }
  *literal = min_cov >= 2 && __ballot(touch) != 0;
  return nstart;                                       // == nend: the last piece has depth 0
}

// intervalList::merge(min_overlap) over the sorted (lo, hi) keys, in place -> merged intervals.
__device__ uint32_t merge_intervals(uint64_t *iv, uint32_t n, uint32_t min_overlap, int lane) {
  uint32_t pm_carry = 0, glo_carry = 0, nil = 0;
  for (uint32_t c = 0; c < n; c += 64) {
    const uint32_t i = c + lane;
    const bool valid = i < n;
    const uint64_t v = valid ? iv[i] : 0, vn = i + 1 < n ? iv[i + 1] : 0;
    const uint32_t lo = (uint32_t)(v >> 32), hi = (uint32_t)v;
    const uint32_t pm = max(pm_carry, wave_incl_max(hi, lane));
    uint32_t pm_prev = __shfl_up(pm, 1);
    if (lane == 0) pm_prev = pm_carry;
    // a group breaks before an interval neither thickly overlapped (in uint32) nor contained
    const bool brk = valid && (i == 0 || (!(pm_prev - min_overlap >= lo) && !(hi <= pm_prev)));
    const uint32_t lon = (uint32_t)(vn >> 32), hin = (uint32_t)vn;
    const bool last = valid && (i + 1 == n || (!(pm - min_overlap >= lon) && !(hin <= pm)));
    const uint64_t bmask = __ballot(brk);
    const uint64_t upto = bmask & (lanes_below(lane) | (1ull << lane));
    const uint32_t from = __shfl(lo, upto ? 63 - __clzll(upto) : 0);
    const uint32_t glo = upto ? from : glo_carry;
    const uint64_t lmask = __ballot(last);
    __syncthreads();                                   // every lane has read its two keys
    if (last) iv[nil + __popcll(lmask & lanes_below(lane))] = ((uint64_t)glo << 32) | pm;
    nil += __popcll(lmask);
    pm_carry = __shfl(pm, 63);
    glo_carry = __shfl(glo, 63);
    __syncthreads();
  }
  return nil;
}

__device__ __forceinline__ uint32_t first_hi_at_least(const uint32_t *idhi, uint32_t nid, uint32_t x) {
  uint32_t lo = 0, hi = nid;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (idhi[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The first strictly longest interval the two-pointer walk of largestCovered:159-204 adds (of
// the merged intervals themselves where there are no depth runs to intersect with).
__device__ bool longest_interval(const Lists &L, uint32_t nil, uint32_t nid, bool use_id, int lane,
                                 uint32_t *fbgn, uint32_t *fend) {
  uint32_t best_len = 0, best_bgn = 0, best_end = 0;
  for (uint32_t c = 0; c < nil; c += 64) {
    const uint32_t l = c + lane;
    uint32_t len = 0, b = 0, e = 0;
    if (l < nil) {
      const uint64_t v = L.iv[l];
      const uint32_t ll = (uint32_t)(v >> 32), lh = (uint32_t)v;
      if (!use_id) {
        len = lh - ll; b = ll; e = lh;
      } else {
        // both lists ascend strictly in hi: interval l meets the runs first .. last
        uint32_t first = 0;
        if (l > 0) {
          const uint32_t ph = (uint32_t)L.iv[l - 1];
          first = first_hi_at_least(L.idhi, nid, ph);
          if (first < nid && L.idhi[first] == ph) first++;
        }
        const uint32_t last = first_hi_at_least(L.idhi, nid, lh);
        for (uint32_t d = first; d <= last && d < nid; d++) {
          const uint32_t dl = L.idlo[d], dh = L.idhi[d];
          uint32_t nl = 0, nh = 0;
          if (ll <= dl && dl < lh) { nl = dl; nh = lh < dh ? lh : dh; }
          if (dl <= ll && ll < dh) { nl = ll; nh = lh < dh ? lh : dh; }
          if (nl < nh && nh - nl > len) { len = nh - nl; b = nl; e = nh; }
        }
      }
    }
    const uint64_t key = wave_max<uint64_t>(((uint64_t)len << 32) | (0xFFFFFFFFu - l));
    const uint32_t wlen = (uint32_t)(key >> 32), wl = 0xFFFFFFFFu - (uint32_t)key;
    const uint32_t wb = __shfl(b, wl & 63), we = __shfl(e, wl & 63);
    if (wlen > best_len) { best_len = wlen; best_bgn = wb; best_end = we; }
  }
  *fbgn = best_bgn;
  *fend = best_end;
  return best_len > 0;
}

// bestEdge after its largestCovered call (lbgn .. lend), trimReads-bestEdge.C:81-402.
__device__ bool best_edge(const Lists &L, const uint2 *span, uint32_t nall, uint32_t len, uint32_t lbgn,
                          uint32_t lend, int lane, uint32_t *fbgn, uint32_t *fend) {
  uint64_t *all = (uint64_t *)L.ev;
  uint32_t *t5 = L.t5 ? L.t5 : (uint32_t *)L.iv, *t3 = L.t3 ? L.t3 : (uint32_t *)L.iv + TR_WAVE_CAP;
  uint32_t n5 = 0, n3 = 0, contained = 0;
  __syncthreads();
  for (uint32_t c = 0; c < nall; c += 64) {
    const uint32_t i = c + lane;
    bool p5 = false, p3 = false, con = false;
    uint32_t tb = 0, te = 0;
    if (i < nall) {
      const uint2 s = span[i];
      tb = s.x; te = s.y >> 1;
      all[i] = ((uint64_t)tb << 32) | te;
      if (!(lend <= tb || te <= lbgn) && !(s.y & 1)) {
        p5 = lbgn <= tb;
        p3 = te <= lend;
        con = tb == 0 && te == len;
      }
    }
    const uint64_t m5 = __ballot(p5), m3 = __ballot(p3);
    if (p5) t5[n5 + __popcll(m5 & lanes_below(lane))] = tb;
    if (p3) t3[n3 + __popcll(m3 & lanes_below(lane))] = ~te;     // ascending ~te: outside-in
    n5 += __popcll(m5);
    n3 += __popcll(m3);
    contained += __popcll(__ballot(con));
  }
  if (contained >= 2) n5 = n3 = 0;
  const uint32_t m5 = pow2_at_least(n5), m3 = pow2_at_least(n3);
  for (uint32_t i = n5 + lane; i < m5; i += 64) t5[i] = 0xFFFFFFFFu;
  for (uint32_t i = n3 + lane; i < m3; i += 64) t3[i] = 0xFFFFFFFFu;
  __syncthreads();
  bitonic_sort(t5, m5, lane);
  bitonic_sort(t3, m3, lane);

  // the 5' points: lbgn, then every distinct point beyond it
  uint32_t best5 = lbgn, best5score = 0, best5end = 0, prev = 0;
  for (uint32_t j = 0; j <= n5; j++) {
    const uint32_t triml = j == 0 ? lbgn : t5[j - 1];
    if (j > 0 && triml == prev) continue;
    prev = triml;
    if (best5score >= len - triml) break;
    uint32_t score = 0;
    for (uint32_t i = lane; i < nall; i += 64) {
      const uint64_t v = all[i];
      const uint32_t tb = (uint32_t)(v >> 32), te = (uint32_t)v;
      if (triml < tb || te <= triml) continue;
      score = max(score, min(te, lend) - triml);
    }
    score = wave_max<uint32_t>(score);
    const uint32_t scend = score ? triml + score : 0;  // equal scores end at equal places
    if ((double)score < best5score * 0.66) break;
    if (best5score < score && best5end < scend) { best5 = triml; best5score = score; best5end = scend; }
  }
  uint32_t best3 = lend, best3score = 0, best3bgn = 0xFFFFFFFFu;
  prev = 0;
  for (uint32_t j = 0; j <= n3; j++) {
    const uint32_t trimr = j == 0 ? lend : ~t3[j - 1];
    if (j > 0 && trimr == prev) continue;
    prev = trimr;
    if (best3score >= trimr) break;
    uint32_t score = 0;
    for (uint32_t i = lane; i < nall; i += 64) {
      const uint64_t v = all[i];
      const uint32_t tb = (uint32_t)(v >> 32), te = (uint32_t)v;
      if (te < trimr || trimr <= tb) continue;
      score = max(score, trimr - max(tb, lbgn));
    }
    score = wave_max<uint32_t>(score);
    const uint32_t scbgn = score ? trimr - score : 0;
    if ((double)score < best3score * 0.66) break;
    if (best3score < score && scbgn < best3bgn) { best3 = trimr; best3score = score; best3bgn = scbgn; }
  }
  uint32_t b = best5, e = best3;
  if (b + 4 < e && 2 < e) { b += 2; e -= 2; }
  if (b < lbgn) b = lbgn;
  if (lend < e) e = lend;
  bool reset = false;
  if (e < b) { b = lbgn; e = lend; reset = true; }
  *fbgn = b;
  *fend = e;
  return reset;
}

struct ReadOut {
  uint32_t *bgn, *end, *n_skipped, *n_used;
  uint8_t *flags;
};

// One read by one wave.  LARGE: ev and iv come sorted (their n_used valid keys first).
template <bool LARGE>
__device__ void trim_one(const Lists &L, const uint2 *span, uint32_t nall, uint32_t read, uint32_t len,
                         uint32_t rule, DevParams P, ReadOut out, int lane) {
  uint32_t n = 0;
  for (uint32_t c = 0; c < nall; c += 64) {
    const uint32_t i = c + lane;
    const uint2 s = i < nall ? span[i] : make_uint2(0, 1);
    const bool used = !(s.y & 1);
    const uint64_t um = __ballot(used);
    if (!LARGE && used) {
      const uint32_t k = n + __popcll(um & lanes_below(lane));
      L.ev[2 * k] = s.x << 1;
      L.ev[2 * k + 1] = s.y | 1;                       // (end << 1) | close
      L.iv[k] = ((uint64_t)s.x << 32) | (s.y >> 1);
    }
    n += __popcll(um);
  }
  bool ok = false, reset = false, literal = false;
  uint32_t fbgn = 0, fend = len;
  if (n > 0) {
    if (!LARGE) {
      const uint32_t me = pow2_at_least(2 * n), mi = pow2_at_least(n);
      for (uint32_t i = 2 * n + lane; i < me; i += 64) L.ev[i] = 0xFFFFFFFFu;
      for (uint32_t i = n + lane; i < mi; i += 64) L.iv[i] = ~0ull;
      __syncthreads();
      bitonic_sort(L.ev, me, lane);
      bitonic_sort(L.iv, mi, lane);
    }
    uint32_t nid = 0;
    if (P.min_coverage > 0) {
      nid = depth_runs(L, 2 * n, P.min_coverage, lane, &literal);
      if (literal) {
        __syncthreads();
        if (lane == 0) nid = depth_runs_literal<LARGE>(L, 2 * n, P.min_coverage);
        nid = __shfl(nid, 0);
      }
      __syncthreads();
    }
    const uint32_t nil = merge_intervals(L.iv, n, P.min_overlap, lane);
    uint32_t lbgn, lend;
    ok = longest_interval(L, nil, nid, P.min_coverage > 0, lane, &lbgn, &lend);
    if (ok) {
      fbgn = lbgn;
      fend = lend;
      if (rule == 2) reset = best_edge(L, span, nall, len, lbgn, lend, lane, &fbgn, &fend);
    }
  }
  if (lane == 0) {
    out.bgn[read] = fbgn;
    out.end[read] = fend;
    out.n_skipped[read] = nall - n;
    out.n_used[read] = n;
    out.flags[read] = (ok ? F_OK : 0) | (reset ? F_RESET : 0) | (literal ? F_LITERAL : 0);
  }
}

// order[block]: the read (1-based); off[r]: its first record.  Arrays of `out` are indexed by
// the read ID.
__global__ __launch_bounds__(64) void k_tr_wave(const uint32_t *__restrict__ order,
                                                const uint64_t *__restrict__ off,
                                                const uint2 *__restrict__ span,
                                                const uint32_t *__restrict__ lengths,
                                                const uint8_t *__restrict__ rules, DevParams P,
                                                ReadOut out) {
  __shared__ __align__(8) uint32_t s_ev[2 * TR_WAVE_CAP];   // bestEdge reads it as uint64
  __shared__ uint64_t s_iv[TR_WAVE_CAP];
  __shared__ uint32_t s_idlo[TR_WAVE_CAP], s_idhi[TR_WAVE_CAP];
  const uint32_t read = order[blockIdx.x];
  const uint64_t first = off[read];
  const uint32_t nall = (uint32_t)(off[read + 1] - first);
  if (nall > TR_WAVE_CAP) return;                      // the host never sends one
  Lists L{s_ev, s_iv, s_idlo, s_idhi, nullptr, nullptr, nullptr};
  trim_one<false>(L, span + first, nall, read, lengths[read - 1], rules[read - 1], P, out,
                  (int)threadIdx.x);
}

// The lists of large read k lie at base[k] (in overlaps) of each array, twice that in ev and
// stack; its trim points at pbase[k].
__global__ __launch_bounds__(256) void k_tr_large_keys(const uint32_t *__restrict__ order,
                                                       const uint64_t *__restrict__ off,
                                                       const uint64_t *__restrict__ base,
                                                       const uint2 *__restrict__ span,
                                                       uint32_t *__restrict__ ev,
                                                       uint64_t *__restrict__ iv) {
  const uint32_t read = order[blockIdx.y];
  const uint64_t first = off[read];
  const uint32_t nall = (uint32_t)(off[read + 1] - first);
  const uint64_t b = base[blockIdx.y];
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nall; i += gridDim.x * 256) {
    const uint2 s = span[first + i];
    const bool used = !(s.y & 1);
    ev[2 * (b + i)] = used ? s.x << 1 : 0xFFFFFFFFu;
    ev[2 * (b + i) + 1] = used ? (s.y | 1) : 0xFFFFFFFFu;
    iv[b + i] = used ? ((uint64_t)s.x << 32) | (s.y >> 1) : ~0ull;
  }
}

__global__ __launch_bounds__(64) void k_tr_large(const uint32_t *__restrict__ order,
                                                 const uint64_t *__restrict__ off,
                                                 const uint64_t *__restrict__ base,
                                                 const uint64_t *__restrict__ pbase,
                                                 const uint2 *__restrict__ span,
                                                 const uint32_t *__restrict__ lengths,
                                                 const uint8_t *__restrict__ rules, uint32_t *ev,
                                                 uint64_t *iv, uint32_t *idlo, uint32_t *idhi,
                                                 uint64_t *stack, uint32_t *t5, uint32_t *t3,
                                                 DevParams P, ReadOut out) {
  const uint32_t read = order[blockIdx.x];
  const uint64_t first = off[read];
  const uint32_t nall = (uint32_t)(off[read + 1] - first);
  const uint64_t b = base[blockIdx.x], pb = pbase[blockIdx.x];
  // bestEdge keeps every overlap's span where the end points were: 2 * nall uint32 hold nall uint64
  Lists L{ev + 2 * b, iv + b, idlo + b, idhi + b, stack + 2 * b, t5 + pb, t3 + pb};
  trim_one<true>(L, span + first, nall, read, lengths[read - 1], rules[read - 1], P, out,
                 (int)threadIdx.x);
}

uint32_t encode_evalue(double q) {                     // AS_OVS_encodeEvalue, ovOverlap.H:44-45
  return q < AS_MAX_EVALUE / 10000.0 ? (uint32_t)(10000.0 * q + 0.5) : AS_MAX_EVALUE;
}

int check_params(const tr_params *p) {
  if (!p) return fail(TR_ERR_BAD_PARAM, "no parameters");
  if (!(p->erate >= 0.0)) return fail(TR_ERR_BAD_PARAM, "erate %g is negative", p->erate);
  return TR_OK;
}

}  // namespace

struct tr_ctx : capi::Device {
  tr_params P{};
  tr_stats S{};
};

extern "C" {

void tr_params_init(tr_params *p) {
  p->erate = 0.015;
  p->min_read_length = 64;
  p->min_evidence_overlap = 40;
  p->min_evidence_coverage = 1;
}

const char *tr_last_error(void) { return capi::g_err.c_str(); }
int tr_abi_version(void) { return TR_ABI_VERSION; }
uint32_t tr_wave_capacity(void) { return TR_WAVE_CAP; }

int tr_ctx_create(const tr_params *p, int device, tr_ctx **out) {
  if (!out) return fail(TR_ERR_BAD_PARAM, "no place for the context");
  *out = nullptr;
  if (int rc = check_params(p)) return rc;
  return capi::create_ctx(p, device, out);
}

void tr_ctx_destroy(tr_ctx *c) { capi::destroy_ctx(c); }

int tr_set_params(tr_ctx *c, const tr_params *p) {
  if (!c) return fail(TR_ERR_STATE, "no context");
  if (int rc = check_params(p)) return rc;
  c->P = *p;
  return TR_OK;
}

int tr_get_stats(const tr_ctx *c, tr_stats *out) {
  if (!c || !out) return fail(TR_ERR_STATE, "no context");
  *out = c->S;
  return TR_OK;
}

int tr_trim_reads(tr_ctx *c, uint32_t num_reads, const uint32_t *lengths, const uint8_t *rules,
                  const ovl_record *records, uint64_t n, int records_on_device, uint32_t id_min,
                  uint32_t id_max, tr_result *out) {
  if (!c) return fail(TR_ERR_STATE, "no context");
  if (!out || !out->bgn || !out->end || !out->status || !out->flags || !out->n_skipped || !out->n_used)
    return fail(TR_ERR_BAD_PARAM, "a result array is missing");
  if (num_reads && (!lengths || !rules)) return fail(TR_ERR_BAD_PARAM, "no lengths or no rules");
  if (n && !records) return fail(TR_ERR_BAD_PARAM, "no records");
  if (num_reads == UINT32_MAX) return fail(TR_ERR_BAD_PARAM, "too many reads");
  HIP_TRY(hipSetDevice(c->device));
  tr_stats &S = c->S;
  S = tr_stats{};
  if (id_min < 1) id_min = 1;                                       // trimReads.C:257-260
  if (id_max > num_reads) id_max = num_reads;
  S.id_min = id_min;
  S.id_max = id_max;
  for (uint32_t i = 0; i < num_reads; i++) {
    out->bgn[i] = 0;
    out->end[i] = lengths[i];
    out->status[i] = TR_NOT_IN_RANGE;
    out->flags[i] = 0;
    out->n_skipped[i] = out->n_used[i] = 0;
    if (lengths[i] > AS_MAX_READLEN)
      return fail(TR_ERR_BAD_INPUT, "read %u is %u bases, beyond AS_MAX_READLEN", i + 1, lengths[i]);
  }
  for (uint32_t r = id_min; r <= id_max && r >= 1; r++)
    if (rules[r - 1] != 1 && rules[r - 1] != 2)
      return fail(TR_ERR_BAD_INPUT, "read %u has trimming rule %u: trimReads asserts there", r,
                  rules[r - 1]);
  const hipStream_t st = c->stream;
  const DevParams P{encode_evalue(c->P.erate), c->P.min_evidence_overlap, c->P.min_evidence_coverage};

  std::vector<uint64_t> off(num_reads + 2, 0);
  DevBuf<ovl_record> d_own;
  DevBuf<uint32_t> d_len, d_order;
  DevBuf<uint8_t> d_rules, d_flags;
  DevBuf<uint2> d_span;
  DevBuf<uint64_t> d_off;
  DevBuf<int> d_err;
  DevBuf<unsigned long long> d_where;
  DevBuf<uint32_t> d_bgn, d_end, d_nskip, d_nused;
  Event e0, e1, e2, e3, e4;
  HIP_TRY(e0.create()); HIP_TRY(e1.create()); HIP_TRY(e2.create()); HIP_TRY(e3.create()); HIP_TRY(e4.create());
  if (n > 0 && id_min <= id_max) {
    const ovl_record *d_rec = records;
    if (!records_on_device) {
      HIP_TRY(d_own.alloc(n));
      HIP_TRY(hipMemcpyAsync(d_own.p, records, n * sizeof(ovl_record), hipMemcpyHostToDevice, st));
      d_rec = d_own.p;
    }
    HIP_TRY(d_len.alloc(num_reads));
    HIP_TRY(d_rules.alloc(num_reads));
    HIP_TRY(d_span.alloc(n));
    HIP_TRY(d_off.alloc(num_reads + 2));
    HIP_TRY(d_err.alloc(1));
    HIP_TRY(d_where.alloc(1));
    HIP_TRY(hipMemcpyAsync(d_len.p, lengths, num_reads * 4ull, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_rules.p, rules, num_reads, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_err.p, 0, sizeof(int), st));
    HIP_TRY(hipMemsetAsync(d_where.p, 0xFF, sizeof(unsigned long long), st));
    if ((n + 255) / 256 > 0x7FFFFFFFull) return fail(TR_ERR_UNSUPPORTED, "%llu overlaps in one call", (unsigned long long)n);
    HIP_TRY(hipEventRecord(e0, st));
    k_tr_segment<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(d_rec, n, d_len.p, num_reads, P.ev_max,
                                                              d_span.p, d_err.p, d_where.p);
    k_tr_offsets<<<(num_reads + 2 + 255) / 256, 256, 0, st>>>(d_rec, n, num_reads, d_off.p);
    HIP_TRY(hipEventRecord(e1, st));
    HIP_TRY(hipGetLastError());
    int err = 0;
    unsigned long long where = 0;
    HIP_TRY(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&where, d_where.p, sizeof where, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(off.data(), d_off.p, (num_reads + 2) * 8ull, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (err & E_BAD_ID)
      return fail(TR_ERR_BAD_INPUT, "an overlap (the first is record %llu) names a read outside 1..%u", where, num_reads);
    if (err & E_UNSORTED)
      return fail(TR_ERR_BAD_INPUT, "the overlaps are not sorted by a_iid (record %llu)", where);
    if (err & E_BAD_SPAN)
      return fail(TR_ERR_BAD_INPUT, "an overlap (the first is record %llu) with a_bgn >= a_end", where);
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    S.ms_segment = ms;

    // the reads with overlaps, most overlaps first: a counting sort below the wave's capacity
    std::vector<uint32_t> head(TR_WAVE_CAP + 2, 0), wave_order, large;
    for (uint32_t r = id_min; r <= id_max; r++) {
      const uint64_t cnt = off[r + 1] - off[r];
      S.n_overlaps += cnt;
      if (cnt > 0xFFFFFFFFull / 4) return fail(TR_ERR_UNSUPPORTED, "read %u has %llu overlaps", r, (unsigned long long)cnt);
      if (cnt > TR_WAVE_CAP) large.push_back(r);
      else if (cnt > 0) head[TR_WAVE_CAP - cnt + 1]++;
    }
    for (uint32_t k = 1; k < head.size(); k++) head[k] += head[k - 1];
    wave_order.resize(head[TR_WAVE_CAP]);
    for (uint32_t r = id_min; r <= id_max; r++) {
      const uint64_t cnt = off[r + 1] - off[r];
      if (cnt > 0 && cnt <= TR_WAVE_CAP) wave_order[head[TR_WAVE_CAP - cnt]++] = r;
    }
    std::stable_sort(large.begin(), large.end(), [&](uint32_t a, uint32_t b) {
      return off[a + 1] - off[a] > off[b + 1] - off[b];
    });
    S.n_wave_reads = wave_order.size();
    S.n_large_reads = large.size();

    HIP_TRY(d_bgn.alloc(num_reads + 1)); HIP_TRY(d_end.alloc(num_reads + 1));
    HIP_TRY(d_nskip.alloc(num_reads + 1)); HIP_TRY(d_nused.alloc(num_reads + 1));
    HIP_TRY(d_flags.alloc(num_reads + 1));
    const ReadOut RO{d_bgn.p, d_end.p, d_nskip.p, d_nused.p, d_flags.p};
    HIP_TRY(d_order.alloc(wave_order.size() + large.size()));
    if (!wave_order.empty())
      HIP_TRY(hipMemcpyAsync(d_order.p, wave_order.data(), wave_order.size() * 4, hipMemcpyHostToDevice, st));
    if (!large.empty())
      HIP_TRY(hipMemcpyAsync(d_order.p + wave_order.size(), large.data(), large.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(e2, st));
    if (!wave_order.empty())
      k_tr_wave<<<(unsigned)wave_order.size(), 64, 0, st>>>(d_order.p, d_off.p, d_span.p, d_len.p,
                                                            d_rules.p, P, RO);
    HIP_TRY(hipEventRecord(e3, st));
    HIP_TRY(hipGetLastError());

    DevBuf<uint64_t> d_base, d_pbase, d_iv, d_iv2, d_stack;
    DevBuf<uint32_t> d_ev, d_ev2, d_idlo, d_idhi, d_t5, d_t3;
    DevBuf<uint64_t> d_segb, d_sege;
    DevBuf<uint8_t> d_tmp;
    if (!large.empty()) {
      // every list of a large read is bounded by its overlap count: 2 per overlap for the end
      // points and the depth pieces, 1 for the rest, the next power of two for the trim points
      const size_t nl = large.size();
      std::vector<uint64_t> base(nl), pbase(nl), segb(2 * nl), sege(2 * nl);
      uint64_t tot = 0, ptot = 0;
      for (size_t k = 0; k < nl; k++) {
        const uint64_t cnt = off[large[k] + 1] - off[large[k]];
        base[k] = tot;
        pbase[k] = ptot;
        segb[k] = 2 * tot; sege[k] = 2 * (tot + cnt);              // ev
        segb[nl + k] = tot; sege[nl + k] = tot + cnt;              // iv
        tot += cnt;
        uint64_t p = 1;
        while (p < cnt) p <<= 1;
        ptot += p;
      }
      if (2 * tot > 0x7FFFFFFFull || nl > 65535)         // hipcub's item count; the key kernel's grid
        return fail(TR_ERR_UNSUPPORTED, "%zu reads with more than %u overlaps each, %llu in all", nl,
                    TR_WAVE_CAP, (unsigned long long)tot);
      HIP_TRY(d_base.alloc(nl)); HIP_TRY(d_pbase.alloc(nl));
      HIP_TRY(d_segb.alloc(2 * nl)); HIP_TRY(d_sege.alloc(2 * nl));
      HIP_TRY(d_ev.alloc(2 * tot)); HIP_TRY(d_ev2.alloc(2 * tot));
      HIP_TRY(d_iv.alloc(tot)); HIP_TRY(d_iv2.alloc(tot));
      HIP_TRY(d_idlo.alloc(tot)); HIP_TRY(d_idhi.alloc(tot));
      HIP_TRY(d_stack.alloc(2 * tot));
      HIP_TRY(d_t5.alloc(ptot)); HIP_TRY(d_t3.alloc(ptot));
      HIP_TRY(hipMemcpyAsync(d_base.p, base.data(), nl * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d_pbase.p, pbase.data(), nl * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d_segb.p, segb.data(), 2 * nl * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(d_sege.p, sege.data(), 2 * nl * 8, hipMemcpyHostToDevice, st));
      const uint32_t *lorder = d_order.p + wave_order.size();
      const uint64_t biggest = off[large[0] + 1] - off[large[0]];
      k_tr_large_keys<<<dim3((unsigned)std::min<uint64_t>((biggest + 255) / 256, 1024), (unsigned)nl), 256, 0, st>>>(
          lorder, d_off.p, d_base.p, d_span.p, d_ev.p, d_iv.p);
      HIP_TRY(hipGetLastError());
      size_t tb1 = 0, tb2 = 0;
      HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, tb1, d_ev.p, d_ev2.p, (int)(2 * tot), (int)nl,
                                                         d_segb.p, d_sege.p, 0, 32, st));
      HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, tb2, d_iv.p, d_iv2.p, (int)tot, (int)nl,
                                                         d_segb.p + nl, d_sege.p + nl, 0, 64, st));
      HIP_TRY(d_tmp.alloc(std::max(tb1, tb2)));
      tb1 = tb2 = d_tmp.bytes;
      HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(d_tmp.p, tb1, d_ev.p, d_ev2.p, (int)(2 * tot), (int)nl,
                                                         d_segb.p, d_sege.p, 0, 32, st));
      HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(d_tmp.p, tb2, d_iv.p, d_iv2.p, (int)tot, (int)nl,
                                                         d_segb.p + nl, d_sege.p + nl, 0, 64, st));
      k_tr_large<<<(unsigned)nl, 64, 0, st>>>(lorder, d_off.p, d_base.p, d_pbase.p, d_span.p, d_len.p,
                                              d_rules.p, d_ev2.p, d_iv2.p, d_idlo.p, d_idhi.p,
                                              d_stack.p, d_t5.p, d_t3.p, P, RO);
      HIP_TRY(hipGetLastError());
      S.scratch_bytes = d_ev.bytes + d_ev2.bytes + d_iv.bytes + d_iv2.bytes + d_idlo.bytes +
                        d_idhi.bytes + d_stack.bytes + d_t5.bytes + d_t3.bytes + d_tmp.bytes;
    }
    HIP_TRY(hipEventRecord(e4, st));

    std::vector<uint32_t> h_bgn(num_reads + 1), h_end(num_reads + 1), h_nskip(num_reads + 1), h_nused(num_reads + 1);
    std::vector<uint8_t> h_flags(num_reads + 1);
    HIP_TRY(hipMemcpyAsync(h_bgn.data(), d_bgn.p, (num_reads + 1) * 4ull, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_end.data(), d_end.p, (num_reads + 1) * 4ull, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_nskip.data(), d_nskip.p, (num_reads + 1) * 4ull, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_nused.data(), d_nused.p, (num_reads + 1) * 4ull, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_flags.data(), d_flags.p, num_reads + 1ull, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&ms, e2, e3));
    S.ms_wave = ms;
    HIP_TRY(hipEventElapsedTime(&ms, e3, e4));
    S.ms_large = ms;
    for (uint32_t r = id_min; r <= id_max; r++) {
      if (off[r + 1] == off[r]) continue;
      const uint32_t i = r - 1;
      const bool ok = h_flags[r] & F_OK;
      out->bgn[i] = h_bgn[r];
      out->end[i] = h_end[r];
      out->n_skipped[i] = h_nskip[r];
      out->n_used[i] = h_nused[r];
      out->flags[i] = (ok ? 0 : TR_FLAG_NO_HQ) | ((h_flags[r] & F_RESET) ? TR_FLAG_RESET : 0);
      S.n_literal += (h_flags[r] & F_LITERAL) != 0;
    }
  }

  // the classification of trimReads.C:375-436
  auto add = [](tr_count &t, uint64_t bases) { t.reads++; t.bases += bases; };
  for (uint32_t r = id_min; r <= id_max; r++) {
    const uint32_t i = r - 1, len = lengths[i], fb = out->bgn[i], fe = out->end[i];
    add(S.reads_in, len);
    if (off[r + 1] == off[r]) {
      add(S.no_ovl_out, len);
      out->status[i] = TR_NOV;
    } else if ((out->flags[i] & TR_FLAG_NO_HQ) || fe - fb < c->P.min_read_length) {
      add(S.deleted_out, len);
      out->status[i] = TR_DEL;
    } else if (fb == 0 && fe == len) {
      add(S.no_change_out, len);
      out->status[i] = TR_NOC;
    } else {
      add(S.reads_out, fe - fb);
      out->status[i] = TR_MOD;
      if (fb > 0) add(S.trim5, fb);
      if (len - fe > 0) add(S.trim3, len - fe);
    }
  }
  return TR_OK;
}

}  // extern "C"
