// sr.hip -- libcanu_sr.so: canu's splitReads on gfx950 (include/canu_sr.h).
//
//   k_sr_reads    one thread per read: where the read's overlaps start (a binary search; the
//                 records are sorted by a_iid), its input clear range (0 .. length without one),
//                 checked, and whether splitReads processes it
//   k_sr_adjust   one thread per overlap record: checks it (IDs, order, spans), gathers both
//                 reads' lengths and clear ranges, does adjustNormal / adjustFlipped in IEEE
//                 double and the two 15-base snaps -> four coordinates, a valid and a flipped bit
//   k_sr_pairs    one thread per record: counts the valid records of its (a, b) pair among its
//                 neighbours (the input is grouped already), writes the record's fate, and for
//                 the first of two in opposite orientations the pair's bad interval and whether
//                 it goes to BAD, to BADall, and whether it is a large palindrome
//   k_sr_wave     one wave per read, reads in descending order of overlap count, lists in LDS:
//                 the bad intervals are compacted by ballot, sorted by (lo, hi) with a bitonic
//                 network and merged with counts; per merged BAD interval allHits is a wave sum
//                 over the merged BADall list and numSpan a wave sum over the read's records;
//                 the inversion and the first strictly largest good piece are a wave maximum
//                 with the lowest index winning ties
//   k_sr_large    the same code for a read with more than SR_WAVE_CAP overlaps, its lists in
//                 device memory sized from the read's overlap count
//
// intervalList::merge(0) over a sorted list fuses an interval into its group when its lo is not
// beyond the largest hi so far (touching fuses), sums the counts, and copies the next interval
// over a (0, 0) one, count and all: the leading (0, 0) intervals fall away unless there is nothing
// else.  A read has few bad intervals (mostly none), so one lane walks the sorted list.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/canu_sr.h"
#include "capi_common.h"

#define SR_WAVE_CAP 1024u     // overlaps of a read k_sr_wave takes (a power of two)
#define SR_LIST_CAP (SR_WAVE_CAP / 2)   // a bad interval needs two overlaps
#define AS_MAX_READLEN ((1u << 21) - 1)

namespace {

using capi::fail;

CAPI_SAME_CODES(SR);

enum { E_BAD_ID = 1, E_UNSORTED = 2, E_BAD_ASPAN = 4, E_BAD_BSPAN = 8, E_BAD_CLEAR = 16 };
enum { A_VALID = 1, A_FLIPPED = 2 };                     // k_sr_adjust's flags of a record
enum { P_BAD = 1, P_ALL = 2, P_PALINDROME = 4 };         // k_sr_pairs' flags of a record
enum { R_PROCESSED = 1 };

__device__ __forceinline__ void note(int *err, unsigned long long *where, int e, unsigned long long i) {
  atomicOr(err, e);
  atomicMin(where, i);
}

// ------------------------------------------------------------------------------ the reads

// off[r], r = 0 .. num_reads + 1: the first record whose a_iid is >= r.  For read r = 1 ..
// num_reads: cb / ce [r - 1] its input clear range, proc[r - 1] whether its overlaps are looked at.
__global__ __launch_bounds__(256) void k_sr_reads(const ovl_record *__restrict__ rec, uint64_t n,
                                                  uint32_t num_reads,
                                                  const uint32_t *__restrict__ lengths,
                                                  const uint8_t *__restrict__ lib,
                                                  const uint32_t *__restrict__ in_cb,
                                                  const uint32_t *__restrict__ in_ce, uint32_t id_min,
                                                  uint32_t id_max, uint64_t *__restrict__ off,
                                                  uint32_t *__restrict__ cb, uint32_t *__restrict__ ce,
                                                  uint8_t *__restrict__ proc, int *__restrict__ err,
                                                  unsigned long long *__restrict__ where) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r > num_reads + 1) return;
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (rec[mid].a_iid < r) lo = mid + 1; else hi = mid;
  }
  off[r] = lo;
  if (r < 1 || r > num_reads) return;
  const uint32_t i = r - 1, len = lengths[i];
  const uint32_t b = in_cb ? in_cb[i] : 0, e = in_ce ? in_ce[i] : len;
  const bool deleted = b == UINT32_MAX && e == UINT32_MAX;
  if (!deleted && (b > e || e > len)) note(err, where, E_BAD_CLEAR, r);
  cb[i] = b;
  ce[i] = e;
  proc[i] = (r >= id_min && r <= id_max && !deleted && (lib[i] & SR_LIB_ELIGIBLE)) ? R_PROCESSED : 0;
}

// ------------------------------------------------------------------------------ the records

__global__ __launch_bounds__(256) void k_sr_adjust(const ovl_record *__restrict__ rec, uint64_t n,
                                                   const uint32_t *__restrict__ lengths,
                                                   uint32_t num_reads, const uint32_t *__restrict__ cb,
                                                   const uint32_t *__restrict__ ce,
                                                   const uint8_t *__restrict__ proc,
                                                   uint4 *__restrict__ adj, uint8_t *__restrict__ aflag,
                                                   int *__restrict__ err,
                                                   unsigned long long *__restrict__ where) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t a = rec[i].a_iid, b = rec[i].b_iid;
  int e = 0;
  if (a == 0 || a > num_reads || b == 0 || b > num_reads) e |= E_BAD_ID;
  if (i > 0) {
    const uint32_t pa = rec[i - 1].a_iid, pb = rec[i - 1].b_iid;
    if (pa > a || (pa == a && pb > b)) e |= E_UNSORTED;
  }
  uint32_t abgn = 0, aend = 0, bbgn = 0, bend = 0;
  uint8_t flag = 0;
  if (!(e & E_BAD_ID)) {
    const uint64_t w0 = rec[i].dat[0], w1 = rec[i].dat[1];
    const uint32_t la = lengths[a - 1], lb = lengths[b - 1];
    const uint32_t ah5 = (uint32_t)(w0 & AS_MAX_READLEN), ah3 = (uint32_t)((w0 >> 21) & AS_MAX_READLEN);
    const uint32_t bh5 = (uint32_t)(w1 & AS_MAX_READLEN), bh3 = (uint32_t)((w1 >> 21) & AS_MAX_READLEN);
    const bool flipped = (w0 >> 54) & 1;
    if ((uint64_t)ah5 + ah3 >= la) e |= E_BAD_ASPAN;     // a_bgn >= a_end, or a_end wraps
    if ((uint64_t)bh5 + bh3 >= lb) e |= E_BAD_BSPAN;
    const uint32_t bcb0 = cb[b - 1], bce0 = ce[b - 1];
    const bool b_deleted = bcb0 == UINT32_MAX && bce0 == UINT32_MAX;
    if (!e && (proc[a - 1] & R_PROCESSED) && !b_deleted) {
      if (flipped) flag |= A_FLIPPED;
      // the B read on the strand of the overlap (adjustFlipped.C:48-58)
      abgn = ah5; aend = la - ah3; bbgn = bh5; bend = lb - bh3;
      const uint32_t acb = cb[a - 1], ace = ce[a - 1];
      const uint32_t bcb = flipped ? lb - bce0 : bcb0, bce = flipped ? lb - bcb0 : bce0;
      if (!(ace <= abgn || aend <= acb || bce <= bbgn || bend <= bcb)) {
        const uint32_t alen = aend - abgn, blen = bend - bbgn;
        const double afb = (double)(acb < abgn ? 0u : acb - abgn) / alen;
        const double bfb = (double)(bcb < bbgn ? 0u : bcb - bbgn) / blen;
        const double afe = (double)(ace > aend ? 0u : aend - ace) / alen;
        const double bfe = (double)(bce > bend ? 0u : bend - bce) / blen;
        const double mb = afb < bfb ? bfb : afb, me = afe < bfe ? bfe : afe;
        abgn += (uint32_t)round(mb * alen);
        bbgn += (uint32_t)round(mb * blen);
        aend -= (uint32_t)round(me * alen);
        bend -= (uint32_t)round(me * blen);
        if (bbgn - bcb < 15) {                           // splitReads-workUnit.C:95-115
          const uint32_t limit = abgn - acb;
          uint32_t adjust = bbgn - bcb;
          if (adjust > limit) adjust = limit;
          abgn -= adjust;
          bbgn -= adjust;
        }
        if (bce - bend < 15) {                           // :118-130
          const uint32_t limit = ace - aend;
          uint32_t adjust = bce - bend;
          if (adjust > limit) adjust = limit;
          aend += adjust;
          bend += adjust;
        }
        flag |= A_VALID;
      }
    }
  }
  adj[i] = make_uint4(abgn, aend, bbgn, bend);
  aflag[i] = flag;
  if (e) note(err, where, e, i);
}

__device__ __forceinline__ uint32_t isect(uint32_t b1, uint32_t e1, uint32_t b2, uint32_t e2) {
  const uint32_t lo = max(b1, b2), hi = min(e1, e2);
  return hi > lo ? hi - lo : 0;
}

// detectSubReads' pair loop (splitReads-subReads.C:95-257), from the side of every record.
__global__ __launch_bounds__(256) void k_sr_pairs(const ovl_record *__restrict__ rec, uint64_t n,
                                                  uint32_t num_reads, const uint8_t *__restrict__ lib,
                                                  const uint8_t *__restrict__ proc,
                                                  const uint4 *__restrict__ adj,
                                                  const uint8_t *__restrict__ aflag,
                                                  uint2 *__restrict__ pair, uint8_t *__restrict__ pflag,
                                                  uint8_t *__restrict__ fate) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t a = rec[i].a_iid, b = rec[i].b_iid;
  uint8_t f = SR_FATE_NOT_IN_RANGE, pf = 0;
  uint2 pr = make_uint2(0, 0);
  if (a >= 1 && a <= num_reads && (proc[a - 1] & R_PROCESSED)) {
    const uint8_t af = aflag[i];
    f = (af & A_VALID) ? SR_FATE_KEPT : SR_FATE_DROPPED;
    if ((af & A_VALID) && (lib[a - 1] & SR_LIB_SUBREADS)) {
      // the valid records of this pair before and after this one, counted up to two
      uint32_t before = 0, after = 0;
      uint64_t second = 0;
      for (uint64_t j = i; j > 0 && before < 2;) {
        j--;
        if (rec[j].a_iid != a || rec[j].b_iid != b) break;
        if (aflag[j] & A_VALID) before++;
      }
      for (uint64_t j = i + 1; j < n && after < 2; j++) {
        if (rec[j].a_iid != a || rec[j].b_iid != b) break;
        if (aflag[j] & A_VALID) {
          if (after == 0) second = j;
          after++;
        }
      }
      if (before + after > 1) {
        f = SR_FATE_MANY;
      } else if (before == 0 && after == 1) {
        const uint8_t sf = aflag[second];
        if (((af ^ sf) & A_FLIPPED) == 0) {
          f = SR_FATE_SAME_ORIENT;
        } else {
          const uint4 o = adj[i], p = adj[second];
          const uint32_t a_ov = isect(o.x, o.y, p.x, p.y), b_ov = isect(o.z, o.w, p.z, p.w);
          if (a_ov != 0 || b_ov != 0) {
            // b is within 1 .. num_reads: the record is valid
            if (a_ov > 1000 && b_ov > 1000 && (lib[b - 1] & SR_LIB_SUBREADS)) pf |= P_PALINDROME;
            if (!(a_ov > 250 || b_ov < 250)) {
              uint32_t lo = o.x < p.x ? o.y : p.y, hi = o.x < p.x ? p.x : o.x;
              if (lo > hi) { const uint32_t t = lo; lo = hi; hi = t; }
              if (hi - lo <= 500) pf |= P_BAD;
              if (hi - lo <= 2000) pf |= P_ALL;
              pr = make_uint2(lo, hi);
            }
          }
        }
      }
    }
  }
  pair[i] = pr;
  pflag[i] = pf;
  fate[i] = f;
}

// ------------------------------------------------------------------------------ wave helpers

__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1; }

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t u = __shfl_xor(v, o);
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
__device__ void bitonic_sort(uint64_t *a, uint32_t m, int lane) {
  for (uint32_t k = 2; k <= m; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = lane; t < (m >> 1); t += 64) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint64_t x = a[i], y = a[l];
        if ((x > y) == ((i & k) == 0)) {
          a[i] = y;
          a[l] = x;
        }
      }
      __syncthreads();
    }
}

// intervalList::merge(0) over n sorted (lo << 32 | hi) keys, in place, by one lane -> the merged
// intervals and their counts.
__device__ uint32_t merge_counts(uint64_t *iv, uint32_t *cnt, uint32_t n) {
  uint32_t nz = 0;
  while (nz < n && iv[nz] == 0) nz++;
  if (nz == n) {                                         // nothing but (0, 0): one of them stays
    cnt[0] = 1;
    return n ? 1 : 0;
  }
  uint32_t m = 0, lo = 0, hi = 0, c = 0;
  for (uint32_t i = nz; i < n; i++) {
    const uint64_t v = iv[i];
    const uint32_t l = (uint32_t)(v >> 32), h = (uint32_t)v;
    if (i == nz || hi < l) {
      if (i != nz) { iv[m] = ((uint64_t)lo << 32) | hi; cnt[m] = c; m++; }
      lo = l; hi = h; c = 1;
    } else {
      hi = max(hi, h);
      c++;
    }
  }
  iv[m] = ((uint64_t)lo << 32) | hi;
  cnt[m] = c;
  return m + 1;
}

// The lists of one read, each with room for the next power of two of half the read's records.
// k_sr_wave points them into LDS, k_sr_large into device memory.
struct Lists {
  uint64_t *bad, *all;      // (lo << 32 | hi) keys, then the merged intervals
  uint32_t *cbad, *call;    // the merged intervals' counts
};

struct ReadOut {            // indexed by the read ID
  uint32_t *bgn, *end, *n_adj, *n_reg;
};

// One read by one wave.  adj, aflag, pair, pflag: what the record kernels left for the read's nall
// records; reg: room for its confirmed regions.
__device__ void split_one(const Lists &L, const uint4 *adj, const uint8_t *aflag, const uint2 *pair,
                          const uint8_t *pflag, uint32_t nall, uint32_t read, bool subreads,
                          uint32_t clr_bgn, uint32_t clr_end, uint2 *reg, ReadOut out, int lane) {
  uint32_t n_adj = 0, nb = 0, na = 0;
  bool palindrome = false;
  for (uint32_t c = 0; c < nall; c += 64) {
    const uint32_t i = c + lane;
    const uint8_t af = i < nall ? aflag[i] : 0, pf = i < nall ? pflag[i] : 0;
    n_adj += __popcll(__ballot(af & A_VALID));
    const bool isb = pf & P_BAD, isa = pf & P_ALL;
    const uint64_t mb = __ballot(isb), ma = __ballot(isa);
    if (isa) {                                           // BAD is within BADall
      const uint2 p = pair[i];
      const uint64_t key = ((uint64_t)p.x << 32) | p.y;
      if (isb) L.bad[nb + __popcll(mb & lanes_below(lane))] = key;
      L.all[na + __popcll(ma & lanes_below(lane))] = key;
    }
    nb += __popcll(mb);
    na += __popcll(ma);
    palindrome |= __ballot(pf & P_PALINDROME) != 0;
  }
  uint32_t n_reg = 0, fbgn = clr_bgn, fend = clr_end;
  if (subreads && nb > 0) {
    const uint32_t pb = pow2_at_least(nb), pa = pow2_at_least(na);
    for (uint32_t i = nb + lane; i < pb; i += 64) L.bad[i] = ~0ull;
    for (uint32_t i = na + lane; i < pa; i += 64) L.all[i] = ~0ull;
    __syncthreads();
    bitonic_sort(L.bad, pb, lane);
    bitonic_sort(L.all, pa, lane);
    uint32_t mbad = 0, mall = 0;
    if (lane == 0) {
      mbad = merge_counts(L.bad, L.cbad, nb);
      mall = merge_counts(L.all, L.call, na);
    }
    mbad = __shfl(mbad, 0);
    mall = __shfl(mall, 0);
    __syncthreads();
    for (uint32_t bb = 0; bb < mbad; bb++) {             // splitReads-subReads.C:268-307
      const uint64_t v = L.bad[bb];
      const uint32_t lo = (uint32_t)(v >> 32), hi = (uint32_t)v;
      uint32_t hits = 0, span = 0;
      for (uint32_t k = lane; k < mall; k += 64) {
        const uint64_t w = L.all[k];
        if ((uint32_t)(w >> 32) <= lo && hi <= (uint32_t)w) hits += L.call[k];
      }
      for (uint32_t i = lane; i < nall; i += 64)
        if (aflag[i] & A_VALID) {
          const uint4 o = adj[i];
          if (o.x + 100 < lo && hi + 100 < o.y) span++;
        }
      hits = wave_sum(hits);
      span = wave_sum(span);
      if (span > 9) continue;
      if (L.cbad[bb] + hits / 4 + (palindrome ? 1u : 0u) < 3) continue;
      if (lane == 0) reg[n_reg] = make_uint2(lo, hi);
      n_reg++;
    }
    if (n_reg > 0) {                                     // splitReads-trimBad.C:54-73
      __syncthreads();
      // invert()'s merge() copies the next region over a leading (0, 0)
      const uint32_t first = (n_reg > 1 && reg[0].x == 0 && reg[0].y == 0) ? 1 : 0, m = n_reg - first;
      uint64_t best = 0;
      uint32_t best_lo = 0, best_hi = 0;
      for (uint32_t c = 0; c <= m; c += 64) {
        const uint32_t k = c + lane;
        uint32_t lo = 0, hi = 0;
        if (k <= m) {
          lo = k == 0 ? clr_bgn : reg[first + k - 1].y;
          hi = k == m ? clr_end : reg[first + k].x;
          if (!(lo < hi)) lo = hi = 0;                   // the end pieces exist only if not empty
        }
        const uint64_t key = wave_max(((uint64_t)(hi - lo) << 32) | (0xFFFFFFFFu - k));
        if ((key >> 32) > (best >> 32)) {                // the first strictly largest
          best = key;
          const int src = (int)((0xFFFFFFFFu - (uint32_t)key) & 63);
          best_lo = __shfl(lo, src);
          best_hi = __shfl(hi, src);
        }
      }
      fbgn = best_lo;
      fend = best_hi;
    }
  }
  if (lane == 0) {
    out.bgn[read] = fbgn;
    out.end[read] = fend;
    out.n_adj[read] = n_adj;
    out.n_reg[read] = n_reg;
  }
}

// order[block]: the read (1-based); off[r]: its first record; a read's regions go to
// reg[off[r] / 2 ..] (half its records bound them).
__global__ __launch_bounds__(64) void k_sr_wave(const uint32_t *__restrict__ order,
                                                const uint64_t *__restrict__ off,
                                                const uint4 *__restrict__ adj,
                                                const uint8_t *__restrict__ aflag,
                                                const uint2 *__restrict__ pair,
                                                const uint8_t *__restrict__ pflag,
                                                const uint8_t *__restrict__ lib,
                                                const uint32_t *__restrict__ cb,
                                                const uint32_t *__restrict__ ce, uint2 *__restrict__ reg,
                                                ReadOut out) {
  __shared__ uint64_t s_bad[SR_LIST_CAP], s_all[SR_LIST_CAP];
  __shared__ uint32_t s_cbad[SR_LIST_CAP], s_call[SR_LIST_CAP];
  const uint32_t read = order[blockIdx.x];
  const uint64_t first = off[read];
  const uint32_t nall = (uint32_t)(off[read + 1] - first);
  if (nall > SR_WAVE_CAP) return;                        // the host never sends one
  const Lists L{s_bad, s_all, s_cbad, s_call};
  split_one(L, adj + first, aflag + first, pair + first, pflag + first, nall, read,
            lib[read - 1] & SR_LIB_SUBREADS, cb[read - 1], ce[read - 1], reg + (first >> 1), out,
            (int)threadIdx.x);
}

// The lists of large read k lie at base[k] of each array.
__global__ __launch_bounds__(64) void k_sr_large(const uint32_t *__restrict__ order,
                                                 const uint64_t *__restrict__ off,
                                                 const uint64_t *__restrict__ base,
                                                 const uint4 *__restrict__ adj,
                                                 const uint8_t *__restrict__ aflag,
                                                 const uint2 *__restrict__ pair,
                                                 const uint8_t *__restrict__ pflag,
                                                 const uint8_t *__restrict__ lib,
                                                 const uint32_t *__restrict__ cb,
                                                 const uint32_t *__restrict__ ce, uint64_t *bad,
                                                 uint64_t *all, uint32_t *cbad, uint32_t *call,
                                                 uint2 *__restrict__ reg, ReadOut out) {
  const uint32_t read = order[blockIdx.x];
  const uint64_t first = off[read], b = base[blockIdx.x];
  const uint32_t nall = (uint32_t)(off[read + 1] - first);
  const Lists L{bad + b, all + b, cbad + b, call + b};
  split_one(L, adj + first, aflag + first, pair + first, pflag + first, nall, read,
            lib[read - 1] & SR_LIB_SUBREADS, cb[read - 1], ce[read - 1], reg + (first >> 1), out,
            (int)threadIdx.x);
}

int check_params(const sr_params *p) {
  if (!p) return fail(SR_ERR_BAD_PARAM, "no parameters");
  if (!(p->erate >= 0.0)) return fail(SR_ERR_BAD_PARAM, "erate %g is negative", p->erate);
  return SR_OK;
}

}  // namespace

struct sr_ctx : capi::Device {
  sr_params P{};
  sr_stats S{};
};

extern "C" {

void sr_params_init(sr_params *p) {
  p->erate = 0.015;
  p->min_read_length = 64;
}

const char *sr_last_error(void) { return capi::g_err.c_str(); }
int sr_abi_version(void) { return SR_ABI_VERSION; }
uint32_t sr_wave_capacity(void) { return SR_WAVE_CAP; }

int sr_ctx_create(const sr_params *p, int device, sr_ctx **out) {
  if (!out) return fail(SR_ERR_BAD_PARAM, "no place for the context");
  *out = nullptr;
  if (int rc = check_params(p)) return rc;
  return capi::create_ctx(p, device, out);
}

void sr_ctx_destroy(sr_ctx *c) { capi::destroy_ctx(c); }

int sr_set_params(sr_ctx *c, const sr_params *p) {
  if (!c) return fail(SR_ERR_STATE, "no context");
  if (int rc = check_params(p)) return rc;
  c->P = *p;
  return SR_OK;
}

int sr_get_stats(const sr_ctx *c, sr_stats *out) {
  if (!c || !out) return fail(SR_ERR_STATE, "no context");
  *out = c->S;
  return SR_OK;
}

int sr_split_reads(sr_ctx *c, uint32_t num_reads, const uint32_t *lengths, const uint8_t *lib_flags,
                   const uint32_t *clr_bgn, const uint32_t *clr_end, const ovl_record *records,
                   uint64_t n, int on_device, uint32_t id_min, uint32_t id_max, sr_result *out) {
  if (!c) return fail(SR_ERR_STATE, "no context");
  if (!out || !out->bgn || !out->end || !out->status || !out->n_adjusted || !out->n_bad_regions ||
      !out->region_off || (n && !out->fate))
    return fail(SR_ERR_BAD_PARAM, "a result array is missing");
  if (num_reads && (!lengths || !lib_flags)) return fail(SR_ERR_BAD_PARAM, "no lengths or no library flags");
  if (n && !records) return fail(SR_ERR_BAD_PARAM, "no records");
  if (num_reads == UINT32_MAX) return fail(SR_ERR_BAD_PARAM, "too many reads");
  if ((clr_bgn == nullptr) != (clr_end == nullptr))
    return fail(SR_ERR_BAD_PARAM, "one of the two clear range arrays is missing");
  const bool rec_dev = on_device & SR_RECORDS_ON_DEVICE, clr_dev = on_device & SR_CLEAR_ON_DEVICE;
  HIP_TRY(hipSetDevice(c->device));
  sr_stats &S = c->S;
  S = sr_stats{};
  if (id_min < 1) id_min = 1;                                       // splitReads.C:221-224
  if (id_max > num_reads) id_max = num_reads;
  S.id_min = id_min;
  S.id_max = id_max;
  for (uint32_t i = 0; i < num_reads; i++) {
    out->bgn[i] = 0;
    out->end[i] = lengths[i];
    out->status[i] = SR_NOT_IN_RANGE;
    out->n_adjusted[i] = out->n_bad_regions[i] = 0;
    out->region_off[i] = 0;
    if (lengths[i] > AS_MAX_READLEN)
      return fail(SR_ERR_BAD_INPUT, "read %u is %u bases, beyond AS_MAX_READLEN", i + 1, lengths[i]);
  }
  out->region_off[num_reads] = 0;
  if (num_reads == 0) {
    if (n) return fail(SR_ERR_BAD_INPUT, "overlaps and no reads");
    return SR_OK;
  }
  if ((n + 255) / 256 > 0x7FFFFFFFull) return fail(SR_ERR_UNSUPPORTED, "%llu overlaps in one call", (unsigned long long)n);
  const hipStream_t st = c->stream;

  std::vector<uint64_t> off(num_reads + 2, 0);
  std::vector<uint32_t> h_cb(num_reads), h_ce(num_reads);
  DevBuf<ovl_record> d_own;
  DevBuf<uint32_t> d_len, d_icb, d_ice, d_cb, d_ce, d_order;
  DevBuf<uint8_t> d_lib, d_proc, d_aflag, d_pflag, d_fate;
  DevBuf<uint4> d_adj;
  DevBuf<uint2> d_pair, d_reg;
  DevBuf<uint64_t> d_off;
  DevBuf<int> d_err;
  DevBuf<unsigned long long> d_where;
  Event e0, e1, e2, e3, e4;
  HIP_TRY(e0.create()); HIP_TRY(e1.create()); HIP_TRY(e2.create()); HIP_TRY(e3.create()); HIP_TRY(e4.create());

  const ovl_record *d_rec = records;
  if (!rec_dev && n) {
    HIP_TRY(d_own.alloc(n));
    HIP_TRY(hipMemcpyAsync(d_own.p, records, n * sizeof(ovl_record), hipMemcpyHostToDevice, st));
    d_rec = d_own.p;
  }
  const uint32_t *d_in_cb = clr_bgn, *d_in_ce = clr_end;
  if (clr_bgn && !clr_dev) {
    HIP_TRY(d_icb.alloc(num_reads)); HIP_TRY(d_ice.alloc(num_reads));
    HIP_TRY(hipMemcpyAsync(d_icb.p, clr_bgn, num_reads * 4ull, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_ice.p, clr_end, num_reads * 4ull, hipMemcpyHostToDevice, st));
    d_in_cb = d_icb.p;
    d_in_ce = d_ice.p;
  }
  HIP_TRY(d_len.alloc(num_reads)); HIP_TRY(d_lib.alloc(num_reads));
  HIP_TRY(d_cb.alloc(num_reads)); HIP_TRY(d_ce.alloc(num_reads)); HIP_TRY(d_proc.alloc(num_reads));
  HIP_TRY(d_off.alloc(num_reads + 2));
  HIP_TRY(d_adj.alloc(n)); HIP_TRY(d_aflag.alloc(n)); HIP_TRY(d_pair.alloc(n)); HIP_TRY(d_pflag.alloc(n));
  HIP_TRY(d_fate.alloc(n));
  HIP_TRY(d_err.alloc(1)); HIP_TRY(d_where.alloc(1));
  HIP_TRY(hipMemcpyAsync(d_len.p, lengths, num_reads * 4ull, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_lib.p, lib_flags, num_reads, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(d_err.p, 0, sizeof(int), st));
  HIP_TRY(hipMemsetAsync(d_where.p, 0xFF, sizeof(unsigned long long), st));
  HIP_TRY(hipEventRecord(e0, st));
  k_sr_reads<<<(num_reads + 2 + 255) / 256, 256, 0, st>>>(d_rec, n, num_reads, d_len.p, d_lib.p, d_in_cb,
                                                          d_in_ce, id_min, id_max, d_off.p, d_cb.p,
                                                          d_ce.p, d_proc.p, d_err.p, d_where.p);
  if (n) {
    const unsigned grid = (unsigned)((n + 255) / 256);
    k_sr_adjust<<<grid, 256, 0, st>>>(d_rec, n, d_len.p, num_reads, d_cb.p, d_ce.p, d_proc.p, d_adj.p,
                                      d_aflag.p, d_err.p, d_where.p);
    k_sr_pairs<<<grid, 256, 0, st>>>(d_rec, n, num_reads, d_lib.p, d_proc.p, d_adj.p, d_aflag.p,
                                     d_pair.p, d_pflag.p, d_fate.p);
  }
  HIP_TRY(hipEventRecord(e1, st));
  HIP_TRY(hipGetLastError());
  int err = 0;
  unsigned long long where = 0;
  HIP_TRY(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&where, d_where.p, sizeof where, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(off.data(), d_off.p, (num_reads + 2) * 8ull, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_cb.data(), d_cb.p, num_reads * 4ull, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_ce.data(), d_ce.p, num_reads * 4ull, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (err & E_BAD_CLEAR)
    return fail(SR_ERR_BAD_INPUT, "a clear range (the first is read %llu's) with bgn > end or end beyond the read", where);
  if (err & E_BAD_ID)
    return fail(SR_ERR_BAD_INPUT, "an overlap (the first is record %llu) names a read outside 1..%u", where, num_reads);
  if (err & E_UNSORTED)
    return fail(SR_ERR_BAD_INPUT, "the overlaps are not sorted by (a_iid, b_iid) (record %llu)", where);
  if (err & E_BAD_ASPAN)
    return fail(SR_ERR_BAD_INPUT, "an overlap (the first is record %llu) with a_bgn >= a_end", where);
  if (err & E_BAD_BSPAN)
    return fail(SR_ERR_BAD_INPUT, "an overlap (the first is record %llu) with b_bgn >= b_end", where);
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  S.ms_records = ms;
  for (uint32_t i = 0; i < num_reads; i++) {
    out->bgn[i] = h_cb[i];
    out->end[i] = h_ce[i];
  }

  auto deleted = [&](uint32_t i) { return h_cb[i] == UINT32_MAX && h_ce[i] == UINT32_MAX; };
  auto processed = [&](uint32_t r) {
    return r >= id_min && r <= id_max && !deleted(r - 1) && (lib_flags[r - 1] & SR_LIB_ELIGIBLE);
  };

  // the processed reads with overlaps, most overlaps first: a counting sort below the capacity
  std::vector<uint32_t> head(SR_WAVE_CAP + 2, 0), wave_order, large;
  for (uint32_t r = id_min; r <= id_max; r++) {
    if (!processed(r)) continue;
    const uint64_t cnt = off[r + 1] - off[r];
    S.n_overlaps += cnt;
    if (cnt > 0x7FFFFFFFull) return fail(SR_ERR_UNSUPPORTED, "read %u has %llu overlaps", r, (unsigned long long)cnt);
    if (cnt > SR_WAVE_CAP) large.push_back(r);
    else if (cnt > 0) head[SR_WAVE_CAP - cnt + 1]++;
  }
  for (uint32_t k = 1; k < head.size(); k++) head[k] += head[k - 1];
  wave_order.resize(head[SR_WAVE_CAP]);
  for (uint32_t r = id_min; r <= id_max; r++) {
    if (!processed(r)) continue;
    const uint64_t cnt = off[r + 1] - off[r];
    if (cnt > 0 && cnt <= SR_WAVE_CAP) wave_order[head[SR_WAVE_CAP - cnt]++] = r;
  }
  std::stable_sort(large.begin(), large.end(), [&](uint32_t a, uint32_t b) {
    return off[a + 1] - off[a] > off[b + 1] - off[b];
  });
  S.n_wave_reads = wave_order.size();
  S.n_large_reads = large.size();

  std::vector<uint32_t> h_bgn(num_reads + 1), h_end(num_reads + 1), h_nadj(num_reads + 1, 0), h_nreg(num_reads + 1, 0);
  std::vector<uint2> h_reg;
  if (!wave_order.empty() || !large.empty()) {
    DevBuf<uint32_t> d_bgn, d_end, d_nadj, d_nreg;
    HIP_TRY(d_bgn.alloc(num_reads + 1)); HIP_TRY(d_end.alloc(num_reads + 1));
    HIP_TRY(d_nadj.alloc(num_reads + 1)); HIP_TRY(d_nreg.alloc(num_reads + 1));
    HIP_TRY(hipMemsetAsync(d_nadj.p, 0, (num_reads + 1) * 4ull, st));
    HIP_TRY(hipMemsetAsync(d_nreg.p, 0, (num_reads + 1) * 4ull, st));
    HIP_TRY(d_reg.alloc(n / 2 + 1));
    const ReadOut RO{d_bgn.p, d_end.p, d_nadj.p, d_nreg.p};
    HIP_TRY(d_order.alloc(wave_order.size() + large.size()));
    if (!wave_order.empty())
      HIP_TRY(hipMemcpyAsync(d_order.p, wave_order.data(), wave_order.size() * 4, hipMemcpyHostToDevice, st));
    if (!large.empty())
      HIP_TRY(hipMemcpyAsync(d_order.p + wave_order.size(), large.data(), large.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipEventRecord(e2, st));
    if (!wave_order.empty())
      k_sr_wave<<<(unsigned)wave_order.size(), 64, 0, st>>>(d_order.p, d_off.p, d_adj.p, d_aflag.p, d_pair.p,
                                                            d_pflag.p, d_lib.p, d_cb.p, d_ce.p, d_reg.p, RO);
    HIP_TRY(hipEventRecord(e3, st));
    HIP_TRY(hipGetLastError());

    DevBuf<uint64_t> d_base, d_lbad, d_lall;
    DevBuf<uint32_t> d_lcbad, d_lcall;
    if (!large.empty()) {
      // a large read's lists: the next power of two of half its overlaps, each
      const size_t nl = large.size();
      std::vector<uint64_t> base(nl);
      uint64_t tot = 0;
      for (size_t k = 0; k < nl; k++) {
        const uint64_t cnt = off[large[k] + 1] - off[large[k]];
        base[k] = tot;
        uint64_t p = 1;
        while (p < cnt / 2) p <<= 1;
        tot += p;
      }
      HIP_TRY(d_base.alloc(nl));
      HIP_TRY(d_lbad.alloc(tot)); HIP_TRY(d_lall.alloc(tot));
      HIP_TRY(d_lcbad.alloc(tot)); HIP_TRY(d_lcall.alloc(tot));
      HIP_TRY(hipMemcpyAsync(d_base.p, base.data(), nl * 8, hipMemcpyHostToDevice, st));
      k_sr_large<<<(unsigned)nl, 64, 0, st>>>(d_order.p + wave_order.size(), d_off.p, d_base.p, d_adj.p,
                                              d_aflag.p, d_pair.p, d_pflag.p, d_lib.p, d_cb.p, d_ce.p,
                                              d_lbad.p, d_lall.p, d_lcbad.p, d_lcall.p, d_reg.p, RO);
      HIP_TRY(hipGetLastError());
      S.scratch_bytes = d_lbad.bytes + d_lall.bytes + d_lcbad.bytes + d_lcall.bytes;
    }
    HIP_TRY(hipEventRecord(e4, st));
    HIP_TRY(hipMemcpyAsync(h_bgn.data(), d_bgn.p, (num_reads + 1) * 4ull, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_end.data(), d_end.p, (num_reads + 1) * 4ull, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_nadj.data(), d_nadj.p, (num_reads + 1) * 4ull, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_nreg.data(), d_nreg.p, (num_reads + 1) * 4ull, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&ms, e2, e3));
    S.ms_wave = ms;
    HIP_TRY(hipEventElapsedTime(&ms, e3, e4));
    S.ms_large = ms;
    uint64_t nreg = 0;
    for (uint32_t r = 1; r <= num_reads; r++) nreg += h_nreg[r];
    if (nreg) {
      h_reg.resize(n / 2 + 1);
      HIP_TRY(hipMemcpy(h_reg.data(), d_reg.p, h_reg.size() * sizeof(uint2), hipMemcpyDeviceToHost));
    }
    S.n_regions = nreg;
    if (nreg > out->regions_cap || (nreg && !out->regions))
      return fail(SR_ERR_BAD_PARAM, "%llu bad regions and room for %llu", (unsigned long long)nreg,
                  (unsigned long long)out->regions_cap);
  }
  if (n) HIP_TRY(hipMemcpy(out->fate, d_fate.p, n, hipMemcpyDeviceToHost));

  // the classification of splitReads.C:236-372
  auto add = [](sr_count &t, uint64_t bases) { t.reads++; t.bases += bases; };
  uint64_t at = 0;
  for (uint32_t r = 1; r <= num_reads; r++) {
    const uint32_t i = r - 1, len = lengths[i];
    out->region_off[i] = at;
    if (r < id_min || r > id_max) continue;
    if (deleted(i)) { add(S.deleted_in, len); out->status[i] = SR_DELETED_IN; continue; }
    if (!(lib_flags[i] & SR_LIB_ELIGIBLE)) { add(S.no_trim_in, len); out->status[i] = SR_NO_TRIM; continue; }
    add(S.reads_in, len);
    if (off[r + 1] == off[r]) { add(S.no_overlaps, len); out->status[i] = SR_NO_OVERLAPS; continue; }
    out->n_adjusted[i] = h_nadj[r];
    if (h_nadj[r] == 0) { add(S.no_coverage, len); out->status[i] = SR_NO_COVERAGE; continue; }
    if (lib_flags[i] & SR_LIB_SUBREADS) add(S.proc_subread, len);
    const uint32_t nreg = h_nreg[r];
    out->n_bad_regions[i] = nreg;
    if (nreg == 0) { add(S.no_change, len); out->status[i] = SR_NO_CHANGE; continue; }
    for (uint32_t k = 0; k < nreg; k++) {
      const uint2 g = h_reg[(off[r] >> 1) + k];
      out->regions[at++] = sr_region{r, g.x, g.y};
      add(S.bases_bad_subread, g.y - g.x);
    }
    add(S.reads_bad_subread, nreg);
    const uint32_t fb = h_bgn[r], fe = h_end[r];
    if (fb < h_cb[i] || fe > h_ce[i])                                // splitReads.C:365-366
      return fail(SR_ERR_BAD_INPUT, "read %u: the clear range %u..%u grew to %u..%u, the reference asserts",
                  r, h_cb[i], h_ce[i], fb, fe);
    out->bgn[i] = fb;
    out->end[i] = fe;
    if (fe - fb < c->P.min_read_length) { add(S.deleted_out, len); out->status[i] = SR_DELETED_OUT; }
    else out->status[i] = SR_TRIMMED;
    if (fb > h_cb[i]) add(S.trimmed5, fb - h_cb[i]);
    if (h_ce[i] > fe) add(S.trimmed3, h_ce[i] - fe);
  }
  out->region_off[num_reads] = at;
  return SR_OK;
}

}  // extern "C"
