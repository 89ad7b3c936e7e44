// fs.hip -- libcanu_fs.so: canu's falconsense (src/correction/falconsense.C, falconConsensus*.C)
// on gfx950.  include/canu_fs.h says what is reproduced; this is how.
//
//   k_fs_locate     one wave per evidence read: edlib's EDLIB_MODE_HW result (edlib_wave.h's
//                   wave_locate), then the two rejection tests of alignReadsToTemplate.
//   k_fs_path       one wave per surviving evidence read: obtainAlignment's recursion
//                   (edlib_wave.h's wave_path, leaves under FS_LEAF_BYTES).  Its operations
//                   become tags 64 at a time with ballots, written with their place in
//                   (evidence, tag) order.  Alignment strings are never made.
//   hipcub          a segmented radix sort of each template's tags by (t_pos, delta, base,
//                   link); the sort is stable, so a run's first value is its first appearance.
//   k_fs_consensus  one wave per template: coverage, links (runs) and columns (runs of runs),
//                   the predecessor column of every link by binary search, the scan over the
//                   columns in (t_pos, delta, base) order, the walk back and the case rule.
//
// The scan in integers: a link scores link_count - coverage * 0.5 plus the score of its
// predecessor column, so every score is a multiple of 0.5 and twice the score is an exact
// integer.  The reference starts every maximum at DBL_MIN, the smallest positive double: it
// vanishes in a sum with any nonzero multiple of 0.5, 0 + DBL_MIN is not greater than DBL_MIN,
// so DBL_MIN is 0 here and "greater than DBL_MIN" is "greater than 0" (tests/test_fs_cpu.py
// compares the two forms).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/canu_fs.h"
#include "capi_common.h"
#include "edlib_launch.h"
#include "fs_fasta.h"

namespace {

using capi::fail;
using edw::LDS_WORDS;
using edw::OP_DELETE;
using edw::OP_INSERT;
using edw::OP_MATCH;
using edw::Span;
using edw::STACK_DEPTH;
using edw::uni;
using edw::WAVES_PER_BLOCK;

CAPI_SAME_CODES(FS);

// the base of a tag and of its predecessor: A C G T N - and '.', the first tag's predecessor
enum : int { CH_N = 4, CH_GAP = 5, CH_NONE = 6 };

// A tag as a sort key: t_pos at bit 43 (21 bits), delta at 27 (16), slot at 24 (3), prel at 19
// (2), p_delta at 3 (16), p_ch at 0 (3); bits 21..23 stay 0.
// slot is the base's column (N and '-' share 4); prel says where the predecessor sits: 0 none
// (p_t_pos -1), 1 at t_pos - 1, 2 at t_pos -- a predecessor is never anywhere else.
constexpr int KEY_COL_SHIFT = 21;                     // key >> 21 names the column
constexpr uint64_t KEY_NONE = ~0ull;

struct Ev {                  // one evidence read of one layout, template included
  uint64_t seq;              // its first base in the fwd or the rc array
  uint64_t tag_off;          // its tags
  uint32_t tag_cap;
  uint32_t rc;
  uint32_t tmpl;             // index of its template in the batch
  int32_t qlen;              // trimmed and cut to the template
  int32_t wb, we;            // the window of the template it is aligned to
  int32_t tol;
  int32_t pad;
};

struct Loc {
  int32_t dist, start, end, ok;
};

struct Tp {                  // one template of the batch
  uint64_t seq;              // in the fwd array
  uint64_t tag_off;          // its evidence reads' tags, contiguous
  uint64_t cov_off;
  uint64_t out_off;          // 2 * len bytes
  uint32_t tag_cap;
  int32_t len;
};

// ------------------------------------------------------------------ the location

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK)
void k_fs_locate(const uint8_t *__restrict__ fwd, const uint8_t *__restrict__ rcs,
                 const Ev *__restrict__ evs, const Tp *__restrict__ tps, const uint32_t n_ev,
                 Loc *__restrict__ loc, unsigned long long *__restrict__ cells,
                 uint32_t *__restrict__ scratch, const uint64_t scratch_words,
                 const double max_difference) {
  __shared__ uint32_t s_row[WAVES_PER_BLOCK][LDS_WORDS];
  const int wave = uni((int)(threadIdx.x >> 6));
  const uint64_t gw = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave;
  const uint32_t n_waves = gridDim.x * WAVES_PER_BLOCK;
  uint32_t *grow = scratch ? scratch + gw * scratch_words : nullptr;
  for (uint32_t e = (uint32_t)gw; e < n_ev; e += n_waves) {
    const Ev ev = evs[e];
    const int m = uni(ev.qlen), wb = uni(ev.wb), n = uni(ev.we) - wb;
    const uint8_t *qp = (uni((int)ev.rc) ? rcs : fwd) + ev.seq;
    const uint8_t *tp = fwd + tps[ev.tmpl].seq + wb;
    const edw::Located L = edw::wave_locate<5>(Span{qp, m}, Span{tp, n}, uni(ev.tol), true,
                                               s_row[wave], grow);
    Loc o{L.dist, L.start, L.end, 0};
    if (L.ok) {
      // alignDiff = editDistance / (double)(end - start): one short of the span, as there
      const double diff = (double)L.dist / (double)(L.end - L.start);
      o.ok = diff >= max_difference ? 0 : 1;
    }
    loc[e] = o;
    cells[e] = L.cells;
  }
}

// ------------------------------------------------------------------ the path and the tags

struct TagState {            // getAlignTags' running values, the same in every lane
  int qi;                    // query bases consumed
  int tj;                    // target bases consumed
  int jj;                    // insertions since the last target base
  int p_j, p_jj, p_ch;       // the last tag written
  uint32_t ntags;
};

__device__ __forceinline__ uint64_t tag_key(int j, int jj, int ch, int p_j, int p_jj, int p_ch) {
  const int slot = ch < 4 ? ch : 4;
  const int prel = p_j < 0 ? 0 : (p_j == j ? 2 : 1);
  return ((uint64_t)j << 43) | ((uint64_t)jj << 27) | ((uint64_t)slot << 24) |
         ((uint64_t)prel << 19) | ((uint64_t)p_jj << 3) | (uint64_t)p_ch;
}

// `count` operations in alignment order -- op_at(i) in every lane -- become tags.  tbgn is the
// template position of the alignment's first target base, tlen its number of target bases:
// insertions before the first and after the last target base are the gaps alignReadsToTemplate
// strips.
template <class OpAt>
__device__ void emit_tags(TagState &S, const int count, OpAt op_at, const uint8_t *qp,
                          const int qlen, const int tbgn, const int tlen, uint64_t *__restrict__ keys,
                          uint32_t *__restrict__ vals, const uint32_t val0, const uint32_t cap) {
  const int lane = threadIdx.x & 63;
  const uint64_t lt = (1ull << lane) - 1;
  for (int c0 = 0; c0 < count; c0 += 64) {
    const int cnt = min(64, count - c0);
    const bool valid = lane < cnt;
    const int op = valid ? op_at(c0 + lane) : OP_MATCH;
    const bool isq = valid && op != OP_DELETE, ist = valid && op != OP_INSERT;
    const uint64_t qmask = __ballot(isq), tmask = __ballot(ist);
    const int qidx = S.qi + __popcll(qmask & lt);
    const int tcons = S.tj + __popcll(tmask & lt) + (ist ? 1 : 0);
    const int j = tbgn - 1 + tcons;
    const uint64_t tbelow = tmask & lt;
    int jj = 0;
    if (!ist) jj = tbelow ? lane - (63 - __clzll(tbelow)) : S.jj + lane + 1;
    const int ch = isq ? (int)qp[min(qidx, qlen - 1)] : CH_GAP;
    // jj >= 65535 is skipped there and never becomes a predecessor, so p_jj never reaches it
    const bool emit = valid && !(op == OP_INSERT && (tcons == 0 || tcons == tlen)) && jj < 65535;
    const uint64_t emask = __ballot(emit);
    const uint64_t ebelow = emask & lt;
    const int src = ebelow ? 63 - __clzll(ebelow) : 0;
    int p_j = __shfl(j, src), p_jj = __shfl(jj, src), p_ch = __shfl(ch, src);
    if (!ebelow) { p_j = S.p_j; p_jj = S.p_jj; p_ch = S.p_ch; }
    const uint32_t at = S.ntags + (uint32_t)__popcll(ebelow);
    if (emit && at < cap) {
      keys[at] = tag_key(j, jj, ch, p_j, p_jj, p_ch);
      vals[at] = val0 + at;
    }
    if (emask) {
      const int lastl = 63 - __clzll(emask);
      S.p_j = __shfl(j, lastl);
      S.p_jj = __shfl(jj, lastl);
      S.p_ch = __shfl(ch, lastl);
      S.ntags += (uint32_t)__popcll(emask);
    }
    S.qi += __popcll(qmask);
    S.tj += __popcll(tmask);
    S.jj = tmask ? cnt - 1 - (63 - __clzll(tmask)) : S.jj + cnt;
  }
}

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK)
void k_fs_path(const uint8_t *__restrict__ fwd, const uint8_t *__restrict__ rcs,
               const Ev *__restrict__ evs, const Tp *__restrict__ tps, const uint32_t n_ev,
               const Loc *__restrict__ loc, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
               uint32_t *__restrict__ ntags_out, unsigned long long *__restrict__ cells,
               uint32_t *__restrict__ nleaf_out, uint32_t *__restrict__ nsplit_out,
               const edw::PathArgs scratch) {
  __shared__ uint32_t s_row[WAVES_PER_BLOCK][LDS_WORDS];
  __shared__ int s_stack[WAVES_PER_BLOCK][STACK_DEPTH][5];
  const int lane = threadIdx.x & 63;
  const int wave = uni((int)(threadIdx.x >> 6));
  const uint64_t gw = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave;
  const uint32_t n_waves = gridDim.x * WAVES_PER_BLOCK;
  const edw::PathScratch W = scratch.wave(gw);

  for (uint32_t e = (uint32_t)gw; e < n_ev; e += n_waves) {
    const Loc L = loc[e];
    if (!uni(L.ok)) {
      if (lane == 0) { ntags_out[e] = 0; nleaf_out[e] = 0; nsplit_out[e] = 0; }
      continue;
    }
    const Ev ev = evs[e];
    const int qlen = uni(ev.qlen);
    const int start = uni(L.start), tlen = uni(L.end) - start + 1;
    const int tbgn = uni(ev.wb) + start;
    const uint8_t *qp = (uni((int)ev.rc) ? rcs : fwd) + ev.seq;
    const uint8_t *tp = fwd + tps[ev.tmpl].seq + tbgn;
    uint64_t *ek = keys + ev.tag_off;
    uint32_t *evl = vals + ev.tag_off;
    const uint32_t val0 = (uint32_t)(ev.tag_off - tps[ev.tmpl].tag_off);
    const uint32_t cap = ev.tag_cap;
    TagState S{0, 0, 0, -1, 0, CH_NONE, 0};
    const edw::PathStats N = edw::wave_path<5>(
        Span{qp, qlen}, Span{tp, tlen}, uni(L.dist), W, s_row[wave], s_stack[wave], FS_LEAF_BYTES,
        [&](int count, auto op_at) {
          emit_tags(S, count, op_at, qp, qlen, tbgn, tlen, ek, evl, val0, cap);
        });
    if (lane == 0) {
      ntags_out[e] = S.ntags;
      cells[e] += N.cells;
      nleaf_out[e] = N.nleaf;
      nsplit_out[e] = N.nsplit;
    }
  }
}

// ------------------------------------------------------------------ consensus

__device__ __forceinline__ long long wave_max(long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const long long w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(64)
void k_fs_consensus(const Tp *__restrict__ tps, const uint32_t n_tp,
                    const uint64_t *__restrict__ skeys, const uint32_t *__restrict__ svals,
                    uint32_t *__restrict__ cov_all, uint32_t *__restrict__ lpos_all,
                    int *__restrict__ lpidx_all, uint64_t *__restrict__ ckey_all,
                    uint32_t *__restrict__ cfl_all, int *__restrict__ cscore_all,
                    int *__restrict__ cback_all, uint32_t *__restrict__ clink_all,
                    uint8_t *__restrict__ out_all, uint32_t *__restrict__ out_len,
                    const uint32_t min_cov) {
  const int lane = threadIdx.x & 63;
  const uint64_t lt = (1ull << lane) - 1;
  for (uint32_t t = blockIdx.x; t < n_tp; t += gridDim.x) {
    const Tp tp = tps[t];
    const uint64_t *K = skeys + tp.tag_off;
    const uint32_t *V = svals + tp.tag_off;
    uint32_t *cov = cov_all + tp.cov_off;
    uint32_t *lpos = lpos_all + tp.tag_off;
    int *lpidx = lpidx_all + tp.tag_off;
    uint64_t *ckey = ckey_all + tp.tag_off;
    uint32_t *cfl = cfl_all + tp.tag_off;
    int *cscore = cscore_all + tp.tag_off;
    int *cback = cback_all + tp.tag_off;
    uint32_t *clink = clink_all + tp.tag_off;
    const uint32_t cap = tp.tag_cap;

    // links: the runs of equal keys; coverage: the tags with delta 0
    uint32_t nl = 0, nvalid = 0;
    for (uint32_t i0 = 0; i0 < cap; i0 += 64) {
      const uint32_t i = i0 + lane;
      const uint64_t k = i < cap ? K[i] : KEY_NONE;
      const bool valid = k != KEY_NONE;
      const bool head = valid && (i == 0 || K[i - 1] != k);
      if (valid && ((k >> 27) & 0xffff) == 0) atomicAdd(&cov[k >> 43], 1u);
      const uint64_t hm = __ballot(head);
      if (head) lpos[nl + __popcll(hm & lt)] = i;
      nl += (uint32_t)__popcll(hm);
      const uint64_t vm = __ballot(valid);
      nvalid += (uint32_t)__popcll(vm);
      if (vm != ~0ull) break;                     // sorted: the unused slots are last
    }
    nl = (uint32_t)uni((int)nl);
    nvalid = (uint32_t)uni((int)nvalid);
    __threadfence();
    // columns: the runs of links with equal (t_pos, delta, slot)
    uint32_t nc = 0;
    for (uint32_t l0 = 0; l0 < nl; l0 += 64) {
      const uint32_t li = l0 + lane;
      const bool in = li < nl;
      const uint64_t ck = in ? K[lpos[li]] >> KEY_COL_SHIFT : 0;
      const bool head = in && (li == 0 || (K[lpos[li - 1]] >> KEY_COL_SHIFT) != ck);
      const uint64_t hm = __ballot(head);
      if (head) {
        const uint32_t at = nc + (uint32_t)__popcll(hm & lt);
        ckey[at] = ck;
        cfl[at] = li;
      }
      nc += (uint32_t)__popcll(hm);
    }
    nc = (uint32_t)uni((int)nc);
    __threadfence();
    // the predecessor column of every link
    for (uint32_t li = lane; li < nl; li += 64) {
      const uint64_t k = K[lpos[li]];
      const int prel = (int)((k >> 19) & 3);
      int idx = -1;
      if (prel) {
        const uint64_t p_t = (k >> 43) - (prel == 1 ? 1 : 0);
        const uint64_t p_ch = k & 7;
        const uint64_t want = (p_t << 22) | (((k >> 3) & 0xffff) << 6) | ((p_ch < 4 ? p_ch : 4) << 3);
        // ckey is key >> 21: t_pos at bit 22, delta at 6, slot at 3, the low three bits 0
        uint32_t lo = 0, hi = nc;
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if ((ckey[mid] >> 3 << 3) < want) lo = mid + 1; else hi = mid;
        }
        if (lo < nc && (ckey[lo] >> 3 << 3) == want) idx = (int)lo;
      }
      lpidx[li] = idx;
    }
    __threadfence();
    // the scan, in (t_pos, delta, slot) order.  ring: lane (x & 63) holds the score of column
    // x for the last 64 columns; an older one is read back from memory.
    int ring = 0;
    int gbest = 0, gcol = -1;
    for (uint32_t c = 0; c < nc; c++) {
      const uint32_t l0 = cfl[c], l1 = c + 1 < nc ? cfl[c + 1] : nl;
      const int covv = (int)cov[ckey[c] >> 22];
      long long bestv = 0;
      int bli = -1, bpidx = -1;
      for (uint32_t lb = l0; lb < l1; lb += 64) {
        const uint32_t li = lb + lane;
        const bool in = li < l1;
        int pidx = -1, cnt = 0;
        uint32_t first = 0;
        if (in) {
          const uint32_t p = lpos[li];
          cnt = (int)((li + 1 < nl ? lpos[li + 1] : nvalid) - p);
          pidx = lpidx[li];
          first = V[p];
        }
        const bool far = pidx >= 0 && c - (uint32_t)pidx > 64;
        if (__any(far)) __threadfence();              // lane 0's stores, for every lane
        const int near = __shfl(ring, pidx & 63);     // every lane is in: a ring lane may be idle
        int s = 2 * cnt - covv;
        if (pidx >= 0) s += far ? cscore[pidx] : near;
        // a higher score wins; at equal scores the link that appeared first
        const long long v = in && s > 0 ? ((long long)s << 32) | (long long)(0xffffffffu - first) : 0;
        const long long mx = wave_max(v);
        if (mx > bestv) {
          bestv = mx;
          const uint64_t who = __ballot(v == mx);
          const int src = __ffsll((unsigned long long)who) - 1;
          bli = __shfl((int)li, src);
          bpidx = __shfl(pidx, src);
        }
      }
      const int cs = (int)(bestv >> 32);
      if (lane == 0) {
        cscore[c] = cs;
        cback[c] = cs > 0 ? bpidx : -1;
        clink[c] = (uint32_t)bli;
      }
      if (lane == (int)(c & 63)) ring = cs;
      if (cs > gbest) { gbest = cs; gcol = (int)c; }
    }
    __threadfence();
    // the walk back.  The first letter is chosen by the index of the best link among the
    // column's links in order of first appearance (g_best_ck, falconConsensus.C:232-236).
    uint32_t index = 0;
    uint8_t *out = out_all + tp.out_off;
    const uint32_t ocap = 2u * (uint32_t)tp.len;
    if (gcol >= 0) {
      const uint32_t l0 = cfl[gcol], l1 = (uint32_t)gcol + 1 < nc ? cfl[gcol + 1] : nl;
      const uint32_t bfirst = V[lpos[clink[gcol]]];
      uint32_t rank = 0;
      for (uint32_t lb = l0; lb < l1; lb += 64) {
        const uint32_t li = lb + lane;
        const bool before = li < l1 ? V[lpos[li]] < bfirst : false;
        rank += (uint32_t)__popcll(__ballot(before));
      }
      int ck = rank < 4 ? (int)rank : 4;
      int col = gcol;
      while (true) {
        const uint32_t pos = (uint32_t)(ckey[col] >> 22);
        const bool low = cov[pos] <= min_cov;
        const uint8_t bb = ck == 4 ? 0 : (uint8_t)((low ? "acgt" : "ACGT")[ck]);
        const int prev = cback[col];
        if (prev < 0 || index >= ocap) break;
        col = prev;
        ck = (int)((ckey[col] >> 3) & 7);
        if (bb) {
          if (lane == 0) out[ocap - 1 - index] = bb;
          index++;
        }
      }
    }
    if (lane == 0) out_len[t] = index;
  }
}

}  // namespace

// ------------------------------------------------------------------ host

struct fs_ctx : capi::Device {
  fs_params P{};
  edw::Strands R;
  // the last result
  bool have = false;
  std::vector<uint32_t> tig_ids;
  std::vector<uint64_t> r_off;
  std::vector<uint8_t> r_bases;
  std::vector<uint32_t> r_counts;
  fs_stats S{};
};

namespace {

int check_params(const fs_params *p) {
  if (!p) return fail(FS_ERR_BAD_PARAM, "null parameters");
  if (!(p->min_identity >= 0.0) || p->min_identity > 1.0)
    return fail(FS_ERR_BAD_PARAM, "min_identity %g outside [0, 1]", p->min_identity);
  return FS_OK;
}

// One batch of layouts on the device.
int run_batch(fs_ctx *c, const std::vector<Tp> &tps_in, const std::vector<Ev> &evs,
              const std::vector<uint32_t> &ev_layout, const uint32_t layout0, uint32_t max_q,
              uint32_t max_window, uint64_t total_tags, uint64_t total_cov, uint64_t total_out) {
  std::vector<Tp> tps = tps_in;
  const uint32_t n_tp = (uint32_t)tps.size(), n_ev = (uint32_t)evs.size();
  fs_stats &S = c->S;
  const uint32_t want_waves = (uint32_t)c->n_cu * 4;
  const uint32_t blocks = std::max<uint32_t>(1, std::min<uint32_t>((n_ev + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK,
                                                                   want_waves / WAVES_PER_BLOCK));
  const uint64_t waves = (uint64_t)blocks * WAVES_PER_BLOCK;
  const edw::PathSize Z = edw::path_size(max_q, max_window, FS_LEAF_BYTES);

  DevBuf<Tp> d_tp;
  DevBuf<Ev> d_ev;
  DevBuf<Loc> d_loc;
  DevBuf<unsigned long long> d_cells;
  DevBuf<uint32_t> d_ntags, d_nleaf, d_nsplit, d_vals, d_vals2, d_cov, d_lpos, d_cfl, d_clink, d_outlen;
  DevBuf<uint64_t> d_keys, d_keys2, d_ckey;
  DevBuf<int> d_lpidx, d_cscore, d_cback, d_segoff;
  DevBuf<uint8_t> d_out, d_sort;
  edw::PathBuffers path;
  HIP_TRY(d_tp.alloc(n_tp));
  HIP_TRY(d_ev.alloc(n_ev));
  HIP_TRY(d_loc.alloc(n_ev));
  HIP_TRY(d_cells.alloc(n_ev));
  HIP_TRY(d_ntags.alloc(n_ev));
  HIP_TRY(d_nleaf.alloc(n_ev));
  HIP_TRY(d_nsplit.alloc(n_ev));
  HIP_TRY(d_keys.alloc(total_tags));
  HIP_TRY(d_keys2.alloc(total_tags));
  HIP_TRY(d_vals.alloc(total_tags));
  HIP_TRY(d_vals2.alloc(total_tags));
  HIP_TRY(path.alloc(Z, waves));
  HIP_TRY(d_cov.alloc(total_cov));
  HIP_TRY(d_lpos.alloc(total_tags));
  HIP_TRY(d_lpidx.alloc(total_tags));
  HIP_TRY(d_ckey.alloc(total_tags));
  HIP_TRY(d_cfl.alloc(total_tags));
  HIP_TRY(d_cscore.alloc(total_tags));
  HIP_TRY(d_cback.alloc(total_tags));
  HIP_TRY(d_clink.alloc(total_tags));
  HIP_TRY(d_out.alloc(total_out));
  HIP_TRY(d_outlen.alloc(n_tp));
  HIP_TRY(d_segoff.alloc(n_tp + 1));
  uint64_t scratch = path.bytes();
  for (size_t b : {d_keys.bytes, d_keys2.bytes, d_vals.bytes, d_vals2.bytes, d_cov.bytes, d_lpos.bytes,
                   d_lpidx.bytes, d_ckey.bytes, d_cfl.bytes, d_cscore.bytes, d_cback.bytes,
                   d_clink.bytes, d_out.bytes})
    scratch += b;
  S.scratch_bytes = std::max<uint64_t>(S.scratch_bytes, scratch);

  std::vector<int> segoff(n_tp + 1);
  for (uint32_t i = 0; i < n_tp; i++) segoff[i] = (int)tps[i].tag_off;
  segoff[n_tp] = (int)total_tags;
  hipStream_t s = c->stream;
  HIP_TRY(hipMemcpyAsync(d_tp.p, tps.data(), n_tp * sizeof(Tp), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_ev.p, evs.data(), n_ev * sizeof(Ev), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d_segoff.p, segoff.data(), (n_tp + 1) * sizeof(int), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(d_keys.p, 0xff, std::max<uint64_t>(total_tags, 1) * 8, s));
  HIP_TRY(hipMemsetAsync(d_vals.p, 0, std::max<uint64_t>(total_tags, 1) * 4, s));
  HIP_TRY(hipMemsetAsync(d_cov.p, 0, std::max<uint64_t>(total_cov, 1) * 4, s));

  hipEvent_t ev[5];
  for (auto &x : ev) HIP_TRY(hipEventCreate(&x));
  HIP_TRY(hipEventRecord(ev[0], s));
  hipLaunchKernelGGL(k_fs_locate, dim3(blocks), dim3(64 * WAVES_PER_BLOCK), 0, s, c->R.fwd.p, c->R.rc.p,
                     d_ev.p, d_tp.p, n_ev, d_loc.p, d_cells.p, path.grow_rows(), Z.grow_words,
                     1.0 - c->P.min_identity);
  hipError_t le = hipGetLastError();
  HIP_TRY(hipEventRecord(ev[1], s));
  if (le == hipSuccess) {
    hipLaunchKernelGGL(k_fs_path, dim3(blocks), dim3(64 * WAVES_PER_BLOCK), 0, s, c->R.fwd.p, c->R.rc.p,
                       d_ev.p, d_tp.p, n_ev, d_loc.p, d_keys.p, d_vals.p, d_ntags.p, d_cells.p,
                       d_nleaf.p, d_nsplit.p, path.args());
    le = hipGetLastError();
  }
  HIP_TRY(hipEventRecord(ev[2], s));
  if (le == hipSuccess && total_tags) {
    size_t tb = 0;
    le = hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, tb, d_keys.p, d_keys2.p, d_vals.p,
                                                     d_vals2.p, (int)total_tags, (int)n_tp,
                                                     d_segoff.p, d_segoff.p + 1, 0, 64, s);
    if (le == hipSuccess) le = d_sort.alloc(tb);
    if (le == hipSuccess)
      le = hipcub::DeviceSegmentedRadixSort::SortPairs(d_sort.p, tb, d_keys.p, d_keys2.p, d_vals.p,
                                                       d_vals2.p, (int)total_tags, (int)n_tp,
                                                       d_segoff.p, d_segoff.p + 1, 0, 64, s);
  }
  HIP_TRY(hipEventRecord(ev[3], s));
  if (le == hipSuccess) {
    hipLaunchKernelGGL(k_fs_consensus, dim3(std::min<uint32_t>(n_tp, 65535u)), dim3(64), 0, s, d_tp.p,
                       n_tp, d_keys2.p, d_vals2.p, d_cov.p, d_lpos.p, d_lpidx.p, d_ckey.p, d_cfl.p,
                       d_cscore.p, d_cback.p, d_clink.p, d_out.p, d_outlen.p, c->P.min_coverage);
    le = hipGetLastError();
  }
  HIP_TRY(hipEventRecord(ev[4], s));
  hipError_t se = hipStreamSynchronize(s);
  float ms[4] = {0, 0, 0, 0};
  if (le == hipSuccess && se == hipSuccess)
    for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
  for (auto &x : ev) (void)hipEventDestroy(x);
  HIP_TRY(le);
  HIP_TRY(se);
  S.ms_locate += ms[0];
  S.ms_path += ms[1];
  S.ms_sort += ms[2];
  S.ms_consensus += ms[3];

  std::vector<Loc> loc(n_ev);
  std::vector<unsigned long long> cells(n_ev);
  std::vector<uint32_t> ntags(n_ev), nleaf(n_ev), nsplit(n_ev), outlen(n_tp);
  std::vector<uint8_t> out(std::max<uint64_t>(total_out, 1));
  HIP_TRY(hipMemcpy(loc.data(), d_loc.p, n_ev * sizeof(Loc), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cells.data(), d_cells.p, n_ev * 8ull, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ntags.data(), d_ntags.p, n_ev * 4ull, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(nleaf.data(), d_nleaf.p, n_ev * 4ull, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(nsplit.data(), d_nsplit.p, n_ev * 4ull, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(outlen.data(), d_outlen.p, n_tp * 4ull, hipMemcpyDeviceToHost));
  if (total_out) HIP_TRY(hipMemcpy(out.data(), d_out.p, total_out, hipMemcpyDeviceToHost));
  for (uint32_t e = 0; e < n_ev; e++) {
    if (ntags[e] > evs[e].tag_cap)
      return fail(FS_ERR_HIP, "evidence %u wrote %u tags into %u slots", e, ntags[e], evs[e].tag_cap);
    const uint32_t l = ev_layout[e];
    if (loc[e].ok) { c->r_counts[3 * (size_t)l + 0]++; S.n_aligned++; }
    else { c->r_counts[3 * (size_t)l + 2]++; S.n_rejected++; }
    S.dp_cells += cells[e];
    S.n_tags += ntags[e];
    S.n_leaves += nleaf[e];
    S.n_splits += nsplit[e];
  }
  for (uint32_t i = 0; i < n_tp; i++) {
    const uint64_t cap = 2ull * (uint64_t)tps[i].len;
    if (outlen[i] > cap) return fail(FS_ERR_HIP, "template %u: consensus of %u bases", i, outlen[i]);
    const uint8_t *p = out.data() + tps[i].out_off + (cap - outlen[i]);
    c->r_bases.insert(c->r_bases.end(), p, p + outlen[i]);
    c->r_off[layout0 + i + 1] = c->r_bases.size();
  }
  S.n_batches++;
  return FS_OK;
}

}  // namespace

extern "C" {

void fs_params_init(fs_params *p) {
  if (!p) return;
  p->min_coverage = 4;          // falconsense.C:218-220
  p->min_identity = 0.5;
  p->min_output_length = 500;
  p->hbm_budget = 0;
}

const char *fs_last_error(void) { return capi::g_err.c_str(); }
int fs_abi_version(void) { return FS_ABI_VERSION; }

int fs_ctx_create(const fs_params *p, int device, fs_ctx **out) {
  if (!out) return fail(FS_ERR_BAD_PARAM, "null out");
  *out = nullptr;
  if (int rc = check_params(p)) return rc;
  return capi::create_ctx(p, device, out);
}

void fs_ctx_destroy(fs_ctx *c) { capi::destroy_ctx(c); }

int fs_set_params(fs_ctx *c, const fs_params *p) {
  if (!c) return fail(FS_ERR_BAD_PARAM, "null context");
  if (int rc = check_params(p)) return rc;
  c->P = *p;
  return FS_OK;
}

int fs_load_reads_device(fs_ctx *c, uint32_t first_iid, uint32_t nreads, const uint8_t *d_bases,
                         const uint64_t *d_offsets, const uint32_t *h_lengths) {
  if (!c) return fail(FS_ERR_BAD_PARAM, "null context");
  if (int rc = capi::check_device_reads(first_iid, nreads, d_bases, d_offsets, h_lengths)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  c->have = false;
  return edw::load_strands(c->R, c->stream, false, first_iid, nreads, d_bases, d_offsets, h_lengths);
}

int fs_load_reads(fs_ctx *c, uint32_t first_iid, uint32_t nreads, const uint8_t *bases,
                  const uint64_t *offsets, const uint32_t *lengths) {
  if (!c) return fail(FS_ERR_BAD_PARAM, "null context");
  DevBuf<uint8_t> d_b;
  DevBuf<uint64_t> d_o;
  if (int rc = capi::stage_reads(c->device, nreads, bases, offsets, lengths, d_b, d_o)) return rc;
  return fs_load_reads_device(c, first_iid, nreads, d_b.p, d_o.p, lengths);
}

int fs_consensus(fs_ctx *c, const fs_layout *layouts, uint64_t n_layouts, const fs_child *children,
                 uint64_t n_children) {
  if (!c) return fail(FS_ERR_BAD_PARAM, "null context");
  if ((n_layouts && !layouts) || (n_children && !children))
    return fail(FS_ERR_BAD_PARAM, "null layouts or children");
  if (n_layouts > 0xfffffff0ull) return fail(FS_ERR_BAD_PARAM, "more than 2^32 layouts in one call");
  HIP_TRY(hipSetDevice(c->device));
  c->have = false;
  c->S = fs_stats{};
  auto loaded = [&](uint32_t id) { return id >= c->R.first_iid && id - c->R.first_iid < c->R.nreads; };
  // the checks the reference leaves to its assertions
  for (uint64_t i = 0; i < n_layouts; i++) {
    const fs_layout &l = layouts[i];
    if (!loaded(l.tig_id))
      return fail(FS_ERR_BAD_INPUT, "layout %llu: template read %u is not loaded",
                  (unsigned long long)i, l.tig_id);
    if (l.n_children > FS_MAX_CHILDREN)
      return fail(FS_ERR_BAD_INPUT, "layout %llu (read %u) has %u children, more than %d",
                  (unsigned long long)i, l.tig_id, l.n_children, FS_MAX_CHILDREN);
    if ((uint64_t)l.first_child + l.n_children > n_children)
      return fail(FS_ERR_BAD_PARAM, "layout %llu: children %u..%llu of %llu", (unsigned long long)i,
                  l.first_child, (unsigned long long)l.first_child + l.n_children,
                  (unsigned long long)n_children);
    for (uint32_t k = 0; k < l.n_children; k++) {
      const fs_child &ch = children[l.first_child + k];
      if (!loaded(ch.ident))
        return fail(FS_ERR_BAD_INPUT, "layout %llu: child read %u is not loaded",
                    (unsigned long long)i, ch.ident);
      const uint32_t len = c->R.len[ch.ident - c->R.first_iid];
      if (ch.askip < 0 || ch.bskip < 0 || (uint64_t)ch.askip + (uint64_t)ch.bskip > len)
        return fail(FS_ERR_BAD_INPUT, "layout %llu: child %u skips %d + %d of %u bases",
                    (unsigned long long)i, ch.ident, ch.askip, ch.bskip, len);
      if (ch.max <= ch.min)
        return fail(FS_ERR_BAD_INPUT, "layout %llu: child %u placed at %d..%d", (unsigned long long)i,
                    ch.ident, ch.min, ch.max);
    }
  }
  c->tig_ids.resize(n_layouts);
  c->r_off.assign(n_layouts + 1, 0);
  c->r_bases.clear();
  c->r_counts.assign(3 * n_layouts, 0);
  c->S.n_layouts = n_layouts;
  const double max_difference = 1.0 - c->P.min_identity;
  const uint64_t budget = c->P.hbm_budget ? c->P.hbm_budget : (4ull << 30);
  // device bytes a tag slot costs: keys and values twice, and the seven per-link arrays
  const uint64_t per_tag = 2 * 8 + 2 * 4 + 4 + 4 + 8 + 4 + 4 + 4 + 4;

  uint64_t i = 0;
  while (i < n_layouts) {
    std::vector<Tp> tps;
    std::vector<Ev> evs;
    std::vector<uint32_t> ev_layout;
    uint64_t tags = 0, cov = 0, out = 0;
    uint32_t max_q = 1, max_window = 1;
    const uint64_t first = i;
    for (; i < n_layouts; i++) {
      const fs_layout &l = layouts[i];
      const uint32_t tr = l.tig_id - c->R.first_iid;
      const int32_t tlen = (int32_t)c->R.len[tr];
      std::vector<Ev> mine;
      uint64_t my_tags = 0;
      uint32_t skipped = 0;
      for (uint32_t k = 0; k <= l.n_children; k++) {
        Ev e{};
        int32_t len, bgn, end;
        if (k == 0) {                               // the template, placed on itself
          e.seq = c->R.off[tr];
          len = tlen; bgn = 0; end = tlen;
        } else {
          const fs_child &ch = children[l.first_child + k - 1];
          const uint32_t r = ch.ident - c->R.first_iid;
          e.rc = ch.reverse ? 1 : 0;
          e.seq = c->R.off[r] + (uint32_t)ch.askip;
          len = (int32_t)c->R.len[r] - ch.askip - ch.bskip;
          bgn = ch.min; end = ch.max;
        }
        if (len > tlen) len = tlen;                 // falconConsensus-alignTag.C:130-134
        if (len < FS_MIN_EVIDENCE) { skipped++; continue; }
        e.qlen = len;
        e.tol = (int32_t)ceil(std::min(len, tlen) * max_difference * 1.1);
        const int32_t expansion = (int32_t)((1.4 * len - (end - bgn)) / 2);
        if (expansion > 0) { bgn -= expansion; end += expansion; }
        if (bgn < 0) bgn = 0;
        if (end > tlen) end = tlen;
        if (end <= bgn)
          return fail(FS_ERR_BAD_INPUT, "layout %llu: an evidence read is placed outside its "
                      "template", (unsigned long long)i);
        e.wb = bgn; e.we = end;
        e.tag_cap = (uint32_t)len + (uint32_t)(end - bgn);
        e.tag_off = my_tags;
        my_tags += e.tag_cap;
        mine.push_back(e);
      }
      const uint64_t need = (tags + my_tags) * per_tag + (cov + (uint64_t)tlen) * 4 + out + 2ull * tlen;
      if (!tps.empty() && (need > budget || tags + my_tags > 0x7fffffffull)) break;
      if (my_tags > 0x7fffffffull)
        return fail(FS_ERR_UNSUPPORTED, "layout %llu needs %llu tag slots, more than 2^31",
                    (unsigned long long)i, (unsigned long long)my_tags);
      Tp t{};
      t.seq = c->R.off[tr];
      t.tag_off = tags;
      t.cov_off = cov;
      t.out_off = out;
      t.tag_cap = (uint32_t)my_tags;
      t.len = tlen;
      for (Ev &e : mine) {
        e.tag_off += tags;
        e.tmpl = (uint32_t)tps.size();
        max_q = std::max<uint32_t>(max_q, (uint32_t)e.qlen);
        max_window = std::max<uint32_t>(max_window, (uint32_t)(e.we - e.wb));
        evs.push_back(e);
        ev_layout.push_back((uint32_t)i);
      }
      tps.push_back(t);
      tags += my_tags;
      cov += (uint64_t)tlen;
      out += 2ull * tlen;
      c->tig_ids[i] = l.tig_id;
      c->r_counts[3 * i + 1] = skipped;
      c->S.n_skipped += skipped;
      c->S.n_evidence += (uint64_t)l.n_children + 1;
    }
    if (int rc = run_batch(c, tps, evs, ev_layout, (uint32_t)first, max_q, max_window, tags, cov, out))
      return rc;
  }
  c->have = true;
  return FS_OK;
}

int fs_result_size(const fs_ctx *c, uint64_t *n_layouts, uint64_t *n_bases) {
  if (!c) return fail(FS_ERR_BAD_PARAM, "null context");
  if (!c->have) return fail(FS_ERR_STATE, "no result: call fs_consensus first");
  if (n_layouts) *n_layouts = c->tig_ids.size();
  if (n_bases) *n_bases = c->r_bases.size();
  return FS_OK;
}

int fs_fetch(const fs_ctx *c, uint8_t *bases, uint64_t *offsets, uint32_t *counts) {
  if (!c) return fail(FS_ERR_BAD_PARAM, "null context");
  if (!c->have) return fail(FS_ERR_STATE, "no result: call fs_consensus first");
  if (bases && !c->r_bases.empty()) memcpy(bases, c->r_bases.data(), c->r_bases.size());
  if (offsets) memcpy(offsets, c->r_off.data(), c->r_off.size() * 8);
  if (counts && !c->r_counts.empty()) memcpy(counts, c->r_counts.data(), c->r_counts.size() * 4);
  return FS_OK;
}

int fs_write_fasta_file(const fs_ctx *c, FILE *f) {
  if (!c || !f) return fail(FS_ERR_BAD_PARAM, "null argument");
  if (!c->have) return fail(FS_ERR_STATE, "no result: call fs_consensus first");
  std::string out;
  for (size_t i = 0; i < c->tig_ids.size(); i++) {
    out.clear();
    fs_fasta_pieces(out, nullptr, c->tig_ids[i], c->r_bases.data() + c->r_off[i],
                    c->r_off[i + 1] - c->r_off[i], c->P.min_output_length);
    if (!out.empty() && fwrite(out.data(), 1, out.size(), f) != out.size())
      return fail(FS_ERR_STATE, "short write");
  }
  return FS_OK;
}

int fs_write_fasta(const fs_ctx *c, const char *path) {
  if (!c || !path) return fail(FS_ERR_BAD_PARAM, "null argument");
  FILE *f = fopen(path, "wb");
  if (!f) return fail(FS_ERR_BAD_PARAM, "cannot write %s", path);
  const int rc = fs_write_fasta_file(c, f);
  if (fclose(f) != 0 && rc == FS_OK) return fail(FS_ERR_STATE, "cannot close %s", path);
  return rc;
}

int fs_get_stats(const fs_ctx *c, fs_stats *out) {
  if (!c || !out) return fail(FS_ERR_BAD_PARAM, "null argument");
  *out = c->S;
  return FS_OK;
}

}  // extern "C"
