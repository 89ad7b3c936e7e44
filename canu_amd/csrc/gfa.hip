// gfa.hip -- libcanu_gfa.so: canu's alignGFA (src/gfa/alignGFA.C) on gfx950.  include/canu_gfa.h
// says what is reproduced; this is how.
//
//   k_gfa_hw     one wave per alignment: edlib's EDLIB_MODE_HW / EDLIB_TASK_LOC result in closed
//                form.  An infix pass gives the distance and the first best end column; where
//                the caller needs it, a prefix pass of the reversed query over the reversed
//                target up to that column gives the longest start.  It serves checkLink's two
//                extension steps (one launch each, all links together) and every round of
//                checkRecord_align's loop (one launch per round over the calls still open).
//   k_gfa_path   one wave per link: the global distance, then -- within 2 * maxEdit --
//                obtainAlignment's recursion with an explicit stack in LDS, as fs.hip's k_fs_path
//                runs it: a split keeps Pv / Mv and the end score of every 64-row block of the
//                two last columns and takes the first row where they meet at the distance; a
//                leaf keeps every column and walks up / left / diagonal from the corner.  The
//                operations of a leaf (one byte each, backwards) become CIGAR runs 64 at a time
//                with ballots; a run that crosses a chunk or a leaf is carried in the wave's
//                state.  Per-base operations never leave the device.
//
// An oriented tig is never copied: a span of a reversed tig is read backwards through the
// complement, with N as a sixth symbol (the NUL of reverseComplementCopy) that equals only
// itself.  The host's part of a link or record is the reference's double arithmetic
// (gfa_host.h) between the launches.
//
// The aligner core (dp_pass) is that of pair.hip and fs.hip: Myers' bit-vector recurrence, lane b
// holding rows 64b..64b+63, columns as a skewed wavefront, 4096-row stripes, the stripe boundary
// row in LDS up to 16384 columns and in a global row beyond.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/canu_gfa.h"
#include "capi_common.h"
#include "gfa_host.h"

namespace {

using capi::fail;

CAPI_SAME_CODES(GFA);
constexpr int WAVES_PER_BLOCK = 4;
constexpr int STRIPE_ROWS = 4096;                     // 64 lanes x 64 rows
constexpr int LDS_COLUMNS = 16384;                    // stripe-boundary row kept in LDS
constexpr int LDS_WORDS = LDS_COLUMNS / 16;           // 2 bits per column
constexpr int LEAF_ENTRIES = GFA_LEAF_BYTES / 20 + 1; // block columns of a leaf
constexpr int STACK_DEPTH = 40;                       // the target halves at every level

enum : int { OP_MATCH = 0, OP_INSERT = 1, OP_DELETE = 2, OP_MISMATCH = 3 };   // EDLIB_EDOP_*
enum : int { CODE_N = 4, CODE_NUL = 5, CODE_PAD = 7 };

struct Span {                // a stretch of a tig, in the tig's own coordinates
  uint64_t off;              // its first byte in the set's array
  int32_t n;
  uint32_t flags;            // bit 0: read as the reverse complement; bit 1: GFA_SET_C
};

struct HwJob {
  Span q, t;
  int32_t k;
  int32_t need_start;
};

struct HwOut {
  int32_t dist, start, end;  // dist -1: nothing within k
  int32_t pad;
  unsigned long long cells;
};

struct NwJob {
  Span q, t;
  int32_t k;
  uint32_t run_cap;
  uint64_t run_off;
};

struct NwOut {
  int32_t dist, align_len;
  uint32_t n_runs, n_leaf, n_split, pad;
  unsigned long long cells;
};

// ------------------------------------------------------------------ tig encoding

__global__ void k_gfa_encode(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ src_off,
                             const uint64_t *__restrict__ dst_off, const uint32_t *__restrict__ len,
                             uint32_t ntigs, uint8_t *__restrict__ codes, uint32_t *__restrict__ bad) {
  for (uint32_t r = blockIdx.x; r < ntigs; r += gridDim.x) {
    const uint8_t *s = bases + src_off[r];
    const uint64_t d = dst_off[r];
    const uint32_t L = len[r];
    for (uint32_t i = threadIdx.x; i < L; i += blockDim.x) {
      const uint8_t ch = s[i];
      uint8_t c = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : CODE_N;
      if (c == CODE_N && ch != 'N') atomicOr(bad, 1u);
      codes[d + i] = c;
    }
  }
}

// ------------------------------------------------------------------ the aligner

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ int dpp_from_lower(int v, int lane0) {   // lane l <- v[l-1]
  return __builtin_amdgcn_update_dpp(lane0, v, 0x138, 0xf, 0xf, false);
}

struct Seq {                 // a span as the aligner reads it
  const uint8_t *p;
  int n;
  int rev;                   // element i is p[n-1-i]
  int comp;                  // through reverseComplementCopy's table: ACGT complemented, N -> NUL
  __device__ __forceinline__ int at(int i) const {
    const int c = p[rev ? n - 1 - i : i];
    return comp ? (c < 4 ? 3 - c : CODE_NUL) : c;
  }
};

struct Ori {                 // an oriented span: element i of it is at(i) of fwd()
  const uint8_t *p;
  int n;
  int rc;
  __device__ __forceinline__ Seq fwd() const { return Seq{p, n, rc, rc}; }
  __device__ __forceinline__ Seq bwd() const { return Seq{p, n, !rc, rc}; }
  __device__ __forceinline__ Ori sub(int o, int len) const {
    return Ori{rc ? p + (n - o - len) : p + o, len, rc};
  }
};

__device__ __forceinline__ Ori ori_of(const Span s, const uint8_t *tigT, const uint8_t *tigC) {
  return Ori{((s.flags & 2u) ? tigC : tigT) + s.off, s.n, (int)(s.flags & 1u)};
}

struct PassOut {
  int best, bestcol;         // minimum of the bottom row, the first column attaining it
  int lastcol;               // last column whose bottom-row score == want (-1: none)
  int fin;                   // bottom-row score at the last column
};

// What a pass leaves behind besides its bottom row.  Block g is rows 64g..64g+63.
struct Keep {
  uint64_t *colP, *colM;     // leaf: Pv / Mv of block g after column j at [g * n + j]
  int *colS;                 //       and the score of the block's last row there
  uint64_t *endP, *endM;     // split: Pv / Mv of block g after the last column at [g]
  int *endS;                 //        and the score of the block's last row there
};

// Bottom row of the edit-distance matrix of q (rows) against t (columns); top_hin 0 lets an
// alignment start at any column (infix), 1 charges every skipped target base (prefix, global).
// Needs q.n >= 1, t.n >= 1.  Every lane of the wave is in, with the same arguments.
__device__ PassOut dp_pass(const Seq q, const Seq t, const int top_hin, const int want,
                           uint32_t *lrow, uint32_t *grow, const Keep keep) {
  const int lane = threadIdx.x & 63;
  const int m = q.n, n = t.n;
  const int nstripes = (m + STRIPE_ROWS - 1) / STRIPE_ROWS;
  const bool use_g = n > LDS_COLUMNS;
  int best = INT_MAX, bestcol = -1, lastcol = -1, sc = m;
  int lb = 0;
  for (int st = 0; st < nstripes; st++) {
    const int r0 = st * STRIPE_ROWS;
    const int rows = min(STRIPE_ROWS, m - r0);
    const int nb = (rows + 63) >> 6;
    const bool last = st == nstripes - 1;
    lb = nb - 1;
    uint64_t pe0 = 0, pe1 = 0, pe2 = 0, pe3 = 0, pe4 = 0, pe5 = 0;
    for (int c = 0; c < nb; c++) {
      const int i = r0 + c * 64 + lane;
      const int code = i < m ? q.at(i) : CODE_PAD;
      const uint64_t b0 = __ballot(code == 0), b1 = __ballot(code == 1),
                     b2 = __ballot(code == 2), b3 = __ballot(code == 3),
                     b4 = __ballot(code == CODE_N), b5 = __ballot(code == CODE_NUL);
      if (lane == c) { pe0 = b0; pe1 = b1; pe2 = b2; pe3 = b3; pe4 = b4; pe5 = b5; }
    }
    uint64_t Pv = ~0ull, Mv = 0;
    const bool trk = last && lane == lb;
    // the last row of this lane's block, whose score the lane follows along the columns (the
    // boundary column holds row + 1)
    const int lrow_abs = min(r0 + 64 * (lane + 1), m) - 1;
    const int rr = lane < nb ? (lrow_abs & 63) : 63;
    sc = lrow_abs + 1;
    const size_t gblk = (size_t)(st * 64 + lane);
    int x = 1;                                  // (hout + 1) | base << 2, handed to lane + 1
    uint32_t cur = lane < n ? (uint32_t)t.at(lane) : (uint32_t)CODE_PAD;
    uint32_t nxt = 64 + lane < n ? (uint32_t)t.at(64 + lane) : (uint32_t)CODE_PAD;
    uint32_t hw = 0, acc = 0;
    const int nsteps = n + nb - 1;
    for (int s = 0; s < nsteps; s++) {
      if ((s & 63) == 0 && s > 0) {
        cur = nxt;
        const int c = s + 64 + lane;
        nxt = c < n ? (uint32_t)t.at(c) : (uint32_t)CODE_PAD;
      }
      const int base0 = __builtin_amdgcn_readlane((int)cur, s & 63);
      int hin0 = top_hin;
      if (st > 0) {
        if ((s & 15) == 0 && s < n) hw = use_g ? grow[s >> 4] : lrow[s >> 4];
        hin0 = (int)((hw >> (2 * (s & 15))) & 3u) - 1;
      }
      const int xin = dpp_from_lower(x, (hin0 + 1) | (base0 << 2));
      const int j = s - lane;
      const bool act = lane < nb && j >= 0 && j < n;
      int d = 0;
      if (act) {
        const int hin = (xin & 3) - 1;
        const int b = xin >> 2;
        const uint64_t s0 = 0 - (uint64_t)(b & 1), s1 = 0 - (uint64_t)((b >> 1) & 1),
                       s2 = 0 - (uint64_t)(b >> 2);
        const uint64_t e01 = (pe0 & ~s0) | (pe1 & s0), e23 = (pe2 & ~s0) | (pe3 & s0);
        const uint64_t e45 = (pe4 & ~s0) | (pe5 & s0);
        const uint64_t e03 = (e01 & ~s1) | (e23 & s1);
        uint64_t Eq = (e03 & ~s2) | (e45 & s2);
        const uint64_t neg = hin < 0 ? 1ull : 0ull, pos = hin > 0 ? 1ull : 0ull;
        const uint64_t Xv = Eq | Mv;
        Eq |= neg;
        const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        uint64_t Ph = Mv | ~(Xh | Pv);
        uint64_t Mh = Pv & Xh;
        d = (int)((Ph >> 63) & 1) - (int)((Mh >> 63) & 1);
        sc += (int)((Ph >> rr) & 1) - (int)((Mh >> rr) & 1);
        Ph = (Ph << 1) | pos;
        Mh = (Mh << 1) | neg;
        Pv = Mh | ~(Xv | Ph);
        Mv = Ph & Xv;
        if (trk) {
          if (sc < best) { best = sc; bestcol = j; }
          if (sc == want) lastcol = j;
        }
        if (keep.colP) {
          const size_t at = gblk * (size_t)n + (size_t)j;
          keep.colP[at] = Pv;
          keep.colM[at] = Mv;
          keep.colS[at] = sc;
        }
        if (!last && lane == lb) {              // lane 63: the next stripe's top boundary
          acc |= (uint32_t)(d + 1) << (2 * (j & 15));
          if ((j & 15) == 15 || j == n - 1) {
            if (use_g) grow[j >> 4] = acc; else lrow[j >> 4] = acc;
            acc = 0;
          }
        }
      }
      x = (d + 1) | (xin & ~3);
    }
    if (keep.endP && lane < nb) {
      keep.endP[gblk] = Pv;
      keep.endM[gblk] = Mv;
      keep.endS[gblk] = sc;
    }
    if (!last) __threadfence();                 // lane 63's row is read by every lane next
  }
  PassOut o;
  o.best = __shfl(best, lb);
  o.bestcol = __shfl(bestcol, lb);
  o.lastcol = __shfl(lastcol, lb);
  o.fin = __shfl(sc, lb);
  return o;
}

// Score of row r (0 <= r < m) from the block's end score and its Pv / Mv: the rows above the
// block's last row down to r + 1 are taken back.
__device__ __forceinline__ int row_score(const uint64_t P, const uint64_t M, const int end_score,
                                         const int r, const int m) {
  const int b = r >> 6;
  const int lastbit = (min(64 * (b + 1), m) - 1) & 63;
  const uint64_t upto = lastbit == 63 ? ~0ull : ((1ull << (lastbit + 1)) - 1);
  const uint64_t above = (r & 63) == 63 ? 0ull : (~0ull << ((r & 63) + 1));
  const uint64_t hi = above & upto;
  return end_score - __popcll(P & hi) + __popcll(M & hi);
}

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK)
void k_gfa_hw(const uint8_t *__restrict__ tigT, const uint8_t *__restrict__ tigC,
              const HwJob *__restrict__ jobs, const uint32_t n_jobs, HwOut *__restrict__ out,
              uint32_t *__restrict__ scratch, const uint64_t scratch_words) {
  __shared__ uint32_t s_row[WAVES_PER_BLOCK][LDS_WORDS];
  const int lane = threadIdx.x & 63;
  const int wave = uni((int)(threadIdx.x >> 6));
  const uint64_t gw = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave;
  const uint32_t n_waves = gridDim.x * WAVES_PER_BLOCK;
  uint32_t *grow = scratch ? scratch + gw * scratch_words : nullptr;
  const Keep none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  for (uint32_t e = (uint32_t)gw; e < n_jobs; e += n_waves) {
    const HwJob jb = jobs[e];
    const Ori q = ori_of(jb.q, tigT, tigC), t = ori_of(jb.t, tigT, tigC);
    const int m = uni(q.n), n = uni(t.n);
    const PassOut f = dp_pass(q.fwd(), t.fwd(), 0, INT_MIN, s_row[wave], grow, none);
    unsigned long long c = (unsigned long long)m * n;
    const int best = uni(f.best), end = uni(f.bestcol);
    HwOut o{-1, 0, 0, 0, 0};
    if (best <= uni(jb.k)) {
      o.dist = best;
      o.end = end;
      if (uni(jb.need_start)) {
        // the last column of the reversed prefix pass still at `best` is the longest alignment
        const PassOut r = dp_pass(q.bwd(), t.sub(0, end + 1).bwd(), 1, best, s_row[wave], grow, none);
        c += (unsigned long long)m * (end + 1);
        o.start = end - uni(r.lastcol);
      }
    }
    o.cells = c;
    if (lane == 0) out[e] = o;
  }
}

// ------------------------------------------------------------------ the path and its runs

struct RunState {            // the run still open, the same in every lane
  int cls;                   // 0 M, 1 I, 2 D; -1 before the first operation
  uint32_t cnt;
  uint32_t nruns;            // runs closed
  uint32_t total;            // operations seen
};

__device__ __forceinline__ uint32_t run_op(int cls) { return cls == 0 ? 'M' : cls == 1 ? 'I' : 'D'; }

// `count` operations in alignment order -- op_at(i) in every lane -- extend the open run or
// close it and open others.  A run is written when it is closed; slots past `cap` are counted
// and not written.
template <class OpAt>
__device__ void emit_runs(RunState &S, const int count, OpAt op_at, gfa_run *__restrict__ runs,
                          const uint32_t cap) {
  const int lane = threadIdx.x & 63;
  const uint64_t lt = (1ull << lane) - 1;
  for (int c0 = 0; c0 < count; c0 += 64) {
    const int cnt = min(64, count - c0);
    const bool valid = lane < cnt;
    const int op = valid ? op_at(c0 + lane) : OP_MATCH;
    const int cls = op == OP_INSERT ? 1 : (op == OP_DELETE ? 2 : 0);
    int prev = __shfl_up(cls, 1);
    if (lane == 0) prev = S.cls;
    const bool head = valid && cls != prev;
    const uint64_t hm = __ballot(head);
    if (!hm) { S.cnt += (uint32_t)cnt; continue; }
    const int first = __ffsll((unsigned long long)hm) - 1;
    const uint32_t pend = S.cnt + (uint32_t)first;
    uint32_t base = S.nruns;
    if (pend > 0) {
      if (lane == 0 && base < cap) runs[base] = gfa_run{pend, run_op(S.cls)};
      base++;
    }
    const uint64_t above = hm & ~lt & ~(1ull << lane);
    const int next = above ? __ffsll((unsigned long long)above) - 1 : cnt;
    const int nheads = __popcll(hm);
    const int idx = __popcll(hm & lt);
    if (head && idx < nheads - 1) {
      const uint32_t at = base + (uint32_t)idx;
      if (at < cap) runs[at] = gfa_run{(uint32_t)(next - lane), run_op(cls)};
    }
    const int lastl = 63 - __clzll((long long)hm);
    S.cls = __shfl(cls, lastl);
    S.cnt = (uint32_t)(cnt - lastl);
    S.nruns = base + (uint32_t)(nheads - 1);
  }
  S.total += (uint32_t)count;
}

struct PathScratch {
  uint64_t *colP, *colM;     // LEAF_ENTRIES each
  int *colS;
  uint64_t *endP, *endM;     // 2 * blocks each: the left pass, then the right pass
  int *endS;
  uint8_t *ops;              // a leaf's operations, last first
  uint32_t *grow;
};

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK)
void k_gfa_path(const uint8_t *__restrict__ tigT, const uint8_t *__restrict__ tigC,
                const NwJob *__restrict__ jobs, const uint32_t n_jobs, NwOut *__restrict__ out,
                gfa_run *__restrict__ runs_all,
                uint64_t *__restrict__ colP_all, uint64_t *__restrict__ colM_all,
                int *__restrict__ colS_all, uint64_t *__restrict__ endP_all,
                uint64_t *__restrict__ endM_all, int *__restrict__ endS_all,
                uint8_t *__restrict__ ops_all, uint32_t *__restrict__ grow_all,
                const uint32_t max_blocks, const uint64_t ops_bytes, const uint64_t grow_words) {
  __shared__ uint32_t s_row[WAVES_PER_BLOCK][LDS_WORDS];
  __shared__ int s_stack[WAVES_PER_BLOCK][STACK_DEPTH][5];
  const int lane = threadIdx.x & 63;
  const int wave = uni((int)(threadIdx.x >> 6));
  const uint64_t gw = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave;
  const uint32_t n_waves = gridDim.x * WAVES_PER_BLOCK;
  PathScratch W;
  W.colP = colP_all + gw * LEAF_ENTRIES;
  W.colM = colM_all + gw * LEAF_ENTRIES;
  W.colS = colS_all + gw * LEAF_ENTRIES;
  W.endP = endP_all + gw * 2 * max_blocks;
  W.endM = endM_all + gw * 2 * max_blocks;
  W.endS = endS_all + gw * 2 * max_blocks;
  W.ops = ops_all + gw * ops_bytes;
  W.grow = grow_words ? grow_all + gw * grow_words : nullptr;
  int (*stack)[5] = s_stack[wave];
  const Keep none{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};

  for (uint32_t e = (uint32_t)gw; e < n_jobs; e += n_waves) {
    const NwJob jb = jobs[e];
    const Ori Q = ori_of(jb.q, tigT, tigC), T = ori_of(jb.t, tigT, tigC);
    const int qlen = uni(Q.n), tlen = uni(T.n);
    gfa_run *runs = runs_all + jb.run_off;
    const uint32_t cap = jb.run_cap;
    unsigned long long c = (unsigned long long)qlen * tlen;
    const PassOut g = dp_pass(Q.fwd(), T.fwd(), 1, INT_MIN, s_row[wave], W.grow, none);
    const int dist = uni(g.fin);
    if (dist > uni(jb.k)) {
      if (lane == 0) out[e] = NwOut{-1, 0, 0, 0, 0, 0, c};
      continue;
    }
    RunState S{-1, 0, 0, 0};
    uint32_t nleaf = 0, nsplit = 0;

    int sp = 0;
    if (lane == 0) {
      stack[0][0] = 0; stack[0][1] = qlen; stack[0][2] = 0; stack[0][3] = tlen;
      stack[0][4] = dist;
    }
    sp = 1;
    __builtin_amdgcn_wave_barrier();
    while (sp > 0) {
      sp--;
      const int q0 = uni(stack[sp][0]), qn = uni(stack[sp][1]), t0 = uni(stack[sp][2]),
                tn = uni(stack[sp][3]), best = uni(stack[sp][4]);
      if (qn == 0 || tn == 0) {
        // an empty side: every remaining base is a DELETE (no query) or an INSERT (no target)
        const int op = qn == 0 ? OP_DELETE : OP_INSERT;
        emit_runs(S, qn + tn, [op](int) { return op; }, runs, cap);
        continue;
      }
      const int nb = (qn + 63) >> 6;
      const Ori q = Q.sub(q0, qn);
      if (20ll * nb * tn + 8ll * tn < (long long)GFA_LEAF_BYTES) {
        // a leaf: the whole matrix, then the walk from the corner
        nleaf++;
        c += (unsigned long long)qn * tn;
        const Keep k{W.colP, W.colM, W.colS, nullptr, nullptr, nullptr};
        (void)dp_pass(q.fwd(), T.sub(t0, tn).fwd(), 1, INT_MIN, s_row[wave], W.grow, k);
        __threadfence();
        // S(r, c) with the boundary row (c + 1) and column (r + 1)
        auto score = [&](int r, int cc) -> int {
          if (r < 0) return cc + 1;
          if (cc < 0) return r + 1;
          const size_t at = (size_t)(r >> 6) * (size_t)tn + (size_t)cc;
          return row_score(W.colP[at], W.colM[at], W.colS[at], r, qn);
        };
        int r = qn - 1, cc = tn - 1, nops = 0;
        int cur = best;
        while (r >= 0 && cc >= 0) {
          const int u = score(r - 1, cc), l = score(r, cc - 1), ul = score(r - 1, cc - 1);
          int op;
          if (u + 1 == cur) { op = OP_INSERT; r--; cur = u; }
          else if (l + 1 == cur) { op = OP_DELETE; cc--; cur = l; }
          else { op = ul == cur ? OP_MATCH : OP_MISMATCH; r--; cc--; cur = ul; }
          if (lane == 0) W.ops[nops] = (uint8_t)op;
          nops++;
        }
        // at a boundary the rest is flushed: the rows left are INSERTs, the columns DELETEs
        const int up = r + 1, left = cc + 1;
        for (int i = lane; i < up + left; i += 64)
          W.ops[nops + i] = (uint8_t)(up ? OP_INSERT : OP_DELETE);
        nops += up + left;
        __threadfence();
        const uint8_t *ops = W.ops;
        emit_runs(S, nops, [ops, nops](int i) { return (int)ops[nops - 1 - i]; }, runs, cap);
        __threadfence();                          // the buffer is reused by the next leaf
        continue;
      }
      // a split (obtainAlignmentHirschberg): the last column of the left half and of the
      // reversed right half, then the first row where the two meet at `best`
      nsplit++;
      c += (unsigned long long)qn * tn;
      const int lw = tn / 2, rw = tn - lw;
      const Keep kl{nullptr, nullptr, nullptr, W.endP, W.endM, W.endS};
      const Keep kr{nullptr, nullptr, nullptr, W.endP + max_blocks, W.endM + max_blocks,
                    W.endS + max_blocks};
      (void)dp_pass(q.fwd(), T.sub(t0, lw).fwd(), 1, INT_MIN, s_row[wave], W.grow, kl);
      (void)dp_pass(q.bwd(), T.sub(t0 + lw, rw).bwd(), 1, INT_MIN, s_row[wave], W.grow, kr);
      __threadfence();
      // L[r] = ED(q[0..r], left), R[r] = ED(q[r..], right) = the reversed pass at row qn-1-r
      auto Lrow = [&](int r) {
        return row_score(W.endP[r >> 6], W.endM[r >> 6], W.endS[r >> 6], r, qn);
      };
      auto Rrow = [&](int r) {
        const int x = qn - 1 - r;
        return row_score(W.endP[max_blocks + (x >> 6)], W.endM[max_blocks + (x >> 6)],
                         W.endS[max_blocks + (x >> 6)], x, qn);
      };
      int split = INT_MIN, ls = 0, rs = 0;
      for (int r0 = 0; r0 <= qn - 2 && split == INT_MIN; r0 += 64) {
        const int r = r0 + lane;
        int a = 0, b = 0;
        bool hit = false;
        if (r <= qn - 2) { a = Lrow(r); b = Rrow(r + 1); hit = a + b == best; }
        const uint64_t hm = __ballot(hit);
        if (hm) {
          const int first = __ffsll((unsigned long long)hm) - 1;
          split = r0 + first;
          ls = __shfl(a, first);
          rs = __shfl(b, first);
        }
      }
      if (split == INT_MIN) {
        const int r_top = uni(Rrow(0)), l_bot = uni(Lrow(qn - 1));
        if (lw + r_top == best) { split = -1; ls = lw; rs = r_top; }
        else if (l_bot + rw == best) { split = qn - 1; ls = l_bot; rs = rw; }
        else { split = qn - 1; ls = l_bot; rs = rw; }   // cannot happen: `best` is the distance
      }
      split = uni(split); ls = uni(ls); rs = uni(rs);
      if (sp + 2 <= STACK_DEPTH) {
        if (lane == 0) {
          stack[sp][0] = q0 + split + 1; stack[sp][1] = qn - (split + 1);
          stack[sp][2] = t0 + lw; stack[sp][3] = rw; stack[sp][4] = rs;
          stack[sp + 1][0] = q0; stack[sp + 1][1] = split + 1;
          stack[sp + 1][2] = t0; stack[sp + 1][3] = lw; stack[sp + 1][4] = ls;
        }
        sp += 2;
      }
      __builtin_amdgcn_wave_barrier();
      __threadfence_block();
    }
    if (S.cnt > 0) {
      if (lane == 0 && S.nruns < cap) runs[S.nruns] = gfa_run{S.cnt, run_op(S.cls)};
      S.nruns++;
    }
    if (lane == 0) out[e] = NwOut{dist, (int32_t)S.total, S.nruns, nleaf, nsplit, 0, c};
  }
}

}  // namespace

// ------------------------------------------------------------------ host

struct TigSet {
  uint32_t n = 0;
  bool loaded = false;
  std::vector<uint32_t> len;
  std::vector<uint64_t> off;
  DevBuf<uint8_t> d_codes;
};

struct gfa_ctx : capi::Device {
  gfa_params P{};
  TigSet sets[2];
  bool have_runs = false, have_tries = false;
  std::vector<gfa_run> runs;
  std::vector<gfa_try> tries;
  gfa_stats S{};
};

namespace {

int check_params(const gfa_params *p) {
  if (!p) return fail(GFA_ERR_BAD_PARAM, "null parameters");
  return GFA_OK;
}

uint32_t blocks_for(const gfa_ctx *c, uint64_t n_jobs) {
  const uint64_t want = (uint64_t)c->n_cu * 4 / WAVES_PER_BLOCK;
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_jobs + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, want));
}

// A span [bgn, end) of tig `id` as it is oriented (fwd: as loaded, else its reverse complement).
Span span_of(const TigSet &ts, int which, uint32_t id, bool fwd, int32_t bgn, int32_t end) {
  const int32_t len = (int32_t)ts.len[id];
  Span s;
  s.off = ts.off[id] + (uint64_t)(fwd ? bgn : len - end);
  s.n = end - bgn;
  s.flags = (fwd ? 0u : 1u) | (which == GFA_SET_C ? 2u : 0u);
  return s;
}

// One launch of k_gfa_hw over `jobs`; `out` gets their results.
int run_hw(gfa_ctx *c, const std::vector<HwJob> &jobs, std::vector<HwOut> &out, double &ms) {
  const uint32_t n = (uint32_t)jobs.size();
  out.resize(n);
  if (!n) return GFA_OK;
  uint32_t max_t = 1;
  for (const HwJob &j : jobs) max_t = std::max<uint32_t>(max_t, (uint32_t)j.t.n);
  const uint32_t blocks = blocks_for(c, n);
  const uint64_t waves = (uint64_t)blocks * WAVES_PER_BLOCK;
  const uint64_t grow_words = max_t > (uint32_t)LDS_COLUMNS ? ((uint64_t)max_t + 15) / 16 : 0;
  DevBuf<HwJob> d_jobs;
  DevBuf<HwOut> d_out;
  DevBuf<uint32_t> d_grow;
  HIP_TRY(d_jobs.alloc(n));
  HIP_TRY(d_out.alloc(n));
  HIP_TRY(d_grow.alloc(grow_words * waves));
  c->S.scratch_bytes = std::max<uint64_t>(c->S.scratch_bytes, d_jobs.bytes + d_out.bytes + d_grow.bytes);
  hipStream_t s = c->stream;
  Event e0, e1;
  HIP_TRY(e0.create());
  HIP_TRY(e1.create());
  HIP_TRY(hipMemcpyAsync(d_jobs.p, jobs.data(), n * sizeof(HwJob), hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(e0, s));
  hipLaunchKernelGGL(k_gfa_hw, dim3(blocks), dim3(64 * WAVES_PER_BLOCK), 0, s, c->sets[0].d_codes.p,
                     c->sets[1].d_codes.p, d_jobs.p, n, d_out.p, grow_words ? d_grow.p : nullptr,
                     grow_words);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e1, s));
  HIP_TRY(hipMemcpyAsync(out.data(), d_out.p, n * sizeof(HwOut), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  float t = 0;
  (void)hipEventElapsedTime(&t, e0, e1);
  ms += t;
  c->S.n_rounds++;
  c->S.n_alignments += n;
  for (uint32_t i = 0; i < n; i++) {
    c->S.dp_cells += out[i].cells;
    c->S.n_passes += 1 + (out[i].dist >= 0 && jobs[i].need_start ? 1 : 0);
  }
  return GFA_OK;
}

// One launch of k_gfa_path over `jobs`, whose runs take `total_runs` slots.
int run_path(gfa_ctx *c, const std::vector<NwJob> &jobs, uint64_t total_runs, std::vector<NwOut> &out,
             std::vector<gfa_run> &runs, double &ms) {
  const uint32_t n = (uint32_t)jobs.size();
  out.resize(n);
  runs.resize(total_runs);
  if (!n) return GFA_OK;
  uint32_t max_q = 1, max_t = 1;
  for (const NwJob &j : jobs) {
    max_q = std::max<uint32_t>(max_q, (uint32_t)j.q.n);
    max_t = std::max<uint32_t>(max_t, (uint32_t)j.t.n);
  }
  const uint32_t blocks = blocks_for(c, n);
  const uint64_t waves = (uint64_t)blocks * WAVES_PER_BLOCK;
  const uint32_t max_blocks = (max_q + 63) / 64 + 1;
  const uint64_t ops_bytes = ((uint64_t)max_q + max_t + 64 + 15) & ~15ull;
  const uint64_t grow_words = max_t > (uint32_t)LDS_COLUMNS ? ((uint64_t)max_t + 15) / 16 : 0;
  DevBuf<NwJob> d_jobs;
  DevBuf<NwOut> d_out;
  DevBuf<gfa_run> d_runs;
  DevBuf<uint64_t> d_colP, d_colM, d_endP, d_endM;
  DevBuf<int> d_colS, d_endS;
  DevBuf<uint8_t> d_ops;
  DevBuf<uint32_t> d_grow;
  HIP_TRY(d_jobs.alloc(n));
  HIP_TRY(d_out.alloc(n));
  HIP_TRY(d_runs.alloc(total_runs));
  HIP_TRY(d_colP.alloc((uint64_t)LEAF_ENTRIES * waves));
  HIP_TRY(d_colM.alloc((uint64_t)LEAF_ENTRIES * waves));
  HIP_TRY(d_colS.alloc((uint64_t)LEAF_ENTRIES * waves));
  HIP_TRY(d_endP.alloc(2ull * max_blocks * waves));
  HIP_TRY(d_endM.alloc(2ull * max_blocks * waves));
  HIP_TRY(d_endS.alloc(2ull * max_blocks * waves));
  HIP_TRY(d_ops.alloc(ops_bytes * waves));
  HIP_TRY(d_grow.alloc(grow_words * waves));
  uint64_t scratch = 0;
  for (size_t b : {d_jobs.bytes, d_out.bytes, d_runs.bytes, d_colP.bytes, d_colM.bytes, d_colS.bytes,
                   d_endP.bytes, d_endM.bytes, d_endS.bytes, d_ops.bytes, d_grow.bytes})
    scratch += b;
  c->S.scratch_bytes = std::max<uint64_t>(c->S.scratch_bytes, scratch);
  hipStream_t s = c->stream;
  Event e0, e1;
  HIP_TRY(e0.create());
  HIP_TRY(e1.create());
  HIP_TRY(hipMemcpyAsync(d_jobs.p, jobs.data(), n * sizeof(NwJob), hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(e0, s));
  hipLaunchKernelGGL(k_gfa_path, dim3(blocks), dim3(64 * WAVES_PER_BLOCK), 0, s, c->sets[0].d_codes.p,
                     c->sets[1].d_codes.p, d_jobs.p, n, d_out.p, d_runs.p, d_colP.p, d_colM.p,
                     d_colS.p, d_endP.p, d_endM.p, d_endS.p, d_ops.p, d_grow.p, max_blocks, ops_bytes,
                     grow_words);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e1, s));
  HIP_TRY(hipMemcpyAsync(out.data(), d_out.p, n * sizeof(NwOut), hipMemcpyDeviceToHost, s));
  if (total_runs)
    HIP_TRY(hipMemcpyAsync(runs.data(), d_runs.p, total_runs * sizeof(gfa_run), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  float t = 0;
  (void)hipEventElapsedTime(&t, e0, e1);
  ms += t;
  c->S.n_rounds++;
  c->S.n_alignments += n;
  for (uint32_t i = 0; i < n; i++) {
    if (out[i].n_runs > jobs[i].run_cap)
      return fail(GFA_ERR_HIP, "alignment %u made %u runs for %u slots", i, out[i].n_runs,
                  jobs[i].run_cap);
    c->S.dp_cells += out[i].cells;
    c->S.n_passes += 1 + out[i].n_leaf + 2ull * out[i].n_split;
    c->S.n_leaves += out[i].n_leaf;
    c->S.n_splits += out[i].n_split;
  }
  return GFA_OK;
}

int check_tig(const gfa_ctx *c, int which, uint32_t id, const char *what, uint64_t i) {
  const TigSet &ts = c->sets[which];
  if (id >= ts.n)
    return fail(GFA_ERR_BAD_INPUT, "%s %llu: tig %u is outside the %u tigs loaded", what,
                (unsigned long long)i, id, ts.n);
  if (ts.len[id] == 0)
    return fail(GFA_ERR_BAD_INPUT, "%s %llu: tig %u has no sequence", what, (unsigned long long)i, id);
  return GFA_OK;
}

// checkLink for links [first, last): the three launches.
int links_batch(gfa_ctx *c, const gfa_link *links, uint64_t first, uint64_t last,
                gfa_link_result *results) {
  const TigSet &ts = c->sets[GFA_SET_T];
  const uint32_t n = (uint32_t)(last - first);
  std::vector<HwJob> hw(n);
  std::vector<HwOut> ho;
  // extend B: the end of A in the begin of B
  for (uint32_t i = 0; i < n; i++) {
    const gfa_link &l = links[first + i];
    gfa_link_result &r = results[first + i];
    r = gfa_link_result{};
    r.a_len = (int32_t)ts.len[l.a_id];
    r.b_len = (int32_t)ts.len[l.b_id];
    r.max_edit = gfa_host::link_max_edit(l.align);
    r.abgn_b = gfa_host::link_abgn_b(r.a_len, l.a_align);
    r.bend_b = gfa_host::link_bend_b(r.b_len, l.b_align);
    hw[i].q = span_of(ts, GFA_SET_T, l.a_id, l.a_fwd != 0, r.abgn_b, r.a_len);
    hw[i].t = span_of(ts, GFA_SET_T, l.b_id, l.b_fwd != 0, 0, r.bend_b);
    hw[i].k = r.max_edit;
    hw[i].need_start = 0;
  }
  if (int rc = run_hw(c, hw, ho, c->S.ms_extend_b)) return rc;
  // extend A: that begin of B in the end of A
  for (uint32_t i = 0; i < n; i++) {
    const gfa_link &l = links[first + i];
    gfa_link_result &r = results[first + i];
    r.dist_b = ho[i].dist;
    r.bend = ho[i].dist >= 0 ? ho[i].end + 1 : r.bend_b;
    r.abgn_a = gfa_host::link_abgn_a(r.a_len, l.a_align);
    hw[i].q = span_of(ts, GFA_SET_T, l.b_id, l.b_fwd != 0, 0, r.bend);
    hw[i].t = span_of(ts, GFA_SET_T, l.a_id, l.a_fwd != 0, r.abgn_a, r.a_len);
    hw[i].k = r.max_edit;
    hw[i].need_start = 1;
  }
  if (int rc = run_hw(c, hw, ho, c->S.ms_extend_a)) return rc;
  // final: the two ends against each other, with the path
  std::vector<NwJob> nw(n);
  std::vector<NwOut> no;
  std::vector<gfa_run> runs;
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    const gfa_link &l = links[first + i];
    gfa_link_result &r = results[first + i];
    r.dist_a = ho[i].dist;
    r.abgn = ho[i].dist >= 0 ? r.abgn_a + ho[i].start : r.abgn_a;
    nw[i].q = span_of(ts, GFA_SET_T, l.a_id, l.a_fwd != 0, r.abgn, r.a_len);
    nw[i].t = span_of(ts, GFA_SET_T, l.b_id, l.b_fwd != 0, 0, r.bend);
    nw[i].k = 2 * r.max_edit;
    // a path of distance d has at most d runs of I or D and one more of M than that, and no
    // more runs than operations
    nw[i].run_cap = (uint32_t)std::min<uint64_t>(2ull * (uint64_t)nw[i].k + 1,
                                                 (uint64_t)nw[i].q.n + (uint64_t)nw[i].t.n);
    nw[i].run_off = total;
    total += nw[i].run_cap;
  }
  if (int rc = run_path(c, nw, total, no, runs, c->S.ms_final)) return rc;
  for (uint32_t i = 0; i < n; i++) {
    gfa_link_result &r = results[first + i];
    r.dist_f = no[i].dist;
    r.success = no[i].dist >= 0;
    r.align_len = no[i].align_len;
    r.n_runs = no[i].n_runs;
    r.run_off = c->runs.size();
    r.n_leaves = no[i].n_leaf;
    r.n_splits = no[i].n_split;
    c->runs.insert(c->runs.end(), runs.begin() + nw[i].run_off, runs.begin() + nw[i].run_off + no[i].n_runs);
  }
  c->S.n_batches++;
  return GFA_OK;
}

struct Call {                // one checkRecord_align
  uint32_t record, kind;
  Span b;                    // what is aligned
  uint32_t a_id;
  int32_t a_len, b_len;
  int32_t abgn, aend, max_edit, step;
  bool open, success;
  std::vector<gfa_try> tries;
};

int records_batch(gfa_ctx *c, const gfa_record *records, uint64_t first, uint64_t last,
                  gfa_record_result *results) {
  const TigSet &T = c->sets[GFA_SET_T], &C = c->sets[GFA_SET_C];
  std::vector<Call> calls;
  auto add = [&](uint64_t i, uint32_t kind, int32_t o, int32_t blen, int32_t abgn, int32_t aend) {
    const gfa_record &r = records[i];
    Call k{};
    k.record = (uint32_t)i;
    k.kind = kind;
    k.b = span_of(T, GFA_SET_T, r.b_id, r.b_fwd != 0, o, o + blen);
    k.a_id = r.a_id;
    k.a_len = (int32_t)C.len[r.a_id];
    k.b_len = blen;
    k.max_edit = gfa_host::rec_max_edit(blen);
    k.step = gfa_host::rec_step(blen);
    k.abgn = abgn;
    k.aend = aend;
    gfa_host::rec_window(k.a_len, blen, k.step, k.abgn, k.aend);
    k.open = true;
    calls.push_back(std::move(k));
  };
  for (uint64_t i = first; i < last; i++) {
    const gfa_record &r = records[i];
    const int32_t blen = (int32_t)T.len[r.b_id];
    if (blen < GFA_END_BASES) {
      add(i, GFA_CALL_ALL, 0, blen, r.bgn, r.end);
    } else {
      add(i, GFA_CALL_LEFT, 0, GFA_END_BASES, r.bgn, r.bgn + GFA_END_BASES);
      add(i, GFA_CALL_RIGHT, blen - GFA_END_BASES, GFA_END_BASES, r.end - GFA_END_BASES, r.end);
    }
  }
  std::vector<HwJob> hw;
  std::vector<HwOut> ho;
  std::vector<size_t> who;
  while (true) {
    hw.clear();
    who.clear();
    for (size_t k = 0; k < calls.size(); k++) {
      const Call &K = calls[k];
      if (!K.open) continue;
      HwJob j;
      j.q = K.b;
      j.t = span_of(C, GFA_SET_C, K.a_id, true, K.abgn, K.aend);
      j.k = K.max_edit;
      j.need_start = 1;
      hw.push_back(j);
      who.push_back(k);
    }
    if (hw.empty()) break;
    if (int rc = run_hw(c, hw, ho, c->S.ms_records)) return rc;
    for (size_t x = 0; x < who.size(); x++) {
      Call &K = calls[who[x]];
      gfa_try t{};
      t.record = K.record;
      t.call = K.kind;
      t.b_len = K.b_len;
      t.abgn = K.abgn;
      t.aend = K.aend;
      t.max_edit = K.max_edit;
      t.dist = ho[x].dist;
      if (ho[x].dist >= 0) {
        t.nbgn = K.abgn + ho[x].start;
        t.nend = K.abgn + ho[x].end + 1;
        if (gfa_host::rec_accept(K.abgn, K.aend, t.nbgn, t.nend, K.a_len)) {
          t.outcome = GFA_TRY_ACCEPT;
          K.abgn = t.nbgn;
          K.aend = t.nend;
          K.open = false;
          K.success = true;
        } else {
          t.outcome = GFA_TRY_EXTEND;
          if (K.abgn == t.nbgn) K.abgn = std::max(K.abgn - K.step, 0);
          if (K.aend == t.nend) K.aend = std::min(K.aend + K.step, K.a_len);
        }
      } else if (gfa_host::rec_can_relax(K.abgn, K.aend, K.b_len, K.max_edit)) {
        t.outcome = GFA_TRY_RELAX;
        K.abgn = std::max(K.abgn - K.step, 0);
        K.aend = std::min(K.aend + K.step, K.a_len);
        K.max_edit = gfa_host::rec_relax(K.max_edit);
      } else {
        t.outcome = GFA_TRY_ABORT;
        K.open = false;
      }
      K.tries.push_back(t);
    }
  }
  size_t k = 0;
  for (uint64_t i = first; i < last; i++) {
    gfa_record_result &r = results[i];
    r = gfa_record_result{};
    r.try_off = c->tries.size();
    bool ok = true;
    int32_t bgn = records[i].bgn, end = records[i].end;
    const size_t k0 = k;
    for (; k < calls.size() && calls[k].record == (uint32_t)i; k++) {
      ok = ok && calls[k].success;
      c->tries.insert(c->tries.end(), calls[k].tries.begin(), calls[k].tries.end());
    }
    if (ok) {
      bgn = calls[k0].abgn;          // ALL's, or LEFT's begin and RIGHT's end
      end = calls[k - 1].aend;
    }
    r.success = ok;
    r.bgn = bgn;
    r.end = end;
    r.n_tries = (uint32_t)(c->tries.size() - r.try_off);
  }
  c->S.n_batches++;
  return GFA_OK;
}

}  // namespace

extern "C" {

void gfa_params_init(gfa_params *p) {
  if (!p) return;
  p->hbm_budget = 0;
}

const char *gfa_last_error(void) { return capi::g_err.c_str(); }
int gfa_abi_version(void) { return GFA_ABI_VERSION; }

int gfa_ctx_create(const gfa_params *p, int device, gfa_ctx **out) {
  if (!out) return fail(GFA_ERR_BAD_PARAM, "null out");
  *out = nullptr;
  if (int rc = check_params(p)) return rc;
  return capi::create_ctx(p, device, out);
}

void gfa_ctx_destroy(gfa_ctx *c) { capi::destroy_ctx(c); }

int gfa_set_params(gfa_ctx *c, const gfa_params *p) {
  if (!c) return fail(GFA_ERR_BAD_PARAM, "null context");
  if (int rc = check_params(p)) return rc;
  c->P = *p;
  return GFA_OK;
}

int gfa_load_tigs(gfa_ctx *c, int which, uint32_t n, const uint8_t *bases, const uint64_t *offsets,
                  const uint32_t *lengths) {
  if (!c) return fail(GFA_ERR_BAD_PARAM, "null context");
  if (which != GFA_SET_T && which != GFA_SET_C)
    return fail(GFA_ERR_BAD_PARAM, "tig set %d is neither GFA_SET_T nor GFA_SET_C", which);
  TigSet &ts = c->sets[which];
  ts.d_codes.release();
  ts.n = 0;
  ts.loaded = false;
  ts.len.clear();
  ts.off.clear();
  c->have_runs = c->have_tries = false;
  std::vector<uint64_t> off(n);
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (lengths && lengths[i] > GFA_MAX_TIGLEN)
      return fail(GFA_ERR_UNSUPPORTED, "tig %u is %u bases, beyond %u", i, lengths[i],
                  (unsigned)GFA_MAX_TIGLEN);
    off[i] = total;
    total += lengths ? lengths[i] : 0;
  }
  DevBuf<uint8_t> d_b;
  DevBuf<uint64_t> d_o, d_off;
  DevBuf<uint32_t> bad, d_len;
  if (int rc = capi::stage_reads(c->device, n, bases, offsets, lengths, d_b, d_o)) return rc;
  HIP_TRY(bad.alloc(1));
  HIP_TRY(d_len.alloc(n));
  HIP_TRY(d_off.alloc(n));
  HIP_TRY(ts.d_codes.alloc(total));
  HIP_TRY(hipMemsetAsync(bad.p, 0, 4, c->stream));
  uint32_t h_bad = 0;
  if (n) {
    HIP_TRY(hipMemcpyAsync(d_off.p, off.data(), n * 8ull, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_len.p, lengths, n * 4ull, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_gfa_encode, dim3(std::min<uint32_t>(n, 4096)), dim3(256), 0, c->stream, d_b.p,
                       d_o.p, d_off.p, d_len.p, n, ts.d_codes.p, bad.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (h_bad) {
    ts.d_codes.release();
    return fail(GFA_ERR_BAD_INPUT, "a tig holds a byte outside ACGTN");
  }
  ts.n = n;
  ts.loaded = true;
  ts.len.assign(lengths, lengths + n);
  ts.off = off;
  return GFA_OK;
}

int gfa_check_links(gfa_ctx *c, const gfa_link *links, uint64_t n, gfa_link_result *results) {
  if (!c) return fail(GFA_ERR_BAD_PARAM, "null context");
  if (n && (!links || !results)) return fail(GFA_ERR_BAD_PARAM, "null links or results");
  if (n > 0xfffffff0ull) return fail(GFA_ERR_BAD_PARAM, "more than 2^32 links in one call");
  if (!c->sets[GFA_SET_T].loaded) return fail(GFA_ERR_STATE, "no tigs: call gfa_load_tigs first");
  HIP_TRY(hipSetDevice(c->device));
  c->have_runs = false;
  c->runs.clear();
  c->S = gfa_stats{};
  // the checks the reference leaves to its assertions
  for (uint64_t i = 0; i < n; i++) {
    const gfa_link &l = links[i];
    if (int rc = check_tig(c, GFA_SET_T, l.a_id, "link", i)) return rc;
    if (int rc = check_tig(c, GFA_SET_T, l.b_id, "link", i)) return rc;
    if (l.a_align <= 0 || l.b_align <= 0 || l.align < 0)
      return fail(GFA_ERR_BAD_INPUT, "link %llu: an alignment of %d and %d bases (%d columns) "
                  "leaves nothing to align", (unsigned long long)i, l.a_align, l.b_align, l.align);
  }
  c->S.n_links = n;
  const uint64_t budget = c->P.hbm_budget ? c->P.hbm_budget : (4ull << 30);
  uint64_t i = 0;
  while (i < n) {
    const uint64_t first = i;
    uint64_t need = 0;
    for (; i < n; i++) {
      const uint64_t cap = 4ull * (uint64_t)gfa_host::link_max_edit(links[i].align) + 1;
      const uint64_t mine = cap * sizeof(gfa_run) + sizeof(NwJob) + sizeof(NwOut) + sizeof(HwJob) +
                            sizeof(HwOut);
      if (i > first && need + mine > budget) break;
      need += mine;
    }
    if (int rc = links_batch(c, links, first, i, results)) return rc;
  }
  c->have_runs = true;
  return GFA_OK;
}

int gfa_runs_size(const gfa_ctx *c, uint64_t *n_runs) {
  if (!c || !n_runs) return fail(GFA_ERR_BAD_PARAM, "null argument");
  if (!c->have_runs) return fail(GFA_ERR_STATE, "no result: call gfa_check_links first");
  *n_runs = c->runs.size();
  return GFA_OK;
}

int gfa_fetch_runs(const gfa_ctx *c, gfa_run *runs) {
  if (!c) return fail(GFA_ERR_BAD_PARAM, "null context");
  if (!c->have_runs) return fail(GFA_ERR_STATE, "no result: call gfa_check_links first");
  if (runs && !c->runs.empty()) memcpy(runs, c->runs.data(), c->runs.size() * sizeof(gfa_run));
  return GFA_OK;
}

int gfa_check_records(gfa_ctx *c, const gfa_record *records, uint64_t n, gfa_record_result *results) {
  if (!c) return fail(GFA_ERR_BAD_PARAM, "null context");
  if (n && (!records || !results)) return fail(GFA_ERR_BAD_PARAM, "null records or results");
  if (n > 0x7ffffff0ull) return fail(GFA_ERR_BAD_PARAM, "more than 2^31 records in one call");
  if (!c->sets[GFA_SET_T].loaded || !c->sets[GFA_SET_C].loaded)
    return fail(GFA_ERR_STATE, "no tigs: call gfa_load_tigs for both sets first");
  HIP_TRY(hipSetDevice(c->device));
  c->have_tries = false;
  c->tries.clear();
  c->S = gfa_stats{};
  for (uint64_t i = 0; i < n; i++) {
    const gfa_record &r = records[i];
    if (int rc = check_tig(c, GFA_SET_C, r.a_id, "record", i)) return rc;
    if (int rc = check_tig(c, GFA_SET_T, r.b_id, "record", i)) return rc;
    const int64_t alen = c->sets[GFA_SET_C].len[r.a_id];
    if (r.bgn < 0 || r.end < r.bgn || (int64_t)r.end > alen)
      return fail(GFA_ERR_BAD_INPUT, "record %llu: %d-%d is outside contig %u of %lld bases",
                  (unsigned long long)i, r.bgn, r.end, r.a_id, (long long)alen);
  }
  c->S.n_records = n;
  const uint64_t budget = c->P.hbm_budget ? c->P.hbm_budget : (4ull << 30);
  const uint64_t per = 2 * (sizeof(HwJob) + sizeof(HwOut));
  const uint64_t step = std::max<uint64_t>(1, budget / per);
  for (uint64_t i = 0; i < n; i += step)
    if (int rc = records_batch(c, records, i, std::min(n, i + step), results)) return rc;
  c->have_tries = true;
  return GFA_OK;
}

int gfa_tries_size(const gfa_ctx *c, uint64_t *n_tries) {
  if (!c || !n_tries) return fail(GFA_ERR_BAD_PARAM, "null argument");
  if (!c->have_tries) return fail(GFA_ERR_STATE, "no result: call gfa_check_records first");
  *n_tries = c->tries.size();
  return GFA_OK;
}

int gfa_fetch_tries(const gfa_ctx *c, gfa_try *tries) {
  if (!c) return fail(GFA_ERR_BAD_PARAM, "null context");
  if (!c->have_tries) return fail(GFA_ERR_STATE, "no result: call gfa_check_records first");
  if (tries && !c->tries.empty()) memcpy(tries, c->tries.data(), c->tries.size() * sizeof(gfa_try));
  return GFA_OK;
}

int gfa_get_stats(const gfa_ctx *c, gfa_stats *out) {
  if (!c || !out) return fail(GFA_ERR_BAD_PARAM, "null argument");
  *out = c->S;
  return GFA_OK;
}

}  // extern "C"
