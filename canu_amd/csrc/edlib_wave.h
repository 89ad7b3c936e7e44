// edlib_wave.h -- edlib's edit distance, location and path by one wave, for k_pair (pair.hip),
// k_fs_locate / k_fs_path (fs.hip) and k_gfa_hw / k_gfa_path (gfa.hip).
//
// The DP is Myers' bit-vector recurrence (Myers 1999; the block step of edlib.C:276-330).
// Lane b holds Pv/Mv of query rows 64b..64b+63 and the match masks of those rows, one per
// symbol.  Columns run as a skewed wavefront: at step s lane b does column s-b and takes the
// horizontal delta and the target base of that column from lane b-1 (one DPP wave_shr:1 of a
// packed word).  Lane 0 gets its base from a 64-column chunk of the target that the wave loads
// coalesced and keeps in a register (v_readlane by the step), and its delta from the top
// boundary (0 infix, +1 prefix/global) or, for a query of more than STRIPE_ROWS rows, from the
// boundary row the previous stripe's last lane left: 2 bits per column, in LDS for targets up
// to LDS_COLUMNS, else in a per-wave global scratch row.
//
//   dp_pass       one pass: the bottom row's minimum, its first column, the last column at a
//                 wanted score and the corner; with a Keep, Pv / Mv / score of every block
//                 column (a leaf) or of the last column (a split) as well.
//   wave_locate   EDLIB_MODE_HW / EDLIB_TASK_LOC in closed form: an infix pass gives the
//                 distance and the first best end column; a prefix pass of the reversed query
//                 over the reversed target up to that column gives the longest start
//                 (edlib.C:216-236).
//   wave_path     obtainAlignment's recursion with an explicit stack in LDS.  A split runs the
//                 left half and the reversed right half, keeps Pv / Mv and the end score of
//                 every 64-row block of the two last columns, and takes the first row r with
//                 L[r] + R[r+1] == best as a wave-wide first match, then the two boundary
//                 rules.  A leaf keeps every column -- under the leaf-byte limit by the leaf
//                 rule, so the scratch of a wave is fixed -- and walks up / left / diagonal
//                 from the corner.  The operations (one byte each, a leaf's backwards through a
//                 per-wave buffer) go to the caller's sink in alignment order.
//
// A sequence is anything with n and at(i); a span is anything with n, sub(o, len), fwd() and
// bwd(), the last two sequences.  Everything here is inlined into its kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "edlib_host.h"

namespace edw {

enum : int { OP_MATCH = 0, OP_INSERT = 1, OP_DELETE = 2, OP_MISMATCH = 3 };   // EDLIB_EDOP_*
// symbols: 0..3 = ACGT, N, the NUL reverseComplementCopy makes of N (it equals only itself),
// and what lies beyond a sequence's end
enum : int { CODE_N = 4, CODE_NUL = 5, CODE_PAD = 7 };

// ------------------------------------------------------------------ read encoding

// fwd gets the codes of every read; rc, where it is given, those of its reverse complement
// at the same offsets.  A byte outside ACGTN sets *bad.
static __global__ void k_encode(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ src_off,
                                const uint64_t *__restrict__ dst_off, const uint32_t *__restrict__ len,
                                uint32_t nreads, uint8_t *__restrict__ fwd, uint8_t *__restrict__ rc,
                                uint32_t *__restrict__ bad) {
  for (uint32_t r = blockIdx.x; r < nreads; r += gridDim.x) {
    const uint8_t *s = bases + src_off[r];
    const uint64_t d = dst_off[r];
    const uint32_t L = len[r];
    for (uint32_t i = threadIdx.x; i < L; i += blockDim.x) {
      const uint8_t ch = s[i];
      uint8_t c = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : CODE_N;
      if (c == CODE_N && ch != 'N') atomicOr(bad, 1u);
      fwd[d + i] = c;
      if (rc) rc[d + (L - 1 - i)] = c < 4 ? (uint8_t)(3 - c) : c;
    }
  }
}

// ------------------------------------------------------------------ the pass

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ int dpp_from_lower(int v, int lane0) {   // lane l <- v[l-1]
  return __builtin_amdgcn_update_dpp(lane0, v, 0x138, 0xf, 0xf, false);
}

struct Seq {                 // bases in memory, read forwards or backwards
  const uint8_t *p;
  int n;
  int rev;                   // element i is p[n-1-i]
  __device__ __forceinline__ int at(int i) const { return p[rev ? n - 1 - i : i]; }
};

struct Span {                // a stretch of an oriented read
  const uint8_t *p;
  int n;
  __device__ __forceinline__ Seq fwd() const { return Seq{p, n, 0}; }
  __device__ __forceinline__ Seq bwd() const { return Seq{p, n, 1}; }
  __device__ __forceinline__ Span sub(int o, int len) const { return Span{p + o, len}; }
};

struct PassOut {
  int best, bestcol;         // minimum of the bottom row, the first column attaining it
  int lastcol;               // last column whose bottom-row score == want (-1: none)
  int fin;                   // bottom-row score at the last column
  unsigned long long steps;  // wavefront steps: columns + lanes - 1 per stripe
};

// What a pass leaves behind besides its bottom row.  Block g is rows 64g..64g+63.
struct Keep {
  static constexpr bool on = true;
  uint64_t *colP, *colM;     // leaf: Pv / Mv of block g after column j at [g * n + j]
  int *colS;                 //       and the score of the block's last row there
  uint64_t *endP, *endM;     // split: Pv / Mv of block g after the last column at [g]
  int *endS;                 //        and the score of the block's last row there
};

struct NoKeep {              // nothing: the stores are compiled away
  static constexpr bool on = false;
};

// Bottom row of the edit-distance matrix of q (rows) against t (columns) over NSYM symbols (5,
// or 6 with NUL); top_hin 0 lets an alignment start at any column (infix), 1 charges every
// skipped target base (prefix, global).  Needs q.n >= 1, t.n >= 1.  Every lane of the wave is
// in, with the same arguments.
template <int NSYM, class SeqQ, class SeqT, class K>
__device__ PassOut dp_pass(const SeqQ q, const SeqT t, const int top_hin, const int want,
                           uint32_t *lrow, uint32_t *grow, const K keep) {
  static_assert(NSYM == 5 || NSYM == 6, "ACGTN, or ACGTN and NUL");
  const int lane = threadIdx.x & 63;
  const int m = q.n, n = t.n;
  const int nstripes = (m + STRIPE_ROWS - 1) / STRIPE_ROWS;
  const bool use_g = n > LDS_COLUMNS;
  int best = INT_MAX, bestcol = -1, lastcol = -1, sc = m;
  int lb = 0;
  unsigned long long steps = 0;
  for (int st = 0; st < nstripes; st++) {
    const int r0 = st * STRIPE_ROWS;
    const int rows = min(STRIPE_ROWS, m - r0);
    const int nb = (rows + 63) >> 6;
    const bool last = st == nstripes - 1;
    lb = nb - 1;
    // match masks: block c's 64 bases are loaded by the wave and balloted per symbol
    uint64_t pe0 = 0, pe1 = 0, pe2 = 0, pe3 = 0, pe4 = 0, pe5 = 0;
    for (int c = 0; c < nb; c++) {
      const int i = r0 + c * 64 + lane;
      const int code = i < m ? q.at(i) : CODE_PAD;
      const uint64_t b0 = __ballot(code == 0), b1 = __ballot(code == 1),
                     b2 = __ballot(code == 2), b3 = __ballot(code == 3),
                     b4 = __ballot(code == CODE_N);
      if (lane == c) { pe0 = b0; pe1 = b1; pe2 = b2; pe3 = b3; pe4 = b4; }
      if constexpr (NSYM == 6) {
        const uint64_t b5 = __ballot(code == CODE_NUL);
        if (lane == c) pe5 = b5;
      }
    }
    uint64_t Pv = ~0ull, Mv = 0;
    const bool trk = last && lane == lb;
    // the last row of this lane's block, whose score the lane follows along the columns (the
    // boundary column holds row + 1).  It is bit 63 but in the pass's last block, whose lane
    // hands its delta to nobody: one bit serves the score and the lane above.
    const int lrow_abs = min(r0 + 64 * (lane + 1), m) - 1;
    const int rr = lane < nb ? (lrow_abs & 63) : 63;
    sc = lrow_abs + 1;
    const size_t gblk = (size_t)(st * 64 + lane);
    int x = 1;                                  // (hout + 1) | base << 2, handed to lane + 1
    uint32_t cur = lane < n ? (uint32_t)t.at(lane) : (uint32_t)CODE_PAD;
    uint32_t nxt = 64 + lane < n ? (uint32_t)t.at(64 + lane) : (uint32_t)CODE_PAD;
    uint32_t hw = 0, acc = 0;
    const int nsteps = n + nb - 1;
    steps += (unsigned long long)nsteps;
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
        // the symbol's match mask by bit selects (a chain of ?: compiles to branches)
        const uint64_t s0 = 0 - (uint64_t)(b & 1), s1 = 0 - (uint64_t)((b >> 1) & 1),
                       s2 = 0 - (uint64_t)(b >> 2);
        const uint64_t e01 = (pe0 & ~s0) | (pe1 & s0), e23 = (pe2 & ~s0) | (pe3 & s0);
        const uint64_t e03 = (e01 & ~s1) | (e23 & s1);
        uint64_t e45 = pe4;
        if constexpr (NSYM == 6) e45 = (pe4 & ~s0) | (pe5 & s0);
        uint64_t Eq = (e03 & ~s2) | (e45 & s2);
        const uint64_t neg = hin < 0 ? 1ull : 0ull, pos = hin > 0 ? 1ull : 0ull;
        const uint64_t Xv = Eq | Mv;
        Eq |= neg;
        const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        uint64_t Ph = Mv | ~(Xh | Pv);
        uint64_t Mh = Pv & Xh;
        d = (int)((Ph >> rr) & 1) - (int)((Mh >> rr) & 1);
        Ph = (Ph << 1) | pos;
        Mh = (Mh << 1) | neg;
        Pv = Mh | ~(Xv | Ph);
        Mv = Ph & Xv;
        sc += d;
        if (trk) {
          if (sc < best) { best = sc; bestcol = j; }
          if (sc == want) lastcol = j;
        }
        if constexpr (K::on) {
          if (keep.colP) {
            const size_t at = gblk * (size_t)n + (size_t)j;
            keep.colP[at] = Pv;
            keep.colM[at] = Mv;
            keep.colS[at] = sc;
          }
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
    if constexpr (K::on) {
      if (keep.endP && lane < nb) {
        keep.endP[gblk] = Pv;
        keep.endM[gblk] = Mv;
        keep.endS[gblk] = sc;
      }
    }
    if (!last) __threadfence();                 // lane 63's row is read by every lane next
  }
  PassOut o;
  o.best = __shfl(best, lb);
  o.bestcol = __shfl(bestcol, lb);
  o.lastcol = __shfl(lastcol, lb);
  o.fin = __shfl(sc, lb);
  o.steps = steps;
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

// ------------------------------------------------------------------ the location

struct Located {
  int dist;                  // the distance, whatever k
  int ok;                    // dist <= k
  int start, end;            // with ok: the first best end column and, if asked for, the start
  unsigned long long cells, steps;
  uint32_t passes;
};

// q in t, anywhere, within k.  Every value is the same in every lane.
template <int NSYM, class SpanQ, class SpanT>
__device__ Located wave_locate(const SpanQ q, const SpanT t, const int k, const bool need_start,
                               uint32_t *lrow, uint32_t *grow) {
  const int m = q.n;
  const PassOut f = dp_pass<NSYM>(q.fwd(), t.fwd(), 0, INT_MIN, lrow, grow, NoKeep{});
  Located o{uni(f.best), 0, 0, uni(f.bestcol), (unsigned long long)m * t.n, f.steps, 1};
  o.ok = o.dist <= k;
  if (o.ok && need_start) {
    // the last column of the reversed prefix pass still at the distance is the longest alignment
    const PassOut r = dp_pass<NSYM>(q.bwd(), t.sub(0, o.end + 1).bwd(), 1, o.dist, lrow, grow, NoKeep{});
    o.cells += (unsigned long long)m * (o.end + 1);
    o.steps += r.steps;
    o.passes++;
    o.start = o.end - uni(r.lastcol);
  }
  return o;
}

// ------------------------------------------------------------------ the path

struct PathScratch {         // of one wave
  uint64_t *colP, *colM;     // a leaf's block columns
  int *colS;
  uint64_t *endP, *endM;     // 2 * max_blocks each: the left pass, then the right pass
  int *endS;
  uint8_t *ops;              // a leaf's operations, last first
  uint32_t *grow;
  uint32_t max_blocks;
};

struct PathArgs {            // of every wave, as a kernel takes it (PathBuffers, edlib_launch.h)
  uint64_t *colP, *colM;
  int *colS;
  uint64_t *endP, *endM;
  int *endS;
  uint8_t *ops;
  uint32_t *grow;
  PathSize Z;
  __device__ __forceinline__ PathScratch wave(const uint64_t gw) const {
    return PathScratch{colP + gw * Z.leaf_entries, colM + gw * Z.leaf_entries,
                       colS + gw * Z.leaf_entries, endP + gw * 2 * Z.max_blocks,
                       endM + gw * 2 * Z.max_blocks, endS + gw * 2 * Z.max_blocks,
                       ops + gw * Z.ops_bytes, Z.grow_words ? grow + gw * Z.grow_words : nullptr,
                       Z.max_blocks};
  }
};

struct PathStats {
  unsigned long long cells;
  uint32_t nleaf, nsplit;
};

// The operations of the global alignment of Q and T, whose distance is dist, in alignment
// order: sink(count, op_at) gets them a stretch at a time, op_at(i) in every lane.  stack is
// the wave's STACK_DEPTH rows of LDS, lrow its boundary row.
template <int NSYM, class SpanQ, class SpanT, class Sink>
__device__ PathStats wave_path(const SpanQ Q, const SpanT T, const int dist, const PathScratch W,
                               uint32_t *lrow, int (*stack)[5], const long long leaf_bytes,
                               Sink sink) {
  const int lane = threadIdx.x & 63;
  const uint32_t max_blocks = W.max_blocks;
  PathStats N{0, 0, 0};
  int sp = 0;
  if (lane == 0) {
    stack[0][0] = 0; stack[0][1] = Q.n; stack[0][2] = 0; stack[0][3] = T.n;
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
      sink(qn + tn, [op](int) { return op; });
      continue;
    }
    const SpanQ q = Q.sub(q0, qn);
    if (is_leaf(qn, tn, leaf_bytes)) {
      // a leaf: the whole matrix, then the walk from the corner
      N.nleaf++;
      N.cells += (unsigned long long)qn * tn;
      const Keep k{W.colP, W.colM, W.colS, nullptr, nullptr, nullptr};
      (void)dp_pass<NSYM>(q.fwd(), T.sub(t0, tn).fwd(), 1, INT_MIN, lrow, W.grow, k);
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
      sink(nops, [ops, nops](int i) { return (int)ops[nops - 1 - i]; });
      __threadfence();                          // the buffer is reused by the next leaf
      continue;
    }
    // a split (obtainAlignmentHirschberg): the last column of the left half and of the
    // reversed right half, then the first row where the two meet at `best`
    N.nsplit++;
    N.cells += (unsigned long long)qn * tn;
    const int lw = tn / 2, rw = tn - lw;
    const Keep kl{nullptr, nullptr, nullptr, W.endP, W.endM, W.endS};
    const Keep kr{nullptr, nullptr, nullptr, W.endP + max_blocks, W.endM + max_blocks,
                  W.endS + max_blocks};
    (void)dp_pass<NSYM>(q.fwd(), T.sub(t0, lw).fwd(), 1, INT_MIN, lrow, W.grow, kl);
    (void)dp_pass<NSYM>(q.bwd(), T.sub(t0 + lw, rw).bwd(), 1, INT_MIN, lrow, W.grow, kr);
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
  return N;
}

}  // namespace edw
