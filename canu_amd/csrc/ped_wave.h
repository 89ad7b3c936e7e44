// ped_wave.h -- Prefix_Edit_Dist and Compute_Delta by one wave, for k_fe_align (fe.hip) and
// k_co_align (co.hip).
//
// findErrors-Prefix_Edit_Distance.C and correctOverlaps-Prefix_Edit_Distance.C are the same
// aligner but for two places: what a row must pass to become the Max_Score cell (the Accept
// functor of ped_rows) and where the traceback starts (the callers choose what they hand to
// ped_delta).  Line numbers below are "fe" for the first file and "co" for the second.
//
// Reads are 2 bits per base.  A row of the edit array lives with lanes as diagonals: lane
// (d & 63) holds diagonal d, so the band may drift without moving registers, and the two
// neighbours come by one DPP wave rotate each.  The slide compares 32 bases per step (xor of two
// 64-bit windows, count of trailing zeros).  A row wider than PED_WINDOW_DIAGS is computed in
// chunks of 64 that read the row before from the row log.  Every row goes to the wave's row log
// in global memory (the traceback needs them all); only its pruned band is ever read again, and
// a read outside that band is the reference's -2.
//
// Everything here is inlined into its kernel: k_fe_align sits at exactly 64 VGPRs for its eighth
// wave per SIMD, which a call boundary would cost.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ped {

constexpr int PED_WINDOW_DIAGS = 64;   // a lane holds a diagonal
constexpr int PAD_WORDS = 3;           // a 32-base window may start at the last base
// words of one LDS strand: a span keeps its bit offset in its first word (up to 15 bases) and
// a 32-base window may start at its last base (PAD_WORDS)
constexpr int lds_strand_words(int lds_bases) { return (lds_bases + 15) / 16 + 4; }

// ------------------------------------------------------------------ wave helpers

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ int from_lower(int v) {   // lane l <- v[(l - 1) & 63]
  return __builtin_amdgcn_update_dpp(0, v, 0x13C, 0xf, 0xf, false);
}
__device__ __forceinline__ int from_upper(int v) {   // lane l <- v[(l + 1) & 63]
  return __builtin_amdgcn_update_dpp(0, v, 0x134, 0xf, 0xf, false);
}

__device__ __forceinline__ int wave_max(int v) {
  const int NEG = (int)0x80000000;
  int t;
  t = __builtin_amdgcn_update_dpp(NEG, v, 0x111, 0xf, 0xf, false); v = v > t ? v : t;
  t = __builtin_amdgcn_update_dpp(NEG, v, 0x112, 0xf, 0xf, false); v = v > t ? v : t;
  t = __builtin_amdgcn_update_dpp(NEG, v, 0x114, 0xf, 0xf, false); v = v > t ? v : t;
  t = __builtin_amdgcn_update_dpp(NEG, v, 0x118, 0xf, 0xf, false); v = v > t ? v : t;
  t = __builtin_amdgcn_update_dpp(NEG, v, 0x142, 0xa, 0xf, false); v = v > t ? v : t;
  t = __builtin_amdgcn_update_dpp(NEG, v, 0x143, 0xc, 0xf, false); v = v > t ? v : t;
  return __builtin_amdgcn_readlane(v, 63);
}

// bit k of the result is bit ((k + s) & 63) of mask: lanes in diagonal order from `left`
__device__ __forceinline__ uint64_t rot_to(uint64_t mask, int left) {
  const int s = left & 63;
  return s ? (mask >> s) | (mask << (64 - s)) : mask;
}

__device__ __forceinline__ void wave_fence() { __threadfence_block(); }

__device__ __forceinline__ uint64_t fetch32(const uint32_t *P, int pos) {
  const uint32_t *w = P + (pos >> 4);
  const int s = (pos & 15) * 2;
  const uint64_t lo = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
  uint64_t x = lo >> s;
  if (s) x |= (uint64_t)w[2] << (64 - s);
  return x;
}

__device__ __forceinline__ int code_at(const uint32_t *P, int pos) {
  return (P[pos >> 4] >> ((pos & 15) * 2)) & 3;
}

// The inner while of Prefix_Edit_Dist (fe :226-227, co :227-228) from (row, row + d).
__device__ __forceinline__ int slide(const uint32_t *A, int ab, const uint32_t *B, int bb, int row,
                                     int d, int m, int n) {
  const int rem = min(m - row, n - (row + d));
  int adv = 0;
  while (adv < rem) {
    const uint64_t x = fetch32(A, ab + row + adv) ^ fetch32(B, bb + row + d + adv);
    if (x) {
      adv += __builtin_ctzll(x) >> 1;
      break;
    }
    adv += 32;
  }
  return row + min(adv, rem);
}

struct RowMeta { int off, lo, hi; };   // value of (e, d) at log[off + d] for lo <= d <= hi, else -2

__device__ __forceinline__ int row_get(const int32_t *log, const RowMeta M, int d) {
  return (d >= M.lo && d <= M.hi) ? log[M.off + d] : -2;
}

__device__ __forceinline__ int block_scan_incl(int v, int *lds, int &total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int s = 1; s < 64; s <<= 1) {
    const int t = __shfl_up(v, s);
    if (lane >= s) v += t;
  }
  __syncthreads();
  if (lane == 63) lds[w] = v;
  __syncthreads();
  int add = 0, tot = 0;
  for (int k = 0; k < (int)(blockDim.x >> 6); k++) {
    if (k < w) add += lds[k];
    tot += lds[k];
  }
  total = tot;
  return v + add;
}

// The next job of a queue the waves share: lane 0 takes it, every lane gets it.  The wave barrier
// (no instruction) keeps the compiler from threading lane 0's branch at the end of one job into
// this one: that splits the job loop in two with lane 0 on the outer one, and the other lanes
// then read "the first lane's" slot without it, for ever.
__device__ __forceinline__ uint32_t next_job(uint32_t *next, int lane) {
  __builtin_amdgcn_wave_barrier();
  uint32_t slot = 0;
  if (lane == 0) slot = atomicAdd(next, 1u);
  return (uint32_t)uni((int)slot);
}

// ------------------------------------------------------------------ the aligner

// The two spans the aligner reads, A from base `as` and B from base `bb`: copied to the wave's
// LDS strands `la` and `lb` where both fit LDS_BASES, else left where they lie.  True if staged;
// the pointers and offsets then name the strands.
template <int LDS_BASES>
__device__ __forceinline__ bool ped_stage(const uint32_t *&As, int &as, const uint32_t *&B, int &bb,
                                          int m, int n, int limit, uint32_t *la, uint32_t *lb,
                                          int lane) {
  // A row never passes min(m, n - d) and |d| <= limit: what lies beyond is never read
  const int ma = min(m, n + limit), nb = min(n, m + limit);
  const bool fits = max(ma, nb) <= LDS_BASES;
  if (fits) {
    const int wa = ((as & 15) + ma) / 16 + PAD_WORDS, wb = ((bb & 15) + nb) / 16 + PAD_WORDS;
    for (int i = lane; i < wa; i += 64) la[i] = As[(as >> 4) + i];
    for (int i = lane; i < wb; i += 64) lb[i] = B[(bb >> 4) + i];
    wave_fence();
    As = la; as &= 15;
    B = lb; bb &= 15;
  }
  return fits;
}

struct PedRows {
  bool aborted;                  // the row log is full: nothing else holds
  bool ended;                    // a row reached the end of A or of B, at (end_e, end_d, end_row)
  int end_e, end_d, end_row;
  int ms_len, ms_d, ms_e;        // the Max_Score cell, for an alignment that did not end
  uint32_t nrows;
  bool generic;                  // a row was wider than the window (F_GENERIC)
};

// Prefix_Edit_Dist's rows (fe :166-309, co :165-312) of A[as, as + m) against B[bb, bb + n) with
// up to `limit` errors.  Row e goes to log[meta[3e] + d] for meta[3e + 1] <= d <= meta[3e + 2];
// the log holds log_cap values.  accept(score, max_score, longest, best_d, best_e) says whether
// a row with a higher score becomes the Max_Score cell.
template <class Accept>
__device__ __forceinline__ PedRows ped_rows(const uint32_t *As, int as, const uint32_t *B, int bb,
                                            int m, int n, int limit, const int32_t *match_limit,
                                            int32_t *log, int32_t *meta, uint64_t log_cap, int lane,
                                            Accept accept) {
  PedRows R{};
  const int row0 = uni(slide(As, as, B, bb, 0, 0, m, n));
  if (row0 == min(m, n)) {                                   // fe :195-200, co :196-201
    R.ended = true;
    R.end_row = row0;
    return R;
  }
  if (lane == 0) { log[0] = row0; meta[0] = 0; meta[1] = 0; meta[2] = 0; }
  RowMeta PM{0, 0, 0};                                       // the row before
  uint64_t logpos = 1;
  int left = 0, right = 0;
  int best_d = 0, best_e = 0, longest = 0;
  double max_score = 0.0;
  int pv = lane == 0 ? row0 : -2;                            // row e-1 at this lane's diagonal
  bool pv_valid = true;

  for (int e = 1; e <= limit; e++) {
    left = max(left - 1, -e);
    right = min(right + 1, e);
    const int width = right - left + 1;
    if (logpos + (uint64_t)width > log_cap) { R.aborted = true; break; }
    const int off = (int)logpos - left;
    const int lim = match_limit[e];
    R.nrows++;
    wave_fence();                                            // row e-1 and its meta are written
    int new_left, new_right, row_max = 0, row_max_d = 0;
    bool hit = false;
    int hit_d = 0, hit_row = 0;

    if (width <= PED_WINDOW_DIAGS) {
      const int d = left + ((lane - left) & 63);
      const bool active = d <= right;
      if (!pv_valid) pv = row_get(log, PM, d);
      const int lo_n = from_lower(pv), up_n = from_upper(pv);
      int row = max(max(1 + pv, lo_n), up_n + 1);
      if (active) {
        row = slide(As, as, B, bb, row, d, m, n);
        log[off + d] = row;
      } else {
        row = -2;
      }
      const uint64_t em = rot_to(__ballot(active && (row == m || row + d == n)), left);
      if (em) {
        hit = true;
        hit_d = left + __builtin_ctzll(em);
        hit_row = __builtin_amdgcn_readlane(row, hit_d & 63);
      } else {
        const bool keep = active && ((d < 0 ? row : row + d) >= lim);   // fe :253-271, co :257-275
        const uint64_t km = rot_to(__ballot(keep), left);
        if (km == 0) {
          new_left = right + 1;
          new_right = right;
        } else {
          new_left = left + __builtin_ctzll(km);
          new_right = left + 63 - __builtin_clzll(km);
          const bool in = active && d >= new_left && d <= new_right;
          row_max = wave_max(in ? row : -2);
          row_max_d = left + __builtin_ctzll(rot_to(__ballot(in && row == row_max), left));
          pv = in ? row : -2;
          pv_valid = true;
        }
      }
    } else {
      R.generic = true;
      pv_valid = false;
      const int nchunk = (width + 63) >> 6;
      // One pass: the pruning (fe :253-271, co :257-275) and the leftmost maximum of the pruned
      // band (fe :275-280, co :279-284) are kept from the ballots of the computing pass.  `com`
      // is the maximum over [new_left, new_right] so far, `pen` over what lies right of
      // new_right and joins the band only if a later diagonal holds the limit.
      new_left = right + 1;
      new_right = right;
      bool any = false;
      int com_max = -2, com_d = 0, pen_max = -2, pen_d = 0;
      for (int c = 0; c < nchunk && !hit; c++) {
        const int base = left + c * 64;
        const int d = base + lane;
        const bool active = d <= right;
        int row = -2;
        if (active) {
          row = max(max(1 + row_get(log, PM, d), row_get(log, PM, d - 1)),
                    row_get(log, PM, d + 1) + 1);
          row = slide(As, as, B, bb, row, d, m, n);
          log[off + d] = row;
        }
        const uint64_t em = __ballot(active && (row == m || row + d == n));
        if (em) {
          hit = true;
          const int l = __builtin_ctzll(em);
          hit_d = base + l;
          hit_row = __builtin_amdgcn_readlane(row, l);
          break;
        }
        const uint64_t km = __ballot(active && ((d < 0 ? row : row + d) >= lim));
        if (km) {
          const int fk = __builtin_ctzll(km), lk = 63 - __builtin_clzll(km);
          const bool in1 = active && lane >= (any ? 0 : fk) && lane <= lk;
          const int mx1 = wave_max(in1 ? row : -2);
          const int d1 = base + __builtin_ctzll(__ballot(in1 && row == mx1));
          if (pen_max > com_max) { com_max = pen_max; com_d = pen_d; }   // strictly: leftmost
          if (mx1 > com_max) { com_max = mx1; com_d = d1; }
          if (!any) new_left = base + fk;
          any = true;
          new_right = base + lk;
          const bool in2 = active && lane > lk;
          pen_max = -2;
          if (__ballot(in2)) {
            pen_max = wave_max(in2 ? row : -2);
            pen_d = base + __builtin_ctzll(__ballot(in2 && row == pen_max));
          }
        } else if (any) {
          const int mx = wave_max(active ? row : -2);
          if (mx > pen_max) {
            pen_max = mx;
            pen_d = base + __builtin_ctzll(__ballot(active && row == mx));
          }
        }
      }
      row_max = com_max;
      row_max_d = com_d;
    }

    if (hit) {                                               // fe :233-250, co :236-254
      if (hit_row == m && 1 + row_get(log, PM, hit_d + 1) == hit_row && hit_d < right)
        hit_d++;                                             // the last error is a mismatch
      R.ended = true;
      R.end_e = e;
      R.end_d = hit_d;
      R.end_row = hit_row;
      break;
    }
    left = new_left;
    right = new_right;
    if (lane == 0) { meta[3 * e] = off; meta[3 * e + 1] = left; meta[3 * e + 2] = right; }
    PM = RowMeta{off, left, right};
    logpos += (uint64_t)width;
    if (left > right) break;
    if (row_max > longest) {                                 // fe :275-280, co :279-284
      best_d = row_max_d;
      best_e = e;
      longest = row_max;
    }
    const int score = (int)((double)longest * 0.272 - (double)e);   // fe :282, co :286; truncated
    if (accept(score, max_score, longest, best_d, best_e)) {        // fe :289-290, co :292
      max_score = (double)score;
      R.ms_len = longest;
      R.ms_d = best_d;
      R.ms_e = best_e;
    }
  }
  return R;
}

// Compute_Delta (fe :30-76, co :30-75) from row `row` of diagonal d with e errors, through the
// rows ped_rows logged; every lane walks the same path, lane 0 writes the stack.  Leaves the
// delta in `delta` and returns its length.  With e == 0 no row is read and the length is 0.
__device__ __forceinline__ int ped_delta(const int32_t *log, const int32_t *meta, int32_t *stk,
                                         int32_t *delta, int e, int d, int row, int lane) {
  wave_fence();
  int last = row, sl = 0;
  for (int k = e; k > 0; k--) {
    const RowMeta M{meta[3 * (k - 1)], meta[3 * (k - 1) + 1], meta[3 * (k - 1) + 2]};
    int from = d;
    int mx = 1 + row_get(log, M, d);
    int j = row_get(log, M, d - 1);
    if (j > mx) { from = d - 1; mx = j; }
    j = 1 + row_get(log, M, d + 1);
    if (j > mx) { from = d + 1; mx = j; }
    if (from == d - 1) {
      if (lane == 0) stk[sl] = mx - last - 1;
      sl++;
      d--;
      last = row_get(log, M, from);
    } else if (from == d + 1) {
      if (lane == 0) stk[sl] = last - (mx - 1);
      sl++;
      d++;
      last = row_get(log, M, from);
    }
  }
  if (lane == 0) stk[sl] = last + 1;
  sl++;
  wave_fence();
  const int delta_len = sl - 1;
  for (int k = lane; k < delta_len; k += 64) {
    const int i = sl - 1 - k;
    const int v = stk[i], s = stk[i - 1];
    delta[k] = abs(v) * ((s > 0) - (s < 0));
  }
  wave_fence();
  return delta_len;
}

}  // namespace ped
