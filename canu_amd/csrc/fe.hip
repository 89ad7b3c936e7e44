// fe.hip -- libcanu_fe.so: canu's findErrors (src/overlapErrorAdjustment/findErrors*.C) on gfx950.
//
// k_fe_align: one wave owns one overlap and runs Process_Olap on the device -- Prefix_Edit_Dist
// (findErrors-Prefix_Edit_Distance.C:166-309), Compute_Delta (:30-76), the rescue rule and the
// error test (findErrors-Process_Olap.C:149-163), then Analyze_Alignment's votes
// (findErrors-Analyze_Alignment.C:100-293) -- so nothing goes back to the host per overlap.
//
// Reads are 2 bits per base (every byte outside ACGTacgt is 'a'), forward and reverse
// complemented.  The aligner is ped_wave.h's, shared with k_co_align: lanes as diagonals, a
// register window of FE_WINDOW_DIAGS diagonals with the row log in global memory behind it.
// Spans of up to FE_LDS_BASES bases are staged in the wave's LDS strands first; longer ones are
// fetched from global memory.  What is findErrors' own is the second clause of the Max_Score
// test and the traceback from the Max_Score cell when no row reaches an end.
//
// Tallies are 32-bit counters per base (44 bytes per base of the range): the nine point votes by
// atomicAdd, `confirmed` and `no_insert` as difference pairs (+1 at the start of a run, -1 past
// its end) that k_fe_decide prefix-sums; every count is clamped to 255 when it is read, which
// is what a saturating increment leaves for any number of votes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/canu_fe.h"
#include "capi_common.h"
#include "ped_launch.h"
#include "ped_wave.h"

namespace {

using namespace ped;
using capi::fail;

CAPI_SAME_CODES(FE);
static_assert(FE_WINDOW_DIAGS == PED_WINDOW_DIAGS, "canu_fe.h names the aligner's window");
constexpr int MAX_VOTE = 255, MAX_DEGREE = 32767;     // findErrors.H:87-90
constexpr int MIN_HAPLO_OCCURS = 3;                   // findErrors.H:102
constexpr int NPLANES = 11;
// Vote_Value_t (correctionOutput.H:24-37) and the tally plane of each vote
enum { V_IDENT = 0, V_DELETE = 1, V_A_SUBST = 2, V_T_SUBST = 5, V_A_INSERT = 6 };
enum { PL_CONFIRMED = 0, PL_DELETES = 1, PL_SUBST = 2, PL_NO_INSERT = 6, PL_INSERT = 7 };
// per-overlap outcome, with ped_host.h's
enum : uint32_t { F_PASSED = 1, F_FAILED = 2 };
constexpr int LDS_STRAND_WORDS = lds_strand_words(FE_LDS_BASES);

struct Job {                 // one overlap, as Process_Olap sets it up (:72-119)
  uint64_t a_word, b_word;   // first packed word of A (forward) and of B (as oriented)
  uint64_t tally;            // first tally slot of the A read
  int32_t a_off, b_off;      // a_offset, b_offset
  int32_t m, n;              // a_part_len, b_part_len
  int32_t clear_len;         // the A read's length
  int32_t limit;             // Error_Bound[min(m, n)]
  uint32_t b_rc;             // B comes from the reverse-complement array
  uint32_t pad;
};

struct AlignArgs {
  const uint32_t *fwd, *rc;          // packed reads
  const Job *jobs;
  const uint32_t *order;             // longest first
  uint32_t njobs, nwaves;            // waves that own scratch
  uint32_t *next;                    // work counter
  uint32_t *flags, *rows;            // per overlap
  int32_t *tallies;                  // NPLANES planes of `plane` slots
  uint64_t plane;
  const int32_t *match_limit;        // Edit_Match_Limit[e]
  int32_t *scratch;                  // per wave: log, meta, stack/delta, changes
  uint64_t log_cap, per_wave;        // ints
  int32_t max_limit;
  double erate;
  int32_t kmer_len, vote_qualify_len, end_exclude_len;
};

__device__ __forceinline__ int error_bound(int i, double erate) {   // findErrors.C:476-477
  return (int)ceil((double)i * erate);
}

// ------------------------------------------------------------------ the aligner and the votes

// Eight waves per SIMD (64 VGPRs): the kernel waits on the row log, and on the utg benchmark the
// bound is worth more than the SGPRs it keeps in VGPR lanes (unbounded: 89 VGPRs, five waves,
// 23.6 ms; six waves 21.1 ms; eight 17.8 ms).
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, 8) void k_fe_align(const AlignArgs X) {
  __shared__ uint32_t s_strand[WAVES_PER_BLOCK][2][LDS_STRAND_WORDS];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
  if (wave >= X.nwaves) return;
  int32_t *const log = X.scratch + (uint64_t)wave * X.per_wave;
  int32_t *const meta = log + X.log_cap;                       // 3 per row
  int32_t *const stk = meta + 3 * (uint64_t)(X.max_limit + 2); // deltaStack
  int32_t *const delta = stk + (X.max_limit + 4);
  int32_t *const chg = delta + (X.max_limit + 4);              // 2 per change
  const int chg_cap = X.max_limit + 8;

  for (;;) {
    const uint32_t slot = next_job(X.next, lane);
    if (slot >= X.njobs) break;
    const uint32_t oi = X.order[slot];
    const Job J = X.jobs[oi];
    const uint32_t *const A = X.fwd + J.a_word;           // the whole A read: the votes' bases
    const int m = J.m, n = J.n, ab = J.a_off;
    const int shorter = min(m, n);
    // the two spans the aligner reads
    const uint32_t *As = A, *B = (J.b_rc ? X.rc : X.fwd) + J.b_word;
    int as = ab, bb = J.b_off;
    uint32_t flags = 0;
    if (ped_stage<FE_LDS_BASES>(As, as, B, bb, m, n, J.limit, s_strand[threadIdx.x >> 6][0],
                                s_strand[threadIdx.x >> 6][1], lane))
      flags |= F_STAGED;

    const double erate = X.erate;
    const PedRows R = ped_rows(
        As, as, B, bb, m, n, J.limit, X.match_limit, log, meta, X.log_cap, lane,
        [erate](int score, double max_score, int longest, int best_d, int best_e) {
          return (double)score > max_score &&
                 best_e <= error_bound(min(longest, longest + best_d), erate);
        });
    if (R.generic) flags |= F_GENERIC;
    if (R.aborted) {
      if (lane == 0) { X.flags[oi] = F_OVERFLOW | flags; X.rows[oi] = R.nrows; }
      continue;
    }
    // the alignment to the end, or else the one to the Max_Score cell (:298-308)
    bool to_end = R.ended;
    int errors, a_end, b_end;
    if (to_end) { errors = R.end_e; a_end = R.end_row; b_end = R.end_row + R.end_d; }
    else { errors = R.ms_e; a_end = R.ms_len; b_end = R.ms_len + R.ms_d; }
    const int delta_len = ped_delta(log, meta, stk, delta, errors, b_end - a_end, a_end, lane);

    int olap_len = shorter;
    if (!to_end && a_end + ab >= J.clear_len - 1) {            // Process_Olap :149-152
      olap_len = min(a_end, b_end);
      to_end = true;
    }
    const bool passed = errors <= error_bound(olap_len, X.erate) && to_end;
    flags |= passed ? F_PASSED : F_FAILED;

    if (passed) {
      // Analyze_Alignment :109-221: the list of changes, in alignment order
      const int a_len = a_end;
      int ct = 1, i = 0, j = 0, p = 0;
      bool bad = false;
      if (lane == 0) { chg[0] = -1; chg[1] = (int)(((uint32_t)-1 << 4) | V_A_SUBST); }
      for (int k = 0; k <= delta_len && !bad; k++) {
        const int dl = k < delta_len ? delta[k] : 0;
        const int L = k < delta_len ? abs(dl) - 1 : a_len - i;
        for (int t0 = 0; t0 < L; t0 += 64) {
          const int t = t0 + lane;
          int bc = 0;
          bool mis = false;
          if (t < L) {
            bc = code_at(B, bb + j + t);
            mis = code_at(As, as + i + t) != bc;
          }
          const uint64_t mm = __ballot(mis);
          if (mm) {
            const int cnt = __builtin_popcountll(mm);
            if (ct + cnt + 2 > chg_cap) { bad = true; break; }
            if (mis) {
              const int at = ct + __builtin_popcountll(mm & ((1ull << lane) - 1));
              chg[2 * at] = i + t;
              chg[2 * at + 1] = ((p + t) << 4) | (V_A_SUBST + bc);
            }
            ct += cnt;
          }
        }
        if (L > 0) { i += L; j += L; p += L; }
        if (k < delta_len) {
          if (ct + 3 > chg_cap) { bad = true; break; }
          if (dl < 0) {
            if (lane == 0) {
              chg[2 * ct] = i - 1;
              chg[2 * ct + 1] = (p << 4) | (V_A_INSERT + code_at(B, bb + j));
            }
            ct++; j++; p++;
          } else if (dl > 0) {
            if (lane == 0) { chg[2 * ct] = i; chg[2 * ct + 1] = (p << 4) | V_DELETE; }
            ct++; i++; p++;
          }
        }
      }
      if (bad) {
        flags = (flags & ~(uint32_t)(F_PASSED | F_FAILED)) | F_INTERNAL;
      } else {
        if (lane == 0) { chg[2 * ct] = i; chg[2 * ct + 1] = p << 4; }
        wave_fence();
        // :239-292, one change per lane
        int32_t *const T = X.tallies + J.tally;
        const int K = X.kmer_len, V = X.vote_qualify_len, XL = X.end_exclude_len;
        for (int c = 1 + lane; c <= ct; c += 64) {
          const int f0 = chg[2 * (c - 1)], w0 = chg[2 * (c - 1) + 1];
          const int f1 = chg[2 * c], w1 = chg[2 * c + 1];
          const int prev_match = (w1 >> 4) - (w0 >> 4) - 1;
          const int p_lo = c == 1 ? 0 : XL;
          const int p_hi = c == ct ? prev_match : prev_match - XL;
          if (prev_match >= K) {
            for (int pass = 0; pass < 2; pass++) {
              const int q0 = pass ? p_hi : 0, q1 = pass ? prev_match : p_lo;
              for (int q = q0; q < q1; q++) {
                const int k = ab + f0 + q + 1;
                if (k >= 0 && k < J.clear_len)
                  atomicAdd(T + (uint64_t)(PL_SUBST + code_at(A, k)) * X.plane + k, 1);
              }
            }
            if (p_hi > p_lo) {
              const int k0 = ab + f0 + p_lo + 1, k1 = ab + f0 + p_hi + 1;
              atomicAdd(T + (uint64_t)PL_CONFIRMED * X.plane + k0, 1);
              atomicAdd(T + (uint64_t)PL_CONFIRMED * X.plane + k1, -1);
              if (k1 - 1 > k0) {
                atomicAdd(T + (uint64_t)PL_NO_INSERT * X.plane + k0, 1);
                atomicAdd(T + (uint64_t)PL_NO_INSERT * X.plane + k1 - 1, -1);
              }
            }
          }
          const int v0 = w0 & 15, v1 = w1 & 15;
          if (c < ct && (prev_match > 0 || v0 <= V_T_SUBST || v1 <= V_T_SUBST)) {
            const int w2 = chg[2 * (c + 1) + 1];
            const int next_match = (w2 >> 4) - (w1 >> 4) - 1;
            const int fs = ab + f1;
            // :282 compares with the aligned length of a_part, not the read's: kept
            if (!(fs < 0 || fs >= a_len) && prev_match + next_match >= V) {
              const int plane = v1 == V_DELETE ? PL_DELETES : v1 <= V_T_SUBST ? v1 : v1 + 1;
              atomicAdd(T + (uint64_t)plane * X.plane + fs, 1);
            }
          }
        }
      }
    }
    if (lane == 0) { X.flags[oi] = flags; X.rows[oi] = R.nrows; }
  }
}

// ------------------------------------------------------------------ the decision

struct DecideArgs {
  int32_t *tallies;
  uint64_t plane;
  const uint64_t *tally_off;       // per read of the range
  const uint64_t *word_off;        // packed words of the same reads
  const uint32_t *len;
  const uint32_t *keep;            // keep_left | keep_right << 1
  const uint32_t *fwd;
  uint32_t bgn_id, nreads;
  int32_t use_haplo_ct;
  uint32_t *count;                 // pass 0: records per read (without IDENT)
  const uint64_t *rec_off;         // pass 1: first record of each read
  fe_correction *out;
};

// Pass 0 prefix-sums the two difference planes, runs the two ladders of Output_Corrections
// (findErrors-Output.C:76-230) per base, leaves `sub | ins << 4` (0: no record) in the
// confirmed plane and counts; pass 1 writes the records behind each read's IDENT record.
template <int PASS>
__global__ __launch_bounds__(256) void k_fe_decide(const DecideArgs X) {
  __shared__ int lds[8];
  for (uint32_t r = blockIdx.x; r < X.nreads; r += gridDim.x) {
    int32_t *const T = X.tallies + X.tally_off[r];
    const int L = (int)X.len[r];
    const uint32_t keep = X.keep[r];
    if (PASS == 0) {
      const uint32_t *A = X.fwd + X.word_off[r];
      int carry_c = 0, carry_n = 0, nrec = 0;
      for (int j0 = 0; j0 < L; j0 += 256) {
        const int j = j0 + (int)threadIdx.x;
        const bool in = j < L;
        int tc, tn;
        const int sc = block_scan_incl(in ? T[(uint64_t)PL_CONFIRMED * X.plane + j] : 0, lds, tc);
        const int sn = block_scan_incl(in ? T[(uint64_t)PL_NO_INSERT * X.plane + j] : 0, lds, tn);
        int code = 0;
        if (in) {
          int t[NPLANES];
          for (int k = 0; k < NPLANES; k++) t[k] = min(T[(uint64_t)k * X.plane + j], MAX_VOTE);
          t[PL_CONFIRMED] = min(carry_c + sc, MAX_VOTE);
          t[PL_NO_INSERT] = min(carry_n + sn, MAX_VOTE);
          bool go_on = true;
          if (t[PL_CONFIRMED] < 2) {
            int vote = V_DELETE, mx = t[PL_DELETES];
            bool is_change = true;
            const int base = code_at(A, j);
            for (int k = 0; k < 4; k++)
              if (t[PL_SUBST + k] > mx) { vote = V_A_SUBST + k; mx = t[PL_SUBST + k]; is_change = base != k; }
            int haplo = t[PL_DELETES] >= MIN_HAPLO_OCCURS, total = t[PL_DELETES];
            for (int k = 0; k < 4; k++) { haplo += t[PL_SUBST + k] >= MIN_HAPLO_OCCURS; total += t[PL_SUBST + k]; }
            // the reference's skip tests `continue` past the insert test as well
            if (total <= 1 || 2 * mx <= total || !is_change || (haplo >= 2 && X.use_haplo_ct) ||
                (t[PL_CONFIRMED] > 0 && (t[PL_CONFIRMED] != 1 || mx <= 6)))
              go_on = false;
            else
              code = vote;
          }
          if (go_on && t[PL_NO_INSERT] < 2) {
            int ins = V_A_INSERT, imx = t[PL_INSERT];
            for (int k = 1; k < 4; k++)
              if (imx < t[PL_INSERT + k]) { ins = V_A_INSERT + k; imx = t[PL_INSERT + k]; }
            int ihap = 0, itot = 0;
            for (int k = 0; k < 4; k++) { ihap += t[PL_INSERT + k] >= MIN_HAPLO_OCCURS; itot += t[PL_INSERT + k]; }
            if (!(itot <= 1 || 2 * imx >= itot || (ihap >= 2 && X.use_haplo_ct) ||
                  (t[PL_NO_INSERT] > 0 && (t[PL_NO_INSERT] != 1 || imx <= 6))))
              code |= ins << 4;
          }
          T[(uint64_t)PL_CONFIRMED * X.plane + j] = code;
        }
        carry_c += tc;
        carry_n += tn;
        int tr;
        block_scan_incl(((code & 15) != 0) + ((code >> 4) != 0), lds, tr);
        nrec += tr;
      }
      if (threadIdx.x == 0) X.count[r] = (uint32_t)nrec;
    } else {
      uint64_t at = X.rec_off[r];
      if (threadIdx.x == 0) X.out[at] = fe_correction{keep, X.bgn_id + r};
      at++;
      for (int j0 = 0; j0 < L; j0 += 256) {
        const int j = j0 + (int)threadIdx.x;
        const int code = j < L ? T[(uint64_t)PL_CONFIRMED * X.plane + j] : 0;
        const int n = ((code & 15) != 0) + ((code >> 4) != 0);
        int tot;
        const int incl = block_scan_incl(n, lds, tot);
        uint64_t w = at + (uint64_t)(incl - n);
        if (code & 15)
          X.out[w++] = fe_correction{keep | ((uint32_t)(code & 15) << 2) | ((uint32_t)j << 6),
                                     X.bgn_id + r};
        if (code >> 4)
          X.out[w] = fe_correction{keep | ((uint32_t)(code >> 4) << 2) | ((uint32_t)j << 6),
                                   X.bgn_id + r};
        at += (uint64_t)tot;
      }
    }
  }
}

int check_params(const fe_params *p) {
  if (!p) return fail(FE_ERR_BAD_PARAM, "null parameters");
  if (!(p->error_rate >= 0.0 && p->error_rate < 1.0))
    return fail(FE_ERR_BAD_PARAM, "error_rate %g outside [0, 1)", p->error_rate);
  if (p->kmer_len < 1 || p->vote_qualify_len < 0 || p->end_exclude_len < 0 ||
      p->degree_threshold < 0)
    return fail(FE_ERR_BAD_PARAM, "kmer_len %d, vote_qualify_len %d, end_exclude_len %d or "
                "degree_threshold %d out of range", p->kmer_len, p->vote_qualify_len,
                p->end_exclude_len, p->degree_threshold);
  return FE_OK;
}

}  // namespace

struct fe_ctx : capi::Device {
  fe_params P;
  PackedReads reads;                 // forward and reverse complement
  MatchLimit ml;
  std::vector<fe_correction> out;
  fe_stats S{};
};

extern "C" {

void fe_params_init(fe_params *p) {
  if (!p) return;
  p->error_rate = 0.06;          // findErrors.H:324-336
  p->degree_threshold = 2;
  p->kmer_len = 9;
  p->vote_qualify_len = 9;
  p->end_exclude_len = 3;
  p->use_haplo_ct = 1;
}

const char *fe_last_error(void) { return capi::g_err.c_str(); }
int fe_abi_version(void) { return FE_ABI_VERSION; }

int fe_ctx_create(const fe_params *p, int device, fe_ctx **out) {
  if (!out) return fail(FE_ERR_BAD_PARAM, "null out");
  *out = nullptr;
  if (int rc = check_params(p)) return rc;
  return capi::create_ctx(p, device, out);
}

void fe_ctx_destroy(fe_ctx *c) { capi::destroy_ctx(c); }

int fe_set_params(fe_ctx *c, const fe_params *p) {
  if (!c) return fail(FE_ERR_BAD_PARAM, "null context");
  if (int rc = check_params(p)) return rc;
  c->P = *p;
  return FE_OK;
}

int fe_load_reads_device(fe_ctx *c, uint32_t first_iid, uint32_t nreads, const uint8_t *d_bases,
                         const uint64_t *d_offsets, const uint32_t *h_lengths) {
  if (!c) return fail(FE_ERR_BAD_PARAM, "null context");
  if (int rc = capi::check_device_reads(first_iid, nreads, d_bases, d_offsets, h_lengths)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  return pack_reads<true>(c->reads, c->stream, PAD_WORDS, false, first_iid, nreads, d_bases,
                          d_offsets, h_lengths);
}

int fe_load_reads(fe_ctx *c, uint32_t first_iid, uint32_t nreads, const uint8_t *bases,
                  const uint64_t *offsets, const uint32_t *lengths) {
  if (!c) return fail(FE_ERR_BAD_PARAM, "null context");
  DevBuf<uint8_t> d_b;
  DevBuf<uint64_t> d_o;
  if (int rc = capi::stage_reads(c->device, nreads, bases, offsets, lengths, d_b, d_o)) return rc;
  return fe_load_reads_device(c, first_iid, nreads, d_b.p, d_o.p, lengths);
}

int fe_find_errors(fe_ctx *c, uint32_t bgn_id, uint32_t end_id, const ovl_record *ov, uint64_t n,
                   uint64_t *n_corrections) {
  if (!c) return fail(FE_ERR_BAD_PARAM, "null context");
  if (n && !ov) return fail(FE_ERR_BAD_PARAM, "null overlaps");
  if (n > 0xfffffff0ull) return fail(FE_ERR_BAD_PARAM, "more than 2^32 overlaps in one call");
  const PackedReads &R = c->reads;
  c->S = fe_stats{};
  c->out.clear();
  if (n_corrections) *n_corrections = 0;
  if (bgn_id > end_id || bgn_id < R.first_iid || end_id - R.first_iid >= R.nreads)
    return fail(FE_ERR_BAD_INPUT, "range %u-%u is not within the loaded reads %u-%u", bgn_id,
                end_id, R.first_iid, R.first_iid + R.nreads - 1);
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t nr = end_id - bgn_id + 1;
  const double erate = c->P.error_rate;
  const uint64_t HM = (1ull << 21) - 1;

  // tally slots: len + 1 per read of the range (a difference may land one past the end)
  std::vector<uint64_t> toff(nr), rwoff(nr);
  std::vector<uint32_t> rlen(nr), keep(nr);
  uint64_t plane = 0;
  for (uint32_t r = 0; r < nr; r++) {
    toff[r] = plane;
    rlen[r] = R.len[bgn_id - R.first_iid + r];
    rwoff[r] = R.word_off[bgn_id - R.first_iid + r];
    plane += (uint64_t)rlen[r] + 1;
  }

  // Process_Olap's setup (:72-119), the checks the reference leaves out, and the degrees
  std::vector<Job> jobs(n);
  std::vector<uint64_t> ldeg(nr, 0), rdeg(nr, 0);
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t a = ov[i].a_iid, b = ov[i].b_iid;
    if (a < bgn_id || a > end_id)
      return fail(FE_ERR_BAD_INPUT, "overlap %llu: a_iid %u is outside the range %u-%u",
                  (unsigned long long)i, a, bgn_id, end_id);
    if (b < R.first_iid || b - R.first_iid >= R.nreads)
      return fail(FE_ERR_BAD_INPUT, "overlap %llu names read %u, not loaded",
                  (unsigned long long)i, b);
    const int64_t a5 = ov[i].dat[0] & HM, a3 = (ov[i].dat[0] >> 21) & HM;
    const int64_t b5 = ov[i].dat[1] & HM, b3 = (ov[i].dat[1] >> 21) & HM;
    const bool flipped = (ov[i].dat[0] >> 54) & 1;
    const int64_t a_hang = a5 - b5, b_hang = b3 - a3;          // ovOverlap.H:227-228
    const int64_t al = R.len[a - R.first_iid], bl = R.len[b - R.first_iid];
    if (a_hang > al || -a_hang > bl)
      return fail(FE_ERR_BAD_INPUT, "overlap %llu: a_hang %lld beyond its read (%u: %lld bases, "
                  "%u: %lld bases)", (unsigned long long)i, (long long)a_hang, a, (long long)al, b,
                  (long long)bl);
    Job &J = jobs[i];
    J.a_word = R.word_off[a - R.first_iid];
    J.b_word = R.word_off[b - R.first_iid];
    J.tally = toff[a - bgn_id];
    J.a_off = a_hang > 0 ? (int32_t)a_hang : 0;
    J.b_off = a_hang < 0 ? (int32_t)-a_hang : 0;
    J.m = (int32_t)al - J.a_off;
    J.n = (int32_t)bl - J.b_off;
    J.clear_len = (int32_t)al;
    J.limit = (int32_t)ceil((double)std::min(J.m, J.n) * erate);
    J.b_rc = flipped;
    J.pad = 0;
    if (a_hang <= 0) ldeg[a - bgn_id]++;
    if (b_hang >= 0) rdeg[a - bgn_id]++;
    c->S.bases += (uint64_t)std::min(J.m, J.n);
  }
  for (uint32_t r = 0; r < nr; r++) {
    const uint64_t l = std::min<uint64_t>(ldeg[r], MAX_DEGREE), g = std::min<uint64_t>(rdeg[r], MAX_DEGREE);
    keep[r] = (l < (uint64_t)c->P.degree_threshold ? 1u : 0u) |
              (g < (uint64_t)c->P.degree_threshold ? 2u : 0u);
  }

  DevBuf<int32_t> d_tally;
  DevBuf<uint64_t> d_toff, d_rwoff, d_recoff;
  DevBuf<uint32_t> d_rlen, d_keep, d_count;
  HIP_TRY(d_tally.alloc(plane * NPLANES));
  HIP_TRY(hipMemsetAsync(d_tally.p, 0, d_tally.bytes, c->stream));

  // behind a wave's delta, k_fe_align's change list: limit + 8 changes of 2 ints
  const AlignStage stage{"CANU_FE_LOG_PER_ERROR", "CANU_FE_LOG_CAP", FE_LOG_PER_ERROR, 2, 16,
                         F_PASSED | F_FAILED, "the change list outgrew its errors"};
  std::vector<uint32_t> fl;
  AlignStats A;
  const int rc = align_all(*c, stage, c->ml, erate, jobs, [&](const AlignLaunch<Job> &L) {
    AlignArgs X{};
    X.fwd = R.fwd.p; X.rc = R.rc.p; X.jobs = L.jobs; X.order = L.order;
    X.njobs = L.njobs; X.nwaves = L.nwaves; X.next = L.next; X.flags = L.flags; X.rows = L.rows;
    X.tallies = d_tally.p; X.plane = plane; X.match_limit = L.match_limit; X.scratch = L.scratch;
    X.log_cap = L.log_cap; X.per_wave = L.per_wave; X.max_limit = L.max_limit; X.erate = erate;
    X.kmer_len = c->P.kmer_len; X.vote_qualify_len = c->P.vote_qualify_len;
    X.end_exclude_len = c->P.end_exclude_len;
    hipLaunchKernelGGL(k_fe_align, dim3(L.blocks), dim3(64 * WAVES_PER_BLOCK), 0, c->stream, X);
    return hipGetLastError();
  }, fl, A);
  c->S.n_generic = A.n_generic; c->S.n_staged = A.n_staged; c->S.rows = A.rows;
  c->S.regrows = A.regrows; c->S.scratch_bytes = A.scratch_bytes; c->S.ms_align = A.ms_align;
  if (rc) return rc;
  for (uint32_t f : fl) {
    c->S.n_passed += !!(f & F_PASSED);
    c->S.n_failed += !!(f & F_FAILED);
  }

  // the two ladders, then the records in file order
  HIP_TRY(d_toff.alloc(nr));
  HIP_TRY(d_rwoff.alloc(nr));
  HIP_TRY(d_recoff.alloc(nr));
  HIP_TRY(d_rlen.alloc(nr));
  HIP_TRY(d_keep.alloc(nr));
  HIP_TRY(d_count.alloc(nr));
  HIP_TRY(hipMemcpyAsync(d_toff.p, toff.data(), nr * 8ull, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_rwoff.p, rwoff.data(), nr * 8ull, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_rlen.p, rlen.data(), nr * 4ull, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_keep.p, keep.data(), nr * 4ull, hipMemcpyHostToDevice, c->stream));
  DecideArgs D{};
  D.tallies = d_tally.p; D.plane = plane; D.tally_off = d_toff.p; D.word_off = d_rwoff.p;
  D.len = d_rlen.p; D.keep = d_keep.p; D.fwd = R.fwd.p; D.bgn_id = bgn_id; D.nreads = nr;
  D.use_haplo_ct = c->P.use_haplo_ct; D.count = d_count.p; D.rec_off = d_recoff.p;
  Event e0, e1, e2, e3;
  HIP_TRY(e0.create());
  HIP_TRY(e1.create());
  HIP_TRY(e2.create());
  HIP_TRY(e3.create());
  const uint32_t grid = std::min<uint32_t>(nr, (uint32_t)c->n_cu * 8);
  HIP_TRY(hipEventRecord(e0, c->stream));
  hipLaunchKernelGGL(k_fe_decide<0>, dim3(grid), dim3(256), 0, c->stream, D);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e1, c->stream));
  std::vector<uint32_t> count(nr);
  HIP_TRY(hipMemcpyAsync(count.data(), d_count.p, nr * 4ull, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::vector<uint64_t> recoff(nr);
  uint64_t total = 0;
  for (uint32_t r = 0; r < nr; r++) {
    recoff[r] = total;
    total += 1 + (uint64_t)count[r];
  }
  DevBuf<fe_correction> d_out;
  HIP_TRY(d_out.alloc(total));
  D.out = d_out.p;
  HIP_TRY(hipMemcpyAsync(d_recoff.p, recoff.data(), nr * 8ull, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipEventRecord(e2, c->stream));
  hipLaunchKernelGGL(k_fe_decide<1>, dim3(grid), dim3(256), 0, c->stream, D);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e3, c->stream));
  c->out.resize(total);
  HIP_TRY(hipMemcpyAsync(c->out.data(), d_out.p, total * sizeof(fe_correction),
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  float m0 = 0, m1 = 0;
  (void)hipEventElapsedTime(&m0, e0, e1);
  (void)hipEventElapsedTime(&m1, e2, e3);
  c->S.ms_decide = m0 + m1;
  if (n_corrections) *n_corrections = total;
  return FE_OK;
}

int fe_fetch_corrections(fe_ctx *c, fe_correction *out, uint64_t cap, uint64_t *n) {
  if (!c) return fail(FE_ERR_BAD_PARAM, "null context");
  if (n) *n = c->out.size();
  if (cap < c->out.size())
    return fail(FE_ERR_BAD_PARAM, "room for %llu records, %llu to fetch", (unsigned long long)cap,
                (unsigned long long)c->out.size());
  if (!c->out.empty()) {
    if (!out) return fail(FE_ERR_BAD_PARAM, "null out");
    memcpy(out, c->out.data(), c->out.size() * sizeof(fe_correction));
  }
  return FE_OK;
}

int fe_write_red(fe_ctx *c, const char *path) {
  if (!c || !path) return fail(FE_ERR_BAD_PARAM, "null context or path");
  FILE *f = fopen(path, "wb");
  if (!f) return fail(FE_ERR_BAD_PARAM, "can't open '%s' for writing: %s", path, strerror(errno));
  const size_t w = c->out.empty() ? 0 : fwrite(c->out.data(), sizeof(fe_correction), c->out.size(), f);
  if (fclose(f) != 0 || w != c->out.size())
    return fail(FE_ERR_BAD_PARAM, "short write to '%s'", path);
  return FE_OK;
}

int fe_get_stats(const fe_ctx *c, fe_stats *out) {
  if (!c || !out) return fail(FE_ERR_BAD_PARAM, "null context or out");
  *out = c->S;
  return FE_OK;
}

}  // extern "C"
