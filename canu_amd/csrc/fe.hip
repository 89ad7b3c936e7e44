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
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/canu_fe.h"
#include "hip_raii.h"
#include "ped_host.h"
#include "ped_wave.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(x)                                                                    \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess)                                                             \
      return fail(e_ == hipErrorOutOfMemory ? FE_ERR_OOM : FE_ERR_HIP, "%s: %s", #x,  \
                  hipGetErrorString(e_));                                             \
  } while (0)

using namespace ped;

static_assert(FE_WINDOW_DIAGS == PED_WINDOW_DIAGS, "canu_fe.h names the aligner's window");
constexpr int WAVES_PER_BLOCK = 4;
constexpr uint64_t SCRATCH_BUDGET = 16ull << 30;      // row logs of one launch, bytes
constexpr int MAX_VOTE = 255, MAX_DEGREE = 32767;     // findErrors.H:87-90
constexpr int MIN_HAPLO_OCCURS = 3;                   // findErrors.H:102
constexpr int NPLANES = 11;
// Vote_Value_t (correctionOutput.H:24-37) and the tally plane of each vote
enum { V_IDENT = 0, V_DELETE = 1, V_A_SUBST = 2, V_T_SUBST = 5, V_A_INSERT = 6 };
enum { PL_CONFIRMED = 0, PL_DELETES = 1, PL_SUBST = 2, PL_NO_INSERT = 6, PL_INSERT = 7 };
// per-overlap outcome
enum : uint32_t { F_PASSED = 1, F_FAILED = 2, F_OVERFLOW = 4, F_GENERIC = 8, F_INTERNAL = 16,
                  F_STAGED = 32 };
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

// ------------------------------------------------------------------ read encoding

__global__ void k_fe_encode(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ src_off,
                            const uint64_t *__restrict__ word_off, const uint32_t *__restrict__ len,
                            uint32_t nreads, uint32_t *__restrict__ fwd, uint32_t *__restrict__ rc) {
  for (uint32_t r = blockIdx.x; r < nreads; r += gridDim.x) {
    const uint8_t *s = bases + src_off[r];
    const uint32_t L = len[r];
    const uint32_t nw = (L + 15) / 16;
    for (uint32_t w = threadIdx.x; w < nw; w += blockDim.x) {
      uint32_t f = 0, v = 0;
      for (uint32_t j = 0; j < 16; j++) {
        const uint32_t i = w * 16 + j;
        if (i >= L) break;
        const uint8_t ch = s[i] | 0x20, cr = s[L - 1 - i] | 0x20;
        const uint32_t c = ch == 'c' ? 1 : ch == 'g' ? 2 : ch == 't' ? 3 : 0;   // the rest is 'a'
        const uint32_t d = cr == 'c' ? 1 : cr == 'g' ? 2 : cr == 't' ? 3 : 0;
        f |= c << (2 * j);
        v |= (3 - d) << (2 * j);
      }
      fwd[word_off[r] + w] = f;
      rc[word_off[r] + w] = v;
    }
  }
}

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

struct fe_ctx {
  fe_params P;
  int device = 0;
  int n_cu = 256;
  hipStream_t stream = nullptr;
  uint32_t *d_fwd = nullptr, *d_rc = nullptr;
  uint32_t first_iid = 0, nreads = 0;
  std::vector<uint32_t> len;
  std::vector<uint64_t> word_off;
  std::vector<int32_t> ml;           // Edit_Match_Limit, grown on demand
  double ml_erate = -1.0;
  std::vector<fe_correction> out;
  fe_stats S{};
};

namespace {

void free_reads(fe_ctx *c) {
  if (c->d_fwd) (void)hipFree(c->d_fwd);
  if (c->d_rc) (void)hipFree(c->d_rc);
  c->d_fwd = c->d_rc = nullptr;
  c->nreads = 0;
  c->len.clear();
  c->word_off.clear();
}

}  // namespace

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

const char *fe_last_error(void) { return g_err.c_str(); }
int fe_abi_version(void) { return FE_ABI_VERSION; }

int fe_ctx_create(const fe_params *p, int device, fe_ctx **out) {
  if (!out) return fail(FE_ERR_BAD_PARAM, "null out");
  *out = nullptr;
  if (int rc = check_params(p)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(FE_ERR_NO_DEVICE, "no HIP device %d", device);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(FE_ERR_NO_DEVICE, "device %d is %s, this library is built for gfx950", device,
                prop.gcnArchName);
  HIP_TRY(hipSetDevice(device));
  fe_ctx *c = new fe_ctx;
  c->device = device;
  c->n_cu = prop.multiProcessorCount;
  c->P = *p;
  hipError_t e = hipStreamCreate(&c->stream);
  if (e != hipSuccess) {
    delete c;
    return fail(FE_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
  }
  *out = c;
  return FE_OK;
}

void fe_ctx_destroy(fe_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  free_reads(c);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int fe_set_params(fe_ctx *c, const fe_params *p) {
  if (!c) return fail(FE_ERR_BAD_PARAM, "null context");
  if (int rc = check_params(p)) return rc;
  c->P = *p;
  return FE_OK;
}

int fe_load_reads_device(fe_ctx *c, uint32_t first_iid, uint32_t nreads, const uint8_t *d_bases,
                         const uint64_t *d_offsets, const uint32_t *h_lengths) {
  if (!c) return fail(FE_ERR_BAD_PARAM, "null context");
  if (nreads && (!d_bases || !d_offsets || !h_lengths))
    return fail(FE_ERR_BAD_PARAM, "null read buffers");
  if ((uint64_t)first_iid + nreads > 0xffffffffull)
    return fail(FE_ERR_BAD_PARAM, "read IDs beyond 32 bits");
  HIP_TRY(hipSetDevice(c->device));
  free_reads(c);
  std::vector<uint64_t> woff(nreads);
  uint64_t words = 0;
  for (uint32_t i = 0; i < nreads; i++) {
    if (h_lengths[i] > AS_MAX_READLEN)
      return fail(FE_ERR_BAD_INPUT, "read %u is %u bases, beyond AS_MAX_READLEN", first_iid + i,
                  h_lengths[i]);
    woff[i] = words;
    words += (h_lengths[i] + 15) / 16 + PAD_WORDS;
  }
  DevBuf<uint64_t> d_woff;
  DevBuf<uint32_t> d_len;
  HIP_TRY(d_woff.alloc(nreads));
  HIP_TRY(d_len.alloc(nreads));
  HIP_TRY(hipMalloc((void **)&c->d_fwd, std::max<uint64_t>(words, 1) * 4));
  HIP_TRY(hipMalloc((void **)&c->d_rc, std::max<uint64_t>(words, 1) * 4));
  HIP_TRY(hipMemsetAsync(c->d_fwd, 0, std::max<uint64_t>(words, 1) * 4, c->stream));
  HIP_TRY(hipMemsetAsync(c->d_rc, 0, std::max<uint64_t>(words, 1) * 4, c->stream));
  if (nreads) {
    HIP_TRY(hipMemcpyAsync(d_woff.p, woff.data(), nreads * 8ull, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_len.p, h_lengths, nreads * 4ull, hipMemcpyHostToDevice, c->stream));
    const uint32_t grid = std::min<uint32_t>(nreads, 4096);
    hipLaunchKernelGGL(k_fe_encode, dim3(grid), dim3(256), 0, c->stream, d_bases, d_offsets,
                       d_woff.p, d_len.p, nreads, c->d_fwd, c->d_rc);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->first_iid = first_iid;
  c->nreads = nreads;
  c->len.assign(h_lengths, h_lengths + nreads);
  c->word_off = std::move(woff);
  return FE_OK;
}

int fe_load_reads(fe_ctx *c, uint32_t first_iid, uint32_t nreads, const uint8_t *bases,
                  const uint64_t *offsets, const uint32_t *lengths) {
  if (!c) return fail(FE_ERR_BAD_PARAM, "null context");
  if (nreads && (!bases || !offsets || !lengths))
    return fail(FE_ERR_BAD_PARAM, "null read buffers");
  HIP_TRY(hipSetDevice(c->device));
  uint64_t bytes = 0;
  for (uint32_t i = 0; i < nreads; i++) bytes = std::max(bytes, offsets[i] + lengths[i]);
  DevBuf<uint8_t> d_b;
  DevBuf<uint64_t> d_o;
  HIP_TRY(d_b.alloc(bytes));
  HIP_TRY(d_o.alloc(nreads));
  if (bytes) HIP_TRY(hipMemcpy(d_b.p, bases, bytes, hipMemcpyHostToDevice));
  if (nreads) HIP_TRY(hipMemcpy(d_o.p, offsets, nreads * 8ull, hipMemcpyHostToDevice));
  return fe_load_reads_device(c, first_iid, nreads, d_b.p, d_o.p, lengths);
}

int fe_find_errors(fe_ctx *c, uint32_t bgn_id, uint32_t end_id, const ovl_record *ov, uint64_t n,
                   uint64_t *n_corrections) {
  if (!c) return fail(FE_ERR_BAD_PARAM, "null context");
  if (n && !ov) return fail(FE_ERR_BAD_PARAM, "null overlaps");
  if (n > 0xfffffff0ull) return fail(FE_ERR_BAD_PARAM, "more than 2^32 overlaps in one call");
  c->S = fe_stats{};
  c->out.clear();
  if (n_corrections) *n_corrections = 0;
  if (bgn_id > end_id || bgn_id < c->first_iid || end_id - c->first_iid >= c->nreads)
    return fail(FE_ERR_BAD_INPUT, "range %u-%u is not within the loaded reads %u-%u", bgn_id,
                end_id, c->first_iid, c->first_iid + c->nreads - 1);
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
    rlen[r] = c->len[bgn_id - c->first_iid + r];
    rwoff[r] = c->word_off[bgn_id - c->first_iid + r];
    plane += (uint64_t)rlen[r] + 1;
  }

  // Process_Olap's setup (:72-119), the checks the reference leaves out, and the degrees
  std::vector<Job> jobs(n);
  std::vector<uint64_t> ldeg(nr, 0), rdeg(nr, 0);
  int32_t max_limit = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t a = ov[i].a_iid, b = ov[i].b_iid;
    if (a < bgn_id || a > end_id)
      return fail(FE_ERR_BAD_INPUT, "overlap %llu: a_iid %u is outside the range %u-%u",
                  (unsigned long long)i, a, bgn_id, end_id);
    if (b < c->first_iid || b - c->first_iid >= c->nreads)
      return fail(FE_ERR_BAD_INPUT, "overlap %llu names read %u, not loaded",
                  (unsigned long long)i, b);
    const int64_t a5 = ov[i].dat[0] & HM, a3 = (ov[i].dat[0] >> 21) & HM;
    const int64_t b5 = ov[i].dat[1] & HM, b3 = (ov[i].dat[1] >> 21) & HM;
    const bool flipped = (ov[i].dat[0] >> 54) & 1;
    const int64_t a_hang = a5 - b5, b_hang = b3 - a3;          // ovOverlap.H:227-228
    const int64_t al = c->len[a - c->first_iid], bl = c->len[b - c->first_iid];
    if (a_hang > al || -a_hang > bl)
      return fail(FE_ERR_BAD_INPUT, "overlap %llu: a_hang %lld beyond its read (%u: %lld bases, "
                  "%u: %lld bases)", (unsigned long long)i, (long long)a_hang, a, (long long)al, b,
                  (long long)bl);
    Job &J = jobs[i];
    J.a_word = c->word_off[a - c->first_iid];
    J.b_word = c->word_off[b - c->first_iid];
    J.tally = toff[a - bgn_id];
    J.a_off = a_hang > 0 ? (int32_t)a_hang : 0;
    J.b_off = a_hang < 0 ? (int32_t)-a_hang : 0;
    J.m = (int32_t)al - J.a_off;
    J.n = (int32_t)bl - J.b_off;
    J.clear_len = (int32_t)al;
    J.limit = (int32_t)ceil((double)std::min(J.m, J.n) * erate);
    J.b_rc = flipped;
    J.pad = 0;
    max_limit = std::max(max_limit, J.limit);
    if (a_hang <= 0) ldeg[a - bgn_id]++;
    if (b_hang >= 0) rdeg[a - bgn_id]++;
    c->S.bases += (uint64_t)std::min(J.m, J.n);
  }
  for (uint32_t r = 0; r < nr; r++) {
    const uint64_t l = std::min<uint64_t>(ldeg[r], MAX_DEGREE), g = std::min<uint64_t>(rdeg[r], MAX_DEGREE);
    keep[r] = (l < (uint64_t)c->P.degree_threshold ? 1u : 0u) |
              (g < (uint64_t)c->P.degree_threshold ? 2u : 0u);
  }

  if (c->ml_erate != erate || (int32_t)c->ml.size() < max_limit + 2) {
    const int32_t max_errors = 1 + (int32_t)(uint32_t)(erate * AS_MAX_READLEN);
    init_match_limit(c->ml, erate, max_errors, max_limit + 1);
    c->ml_erate = erate;
  }

  DevBuf<int32_t> d_tally, d_ml;
  DevBuf<uint64_t> d_toff, d_rwoff, d_recoff;
  DevBuf<uint32_t> d_rlen, d_keep, d_count;
  HIP_TRY(d_tally.alloc(plane * NPLANES));
  HIP_TRY(hipMemsetAsync(d_tally.p, 0, std::max<uint64_t>(plane * NPLANES, 1) * 4, c->stream));
  float ms_align = 0;

  if (n) {
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
      return std::min(jobs[x].m, jobs[x].n) > std::min(jobs[y].m, jobs[y].n);
    });
    DevBuf<Job> d_jobs;
    DevBuf<uint32_t> d_order, d_next, d_flags, d_rows;
    HIP_TRY(d_jobs.alloc(n));
    HIP_TRY(d_order.alloc(n));
    HIP_TRY(d_next.alloc(1));
    HIP_TRY(d_flags.alloc(n));
    HIP_TRY(d_rows.alloc(n));
    HIP_TRY(d_ml.alloc(c->ml.size()));
    HIP_TRY(hipMemcpyAsync(d_jobs.p, jobs.data(), n * sizeof(Job), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_ml.p, c->ml.data(), c->ml.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(d_flags.p, 0, n * 4, c->stream));
    HIP_TRY(hipMemsetAsync(d_rows.p, 0, n * 4, c->stream));

    int per_error = FE_LOG_PER_ERROR;
    if (const char *e = getenv("CANU_FE_LOG_PER_ERROR")) per_error = std::max(1, atoi(e));
    std::vector<uint32_t> todo = order, fl(n), rows(n);
    int32_t cur_limit = max_limit;
    uint64_t log_cap = row_log_first(per_error, max_limit);
    // test knob: the exact size of the first row log
    if (const char *e = getenv("CANU_FE_LOG_CAP")) log_cap = std::max<uint64_t>(2, strtoull(e, nullptr, 10));
    Event e0, e1;
    HIP_TRY(e0.create());
    HIP_TRY(e1.create());
    while (!todo.empty()) {
      const uint64_t nt = todo.size();
      const uint64_t per_wave = log_cap + 3ull * (cur_limit + 2) + 2ull * (cur_limit + 4) +
                                2ull * (cur_limit + 8) + 8;
      // 64 VGPRs and 4 KB of LDS per wave: eight waves per SIMD fit, if their row logs fit the
      // budget; no more waves (and logs) than overlaps, and one wave always
      const uint64_t fit = std::max<uint64_t>(1, SCRATCH_BUDGET / (per_wave * 4));
      const uint64_t nwaves = std::min<uint64_t>({nt, (uint64_t)c->n_cu * 8 * WAVES_PER_BLOCK, fit});
      const uint32_t blocks = (uint32_t)((nwaves + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK);
      if (log_cap > ROW_LOG_MAX)
        return fail(FE_ERR_UNSUPPORTED, "a row log of %llu entries (%d errors allowed) is beyond "
                    "the 32-bit offsets of this build", (unsigned long long)log_cap, cur_limit);
      DevBuf<int32_t> d_scratch;
      HIP_TRY(d_scratch.alloc(per_wave * nwaves));
      c->S.scratch_bytes = per_wave * nwaves * 4;
      HIP_TRY(hipMemcpyAsync(d_order.p, todo.data(), nt * 4, hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipMemsetAsync(d_next.p, 0, 4, c->stream));
      AlignArgs X{};
      X.fwd = c->d_fwd; X.rc = c->d_rc; X.jobs = d_jobs.p; X.order = d_order.p;
      X.njobs = (uint32_t)nt; X.nwaves = (uint32_t)nwaves; X.next = d_next.p; X.flags = d_flags.p; X.rows = d_rows.p;
      X.tallies = d_tally.p; X.plane = plane; X.match_limit = d_ml.p; X.scratch = d_scratch.p;
      X.log_cap = log_cap; X.per_wave = per_wave; X.max_limit = cur_limit; X.erate = erate;
      X.kmer_len = c->P.kmer_len; X.vote_qualify_len = c->P.vote_qualify_len;
      X.end_exclude_len = c->P.end_exclude_len;
      HIP_TRY(hipEventRecord(e0, c->stream));
      hipLaunchKernelGGL(k_fe_align, dim3(blocks), dim3(64 * WAVES_PER_BLOCK), 0, c->stream, X);
      hipError_t le = hipGetLastError();
      HIP_TRY(hipEventRecord(e1, c->stream));
      hipError_t se = hipStreamSynchronize(c->stream);
      HIP_TRY(le);
      HIP_TRY(se);
      float ms = 0;
      (void)hipEventElapsedTime(&ms, e0, e1);
      ms_align += ms;
      HIP_TRY(hipMemcpy(fl.data(), d_flags.p, n * 4, hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(rows.data(), d_rows.p, n * 4, hipMemcpyDeviceToHost));
      std::vector<uint32_t> again;
      int32_t next_limit = 0;
      for (uint32_t i : todo) {
        c->S.rows += rows[i];
        if (fl[i] & F_INTERNAL)
          return fail(FE_ERR_HIP, "overlap %u: the change list outgrew its errors", i);
        if (fl[i] & F_OVERFLOW) {
          again.push_back(i);
          next_limit = std::max(next_limit, jobs[i].limit);
        } else if (!(fl[i] & (F_PASSED | F_FAILED))) {
          return fail(FE_ERR_HIP, "overlap %u was not processed", i);
        }
      }
      if (!again.empty()) {
        log_cap = row_log_regrown(log_cap, next_limit);
        if (!log_cap) return fail(FE_ERR_HIP, "row log overflow at its worst-case size");
        c->S.regrows++;
        cur_limit = next_limit;
      }
      todo.swap(again);
    }
    for (uint64_t i = 0; i < n; i++) {
      c->S.n_passed += !!(fl[i] & F_PASSED);
      c->S.n_failed += !!(fl[i] & F_FAILED);
      c->S.n_generic += !!(fl[i] & F_GENERIC);
      c->S.n_staged += !!(fl[i] & F_STAGED);
    }
  }
  c->S.ms_align = ms_align;

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
  D.len = d_rlen.p; D.keep = d_keep.p; D.fwd = c->d_fwd; D.bgn_id = bgn_id; D.nreads = nr;
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
