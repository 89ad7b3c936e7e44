// co.hip -- libcanu_co.so: canu's correctOverlaps (src/overlapErrorAdjustment/correctOverlaps*.C)
// on gfx950.
//
// k_co_correct: one block owns one read and runs correctRead (correctOverlaps-Correct_Frags.C:
// 38-179).  One thread walks the read's corrections -- a few dozen records, each acting on the
// base the loop variable `i` of the reference stands on, which depends on the record before --
// and leaves per base what becomes of it and a +1 / -1 where the length changes; the block then
// prefix-sums the changes, moves every base to its place, and packs the corrected read 2 bits
// per base, forward and reverse complemented.  The walk also writes the forward adjust list;
// the reverse list is Make_Rev_Adjust's closed form (correctOverlaps-Redo_Olaps.C:173-230),
// computed where it is read.
//
// k_co_align: one wave owns one overlap and runs the body of Redo_Olaps (:367-521) -- Hang_Adjust,
// correctOverlaps' Prefix_Edit_Dist (correctOverlaps-Prefix_Edit_Distance.C:165-312) with
// Compute_Delta on the path that reaches an end, the leading-gap trim, the failure tests and
// the nine counters -- and leaves `errors` and `olapLen`; the host encodes the evalue.  The
// aligner is ped_wave.h's, shared with k_fe_align: lanes as diagonals, 32 bases per slide step,
// spans staged in LDS, a register window with the row log in global memory behind it, a re-run
// with the worst-case log for the alignments that outgrow the first.  What is correctOverlaps'
// own is the one-clause Max_Score test and that only an alignment to an end is traced back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/canu_co.h"
#include "capi_common.h"
#include "ped_launch.h"
#include "ped_wave.h"

namespace {

using namespace ped;
using capi::fail;

CAPI_SAME_CODES(CO);
static_assert(CO_WINDOW_DIAGS == PED_WINDOW_DIAGS, "canu_co.h names the aligner's window");
constexpr uint64_t CORRECT_BUDGET = 4ull << 30;       // per-block work areas of k_co_correct
constexpr int AS_MAX_EVALUE = 4095;                   // ovOverlap.H:41-42
// Vote_Value_t (correctionOutput.H:24-37)
enum { V_IDENT = 0, V_DELETE = 1, V_A_SUBST = 2, V_T_SUBST = 5, V_A_INSERT = 6, V_T_INSERT = 9 };
// what k_co_correct thinks of a read
enum : uint32_t { R_OK = 0, R_NO_IDENT = 1, R_BAD_POSITION = 2 };
// per-overlap outcome, with ped_host.h's
enum : uint32_t { F_DONE = 1, F_TO_END = 2 };
// the nine counters, in the order Redo_Olaps prints them
enum { C_FWD = 0, C_REV, C_TOTAL, C_BOTH, C_EITHER, C_END, C_LENGTH, C_RHA_FAIL, C_RHA_PASS, NCOUNT };
constexpr int LDS_STRAND_WORDS = lds_strand_words(CO_LDS_BASES);

struct Adjust { int32_t adjpos, adjust; };   // Adjust_t, correctOverlaps.H:107-110

struct Job {                 // one overlap, as Redo_Olaps sets it up (:367-410)
  uint64_t a_word, b_word;   // first packed word of corrected A (forward) and of B (as oriented)
  uint32_t a_read, b_read;   // among the loaded reads
  int32_t a_hang;            // as the store has it
  int32_t a_off, b_off;      // the adjusted hangs, as the host computed them
  int32_t m, n;              // a_part_len, b_part_len
  int32_t limit;             // Error_Bound[min(m, n)]
  uint32_t b_rc;             // B comes from the reverse-complement array
  uint32_t pad;
};

struct AlignArgs {
  const uint32_t *fwd, *rc;          // packed corrected reads
  const Job *jobs;
  const uint32_t *order;             // longest first
  uint32_t njobs, nwaves;            // waves that own scratch
  uint32_t *next;                    // work counter
  uint32_t *flags, *rows;            // per overlap
  int32_t *errors, *olap_len;        // per overlap
  unsigned long long *counters;      // NCOUNT
  const Adjust *adj;                 // forward adjust lists
  const uint64_t *adj_off;           // per read
  const uint32_t *adj_cnt, *clen;    // per read
  const int32_t *match_limit;        // Edit_Match_Limit[e]
  int32_t *scratch;                  // per wave: log, meta, stack, delta
  uint64_t log_cap, per_wave;        // ints
  int32_t max_limit;
};

// ------------------------------------------------------------------ the corrections

struct CorrectArgs {
  const uint32_t *ofwd;              // the reads as loaded, packed
  const uint64_t *oword_off;
  const uint32_t *len;
  uint32_t nreads;
  const fe_correction *red;
  const uint64_t *rec_first;         // a read's records behind its IDENT record
  const uint32_t *rec_cnt;
  int32_t *delta;                    // per block: max_len + 1 length changes
  uint8_t *op;                       // per block: max_len fates (0 copy, 1 drop, 2 + letter)
  uint8_t *cbytes;                   // per block: the corrected read, a byte per base
  uint64_t max_len, max_out;
  uint32_t *cfwd, *crc;              // the corrected reads, packed
  const uint64_t *cword_off;
  uint32_t *clen;
  Adjust *adj;
  const uint64_t *adj_off;
  uint32_t *adj_cnt;
  uint32_t *status;                  // R_NO_IDENT comes from the host and stays
  uint32_t *changes;                 // per read: substitutions, deletions, insertions applied
};

__global__ __launch_bounds__(256) void k_co_correct(const CorrectArgs X) {
  __shared__ int lds[8];
  __shared__ int s_clen;
  int32_t *const delta = X.delta + (uint64_t)blockIdx.x * (X.max_len + 1);
  uint8_t *const op = X.op + (uint64_t)blockIdx.x * X.max_len;
  uint8_t *const cb = X.cbytes + (uint64_t)blockIdx.x * X.max_out;
  for (uint32_t r = blockIdx.x; r < X.nreads; r += gridDim.x) {
    const int L = (int)X.len[r];
    const uint32_t *const O = X.ofwd + X.oword_off[r];
    for (int i = threadIdx.x; i <= L; i += blockDim.x) {
      delta[i] = 0;
      if (i < L) op[i] = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      // correctRead's loop (:76-172), one record at a time.  `after` is where its `i` stands
      // when a record is done; the next record acts at max(after, pos), which the assertion
      // (:95-96) wants at pos or pos + 1.  A record the loop never reaches (i >= oseqLen) is
      // not applied.  An insert lands in front of base pos + 1 in both of its forms, behind
      // the inserts already there, at pos + 1 + adjVal of the corrected read.
      const fe_correction *C = X.red + X.rec_first[r];
      const uint32_t nc = X.rec_cnt[r];
      Adjust *const adj = X.adj + X.adj_off[r];
      int after = 0, adj_val = 0, nadj = 0, nsub = 0, ndel = 0, nins = 0;
      uint32_t st = R_OK;
      for (uint32_t k = 0; k < nc; k++) {
        const uint32_t w = C[k].word;
        const int type = (int)((w >> 2) & 15), pos = (int)(w >> 6);
        const int i = max(after, pos);
        if (i >= L) break;
        if ((i != pos && i != pos + 1) || type < V_DELETE || type > V_T_INSERT) {
          st = R_BAD_POSITION;
          break;
        }
        if (type == V_DELETE) {
          op[i] = 1;
          delta[i + 1] -= 1;
          adj[nadj++] = Adjust{i + 1, --adj_val};
          ndel++;
          after = i + 1;
        } else if (type <= V_T_SUBST) {
          op[i] = (uint8_t)(2 + type - V_A_SUBST);
          nsub++;
          after = i + 1;
        } else {
          cb[pos + 1 + adj_val] = (uint8_t)(type - V_A_INSERT);
          delta[pos + 1] += 1;
          adj[nadj++] = Adjust{pos + 2, ++adj_val};
          nins++;
          after = pos + 1;
        }
      }
      s_clen = L + nins - ndel;
      X.clen[r] = (uint32_t)(L + nins - ndel);
      X.adj_cnt[r] = (uint32_t)nadj;
      if (st != R_OK) X.status[r] = st;
      X.changes[3 * r] = (uint32_t)nsub;
      X.changes[3 * r + 1] = (uint32_t)ndel;
      X.changes[3 * r + 2] = (uint32_t)nins;
    }
    __syncthreads();
    const int Lc = s_clen;
    // every base to i + (inserts in front of it) - (deletions before it)
    int carry = 0;
    for (int i0 = 0; i0 < L; i0 += 256) {
      const int i = i0 + (int)threadIdx.x;
      int tot;
      const int s = block_scan_incl(i < L ? delta[i] : 0, lds, tot);
      if (i < L) {
        const int o = op[i];
        if (o != 1) cb[i + carry + s] = (uint8_t)(o >= 2 ? o - 2 : code_at(O, i));
      }
      carry += tot;
    }
    __syncthreads();
    const int nw = (Lc + 15) / 16 + PAD_WORDS;
    for (int w = threadIdx.x; w < nw; w += blockDim.x) {
      uint32_t f = 0, v = 0;
      for (int j = 0; j < 16; j++) {
        const int i = w * 16 + j;
        if (i >= Lc) break;
        f |= (uint32_t)cb[i] << (2 * j);
        v |= (uint32_t)(3 - cb[Lc - 1 - i]) << (2 * j);
      }
      X.cfwd[X.cword_off[r] + w] = f;
      X.crc[X.cword_off[r] + w] = v;
    }
    __syncthreads();
  }
}

// Entry j of a read's adjust list: the forward list as stored, or the reverse list as
// Make_Rev_Adjust (:173-230) builds it from the forward one -- entry j comes from forward entry
// i = ct - 1 - j, whose step (+1 an insert, -1 a deletion) decides the position, and carries the
// sum of the steps from i on.
__host__ __device__ inline Adjust adjust_entry(const Adjust *adj, int ct, int j, bool rev, int frag_len) {
  if (!rev) return adj[j];
  const int i = ct - 1 - j;
  const int prev = i > 0 ? adj[i - 1].adjust : 0;
  const int step = adj[i].adjust - prev;
  return Adjust{(step == 1 ? 2 : 3) + frag_len - adj[i].adjpos, adj[ct - 1].adjust - prev};
}

// Hang_Adjust (:238-257) by a wave: the scan stops at the first entry beyond the hang.
__device__ __forceinline__ int hang_adjust(const Adjust *adj, int ct, int hang, bool rev,
                                           int frag_len, int lane) {
  for (int j0 = 0; j0 < ct; j0 += 64) {
    const int j = j0 + lane;
    bool stop = false;
    if (j < ct) stop = hang < adjust_entry(adj, ct, j, rev, frag_len).adjpos;
    const uint64_t sm = __ballot(stop);
    if (sm || j0 + 64 >= ct) {
      const int first = sm ? j0 + __builtin_ctzll(sm) : ct;
      return first == 0 ? hang : hang + adjust_entry(adj, ct, first - 1, rev, frag_len).adjust;
    }
  }
  return hang;
}

int hang_adjust_host(const Adjust *adj, int ct, int hang, bool rev, int frag_len) {
  int delta = 0;
  for (int j = 0; j < ct; j++) {
    const Adjust a = adjust_entry(adj, ct, j, rev, frag_len);
    if (hang < a.adjpos) break;
    delta = a.adjust;
  }
  return hang + delta;
}

// ------------------------------------------------------------------ the aligner

// Eight waves per SIMD (64 VGPRs) and 4 KB of LDS per wave, as k_fe_align: the kernel waits on
// the row log.
__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, 8) void k_co_align(const AlignArgs X) {
  __shared__ uint32_t s_strand[WAVES_PER_BLOCK][2][LDS_STRAND_WORDS];
  const int lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
  if (wave >= X.nwaves) return;
  int32_t *const log = X.scratch + (uint64_t)wave * X.per_wave;
  int32_t *const meta = log + X.log_cap;                       // 3 per row
  int32_t *const stk = meta + 3 * (uint64_t)(X.max_limit + 2); // deltaStack
  int32_t *const delta = stk + (X.max_limit + 4);

  for (;;) {
    const uint32_t slot = next_job(X.next, lane);
    if (slot >= X.njobs) break;
    const uint32_t oi = X.order[slot];
    const Job J = X.jobs[oi];
    // :375-404, the adjusted hangs
    int ab = 0, bb = 0;
    if (J.a_hang > 0)
      ab = hang_adjust(X.adj + X.adj_off[J.a_read], (int)X.adj_cnt[J.a_read], J.a_hang, false,
                       (int)X.clen[J.a_read], lane);
    if (J.a_hang < 0)
      bb = hang_adjust(X.adj + X.adj_off[J.b_read], (int)X.adj_cnt[J.b_read], -J.a_hang, J.b_rc != 0,
                       (int)X.clen[J.b_read], lane);
    ab = uni(ab);
    bb = uni(bb);
    const int m = (int)X.clen[J.a_read] - ab, n = (int)X.clen[J.b_read] - bb;
    if (ab != J.a_off || bb != J.b_off || m != J.m || n != J.n) {   // the host sized for its own
      if (lane == 0) { X.flags[oi] = F_INTERNAL; X.rows[oi] = 0; }
      continue;
    }
    // the two spans the aligner reads
    const uint32_t *As = X.fwd + J.a_word, *B = (J.b_rc ? X.rc : X.fwd) + J.b_word;
    int as = ab;
    uint32_t flags = 0;
    if (ped_stage<CO_LDS_BASES>(As, as, B, bb, m, n, J.limit, s_strand[threadIdx.x >> 6][0],
                                s_strand[threadIdx.x >> 6][1], lane))
      flags |= F_STAGED;

    const PedRows R = ped_rows(As, as, B, bb, m, n, J.limit, X.match_limit, log, meta, X.log_cap, lane,
                               [](int score, double max_score, int, int, int) {
                                 return (double)score > max_score;
                               });
    if (R.generic) flags |= F_GENERIC;
    if (R.aborted) {
      if (lane == 0) { X.flags[oi] = F_OVERFLOW | flags; X.rows[oi] = R.nrows; }
      continue;
    }
    // the alignment to the end and its delta, or else the Max_Score cell as where it stopped and
    // one error too many (:303-311)
    const bool to_end = R.ended;
    int errors, a_end, b_end, delta_len = 0;
    if (!to_end) {
      errors = J.limit + 1; a_end = R.ms_len; b_end = R.ms_len + R.ms_d;
    } else {
      errors = R.end_e; a_end = R.end_row; b_end = R.end_row + R.end_d;
      delta_len = ped_delta(log, meta, stk, delta, R.end_e, R.end_d, R.end_row, lane);
    }

    // :431-468: a leading run of gaps on the side that hangs, against the hang as stored
    if (delta_len > 0 && J.a_hang != 0) {
      const int want = J.a_hang > 0 ? 1 : -1;
      const int stop = min(delta_len, abs(J.a_hang));
      int run = 0;
      for (int k0 = 0; k0 < stop; k0 += 64) {
        const int k = k0 + lane;
        const uint64_t bm = __ballot(k < stop && delta[k] != want);
        if (bm) { run = k0 + __builtin_ctzll(bm); break; }
        run = min(k0 + 64, stop);
      }
      if (want > 0) a_end -= run; else b_end -= run;
      errors -= run;
    }
    const int olap_len = min(a_end, b_end);                    // :474
    if (to_end) flags |= F_TO_END;
    if (lane == 0) {
      const bool rha = J.a_hang < 0, bad = !to_end || olap_len <= 0;
      atomicAdd(X.counters + (J.b_rc ? C_REV : C_FWD), 1ull);
      atomicAdd(X.counters + C_TOTAL, 1ull);
      if (!to_end && olap_len <= 0) atomicAdd(X.counters + C_BOTH, 1ull);
      if (!to_end) atomicAdd(X.counters + C_END, 1ull);
      if (olap_len <= 0) atomicAdd(X.counters + C_LENGTH, 1ull);
      if (bad) atomicAdd(X.counters + C_EITHER, 1ull);
      if (rha) atomicAdd(X.counters + (bad ? C_RHA_FAIL : C_RHA_PASS), 1ull);
      X.errors[oi] = errors;
      X.olap_len[oi] = olap_len;
      X.flags[oi] = flags | F_DONE;
      X.rows[oi] = R.nrows;
    }
  }
}

int check_params(const co_params *p) {
  if (!p) return fail(CO_ERR_BAD_PARAM, "null parameters");
  if (!(p->error_rate >= 0.0 && p->error_rate < 1.0))
    return fail(CO_ERR_BAD_PARAM, "error_rate %g outside [0, 1)", p->error_rate);
  return CO_OK;
}

}  // namespace

struct co_ctx : capi::Device {
  co_params P;
  PackedReads reads;                 // as loaded: forward only, with the device tables
  // the corrected reads
  bool corrected = false;
  DevBuf<uint32_t> d_cfwd, d_crc, d_clen, d_adj_cnt;
  DevBuf<uint64_t> d_adj_off;
  DevBuf<Adjust> d_adj;
  std::vector<uint64_t> cword_off, adj_off;
  std::vector<uint32_t> clen, adj_cnt, status, changes;
  std::vector<Adjust> adj;
  MatchLimit ml;
  // the last result
  uint32_t bgn_id = 0, end_id = 0;
  std::vector<uint16_t> evalues;
  co_stats S{};
};

namespace {

void drop_corrections(co_ctx *c) {
  c->corrected = false;
  c->d_cfwd.release(); c->d_crc.release(); c->d_clen.release(); c->d_adj_cnt.release();
  c->d_adj_off.release(); c->d_adj.release();
  c->cword_off.clear(); c->adj_off.clear(); c->clen.clear(); c->adj_cnt.clear();
  c->status.clear(); c->changes.clear(); c->adj.clear();
}

}  // namespace

extern "C" {

void co_params_init(co_params *p) {
  if (!p) return;
  p->error_rate = 0.06;          // correctOverlaps.H:271
}

const char *co_last_error(void) { return capi::g_err.c_str(); }
int co_abi_version(void) { return CO_ABI_VERSION; }

int co_ctx_create(const co_params *p, int device, co_ctx **out) {
  if (!out) return fail(CO_ERR_BAD_PARAM, "null out");
  *out = nullptr;
  if (int rc = check_params(p)) return rc;
  return capi::create_ctx(p, device, out);
}

void co_ctx_destroy(co_ctx *c) { capi::destroy_ctx(c); }

int co_set_params(co_ctx *c, const co_params *p) {
  if (!c) return fail(CO_ERR_BAD_PARAM, "null context");
  if (int rc = check_params(p)) return rc;
  c->P = *p;
  return CO_OK;
}

int co_load_reads_device(co_ctx *c, uint32_t first_iid, uint32_t nreads, const uint8_t *d_bases,
                         const uint64_t *d_offsets, const uint32_t *h_lengths) {
  if (!c) return fail(CO_ERR_BAD_PARAM, "null context");
  if (int rc = capi::check_device_reads(first_iid, nreads, d_bases, d_offsets, h_lengths)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  drop_corrections(c);
  return pack_reads<false>(c->reads, c->stream, 1, true, first_iid, nreads, d_bases, d_offsets,
                           h_lengths);
}

int co_load_reads(co_ctx *c, uint32_t first_iid, uint32_t nreads, const uint8_t *bases,
                  const uint64_t *offsets, const uint32_t *lengths) {
  if (!c) return fail(CO_ERR_BAD_PARAM, "null context");
  DevBuf<uint8_t> d_b;
  DevBuf<uint64_t> d_o;
  if (int rc = capi::stage_reads(c->device, nreads, bases, offsets, lengths, d_b, d_o)) return rc;
  return co_load_reads_device(c, first_iid, nreads, d_b.p, d_o.p, lengths);
}

int co_set_corrections(co_ctx *c, const fe_correction *red, uint64_t n) {
  if (!c) return fail(CO_ERR_BAD_PARAM, "null context");
  if (n && !red) return fail(CO_ERR_BAD_PARAM, "null corrections");
  HIP_TRY(hipSetDevice(c->device));
  drop_corrections(c);
  c->S.ms_correct = 0;
  const uint32_t nr = c->reads.nreads;
  for (uint64_t k = 1; k < n; k++)
    if (red[k].read_id < red[k - 1].read_id)
      return fail(CO_ERR_BAD_INPUT, "corrections are not ascending by read: record %llu is of read "
                  "%u, the one before of read %u", (unsigned long long)k, red[k].read_id,
                  red[k - 1].read_id);

  // a read's records: the first one is its IDENT record (correctRead :58-70), the rest follow
  std::vector<uint64_t> rec_first(nr, 0), cwoff(nr), adj_off(nr);
  std::vector<uint32_t> rec_cnt(nr, 0), status(nr, R_NO_IDENT);
  std::vector<uint32_t> nins(nr, 0);
  for (uint64_t k = 0; k < n;) {
    uint64_t e = k + 1;
    while (e < n && red[e].read_id == red[k].read_id) e++;
    const uint32_t id = red[k].read_id;
    if (id >= c->reads.first_iid && id - c->reads.first_iid < nr && ((red[k].word >> 2) & 15) == V_IDENT) {
      const uint32_t r = id - c->reads.first_iid;
      status[r] = R_OK;
      rec_first[r] = k + 1;
      rec_cnt[r] = (uint32_t)std::min<uint64_t>(e - k - 1, 0xffffffffull);
    }
    k = e;
  }
  uint64_t words = 0, nadj = 0, max_len = 0, max_out = 0;
  for (uint32_t r = 0; r < nr; r++) {
    uint64_t ins = 0, indel = 0;
    for (uint64_t k = rec_first[r]; k < rec_first[r] + rec_cnt[r]; k++) {
      const uint32_t t = (red[k].word >> 2) & 15;
      ins += t >= V_A_INSERT && t <= V_T_INSERT;
      indel += t == V_DELETE || (t >= V_A_INSERT && t <= V_T_INSERT);
    }
    cwoff[r] = words;
    words += (c->reads.len[r] + ins + 15) / 16 + PAD_WORDS;
    adj_off[r] = nadj;
    nadj += indel;
    max_len = std::max<uint64_t>(max_len, c->reads.len[r]);
    max_out = std::max<uint64_t>(max_out, c->reads.len[r] + ins);
    if (c->reads.len[r] + ins > 0x7ffffff0ull)
      return fail(CO_ERR_BAD_INPUT, "read %u: %llu insertions", c->reads.first_iid + r, (unsigned long long)ins);
  }
  max_out += 1;

  DevBuf<fe_correction> d_red;
  DevBuf<uint64_t> d_rec_first, d_cwoff;
  DevBuf<uint32_t> d_rec_cnt, d_status, d_changes;
  DevBuf<int32_t> d_delta;
  DevBuf<uint8_t> d_op, d_cb;
  HIP_TRY(d_red.alloc(n));
  HIP_TRY(d_rec_first.alloc(nr));
  HIP_TRY(d_cwoff.alloc(nr));
  HIP_TRY(d_rec_cnt.alloc(nr));
  HIP_TRY(d_status.alloc(nr));
  HIP_TRY(d_changes.alloc(3ull * nr));
  HIP_TRY(c->d_cfwd.alloc(words));
  HIP_TRY(c->d_crc.alloc(words));
  HIP_TRY(c->d_clen.alloc(nr));
  HIP_TRY(c->d_adj_cnt.alloc(nr));
  HIP_TRY(c->d_adj_off.alloc(nr));
  HIP_TRY(c->d_adj.alloc(nadj));
  c->clen.assign(nr, 0);
  c->adj_cnt.assign(nr, 0);
  c->changes.assign(3ull * nr, 0);
  c->adj.assign(nadj, Adjust{0, 0});
  if (nr) {
    // a work area per block, sized for the longest read: no more blocks than fit the budget
    const uint64_t per_block = (max_len + 1) * 4 + max_len + max_out;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>({(uint64_t)nr, (uint64_t)c->n_cu * 8, CORRECT_BUDGET / per_block}));
    HIP_TRY(d_delta.alloc((max_len + 1) * grid));
    HIP_TRY(d_op.alloc(max_len * grid));
    HIP_TRY(d_cb.alloc(max_out * grid));
    if (n) HIP_TRY(hipMemcpyAsync(d_red.p, red, n * sizeof(fe_correction), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_rec_first.p, rec_first.data(), nr * 8ull, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_cwoff.p, cwoff.data(), nr * 8ull, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_rec_cnt.p, rec_cnt.data(), nr * 4ull, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_status.p, status.data(), nr * 4ull, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->d_adj_off.p, adj_off.data(), nr * 8ull, hipMemcpyHostToDevice, c->stream));
    CorrectArgs X{};
    X.ofwd = c->reads.fwd.p; X.oword_off = c->reads.d_word_off.p; X.len = c->reads.d_len.p; X.nreads = nr;
    X.red = d_red.p; X.rec_first = d_rec_first.p; X.rec_cnt = d_rec_cnt.p;
    X.delta = d_delta.p; X.op = d_op.p; X.cbytes = d_cb.p; X.max_len = max_len; X.max_out = max_out;
    X.cfwd = c->d_cfwd.p; X.crc = c->d_crc.p; X.cword_off = d_cwoff.p; X.clen = c->d_clen.p;
    X.adj = c->d_adj.p; X.adj_off = c->d_adj_off.p; X.adj_cnt = c->d_adj_cnt.p;
    X.status = d_status.p; X.changes = d_changes.p;
    Event e0, e1;
    HIP_TRY(e0.create());
    HIP_TRY(e1.create());
    HIP_TRY(hipEventRecord(e0, c->stream));
    hipLaunchKernelGGL(k_co_correct, dim3(grid), dim3(256), 0, c->stream, X);
    hipError_t le = hipGetLastError();
    HIP_TRY(hipEventRecord(e1, c->stream));
    hipError_t se = hipStreamSynchronize(c->stream);
    HIP_TRY(le);
    HIP_TRY(se);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    c->S.ms_correct = ms;
    HIP_TRY(hipMemcpy(c->clen.data(), c->d_clen.p, nr * 4ull, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c->adj_cnt.data(), c->d_adj_cnt.p, nr * 4ull, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(status.data(), d_status.p, nr * 4ull, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c->changes.data(), d_changes.p, 3ull * nr * 4, hipMemcpyDeviceToHost));
    if (nadj) HIP_TRY(hipMemcpy(c->adj.data(), c->d_adj.p, nadj * sizeof(Adjust), hipMemcpyDeviceToHost));
  }
  c->cword_off = std::move(cwoff);
  c->adj_off = std::move(adj_off);
  c->status = std::move(status);
  c->corrected = true;
  return CO_OK;
}

int co_correct_overlaps(co_ctx *c, uint32_t bgn_id, uint32_t end_id, const ovl_record *ov, uint64_t n,
                        uint16_t *evalues) {
  if (!c) return fail(CO_ERR_BAD_PARAM, "null context");
  if (n && (!ov || !evalues)) return fail(CO_ERR_BAD_PARAM, "null overlaps or evalues");
  if (n > 0xfffffff0ull) return fail(CO_ERR_BAD_PARAM, "more than 2^32 overlaps in one call");
  const double ms_correct = c->S.ms_correct;
  c->S = co_stats{};
  c->S.ms_correct = ms_correct;
  c->evalues.clear();
  if (!c->corrected) return fail(CO_ERR_STATE, "no corrections: call co_set_corrections first");
  if (bgn_id > end_id || bgn_id < c->reads.first_iid || end_id - c->reads.first_iid >= c->reads.nreads)
    return fail(CO_ERR_BAD_INPUT, "range %u-%u is not within the loaded reads %u-%u", bgn_id,
                end_id, c->reads.first_iid, c->reads.first_iid + c->reads.nreads - 1);
  HIP_TRY(hipSetDevice(c->device));
  const double erate = c->P.error_rate;
  const uint64_t HM = (1ull << 21) - 1;

  auto refused = [&](uint32_t id) -> int {
    const uint32_t st = c->status[id - c->reads.first_iid];
    if (st == R_NO_IDENT)
      return fail(CO_ERR_BAD_INPUT, "read %u has no IDENT record among the corrections", id);
    if (st == R_BAD_POSITION)
      return fail(CO_ERR_BAD_INPUT, "read %u: a correction that is not at the position the one "
                  "before left, or of no vote type", id);
    return CO_OK;
  };

  // Correct_Frags wants every read of the range (:287-296)
  for (uint32_t id = bgn_id; id <= end_id; id++) {
    if (int rc = refused(id)) return rc;
    const uint32_t r = id - c->reads.first_iid;
    c->S.corrected_bases += (uint64_t)c->clen[r] + 1;
    c->S.substitutions += c->changes[3ull * r];
    c->S.deletions += c->changes[3ull * r + 1];
    c->S.insertions += c->changes[3ull * r + 2];
    if (id == 0xffffffffu) break;
  }

  std::vector<Job> jobs(n);
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t a = ov[i].a_iid, b = ov[i].b_iid;
    if (a < bgn_id || a > end_id)
      return fail(CO_ERR_BAD_INPUT, "overlap %llu: a_iid %u is outside the range %u-%u",
                  (unsigned long long)i, a, bgn_id, end_id);
    if (b < c->reads.first_iid || b - c->reads.first_iid >= c->reads.nreads)
      return fail(CO_ERR_BAD_INPUT, "overlap %llu names read %u, not loaded",
                  (unsigned long long)i, b);
    if (int rc = refused(b)) return rc;
    const uint32_t ar = a - c->reads.first_iid, br = b - c->reads.first_iid;
    const int64_t a5 = ov[i].dat[0] & HM, b5 = ov[i].dat[1] & HM;
    const bool flipped = (ov[i].dat[0] >> 54) & 1;
    const int64_t a_hang = a5 - b5;                            // ovOverlap.H:227
    const int64_t al = c->clen[ar], bl = c->clen[br];
    Job &J = jobs[i];
    J.a_word = c->cword_off[ar];
    J.b_word = c->cword_off[br];
    J.a_read = ar;
    J.b_read = br;
    J.a_hang = (int32_t)a_hang;
    J.a_off = J.b_off = 0;
    if (a_hang > 0)
      J.a_off = hang_adjust_host(c->adj.data() + c->adj_off[ar], (int)c->adj_cnt[ar], (int)a_hang,
                                 false, (int)al);
    if (a_hang < 0)
      J.b_off = hang_adjust_host(c->adj.data() + c->adj_off[br], (int)c->adj_cnt[br], (int)-a_hang,
                                 flipped, (int)bl);
    if (J.a_off < 0 || J.a_off > al || J.b_off < 0 || J.b_off > bl)
      return fail(CO_ERR_BAD_INPUT, "overlap %llu: a_hang %lld, adjusted to %d, is beyond its "
                  "corrected read (%u: %lld bases, %u: %lld bases)", (unsigned long long)i,
                  (long long)a_hang, a_hang > 0 ? J.a_off : J.b_off, a, (long long)al, b,
                  (long long)bl);
    J.m = (int32_t)al - J.a_off;
    J.n = (int32_t)bl - J.b_off;
    J.limit = (int32_t)ceil((double)std::min(J.m, J.n) * erate);   // correctOverlaps.C:135-136
    J.b_rc = flipped;
    J.pad = 0;
    c->S.bases += (uint64_t)std::min(J.m, J.n);
  }

  c->bgn_id = bgn_id;
  c->end_id = end_id;
  if (n == 0) return CO_OK;

  DevBuf<int32_t> d_errors, d_olen;
  DevBuf<unsigned long long> d_counters;
  HIP_TRY(d_errors.alloc(n));
  HIP_TRY(d_olen.alloc(n));
  HIP_TRY(d_counters.alloc(NCOUNT));
  HIP_TRY(hipMemsetAsync(d_errors.p, 0, n * 4, c->stream));
  HIP_TRY(hipMemsetAsync(d_olen.p, 0, n * 4, c->stream));
  HIP_TRY(hipMemsetAsync(d_counters.p, 0, NCOUNT * sizeof(unsigned long long), c->stream));

  const AlignStage stage{"CANU_CO_LOG_PER_ERROR", "CANU_CO_LOG_CAP", CO_LOG_PER_ERROR, 0, 0, F_DONE,
                         "the device adjusted its hang differently"};
  std::vector<uint32_t> fl;
  AlignStats A;
  const int rc = align_all(*c, stage, c->ml, erate, jobs, [&](const AlignLaunch<Job> &L) {
    AlignArgs X{};
    X.fwd = c->d_cfwd.p; X.rc = c->d_crc.p; X.jobs = L.jobs; X.order = L.order;
    X.njobs = L.njobs; X.nwaves = L.nwaves; X.next = L.next;
    X.flags = L.flags; X.rows = L.rows; X.errors = d_errors.p; X.olap_len = d_olen.p;
    X.counters = d_counters.p; X.adj = c->d_adj.p; X.adj_off = c->d_adj_off.p;
    X.adj_cnt = c->d_adj_cnt.p; X.clen = c->d_clen.p; X.match_limit = L.match_limit;
    X.scratch = L.scratch; X.log_cap = L.log_cap; X.per_wave = L.per_wave; X.max_limit = L.max_limit;
    hipLaunchKernelGGL(k_co_align, dim3(L.blocks), dim3(64 * WAVES_PER_BLOCK), 0, c->stream, X);
    return hipGetLastError();
  }, fl, A);
  c->S.n_generic = A.n_generic; c->S.n_staged = A.n_staged; c->S.rows = A.rows;
  c->S.regrows = A.regrows; c->S.scratch_bytes = A.scratch_bytes; c->S.ms_align = A.ms_align;
  if (rc) return rc;

  std::vector<int32_t> errors(n), olen(n);
  unsigned long long cnt[NCOUNT];
  HIP_TRY(hipMemcpy(errors.data(), d_errors.p, n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(olen.data(), d_olen.p, n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cnt, d_counters.p, sizeof cnt, hipMemcpyDeviceToHost));
  c->S.olaps_fwd = cnt[C_FWD]; c->S.olaps_rev = cnt[C_REV]; c->S.total = cnt[C_TOTAL];
  c->S.failed_both = cnt[C_BOTH]; c->S.failed_either = cnt[C_EITHER]; c->S.failed_end = cnt[C_END];
  c->S.failed_length = cnt[C_LENGTH]; c->S.rha_fail = cnt[C_RHA_FAIL]; c->S.rha_pass = cnt[C_RHA_PASS];
  c->evalues.resize(n);
  for (uint64_t i = 0; i < n; i++) {
    if (!(fl[i] & F_TO_END) || olen[i] <= 0) {                 // :485-516: the evalue stays
      c->evalues[i] = (uint16_t)((ov[i].dat[0] >> 42) & 0xfff);
    } else {                                                   // :521, ovOverlap.H:44-45
      const double q = (double)errors[i] / olen[i];
      c->evalues[i] = (uint16_t)(q < AS_MAX_EVALUE / 10000.0 ? (int)(10000.0 * q + 0.5) : AS_MAX_EVALUE);
    }
    evalues[i] = c->evalues[i];
  }
  return CO_OK;
}

int co_write_oea(co_ctx *c, const char *path) {
  if (!c || !path) return fail(CO_ERR_BAD_PARAM, "null context or path");
  FILE *f = fopen(path, "wb");
  if (!f) return fail(CO_ERR_BAD_PARAM, "can't open '%s' for writing: %s", path, strerror(errno));
  const int32_t ids[2] = {(int32_t)c->bgn_id, (int32_t)c->end_id};     // correctOverlaps.C:203-215
  const uint64_t n = c->evalues.size();
  size_t w = fwrite(ids, 4, 2, f) + fwrite(&n, 8, 1, f);
  if (n) w += fwrite(c->evalues.data(), 2, n, f);
  if (fclose(f) != 0 || w != 3 + n)
    return fail(CO_ERR_BAD_PARAM, "short write to '%s'", path);
  return CO_OK;
}

int co_get_stats(const co_ctx *c, co_stats *out) {
  if (!c || !out) return fail(CO_ERR_BAD_PARAM, "null context or out");
  *out = c->S;
  return CO_OK;
}

}  // extern "C"
