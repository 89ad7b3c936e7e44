// pair.hip -- libcanu_pair.so: canu's overlapPair (src/overlapInCore/overlapPair.C) on gfx950.
//
// One wave owns one overlap and runs recomputeOverlaps (:346-662) on the device: up to 13
// dependent edit-distance passes (edlibAlign, restated in include/canu_pair.h) with the hang
// arithmetic between them, so nothing goes back to the host between passes.
//
// The passes are edlib_wave.h's: a wave_locate per extension, a global dp_pass at the end, over
// five symbols (A, C, G, T, N) and with nothing kept but the bottom row.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../include/canu_pair.h"
#include "capi_common.h"
#include "edlib_launch.h"

namespace {

using capi::fail;
using edw::LDS_WORDS;
using edw::Span;
using edw::uni;
using edw::WAVES_PER_BLOCK;

CAPI_SAME_CODES(PAIR);
static_assert(PAIR_STRIPE_ROWS == edw::STRIPE_ROWS && PAIR_LDS_COLUMNS == edw::LDS_COLUMNS,
              "canu_pair.h names the aligner's stripe and LDS row");
constexpr int MHAP_SLOP = 500;                         // overlapPair.C:64
constexpr uint32_t MAX_EVALUE = 4095;                  // AS_MAX_EVALUE, ovOverlap.H:42

// per-overlap outcome bits, summed on the host into alignStats' counters
enum : uint32_t {
  F_SKIPPED = 1u << 0, F_PASSED = 1u << 1, F_FAILED = 1u << 2, F_FAILEXTA = 1u << 3,
  F_FAILEXTB = 1u << 4, F_FAILEXT = 1u << 5, F_PARTIAL = 1u << 6, F_DOVETAIL = 1u << 7,
  F_EXT5B = 1u << 8, F_EXT5A = 1u << 9, F_EXT3A = 1u << 10, F_EXT3B = 1u << 11
};

struct ReadTable {
  const uint8_t *fwd;        // codes 0..3 = ACGT, 4 = N, read r at off[r]
  const uint8_t *rc;         // the reverse complement of every read, same offsets
  const uint64_t *off;
  const uint32_t *len;
  uint32_t first_iid, nreads;
};

struct WaveCtx {
  uint32_t *lrow, *grow;
  double erate;
  unsigned long long cells;
  unsigned long long steps;   // wavefront steps: columns + lanes - 1 per stripe
  uint32_t passes;
};

__device__ __forceinline__ int max_edit(int a, int b, double erate) {
  return (int)ceil(max(a, b) * erate * 1.1);
}

// extendAlignment (overlapPair.C:255-304): Q[qb,qe) is the query, T[tb,te) widened by slop
// the target; on success tb/te move to the alignment found.
__device__ bool extend_alignment(WaveCtx &w, const Span Q, int qb, int qe, const Span T, int &tb,
                                 int &te, int slop, int &edit_dist, int &align_len) {
  const int tbx = max(0, tb - slop);
  const int tex = min(T.n, te + slop);
  const int m = qe - qb, n = tex - tbx;
  if (m <= 0 || n <= 0) return false;           // cannot happen with min_overlap_length >= 1
  const edw::Located L = edw::wave_locate<5>(Q.sub(qb, m), T.sub(tbx, n), max_edit(m, n, w.erate),
                                             true, w.lrow, w.grow);
  w.cells += L.cells;
  w.steps += L.steps;
  w.passes += L.passes;
  if (!L.ok) return false;
  tb = tbx + L.start;
  te = tbx + L.end + 1;
  edit_dist = L.dist;
  align_len = (m + (te - tb) + L.dist) / 2;
  return true;
}

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK, 8)
void k_pair(const ReadTable R, const ovl_record *__restrict__ in, const uint32_t *__restrict__ order,
            const uint32_t n_olaps, ovl_record *__restrict__ out, uint32_t *__restrict__ flags_out,
            unsigned long long *__restrict__ cells_out,
            unsigned long long *__restrict__ steps_out, uint32_t *__restrict__ passes_out,
            uint32_t *__restrict__ scratch,
            const uint64_t scratch_words, const double erate, const uint32_t min_len,
            const int partial, const int invert) {
  __shared__ uint32_t s_row[WAVES_PER_BLOCK][LDS_WORDS];
  const int lane = threadIdx.x & 63;
  const int wave = uni((int)(threadIdx.x >> 6));
  const uint64_t gw = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave;   // uniform: see `wave`
  WaveCtx w;
  w.lrow = s_row[wave];
  w.grow = scratch ? scratch + gw * scratch_words : nullptr;
  w.erate = erate;
  const uint64_t HM = (1ull << 21) - 1;

  // Overlaps come longest first in `order`; wave g takes slots g, g + waves, ... (the slot
  // arithmetic is scalar: nothing in this loop depends on the lane)
  const uint32_t n_waves = gridDim.x * WAVES_PER_BLOCK;
  for (uint32_t slot = (uint32_t)gw; slot < n_olaps; slot += n_waves) {
    const uint32_t oi = (uint32_t)uni((int)order[slot]);
    w.cells = 0;
    w.steps = 0;
    w.passes = 0;

    uint32_t a_iid = (uint32_t)uni((int)in[oi].a_iid), b_iid = (uint32_t)uni((int)in[oi].b_iid);
    const uint64_t d0 = in[oi].dat[0], d1 = in[oi].dat[1];
    int ahg5 = uni((int)(d0 & HM)), ahg3 = uni((int)((d0 >> 21) & HM));
    int bhg5 = uni((int)(d1 & HM)), bhg3 = uni((int)((d1 >> 21) & HM));
    const uint32_t d0_hi = (uint32_t)uni((int)(d0 >> 32));    // evalue 10.., flipped 22, flags
    const uint32_t d1_hi = (uint32_t)uni((int)(d1 >> 32));
    const uint32_t d1_lo = (uint32_t)uni((int)d1);
    const bool flipped = (d0_hi >> 22) & 1;
    if (invert) {                                             // ovOverlap::swapIDs
      const uint32_t ti = a_iid; a_iid = b_iid; b_iid = ti;
      const int o_a5 = ahg5, o_a3 = ahg3, o_b5 = bhg5, o_b3 = bhg3;
      if (!flipped) { ahg5 = o_b5; ahg3 = o_b3; bhg5 = o_a5; bhg3 = o_a3; }
      else          { ahg5 = o_b3; ahg3 = o_b5; bhg5 = o_a3; bhg3 = o_a5; }
    }
    const uint32_t ra = a_iid - R.first_iid, rb = b_iid - R.first_iid;   // checked on the host
    const int alen = uni((int)R.len[ra]), blen = uni((int)R.len[rb]);
    const Span A{R.fwd + R.off[ra], alen};
    const Span B{(flipped ? R.rc : R.fwd) + R.off[rb], blen};

    int abgn = ahg5, aend = alen - ahg3, bbgn = bhg5, bend = blen - bhg3;
    int align_len = 1, edit_dist = INT_MAX;
    uint32_t fl = 0;
    // the record's hangs, as the reference keeps them in *ovl, and the working copies of the
    // dovetail extensions (:487-491)
    int r_a5 = ahg5, r_a3 = ahg3, r_b5 = bhg5, r_b3 = bhg3;
    int a5 = 0, a3 = 0, b5 = 0, b3 = 0;

    // recomputeOverlaps as seven steps, so that the aligner is inlined once: the two initial
    // alignments, the four dovetail extensions in the reference's order, finalAlignment
    enum { INIT_A, INIT_B, EXT5B, EXT5A, EXT3A, EXT3B, FINAL, N_STEPS };
    bool live = true;
    if ((uint32_t)(aend - abgn) < min_len || (uint32_t)(bend - bbgn) < min_len) {
      fl |= F_SKIPPED;
      live = false;
    }
    for (int step = INIT_A; step < N_STEPS && live; step++) {
      bool run = true, q_is_b = false;
      int slop = 100;                           // (a hang already zeroed) * erate + 100
      switch (step) {
        case INIT_A: q_is_b = true; slop = MHAP_SLOP; break;
        case INIT_B: q_is_b = false; slop = MHAP_SLOP; break;
        case EXT5B:
          run = a5 >= b5 && b5 > 0;
          if (run) { a5 -= b5; b5 = 0; q_is_b = true; }
          break;
        case EXT5A:
          run = b5 >= a5 && a5 > 0;
          if (run) { b5 -= a5; a5 = 0; q_is_b = false; }
          break;
        case EXT3A:
          run = b3 >= a3 && a3 > 0;
          if (run) { b3 -= a3; a3 = 0; q_is_b = false; }
          break;
        case EXT3B:
          run = a3 >= b3 && b3 > 0;
          if (run) { a3 -= b3; b3 = 0; q_is_b = true; }
          break;
        default: break;
      }
      if (step == FINAL) {
        r_a5 = a5; r_a3 = a3; r_b5 = b5; r_b3 = b3;
        // finalAlignment (:308-341): global, over the record's spans
        const int fa = r_a5, fe = alen - r_a3, fb = r_b5, fbe = blen - r_b3;
        const int m = fe - fa, n = fbe - fb;
        if (m > 0 && n > 0) {
          const int k = max_edit(m, n, erate);
          const edw::PassOut g = edw::dp_pass<5>(A.sub(fa, m).fwd(), B.sub(fb, n).fwd(), 1, INT_MIN,
                                                 w.lrow, w.grow, edw::NoKeep{});
          w.cells += (unsigned long long)m * n;
          w.steps += g.steps;
          w.passes++;
          const int ed = uni(g.fin);
          if (ed <= k) { edit_dist = ed; align_len = (m + n + ed) / 2; }
        }
        continue;
      }
      if (!run) continue;
      if (step >= EXT5B) { abgn = a5; aend = alen - a3; bbgn = b5; bend = blen - b3; }
      bool ok;
      if (q_is_b) ok = extend_alignment(w, B, bbgn, bend, A, abgn, aend, slop, edit_dist, align_len);
      else        ok = extend_alignment(w, A, abgn, aend, B, bbgn, bend, slop, edit_dist, align_len);
      switch (step) {
        case INIT_A: if (!ok) fl |= F_FAILEXTA; break;
        case INIT_B:
          if (!ok) fl |= F_FAILEXTB;
          if (align_len == 1) {
            fl |= F_FAILEXT;
            live = false;
          } else {
            r_a5 = abgn; r_a3 = alen - aend; r_b5 = bbgn; r_b3 = blen - bend;
            if (partial) {
              fl |= F_PARTIAL;
              live = false;
            } else if ((r_a5 == 0 || r_b5 == 0) && (r_a3 == 0 || r_b3 == 0)) {
              fl |= F_DOVETAIL;
              live = false;
            }
            a5 = r_a5; a3 = r_a3; b5 = r_b5; b3 = r_b3;
          }
          break;
        case EXT5B: if (ok) a5 = abgn; else { a5 = r_a5; b5 = r_b5; } fl |= F_EXT5B; break;
        case EXT5A: if (ok) b5 = bbgn; else { b5 = r_b5; a5 = r_a5; } fl |= F_EXT5A; break;
        case EXT3A: if (ok) b3 = blen - bend; else { b3 = r_b3; a3 = r_a3; } fl |= F_EXT3A; break;
        case EXT3B: if (ok) a3 = alen - aend; else { a3 = r_a3; b3 = r_b3; } fl |= F_EXT3B; break;
        default: break;
      }
    }
    const double e_rate = edit_dist / (double)align_len;
    uint32_t evalue = MAX_EVALUE, for_obt = 0, for_dup = 0, for_utg = 0;
    if ((uint32_t)align_len < min_len || e_rate > erate) {
      fl |= F_FAILED;
    } else {
      fl |= F_PASSED;
      evalue = e_rate < (MAX_EVALUE / 10000.0) ? (uint32_t)(int)(10000.0 * e_rate + 0.5) : MAX_EVALUE;
      evalue &= MAX_EVALUE;
      for_obt = for_dup = partial ? 1 : 0;
      for_utg = (!partial && (r_a5 == 0 || r_b5 == 0) && (r_a3 == 0 || r_b3 == 0)) ? 1 : 0;
    }
    // dat[0]: ahg5:21 ahg3:21 evalue:12 flipped forOBT forDUP forUTG extra1:6
    const uint64_t o0 = ((uint64_t)r_a5 & HM) | (((uint64_t)r_a3 & HM) << 21) |
                        ((uint64_t)evalue << 42) | ((uint64_t)(flipped ? 1 : 0) << 54) |
                        ((uint64_t)for_obt << 55) | ((uint64_t)for_dup << 56) |
                        ((uint64_t)for_utg << 57) | ((uint64_t)(d0_hi >> 26) << 58);
    // dat[1]: bhg5:21 bhg3:21 span:21 extra2:1 -- span and extra2 are carried over
    const uint64_t keep1 = (((uint64_t)d1_hi << 32) | d1_lo) & ~((1ull << 42) - 1);
    const uint64_t o1 = ((uint64_t)r_b5 & HM) | (((uint64_t)r_b3 & HM) << 21) | keep1;
    // every lane holds the same values and stores them: no lane-dependent branch in this loop
    out[oi].a_iid = a_iid;
    out[oi].b_iid = b_iid;
    out[oi].dat[0] = o0;
    out[oi].dat[1] = o1;
    flags_out[oi] = fl;
    cells_out[oi] = w.cells;
    steps_out[oi] = w.steps;
    passes_out[oi] = w.passes;
  }
}

}  // namespace

// ------------------------------------------------------------------ host

struct pair_ctx : capi::Device {
  pair_params P{};
  edw::Strands R;
  pair_stats S{};
};

namespace {

int check_params(const pair_params *p) {
  if (!p) return fail(PAIR_ERR_BAD_PARAM, "null parameters");
  if (!(p->max_erate >= 0.0) || p->max_erate > 1.0)
    return fail(PAIR_ERR_BAD_PARAM, "max_erate %g outside [0, 1]", p->max_erate);
  if (p->min_overlap_length == 0)
    return fail(PAIR_ERR_BAD_PARAM, "min_overlap_length 0 is not supported: the reference "
                                    "aligns empty spans there; use 1 or more");
  return PAIR_OK;
}

}  // namespace

extern "C" {

void pair_params_init(pair_params *p) {
  if (!p) return;
  p->max_erate = 0.12;          // overlapPair.C:680
  p->min_overlap_length = 1;    // the reference's default 0 is refused
  p->partial = 0;
  p->invert = 0;
}

const char *pair_last_error(void) { return capi::g_err.c_str(); }
int pair_abi_version(void) { return PAIR_ABI_VERSION; }

int pair_ctx_create(const pair_params *p, int device, pair_ctx **out) {
  if (!out) return fail(PAIR_ERR_BAD_PARAM, "null out");
  *out = nullptr;
  if (int rc = check_params(p)) return rc;
  return capi::create_ctx(p, device, out);
}

void pair_ctx_destroy(pair_ctx *c) { capi::destroy_ctx(c); }

int pair_set_params(pair_ctx *c, const pair_params *p) {
  if (!c) return fail(PAIR_ERR_BAD_PARAM, "null context");
  if (int rc = check_params(p)) return rc;
  c->P = *p;
  return PAIR_OK;
}

int pair_load_reads_device(pair_ctx *c, uint32_t first_iid, uint32_t nreads,
                           const uint8_t *d_bases, const uint64_t *d_offsets,
                           const uint32_t *h_lengths) {
  if (!c) return fail(PAIR_ERR_BAD_PARAM, "null context");
  if (int rc = capi::check_device_reads(first_iid, nreads, d_bases, d_offsets, h_lengths)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  return edw::load_strands(c->R, c->stream, true, first_iid, nreads, d_bases, d_offsets, h_lengths);
}

int pair_load_reads(pair_ctx *c, uint32_t first_iid, uint32_t nreads, const uint8_t *bases,
                    const uint64_t *offsets, const uint32_t *lengths) {
  if (!c) return fail(PAIR_ERR_BAD_PARAM, "null context");
  DevBuf<uint8_t> d_b;
  DevBuf<uint64_t> d_o;
  if (int rc = capi::stage_reads(c->device, nreads, bases, offsets, lengths, d_b, d_o)) return rc;
  return pair_load_reads_device(c, first_iid, nreads, d_b.p, d_o.p, lengths);
}

int pair_realign(pair_ctx *c, const ovl_record *in, uint64_t n, ovl_record *out) {
  if (!c) return fail(PAIR_ERR_BAD_PARAM, "null context");
  if (n && (!in || !out)) return fail(PAIR_ERR_BAD_PARAM, "null records");
  if (n > 0xfffffff0ull) return fail(PAIR_ERR_BAD_PARAM, "more than 2^32 overlaps in one call");
  c->S = pair_stats{};
  if (n == 0) return PAIR_OK;
  HIP_TRY(hipSetDevice(c->device));
  const uint64_t HM = (1ull << 21) - 1;
  // the checks the reference leaves out, and the cost estimate the order comes from
  std::vector<uint64_t> est(n);
  bool need_scratch = false;
  for (uint64_t i = 0; i < n; i++) {
    uint32_t a = in[i].a_iid, b = in[i].b_iid;
    uint64_t a5 = in[i].dat[0] & HM, a3 = (in[i].dat[0] >> 21) & HM;
    uint64_t b5 = in[i].dat[1] & HM, b3 = (in[i].dat[1] >> 21) & HM;
    if (c->P.invert) { std::swap(a, b); std::swap(a5, b5); std::swap(a3, b3); }
    if (a < c->R.first_iid || a - c->R.first_iid >= c->R.nreads || b < c->R.first_iid ||
        b - c->R.first_iid >= c->R.nreads)
      return fail(PAIR_ERR_BAD_INPUT, "overlap %llu names read %u or %u, not loaded",
                  (unsigned long long)i, a, b);
    const uint64_t al = c->R.len[a - c->R.first_iid], bl = c->R.len[b - c->R.first_iid];
    if (a5 + a3 > al || b5 + b3 > bl)
      return fail(PAIR_ERR_BAD_INPUT, "overlap %llu: hangs beyond its reads (%u: %llu+%llu of "
                  "%llu, %u: %llu+%llu of %llu)", (unsigned long long)i, a,
                  (unsigned long long)a5, (unsigned long long)a3, (unsigned long long)al, b,
                  (unsigned long long)b5, (unsigned long long)b3, (unsigned long long)bl);
    const uint64_t as = al - a5 - a3, bs = bl - b5 - b3;
    est[i] = bs * std::min<uint64_t>(al, as + 2 * MHAP_SLOP);
    // a dovetail extension can stretch a span to its whole read, so the reads decide
    if (std::max(al, bl) > PAIR_LDS_COLUMNS) need_scratch = true;
  }
  std::vector<uint32_t> order(n);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t x, uint32_t y) { return est[x] > est[y]; });

  const uint64_t max_blocks = (uint64_t)c->n_cu * 8;   // 8 waves per SIMD
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK,
                                                       max_blocks);
  const uint64_t scratch_words = need_scratch ? edw::grow_words(c->R.max_len) : 0;

  DevBuf<ovl_record> d_in, d_out;
  DevBuf<uint32_t> d_order, d_flags, d_passes, d_scratch;
  DevBuf<unsigned long long> d_cells, d_steps;
  HIP_TRY(d_in.alloc(n));
  HIP_TRY(d_out.alloc(n));
  HIP_TRY(d_order.alloc(n));
  HIP_TRY(d_flags.alloc(n));
  HIP_TRY(d_passes.alloc(n));
  HIP_TRY(d_cells.alloc(n));
  HIP_TRY(d_steps.alloc(n));
  if (scratch_words) HIP_TRY(d_scratch.alloc(scratch_words * blocks * WAVES_PER_BLOCK));
  HIP_TRY(hipMemcpyAsync(d_in.p, in, n * sizeof(ovl_record), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d_order.p, order.data(), n * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(d_flags.p, 0, n * 4, c->stream));

  ReadTable R{c->R.fwd.p, c->R.rc.p, c->R.d_off.p, c->R.d_len.p, c->R.first_iid, c->R.nreads};
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  HIP_TRY(hipEventRecord(e0, c->stream));
  hipLaunchKernelGGL(k_pair, dim3(blocks), dim3(64 * WAVES_PER_BLOCK), 0, c->stream, R, d_in.p,
                     d_order.p, (uint32_t)n, d_out.p, d_flags.p, d_cells.p, d_steps.p, d_passes.p,
                     d_scratch.p, scratch_words, c->P.max_erate, c->P.min_overlap_length,
                     c->P.partial ? 1 : 0, c->P.invert ? 1 : 0);
  hipError_t le = hipGetLastError();
  HIP_TRY(hipEventRecord(e1, c->stream));
  std::vector<ovl_record> h_out(n);
  std::vector<uint32_t> fl(n), ps(n);
  std::vector<unsigned long long> cells(n), steps(n);
  hipError_t se = hipStreamSynchronize(c->stream);
  float ms = 0;
  if (le == hipSuccess && se == hipSuccess) (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  HIP_TRY(le);
  HIP_TRY(se);
  HIP_TRY(hipMemcpy(h_out.data(), d_out.p, n * sizeof(ovl_record), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(fl.data(), d_flags.p, n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ps.data(), d_passes.p, n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cells.data(), d_cells.p, n * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(steps.data(), d_steps.p, n * 8, hipMemcpyDeviceToHost));
  memcpy(out, h_out.data(), n * sizeof(ovl_record));
  pair_stats &S = c->S;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t f = fl[i];
    if (!(f & (F_PASSED | F_FAILED)))
      return fail(PAIR_ERR_HIP, "overlap %llu was not processed", (unsigned long long)i);
    S.n_skipped += !!(f & F_SKIPPED);
    S.n_passed += !!(f & F_PASSED);
    S.n_failed += !!(f & F_FAILED);
    S.n_fail_ext_a += !!(f & F_FAILEXTA);
    S.n_fail_ext_b += !!(f & F_FAILEXTB);
    S.n_fail_ext += !!(f & F_FAILEXT);
    S.n_partial += !!(f & F_PARTIAL);
    S.n_dovetail += !!(f & F_DOVETAIL);
    S.n_ext5a += !!(f & F_EXT5A);
    S.n_ext3a += !!(f & F_EXT3A);
    S.n_ext5b += !!(f & F_EXT5B);
    S.n_ext3b += !!(f & F_EXT3B);
    S.dp_cells += cells[i];
    S.dp_steps += steps[i];
    S.dp_passes += ps[i];
  }
  S.scratch_bytes = scratch_words * 4 * blocks * WAVES_PER_BLOCK;
  S.ms_kernel = ms;
  return PAIR_OK;
}

int pair_get_stats(const pair_ctx *c, pair_stats *out) {
  if (!c || !out) return fail(PAIR_ERR_BAD_PARAM, "null argument");
  *out = c->S;
  return PAIR_OK;
}

}  // extern "C"
