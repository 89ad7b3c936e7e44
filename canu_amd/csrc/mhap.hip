// mhap.hip -- MHAP 2.1.2's sketch / two-stage filter on gfx950, behind include/canu_mhap.h.
//
// Replaces the MHAP jar canu runs for overlapper=mhap (src/pipelines/canu/OverlapMhap.pm:
// precompute :374-399, compare :476-498); the text line it writes is MatchResult.toString's,
// which src/mhap/mhapConvert.C:114-150 converts to ovOverlap records.  What the jar computes
// was read from its bytecode and is restated, method by method, in oracle/mhap_jar.py (the
// parity checker); the kernels below compute the same integers:
//
//   k_mh_ordered   one block per strand: BottomOverlapSketch -- Murmur3_x86_32 of every
//                  k'-mer's UTF-16 chars; the S smallest (hash, position) keys by a 4096-bin
//                  radix select (one histogram pass in practice, deeper digits when a bin
//                  overflows LDS), then a bitonic sort of the selected keys in LDS.
//   k_mh_keys      Murmur3_x64_128 h1 of every k-mer of every strand (the MinHash keys);
//                  a segmented radix sort (hipcub) makes each strand's keys runs: a run is a
//                  distinct k-mer, its length the count, its first value the first position.
//   k_mh_minhash   one block per strand over its sorted keys: per distinct k-mer the weight
//                  w (tf-idf), then for every hash function j, w xorshift64 draws of the
//                  k-mer's chain; the signed-smallest draw (earliest first occurrence on ties)
//                  stores the key's low / high 32 bits.  Integer-VALU bound (the draws).
//   index          (j, value) -> stored strand, hipcub radix sort, per-function offsets.
//   k_mh_candidates one wave per query: its forward row's H values looked up, matches counted
//                  per stored strand in an LDS table, the self / length rules of
//                  MinHashSearch.findMatches applied, >= min_matches emitted.
//   k_mh_compare   one wave per candidate: BottomOverlapSketch.getOverlapInfo.  The jar's
//                  sequential merge (recordMatchingKmers) decomposes into independent groups
//                  of equal hashes, so lanes take groups; the three medians are radix
//                  selects over regenerated records; the final bottom-sketch Jaccard merge is
//                  evaluated in closed form from per-group counts and prefix sums.
//
// One translation unit: the hashes are in mhap_hash.h, the shared constants, records and wave
// helpers in mhap_common.h, the kernels in mhap_sketch.hip and mhap_filter.hip, the host
// arithmetic in mhap_host.h (no HIP; tests/mhap_host_check.cpp runs it) and the context in
// mhap_ctx.h.  This file is the host sequence of each extern "C" function of canu_mhap.h.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/canu_mhap.h"
#include "../../include/canu_ovl.h"
#include "capi_common.h"
#include "mhap_common.h"

// the kernels, in the order that keeps the code object as it was in one file
#include "mhap_sketch.hip"
#include "mhap_filter.hip"

#include "mhap_host.h"

using namespace mh;
namespace host = mhap_host;
using capi::fail;

CAPI_SAME_CODES(OVL);             // canu_mhap.h: "same codes as canu_ovl.h"

#include "mhap_ctx.h"

// a refusal of mhap_host.h's checks
#define MHAP_CHECK(msg_expr)                                                   \
  do {                                                                         \
    const std::string m_ = (msg_expr);                                         \
    if (!m_.empty()) return fail(capi::ERR_BAD_PARAM, "%s", m_.c_str());       \
  } while (0)

extern "C" {

int mhap_abi_version(void) { return MHAP_ABI_VERSION; }
const char *mhap_last_error(void) { return capi::g_err.c_str(); }

void mhap_params_init(mhap_params *p) {
  p->k = 16;
  p->num_hashes = 512;
  p->min_matches = 3;
  p->ordered_sketch = 1536;
  p->ordered_k = 12;
  p->min_olap = 500;
  p->threshold = 0.78;
  p->max_shift = 0.2;
  p->min_store = 0;
  p->no_rc = 0;
}

void mhap_weighting_init(mhap_weighting *w) {
  w->repeat_weight = 0.9;
  w->repeat_idf_scale = 3.0;
  w->filter_threshold = 1e-5;
  w->no_tf = 0;
  w->supress_noise = 0;
}

// what a new context holds on its device: events, counters, the complement table
// (Utils$Translate) and the acceptance bits
static int init_ctx(mhap_ctx *c) {
  for (auto &e : c->ev)
    if (e.create() != hipSuccess) return fail(capi::ERR_HIP, "stream/event creation failed");
  if (c->ctr.reserve(16) != hipSuccess || c->kctr.reserve(2) != hipSuccess)
    return fail(capi::ERR_OOM, "counters");
  if (hipMemcpyToSymbol(HIP_SYMBOL(c_comp), COMP_MAP.to, 256) != hipSuccess)
    return fail(capi::ERR_HIP, "complement table");
  const std::vector<uint32_t> bits =
      host::accept_bits(c->P.ordered_sketch, (int)c->P.ordered_k, c->P.threshold);
  c->pass_empty = host::pass_empty((int)c->P.ordered_k, c->P.threshold);
  if (c->pass.reserve(bits.size()) != hipSuccess ||
      hipMemcpy(c->pass.p, bits.data(), 4 * bits.size(), hipMemcpyHostToDevice) != hipSuccess)
    return fail(capi::ERR_OOM, "acceptance table");
  return capi::OK;
}

void mhap_ctx_destroy(mhap_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  capi::destroy_ctx(c);
}

int mhap_ctx_create(const mhap_params *p, int device, mhap_ctx **out) {
  *out = nullptr;
  MHAP_CHECK(host::check_params(p));
  mhap_ctx *c = nullptr;
  if (int rc = capi::create_ctx(p, device, &c, hipStreamNonBlocking)) return rc;
  if (int rc = init_ctx(c)) {
    mhap_ctx_destroy(c);
    return rc;
  }
  *out = c;
  return capi::OK;
}

static int alloc_sketches(mhap_ctx *c) {
  const size_t n = 2ull * c->nreads;
  if (c->minhash.reserve(n * c->P.num_hashes) || c->ordered.reserve(n * c->P.ordered_sketch) ||
      c->ocount.reserve(n))
    return fail(capi::ERR_OOM, "sketch arrays for %u reads", c->nreads);
  HIP_TRY(hipMemsetAsync(c->ocount.p, 0, 4 * n, c->stream));
  c->indexed = false;
  return capi::OK;
}

static int set_lengths(mhap_ctx *c, uint32_t first_iid, uint32_t nreads, const uint32_t *lens) {
  if (first_iid == 0) return fail(capi::ERR_BAD_PARAM, "gkStore IDs start at 1");
  if (nreads >= 0x7FFFFFF0u) return fail(capi::ERR_BAD_PARAM, "too many reads");
  for (uint32_t i = 0; i < nreads; i++)
    if (lens[i] >= 0x7FFFFFFFu)
      return fail(capi::ERR_BAD_INPUT, "read %u too long", first_iid + i);
  c->first_iid = first_iid;
  c->nreads = nreads;
  c->h_len.assign(lens, lens + nreads);
  if (c->d_len.reserve(nreads)) return fail(capi::ERR_OOM, "lengths");
  HIP_TRY(hipMemcpyAsync(c->d_len.p, lens, 4ull * nreads, hipMemcpyHostToDevice, c->stream));
  return alloc_sketches(c);
}

int mhap_load_reads(mhap_ctx *c, uint32_t first_iid, uint32_t nreads, const uint8_t *bases,
                    const uint64_t *offsets, const uint32_t *lengths) {
  if (!c) return fail(capi::ERR_STATE, "null context");
  if (nreads && (!bases || !offsets || !lengths))
    return fail(capi::ERR_BAD_PARAM, "null read buffers");
  HIP_TRY(hipSetDevice(c->device));
  uint64_t total = 0;
  for (uint32_t i = 0; i < nreads; i++)
    total = std::max<uint64_t>(total, offsets[i] + lengths[i]);
  // 64 bytes of slack behind the bases (capi::stage_reads allocates none: not used here)
  if (c->bases_own.reserve(total + 64) || c->off_own.reserve(nreads))
    return fail(capi::ERR_OOM, "reads (%llu bytes)", (unsigned long long)total);
  HIP_TRY(hipMemcpyAsync(c->bases_own.p, bases, total, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->off_own.p, offsets, 8ull * nreads, hipMemcpyHostToDevice, c->stream));
  c->d_bases = c->bases_own.p;
  c->d_off = c->off_own.p;
  int rc = set_lengths(c, first_iid, nreads, lengths);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return capi::OK;
}

int mhap_load_reads_device(mhap_ctx *c, uint32_t first_iid, uint32_t nreads,
                           const uint8_t *d_bases, const uint64_t *d_offsets,
                           const uint32_t *h_lengths) {
  if (!c) return fail(capi::ERR_STATE, "null context");
  HIP_TRY(hipSetDevice(c->device));
  c->d_bases = d_bases;
  c->d_off = d_offsets;
  int rc = set_lengths(c, first_iid, nreads, h_lengths);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return capi::OK;
}

int mhap_set_weighting(mhap_ctx *c, const mhap_weighting *w) {
  if (!c) return fail(capi::ERR_STATE, "null context");
  MHAP_CHECK(host::check_weighting(w));
  c->W = *w;
  c->has_table = false;                 // no -f: no FrequencyCounts, so no keepKmer either
  c->has_bloom = false;
  return capi::OK;
}

int mhap_set_kmer_frequencies(mhap_ctx *c, const char *kmers, const double *fractions,
                              uint64_t n, const mhap_weighting *w) {
  return mhap_set_kmer_frequencies_ex(c, kmers, fractions, n, n, w);
}

// FrequencyCounts (mhap_host.h freq_table); with --supress-noise 1 also its Bloom filter of
// every line's key.  removeUnique 2 builds the filter and never reads it (keepKmer @0-21), so
// only 1 does here.
int mhap_set_kmer_frequencies_ex(mhap_ctx *c, const char *kmers, const double *fractions,
                                 uint64_t n, uint64_t expected, const mhap_weighting *w) {
  if (!c) return fail(capi::ERR_STATE, "null context");
  MHAP_CHECK(host::check_weighting(w));
  if (n && (!kmers || !fractions)) return fail(capi::ERR_BAD_PARAM, "null k-mers / fractions");
  const bool bloom = w->supress_noise == 1;
  const host::BloomPlan plan = bloom ? host::bloom_plan(expected) : host::BloomPlan{};
  if (bloom && plan.words == 0) return fail(capi::ERR_BAD_PARAM, "Bloom filter of 0 bits");
  const host::FreqTable T =
      host::freq_table(kmers, fractions, n, c->P.k, !c->P.no_rc, *w, bloom ? &plan : nullptr);
  HIP_TRY(hipSetDevice(c->device));
  if (c->ftab.reserve(T.slots.size())) return fail(capi::ERR_OOM, "k-mer frequency table");
  HIP_TRY(hipMemcpy(c->ftab.p, T.slots.data(), sizeof(FreqSlot) * T.slots.size(),
                    hipMemcpyHostToDevice));
  c->fmask = T.mask;
  if (bloom) {
    if (c->bloom.reserve(T.bloom.size())) return fail(capi::ERR_OOM, "k-mer Bloom filter");
    HIP_TRY(hipMemcpy(c->bloom.p, T.bloom.data(), 8ull * T.bloom.size(), hipMemcpyHostToDevice));
    c->bloom_bits = plan.bits;
    c->bloom_k = plan.k;
  }
  c->has_bloom = bloom;
  c->W = *w;
  c->has_table = true;
  return capi::OK;
}

// What the MinHash launches of mhap_sketch share
struct SketchRun {
  int mode;
  int32_t bs_w;                   // the weight k_mh_bitslice draws (0: off; MHAP_BITSLICE=0)
  uint32_t bs_sample;
  int32_t H;
};

// MHAP_BS_DUMP (checks, tools/mhap_bs_debug.py): the exact pass's minima and lists of a batch
static int dump_bitslice(mhap_ctx *c, const char *path, const uint32_t *sids, uint32_t nb,
                         int32_t H) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::vector<BestOut> hb((size_t)nb * H);
  std::vector<uint32_t> hc(nb);
  HIP_TRY(hipMemcpy(hb.data(), c->mbest.p, sizeof(BestOut) * hb.size(), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hc.data(), c->mbscnt.p, 4ull * nb, hipMemcpyDeviceToHost));
  if (FILE *f = fopen(path, "wb")) {
    fwrite(&nb, 4, 1, f);
    fwrite(sids, 4, nb, f);
    fwrite(hc.data(), 4, nb, f);
    fwrite(hb.data(), sizeof(BestOut), hb.size(), f);
    fclose(f);
  }
  return capi::OK;
}

// One batch: keys, segmented radix sort of (key, position), draws (exact for the first round of
// every strand and for k-mers of other weights, bit-sliced for the rest).
static int sketch_batch(mhap_ctx *c, const SketchRun &R, const uint32_t *sids,
                        const host::SketchBatch &B) {
  hipStream_t s = c->stream;
  const int32_t H = R.H;
  const uint32_t nb = (uint32_t)(B.b - B.a);
  const uint64_t tot = B.tot;
  // reserve
  if (c->mkoff.reserve(nb + 1) || c->msids.reserve(nb) || c->mkeys.reserve(tot) ||
      c->mkeys2.reserve(tot) || c->mpos.reserve(tot) || c->mpos2.reserve(tot))
    return fail(capi::ERR_OOM, "MinHash keys (%llu)", (unsigned long long)tot);
  // upload
  HIP_TRY(hipMemcpyAsync(c->mkoff.p, B.koff.data(), 8ull * (nb + 1), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->msids.p, sids + B.a, 4ull * nb, hipMemcpyHostToDevice, s));
  // keys, sorted per strand
  KeyArgs KA{c->d_bases, c->d_off, c->d_len.p, c->msids.p, c->mkoff.p, (int32_t)c->P.k,
             c->mkeys.p, c->mpos.p};
  hipLaunchKernelGGL(k_mh_keys, dim3(nb), dim3(256), 0, s, KA);
  HIP_TRY(hipGetLastError());
  size_t tb = 0;
  HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairs(nullptr, tb, c->mkeys.p, c->mkeys2.p,
                                                      c->mpos.p, c->mpos2.p, (int)tot, (int)nb,
                                                      c->mkoff.p, c->mkoff.p + 1, 0, 64, s));
  if (c->msort_tmp.reserve(std::max<size_t>(tb, 1))) return fail(capi::ERR_OOM, "sort scratch");
  HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortPairs(c->msort_tmp.p, tb, c->mkeys.p, c->mkeys2.p,
                                                      c->mpos.p, c->mpos2.p, (int)tot, (int)nb,
                                                      c->mkoff.p, c->mkoff.p + 1, 0, 64, s));
  if (R.bs_w && (c->mbscnt.reserve(nb) || c->mbest.reserve((size_t)nb * H)))
    return fail(capi::ERR_OOM, "bit-sliced draws (%u strands)", nb);
  // draws: the sorted keys are in mkeys2 / mpos2: mkeys / mpos hold the bit-sliced lists
  SketchArgs SA{c->mkeys2.p, c->mpos2.p, c->mkoff.p, c->msids.p, H,
                R.mode, c->has_table ? c->ftab.p : nullptr, c->fmask, c->W.repeat_idf_scale,
                c->W.no_tf, c->minhash.p, c->ocount.p, c->kctr.p,
                R.bs_w, R.bs_sample, c->mkeys.p, c->mpos.p, c->mbscnt.p, c->mbest.p,
                BloomDev{c->has_bloom ? c->bloom.p : nullptr, c->bloom_bits, c->bloom_k}};
  HIP_TRY(hipEventRecord(c->ev[2], s));
  hipLaunchKernelGGL(k_mh_minhash, dim3(nb), dim3(256), host::minhash_lds(c->P.num_hashes), s, SA);
  HIP_TRY(hipGetLastError());
  if (R.bs_w) {
    if (const char *path = getenv("MHAP_BS_DUMP"))
      if (int rc = dump_bitslice(c, path, sids + B.a, nb, H)) return rc;
    const char *zm = getenv("MHAP_BS_ZMAX");
    BsArgs BA{c->mkeys.p, c->mpos.p, c->mbscnt.p, c->mkoff.p, c->msids.p, c->mbest.p, H, R.bs_w,
              c->minhash.p, zm ? atoi(zm) : 64};
    hipLaunchKernelGGL(k_mh_bitslice, dim3(nb), dim3(64), host::bitslice_lds(H), s, BA);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(c->ev[3], s));
  HIP_TRY(hipStreamSynchronize(s));                 // koff / sids are rewritten next batch
  // account
  c->stats.ms_sketch_kernel += elapsed(c->ev[2], c->ev[3]);
  c->stats.sketch_launches++;
  return capi::OK;
}

// The MinHash sketches of strands (sids) in batches of <= MHAP_KEY_BUDGET k-mers.
static int sketch_minhash(mhap_ctx *c, const std::vector<uint32_t> &sids) {
  SketchRun R;
  R.mode = host::weighting_mode(c->W.repeat_weight, c->has_table);
  R.bs_w = host::bitslice_weight(R.mode, c->W.repeat_idf_scale);
  if (const char *e = getenv("MHAP_BITSLICE"))
    if (atoi(e) == 0) R.bs_w = 0;
  R.H = (int32_t)c->P.num_hashes;
  // the exact sample: a strand's first 2,048 sorted k-mers (x w draws) put a function's
  // minimum near 2^64 / 20,480 above -2^63, so the bit-sliced filter starts at ~14 planes;
  // measured on configs[3]: sketch 5.62 s with 2,048, 6.37 s with 512, 6.61 s with 128
  // (profiles/r06s_mhap_sample_ab.txt; MHAP_BS_SAMPLE for A/Bs)
  R.bs_sample = 2048;
  if (const char *e = getenv("MHAP_BS_SAMPLE")) R.bs_sample = (uint32_t)std::max(0, atoi(e));
  uint64_t key_budget = host::KEY_BUDGET;           // MHAP_KEY_BUDGET: tests, for more batches
  if (const char *e = getenv("MHAP_KEY_BUDGET")) key_budget = (uint64_t)std::max(0ll, atoll(e));
  for (const host::SketchBatch &B : host::sketch_batches(sids, c->h_len.data(), (int32_t)c->P.k,
                                                   key_budget, host::BATCH_STRANDS))
    if (int rc = sketch_batch(c, R, sids.data(), B)) return rc;
  return capi::OK;
}

int mhap_sketch(mhap_ctx *c, uint32_t bgn, uint32_t end) {
  if (!c || !c->nreads) return fail(capi::ERR_STATE, "no reads loaded");
  if (!c->d_bases || !c->d_off)
    return fail(capi::ERR_STATE, "no bases loaded (lengths only: import sketches instead)");
  if (!c->loaded(bgn, end))
    return fail(capi::ERR_BAD_PARAM, "sketch range %u-%u outside the loaded reads", bgn, end);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const uint32_t r0 = bgn - c->first_iid, nr = end - bgn + 1;
  HIP_TRY(hipMemsetAsync(c->kctr.p, 0, 16, s));
  c->stats.ms_sketch_kernel = 0;
  c->stats.sketch_launches = 0;
  HIP_TRY(hipEventRecord(c->ev[0], s));
  // ordered sketches first: they decide which strands are used (ocount > 0)
  const int32_t min_use = host::min_use(c->P.min_olap, c->P.k);
  for (uint32_t a = 0; a < nr; a += 1u << 19) {
    const uint32_t n = std::min<uint32_t>(nr - a, 1u << 19);
    OrderedArgs OA{c->d_bases, c->d_off, c->d_len.p, r0 + a, 2 * n, (int32_t)c->P.ordered_k,
                   (int32_t)c->P.ordered_sketch, min_use, c->P.no_rc, c->ordered.p, c->ocount.p};
    hipLaunchKernelGGL(k_mh_ordered, dim3(2 * n), dim3(256), 0, s, OA);
    HIP_TRY(hipGetLastError());
  }
  // the MinHash sketches of the strands in use (host lengths decide the same way)
  std::vector<uint32_t> sids;
  const uint64_t used = host::strands_in_use(c->h_len.data(), r0, nr, c->P.min_olap, c->P.k,
                                          c->P.ordered_k, c->P.no_rc != 0, sids);
  int rc = sketch_minhash(c, sids);
  if (rc) return rc;
  hipLaunchKernelGGL(k_mh_strand_fixup, dim3((nr + 255) / 256), dim3(256), 0, s, c->ocount.p,
                     r0, nr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[1], s));
  unsigned long long st[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(st, c->kctr.p, 16, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  c->stats.ms_sketch = elapsed(c->ev[0], c->ev[1]);
  c->stats.sketched_reads = used;
  c->stats.sketch_kmers = st[0];
  c->stats.sketch_draws = st[1];
  c->indexed = false;
  return capi::OK;
}

int mhap_sketch_buffers(mhap_ctx *c, void **d_minhash, void **d_ordered, void **d_ocount) {
  if (!c || !c->nreads) return fail(capi::ERR_STATE, "no reads loaded");
  *d_minhash = c->minhash.p;
  *d_ordered = c->ordered.p;
  *d_ocount = c->ocount.p;
  return capi::OK;
}

static int copy_rows(mhap_ctx *c, uint32_t first, uint32_t n, void *mh, void *od, void *oc,
                     int to_ctx, bool host) {
  if (!c || !c->nreads) return fail(capi::ERR_STATE, "no reads loaded");
  if (n == 0) return capi::OK;
  if (first < c->first_iid || (uint64_t)first + n > (uint64_t)c->first_iid + c->nreads)
    return fail(capi::ERR_BAD_PARAM, "rows %u..%u outside the loaded reads", first, first + n - 1);
  if (!mh || !od || !oc) return fail(capi::ERR_BAD_PARAM, "null buffer");
  HIP_TRY(hipSetDevice(c->device));
  const size_t s0 = 2ull * (first - c->first_iid), ns = 2ull * n;
  const size_t H = c->P.num_hashes, S = c->P.ordered_sketch;
  struct { void *ctx; void *user; size_t bytes; } parts[3] = {
      {c->minhash.p + s0 * H, mh, 4 * H * ns},
      {c->ordered.p + s0 * S, od, 8 * S * ns},
      {c->ocount.p + s0, oc, 4 * ns}};
  const hipMemcpyKind in = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
  const hipMemcpyKind outk = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  for (auto &pt : parts) {
    if (to_ctx) HIP_TRY(hipMemcpyAsync(pt.ctx, pt.user, pt.bytes, in, c->stream));
    else        HIP_TRY(hipMemcpyAsync(pt.user, pt.ctx, pt.bytes, outk, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (to_ctx) c->indexed = false;
  return capi::OK;
}

int mhap_copy_sketches(mhap_ctx *c, uint32_t first, uint32_t n, void *d_minhash,
                       void *d_ordered, void *d_ocount, int to_ctx) {
  return copy_rows(c, first, n, d_minhash, d_ordered, d_ocount, to_ctx, false);
}

int mhap_copy_sketches_host(mhap_ctx *c, uint32_t first, uint32_t n, void *h_minhash,
                            void *h_ordered, void *h_ocount, int to_ctx) {
  return copy_rows(c, first, n, h_minhash, h_ordered, h_ocount, to_ctx, true);
}

int mhap_build_index(mhap_ctx *c) {
  if (!c || !c->nreads) return fail(capi::ERR_STATE, "no reads loaded");
  return mhap_build_index_range(c, c->first_iid, c->first_iid + c->nreads - 1);
}

int mhap_build_index_range(mhap_ctx *c, uint32_t bgn, uint32_t end) {
  if (!c || !c->nreads) return fail(capi::ERR_STATE, "no reads loaded");
  if (!c->loaded(bgn, end))
    return fail(capi::ERR_BAD_PARAM, "index range %u-%u outside the loaded reads", bgn, end);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const int32_t H = (int32_t)c->P.num_hashes;
  const uint32_t s0 = 2 * (bgn - c->first_iid), ns = 2 * (end - bgn + 1);
  const size_t n = (size_t)ns * H;
  if (n >= 0x7FFFFFFFull) return fail(capi::ERR_BAD_PARAM, "index of %zu entries too large", n);
  if (c->keys.reserve(n) || c->vals.reserve(n) || c->keys2.reserve(n) || c->vals2.reserve(n) ||
      c->toff.reserve(H + 1))
    return fail(capi::ERR_OOM, "index (%zu entries)", n);
  HIP_TRY(hipEventRecord(c->ev[0], s));
  hipLaunchKernelGGL(k_mh_index_keys, dim3(4096), dim3(256), 0, s, c->minhash.p, c->ocount.p,
                     s0, ns, H, c->keys.p, c->vals.p);
  HIP_TRY(hipGetLastError());
  const int end_bit = host::index_end_bit(H);
  size_t tmp = 0;
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, c->keys.p, c->keys2.p, c->vals.p,
                                             c->vals2.p, (int)n, 0, end_bit, s));
  if (c->sort_tmp.reserve(tmp)) return fail(capi::ERR_OOM, "sort scratch");
  HIP_TRY(hipcub::DeviceRadixSort::SortPairs(c->sort_tmp.p, tmp, c->keys.p, c->keys2.p, c->vals.p,
                                             c->vals2.p, (int)n, 0, end_bit, s));
  hipLaunchKernelGGL(k_mh_table_offsets, dim3((H + 1 + 255) / 256), dim3(256), 0, s,
                     c->keys2.p, n, H, c->toff.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev[1], s));
  HIP_TRY(hipStreamSynchronize(s));
  c->stats.ms_index = elapsed(c->ev[0], c->ev[1]);
  c->nkeys = n;
  c->indexed = true;
  return capi::OK;
}

// First stage: the candidates of queries [q0, q1), the buffer grown and the launch redone on
// overflow; *ncand of them in c->cand, *ms the launches' device time.
static int find_candidates(mhap_ctx *c, uint32_t q0, uint32_t q1, uint32_t self, uint32_t *ncand,
                           float *ms) {
  hipStream_t s = c->stream;
  const uint32_t nq = q1 - q0;
  size_t cap = host::cand_cap_initial(nq);
  uint32_t h[4];
  *ms = 0;
  for (;;) {
    if (cap > host::CAND_CAP_MAX) return fail(capi::ERR_OOM, "candidate list too large");
    if (c->cand.reserve(cap)) return fail(capi::ERR_OOM, "candidates");
    HIP_TRY(hipMemsetAsync(c->ctr.p, 0, 64, s));
    CandArgs CA{c->minhash.p, c->ocount.p, c->d_len.p, c->keys2.p, c->vals2.p, c->toff.p,
                (int32_t)c->P.num_hashes, q0, q1, self, c->P.min_store, c->P.min_matches,
                c->cand.p, c->ctr.p, (uint32_t)cap, c->ctr.p + 1};
    HIP_TRY(hipEventRecord(c->ev[0], s));
    hipLaunchKernelGGL(k_mh_candidates, dim3((nq + 3) / 4), dim3(256), host::candidates_lds(), s, CA);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[1], s));
    HIP_TRY(hipMemcpyAsync(h, c->ctr.p, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *ms += elapsed(c->ev[0], c->ev[1]);
    if (h[1] & 1u)
      return fail(capi::ERR_BAD_INPUT, "a query has more than %d candidate strands", TSLOTS);
    if (h[1] & 2u) { cap = host::cand_cap_grown(h[0]); continue; }
    break;
  }
  *ncand = h[0];
  return capi::OK;
}

static int compare_impl(mhap_ctx *c, uint32_t bgn, uint32_t end, uint32_t self,
                        uint64_t *n_out) {
  if (!c || !c->indexed) return fail(capi::ERR_STATE, "mhap_build_index() first");
  if (!c->loaded(bgn, end))
    return fail(capi::ERR_BAD_PARAM, "query range %u-%u outside the loaded reads", bgn, end);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const uint32_t q0 = bgn - c->first_iid, q1 = end - c->first_iid + 1;
  uint32_t ncand = 0;
  float ms_cand = 0;
  if (int rc = find_candidates(c, q0, q1, self, &ncand, &ms_cand)) return rc;
  // second stage
  const size_t rcap = host::rec_cap(ncand);
  if (c->rec.reserve(rcap)) return fail(capi::ERR_OOM, "records");
  HIP_TRY(hipMemsetAsync(c->ctr.p + 4, 0, 16, s));
  const int32_t S = (int32_t)c->P.ordered_sketch;
  CmpArgs MA{c->cand.p, ncand, c->ordered.p, c->ocount.p, c->d_len.p, S,
             (int32_t)c->P.ordered_k, c->P.max_shift, c->pass.p, c->pass_empty, c->rec.p,
             c->ctr.p + 4, (uint32_t)rcap, c->ctr.p + 5};
  HIP_TRY(hipEventRecord(c->ev[0], s));
  if (ncand) {
    hipLaunchKernelGGL(k_mh_compare, dim3(host::compare_blocks(ncand)), dim3(64), host::compare_lds(S),
                       s, MA);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(c->ev[1], s));
  uint32_t h[2];
  HIP_TRY(hipMemcpyAsync(h, c->ctr.p + 4, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (h[1]) return fail(capi::ERR_OOM, "record capacity exceeded");
  c->stats.ms_candidates = ms_cand;
  c->stats.ms_compare = elapsed(c->ev[0], c->ev[1]);
  c->stats.candidates = ncand;
  c->stats.overlaps = h[0];
  c->nrec = h[0];
  *n_out = c->nrec;
  return capi::OK;
}

int mhap_compare(mhap_ctx *c, uint32_t bgn, uint32_t end, uint64_t *n_out) {
  return compare_impl(c, bgn, end, 1, n_out);
}

int mhap_compare_all(mhap_ctx *c, uint32_t bgn, uint32_t end, uint64_t *n_out) {
  return compare_impl(c, bgn, end, 0, n_out);
}

int mhap_fetch(mhap_ctx *c, mhap_record *out, uint64_t max_records, uint64_t *n_copied) {
  if (!c) return fail(capi::ERR_STATE, "null context");
  HIP_TRY(hipSetDevice(c->device));
  std::vector<RecDev> h(c->nrec);
  if (c->nrec)
    HIP_TRY(hipMemcpy(h.data(), c->rec.p, sizeof(RecDev) * c->nrec, hipMemcpyDeviceToHost));
  host::sort_records(h);
  const uint64_t n = std::min<uint64_t>(max_records, h.size());
  for (uint64_t i = 0; i < n; i++) out[i] = host::to_record(h[i], c->first_iid, (int)c->P.ordered_k);
  *n_copied = n;
  return capi::OK;
}

int mhap_format_line(const mhap_record *x, uint32_t hash_base, uint32_t num_hash,
                     uint32_t query_base, char *buf, size_t cap) {
  if (!x || !buf) return fail(capi::ERR_BAD_PARAM, "null argument");
  if (hash_base == 0 || query_base == 0)
    return fail(capi::ERR_BAD_PARAM, "bases are 1-based IDs");
  const int n = host::format_line(*x, hash_base, num_hash, query_base, buf, cap);
  if (n < 0 || (size_t)n >= cap) return fail(capi::ERR_BAD_PARAM, "line buffer too small");
  return capi::OK;
}

int mhap_write_text(mhap_ctx *c, const char *path, uint32_t hash_base, uint32_t num_hash,
                    uint32_t query_base) {
  if (!c || !path) return fail(capi::ERR_STATE, "null argument");
  if (hash_base == 0 || query_base == 0)
    return fail(capi::ERR_BAD_PARAM, "bases are 1-based IDs");
  std::vector<mhap_record> r(c->nrec);
  uint64_t n = 0;
  int rc = mhap_fetch(c, r.data(), r.size(), &n);
  if (rc) return rc;
  FILE *F = fopen(path, "w");
  if (!F) return fail(capi::ERR_BAD_INPUT, "open '%s': %s", path, strerror(errno));
  char line[256];
  for (uint64_t i = 0; i < n; i++) {
    rc = mhap_format_line(&r[i], hash_base, num_hash, query_base, line, sizeof line);
    if (rc) { fclose(F); return rc; }
    fputs(line, F);
    fputc('\n', F);
  }
  if (fclose(F) != 0) return fail(capi::ERR_BAD_INPUT, "write '%s': %s", path, strerror(errno));
  return capi::OK;
}

int mhap_get_stats(mhap_ctx *c, mhap_stats *out) {
  if (!c) return fail(capi::ERR_STATE, "null context");
  *out = c->stats;
  return capi::OK;
}

}  // extern "C"
