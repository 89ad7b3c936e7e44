// ovl_api.hip -- the C-ABI (include/canu_ovl.h) over the host side of the HIP path: one
// translation unit, whose host code is in ovl_ctx.h (context), ovl_build.hip (index and hash
// batches), ovl_sq.hip (sorted query windows), ovl_find.hip (one search) and ovl_driver.hip
// (OverlapDriver), and whose arithmetic is in ovl_plan.h.
//
// Host responsibilities mirror overlapInCore's driver (overlapInCore.C:190 OverlapDriver,
// :306 main): option fix-ups, the maxErate tables (prefixEditDistance.C:40-116,
// Binomial_Bound.C), read loading, then the per-batch kernel sequence
//   k_probe -> k_chain -> k_extend
// over (query, orientation) units.  There is no CPU fallback for any of it.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <chrono>
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/canu_ovl.h"
#include "ovl_common.h"

#include "ovl_index.hip"
#include "ovl_seed.hip"
#include "ovl_extend.hip"
#include "ovl_ovb.h"
#include "ovl_plan.h"
#include "ped_host.h"

using namespace ovl;

// ovl_probe_ceiling: Q independent random 16-B loads in flight per lane over the table's
// 2^tab_bits slots (masked index, an LCG per lane: nothing in the loop but the loads)
template <int Q>
__global__ void __launch_bounds__(256) k_rand_lookup(const uint4 *t, uint64_t mask,
                                                     uint32_t iters, uint32_t *sink) {
  uint32_t acc = 0;
  uint64_t x = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x + 1) * 0x9E3779B97F4A7C15ull;
  for (uint32_t i = 0; i < iters; i++) {
    uint4 v[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      v[q] = t[(x >> 17) & mask];
    }
#pragma unroll
    for (int q = 0; q < Q; q++) acc ^= v[q].x ^ v[q].y ^ v[q].z ^ v[q].w;   // whole 16-B loads
  }
  if (acc == 0x9E3779B9u) sink[0] = acc;       // keeps the loads live; (almost) never taken
}
// instantiated here only so that the code object keeps this kernel's place, and with it every
// other kernel's address, as they were before the host code was split into files
template __global__ void k_rand_lookup<8>(const uint4 *, uint64_t, uint32_t, uint32_t *);

// ovl_probe_replay: the table slot of every query window (k_probe's window rule and hash),
// written as a 32-bit slot list (0xFFFFFFFF: no k-mer), one wave per unit
__global__ void __launch_bounds__(256) k_slot_list(ReadsDev R, const Unit *units,
                                                   const uint64_t *wbase, uint32_t nunits,
                                                   uint32_t k, uint64_t kmask, uint32_t tab_bits,
                                                   uint32_t *slot) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t u = blockIdx.x * 4 + wave;
  if (u >= nunits) return;
  const Unit un = units[u];
  const Strand S = un.dir ? strand_rc(R, un.r) : strand_fwd(R, un.r);
  const uint32_t *bad = un.dir ? S.ex_nul : S.ex_wild;
  const uint32_t nw = (uint32_t)(wbase[u + 1] - wbase[u]);
  const uint32_t kbits = (1u << k) - 1u;
  for (uint32_t o = lane; o < nw; o += 64) {
    bool ok = (int32_t)(o + k) <= S.len;
    if (ok && bad) ok = (mask_at(bad, (int32_t)o) & kbits) == 0;
    slot[wbase[u] + o] =
        ok ? (uint32_t)(mix64(bases_at(S.w, (int32_t)o) & kmask) >> (64 - tab_bits)) : 0xFFFFFFFFu;
  }
}

// the same lookups as pure loads: 8 table entries per lane in flight, the next group's 8
// slot indices loaded while they are (so no phase of the loop waits on the slot stream)
__global__ void __launch_bounds__(256) k_slot_replay(const uint4 *t, const uint32_t *slot,
                                                     uint64_t n, uint32_t *sink) {
  uint32_t acc = 0;
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint64_t i0 = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  uint32_t sl[8];
#pragma unroll
  for (int q = 0; q < 8; q++) {
    const uint64_t i = i0 + q * stride;
    sl[q] = i < n ? slot[i] : 0xFFFFFFFFu;
  }
  for (; i0 < n; i0 += 8 * stride) {
    uint4 v[8];
#pragma unroll
    for (int q = 0; q < 8; q++) v[q] = sl[q] != 0xFFFFFFFFu ? t[sl[q]] : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const uint64_t i = i0 + 8 * stride + q * stride;
      sl[q] = i < n ? slot[i] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int q = 0; q < 8; q++) acc ^= v[q].x ^ v[q].y ^ v[q].z ^ v[q].w;   // whole 16-B loads
  }
  if (acc == 0x9E3779B9u) sink[0] = acc;
}

// the host side, one file per concern (in the order that keeps the kernels' addresses in the
// code object: ovl_build.hip names k_fine before ovl_sq.hip names the radix sort)
#include "ovl_ctx.h"
#include "ovl_build.hip"
#include "ovl_sq.hip"
#include "ovl_find.hip"
#include "ovl_driver.hip"

extern "C" {

int ovl_abi_version(void) { return OVL_ABI_VERSION; }

const char *ovl_last_error(void) { return g_err.c_str(); }

void ovl_params_init(ovl_params *p) {
  p->kmer_len = 0;
  p->max_erate = 0.06;
  p->min_olap_len = 0;
  p->partial = 0;
  p->unique_olap_per_pair = 1;
  p->use_window_filter = 0;
  p->use_hopeless_check = 1;
  p->frag_olap_limit = UINT64_MAX;
  p->filter_by_kmer_count = 0;
}

void ovl_params_finalize(ovl_params *p) {
  if (p->max_erate > 0.06) {
    p->use_window_filter = 0;
    p->use_hopeless_check = 0;
  }
}

void *ovl_ctx_stream(ovl_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int ovl_traceback_window_rows(void) { return OVL_TBR; }

int ovl_row_end_margin(void) { return OVL_END_MARGIN; }

int ovl_probe_ceiling(ovl_ctx *c, double *gloads_per_s, uint64_t *table_bytes) {
  if (!c || !gloads_per_s || !table_bytes) return fail(OVL_ERR_STATE, "null argument");
  if (!c->have_index || !c->d_tab.p) return fail(OVL_ERR_STATE, "no index table");
  HIPC(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const uint64_t slots = 1ull << c->tab_bits;
  DBuf<uint32_t> sink;
  if (sink.alloc(1)) return fail(OVL_ERR_OOM, "sink");
  const uint32_t blocks = 8u * (uint32_t)c->n_cu, iters = 64;
  hipLaunchKernelGGL(k_rand_lookup<8>, dim3(blocks), dim3(256), 0, s,
                     (const uint4 *)c->d_tab.p, slots - 1, iters, sink.p);   // warm
  HIPC(hipEventRecord(c->ev[6], s));
  const int reps = 3;
  for (int r = 0; r < reps; r++)
    hipLaunchKernelGGL(k_rand_lookup<8>, dim3(blocks), dim3(256), 0, s,
                       (const uint4 *)c->d_tab.p, slots - 1, iters, sink.p);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(c->ev[7], s));
  HIPC(hipEventSynchronize(c->ev[7]));
  float ms = 0;
  HIPC(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
  const double loads = (double)reps * blocks * 256.0 * iters * 8.0;
  *gloads_per_s = ms > 0 ? loads / (ms * 1e-3) / 1e9 : 0.0;
  *table_bytes = slots * sizeof(TabEntry);
  return OVL_OK;
}

int ovl_probe_replay(ovl_ctx *c, uint32_t bgn, uint32_t end, double *gloads_per_s,
                     uint64_t *n_windows) {
  if (!c || !gloads_per_s || !n_windows) return fail(OVL_ERR_STATE, "null argument");
  if (!c->have_index || !c->d_tab.p) return fail(OVL_ERR_STATE, "no index table");
  if (c->tab_bits > 32) return fail(OVL_ERR_UNSUPPORTED, "table of 2^%u slots", c->tab_bits);
  HIPC(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if (bgn < c->first_iid) bgn = c->first_iid;
  const uint32_t last = c->first_iid + c->nreads - 1;
  if (end > last) end = last;
  // the query units (both orientations, --minlength, k) up to the read that passes 2^28
  // windows: a sample of the same lookup stream k_probe runs over these reads
  std::vector<Unit> units;
  std::vector<uint64_t> wb(1, 0);
  const uint32_t k = c->P.kmer_len;
  query_rule(c).each(bgn, end, [&](uint32_t a, bool, uint64_t w) {
    if (!w || wb.back() >= (1ull << 28)) return;
    for (uint32_t dir = 0; dir < 2; dir++) {
      units.push_back(Unit{a - c->first_iid, dir});
      wb.push_back(wb.back() + w);
    }
  });
  const uint64_t n = wb.back();
  *n_windows = n;
  *gloads_per_s = 0.0;
  if (n == 0) return OVL_OK;
  DBuf<uint32_t> slot, sink;
  DBuf<Unit> du;
  DBuf<uint64_t> dwb;
  if (slot.alloc(n) || sink.alloc(1) || du.alloc(units.size()) || dwb.alloc(wb.size()))
    return fail(OVL_ERR_OOM, "probe replay (%llu windows)", (unsigned long long)n);
  HIPC(hipMemcpyAsync(du.p, units.data(), sizeof(Unit) * units.size(), hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(dwb.p, wb.data(), 8ull * wb.size(), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_slot_list, dim3(((uint32_t)units.size() + 3) / 4), dim3(256), 0, s,
                     c->reads(), du.p, dwb.p, (uint32_t)units.size(), k,
                     (1ull << (2 * k)) - 1, c->tab_bits, slot.p);
  const uint32_t blocks = 8u * (uint32_t)c->n_cu;
  hipLaunchKernelGGL(k_slot_replay, dim3(blocks), dim3(256), 0, s, (const uint4 *)c->d_tab.p,
                     slot.p, n, sink.p);                                       // warm
  HIPC(hipEventRecord(c->ev[6], s));
  const int reps = 3;
  for (int r = 0; r < reps; r++)
    hipLaunchKernelGGL(k_slot_replay, dim3(blocks), dim3(256), 0, s, (const uint4 *)c->d_tab.p,
                       slot.p, n, sink.p);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(c->ev[7], s));
  HIPC(hipEventSynchronize(c->ev[7]));
  float ms = 0;
  HIPC(hipEventElapsedTime(&ms, c->ev[6], c->ev[7]));
  *gloads_per_s = ms > 0 ? (double)reps * (double)n / (ms * 1e-3) / 1e9 : 0.0;
  return OVL_OK;
}

// ---- index export / import (ABI 7) ----------------------------------------------------
int ovl_export_index(ovl_ctx *c, ovl_index_desc *o) {
  if (!c || !o) return fail(OVL_ERR_STATE, "null argument");
  if (!c->have_index) return fail(OVL_ERR_STATE, "no index built");
  memset(o, 0, sizeof(*o));
  o->bgn_iid = c->hash_bgn_iid;
  o->end_iid = c->hash_end_iid;
  o->first_iid = c->first_iid;
  o->nreads = c->nreads;
  o->kmer_len = c->P.kmer_len;
  o->tab_bits = c->tab_bits;
  o->slice_bits = c->slice_bits;
  o->hash_lib_lo = c->stats_hash_lib_lo;
  o->hash_lib_hi = c->stats_hash_lib_hi;
  o->records = c->index_records;
  o->table = c->d_tab.p;
  o->table_bytes = sizeof(TabEntry) << c->tab_bits;
  o->occ = c->d_occ.p;
  o->occ_bytes = 8ull * c->index_records;
  if (c->bloom_ok) {
    o->bloom_w = c->bloom_w;
    o->bloom = c->d_bloom.p;
    o->bloom_bytes = 8ull * ((1ull << (c->tab_bits - c->slice_bits)) << c->bloom_w);
  }
  o->read_flags = c->d_flags.p;
  o->read_flags_bytes = 4ull * c->nreads;
  return OVL_OK;
}

int ovl_import_index(ovl_ctx *c, const ovl_index_desc *in) {
  if (!c || !in) return fail(OVL_ERR_STATE, "null argument");
  if (c->nreads == 0) return fail(OVL_ERR_STATE, "no reads loaded");
  if (in->first_iid != c->first_iid || in->nreads != c->nreads)
    return fail(OVL_ERR_BAD_PARAM, "index of reads %u+%u, this context holds %u+%u",
                in->first_iid, in->nreads, c->first_iid, c->nreads);
  if (in->kmer_len != c->P.kmer_len)
    return fail(OVL_ERR_BAD_PARAM, "index of %u-mers, this context uses -k %u", in->kmer_len,
                c->P.kmer_len);
  if (in->tab_bits > 40 || in->slice_bits > in->tab_bits ||
      in->table_bytes != (sizeof(TabEntry) << in->tab_bits) || in->occ_bytes != 8ull * in->records ||
      in->read_flags_bytes != 4ull * in->nreads || !in->table || (in->records && !in->occ) ||
      !in->read_flags || (in->bloom_bytes && (!in->bloom ||
      in->bloom_w > 6 ||
      in->bloom_bytes != 8ull * ((1ull << (in->tab_bits - in->slice_bits)) << in->bloom_w))))
    return fail(OVL_ERR_BAD_PARAM, "inconsistent index descriptor");
  // the limits build_index keeps (and the table / probe kernels assume): 32-bit run offsets,
  // a slice (and, with the filter, its filter region) within one wave's 64 KB of LDS
  if (in->records >= 0xFFFFFFF0ull || in->slice_bits < 1 || (16ull << in->slice_bits) > 65536 ||
      (in->bloom_bytes && (16ull << in->slice_bits) + (8ull << in->bloom_w) > 65536))
    return fail(OVL_ERR_BAD_PARAM, "index descriptor past the build's limits (records %llu, "
                "slice 2^%u, filter 2^%u words)", (unsigned long long)in->records,
                in->slice_bits, in->bloom_w);
  if (in->end_iid < in->bgn_iid || in->bgn_iid < c->first_iid ||
      in->end_iid > c->first_iid + c->nreads - 1)
    return fail(OVL_ERR_BAD_PARAM, "index of hash reads %u-%u outside the loaded reads",
                in->bgn_iid, in->end_iid);
  HIPC(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  c->have_index = false;
  if (c->d_tab.alloc(1ull << in->tab_bits) || c->d_occ.alloc(std::max<uint64_t>(in->records, 1)) ||
      (in->bloom_bytes && c->d_bloom.alloc(in->bloom_bytes / 8)))
    return fail(OVL_ERR_OOM, "imported index (%.1f GB)",
                (in->table_bytes + in->occ_bytes + in->bloom_bytes) / 1e9);
  HIPC(hipEventRecord(c->ev[0], s));
  HIPC(hipMemcpyAsync(c->d_tab.p, in->table, in->table_bytes, hipMemcpyDefault, s));
  if (in->records)
    HIPC(hipMemcpyAsync(c->d_occ.p, in->occ, in->occ_bytes, hipMemcpyDefault, s));
  if (in->bloom_bytes)
    HIPC(hipMemcpyAsync(c->d_bloom.p, in->bloom, in->bloom_bytes, hipMemcpyDefault, s));
  HIPC(hipMemcpyAsync(c->d_flags.p, in->read_flags, in->read_flags_bytes, hipMemcpyDefault, s));
  HIPC(hipEventRecord(c->ev[1], s));
  HIPC(hipStreamSynchronize(s));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
  c->stats.ms_index = ms;                      // the copy stands in for the build
  c->hash_bgn_iid = in->bgn_iid;
  c->hash_end_iid = in->end_iid;
  c->tab_bits = in->tab_bits;
  c->slice_bits = in->slice_bits;
  c->bloom_w = in->bloom_bytes ? in->bloom_w : 0;
  c->bloom_ok = in->bloom_bytes != 0;
  c->index_records = in->records;
  c->stats_hash_lib_lo = in->hash_lib_lo;
  c->stats_hash_lib_hi = in->hash_lib_hi;
  // the copied flags carry the exporter's NOHASH bits (-H): a later build re-derives them
  if (in->hash_lib_lo != 0 || in->hash_lib_hi != UINT32_MAX) c->nohash_set = true;
  c->have_index = true;
  return OVL_OK;
}

int ovl_ctx_create(const ovl_params *p, int device, ovl_ctx **out) {
  *out = nullptr;
  if (p->kmer_len == 0) return fail(OVL_ERR_BAD_PARAM, "kmer length (-k) needed");
  if (p->kmer_len > 31) return fail(OVL_ERR_BAD_PARAM, "kmer length must be <= 31");
  if (!(p->max_erate > 0.0) || p->max_erate >= 1.0)
    return fail(OVL_ERR_BAD_PARAM, "maxErate out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(OVL_ERR_NO_DEVICE, "no HIP device");
  if (device < 0 || device >= ndev) return fail(OVL_ERR_NO_DEVICE, "bad device ordinal %d", device);
  hipDeviceProp_t prop;
  HIPC(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(OVL_ERR_NO_DEVICE, "device %d is %s, not gfx950", device, prop.gcnArchName);
  HIPC(hipSetDevice(device));

  ovl_ctx *c = new ovl_ctx();
  c->P = *p;
  ovl_params_finalize(&c->P);
  c->device = device;
  c->n_cu = prop.multiProcessorCount;
  memset(&c->stats, 0, sizeof(c->stats));
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return fail(OVL_ERR_HIP, "stream create failed");
  }
  for (int i = 0; i < 8; i++) (void)hipEventCreate(&c->ev[i]);
  for (int i = 0; i < 2; i++) (void)hipEventCreate(&c->xev[i]);

  double er = c->P.max_erate;
  c->max_errors = 1 + (int32_t)ceil(er * AS_MAX_READLEN);
  c->branch_match_value = er / (1 + er);
  c->min_branch_tail_slope = (er > 0.06) ? 1.0 : 0.20;
  c->h_error_bound.resize(AS_MAX_READLEN + 1);
  for (uint32_t i = 0; i <= AS_MAX_READLEN; i++)
    c->h_error_bound[i] = (int32_t)ceil(i * er);
  std::vector<int32_t> ml;
  ped::init_match_limit(ml, er, c->max_errors, c->max_errors);
  // padded past max_errors: the staged kernel may read its rows' limits straight from here
  // (OVL_GML), where a block's LDS copy held 0x7fffffff beyond max_errors
  ml.resize(ml.size() + 64, 0x7fffffff);
  if (c->d_error_bound.alloc(AS_MAX_READLEN + 1) != hipSuccess ||
      c->d_match_limit.alloc(ml.size()) != hipSuccess) {
    ovl_ctx_destroy(c);
    return fail(OVL_ERR_OOM, "table alloc");
  }
  (void)hipMemcpy(c->d_error_bound.p, c->h_error_bound.data(), 4ull * (AS_MAX_READLEN + 1),
                  hipMemcpyHostToDevice);
  (void)hipMemcpy(c->d_match_limit.p, ml.data(), 4ull * ml.size(), hipMemcpyHostToDevice);
  *out = c;
  return OVL_OK;
}

void ovl_ctx_destroy(ovl_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (int i = 0; i < 8; i++)
    if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
  for (int i = 0; i < 2; i++)
    if (c->xev[i]) (void)hipEventDestroy(c->xev[i]);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

static int load_common(ovl_ctx *c, uint32_t first_iid, uint32_t nreads, const uint8_t *d_bases,
                       const uint64_t *d_offsets, const uint32_t *h_lengths) {
  // Until every check and allocation has passed the context holds no reads, so a failed
  // load leaves nothing for a later build / find to run over (they return OVL_ERR_STATE).
  c->nreads = 0;
  c->have_index = false;
  c->have_qual = false;
  c->h_lib.clear();
  c->nohash_set = false;
  if (first_iid == 0 && nreads) return fail(OVL_ERR_BAD_PARAM, "read IDs start at 1");
  if ((uint64_t)first_iid + nreads > 0xFFFFFFFFull)
    return fail(OVL_ERR_BAD_PARAM, "read IDs past 2^32");
  std::vector<uint64_t> wofs(nreads + 1);
  uint64_t w = 0;
  uint32_t max_len = 0;
  for (uint32_t i = 0; i < nreads; i++) {
    if (h_lengths[i] > AS_MAX_READLEN)
      return fail(OVL_ERR_BAD_INPUT, "read %u longer than AS_MAX_READLEN", first_iid + i);
    wofs[i] = w;
    w += (h_lengths[i] + 31) / 32 + 1;
    max_len = std::max(max_len, h_lengths[i]);
  }
  wofs[nreads] = w;
  w += 2;
  if (c->d_fwd.alloc(w) || c->d_rc.alloc(w) || c->d_fwdN.alloc(w) || c->d_rcNul.alloc(w) ||
      c->d_wofs.alloc(nreads + 1) || c->d_len.alloc(nreads) || c->d_flags.alloc(nreads) ||
      c->d_rcFirstNul.alloc(nreads))
    return fail(OVL_ERR_OOM, "read buffers (%llu words)", (unsigned long long)w);
  c->h_len.assign(h_lengths, h_lengths + nreads);
  c->h_wofs.swap(wofs);
  c->max_len = max_len;
  HIPC(hipMemsetAsync(c->d_fwd.p, 0, 8 * w, c->stream));
  HIPC(hipMemsetAsync(c->d_rc.p, 0, 8 * w, c->stream));
  HIPC(hipMemsetAsync(c->d_fwdN.p, 0, 4 * w, c->stream));
  HIPC(hipMemsetAsync(c->d_rcNul.p, 0, 4 * w, c->stream));
  HIPC(hipMemcpyAsync(c->d_wofs.p, c->h_wofs.data(), 8ull * (nreads + 1), hipMemcpyHostToDevice,
                      c->stream));
  HIPC(hipMemcpyAsync(c->d_len.p, h_lengths, 4ull * nreads, hipMemcpyHostToDevice, c->stream));
  DBuf<uint32_t> err;
  if (err.alloc(1)) return fail(OVL_ERR_OOM, "err flag");
  HIPC(hipMemsetAsync(err.p, 0, 4, c->stream));
  if (nreads)
    hipLaunchKernelGGL(k_pack, dim3(nreads), dim3(128), 0, c->stream, d_bases, d_offsets,
                       c->d_len.p, c->d_wofs.p, c->d_fwd.p, c->d_rc.p, c->d_fwdN.p,
                       c->d_rcNul.p, c->d_flags.p, c->d_rcFirstNul.p, err.p,
                       c->P.kmer_len);
  HIPC(hipGetLastError());
  uint32_t h_err = 0;
  HIPC(hipMemcpyAsync(&h_err, err.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  if (h_err)
    return fail(OVL_ERR_BAD_INPUT,
                "reads hold characters other than ACGTN; the GPU path cannot represent them");
  c->first_iid = first_iid;
  c->nreads = nreads;
  return OVL_OK;
}

// Qualities (-w) into the packed layout: read r base i at wofs[r] * 32 + i.
__global__ void k_pack_quals(const uint8_t *q, const uint64_t *offs, const uint32_t *lens,
                             const uint64_t *wofs, uint8_t *out) {
  const uint32_t r = blockIdx.x;
  const uint64_t o = offs[r], w = wofs[r] * 32;
  for (uint32_t i = threadIdx.x; i < lens[r]; i += blockDim.x) out[w + i] = q[o + i];
}

static int load_quals(ovl_ctx *c, const uint8_t *d_quals, const uint64_t *d_offsets) {
  c->have_qual = false;
  if (!d_quals) return OVL_OK;
  uint64_t words = c->h_wofs.empty() ? 0 : c->h_wofs.back() + (c->h_len.back() + 31) / 32 + 1;
  if (c->d_qual.alloc(words * 32 + 64)) return fail(OVL_ERR_OOM, "qualities");
  hipLaunchKernelGGL(k_pack_quals, dim3(c->nreads), dim3(256), 0, c->stream, d_quals, d_offsets,
                     c->d_len.p, c->d_wofs.p, c->d_qual.p);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(c->stream));
  c->have_qual = true;
  return OVL_OK;
}

int ovl_load_reads(ovl_ctx *c, uint32_t first_iid, uint32_t nreads, const uint8_t *bases,
                   const uint64_t *offsets, const uint32_t *lengths, const uint8_t *quals) {
  if (!c) return fail(OVL_ERR_STATE, "null context");
  HIPC(hipSetDevice(c->device));
  uint64_t total = 0;
  for (uint32_t i = 0; i < nreads; i++) total = std::max(total, offsets[i] + lengths[i]);
  DBuf<uint8_t> db, dq;
  DBuf<uint64_t> doff;
  if (db.alloc(total + 64) || doff.alloc(nreads + 1)) return fail(OVL_ERR_OOM, "staging");
  HIPC(hipMemcpyAsync(db.p, bases, total, hipMemcpyHostToDevice, c->stream));
  HIPC(hipMemcpyAsync(doff.p, offsets, 8ull * nreads, hipMemcpyHostToDevice, c->stream));
  int rc = load_common(c, first_iid, nreads, db.p, doff.p, lengths);
  if (rc == OVL_OK && quals) {
    if (dq.alloc(total + 64)) return fail(OVL_ERR_OOM, "quality staging");
    HIPC(hipMemcpyAsync(dq.p, quals, total, hipMemcpyHostToDevice, c->stream));
    rc = load_quals(c, dq.p, doff.p);
  } else if (rc == OVL_OK) {
    c->have_qual = false;
  }
  (void)hipStreamSynchronize(c->stream);
  return rc;
}

int ovl_load_reads_device(ovl_ctx *c, uint32_t first_iid, uint32_t nreads,
                          const uint8_t *d_bases, const uint64_t *d_offsets,
                          const uint32_t *h_lengths, const uint8_t *d_quals) {
  if (!c) return fail(OVL_ERR_STATE, "null context");
  HIPC(hipSetDevice(c->device));
  int rc = load_common(c, first_iid, nreads, d_bases, d_offsets, h_lengths);
  if (rc == OVL_OK) rc = load_quals(c, d_quals, d_offsets);
  return rc;
}

static uint64_t kmer_code(const char *s, uint32_t k, bool *ok) {
  uint64_t key = 0;
  *ok = true;
  for (uint32_t j = 0; j < k; j++) {
    int v;
    switch (s[j] | 0x20) {
      case 'a': v = 0; break;
      case 'c': v = 1; break;
      case 'g': v = 2; break;
      case 't': v = 3; break;
      default: v = 0; *ok = false;
    }
    key |= (uint64_t)v << (2 * j);
  }
  return key;
}

int ovl_set_skip_kmers(ovl_ctx *c, const char *kmers, uint64_t n) {
  if (!c) return fail(OVL_ERR_STATE, "null context");
  uint32_t k = c->P.kmer_len;
  c->h_skip.clear();
  std::vector<char> rc(k);
  for (uint64_t i = 0; i < n; i++) {
    const char *s = kmers + i * k;
    bool ok;
    uint64_t f = kmer_code(s, k, &ok);
    if (!ok) return fail(OVL_ERR_BAD_INPUT, "skip k-mer %llu is not ACGT", (unsigned long long)i);
    c->h_skip.push_back(f);
    uint64_t r = 0;                                // reverse complement code
    for (uint32_t j = 0; j < k; j++) {
      uint64_t b = (f >> (2 * j)) & 3;
      r |= (3 - b) << (2 * (k - 1 - j));
    }
    c->h_skip.push_back(r);
  }
  std::sort(c->h_skip.begin(), c->h_skip.end());
  c->h_skip.erase(std::unique(c->h_skip.begin(), c->h_skip.end()), c->h_skip.end());
  c->have_index = false;
  return OVL_OK;
}

int ovl_build_hash_index(ovl_ctx *c, uint32_t bgn, uint32_t end) {
  int rc = clip_hash_range(c, bgn, end);
  if (rc) return rc;
  c->stats_hash_lib_lo = 0;
  c->stats_hash_lib_hi = UINT32_MAX;
  if ((rc = apply_hash_libs(c, 0, UINT32_MAX))) return rc;
  c->stats.ms_index = 0;
  return build_index(c, bgn, end);
}

int ovl_set_read_libraries(ovl_ctx *c, const uint32_t *lib_ids) {
  if (!c) return fail(OVL_ERR_STATE, "null context");
  if (c->nreads == 0) return fail(OVL_ERR_STATE, "no reads loaded");
  if (!lib_ids) { c->h_lib.clear(); return OVL_OK; }
  c->h_lib.assign(lib_ids, lib_ids + c->nreads);
  c->have_index = false;
  return OVL_OK;
}

void ovl_hash_limits_init(ovl_hash_limits *l) {
  l->max_hash_strings = 10000;
  l->max_hash_data_len = 100000000ull;
  l->hash_mask_bits = 22;
  l->max_hash_load = 0.6;
  l->min_lib_hash = 0;
  l->max_lib_hash = UINT32_MAX;
}

void ovl_driver_params_init(ovl_driver_params *d) {
  d->bgn_hash_iid = 1;
  d->end_hash_iid = UINT32_MAX;
  d->bgn_ref_iid = 1;
  d->end_ref_iid = UINT32_MAX;
  d->min_lib_ref = 0;
  d->max_lib_ref = UINT32_MAX;
  d->num_threads = 1;
  d->store_num_reads = 0;
  ovl_hash_limits_init(&d->limits);
}

int ovl_build_hash_batch(ovl_ctx *c, uint32_t bgn, uint32_t end, const ovl_hash_limits *L,
                         uint32_t *last_iid) {
  if (c) c->stats.ms_index = 0;
  return build_batch_impl(c, bgn, end, L, last_iid);
}

int ovl_seed_hits(ovl_ctx *c, uint32_t bgn, uint32_t end, ovl_seed_hit *out, uint64_t max_hits,
                  uint64_t *n_hits) {
  if (!c || !n_hits) return fail(OVL_ERR_STATE, "null argument");
  if (!c->have_index) return fail(OVL_ERR_STATE, "ovl_build_hash_index() first");
  HIPC(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  const uint32_t k = c->P.kmer_len;
  if (bgn < 1) bgn = 1;
  if (bgn < c->first_iid) bgn = c->first_iid;
  uint32_t last = c->first_iid + c->nreads - 1;
  if (end > last) end = last;
  std::vector<Unit> units;
  std::vector<uint64_t> uwin;
  query_rule(c).each(bgn, end, [&](uint32_t a, bool, uint64_t w) {
    for (uint32_t dir = 0; w && dir < 2; dir++) {
      units.push_back(Unit{a - c->first_iid, dir});
      uwin.push_back(w);
    }
  });
  // units in batches of <= 512 M probe slots; each batch's hits are written to a device
  // buffer of at most 256 M hits (4 GB), in pieces of whole units
  const uint64_t WIN_BUDGET = 512ull << 20, HIT_BUF = 256ull << 20;
  auto &fb = c->fb;
  // kept in the context (grow-only): a repeated call allocates nothing
  DBuf<uint64_t> &ucnt = fb.hcnt, &ubase = fb.hbase;
  DBuf<uint4> &hbuf = fb.hbuf;
  uint64_t total = 0, copied = 0;
  float ms_tot = 0;
  const uint32_t nu = (uint32_t)units.size();
  for (uint32_t u0 = 0; u0 < nu;) {
    const uint32_t u1 = take_within(uwin, u0, nu, WIN_BUDGET);
    const uint32_t nb = u1 - u0;
    std::vector<uint64_t> rbase;
    if (ucnt.grow(nb) || ubase.grow(nb)) return fail(OVL_ERR_OOM, "seed-hit buffers");
    if (int rc = probe_batch(c, units.data() + u0, uwin.data() + u0, nb, false, &rbase))
      return rc == OVL_ERR_OOM ? fail(OVL_ERR_OOM, "seed-hit buffers") : rc;
    HitArgs HA;
    HA.R = c->reads();
    HA.occ = c->d_occ.p;
    HA.units = fb.units.p;
    HA.rbase = fb.rbase.p;
    HA.probes = fb.probe.p;
    HA.nunits = nb;
    HA.k = k;
    HA.unit_hits = ucnt.p;
    HA.unit_base = nullptr;
    HA.out = nullptr;
    hipLaunchKernelGGL(k_hitlist, dim3((nb + 3) / 4), dim3(256), 0, s, HA);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(c->ev[3], s));
    std::vector<uint64_t> cnt(nb);
    HIPC(hipMemcpyAsync(cnt.data(), ucnt.p, 8ull * nb, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    // ms_seed_hits is device time of the kernels alone: the probe + count pass here, each
    // write pass below; the host's piece cuts, buffer growth, uploads, the hit copies to
    // the host and the syncs between pieces are outside every event pair
    {
      float t = 0;
      (void)hipEventElapsedTime(&t, c->ev[2], c->ev[3]);
      ms_tot += t;
    }
    // write pass, in pieces of whole units that fit the hit buffer: every unit's base
    // within its piece is computed once (one host pass over the batch) and uploaded once;
    // the hit buffer only grows (one allocation at the largest piece)
    std::vector<uint64_t> base(nb, 0);
    std::vector<uint32_t> cuts{0};
    uint64_t hmax = 1;
    for (uint32_t p0 = 0; p0 < nb; p0 = cuts.back()) {
      uint64_t h = 0;
      cuts.push_back(take_within(cnt, p0, nb, HIT_BUF, &h));
      for (uint32_t i = p0 + 1; i < cuts.back(); i++) base[i] = base[i - 1] + cnt[i - 1];
      hmax = std::max<uint64_t>(hmax, h);
    }
    if (hbuf.grow(hmax))
      return fail(OVL_ERR_OOM, "seed-hit list (%llu hits)", (unsigned long long)hmax);
    HIPC(hipMemcpyAsync(ubase.p, base.data(), 8ull * nb, hipMemcpyHostToDevice, s));
    for (size_t pc = 0; pc + 1 < cuts.size(); pc++) {
      const uint32_t p0 = cuts[pc], p1 = cuts[pc + 1];
      const uint64_t a2 = base[p1 - 1] + cnt[p1 - 1];
      HA.out = hbuf.p;
      HA.units = fb.units.p + p0;
      HA.rbase = fb.rbase.p + p0;
      HA.unit_base = ubase.p + p0;
      HA.nunits = p1 - p0;
      HIPC(hipEventRecord(c->ev[4], s));
      hipLaunchKernelGGL(k_hitlist, dim3((p1 - p0 + 3) / 4), dim3(256), 0, s, HA);
      HIPC(hipGetLastError());
      HIPC(hipEventRecord(c->ev[5], s));
      if (out && copied < max_hits && a2) {
        uint64_t n = std::min<uint64_t>(a2, max_hits - copied);
        HIPC(hipMemcpyAsync(out + copied, hbuf.p, 16ull * n, hipMemcpyDeviceToHost, s));
        copied += n;
      }
      HIPC(hipStreamSynchronize(s));
      float t = 0;
      (void)hipEventElapsedTime(&t, c->ev[4], c->ev[5]);
      ms_tot += t;
      total += a2;
    }
    u0 = u1;
  }
  c->stats.ms_seed_hits = ms_tot;
  *n_hits = total;
  return OVL_OK;
}

int ovl_find_overlaps(ovl_ctx *c, uint32_t bgn, uint32_t end, uint64_t *n_out) {
  return find_impl(c, bgn, end, 0, UINT32_MAX, false, n_out);
}

int ovl_overlap_driver(ovl_ctx *c, const ovl_driver_params *d, uint64_t *n_out) {
  if (!c || !d || !n_out) return fail(OVL_ERR_STATE, "null argument");
  DriverJob job{c, d};
  if (int rc = job.begin()) return rc;
  struct SqOff {
    ovl_ctx *c;
    ~SqOff() { c->sq_request = false; sq_release(c, false); }
  } sq_off{c};
  if (int rc = job.run()) return rc;
  *n_out = c->nout;
  return OVL_OK;
}

int ovl_fetch_overlaps(ovl_ctx *c, ovl_record *out, uint64_t max_records, uint64_t *n_copied) {
  if (!c) return fail(OVL_ERR_STATE, "null context");
  HIPC(hipSetDevice(c->device));
  std::vector<Rec> h(c->nout);
  if (c->nout)
    HIPC(hipMemcpy(h.data(), c->d_out.p, sizeof(Rec) * c->nout, hipMemcpyDeviceToHost));
  std::sort(h.begin(), h.end(), [](const Rec &x, const Rec &y) {
    if (x.a_iid != y.a_iid) return x.a_iid < y.a_iid;
    if (x.b_iid != y.b_iid) return x.b_iid < y.b_iid;
    if (x.w0 != y.w0) return x.w0 < y.w0;
    return x.w1 < y.w1;
  });
  uint64_t n = std::min<uint64_t>(max_records, h.size());
  for (uint64_t i = 0; i < n; i++) {
    out[i].a_iid = h[i].a_iid;
    out[i].b_iid = h[i].b_iid;
    out[i].dat[0] = h[i].w0;
    out[i].dat[1] = h[i].w1;
  }
  *n_copied = n;
  return OVL_OK;
}

int ovl_write_ovb(const ovl_record *recs, uint64_t n, const char *path, int with_counts) {
  if (!path || (n && !recs)) return fail(OVL_ERR_BAD_PARAM, "null argument");
  if (write_ovb_file(recs, n, path, with_counts != 0))
    return fail(OVL_ERR_BAD_INPUT, "writing '%s': %s", path, strerror(errno));
  return OVL_OK;
}

int ovl_ctx_write_ovb(ovl_ctx *c, const char *path) {
  if (!c) return fail(OVL_ERR_STATE, "null context");
  std::vector<ovl_record> h(c->nout);
  uint64_t got = 0;
  int rc = ovl_fetch_overlaps(c, h.data(), h.size(), &got);
  if (rc) return rc;
  return ovl_write_ovb(h.data(), got, path, 1);
}

int ovl_ctx_write_stats(ovl_ctx *c, const char *path) {
  if (!c || !path) return fail(OVL_ERR_STATE, "null argument");
  if (write_stats_file(c->stats, path))
    return fail(OVL_ERR_BAD_INPUT, "writing '%s': %s", path, strerror(errno));
  return OVL_OK;
}

int ovl_get_stats(ovl_ctx *c, ovl_stats *out) {
  if (!c) return fail(OVL_ERR_STATE, "null context");
  *out = c->stats;
  return OVL_OK;
}

}  // extern "C"
