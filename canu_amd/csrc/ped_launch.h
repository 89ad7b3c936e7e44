// ped_launch.h -- the host side of ped_wave.h's aligner that findErrors (fe.hip) and
// correctOverlaps (co.hip) share: the reads packed 2 bits per base, and the launches of a
// stage's align kernel over its overlaps, longest first, until every row log was large enough.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "capi_common.h"
#include "hip_raii.h"
#include "ped_host.h"

namespace ped {

// ------------------------------------------------------------------ packed reads

struct PackedReads {
  DevBuf<uint32_t> fwd, rc;          // rc only for the stage that reads it
  DevBuf<uint32_t> d_len;            // the two device tables only for the stage that keeps them
  DevBuf<uint64_t> d_word_off;
  uint32_t first_iid = 0, nreads = 0;
  std::vector<uint32_t> len;
  std::vector<uint64_t> word_off;    // first packed word of a read
  void clear() {
    fwd.release(); rc.release(); d_len.release(); d_word_off.release();
    nreads = 0;
    len.clear();
    word_off.clear();
  }
};

template <bool RC>
__global__ void k_ped_encode(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ src_off,
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
        const uint8_t ch = s[i] | 0x20;
        f |= (uint32_t)(ch == 'c' ? 1 : ch == 'g' ? 2 : ch == 't' ? 3 : 0) << (2 * j);   // the rest is 'a'
        if constexpr (RC) {
          const uint8_t cr = s[L - 1 - i] | 0x20;
          v |= (3 - (uint32_t)(cr == 'c' ? 1 : cr == 'g' ? 2 : cr == 't' ? 3 : 0)) << (2 * j);
        }
      }
      fwd[word_off[r] + w] = f;
      if constexpr (RC) rc[word_off[r] + w] = v;
    }
  }
}

// The reads of *_load_reads_device into R, every read followed by pad_words words of zero.
// RC: with the reverse complement.  keep_tables: d_len and d_word_off outlive the call.
template <bool RC>
int pack_reads(PackedReads &R, hipStream_t stream, int pad_words, bool keep_tables,
               uint32_t first_iid, uint32_t nreads, const uint8_t *d_bases,
               const uint64_t *d_offsets, const uint32_t *h_lengths) {
  R.clear();
  std::vector<uint64_t> woff(nreads);
  uint64_t words = 0;
  for (uint32_t i = 0; i < nreads; i++) {
    if (h_lengths[i] > AS_MAX_READLEN)
      return capi::fail(capi::ERR_BAD_INPUT, "read %u is %u bases, beyond AS_MAX_READLEN",
                        first_iid + i, h_lengths[i]);
    woff[i] = words;
    words += (h_lengths[i] + 15) / 16 + pad_words;
  }
  HIP_TRY(R.d_word_off.alloc(nreads));
  HIP_TRY(R.d_len.alloc(nreads));
  HIP_TRY(R.fwd.alloc(words));
  HIP_TRY(hipMemsetAsync(R.fwd.p, 0, R.fwd.bytes, stream));
  if (RC) {
    HIP_TRY(R.rc.alloc(words));
    HIP_TRY(hipMemsetAsync(R.rc.p, 0, R.rc.bytes, stream));
  }
  if (nreads) {
    HIP_TRY(hipMemcpyAsync(R.d_word_off.p, woff.data(), nreads * 8ull, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(R.d_len.p, h_lengths, nreads * 4ull, hipMemcpyHostToDevice, stream));
    const uint32_t grid = std::min<uint32_t>(nreads, 4096);
    hipLaunchKernelGGL(k_ped_encode<RC>, dim3(grid), dim3(256), 0, stream, d_bases, d_offsets,
                       R.d_word_off.p, R.d_len.p, nreads, R.fwd.p, R.rc.p);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipStreamSynchronize(stream));
  if (!keep_tables) { R.d_len.release(); R.d_word_off.release(); }
  R.first_iid = first_iid;
  R.nreads = nreads;
  R.len.assign(h_lengths, h_lengths + nreads);
  R.word_off = std::move(woff);
  return capi::OK;
}

// ------------------------------------------------------------------ the launches

struct MatchLimit {                  // Edit_Match_Limit of a context, grown on demand
  std::vector<int32_t> ml;
  double erate = -1.0;
};

struct AlignStage {                  // what differs between the stages, but for the kernel
  const char *env_per_error, *env_cap;   // the knobs: values per error, the exact first log
  int per_error;                     // *_LOG_PER_ERROR
  int extra_per_error, extra_fixed;  // ints a wave keeps behind its delta, from the limit
  uint32_t done_mask;                // an overlap with one of these bits was processed
  const char *internal;              // what F_INTERNAL means here
};

template <class Job>
struct AlignLaunch {                 // one launch, for the stage's argument struct
  const Job *jobs;
  const uint32_t *order;             // longest first
  uint32_t njobs, nwaves, blocks;
  uint32_t *next, *flags, *rows;
  const int32_t *match_limit;
  int32_t *scratch;
  uint64_t log_cap, per_wave;
  int32_t max_limit;
};

struct AlignStats {
  uint64_t n_generic = 0, n_staged = 0, rows = 0, regrows = 0, scratch_bytes = 0;
  double ms_align = 0;
};

// Every job (m, n, limit) through the stage's kernel: launch(L) fills the stage's arguments
// from L, launches on dev.stream and returns hipGetLastError().  The overlaps whose row log
// overflowed run again with the worst-case log of the largest among them.  fl gets the
// outcome bits of every job; S is kept up to date on a failure as well.
template <class Job, class Launch>
int align_all(const capi::Device &dev, const AlignStage &stage, MatchLimit &cache, double erate,
              const std::vector<Job> &jobs, Launch launch, std::vector<uint32_t> &fl,
              AlignStats &S) {
  const uint64_t n = jobs.size();
  fl.assign(n, 0);
  if (n == 0) return capi::OK;
  hipStream_t stream = dev.stream;
  int32_t max_limit = 0;
  for (const Job &J : jobs) max_limit = std::max(max_limit, J.limit);
  if (cache.erate != erate || (int32_t)cache.ml.size() < max_limit + 2) {
    const int32_t max_errors = 1 + (int32_t)(uint32_t)(erate * AS_MAX_READLEN);
    init_match_limit(cache.ml, erate, max_errors, max_limit + 1);
    cache.erate = erate;
  }

  std::vector<uint32_t> todo(n), rows(n);
  std::iota(todo.begin(), todo.end(), 0u);
  std::stable_sort(todo.begin(), todo.end(), [&](uint32_t x, uint32_t y) {
    return std::min(jobs[x].m, jobs[x].n) > std::min(jobs[y].m, jobs[y].n);
  });
  DevBuf<Job> d_jobs;
  DevBuf<uint32_t> d_order, d_next, d_flags, d_rows;
  DevBuf<int32_t> d_ml;
  HIP_TRY(d_jobs.alloc(n));
  HIP_TRY(d_order.alloc(n));
  HIP_TRY(d_next.alloc(1));
  HIP_TRY(d_flags.alloc(n));
  HIP_TRY(d_rows.alloc(n));
  HIP_TRY(d_ml.alloc(cache.ml.size()));
  HIP_TRY(hipMemcpyAsync(d_jobs.p, jobs.data(), n * sizeof(Job), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemcpyAsync(d_ml.p, cache.ml.data(), cache.ml.size() * 4, hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(d_flags.p, 0, n * 4, stream));
  HIP_TRY(hipMemsetAsync(d_rows.p, 0, n * 4, stream));

  int per_error = stage.per_error;
  if (const char *e = getenv(stage.env_per_error)) per_error = std::max(1, atoi(e));
  int32_t cur_limit = max_limit;
  uint64_t log_cap = row_log_first(per_error, max_limit);
  // test knob: the exact size of the first row log
  if (const char *e = getenv(stage.env_cap)) log_cap = std::max<uint64_t>(2, strtoull(e, nullptr, 10));
  Event e0, e1;
  HIP_TRY(e0.create());
  HIP_TRY(e1.create());
  while (!todo.empty()) {
    const uint64_t nt = todo.size();
    const uint64_t extra = (uint64_t)stage.extra_per_error * cur_limit + stage.extra_fixed;
    const LaunchSize Z = launch_size(log_cap, cur_limit, extra, nt, dev.n_cu);
    if (!Z.ok)
      return capi::fail(capi::ERR_UNSUPPORTED, "a row log of %llu entries (%d errors allowed) is "
                        "beyond the 32-bit offsets of this build", (unsigned long long)log_cap,
                        cur_limit);
    DevBuf<int32_t> d_scratch;
    HIP_TRY(d_scratch.alloc(Z.per_wave * Z.nwaves));
    S.scratch_bytes = Z.scratch_bytes;
    HIP_TRY(hipMemcpyAsync(d_order.p, todo.data(), nt * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(d_next.p, 0, 4, stream));
    const AlignLaunch<Job> L{d_jobs.p, d_order.p, (uint32_t)nt, (uint32_t)Z.nwaves, Z.blocks,
                             d_next.p, d_flags.p, d_rows.p, d_ml.p, d_scratch.p, log_cap,
                             Z.per_wave, cur_limit};
    HIP_TRY(hipEventRecord(e0, stream));
    hipError_t le = launch(L);
    HIP_TRY(hipEventRecord(e1, stream));
    hipError_t se = hipStreamSynchronize(stream);
    HIP_TRY(le);
    HIP_TRY(se);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    S.ms_align += ms;
    HIP_TRY(hipMemcpy(fl.data(), d_flags.p, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rows.data(), d_rows.p, n * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> again;
    int32_t next_limit = 0;
    for (uint32_t i : todo) {
      S.rows += rows[i];
      if (fl[i] & F_INTERNAL) return capi::fail(capi::ERR_HIP, "overlap %u: %s", i, stage.internal);
      if (fl[i] & F_OVERFLOW) {
        again.push_back(i);
        next_limit = std::max(next_limit, jobs[i].limit);
      } else if (!(fl[i] & stage.done_mask)) {
        return capi::fail(capi::ERR_HIP, "overlap %u was not processed", i);
      }
    }
    if (!again.empty()) {
      log_cap = row_log_regrown(log_cap, next_limit);
      if (!log_cap) return capi::fail(capi::ERR_HIP, "row log overflow at its worst-case size");
      S.regrows++;
      cur_limit = next_limit;
    }
    todo.swap(again);
  }
  for (uint64_t i = 0; i < n; i++) {
    S.n_generic += !!(fl[i] & F_GENERIC);
    S.n_staged += !!(fl[i] & F_STAGED);
  }
  return capi::OK;
}

}  // namespace ped
