// mhap_ctx.h -- the context of the MHAP stage: its device (capi::Device), the reads, the -f
// table, the sketch / index / compare buffers and the events that time a step.  Included by
// mhap.hip after the kernels.
#pragma once

struct mhap_ctx : capi::Device {
  mhap_params P;
  Event ev[4];                    // [0..1]: a step; [2..3]: the MinHash kernels of one batch
  uint32_t first_iid = 1, nreads = 0;
  std::vector<uint32_t> h_len;
  DevBuf<uint8_t> bases_own;
  const uint8_t *d_bases = nullptr;
  DevBuf<uint64_t> off_own;
  const uint64_t *d_off = nullptr;
  DevBuf<uint32_t> d_len;
  // weighting (MhapMain options + FrequencyCounts)
  mhap_weighting W{0.9, 3.0, 1e-5, 0, 0};
  bool has_table = false;
  DevBuf<FreqSlot> ftab;
  uint64_t fmask = 0;
  bool has_bloom = false;               // --supress-noise 1 with a -f table
  DevBuf<uint64_t> bloom;
  uint64_t bloom_bits = 0;
  int32_t bloom_k = 0;
  // second-stage acceptance: identity(inter / n) >= threshold, per (n, inter)
  DevBuf<uint32_t> pass;
  uint32_t pass_empty = 0;
  // sketches
  DevBuf<int32_t> minhash;
  DevBuf<uint64_t> ordered;
  DevBuf<uint32_t> ocount;
  DevBuf<uint64_t> mkeys, mkeys2;
  DevBuf<uint32_t> mpos, mpos2, msids;
  DevBuf<uint64_t> mkoff;
  DevBuf<uint8_t> msort_tmp;
  DevBuf<uint32_t> mbscnt;        // bit-sliced draws: per batch strand, its listed k-mers
  DevBuf<BestOut> mbest;          //   and the exact pass's minima [batch strand][H]
  // index
  DevBuf<uint64_t> keys, keys2, toff;
  DevBuf<uint32_t> vals, vals2;
  DevBuf<uint8_t> sort_tmp;
  size_t nkeys = 0;
  bool indexed = false;
  DevBuf<Cand> cand;
  DevBuf<RecDev> rec;
  DevBuf<uint32_t> ctr;
  DevBuf<unsigned long long> kctr;
  uint64_t nrec = 0;
  mhap_stats stats{};

  bool loaded(uint32_t bgn, uint32_t end) const {
    return mhap_host::range_loaded(bgn, end, first_iid, nreads);
  }
};

// milliseconds between two recorded events, after the stream was synchronised
static float elapsed(const Event &from, const Event &to) {
  float t = 0;
  (void)hipEventElapsedTime(&t, from, to);
  return t;
}
