// ovl_build.hip -- the index and hash-batch builder, host side (the kernels are in
// ovl_index.hip): build_index and its steps, the window cap of one index, and
// Build_Hash_Index's loading loop (build_batch_impl).  The shapes and stop rules are
// ovl_plan.h's.  Part of ovl_api.hip's translation unit.

// ovl_sq.hip's, which comes after this file
static void sq_release(ovl_ctx *c, bool free_mem = true);
static size_t sq_held_bytes(const ovl_ctx *c);
static bool sq_bloom();

static __global__ void k_clear_screen(uint32_t *flags, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flags[i] &= ~6u;                 // the screened-end bits of the last index
}

// OVL_RFLAG_NOHASH from a per-read byte (1 = not hashed); nohash == null clears it.
static __global__ void k_set_nohash(uint32_t *flags, const uint8_t *nohash, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    uint32_t f = flags[i] & ~OVL_RFLAG_NOHASH;
    if (nohash && nohash[i]) f |= OVL_RFLAG_NOHASH;
    flags[i] = f;
  }
}

// Mark the reads outside [lo, hi] as not hashed (device flag), or clear every mark.
static int apply_hash_libs(ovl_ctx *c, uint32_t lo, uint32_t hi) {
  bool any = false;
  std::vector<uint8_t> nh;
  if (!c->h_lib.empty() && (lo > 0 || hi < UINT32_MAX)) {
    nh.resize(c->nreads);
    for (uint32_t r = 0; r < c->nreads; r++) {
      nh[r] = (c->h_lib[r] < lo || c->h_lib[r] > hi) ? 1 : 0;
      any |= nh[r] != 0;
    }
  }
  if (!any && !c->nohash_set) return OVL_OK;
  DBuf<uint8_t> d;
  if (any) {
    if (d.alloc(c->nreads)) return fail(OVL_ERR_OOM, "library flags");
    HIPC(hipMemcpyAsync(d.p, nh.data(), c->nreads, hipMemcpyHostToDevice, c->stream));
  }
  hipLaunchKernelGGL(k_set_nohash, dim3((c->nreads + 255) / 256), dim3(256), 0, c->stream,
                     c->d_flags.p, any ? d.p : nullptr, c->nreads);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(c->stream));
  c->nohash_set = any;
  return OVL_OK;
}

// ends the bracket that an hipEventRecord(ev[0]) opened: its device time goes to ms_index
static int close_index_bracket(ovl_ctx *c) {
  HIPC(hipEventRecord(c->ev[1], c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  float ms = 0;
  (void)hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
  c->stats.ms_index += ms;
  return OVL_OK;
}

// One build_index call: the shapes (ovl_plan.h) and the build's steps in order.
struct IndexBuild {
  ovl_ctx *c;
  hipStream_t s;
  uint32_t h0, h1;               // hash reads [h0, h1), 0-based
  uint32_t n_skip = 0;
  uint64_t P = 0;                // record bound: every window of the hash reads + the skip k-mers
  IndexShape X;
  uint32_t hm[4] = {0, 0, 0, 0}; // b_misc: records, big buckets, the largest bucket's distinct k-mers
  bool bloom_built = false;      // table(): the filter was asked for and fits

  // P, the skip k-mers uploaded, the shapes.  P follows the device's rule (k_coarse_*): a read
  // is left out for its library only when apply_hash_libs marked reads (nohash_set), which it
  // does for the range in stats_hash_lib_* and only when libraries are loaded
  int shapes() {
    const bool marked = c->nohash_set;
    const HashRule H = hash_rule(c, marked ? c->stats_hash_lib_lo : 0,
                                 marked ? c->stats_hash_lib_hi : UINT32_MAX);
    if (h1 > h0) P = hash_windows(H, c->first_iid + h0, c->first_iid + h1 - 1);
    n_skip = (uint32_t)c->h_skip.size();
    P += n_skip;
    if (P >= 0xFFFFFFF0ull)
      return fail(OVL_ERR_UNSUPPORTED, "hash batch with %llu k-mers; use a smaller -h range",
                  (unsigned long long)P);
    if (n_skip) {
      if (c->d_skip.alloc(n_skip)) return fail(OVL_ERR_OOM, "skip");
      HIPC(hipMemcpyAsync(c->d_skip.p, c->h_skip.data(), 8ull * n_skip, hipMemcpyHostToDevice, s));
    }
    X = index_shape(P);
    return OVL_OK;
  }

  int allocate() {
    auto rec_alloc = [&](uint64_t n) {
      return c->d_tmpR.alloc(n) || c->d_midR.alloc(n) || c->d_tmpM2.alloc(n) || c->d_occ.alloc(n);
    };
    if (!(c->index_reserve > P && !rec_alloc(c->index_reserve)) && rec_alloc(P))
      return fail(OVL_ERR_OOM, "index records (%llu)", (unsigned long long)P);
    const uint32_t ncb = 1u << X.cb;
    if (c->b_hist.alloc(ncb) || c->b_cstart.alloc(ncb) || c->b_cursor.alloc(ncb) ||
        c->b_fstart.alloc(X.nfine) || c->b_fcnt.alloc(X.nfine) || c->b_misc.alloc(8) ||
        c->b_big.alloc(2 * (size_t)X.nfine))
      return fail(OVL_ERR_OOM, "index scratch");
    HIPC(hipMemsetAsync(c->b_hist.p, 0, 4 * ncb, s));
    HIPC(hipMemsetAsync(c->b_misc.p, 0, 32, s));
    return OVL_OK;
  }

  // coarse passes: 2 blocks of 16 waves per CU (32 waves: the coarse scatter is latency-
  // bound -- a dependent packed-base load, LDS atomic and 16-B store per window -- and its
  // 32 KB of LDS histograms per block would cap 4-wave blocks at 20 waves per CU).
  // Measured on 50k x 10 kb: 256 threads x 4 per CU 35.7 ms index, 512 x 4 34.0, 1024 x 2
  // 32.4 (with the parallel fine-bucket scan)
#ifndef OVL_COARSE_BPCU
#define OVL_COARSE_BPCU 2
#endif
#ifndef OVL_COARSE_THREADS
#define OVL_COARSE_THREADS 1024
#endif
  int coarse_passes() {
    const uint32_t k = c->P.kmer_len, ncb = 1u << X.cb;
    BuildArgs A;
    A.R = c->reads();
    A.h0 = h0;
    A.h1 = h1;
    uint32_t nblk = std::max<uint32_t>(1, std::min<uint32_t>(h1 - h0, OVL_COARSE_BPCU * c->n_cu));
    A.reads_per_block = (h1 - h0 + nblk - 1) / nblk;
    if (A.reads_per_block == 0) A.reads_per_block = 1;
    A.k = k;
    A.min_len = c->P.min_olap_len;
    A.kmask = (1ull << (2 * k)) - 1;
    A.skip = n_skip ? c->d_skip.p : nullptr;
    A.n_skip = n_skip;
    A.cb_bits = X.cb;
    A.fb_bits = X.fb;
    hipLaunchKernelGGL(k_coarse_hist, dim3(nblk), dim3(OVL_COARSE_THREADS), 0, s, A, c->b_hist.p);
    hipLaunchKernelGGL(k_scan_u32, dim3(1), dim3(1024), 0, s, c->b_hist.p, c->b_cstart.p, ncb,
                       c->b_misc.p + 0);
    HIPC(hipMemcpyAsync(c->b_cursor.p, c->b_cstart.p, 4 * ncb, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_coarse_scatter, dim3(nblk), dim3(OVL_COARSE_THREADS), 0, s, A,
                       c->b_cursor.p, c->d_tmpR.p);
    return OVL_OK;
  }

  // the fine pass (every coarse bucket's records into sorted k-mer runs), then the fine
  // buckets too large for a wave's sort buffer; hm holds the build's counts afterwards
  int fine_pass() {
    const uint32_t nfb = 1u << X.fb;
    uint32_t *misc = c->b_misc.p;
    FineArgs F;
    F.inR = c->d_tmpR.p;
    F.midR = c->d_midR.p;
    F.outM = c->d_tmpM2.p;
    F.outP = c->d_occ.p;
    F.cstart = c->b_cstart.p;
    F.ccnt = c->b_hist.p;
    F.fstart = c->b_fstart.p;
    F.fcnt = c->b_fcnt.p;
    F.big_list = c->b_big.p;
    F.big_n = misc + 1;
    F.max_distinct = misc + 2;
    F.cb_bits = X.cb;
    F.fb_bits = X.fb;
    F.cap = X.cap;
    // the sort phase: runs grouped in an LDS hash table, records in registers (cap / 64 per
    // lane); bitonic sorts when the grouped layout would not fit a CU's LDS (cap 1024)
    const bool group = fine_lds_bytes(true, nfb, F.cap) + 256 <= 160 * 1024;
    const size_t fine_lds = fine_lds_bytes(group, nfb, F.cap);
    const void *kf =
        !group           ? reinterpret_cast<const void *>(k_fine<1, false>)
        : F.cap <= 64    ? reinterpret_cast<const void *>(k_fine<1, true>)
        : F.cap <= 128   ? reinterpret_cast<const void *>(k_fine<2, true>)
        : F.cap <= 256   ? reinterpret_cast<const void *>(k_fine<4, true>)
                         : reinterpret_cast<const void *>(k_fine<8, true>);
    if (fine_lds > 65536)
      HIPC(hipFuncSetAttribute(kf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fine_lds));
    void *kargs[] = {&F};
    HIPC(hipLaunchKernel(kf, dim3(1u << X.cb), dim3(OVL_FINE_WAVES * 64), kargs, fine_lds, s));
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(hm, misc, 16, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    // P counted every window; windows holding an 'n' are not hashed (key_is_bad)
    if (hm[0] > P) return fail(OVL_ERR_HIP, "index count %u exceeds bound %llu", hm[0],
                               (unsigned long long)P);
    const uint32_t nbig = hm[1];
    if (!nbig) return OVL_OK;
    std::vector<uint32_t> bl(2 * nbig);
    HIPC(hipMemcpy(bl.data(), c->b_big.p, 8ull * nbig, hipMemcpyDeviceToHost));
    uint32_t mx = 0;
    for (uint32_t i = 0; i < nbig; i++) mx = std::max(mx, bl[2 * i + 1]);
    uint32_t n2 = 1;
    while (n2 < mx) n2 <<= 1;
    DBuf<uint64_t> sM, sP;
    if (sM.alloc((size_t)n2 * nbig) || sP.alloc((size_t)n2 * nbig))
      return fail(OVL_ERR_OOM, "big fine buckets");
    hipLaunchKernelGGL(k_fine_big, dim3(nbig), dim3(1024), 0, s, c->d_tmpM2.p, c->d_occ.p,
                       c->b_big.p, sM.p, sP.p, n2, misc + 2);
    HIPC(hipMemcpyAsync(hm, misc, 16, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    return OVL_OK;
  }

  // the table (and the batch's Bloom filter) from the sorted runs: one wave per fine bucket
  int table(bool bloom) {
    const TableShape S = table_shape(X, hm[2], c->dense_tables, hm[0], bloom);
    c->slice_bits = S.slice_bits;
    c->tab_bits = S.tab_bits;
    if (c->d_tab.alloc(1ull << c->tab_bits)) return fail(OVL_ERR_OOM, "table 2^%u", c->tab_bits);
    if (bloom) {
      if (c->d_bloom.alloc((size_t)X.nfine << S.bloom_w)) return fail(OVL_ERR_OOM, "bloom filter");
      c->bloom_w = S.bloom_w;
    }
    if (S.refused)
      return fail(OVL_ERR_UNSUPPORTED, "k-mer slice too large (%u)", 1u << c->slice_bits);
    TableArgs T;
    T.M = c->d_tmpM2.p;
    T.P = c->d_occ.p;
    T.fstart = c->b_fstart.p;
    T.fcnt = c->b_fcnt.p;
    T.tab = c->d_tab.p;
    T.nfine = X.nfine;
    T.slice_bits = c->slice_bits;
    T.tab_bits = c->tab_bits;
    T.len = c->d_len.p;
    T.rflags = c->d_flags.p;
    T.first_iid = c->first_iid;
    T.k = c->P.kmer_len;
    T.bloom = S.bloom ? c->d_bloom.p : nullptr;
    T.bloom_w = S.bloom ? S.bloom_w : 0;
    hipLaunchKernelGGL(k_table, dim3((X.nfine + S.wpb - 1) / S.wpb), dim3(64 * S.wpb), S.lds, s, T);
    HIPC(hipGetLastError());
    bloom_built = S.bloom;
    return OVL_OK;
  }
};

// The index over hash reads bgn..end (clipped to the loaded reads by the callers).
// bloom: also build the batch's Bloom filter (OverlapDriver batches, whose searches are
// mostly by reads outside the hash range; see use_bloom)
// table = false: the records grouped into k-mer runs only (what the driver's first-read
// histogram reads to find a load cut), no table, filter or screened-end flags: the index is
// not searchable (have_index stays false)
static int build_index(ovl_ctx *c, uint32_t bgn, uint32_t end, bool bloom = false,
                       bool table = true) {
  hipStream_t s = c->stream;
  c->hash_bgn_iid = bgn;
  c->hash_end_iid = end;
  c->have_index = false;
  c->bloom_ok = false;
  HIPC(hipEventRecord(c->ev[0], s));
  hipLaunchKernelGGL(k_clear_screen, dim3((c->nreads + 255) / 256), dim3(256), 0, s,
                     c->d_flags.p, c->nreads);
  const uint32_t h0 = bgn - c->first_iid;
  IndexBuild B{c, s, h0, (end >= bgn) ? end - c->first_iid + 1 : h0};
  int rc;
  if ((rc = B.shapes()) || (rc = B.allocate()) || (rc = B.coarse_passes()) || (rc = B.fine_pass()))
    return rc;
  if (table && (rc = B.table(bloom))) return rc;
  if ((rc = close_index_bracket(c))) return rc;
  c->index_records = B.hm[0];
  // the build scratch (2 x 16 B per window) stays allocated for the next build: freeing and
  // re-allocating gigabytes per job costs tens of ms on some hosts (and HBM is plentiful)
  c->have_index = table;
  c->bloom_ok = B.bloom_built;
  return OVL_OK;
}

static int clip_hash_range(ovl_ctx *c, uint32_t &bgn, uint32_t &end) {
  if (!c) return fail(OVL_ERR_STATE, "null context");
  if (c->nreads == 0) return fail(OVL_ERR_STATE, "no reads loaded");
  HIPC(hipSetDevice(c->device));
  if (bgn < 1) bgn = 1;
  if (bgn < c->first_iid) bgn = c->first_iid;
  uint32_t last = c->first_iid + c->nreads - 1;
  if (end > last) end = last;
  return OVL_OK;
}

// the previous search's buffers freed, when an index build needs their memory
static void release_find_buffers(ovl_ctx *c) {
  auto &f = c->fb;
  f.units.release(); f.pnodes.release(); f.pairs.release();
  f.rbase.release(); f.probe.release(); f.uhits.release();
  f.uflags.release(); f.done.release(); f.dset.release(); f.big.release(); f.live.release();
  f.defer.release(); f.defer2.release(); f.okey.release(); f.oidx.release();
  f.okey2.release(); f.oidx2.release(); f.otmp.release(); f.pool.release();
  f.ok64a.release(); f.ok64b.release(); f.dkey.release(); f.oa.release(); f.ob.release();
  f.ucnt.release(); f.useg.release(); f.hcnt.release(); f.hbase.release(); f.hbuf.release();
  f.rows.release(); f.rowdir.release(); f.deltas.release();
  sq_release(c);
  // the extension accumulator's buffers, once nothing waits in them
  if (c->acc.np == 0) {
    c->acc.units.release(); c->acc.pnodes.release(); c->acc.pairs.release();
    c->acc.nu = c->acc.nn = 0;
  }
}

// HBM figures of the last index_window_cap call, for error messages
static thread_local uint64_t g_cap_free = 0, g_cap_reserve = 0;

// The most windows one index build may take: its records are 32-bit indexed, and its build
// needs ~112 B per window (two 16-B record arrays, keys and positions, a table of up to 4
// slots per window) out of the HBM that is free now plus what the current index and the
// previous search hold (released when a build needs it), less 64 GB kept for the seed and
// extension buffers (whose budgets shrink to fit).  OVL_TEST_INDEX_WINDOW_CAP lowers
// it (tests of the capped path).
static uint64_t index_window_cap(ovl_ctx *c) {
  uint64_t cap = 0xFFFFFFF0ull - 64 - c->h_skip.size();
  size_t fr = 0, tot = 0;
  g_cap_free = g_cap_reserve = 0;
  if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
    const auto &f = c->fb;
    const uint64_t held = 2ull * c->d_tmpR.n * sizeof(Rec2) + 2ull * c->d_occ.n * 8 +
                          (uint64_t)c->d_tab.n * sizeof(TabEntry) + f.probe.n * sizeof(Probe) +
                          (f.pool.n + f.pnodes.n) * sizeof(Node) + f.pairs.n * sizeof(PairRec) +
                          4ull * (f.rows.n + f.rowdir.n + f.deltas.n) +
                          c->acc.units.n * sizeof(Unit) + c->acc.pnodes.n * sizeof(Node) +
                          c->acc.pairs.n * sizeof(PairRec) +
                          (c->sq.on ? 0 : sq_held_bytes(c));   // an earlier job's sorted windows
    // the search and extension buffers of the batch are sized by budget (up to ~64 GB on a
    // 288 GB part): keep that much aside, or a fifth of a smaller device
    const uint64_t avail = fr + held;
    const uint64_t reserve = std::min<uint64_t>(64ull << 30, (uint64_t)tot / 5);
    g_cap_free = avail;
    g_cap_reserve = reserve;
    cap = std::min<uint64_t>(cap, avail > reserve ? (avail - reserve) / 112 : 0);
  }
  if (const char *e = getenv("OVL_TEST_INDEX_WINDOW_CAP"))
    cap = std::min<uint64_t>(cap, strtoull(e, nullptr, 10));
  return std::max<uint64_t>(cap, 1);
}

// build_index; when it runs out of memory the previous batch's search buffers make room (the
// next search grows them again) and it runs once more
static int build_with_release(ovl_ctx *c, uint32_t bgn, uint32_t end, bool bloom, bool table = true) {
  int rc = build_index(c, bgn, end, bloom, table);
  if (rc != OVL_ERR_OOM) return rc;
  release_find_buffers(c);
  c->stats.find_releases++;
  return build_index(c, bgn, end, bloom, table);
}

static int batch_too_big(uint32_t bgn, uint32_t e, uint64_t windows, uint64_t wcap) {
  return fail(OVL_ERR_UNSUPPORTED, "hash batch %u-%u holds %llu k-mers, more than one index "
              "on this GPU (%llu: %.1f GB free or held by this context, %.1f GB kept for "
              "the search buffers); lower --hashstrings", bgn, e,
              (unsigned long long)windows, (unsigned long long)wcap, g_cap_free / 1e9,
              g_cap_reserve / 1e9);
}

// Per read of bgn..eb, the k-mers of the index just built over them that no earlier read
// holds (what Hash_Entries grows by when the reference loads that read)
static int first_read_histogram(ovl_ctx *c, uint32_t bgn, uint32_t eb, std::vector<uint32_t> *h) {
  hipStream_t s = c->stream;
  const uint32_t nr = eb - bgn + 1;
  DBuf<uint32_t> &hist = c->b_first;
  if (hist.alloc(nr)) return fail(OVL_ERR_OOM, "first-read histogram");
  HIPC(hipMemsetAsync(hist.p, 0, 4ull * nr, s));
  const uint32_t n = (uint32_t)c->index_records;
  if (n && nr <= 2u * OVL_FR_WORDS)
    hipLaunchKernelGGL(k_first_reads_lds, dim3((n + OVL_FR_CHUNK - 1) / OVL_FR_CHUNK), dim3(1024),
                       0, s, c->d_tmpM2.p, c->d_occ.p, n, bgn, nr, hist.p);
  else if (n)
    hipLaunchKernelGGL(k_first_reads, dim3(std::min<uint32_t>((n + 255) / 256, 16384)), dim3(256),
                       0, s, c->d_tmpM2.p, c->d_occ.p, n, bgn, hist.p);
  HIPC(hipGetLastError());
  h->resize(nr);
  HIPC(hipMemcpyAsync(h->data(), hist.p, 4ull * nr, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  return OVL_OK;
}

// The index of a prefix bgn..eb made the index of the batch bgn..el, el < eb: cut down
// (k_cut_index), or built again over the batch (OVL_CUT_FILTER=0; read per build, so a test can
// compare the two in one process).
// After a cut, index_records stays the prefix's count on purpose: the occurrence array is the
// prefix's, and the cut table's runs point into it (an export copies all of it).  Reads in
// (el, eb] keep the screened-end bits the prefix build set; they are no target of this batch,
// and the next build clears every read's bits (k_clear_screen)
static int apply_load_cut(ovl_ctx *c, uint32_t bgn, uint32_t el, bool bloom) {
  const bool cut = !getenv("OVL_CUT_FILTER") || atoi(getenv("OVL_CUT_FILTER")) != 0;
  if (!cut) return build_index(c, bgn, el, bloom);
  hipStream_t s = c->stream;
  HIPC(hipEventRecord(c->ev[0], s));
  hipLaunchKernelGGL(k_cut_index, dim3(8 * c->n_cu), dim3(256), 0, s, c->d_tab.p,
                     1ull << c->tab_bits, (const uint64_t *)c->d_occ.p, el);
  HIPC(hipGetLastError());
  if (int rc = close_index_bracket(c)) return rc;
  c->hash_end_iid = el;
  return OVL_OK;
}

// Build_Hash_Index's loading loop (overlapInCore-Build_Hash_Index.C:495-541): before each
// read it requires String_Ct < Max_Hash_Strings, total_len < Max_Hash_Data_Len and
// Hash_Entries < hash_entry_limit.  The first two are known from the lengths (ovl_plan.h
// hash_stop); the third needs the batch's k-mers, so the index is built over the first two's
// range and its first-occurrence histogram decides -- cutting or rebuilding the shorter batch
// when the table load stops it earlier.
// boundaries_only: the batch's end alone (the driver's first phase, super-batches): no
// build unless the table load may cut the batch, and then no table and no cut index
static int build_batch_impl(ovl_ctx *c, uint32_t bgn, uint32_t end, const ovl_hash_limits *L,
                            uint32_t *last_iid, bool boundaries_only = false) {
  int rc = clip_hash_range(c, bgn, end);
  if (rc) return rc;
  if (!L) return fail(OVL_ERR_BAD_PARAM, "null limits");
  if (L->max_hash_strings == 0) return fail(OVL_ERR_BAD_PARAM, "no memory model (--hashstrings 0)");
  if (L->hash_mask_bits == 0 || L->hash_mask_bits > 40)
    return fail(OVL_ERR_BAD_PARAM, "--hashbits %u", L->hash_mask_bits);
  if (end < bgn) return fail(OVL_ERR_BAD_PARAM, "empty hash range %u-%u", bgn, end);
  const HashRule H = hash_rule(c, L->min_lib_hash, L->max_lib_hash);
  const uint64_t max_alloc = hash_alloc_bases(H, bgn, end);
  if (hash_alloc_refused(max_alloc, L->max_hash_data_len, AS_MAX_READLEN))
    return fail(OVL_ERR_BAD_PARAM,
                "hash range %u-%u holds %llu bases, more than --hashdatalen %llu + "
                "AS_MAX_READLEN (Build_Hash_Index.C:523 asserts)", bgn, end,
                (unsigned long long)max_alloc, (unsigned long long)L->max_hash_data_len);
  const HashStop S = hash_stop(H, bgn, end, L->max_hash_strings, L->max_hash_data_len);
  const uint64_t windows = S.windows;
  uint32_t e = S.e;
  c->stats_hash_lib_lo = L->min_lib_hash;
  c->stats_hash_lib_hi = L->max_lib_hash;
  if ((rc = apply_hash_libs(c, L->min_lib_hash, L->max_lib_hash))) return rc;
  // table load: at most one entry per window, so only a batch with more windows than the
  // limit can be stopped by it
  const uint64_t entry_limit = hash_entry_limit(L->max_hash_load, L->hash_mask_bits);
  const bool load_may_cut = windows >= entry_limit && e > bgn;
  if (boundaries_only && !load_may_cut) {
    // the driver's first phase builds nothing here, but a batch no index can hold would
    // become a super-batch of its own and fail later with a bare out-of-memory
    const uint64_t wcap = index_window_cap(c);
    if (windows > wcap) return batch_too_big(bgn, e, windows, wcap);
    *last_iid = e;
    return OVL_OK;
  }
  // When the load may cut the batch, the first build covers only a prefix (ovl_plan.h
  // first_build_target), doubled while the load does not stop inside it.  One index holds at
  // most wcap windows (32-bit records; this GPU's free HBM): the previous batch's search
  // buffers are released only when the build needs their memory, since every (re)allocation
  // costs ~30 GB/s of clearing.
  uint64_t target = load_may_cut ? first_build_target(windows, entry_limit, c->cut_windows_hint)
                                 : windows;
  for (;;) {
    const uint64_t wcap = index_window_cap(c);
    if (!load_may_cut && windows > wcap) return batch_too_big(bgn, e, windows, wcap);
    const uint64_t tw = std::min(target, wcap);
    const uint32_t eb = prefix_end(H, bgn, e, tw);
    const bool bloom = !boundaries_only && (!c->sq.on || sq_bloom());
    if ((rc = build_with_release(c, bgn, eb, bloom, !boundaries_only))) return rc;
    if (!load_may_cut) break;
    std::vector<uint32_t> h;
    if ((rc = first_read_histogram(c, bgn, eb, &h))) return rc;
    const uint32_t cut = load_cut(h.data(), (uint32_t)h.size(), entry_limit);
    if (cut < h.size()) {
      const uint32_t el = bgn + cut;
      if (el < eb && !boundaries_only && (rc = apply_load_cut(c, bgn, el, bloom))) return rc;
      e = el;
      c->cut_windows_hint = hash_windows(H, bgn, el);
      break;
    }
    if (eb == e) break;                           // the whole range, under the load limit
    if (tw >= wcap)
      return fail(OVL_ERR_UNSUPPORTED, "hash batch from %u: the table load limit (%llu entries, "
                  "--hashbits %u --hashload %g) is not reached within %llu k-mers, the most one "
                  "index holds on this GPU; lower --hashbits or --hashload", bgn,
                  (unsigned long long)entry_limit, L->hash_mask_bits, L->max_hash_load,
                  (unsigned long long)wcap);
    target = doubled_build_target(windows, tw);
  }
  *last_iid = e;
  return OVL_OK;
}
