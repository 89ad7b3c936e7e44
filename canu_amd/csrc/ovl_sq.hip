// ovl_sq.hip -- the sorted query windows of an OverlapDriver job, host side (the kernels are in
// ovl_seed.hip): units, run layout (ovl_plan.h sq_layout), fit-or-decline, allocation, and
// every run's sort and check.  Part of ovl_api.hip's translation unit.

// the sorted-window probe checks the batch's Bloom filter before the table (OVL_SQ_BLOOM=0:
// it reads the table for every window, and the batch is built without the filter)
static bool sq_bloom() {
  static const bool on = !getenv("OVL_SQ_BLOOM") || atoi(getenv("OVL_SQ_BLOOM")) != 0;
  return on;
}

// The sorted query windows of an OverlapDriver job (k_sq_keys / k_probe_sorted): the units
// find_impl searches (ref reads bgn..end of libraries [lib_lo, lib_hi] at least --minlength
// and k long, both orientations, read order), their windows keyed by mix64(k-mer) and
// radix-sorted once, in runs of <= 2^29 windows.  A batch searches the units of the reads
// below its last hash read: a prefix of them, so per run a window-id bound.  Off (and the
// random-lookup probe used) when the keys would take more than half the free HBM.
//
// The device arrays outlive the job (free_mem false at a job's end): they are grow-only like
// the search buffers, since hipMalloc of the ~58 GB a configs[4] rank job sorts takes ~1.7 s
// here (profiles/r04s_chain_occ_c4_sq.txt) -- the keys themselves are recomputed and sorted by
// every job.
static size_t sq_held_bytes(const ovl_ctx *c) {
  const auto &Q = c->sq;
  return 8 * (Q.key.n + Q.key2.n + Q.dwbase.n) + 4 * (Q.wid.n + Q.wid2.n + Q.ublk.n + Q.uhits.n +
         Q.uflags.n) + Q.tmp.n + sizeof(Unit) * Q.dunits.n;
}
static void sq_release(ovl_ctx *c, bool free_mem) {
  auto &Q = c->sq;
  Q.on = false;
  if (free_mem) {
    Q.key.release(); Q.key2.release(); Q.wid.release(); Q.wid2.release(); Q.ublk.release();
    Q.dwbase.release(); Q.dunits.release(); Q.tmp.release(); Q.uhits.release(); Q.uflags.release();
    Q.sig.release();
  }
  Q.units.clear(); Q.ureadiid.clear(); Q.uwin.clear(); Q.wb.clear(); Q.runs.clear();
  Q.probed = -1;
}

// Windows need only be ordered by the key's top 24 bits (a table slot is its top tab_bits): 3
// radix passes instead of 8.  This ROCm's hipcub / rocPRIM radix sort over a partial bit range
// of 64-bit keys returned duplicated ids and an unsorted order below ~1.4 M items
// (tools/sortcheck.hip: 100 k and 882,524 items wrong for [32|40|48, 64), 1.44 M to 2^27
// right; profiles/r04n_sortcheck.log), so runs under SQ_PART_MIN windows sort all 64 bits, and
// a partially sorted run is checked on both properties that broke (k_sq_sorted_check: key
// order, and the (key, wid) multiset against k_sq_keys' signature) and sorted again over all
// bits if either fails.  OVL_TEST_SQ_CORRUPT=1 (tests) checks every run and duplicates a
// window id in the first run's sorted output, so the fallback path runs.
static const uint64_t SQ_PART_MIN = 1ull << 22;
static const int SQ_PART_LO = 40;
// runs of <= SQ_RUN windows (hipcub sorts index with int)
// 2^29 windows per run: a run's sort needs ~24 B per window beside the 12 B it keeps (the
// configs[4] rank-0 job at 1/8 scale: 3.8 G windows, 58 GB with 2^29-window runs, 71 GB
// with 2^30 -- past half of the ~133 GB free when its second batch starts)
static const uint64_t SQ_RUN = 1ull << 29;

// The job's query units (read order) and their layout in runs
static void sq_units(ovl_ctx *c, uint32_t bgn, uint32_t end, uint32_t lib_lo, uint32_t lib_hi) {
  auto &Q = c->sq;
  query_rule(c, lib_lo, lib_hi).each(bgn, end, [&](uint32_t a, bool, uint64_t w) {
    for (uint32_t dir = 0; w && dir < 2; dir++) {
      Q.units.push_back(Unit{a - c->first_iid, dir});
      Q.ureadiid.push_back(a);
      Q.uwin.push_back(w);
    }
  });
}

// Whether the sorted windows fit: up to half the free HBM (the configs[4] rank-0 job at 1/8
// scale: 3.8 G windows, 67 GB), counting what an earlier job's arrays hold as free.  A driver
// job's query chunks were planned against that rule before its search buffers existed
// (plan_query_chunks); from then on those buffers keep their size (sticky_budgets), so a later
// chunk needs only fit what is free beside them -- under the half rule the full-size
// configs[4] job sorted its first chunk only and probed the other five by random lookups
// (r05g: 120 launches)
static bool sq_fits(ovl_ctx *c, uint64_t total, uint64_t maxrun, size_t fr) {
  auto &Q = c->sq;
  const uint32_t nu = (uint32_t)Q.units.size();
  const uint64_t need = 12ull * total + 24ull * maxrun + 8ull * (maxrun >> 9) + 64ull * nu;
  Q.resorted = 0;
  if (getenv("OVL_TIMING"))
    fprintf(stderr, "OVL_TIMING sorted query windows: %u units, %llu windows in %zu runs, "
            "%.1f GB needed, %.1f GB free\n", nu, (unsigned long long)total, Q.runs.size(),
            need / 1e9, fr / 1e9);
  const uint64_t avail = fr + sq_held_bytes(c);
  if (c->sticky_budgets ? need + (4ull << 30) <= avail : need <= avail / 2) return true;
  sq_release(c);
  c->stats.sq_declined++;
  if (getenv("OVL_TIMING"))
    fprintf(stderr, "OVL_TIMING sorted query windows declined: %.1f GB needed, %.1f GB "
            "available -> random-lookup probes\n", need / 1e9, avail / 1e9);
  return false;
}

// The device arrays, the unit tables uploaded.  *tmpb: the radix sort's scratch bytes;
// *fits false (and the sorted windows released): no room, the random-lookup probe
static int sq_allocate(ovl_ctx *c, uint64_t total, uint64_t maxrun, const std::vector<uint32_t> &ublk,
                       size_t *tmpb, bool *fits) {
  auto &Q = c->sq;
  hipStream_t s = c->stream;
  const uint32_t nu = (uint32_t)Q.units.size();
  size_t t64 = 0;
  HIPC(hipcub::DeviceRadixSort::SortPairs(nullptr, *tmpb, Q.key2.p, Q.key.p, Q.wid2.p, Q.wid.p,
                                          (int)std::min<uint64_t>(maxrun, SQ_RUN), SQ_PART_LO, 64, s));
  HIPC(hipcub::DeviceRadixSort::SortPairs(nullptr, t64, Q.key2.p, Q.key.p, Q.wid2.p, Q.wid.p,
                                          (int)std::min<uint64_t>(maxrun, SQ_RUN), 0, 64, s));
  *tmpb = std::max(*tmpb, t64);
  // a driver job's chunks differ by a few windows: the first one takes the largest chunk's
  // size (ovl_ctx::sq_reserve), or the next would free and reallocate ~57 GB (~1.7 s here)
  if (c->sq_reserve > total && (Q.key.n < c->sq_reserve || Q.wid.n < c->sq_reserve))
    if (Q.key.alloc(c->sq_reserve) || Q.wid.alloc(c->sq_reserve)) { /* exact sizes below */ }
  if (Q.key.alloc(total) || Q.wid.alloc(total) || Q.key2.alloc(maxrun) || Q.wid2.alloc(maxrun) ||
      Q.tmp.alloc(std::max<size_t>(*tmpb, 1)) || Q.dwbase.alloc(Q.wb.size()) ||
      Q.dunits.alloc(nu) || Q.ublk.alloc(std::max<size_t>(ublk.size(), 1)) ||
      Q.uhits.alloc(nu) || Q.uflags.alloc(nu) || Q.sig.alloc(5)) {
    sq_release(c);
    *fits = false;
    return OVL_OK;
  }
  *fits = true;
  HIPC(hipMemcpyAsync(Q.dwbase.p, Q.wb.data(), 8ull * Q.wb.size(), hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(Q.dunits.p, Q.units.data(), sizeof(Unit) * nu, hipMemcpyHostToDevice, s));
  if (!ublk.empty())
    HIPC(hipMemcpyAsync(Q.ublk.p, ublk.data(), 4ull * ublk.size(), hipMemcpyHostToDevice, s));
  return OVL_OK;
}

// A run's keys (k_sq_keys, with their signature) and its sort over bits [bits_lo, 64)
static int sq_sort_run(ovl_ctx *c, const SqRun &R, size_t tmpb, int bits_lo, bool corrupt) {
  auto &Q = c->sq;
  hipStream_t s = c->stream;
  const uint32_t k = c->P.kmer_len;
  SqKeyArgs KA;
  KA.R = c->reads();
  KA.units = Q.dunits.p + R.u0;
  KA.wbase = Q.dwbase.p + R.wb0;
  KA.nunits = R.u1 - R.u0;
  KA.k = k;
  KA.kmask = (1ull << (2 * k)) - 1;
  KA.key = Q.key2.p;
  KA.wid = Q.wid2.p;
  KA.sig = Q.sig.p;
  HIPC(hipMemsetAsync(Q.sig.p, 0, 5 * sizeof(unsigned long long), s));
  hipLaunchKernelGGL(k_sq_keys, dim3((KA.nunits + 3) / 4), dim3(256), 0, s, KA);
  HIPC(hipGetLastError());
  HIPC(hipcub::DeviceRadixSort::SortPairs(Q.tmp.p, tmpb, Q.key2.p, Q.key.p + R.e0, Q.wid2.p,
                                          Q.wid.p + R.e0, (int)R.n, bits_lo, 64, s));
  if (corrupt && R.n >= 2)
    HIPC(hipMemcpyAsync(Q.wid.p + R.e0 + 1, Q.wid.p + R.e0, 4, hipMemcpyDeviceToDevice, s));
  return OVL_OK;
}

// *broken: the sorted run is out of key order over [bits_lo, 64) or not the keys' multiset
static int sq_check_run(ovl_ctx *c, const SqRun &R, int bits_lo, bool *broken) {
  auto &Q = c->sq;
  hipStream_t s = c->stream;
  hipLaunchKernelGGL(k_sq_sorted_check, dim3(4 * c->n_cu), dim3(256), 0, s,
                     (const uint64_t *)(Q.key.p + R.e0), (const uint32_t *)(Q.wid.p + R.e0),
                     R.n, (uint32_t)bits_lo, Q.sig.p, (uint32_t *)(Q.sig.p + 4));
  HIPC(hipGetLastError());
  unsigned long long h[5] = {0, 0, 0, 0, 0};
  HIPC(hipMemcpyAsync(h, Q.sig.p, sizeof(h), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  *broken = (uint32_t)h[4] != 0 || h[0] != h[2] || h[1] != h[3];
  return OVL_OK;
}

// one run sorted: over the top bits when it is long enough, checked, and sorted again over
// every bit when the check fails
static int sq_sort_checked(ovl_ctx *c, const SqRun &R, size_t tmpb, bool test_corrupt, bool corrupt) {
  const int lo = R.n >= SQ_PART_MIN ? SQ_PART_LO : 0;
  if (int rc = sq_sort_run(c, R, tmpb, lo, corrupt)) return rc;
  if (!lo && !test_corrupt) return OVL_OK;
  bool broken = false;
  if (int rc = sq_check_run(c, R, lo, &broken)) return rc;
  if (!broken) return OVL_OK;
  if (int rc = sq_sort_run(c, R, tmpb, 0, false)) return rc;
  if (int rc = sq_check_run(c, R, 0, &broken)) return rc;
  if (broken)
    return fail(OVL_ERR_HIP, "sorted query windows: run of %llu windows failed its check "
                "after a full-range sort", (unsigned long long)R.n);
  c->sq.resorted++;
  return OVL_OK;
}

static int sq_prepare(ovl_ctx *c, uint32_t bgn, uint32_t end, uint32_t lib_lo, uint32_t lib_hi) {
  auto &Q = c->sq;
  if (Q.on && Q.ref_bgn == bgn && Q.ref_end == end && Q.lib_lo == lib_lo && Q.lib_hi == lib_hi)
    return OVL_OK;
  sq_release(c, false);
  sq_units(c, bgn, end, lib_lo, lib_hi);
  if (Q.units.empty()) return OVL_OK;
  SqLayout lay = sq_layout(Q.uwin, SQ_RUN);
  Q.wb.swap(lay.wb);
  Q.runs.swap(lay.runs);
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) return OVL_OK;
  if (!sq_fits(c, lay.total, lay.maxrun, fr)) return OVL_OK;
  const auto t0 = std::chrono::steady_clock::now();
  size_t tmpb = 0;
  bool fits = false;
  if (int rc = sq_allocate(c, lay.total, lay.maxrun, lay.ublk, &tmpb, &fits)) return rc;
  if (!fits) return OVL_OK;
  const bool test_corrupt = getenv("OVL_TEST_SQ_CORRUPT") && atoi(getenv("OVL_TEST_SQ_CORRUPT"));
  for (const auto &R : Q.runs)
    if (int rc = sq_sort_checked(c, R, tmpb, test_corrupt, test_corrupt && &R == &Q.runs[0]))
      return rc;
  c->stats.sq_resorted += Q.resorted;
  HIPC(hipStreamSynchronize(c->stream));
  Q.ms_sort = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (getenv("OVL_TIMING"))
    fprintf(stderr, "OVL_TIMING sorted query windows: sorted in %.1f ms (%u runs sorted again "
            "over all bits)\n", Q.ms_sort, Q.resorted);
  c->stats.ms_seed += Q.ms_sort;
  Q.ref_bgn = bgn; Q.ref_end = end; Q.lib_lo = lib_lo; Q.lib_hi = lib_hi;
  Q.on = true;
  Q.probed = -1;
  return OVL_OK;
}
