// ovl_ctx.h -- the context behind the C-ABI's ovl_ctx handle, with the error report (fail,
// HIPC) and the timed grow-only device buffer (DBuf) every host file of the library uses.
// Part of ovl_api.hip's translation unit: included there, after the kernels and ovl_plan.h.
#pragma once

static thread_local std::string g_err;

static int fail(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPC(x)                                                                         \
  do {                                                                                  \
    hipError_t _e = (x);                                                                \
    if (_e != hipSuccess)                                                               \
      return fail(OVL_ERR_HIP, "%s:%d %s: %s", __FILE__, __LINE__, #x,                 \
                  hipGetErrorString(_e));                                               \
  } while (0)

// wall time spent in device (re)allocation and frees (OVL_TIMING reports it)
static double g_alloc_ms = 0;
static uint64_t g_alloc_n = 0, g_alloc_bytes = 0;

template <typename T>
struct DBuf {
  T *p = nullptr;
  size_t n = 0;
  ~DBuf() { release(); }
  void release() {
    if (p) {
      const auto t0 = std::chrono::steady_clock::now();
      (void)hipFree(p);
      g_alloc_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    p = nullptr;
    n = 0;
  }
  hipError_t alloc(size_t count) {
    if (count <= n && p) return hipSuccess;
    release();
    size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t e = hipMalloc((void **)&p, bytes);
    g_alloc_n++;
    g_alloc_bytes += bytes;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    g_alloc_ms += ms;
    static const bool trace = getenv("OVL_TIMING") != nullptr;
    if (trace && bytes >= (1ull << 30))
      fprintf(stderr, "OVL_TIMING alloc %.2f GB (%zu x %zu B) %.1f ms%s\n", bytes / 1e9, count,
              sizeof(T), ms, e == hipSuccess ? "" : " FAILED");
    if (e == hipSuccess) n = count;
    else (void)hipGetLastError();                  // an OOM must not surface at a later check
    return e;
  }
  // search working buffers: sizes vary from batch to batch, so a regrow takes 1.5x (each
  // hipMalloc / hipFree of tens of GB costs seconds), or exactly `count` when 1.5x does not fit
  hipError_t grow(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p && alloc(std::max(count, n + n / 2)) == hipSuccess) return hipSuccess;
    return alloc(count);
  }
};

// the maxErate tables' Edit_Match_Limit (prefixEditDistance.C:40-116) is ped_host.h's
using ped::AS_MAX_READLEN;

// ---------------------------------------------------------------------------------------

struct ovl_ctx {
  ovl_params P;
  int device = 0;
  int n_cu = 256;
  hipStream_t stream = nullptr;
  hipEvent_t ev[8];
  // xev[0] / xev[1] bracket an extension launch (find_impl), which runs on `stream` like the
  // probe and the chain: extending chunk i on a second stream beside chunk i+1's probe and
  // chain was tried, measured 4-7 % slower, and removed
  hipEvent_t xev[2];

  // tables
  int32_t max_errors = 0;
  double branch_match_value = 0, min_branch_tail_slope = 0;
  DBuf<int32_t> d_error_bound, d_match_limit;
  std::vector<int32_t> h_error_bound;

  // reads
  uint32_t first_iid = 0, nreads = 0;
  std::vector<uint32_t> h_len;
  std::vector<uint64_t> h_wofs;
  DBuf<uint64_t> d_fwd, d_rc, d_wofs;
  DBuf<uint32_t> d_fwdN, d_rcNul, d_len, d_flags, d_rcFirstNul;
  DBuf<uint8_t> d_qual;          // -w only: read r base i at wofs[r] * 32 + i
  bool have_qual = false;
  uint32_t max_len = 0;

  // skip k-mers (both strands, deduplicated codes)
  std::vector<uint64_t> h_skip;
  DBuf<uint64_t> d_skip;

  // index
  bool have_index = false;
  uint32_t hash_bgn_iid = 0, hash_end_iid = 0;
  DBuf<uint64_t> d_occ, d_tmpM2;
  DBuf<Rec2> d_tmpR, d_midR;     // build scratch: coarse- and fine-bucketed records
  // the build's bucket bookkeeping (coarse histogram and starts, fine starts and counts, a
  // few counters, the big-bucket list): kept too -- the driver's load cuts build the index
  // twice per hash batch, and a hipMalloc / hipFree pair per array per build added up
  DBuf<uint32_t> b_hist, b_cstart, b_cursor, b_fstart, b_fcnt, b_misc, b_big;
  DBuf<uint32_t> b_first;        // the driver's first-read histogram (load cuts)
  uint64_t cut_windows_hint = 0; // windows of the job's last load-cut batch (0: none yet)
  DBuf<TabEntry> d_tab;
  uint32_t tab_bits = 0, slice_bits = 0;
  DBuf<uint64_t> d_bloom;        // the batch's Bloom filter (driver batches: k_table)
  bool bloom_ok = false;
  uint32_t bloom_w = 0;

  // find_overlaps working buffers: kept across calls (grow-only), hipMalloc of tens of
  // GB per call would cost seconds
  struct {
    DBuf<Unit> units;
    DBuf<uint64_t> rbase;
    DBuf<Probe> probe;
    DBuf<uint32_t> uhits, uflags, ctr, done, dset, big, defer, defer2, okey, oidx, okey2, oidx2;
    DBuf<uint32_t> live;          // the chain's units with at least one hit
    DBuf<uint32_t> xctr, xnout;
    DBuf<unsigned long long> chits;
    DBuf<uint8_t> otmp;
    DBuf<uint64_t> ok64a, ok64b, dkey;       // -l orders
    DBuf<uint64_t> hcnt, hbase;              // ovl_seed_hits: per-unit hit counts / bases
    DBuf<uint4> hbuf;                        // ovl_seed_hits: one piece of the hit list
    DBuf<uint32_t> oa, ob, ucnt, useg;
    DBuf<Node> pool, pnodes;
    DBuf<PairRec> pairs;
    DBuf<unsigned long long> stats;
    DBuf<int32_t> rows, rowdir, deltas;
  } fb;

  // library IDs (-H / -R filters); empty = every read in library 0
  std::vector<uint32_t> h_lib;
  bool nohash_set = false;       // some read carries OVL_RFLAG_NOHASH
  uint32_t stats_hash_lib_lo = 0, stats_hash_lib_hi = UINT32_MAX;   // -H of the index
  uint64_t index_records = 0;    // records of the current index (windows + skip markers)
  // an OverlapDriver job's phase 3 (ovl_overlap_driver): the index buffers are allocated for
  // the largest super-batch at once, and the search buffers keep the size the first search
  // gave them -- a hipFree / hipMalloc of tens of GB on a nearly full device costs ~0.5 s
  uint64_t index_reserve = 0, sq_reserve = 0;
  bool sticky_budgets = false;
  // an OverlapDriver job whose sorted query windows need several chunks: tables at half the
  // slots (slices 1x the largest fine bucket's distinct k-mers instead of 2x), so that more
  // of the HBM holds query windows (fewer chunks, fewer super-batch rebuilds and probes)
  bool dense_tables = false;

  // pending extension work (see find_impl): chains of several probe chunks -- and of the
  // driver's hash batches -- are appended here and extended together in one launch
  struct {
    DBuf<Unit> units;
    DBuf<Node> pnodes;
    DBuf<PairRec> pairs;
    uint64_t nu = 0, nn = 0, np = 0;
  } acc;

  // OverlapDriver jobs: the query windows sorted by k-mer once per job (k_sq_keys,
  // k_probe_sorted in ovl_seed.hip; sq_prepare in ovl_sq.hip).  sq_request: the driver asks
  // find_impl to use them from its second hash batch on (OVL_SQ=0 never, =1 from the first).
  bool sq_request = false;
  struct {
    bool on = false;
    uint32_t ref_bgn = 0, ref_end = 0, lib_lo = 0, lib_hi = 0, hash_lo = 0;
    std::vector<Unit> units;     // the job's query units, read order
    std::vector<uint32_t> ureadiid;
    std::vector<uint64_t> uwin;  // windows per unit
    std::vector<uint64_t> wb;    // per unit + one per run: run-local first window (as dwbase)
    std::vector<SqRun> runs;     // ovl_plan.h sq_layout
    DBuf<uint64_t> key, key2;
    DBuf<uint32_t> wid, wid2, ublk;
    DBuf<uint64_t> dwbase;
    DBuf<Unit> dunits;
    DBuf<uint8_t> tmp;
    DBuf<uint32_t> uhits, uflags;
    DBuf<unsigned long long> sig;   // a run's (key, wid) signatures before / after its sort + flag
    uint32_t resorted = 0;       // runs whose partial-range sort failed its check
    int probed = -1;             // the run whose records fb.probe holds for this batch
    uint32_t probed_nu = 0;      // ... for this many of its units
    double ms_sort = 0;
  } sq;

  // results
  DBuf<Rec> d_out;
  uint64_t nout = 0;
  ovl_stats stats;
  DBuf<unsigned long long> dbg;  // OVL_DEBUG counters of this context's extension kernels

  ReadsDev reads() const {
    ReadsDev R;
    R.fwd = d_fwd.p;
    R.rc = d_rc.p;
    R.fwdN = d_fwdN.p;
    R.rcNul = d_rcNul.p;
    R.wofs = d_wofs.p;
    R.len = d_len.p;
    R.flags = d_flags.p;
    R.rcFirstNul = d_rcFirstNul.p;
    R.qual = have_qual ? d_qual.p : nullptr;
    R.first_iid = first_iid;
    R.nreads = nreads;
    return R;
  }
};

// the query reads of the loaded reads' libraries [lib_lo, lib_hi] (every library by default)
static QueryRule query_rule(const ovl_ctx *c, uint32_t lib_lo = 0, uint32_t lib_hi = UINT32_MAX) {
  QueryRule Q;
  Q.len = c->h_len.data();
  Q.lib = c->h_lib.empty() ? nullptr : c->h_lib.data();
  Q.first_iid = c->first_iid;
  Q.min_olap_len = c->P.min_olap_len;
  Q.k = c->P.kmer_len;
  Q.lib_lo = lib_lo;
  Q.lib_hi = lib_hi;
  return Q;
}
// the hash reads of the loaded reads' libraries [lib_lo, lib_hi] (-H)
static HashRule hash_rule(const ovl_ctx *c, uint32_t lib_lo, uint32_t lib_hi) {
  HashRule H;
  static_cast<QueryRule &>(H) = query_rule(c, lib_lo, lib_hi);
  return H;
}
