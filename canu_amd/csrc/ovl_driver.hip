// ovl_driver.hip -- OverlapDriver (overlapInCore.C:190-300): which index is built and which
// search runs against it.  The decisions from lengths and counts are ovl_plan.h's; DriverJob
// holds one job's plan and runs it.  Part of ovl_api.hip's translation unit.

static const uint64_t MAX_STRING_NUM = (1ull << 31) - 1; // overlapInCore.C:57-63

// Query chunks of an OverlapDriver job whose sorted query windows (sq_prepare) would not fit
// the HBM all at once (configs[4]'s full-size rank jobs: ~28 G windows, 330 GB of keys and
// ids).  The ref range bgn..end is cut into consecutive chunks whose windows fit the budget
// sq_prepare checks against (half the HBM free now and held by sorted windows, less a margin
// for the next builds), counted with sq_prepare's unit rule.  One chunk: the whole range.
// OVL_SQ_CHUNK_WINDOWS (tests) caps a chunk's windows.
static std::vector<IidRange> plan_query_chunks(ovl_ctx *c, uint32_t bgn, uint32_t end,
                                               uint32_t lib_lo, uint32_t lib_hi,
                                               uint64_t *max_windows) {
  size_t fr = 0, tot = 0;
  uint64_t budget = UINT64_MAX;
  if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
    const uint64_t half = (fr + sq_held_bytes(c)) / 2;
    const uint64_t fixed = 24ull * (1ull << 29) + 8ull * (1ull << 20);   // one run's sort scratch
    budget = half > fixed ? (half - fixed) * 9 / 10 : 0;
  }
  uint64_t wcap = budget / 13;                       // 12 B per window + the unit arrays
  if (const char *e = getenv("OVL_SQ_CHUNK_WINDOWS")) wcap = std::min<uint64_t>(wcap, strtoull(e, nullptr, 10));
  wcap = std::max<uint64_t>(wcap, 1);
  return cut_query_chunks(query_rule(c, lib_lo, lib_hi), bgn, end, wcap, max_windows);
}

// One ovl_overlap_driver job: its clamped ranges, the knobs read at its start, and its plan --
// the reference's hash batches, the super-batches they are packed into, the query chunks.
struct DriverJob {
  using clk = std::chrono::steady_clock;
  ovl_ctx *c;
  const ovl_driver_params *d;
  uint32_t bgn_hash = 0, end_hash = 0, bgn_ref = 0, end_ref = 0;
  RefSchedule ref;                 // ref.last: the last searched ref read
  // the query windows sorted once per query chunk (sq_prepare): OVL_SQ=1 always, 0 never,
  // 2 from a job's second search on, 3 (the default) when a query chunk is searched by
  // SQ_AUTO_SEARCHES indexes or more.  The sort costs about one random-lookup probe of the
  // same windows (the configs[4] rank-0 job at 1/8 scale, 14 batches: sort 134 ms, seed 847
  // against 892 ms; profiles/r04y_c4_*.log).
  static const uint64_t SQ_AUTO_SEARCHES = 3;
  int sq_mode = 3;
  int sb_mode = 1;                 // OVL_SUPERBATCH
  uint64_t batches = 0;
  std::vector<IidRange> bat;       // the reference's batches
  std::vector<IidRange> sbs;       // super-batches
  uint64_t sb_cap = 0, sb_max = 0; // their window cap; the largest one's windows
  bool sq_on = false;
  std::vector<IidRange> qchunks;
  std::vector<std::pair<size_t, size_t>> plan;   // (chunk, super-batch) in search order

  static double ms_since(clk::time_point a, clk::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
  }
  void timing_line(const char *what, double build_ms, double find_ms) const {
    if (!getenv("OVL_TIMING")) return;
    fprintf(stderr, "OVL_TIMING %s: wall build %.1f ms, find %.1f ms; device index %.1f seed %.1f "
            "extend %.1f ms, alloc/free %.1f ms (%llu allocs, %.1f GB) so far\n", what, build_ms,
            find_ms, c->stats.ms_index, c->stats.ms_seed, c->stats.ms_extend, g_alloc_ms,
            (unsigned long long)g_alloc_n, g_alloc_bytes / 1e9);
  }

  // argument checks, the clamped ranges, the job's resets
  int begin() {
    if (c->nreads == 0) return fail(OVL_ERR_STATE, "no reads loaded");
    const ovl_hash_limits &L = d->limits;
    if (L.max_hash_strings == 0)                                    // main() :423
      return fail(OVL_ERR_BAD_PARAM, "No memory model supplied; -M needed!");
    if (L.max_hash_strings > MAX_STRING_NUM)                        // :429
      return fail(OVL_ERR_BAD_PARAM, "Too many strings (--hashstrings), must be less than %llu",
                  (unsigned long long)MAX_STRING_NUM);
    HIPC(hipSetDevice(c->device));
    const uint32_t last_loaded = c->first_iid + c->nreads - 1;
    const uint32_t num_reads = d->store_num_reads ? d->store_num_reads : last_loaded;
    bgn_hash = std::max<uint32_t>(d->bgn_hash_iid, 1);                  // :208-212
    end_hash = std::min<uint32_t>(d->end_hash_iid, num_reads);
    bgn_ref = std::max<uint32_t>(d->bgn_ref_iid, 1);                    // :237-241
    end_ref = std::min<uint32_t>(d->end_ref_iid, num_reads);
    // every read the job touches must be loaded
    if ((bgn_hash < end_hash && (bgn_hash < c->first_iid || end_hash > last_loaded)) ||
        (bgn_ref < end_ref && (bgn_ref < c->first_iid || end_ref > last_loaded)))
      return fail(OVL_ERR_BAD_PARAM, "-h %u-%u / -r %u-%u reach past the loaded reads %u-%u",
                  bgn_hash, end_hash, bgn_ref, end_ref, c->first_iid, last_loaded);
    ref = ref_schedule(bgn_ref, end_ref, d->num_threads);
    memset(&c->stats, 0, sizeof(c->stats));
    c->nout = 0;
    c->acc.nu = c->acc.nn = c->acc.np = 0;
    c->cut_windows_hint = 0;
    c->have_index = false;                    // a job builds its own indexes (none is reused)
    if (const char *e = getenv("OVL_SQ")) sq_mode = atoi(e);
    if (const char *e = getenv("OVL_SUPERBATCH")) sb_mode = atoi(e);
    return OVL_OK;
  }

  // The reference's hash-batch loading loop (overlapInCore.C:222): f(bgn, end, t0, t1) after
  // every batch bgn..end, built (or, boundaries_only, only bounded) between t0 and t1
  template <typename F>
  int each_hash_batch(bool boundaries_only, F &&f) {
    const ovl_hash_limits &L = d->limits;
    uint32_t bgn = bgn_hash;
    uint32_t end = bgn_hash + L.max_hash_strings - 1;                    // inclusive
    while (bgn < end_hash) {
      if (end > end_hash) end = end_hash;
      uint32_t loaded = 0;
      const auto t0 = clk::now();
      if (int rc = build_batch_impl(c, bgn, end, &L, &loaded, boundaries_only)) return rc;
      const auto t1 = clk::now();
      end = loaded;
      batches++;
      if (int rc = f(bgn, end, t0, t1)) return rc;
      bgn = end + 1;
      end = bgn + L.max_hash_strings - 1;
    }
    c->stats.hash_batches = batches;
    return OVL_OK;
  }

  // every batch built and searched in turn, as the reference does
  int run_batch_by_batch() {
    int rc = each_hash_batch(false, [&](uint32_t bgn, uint32_t end, clk::time_point t0,
                                        clk::time_point t1) -> int {
      if (ref.any) {
        // the batches' pairs are extended together: the last batch flushes what is pending
        uint64_t n = 0;
        const bool last_batch = !(end + 1 < end_hash);
        c->sq_request = sq_mode == 1 || (sq_mode == 2 && batches >= 2);
        if (int rc = find_impl(c, bgn_ref, ref.last, d->min_lib_ref, d->max_lib_ref, true, &n,
                               last_batch))
          return rc;
      }
      char what[96];
      snprintf(what, sizeof(what), "batch %llu: hash %u-%u", (unsigned long long)batches, bgn, end);
      timing_line(what, ms_since(t0, t1), ms_since(t1, clk::now()));
      return OVL_OK;
    });
    if (rc) return rc;
    c->stats.query_chunks = ref.any ? 1 : 0;
    return OVL_OK;
  }

  // phase 2: super-batches of up to sb_cap windows -- a share of what one index may take
  // (index_window_cap, with this context's current index counted as free), leaving the rest
  // of the HBM to the sorted query windows and the search buffers.  OVL_SB_WINDOWS caps it.
  void pack_super_batches() {
    const HashRule H = hash_rule(c, d->limits.min_lib_hash, d->limits.max_lib_hash);
    uint64_t sb_pct = 55;
    if (const char *e = getenv("OVL_SB_PCT")) sb_pct = std::min<uint64_t>(95, std::max(5, atoi(e)));
    sb_cap = index_window_cap(c) * sb_pct / 100;
    if (const char *e = getenv("OVL_SB_WINDOWS")) sb_cap = std::min<uint64_t>(sb_cap, strtoull(e, nullptr, 10));
    sb_cap = std::max<uint64_t>(sb_cap, 1);
    std::vector<uint64_t> bw;
    for (const auto &b : bat) bw.push_back(hash_windows(H, b.first, b.second));
    SuperBatches S = ovl::pack_super_batches(bat, bw, sb_cap);
    sbs.swap(S.sbs);
    sb_max = S.max_windows;
  }

  int build_super_batch(size_t si) {
    uint32_t hb = sbs[si].first, he = sbs[si].second;
    if (c->have_index && c->hash_bgn_iid == hb && c->hash_end_iid == he) return OVL_OK;
    if (int rc = clip_hash_range(c, hb, he)) return rc;
    return build_with_release(c, hb, he, !c->sq.on || sq_bloom());
  }

  // whether the job sorts its query windows, and with them the dense-tables rule: sorted
  // windows (12 B + unit arrays) past a quarter of the device will need chunks: the full-size
  // configs[4] rank job (13.7 G windows, ~180 GB) does, its 1/8-scale side line (3.8 G,
  // ~50 GB) does not.  OVL_DENSE_TABLES=0|1 overrides.
  void decide_sorted_windows() {
    sq_on = sq_mode == 1 || (sq_mode == 2 && sbs.size() >= 2) ||
            (sq_mode == 3 && searches_of(sbs, bgn_ref) >= SQ_AUTO_SEARCHES);
    if (!sq_on) return;
    uint64_t qw = 0;
    query_rule(c, d->min_lib_ref, d->max_lib_ref)
        .each(bgn_ref, ref.last, [&](uint32_t, bool, uint64_t w) { qw += 2 * w; });
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) c->dense_tables = 13 * qw > tot / 4;
    if (const char *e = getenv("OVL_DENSE_TABLES")) c->dense_tables = atoi(e) != 0;
  }

  // the query chunks (planned with the first super-batch's index resident: what the sorted
  // windows may take) and the order of the searches
  void plan_chunks(double phase1_ms) {
    if (sq_on) qchunks = plan_query_chunks(c, bgn_ref, ref.last, d->min_lib_ref, d->max_lib_ref,
                                           &c->sq_reserve);
    if (qchunks.empty()) qchunks.push_back({bgn_ref, ref.last});
    plan = search_order(qchunks, sbs);
    if (getenv("OVL_TIMING"))
      fprintf(stderr, "OVL_TIMING super-batches: %llu batches (phase 1 %.1f ms) -> %zu super-batches "
              "of <= %llu windows, %zu query chunks over refs %u-%u, %zu searches, sorted windows %s%s\n",
              (unsigned long long)batches, phase1_ms, sbs.size(), (unsigned long long)sb_cap,
              qchunks.size(), bgn_ref, ref.last, plan.size(), sq_on ? "on" : "off", c->dense_tables ? ", dense tables" : "");
  }

  // phase 3: every (query chunk, super-batch) pair whose reads can meet; sb0_ms: the wall time
  // of the first super-batch's build, done before the chunks were planned
  int run_searches(double sb0_ms) {
    c->sq_request = sq_on;
    for (size_t pi = 0; pi < plan.size(); pi++) {
      const auto [qi, si] = plan[pi];
      const auto t0 = clk::now();
      if (int rc = build_super_batch(si)) return rc;
      const auto t1 = clk::now();
      uint64_t n = 0;
      if (int rc = find_impl(c, qchunks[qi].first, qchunks[qi].second, d->min_lib_ref,
                             d->max_lib_ref, true, &n, pi + 1 == plan.size()))
        return rc;
      char what[128];
      snprintf(what, sizeof(what), "query chunk %zu (refs %u-%u) x super-batch %zu (hash %u-%u)", qi,
               qchunks[qi].first, qchunks[qi].second, si, sbs[si].first, sbs[si].second);
      timing_line(what, pi == 0 ? sb0_ms : ms_since(t0, t1), ms_since(t1, clk::now()));
    }
    return OVL_OK;
  }

  // ---- super-batches (the default without -l) -----------------------------------------
  // A query read meets, in every batch it searches, exactly the hashed reads with larger IDs
  // (Find_Overlaps.C:328), and everything Process_String_Olaps reads of a (query, target)
  // pair -- its seed hits in window and chain order, its Add_Match list, the target's
  // screened ends (Mark_Screened_Ends_Chain, Build_Hash_Index.C:147-170: per read), the
  // query's hi_hits flags (skip k-mers are in every batch's table) -- depends on the pair
  // alone.  So searching the UNION of consecutive batches' hashed reads gives every pair,
  // record and -s counter the batches give one by one; only the batches' ends (the table-load
  // cuts, the one-read tail that is never hashed, :222) need the reference's loading loop.
  // Phase 1 runs that loop (Build_Hash_Index's stop rules, build_batch_impl) and records the
  // batches; phase 2 groups consecutive batches into super-batches of up to sb_cap windows;
  // phase 3 searches every (query chunk, super-batch) pair whose reads can meet: a canu job
  // of ~100 batches is then ~10 searches of each query instead of ~100.
  int run_super_batches() {
    const auto t_p1 = clk::now();
    if (int rc = each_hash_batch(true, [&](uint32_t bgn, uint32_t end, clk::time_point,
                                           clk::time_point) -> int {
          bat.push_back({bgn, end});
          return OVL_OK;
        }))
      return rc;
    const double phase1_ms = ms_since(t_p1, clk::now());
    if (bat.empty()) {
      c->stats.query_chunks = 0;
      return OVL_OK;
    }
    pack_super_batches();
    // the index buffers for the largest super-batch from the first build on, and search buffers
    // that keep their first size (ovl_ctx::index_reserve / sticky_budgets), for this job only
    struct Reserve {
      ovl_ctx *c;
      ~Reserve() {
        c->index_reserve = 0; c->sq_reserve = 0; c->sticky_budgets = false; c->dense_tables = false;
      }
    } reserve_guard{c};
    c->index_reserve = sb_max + c->h_skip.size();
    c->sticky_budgets = true;
    decide_sorted_windows();
    const auto t_sb0 = clk::now();
    if (int rc = build_super_batch(0)) return rc;
    const double sb0_ms = ms_since(t_sb0, clk::now());
    plan_chunks(phase1_ms);
    if (int rc = run_searches(sb0_ms)) return rc;
    // ref_reads as the reference counts them: every batch's search over the whole -r range
    uint64_t refs = 0;
    query_rule(c, d->min_lib_ref, d->max_lib_ref)
        .each(bgn_ref, ref.last, [&](uint32_t, bool is_ref, uint64_t) { refs += is_ref; });
    c->stats.ref_reads = batches * refs;
    c->stats.query_chunks = (uint32_t)qchunks.size();
    c->stats.super_batches = (uint32_t)sbs.size();
    return OVL_OK;
  }

  // -l (Frag_Olap_Limit) counts a query's overlaps per Find_Overlaps call, i.e. per hash
  // batch (A_/B_Olaps_For_Frag, Find_Overlaps.C:306), and orders its targets by their first
  // hit in the batch: those jobs search batch by batch, as the reference does.
  int run() {
    const bool ordered = c->P.frag_olap_limit != UINT64_MAX;
    return (!ref.any || ordered || sb_mode == 0) ? run_batch_by_batch() : run_super_batches();
  }
};
