// ovl_find.hip -- one search of ref reads against the current index, host side: the
// extension's launch plan (ExtPlan), the probe batch, FindRun's steps and find_impl, with the
// small kernels that order and append pairs between them.  Part of ovl_api.hip's translation
// unit.

extern "C" {   // these kernels' names are unmangled (the profiles key on them)

// Work-order keys for the extension queue: a pair's match-node count (its extension work
// grows with it), so the longest pairs start first and the kernel's tail is short.
__global__ void k_pair_order_keys(const PairRec *pairs, uint32_t n, uint32_t *keys,
                                  uint32_t *idx) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    keys[i] = pairs[i].node_cnt;
    idx[i] = i;
  }
}

// ---- -l (Frag_Olap_Limit): the reference's per-unit pair orders -----------------------
// Process_String_Olaps (Process_String_Overlaps.C:687) walks a query's targets in
// String_Olap_Space order -- Add_Ref (Find_Overlaps.C:158) gives a new target its hash
// slot (StrNum ^ StrNum >> 8) & 255 when that slot is free, else the next overflow entry
// (256, 257, .. in first-hit order) -- and, past the limit, sorted by average diagonal
// (qsort By_Diag_Sum, glibc's stable merge sort: ties keep String_Olap_Space order).
// A target's first hit is its smallest window (diag_bgn); targets first hit in the same
// window come in the occurrence list's order, iid-descending.

// per pair: first-hit keys, the unit's pair count, and the average diagonal (the
// reference sums diagonals in a double: exact for integers, so the sum over nodes is the
// same number; each node of length Len holds Len - k + 1 hits on its diagonal)
__global__ void k_olim_keys(const PairRec *pairs, const Node *pnodes, uint32_t n, int32_t k,
                            uint32_t *ktgt, uint64_t *kfirst, uint32_t *idx, uint64_t *dkey,
                            uint32_t *ucnt) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const PairRec P = pairs[i];
    ktgt[i] = ~P.tgt;
    kfirst[i] = ((uint64_t)P.unit << 24) | (uint32_t)P.diag_bgn;
    idx[i] = i;
    int64_t sum = 0;
    for (uint32_t j = 0; j < P.node_cnt; j++) {
      const Node nd = pnodes[P.node_off + j];
      sum += (int64_t)(nd.Len - k + 1) * (int64_t)(nd.Offset - nd.Start);
    }
    const double avg = (double)sum / (double)P.diag_ct;
    const uint64_t b = __builtin_bit_cast(uint64_t, avg);
    dkey[i] = (b >> 63) ? ~b : (b | (1ull << 63));     // order-preserving
    atomicAdd(&ucnt[P.unit], 1u);
  }
}

__global__ void k_gather_u64(const uint64_t *src, const uint32_t *idx, uint32_t n, uint64_t *dst) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    dst[i] = src[idx[i]];
}

// A chunk's pairs appended to the pending-extension accumulator: their unit and node indices
// move by where the chunk's units and nodes land there.
__global__ void k_append_pairs(const PairRec *src, uint32_t n, uint32_t unit_base,
                               uint32_t node_base, PairRec *dst) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    PairRec p = src[i];
    p.unit += unit_base;
    p.node_off += node_base;
    dst[i] = p;
  }
}

__global__ void k_gather_unit(const PairRec *pairs, const uint32_t *idx, uint32_t n, uint32_t *dst) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    dst[i] = pairs[idx[i]].unit;
}

// One wave per unit over its pairs in first-hit order: String_Olap_Space index per pair,
// written as the sort key unit << 32 | index (ks) next to the pair index (ki).
__global__ void __launch_bounds__(256) k_olim_slots(const PairRec *pairs, const uint32_t *first,
                                                    const uint32_t *useg, uint32_t nunits,
                                                    uint32_t str_off, uint64_t *ks, uint32_t *ki) {
  __shared__ uint32_t s_first[4][256];
  __shared__ uint8_t s_taken[4][256];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t *fst = s_first[wave];
  uint8_t *taken = s_taken[wave];
  for (uint32_t i = lane; i < 256; i += 64) { fst[i] = 64; taken[i] = 0; }
  __builtin_amdgcn_wave_barrier();
  for (uint32_t u = blockIdx.x * 4 + wave; u < nunits; u += gridDim.x * 4) {
    const uint32_t b = useg[u], e = useg[u + 1];
    uint32_t novf = 0;
    for (uint32_t c0 = b; c0 < e; c0 += 64) {
      const uint32_t i = c0 + lane;
      const bool valid = i < e;
      uint32_t pi = 0, h = 0;
      if (valid) {
        pi = first[i];
        const uint32_t sn = pairs[pi].tgt + str_off;   // StrNum: index in the hash batch
        h = (sn ^ (sn >> 8)) & 255u;
        atomicMin(&fst[h], lane);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const bool own = valid && fst[h] == lane && !taken[h];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (valid) fst[h] = 64;
      if (own) taken[h] = 1;
      const uint64_t om = __ballot(valid && !own);
      const uint32_t slot = own ? h : 256u + novf + (uint32_t)__builtin_popcountll(om & ((1ull << lane) - 1));
      novf += (uint32_t)__builtin_popcountll(om);
      if (valid) {
        ks[i] = ((uint64_t)u << 32) | slot;
        ki[i] = pi;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    for (uint32_t i = lane; i < 256; i += 64) taken[i] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

}  // extern "C"

static IndexDev index_dev(const ovl_ctx *c) {
  IndexDev X;
  X.tab = c->d_tab.p;
  X.occ = c->d_occ.p;
  X.tab_bits = c->tab_bits;
  X.slice_bits = c->slice_bits;
  X.k = c->P.kmer_len;
  X.kmask = (1ull << (2 * c->P.kmer_len)) - 1;
  X.bloom = nullptr;
  X.bloom_w = 0;
  return X;
}

// Whether a search of ref reads bgn..end should probe through the Bloom filter: when at
// least 3/4 of them lie outside the hash range (OverlapDriver's later batches, probed by
// every earlier query), most of their windows miss the table.  OVL_BLOOM=0/1 forces it.
static bool use_bloom(const ovl_ctx *c, uint32_t bgn, uint32_t end) {
  if (!c->bloom_ok) return false;                 // only driver batches build one
  if (const char *e = getenv("OVL_BLOOM")) return atoi(e) != 0;
  if (end < bgn) return false;
  const uint64_t q = (uint64_t)end - bgn + 1;
  const uint32_t lo = std::max(bgn, c->hash_bgn_iid), hi = std::min(end, c->hash_end_iid);
  const uint64_t inside = hi >= lo ? (uint64_t)hi - lo + 1 : 0;
  return 4 * (q - inside) >= 3 * q;
}

// ---- the extension's launch plan ---------------------------------------------------------
// Pairs go through up to three launches: the staged kernel at full occupancy (8 waves per
// <= 64 KB block) for pairs whose reads are both <= len1, the staged kernel with more LDS
// per wave for reads <= len2, and the generic kernel for the rest (reads with an 'n',
// bands wider than the register window, longer reads).  Each launch's scratch and LDS are
// sized for its own length class, so one long read in a job does not shrink the others.
struct ExtClass {
  uint32_t len = 0, wpb = 1, waves = 0;
  int32_t ecap = 0, sw = 0;
  size_t lds = 0;
  bool l16 = false;              // staged: 16-bit row log; generic: rows in global memory (GR)
  uint64_t stride = 0;
  bool wide = false;             // the 2 x OVL_RJ-chunk register window (wide bands)
  uint64_t per_wave_bytes() const { return stride * 4 + 16ull * (ecap + 2) + 28ull * (ecap + 8); }
};
struct ExtPlan {
  std::vector<ExtClass> stage;   // the staged launches in order; the wide class, if any, last
  ExtClass gen;                  // the generic kernel: every read length
  uint64_t rows_n = 0, rowdir_n = 0, deltas_n = 0;   // the scratch that fits every launch
};

// the k_extend instance of a launch: its address serves the attribute call, the occupancy
// query and hipLaunchKernel
static const void *extend_instance(bool staged, bool l16, bool ordered, bool wide) {
#define OVL_KX(...) reinterpret_cast<const void *>(k_extend<__VA_ARGS__>)
  if (staged && wide) return l16 ? OVL_KX(true, true, false, 2 * OVL_RJ) : OVL_KX(true, false, false, 2 * OVL_RJ);
  if (staged) return l16 ? OVL_KX(true, true) : OVL_KX(true, false);
  if (!ordered) return l16 ? OVL_KX(false, true) : OVL_KX(false, false);
  return l16 ? OVL_KX(false, true, true) : OVL_KX(false, false, true);
#undef OVL_KX
}
static int launch_extend(const ExtClass &g, bool staged, bool ordered, ExtendArgs &EA, hipStream_t s) {
  void *args[] = {&EA};
  HIPC(hipLaunchKernel(extend_instance(staged, g.l16, ordered, g.wide), dim3(g.waves / g.wpb),
                       dim3(64 * g.wpb), args, g.lds, s));
  return OVL_OK;
}

static int32_t ecap_of(const ovl_ctx *c, uint64_t L) {
  return c->h_error_bound[std::min<uint64_t>(L, AS_MAX_READLEN)] + 2;
}
static int32_t sw_of(uint64_t L) { return (int32_t)(((L + 31) / 32 + 2) & ~1ull); }
// per wave: the two strands' plane words, the scratch and the pair-state block
static uint64_t stg_lds_of(uint64_t L) {
  return 4ull * (4ull * (uint64_t)sw_of(L) + OVL_SCR_STAGE + OVL_STATE_INTS);
}
// a block's Edit_Match_Limit table
static uint64_t ml_of(int32_t ec) { return 4ull * (((uint64_t)(ec + 2) + 3) & ~3ull); }
// the longest read whose staged block of wpb waves fits cap bytes of LDS
static uint32_t longest_fitting(const ovl_ctx *c, uint32_t wpb, size_t cap) {
  auto fits = [&](uint64_t L) { return stg_lds_of(L) * wpb + ml_of(ecap_of(c, L)) <= cap; };
  uint64_t lo = 0, hi = c->max_len;
  if (fits(hi)) return (uint32_t)hi;
  while (lo + 1 < hi) {
    const uint64_t mid = (lo + hi) / 2;
    if (fits(mid)) lo = mid; else hi = mid;
  }
  return (uint32_t)lo;
}
// the staged class of reads <= L within cap bytes of LDS per block
static int make_stage(const ovl_ctx *c, bool window, uint32_t L, size_t cap, bool allow_knob,
                      bool wide, ExtClass *out) {
  ExtClass g;
  g.len = L;
  g.wide = wide;
  g.ecap = ecap_of(c, L);
  g.sw = sw_of(L);
  g.l16 = L < 16384;
  g.wpb = (uint32_t)std::min<uint64_t>(8, (cap - std::min<uint64_t>(cap, ml_of(g.ecap))) / stg_lds_of(L));
  if (g.wpb < 1) return -1;
  g.lds = stg_lds_of(L) * g.wpb + ml_of(g.ecap);
  // experiment knob: OVL_EXT_BLOCKS_PER_CU pads the LDS so that at most that many blocks
  // fit on a CU (occupancy studies); unset = natural occupancy
  if (allow_knob)
    if (const char *bp = getenv("OVL_EXT_BLOCKS_PER_CU")) {
      int nb = atoi(bp);
      if (nb > 0) g.lds = std::max<size_t>(g.lds, (160 * 1024) / nb - 256);
    }
  const uint64_t lw = wide ? std::max<uint64_t>(OVL_LOGW, 128 * OVL_RJ) : OVL_LOGW;
  uint64_t st = (uint64_t)(g.ecap + 2) * lw / (g.l16 ? 2 : 1);   // the row log
  if (window) st = std::max<uint64_t>(st, 3ull * (g.ecap + 9) + 2ull * L + 64);
  g.stride = (st + 63) & ~63ull;
  const void *kfn = extend_instance(true, g.l16, false, wide);
  if (g.lds > 64 * 1024)
    if (hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds) != hipSuccess)
      return -1;
  // persistent grid: as many blocks as are resident at once (registers and LDS), so no
  // block starts only after the work queue has drained; within the scratch budget
  const uint64_t SCRATCH_BUDGET = 24ull << 30;
  uint32_t waves = 4u * OVL_EXT_OCC * c->n_cu;
  int bpc = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, kfn, 64 * g.wpb, g.lds) == hipSuccess &&
      bpc > 0)
    waves = std::min<uint32_t>(waves, (uint32_t)bpc * g.wpb * c->n_cu);
  while (waves > g.wpb && (uint64_t)waves * g.per_wave_bytes() > SCRATCH_BUDGET) waves /= 2;
  g.waves = std::max<uint32_t>(g.wpb, (waves / g.wpb) * g.wpb);
  *out = g;
  return 0;
}

static int plan_extension(const ovl_ctx *c, bool window, bool ordered, ExtPlan *out) {
  ExtPlan X;
  // occupancy tiers of the staged kernel: 3 blocks of 8 waves per CU (the register limit),
  // 3 blocks of 6, then blocks of up to 8 waves within 160 KB (as many as fit a CU).  A
  // class's length is the span it stages (k_extend stages a pair's overlap span, not its
  // whole reads): the tier's limit, or the longest loaded read when that is shorter, so a
  // short-read job's launch is exactly what it was and a long-read job's pairs with shorter
  // spans run at the higher occupancy.
  uint32_t prev = 0;
  const size_t tier_cap[3] = {52 * 1024, 52 * 1024, 160 * 1024};
  const uint32_t tier_wpb[3] = {8, 6, 1};
  ExtClass g;
  for (int t = 0; t < 3; t++) {
    const uint32_t T = longest_fitting(c, tier_wpb[t], tier_cap[t]);
    const uint32_t L = std::min<uint32_t>(T, c->max_len);
    if (L < 64 || L <= prev) continue;
    if (make_stage(c, window, L, tier_cap[t], t == 0, false, &g))
      return fail(OVL_ERR_HIP, "staged kernel setup");
    X.stage.push_back(g);
    prev = L;
  }
  // the wide class: the pairs of every staged class whose band outgrew the register window
  // (the rest of their deferrals -- 'n' bases -- pass on to the generic kernel)
  if (!X.stage.empty() && !getenv("OVL_NO_WIDE")) {
    if (make_stage(c, window, X.stage.back().len, 160 * 1024, false, true, &g))
      return fail(OVL_ERR_HIP, "wide staged kernel setup");
    X.stage.push_back(g);
  }
  // the generic kernel: every read length; rows in LDS while two row buffers and the
  // Edit_Match_Limit table fit a CU, else in global memory (GR)
  ExtClass &gen = X.gen;
  gen.len = c->max_len;
  gen.ecap = ecap_of(c, c->max_len);
  const size_t ml = ml_of(gen.ecap);
  size_t w = 4ull * ((2ull * (2 * gen.ecap + 8) + TB_ROWS * TB_W + OVL_LDCAP + OVL_STATE_INTS + 3) & ~3ull);
  gen.l16 = w + ml > 160 * 1024;                       // GR
  if (gen.l16) w = 4ull * ((TB_ROWS * TB_W + OVL_LDCAP + OVL_STATE_INTS + 3) & ~3ull);
  gen.wpb = (4 * w <= 80 * 1024) ? 4 : (2 * w <= 80 * 1024) ? 2 : 1;
  gen.lds = w * gen.wpb + (gen.l16 ? 0 : ml);
  uint64_t st = (uint64_t)(gen.ecap + 2) * (gen.ecap + 2) + 4ull * (gen.ecap + 2) + 64;
  if (window) st = std::max<uint64_t>(st, 3ull * (gen.ecap + 9) + 2ull * c->max_len + 64);
  // a wave's band-compact row log holds every row of one extension (quadratic in the
  // error limit); past 2^28 ints the GR kernel checks its cursor and fails loudly
  if (gen.l16) st = std::min<uint64_t>(st, 1ull << 28);
  gen.stride = (st + 63) & ~63ull;
  uint32_t waves = 24u * c->n_cu;
  while (waves > gen.wpb && (uint64_t)waves * gen.per_wave_bytes() > (16ull << 30)) waves /= 2;
  gen.waves = std::max<uint32_t>(gen.wpb, (waves / gen.wpb) * gen.wpb);
  if (gen.lds > 64 * 1024)
    HIPC(hipFuncSetAttribute(extend_instance(false, gen.l16, ordered, false),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)gen.lds));
  X.rows_n = gen.stride * gen.waves;
  X.rowdir_n = 4ull * (gen.ecap + 2) * gen.waves;
  X.deltas_n = 7ull * (gen.ecap + 8) * gen.waves;
  for (const ExtClass &s : X.stage) {
    X.rows_n = std::max<uint64_t>(X.rows_n, s.stride * s.waves);
    X.rowdir_n = std::max<uint64_t>(X.rowdir_n, 4ull * (s.ecap + 2) * s.waves);
    X.deltas_n = std::max<uint64_t>(X.deltas_n, 7ull * (s.ecap + 8) * s.waves);
  }
  *out = X;
  return OVL_OK;
}

// One random-lookup probe batch: nb units and their window bases (windows uwin[0..nb)) uploaded
// to fb.units / fb.rbase, k_probe launched on the context's stream after event ev[2] -- not
// waited for.  OVL_ERR_OOM, nothing launched: the buffers do not fit.
static int probe_batch(ovl_ctx *c, const Unit *units, const uint64_t *uwin, uint32_t nb,
                       bool bloom, std::vector<uint64_t> *rbase) {
  auto &fb = c->fb;
  hipStream_t s = c->stream;
  rbase->resize(nb + 1);
  uint64_t acc = 0;
  for (uint32_t i = 0; i < nb; i++) { (*rbase)[i] = acc; acc += uwin[i]; }
  (*rbase)[nb] = acc;
  if (fb.units.grow(nb) || fb.rbase.grow(nb + 1) || fb.probe.grow(acc) || fb.uhits.grow(nb) ||
      fb.uflags.grow(nb))
    return fail(OVL_ERR_OOM, "probe buffers");
  HIPC(hipMemcpyAsync(fb.units.p, units, sizeof(Unit) * nb, hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(fb.rbase.p, rbase->data(), 8ull * (nb + 1), hipMemcpyHostToDevice, s));
  ProbeArgs PA;
  PA.R = c->reads();
  PA.X = index_dev(c);
  if (bloom) {
    PA.X.bloom = c->d_bloom.p;
    PA.X.bloom_w = c->bloom_w;
  }
  PA.units = fb.units.p;
  PA.rbase = fb.rbase.p;
  PA.nunits = nb;
  PA.out = fb.probe.p;
  PA.unit_hits = fb.uhits.p;
  PA.unit_flags = fb.uflags.p;
  PA.k = c->P.kmer_len;
  HIPC(hipEventRecord(c->ev[2], s));
  if (bloom) hipLaunchKernelGGL(k_probe<true>, dim3((nb + 3) / 4), dim3(256), 0, s, PA);
  else       hipLaunchKernelGGL(k_probe<false>, dim3((nb + 3) / 4), dim3(256), 0, s, PA);
  HIPC(hipGetLastError());
  return OVL_OK;
}

// ---- one search (find_impl) and its steps ------------------------------------------------
// One probed batch of query units: what the chain needs of it.
struct ProbedBatch {
  uint32_t nb = 0;                 // units, uploaded to fb.units
  std::vector<uint64_t> rbase;     // nb + 1 window bases within fb.probe, uploaded to fb.rbase
  std::vector<uint32_t> uh;        // the units' seed hits
  uint32_t *uflags = nullptr;      // device: the units' flags
};

// the accumulator's flush thresholds (see FindRun::acc_append); FindRun::acc_pairs is the
// pairs' one, this its default
static const uint64_t ACC_PAIRS = 4ull << 20, ACC_NODES = 1ull << 30;
// per staged class: its work-queue cursor and its defer count in the extension's counters
static const uint32_t ctr_next[4] = {5, 11, 13, 15}, ctr_defer[4] = {8, 12, 14, 10};

struct FindRun {
  ovl_ctx *c;
  hipStream_t s;
  uint32_t k;
  bool ordered;                    // -l: every pair through the ordered generic kernel
  bool window;                     // -w
  // A batch is sized by seed hits (node pool + list-ordered copy: 32 B per hit); the probe
  // window budget adapts to the hits-per-window ratio seen so far (plan_chain)
  uint64_t hit_budget = 0, win_budget = 512ull << 20, win_cap = 1536ull << 20;
  uint64_t win_floor = WIN_FLOOR;  // the window budget does not adapt or halve below this
  uint64_t per_unit = 256;         // pairs per unit the chain first allows
  uint64_t acc_pairs = ACC_PAIRS;  // the accumulator is extended once it holds this many pairs
  uint64_t out_first = 0;          // test knob: the output buffer's first room (0: the default)
  uint32_t alloc_fails = 0;        // test knob: chain-buffer allocations still to count as failed
  bool fake_oom = false;           // ... and whether that knob is set at all
  uint32_t chain_waves = 0;
  ExtPlan ext;
  uint64_t nout_ub = 0;            // records: an upper bound (<= 3 per pair) of the device counter
  bool pending = false;            // an extension launched and not yet collected
  uint32_t pending_pairs = 0;

  // The hit budget, the counters, the extension plan and its scratch, the output buffer.
  int begin(size_t nunits) {
    auto &fb = c->fb;
    // seed hits per batch; halved while the chain buffers do not fit the HBM the index
    // leaves, as the probe-slot cap is for the probe records
    // 3.5 G: the 50k x 10 kb job in 2 chunks (1.27 s per step) rather than 4 (1.29 s) or 8
    // (1.34 s) -- fewer re-probed windows and extension tails; node indices stay < 2^32
    hit_budget = 3584ull << 20;
    // within the HBM left beside the index: the node pool and its list-ordered copy take
    // ~33 B per hit; keep them under 60 % of what is free now plus what they already hold
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
      const uint64_t held = (fb.pool.n + fb.pnodes.n) * sizeof(Node);
      hit_budget = std::min<uint64_t>(hit_budget, (uint64_t)((fr + held) * 0.6) / 33);
    }
    // a driver job's later searches chain within the buffers its first one sized (more hit
    // chunks per run instead of a regrow of the pool and its copy)
    if (c->sticky_budgets && fb.pnodes.n > (16ull << 20))
      hit_budget = std::min<uint64_t>(hit_budget, fb.pnodes.n - 1);
    if (const char *e = getenv("OVL_HIT_BUDGET_M"))             // experiments: millions of hits
      hit_budget = std::max<uint64_t>(16, strtoull(e, nullptr, 10)) << 20;
    hit_budget = std::max<uint64_t>(hit_budget, 16ull << 20);
    if (const char *e = getenv("OVL_TEST_PAIRS_PER_UNIT"))      // test knob: force the regrow path
      per_unit = std::max(1, atoi(e));
    // test knobs: budgets far below the floors above, so that a job of a few hundred reads
    // takes several probe batches, chain chunks, accumulator flushes and output regrows
    // (tests/test_gpu_search_seams.py)
    auto knob = [](const char *name, uint64_t *v) {
      const char *e = getenv(name);
      if (e) *v = std::max<uint64_t>(1, strtoull(e, nullptr, 10));
      return e != nullptr;
    };
    knob("OVL_TEST_HIT_BUDGET", &hit_budget);                   // hits, no floor
    if (knob("OVL_TEST_WIN_BUDGET", &win_budget)) {             // windows, no floor
      win_cap = win_budget;
      win_floor = 1;
    }
    knob("OVL_TEST_ACC_PAIRS", &acc_pairs);                     // the flush threshold
    knob("OVL_TEST_OUT_RECORDS", &out_first);                   // records of room at the start
    if (const char *e = getenv("OVL_TEST_CHAIN_ALLOC_FAILS")) { // force the halve-and-replan path
      fake_oom = true;
      alloc_fails = (uint32_t)std::max(0, atoi(e));
    }
    chain_waves = 4u * OVL_CHAIN_OCC * c->n_cu;   // OVL_CHAIN_OCC blocks of 4 waves per CU
    if (fb.ctr.alloc(16) || fb.stats.alloc(16) || fb.xctr.alloc(16) || fb.xnout.alloc(1))
      return fail(OVL_ERR_OOM, "counters");
    HIPC(hipMemsetAsync(fb.stats.p, 0, 128, s));
    if (int rc = plan_extension(c, window, ordered, &ext)) return rc;
    if (fb.rows.alloc(ext.rows_n) || fb.rowdir.alloc(ext.rowdir_n) || fb.deltas.alloc(ext.deltas_n))
      return fail(OVL_ERR_OOM, "extension scratch");
    // records: the device counter xnout continues from the records already held (the
    // driver's earlier hash batches)
    uint32_t nout32 = (uint32_t)c->nout;
    HIPC(hipMemcpyAsync(fb.xnout.p, &nout32, 4, hipMemcpyHostToDevice, s));
    HIPC(hipStreamSynchronize(s));
    nout_ub = c->nout;
    if (out_first) return ensure_out(c->nout + out_first);
    return ensure_out(std::max<uint64_t>(c->nout + (1u << 20), c->nout + nunits * 8));
  }

  int ensure_out(uint64_t need) {
    if (need <= c->d_out.n && c->d_out.p) return OVL_OK;
    HIPC(hipStreamSynchronize(s));
    uint32_t cur = 0;
    HIPC(hipMemcpy(&cur, c->fb.xnout.p, 4, hipMemcpyDeviceToHost));
    DBuf<Rec> bigger;
    if (bigger.alloc(need + (need >> 2))) return fail(OVL_ERR_OOM, "output grow");
    if (cur) {
      HIPC(hipMemcpyAsync(bigger.p, c->d_out.p, sizeof(Rec) * cur, hipMemcpyDeviceToDevice, s));
      c->stats.out_regrows++;
    }
    HIPC(hipStreamSynchronize(s));
    std::swap(bigger.p, c->d_out.p);
    std::swap(bigger.n, c->d_out.n);
    return OVL_OK;
  }

  // The launched extension has finished: its counters, class split and time.
  int collect_extension() {
    if (!pending) return OVL_OK;
    pending = false;
    HIPC(hipEventSynchronize(c->xev[1]));
    uint32_t hx[16];
    HIPC(hipMemcpy(hx, c->fb.xctr.p, 64, hipMemcpyDeviceToHost));
    float t = 0;
    (void)hipEventElapsedTime(&t, c->xev[0], c->xev[1]);
    c->stats.ms_extend += t;
    if (hx[7] & 32u)
      return fail(OVL_ERR_UNSUPPORTED, "an extension needs more than 2^28 row cells (error limit "
                  "%d of a %u-base read): past the generic kernel's per-wave row log",
                  ecap_of(c, c->max_len), c->max_len);
    if (hx[7]) return fail(OVL_ERR_HIP, "extension capacity exceeded (flags %u)", hx[7]);
    uint32_t left = pending_pairs;
    for (size_t ci = 0; ci < ext.stage.size() && !ordered; ci++) {
      const uint32_t nd = hx[ctr_defer[ci]];
      if (getenv("OVL_DEBUG"))
        fprintf(stderr, "OVL_DEBUG class %zu (reads <= %u): deferred %u of %u pairs\n", ci,
                ext.stage[ci].len, nd, left);
      if (ci == 0) c->stats.staged_pairs += left - nd;
      else c->stats.long_pairs += left - nd;
      left = nd;
    }
    c->stats.generic_pairs += left;
    return OVL_OK;
  }

  // -l: the reference's two pair orders per unit (see k_olim_keys), String_Olap_Space order and
  // By_Diag_Sum order, by stable radix sorts
  int order_pairs_olim(const PairRec *pairs, const Node *pnodes, uint32_t npairs,
                                uint32_t nc, ExtendArgs *EA) {
    auto &fb = c->fb;
    const int n = (int)npairs;
    size_t t1 = 0, t2 = 0, t3 = 0;
    HIPC(hipcub::DeviceRadixSort::SortPairs(nullptr, t1, fb.okey.p, fb.okey2.p, fb.oa.p,
                                            fb.ob.p, n, 0, 32, s));
    HIPC(hipcub::DeviceRadixSort::SortPairs(nullptr, t2, fb.ok64a.p, fb.ok64b.p, fb.oa.p,
                                            fb.ob.p, n, 0, 64, s));
    HIPC(hipcub::DeviceScan::ExclusiveSum(nullptr, t3, fb.ucnt.p, fb.useg.p, (int)nc + 1, s));
    const size_t tmp = std::max(std::max(t1, t2), t3);
    HIPC(hipStreamSynchronize(s));
    if (fb.okey.grow(npairs) || fb.okey2.grow(npairs) || fb.oa.grow(npairs) ||
        fb.ob.grow(npairs) || fb.oidx.grow(npairs) || fb.oidx2.grow(npairs) ||
        fb.ok64a.grow(npairs) || fb.ok64b.grow(npairs) || fb.dkey.grow(npairs) ||
        fb.ucnt.grow((size_t)nc + 1) || fb.useg.grow((size_t)nc + 1) ||
        fb.otmp.grow(std::max<size_t>(tmp, 1)))
      return fail(OVL_ERR_OOM, "-l pair orders");
    const dim3 grid(std::min<uint32_t>((npairs + 255) / 256, 4096)), blk(256);
    HIPC(hipMemsetAsync(fb.ucnt.p, 0, 4ull * (nc + 1), s));
    // first-hit order: by ~tgt, then (stably) by (unit, diag_bgn)
    hipLaunchKernelGGL(k_olim_keys, grid, blk, 0, s, pairs, pnodes, npairs, (int32_t)k,
                       fb.okey.p, fb.ok64a.p, fb.oa.p, fb.dkey.p, fb.ucnt.p);
    HIPC(hipGetLastError());
    HIPC(hipcub::DeviceScan::ExclusiveSum(fb.otmp.p, t3, fb.ucnt.p, fb.useg.p, (int)nc + 1, s));
    size_t tt = t1;
    HIPC(hipcub::DeviceRadixSort::SortPairs(fb.otmp.p, tt, fb.okey.p, fb.okey2.p, fb.oa.p,
                                            fb.ob.p, n, 0, 32, s));
    hipLaunchKernelGGL(k_gather_u64, grid, blk, 0, s, fb.ok64a.p, fb.ob.p, npairs, fb.ok64b.p);
    tt = t2;
    HIPC(hipcub::DeviceRadixSort::SortPairs(fb.otmp.p, tt, fb.ok64b.p, fb.ok64a.p, fb.ob.p,
                                            fb.oa.p, n, 0, 64, s));
    // String_Olap_Space indices, then the order by (unit, index)
    hipLaunchKernelGGL(k_olim_slots, dim3(std::min<uint32_t>((nc + 3) / 4, 8192)), blk, 0, s,
                       pairs, fb.oa.p, fb.useg.p, nc,
                       c->first_iid - c->hash_bgn_iid, fb.ok64b.p, fb.ob.p);
    HIPC(hipGetLastError());
    tt = t2;
    HIPC(hipcub::DeviceRadixSort::SortPairs(fb.otmp.p, tt, fb.ok64b.p, fb.ok64a.p, fb.ob.p,
                                            fb.oidx.p, n, 0, 64, s));       // oidx: ord_slot
    // By_Diag_Sum: stably by the diagonal key, then stably by unit
    hipLaunchKernelGGL(k_gather_u64, grid, blk, 0, s, fb.dkey.p, fb.oidx.p, npairs, fb.ok64a.p);
    tt = t2;
    HIPC(hipcub::DeviceRadixSort::SortPairs(fb.otmp.p, tt, fb.ok64a.p, fb.ok64b.p, fb.oidx.p,
                                            fb.oa.p, n, 0, 64, s));
    hipLaunchKernelGGL(k_gather_unit, grid, blk, 0, s, pairs, fb.oa.p, npairs, fb.okey.p);
    tt = t1;
    HIPC(hipcub::DeviceRadixSort::SortPairs(fb.otmp.p, tt, fb.okey.p, fb.okey2.p, fb.oa.p,
                                            fb.oidx2.p, n, 0, 32, s));      // oidx2: ord_diag
    HIPC(hipGetLastError());
    EA->useg = fb.useg.p;
    EA->ord_slot = fb.oidx.p;
    EA->ord_diag = fb.oidx2.p;
    EA->dkey = fb.dkey.p;
    return OVL_OK;
  }

  // longest-first work order (node count descending; ties keep pair order), and the defer lists
  int order_pairs_longest_first(const PairRec *pairs, uint32_t npairs, ExtendArgs *EA) {
    auto &fb = c->fb;
    size_t tmp = 0;
    HIPC(hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tmp, fb.okey.p, fb.okey2.p,
                                                      fb.oidx.p, fb.oidx2.p, (int)npairs, 0,
                                                      32, s));
    if (fb.okey.n < npairs || fb.oidx.n < npairs || fb.okey2.n < npairs || fb.oidx2.n < npairs ||
        fb.defer.n < npairs || fb.defer2.n < npairs || fb.otmp.n < tmp || !fb.otmp.p) {
      HIPC(hipStreamSynchronize(s));
      if (fb.okey.grow(npairs) || fb.oidx.grow(npairs) || fb.okey2.grow(npairs) ||
          fb.oidx2.grow(npairs) || fb.defer.grow(npairs) || fb.defer2.grow(npairs) ||
          fb.otmp.grow(std::max<size_t>(tmp, 1)))
        return fail(OVL_ERR_OOM, "work order");
    }
    if (npairs > 1) {
      hipLaunchKernelGGL(k_pair_order_keys, dim3(std::min<uint32_t>((npairs + 255) / 256, 4096)),
                         dim3(256), 0, s, pairs, npairs, fb.okey.p, fb.oidx.p);
      HIPC(hipGetLastError());
      HIPC(hipcub::DeviceRadixSort::SortPairsDescending(fb.otmp.p, tmp, fb.okey.p, fb.okey2.p,
                                                        fb.oidx.p, fb.oidx2.p, (int)npairs, 0,
                                                        32, s));
      EA->list = fb.oidx2.p;
    }
    return OVL_OK;
  }

  // One chunk's (or the accumulator's) pairs through the extension kernels, the host not waiting
  // for the last one: work order, the staged classes, the generic kernel; collect_extension()
  // reads its counters back.
  int launch_extension(const Unit *units, PairRec *pairs, Node *pnodes, uint32_t npairs,
                                uint32_t nc) {
    auto &fb = c->fb;
    uint32_t *x_ctr = fb.xctr.p;
    nout_ub += 3ull * npairs;
    if (int rc = ensure_out(nout_ub)) return rc;
    ExtendArgs EA = {};              // every field not set here is 0 / null
    EA.R = c->reads();
    EA.units = units;
    EA.pairs = pairs;
    EA.npairs = npairs;
    EA.pnodes = pnodes;
    EA.pair_next = x_ctr + 5;
    EA.error_bound = c->d_error_bound.p;
    EA.match_limit = c->d_match_limit.p;
    EA.max_errors = c->max_errors;
    EA.branch_match_value = c->branch_match_value;
    EA.min_branch_tail_slope = c->min_branch_tail_slope;
    EA.min_branch_end_dist = 20;
    EA.partial = c->P.partial;
    EA.unique = c->P.unique_olap_per_pair;
    EA.min_olap_len = c->P.min_olap_len;
    EA.use_hopeless = c->P.use_hopeless_check;
    EA.k = (int32_t)k;
    EA.filter_by_kmer_count = c->P.filter_by_kmer_count;
    EA.minkmer_exp = exp(-1.0 * (double)k * c->P.max_erate);
    EA.rows = fb.rows.p;
    EA.rowdir = fb.rowdir.p;
    EA.deltas = fb.deltas.p;
    EA.out = c->d_out.p;
    EA.nout = fb.xnout.p;
    EA.out_cap = (uint32_t)std::min<uint64_t>(c->d_out.n, 0xFFFFFFF0ull);
    EA.stats = fb.stats.p;
    EA.window = window ? 1 : 0;
    EA.overflow = x_ctr + 7;
    if (getenv("OVL_DEBUG")) {
      if (!c->dbg.p) {
        HIPC(hipStreamSynchronize(s));
        if (c->dbg.alloc(32)) return fail(OVL_ERR_OOM, "debug counters");
        HIPC(hipMemsetAsync(c->dbg.p, 0, 256, s));
      }
      EA.dbg = c->dbg.p;
    }
    EA.olim = c->P.frag_olap_limit;
    EA.nunits = nc;
    pending_pairs = npairs;
    HIPC(hipMemsetAsync(x_ctr, 0, 64, s));
    if (npairs && ordered)
      if (int rc = order_pairs_olim(pairs, pnodes, npairs, nc, &EA)) return rc;
    if (npairs && !ordered)
      if (int rc = order_pairs_longest_first(pairs, npairs, &EA)) return rc;
    HIPC(hipEventRecord(c->xev[0], s));
    // the generic kernel's arguments
    auto generic_args = [](ExtendArgs &A, const ExtClass &gen, uint32_t *ctr) {
      A.e_cap = gen.ecap;
      A.rows_cap = gen.stride;
      A.sw_words = 0;
      A.pair_next = ctr + 9;
      A.defer = nullptr;
      A.ndefer = nullptr;
    };
    // the host reads a class's defer count before the next launch: a launch whose input list is
    // empty is skipped (the bench job's one staged launch then is the extension's only launch)
    auto deferred = [&](size_t ci, uint32_t *nd) -> int {
      HIPC(hipMemcpyAsync(nd, x_ctr + ctr_defer[ci], 4, hipMemcpyDeviceToHost, s));
      HIPC(hipStreamSynchronize(s));
      return OVL_OK;
    };
    if (npairs && ordered) {
      generic_args(EA, ext.gen, x_ctr);
      c->stats.extend_launches++;
      if (int rc = launch_extend(ext.gen, false, true, EA, s)) return rc;
    } else if (npairs) {
      // the staged classes in turn, each deferring what it cannot take to the next list
      // (whose length the next launch reads from the device counter); the generic kernel
      // takes the last list, or every pair when no class exists
      uint32_t *defer_buf[2] = {fb.defer.p, fb.defer2.p};
      uint32_t nd = 1;                   // pairs the previous class left
      for (size_t ci = 0; ci < ext.stage.size(); ci++) {
        const ExtClass &g = ext.stage[ci];
        EA.e_cap = g.ecap;
        EA.rows_cap = g.stride;
        EA.sw_words = g.sw;
        EA.pair_next = x_ctr + ctr_next[ci];
        EA.defer = defer_buf[ci & 1];
        EA.ndefer = x_ctr + ctr_defer[ci];
        if (ci > 0)
          if (int rc = deferred(ci - 1, &nd)) return rc;
        if (nd) {                        // an empty class defers nothing: its counter stays 0
          c->stats.extend_launches++;
          if (int rc = launch_extend(g, true, false, EA, s)) return rc;
        }
        EA.list = defer_buf[ci & 1];
        EA.npairs_dev = x_ctr + ctr_defer[ci];
        EA.restore = 1;          // a deferred pair may have had nodes removed (~Len)
      }
      generic_args(EA, ext.gen, x_ctr);
      if (!ext.stage.empty())
        if (int rc = deferred(ext.stage.size() - 1, &nd)) return rc;
      if (nd) {
        c->stats.extend_launches++;
        if (int rc = launch_extend(ext.gen, false, false, EA, s)) return rc;
      }
    }
    HIPC(hipEventRecord(c->xev[1], s));
    pending = true;
    return OVL_OK;
  }

  // Extend everything the accumulator holds; it is empty again for the next chunk (the
  // stream orders the next appends after this launch's reads).
  int flush_acc() {
    if (int rc = collect_extension()) return rc;
    auto &A = c->acc;
    if (A.np) c->stats.acc_flushes++;
    int rc = launch_extension(A.units.p, A.pairs.p, A.pnodes.p, (uint32_t)A.np, (uint32_t)A.nu);
    A.nu = A.nn = A.np = 0;
    return rc;
  }

  // Append a chunk's units, list nodes and pairs to the accumulator (device copies on the
  // stream the extension also runs on: nothing is overwritten early).
  int acc_append(const Unit *u, uint32_t nu_c, const Node *nodes, uint64_t nn_c,
                          const PairRec *pairs, uint32_t np_c) {
    auto &A = c->acc;
    if (A.nu + nu_c >= 0xFFFFFFF0ull || A.nn + nn_c >= 0xFFFFFFF0ull)
      return fail(OVL_ERR_UNSUPPORTED, "extension accumulator past 2^32 entries");
    auto acc_fits = [&]() {
      return A.units.n >= A.nu + nu_c && A.pnodes.n >= A.nn + nn_c && A.pairs.n >= A.np + np_c;
    };
    // once it holds a launch's worth (a quarter of the flush thresholds), what the
    // accumulator holds is extended rather than moved into bigger buffers: a regrow on a full
    // device costs ~1 s (the full-size configs[4] job, r05e), while smaller launches lose to
    // their tails (one launch per search: extension 8.4 -> 23 s, r05f)
    if (!acc_fits() && (A.np >= std::max<uint64_t>(1, acc_pairs / 4) || A.nn >= ACC_NODES / 4))
      if (int rc = flush_acc()) return rc;
    if (!acc_fits()) {
      // growing moves the buffers: the pending extension (which reads them) must be done,
      // and what the accumulator holds is carried over
      HIPC(hipStreamSynchronize(s));
      // a buffer moved into one of at least `need` entries, its first `used` kept
      auto regrow = [](auto &buf, uint64_t used, uint64_t need) -> int {
        if (buf.n >= need && buf.p) return OVL_OK;
        typename std::remove_reference<decltype(buf)>::type bigger;
        if (bigger.alloc(std::max<uint64_t>(need, buf.n + buf.n / 2))) return -1;
        if (used) HIPC(hipMemcpy(bigger.p, buf.p, used * sizeof(*buf.p), hipMemcpyDeviceToDevice));
        std::swap(bigger.p, buf.p);
        std::swap(bigger.n, buf.n);
        return OVL_OK;
      };
      if (regrow(A.units, A.nu, A.nu + nu_c) || regrow(A.pnodes, A.nn, A.nn + nn_c) ||
          regrow(A.pairs, A.np, A.np + np_c)) {
        // no room for bigger buffers beside the ones being copied (a device nearly full of
        // sorted windows, index and search buffers): what the accumulator holds is extended
        // now, and the emptied buffers are freed before this chunk's own are allocated
        if (A.nu || A.nn || A.np) {
          if (int rc = flush_acc()) return rc;
          HIPC(hipStreamSynchronize(s));
        }
        if ((A.units.n < nu_c && A.units.alloc(nu_c)) ||
            (A.pnodes.n < nn_c && A.pnodes.alloc(nn_c)) || (A.pairs.n < np_c && A.pairs.alloc(np_c)))
          return fail(OVL_ERR_OOM, "extension accumulator (%llu nodes)", (unsigned long long)nn_c);
      }
    }
    if (nu_c)
      HIPC(hipMemcpyAsync(A.units.p + A.nu, u, sizeof(Unit) * nu_c, hipMemcpyDeviceToDevice, s));
    if (nn_c)
      HIPC(hipMemcpyAsync(A.pnodes.p + A.nn, nodes, sizeof(Node) * nn_c, hipMemcpyDeviceToDevice, s));
    if (np_c) {
      hipLaunchKernelGGL(k_append_pairs, dim3(std::min<uint32_t>((np_c + 255) / 256, 4096)),
                         dim3(256), 0, s, pairs, np_c, (uint32_t)A.nu, (uint32_t)A.nn,
                         A.pairs.p + A.np);
      HIPC(hipGetLastError());
    }
    A.nu += nu_c;
    A.nn += nn_c;
    A.np += np_c;
    return OVL_OK;
  }

  // The units from u0 on that fit the window budget, probed by random lookups.
  int probe_lookup(const std::vector<Unit> &units, const std::vector<uint64_t> &uwin,
                            uint32_t u0, bool bloom, ProbedBatch *B) {
    for (;;) {
      B->nb = take_within(uwin, u0, (uint32_t)units.size(), win_budget) - u0;
      const int rc = probe_batch(c, units.data() + u0, uwin.data() + u0, B->nb, bloom, &B->rbase);
      if (rc == OVL_OK) break;
      if (rc != OVL_ERR_OOM || B->nb == 1 || win_budget <= win_floor) return rc;
      win_cap = win_budget = win_budget / 2;
    }
    const uint32_t nb = B->nb;
    c->stats.probe_launches++;
    HIPC(hipEventRecord(c->ev[3], s));
    B->uh.resize(nb);
    HIPC(hipMemcpyAsync(B->uh.data(), c->fb.uhits.p, 4ull * nb, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    float t = 0;
    (void)hipEventElapsedTime(&t, c->ev[2], c->ev[3]);
    c->stats.ms_seed += t;
    c->stats.ms_probe_kernel += t;
    const uint64_t nwin = B->rbase[nb];
    if (getenv("OVL_TIMING"))
      fprintf(stderr, "OVL_TIMING probe launch: %u units, %llu windows, %.3f ms\n", nb,
              (unsigned long long)nwin, t);
    // algorithmic bytes: per window one 16-B table entry and one 8-B Probe record, plus the
    // packed query (2 bits per base); see DESIGN.md
    c->stats.probe_bytes += nwin * 24 + nwin / 4;
    B->uflags = c->fb.uflags.p;
    return OVL_OK;
  }

  // The run of sorted windows holding unit u0: probed once per batch (k_probe_sorted), its
  // records then chained in hit-budget chunks.  *sq_run: the run; *run_uh: its units' hits.
  int probe_sorted_run(const std::vector<Unit> &units, uint32_t u0, size_t *sq_run,
                                std::vector<uint32_t> *run_uh, ProbedBatch *B) {
    auto &fb = c->fb;
    auto &Q = c->sq;
    const uint32_t nu = (uint32_t)units.size();
    while (Q.runs[*sq_run].u1 <= u0) (*sq_run)++;
    const auto &R = Q.runs[*sq_run];
    const uint32_t ue = std::min<uint32_t>(R.u1, nu);
    if (Q.probed != (int)*sq_run) {
      const uint64_t wlim = Q.wb[R.wb0 + (ue - R.u0)];
      if (fb.probe.grow(R.n)) return fail(OVL_ERR_OOM, "probe records (%llu)", (unsigned long long)R.n);
      HIPC(hipEventRecord(c->ev[4], s));           // the probe step: seed-phase time
      HIPC(hipMemsetAsync(fb.probe.p, 0, 8ull * wlim, s));
      HIPC(hipMemsetAsync(Q.uflags.p + R.u0, 0, 4ull * (ue - R.u0), s));
      HIPC(hipMemsetAsync(Q.uhits.p + R.u0, 0, 4ull * (ue - R.u0), s));
      SqProbeArgs SA;
      SA.X = index_dev(c);
      if (c->bloom_ok && sq_bloom()) {        // the filter in front of the table
        SA.X.bloom = c->d_bloom.p;
        SA.X.bloom_w = c->bloom_w;
      }
      SA.R = c->reads();
      SA.key = Q.key.p + R.e0;
      SA.wid = Q.wid.p + R.e0;
      SA.n = R.n;
      SA.wlim = (uint32_t)wlim;
      SA.units = Q.dunits.p + R.u0;
      SA.wbase = Q.dwbase.p + R.wb0;
      SA.ublk = Q.ublk.p + R.ub0;
      SA.k = k;
      SA.out = fb.probe.p;
      SA.unit_flags = Q.uflags.p + R.u0;
      SA.unit_hits = Q.uhits.p + R.u0;
      // the kernel alone is timed (the records' zeroing and the unit hit counts around it
      // are not the probe's bytes)
      HIPC(hipEventRecord(c->ev[2], s));
      hipLaunchKernelGGL(k_probe_sorted, dim3(8 * c->n_cu), dim3(256), 0, s, SA);
      HIPC(hipEventRecord(c->ev[3], s));
      c->stats.probe_launches++;
      c->stats.probe_sorted_launches++;
      HIPC(hipGetLastError());
      HIPC(hipEventRecord(c->ev[5], s));
      run_uh->resize(ue - R.u0);
      HIPC(hipMemcpyAsync(run_uh->data(), Q.uhits.p + R.u0, 4ull * (ue - R.u0),
                          hipMemcpyDeviceToHost, s));
      HIPC(hipStreamSynchronize(s));
      float t = 0, tstep = 0;
      (void)hipEventElapsedTime(&t, c->ev[2], c->ev[3]);
      (void)hipEventElapsedTime(&tstep, c->ev[4], c->ev[5]);
      c->stats.ms_probe_kernel += t;
      c->stats.ms_seed += std::max(t, tstep);          // beside the kernel: the records' zeroing
      // algorithmic bytes: the sorted windows (8-B key + 4-B id), and the table and its
      // filter read once each -- or, when they are larger than the run (a full-size
      // configs[4] super-batch's 68.7 GB table against a run of 2^29 windows), at most one
      // entry and one filter word per window (the hits' 8-B records are not counted)
      const uint64_t tab_b = 16ull << c->tab_bits;
      const uint64_t flt_b = SA.X.bloom ? 8ull * ((1ull << (c->tab_bits - c->slice_bits)) << c->bloom_w) : 0ull;
      c->stats.probe_bytes += 12ull * R.n + std::min<uint64_t>(tab_b, 16ull * R.n) +
                              std::min<uint64_t>(flt_b, 8ull * R.n);
      Q.probed = (int)*sq_run;
    }
    const uint32_t nb = B->nb = ue - u0;
    B->rbase.assign(Q.wb.begin() + R.wb0 + (u0 - R.u0), Q.wb.begin() + R.wb0 + (ue - R.u0) + 1);
    B->uh.assign(run_uh->begin() + (u0 - R.u0), run_uh->begin() + (ue - R.u0));
    B->uflags = Q.uflags.p + u0;
    if (fb.units.grow(nb) || fb.rbase.grow(nb + 1)) return fail(OVL_ERR_OOM, "unit buffers");
    HIPC(hipMemcpyAsync(fb.units.p, units.data() + u0, sizeof(Unit) * nb, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(fb.rbase.p, B->rbase.data(), 8ull * (nb + 1), hipMemcpyHostToDevice, s));
    return OVL_OK;
  }

  // Chaining.  The batch is cut to the hit budget (plan_chain); *nc units are chained.  The first
  // launch chains every unit whose targets fit one pass of the 128-target table and lists the
  // others; the second chains the listed units over several passes with a done set sized for
  // their targets.  Capacities come from the probe's hit counts; a batch that still overflows
  // one (the counters say by how much) is chained again with bigger buffers -- never dropped.
  int chain_batch(const ProbedBatch &B, uint32_t *nc, uint32_t *npairs, uint32_t *nnodes) {
    auto &fb = c->fb;
    const uint32_t hash_reads = c->hash_end_iid - c->hash_bgn_iid + 1;
    auto plan = [&]() {
      return plan_chain(B.uh.data(), B.nb, B.rbase.data(), hit_budget, per_unit, chain_waves,
                        OVL_NODE_BLOCK, win_cap, win_floor);
    };
    // OVL_TEST_CHAIN_ALLOC_FAILS: the first evaluations count as failed whatever the grows said
    // (what they allocated is dropped below, as after a real failure)
    auto grow_failed = [&](bool failed) {
      if (!alloc_fails) return failed;
      alloc_fails--;
      return true;
    };
    ChainPlan P = plan();
    bool planned = true;               // P is new: its live list is not uploaded yet
    uint32_t hc[16];
    for (int attempt = 0;; attempt++) {
      if (P.pool_cap >= 0xFFFFFFF0ull || P.pairs_cap >= 0xFFFFFFF0ull || P.pnodes_cap >= 0xFFFFFFF0ull)
        return fail(OVL_ERR_UNSUPPORTED, "chain buffers past 2^32 entries (%llu hits)",
                    (unsigned long long)P.hsum);
      // sized for the hit budget, not this batch's hits: the next batch reuses them as they are
      if (grow_failed(fb.pool.grow(std::max(P.pool_cap, chain_pool_for(hit_budget, chain_waves, OVL_NODE_BLOCK))) ||
                      fb.pnodes.grow(std::max<uint64_t>(P.pnodes_cap, hit_budget + 1)) ||
                      fb.pairs.grow(P.pairs_cap) || fb.big.grow(P.nc) || fb.chits.grow(1))) {
        if (P.nc == 1 || P.hsum <= (fake_oom ? 1 : 16ull << 20))
          return fail(OVL_ERR_OOM, "chain buffers (%llu hits)", (unsigned long long)P.hsum);
        c->stats.budget_halvings++;
        hit_budget = P.hsum / 2;                         // fewer units per chain launch
        // the buffers that did fit were sized for the larger budget: drop them too
        fb.pool.release();
        fb.pnodes.release();
        fb.pairs.release();
        P = plan();
        planned = true;
        attempt--;
        continue;
      }
      if (planned && !P.all_live() && !P.live.empty()) {
        if (fb.live.grow(P.live.size())) return fail(OVL_ERR_OOM, "unit list");
        HIPC(hipMemcpyAsync(fb.live.p, P.live.data(), 4ull * P.live.size(), hipMemcpyHostToDevice, s));
      }
      planned = false;
      uint32_t ctr_init[16] = {0};
      ctr_init[1] = 1;                                 // pool_next: node 0 is null
      HIPC(hipMemcpyAsync(fb.ctr.p, ctr_init, 64, hipMemcpyHostToDevice, s));
      HIPC(hipMemsetAsync(fb.chits.p, 0, 8, s));
      ChainArgs CA = {};             // no done set, no profile counters
      CA.R = c->reads();
      CA.occ = c->d_occ.p;
      CA.units = fb.units.p;
      CA.rbase = fb.rbase.p;
      CA.probes = fb.probe.p;
      CA.unit_flags = B.uflags;
      CA.nunits = P.all_live() ? P.nc : (uint32_t)P.live.size();
      CA.k = k;
      CA.unit_next = fb.ctr.p + 0;
      CA.pool = fb.pool.p;
      CA.pool_next = fb.ctr.p + 1;
      CA.pool_cap = (uint32_t)P.pool_cap;
      CA.pnodes = fb.pnodes.p;
      CA.pnodes_next = fb.ctr.p + 2;
      CA.pnodes_cap = (uint32_t)P.pnodes_cap;
      CA.pairs = fb.pairs.p;
      CA.npairs = fb.ctr.p + 3;
      CA.pairs_cap = (uint32_t)P.pairs_cap;
      CA.overflow = fb.ctr.p + 4;
      CA.unit_list = P.all_live() ? nullptr : fb.live.p;
      CA.big_units = fb.big.p;
      CA.n_big = fb.ctr.p + 10;
      CA.seed_hits = fb.chits.p;
#ifdef OVL_CHAIN_PROF
      if (!c->dbg.p) {
        if (c->dbg.alloc(32)) return fail(OVL_ERR_OOM, "debug counters");
        HIPC(hipMemsetAsync(c->dbg.p, 0, 256, s));
      }
      CA.prof = c->dbg.p + 24;
#endif
      HIPC(hipEventRecord(c->ev[4], s));
      hipLaunchKernelGGL(k_chain, dim3(chain_waves / 4), dim3(256), 0, s, CA);
      HIPC(hipGetLastError());
      HIPC(hipMemcpyAsync(hc, fb.ctr.p, 64, hipMemcpyDeviceToHost, s));
      HIPC(hipStreamSynchronize(s));
      const uint32_t n_big = hc[10];
      if (n_big && !hc[4]) {
        std::vector<uint32_t> big(n_big);
        HIPC(hipMemcpy(big.data(), fb.big.p, 4ull * n_big, hipMemcpyDeviceToHost));
        uint32_t cap = 1;                              // distinct targets of any listed unit
        for (uint32_t b : big) cap = std::max<uint32_t>(cap, std::min<uint32_t>(B.uh[b], hash_reads));
        uint32_t smask = 1;
        while (smask + 1 < 2ull * cap) smask = 2 * smask + 1;
        uint32_t w2 = std::min<uint32_t>(chain_waves, (n_big + 3) & ~3u);
        while (w2 > 4 && (uint64_t)w2 * (cap + smask + 1) * 4 > (4ull << 30)) w2 = (w2 / 2 + 3) & ~3u;
        if (fb.done.grow((size_t)w2 * cap) || fb.dset.grow((size_t)w2 * (smask + 1)))
          return fail(OVL_ERR_OOM, "done sets (%u targets x %u waves)", cap, w2);
        HIPC(hipMemsetAsync(fb.dset.p, 0, 4ull * w2 * (smask + 1), s));
        HIPC(hipMemsetAsync(fb.ctr.p, 0, 4, s));      // unit_next
        CA.unit_list = fb.big.p;
        CA.nunits = n_big;
        CA.big_units = nullptr;
        CA.n_big = nullptr;
        CA.done_slots = fb.done.p;
        CA.done_set = fb.dset.p;
        CA.done_cap = cap;
        CA.set_mask = smask;
        hipLaunchKernelGGL(k_chain, dim3(w2 / 4), dim3(256), 0, s, CA);
        HIPC(hipGetLastError());
        HIPC(hipMemcpyAsync(hc, fb.ctr.p, 64, hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        c->stats.multi_pass_units += n_big;
      }
      HIPC(hipEventRecord(c->ev[5], s));
      HIPC(hipStreamSynchronize(s));
      if (!hc[4]) break;
      if ((hc[4] & 4u) || attempt >= 3)
        return fail(OVL_ERR_HIP, "chain capacity still exceeded after %d attempts (flags %u)",
                    attempt + 1, hc[4]);
      // grow what overflowed from what the counters asked for, then chain the batch again
      if (hc[4] & 1u) P.pool_cap = (uint64_t)hc[1] + (uint64_t)(chain_waves + 2) * OVL_NODE_BLOCK;
      if (hc[4] & 2u) {
        P.pairs_cap = std::max<uint64_t>(P.pairs_cap, (uint64_t)hc[3] + 1024);
        P.pnodes_cap = std::max<uint64_t>(P.pnodes_cap, (uint64_t)hc[2] + 1024);
      }
      c->stats.chain_retries++;
    }
    win_budget = P.win_budget;
    c->stats.chain_launches++;
    float t = 0;
    (void)hipEventElapsedTime(&t, c->ev[4], c->ev[5]);
    c->stats.ms_seed += t;
    unsigned long long h = 0;
    HIPC(hipMemcpy(&h, fb.chits.p, 8, hipMemcpyDeviceToHost));
    c->stats.seed_hits += h;
    c->stats.pairs += hc[3];
    c->stats.seed_nodes += hc[2];                        // pnodes_next: the lists' nodes
    *nc = P.nc;
    *npairs = hc[3];
    *nnodes = hc[2];
    return OVL_OK;
  }

  // The extension kernels' device counters and the launch plan's figures into the context's
  // ovl_stats (the steps add their own as they go).  Counters add up over the driver's hash
  // batches (the reference sums its per-thread counters into globals, Process_Overlaps.C:156-163).
  int add_stats() {
    unsigned long long hs[16];
    HIPC(hipMemcpy(hs, c->fb.stats.p, 128, hipMemcpyDeviceToHost));
#ifdef OVL_CHAIN_PROF
    if (c->dbg.p) {
      unsigned long long cp[8];
      (void)hipMemcpy(cp, c->dbg.p + 24, 64, hipMemcpyDeviceToHost);
      const double tot = (double)(cp[0] + cp[1] + cp[2] + cp[3] + cp[4] + cp[5]) + 1e-9;
      fprintf(stderr, "OVL_CHAIN_PROF wave-cycles (cumulative): probe+qualify %.3f stage %.3f "
              "discover %.3f scatter %.3f replay %.3f emit %.3f (shares); %llu chunks, %llu "
              "staged occurrences, %.0f cycles per chunk\n", cp[0] / tot, cp[1] / tot,
              cp[2] / tot, cp[3] / tot, cp[4] / tot, cp[5] / tot, cp[6], cp[7],
              tot / (double)(cp[6] ? cp[6] : 1));
    }
#endif
    if (c->dbg.p) {
      unsigned long long dd[32];
      (void)hipMemcpy(dd, c->dbg.p, 256, hipMemcpyDeviceToHost);
      fprintf(stderr, "OVL_DEBUG cyc_A=%llu cyc_B=%llu cyc_cont=%llu cyc_C=%llu cyc_argmax=%llu "
              "cyc_remove=%llu nodes=%llu\n", dd[16], dd[17], dd[18], dd[19], dd[20], dd[21],
              dd[22]);
      fprintf(stderr, "OVL_DEBUG ped=%llu rows=%llu chunks=%llu slide_iters=%llu tb=%llu iters=%llu "
              "cyc_chunks=%llu cyc_tb=%llu pairs=%llu maxrows=%llu cyc_rest=%llu cyc_ped=%llu "
              "cyc_calls=%llu cyc_pair=%llu cyc_stage=%llu cyc_extend=%llu\n",
              dd[0], dd[1], dd[2], dd[3], dd[4], dd[5], dd[6], dd[7], dd[8], dd[9], dd[10], dd[11],
              dd[12], dd[13], dd[14], dd[15]);
    }
    ovl_stats &S = c->stats;
    S.kmer_hits_without_olap += hs[0];
    S.kmer_hits_with_olap += hs[1];
    S.kmer_hits_skipped += hs[2];
    S.multi_overlaps += hs[3];
    S.total_overlaps += hs[4];
    S.contained_overlaps += hs[5];
    S.dovetail_overlaps += hs[6];
    S.bad_short_window += hs[8];
    S.bad_long_window += hs[9];
    // the read-length cap of the first staged launch, and of the last when there are several
    // (the wide class, always last, shares its predecessor's)
    const size_t ns = ext.stage.size() - (!ext.stage.empty() && ext.stage.back().wide);
    S.ext_waves = ns ? ext.stage[0].waves : 0;
    S.generic_waves = ext.gen.waves;
    S.stage_len = ns ? ext.stage[0].len : 0;
    S.long_stage_len = ns > 1 ? ext.stage[ns - 1].len : 0;
    return OVL_OK;
  }
};

// Process_Overlaps (overlapInCore-Process_Overlaps.C:101-137) over ref reads bgn..end of
// libraries [lib_lo, lib_hi] against the current index.  append: keep the records and
// counters already held (the driver's later hash batches).
static int find_impl(ovl_ctx *c, uint32_t bgn, uint32_t end, uint32_t lib_lo, uint32_t lib_hi,
                     bool append, uint64_t *n_out, bool flush = true) {
  if (!c) return fail(OVL_ERR_STATE, "null context");
  if (!c->have_index) return fail(OVL_ERR_STATE, "ovl_build_hash_index() first");
  HIPC(hipSetDevice(c->device));
  if (bgn < 1) bgn = 1;
  if (bgn < c->first_iid) bgn = c->first_iid;
  uint32_t last = c->first_iid + c->nreads - 1;
  if (end > last) end = last;

  // units: (query, FORWARD), (query, REVERSE) -- Process_Overlaps.C:124-128
  std::vector<Unit> units;
  std::vector<uint64_t> uwin;
  uint64_t nref = 0;
  query_rule(c, lib_lo, lib_hi).each(bgn, end, [&](uint32_t a, bool ref, uint64_t w) {
    nref += ref;
    if (!w || a >= c->hash_end_iid) return;        // no hash read with a larger ID
    for (uint32_t dir = 0; dir < 2; dir++) {
      units.push_back(Unit{a - c->first_iid, dir});
      uwin.push_back(w);
    }
  });
  if (!append) {
    c->acc.nu = c->acc.nn = c->acc.np = 0;          // a new job: nothing pending
    ovl_stats keep_idx = c->stats;
    memset(&c->stats, 0, sizeof(c->stats));
    c->stats.ms_index = keep_idx.ms_index;
    c->stats.hash_batches = 1;
    c->nout = 0;
  }
  c->stats.ref_reads += nref;

  // OverlapDriver batches: the job's query windows sorted once (sq_prepare); this batch's
  // units are the first nu of the job's (the reads below its last hash read)
  if (c->sq_request && !units.empty())
    if (int rc = sq_prepare(c, bgn, end, lib_lo, lib_hi)) return rc;
  const bool sqm = c->sq_request && c->sq.on && !units.empty();
  if (sqm) {
    auto &Q = c->sq;
    if (units.size() > Q.units.size() ||
        memcmp(units.data(), Q.units.data(), sizeof(Unit) * units.size()) != 0)
      return fail(OVL_ERR_HIP, "sorted query windows: unit list mismatch");
    Q.probed = -1;                                  // a new index: no run probed against it
  }

  FindRun run{c, c->stream, c->P.kmer_len, c->P.frag_olap_limit != UINT64_MAX,
              c->P.use_window_filter && c->P.max_erate <= 0.06};
  if (run.window && !c->have_qual)
    return fail(OVL_ERR_BAD_PARAM, "-w (window filter) needs the reads' qualities");
  if (int rc = run.begin(units.size())) return rc;

  const uint32_t nu = (uint32_t)units.size();
  const bool bloom = nu > 0 && use_bloom(c, bgn, end);
  std::vector<uint32_t> sq_uh;                      // the probed run's unit hit counts
  size_t sq_run = 0;
  for (uint32_t u0 = 0; u0 < nu;) {
    // the search buffers are free once the extension launched from them has finished
    if (int rc = run.collect_extension()) return rc;
    ProbedBatch B;
    if (int rc = sqm ? run.probe_sorted_run(units, u0, &sq_run, &sq_uh, &B)
                     : run.probe_lookup(units, uwin, u0, bloom, &B))
      return rc;
    uint32_t nc = 0, npairs = 0, nnodes = 0;
    if (int rc = run.chain_batch(B, &nc, &npairs, &nnodes)) return rc;
    // The chunk's chains go to the accumulator (c->acc) and are extended together once
    // ACC_PAIRS pairs have gathered or the job ends, so a launch's tail (its last, longest
    // pairs on few waves) is paid once per job rather than once per probe chunk and per hash
    // batch (canu's small --hashbits batches made that tail most of a configs[4] rank's
    // extension time).  -l (a unit's pairs in the reference's order) extends each chunk as it
    // comes, from the search buffers.
    auto &fb = c->fb;
    if (!run.ordered) {
      if (int rc = run.acc_append(fb.units.p, nc, fb.pnodes.p, nnodes, fb.pairs.p, npairs)) return rc;
      if (c->acc.np >= run.acc_pairs || c->acc.nn >= ACC_NODES)
        if (int rc = run.flush_acc()) return rc;
    } else {
      if (int rc = run.launch_extension(fb.units.p, fb.pairs.p, fb.pnodes.p, npairs, nc)) return rc;
    }
    u0 += nc;
  }
  if (flush && c->acc.np)
    if (int rc = run.flush_acc()) return rc;
  if (int rc = run.collect_extension()) return rc;
  uint32_t n = 0;
  HIPC(hipMemcpy(&n, c->fb.xnout.p, 4, hipMemcpyDeviceToHost));
  c->nout = n;
  if (int rc = run.add_stats()) return rc;
  *n_out = c->nout;
  return OVL_OK;
}
