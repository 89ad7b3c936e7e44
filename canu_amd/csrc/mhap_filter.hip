// mhap_filter.hip -- the index and the two-stage filter of mhap.hip: k_mh_index_keys,
// k_mh_table_offsets, k_mh_candidates and k_mh_compare, with their argument structs.  Included by
// mhap.hip.
namespace mh {

// ---- index ----------------------------------------------------------------------------------
// (j << 32 | value ^ 0x80000000) -> stored strand; strands not stored -> table H
__global__ void k_mh_index_keys(const int32_t *mh, const uint32_t *ocount, uint32_t s0,
                                uint32_t ns, int32_t H, uint64_t *keys, uint32_t *vals) {
  const size_t n = (size_t)ns * H;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < n;
       e += (size_t)gridDim.x * blockDim.x) {
    const uint32_t sid = s0 + (uint32_t)(e / H), j = (uint32_t)(e % H);
    const int32_t v = mh[(size_t)s0 * H + e];
    keys[e] = ocount[sid] == 0 ? ((uint64_t)H << 32)
                               : (((uint64_t)j << 32) | ((uint32_t)v ^ 0x80000000u));
    vals[e] = sid;
  }
}

__global__ void k_mh_table_offsets(const uint64_t *keys, size_t n, int32_t H, uint64_t *off) {
  const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j > H) return;
  const uint64_t key = (uint64_t)j << 32;
  size_t lo = 0, hi = n;
  while (lo < hi) {
    const size_t mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  off[j] = lo;
}

// ---- first stage ----------------------------------------------------------------------------
struct CandArgs {
  const int32_t *mh;
  const uint32_t *ocount;
  const uint32_t *len;
  const uint64_t *keys;
  const uint32_t *vals;
  const uint64_t *toff;
  int32_t H;
  uint32_t q0, q1;                // query reads [q0, q1)
  uint32_t self;                  // 1: toSelf (stored reads of smaller ID), 0: all but q
  int32_t min_store;
  uint32_t min_matches;
  Cand *out;
  uint32_t *nout;
  uint32_t cap;
  uint32_t *overflow;
};

// MinHashSearch.findMatches(query, toSelf) @0-492 (oracle mhap_jar.find_matches)
__global__ void __launch_bounds__(256) k_mh_candidates(CandArgs A) {
  extern __shared__ uint32_t s_tab[];              // [4][TSLOTS] keys, then [4][TSLOTS] counts
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t q = A.q0 + blockIdx.x * 4 + wave;
  if (q >= A.q1) return;                           // whole wave leaves together
  if (A.ocount[2 * q] == 0) return;                // query not used
  uint32_t *tk = s_tab + wave * TSLOTS;
  uint32_t *tc = s_tab + 4 * TSLOTS + wave * TSLOTS;
  for (uint32_t i = lane; i < TSLOTS; i += 64) { tk[i] = 0; tc[i] = 0; }
  wave_sync();
  const int32_t qlen = (int32_t)A.len[q], ms = A.min_store;
  bool ovf = false;
  for (int32_t j = lane; j < A.H; j += 64) {
    const int32_t v = A.mh[(size_t)(2 * q) * A.H + j];
    const uint64_t key = ((uint64_t)j << 32) | ((uint32_t)v ^ 0x80000000u);
    uint64_t lo = A.toff[j], hi = A.toff[j + 1];
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (A.keys[mid] < key) lo = mid + 1;
      else hi = mid;
    }
    const uint64_t end = A.toff[j + 1];
    for (uint64_t i = lo; i < end && A.keys[i] == key; i++) {
      const uint32_t t = A.vals[i], tr = t >> 1;
      if (tr == q) continue;
      const int32_t tlen = (int32_t)A.len[tr];
      if (tlen < ms && qlen < ms) continue;                                 // @393-416
      if (A.self && tr > q && tlen >= ms && qlen >= ms) continue;           // @419-462
      if (A.self && tlen < ms && qlen >= ms) continue;                      // @465-492
      uint32_t sl = ((t + 1) * 2654435761u) >> TSHIFT;
      uint32_t probes = 0;
      for (;;) {
        const uint32_t old = atomicCAS(&tk[sl], 0u, t + 1);
        if (old == 0u || old == t + 1) { atomicAdd(&tc[sl], 1u); break; }
        sl = (sl + 1) & (TSLOTS - 1);
        if (++probes >= TSLOTS) { ovf = true; break; }
      }
      if (ovf) break;
    }
  }
  wave_sync();
  if (ovf) atomicOr(A.overflow, 1u);
  for (uint32_t i = lane; i < TSLOTS; i += 64) {
    const uint32_t key = tk[i], c = tc[i];
    if (key && c >= A.min_matches) {
      const uint32_t idx = atomicAdd(A.nout, 1u);
      if (idx < A.cap) A.out[idx] = Cand{q, key - 1, c, 0};
      else atomicOr(A.overflow, 2u);
    }
  }
}

// ---- second stage ---------------------------------------------------------------------------
struct CmpArgs {
  const Cand *cand;
  uint32_t ncand;
  const uint64_t *ordered;
  const uint32_t *ocount;
  const uint32_t *len;
  int32_t S, kk;
  double max_shift;
  const uint32_t *pass;           // bit n (S + 1) + inter: identity(inter / n) >= threshold
  uint32_t pass_empty;            // identity 0 (n = 0) >= threshold
  RecDev *out;
  uint32_t *nout;
  uint32_t cap;
  uint32_t *overflow;
};

__device__ __forceinline__ uint32_t hash_of(uint64_t e) { return (uint32_t)(e >> 32); }
__device__ __forceinline__ int32_t pos_of(uint64_t e) { return (int32_t)(uint32_t)e; }

// A group: the entries of one hash present in both sketches, A[a0, a1) and B[b0, b1)
struct Group {
  uint32_t a0, a1, b0, b1;
};
__device__ __forceinline__ uint64_t pack_group(uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
  return (uint64_t)a0 | ((uint64_t)a1 << 16) | ((uint64_t)b0 << 32) | ((uint64_t)b1 << 48);
}
__device__ __forceinline__ Group unpack_group(uint64_t g) {
  return Group{(uint32_t)(g & 0xFFFF), (uint32_t)((g >> 16) & 0xFFFF),
               (uint32_t)((g >> 32) & 0xFFFF), (uint32_t)(g >> 48)};
}

// MatchData's state for one recordMatchingKmers pass: median shift, its absMax and the
// valid position windows (performUpdate @0-134, valid1/2Lower/Upper)
struct Window {
  int32_t m, amax, v1lo, v1hi, v2lo, v2hi;
};

__device__ __forceinline__ Window make_window(int32_t m, int32_t amax, int32_t sl1, int32_t sl2) {
  Window w;
  w.m = m;
  w.amax = amax;
  w.v1lo = max(0, -m - amax);
  w.v2lo = max(0, m - amax);
  w.v1hi = min(sl1, sl2 - m + amax);
  w.v2hi = min(sl2, sl1 + m + amax);
  return w;
}

// performUpdate with records whose median shift is m
__device__ __forceinline__ int32_t abs_max(int32_t m, int32_t sl1, int32_t sl2, double msp) {
  const int32_t lo = max(0, -m);
  const int32_t hi = min(sl1, sl2 - m);
  const int32_t olap = max(10, hi - lo);
  return min(max(sl1, sl2), (int32_t)__dmul_rn((double)olap, msp));
}

// recordMatchingKmers @0-450 restricted to one group (the jar's merge only ever compares
// entries of equal hash when it records, and enters each group at its first entries on both
// sides, so groups are independent): emit(p1, p2) per recorded match, in the jar's order
template <class Emit>
__device__ __forceinline__ void group_records(const uint64_t *A, const uint64_t *B, Group g,
                                              const Window &w, Emit emit) {
  uint32_t i1 = g.a0, i2 = g.b0;
  while (i1 < g.a1 && i2 < g.b1) {
    const int32_t p1 = pos_of(A[i1]);
    if (p1 < w.v1lo || p1 >= w.v1hi) { i1++; continue; }
    const int32_t p2 = pos_of(B[i2]);
    if (p2 < w.v2lo || p2 >= w.v2hi) { i2++; continue; }
    const int32_t d = (p2 - p1) - w.m;
    if (d > w.amax) { i1++; continue; }
    if (d < -w.amax) { i2++; continue; }
    emit(p1, p2);
    uint32_t l1 = i1, l2 = i2;
    for (uint32_t j = i1 + 1; j < g.a1; j++) {
      const int32_t p = pos_of(A[j]);
      if (p < w.v1lo || p >= w.v1hi) break;
      l1 = j;
    }
    for (uint32_t j = i2 + 1; j < g.b1; j++) {
      const int32_t p = pos_of(B[j]);
      if (p < w.v2lo || p >= w.v2hi) break;
      l2 = j;
    }
    if (l1 == i1 && l2 == i2) {
      i1++;
      i2++;
    } else {
      emit(pos_of(A[l1]), pos_of(B[l2]));
      i1 = l1 + 1;
      i2 = l2 + 1;
    }
  }
}

// the same records after optimizeShifts @0-165 (consecutive records of one p1 keep the one
// whose shift is nearest the median m; equal p1 only ever occur inside a group)
template <class Emit>
__device__ __forceinline__ void group_records_opt(const uint64_t *A, const uint64_t *B, Group g,
                                                  const Window &w, int32_t m, Emit emit) {
  bool has = false;
  int32_t q1 = 0, q2 = 0;
  group_records(A, B, g, w, [&](int32_t p1, int32_t p2) {
    if (has && q1 == p1) {
      if (abs(q2 - q1 - m) > abs(p2 - p1 - m)) q2 = p2;
    } else {
      if (has) emit(q1, q2);
      has = true;
      q1 = p1;
      q2 = p2;
    }
  });
  if (has) emit(q1, q2);
}

// The (count / 2)-th smallest shift p2 - p1 over the records gen() emits (Utils.quickSelect
// of performUpdate): a radix select over u = shift + off (off = sl1, so u > 0) in 8-bit
// digits; count = the number of records (0: none)
template <class Gen>
__device__ int32_t wave_median(Gen gen, int32_t off, uint32_t bits, uint32_t *hist,
                               uint32_t lane, uint32_t &count) {
  const int npass = (int)((bits + 7) / 8);
  uint32_t prefix = 0, pmask = 0, kth = 0;
  count = 0;
  for (int pass = npass - 1; pass >= 0; pass--) {
    for (uint32_t i = lane; i < 256; i += 64) hist[i] = 0;
    wave_sync();
    gen([&](int32_t p1, int32_t p2) {
      const uint32_t u = (uint32_t)(p2 - p1 + off);
      if ((u & pmask) == prefix) atomicAdd(&hist[(u >> (8 * pass)) & 255u], 1u);
    });
    wave_sync();
    const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2],
                   h3 = hist[4 * lane + 3];
    const uint32_t tot = h0 + h1 + h2 + h3;
    uint32_t incl = tot;
    for (int sft = 1; sft < 64; sft <<= 1) {
      const uint32_t v = __shfl_up(incl, sft);
      if ((int)lane >= sft) incl += v;
    }
    if (pass == npass - 1) {
      count = __shfl(incl, 63);
      if (count == 0) return 0;
      kth = count / 2;
    }
    const uint32_t excl = incl - tot;
    const bool mine = excl <= kth && kth < incl;
    const uint64_t who = __builtin_amdgcn_ballot_w64(mine);
    const uint32_t owner = (uint32_t)__builtin_ctzll(who);
    uint32_t bin = 0, before = excl;
    if (mine) {
      const uint32_t rem = kth - excl;
      if (rem < h0) bin = 0;
      else if (rem < h0 + h1) { bin = 1; before += h0; }
      else if (rem < h0 + h1 + h2) { bin = 2; before += h0 + h1; }
      else { bin = 3; before += h0 + h1 + h2; }
      bin += 4 * lane;
    }
    bin = __shfl(bin, owner);
    before = __shfl(before, owner);
    kth -= before;
    prefix |= bin << (8 * pass);
    pmask |= 255u << (8 * pass);
    wave_sync();
  }
  return (int32_t)prefix - off;
}

// BottomOverlapSketch.getOverlapInfo(other, maxShift) @0-211 (oracle mhap_jar.overlap_info);
// one wave per candidate; LDS per wave: A [S], B [S], groups [S] (u64) and a 256-bin histogram
__global__ void __launch_bounds__(64) k_mh_compare(CmpArgs A) {
  extern __shared__ uint64_t s_cmp[];
  const uint32_t lane = threadIdx.x;
  const int32_t S = A.S;
  uint64_t *la = s_cmp;
  uint64_t *lb = la + S;
  uint64_t *lg = lb + S;
  uint32_t *hist = (uint32_t *)(lg + S);
  const uint64_t lane_lt = (1ull << lane) - 1;
  for (uint32_t c = blockIdx.x; c < A.ncand; c += gridDim.x) {
    wave_sync();                                   // the previous pair's LDS reads are done
    const Cand cd = A.cand[c];
    const uint32_t sa = 2 * cd.q, sb = cd.t;
    const uint32_t na = A.ocount[sa], nb = A.ocount[sb];
    const int32_t la_len = (int32_t)A.len[cd.q], lb_len = (int32_t)A.len[sb >> 1];
    const int32_t sl1 = la_len - A.kk + 1, sl2 = lb_len - A.kk + 1;   // seqLength
    {
      const uint64_t *ga = A.ordered + (size_t)sa * S;
      const uint64_t *gb = A.ordered + (size_t)sb * S;
      for (uint32_t i = lane; i < na; i += 64) la[i] = ga[i];
      for (uint32_t i = lane; i < nb; i += 64) lb[i] = gb[i];
    }
    wave_sync();
    // groups, in hash order: lane l owns A[l c, l c + c) and the groups starting there
    const uint32_t crun = (na + 63) / 64;
    const uint32_t a_lo = lane * crun, a_hi = min(a_lo + crun, na);
    auto discover = [&](auto found) {
      uint32_t bp = 0;
      if (a_lo < a_hi) {                           // lower bound of A[a_lo]'s hash in B
        const uint32_t h = hash_of(la[a_lo]);
        uint32_t lo = 0, hi = nb;
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (hash_of(lb[mid]) < h) lo = mid + 1;
          else hi = mid;
        }
        bp = lo;
      }
      for (uint32_t i = a_lo; i < a_hi; i++) {
        const uint32_t h = hash_of(la[i]);
        if (i > 0 && hash_of(la[i - 1]) == h) continue;   // not a group start
        while (bp < nb && hash_of(lb[bp]) < h) bp++;
        if (bp < nb && hash_of(lb[bp]) == h) {
          uint32_t ae = i + 1, be = bp + 1;
          while (ae < na && hash_of(la[ae]) == h) ae++;
          while (be < nb && hash_of(lb[be]) == h) be++;
          found(i, ae, bp, be);
        }
      }
    };
    uint32_t mine = 0;
    discover([&](uint32_t, uint32_t, uint32_t, uint32_t) { mine++; });
    uint32_t goff = mine;                          // exclusive scan over lanes
    for (int sft = 1; sft < 64; sft <<= 1) {
      const uint32_t v = __shfl_up(goff, sft);
      if ((int)lane >= sft) goff += v;
    }
    const uint32_t ngroups = __shfl(goff, 63);
    goff -= mine;
    if (ngroups == 0) continue;                    // no shared k'-mer: EMPTY
    discover([&](uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
      lg[goff++] = pack_group(a0, a1, b0, b1);
    });
    wave_sync();
    const uint32_t bits = 32u - (uint32_t)__builtin_clz((uint32_t)(sl1 + sl2));
    // pass 0: no records yet -> median 0, absMax = max(seqLength) + 1, everything valid
    const Window w0 = make_window(0, max(sl1, sl2) + 1, sl1, sl2);
    uint32_t n0 = 0;
    const int32_t m0 = wave_median([&](auto emit) {
      for (uint32_t g = lane; g < ngroups; g += 64) group_records(la, lb, unpack_group(lg[g]), w0, emit);
    }, sl1, bits, hist, lane, n0);
    if (n0 == 0) continue;
    // pass 1 in the windows of pass 0's median
    const Window w1 = make_window(m0, abs_max(m0, sl1, sl2, A.max_shift), sl1, sl2);
    uint32_t n1 = 0;
    const int32_t m1 = wave_median([&](auto emit) {
      for (uint32_t g = lane; g < ngroups; g += 64) group_records(la, lb, unpack_group(lg[g]), w1, emit);
    }, sl1, bits, hist, lane, n1);
    if (n1 == 0) continue;
    // optimizeShifts with pass 1's median, then computeEdges with the new median
    uint32_t n2 = 0;
    const int32_t m2 = wave_median([&](auto emit) {
      for (uint32_t g = lane; g < ngroups; g += 64)
        group_records_opt(la, lb, unpack_group(lg[g]), w1, m1, emit);
    }, sl1, bits, hist, lane, n2);
    const int32_t a2m = abs_max(m2, sl1, sl2, A.max_shift);
    int32_t cnt = 0, l1 = 0x7FFFFFFF, l2 = 0x7FFFFFFF, r1 = (int32_t)0x80000000,
            r2 = (int32_t)0x80000000;
    for (uint32_t g = lane; g < ngroups; g += 64) {
      group_records_opt(la, lb, unpack_group(lg[g]), w1, m1, [&](int32_t p1, int32_t p2) {
        if (abs(p2 - p1 - m2) > a2m) return;
        l1 = min(l1, p1); l2 = min(l2, p2);
        r1 = max(r1, p1); r2 = max(r2, p2);
        cnt++;
      });
    }
    cnt = wave_sum_i32(cnt);
    if (cnt < 3) continue;
    l1 = wave_min_i32(l1); l2 = wave_min_i32(l2);
    r1 = wave_max_i32(r1); r2 = wave_max_i32(r2);
    // computeEdges @118-236: int imul / isub (wrapping), i2d, ddiv, Math.round, l2i
    auto edge = [&](int32_t x, int32_t y) {
      const int32_t num = (int32_t)((uint32_t)((uint32_t)cnt * (uint32_t)x) - (uint32_t)y);
      return (int32_t)java_round((double)num / (double)(cnt - 1));
    };
    const int32_t e_a1 = max(0, edge(l1, r1));
    const int32_t e_a2 = min(sl1, edge(r1, l1));
    const int32_t e_b1 = max(0, edge(l2, r2));
    const int32_t e_b2 = min(sl2, edge(r2, l2));
    // computeKBottomSketchJaccard @0-227: the entries of each sketch whose position lies in
    // its edge range (in hash order), n = min of the two counts, a merge of n steps counting
    // equal hashes.  Closed form: a value v present in both with rx / ry entries in range
    // takes max(rx, ry) steps, min(rx, ry) of them equal, after xr + yr - E(< v) steps (xr,
    // yr: entries in range below v; E: equal steps of smaller values); a value in one
    // sketch only adds steps, no equality.  The hash halves of la / lb are replaced by the
    // exclusive prefix counts of in-range entries (group discovery is done).
    uint32_t nx = 0, ny = 0;
    for (uint32_t i0 = 0; i0 < na; i0 += 64) {
      const uint32_t i = i0 + lane;
      bool in = false;
      int32_t p = 0;
      if (i < na) { p = pos_of(la[i]); in = p >= e_a1 && p <= e_a2; }
      const uint64_t m = __builtin_amdgcn_ballot_w64(in);
      if (i < na) la[i] = ((uint64_t)(nx + popc64(m & lane_lt)) << 32) | (uint32_t)p;
      nx += popc64(m);
    }
    for (uint32_t i0 = 0; i0 < nb; i0 += 64) {
      const uint32_t i = i0 + lane;
      bool in = false;
      int32_t p = 0;
      if (i < nb) { p = pos_of(lb[i]); in = p >= e_b1 && p <= e_b2; }
      const uint64_t m = __builtin_amdgcn_ballot_w64(in);
      if (i < nb) lb[i] = ((uint64_t)(ny + popc64(m & lane_lt)) << 32) | (uint32_t)p;
      ny += popc64(m);
    }
    wave_sync();
    const uint32_t n = min(nx, ny);
    uint32_t inter = 0;
    if (n > 0) {
      uint32_t carry = 0;                         // E over the groups before this chunk
      for (uint32_t g0 = 0; g0 < ngroups; g0 += 64) {
        const uint32_t g = g0 + lane;
        uint32_t eq = 0, xr = 0, yr = 0;
        if (g < ngroups) {
          const Group G = unpack_group(lg[g]);
          xr = hash_of(la[G.a0]);
          yr = hash_of(lb[G.b0]);
          const uint32_t xe = G.a1 < na ? hash_of(la[G.a1]) : nx;
          const uint32_t ye = G.b1 < nb ? hash_of(lb[G.b1]) : ny;
          eq = min(xe - xr, ye - yr);
        }
        uint32_t incl = eq;
        for (int sft = 1; sft < 64; sft <<= 1) {
          const uint32_t v = __shfl_up(incl, sft);
          if ((int)lane >= sft) incl += v;
        }
        const int64_t steps = (int64_t)xr + yr - (int64_t)(carry + incl - eq);
        const int64_t left = (int64_t)n - steps;
        uint32_t got = 0;
        if (eq && left > 0) got = (uint32_t)min<int64_t>(eq, left);
        inter += got;
        carry += __shfl(incl, 63);
      }
      inter = (uint32_t)wave_sum_i32((int32_t)inter);
    }
    const bool ok = n == 0 ? A.pass_empty != 0
                           : ((A.pass[((size_t)n * (S + 1) + inter) >> 5] >> (((size_t)n * (S + 1) + inter) & 31)) & 1u) != 0;
    if (!ok) continue;
    if (lane == 0) {
      const uint32_t idx = atomicAdd(A.nout, 1u);
      if (idx < A.cap) {
        RecDev rr;
        rr.a = cd.q;
        rr.b = sb >> 1;
        rr.o = sb & 1;
        rr.cnt = cd.cnt;
        rr.inter = inter;
        rr.n = n;
        rr.raw = (uint32_t)cnt;
        rr.pad = 0;
        rr.a1 = e_a1; rr.a2 = e_a2; rr.a_len = la_len;
        // MatchResult.<init> @86-143: reverse-strand coordinates mirrored on the read
        rr.b1 = rr.o ? lb_len - e_b2 - 1 : e_b1;
        rr.b2 = rr.o ? lb_len - e_b1 - 1 : e_b2;
        rr.b_len = lb_len;
        A.out[idx] = rr;
      } else {
        atomicOr(A.overflow, 1u);
      }
    }
  }
}

}  // namespace mh
