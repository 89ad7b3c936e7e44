// mhap_sketch.hip -- the sketch kernels of mhap.hip: k_mh_ordered, k_mh_keys, k_mh_minhash,
// k_mh_bitslice and k_mh_strand_fixup, with their argument structs.  Included by mhap.hip.
namespace mh {

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// Guava Hashing.murmur3_32(0) of the chars as UTF-16 (HashUtils.computeSequenceHashes
// @0-106; oracle mhap_jar.murmur3_32)
__device__ __forceinline__ uint32_t murmur32(const Strand &S, int32_t p, int32_t k) {
  const uint32_t c1 = 0xCC9E2D51u, c2 = 0x1B873593u;
  uint32_t h = 0;
  const int32_t nb = k >> 1;
  for (int32_t b = 0; b < nb; b++) {
    uint32_t kk = (uint32_t)S.ch(p + 2 * b) | ((uint32_t)S.ch(p + 2 * b + 1) << 16);
    kk *= c1; kk = rotl32(kk, 15); kk *= c2;
    h ^= kk;
    h = rotl32(h, 13); h = h * 5 + 0xE6546B64u;
  }
  if (k & 1) {
    uint32_t kk = (uint32_t)S.ch(p + k - 1);
    kk *= c1; kk = rotl32(kk, 15); kk *= c2;
    h ^= kk;
  }
  h ^= (uint32_t)(2 * k);
  h ^= h >> 16; h *= 0x85EBCA6Bu;
  h ^= h >> 13; h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// ---- ordered sketch -----------------------------------------------------------------------
struct OrderedArgs {
  const uint8_t *bases;
  const uint64_t *off;
  const uint32_t *len;
  uint32_t r0, nstrands;          // strands 2 r0 .. 2 r0 + nstrands - 1
  int32_t kk, S, min_use;         // k', ordered sketch size, shortest used read
  int32_t no_rc;
  uint64_t *ordered;              // [strand][S]: (hash ^ 0x80000000) << 32 | position
  uint32_t *ocount;
};

// key of the k'-mer at p: signed hash order, then position (stable radix sort of the jar)
__device__ __forceinline__ uint64_t okey(const Strand &S, int32_t p, int32_t kk) {
  return ((uint64_t)(murmur32(S, p, kk) ^ 0x80000000u) << 32) | (uint32_t)p;
}

// BottomOverlapSketch.<init>(s, k', S, false) @0-177 (oracle mhap_jar.ordered_sketch)
__global__ void __launch_bounds__(256) k_mh_ordered(OrderedArgs A) {
  __shared__ uint32_t hist[NBIN];
  __shared__ uint64_t list[OCAP];
  __shared__ uint32_t sD, sCnt, sBelow, sDone;
  const uint32_t sid = 2 * A.r0 + blockIdx.x;
  const uint32_t r = sid >> 1, tid = threadIdx.x;
  const int32_t L = (int32_t)A.len[r];
  const int32_t kk = A.kk;
  const int32_t npos = L - kk + 1;
  // a read shorter than --min-olap-length, or without a k'-mer, is not used; --no-rc: the
  // reverse strand is not stored
  if (L < A.min_use || npos <= 0 || ((sid & 1) && A.no_rc)) {
    if (tid == 0) A.ocount[sid] = 0;
    return;
  }
  const Strand St{A.bases + A.off[r], L, (int32_t)(sid & 1)};
  const uint32_t want = (uint32_t)min(A.S, npos);
  // radix select of the `want` smallest keys: digits of 12 bits from the top; prefix =
  // the digits fixed so far, below = keys known to be smaller than the prefix's range
  uint64_t prefix = 0;
  int32_t fixed = 0;
  uint32_t below = 0;
  uint64_t bound = 0;             // collect keys whose top (fixed + 12) bits <= bound
  int32_t bshift = 0;
  for (;;) {
    for (int32_t i = tid; i < NBIN; i += 256) hist[i] = 0;
    __syncthreads();
    const int32_t width = fixed + 12 <= 64 ? 12 : 64 - fixed;
    const int32_t sh = 64 - fixed - width;
    for (int32_t p = tid; p < npos; p += 256) {
      const uint64_t key = okey(St, p, kk);
      if (fixed == 0 || (key >> (64 - fixed)) == prefix)
        atomicAdd(&hist[(uint32_t)((key >> sh) & ((1ull << width) - 1))], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      const uint32_t need = want - below;
      uint32_t cs = 0, D = (1u << width) - 1;
      for (uint32_t b = 0; b < (1u << width); b++) {
        if (cs + hist[b] >= need) { D = b; break; }
        cs += hist[b];
      }
      sD = D;
      sBelow = below + cs;                        // keys below digit D (all selected)
      sDone = (below + cs + hist[D] <= (uint32_t)OCAP) ? 1u : 0u;
    }
    __syncthreads();
    const uint32_t D = sD;
    if (sDone) {
      bound = (fixed == 0 ? 0 : prefix << width) | D;
      bshift = sh;
      break;
    }
    below = sBelow;
    prefix = (fixed == 0 ? 0 : prefix << width) | D;
    fixed += width;
    __syncthreads();
  }
  // collect every key whose top bits are <= (prefix, D): exactly the selected ones below
  // plus all of bin D (>= want in total, <= OCAP)
  if (tid == 0) sCnt = 0;
  __syncthreads();
  for (int32_t p = tid; p < npos; p += 256) {
    const uint64_t key = okey(St, p, kk);
    if ((key >> bshift) <= bound) {
      const uint32_t idx = atomicAdd(&sCnt, 1u);
      if (idx < (uint32_t)OCAP) list[idx] = key;
    }
  }
  __syncthreads();
  const uint32_t n = min(sCnt, (uint32_t)OCAP);
  uint32_t P = 1;
  while (P < n) P <<= 1;
  for (uint32_t i = n + tid; i < P; i += 256) list[i] = ~0ull;
  __syncthreads();
  for (uint32_t kb = 2; kb <= P; kb <<= 1) {
    for (uint32_t jb = kb >> 1; jb > 0; jb >>= 1) {
      for (uint32_t i = tid; i < P; i += 256) {
        const uint32_t ix = i ^ jb;
        if (ix > i) {
          const uint64_t a = list[i], b = list[ix];
          const bool up = (i & kb) == 0;
          if ((a > b) == up) { list[i] = b; list[ix] = a; }
        }
      }
      __syncthreads();
    }
  }
  uint64_t *dst = A.ordered + (size_t)sid * A.S;
  for (uint32_t i = tid; i < want; i += 256) dst[i] = list[i];
  if (tid == 0) A.ocount[sid] = want;
}

// ---- MinHash keys ---------------------------------------------------------------------------
struct KeyArgs {
  const uint8_t *bases;
  const uint64_t *off;
  const uint32_t *len;
  const uint32_t *sids;           // the batch's strands
  const uint64_t *koff;           // per batch strand: its first key
  int32_t k;
  uint64_t *keys;
  uint32_t *pos;
};

// HashUtils.computeSequenceHashesLong(s, k, 0, false) of one strand per block
__global__ void __launch_bounds__(256) k_mh_keys(KeyArgs A) {
  const uint32_t bi = blockIdx.x, sid = A.sids[bi], r = sid >> 1;
  const int32_t L = (int32_t)A.len[r], k = A.k;
  const int32_t npos = L - k + 1;
  const Strand St{A.bases + A.off[r], L, (int32_t)(sid & 1)};
  uint64_t *out = A.keys + A.koff[bi];
  uint32_t *po = A.pos + A.koff[bi];
  for (int32_t p = threadIdx.x; p < npos; p += 256) {
    out[p] = murmur128_h1([&](int32_t q) { return St.ch(p + q); }, k);
    po[p] = (uint32_t)p;
  }
}

// ---- MinHash sketch -------------------------------------------------------------------------
struct SketchArgs {
  const uint64_t *keys;           // sorted per strand
  const uint32_t *pos;            // first positions ride along (stable sort)
  const uint64_t *koff;           // per batch strand: segment start, [nb + 1]
  const uint32_t *sids;
  int32_t H;
  int32_t mode;                   // W_ONE (repeat_weight < 0), W_TFIDF, W_COUNT
  const FreqSlot *ftab;           // null: no -f table
  uint64_t fmask;
  double range;                   // scaledIdf of a k-mer not in the table
  int32_t no_tf;
  int32_t *minhash;               // [strand][H]
  uint32_t *ocount;               // zeroed for a strand with no k-mer of weight > 0
  unsigned long long *stat;       // [0] distinct k-mers, [1] draws
  // bit-sliced draws (k_mh_bitslice; bs_w = 0: every k-mer here).  The k-mers of weight bs_w
  // past the strand's first round go to its list (bs_key / bs_fp at koff[b], bs_cnt[b] of
  // them) and this kernel leaves its exact minima in best_out instead of the sketch
  int32_t bs_w;
  uint32_t bs_sample;             // a strand's first bs_sample sorted k-mers are drawn here
  uint64_t *bs_key;
  uint32_t *bs_fp;
  uint32_t *bs_cnt;
  struct BestOut *best_out;       // [batch strand][H]
  BloomDev keep;                  // --supress-noise 1: k-mers the filter rejects never count
};

__device__ __forceinline__ const FreqSlot *table_find(const FreqSlot *t, uint64_t mask,
                                                      uint64_t key) {
  for (uint64_t h = slot_hash(key) & mask;; h = (h + 1) & mask) {
    const FreqSlot *s = t + h;
    if (!s->used) return nullptr;
    if (s->key == key) return s;
  }
}

// Math.round(double): the closest long, ties toward positive infinity
__device__ __forceinline__ int64_t java_round(double x) {
  const double f = floor(x);
  return (int64_t)f + (__dsub_rn(x, f) >= 0.5 ? 1 : 0);
}

// one xorshift64 step (<<21, >>>35, <<4)
__device__ __forceinline__ uint64_t xs64(uint64_t x) {
  x ^= x << 21;
  x ^= x >> 35;
  x ^= x << 4;
  return x;
}

// exact minimum (signed) of w xorshift64 draws from chain state x (w = 0: x is the value)
__device__ __forceinline__ int64_t exact_min(uint64_t x, int32_t w) {
  if (w == 0) return (int64_t)x;
  int64_t m = LMAX;
  for (int32_t t = 0; t < w; t++) {
    x = xs64(x);
    m = (int64_t)x < m ? (int64_t)x : m;
  }
  return m;
}

// the jar's order of candidates: the smaller draw, then the earlier first occurrence
__device__ __forceinline__ bool rec_less(const BestRec &a, const BestRec &b) {
  if (b.fp == FP_NONE) return a.fp != FP_NONE;
  if (a.fp == FP_NONE) return false;
  if (a.hi != b.hi) return a.hi < b.hi;
  const int64_t xa = exact_min(a.state, a.w), xb = exact_min(b.state, b.w);
  return xa < xb || (xa == xb && a.fp < b.fp);
}

// MinHashSketch.computeNgramMinHashesWeighted @0-476 (oracle mhap_jar.minhash); one block
// per strand, RKW distinct k-mers per thread per round.  LDS: per wave and hash function the
// best candidate so far (BestRec).
__global__ void __launch_bounds__(256) k_mh_minhash(SketchArgs A) {
  extern __shared__ uint8_t s_raw[];
  const int32_t H = A.H;
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  BestRec *best_all = (BestRec *)s_raw;                      // [4][H]
  __shared__ uint32_t s_live, s_bsn;
  for (int32_t j = tid; j < 4 * H; j += 256) best_all[j] = BestRec{0x7FFFFFFF, FP_NONE, 0, 0, 0};
  if (tid == 0) { s_live = 0; s_bsn = 0; }
  __syncthreads();
  const uint32_t bi = blockIdx.x, sid = A.sids[bi];
  const uint64_t s0 = A.koff[bi], s1 = A.koff[bi + 1];
  BestRec *best = best_all + wave * H;
  unsigned long long nkm = 0, ndraw = 0;
  for (uint64_t base = s0; base < s1; base += 256 * RKW) {
    const uint64_t p0 = base + (uint64_t)tid * RKW;
    uint64_t X[RKW];
    uint32_t KL[RKW], KH[RKW], FP[RKW];
    int32_t W[RKW];
    uint32_t listed = 0;                 // bit i: slot i's k-mer goes to the bit-sliced list
#pragma unroll
    for (int i = 0; i < RKW; i++) {
      X[i] = 0; KL[i] = KH[i] = 0; FP[i] = FP_NONE; W[i] = 0;
      const uint64_t p = p0 + i;
      if (p < s1) {
        const uint64_t key = A.keys[p];
        if (p == s0 || A.keys[p - 1] != key) {             // a run start: a distinct k-mer
          uint64_t e = p + 1;
          while (e < s1 && A.keys[e] == key) e++;
          const uint32_t cnt = (uint32_t)(e - p);
          int64_t w = cnt;
          if (A.keep.words && !bloom_has(A.keep.words, A.keep.bit_size, A.keep.k, key)) {
            w = 0;                         // keepKmer @70-83: never in the map, never drawn
          } else if (A.mode == W_ONE) {
            w = (A.ftab && table_find(A.ftab, A.fmask, key)) ? 0 : 1;
          } else if (A.mode == W_TFIDF) {
            const FreqSlot *f = A.ftab ? table_find(A.ftab, A.fmask, key) : nullptr;
            const double sidf = f ? f->sidf : A.range;
            const double tf = A.no_tf ? 1.0 : (double)cnt;
            w = java_round(__dmul_rn(tf, sidf));
            if (w < 1) w = 1;
          }
          if (w > 0 && w == A.bs_w && p >= s0 + A.bs_sample) {
            // past the strand's first bs_sample sorted positions (a sample whose minima make
            // the bit-sliced threshold tight), the dominant weight's k-mers are drawn
            // bit-sliced (k_mh_bitslice, from the minima this kernel leaves): listed below
            listed |= 1u << i;
            nkm++;
            ndraw += (unsigned long long)w * (unsigned long long)H;
            w = 0;
          }
          if (w > 0) {
            W[i] = (int32_t)(w > 0x7FFFFFFF ? 0x7FFFFFFF : w);
            X[i] = key;
            KL[i] = (uint32_t)key;
            KH[i] = (uint32_t)(key >> 32);
            FP[i] = A.pos[p];
            nkm++;
            ndraw += (unsigned long long)W[i] * (unsigned long long)H;
          }
        }
      }
    }
    if (A.bs_w) {
      // the listed k-mers appended to the strand's list, one LDS atomic per wave and slot
      const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
      for (int i = 0; i < RKW; i++) {
        const uint64_t m = __builtin_amdgcn_ballot_w64((listed >> i) & 1u);
        if (!m) continue;
        uint32_t at = 0;
        if (lane == 0) at = atomicAdd(&s_bsn, (uint32_t)popc64(m));
        at = (uint32_t)__shfl((int)at, 0) + popc64(m & lt);
        if ((listed >> i) & 1u) {
          const uint64_t p = p0 + i;
          A.bs_key[s0 + at] = A.keys[p];
          A.bs_fp[s0 + at] = A.pos[p];
        }
      }
    }
    // dead slots (W = 0) take a live slot's chain, weight and payload: a duplicate candidate
    // changes no minimum and no tie; a lane with no live slot is masked at the wave minimum
    bool live = false;
    {
      uint64_t x0 = 0;
      uint32_t l0 = 0, h0 = 0, f0 = FP_NONE;
      int32_t w0 = 0;
#pragma unroll
      for (int i = RKW - 1; i >= 0; i--)
        if (W[i] > 0) { x0 = X[i]; l0 = KL[i]; h0 = KH[i]; f0 = FP[i]; w0 = W[i]; live = true; }
#pragma unroll
      for (int i = 0; i < RKW; i++)
        if (W[i] == 0) { X[i] = x0; KL[i] = l0; KH[i] = h0; FP[i] = f0; W[i] = w0; }
    }
    if (__builtin_amdgcn_ballot_w64(live) == 0) continue;   // nothing in this wave
    // one weight for every live slot of the wave (canu's weighting: a k-mer seen once and not
    // in the -f table weighs round(1 x 10) = 10, nearly all of them): the draws are a
    // wave-uniform loop instead of a per-lane one under an exec mask per slot and draw
    int32_t wmn = 0x7FFFFFFF, wmx = 0;
#pragma unroll
    for (int i = 0; i < RKW; i++) { wmn = min(wmn, W[i]); wmx = max(wmx, W[i]); }
    if (!live) { wmn = 0x7FFFFFFF; wmx = 0; }
    wmn = wave_min_i32(wmn);
    wmx = wave_max_i32(wmx);
    const int32_t wu = wmn == wmx ? __builtin_amdgcn_readfirstlane(wmx) : 0;
    for (int32_t j = 0; j < H; j++) {
      const BestRec cur = best[j];                     // uniform (LDS broadcast)
      if (wu >= 2) {
        // high-word minima: one v_min per draw instead of a 64-bit compare and two selects
        uint64_t X0[RKW];
        int32_t mh[RKW];
#pragma unroll
        for (int i = 0; i < RKW; i++) { X0[i] = X[i]; mh[i] = 0x7FFFFFFF; }
        for (int32_t t = 0; t < wu; t++) {
#pragma unroll
          for (int i = 0; i < RKW; i++) {
            X[i] = xs64(X[i]);
            const int32_t h = (int32_t)(X[i] >> 32);
            mh[i] = h < mh[i] ? h : mh[i];
          }
        }
        int32_t lh = mh[0];
#pragma unroll
        for (int i = 1; i < RKW; i++) lh = mh[i] < lh ? mh[i] : lh;
        if (!live) lh = 0x7FFFFFFF;
        const int32_t wh = wave_min_i32(lh);
        if (cur.fp != FP_NONE && wh > cur.hi) continue;       // cannot beat the best so far
        // slots holding the wave's smallest high word
        uint32_t nmine = 0, li = 0;
#pragma unroll
        for (int i = RKW - 1; i >= 0; i--)
          if (live && mh[i] == wh) { nmine++; li = i; }
        const uint64_t who = __builtin_amdgcn_ballot_w64(nmine > 0);
        const uint32_t ln = (uint32_t)__builtin_ctzll(who);
        const bool unique = popc64(who) == 1 && __builtin_amdgcn_readlane(nmine, ln) == 1 &&
                            wh != 0x7FFFFFFF && (cur.fp == FP_NONE || wh < cur.hi);
        BestRec nb;
        if (unique) {
          // the candidate's own (state, w) stand for its exact value, fetched from lane ln
          uint64_t st = 0;
          uint32_t fp = 0, v = 0;
#pragma unroll
          for (int i = 0; i < RKW; i++)
            if ((uint32_t)i == li) { st = X0[i]; fp = FP[i]; v = (j & 1) ? KH[i] : KL[i]; }
          nb.hi = wh;
          nb.fp = __builtin_amdgcn_readlane(fp, ln);
          nb.v = __builtin_amdgcn_readlane(v, ln);
          nb.w = wu;
          // (readlane returns an int: the low word is widened unsigned, or a set bit 31 would
          // smear over the high word -- the state is a number k_mh_bitslice compares with)
          nb.state = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)(st >> 32), ln) << 32) |
                     (uint64_t)(uint32_t)__builtin_amdgcn_readlane((uint32_t)st, ln);
        } else {
          // a tie on the high word (rare): exact values by replaying the tied slots' draws
          int64_t ex = LMAX;
          uint32_t ep = FP_NONE, ev = 0;
          uint64_t es = 0;
#pragma unroll
          for (int i = 0; i < RKW; i++) {
            if (live && mh[i] == wh) {
              const int64_t e = exact_min(X0[i], wu);
              if (e < ex || (e == ex && FP[i] < ep)) {
                ex = e; ep = FP[i]; es = X0[i]; ev = (j & 1) ? KH[i] : KL[i];
              }
            }
          }
          const int64_t wx = wave_min_i64(ex);
          const uint32_t wp = wave_min_u32(ex == wx ? ep : FP_NONE);
          const uint64_t w2 = __builtin_amdgcn_ballot_w64(ex == wx && ep == wp);
          const uint32_t l2 = (uint32_t)__builtin_ctzll(w2);
          if (wx == LMAX) continue;                   // never below the jar's initial value
          nb.hi = (int32_t)((uint64_t)wx >> 32);
          nb.fp = wp;
          nb.v = __builtin_amdgcn_readlane(ev, l2);
          nb.w = 0;
          nb.state = (uint64_t)wx;
          (void)es;
        }
        if (rec_less(nb, cur) && lane == 0) best[j] = nb;
      } else {
        // exact 64-bit minima (one draw per function, or weights that differ in the wave)
        int64_t mi[RKW];
#pragma unroll
        for (int i = 0; i < RKW; i++) mi[i] = LMAX;
        if (wu == 1) {
#pragma unroll
          for (int i = 0; i < RKW; i++) {
            X[i] = xs64(X[i]);
            mi[i] = (int64_t)X[i];
          }
        } else {
#pragma unroll
          for (int i = 0; i < RKW; i++) {
            for (int32_t t = 0; t < W[i]; t++) {
              X[i] = xs64(X[i]);
              mi[i] = (int64_t)X[i] < mi[i] ? (int64_t)X[i] : mi[i];
            }
          }
        }
        // the jar's strict '<' in key order: equal draws keep the earlier first occurrence
        int64_t mx = LMAX;
        uint32_t mp = FP_NONE, mv = 0;
#pragma unroll
        for (int i = 0; i < RKW; i++) {
          if (mi[i] < mx || (mi[i] == mx && FP[i] < mp)) {
            mx = mi[i];
            mp = FP[i];
            mv = (j & 1) ? KH[i] : KL[i];
          }
        }
        if (!live) mx = LMAX;
        const int64_t wx = wave_min_i64(mx);
        if (wx == LMAX) continue;                     // no draw below the initial value
        if (cur.fp != FP_NONE && (int32_t)((uint64_t)wx >> 32) > cur.hi) continue;
        const uint64_t hold = __builtin_amdgcn_ballot_w64(mx == wx);
        uint32_t wp, wv;
        if (popc64(hold) == 1) {
          const uint32_t ln = (uint32_t)__builtin_ctzll(hold);
          wp = __builtin_amdgcn_readlane(mp, ln);
          wv = __builtin_amdgcn_readlane(mv, ln);
        } else {
          wp = wave_min_u32(mx == wx ? mp : FP_NONE);
          const uint64_t who = __builtin_amdgcn_ballot_w64(mx == wx && mp == wp);
          wv = __builtin_amdgcn_readlane(mv, (uint32_t)__builtin_ctzll(who));
        }
        const BestRec nb{(int32_t)((uint64_t)wx >> 32), wp, wv, 0, (uint64_t)wx};
        if (rec_less(nb, cur) && lane == 0) best[j] = nb;
      }
    }
  }
  for (int s = 32; s > 0; s >>= 1) {
    nkm += __shfl_xor(nkm, s);
    ndraw += __shfl_xor(ndraw, s);
  }
  if (lane == 0 && nkm) {
    atomicAdd(&s_live, 1u);
    if (A.stat) {
      atomicAdd(&A.stat[0], nkm);
      atomicAdd(&A.stat[1], ndraw);
    }
  }
  __syncthreads();
  if (A.bs_w && tid == 0) A.bs_cnt[bi] = s_bsn;
  for (int32_t j = tid; j < H; j += 256) {
    BestRec b = best_all[j];
    for (int w = 1; w < 4; w++) {
      const BestRec c = best_all[w * H + j];
      if (rec_less(c, b)) b = c;
    }
    if (A.bs_w) {
      BestOut o;
      o.val = b.fp == FP_NONE ? LMAX : exact_min(b.state, b.w);
      o.fp = b.fp;
      o.v = b.v;
      A.best_out[(size_t)bi * H + j] = o;
    } else {
      A.minhash[(size_t)sid * H + j] = b.fp == FP_NONE ? 0 : (int32_t)b.v;
    }
  }
  // no k-mer of positive weight: the jar's sketch constructor fails and the read (or this
  // strand) is skipped
  if (tid == 0 && s_live == 0) A.ocount[sid] = 0;
}

// ---- bit-sliced draws ------------------------------------------------------------------
// Nearly every k-mer of a canu sketch has the same weight (seen once, not in the -f table:
// round(1 x 10) = 10), so after a strand's first round (k_mh_minhash, exact, which leaves the
// minima so far in best_out) its k-mers of that weight are drawn 32 to a lane in BIT PLANES:
// plane b (one VGPR) holds bit b of 32 chains' states (bit p: the lane's chain p, list entry
// base + 64 p + lane).  A xorshift64 step is then 132 plane XORs for 32 chains -- the shifts
// are renamings of planes -- instead of 2 64-bit shifts, 5 XORs and a right shift per chain.
// The minimum is not tracked per chain: a draw matters only if it is <= the function's best
// so far T, and since T is small after the exact round (the minimum of ~20 k draws), a draw
// can be below it only if the top Z bits of x ^ 2^63 are zero, Z = clz(T ^ 2^63): one OR over
// Z planes tests 32 chains.  The few chains that pass are read out of the planes (the exact
// 64-bit draw) and compared with the best in the jar's order -- smaller draw, then earlier
// first occurrence -- so the result is the exact minimum whatever the draw order.
constexpr uint32_t BS_CHAINS = 2048;     // k-mers per wave per batch (64 lanes x 32 planes)

__device__ __forceinline__ void bs_step(uint32_t (&S)[64]) {
#pragma unroll
  for (int b = 63; b >= 21; b--) S[b] ^= S[b - 21];       // x ^= x << 21
#pragma unroll
  for (int b = 0; b <= 28; b++) S[b] ^= S[b + 35];        // x ^= x >>> 35
#pragma unroll
  for (int b = 63; b >= 4; b--) S[b] ^= S[b - 4];         // x ^= x << 4
}

// draws t.. of the current function until one leaves a chain that may be <= T (its top Z
// bits of x ^ 2^63 all zero) or the function's w draws are done; returns the next draw
template <int Z>
__device__ __forceinline__ int32_t bs_draws(uint32_t (&S)[64], uint32_t valid, int32_t t,
                                            int32_t w, uint32_t &cand) {
  for (; t < w;) {
    bs_step(S);
    t++;
    uint32_t c = valid;
    if constexpr (Z > 0) {
      uint32_t z = ~S[63];                                  // the sign bit, flipped
#pragma unroll
      for (int i = 1; i < Z; i++) z |= S[63 - i];
      c &= ~z;
    }
    if (__builtin_amdgcn_ballot_w64(c != 0)) { cand = c; return t; }
  }
  cand = 0;
  return t;
}

struct BsArgs {
  const uint64_t *bs_key;         // per batch strand at koff[b]: keys of its listed k-mers
  const uint32_t *bs_fp;          //   and their first positions
  const uint32_t *bs_cnt;
  const uint64_t *koff;
  const uint32_t *sids;
  const BestOut *best_in;         // [batch strand][H]: k_mh_minhash's minima
  int32_t H;
  int32_t w;                      // the listed k-mers' weight
  int32_t *minhash;               // [strand][H]
  int32_t zmax;                   // planes tested at most (MHAP_BS_ZMAX, A/B and checks: 64)
};

__device__ __forceinline__ uint32_t uni_u32(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)v);
}

// one wave per strand
__global__ void __launch_bounds__(64, 5) k_mh_bitslice(BsArgs A) {
  extern __shared__ uint8_t s_raw[];
  BestOut *best = (BestOut *)s_raw;                          // [H]
  const uint32_t lane = threadIdx.x, bi = blockIdx.x, sid = A.sids[bi];
  const int32_t H = A.H, w = A.w;
  for (int32_t j = lane; j < H; j += 64) best[j] = A.best_in[(size_t)bi * H + j];
  wave_sync();
  const uint64_t s0 = A.koff[bi];
  const uint32_t n = A.bs_cnt[bi];
  const uint64_t *keys = A.bs_key + s0;
  const uint32_t *fps = A.bs_fp + s0;
  for (uint32_t base = 0; base < n; base += BS_CHAINS) {
    uint32_t S[64];
#pragma unroll
    for (int b = 0; b < 64; b++) S[b] = 0;
    uint32_t valid = 0;
    for (uint32_t p = 0; p < 32; p++) {
      const uint32_t idx = base + p * 64 + lane;
      if (idx < n) {
        const uint64_t key = keys[idx];
        const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
        valid |= 1u << p;
#pragma unroll
        for (int b = 0; b < 32; b++) {
          S[b] |= ((lo >> b) & 1u) << p;
          S[b + 32] |= ((hi >> b) & 1u) << p;
        }
      }
    }
    for (int32_t j = 0; j < H; j++) {
      BestOut cur = best[j];
      cur.fp = uni_u32(cur.fp);
      cur.v = uni_u32(cur.v);
      cur.val = (int64_t)(((uint64_t)uni_u32((uint32_t)((uint64_t)cur.val >> 32)) << 32) |
                          uni_u32((uint32_t)cur.val));
      bool changed = false;
      for (int32_t t = 0; t < w;) {
        // draws may be <= T only with their top Z bits (of x ^ 2^63) clear; fewer planes
        // tested is a looser filter, never a wrong one
        const uint64_t U = cur.fp == FP_NONE ? ~0ull : ((uint64_t)cur.val ^ (1ull << 63));
        const int32_t Z = min(U == 0 ? 64 : (int32_t)__builtin_clzll(U), A.zmax);
        uint32_t cand = 0;
        // a filter of fewer planes than Z lets up to 2^(Z - planes) x the true candidates
        // through: a step per plane where the sample leaves Z (13-16), coarser outside
        if (Z >= 20)      t = bs_draws<20>(S, valid, t, w, cand);
        else if (Z >= 18) t = bs_draws<18>(S, valid, t, w, cand);
        else if (Z >= 16) t = bs_draws<16>(S, valid, t, w, cand);
        else if (Z == 15) t = bs_draws<15>(S, valid, t, w, cand);
        else if (Z == 14) t = bs_draws<14>(S, valid, t, w, cand);
        else if (Z == 13) t = bs_draws<13>(S, valid, t, w, cand);
        else if (Z >= 10) t = bs_draws<10>(S, valid, t, w, cand);
        else if (Z >= 6)  t = bs_draws<6>(S, valid, t, w, cand);
        else              t = bs_draws<0>(S, valid, t, w, cand);
        if (!__builtin_amdgcn_ballot_w64(cand != 0)) continue;
        const uint32_t T_hi = (uint32_t)((uint64_t)cur.val >> 32);
        // the lane's smallest (draw, first position) among its passing chains that beats the
        // best so far (a strict '<' on the draw, then the earlier first occurrence)
        int64_t bv = LMAX;
        uint32_t bfp = FP_NONE, bidx = 0;
        for (uint32_t m = cand; m;) {
          const uint32_t c = (uint32_t)__builtin_ctz(m);
          m &= m - 1;
          // the high word first: most passing chains are above T there
          uint32_t hi = 0;
#pragma unroll
          for (int b = 0; b < 32; b++) hi |= ((S[b + 32] >> c) & 1u) << b;
          if (cur.fp != FP_NONE && (int32_t)hi > (int32_t)T_hi) continue;
          uint32_t lo = 0;
#pragma unroll
          for (int b = 0; b < 32; b++) lo |= ((S[b] >> c) & 1u) << b;
          const int64_t v = (int64_t)(((uint64_t)hi << 32) | lo);
          const uint32_t idx = base + c * 64 + lane;
          const uint32_t fp = fps[idx];
          const bool beats = cur.fp == FP_NONE ? v < LMAX
                                               : (v < cur.val || (v == cur.val && fp < cur.fp));
          if (beats && (v < bv || (v == bv && fp < bfp))) { bv = v; bfp = fp; bidx = idx; }
        }
        if (!__builtin_amdgcn_ballot_w64(bv != LMAX)) continue;   // no draw beat it
        const int64_t wv = wave_min_i64(bv);
        const uint32_t wp = wave_min_u32(bv == wv ? bfp : FP_NONE);
        const uint64_t who = __builtin_amdgcn_ballot_w64(bv == wv && bfp == wp);
        const uint32_t widx = uni_u32(__builtin_amdgcn_readlane(bidx, (uint32_t)__builtin_ctzll(who)));
        const uint64_t key = keys[widx];
        cur.val = wv;
        cur.fp = wp;
        cur.v = (j & 1) ? (uint32_t)(key >> 32) : (uint32_t)key;
        changed = true;
      }
      if (changed) {
        if (lane == 0) best[j] = cur;
        wave_sync();
      }
    }
  }
  wave_sync();
  for (int32_t j = lane; j < H; j += 64) {
    const BestOut b = best[j];
    A.minhash[(size_t)sid * H + j] = b.fp == FP_NONE ? 0 : (int32_t)b.v;
  }
}

// a read whose forward strand was skipped is skipped whole (SequenceSketchStreamer
// .enqueue @67-95: the reverse strand is made only after the forward one)
__global__ void k_mh_strand_fixup(uint32_t *ocount, uint32_t r0, uint32_t nr) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nr && ocount[2 * (r0 + i)] == 0) ocount[2 * (r0 + i) + 1] = 0;
}
}  // namespace mh
