// meryl.hip -- libcanu_meryl.so: canu's k-mer count (meryl -B -C -L) on one gfx950 device.
//
// The reads stay resident, 2-bit packed with an exception mask (one invalid position is
// inserted after every read, so "no invalid position among the k" is the whole validity
// rule: a mer spans neither a read end nor a non-ACGT byte).  The mers are never all
// resident: the key space (the canonical mer as a 2k-bit number) is cut into consecutive
// ranges that each fit the budget, and every range is one pass:
//
//   k_prefix_hist   scan the reads, histogram the keys of a range by their top bits (LDS-
//                   privatised).  Used by the planner (which cuts the ranges, recursing into
//                   a bin that alone exceeds the budget, down to a single key whose count the
//                   histogram then is) and, per pass, for the bucket sizes.
//   k_scatter       scan the reads again, keep the keys of the pass, collect them in an LDS
//                   tile, order the tile by bucket and write every bucket's run to consecutive
//                   addresses (one cursor reservation per bucket and tile).
//   k_fine          one work-group per bucket: bitonic sort in LDS, run lengths by binary
//                   search, (mer, count >= L) out by a block prefix sum, counts into the
//                   histogram.  A bucket larger than the LDS sort is split on further key
//                   bits, as often as needed; a sub-range of one key is counted directly.
//   k_compact       close the gaps between the buckets' outputs.
//
// Passes run in ascending key order, so their outputs concatenate into the sorted list.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <map>
#include <string>
#include <vector>

#include "../../include/canu_meryl.h"
#include "meryl_host.h"

typedef unsigned long long u64;
typedef unsigned int u32;

namespace {

constexpr u32 PLAN_BITS = 12;           // planner / bucket histogram: at most 4096 bins
constexpr u32 NB_MAX = 4096;            // buckets of one pass
constexpr u32 BUCKET_TARGET = 8192;     // mean keys per bucket the pass size aims at
constexpr u32 FINE_CAP = 16384;         // keys k_fine sorts in LDS at once
constexpr u32 FINE_THREADS = 1024;
constexpr u32 SUB_BINS = 1024;          // k_fine's split of an oversize bucket
constexpr u32 SC_THREADS = 512;
constexpr u32 SC_PER_THREAD = 8;        // mer starts per thread and chunk
constexpr u32 SC_CHUNK_WORDS = SC_THREADS * SC_PER_THREAD / 32;   // 128 words = 4096 starts
constexpr u32 SC_TILE = 8192;           // keys of one LDS tile (flushed above SC_TILE - 4096)
constexpr u32 HIST_DENSE = 65536;       // device histogram length; larger counts: overflow list
constexpr u32 OVF_CAP = 4096;           // overflow list, drained after every pass; a pass is cut to
                                        // at most dense length x list length mers, so it cannot fill
constexpr u32 SMALL_HIST = 256;
constexpr size_t SC_LDS = SC_TILE * 8 + SC_TILE * 2 + 3 * NB_MAX * 4 + 128;
constexpr size_t FINE_LDS = FINE_CAP * 8 + SUB_BINS * 4 + SMALL_HIST * 4 + 256;
constexpr u64 STAGE_POSITIONS = 16ull << 20;   // host upload staging, one byte per position
constexpr u64 PASS_BYTES_PER_KEY = 24;  // keys 8 (reused by the compaction) + out 8+4 + 4

thread_local std::string g_err;
int fail(int code, const std::string &m) { g_err = m; return code; }

#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess)                                                                  \
      return fail(e_ == hipErrorOutOfMemory ? MER_ERR_OOM : MER_ERR_HIP,                   \
                  std::string(#x) + ": " + hipGetErrorString(e_));                         \
  } while (0)

// ---------------------------------------------------------------------------------- device

// The key of the mer that starts at bit offset j (0..31) of the word pair (hi, lo); mask bits
// are one per position, most significant first like the bases.
__device__ __forceinline__ bool mer_at(u64 hi, u64 lo, u64 m64, u32 j, u32 k, int canonical,
                                       u64 &key) {
  if (((m64 << j) >> (64 - k)) != 0) return false;
  u64 x = j ? ((hi << (2 * j)) | (lo >> (64 - 2 * j))) : hi;
  u64 f = x >> (64 - 2 * k);
  if (canonical) {
    u64 r = __brevll(~f);
    r = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);
    r >>= (64 - 2 * k);
    f = r < f ? r : f;
  }
  key = f;
  return true;
}

__device__ __forceinline__ u32 base_code(unsigned char c) {
  c &= 0xDF;
  return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}

// stage: one byte per position for words [w0, w0 + n), separators and padding as 0.
__global__ void k_pack_stage(const unsigned char *__restrict__ stage, u64 w0, u64 n,
                             u64 *__restrict__ W, u32 *__restrict__ M) {
  u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint4 *p = reinterpret_cast<const uint4 *>(stage + t * 32);
  uint4 q[2] = {p[0], p[1]};
  const unsigned char *b = reinterpret_cast<const unsigned char *>(q);
  u64 w = 0;
  u32 m = 0;
  for (int i = 0; i < 32; i++) {
    u32 c = base_code(b[i]);
    w = (w << 2) | (c & 3);
    m = (m << 1) | (c >> 2);
  }
  W[w0 + t] = w;
  M[w0 + t] = m;
}

// The same from reads in device memory: pstart[r] = first position of read r (its bases, then
// one separator), pstart[nreads] = P.
__global__ void k_pack_reads(const unsigned char *__restrict__ bases,
                             const u64 *__restrict__ offsets, const u64 *__restrict__ pstart,
                             u32 nreads, u64 nw, u64 *__restrict__ W, u32 *__restrict__ M) {
  u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nw) return;
  u64 P = pstart[nreads];
  u64 p = t * 32;
  u32 lo = 0, hi = nreads;            // last r with pstart[r] <= p
  while (hi - lo > 1) {
    u32 mid = lo + (hi - lo) / 2;
    if (pstart[mid] <= p) lo = mid; else hi = mid;
  }
  u32 r = lo;
  u64 w = 0;
  u32 m = 0;
  for (int i = 0; i < 32; i++, p++) {
    u32 c = 4;
    if (p < P) {
      while (p >= pstart[r + 1]) r++;
      u64 j = p - pstart[r];
      if (j + 1 < pstart[r + 1] - pstart[r]) c = base_code(bases[offsets[r] + j]);
    }
    w = (w << 2) | (c & 3);
    m = (m << 1) | (c >> 2);
  }
  W[t] = w;
  M[t] = m;
}

// hist[(key - lo) >> shift] += 1 for every key in [lo, hi]; nbins <= 4096.
__global__ void __launch_bounds__(256)
k_prefix_hist(const u64 *__restrict__ W, const u32 *__restrict__ M, u64 nw, u32 k,
              int canonical, u64 lo, u64 hi, u32 shift, u32 nbins, u64 *__restrict__ hist) {
  __shared__ u32 sh[1u << PLAN_BITS];
  for (u32 i = threadIdx.x; i < nbins; i += blockDim.x) sh[i] = 0;
  __syncthreads();
  for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < nw;
       t += (u64)gridDim.x * blockDim.x) {
    u64 h = W[t], l = W[t + 1];
    u64 m64 = ((u64)M[t] << 32) | M[t + 1];
    for (u32 j = 0; j < 32; j++) {
      u64 key;
      if (mer_at(h, l, m64, j, k, canonical, key) && key >= lo && key <= hi)
        atomicAdd(&sh[(u32)((key - lo) >> shift)], 1u);
    }
  }
  __syncthreads();
  for (u32 i = threadIdx.x; i < nbins; i += blockDim.x)
    if (sh[i]) atomicAdd(&hist[i], (u64)sh[i]);
}

// Exclusive prefix of v over the block (blockDim a multiple of 64, at most 1024).
// wsum: 17 words of LDS.  Every thread of the block calls it.
__device__ __forceinline__ u32 block_excl_scan(u32 v, u32 *wsum, u32 &total) {
  u32 lane = threadIdx.x & 63, w = threadIdx.x >> 6, nwv = blockDim.x >> 6;
  u32 x = v;
  for (u32 d = 1; d < 64; d <<= 1) {
    u32 y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[w] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 a = 0;
    for (u32 i = 0; i < nwv; i++) { u32 s = wsum[i]; wsum[i] = a; a += s; }
    wsum[16] = a;
  }
  __syncthreads();
  u32 r = wsum[w] + x - v;
  total = wsum[16];
  __syncthreads();
  return r;
}

// Keys of [lo, hi] into buckets (key - lo) >> bshift.  cursor[b] starts at the bucket's first
// slot in `keys` (from k_prefix_hist's counts); ncap = slots of `keys`.
__global__ void __launch_bounds__(SC_THREADS)
k_scatter(const u64 *__restrict__ W, const u32 *__restrict__ M, u64 nw, u32 k, int canonical,
          u64 lo, u64 hi, u32 bshift, u32 nb, u32 *__restrict__ cursor, u64 *__restrict__ keys,
          u32 ncap, u32 *__restrict__ errflag) {
  extern __shared__ __align__(16) unsigned char smem[];
  u64 *tk = reinterpret_cast<u64 *>(smem);
  unsigned short *perm = reinterpret_cast<unsigned short *>(smem + SC_TILE * 8);
  u32 *cnt = reinterpret_cast<u32 *>(smem + SC_TILE * 8 + SC_TILE * 2);
  u32 *loff = cnt + NB_MAX;
  u32 *gbase = loff + NB_MAX;
  u32 *wsum = gbase + NB_MAX;          // 17
  u32 *fill = wsum + 20;
  const u32 tid = threadIdx.x, lane = tid & 63;
  const u32 per = (nb + SC_THREADS - 1) / SC_THREADS;   // buckets a thread owns in the scan
  if (tid == 0) *fill = 0;
  __syncthreads();
  const u64 nchunks = (nw + SC_CHUNK_WORDS - 1) / SC_CHUNK_WORDS;
  for (u64 c = blockIdx.x;; c += gridDim.x) {
    const bool more = c < nchunks;
    if (more) {
      u64 t = c * SC_CHUNK_WORDS + tid / 4;
      u32 j0 = (tid & 3) * SC_PER_THREAD;
      bool live = t < nw;
      u64 h = 0, l = 0, m64 = ~0ull;
      if (live) {
        h = W[t];
        l = W[t + 1];
        m64 = ((u64)M[t] << 32) | M[t + 1];
      }
      for (u32 j = 0; j < SC_PER_THREAD; j++) {
        u64 key = 0;
        bool in = live && mer_at(h, l, m64, j0 + j, k, canonical, key) && key >= lo && key <= hi;
        u64 bm = __ballot(in);
        u32 base = 0;
        if (lane == 0 && bm) base = atomicAdd(fill, (u32)__popcll(bm));
        base = __shfl(base, 0);
        if (in) tk[base + __popcll(bm & ((1ull << lane) - 1))] = key;
      }
    }
    __syncthreads();
    const u32 T = *fill;
    __syncthreads();                     // everyone has T before the next chunk adds to it
    if (more && T <= SC_TILE - SC_CHUNK_WORDS * 32) continue;   // room for one more chunk
    if (T) {
      // order the tile by bucket, then write each bucket's run with consecutive lanes
      for (u32 i = tid; i < nb; i += SC_THREADS) cnt[i] = 0;
      __syncthreads();
      for (u32 i = tid; i < T; i += SC_THREADS) atomicAdd(&cnt[(u32)((tk[i] - lo) >> bshift)], 1u);
      __syncthreads();
      u32 mine = 0;
      for (u32 b = tid * per; b < min(nb, (tid + 1) * per); b++) mine += cnt[b];
      u32 total;
      u32 at = block_excl_scan(mine, wsum, total);
      for (u32 b = tid * per; b < min(nb, (tid + 1) * per); b++) {
        u32 n = cnt[b];
        loff[b] = at;
        at += n;
        if (n) gbase[b] = atomicAdd(&cursor[b], n);
        cnt[b] = 0;
      }
      __syncthreads();
      for (u32 i = tid; i < T; i += SC_THREADS) {
        u32 b = (u32)((tk[i] - lo) >> bshift);
        perm[loff[b] + atomicAdd(&cnt[b], 1u)] = (unsigned short)i;
      }
      __syncthreads();
      for (u32 j = tid; j < T; j += SC_THREADS) {
        u64 key = tk[perm[j]];
        u32 b = (u32)((key - lo) >> bshift);
        u32 dst = gbase[b] + (j - loff[b]);
        if (dst < ncap) keys[dst] = key; else *errflag = 1;
      }
      __syncthreads();
      if (tid == 0) *fill = 0;
      __syncthreads();
    }
    if (!more) break;
  }
}

struct FineArgs {
  const u64 *keys;
  const u32 *bstart;     // nb + 1
  u64 lo, hi;
  u32 bshift, low_count;
  u64 *outm;
  u32 *outc;
  u32 *nk;               // kept entries per bucket
  u64 *hist;             // dense entries
  u32 *ovf;              // ovcap counts >= dense
  u32 *ovn;
  u32 *oversize;
  u32 dense, ovcap;      // histogram limits in force (mer_set_histogram_limits)
};

__device__ __forceinline__ void hist_add(const FineArgs &a, u32 *hp, u32 c) {
  if (c < SMALL_HIST && c < a.dense) atomicAdd(&hp[c], 1u);
  else if (c < a.dense) atomicAdd(&a.hist[c], 1ull);
  else {
    u32 i = atomicAdd(a.ovn, 1u);
    if (i < a.ovcap) a.ovf[i] = c;
  }
}

// Sort sk[0..T), then emit (key, run length >= L) at out[obase + opos ...]; opos advances.
// Every thread of the block calls it with the same T.
__device__ void sort_emit(const FineArgs &a, u64 *sk, u32 *hp, u32 *wsum, u32 T, u32 obase,
                          u32 &opos) {
  const u32 tid = threadIdx.x;
  if (T == 0) return;
  u32 Np = 2;
  while (Np < T) Np <<= 1;
  for (u32 i = T + tid; i < Np; i += FINE_THREADS) sk[i] = ~0ull;
  __syncthreads();
  for (u32 k2 = 2; k2 <= Np; k2 <<= 1)
    for (u32 j = k2 >> 1; j > 0; j >>= 1) {
      for (u32 i = tid; i < Np; i += FINE_THREADS) {
        u32 x = i ^ j;
        if (x > i) {
          u64 p = sk[i], q = sk[x];
          bool up = (i & k2) == 0;
          if ((p > q) == up && p != q) { sk[i] = q; sk[x] = p; }
        }
      }
      __syncthreads();
    }
  for (u32 i0 = 0; i0 < T; i0 += FINE_THREADS) {
    u32 i = i0 + tid;
    u64 key = 0;
    u32 c = 0;
    if (i < T && (i == 0 || sk[i] != sk[i - 1])) {
      key = sk[i];
      u32 l = i, h = T;               // first index > i with another key, in (l, h]
      while (h - l > 1) {
        u32 mid = l + (h - l) / 2;
        if (sk[mid] == key) l = mid; else h = mid;
      }
      c = h - i;
      hist_add(a, hp, c);
    }
    bool keep = c >= a.low_count && c > 0;
    u32 total;
    u32 at = block_excl_scan(keep ? 1u : 0u, wsum, total);
    if (keep) {
      a.outm[obase + opos + at] = key;
      a.outc[obase + opos + at] = c;
    }
    opos += total;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(FINE_THREADS) k_fine(FineArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  u64 *sk = reinterpret_cast<u64 *>(smem);
  u32 *sh = reinterpret_cast<u32 *>(smem + FINE_CAP * 8);
  u32 *hp = sh + SUB_BINS;
  u32 *wsum = hp + SMALL_HIST;         // 17
  u32 *fill = wsum + 20;
  u32 *act = wsum + 21;                // 0 leaf, 1 direct, 2 narrow
  u32 *lcnt = wsum + 22;
  u64 *lhi = reinterpret_cast<u64 *>(wsum + 24);
  const u32 tid = threadIdx.x, b = blockIdx.x;
  const u32 bs = a.bstart[b], m = a.bstart[b + 1] - bs;
  for (u32 i = tid; i < SMALL_HIST; i += FINE_THREADS) hp[i] = 0;
  if (tid == 0) *fill = 0;
  __syncthreads();
  u32 opos = 0;
  if (m) {
    const u64 blo = a.lo + ((u64)b << a.bshift);
    u64 bhi = blo + ((1ull << a.bshift) - 1);
    if (bhi < blo || bhi > a.hi) bhi = a.hi;
    if (m > FINE_CAP && tid == 0) atomicAdd(a.oversize, 1u);
    if (blo == bhi) {
      // one key: its count is the bucket's size
      if (tid == 0) {
        hist_add(a, hp, m);
        if (m >= a.low_count) { a.outm[bs] = blo; a.outc[bs] = m; }
      }
      opos = m >= a.low_count ? 1 : 0;
    } else if (m <= FINE_CAP) {
      for (u32 i = tid; i < m; i += FINE_THREADS) sk[i] = a.keys[bs + i];
      __syncthreads();
      sort_emit(a, sk, hp, wsum, m, bs, opos);
    } else {
      // oversize: take the longest prefix of the remaining key range that fits the LDS sort,
      // narrowing onto the first sub-bin while that one alone does not fit
      u64 cur = blo;
      for (;;) {
        u64 l = cur, h = bhi;
        for (;;) {
          u32 s = 0;
          while (((h - l) >> s) >= SUB_BINS) s++;
          for (u32 i = tid; i < SUB_BINS; i += FINE_THREADS) sh[i] = 0;
          __syncthreads();
          for (u32 i = tid; i < m; i += FINE_THREADS) {
            u64 key = a.keys[bs + i];
            if (key >= l && key <= h) atomicAdd(&sh[(u32)((key - l) >> s)], 1u);
          }
          __syncthreads();
          if (tid == 0) {
            u32 c = 0, g = 0;
            for (; g < SUB_BINS; g++) {
              if (c + sh[g] > FINE_CAP) break;
              c += sh[g];
            }
            if (g == SUB_BINS) { *act = 0; *lhi = h; *lcnt = c; }
            else if (g >= 1) { *act = 0; *lhi = l + ((u64)g << s) - 1; *lcnt = c; }
            else if (s == 0) { *act = 1; *lhi = l; *lcnt = sh[0]; }
            else { *act = 2; *lhi = l + ((1ull << s) - 1); }
          }
          __syncthreads();
          if (*act != 2) break;
          h = *lhi;
          __syncthreads();
        }
        const u64 leaf_hi = *lhi;
        const u32 c = *lcnt, what = *act;
        __syncthreads();
        if (what == 1) {
          if (tid == 0) {
            hist_add(a, hp, c);
            if (c >= a.low_count) { a.outm[bs + opos] = l; a.outc[bs + opos] = c; }
          }
          if (c >= a.low_count) opos++;
        } else if (c) {
          for (u32 i = tid; i < m; i += FINE_THREADS) {
            u64 key = a.keys[bs + i];
            if (key >= l && key <= leaf_hi) {
              u32 slot = atomicAdd(fill, 1u);
              if (slot < FINE_CAP) sk[slot] = key;
            }
          }
          __syncthreads();
          if (tid == 0) *fill = 0;
          sort_emit(a, sk, hp, wsum, c, bs, opos);
        }
        if (leaf_hi == bhi) break;
        cur = leaf_hi + 1;
      }
    }
  }
  __syncthreads();
  if (tid == 0) a.nk[b] = opos;
  for (u32 i = tid; i < SMALL_HIST; i += FINE_THREADS)
    if (hp[i]) atomicAdd(&a.hist[i], (u64)hp[i]);
}

__global__ void k_compact(const u64 *__restrict__ outm, const u32 *__restrict__ outc,
                          const u32 *__restrict__ bstart, const u32 *__restrict__ nk,
                          const u32 *__restrict__ koff, u64 *__restrict__ cm,
                          u32 *__restrict__ cc) {
  u32 b = blockIdx.x, s = bstart[b], n = nk[b], d = koff[b];
  for (u32 i = threadIdx.x; i < n; i += blockDim.x) {
    cm[d + i] = outm[s + i];
    cc[d + i] = outc[s + i];
  }
}

// ------------------------------------------------------------------------------------ host

struct Pass {
  u64 lo, hi, n;
  bool direct;          // lo == hi, n known from the planner's histogram
};

}  // namespace

struct mer_ctx {
  mer_params P{};
  int device = -1;
  bool host_only = false;
  bool counted = false;
  u32 hist_dense = HIST_DENSE, ovf_cap = OVF_CAP;
  // device
  u64 *W = nullptr;
  u32 *M = nullptr;
  u64 nw = 0;
  u64 cur_bytes = 0, peak_bytes = 0;
  std::vector<std::pair<void *, u64>> allocs;
  mer_stats S{};
  merhost::MerDb db;
};

namespace {

int dmalloc(mer_ctx *c, void **p, u64 bytes) {
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(MER_ERR_OOM, "hipMalloc of " + std::to_string(bytes) + " bytes: " +
                                 hipGetErrorString(e));
  }
  c->allocs.push_back({*p, bytes});
  c->cur_bytes += bytes;
  c->peak_bytes = std::max(c->peak_bytes, c->cur_bytes);
  return MER_OK;
}

void dfree(mer_ctx *c, void *p) {
  if (!p) return;
  for (size_t i = 0; i < c->allocs.size(); i++)
    if (c->allocs[i].first == p) {
      c->cur_bytes -= c->allocs[i].second;
      c->allocs.erase(c->allocs.begin() + i);
      break;
    }
  (void)hipFree(p);
}

template <class T> int dalloc(mer_ctx *c, T **p, u64 n) {
  return dmalloc(c, reinterpret_cast<void **>(p), n * sizeof(T));
}

void drop_reads(mer_ctx *c) {
  dfree(c, c->W);
  dfree(c, c->M);
  c->W = nullptr;
  c->M = nullptr;
  c->nw = 0;
}

int alloc_packed(mer_ctx *c, u64 P) {
  drop_reads(c);
  c->counted = false;
  c->nw = (P + 31) / 32;
  int rc;
  if ((rc = dalloc(c, &c->W, c->nw + 1))) return rc;
  if ((rc = dalloc(c, &c->M, c->nw + 1))) return rc;
  // the word after the last: all invalid (every scan reads word t + 1)
  HIPCHK(hipMemset(c->W + c->nw, 0, 8));
  HIPCHK(hipMemset(c->M + c->nw, 0xFF, 4));
  c->S.packed_read_bytes = (c->nw + 1) * 12;
  return MER_OK;
}

u32 scan_grid(u64 nw) { return (u32)std::min<u64>(std::max<u64>((nw + 255) / 256, 1), 2048); }

int run_hist(mer_ctx *c, u64 *d_hist, u64 lo, u64 hi, u32 shift, u32 nbins,
             std::vector<u64> &out) {
  HIPCHK(hipMemset(d_hist, 0, nbins * 8));
  if (c->nw)
    k_prefix_hist<<<scan_grid(c->nw), 256>>>(c->W, c->M, c->nw, c->P.kmer_len, c->P.canonical,
                                             lo, hi, shift, nbins, d_hist);
  HIPCHK(hipGetLastError());
  out.resize(nbins);
  HIPCHK(hipMemcpy(out.data(), d_hist, nbins * 8, hipMemcpyDeviceToHost));
  return MER_OK;
}

// Cut the keys lo .. lo + 2^bits - 1 into passes of at most cap mers, ascending.
int plan_range(mer_ctx *c, u64 *d_hist, u64 lo, u32 bits, u64 cap, std::vector<Pass> &out) {
  u32 b = std::min(PLAN_BITS, bits), shift = bits - b, nbins = 1u << b;
  u64 hi = bits == 64 ? ~0ull : lo + ((1ull << bits) - 1);
  std::vector<u64> h;
  int rc = run_hist(c, d_hist, lo, hi, shift, nbins, h);
  if (rc) return rc;
  c->S.plan_scans++;
  u64 acc = 0;
  u32 first = 0;
  auto flush = [&](u32 end) {          // bins [first, end)
    if (acc) out.push_back({lo + ((u64)first << shift), lo + ((u64)(end - 1) << shift) +
                                                            ((1ull << shift) - 1), acc, false});
    acc = 0;
    first = end;
  };
  for (u32 i = 0; i < nbins; i++) {
    if (h[i] > cap) {
      flush(i);
      if (shift == 0) out.push_back({lo + i, lo + i, h[i], true});
      else if ((rc = plan_range(c, d_hist, lo + ((u64)i << shift), shift, cap, out))) return rc;
      first = i + 1;
      continue;
    }
    if (acc + h[i] > cap) flush(i);
    acc += h[i];
  }
  flush(nbins);
  return MER_OK;
}

}  // namespace

extern "C" {

void mer_params_init(mer_params *p) {
  p->kmer_len = 22;
  p->canonical = 1;
  p->low_count = 2;
  p->hbm_budget_bytes = 0;
}

const char *mer_last_error(void) { return g_err.c_str(); }
int mer_abi_version(void) { return MER_ABI_VERSION; }

int mer_ctx_create(const mer_params *p, int device, mer_ctx **out) {
  if (!p || !out) return fail(MER_ERR_BAD_PARAM, "null argument");
  if (p->kmer_len < 1 || p->kmer_len > 32)
    return fail(MER_ERR_BAD_PARAM, "kmer_len " + std::to_string(p->kmer_len) + " not in 1..32");
  if (p->low_count < 1) return fail(MER_ERR_BAD_PARAM, "low_count must be at least 1");
  if (p->hbm_budget_bytes && p->hbm_budget_bytes < MER_MIN_BUDGET_BYTES)
    return fail(MER_ERR_BAD_PARAM, "hbm_budget_bytes below MER_MIN_BUDGET_BYTES");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) {
    (void)hipGetLastError();
    return fail(MER_ERR_NO_DEVICE, "no HIP device " + std::to_string(device));
  }
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
    return fail(MER_ERR_UNSUPPORTED, std::string("device is ") + prop.gcnArchName +
                                         ", this library is built for gfx950");
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_scatter),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)SC_LDS));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fine),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)FINE_LDS));
  mer_ctx *c = new mer_ctx;
  c->P = *p;
  c->device = device;
  c->db.k = p->kmer_len;
  c->db.canonical = p->canonical ? 1 : 0;
  c->db.low_count = p->low_count;
  *out = c;
  return MER_OK;
}

void mer_ctx_destroy(mer_ctx *c) {
  if (!c) return;
  if (!c->host_only) {
    (void)hipSetDevice(c->device);
    while (!c->allocs.empty()) dfree(c, c->allocs.back().first);
  }
  delete c;
}

int mer_load_reads(mer_ctx *c, uint32_t nreads, const uint8_t *bases, const uint64_t *offsets,
                   const uint32_t *lengths) {
  if (!c || c->host_only) return fail(MER_ERR_STATE, "not a counting context");
  if (nreads && (!bases || !offsets || !lengths)) return fail(MER_ERR_BAD_PARAM, "null argument");
  HIPCHK(hipSetDevice(c->device));
  u64 P = 0;
  for (u32 r = 0; r < nreads; r++) P += (u64)lengths[r] + 1;
  int rc = alloc_packed(c, P);
  if (rc) return rc;
  if (!c->nw) return MER_OK;
  const u64 stage_n = std::min<u64>(STAGE_POSITIONS, c->nw * 32);
  unsigned char *d_stage = nullptr;
  if ((rc = dalloc(c, &d_stage, stage_n))) return rc;
  std::vector<unsigned char> stage(stage_n);
  u32 r = 0;
  u64 j = 0;                           // next position: base j of read r (j == length: separator)
  for (u64 p0 = 0; p0 < c->nw * 32; p0 += stage_n) {
    u64 n = std::min<u64>(stage_n, c->nw * 32 - p0), at = 0;
    while (at < n && r < nreads) {
      u64 left = lengths[r] - j;
      u64 take = std::min<u64>(left, n - at);
      if (take) memcpy(&stage[at], bases + offsets[r] + j, take);
      at += take;
      j += take;
      if (j == lengths[r] && at < n) { stage[at++] = 0; r++; j = 0; }
    }
    if (at < n) memset(&stage[at], 0, n - at);
    hipError_t e = hipMemcpy(d_stage, stage.data(), n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      k_pack_stage<<<(u32)((n / 32 + 255) / 256), 256>>>(d_stage, p0 / 32, n / 32, c->W, c->M);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { dfree(c, d_stage); HIPCHK(e); }
  }
  dfree(c, d_stage);
  return MER_OK;
}

int mer_load_reads_device(mer_ctx *c, uint32_t nreads, const uint8_t *d_bases,
                          const uint64_t *d_offsets, const uint32_t *lengths) {
  if (!c || c->host_only) return fail(MER_ERR_STATE, "not a counting context");
  if (nreads && (!d_bases || !d_offsets || !lengths))
    return fail(MER_ERR_BAD_PARAM, "null argument");
  HIPCHK(hipSetDevice(c->device));
  std::vector<u64> pstart((size_t)nreads + 1);
  u64 P = 0;
  for (u32 r = 0; r < nreads; r++) { pstart[r] = P; P += (u64)lengths[r] + 1; }
  pstart[nreads] = P;
  int rc = alloc_packed(c, P);
  if (rc) return rc;
  if (!c->nw) return MER_OK;
  u64 *d_ps = nullptr;
  if ((rc = dalloc(c, &d_ps, pstart.size()))) return rc;
  hipError_t e = hipMemcpy(d_ps, pstart.data(), pstart.size() * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    k_pack_reads<<<(u32)((c->nw + 255) / 256), 256>>>(d_bases, (const u64 *)d_offsets, d_ps,
                                                      nreads, c->nw, c->W, c->M);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  dfree(c, d_ps);
  HIPCHK(e);
  return MER_OK;
}

int mer_count(mer_ctx *c) {
  if (!c || c->host_only) return fail(MER_ERR_STATE, "not a counting context");
  if (!c->W) return fail(MER_ERR_STATE, "mer_count before mer_load_reads");
  HIPCHK(hipSetDevice(c->device));
  auto t0 = std::chrono::steady_clock::now();
  const u32 k = c->P.kmer_len;
  mer_stats &S = c->S;
  u64 packed = S.packed_read_bytes;
  S = mer_stats{};
  S.packed_read_bytes = packed;
  c->peak_bytes = c->cur_bytes;
  c->db.hist.clear();
  c->db.mers.clear();
  c->db.counts.clear();
  c->counted = false;

  u64 budget = c->P.hbm_budget_bytes;
  if (!budget) {
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    budget = std::max<u64>(fr / 2, MER_MIN_BUDGET_BYTES);
  }
  // a pass of n mers holds at most n / dense counts >= dense: within the overflow list
  const u64 cap = std::min<u64>({budget / PASS_BYTES_PER_KEY, (u64)NB_MAX * BUCKET_TARGET,
                                 (u64)c->hist_dense * c->ovf_cap});
  S.budget_bytes = std::min<u64>(budget, cap * PASS_BYTES_PER_KEY);

  // buffers that live for the whole count
  u64 *d_plan = nullptr, *d_hist = nullptr;
  u32 *d_cursor = nullptr, *d_bstart = nullptr, *d_nk = nullptr, *d_koff = nullptr;
  u32 *d_ovf = nullptr, *d_misc = nullptr;   // misc: ovn, oversize, errflag
  u64 *d_keys = nullptr, *d_outm = nullptr;
  u32 *d_outc = nullptr, *d_cc = nullptr;
  hipEvent_t ev[4] = {};
  int rc = MER_OK;
  auto cleanup = [&]() {
    for (void *p : {(void *)d_plan, (void *)d_hist, (void *)d_cursor, (void *)d_bstart,
                    (void *)d_nk, (void *)d_koff, (void *)d_ovf, (void *)d_misc, (void *)d_keys,
                    (void *)d_outm, (void *)d_outc, (void *)d_cc})
      dfree(c, p);
    for (auto &e : ev)
      if (e) (void)hipEventDestroy(e);
  };
#define TRY(x)                     \
  do {                             \
    if ((rc = (x))) {              \
      cleanup();                   \
      return rc;                   \
    }                              \
  } while (0)
#define TRYHIP(x)                                                                  \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      cleanup();                                                                   \
      return fail(MER_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));    \
    }                                                                              \
  } while (0)

  TRY(dalloc(c, &d_plan, 1u << PLAN_BITS));
  TRY(dalloc(c, &d_hist, HIST_DENSE));
  TRY(dalloc(c, &d_cursor, NB_MAX));
  TRY(dalloc(c, &d_bstart, NB_MAX + 1));
  TRY(dalloc(c, &d_nk, NB_MAX));
  TRY(dalloc(c, &d_koff, NB_MAX));
  TRY(dalloc(c, &d_ovf, OVF_CAP));
  TRY(dalloc(c, &d_misc, 4));
  TRYHIP(hipMemset(d_hist, 0, HIST_DENSE * 8));
  TRYHIP(hipMemset(d_misc, 0, 16));
  for (auto &e : ev) TRYHIP(hipEventCreate(&e));

  // plan
  std::vector<Pass> passes;
  TRYHIP(hipEventRecord(ev[0]));
  TRY(plan_range(c, d_plan, 0, 2 * k, cap, passes));
  TRYHIP(hipEventRecord(ev[1]));
  TRYHIP(hipEventSynchronize(ev[1]));
  float ms = 0;
  TRYHIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
  S.ms_plan = ms;

  u64 maxn = 0;
  for (auto &p : passes)
    if (!p.direct) maxn = std::max(maxn, p.n);
  if (maxn) {
    TRY(dalloc(c, &d_keys, maxn));
    TRY(dalloc(c, &d_outm, maxn));
    TRY(dalloc(c, &d_outc, maxn));
    TRY(dalloc(c, &d_cc, maxn));
  }

  std::map<u64, u64> hist;             // counts the device histogram does not hold
  std::vector<u64> hb;
  std::vector<u32> bstart, nk, koff, ov;
  for (auto &p : passes) {
    if (p.direct) {
      S.direct_keys++;
      if (p.n > 0xFFFFFFFFull) {
        cleanup();
        return fail(MER_ERR_UNSUPPORTED, "one mer occurs more than 2^32-1 times");
      }
      hist[p.n]++;
      if (p.n >= c->P.low_count) {
        c->db.mers.push_back(p.lo);
        c->db.counts.push_back((u32)p.n);
      }
      continue;
    }
    S.passes++;
    // buckets: the fewest key bits that give at most nb of them
    u32 nb = 64;
    while (nb < NB_MAX && (u64)nb * BUCKET_TARGET < p.n) nb <<= 1;
    u32 bshift = 0;
    while (((p.hi - p.lo) >> bshift) >= nb) bshift++;
    nb = (u32)((p.hi - p.lo) >> bshift) + 1;
    TRYHIP(hipEventRecord(ev[0]));
    TRY(run_hist(c, d_plan, p.lo, p.hi, bshift, nb, hb));
    bstart.assign(nb + 1, 0);
    for (u32 b = 0; b < nb; b++) bstart[b + 1] = bstart[b] + (u32)hb[b];
    if (bstart[nb] != p.n) {
      cleanup();
      return fail(MER_ERR_STATE, "pass histogram disagrees with the plan");
    }
    TRYHIP(hipMemcpy(d_bstart, bstart.data(), (nb + 1) * 4, hipMemcpyHostToDevice));
    TRYHIP(hipMemcpy(d_cursor, bstart.data(), nb * 4, hipMemcpyHostToDevice));
    u64 nchunks = (c->nw + SC_CHUNK_WORDS - 1) / SC_CHUNK_WORDS;
    k_scatter<<<(u32)std::min<u64>(nchunks, 512), SC_THREADS, SC_LDS>>>(
        c->W, c->M, c->nw, k, c->P.canonical, p.lo, p.hi, bshift, nb, d_cursor, d_keys,
        (u32)p.n, d_misc + 2);
    TRYHIP(hipGetLastError());
    TRYHIP(hipEventRecord(ev[1]));
    FineArgs fa{d_keys, d_bstart, p.lo, p.hi, bshift, c->P.low_count, d_outm, d_outc, d_nk,
                d_hist, d_ovf, d_misc, d_misc + 1, c->hist_dense, c->ovf_cap};
    k_fine<<<nb, FINE_THREADS, FINE_LDS>>>(fa);
    TRYHIP(hipGetLastError());
    nk.resize(nb);
    TRYHIP(hipMemcpy(nk.data(), d_nk, nb * 4, hipMemcpyDeviceToHost));
    // drain the overflow list: it is sized for one pass, not for the whole count
    u32 novf = 0;
    TRYHIP(hipMemcpy(&novf, d_misc, 4, hipMemcpyDeviceToHost));
    if (novf > c->ovf_cap) {
      cleanup();
      return fail(MER_ERR_STATE, "count overflow list exhausted within one pass");
    }
    if (novf) {
      ov.resize(novf);
      TRYHIP(hipMemcpy(ov.data(), d_ovf, (u64)novf * 4, hipMemcpyDeviceToHost));
      for (u32 v : ov) hist[v]++;
      S.overflow_counts += novf;
      TRYHIP(hipMemset(d_misc, 0, 4));
    }
    koff.assign(nb, 0);
    u32 kept = 0;
    for (u32 b = 0; b < nb; b++) { koff[b] = kept; kept += nk[b]; }
    TRYHIP(hipMemcpy(d_koff, koff.data(), nb * 4, hipMemcpyHostToDevice));
    // the keys are dead after k_fine: the compacted mers go over them
    k_compact<<<nb, 256>>>(d_outm, d_outc, d_bstart, d_nk, d_koff, d_keys, d_cc);
    TRYHIP(hipGetLastError());
    TRYHIP(hipEventRecord(ev[2]));
    size_t at = c->db.mers.size();
    c->db.mers.resize(at + kept);
    c->db.counts.resize(at + kept);
    if (kept) {
      TRYHIP(hipMemcpy(&c->db.mers[at], d_keys, (u64)kept * 8, hipMemcpyDeviceToHost));
      TRYHIP(hipMemcpy(&c->db.counts[at], d_cc, (u64)kept * 4, hipMemcpyDeviceToHost));
    }
    TRYHIP(hipEventSynchronize(ev[2]));
    TRYHIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    S.ms_partition += ms;
    TRYHIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
    S.ms_sort += ms;
  }

  // histogram: the dense part joins the drained overflow counts and the direct keys
  {
    std::vector<u64> dh(HIST_DENSE);
    std::vector<u32> misc(4);
    TRYHIP(hipMemcpy(dh.data(), d_hist, HIST_DENSE * 8, hipMemcpyDeviceToHost));
    TRYHIP(hipMemcpy(misc.data(), d_misc, 16, hipMemcpyDeviceToHost));
    if (misc[2]) {
      cleanup();
      return fail(MER_ERR_STATE, "scatter ran past its bucket table");
    }
    for (u32 i = 1; i < HIST_DENSE; i++)
      if (dh[i]) hist[i] += dh[i];
    S.oversize_buckets = misc[1];
  }
  c->db.hist.assign(hist.begin(), hist.end());
  merhost::finish_totals(c->db);
  S.total_mers = c->db.total;
  S.distinct_mers = c->db.distinct;
  S.unique_mers = c->db.unique;
  S.largest_count = c->db.largest;
  S.kept_mers = c->db.mers.size();
  S.peak_device_bytes = c->peak_bytes;
  cleanup();
#undef TRY
#undef TRYHIP
  S.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0)
                   .count();
  c->counted = true;
  return MER_OK;
}

int mer_get_stats(const mer_ctx *c, mer_stats *out) {
  if (!c || !out) return fail(MER_ERR_BAD_PARAM, "null argument");
  *out = c->S;
  return MER_OK;
}

int mer_set_histogram_limits(mer_ctx *c, uint32_t dense_len, uint32_t overflow_cap) {
  if (!c || c->host_only) return fail(MER_ERR_STATE, "not a counting context");
  if (dense_len < 2 || dense_len > HIST_DENSE || overflow_cap < 1 || overflow_cap > OVF_CAP ||
      (u64)dense_len * overflow_cap < MER_MIN_BUDGET_BYTES / PASS_BYTES_PER_KEY)
    return fail(MER_ERR_BAD_PARAM, "dense_len 2..65536, overflow_cap 1..4096, product >= 4096");
  c->hist_dense = dense_len;
  c->ovf_cap = overflow_cap;
  return MER_OK;
}

int mer_get_params(const mer_ctx *c, mer_params *out) {
  if (!c || !out) return fail(MER_ERR_BAD_PARAM, "null argument");
  *out = c->P;
  return MER_OK;
}

static int need_counts(const mer_ctx *c) {
  if (!c) return fail(MER_ERR_BAD_PARAM, "null context");
  if (!c->counted) return fail(MER_ERR_STATE, "no counts yet: mer_count or mer_open first");
  return MER_OK;
}

int mer_histogram(const mer_ctx *c, uint64_t *hist, uint64_t cap, uint64_t *len) {
  int rc = need_counts(c);
  if (rc) return rc;
  if (len) *len = c->db.largest + 1;
  if (hist) {
    for (u64 i = 0; i < std::min<u64>(cap, c->db.largest + 1); i++) hist[i] = 0;
    for (auto &h : c->db.hist)
      if (h.first < cap) hist[h.first] = h.second;
  }
  return MER_OK;
}

int mer_frequent(const mer_ctx *c, uint64_t min_count, uint64_t *mers, uint32_t *counts,
                 uint64_t cap, uint64_t *n) {
  int rc = need_counts(c);
  if (rc) return rc;
  u64 found = 0;
  for (size_t i = 0; i < c->db.mers.size(); i++)
    if (c->db.counts[i] >= min_count) {
      if (found < cap) {
        if (mers) mers[found] = c->db.mers[i];
        if (counts) counts[found] = c->db.counts[i];
      }
      found++;
    }
  if (n) *n = found;
  return MER_OK;
}

int mer_save(const mer_ctx *c, const char *prefix) {
  int rc = need_counts(c);
  if (rc) return rc;
  if (!prefix) return fail(MER_ERR_BAD_PARAM, "null prefix");
  std::string err;
  if (!merhost::save(c->db, prefix, err)) return fail(MER_ERR_IO, err);
  return MER_OK;
}

int mer_open(const char *prefix, mer_ctx **out) {
  if (!prefix || !out) return fail(MER_ERR_BAD_PARAM, "null argument");
  mer_ctx *c = new mer_ctx;
  std::string err;
  if (!merhost::open(prefix, c->db, err)) {
    delete c;
    return fail(MER_ERR_IO, err);
  }
  c->host_only = true;
  c->counted = true;
  c->P.kmer_len = c->db.k;
  c->P.canonical = (int)c->db.canonical;
  c->P.low_count = c->db.low_count;
  c->S.total_mers = c->db.total;
  c->S.distinct_mers = c->db.distinct;
  c->S.unique_mers = c->db.unique;
  c->S.largest_count = c->db.largest;
  c->S.kept_mers = c->db.mers.size();
  *out = c;
  return MER_OK;
}

int mer_write_histogram(const mer_ctx *c, const char *hist_path, const char *info_path) {
  int rc = need_counts(c);
  if (rc) return rc;
  FILE *h = hist_path ? fopen(hist_path, "w") : nullptr;
  FILE *i = info_path ? fopen(info_path, "w") : nullptr;
  if ((hist_path && !h) || (info_path && !i)) {
    if (h) fclose(h);
    if (i) fclose(i);
    return fail(MER_ERR_IO, std::string("cannot write ") + (hist_path && !h ? hist_path : info_path));
  }
  merhost::write_histogram(c->db, h, i);
  bool ok = true;
  if (h) ok = fclose(h) == 0 && ok;
  if (i) ok = fclose(i) == 0 && ok;
  return ok ? MER_OK : fail(MER_ERR_IO, "short write");
}

int mer_write_threshold(const mer_ctx *c, uint64_t min_count, const char *path) {
  int rc = need_counts(c);
  if (rc) return rc;
  FILE *f = path ? fopen(path, "w") : nullptr;
  if (!f) return fail(MER_ERR_IO, std::string("cannot write ") + (path ? path : "(null)"));
  merhost::write_threshold(c->db, min_count, f);
  return fclose(f) == 0 ? MER_OK : fail(MER_ERR_IO, "short write");
}

}  // extern "C"
