// gfa.hip -- libcanu_gfa.so: canu's alignGFA (src/gfa/alignGFA.C) on gfx950.  include/canu_gfa.h
// says what is reproduced; this is how.
//
//   k_gfa_hw     one wave per alignment: edlib's EDLIB_MODE_HW / EDLIB_TASK_LOC result
//                (edlib_wave.h's wave_locate), with the start only where the caller needs it.
//                It serves checkLink's two extension steps (one launch each, all links
//                together) and every round of checkRecord_align's loop (one launch per round
//                over the calls still open).
//   k_gfa_path   one wave per link: the global distance, then -- within 2 * maxEdit --
//                obtainAlignment's recursion (edlib_wave.h's wave_path, leaves under
//                GFA_LEAF_BYTES).  Its operations become CIGAR runs 64 at a time with ballots;
//                a run that crosses a chunk or a leaf is carried in the wave's state.  Per-base
//                operations never leave the device.
//
// An oriented tig is never copied: a span of a reversed tig is read backwards through the
// complement, with N as a sixth symbol (the NUL of reverseComplementCopy) that equals only
// itself.  The host's part of a link or record is the reference's double arithmetic
// (gfa_host.h) between the launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/canu_gfa.h"
#include "capi_common.h"
#include "edlib_launch.h"
#include "gfa_host.h"

namespace {

using capi::fail;
using edw::CODE_NUL;
using edw::LDS_WORDS;
using edw::OP_DELETE;
using edw::OP_INSERT;
using edw::OP_MATCH;
using edw::STACK_DEPTH;
using edw::uni;
using edw::WAVES_PER_BLOCK;

CAPI_SAME_CODES(GFA);

struct Span {                // a stretch of a tig, in the tig's own coordinates
  uint64_t off;              // its first byte in the set's array
  int32_t n;
  uint32_t flags;            // bit 0: read as the reverse complement; bit 1: GFA_SET_C
};

struct HwJob {
  Span q, t;
  int32_t k;
  int32_t need_start;
};

struct HwOut {
  int32_t dist, start, end;  // dist -1: nothing within k
  int32_t pad;
  unsigned long long cells;
};

struct NwJob {
  Span q, t;
  int32_t k;
  uint32_t run_cap;
  uint64_t run_off;
};

struct NwOut {
  int32_t dist, align_len;
  uint32_t n_runs, n_leaf, n_split, pad;
  unsigned long long cells;
};

// ------------------------------------------------------------------ the spans

struct Seq {                 // a span as the aligner reads it
  const uint8_t *p;
  int n;
  int rev;                   // element i is p[n-1-i]
  int comp;                  // through reverseComplementCopy's table: ACGT complemented, N -> NUL
  __device__ __forceinline__ int at(int i) const {
    const int c = p[rev ? n - 1 - i : i];
    return comp ? (c < 4 ? 3 - c : CODE_NUL) : c;
  }
};

struct Ori {                 // an oriented span: element i of it is at(i) of fwd()
  const uint8_t *p;
  int n;
  int rc;
  __device__ __forceinline__ Seq fwd() const { return Seq{p, n, rc, rc}; }
  __device__ __forceinline__ Seq bwd() const { return Seq{p, n, !rc, rc}; }
  __device__ __forceinline__ Ori sub(int o, int len) const {
    return Ori{rc ? p + (n - o - len) : p + o, len, rc};
  }
};

__device__ __forceinline__ Ori ori_of(const Span s, const uint8_t *tigT, const uint8_t *tigC) {
  return Ori{((s.flags & 2u) ? tigC : tigT) + s.off, s.n, (int)(s.flags & 1u)};
}

// ------------------------------------------------------------------ the location

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK)
void k_gfa_hw(const uint8_t *__restrict__ tigT, const uint8_t *__restrict__ tigC,
              const HwJob *__restrict__ jobs, const uint32_t n_jobs, HwOut *__restrict__ out,
              uint32_t *__restrict__ scratch, const uint64_t scratch_words) {
  __shared__ uint32_t s_row[WAVES_PER_BLOCK][LDS_WORDS];
  const int lane = threadIdx.x & 63;
  const int wave = uni((int)(threadIdx.x >> 6));
  const uint64_t gw = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave;
  const uint32_t n_waves = gridDim.x * WAVES_PER_BLOCK;
  uint32_t *grow = scratch ? scratch + gw * scratch_words : nullptr;
  for (uint32_t e = (uint32_t)gw; e < n_jobs; e += n_waves) {
    const HwJob jb = jobs[e];
    const edw::Located L = edw::wave_locate<6>(ori_of(jb.q, tigT, tigC), ori_of(jb.t, tigT, tigC),
                                               uni(jb.k), uni(jb.need_start) != 0, s_row[wave], grow);
    HwOut o{-1, 0, 0, 0, L.cells};
    if (L.ok) {
      o.dist = L.dist;
      o.start = L.start;
      o.end = L.end;
    }
    if (lane == 0) out[e] = o;
  }
}

// ------------------------------------------------------------------ the path and its runs

struct RunState {            // the run still open, the same in every lane
  int cls;                   // 0 M, 1 I, 2 D; -1 before the first operation
  uint32_t cnt;
  uint32_t nruns;            // runs closed
  uint32_t total;            // operations seen
};

__device__ __forceinline__ uint32_t run_op(int cls) { return cls == 0 ? 'M' : cls == 1 ? 'I' : 'D'; }

// `count` operations in alignment order -- op_at(i) in every lane -- extend the open run or
// close it and open others.  A run is written when it is closed; slots past `cap` are counted
// and not written.
template <class OpAt>
__device__ void emit_runs(RunState &S, const int count, OpAt op_at, gfa_run *__restrict__ runs,
                          const uint32_t cap) {
  const int lane = threadIdx.x & 63;
  const uint64_t lt = (1ull << lane) - 1;
  for (int c0 = 0; c0 < count; c0 += 64) {
    const int cnt = min(64, count - c0);
    const bool valid = lane < cnt;
    const int op = valid ? op_at(c0 + lane) : OP_MATCH;
    const int cls = op == OP_INSERT ? 1 : (op == OP_DELETE ? 2 : 0);
    int prev = __shfl_up(cls, 1);
    if (lane == 0) prev = S.cls;
    const bool head = valid && cls != prev;
    const uint64_t hm = __ballot(head);
    if (!hm) { S.cnt += (uint32_t)cnt; continue; }
    const int first = __ffsll((unsigned long long)hm) - 1;
    const uint32_t pend = S.cnt + (uint32_t)first;
    uint32_t base = S.nruns;
    if (pend > 0) {
      if (lane == 0 && base < cap) runs[base] = gfa_run{pend, run_op(S.cls)};
      base++;
    }
    const uint64_t above = hm & ~lt & ~(1ull << lane);
    const int next = above ? __ffsll((unsigned long long)above) - 1 : cnt;
    const int nheads = __popcll(hm);
    const int idx = __popcll(hm & lt);
    if (head && idx < nheads - 1) {
      const uint32_t at = base + (uint32_t)idx;
      if (at < cap) runs[at] = gfa_run{(uint32_t)(next - lane), run_op(cls)};
    }
    const int lastl = 63 - __clzll((long long)hm);
    S.cls = __shfl(cls, lastl);
    S.cnt = (uint32_t)(cnt - lastl);
    S.nruns = base + (uint32_t)(nheads - 1);
  }
  S.total += (uint32_t)count;
}

__global__ __launch_bounds__(64 * WAVES_PER_BLOCK)
void k_gfa_path(const uint8_t *__restrict__ tigT, const uint8_t *__restrict__ tigC,
                const NwJob *__restrict__ jobs, const uint32_t n_jobs, NwOut *__restrict__ out,
                gfa_run *__restrict__ runs_all, const edw::PathArgs scratch) {
  __shared__ uint32_t s_row[WAVES_PER_BLOCK][LDS_WORDS];
  __shared__ int s_stack[WAVES_PER_BLOCK][STACK_DEPTH][5];
  const int lane = threadIdx.x & 63;
  const int wave = uni((int)(threadIdx.x >> 6));
  const uint64_t gw = (uint64_t)blockIdx.x * WAVES_PER_BLOCK + wave;
  const uint32_t n_waves = gridDim.x * WAVES_PER_BLOCK;
  const edw::PathScratch W = scratch.wave(gw);

  for (uint32_t e = (uint32_t)gw; e < n_jobs; e += n_waves) {
    const NwJob jb = jobs[e];
    Ori Q = ori_of(jb.q, tigT, tigC), T = ori_of(jb.t, tigT, tigC);
    Q.n = uni(Q.n);
    T.n = uni(T.n);
    gfa_run *runs = runs_all + jb.run_off;
    const uint32_t cap = jb.run_cap;
    const unsigned long long c = (unsigned long long)Q.n * T.n;
    const edw::PassOut g = edw::dp_pass<6>(Q.fwd(), T.fwd(), 1, INT_MIN, s_row[wave], W.grow,
                                           edw::NoKeep{});
    const int dist = uni(g.fin);
    if (dist > uni(jb.k)) {
      if (lane == 0) out[e] = NwOut{-1, 0, 0, 0, 0, 0, c};
      continue;
    }
    RunState S{-1, 0, 0, 0};
    const edw::PathStats N = edw::wave_path<6>(
        Q, T, dist, W, s_row[wave], s_stack[wave], GFA_LEAF_BYTES,
        [&](int count, auto op_at) { emit_runs(S, count, op_at, runs, cap); });
    if (S.cnt > 0) {
      if (lane == 0 && S.nruns < cap) runs[S.nruns] = gfa_run{S.cnt, run_op(S.cls)};
      S.nruns++;
    }
    if (lane == 0) out[e] = NwOut{dist, (int32_t)S.total, S.nruns, N.nleaf, N.nsplit, 0, c + N.cells};
  }
}

}  // namespace

// ------------------------------------------------------------------ host

struct TigSet {
  uint32_t n = 0;
  bool loaded = false;
  std::vector<uint32_t> len;
  std::vector<uint64_t> off;
  DevBuf<uint8_t> d_codes;
};

struct gfa_ctx : capi::Device {
  gfa_params P{};
  TigSet sets[2];
  bool have_runs = false, have_tries = false;
  std::vector<gfa_run> runs;
  std::vector<gfa_try> tries;
  gfa_stats S{};
};

namespace {

int check_params(const gfa_params *p) {
  if (!p) return fail(GFA_ERR_BAD_PARAM, "null parameters");
  return GFA_OK;
}

uint32_t blocks_for(const gfa_ctx *c, uint64_t n_jobs) {
  const uint64_t want = (uint64_t)c->n_cu * 4 / WAVES_PER_BLOCK;
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_jobs + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK, want));
}

// A span [bgn, end) of tig `id` as it is oriented (fwd: as loaded, else its reverse complement).
Span span_of(const TigSet &ts, int which, uint32_t id, bool fwd, int32_t bgn, int32_t end) {
  const int32_t len = (int32_t)ts.len[id];
  Span s;
  s.off = ts.off[id] + (uint64_t)(fwd ? bgn : len - end);
  s.n = end - bgn;
  s.flags = (fwd ? 0u : 1u) | (which == GFA_SET_C ? 2u : 0u);
  return s;
}

// One launch of k_gfa_hw over `jobs`; `out` gets their results.
int run_hw(gfa_ctx *c, const std::vector<HwJob> &jobs, std::vector<HwOut> &out, double &ms) {
  const uint32_t n = (uint32_t)jobs.size();
  out.resize(n);
  if (!n) return GFA_OK;
  uint32_t max_t = 1;
  for (const HwJob &j : jobs) max_t = std::max<uint32_t>(max_t, (uint32_t)j.t.n);
  const uint32_t blocks = blocks_for(c, n);
  const uint64_t waves = (uint64_t)blocks * WAVES_PER_BLOCK;
  const uint64_t grow_words = edw::grow_words(max_t);
  DevBuf<HwJob> d_jobs;
  DevBuf<HwOut> d_out;
  DevBuf<uint32_t> d_grow;
  HIP_TRY(d_jobs.alloc(n));
  HIP_TRY(d_out.alloc(n));
  HIP_TRY(d_grow.alloc(grow_words * waves));
  c->S.scratch_bytes = std::max<uint64_t>(c->S.scratch_bytes, d_jobs.bytes + d_out.bytes + d_grow.bytes);
  hipStream_t s = c->stream;
  Event e0, e1;
  HIP_TRY(e0.create());
  HIP_TRY(e1.create());
  HIP_TRY(hipMemcpyAsync(d_jobs.p, jobs.data(), n * sizeof(HwJob), hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(e0, s));
  hipLaunchKernelGGL(k_gfa_hw, dim3(blocks), dim3(64 * WAVES_PER_BLOCK), 0, s, c->sets[0].d_codes.p,
                     c->sets[1].d_codes.p, d_jobs.p, n, d_out.p, grow_words ? d_grow.p : nullptr,
                     grow_words);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e1, s));
  HIP_TRY(hipMemcpyAsync(out.data(), d_out.p, n * sizeof(HwOut), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  float t = 0;
  (void)hipEventElapsedTime(&t, e0, e1);
  ms += t;
  c->S.n_rounds++;
  c->S.n_alignments += n;
  for (uint32_t i = 0; i < n; i++) {
    c->S.dp_cells += out[i].cells;
    c->S.n_passes += 1 + (out[i].dist >= 0 && jobs[i].need_start ? 1 : 0);
  }
  return GFA_OK;
}

// One launch of k_gfa_path over `jobs`, whose runs take `total_runs` slots.
int run_path(gfa_ctx *c, const std::vector<NwJob> &jobs, uint64_t total_runs, std::vector<NwOut> &out,
             std::vector<gfa_run> &runs, double &ms) {
  const uint32_t n = (uint32_t)jobs.size();
  out.resize(n);
  runs.resize(total_runs);
  if (!n) return GFA_OK;
  uint32_t max_q = 1, max_t = 1;
  for (const NwJob &j : jobs) {
    max_q = std::max<uint32_t>(max_q, (uint32_t)j.q.n);
    max_t = std::max<uint32_t>(max_t, (uint32_t)j.t.n);
  }
  const uint32_t blocks = blocks_for(c, n);
  const uint64_t waves = (uint64_t)blocks * WAVES_PER_BLOCK;
  DevBuf<NwJob> d_jobs;
  DevBuf<NwOut> d_out;
  DevBuf<gfa_run> d_runs;
  edw::PathBuffers path;
  HIP_TRY(d_jobs.alloc(n));
  HIP_TRY(d_out.alloc(n));
  HIP_TRY(d_runs.alloc(total_runs));
  HIP_TRY(path.alloc(edw::path_size(max_q, max_t, GFA_LEAF_BYTES), waves));
  c->S.scratch_bytes = std::max<uint64_t>(c->S.scratch_bytes,
                                          d_jobs.bytes + d_out.bytes + d_runs.bytes + path.bytes());
  hipStream_t s = c->stream;
  Event e0, e1;
  HIP_TRY(e0.create());
  HIP_TRY(e1.create());
  HIP_TRY(hipMemcpyAsync(d_jobs.p, jobs.data(), n * sizeof(NwJob), hipMemcpyHostToDevice, s));
  HIP_TRY(hipEventRecord(e0, s));
  hipLaunchKernelGGL(k_gfa_path, dim3(blocks), dim3(64 * WAVES_PER_BLOCK), 0, s, c->sets[0].d_codes.p,
                     c->sets[1].d_codes.p, d_jobs.p, n, d_out.p, d_runs.p, path.args());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e1, s));
  HIP_TRY(hipMemcpyAsync(out.data(), d_out.p, n * sizeof(NwOut), hipMemcpyDeviceToHost, s));
  if (total_runs)
    HIP_TRY(hipMemcpyAsync(runs.data(), d_runs.p, total_runs * sizeof(gfa_run), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  float t = 0;
  (void)hipEventElapsedTime(&t, e0, e1);
  ms += t;
  c->S.n_rounds++;
  c->S.n_alignments += n;
  for (uint32_t i = 0; i < n; i++) {
    if (out[i].n_runs > jobs[i].run_cap)
      return fail(GFA_ERR_HIP, "alignment %u made %u runs for %u slots", i, out[i].n_runs,
                  jobs[i].run_cap);
    c->S.dp_cells += out[i].cells;
    c->S.n_passes += 1 + out[i].n_leaf + 2ull * out[i].n_split;
    c->S.n_leaves += out[i].n_leaf;
    c->S.n_splits += out[i].n_split;
  }
  return GFA_OK;
}

int check_tig(const gfa_ctx *c, int which, uint32_t id, const char *what, uint64_t i) {
  const TigSet &ts = c->sets[which];
  if (id >= ts.n)
    return fail(GFA_ERR_BAD_INPUT, "%s %llu: tig %u is outside the %u tigs loaded", what,
                (unsigned long long)i, id, ts.n);
  if (ts.len[id] == 0)
    return fail(GFA_ERR_BAD_INPUT, "%s %llu: tig %u has no sequence", what, (unsigned long long)i, id);
  return GFA_OK;
}

// checkLink for links [first, last): the three launches.
int links_batch(gfa_ctx *c, const gfa_link *links, uint64_t first, uint64_t last,
                gfa_link_result *results) {
  const TigSet &ts = c->sets[GFA_SET_T];
  const uint32_t n = (uint32_t)(last - first);
  std::vector<HwJob> hw(n);
  std::vector<HwOut> ho;
  // extend B: the end of A in the begin of B
  for (uint32_t i = 0; i < n; i++) {
    const gfa_link &l = links[first + i];
    gfa_link_result &r = results[first + i];
    r = gfa_link_result{};
    r.a_len = (int32_t)ts.len[l.a_id];
    r.b_len = (int32_t)ts.len[l.b_id];
    r.max_edit = gfa_host::link_max_edit(l.align);
    r.abgn_b = gfa_host::link_abgn_b(r.a_len, l.a_align);
    r.bend_b = gfa_host::link_bend_b(r.b_len, l.b_align);
    hw[i].q = span_of(ts, GFA_SET_T, l.a_id, l.a_fwd != 0, r.abgn_b, r.a_len);
    hw[i].t = span_of(ts, GFA_SET_T, l.b_id, l.b_fwd != 0, 0, r.bend_b);
    hw[i].k = r.max_edit;
    hw[i].need_start = 0;
  }
  if (int rc = run_hw(c, hw, ho, c->S.ms_extend_b)) return rc;
  // extend A: that begin of B in the end of A
  for (uint32_t i = 0; i < n; i++) {
    const gfa_link &l = links[first + i];
    gfa_link_result &r = results[first + i];
    r.dist_b = ho[i].dist;
    r.bend = ho[i].dist >= 0 ? ho[i].end + 1 : r.bend_b;
    r.abgn_a = gfa_host::link_abgn_a(r.a_len, l.a_align);
    hw[i].q = span_of(ts, GFA_SET_T, l.b_id, l.b_fwd != 0, 0, r.bend);
    hw[i].t = span_of(ts, GFA_SET_T, l.a_id, l.a_fwd != 0, r.abgn_a, r.a_len);
    hw[i].k = r.max_edit;
    hw[i].need_start = 1;
  }
  if (int rc = run_hw(c, hw, ho, c->S.ms_extend_a)) return rc;
  // final: the two ends against each other, with the path
  std::vector<NwJob> nw(n);
  std::vector<NwOut> no;
  std::vector<gfa_run> runs;
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    const gfa_link &l = links[first + i];
    gfa_link_result &r = results[first + i];
    r.dist_a = ho[i].dist;
    r.abgn = ho[i].dist >= 0 ? r.abgn_a + ho[i].start : r.abgn_a;
    nw[i].q = span_of(ts, GFA_SET_T, l.a_id, l.a_fwd != 0, r.abgn, r.a_len);
    nw[i].t = span_of(ts, GFA_SET_T, l.b_id, l.b_fwd != 0, 0, r.bend);
    nw[i].k = 2 * r.max_edit;
    // a path of distance d has at most d runs of I or D and one more of M than that, and no
    // more runs than operations
    nw[i].run_cap = (uint32_t)std::min<uint64_t>(2ull * (uint64_t)nw[i].k + 1,
                                                 (uint64_t)nw[i].q.n + (uint64_t)nw[i].t.n);
    nw[i].run_off = total;
    total += nw[i].run_cap;
  }
  if (int rc = run_path(c, nw, total, no, runs, c->S.ms_final)) return rc;
  for (uint32_t i = 0; i < n; i++) {
    gfa_link_result &r = results[first + i];
    r.dist_f = no[i].dist;
    r.success = no[i].dist >= 0;
    r.align_len = no[i].align_len;
    r.n_runs = no[i].n_runs;
    r.run_off = c->runs.size();
    r.n_leaves = no[i].n_leaf;
    r.n_splits = no[i].n_split;
    c->runs.insert(c->runs.end(), runs.begin() + nw[i].run_off, runs.begin() + nw[i].run_off + no[i].n_runs);
  }
  c->S.n_batches++;
  return GFA_OK;
}

struct Call {                // one checkRecord_align
  uint32_t record, kind;
  Span b;                    // what is aligned
  uint32_t a_id;
  int32_t a_len, b_len;
  int32_t abgn, aend, max_edit, step;
  bool open, success;
  std::vector<gfa_try> tries;
};

int records_batch(gfa_ctx *c, const gfa_record *records, uint64_t first, uint64_t last,
                  gfa_record_result *results) {
  const TigSet &T = c->sets[GFA_SET_T], &C = c->sets[GFA_SET_C];
  std::vector<Call> calls;
  auto add = [&](uint64_t i, uint32_t kind, int32_t o, int32_t blen, int32_t abgn, int32_t aend) {
    const gfa_record &r = records[i];
    Call k{};
    k.record = (uint32_t)i;
    k.kind = kind;
    k.b = span_of(T, GFA_SET_T, r.b_id, r.b_fwd != 0, o, o + blen);
    k.a_id = r.a_id;
    k.a_len = (int32_t)C.len[r.a_id];
    k.b_len = blen;
    k.max_edit = gfa_host::rec_max_edit(blen);
    k.step = gfa_host::rec_step(blen);
    k.abgn = abgn;
    k.aend = aend;
    gfa_host::rec_window(k.a_len, blen, k.step, k.abgn, k.aend);
    k.open = true;
    calls.push_back(std::move(k));
  };
  for (uint64_t i = first; i < last; i++) {
    const gfa_record &r = records[i];
    const int32_t blen = (int32_t)T.len[r.b_id];
    if (blen < GFA_END_BASES) {
      add(i, GFA_CALL_ALL, 0, blen, r.bgn, r.end);
    } else {
      add(i, GFA_CALL_LEFT, 0, GFA_END_BASES, r.bgn, r.bgn + GFA_END_BASES);
      add(i, GFA_CALL_RIGHT, blen - GFA_END_BASES, GFA_END_BASES, r.end - GFA_END_BASES, r.end);
    }
  }
  std::vector<HwJob> hw;
  std::vector<HwOut> ho;
  std::vector<size_t> who;
  while (true) {
    hw.clear();
    who.clear();
    for (size_t k = 0; k < calls.size(); k++) {
      const Call &K = calls[k];
      if (!K.open) continue;
      HwJob j;
      j.q = K.b;
      j.t = span_of(C, GFA_SET_C, K.a_id, true, K.abgn, K.aend);
      j.k = K.max_edit;
      j.need_start = 1;
      hw.push_back(j);
      who.push_back(k);
    }
    if (hw.empty()) break;
    if (int rc = run_hw(c, hw, ho, c->S.ms_records)) return rc;
    for (size_t x = 0; x < who.size(); x++) {
      Call &K = calls[who[x]];
      gfa_try t{};
      t.record = K.record;
      t.call = K.kind;
      t.b_len = K.b_len;
      t.abgn = K.abgn;
      t.aend = K.aend;
      t.max_edit = K.max_edit;
      t.dist = ho[x].dist;
      if (ho[x].dist >= 0) {
        t.nbgn = K.abgn + ho[x].start;
        t.nend = K.abgn + ho[x].end + 1;
        if (gfa_host::rec_accept(K.abgn, K.aend, t.nbgn, t.nend, K.a_len)) {
          t.outcome = GFA_TRY_ACCEPT;
          K.abgn = t.nbgn;
          K.aend = t.nend;
          K.open = false;
          K.success = true;
        } else {
          t.outcome = GFA_TRY_EXTEND;
          if (K.abgn == t.nbgn) K.abgn = std::max(K.abgn - K.step, 0);
          if (K.aend == t.nend) K.aend = std::min(K.aend + K.step, K.a_len);
        }
      } else if (gfa_host::rec_can_relax(K.abgn, K.aend, K.b_len, K.max_edit)) {
        t.outcome = GFA_TRY_RELAX;
        K.abgn = std::max(K.abgn - K.step, 0);
        K.aend = std::min(K.aend + K.step, K.a_len);
        K.max_edit = gfa_host::rec_relax(K.max_edit);
      } else {
        t.outcome = GFA_TRY_ABORT;
        K.open = false;
      }
      K.tries.push_back(t);
    }
  }
  size_t k = 0;
  for (uint64_t i = first; i < last; i++) {
    gfa_record_result &r = results[i];
    r = gfa_record_result{};
    r.try_off = c->tries.size();
    bool ok = true;
    int32_t bgn = records[i].bgn, end = records[i].end;
    const size_t k0 = k;
    for (; k < calls.size() && calls[k].record == (uint32_t)i; k++) {
      ok = ok && calls[k].success;
      c->tries.insert(c->tries.end(), calls[k].tries.begin(), calls[k].tries.end());
    }
    if (ok) {
      bgn = calls[k0].abgn;          // ALL's, or LEFT's begin and RIGHT's end
      end = calls[k - 1].aend;
    }
    r.success = ok;
    r.bgn = bgn;
    r.end = end;
    r.n_tries = (uint32_t)(c->tries.size() - r.try_off);
  }
  c->S.n_batches++;
  return GFA_OK;
}

}  // namespace

extern "C" {

void gfa_params_init(gfa_params *p) {
  if (!p) return;
  p->hbm_budget = 0;
}

const char *gfa_last_error(void) { return capi::g_err.c_str(); }
int gfa_abi_version(void) { return GFA_ABI_VERSION; }

int gfa_ctx_create(const gfa_params *p, int device, gfa_ctx **out) {
  if (!out) return fail(GFA_ERR_BAD_PARAM, "null out");
  *out = nullptr;
  if (int rc = check_params(p)) return rc;
  return capi::create_ctx(p, device, out);
}

void gfa_ctx_destroy(gfa_ctx *c) { capi::destroy_ctx(c); }

int gfa_set_params(gfa_ctx *c, const gfa_params *p) {
  if (!c) return fail(GFA_ERR_BAD_PARAM, "null context");
  if (int rc = check_params(p)) return rc;
  c->P = *p;
  return GFA_OK;
}

int gfa_load_tigs(gfa_ctx *c, int which, uint32_t n, const uint8_t *bases, const uint64_t *offsets,
                  const uint32_t *lengths) {
  if (!c) return fail(GFA_ERR_BAD_PARAM, "null context");
  if (which != GFA_SET_T && which != GFA_SET_C)
    return fail(GFA_ERR_BAD_PARAM, "tig set %d is neither GFA_SET_T nor GFA_SET_C", which);
  TigSet &ts = c->sets[which];
  ts.d_codes.release();
  ts.n = 0;
  ts.loaded = false;
  ts.len.clear();
  ts.off.clear();
  c->have_runs = c->have_tries = false;
  std::vector<uint64_t> off(n);
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (lengths && lengths[i] > GFA_MAX_TIGLEN)
      return fail(GFA_ERR_UNSUPPORTED, "tig %u is %u bases, beyond %u", i, lengths[i],
                  (unsigned)GFA_MAX_TIGLEN);
    off[i] = total;
    total += lengths ? lengths[i] : 0;
  }
  DevBuf<uint8_t> d_b;
  DevBuf<uint64_t> d_o, d_off;
  DevBuf<uint32_t> bad, d_len;
  if (int rc = capi::stage_reads(c->device, n, bases, offsets, lengths, d_b, d_o)) return rc;
  HIP_TRY(bad.alloc(1));
  HIP_TRY(d_len.alloc(n));
  HIP_TRY(d_off.alloc(n));
  HIP_TRY(ts.d_codes.alloc(total));
  HIP_TRY(hipMemsetAsync(bad.p, 0, 4, c->stream));
  uint32_t h_bad = 0;
  if (n) {
    HIP_TRY(hipMemcpyAsync(d_off.p, off.data(), n * 8ull, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_len.p, lengths, n * 4ull, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(edw::k_encode, dim3(std::min<uint32_t>(n, 4096)), dim3(256), 0, c->stream, d_b.p,
                       d_o.p, d_off.p, d_len.p, n, ts.d_codes.p, (uint8_t *)nullptr, bad.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (h_bad) {
    ts.d_codes.release();
    return fail(GFA_ERR_BAD_INPUT, "a tig holds a byte outside ACGTN");
  }
  ts.n = n;
  ts.loaded = true;
  ts.len.assign(lengths, lengths + n);
  ts.off = off;
  return GFA_OK;
}

int gfa_check_links(gfa_ctx *c, const gfa_link *links, uint64_t n, gfa_link_result *results) {
  if (!c) return fail(GFA_ERR_BAD_PARAM, "null context");
  if (n && (!links || !results)) return fail(GFA_ERR_BAD_PARAM, "null links or results");
  if (n > 0xfffffff0ull) return fail(GFA_ERR_BAD_PARAM, "more than 2^32 links in one call");
  if (!c->sets[GFA_SET_T].loaded) return fail(GFA_ERR_STATE, "no tigs: call gfa_load_tigs first");
  HIP_TRY(hipSetDevice(c->device));
  c->have_runs = false;
  c->runs.clear();
  c->S = gfa_stats{};
  // the checks the reference leaves to its assertions
  for (uint64_t i = 0; i < n; i++) {
    const gfa_link &l = links[i];
    if (int rc = check_tig(c, GFA_SET_T, l.a_id, "link", i)) return rc;
    if (int rc = check_tig(c, GFA_SET_T, l.b_id, "link", i)) return rc;
    if (l.a_align <= 0 || l.b_align <= 0 || l.align < 0)
      return fail(GFA_ERR_BAD_INPUT, "link %llu: an alignment of %d and %d bases (%d columns) "
                  "leaves nothing to align", (unsigned long long)i, l.a_align, l.b_align, l.align);
  }
  c->S.n_links = n;
  const uint64_t budget = c->P.hbm_budget ? c->P.hbm_budget : (4ull << 30);
  uint64_t i = 0;
  while (i < n) {
    const uint64_t first = i;
    uint64_t need = 0;
    for (; i < n; i++) {
      const uint64_t cap = 4ull * (uint64_t)gfa_host::link_max_edit(links[i].align) + 1;
      const uint64_t mine = cap * sizeof(gfa_run) + sizeof(NwJob) + sizeof(NwOut) + sizeof(HwJob) +
                            sizeof(HwOut);
      if (i > first && need + mine > budget) break;
      need += mine;
    }
    if (int rc = links_batch(c, links, first, i, results)) return rc;
  }
  c->have_runs = true;
  return GFA_OK;
}

int gfa_runs_size(const gfa_ctx *c, uint64_t *n_runs) {
  if (!c || !n_runs) return fail(GFA_ERR_BAD_PARAM, "null argument");
  if (!c->have_runs) return fail(GFA_ERR_STATE, "no result: call gfa_check_links first");
  *n_runs = c->runs.size();
  return GFA_OK;
}

int gfa_fetch_runs(const gfa_ctx *c, gfa_run *runs) {
  if (!c) return fail(GFA_ERR_BAD_PARAM, "null context");
  if (!c->have_runs) return fail(GFA_ERR_STATE, "no result: call gfa_check_links first");
  if (runs && !c->runs.empty()) memcpy(runs, c->runs.data(), c->runs.size() * sizeof(gfa_run));
  return GFA_OK;
}

int gfa_check_records(gfa_ctx *c, const gfa_record *records, uint64_t n, gfa_record_result *results) {
  if (!c) return fail(GFA_ERR_BAD_PARAM, "null context");
  if (n && (!records || !results)) return fail(GFA_ERR_BAD_PARAM, "null records or results");
  if (n > 0x7ffffff0ull) return fail(GFA_ERR_BAD_PARAM, "more than 2^31 records in one call");
  if (!c->sets[GFA_SET_T].loaded || !c->sets[GFA_SET_C].loaded)
    return fail(GFA_ERR_STATE, "no tigs: call gfa_load_tigs for both sets first");
  HIP_TRY(hipSetDevice(c->device));
  c->have_tries = false;
  c->tries.clear();
  c->S = gfa_stats{};
  for (uint64_t i = 0; i < n; i++) {
    const gfa_record &r = records[i];
    if (int rc = check_tig(c, GFA_SET_C, r.a_id, "record", i)) return rc;
    if (int rc = check_tig(c, GFA_SET_T, r.b_id, "record", i)) return rc;
    const int64_t alen = c->sets[GFA_SET_C].len[r.a_id];
    if (r.bgn < 0 || r.end < r.bgn || (int64_t)r.end > alen)
      return fail(GFA_ERR_BAD_INPUT, "record %llu: %d-%d is outside contig %u of %lld bases",
                  (unsigned long long)i, r.bgn, r.end, r.a_id, (long long)alen);
  }
  c->S.n_records = n;
  const uint64_t budget = c->P.hbm_budget ? c->P.hbm_budget : (4ull << 30);
  const uint64_t per = 2 * (sizeof(HwJob) + sizeof(HwOut));
  const uint64_t step = std::max<uint64_t>(1, budget / per);
  for (uint64_t i = 0; i < n; i += step)
    if (int rc = records_batch(c, records, i, std::min(n, i + step), results)) return rc;
  c->have_tries = true;
  return GFA_OK;
}

int gfa_tries_size(const gfa_ctx *c, uint64_t *n_tries) {
  if (!c || !n_tries) return fail(GFA_ERR_BAD_PARAM, "null argument");
  if (!c->have_tries) return fail(GFA_ERR_STATE, "no result: call gfa_check_records first");
  *n_tries = c->tries.size();
  return GFA_OK;
}

int gfa_fetch_tries(const gfa_ctx *c, gfa_try *tries) {
  if (!c) return fail(GFA_ERR_BAD_PARAM, "null context");
  if (!c->have_tries) return fail(GFA_ERR_STATE, "no result: call gfa_check_records first");
  if (tries && !c->tries.empty()) memcpy(tries, c->tries.data(), c->tries.size() * sizeof(gfa_try));
  return GFA_OK;
}

int gfa_get_stats(const gfa_ctx *c, gfa_stats *out) {
  if (!c || !out) return fail(GFA_ERR_BAD_PARAM, "null argument");
  *out = c->S;
  return GFA_OK;
}

}  // extern "C"
