// edlib_launch.h -- the host side of edlib_wave.h's aligner that allocates: both strands of the
// reads as the aligner's codes (pair.hip, fs.hip) and the path scratch of a launch's waves
// (fs.hip, gfa.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "capi_common.h"
#include "edlib_host.h"
#include "edlib_wave.h"
#include "hip_raii.h"

namespace edw {

// ------------------------------------------------------------------ the reads

struct Strands {
  DevBuf<uint8_t> fwd, rc;           // codes 0..3 = ACGT, 4 = N; read r at off[r] in both
  DevBuf<uint64_t> d_off;            // the two device tables only for the library that keeps them
  DevBuf<uint32_t> d_len;
  uint32_t first_iid = 0, nreads = 0, max_len = 0;
  std::vector<uint32_t> len;
  std::vector<uint64_t> off;
  void clear() {
    fwd.release(); rc.release(); d_off.release(); d_len.release();
    nreads = 0;
    max_len = 0;
    len.clear();
    off.clear();
  }
};

// The reads of *_load_reads_device into R, encoded on the device.  keep_tables: d_off and d_len
// outlive the call.
inline int load_strands(Strands &R, hipStream_t stream, bool keep_tables, uint32_t first_iid,
                        uint32_t nreads, const uint8_t *d_bases, const uint64_t *d_offsets,
                        const uint32_t *h_lengths) {
  R.clear();
  std::vector<uint64_t> off(nreads);
  uint64_t total = 0;
  uint32_t mx = 0;
  for (uint32_t i = 0; i < nreads; i++) {
    if (h_lengths[i] > AS_MAX_READLEN)
      return capi::fail(capi::ERR_BAD_INPUT, "read %u is %u bases, beyond AS_MAX_READLEN",
                        first_iid + i, h_lengths[i]);
    off[i] = total;
    total += h_lengths[i];
    mx = std::max(mx, h_lengths[i]);
  }
  DevBuf<uint32_t> bad;
  HIP_TRY(bad.alloc(1));
  HIP_TRY(R.fwd.alloc(total));
  HIP_TRY(R.rc.alloc(total));
  HIP_TRY(R.d_off.alloc(nreads));
  HIP_TRY(R.d_len.alloc(nreads));
  HIP_TRY(hipMemsetAsync(bad.p, 0, 4, stream));
  uint32_t h_bad = 0;
  if (nreads) {
    HIP_TRY(hipMemcpyAsync(R.d_off.p, off.data(), nreads * 8ull, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(R.d_len.p, h_lengths, nreads * 4ull, hipMemcpyHostToDevice, stream));
    const uint32_t grid = std::min<uint32_t>(nreads, 4096);
    hipLaunchKernelGGL(k_encode, dim3(grid), dim3(256), 0, stream, d_bases, d_offsets, R.d_off.p,
                       R.d_len.p, nreads, R.fwd.p, R.rc.p, bad.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, stream));
  }
  HIP_TRY(hipStreamSynchronize(stream));
  if (h_bad) {
    R.clear();
    return capi::fail(capi::ERR_BAD_INPUT, "a read holds a byte outside ACGTN");
  }
  if (!keep_tables) { R.d_off.release(); R.d_len.release(); }
  R.first_iid = first_iid;
  R.nreads = nreads;
  R.max_len = mx;
  R.len.assign(h_lengths, h_lengths + nreads);
  R.off = std::move(off);
  return capi::OK;
}

// ------------------------------------------------------------------ the path scratch

struct PathBuffers {                 // the path scratch of every wave of a launch
  DevBuf<uint64_t> colP, colM, endP, endM;
  DevBuf<int> colS, endS;
  DevBuf<uint8_t> ops;
  DevBuf<uint32_t> grow;
  PathSize Z{};

  hipError_t alloc(const PathSize &size, uint64_t waves) {
    Z = size;
    const uint64_t leaf = (uint64_t)Z.leaf_entries * waves, end = 2ull * Z.max_blocks * waves;
    hipError_t e = colP.alloc(leaf);
    if (e == hipSuccess) e = colM.alloc(leaf);
    if (e == hipSuccess) e = colS.alloc(leaf);
    if (e == hipSuccess) e = endP.alloc(end);
    if (e == hipSuccess) e = endM.alloc(end);
    if (e == hipSuccess) e = endS.alloc(end);
    if (e == hipSuccess) e = ops.alloc(Z.ops_bytes * waves);
    if (e == hipSuccess) e = grow.alloc(Z.grow_words * waves);
    return e;
  }
  uint64_t bytes() const {
    return colP.bytes + colM.bytes + colS.bytes + endP.bytes + endM.bytes + endS.bytes + ops.bytes +
           grow.bytes;
  }
  // a kernel's argument: PathArgs::wave(g) is wave g's part
  PathArgs args() const {
    return PathArgs{colP.p, colM.p, colS.p, endP.p, endM.p, endS.p, ops.p, grow.p, Z};
  }
  // the boundary rows alone, for a kernel that only locates
  uint32_t *grow_rows() const { return Z.grow_words ? grow.p : nullptr; }
};

}  // namespace edw
