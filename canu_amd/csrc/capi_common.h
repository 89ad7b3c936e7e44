// capi_common.h -- what the C APIs of fe.hip, co.hip, pair.hip, fs.hip, tr.hip and mhap.hip
// share: the last error of a thread, HIP_TRY, the opening of a gfx950 device and the staging of
// host reads.
// Each of them is one translation unit of a library of its own, so all of it is inline.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "hip_raii.h"

namespace capi {

// The status codes, which every public header names with a prefix of its own.
enum { OK = 0, ERR_NO_DEVICE = -1, ERR_BAD_PARAM = -2, ERR_UNSUPPORTED = -3, ERR_BAD_INPUT = -4,
       ERR_HIP = -5, ERR_OOM = -6, ERR_STATE = -7 };

#define CAPI_SAME_CODES(P)                                                                        \
  static_assert(P##_OK == capi::OK && P##_ERR_NO_DEVICE == capi::ERR_NO_DEVICE &&                 \
                P##_ERR_BAD_PARAM == capi::ERR_BAD_PARAM &&                                       \
                P##_ERR_UNSUPPORTED == capi::ERR_UNSUPPORTED &&                                   \
                P##_ERR_BAD_INPUT == capi::ERR_BAD_INPUT && P##_ERR_HIP == capi::ERR_HIP &&       \
                P##_ERR_OOM == capi::ERR_OOM && P##_ERR_STATE == capi::ERR_STATE,                 \
                #P " status codes differ from capi_common.h's")

inline thread_local std::string g_err;

inline int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(x)                                                                          \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess)                                                                   \
      return capi::fail(e_ == hipErrorOutOfMemory ? capi::ERR_OOM : capi::ERR_HIP, "%s: %s", \
                        #x, hipGetErrorString(e_));                                         \
  } while (0)

struct Device {              // a context derives from it
  int device = 0;
  int n_cu = 256;
  hipStream_t stream = nullptr;
};

// Device `device` if it is a gfx950, made current, with a stream of the context's own
// (stream_flags: hipStreamDefault, or hipStreamNonBlocking).
inline int open_device(int device, Device &d, unsigned stream_flags = hipStreamDefault) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(ERR_NO_DEVICE, "no HIP device %d", device);
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(ERR_NO_DEVICE, "device %d is %s, this library is built for gfx950", device,
                prop.gcnArchName);
  HIP_TRY(hipSetDevice(device));
  hipError_t e = hipStreamCreateWithFlags(&d.stream, stream_flags);
  if (e != hipSuccess) return fail(ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
  d.device = device;
  d.n_cu = prop.multiProcessorCount;
  return OK;
}

// *_ctx_create once the arguments are checked: a context on its device, with its parameters.
template <class Ctx, class Params>
int create_ctx(const Params *p, int device, Ctx **out, unsigned stream_flags = hipStreamDefault) {
  Ctx *c = new Ctx;
  if (int rc = open_device(device, *c, stream_flags)) {
    delete c;
    return rc;
  }
  c->P = *p;
  *out = c;
  return OK;
}

// *_ctx_destroy: the context's DevBufs go with it, on its device.
template <class Ctx>
void destroy_ctx(Ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// The arguments of *_load_reads_device.
inline int check_device_reads(uint32_t first_iid, uint32_t nreads, const uint8_t *d_bases,
                              const uint64_t *d_offsets, const uint32_t *h_lengths) {
  if (nreads && (!d_bases || !d_offsets || !h_lengths))
    return fail(ERR_BAD_PARAM, "null read buffers");
  if ((uint64_t)first_iid + nreads > 0xffffffffull)
    return fail(ERR_BAD_PARAM, "read IDs beyond 32 bits");
  return OK;
}

// The host half of *_load_reads: bases and offsets to the device, for *_load_reads_device.
inline int stage_reads(int device, uint32_t nreads, const uint8_t *bases, const uint64_t *offsets,
                       const uint32_t *lengths, DevBuf<uint8_t> &d_b, DevBuf<uint64_t> &d_o) {
  if (nreads && (!bases || !offsets || !lengths))
    return fail(ERR_BAD_PARAM, "null read buffers");
  HIP_TRY(hipSetDevice(device));
  uint64_t bytes = 0;
  for (uint32_t i = 0; i < nreads; i++) bytes = std::max(bytes, offsets[i] + lengths[i]);
  HIP_TRY(d_b.alloc(bytes));
  HIP_TRY(d_o.alloc(nreads));
  if (bytes) HIP_TRY(hipMemcpy(d_b.p, bases, bytes, hipMemcpyHostToDevice));
  if (nreads) HIP_TRY(hipMemcpy(d_o.p, offsets, nreads * 8ull, hipMemcpyHostToDevice));
  return OK;
}

}  // namespace capi
