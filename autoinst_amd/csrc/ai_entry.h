// What the point-cloud entry points (preparation, finish, pooling, camera, aggregate, ground, merge, labels) share on the host side
// of one API call -- the copy of a caller's buffer to the device, an output's place on the device, the way back, launch grids, key
// bits, the bad-argument report -- and the two searches in an offset array their kernels use.  Nothing here needs rocPRIM.
// Everything has internal linkage.
#pragma once
#include "ai_common.h"

namespace {

inline unsigned grid_for(int64_t n) { return (unsigned)((n + AI_BLOCK - 1) / AI_BLOCK); }

inline int bits_for(int64_t count) {  // bits that hold 0 .. count - 1
  int b = 0;
  while (b < 63 && ((int64_t)1 << b) < count) ++b;
  return b;
}

inline int bad_arg(const char* entry, const char* what) {
  ai_set_error("%s: %s", entry, what);
  return AI_ERR_BAD_ARG;
}

// an input of the call on the device: the caller's buffer with device memory, else a copy in a buffer of the call
template <typename T>
int to_device(const T* src, size_t count, int mem_kind, DevBuf<T>& own, const T** dev, hipStream_t st) {
  if (mem_kind == AI_MEM_DEVICE) {
    *dev = src;
    return AI_OK;
  }
  AI_TRY(own.alloc(count));
  AI_HIP(hipMemcpyAsync(own.p, src, count * sizeof(T), hipMemcpyHostToDevice, st));
  *dev = own.p;
  return AI_OK;
}

template <typename T>
int upload(const std::vector<T>& h, DevBuf<T>& d, hipStream_t st) {
  AI_TRY(d.alloc(h.size()));
  if (!h.empty()) AI_HIP(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st));
  return AI_OK;
}

// an output of the call on the device: the caller's buffer with device memory, else a buffer of the call (copied back at the end)
template <typename T>
int dev_out(T* user, size_t count, int mem_kind, DevBuf<T>& own, T** dev) {
  if (mem_kind == AI_MEM_DEVICE && user) {
    *dev = user;
    return AI_OK;
  }
  AI_TRY(own.alloc(count));
  *dev = own.p;
  return AI_OK;
}

// a device buffer for one optional output of a host call: nothing (null) when the caller does not want it
template <typename T>
int dev_out_if_wanted(T* host, int64_t count, DevBuf<T>& buf, T** dev) {
  *dev = nullptr;
  if (!host) return AI_OK;
  AI_TRY(buf.alloc((size_t)count));
  *dev = buf.p;
  return AI_OK;
}

template <typename T>
int to_caller(T* dst, const T* src, size_t count, int mem_kind, hipStream_t st) {
  if (!dst || count == 0) return AI_OK;
  AI_HIP(hipMemcpyAsync(dst, src, count * sizeof(T), mem_kind == AI_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  return AI_OK;
}

// the segment of position i: the last s in [0, n) with off[s] <= i (segments without elements are passed over: their successor
// starts at the same offset)
__device__ __forceinline__ int32_t segment_of(const int64_t* __restrict__ off, int32_t n, int64_t i) {
  int32_t a = 0, b = n;  // off[a] <= i < off[b]
  while (b - a > 1) {
    const int32_t h = (a + b) >> 1;
    if (off[h] <= i)
      a = h;
    else
      b = h;
  }
  return a;
}

// the same inside a known range: the last s in [lo, hi] with off[s] <= i (off[lo] <= i)
__device__ __forceinline__ int32_t segment_in(const int64_t* __restrict__ off, int32_t lo, int32_t hi, int64_t i) {
  while (lo < hi) {
    const int32_t h = (lo + hi + 1) >> 1;
    if (off[h] <= i)
      lo = h;
    else
      hi = h - 1;
  }
  return lo;
}

}  // namespace
