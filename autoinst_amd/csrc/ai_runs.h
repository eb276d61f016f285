// Sorted runs, as the point-cloud entries build them: a stable rocPRIM radix sort of (key, value) pairs, the first-of-its-run flags of
// the sorted keys, the exclusive scan of flags, and what the scan is turned into -- the start of every run, or the flagged positions
// compacted.  Everything has internal linkage.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>

#include "ai_common.h"

namespace {

// stable sort by the low `bits` of the key; `tmp` is the caller's, for a caller that keeps it alive beyond the sort
template <typename K, typename V>
int sort_pairs(hipStream_t st, K* key, K* skey, V* val, V* sval, int64_t n, int bits, DevBuf<uint8_t>& tmp) {
  size_t tmp_bytes = 0;
  AI_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, key, skey, val, sval, (size_t)n, 0, bits, st));
  AI_TRY(tmp.alloc(tmp_bytes));
  AI_HIP(rocprim::radix_sort_pairs(tmp.p, tmp_bytes, key, skey, val, sval, (size_t)n, 0, bits, st));
  return AI_OK;
}

template <typename K, typename V>
int sort_pairs(hipStream_t st, K* key, K* skey, V* val, V* sval, int64_t n, int bits) {
  DevBuf<uint8_t> tmp;
  return sort_pairs(st, key, skey, val, sval, n, bits, tmp);
}

int scan_flags(hipStream_t st, int32_t* flag_to_pos, int64_t n, DevBuf<int32_t>& tmp) {
  AI_TRY(tmp.alloc(ai_scan_tmp_elems(n)));
  return ai_exclusive_scan_i32(st, flag_to_pos, flag_to_pos, n, tmp.p);
}

template <typename K>
__global__ __launch_bounds__(AI_BLOCK) void kl_heads(const K* __restrict__ key, int64_t n, int32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  head[i] = (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}

// vid = exclusive scan of the heads: start[vid[p]] = p at every head, start[m] = n
__global__ __launch_bounds__(AI_BLOCK) void kv_starts(const int32_t* __restrict__ vid, int64_t n, int32_t* __restrict__ start) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p < n && (p == 0 || vid[p + 1] != vid[p])) start[vid[p]] = (int32_t)p;
  if (p == n) start[vid[n]] = (int32_t)n;
}

// pos = exclusive scan of flags: out[pos[i]] = i at every flagged i, ascending
__global__ __launch_bounds__(AI_BLOCK) void kq_compact(const int32_t* __restrict__ pos, int64_t n, int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < n && pos[i + 1] != pos[i]) out[pos[i]] = (int32_t)i;
}

}  // namespace
