// What the label bookkeeping (ai_labels.hip) and the whole-map merge (ai_merge.hip) share: the order-preserving integer forms of a
// float64 and the kernels both use unchanged (first-occurrence flags of ai_unique_points; boxes, distinct (value, tag) entries and the
// common-scalar walk of ai_merge_associate).  The host plumbing and the sort / scan wrappers are ai_entry.h's and ai_runs.h's.
// Everything has internal linkage.
#pragma once
#include <cstring>

#include "ai_entry.h"
#include "ai_runs.h"

namespace {

// float64 -> uint64 with the same order (and -0.0 == +0.0, as np.unique compares values)
__device__ __forceinline__ uint64_t ordered_bits(double v) {
  if (v == 0.0) v = 0.0;
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b & 0x8000000000000000ull) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double from_ordered_bits(uint64_t k) {
  const uint64_t b = (k & 0x8000000000000000ull) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

__global__ __launch_bounds__(AI_BLOCK) void km_box_init(unsigned long long* __restrict__ box, int32_t n_inst) {
  const int i = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n_inst * 6) return;
  box[i] = (i % 6 < 3) ? ~0ull : 0ull;
}

__global__ __launch_bounds__(AI_BLOCK) void km_val_tag_heads(const uint64_t* __restrict__ val, const uint32_t* __restrict__ tag, int64_t n,
                                                             int32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  head[i] = (i == 0 || val[i] != val[i - 1] || tag[i] != tag[i - 1]) ? 1 : 0;
}

// distinct (value, instance) entries, compacted; every entry counts one distinct scalar of its instance
__global__ __launch_bounds__(AI_BLOCK) void km_distinct(const uint64_t* __restrict__ val, const uint32_t* __restrict__ tag,
                                                        const int32_t* __restrict__ pos, int64_t n, uint64_t* __restrict__ dval,
                                                        uint32_t* __restrict__ dtag, int32_t* __restrict__ nscal1,
                                                        int32_t* __restrict__ nscal2) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (pos[i + 1] == pos[i]) return;
  const uint32_t t = tag[i];
  dval[pos[i]] = val[i];
  dtag[pos[i]] = t;
  atomicAdd((t >> 31) ? &nscal2[t & 0x7fffffffu] : &nscal1[t], 1);
}

// a value's entries are sorted side 0 first; every side-0 entry walks to the value's side-1 entries
__global__ __launch_bounds__(AI_BLOCK) void km_common(const uint64_t* __restrict__ dval, const uint32_t* __restrict__ dtag, int64_t nd,
                                                      int32_t n2, int32_t* __restrict__ common) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= nd) return;
  const uint32_t t = dtag[i];
  if (t >> 31) return;
  const uint64_t v = dval[i];
  for (int64_t j = i + 1; j < nd && dval[j] == v; ++j) {
    const uint32_t u = dtag[j];
    if (u >> 31) atomicAdd(&common[(size_t)t * n2 + (u & 0x7fffffffu)], 1);
  }
}

// ------------------------------------------------------------------ label pairs by sorting (ai_label_pairs; the fallback of ai_label_tables)
// one uint64 per point whose unsigned order is the signed order of (a, b)
__host__ __device__ __forceinline__ uint64_t pair_key(int32_t a, int32_t b) {
  return ((uint64_t)((uint32_t)a ^ 0x80000000u) << 32) | (uint64_t)((uint32_t)b ^ 0x80000000u);
}
__host__ __device__ __forceinline__ int32_t pair_key_a(uint64_t k) { return (int32_t)((uint32_t)(k >> 32) ^ 0x80000000u); }
__host__ __device__ __forceinline__ int32_t pair_key_b(uint64_t k) { return (int32_t)((uint32_t)k ^ 0x80000000u); }

__global__ __launch_bounds__(AI_BLOCK) void kl_pair_keys(const int32_t* __restrict__ a, const int32_t* __restrict__ b, int64_t n,
                                                         uint64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  key[i] = pair_key(a[i], b[i]);
}

// one thread per sorted element: a run's head writes the run's key and start
__global__ __launch_bounds__(AI_BLOCK) void kl_pair_emit(const uint64_t* __restrict__ key, const int32_t* __restrict__ pos, int64_t n,
                                                         int32_t* __restrict__ out_a, int32_t* __restrict__ out_b,
                                                         int32_t* __restrict__ start) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (pos[i + 1] == pos[i]) return;
  const int64_t r = pos[i];
  const uint64_t k = key[i];
  out_a[r] = pair_key_a(k);
  out_b[r] = pair_key_b(k);
  start[r] = (int32_t)i;
}

// The sorted keys of n > 0 points and, per sorted position, the number of runs before it (pos[n]: the number of distinct pairs).
// Everything is queued on `st`; nothing is waited for.
struct PairRuns {
  DevBuf<uint64_t> key, skey;
  DevBuf<int32_t> pos, scan_tmp;
  DevBuf<uint8_t> tmp;
};
int sorted_pair_runs(hipStream_t st, const int32_t* da, const int32_t* db, int64_t n, PairRuns& r) {
  AI_TRY(r.key.ensure(n));
  AI_TRY(r.skey.ensure(n));
  AI_TRY(r.pos.ensure(n + 1));
  hipLaunchKernelGGL(kl_pair_keys, dim3(grid_for(n)), dim3(AI_BLOCK), 0, st, da, db, n, r.key.p);
  AI_KERNEL_CHECK();
  size_t tmp_bytes = 0;
  AI_HIP(rocprim::radix_sort_keys(nullptr, tmp_bytes, r.key.p, r.skey.p, (size_t)n, 0, 64, st));
  AI_TRY(r.tmp.ensure(tmp_bytes));
  AI_HIP(rocprim::radix_sort_keys(r.tmp.p, tmp_bytes, r.key.p, r.skey.p, (size_t)n, 0, 64, st));
  hipLaunchKernelGGL(kl_heads<uint64_t>, dim3(grid_for(n)), dim3(AI_BLOCK), 0, st, (const uint64_t*)r.skey.p, n, r.pos.p);
  AI_KERNEL_CHECK();
  AI_TRY(r.scan_tmp.ensure(ai_scan_tmp_elems(n)));
  return ai_exclusive_scan_i32(st, r.pos.p, r.pos.p, n, r.scan_tmp.p);
}

// open3d keys an unordered_map on the Eigen vector: equality by value and std::hash<double>, which maps
// -0.0 and +0.0 to the same bucket; every other pair of distinct bit patterns is a distinct point
__device__ __forceinline__ uint64_t value_bits(double v) {
  if (v == 0.0) v = 0.0;
  return (uint64_t)__double_as_longlong(v);
}

__global__ __launch_bounds__(AI_BLOCK) void ku_axis_keys(const double* __restrict__ xyz, const int32_t* __restrict__ order, int64_t n,
                                                         int axis, uint64_t* __restrict__ key) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int64_t p = order ? order[i] : i;
  key[i] = value_bits(xyz[p * 3 + axis]);
}

__global__ __launch_bounds__(AI_BLOCK) void ku_iota(int32_t* __restrict__ a, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < n) a[i] = (int32_t)i;
}

__global__ __launch_bounds__(AI_BLOCK) void ku_first_flags(const double* __restrict__ xyz, const int32_t* __restrict__ order, int64_t n,
                                                           int32_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int64_t p = order[i];
  bool first = i == 0;
  if (!first) {
    const int64_t q = order[i - 1];
#pragma unroll
    for (int a = 0; a < 3; ++a) first |= value_bits(xyz[p * 3 + a]) != value_bits(xyz[q * 3 + a]);
  }
  keep[p] = first ? 1 : 0;  // stable sorts: the first of a run is the smallest original index
}

}  // namespace
