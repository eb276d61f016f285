// ai_ground_planes: one RANSAC ground plane per scan of a map in one call -- the open3d branch of aggregate_pointcloud
// (pipeline/utils/point_cloud/aggregate_pointcloud.py:115-123: segment_plane(distance_threshold=0.4, ransac_n=3,
// num_iterations=2000)) with a counter-based sampler, so that the result is a function of (points, seed, scan key) alone.  The
// rules (G1-G7) are in include/autoinst_hip.h and DESIGN.md section 18.
//
//   kg_keep        every point's kept flag (rules A1 and A2 through ai_keep.h);
//   (scan)         exclusive scan of the flags: a kept point's rank in the map, and with it in its scan;
//   kg_compact     rank -> input position (the sampler needs it);
//   kg_hypotheses  one thread per (scan, hypothesis): the three ranks (G2), the plane (G3) or a degenerate mark;
//   kg_score       one hypothesis per thread: a block owns GR_HYPS hypotheses of one scan and a slab of GR_SLAB of its input points,
//                  staged in LDS as float64 (NaN for a point that is not kept, so that G4 drops it without a branch).  Every lane
//                  reads the same point (a broadcast LDS read), tests it against its own plane in registers and counts; one
//                  atomicAdd per thread and slab.  No cross-lane reduction;
//   kg_choose      one block per scan: the largest count, ties to the smallest hypothesis (G5);
//   kg_flags       the per-point flags from the chosen plane, by the expression kg_score counted with (G6).
//
// Counts are integers added with integer atomics: nothing depends on the order in which blocks run (G7).
#include <cmath>

#include "ai_entry.h"
#include "ai_keep.h"

namespace {

#define GR_SLAB 1024           // input points per kg_score block: 24 KiB of LDS as float64
#define GR_HYPS AI_BLOCK       // hypotheses per kg_score block, one per thread
#define GR_MAX_HYP 4096

struct GRIn {
  const float* xyz;        // M x 3
  const uint32_t* word;    // M, or null
  int64_t n;               // M
  AIKeep keep;
};

__device__ __forceinline__ bool gr_kept(const GRIn& a, int64_t i, float& x, float& y, float& z) {
  x = a.xyz[i * 3];
  y = a.xyz[i * 3 + 1];
  z = a.xyz[i * 3 + 2];
  return ai_keep_point(a.keep, x, y, z, a.word ? a.word[i] : 0u);
}

// G4: the distance of a point from a plane, every step rounded on its own
__device__ __forceinline__ double gr_dist(double a, double b, double c, double d, double x, double y, double z) {
#pragma clang fp contract(off)
  return fabs(((a * x + b * y) + c * z) + d);
}

// G2: the generator's word for counter c
__device__ __forceinline__ uint64_t gr_mix(uint64_t seed, uint64_t c) {
  uint64_t z = seed + (c + 1ull) * 0x9E3779B97F4A7C15ull;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
__device__ __forceinline__ uint64_t gr_draw(uint64_t seed, uint64_t counter4, int j, uint64_t n) {
  return ((gr_mix(seed, counter4 + (uint64_t)j) >> 32) * n) >> 32;
}

__global__ __launch_bounds__(AI_BLOCK) void kg_keep(GRIn a, int32_t* __restrict__ kept) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  float x, y, z;
  kept[i] = gr_kept(a, i, x, y, z) ? 1 : 0;
}

// pre: the exclusive scan of the kept flags (M + 1 entries).  A kept point i has pre[i + 1] == pre[i] + 1.
__global__ __launch_bounds__(AI_BLOCK) void kg_compact(int64_t n, const int32_t* __restrict__ pre, int32_t* __restrict__ pos) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t r = pre[i];
  if (pre[i + 1] != r) pos[r] = (int32_t)i;   // r < the number of kept points <= M
}

// thread (s, h): plane[(s * n_hyp + h) * 4 ..] = (a, b, c, d) and hyp_count = 0, or NaNs and hyp_count = -1 for a degenerate one
__global__ __launch_bounds__(AI_BLOCK) void kg_hypotheses(GRIn a, const int64_t* __restrict__ scan_off, int32_t n_scans, int32_t n_hyp,
                                                          const int32_t* __restrict__ pre, const int32_t* __restrict__ pos,
                                                          uint64_t seed, uint64_t scan_base, double* __restrict__ plane,
                                                          int32_t* __restrict__ hyp_count) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (t >= (int64_t)n_scans * n_hyp) return;
  const int32_t s = (int32_t)(t / n_hyp), h = (int32_t)(t % n_hyp);
  const int32_t k0 = pre[scan_off[s]];
  const uint64_t m = (uint64_t)(pre[scan_off[s + 1]] - k0);
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  double pa = nan, pb = nan, pc = nan, pd = nan;
  bool ok = false;
  if (m >= 3) {
    const uint64_t c4 = (((scan_base + (uint64_t)s) * (uint64_t)GR_MAX_HYP) + (uint64_t)h) * 4ull;
    const uint64_t r0 = gr_draw(seed, c4, 0, m);
    uint64_t r1 = gr_draw(seed, c4, 1, m - 1);
    if (r1 >= r0) ++r1;
    uint64_t r2 = gr_draw(seed, c4, 2, m - 2);
    const uint64_t lo = r0 < r1 ? r0 : r1, hi = r0 < r1 ? r1 : r0;
    if (r2 >= lo) ++r2;
    if (r2 >= hi) ++r2;
    const int64_t i0 = pos[k0 + (int64_t)r0], i1 = pos[k0 + (int64_t)r1], i2 = pos[k0 + (int64_t)r2];   // ranks < m
    const double x0 = (double)a.xyz[i0 * 3], y0 = (double)a.xyz[i0 * 3 + 1], z0 = (double)a.xyz[i0 * 3 + 2];
    const double e0x = (double)a.xyz[i1 * 3] - x0, e0y = (double)a.xyz[i1 * 3 + 1] - y0, e0z = (double)a.xyz[i1 * 3 + 2] - z0;
    const double e1x = (double)a.xyz[i2 * 3] - x0, e1y = (double)a.xyz[i2 * 3 + 1] - y0, e1z = (double)a.xyz[i2 * 3 + 2] - z0;
    const double nx = (e0y * e1z) - (e0z * e1y);
    const double ny = (e0z * e1x) - (e0x * e1z);
    const double nz = (e0x * e1y) - (e0y * e1x);
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    if (len > 0.0 && len < INFINITY) {
      ok = true;
      pa = nx / len;
      pb = ny / len;
      pc = nz / len;
      pd = -((pa * x0 + pb * y0) + pc * z0);
    }
  }
  plane[t * 4] = pa;
  plane[t * 4 + 1] = pb;
  plane[t * 4 + 2] = pc;
  plane[t * 4 + 3] = pd;
  hyp_count[t] = ok ? 0 : -1;
}

// block (g, hb): slab g of the map's slabs (slab_off[s] = the slabs in front of scan s: the host's task list) and the hypotheses
// hb * GR_HYPS .. of its scan.  A degenerate hypothesis has a NaN plane: it counts nothing and its -1 stays.
__global__ __launch_bounds__(AI_BLOCK) void kg_score(GRIn a, const int64_t* __restrict__ scan_off, const int64_t* __restrict__ slab_off,
                                                     int32_t n_scans, int32_t n_hyp, double thr, const double* __restrict__ plane,
                                                     int32_t* __restrict__ hyp_count) {
  __shared__ double pts[GR_SLAB * 3];
  const int64_t g = blockIdx.x;
  const int32_t s = segment_in(slab_off, 0, n_scans - 1, g);
  const int64_t first = scan_off[s] + (g - slab_off[s]) * GR_SLAB;
  const int64_t last = min(first + (int64_t)GR_SLAB, scan_off[s + 1]);
  const int32_t cnt = (int32_t)(last - first);   // 1 .. GR_SLAB
  const double nan = __longlong_as_double(0x7FF8000000000000ll);
  for (int32_t t = threadIdx.x; t < cnt; t += AI_BLOCK) {
    float x, y, z;
    const bool k = gr_kept(a, first + t, x, y, z);
    pts[t * 3] = k ? (double)x : nan;
    pts[t * 3 + 1] = k ? (double)y : nan;
    pts[t * 3 + 2] = k ? (double)z : nan;
  }
  const int32_t h = (int32_t)blockIdx.y * GR_HYPS + (int32_t)threadIdx.x;
  const bool live = h < n_hyp;
  const int64_t q = (int64_t)s * n_hyp + (live ? h : 0);
  const double pa = live ? plane[q * 4] : nan, pb = live ? plane[q * 4 + 1] : nan, pc = live ? plane[q * 4 + 2] : nan,
               pd = live ? plane[q * 4 + 3] : nan;
  __syncthreads();
  int32_t c = 0;
#pragma unroll 4
  for (int32_t t = 0; t < cnt; ++t) c += gr_dist(pa, pb, pc, pd, pts[t * 3], pts[t * 3 + 1], pts[t * 3 + 2]) < thr ? 1 : 0;
  if (live && c > 0) atomicAdd(&hyp_count[q], c);
}

// block s: the hypothesis with the largest count, ties to the smallest index; degenerate ones (-1) never win
__global__ __launch_bounds__(AI_BLOCK) void kg_choose(int32_t n_hyp, const int32_t* __restrict__ hyp_count, const double* __restrict__ plane,
                                                      int32_t* __restrict__ best_hyp, int32_t* __restrict__ best_count,
                                                      double* __restrict__ best_plane) {
  __shared__ int32_t sc[AI_BLOCK], sh[AI_BLOCK];
  const int64_t base = (int64_t)blockIdx.x * n_hyp;
  int32_t bc = -1, bh = -1;
  for (int32_t h = threadIdx.x; h < n_hyp; h += AI_BLOCK) {   // ascending h: a later equal count does not replace an earlier one
    const int32_t c = hyp_count[base + h];
    if (c > bc) bc = c, bh = h;
  }
  sc[threadIdx.x] = bc;
  sh[threadIdx.x] = bh;
  __syncthreads();
  for (int w = AI_BLOCK / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const int32_t c = sc[threadIdx.x + w], h = sh[threadIdx.x + w];
      if (c > sc[threadIdx.x] || (c == sc[threadIdx.x] && c >= 0 && h < sh[threadIdx.x])) sc[threadIdx.x] = c, sh[threadIdx.x] = h;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int32_t h = sh[0];
    best_hyp[blockIdx.x] = h;
    best_count[blockIdx.x] = h >= 0 ? sc[0] : 0;
    for (int k = 0; k < 4; ++k) best_plane[(int64_t)blockIdx.x * 4 + k] = h >= 0 ? plane[(base + h) * 4 + k] : 0.0;
  }
}

__global__ __launch_bounds__(AI_BLOCK) void kg_flags(GRIn a, const int64_t* __restrict__ scan_off, int32_t n_scans, double thr,
                                                     const int32_t* __restrict__ best_hyp, const double* __restrict__ best_plane,
                                                     uint8_t* __restrict__ flag) {
  const int64_t first = (int64_t)blockIdx.x * AI_BLOCK, last = min(first + AI_BLOCK, a.n);
  const int32_t s_lo = segment_in(scan_off, 0, n_scans - 1, first), s_hi = segment_in(scan_off, s_lo, n_scans - 1, last - 1);
  const int64_t i = first + threadIdx.x;
  if (i >= last) return;
  const int32_t s = segment_in(scan_off, s_lo, s_hi, i);
  float x, y, z;
  uint8_t f = 0;
  if (gr_kept(a, i, x, y, z) && best_hyp[s] >= 0) {
    const double* p = best_plane + (int64_t)s * 4;
    f = gr_dist(p[0], p[1], p[2], p[3], (double)x, (double)y, (double)z) < thr ? 1 : 0;
  }
  flag[i] = f;
}

}  // namespace

extern "C" int ai_ground_planes(ai_ctx* ctx, const float* scan_xyz, const int64_t* scan_off, int32_t n_scans, const uint32_t* label_word,
                                int32_t moving_index, double range_min, double range_max, double distance_threshold, int32_t n_hyp,
                                uint64_t seed, int64_t scan_base, int mem_kind, uint8_t* ground_flag, double* plane, int32_t* best_hyp,
                                int32_t* best_count, int32_t* hyp_count) {
  const auto bad = [](const char* what) { return bad_arg("ai_ground_planes", what); };
  if (!ctx || !scan_off || n_scans < 0) return bad("null pointer or negative count");
  if (mem_kind != AI_MEM_HOST && mem_kind != AI_MEM_DEVICE) return bad("mem_kind must be AI_MEM_HOST or AI_MEM_DEVICE");
  if (scan_off[0] != 0) return bad("scan_off must start at 0");
  for (int32_t s = 0; s < n_scans; ++s)
    if (scan_off[s + 1] < scan_off[s]) return bad("scan_off is not monotone");
  const int64_t M = scan_off[n_scans];
  if (M >= ((int64_t)1 << 31) - AI_BLOCK) return bad("M must be below 2^31 - 256");
  if (!(distance_threshold > 0.0) || !std::isfinite(distance_threshold)) return bad("distance_threshold must be finite and positive");
  if (n_hyp < 1 || n_hyp > GR_MAX_HYP) return bad("n_hyp must lie in 1 .. 4096");
  if (scan_base < 0 || scan_base > ((int64_t)1 << 48) - (int64_t)n_scans) return bad("scan_base must be >= 0 and every scan key below 2^48");
  if ((int64_t)n_scans * n_hyp >= ((int64_t)1 << 31)) return bad("n_scans x n_hyp must be below 2^31");
  const AIKeep keep = ai_keep_rules(moving_index, range_min, range_max);
  if (M > 0 && keep.use_moving && !label_word) return bad("the moving-object filter needs label_word");
  if (keep.use_range && !(range_min <= range_max)) return bad("range_min must not exceed range_max (and neither may be NaN)");
  if (M > 0 && (!scan_xyz || !ground_flag)) return bad("null pointer");
  if (n_scans > 0 && (!plane || !best_hyp || !best_count)) return bad("null pointer");
  if (n_scans == 0) return AI_OK;

  // the task list of kg_score: scan s owns the slabs slab_off[s] .. slab_off[s + 1] of GR_SLAB consecutive input points each
  const size_t n_bound = (size_t)n_scans + 1;
  std::vector<int64_t> slab_off(n_bound, 0);
  for (int32_t s = 0; s < n_scans; ++s) slab_off[s + 1] = slab_off[s] + (scan_off[s + 1] - scan_off[s] + GR_SLAB - 1) / GR_SLAB;
  const int64_t n_slabs = slab_off[n_scans];
  if (n_slabs >= ((int64_t)1 << 31) - 1) return bad("too many slabs");   // (out of reach: M / 1024 + n_scans)

  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<float> own_x;
  DevBuf<uint32_t> own_w;
  DevBuf<int64_t> d_off, d_slab;
  DevBuf<int32_t> pre, pos, scan_tmp, b_hyp, b_cnt, b_hc;
  DevBuf<double> hyp_plane, b_plane;
  DevBuf<uint8_t> b_flag;
  GRIn in = {};
  in.n = M;
  in.keep = keep;
  if (M > 0) {
    AI_TRY(to_device(scan_xyz, (size_t)M * 3, mem_kind, own_x, &in.xyz, st));
    if (label_word) AI_TRY(to_device(label_word, (size_t)M, mem_kind, own_w, &in.word, st));
  }
  AI_TRY(d_off.alloc(n_bound));
  AI_TRY(d_slab.alloc(n_bound));
  AI_HIP(hipMemcpyAsync(d_off.p, scan_off, n_bound * sizeof(int64_t), hipMemcpyHostToDevice, st));
  AI_HIP(hipMemcpyAsync(d_slab.p, slab_off.data(), n_bound * sizeof(int64_t), hipMemcpyHostToDevice, st));
  const size_t n_plane = (size_t)n_scans * (size_t)n_hyp;
  uint8_t* d_flag = nullptr;
  double* d_plane = nullptr;
  int32_t *d_hyp = nullptr, *d_cnt = nullptr, *d_hc = nullptr;
  AI_TRY(dev_out(ground_flag, (size_t)M, mem_kind, b_flag, &d_flag));
  AI_TRY(dev_out(plane, (size_t)n_scans * 4, mem_kind, b_plane, &d_plane));
  AI_TRY(dev_out(best_hyp, (size_t)n_scans, mem_kind, b_hyp, &d_hyp));
  AI_TRY(dev_out(best_count, (size_t)n_scans, mem_kind, b_cnt, &d_cnt));
  AI_TRY(dev_out(hyp_count, n_plane, mem_kind, b_hc, &d_hc));
  AI_TRY(hyp_plane.alloc(n_plane * 4));
  AI_TRY(pre.alloc((size_t)M + 1));
  AI_TRY(pos.alloc((size_t)M));
  const unsigned nb = grid_for(M);
  if (M > 0) {
    AI_TRY(scan_tmp.alloc(ai_scan_tmp_elems(M)));
    hipLaunchKernelGGL(kg_keep, dim3(nb), dim3(AI_BLOCK), 0, st, in, pre.p);
    AI_KERNEL_CHECK();
    AI_TRY(ai_exclusive_scan_i32(st, pre.p, pre.p, M, scan_tmp.p));
    hipLaunchKernelGGL(kg_compact, dim3(nb), dim3(AI_BLOCK), 0, st, M, (const int32_t*)pre.p, pos.p);
    AI_KERNEL_CHECK();
  } else {
    AI_HIP(hipMemsetAsync(pre.p, 0, sizeof(int32_t), st));
  }
  hipLaunchKernelGGL(kg_hypotheses, dim3(grid_for((int64_t)n_plane)), dim3(AI_BLOCK), 0, st, in,
                     (const int64_t*)d_off.p, n_scans, n_hyp, (const int32_t*)pre.p, (const int32_t*)pos.p, seed, (uint64_t)scan_base,
                     hyp_plane.p, d_hc);
  AI_KERNEL_CHECK();
  if (n_slabs > 0) {
    hipLaunchKernelGGL(kg_score, dim3((unsigned)n_slabs, (unsigned)((n_hyp + GR_HYPS - 1) / GR_HYPS)), dim3(AI_BLOCK), 0, st, in,
                       (const int64_t*)d_off.p, (const int64_t*)d_slab.p, n_scans, n_hyp, distance_threshold,
                       (const double*)hyp_plane.p, d_hc);
    AI_KERNEL_CHECK();
  }
  hipLaunchKernelGGL(kg_choose, dim3((unsigned)n_scans), dim3(AI_BLOCK), 0, st, n_hyp, (const int32_t*)d_hc, (const double*)hyp_plane.p,
                     d_hyp, d_cnt, d_plane);
  AI_KERNEL_CHECK();
  if (M > 0) {
    hipLaunchKernelGGL(kg_flags, dim3(nb), dim3(AI_BLOCK), 0, st, in, (const int64_t*)d_off.p, n_scans, distance_threshold,
                       (const int32_t*)d_hyp, (const double*)d_plane, d_flag);
    AI_KERNEL_CHECK();
  }
  if (mem_kind != AI_MEM_DEVICE) {
    if (M > 0) AI_HIP(hipMemcpyAsync(ground_flag, d_flag, (size_t)M, hipMemcpyDeviceToHost, st));
    AI_HIP(hipMemcpyAsync(plane, d_plane, (size_t)n_scans * 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    AI_HIP(hipMemcpyAsync(best_hyp, d_hyp, (size_t)n_scans * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AI_HIP(hipMemcpyAsync(best_count, d_cnt, (size_t)n_scans * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (hyp_count) AI_HIP(hipMemcpyAsync(hyp_count, d_hc, n_plane * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  }
  AI_HIP(hipStreamSynchronize(st));
  return AI_OK;
}
