// Label bookkeeping after the NCuts hot path ("next" row 4): the per-point
// parts of the scorer and of the chunk merge, as sorts / histograms on the device.  The O(#instances)
// arithmetic on top of them (IoU tables, greedy matching, AP integration) stays on the host.
//
//   ai_label_pairs      -- the contingency table every score is made of: sorted distinct (a_i, b_i)
//                          pairs with their counts.  pipeline/metrics/metrics_class.py:302-309
//                          (filter_labels: np.unique + np.where per label), :60-114 / :181-235
//                          (np.intersect1d / np.union1d of index lists per (pred, gt) pair),
//                          pipeline/metrics/modified_LSTQ.py:34-60 (np.unique of pred + gt * 2^32).
//   ai_merge_associate  -- pipeline/utils/point_cloud/point_cloud_utils.py:397-463: crop of the merged map
//                          to a cube around the new chunk, per-instance bounding boxes, number of chunk
//                          points of instance id2 inside the box of instance id1, and the reference's
//                          "union" = number of distinct scalar coordinate values of both instances
//                          (np.unique of the concatenated (K, 3) arrays WITHOUT axis flattens them).
//   ai_unique_points    -- open3d's PointCloud.remove_duplicated_points() at :489: keep the first
//                          point of every exact coordinate triple, order preserved.
//   ai_ncut_relabel     -- the labels of a map's chunks at k thresholds from their cut trees (ai_ncut_tree,
//                          DESIGN.md section 21): a boundary exists at T' iff its height < T', so a point's
//                          group is the number of existing boundaries up to its leaf.
#include <cmath>
#include <cstring>

#include "ai_labels_shared.h"

namespace {

// ------------------------------------------------------------------ merge association
struct Cube {
  double lo[3], hi[3];
};

// crop flags (:405-417, open3d's crop keeps min <= p <= max) for map points that belong to an instance
__global__ __launch_bounds__(AI_BLOCK) void km_crop(const double* __restrict__ xyz, const int32_t* __restrict__ inst, int64_t n, Cube c,
                                                    int32_t n_inst, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  const double x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
  const int32_t id = inst[i];
  flag[i] = (id > 0 && id < n_inst && x >= c.lo[0] && x <= c.hi[0] && y >= c.lo[1] && y <= c.hi[1] && z >= c.lo[2] && z <= c.hi[2]) ? 1 : 0;
}

__global__ __launch_bounds__(AI_BLOCK) void km_inst_flag(const int32_t* __restrict__ inst, int64_t n, int32_t n_inst,
                                                         int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t id = inst[i];
  flag[i] = (id > 0 && id < n_inst) ? 1 : 0;
}

// selected points -> three (value, tag) entries each; side 0 additionally feeds its instance's box
// (min / max of order-preserving integers: exact and order-independent) and point count
__global__ __launch_bounds__(AI_BLOCK) void km_scalars(const double* __restrict__ xyz, const int32_t* __restrict__ inst,
                                                       const int32_t* __restrict__ pos, int64_t n, int64_t base, uint32_t side,
                                                       uint64_t* __restrict__ val, uint32_t* __restrict__ tag,
                                                       unsigned long long* __restrict__ box, int32_t* __restrict__ npts) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (pos[i + 1] == pos[i]) return;
  const int64_t o = (base + pos[i]) * 3;
  const uint32_t id = (uint32_t)inst[i];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const uint64_t k = ordered_bits(xyz[i * 3 + a]);
    val[o + a] = k;
    tag[o + a] = (side << 31) | id;
    if (side == 0) {
      atomicMin(&box[(size_t)id * 6 + a], (unsigned long long)k);
      atomicMax(&box[(size_t)id * 6 + 3 + a], (unsigned long long)k);
    }
  }
  atomicAdd(&npts[id], 1);
}

// The (value, tag) entries -- three per selected point -- are ranked by an int32 scan over ns + 1 positions, so ns + 1 must fit
// in int32.  n_map, n_chunk < 2^29 do not ensure that: 3 * (2^29 - 1 + 2^29 - 1) > 2^31.
#define KM_MAX_SCALARS 2147483646

// :451-456  intersection = #points of instance id2 with min_bound <= p <= max_bound of instance id1
#define KM_BOX_TILE 256
__global__ __launch_bounds__(AI_BLOCK) void km_inside(const double* __restrict__ xyz, const int32_t* __restrict__ inst, int64_t n,
                                                      int32_t n1, int32_t n2, const unsigned long long* __restrict__ box,
                                                      int32_t* __restrict__ inter) {
  __shared__ double sb[KM_BOX_TILE][6];
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const int32_t id2 = (i < n) ? inst[i] : 0;
  const bool live = id2 > 0 && id2 < n2;
  double x = 0.0, y = 0.0, z = 0.0;
  if (live) {
    x = xyz[i * 3];
    y = xyz[i * 3 + 1];
    z = xyz[i * 3 + 2];
  }
  for (int32_t b0 = 1; b0 < n1; b0 += KM_BOX_TILE) {
    const int32_t nb = min(KM_BOX_TILE, n1 - b0);
    __syncthreads();
    for (int q = threadIdx.x; q < nb * 6; q += AI_BLOCK) {
      const unsigned long long k = box[(size_t)b0 * 6 + q];
      // an instance without cropped points keeps (max, min) = (+inf-ish, -inf-ish) reversed: never inside
      sb[q / 6][q % 6] = from_ordered_bits(k);
    }
    __syncthreads();
    if (!live) continue;
    for (int32_t b = 0; b < nb; ++b)
      if (x >= sb[b][0] && x <= sb[b][3] && y >= sb[b][1] && y <= sb[b][4] && z >= sb[b][2] && z <= sb[b][5])
        atomicAdd(&inter[(size_t)(b0 + b) * n2 + id2], 1);
  }
}

// ------------------------------------------------------------------ cut tree -> labels at k thresholds
// flag[t * G + g] = 1 iff the boundary in front of group g exists at thresholds[t] (strict, as the frontier compares mcut < T)
__global__ __launch_bounds__(AI_BLOCK) void kl_height_flags(const double* __restrict__ height, int64_t G, const double* __restrict__ thr,
                                                            int32_t k, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= G * k) return;
  flag[i] = (height[i % G] < thr[i / G]) ? 1 : 0;
}

// scan = exclusive scan of the flags (k * G + 1 entries).  One thread per point: its chunk by a search of off, its label checked
// against the chunk's group count, then per threshold the existing boundaries in (first group of the chunk, its own group] -- the
// first group's own flag (height -inf: always set) is left out.  Threads [0, n_chunks) also check the head of their chunk's
// heights and count its groups.  write == 0: the checks alone (err: 1 = a label out of range, 2 = a head that is not -inf).
__global__ __launch_bounds__(AI_BLOCK) void kl_relabel(const int32_t* __restrict__ labels, const int64_t* __restrict__ off, int32_t n_chunks,
                                                       const double* __restrict__ height, const int64_t* __restrict__ goff,
                                                       const int32_t* __restrict__ scan, int64_t G, int32_t k, int64_t N, int write,
                                                       int32_t* __restrict__ labels_out, int32_t* __restrict__ counts,
                                                       int32_t* __restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < n_chunks) {
    const int64_t g0 = goff[i], g1 = goff[i + 1];
    if (!write) {
      if (g1 > g0 && height[g0] != -INFINITY) atomicOr(err, 2);
    } else {
      for (int32_t t = 0; t < k; ++t) counts[(int64_t)t * n_chunks + i] = (g1 > g0) ? scan[t * G + g1] - scan[t * G + g0 + 1] + 1 : 0;
    }
  }
  if (i >= N) return;
  const int32_t c = segment_of(off, n_chunks, i);
  const int64_t g0 = goff[c], ng = goff[c + 1] - g0;
  const int32_t l = labels[i];
  if (l < 0 || l >= ng) {
    if (!write) atomicOr(err, 1);
    return;
  }
  if (!write) return;
  for (int32_t t = 0; t < k; ++t) labels_out[t * N + i] = scan[t * G + g0 + l + 1] - scan[t * G + g0 + 1];
}

}  // namespace

extern "C" int ai_ncut_relabel(ai_ctx* ctx, const int32_t* labels, const int64_t* off, int32_t n_chunks, const double* cut_height,
                               const int64_t* goff, double T_max, const double* thresholds, int32_t k, int mem_kind, int32_t* labels_out,
                               int32_t* n_groups_out) {
  const char* me = "ai_ncut_relabel";
  if (!ctx || !off || !goff || !thresholds || !n_groups_out || n_chunks < 1 || (mem_kind != AI_MEM_HOST && mem_kind != AI_MEM_DEVICE))
    return bad_arg(me, "bad argument");
  if (k < 1) return bad_arg(me, "k < 1 thresholds");
  for (int32_t t = 0; t < k; ++t) {
    if (!std::isfinite(thresholds[t])) return bad_arg(me, "a threshold is NaN or infinite");
    if (!(thresholds[t] <= T_max)) return bad_arg(me, "a threshold lies above T_max: the tree holds no cut that expensive");
  }
  if (off[0] != 0 || goff[0] != 0) return bad_arg(me, "offsets do not start at 0");
  for (int32_t c = 0; c < n_chunks; ++c)
    if (off[c + 1] < off[c] || goff[c + 1] < goff[c]) return bad_arg(me, "offsets decrease");
  const int64_t N = off[n_chunks], G = goff[n_chunks];
  if (N >= ((int64_t)1 << 31) - 1 || G * k >= ((int64_t)1 << 31) - 1) return bad_arg(me, "points, or groups x thresholds, exceed the int32 range of the scan");
  if ((N > 0 && (!labels || !labels_out)) || (G > 0 && !cut_height)) return bad_arg(me, "null label / height buffer");
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<int32_t> own_l, own_out, flag, scan_tmp, d_cnt, d_err;
  DevBuf<double> own_h, d_thr;
  DevBuf<int64_t> d_off, d_goff;
  const int32_t* dl = nullptr;
  const double* dh = nullptr;
  int32_t* dout = nullptr;
  if (N > 0) AI_TRY(to_device(labels, (size_t)N, mem_kind, own_l, &dl, st));
  if (G > 0) AI_TRY(to_device(cut_height, (size_t)G, mem_kind, own_h, &dh, st));
  if (N > 0) AI_TRY(dev_out(labels_out, (size_t)N * k, mem_kind, own_out, &dout));
  AI_TRY(d_off.alloc((size_t)n_chunks + 1));
  AI_TRY(d_goff.alloc((size_t)n_chunks + 1));
  AI_TRY(d_thr.alloc((size_t)k));
  AI_HIP(hipMemcpyAsync(d_off.p, off, ((size_t)n_chunks + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  AI_HIP(hipMemcpyAsync(d_goff.p, goff, ((size_t)n_chunks + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  AI_HIP(hipMemcpyAsync(d_thr.p, thresholds, (size_t)k * sizeof(double), hipMemcpyHostToDevice, st));
  AI_TRY(flag.alloc((size_t)G * k + 1));
  AI_TRY(d_cnt.alloc((size_t)n_chunks * k));
  AI_TRY(d_err.alloc(1));
  AI_HIP(hipMemsetAsync(d_err.p, 0, sizeof(int32_t), st));
  const unsigned grid = grid_for(std::max<int64_t>(N, n_chunks));
  hipLaunchKernelGGL(kl_relabel, dim3(grid), dim3(AI_BLOCK), 0, st, dl, (const int64_t*)d_off.p, n_chunks, dh, (const int64_t*)d_goff.p,
                     (const int32_t*)nullptr, G, k, N, 0, (int32_t*)nullptr, (int32_t*)nullptr, d_err.p);
  AI_KERNEL_CHECK();
  int32_t err = 0;
  AI_HIP(hipMemcpyAsync(&err, d_err.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  if (err & 2) return bad_arg(me, "the heights of a chunk do not start with -inf");
  if (err & 1) return bad_arg(me, "a label lies outside its chunk's groups");
  if (G > 0) {
    hipLaunchKernelGGL(kl_height_flags, dim3(grid_for(G * k)), dim3(AI_BLOCK), 0, st, dh, G, (const double*)d_thr.p, k, flag.p);
    AI_KERNEL_CHECK();
  }
  AI_TRY(scan_flags(st, flag.p, G * k, scan_tmp));
  hipLaunchKernelGGL(kl_relabel, dim3(grid), dim3(AI_BLOCK), 0, st, dl, (const int64_t*)d_off.p, n_chunks, dh, (const int64_t*)d_goff.p,
                     (const int32_t*)flag.p, G, k, N, 1, dout, d_cnt.p, d_err.p);
  AI_KERNEL_CHECK();
  if (mem_kind != AI_MEM_DEVICE) AI_TRY(to_caller(labels_out, (const int32_t*)dout, (size_t)N * k, mem_kind, st));
  AI_HIP(hipMemcpyAsync(n_groups_out, d_cnt.p, (size_t)n_chunks * k * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  return AI_OK;
}

extern "C" int ai_label_pairs(ai_ctx* ctx, const int32_t* a, const int32_t* b, int64_t n, int mem_kind, int64_t cap, int32_t* pair_a,
                              int32_t* pair_b, int64_t* pair_count, int64_t* n_pairs) {
  if (!ctx || !a || !b || !n_pairs || n < 0 || n >= ((int64_t)1 << 31) - 1 || cap < 0 || (cap > 0 && (!pair_a || !pair_b || !pair_count))) {
    ai_set_error("ai_label_pairs: bad argument");
    return AI_ERR_BAD_ARG;
  }
  *n_pairs = 0;
  if (n == 0) return AI_OK;
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<int32_t> own_a, own_b, oa, ob, ostart;
  PairRuns runs;
  const int32_t *da, *db;
  AI_TRY(to_device(a, (size_t)n, mem_kind, own_a, &da, st));
  AI_TRY(to_device(b, (size_t)n, mem_kind, own_b, &db, st));
  AI_TRY(sorted_pair_runs(st, da, db, n, runs));
  DevBuf<uint64_t>& skey = runs.skey;
  DevBuf<int32_t>& pos = runs.pos;
  int32_t total = 0;
  AI_HIP(hipMemcpyAsync(&total, pos.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  *n_pairs = total;
  const int64_t m = std::min<int64_t>(total, cap);
  if (m == 0) return AI_OK;
  AI_TRY(oa.alloc(total));
  AI_TRY(ob.alloc(total));
  AI_TRY(ostart.alloc(total));
  hipLaunchKernelGGL(kl_pair_emit, dim3(grid_for(n)), dim3(AI_BLOCK), 0, st, (const uint64_t*)skey.p, (const int32_t*)pos.p, n, oa.p, ob.p,
                     ostart.p);
  AI_KERNEL_CHECK();
  // run r covers sorted positions [start[r], start[r + 1]); the last run ends at n
  std::vector<int32_t> hs((size_t)m + 1);
  const int64_t ncopy = std::min<int64_t>(m + 1, total);
  AI_HIP(hipMemcpyAsync(pair_a, oa.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipMemcpyAsync(pair_b, ob.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipMemcpyAsync(hs.data(), ostart.p, (size_t)ncopy * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  if (ncopy == m) hs[m] = (int32_t)n;
  for (int64_t r = 0; r < m; ++r) pair_count[r] = (int64_t)hs[r + 1] - hs[r];
  return AI_OK;
}

extern "C" int ai_merge_associate(ai_ctx* ctx, const double* map_xyz, const int32_t* map_inst, int64_t n_map, const double* chunk_xyz,
                                  const int32_t* chunk_inst, int64_t n_chunk, const double* center, double side_length, int32_t n_inst1,
                                  int32_t n_inst2, int mem_kind, int32_t* inter, int32_t* common, int32_t* n_scalars1,
                                  int32_t* n_scalars2, int32_t* n_points1) {
  if (!ctx || !map_xyz || !map_inst || !chunk_xyz || !chunk_inst || !center || !inter || !common || !n_scalars1 || !n_scalars2 ||
      !n_points1 || n_map <= 0 || n_chunk <= 0 || n_inst1 < 1 || n_inst2 < 1 || !(side_length > 0.0) || n_map >= ((int64_t)1 << 29) ||
      n_chunk >= ((int64_t)1 << 29) || (int64_t)n_inst1 * n_inst2 >= ((int64_t)1 << 28)) {
    ai_set_error("ai_merge_associate: bad argument");
    return AI_ERR_BAD_ARG;
  }
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<double> own_m, own_c;
  DevBuf<int32_t> own_mi, own_ci, pos1, pos2, scan_tmp, d_inter, d_common, d_ns1, d_ns2, d_np1, d_np2, head;
  DevBuf<unsigned long long> box;
  const double *dm, *dc;
  const int32_t *dmi, *dci;
  AI_TRY(to_device(map_xyz, (size_t)n_map * 3, mem_kind, own_m, &dm, st));
  AI_TRY(to_device(map_inst, (size_t)n_map, mem_kind, own_mi, &dmi, st));
  AI_TRY(to_device(chunk_xyz, (size_t)n_chunk * 3, mem_kind, own_c, &dc, st));
  AI_TRY(to_device(chunk_inst, (size_t)n_chunk, mem_kind, own_ci, &dci, st));
  Cube cube;
  for (int a = 0; a < 3; ++a) {  // :405-413  min_bound = center - side / 2, max_bound = center + side / 2
    const double half = side_length / 2.0;
    cube.lo[a] = center[a] - half;
    cube.hi[a] = center[a] + half;
  }
  const size_t n12 = (size_t)n_inst1 * n_inst2;
  AI_TRY(pos1.alloc(n_map + 1));
  AI_TRY(pos2.alloc(n_chunk + 1));
  AI_TRY(d_inter.alloc(n12));
  AI_TRY(d_common.alloc(n12));
  AI_TRY(d_ns1.alloc(n_inst1));
  AI_TRY(d_ns2.alloc(n_inst2));
  AI_TRY(d_np1.alloc(n_inst1));
  AI_TRY(d_np2.alloc(n_inst2));
  AI_TRY(box.alloc((size_t)n_inst1 * 6));
  AI_HIP(hipMemsetAsync(d_inter.p, 0, n12 * sizeof(int32_t), st));
  AI_HIP(hipMemsetAsync(d_common.p, 0, n12 * sizeof(int32_t), st));
  AI_HIP(hipMemsetAsync(d_ns1.p, 0, (size_t)n_inst1 * sizeof(int32_t), st));
  AI_HIP(hipMemsetAsync(d_ns2.p, 0, (size_t)n_inst2 * sizeof(int32_t), st));
  AI_HIP(hipMemsetAsync(d_np1.p, 0, (size_t)n_inst1 * sizeof(int32_t), st));
  AI_HIP(hipMemsetAsync(d_np2.p, 0, (size_t)n_inst2 * sizeof(int32_t), st));
  hipLaunchKernelGGL(km_box_init, dim3(grid_for((int64_t)n_inst1 * 6)), dim3(AI_BLOCK), 0, st, box.p, n_inst1);
  hipLaunchKernelGGL(km_crop, dim3(grid_for(n_map)), dim3(AI_BLOCK), 0, st, dm, dmi, n_map, cube, n_inst1, pos1.p);
  hipLaunchKernelGGL(km_inst_flag, dim3(grid_for(n_chunk)), dim3(AI_BLOCK), 0, st, dci, n_chunk, n_inst2, pos2.p);
  AI_KERNEL_CHECK();
  AI_TRY(scan_flags(st, pos1.p, n_map, scan_tmp));
  DevBuf<int32_t> scan_tmp2;
  AI_TRY(scan_flags(st, pos2.p, n_chunk, scan_tmp2));
  int32_t sel[2] = {0, 0};
  AI_HIP(hipMemcpyAsync(&sel[0], pos1.p + n_map, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipMemcpyAsync(&sel[1], pos2.p + n_chunk, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  const int64_t ns = 3 * ((int64_t)sel[0] + sel[1]);
  if (ns > KM_MAX_SCALARS) {
    ai_set_error("ai_merge_associate: %d cropped map points + %d chunk points of instances give %lld coordinate scalars, "
                 "more than the %lld that int32 positions can index",
                 sel[0], sel[1], (long long)ns, (long long)KM_MAX_SCALARS);
    return AI_ERR_BAD_ARG;
  }
  if (ns > 0) {
    DevBuf<uint64_t> val, val2, dval;
    DevBuf<uint32_t> tag, tag2, dtag;
    AI_TRY(val.alloc(ns));
    AI_TRY(val2.alloc(ns));
    AI_TRY(tag.alloc(ns));
    AI_TRY(tag2.alloc(ns));
    hipLaunchKernelGGL(km_scalars, dim3(grid_for(n_map)), dim3(AI_BLOCK), 0, st, dm, dmi, (const int32_t*)pos1.p, n_map, (int64_t)0, 0u, val.p,
                       tag.p, box.p, d_np1.p);
    hipLaunchKernelGGL(km_scalars, dim3(grid_for(n_chunk)), dim3(AI_BLOCK), 0, st, dc, dci, (const int32_t*)pos2.p, n_chunk, (int64_t)sel[0], 1u,
                       val.p, tag.p, box.p, d_np2.p);
    AI_KERNEL_CHECK();
    // order by (value, side, instance): stable sort by the tag, then by the value
    AI_TRY(sort_pairs(st, tag.p, tag2.p, val.p, val2.p, ns, 32));
    AI_TRY(sort_pairs(st, val2.p, val.p, tag2.p, tag.p, ns, 64));
    AI_TRY(head.alloc(ns + 1));
    hipLaunchKernelGGL(km_val_tag_heads, dim3(grid_for(ns)), dim3(AI_BLOCK), 0, st, (const uint64_t*)val.p, (const uint32_t*)tag.p, ns, head.p);
    AI_KERNEL_CHECK();
    DevBuf<int32_t> scan_tmp3;
    AI_TRY(scan_flags(st, head.p, ns, scan_tmp3));
    int32_t nd = 0;
    AI_HIP(hipMemcpyAsync(&nd, head.p + ns, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AI_HIP(hipStreamSynchronize(st));
    AI_TRY(dval.alloc(nd));
    AI_TRY(dtag.alloc(nd));
    hipLaunchKernelGGL(km_distinct, dim3(grid_for(ns)), dim3(AI_BLOCK), 0, st, (const uint64_t*)val.p, (const uint32_t*)tag.p,
                       (const int32_t*)head.p, ns, dval.p, dtag.p, d_ns1.p, d_ns2.p);
    hipLaunchKernelGGL(km_common, dim3(grid_for(nd)), dim3(AI_BLOCK), 0, st, (const uint64_t*)dval.p, (const uint32_t*)dtag.p, (int64_t)nd,
                       n_inst2, d_common.p);
    hipLaunchKernelGGL(km_inside, dim3(grid_for(n_chunk)), dim3(AI_BLOCK), 0, st, dc, dci, n_chunk, n_inst1, n_inst2,
                       (const unsigned long long*)box.p, d_inter.p);
    AI_KERNEL_CHECK();
  }
  AI_HIP(hipMemcpyAsync(inter, d_inter.p, n12 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipMemcpyAsync(common, d_common.p, n12 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipMemcpyAsync(n_scalars1, d_ns1.p, (size_t)n_inst1 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipMemcpyAsync(n_scalars2, d_ns2.p, (size_t)n_inst2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipMemcpyAsync(n_points1, d_np1.p, (size_t)n_inst1 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  return AI_OK;
}

extern "C" int ai_unique_points(ai_ctx* ctx, const double* xyz, int64_t n, int mem_kind, int32_t* keep_index, int64_t* n_keep) {
  if (!ctx || !xyz || !keep_index || !n_keep || n < 0 || n >= ((int64_t)1 << 30)) {
    ai_set_error("ai_unique_points: bad argument");
    return AI_ERR_BAD_ARG;
  }
  *n_keep = 0;
  if (n == 0) return AI_OK;
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<double> own;
  DevBuf<uint64_t> key, skey;
  DevBuf<int32_t> oa, ob, keep, scan_tmp, out;
  const double* dx;
  AI_TRY(to_device(xyz, (size_t)n * 3, mem_kind, own, &dx, st));
  AI_TRY(key.alloc(n));
  AI_TRY(skey.alloc(n));
  AI_TRY(oa.alloc(n));
  AI_TRY(ob.alloc(n));
  AI_TRY(keep.alloc(n + 1));
  hipLaunchKernelGGL(ku_iota, dim3(grid_for(n)), dim3(AI_BLOCK), 0, st, oa.p, n);
  AI_KERNEL_CHECK();
  int32_t *cur = oa.p, *nxt = ob.p;
  for (int axis = 2; axis >= 0; --axis) {  // least-significant key first; each pass is stable
    hipLaunchKernelGGL(ku_axis_keys, dim3(grid_for(n)), dim3(AI_BLOCK), 0, st, dx, (const int32_t*)cur, n, axis, key.p);
    AI_KERNEL_CHECK();
    AI_TRY(sort_pairs(st, key.p, skey.p, cur, nxt, n, 64));
    std::swap(cur, nxt);
  }
  hipLaunchKernelGGL(ku_first_flags, dim3(grid_for(n)), dim3(AI_BLOCK), 0, st, dx, (const int32_t*)cur, n, keep.p);
  AI_KERNEL_CHECK();
  AI_TRY(scan_flags(st, keep.p, n, scan_tmp));
  int32_t total = 0;
  AI_HIP(hipMemcpyAsync(&total, keep.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  AI_TRY(out.alloc(total));
  hipLaunchKernelGGL(kq_compact, dim3(grid_for(n)), dim3(AI_BLOCK), 0, st, (const int32_t*)keep.p, n, out.p);
  AI_KERNEL_CHECK();
  if (mem_kind == AI_MEM_DEVICE)
    AI_HIP(hipMemcpyAsync(keep_index, out.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  else
    AI_HIP(hipMemcpyAsync(keep_index, out.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  *n_keep = total;
  return AI_OK;
}
