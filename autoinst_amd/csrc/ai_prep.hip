// The step that produces the chunks (chunk_and_downsample_point_clouds, pipeline/dataset/dataset_utils.py:489-567, called at
// run_pipeline.py:129), for the non-ground and the ground minor-voxel maps alike:
//
//   ai_box_select          -- the crop of every chunk from the whole map (pipeline/utils/point_cloud/chunk_generation.py:
//                             134-137): for each axis-aligned box the ascending indices of the points strictly inside it.
//                             One pass over the map for all boxes: per-tile counts, one exclusive scan, fill.  The fill ranks
//                             a point inside its tile with a wave ballot, so the output order is the index order (no atomics).
//   ai_statistical_inliers -- open3d 0.17 PointCloud::RemoveStatisticalOutliers (called through point_cloud_utils.py:198-202
//                             at chunk_generation.py:143) as it is written:
//                               k = min(nb_neighbors, n); avg[i] = mean of the Euclidean distances of the k nearest points of
//                               point i (itself included, at distance 0), summed in ascending order and divided by k;
//                               mean = sum of the avg > 0 over ALL n points (the avg == 0 ones count in the denominator);
//                               std = sqrt(sum over avg > 0 of (avg - mean)^2 / (n - 1));
//                               point i is kept iff avg[i] > 0 && avg[i] < mean + std_ratio * std (ascending indices).
//                             nb_neighbors < 1 or std_ratio <= 0 is AI_ERR_BAD_ARG; an empty cloud keeps nothing; n = 1 keeps
//                             nothing (its avg is 0).  The kNN is exact: a ring search over a cell list (kp_nn1's stop rule),
//                             the k best squared distances in registers through an unrolled insertion network of compile-time
//                             length (20 / 32 / 64, k <= 64), so nothing spills to scratch.  The cell list is the points sorted
//                             by (z, y, x) cell plus one [start, end) pair per (z, y) row: memory grows with the points and the
//                             box's cross-section, not its volume; within a row a binary search finds the x range.  mean and
//                             std are fixed-order block reductions: bit-identical from call to call.
//   ai_voxel_down_sample   -- open3d PointCloud::VoxelDownSample (dataset_utils.py:534-535): vmin = min_bound - voxel_size / 2,
//                             voxel = floor((p - vmin) / voxel_size) with a true division, output point = the sum of the
//                             voxel's points in input-index order divided by their count.  open3d's output order comes from
//                             a hash map; ours is ascending (ix, iy, iz).  Stable radix sort by a 64-bit voxel key, then one
//                             thread per voxel sums serially: bit-equal to an np.add.at restatement.
//   ai_voxel_down_sample_nearest -- the minor-voxel map of load_and_downsample_point_clouds (dataset_utils.py:285-370): the same
//                             means (the same kernels, bit for bit) plus, per voxel, the input point nearest to its mean -- the
//                             point whose label the reference copies (:306-311).  Smallest (dx*dx + dy*dy) + dz*dz, ties to the
//                             smaller input index (our rule, ai_nn1_project's: open3d's KD-tree defines none).  The search runs
//                             on the sort that made the means: the sorted unique keys are the table of occupied voxels, and the
//                             voxels iz - r .. iz + r of one (ix, iy) row are one key range, i.e. one run of sorted points.
#include <climits>
#include <cmath>

#include <rocprim/device/device_scan.hpp>

#include "ai_cells.inc"

namespace {

// ----------------------------------------------------------------------------- bounds

constexpr int BOUND_BLOCKS = 256;

__global__ __launch_bounds__(AI_BLOCK) void kq_bounds(const double* __restrict__ xyz, int64_t n, double* __restrict__ part) {
  __shared__ double sm[6][AI_BLOCK / 64];
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AI_BLOCK)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      // fmin / fmax drop a NaN: a coordinate that is not finite goes in as +inf (kp_bounds' rule, ai_cells.inc), so that
      // bounds() sees it in the maximum
      const double c = xyz[i * 3 + a];
      const double v = fabs(c) < INFINITY ? c : INFINITY;
      mn[a] = fmin(mn[a], v);
      mx[a] = fmax(mx[a], v);
    }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[a] = fmin(mn[a], __shfl_xor(mn[a], o, 64));
      mx[a] = fmax(mx[a], __shfl_xor(mx[a], o, 64));
    }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      sm[a][w] = mn[a];
      sm[3 + a][w] = mx[a];
    }
  __syncthreads();
  if (threadIdx.x < 6) {
    double r = sm[threadIdx.x][0];
    for (int i = 1; i < AI_BLOCK / 64; ++i) r = (threadIdx.x < 3) ? fmin(r, sm[threadIdx.x][i]) : fmax(r, sm[threadIdx.x][i]);
    part[blockIdx.x * 6 + threadIdx.x] = r;
  }
}

// min / max per axis of n >= 1 points; AI_ERR_BAD_ARG when a coordinate is not finite
int bounds(ai_ctx* ctx, const double* d_xyz, int64_t n, double mn[3], double mx[3], const char* who) {
  hipStream_t st = ctx->stream;
  DevBuf<double> part;
  AI_TRY(part.alloc((size_t)BOUND_BLOCKS * 6));
  hipLaunchKernelGGL(kq_bounds, dim3(BOUND_BLOCKS), dim3(AI_BLOCK), 0, st, d_xyz, n, part.p);
  AI_KERNEL_CHECK();
  std::vector<double> hp((size_t)BOUND_BLOCKS * 6);
  AI_HIP(hipMemcpyAsync(hp.data(), part.p, hp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  for (int a = 0; a < 3; ++a) {
    mn[a] = INFINITY;
    mx[a] = -INFINITY;
  }
  for (int b = 0; b < BOUND_BLOCKS; ++b)
    for (int a = 0; a < 3; ++a) {
      mn[a] = std::min(mn[a], hp[b * 6 + a]);
      mx[a] = std::max(mx[a], hp[b * 6 + 3 + a]);
    }
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(mn[a]) || !std::isfinite(mx[a]) || !(mx[a] - mn[a] < 1e15)) {
      ai_set_error("%s: coordinates are not finite", who);
      return AI_ERR_BAD_ARG;
    }
  return AI_OK;
}

// ----------------------------------------------------------------------------- box select

// cnt[b * ntile + t] = #points of tile t (AI_BLOCK points) strictly inside box b (lo = box[6b..6b+2], hi = box[6b+3..6b+5])
__device__ __forceinline__ bool in_box(const double* __restrict__ B, double x, double y, double z) {
  return x > B[0] && y > B[1] && z > B[2] && x < B[3] && y < B[4] && z < B[5];
}

__global__ __launch_bounds__(AI_BLOCK) void kb_count(const double* __restrict__ xyz, int64_t n, const double* __restrict__ box,
                                                     int32_t nbox, int64_t* __restrict__ cnt) {
  __shared__ int32_t wc[AI_BLOCK / 64];
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const bool ok = i < n;
  const double x = ok ? xyz[i * 3] : 0.0, y = ok ? xyz[i * 3 + 1] : 0.0, z = ok ? xyz[i * 3 + 2] : 0.0;
  const int64_t ntile = gridDim.x;
  for (int b = 0; b < nbox; ++b) {
    const uint64_t m = __ballot(ok && in_box(box + 6 * b, x, y, z));
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
      int32_t s = 0;
#pragma unroll
      for (int w = 0; w < AI_BLOCK / 64; ++w) s += wc[w];
      cnt[(int64_t)b * ntile + blockIdx.x] = s;
    }
    __syncthreads();
  }
}

// off = exclusive scan of kb_count's counts (box-major): box b's indices are contiguous, in tile order, and inside a tile in
// lane order, i.e. ascending
__global__ __launch_bounds__(AI_BLOCK) void kb_fill(const double* __restrict__ xyz, int64_t n, const double* __restrict__ box,
                                                    int32_t nbox, const int64_t* __restrict__ off, int64_t cap,
                                                    int32_t* __restrict__ out) {
  __shared__ int32_t wc[AI_BLOCK / 64];
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const bool ok = i < n;
  const double x = ok ? xyz[i * 3] : 0.0, y = ok ? xyz[i * 3 + 1] : 0.0, z = ok ? xyz[i * 3 + 2] : 0.0;
  const int64_t ntile = gridDim.x;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int b = 0; b < nbox; ++b) {
    const bool in = ok && in_box(box + 6 * b, x, y, z);
    const uint64_t m = __ballot(in);
    if (lane == 0) wc[w] = __popcll(m);
    __syncthreads();
    if (in) {
      int64_t pos = off[(int64_t)b * ntile + blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
      for (int v = 0; v < w; ++v) pos += wc[v];
      if (pos < cap) out[pos] = (int32_t)i;
    }
    __syncthreads();
  }
}

__global__ void kb_box_offsets(const int64_t* __restrict__ off, int32_t nbox, int64_t ntile, int64_t* __restrict__ boff) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b <= nbox) boff[b] = off[(int64_t)b * ntile];  // off has nbox * ntile + 1 entries: boff[nbox] is the total
}

// ----------------------------------------------------------------------------- statistical inliers

// sort key: row (z, y) in the high bits, x cell in the low 32
__global__ __launch_bounds__(AI_BLOCK) void kq_keys(const double* __restrict__ xyz, int64_t n, KGrid g, uint64_t* __restrict__ key,
                                                    int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  int cx, cy, cz;
  kcell_of(g, xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], cx, cy, cz);
  key[i] = ((uint64_t)((int64_t)cz * g.ny + cy) << 32) | (uint32_t)cx;
  idx[i] = (int32_t)i;
}

// One thread per point (in cell order, so that a wave's queries are neighbours): the k <= K smallest squared distances to the
// cloud (the point itself included) by rings of cells around its own cell.  Ring r is the shell of Chebyshev cell distance r: in
// the rows (dz, dy) on the shell's faces the whole x range [cx - r, cx + r], in the other rows the cells cx - r and cx + r.
// Stop rule: the ring searches' (ai_cells.inc, where it is derived), for the k-th best in place of the best: the k smallest squares
// seen are then the k smallest of the whole cloud, whatever the grid is.
// avg[order[p]] = (sum of the k distances in ascending order) / k.
template <int K>
__global__ __launch_bounds__(AI_BLOCK) void kq_knn_avg(int64_t n, int32_t k, KGrid g, const double* __restrict__ X,
                                                       const double* __restrict__ Y, const double* __restrict__ Z,
                                                       const int32_t* __restrict__ scx, const int32_t* __restrict__ rstart,
                                                       const int32_t* __restrict__ rend, const int32_t* __restrict__ order,
                                                       double* __restrict__ avg) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p >= n) return;
  const double x = X[p], y = Y[p], z = Z[p];
  int cx, cy, cz;
  kcell_of(g, x, y, z, cx, cy, cz);
  double best[K];
#pragma unroll
  for (int j = 0; j < K; ++j) best[j] = INFINITY;
  int64_t seen = 0;
  const double eps = 2.220446049250313e-16;
  const double slack = 8.0 * eps * fmax(fmax(axis_mag(x, g.minx, g.cell, g.nx), axis_mag(y, g.miny, g.cell, g.ny)), axis_mag(z, g.minz, g.cell, g.nz));
  const int rmax = max(g.nx, max(g.ny, g.nz));
  for (int r = 0; r <= rmax; ++r) {
    const int z0 = max(cz - r, 0), z1 = min(cz + r, g.nz - 1);
    const int y0 = max(cy - r, 0), y1 = min(cy + r, g.ny - 1);
    for (int zz = z0; zz <= z1; ++zz) {
      for (int yy = y0; yy <= y1; ++yy) {
        const int row = zz * g.ny + yy;
        const int32_t s = rstart[row], e = rend[row];
        if (s >= e) continue;
        const bool face = (abs(zz - cz) == r) || (abs(yy - cy) == r);
        // face row: one range [cx - r, cx + r]; other rows: the two single cells cx - r and cx + r
        for (int part = 0; part < (face ? 1 : 2); ++part) {
          int lo, hi;
          if (face) {
            lo = cx - r;
            hi = cx + r;
          } else {
            lo = hi = (part == 0) ? cx - r : cx + r;
          }
          lo = max(lo, 0);
          hi = min(hi, g.nx - 1);
          if (lo > hi) continue;
          int32_t a = s, b = e;  // first q in [s, e) with scx[q] >= lo
          while (a < b) {
            const int32_t m = (a + b) >> 1;
            if (scx[m] < lo)
              a = m + 1;
            else
              b = m;
          }
          for (int32_t q = a; q < e && scx[q] <= hi; ++q) {
            knn_insert<K>(best, sq_dist3(x, y, z, X[q], Y[q], Z[q]));
            ++seen;
          }
        }
      }
    }
    if (seen >= k) {
      double kth = best[0];
#pragma unroll
      for (int j = 1; j < K; ++j)
        if (j == k - 1) kth = best[j];
      const double lb = fmin(face_gap(x, g.minx, g.cell, cx, r, g.nx), fmin(face_gap(y, g.miny, g.cell, cy, r, g.ny), face_gap(z, g.minz, g.cell, cz, r, g.nz))) - slack;
      if (sqrt(kth) * (1.0 + 4.0 * eps) <= lb) break;
    }
  }
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < K; ++j)
    if (j < k) sum += sqrt(best[j]);
  avg[order[p]] = sum / (double)k;
}

constexpr int RED_BLOCKS = 256;

// part[block] = sum over the block's fixed share of i with avg[i] > 0 of (avg[i] - centre)^pw, pw = 1 or 2
__global__ __launch_bounds__(AI_BLOCK) void kq_partial(const double* __restrict__ avg, int64_t n, const double* __restrict__ stats,
                                                       int pw, double* __restrict__ part) {
  __shared__ double sm[AI_BLOCK / 64];
  const double c = pw == 2 ? stats[0] : 0.0;
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AI_BLOCK) {
    const double v = avg[i];
    if (v > 0.0) s += pw == 2 ? (v - c) * (v - c) : v;
  }
  s = ai_block_sum_first(s, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// stats[0] = mean = total / n (pw 1); stats[1] = std = sqrt(total / (n - 1)), stats[2] = threshold (pw 2)
__global__ __launch_bounds__(AI_BLOCK) void kq_finish(const double* __restrict__ part, int64_t n, int pw, double std_ratio,
                                                      double* __restrict__ stats) {
  __shared__ double sm[AI_BLOCK / 64];
  static_assert(RED_BLOCKS == AI_BLOCK, "one partial per thread");
  const double t = ai_block_sum_first(part[threadIdx.x], sm);
  if (threadIdx.x == 0) {
    if (pw == 1) {
      stats[0] = t / (double)n;
    } else {
      const double sd = sqrt(t / (double)(n - 1));  // n = 1: 0 / 0, NaN, and nothing is kept (avg is 0 anyway)
      stats[1] = sd;
      stats[2] = stats[0] + std_ratio * sd;
    }
  }
}

// flag[i] = avg[i] > 0 && avg[i] < threshold
__global__ __launch_bounds__(AI_BLOCK) void kq_keep_flags(const double* __restrict__ avg, int64_t n, const double* __restrict__ stats,
                                                          int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  const double v = avg[i];
  flag[i] = (v > 0.0 && v < stats[2]) ? 1 : 0;
}

// ----------------------------------------------------------------------------- voxel down-sampling

struct VGrid {
  double vminx, vminy, vminz, size;
  int sy, sz;  // key = ix << sy | iy << sz | iz
};

__global__ __launch_bounds__(AI_BLOCK) void kv_keys(const double* __restrict__ xyz, int64_t n, VGrid g, uint64_t* __restrict__ key,
                                                    int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  // open3d: ref_coord = (p - voxel_min_bound) / voxel_size; int(floor(ref_coord)) -- a true division
  const uint64_t ix = (uint64_t)(int64_t)floor((xyz[i * 3] - g.vminx) / g.size);
  const uint64_t iy = (uint64_t)(int64_t)floor((xyz[i * 3 + 1] - g.vminy) / g.size);
  const uint64_t iz = (uint64_t)(int64_t)floor((xyz[i * 3 + 2] - g.vminz) / g.size);
  key[i] = (ix << g.sy) | (iy << g.sz) | iz;
  idx[i] = (int32_t)i;
}

// one thread per voxel: the sum of its points in input-index order (the sort is stable), divided by their count
__global__ __launch_bounds__(AI_BLOCK) void kv_mean(const double* __restrict__ xyz, const int32_t* __restrict__ order,
                                                    const int32_t* __restrict__ start, int64_t m, double* __restrict__ out,
                                                    int32_t* __restrict__ trace) {
  const int64_t v = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (v >= m) return;
  const int32_t s = start[v], e = start[v + 1];
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int32_t p = s; p < e; ++p) {
    const int64_t o = order[p];
    sx += xyz[o * 3];
    sy += xyz[o * 3 + 1];
    sz += xyz[o * 3 + 2];
    if (trace) trace[o] = (int32_t)v;
  }
  const double c = (double)(e - s);
  out[v * 3] = sx / c;
  out[v * 3 + 1] = sy / c;
  out[v * 3 + 2] = sz / c;
}

// ----------------------------------------------------------------------------- nearest input point of every voxel mean

// the sorted points' coordinates, contiguous per voxel run (kq_gather's layout), and the table of occupied voxels: ukey[v] = the
// key of voxel v (ascending, as the voxels are)
__global__ __launch_bounds__(AI_BLOCK) void kn_gather(const double* __restrict__ xyz, const int32_t* __restrict__ order,
                                                      const uint64_t* __restrict__ skey, const int32_t* __restrict__ vid, int64_t n,
                                                      double* __restrict__ X, double* __restrict__ Y, double* __restrict__ Z,
                                                      uint64_t* __restrict__ ukey) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p >= n) return;
  const int64_t o = order[p];
  X[p] = xyz[o * 3];
  Y[p] = xyz[o * 3 + 1];
  Z[p] = xyz[o * 3 + 2];
  if (vid[p + 1] != vid[p]) ukey[vid[p]] = skey[p];  // p is the head of its voxel's run
}

struct NGrid {
  double vmin[3], size;
  int sy, sz;      // key = ix << sy | iy << sz | iz, as VGrid
  int nx, ny, nz;  // indices per axis that the key has room for (powers of two >= the occupied range)
};

// One thread per voxel v (in key order, so that a wave's voxels are neighbours): the input point nearest to the voxel's mean c.
// Ring r is the shell of voxels at Chebyshev index distance r from v's own voxel.  In a row (ix + dx, iy + dy) on the shell's
// faces (max(|dx|, |dy|) == r) the voxels iz - r .. iz + r are one key range; in an inner row the shell has the two voxels
// iz - r and iz + r.  A key range is found by a binary search in ukey (for v's own row inside [v - r, v + r]: the row's voxels
// are v's neighbours in the table) and is one run [start[a], start[b]) of the sorted points.
// Stop rule (kp_nn1's, with the rounding counted): a point outside rings 0..r has, on some axis, a computed voxel index beyond
// i - r .. i + r, so it lies beyond that face of the box of rings 0..r.  `lb` is the distance from c to the nearest such face,
// less 8 ulps of the largest magnitude that enters the index and the face (the subtraction p - vmin, the division, i * size +
// vmin), which covers the rounding of every one of them: strictly below the distance of every unvisited point.  Hence
// sqrt(best) <= lb leaves no unvisited point that is nearer or tied.  In exact arithmetic ring 1 always ends the search (DESIGN.md
// section 13); the loop does not rely on it.
__global__ __launch_bounds__(AI_BLOCK) void kn_nearest(int64_t m, NGrid g, const double* __restrict__ cen,
                                                       const uint64_t* __restrict__ ukey, const int32_t* __restrict__ start,
                                                       const double* __restrict__ X, const double* __restrict__ Y,
                                                       const double* __restrict__ Z, const int32_t* __restrict__ order,
                                                       int32_t* __restrict__ nn_idx, double* __restrict__ nn_dist) {
  const int64_t v = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (v >= m) return;
  const double cx = cen[v * 3], cy = cen[v * 3 + 1], cz = cen[v * 3 + 2];
  const uint64_t key = ukey[v];
  const int64_t iz = (int64_t)(key & ((uint64_t)g.nz - 1));
  const int64_t iy = (int64_t)((key >> g.sz) & ((uint64_t)g.ny - 1));
  const int64_t ix = (int64_t)(key >> g.sy);
  const double mag = fmax(fmax(fabs(g.vmin[0]) + (double)g.nx * g.size, fabs(g.vmin[1]) + (double)g.ny * g.size),
                          fabs(g.vmin[2]) + (double)g.nz * g.size);
  const double slack = 8.0 * 2.220446049250313e-16 * (mag + 2.0 * g.size);
  double best = INFINITY;
  int32_t bi = INT_MAX;
  auto scan = [&](int32_t s, int32_t e) {
    for (int32_t p = s; p < e; ++p) {
      const double d2 = sq_dist3(cx, cy, cz, X[p], Y[p], Z[p]);
      if (d2 <= best) {  // ties: the smaller input index wins, whichever voxel is visited first
        const int32_t o = order[p];
        if (d2 < best || o < bi) {
          best = d2;
          bi = o;
        }
      }
    }
  };
  // the points of the voxels z0 .. z1 (clamped to the grid) of row (xx, yy); the range's first voxel is searched in [a, b)
  auto scan_row = [&](int64_t xx, int64_t yy, int64_t z0, int64_t z1, int64_t a, int64_t b) {
    z0 = max(z0, (int64_t)0);
    z1 = min(z1, (int64_t)g.nz - 1);
    if (z0 > z1) return;
    const uint64_t row = ((uint64_t)xx << g.sy) | ((uint64_t)yy << g.sz);
    const uint64_t klo = row | (uint64_t)z0, khi = row | (uint64_t)z1;
    while (a < b) {  // first voxel with ukey >= klo
      const int64_t h = (a + b) >> 1;
      if (ukey[h] < klo)
        a = h + 1;
      else
        b = h;
    }
    int64_t u = a;
    while (u < m && ukey[u] <= khi) ++u;  // at most z1 - z0 + 1 steps
    if (u > a) scan(start[a], start[u]);
  };
  scan(start[v], start[v + 1]);  // ring 0: the voxel's own members
  const int64_t rmax = max(g.nx, max(g.ny, g.nz));
  for (int64_t r = 0;; ++r) {
    if (r > 0) {
      for (int64_t dx = -r; dx <= r; ++dx) {
        const int64_t xx = ix + dx;
        if (xx < 0 || xx >= g.nx) continue;
        for (int64_t dy = -r; dy <= r; ++dy) {
          const int64_t yy = iy + dy;
          if (yy < 0 || yy >= g.ny) continue;
          const bool own = dx == 0 && dy == 0;
          const int64_t a = own ? max(v - r, (int64_t)0) : 0, b = own ? min(v + r + 1, m) : m;
          if (max(dx < 0 ? -dx : dx, dy < 0 ? -dy : dy) == r) {
            scan_row(xx, yy, iz - r, iz + r, a, b);
          } else {
            scan_row(xx, yy, iz - r, iz - r, a, b);
            scan_row(xx, yy, iz + r, iz + r, a, b);
          }
        }
      }
    }
    if (r >= rmax) break;  // every voxel of the grid has been visited
    const double rr = (double)r;
    const double fx = fmin(cx - (g.vmin[0] + ((double)ix - rr) * g.size), (g.vmin[0] + ((double)ix + rr + 1.0) * g.size) - cx);
    const double fy = fmin(cy - (g.vmin[1] + ((double)iy - rr) * g.size), (g.vmin[1] + ((double)iy + rr + 1.0) * g.size) - cy);
    const double fz = fmin(cz - (g.vmin[2] + ((double)iz - rr) * g.size), (g.vmin[2] + ((double)iz + rr + 1.0) * g.size) - cz);
    const double lb = fmin(fx, fmin(fy, fz)) - slack;
    if (sqrt(best) * (1.0 + 4.0 * 2.220446049250313e-16) <= lb) break;
  }
  nn_idx[v] = bi;
  if (nn_dist) nn_dist[v] = sqrt(best);
}

}  // namespace

extern "C" int ai_box_select(ai_ctx* ctx, const double* xyz, int64_t n, const double* boxes, int32_t n_boxes, int mem_kind, int64_t cap,
                             int32_t* out_index, int64_t* box_offsets, int64_t* n_total) {
  if (!ctx || !xyz || !boxes || !box_offsets || !n_total || (cap > 0 && !out_index) || n < 0 || cap < 0 || n_boxes < 1 ||
      n_boxes > 65536 || n >= ((int64_t)1 << 31) - AI_BLOCK) {
    ai_set_error("ai_box_select: bad argument");
    return AI_ERR_BAD_ARG;
  }
  *n_total = 0;
  if (n == 0) {
    for (int b = 0; b <= n_boxes; ++b) box_offsets[b] = 0;
    return AI_OK;
  }
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<double> own, d_box;
  DevBuf<int64_t> cnt, off, boff;
  DevBuf<int32_t> d_out;
  const double* dx;
  AI_TRY(to_device(xyz, (size_t)n * 3, mem_kind, own, &dx, st));
  AI_TRY(d_box.alloc((size_t)n_boxes * 6));
  AI_HIP(hipMemcpyAsync(d_box.p, boxes, (size_t)n_boxes * 6 * sizeof(double), hipMemcpyHostToDevice, st));
  const int64_t ntile = grid_for(n);
  const int64_t m = ntile * n_boxes;
  AI_TRY(cnt.alloc(m + 1));
  AI_TRY(off.alloc(m + 1));
  AI_TRY(boff.alloc(n_boxes + 1));
  AI_HIP(hipMemsetAsync(cnt.p + m, 0, sizeof(int64_t), st));
  hipLaunchKernelGGL(kb_count, dim3((unsigned)ntile), dim3(AI_BLOCK), 0, st, dx, n, (const double*)d_box.p, n_boxes, cnt.p);
  AI_KERNEL_CHECK();
  size_t tmp_bytes = 0;
  AI_HIP(rocprim::exclusive_scan(nullptr, tmp_bytes, cnt.p, off.p, (int64_t)0, (size_t)(m + 1), rocprim::plus<int64_t>(), st));
  DevBuf<uint8_t> tmp;
  AI_TRY(tmp.alloc(tmp_bytes));
  AI_HIP(rocprim::exclusive_scan(tmp.p, tmp_bytes, cnt.p, off.p, (int64_t)0, (size_t)(m + 1), rocprim::plus<int64_t>(), st));
  hipLaunchKernelGGL(kb_box_offsets, dim3((unsigned)((n_boxes + 1 + 63) / 64)), dim3(64), 0, st, (const int64_t*)off.p, n_boxes, ntile,
                     boff.p);
  AI_KERNEL_CHECK();
  AI_HIP(hipMemcpyAsync(box_offsets, boff.p, (size_t)(n_boxes + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  const int64_t total = box_offsets[n_boxes];
  *n_total = total;
  if (total > cap || total == 0) return AI_OK;  // the caller calls again with cap >= *n_total
  int32_t* o = out_index;
  if (mem_kind != AI_MEM_DEVICE) {
    AI_TRY(d_out.alloc(total));
    o = d_out.p;
  }
  hipLaunchKernelGGL(kb_fill, dim3((unsigned)ntile), dim3(AI_BLOCK), 0, st, dx, n, (const double*)d_box.p, n_boxes, (const int64_t*)off.p,
                     total, o);
  AI_KERNEL_CHECK();
  if (mem_kind != AI_MEM_DEVICE) AI_HIP(hipMemcpyAsync(out_index, o, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  return AI_OK;
}

extern "C" int ai_statistical_inliers(ai_ctx* ctx, const double* xyz, int64_t n, int32_t nb_neighbors, double std_ratio, int mem_kind,
                                      int32_t* keep_index, int64_t* n_keep, double* avg_out, double* stats_out) {
  if (!ctx || !n_keep || (n > 0 && (!xyz || !keep_index)) || n < 0 || n >= ((int64_t)1 << 30)) {
    ai_set_error("ai_statistical_inliers: bad argument");
    return AI_ERR_BAD_ARG;
  }
  if (nb_neighbors < 1 || !(std_ratio > 0.0)) {  // open3d: "Illegal input parameters, ... must be positive"
    ai_set_error("ai_statistical_inliers: nb_neighbors must be >= 1 and std_ratio > 0");
    return AI_ERR_BAD_ARG;
  }
  if (nb_neighbors > 64 && n > 64) {
    ai_set_error("ai_statistical_inliers: nb_neighbors > 64 is not supported");
    return AI_ERR_BAD_ARG;
  }
  *n_keep = 0;
  if (n == 0) return AI_OK;
  const int32_t k = (int32_t)std::min<int64_t>(nb_neighbors, n);
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<double> own, X, Y, Z, d_avg, part, stats;
  DevBuf<uint64_t> key, skey;
  DevBuf<int32_t> idx, order, scx, rstart, rend, flag, scan_tmp, d_keep;
  const double* dx;
  AI_TRY(to_device(xyz, (size_t)n * 3, mem_kind, own, &dx, st));
  double mn[3], mx[3];
  AI_TRY(bounds(ctx, dx, n, mn, mx, "ai_statistical_inliers"));
  // cell edge: the side of the bounding box's volume per point (thin axes count as 1e-3 of the widest), grown until the rows and
  // the x cells fit their 32-bit key halves and the row table has at most 2 n + 1024 entries
  double ext[3], emax = 0.0;
  for (int a = 0; a < 3; ++a) emax = std::max(emax, mx[a] - mn[a]);
  double vol = 1.0;
  for (int a = 0; a < 3; ++a) {
    ext[a] = mx[a] - mn[a];
    vol *= std::max(ext[a], std::max(1e-3 * emax, 1e-9));
  }
  double cell = std::cbrt(vol / (double)n);
  KGrid g;
  for (;;) {
    const double fx = floor(ext[0] / cell) + 1, fy = floor(ext[1] / cell) + 1, fz = floor(ext[2] / cell) + 1;
    if (fx < 1e9 && fy * fz <= 2.0 * (double)n + 1024.0) {
      g.nx = (int)fx;
      g.ny = (int)fy;
      g.nz = (int)fz;
      break;
    }
    cell *= 1.5;
  }
  g.minx = mn[0];
  g.miny = mn[1];
  g.minz = mn[2];
  g.cell = cell;
  g.inv_cell = 1.0 / cell;
  const int64_t nrow = (int64_t)g.ny * g.nz;
  const unsigned gb = grid_for(n);
  AI_TRY(key.alloc(n));
  AI_TRY(skey.alloc(n));
  AI_TRY(idx.alloc(n));
  AI_TRY(order.alloc(n));
  AI_TRY(X.alloc(n));
  AI_TRY(Y.alloc(n));
  AI_TRY(Z.alloc(n));
  AI_TRY(scx.alloc(n));
  AI_TRY(rstart.alloc(nrow));
  AI_TRY(rend.alloc(nrow));
  hipLaunchKernelGGL(kq_keys, dim3(gb), dim3(AI_BLOCK), 0, st, dx, n, g, key.p, idx.p);
  AI_KERNEL_CHECK();
  AI_TRY(sort_pairs(st, key.p, skey.p, idx.p, order.p, n, 32 + bits_for(nrow)));
  AI_HIP(hipMemsetAsync(rstart.p, 0, (size_t)nrow * sizeof(int32_t), st));
  AI_HIP(hipMemsetAsync(rend.p, 0, (size_t)nrow * sizeof(int32_t), st));
  hipLaunchKernelGGL(kq_gather, dim3(gb), dim3(AI_BLOCK), 0, st, dx, (const int32_t*)order.p, (const uint64_t*)skey.p, n, X.p, Y.p, Z.p,
                     scx.p, rstart.p, rend.p);
  AI_KERNEL_CHECK();
  double* avg = avg_out;
  if (mem_kind != AI_MEM_DEVICE || !avg_out) {
    AI_TRY(d_avg.alloc(n));
    avg = d_avg.p;
  }
#define KQ_ARGS                                                                                                                      \
  dim3(gb), dim3(AI_BLOCK), 0, st, n, k, g, (const double*)X.p, (const double*)Y.p, (const double*)Z.p, (const int32_t*)scx.p,   \
      (const int32_t*)rstart.p, (const int32_t*)rend.p, (const int32_t*)order.p, avg
  if (k <= 20)
    hipLaunchKernelGGL(kq_knn_avg<20>, KQ_ARGS);
  else if (k <= 32)
    hipLaunchKernelGGL(kq_knn_avg<32>, KQ_ARGS);
  else
    hipLaunchKernelGGL(kq_knn_avg<64>, KQ_ARGS);
#undef KQ_ARGS
  AI_KERNEL_CHECK();
  AI_TRY(part.alloc(RED_BLOCKS));
  AI_TRY(stats.alloc(3));
  hipLaunchKernelGGL(kq_partial, dim3(RED_BLOCKS), dim3(AI_BLOCK), 0, st, (const double*)avg, n, (const double*)stats.p, 1, part.p);
  AI_KERNEL_CHECK();
  hipLaunchKernelGGL(kq_finish, dim3(1), dim3(AI_BLOCK), 0, st, (const double*)part.p, n, 1, std_ratio, stats.p);
  AI_KERNEL_CHECK();
  hipLaunchKernelGGL(kq_partial, dim3(RED_BLOCKS), dim3(AI_BLOCK), 0, st, (const double*)avg, n, (const double*)stats.p, 2, part.p);
  AI_KERNEL_CHECK();
  hipLaunchKernelGGL(kq_finish, dim3(1), dim3(AI_BLOCK), 0, st, (const double*)part.p, n, 2, std_ratio, stats.p);
  AI_KERNEL_CHECK();
  AI_TRY(flag.alloc(n + 1));
  AI_TRY(scan_tmp.alloc(ai_scan_tmp_elems(n)));
  hipLaunchKernelGGL(kq_keep_flags, dim3(gb), dim3(AI_BLOCK), 0, st, (const double*)avg, n, (const double*)stats.p, flag.p);
  AI_KERNEL_CHECK();
  AI_TRY(ai_exclusive_scan_i32(st, flag.p, flag.p, n, scan_tmp.p));
  int32_t* o = keep_index;
  if (mem_kind != AI_MEM_DEVICE) {
    AI_TRY(d_keep.alloc(n));
    o = d_keep.p;
  }
  hipLaunchKernelGGL(kq_compact, dim3(gb), dim3(AI_BLOCK), 0, st, (const int32_t*)flag.p, n, o);
  AI_KERNEL_CHECK();
  int32_t total = 0;
  AI_HIP(hipMemcpyAsync(&total, flag.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (stats_out) AI_HIP(hipMemcpyAsync(stats_out, stats.p, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  if (mem_kind != AI_MEM_DEVICE) {
    AI_HIP(hipMemcpyAsync(keep_index, o, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (avg_out) AI_HIP(hipMemcpyAsync(avg_out, avg, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    AI_HIP(hipStreamSynchronize(st));
  }
  *n_keep = total;
  return AI_OK;
}

extern "C" int ai_voxel_down_sample(ai_ctx* ctx, const double* xyz, int64_t n, double voxel_size, int mem_kind, double* out_xyz,
                                    int64_t* n_out, int32_t* trace) {
  if (!ctx || !n_out || (n > 0 && (!xyz || !out_xyz)) || n < 0 || n >= ((int64_t)1 << 30)) {
    ai_set_error("ai_voxel_down_sample: bad argument");
    return AI_ERR_BAD_ARG;
  }
  if (!(voxel_size > 0.0) || !std::isfinite(voxel_size)) {
    ai_set_error("ai_voxel_down_sample: voxel_size <= 0");
    return AI_ERR_BAD_ARG;
  }
  *n_out = 0;
  if (n == 0) return AI_OK;
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<double> own, d_out;
  DevBuf<uint64_t> key, skey;
  DevBuf<int32_t> idx, order, vid, start, scan_tmp, d_trace;
  const double* dx;
  AI_TRY(to_device(xyz, (size_t)n * 3, mem_kind, own, &dx, st));
  double mn[3], mx[3];
  AI_TRY(bounds(ctx, dx, n, mn, mx, "ai_voxel_down_sample"));
  VGrid g;
  double vmin[3], span = 0.0;
  int bits[3];
  for (int a = 0; a < 3; ++a) {
    vmin[a] = mn[a] - voxel_size * 0.5;
    span = std::max(span, (mx[a] + voxel_size * 0.5) - vmin[a]);
  }
  if (voxel_size * (double)INT_MAX < span) {  // open3d: "voxel_size is too small."
    ai_set_error("ai_voxel_down_sample: voxel_size is too small (a voxel index would leave the int range)");
    return AI_ERR_BAD_ARG;
  }
  for (int a = 0; a < 3; ++a) bits[a] = bits_for((int64_t)floor((mx[a] - vmin[a]) / voxel_size) + 1);  // the largest index + 1
  if (bits[0] + bits[1] + bits[2] > 64) {
    ai_set_error("ai_voxel_down_sample: the voxel grid needs %d key bits (at most 64)", bits[0] + bits[1] + bits[2]);
    return AI_ERR_BAD_ARG;
  }
  g.vminx = vmin[0];
  g.vminy = vmin[1];
  g.vminz = vmin[2];
  g.size = voxel_size;
  g.sz = bits[2];
  g.sy = bits[1] + bits[2];
  const unsigned gb = grid_for(n);
  AI_TRY(key.alloc(n));
  AI_TRY(skey.alloc(n));
  AI_TRY(idx.alloc(n));
  AI_TRY(order.alloc(n));
  AI_TRY(vid.alloc(n + 1));
  AI_TRY(start.alloc(n + 1));
  AI_TRY(scan_tmp.alloc(ai_scan_tmp_elems(n)));
  hipLaunchKernelGGL(kv_keys, dim3(gb), dim3(AI_BLOCK), 0, st, dx, n, g, key.p, idx.p);
  AI_KERNEL_CHECK();
  AI_TRY(sort_pairs(st, key.p, skey.p, idx.p, order.p, n, std::max(1, bits[0] + bits[1] + bits[2])));
  hipLaunchKernelGGL(kl_heads<uint64_t>, dim3(gb), dim3(AI_BLOCK), 0, st, (const uint64_t*)skey.p, n, vid.p);
  AI_KERNEL_CHECK();
  AI_TRY(ai_exclusive_scan_i32(st, vid.p, vid.p, n, scan_tmp.p));
  hipLaunchKernelGGL(kv_starts, dim3(grid_for(n + 1)), dim3(AI_BLOCK), 0, st, (const int32_t*)vid.p, n, start.p);
  AI_KERNEL_CHECK();
  int32_t m = 0;
  AI_HIP(hipMemcpyAsync(&m, vid.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  double* o = out_xyz;
  int32_t* tr = trace;
  if (mem_kind != AI_MEM_DEVICE) {
    AI_TRY(d_out.alloc((size_t)m * 3));
    o = d_out.p;
    if (trace) {
      AI_TRY(d_trace.alloc(n));
      tr = d_trace.p;
    }
  }
  hipLaunchKernelGGL(kv_mean, dim3(grid_for(m)), dim3(AI_BLOCK), 0, st, dx, (const int32_t*)order.p, (const int32_t*)start.p, (int64_t)m,
                     o, tr);
  AI_KERNEL_CHECK();
  if (mem_kind != AI_MEM_DEVICE) {
    AI_HIP(hipMemcpyAsync(out_xyz, o, (size_t)m * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (trace) AI_HIP(hipMemcpyAsync(trace, tr, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  }
  AI_HIP(hipStreamSynchronize(st));
  *n_out = m;
  return AI_OK;
}

extern "C" int ai_voxel_down_sample_nearest(ai_ctx* ctx, const double* xyz, int64_t n, double voxel_size, int mem_kind, double* out_xyz,
                                            int64_t* n_out, int32_t* trace, int32_t* nearest_index, double* nearest_dist) {
  if (!ctx || !n_out || (n > 0 && (!xyz || !out_xyz || !nearest_index)) || n < 0 || n >= ((int64_t)1 << 31) - AI_BLOCK) {
    ai_set_error("ai_voxel_down_sample_nearest: bad argument");
    return AI_ERR_BAD_ARG;
  }
  if (!(voxel_size > 0.0) || !std::isfinite(voxel_size)) {
    ai_set_error("ai_voxel_down_sample_nearest: voxel_size <= 0");
    return AI_ERR_BAD_ARG;
  }
  *n_out = 0;
  if (n == 0) return AI_OK;
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<double> own, d_out, X, Y, Z, d_dist;
  DevBuf<uint64_t> key, skey;
  DevBuf<int32_t> idx, order, vid, start, scan_tmp, d_trace, d_nn;
  const double* dx;
  AI_TRY(to_device(xyz, (size_t)n * 3, mem_kind, own, &dx, st));
  double mn[3], mx[3];
  AI_TRY(bounds(ctx, dx, n, mn, mx, "ai_voxel_down_sample_nearest"));
  // the grid, the keys and the means are ai_voxel_down_sample's, step for step (and kernel for kernel)
  VGrid g;
  double vmin[3], span = 0.0;
  int bits[3];
  for (int a = 0; a < 3; ++a) {
    vmin[a] = mn[a] - voxel_size * 0.5;
    span = std::max(span, (mx[a] + voxel_size * 0.5) - vmin[a]);
  }
  if (voxel_size * (double)INT_MAX < span) {  // open3d: "voxel_size is too small."
    ai_set_error("ai_voxel_down_sample_nearest: voxel_size is too small (a voxel index would leave the int range)");
    return AI_ERR_BAD_ARG;
  }
  for (int a = 0; a < 3; ++a) bits[a] = bits_for((int64_t)floor((mx[a] - vmin[a]) / voxel_size) + 1);  // the largest index + 1
  if (bits[0] + bits[1] + bits[2] > 64) {
    ai_set_error("ai_voxel_down_sample_nearest: the voxel grid needs %d key bits (at most 64)", bits[0] + bits[1] + bits[2]);
    return AI_ERR_BAD_ARG;
  }
  g.vminx = vmin[0];
  g.vminy = vmin[1];
  g.vminz = vmin[2];
  g.size = voxel_size;
  g.sz = bits[2];
  g.sy = bits[1] + bits[2];
  const unsigned gb = grid_for(n);
  AI_TRY(key.alloc(n));
  AI_TRY(skey.alloc(n));
  AI_TRY(idx.alloc(n));
  AI_TRY(order.alloc(n));
  AI_TRY(vid.alloc(n + 1));
  AI_TRY(start.alloc(n + 1));
  AI_TRY(scan_tmp.alloc(ai_scan_tmp_elems(n)));
  hipLaunchKernelGGL(kv_keys, dim3(gb), dim3(AI_BLOCK), 0, st, dx, n, g, key.p, idx.p);
  AI_KERNEL_CHECK();
  AI_TRY(sort_pairs(st, key.p, skey.p, idx.p, order.p, n, std::max(1, bits[0] + bits[1] + bits[2])));
  hipLaunchKernelGGL(kl_heads<uint64_t>, dim3(gb), dim3(AI_BLOCK), 0, st, (const uint64_t*)skey.p, n, vid.p);
  AI_KERNEL_CHECK();
  AI_TRY(ai_exclusive_scan_i32(st, vid.p, vid.p, n, scan_tmp.p));
  hipLaunchKernelGGL(kv_starts, dim3(grid_for(n + 1)), dim3(AI_BLOCK), 0, st, (const int32_t*)vid.p, n, start.p);
  AI_KERNEL_CHECK();
  int32_t m = 0;
  AI_HIP(hipMemcpyAsync(&m, vid.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  // the sorted coordinates and the voxel table do not need m: they run while the count comes back
  AI_TRY(X.alloc(n));
  AI_TRY(Y.alloc(n));
  AI_TRY(Z.alloc(n));
  uint64_t* ukey = key.p;  // the unsorted keys are dead after the sort: their buffer holds the voxel table
  hipLaunchKernelGGL(kn_gather, dim3(gb), dim3(AI_BLOCK), 0, st, dx, (const int32_t*)order.p, (const uint64_t*)skey.p,
                     (const int32_t*)vid.p, n, X.p, Y.p, Z.p, ukey);
  AI_KERNEL_CHECK();
  AI_HIP(hipStreamSynchronize(st));
  double* o = out_xyz;
  int32_t* tr = trace;
  int32_t* ni = nearest_index;
  double* nd = nearest_dist;
  if (mem_kind != AI_MEM_DEVICE) {
    AI_TRY(d_out.alloc((size_t)m * 3));
    AI_TRY(d_nn.alloc(m));
    o = d_out.p;
    ni = d_nn.p;
    if (trace) {
      AI_TRY(d_trace.alloc(n));
      tr = d_trace.p;
    }
    if (nearest_dist) {
      AI_TRY(d_dist.alloc(m));
      nd = d_dist.p;
    }
  }
  hipLaunchKernelGGL(kv_mean, dim3(grid_for(m)), dim3(AI_BLOCK), 0, st, dx, (const int32_t*)order.p, (const int32_t*)start.p, (int64_t)m,
                     o, tr);
  AI_KERNEL_CHECK();
  NGrid ng;
  for (int a = 0; a < 3; ++a) ng.vmin[a] = vmin[a];
  ng.size = voxel_size;
  ng.sy = g.sy;
  ng.sz = g.sz;
  ng.nx = 1 << bits[0];  // bits[a] <= 31: an index fits the int range
  ng.ny = 1 << bits[1];
  ng.nz = 1 << bits[2];
  hipLaunchKernelGGL(kn_nearest, dim3(grid_for(m)), dim3(AI_BLOCK), 0, st, (int64_t)m, ng, (const double*)o, (const uint64_t*)ukey,
                     (const int32_t*)start.p, (const double*)X.p, (const double*)Y.p, (const double*)Z.p, (const int32_t*)order.p, ni, nd);
  AI_KERNEL_CHECK();
  if (mem_kind != AI_MEM_DEVICE) {
    AI_HIP(hipMemcpyAsync(out_xyz, o, (size_t)m * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    AI_HIP(hipMemcpyAsync(nearest_index, ni, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (trace) AI_HIP(hipMemcpyAsync(trace, tr, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (nearest_dist) AI_HIP(hipMemcpyAsync(nearest_dist, nd, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  AI_HIP(hipStreamSynchronize(st));
  *n_out = m;
  return AI_OK;
}
