// The tail of ncuts_chunk (pipeline/ncuts/ncuts_utils.py:177-204) and get_corrected_ground (pipeline/utils/point_cloud/
// point_cloud_utils.py:331-342) for every chunk of a map in one call:
//
//   ai_chunk_finish -- per chunk: every fine (minor-voxel) point takes the group of its nearest major-voxel point
//                      (kDTree_1NN_feature_reprojection, :185-188); the chunk's ground cloud loses its statistical outliers
//                      (:191-192), then every inlier at or above mean z of the inliers + mean_height (:193-197); the fine points
//                      and the kept ground points form the merged chunk (:199).  Rules F1-F7 in include/autoinst_hip.h.
//
// All chunks lie one after the other in three arrays.  A block works for one chunk: a table of tiles (AI_BLOCK rows of a
// chunk) maps blockIdx.x to (chunk, tile), so that the chunk's record -- its two grids, its row bases -- is block-uniform.  The two
// searches are ai_nn1_project's and ai_statistical_inliers' with the chunk folded into the sort key: one radix sort per search for
// the whole map, a cell (1-NN: dense cells of 0.5 m) or row (kNN: (z, y) rows, x by binary search) base per chunk.  A chunk's
// tables only hold its own points (F1).  The kNN search body and the reductions have the shape of kq_knn_avg / kq_partial /
// kq_finish (ai_prep.hip) with the chunk in blockIdx.y, and each chunk gets the grid the single call derives from its bounds and
// size: avg, mean, std and threshold are bit-equal to ai_statistical_inliers on the chunk alone (F3).
#include <climits>
#include <cmath>
#include <cstring>

#include "ai_cells.inc"

namespace {

// one chunk: where its rows start, the cell list of its major points (1-NN) and the row list of its ground points (kNN)
struct FChunk {
  int64_t foff, moff, goff;  // first fine / major / ground row
  int32_t nf, nm, ng;
  int32_t k;                 // min(nb_neighbors, ng)
  PGrid pg;                  // 1-NN grid (ai_nn1_project's for this chunk's major points)
  double pcell;
  KGrid kg;                  // kNN grid (ai_statistical_inliers' for this chunk's ground points)
  uint32_t cellbase;         // first entry of the chunk in the dense cell table
  uint32_t rowbase;          // first entry of the chunk in the row table
};

constexpr int BB = 8;            // blocks per chunk of the bounds pass
constexpr int RED_BLOCKS = 256;  // blocks per chunk of a reduction: kq_partial's
constexpr int NSTAT = 6;         // mean, std, threshold, n_inliers, mean_z, z_limit

// the chunk whose tiles hold block blockIdx.x: the largest c with tstart[c] <= blockIdx.x (chunks without rows have no tile)
__device__ __forceinline__ int tile_chunk(const int32_t* __restrict__ tstart, int nch) {
  int a = 0, b = nch;
  while (b - a > 1) {
    const int m = (a + b) >> 1;
    if (tstart[m] <= (int32_t)blockIdx.x)
      a = m;
    else
      b = m;
  }
  return a;
}

// ----------------------------------------------------------------------------- bounds, segmented

// part[(c * BB + b) * 6 ..] = min x, y, z, max x, y, z over block b's share of chunk c = blockIdx.y.  A coordinate that is not
// finite goes in as +inf (fmin / fmax would drop a NaN), so that the host sees it in the maximum.
__global__ __launch_bounds__(AI_BLOCK) void kf_bounds(const double* __restrict__ xyz, const int64_t* __restrict__ off,
                                                      double* __restrict__ part) {
  __shared__ double sm[6][AI_BLOCK / 64];
  const int c = blockIdx.y;
  const int64_t s = off[c], e = off[c + 1];
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = s + (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x; i < e; i += (int64_t)BB * AI_BLOCK)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double v0 = xyz[i * 3 + a];
      const double v = fabs(v0) < INFINITY ? v0 : INFINITY;
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
    part[((int64_t)c * BB + blockIdx.x) * 6 + threadIdx.x] = r;
  }
}

// ----------------------------------------------------------------------------- nearest major point (F2)

// sort key: the chunk's cell base + the linear cell of the chunk's own grid; value = the global major row
__global__ __launch_bounds__(AI_BLOCK) void kf_mkeys(const double* __restrict__ xyz, const FChunk* __restrict__ tab,
                                                     const int32_t* __restrict__ tstart, int nch, uint32_t* __restrict__ key,
                                                     int32_t* __restrict__ idx) {
  const int c = tile_chunk(tstart, nch);
  const FChunk& ch = tab[c];
  const int64_t local = (int64_t)(blockIdx.x - tstart[c]) * AI_BLOCK + threadIdx.x;
  if (local >= ch.nm) return;
  const int64_t i = ch.moff + local;
  int cx, cy, cz;
  pcell_of(ch.pg, xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], cx, cy, cz);
  key[i] = ch.cellbase + (uint32_t)((cz * ch.pg.ny + cy) * ch.pg.nx + cx);
  idx[i] = (int32_t)i;
}

// One thread per fine point, a block inside one chunk: the exact nearest major point of the chunk (smallest sq_dist3, ties to the
// smaller major row; distance = its correctly rounded sqrt) by growing rings of the chunk's cells: kp_nn1's search body (ai_points.hip)
// and the ring searches' stop rule (ai_cells.inc, where it is derived), for the best.
__global__ __launch_bounds__(AI_BLOCK) void kf_nn1(const double* __restrict__ q, const FChunk* __restrict__ tab,
                                                   const int32_t* __restrict__ tstart, int nch, const double* __restrict__ X,
                                                   const double* __restrict__ Y, const double* __restrict__ Z,
                                                   const int32_t* __restrict__ order, const int32_t* __restrict__ cstart,
                                                   const int32_t* __restrict__ cend, const int32_t* __restrict__ major_label,
                                                   int32_t* __restrict__ nn_idx, double* __restrict__ nn_dist,
                                                   int32_t* __restrict__ label) {
  const int c = tile_chunk(tstart, nch);
  const FChunk& ch = tab[c];
  const int64_t local = (int64_t)(blockIdx.x - tstart[c]) * AI_BLOCK + threadIdx.x;
  if (local >= ch.nf) return;
  const int64_t i = ch.foff + local;
  const PGrid g = ch.pg;
  const double cell = ch.pcell;
  const int32_t* __restrict__ cs = cstart + ch.cellbase;
  const int32_t* __restrict__ ce = cend + ch.cellbase;
  const double x = q[i * 3], y = q[i * 3 + 1], z = q[i * 3 + 2];
  int cx, cy, cz;
  pcell_of(g, x, y, z, cx, cy, cz);
  const double eps = 2.220446049250313e-16;
  const double slack = 8.0 * eps * fmax(fmax(axis_mag(x, g.minx, cell, g.nx), axis_mag(y, g.miny, cell, g.ny)), axis_mag(z, g.minz, cell, g.nz));
  double best = 1e300;
  int32_t bi = -1;
  const int rmax = max(g.nx, max(g.ny, g.nz));
  for (int r = 0; r <= rmax; ++r) {
    for (int dz = -r; dz <= r; ++dz) {
      const int zz = cz + dz;
      if (zz < 0 || zz >= g.nz) continue;
      for (int dy = -r; dy <= r; ++dy) {
        const int yy = cy + dy;
        if (yy < 0 || yy >= g.ny) continue;
        for (int dx = -r; dx <= r; ++dx) {
          if (max(abs(dx), max(abs(dy), abs(dz))) != r) continue;  // only the shell of ring r
          const int xx = cx + dx;
          if (xx < 0 || xx >= g.nx) continue;
          const int32_t cc = (zz * g.ny + yy) * g.nx + xx;
          const int32_t s = cs[cc];
          if (s < 0) continue;
          const int32_t e = ce[cc];
          for (int32_t p = s; p < e; ++p) {
            const double d2 = sq_dist3(x, y, z, X[p], Y[p], Z[p]);
            // ties: the smaller major row wins, so the answer does not depend on the cell order
            if (d2 < best || (d2 == best && order[p] < bi)) {
              best = d2;
              bi = order[p];
            }
          }
        }
      }
    }
    const double lb = fmin(face_gap(x, g.minx, cell, cx, r, g.nx), fmin(face_gap(y, g.miny, cell, cy, r, g.ny), face_gap(z, g.minz, cell, cz, r, g.nz))) - slack;
    if (bi >= 0 && sqrt(best) * (1.0 + 4.0 * eps) <= lb) break;
  }
  if (nn_idx) nn_idx[i] = bi >= 0 ? (int32_t)(bi - ch.moff) : -1;
  if (nn_dist) nn_dist[i] = sqrt(best);
  if (label) label[i] = bi >= 0 ? major_label[bi] : -1;
}

// ----------------------------------------------------------------------------- ground inliers (F3)

// sort key: the chunk's row base + row (z, y) in the high 32 bits, the x cell in the low 32 (kq_keys with a row base)
__global__ __launch_bounds__(AI_BLOCK) void kf_gkeys(const double* __restrict__ xyz, const FChunk* __restrict__ tab,
                                                     const int32_t* __restrict__ tstart, int nch, uint64_t* __restrict__ key,
                                                     int32_t* __restrict__ idx) {
  const int c = tile_chunk(tstart, nch);
  const FChunk& ch = tab[c];
  const int64_t local = (int64_t)(blockIdx.x - tstart[c]) * AI_BLOCK + threadIdx.x;
  if (local >= ch.ng) return;
  const int64_t i = ch.goff + local;
  int cx, cy, cz;
  kcell_of(ch.kg, xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], cx, cy, cz);
  key[i] = ((uint64_t)(ch.rowbase + (uint32_t)(cz * ch.kg.ny + cy)) << 32) | (uint32_t)cx;
  idx[i] = (int32_t)i;
}

// kq_knn_avg (ai_prep.hip) inside one chunk: one thread per ground point in the chunk's cell order, the k smallest squared distances
// to the chunk's ground points by rings of the chunk's cells: kq_knn_avg's search body and the ring searches' stop rule (ai_cells.inc,
// where it is derived), for the k-th best.  The kNN is exact, so avg does not depend on the grid; the chunk still gets the single call's grid, and its sorted run starts at its first row,
// so the thread of local position p serves the point the single call's thread p serves, over the same rows.
template <int K>
__global__ __launch_bounds__(AI_BLOCK) void kf_knn_avg(const FChunk* __restrict__ tab, const int32_t* __restrict__ tstart, int nch,
                                                       const double* __restrict__ X, const double* __restrict__ Y,
                                                       const double* __restrict__ Z, const int32_t* __restrict__ scx,
                                                       const int32_t* __restrict__ rstart_all, const int32_t* __restrict__ rend_all,
                                                       const int32_t* __restrict__ order, double* __restrict__ avg) {
  const int c = tile_chunk(tstart, nch);
  const FChunk& ch = tab[c];
  const int64_t local = (int64_t)(blockIdx.x - tstart[c]) * AI_BLOCK + threadIdx.x;
  if (local >= ch.ng) return;
  const int64_t p = ch.goff + local;
  const KGrid g = ch.kg;
  const int32_t k = ch.k;
  const int32_t* __restrict__ rstart = rstart_all + ch.rowbase;
  const int32_t* __restrict__ rend = rend_all + ch.rowbase;
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

// kq_partial with the chunk in blockIdx.y: part[c * RED_BLOCKS + block] = sum over the block's fixed share of the chunk's i with
// avg[i] > 0 of (avg[i] - centre)^pw, pw = 1 or 2
__global__ __launch_bounds__(AI_BLOCK) void kf_partial(const double* __restrict__ avg_all, const FChunk* __restrict__ tab,
                                                       const double* __restrict__ stats_all, int pw, double* __restrict__ part) {
  __shared__ double sm[AI_BLOCK / 64];
  const int ch = blockIdx.y;
  const double* __restrict__ avg = avg_all + tab[ch].goff;
  const double* __restrict__ stats = stats_all + (int64_t)ch * NSTAT;
  const int64_t n = tab[ch].ng;
  const double c = pw == 2 ? stats[0] : 0.0;
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AI_BLOCK) {
    const double v = avg[i];
    if (v > 0.0) s += pw == 2 ? (v - c) * (v - c) : v;
  }
  s = ai_block_sum_first(s, sm);
  if (threadIdx.x == 0) part[(int64_t)ch * RED_BLOCKS + blockIdx.x] = s;
}

// kq_finish per chunk (block = chunk): stats[0] = mean = total / n (pw 1); stats[1] = std = sqrt(total / (n - 1)), stats[2] =
// threshold (pw 2).  A chunk without ground has no statistics: NaN.
__global__ __launch_bounds__(AI_BLOCK) void kf_finish(const double* __restrict__ part_all, const FChunk* __restrict__ tab, int pw,
                                                      double std_ratio, double* __restrict__ stats_all) {
  __shared__ double sm[AI_BLOCK / 64];
  static_assert(RED_BLOCKS == AI_BLOCK, "one partial per thread");
  const int ch = blockIdx.x;
  const double* __restrict__ part = part_all + (int64_t)ch * RED_BLOCKS;
  double* __restrict__ stats = stats_all + (int64_t)ch * NSTAT;
  const int64_t n = tab[ch].ng;
  const double t = ai_block_sum_first(part[threadIdx.x], sm);
  if (threadIdx.x == 0) {
    if (n == 0) {
      stats[0] = stats[1] = stats[2] = NAN;
    } else if (pw == 1) {
      stats[0] = t / (double)n;
    } else {
      const double sd = sqrt(t / (double)(n - 1));  // n = 1: 0 / 0, NaN, and nothing is kept (avg is 0 anyway)
      stats[1] = sd;
      stats[2] = stats[0] + std_ratio * sd;
    }
  }
}

// ----------------------------------------------------------------------------- mean height and the cut (F4, F5)

// The sum of z over a chunk's inliers (avg > 0 && avg < threshold) and their number, in F4's order: thread t of block b adds the
// chunk-local indices i = b * 256 + t, + 65536, + 2 * 65536, ... in ascending order; the block's 256 sums go through
// ai_block_sum_first (per wave a pairwise tree over the lanes: neighbours, pairs of 2, of 4, ..., of 32; then ((w0 + w1) + w2) + w3).
__global__ __launch_bounds__(AI_BLOCK) void kf_zpartial(const double* __restrict__ xyz, const double* __restrict__ avg_all,
                                                        const FChunk* __restrict__ tab, const double* __restrict__ stats_all,
                                                        double* __restrict__ part_z, double* __restrict__ part_n) {
  __shared__ double sm[AI_BLOCK / 64], sn[AI_BLOCK / 64];
  const int ch = blockIdx.y;
  const int64_t base = tab[ch].goff, n = tab[ch].ng;
  const double thr = stats_all[(int64_t)ch * NSTAT + 2];
  double s = 0.0, cnt = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AI_BLOCK) {
    const double v = avg_all[base + i];
    if (v > 0.0 && v < thr) {
      s += xyz[(base + i) * 3 + 2];
      cnt += 1.0;
    }
  }
  s = ai_block_sum_first(s, sm);
  cnt = ai_block_sum_first(cnt, sn);
  if (threadIdx.x == 0) {
    part_z[(int64_t)ch * RED_BLOCKS + blockIdx.x] = s;
    part_n[(int64_t)ch * RED_BLOCKS + blockIdx.x] = cnt;
  }
}

// the 256 block sums of a chunk through ai_block_sum_first once more; mean_z = sum / count (0 / 0 = NaN without inliers: nothing
// compares below NaN, nothing is kept), z_limit = mean_z + mean_height, one rounding each
__global__ __launch_bounds__(AI_BLOCK) void kf_zfinish(const double* __restrict__ part_z, const double* __restrict__ part_n,
                                                       double mean_height, double* __restrict__ stats_all) {
  __shared__ double sm[AI_BLOCK / 64], sn[AI_BLOCK / 64];
  const int ch = blockIdx.x;
  const double t = ai_block_sum_first(part_z[(int64_t)ch * RED_BLOCKS + threadIdx.x], sm);
  const double cnt = ai_block_sum_first(part_n[(int64_t)ch * RED_BLOCKS + threadIdx.x], sn);
  if (threadIdx.x == 0) {
    double* __restrict__ stats = stats_all + (int64_t)ch * NSTAT;
    const double mz = t / cnt;
    stats[3] = cnt;
    stats[4] = mz;
    stats[5] = mz + mean_height;
  }
}

// flag[i] = ground point i is an inlier and strictly below its chunk's z_limit
__global__ __launch_bounds__(AI_BLOCK) void kf_keep_flags(const double* __restrict__ xyz, const double* __restrict__ avg,
                                                          const FChunk* __restrict__ tab, const int32_t* __restrict__ tstart, int nch,
                                                          const double* __restrict__ stats_all, int32_t* __restrict__ flag) {
  const int c = tile_chunk(tstart, nch);
  const FChunk& ch = tab[c];
  const int64_t local = (int64_t)(blockIdx.x - tstart[c]) * AI_BLOCK + threadIdx.x;
  if (local >= ch.ng) return;
  const int64_t i = ch.goff + local;
  const double v = avg[i];
  flag[i] = (v > 0.0 && v < stats_all[(int64_t)c * NSTAT + 2] && xyz[i * 3 + 2] < stats_all[(int64_t)c * NSTAT + 5]) ? 1 : 0;
}

// ----------------------------------------------------------------------------- compaction and the merged chunks (F5, F6)

// koff[c] = kept ground points before chunk c (pos = exclusive scan of the flags); koff[nch] = their total
__global__ void kf_keep_offsets(const int32_t* __restrict__ pos, const int64_t* __restrict__ goff, int nch, int64_t* __restrict__ koff) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c <= nch) koff[c] = pos[goff[c]];
}

// a kept ground point goes to ground_keep (its chunk-local index; ascending, as the scan is) and behind its chunk's fine points
__global__ __launch_bounds__(AI_BLOCK) void kf_write_ground(const double* __restrict__ xyz, const int32_t* __restrict__ pos,
                                                            const FChunk* __restrict__ tab, const int32_t* __restrict__ tstart, int nch,
                                                            int32_t* __restrict__ keep, double* __restrict__ mxyz,
                                                            int32_t* __restrict__ mlabel) {
  const int c = tile_chunk(tstart, nch);
  const FChunk& ch = tab[c];
  const int64_t local = (int64_t)(blockIdx.x - tstart[c]) * AI_BLOCK + threadIdx.x;
  if (local >= ch.ng) return;
  const int64_t i = ch.goff + local;
  const int32_t q = pos[i];
  if (pos[i + 1] == q) return;
  if (keep) keep[q] = (int32_t)local;
  if (mxyz) {
    const int64_t d = ch.foff + ch.nf + q;  // merged_off[c] + nf + (q - koff[c]), merged_off[c] = foff + koff[c]
    mxyz[d * 3] = xyz[i * 3];
    mxyz[d * 3 + 1] = xyz[i * 3 + 1];
    mxyz[d * 3 + 2] = xyz[i * 3 + 2];
    mlabel[d] = 0;
  }
}

__global__ __launch_bounds__(AI_BLOCK) void kf_write_fine(const double* __restrict__ xyz, const int32_t* __restrict__ label,
                                                          const FChunk* __restrict__ tab, const int32_t* __restrict__ tstart, int nch,
                                                          const int64_t* __restrict__ koff, double* __restrict__ mxyz,
                                                          int32_t* __restrict__ mlabel) {
  const int c = tile_chunk(tstart, nch);
  const FChunk& ch = tab[c];
  const int64_t local = (int64_t)(blockIdx.x - tstart[c]) * AI_BLOCK + threadIdx.x;
  if (local >= ch.nf) return;
  const int64_t i = ch.foff + local, d = i + koff[c];
  mxyz[d * 3] = xyz[i * 3];
  mxyz[d * 3 + 1] = xyz[i * 3 + 1];
  mxyz[d * 3 + 2] = xyz[i * 3 + 2];
  mlabel[d] = label[i] + 1;
}

// ----------------------------------------------------------------------------- host

int check_offsets(const int64_t* off, int32_t n, const char* name) {
  if (off[0] != 0) {
    ai_set_error("ai_chunk_finish: %s must start at 0", name);
    return AI_ERR_BAD_ARG;
  }
  for (int32_t c = 0; c < n; ++c)
    if (off[c + 1] < off[c]) {
      ai_set_error("ai_chunk_finish: %s decreases at chunk %d", name, c);
      return AI_ERR_BAD_ARG;
    }
  if (off[n] >= ((int64_t)1 << 30)) {
    ai_set_error("ai_chunk_finish: %s ends at %lld rows (the limit is 2^30 - 1)", name, (long long)off[n]);
    return AI_ERR_BAD_ARG;
  }
  return AI_OK;
}

// min / max of a chunk from its BB partial rows; AI_ERR_BAD_ARG when a coordinate is not finite
int chunk_bounds(const double* hp, int c, double mn[3], double mx[3], const char* cloud) {
  for (int a = 0; a < 3; ++a) {
    mn[a] = INFINITY;
    mx[a] = -INFINITY;
  }
  for (int b = 0; b < BB; ++b)
    for (int a = 0; a < 3; ++a) {
      mn[a] = std::min(mn[a], hp[((size_t)c * BB + b) * 6 + a]);
      mx[a] = std::max(mx[a], hp[((size_t)c * BB + b) * 6 + 3 + a]);
    }
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(mn[a]) || !std::isfinite(mx[a]) || !(mx[a] - mn[a] < 1e15)) {
      ai_set_error("ai_chunk_finish: the %s coordinates of chunk %d are not finite", cloud, c);
      return AI_ERR_BAD_ARG;
    }
  return AI_OK;
}

void tiles_of(const int64_t* off, int32_t n, std::vector<int32_t>& t) {
  t.assign((size_t)n + 1, 0);
  for (int32_t c = 0; c < n; ++c) t[c + 1] = t[c] + (int32_t)((off[c + 1] - off[c] + AI_BLOCK - 1) / AI_BLOCK);
}

}  // namespace

extern "C" int ai_chunk_finish(ai_ctx* ctx, const double* fine_xyz, const int64_t* fine_off, const double* major_xyz,
                               const int64_t* major_off, const int32_t* major_label, const double* ground_xyz,
                               const int64_t* ground_off, int32_t n_chunks, int32_t nb_neighbors, double std_ratio, double mean_height,
                               int mem_kind, int32_t* fine_nn, double* fine_dist, int32_t* fine_label, double* ground_avg,
                               int32_t* ground_keep, int64_t* keep_off, double* ground_stats, double* merged_xyz, int32_t* merged_label,
                               int64_t* merged_off) {
  if (!ctx || !fine_off || !major_off || !ground_off || n_chunks < 0 || n_chunks > 65535) {
    ai_set_error("ai_chunk_finish: bad argument (null context or offsets, or n_chunks outside 0 .. 65535)");
    return AI_ERR_BAD_ARG;
  }
  AI_TRY(check_offsets(fine_off, n_chunks, "fine_off"));
  AI_TRY(check_offsets(major_off, n_chunks, "major_off"));
  AI_TRY(check_offsets(ground_off, n_chunks, "ground_off"));
  const int64_t Nf = fine_off[n_chunks], Nm = major_off[n_chunks], Ng = ground_off[n_chunks];
  if ((Nf > 0 && !fine_xyz) || (Nm > 0 && !major_xyz) || (Ng > 0 && !ground_xyz)) {
    ai_set_error("ai_chunk_finish: a point array is NULL");
    return AI_ERR_BAD_ARG;
  }
  if (fine_label && !major_label) {
    ai_set_error("ai_chunk_finish: fine_label needs major_label");
    return AI_ERR_BAD_ARG;
  }
  const int n_merged = (merged_xyz ? 1 : 0) + (merged_label ? 1 : 0) + (merged_off ? 1 : 0);
  if (n_merged != 0 && n_merged != 3) {
    ai_set_error("ai_chunk_finish: merged_xyz, merged_label and merged_off must be all NULL or all given");
    return AI_ERR_BAD_ARG;
  }
  if (n_merged && !major_label) {
    ai_set_error("ai_chunk_finish: the merged outputs need major_label");
    return AI_ERR_BAD_ARG;
  }
  if (nb_neighbors < 1 || !(std_ratio > 0.0)) {  // open3d: "Illegal input parameters, ... must be positive"
    ai_set_error("ai_chunk_finish: nb_neighbors must be >= 1 and std_ratio > 0");
    return AI_ERR_BAD_ARG;
  }
  if (!std::isfinite(mean_height)) {
    ai_set_error("ai_chunk_finish: mean_height is not finite");
    return AI_ERR_BAD_ARG;
  }
  int64_t ng_max = 0;
  for (int32_t c = 0; c < n_chunks; ++c) {
    if (fine_off[c + 1] > fine_off[c] && major_off[c + 1] == major_off[c]) {
      ai_set_error("ai_chunk_finish: chunk %d has fine points and no major points", c);
      return AI_ERR_BAD_ARG;
    }
    ng_max = std::max(ng_max, ground_off[c + 1] - ground_off[c]);
  }
  if (nb_neighbors > 64 && ng_max > 64) {
    ai_set_error("ai_chunk_finish: nb_neighbors > 64 is not supported");
    return AI_ERR_BAD_ARG;
  }
  const bool merged = n_merged == 3;
  const bool want_fine = Nf > 0 && (fine_nn || fine_dist || fine_label || merged);
  const bool want_ground = ground_avg || ground_keep || keep_off || ground_stats || merged;

  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  const bool dev = mem_kind == AI_MEM_DEVICE;
  const int nch = n_chunks;
  DevBuf<double> own_f, own_m, own_g;
  DevBuf<int32_t> own_l;
  const double *df = nullptr, *dm = nullptr, *dg = nullptr;
  const int32_t* dl = nullptr;
  if (Nf) AI_TRY(to_device(fine_xyz, (size_t)Nf * 3, mem_kind, own_f, &df, st));
  if (Nm) AI_TRY(to_device(major_xyz, (size_t)Nm * 3, mem_kind, own_m, &dm, st));
  if (Ng) AI_TRY(to_device(ground_xyz, (size_t)Ng * 3, mem_kind, own_g, &dg, st));
  if (Nm && major_label) AI_TRY(to_device(major_label, (size_t)Nm, mem_kind, own_l, &dl, st));

  // ---- bounds of every chunk's three clouds: the one synchronisation in front of the searches
  std::vector<int64_t> h_foff(fine_off, fine_off + nch + 1), h_moff(major_off, major_off + nch + 1), h_goff(ground_off, ground_off + nch + 1);
  DevBuf<int64_t> d_foff, d_moff, d_goff;
  AI_TRY(upload(h_foff, d_foff, st));
  AI_TRY(upload(h_moff, d_moff, st));
  AI_TRY(upload(h_goff, d_goff, st));
  const size_t per = (size_t)nch * BB * 6;
  std::vector<double> hp(3 * per);
  DevBuf<double> d_part;
  AI_TRY(d_part.alloc(3 * per));
  if (nch > 0 && Nf + Nm + Ng > 0) {
    const double* src[3] = {df, dm, dg};
    const int64_t* off[3] = {d_foff.p, d_moff.p, d_goff.p};
    const int64_t cnt[3] = {Nf, Nm, Ng};
    for (int a = 0; a < 3; ++a)
      if (cnt[a]) {
        hipLaunchKernelGGL(kf_bounds, dim3(BB, nch), dim3(AI_BLOCK), 0, st, src[a], off[a], d_part.p + a * per);
        AI_KERNEL_CHECK();
        AI_HIP(hipMemcpyAsync(hp.data() + a * per, d_part.p + a * per, per * sizeof(double), hipMemcpyDeviceToHost, st));
      }
    AI_HIP(hipStreamSynchronize(st));
  }

  // ---- the chunk table: each chunk gets the grids the single-cloud entries derive from its bounds and its size
  std::vector<FChunk> tab((size_t)nch);
  const double cell_cap = std::max(64.0, (double)((int64_t)1 << 27) / (double)std::max(nch, 1));  // dense cells per chunk
  int64_t ncell = 0, nrow = 0;
  int32_t k_max = 0;
  for (int c = 0; c < nch; ++c) {
    FChunk& ch = tab[c];
    memset(&ch, 0, sizeof(ch));
    ch.foff = fine_off[c];
    ch.moff = major_off[c];
    ch.goff = ground_off[c];
    ch.nf = (int32_t)(fine_off[c + 1] - fine_off[c]);
    ch.nm = (int32_t)(major_off[c + 1] - major_off[c]);
    ch.ng = (int32_t)(ground_off[c + 1] - ground_off[c]);
    ch.k = (int32_t)std::min<int64_t>(nb_neighbors, ch.ng);
    k_max = std::max(k_max, ch.k);
    double mn[3], mx[3];
    if (ch.nf) AI_TRY(chunk_bounds(hp.data(), c, mn, mx, "fine"));
    ch.cellbase = (uint32_t)ncell;
    if (ch.nm) {
      AI_TRY(chunk_bounds(hp.data() + per, c, mn, mx, "major"));
      // ai_nn1_project's grid: 0.5 m cells, grown until the chunk's dense table fits its share
      double cell = 0.5;
      for (;;) {
        const double ex = (mx[0] - mn[0]) / cell, ey = (mx[1] - mn[1]) / cell, ez = (mx[2] - mn[2]) / cell;
        if ((floor(ex) + 1) * (floor(ey) + 1) * (floor(ez) + 1) <= cell_cap) break;
        cell *= 1.5;
      }
      ch.pcell = cell;
      ch.pg.minx = mn[0];
      ch.pg.miny = mn[1];
      ch.pg.minz = mn[2];
      ch.pg.inv_cell = 1.0 / cell;
      ch.pg.nx = (int)floor((mx[0] - mn[0]) / cell) + 1;
      ch.pg.ny = (int)floor((mx[1] - mn[1]) / cell) + 1;
      ch.pg.nz = (int)floor((mx[2] - mn[2]) / cell) + 1;
      ncell += (int64_t)ch.pg.nx * ch.pg.ny * ch.pg.nz;
    }
    ch.rowbase = (uint32_t)nrow;
    if (ch.ng) {
      AI_TRY(chunk_bounds(hp.data() + 2 * per, c, mn, mx, "ground"));
      // ai_statistical_inliers' grid, step for step: the side of the bounding box's volume per point (thin axes count as 1e-3 of
      // the widest), grown until the x cells fit their key half and the row table has at most 2 n + 1024 entries
      const int64_t n = ch.ng;
      double ext[3], emax = 0.0;
      for (int a = 0; a < 3; ++a) emax = std::max(emax, mx[a] - mn[a]);
      double vol = 1.0;
      for (int a = 0; a < 3; ++a) {
        ext[a] = mx[a] - mn[a];
        vol *= std::max(ext[a], std::max(1e-3 * emax, 1e-9));
      }
      double cell = std::cbrt(vol / (double)n);
      KGrid& g = ch.kg;
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
      nrow += (int64_t)g.ny * g.nz;
    }
  }
  // ncell <= 2^27 + 64 * 65535 and nrow <= 2 * 2^30 + 1024 * 65535: both bases fit 32 bits
  std::vector<int32_t> h_tf, h_tm, h_tg;
  tiles_of(fine_off, nch, h_tf);
  tiles_of(major_off, nch, h_tm);
  tiles_of(ground_off, nch, h_tg);
  DevBuf<FChunk> d_tab;
  DevBuf<int32_t> d_tf, d_tm, d_tg;
  AI_TRY(upload(tab, d_tab, st));
  AI_TRY(upload(h_tf, d_tf, st));
  AI_TRY(upload(h_tm, d_tm, st));
  AI_TRY(upload(h_tg, d_tg, st));
  const unsigned tiles_f = (unsigned)h_tf[nch], tiles_m = (unsigned)h_tm[nch], tiles_g = (unsigned)h_tg[nch];
  const FChunk* T = d_tab.p;

  // ---- F2: nearest major point of every fine point
  DevBuf<uint32_t> mkey, mskey;
  DevBuf<int32_t> midx, morder, cstart, cend, d_nn, d_label;
  DevBuf<double> MX, MY, MZ, d_dist;
  DevBuf<uint8_t> sort_tmp_m, sort_tmp_g;
  int32_t *o_nn = nullptr, *o_label = nullptr;
  double* o_dist = nullptr;
  if (want_fine) {
    AI_TRY(mkey.alloc(Nm));
    AI_TRY(mskey.alloc(Nm));
    AI_TRY(midx.alloc(Nm));
    AI_TRY(morder.alloc(Nm));
    AI_TRY(cstart.alloc(ncell));
    AI_TRY(cend.alloc(ncell));
    AI_TRY(MX.alloc(Nm));
    AI_TRY(MY.alloc(Nm));
    AI_TRY(MZ.alloc(Nm));
    hipLaunchKernelGGL(kf_mkeys, dim3(tiles_m), dim3(AI_BLOCK), 0, st, dm, T, (const int32_t*)d_tm.p, nch, mkey.p, midx.p);
    AI_KERNEL_CHECK();
    AI_TRY(sort_pairs(st, mkey.p, mskey.p, midx.p, morder.p, Nm, std::max(1, bits_for(ncell)), sort_tmp_m));
    AI_HIP(hipMemsetAsync(cstart.p, 0xff, (size_t)ncell * sizeof(int32_t), st));
    AI_HIP(hipMemsetAsync(cend.p, 0, (size_t)ncell * sizeof(int32_t), st));
    // kp_gather (ai_cells.inc): the sorted coordinates and the [start, end) run of every occupied cell; a chunk's cells are a range of
    // their own in the table, so its runs never hold another chunk's point
    hipLaunchKernelGGL(kp_gather, dim3(grid_for(Nm)), dim3(AI_BLOCK), 0, st, dm, (const int32_t*)morder.p,
                       (const uint32_t*)mskey.p, Nm, MX.p, MY.p, MZ.p, cstart.p, cend.p);
    AI_KERNEL_CHECK();
    o_nn = fine_nn;
    o_dist = fine_dist;
    o_label = fine_label;
    if (!dev && fine_nn) {
      AI_TRY(d_nn.alloc(Nf));
      o_nn = d_nn.p;
    }
    if (!dev && fine_dist) {
      AI_TRY(d_dist.alloc(Nf));
      o_dist = d_dist.p;
    }
    if ((!dev && fine_label) || (merged && !fine_label)) {
      AI_TRY(d_label.alloc(Nf));
      o_label = d_label.p;
    }
    hipLaunchKernelGGL(kf_nn1, dim3(tiles_f), dim3(AI_BLOCK), 0, st, df, T, (const int32_t*)d_tf.p, nch, (const double*)MX.p,
                       (const double*)MY.p, (const double*)MZ.p, (const int32_t*)morder.p, (const int32_t*)cstart.p,
                       (const int32_t*)cend.p, dl, o_nn, o_dist, o_label);
    AI_KERNEL_CHECK();
  }

  // ---- F3-F5: the ground of every chunk
  DevBuf<uint64_t> gkey, gskey;
  DevBuf<int32_t> gidx, gorder, scx, rstart, rend, flag, scan_tmp, d_keep;
  DevBuf<double> GX, GY, GZ, d_avg, part, part_n, d_stats;
  DevBuf<int64_t> d_koff;
  double* avg = nullptr;
  int32_t* o_keep = nullptr;
  std::vector<int64_t> h_koff((size_t)nch + 1, 0);
  std::vector<double> h_stats((size_t)nch * NSTAT, NAN);
  if (want_ground && nch > 0) {
    AI_TRY(d_stats.alloc((size_t)nch * NSTAT));
    AI_TRY(part.alloc((size_t)nch * RED_BLOCKS));
    AI_TRY(part_n.alloc((size_t)nch * RED_BLOCKS));
    AI_TRY(flag.alloc(Ng + 1));
    AI_TRY(scan_tmp.alloc(ai_scan_tmp_elems(Ng)));
    AI_TRY(d_koff.alloc((size_t)nch + 1));
    avg = ground_avg;
    if (!dev || !ground_avg) {
      AI_TRY(d_avg.alloc(Ng));
      avg = d_avg.p;
    }
    if (Ng) {
      AI_TRY(gkey.alloc(Ng));
      AI_TRY(gskey.alloc(Ng));
      AI_TRY(gidx.alloc(Ng));
      AI_TRY(gorder.alloc(Ng));
      AI_TRY(GX.alloc(Ng));
      AI_TRY(GY.alloc(Ng));
      AI_TRY(GZ.alloc(Ng));
      AI_TRY(scx.alloc(Ng));
      AI_TRY(rstart.alloc(nrow));
      AI_TRY(rend.alloc(nrow));
      hipLaunchKernelGGL(kf_gkeys, dim3(tiles_g), dim3(AI_BLOCK), 0, st, dg, T, (const int32_t*)d_tg.p, nch, gkey.p, gidx.p);
      AI_KERNEL_CHECK();
      AI_TRY(sort_pairs(st, gkey.p, gskey.p, gidx.p, gorder.p, Ng, 32 + std::max(1, bits_for(nrow)), sort_tmp_g));
      AI_HIP(hipMemsetAsync(rstart.p, 0, (size_t)nrow * sizeof(int32_t), st));
      AI_HIP(hipMemsetAsync(rend.p, 0, (size_t)nrow * sizeof(int32_t), st));
      hipLaunchKernelGGL(kq_gather, dim3(grid_for(Ng)), dim3(AI_BLOCK), 0, st, dg, (const int32_t*)gorder.p,
                         (const uint64_t*)gskey.p, Ng, GX.p, GY.p, GZ.p, scx.p, rstart.p, rend.p);
      AI_KERNEL_CHECK();
#define KF_ARGS                                                                                                                     \
  dim3(tiles_g), dim3(AI_BLOCK), 0, st, T, (const int32_t*)d_tg.p, nch, (const double*)GX.p, (const double*)GY.p, (const double*)GZ.p, \
      (const int32_t*)scx.p, (const int32_t*)rstart.p, (const int32_t*)rend.p, (const int32_t*)gorder.p, avg
      if (k_max <= 20)
        hipLaunchKernelGGL(kf_knn_avg<20>, KF_ARGS);
      else if (k_max <= 32)
        hipLaunchKernelGGL(kf_knn_avg<32>, KF_ARGS);
      else
        hipLaunchKernelGGL(kf_knn_avg<64>, KF_ARGS);
#undef KF_ARGS
      AI_KERNEL_CHECK();
    }
    const double* S = d_stats.p;
    for (int pw = 1; pw <= 2; ++pw) {
      hipLaunchKernelGGL(kf_partial, dim3(RED_BLOCKS, nch), dim3(AI_BLOCK), 0, st, (const double*)avg, T, S, pw, part.p);
      AI_KERNEL_CHECK();
      hipLaunchKernelGGL(kf_finish, dim3(nch), dim3(AI_BLOCK), 0, st, (const double*)part.p, T, pw, std_ratio, d_stats.p);
      AI_KERNEL_CHECK();
    }
    hipLaunchKernelGGL(kf_zpartial, dim3(RED_BLOCKS, nch), dim3(AI_BLOCK), 0, st, dg, (const double*)avg, T, S, part.p, part_n.p);
    AI_KERNEL_CHECK();
    hipLaunchKernelGGL(kf_zfinish, dim3(nch), dim3(AI_BLOCK), 0, st, (const double*)part.p, (const double*)part_n.p, mean_height,
                       d_stats.p);
    AI_KERNEL_CHECK();
    if (Ng) {
      hipLaunchKernelGGL(kf_keep_flags, dim3(tiles_g), dim3(AI_BLOCK), 0, st, dg, (const double*)avg, T, (const int32_t*)d_tg.p, nch, S,
                         flag.p);
      AI_KERNEL_CHECK();
    }
    AI_TRY(ai_exclusive_scan_i32(st, flag.p, flag.p, Ng, scan_tmp.p));
    hipLaunchKernelGGL(kf_keep_offsets, dim3((unsigned)((nch + 1 + 63) / 64)), dim3(64), 0, st, (const int32_t*)flag.p,
                       (const int64_t*)d_goff.p, nch, d_koff.p);
    AI_KERNEL_CHECK();
  }

  // ---- F5, F6: the kept indices and the merged chunks
  DevBuf<double> d_mxyz;
  DevBuf<int32_t> d_mlabel;
  double* o_mxyz = merged_xyz;
  int32_t* o_mlabel = merged_label;
  if (merged && !dev) {
    AI_TRY(d_mxyz.alloc((size_t)(Nf + Ng) * 3));
    AI_TRY(d_mlabel.alloc((size_t)(Nf + Ng)));
    o_mxyz = d_mxyz.p;
    o_mlabel = d_mlabel.p;
  }
  if (want_ground && nch > 0) {
    o_keep = ground_keep;
    if (!dev && ground_keep) {
      AI_TRY(d_keep.alloc(Ng));
      o_keep = d_keep.p;
    }
    if (Ng && (o_keep || merged)) {
      hipLaunchKernelGGL(kf_write_ground, dim3(tiles_g), dim3(AI_BLOCK), 0, st, dg, (const int32_t*)flag.p, T, (const int32_t*)d_tg.p, nch,
                         o_keep, merged ? o_mxyz : nullptr, o_mlabel);
      AI_KERNEL_CHECK();
    }
    if (merged && Nf) {
      hipLaunchKernelGGL(kf_write_fine, dim3(tiles_f), dim3(AI_BLOCK), 0, st, df, (const int32_t*)o_label, T, (const int32_t*)d_tf.p, nch,
                         (const int64_t*)d_koff.p, o_mxyz, o_mlabel);
      AI_KERNEL_CHECK();
    }
    AI_HIP(hipMemcpyAsync(h_koff.data(), d_koff.p, ((size_t)nch + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    AI_HIP(hipMemcpyAsync(h_stats.data(), d_stats.p, (size_t)nch * NSTAT * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  AI_HIP(hipStreamSynchronize(st));  // the second synchronisation: the kept counts and the statistics are on the host
  const int64_t n_keep = h_koff[nch];
  if (!dev) {
    if (want_fine) {
      if (fine_nn) AI_HIP(hipMemcpyAsync(fine_nn, o_nn, (size_t)Nf * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      if (fine_dist) AI_HIP(hipMemcpyAsync(fine_dist, o_dist, (size_t)Nf * sizeof(double), hipMemcpyDeviceToHost, st));
      if (fine_label) AI_HIP(hipMemcpyAsync(fine_label, o_label, (size_t)Nf * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    if (ground_avg && Ng) AI_HIP(hipMemcpyAsync(ground_avg, avg, (size_t)Ng * sizeof(double), hipMemcpyDeviceToHost, st));
    if (ground_keep && n_keep) AI_HIP(hipMemcpyAsync(ground_keep, o_keep, (size_t)n_keep * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (merged && Nf + n_keep) {
      AI_HIP(hipMemcpyAsync(merged_xyz, o_mxyz, (size_t)(Nf + n_keep) * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
      AI_HIP(hipMemcpyAsync(merged_label, o_mlabel, (size_t)(Nf + n_keep) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    AI_HIP(hipStreamSynchronize(st));  // host memory only: the third
  }
  if (keep_off) memcpy(keep_off, h_koff.data(), ((size_t)nch + 1) * sizeof(int64_t));
  if (ground_stats && nch) memcpy(ground_stats, h_stats.data(), (size_t)nch * NSTAT * sizeof(double));
  if (merged)
    for (int c = 0; c <= nch; ++c) merged_off[c] = fine_off[c] + h_koff[c];
  return AI_OK;
}
