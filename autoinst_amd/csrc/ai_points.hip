// The two point-cloud steps on either side of the NCuts hot path ("next" rows 1-2),
// on the same uniform-cell-list machinery as the affinity build:
//
//   ai_radius_mean_pool  -- pipeline/utils/point_cloud/chunk_generation.py:243-256: for every major-voxel
//                           point, the mean of the TARL features of all scan points within
//                           MAJOR_VOXEL_SIZE / 2 (zero row if none)  -> the (N, 96) float64 matrix that
//                           ncuts_utils.py:136-142 feeds to the TARL factor;
//   ai_nn1_project       -- pipeline/utils/point_cloud/point_cloud_utils.py:144-174
//                           (kDTree_1NN_feature_reprojection): every fine point takes the label of its
//                           nearest major-voxel point (optionally only within max_radius).
//
// The reference does both with a Python loop over points around an open3d KD-tree query.
#include <cstring>

#include "ai_cells.inc"

namespace {

// 16 lanes per query point: mean of the float32 feature rows of all source points whose squared
// distance (sq_dist3) is strictly below radius * radius rounded once -- nanoflann's radius search,
// to which open3d passes the squared radius -- accumulated in float64 like np.mean over the float64
// copy the reference holds.
__global__ __launch_bounds__(AI_BLOCK) void kp_radius_mean(const double* __restrict__ q, int64_t nq, PGrid g, double radius,
                                                           const double* __restrict__ X, const double* __restrict__ Y,
                                                           const double* __restrict__ Z, const int32_t* __restrict__ order,
                                                           const int32_t* __restrict__ cstart, const int32_t* __restrict__ cend,
                                                           const float* __restrict__ feat, int32_t dim, double* __restrict__ out,
                                                           int32_t* __restrict__ count) {
  const int64_t gid = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const int64_t i = gid >> 4;
  const int t = (int)(gid & 15);
  if (i >= nq) return;
  const double x = q[i * 3], y = q[i * 3 + 1], z = q[i * 3 + 2];
  int cx, cy, cz;
  // a query may lie outside the sources' bounding box: clamp, the +-1 ring still covers radius <= cell
  pcell_of(g, x, y, z, cx, cy, cz);
  constexpr int MAXK = 24;  // dim <= 384
  double acc[MAXK];
#pragma unroll
  for (int k = 0; k < MAXK; ++k) acc[k] = 0.0;
  int cnt = 0;
  const double r2 = radius * radius;
  for (int dz = -1; dz <= 1; ++dz) {
    const int zz = cz + dz;
    if (zz < 0 || zz >= g.nz) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = cy + dy;
      if (yy < 0 || yy >= g.ny) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int xx = cx + dx;
        if (xx < 0 || xx >= g.nx) continue;
        const int32_t cc = (zz * g.ny + yy) * g.nx + xx;
        const int32_t s = cstart[cc];
        if (s < 0) continue;
        const int32_t e = cend[cc];
        for (int32_t p = s; p < e; ++p) {
          if (sq_dist3(x, y, z, X[p], Y[p], Z[p]) < r2) {
            const float* f = feat + (int64_t)order[p] * dim;
#pragma unroll
            for (int k = 0; k < MAXK; ++k) {
              const int c = t + 16 * k;
              if (c < dim) acc[k] += (double)f[c];
            }
            ++cnt;
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    const int c = t + 16 * k;
    if (c < dim) out[i * dim + c] = cnt ? acc[k] / (double)cnt : 0.0;  // np.mean: sum, then one division
  }
  if (t == 0 && count) count[i] = cnt;
}

// One thread per fine point: exact nearest source point (smallest sq_dist3, ties to the smaller source index; distance = its
// correctly rounded sqrt) by growing rings of cells.  Stop rule: the ring searches' (ai_cells.inc, where it is derived), for the best.
__global__ __launch_bounds__(AI_BLOCK) void kp_nn1(const double* __restrict__ q, int64_t nq, PGrid g, double cell,
                                                   const double* __restrict__ X, const double* __restrict__ Y,
                                                   const double* __restrict__ Z, const int32_t* __restrict__ order,
                                                   const int32_t* __restrict__ cstart, const int32_t* __restrict__ cend,
                                                   int32_t* __restrict__ nn_idx, double* __restrict__ nn_dist) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= nq) return;
  const double x = q[i * 3], y = q[i * 3 + 1], z = q[i * 3 + 2];
  if (!(fabs(x) < INFINITY && fabs(y) < INFINITY && fabs(z) < INFINITY)) {
    // no square of a NaN or infinite query compares below any other: no nearest source, and no walk over the whole grid
    nn_idx[i] = -1;
    if (nn_dist) nn_dist[i] = NAN;
    return;
  }
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
          const int32_t s = cstart[cc];
          if (s < 0) continue;
          const int32_t e = cend[cc];
          for (int32_t p = s; p < e; ++p) {
            const double d2 = sq_dist3(x, y, z, X[p], Y[p], Z[p]);
            // ties: the smaller source index wins, so the answer does not depend on the cell order
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
  nn_idx[i] = bi;
  if (nn_dist) nn_dist[i] = sqrt(best);
}

}  // namespace

extern "C" int ai_radius_mean_pool(ai_ctx* ctx, const double* query_xyz, int64_t nq, const double* src_xyz, int64_t ns,
                                   const float* src_feat, int32_t dim, double radius, int mem_kind, double* out, int32_t* count_out) {
  if (!ctx || !query_xyz || !src_xyz || !src_feat || !out || nq <= 0 || ns <= 0 || dim <= 0 || dim > 384 || !(radius > 0.0) ||
      nq >= ((int64_t)1 << 30) || ns >= ((int64_t)1 << 30)) {
    ai_set_error("ai_radius_mean_pool: bad argument (null pointer, empty input, dim > 384 or radius <= 0)");
    return AI_ERR_BAD_ARG;
  }
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<double> own_q, own_s, d_out;
  DevBuf<float> own_f;
  DevBuf<int32_t> d_cnt;
  const double *dq, *ds;
  const float* df;
  AI_TRY(to_device(query_xyz, (size_t)nq * 3, mem_kind, own_q, &dq, st));
  AI_TRY(to_device(src_xyz, (size_t)ns * 3, mem_kind, own_s, &ds, st));
  AI_TRY(to_device(src_feat, (size_t)ns * dim, mem_kind, own_f, &df, st));
  Cells C;
  AI_TRY(build_cells(ctx, ds, ns, radius * (1.0 + 1e-9), C, "ai_radius_mean_pool"));
  double* o = out;
  int32_t* c = count_out;
  if (mem_kind != AI_MEM_DEVICE) {
    AI_TRY(d_out.alloc((size_t)nq * dim));
    AI_TRY(d_cnt.alloc(nq));
    o = d_out.p;
    c = d_cnt.p;
  }
  const unsigned gq = grid_for(nq * 16);
  hipLaunchKernelGGL(kp_radius_mean, dim3(gq), dim3(AI_BLOCK), 0, st, dq, nq, C.g, radius, (const double*)C.X.p, (const double*)C.Y.p,
                     (const double*)C.Z.p, (const int32_t*)C.order.p, (const int32_t*)C.cstart.p, (const int32_t*)C.cend.p, df, dim, o, c);
  AI_KERNEL_CHECK();
  if (mem_kind != AI_MEM_DEVICE) {
    AI_HIP(hipMemcpyAsync(out, o, (size_t)nq * dim * sizeof(double), hipMemcpyDeviceToHost, st));
    if (count_out) AI_HIP(hipMemcpyAsync(count_out, c, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  }
  AI_HIP(hipStreamSynchronize(st));
  return AI_OK;
}

extern "C" int ai_nn1_project(ai_ctx* ctx, const double* to_xyz, int64_t nt, const double* from_xyz, int64_t nf, int mem_kind,
                              int32_t* nn_index, double* nn_dist) {
  if (!ctx || !to_xyz || !from_xyz || !nn_index || nt <= 0 || nf <= 0 || nt >= ((int64_t)1 << 30) || nf >= ((int64_t)1 << 30)) {
    ai_set_error("ai_nn1_project: bad argument");
    return AI_ERR_BAD_ARG;
  }
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<double> own_t, own_f, d_dist;
  DevBuf<int32_t> d_idx;
  const double *dt, *dfm;
  AI_TRY(to_device(to_xyz, (size_t)nt * 3, mem_kind, own_t, &dt, st));
  AI_TRY(to_device(from_xyz, (size_t)nf * 3, mem_kind, own_f, &dfm, st));
  // 0.5 m cells: a couple of 0.35 m major-voxel points per cell on a surface-like cloud
  Cells C;
  AI_TRY(build_cells(ctx, dfm, nf, 0.5, C, "ai_nn1_project"));
  int32_t* oi = nn_index;
  double* od = nn_dist;
  if (mem_kind != AI_MEM_DEVICE) {
    AI_TRY(d_idx.alloc(nt));
    AI_TRY(d_dist.alloc(nt));
    oi = d_idx.p;
    od = d_dist.p;
  }
  const unsigned gq = grid_for(nt);
  hipLaunchKernelGGL(kp_nn1, dim3(gq), dim3(AI_BLOCK), 0, st, dt, nt, C.g, C.cell, (const double*)C.X.p, (const double*)C.Y.p,
                     (const double*)C.Z.p, (const int32_t*)C.order.p, (const int32_t*)C.cstart.p, (const int32_t*)C.cend.p, oi, od);
  AI_KERNEL_CHECK();
  if (mem_kind != AI_MEM_DEVICE) {
    AI_HIP(hipMemcpyAsync(nn_index, oi, (size_t)nt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (nn_dist) AI_HIP(hipMemcpyAsync(nn_dist, od, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  AI_HIP(hipStreamSynchronize(st));
  return AI_OK;
}
