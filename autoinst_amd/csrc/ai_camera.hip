// The camera projection of the tri-modal configuration: image_based_features_per_patch (pipeline/utils/image/image_utils.py:
// 146-348, with point_to_pixel of pipeline/utils/image/point_to_pixels.py:6-35) and dinov2_mean (image_utils.py:363-371) for
// every (major-voxel point, view) pair of a chunk at once:
//
//   ai_camera_project -- a point is seen by a view iff a point of the view's visible set lies within max_dist of it in the
//                        camera frame (the reference's KD-tree 1-NN followed by norm < MAJOR_VOXEL_SIZE / 2); a seen point is
//                        projected through K and rounded half to even; a pixel inside the image gives its SAM label and the
//                        DINOv2 cell under it, and the mean of the non-zero cells over the views is formed in registers.
//
// The reference loops over points in Python per view and holds an (N, V, 384) float64 block to average it away; nothing of that
// size exists here.  Rules and kernels: DESIGN.md section 12.
#include <cmath>
#include <cstring>

#include "ai_cells.inc"
#include "ai_xform.h"  // ai_xf: the fixed-order transform (step 1)

namespace {

#define AI_CAM_MAX_VIEWS 64

// one bit per view in every cloud point that a view's visible set names; an index outside [0, nc) raises *bad
__global__ __launch_bounds__(AI_BLOCK) void kc_view_bits(const int32_t* __restrict__ vis_index, int64_t total,
                                                         const int64_t* __restrict__ vis_off, int n_views, int64_t nc,
                                                         unsigned long long* __restrict__ bits, int32_t* __restrict__ bad) {
  const int64_t j = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (j >= total) return;
  int lo = 0, hi = n_views - 1;  // the view whose [vis_off[v], vis_off[v + 1]) holds j (empty views are skipped over)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (vis_off[mid] <= j) lo = mid;
    else hi = mid - 1;
  }
  const int64_t p = vis_index[j];
  if (p < 0 || p >= nc) {
    *bad = 1;
    return;
  }
  atomicOr(bits + p, 1ull << lo);
}

__global__ __launch_bounds__(AI_BLOCK) void kc_gather_bits(const unsigned long long* __restrict__ bits, const int32_t* __restrict__ order,
                                                           int64_t n, unsigned long long* __restrict__ sorted_bits) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p < n) sorted_bits[p] = bits[order[p]];
}

// OR of a 64-bit view mask over the 16 lanes of a query's group (every lane of the group must be active)
__device__ __forceinline__ unsigned long long group16_or(unsigned long long m) {
  unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    lo |= __shfl_xor(lo, o, 16);
    hi |= __shfl_xor(hi, o, 16);
  }
  return ((unsigned long long)hi << 32) | lo;
}

// 16 lanes per query (one thread per query left most of the chip idle at 33 k queries: 672 us): the group walks the 27 cells
// around the query in the pcd frame once, 16 points of a cell per step, lane t taking point t of the step.  A cloud point within
// the pcd-frame search radius (which bounds the camera-frame max_dist of every view, rounding included) is tested in the camera
// frame of each of its views not found yet, by the exact rule sqrt(sq_dist3(q_cam, p_cam)) < max_dist.  The group ORs its
// found views after every step (its trip counts are the group's, so all 16 lanes are there), so that no view is tested again
// once one lane has found it: with per-lane masks the 200 k-query launch took twice as long as with one thread per query.
// seen[i] = the views found (an OR: order-free, so reproducible).
__global__ __launch_bounds__(AI_BLOCK) void kc_visible(const double* __restrict__ q, int64_t nq, PGrid g, double search2,
                                                       const double* __restrict__ X, const double* __restrict__ Y,
                                                       const double* __restrict__ Z, const unsigned long long* __restrict__ B,
                                                       const int32_t* __restrict__ cstart, const int32_t* __restrict__ cend,
                                                       const double* __restrict__ T, unsigned long long all_views, double max_dist,
                                                       unsigned long long* __restrict__ seen) {
  const int64_t gid = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const int64_t i = gid >> 4;
  const int t = (int)(gid & 15);
  // nq * 16 is a multiple of 16 and every block a multiple of 64, so a 16-lane group is either wholly in range or wholly out
  if (i >= nq) return;
  const double x = q[i * 3], y = q[i * 3 + 1], z = q[i * 3 + 2];
  int cx, cy, cz;
  pcell_of(g, x, y, z, cx, cy, cz);
  unsigned long long found = 0;
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
        for (int32_t base = s; base < e; base += 16) {  // the same trip count for the whole group
          const int32_t p = base + t;
          unsigned long long m = p < e ? B[p] & ~found : 0ull;
          if (m) {
            const double px = X[p], py = Y[p], pz = Z[p];
            if (sq_dist3(x, y, z, px, py, pz) <= search2) {
              while (m) {
                const int v = __ffsll((long long)m) - 1;
                m &= m - 1;
                double qx, qy, qz, ux, uy, uz;
                ai_xf(T + 16 * v, x, y, z, qx, qy, qz);
                ai_xf(T + 16 * v, px, py, pz, ux, uy, uz);
                if (sqrt(sq_dist3(qx, qy, qz, ux, uy, uz)) < max_dist) found |= 1ull << v;
              }
            }
          }
          found = group16_or(found);
          if (found == all_views) goto done;  // uniform in the group
        }
      }
    }
  }
done:
  if (t == 0) seen[i] = found;
}

struct CamParams {
  int32_t n_views, img_h, img_w, fh, fw, fdim;
  double K[9];
  double f0, f1;  // fh / img_h, fw / img_w (image_utils.py:259-260)
};

// One wave per query, lane v = view v.  Lane v projects the query for view v (if it is seen there), writes the pixel and the SAM
// label of the pair, and finds the feature cell under the pixel; then the wave walks the views in order, lanes striding over the
// feature row, and sums the rows with a non-zero element (np.any) in float64: the mean of dinov2_mean, one element at a time.
// K: feature columns per lane and pass; a row wider than 64 K is summed in several passes over the views.
template <int K>
__global__ __launch_bounds__(AI_BLOCK) void kc_project(const double* __restrict__ q, int64_t nq, const unsigned long long* __restrict__ seen,
                                                       const double* __restrict__ T, CamParams P, const float* __restrict__ feat,
                                                       const int32_t* __restrict__ sam_img, int32_t* __restrict__ pixel_out,
                                                       int32_t* __restrict__ sam_out, double* __restrict__ feat_mean,
                                                       int32_t* __restrict__ feat_views, int32_t* __restrict__ bad) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (AI_BLOCK / 64) + (threadIdx.x >> 6);
  if (i >= nq) return;  // wave-uniform
  const int V = P.n_views;
  bool keep = false;
  int32_t pu = -1, pv = -1;
  if (lane < V && ((seen[i] >> lane) & 1ull)) {
    double x, y, z;
    ai_xf(T + 16 * lane, q[i * 3], q[i * 3 + 1], q[i * 3 + 2], x, y, z);
    const double u1 = (P.K[0] * x + P.K[1] * y) + P.K[2] * z;
    const double v1 = (P.K[3] * x + P.K[4] * y) + P.K[5] * z;
    const double w1 = (P.K[6] * x + P.K[7] * y) + P.K[8] * z;
    const double u = rint(u1 / w1), v = rint(v1 / w1);  // np.round: half to even
    // point_to_pixels.py:26-29 in double; NaN fails every comparison
    keep = (u < (double)P.img_w) && (u >= 0.0) && (v < (double)P.img_h) && (v >= 0.0) && (w1 > 0.0);
    if (keep) {
      pu = (int32_t)u;
      pv = (int32_t)v;
    }
  }
  if (lane < V) {
    const int64_t o = i * V + lane;
    if (pixel_out) {
      pixel_out[o * 2] = pu;
      pixel_out[o * 2 + 1] = pv;
    }
    if (sam_out) {
      const int32_t label = keep ? sam_img[((int64_t)lane * P.img_h + pv) * P.img_w + pu] : 0;
      sam_out[o] = label != 0 ? label : -1;  // image_utils.py:131-133, :339-340
    }
  }
  if (!feat) return;
  int64_t off = -1;
  if (keep) {
    const int64_t c0 = (int64_t)(P.f0 * (double)pv), c1 = (int64_t)(P.f1 * (double)pu);  // int(): toward zero, both >= 0
    if (c0 < 0 || c0 >= P.fh || c1 < 0 || c1 >= P.fw) {
      *bad = 2;  // the reference indexes past the map (IndexError)
      keep = false;
    } else {
      off = (((int64_t)lane * P.fh + c0) * P.fw + c1) * P.fdim;
    }
  }
  const unsigned long long kept = __ballot(keep);
  const int fdim = P.fdim;
  const bool one_pass = fdim <= 64 * K;
  for (int c0 = 0; c0 < fdim; c0 += 64 * K) {
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = -0.0;  // -0.0 + x == x for every x: the sum starts at the first row, as np.add.reduce
    int cnt = 0;
    unsigned long long m = kept;
    while (m) {
      const int v = __ffsll((long long)m) - 1;
      m &= m - 1;
      const float* row = feat + __shfl(off, v, 64);
      float f[K];
      bool nz = false;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int c = c0 + lane + 64 * k;
        f[k] = c < fdim ? row[c] : 0.0f;
        nz |= f[k] != 0.0f;  // -0.0 is zero, NaN is not
      }
      if (!one_pass)
        for (int c = lane; c < fdim; c += 64) nz |= row[c] != 0.0f;
      if (__any(nz)) {
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += (double)f[k];
        ++cnt;
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int c = c0 + lane + 64 * k;
      if (c < fdim) feat_mean[i * fdim + c] = cnt ? acc[k] / (double)cnt : 0.0;
    }
    if (c0 == 0 && lane == 0) feat_views[i] = cnt;
  }
}

// A lower bound of the smallest singular value of the linear part R of T: the larger of sqrt(1 - ||R^T R - I||_F) (tight for a
// rotation) and 1 / ||R^-1||_F.  0 when R is singular.
double sigma_min_bound(const double* T) {
  double R[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[r][c] = T[r * 4 + c];
  double e2 = 0.0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double s = 0.0;
      for (int r = 0; r < 3; ++r) s += R[r][a] * R[r][b];
      const double d = s - (a == b ? 1.0 : 0.0);
      e2 += d * d;
    }
  const double e = std::sqrt(e2);
  double s1 = e < 1.0 ? std::sqrt(1.0 - e) : 0.0;
  const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                     R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
  double s2 = 0.0;
  if (det != 0.0 && std::isfinite(det)) {
    double f2 = 0.0;  // ||adj(R)||_F^2; ||R^-1||_F = ||adj(R)||_F / |det|
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
        const double m = R[r1][c1] * R[r2][c2] - R[r1][c2] * R[r2][c1];
        f2 += m * m;
      }
    if (f2 > 0.0) s2 = std::fabs(det) / std::sqrt(f2);
  }
  return std::max(s1, s2);
}

}  // namespace

extern "C" int ai_camera_project(ai_ctx* ctx, const double* query_xyz, int64_t nq, const double* cloud_xyz, int64_t nc,
                                 const int32_t* vis_index, const int64_t* vis_off, int32_t n_views, const double* T_pcd2cam,
                                 const double* K, int32_t img_h, int32_t img_w, double max_dist, const float* feat, int32_t fh,
                                 int32_t fw, int32_t fdim, const int32_t* sam_img, int mem_kind, int32_t* pixel_out, int32_t* sam_out,
                                 double* feat_mean, int32_t* feat_views) {
  const char* who = "ai_camera_project";
  if (!ctx || nq < 0 || nc < 0 || n_views < 0 || n_views > AI_CAM_MAX_VIEWS || (nq > 0 && !query_xyz) || (nc > 0 && !cloud_xyz) ||
      !vis_off || (n_views > 0 && (!T_pcd2cam || !K)) || img_h <= 0 || img_w <= 0 || !(max_dist > 0.0) || !std::isfinite(max_dist) ||
      nq >= ((int64_t)1 << 30) || nc >= ((int64_t)1 << 30) || (!sam_img) != (!sam_out) || (!feat) != (!feat_mean) ||
      (!feat) != (!feat_views) || (feat && (fh < 0 || fw < 0 || fdim <= 0))) {
    ai_set_error("%s: bad argument (null pointer, n_views outside 0..64, image size <= 0, max_dist <= 0, sam_img / sam_out or "
                 "feat / feat_mean / feat_views given without the other)", who);
    return AI_ERR_BAD_ARG;
  }
  if (vis_off[0] != 0) {
    ai_set_error("%s: vis_off[0] must be 0", who);
    return AI_ERR_BAD_ARG;
  }
  for (int v = 0; v < n_views; ++v)
    if (vis_off[v + 1] < vis_off[v]) {
      ai_set_error("%s: vis_off must be non-decreasing", who);
      return AI_ERR_BAD_ARG;
    }
  const int64_t total = vis_off[n_views];
  if (total > 0 && !vis_index) {
    ai_set_error("%s: vis_index is NULL", who);
    return AI_ERR_BAD_ARG;
  }
  // the pcd-frame search radius: camera-frame distance >= sigma_min(R) x pcd-frame distance for an affine T
  double radius = 0.0;
  for (int v = 0; v < n_views; ++v) {
    const double* T = T_pcd2cam + 16 * v;
    for (int k = 0; k < 16; ++k)
      if (!std::isfinite(T[k])) {
        ai_set_error("%s: T_pcd2cam of view %d is not finite", who, v);
        return AI_ERR_BAD_ARG;
      }
    if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0) {
      ai_set_error("%s: the last row of T_pcd2cam of view %d must be (0, 0, 0, 1)", who, v);
      return AI_ERR_BAD_ARG;
    }
    const double s = sigma_min_bound(T);
    if (!(s > 1e-6)) {
      ai_set_error("%s: T_pcd2cam of view %d is (nearly) singular", who, v);
      return AI_ERR_BAD_ARG;
    }
    radius = std::max(radius, max_dist / s);
  }
  // slack for the rounding of both transforms and of the pcd-frame distance: far below 1e-6 relative for coordinates < 1e8
  radius = radius * (1.0 + 1e-6) + 1e-9;
  if (nq == 0) return AI_OK;
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;

  const int64_t n_feat = feat ? (int64_t)n_views * fh * fw * fdim : 0;
  const int64_t n_sam = sam_img ? (int64_t)n_views * img_h * img_w : 0;
  DevBuf<double> own_q, own_c, d_T, d_mean;
  DevBuf<int32_t> own_vi, own_sam, d_pix, d_samo, d_views, d_bad;
  DevBuf<float> own_f;
  DevBuf<int64_t> d_off;
  DevBuf<unsigned long long> d_bits, d_sbits, d_seen;
  const double *dq, *dc = nullptr;
  const int32_t *dvi = nullptr, *dsam = nullptr;
  const float* df = nullptr;
  AI_TRY(to_device(query_xyz, (size_t)nq * 3, mem_kind, own_q, &dq, st));
  if (feat && n_feat > 0) AI_TRY(to_device(feat, (size_t)n_feat, mem_kind, own_f, &df, st));
  if (feat && n_feat == 0) df = feat;  // never read: every cell index is out of range of an empty map
  if (sam_img && n_sam > 0) AI_TRY(to_device(sam_img, (size_t)n_sam, mem_kind, own_sam, &dsam, st));
  AI_TRY(d_T.alloc((size_t)std::max(n_views, 1) * 16));
  if (n_views > 0) AI_HIP(hipMemcpyAsync(d_T.p, T_pcd2cam, (size_t)n_views * 16 * sizeof(double), hipMemcpyHostToDevice, st));
  AI_TRY(d_bad.alloc(1));
  AI_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(int32_t), st));
  AI_TRY(d_seen.alloc((size_t)nq));

  const unsigned long long all_views = n_views == 64 ? ~0ull : ((1ull << n_views) - 1);
  if (nc > 0 && total > 0 && n_views > 0) {
    AI_TRY(to_device(cloud_xyz, (size_t)nc * 3, mem_kind, own_c, &dc, st));
    AI_TRY(to_device(vis_index, (size_t)total, mem_kind, own_vi, &dvi, st));
    AI_TRY(d_off.alloc((size_t)n_views + 1));
    AI_HIP(hipMemcpyAsync(d_off.p, vis_off, ((size_t)n_views + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    AI_TRY(d_bits.alloc((size_t)nc));
    AI_HIP(hipMemsetAsync(d_bits.p, 0, (size_t)nc * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(kc_view_bits, dim3(grid_for(total)), dim3(AI_BLOCK), 0, st, dvi, total,
                       (const int64_t*)d_off.p, (int)n_views, nc, d_bits.p, d_bad.p);
    AI_KERNEL_CHECK();
    Cells C;
    AI_TRY(build_cells(ctx, dc, nc, radius, C, who));
    AI_TRY(d_sbits.alloc((size_t)nc));
    const unsigned gc = grid_for(nc);
    hipLaunchKernelGGL(kc_gather_bits, dim3(gc), dim3(AI_BLOCK), 0, st, (const unsigned long long*)d_bits.p, (const int32_t*)C.order.p, nc,
                       d_sbits.p);
    AI_KERNEL_CHECK();
    const unsigned gq = grid_for(nq * 16);
    hipLaunchKernelGGL(kc_visible, dim3(gq), dim3(AI_BLOCK), 0, st, dq, nq, C.g, radius * radius, (const double*)C.X.p,
                       (const double*)C.Y.p, (const double*)C.Z.p, (const unsigned long long*)d_sbits.p, (const int32_t*)C.cstart.p,
                       (const int32_t*)C.cend.p, (const double*)d_T.p, all_views, max_dist, d_seen.p);
    AI_KERNEL_CHECK();
    AI_HIP(hipStreamSynchronize(st));  // C's buffers go out of scope
  } else {
    AI_HIP(hipMemsetAsync(d_seen.p, 0, (size_t)nq * sizeof(unsigned long long), st));
  }

  CamParams P;
  P.n_views = n_views;
  P.img_h = img_h;
  P.img_w = img_w;
  P.fh = feat ? fh : 0;
  P.fw = feat ? fw : 0;
  P.fdim = feat ? fdim : 0;
  for (int k = 0; k < 9; ++k) P.K[k] = n_views > 0 ? K[k] : 0.0;
  P.f0 = (double)P.fh / (double)img_h;
  P.f1 = (double)P.fw / (double)img_w;
  int32_t* o_pix = pixel_out;
  int32_t* o_sam = sam_out;
  double* o_mean = feat_mean;
  int32_t* o_views = feat_views;
  const int64_t n_pairs = nq * n_views;
  if (mem_kind != AI_MEM_DEVICE) {
    if (pixel_out) {
      AI_TRY(d_pix.alloc((size_t)n_pairs * 2));
      o_pix = d_pix.p;
    }
    if (sam_out) {
      AI_TRY(d_samo.alloc((size_t)n_pairs));
      o_sam = d_samo.p;
    }
    if (feat) {
      AI_TRY(d_mean.alloc((size_t)nq * fdim));
      AI_TRY(d_views.alloc((size_t)nq));
      o_mean = d_mean.p;
      o_views = d_views.p;
    }
  }
  const unsigned gw = (unsigned)((nq + AI_BLOCK / 64 - 1) / (AI_BLOCK / 64));
  if (P.fdim <= 128)
    hipLaunchKernelGGL(kc_project<2>, dim3(gw), dim3(AI_BLOCK), 0, st, dq, nq, (const unsigned long long*)d_seen.p, (const double*)d_T.p, P,
                       df, dsam, o_pix, o_sam, o_mean, o_views, d_bad.p);
  else
    hipLaunchKernelGGL(kc_project<6>, dim3(gw), dim3(AI_BLOCK), 0, st, dq, nq, (const unsigned long long*)d_seen.p, (const double*)d_T.p, P,
                       df, dsam, o_pix, o_sam, o_mean, o_views, d_bad.p);
  AI_KERNEL_CHECK();
  int32_t bad = 0;
  AI_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (mem_kind != AI_MEM_DEVICE) {
    if (pixel_out && n_pairs > 0)
      AI_HIP(hipMemcpyAsync(pixel_out, o_pix, (size_t)n_pairs * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (sam_out && n_pairs > 0) AI_HIP(hipMemcpyAsync(sam_out, o_sam, (size_t)n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (feat) {
      AI_HIP(hipMemcpyAsync(feat_mean, o_mean, (size_t)nq * fdim * sizeof(double), hipMemcpyDeviceToHost, st));
      AI_HIP(hipMemcpyAsync(feat_views, o_views, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
  }
  AI_HIP(hipStreamSynchronize(st));
  if (bad == 1) {
    ai_set_error("%s: vis_index holds an index outside [0, nc)", who);
    return AI_ERR_BAD_ARG;
  }
  if (bad == 2) {
    ai_set_error("%s: feature cell out of range: a projected pixel maps outside the %d x %d feature map", who, fh, fw);
    return AI_ERR_BAD_ARG;
  }
  return AI_OK;
}
