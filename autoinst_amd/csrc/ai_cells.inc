// The cell lists of the point-cloud searches (ai_points.hip, ai_camera.hip, ai_scanpool.hip, ai_finish.hip, ai_prep.hip): the squared
// distance of every radius / nearest-point test; the dense list (PGrid: [start, end) cell ranges over points sorted by cell) of the
// radius and 1-NN searches; the row list (KGrid: points sorted by (z, y) row, x by binary search) of the kNN searches; the stop rule
// the ring searches share, with its two helpers.  A header like any other (included at file scope, its own anonymous namespace) under
// the file name the cell list always had.  Everything has internal linkage.
#pragma once
#include <climits>
#include <cmath>

#include "ai_entry.h"
#include "ai_runs.h"

namespace {

// The squared distance of both searches, in the order of nanoflann's L2_Adaptor (what open3d's KDTreeFlann runs) and of
// cdist: (dx*dx + dy*dy) + dz*dz, every product and sum rounded on its own.  The default -ffp-contract=fast would fuse the
// two adds into v_fmac_f64 and move a point within an ulp of the radius, or a near-tie, to the other side
// (tests/test_gpu_edges.py).  No contraction in this function.
__device__ __forceinline__ double sq_dist3(double x, double y, double z, double px, double py, double pz) {
#pragma clang fp contract(off)
  const double dx = x - px, dy = y - py, dz = z - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

struct PGrid {
  double minx, miny, minz, inv_cell;
  int nx, ny, nz;
};

__device__ __forceinline__ void pcell_of(const PGrid& g, double x, double y, double z, int& cx, int& cy, int& cz) {
  cx = min(max((int)floor((x - g.minx) * g.inv_cell), 0), g.nx - 1);
  cy = min(max((int)floor((y - g.miny) * g.inv_cell), 0), g.ny - 1);
  cz = min(max((int)floor((z - g.minz) * g.inv_cell), 0), g.nz - 1);
}

__global__ __launch_bounds__(AI_BLOCK) void kp_bounds(const double* __restrict__ xyz, int64_t n, double* __restrict__ part) {
  __shared__ double sm[6][AI_BLOCK / 64];
  double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
  for (int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AI_BLOCK)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      // fmin / fmax drop a NaN: a coordinate that is not finite goes in as +inf, so that build_cells' extent check sees it
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

// linear cell id as the sort key (the grid is small enough for 32 bits), value = point index
__global__ __launch_bounds__(AI_BLOCK) void kp_keys(const double* __restrict__ xyz, int64_t n, PGrid g, uint32_t* __restrict__ key,
                                                    int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  int cx, cy, cz;
  pcell_of(g, xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], cx, cy, cz);
  key[i] = (uint32_t)((cz * g.ny + cy) * g.nx + cx);
  idx[i] = (int32_t)i;
}

__global__ __launch_bounds__(AI_BLOCK) void kp_gather(const double* __restrict__ xyz, const int32_t* __restrict__ order,
                                                      const uint32_t* __restrict__ skey, int64_t n, double* __restrict__ X,
                                                      double* __restrict__ Y, double* __restrict__ Z, int32_t* __restrict__ cstart,
                                                      int32_t* __restrict__ cend) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p >= n) return;
  const int64_t o = order[p];
  X[p] = xyz[o * 3];
  Y[p] = xyz[o * 3 + 1];
  Z[p] = xyz[o * 3 + 2];
  const uint32_t c = skey[p];
  if (p == 0 || skey[p - 1] != c) cstart[c] = (int32_t)p;
  if (p == n - 1 || skey[p + 1] != c) cend[c] = (int32_t)(p + 1);
}

struct Cells {
  PGrid g;
  double cell;
  DevBuf<int32_t> order, cstart, cend;
  DevBuf<double> X, Y, Z;
};

// A template only so that the 32-bit radix sort is instantiated in the sources that build a dense list, not in every source that
// includes this header for its helpers.
template <typename Key = uint32_t>
int build_cells(ai_ctx* ctx, const double* d_xyz, int64_t n, double cell, Cells& C, const char* who) {
  hipStream_t st = ctx->stream;
  const int nb = 256;
  DevBuf<double> part;
  AI_TRY(part.alloc((size_t)nb * 6));
  hipLaunchKernelGGL(kp_bounds, dim3(nb), dim3(AI_BLOCK), 0, st, d_xyz, n, part.p);
  AI_KERNEL_CHECK();
  std::vector<double> hp((size_t)nb * 6);
  AI_HIP(hipMemcpyAsync(hp.data(), part.p, hp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
  for (int b = 0; b < nb; ++b)
    for (int a = 0; a < 3; ++a) {
      mn[a] = std::min(mn[a], hp[b * 6 + a]);
      mx[a] = std::max(mx[a], hp[b * 6 + 3 + a]);
    }
  for (int a = 0; a < 3; ++a)
    if (!(mn[a] <= mx[a]) || !(mx[a] - mn[a] < 1e15)) {
      ai_set_error("%s: coordinates are not finite", who);
      return AI_ERR_BAD_ARG;
    }
  // grow the cell until the dense table fits (a coarser grid only means more candidates per query)
  for (;;) {
    const double ex = (mx[0] - mn[0]) / cell, ey = (mx[1] - mn[1]) / cell, ez = (mx[2] - mn[2]) / cell;
    if ((floor(ex) + 1) * (floor(ey) + 1) * (floor(ez) + 1) <= (double)((int64_t)1 << 27)) break;
    cell *= 1.5;
  }
  C.cell = cell;
  C.g.minx = mn[0];
  C.g.miny = mn[1];
  C.g.minz = mn[2];
  C.g.inv_cell = 1.0 / cell;
  C.g.nx = (int)floor((mx[0] - mn[0]) / cell) + 1;
  C.g.ny = (int)floor((mx[1] - mn[1]) / cell) + 1;
  C.g.nz = (int)floor((mx[2] - mn[2]) / cell) + 1;
  const int64_t ncell = (int64_t)C.g.nx * C.g.ny * C.g.nz;
  const unsigned gb = grid_for(n);
  DevBuf<Key> key, skey;
  DevBuf<int32_t> idx;
  DevBuf<uint8_t> tmp;
  AI_TRY(key.alloc(n));
  AI_TRY(skey.alloc(n));
  AI_TRY(idx.alloc(n));
  AI_TRY(C.order.alloc(n));
  AI_TRY(C.cstart.alloc(ncell));
  AI_TRY(C.cend.alloc(ncell));
  AI_TRY(C.X.alloc(n));
  AI_TRY(C.Y.alloc(n));
  AI_TRY(C.Z.alloc(n));
  hipLaunchKernelGGL(kp_keys, dim3(gb), dim3(AI_BLOCK), 0, st, d_xyz, n, C.g, key.p, idx.p);
  AI_KERNEL_CHECK();
  AI_TRY(sort_pairs(st, key.p, skey.p, idx.p, C.order.p, n, std::max(1, bits_for(ncell)), tmp));
  AI_HIP(hipMemsetAsync(C.cstart.p, 0xff, (size_t)ncell * sizeof(int32_t), st));
  AI_HIP(hipMemsetAsync(C.cend.p, 0, (size_t)ncell * sizeof(int32_t), st));
  hipLaunchKernelGGL(kp_gather, dim3(gb), dim3(AI_BLOCK), 0, st, d_xyz, (const int32_t*)C.order.p, (const uint32_t*)skey.p, n, C.X.p, C.Y.p,
                     C.Z.p, C.cstart.p, C.cend.p);
  AI_KERNEL_CHECK();
  AI_HIP(hipStreamSynchronize(st));  // key / skey / idx / tmp go out of scope
  return AI_OK;
}

// ----------------------------------------------------------------------------- the stop rule of the ring searches
// A ring search visits the cells around a query's own cell c by rings (ring r: the shell of Chebyshev cell distance r) and stops
// when nothing unvisited can matter.  A source outside rings 0..r has, on some axis, a stored cell index k >= c + r + 1 (or
// <= c - r - 1), so it lies beyond that face F = min + k * cell of the box of those rings -- up to the rounding of pcell_of /
// kcell_of.  With u = 2^-53: the index is floor(fl(fl(p - min) * inv_cell)) and inv_cell = fl(1 / cell), three roundings, so
// fl(..) >= k only gives p - min >= k * cell * (1 - 4u) (and < k * cell * (1 + 4u) on the low side; the clamp to n - 1 only lowers
// a stored index): the source may lie 4u * k * cell inside the face.  face_gap computes |F - x| with three more roundings, of
// k * cell, of F and of the difference: at most u * (k * cell + |F| + |F| + |x|) off.  With mag >= |min| + (n + 1) * cell + |x| on
// every axis (axis_mag), which bounds k * cell, |F| and |x|, all of it stays below 8u * mag; `slack` is 16u * mag = 8 ulps of mag,
// as in kn_nearest (ai_prep.hip).  So every unvisited source is more than lb = (nearest face gap) - slack away, in exact arithmetic.
// sq_dist3 rounds five times, hence returns at least d^2 * (1 - 5u) for a source at distance d > lb; sqrt(best) * (1 + 8u) <= lb
// gives best <= lb^2 * (1 - 11u) after the rounding of the sqrt and of the product: strictly below the square of every unvisited
// source, so none is nearer or tied -- for the best of the 1-NN search and for the k-th best of the kNN search alike, whatever the
// grid is.  The face gap is at least r * cell, the bound the rule had before the rounding was counted (sqrt(best) <= r * cell
// missed a source that fl(p - min) had rounded up onto a cell border when sqrt(best) was within a few ulps of r * cell:
// tests/points_cases.py and tests/prep_cases.py find such clouds): an extra ring is searched only when sqrt(best) is within the
// slack of it.  With no cell left on any side lb is +inf and the loop ends.

// The distances from x to the two faces, on one axis, of the box of rings 0..r around cell c: the planes min + (c - r) * cell and
// min + (c + r + 1) * cell.  A side on which the grid has no cell left counts as infinitely far.  Every step is rounded on its own
// (no contraction), so that the slack of the stop rule can be counted and tests/points_cases.py can restate it.
__device__ __forceinline__ double face_gap(double x, double mn, double cell, int c, int r, int n) {
#pragma clang fp contract(off)
  const double lo = (c - r - 1 >= 0) ? x - (mn + (double)(c - r) * cell) : INFINITY;
  const double hi = (c + r + 1 <= n - 1) ? (mn + (double)(c + r + 1) * cell) - x : INFINITY;
  return fmin(lo, hi);
}

// |min| + (n + 1) * cell + |x|: above every magnitude that enters an index or a face on this axis
__device__ __forceinline__ double axis_mag(double x, double mn, double cell, int n) {
#pragma clang fp contract(off)
  return (fabs(mn) + (double)(n + 1) * cell) + fabs(x);
}

// ----------------------------------------------------------------------------- the row list
struct KGrid {
  double minx, miny, minz, inv_cell, cell;
  int nx, ny, nz;
};

// pcell_of's three roundings (the subtraction, the product, inv_cell = fl(1 / cell)): the stop rule counts them
__device__ __forceinline__ void kcell_of(const KGrid& g, double x, double y, double z, int& cx, int& cy, int& cz) {
  cx = min(max((int)floor((x - g.minx) * g.inv_cell), 0), g.nx - 1);
  cy = min(max((int)floor((y - g.miny) * g.inv_cell), 0), g.ny - 1);
  cz = min(max((int)floor((z - g.minz) * g.inv_cell), 0), g.nz - 1);
}

// skey = the sorted keys, row (z, y) in the high 32 bits and the x cell in the low 32: the sorted coordinates, the x cell of every
// sorted point and the [start, end) run of every occupied row
__global__ __launch_bounds__(AI_BLOCK) void kq_gather(const double* __restrict__ xyz, const int32_t* __restrict__ order,
                                                      const uint64_t* __restrict__ skey, int64_t n, double* __restrict__ X,
                                                      double* __restrict__ Y, double* __restrict__ Z, int32_t* __restrict__ scx,
                                                      int32_t* __restrict__ rstart, int32_t* __restrict__ rend) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p >= n) return;
  const int64_t o = order[p];
  X[p] = xyz[o * 3];
  Y[p] = xyz[o * 3 + 1];
  Z[p] = xyz[o * 3 + 2];
  const uint64_t k = skey[p];
  scx[p] = (int32_t)(uint32_t)k;
  const uint32_t row = (uint32_t)(k >> 32);
  if (p == 0 || (uint32_t)(skey[p - 1] >> 32) != row) rstart[row] = (int32_t)p;
  if (p == n - 1 || (uint32_t)(skey[p + 1] >> 32) != row) rend[row] = (int32_t)(p + 1);
}

// keep the K smallest values seen in best[0..K-1] (ascending); compile-time indices only, so the list stays in registers
template <int K>
__device__ __forceinline__ void knn_insert(double (&best)[K], double d2) {
  if (d2 < best[K - 1]) {
#pragma unroll
    for (int j = K - 1; j > 0; --j) best[j] = d2 < best[j - 1] ? best[j - 1] : fmin(d2, best[j]);
    best[0] = fmin(best[0], d2);
  }
}

}  // namespace
