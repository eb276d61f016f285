// ai_dbscan: DBSCAN of many clouds in one call -- sklearn.cluster.DBSCAN as AggregationClustering.clusters_hdbscan / clusterize_pcd
// run it (pipeline/utils/aggregate.py:253-327), label for label.  The rules (D1-D6) are in include/autoinst_hip.h and DESIGN.md
// section 23.  No neighbour list is stored: three searches over the cell ring of every point, in cell-sorted order.
//
//   (cells)     build_cells over all points of the call, cell = eps * (1 + 1e-6) or coarser: see DB_CELL_SLACK;
//   kd_cloud    the cloud of every sorted point (binary search in the offsets; only with more than one cloud);
//   kd_count    search 1: neighbours counted up to min_samples (early exit) -> core flags, saturated counts; parent[i] = i;
//   kd_union    search 2: every core point is united with its core neighbours of smaller index (lock-free, see db_unite);
//   kd_flatten  (a launch of its own: the kernel boundary is the fence) root of every core point; flag = "is a root";
//   (scan)      exclusive scan of the root flags over the point indices: the rank of a root among all roots of the call;
//   kd_labels   search 3, for the points that are not core: the smallest root among the core neighbours; then for every point
//               label = rank[root] - rank[first point of the cloud], and the cluster sizes (integer atomics);
//   kd_nclusters  rank differences at the cloud borders.
//
// A root is the smallest core index of its component (db_unite only ever hooks the larger root under the smaller), the points of
// a cloud are contiguous in the index, so the rank of a root minus the rank at the cloud's start IS the cluster number of D4 and
// the smallest root IS the smallest cluster number of D5: nothing is sorted or renumbered.
#include <climits>
#include <cmath>

#include "ai_cells.inc"

namespace {

// The ring of +-1 cells holds every neighbour iff two points at most eps apart on an axis never get cell indices 2 apart.  Their
// exact positions in cell units differ by at most eps / cell = 1 / (1 + s); pcell_of rounds three times (the subtraction, the
// product, inv_cell), so a computed position t is off by at most 3 * 2^-53 * t, t < 2^27 (build_cells' table limit): together
// below 9e-8.  s = 1e-6 leaves the computed difference below 1, hence the floors at most 1 apart, on any grid build_cells makes.
#define DB_CELL_SLACK 1e-6

struct DBView {
  PGrid g;
  const double *X, *Y, *Z;
  const int32_t *cstart, *cend, *cloud;  // cloud: per sorted point, null with one cloud
  double e2;
};

// f(q) for every neighbour q (D1) of sorted point p, p itself included, until f returns true.  The three cells of a (z, y) row
// have consecutive keys, so their points are one contiguous range of the sorted order: 9 ranges, not 27.
template <bool MULTI, typename F>
__device__ __forceinline__ void db_neighbours(const DBView& v, int32_t p, F&& f) {
  const double x = v.X[p], y = v.Y[p], z = v.Z[p];
  const int32_t c = MULTI ? v.cloud[p] : 0;
  int cx, cy, cz;
  pcell_of(v.g, x, y, z, cx, cy, cz);  // the cell kp_keys gave it: same operands, same operations
  const int x0 = max(cx - 1, 0), x1 = min(cx + 1, v.g.nx - 1);
  for (int zz = max(cz - 1, 0); zz <= min(cz + 1, v.g.nz - 1); ++zz)
    for (int yy = max(cy - 1, 0); yy <= min(cy + 1, v.g.ny - 1); ++yy) {
      const int32_t row = (zz * v.g.ny + yy) * v.g.nx;
      int32_t s = -1, e = 0;
      for (int xx = x0; xx <= x1; ++xx) {
        const int32_t cs = v.cstart[row + xx];
        if (cs < 0) continue;
        if (s < 0) s = cs;
        e = v.cend[row + xx];
      }
      if (s < 0) continue;  // the row's three cells are empty
      for (int32_t q = s; q < e; ++q) {
        if (MULTI && v.cloud[q] != c) continue;
        if (sq_dist3(x, y, z, v.X[q], v.Y[q], v.Z[q]) <= v.e2 && f(q)) return;
      }
    }
}

__global__ __launch_bounds__(AI_BLOCK) void kd_cloud(const int32_t* __restrict__ order, int64_t n, const int64_t* __restrict__ off,
                                                     int32_t n_clouds, int32_t* __restrict__ cloud) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p < n) cloud[p] = segment_of(off, n_clouds, order[p]);
}

template <bool MULTI>
__global__ __launch_bounds__(AI_BLOCK) void kd_count(DBView v, const int32_t* __restrict__ order, int64_t n, int32_t min_samples,
                                                     uint8_t* __restrict__ core, int32_t* __restrict__ parent,
                                                     int32_t* __restrict__ count_out) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p >= n) return;
  int32_t cnt = 0;
  db_neighbours<MULTI>(v, (int32_t)p, [&](int32_t) { return ++cnt >= min_samples; });
  const int32_t o = order[p];
  core[p] = cnt >= min_samples ? 1 : 0;
  parent[o] = o;
  if (count_out) count_out[o] = cnt;
}

// The union.  parent[x] <= x at all times, and parent[x] only ever decreases: a root (parent[x] == x) is hooked under a smaller
// root by the compare-and-swap of db_unite, a non-root is moved to a farther ancestor by the atomic minimum of db_find.  So any
// value ever read from parent[x], however stale (another XCD's L2, this CU's L1), is an ancestor of x or x itself, and walking
// it is correct; the agent-scope loads only shorten the walk.  Every loop follows a strictly decreasing index, no thread waits
// for another.
__device__ __forceinline__ int32_t db_find(int32_t* parent, int32_t x) {
  for (;;) {
    const int32_t p = ai_ld_agent(parent + x);
    if (p >= x) return x;
    const int32_t gp = ai_ld_agent(parent + p);
    if (gp >= p) return p;
    atomicMin(parent + x, gp);  // path halving: gp is an ancestor of x
    x = gp;
  }
}

// the (then) common root of a and b, b < a's point: a + b decreases with every pass that does not return
__device__ __forceinline__ int32_t db_unite(int32_t* parent, int32_t a, int32_t b) {
  for (;;) {
    a = db_find(parent, a);
    b = db_find(parent, b);
    if (a == b) return a;
    const int32_t hi = max(a, b), lo = min(a, b);
    const int32_t old = atomicCAS(parent + hi, hi, lo);  // agent scope
    if (old == hi) return lo;
    a = old;  // hi was hooked meanwhile: old < hi is its parent
    b = lo;
  }
}

template <bool MULTI>
__global__ __launch_bounds__(AI_BLOCK) void kd_union(DBView v, const int32_t* __restrict__ order, int64_t n,
                                                     const uint8_t* __restrict__ core, int32_t* parent) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p >= n || !core[p]) return;
  const int32_t o = order[p];
  int32_t r = o;  // an ancestor of o
  db_neighbours<MULTI>(v, (int32_t)p, [&](int32_t q) {
    if (core[q]) {
      const int32_t oq = order[q];
      if (oq < o) r = db_unite(parent, r, oq);
    }
    return false;
  });
}

// after the union's launch has ended: plain loads see its last values
__global__ __launch_bounds__(AI_BLOCK) void kd_flatten(const int32_t* __restrict__ order, int64_t n, const uint8_t* __restrict__ core,
                                                       const int32_t* __restrict__ parent, int32_t* __restrict__ root,
                                                       int32_t* __restrict__ flag) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p >= n) return;
  const int32_t o = order[p];
  int32_t r = -1;
  if (core[p]) {
    r = o;
    for (int32_t up = parent[r]; up < r; up = parent[r]) r = up;
  }
  root[p] = r;
  flag[o] = r == o ? 1 : 0;
}

template <bool MULTI>
__global__ __launch_bounds__(AI_BLOCK) void kd_labels(DBView v, const int32_t* __restrict__ order, int64_t n,
                                                      const int64_t* __restrict__ off, const int32_t* __restrict__ root, const int32_t* __restrict__ rank,
                                                      int32_t* __restrict__ labels, int32_t* __restrict__ sizes) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p >= n) return;
  int32_t r = root[p];
  if (r < 0) {  // not core: D5
    int32_t best = INT_MAX;
    db_neighbours<MULTI>(v, (int32_t)p, [&](int32_t q) {
      const int32_t rq = root[q];  // -1: q is not core
      if (rq >= 0) best = min(best, rq);
      return false;
    });
    r = best == INT_MAX ? -1 : best;
  }
  const int64_t first = MULTI ? off[v.cloud[p]] : 0;
  const int32_t lab = r < 0 ? -1 : rank[r] - rank[first];
  labels[order[p]] = lab;
  if (sizes && lab >= 0) atomicAdd(sizes + first + lab, 1);
}

__global__ __launch_bounds__(AI_BLOCK) void kd_nclusters(const int64_t* __restrict__ off, int32_t n_clouds,
                                                         const int32_t* __restrict__ rank, int32_t* __restrict__ n_clusters) {
  const int32_t c = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (c < n_clouds) n_clusters[c] = rank[off[c + 1]] - rank[off[c]];
}

}  // namespace

extern "C" int ai_dbscan(ai_ctx* ctx, const double* xyz, const int64_t* off, int32_t n_clouds, double eps, int32_t min_samples,
                         int mem_kind, int32_t* labels, int32_t* n_clusters, int32_t* count_out, int32_t* sizes_out) {
  const auto bad = [](const char* what) { return bad_arg("ai_dbscan", what); };
  if (!ctx || !off || n_clouds < 0) return bad("null pointer or negative count");
  if (!(eps > 0.0) || !std::isfinite(eps)) return bad("eps must be positive and finite");
  if (min_samples < 1) return bad("min_samples must be at least 1");
  if (off[0] != 0) return bad("off must start at 0");
  for (int32_t c = 0; c < n_clouds; ++c)
    if (off[c + 1] < off[c]) return bad("off is not monotone");
  const int64_t n = off[n_clouds];
  if (n >= ((int64_t)1 << 30)) return bad("the call must hold fewer than 2^30 points");
  if ((n_clouds > 0 && !n_clusters) || (n > 0 && (!xyz || !labels))) return bad("null pointer");
  if (n == 0) {
    for (int32_t c = 0; c < n_clouds; ++c) n_clusters[c] = 0;
    return AI_OK;
  }
  const double e2 = eps * eps;  // rounded once (D1)
  if (!(e2 > 0.0) || !std::isfinite(e2)) return bad("eps * eps must be positive and finite");

  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<double> own_xyz;
  DevBuf<int64_t> d_off;
  DevBuf<int32_t> cloud, parent, root, rank, scan_tmp, own_lab, own_cnt, own_siz, d_ncl;
  DevBuf<uint8_t> core;
  const double* dx = nullptr;
  AI_TRY(to_device(xyz, (size_t)n * 3, mem_kind, own_xyz, &dx, st));
  AI_TRY(d_off.alloc((size_t)n_clouds + 1));
  AI_HIP(hipMemcpyAsync(d_off.p, off, ((size_t)n_clouds + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  Cells C;
  AI_TRY(build_cells(ctx, dx, n, eps * (1.0 + DB_CELL_SLACK), C, "ai_dbscan"));

  const bool multi = n_clouds > 1;
  const unsigned gb = grid_for(n);
  int32_t *d_lab = nullptr, *d_cnt = nullptr, *d_siz = nullptr;
  AI_TRY(dev_out(labels, (size_t)n, mem_kind, own_lab, &d_lab));
  if (count_out) AI_TRY(dev_out(count_out, (size_t)n, mem_kind, own_cnt, &d_cnt));
  if (sizes_out) AI_TRY(dev_out(sizes_out, (size_t)n, mem_kind, own_siz, &d_siz));
  AI_TRY(core.alloc(n));
  AI_TRY(parent.alloc(n));
  AI_TRY(root.alloc(n));
  AI_TRY(rank.alloc((size_t)n + 1));
  AI_TRY(d_ncl.alloc(n_clouds));
  if (multi) {
    AI_TRY(cloud.alloc(n));
    hipLaunchKernelGGL(kd_cloud, dim3(gb), dim3(AI_BLOCK), 0, st, (const int32_t*)C.order.p, n, (const int64_t*)d_off.p, n_clouds, cloud.p);
    AI_KERNEL_CHECK();
  }
  if (d_siz) AI_HIP(hipMemsetAsync(d_siz, 0, (size_t)n * sizeof(int32_t), st));
  const DBView v = {C.g, C.X.p, C.Y.p, C.Z.p, C.cstart.p, C.cend.p, multi ? cloud.p : nullptr, e2};
  const int32_t* order = C.order.p;

  if (multi)
    hipLaunchKernelGGL(kd_count<true>, dim3(gb), dim3(AI_BLOCK), 0, st, v, order, n, min_samples, core.p, parent.p, d_cnt);
  else
    hipLaunchKernelGGL(kd_count<false>, dim3(gb), dim3(AI_BLOCK), 0, st, v, order, n, min_samples, core.p, parent.p, d_cnt);
  AI_KERNEL_CHECK();
  if (multi)
    hipLaunchKernelGGL(kd_union<true>, dim3(gb), dim3(AI_BLOCK), 0, st, v, order, n, (const uint8_t*)core.p, parent.p);
  else
    hipLaunchKernelGGL(kd_union<false>, dim3(gb), dim3(AI_BLOCK), 0, st, v, order, n, (const uint8_t*)core.p, parent.p);
  AI_KERNEL_CHECK();
  hipLaunchKernelGGL(kd_flatten, dim3(gb), dim3(AI_BLOCK), 0, st, order, n, (const uint8_t*)core.p, (const int32_t*)parent.p, root.p, rank.p);
  AI_KERNEL_CHECK();
  AI_TRY(scan_flags(st, rank.p, n, scan_tmp));
  if (multi)
    hipLaunchKernelGGL(kd_labels<true>, dim3(gb), dim3(AI_BLOCK), 0, st, v, order, n, (const int64_t*)d_off.p,
                       (const int32_t*)root.p, (const int32_t*)rank.p, d_lab, d_siz);
  else
    hipLaunchKernelGGL(kd_labels<false>, dim3(gb), dim3(AI_BLOCK), 0, st, v, order, n, (const int64_t*)d_off.p,
                       (const int32_t*)root.p, (const int32_t*)rank.p, d_lab, d_siz);
  AI_KERNEL_CHECK();
  hipLaunchKernelGGL(kd_nclusters, dim3(grid_for(n_clouds)), dim3(AI_BLOCK), 0, st, (const int64_t*)d_off.p, n_clouds,
                     (const int32_t*)rank.p, d_ncl.p);
  AI_KERNEL_CHECK();
  AI_HIP(hipMemcpyAsync(n_clusters, d_ncl.p, (size_t)n_clouds * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (d_lab != labels) AI_TRY(to_caller(labels, (const int32_t*)d_lab, (size_t)n, mem_kind, st));
  if (d_cnt && d_cnt != count_out) AI_TRY(to_caller(count_out, (const int32_t*)d_cnt, (size_t)n, mem_kind, st));
  if (d_siz && d_siz != sizes_out) AI_TRY(to_caller(sizes_out, (const int32_t*)d_siz, (size_t)n, mem_kind, st));
  AI_HIP(hipStreamSynchronize(st));
  return AI_OK;
}
