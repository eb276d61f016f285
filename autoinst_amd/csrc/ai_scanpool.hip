// ai_scan_pool: the TARL scan features of every chunk of a map in one call -- tarl_features_per_patch
// (pipeline/utils/point_cloud/chunk_generation.py:221-256) for all chunks at once.  The rules (R1-R5) are in
// include/autoinst_hip.h and DESIGN.md section 14.
//
//   ks_flag    every source point: its scan (binary search in the scan offsets), the fixed-order transform (R1), and whether
//              it lies strictly inside some box whose window holds its scan (the chunk table sits in LDS, a tile at a time);
//   (scan)     exclusive scan of the flags: the survivors keep their order in scan_xyz;
//   ks_keys    the survivors' 64-bit cell keys ix << sy | iy << sz | iz and their source indices;
//   (sort)     stable rocPRIM radix sort by key: ascending (ix, iy, iz), then ascending position in scan_xyz (R4);
//   kl_heads / scan / kv_starts (ai_runs.h): the table of occupied cells (sorted distinct keys with their runs); no dense grid;
//   ks_gather  coordinates and scan positions in sort order, the distinct keys;
//   ks_pool    16 lanes per query: 9 binary searches (one (ix, iy) row of three iz cells is one key range), shared membership
//              tests (lane t tests candidate t), then the group walks the ballot in candidate order and every lane adds its
//              columns of the member row to float64 accumulators in registers.
//
// The cell index is floor(coord * (1 / cell)), cell = radius * (1 + 1e-9), origin 0: which cell a point is in depends on its
// coordinates alone.  The key stores index - bias per axis, bias = the smallest index a point strictly inside any box can have;
// a bias moves no point past another, so the order of the members of a mean is a function of the coordinates alone.
#include <climits>
#include <cmath>

#include "ai_cells.inc"
#include "ai_xform.h"  // ai_xf: the fixed-order transform (R1)

namespace {

#define SP_TILE 256           // chunk records per LDS tile of ks_flag
#define SP_MAX_INDEX 1073741824.0  // |cell index| < 2^30

struct SPChunk {   // one chunk: its box and its window of scan positions
  double lo[3], hi[3];
  int32_t w0, w1;
};

struct SPGrid {
  double inv_cell;
  int32_t bx, by, bz;  // bias: key index = floor(coord * inv_cell) - bias
  int32_t nx, ny, nz;  // indices per axis that the key has room for (powers of two)
  int32_t sy, sz;      // key = ix << sy | iy << sz | iz
};

__device__ __forceinline__ bool sp_in_box(const SPChunk& c, double x, double y, double z) {
  return x > c.lo[0] && y > c.lo[1] && z > c.lo[2] && x < c.hi[0] && y < c.hi[1] && z < c.hi[2];
}

// the transformed point of source index i and its scan position
__device__ __forceinline__ int32_t sp_source(const double* __restrict__ xyz, const int64_t* __restrict__ scan_off, int32_t n_scans,
                                             const double* __restrict__ T, int64_t i, double& x, double& y, double& z) {
  const int32_t s = segment_of(scan_off, n_scans, i);
  ai_xf(T + (int64_t)s * 16, xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], x, y, z);
  return s;
}

// flag[i] = 1 iff source point i is inside some box whose window holds its scan; *err |= 1 for a non-finite coordinate
__global__ __launch_bounds__(AI_BLOCK) void ks_flag(const double* __restrict__ xyz, int64_t n, const int64_t* __restrict__ scan_off,
                                                    int32_t n_scans, const double* __restrict__ T, const SPChunk* __restrict__ chunks,
                                                    int32_t n_chunks, int32_t* __restrict__ flag, int32_t* __restrict__ err) {
  __shared__ SPChunk sm[SP_TILE];
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const bool ok = i < n;
  double x = 0.0, y = 0.0, z = 0.0;
  int32_t s = -1;
  if (ok) {
    s = sp_source(xyz, scan_off, n_scans, T, i, x, y, z);
    if (!(fabs(x) < INFINITY && fabs(y) < INFINITY && fabs(z) < INFINITY)) atomicOr(err, 1);  // NaN fails the comparison too
  }
  bool keep = false;
  for (int32_t base = 0; base < n_chunks; base += SP_TILE) {
    const int32_t cnt = min(SP_TILE, n_chunks - base);
    __syncthreads();
    {  // the tile as 32-bit words, every word loaded once
      const int32_t* src = reinterpret_cast<const int32_t*>(chunks + base);
      int32_t* dst = reinterpret_cast<int32_t*>(sm);
      const int nw = cnt * (int)(sizeof(SPChunk) / 4);
      for (int w = threadIdx.x; w < nw; w += AI_BLOCK) dst[w] = src[w];
    }
    __syncthreads();
    for (int32_t b = 0; b < cnt; ++b) {
      if (__ballot(ok && !keep) == 0) break;  // every point of the wave is placed
      if (s >= sm[b].w0 && s < sm[b].w1 && sp_in_box(sm[b], x, y, z)) keep = true;
    }
  }
  if (ok) flag[i] = keep ? 1 : 0;
}

__device__ __forceinline__ uint64_t sp_key(const SPGrid& g, double x, double y, double z) {
  const uint64_t ix = (uint64_t)((int64_t)floor(x * g.inv_cell) - g.bx);
  const uint64_t iy = (uint64_t)((int64_t)floor(y * g.inv_cell) - g.by);
  const uint64_t iz = (uint64_t)((int64_t)floor(z * g.inv_cell) - g.bz);
  return (ix << g.sy) | (iy << g.sz) | iz;
}

// pos = exclusive scan of the flags.  A survivor lies strictly inside a box, so its indices are inside the range the host
// derived from the boxes (floor and the product are monotone) and fit their key fields.
__global__ __launch_bounds__(AI_BLOCK) void ks_keys(const double* __restrict__ xyz, int64_t n, const int64_t* __restrict__ scan_off,
                                                    int32_t n_scans, const double* __restrict__ T, const int32_t* __restrict__ pos,
                                                    SPGrid g, uint64_t* __restrict__ key, int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t p = pos[i];
  if (pos[i + 1] == p) return;
  double x, y, z;
  sp_source(xyz, scan_off, n_scans, T, i, x, y, z);
  key[p] = sp_key(g, x, y, z);
  idx[p] = (int32_t)i;
}

// the survivors in sort order: transformed coordinates, scan position; ukey[v] = the key of occupied cell v (ascending)
__global__ __launch_bounds__(AI_BLOCK) void ks_gather(const double* __restrict__ xyz, const int64_t* __restrict__ scan_off,
                                                      int32_t n_scans, const double* __restrict__ T, const int32_t* __restrict__ order,
                                                      const uint64_t* __restrict__ skey, const int32_t* __restrict__ vid, int64_t n,
                                                      double* __restrict__ X, double* __restrict__ Y, double* __restrict__ Z,
                                                      int32_t* __restrict__ S, uint64_t* __restrict__ ukey) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p >= n) return;
  double x, y, z;
  S[p] = sp_source(xyz, scan_off, n_scans, T, order[p], x, y, z);
  X[p] = x;
  Y[p] = y;
  Z[p] = z;
  if (vid[p + 1] != vid[p]) ukey[vid[p]] = skey[p];  // p is the head of its cell's run
}

// 16 lanes per query.  MAXK = ceil(dim / 16) accumulators per lane (6: dim <= 96, 24: dim <= 384).
// Lane t < 9 finds the run of row (ix + t / 3 - 1, iy + t % 3 - 1), cells iz - 1 .. iz + 1 clamped to the iz field (so that a range
// never reaches into the neighbouring row); the rows are then visited in ascending (ix, iy), which with iz in the low key bits is
// ascending key order.  In a run lane t tests candidate base + t (R2); the group walks the hits in candidate order (R4).
template <int MAXK>
__global__ __launch_bounds__(AI_BLOCK) void ks_pool(const double* __restrict__ q, int64_t nq, const int64_t* __restrict__ query_off,
                                                    int32_t n_chunks, const SPChunk* __restrict__ chunks, SPGrid g, double radius,
                                                    int64_t m, const uint64_t* __restrict__ ukey, const int32_t* __restrict__ start,
                                                    const double* __restrict__ X, const double* __restrict__ Y,
                                                    const double* __restrict__ Z, const int32_t* __restrict__ S,
                                                    const int32_t* __restrict__ order, const float* __restrict__ feat, int32_t dim,
                                                    double* __restrict__ out, int32_t* __restrict__ count, int32_t* __restrict__ err) {
  const int64_t gid = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const int64_t i = gid >> 4;
  const int t = (int)(gid & 15);
  if (i >= nq) return;
  const int shift = (int)(threadIdx.x & 48);  // where the group's 16 bits sit in the wave's ballot
  const double x = q[i * 3], y = q[i * 3 + 1], z = q[i * 3 + 2];
  const SPChunk ck = chunks[segment_of(query_off, n_chunks, i)];
  const double fx = floor(x * g.inv_cell), fy = floor(y * g.inv_cell), fz = floor(z * g.inv_cell);
  double acc[MAXK];
#pragma unroll
  for (int k = 0; k < MAXK; ++k) acc[k] = 0.0;
  int cnt = 0;
  // a NaN or an infinite coordinate fails the comparison: no search, a zero row, and the call reports the bad argument
  const bool sane = fabs(fx) < SP_MAX_INDEX && fabs(fy) < SP_MAX_INDEX && fabs(fz) < SP_MAX_INDEX;
  if (!sane && t == 0) atomicOr(err, 2);
  int32_t rs = 0, re = 0;
  if (sane && t < 9) {
    const int64_t xx = (int64_t)fx - g.bx + (t / 3 - 1), yy = (int64_t)fy - g.by + (t % 3 - 1), zz = (int64_t)fz - g.bz;
    const int64_t z0 = max(zz - 1, (int64_t)0), z1 = min(zz + 1, (int64_t)g.nz - 1);
    if (xx >= 0 && xx < g.nx && yy >= 0 && yy < g.ny && z0 <= z1) {
      const uint64_t row = ((uint64_t)xx << g.sy) | ((uint64_t)yy << g.sz);
      const uint64_t klo = row | (uint64_t)z0, khi = row | (uint64_t)z1;
      int64_t a = 0, b = m;
      while (a < b) {  // first occupied cell with ukey >= klo
        const int64_t h = (a + b) >> 1;
        if (ukey[h] < klo)
          a = h + 1;
        else
          b = h;
      }
      int64_t u = a;
      while (u < m && ukey[u] <= khi) ++u;  // at most three steps
      if (u > a) {
        rs = start[a];
        re = start[u];
      }
    }
  }
  const double r2 = radius * radius;
  for (int r = 0; r < 9; ++r) {
    const int32_t s = __shfl(rs, r, 16), e = __shfl(re, r, 16);
    for (int32_t base = s; base < e; base += 16) {
      const int32_t p = base + t;
      bool hit = false;
      if (p < e) {
        const int32_t sc = S[p];
        const double px = X[p], py = Y[p], pz = Z[p];
        hit = sc >= ck.w0 && sc < ck.w1 && sp_in_box(ck, px, py, pz) && sq_dist3(x, y, z, px, py, pz) < r2;
      }
      uint32_t bits = (uint32_t)(__ballot(hit) >> shift) & 0xffffu;
      while (bits) {
        const int j = __ffs(bits) - 1;
        bits &= bits - 1;
        const float* f = feat + (int64_t)order[base + j] * dim;
#pragma unroll
        for (int k = 0; k < MAXK; ++k) {
          const int c = t + 16 * k;
          if (c < dim) acc[k] += (double)f[c];
        }
        ++cnt;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    const int c = t + 16 * k;
    if (c < dim) out[i * dim + c] = cnt ? acc[k] / (double)cnt : 0.0;  // R3: sum, then one division
  }
  if (t == 0 && count) count[i] = cnt;
}

}  // namespace

extern "C" int ai_scan_pool(ai_ctx* ctx, const double* scan_xyz, const int64_t* scan_off, int32_t n_scans, const double* T_scan2pcd,
                            const float* scan_feat, int32_t dim, const double* query_xyz, const int64_t* query_off, int32_t n_chunks,
                            const double* boxes, const int32_t* scan_win, double radius, int mem_kind, double* out, int32_t* count_out) {
  const auto bad = [](const char* what) { return bad_arg("ai_scan_pool", what); };
  if (!ctx || !scan_off || !query_off || n_scans < 0 || n_chunks < 0) return bad("null pointer or negative count");
  if (dim < 1 || dim > 384) return bad("dim must be 1 .. 384");
  if (!(radius > 0.0) || !std::isfinite(radius)) return bad("radius must be positive and finite");
  if (scan_off[0] != 0 || query_off[0] != 0) return bad("an offset array must start at 0");
  for (int32_t s = 0; s < n_scans; ++s)
    if (scan_off[s + 1] < scan_off[s]) return bad("scan_off is not monotone");
  for (int32_t c = 0; c < n_chunks; ++c)
    if (query_off[c + 1] < query_off[c]) return bad("query_off is not monotone");
  const int64_t M = scan_off[n_scans], Nq = query_off[n_chunks];
  const int64_t lim = ((int64_t)1 << 31) - AI_BLOCK;
  if (M >= lim || Nq >= lim) return bad("M and Nq must be below 2^31 - 256");
  if ((n_scans > 0 && !T_scan2pcd) || (n_chunks > 0 && (!boxes || !scan_win)) || (M > 0 && (!scan_xyz || !scan_feat)) ||
      (Nq > 0 && (!query_xyz || !out)))
    return bad("null pointer");
  for (int32_t s = 0; s < n_scans; ++s) {
    const double* T = T_scan2pcd + (size_t)s * 16;
    for (int k = 0; k < 12; ++k)
      if (!std::isfinite(T[k])) return bad("T_scan2pcd is not finite");
    if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0) return bad("the last row of T_scan2pcd must be (0, 0, 0, 1)");
  }
  const double cell = radius * (1.0 + 1e-9), inv_cell = 1.0 / cell;
  std::vector<SPChunk> hc((size_t)std::max(n_chunks, 1));
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int32_t c = 0; c < n_chunks; ++c) {
    SPChunk& k = hc[c];
    for (int a = 0; a < 3; ++a) {
      k.lo[a] = boxes[(size_t)c * 6 + a];
      k.hi[a] = boxes[(size_t)c * 6 + 3 + a];
      if (!std::isfinite(k.lo[a]) || !std::isfinite(k.hi[a])) return bad("a box bound is not finite");
      lo[a] = std::min(lo[a], k.lo[a]);
      hi[a] = std::max(hi[a], k.hi[a]);
    }
    k.w0 = scan_win[(size_t)c * 2];
    k.w1 = scan_win[(size_t)c * 2 + 1];
    if (k.w0 < 0 || k.w1 > n_scans || k.w0 > k.w1) return bad("scan_win must satisfy 0 <= first <= last <= n_scans");
  }
  if (M == 0 && Nq == 0) return AI_OK;  // nothing to examine and nothing to write
  // the key fields: every survivor is strictly inside a box, so its index lies in floor(lo * inv) .. floor(hi * inv) per axis.
  // Without a query nothing is keyed (the scans' coordinates are still examined below), and there may be no box at all.
  SPGrid g = {};
  g.inv_cell = inv_cell;
  int bits[3] = {0, 0, 0};
  int32_t bias[3] = {0, 0, 0};
  for (int a = 0; a < 3 && Nq > 0; ++a) {
    const double i0 = floor(lo[a] * inv_cell), i1 = floor(hi[a] * inv_cell);
    if (!(fabs(i0) < SP_MAX_INDEX) || !(fabs(i1) < SP_MAX_INDEX)) return bad("a cell index does not fit its key field (|index| >= 2^30)");
    bias[a] = (int32_t)i0;
    bits[a] = bits_for(std::max((int64_t)i1 - (int64_t)i0 + 1, (int64_t)1));
    if (bits[a] > 30) return bad("a cell index does not fit its key field (the boxes span 2^30 cells or more on an axis)");
  }
  if (bits[0] + bits[1] + bits[2] > 63) return bad("the cell indices of the boxes do not fit a 64-bit key");
  g.bx = bias[0];
  g.by = bias[1];
  g.bz = bias[2];
  g.nx = 1 << bits[0];
  g.ny = 1 << bits[1];
  g.nz = 1 << bits[2];
  g.sz = bits[2];
  g.sy = bits[1] + bits[2];

  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<double> own_s, own_q, d_T, d_out, X, Y, Z;
  DevBuf<float> own_f;
  DevBuf<int64_t> d_soff, d_qoff;
  DevBuf<SPChunk> d_chunks;
  DevBuf<int32_t> d_cnt, pos, scan_tmp, d_err, idx, order, vid, start, S;
  DevBuf<uint64_t> key, skey;
  const double *ds = nullptr, *dq = nullptr;
  const float* df = nullptr;
  if (M > 0) {
    AI_TRY(to_device(scan_xyz, (size_t)M * 3, mem_kind, own_s, &ds, st));
    if (Nq > 0) AI_TRY(to_device(scan_feat, (size_t)M * dim, mem_kind, own_f, &df, st));
  }
  if (Nq > 0) AI_TRY(to_device(query_xyz, (size_t)Nq * 3, mem_kind, own_q, &dq, st));
  AI_TRY(d_T.alloc((size_t)std::max(n_scans, 1) * 16));
  AI_TRY(d_soff.alloc((size_t)n_scans + 1));
  AI_TRY(d_qoff.alloc((size_t)n_chunks + 1));
  AI_TRY(d_chunks.alloc((size_t)n_chunks));
  AI_TRY(d_err.alloc(1));
  if (n_scans > 0) AI_HIP(hipMemcpyAsync(d_T.p, T_scan2pcd, (size_t)n_scans * 16 * sizeof(double), hipMemcpyHostToDevice, st));
  AI_HIP(hipMemcpyAsync(d_soff.p, scan_off, ((size_t)n_scans + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  AI_HIP(hipMemcpyAsync(d_qoff.p, query_off, ((size_t)n_chunks + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  if (n_chunks > 0) AI_HIP(hipMemcpyAsync(d_chunks.p, hc.data(), (size_t)n_chunks * sizeof(SPChunk), hipMemcpyHostToDevice, st));
  AI_HIP(hipMemsetAsync(d_err.p, 0, sizeof(int32_t), st));

  int32_t ns = 0, m = 0, herr = 0;
  if (M > 0) {
    AI_TRY(pos.alloc((size_t)M + 1));
    AI_TRY(scan_tmp.alloc(ai_scan_tmp_elems(M)));
    hipLaunchKernelGGL(ks_flag, dim3(grid_for(M)), dim3(AI_BLOCK), 0, st, ds, M, (const int64_t*)d_soff.p, n_scans, (const double*)d_T.p,
                       (const SPChunk*)d_chunks.p, n_chunks, pos.p, d_err.p);
    AI_KERNEL_CHECK();
    AI_TRY(ai_exclusive_scan_i32(st, pos.p, pos.p, M, scan_tmp.p));
    AI_HIP(hipMemcpyAsync(&ns, pos.p + M, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AI_HIP(hipMemcpyAsync(&herr, d_err.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AI_HIP(hipStreamSynchronize(st));
    if (herr) return bad("a scan coordinate is not finite");
  }
  if (Nq == 0) return AI_OK;  // no chunk has a query: the arguments are checked, there is nothing to write
  AI_TRY(key.alloc(ns));
  AI_TRY(skey.alloc(ns));
  AI_TRY(idx.alloc(ns));
  AI_TRY(order.alloc(ns));
  AI_TRY(vid.alloc((size_t)ns + 1));
  AI_TRY(start.alloc((size_t)ns + 1));
  AI_TRY(X.alloc(ns));
  AI_TRY(Y.alloc(ns));
  AI_TRY(Z.alloc(ns));
  AI_TRY(S.alloc(ns));
  uint64_t* ukey = key.p;  // the unsorted keys are dead after the sort: their buffer holds the table of occupied cells
  if (ns > 0) {
    DevBuf<int32_t> scan_tmp2;
    DevBuf<uint8_t> tmp;
    const unsigned gb = grid_for(ns);
    hipLaunchKernelGGL(ks_keys, dim3(grid_for(M)), dim3(AI_BLOCK), 0, st, ds, M, (const int64_t*)d_soff.p, n_scans, (const double*)d_T.p,
                       (const int32_t*)pos.p, g, key.p, idx.p);
    AI_KERNEL_CHECK();
    const int kbits = std::max(1, bits[0] + bits[1] + bits[2]);
    AI_TRY(sort_pairs(st, key.p, skey.p, idx.p, order.p, (int64_t)ns, kbits, tmp));
    AI_TRY(scan_tmp2.alloc(ai_scan_tmp_elems(ns)));
    hipLaunchKernelGGL(kl_heads<uint64_t>, dim3(gb), dim3(AI_BLOCK), 0, st, (const uint64_t*)skey.p, (int64_t)ns, vid.p);
    AI_KERNEL_CHECK();
    AI_TRY(ai_exclusive_scan_i32(st, vid.p, vid.p, ns, scan_tmp2.p));
    hipLaunchKernelGGL(kv_starts, dim3(grid_for((int64_t)ns + 1)), dim3(AI_BLOCK), 0, st, (const int32_t*)vid.p, (int64_t)ns, start.p);
    AI_KERNEL_CHECK();
    AI_HIP(hipMemcpyAsync(&m, vid.p + ns, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(ks_gather, dim3(gb), dim3(AI_BLOCK), 0, st, ds, (const int64_t*)d_soff.p, n_scans, (const double*)d_T.p,
                       (const int32_t*)order.p, (const uint64_t*)skey.p, (const int32_t*)vid.p, (int64_t)ns, X.p, Y.p, Z.p, S.p, ukey);
    AI_KERNEL_CHECK();
    AI_HIP(hipStreamSynchronize(st));  // m; tmp and scan_tmp2 go out of scope
  }
  double* o = out;
  int32_t* c = count_out;
  if (mem_kind != AI_MEM_DEVICE) {
    AI_TRY(d_out.alloc((size_t)Nq * dim));
    o = d_out.p;
    if (count_out) {
      AI_TRY(d_cnt.alloc(Nq));
      c = d_cnt.p;
    }
  }
  const unsigned gq = grid_for(Nq * 16);
  if (dim <= 96)
    hipLaunchKernelGGL(ks_pool<6>, dim3(gq), dim3(AI_BLOCK), 0, st, dq, Nq, (const int64_t*)d_qoff.p, n_chunks, (const SPChunk*)d_chunks.p,
                       g, radius, (int64_t)m, (const uint64_t*)ukey, (const int32_t*)start.p, (const double*)X.p, (const double*)Y.p,
                       (const double*)Z.p, (const int32_t*)S.p, (const int32_t*)order.p, df, dim, o, c, d_err.p);
  else
    hipLaunchKernelGGL(ks_pool<24>, dim3(gq), dim3(AI_BLOCK), 0, st, dq, Nq, (const int64_t*)d_qoff.p, n_chunks, (const SPChunk*)d_chunks.p,
                       g, radius, (int64_t)m, (const uint64_t*)ukey, (const int32_t*)start.p, (const double*)X.p, (const double*)Y.p,
                       (const double*)Z.p, (const int32_t*)S.p, (const int32_t*)order.p, df, dim, o, c, d_err.p);
  AI_KERNEL_CHECK();
  AI_HIP(hipMemcpyAsync(&herr, d_err.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (mem_kind != AI_MEM_DEVICE) {
    AI_HIP(hipMemcpyAsync(out, o, (size_t)Nq * dim * sizeof(double), hipMemcpyDeviceToHost, st));
    if (count_out) AI_HIP(hipMemcpyAsync(count_out, c, (size_t)Nq * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  }
  AI_HIP(hipStreamSynchronize(st));
  if (herr) return bad("a query coordinate is not finite, or its cell index does not fit (|index| >= 2^30)");
  return AI_OK;
}
