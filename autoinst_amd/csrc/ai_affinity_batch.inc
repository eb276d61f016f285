// ai_affinity_build_batch: the affinity graphs of many chunks in one call (DESIGN.md section 24).  Included at the end of
// ai_affinity.hip: it launches that file's kernels (k_nb_unstash, k_count_total, k_count_over, k_zero_rows and the weight
// kernels through launch_weights) on the rows of a whole GROUP of chunks, and shares the walk (nb_walk) and the grid
// (affinity_grid) with the single build.
//
// A group lives in one position space: row p of the group is a row of exactly one chunk, chunk c owning the positions
// rows[c] .. rows[c + 1], which are also its rows of the caller's concatenated input counted from the group's first row.  Every
// chunk has its own grid (BGrid); a stable sort on (chunk, Morton key) leaves each chunk's rows in the single build's order
// inside its own range; columns are group positions until k_b_split_* writes each chunk's CSR with local ids.
namespace {

struct BGrid {  // the grid of one chunk of a group and where its cells start in the group's cell tables
  double minx, miny, minz, inv_cell;
  int nx, ny, nz, pad;
  int64_t cell0;
};

struct BOut {  // the buffers of one chunk's graph
  int32_t* rowptr;
  int32_t* col;
  double* val;
  int32_t* orig;
  double* xyz;
};

#define AB_PART 7  // per-block bounds record: min xyz, max xyz, "a coordinate is not finite"

// segmented bounding box: block (s, c) folds the rows s, s + S, ... (in units of AI_BLOCK) of chunk c -> part[c][s][AB_PART]
__global__ __launch_bounds__(AI_BLOCK) void k_b_bounds(const double* __restrict__ xyz, const int32_t* __restrict__ rows,
                                                       double* __restrict__ part) {
  __shared__ double sm[6][AI_BLOCK / 64];
  __shared__ int s_bad;
  const int c = blockIdx.y;
  const int64_t r0 = rows[c], r1 = rows[c + 1];
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
  bool bad = false;
  for (int64_t i = r0 + (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x; i < r1; i += (int64_t)gridDim.x * AI_BLOCK) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double v = xyz[i * 3 + a];
      bad |= !(fabs(v) <= 1.7976931348623157e308);  // NaN or infinite (fmin / fmax alone would pass a NaN by)
      mn[a] = fmin(mn[a], v);
      mx[a] = fmax(mx[a], v);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[a] = fmin(mn[a], __shfl_xor(mn[a], o, 64));
      mx[a] = fmax(mx[a], __shfl_xor(mx[a], o, 64));
    }
  }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      sm[a][w] = mn[a];
      sm[3 + a][w] = mx[a];
    }
  }
  if (bad) s_bad = 1;
  __syncthreads();
  double* out = part + ((int64_t)c * gridDim.x + blockIdx.x) * AB_PART;
  if (threadIdx.x < 6) {
    double r = sm[threadIdx.x][0];
    for (int i = 1; i < AI_BLOCK / 64; ++i) r = (threadIdx.x < 3) ? fmin(r, sm[threadIdx.x][i]) : fmax(r, sm[threadIdx.x][i]);
    out[threadIdx.x] = r;
  }
  if (threadIdx.x == 6) out[6] = s_bad ? 1.0 : 0.0;
}

// the chunk of row i: the c with rows[c] <= i < rows[c + 1] (no chunk is empty)
__device__ __forceinline__ int b_chunk_of(const int32_t* __restrict__ rows, int nc, int32_t i) {
  int lo = 0, hi = nc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// sort key (chunk, Morton cell key in the chunk's own grid) and the row's chunk, which is also the chunk of POSITION i after
// the sort (a chunk's rows stay inside its range)
__global__ __launch_bounds__(AI_BLOCK) void k_b_cell_keys(const double* __restrict__ xyz, int64_t n, const int32_t* __restrict__ rows,
                                                          int nc, const BGrid* __restrict__ grids, uint64_t* __restrict__ key,
                                                          int32_t* __restrict__ idx, int32_t* __restrict__ rchunk) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int c = b_chunk_of(rows, nc, (int32_t)i);
  const BGrid b = grids[c];
  Grid g;
  g.minx = b.minx, g.miny = b.miny, g.minz = b.minz, g.inv_cell = b.inv_cell, g.nx = b.nx, g.ny = b.ny, g.nz = b.nz;
  int cx, cy, cz;
  cell_of(g, xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], cx, cy, cz);
  const uint32_t m = part1by2((uint32_t)cx) | (part1by2((uint32_t)cy) << 1) | (part1by2((uint32_t)cz) << 2);
  key[i] = ((uint64_t)c << 30) | (uint64_t)m;
  idx[i] = (int32_t)i;
  rchunk[i] = c;
}

// sorted SoA coordinates + linear cell id (in the chunk's grid) per position
__global__ __launch_bounds__(AI_BLOCK) void k_b_gather_sorted(const double* __restrict__ xyz, const int32_t* __restrict__ orig, int64_t n,
                                                              const int32_t* __restrict__ rchunk, const BGrid* __restrict__ grids,
                                                              double* __restrict__ X, double* __restrict__ Y, double* __restrict__ Z,
                                                              int32_t* __restrict__ cellid) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p >= n) return;
  const int64_t o = orig[p];
  const double x = xyz[o * 3], y = xyz[o * 3 + 1], z = xyz[o * 3 + 2];
  X[p] = x;
  Y[p] = y;
  Z[p] = z;
  const BGrid b = grids[rchunk[p]];
  Grid g;
  g.minx = b.minx, g.miny = b.miny, g.minz = b.minz, g.inv_cell = b.inv_cell, g.nx = b.nx, g.ny = b.ny, g.nz = b.nz;
  int cx, cy, cz;
  cell_of(g, x, y, z, cx, cy, cz);
  cellid[p] = (cz * g.ny + cy) * g.nx + cx;
}

// cell ranges (group positions) in the concatenated cell tables: chunk c's cells start at grids[c].cell0
__global__ __launch_bounds__(AI_BLOCK) void k_b_cell_ranges(const int32_t* __restrict__ cellid, const int32_t* __restrict__ rchunk, int64_t n,
                                                            const BGrid* __restrict__ grids, int32_t* __restrict__ cstart,
                                                            int32_t* __restrict__ cend) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p >= n) return;
  const int32_t c = cellid[p], ch = rchunk[p];
  const int64_t at = grids[ch].cell0 + c;
  if (p == 0 || rchunk[p - 1] != ch || cellid[p - 1] != c) cstart[at] = (int32_t)p;
  if (p == n - 1 || rchunk[p + 1] != ch || cellid[p + 1] != c) cend[at] = (int32_t)(p + 1);
}

// k_neighbours on a group: the row's chunk grid is loaded ONCE per row (its three sizes and where its cells start); the walk
// itself is nb_walk, with the cell tables offset to the chunk's cells, so no candidate waits for the grid table
template <bool FILL>
__global__ __launch_bounds__(AI_BLOCK) void k_b_neighbours(const double* __restrict__ X, const double* __restrict__ Y,
                                                           const double* __restrict__ Z, const int32_t* __restrict__ cellid,
                                                           const int32_t* __restrict__ rchunk, const BGrid* __restrict__ grids,
                                                           const int32_t* __restrict__ cstart, const int32_t* __restrict__ cend, int64_t n,
                                                           double radius, int32_t* __restrict__ cnt, const int32_t* __restrict__ rowptr,
                                                           int32_t* __restrict__ col, double* __restrict__ dist,
                                                           int32_t* __restrict__ stash_col, double* __restrict__ stash_dist, int stash_cap,
                                                           const int32_t* __restrict__ cnt_in) {
  const int64_t gid = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const int64_t p = gid / AI_NB_LANES;
  const int l = (int)(gid % AI_NB_LANES);
  const int sub = (threadIdx.x & 63) / AI_NB_LANES;
  const bool live = p < n && !(FILL && cnt_in != nullptr && cnt_in[p < n ? p : 0] <= stash_cap);
  const int64_t pp = live ? p : n - 1;
  const double x = X[pp], y = Y[pp], z = Z[pp];
  const int32_t c = cellid[pp];
  const BGrid* b = grids + rchunk[pp];
  const int nx = b->nx, ny = b->ny, nz = b->nz;
  const int64_t cell0 = b->cell0;
  const int32_t base = (FILL && live) ? rowptr[p] : 0;
  const int32_t k = nb_walk<FILL>(X, Y, Z, cstart + cell0, cend + cell0, nx, ny, nz, live, p, l, sub, x, y, z, c, radius, base, col, dist,
                                  stash_col, stash_dist, stash_cap);
  if (!FILL && live && l == 0) cnt[p] = k;
}

// first entry of every chunk (and the group's total) out of the group's row pointers
__global__ __launch_bounds__(AI_BLOCK) void k_b_chunk_entries(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ rows, int nc,
                                                              int32_t* __restrict__ ebase) {
  const int c = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (c <= nc) ebase[c] = rowptr[rows[c]];
}

// the group's position space into per-chunk graphs, rows: local row pointers, local original ids, the chunk's points
__global__ __launch_bounds__(AI_BLOCK) void k_b_split_rows(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ orig,
                                                           const double* __restrict__ xyz, const int32_t* __restrict__ rchunk,
                                                           const int32_t* __restrict__ rows, int64_t n, const BOut* __restrict__ outs) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int c = rchunk[i];
  const int32_t r0 = rows[c];
  const int64_t li = i - r0;
  const BOut o = outs[c];
  const int32_t e0 = rowptr[r0];
  o.rowptr[li] = rowptr[i] - e0;
  if (i + 1 == rows[c + 1]) o.rowptr[li + 1] = rowptr[i + 1] - e0;
  o.orig[li] = orig[i] - r0;
  o.xyz[li * 3] = xyz[i * 3];
  o.xyz[li * 3 + 1] = xyz[i * 3 + 1];
  o.xyz[li * 3 + 2] = xyz[i * 3 + 2];
}

// ... and entries: AI_NB_LANES lanes per row copy its columns (made local) and values
__global__ __launch_bounds__(AI_BLOCK) void k_b_split_entries(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                              const double* __restrict__ val, const int32_t* __restrict__ rchunk,
                                                              const int32_t* __restrict__ rows, int64_t n, const BOut* __restrict__ outs) {
  const int64_t gid = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const int64_t p = gid / AI_NB_LANES;
  const int l = (int)(gid % AI_NB_LANES);
  if (p >= n) return;
  const int c = rchunk[p];
  const int32_t r0 = rows[c];
  const BOut o = outs[c];
  const int32_t e0 = rowptr[r0];
  const int32_t s = rowptr[p], e = rowptr[p + 1];
  for (int32_t k = s + l; k < e; k += AI_NB_LANES) {
    o.col[k - e0] = col[k] - r0;
    o.val[k - e0] = val[k];
  }
}

}  // namespace

// ----------------------------------------------------------------------------- host side
#define AB_DEFAULT_GROUP_ROWS ((int64_t)1 << 21)
#define AB_SPLIT 1  // (internal status) the group does not fit an int32 counter or the cell-table limit: halve it and redo

// The chunks lo .. hi of the call in groups of whole chunks: at most `budget` rows each (a larger chunk is a group of its own),
// and a group of several chunks stays inside what its int32 position space and the tiled weights' 32-bit staging offsets hold
// (fewer than 2^30 rows, rows x widest feature < 2^33), so that its weights path is the one every chunk of it takes alone.
static std::vector<int32_t> affinity_groups(const int64_t* off, int32_t n_chunks, int64_t budget, int64_t widest) {
  std::vector<int32_t> cut(1, 0);
  const int64_t cap = std::min((int64_t)1 << 30, widest > 0 ? (((int64_t)1 << 33) + widest - 1) / widest : (int64_t)1 << 30);
  const int64_t lim = std::min(budget, cap - 1);
  for (int32_t c = 0; c < n_chunks; ++c)
    if (c > cut.back() && off[c + 1] - off[cut.back()] > lim) cut.push_back(c);
  cut.push_back(n_chunks);
  return cut;
}

namespace {
struct BatchCall {
  ai_ctx* ctx;
  const double *xyz, *tarl, *dino;
  const int64_t* off;
  int32_t tarl_dim, dino_dim;
  double alpha, theta, gamma, radius;
  int mem_kind;
  ai_csr** out;
  std::vector<ai_csr*> made;  // graphs registered so far: freed together when the call fails
  // tables a group uploads (they outlive the group's function: a failed group's copies may still be in flight when it returns)
  std::vector<int32_t> hrows;
  std::vector<BGrid> hgrid;
  std::vector<BOut> houts;
};
}  // namespace

// one group: chunks lo .. hi - 1.  AI_OK, AB_SPLIT (nothing made for this group) or an error.
static int affinity_build_group(BatchCall& B, int32_t lo, int32_t hi) {
  ai_ctx* ctx = B.ctx;
  hipStream_t st = ctx->stream;
  const int nc = hi - lo;
  const int64_t row0 = B.off[lo], n = B.off[hi] - row0;
  ctx->arena.rewind();  // the previous group has drained: its workspace is this group's
  DevBuf<double> own_xyz, own_tarl, own_dino;
  const double *d_xyz, *d_tarl, *d_dino;
  const int32_t tdim = B.tarl_dim, ddim = B.dino_dim;
  AI_TRY(upload_if_host(B.xyz + row0 * 3, (size_t)n * 3, B.mem_kind, own_xyz, &d_xyz, st));
  AI_TRY(upload_if_host(B.theta != 0.0 ? B.tarl + row0 * tdim : nullptr, (size_t)n * (size_t)tdim, B.mem_kind, own_tarl, &d_tarl, st));
  AI_TRY(upload_if_host(B.gamma != 0.0 ? B.dino + row0 * ddim : nullptr, (size_t)n * (size_t)ddim, B.mem_kind, own_dino, &d_dino, st));

  // ---- bounds of every chunk: one launch, one host round trip for the group
  std::vector<int32_t>& hrows = B.hrows;
  hrows.assign((size_t)nc + 1, 0);
  int64_t longest = 0;
  for (int c = 0; c <= nc; ++c) hrows[c] = (int32_t)(B.off[lo + c] - row0);
  for (int c = 0; c < nc; ++c) longest = std::max<int64_t>(longest, hrows[c + 1] - hrows[c]);
  const int S = (int)std::min<int64_t>(256, std::max<int64_t>(1, (longest + 16 * AI_BLOCK - 1) / (16 * AI_BLOCK)));
  DevBuf<int32_t> rows;
  DevBuf<double> part;
  AI_TRY(rows.alloc((size_t)nc + 1));
  AI_TRY(part.alloc((size_t)nc * S * AB_PART));
  AI_HIP(hipMemcpyAsync(rows.p, hrows.data(), hrows.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_b_bounds, dim3(S, nc), dim3(AI_BLOCK), 0, st, d_xyz, (const int32_t*)rows.p, part.p);
  AI_KERNEL_CHECK();
  std::vector<double> hpart((size_t)nc * S * AB_PART);
  AI_HIP(hipMemcpyAsync(hpart.data(), part.p, hpart.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  std::vector<BGrid>& hgrid = B.hgrid;
  hgrid.assign((size_t)nc, BGrid{});
  int64_t ncell = 0;
  for (int c = 0; c < nc; ++c) {
    double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
    bool bad = false;
    for (int s = 0; s < S; ++s) {
      const double* r = &hpart[((size_t)c * S + s) * AB_PART];
      for (int a = 0; a < 3; ++a) {
        if (r[a] < mn[a]) mn[a] = r[a];
        if (r[3 + a] > mx[a]) mx[a] = r[3 + a];
      }
      bad = bad || r[6] != 0.0;
    }
    Grid g;
    int64_t cells = 0;
    double ext[3];
    const int why = bad ? 1 : affinity_grid(mn, mx, B.radius, g, cells, ext);
    if (why == 1) {
      ai_set_error("ai_affinity_build_batch: chunk %d: coordinates are not finite", lo + c);
      return AI_ERR_BAD_ARG;
    }
    if (why == 2) {
      ai_set_error("ai_affinity_build_batch: chunk %d: extent / radius = (%.0f, %.0f, %.0f) exceeds 1023 cells per axis", lo + c, ext[0],
                   ext[1], ext[2]);
      return AI_ERR_BAD_ARG;
    }
    if (why == 3) {
      ai_set_error("ai_affinity_build_batch: chunk %d: %lld grid cells exceed the dense cell-table limit", lo + c, (long long)cells);
      return AI_ERR_BAD_ARG;
    }
    BGrid& b = hgrid[c];
    b.minx = g.minx, b.miny = g.miny, b.minz = g.minz, b.inv_cell = g.inv_cell;
    b.nx = g.nx, b.ny = g.ny, b.nz = g.nz, b.pad = 0;
    b.cell0 = ncell;
    ncell += cells;
  }
  // the cell tables of a group stay within what ONE chunk may ask for, so a call never needs more than its loop
  if (nc > 1 && ncell > ((int64_t)1 << 28)) return AB_SPLIT;

  const unsigned gb = (unsigned)((n + AI_BLOCK - 1) / AI_BLOCK);
  const unsigned gnb = (unsigned)((n * AI_NB_LANES + AI_BLOCK - 1) / AI_BLOCK);
  constexpr int AI_NB_STASH = 128;
  DevBuf<BGrid> grids;
  DevBuf<uint64_t> key, key2;
  DevBuf<int32_t> idx, orig, rchunk, cellid, cstart, cend, cnt, scantmp, rowptr, ebase, stash_col;
  DevBuf<double> X, Y, Z, stash_dist;
  DevBuf<unsigned long long> total;
  AI_TRY(grids.alloc((size_t)nc));
  AI_TRY(key.alloc(n));
  AI_TRY(key2.alloc(n));
  AI_TRY(idx.alloc(n));
  AI_TRY(orig.alloc(n));
  AI_TRY(rchunk.alloc(n));
  AI_HIP(hipMemcpyAsync(grids.p, hgrid.data(), hgrid.size() * sizeof(BGrid), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_b_cell_keys, dim3(gb), dim3(AI_BLOCK), 0, st, d_xyz, n, (const int32_t*)rows.p, nc, (const BGrid*)grids.p, key.p, idx.p,
                     rchunk.p);
  AI_KERNEL_CHECK();
  {
    int cbits = 0;
    while (((int64_t)1 << cbits) < nc) ++cbits;
    size_t tmp_bytes = 0;
    AI_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, key.p, key2.p, idx.p, orig.p, (size_t)n, 0, 30 + cbits, st));
    DevBuf<uint8_t> tmp;
    AI_TRY(tmp.alloc(tmp_bytes));
    AI_HIP(rocprim::radix_sort_pairs(tmp.p, tmp_bytes, key.p, key2.p, idx.p, orig.p, (size_t)n, 0, 30 + cbits, st));
    if (!ai_current_arena()) AI_HIP(hipStreamSynchronize(st));
  }
  AI_TRY(X.alloc(n));
  AI_TRY(Y.alloc(n));
  AI_TRY(Z.alloc(n));
  AI_TRY(cellid.alloc(n));
  AI_TRY(cstart.alloc(ncell));
  AI_TRY(cend.alloc(ncell));
  AI_TRY(cnt.alloc(n + 1));
  AI_TRY(rowptr.alloc(n + 1));
  AI_TRY(ebase.alloc((size_t)nc + 1));
  AI_TRY(scantmp.alloc(ai_scan_tmp_elems(n)));
  AI_TRY(stash_col.alloc((size_t)n * AI_NB_STASH));
  AI_TRY(stash_dist.alloc((size_t)n * AI_NB_STASH));
  AI_TRY(total.alloc(2));
  hipLaunchKernelGGL(k_b_gather_sorted, dim3(gb), dim3(AI_BLOCK), 0, st, d_xyz, (const int32_t*)orig.p, n, (const int32_t*)rchunk.p,
                     (const BGrid*)grids.p, X.p, Y.p, Z.p, cellid.p);
  AI_KERNEL_CHECK();
  AI_HIP(hipMemsetAsync(cstart.p, 0xff, (size_t)ncell * sizeof(int32_t), st));
  AI_HIP(hipMemsetAsync(cend.p, 0, (size_t)ncell * sizeof(int32_t), st));
  hipLaunchKernelGGL(k_b_cell_ranges, dim3(gb), dim3(AI_BLOCK), 0, st, (const int32_t*)cellid.p, (const int32_t*)rchunk.p, n,
                     (const BGrid*)grids.p, cstart.p, cend.p);
  AI_KERNEL_CHECK();
  hipLaunchKernelGGL(k_b_neighbours<false>, dim3(gnb), dim3(AI_BLOCK), 0, st, X.p, Y.p, Z.p, cellid.p, rchunk.p, grids.p, cstart.p, cend.p, n,
                     B.radius, cnt.p, (const int32_t*)nullptr, (int32_t*)nullptr, (double*)nullptr, stash_col.p, stash_dist.p, AI_NB_STASH,
                     (const int32_t*)nullptr);
  AI_KERNEL_CHECK();
  AI_HIP(hipMemsetAsync(total.p, 0, 2 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(k_count_total, dim3(256), dim3(AI_BLOCK), 0, st, (const int32_t*)cnt.p, n, total.p);
  AI_KERNEL_CHECK();
  hipLaunchKernelGGL(k_count_over, dim3(256), dim3(AI_BLOCK), 0, st, (const int32_t*)cnt.p, n, AI_NB_STASH, total.p + 1);
  AI_KERNEL_CHECK();
  // the scan wraps in int32 where the group's entries pass 2^31: the 64-bit total below is looked at before anything reads it
  AI_TRY(ai_exclusive_scan_i32(st, cnt.p, rowptr.p, n, scantmp.p));
  hipLaunchKernelGGL(k_b_chunk_entries, dim3((unsigned)((nc + 1 + AI_BLOCK - 1) / AI_BLOCK)), dim3(AI_BLOCK), 0, st, (const int32_t*)rowptr.p,
                     (const int32_t*)rows.p, nc, ebase.p);
  AI_KERNEL_CHECK();
  std::vector<int32_t> hebase((size_t)nc + 1);
  unsigned long long tot2[2] = {0, 0};
  AI_HIP(hipMemcpyAsync(hebase.data(), ebase.p, hebase.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipMemcpyAsync(tot2, total.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  const unsigned long long nnz64 = tot2[0], rows_over = tot2[1];
  if (nnz64 >= (1ull << 31)) {
    if (nc > 1) return AB_SPLIT;
    ai_set_error("ai_affinity_build_batch: chunk %d: the radius graph has %llu entries; this build indexes entries with int32 (< 2^31)", lo,
                 nnz64);
    return AI_ERR_BAD_ARG;
  }
  for (int c = 0; c < nc; ++c)
    if (hebase[c + 1] - hebase[c] < hrows[c + 1] - hrows[c]) {
      ai_set_error("ai_affinity_build_batch: internal error, chunk %d has fewer entries than points (every point is its own neighbour)", lo + c);
      return AI_ERR_INTERNAL;
    }

  // ---- the graphs of the group's chunks (from here on a failure leaves them to the caller of this function, who frees B.made)
  std::vector<BOut>& houts = B.houts;
  houts.assign((size_t)nc, BOut{});
  for (int c = 0; c < nc; ++c) {
    const int64_t cn = hrows[c + 1] - hrows[c], cnnz = hebase[c + 1] - hebase[c];
    ai_csr* A = new ai_csr();
    A->n = cn;
    A->nnz = cnnz;
    A->rowptr = nullptr;
    A->col = nullptr;
    A->val = nullptr;
    A->orig = nullptr;
    A->device = ctx->device;
    ai_register_graph(ctx, A);
    B.made.push_back(A);
    AI_HIP(ctx->graphs.alloc((void**)&A->orig, (size_t)cn * sizeof(int32_t)));
    AI_HIP(ctx->graphs.alloc((void**)&A->rowptr, (size_t)(cn + 1) * sizeof(int32_t)));
    AI_HIP(ctx->graphs.alloc((void**)&A->xyz, (size_t)cn * 3 * sizeof(double)));
    AI_HIP(ctx->graphs.alloc((void**)&A->col, (size_t)cnnz * sizeof(int32_t)));
    AI_HIP(ctx->graphs.alloc((void**)&A->val, (size_t)cnnz * sizeof(double)));
    houts[c] = BOut{A->rowptr, A->col, A->val, A->orig, A->xyz};
  }
  DevBuf<BOut> outs;
  DevBuf<int32_t> col;
  DevBuf<double> val;
  DevBuf<uint8_t> notarl;
  AI_TRY(outs.alloc((size_t)nc));
  AI_TRY(col.alloc((size_t)nnz64));
  AI_TRY(val.alloc((size_t)nnz64));
  AI_HIP(hipMemcpyAsync(outs.p, houts.data(), houts.size() * sizeof(BOut), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_nb_unstash, dim3(gnb), dim3(AI_BLOCK), 0, st, (const int32_t*)cnt.p, (const int32_t*)rowptr.p, (const int32_t*)stash_col.p,
                     (const double*)stash_dist.p, AI_NB_STASH, n, col.p, val.p);
  AI_KERNEL_CHECK();
  if (rows_over > 0) {
    hipLaunchKernelGGL(k_b_neighbours<true>, dim3(gnb), dim3(AI_BLOCK), 0, st, X.p, Y.p, Z.p, cellid.p, rchunk.p, grids.p, cstart.p, cend.p, n,
                       B.radius, (int32_t*)nullptr, (const int32_t*)rowptr.p, col.p, val.p, (int32_t*)nullptr, (double*)nullptr, AI_NB_STASH,
                       (const int32_t*)cnt.p);
    AI_KERNEL_CHECK();
  }
  if (d_tarl) {
    AI_TRY(notarl.alloc(n));
    const unsigned gz = (unsigned)((n * 16 + AI_BLOCK - 1) / AI_BLOCK);
    hipLaunchKernelGGL(k_zero_rows, dim3(gz), dim3(AI_BLOCK), 0, st, d_tarl, tdim, (const int32_t*)orig.p, n, notarl.p);
    AI_KERNEL_CHECK();
  }
  launch_weights(st, rowptr.p, col.p, val.p, orig.p, n, d_tarl, tdim, notarl.p, d_dino, ddim, B.alpha, B.theta, B.gamma, nullptr, 0, 0.0);
  AI_KERNEL_CHECK();
  hipLaunchKernelGGL(k_b_split_rows, dim3(gb), dim3(AI_BLOCK), 0, st, (const int32_t*)rowptr.p, (const int32_t*)orig.p, d_xyz,
                     (const int32_t*)rchunk.p, (const int32_t*)rows.p, n, (const BOut*)outs.p);
  AI_KERNEL_CHECK();
  hipLaunchKernelGGL(k_b_split_entries, dim3(gnb), dim3(AI_BLOCK), 0, st, (const int32_t*)rowptr.p, (const int32_t*)col.p, (const double*)val.p,
                     (const int32_t*)rchunk.p, (const int32_t*)rows.p, n, (const BOut*)outs.p);
  AI_KERNEL_CHECK();
  AI_HIP(hipStreamSynchronize(st));  // the group's workspace is free for the next group; the tables uploaded above have been read
  return AI_OK;
}

extern "C" int ai_affinity_build_batch(ai_ctx* ctx, const double* xyz, const int64_t* off, int32_t n_chunks, const double* tarl,
                                       int32_t tarl_dim, const double* dino, int32_t dino_dim, double alpha, double theta, double gamma,
                                       double radius, int64_t group_rows, int mem_kind, ai_csr** out) {
  if (out && n_chunks > 0)
    for (int32_t c = 0; c < n_chunks; ++c) out[c] = nullptr;
  if (!ctx || !xyz || !off || !out || n_chunks <= 0 || !(radius > 0.0)) {
    ai_set_error("ai_affinity_build_batch: bad argument (ctx/xyz/off/out null, n_chunks <= 0 or radius <= 0)");
    return AI_ERR_BAD_ARG;
  }
  if (off[0] != 0) {
    ai_set_error("ai_affinity_build_batch: off[0] = %lld, the offsets start at 0", (long long)off[0]);
    return AI_ERR_BAD_ARG;
  }
  for (int32_t c = 0; c < n_chunks; ++c) {
    const int64_t cn = off[c + 1] - off[c];
    if (cn <= 0) {
      ai_set_error(cn < 0 ? "ai_affinity_build_batch: chunk %d: the offsets decrease" : "ai_affinity_build_batch: chunk %d is empty", c);
      return AI_ERR_BAD_ARG;
    }
    if (cn >= (int64_t)1 << 30) {
      ai_set_error("ai_affinity_build_batch: chunk %d: n = %lld exceeds the int32 row-id range of this build", c, (long long)cn);
      return AI_ERR_BAD_ARG;
    }
  }
  if (gamma != 0.0 && (dino == nullptr || dino_dim <= 0)) {
    ai_set_error("ai_affinity_build_batch: gamma != 0 needs DINO features (the reference raises ValueError here)");
    return AI_ERR_BAD_ARG;
  }
  if (theta != 0.0 && (tarl == nullptr || tarl_dim <= 0)) {
    ai_set_error("ai_affinity_build_batch: theta != 0 needs TARL features");
    return AI_ERR_BAD_ARG;
  }
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  BatchCall B{ctx, xyz, tarl, dino, off, theta != 0.0 ? tarl_dim : 0, gamma != 0.0 ? dino_dim : 0, alpha, theta, gamma, radius, mem_kind, out, {}, {}, {}, {}};
  const std::vector<int32_t> cut =
      affinity_groups(off, n_chunks, group_rows > 0 ? group_rows : AB_DEFAULT_GROUP_ROWS, std::max(B.tarl_dim, B.dino_dim));
  // groups in order; one that reports AB_SPLIT is redone as its two halves (lower half first)
  std::vector<std::pair<int32_t, int32_t>> todo;
  for (size_t g = cut.size() - 1; g > 0; --g) todo.push_back({cut[g - 1], cut[g]});
  int status = AI_OK;
  while (!todo.empty() && status == AI_OK) {
    const std::pair<int32_t, int32_t> g = todo.back();
    todo.pop_back();
    status = affinity_build_group(B, g.first, g.second);
    if (status == AB_SPLIT) {
      const int32_t mid = g.first + (g.second - g.first) / 2;
      todo.push_back({mid, g.second});
      todo.push_back({g.first, mid});
      status = AI_OK;
    }
  }
  if (status != AI_OK) {
    (void)hipStreamSynchronize(ctx->stream);  // nothing of the failed group is in flight on buffers about to be released
    for (ai_csr* A : B.made) ai_csr_free(ctx, A);
    return status;
  }
  for (int32_t c = 0; c < n_chunks; ++c) out[c] = B.made[c];
  return AI_OK;
}
