// ai_affinity_build_batch: the affinity graphs of many chunks in one call (DESIGN.md section 24).  Included at the end of
// ai_affinity.hip, whose radius-graph pipeline (RadiusGraph, with the grid kernels on GroupGrids) and weights (launch_weights) it
// runs on the rows of a whole GROUP of chunks.  What is here is what only a group has: the per-chunk bounds that report a
// coordinate that is not finite, the grouping, and the split of the group's graph into one graph per chunk.
//
// A group lives in one position space: row p of the group is a row of exactly one chunk, chunk c owning the positions
// rows[c] .. rows[c + 1], which are also its rows of the caller's concatenated input counted from the group's first row.  Every
// chunk has its own grid (BGrid); a stable sort on (chunk, Morton key) leaves each chunk's rows in the single build's order
// inside its own range; columns are group positions until k_b_split_* writes each chunk's CSR with local ids.
namespace {

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
#define AB_MAX_GROUP_CHUNKS 65535  // chunks of one group: k_b_bounds has one grid row (blockIdx.y) per chunk

// The chunks lo .. hi of the call in groups of whole chunks: at most `budget` rows each (a larger chunk is a group of its own),
// at most AB_MAX_GROUP_CHUNKS chunks, and a group of several chunks stays inside what its int32 position space and the tiled
// weights' 32-bit staging offsets hold (fewer than 2^30 rows, rows x widest feature < 2^33), so that its weights path is the one
// every chunk of it takes alone.
static std::vector<int32_t> affinity_groups(const int64_t* off, int32_t n_chunks, int64_t budget, int64_t widest) {
  std::vector<int32_t> cut(1, 0);
  const int64_t cap = std::min(AI_MAX_ROWS, widest > 0 ? (((int64_t)1 << 33) + widest - 1) / widest : AI_MAX_ROWS);
  const int64_t lim = std::min(budget, cap - 1);
  for (int32_t c = 0; c < n_chunks; ++c)
    if (c > cut.back() && (off[c + 1] - off[cut.back()] > lim || c - cut.back() >= AB_MAX_GROUP_CHUNKS)) cut.push_back(c);
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
  // tables a group uploads (they outlive the group's function: a failed group's copies may still be in flight when it returns)
  std::vector<int32_t> hrows;
  std::vector<BGrid> hgrid;
  std::vector<BOut> houts;
  GraphOwner owner;  // the graphs of the groups so far, in chunk order (last member: it waits for the stream before the tables go)
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
  const double *d_xyz = nullptr, *d_tarl = nullptr, *d_dino = nullptr;
  const int32_t tdim = B.tarl_dim, ddim = B.dino_dim;
  AI_TRY(to_device(B.xyz + row0 * 3, (size_t)n * 3, B.mem_kind, own_xyz, &d_xyz, st));
  if (B.theta != 0.0) AI_TRY(to_device(B.tarl + row0 * tdim, (size_t)n * (size_t)tdim, B.mem_kind, own_tarl, &d_tarl, st));
  if (B.gamma != 0.0) AI_TRY(to_device(B.dino + row0 * ddim, (size_t)n * (size_t)ddim, B.mem_kind, own_dino, &d_dino, st));

  // ---- bounds of every chunk: one launch, one host round trip for the group
  std::vector<int32_t>& hrows = B.hrows;
  hrows.assign((size_t)nc + 1, 0);
  int64_t longest = 0;
  for (int c = 0; c <= nc; ++c) hrows[c] = (int32_t)(B.off[lo + c] - row0);
  for (int c = 0; c < nc; ++c) longest = std::max<int64_t>(longest, hrows[c + 1] - hrows[c]);
  const int S = (int)std::min<int64_t>(256, std::max<int64_t>(1, (longest + 16 * AI_BLOCK - 1) / (16 * AI_BLOCK)));
  DevBuf<int32_t> rows;
  DevBuf<double> part;
  AI_TRY(upload(hrows, rows, st));
  AI_TRY(part.alloc((size_t)nc * S * AB_PART));
  hipLaunchKernelGGL(k_b_bounds, dim3(S, nc), dim3(AI_BLOCK), 0, st, d_xyz, (const int32_t*)rows.p, part.p);
  AI_KERNEL_CHECK();
  std::vector<double> hpart((size_t)nc * S * AB_PART);
  AI_HIP(hipMemcpyAsync(hpart.data(), part.p, hpart.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  std::vector<BGrid>& hgrid = B.hgrid;
  hgrid.assign((size_t)nc, BGrid{});
  int64_t ncell = 0;
  for (int c = 0; c < nc; ++c) {
    const double* r = &hpart[(size_t)c * S * AB_PART];
    double mn[3], mx[3], ext[3];
    fold_bounds(r, S, AB_PART, mn, mx);
    bool bad = false;
    for (int s = 0; s < S; ++s) bad = bad || r[s * AB_PART + 6] != 0.0;
    int64_t cells = 0;
    const int why = bad ? 1 : affinity_grid(mn, mx, B.radius, hgrid[c].g, cells, ext);
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
    hgrid[c].cell0 = ncell;
    ncell += cells;
  }
  // the cell tables of a group stay within what ONE chunk may ask for, so a call never needs more than its loop
  if (nc > 1 && ncell > ((int64_t)1 << 28)) return AB_SPLIT;

  // ---- the radius graph of the group in its own buffers; the first entry of every chunk comes down with the totals
  DevBuf<BGrid> grids;
  DevBuf<int32_t> orig, rchunk, rowptr, ebase;
  AI_TRY(upload(hgrid, grids, st));
  AI_TRY(orig.alloc(n));
  AI_TRY(rchunk.alloc(n));
  AI_TRY(rowptr.alloc(n + 1));
  AI_TRY(ebase.alloc((size_t)nc + 1));
  RadiusGraph<GroupGrids> R(st, GroupGrids{rows.p, nc, grids.p, rchunk.p}, n, ncell, B.radius);
  AI_TRY(R.count(d_xyz, orig.p, rowptr.p));
  hipLaunchKernelGGL(k_b_chunk_entries, dim3(grid_for(nc + 1)), dim3(AI_BLOCK), 0, st, (const int32_t*)rowptr.p, (const int32_t*)rows.p, nc,
                     ebase.p);
  AI_KERNEL_CHECK();
  std::vector<int32_t> hebase((size_t)nc + 1);
  AI_HIP(hipMemcpyAsync(hebase.data(), ebase.p, hebase.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_TRY(R.totals());
  if (nnz_overflows(R.nnz)) {
    if (nc > 1) return AB_SPLIT;
    ai_set_error("ai_affinity_build_batch: chunk %d: the radius graph has %llu entries; this build indexes entries with int32 (< 2^31)", lo,
                 R.nnz);
    return AI_ERR_BAD_ARG;
  }
  for (int c = 0; c < nc; ++c)
    if (nnz_below_rows(hebase[c + 1] - hebase[c], hrows[c + 1] - hrows[c])) {
      ai_set_error("ai_affinity_build_batch: internal error, chunk %d has fewer entries than points (every point is its own neighbour)", lo + c);
      return AI_ERR_INTERNAL;
    }

  // ---- the graphs of the group's chunks
  std::vector<BOut>& houts = B.houts;
  houts.assign((size_t)nc, BOut{});
  for (int c = 0; c < nc; ++c) {
    const int64_t cn = hrows[c + 1] - hrows[c], cnnz = hebase[c + 1] - hebase[c];
    ai_csr* A = B.owner.add(cn, cnnz);
    AI_HIP(B.owner.alloc(&A->orig, (size_t)cn));
    AI_HIP(B.owner.alloc(&A->rowptr, (size_t)cn + 1));
    AI_HIP(B.owner.alloc(&A->xyz, (size_t)cn * 3));
    AI_HIP(B.owner.alloc(&A->col, (size_t)cnnz));
    AI_HIP(B.owner.alloc(&A->val, (size_t)cnnz));
    houts[c] = BOut{A->rowptr, A->col, A->val, A->orig, A->xyz};
  }
  DevBuf<BOut> outs;
  DevBuf<int32_t> col;
  DevBuf<double> val;
  DevBuf<uint8_t> notarl;
  AI_TRY(upload(houts, outs, st));
  AI_TRY(col.alloc((size_t)R.nnz));
  AI_TRY(val.alloc((size_t)R.nnz));
  AI_TRY(R.fill(rowptr.p, col.p, val.p));
  AI_TRY(launch_weights(st, rowptr.p, col.p, val.p, orig.p, n, d_tarl, tdim, d_dino, ddim, B.alpha, B.theta, B.gamma, nullptr, 0, 0.0, notarl));
  const unsigned gb = grid_for(n), gnb = grid_for(n * AI_NB_LANES);
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
  static const char* const entry = "ai_affinity_build_batch";
  if (out && n_chunks > 0)
    for (int32_t c = 0; c < n_chunks; ++c) out[c] = nullptr;
  if (!ctx || !xyz || !off || !out || n_chunks <= 0 || !(radius > 0.0))
    return bad_arg(entry, "bad argument (ctx/xyz/off/out null, n_chunks <= 0 or radius <= 0)");
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
    if (cn >= AI_MAX_ROWS) {
      ai_set_error("ai_affinity_build_batch: chunk %d: n = %lld exceeds the int32 row-id range of this build", c, (long long)cn);
      return AI_ERR_BAD_ARG;
    }
  }
  AI_TRY(check_features(entry, gamma, dino, dino_dim, theta, tarl, tarl_dim));
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  BatchCall B{ctx, xyz, tarl, dino, off, theta != 0.0 ? tarl_dim : 0, gamma != 0.0 ? dino_dim : 0, alpha, theta, gamma, radius, mem_kind,
              {}, {}, {}, GraphOwner(ctx)};
  const std::vector<int32_t> cut =
      affinity_groups(off, n_chunks, group_rows > 0 ? group_rows : AB_DEFAULT_GROUP_ROWS, std::max(B.tarl_dim, B.dino_dim));
  // groups in order; one that reports AB_SPLIT is redone as its two halves (lower half first)
  std::vector<std::pair<int32_t, int32_t>> todo;
  for (size_t g = cut.size() - 1; g > 0; --g) todo.push_back({cut[g - 1], cut[g]});
  while (!todo.empty()) {
    const std::pair<int32_t, int32_t> g = todo.back();
    todo.pop_back();
    const int status = affinity_build_group(B, g.first, g.second);
    if (status == AB_SPLIT) {
      const int32_t mid = g.first + (g.second - g.first) / 2;
      todo.push_back({mid, g.second});
      todo.push_back({g.first, mid});
    } else if (status != AI_OK) {
      return status;  // B.owner frees what the groups so far have made
    }
  }
  B.owner.keep(out);
  return AI_OK;
}
