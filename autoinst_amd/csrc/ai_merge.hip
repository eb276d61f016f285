// The step that turns the chunks into the map, for all chunks of a map in one resident call:
// merge_chunks_unite_instances2 (pipeline/utils/point_cloud/point_cloud_utils.py:387-491) with the instance id as the identity.
//
//   ai_merge_map -- rules M1-M10 of include/autoinst_hip.h.  The concatenated points stay where they are; one int32 array holds the
//                   global id of every point and is filled chunk by chunk.  The duplicate flags (M2) are computed once for the
//                   whole map (three stable 64-bit radix passes, as ai_unique_points).  A step crops the map before its chunk,
//                   ranks the instances present in the crop densely, and forms the (map instance x local instance) tables of
//                   ai_merge_associate over those ranks only; the association (M8-M9) is one more kernel.  Per step three counts
//                   cross to the host (selected points, instances in the crop, distinct scalar entries): three synchronisations.
#include <cmath>

#include "ai_labels_shared.h"

namespace {

struct MCube {
  double lo[3], hi[3];
};

// blocks per chunk of the centre reduction (M4): ai_chunk_finish's RED_BLOCKS, F4's order
#define MM_RED_BLOCKS 256
// boxes per LDS tile of kg_inside
#define MM_BOX_TILE 256
// three (value, tag) entries per selected point are ranked by an int32 scan over ns + 1 positions
#define MM_MAX_SCALARS 2147483646
// entries of one (map instance in the crop) x (local id) table
#define MM_MAX_TABLE 268435456
// chunks per launch of the centre reduction (MM_RED_BLOCKS * 3 partial sums each)
#define MM_CENTER_BATCH 4096

// M1 / M10: the largest local id of every chunk; the first chunk with a non-finite coordinate (bad[0]) or a negative id (bad[1]).
// A wave whose 64 points lie in one chunk (nearly all do) reduces its ids first and sends one atomic: 2 M points of 72 chunks
// would otherwise queue at 72 words.
__global__ __launch_bounds__(AI_BLOCK) void kg_validate(const double* __restrict__ xyz, const int32_t* __restrict__ inst, int64_t m,
                                                        const int64_t* __restrict__ off, int32_t n_chunks, int32_t* __restrict__ nloc,
                                                        int32_t* __restrict__ bad) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const bool valid = i < m;
  int32_t c = -1, l = 0;
  if (valid) {
    c = segment_of(off, n_chunks, i);
    const double x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) atomicMin(&bad[0], c);
    l = inst[i];
    if (l < 0) atomicMin(&bad[1], c);
  }
  const int32_t c0 = __shfl(c, 0, 64);
  if (__all(c == c0)) {  // wave-uniform: every lane takes this branch
    int32_t w = l;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) w = max(w, __shfl_xor(w, o, 64));
    if ((threadIdx.x & 63) == 0 && w > 0) atomicMax(&nloc[c0], w);
  } else if (l > 0) {
    atomicMax(&nloc[c], l);
  }
}

__global__ __launch_bounds__(AI_BLOCK) void kg_fill(int32_t* __restrict__ a, int64_t n, int32_t v) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < n) a[i] = v;
}

// M4, F4's order: thread t of block b adds the chunk-local rows b * 256 + t, + 65536, ... in ascending order
__global__ __launch_bounds__(AI_BLOCK) void kg_center_partial(const double* __restrict__ xyz, const int64_t* __restrict__ off, int32_t c0,
                                                              double* __restrict__ part) {
  __shared__ double sm[3][AI_BLOCK / 64];
  const int32_t ch = c0 + blockIdx.y;
  const int64_t base = off[ch], n = off[ch + 1] - base;
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x; i < n; i += (int64_t)MM_RED_BLOCKS * AI_BLOCK) {
#pragma unroll
    for (int a = 0; a < 3; ++a) s[a] += xyz[(base + i) * 3 + a];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double t = ai_block_sum_first(s[a], sm[a]);
    if (threadIdx.x == 0) part[((int64_t)blockIdx.y * MM_RED_BLOCKS + blockIdx.x) * 3 + a] = t;
  }
}

// the 256 block sums of a chunk summed the same way, then one division by the count (0 / 0 = NaN for an empty chunk: skipped)
__global__ __launch_bounds__(AI_BLOCK) void kg_center_finish(const double* __restrict__ part, const int64_t* __restrict__ off, int32_t c0,
                                                             double* __restrict__ center) {
  __shared__ double sm[3][AI_BLOCK / 64];
  const int32_t ch = c0 + blockIdx.x;
  const double n = (double)(off[ch + 1] - off[ch]);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double t = ai_block_sum_first(part[((int64_t)blockIdx.x * MM_RED_BLOCKS + threadIdx.x) * 3 + a], sm[a]);
    if (threadIdx.x == 0) center[(int64_t)ch * 3 + a] = t / n;
  }
}

// the global id a chunk's step gave its points: table[l] for l > 0 (table = the chunk's slice of the id table), 0 stays 0
__global__ __launch_bounds__(AI_BLOCK) void kg_relabel(const int32_t* __restrict__ inst, int64_t n, const int32_t* __restrict__ table,
                                                       int32_t* __restrict__ gid) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t l = inst[i];
  gid[i] = l > 0 ? table[l] : 0;
}

// M3 + M5: map points before the chunk that carry an instance, are kept (every point of chunk 0 at step 1) and lie in the cube
__global__ __launch_bounds__(AI_BLOCK) void kg_crop(const double* __restrict__ xyz, const int32_t* __restrict__ gid,
                                                    const int32_t* __restrict__ keep, int64_t n, MCube c, int use_keep,
                                                    int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  int32_t f = 0;
  if (gid[i] > 0 && (!use_keep || keep[i])) {
    const double x = xyz[i * 3], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
    f = (x >= c.lo[0] && x <= c.hi[0] && y >= c.lo[1] && y <= c.hi[1] && z >= c.lo[2] && z <= c.hi[2]) ? 1 : 0;
  }
  flag[i] = f;
}

__global__ __launch_bounds__(AI_BLOCK) void kg_inst_flag(const int32_t* __restrict__ inst, int64_t n, int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < n) flag[i] = inst[i] > 0 ? 1 : 0;
}

// the global ids of the cropped points, compacted (sorted next: their distinct values are the instances present in the crop)
// and their positions: the kernels behind this one run over the cropped points alone, not over the map
__global__ __launch_bounds__(AI_BLOCK) void kg_gather_ids(const int32_t* __restrict__ gid, const int32_t* __restrict__ pos, int64_t n,
                                                          uint32_t* __restrict__ out, int32_t* __restrict__ where) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (pos[i + 1] != pos[i]) {
    out[pos[i]] = (uint32_t)gid[i];
    where[pos[i]] = (int32_t)i;
  }
}

// rank r of the crop = the r-th smallest global id present: dense and order-preserving
__global__ __launch_bounds__(AI_BLOCK) void kg_emit_ids(const uint32_t* __restrict__ key, const int32_t* __restrict__ pos, int64_t n,
                                                        int32_t* __restrict__ glist) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (pos[i + 1] != pos[i]) glist[pos[i]] = (int32_t)key[i];
}

// cropped map points (j-th at row where[j]) -> three (value, rank) entries each, and the box of their rank (min / max of
// order-preserving integers: exact and order-independent).  A block takes MM_SCALAR_TILE points and, while the boxes of the crop
// fit (n1 <= MM_LDS_BOXES), gathers them in LDS first: all points of a crop otherwise queue at the few words of its few boxes.
#define MM_LDS_BOXES 512
#define MM_SCALAR_TILE 1024
__global__ __launch_bounds__(AI_BLOCK) void kg_scalars_map(const double* __restrict__ xyz, const int32_t* __restrict__ gid,
                                                           const int32_t* __restrict__ where, int64_t n_sel,
                                                           const int32_t* __restrict__ glist, int32_t n1, uint64_t* __restrict__ val,
                                                           uint32_t* __restrict__ tag, unsigned long long* __restrict__ box) {
  __shared__ unsigned long long sbox[MM_LDS_BOXES * 6];
  const bool in_lds = n1 <= MM_LDS_BOXES;
  if (in_lds) {
    for (int q = threadIdx.x; q < n1 * 6; q += AI_BLOCK) sbox[q] = (q % 6 < 3) ? ~0ull : 0ull;
    __syncthreads();
  }
  for (int t = 0; t < MM_SCALAR_TILE / AI_BLOCK; ++t) {
    const int64_t j = (int64_t)blockIdx.x * MM_SCALAR_TILE + (int64_t)t * AI_BLOCK + threadIdx.x;
    if (j >= n_sel) continue;
    const int64_t i = where[j];
    const int32_t g = gid[i];
    int32_t lo = 0, hi = n1 - 1;  // g is in glist: glist[lo] <= g <= glist[hi]
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (glist[mid] < g) lo = mid + 1; else hi = mid;
    }
    const int64_t o = j * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const unsigned long long k = ordered_bits(xyz[i * 3 + a]);
      val[o + a] = k;
      tag[o + a] = (uint32_t)lo;
      if (in_lds) {
        atomicMin(&sbox[lo * 6 + a], k);
        atomicMax(&sbox[lo * 6 + 3 + a], k);
      } else {
        // a bound only moves outwards: a point inside the (possibly stale) box cannot move it and skips the atomics
        unsigned long long* bmin = &box[(size_t)lo * 6 + a];
        unsigned long long* bmax = &box[(size_t)lo * 6 + 3 + a];
        if (k < ai_ld_agent(bmin)) atomicMin(bmin, k);
        if (k > ai_ld_agent(bmax)) atomicMax(bmax, k);
      }
    }
  }
  if (in_lds) {
    __syncthreads();
    for (int q = threadIdx.x; q < n1 * 6; q += AI_BLOCK) {
      const unsigned long long v = sbox[q];
      if (q % 6 < 3) {
        if (v != ~0ull) atomicMin(&box[q], v);
      } else if (v != 0ull) {
        atomicMax(&box[q], v);
      }
    }
  }
}

// chunk points of a local instance -> three (value, side 1 | local id) entries each, behind the map's
__global__ __launch_bounds__(AI_BLOCK) void kg_scalars_chunk(const double* __restrict__ xyz, const int32_t* __restrict__ inst,
                                                             const int32_t* __restrict__ pos, int64_t n, int64_t base,
                                                             uint64_t* __restrict__ val, uint32_t* __restrict__ tag) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (pos[i + 1] == pos[i]) return;
  const int64_t o = (base + pos[i]) * 3;
  const uint32_t t = 0x80000000u | (uint32_t)inst[i];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    val[o + a] = ordered_bits(xyz[i * 3 + a]);
    tag[o + a] = t;
  }
}

// distinct (value, tag) entries, compacted; every entry counts one distinct scalar of its instance.  count = n1 counters of the
// ranks, then n2 of the local ids.  A block takes MM_DISTINCT_TILE sorted entries and counts them in LDS first when the counters
// fit (the entries are ordered by value, so a block meets every instance: straight global atomics all land on the same few words)
#define MM_HIST 2048
#define MM_DISTINCT_TILE 2048
__global__ __launch_bounds__(AI_BLOCK) void kg_distinct(const uint64_t* __restrict__ val, const uint32_t* __restrict__ tag,
                                                        const int32_t* __restrict__ pos, int64_t n, uint64_t* __restrict__ dval,
                                                        uint32_t* __restrict__ dtag, int32_t n1, int32_t n2,
                                                        int32_t* __restrict__ count) {
  __shared__ int32_t hist[MM_HIST];
  const int32_t nc = n1 + n2;
  const bool in_lds = nc <= MM_HIST;
  if (in_lds) {
    for (int q = threadIdx.x; q < nc; q += AI_BLOCK) hist[q] = 0;
    __syncthreads();
  }
  const int64_t base = (int64_t)blockIdx.x * MM_DISTINCT_TILE;
  for (int k = 0; k < MM_DISTINCT_TILE / AI_BLOCK; ++k) {
    const int64_t i = base + (int64_t)k * AI_BLOCK + threadIdx.x;
    if (i >= n || pos[i + 1] == pos[i]) continue;
    const uint32_t t = tag[i];
    dval[pos[i]] = val[i];
    dtag[pos[i]] = t;
    const int32_t slot = (t >> 31) ? n1 + (int32_t)(t & 0x7fffffffu) : (int32_t)t;
    if (in_lds)
      atomicAdd(&hist[slot], 1);
    else
      atomicAdd(&count[slot], 1);
  }
  if (in_lds) {
    __syncthreads();
    for (int q = threadIdx.x; q < nc; q += AI_BLOCK)
      if (hist[q]) atomicAdd(&count[q], hist[q]);
  }
}

// M8 inter: chunk points of local id l inside the box of rank r, boxes staged through LDS in tiles
__global__ __launch_bounds__(AI_BLOCK) void kg_inside(const double* __restrict__ xyz, const int32_t* __restrict__ inst, int64_t n,
                                                      int32_t n1, int32_t n2, const unsigned long long* __restrict__ box,
                                                      int32_t* __restrict__ inter) {
  __shared__ double sb[MM_BOX_TILE][6];
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const int32_t l = (i < n) ? inst[i] : 0;
  const bool live = l > 0 && l < n2;
  double x = 0.0, y = 0.0, z = 0.0;
  if (live) {
    x = xyz[i * 3];
    y = xyz[i * 3 + 1];
    z = xyz[i * 3 + 2];
  }
  for (int32_t b0 = 0; b0 < n1; b0 += MM_BOX_TILE) {
    const int32_t nb = min(MM_BOX_TILE, n1 - b0);
    __syncthreads();
    for (int q = threadIdx.x; q < nb * 6; q += AI_BLOCK) sb[q / 6][q % 6] = from_ordered_bits(box[(size_t)b0 * 6 + q]);
    __syncthreads();
    if (!live) continue;
    for (int32_t b = 0; b < nb; ++b)
      if (x >= sb[b][0] && x <= sb[b][3] && y >= sb[b][1] && y <= sb[b][4] && z >= sb[b][2] && z <= sb[b][5])
        atomicAdd(&inter[(size_t)(b0 + b) * n2 + l], 1);
  }
}

// M8 + M9, one thread per local id: ranks ascend with the global id, and only a strictly larger iou replaces, so among equal
// iou the smallest global id stays.  table = the chunk's slice of the id table; stat = {qualifying pairs, re-labelled ids}.
__global__ __launch_bounds__(AI_BLOCK) void kg_associate(const int32_t* __restrict__ inter, const int32_t* __restrict__ common,
                                                         const int32_t* __restrict__ ns1, const int32_t* __restrict__ ns2, int32_t n1,
                                                         int32_t n2, double iou_min, const int32_t* __restrict__ glist,
                                                         int32_t* __restrict__ table, int32_t* __restrict__ stat) {
  const int32_t l = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (l < 1 || l >= n2) return;
  double best = 0.0;
  int32_t best_r = -1, pairs = 0;
  const int64_t s2 = ns2[l];
  for (int32_t r = 0; r < n1; ++r) {
    const int32_t in = inter[(size_t)r * n2 + l];
    if (in <= 0) continue;
    const int64_t uni = (int64_t)ns1[r] + s2 - common[(size_t)r * n2 + l];
    const double iou = (double)in / (double)uni;
    if (!(iou > iou_min)) continue;
    ++pairs;
    if (best_r < 0 || iou > best) {
      best = iou;
      best_r = r;
    }
  }
  if (pairs) atomicAdd(&stat[0], pairs);
  if (best_r >= 0) {
    table[l] = glist[best_r];
    atomicAdd(&stat[1], 1);
  }
}

// the kept points in ascending position: coordinates bit for bit, the global id, the position in the concatenation
__global__ __launch_bounds__(AI_BLOCK) void kg_emit(const double* __restrict__ xyz, const int32_t* __restrict__ gid,
                                                    const int32_t* __restrict__ pos, int64_t m, double* __restrict__ out_xyz,
                                                    int32_t* __restrict__ out_inst, int64_t* __restrict__ out_src) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= m) return;
  if (pos[i + 1] == pos[i]) return;
  const int64_t o = pos[i];
  if (out_xyz) {
#pragma unroll
    for (int a = 0; a < 3; ++a) out_xyz[o * 3 + a] = xyz[i * 3 + a];
  }
  if (out_inst) out_inst[o] = gid[i];
  if (out_src) out_src[o] = i;
}

// the arena's fill level before a step; a step's buffers are handed back when it ends (everything runs on one stream, so the next
// step's kernels queue behind the last reader)
struct ArenaMark {
  ai_arena* a;
  size_t cur, off, need;
  ArenaMark() : a(ai_current_arena()) {
    if (a) cur = a->cur, off = a->off, need = a->need;
  }
  ~ArenaMark() {
    if (!a) return;
    if (a->need > a->need_max) a->need_max = a->need;
    a->cur = cur, a->off = off, a->need = need;
  }
};

}  // namespace

extern "C" int ai_merge_map(ai_ctx* ctx, const double* xyz, const int32_t* inst, const int64_t* off, int32_t n_chunks,
                            const double* centers, double side_length, double iou_min, int mem_kind, double* out_xyz,
                            int32_t* out_inst, int64_t* out_src, int64_t* n_out, int32_t* inst_table, int64_t* stats,
                            double* centers_used) {
  if (!ctx) {
    ai_set_error("ai_merge_map: no context");
    return AI_ERR_BAD_ARG;
  }
  if (!n_out) {
    ai_set_error("ai_merge_map: n_out is NULL, and the other outputs cannot be returned without it");
    return AI_ERR_BAD_ARG;
  }
  *n_out = 0;
  if (n_chunks < 0 || n_chunks > 65535) {
    ai_set_error("ai_merge_map: n_chunks = %d is outside 0 .. 65535", n_chunks);
    return AI_ERR_BAD_ARG;
  }
  if (!(side_length > 0.0) || !std::isfinite(side_length)) {
    ai_set_error("ai_merge_map: side_length must be positive and finite");
    return AI_ERR_BAD_ARG;
  }
  if (!std::isfinite(iou_min)) {
    ai_set_error("ai_merge_map: iou_min is not finite");
    return AI_ERR_BAD_ARG;
  }
  if (n_chunks == 0) {
    if (inst_table) inst_table[0] = 0;
    return AI_OK;
  }
  if (!off) {
    ai_set_error("ai_merge_map: off is NULL");
    return AI_ERR_BAD_ARG;
  }
  if (off[0] != 0) {
    ai_set_error("ai_merge_map: the offsets do not start at 0 (chunk 0 starts at %lld)", (long long)off[0]);
    return AI_ERR_BAD_ARG;
  }
  for (int32_t c = 0; c < n_chunks; ++c)
    if (off[c + 1] < off[c]) {
      ai_set_error("ai_merge_map: the offsets decrease at chunk %d (%lld after %lld)", c, (long long)off[c + 1], (long long)off[c]);
      return AI_ERR_BAD_ARG;
    }
  const int64_t m = off[n_chunks];
  if (m >= ((int64_t)1 << 30)) {
    ai_set_error("ai_merge_map: %lld points, the limit is 2^30 - 1", (long long)m);
    return AI_ERR_BAD_ARG;
  }
  if (centers)
    for (int32_t c = 0; c < n_chunks; ++c)
      for (int a = 0; a < 3; ++a)
        if (!std::isfinite(centers[(size_t)c * 3 + a])) {
          ai_set_error("ai_merge_map: the centre of chunk %d is not finite", c);
          return AI_ERR_BAD_ARG;
        }
  if (stats) memset(stats, 0, (size_t)n_chunks * 4 * sizeof(int64_t));
  if (m == 0) {
    if (inst_table) inst_table[0] = 0;
    if (centers_used)
      for (size_t k = 0; k < (size_t)n_chunks * 3; ++k) centers_used[k] = centers ? centers[k] : std::nan("");
    return AI_OK;
  }
  if (!xyz || !inst) {
    ai_set_error("ai_merge_map: xyz or inst is NULL");
    return AI_ERR_BAD_ARG;
  }
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<double> own_x, d_center, d_part;
  DevBuf<int32_t> own_i, d_nloc, d_bad, gid, keep, kpos, pos1, pos2, scan_tmp, table, d_stat;
  DevBuf<int64_t> d_off;
  const double* dx;
  const int32_t* di;
  AI_TRY(to_device(xyz, (size_t)m * 3, mem_kind, own_x, &dx, st));
  AI_TRY(to_device(inst, (size_t)m, mem_kind, own_i, &di, st));
  AI_TRY(d_off.alloc((size_t)n_chunks + 1));
  AI_TRY(d_nloc.alloc(n_chunks));
  AI_TRY(d_bad.alloc(2));
  AI_HIP(hipMemcpyAsync(d_off.p, off, ((size_t)n_chunks + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
  AI_HIP(hipMemsetAsync(d_nloc.p, 0, (size_t)n_chunks * sizeof(int32_t), st));
  AI_HIP(hipMemsetAsync(d_bad.p, 0x7f, 2 * sizeof(int32_t), st));
  hipLaunchKernelGGL(kg_validate, dim3(grid_for(m)), dim3(AI_BLOCK), 0, st, dx, di, m, (const int64_t*)d_off.p, n_chunks, d_nloc.p, d_bad.p);
  AI_KERNEL_CHECK();
  // M4: the centres of all chunks, one fixed reduction shape per chunk
  std::vector<double> h_center((size_t)n_chunks * 3);
  if (centers) {
    memcpy(h_center.data(), centers, h_center.size() * sizeof(double));
  } else {
    const int32_t batch = std::min<int32_t>(n_chunks, MM_CENTER_BATCH);
    AI_TRY(d_center.alloc((size_t)n_chunks * 3));
    AI_TRY(d_part.alloc((size_t)batch * MM_RED_BLOCKS * 3));
    for (int32_t c0 = 0; c0 < n_chunks; c0 += batch) {
      const int32_t nb = std::min<int32_t>(batch, n_chunks - c0);
      hipLaunchKernelGGL(kg_center_partial, dim3(MM_RED_BLOCKS, nb), dim3(AI_BLOCK), 0, st, dx, (const int64_t*)d_off.p, c0, d_part.p);
      hipLaunchKernelGGL(kg_center_finish, dim3(nb), dim3(AI_BLOCK), 0, st, (const double*)d_part.p, (const int64_t*)d_off.p, c0, d_center.p);
      AI_KERNEL_CHECK();
    }
    AI_HIP(hipMemcpyAsync(h_center.data(), d_center.p, h_center.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  std::vector<int32_t> nloc(n_chunks);
  int32_t bad[2];
  AI_HIP(hipMemcpyAsync(nloc.data(), d_nloc.p, (size_t)n_chunks * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipMemcpyAsync(bad, d_bad.p, sizeof(bad), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  if (bad[0] < n_chunks) {
    ai_set_error("ai_merge_map: chunk %d has a coordinate that is not finite", bad[0]);
    return AI_ERR_BAD_ARG;
  }
  if (bad[1] < n_chunks) {
    ai_set_error("ai_merge_map: chunk %d has a negative local instance id", bad[1]);
    return AI_ERR_BAD_ARG;
  }
  // M1: provisional global id of local id l of chunk c = goff[c] + l
  std::vector<int64_t> goff((size_t)n_chunks + 1, 0);
  for (int32_t c = 0; c < n_chunks; ++c) {
    goff[c + 1] = goff[c] + nloc[c];
    if (goff[c + 1] >= 2147483647ll) {
      ai_set_error("ai_merge_map: the local ids up to chunk %d give %lld global ids, the limit is 2^31 - 2", c, (long long)goff[c + 1]);
      return AI_ERR_BAD_ARG;
    }
  }
  const int64_t n_ids = goff[n_chunks] + 1;
  int64_t max_n = 0;
  for (int32_t c = 0; c < n_chunks; ++c) max_n = std::max(max_n, off[c + 1] - off[c]);
  AI_TRY(gid.alloc(m));
  AI_TRY(keep.alloc(m + 1));
  AI_TRY(kpos.alloc(m + 1));
  AI_TRY(pos1.alloc(m + 1));
  AI_TRY(pos2.alloc(max_n + 1));
  AI_TRY(scan_tmp.alloc(ai_scan_tmp_elems(m)));
  AI_TRY(table.alloc(n_ids));
  AI_TRY(d_stat.alloc((size_t)n_chunks * 2));
  AI_HIP(hipMemsetAsync(d_stat.p, 0, (size_t)n_chunks * 2 * sizeof(int32_t), st));
  hipLaunchKernelGGL(ku_iota, dim3(grid_for(n_ids)), dim3(AI_BLOCK), 0, st, table.p, n_ids);
  AI_KERNEL_CHECK();
  // M2 once for the whole map: first occurrences after three stable passes (z, y, x); one chunk keeps everything
  if (n_chunks == 1) {
    hipLaunchKernelGGL(kg_fill, dim3(grid_for(m)), dim3(AI_BLOCK), 0, st, keep.p, m, 1);
    AI_KERNEL_CHECK();
  } else {
    ArenaMark mark;
    DevBuf<uint64_t> key, skey;
    DevBuf<int32_t> oa, ob;
    AI_TRY(key.alloc(m));
    AI_TRY(skey.alloc(m));
    AI_TRY(oa.alloc(m));
    AI_TRY(ob.alloc(m));
    hipLaunchKernelGGL(ku_iota, dim3(grid_for(m)), dim3(AI_BLOCK), 0, st, oa.p, m);
    AI_KERNEL_CHECK();
    int32_t *cur = oa.p, *nxt = ob.p;
    for (int axis = 2; axis >= 0; --axis) {
      hipLaunchKernelGGL(ku_axis_keys, dim3(grid_for(m)), dim3(AI_BLOCK), 0, st, dx, (const int32_t*)cur, m, axis, key.p);
      AI_KERNEL_CHECK();
      AI_TRY(sort_pairs(st, key.p, skey.p, cur, nxt, m, 64));
      std::swap(cur, nxt);
    }
    hipLaunchKernelGGL(ku_first_flags, dim3(grid_for(m)), dim3(AI_BLOCK), 0, st, dx, (const int32_t*)cur, m, keep.p);
    AI_KERNEL_CHECK();
  }
  AI_HIP(hipMemcpyAsync(kpos.p, keep.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  AI_TRY(ai_exclusive_scan_i32(st, kpos.p, kpos.p, m, scan_tmp.p));
  int32_t total = 0;
  AI_HIP(hipMemcpyAsync(&total, kpos.p + m, sizeof(int32_t), hipMemcpyDeviceToHost, st));

  const double half = side_length / 2.0;
  for (int32_t c = 0; c < n_chunks; ++c) {
    const int64_t a = off[c], n = off[c + 1] - a;
    if (n == 0) continue;  // M3: an empty chunk associates nothing and adds nothing
    const int32_t n2 = nloc[c] + 1;
    int32_t* tab = table.p + goff[c];  // tab[l] = global id of local id l (tab[0] belongs to the chunk before and is not touched)
    int32_t sel[2] = {0, 0};
    if (c >= 1 && a > 0 && n2 > 1) {
      ArenaMark mark;
      MCube cube;
      for (int k = 0; k < 3; ++k) {  // M5: the bounds as written
        cube.lo[k] = h_center[(size_t)c * 3 + k] - half;
        cube.hi[k] = h_center[(size_t)c * 3 + k] + half;
      }
      hipLaunchKernelGGL(kg_crop, dim3(grid_for(a)), dim3(AI_BLOCK), 0, st, dx, (const int32_t*)gid.p, (const int32_t*)keep.p, a, cube,
                         c == 1 ? 0 : 1, pos1.p);
      hipLaunchKernelGGL(kg_inst_flag, dim3(grid_for(n)), dim3(AI_BLOCK), 0, st, di + a, n, pos2.p);
      AI_KERNEL_CHECK();
      AI_TRY(ai_exclusive_scan_i32(st, pos1.p, pos1.p, a, scan_tmp.p));
      AI_TRY(ai_exclusive_scan_i32(st, pos2.p, pos2.p, n, scan_tmp.p));
      AI_HIP(hipMemcpyAsync(&sel[0], pos1.p + a, sizeof(int32_t), hipMemcpyDeviceToHost, st));
      AI_HIP(hipMemcpyAsync(&sel[1], pos2.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
      AI_HIP(hipStreamSynchronize(st));
      if (stats) stats[(size_t)c * 4] = sel[0];
      const int64_t ns = 3 * ((int64_t)sel[0] + sel[1]);
      if (ns > MM_MAX_SCALARS) {
        ai_set_error("ai_merge_map: chunk %d: %d cropped map points + %d chunk points of instances give %lld coordinate scalars, "
                     "more than the %lld that int32 positions can index",
                     c, sel[0], sel[1], (long long)ns, (long long)MM_MAX_SCALARS);
        return AI_ERR_BAD_ARG;
      }
      if (sel[0] > 0 && sel[1] > 0) {
        // the instances present in the crop, ranked densely in ascending id order
        DevBuf<uint32_t> ids, sids;
        DevBuf<int32_t> head, glist, where;
        DevBuf<uint8_t> tmp;
        AI_TRY(ids.alloc(sel[0]));
        AI_TRY(where.alloc(sel[0]));
        AI_TRY(sids.alloc(sel[0]));
        AI_TRY(head.alloc((size_t)sel[0] + 1));
        hipLaunchKernelGGL(kg_gather_ids, dim3(grid_for(a)), dim3(AI_BLOCK), 0, st, (const int32_t*)gid.p, (const int32_t*)pos1.p, a, ids.p,
                           where.p);
        AI_KERNEL_CHECK();
        size_t tmp_bytes = 0;
        AI_HIP(rocprim::radix_sort_keys(nullptr, tmp_bytes, ids.p, sids.p, (size_t)sel[0], 0, 32, st));
        AI_TRY(tmp.alloc(tmp_bytes));
        AI_HIP(rocprim::radix_sort_keys(tmp.p, tmp_bytes, ids.p, sids.p, (size_t)sel[0], 0, 32, st));
        hipLaunchKernelGGL(kl_heads<uint32_t>, dim3(grid_for(sel[0])), dim3(AI_BLOCK), 0, st, (const uint32_t*)sids.p, (int64_t)sel[0], head.p);
        AI_KERNEL_CHECK();
        AI_TRY(ai_exclusive_scan_i32(st, head.p, head.p, sel[0], scan_tmp.p));
        int32_t n1 = 0;
        AI_HIP(hipMemcpyAsync(&n1, head.p + sel[0], sizeof(int32_t), hipMemcpyDeviceToHost, st));
        AI_HIP(hipStreamSynchronize(st));
        if (stats) stats[(size_t)c * 4 + 1] = n1;
        if ((int64_t)n1 * n2 >= MM_MAX_TABLE) {
          ai_set_error("ai_merge_map: chunk %d: %d map instances in the crop x %d local ids need a table of 2^28 entries or more", c, n1,
                       n2);
          return AI_ERR_BAD_ARG;
        }
        AI_TRY(glist.alloc(n1));
        hipLaunchKernelGGL(kg_emit_ids, dim3(grid_for(sel[0])), dim3(AI_BLOCK), 0, st, (const uint32_t*)sids.p, (const int32_t*)head.p,
                           (int64_t)sel[0], glist.p);
        AI_KERNEL_CHECK();
        // the tables of ai_merge_associate over (rank, local id)
        const size_t n12 = (size_t)n1 * n2;
        DevBuf<int32_t> tables, shead;
        DevBuf<unsigned long long> box;
        DevBuf<uint64_t> val, val2, dval;
        DevBuf<uint32_t> tag, tag2, dtag;
        AI_TRY(tables.alloc(2 * n12 + n1 + n2));
        int32_t *d_inter = tables.p, *d_common = tables.p + n12, *d_ns1 = tables.p + 2 * n12, *d_ns2 = d_ns1 + n1;
        AI_HIP(hipMemsetAsync(tables.p, 0, (2 * n12 + n1 + n2) * sizeof(int32_t), st));
        AI_TRY(box.alloc((size_t)n1 * 6));
        AI_TRY(val.alloc(ns));
        AI_TRY(val2.alloc(ns));
        AI_TRY(tag.alloc(ns));
        AI_TRY(tag2.alloc(ns));
        AI_TRY(shead.alloc(ns + 1));
        hipLaunchKernelGGL(km_box_init, dim3(grid_for((int64_t)n1 * 6)), dim3(AI_BLOCK), 0, st, box.p, n1);
        hipLaunchKernelGGL(kg_scalars_map, dim3((unsigned)((sel[0] + MM_SCALAR_TILE - 1) / MM_SCALAR_TILE)), dim3(AI_BLOCK), 0, st, dx, (const int32_t*)gid.p,
                           (const int32_t*)where.p, (int64_t)sel[0], (const int32_t*)glist.p, n1, val.p, tag.p, box.p);
        hipLaunchKernelGGL(kg_scalars_chunk, dim3(grid_for(n)), dim3(AI_BLOCK), 0, st, dx + a * 3, di + a, (const int32_t*)pos2.p, n,
                           (int64_t)sel[0], val.p, tag.p);
        AI_KERNEL_CHECK();
        // order by (value, side, instance): stable sort by the tag, then by the value
        AI_TRY(sort_pairs(st, tag.p, tag2.p, val.p, val2.p, ns, 32));
        AI_TRY(sort_pairs(st, val2.p, val.p, tag2.p, tag.p, ns, 64));
        hipLaunchKernelGGL(km_val_tag_heads, dim3(grid_for(ns)), dim3(AI_BLOCK), 0, st, (const uint64_t*)val.p, (const uint32_t*)tag.p, ns,
                           shead.p);
        AI_KERNEL_CHECK();
        DevBuf<int32_t> stmp;  // ns may exceed the number of points: three entries per selected point
        AI_TRY(stmp.alloc(ai_scan_tmp_elems(ns)));
        AI_TRY(ai_exclusive_scan_i32(st, shead.p, shead.p, ns, stmp.p));
        int32_t nd = 0;
        AI_HIP(hipMemcpyAsync(&nd, shead.p + ns, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        AI_HIP(hipStreamSynchronize(st));
        AI_TRY(dval.alloc(nd));
        AI_TRY(dtag.alloc(nd));
        hipLaunchKernelGGL(kg_distinct, dim3((unsigned)((ns + MM_DISTINCT_TILE - 1) / MM_DISTINCT_TILE)), dim3(AI_BLOCK), 0, st,
                           (const uint64_t*)val.p, (const uint32_t*)tag.p, (const int32_t*)shead.p, ns, dval.p, dtag.p, n1, n2, d_ns1);
        hipLaunchKernelGGL(km_common, dim3(grid_for(nd)), dim3(AI_BLOCK), 0, st, (const uint64_t*)dval.p, (const uint32_t*)dtag.p,
                           (int64_t)nd, n2, d_common);
        hipLaunchKernelGGL(kg_inside, dim3(grid_for(n)), dim3(AI_BLOCK), 0, st, dx + a * 3, di + a, n, n1, n2,
                           (const unsigned long long*)box.p, d_inter);
        hipLaunchKernelGGL(kg_associate, dim3(grid_for(n2)), dim3(AI_BLOCK), 0, st, (const int32_t*)d_inter, (const int32_t*)d_common,
                           (const int32_t*)d_ns1, (const int32_t*)d_ns2, n1, n2, iou_min, (const int32_t*)glist.p, tab,
                           d_stat.p + (size_t)c * 2);
        AI_KERNEL_CHECK();
      }
    }
    hipLaunchKernelGGL(kg_relabel, dim3(grid_for(n)), dim3(AI_BLOCK), 0, st, di + a, n, (const int32_t*)tab, gid.p + a);
    AI_KERNEL_CHECK();
  }
  AI_HIP(hipStreamSynchronize(st));  // `total` has arrived (with one chunk, or chunks without instances, nothing waited for it yet)

  // M2: the kept points in ascending position
  if (total > 0 && (out_xyz || out_inst || out_src)) {
    DevBuf<double> t_xyz;
    DevBuf<int32_t> t_inst;
    DevBuf<int64_t> t_src;
    double* o_xyz = out_xyz;
    int32_t* o_inst = out_inst;
    int64_t* o_src = out_src;
    if (mem_kind != AI_MEM_DEVICE) {
      if (out_xyz) {
        AI_TRY(t_xyz.alloc((size_t)total * 3));
        o_xyz = t_xyz.p;
      }
      if (out_inst) {
        AI_TRY(t_inst.alloc(total));
        o_inst = t_inst.p;
      }
      if (out_src) {
        AI_TRY(t_src.alloc(total));
        o_src = t_src.p;
      }
    }
    hipLaunchKernelGGL(kg_emit, dim3(grid_for(m)), dim3(AI_BLOCK), 0, st, dx, (const int32_t*)gid.p, (const int32_t*)kpos.p, m, o_xyz, o_inst,
                       o_src);
    AI_KERNEL_CHECK();
    if (mem_kind != AI_MEM_DEVICE) {
      AI_TRY(to_caller(out_xyz, (const double*)t_xyz.p, (size_t)total * 3, mem_kind, st));
      AI_TRY(to_caller(out_inst, (const int32_t*)t_inst.p, (size_t)total, mem_kind, st));
      AI_TRY(to_caller(out_src, (const int64_t*)t_src.p, (size_t)total, mem_kind, st));
    }
  }
  std::vector<int32_t> h_stat;
  if (stats) {
    h_stat.resize((size_t)n_chunks * 2);
    AI_HIP(hipMemcpyAsync(h_stat.data(), d_stat.p, h_stat.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  }
  if (inst_table) AI_HIP(hipMemcpyAsync(inst_table, table.p, (size_t)n_ids * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  if (stats)
    for (int32_t c = 0; c < n_chunks; ++c) {
      stats[(size_t)c * 4 + 2] = h_stat[(size_t)c * 2];
      stats[(size_t)c * 4 + 3] = h_stat[(size_t)c * 2 + 1];
    }
  if (centers_used) memcpy(centers_used, h_center.data(), h_center.size() * sizeof(double));
  *n_out = total;
  return AI_OK;
}
