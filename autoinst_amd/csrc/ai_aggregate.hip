// ai_aggregate_scans: the scans of a map go to the two aggregated clouds (ground / non-ground) in one call -- the loop of
// aggregate_pointcloud (pipeline/utils/point_cloud/aggregate_pointcloud.py:99-186) with the dataset's filter chain
// (pipeline/dataset/filters/kitti_gt_mo_filter.py:40-51, range_filter.py:23-36) and the three label decodes
// (pipeline/dataset/kitti_odometry_dataset.py:73-104).  The rules (A1-A6) are in include/autoinst_hip.h and DESIGN.md section 15.
//
//   ka_count   every point's class (dropped / ground / non-ground) from its coordinates, label word and ground flag; the two
//              counts of every tile of AG_TILE consecutive points;
//   (scan)     exclusive scans of the two count arrays: where each tile's run starts in each map;
//   ka_starts  one block per scan boundary: the tile's start plus the class counts of the tile's points in front of the boundary
//              (class_off, and with the last boundary the two totals);
//   ka_write   the class again (17 bytes per point: cheaper than storing it), the rank inside the tile by wave ballots and an LDS
//              prefix over the (pass, wave) counts, the transform (A4); the tile's output rows are staged in LDS and leave as two
//              linear runs of doubles, labels and source positions as compacted 4-byte stores.
//
// A tile's points are visited in passes of AI_BLOCK consecutive points, so (pass, wave, lane) order is input order: a stable
// partition (A5).  Nothing here depends on the order in which blocks run.
#include <cmath>

#include "ai_entry.h"
#include "ai_keep.h"
#include "ai_xform.h"

namespace {

#define AG_ITEMS 4
#define AG_TILE (AI_BLOCK * AG_ITEMS)  // 1024 points per block
#define AG_WAVES (AI_BLOCK / 64)

enum { AG_DROP = 0, AG_GROUND = 1, AG_NONGROUND = 2 };

struct AGIn {
  const float* xyz;        // n x 3
  const uint32_t* word;    // n, or null
  const uint8_t* ground;   // n, or null
  int64_t n;
  AIKeep keep;             // A1 and A2 (ai_keep.h)
};

struct AGOut {  // index 0: ground, 1: non-ground; label and source outputs may be null
  double *xyz_g, *xyz_n;
  uint32_t *seg_g, *seg_n, *inst_g, *inst_n, *pan_g, *pan_n;
  int32_t *src_g, *src_n;
};

// A1-A3 for point i: its class, coordinates and label word (A1 and A2 are ai_keep_point, shared with ai_ground_planes).
__device__ __forceinline__ int ag_classify(const AGIn& a, int64_t i, float& x, float& y, float& z, uint32_t& w) {
  x = a.xyz[i * 3];
  y = a.xyz[i * 3 + 1];
  z = a.xyz[i * 3 + 2];
  w = a.word ? a.word[i] : 0u;
  if (!ai_keep_point(a.keep, x, y, z, w)) return AG_DROP;
  return (a.ground && a.ground[i]) ? AG_GROUND : AG_NONGROUND;
}

// the class counts of the points [first, last) (at most AG_TILE of them), for thread 0 of the block
__device__ __forceinline__ void ag_block_counts(const AGIn& a, int64_t first, int64_t last, int32_t (*wc)[AG_WAVES], int32_t& g, int32_t& n) {
  int32_t cg = 0, cn = 0;
#pragma unroll
  for (int j = 0; j < AG_ITEMS; ++j) {
    const int64_t i = first + (int64_t)j * AI_BLOCK + threadIdx.x;
    float x, y, z;
    uint32_t w;
    const int c = i < last ? ag_classify(a, i, x, y, z, w) : AG_DROP;
    cg += __popcll(__ballot(c == AG_GROUND));
    cn += __popcll(__ballot(c == AG_NONGROUND));
  }
  if ((threadIdx.x & 63) == 0) {
    wc[0][threadIdx.x >> 6] = cg;
    wc[1][threadIdx.x >> 6] = cn;
  }
  __syncthreads();
  g = 0, n = 0;
#pragma unroll
  for (int k = 0; k < AG_WAVES; ++k) {
    g += wc[0][k];
    n += wc[1][k];
  }
}

__global__ __launch_bounds__(AI_BLOCK) void ka_count(AGIn a, int32_t* __restrict__ cnt_g, int32_t* __restrict__ cnt_n) {
  __shared__ int32_t wc[2][AG_WAVES];
  const int64_t first = (int64_t)blockIdx.x * AG_TILE;
  int32_t g, n;
  ag_block_counts(a, first, min(first + AG_TILE, a.n), wc, g, n);
  if (threadIdx.x == 0) {
    cnt_g[blockIdx.x] = g;
    cnt_n[blockIdx.x] = n;
  }
}

// block s: class_off[c][s] = kept points of class c in front of input position scan_off[s] = the start of that position's tile
// (base[tile], with base[number of tiles] = the total) + the tile's points in front of it.  n_bound = n_scans + 1.
__global__ __launch_bounds__(AI_BLOCK) void ka_starts(AGIn a, const int64_t* __restrict__ scan_off, int32_t n_bound,
                                                      const int32_t* __restrict__ base_g, const int32_t* __restrict__ base_n,
                                                      int64_t* __restrict__ class_off) {
  __shared__ int32_t wc[2][AG_WAVES];
  const int64_t p = scan_off[blockIdx.x];
  const int64_t tile = p / AG_TILE;
  int32_t g, n;
  ag_block_counts(a, tile * AG_TILE, p, wc, g, n);
  if (threadIdx.x == 0) {
    class_off[blockIdx.x] = (int64_t)base_g[tile] + g;
    class_off[n_bound + blockIdx.x] = (int64_t)base_n[tile] + n;
  }
}

__global__ __launch_bounds__(AI_BLOCK) void ka_write(AGIn a, const int64_t* __restrict__ scan_off, int32_t n_scans,
                                                     const double* __restrict__ T, const int32_t* __restrict__ base_g,
                                                     const int32_t* __restrict__ base_n, AGOut o) {
  __shared__ double stage[AG_TILE * 3];  // the tile's output rows: ground first, then non-ground
  __shared__ int32_t wc[2][AG_ITEMS][AG_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t first = (int64_t)blockIdx.x * AG_TILE, last = min(first + AG_TILE, a.n);
  // the scans the tile touches (the same for the whole block): a point's scan is searched for among them only
  const int32_t s_lo = segment_in(scan_off, 0, n_scans - 1, first), s_hi = segment_in(scan_off, s_lo, n_scans - 1, last - 1);
  float x[AG_ITEMS], y[AG_ITEMS], z[AG_ITEMS];
  uint32_t w[AG_ITEMS];
  int c[AG_ITEMS];
  int32_t rank[AG_ITEMS];  // among the class's points of the same pass and wave
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < AG_ITEMS; ++j) {
    const int64_t i = first + (int64_t)j * AI_BLOCK + threadIdx.x;
    c[j] = i < last ? ag_classify(a, i, x[j], y[j], z[j], w[j]) : AG_DROP;
    const unsigned long long mg = __ballot(c[j] == AG_GROUND), mn = __ballot(c[j] == AG_NONGROUND);
    rank[j] = __popcll((c[j] == AG_GROUND ? mg : mn) & below);
    if (lane == 0) {
      wc[0][j][wave] = __popcll(mg);
      wc[1][j][wave] = __popcll(mn);
    }
  }
  __syncthreads();
  int32_t pre_g[AG_ITEMS], pre_n[AG_ITEMS], tot_g = 0, tot_n = 0;  // the counts in front of (pass j, this wave); the tile's totals
#pragma unroll
  for (int j = 0; j < AG_ITEMS; ++j) {
#pragma unroll
    for (int k = 0; k < AG_WAVES; ++k) {
      if (k == wave) {
        pre_g[j] = tot_g;
        pre_n[j] = tot_n;
      }
      tot_g += wc[0][j][k];
      tot_n += wc[1][j][k];
    }
  }
  const int64_t bg = base_g[blockIdx.x], bn = base_n[blockIdx.x];
#pragma unroll
  for (int j = 0; j < AG_ITEMS; ++j) {
    if (c[j] == AG_DROP) continue;
    const int64_t i = first + (int64_t)j * AI_BLOCK + threadIdx.x;
    const bool gr = c[j] == AG_GROUND;
    const int32_t r = (gr ? pre_g[j] : pre_n[j]) + rank[j];
    const int32_t row = gr ? r : tot_g + r;  // < tot_g + tot_n <= AG_TILE
    const int64_t dst = (gr ? bg : bn) + r;
    const int32_t s = segment_in(scan_off, s_lo, s_hi, i);
    double ox, oy, oz;
    ai_xf(T + (int64_t)s * 16, (double)x[j], (double)y[j], (double)z[j], ox, oy, oz);
    stage[row * 3] = ox;
    stage[row * 3 + 1] = oy;
    stage[row * 3 + 2] = oz;
    // A6, all in uint32: the instance product wraps
    const uint32_t hi = w[j] & 0xFFFF0000u, lo = w[j] & 0xFFFFu;
    uint32_t* seg = gr ? o.seg_g : o.seg_n;
    uint32_t* inst = gr ? o.inst_g : o.inst_n;
    uint32_t* pan = gr ? o.pan_g : o.pan_n;
    int32_t* src = gr ? o.src_g : o.src_n;
    if (seg) seg[dst] = lo;
    if (inst) inst[dst] = hi * (w[j] & 0x10009u);
    if (pan) pan[dst] = hi ? hi : lo;
    if (src) src[dst] = (int32_t)i;
  }
  __syncthreads();
  double* dg = o.xyz_g + bg * 3;
  for (int32_t t = threadIdx.x; t < tot_g * 3; t += AI_BLOCK) dg[t] = stage[t];
  double* dn = o.xyz_n + bn * 3;
  const double* sn = stage + tot_g * 3;
  for (int32_t t = threadIdx.x; t < tot_n * 3; t += AI_BLOCK) dn[t] = sn[t];
}

}  // namespace

extern "C" int ai_aggregate_scans(ai_ctx* ctx, const float* scan_xyz, const int64_t* scan_off, int32_t n_scans, const double* pose,
                                  const uint32_t* label_word, const uint8_t* ground_flag, int32_t moving_index, double range_min,
                                  double range_max, int mem_kind, double* out_xyz_ground, double* out_xyz_nonground,
                                  uint32_t* out_seg_ground, uint32_t* out_seg_nonground, uint32_t* out_instance_ground,
                                  uint32_t* out_instance_nonground, uint32_t* out_panoptic_ground, uint32_t* out_panoptic_nonground,
                                  int32_t* out_src_ground, int32_t* out_src_nonground, int64_t* class_off, int64_t* n_ground,
                                  int64_t* n_nonground) {
  const auto bad = [](const char* what) { return bad_arg("ai_aggregate_scans", what); };
  if (!ctx || !scan_off || n_scans < 0 || !n_ground || !n_nonground) return bad("null pointer or negative count");
  if (mem_kind != AI_MEM_HOST && mem_kind != AI_MEM_DEVICE) return bad("mem_kind must be AI_MEM_HOST or AI_MEM_DEVICE");
  if (scan_off[0] != 0) return bad("scan_off must start at 0");
  for (int32_t s = 0; s < n_scans; ++s)
    if (scan_off[s + 1] < scan_off[s]) return bad("scan_off is not monotone");
  const int64_t M = scan_off[n_scans];
  if (M >= ((int64_t)1 << 31) - AI_BLOCK) return bad("M must be below 2^31 - 256");
  if (n_scans > 0 && !pose) return bad("null pointer");
  for (int32_t s = 0; s < n_scans; ++s) {
    const double* T = pose + (size_t)s * 16;
    for (int k = 0; k < 12; ++k)
      if (!std::isfinite(T[k])) return bad("a pose is not finite");
    if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0) return bad("the last row of a pose must be (0, 0, 0, 1)");
  }
  const bool use_moving = moving_index >= 0, use_range = !(range_max < 0.0);
  // (a null array of no points is an empty array: nothing below asks for an element of it)
  if (M > 0 && use_moving && !label_word) return bad("the moving-object filter needs label_word");
  if (use_range && !(range_min <= range_max)) return bad("range_min must not exceed range_max (and neither may be NaN)");
  const bool any_label = out_seg_ground || out_seg_nonground || out_instance_ground || out_instance_nonground || out_panoptic_ground ||
                         out_panoptic_nonground;
  if (M > 0 && !label_word && any_label) return bad("label outputs need label_word");
  if (M > 0 && (!scan_xyz || !out_xyz_ground || !out_xyz_nonground)) return bad("null pointer");

  const size_t n_bound = (size_t)n_scans + 1;
  std::vector<int64_t> coff(2 * n_bound, 0);
  if (M > 0) {
    AI_HIP(hipSetDevice(ctx->device));
    ArenaScope arena_scope(&ctx->arena);
    hipStream_t st = ctx->stream;
    DevBuf<float> own_x;
    DevBuf<uint32_t> own_w, b_seg_g, b_seg_n, b_inst_g, b_inst_n, b_pan_g, b_pan_n;
    DevBuf<uint8_t> own_f;
    DevBuf<int64_t> d_off, d_coff;
    DevBuf<double> d_T, b_xyz_g, b_xyz_n;
    DevBuf<int32_t> base_g, base_n, scan_tmp, b_src_g, b_src_n;
    AGIn in = {};
    in.n = M;
    in.keep = ai_keep_rules(moving_index, range_min, range_max);
    AI_TRY(to_device(scan_xyz, (size_t)M * 3, mem_kind, own_x, &in.xyz, st));
    if (label_word) AI_TRY(to_device(label_word, (size_t)M, mem_kind, own_w, &in.word, st));
    if (ground_flag) AI_TRY(to_device(ground_flag, (size_t)M, mem_kind, own_f, &in.ground, st));
    AI_TRY(d_off.alloc(n_bound));
    AI_TRY(d_coff.alloc(2 * n_bound));
    AI_TRY(d_T.alloc((size_t)n_scans * 16));
    AI_HIP(hipMemcpyAsync(d_off.p, scan_off, n_bound * sizeof(int64_t), hipMemcpyHostToDevice, st));
    AI_HIP(hipMemcpyAsync(d_T.p, pose, (size_t)n_scans * 16 * sizeof(double), hipMemcpyHostToDevice, st));
    const int64_t nt = (M + AG_TILE - 1) / AG_TILE;
    AI_TRY(base_g.alloc((size_t)nt + 1));
    AI_TRY(base_n.alloc((size_t)nt + 1));
    AI_TRY(scan_tmp.alloc(ai_scan_tmp_elems(nt)));
    hipLaunchKernelGGL(ka_count, dim3((unsigned)nt), dim3(AI_BLOCK), 0, st, in, base_g.p, base_n.p);
    AI_KERNEL_CHECK();
    AI_TRY(ai_exclusive_scan_i32(st, base_g.p, base_g.p, nt, scan_tmp.p));
    AI_TRY(ai_exclusive_scan_i32(st, base_n.p, base_n.p, nt, scan_tmp.p));
    hipLaunchKernelGGL(ka_starts, dim3((unsigned)n_bound), dim3(AI_BLOCK), 0, st, in, (const int64_t*)d_off.p, (int32_t)n_bound,
                       (const int32_t*)base_g.p, (const int32_t*)base_n.p, d_coff.p);
    AI_KERNEL_CHECK();
    AI_HIP(hipMemcpyAsync(coff.data(), d_coff.p, 2 * n_bound * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    AI_HIP(hipStreamSynchronize(st));
    const int64_t ng = coff[n_scans], nn = coff[n_bound + n_scans];
    AGOut o = {out_xyz_ground,      out_xyz_nonground,      out_seg_ground,      out_seg_nonground, out_instance_ground,
               out_instance_nonground, out_panoptic_ground, out_panoptic_nonground, out_src_ground,    out_src_nonground};
    if (mem_kind != AI_MEM_DEVICE) {  // the totals are known: device copies of exactly the rows that will be written
      AI_TRY(dev_out_if_wanted(out_xyz_ground, ng * 3, b_xyz_g, &o.xyz_g));
      AI_TRY(dev_out_if_wanted(out_xyz_nonground, nn * 3, b_xyz_n, &o.xyz_n));
      AI_TRY(dev_out_if_wanted(out_seg_ground, ng, b_seg_g, &o.seg_g));
      AI_TRY(dev_out_if_wanted(out_seg_nonground, nn, b_seg_n, &o.seg_n));
      AI_TRY(dev_out_if_wanted(out_instance_ground, ng, b_inst_g, &o.inst_g));
      AI_TRY(dev_out_if_wanted(out_instance_nonground, nn, b_inst_n, &o.inst_n));
      AI_TRY(dev_out_if_wanted(out_panoptic_ground, ng, b_pan_g, &o.pan_g));
      AI_TRY(dev_out_if_wanted(out_panoptic_nonground, nn, b_pan_n, &o.pan_n));
      AI_TRY(dev_out_if_wanted(out_src_ground, ng, b_src_g, &o.src_g));
      AI_TRY(dev_out_if_wanted(out_src_nonground, nn, b_src_n, &o.src_n));
    }
    hipLaunchKernelGGL(ka_write, dim3((unsigned)nt), dim3(AI_BLOCK), 0, st, in, (const int64_t*)d_off.p, n_scans, (const double*)d_T.p,
                       (const int32_t*)base_g.p, (const int32_t*)base_n.p, o);
    AI_KERNEL_CHECK();
    if (mem_kind != AI_MEM_DEVICE) {
#define AG_BACK(host, dev, count)                                                                                         \
  if ((host) && (count) > 0) AI_HIP(hipMemcpyAsync((host), (dev), (size_t)(count) * sizeof(*(host)), hipMemcpyDeviceToHost, st))
      AG_BACK(out_xyz_ground, o.xyz_g, ng * 3);
      AG_BACK(out_xyz_nonground, o.xyz_n, nn * 3);
      AG_BACK(out_seg_ground, o.seg_g, ng);
      AG_BACK(out_seg_nonground, o.seg_n, nn);
      AG_BACK(out_instance_ground, o.inst_g, ng);
      AG_BACK(out_instance_nonground, o.inst_n, nn);
      AG_BACK(out_panoptic_ground, o.pan_g, ng);
      AG_BACK(out_panoptic_nonground, o.pan_n, nn);
      AG_BACK(out_src_ground, o.src_g, ng);
      AG_BACK(out_src_nonground, o.src_n, nn);
#undef AG_BACK
    }
    AI_HIP(hipStreamSynchronize(st));
  }
  if (class_off)
    for (size_t k = 0; k < 2 * n_bound; ++k) class_off[k] = coff[k];
  *n_ground = coff[n_scans];
  *n_nonground = coff[n_bound + n_scans];
  return AI_OK;
}
