// ai_ncut / ai_ncut_batch: the recursive normalized cut of the shipped library (replaces pipeline/ncuts/normalized_cut.py:1-63).
// ai_ncut_tree / ai_ncut_tree_batch: the same calls, which also return what the recursion knows about every smaller threshold (the
// height of every group boundary and the cost of the cut every group was refused).
// This unit is everything those calls execute: the asynchronous frontier (class Flow in ai_flow.inc, the fk_* kernels in
// ai_flow_kernels.inc) and the few helpers it has in common with the level-synchronous Solver (ai_ncut_shared.h).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <deque>
#include <map>

#include <rocprim/device/device_radix_sort.hpp>

#include "ai_common.h"

#include "ai_dense_sym.h"
#include "ai_flow_host.h"
#include "ai_ncut_params.h"
#include "ai_ncut_shared.h"
#include "ai_tridiag.h"

namespace {
#include "ai_flow_kernels.inc"
#include "ai_flow.inc"
// dst[i] = src[i] + add (src == nullptr: dst[i] = i + add): concatenation of several CSR graphs
__global__ __launch_bounds__(AI_BLOCK) void k_offset_copy(int32_t* __restrict__ dst, const int32_t* __restrict__ src, int64_t n,
                                                          int32_t add) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < n) dst[i] = (src ? src[i] : (int32_t)i) + add;
}
}  // namespace

#ifdef AI_WITH_LOCKSTEP  // defined in ai_solver.hip; internal to the library: neither exported nor in include/autoinst_hip.h
__attribute__((visibility("hidden"))) int ncut_lockstep(ai_ctx* ctx, const ai_csr* csr, int nchunks, const int64_t* off, const int64_t* n_orig, double T,
                                                        double split_lim, const ai_ncut_opts* opts, int32_t* const* labels_out, int32_t* n_groups,
                                                        ai_ncut_stats* stats_out, double t0);
#endif

// The shipped library has ONE recursion driver, the asynchronous frontier (ai_flow.inc).  The level-synchronous driver of rounds
// 1-2 (ncut_lockstep in ai_solver.hip: the same per-segment arithmetic, one recursion depth at a time) is compiled only into the test-only
// build libautoinst_hip_lockstep.so (-DAI_WITH_LOCKSTEP), where AI_NCUT_LOCKSTEP=1 selects it: tests/test_gpu_parity.py and
// tests/tools/fuzz_drivers.py load that build to check that both drivers give identical labels.
static int ncut_impl(ai_ctx* ctx, const ai_csr* csr, int nchunks, const int64_t* off, const int64_t* n_orig, double T, double split_lim,
                     const ai_ncut_opts* opts, int32_t* const* labels_out, int32_t* n_groups, ai_ncut_stats* stats_out, double t0,
                     double* const* cut_height, double* const* leaf_cost) {
  static const int lockstep = getenv("AI_NCUT_LOCKSTEP") ? atoi(getenv("AI_NCUT_LOCKSTEP")) : 0;
  if (lockstep && cut_height) {
    ai_set_error("AI_NCUT_LOCKSTEP=1: the level-synchronous driver does not record the cut tree");
    return AI_ERR_BAD_ARG;
  }
#ifdef AI_WITH_LOCKSTEP
  if (lockstep) return ncut_lockstep(ctx, csr, nchunks, off, n_orig, T, split_lim, opts, labels_out, n_groups, stats_out, t0);
#else
  if (lockstep) {
    ai_set_error("AI_NCUT_LOCKSTEP=1: this build has no level-synchronous driver (load libautoinst_hip_lockstep.so: make -C autoinst_amd/csrc lockstep)");
    return AI_ERR_BAD_ARG;
  }
#endif
  return ncut_flow(ctx, csr, nchunks, off, n_orig, T, split_lim, opts, labels_out, n_groups, stats_out, t0, cut_height, leaf_cost);
}

extern "C" int ai_ncut(ai_ctx* ctx, const ai_csr* csr, int64_t num_points_orig, double T, double split_lim, const ai_ncut_opts* opts,
                       int32_t* labels_out, int32_t* n_groups, ai_ncut_stats* stats_out) {
  if (!ctx || !csr || !labels_out || !n_groups || num_points_orig < 0) {
    ai_set_error("ai_ncut: bad argument");
    return AI_ERR_BAD_ARG;
  }
  AI_CHECK_GRAPH(csr, "ai_ncut");
  // one chunk = a batch of one: the recursion keeps its even depths in a call-owned copy of the graph
  const ai_csr* graphs[1] = {csr};
  int32_t* lab[1] = {labels_out};
  return ai_ncut_batch(ctx, graphs, 1, &num_points_orig, T, split_lim, opts, lab, n_groups, stats_out);
}

// the batched cut; cut_height / leaf_cost: per chunk, where the cut tree goes (both null: the plain cut; leaf_cost alone may be null)
static int ncut_batch(ai_ctx* ctx, const ai_csr* const* graphs, int32_t count, const int64_t* num_points_orig, double T, double split_lim,
                      const ai_ncut_opts* opts, int32_t* const* labels_out, int32_t* n_groups, ai_ncut_stats* stats_out,
                      double* const* cut_height, double* const* leaf_cost) {
  int64_t N = 0, E = 0;
  for (int c = 0; c < count; ++c) {
    if (!graphs[c] || !labels_out[c] || num_points_orig[c] < 0 || (cut_height && !cut_height[c])) {
      ai_set_error("ai_ncut_batch: null graph / label buffer at position %d", c);
      return AI_ERR_BAD_ARG;
    }
    AI_CHECK_GRAPH(graphs[c], "ai_ncut_batch");
    N += graphs[c]->n;
    E += graphs[c]->nnz;
  }
  if (N >= ((int64_t)1 << 30) || E >= ((int64_t)1 << 31)) {
    ai_set_error("ai_ncut_batch: %lld rows / %lld entries exceed the int32 index range of this build", (long long)N, (long long)E);
    return AI_ERR_BAD_ARG;
  }
  AI_HIP(hipSetDevice(ctx->device));
  const double t0 = now_ms();
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  // The frontier's compact order starts with the rows of the chunks that can be split at all (normalized_cut.py:39-40);
  // chunks that cannot (n <= 2 or below split_lim) are placed behind them, whatever their position in the call.
  std::vector<int> order;
  for (int pass = 0; pass < 2; ++pass)
    for (int c = 0; c < count; ++c)
      if (eligible((int)graphs[c]->n, num_points_orig[c], split_lim) == (pass == 0)) order.push_back(c);
  std::vector<int64_t> norig_p(count);
  std::vector<int32_t*> labels_p(count);
  std::vector<double*> height_p(count, nullptr), cost_p(count, nullptr);
  std::vector<int32_t> ngroups_p(count, 0);
  // one block-diagonal graph: the chunks back to back (column ids shifted by the chunk's first row)
  DevBuf<int32_t> rp, cl, og;
  DevBuf<double> vl;
  AI_TRY(rp.alloc((size_t)N + 1));
  AI_TRY(cl.alloc((size_t)E));
  AI_TRY(vl.alloc((size_t)E));
  AI_TRY(og.alloc((size_t)N));
  std::vector<int64_t> off(count + 1, 0);
  std::vector<const double*> chunk_xyz(count);
  int64_t eoff = 0;
  for (int c = 0; c < count; ++c) {
    const ai_csr* g = graphs[order[c]];
    chunk_xyz[c] = g->xyz;
    norig_p[c] = num_points_orig[order[c]];
    labels_p[c] = labels_out[order[c]];
    if (cut_height) height_p[c] = cut_height[order[c]];
    if (leaf_cost) cost_p[c] = leaf_cost[order[c]];
    const int64_t n = g->n, e = g->nnz;
    off[c + 1] = off[c] + n;
    hipLaunchKernelGGL(k_offset_copy, dim3((unsigned)((n + 1 + AI_BLOCK - 1) / AI_BLOCK)), dim3(AI_BLOCK), 0, st, rp.p + off[c],
                       (const int32_t*)g->rowptr, n + 1, (int32_t)eoff);
    AI_KERNEL_CHECK();
    if (e) {
      hipLaunchKernelGGL(k_offset_copy, dim3((unsigned)((e + AI_BLOCK - 1) / AI_BLOCK)), dim3(AI_BLOCK), 0, st, cl.p + eoff, (const int32_t*)g->col,
                         e, (int32_t)off[c]);
      AI_KERNEL_CHECK();
      AI_HIP(hipMemcpyAsync(vl.p + eoff, g->val, (size_t)e * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    hipLaunchKernelGGL(k_offset_copy, dim3((unsigned)((n + AI_BLOCK - 1) / AI_BLOCK)), dim3(AI_BLOCK), 0, st, og.p + off[c],
                       (const int32_t*)g->orig, n, 0);
    AI_KERNEL_CHECK();
    eoff += e;
  }
  ai_csr merged;
  merged.n = N;
  merged.nnz = E;
  merged.rowptr = rp.p;
  merged.col = cl.p;
  merged.val = vl.p;
  merged.orig = og.p;
  merged.device = ctx->device;
  merged.chunk_xyz = chunk_xyz.data();
  const int rc = ncut_impl(ctx, &merged, count, off.data(), norig_p.data(), T, split_lim, opts, labels_p.data(), ngroups_p.data(), stats_out, t0,
                           cut_height ? height_p.data() : nullptr, leaf_cost ? cost_p.data() : nullptr);
  for (int c = 0; c < count; ++c) n_groups[order[c]] = ngroups_p[c];
  return rc;
}

extern "C" int ai_ncut_batch(ai_ctx* ctx, const ai_csr* const* graphs, int32_t count, const int64_t* num_points_orig, double T,
                             double split_lim, const ai_ncut_opts* opts, int32_t* const* labels_out, int32_t* n_groups,
                             ai_ncut_stats* stats_out) {
  if (!ctx || !graphs || count < 1 || !num_points_orig || !labels_out || !n_groups) {
    ai_set_error("ai_ncut_batch: bad argument");
    return AI_ERR_BAD_ARG;
  }
  return ncut_batch(ctx, graphs, count, num_points_orig, T, split_lim, opts, labels_out, n_groups, stats_out, nullptr, nullptr);
}

extern "C" int ai_ncut_tree(ai_ctx* ctx, const ai_csr* csr, int64_t num_points_orig, double T_max, double split_lim, const ai_ncut_opts* opts,
                            int32_t* labels_out, int32_t* n_groups, double* cut_height, double* leaf_cost, ai_ncut_stats* stats_out) {
  if (!ctx || !csr || !labels_out || !n_groups || !cut_height || num_points_orig < 0) {
    ai_set_error("ai_ncut_tree: bad argument");
    return AI_ERR_BAD_ARG;
  }
  AI_CHECK_GRAPH(csr, "ai_ncut_tree");
  const ai_csr* graphs[1] = {csr};
  int32_t* lab[1] = {labels_out};
  double* hgt[1] = {cut_height};
  double* cst[1] = {leaf_cost};
  return ncut_batch(ctx, graphs, 1, &num_points_orig, T_max, split_lim, opts, lab, n_groups, stats_out, hgt, leaf_cost ? cst : nullptr);
}

extern "C" int ai_ncut_tree_batch(ai_ctx* ctx, const ai_csr* const* graphs, int32_t count, const int64_t* num_points_orig, double T_max,
                                  double split_lim, const ai_ncut_opts* opts, int32_t* const* labels_out, int32_t* n_groups,
                                  double* const* cut_height, double* const* leaf_cost, ai_ncut_stats* stats_out) {
  if (!ctx || !graphs || count < 1 || !num_points_orig || !labels_out || !n_groups || !cut_height) {
    ai_set_error("ai_ncut_tree_batch: bad argument");
    return AI_ERR_BAD_ARG;
  }
  return ncut_batch(ctx, graphs, count, num_points_orig, T_max, split_lim, opts, labels_out, n_groups, stats_out, cut_height, leaf_cost);
}
