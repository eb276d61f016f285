// Tile shapes and capacities shared by the kernels and the host drivers of the recursion (ai_ncut.hip, ai_solver.hip), and the rule of
// who may be split at all.  Free of HIP: ai_flow_host.h and the host tests include it.
#pragma once
#include <stdint.h>
#ifndef AI_FINE_ROWS
#define AI_FINE_ROWS 32      // rows per block in the 16-lanes-per-row kernels (2 rows in flight per lane group; 16 / 128 measured slower, 64: 20.6 vs 17.4 us per launch on a whole 200k graph, 111 vs 121 chunks/s with the quad kernel)
#endif
#ifndef AI_COARSE_ROWS
#define AI_COARSE_ROWS 512   // rows per block in the thread-per-row kernels (256 / 1024 measured within 2 %)
#endif
#define AI_ROW_ILP (AI_FINE_ROWS / (AI_BLOCK / AI_LPR))
#define AI_SLAB_VECS 32      // Lanczos vectors per HBM slab
#define AI_ROW_PF 4         // rounds of 16 entries per row loaded together in the 16-lanes-per-row kernels
#define AI_SWEEP_VALS 40     // per-task sweep partials: cut[10], assocA[10], assocB[10], cntA[10]
#define AI_MAX_CHECKS 4096   // convergence checks per level (one counter slot each)
#define AI_FLOW_UPSLOTS 32   // pinned upload ring of the asynchronous frontier (ai_flow.inc)

namespace {
static bool eligible(int n, int64_t n_orig, double split_lim) {
  // normalized_cut.py:39-40: W.shape[0] > 2 and len(labels) / (num_points_orig + 1e-8) > split_lim
  return n > 2 && ((double)n / ((double)n_orig + 1e-8)) > split_lim;
}
}  // namespace
