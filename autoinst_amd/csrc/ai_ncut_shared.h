// What the two solvers of the recursive normalized cut have in common: the asynchronous frontier that ai_ncut runs
// (ai_ncut.hip: ai_flow_kernels.inc, ai_flow.inc) and the level-synchronous Solver behind the diagnostic entry points,
// ai_eigs_smallest and the test-only lock-step driver (ai_solver.hip: ai_ncut_kernels.inc, ai_ncut_solver.inc).
// CONTRACT: both units form these values with these very instructions, and the labels ai_ncut ships depend on them bit for
// bit (the parity tests compare the two drivers label for label; mm_thresholds exists because ONE fused multiply-add moved a
// threshold off np.linspace's).  Whatever only one of the solvers uses stays in that solver's own files.
#pragma once
#include <chrono>

#include "ai_common.h"

namespace {

// A task = one block's contiguous row range inside ONE segment: {lo, hi, segment, first task of its segment}.
typedef int4 Task;

static double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

static bool eligible(int n, int64_t n_orig, double split_lim) {
  // normalized_cut.py:39-40: W.shape[0] > 2 and len(labels) / (num_points_orig + 1e-8) > split_lim
  return n > 2 && ((double)n / ((double)n_orig + 1e-8)) > split_lim;
}

// fixed-order sum of part[t0..t1) by one block; every thread returns the same value
__device__ __forceinline__ double ai_range_sum(const double* __restrict__ part, int t0, int t1, double* sm) {
  double a = 0.0;
  for (int t = t0 + threadIdx.x; t < t1; t += AI_BLOCK) a += part[t];
  return ai_block_sum(a, sm);
}

// Union-find with the smaller root as representative, so a component's label is its first row
// and labels do not depend on scheduling.  Plain loads may be stale inside a launch (a CU's L1 is
// not refreshed by other CUs' stores); that is harmless here: every value ever stored in
// parent[x] is an ancestor of x with a smaller-or-equal id, and hooking is decided by an
// agent-scope compare-and-swap whose failure returns the up-to-date parent.
__device__ __forceinline__ int32_t uf_find(int32_t* parent, int32_t x) {
  int32_t p = parent[x];
  while (p != x) {
    const int32_t gp = parent[p];
    if (gp != p) parent[x] = gp;  // path halving (benign race)
    x = p;
    p = gp;
  }
  return x;
}
__device__ __forceinline__ void uf_unite(int32_t* parent, int32_t a, int32_t b) {
  for (int guard = 0; guard < (1 << 22); ++guard) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int32_t t = a;
      a = b;
      b = t;
    }
    const int32_t old = atomicCAS(&parent[a], a, b);  // hook the larger (apparent) root under the smaller id
    if (old == a) return;
    a = old;  // a was no longer a root: continue from its true parent
  }
}

// staged-gather encoding of a task (k_lz_encode / fk_encode)
#define AI_ENC_MAXNNZ 4096  // entries of a task the encoder sorts in LDS
#define AI_ENC_XCAP 1024    // distinct columns of a task staged in LDS (8 KB)
struct TaskEnc {
  int32_t uoff, ucnt;  // slice of the ucol pool; ucnt < 0: not encoded, the task gathers from global memory
};

// span[0] = earliest block start, span[1] = latest block end of one launch (profiling only)
__global__ __launch_bounds__(AI_BLOCK) void k_ts_reduce(const unsigned long long* __restrict__ ts, int nblk, unsigned long long* __restrict__ span) {
  __shared__ unsigned long long smn[AI_BLOCK], smx[AI_BLOCK];
  unsigned long long mn = ~0ull, mx = 0ull;
  for (int b = threadIdx.x; b < nblk; b += AI_BLOCK) {
    mn = min(mn, ts[2 * b]);
    mx = max(mx, ts[2 * b + 1]);
  }
  smn[threadIdx.x] = mn;
  smx[threadIdx.x] = mx;
  __syncthreads();
  for (int o = AI_BLOCK / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      smn[threadIdx.x] = min(smn[threadIdx.x], smn[threadIdx.x + o]);
      smx[threadIdx.x] = max(smx[threadIdx.x], smx[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    span[0] = smn[0];
    span[1] = smx[0];
  }
}

// Number of eigenvalues of T_m (diag a[0..m), squared off-diagonals bb[1..m), both in LDS) that
// are < x, by sign changes of the leading principal minors p_i = det(T_i - x I), rescaled by
// powers of two.  The LDS reads do not depend on the recurrence, so they pipeline.
// `used`: compiled for ANY caller.  With fk_check as its only caller in a unit the compiler carries that caller's 1 <= m <= 64 into
// this function before it inlines it and fk_check comes out with other compares than beside k_lz_check; a used function keeps
// arguments of unknown range, so both units get the code they had when the two checks shared one unit.
__attribute__((used)) __device__ __forceinline__ int sturm_lt(const double* a, const double* bb, int m, double x) {
  // one wave per SIMD: the recurrence is bound by instruction issue, so magnitudes are looked at every
  // 8 rows only (|a - x| + b^2 < 4: eight rows move them by < 2^16; the rescale leaves 200 decades)
  double pm = 1.0, p = a[0] - x;
  int cnt = (p < 0.0) ? 1 : 0;
  for (int i0 = 1; i0 < m; i0 += 8) {
    double av[8], bv[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int i = min(i0 + t, m - 1);
      av[t] = a[i];
      bv[t] = bb[i];
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      if (i0 + t < m) {
        double pn = (av[t] - x) * p - bv[t] * pm;
        if (pn == 0.0) pn = (p > 0.0) ? -1e-300 : 1e-300;  // a zero takes the sign opposite to its predecessor
        cnt += ((pn < 0.0) != (p < 0.0)) ? 1 : 0;
        pm = p;
        p = pn;
      }
    }
    const double ap = fabs(p);
    if (ap > 1e100 || ap < 1e-100) {
      const double sc = (ap > 1e100) ? 0x1p-400 : 0x1p400;
      p *= sc;
      pm *= sc;
    }
  }
  return cnt;
}

// threads of a convergence-check block (k_lz_check / fk_check): one Sturm count each
#define AI_CHECK_THREADS 256

struct MinMaxPart {
  double mn, mx, sumsq, amax;
  int32_t amax_id;   // original id of the entry of largest magnitude (smallest id on ties)
  int32_t amax_neg;  // that entry is negative
};

__device__ __forceinline__ void mm_merge(MinMaxPart& r, const MinMaxPart& q) {
  r.mn = fmin(r.mn, q.mn);
  r.mx = fmax(r.mx, q.mx);
  r.sumsq += q.sumsq;
  if (q.amax > r.amax || (q.amax == r.amax && q.amax_id < r.amax_id)) {
    r.amax = q.amax;
    r.amax_id = q.amax_id;
    r.amax_neg = q.amax_neg;
  }
}

// np.allclose(mn, mx) and thr[k] = np.linspace(mn, mx, 10, endpoint=False)[k] (normalized_cut.py:27): k * step + mn with TWO roundings,
// as numpy forms it.  HIP's __dmul_rn / __dadd_rn are plain * and +, which the default -ffp-contract=fast fuses into one fma: up to
// 1 ulp off numpy's thresholds (tests/test_gpu_flow_values.py compares them bit for bit).  No contraction in this function.
__device__ __forceinline__ int32_t mm_thresholds(double mn, double mx, double* __restrict__ thr) {
#pragma clang fp contract(off)
  const double step = (mx - mn) / 10.0;
  for (int k = 0; k < AI_NUM_CUTS; ++k) thr[k] = (double)k * step + mn;
  return (fabs(mn - mx) <= 1e-8 + 1e-5 * fabs(mx)) ? 1 : 0;
}

// task stripes that k_sweep_final / fk_sweep_final sum a partial column over before adding them in stripe order
#define SWF_STRIPES 6

}  // namespace
