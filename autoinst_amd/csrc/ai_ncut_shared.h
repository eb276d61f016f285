// What the two solvers of the recursive normalized cut have in common: the asynchronous frontier that ai_ncut runs
// (ai_ncut.hip: ai_flow_kernels.inc, ai_flow.inc) and the level-synchronous Solver behind the diagnostic entry points,
// ai_eigs_smallest and the test-only lock-step driver (ai_solver.hip: ai_ncut_kernels.inc, ai_ncut_solver.inc).
// CONTRACT: both units form these values with these very instructions, and the labels ai_ncut ships depend on them bit for
// bit (the parity tests compare the two drivers label for label; mm_thresholds exists because ONE fused multiply-add moved a
// threshold off np.linspace's).  Whatever only one of the solvers uses stays in that solver's own files.
//
// SHARED BY DEFINITION (one text, so the contract holds by construction; tests/test_ncut_bodies_once.py):
//   ai_range_sum, uf_find / uf_unite, sturm_lt, mm_merge, mm_thresholds, and the bodies of the kernels that form the degree, the
//   scaling, the min/max, the thresholds, the bins and the ten cut costs: degree_body, scale_body, minmax_body, minmax_final_body,
//   bin_body, sweep_body, sweep_final_body.  Each k_* / fk_* kernel of those keeps its name, its arguments and its launch bounds
//   in its own file and is a wrapper: its own prologue (fk_scale: gate / nbin and the volume through recs[].aux; k_minmax*: mode;
//   k_sweep_final / fk_sweep_final: what a segment that is not split stores -- NAN costs in the Solver, INFINITY and only if wanted
//   in the frontier: do not unify the two), then the body.  A body is a template over the two things that differ: how a task
//   reaches its rows, columns and weights (a graph policy: CsrGraph in ai_ncut_kernels.inc, FlowGraph in ai_flow_kernels.inc;
//   rows(tk) hands back an int2 operator()(row), col(tk) and w(tk) the pointers), and where a segment's run of partials lies (two
//   ints).  All fourteen kernels came out with the registers, LDS and floating-point instructions they had as copies (DESIGN.md
//   section 28 has the table); a pair that stops doing so goes back to two copies.
// STILL WRITTEN TWICE, on purpose -- do not "finish the job" without knowing why:
//   k_lz_encode / fk_encode: a bitonic sort against a hash table, different algorithms;
//   the cc_* kernels: the frontier has a sampling pass and record gates;
//   partition, comp_table, rebuild_*: different buffer layouts and child bookkeeping;
//   k_seg_sum / fk_seg_sum: already one call to ai_range_sum each;
//   the whole Lanczos step -- spmv_body / fk_spmv*, update_body / fk_update, k_lz_check / fk_check, k_ritz / fk_ritz, the freeze
//   helpers: the frontier's versions have diverged on purpose (argument order for kernarg preload, per-task step counts, frozen
//   segments), and a function shared across the two units can change a kernel that was not touched (see sturm_lt below).
#pragma once
#include <chrono>

#include "ai_common.h"
#include "ai_ncut_params.h"

namespace {

// A task = one block's contiguous row range inside ONE segment: {lo, hi, segment, first task of its segment}.
typedef int4 Task;

static double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
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

// ============================================================================= kernel bodies that both solvers run
// Graph: how a task reaches its rows, columns and weights (see the contract above).

// deg_i = 1 + sum_j w_ij (W = w + I, normalized_cut.py:38,42); s_i = 1 / sqrt(deg_i) (:43); pvol[block] = the task's sum of deg
template <class Graph>
__device__ __forceinline__ void degree_body(const Task tk, const Graph g, double* __restrict__ deg, double* __restrict__ sinv,
                                            double* __restrict__ pvol) {
  __shared__ double sm[AI_BLOCK / 64];
  const auto rows = g.rows(tk);
  const double* __restrict__ wraw = g.w(tk);
  const int l = threadIdx.x & (AI_LPR - 1), r = threadIdx.x / AI_LPR;
  double acc = 0.0;
  for (int row = tk.x + r; row < tk.y; row += AI_BLOCK / AI_LPR) {
    const int2 se = rows(row);
    const int p0 = se.x, p1 = se.y;
    double s = 0.0;
    {
      // the first AI_ROW_PF rounds of a row (64 entries: nearly every row) are loaded together, then added in order
      double w[AI_ROW_PF];
#pragma unroll
      for (int q = 0; q < AI_ROW_PF; ++q) {
        const int p = p0 + l + q * AI_LPR;
        w[q] = (p < p1) ? wraw[p] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < AI_ROW_PF; ++q)
        if (p0 + l + q * AI_LPR < p1) s += w[q];
    }
    for (int p = p0 + l + AI_ROW_PF * AI_LPR; p < p1; p += AI_LPR) s += wraw[p];
    s = ai_group16_sum(s);
    if (l == 0) {
      const double d = s + 1.0;
      deg[row] = d;
      sinv[row] = 1.0 / sqrt(d);
      acc += d;
    }
  }
  const double tot = ai_block_sum(acc, sm);
  if (threadIdx.x == 0) pvol[blockIdx.x] = tot;
}

// wm_ij = (s_i * w_ij) * s_j  (row scaling then column scaling, like D2 * (D - W) * D2, :47);
// sinv2_i = s_i * s_i is the "+ I" term of W; u1_i = sqrt(deg_i / v), v = the volume of the task's segment
template <class Graph>
__device__ __forceinline__ void scale_body(const Task tk, const Graph g, const double v, const double* __restrict__ deg,
                                           const double* __restrict__ sinv, double* __restrict__ wm, double* __restrict__ sinv2,
                                           double* __restrict__ u1) {
  const auto rows = g.rows(tk);
  const int32_t* __restrict__ col = g.col(tk);
  const double* __restrict__ wraw = g.w(tk);
  const int l = threadIdx.x & (AI_LPR - 1), r = threadIdx.x / AI_LPR;
  for (int row = tk.x + r; row < tk.y; row += AI_BLOCK / AI_LPR) {
    const int2 se = rows(row);
    const int p0 = se.x, p1 = se.y;
    const double si = sinv[row];
    {
      int c[AI_ROW_PF];
      double w[AI_ROW_PF], sj[AI_ROW_PF];
#pragma unroll
      for (int q = 0; q < AI_ROW_PF; ++q) {
        const int p = p0 + l + q * AI_LPR;
        const bool ok = p < p1;
        c[q] = ok ? col[p] : -1;
        w[q] = ok ? wraw[p] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < AI_ROW_PF; ++q) sj[q] = (c[q] >= 0) ? sinv[c[q]] : 0.0;
#pragma unroll
      for (int q = 0; q < AI_ROW_PF; ++q)
        if (c[q] >= 0) wm[p0 + l + q * AI_LPR] = (si * w[q]) * sj[q];
    }
    for (int p = p0 + l + AI_ROW_PF * AI_LPR; p < p1; p += AI_LPR) wm[p] = (si * wraw[p]) * sinv[col[p]];
    if (l == 0) {
      sinv2[row] = si * si;
      u1[row] = sqrt(deg[row] / v);
    }
  }
}

// part[block] = min, max, sum of squares and the entry of largest magnitude of ev over the task's rows (orig: the rows' original ids)
__device__ __forceinline__ void minmax_body(const Task tk, const double* __restrict__ ev, const int32_t* __restrict__ orig,
                                            MinMaxPart* __restrict__ part) {
  __shared__ MinMaxPart sm[AI_BLOCK / 64];
  MinMaxPart r;
  r.mn = 1e300;
  r.mx = -1e300;
  r.sumsq = 0.0;
  r.amax = -1.0;
  r.amax_id = 0x7fffffff;
  r.amax_neg = 0;
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    const double e = ev[row];
    MinMaxPart q;
    q.mn = e;
    q.mx = e;
    q.sumsq = e * e;
    q.amax = fabs(e);
    q.amax_id = orig[row];
    q.amax_neg = e < 0.0;
    mm_merge(r, q);
  }
  for (int o = 32; o > 0; o >>= 1) {
    MinMaxPart q;
    q.mn = __shfl_xor(r.mn, o, 64);
    q.mx = __shfl_xor(r.mx, o, 64);
    q.sumsq = __shfl_xor(r.sumsq, o, 64);
    q.amax = __shfl_xor(r.amax, o, 64);
    q.amax_id = __shfl_xor(r.amax_id, o, 64);
    q.amax_neg = __shfl_xor(r.amax_neg, o, 64);
    mm_merge(r, q);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[w] = r;
  __syncthreads();
  if (threadIdx.x == 0) {
    MinMaxPart t = sm[0];
    for (int i = 1; i < AI_BLOCK / 64; ++i) mm_merge(t, sm[i]);
    part[blockIdx.x] = t;
  }
}

// Segment s, partials part[t0..t1): unit norm + sign convention folded into one scale (raw: the vector is taken as it is);
// np.allclose(mn, mx) test (normalized_cut.py:22); thresholds t_k = k * step + mn, step = (mx - mn) / 10, exactly as
// np.linspace(mn, mx, 10, endpoint=False) computes them (:28).
__device__ __forceinline__ void minmax_final_body(const MinMaxPart* __restrict__ part, int t0, int t1, int raw, int s,
                                                  double* __restrict__ scale, int32_t* __restrict__ nosplit, double* __restrict__ thr) {
  MinMaxPart r = part[t0];
  for (int t = t0 + 1; t < t1; ++t) mm_merge(r, part[t]);
  double sc = 1.0;
  if (!raw) {
    const double nrm = sqrt(r.sumsq);
    sc = (nrm > 0.0) ? 1.0 / nrm : 1.0;
    if (r.amax_neg) sc = -sc;
  }
  const double mn = (sc > 0.0) ? r.mn * sc : r.mx * sc;
  const double mx = (sc > 0.0) ? r.mx * sc : r.mn * sc;
  scale[s] = sc;
  nosplit[s] = mm_thresholds(mn, mx, thr + s * AI_NUM_CUTS);
}

// bin_i = number of thresholds strictly below ev_i: mask_k(i) = (ev_i > t_k) = (k < bin_i)
__device__ __forceinline__ void bin_body(const Task* __restrict__ ctasks, const int32_t* __restrict__ nosplit,
                                         const double* __restrict__ scale, const double* __restrict__ thr,
                                         const double* __restrict__ ev, uint8_t* __restrict__ bin) {
  const Task tk = ctasks[blockIdx.x];
  const int s = tk.z;
  if (nosplit[s]) return;  // no threshold will be applied to this segment (the split flags look at split[] first)
  const double sc = scale[s];
  double th[AI_NUM_CUTS];
#pragma unroll
  for (int k = 0; k < AI_NUM_CUTS; ++k) th[k] = thr[s * AI_NUM_CUTS + k];
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    const double e = ev[row] * sc;
    int b = 0;
#pragma unroll
    for (int k = 0; k < AI_NUM_CUTS; ++k) b += (e > th[k]) ? 1 : 0;
    bin[row] = (uint8_t)b;
  }
}

// All 10 cut costs in one pass over the edges (normalized_cut.py:4-11 for each threshold):
//   cut_k    = sum over stored (i, j) with i in A_k, j in B_k of w_ij   (= (sum W - W_AA - W_BB) / 2)
//   assocA_k = sum_{i in A_k} deg_i, assocB_k = sum_{i in B_k} deg_i   (deg of W = w + I)
// An entry (i, j) with bin_j < bin_i is cut for every k in [bin_j, bin_i).  part[block][AI_SWEEP_VALS]: the task's partials.
template <class Graph>
__device__ __forceinline__ void sweep_body(const Task* __restrict__ ftasks, const int32_t* __restrict__ nosplit, const Graph g,
                                           const double* __restrict__ deg, const uint8_t* __restrict__ bin, double* __restrict__ part) {
  // the block's partial cut sums go through LDS transposed, so that each of the 10 columns is
  // reduced by ONE wave (fixed order) instead of 40 block-wide reductions with two barriers each
  __shared__ double scut[AI_NUM_CUTS][AI_BLOCK + 1];
  __shared__ double sdeg[AI_FINE_ROWS];
  __shared__ int sbin[AI_FINE_ROWS];
  const Task tk = ftasks[blockIdx.x];
  if (nosplit[tk.z]) return;
  const auto rows = g.rows(tk);
  const int32_t* __restrict__ col = g.col(tk);
  const double* __restrict__ wraw = g.w(tk);
  const int l = threadIdx.x & (AI_LPR - 1), r = threadIdx.x / AI_LPR;
  if (threadIdx.x < AI_FINE_ROWS) {
    const int row = tk.x + threadIdx.x;
    sbin[threadIdx.x] = (row < tk.y) ? (int)bin[row] : -1;
    sdeg[threadIdx.x] = (row < tk.y) ? deg[row] : 0.0;
  }
  double cut[AI_NUM_CUTS];
#pragma unroll
  for (int k = 0; k < AI_NUM_CUTS; ++k) cut[k] = 0.0;
  for (int row = tk.x + r; row < tk.y; row += AI_BLOCK / AI_LPR) {
    const int bi = bin[row];
    const int2 se = rows(row);
    const int p0 = se.x, p1 = se.y;
    {
      int c[AI_ROW_PF], bj[AI_ROW_PF];
      double w[AI_ROW_PF];
#pragma unroll
      for (int q = 0; q < AI_ROW_PF; ++q) {
        const int p = p0 + l + q * AI_LPR;
        const bool ok = p < p1;
        c[q] = ok ? col[p] : -1;
        w[q] = ok ? wraw[p] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < AI_ROW_PF; ++q) bj[q] = (c[q] >= 0) ? (int)bin[c[q]] : 0;
#pragma unroll
      for (int q = 0; q < AI_ROW_PF; ++q)
        if (c[q] >= 0) {
#pragma unroll
          for (int k = 0; k < AI_NUM_CUTS; ++k) cut[k] += (k >= bj[q] && k < bi) ? w[q] : 0.0;
        }
    }
    for (int p = p0 + l + AI_ROW_PF * AI_LPR; p < p1; p += AI_LPR) {
      const int bj = bin[col[p]];
      const double w = wraw[p];
#pragma unroll
      for (int k = 0; k < AI_NUM_CUTS; ++k) cut[k] += (k >= bj && k < bi) ? w : 0.0;
    }
  }
#pragma unroll
  for (int k = 0; k < AI_NUM_CUTS; ++k) scut[k][threadIdx.x] = cut[k];
  __syncthreads();
  double* out = part + (size_t)blockIdx.x * AI_SWEEP_VALS;
  const int w = threadIdx.x >> 6, ln = threadIdx.x & 63;
  for (int k = w; k < AI_NUM_CUTS; k += AI_BLOCK / 64) {
    double a = 0.0;
#pragma unroll
    for (int q = 0; q < AI_BLOCK / 64; ++q) a += scut[k][ln + 64 * q];
    a = ai_wave_sum(a);
    if (ln == 0) out[k] = a;
  }
  // assocA_k / assocB_k / |A_k| over the task's rows in row order (30 threads, 32 rows each)
  if (threadIdx.x < 3 * AI_NUM_CUTS) {
    const int which = threadIdx.x / AI_NUM_CUTS, k = threadIdx.x % AI_NUM_CUTS;
    double a = 0.0;
    for (int i = 0; i < AI_FINE_ROWS; ++i) {
      const int bi = sbin[i];
      if (bi < 0) break;
      const bool inA = k < bi;
      a += (which == 0) ? (inA ? sdeg[i] : 0.0) : (which == 1) ? (inA ? 0.0 : sdeg[i]) : (inA ? 1.0 : 0.0);
    }
    out[(which + 1) * AI_NUM_CUTS + k] = a;
  }
}

// task stripes that sweep_final_body sums a partial column over before adding them in stripe order
#define SWF_STRIPES 6

// One segment, one block, partials part[t0..t1): ncut_k = cut_k / assocA_k + cut_k / assocB_k; first strictly smaller cost wins
// (normalized_cut.py:29-32); split iff mcut < T (:56).  Column c of the 40 partial columns is summed by 6 threads over interleaved
// task stripes, then in stripe order.  Results go to element s of each array; costs[s][10] may be null: nobody wants them.
__device__ __forceinline__ void sweep_final_body(const double* __restrict__ part, int t0, int t1, double T, int s,
                                                 double* __restrict__ costs, int32_t* __restrict__ kstar, int32_t* __restrict__ split,
                                                 int32_t* __restrict__ ntrue, double* __restrict__ mcut) {
  __shared__ double acc[SWF_STRIPES][AI_SWEEP_VALS];
  const int c = threadIdx.x % AI_SWEEP_VALS, stripe = threadIdx.x / AI_SWEEP_VALS;
  if (stripe < SWF_STRIPES) {
    double a = 0.0;
    for (int t = t0 + stripe; t < t1; t += SWF_STRIPES) a += part[(size_t)t * AI_SWEEP_VALS + c];
    acc[stripe][c] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double best = INFINITY;
    int kb = 0;
    double nb = 0.0;
    for (int k = 0; k < AI_NUM_CUTS; ++k) {
      double v[4];
      for (int q = 0; q < 4; ++q) {
        double a = 0.0;
        for (int st = 0; st < SWF_STRIPES; ++st) a += acc[st][q * AI_NUM_CUTS + k];
        v[q] = a;
      }
      const double cost = __dadd_rn(__ddiv_rn(v[0], v[1]), __ddiv_rn(v[0], v[2]));
      if (costs) costs[s * AI_NUM_CUTS + k] = cost;
      if (cost < best) {
        best = cost;
        kb = k;
        nb = v[3];
      }
    }
    kstar[s] = kb;
    mcut[s] = best;
    split[s] = (best < T) ? 1 : 0;
    ntrue[s] = (int32_t)nb;
  }
}

}  // namespace
