// Chebyshev-filtered subspace iteration for the k smallest non-trivial eigenpairs of L_sym of ONE connected graph
// (BASELINE.json configs[4]: k = 64 on a ~1M-row graph).  Included by ai_eigs.inc after the Solver class.
//
// The reference only ever asks for k = 2 (normalized_cut.py:49); for k = 64 on a million rows single-vector Lanczos
// with full re-orthogonalisation needs > 4000 steps (the 64th eigenvalue is 1e-5 of the spectrum away from the 65th)
// and O(m^2 N) bytes of Gram-Schmidt traffic: measured 102 s WITHOUT converging (profiles/r02_cfg5_lanczos_fro.json).
// A block method converges with the gap to the first eigenvalue OUTSIDE the block instead: here a block of
// B = 64 or 128 vectors is filtered with a scaled Chebyshev polynomial of M = I - L that damps [-1, theta_B] and
// amplifies everything above (Zhou & Saad's ChFSI), re-orthonormalised (Cholesky QR, twice) and Rayleigh-Ritz
// rotated, until the first k residuals are below the tolerance.  One polynomial degree = ONE fused kernel over the
// graph (SpMM + three-term recurrence); the rotations X <- X Q are plain library GEMMs (rocBLAS, float64); the Gram and
// projected matrices (128 x 128 reductions over a million rows, a shape rocBLAS runs at 0.6 TFLOP/s) are reduced by k_cf_gram.  The known top eigenvector u1 = D^1/2 1 / sqrt(vol) is projected out of the block.
#include <rocblas/rocblas.h>
#include "ai_dense_sym.h"
#ifndef AI_CF_GROUP_ROWS
#define AI_CF_GROUP_ROWS 8
#endif

namespace {

#define AI_RB(expr)                                                                            \
  do {                                                                                         \
    rocblas_status _s = (expr);                                                                \
    if (_s != rocblas_status_success) {                                                        \
      ai_set_error("%s:%d: %s -> rocblas status %d", __FILE__, __LINE__, #expr, (int)_s);      \
      return AI_ERR_HIP;                                                                       \
    }                                                                                          \
  } while (0)

// X[row, c] = deterministic pseudo-random start entry from the caller's row id and the column
template <int CPL>
__global__ __launch_bounds__(AI_BLOCK) void k_cf_init(int32_t n, const int32_t* __restrict__ orig, double* __restrict__ X) {
  constexpr int B = 64 * CPL;
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= (int64_t)n * B) return;
  const int row = (int)(i / B), c = (int)(i % B);
  X[i] = ai_hash_unit((uint32_t)orig[row] * 2654435761u + (uint32_t)(c + 1) * 40503u);
}

// One polynomial degree: Yn[row, :] = alpha * (M Y)[row, :] + beta * Y[row, :] + gamma * Xp[row, :],
// (M Y)[row, :] = sum_j wm[row, j] Y[j, :] + sinv2[row] Y[row, :].  One wave per row, lane t owns columns
// t * CPL .. t * CPL + CPL - 1: a gathered row of Y is one coalesced 512 B / 1 KB read, the row's entries are
// wave-uniform (scalar) loads.  Rows are dealt to the XCDs in contiguous eighths so that the neighbours' rows of Y
// are re-used from that XCD's L2.
template <int CPL>
__global__ __launch_bounds__(AI_BLOCK) void k_cf_spmm(int32_t n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                      const double* __restrict__ wm, const double* __restrict__ sinv2,
                                                      const double* __restrict__ Y, const double* __restrict__ Xp,
                                                      double* __restrict__ Yn, double alpha, double beta, double gamma) {
  constexpr int B = 64 * CPL;
  const int row = ai_xcd_task(blockIdx.x, gridDim.x) * (AI_BLOCK / 64) + (threadIdx.x >> 6);
  if (row >= n) return;
  const int lane = threadIdx.x & 63;
  const int p0 = __builtin_amdgcn_readfirstlane(rowptr[row]), p1 = __builtin_amdgcn_readfirstlane(rowptr[row + 1]);
  double acc[CPL];
#pragma unroll
  for (int i = 0; i < CPL; ++i) acc[i] = 0.0;
  int p = p0;
  for (; p + 8 <= p1; p += 8) {
    int c[8];
    double w[8], v[8][CPL];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      c[q] = __builtin_amdgcn_readfirstlane(col[p + q]);
      w[q] = wm[p + q];
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int i = 0; i < CPL; ++i) v[q][i] = Y[(size_t)c[q] * B + lane * CPL + i];
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int i = 0; i < CPL; ++i) acc[i] = fma(w[q], v[q][i], acc[i]);
  }
  for (; p < p1; ++p) {
    const int c = __builtin_amdgcn_readfirstlane(col[p]);
    const double w = wm[p];
#pragma unroll
    for (int i = 0; i < CPL; ++i) acc[i] = fma(w, Y[(size_t)c * B + lane * CPL + i], acc[i]);
  }
  const double s2 = sinv2[row];
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const size_t o = (size_t)row * B + lane * CPL + i;
    const double y = Y[o];
    double r = alpha * fma(s2, y, acc[i]) + beta * y;
    if (gamma != 0.0) r = fma(gamma, Xp[o], r);
    Yn[o] = r;
  }
}

// ---- grouped SpMM.  k_cf_spmm reads one 512 B / 1 KB row of Y per stored ENTRY: 48 rows per output row, ~14 x the
// algorithmic bytes, all of it L2 traffic (the kernel sits on the L2, not on HBM).  Consecutive (Morton-ordered) rows share most
// of their neighbours, so R consecutive rows are given ONE merged, column-sorted list of their distinct neighbours with an R-vector
// of weights per neighbour (0 where a row does not have it); a wave then reads each distinct row of Y once and feeds R
// accumulators.  A row's sum is formed in the same (column) order as before, the extra terms are exact zeros: the result is bit
// for bit k_cf_spmm's when every row's columns are stored ascending (checked once; otherwise the plain kernel runs).
__global__ __launch_bounds__(AI_BLOCK) void k_cf_sorted(int32_t n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                        int32_t* __restrict__ unsorted) {
  const int row = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (row >= n) return;
  for (int p = rowptr[row] + 1; p < rowptr[row + 1]; ++p)
    if (col[p] <= col[p - 1]) {
      *unsorted = 1;
      return;
    }
}
// one thread per group: R-way merge of the rows' sorted lists; FILL = false counts the distinct columns, true writes them
template <int R, bool FILL>
__global__ __launch_bounds__(AI_BLOCK) void k_cf_group(int32_t n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                       const double* __restrict__ wm, const int32_t* __restrict__ goff,
                                                       int32_t* __restrict__ gcnt, int32_t* __restrict__ gcol, double* __restrict__ gw) {
  const int g = blockIdx.x * AI_BLOCK + threadIdx.x;
  const int ng = (n + R - 1) / R;
  if (g >= ng) return;
  int p[R], e[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = g * R + r;
    p[r] = row < n ? rowptr[row] : 0;
    e[r] = row < n ? rowptr[row + 1] : 0;
  }
  int cnt = 0;
  const int base = FILL ? goff[g] : 0;
  for (;;) {
    int c = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (p[r] < e[r]) c = min(c, col[p[r]]);
    if (c == 0x7fffffff) break;
    if (FILL) gcol[base + cnt] = c;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      double w = 0.0;
      if (p[r] < e[r] && col[p[r]] == c) {
        if (FILL) w = wm[p[r]];
        ++p[r];
      }
      if (FILL) gw[(size_t)(base + cnt) * R + r] = w;
    }
    ++cnt;
  }
  if (!FILL) gcnt[g] = cnt;
}
// VT = double, or float for the EARLY outer iterations of the filter (round 5): while the block's residuals are above ~1e-4 the
// polynomial only has to separate the wanted end of the spectrum from the rest, which a float32 recurrence does as well (its rounding,
// ~1e-6 after a few hundred degrees, is far below the residuals it is asked to reduce); orthonormalisation, Rayleigh-Ritz and the
// residual test stay float64, and the last outer iterations run in float64 so that the pairs reach the tolerance.  Half the bytes per
// gathered row of the block, which is what this kernel waits for.
template <int CPL, int R, typename VT>
__global__ __launch_bounds__(AI_BLOCK) void k_cf_spmm_g(int32_t n, const int32_t* __restrict__ goff, const int32_t* __restrict__ gcol,
                                                        const VT* __restrict__ gw, const double* __restrict__ sinv2,
                                                        const VT* __restrict__ Y, const VT* __restrict__ Xp,
                                                        VT* __restrict__ Yn, double alpha_, double beta_, double gamma_) {
  const VT alpha = (VT)alpha_, beta = (VT)beta_, gamma = (VT)gamma_;
  constexpr int B = 64 * CPL;
  const int ng = (n + R - 1) / R;
  const int g = ai_xcd_task(blockIdx.x, gridDim.x) * (AI_BLOCK / 64) + (threadIdx.x >> 6);
  if (g >= ng) return;
  const int lane = threadIdx.x & 63;
  const int p0 = __builtin_amdgcn_readfirstlane(goff[g]), p1 = __builtin_amdgcn_readfirstlane(goff[g + 1]);
  VT acc[R][CPL];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int i = 0; i < CPL; ++i) acc[r][i] = (VT)0;
#ifndef AI_CF_INFLIGHT
#define AI_CF_INFLIGHT 4
#endif
  constexpr int U = AI_CF_INFLIGHT;  // distinct rows of Y in flight
  int p = p0;
  for (; p + U <= p1; p += U) {
    int c[U];
    VT v[U][CPL];
#pragma unroll
    for (int q = 0; q < U; ++q) c[q] = __builtin_amdgcn_readfirstlane(gcol[p + q]);
#pragma unroll
    for (int q = 0; q < U; ++q)
#pragma unroll
      for (int i = 0; i < CPL; ++i) v[q][i] = Y[(size_t)c[q] * B + lane * CPL + i];
#pragma unroll
    for (int q = 0; q < U; ++q)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const VT w = gw[(size_t)(p + q) * R + r];
#pragma unroll
        for (int i = 0; i < CPL; ++i) acc[r][i] = fma(w, v[q][i], acc[r][i]);
      }
  }
  for (; p < p1; ++p) {
    const int c = __builtin_amdgcn_readfirstlane(gcol[p]);
    VT v[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) v[i] = Y[(size_t)c * B + lane * CPL + i];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const VT w = gw[(size_t)p * R + r];
#pragma unroll
      for (int i = 0; i < CPL; ++i) acc[r][i] = fma(w, v[i], acc[r][i]);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int row = g * R + r;
    if (row < n) {
      const VT s2 = (VT)sinv2[row];
#pragma unroll
      for (int i = 0; i < CPL; ++i) {
        const size_t o = (size_t)row * B + lane * CPL + i;
        const VT y = Y[o];
        VT x = alpha * fma(s2, y, acc[r][i]) + beta * y;
        if (gamma_ != 0.0) x = fma(gamma, Xp[o], x);
        Yn[o] = x;
      }
    }
  }
}

template <typename A, typename Bt>
__global__ __launch_bounds__(AI_BLOCK) void k_cf_convert(size_t count, const A* __restrict__ in, Bt* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * AI_BLOCK + threadIdx.x; i < count; i += (size_t)gridDim.x * AI_BLOCK) out[i] = (Bt)in[i];
}

// part[block][c] = sum over the block's rows of f(row, c); f = u1[row] * X[row, c] (mode 0) or
// (Z[row, c] - theta[c] * X[row, c])^2 (mode 1).  Fixed summation order: rows strided by the grid, waves added in order.
template <int CPL>
__global__ __launch_bounds__(AI_BLOCK) void k_cf_colsum(int32_t n, int mode, const double* __restrict__ u1, const double* __restrict__ X,
                                                        const double* __restrict__ Z, const double* __restrict__ theta,
                                                        double* __restrict__ part) {
  constexpr int B = 64 * CPL;
  __shared__ double sm[AI_BLOCK / 64][B];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc[CPL], th[CPL];
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    acc[i] = 0.0;
    th[i] = (mode == 1) ? theta[lane * CPL + i] : 0.0;
  }
  for (int row = blockIdx.x * (AI_BLOCK / 64) + w; row < n; row += gridDim.x * (AI_BLOCK / 64)) {
    const double u = (mode == 0) ? u1[row] : 0.0;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
      const size_t o = (size_t)row * B + lane * CPL + i;
      if (mode == 0) {
        acc[i] = fma(u, X[o], acc[i]);
      } else {
        const double r = Z[o] - th[i] * X[o];
        acc[i] = fma(r, r, acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < CPL; ++i) sm[w][lane * CPL + i] = acc[i];
  __syncthreads();
  for (int c = threadIdx.x; c < B; c += AI_BLOCK) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < AI_BLOCK / 64; ++q) t += sm[q][c];
    part[(size_t)blockIdx.x * B + c] = t;
  }
}

// X[row, c] -= u1[row] * g[c]
template <int CPL>
__global__ __launch_bounds__(AI_BLOCK) void k_cf_rank1(int32_t n, const double* __restrict__ u1, const double* __restrict__ g,
                                                       double* __restrict__ X) {
  constexpr int B = 64 * CPL;
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= (int64_t)n * B) return;
  X[i] = fma(-u1[i / B], g[i % B], X[i]);
}

// out[c][row] = X[row, c] for c < kv (Ritz vectors as contiguous rows, like lanczos_fro's output; u1 is not in the block)
template <int CPL>
__global__ __launch_bounds__(AI_BLOCK) void k_cf_extract(int32_t n, int kv, const double* __restrict__ X, double* __restrict__ out,
                                                         size_t out_stride) {
  constexpr int B = 64 * CPL;
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= (int64_t)n * kv) return;
  const int c = (int)(i / n), row = (int)(i % n);
  out[(size_t)c * out_stride + row] = X[(size_t)row * B + c];
}

// C = A^T B for two tall-skinny row-major blocks (n x B each), B = 64 * CPL: the Gram matrix of the block and the
// projected matrix of the Rayleigh-Ritz step.  rocBLAS runs this shape (m = n = 128, k = 10^6) at 0.6 TFLOP/s, 53 ms a
// call, a third of the whole solve, so it is reduced here: a block owns a contiguous range of rows, stages 8 rows of
// A and B at a time in LDS, and every thread keeps a TT x TT tile of C in registers; per-block partial matrices are
// then added in block order (fixed summation order: reproducible).
template <int CPL>
__global__ __launch_bounds__(AI_BLOCK) void k_cf_gram(int32_t n, const double* __restrict__ A, const double* __restrict__ Bm,
                                                      double* __restrict__ part) {
  constexpr int B = 64 * CPL, TT = B / 16, RB = 8;
  __shared__ double As[RB][B], Bs[RB][B];
  const int ti = threadIdx.x / 16, tj = threadIdx.x % 16;
  double c[TT][TT];
#pragma unroll
  for (int i = 0; i < TT; ++i)
#pragma unroll
    for (int j = 0; j < TT; ++j) c[i][j] = 0.0;
  const int64_t per = ((int64_t)n + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = min(r0 + per, (int64_t)n);
  for (int64_t rb = r0; rb < r1; rb += RB) {
    __syncthreads();
    for (int i = threadIdx.x; i < RB * B; i += AI_BLOCK) {
      const int rr = i / B, cc = i % B;
      const bool ok = rb + rr < r1;
      As[rr][cc] = ok ? A[(size_t)(rb + rr) * B + cc] : 0.0;
      Bs[rr][cc] = ok ? Bm[(size_t)(rb + rr) * B + cc] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < RB; ++rr) {
      double a[TT], b[TT];
#pragma unroll
      for (int i = 0; i < TT; ++i) {
        a[i] = As[rr][ti + 16 * i];   // strided ownership: consecutive threads read consecutive LDS words
        b[i] = Bs[rr][tj + 16 * i];
      }
#pragma unroll
      for (int i = 0; i < TT; ++i)
#pragma unroll
        for (int j = 0; j < TT; ++j) c[i][j] = fma(a[i], b[j], c[i][j]);
    }
  }
  double* out = part + (size_t)blockIdx.x * B * B;
#pragma unroll
  for (int i = 0; i < TT; ++i)
#pragma unroll
    for (int j = 0; j < TT; ++j) out[(size_t)(ti + 16 * i) * B + (tj + 16 * j)] = c[i][j];
}

// C[e] = sum over blocks (in block order) of part[block][e]
__global__ __launch_bounds__(AI_BLOCK) void k_cf_gram_sum(int nblk, int elems, const double* __restrict__ part, double* __restrict__ C) {
  const int e = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (e >= elems) return;
  double t = 0.0;
  for (int b = 0; b < nblk; ++b) t += part[(size_t)b * elems + e];
  C[e] = t;
}

// ---- host: dense symmetric helpers on B x B matrices (B <= 128), row-major
// Cholesky G = L L^T (lower, in place in `a`); returns false on a non-positive pivot
bool cf_cholesky(std::vector<double>& a, int B) {
  for (int j = 0; j < B; ++j) {
    double d = a[(size_t)j * B + j];
    for (int k = 0; k < j; ++k) d -= a[(size_t)j * B + k] * a[(size_t)j * B + k];
    if (!(d > 0.0)) return false;
    d = sqrt(d);
    a[(size_t)j * B + j] = d;
    for (int i = j + 1; i < B; ++i) {
      double s = a[(size_t)i * B + j];
      for (int k = 0; k < j; ++k) s -= a[(size_t)i * B + k] * a[(size_t)j * B + k];
      a[(size_t)i * B + j] = s / d;
    }
  }
  return true;
}
// rinv (row-major, upper triangular) = (L^T)^-1
void cf_rinv(const std::vector<double>& L, int B, std::vector<double>& rinv) {
  std::vector<double> li((size_t)B * B, 0.0);  // L^-1 (lower)
  for (int j = 0; j < B; ++j) {
    li[(size_t)j * B + j] = 1.0 / L[(size_t)j * B + j];
    for (int i = j + 1; i < B; ++i) {
      double s = 0.0;
      for (int k = j; k < i; ++k) s -= L[(size_t)i * B + k] * li[(size_t)k * B + j];
      li[(size_t)i * B + j] = s / L[(size_t)i * B + i];
    }
  }
  rinv.assign((size_t)B * B, 0.0);
  for (int i = 0; i < B; ++i)
    for (int j = i; j < B; ++j) rinv[(size_t)i * B + j] = li[(size_t)j * B + i];
}
struct ChfsiStats {
  int outer = 0, degrees = 0, spmm = 0, spmm32 = 0;
  double ms_filter = 0.0, ms_rr = 0.0, ms_host_eig = 0.0, ms_host_chol = 0.0;
};

// k1 largest eigenpairs of M restricted to the complement of u1 (= eigenpairs 2 .. k1 + 1 of L_sym) of the ONE
// connected segment the solver holds (after begin / build_tasks / prepare).  thetas descending; Ritz vectors into
// out (k1 rows of out_stride doubles, compact row order); resids = true residual norms ||M x - theta x||.
template <int CPL>
int chfsi_solve(Solver& S, int k1, double tol, std::vector<double>& thetas, std::vector<double>& resids, double* out, size_t out_stride,
                ChfsiStats* cs) {
  constexpr int B = 64 * CPL;
  const int n = S.segs[0].n;
  hipStream_t st = S.st;
  const size_t nb = (size_t)n * B;
  DevBuf<double> bx, by, bt, bz, dG, dQ, dpart, dvec, dgp;
  AI_TRY(bx.alloc(nb));
  AI_TRY(by.alloc(nb));
  AI_TRY(bt.alloc(nb));
  AI_TRY(bz.alloc(nb));
  AI_TRY(dG.alloc((size_t)B * B));
  AI_TRY(dQ.alloc((size_t)B * B));
  const int PB = 512;  // blocks of the column reductions
  AI_TRY(dpart.alloc((size_t)PB * B));
  AI_TRY(dvec.alloc(B));
  const int GB = 512;  // blocks (row ranges) of the Gram reduction
  AI_TRY(dgp.alloc((size_t)GB * B * B));
  double *X = bx.p, *Y = by.p, *T = bt.p, *Z = bz.p;
  rocblas_handle h = nullptr;
  AI_RB(rocblas_create_handle(&h));
  struct HandleGuard {
    rocblas_handle h;
    ~HandleGuard() { (void)rocblas_destroy_handle(h); }
  } guard{h};
  AI_RB(rocblas_set_stream(h, st));
  AI_RB(rocblas_set_pointer_mode(h, rocblas_pointer_mode_host));
  const double one = 1.0, zero = 0.0;
  const unsigned gel = (unsigned)((nb + AI_BLOCK - 1) / AI_BLOCK), grow = (unsigned)((n + (AI_BLOCK / 64) - 1) / (AI_BLOCK / 64));
  std::vector<double> hpart((size_t)PB * B), hv(B), hG((size_t)B * B), hQ, hR;

  // merged neighbour lists of GR consecutive rows (see k_cf_spmm_g), built once per solve when every row's columns ascend
  constexpr int GR = AI_CF_GROUP_ROWS;
  const int ng = (n + GR - 1) / GR;
  DevBuf<int32_t> gflag, gcnt, goff, gcol, gtmp;
  DevBuf<double> gw;
  bool grouped = false;
  {
    AI_TRY(gflag.alloc(1));
    AI_HIP(hipMemsetAsync(gflag.p, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(k_cf_sorted, dim3((n + AI_BLOCK - 1) / AI_BLOCK), dim3(AI_BLOCK), 0, st, (int32_t)n, S.rowptr, S.col, gflag.p);
    AI_KERNEL_CHECK();
    int32_t unsorted = 0;
    AI_HIP(hipMemcpyAsync(&unsorted, gflag.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AI_HIP(hipStreamSynchronize(st));
    if (!unsorted && !getenv("AI_EIGS_PLAIN_SPMM")) {
      AI_TRY(gcnt.alloc((size_t)ng + 1));
      AI_TRY(goff.alloc((size_t)ng + 1));
      AI_TRY(gtmp.alloc(ai_scan_tmp_elems((int64_t)ng)));
      hipLaunchKernelGGL((k_cf_group<GR, false>), dim3((ng + AI_BLOCK - 1) / AI_BLOCK), dim3(AI_BLOCK), 0, st, (int32_t)n, S.rowptr, S.col,
                         (const double*)S.wm.p, (const int32_t*)nullptr, gcnt.p, (int32_t*)nullptr, (double*)nullptr);
      AI_KERNEL_CHECK();
      AI_TRY(ai_exclusive_scan_i32(st, gcnt.p, goff.p, ng, gtmp.p));
      int32_t total = 0;
      AI_HIP(hipMemcpyAsync(&total, goff.p + ng, sizeof(int32_t), hipMemcpyDeviceToHost, st));
      AI_HIP(hipStreamSynchronize(st));
      AI_TRY(gcol.alloc((size_t)total + 1));
      AI_TRY(gw.alloc((size_t)total * GR + 1));
      hipLaunchKernelGGL((k_cf_group<GR, true>), dim3((ng + AI_BLOCK - 1) / AI_BLOCK), dim3(AI_BLOCK), 0, st, (int32_t)n, S.rowptr, S.col,
                         (const double*)S.wm.p, (const int32_t*)goff.p, (int32_t*)nullptr, gcol.p, gw.p);
      AI_KERNEL_CHECK();
      grouped = true;
      if (getenv("AI_NCUT_DEBUG"))
        fprintf(stderr, "[ai_eigs chfsi] %d rows in groups of %d: %d distinct neighbours\n", n, GR, total);
    }
  }
  const unsigned ggrid = (unsigned)((ng + (AI_BLOCK / 64) - 1) / (AI_BLOCK / 64));
  auto spmm = [&](const double* in, const double* prev, double* o, double alpha, double beta, double gamma) -> int {
    if (grouped)
      hipLaunchKernelGGL((k_cf_spmm_g<CPL, GR, double>), dim3(ggrid), dim3(AI_BLOCK), 0, st, (int32_t)n, (const int32_t*)goff.p, (const int32_t*)gcol.p,
                         (const double*)gw.p, (const double*)S.sinv2.p, in, prev, o, alpha, beta, gamma);
    else
      hipLaunchKernelGGL((k_cf_spmm<CPL>), dim3(grow), dim3(AI_BLOCK), 0, st, (int32_t)n, S.rowptr, S.col, (const double*)S.wm.p,
                         (const double*)S.sinv2.p, in, prev, o, alpha, beta, gamma);
    AI_KERNEL_CHECK();
    if (cs) ++cs->spmm;
    return AI_OK;
  };
  // the same product on a float32 copy of the block (early outer iterations of the filter: k_cf_spmm_g<.., float>); the float32
  // buffers: three blocks and the merged weights
  DevBuf<float> fx, fy, ft, gwf;
  static const int f32_filter = getenv("AI_EIGS_F32_FILTER") ? atoi(getenv("AI_EIGS_F32_FILTER")) : 1;
  const double f32_above = 1e-4;   // worst residual above which an outer iteration filters in float32
  auto spmm32 = [&](const float* in, const float* prev, float* o, double alpha, double beta, double gamma) -> int {
    hipLaunchKernelGGL((k_cf_spmm_g<CPL, GR, float>), dim3(ggrid), dim3(AI_BLOCK), 0, st, (int32_t)n, (const int32_t*)goff.p, (const int32_t*)gcol.p,
                       (const float*)gwf.p, (const double*)S.sinv2.p, in, prev, o, alpha, beta, gamma);
    AI_KERNEL_CHECK();
    if (cs) {
      ++cs->spmm;
      ++cs->spmm32;
    }
    return AI_OK;
  };
  if (grouped && f32_filter) {   // taken with the other blocks, so that the call's workspace has its final size from the first call on
    AI_TRY(fx.alloc(nb));
    AI_TRY(fy.alloc(nb));
    AI_TRY(ft.alloc(nb));
    AI_TRY(gwf.alloc(gw.count));
    hipLaunchKernelGGL((k_cf_convert<double, float>), dim3(4096), dim3(AI_BLOCK), 0, st, gw.count, (const double*)gw.p, gwf.p);
    AI_KERNEL_CHECK();
  }
  // dG (row-major B x B) = A^T Bm
  auto gram = [&](const double* A, const double* Bm) -> int {
    hipLaunchKernelGGL((k_cf_gram<CPL>), dim3(GB), dim3(AI_BLOCK), 0, st, (int32_t)n, A, Bm, dgp.p);
    AI_KERNEL_CHECK();
    hipLaunchKernelGGL(k_cf_gram_sum, dim3((B * B + AI_BLOCK - 1) / AI_BLOCK), dim3(AI_BLOCK), 0, st, GB, B * B, (const double*)dgp.p, dG.p);
    AI_KERNEL_CHECK();
    return AI_OK;
  };
  // column sums -> hv (host), fixed order
  auto colsum = [&](int mode, const double* A, const double* Zz, const double* theta_dev) -> int {
    hipLaunchKernelGGL((k_cf_colsum<CPL>), dim3(PB), dim3(AI_BLOCK), 0, st, (int32_t)n, mode, (const double*)S.u1.p, A, Zz, theta_dev, dpart.p);
    AI_KERNEL_CHECK();
    AI_HIP(hipMemcpyAsync(hpart.data(), dpart.p, hpart.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    AI_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < B; ++c) {
      double t = 0.0;
      for (int b = 0; b < PB; ++b) t += hpart[(size_t)b * B + c];
      hv[c] = t;
    }
    return AI_OK;
  };
  // A <- A - u1 (u1^T A)
  auto project = [&](double* A) -> int {
    AI_TRY(colsum(0, A, nullptr, nullptr));
    AI_HIP(hipMemcpyAsync(dvec.p, hv.data(), B * sizeof(double), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL((k_cf_rank1<CPL>), dim3(gel), dim3(AI_BLOCK), 0, st, (int32_t)n, (const double*)S.u1.p, (const double*)dvec.p, A);
    AI_KERNEL_CHECK();
    AI_HIP(hipStreamSynchronize(st));  // hv is re-used by the next reduction
    return AI_OK;
  };
  // A <- A R^-1 with G = A^T A = R^T R (result in `tmp`, pointers swapped by the caller)
  auto cholqr = [&](double*& A, double*& tmp) -> int {
    AI_TRY(gram(A, A));
    AI_HIP(hipMemcpyAsync(hG.data(), dG.p, hG.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    AI_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < B; ++i)
      for (int j = i + 1; j < B; ++j) hG[(size_t)i * B + j] = hG[(size_t)j * B + i] = 0.5 * (hG[(size_t)i * B + j] + hG[(size_t)j * B + i]);
    const double tc0 = now_ms();
    if (!cf_cholesky(hG, B)) {
      ai_set_error("ai_eigs_smallest: the filtered block lost rank (Cholesky of its Gram matrix failed)");
      return AI_ERR_NO_CONVERGENCE;
    }
    cf_rinv(hG, B, hR);
    if (cs) cs->ms_host_chol += now_ms() - tc0;
    AI_HIP(hipMemcpyAsync(dQ.p, hR.data(), hR.size() * sizeof(double), hipMemcpyHostToDevice, st));
    AI_RB(rocblas_dgemm(h, rocblas_operation_none, rocblas_operation_none, B, n, B, &one, dQ.p, B, A, B, &zero, tmp, B));
    AI_HIP(hipStreamSynchronize(st));  // hR is re-used
    std::swap(A, tmp);
    return AI_OK;
  };
  // Rayleigh-Ritz of the orthonormal block A: Z = M A; H = A^T Z; A <- A Q, Z <- Z Q; theta descending
  std::vector<double> theta(B, 0.0);
  auto rayleigh_ritz = [&](double*& A, double*& tmp) -> int {
    AI_TRY(spmm(A, nullptr, Z, 1.0, 0.0, 0.0));
    AI_TRY(gram(A, Z));
    AI_HIP(hipMemcpyAsync(hG.data(), dG.p, hG.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    AI_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < B; ++i)
      for (int j = i + 1; j < B; ++j) hG[(size_t)i * B + j] = hG[(size_t)j * B + i] = 0.5 * (hG[(size_t)i * B + j] + hG[(size_t)j * B + i]);
    const double tj0 = now_ms();
    if (!cf_eigh(hG, B, theta, hQ)) cf_jacobi(hG, B, theta, hQ);
    if (cs) cs->ms_host_eig += now_ms() - tj0;
    if (getenv("AI_NCUT_DEBUG")) {  // cross-check against the Jacobi solver
      std::vector<double> tj, qj;
      cf_jacobi(hG, B, tj, qj);
      double dmax = 0.0, omax = 0.0;
      for (int i = 0; i < B; ++i) dmax = std::max(dmax, fabs(tj[i] - theta[i]));
      for (int i = 0; i < B; ++i)
        for (int j = 0; j < B; ++j) {
          double t = 0.0;
          for (int k = 0; k < B; ++k) t += hQ[(size_t)k * B + i] * hQ[(size_t)k * B + j];
          omax = std::max(omax, fabs(t - (i == j ? 1.0 : 0.0)));
        }
      fprintf(stderr, "[ai_eigs chfsi] projected eigenproblem: QL against Jacobi, largest eigenvalue difference %.3e; QL eigenvectors orthonormal to %.3e\n", dmax, omax);
    }
    AI_HIP(hipMemcpyAsync(dQ.p, hQ.data(), hQ.size() * sizeof(double), hipMemcpyHostToDevice, st));
    AI_RB(rocblas_dgemm(h, rocblas_operation_none, rocblas_operation_none, B, n, B, &one, dQ.p, B, A, B, &zero, tmp, B));
    std::swap(A, tmp);
    AI_RB(rocblas_dgemm(h, rocblas_operation_none, rocblas_operation_none, B, n, B, &one, dQ.p, B, Z, B, &zero, tmp, B));
    std::swap(Z, tmp);
    AI_HIP(hipStreamSynchronize(st));  // hQ is re-used
    return AI_OK;
  };

  hipLaunchKernelGGL((k_cf_init<CPL>), dim3(gel), dim3(AI_BLOCK), 0, st, (int32_t)n, S.orig, X);
  AI_KERNEL_CHECK();
  AI_TRY(project(X));
  AI_TRY(cholqr(X, T));
  AI_TRY(cholqr(X, T));
  AI_TRY(rayleigh_ritz(X, T));
  const double a = -1.0;  // every eigenvalue of M = D^-1/2 (w + I) D^-1/2 lies in [-1, 1]
  resids.assign(k1, 1e300);
  const int max_outer = 80;
  bool done = false;
  double worst_hist[2] = {-1.0, -1.0};  // worst residual before / after the previous filter
  int deg_hist = 0;
  for (int it = 0; it < max_outer && !done; ++it) {
    // damp [a, b], b = the block's smallest Ritz value; scaled Chebyshev recurrence (the value at 1 stays ~1)
    const double b = std::min(theta[B - 1], 1.0 - 1e-12);
    const double e = 0.5 * (b - a), c = 0.5 * (b + a);
    const double ttop = (1.0 - c) / e;
    const double rate = log(ttop + sqrt(std::max(ttop * ttop - 1.0, 0.0)));  // acosh
    int deg = (rate > 0.0) ? (int)ceil(log(2e5) / rate) : 300;
    deg = std::max(10, std::min(deg, 300));
    // the last filter need not amplify by 2e5: aim at tol / 3 at the per-degree reduction the previous filter achieved (the
    // reduction per degree grows from one outer iteration to the next, so this errs on the long side)
    if (worst_hist[0] > 0.0 && worst_hist[1] > 0.0 && worst_hist[1] < worst_hist[0] && deg_hist > 0 && worst_hist[1] > tol) {
      const double rho = log(worst_hist[0] / worst_hist[1]) / deg_hist;
      const double needd = log(worst_hist[1] / (tol / 3.0)) / rho;
      deg = std::min(deg, std::max(10, (int)ceil(1.15 * needd)));
    }
    double sigma = e / (1.0 - c);
    const double sigma1 = sigma;
    AI_HIP(hipEventRecord(S.ctx->ev[0], st));
    const bool in32 = grouped && f32_filter && (worst_hist[1] < 0.0 || worst_hist[1] > f32_above);
    if (in32) {
      float *Xf = fx.p, *Yf = fy.p, *Tf = ft.p;
      hipLaunchKernelGGL((k_cf_convert<double, float>), dim3(8192), dim3(AI_BLOCK), 0, st, nb, (const double*)X, Xf);
      AI_KERNEL_CHECK();
      AI_TRY(spmm32(Xf, nullptr, Yf, sigma1 / e, -c * sigma1 / e, 0.0));
      for (int t = 2; t <= deg; ++t) {
        const double sigma2 = 1.0 / (2.0 / sigma1 - sigma);
        AI_TRY(spmm32(Yf, Xf, Tf, 2.0 * sigma2 / e, -2.0 * sigma2 * c / e, -sigma * sigma2));
        float* old = Xf;
        Xf = Yf;
        Yf = Tf;
        Tf = old;
        sigma = sigma2;
      }
      // the filtered block is Yf (deg = 1) or, after the rotation above, Yf as well: back to float64 into X
      hipLaunchKernelGGL((k_cf_convert<float, double>), dim3(8192), dim3(AI_BLOCK), 0, st, nb, (const float*)Yf, X);
      AI_KERNEL_CHECK();
      AI_HIP(hipEventRecord(S.ctx->ev[1], st));
    } else {
    AI_TRY(spmm(X, nullptr, Y, sigma1 / e, -c * sigma1 / e, 0.0));
    for (int t = 2; t <= deg; ++t) {
      const double sigma2 = 1.0 / (2.0 / sigma1 - sigma);
      AI_TRY(spmm(Y, X, T, 2.0 * sigma2 / e, -2.0 * sigma2 * c / e, -sigma * sigma2));
      double* old = X;
      X = Y;
      Y = T;
      T = old;
      sigma = sigma2;
    }
    AI_HIP(hipEventRecord(S.ctx->ev[1], st));
    std::swap(X, Y);  // the filtered block
    }
    AI_TRY(project(X));
    AI_TRY(cholqr(X, T));
    AI_TRY(cholqr(X, T));
    AI_TRY(rayleigh_ritz(X, T));
    // residuals ||M x_i - theta_i x_i|| of the block (columns have unit norm)
    AI_HIP(hipMemcpyAsync(dvec.p, theta.data(), B * sizeof(double), hipMemcpyHostToDevice, st));
    AI_TRY(colsum(1, X, Z, dvec.p));
    double worst = 0.0;
    for (int i = 0; i < k1; ++i) {
      resids[i] = sqrt(std::max(hv[i], 0.0));
      worst = std::max(worst, resids[i]);
    }
    AI_HIP(hipEventRecord(S.ctx->ev[2], st));
    AI_HIP(hipStreamSynchronize(st));
    float m0 = 0.f, m1 = 0.f;
    AI_HIP(hipEventElapsedTime(&m0, S.ctx->ev[0], S.ctx->ev[1]));
    AI_HIP(hipEventElapsedTime(&m1, S.ctx->ev[1], S.ctx->ev[2]));
    if (cs) {
      ++cs->outer;
      cs->degrees += deg;
      cs->ms_filter += m0;
      cs->ms_rr += m1;
    }
    if (getenv("AI_NCUT_DEBUG"))
      fprintf(stderr, "[ai_eigs chfsi] outer %d%s: degree %d, b = %.9f, theta[%d] = %.12f, worst residual of the first %d = %.3e (filter %.1f ms, rr %.1f ms)\n",
              it, in32 ? " (float32 filter)" : "", deg, b, k1 - 1, theta[k1 - 1], k1, worst, m0, m1);
    worst_hist[0] = worst_hist[1];
    worst_hist[1] = worst;
    deg_hist = deg;
    if (worst <= tol) done = true;
  }
  thetas.assign(theta.begin(), theta.begin() + k1);
  hipLaunchKernelGGL((k_cf_extract<CPL>), dim3((unsigned)(((size_t)n * k1 + AI_BLOCK - 1) / AI_BLOCK)), dim3(AI_BLOCK), 0, st, (int32_t)n, k1,
                     (const double*)X, out, out_stride);
  AI_KERNEL_CHECK();
  AI_HIP(hipStreamSynchronize(st));
  return AI_OK;
}

}  // namespace
