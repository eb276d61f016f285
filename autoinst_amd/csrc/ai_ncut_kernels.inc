// Device kernels of the level-synchronous Solver (included by ai_solver.hip inside its anonymous namespace, after
// ai_ncut_shared.h; the shipped frontier has its own kernels in ai_flow_kernels.inc and takes nothing from this file).
// Sections: degrees / scaling, connected components, null-space vector (ai_fiedler on a disconnected graph), lock-step
// Lanczos (fused SpMV, update, convergence check, Ritz vectors), full re-orthogonalisation, threshold sweep,
// partition + CSR rebuild (binary Fiedler cuts and the split into connected components).

// For coarse tasks: the segment's fine-task range [x, y) and coarse-task range [z, w).
typedef int4 TaskRange;

// How a task of the Solver reaches its rows, columns and weights (the graph policy of the bodies in ai_ncut_shared.h): one CSR
// for every task of a level.
struct CsrGraph {
  const int32_t* __restrict__ rowptr;
  const int32_t* __restrict__ colp;
  const double* __restrict__ wp;
  struct Rows {
    const int32_t* __restrict__ rowptr;
    __device__ __forceinline__ int2 operator()(int row) const { return make_int2(rowptr[row], rowptr[row + 1]); }
  };
  __device__ __forceinline__ Rows rows(const Task&) const { return Rows{rowptr}; }
  __device__ __forceinline__ const int32_t* col(const Task&) const { return colp; }
  __device__ __forceinline__ const double* w(const Task&) const { return wp; }
};

// ----------------------------------------------------------------------------- degrees, scaling
// deg_i = 1 + sum_j w_ij (W = w + I, normalized_cut.py:38,42); s_i = 1 / sqrt(deg_i) (:43)
__global__ __launch_bounds__(AI_BLOCK) void k_degree(const Task* __restrict__ tasks, const int32_t* __restrict__ rowptr,
                                                     const double* __restrict__ wraw, double* __restrict__ deg,
                                                     double* __restrict__ sinv, double* __restrict__ pvol) {
  degree_body(tasks[blockIdx.x], CsrGraph{rowptr, nullptr, wraw}, deg, sinv, pvol);
}

// one block per segment: out[s] = sum of part[task0[s] .. task0[s+1]) in a fixed order
__global__ __launch_bounds__(AI_BLOCK) void k_seg_sum(const int32_t* __restrict__ task0, const double* __restrict__ part,
                                                      double* __restrict__ out) {
  __shared__ double sm[AI_BLOCK / 64];
  const int s = blockIdx.x;
  const double tot = ai_range_sum(part, task0[s], task0[s + 1], sm);
  if (threadIdx.x == 0) out[s] = tot;
}

// wm_ij = (s_i * w_ij) * s_j  (row scaling then column scaling, like D2 * (D - W) * D2, :47);
// sinv2_i = s_i * s_i is the "+ I" term of W; u1_i = sqrt(deg_i / vol_seg)
__global__ __launch_bounds__(AI_BLOCK) void k_scale(const Task* __restrict__ tasks, const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ col, const double* __restrict__ wraw,
                                                    const double* __restrict__ deg, const double* __restrict__ sinv,
                                                    const double* __restrict__ vol, double* __restrict__ wm,
                                                    double* __restrict__ sinv2, double* __restrict__ u1) {
  const Task tk = tasks[blockIdx.x];
  scale_body(tk, CsrGraph{rowptr, col, wraw}, vol[tk.z], deg, sinv, wm, sinv2, u1);
}

// ----------------------------------------------------------------------------- connected components
// rows of segments that need a fresh labelling: parent = smallest neighbour id <= row (no cycles:
// strictly decreasing chains); rows of the other segments keep the labels carried over the split
__global__ __launch_bounds__(AI_BLOCK) void k_cc_init(const Task* __restrict__ tasks, const int32_t* __restrict__ need_cc,
                                                      const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                      int32_t* __restrict__ parent) {
  const Task tk = tasks[blockIdx.x];
  if (!need_cc[tk.z]) return;
  const int l = threadIdx.x & (AI_LPR - 1), r = threadIdx.x / AI_LPR;
  for (int row = tk.x + r; row < tk.y; row += AI_BLOCK / AI_LPR) {
    int32_t mn = row;
    for (int p = rowptr[row] + l; p < rowptr[row + 1]; p += AI_LPR) mn = min(mn, col[p]);
    mn = min(mn, __shfl_xor(mn, 8, 16));
    mn = min(mn, __shfl_xor(mn, 4, 16));
    mn = min(mn, __shfl_xor(mn, 2, 16));
    mn = min(mn, __shfl_xor(mn, 1, 16));
    if (l == 0) parent[row] = mn;
  }
}

__global__ __launch_bounds__(AI_BLOCK) void k_cc_hook(const Task* __restrict__ tasks, const int32_t* __restrict__ need_cc,
                                                      const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                      int32_t* parent) {
  const Task tk = tasks[blockIdx.x];
  if (!need_cc[tk.z]) return;
  const int l = threadIdx.x & (AI_LPR - 1), r = threadIdx.x / AI_LPR;
  for (int row = tk.x + r; row < tk.y; row += AI_BLOCK / AI_LPR) {
    for (int p = rowptr[row] + l; p < rowptr[row + 1]; p += AI_LPR) {
      const int32_t c = col[p];
      if (c < row) uf_unite(parent, row, c);
    }
  }
}

__global__ __launch_bounds__(AI_BLOCK) void k_cc_compress(const Task* __restrict__ tasks, const int32_t* __restrict__ need_cc,
                                                          int32_t* parent) {
  const Task tk = tasks[blockIdx.x];
  if (!need_cc[tk.z]) return;
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    int32_t x = row;
    // chains are static in this launch (no hooking); stale values are still ancestors
    for (;;) {
      const int32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (p == x) break;
      x = p;
    }
    parent[row] = x;
  }
}

// roots per segment (integer atomics: order independent)
__global__ __launch_bounds__(AI_BLOCK) void k_cc_count(const Task* __restrict__ tasks, const int32_t* __restrict__ parent,
                                                       int32_t* __restrict__ ncomp) {
  const Task tk = tasks[blockIdx.x];
  int c = 0;
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) c += (parent[row] == row);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&ncomp[tk.z], c);
}

// ----------------------------------------------------------------------------- null-space vector
// rcnt[root] = rows of the component; runs of equal roots inside a wave are added once
__global__ __launch_bounds__(AI_BLOCK) void k_null_rootcount(const Task* __restrict__ tasks, const int32_t* __restrict__ mode,
                                                             const int32_t* __restrict__ parent, int32_t* __restrict__ rcnt) {
  const Task tk = tasks[blockIdx.x];
  if (mode[tk.z] != 1) return;
  const int lane = threadIdx.x & 63;
  for (int base = tk.x; base < tk.y; base += AI_BLOCK) {
    const int row = base + threadIdx.x;
    const bool live = row < tk.y;
    const int32_t r = live ? parent[row] : -1;
    const int32_t prev = __shfl_up(r, 1, 64);
    const bool head = live && (lane == 0 || prev != r);
    const unsigned long long heads = __ballot(head);
    const unsigned long long lives = __ballot(live);
    if (head) {
      // run length = distance to the next head (or to the end of the live lanes)
      const unsigned long long later = (lane == 63) ? 0ull : (heads >> (lane + 1));
      const int nlive = __popcll(lives);
      const int len = later ? (__ffsll((long long)later)) : (nlive - lane);
      atomicAdd(&rcnt[r], len);
    }
  }
}

// rc[row] = size of the component if row is its root, else 0 (scanned to rank components by first row)
__global__ __launch_bounds__(AI_BLOCK) void k_null_rootvals(const int32_t* __restrict__ parent, const int32_t* __restrict__ rcnt,
                                                            int32_t n, int32_t* __restrict__ rc) {
  const int i = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < n) rc[i] = (parent[i] == i) ? rcnt[i] : 0;
}

// side A = first component + every later component that still ends within the first half of
// the segment's rows; partial volumes of both sides
__global__ __launch_bounds__(AI_BLOCK) void k_null_side(const Task* __restrict__ tasks, const int32_t* __restrict__ mode,
                                                        const int32_t* __restrict__ seg_start, const int32_t* __restrict__ parent,
                                                        const int32_t* __restrict__ rcnt, const int32_t* __restrict__ ex,
                                                        const double* __restrict__ deg, uint8_t* __restrict__ side,
                                                        double* __restrict__ pvolA, double* __restrict__ pvolB) {
  __shared__ double sm[AI_BLOCK / 64];
  const Task tk = tasks[blockIdx.x];
  const int s = tk.z;
  if (mode[s] != 1) {
    if (threadIdx.x == 0) {
      pvolA[blockIdx.x] = 0.0;
      pvolB[blockIdx.x] = 0.0;
    }
    return;
  }
  const int s0 = seg_start[s], ns = seg_start[s + 1] - s0;
  const int exs = ex[s0];
  double va = 0.0, vb = 0.0;
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    const int r = parent[row];
    const int cb = ex[r] - exs;
    const bool inA = (r == s0) || (2 * (int64_t)(cb + rcnt[r]) <= (int64_t)ns);
    side[row] = inA ? 1 : 0;
    if (inA) va += deg[row]; else vb += deg[row];
  }
  const double ta = ai_block_sum(va, sm);
  const double tb = ai_block_sum(vb, sm);
  if (threadIdx.x == 0) {
    pvolA[blockIdx.x] = ta;
    pvolB[blockIdx.x] = tb;
  }
}

__global__ __launch_bounds__(AI_BLOCK) void k_null_vec(const Task* __restrict__ tasks, const int32_t* __restrict__ mode,
                                                       const double* __restrict__ volA, const double* __restrict__ volB,
                                                       const double* __restrict__ deg, const uint8_t* __restrict__ side,
                                                       double* __restrict__ ev) {
  const Task tk = tasks[blockIdx.x];
  const int s = tk.z;
  if (mode[s] != 1) return;
  const double ia = 1.0 / volA[s], ib = 1.0 / volB[s];
  const double rn = 1.0 / sqrt(ia + ib);  // ||D^1/2 (1_A/volA - 1_B/volB)||^2 = 1/volA + 1/volB
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) ev[row] = sqrt(deg[row]) * (side[row] ? ia : -ib) * rn;
}

// ----------------------------------------------------------------------------- Lanczos
// Notation: R_j is the stored (unnormalised, unprojected) j-th vector, g_j = u1 . R_j,
// b_j = ||R_j - g_j u1||, v_j = (R_j - g_j u1) / b_j the Lanczos vector.  T has diagonal
// alpha_j = v_j . M v_j and off-diagonals b_1, b_2, ...

// R_0 = hash(original id); partials of (R.R, u1.R)
__global__ __launch_bounds__(AI_BLOCK) void k_lz_init(const Task* __restrict__ ctasks, const int32_t* __restrict__ cactive,
                                                      const int32_t* __restrict__ orig, const double* __restrict__ u1,
                                                      double* __restrict__ R0, double2* __restrict__ pB) {
  __shared__ double sm[AI_BLOCK / 64];
  if (!cactive[blockIdx.x]) return;
  const Task tk = ctasks[blockIdx.x];
  double nn = 0.0, gg = 0.0;
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    const double r = ai_hash_unit((uint32_t)orig[row]);
    R0[row] = r;
    nn = fma(r, r, nn);
    gg = fma(u1[row], r, gg);
  }
  const double tn = ai_block_sum(nn, sm);
  const double tg = ai_block_sum(gg, sm);
  if (threadIdx.x == 0) pB[blockIdx.x] = make_double2(tn, tg);
}

// THE hot kernel: z = M R_j for every running segment,
//   z_i = sum_k wm_ik R_j[k] + sinv2_i R_j[i]            (M = D^-1/2 (w + I) D^-1/2)
// and the per-block partial of R_j . z.  No per-segment scalar is needed here: with v = (R - g u1)/b
// and M u1 = u1,  alpha = v . M v = (R.z - g^2) / b^2  -- the update kernel finishes it.
// 16 lanes per row (neighbour counts ~30-40) read 64-B / 128-B runs of col / wm; each lane group
// keeps AI_ROW_ILP rows in flight so that the dependent chain rowptr -> col -> gather is overlapped
// four deep; gathers of R_j are served by L2 / MALL.
template <int LPR, int ILP>
__device__ __forceinline__ void spmv_body(int t, const Task* __restrict__ ftasks, const int32_t* __restrict__ factive,
                                          const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                          const double* __restrict__ wm, const double* __restrict__ sinv2,
                                          const double* __restrict__ Rj, double* __restrict__ Z, double* __restrict__ pA,
                                          double* sm) {
  const int act = factive[t];
  const Task tk = ftasks[t];  // independent of the flag: both loads are in flight together
  if (!act) return;
  const int l = threadIdx.x & (LPR - 1), r = threadIdx.x / LPR;
  constexpr int GROUPS = AI_BLOCK / LPR;
  int p0[ILP], p1[ILP];
  double sum[ILP], ri[ILP], s2[ILP];
  int len = 0;
#pragma unroll
  for (int u = 0; u < ILP; ++u) {
    const int row = tk.x + r + u * GROUPS;
    const bool ok = row < tk.y;
    p0[u] = ok ? rowptr[row] : 0;
    p1[u] = ok ? rowptr[row + 1] : 0;
    // the diagonal "+ I" term needs only the row id: issue these loads before the dependent chain
    ri[u] = (ok && l == 0) ? Rj[row] : 0.0;
    s2[u] = (ok && l == 0) ? sinv2[row] : 0.0;
    sum[u] = 0.0;
  }
#pragma unroll
  for (int u = 0; u < ILP; ++u) len = max(len, p1[u] - p0[u]);
  for (int k = l; k < len; k += LPR) {
    int c[ILP];
    double w[ILP];
#pragma unroll
    for (int u = 0; u < ILP; ++u) {
      const int p = p0[u] + k;
      const bool ok = p < p1[u];
      c[u] = ok ? col[p] : -1;
      w[u] = ok ? wm[p] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < ILP; ++u)
      if (c[u] >= 0) sum[u] = fma(w[u], Rj[c[u]], sum[u]);
  }
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < ILP; ++u) {
    double sg = sum[u];
    static_assert(LPR == 16, "the row reduction uses the 16-lane DPP row");
    sg = ai_group16_sum(sg);
    const int row = tk.x + r + u * GROUPS;
    if (l == 0 && row < tk.y) {
      const double z = fma(s2[u], ri[u], sg);
      Z[row] = z;
      acc = fma(ri[u], z, acc);
    }
  }
  const double tot = ai_block_sum(acc, sm);
  if (threadIdx.x == 0) pA[t] = tot;
}

template <int LPR, int ILP>
__global__ __launch_bounds__(AI_BLOCK) void k_lz_spmv_t(const Task* __restrict__ ftasks, const int32_t* __restrict__ factive, int ntask,
                                                      const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                      const double* __restrict__ wm, const double* __restrict__ sinv2,
                                                      const double* __restrict__ Rj, double* __restrict__ Z,
                                                      double* __restrict__ pA) {
  __shared__ double sm[AI_BLOCK / 64];
  spmv_body<LPR, ILP>(ai_xcd_task(blockIdx.x, ntask), ftasks, factive, rowptr, col, wm, sinv2, Rj, Z, pA, sm);
}

// ---- staged gather (the default SpMV): the 8-byte gathers of R_j, not the streamed bytes, bound the
// plain kernel (DESIGN.md section 5).  The ~1200 entries of a 32-row task touch only ~150-300 DISTINCT
// columns (consecutive Morton-ordered rows share their 27 neighbour cells), so once per level every
// Lanczos task gets its sorted distinct-column list `ucol` and every entry a 16-bit index into it;
// a step then gathers each distinct R_j value ONCE into LDS (coalesced runs) and the per-entry
// gather becomes an LDS read.  Sums are formed in exactly the order of the plain kernel.
#define AI_SPMV_PF 4         // rounds of 16 entries per row whose loads are in flight before the barrier

__global__ __launch_bounds__(AI_BLOCK) void k_lz_encode(const Task* __restrict__ ftasks, const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col, int32_t pool_cap,
                                                        int32_t* __restrict__ pool_ctr, int32_t* __restrict__ ucol,
                                                        uint16_t* __restrict__ lidx, TaskEnc* __restrict__ enc) {
  __shared__ int32_t sk[AI_ENC_MAXNNZ];
  __shared__ int32_t uq[AI_ENC_XCAP];
  __shared__ int32_t wsum[AI_BLOCK / 64];
  __shared__ int32_t s_off;
  const Task tk = ftasks[blockIdx.x];
  const int p0 = rowptr[tk.x], cnt = rowptr[tk.y] - p0;
  if (cnt > AI_ENC_MAXNNZ || cnt <= 0) {
    if (threadIdx.x == 0) enc[blockIdx.x] = TaskEnc{0, -1};
    return;
  }
  int n = 64;
  while (n < cnt) n <<= 1;
  for (int i = threadIdx.x; i < n; i += AI_BLOCK) sk[i] = (i < cnt) ? col[p0 + i] : 0x7fffffff;
  __syncthreads();
  // bitonic sort of n (a power of two) keys in LDS
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < (n >> 1); i += AI_BLOCK) {
        const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
        const int32_t a = sk[lo], b = sk[hi];
        const bool up = (lo & k) == 0;
        if ((a > b) == up) {
          sk[lo] = b;
          sk[hi] = a;
        }
      }
      __syncthreads();
    }
  // distinct values: thread t owns the sorted positions [t * per, (t + 1) * per)
  const int per = n / AI_BLOCK > 0 ? n / AI_BLOCK : 1;
  int heads = 0;
  for (int q = 0; q < per; ++q) {
    const int i = threadIdx.x * per + q;
    if (i < cnt && (i == 0 || sk[i] != sk[i - 1])) ++heads;
  }
  int incl = heads;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if ((threadIdx.x & 63) >= o) incl += v;
  }
  if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
  __syncthreads();
  int base = incl - heads, total = 0;
#pragma unroll
  for (int w = 0; w < AI_BLOCK / 64; ++w) {
    if (w < (int)(threadIdx.x >> 6)) base += wsum[w];
    total += wsum[w];
  }
  if (total > AI_ENC_XCAP) {
    if (threadIdx.x == 0) enc[blockIdx.x] = TaskEnc{0, -1};
    return;
  }
  for (int q = 0; q < per; ++q) {
    const int i = threadIdx.x * per + q;
    if (i < cnt && (i == 0 || sk[i] != sk[i - 1])) uq[base++] = sk[i];
  }
  if (threadIdx.x == 0) s_off = atomicAdd(pool_ctr, total);
  __syncthreads();
  const int off = s_off;
  if (off + total > pool_cap) {  // pool exhausted (never with the default sizing): plain gather for this task
    if (threadIdx.x == 0) enc[blockIdx.x] = TaskEnc{0, -1};
    return;
  }
  for (int i = threadIdx.x; i < total; i += AI_BLOCK) ucol[off + i] = uq[i];
  for (int e = threadIdx.x; e < cnt; e += AI_BLOCK) {
    const int32_t c = col[p0 + e];
    int lo = 0, hi = total - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (uq[mid] < c) lo = mid + 1; else hi = mid;
    }
    lidx[p0 + e] = (uint16_t)lo;
  }
  if (threadIdx.x == 0) enc[blockIdx.x] = TaskEnc{off, total};
}

// Entries are taken four at a time: lane l of a row's 16 owns the ALIGNED quads (p0 >> 2) + l, + 16, ... of the
// entry stream -- one 8-byte load of four 2-byte indices and two 16-byte loads of four weights per quad instead of four
// 2-byte and four 8-byte loads (the kernel is bound by memory requests, not bytes: section 5) -- and masks what lies
// outside [p0, p1) (a neighbouring row's entries: weight 0, index 0).  16 quads cover rows of up to 61 entries in one round.
// lidx and wm carry 4 entries of slack at the end.  The sum of a row is: per lane its (up to) four products in entry order,
// then the 16-lane tree -- fixed for a given layout of the level's entry stream.
template <int ILP>
__global__ __launch_bounds__(AI_BLOCK) void k_lz_spmv_q(const Task* __restrict__ ftasks, const int32_t* __restrict__ factive, int ntask,
                                                        const TaskEnc* __restrict__ enc, const int32_t* __restrict__ ucol,
                                                        const uint16_t* __restrict__ lidx, const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col, const double* __restrict__ wm,
                                                        const double* __restrict__ sinv2, const double* __restrict__ Rj,
                                                        double* __restrict__ Z, double* __restrict__ pA,
                                                        unsigned long long* __restrict__ tstamp) {
  constexpr int LPR = 16;
  __shared__ double sm[AI_BLOCK / 64];
  __shared__ double xs[AI_ENC_XCAP];
  struct Stamp {
    unsigned long long* ts;
    __device__ explicit Stamp(unsigned long long* p) : ts(p) {
      if (ts && threadIdx.x == 0) ts[2 * blockIdx.x] = (unsigned long long)wall_clock64();
    }
    __device__ ~Stamp() {
      if (ts && threadIdx.x == 0) ts[2 * blockIdx.x + 1] = (unsigned long long)wall_clock64();
    }
  } stamp(tstamp);
  const int t = ai_xcd_task(blockIdx.x, ntask);
  const int act = factive[t];
  const Task tk = ftasks[t];
  const TaskEnc en = enc[t];
  if (!act) return;
  if (en.ucnt < 0) {
    spmv_body<LPR, ILP>(t, ftasks, factive, rowptr, col, wm, sinv2, Rj, Z, pA, sm);
    return;
  }
  for (int i = threadIdx.x; i < en.ucnt; i += AI_BLOCK) xs[i] = Rj[ucol[en.uoff + i]];
  const int l = threadIdx.x & (LPR - 1), r = threadIdx.x / LPR;
  constexpr int GROUPS = AI_BLOCK / LPR;
  const uint2* __restrict__ lidx4 = reinterpret_cast<const uint2*>(lidx);
  const double2* __restrict__ wm2 = reinterpret_cast<const double2*>(wm);
  int p0[ILP], p1[ILP];
  double sum[ILP], ri[ILP], s2[ILP];
  int maxq = 0;
#pragma unroll
  for (int u = 0; u < ILP; ++u) {
    const int row = tk.x + r + u * GROUPS;
    const bool ok = row < tk.y;
    p0[u] = ok ? rowptr[row] : 0;
    p1[u] = ok ? rowptr[row + 1] : 0;
    ri[u] = (ok && l == 0) ? Rj[row] : 0.0;
    s2[u] = (ok && l == 0) ? sinv2[row] : 0.0;
    sum[u] = 0.0;
    maxq = max(maxq, ((p1[u] + 3) >> 2) - (p0[u] >> 2));
  }
  // first round: loads in flight before the barrier (they do not depend on xs)
  uint2 iq[ILP];
  double2 wa[ILP], wb[ILP];
#pragma unroll
  for (int u = 0; u < ILP; ++u) {
    const int q = (p0[u] >> 2) + l;
    const bool ok = 4 * q < p1[u];
    iq[u] = ok ? lidx4[q] : make_uint2(0u, 0u);
    wa[u] = ok ? wm2[2 * q] : make_double2(0.0, 0.0);
    wb[u] = ok ? wm2[2 * q + 1] : make_double2(0.0, 0.0);
  }
  __syncthreads();
  auto quad = [&](int u, int q, uint2 ix, double2 a, double2 b) {
    const int e = 4 * q;
    const bool v0 = e >= p0[u] && e < p1[u], v1 = e + 1 >= p0[u] && e + 1 < p1[u];
    const bool v2 = e + 2 >= p0[u] && e + 2 < p1[u], v3 = e + 3 >= p0[u] && e + 3 < p1[u];
    const unsigned i0 = v0 ? (ix.x & 0xFFFFu) : 0u, i1 = v1 ? (ix.x >> 16) : 0u;
    const unsigned i2 = v2 ? (ix.y & 0xFFFFu) : 0u, i3 = v3 ? (ix.y >> 16) : 0u;
    const double x0 = xs[i0], x1 = xs[i1], x2 = xs[i2], x3 = xs[i3];
    double sacc = sum[u];
    sacc = fma(v0 ? a.x : 0.0, x0, sacc);
    sacc = fma(v1 ? a.y : 0.0, x1, sacc);
    sacc = fma(v2 ? b.x : 0.0, x2, sacc);
    sacc = fma(v3 ? b.y : 0.0, x3, sacc);
    sum[u] = sacc;
  };
#pragma unroll
  for (int u = 0; u < ILP; ++u) quad(u, (p0[u] >> 2) + l, iq[u], wa[u], wb[u]);
  for (int k = LPR; k < maxq; k += LPR) {  // rows of more than ~61 entries: one more round at a time
#pragma unroll
    for (int u = 0; u < ILP; ++u) {
      const int q = (p0[u] >> 2) + l + k;
      if (4 * q < p1[u]) quad(u, q, lidx4[q], wm2[2 * q], wm2[2 * q + 1]);
    }
  }
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < ILP; ++u) {
    const double sg = ai_group16_sum(sum[u]);
    const int row = tk.x + r + u * GROUPS;
    if (l == 0 && row < tk.y) {
      const double z = fma(s2[u], ri[u], sg);
      Z[row] = z;
      acc = fma(ri[u], z, acc);
    }
  }
  const double tot = ai_block_sum(acc, sm);
  if (threadIdx.x == 0) pA[t] = tot;
}

struct LzSeg {
  int32_t* frozen;      // [S]
  int32_t* m;           // [S] size of T at freeze
  double* alpha_hist;   // [S][mcap]
  double* b_hist;       // [S][mcap + 1]
  double* g_hist;       // [S][mcap + 1]
  int32_t* factive;     // fine-task activity flags
  int32_t* cactive;     // coarse-task activity flags
  int mcap;
};

__device__ __forceinline__ void lz_freeze(const LzSeg& L, int s, int m, TaskRange rg, int lane, int nlanes) {
  if (lane == 0) {
    L.frozen[s] = 1;
    L.m[s] = m;
  }
  for (int t = rg.x + lane; t < rg.y; t += nlanes) L.factive[t] = 0;
  for (int t = rg.z + lane; t < rg.w; t += nlanes) L.cactive[t] = 0;
}

// Step j, second launch: every block of a segment re-derives the segment's scalars from the
// per-block partials in the same fixed order (so all blocks agree bit for bit):
//   g_j, b_j from the partials of R_j;  alpha_j = (R_j . z - g_j^2) / b_j^2;
// then  R_{j+1} = y - alpha_j v_j - b_j v_{j-1},  y = (z - g_j u1) / b_j,
// and the partials (R.R, u1.R) of R_{j+1}.  The segment's first block records alpha_j, b_j, g_j.
// A vanishing b_j (Krylov space exhausted) freezes the segment with T of size j.
__device__ __forceinline__ void update_body(int bid, const Task* __restrict__ ctasks, const TaskRange* __restrict__ cranges,
                                            const LzSeg& L, int j, const double* __restrict__ pA,
                                            const double2* __restrict__ pBcur, double2* __restrict__ pBnext,
                                            const double* __restrict__ u1, const double* __restrict__ Z,
                                            const double* __restrict__ Rj, const double* __restrict__ Rjm1,
                                            double* __restrict__ Rnext, double (*sm3)[AI_BLOCK / 64]) {
  constexpr int RPT = AI_COARSE_ROWS / AI_BLOCK;  // rows per thread
  const int act = L.cactive[bid];
  const Task tk = ctasks[bid];
  const TaskRange rg = cranges[bid];
  if (!act) return;
  const int s = tk.z;
  if (j >= (tk.w >> 1)) return;  // the segment's Krylov space is exhausted at its own dimension
  // row data does not depend on the segment scalars: get it moving before the reductions
  double zr[RPT], rr[RPT], rm[RPT], ur[RPT];
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int row = tk.x + threadIdx.x + q * AI_BLOCK;
    const bool ok = row < tk.y;
    zr[q] = ok ? Z[row] : 0.0;
    rr[q] = ok ? Rj[row] : 0.0;
    rm[q] = (ok && j > 0) ? Rjm1[row] : 0.0;
    ur[q] = ok ? u1[row] : 0.0;
  }
  // previous step's scalars come from the history (written by an earlier launch)
  double gp = 0.0, rbp = 0.0;
  if (j > 0) {
    gp = L.g_hist[(size_t)s * (L.mcap + 1) + j - 1];
    rbp = 1.0 / L.b_hist[(size_t)s * (L.mcap + 1) + j - 1];
  }
  double a = 0.0, nn = 0.0, gg = 0.0;
  for (int t = rg.x + threadIdx.x; t < rg.y; t += AI_BLOCK) a += pA[t];
  for (int t = rg.z + threadIdx.x; t < rg.w; t += AI_BLOCK) {
    const double2 v = pBcur[t];
    nn += v.x;
    gg += v.y;
  }
  // three block sums behind one pair of barriers; every thread adds the wave partials in the same order
  a = ai_wave_sum(a);
  nn = ai_wave_sum(nn);
  gg = ai_wave_sum(gg);
  const int w = threadIdx.x >> 6, ln = threadIdx.x & 63;
  if (ln == 0) {
    sm3[0][w] = a;
    sm3[1][w] = nn;
    sm3[2][w] = gg;
  }
  __syncthreads();
  a = 0.0;
  nn = 0.0;
  double g = 0.0;
#pragma unroll
  for (int i = 0; i < AI_BLOCK / 64; ++i) {
    a += sm3[0][i];
    nn += sm3[1][i];
    g += sm3[2][i];
  }
  __syncthreads();
  const double b = sqrt(fmax(nn - g * g, 0.0));  // ||R_j - g u1||, u1 has unit norm
  if (j > 0 && !(b > 1e-14)) {
    if (tk.w & 1) lz_freeze(L, s, j, rg, threadIdx.x, AI_BLOCK);
    return;
  }
  const double rb = 1.0 / b;
  const double al = rb * rb * (a - g * g);
  if ((tk.w & 1) && threadIdx.x == 0) {
    L.alpha_hist[(size_t)s * L.mcap + j] = al;
    L.b_hist[(size_t)s * (L.mcap + 1) + j] = b;
    L.g_hist[(size_t)s * (L.mcap + 1) + j] = g;
  }
  double n2 = 0.0, g2 = 0.0;
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int row = tk.x + threadIdx.x + q * AI_BLOCK;
    if (row < tk.y) {
      const double ui = ur[q];
      const double y = (zr[q] - g * ui) * rb;
      const double v = (rr[q] - g * ui) * rb;
      const double vm = (j > 0) ? (rm[q] - gp * ui) * rbp : 0.0;
      const double rnew = y - al * v - b * vm;
      Rnext[row] = rnew;
      n2 = fma(rnew, rnew, n2);
      g2 = fma(ui, rnew, g2);
    }
  }
  n2 = ai_wave_sum(n2);
  g2 = ai_wave_sum(g2);
  if (ln == 0) {
    sm3[0][w] = n2;
    sm3[1][w] = g2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tn = 0.0, tg = 0.0;
#pragma unroll
    for (int i = 0; i < AI_BLOCK / 64; ++i) {
      tn += sm3[0][i];
      tg += sm3[1][i];
    }
    pBnext[bid] = make_double2(tn, tg);
  }
}

__global__ __launch_bounds__(AI_BLOCK) void k_lz_update(const Task* __restrict__ ctasks, const TaskRange* __restrict__ cranges,
                                                        LzSeg L, int j, const double* __restrict__ pA,
                                                        const double2* __restrict__ pBcur, double2* __restrict__ pBnext,
                                                        const double* __restrict__ u1, const double* __restrict__ Z,
                                                        const double* __restrict__ Rj, const double* __restrict__ Rjm1,
                                                        double* __restrict__ Rnext) {
  __shared__ double sm3[3][AI_BLOCK / 64];
  update_body(blockIdx.x, ctasks, cranges, L, j, pA, pBcur, pBnext, u1, Z, Rj, Rjm1, Rnext, sm3);
}

// b_m = ||R_m - g_m u1|| per running segment from the update kernel's partials (main stream: the
// partials are overwritten two steps later, the check itself runs on the side stream)
__global__ __launch_bounds__(64) void k_lz_bnew(const TaskRange* __restrict__ seg_range, const int32_t* __restrict__ mode,
                                                const int32_t* __restrict__ frozen, const double2* __restrict__ pB,
                                                double* __restrict__ bnew_out) {
  const int s = blockIdx.x;
  if (mode[s] != 0 || frozen[s]) return;
  const TaskRange rg = seg_range[s];
  double nn = 0.0, gg = 0.0;
  for (int t = rg.z + threadIdx.x; t < rg.w; t += 64) {
    const double2 v = pB[t];
    nn += v.x;
    gg += v.y;
  }
  nn = ai_wave_sum(nn);
  gg = ai_wave_sum(gg);
  if (threadIdx.x == 0) bnew_out[s] = sqrt(fmax(nn - gg * gg, 0.0));
}

// Convergence check after step j (m = j + 1 rows of T), one 256-thread block per running segment, on
// the side stream: top eigenvalue of T_m by 256-way multisection (every thread one Sturm count, the
// four waves on the CU's four SIMDs); |s_m| by the recurrence from the bottom row upwards (the growing,
// hence stable, direction); residual = b_m |s_m|.  Freezes the segment when residual <= tol or T has
// reached the segment's dimension / the step cap.  slot[0] counts the segments still running; work[]
// accumulates rows and stored entries the SpMV kernel processed since the last check.  Reads only
// history entries [0, m), which later steps never touch.
__global__ __launch_bounds__(AI_CHECK_THREADS) void k_lz_check(const int32_t* __restrict__ seg_start, const TaskRange* __restrict__ seg_range,
                                                               const int32_t* __restrict__ mode, LzSeg L, const double* __restrict__ bnew_in,
                                                               int m, double tol, int max_iter, int steps_since,
                                                               const int32_t* __restrict__ rowptr, double* __restrict__ theta_out,
                                                               double* __restrict__ resid_out, int32_t* __restrict__ slot,
                                                               unsigned long long* __restrict__ work, int with_rb) {
  constexpr int NT = AI_CHECK_THREADS, NW = NT / 64;
  __shared__ double smm[2][NW];
  __shared__ int sfirst[2][NW];
  const int s = blockIdx.x;
  // The per-segment records of a level live in buffers that the next level rewrites, and this kernel runs on the side stream:
  // they are loaded once, by one thread, with agent-scope loads and handed to the block through LDS (block-uniform plain loads
  // become scalar loads through the scalar cache, one per wave; ai_flow_kernels.inc::fk_check tells what that cost there).
  __shared__ int32_t sh_i[8];
  __shared__ double sh_d[3];
  if (threadIdx.x == 0) {
    sh_i[0] = __hip_atomic_load(const_cast<int32_t*>(&mode[s]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh_i[1] = __hip_atomic_load(&L.frozen[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh_i[2] = __hip_atomic_load(const_cast<int32_t*>(&seg_start[s]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh_i[3] = __hip_atomic_load(const_cast<int32_t*>(&seg_start[s + 1]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int32_t* rw = reinterpret_cast<const int32_t*>(&seg_range[s]);
    static_assert(sizeof(TaskRange) == 4 * sizeof(int32_t), "TaskRange is four ints");
    for (int k = 0; k < 4; ++k) sh_i[4 + k] = __hip_atomic_load(const_cast<int32_t*>(rw + k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh_d[0] = __hip_atomic_load(const_cast<double*>(&bnew_in[s]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh_d[1] = __hip_atomic_load(&theta_out[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh_d[2] = __hip_atomic_load(&resid_out[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (sh_i[0] != 0) return;
  if (sh_i[1]) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ns = sh_i[3] - sh_i[2];
  TaskRange rg;
  {
    int32_t* rw = reinterpret_cast<int32_t*>(&rg);
    for (int k = 0; k < 4; ++k) rw[k] = sh_i[4 + k];
  }
  if (tid == 0) {
    atomicAdd(&work[0], (unsigned long long)ns * (unsigned long long)steps_since);
    atomicAdd(&work[1], (unsigned long long)(rowptr[sh_i[3]] - rowptr[sh_i[2]]) * (unsigned long long)steps_since);
  }
  const double bnew = sh_d[0];
  const double* bh = L.b_hist + (size_t)s * (L.mcap + 1);
  const double* ah = L.alpha_hist + (size_t)s * L.mcap;
  const int cap = min(min(ns - 1, max_iter), L.mcap);
  const bool last = (m >= cap) || !(bnew > 1e-14);
  m = min(m, cap);  // steps launched past the segment's cap did nothing (graph replay works in batches)
  // T_m into LDS: a[0..m), b^2[0..m) (b^2[0] unused) and, when it fits, 1 / b[0..m)
  extern __shared__ double lds[];
  double* la = lds;
  double* lbb = lds + m;
  double* lrb = lds + 2 * m;
  double lo = -1e300, hi = -1e300;  // lambda_max >= max diagonal, <= Gershgorin bound
  for (int i = tid; i < m; i += NT) {
    const double ai = ah[i];
    const double bi = (i > 0) ? bh[i] : 0.0, br = (i + 1 < m) ? bh[i + 1] : 0.0;
    la[i] = ai;
    lbb[i] = bi * bi;
    if (with_rb) lrb[i] = (i > 0) ? 1.0 / bi : 0.0;
    lo = fmax(lo, ai);
    hi = fmax(hi, ai + fabs(bi) + fabs(br));
  }
  for (int o = 32; o > 0; o >>= 1) {
    lo = fmax(lo, __shfl_xor(lo, o, 64));
    hi = fmax(hi, __shfl_xor(hi, o, 64));
  }
  if (lane == 0) {
    smm[0][wv] = lo;
    smm[1][wv] = hi;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    lo = fmax(lo, smm[0][w]);
    hi = fmax(hi, smm[1][w]);
  }
  lo -= 1e-14 * fmax(fabs(lo), 1.0);
  hi += 1e-14 * fmax(fabs(hi), 1.0);
  // index of the first thread of the block whose shift exceeds every eigenvalue (Sturm count m), or -1
  int phase = 0;
  auto first_above = [&](bool mine) -> int {
    const unsigned long long above = __ballot(mine);
    if (lane == 0) sfirst[phase][wv] = above ? wv * 64 + __ffsll((long long)above) - 1 : (1 << 30);
    __syncthreads();
    int j = 1 << 30;
#pragma unroll
    for (int w = 0; w < NW; ++w) j = min(j, sfirst[phase][w]);
    phase ^= 1;  // the next call writes the other row: one barrier per call is enough
    return (j == (1 << 30)) ? -1 : j;
  };
  // Warm start from the previous check of this solve: T grew by rows and columns, so its top
  // eigenvalue did not decrease (interlacing), and it normally lies within the previous residual of
  // the previous value.  One round probes the ladder theta' + resid' * 2^j; the lowest rung above
  // every eigenvalue closes the bracket, the rung below it opens it.
  const double tprev = sh_d[1], rprev = sh_d[2];
  if (tprev > 0.0 && rprev > 0.0) {
    const double hi_g = hi, eps = 1e-15 * fmax(fabs(tprev), 1.0);
    const double lo_w = fmax(lo, tprev - 1e-14 * fmax(fabs(tprev), 1.0));
    const double x = fmin(hi_g, tprev + ldexp(rprev, tid) + eps);
    const int j0 = first_above(sturm_lt(la, lbb, m, x) == m);
    lo = lo_w;
    if (j0 >= 0) {
      hi = fmin(hi_g, tprev + ldexp(rprev, j0) + eps);
      if (j0 > 0) lo = fmax(lo_w, fmin(hi_g, tprev + ldexp(rprev, j0 - 1) + eps));
    }
  }
  for (int round = 0; round < 12; ++round) {
    // 5e-14 relative is enough: the residual estimate below needs the eigenvalue only to a small
    // fraction of T's top gap, and the host refines it inside a +-1e-13 bracket (tridiag_top)
    if (hi - lo <= 5e-14 * fmax(fabs(hi), 1e-300)) break;  // block-uniform
    const double w = (hi - lo) * (1.0 / (NT + 1));
    const double x = lo + (tid + 1) * w;
    const int j0 = first_above(sturm_lt(la, lbb, m, x) == m);
    if (j0 < 0) {
      lo = lo + (double)NT * w;
    } else {
      hi = lo + (j0 + 1) * w;
      lo = lo + j0 * w;
    }
  }
  if (wv != 0) return;
  const double theta = 0.5 * (lo + hi);
  // ---- |s_m| / ||s||: s_m = 1 at the start; `scale` follows the rescalings
  double sk1 = 0.0, sk = 1.0, sumsq = 1.0, scale = 1.0;  // s_{k+1}, s_k (every lane computes the same)
#pragma unroll 8
  for (int k = m - 1; k >= 1; --k) {
    const double bu = (k + 1 < m) ? bh[k + 1] : 0.0;
    const double num = (theta - la[k]) * sk - bu * sk1;
    const double sm1 = with_rb ? num * lrb[k] : num / bh[k];
    sk1 = sk;
    sk = sm1;
    sumsq += sk * sk;
    if (sumsq > 1e200) {  // only ratios matter
      sk *= 1e-100;
      sk1 *= 1e-100;
      sumsq *= 1e-200;
      scale *= 1e-100;
    }
  }
  const double resid = bnew * scale / sqrt(sumsq);
  if (lane == 0) {
    theta_out[s] = theta;
    resid_out[s] = resid;
  }
  if (resid <= tol || last) {
    lz_freeze(L, s, m, rg, lane, 64);
  } else if (lane == 0) {
    atomicAdd(slot, 1);
  }
}

// ev = sum_j coef_j R_j + cu u1 for the rows of Lanczos segments (one slab of vectors per launch)
__global__ __launch_bounds__(AI_BLOCK) void k_ritz(const Task* __restrict__ ctasks, const int32_t* __restrict__ mode,
                                                   const int32_t* __restrict__ seg_m, const double* __restrict__ coef, int mcap,
                                                   const double* __restrict__ cu, const double* __restrict__ u1,
                                                   const double* __restrict__ slab, size_t stride, int j0, int nvec, int first,
                                                   double* __restrict__ ev) {
  const Task tk = ctasks[blockIdx.x];
  const int s = tk.z;
  if (mode[s] != 0) return;
  const int m = seg_m[s];
  const int jn = min(nvec, m - j0);
  if (jn <= 0 && !first) return;
  const double* cs = coef + (size_t)s * mcap + j0;
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    double acc = first ? cu[s] * u1[row] : ev[row];
#pragma unroll 8
    for (int j = 0; j < jn; ++j) acc = fma(cs[j], slab[(size_t)j * stride + row], acc);  // same order, eight loads in flight
    ev[row] = acc;
  }
}

// ----------------------------------------------------------------------------- full re-orthogonalisation (ai_eigs_smallest)
// For k > 2 eigenpairs the three-term recurrence alone is not enough: once a Ritz pair has
// converged, copies of it re-enter.  Each new vector r = R_{j+1} is therefore orthogonalised
// against ALL kept Lanczos vectors v_i = (R_i - g_i u1) / b_i, i <= j, before it is normalised:
//   c_i = v_i . r = (R_i . r - g_i (u1 . r)) / b_i,   r <- r - sum_i c_i v_i.
#define FRO_CH 16

// part[task][i] = sum over the task's rows of R_i[row] * r[row], 16 vectors per block
__global__ __launch_bounds__(AI_BLOCK) void k_fro_dots(const Task* __restrict__ ctasks, const double* __restrict__ r,
                                                       double* const* __restrict__ slabs, size_t stride, int nvec,
                                                       double* __restrict__ part, int pitch) {
  constexpr int RPT = AI_COARSE_ROWS / AI_BLOCK;
  __shared__ double sm[FRO_CH][AI_BLOCK / 64];
  const Task tk = ctasks[blockIdx.x];
  const int i0 = blockIdx.y * FRO_CH;
  double rv[RPT];
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int row = tk.x + threadIdx.x + q * AI_BLOCK;
    rv[q] = (row < tk.y) ? r[row] : 0.0;
  }
  double acc[FRO_CH];
#pragma unroll
  for (int ii = 0; ii < FRO_CH; ++ii) {
    acc[ii] = 0.0;
    const int i = i0 + ii;
    if (i < nvec) {
      const double* Ri = slabs[i / AI_SLAB_VECS] + (size_t)(i % AI_SLAB_VECS) * stride;
#pragma unroll
      for (int q = 0; q < RPT; ++q) {
        const int row = tk.x + threadIdx.x + q * AI_BLOCK;
        if (row < tk.y) acc[ii] = fma(rv[q], Ri[row], acc[ii]);
      }
    }
  }
  const int w = threadIdx.x >> 6, ln = threadIdx.x & 63;
#pragma unroll
  for (int ii = 0; ii < FRO_CH; ++ii) {
    const double v = ai_wave_sum(acc[ii]);
    if (ln == 0) sm[ii][w] = v;
  }
  __syncthreads();
  if (threadIdx.x < FRO_CH && i0 + (int)threadIdx.x < nvec) {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < AI_BLOCK / 64; ++i) t += sm[threadIdx.x][i];
    part[(size_t)blockIdx.x * pitch + i0 + threadIdx.x] = t;
  }
}

// coef_i = c_i / b_i and cu = sum_i c_i g_i / b_i (one block; fixed summation orders)
__global__ __launch_bounds__(AI_BLOCK) void k_fro_coef(int ntask, const double* __restrict__ part, int pitch, int nvec,
                                                       const double* __restrict__ g_hist, const double* __restrict__ b_hist,
                                                       const double2* __restrict__ pBr, double* __restrict__ coef,
                                                       double* __restrict__ cu) {
  __shared__ double sm[AI_BLOCK / 64];
  double gq = 0.0;
  for (int t = threadIdx.x; t < ntask; t += AI_BLOCK) gq += pBr[t].y;
  gq = ai_block_sum(gq, sm);  // u1 . r
  double cuacc = 0.0;
  for (int i = threadIdx.x; i < nvec; i += AI_BLOCK) {
    double d = 0.0;
    for (int t = 0; t < ntask; ++t) d += part[(size_t)t * pitch + i];
    const double rb = 1.0 / b_hist[i];
    const double c = (d - g_hist[i] * gq) * rb;
    coef[i] = c * rb;
    cuacc += c * g_hist[i] * rb;
  }
  const double tot = ai_block_sum(cuacc, sm);
  if (threadIdx.x == 0) cu[0] = tot;
}

// r <- r - sum_i coef_i R_i + cu u1; new partials (r.r, u1.r)
__global__ __launch_bounds__(AI_BLOCK) void k_fro_apply(const Task* __restrict__ ctasks, double* __restrict__ r,
                                                        double* const* __restrict__ slabs, size_t stride, int nvec,
                                                        const double* __restrict__ coef, const double* __restrict__ cu,
                                                        const double* __restrict__ u1, double2* __restrict__ pBout) {
  constexpr int RPT = AI_COARSE_ROWS / AI_BLOCK;
  __shared__ double sm[AI_BLOCK / 64];
  const Task tk = ctasks[blockIdx.x];
  double rv[RPT];
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int row = tk.x + threadIdx.x + q * AI_BLOCK;
    rv[q] = (row < tk.y) ? r[row] : 0.0;
  }
  for (int i = 0; i < nvec; ++i) {
    const double* Ri = slabs[i / AI_SLAB_VECS] + (size_t)(i % AI_SLAB_VECS) * stride;
    const double c = coef[i];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      const int row = tk.x + threadIdx.x + q * AI_BLOCK;
      if (row < tk.y) rv[q] = fma(-c, Ri[row], rv[q]);
    }
  }
  const double cuv = cu[0];
  double nn = 0.0, gg = 0.0;
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int row = tk.x + threadIdx.x + q * AI_BLOCK;
    if (row < tk.y) {
      const double ui = u1[row];
      const double v = fma(cuv, ui, rv[q]);
      r[row] = v;
      nn = fma(v, v, nn);
      gg = fma(ui, v, gg);
    }
  }
  const double tn = ai_block_sum(nn, sm);
  const double tg = ai_block_sum(gg, sm);
  if (threadIdx.x == 0) pBout[blockIdx.x] = make_double2(tn, tg);
}

// out[i][row] (+)= sum_j coefT[j][i] R_j[row] for up to 64 Ritz vectors at once, one slab per launch;
// the first launch starts from cu_i u1[row]
#define RITZ_MAXK 64
__global__ __launch_bounds__(AI_BLOCK) void k_ritz_multi(const Task* __restrict__ ctasks, int kv, const double* __restrict__ coefT,
                                                         const double* __restrict__ cuv, const double* __restrict__ u1,
                                                         const double* __restrict__ slab, size_t stride, int j0, int nvec, int m,
                                                         int first, double* __restrict__ out, size_t out_stride) {
  const Task tk = ctasks[blockIdx.x];
  const int jn = min(nvec, m - j0);
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    double acc[RITZ_MAXK];
    const double ui = u1[row];
#pragma unroll
    for (int i = 0; i < RITZ_MAXK; ++i) acc[i] = (i < kv) ? (first ? cuv[i] * ui : out[(size_t)i * out_stride + row]) : 0.0;
    for (int j = 0; j < jn; ++j) {
      const double v = slab[(size_t)j * stride + row];
      const double* cj = coefT + (size_t)(j0 + j) * RITZ_MAXK;
#pragma unroll
      for (int i = 0; i < RITZ_MAXK; ++i) acc[i] = fma(cj[i], v, acc[i]);
    }
#pragma unroll
    for (int i = 0; i < RITZ_MAXK; ++i)
      if (i < kv) out[(size_t)i * out_stride + row] = acc[i];
  }
}

// ----------------------------------------------------------------------------- threshold sweep
__global__ __launch_bounds__(AI_BLOCK) void k_minmax(const Task* __restrict__ ctasks, const int32_t* __restrict__ mode,
                                                     const double* __restrict__ ev, const int32_t* __restrict__ orig,
                                                     MinMaxPart* __restrict__ part) {
  const Task tk = ctasks[blockIdx.x];
  if (mode && mode[tk.z] != 0) return;  // a disconnected segment has no eigenvector: it is split by components
  minmax_body(tk, ev, orig, part);
}

// Per segment: scale, np.allclose test and the 10 thresholds (minmax_final_body)
__global__ void k_minmax_final(const int32_t* __restrict__ ctask0, const int32_t* __restrict__ mode,
                               const MinMaxPart* __restrict__ part, int S, int raw, double* __restrict__ scale,
                               int32_t* __restrict__ nosplit, double* __restrict__ thr) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S) return;
  if (mode && mode[s] != 0) {
    scale[s] = 1.0;
    nosplit[s] = 1;
    return;
  }
  minmax_final_body(part, ctask0[s], ctask0[s + 1], raw, s, scale, nosplit, thr);
}

// bin_i = number of thresholds strictly below ev_i: mask_k(i) = (ev_i > t_k) = (k < bin_i)
__global__ __launch_bounds__(AI_BLOCK) void k_bin(const Task* __restrict__ ctasks, const int32_t* __restrict__ nosplit,
                                                  const double* __restrict__ scale, const double* __restrict__ thr,
                                                  const double* __restrict__ ev, uint8_t* __restrict__ bin) {
  bin_body(ctasks, nosplit, scale, thr, ev, bin);
}

// All 10 cut costs in one pass over the edges (sweep_body)
__global__ __launch_bounds__(AI_BLOCK) void k_sweep(const Task* __restrict__ ftasks, const int32_t* __restrict__ nosplit,
                                                    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                    const double* __restrict__ wraw, const double* __restrict__ deg,
                                                    const uint8_t* __restrict__ bin, double* __restrict__ part) {
  sweep_body(ftasks, nosplit, CsrGraph{rowptr, col, wraw}, deg, bin, part);
}

// Per segment: the 10 costs, the winning threshold, split iff mcut < T (sweep_final_body); one block per segment
__global__ __launch_bounds__(AI_BLOCK) void k_sweep_final(const int32_t* __restrict__ ftask0, const int32_t* __restrict__ nosplit,
                                                          const double* __restrict__ part, double T, double* __restrict__ costs,
                                                          int32_t* __restrict__ kstar, int32_t* __restrict__ split,
                                                          int32_t* __restrict__ ntrue, double* __restrict__ mcut_out) {
  const int s = blockIdx.x;
  if (nosplit[s]) {
    if (threadIdx.x == 0) {
      split[s] = 0;
      kstar[s] = 0;
      ntrue[s] = 0;
      mcut_out[s] = INFINITY;
    }
    if (threadIdx.x < AI_NUM_CUTS) costs[s * AI_NUM_CUTS + threadIdx.x] = NAN;
    return;
  }
  __builtin_assume(costs != nullptr);  // the Solver always wants them; with the body's test left in, this kernel takes 240 VGPRs for 90
  sweep_final_body(part, ftask0[s], ftask0[s + 1], T, s, costs, kstar, split, ntrue, mcut_out);
}

// ----------------------------------------------------------------------------- partition + rebuild
__global__ __launch_bounds__(AI_BLOCK) void k_split_flags(const Task* __restrict__ ctasks, const int32_t* __restrict__ split,
                                                          const int32_t* __restrict__ kstar, const uint8_t* __restrict__ bin,
                                                          int32_t* __restrict__ flag) {
  const Task tk = ctasks[blockIdx.x];
  const int sp = split[tk.z], ks = kstar[tk.z];
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) flag[row] = (sp && (int)bin[row] > ks) ? 1 : 0;
}

// Stable partition inside each parent (mask side first, normalized_cut.py:57-59).  Writes the
// caller-order id of every row to its position in the final ordering and the row's index in the
// next level's compact order (-1: the row's segment is finished).
__global__ __launch_bounds__(AI_BLOCK) void k_partition(const Task* __restrict__ ctasks, const int32_t* __restrict__ seg_start,
                                                        const int32_t* __restrict__ seg_gstart, const int32_t* __restrict__ split,
                                                        const int32_t* __restrict__ ntrue, const int32_t* __restrict__ childA,
                                                        const int32_t* __restrict__ childB, const int32_t* __restrict__ flag,
                                                        const int32_t* __restrict__ fscan, const int32_t* __restrict__ orig,
                                                        int32_t* __restrict__ final_order, int32_t* __restrict__ map,
                                                        int32_t* __restrict__ orig_next, const int32_t* __restrict__ multi) {
  const Task tk = ctasks[blockIdx.x];
  const int s = tk.z;
  if (multi[s]) return;  // split by components: k_partition_multi
  const int s0 = seg_start[s], g0 = seg_gstart[s], nt = split[s] ? ntrue[s] : 0;
  const int cA = childA[s], cB = childB[s];
  const int f0 = fscan[s0];
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    const int f = flag[row];
    const int rt = fscan[row] - f0;  // mask-side rows before this one
    const int rf = (row - s0) - rt;  // other-side rows before this one
    const int newpos = f ? rt : nt + rf;
    const int32_t id = orig[row];
    final_order[g0 + newpos] = id;
    int32_t dst = -1;
    if (f) {
      if (cA >= 0) dst = cA + rt;
    } else {
      if (cB >= 0) dst = cB + rf;
    }
    map[row] = dst;
    if (dst >= 0) orig_next[dst] = id;
  }
}


// ---- a disconnected segment is split into ALL its connected components at once (see the file header).
// Component = union-find root = its first row; components keep the order of their first rows, rows keep
// their order inside a component: a stable sort of the rows by root id (segments stay where they are,
// because a root lies inside its segment's row range).

// rc[row] = 1 for the roots of the segments that are split by components
__global__ __launch_bounds__(AI_BLOCK) void k_comp_rootflag(const Task* __restrict__ ctasks, const int32_t* __restrict__ multi,
                                                            const int32_t* __restrict__ parent, int32_t* __restrict__ rc) {
  const Task tk = ctasks[blockIdx.x];
  const int m = multi[tk.z];
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) rc[row] = (m && parent[row] == row) ? 1 : 0;
}

// component table in row order: (root row, rows of the component)
__global__ __launch_bounds__(AI_BLOCK) void k_comp_table(const Task* __restrict__ ctasks, const int32_t* __restrict__ multi,
                                                         const int32_t* __restrict__ parent, const int32_t* __restrict__ rootord,
                                                         const int32_t* __restrict__ rcnt, int32_t* __restrict__ troot,
                                                         int32_t* __restrict__ tsize) {
  const Task tk = ctasks[blockIdx.x];
  if (!multi[tk.z]) return;
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK)
    if (parent[row] == row) {
      const int o = rootord[row];
      troot[o] = row;
      tsize[o] = rcnt[row];
    }
}

// p = position of a row after the stable sort by root.  The row goes to position p of its parent's range in the
// final ordering and, if its component continues (cbase >= 0), to row cbase + (rank inside the component) of
// the next level's compact order.
__global__ __launch_bounds__(AI_BLOCK) void k_partition_multi(const Task* __restrict__ ctasks, const int32_t* __restrict__ multi,
                                                              const int32_t* __restrict__ seg_start, const int32_t* __restrict__ seg_gstart,
                                                              const int32_t* __restrict__ sorted_rows, const int32_t* __restrict__ parent,
                                                              const int32_t* __restrict__ rootord, const int32_t* __restrict__ cpos,
                                                              const int32_t* __restrict__ cbase, const int32_t* __restrict__ orig,
                                                              int32_t* __restrict__ final_order, int32_t* __restrict__ map,
                                                              int32_t* __restrict__ orig_next) {
  const Task tk = ctasks[blockIdx.x];
  const int s = tk.z;
  if (!multi[s]) return;
  const int s0 = seg_start[s], g0 = seg_gstart[s];
  for (int p = tk.x + threadIdx.x; p < tk.y; p += AI_BLOCK) {
    const int row = sorted_rows[p];
    const int o = rootord[parent[row]];
    const int32_t id = orig[row];
    final_order[g0 + (p - s0)] = id;
    const int base = cbase[o];
    const int32_t dst = (base >= 0) ? base + (p - cpos[o]) : -1;
    map[row] = dst;
    if (dst >= 0) orig_next[dst] = id;
  }
}

// parent_next[map[row]] = map[parent[row]]: a component's first row stays its first row under a
// stable partition, and when the cut ran between whole components it lands in the same child
__global__ __launch_bounds__(AI_BLOCK) void k_carry_parent(const int32_t* __restrict__ parent, const int32_t* __restrict__ map,
                                                           int32_t n, int32_t* __restrict__ parent_next) {
  const int i = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int32_t dst = map[i];
  if (dst >= 0) {
    const int32_t pr = map[parent[i]];
    parent_next[dst] = (pr >= 0) ? pr : dst;
  }
}

// kept entries of a surviving row: both ends on the same side of the cut
__global__ __launch_bounds__(AI_BLOCK) void k_rebuild_count(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                            const int32_t* __restrict__ flag, const int32_t* __restrict__ map,
                                                            int32_t n, int32_t* __restrict__ newcnt) {
  const int64_t gid = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const int32_t row = (int32_t)(gid / AI_LPR);
  const int l = (int)(gid & (AI_LPR - 1));
  if (row >= n) return;
  const int32_t dst = map[row];
  if (dst < 0) return;
  const int f = flag[row];
  int c = 0;
  const int p0 = rowptr[row], p1 = rowptr[row + 1];
  {
    int cc[AI_ROW_PF];
#pragma unroll
    for (int q = 0; q < AI_ROW_PF; ++q) {
      const int p = p0 + l + q * AI_LPR;
      cc[q] = (p < p1) ? col[p] : -1;
    }
#pragma unroll
    for (int q = 0; q < AI_ROW_PF; ++q)
      if (cc[q] >= 0) c += (flag[cc[q]] == f) ? 1 : 0;
  }
  for (int p = p0 + l + AI_ROW_PF * AI_LPR; p < p1; p += AI_LPR) c += (flag[col[p]] == f) ? 1 : 0;
  c += __shfl_xor(c, 8, 16);
  c += __shfl_xor(c, 4, 16);
  c += __shfl_xor(c, 2, 16);
  c += __shfl_xor(c, 1, 16);
  if (l == 0) newcnt[dst] = c;
}

__global__ __launch_bounds__(AI_BLOCK) void k_rebuild_fill(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                           const double* __restrict__ wraw, const int32_t* __restrict__ flag,
                                                           const int32_t* __restrict__ map, int32_t n,
                                                           const int32_t* __restrict__ new_rowptr, int32_t* __restrict__ new_col,
                                                           double* __restrict__ new_w) {
  const int64_t gid = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const int32_t row = (int32_t)(gid / AI_LPR);
  const int l = (int)(gid & (AI_LPR - 1));
  const int grp = (threadIdx.x & 63) / AI_LPR;
  const bool live = row < n;
  const int32_t dst = live ? map[row] : -1;
  const int f = (live && dst >= 0) ? flag[row] : -1;
  const int p0 = (dst >= 0) ? rowptr[row] : 0, p1 = (dst >= 0) ? rowptr[row + 1] : 0;
  int out = (dst >= 0) ? new_rowptr[dst] : 0;
  // all 64 lanes run the same number of rounds so that __ballot sees the whole wave
  int rounds = (p1 - p0 + AI_LPR - 1) / AI_LPR;
  for (int o = 32; o >= AI_LPR; o >>= 1) rounds = max(rounds, __shfl_xor(rounds, o, 64));
  // the first AI_ROW_PF rounds: every load of the chain col -> (flag, map), and the weights, in flight together
  int cq[AI_ROW_PF], mq[AI_ROW_PF];
  bool kq[AI_ROW_PF];
  double wq[AI_ROW_PF];
#pragma unroll
  for (int q = 0; q < AI_ROW_PF; ++q) {
    const int p = p0 + q * AI_LPR + l;
    const bool ok = p < p1;
    cq[q] = ok ? col[p] : -1;
    wq[q] = ok ? wraw[p] : 0.0;
  }
#pragma unroll
  for (int q = 0; q < AI_ROW_PF; ++q) {
    kq[q] = (cq[q] >= 0) && (flag[cq[q]] == f);
    mq[q] = (cq[q] >= 0) ? map[cq[q]] : -1;
  }
#pragma unroll
  for (int q = 0; q < AI_ROW_PF; ++q) {
    if (q >= rounds) break;  // wave-uniform
    const unsigned long long bal = __ballot(kq[q]);
    const unsigned int gbits = (unsigned int)((bal >> (grp * AI_LPR)) & 0xffffull);
    const int before = __popc(gbits & ((1u << l) - 1u));
    if (kq[q]) {
      new_col[out + before] = mq[q];
      new_w[out + before] = wq[q];
    }
    out += __popc(gbits);
  }
  for (int it = AI_ROW_PF; it < rounds; ++it) {
    const int p = p0 + it * AI_LPR + l;
    int c = -1;
    bool keep = false;
    if (p < p1) {
      c = col[p];
      keep = (flag[c] == f);
    }
    const unsigned long long bal = __ballot(keep);
    const unsigned int gbits = (unsigned int)((bal >> (grp * AI_LPR)) & 0xffffull);
    const int before = __popc(gbits & ((1u << l) - 1u));
    if (keep) {
      new_col[out + before] = map[c];
      new_w[out + before] = wraw[p];
    }
    out += __popc(gbits);
  }
}

// y = L_sym x = x - M x  (test hook, whole graph as one segment)
__global__ __launch_bounds__(AI_BLOCK) void k_lsym_apply(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         const double* __restrict__ wm, const double* __restrict__ sinv2,
                                                         const double* __restrict__ x, int32_t n, double* __restrict__ y) {
  const int64_t gid = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const int32_t row = (int32_t)(gid / AI_LPR);
  const int l = (int)(gid & (AI_LPR - 1));
  if (row >= n) return;
  double sum = 0.0;
  for (int p = rowptr[row] + l; p < rowptr[row + 1]; p += AI_LPR) sum = fma(wm[p], x[col[p]], sum);
  sum = ai_group16_sum(sum);
  if (l == 0) y[row] = x[row] - fma(sinv2[row], x[row], sum);
}

__global__ __launch_bounds__(AI_BLOCK) void k_iota(int32_t* __restrict__ a, int32_t n) {
  const int i = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < n) a[i] = i;
}
__global__ __launch_bounds__(AI_BLOCK) void k_scatter_d(const double* __restrict__ src, const int32_t* __restrict__ orig,
                                                        int32_t n, double scale, double* __restrict__ dst) {
  const int i = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < n) dst[orig[i]] = src[i] * scale;
}
__global__ __launch_bounds__(AI_BLOCK) void k_gather_d(const double* __restrict__ src, const int32_t* __restrict__ orig,
                                                       int32_t n, double* __restrict__ dst) {
  const int i = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < n) dst[i] = src[orig[i]];
}
__global__ __launch_bounds__(AI_BLOCK) void k_scatter_mask(const uint8_t* __restrict__ bin, const int32_t* __restrict__ orig,
                                                           int32_t n, int kstar, uint8_t* __restrict__ dst) {
  const int i = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < n) dst[orig[i]] = ((int)bin[i] > kstar) ? 1 : 0;
}


