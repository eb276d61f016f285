// Device kernels of the ASYNCHRONOUS FRONTIER of the recursive normalized cut (included by ai_ncut.hip inside its
// anonymous namespace; the device helpers it has in common with the level-synchronous Solver -- Task, uf_find / uf_unite,
// sturm_lt, MinMaxPart, mm_merge, TaskEnc, the AI_ENC_* capacities -- come from ai_ncut_shared.h).
//
// Layout (DESIGN.md section 3): every row of the call lives at its position p in the FINAL ordering from the start;
// a segment is the position range [g0, g0 + n) and its children are sub-ranges of it (mask side first,
// normalized_cut.py:57-59), so no per-row array is ever compacted.  The graph of a segment at recursion depth d is
// stored in buffer (d & 1): rows as {first, last+1} entry offsets (int2: a child's entries are packed into the front
// of its parent's entry range of the OTHER buffer, so consecutive segments of one buffer leave gaps and a shared
// rowptr[n + 1] would not do), columns as positions, raw weights.  Live segments are disjoint in position AND in
// entry-offset space, whatever their depth, so everything derived per segment (scaled weights, staged-gather
// encoding, Lanczos vectors, degrees ...) needs one array only.
//
// Two groups of kernels:
//   * "wave" kernels work on the segments the host has just harvested (frozen Lanczos segments, disconnected
//     segments, their children): task lists of int4 {lo, hi, slot, flags}, flags bit 0 = first task of its segment,
//     bit 1 = buffer of the segment's graph;
//   * "pool" kernels are one Lanczos step for every segment that is iterating, each at its OWN step count:
//     the launch carries the global step J, a task carries the step t0 at which its segment joined, j = J - t0.

struct FlowCsr {
  int2* rowse[2];
  int32_t* col[2];
  double* w[2];
  int32_t* orig[2];
};

#define FK_PAR(tk) (((tk).w >> 1) & 1)

// How a task of the frontier reaches its rows, columns and weights (the graph policy of the bodies in ai_ncut_shared.h): the
// buffer of its segment's depth.
struct FlowGraph {
  const FlowCsr& G;
  struct Rows {
    const int2* __restrict__ rowse;
    __device__ __forceinline__ int2 operator()(int row) const { return rowse[row]; }
  };
  __device__ __forceinline__ Rows rows(const Task& tk) const { return Rows{G.rowse[FK_PAR(tk)]}; }
  __device__ __forceinline__ const int32_t* col(const Task& tk) const { return G.col[FK_PAR(tk)]; }
  __device__ __forceinline__ const double* w(const Task& tk) const { return G.w[FK_PAR(tk)]; }
};

// What the host uploads per segment; the task lists of a launch are expanded from these records on the device
// (a pool of 24 chunks has ~150 k fine tasks: 5 MB per re-listing if the host wrote them).
struct __attribute__((aligned(16))) SegRec {
  int32_t g0, n;       // position range
  int32_t slot;        // Lanczos state (histories, frozen, m) of the segment
  int32_t par;         // buffer of its graph
  int32_t f0, c0;      // first stable fine / coarse index
  int32_t foff, coff;  // first task of the segment in this launch's fine / coarse list
  int32_t t0, cap;     // pool: start step, Krylov dimension limit
  int32_t idx;         // index of the record in its list (wave-local segment index)
  int32_t aux;         // index of the segment in the list its per-segment inputs (volume) were computed for
  int32_t vdelta;      // row of the Lanczos vector slabs that holds position 0 of the segment's chunk (slabs cover a WINDOW of chunks)
  int32_t pad0;        // (warm start) rows of the vector that lies at the segment's positions in warm[]; 0: none (fk_lz_init)
  int32_t pad1;        // (principal-axis start) 1 + the segment's chunk, 0: the segment does not take part (fk_pca_*)
  int32_t pad2;
};

#define FK_NF(sr) (((sr).n + AI_FINE_ROWS - 1) / AI_FINE_ROWS)
#define FK_NC(sr) (((sr).n + AI_COARSE_ROWS - 1) / AI_COARSE_ROWS)

// ----------------------------------------------------------------------------- root set-up
// rowse[p] = {rowptr[p], rowptr[p + 1]} of the (merged) input graph
__global__ __launch_bounds__(AI_BLOCK) void fk_rowse_from_rowptr(const int32_t* __restrict__ rowptr, int32_t n, int2* __restrict__ rowse) {
  const int i = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < n) rowse[i] = make_int2(rowptr[i], rowptr[i + 1]);
}

// ----------------------------------------------------------------------------- degrees, scaling (normalized_cut.py:38-47)
__global__ __launch_bounds__(AI_BLOCK) void fk_degree(const Task* __restrict__ tasks, FlowCsr G, double* __restrict__ deg,
                                                      double* __restrict__ sinv, double* __restrict__ pvol) {
  degree_body(tasks[blockIdx.x], FlowGraph{G}, deg, sinv, pvol);
}

// one block per record i: out[i] = sum of the partials of its fine tasks in a fixed order
__global__ __launch_bounds__(AI_BLOCK) void fk_seg_sum(const SegRec* __restrict__ recs, const double* __restrict__ part, double* __restrict__ out) {
  __shared__ double sm[AI_BLOCK / 64];
  const SegRec sr = recs[blockIdx.x];
  const double tot = ai_range_sum(part, sr.foff, sr.foff + FK_NF(sr), sm);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

__global__ __launch_bounds__(AI_BLOCK) void fk_scale(const Task* __restrict__ tasks, const SegRec* __restrict__ recs, FlowCsr G,
                                                     const double* __restrict__ deg, const double* __restrict__ sinv,
                                                     const double* __restrict__ vol, double* __restrict__ wm, double* __restrict__ sinv2,
                                                     double* __restrict__ u1, const int32_t* __restrict__ gate, int nbin) {
  const Task tk = tasks[blockIdx.x];
  if (tk.z < nbin && gate[tk.z] != 1) return;  // a child of a cut that fell apart: it is split by components first
  scale_body(tk, FlowGraph{G}, vol[recs[tk.z].aux], deg, sinv, wm, sinv2, u1);
}

// ----------------------------------------------------------------------------- connected components (labels = positions)
__global__ __launch_bounds__(AI_BLOCK) void fk_cc_init(const Task* __restrict__ tasks, FlowCsr G, int32_t* __restrict__ parent,
                                                       int32_t* __restrict__ ncomp) {
  const Task tk = tasks[blockIdx.x];
  if ((tk.w & 1) && threadIdx.x == 0) ncomp[tk.z] = 0;  // first task of its segment: fk_cc_count adds the roots up (three launches later)
  const int2* __restrict__ rowse = G.rowse[FK_PAR(tk)];
  const int32_t* __restrict__ col = G.col[FK_PAR(tk)];
  const int l = threadIdx.x & (AI_LPR - 1), r = threadIdx.x / AI_LPR;
  for (int row = tk.x + r; row < tk.y; row += AI_BLOCK / AI_LPR) {
    const int2 se = rowse[row];
    int32_t mn = row;
    for (int p = se.x + l; p < se.y; p += AI_LPR) mn = min(mn, col[p]);
    mn = min(mn, __shfl_xor(mn, 8, 16));
    mn = min(mn, __shfl_xor(mn, 4, 16));
    mn = min(mn, __shfl_xor(mn, 2, 16));
    mn = min(mn, __shfl_xor(mn, 1, 16));
    if (l == 0) parent[row] = mn;
  }
}

// Sampled hooking (after Afforest, Sutton et al. 2018).  fk_cc_init has linked every row to its smallest neighbour; fk_cc_sample
// unites it with two more (its last and its middle entry); after a compression nearly every row of a child that is connected --
// the usual case -- sits in the tree of the segment's first row, and fk_cc_hook walks the entries of the OTHER rows only (in both
// directions: the rows that skip do not look at their side of an edge).  Until round 4 every stored edge went through the
// union-find: 95 us per launch on average, 2.4 ms for the roots of a 12-chunk call.  Roots are still the smallest position of a
// component, so the component labels, hence the children's order, are what they were.
__global__ __launch_bounds__(AI_BLOCK) void fk_cc_sample(const Task* __restrict__ tasks, FlowCsr G, int32_t* parent) {
  const Task tk = tasks[blockIdx.x];
  const int2* __restrict__ rowse = G.rowse[FK_PAR(tk)];
  const int32_t* __restrict__ col = G.col[FK_PAR(tk)];
  const int l = threadIdx.x & (AI_LPR - 1), r = threadIdx.x / AI_LPR;
  for (int row = tk.x + r; row < tk.y; row += AI_BLOCK / AI_LPR) {
    const int2 se = rowse[row];
    if (l < 2 && se.y > se.x) {
      const int32_t c = col[l == 0 ? se.y - 1 : (se.x + se.y) >> 1];
      if (c != row) uf_unite(parent, row, c);
    }
  }
}

__global__ __launch_bounds__(AI_BLOCK) void fk_cc_hook(const Task* __restrict__ tasks, const SegRec* __restrict__ recs, FlowCsr G, int32_t* parent) {
  __shared__ int32_t s_giant;
  const Task tk = tasks[blockIdx.x];
  const int2* __restrict__ rowse = G.rowse[FK_PAR(tk)];
  const int32_t* __restrict__ col = G.col[FK_PAR(tk)];
  if (threadIdx.x == 0) s_giant = uf_find(parent, recs[tk.z].g0);  // the tree of the segment's first row (a stale root only costs work)
  __syncthreads();
  const int32_t giant = s_giant;
  const int l = threadIdx.x & (AI_LPR - 1), r = threadIdx.x / AI_LPR;
  for (int row = tk.x + r; row < tk.y; row += AI_BLOCK / AI_LPR) {
    int32_t rr = (l == 0) ? uf_find(parent, row) : 0;
    rr = __shfl(rr, (threadIdx.x & 63) & ~(AI_LPR - 1), 64);
    if (rr == giant) continue;  // (uniform over the row's 16 lanes)
    const int2 se = rowse[row];
    for (int p = se.x + l; p < se.y; p += AI_LPR) {
      const int32_t c = col[p];
      if (c != row) uf_unite(parent, row, c);
    }
  }
}

__global__ __launch_bounds__(AI_BLOCK) void fk_cc_compress(const Task* __restrict__ tasks, int32_t* parent) {
  const Task tk = tasks[blockIdx.x];
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    int32_t x = row;
    for (;;) {
      const int32_t p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (p == x) break;
      x = p;
    }
    parent[row] = x;
  }
}

// roots per segment slot (integer atomics: order independent); ncomp[slot] zeroed by the caller
__global__ __launch_bounds__(AI_BLOCK) void fk_cc_count(const Task* __restrict__ tasks, const int32_t* __restrict__ parent,
                                                        int32_t* __restrict__ ncomp) {
  const Task tk = tasks[blockIdx.x];
  int c = 0;
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) c += (parent[row] == row);
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(&ncomp[tk.z], c);
}

// ----------------------------------------------------------------------------- staged-gather encoding
// As k_lz_encode, but the distinct-column list of a task is stored at the task's own first entry offset
// (a task has at least as many entries as distinct columns; live segments own disjoint offset ranges), and
// the record goes to the task's STABLE index (Task.w >> 2), which survives every re-listing of the pool.
// Round 4: the distinct columns are found with an LDS hash table and only THEY are ordered (each by counting the smaller ones:
// ~180 broadcast reads per thread), instead of a bitonic sort of all ~1200 entries (66 passes with a barrier each) and a binary
// search per entry.  Same output -- the ascending list of distinct columns and every entry's index into it -- at a third of the time.
#define FK_ENC_HT 2048  // hash slots (>= 2 x AI_ENC_XCAP)
__global__ __launch_bounds__(AI_BLOCK) void fk_encode(const Task* __restrict__ ftasks, FlowCsr G, int32_t* __restrict__ ucol,
                                                      uint16_t* __restrict__ lidx, TaskEnc* __restrict__ enc,
                                                      const int32_t* __restrict__ gate, int nbin) {
  static_assert(FK_ENC_HT >= 2 * AI_ENC_XCAP && FK_ENC_HT % AI_BLOCK == 0 && (FK_ENC_HT & (FK_ENC_HT - 1)) == 0, "hash table shape");
  __shared__ int32_t keys[FK_ENC_HT];       // column of a slot, -1 = free
  __shared__ uint16_t srank[FK_ENC_HT];     // slot -> compact index, then -> rank in the ascending list
  __shared__ uint16_t eslot[AI_ENC_MAXNNZ]; // slot of every entry
  __shared__ int32_t uq[AI_ENC_XCAP];       // distinct columns, compact (slot order)
  __shared__ int32_t usort[AI_ENC_XCAP];    // ... ascending
  __shared__ int32_t wsum[AI_BLOCK / 64];
  __shared__ int32_t s_over;
  const Task tk = ftasks[blockIdx.x];
  if (tk.z < nbin && gate[tk.z] != 1) return;
  const int2* __restrict__ rowse = G.rowse[FK_PAR(tk)];
  const int32_t* __restrict__ col = G.col[FK_PAR(tk)];
  const int pidx = tk.w >> 2;
  const int p0 = rowse[tk.x].x, cnt = rowse[tk.y - 1].y - p0;
  if (cnt > AI_ENC_MAXNNZ || cnt <= 0) {
    if (threadIdx.x == 0) enc[pidx] = TaskEnc{0, -1};
    return;
  }
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < FK_ENC_HT / AI_BLOCK; ++q) keys[tid + q * AI_BLOCK] = -1;
  if (tid == 0) s_over = 0;
  __syncthreads();
  // ---- every entry finds (or takes) the slot of its column
  for (int e = tid; e < cnt; e += AI_BLOCK) {
    const int32_t c = col[p0 + e];
    unsigned h = ((unsigned)c * 2654435761u) >> 21;  // 11 bits
    bool done = false;
    for (int i = 0; i < FK_ENC_HT && !done; ++i) {
      const int32_t old = atomicCAS(&keys[h], -1, c);
      if (old == -1 || old == c) done = true; else h = (h + 1) & (FK_ENC_HT - 1);
    }
    if (!done) s_over = 1;
    eslot[e] = (uint16_t)h;
  }
  __syncthreads();
  // ---- number the occupied slots (prefix over the block) and collect the distinct columns
  constexpr int SPT = FK_ENC_HT / AI_BLOCK;  // slots per thread
  int mine = 0;
#pragma unroll
  for (int q = 0; q < SPT; ++q) mine += keys[tid * SPT + q] >= 0;
  int incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(incl, o, 64);
    if ((tid & 63) >= o) incl += v;
  }
  if ((tid & 63) == 63) wsum[tid >> 6] = incl;
  __syncthreads();
  int base = incl - mine, total = 0;
#pragma unroll
  for (int w = 0; w < AI_BLOCK / 64; ++w) {
    if (w < (tid >> 6)) base += wsum[w];
    total += wsum[w];
  }
  if (total > AI_ENC_XCAP || s_over) {
    if (tid == 0) enc[pidx] = TaskEnc{0, -1};
    return;
  }
#pragma unroll
  for (int q = 0; q < SPT; ++q) {
    const int32_t k = keys[tid * SPT + q];
    if (k >= 0) {
      srank[tid * SPT + q] = (uint16_t)base;
      uq[base++] = k;
    }
  }
  __syncthreads();
  // ---- rank of every distinct column = how many are smaller (the list is short: broadcast reads)
  for (int i0 = tid; i0 < total; i0 += AI_BLOCK) {
    const int32_t v = uq[i0];
    int r = 0;
    for (int i = 0; i < total; ++i) r += uq[i] < v;
    usort[r] = v;
    keys[i0] = r;  // (keys[] is dead as a hash table since the barrier above: its first `total` words now map compact index -> rank)
  }
  __syncthreads();
  for (int i = tid; i < total; i += AI_BLOCK) ucol[p0 + i] = usort[i];
  for (int e = tid; e < cnt; e += AI_BLOCK) lidx[p0 + e] = (uint16_t)keys[srank[eslot[e]]];
  if (tid == 0) enc[pidx] = TaskEnc{p0, total};
}

// ----------------------------------------------------------------------------- the pool: one Lanczos step for every running segment
// A pool task: what one block needs without a second look-up.
struct __attribute__((aligned(16))) FTask {       // 32-row task of the SpMV
  int32_t lo, hi;    // position range
  int32_t vdelta;    // slab row of position 0 of the segment's chunk
  int32_t flags;     // bit 1: buffer of the segment's graph
  int32_t pidx;      // stable fine index: activity flag, partial of R.z, encoding record
  int32_t uoff, ucnt;  // staged-gather record (filled on the device by fk_list_finish)
  int32_t t0;        // global step at which the segment started: its own step is j = J - t0
};
struct __attribute__((aligned(16))) CTask {       // 512-row task of the update
  int32_t lo, hi, slot, flags;   // flags bit 0: first task of its segment
  int32_t pidx;      // stable coarse index: activity flag, partials of (R.R, u1.R)
  int32_t f0, f1;    // the segment's stable fine range
  int32_t c0, c1;    // the segment's stable coarse range
  int32_t t0;
  int32_t cap;       // Krylov dimension limit of the segment: min(max_iter, n - 1)
  int32_t vdelta;
};

// FK_HIST_HEAD (doubles in front of a packed history row: theta, resid, m, checksum) comes from ai_flow_host.h with the rows' layout
struct FlowLz {
  int32_t* frozen;      // [slot]
  int32_t* m;           // [slot] size of T at freeze
  double* alpha_hist;   // [slot][mcap]
  double* b_hist;       // [slot][mcap + 1]
  double* g_hist;       // [slot][mcap + 1]
  int32_t* factive;     // [stable fine index]
  int32_t* cactive;     // [stable coarse index]
  int mcap;
#ifdef AI_TRACE_HIST
  // diagnosis build: who wrote history row j < 64 of a slot last ({J, t0, pidx, block} and {a, alpha}), and what the check saw when it
  // froze the slot ({J, m, prev_m, rounds} and {theta, resid, a_0, a_1, a_{m-1}, b_1^2, lo_0, hi_0})
  int4* sig_i;          // [slot][64]
  double2* sig_d;       // [slot][64]
  int4* chk_i;          // [slot]
  double* chk_d;        // [slot][8]
#endif
};

// What a convergence check needs to know about a pool segment (one record per pool entry, rebuilt with the lists)
struct __attribute__((aligned(16))) PoolSeg {
  int32_t slot, n, g0, t0;
  int32_t f0, f1, c0, c1;
  int32_t cap, par, pad1, pad2;
};

// wave lists: Task {lo, hi, record index, first | par << 1 | x << 2}, x = the task's stable index (stable != 0) or
// the record index
// `recs` may be pinned host memory (each block reads its one record over the bus); `keep` receives a device copy
__global__ __launch_bounds__(AI_BLOCK) void fk_expand_wave(const SegRec* __restrict__ recs, SegRec* __restrict__ keep, Task* __restrict__ fine,
                                                           Task* __restrict__ coarse, int stable, const int4* __restrict__ xs0,
                                                           int4* __restrict__ xd0, int xn0, const int4* __restrict__ xs1,
                                                           int4* __restrict__ xd1, int xn1) {
  __shared__ int32_t sm_rec[sizeof(SegRec) / 4];
  const SegRec sr = ai_ld_sys_record_block(&recs[blockIdx.x], sm_rec);  // (pinned, rewritten by the host per wave stage: see ai_ld_sys)
  if (keep && threadIdx.x == 0) keep[blockIdx.x] = sr;
  // up to two small tables (split records, component flags ...) ride along: 16-byte words, strided over the grid
  for (int i = blockIdx.x * AI_BLOCK + threadIdx.x; i < xn0; i += gridDim.x * AI_BLOCK) xd0[i] = ai_ld_sys_record(&xs0[i]);
  for (int i = blockIdx.x * AI_BLOCK + threadIdx.x; i < xn1; i += gridDim.x * AI_BLOCK) xd1[i] = ai_ld_sys_record(&xs1[i]);
  const int nf = (sr.n + AI_FINE_ROWS - 1) / AI_FINE_ROWS, nc = (sr.n + AI_COARSE_ROWS - 1) / AI_COARSE_ROWS;
  if (fine)
    for (int k = threadIdx.x; k < nf; k += AI_BLOCK) {
      Task t;
      t.x = sr.g0 + k * AI_FINE_ROWS;
      t.y = min(t.x + AI_FINE_ROWS, sr.g0 + sr.n);
      t.z = sr.idx;
      t.w = (k == 0 ? 1 : 0) | (sr.par << 1) | ((stable ? sr.f0 + k : sr.idx) << 2);
      fine[sr.foff + k] = t;
    }
  if (coarse)
    for (int k = threadIdx.x; k < nc; k += AI_BLOCK) {
      Task t;
      t.x = sr.g0 + k * AI_COARSE_ROWS;
      t.y = min(t.x + AI_COARSE_ROWS, sr.g0 + sr.n);
      t.z = sr.idx;
      t.w = (k == 0 ? 1 : 0) | (sr.par << 1) | ((stable ? sr.c0 + k : sr.idx) << 2);
      coarse[sr.coff + k] = t;
    }
}

// pool lists (one block per pool segment)
__global__ __launch_bounds__(AI_BLOCK) void fk_expand_pool(const SegRec* __restrict__ recs /* pinned host memory */, const TaskEnc* __restrict__ enc,
                                                           int force_plain, FTask* __restrict__ fine, CTask* __restrict__ coarse,
                                                           PoolSeg* __restrict__ pool) {
  __shared__ int32_t sm_rec[sizeof(SegRec) / 4];
  const SegRec sr = ai_ld_sys_record_block(&recs[blockIdx.x], sm_rec);  // (a ring of pinned tables the host rewrites at every relist)
  const int nf = (sr.n + AI_FINE_ROWS - 1) / AI_FINE_ROWS, nc = (sr.n + AI_COARSE_ROWS - 1) / AI_COARSE_ROWS;
  for (int k = threadIdx.x; k < nf; k += AI_BLOCK) {
    FTask t;
    t.lo = sr.g0 + k * AI_FINE_ROWS;
    t.hi = min(t.lo + AI_FINE_ROWS, sr.g0 + sr.n);
    t.vdelta = sr.vdelta;
    t.flags = (k == 0 ? 1 : 0) | (sr.par << 1);
    t.pidx = sr.f0 + k;
    const TaskEnc e = enc[sr.f0 + k];
    t.uoff = e.uoff;
    t.ucnt = force_plain ? -1 : e.ucnt;
    t.t0 = sr.t0;
    fine[sr.foff + k] = t;
  }
  for (int k = threadIdx.x; k < nc; k += AI_BLOCK) {
    CTask t;
    t.lo = sr.g0 + k * AI_COARSE_ROWS;
    t.hi = min(t.lo + AI_COARSE_ROWS, sr.g0 + sr.n);
    t.slot = sr.slot;
    t.flags = (k == 0 ? 1 : 0) | (sr.par << 1);
    t.pidx = sr.c0 + k;
    t.f0 = sr.f0;
    t.f1 = sr.f0 + nf;
    t.c0 = sr.c0;
    t.c1 = sr.c0 + nc;
    t.t0 = sr.t0;
    t.cap = sr.cap;
    t.vdelta = sr.vdelta;
    coarse[sr.coff + k] = t;
  }
  if (threadIdx.x == 0) {
    PoolSeg ps;
    ps.slot = sr.slot;
    ps.n = sr.n;
    ps.g0 = sr.g0;
    ps.t0 = sr.t0;
    ps.f0 = sr.f0;
    ps.f1 = sr.f0 + nf;
    ps.c0 = sr.c0;
    ps.c1 = sr.c0 + nc;
    ps.cap = sr.cap;
    ps.par = sr.par;
    ps.pad1 = ps.pad2 = 0;
    pool[blockIdx.x] = ps;
  }
}

// a recycled slot starts a new solve
__global__ __launch_bounds__(AI_BLOCK) void fk_reset_slots(const SegRec* __restrict__ recs, int n, FlowLz L, int32_t* __restrict__ lastm,
                                                           int32_t* __restrict__ nextm, int first_check, double* __restrict__ theta,
                                                           double* __restrict__ resid, const int32_t* __restrict__ gate, int nbin,
                                                           int32_t* __restrict__ ncomp_host) {
  const int i = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  if (i < nbin) __hip_atomic_store(&ncomp_host[i], gate[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // straight into pinned memory
  if (i < nbin && gate[i] != 1) return;
  const int s = recs[i].slot;
  // (per-slot check state: read by fk_check on another stream with ai_ld_agent)
  ai_st_agent(&L.frozen[s], 0);
  ai_st_agent(&L.m[s], 0);
  ai_st_agent(&lastm[s], 0);
  ai_st_agent(&nextm[s], (int32_t)first_check);
  ai_st_agent(&theta[s], 0.0);
  ai_st_agent(&resid[s], 0.0);
}

__device__ __forceinline__ const double* fk_vec(double* const* __restrict__ slabs, size_t stride, int j) {
  return slabs[j / AI_SLAB_VECS] + (size_t)(j % AI_SLAB_VECS) * stride;
}

// ----------------------------------------------------------------------------- start vector of the ancestor-less segments
// A segment without a solved ancestor (a component a chunk falls into first: half of a chunk's row-steps) whose graph kept its points
// (ai_csr::xyz: ai_affinity_build*) starts from the smooth vector the points themselves give: u1 * t, t = the coordinate along the
// principal axis of the segment's own points, centred.  Three small launches before fk_lz_init, two passes over the segment's rows:
//   fk_pca_moments  per coarse task: the three coordinate sums and six second-moment sums of its rows about the segment's FIRST row's
//                   point (so that they do not cancel), at the task's stable coarse index (Task.w >> 2), one plane per sum;
//   fk_pca_axis     per segment: the partials added in task order, mean and covariance, its leading eigenvector e (ai_jacobi3: the
//                   component of e largest in magnitude is positive), sigma = the standard deviation of t; sigma > 0 and finite:
//                   axis[i] = {e, centre, sqrt(n) / sigma} and SegRec.pad0 = n, else pad0 stays 0 and the segment starts from the hash;
//   fk_pca_fill     per coarse task: warm[row] = u1[row] * t[row] * sqrt(n) / sigma (root-mean-square 1 up to the correlation of degree
//                   and coordinate), which fk_lz_init then treats like a carried warm vector of an n-row ancestor.
// SegRec.pad1 = 1 + chunk of a segment that takes part (0: none), xyz_tab[chunk] = the chunk's points by ORIGINAL id.  The sums depend
// on the segment's own rows and tasks only: a chunk cut in a batch gets the bits of the chunk cut alone, and a segment that is sent
// back by the true-residual test gets the same vector again.
#define FK_PCA_VALS 9
__global__ __launch_bounds__(AI_BLOCK) void fk_pca_moments(const Task* __restrict__ ctasks, const SegRec* __restrict__ recs, FlowCsr G,
                                                           const double* const* __restrict__ xyz_tab, double* __restrict__ part, size_t pstride,
                                                           const int32_t* __restrict__ gate, int nbin) {
  __shared__ double sm[AI_BLOCK / 64];
  const Task tk = ctasks[blockIdx.x];
  if (tk.z < nbin && gate[tk.z] != 1) return;
  const SegRec sr = recs[tk.z];
  if (sr.pad1 == 0) return;
  const double* __restrict__ xyz = xyz_tab[sr.pad1 - 1];
  const int32_t* __restrict__ orig = G.orig[FK_PAR(tk)];
  const size_t o0 = (size_t)3 * (size_t)orig[sr.g0];
  const double rx = xyz[o0], ry = xyz[o0 + 1], rz = xyz[o0 + 2];
  double s[FK_PCA_VALS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    const size_t o = (size_t)3 * (size_t)orig[row];
    const double dx = xyz[o] - rx, dy = xyz[o + 1] - ry, dz = xyz[o + 2] - rz;
    s[0] += dx;
    s[1] += dy;
    s[2] += dz;
    s[3] = fma(dx, dx, s[3]);
    s[4] = fma(dx, dy, s[4]);
    s[5] = fma(dx, dz, s[5]);
    s[6] = fma(dy, dy, s[6]);
    s[7] = fma(dy, dz, s[7]);
    s[8] = fma(dz, dz, s[8]);
  }
#pragma unroll
  for (int k = 0; k < FK_PCA_VALS; ++k) {
    const double tot = ai_block_sum(s[k], sm);
    if (threadIdx.x == 0) part[(size_t)k * pstride + (size_t)(tk.w >> 2)] = tot;
  }
}

// one block per record of the wave's children
__global__ __launch_bounds__(AI_BLOCK) void fk_pca_axis(SegRec* __restrict__ recs, FlowCsr G, const double* const* __restrict__ xyz_tab,
                                                        const double* __restrict__ part, size_t pstride, double* __restrict__ axis,
                                                        const int32_t* __restrict__ gate, int nbin) {
  __shared__ double sm[AI_BLOCK / 64];
  const int i = blockIdx.x;
  if (i < nbin && gate[i] != 1) return;
  const SegRec sr = recs[i];
  if (sr.pad1 == 0) return;
  double s[FK_PCA_VALS];
#pragma unroll
  for (int k = 0; k < FK_PCA_VALS; ++k) s[k] = ai_range_sum(part + (size_t)k * pstride, sr.c0, sr.c0 + FK_NC(sr), sm);
  if (threadIdx.x != 0) return;
  const double inv = 1.0 / (double)sr.n;
  const double mx = s[0] * inv, my = s[1] * inv, mz = s[2] * inv;
  const double cov[6] = {s[3] * inv - mx * mx, s[4] * inv - mx * my, s[5] * inv - mx * mz,
                         s[6] * inv - my * my, s[7] * inv - my * mz, s[8] * inv - mz * mz};
  double e[3];
  const double sigma = sqrt(ai_jacobi3(cov, e));
  const double* __restrict__ xyz = xyz_tab[sr.pad1 - 1];
  const size_t o0 = (size_t)3 * (size_t)G.orig[sr.par][sr.g0];
  const double cx = xyz[o0] + mx, cy = xyz[o0 + 1] + my, cz = xyz[o0 + 2] + mz;
  // every point the same (sigma = 0), or a sum that is not finite: the segment keeps the hash start
  if (!(sigma > 0.0) || !(fabs(sigma) + fabs(cx) + fabs(cy) + fabs(cz) <= 1.7976931348623157e308)) return;
  double* a = axis + (size_t)8 * i;
  a[0] = e[0];
  a[1] = e[1];
  a[2] = e[2];
  a[3] = cx;
  a[4] = cy;
  a[5] = cz;
  a[6] = sqrt((double)sr.n) / sigma;
  a[7] = sigma;
  recs[i].pad0 = sr.n;
}

__global__ __launch_bounds__(AI_BLOCK) void fk_pca_fill(const Task* __restrict__ ctasks, const SegRec* __restrict__ recs, FlowCsr G,
                                                        const double* const* __restrict__ xyz_tab, const double* __restrict__ axis,
                                                        const double* __restrict__ u1, double* __restrict__ warm,
                                                        const int32_t* __restrict__ gate, int nbin) {
  const Task tk = ctasks[blockIdx.x];
  if (tk.z < nbin && gate[tk.z] != 1) return;
  const SegRec sr = recs[tk.z];
  if (sr.pad1 == 0 || sr.pad0 == 0) return;
  const double* __restrict__ xyz = xyz_tab[sr.pad1 - 1];
  const int32_t* __restrict__ orig = G.orig[FK_PAR(tk)];
  const double* __restrict__ a = axis + (size_t)8 * tk.z;
  const double ex = a[0], ey = a[1], ez = a[2], cx = a[3], cy = a[4], cz = a[5], sc = a[6];
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    const size_t o = (size_t)3 * (size_t)orig[row];
    const double t = fma(xyz[o + 2] - cz, ez, fma(xyz[o + 1] - cy, ey, (xyz[o] - cx) * ex));
    warm[row] = (u1[row] * t) * sc;
  }
}

// R_0 = hash(original id); partials of (R.R, u1.R) at the tasks' stable coarse indices (Task.w >> 2); flags on
// (warm != null, round 5: a segment with a solved ancestor starts from that ancestor's SECOND Ritz vector at its own rows -- warm[],
// carried through the partitions -- scaled to entries of order 1, plus a thousandth of the hash vector so that the start can never be
// degenerate (CPU study: 0.1 / 0.01 / 0.001 / 0.0001 of it leave 0.931 / 0.916 / 0.908 / 0.902 of the hash start's row-steps);
// SegRec.pad0 = the ancestor's row count, 0 = no ancestor: the hash vector alone -- unless fk_pca_axis above has set it to the segment's
// own row count and fk_pca_fill has written warm[] at its rows)
__global__ __launch_bounds__(AI_BLOCK) void fk_lz_init(const Task* __restrict__ ctasks, const SegRec* __restrict__ recs, FlowCsr G,
                                                       const double* __restrict__ u1, double* __restrict__ R0, double2* __restrict__ pB0,
                                                       int32_t* __restrict__ cactive, const int32_t* __restrict__ gate, int nbin,
                                                       const double* __restrict__ warm, double2* __restrict__ pBw) {
  __shared__ double sm[AI_BLOCK / 64];
  const Task tk = ctasks[blockIdx.x];
  if (tk.z < nbin && gate[tk.z] != 1) return;
  R0 += recs[tk.z].vdelta;
  const int wn = warm ? recs[tk.z].pad0 : 0;
  if (wn > 0) pB0 = pBw;  // a start that carries a warm vector passes fk_lz_project, which reads all of the segment's partials
  const double wscale = sqrt((double)wn);
  const int32_t* __restrict__ orig = G.orig[FK_PAR(tk)];
  double nn = 0.0, gg = 0.0;
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    double r = ai_hash_unit((uint32_t)orig[row]);
    if (wn > 0) r = fma(warm[row], wscale, 1e-3 * r);
    R0[row] = r;
    nn = fma(r, r, nn);
    gg = fma(u1[row], r, gg);
  }
  const double tn = ai_block_sum(nn, sm);
  const double tg = ai_block_sum(gg, sm);
  if (threadIdx.x == 0) {
    pB0[tk.w >> 2] = make_double2(tn, tg);
    ai_st_agent(&cactive[tk.w >> 2], 1);
  }
}
// A warm vector can be all but parallel to the segment's u1: the second Ritz vector of an ancestor is all but constant times sqrt(d)
// on a block that ancestor cut off along a weak bridge.  Step 0 of fk_update takes b_0^2 = R.R - (u1.R)^2 and alpha_0 from
// R.MR - (u1.R)^2, which then cancel: with 1e-7 of R.R left, the first Lanczos vector's norm is off by 5e-9, and a solve that would
// take 9 steps stalls at residuals of 1e-7 until its Krylov space is exhausted (tests/csr_cases.py BAND; the NumPy model shows the
// same with that norm).  So where less than a hundredth of R.R is left, u1 is taken out of R_0 here, once, before the first step,
// and the partials are those of the projected vector; every other start goes on unchanged, bit for bit.  The decision is made
// from the segment's own partials in a fixed order: a chunk cut in a batch decides as the chunk cut alone.
// pBw: the partials fk_lz_init wrote for segments with a warm vector (read by every block of the segment); pB0: where step 0 reads.
__global__ __launch_bounds__(AI_BLOCK) void fk_lz_project(const Task* __restrict__ ctasks, const SegRec* __restrict__ recs,
                                                          const double* __restrict__ u1, double* __restrict__ R0,
                                                          const double2* __restrict__ pBw, double2* __restrict__ pB0,
                                                          const int32_t* __restrict__ gate, int nbin) {
  __shared__ double sm[AI_BLOCK / 64];
  const Task tk = ctasks[blockIdx.x];
  if (tk.z < nbin && gate[tk.z] != 1) return;
  const SegRec sr = recs[tk.z];
  if (sr.pad0 <= 0) return;  // no warm vector: fk_lz_init wrote pB0 itself
  double nn = 0.0, g = 0.0;
  for (int t = sr.c0 + threadIdx.x; t < sr.c0 + FK_NC(sr); t += AI_BLOCK) {
    const double2 v = pBw[t];
    nn += v.x;
    g += v.y;
  }
  nn = ai_block_sum(nn, sm);
  g = ai_block_sum(g, sm);
  if (!(nn - g * g < 1e-2 * nn)) {  // (also a sum that is not finite: left to the solve as before)
    if (threadIdx.x == 0) pB0[tk.w >> 2] = pBw[tk.w >> 2];
    return;
  }
  R0 += sr.vdelta;
  double n2 = 0.0, g2 = 0.0;
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    const double u = u1[row];
    const double r = fma(-g, u, R0[row]);
    R0[row] = r;
    n2 = fma(r, r, n2);
    g2 = fma(u, r, g2);
  }
  const double tn = ai_block_sum(n2, sm);
  const double tg = ai_block_sum(g2, sm);
  if (threadIdx.x == 0) pB0[tk.w >> 2] = make_double2(tn, tg);
}
__global__ __launch_bounds__(AI_BLOCK) void fk_set_flags(const Task* __restrict__ ftasks, int n, int32_t* __restrict__ factive,
                                                         const int32_t* __restrict__ gate, int nbin) {
  const int i = blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  const Task t = ftasks[i];
  if (t.z < nbin && gate[t.z] != 1) return;
  ai_st_agent(&factive[t.w >> 2], 1);  // (read by fk_spmv on the stepping stream with ai_ld_agent)
}

// z = M R_j for the rows of one task (plain gather; tasks the encoder could not take)
template <int ILP>
__device__ __forceinline__ void fk_spmv_plain(const FTask tk, const int2* __restrict__ rowse, const int32_t* __restrict__ col,
                                              const double* __restrict__ wm, const double* __restrict__ sinv2,
                                              const double* __restrict__ Rj, double* __restrict__ Z, double* __restrict__ pA,
                                              double* sm) {
  constexpr int LPR = 16;
  const int l = threadIdx.x & (LPR - 1), r = threadIdx.x / LPR;
  constexpr int GROUPS = AI_BLOCK / LPR;
  int p0[ILP], p1[ILP];
  double sum[ILP], ri[ILP], s2[ILP];
  int len = 0;
#pragma unroll
  for (int u = 0; u < ILP; ++u) {
    const int row = tk.lo + r + u * GROUPS;
    const bool ok = row < tk.hi;
    const int2 se = ok ? rowse[row] : make_int2(0, 0);
    p0[u] = se.x;
    p1[u] = se.y;
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
    const double sg = ai_group16_sum(sum[u]);
    const int row = tk.lo + r + u * GROUPS;
    if (l == 0 && row < tk.hi) {
      const double z = fma(s2[u], ri[u], sg);
      Z[row] = z;
      acc = fma(ri[u], z, acc);
    }
  }
  const double tot = ai_block_sum(acc, sm);
  if (threadIdx.x == 0) pA[tk.pidx] = tot;
}

// THE hot kernel (k_lz_spmv_q of the lock-step driver, per-segment step counts): z = M R_j, partial of R_j . z.
template <int ILP, bool STAMP>
// (argument order: the 16 dwords the front of every block needs come first, so that they are preloaded into SGPRs with the
// wave -- Makefile: -amdgpu-kernarg-preload-count=16 -- instead of being fetched by the block's first scalar loads)
__global__ __launch_bounds__(AI_BLOCK) void fk_spmv(const FTask* __restrict__ ftasks, int ntask, int J, double* const* __restrict__ slabs,
                                                    size_t stride, const int32_t* __restrict__ ucol, const uint16_t* __restrict__ lidx,
                                                    const double* __restrict__ wm, const double* __restrict__ sinv2, FlowLz L, FlowCsr G,
                                                    double* __restrict__ Z, double* __restrict__ pA,
                                                    unsigned long long* __restrict__ tstamp, unsigned long long* __restrict__ idle_ctr) {
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
  } stamp(STAMP ? tstamp : nullptr);
  const int t = ai_xcd_task(blockIdx.x, ntask);
  const FTask tk = ftasks[t];
  const int j = J - tk.t0;
  // (the second, never-true condition makes the whole record one load in front of the branch instead of t0 first and the rest
  // after it: one scalar round trip less in every block's dependent chain)
  if ((j < 0) | ((tk.lo | tk.hi | tk.flags | tk.pidx | tk.uoff) < 0) | (tk.vdelta == (int)0x80000000)) return;  // the segment starts at its own step
  const int par = (tk.flags >> 1) & 1;
  const int2* __restrict__ rowse = G.rowse[par];
  const double* __restrict__ Rj = fk_vec(slabs, stride, j) + tk.vdelta;  // indexed by position from here on
  // second round trip: activity flag, distinct-column list, row records, diagonal terms -- all in flight together
  // (agent-scope load: the flag is cleared by the check kernel and set by the harvest, both on other streams, at stable indices
  // that are re-used; a plain block-uniform load would go through the scalar cache, see fk_check)
  const int actv = __hip_atomic_load(&L.factive[tk.pidx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // waited for where it is used
  // (profiling instantiation only: blocks dispatched for a segment that froze since the lists were written -- they cost a record and a flag load)
  if (STAMP && !__builtin_amdgcn_readfirstlane(actv) && threadIdx.x == 0) atomicAdd(idle_ctr, 1ull);
  if (tk.ucnt < 0) {
    if (!__builtin_amdgcn_readfirstlane(actv)) return;
    fk_spmv_plain<ILP>(tk, rowse, G.col[par], wm, sinv2, Rj, Z, pA, sm);
    return;
  }
  int uc[AI_ENC_XCAP / AI_BLOCK];
#pragma unroll
  for (int q = 0; q < AI_ENC_XCAP / AI_BLOCK; ++q) {
    const int i = threadIdx.x + q * AI_BLOCK;
    uc[q] = (i < tk.ucnt) ? ucol[tk.uoff + i] : -1;
  }
  const int l = threadIdx.x & (LPR - 1), r = threadIdx.x / LPR;
  constexpr int GROUPS = AI_BLOCK / LPR;
  int p0[ILP], p1[ILP];
  double sum[ILP], ri[ILP], s2[ILP];
  int maxq = 0;
#pragma unroll
  for (int u = 0; u < ILP; ++u) {
    const int row = tk.lo + r + u * GROUPS;
    const bool ok = row < tk.hi;
    const int2 se = ok ? rowse[row] : make_int2(0, 0);
    p0[u] = se.x;
    p1[u] = se.y;
    ri[u] = (ok && l == 0) ? Rj[row] : 0.0;
    s2[u] = (ok && l == 0) ? sinv2[row] : 0.0;
    sum[u] = 0.0;
    maxq = max(maxq, ((p1[u] + 3) >> 2) - (p0[u] >> 2));
  }
  if (!__builtin_amdgcn_readfirstlane(actv)) return;
#pragma unroll
  for (int q = 0; q < AI_ENC_XCAP / AI_BLOCK; ++q)
    if (uc[q] >= 0) xs[threadIdx.x + q * AI_BLOCK] = Rj[uc[q]];
  const uint2* __restrict__ lidx4 = reinterpret_cast<const uint2*>(lidx);
  const double2* __restrict__ wm2 = reinterpret_cast<const double2*>(wm);
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
  for (int k = LPR; k < maxq; k += LPR) {
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
    const int row = tk.lo + r + u * GROUPS;
    if (l == 0 && row < tk.hi) {
      const double z = fma(s2[u], ri[u], sg);
      Z[row] = z;
      acc = fma(ri[u], z, acc);
    }
  }
  const double tot = ai_block_sum_first(acc, sm);  // (sm's only use in this kernel)
  if (threadIdx.x == 0) pA[tk.pidx] = tot;
}

// Two kernels freeze a segment: the convergence check (stream ss) at one of the segment's scheduled sizes of T, and the update
// kernel (stream sm) when a step finds the Krylov space exhausted (b_j = 0).  They race: a check that judges T_32 runs for
// tens of microseconds while steps 33 .. 36 of a small segment execute, and step 36 may be the exhausted one.  Until round 4
// both wrote L.m, the later one won, and the host (which takes the size from status[slot], written by the check only) and
// fk_pack_hist (which takes it from L.m) could disagree: 36 rows packed where the host expected 32 -- and, when 36 exceeded the
// wave's pitch, the excess landed on the head of the NEXT segment's row: that segment's theta, residual and first alphas
// replaced by this one's g values, its Ritz pair garbage (the soak's once-in-10^5 wrong cut; DESIGN_EXPERIMENTS F9).
// Now the size at which a segment freezes is a function of its history only: the smallest scheduled size at which the check
// finds it converged, else the exhausted step.  L.frozen: 0 running, 1 frozen by the check (final), 2 frozen by the update
// kernel at L.m = j_b -- scheduled sizes below j_b are still judged (fk_check's scan) and, if one converges, lower L.m.
__device__ __forceinline__ void fk_clear_flags(const FlowLz& L, int f0, int f1, int c0, int c1, int lane, int nlanes) {
  for (int t = f0 + lane; t < f1; t += nlanes) ai_st_agent(&L.factive[t], 0);
  for (int t = c0 + lane; t < c1; t += nlanes) ai_st_agent(&L.cactive[t], 0);
}
// the check's freeze: its size is never above an exhausted step's, so it overwrites
__device__ __forceinline__ void fk_freeze(const FlowLz& L, int s, int m, int f0, int f1, int c0, int c1, int lane, int nlanes) {
  if (lane == 0) {
    ai_st_agent(&L.m[s], (int32_t)m);
    __threadfence();
    ai_st_agent(&L.frozen[s], 1);
  }
  fk_clear_flags(L, f0, f1, c0, c1, lane, nlanes);
}
// the update kernel's freeze (Krylov space exhausted at step j): only if nothing has frozen the segment yet
__device__ __forceinline__ void fk_freeze_exhausted(const FlowLz& L, int s, int j, int f0, int f1, int c0, int c1, int lane, int nlanes) {
  if (lane == 0) {
    int32_t unset = 0;
    __hip_atomic_compare_exchange_strong(&L.m[s], &unset, (int32_t)j, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    int32_t running = 0;
    __hip_atomic_compare_exchange_strong(&L.frozen[s], &running, 2, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  fk_clear_flags(L, f0, f1, c0, c1, lane, nlanes);
}

// Step j = J - t0 of a segment, second launch (update_body of the lock-step driver): every block of the segment
// re-derives g_j, b_j, alpha_j from the partials in the same fixed order, forms R_{j+1} and its partials.
__global__ __launch_bounds__(AI_BLOCK) void fk_update(const CTask* __restrict__ ctasks, int J, FlowLz L, const double* __restrict__ pA,
                                                      double2* __restrict__ pB0, double2* __restrict__ pB1,
                                                      const double* __restrict__ u1, const double* __restrict__ Z,
                                                      double* const* __restrict__ slabs, size_t stride, int32_t* __restrict__ progress,
                                                      int32_t* __restrict__ dprog) {
  constexpr int RPT = AI_COARSE_ROWS / AI_BLOCK;
  __shared__ double sm3[3][AI_BLOCK / 64];
  // how far the device has come, for the host's run-ahead limit (pinned host memory; approximate by design)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // this launch has started, so every launch before it has finished: steps 0 .. J - 1 are complete.  The check kernel
    // (side stream, no event in between) judges only what that counter covers
    __hip_atomic_store(dprog, J, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((J & 1) == 1) __hip_atomic_store(progress, J + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  const CTask tk = ctasks[blockIdx.x];
  const int actv = __hip_atomic_load(&L.cactive[tk.pidx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // waited for after the row loads
  const int j = J - tk.t0;
  if (j < 0) return;
  if (j > tk.cap) return;  // the segment's Krylov space is exhausted at its own dimension (step `cap` only records b_cap)
  const int s = tk.slot;
  const double* __restrict__ Rj = fk_vec(slabs, stride, j) + tk.vdelta;
  const double* __restrict__ Rjm1 = fk_vec(slabs, stride, j > 0 ? j - 1 : 0) + tk.vdelta;
  double* __restrict__ Rnext = const_cast<double*>(fk_vec(slabs, stride, j + 1)) + tk.vdelta;
  const double2* __restrict__ pBcur = (j & 1) ? pB1 : pB0;
  double2* __restrict__ pBnext = (j & 1) ? pB0 : pB1;
  double zr[RPT], rr[RPT], rm[RPT], ur[RPT];
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int row = tk.lo + threadIdx.x + q * AI_BLOCK;
    const bool ok = row < tk.hi;
    zr[q] = ok ? Z[row] : 0.0;
    rr[q] = ok ? Rj[row] : 0.0;
    rm[q] = (ok && j > 0) ? Rjm1[row] : 0.0;
    ur[q] = ok ? u1[row] : 0.0;
  }
  // Everything the block needs is requested before anything is waited for: the rows above, the two history scalars, and the
  // segment's partials in batches of 8 (fine) / 4 (coarse) loads per thread.  (The plain loops "a += pA[t]" compiled to one load,
  // one wait per iteration: 24 dependent L2 round trips for a 200k-row segment, which made this launch slower than the SpMV it
  // follows.)  The sums are formed in the same order as before.
  double gpv = 0.0, bpv = 1.0;
  if (j > 0) {  // (every access to the histories is an agent-scope access: fk_check reads them from another stream, see there)
    gpv = __hip_atomic_load(&L.g_hist[(size_t)s * (L.mcap + 1) + j - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bpv = __hip_atomic_load(&L.b_hist[(size_t)s * (L.mcap + 1) + j - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  double a = 0.0, nn = 0.0, gg = 0.0;
  constexpr int UA = 8, UB = 4;
  for (int t0 = tk.f0 + threadIdx.x; t0 < tk.f1; t0 += UA * AI_BLOCK) {
    double v[UA];
#pragma unroll
    for (int u = 0; u < UA; ++u) {
      const int t = t0 + u * AI_BLOCK;
      v[u] = (t < tk.f1) ? pA[t] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < UA; ++u)
      if (t0 + u * AI_BLOCK < tk.f1) a += v[u];
  }
  for (int t0 = tk.c0 + threadIdx.x; t0 < tk.c1; t0 += UB * AI_BLOCK) {
    double2 v[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int t = t0 + u * AI_BLOCK;
      v[u] = (t < tk.c1) ? pBcur[t] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int u = 0; u < UB; ++u)
      if (t0 + u * AI_BLOCK < tk.c1) {
        nn += v[u].x;
        gg += v[u].y;
      }
  }
  if (!__builtin_amdgcn_readfirstlane(actv)) return;
  const double gp = gpv, rbp = (j > 0) ? 1.0 / bpv : 0.0;
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
  const double b = sqrt(fmax(nn - g * g, 0.0));
  if (j > 0 && !(b > 1e-14)) {
    if (tk.flags & 1) fk_freeze_exhausted(L, s, j, tk.f0, tk.f1, tk.c0, tk.c1, threadIdx.x, AI_BLOCK);
    return;
  }
  if (j == tk.cap) {  // T is complete: b_cap is all the convergence check still needs
    if ((tk.flags & 1) && threadIdx.x == 0)
      __hip_atomic_store(&L.b_hist[(size_t)s * (L.mcap + 1) + j], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const double rb = 1.0 / b;
  const double al = rb * rb * (a - g * g);
  if ((tk.flags & 1) && threadIdx.x == 0) {
    // write-through stores: the check kernel of another stream reads these while later steps run; a plain store would stay in
    // this XCD's L2 until the end of the launch
    __hip_atomic_store(&L.alpha_hist[(size_t)s * L.mcap + j], al, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&L.b_hist[(size_t)s * (L.mcap + 1) + j], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&L.g_hist[(size_t)s * (L.mcap + 1) + j], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifdef AI_TRACE_HIST
    if (j < 64) {
      L.sig_i[(size_t)s * 64 + j] = make_int4(J, tk.t0, tk.pidx, (int)blockIdx.x);
      L.sig_d[(size_t)s * 64 + j] = make_double2(a, al);
    }
#endif
  }
  double n2 = 0.0, g2 = 0.0;
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int row = tk.lo + threadIdx.x + q * AI_BLOCK;
    if (row < tk.hi) {
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
    pBnext[tk.pidx] = make_double2(tn, tg);
  }
}

// Convergence check of every pool segment after J launched steps (k_lz_check of the lock-step driver).  Step j = m of a
// segment recorded b_m = ||R_m - g_m u1||, so after J launches T_m with m = J - t0 - 1 rows can be judged.
// lastm[slot] = rows at the previous check (work counters, warm start validity).
// Every segment carries the size of T it wants judged next (nextm[slot]; 16 at the start).  A launch judges exactly THAT
// T_m from the kept history as soon as the segment has got that far -- however late the launch comes -- and then picks the
// next size from the residual trend (geometric extrapolation to tol, aimed a little early; superlinear convergence and
// the re-aim make the last check land within a few steps of convergence).  The sizes of T at which a segment can freeze,
// hence its Ritz vector bit for bit, are a function of its own history only, not of when the host launched what.
// The launch is not ordered against the stepping stream: it reads the device's own step counter (written by the update
// kernel: steps below it are complete) and the histories with agent-scope loads.  A frozen segment's size of T goes
// straight into pinned host memory (status[slot]).
// Round 4: a launch no longer spends a block on every pool segment.  Most segments of a launch are not due (a solve is judged ~8
// times in its life, a launch comes every 4th step), yet until round 3 every one of them cost a 256-thread block with the launch's
// full LDS allocation (3 x 8 B x the oldest segment's steps: up to 96 KB, i.e. one block per CU), 800 blocks per launch of a
// 12-chunk pool: 67 us per launch, 20 % of the device's kernel time, beside the SpMV whose vector ALUs are already half busy.
// Now the first ceil(npool / 256) blocks SCAN the pool one segment per thread (pool entry, frozen flag, next size of T: agent-scope
// vector loads, which also keeps them out of the scalar cache) and queue the due ones; the other FK_CHECK_JUDGES blocks wait for
// the scan (its blocks are dispatched first, so they are running) and judge the queue, one segment per block at a time, with exactly
// the arithmetic of before: same T_m, same multisection, same recurrence, so the same sizes of T at the freeze.
// ctr: 8 x {queued, scan blocks done} -- launch L uses entry L & 7 and zeroes entry (L + 1) & 7 (launches are serialised on their stream).
// ---- fk_check's arithmetic, round 5: WAVE-PARALLEL three-term recurrences.
// Both halves of a judgment are recurrences x_{i+1} = t_i x_i - e_i x_{i-1} over the m rows of T: the Sturm sequence p_i = det(T_i - x I)
// whose sign changes count the eigenvalues below x, and the eigenvector recurrence from the last component upwards.  Until round 4 one
// thread walked all m rows per probe (256 probes per sweep, ~5 sweeps of m dependent rows per judgment, then m more rows on one
// wave for the vector): 75 us per launch, a fifth of the device's kernel time, and on every solve's critical path.  The recurrences
// are LINEAR in (x_i, x_{i-1}), so a wave can walk them in m / 64 dependent steps: every lane multiplies the 2 x 2 transfer matrices
// of its own ceil(m / 64) rows, an inclusive scan over the lanes (6 shuffle steps) gives every lane the state its rows start from,
// and a second walk of the lane's rows produces what is wanted (sign changes; sums of squares).  One probe per wave and round instead
// of 256 per block, but a round is ~m / 20 times shorter: 2.3 bits of the eigenvalue per ~1 us instead of 8 bits per ~m x 25 ns.
struct M22 {
  double a, b, c, d;  // (x', y') = (a x + b y, c x + d y)
};
__device__ __forceinline__ M22 m22_mul(const M22& L, const M22& R) {  // L after R
  return M22{fma(L.a, R.a, L.b * R.c), fma(L.a, R.b, L.b * R.d), fma(L.c, R.a, L.d * R.c), fma(L.c, R.b, L.d * R.d)};
}
// positive power-of-two rescale (exact): for the Sturm sequence only signs matter
__device__ __forceinline__ void m22_norm(M22& M) {
  const double mx = fmax(fmax(fabs(M.a), fabs(M.b)), fmax(fabs(M.c), fabs(M.d)));
  int e = 0;
  (void)frexp(mx, &e);
  M.a = ldexp(M.a, -e);
  M.b = ldexp(M.b, -e);
  M.c = ldexp(M.c, -e);
  M.d = ldexp(M.d, -e);
}
// inclusive prefix over the lanes of a wave: P_l = M_l M_{l-1} ... M_0
template <bool NORM>
__device__ __forceinline__ M22 m22_scan(M22 P, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const M22 O{__shfl_up(P.a, d, 64), __shfl_up(P.b, d, 64), __shfl_up(P.c, d, 64), __shfl_up(P.d, d, 64)};
    if (lane >= d) {
      P = m22_mul(P, O);
      if (NORM) m22_norm(P);
    }
  }
  return P;
}
// T in LDS, lane-interleaved: row i = L c + j (lane L's j-th row, c = ceil(m / 64) rows per lane) lives at j * 64 + L, so that the 64
// lanes of a wave, each at the j-th row of its own chunk, read 64 consecutive doubles (row-major order would put them c * 8 bytes
// apart: for c = 16 every lane on the same bank, each LDS read serialised 64-fold).  For m <= 64, c = 1 and the layout is the plain one.
#define FK_TIX(i, c) (((i) % (c)) * 64 + (i) / (c))
// Number of eigenvalues of T_m (diagonal a, squared off-diagonals bb (bb of row 0 = 0), both in LDS in the FK_TIX layout) below x, by ONE
// WAVE (the same count as sturm_lt; every lane returns it).  c = ceil(m / 64) rows per lane.
__device__ __forceinline__ int fk_sturm_wave(const double* a, const double* bb, int m, int c, double x, int lane) {
  const int i0 = min(lane * c, m), i1 = min(i0 + c, m);
  a += lane - i0 * 64;   // row i of this lane: a[(i - i0) * 64 + lane] = a[i * 64]
  bb += lane - i0 * 64;
  // walk 1: transfer matrix of the lane's rows, (p_{i+1}, p_i) = [[a_i - x, -bb_i], [1, 0]] (p_i, p_{i-1})
  M22 M{1.0, 0.0, 0.0, 1.0};
  for (int i = i0; i < i1; ++i) {
    const double t = a[i * 64] - x, b2 = bb[i * 64];
    const double na = fma(t, M.a, -(b2 * M.c)), nb = fma(t, M.b, -(b2 * M.d));
    M.c = M.a;
    M.d = M.b;
    M.a = na;
    M.b = nb;
    if (((i - i0) & 7) == 7) m22_norm(M);  // (|a - x| + b^2 < 4: eight rows move the magnitudes by < 2^16 upwards; downwards the rescale leaves 300 decades)
  }
  m22_norm(M);
  const M22 P = m22_scan<true>(M, lane);
  // state in front of the lane's first row: the first column of P_{lane-1} applied to (p_0, p_{-1}) = (1, 0)
  double p = __shfl_up(P.a, 1, 64), q = __shfl_up(P.c, 1, 64);
  if (lane == 0) {
    p = 1.0;
    q = 0.0;
  }
  if (p == 0.0) p = (q > 0.0) ? -1e-300 : 1e-300;  // a zero takes the sign opposite to its predecessor (as in sturm_lt)
  // walk 2: the lane's p_i and their sign changes
  const bool in_neg = p < 0.0;
  bool cur_neg = in_neg, first_neg = in_neg;
  int cnt = 0;
  for (int i = i0; i < i1; ++i) {
    double pn = fma(a[i * 64] - x, p, -(bb[i * 64] * q));
    if (pn == 0.0) pn = cur_neg ? 1e-300 : -1e-300;
    const bool nn = pn < 0.0;
    cnt += (nn != cur_neg) ? 1 : 0;
    if (i == i0) first_neg = nn;
    q = p;
    p = pn;
    cur_neg = nn;
    if (((i - i0) & 7) == 7) {
      int e = 0;
      (void)frexp(fmax(fabs(p), fabs(q)), &e);
      p = ldexp(p, -e);
      q = ldexp(q, -e);
    }
  }
  // The sign of p_{i0} this lane started from came out of the scan; the previous lane ARRIVED at p_{i0} by its own walk.  In exact
  // arithmetic they agree; when p_{i0} is nearly zero (x within rounding of an eigenvalue of the leading i0 rows) they may not, and a
  // chain that changes its mind at a lane boundary would miscount by one.  So the previous lane's sign is the predecessor of this
  // lane's first row: the chain of signs that is counted is then one chain, whatever the scan rounded.  (p_{i0+1} ~ -bb p_{i0-1}
  // there, so it does not depend on which sign p_{i0} was given.)
  const int prev_neg = __shfl_up((int)cur_neg, 1, 64);
  if (lane > 0 && i1 > i0) cnt += ((first_neg != (prev_neg != 0)) ? 1 : 0) - ((first_neg != in_neg) ? 1 : 0);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  return cnt;
}
// sum_k s_k^2 of the eigenvector recurrence of T_m at theta, normalised to s_{m-1} = 1 (so |s_{m-1}| / ||s|| = 1 / sqrt of it), by
// ONE WAVE: row k = m - 1 .. 1 gives s_{k-1} = ((theta - a_k) s_k - b_{k+1} s_{k+1}) / b_k.  Lane l walks the rows of chunk L = 63 - l of
// the FK_TIX layout downwards (the recurrence starts at the last row, so the chunks come in descending order), twice over at once
// -- from the states (1, 0) and (0, 1) -- keeping the three sums of squares and products, so that after the scan its share of the
// sum is a quadratic form in the state it starts from.  rb = 1 / b in LDS.  Returns a non-finite or huge value when the plain-double
// products overflowed (|s_{m-1}| below 1e-140 of the norm): the caller then walks the rows serially with rescaling, as until round 4.
__device__ __forceinline__ double fk_vec_sumsq_wave(const double* a, const double* bb, const double* rb, int m, int c, double theta, int lane) {
  const int L = 63 - lane;
  const int khi = min(L * c + c, m) - 1, klo = max(L * c, 1);   // rows khi .. klo (none when khi < klo)
  double f1 = 1.0, f0 = 0.0, h1 = 0.0, h0 = 1.0, F = 0.0, H = 0.0, X = 0.0;
  for (int k = khi; k >= klo; --k) {
    const int ix = FK_TIX(k, c), ixu = FK_TIX(k + 1, c);
    const double ct = theta - a[ix], et = (k + 1 < m) ? bb[ixu] * rb[ixu] : 0.0, rt = rb[ix];
    const double nf = (ct * f1 - et * f0) * rt, nh = (ct * h1 - et * h0) * rt;
    f0 = f1;
    f1 = nf;
    h0 = h1;
    h1 = nh;
    F = fma(nf, nf, F);
    H = fma(nh, nh, H);
    X = fma(nf, nh, X);
  }
  const M22 P = m22_scan<false>(M22{f1, h1, f0, h0}, lane);
  double u = __shfl_up(P.a, 1, 64), v = __shfl_up(P.c, 1, 64);
  if (lane == 0) {
    u = 1.0;
    v = 0.0;
  }
  double sh = (khi >= klo) ? (u * u) * F + 2.0 * (u * v) * X + (v * v) * H : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sh += __shfl_xor(sh, o, 64);  // (fixed order: the same bits run to run)
  return 1.0 + sh;
}

#define FK_CHECK_JUDGES 96
#define FK_CHECK_WIDE_M 64   // sizes of T up to which a sweep is 256 serial probes (above: one wave-parallel probe per wave)
__global__ __launch_bounds__(AI_CHECK_THREADS) void fk_check(const PoolSeg* __restrict__ pool, int npool, int launch, int32_t* __restrict__ ctr,
                                                             int32_t* __restrict__ queue, const int32_t* __restrict__ dprog, FlowLz L, FlowCsr G,
                                                             double tol, int lds_m,
                                                             double* __restrict__ theta_out, double* __restrict__ resid_out,
                                                             int32_t* __restrict__ lastm, int32_t* __restrict__ nextm,
                                                             unsigned long long* __restrict__ work, int with_rb,
                                                             int32_t* __restrict__ status) {
  constexpr int NT = AI_CHECK_THREADS, NW = NT / 64;
  __shared__ double smm[2][NW];
  __shared__ int sfirst[2][NW];
  __shared__ int32_t sh_i[16];
  __shared__ double sh_d[2];
  extern __shared__ double lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nscan = (npool + NT - 1) / NT;
  int32_t* my = ctr + 2 * (launch & 7);
  if ((int)blockIdx.x < nscan) {
    const int J = __hip_atomic_load(const_cast<int32_t*>(dprog), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // steps 0 .. J - 1 are complete
    const int i = blockIdx.x * NT + tid;
    if (blockIdx.x == 0 && tid == 0) {
      int32_t* nx = ctr + 2 * ((launch + 1) & 7);
      __hip_atomic_store(nx, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(nx + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (i < npool) {
      const int32_t* pw = (const int32_t*)&pool[i];
      const int s_ = __hip_atomic_load(pw + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int t0_ = __hip_atomic_load(pw + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int cap_ = __hip_atomic_load(pw + 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int fz = __hip_atomic_load(&L.frozen[s_], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);  // (L.m is read after it)
      const int nm = __hip_atomic_load(&nextm[s_], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int m_ = min(nm, min(cap_, L.mcap));
      bool due;
      if (fz) {
        const int mfz = __hip_atomic_load(&L.m[s_], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // frozen by a check (1: final, already reported) or by the update kernel at the exhausted step mfz (2): a scheduled size
        // below mfz is still judged -- whether this launch or the update kernel got there first must not decide the size of T
        due = (fz == 2) && m_ < mfz;
        if (!due) status[s_] = max(mfz, 1);
      } else {
        const int avail = J - t0_ - 1;  // step j = m records b_m: T_m can be judged after m + 1 steps
        due = avail > 0 && avail >= m_;
      }
      if (due) {
        const int q = __hip_atomic_fetch_add(my, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&queue[q], i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();
    if (tid == 0) {
      __threadfence();
      __hip_atomic_fetch_add(my + 1, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  // ---- judges
  if (tid == 0) {
    int spins = 0;
    while (__hip_atomic_load(my + 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < nscan && ++spins < (1 << 22)) __builtin_amdgcn_s_sleep(4);
    sh_i[15] = (spins < (1 << 22)) ? __hip_atomic_load(my, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;  // (a scan that never finishes: judge nothing)
    if (spins >= (1 << 22)) atomicAdd(&work[2], 1ull);  // counted: ai_ncut_stats.check_timeouts
  }
  __syncthreads();
  const int nd = sh_i[15];
  {
    for (int d = (int)blockIdx.x - nscan; d < nd; d += FK_CHECK_JUDGES) {
      __syncthreads();  // the previous segment's LDS (T, hand-off words) has been consumed
      // Everything another launch may have written since this block's CU last looked -- the pool entry (its list buffer is rewritten
      // every RING relists), the slot's check state -- is loaded ONCE, by one thread, with agent-scope loads, and handed to the
      // block through LDS.  The compiler turns block-uniform plain loads of such data into scalar loads, each wave issuing its own
      // through the scalar cache, which is not coherent: about once in 50 000 solves the waves of a block disagreed on the slot or
      // on the size of T (one wave read another segment's history), the bisection returned garbage and the segment froze at a size
      // of T that depended on timing -- once in a few thousand chunks at a wrong one.
      if (tid == 0) {
        const int32_t* pw = (const int32_t*)&pool[__hip_atomic_load(&queue[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)];
        for (int k = 0; k < 10; ++k) sh_i[k] = __hip_atomic_load(pw + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int s0 = sh_i[0];
        sh_i[12] = __hip_atomic_load(&nextm[s0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sh_i[13] = __hip_atomic_load(&lastm[s0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sh_d[0] = __hip_atomic_load(&theta_out[s0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sh_d[1] = __hip_atomic_load(&resid_out[s0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
      PoolSeg ps;
      ps.slot = sh_i[0], ps.n = sh_i[1], ps.g0 = sh_i[2], ps.t0 = sh_i[3], ps.f0 = sh_i[4], ps.f1 = sh_i[5], ps.c0 = sh_i[6], ps.c1 = sh_i[7];
      ps.cap = sh_i[8], ps.par = sh_i[9];
      const int s = ps.slot;
      const int cap = min(ps.cap, L.mcap);
      const int m = min(sh_i[12], cap);
      const int c = (m + 63) >> 6;       // rows of T per lane of a wave (FK_TIX layout)
      if (64 * c > lds_m || m < 1) continue;  // cannot happen: the host sizes the LDS for the oldest segment of the pool, rounded up to 64 rows (block-uniform)
      const double bnew = __hip_atomic_load(&L.b_hist[(size_t)s * (L.mcap + 1) + m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool last = (m >= cap) || !(bnew > 1e-14);
      const int prev_m = sh_i[13];
      if (tid == 0) {
        const int since = max(m - prev_m, 0);
        atomicAdd(&work[0], (unsigned long long)ps.n * (unsigned long long)since);
        const int2* rs = G.rowse[ps.par];
        atomicAdd(&work[1], (unsigned long long)(rs[ps.g0 + ps.n - 1].y - rs[ps.g0].x) * (unsigned long long)since);
      }
      const double* bh = L.b_hist + (size_t)s * (L.mcap + 1);
      const double* ah = L.alpha_hist + (size_t)s * L.mcap;
      double* la = lds;
      double* lbb = lds + lds_m;
      double* lrb = lds + 2 * lds_m;
      double lo = -1e300, hi = -1e300;
      for (int i = tid; i < m; i += NT) {
        const double ai = __hip_atomic_load(&ah[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double bi = (i > 0) ? __hip_atomic_load(&bh[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        const double br = (i + 1 < m) ? __hip_atomic_load(&bh[i + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
        const int ix = FK_TIX(i, c);
        la[ix] = ai;
        lbb[ix] = bi * bi;
        if (with_rb) lrb[ix] = 1.0 / bi;  // the upward recurrence below multiplies by 1 / b_k (b_0 is never used) and forms b_{k+1} = b^2 / b
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
      int phase = 0;
      auto first_above = [&](bool mine) -> int {
        const unsigned long long above = __ballot(mine);
        if (lane == 0) sfirst[phase][wv] = above ? wv * 64 + __ffsll((long long)above) - 1 : (1 << 30);
        __syncthreads();
        int jj = 1 << 30;
#pragma unroll
        for (int w = 0; w < NW; ++w) jj = min(jj, sfirst[phase][w]);
        phase ^= 1;
        return (jj == (1 << 30)) ? -1 : jj;
      };
      const double tprev = sh_d[0], rprev = sh_d[1];
      const bool warm = prev_m > 0 && tprev > 0.0 && rprev > 0.0;
      int rounds = 0;
      if (m <= FK_CHECK_WIDE_M) {
        // ---- a small T: 256 probes per sweep, one thread per probe walks the m rows (sturm_lt)
        // warm start from this solve's previous check (T only grew: its top eigenvalue did not decrease)
        if (warm) {
          const double hi_g = hi, eps = 1e-15 * fmax(fabs(tprev), 1.0);
          const double lo_w = fmax(lo, tprev - 1e-14 * fmax(fabs(tprev), 1.0));
          const double x = fmin(hi_g, tprev + ldexp(rprev, tid) + eps);
          const int j0 = first_above(sturm_lt(la, lbb, m, x) == m);
          lo = lo_w;
          if (j0 >= 0) {
            hi = fmin(hi_g, tprev + ldexp(rprev, j0) + eps);
            if (j0 > 0) lo = fmax(lo_w, fmin(hi_g, tprev + ldexp(rprev, j0 - 1) + eps));
          }
          ++rounds;
        }
        for (int round = 0; round < 12; ++round) {
          if (hi - lo <= 5e-14 * fmax(fabs(hi), 1e-300)) break;
          const double w = (hi - lo) * (1.0 / (NT + 1));
          const double x = lo + (tid + 1) * w;
          const int j0 = first_above(sturm_lt(la, lbb, m, x) == m);
          if (j0 < 0) {
            lo = lo + (double)NT * w;
          } else {
            hi = lo + (j0 + 1) * w;
            lo = lo + j0 * w;
          }
          ++rounds;
        }
      } else {
        // ---- one probe per WAVE and round (fk_sturm_wave).  The top eigenvalue moved by ~resid^2 / gap since the previous check:
        // a geometric ladder of four probes from the previous value (steps of 16 from 16 resid^2, never below what the stopping
        // width resolves) brackets it within a factor 16, five-section rounds finish.  Late in a solve that is 1-3 rounds.
        bool geo = true;
        double g;
        if (warm) {
          lo = fmax(lo, tprev - 1e-14 * fmax(fabs(tprev), 1.0));
          g = fmax(16.0 * rprev * rprev, 2.5e-14 * fmax(fabs(tprev), 1.0));
        } else {
          g = (hi - lo) * (1.0 / 4096.0);
        }
        for (int round = 0; round < 80; ++round) {
          const double width = hi - lo;
          if (width <= 5e-14 * fmax(fabs(hi), 1e-300)) break;
          if (geo && g * 4096.0 >= width) geo = false;  // the ladder would overshoot the bracket: plain sections
          double x0, x1, x2, x3;
          if (geo) {
            x0 = lo + g, x1 = lo + 16.0 * g, x2 = lo + 256.0 * g, x3 = lo + 4096.0 * g;
          } else {
            const double w5 = width * 0.2;
            x0 = lo + w5, x1 = lo + 2.0 * w5, x2 = lo + 3.0 * w5, x3 = lo + 4.0 * w5;
          }
          const double x = (wv == 0) ? x0 : (wv == 1) ? x1 : (wv == 2) ? x2 : x3;
          // (a probe that rounding put outside the open bracket has a known answer)
          const bool above = (x >= hi) ? true : (x <= lo) ? false : (fk_sturm_wave(la, lbb, m, c, x, lane) == m);
          const int j0 = first_above(above);   // first LANE of the block that is above: its wave is the first probe above
          const int w0 = (j0 < 0) ? -1 : (j0 >> 6);
          const double xl = (w0 <= 0) ? lo : (w0 == 1) ? x0 : (w0 == 2) ? x1 : x2;
          if (w0 < 0) {
            lo = fmax(lo, x3);
            if (geo) g *= 65536.0;
          } else {
            hi = fmin(hi, (w0 == 0) ? x0 : (w0 == 1) ? x1 : (w0 == 2) ? x2 : x3);
            lo = fmax(lo, xl);
            geo = false;
          }
          ++rounds;
        }
      }
      if (wv == 0) {
        const double theta = 0.5 * (lo + hi);
        double sumsq = with_rb ? fk_vec_sumsq_wave(la, lbb, lrb, m, c, theta, lane) : -1.0;
        double scale = 1.0;
        if (!(sumsq >= 1.0 && sumsq < 1e280)) {
          // the serial walk with rescaling (the arithmetic of rounds 1-4): T too large for the reciprocals in LDS, or a last component
          // more than 140 decades below the norm
          double sk1 = 0.0, sk = 1.0;
          sumsq = 1.0;
#pragma unroll 4
          for (int k = m - 1; k >= 1; --k) {
            double sm1;
            if (with_rb) {
              const double bu = (k + 1 < m) ? lbb[FK_TIX(k + 1, c)] * lrb[FK_TIX(k + 1, c)] : 0.0;
              sm1 = ((theta - la[FK_TIX(k, c)]) * sk - bu * sk1) * lrb[FK_TIX(k, c)];
            } else {
              const double bk = __hip_atomic_load(&bh[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              const double bu = (k + 1 < m) ? __hip_atomic_load(&bh[k + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
              sm1 = ((theta - la[FK_TIX(k, c)]) * sk - bu * sk1) / bk;
            }
            sk1 = sk;
            sk = sm1;
            sumsq += sk * sk;
            if (sumsq > 1e200) {
              sk *= 1e-100;
              sk1 *= 1e-100;
              sumsq *= 1e-200;
              scale *= 1e-100;
            }
          }
        }
        const double resid = bnew * scale / sqrt(sumsq);
        if (lane == 0) atomicAdd(&work[3], (unsigned long long)rounds);
        if (lane == 0) atomicAdd(&work[4], 1ull);
        if (lane == 0) __hip_atomic_store(&lastm[s], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (resid <= tol || last) {
#ifdef AI_TRACE_HIST
          if (lane == 0) {
            L.chk_i[s] = make_int4(__hip_atomic_load(const_cast<int32_t*>(dprog), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), m, prev_m, launch);
            double* cd = L.chk_d + (size_t)s * 8;
            cd[0] = theta, cd[1] = resid, cd[2] = la[0], cd[3] = la[FK_TIX(m > 1 ? 1 : 0, c)], cd[4] = la[FK_TIX(m - 1, c)], cd[5] = lbb[FK_TIX(m > 1 ? 1 : 0, c)], cd[6] = bnew, cd[7] = sumsq;
          }
#endif
          if (lane == 0) {
            __hip_atomic_store(&theta_out[s], theta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&resid_out[s], resid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          fk_freeze(L, s, m, ps.f0, ps.f1, ps.c0, ps.c1, lane, 64);
          if (lane == 0) {
            __threadfence_system();
            status[s] = max(m, 1);
          }
        } else if (lane == 0) {
          // next size of T: steps to tol at the rate of the last interval, aimed at 3/4 of that (4 .. 48 steps); 16 while the
          // residual is not falling yet
          int inc = 16;
          if (prev_m > 0 && rprev > 0.0 && resid < rprev) {
            const double rate = log(rprev / resid) / (double)(m - prev_m);
            const double need = log(resid / tol) / rate;
            inc = (int)ceil(0.75 * need);
            inc = max(4, min(inc, 48));
          }
          __hip_atomic_store(&nextm[s], m + inc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(&theta_out[s], theta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          __hip_atomic_store(&resid_out[s], resid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
    }
  }
}


// ----------------------------------------------------------------------------- harvest: Ritz vector
// T of the harvested segments for the host, rows of pitch 3 * mp + FK_HIST_HEAD doubles: {theta, resid, m, checksum, alpha[mp], b[mp], g[mp]}
__global__ __launch_bounds__(AI_BLOCK) void fk_pack_hist(const SegRec* __restrict__ recs, FlowLz L, const double* __restrict__ theta,
                                                         const double* __restrict__ resid, int mp, double* __restrict__ out) {
  // Row of segment i in pinned host memory: {theta, resid, m, checksum, a[mp], b[mp], g[mp]}.  m is the DEVICE's size of T (the host
  // has its own copy from status[slot] and compares), the checksum is the sum of the 64-bit patterns of everything else in the row
  // (integer addition: any order).  Round 4's soaks saw, twice in 140 000 chunk cuts, a row whose first 32 / 112 bytes held
  // g-like values of another row when the host read it (DESIGN_EXPERIMENTS F9): with the header the host knows before it
  // uses a row, asks for the rows again, and counts the event (stats.hist_retries).
  __shared__ unsigned long long smu[AI_BLOCK / 64];
  const int s = recs[blockIdx.x].slot;
  // written by the check kernel on another stream: agent-scope loads, not the scalar cache (see fk_check)
  const int m = __hip_atomic_load(&L.m[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  double* o = out + (size_t)blockIdx.x * (3 * (size_t)mp + FK_HIST_HEAD);
  unsigned long long acc = 0;
  double th = 0.0, rs = 0.0;
  if (threadIdx.x == 0) {
    th = __hip_atomic_load(const_cast<double*>(&theta[s]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    rs = __hip_atomic_load(const_cast<double*>(&resid[s]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    acc = (unsigned long long)__double_as_longlong(th) + (unsigned long long)__double_as_longlong(rs) + (unsigned long long)(long long)m;
  }
  const double* a = L.alpha_hist + (size_t)s * L.mcap;
  const double* b = L.b_hist + (size_t)s * (L.mcap + 1);
  const double* g = L.g_hist + (size_t)s * (L.mcap + 1);
  const int mw = min(m, mp);  // (a size of T beyond the wave's pitch is the host's to report: never write past the row)
  for (int i = threadIdx.x; i < mw; i += AI_BLOCK) {
    const double av = __hip_atomic_load(const_cast<double*>(&a[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double bv = __hip_atomic_load(const_cast<double*>(&b[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double gv = __hip_atomic_load(const_cast<double*>(&g[i]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    o[FK_HIST_HEAD + i] = av;
    o[FK_HIST_HEAD + mp + i] = bv;
    o[FK_HIST_HEAD + 2 * mp + i] = gv;
    acc += (unsigned long long)__double_as_longlong(av) + (unsigned long long)__double_as_longlong(bv) + (unsigned long long)__double_as_longlong(gv);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) smu[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long tot = 0;
#pragma unroll
    for (int w = 0; w < AI_BLOCK / 64; ++w) tot += smu[w];
    o[0] = th;
    o[1] = rs;
    o[2] = (double)m;
    o[3] = __longlong_as_double((long long)tot);
  }
}

// ev = sum_j coef_j R_j + cu u1 for the rows of the harvested segments (one slab of vectors per launch);
// coef rows are wave-local: coef[wi][mp], wi = Task.z
__global__ __launch_bounds__(AI_BLOCK) void fk_ritz(const Task* __restrict__ ctasks, const SegRec* __restrict__ recs, const int32_t* __restrict__ wm_, const double* __restrict__ coef,
                                                    int mp, const double* __restrict__ cu, const double* __restrict__ u1,
                                                    double* const* __restrict__ slabs, size_t stride, double* __restrict__ ev,
                                                    const double* __restrict__ coef2, const double* __restrict__ cu2, double* __restrict__ ev2) {
  // ONE launch per wave: every block walks its segment's m vectors through the slab table (a launch per 32-vector slab, as until
  // round 3, was up to 15 launches per wave and ~1 100 per 12-chunk call: 4 ms of the host's launch time).  Same order of the
  // fused multiply-adds, so the same bits.
  const Task tk = ctasks[blockIdx.x];
  const int wi = tk.z;
  const int m = wm_[wi];
  const double* cs = coef + (size_t)wi * mp;
  const int vd = recs[wi].vdelta;
  constexpr int RPT = AI_COARSE_ROWS / AI_BLOCK;
  double acc[RPT];
  int row[RPT];
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    row[q] = tk.x + threadIdx.x + q * AI_BLOCK;
    acc[q] = (row[q] < tk.y) ? cu[wi] * u1[row[q]] : 0.0;
    if (row[q] >= tk.y) row[q] = tk.x;  // (a valid address; the value is not stored)
  }
  if (ev2 == nullptr) {
    for (int j0 = 0; j0 < m; j0 += AI_SLAB_VECS) {
      const double* __restrict__ slab = slabs[j0 / AI_SLAB_VECS] + vd;
      const int jn = min(AI_SLAB_VECS, m - j0);
#pragma unroll 8
      for (int j = 0; j < jn; ++j) {
        const double c = cs[j0 + j];
#pragma unroll
        for (int q = 0; q < RPT; ++q) acc[q] = fma(c, slab[(size_t)j * stride + row[q]], acc[q]);
      }
    }
  } else {
    // the SECOND Ritz vector from the same pass over the kept Lanczos vectors (the children's warm start: fk_lz_init)
    const double* cs2 = coef2 + (size_t)wi * mp;
    double acc2[RPT];
#pragma unroll
    for (int q = 0; q < RPT; ++q) acc2[q] = (tk.x + threadIdx.x + q * AI_BLOCK < tk.y) ? cu2[wi] * u1[row[q]] : 0.0;
    for (int j0 = 0; j0 < m; j0 += AI_SLAB_VECS) {
      const double* __restrict__ slab = slabs[j0 / AI_SLAB_VECS] + vd;
      const int jn = min(AI_SLAB_VECS, m - j0);
#pragma unroll 4
      for (int j = 0; j < jn; ++j) {
        const double c = cs[j0 + j], c2 = cs2[j0 + j];
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
          const double x = slab[(size_t)j * stride + row[q]];
          acc[q] = fma(c, x, acc[q]);
          acc2[q] = fma(c2, x, acc2[q]);
        }
      }
    }
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      const int r = tk.x + threadIdx.x + q * AI_BLOCK;
      if (r < tk.y) ev2[r] = acc2[q];
    }
  }
#pragma unroll
  for (int q = 0; q < RPT; ++q) {
    const int r = tk.x + threadIdx.x + q * AI_BLOCK;
    if (r < tk.y) ev[r] = acc[q];
  }
}

// rows of the wave's disconnected segments: their warm vector into the staging array the partition permutes from
__global__ __launch_bounds__(AI_BLOCK) void fk_copy_rows(const Task* __restrict__ ctasks, const double* __restrict__ src, double* __restrict__ dst) {
  const Task tk = ctasks[blockIdx.x];
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) dst[row] = src[row];
}

// ----------------------------------------------------------------------------- harvest: the TRUE residual of the Ritz pair
// ||M ev - theta ev|| / ||ev|| of every harvested segment, formed from the segment's own graph: the Lanczos residual estimate
// that froze the segment is a statement about T_m, this one is about the vector that is about to be cut.  One pass over the
// segment's entries (the sweep makes another); partials per fine task: {sum r^2, sum ev^2}.  A converged segment whose true
// residual is orders of magnitude above the tolerance was frozen on bad data: the host solves it again from scratch (the same
// start vector, hence the same bits as an undisturbed solve) instead of cutting a wrong vector -- Flow::wave_s3.
__global__ __launch_bounds__(AI_BLOCK) void fk_resid(const Task* __restrict__ ftasks, FlowCsr G, const double* __restrict__ wm,
                                                     const double* __restrict__ sinv2, const double* __restrict__ ev,
                                                     const double* __restrict__ theta, double2* __restrict__ part) {
  __shared__ double sm[AI_BLOCK / 64];
  const Task tk = ftasks[blockIdx.x];
  const int2* __restrict__ rowse = G.rowse[FK_PAR(tk)];
  const int32_t* __restrict__ col = G.col[FK_PAR(tk)];
  const double th = theta[tk.z];
  const int l = threadIdx.x & (AI_LPR - 1), r = threadIdx.x / AI_LPR;
  double rr = 0.0, ee = 0.0;
  for (int row = tk.x + r; row < tk.y; row += AI_BLOCK / AI_LPR) {
    const int2 se = rowse[row];
    double z = 0.0;
    for (int p = se.x + l; p < se.y; p += AI_LPR) z = fma(wm[p], ev[col[p]], z);
    z = ai_group16_sum(z);
    if (l == 0) {
      const double e = ev[row];
      const double res = fma(sinv2[row], e, z) - th * e;
      rr = fma(res, res, rr);
      ee = fma(e, e, ee);
    }
  }
  const double trr = ai_block_sum(rr, sm);
  const double tee = ai_block_sum(ee, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = make_double2(trr, tee);
}
// per harvested segment: sqrt(sum r^2 / sum ev^2) straight into pinned memory
__global__ __launch_bounds__(AI_BLOCK) void fk_resid_final(const SegRec* __restrict__ recs, const double2* __restrict__ part, double* __restrict__ out) {
  __shared__ double sm[AI_BLOCK / 64];
  const SegRec sr = recs[blockIdx.x];
  double rr = 0.0, ee = 0.0;
  for (int t = sr.foff + threadIdx.x; t < sr.foff + FK_NF(sr); t += AI_BLOCK) {
    const double2 v = part[t];
    rr += v.x;
    ee += v.y;
  }
  const double trr = ai_block_sum(rr, sm);
  const double tee = ai_block_sum(ee, sm);
  if (threadIdx.x == 0) out[blockIdx.x] = (tee > 0.0) ? sqrt(trr / tee) : 1e300;
}

// ----------------------------------------------------------------------------- harvest: threshold sweep (normalized_cut.py:13-34)
__global__ __launch_bounds__(AI_BLOCK) void fk_minmax(const Task* __restrict__ ctasks, FlowCsr G, const double* __restrict__ ev,
                                                      MinMaxPart* __restrict__ part) {
  const Task tk = ctasks[blockIdx.x];
  minmax_body(tk, ev, G.orig[FK_PAR(tk)], part);
}

// per record i: scale, np.allclose test, the 10 thresholds
__global__ void fk_minmax_final(const SegRec* __restrict__ recs, const MinMaxPart* __restrict__ part,
                                int S, double* __restrict__ scale, int32_t* __restrict__ nosplit, double* __restrict__ thr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= S) return;
  const SegRec sr = recs[i];
  minmax_final_body(part, sr.coff, sr.coff + FK_NC(sr), 0, i, scale, nosplit, thr);
}

__global__ __launch_bounds__(AI_BLOCK) void fk_sweep(const Task* __restrict__ ftasks, const int32_t* __restrict__ nosplit, FlowCsr G,
                                                     const double* __restrict__ deg, const uint8_t* __restrict__ bin,
                                                     double* __restrict__ part) {
  sweep_body(ftasks, nosplit, FlowGraph{G}, deg, bin, part);
}

// per record i: the 10 costs, first strictly smaller wins, split iff mcut < T (res_*: what the host reads back; res_costs[i][10]:
// the costs themselves, written only when non-null -- the test-only per-segment dump, Flow::dump_seg; the shipped driver passes null)
__global__ __launch_bounds__(AI_BLOCK) void fk_sweep_final(const SegRec* __restrict__ recs,
                                                           const int32_t* __restrict__ nosplit, const double* __restrict__ part, double T,
                                                           int32_t* __restrict__ kstar,
                                                           int32_t* __restrict__ res_split, int32_t* __restrict__ res_ntrue,
                                                           double* __restrict__ res_mcut, double* __restrict__ res_costs) {
  const int i = blockIdx.x;
  const int s = i;  // the record's index is its slot in the per-segment tables
  const SegRec sr = recs[i];
  if (nosplit[s]) {
    if (threadIdx.x == 0) {
      kstar[s] = 0;
      res_split[i] = 0;
      res_ntrue[i] = 0;
      res_mcut[i] = INFINITY;
      if (res_costs)
        for (int k = 0; k < AI_NUM_CUTS; ++k) res_costs[i * AI_NUM_CUTS + k] = INFINITY;
    }
    return;
  }
  sweep_final_body(part, sr.foff, sr.foff + FK_NF(sr), T, s, res_costs, kstar, res_split, res_ntrue, res_mcut);
}

// ----------------------------------------------------------------------------- harvest: partition + rebuild, in place
// What the partition kernels need per segment slot
struct __attribute__((aligned(16))) SplitSeg {
  int32_t g0, n;        // position range of the parent
  int32_t ntrue;        // rows on the mask side (binary split)
  int32_t contA, contB; // the mask-side / other-side child continues (its graph is rebuilt)
  int32_t multi;        // split into connected components instead
  int32_t kstar;        // winning threshold of a binary split
  int32_t pad1;
};

// flag[row] = 1 on the mask side of a binary split (0 everywhere in a component split)
__global__ __launch_bounds__(AI_BLOCK) void fk_split_flags(const Task* __restrict__ ctasks, const SplitSeg* __restrict__ ss,
                                                           const uint8_t* __restrict__ bin, int32_t* __restrict__ flag) {
  const Task tk = ctasks[blockIdx.x];
  const int multi = ss[tk.z].multi, ks = ss[tk.z].kstar;
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) flag[row] = (!multi && (int)bin[row] > ks) ? 1 : 0;
}

// Stable partition of a parent's rows (mask side first, normalized_cut.py:57-59): new position of every row, the
// original ids at their new positions (final ordering and the children's buffer), zeroed entry counts.
// fscan = exclusive scan of flag over a range containing the parent.
__global__ __launch_bounds__(AI_BLOCK) void fk_partition(const Task* __restrict__ ctasks, const SplitSeg* __restrict__ ss,
                                                         const int32_t* __restrict__ flag, const int32_t* __restrict__ fscan, FlowCsr G,
                                                         int32_t* __restrict__ final_order, int32_t* __restrict__ map,
                                                         int32_t* __restrict__ newcnt, const double* __restrict__ ev2, double* __restrict__ warm) {
  const Task tk = ctasks[blockIdx.x];
  const SplitSeg sg = ss[tk.z];
  if (sg.multi) return;
  const int32_t* __restrict__ orig = G.orig[FK_PAR(tk)];
  int32_t* __restrict__ orig_next = G.orig[FK_PAR(tk) ^ 1];
  const int f0 = fscan[sg.g0];
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    const int f = flag[row];
    const int rt = fscan[row] - f0;
    const int rf = (row - sg.g0) - rt;
    const int np = sg.g0 + (f ? rt : sg.ntrue + rf);
    const int32_t id = orig[row];
    final_order[np] = id;
    orig_next[np] = id;
    if (warm) warm[np] = ev2[row];   // the parent's second Ritz vector at the row's new position (the children's warm start)
    map[row] = (f ? sg.contA : sg.contB) ? np : -1;
    newcnt[np] = 0;
  }
}

// rcnt[root] = rows of the component (rcnt zeroed over the parents' ranges by the caller)
__global__ __launch_bounds__(AI_BLOCK) void fk_rootcount(const Task* __restrict__ tasks, const int32_t* __restrict__ parent,
                                                         int32_t* __restrict__ rcnt) {
  const Task tk = tasks[blockIdx.x];
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
      const unsigned long long later = (lane == 63) ? 0ull : (heads >> (lane + 1));
      const int nlive = __popcll(lives);
      const int len = later ? (__ffsll((long long)later)) : (nlive - lane);
      atomicAdd(&rcnt[r], len);
    }
  }
}

// rc[row] = 1 for component roots; key[row] = root of the row (the sort key); rows outside the wave's
// disconnected segments keep rc = 0 (zeroed by the caller) and key = their own position (fk_iota)
__global__ __launch_bounds__(AI_BLOCK) void fk_rootflag(const Task* __restrict__ ctasks, const int32_t* __restrict__ parent,
                                                        int32_t* __restrict__ rc, int32_t* __restrict__ key) {
  const Task tk = ctasks[blockIdx.x];
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK) {
    const int32_t p = parent[row];
    rc[row] = (p == row) ? 1 : 0;
    key[row] = p;
  }
}
__global__ __launch_bounds__(AI_BLOCK) void fk_iota2(int32_t* __restrict__ a, int32_t* __restrict__ b, int32_t* __restrict__ z0,
                                                     int32_t* __restrict__ z1, int32_t lo, int32_t hi) {
  const int i = lo + blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < hi) {
    a[i] = i;
    b[i] = i;
    z0[i] = 0;  // (the root counts and flags of the range start from zero: two memset launches less per wave)
    z1[i] = 0;
  }
}

// component table in position order: (root, rows); `ord` = exclusive scan of rc over the range [base, ...)
__global__ __launch_bounds__(AI_BLOCK) void fk_comp_table(const Task* __restrict__ ctasks, const int32_t* __restrict__ parent,
                                                          const int32_t* __restrict__ ord, const int32_t* __restrict__ rcnt,
                                                          int32_t* __restrict__ troot, int32_t* __restrict__ tsize) {
  const Task tk = ctasks[blockIdx.x];
  for (int row = tk.x + threadIdx.x; row < tk.y; row += AI_BLOCK)
    if (parent[row] == row) {
      const int o = ord[row];
      troot[o] = row;
      tsize[o] = rcnt[row];
    }
}

// p = a position of a disconnected parent after the stable sort of its rows by root: the row sorted_rows[p] moves
// to p; ccont[o] = component o continues
__global__ __launch_bounds__(AI_BLOCK) void fk_partition_multi(const Task* __restrict__ ctasks, const SplitSeg* __restrict__ ss,
                                                               const int32_t* __restrict__ sorted_rows, const int32_t* __restrict__ parent,
                                                               const int32_t* __restrict__ ord, const int32_t* __restrict__ ccont, FlowCsr G,
                                                               int32_t* __restrict__ final_order, int32_t* __restrict__ map,
                                                               int32_t* __restrict__ newcnt, const double* __restrict__ ev2, double* __restrict__ warm) {
  const Task tk = ctasks[blockIdx.x];
  if (!ss[tk.z].multi) return;
  const int32_t* __restrict__ orig = G.orig[FK_PAR(tk)];
  int32_t* __restrict__ orig_next = G.orig[FK_PAR(tk) ^ 1];
  for (int p = tk.x + threadIdx.x; p < tk.y; p += AI_BLOCK) {
    const int row = sorted_rows[p];
    const int o = ord[parent[row]];
    const int32_t id = orig[row];
    final_order[p] = id;
    orig_next[p] = id;
    if (warm) warm[p] = ev2[row];   // (ev2 holds a copy of the segment's inherited warm vector: fk_copy_rows)
    map[row] = ccont[o] ? p : -1;
    newcnt[p] = 0;
  }
}

// kept entries of a surviving row (both ends on the same side); fine tasks of the parents, 16 lanes per row
__global__ __launch_bounds__(AI_BLOCK) void fk_rebuild_count(const Task* __restrict__ ftasks, FlowCsr G, const int32_t* __restrict__ flag,
                                                             const int32_t* __restrict__ map, int32_t* __restrict__ newcnt) {
  const Task tk = ftasks[blockIdx.x];
  const int2* __restrict__ rowse = G.rowse[FK_PAR(tk)];
  const int32_t* __restrict__ col = G.col[FK_PAR(tk)];
  const int l = threadIdx.x & (AI_LPR - 1), r = threadIdx.x / AI_LPR;
  for (int row = tk.x + r; row < tk.y; row += AI_BLOCK / AI_LPR) {
    const int32_t dst = map[row];
    int c = 0;
    if (dst >= 0) {
      const int f = flag[row];
      const int2 se = rowse[row];
      for (int p = se.x + l; p < se.y; p += AI_LPR) c += (flag[col[p]] == f) ? 1 : 0;
    }
    c += __shfl_xor(c, 8, 16);
    c += __shfl_xor(c, 4, 16);
    c += __shfl_xor(c, 2, 16);
    c += __shfl_xor(c, 1, 16);
    if (l == 0 && dst >= 0) newcnt[dst] = c;
  }
}

// row records of the children: entries packed from the parent's first entry offset on, in position order
// (nscan = exclusive scan of newcnt over a range containing the parent); coarse tasks of the parents
__global__ __launch_bounds__(AI_BLOCK) void fk_child_rows(const Task* __restrict__ ctasks, const SplitSeg* __restrict__ ss, FlowCsr G,
                                                          const int32_t* __restrict__ newcnt, const int32_t* __restrict__ nscan) {
  const Task tk = ctasks[blockIdx.x];
  const SplitSeg sg = ss[tk.z];
  const int e0 = G.rowse[FK_PAR(tk)][sg.g0].x - nscan[sg.g0];
  int2* __restrict__ next = G.rowse[FK_PAR(tk) ^ 1];
  for (int p = tk.x + threadIdx.x; p < tk.y; p += AI_BLOCK) {
    const int b = e0 + nscan[p];
    next[p] = make_int2(b, b + newcnt[p]);
  }
}

__global__ __launch_bounds__(AI_BLOCK) void fk_rebuild_fill(const Task* __restrict__ ftasks, FlowCsr G, const int32_t* __restrict__ flag,
                                                            const int32_t* __restrict__ map) {
  const Task tk = ftasks[blockIdx.x];
  const int par = FK_PAR(tk);
  const int2* __restrict__ rowse = G.rowse[par];
  const int32_t* __restrict__ col = G.col[par];
  const double* __restrict__ wraw = G.w[par];
  const int2* __restrict__ rowse_next = G.rowse[par ^ 1];
  int32_t* __restrict__ new_col = G.col[par ^ 1];
  double* __restrict__ new_w = G.w[par ^ 1];
  const int l = threadIdx.x & (AI_LPR - 1), r = threadIdx.x / AI_LPR;
  const int grp = (threadIdx.x & 63) / AI_LPR;
  // every wave runs the same number of row passes and, per pass, of rounds: __ballot sees whole waves
  for (int base = tk.x; base < tk.y; base += AI_BLOCK / AI_LPR) {
    const int row = base + r;
    const bool live = row < tk.y;
    const int32_t dst = live ? map[row] : -1;
    const int f = (dst >= 0) ? flag[row] : -1;
    const int2 se = (dst >= 0) ? rowse[row] : make_int2(0, 0);
    const int p0 = se.x, p1 = se.y;
    int out = (dst >= 0) ? rowse_next[dst].x : 0;
    int rounds = (p1 - p0 + AI_LPR - 1) / AI_LPR;
    for (int o = 32; o >= AI_LPR; o >>= 1) rounds = max(rounds, __shfl_xor(rounds, o, 64));
    for (int it = 0; it < rounds; ++it) {
      const int p = p0 + it * AI_LPR + l;
      int c = -1;
      bool keep = false;
      double w = 0.0;
      if (p < p1) {
        c = col[p];
        w = wraw[p];
        keep = (flag[c] == f);
      }
      const unsigned long long bal = __ballot(keep);
      const unsigned int gbits = (unsigned int)((bal >> (grp * AI_LPR)) & 0xffffull);
      const int before = __popc(gbits & ((1u << l) - 1u));
      if (keep) {
        new_col[out + before] = map[c];
        new_w[out + before] = w;
      }
      out += __popc(gbits);
    }
  }
}

// bin_i = number of thresholds strictly below ev_i (k_bin with per-slot tables)
__global__ __launch_bounds__(AI_BLOCK) void fk_bin(const Task* __restrict__ ctasks, const int32_t* __restrict__ nosplit,
                                                   const double* __restrict__ scale, const double* __restrict__ thr,
                                                   const double* __restrict__ ev, uint8_t* __restrict__ bin) {
  bin_body(ctasks, nosplit, scale, thr, ev, bin);
}
