// Host side of one level of the level-synchronous recursion: task lists, packed uploads, degrees / components / scaling,
// lock-step Lanczos, Lanczos with full re-orthogonalisation, threshold sweep (class Solver).  Included by ai_solver.hip
// inside its anonymous namespace, after ai_ncut_kernels.inc.
// ----------------------------------------------------------------------------- host: driver
struct SegHost {
  int start, n, gstart;
  int mode;     // 0 Lanczos, 1 null vector
  int need_cc;  // 0: component labels were carried over a cut between whole components
  int chunk;    // which chunk of a batched call the segment belongs to
};

template <typename T>
struct Ptr {  // a device pointer into a larger blob (same `.p` spelling as DevBuf)
  T* p = nullptr;
};

struct TaskList {
  int rows_per_task = 0;
  int n = 0;
  std::vector<Task> h;
  std::vector<int32_t> h_seg0;
  Ptr<Task> d;
  Ptr<int32_t> d_seg0;
};

// Several small host arrays -> the context's pinned staging buffer -> ONE async copy into one
// device blob; the device pointers are handed out after the copy is queued.
struct Pack {
  char* stage;
  size_t cap, off = 0;
  struct Item {
    void** dst;
    size_t off;
  };
  std::vector<Item> items;
  bool overflow = false;
  Pack(char* stage_, size_t cap_) : stage(stage_), cap(cap_) {}
  template <typename T>
  void add(T** dst, const T* src, size_t count) {
    off = (off + 63) & ~(size_t)63;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    if (off + bytes > cap) {
      overflow = true;
      return;
    }
    if (count) memcpy(stage + off, src, count * sizeof(T));
    items.push_back(Item{(void**)dst, off});
    off += bytes;
  }
  int flush(DevBuf<char>& blob, hipStream_t st) {
    if (overflow) {
      ai_set_error("per-level task tables exceed the %zu-byte staging buffer (too many segments for this build)", cap);
      return AI_ERR_INTERNAL;
    }
    AI_TRY(blob.ensure(off + 64));
    AI_HIP(hipMemcpyAsync(blob.p, stage, off, hipMemcpyHostToDevice, st));
    for (auto& it : items) *it.dst = blob.p + it.off;
    return AI_OK;
  }
};

class Solver {
 public:
  Solver(ai_ctx* c, const ai_csr* a) : ctx(c), A(a), st(c->stream) {}

  ai_ctx* ctx;
  const ai_csr* A;
  hipStream_t st;
  ai_ncut_opts opt{1e-10, 4000, 16, 0, 0};
  bool time_spmv = false;           // opts.reserved bit 0: HIP events around every SpMV launch
  bool clock_spmv = false;          // opts.reserved bit 1: every SpMV launch stamps its own span on the device clock
  DevBuf<unsigned long long> tstamps, tblock;  // {start, end} per launch of the current level; per block of the launch in flight
  double clock_khz = 0.0;
  std::vector<hipEvent_t> evpool;   // 2 per launch of the current level
  DevBuf<unsigned long long> work;  // [rows, nnz] processed by the SpMV kernel
  ai_ncut_stats stats{};

  // active set
  int na = 0;                 // active rows
  std::vector<SegHost> segs;  // active segments (host copy)
  int S() const { return (int)segs.size(); }
  const int32_t *rowptr = nullptr, *col = nullptr, *orig = nullptr;
  const double* wraw = nullptr;
  int32_t* parent = nullptr;  // component labels of the current level
  DevBuf<int32_t> b_rowptr[2], b_col[2], b_orig[2], b_parent[2];
  DevBuf<double> b_wraw[2];
  DevBuf<int32_t> orig_id;  // identity when the graph has no permutation of its own
  int pp = 0;               // ping-pong index of the NEXT level's buffers

  // per-row work arrays
  DevBuf<double> deg, sinv, sinv2, u1, wm, ev, Y;
  DevBuf<int32_t> rcnt, rc, ex, flag, fscan, map, newcnt, scantmp, final_order;
  DevBuf<uint8_t> side, bin;
  // tasks
  TaskList fine, coarse;  // every active row
  TaskList lzf, lzc;      // rows of the Lanczos-mode segments only (grids of the step kernels)
  std::vector<TaskRange> h_cranges, h_segrange;
  Ptr<TaskRange> cranges, segrange;
  DevBuf<char> blobA, blobB, blobC, blobD, resblob, lzres;
  DevBuf<int32_t> t_root, t_size;  // component table of the disconnected segments
  DevBuf<uint8_t> sorttmp;
  size_t rescap = 0;
  std::vector<int32_t> h_seg_start;
  Ptr<int32_t> seg_start, factive, cactive;
  DevBuf<double> pvol, pA, pvolA, pvolB, psweep;
  DevBuf<double2> pB[2];
  DevBuf<MinMaxPart> pmm;
  // per-segment device arrays
  Ptr<int32_t> s_mode, s_needcc, s_gstart, s_childA, s_childB, s_multi, c_pos, c_base;  // uploaded per level (blobs)
  Ptr<int32_t> s_split, s_ntrue, s_frozen, s_m;                  // downloaded per level (resblob / lzres)
  Ptr<double> s_mcut, s_resid, s_theta;
  DevBuf<int32_t> s_ncomp, s_nosplit, s_kstar, slots;
  DevBuf<double> s_vol, s_volA, s_volB, s_scale, s_thr, s_costs, s_cu;
  // Lanczos history + vectors
  DevBuf<double> alpha_hist, b_hist, g_hist, coef, bnew_buf;
  // staged-gather encoding of the Lanczos tasks (k_lz_encode), rebuilt per level
  DevBuf<uint16_t> lidx;
  DevBuf<int32_t> ucol, enc_ctr;
  DevBuf<TaskEnc> enc;
  int32_t ucol_cap = 0;
  bool enc_ready = false;
  int mcap = 0;
  std::vector<double*> slabs, owned_slabs;
  size_t slab_stride = 0;
  ~Solver() {
    for (double* p : owned_slabs) (void)hipFree(p);
    for (hipEvent_t e : evpool) (void)hipEventDestroy(e);
  }

  LzSeg lzseg() {
    LzSeg L;
    L.frozen = s_frozen.p;
    L.m = s_m.p;
    L.alpha_hist = alpha_hist.p;
    L.b_hist = b_hist.p;
    L.g_hist = g_hist.p;
    L.factive = factive.p;
    L.cactive = cactive.p;
    L.mcap = mcap;
    return L;
  }

  int alloc_rows() {
    const size_t n = (size_t)A->n, e = (size_t)A->nnz;
    AI_TRY(deg.alloc(n));
    AI_TRY(sinv.alloc(n));
    AI_TRY(sinv2.alloc(n));
    AI_TRY(u1.alloc(n));
    AI_TRY(wm.alloc(e + 8));   // k_lz_spmv_q reads whole aligned quads of entries
    AI_TRY(ev.alloc(n));
    AI_TRY(Y.alloc(n));
    AI_TRY(b_parent[0].alloc(n));
    AI_TRY(b_parent[1].alloc(n));
    // children never have more rows / entries than the chunk: size the ping-pong halves once
    for (int h = 0; h < 2; ++h) {
      AI_TRY(b_rowptr[h].alloc(n + 1));
      AI_TRY(b_orig[h].alloc(n));
      AI_TRY(b_col[h].alloc(e));
      AI_TRY(b_wraw[h].alloc(e));
    }
    AI_TRY(rcnt.alloc(n));
    AI_TRY(rc.alloc(n + 1));
    AI_TRY(ex.alloc(n + 1));
    AI_TRY(flag.alloc(n + 1));
    AI_TRY(fscan.alloc(n + 1));
    AI_TRY(map.alloc(n));
    AI_TRY(newcnt.alloc(n + 1));
    AI_TRY(scantmp.alloc(ai_scan_tmp_elems((int64_t)n)));
    AI_TRY(final_order.alloc(n));
    AI_TRY(side.alloc(n));
    AI_TRY(bin.alloc(n));
    AI_TRY(slots.alloc(AI_MAX_CHECKS));
    AI_TRY(lidx.alloc(e + 8));
    ucol_cap = (int32_t)std::min<size_t>(e / 2 + 4096, (size_t)1 << 30);
    AI_TRY(ucol.alloc((size_t)ucol_cap));
    AI_TRY(enc_ctr.alloc(1));
    AI_TRY(work.alloc(2));
    AI_HIP(hipMemsetAsync(work.p, 0, 2 * sizeof(unsigned long long), st));
    return AI_OK;
  }

  int alloc_segs(int S_) {
    const size_t s = (size_t)S_ + 1;
    AI_TRY(s_ncomp.ensure(s));
    AI_TRY(s_nosplit.ensure(s));
    AI_TRY(s_kstar.ensure(s));
    AI_TRY(s_vol.ensure(s));
    AI_TRY(s_volA.ensure(s));
    AI_TRY(s_volB.ensure(s));
    AI_TRY(s_scale.ensure(s));
    AI_TRY(s_thr.ensure(s * AI_NUM_CUTS));
    AI_TRY(s_costs.ensure(s * AI_NUM_CUTS));
    AI_TRY(s_cu.ensure(s));
    if (s > rescap) {
      // results that the host reads every level sit together so that one copy fetches them
      rescap = std::max(s, (size_t)128);
      AI_TRY(resblob.alloc(rescap * 16));
      AI_TRY(lzres.alloc(rescap * 24));
    }
    s_split.p = (int32_t*)resblob.p;
    s_ntrue.p = s_split.p + rescap;
    s_mcut.p = (double*)(s_ntrue.p + rescap);
    s_m.p = (int32_t*)lzres.p;
    s_frozen.p = s_m.p + rescap;
    s_resid.p = (double*)(s_frozen.p + rescap);
    s_theta.p = s_resid.p + rescap;
    return AI_OK;
  }

  // Level 0: the whole graph is one segment, rows in the graph's own order.
  int begin(bool force_single_segment) {
    const int n = (int)A->n;
    AI_TRY(alloc_rows());
    rowptr = A->rowptr;
    col = A->col;
    wraw = A->val;
    parent = b_parent[0].p;
    if (A->orig) {
      orig = A->orig;
    } else {
      AI_TRY(orig_id.alloc(n));
      hipLaunchKernelGGL(k_iota, dim3((n + AI_BLOCK - 1) / AI_BLOCK), dim3(AI_BLOCK), 0, st, orig_id.p, n);
      AI_KERNEL_CHECK();
      orig = orig_id.p;
    }
    AI_HIP(hipMemcpyAsync(final_order.p, orig, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    na = n;
    segs.clear();
    if (force_single_segment) segs.push_back(SegHost{0, n, 0, 0, 1, 0});
    return AI_OK;
  }

  void make_tasks(TaskList& tl, int rows_per_task, bool lanczos_only = false) {
    const int S_ = S();
    tl.rows_per_task = rows_per_task;
    tl.h.clear();
    tl.h_seg0.assign(S_ + 1, 0);
    for (int s = 0; s < S_; ++s) {
      tl.h_seg0[s] = (int32_t)tl.h.size();
      if (lanczos_only && segs[s].mode != 0) continue;
      bool first = true;
      for (int lo = segs[s].start; lo < segs[s].start + segs[s].n; lo += rows_per_task) {
        Task t;
        t.x = lo;
        t.y = std::min(lo + rows_per_task, segs[s].start + segs[s].n);
        t.z = s;
        t.w = first ? 1 : 0;
        // Lanczos lists, bits 1..: coarse tasks carry the segment's step cap (its Krylov dimension / the
        // step limit), fine tasks their index among ALL fine tasks
        if (lanczos_only) {
          if (rows_per_task == AI_FINE_ROWS)
            t.w |= (fine.h_seg0[s] + (lo - segs[s].start) / AI_FINE_ROWS) << 1;
          else
            t.w |= std::max(1, std::min(opt.max_iter, segs[s].n - 1)) << 1;
        }
        first = false;
        tl.h.push_back(t);
      }
    }
    tl.h_seg0[S_] = (int32_t)tl.h.size();
    tl.n = (int)tl.h.size();
  }

  // task lists + segment offsets for the current `segs`
  int build_tasks() {
    const int S_ = S();
    make_tasks(fine, AI_FINE_ROWS);
    make_tasks(coarse, AI_COARSE_ROWS);
    h_seg_start.assign(S_ + 1, 0);
    std::vector<int32_t> h_gstart(S_ + 1, 0), h_needcc(S_ + 1, 0);
    for (int s = 0; s < S_; ++s) {
      h_seg_start[s] = segs[s].start;
      h_gstart[s] = segs[s].gstart;
      h_needcc[s] = segs[s].need_cc;
    }
    h_seg_start[S_] = S_ ? segs[S_ - 1].start + segs[S_ - 1].n : 0;
    AI_TRY(alloc_segs(S_));
    AI_TRY(pvol.ensure(fine.n + 1));
    AI_TRY(psweep.ensure((size_t)(fine.n + 1) * AI_SWEEP_VALS));
    AI_TRY(pvolA.ensure(coarse.n + 1));
    AI_TRY(pvolB.ensure(coarse.n + 1));
    AI_TRY(pmm.ensure(coarse.n + 1));
    Pack pk(ctx->stage, AI_STAGE_BYTES / 4);
    pk.add(&fine.d.p, fine.h.data(), (size_t)fine.n);
    pk.add(&coarse.d.p, coarse.h.data(), (size_t)coarse.n);
    pk.add(&fine.d_seg0.p, fine.h_seg0.data(), (size_t)S_ + 1);
    pk.add(&coarse.d_seg0.p, coarse.h_seg0.data(), (size_t)S_ + 1);
    pk.add(&seg_start.p, h_seg_start.data(), (size_t)S_ + 1);
    pk.add(&s_gstart.p, h_gstart.data(), (size_t)S_ + 1);
    pk.add(&s_needcc.p, h_needcc.data(), (size_t)S_ + 1);
    AI_TRY(pk.flush(blobA, st));
    return AI_OK;
  }

  // degrees, scaled matrix, u1, connected components -> segs[s].mode
  int prepare(bool want_cc) {
    const int S_ = S();
    hipLaunchKernelGGL(k_degree, dim3(fine.n), dim3(AI_BLOCK), 0, st, fine.d.p, rowptr, wraw, deg.p, sinv.p, pvol.p);
    AI_KERNEL_CHECK();
    hipLaunchKernelGGL(k_seg_sum, dim3(S_), dim3(AI_BLOCK), 0, st, fine.d_seg0.p, pvol.p, s_vol.p);
    AI_KERNEL_CHECK();
    std::vector<int32_t> ncomp(S_, 1);
    if (want_cc) {
      bool any = false;
      for (auto& s : segs) any |= (s.need_cc != 0);
      if (any) {
        hipLaunchKernelGGL(k_cc_init, dim3(fine.n), dim3(AI_BLOCK), 0, st, fine.d.p, s_needcc.p, rowptr, col, parent);
        AI_KERNEL_CHECK();
        hipLaunchKernelGGL(k_cc_hook, dim3(fine.n), dim3(AI_BLOCK), 0, st, fine.d.p, s_needcc.p, rowptr, col, parent);
        AI_KERNEL_CHECK();
        hipLaunchKernelGGL(k_cc_compress, dim3(coarse.n), dim3(AI_BLOCK), 0, st, coarse.d.p, s_needcc.p, parent);
        AI_KERNEL_CHECK();
      }
      AI_HIP(hipMemsetAsync(s_ncomp.p, 0, (size_t)S_ * sizeof(int32_t), st));
      hipLaunchKernelGGL(k_cc_count, dim3(coarse.n), dim3(AI_BLOCK), 0, st, coarse.d.p, parent, s_ncomp.p);
      AI_KERNEL_CHECK();
      int32_t* dl = (int32_t*)(ctx->stage + AI_STAGE_BYTES / 2);
      AI_HIP(hipMemcpyAsync(dl, s_ncomp.p, (size_t)S_ * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      AI_HIP(hipStreamSynchronize(st));
      for (int s = 0; s < S_; ++s) ncomp[s] = dl[s];
    }
    std::vector<int32_t> mode(S_ + 1, 0);
    for (int s = 0; s < S_; ++s) {
      segs[s].mode = (ncomp[s] > 1) ? 1 : 0;
      mode[s] = segs[s].mode;
    }
    // step kernels run on the Lanczos-mode segments only: their own (compact) task lists, so that
    // a frontier with few connected segments launches few blocks and the XCD remap still spreads
    // them over the whole chip
    make_tasks(lzf, AI_FINE_ROWS, true);
    make_tasks(lzc, AI_COARSE_ROWS, true);
    h_segrange.assign(S_ + 1, TaskRange{0, 0, 0, 0});
    for (int s = 0; s < S_; ++s) h_segrange[s] = TaskRange{lzf.h_seg0[s], lzf.h_seg0[s + 1], lzc.h_seg0[s], lzc.h_seg0[s + 1]};
    h_cranges.resize(lzc.n);
    for (int t = 0; t < lzc.n; ++t) h_cranges[t] = h_segrange[lzc.h[t].z];
    std::vector<int32_t> ones((size_t)std::max(lzf.n, lzc.n) + 1, 1);
    AI_TRY(pA.ensure(lzf.n + 1));
    AI_TRY(pB[0].ensure(lzc.n + 1));
    AI_TRY(pB[1].ensure(lzc.n + 1));
    Pack pk(ctx->stage + AI_STAGE_BYTES / 4, AI_STAGE_BYTES / 4 - 16384);  // the tail holds the slab table
    pk.add(&s_mode.p, mode.data(), (size_t)S_ + 1);
    pk.add(&segrange.p, h_segrange.data(), (size_t)S_ + 1);
    pk.add(&lzf.d.p, lzf.h.data(), (size_t)lzf.n);
    pk.add(&lzc.d.p, lzc.h.data(), (size_t)lzc.n);
    pk.add(&cranges.p, h_cranges.data(), (size_t)lzc.n);
    pk.add(&factive.p, ones.data(), (size_t)lzf.n);
    pk.add(&cactive.p, ones.data(), (size_t)lzc.n);
    AI_TRY(pk.flush(blobB, st));
    // scaled matrix, 1 / deg and u1 are only read by the Lanczos kernels: rows of null-vector segments skip them
    if (lzf.n > 0) {
      hipLaunchKernelGGL(k_scale, dim3(lzf.n), dim3(AI_BLOCK), 0, st, (const Task*)lzf.d.p, rowptr, col, wraw, deg.p, sinv.p, s_vol.p, wm.p,
                         sinv2.p, u1.p);
      AI_KERNEL_CHECK();
    }
    enc_ready = false;
    if (lzf.n > 0) {
      AI_TRY(enc.ensure((size_t)lzf.n));
      AI_HIP(hipMemsetAsync(enc_ctr.p, 0, sizeof(int32_t), st));
      hipLaunchKernelGGL(k_lz_encode, dim3(lzf.n), dim3(AI_BLOCK), 0, st, (const Task*)lzf.d.p, rowptr, col, ucol_cap, enc_ctr.p, ucol.p, lidx.p,
                         enc.p);
      AI_KERNEL_CHECK();
      enc_ready = true;
    }
    return AI_OK;
  }

  int null_vectors() {
    const int S_ = S();
    bool any = false;
    for (auto& s : segs) any |= (s.mode == 1);
    if (!any) return AI_OK;
    const unsigned gr = (unsigned)((na + AI_BLOCK - 1) / AI_BLOCK);
    AI_HIP(hipMemsetAsync(rcnt.p, 0, (size_t)na * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_null_rootcount, dim3(coarse.n), dim3(AI_BLOCK), 0, st, coarse.d.p, s_mode.p, (const int32_t*)parent, rcnt.p);
    AI_KERNEL_CHECK();
    hipLaunchKernelGGL(k_null_rootvals, dim3(gr), dim3(AI_BLOCK), 0, st, (const int32_t*)parent, rcnt.p, na, rc.p);
    AI_KERNEL_CHECK();
    AI_TRY(ai_exclusive_scan_i32(st, rc.p, ex.p, na, scantmp.p));
    hipLaunchKernelGGL(k_null_side, dim3(coarse.n), dim3(AI_BLOCK), 0, st, coarse.d.p, s_mode.p, seg_start.p, (const int32_t*)parent, rcnt.p,
                       ex.p, deg.p, side.p, pvolA.p, pvolB.p);
    AI_KERNEL_CHECK();
    hipLaunchKernelGGL(k_seg_sum, dim3(S_), dim3(AI_BLOCK), 0, st, coarse.d_seg0.p, pvolA.p, s_volA.p);
    AI_KERNEL_CHECK();
    hipLaunchKernelGGL(k_seg_sum, dim3(S_), dim3(AI_BLOCK), 0, st, coarse.d_seg0.p, pvolB.p, s_volB.p);
    AI_KERNEL_CHECK();
    hipLaunchKernelGGL(k_null_vec, dim3(coarse.n), dim3(AI_BLOCK), 0, st, coarse.d.p, s_mode.p, s_volA.p, s_volB.p, deg.p, side.p, ev.p);
    AI_KERNEL_CHECK();
    for (auto& s : segs) stats.null_solves += (s.mode == 1);
    return AI_OK;
  }

  double* vec(int j) { return slabs[(size_t)j / AI_SLAB_VECS] + (size_t)(j % AI_SLAB_VECS) * slab_stride; }
  int ensure_vec(int j) {
    while ((size_t)j / AI_SLAB_VECS >= slabs.size()) {
      const size_t bytes = (size_t)AI_SLAB_VECS * slab_stride * sizeof(double);
      double* p = nullptr;
      if (ai_arena* a = ai_current_arena()) {
        p = (double*)a->alloc(bytes);
      } else if (hipMalloc((void**)&p, bytes) == hipSuccess) {
        owned_slabs.push_back(p);
      } else {
        p = nullptr;
      }
      if (!p) {
        ai_set_error("Lanczos vector slab %zu (%zu bytes) could not be allocated", slabs.size(), bytes);
        return AI_ERR_OOM;
      }
      slabs.push_back(p);
    }
    return AI_OK;
  }

  // e0 / e1 (optional): HIP events that receive this dispatch's own start / stop timestamps
  int spmv_variant = -1;
  template <int LPR, int ILP>
  int launch_spmv_t(int j, hipEvent_t e0, hipEvent_t e1) {
    static_assert((AI_BLOCK / LPR) * ILP == AI_FINE_ROWS, "a block covers exactly one fine task");
    if (e0) {
      hipExtLaunchKernelGGL((k_lz_spmv_t<LPR, ILP>), dim3(lzf.n), dim3(AI_BLOCK), 0, st, e0, e1, 0, (const Task*)lzf.d.p, (const int32_t*)factive.p,
                            lzf.n, rowptr, col, (const double*)wm.p, (const double*)sinv2.p, (const double*)vec(j), Y.p, pA.p);
    } else {
      hipLaunchKernelGGL((k_lz_spmv_t<LPR, ILP>), dim3(lzf.n), dim3(AI_BLOCK), 0, st, (const Task*)lzf.d.p, (const int32_t*)factive.p, lzf.n,
                         rowptr, col, (const double*)wm.p, (const double*)sinv2.p, (const double*)vec(j), Y.p, pA.p);
    }
    AI_KERNEL_CHECK();
    return AI_OK;
  }
  int launch_spmv(int j, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr) {
    if (spmv_variant < 0) {
      const char* v = getenv("AI_SPMV_VARIANT");
      spmv_variant = v ? atoi(v) : 0;
    }
    if (spmv_variant == 1) return launch_spmv_t<16, AI_ROW_ILP>(j, e0, e1);  // plain gather from global memory
    if (!enc_ready) return launch_spmv_t<16, AI_ROW_ILP>(j, e0, e1);
    unsigned long long* ts = (clock_spmv && tblock.p) ? tblock.p : (unsigned long long*)nullptr;
#define AI_SPMV_ARGS                                                                                                                 \
  (const Task*)lzf.d.p, (const int32_t*)factive.p, lzf.n, (const TaskEnc*)enc.p, (const int32_t*)ucol.p, (const uint16_t*)lidx.p, rowptr, col, \
      (const double*)wm.p, (const double*)sinv2.p, (const double*)vec(j), Y.p, pA.p
    if (e0)
      hipExtLaunchKernelGGL((k_lz_spmv_q<AI_ROW_ILP>), dim3(lzf.n), dim3(AI_BLOCK), 0, st, e0, e1, 0, AI_SPMV_ARGS, (unsigned long long*)nullptr);
    else
      hipLaunchKernelGGL((k_lz_spmv_q<AI_ROW_ILP>), dim3(lzf.n), dim3(AI_BLOCK), 0, st, AI_SPMV_ARGS, ts);
#undef AI_SPMV_ARGS
    AI_KERNEL_CHECK();
    return AI_OK;
  }

  // Lock-step Lanczos over every mode-0 segment, then Ritz vectors into ev.
  // theta_out / iters_out / resid_out (optional): values of segment 0.
  int lanczos(double* theta_out, int* iters_out, double* resid_out) {
    const int S_ = S();
    int nl = 0, max_n = 0, min_n = 1 << 30;
    std::set<int> forced;  // steps at which some segment reaches its own dimension
    for (auto& s : segs)
      if (s.mode == 0) {
        ++nl;
        max_n = std::max(max_n, s.n);
        min_n = std::min(min_n, s.n);
        forced.insert(std::min(opt.max_iter, s.n - 1));
      }
    if (nl == 0) return AI_OK;
    if (spmv_variant < 0) spmv_variant = getenv("AI_SPMV_VARIANT") ? atoi(getenv("AI_SPMV_VARIANT")) : 0;
    stats.lanczos_solves += nl;
    mcap = std::max(1, std::min(opt.max_iter, max_n - 1));
    {
      // sized once for the usual frontier (children are > 1 % of the chunk, so <= ~100 segments)
      const size_t scap = (size_t)std::max(S_, 128), mc = (size_t)std::max(mcap, opt.max_iter);
      AI_TRY(alpha_hist.ensure(scap * mc));
      AI_TRY(b_hist.ensure(scap * (mc + 1)));
      AI_TRY(g_hist.ensure(scap * (mc + 1)));
      AI_TRY(coef.ensure(scap * mc));
      AI_TRY(bnew_buf.ensure((size_t)AI_CHECK_DEPTH * (scap + 1)));
    }
    // vectors live in slabs whose stride is the row count of the first level that needs them
    // (levels only shrink)
    if (slab_stride == 0) slab_stride = (size_t)na;
    AI_HIP(hipMemsetAsync(lzres.p, 0, rescap * 24, st));  // m, frozen, resid, theta
    AI_HIP(hipMemsetAsync(slots.p, 0, AI_MAX_CHECKS * sizeof(int32_t), st));
    LzSeg L = lzseg();
    AI_TRY(ensure_vec(0));
    AI_TRY(ensure_vec(1));
    AI_HIP(hipEventRecord(ctx->ev[0], st));
    hipLaunchKernelGGL(k_lz_init, dim3(lzc.n), dim3(AI_BLOCK), 0, st, lzc.d.p, cactive.p, orig, u1.p, vec(0), pB[0].p);
    AI_KERNEL_CHECK();
    if (clock_spmv) {
      // slot j: {earliest block start, latest block end} of launch j on the device's wall clock
      AI_TRY(tstamps.ensure((size_t)2 * (mcap + 1)));
      AI_TRY(tblock.ensure((size_t)2 * (lzf.n + 1)));
      if (clock_khz == 0.0) {
        int khz = 0;
        AI_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
        clock_khz = khz > 0 ? (double)khz : 100000.0;
      }
    }
    const bool dense_checks = (min_n <= 512);
    int next_check = dense_checks ? 1 : opt.check_every;
    int steps = 0, nchecks = 0, last_check_m = 0;
    // Checks are asynchronous: the check kernel's counter is copied to pinned host memory behind
    // an event and read a few steps later, so the stream never drains.  A finished segment's
    // blocks exit at their activity flag, so steps launched past the end cost next to nothing;
    // the host still never runs more than AI_RUNAHEAD steps past an unread check.
    constexpr int AI_RUNAHEAD = 10;  // swept in round 1 (3 .. 20): throughput flat, one chunk alone gains a little up to ~10
    struct Pending { int slot, m, ev; };
    std::vector<Pending> pending;  // FIFO of in-flight checks
    size_t phead = 0;
    bool done = false;
    auto reap = [&](bool block) -> int {
      while (phead < pending.size()) {
        const Pending pc = pending[phead];
        hipEvent_t e = ctx->chk_ev[pc.ev];
        if (block) {
          AI_HIP(hipEventSynchronize(e));
        } else {
          hipError_t q = hipEventQuery(e);
          if (q == hipErrorNotReady) break;
          AI_HIP(q);
        }
        if (ctx->pinned[pc.slot % AI_PINNED_INTS] == 0) done = true;
        ++phead;
        block = false;
      }
      return AI_OK;
    };
    for (int j = 0; j < mcap && !done; ++j) {
      AI_TRY(ensure_vec(j + 1));
      if (time_spmv) {
        while (evpool.size() < (size_t)2 * (j + 1)) {
          hipEvent_t e;
          AI_HIP(hipEventCreate(&e));
          evpool.push_back(e);
        }
        AI_TRY(launch_spmv(j, evpool[2 * j], evpool[2 * j + 1]));
      } else {
        AI_TRY(launch_spmv(j));
        if (clock_spmv && enc_ready && spmv_variant == 0) {
          hipLaunchKernelGGL(k_ts_reduce, dim3(1), dim3(AI_BLOCK), 0, st, (const unsigned long long*)tblock.p, lzf.n, tstamps.p + 2 * (size_t)j);
          AI_KERNEL_CHECK();
        }
      }
      hipLaunchKernelGGL(k_lz_update, dim3(lzc.n), dim3(AI_BLOCK), 0, st, lzc.d.p, cranges.p, L, j, (const double*)pA.p,
                         (const double2*)pB[j & 1].p, pB[(j + 1) & 1].p, u1.p, (const double*)Y.p, (const double*)vec(j),
                         (const double*)vec(j > 0 ? j - 1 : 0), vec(j + 1));
      AI_KERNEL_CHECK();
      ++steps;
      const int m = j + 1;
      const bool check = dense_checks || (m >= next_check) || (m == mcap) || forced.count(m) > 0;
      if (check && nchecks < AI_MAX_CHECKS) {
        // at most AI_CHECK_DEPTH checks in flight (their events and pinned slots are recycled)
        if (pending.size() - phead >= (size_t)AI_CHECK_DEPTH - 1) AI_TRY(reap(true));
        const int cd = nchecks % AI_CHECK_DEPTH;
        double* bn = bnew_buf.p + (size_t)cd * (S_ + 1);
        hipLaunchKernelGGL(k_lz_bnew, dim3(S_), dim3(64), 0, st, segrange.p, s_mode.p, s_frozen.p, (const double2*)pB[(j + 1) & 1].p, bn);
        AI_KERNEL_CHECK();
        AI_HIP(hipEventRecord(ctx->chk_ev1[cd], st));
        AI_HIP(hipStreamWaitEvent(ctx->side, ctx->chk_ev1[cd], 0));
        const int with_rb = (size_t)3 * m * sizeof(double) <= (size_t)64 * 1024;
        hipLaunchKernelGGL(k_lz_check, dim3(S_), dim3(AI_CHECK_THREADS), (size_t)(with_rb ? 3 : 2) * m * sizeof(double), ctx->side, seg_start.p, segrange.p,
                           s_mode.p, L, (const double*)bn, m, opt.tol, opt.max_iter, m - last_check_m, rowptr, s_theta.p, s_resid.p,
                           slots.p + nchecks, work.p, with_rb);
        AI_KERNEL_CHECK();
        AI_HIP(hipMemcpyAsync(&ctx->pinned[nchecks % AI_PINNED_INTS], slots.p + nchecks, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->side));
        AI_HIP(hipEventRecord(ctx->chk_ev[cd], ctx->side));
        pending.push_back(Pending{nchecks, m, cd});
        ++nchecks;
        last_check_m = m;
        if (m >= next_check) next_check = m + std::max(opt.check_every, (m / 8 / opt.check_every) * opt.check_every);
      }
      // read whatever has arrived; block only when the oldest unread check is AI_RUNAHEAD steps old
      const bool must = (phead < pending.size()) && (m - pending[phead].m >= AI_RUNAHEAD || m == mcap);
      AI_TRY(reap(must));
    }
    while (phead < pending.size()) AI_TRY(reap(true));
    stats.lanczos_steps += steps;
    if (getenv("AI_NCUT_DEBUG")) {
      fprintf(stderr, "[ai_ncut] level %lld: segments %d (lanczos %d, rows %d..%d), active rows %d, steps %d, checks %d\n",
              (long long)stats.levels, S_, nl, min_n, max_n, na, steps, nchecks);
    }
    if (clock_spmv && enc_ready && spmv_variant == 0) {
      std::vector<unsigned long long> hts((size_t)2 * steps);
      AI_HIP(hipMemcpyAsync(hts.data(), tstamps.p, hts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      AI_HIP(hipStreamSynchronize(st));
      for (int j = 0; j < steps; ++j)
        if (hts[2 * j + 1] > hts[2 * j]) stats.ms_spmv += (double)(hts[2 * j + 1] - hts[2 * j]) / clock_khz;
    }
    if (time_spmv) {
      AI_HIP(hipStreamSynchronize(st));
      for (int j = 0; j < steps; ++j) {
        float e = 0.f;
        AI_HIP(hipEventElapsedTime(&e, evpool[2 * j], evpool[2 * j + 1]));
        stats.ms_spmv += e;
      }
    }
    // ---- Ritz coefficients on the host (tiny), Ritz vectors on the device
    std::vector<int32_t> h_m(S_), h_frozen(S_);
    std::vector<double> h_a((size_t)S_ * mcap), h_b((size_t)S_ * (mcap + 1)), h_g((size_t)S_ * (mcap + 1)), h_coef((size_t)S_ * mcap, 0.0),
        h_cu(S_, 0.0), h_resid(S_, 0.0), h_theta(S_, 0.0);
    char* dl = ctx->stage + AI_STAGE_BYTES / 2;
    AI_HIP(hipMemcpyAsync(dl, lzres.p, rescap * 24, hipMemcpyDeviceToHost, st));
    {
      // only the columns the steps have filled
      const size_t wa = (size_t)std::min(steps, mcap) * sizeof(double), wb = (size_t)std::min(steps + 1, mcap + 1) * sizeof(double);
      AI_HIP(hipMemcpy2DAsync(h_a.data(), (size_t)mcap * sizeof(double), alpha_hist.p, (size_t)mcap * sizeof(double), wa, S_, hipMemcpyDeviceToHost, st));
      AI_HIP(hipMemcpy2DAsync(h_b.data(), (size_t)(mcap + 1) * sizeof(double), b_hist.p, (size_t)(mcap + 1) * sizeof(double), wb, S_, hipMemcpyDeviceToHost, st));
      AI_HIP(hipMemcpy2DAsync(h_g.data(), (size_t)(mcap + 1) * sizeof(double), g_hist.p, (size_t)(mcap + 1) * sizeof(double), wb, S_, hipMemcpyDeviceToHost, st));
    }
    AI_HIP(hipStreamSynchronize(st));
    for (int s = 0; s < S_; ++s) {
      h_m[s] = ((const int32_t*)dl)[s];
      h_frozen[s] = ((const int32_t*)dl)[rescap + s];
      h_resid[s] = ((const double*)(dl + rescap * 8))[s];
      h_theta[s] = ((const double*)(dl + rescap * 16))[s];
    }
    int max_m = 0;
    std::vector<double> sv;
    for (int s = 0; s < S_; ++s) {
      if (segs[s].mode != 0) continue;
      int m = h_m[s];
      if (!h_frozen[s]) {
        // the check budget ran out before this segment was frozen: use everything computed
        m = steps;
        h_m[s] = m;
        ++stats.unconverged;
      }
      if (m <= 0) {
        ai_set_error("internal: Lanczos segment %d finished with an empty tridiagonal matrix", s);
        return AI_ERR_INTERNAL;
      }
      max_m = std::max(max_m, m);
      const double* a = &h_a[(size_t)s * mcap];
      const double* b = &h_b[(size_t)s * (mcap + 1)];
      const double* g = &h_g[(size_t)s * (mcap + 1)];
      double theta = 0.0;
      ai_tridiag_top(a, b, m, (h_frozen[s] && h_m[s] == m) ? &h_theta[s] : nullptr, &theta, sv);
      double cu = 0.0;
      for (int j = 0; j < m; ++j) {
        const double c = sv[j] / b[j];  // v_j = (R_j - g_j u1) / b_j
        h_coef[(size_t)s * mcap + j] = c;
        cu -= c * g[j];
      }
      h_cu[s] = cu;
      // a residual above tol is a failure only if T is smaller than the segment's own dimension
      if (h_frozen[s] && h_resid[s] > opt.tol && m < segs[s].n - 1) ++stats.unconverged;
      stats.max_resid = std::max(stats.max_resid, h_resid[s]);
      if (s == 0) {
        if (theta_out) *theta_out = theta;
        if (iters_out) *iters_out = m;
        if (resid_out) *resid_out = h_resid[s];
      }
    }
    AI_HIP(hipMemcpyAsync(s_m.p, h_m.data(), (size_t)S_ * sizeof(int32_t), hipMemcpyHostToDevice, st));
    AI_HIP(hipMemcpy2DAsync(coef.p, (size_t)mcap * sizeof(double), h_coef.data(), (size_t)mcap * sizeof(double),
                            (size_t)std::max(max_m, 1) * sizeof(double), S_, hipMemcpyHostToDevice, st));
    AI_HIP(hipMemcpyAsync(s_cu.p, h_cu.data(), (size_t)S_ * sizeof(double), hipMemcpyHostToDevice, st));
    for (int j0 = 0; j0 < max_m; j0 += AI_SLAB_VECS) {
      hipLaunchKernelGGL(k_ritz, dim3(lzc.n), dim3(AI_BLOCK), 0, st, lzc.d.p, s_mode.p, s_m.p, coef.p, mcap, s_cu.p, u1.p,
                         (const double*)slabs[(size_t)j0 / AI_SLAB_VECS], slab_stride, j0, AI_SLAB_VECS, j0 == 0 ? 1 : 0, ev.p);
      AI_KERNEL_CHECK();
    }
    AI_HIP(hipEventRecord(ctx->ev[1], st));
    AI_HIP(hipStreamSynchronize(st));  // h_coef / h_cu are read by the copies above
    float ms = 0.f;
    AI_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    stats.ms_eigen += ms;
    return AI_OK;
  }

  // ---- k1 largest eigenpairs of the deflated M (= the k1 smallest non-zero of L) of ONE connected
  // segment: Lanczos with full re-orthogonalisation.  thetas[i] descending; Ritz vectors into
  // out (k1 x out_stride, compact row order).
  DevBuf<double*> d_slabtab;
  DevBuf<double> fro_part, fro_coef, fro_cu, coefT, cuv;
  size_t slabtab_n = 0;
  int sync_slabtab() {
    if (slabtab_n == slabs.size()) return AI_OK;
    if (slabs.size() > 500) {
      ai_set_error("internal: more than 500 Lanczos slabs");
      return AI_ERR_INTERNAL;
    }
    AI_TRY(d_slabtab.ensure(512));
    // the table only ever grows by appending, so rewriting the pinned copy while an earlier
    // upload is still in flight is harmless; no synchronisation needed
    double** pin = (double**)(ctx->stage + AI_STAGE_BYTES / 2 - 8192);
    for (size_t i = 0; i < slabs.size(); ++i) pin[i] = slabs[i];
    AI_HIP(hipMemcpyAsync(d_slabtab.p, pin, slabs.size() * sizeof(double*), hipMemcpyHostToDevice, st));
    slabtab_n = slabs.size();
    return AI_OK;
  }


  int lanczos_fro(int k1, std::vector<double>& thetas, std::vector<double>& resids, double* out, size_t out_stride, int* steps_out) {
    const int S_ = S();
    if (S_ != 1 || segs[0].mode != 0) {
      ai_set_error("internal: lanczos_fro needs one connected segment");
      return AI_ERR_INTERNAL;
    }
    const int n = segs[0].n;
    mcap = std::max(1, std::min(opt.max_iter, n - 1));
    if (k1 > mcap) k1 = mcap;
    {
      const size_t scap = 128, mc = (size_t)std::max(mcap, opt.max_iter);
      AI_TRY(alpha_hist.ensure(scap * mc));
      AI_TRY(b_hist.ensure(scap * (mc + 1)));
      AI_TRY(g_hist.ensure(scap * (mc + 1)));
      AI_TRY(bnew_buf.ensure((size_t)AI_CHECK_DEPTH * (scap + 1)));
    }
    const int pitch = mcap + 1;
    AI_TRY(fro_part.ensure((size_t)lzc.n * pitch));
    AI_TRY(fro_coef.ensure((size_t)pitch));
    AI_TRY(fro_cu.ensure(8));
    if (slab_stride == 0) slab_stride = (size_t)na;
    AI_HIP(hipMemsetAsync(lzres.p, 0, rescap * 24, st));
    LzSeg L = lzseg();
    AI_TRY(ensure_vec(0));
    AI_TRY(ensure_vec(1));
    hipLaunchKernelGGL(k_lz_init, dim3(lzc.n), dim3(AI_BLOCK), 0, st, lzc.d.p, cactive.p, orig, u1.p, vec(0), pB[0].p);
    AI_KERNEL_CHECK();
    std::vector<double> h_a, h_b, h_g;
    std::vector<std::vector<double>> svec;
    int m = 0;
    bool done = false;
    const int chk = std::max(8, opt.check_every);
    int next_check = std::max(2 * k1, chk);
    for (int j = 0; j < mcap && !done; ++j) {
      AI_TRY(ensure_vec(j + 1));
      AI_TRY(sync_slabtab());
      AI_TRY(launch_spmv(j));
      hipLaunchKernelGGL(k_lz_update, dim3(lzc.n), dim3(AI_BLOCK), 0, st, lzc.d.p, cranges.p, L, j, (const double*)pA.p,
                         (const double2*)pB[j & 1].p, pB[(j + 1) & 1].p, u1.p, (const double*)Y.p, (const double*)vec(j),
                         (const double*)vec(j > 0 ? j - 1 : 0), vec(j + 1));
      AI_KERNEL_CHECK();
      // full re-orthogonalisation of R_{j+1} against v_0 .. v_j (two passes: "twice is enough")
      for (int pass = 0; pass < 2; ++pass) {
        const int nvec = j + 1;
        hipLaunchKernelGGL(k_fro_dots, dim3(lzc.n, (nvec + FRO_CH - 1) / FRO_CH), dim3(AI_BLOCK), 0, st, lzc.d.p, (const double*)vec(j + 1),
                           (double* const*)d_slabtab.p, slab_stride, nvec, fro_part.p, pitch);
        AI_KERNEL_CHECK();
        hipLaunchKernelGGL(k_fro_coef, dim3(1), dim3(AI_BLOCK), 0, st, lzc.n, (const double*)fro_part.p, pitch, nvec, (const double*)g_hist.p,
                           (const double*)b_hist.p, (const double2*)pB[(j + 1) & 1].p, fro_coef.p, fro_cu.p);
        AI_KERNEL_CHECK();
        hipLaunchKernelGGL(k_fro_apply, dim3(lzc.n), dim3(AI_BLOCK), 0, st, lzc.d.p, vec(j + 1), (double* const*)d_slabtab.p, slab_stride, nvec,
                           (const double*)fro_coef.p, (const double*)fro_cu.p, u1.p, pB[(j + 1) & 1].p);
        AI_KERNEL_CHECK();
      }
      m = j + 1;
      if (m >= next_check || m == mcap) {
        next_check = m + chk;
        // T_m and b_m to the host; the innermost wanted pair converges last: look at it first
        double* bn = bnew_buf.p;
        hipLaunchKernelGGL(k_lz_bnew, dim3(1), dim3(64), 0, st, segrange.p, s_mode.p, s_frozen.p, (const double2*)pB[(j + 1) & 1].p, bn);
        AI_KERNEL_CHECK();
        h_a.resize(m);
        h_b.resize(m + 1);
        AI_HIP(hipMemcpyAsync(h_a.data(), alpha_hist.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
        AI_HIP(hipMemcpyAsync(h_b.data(), b_hist.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
        AI_HIP(hipMemcpyAsync(&h_b[m], bn, sizeof(double), hipMemcpyDeviceToHost, st));
        int32_t frozen = 0;
        AI_HIP(hipMemcpyAsync(&frozen, s_frozen.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        AI_HIP(hipStreamSynchronize(st));
        const int kk = std::min(k1, m);
        double glo = -1e300, ghi = -1e300;
        for (int i = 0; i < m; ++i) {
          glo = std::max(glo, h_a[i]);
          ghi = std::max(ghi, h_a[i] + (i > 0 ? fabs(h_b[i]) : 0.0) + (i + 1 < m ? fabs(h_b[i + 1]) : 0.0));
        }
        double gmin = 1e300;
        for (int i = 0; i < m; ++i) gmin = std::min(gmin, h_a[i] - (i > 0 ? fabs(h_b[i]) : 0.0) - (i + 1 < m ? fabs(h_b[i + 1]) : 0.0));
        ghi += 1e-14 * std::max(fabs(ghi), 1.0);
        gmin -= 1e-14 * std::max(fabs(gmin), 1.0);
        std::vector<double> sv;
        std::vector<std::vector<double>> none;
        std::vector<int> nocl;
        const double th_in = ai_tridiag_eigval(h_a.data(), h_b.data(), m, kk - 1, gmin, ghi);
        ai_tridiag_eigvec(h_a.data(), h_b.data(), m, th_in, none, nocl, sv);
        const double r_in = fabs(h_b[m] * sv[m - 1]);
        if (getenv("AI_NCUT_DEBUG")) fprintf(stderr, "[ai_eigs] m=%d innermost theta=%.12f resid=%.3e\n", m, th_in, r_in);
        if ((r_in <= opt.tol && kk == k1) || m == mcap || frozen) done = true;
        if (frozen) {
          // Krylov space exhausted inside the update kernel: T stops at the size recorded there
          int32_t fm = m;
          AI_HIP(hipMemcpyAsync(&fm, s_m.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
          AI_HIP(hipStreamSynchronize(st));
          m = std::max(1, std::min(m, (int)fm));
        }
      }
    }
    if (steps_out) *steps_out = m;
    // ---- all k1 Ritz pairs of T_m on the host
    h_a.resize(m);
    h_b.resize(m + 1);
    h_g.resize(m);
    AI_HIP(hipMemcpyAsync(h_a.data(), alpha_hist.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
    AI_HIP(hipMemcpyAsync(h_b.data(), b_hist.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
    AI_HIP(hipMemcpyAsync(h_g.data(), g_hist.p, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
    {
      hipLaunchKernelGGL(k_lz_bnew, dim3(1), dim3(64), 0, st, segrange.p, s_mode.p, s_frozen.p, (const double2*)pB[m & 1].p, bnew_buf.p);
      AI_KERNEL_CHECK();
      AI_HIP(hipMemcpyAsync(&h_b[m], bnew_buf.p, sizeof(double), hipMemcpyDeviceToHost, st));
    }
    AI_HIP(hipStreamSynchronize(st));
    const int kk = std::min(k1, m);
    double ghi = -1e300, gmin = 1e300, nrm = 0.0;
    for (int i = 0; i < m; ++i) {
      const double rad = (i > 0 ? fabs(h_b[i]) : 0.0) + (i + 1 < m ? fabs(h_b[i + 1]) : 0.0);
      ghi = std::max(ghi, h_a[i] + rad);
      gmin = std::min(gmin, h_a[i] - rad);
      nrm = std::max(nrm, fabs(h_a[i]) + rad);
    }
    ghi += 1e-14 * std::max(fabs(ghi), 1.0);
    gmin -= 1e-14 * std::max(fabs(gmin), 1.0);
    thetas.assign(kk, 0.0);
    resids.assign(kk, 0.0);
    svec.assign(kk, std::vector<double>());
    std::vector<double> h_coefT((size_t)m * RITZ_MAXK, 0.0), h_cuv(RITZ_MAXK, 0.0);
    for (int i = 0; i < kk; ++i) {
      thetas[i] = ai_tridiag_eigval(h_a.data(), h_b.data(), m, i, gmin, ghi);
      std::vector<int> cluster;
      for (int c = 0; c < i; ++c)
        if (fabs(thetas[c] - thetas[i]) <= 1e-3 * nrm) cluster.push_back(c);
      ai_tridiag_eigvec(h_a.data(), h_b.data(), m, thetas[i], svec, cluster, svec[i]);
      resids[i] = fabs(h_b[m] * svec[i][m - 1]);
      double cu = 0.0;
      for (int j = 0; j < m; ++j) {
        const double c = svec[i][j] / h_b[j];
        h_coefT[(size_t)j * RITZ_MAXK + i] = c;
        cu -= c * h_g[j];
      }
      h_cuv[i] = cu;
    }
    AI_TRY(coefT.ensure(h_coefT.size()));
    AI_TRY(cuv.ensure(RITZ_MAXK));
    AI_HIP(hipMemcpyAsync(coefT.p, h_coefT.data(), h_coefT.size() * sizeof(double), hipMemcpyHostToDevice, st));
    AI_HIP(hipMemcpyAsync(cuv.p, h_cuv.data(), RITZ_MAXK * sizeof(double), hipMemcpyHostToDevice, st));
    for (int j0 = 0; j0 < m; j0 += AI_SLAB_VECS) {
      hipLaunchKernelGGL(k_ritz_multi, dim3(lzc.n), dim3(AI_BLOCK), 0, st, lzc.d.p, kk, (const double*)coefT.p, (const double*)cuv.p, u1.p,
                         (const double*)slabs[(size_t)j0 / AI_SLAB_VECS], slab_stride, j0, AI_SLAB_VECS, m, j0 == 0 ? 1 : 0, out, out_stride);
      AI_KERNEL_CHECK();
    }
    AI_HIP(hipStreamSynchronize(st));
    return AI_OK;
  }

  // min/max, bins, 10 costs, decision -> host vectors (raw = 1: ev used as given)
  // skip_disconnected: segments of mode 1 have no eigenvector (they are split by components) and are left out
  int sweep(double T, int raw, bool skip_disconnected, std::vector<int32_t>& h_split, std::vector<int32_t>& h_ntrue, std::vector<double>& h_mcut) {
    const int S_ = S();
    const int32_t* md = skip_disconnected ? (const int32_t*)s_mode.p : nullptr;
    AI_HIP(hipEventRecord(ctx->ev[2], st));
    hipLaunchKernelGGL(k_minmax, dim3(coarse.n), dim3(AI_BLOCK), 0, st, coarse.d.p, md, ev.p, orig, pmm.p);
    AI_KERNEL_CHECK();
    hipLaunchKernelGGL(k_minmax_final, dim3((S_ + 63) / 64), dim3(64), 0, st, coarse.d_seg0.p, md, pmm.p, S_, raw, s_scale.p, s_nosplit.p, s_thr.p);
    AI_KERNEL_CHECK();
    hipLaunchKernelGGL(k_bin, dim3(coarse.n), dim3(AI_BLOCK), 0, st, coarse.d.p, s_nosplit.p, s_scale.p, s_thr.p, ev.p, bin.p);
    AI_KERNEL_CHECK();
    hipLaunchKernelGGL(k_sweep, dim3(fine.n), dim3(AI_BLOCK), 0, st, fine.d.p, s_nosplit.p, rowptr, col, wraw, deg.p, bin.p, psweep.p);
    AI_KERNEL_CHECK();
    hipLaunchKernelGGL(k_sweep_final, dim3(S_), dim3(AI_BLOCK), 0, st, fine.d_seg0.p, s_nosplit.p, psweep.p, T, s_costs.p, s_kstar.p, s_split.p,
                       s_ntrue.p, s_mcut.p);
    AI_KERNEL_CHECK();
    AI_HIP(hipEventRecord(ctx->ev[3], st));
    h_split.resize(S_);
    h_ntrue.resize(S_);
    h_mcut.resize(S_);
    {
      char* dl = ctx->stage + AI_STAGE_BYTES / 2;
      AI_HIP(hipMemcpyAsync(dl, resblob.p, rescap * 16, hipMemcpyDeviceToHost, st));
      AI_HIP(hipStreamSynchronize(st));
      const int32_t* sp = (const int32_t*)dl;
      const int32_t* nt = sp + rescap;
      const double* mc = (const double*)(nt + rescap);
      for (int s = 0; s < S_; ++s) {
        h_split[s] = sp[s];
        h_ntrue[s] = nt[s];
        h_mcut[s] = mc[s];
      }
    }
    float ms = 0.f;
    AI_HIP(hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]));
    stats.ms_sweep += ms;
    return AI_OK;
  }
};


void fill_opts(Solver& S, const ai_ncut_opts* opts) {
  if (!opts) return;
  if (opts->tol > 0.0) S.opt.tol = opts->tol;
  if (opts->max_iter > 0) S.opt.max_iter = std::min(opts->max_iter, 4000);  // T_m must fit the check kernel's 64 KB of LDS
  if (opts->check_every > 0) S.opt.check_every = opts->check_every;
  S.time_spmv = (opts->reserved & 1) != 0;
  S.clock_spmv = !S.time_spmv && (opts->reserved & 2) != 0;
}

// The recursion over one graph that holds `nchunks` independent chunks back to back (rows
// off[c] .. off[c+1]); every chunk starts as its own root segment and keeps its own original
// point count for the split_lim gate.  csr->orig holds chunk-LOCAL point ids.
