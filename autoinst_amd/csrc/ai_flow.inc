// Host side of the ASYNCHRONOUS FRONTIER of the recursive normalized cut (class Flow; kernels in ai_flow_kernels.inc).
//
// The lock-step driver (ncut_lockstep in ai_solver.hip, test-only build) processes one recursion depth at a time: a level lasts until
// its slowest segment has converged, and the deep levels of a chunk run alone on the device.  Here every segment
// advances on its own:
//   * the POOL holds every connected segment that is iterating; one Lanczos step = two launches (fk_spmv, fk_update)
//     over the pool's task lists on the context's main stream, each segment at its own step count j = J - t0;
//   * a convergence check of the whole pool runs on the side stream every `check_every` steps and freezes segments;
//   * frozen segments are HARVESTED by a wave on a third stream while the pool keeps stepping: Ritz vector,
//     10-threshold sweep (normalized_cut.py:13-34), stable partition + CSR rebuild of the children in place,
//     degrees / connected components / scaling / staged-gather encoding of the children, which then JOIN the pool
//     (t0 = the step at which they join).  Disconnected segments are split into all their components by the next wave.
// One wave is in flight at a time; the host never waits for the device while the pool has work.
// Groups come out in the reference's emission order (mask side first, normalized_cut.py:57-59); no float atomics,
// so labels are reproducible run to run.
// Every segment also carries the heights of the cut tree (FSeg::front / path; DESIGN.md section 21) and every group records the
// height of the boundary in front of it and the cost of the cut it was refused: ai_ncut_tree returns them, ai_ncut drops them.

// The segment and group records (FSeg, FLeaf), the allocator of stable task indices (RangeAlloc), the map of the pinned host area with
// the layouts of a wave's tables (WaveResults, HistRows, CoefTable) and the rules that turn a harvested segment into children and
// groups (child_solve_again, children_of_cut, children_of_components) are host-only and live in ai_flow_host.h, where a CPU test
// reaches them (tests/test_host_flow.py; DESIGN.md section 29).  This file holds no offset into the pinned area of its own.

struct Rider {  // a small host table that rides along with a wave's records (Flow::expand): where it is, where it goes on the device, its bytes
  const void* host = nullptr;
  void* dev = nullptr;
  size_t bytes = 0;
};

class Flow {
 public:
  static constexpr int RING = 16;      // pool list versions kept alive (a relist waits for the checks that still read the entry it rewrites: with 4 entries it waited ~40 us on average, 18 ms of a 12-chunk call)
  static constexpr int TS_CAP = 1 << 16;  // launches whose device-clock stamps are kept
  static constexpr int AHEAD = 10;        // steps the host may launch past the last step the device has reported (it reports every 2nd)
  static constexpr int AHEAD_SMALL = 8;   // ... for a small pool: short steps, children should not wait long for the host's position (4 .. 12 measured: no difference beyond the run-to-run spread)

  explicit Flow(ai_ctx* c) : ctx(c), sm(c->stream), ss(c->side) {}
  ai_ctx* ctx;
  hipStream_t sm, ss, sw = nullptr;
  ai_ncut_opts opt{1e-10, 4000, 16, 0, 0};
  bool clock_spmv = false;
  ai_ncut_stats stats{};
  // problem
  int N = 0;
  int64_t E = 0;
  int nchunks = 0;
  const int64_t* off = nullptr;
  const int64_t* n_orig = nullptr;
  double T = 0.0;
  int SMAX = 0, WCAP = 0, FCAP = 0, CCAP = 0, FLIST = 0, CLIST = 0, mcap = 0;
  int W = 0;                       // rows of the Lanczos vector slabs: the chunks in flight at one time (the admission window)
  RangeAlloc sa;                   // slab rows -> chunks in flight
  std::vector<int> chunk_sbase, chunk_live;  // slab rows of an admitted chunk (-1: not admitted / finished); its open segments
  std::deque<int> waiting;         // chunks not admitted yet
  std::vector<FSeg> new_roots;     // admitted, waiting for the next wave
  int64_t window_rows = 0;         // caller's limit (0: everything at once)
  // device
  FlowCsr G{};
  DevBuf<int2> rowse0, rowse1;
  DevBuf<int32_t> col1, orig1;
  DevBuf<double> w1;
  DevBuf<double> deg, sinv, sinv2, u1, wm, ev, Z;
  DevBuf<double> ev2, warmv;   // (warm start) the harvested segments' second Ritz vectors in their parents' row order; the same carried to the children's positions
  // A child starts its solve from the second Ritz vector of its last solved ancestor instead of the hash vector alone: 8-9 % fewer
  // row-steps in round 5's CPU study (below the 15 % it was to be built for), but the whole of it is one more accumulator in fk_ritz
  // and one array carried by the partitions, so it was built as an A/B and measured: 132 -> 142 chunks/s, one 12-chunk call alone
  // 105 -> 97 ms, the same partitions on every fixture of the GPU suite (DESIGN_EXPERIMENTS G1, G8).  AI_FLOW_WARM=0 is the hash start
  // of rounds 1-4 (a variant selector, read per call: tests/test_gpu_parity.py compares the two).
  int warm = (getenv("AI_FLOW_WARM") && atoi(getenv("AI_FLOW_WARM")) == 0) ? 0 : 1;
  // A segment WITHOUT a solved ancestor (the components a chunk falls into first: 55 % of the headline chunk's row-steps) starts from
  // u1 * (its points' coordinate along their principal axis) where the graph kept its points (fk_pca_* in ai_flow_kernels.inc; CPU
  // study tests/tools/root_start_study.py: 0.956 of the row-steps, the same partitions; DESIGN_EXPERIMENTS G10).  Part of the warm
  // start: AI_FLOW_WARM=0 is the pure hash start for these segments too.
  std::vector<const double*> h_xyz;   // per chunk: its points by original id (device), nullptr: none
  bool any_xyz = false;
  DevBuf<const double*> d_xyz;
  DevBuf<double> pca_part, pca_axis;  // FK_PCA_VALS planes of partials at the stable coarse indices; {axis, centre, scale} per record of a wave
  DevBuf<uint8_t> bin;
  DevBuf<int32_t> flag, fscan, map, newcnt, nscan, parent, rcnt, rc, ord, key, key_out, val, sorted_rows, final_order, scantmp;
  DevBuf<uint8_t> sorttmp;
  DevBuf<uint16_t> lidx;
  DevBuf<int32_t> ucol;
  DevBuf<TaskEnc> enc;
  DevBuf<int32_t> factive, cactive;
  DevBuf<double> pA;
  DevBuf<double2> pB0, pB1;
  DevBuf<int32_t> s_frozen, s_m, s_lastm, s_nextm;
  DevBuf<double> s_theta, s_resid, alpha_hist, b_hist, g_hist;
#ifdef AI_TRACE_HIST
  DevBuf<int4> sig_i, chk_i;
  DevBuf<double2> sig_d;
  DevBuf<double> chk_d;
#endif
  DevBuf<unsigned long long> work, tstamps, tblock;
  DevBuf<int32_t> dprog;  // the device's own step counter (steps below it are complete)
  DevBuf<int32_t> chk_ctr, chk_queue;  // fk_check: 8 x {queued, scan blocks done}; the segments due in a launch
  DevBuf<double*> d_slabtab;
  DevBuf<FTask> d_ft[RING];
  DevBuf<CTask> d_ct[RING];
  DevBuf<PoolSeg> d_ps[RING];
  DevBuf<SegRec> d_poolrec;
  // wave scratch
  DevBuf<SegRec> wrecP, wrecC;
  DevBuf<Task> fineP, coarseP, fineC, coarseC;
  DevBuf<double> pvol, psweep, w_scale, w_thr, w_vol, coef_d;
  DevBuf<double2> presid;        // per fine task of a wave's frozen segments: {sum r^2, sum ev^2} (fk_resid)
  long long n_restarted = 0;     // solves repeated after a failed true-residual test
  const char* guard_log = getenv("AI_FLOW_GUARD_LOG");   // diagnosis: file that receives T_m of every rejected Ritz pair and of its repeat
  std::vector<double> hist_copy;  // (guard_log) the wave's packed histories, kept past stage 2 (the pinned area is re-used)
  std::vector<double> coef_copy;  // (guard_log) ... and the Ritz coefficients that were uploaded
  double max_true_resid = 0.0;
  // ||M ev - theta ev|| / ||ev|| above which a 'converged' Ritz pair is rejected: healthy solves measure <= 1.0 x tol (the estimate
  // and the true residual agree to two digits on every segment of the bench chunks), a segment frozen early or on bad data is far above
  double true_resid_limit = 1e-6;
  // Test hooks (spoil the Ritz coefficients of the n-th harvested segment; reject a wave's packed rows once; another true-residual
  // limit; few Lanczos slots) exist in the test-only build alone (make lockstep: -DAI_TEST_HOOKS): the shipped library reads
  // nothing from the environment that can change a result.
#ifdef AI_TEST_HOOKS
  int inject = getenv("AI_FLOW_INJECT") ? atoi(getenv("AI_FLOW_INJECT")) : -1;
#else
  static constexpr int inject = -1;
#endif
#ifdef AI_TEST_HOOKS
  const char* dump_path = getenv("AI_FLOW_DUMP");  // one record per harvested / component-split segment appended here (dump_seg)
  DevBuf<double> w_costs;                           // the wave's 10 costs per segment as fk_sweep_final formed them
  double* dump_costs() { return dump_path ? w_costs.p : nullptr; }
#else
  double* dump_costs() { return nullptr; }
#endif
  long long n_above_limit = 0;     // Ritz pairs accepted above the limit because the repeated solve reproduced the residual bit for bit
  unsigned long long n_check_timeouts = 0;  // fk_check judging blocks that gave up waiting for the launch's scanning blocks
  long long n_harvested = 0;
  DevBuf<MinMaxPart> pmm;
  DevBuf<int32_t> w_nosplit, w_ncomp, troot, tsize, ccont_d;
  DevBuf<SplitSeg> ss_d;
  // slabs of Lanczos vectors [slot j][position]
  std::vector<double*> slabs;
  size_t slabtab_n = 0;
  double clock_khz = 0.0;
  // host state
  std::vector<FSeg> pool;  // segments listed in the current pool lists (some may be frozen already)
  std::deque<FSeg> pend_solved;
  std::vector<FSeg> pend_multi;
  std::vector<FLeaf> leaves;          // the groups, in the order they were found (sorted by start at the end of the call)
  std::vector<int> free_slots;
  RangeAlloc fa, ca;
  int J = 0;             // Lanczos steps launched so far
  int ver = 0;           // pool list version
  int nft = 0, nct = 0;  // tasks of the current pool lists
  int min_t0 = 0;
  int last_check_J = 0;
  char* pin = nullptr;
  bool need_relist = false;
  bool relist_urgent = false;  // segments are waiting to JOIN (a relist that only drops frozen segments may wait a few steps)
  int last_relist_J = 0;
  int wd_pg = -1, wd_J = -1;       // watchdog: last values of the device's and the host's step counters
  unsigned wd_iter = 0;
  struct Chk {
    int evi, J, npool, lver;
  };
  std::deque<Chk> checks;
  int nchecks = 0;
  // wave
  enum WState { W_IDLE, W_S1, W_S1H, W_S2, W_S3 };  // W_S1H: the helper thread is computing the wave's Ritz coefficients
  int ritz_err = 0;   // set by the helper thread: a frozen segment with an impossible size of T
  // set by the helper thread: a packed history row whose header does not match (device m != host m, or checksum): the wave asks again
  int hist_bad = 0, hist_bad_m_host = 0, hist_bad_row = 0, hist_bad_sum = 0, hist_tries = 0;
  double hist_bad_m_dev = 0.0;
  long long n_hist_retries = 0;
#ifdef AI_TEST_HOOKS
  int inject_hist = getenv("AI_FLOW_INJECT_HIST") ? atoi(getenv("AI_FLOW_INJECT_HIST")) : -1;  // reject the rows of the wave that holds the k-th harvested segment once
#else
  static constexpr int inject_hist = -1;
#endif
  WState wstate = W_IDLE;
  std::vector<FSeg> wA, wM, wP, wC;
  std::vector<int> wslots_to_free;
  int w_mp = 0, w_loM = 0, w_hiM = 0, w_coffM = 0, w_ncM = 0, w_nfA = 0, w_ncA = 0, w_nbin = 0, w_start_ver = 0;
  int32_t w_ncomp_all = 0;
  bool w_tab_pinned = false;
  std::vector<int32_t> h_troot, h_tsize;
  double t_pool = 0.0, t_pool_start = 0.0;
  double th_ritz = 0.0, th_s3 = 0.0, th_relist = 0.0, th_start = 0.0, th_finish = 0.0;  // host time per part (AI_NCUT_PHASES)
  long long n_starved = 0, n_ritz_segs = 0, n_relist = 0, stats_deferred = 0;
  long long n_stamped_blocks = 0;   // (profiling) blocks of the stamped SpMV launches
  bool pool_running = false;
  bool debug = getenv("AI_NCUT_DEBUG") != nullptr;
  bool trace = debug && atoi(getenv("AI_NCUT_DEBUG")) == 2;  // one line per harvested segment, nothing else
  std::vector<double> w_theta;
  int force_plain = (getenv("AI_SPMV_VARIANT") && atoi(getenv("AI_SPMV_VARIANT")) == 1) ? 1 : 0;  // test hook: plain gather of R_j everywhere
  volatile int32_t* progress = nullptr;  // pinned: the last step whose update kernel has started
  double t_progress = 0.0, t_call = now_ms();


  // PIN_UP: first half = the wave's stage area (bump-allocated, reset per stage: a stage's tables are consumed when its
  // event has completed), second half = ring of pool record tables (consumed by fk_expand_pool on the main stream)
  static constexpr int POOL_SLOTS = 8;
  static constexpr size_t POOL_SLOT_BYTES = PIN_UP / 2 / POOL_SLOTS;
  size_t wpin_off = 0;
  char* wpin(size_t bytes) {
    wpin_off = (wpin_off + 15) & ~(size_t)15;
    if (wpin_off + bytes > PIN_UP / 2) return nullptr;
    char* p = pin + wpin_off;
    wpin_off += bytes;
    return p;
  }
  int pool_slot = 0;
  bool pool_slot_used[POOL_SLOTS] = {false};
  // the regions of the pinned area; what lies inside them is ai_flow_host.h's to say
  char* pin_status() { return pin + PIN_OFF_STATUS; }
  char* pin_res() { return pin + PIN_OFF_RES; }
  char* pin_hist() { return pin + PIN_OFF_HIST; }
  char* pin_coef() { return pin + PIN_OFF_COEF; }
  double* hist_rows() { return (double*)pin_hist(); }   // HistRows(w_mp)
  double* coef_host() { return (double*)pin_coef(); }   // CoefTable(nA, w_mp, warm)

  FlowLz lz() {
    FlowLz L;
    L.frozen = s_frozen.p;
    L.m = s_m.p;
    L.alpha_hist = alpha_hist.p;
    L.b_hist = b_hist.p;
    L.g_hist = g_hist.p;
    L.factive = factive.p;
    L.cactive = cactive.p;
    L.mcap = mcap;
#ifdef AI_TRACE_HIST
    L.sig_i = sig_i.p, L.sig_d = sig_d.p, L.chk_i = chk_i.p, L.chk_d = chk_d.p;
#endif
    return L;
  }

  // ---- context-owned resources (created on the first call, kept for the life of the context)
  int ensure_ctx() {
    if (!ctx->wave) AI_HIP(hipStreamCreateWithFlags(&ctx->wave, hipStreamNonBlocking));
    if (!ctx->fpin) AI_HIP(hipHostMalloc((void**)&ctx->fpin, PIN_TOTAL, hipHostMallocCoherent));
    for (int i = 0; i < AI_FLOW_EVENTS; ++i)
      if (!ctx->fev[i]) AI_HIP(hipEventCreateWithFlags(&ctx->fev[i], hipEventDisableTiming));
    sw = ctx->wave;
    pin = ctx->fpin;
    progress = res_progress(pin_res());
    *progress = 0;
    return AI_OK;
  }
  hipEvent_t wave_ev() { return ctx->fev[AI_FLOW_UPSLOTS]; }
  hipEvent_t mark_ev() { return ctx->fev[AI_FLOW_UPSLOTS + 1]; }

  int ensure_vec(int j) {
    while ((size_t)j / AI_SLAB_VECS >= slabs.size()) {
      const size_t bytes = (size_t)AI_SLAB_VECS * (size_t)W * sizeof(double);
      double* p = nullptr;
      if (ai_arena* a = ai_current_arena()) p = (double*)a->alloc(bytes);
      if (!p) {
        ai_set_error("Lanczos vector slab %zu (%zu bytes) could not be allocated", slabs.size(), bytes);
        return AI_ERR_OOM;
      }
      slabs.push_back(p);
    }
    return AI_OK;
  }
  int sync_slabtab() {
    if (slabtab_n == slabs.size()) return AI_OK;
    if (slabs.size() > 500) {
      ai_set_error("internal: more than 500 Lanczos slabs");
      return AI_ERR_INTERNAL;
    }
    // the table only ever grows by appending: rewriting the pinned copy while an earlier upload is in flight is harmless
    double** tab = res_slab_table(pin_res());  // second half of the result area: the wave's results stay below
    for (size_t i = 0; i < slabs.size(); ++i) tab[i] = slabs[i];
    AI_HIP(hipMemcpyAsync(d_slabtab.p, tab, slabs.size() * sizeof(double*), hipMemcpyHostToDevice, sm));
    slabtab_n = slabs.size();
    return AI_OK;
  }

  // records of a list of segments, tasks numbered back to back
  static void make_recs(const std::vector<FSeg>& segs, std::vector<SegRec>& out, int& nf, int& nc) {
    out.resize(segs.size());
    nf = nc = 0;
    for (size_t i = 0; i < segs.size(); ++i) {
      const FSeg& s = segs[i];
      SegRec r;
      r.g0 = s.g0;
      r.n = s.n;
      r.slot = s.slot;
      r.par = s.par;
      r.f0 = s.f0;
      r.c0 = s.c0;
      r.foff = nf;
      r.coff = nc;
      r.t0 = s.t0;
      r.cap = s.cap;
      r.idx = (int)i;
      r.aux = s.aux;
      r.vdelta = s.vdelta;
      r.pad0 = s.warm_n;
      r.pad1 = s.pca;
      r.pad2 = 0;
      out[i] = r;
      nf += fk_nf(s.n);
      nc += fk_nc(s.n);
    }
  }

  int setup(const ai_csr* A, int nchunks_, const int64_t* off_, const int64_t* n_orig_, double T_) {
    AI_TRY(ensure_ctx());
    N = (int)A->n;
    E = A->nnz;
    nchunks = nchunks_;
    off = off_;
    n_orig = n_orig_;
    T = T_;
    mcap = std::max(1, opt.max_iter);
    {
      int64_t big = 0;
      for (int c = 0; c < nchunks; ++c) big = std::max<int64_t>(big, off[c + 1] - off[c]);
      if (window_rows <= 0) window_rows = 4800000;
      W = (int)std::min<int64_t>(N, std::max<int64_t>(window_rows, big));
      sa.init(W);
      chunk_sbase.assign(nchunks, -1);
      chunk_live.assign(nchunks, 0);
    }
    if (opt.check_every > 64) opt.check_every = 64;
    SMAX = std::min(208 * nchunks + 64, (int)(STATUS_BYTES / sizeof(int32_t)));
#ifdef AI_TEST_HOOKS
    if (const char* e = getenv("AI_FLOW_SMAX")) SMAX = std::max(4, std::min(SMAX, atoi(e)));  // few Lanczos slots, so that children have to wait for one (children_prep)
#endif
    WCAP = 2 * SMAX;
    FCAP = 2 * (N / AI_FINE_ROWS + SMAX) + 64;
    CCAP = 2 * (N / AI_COARSE_ROWS + SMAX) + 64;
    FLIST = N / AI_FINE_ROWS + WCAP + 64;
    CLIST = N / AI_COARSE_ROWS + WCAP + 64;
    const size_t n = (size_t)N, e = (size_t)E;
    AI_TRY(rowse0.alloc(n));
    AI_TRY(rowse1.alloc(n));
    AI_TRY(col1.alloc(e));
    AI_TRY(w1.alloc(e));
    AI_TRY(orig1.alloc(n));
    G.rowse[0] = rowse0.p;
    G.rowse[1] = rowse1.p;
    G.col[0] = A->col;
    G.col[1] = col1.p;
    G.w[0] = A->val;
    G.w[1] = w1.p;
    G.orig[0] = A->orig;
    G.orig[1] = orig1.p;
    AI_TRY(deg.alloc(n));
    AI_TRY(sinv.alloc(n));
    AI_TRY(sinv2.alloc(n));
    AI_TRY(u1.alloc(n));
    AI_TRY(wm.alloc(e + 8));
    AI_TRY(ev.alloc(n));
    AI_TRY(Z.alloc(n));
    if (warm) {
      AI_TRY(ev2.alloc(n));
      AI_TRY(warmv.alloc(n));
      h_xyz.assign((size_t)nchunks, nullptr);
      for (int c = 0; c < nchunks; ++c) {
        h_xyz[c] = A->chunk_xyz ? A->chunk_xyz[c] : (nchunks == 1 ? (const double*)A->xyz : nullptr);
        any_xyz |= h_xyz[c] != nullptr;
      }
      if (any_xyz) {
        AI_TRY(d_xyz.alloc((size_t)nchunks));
        AI_TRY(pca_part.alloc((size_t)FK_PCA_VALS * CCAP));
        AI_TRY(pca_axis.alloc((size_t)8 * WCAP));
        AI_HIP(hipMemcpyAsync(d_xyz.p, h_xyz.data(), (size_t)nchunks * sizeof(const double*), hipMemcpyHostToDevice, sm));
      }
    }
    AI_TRY(bin.alloc(n));
    AI_TRY(flag.alloc(n + 1));
    AI_TRY(fscan.alloc(n + 1));
    AI_TRY(map.alloc(n));
    AI_TRY(newcnt.alloc(n + 1));
    AI_TRY(nscan.alloc(n + 1));
    AI_TRY(parent.alloc(n));
    AI_TRY(rcnt.alloc(n));
    AI_TRY(rc.alloc(n + 1));
    AI_TRY(ord.alloc(n + 1));
    AI_TRY(key.alloc(n));
    AI_TRY(key_out.alloc(n));
    AI_TRY(val.alloc(n));
    AI_TRY(sorted_rows.alloc(n));
    AI_TRY(final_order.alloc(n));
    AI_TRY(scantmp.alloc(ai_scan_tmp_elems((int64_t)n)));
    AI_TRY(lidx.alloc(e + 8));
    AI_TRY(ucol.alloc(e + 8));
    AI_TRY(enc.alloc((size_t)FCAP));
    AI_TRY(factive.alloc((size_t)FCAP));
    AI_TRY(cactive.alloc((size_t)CCAP));
    AI_TRY(pA.alloc((size_t)FCAP));
    AI_TRY(pB0.alloc((size_t)CCAP));
    AI_TRY(pB1.alloc((size_t)CCAP));
    AI_TRY(s_frozen.alloc((size_t)SMAX));
    AI_TRY(s_m.alloc((size_t)SMAX));
    AI_TRY(s_lastm.alloc((size_t)SMAX));
    AI_TRY(s_nextm.alloc((size_t)SMAX));
    AI_TRY(s_theta.alloc((size_t)SMAX));
    AI_TRY(s_resid.alloc((size_t)SMAX));
    AI_TRY(alpha_hist.alloc((size_t)SMAX * mcap));
    AI_TRY(b_hist.alloc((size_t)SMAX * (mcap + 1)));
    AI_TRY(g_hist.alloc((size_t)SMAX * (mcap + 1)));
#ifdef AI_TRACE_HIST
    AI_TRY(sig_i.alloc((size_t)SMAX * 64));
    AI_TRY(sig_d.alloc((size_t)SMAX * 64));
    AI_TRY(chk_i.alloc((size_t)SMAX));
    AI_TRY(chk_d.alloc((size_t)SMAX * 8));
#endif
    AI_TRY(work.alloc(8));
    AI_TRY(dprog.alloc(1));
    AI_TRY(chk_ctr.alloc(16));
    AI_TRY(chk_queue.alloc((size_t)SMAX));
    AI_HIP(hipMemsetAsync(chk_ctr.p, 0, 16 * sizeof(int32_t), sm));
    AI_HIP(hipMemsetAsync(dprog.p, 0, sizeof(int32_t), sm));
    memset(pin_status(), 0, (size_t)SMAX * sizeof(int32_t));
    AI_TRY(d_slabtab.alloc(512));
    for (int r = 0; r < RING; ++r) {
      AI_TRY(d_ft[r].alloc((size_t)FLIST));
      AI_TRY(d_ct[r].alloc((size_t)CLIST));
      AI_TRY(d_ps[r].alloc((size_t)SMAX));
    }
    AI_TRY(d_poolrec.alloc((size_t)SMAX));
    AI_TRY(wrecP.alloc((size_t)WCAP));
    AI_TRY(wrecC.alloc((size_t)WCAP));
    AI_TRY(fineP.alloc((size_t)FLIST));
    AI_TRY(coarseP.alloc((size_t)CLIST));
    AI_TRY(fineC.alloc((size_t)FLIST));
    AI_TRY(coarseC.alloc((size_t)CLIST));
    AI_TRY(pvol.alloc((size_t)FLIST));
    AI_TRY(psweep.alloc((size_t)FLIST * AI_SWEEP_VALS));
    AI_TRY(presid.alloc((size_t)FLIST));
    AI_TRY(pmm.alloc((size_t)CLIST));
    AI_TRY(w_scale.alloc((size_t)WCAP));
    AI_TRY(w_thr.alloc((size_t)WCAP * AI_NUM_CUTS));
#ifdef AI_TEST_HOOKS
    if (dump_path) AI_TRY(w_costs.alloc((size_t)WCAP * AI_NUM_CUTS));
#endif
    AI_TRY(w_vol.alloc((size_t)WCAP));
    AI_TRY(w_nosplit.alloc((size_t)WCAP));
    AI_TRY(w_ncomp.alloc((size_t)WCAP));
    AI_TRY(ss_d.alloc((size_t)WCAP));
    AI_TRY(coef_d.alloc(COEF_DEV_DOUBLES));
    if (clock_spmv) {
      AI_TRY(tstamps.alloc((size_t)2 * TS_CAP));
      AI_TRY(tblock.alloc((size_t)2 * (FLIST + 1)));
      AI_HIP(hipMemsetAsync(tstamps.p, 0, (size_t)2 * TS_CAP * sizeof(unsigned long long), sm));
      int khz = 0;
      AI_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
      clock_khz = khz > 0 ? (double)khz : 100000.0;
    }
    AI_HIP(hipMemsetAsync(work.p, 0, 8 * sizeof(unsigned long long), sm));
    AI_HIP(hipMemsetAsync(s_frozen.p, 0, (size_t)SMAX * sizeof(int32_t), sm));
    AI_HIP(hipMemsetAsync(factive.p, 0, (size_t)FCAP * sizeof(int32_t), sm));
    AI_HIP(hipMemsetAsync(cactive.p, 0, (size_t)CCAP * sizeof(int32_t), sm));
    hipLaunchKernelGGL(fk_rowse_from_rowptr, dim3((N + AI_BLOCK - 1) / AI_BLOCK), dim3(AI_BLOCK), 0, sm, (const int32_t*)A->rowptr, N, rowse0.p);
    AI_KERNEL_CHECK();
    AI_HIP(hipMemcpyAsync(final_order.p, A->orig, n * sizeof(int32_t), hipMemcpyDeviceToDevice, sm));
    fa.init(FCAP);
    ca.init(CCAP);
    free_slots.clear();
    for (int s = SMAX - 1; s >= 0; --s) free_slots.push_back(s);
    AI_TRY(ensure_vec(1));
    AI_HIP(hipStreamSynchronize(sm));  // the wave stream starts from a finished set-up
    return AI_OK;
  }

  // ------------------------------------------------------------------------------------------------- the pool
  int relist() {
    ++ver;
    const int cur = ver % RING;
    // a check that still reads this ring entry's lists must have finished
    for (;;) {
      bool any = false;
      for (auto& c : checks) any |= (c.lver % RING == cur);
      if (!any) break;
      AI_TRY(reap_check(true));
    }
    pool.erase(std::remove_if(pool.begin(), pool.end(), [](const FSeg& s) { return s.frozen; }), pool.end());
    need_relist = relist_urgent = false;
    last_relist_J = J;
    nft = nct = 0;
    min_t0 = J;
    if (pool.empty()) {
      if (pool_running) {
        t_pool += now_ms() - t_pool_start;
        pool_running = false;
      }
      return AI_OK;
    }
    if ((int)pool.size() > SMAX) {
      ai_set_error("internal: %zu segments in the pool (capacity %d)", pool.size(), SMAX);
      return AI_ERR_INTERNAL;
    }
    std::vector<SegRec> recs;
    make_recs(pool, recs, nft, nct);
    if (nft > FLIST || nct > CLIST) {
      ai_set_error("internal: pool task lists overflow (%d / %d fine, %d / %d coarse)", nft, FLIST, nct, CLIST);
      return AI_ERR_INTERNAL;
    }
    for (auto& s : pool) min_t0 = std::min(min_t0, s.t0);
    if (recs.size() * sizeof(SegRec) > POOL_SLOT_BYTES) {
      ai_set_error("internal: %zu pool records exceed a pinned table slot", recs.size());
      return AI_ERR_INTERNAL;
    }
    const int ps = pool_slot;
    pool_slot = (pool_slot + 1) % POOL_SLOTS;
    if (pool_slot_used[ps]) AI_HIP(hipEventSynchronize(ctx->fev[ps]));  // the expansion that read this slot last (long done)
    char* prec = pin + PIN_UP / 2 + (size_t)ps * POOL_SLOT_BYTES;
    memcpy(prec, recs.data(), recs.size() * sizeof(SegRec));
    hipLaunchKernelGGL(fk_expand_pool, dim3((unsigned)pool.size()), dim3(AI_BLOCK), 0, sm, (const SegRec*)prec, (const TaskEnc*)enc.p, force_plain,
                       d_ft[cur].p, d_ct[cur].p, d_ps[cur].p);
    AI_KERNEL_CHECK();
    AI_HIP(hipEventRecord(ctx->fev[ps], sm));
    pool_slot_used[ps] = true;
    // checks are not ordered against the stepping stream, except here: they must not read these lists before they are written
    AI_HIP(hipStreamWaitEvent(ss, ctx->fev[ps], 0));
    if (!pool_running) {
      t_pool_start = now_ms();
      pool_running = true;
    }
    return AI_OK;
  }

  int step() {
    const int cur = ver % RING;
    AI_TRY(ensure_vec(J - min_t0 + 1));
    AI_TRY(sync_slabtab());
    const FlowLz L = lz();
    unsigned long long* ts = (clock_spmv && J < TS_CAP) ? tblock.p : (unsigned long long*)nullptr;
    if (ts)
      hipLaunchKernelGGL((fk_spmv<AI_ROW_ILP, true>), dim3(nft), dim3(AI_BLOCK), 0, sm, (const FTask*)d_ft[cur].p, nft, J, (double* const*)d_slabtab.p,
                         (size_t)W, (const int32_t*)ucol.p, (const uint16_t*)lidx.p, (const double*)wm.p, (const double*)sinv2.p, L, G, Z.p, pA.p, ts, work.p + 5);
    else
      hipLaunchKernelGGL((fk_spmv<AI_ROW_ILP, false>), dim3(nft), dim3(AI_BLOCK), 0, sm, (const FTask*)d_ft[cur].p, nft, J, (double* const*)d_slabtab.p,
                         (size_t)W, (const int32_t*)ucol.p, (const uint16_t*)lidx.p, (const double*)wm.p, (const double*)sinv2.p, L, G, Z.p, pA.p, ts, work.p + 5);
    AI_KERNEL_CHECK();
    if (ts) {
      n_stamped_blocks += nft;
      hipLaunchKernelGGL(k_ts_reduce, dim3(1), dim3(AI_BLOCK), 0, sm, (const unsigned long long*)tblock.p, nft, tstamps.p + 2 * (size_t)J);
      AI_KERNEL_CHECK();
      if (debug && getenv("AI_NCUT_BLOCKS") && J == atoi(getenv("AI_NCUT_BLOCKS"))) {
        // experiment: residence time of every block of this one launch (device clock, 10 ns ticks)
        std::vector<unsigned long long> hb((size_t)2 * nft);
        AI_HIP(hipStreamSynchronize(sm));
        AI_HIP(hipMemcpy(hb.data(), tblock.p, hb.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull, t1 = 0;
        double sum = 0.0;
        std::vector<double> dur;
        for (int b = 0; b < nft; ++b) {
          if (hb[2 * b + 1] <= hb[2 * b]) continue;
          t0 = std::min(t0, hb[2 * b]);
          t1 = std::max(t1, hb[2 * b + 1]);
          dur.push_back((double)(hb[2 * b + 1] - hb[2 * b]));
          sum += dur.back();
        }
        std::sort(dur.begin(), dur.end());
        const double tick_us = 1e3 / clock_khz;
        // how many blocks had started by 10 %, 25 %, 50 %, 75 % of the span
        int started[4] = {0, 0, 0, 0};
        for (int b = 0; b < nft; ++b)
          for (int q = 0; q < 4; ++q)
            if (hb[2 * b + 1] > hb[2 * b] && (double)(hb[2 * b] - t0) <= (q == 0 ? 0.10 : q == 1 ? 0.25 : q == 2 ? 0.5 : 0.75) * (double)(t1 - t0)) ++started[q];
        if (!dur.empty())
          fprintf(stderr, "[blocks] J=%d blocks=%d live=%zu span=%.2f us; residence us: mean %.2f p10 %.2f p50 %.2f p90 %.2f max %.2f; mean blocks in flight %.0f; started by 10/25/50/75 %% of the span: %d %d %d %d\n",
                  J, nft, dur.size(), (double)(t1 - t0) * tick_us, sum / dur.size() * tick_us, dur[dur.size() / 10] * tick_us, dur[dur.size() / 2] * tick_us,
                  dur[dur.size() * 9 / 10] * tick_us, dur.back() * tick_us, sum / (double)(t1 - t0), started[0], started[1], started[2], started[3]);
      }
    }
    hipLaunchKernelGGL(fk_update, dim3(nct), dim3(AI_BLOCK), 0, sm, (const CTask*)d_ct[cur].p, J, L, (const double*)pA.p, pB0.p, pB1.p,
                       (const double*)u1.p, (const double*)Z.p, (double* const*)d_slabtab.p, (size_t)W, (int32_t*)progress, dprog.p);
    AI_KERNEL_CHECK();
    ++J;
    return AI_OK;
  }

  // One check launch on the side stream: not ordered against the stepping stream (fk_check reads the device's own step
  // counter); frozen segments appear in pinned status[slot].  The event only guards the re-use of slots and list buffers.
  int launch_check() {
    while ((int)checks.size() >= AI_CHECK_DEPTH - 1) AI_TRY(reap_check(true));
    const int cur = ver % RING;
    const int cd = nchecks % AI_CHECK_DEPTH;
    const int npool = (int)pool.size();
    const FlowLz L = lz();
    const int lds_m = (std::max(1, std::min(J - min_t0, mcap)) + 63) & ~63;   // fk_check keeps T lane-interleaved: 64 x ceil(m / 64) rows
    const int with_rb = (size_t)3 * lds_m * sizeof(double) <= (size_t)64 * 1024;
    // ceil(npool / 256) scanning blocks + FK_CHECK_JUDGES judging blocks (fk_check)
    const int ncb = (npool + AI_CHECK_THREADS - 1) / AI_CHECK_THREADS + FK_CHECK_JUDGES;
    hipLaunchKernelGGL(fk_check, dim3(ncb), dim3(AI_CHECK_THREADS), (size_t)(with_rb ? 3 : 2) * lds_m * sizeof(double), ss, (const PoolSeg*)d_ps[cur].p, npool,
                       nchecks, chk_ctr.p, chk_queue.p,
                       (const int32_t*)dprog.p, L, G, opt.tol, lds_m, s_theta.p, s_resid.p, s_lastm.p, s_nextm.p, work.p, with_rb,
                       (int32_t*)pin_status());
    AI_KERNEL_CHECK();
    AI_HIP(hipEventRecord(ctx->chk_ev[cd], ss));
    Chk c;
    c.evi = cd;
    c.J = J;
    c.npool = npool;
    c.lver = ver;
    checks.push_back(std::move(c));
    ++nchecks;
    last_check_J = J;
    return AI_OK;
  }

  // segments the device has frozen since the last look (status[slot] = rows of T)
  void scan_status() {
    const volatile int32_t* st = (const volatile int32_t*)pin_status();
    for (auto& s : pool)
      if (!s.frozen && st[s.slot] > 0) {
        s.frozen = true;
        s.m = st[s.slot];
        pend_solved.push_back(s);
        need_relist = true;
      }
  }

  // the oldest in-flight check: read its result if it has arrived (or wait for it)
  int reap_check(bool block) {
    if (checks.empty()) return AI_OK;
    Chk& c = checks.front();
    hipEvent_t e = ctx->chk_ev[c.evi];
    if (block) {
      AI_HIP(hipEventSynchronize(e));
    } else {
      hipError_t q = hipEventQuery(e);
      if (q == hipErrorNotReady) return AI_OK;
      AI_HIP(q);
    }
    checks.pop_front();
    return AI_OK;
  }

  // ------------------------------------------------------------------------------------------------- waves
  // records of `segs` -> pinned stage area -> (on the device) a kept copy + the task lists; up to two small host tables ride along
  int expand(const std::vector<FSeg>& segs, DevBuf<SegRec>& drec, Task* fine, Task* coarse, int stable, int& nf, int& nc, Rider x0 = {}, Rider x1 = {}) {
    if (segs.empty()) {
      nf = nc = 0;
      return AI_OK;
    }
    if ((int)segs.size() > WCAP || !res_child_comps_fit(segs.size())) {
      ai_set_error("internal: %zu segments in one wave (capacity %d)", segs.size(), WCAP);
      return AI_ERR_INTERNAL;
    }
    std::vector<SegRec> recs;
    make_recs(segs, recs, nf, nc);
    if (nf > FLIST || nc > CLIST) {
      ai_set_error("internal: wave task lists overflow (%d fine, %d coarse)", nf, nc);
      return AI_ERR_INTERNAL;
    }
    const size_t r0 = (x0.bytes + 15) & ~(size_t)15, r1 = (x1.bytes + 15) & ~(size_t)15;
    char* pr = wpin(recs.size() * sizeof(SegRec));
    char* p0 = r0 ? wpin(r0) : nullptr;
    char* p1 = r1 ? wpin(r1) : nullptr;
    if (!pr || (r0 && !p0) || (r1 && !p1)) {
      ai_set_error("internal: the wave's pinned stage area is full");
      return AI_ERR_INTERNAL;
    }
    memcpy(pr, recs.data(), recs.size() * sizeof(SegRec));
    if (r0) memcpy(p0, x0.host, x0.bytes);
    if (r1) memcpy(p1, x1.host, x1.bytes);
    hipLaunchKernelGGL(fk_expand_wave, dim3((unsigned)segs.size()), dim3(AI_BLOCK), 0, sw, (const SegRec*)pr, drec.p, fine, coarse, stable, (const int4*)p0,
                       (int4*)x0.dev, (int)(r0 / 16), (const int4*)p1, (int4*)x1.dev, (int)(r1 / 16));
    AI_KERNEL_CHECK();
    return AI_OK;
  }

  void leaf(int g0, double front, double cost) { leaves.push_back(FLeaf{g0, front, cost}); }

  // A segment gives back what it holds of the pool: its stable task ranges at once, its Lanczos slot to `slots` -- free_slots where
  // nothing on the device can name the slot any more, wslots_to_free for a harvested parent (checks launched before it left the
  // lists may still name it: wave_finish frees those after children_prep has reaped them).  The record keeps its numbers: a parent
  // that split is listed once more with them; who lets the segment wait clears them (FSeg::detach).
  void give_back(const FSeg& s, std::vector<int>& slots) {
    if (s.slot >= 0) slots.push_back(s.slot);
    if (s.f0 >= 0) fa.release(s.f0, fk_nf(s.n));
    if (s.c0 >= 0) ca.release(s.c0, fk_nc(s.n));
  }

  // chunks whose last segment has become a group give their slab rows back; waiting chunks take them
  int retire_chunks() {
    bool freed = false;
    for (int c = 0; c < nchunks; ++c)
      if (chunk_sbase[c] >= 0 && chunk_live[c] == 0) {
        sa.release(chunk_sbase[c], (int)(off[c + 1] - off[c]));
        chunk_sbase[c] = -1;
        freed = true;
      }
    if (freed) admit();
    return AI_OK;
  }
  void admit() {
    while (!waiting.empty()) {
      const int c = waiting.front();
      const int nc = (int)(off[c + 1] - off[c]);
      const int sb = sa.alloc(nc);
      if (sb < 0) break;
      waiting.pop_front();
      chunk_sbase[c] = sb;
      chunk_live[c] = 1;
      FSeg s;
      s.g0 = (int)off[c];
      s.n = nc;
      s.chunk = c;
      s.par = 0;
      s.binary_child = true;
      s.vdelta = sb - (int)off[c];
      new_roots.push_back(s);
    }
  }

  // stage 1: histories of the frozen segments to the host; component counts of the disconnected ones
  int start_wave() {
    wpin_off = 0;
    ++stats.levels;
    w_start_ver = ver;
    wA.clear();
    wM.clear();
    // as many frozen segments as the pinned history / coefficient buffers take
    w_mp = 0;
    while (!pend_solved.empty() && wA.size() < (size_t)WAVE_MAX_SEGS) {
      const int mp = std::max(w_mp, pend_solved.front().m);
      const size_t k = wA.size() + 1;
      if (!wave_fits(k, (size_t)mp, warm != 0)) {
        if (wA.empty()) {
          ai_set_error("internal: one segment's T (%d rows) exceeds the pinned buffers", mp);
          return AI_ERR_INTERNAL;
        }
        break;
      }
      w_mp = mp;
      wA.push_back(pend_solved.front());
      pend_solved.pop_front();
    }
    wM.swap(pend_multi);
    std::sort(wM.begin(), wM.end(), [](const FSeg& a, const FSeg& b) { return a.g0 < b.g0; });
    wP = wA;
    wP.insert(wP.end(), wM.begin(), wM.end());
    int nf = 0, nc = 0;
    AI_HIP(hipEventRecord(mark_ev(), sm));
    AI_HIP(hipStreamWaitEvent(sw, mark_ev(), 0));
    AI_TRY(expand(wP, wrecP, fineP.p, coarseP.p, 0, nf, nc));
    w_nfA = w_ncA = 0;
    for (auto& s : wA) {
      w_nfA += fk_nf(s.n);
      w_ncA += fk_nc(s.n);
    }
    w_coffM = w_ncA;
    w_ncM = nc - w_ncA;
    const FlowLz L = lz();
    if (!wA.empty()) {
      stats.lanczos_solves += (int64_t)wA.size();
      hipLaunchKernelGGL(fk_pack_hist, dim3((unsigned)wA.size()), dim3(AI_BLOCK), 0, sw, (const SegRec*)wrecP.p, L, (const double*)s_theta.p,
                         (const double*)s_resid.p, w_mp, hist_rows());  // straight into pinned host memory
      AI_KERNEL_CHECK();
    }
    if (!wM.empty()) {
      stats.null_solves += (int64_t)wM.size();
      w_loM = wM.front().g0;
      w_hiM = wM.back().g0 + wM.back().n;
      const int len = w_hiM - w_loM;
      hipLaunchKernelGGL(fk_iota2, dim3((len + AI_BLOCK - 1) / AI_BLOCK), dim3(AI_BLOCK), 0, sw, key.p, val.p, rcnt.p, rc.p, w_loM, w_hiM);
      AI_KERNEL_CHECK();
      hipLaunchKernelGGL(fk_rootcount, dim3(w_ncM), dim3(AI_BLOCK), 0, sw, (const Task*)(coarseP.p + w_coffM), (const int32_t*)parent.p, rcnt.p);
      AI_KERNEL_CHECK();
      hipLaunchKernelGGL(fk_rootflag, dim3(w_ncM), dim3(AI_BLOCK), 0, sw, (const Task*)(coarseP.p + w_coffM), (const int32_t*)parent.p, rc.p, key.p);
      AI_KERNEL_CHECK();
      AI_TRY(ai_exclusive_scan_i32(sw, rc.p + w_loM, ord.p + w_loM, len, scantmp.p, res_comp_total(pin_res())));  // the total straight into pinned memory
    }
    if (wM.empty() && wA.empty()) return wave_s2();  // only new roots: nothing for the host to do in between (no coefficients either)
    AI_HIP(hipEventRecord(wave_ev(), sw));
    wstate = W_S1;
    return AI_OK;
  }

  // stage 2: Ritz vectors + sweep of the frozen segments; component table of the disconnected ones.
  // The Ritz coefficients (eigenvector of every frozen segment's T_m: bisection + pivoted inverse iteration, ~20 us per segment,
  // 18 ms of a 12-chunk call) are computed by the context's helper thread while this thread keeps the stepping stream fed
  // (it launched on a drained queue ~70 times per call while it did that work itself); the wave waits in W_S1H meanwhile.
  // The same on the device (one wave per segment, T in LDS) was built in round 3 and was slower than the host round trip.
  int wave_s2_begin() {
    const size_t nA = wA.size();
    if (!nA) return wave_s2();
    if (trace) w_theta.assign(nA, 0.0);
    ritz_err = 0;
    const double t_r0 = now_ms();
    ctx->helper.submit([this, nA] { ritz_job(nA); });
    th_ritz += now_ms() - t_r0;
    n_ritz_segs += (long long)nA;
    wstate = W_S1H;
    return AI_OK;
  }
  // (helper thread) reads the packed histories in pinned memory, writes the packed upload {cu[nA], m[nA], coef[nA][mp]} and resid[nA]
  void ritz_job(size_t nA) {
    double* pr_resid = WaveResults(nA).resid(res_wave(pin_res()));
    const HistRows H((size_t)w_mp);
    const double* hp = hist_rows();
    const CoefTable C(nA, (size_t)w_mp, warm != 0);
    double* const ct = coef_host();
    double *h_cu = C.cu(ct), *h_th = C.theta(ct), *h_cu2 = C.cu2(ct);   // (warm start) second Ritz vector: cu2[nA], coef2[nA][mp]
    int32_t* h_m = C.m(ct);
    std::vector<double> sv, sv2;
    std::vector<std::vector<double>> prevv(1);
    const std::vector<int> cluster0{0};
    // every row first: the device's size of T equals the host's, and the row's integer checksum holds (fk_pack_hist)
    hist_bad = 0;
    for (size_t i = 0; i < nA; ++i) {
      const FSeg& s = wA[i];
      const double* row = H.row(hp, i);
      const int m = s.m;
      if (m <= 0 || m > w_mp) {
        ritz_err = m == 0 ? -1 : m;
        return;
      }
      const bool sum_ok = H.sum_matches(row, m);
      const bool spoil = inject_hist >= 0 && n_harvested + (long long)i == inject_hist && hist_tries == 0;  // test hook
      if (!H.m_matches(row, m) || !sum_ok || spoil) {
        hist_bad = 1;
        hist_bad_m_dev = H.m_dev(row);
        hist_bad_m_host = m;
        hist_bad_row = (int)i;
        hist_bad_sum = !sum_ok;
        return;
      }
    }
    for (size_t i = 0; i < nA; ++i) {
      const FSeg& s = wA[i];
      const double* row = H.row(hp, i);
      const double h_theta = H.theta(row), h_resid = H.resid(row);
      const double *a = H.a(row), *b = H.b(row), *g = H.g(row);
      const int m = s.m;
      double theta = 0.0;
      ai_tridiag_top(a, b, m, (h_theta > 0.0) ? &h_theta : nullptr, &theta, sv);
      double cu = 0.0;
      double* c = C.coef(ct, i);
      for (int j = 0; j < m; ++j) {
        const double cj = sv[j] / b[j];  // v_j = (R_j - g_j u1) / b_j
        c[j] = cj;
        cu -= cj * g[j];
      }
      for (int j = m; j < w_mp; ++j) c[j] = 0.0;
      if (inject >= 0 && n_harvested + (long long)i == inject && s.restarts == 0) {
        // test hook: a Ritz pair as a check that froze on bad data would leave it (the coefficients of another vector)
        for (int j = 0; j < m / 2; ++j) std::swap(c[j], c[m - 1 - j]);
      }
      if (warm) {
        double* c2 = C.coef2(ct, i);
        double cu2 = 0.0;
        if (m >= 2) {
          // The next Ritz vector(s) below the top one, cheaply: inverse iteration with a shift just below theta, kept orthogonal to
          // the top eigenvector, converges to the eigenvector whose eigenvalue is nearest below (a mix of the next few when they are
          // close: as good a start for the children).  Locating theta_2 by bisection first cost the helper thread ~80 us per
          // segment -- 66 ms per 12-chunk call, and the waves of a call alone waited for it (call 103 -> 117 ms).
          prevv[0] = sv;
          ai_tridiag_eigvec(a, b, m, theta - 1e-4 * std::max(1.0, fabs(theta)), prevv, cluster0, sv2);
          for (int j = 0; j < m; ++j) {
            const double cj = sv2[j] / b[j];
            c2[j] = cj;
            cu2 -= cj * g[j];
          }
          for (int j = m; j < w_mp; ++j) c2[j] = 0.0;
        } else {
          for (int j = 0; j < w_mp; ++j) c2[j] = 0.0;
        }
        h_cu2[i] = cu2;
      }
      h_cu[i] = cu;
      h_th[i] = theta;
      h_m[i] = m;
      if (trace) w_theta[i] = theta;
      pr_resid[i] = h_resid;
    }
    if (guard_log) {
      hist_copy.assign(hp, hp + H.doubles(nA));
      coef_copy.assign(ct, ct + C.top_doubles());
    }
  }
  int wave_s2() {
    wpin_off = 0;
    const size_t nA = wA.size();
    const CoefTable C(nA, (size_t)w_mp, warm != 0);
    const double* const cd = coef_d.p;
    // results straight into pinned host memory (WaveResults)
    const WaveResults R(nA);
    char* const rw = res_wave(pin_res());
    if (nA && hist_bad) {
      // a row of the packed histories arrived damaged (or the device froze a segment at another size of T than the host knows):
      // nothing of the wave has been used yet -- pack again and look again; three failures end the call
      ++n_hist_retries;
      if (debug) fprintf(stderr, "[flow] packed history row %d failed its header check (%s; device m %.0f, host m %d), attempt %d\n", hist_bad_row,
                         hist_bad_sum ? "checksum" : "size of T", hist_bad_m_dev, hist_bad_m_host, hist_tries + 1);
      if (guard_log) {
        if (FILE* f = fopen(guard_log, "a")) {
          fprintf(f, "HISTROW wave_rows %zu row %d mp %d %s device_m %.0f host_m %d attempt %d J %d g0 %d n %d\n", nA, hist_bad_row, w_mp, hist_bad_sum ? "checksum" : "size", hist_bad_m_dev,
                  hist_bad_m_host, hist_tries + 1, J, wA[hist_bad_row].g0, wA[hist_bad_row].n);
          const HistRows H((size_t)w_mp);
          const double* row = H.row(hist_rows(), (size_t)hist_bad_row);
          fprintf(f, "head");
          for (int j = 0; j < 20 && j < (int)H.pitch(); ++j) fprintf(f, " %a", row[j]);
          fprintf(f, "\n");
          fclose(f);
        }
      }
      if (++hist_tries >= 3) {
        ai_set_error("internal: a packed history row failed its header check three times (%s; device m %.0f, host m %d)", hist_bad_sum ? "checksum" : "size of T", hist_bad_m_dev,
                     hist_bad_m_host);
        return AI_ERR_INTERNAL;
      }
      const FlowLz L = lz();
      hipLaunchKernelGGL(fk_pack_hist, dim3((unsigned)nA), dim3(AI_BLOCK), 0, sw, (const SegRec*)wrecP.p, L, (const double*)s_theta.p, (const double*)s_resid.p, w_mp,
                         hist_rows());
      AI_KERNEL_CHECK();
      AI_HIP(hipEventRecord(wave_ev(), sw));
      wstate = W_S1;
      return AI_OK;
    }
    hist_tries = 0;
    if (nA && ctx->helper.failed.load()) {
      ai_set_error("the helper thread's Ritz job failed (out of host memory?)");
      return AI_ERR_OOM;
    }
    if (nA) {
      if (ritz_err) {
        ai_set_error("internal: frozen segment with %d rows of T", ritz_err);
        return AI_ERR_INTERNAL;
      }
      n_harvested += (long long)nA;
      AI_HIP(hipMemcpyAsync(coef_d.p, coef_host(), C.bytes(), hipMemcpyHostToDevice, sw));
    }
    if (nA) {
      hipLaunchKernelGGL(fk_ritz, dim3(w_ncA), dim3(AI_BLOCK), 0, sw, (const Task*)coarseP.p, (const SegRec*)wrecP.p, C.m(cd), C.coef(cd), w_mp, C.cu(cd),
                         (const double*)u1.p, (double* const*)d_slabtab.p, (size_t)W, ev.p, warm ? C.coef2(cd) : (const double*)nullptr,
                         warm ? C.cu2(cd) : (const double*)nullptr, warm ? ev2.p : (double*)nullptr);
      AI_KERNEL_CHECK();
      // the true residual of every Ritz pair, into pinned memory behind the sweep results (r_true[nA])
      hipLaunchKernelGGL(fk_resid, dim3(w_nfA), dim3(AI_BLOCK), 0, sw, (const Task*)fineP.p, G, (const double*)wm.p, (const double*)sinv2.p,
                         (const double*)ev.p, C.theta(cd), presid.p);
      AI_KERNEL_CHECK();
      hipLaunchKernelGGL(fk_resid_final, dim3((unsigned)nA), dim3(AI_BLOCK), 0, sw, (const SegRec*)wrecP.p, (const double2*)presid.p, R.rtrue(rw));
      AI_KERNEL_CHECK();
      hipLaunchKernelGGL(fk_minmax, dim3(w_ncA), dim3(AI_BLOCK), 0, sw, (const Task*)coarseP.p, G, (const double*)ev.p, pmm.p);
      AI_KERNEL_CHECK();
      hipLaunchKernelGGL(fk_minmax_final, dim3(((unsigned)nA + 63) / 64), dim3(64), 0, sw, (const SegRec*)wrecP.p, (const MinMaxPart*)pmm.p, (int)nA,
                         w_scale.p, w_nosplit.p, w_thr.p);
      AI_KERNEL_CHECK();
      hipLaunchKernelGGL(fk_bin, dim3(w_ncA), dim3(AI_BLOCK), 0, sw, (const Task*)coarseP.p, (const int32_t*)w_nosplit.p, (const double*)w_scale.p,
                         (const double*)w_thr.p, (const double*)ev.p, bin.p);
      AI_KERNEL_CHECK();
      hipLaunchKernelGGL(fk_sweep, dim3(w_nfA), dim3(AI_BLOCK), 0, sw, (const Task*)fineP.p, (const int32_t*)w_nosplit.p, G, (const double*)deg.p,
                         (const uint8_t*)bin.p, psweep.p);
      AI_KERNEL_CHECK();
      hipLaunchKernelGGL(fk_sweep_final, dim3((unsigned)nA), dim3(AI_BLOCK), 0, sw, (const SegRec*)wrecP.p, (const int32_t*)w_nosplit.p,
                         (const double*)psweep.p, T, R.kstar(rw), R.split(rw), R.ntrue(rw), R.mcut(rw), dump_costs());
      AI_KERNEL_CHECK();
    }
    if (!wM.empty()) {
      w_ncomp_all = *res_comp_total(pin_res());
      const int len = w_hiM - w_loM;
      if (w_ncomp_all < 2 || w_ncomp_all > len) {
        ai_set_error("internal: %d components in the disconnected segments of a wave with %d rows", w_ncomp_all, len);
        return AI_ERR_INTERNAL;
      }
      // the component table goes straight into pinned memory (the histories' area: the helper thread has read them by now)
      const CompTable CT((size_t)w_ncomp_all);
      w_tab_pinned = CT.fits_pinned();
      int32_t* d_troot;
      int32_t* d_tsize;
      if (w_tab_pinned) {
        d_troot = CT.troot(pin_hist());
        d_tsize = CT.tsize(pin_hist());
      } else {
        AI_TRY(troot.ensure((size_t)w_ncomp_all));
        AI_TRY(tsize.ensure((size_t)w_ncomp_all));
        d_troot = troot.p;
        d_tsize = tsize.p;
      }
      AI_TRY(ccont_d.ensure((size_t)w_ncomp_all));
      if (warm) {   // the disconnected segments' inherited warm vector, staged where the partition permutes from
        hipLaunchKernelGGL(fk_copy_rows, dim3(w_ncM), dim3(AI_BLOCK), 0, sw, (const Task*)(coarseP.p + w_coffM), (const double*)warmv.p, ev2.p);
        AI_KERNEL_CHECK();
      }
      hipLaunchKernelGGL(fk_comp_table, dim3(w_ncM), dim3(AI_BLOCK), 0, sw, (const Task*)(coarseP.p + w_coffM), (const int32_t*)parent.p,
                         (const int32_t*)ord.p, (const int32_t*)rcnt.p, d_troot, d_tsize);
      AI_KERNEL_CHECK();
      if (!w_tab_pinned) {
        h_troot.resize(w_ncomp_all);
        h_tsize.resize(w_ncomp_all);
        AI_HIP(hipMemcpyAsync(h_troot.data(), troot.p, (size_t)w_ncomp_all * sizeof(int32_t), hipMemcpyDeviceToHost, sw));
        AI_HIP(hipMemcpyAsync(h_tsize.data(), tsize.p, (size_t)w_ncomp_all * sizeof(int32_t), hipMemcpyDeviceToHost, sw));
      }
    }
    AI_HIP(hipEventRecord(wave_ev(), sw));
    wstate = W_S2;
    return AI_OK;
  }

  // stage 3: children of every parent; partition + rebuild of the parents that split; degrees / components of the children
  // (diagnosis, AI_FLOW_GUARD_LOG) everything the host knew of harvested segment i of this wave, bit for bit (%a)
  void guard_dump(const char* tag, size_t i, size_t nA, const FSeg& sg, double resid, double rtrue) {
    FILE* f = fopen(guard_log, "a");
    if (!f) return;
    const HistRows H((size_t)w_mp);
    const CoefTable C(nA, (size_t)w_mp, false);   // coef_copy holds the first vector's part
    const double* row = H.row(hist_copy.data(), i);
    const double* c = C.coef(coef_copy.data(), i);
    fprintf(f, "%s g0 %d n %d m %d restarts %d slot %d chunk %d par %d J %d wave_mp %d dev_theta %a dev_resid %a host_theta %a cu %a est %a true %a\n", tag, sg.g0, sg.n, sg.m,
            sg.restarts, sg.slot, sg.chunk, sg.par, J, w_mp, H.theta(row), H.resid(row), C.theta(coef_copy.data())[i], C.cu(coef_copy.data())[i], resid, rtrue);
    const char* names[4] = {"a", "b", "g", "c"};
    const double* vals[4] = {H.a(row), H.b(row), H.g(row), c};
    for (int k = 0; k < 4; ++k) {
      const double* v = vals[k];
      fprintf(f, "%s", names[k]);
      for (int j = 0; j < sg.m && j < w_mp; ++j) fprintf(f, " %a", v[j]);
      fprintf(f, "\n");
    }
#ifdef AI_TRACE_HIST
    if (sg.slot >= 0) {
      std::vector<int4> hi_(64);
      std::vector<double2> hd_(64);
      int4 ci_;
      double cd_[8];
      (void)hipMemcpy(hi_.data(), sig_i.p + (size_t)sg.slot * 64, 64 * sizeof(int4), hipMemcpyDeviceToHost);
      (void)hipMemcpy(hd_.data(), sig_d.p + (size_t)sg.slot * 64, 64 * sizeof(double2), hipMemcpyDeviceToHost);
      (void)hipMemcpy(&ci_, chk_i.p + sg.slot, sizeof(int4), hipMemcpyDeviceToHost);
      (void)hipMemcpy(cd_, chk_d.p + (size_t)sg.slot * 8, sizeof(cd_), hipMemcpyDeviceToHost);
      fprintf(f, "check J %d m %d prev_m %d launch %d theta %a resid %a a0 %a a1 %a alast %a bb1 %a bnew %a sumsq %a seg_t0 %d f0 %d c0 %d\n", ci_.x, ci_.y, ci_.z, ci_.w, cd_[0], cd_[1],
              cd_[2], cd_[3], cd_[4], cd_[5], cd_[6], cd_[7], sg.t0, sg.f0, sg.c0);
      for (int j = 0; j < 64 && j < sg.m; ++j)
        fprintf(f, "writer row %d J %d t0 %d pidx %d block %d a %a alpha %a\n", j, hi_[j].x, hi_[j].y, hi_[j].z, hi_[j].w, hd_[j].x, hd_[j].y);
    }
#endif
    fclose(f);
  }
#ifdef AI_TEST_HOOKS
  // (test-only build, AI_FLOW_DUMP) one record per segment of the wave, appended to the file before stage 3 permutes any row: the stage-2
  // event has completed, fk_partition has not run.  Fixed little-endian layout (tests/flow_dump.py reads it):
  //   int64  kind ('L' = 76: harvested Lanczos segment, 'C' = 67: split into its connected components), chunk, n, m, restarts, nosplit,
  //          kstar, split, ntrue
  //   double theta (as the host used it), resid (estimate), true resid (fk_resid_final), scale, mcut, thr[10] (fk_minmax_final),
  //          costs[10] (fk_sweep_final)
  //   int32  ids[n]: chunk-local original ids of the rows in position order (G.orig[par])
  //   L: double ev[n], fk_ritz's raw vector at those positions | C: int32 comp[n], the device's component label per row
  // A C record leaves every field after n at 0.  A rejected Ritz pair that is solved again is not dumped; its repeat is.
  struct DumpHead {
    int64_t kind, chunk, n, m, restarts, nosplit, kstar, split, ntrue;
    double theta, resid, rtrue, scale, mcut, thr[AI_NUM_CUTS], costs[AI_NUM_CUTS];
  };
  int dump_seg(const FSeg& s, DumpHead& h, int wi) {
    h.chunk = s.chunk;
    h.n = s.n;
    std::vector<int32_t> ids((size_t)s.n), comp;
    std::vector<double> v;
    AI_HIP(hipMemcpyAsync(ids.data(), G.orig[s.par] + s.g0, (size_t)s.n * sizeof(int32_t), hipMemcpyDeviceToHost, sw));
    if (wi < 0) {
      h.kind = 'C';
      comp.resize((size_t)s.n);
      AI_HIP(hipMemcpyAsync(comp.data(), parent.p + s.g0, (size_t)s.n * sizeof(int32_t), hipMemcpyDeviceToHost, sw));
    } else {
      int32_t ns = 0;
      h.kind = 'L';
      h.m = s.m;
      h.restarts = s.restarts;
      v.resize((size_t)s.n);
      AI_HIP(hipMemcpyAsync(v.data(), ev.p + s.g0, (size_t)s.n * sizeof(double), hipMemcpyDeviceToHost, sw));
      AI_HIP(hipMemcpyAsync(&h.theta, CoefTable(wA.size(), (size_t)w_mp, warm != 0).theta(coef_d.p) + wi, sizeof(double), hipMemcpyDeviceToHost, sw));
      AI_HIP(hipMemcpyAsync(&h.scale, w_scale.p + wi, sizeof(double), hipMemcpyDeviceToHost, sw));
      AI_HIP(hipMemcpyAsync(&ns, w_nosplit.p + wi, sizeof(int32_t), hipMemcpyDeviceToHost, sw));
      AI_HIP(hipMemcpyAsync(h.thr, w_thr.p + (size_t)wi * AI_NUM_CUTS, sizeof h.thr, hipMemcpyDeviceToHost, sw));
      AI_HIP(hipMemcpyAsync(h.costs, w_costs.p + (size_t)wi * AI_NUM_CUTS, sizeof h.costs, hipMemcpyDeviceToHost, sw));
      h.nosplit = ns;
    }
    AI_HIP(hipStreamSynchronize(sw));
    FILE* f = fopen(dump_path, "ab");
    if (!f) {
      ai_set_error("AI_FLOW_DUMP: %s cannot be opened", dump_path);
      return AI_ERR_BAD_ARG;
    }
    bool ok = fwrite(&h, sizeof h, 1, f) == 1 && fwrite(ids.data(), sizeof(int32_t), ids.size(), f) == ids.size();
    ok = ok && (wi < 0 ? fwrite(comp.data(), sizeof(int32_t), comp.size(), f) == comp.size() : fwrite(v.data(), sizeof(double), v.size(), f) == v.size());
    ok = (fclose(f) == 0) && ok;
    if (!ok) {
      ai_set_error("AI_FLOW_DUMP: writing %s failed", dump_path);
      return AI_ERR_BAD_ARG;
    }
    return AI_OK;
  }
#endif
  int wave_s3() {
    wpin_off = 0;
    const size_t nA = wA.size();
    std::vector<FSeg> P2;          // parents that split: binary first, then by components
    std::vector<SplitSeg> ssv;
    std::vector<FSeg> cbin, ccomp;  // continuing children
    std::vector<int32_t> ccont;
    if (nA) {
      const WaveResults R(nA);
      char* const rw = res_wave(pin_res());
      const int32_t *r_split = R.split(rw), *r_ntrue = R.ntrue(rw), *r_kstar = R.kstar(rw);
      const double *r_mcut = R.mcut(rw), *r_resid = R.resid(rw), *r_true = R.rtrue(rw);
      if (trace)
        for (size_t i = 0; i < nA; ++i)
          fprintf(stderr, "[seg] %d %d m=%d theta=%.17g resid=%.6e true=%.6e split=%d ntrue=%d k=%d mcut=%.17g\n", wA[i].g0, wA[i].n, wA[i].m, w_theta[i],
                  r_resid[i], r_true[i], r_split[i], r_ntrue[i], r_kstar[i], r_mcut[i]);
      for (size_t i = 0; i < nA; ++i) {
        const FSeg& s = wA[i];
        // a residual above tol is a failure only if T is smaller than the segment's own dimension
        if (r_resid[i] > opt.tol && s.m < s.n - 1) ++stats.unconverged;
        stats.max_resid = std::max(stats.max_resid, r_resid[i]);
        give_back(s, wslots_to_free);   // (the slot only when the wave is over)
        --chunk_live[s.chunk];
        if (r_resid[i] <= opt.tol && r_true[i] > true_resid_limit && !(s.restarts > 0 && r_true[i] == s.prev_true)) {
          // The check froze this segment as converged, but its Ritz pair is not an eigenpair of the segment's operator: it was built
          // from bad data (round 4's soaks: once in ~70 000 chunk cuts the packed history of ANOTHER segment had been written over
          // the head of this one's row -- fk_pack_hist / fk_freeze_exhausted have the story; that cause is removed and the rows
          // carry a checksum now, this test stays behind both).  Nothing of the pair is used: the segment is solved again from
          // scratch -- same graph, same start vector, so the same bits as an undisturbed solve -- like a connected child that joins
          // the pool.  A repeat that arrives at the SAME true residual, bit for bit, is the algorithm's own answer (Lanczos without
          // reorthogonalisation on a dense blob whose top eigenvalues cluster: estimate 2e-15, true 3e-7 in
          // tests/test_gpu_parity.py's dense cases) and is accepted; one that differs again is repeated once more, then the call fails.
          if (s.restarts >= 2) {
            ai_set_error("internal: a %d-row segment failed the true-residual test three times with different residuals (estimate %.3g, true %.3g)", s.n, r_resid[i], r_true[i]);
            return AI_ERR_INTERNAL;
          }
          if (guard_log && hist_copy.size()) guard_dump("BAD", i, nA, s, r_resid[i], r_true[i]);
          if (debug) fprintf(stderr, "[flow] segment %d+%d: Ritz residual estimate %.3g but true residual %.3g: solved again\n", s.g0, s.n, r_resid[i], r_true[i]);
          ++n_restarted;
          --stats.lanczos_solves;
          child_solve_again(s, r_true[i], ccomp);   // (chunk_live is counted with the other continuing children below)
          continue;
        }
        if (guard_log && s.restarts > 0 && hist_copy.size()) guard_dump("REPEAT", i, nA, s, r_resid[i], r_true[i]);
        if (r_resid[i] <= opt.tol && r_true[i] > true_resid_limit) ++n_above_limit;  // (accepted: the repeat reproduced it bit for bit)
        max_true_resid = std::max(max_true_resid, r_true[i]);  // of the pairs that are CUT (a rejected pair is not)
#ifdef AI_TEST_HOOKS
        if (dump_path) {
          DumpHead h{};
          h.resid = r_resid[i];
          h.rtrue = r_true[i];
          h.mcut = r_mcut[i];
          h.kstar = r_kstar[i];
          h.split = r_split[i];
          h.ntrue = r_ntrue[i];
          AI_TRY(dump_seg(s, h, (int)i));
        }
#endif
        if (!r_split[i]) {
          leaf(s.g0, s.front, r_mcut[i]);
          continue;
        }
        const CutSides cs = children_of_cut(s, r_ntrue[i], r_mcut[i], n_orig[s.chunk], cbin, leaves);
        if (!cs.ok) {
          ai_set_error("internal: split of a %d-row segment produced an empty side (%d / %d)", s.n, cs.na, cs.nb);
          return AI_ERR_INTERNAL;
        }
        SplitSeg q{};
        q.g0 = s.g0;
        q.n = s.n;
        q.ntrue = cs.na;
        q.multi = 0;
        q.kstar = r_kstar[i];
        q.contA = cs.contA ? 1 : 0;
        q.contB = cs.contB ? 1 : 0;
        P2.push_back(s);
        ssv.push_back(q);
      }
    }
    const size_t nP2bin = P2.size();
    if (!wM.empty()) {
      if (w_tab_pinned) {
        const CompTable CT((size_t)w_ncomp_all);
        h_troot.assign(CT.troot(pin_hist()), CT.troot(pin_hist()) + CT.n);
        h_tsize.assign(CT.tsize(pin_hist()), CT.tsize(pin_hist()) + CT.n);
      } else {
        AI_HIP(hipStreamSynchronize(sw));  // the component table went to pageable memory
      }
      ccont.assign((size_t)w_ncomp_all, 0);
      size_t ti = 0;
      for (const FSeg& s : wM) {
#ifdef AI_TEST_HOOKS
        if (dump_path) {
          DumpHead h{};
          AI_TRY(dump_seg(s, h, -1));
        }
#endif
        const CompSplit sp = children_of_components(s, h_troot.data(), h_tsize.data(), h_troot.size(), ti, n_orig[s.chunk], ccont.data(), ccomp, leaves);
        if (sp.status == COMP_NO_TILE) {
          ai_set_error("internal: component table does not tile a %d-row segment", s.n);
          return AI_ERR_INTERNAL;
        }
        if (sp.status == COMP_SHORT) {
          ai_set_error("internal: components of a segment cover %d of %d rows", sp.covered, s.n);
          return AI_ERR_INTERNAL;
        }
        SplitSeg q{};
        q.g0 = s.g0;
        q.n = s.n;
        q.multi = 1;
        P2.push_back(s);
        ssv.push_back(q);
      }
    }
    for (const FSeg& s : wM) --chunk_live[s.chunk];
    for (const FSeg& s : cbin) ++chunk_live[s.chunk];
    for (const FSeg& s : ccomp) ++chunk_live[s.chunk];
    // chunks admitted since the last wave start here: their roots are prepared like the children of a cut
    cbin.insert(cbin.end(), new_roots.begin(), new_roots.end());
    new_roots.clear();
    wC = cbin;
    wC.insert(wC.end(), ccomp.begin(), ccomp.end());
    w_nbin = (int)cbin.size();
    AI_TRY(retire_chunks());
    if (!P2.empty()) {
      int nfP = 0, ncP = 0;
      AI_TRY(expand(P2, wrecP, fineP.p, coarseP.p, 0, nfP, ncP, Rider{ssv.data(), ss_d.p, ssv.size() * sizeof(SplitSeg)},
                    Rider{ccont.data(), ccont_d.p, ccont.size() * sizeof(int32_t)}));
      int lo = N, hi = 0;
      for (auto& s : P2) {
        lo = std::min(lo, s.g0);
        hi = std::max(hi, s.g0 + s.n);
      }
      const int len = hi - lo;
      hipLaunchKernelGGL(fk_split_flags, dim3(ncP), dim3(AI_BLOCK), 0, sw, (const Task*)coarseP.p, (const SplitSeg*)ss_d.p, (const uint8_t*)bin.p,
                         flag.p);
      AI_KERNEL_CHECK();
      if (nP2bin) {
        AI_TRY(ai_exclusive_scan_i32(sw, flag.p + lo, fscan.p + lo, len, scantmp.p));
        hipLaunchKernelGGL(fk_partition, dim3(ncP), dim3(AI_BLOCK), 0, sw, (const Task*)coarseP.p, (const SplitSeg*)ss_d.p, (const int32_t*)flag.p,
                           (const int32_t*)fscan.p, G, final_order.p, map.p, newcnt.p, (const double*)(warm ? ev2.p : nullptr), warm ? warmv.p : (double*)nullptr);
        AI_KERNEL_CHECK();
      }
      if (!wM.empty()) {
        // stable sort of the range's rows by root (rows outside the disconnected segments carry their own position)
        const int lenM = w_hiM - w_loM;
        int bits = 1;
        while ((1ll << bits) < (long long)N) ++bits;
        size_t tmp_bytes = 0;
        AI_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, (const uint32_t*)(key.p + w_loM), (uint32_t*)(key_out.p + w_loM),
                                         (const int32_t*)(val.p + w_loM), sorted_rows.p + w_loM, (size_t)lenM, 0, bits, sw));
        AI_TRY(sorttmp.ensure(tmp_bytes));
        AI_HIP(rocprim::radix_sort_pairs((void*)sorttmp.p, tmp_bytes, (const uint32_t*)(key.p + w_loM), (uint32_t*)(key_out.p + w_loM),
                                         (const int32_t*)(val.p + w_loM), sorted_rows.p + w_loM, (size_t)lenM, 0, bits, sw));
        hipLaunchKernelGGL(fk_partition_multi, dim3(ncP), dim3(AI_BLOCK), 0, sw, (const Task*)coarseP.p, (const SplitSeg*)ss_d.p,
                           (const int32_t*)sorted_rows.p, (const int32_t*)parent.p, (const int32_t*)ord.p, (const int32_t*)ccont_d.p, G,
                           final_order.p, map.p, newcnt.p, (const double*)(warm ? ev2.p : nullptr), warm ? warmv.p : (double*)nullptr);
        AI_KERNEL_CHECK();
      }
      if (!wC.empty()) {
        hipLaunchKernelGGL(fk_rebuild_count, dim3(nfP), dim3(AI_BLOCK), 0, sw, (const Task*)fineP.p, G, (const int32_t*)flag.p, (const int32_t*)map.p,
                           newcnt.p);
        AI_KERNEL_CHECK();
        AI_TRY(ai_exclusive_scan_i32(sw, newcnt.p + lo, nscan.p + lo, len, scantmp.p));
        hipLaunchKernelGGL(fk_child_rows, dim3(ncP), dim3(AI_BLOCK), 0, sw, (const Task*)coarseP.p, (const SplitSeg*)ss_d.p, G, (const int32_t*)newcnt.p,
                           (const int32_t*)nscan.p);
        AI_KERNEL_CHECK();
        hipLaunchKernelGGL(fk_rebuild_fill, dim3(nfP), dim3(AI_BLOCK), 0, sw, (const Task*)fineP.p, G, (const int32_t*)flag.p, (const int32_t*)map.p);
        AI_KERNEL_CHECK();
      }
    }
    AI_TRY(children_prep());
    return AI_OK;
  }

  // Stage 3, second half: the children wC (children of cuts first: their connectivity is not known yet) get degrees and
  // component counts, and -- speculatively, gated on the device by "exactly one component" -- scaling, staged-gather
  // encoding and the start vector, so that a connected child is ready to join when the host learns its count.
  int children_prep() {
    if (!wC.empty()) {
      // slots of earlier waves' parents may still be named by checks launched before those parents left the lists
      while (!checks.empty() && checks.front().lver < w_start_ver) AI_TRY(reap_check(true));
      // Admission is slot-aware: a child takes a Lanczos slot, stable task indices, a record of the pool table and a record of
      // this wave's tables.  Whatever does not fit waits as a root of a later wave (new_roots: prepared like the child of a cut,
      // i.e. its connectivity is looked at again) instead of failing the call -- hundreds of small chunks in one call, or chunks
      // whose num_points_orig is far below their size (the 1 % rule then allows thousands of live segments), get through with the
      // capacities a call was set up with.
      const int pool_cap = std::min(SMAX, (int)(POOL_SLOT_BYTES / sizeof(SegRec)));
      const int room = std::max(0, std::min(pool_cap - (int)pool.size(), WCAP));
      size_t take = 0;
      for (; take < wC.size(); ++take) {
        FSeg& s = wC[take];
        if (free_slots.empty() || (int)take >= room) break;
        s.f0 = fa.alloc(fk_nf(s.n));
        s.c0 = (s.f0 >= 0) ? ca.alloc(fk_nc(s.n)) : -1;
        if (s.f0 < 0 || s.c0 < 0) {
          give_back(s, free_slots);   // (the fine range, if it got one: it has no slot yet; detached with the others below)
          break;
        }
        s.aux = (int)take;
        s.slot = free_slots.back();
        free_slots.pop_back();
        ((volatile int32_t*)pin_status())[s.slot] = 0;
        s.cap = std::max(1, std::min(opt.max_iter, s.n - 1));
        s.frozen = false;
        s.m = 0;
      }
      if (take < wC.size()) {
        stats_deferred += (long long)(wC.size() - take);
        for (size_t i = take; i < wC.size(); ++i) {
          FSeg s = wC[i];
          s.binary_child = true;
          s.detach();
          new_roots.push_back(s);
        }
        wC.resize(take);
        w_nbin = std::min(w_nbin, (int)take);
      }
    }
    bool any_pca = false;
    for (FSeg& s : wC) {
      s.pca = (any_xyz && s.warm_n == 0 && h_xyz[s.chunk]) ? s.chunk + 1 : 0;
      any_pca |= s.pca != 0;
    }
    if (!wC.empty()) {
      int nfC = 0, ncC = 0;
      AI_TRY(expand(wC, wrecC, fineC.p, coarseC.p, 1, nfC, ncC));
      hipLaunchKernelGGL(fk_degree, dim3(nfC), dim3(AI_BLOCK), 0, sw, (const Task*)fineC.p, G, deg.p, sinv.p, pvol.p);
      AI_KERNEL_CHECK();
      hipLaunchKernelGGL(fk_seg_sum, dim3((unsigned)wC.size()), dim3(AI_BLOCK), 0, sw, (const SegRec*)wrecC.p, (const double*)pvol.p, w_vol.p);
      AI_KERNEL_CHECK();
      if (w_nbin > 0) {
        int nfb = 0, ncb = 0;
        for (int i = 0; i < w_nbin; ++i) {
          nfb += fk_nf(wC[i].n);
          ncb += fk_nc(wC[i].n);
        }
        hipLaunchKernelGGL(fk_cc_init, dim3(nfb), dim3(AI_BLOCK), 0, sw, (const Task*)fineC.p, G, parent.p, w_ncomp.p);
        AI_KERNEL_CHECK();
        hipLaunchKernelGGL(fk_cc_sample, dim3(nfb), dim3(AI_BLOCK), 0, sw, (const Task*)fineC.p, G, parent.p);
        AI_KERNEL_CHECK();
        hipLaunchKernelGGL(fk_cc_compress, dim3(ncb), dim3(AI_BLOCK), 0, sw, (const Task*)coarseC.p, parent.p);
        AI_KERNEL_CHECK();
        hipLaunchKernelGGL(fk_cc_hook, dim3(nfb), dim3(AI_BLOCK), 0, sw, (const Task*)fineC.p, (const SegRec*)wrecC.p, G, parent.p);
        AI_KERNEL_CHECK();
        hipLaunchKernelGGL(fk_cc_compress, dim3(ncb), dim3(AI_BLOCK), 0, sw, (const Task*)coarseC.p, parent.p);
        AI_KERNEL_CHECK();
        hipLaunchKernelGGL(fk_cc_count, dim3(ncb), dim3(AI_BLOCK), 0, sw, (const Task*)coarseC.p, (const int32_t*)parent.p, w_ncomp.p);
        AI_KERNEL_CHECK();
      }
      const FlowLz L = lz();
      const int32_t* gate = w_ncomp.p;
      hipLaunchKernelGGL(fk_scale, dim3(nfC), dim3(AI_BLOCK), 0, sw, (const Task*)fineC.p, (const SegRec*)wrecC.p, G, (const double*)deg.p,
                         (const double*)sinv.p, (const double*)w_vol.p, wm.p, sinv2.p, u1.p, gate, w_nbin);
      AI_KERNEL_CHECK();
      hipLaunchKernelGGL(fk_encode, dim3(nfC), dim3(AI_BLOCK), 0, sw, (const Task*)fineC.p, G, ucol.p, lidx.p, enc.p, gate, w_nbin);
      AI_KERNEL_CHECK();
      hipLaunchKernelGGL(fk_reset_slots, dim3(((unsigned)wC.size() + AI_BLOCK - 1) / AI_BLOCK), dim3(AI_BLOCK), 0, sw, (const SegRec*)wrecC.p,
                         (int)wC.size(), L, s_lastm.p, s_nextm.p, opt.check_every, s_theta.p, s_resid.p, gate, w_nbin, res_child_comps(pin_res()));
      AI_KERNEL_CHECK();
      if (any_pca) {  // ancestor-less segments: warm[] = u1 * principal-axis coordinate, SegRec.pad0 = their own row count
        hipLaunchKernelGGL(fk_pca_moments, dim3(ncC), dim3(AI_BLOCK), 0, sw, (const Task*)coarseC.p, (const SegRec*)wrecC.p, G,
                           (const double* const*)d_xyz.p, pca_part.p, (size_t)CCAP, gate, w_nbin);
        AI_KERNEL_CHECK();
        hipLaunchKernelGGL(fk_pca_axis, dim3((unsigned)wC.size()), dim3(AI_BLOCK), 0, sw, wrecC.p, G, (const double* const*)d_xyz.p,
                           (const double*)pca_part.p, (size_t)CCAP, pca_axis.p, gate, w_nbin);
        AI_KERNEL_CHECK();
        hipLaunchKernelGGL(fk_pca_fill, dim3(ncC), dim3(AI_BLOCK), 0, sw, (const Task*)coarseC.p, (const SegRec*)wrecC.p, G,
                           (const double* const*)d_xyz.p, (const double*)pca_axis.p, (const double*)u1.p, warmv.p, gate, w_nbin);
        AI_KERNEL_CHECK();
      }
      hipLaunchKernelGGL(fk_lz_init, dim3(ncC), dim3(AI_BLOCK), 0, sw, (const Task*)coarseC.p, (const SegRec*)wrecC.p, G, (const double*)u1.p, slabs[0],
                         pB0.p, cactive.p, gate, w_nbin, warm ? (const double*)warmv.p : (const double*)nullptr, pB1.p);
      AI_KERNEL_CHECK();
      if (warm) {  // starts that carry a warm vector: u1 taken out where the start is all but parallel to it; their partials pB1 -> pB0
        hipLaunchKernelGGL(fk_lz_project, dim3(ncC), dim3(AI_BLOCK), 0, sw, (const Task*)coarseC.p, (const SegRec*)wrecC.p, (const double*)u1.p,
                           slabs[0], (const double2*)pB1.p, pB0.p, gate, w_nbin);
        AI_KERNEL_CHECK();
      }
      hipLaunchKernelGGL(fk_set_flags, dim3((nfC + AI_BLOCK - 1) / AI_BLOCK), dim3(AI_BLOCK), 0, sw, (const Task*)fineC.p, nfC, factive.p, gate, w_nbin);
      AI_KERNEL_CHECK();
    }
    AI_HIP(hipEventRecord(wave_ev(), sw));
    wstate = W_S3;
    return AI_OK;
  }

  // the wave is over: connected children start iterating at the step the host has reached; children of a cut that fell
  // apart give their slot back and wait for the next wave, which splits them into their components
  int wave_finish() {
    const int32_t* r_ncomp = res_child_comps(pin_res());
    int joined = 0;
    for (size_t i = 0; i < wC.size(); ++i) {
      FSeg s = wC[i];
      if ((int)i < w_nbin && r_ncomp[i] != 1) {
        if (r_ncomp[i] < 1) {
          ai_set_error("internal: %d components counted in a %d-row child", r_ncomp[i], s.n);
          return AI_ERR_INTERNAL;
        }
        give_back(s, free_slots);
        s.detach();
        // the cut between whole components costs exactly 0, and the reference splits iff mcut < T (normalized_cut.py:56)
        if (T > 0.0) {
          pend_multi.push_back(s);
        } else {
          leaf(s.g0, s.front, NAN);
          --chunk_live[s.chunk];
        }
        continue;
      }
      s.t0 = J;  // the sizes of T at which a segment is judged do not depend on when it starts
      pool.push_back(s);
      ++joined;
    }
    if (joined) need_relist = relist_urgent = true;
    AI_TRY(retire_chunks());
    for (int sl : wslots_to_free) free_slots.push_back(sl);
    wslots_to_free.clear();
    wC.clear();
    wstate = W_IDLE;
    return AI_OK;
  }

  int advance_wave() {
    t_progress = now_ms();
    if (debug && !trace)
      fprintf(stderr, "[flow] t=%.2f J=%d nft=%d wave stage %d done: A=%zu M=%zu C=%zu pool=%zu pend=%zu/%zu leaves=%zu\n", now_ms() - t_call, J, nft, (int)wstate, wA.size(), wM.size(),
              wC.size(), pool.size(), pend_solved.size(), pend_multi.size(), leaves.size());
    const double t_a0 = now_ms();
    int rc = AI_OK;
    switch (wstate) {
      case W_S1: rc = wave_s2_begin(); th_start += now_ms() - t_a0; break;
      case W_S1H: rc = wave_s2(); th_start += now_ms() - t_a0; break;
      case W_S2: rc = wave_s3(); th_s3 += now_ms() - t_a0; break;
      case W_S3: rc = wave_finish(); th_finish += now_ms() - t_a0; break;
      default: break;
    }
    return rc;
  }

  // ------------------------------------------------------------------------------------------------- the run
  int run(double split_lim) {
    // roots: every chunk that may be split at all (normalized_cut.py:39-40), admitted as far as the slab window allows
    for (int c = 0; c < nchunks; ++c) {
      const int nc = (int)(off[c + 1] - off[c]);
      if (eligible(nc, n_orig[c], split_lim))
        waiting.push_back(c);
      else if (nc > 0)
        leaf((int)off[c], -INFINITY, NAN);
    }
    admit();
    wC = new_roots;
    new_roots.clear();
    w_nbin = (int)wC.size();
    w_start_ver = ver;
    if (!wC.empty()) AI_TRY(children_prep());
    t_progress = now_ms();
    for (;;) {
      if (now_ms() - t_progress > 30000.0) {
        ai_set_error("internal: the frontier made no progress for 30 s (J = %d, pool %zu, wave stage %d, pending %zu / %zu, checks %zu)", J, pool.size(),
                     (int)wstate, pend_solved.size(), pend_multi.size(), checks.size());
        return AI_ERR_INTERNAL;
      }
      {
        // progress = the device's step counter or the host's own moved (a wave stage that completes refreshes t_progress as well)
        const int pg = *progress;
        if (pg != wd_pg || J != wd_J) {
          wd_pg = pg;
          wd_J = J;
          t_progress = now_ms();
        }
        if ((++wd_iter & 1023) == 0) {  // a fault on the stepping stream shows here, not only when a wave or a check is reaped
          const hipError_t q = hipStreamQuery(sm);
          if (q != hipSuccess && q != hipErrorNotReady) AI_HIP(q);
        }
      }
      if (nft > 0) {
        // stay a few steps ahead of the device, no more: children join at the step the host has reached, and a
        // host that waits inside the runtime cannot drive the wave
        // a large pool's steps are long and its waves keep the host busy for milliseconds (Ritz coefficients of hundreds of
        // segments): queue deeper there -- children that join 50 steps late cost nothing when thousands of tasks are stepping
        const int ahead = (nft > 2000) ? 16 : (nft > 300) ? AHEAD : AHEAD_SMALL;
        if (J - *progress >= ahead) {
          // far enough ahead: a short pause instead of hammering the pinned counter and the event queries (~0.3 us)
          for (int k = 0; k < 32; ++k) __builtin_ia32_pause();
        } else {
          if (J > 0 && *progress >= J) ++n_starved;  // the device had nothing of this pool queued
          AI_TRY(step());
          // the check kernel decides per segment whether the size of T it wants judged has been reached; a launch costs an
          // event on this stream and a few blocks on the side stream: every 4th step
          const bool chk = (J - last_check_J) >= 4;
          if (chk) AI_TRY(launch_check());
        }
      }
      scan_status();
      if (checks.size() > 8) AI_TRY(reap_check(false));
      // (letting a relist that only drops frozen segments wait up to 8 steps was measured in round 4: 183 instead of 420 relists per
      // 12-chunk call, 2.7 instead of 10 ms of this thread, and the call 4 ms SLOWER: the frozen segments' blocks are still dispatched)
      if (need_relist) {
        const double t_l0 = now_ms();
        AI_TRY(relist());
        th_relist += now_ms() - t_l0;
        ++n_relist;
      }
      if (wstate == W_S1H) {
        if (ctx->helper.try_done()) {
          AI_TRY(advance_wave());
          if (need_relist) AI_TRY(relist());
        }
      } else if (wstate != W_IDLE) {
        hipError_t q = hipEventQuery(wave_ev());
        if (q == hipSuccess) {
          AI_TRY(advance_wave());
          if (need_relist) AI_TRY(relist());
        } else if (q != hipErrorNotReady) {
          AI_HIP(q);
        }
      }
      // (gathering what freezes over 16-48 steps of a large pool into fewer, larger waves was measured: no effect beyond the
      // run-to-run spread of the two-thread bench, 114-120 chunks/s either way)
      // (roots that wait for a slot start a wave of their own only when there is one)
      const bool roots_can_start = !new_roots.empty() && !free_slots.empty() && (int)pool.size() < std::min(SMAX, (int)(POOL_SLOT_BYTES / sizeof(SegRec)));
      if (wstate == W_IDLE && (!pend_solved.empty() || !pend_multi.empty() || roots_can_start)) {
        // a segment that is harvested must have left the pool lists: its stable task indices go to its children
        if (need_relist) {
          const double t_l0 = now_ms();
          AI_TRY(relist());
          th_relist += now_ms() - t_l0;
          ++n_relist;
        }
        AI_TRY(start_wave());
      }
      if (nft == 0) {
        // nothing to step: wait for whatever is in flight
        if (!checks.empty()) {
          AI_TRY(reap_check(true));
        } else if (wstate == W_S1H) {
          ctx->helper.wait();
        } else if (wstate != W_IDLE) {
          AI_HIP(hipEventSynchronize(wave_ev()));
        } else if (pend_solved.empty() && pend_multi.empty() && pool.empty() && new_roots.empty()) {
          if (!waiting.empty()) {
            ai_set_error("internal: %zu chunks were never admitted", waiting.size());
            return AI_ERR_INTERNAL;
          }
          break;
        } else if (!pool.empty()) {
          need_relist = relist_urgent = true;  // only frozen segments are left in the lists
        }
      }
    }
    AI_HIP(hipStreamSynchronize(sm));
    AI_HIP(hipStreamSynchronize(ss));
    AI_HIP(hipStreamSynchronize(sw));
    stats.lanczos_steps = J;
    stats.ms_eigen = t_pool;
    return AI_OK;
  }
};

// The recursion over one graph that holds `nchunks` independent chunks back to back (rows off[c] .. off[c+1]);
// csr->orig holds chunk-LOCAL point ids; csr's arrays belong to the call (the recursion's even depths live in them).
static int ncut_flow(ai_ctx* ctx, const ai_csr* csr, int nchunks, const int64_t* off, const int64_t* n_orig, double T, double split_lim,
                     const ai_ncut_opts* opts, int32_t* const* labels_out, int32_t* n_groups, ai_ncut_stats* stats_out, double t0,
                     double* const* cut_height = nullptr, double* const* leaf_cost = nullptr) {
  Flow F(ctx);
  struct Drain {  // whatever way the call ends, nothing of it may still be running when its workspace is rewound
    Flow& f;
    ~Drain() {
      f.ctx->helper.wait();  // (a helper job reads and writes this Flow)
      (void)hipStreamSynchronize(f.sm);
      (void)hipStreamSynchronize(f.ss);
      if (f.sw) (void)hipStreamSynchronize(f.sw);
    }
  } drain{F};
  if (opts) {
    if (opts->tol > 0.0) F.opt.tol = opts->tol;
    if (opts->max_iter > 0) F.opt.max_iter = std::min(opts->max_iter, 4000);  // T_m must fit the check kernel's 64 KB of LDS
    if (opts->check_every > 0) F.opt.check_every = opts->check_every;
    F.clock_spmv = (opts->reserved & 3) != 0;
    F.window_rows = opts->window_rows;
  }
  F.true_resid_limit = std::max(1e-6, 100.0 * F.opt.tol);
#ifdef AI_TEST_HOOKS
  if (const char* e = getenv("AI_FLOW_TRUE_LIMIT")) F.true_resid_limit = atof(e);  // a limit below every residual sends EVERY segment back once (its repeat must reproduce the residual bit for bit)
#endif
  const int n = (int)csr->n;
  const double tp0 = now_ms();
  AI_TRY(F.setup(csr, nchunks, off, n_orig, T));
  const double tp1 = now_ms();
  AI_TRY(F.run(split_lim));
  const double tp2 = now_ms();
  hipStream_t st = ctx->stream;
  std::vector<int32_t> order((size_t)n);
  AI_HIP(hipMemcpyAsync(order.data(), F.final_order.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  unsigned long long hw[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // rows x steps, entries x steps, check time-outs, Sturm rounds, judgments
  AI_HIP(hipMemcpyAsync(hw, F.work.p, sizeof(hw), hipMemcpyDeviceToHost, st));
  std::vector<unsigned long long> hts;
  if (F.clock_spmv) {
    hts.resize((size_t)2 * std::min(F.J, (int)Flow::TS_CAP));
    if (!hts.empty()) AI_HIP(hipMemcpyAsync(hts.data(), F.tstamps.p, hts.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  }
  AI_HIP(hipStreamSynchronize(st));
  for (size_t j = 0; j + 1 < hts.size(); j += 2)
    if (hts[j + 1] > hts[j]) F.stats.ms_spmv += (double)(hts[j + 1] - hts[j]) / F.clock_khz;
  F.stats.spmv_rows = (int64_t)hw[0];
  F.stats.spmv_nnz = (int64_t)hw[1];
  std::sort(F.leaves.begin(), F.leaves.end(), [](const FLeaf& a, const FLeaf& b) { return a.g0 < b.g0; });
  // groups of chunk c = the leaf ranges inside [off[c], off[c+1]), numbered from 0 in emission order; the cut tree of the chunk
  // (ai_ncut_tree) is what the leaves recorded, in the same order: cut_height[c][g], leaf_cost[c][g]
  size_t li = 0;
  int64_t total_groups = 0;
  for (int c = 0; c < nchunks; ++c) {
    int g = -1;
    const int32_t nloc = (int32_t)(off[c + 1] - off[c]);
    for (int64_t p = off[c]; p < off[c + 1]; ++p) {
      while (li < F.leaves.size() && F.leaves[li].g0 == p) {
        ++g;
        if (cut_height && cut_height[c]) cut_height[c][g] = F.leaves[li].front;
        if (leaf_cost && leaf_cost[c]) leaf_cost[c][g] = F.leaves[li].cost;
        ++li;
      }
      if (g < 0 || order[p] < 0 || order[p] >= nloc) {
        ai_set_error("internal: final ordering is not a permutation (chunk %d, position %lld)", c, (long long)p);
        return AI_ERR_INTERNAL;
      }
      labels_out[c][order[p]] = g;
    }
    n_groups[c] = g + 1;
    total_groups += g + 1;
  }
  F.stats.n_groups = total_groups;
  F.stats.restarted_solves = F.n_restarted;
  F.stats.hist_retries = F.n_hist_retries;
  F.stats.max_true_resid = F.max_true_resid;
  F.stats.true_resid_limit = F.true_resid_limit;
  F.stats.accepted_above_limit = F.n_above_limit;
  F.stats.check_timeouts = (int64_t)hw[2];
  F.stats.spmv_blocks = F.n_stamped_blocks;
  F.stats.spmv_blocks_idle = (int64_t)hw[5];
  F.stats.ms_total = now_ms() - t0;
  if (getenv("AI_NCUT_PHASES"))  // where a call's wall time goes: merge of the chunks' graphs | set-up | the frontier | labels
    fprintf(stderr, "[phases] chunks %d rows %d: merge %.2f ms, set-up %.2f, frontier %.2f (stepping %.2f), labels %.2f, total %.2f; steps %d waves %lld\n", nchunks, n,
            tp0 - t0, tp1 - tp0, tp2 - tp1, F.t_pool, now_ms() - tp2, F.stats.ms_total, F.J, (long long)F.stats.levels);
  if (getenv("AI_NCUT_PHASES"))
    fprintf(stderr, "[phases] host ms: wave stage 2 %.2f (Ritz coefficients of %lld segments %.2f), stage 3 %.2f, finish %.2f, %lld relists %.2f; steps launched on a drained queue %lld; children that waited for a slot %lld; largest true residual %.3g, solves repeated %lld, history rows asked for again %lld; convergence judgments %llu, Sturm rounds per judgment %.2f, check time-outs %llu\n",
            F.th_start, F.n_ritz_segs, F.th_ritz, F.th_s3, F.th_finish, F.n_relist, F.th_relist, F.n_starved, F.stats_deferred, F.max_true_resid, F.n_restarted, F.n_hist_retries, hw[4], hw[4] ? (double)hw[3] / (double)hw[4] : 0.0, hw[2]);
  if (stats_out) *stats_out = F.stats;
  if (F.stats.unconverged > 0) {
    // the reference's eigsh raises ArpackNoConvergence (normalized_cut.py:49); labels and stats are filled all the same
    ai_set_error("ai_ncut: %lld Lanczos solve(s) reached max_iter = %d before the Ritz residual fell to %.3g (largest %.3g)",
                 (long long)F.stats.unconverged, F.opt.max_iter, F.opt.tol, F.stats.max_resid);
    return AI_ERR_NO_CONVERGENCE;
  }
  return AI_OK;
}
