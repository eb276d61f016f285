/*
 * autoinst_hip.h -- C ABI of libautoinst_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE hot path of artonson/autoinst: the per-chunk pairwise
 * affinity build and the recursive normalized cut.  The
 * reference is pure Python (no FFI of its own); each entry point cites the reference
 * lines it replaces (paths relative to the reference root).  Plain pointers and
 * sizes only -- no torch / numpy types.  All matrices are float64, like the
 * reference's arithmetic.
 *
 * Threading: an ai_ctx owns its HIP streams (one for the affinity build and the Lanczos steps, one for the convergence
 * checks, one for the harvest waves of the normalized cut) and one helper thread; it is not thread-safe, the library is
 * re-entrant across contexts.  One process per GPU for multi-GPU use.
 * Ownership: the caller owns every array it passes; nothing is retained after a
 * call returns.  Handles returned here are freed with the matching *_free/destroy.
 * Errors: every function returns AI_OK (0) or a negative ai_status; the text of the
 * last error of the calling thread is ai_last_error().
 */
#ifndef AUTOINST_HIP_H
#define AUTOINST_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ai_ctx ai_ctx;
typedef struct ai_csr ai_csr; /* device-resident symmetric affinity graph */

/*
 * ABI version: bumped whenever a struct of this header changes size or a field changes meaning (6: ai_ncut_stats gained max_true_resid,
 * true_resid_limit, accepted_above_limit, check_timeouts, spmv_blocks and spmv_blocks_idle; 5: restarted_solves and hist_retries; 4: round 4; 3 added
 * ai_ncut_opts.window_rows).  A binding checks ai_abi_version() == AI_ABI_VERSION and ai_abi_sizeof(which) against its own
 * struct sizes when it loads the library (autoinst_amd/_ffi.py does): a caller built against an older header would otherwise
 * pass a shorter ai_ncut_opts and have the library read past it.
 */
#define AI_ABI_VERSION 6
int ai_abi_version(void);
int64_t ai_abi_sizeof(int which); /* 0: ai_ncut_opts, 1: ai_ncut_stats; -1 otherwise */

typedef enum {
  AI_OK = 0,
  AI_ERR_BAD_ARG = -1,
  AI_ERR_OOM = -2,
  AI_ERR_NO_CONVERGENCE = -3,
  AI_ERR_HIP = -4,
  AI_ERR_INTERNAL = -5
} ai_status;

/* where the caller's buffers live */
typedef enum { AI_MEM_HOST = 0, AI_MEM_DEVICE = 1 } ai_mem;

#define AI_NUM_CUTS 10 /* pipeline/ncuts/normalized_cut.py:54  get_min_ncut(ev, D, w, 10) */

int ai_version(void);
const char* ai_last_error(void);

int ai_ctx_create(int device, ai_ctx** out);
int ai_ctx_destroy(ai_ctx* ctx);
/*
 * Device memory a context holds between calls (no reference counterpart: the reference's arrays are NumPy's).
 * out[0] = bytes of the call workspace (one block once the largest call has been seen: a longer list of blocks is replaced
 * by one of the peak need + 6 % at the start of the next call), out[1] = its number of blocks, out[2] = bytes of graphs
 * handed out and not yet freed, out[3] = bytes of freed graph buffers kept for re-use.
 */
int ai_ctx_mem_info(ai_ctx* ctx, int64_t out[4]);

/*
 * Affinity build.  Replaces pipeline/ncuts/ncuts_utils.py:60-67 (cdist + radius mask +
 * spatial weights), :125-133 (DINO factor), :135-149 (TARL factor with the all-zero-row
 * exemption), :151-156 (product), :159 (remove_isolated_points: identity, A_ii = 1) and
 * :167 (CSR conversion):
 *     A_ij = 1[d_ij <= radius] * exp(-theta t_ij) * exp(-alpha d_ij) * exp(-gamma g_ij)
 * xyz: n x 3 row-major; tarl: n x tarl_dim or NULL (theta ignored); dino likewise.
 * A falsy alpha / theta / gamma (0.0) drops that factor, as the reference's `if CONFIG[..]`.
 * gamma != 0 with dino == NULL is AI_ERR_BAD_ARG (reference raises ValueError, :126-127).
 * The graph stays on the device in the library's own (cell-sorted) row order.  It keeps a device copy of xyz (24 bytes per point,
 * released with the graph): ai_ncut / ai_ncut_batch start the solves of segments without a solved ancestor from their points'
 * principal-axis coordinate.  A graph made by ai_csr_from_host has no points; its segments start from the hash vector.
 */
int ai_affinity_build(ai_ctx* ctx, const double* xyz, int64_t n,
                      const double* tarl, int32_t tarl_dim,
                      const double* dino, int32_t dino_dim,
                      double alpha, double theta, double gamma, double radius,
                      int mem_kind, ai_csr** out);

/*
 * The same with the SAM factor of ncuts_utils.py:112-123 / utils/image/image_utils.py:64-89 (beta is 0.0 in
 * every shipped config, config.py:12,23,34,45, so the reference pipeline never takes this path): sam =
 * (n, sam_views) int32 SAM ids of one camera, -1 = no id in that view; per pair inside the radius the
 * factor is exp(-beta * fraction of the co-labelled views whose ids differ).  Factors are multiplied in
 * the reference's order tarl * spatial * sam * dino (:151-156).  beta != 0 without ids is a bad argument
 * (the reference raises ValueError, :116-117).
 */
int ai_affinity_build_sam(ai_ctx* ctx, const double* xyz, int64_t n, const double* tarl, int32_t tarl_dim,
                          const double* dino, int32_t dino_dim, const int32_t* sam, int32_t sam_views, double alpha,
                          double beta, double gamma, double theta, double radius, int mem_kind, ai_csr** out);

/*
 * One more camera (the loops over cameras at ncuts_utils.py:118-123 and :128-133; CAM_IDS has a single entry
 * in the reference's config.py:72): multiplies every stored value of an existing graph by that camera's
 * exp(-beta * SAM fraction) and exp(-gamma * ||dino_i - dino_j||).  The product is then associated
 * ((... * cam1) * cam2) instead of the reference's (cam1 * cam2): values agree to 1 ulp.
 */
int ai_affinity_apply_camera(ai_ctx* ctx, ai_csr* csr, const double* dino, int32_t dino_dim, const int32_t* sam,
                             int32_t sam_views, double beta, double gamma, int mem_kind);

/*
 * ai_affinity_build for every chunk of a map in one call (no reference counterpart: the reference builds chunk by chunk inside
 * ncuts_chunk).  xyz / tarl / dino hold the rows of all chunks one after the other (host or device by mem_kind), chunk c owning
 * rows off[c] .. off[c + 1]; off is a host array of n_chunks + 1 offsets from 0.  out[c] is a full graph of its own (own buffers,
 * own copy of the chunk's points; freed in any order, from any thread, accepted wherever a graph of ai_affinity_build is) and
 * equals, bit for bit in row pointers, columns, values and row order, what ai_affinity_build returns for that chunk's rows alone
 * with the same weights -- whichever chunks share the call, in whatever order, at whatever group_rows.
 * The call works through the chunks in groups of whole chunks of at most group_rows rows (<= 0: 2^21; a larger chunk is a group
 * of its own), so its workspace is that of one group however large the map.  The limits of ai_affinity_build hold per chunk.
 * AI_ERR_BAD_ARG: n_chunks <= 0, off[0] != 0, offsets that decrease, an empty chunk, a coordinate that is not finite (the
 * message names the first offending chunk), theta != 0 without tarl, gamma != 0 without dino.  On any failure every out[c] is
 * NULL and no graph of the call stays registered.  No SAM factor and no extra cameras here: ai_affinity_apply_camera per graph.
 */
int ai_affinity_build_batch(ai_ctx* ctx, const double* xyz, const int64_t* off, int32_t n_chunks, const double* tarl,
                            int32_t tarl_dim, const double* dino, int32_t dino_dim, double alpha, double theta, double gamma,
                            double radius, int64_t group_rows, int mem_kind, ai_csr** out);

/*
 * Upload a caller-built symmetric CSR (what ncuts_utils.py:167 hands to
 * normalized_cut at :168).  indptr has n+1 entries.  Row order is kept.
 *
 * The contract.  The cut reads the STORED entries (its connected components never look at a value, and a row trusts the other
 * row's copy of an edge), the reference is defined by the matrix's VALUE; the two agree only on a graph that keeps these rules,
 * so everything else is refused with AI_ERR_BAD_ARG and a message that starts "ai_csr_from_host:" and names the first offending
 * row and column:
 *   - a value that is not finite, a negative value, a stored zero of either sign;
 *   - a second entry with the same (row, col) -- duplicates are not summed;
 *   - an entry (i, j) whose mirror (j, i) is missing, or whose mirror's value differs in any bit.
 * Accepted exactly as stored (nothing is sorted or rewritten): any column order within a row; a diagonal that is present, absent
 * or partial, with any positive value (the cut adds the reference's identity on top of it); empty rows.
 * Values and duplicates are judged on the host before anything is allocated.  Mirrors: on the host too when some row's columns do
 * not ascend as stored; otherwise by one kernel on the uploaded copy, which is released again on refusal.  Either way a refused
 * graph leaves *out unwritten and ai_ctx_mem_info's out[2] as it was, and the context serves the next call.
 * Graphs built on the device (ai_affinity_build*) do not pass this door.
 */
int ai_csr_from_host(ai_ctx* ctx, int64_t n, const int64_t* indptr, const int32_t* indices,
                     const double* data, ai_csr** out);

int ai_csr_dims(const ai_csr* csr, int64_t* n, int64_t* nnz);

/*
 * Copy the graph out as scipy.sparse.csr_matrix(A) would hold it: rows and columns in
 * the caller's ORIGINAL point order, column indices ascending within a row.  (A graph from
 * ai_csr_from_host comes back as it was stored, bit for bit, whatever its column order.)
 * indptr: n+1, indices/data: nnz (host buffers).
 */
int ai_csr_export(ai_ctx* ctx, const ai_csr* csr, int64_t* indptr, int32_t* indices, double* data);

/*
 * Release a graph.  The device buffers go back to the cache of the context that BUILT the graph, whichever
 * context (or NULL) is passed here (hipFree would synchronise the whole device and stall other host threads);
 * they are re-used by that context's next graph of similar size and returned to the driver by ai_ctx_destroy.
 * A graph that outlives its context keeps a valid handle (free it as usual) but no buffers: every other call
 * on it returns AI_ERR_BAD_ARG ("the graph's context was destroyed").
 */
int ai_csr_free(ai_ctx* ctx, ai_csr* csr);

typedef struct {
  double tol;           /* Ritz residual |beta_m s_m| at which a Lanczos solve stops (default 1e-10) */
  int32_t max_iter;     /* Lanczos step cap per solve (default 4000; larger values are clamped to 4000: the convergence check keeps T_m in 64 KB of LDS) */
  int32_t check_every;  /* size of T at a solve's FIRST convergence check (default 16, at most 64); later checks are placed by the residual trend, 4 .. 48 steps apart */
  int32_t reserved;     /* profiling, fills ms_spmv (for bench.py): bit 0 or 1 = every SpMV launch stamps its own span (first block in .. last block out) on the device clock, which does not perturb how launches of several streams overlap */
  int64_t window_rows;  /* ai_ncut_batch: rows (points) of the chunks that iterate at one time; further chunks of the call are admitted as earlier ones finish, so the Lanczos vector storage is sized for the window, not for the call (0 = 4 800 000; never less than the call's largest chunk) */
} ai_ncut_opts;

typedef struct {
  int64_t levels;          /* harvest waves run (asynchronous frontier) / frontier levels processed (level-synchronous driver) */
  int64_t lanczos_solves;  /* connected segments solved by Lanczos */
  int64_t null_solves;     /* disconnected segments, split into their connected components in one step */
  int64_t lanczos_steps;   /* Lanczos steps launched (= fused SpMV launches); every iterating segment of the call takes part in a step at its own step count */
  int64_t spmv_rows;       /* rows processed by the SpMV kernel, summed over launches (exact, counted on device) */
  int64_t spmv_nnz;        /* stored entries processed by the SpMV kernel, summed over launches */
  int64_t unconverged;     /* solves that hit max_iter before tol */
  int64_t n_groups;
  double ms_total;         /* host wall time of the call */
  double ms_eigen;         /* wall time during which Lanczos segments were iterating (host clock) */
  double ms_spmv;          /* device time in the fused SpMV kernel alone (only with reserved bit 0 or 1) */
  double ms_sweep;         /* level-synchronous driver only: device time in min/max + bin + sweep */
  double ms_rebuild;       /* level-synchronous driver only: device time in CC + partition + CSR rebuild */
  double max_resid;        /* largest accepted Ritz residual */
  int64_t restarted_solves; /* solves repeated because the Ritz pair of a 'converged' segment failed the true-residual test
                               ||M v - theta v|| <= max(1e-6, 100 tol) ||v||.  Healthy solves measure <= tol; the repeat starts from
                               the same vector and is bit-identical to an undisturbed solve.  A repeat that arrives at the same
                               residual bit for bit is accepted (dense graphs with clustered top eigenvalues: Lanczos without
                               reorthogonalisation gives 3e-7 there), so the labels never depend on the test */
  int64_t hist_retries;     /* waves whose packed Lanczos histories (device -> pinned host memory) failed their header check (size of T,
                               integer checksum) and were packed again; 0 in a healthy run, labels do not depend on it */
  double max_true_resid;    /* largest TRUE residual ||M v - theta v|| / ||v|| of any Ritz pair that was cut (max_resid is the Lanczos
                               ESTIMATE |beta_m s_m| that stopped the solve; this one is measured on the segment's own entries) */
  double true_resid_limit;  /* the bar the call enforced on it: max(1e-6, 100 tol).  Above it a pair is solved again and cut only if the
                               repeat reproduces the residual bit for bit (then it is the algorithm's own answer) */
  int64_t accepted_above_limit; /* pairs cut with a true residual above the limit for that reason (dense blobs whose top eigenvalues
                               cluster: 3e-7 without re-orthogonalisation); 0 on the benchmark's chunks */
  int64_t check_timeouts;   /* convergence-check blocks that gave up waiting for their launch's scanning blocks (they judge nothing and
                               the next launch judges instead); 0 unless the device is oversubscribed */
  int64_t spmv_blocks;      /* only with opts->reserved bit 0 or 1: blocks dispatched by the stamped SpMV launches ... */
  int64_t spmv_blocks_idle; /* ... and how many of them found their segment frozen since the task lists were written (they end after a
                               record and a flag load; the lists are rewritten at the next relist) */
} ai_ncut_stats;

/*
 * Recursive normalized cut.  Replaces pipeline/ncuts/normalized_cut.py:37-63
 * (normalized_cut), :13-34 (get_min_ncut), :4-11 (cut_cost / ncut_cost) and the
 * scipy eigsh call at :49.  labels_out[i] (i in the caller's ORIGINAL row order) is the
 * index of point i's group in the order the reference's recursion emits groups
 * (mask side first); *n_groups receives their number.  split_lim applies to the top
 * call only; deeper calls use 0.01 as the reference does (:57-58 rely on the default).
 * opts / stats may be NULL.
 * A solve that reaches opts->max_iter before its residual falls to opts->tol makes the call return
 * AI_ERR_NO_CONVERGENCE (the reference's eigsh raises ArpackNoConvergence, normalized_cut.py:49); labels,
 * n_groups and stats (stats->unconverged, max_resid) are filled from the best vectors all the same.
 */
int ai_ncut(ai_ctx* ctx, const ai_csr* csr, int64_t num_points_orig, double T, double split_lim,
            const ai_ncut_opts* opts, int32_t* labels_out, int32_t* n_groups, ai_ncut_stats* stats);

/*
 * The same recursion over `count` independent chunks at once (run_pipeline.py:160-179 loops over
 * them one by one).  The connected segments of all chunks iterate in ONE pool, each at its own Lanczos
 * step count, so every kernel launch is shared by all of them: a single chunk's launches are
 * latency-bound, a batch fills them.  Chunks beyond opts->window_rows wait inside the call and are
 * admitted as earlier ones finish (a whole map can be one call).  Per chunk c: graphs[c], num_points_orig[c], labels_out[c] (graphs[c]->n ints, group
 * ids from 0 in that chunk's own emission order), n_groups[c].  Results are those of `count`
 * separate ai_ncut calls.  stats (may be NULL) describes the whole batch.
 */
int ai_ncut_batch(ai_ctx* ctx, const ai_csr* const* graphs, int32_t count, const int64_t* num_points_orig,
                  double T, double split_lim, const ai_ncut_opts* opts, int32_t* const* labels_out,
                  int32_t* n_groups, ai_ncut_stats* stats);

/*
 * The cut tree of a chunk: one cut at T_max that also answers every threshold T' <= T_max.  A segment is
 * split iff its best cut costs less than T, and neither the eligibility of a segment nor its solve depends on T, so the recursion
 * at T' is a prefix of the recursion at T_max.  The groups are position ranges of one array, in emission order, so the tree is flat:
 *   cut_height[g], g >= 1: the threshold above which the boundary between group g - 1 and group g exists -- the LARGEST cost among
 *     the cut that made the boundary and that cut's ancestors (costs are not monotone down the tree).  A Fiedler cut costs its mcut,
 *     a split into connected components exactly 0.0.  cut_height[0] = -inf.
 *   leaf_cost[g]: the mcut of the cut group g itself was refused (>= T_max; +inf where the sweep found none); NaN where the group
 *     was never solved (not eligible, or a disconnected segment under T_max <= 0).  The smallest one is the smallest threshold
 *     above T_max at which the partition would change.
 *   The group of point i at T' <= T_max is #{ j in [1, labels[i]] : cut_height[j] < T' } (strict, as the device compares);
 *   T' <= 0 leaves one group per chunk.
 * ai_ncut_tree / ai_ncut_tree_batch behave as ai_ncut / ai_ncut_batch with T = T_max (same labels, bit for bit) and fill
 * cut_height / leaf_cost (HOST arrays of capacity graphs[c]->n per chunk; leaf_cost may be NULL) wherever those fill the labels,
 * on AI_ERR_NO_CONVERGENCE too.
 *
 * ai_ncut_relabel: the labels at k thresholds from the trees of n_chunks chunks, in one call.  labels: the chunks' labels
 *   concatenated (off: HOST, n_chunks + 1); cut_height: their heights concatenated (goff: HOST, n_chunks + 1; chunk c has
 *   goff[c + 1] - goff[c] groups); thresholds: HOST, k values.  labels_out[t * N + i] (N = off[n_chunks]) is point i's group at
 *   thresholds[t], n_groups_out[t * n_chunks + c] (HOST) the number of chunk c's groups there.  labels, cut_height and labels_out
 *   are host or device per mem_kind.  AI_ERR_BAD_ARG, with no output written, for k < 1, a NaN or infinite threshold, a threshold
 *   above T_max, cut_height[goff[c]] != -inf, or a label outside [0, goff[c + 1] - goff[c]).  Chunks without points are allowed.
 */
int ai_ncut_tree(ai_ctx* ctx, const ai_csr* csr, int64_t num_points_orig, double T_max, double split_lim,
                 const ai_ncut_opts* opts, int32_t* labels_out, int32_t* n_groups, double* cut_height, double* leaf_cost,
                 ai_ncut_stats* stats);
int ai_ncut_tree_batch(ai_ctx* ctx, const ai_csr* const* graphs, int32_t count, const int64_t* num_points_orig,
                       double T_max, double split_lim, const ai_ncut_opts* opts, int32_t* const* labels_out,
                       int32_t* n_groups, double* const* cut_height, double* const* leaf_cost, ai_ncut_stats* stats);
int ai_ncut_relabel(ai_ctx* ctx, const int32_t* labels, const int64_t* off, int32_t n_chunks, const double* cut_height,
                    const int64_t* goff, double T_max, const double* thresholds, int32_t k, int mem_kind,
                    int32_t* labels_out, int32_t* n_groups_out);

/*
 * Building blocks exposed for parity tests (top-level call of the recursion only).  These run the
 * legacy Solver kernels (k_lz_* / k_sweep), NOT the ai_ncut / ai_ncut_batch path: the values of the
 * path that ships are pinned per segment by the test-only dump (tests/test_gpu_flow_values.py).
 * ai_fiedler: eigenpair of the 2nd-smallest eigenvalue of L_sym = D^-1/2 (D - W) D^-1/2,
 *   W = w + I (normalized_cut.py:38-53); ev_out (n, host, original order) has unit norm and
 *   the library's sign convention (entry of largest magnitude positive).  The graph must be
 *   connected, else a null-space vector is returned and *lambda2 = 0.
 * ai_sweep: the 10 threshold costs of normalized_cut.py:13-34 for a caller-given ev
 *   (host, original order); costs[10], mask_out[n] (uint8), *mcut.
 * ai_lsym_apply: y = L_sym x (host vectors, original order) through the SpMV kernel.
 */
int ai_fiedler(ai_ctx* ctx, const ai_csr* csr, const ai_ncut_opts* opts, double* lambda2,
               double* ev_out, int32_t* iters, double* resid);
int ai_sweep(ai_ctx* ctx, const ai_csr* csr, const double* ev, double* costs, uint8_t* mask_out,
             double* mcut);
int ai_lsym_apply(ai_ctx* ctx, const ai_csr* csr, const double* x, double* y);

/*
 * k smallest eigenpairs of L_sym = D^-1/2 (D - W) D^-1/2, W = w + I (BASELINE.json configs[4]; the
 * reference itself only ever asks for k = 2, normalized_cut.py:49).  1 <= k <= 64.
 * evals[k] ascending; evecs[j * n + i] = component i (caller's original order) of unit vector j.
 * Every connected component contributes one zero eigenvalue with eigenvector D^1/2 1_C / sqrt(vol_C)
 * (formed explicitly).  With >= k components the answer is k such pairs (any k of them are a
 * valid answer, as with SciPy).  Otherwise the remaining pairs are the smallest non-zero ones of the
 * union of the components' spectra: each component is solved on its own -- by Chebyshev-filtered subspace iteration
 * (n >= 1024 and >= 3 pairs wanted; stops when the true residuals of the first k - 1 pairs are <= opts->tol), else by Lanczos
 * with full re-orthogonalisation (stops when the innermost wanted pair's Ritz residual <= opts->tol) -- and the results are merged.
 */
int ai_eigs_smallest(ai_ctx* ctx, const ai_csr* csr, int32_t k, const ai_ncut_opts* opts, double* evals,
                     double* evecs, int32_t* iters, double* max_resid);

/*
 * "Next" rows on either side of the hot path.
 *
 * ai_radius_mean_pool: pipeline/utils/point_cloud/chunk_generation.py:243-256 -- out[i] (dim float64) =
 *   mean of the float32 feature rows of all source points with distance < radius from query i (a zero
 *   row when there is none); count_out[i] (may be NULL) = how many.  dim <= 384.
 * ai_nn1_project: pipeline/utils/point_cloud/point_cloud_utils.py:144-174 (kDTree_1NN_feature_reprojection)
 *   -- nn_index[i] = index of the source point nearest to fine point i, nn_dist[i] (may be NULL) its
 *   distance; the caller gathers labels / colours and applies max_radius.  A fine point with a NaN or infinite coordinate
 *   has no nearest source: nn_index[i] = -1, nn_dist[i] = NaN.
 * A NaN or infinite source coordinate is AI_ERR_BAD_ARG ("coordinates are not finite") in both.
 * Buffers are host or device according to mem_kind (all of one kind).
 */
int ai_radius_mean_pool(ai_ctx* ctx, const double* query_xyz, int64_t nq, const double* src_xyz, int64_t ns,
                        const float* src_feat, int32_t dim, double radius, int mem_kind, double* out,
                        int32_t* count_out);
int ai_nn1_project(ai_ctx* ctx, const double* to_xyz, int64_t nt, const double* from_xyz, int64_t nf,
                   int mem_kind, int32_t* nn_index, double* nn_dist);

/*
 * "Next" row 4: the per-point parts of the scorer and of the chunk merge.
 *
 * ai_label_pairs: the contingency table of two label arrays -- the distinct (a[i], b[i]) pairs in
 *   ascending (a, b) order with their counts.  Replaces the per-label np.unique / np.where /
 *   np.intersect1d / np.union1d passes of pipeline/metrics/metrics_class.py:302-309 (filter_labels),
 *   :60-114 (get_tp_fp), :181-235 (average_precision) and the np.unique of pred + gt * 2^32 of
 *   pipeline/metrics/modified_LSTQ.py:34-60.  a, b: host or device per mem_kind.  pair_a / pair_b /
 *   pair_count: HOST arrays of capacity `cap`; *n_pairs is always the full number of distinct pairs
 *   (call again with a larger cap when it exceeds cap).
 *
 * ai_merge_associate: the per-point work of one iteration of merge_chunks_unite_instances2
 *   (pipeline/utils/point_cloud/point_cloud_utils.py:397-463).  Instances are dense ids (0 = street /
 *   no instance, the reference's black colour) whose numeric order is the order of the reference's
 *   np.unique(colors, axis=0).  The map is cropped to the cube center +- side_length / 2 (inclusive,
 *   :405-417).  For id1 in [1, n_inst1), id2 in [1, n_inst2), row-major [id1 * n_inst2 + id2]:
 *     inter      = #chunk points of id2 inside the bounding box of the cropped points of id1 (:446-456);
 *     common     = #distinct scalar coordinate values the two instances share, so that the reference's
 *                  union (:458, np.unique of the concatenated arrays, flattened) is
 *                  n_scalars1[id1] + n_scalars2[id2] - common;
 *   n_points1[id1] = #cropped map points of id1 (0: the instance is not in the crop).
 *   Outputs are HOST arrays; the point / id arrays are host or device per mem_kind.
 *
 * ai_unique_points: PointCloud.remove_duplicated_points() (:489): indices (ascending) of the first point
 *   of every distinct coordinate triple.  keep_index (capacity n) is host or device per mem_kind.
 */
int ai_label_pairs(ai_ctx* ctx, const int32_t* a, const int32_t* b, int64_t n, int mem_kind, int64_t cap,
                   int32_t* pair_a, int32_t* pair_b, int64_t* pair_count, int64_t* n_pairs);
int ai_merge_associate(ai_ctx* ctx, const double* map_xyz, const int32_t* map_inst, int64_t n_map,
                       const double* chunk_xyz, const int32_t* chunk_inst, int64_t n_chunk, const double* center,
                       double side_length, int32_t n_inst1, int32_t n_inst2, int mem_kind, int32_t* inter,
                       int32_t* common, int32_t* n_scalars1, int32_t* n_scalars2, int32_t* n_points1);
int ai_unique_points(ai_ctx* ctx, const double* xyz, int64_t n, int mem_kind, int32_t* keep_index, int64_t* n_keep);

/*
 * The tail of the reference's loop (run_pipeline.py:214-238) for k label maps at once: what the scorer needs of k predictions of one
 * map against one ground truth, with remove_semantics (pipeline/utils/point_cloud/point_cloud_utils.py:249-287, called at
 * run_pipeline.py:223) applied by the reference's rule.  pred: k x n int32, row-major -- the layout
 * ai_ncut_relabel writes; gt: n int32; both host or device per mem_kind.  Every int32 value is a legal label, as for ai_label_pairs.
 *   S1  Tables.  For every row t the distinct pairs (pred[t][i], gt[i]) with their int64 counts, in ascending (pred, gt) order: row
 *       t of the call equals ai_label_pairs(pred[t], gt) exactly.  The rows stand behind each other; row t is the pairs
 *       row_off[t] .. row_off[t + 1] - 1.
 *   S2  Removal (remove_semantics).  For a label u of row t let m = #{i : pred[t][i] == u} and z = #{i : pred[t][i] == u and
 *       gt[i] == 0}.  u is removed iff (double)z > threshold * (double)m: one float64 multiply and one strict comparison, the
 *       reference's `cur_intersect > threshold * len(pred_idcs)`.  Label 0 takes part like any other label; removing it changes
 *       nothing.  pred_removed[t][i] = 0 where the label of the point is removed, pred[t][i] elsewhere.  Rows do not see each other.
 *   S3  Small labels (filter_labels, pipeline/metrics/metrics_class.py:302-309).  u is small iff m < min_points.  The scorer filters
 *       AFTER the removal, this entry decides on the labels as given, and that is the same: the removal moves whole labels to 0, so
 *       a label u != 0 that survives it keeps every one of its m points and gains none -- it is small after iff it was small before
 *       -- and a removed label no longer exists.  Only label 0 grows, and whether 0 is small makes no difference: a small label
 *       becomes 0.
 *   S4  What the scorer sees.  `all` is pred with the small labels set to 0; `scored` is pred with the removed or small labels set
 *       to 0 (pred_scored).  Every pair carries the flags of its label, pair_flags bit 0 = removed and bit 1 = small, so the host
 *       forms both contingency tables by uniting the rows of the flagged labels with label 0's: no second pass over the points.
 *   S5  Limits and errors.  1 <= k <= 64, n < 2^31 - 1, threshold finite and >= 0, min_points >= 0; any of them violated is
 *       AI_ERR_BAD_ARG with no output written.  n == 0 is no error: every row has zero pairs.  pair_pred / pair_gt / pair_count /
 *       pair_flags are HOST arrays of capacity `cap`; row_off (HOST, k + 1 entries) is always filled with the full counts: call again
 *       when row_off[k] > cap, as with ai_label_pairs.  Then exactly the leading cap pairs are written and nothing beyond them.
 *       pred_removed and pred_scored (k x n, placed per mem_kind, each may be NULL) are written in full whatever cap is.
 * A row is counted in hash tables (block-local in LDS, then one 64-bit atomic add per distinct pair and block) of 8192 and, when it
 * has more than 4096 distinct pairs, 131072 slots; a row with more than 65536 distinct pairs goes through ai_label_pairs' sort.  The
 * result does not depend on the path a row took: counts are integers, and every row's pairs are sorted at the end.
 * Host synchronisations: two when every row fits its first table (the rows' sizes, the result); one more when a row needs the
 * second table, and one more -- for all such rows together -- when a row needs the sort.  At most four, whatever k is.
 */
int ai_label_tables(ai_ctx* ctx, const int32_t* pred, const int32_t* gt, int32_t k, int64_t n, double threshold, int64_t min_points,
                    int mem_kind, int64_t cap, int32_t* pair_pred, int32_t* pair_gt, int64_t* pair_count, uint8_t* pair_flags,
                    int64_t* row_off, int32_t* pred_removed, int32_t* pred_scored);

/*
 * The instance-level arithmetic of the scorer for the same k label maps, on the device: the greedy matching of get_tp_fp /
 * average_precision (pipeline/metrics/metrics_class.py:60-114, :181-235) at every overlap and S_assoc (pipeline/metrics/
 * modified_LSTQ.py:23-80) per row, from the sorted pairs ai_label_tables forms.  pred, gt, k, n, threshold,
 * min_points and mem_kind are ai_label_tables'; remove != 0 scores the labels after remove_semantics, remove == 0 the labels as given
 * (after filter_labels either way).  overlaps: HOST, n_overlaps float64 IoU thresholds (metrics_class.py:37).
 *   Q1  Tables and flags.  Exactly S1-S3 of ai_label_tables on the same input.
 *   Q2  Labels.  The scored labels of row t are the labels u != 0 whose flags have no bit of `mask` set, mask = removed | small with
 *       remove and small without it, in ascending signed order; their number is n_pred.  Negative labels take part.  The association
 *       labels are the labels u > 0 that are not small, whatever remove is.
 *   Q3  Areas.  ap(u) is the m of rule S2.  ag(v) is the number of points with gt == v, the points of flagged labels included: the
 *       column sum of the full table.
 *   Q4  IoU of a stored pair (u, v, c): (double)c / (double)max(ap(u) + ag(v) - c, 1), one correctly rounded float64 division.  The
 *       pair is a candidate at overlap o iff iou >= overlaps[o] and v != 0.  A pair that is not stored has IoU 0 and is no candidate.
 *   Q5  Greedy match, per overlap independently.  The scored labels go in ascending order; a label takes the first of its
 *       candidates, v ascending, that no earlier label of this overlap took -- a hit -- and a label with none left is a miss.  For
 *       row t one byte (1 hit, 0 miss) per (overlap, scored label), overlap-major and in label order: byte
 *       hit_off[t] * n_overlaps + o * n_pred + rank.
 *   Q6  Integers per row.  row_counts[3 t + 0 .. 2] = n_pred, the number of distinct v != 0, whether v == 0 occurs (0 / 1);
 *       tp[t * n_overlaps + o] = the hits of overlap o.
 *   Q7  S_assoc per row (modified_LSTQ.py:23-80).  v is kept iff v != 0 and ag(v) > min_points; with no kept v the result is NaN.
 *       inner(v) is 0.0 unless v > 0; then it is the sum, over the association labels u ascending that have a pair (u, v, c), of
 *       (double)c * ((double)c / (double)(ag(v) + ap(u) - c)), added in that order starting from 0.0.  outer is the sum over the kept
 *       v ascending of inner(v) / (double)ag(v), and s_assoc[t] = outer / (double)#kept.  Every operation is rounded once; nothing is
 *       fused.
 *   Q8  Limits and errors.  S5's limits; 1 <= n_overlaps <= 16; every overlap finite and in (0, 1] (an overlap above 0 is what lets
 *       only stored pairs be candidates); any of them violated is AI_ERR_BAD_ARG with no output written.  n == 0 is no error: every row
 *       gets zeros and a NaN s_assoc.  hit_off (k + 1 entries, in scored labels), row_counts (3 k), tp (k * n_overlaps) and s_assoc
 *       (k) are HOST arrays and always complete.  hits (HOST, capacity cap bytes) follows the capacity rule of ai_label_pairs: call
 *       again when hit_off[k] * n_overlaps > cap; then exactly the leading cap bytes are written and nothing beyond them.
 * Results are integers or float64 sums in a fixed order: bit-identical from run to run, between host and device inputs and
 * whichever table path a row took.  The taken-flags of a (row, overlap) are one bit per distinct v != 0: in LDS up to 2048 of them,
 * in global scratch beyond.
 * Host synchronisations: those of ai_label_tables on the same input, whose last one here brings the per-row results, and one more
 * for the hit bytes (none when there are none): at most five.
 */
int ai_label_scores(ai_ctx* ctx, const int32_t* pred, const int32_t* gt, int32_t k, int64_t n, double threshold, int64_t min_points,
                    int mem_kind, int32_t remove, const double* overlaps, int32_t n_overlaps, int64_t cap, uint8_t* hits,
                    int64_t* hit_off, int32_t* row_counts, int32_t* tp, double* s_assoc);

/*
 * The step that produces the chunks: chunk_and_downsample_point_clouds (pipeline/dataset/dataset_utils.py:489-567, called at
 * run_pipeline.py:129), per chunk and per cloud (non-ground / ground).  xyz and the index / point outputs are host or device
 * according to mem_kind; counts, offsets and stats are HOST values.  Indices are int32 (n < 2^30; box select: n < 2^31 - 256).
 *
 * ai_box_select: the crop of chunk_generation.py:134-137 for n_boxes boxes at once.  boxes (HOST, n_boxes x 6 doubles: lo x, y,
 *   z, hi x, y, z); a point is inside box b iff lo < p < hi on all three axes (strict).  out_index receives, box after box, the
 *   ascending indices of the points inside each box; box_offsets (HOST, n_boxes + 1) the start of each box's run and the total.
 *   *n_total is always the full count: when it exceeds cap nothing is written to out_index (call again with cap >= *n_total).
 *
 * ai_statistical_inliers: open3d 0.17 PointCloud::RemoveStatisticalOutliers (pipeline/utils/point_cloud/point_cloud_utils.py:
 *   198-202, called at chunk_generation.py:143) as it is written: k = min(nb_neighbors, n); avg[i] = the mean of the Euclidean
 *   distances of the k nearest points of i (i itself included, at distance 0), summed in ascending order; mean = (sum of the
 *   avg > 0) / n (all n points in the denominator); std = sqrt(sum over avg > 0 of (avg - mean)^2 / (n - 1)); i is kept iff
 *   avg[i] > 0 && avg[i] < mean + std_ratio * std.  keep_index (capacity n) receives the kept indices in ascending order and
 *   *n_keep their number.  avg_out (n, per mem_kind) and stats_out (HOST: mean, std, threshold) may be NULL.  nb_neighbors < 1,
 *   std_ratio <= 0, or k > 64 is AI_ERR_BAD_ARG; n = 0 keeps nothing (stats_out is not written).  Reproducible bit for bit.
 *   The kNN is exact: the k distances of a point are the square roots of the k smallest (dx*dx + dy*dy) + dz*dz (every step
 *   rounded, no contraction) over the whole cloud, so avg is a function of the points alone -- not of the cell list the search
 *   runs on -- and equals a brute-force restatement bit for bit.  mean and std are fixed-order sums (tests/prep_cases.py bounds
 *   them against the correctly rounded ones).
 *
 * A NaN or infinite coordinate is AI_ERR_BAD_ARG ("coordinates are not finite") in ai_statistical_inliers and in both voxel
 *   entries, and so is a bounding box of 1e15 or more on an axis; no output array is written then.  ai_box_select takes no
 *   bounds: such a point fails every comparison and is inside no box.
 *
 * ai_voxel_down_sample: open3d PointCloud::VoxelDownSample (dataset_utils.py:534-535): vmin = min_bound - voxel_size / 2, voxel
 *   of p = floor((p - vmin) / voxel_size), output point = sum of the voxel's points in input-index order / their count.  Output
 *   order: ascending (ix, iy, iz) (open3d's is the order of a hash map).  out_xyz (capacity n x 3), trace (n, may be NULL: the
 *   output row of every input point); *n_out = number of voxels.  voxel_size <= 0, or a voxel index outside the int range
 *   (open3d's "voxel_size is too small"), is AI_ERR_BAD_ARG.
 *
 * ai_voxel_down_sample_nearest: the minor-voxel map of load_and_downsample_point_clouds (dataset_utils.py:285-370), i.e.
 *   voxel_down_sample_and_trace(voxel_size, min_bound, max_bound) plus, per output point, the raw point whose label the reference's
 *   KD-tree loops copy (:306-311, :324-328, :340-350, :362-367).  out_xyz, *n_out and trace are ai_voxel_down_sample's, bit for bit,
 *   with the same errors.  nearest_index[v] (capacity n) = the index of the input point nearest to out_xyz[v]: the smallest
 *   (dx*dx + dy*dy) + dz*dz (every step rounded, no contraction), ties to the smaller input index -- ai_nn1_project's rule.  The tie
 *   rule is ours: open3d's KD-tree defines none (and open3d is not installed where this is tested).  nearest_dist[v] (may be NULL) =
 *   the correctly rounded sqrt of that square.  n = 0 gives *n_out = 0; n < 2^31 - 256 as for ai_box_select.
 */
int ai_box_select(ai_ctx* ctx, const double* xyz, int64_t n, const double* boxes, int32_t n_boxes, int mem_kind,
                  int64_t cap, int32_t* out_index, int64_t* box_offsets, int64_t* n_total);
int ai_statistical_inliers(ai_ctx* ctx, const double* xyz, int64_t n, int32_t nb_neighbors, double std_ratio,
                           int mem_kind, int32_t* keep_index, int64_t* n_keep, double* avg_out, double* stats_out);
int ai_voxel_down_sample(ai_ctx* ctx, const double* xyz, int64_t n, double voxel_size, int mem_kind, double* out_xyz,
                         int64_t* n_out, int32_t* trace);
int ai_voxel_down_sample_nearest(ai_ctx* ctx, const double* xyz, int64_t n, double voxel_size, int mem_kind,
                                 double* out_xyz, int64_t* n_out, int32_t* trace, int32_t* nearest_index,
                                 double* nearest_dist);

/*
 * The camera projection of the tri-modal configuration: image_based_features_per_patch (pipeline/utils/image/image_utils.py:
 * 146-348, point_to_pixels.py:6-35) and dinov2_mean (:363-371) for every (query point i, view v) pair:
 *   1. q and the visible points go to the camera frame: row r = ((T[r,0]*x + T[r,1]*y) + T[r,2]*z) + T[r,3], divided by row 3;
 *   2. (i, v) is seen iff some cloud_xyz[vis_index[k]], vis_off[v] <= k < vis_off[v+1], has sqrt(squared distance) < max_dist in
 *      the camera frame (squared distance (dx*dx + dy*dy) + dz*dz);
 *   3. u' = (K00*x + K01*y) + K02*z (v', w' likewise), u = rint(u'/w'), v = rint(v'/w'); kept iff 0 <= u < img_w, 0 <= v < img_h
 *      and w' > 0 in double: pixel_out[i, v] = (u, v), else (-1, -1);
 *   4. sam_out[i, v] = sam_img[v][v_px][u_px] when kept and that label is not 0, else -1;
 *   5. the feature cell of a kept pair is ((int)(fh / img_h * v_px), (int)(fw / img_w * u_px)); a cell outside the map is
 *      AI_ERR_BAD_ARG (the reference raises IndexError);
 *   6. feat_mean[i] = the float64 sum, in view order, of the cells' rows that hold an element != 0, divided by their number
 *      feat_views[i] (a zero row when there is none).
 * query_xyz (nq x 3), cloud_xyz (nc x 3), vis_index, feat (n_views x fh x fw x fdim float32), sam_img (n_views x img_h x img_w) and
 * the outputs are host or device per mem_kind; vis_off (n_views + 1), T_pcd2cam (n_views x 16, row-major 4 x 4, last row
 * 0 0 0 1) and K (9, row-major) are HOST arrays.  n_views <= 64.  pixel_out (nq x n_views x 2) may be NULL; sam_out (nq x n_views)
 * is NULL iff sam_img is; feat_mean (nq x fdim) and feat_views (nq) are NULL iff feat is.
 */
int ai_camera_project(ai_ctx* ctx, const double* query_xyz, int64_t nq, const double* cloud_xyz, int64_t nc,
                      const int32_t* vis_index, const int64_t* vis_off, int32_t n_views, const double* T_pcd2cam, const double* K,
                      int32_t img_h, int32_t img_w, double max_dist, const float* feat, int32_t fh, int32_t fw, int32_t fdim,
                      const int32_t* sam_img, int mem_kind, int32_t* pixel_out, int32_t* sam_out, double* feat_mean,
                      int32_t* feat_views);

/*
 * The TARL scan features of every chunk of a map in one call: tarl_features_per_patch (pipeline/utils/point_cloud/
 * chunk_generation.py:221-256) for all chunks at once.  scan_xyz holds all sampled scans, one after the
 * other, each in its own sensor frame (scan s: rows scan_off[s] .. scan_off[s+1]); scan_feat their float32 features (M x dim);
 * query_xyz all chunks' major-voxel points (chunk c: rows query_off[c] .. query_off[c+1]); boxes[c] = lo x, y, z, hi x, y, z;
 * scan_win[c] = [first, last) positions in the scan list (the reference's slice of sampled_indices_global, :261-271).
 *   R1 Transform.  A scan point goes to the pcd frame in a fixed order: row r = ((T[r,0]*x + T[r,1]*y) + T[r,2]*z) + T[r,3],
 *      divided by row 3, every step rounded on its own (no contraction; not a BLAS product).  A last row of T other than
 *      (0, 0, 0, 1) is AI_ERR_BAD_ARG.
 *   R2 Membership.  Point p of scan s is in the mean of query i of chunk c iff scan_win[c][0] <= s < scan_win[c][1], the
 *      transformed p is strictly inside box c on all three axes (lo < p < hi), and (dx*dx + dy*dy) + dz*dz, every step rounded,
 *      is strictly below radius * radius rounded once (ai_radius_mean_pool's test).
 *   R3 Mean.  out[i] = the float64 sum of the member rows (float32 widened) divided once by their number count_out[i] (may be
 *      NULL); a zero row when there is no member.
 *   R4 Order.  Members are summed in ascending order of their cell index (ix, iy, iz), then ascending position in scan_xyz.
 *      The cell index is floor(coord * (1 / cell)), cell = radius * (1 + 1e-9), origin 0 and signed (the key stores it less a
 *      bias): the order is a function of the coordinates alone.  Two calls are bit-identical, and so are a chunk's rows
 *      whether it is pooled alone or with other chunks, with only its window's scans or with the whole map's.
 *   R5 Limits and errors.  M = scan_off[n_scans] and Nq = query_off[n_chunks] < 2^31 - 256.  AI_ERR_BAD_ARG: dim < 1 or > 384;
 *      radius <= 0 or not finite; a window outside [0, n_scans] or with first > last; an offset array that does not start at 0
 *      or decreases; a non-finite coordinate, box bound or transform; a cell index that does not fit its key field
 *      (|index| >= 2^30, or the boxes' index ranges need more than 30 key bits on an axis or 63 together).  Not errors: n_chunks == 0, a chunk
 *      with no queries, an empty window, a scan with no points, M == 0; a chunk with no members gets zero rows and counts.
 *      The arguments are checked in full whether or not there is a query (scan coordinates included).
 * scan_xyz, scan_feat, query_xyz, out and count_out are host or device per mem_kind; every other array is a HOST array
 * (T_scan2pcd: n_scans x 16 row-major; boxes: n_chunks x 6; scan_win: n_chunks x 2; the offsets: n + 1 entries).
 */
int ai_scan_pool(ai_ctx* ctx, const double* scan_xyz, const int64_t* scan_off, int32_t n_scans, const double* T_scan2pcd,
                 const float* scan_feat, int32_t dim, const double* query_xyz, const int64_t* query_off, int32_t n_chunks,
                 const double* boxes, const int32_t* scan_win, double radius, int mem_kind, double* out, int32_t* count_out);

/*
 * The aggregated raw clouds of a map from its scans in one call: the loop of aggregate_pointcloud (pipeline/utils/point_cloud/
 * aggregate_pointcloud.py:99-186) with the dataset's filter chain (pipeline/dataset/filters/kitti_gt_mo_filter.py:40-51,
 * range_filter.py:23-36) and the three label decodes (pipeline/dataset/kitti_odometry_dataset.py:73-104).
 * scan_xyz holds all scans one after the other, each in its own sensor frame, float32 as the dataset returns them (scan s: rows
 * scan_off[s] .. scan_off[s+1]); pose[s] takes scan s to the map frame; label_word (may be NULL) the raw .label words;
 * ground_flag (may be NULL) one byte per INPUT point, non-zero = ground (the ground segmentation itself stays the caller's).
 *   A1 Moving-object filter.  With moving_index >= 0 a point is kept iff (label_word & 0xFFFF) < moving_index (the reference's
 *      value is 251); moving_index < 0 switches the filter off.  The filter without label_word is AI_ERR_BAD_ARG.
 *   A2 Range filter (is_centered = True).  s = (x*x + y*y) + z*z in float32, every step rounded, no contraction; r = the correctly
 *      rounded float32 square root of s; kept iff r >= (float)range_min && r <= (float)range_max, both ends inclusive.  A NaN
 *      coordinate fails both comparisons and is dropped, as in NumPy.  range_max < 0 switches the filter off.
 *   A3 Class.  A kept point is ground iff ground_flag is given and non-zero there, else non-ground; with ground_flag == NULL every
 *      kept point is non-ground (the reference's ground_segmentation=None branch, :46-87).
 *   A4 Transform.  The float32 coordinates are widened to float64 (exact), then rule R1 of ai_scan_pool: row r = ((T[r,0]*x +
 *      T[r,1]*y) + T[r,2]*z) + T[r,3], divided by row 3, every step rounded on its own.  A last row of a pose other than exactly
 *      (0, 0, 0, 1) is AI_ERR_BAD_ARG.
 *   A5 Order.  Each output map holds its points in ascending input position: scan after scan (the reference's map += pcd),
 *      ascending index within a scan -- a stable partition.  The order within a scan is ours: the reference's is that of the
 *      index list its ground segmentation returns.
 *   A6 Labels, per kept point from its word w, all in uint32 arithmetic: seg = w & 0xFFFF; panoptic = (w & 0xFFFF0000) if that
 *      is not 0, else w & 0xFFFF; instance = (w & 0xFFFF0000) * (w & 0x10009) modulo 2^32.  The reference writes
 *      `labels_orig & 0xFFFF + 10` (:102), and + binds before &: the mask really is 0x10009, and the uint32 product wraps.  That
 *      is reproduced, not mended.
 *   Limits and errors.  M = scan_off[n_scans] < 2^31 - 256, as for ai_box_select.  AI_ERR_BAD_ARG: an offset array that does not
 *      start at 0 or decreases; a non-finite pose entry; range_min > range_max (or a NaN bound) while the range filter is on; a
 *      label output without label_word.  Not errors: n_scans == 0, a scan with no points, a call in which nothing survives or in
 *      which everything is ground.  The arguments are checked in full before any output is written.
 * Outputs, per class: out_xyz_* (float64, capacity M x 3), out_seg_*, out_instance_*, out_panoptic_* (uint32, capacity M) and
 * out_src_* (int32, capacity M: the input position of every output point).  The label outputs and out_src_* may be NULL each.
 * class_off (HOST, 2 x (n_scans + 1) int64, may be NULL): row 0 where each scan's run starts in the ground map, row 1 in the
 * non-ground map; entry n_scans of a row is the map's size, also returned in *n_ground / *n_nonground (HOST).  scan_xyz,
 * label_word, ground_flag and the out_* arrays are host or device per mem_kind; scan_off (n_scans + 1) and pose (n_scans x 16
 * doubles, row-major 4 x 4) are HOST arrays.  Two calls are bit-identical, and a scan's run is the same whether it is aggregated
 * alone or among others.
 */
int ai_aggregate_scans(ai_ctx* ctx, const float* scan_xyz, const int64_t* scan_off, int32_t n_scans, const double* pose,
                       const uint32_t* label_word, const uint8_t* ground_flag, int32_t moving_index, double range_min,
                       double range_max, int mem_kind, double* out_xyz_ground, double* out_xyz_nonground, uint32_t* out_seg_ground,
                       uint32_t* out_seg_nonground, uint32_t* out_instance_ground, uint32_t* out_instance_nonground,
                       uint32_t* out_panoptic_ground, uint32_t* out_panoptic_nonground, int32_t* out_src_ground,
                       int32_t* out_src_nonground, int64_t* class_off, int64_t* n_ground, int64_t* n_nonground);

/*
 * The tail of ncuts_chunk (pipeline/ncuts/ncuts_utils.py:177-204) and get_corrected_ground (pipeline/utils/point_cloud/
 * point_cloud_utils.py:331-342) for every chunk of a map in one call: from the group of every major-voxel
 * point to the merged chunk that merge_chunks_unite_instances2 takes.  All chunks lie one after the other: fine_xyz the minor
 * non-ground chunk points (chunk c: rows fine_off[c] .. fine_off[c+1]), major_xyz the major-voxel points the cut labelled, with
 * one group id each in major_label (may be NULL), ground_xyz the ground chunk points.
 *   F1 Segmentation.  A fine point of chunk c sees only the major rows major_off[c] .. major_off[c+1], a ground point only its
 *      own chunk's ground rows (chunks overlap in space).
 *   F2 Nearest major point: the rule of ai_nn1_project.  Smallest (dx*dx + dy*dy) + dz*dz, every step rounded, no contraction;
 *      ties to the smaller major index; fine_nn[i] is chunk-local; fine_dist[i] = the correctly rounded sqrt;
 *      fine_label[i] = major_label[major_off[c] + fine_nn[i]].  No radius (the reference passes max_radius=None).
 *   F3 Ground inliers: the rules of ai_statistical_inliers on the chunk's ground rows alone, k = min(nb_neighbors, n_c).
 *      ground_avg, mean, std and threshold are bit-equal to that entry called on the chunk by itself.
 *   F4 Mean height.  mean_z = the float64 sum of z over the chunk's inliers divided once by their number.  Order of the sum,
 *      with i the chunk-local index: slot s = i mod 65536 adds its inliers i = s, s + 65536, ... in ascending order; the slots
 *      256 b .. 256 b + 255 of block b are summed as four waves of 64, each by a pairwise tree (neighbours, then pairs of 2, 4,
 *      8, 16, 32 slots), then ((w0 + w1) + w2) + w3; the 256 block sums are summed the same way.  Without inliers mean_z is NaN
 *      (np.mean of an empty array) and nothing is kept.
 *   F5 Height cut.  z_limit = mean_z + mean_height, rounded once; a ground point is kept iff it is an inlier and z < z_limit
 *      (strict).  ground_keep holds, chunk after chunk, the ascending chunk-local indices of the kept points (the reference's
 *      [inliers][in_idcs]); chunk c's run is keep_off[c] .. keep_off[c+1].
 *   F6 Merged chunk (the reference's pcd_chunk + cut_hight): rows merged_off[c] .. merged_off[c+1] hold chunk c's fine points in
 *      input order, then its kept ground points in ascending order, coordinates copied bit for bit; merged_label is
 *      fine_label + 1 for the fine part and 0 (the merge's "no instance") for the ground part.
 *   F7 Independence.  Two calls are bit-identical, and so are a chunk's outputs whether it is finished alone, with other
 *      chunks, or in another chunk order.
 *   Limits and errors.  Each of the three totals is below 2^30; n_chunks <= 65535.  AI_ERR_BAD_ARG: an offset array that does
 *      not start at 0 or decreases; a non-finite coordinate; a chunk with fine points and no major points; nb_neighbors < 1,
 *      std_ratio <= 0, or nb_neighbors > 64 with some chunk above 64 ground points; a non-finite mean_height; fine_label or the
 *      merged outputs without major_label; the merged outputs not all NULL or all given.  The arguments are checked in full before
 *      any output is written.  Not errors: n_chunks == 0, an empty chunk, a chunk without ground, a chunk with one ground point
 *      (its avg is 0: nothing is kept).
 * Outputs, each may be NULL: fine_nn, fine_label (Nf int32), fine_dist (Nf doubles), ground_avg (Ng doubles), ground_keep
 * (capacity Ng int32), merged_xyz (capacity (Nf + Ng) x 3), merged_label (capacity Nf + Ng) -- host or device per mem_kind, as
 * the three point arrays and major_label are; keep_off, merged_off (n_chunks + 1 int64) and ground_stats (n_chunks x 6 doubles:
 * mean, std, threshold, n_inliers, mean_z, z_limit; NaN statistics for a chunk without ground) are HOST arrays, as the three offset
 * arrays are.  Two host synchronisations per call with device memory, three with host memory, whatever n_chunks is.
 */
int ai_chunk_finish(ai_ctx* ctx, const double* fine_xyz, const int64_t* fine_off, const double* major_xyz,
                    const int64_t* major_off, const int32_t* major_label, const double* ground_xyz, const int64_t* ground_off,
                    int32_t n_chunks, int32_t nb_neighbors, double std_ratio, double mean_height, int mem_kind, int32_t* fine_nn,
                    double* fine_dist, int32_t* fine_label, double* ground_avg, int32_t* ground_keep, int64_t* keep_off,
                    double* ground_stats, double* merged_xyz, int32_t* merged_label, int64_t* merged_off);

/*
 * The step that turns the chunks into the map, merge_chunks_unite_instances2 (pipeline/utils/point_cloud/point_cloud_utils.py:387-491),
 * for all chunks of a map in one resident call.  The identity of an instance is its id, not a colour.
 * xyz: (M, 3) float64, all chunks one after the other; inst: M int32 chunk-local instance ids, 0 = no instance (street); chunk c
 * is rows a = off[c] .. b = off[c+1] (off: HOST, n_chunks + 1 entries).  Chunks are taken in order.
 *   M1  Ids.  nloc[c] = the largest local id of chunk c, goff = its exclusive prefix sum.  The provisional global id of local id
 *       l > 0 of chunk c is goff[c] + l; 0 stays 0.  Global ids are not compacted.
 *   M2  Duplicates.  Two points are the same if all three coordinates are equal as values (-0.0 == +0.0, ai_unique_points' rule).
 *       keep[i] is true for the first point of every distinct triple over the whole concatenation; the output is exactly the kept
 *       points in ascending position.  A kept point has the global id its own chunk's step gave it; it never changes afterwards.
 *       With n_chunks == 1 every point is kept, duplicates too (the reference's loop, which removes them, does not run).
 *   M3  The map a step sees.  Step c >= 1 sees the kept points at positions < a whose global id is > 0; step 1 alone sees every
 *       point of chunk 0, kept or not (the reference removes duplicates only at the end of its first iteration).  An empty chunk
 *       is skipped: it associates nothing and adds nothing.
 *   M4  Centre.  centers[c] if given; otherwise per axis the sum of the chunk's coordinates divided once by their number, the sum in
 *       F4's order (ai_chunk_finish above) over the chunk-local row index: 65536 slots, 256 blocks of four waves, pairwise trees,
 *       the 256 block sums the same way.  Bit-identical from call to call and independent of the other chunks of the call.
 *   M5  Crop.  A map point of M3 is cropped in iff centre - side_length / 2 <= p <= centre + side_length / 2 on all axes, both
 *       sides inclusive, the bounds computed as written.
 *   M6  Per map instance g present in the crop: its box is the min and max per axis of its cropped points; S1(g) is the set of
 *       distinct scalar coordinate values of its cropped points, the three axes pooled (np.unique without axis).
 *   M7  Per local instance l > 0 of the chunk: S2(l) is the same set over ALL chunk points of l, duplicates and already-known
 *       points included.
 *   M8  Pair.  inter(g, l) = the number of chunk points of l with box_min <= p <= box_max of g; only inter > 0 counts.
 *       union = |S1| + |S2| - |S1 n S2|; iou = double(inter) / double(union); the pair qualifies iff iou > iou_min, strictly.
 *   M9  Association.  l takes the global id of the qualifying g with the largest iou, among equal iou the smallest g (the
 *       order-free form of :465-477).  Several l may take the same g; an l without a qualifying pair keeps its provisional id.
 *   M10 Limits and errors.  M < 2^30, n_chunks <= 65535, goff[n_chunks] < 2^31 - 1.  AI_ERR_BAD_ARG, with the chunk named: offsets
 *       that do not start at 0 or that decrease; a negative local id; a non-finite coordinate; a non-finite centre;
 *       side_length <= 0; iou_min not finite; n_out == NULL (the one output the others cannot be returned without).  Per step at
 *       most 3 * (cropped + chunk points of instances) <= 2^31 - 2 scalar entries and (instances in the crop) x (nloc[c] + 1)
 *       < 2^28 table entries; a step beyond either is AI_ERR_BAD_ARG.  n_chunks == 0 or M == 0 gives *n_out = 0.
 * Outputs of capacity M, host or device per mem_kind as xyz and inst are, each may be NULL: out_xyz (n_out x 3, coordinates bit for
 * bit), out_inst (int32 global ids), out_src (int64, the position of each kept point in the concatenation, ascending).  HOST
 * outputs: *n_out; inst_table (goff[n_chunks] + 1 int32, may be NULL): the global id local id l of chunk c ended with at
 * [goff[c] + l], entry 0 is 0 -- size it as 1 + the sum over the chunks of their largest id; stats (n_chunks x 4 int64, may be NULL):
 * cropped map points, map instances present in the crop, pairs above iou_min, local instances re-labelled; centers_used
 * (n_chunks x 3 doubles, may be NULL): the centre of every chunk (NaN for an empty chunk without a given centre).
 * Working memory and the box loop scale with the instances present in a step's crop, not with the ids of the map.  Three host
 * synchronisations per step, each for one or two counts; no array of points crosses the host link with device memory.
 */
int ai_merge_map(ai_ctx* ctx, const double* xyz, const int32_t* inst, const int64_t* off, int32_t n_chunks, const double* centers,
                 double side_length, double iou_min, int mem_kind, double* out_xyz, int32_t* out_inst, int64_t* out_src,
                 int64_t* n_out, int32_t* inst_table, int64_t* stats, double* centers_used);

/*
 * The ground / non-ground split of every scan of a map in one call: one RANSAC plane per scan, the open3d branch of
 * aggregate_pointcloud (pipeline/utils/point_cloud/aggregate_pointcloud.py:115-123: segment_plane(distance_threshold=0.4,
 * ransac_n=3, num_iterations=2000)) with a counter-based sampler in place of open3d's unseeded generator.
 * The result is a function of (points, seed, scan key) alone; ground_flag goes unchanged into ai_aggregate_scans.
 *   G1 Kept points.  The scans lie one after the other as for ai_aggregate_scans: float32 scan_xyz, HOST scan_off.  A point takes
 *      part iff it passes rules A1 and A2 of ai_aggregate_scans, with the same arguments and the same switches-off (one shared
 *      predicate, csrc/ai_keep.h): the reference segments dataset[i].point_cloud, which is already filtered.  A point that is not
 *      kept is absent: never sampled, never counted, never flagged.  m = the number of kept points of the scan, ranked in ascending
 *      input position.
 *   G2 Sampling.  Hypothesis h (0 <= h < n_hyp <= 4096) of the scan with key k = scan_base + s draws three distinct ranks in
 *      [0, m), all in uint64 arithmetic modulo 2^64.  Counter c = ((k*4096 + h)*4 + j); z = seed + (c+1)*0x9E3779B97F4A7C15;
 *      z ^= z>>30; z *= 0xBF58476D1CE4E5B9; z ^= z>>27; z *= 0x94D049BB133111EB; z ^= z>>31 (splitmix64's finaliser);
 *      draw(j, n) = ((z>>32) * n) >> 32.  r0 = draw(0, m); r1 = draw(1, m-1), incremented if r1 >= r0; r2 = draw(2, m-2), then for
 *      each of r0, r1 in ascending order incremented if r2 >= it.  Rank r names the r-th kept point.  A scan with m < 3 has no
 *      plane.  scan_base (>= 0, every key below 2^48) is an argument, so that a scan segmented alone with its own key gives what
 *      it gives inside a map.
 *   G3 Plane.  The three points are widened to float64.  e0 = p1-p0, e1 = p2-p0, n = e0 x e1 with each component as
 *      (a*b) - (c*d); len = the correctly rounded sqrt((nx*nx + ny*ny) + nz*nz).  The hypothesis is DEGENERATE unless len > 0 &&
 *      len < inf.  (a, b, c) = n / len, three divisions; d = -((a*x0 + b*y0) + c*z0).  Every step is rounded on its own (no
 *      contraction).  The normal's sign is whatever comes out.
 *   G4 Distance.  dist = |((a*x + b*y) + c*z) + d| on the widened coordinates, no contraction; a point is an inlier iff
 *      dist < distance_threshold: the comparison is strict, and NaN fails.
 *   G5 Choice.  A hypothesis' score is its inlier count over the scan's kept points; the best is the largest count, ties go to the
 *      smallest h; degenerate hypotheses never win; if all are degenerate, or m < 3, the scan has no plane.  The tie rule is ours:
 *      open3d breaks ties by an rmse and may stop early (`probability`); both depend on summation order or thread timing there
 *      and neither is reproduced.
 *   G6 Outputs.  ground_flag (uint8 per INPUT point, may not be NULL): 1 iff the point is kept and is an inlier of its scan's best
 *      plane by the expression of G4, so a scan's flags sum to its best count.  plane (n_scans x 4 float64): the best plane of
 *      G3, zeros when there is none; there is no refit (the reference discards the model).  best_hyp (int32, -1 when there is no
 *      plane) and best_count (int32, 0 then).  hyp_count (n_scans x n_hyp int32, may be NULL): every hypothesis' count, -1 for
 *      a degenerate one (all of them for a scan with m < 3).
 *   G7 Determinism, limits, errors.  Counts are integers summed with integer atomics: two calls are bit-identical.
 *      M = scan_off[n_scans] < 2^31 - 256; n_scans x n_hyp < 2^31.  AI_ERR_BAD_ARG: a distance_threshold that is not finite and
 *      positive; n_hyp outside 1 .. 4096; a negative scan_base (or a key of 2^48 and above); an offset array that does not start
 *      at 0 or decreases; the moving-object filter without label_word; range_min > range_max (or a NaN bound) while the range filter
 *      is on.  The arguments are checked in full before anything is written.  Not errors: no scans, empty scans, a scan with no plane.
 * scan_xyz, label_word and the five outputs are host or device per mem_kind; scan_off (n_scans + 1) is a HOST array.
 */
int ai_ground_planes(ai_ctx* ctx, const float* scan_xyz, const int64_t* scan_off, int32_t n_scans, const uint32_t* label_word,
                     int32_t moving_index, double range_min, double range_max, double distance_threshold, int32_t n_hyp,
                     uint64_t seed, int64_t scan_base, int mem_kind, uint8_t* ground_flag, double* plane, int32_t* best_hyp,
                     int32_t* best_count, int32_t* hyp_count);

/*
 * Hidden point removal of V views in one call: open3d 0.17 PointCloud::HiddenPointRemoval as hidden_point_removal_o3d calls it
 * (pipeline/utils/image/hidden_points_removal.py:6-25) inside image_based_features_per_patch (pipeline/utils/image/image_utils.py:
 * 155-204), without a hull: one linear program in two unknowns per point.  cloud_xyz: M points in the pcd
 * frame; subset (may be NULL: all M points, m = M): m rows of the cloud, the reference's bound_indices; T_pcd2cam: V transforms.
 *   H1 Transform.  Point j of the subset goes to the camera frame of view v by rule R1 of ai_scan_pool (fixed order, no
 *      contraction).  A last row of T other than (0, 0, 0, 1), or an entry that is not finite, is AI_ERR_BAD_ARG for the call.
 *   H2 Sphere.  D = sqrt((dx*dx + dy*dy) + dz*dz) of the extent of the view's points, R = radius_factor * D, S = (2R) * (2R).
 *      d_j = sqrt((x*x + y*y) + z*z); d_j == 0 counts as 1e-4 with direction 0 (the host function's rule).  e_j = p_j / d_j
 *      (three divisions), r_j = 2R - d_j, u_j = S / r_j.  The flipped point is r_j e_j; the origin is appended.
 *   H3 Constraint.  Point i is a vertex of the flipped hull iff some t in the plane orthogonal to e_i satisfies, for every j,
 *      t . w_ij <= g_ij with c = (ex_i*ex_j + ey_i*ey_j) + ez_i*ez_j -- exactly 1 when e_j equals e_i in all three components --
 *      w = e_j - c * e_i, g = u_j - c * u_i (4R^2 times 1/r_j - c/r_i).  In the basis a = (e_i x axis) / |e_i x axis|, axis the
 *      unit axis of the smallest |component| of e_i (the lower axis on a tie), b = e_i x a, the constraint reads
 *      t0 * A0 + t1 * A1 <= g with A0 = (wx*ax + wy*ay) + wz*az, A1 = (wx*bx + wy*by) + wz*bz.  Every product, sum, quotient and
 *      square root is rounded on its own.  The boundary is feasible: two equal points are both visible (0 <= 0), a point straight
 *      behind a nearer one is hidden (w = 0, g < 0).  The constraint of i itself is 0 <= 0.
 *   H4 Decision.  Seidel's incremental program over a list of constraints, from a start t: the first constraint k of the list,
 *      after the last one re-solved, with t0*A0 + t1*A1 > g is re-solved: nn = A0*A0 + A1*A1 (nn == 0: infeasible), f = (t.A - g)
 *      / nn, p = t - A * f, dir = (-A1, A0); every earlier constraint j of the list, and the four of the box |t_k| <= 1e12, gives
 *      den = A_j . dir, num = g_j - A_j . p; den > 0: hi = min(hi, num / den); den < 0: lo = max(lo, num / den); den == 0 and
 *      num < 0: infeasible.  lo > hi: infeasible.  Else t = p + min(max(0, lo), hi) * dir.  min and max are exact, so the order
 *      in which a re-solve visits the earlier constraints does not matter.
 *   H5 Lists.  The view's points are sorted (stable) by the cell of e_j in the fixed grid of 64^3 cells over [-1, 1]^3 (cell index
 *      min(max(floor((e + 1) * 32), 0), 63) per axis, key (cz * 64 + cy) * 64 + cx).  Local pass, from t = 0: the points of i's
 *      own cell, then of the 26 cells around it in (dz, dy, dx) order, each cell in sorted order; an infeasible list proves i
 *      hidden.  Global pass, from the local pass's t: all points in sorted order.  i is visible iff both lists are feasible.
 *      A point at the camera (d_i == 0 before the replacement) coincides with the appended origin and is not visible: this is
 *      this project's own rule (the reference's hull has the origin and such a point as one location and defines no flag for it).
 *      The global pass may pass over records that cannot be violated at its t (a proven bound): H4 does
 *      nothing at a constraint that is not violated, so the result is that of the plain scan bit for bit.
 *   H6 Skipped views.  Fewer than 4 points, R not positive (all points equal), S not finite, a coordinate that is not finite in
 *      the camera frame, or a sphere that does not hold the points (far >= 2R, far = sqrt((fx*fx + fy*fy) + fz*fz) of the largest
 *      |coordinate| per axis, so that every r_j of a computed view is positive; a small cloud far from the camera with a small
 *      radius_factor): status_out[v] = 1, the view's flags and count are not written, the call goes on (the reference's "hpr
 *      skip": open3d raises there).  status_out[v] = 0 for a computed view.
 * flags_out (V x m, one byte per point, 1 = visible) and count_out (V) depend on nothing but the view's own points: a view gives
 * the same bytes alone or among others.  stats_out (may be NULL): V x 4 -- points settled by the local pass, re-solves summed over
 * the points, the largest number of re-solves of one point, points at the camera.  AI_ERR_BAD_ARG: m or M outside [0, 2^30),
 * V < 0, a subset row outside [0, M), radius_factor not finite.  cloud_xyz, subset and flags_out are host or device per mem_kind;
 * T_pcd2cam (V x 16 row-major), count_out, status_out and stats_out are HOST arrays.
 */
int ai_hidden_points(ai_ctx* ctx, const double* cloud_xyz, int64_t n_cloud, const int32_t* subset, int64_t n_subset,
                     const double* T_pcd2cam, int32_t n_views, double radius_factor, int mem_kind, uint8_t* flags_out,
                     int64_t* count_out, int32_t* status_out, int64_t* stats_out);

/*
 * DBSCAN of n_clouds clouds in one call: sklearn.cluster.DBSCAN(eps, min_samples).fit(cloud).labels_ for every cloud, as
 * AggregationClustering.clusters_hdbscan / clusterize_pcd run it on the non-ground points (pipeline/utils/aggregate.py:253-327),
 * label for label.  xyz: the concatenated clouds, off[n_clouds] points; cloud c is rows off[c] .. off[c + 1]
 * and may be empty.  Indices below are rows of xyz.
 *   D1 Neighbour.  j is a neighbour of i iff both are in the same cloud and (dx*dx + dy*dy) + dz*dz <= eps*eps, every product
 *      and sum rounded on its own (no contraction), eps*eps rounded once, the test inclusive.  i is its own neighbour; points
 *      with equal coordinates count once each.
 *   D2 Core.  i is a core point iff it has at least min_samples neighbours.  count_out[i] = min(neighbours, min_samples): the
 *      count is saturated, the search stops where the answer is known.
 *   D3 Clusters.  The clusters are the connected components of the core points under D1.
 *   D4 Numbering.  Within a cloud the clusters are numbered 0, 1, ... in ascending order of their smallest core index.
 *   D5 Border and noise.  A point that is not core takes the smallest cluster number among its core neighbours; with no core
 *      neighbour its label is -1.  It joins one cluster and connects none.
 *   D6 Independence.  A cloud's outputs are the same bits whatever other clouds share the call, wherever its points lie and
 *      whatever cell size the search grid ended up with: they are a function of D1 on the cloud's own points alone.
 * labels (one int32 per point), n_clusters (one per cloud), count_out (may be NULL), sizes_out (may be NULL; as long as labels:
 * the size of cluster k of cloud c at off[c] + k, border points included, the rest of the cloud's stretch 0).  Sizes are integer
 * sums: two calls are bit-identical.  AI_ERR_BAD_ARG: eps (or eps*eps) not positive or not finite; min_samples < 1; off not
 * starting at 0 or decreasing; 2^30 points or more; a coordinate that is not finite.  No point at all (off[n_clouds] == 0) is not
 * an error: every n_clusters is 0.  xyz, labels, count_out and sizes_out are host or device per mem_kind; off (n_clouds + 1) and
 * n_clusters are HOST arrays.
 */
int ai_dbscan(ai_ctx* ctx, const double* xyz, const int64_t* off, int32_t n_clouds, double eps, int32_t min_samples,
              int mem_kind, int32_t* labels, int32_t* n_clusters, int32_t* count_out, int32_t* sizes_out);

/*
 * Timing hook for bench.py: runs `reps` fused Lanczos SpMV steps on the whole graph as
 * one segment and returns the average kernel time (HIP events on the context's stream)
 * plus the algorithmic byte count of one launch.
 */
int ai_bench_spmv(ai_ctx* ctx, const ai_csr* csr, int32_t reps, double* avg_ms, double* bytes_per_launch);

/*
 * Timing hook for bench.py: the box's plain stream rate.  `reps` device-to-device copies of `bytes` bytes (16 bytes per lane per
 * access, four accesses in flight per thread, every block its own contiguous range), timed with HIP events on the context's stream;
 * *gbps = read + written bytes per second / 1e9.  What a roofline fraction of an HBM-bound kernel is quoted beside.
 */
int ai_bench_copy(ai_ctx* ctx, int64_t bytes, int32_t reps, double* gbps);

#ifdef __cplusplus
}
#endif
#endif /* AUTOINST_HIP_H */
