// What the scorer sees of k label maps at once (rules S1-S5 of include/autoinst_hip.h): per row the contingency
// table with the ground truth, remove_semantics (pipeline/utils/point_cloud/point_cloud_utils.py:249-287) and filter_labels
// (pipeline/metrics/metrics_class.py:302-309) decided per label on the device, and the labels the two leave per point.
//
//   ks_count    -- pass 1: a block counts one tile of one row in an LDS table, then adds every occupied slot to the row's table in
//                  global memory with one 64-bit atomic.  A slot is claimed with the INDEX of a point that carries its pair, never
//                  with the pair itself: every 64-bit key is a legal pair, an index + 1 is never 0.  Whoever finds a slot taken
//                  compares its pair with the pair of the point named there -- data nobody writes -- so no claimant ever waits.
//   ks_compact  -- the occupied slots of every row, behind each other
//   ks_runs     -- the same for a row that went through the sort (sorted_pair_runs of ai_labels_shared.h, ai_label_pairs' path)
//   ks_fold     -- pass 2: per label of a row m and z from the row's sorted pairs, rules S2 and S3, the flags of its pairs
//   ks_points   -- pass 3: per point the flags of its label, by a search in the row's sorted pairs
// ai_label_scores (rules Q1-Q8) goes on from pass 2 with the kq_ kernels below: the scores of every row.
#include <cmath>
#include <cstring>

#include "ai_labels_shared.h"

#define KS_TILE 4096         // points of one row per block: far below 2^32, so a 32-bit LDS counter cannot overflow
#define KS_LDS_SLOTS 1024    // slots of the block's table
#define KS_LDS_PROBES 16     // a point that finds neither its pair nor a free slot in this many steps adds to the global table itself
#define KS_TABLE_MIN 8192    // slots of a row's first global table
#define KS_TABLE_MAX 131072  // slots of its second one; a row that outgrows it is sorted
#define KS_LOAD_DEN 2        // a table of C slots takes C / KS_LOAD_DEN distinct pairs
#define KS_MAX_ROWS 64

namespace {

__device__ __forceinline__ uint64_t ks_mix(uint64_t x) {  // splitmix64 finaliser
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// c more points of the pair (a, b), which point `idx` of the row carries.  owner[s] == 0: free, else 1 + the index of a point of the
// pair that holds slot s.  The row's distinct pairs are counted as slots are claimed; the claim that exceeds `limit`, or a walk
// round the whole table, marks the row as outgrown: its table is then dropped as a whole (the caller counts the row again from zeroed
// tables or sorts it), so that a half-added tile costs nothing.
__device__ __forceinline__ void ks_global_add(const int32_t* __restrict__ prow, const int32_t* __restrict__ gt, uint32_t* __restrict__ owner,
                                              unsigned long long* __restrict__ count, uint32_t cap, int32_t limit,
                                              int32_t* __restrict__ claimed, int32_t* __restrict__ outgrown, int64_t idx, int32_t a,
                                              int32_t b, unsigned long long c) {
  uint32_t s = (uint32_t)(ks_mix(pair_key(a, b)) >> 20) & (cap - 1);
  const uint32_t me = (uint32_t)idx + 1u;
  for (uint32_t probe = 0; probe < cap; ++probe, s = (s + 1) & (cap - 1)) {
    uint32_t o = atomicCAS(&owner[s], 0u, me);
    if (o == 0u) {
      if (atomicAdd(claimed, 1) >= limit) atomicExch(outgrown, 1);
      o = me;
    }
    if (o == me || (prow[o - 1] == a && gt[o - 1] == b)) {
      atomicAdd(&count[s], c);
      return;
    }
    if (ai_ld_agent(outgrown)) return;
  }
  atomicExch(outgrown, 1);
}

// grid (tiles, rows of this launch).  rows: the row of pred each blockIdx.y counts (null: itself)
__global__ __launch_bounds__(AI_BLOCK) void ks_count(const int32_t* __restrict__ pred, const int32_t* __restrict__ gt, int64_t n,
                                                     const int32_t* __restrict__ rows, uint32_t cap, uint32_t* __restrict__ owner,
                                                     unsigned long long* __restrict__ count, int32_t* __restrict__ claimed,
                                                     int32_t* __restrict__ outgrown) {
  __shared__ int32_t sp[KS_TILE], sg[KS_TILE];
  __shared__ uint32_t so[KS_LDS_SLOTS], sc[KS_LDS_SLOTS];
  const int r = blockIdx.y;
  const int t = rows ? rows[r] : r;
  const int64_t base = (int64_t)blockIdx.x * KS_TILE;
  const int m = (int)min((int64_t)KS_TILE, n - base);
  const int32_t* __restrict__ prow = pred + (int64_t)t * n;
  for (int q = threadIdx.x; q < KS_LDS_SLOTS; q += AI_BLOCK) so[q] = 0u, sc[q] = 0u;
  for (int q = threadIdx.x; q < m; q += AI_BLOCK) sp[q] = prow[base + q], sg[q] = gt[base + q];
  __syncthreads();
  uint32_t* go = owner + (size_t)r * cap;
  unsigned long long* gc = count + (size_t)r * cap;
  const int32_t limit = (int32_t)(cap / KS_LOAD_DEN);
  const int lane = threadIdx.x & 63;
  for (int q = threadIdx.x; q < KS_TILE; q += AI_BLOCK) {  // the same trip count for every lane: the wave votes below
    const bool live = q < m;
    const unsigned long long lives = __ballot(live);
    if (lives == 0ull) break;
    const int32_t a = live ? sp[q] : 0, b = live ? sg[q] : 0;
    // the lanes that carry the pair of the wave's first live lane are added by that lane alone (the ground's pair holds a large
    // share of a map: 64 adds to one LDS address would queue up)
    const int lead = __ffsll((long long)lives) - 1;
    const int32_t a0 = __shfl(a, lead, 64), b0 = __shfl(b, lead, 64);
    const bool same = live && a == a0 && b == b0;
    const unsigned long long sames = __ballot(same);
    if (!live || (same && lane != lead)) continue;
    const uint32_t c = same ? (uint32_t)__popcll(sames) : 1u;
    uint32_t s = (uint32_t)ks_mix(pair_key(a, b)) & (KS_LDS_SLOTS - 1);
    bool done = false;
    for (int probe = 0; probe < KS_LDS_PROBES; ++probe, s = (s + 1) & (KS_LDS_SLOTS - 1)) {
      uint32_t o = atomicCAS(&so[s], 0u, (uint32_t)q + 1u);
      if (o == 0u) o = (uint32_t)q + 1u;
      if (o == (uint32_t)q + 1u || (sp[o - 1] == a && sg[o - 1] == b)) {
        atomicAdd(&sc[s], c);
        done = true;
        break;
      }
    }
    if (!done && !ai_ld_agent(outgrown + r)) ks_global_add(prow, gt, go, gc, cap, limit, claimed + r, outgrown + r, base + q, a, b, c);
  }
  __syncthreads();
  if (ai_ld_agent(outgrown + r)) return;
  for (int s = threadIdx.x; s < KS_LDS_SLOTS; s += AI_BLOCK) {
    const uint32_t o = so[s];
    if (o) ks_global_add(prow, gt, go, gc, cap, limit, claimed + r, outgrown + r, base + o - 1, sp[o - 1], sg[o - 1], sc[s]);
  }
}

// grid (cap / AI_BLOCK, rows of this launch): an occupied slot of a row that fitted goes to the next free place of the row's segment
__global__ __launch_bounds__(AI_BLOCK) void ks_compact(const int32_t* __restrict__ pred, const int32_t* __restrict__ gt, int64_t n,
                                                       const int32_t* __restrict__ rows, uint32_t cap, const uint32_t* __restrict__ owner,
                                                       const unsigned long long* __restrict__ count, const int32_t* __restrict__ outgrown,
                                                       const int64_t* __restrict__ off, int32_t* __restrict__ fill,
                                                       uint64_t* __restrict__ ckey, unsigned long long* __restrict__ ccnt) {
  const int r = blockIdx.y;
  if (outgrown[r]) return;
  const int t = rows ? rows[r] : r;
  const size_t s = (size_t)r * cap + (size_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  const uint32_t o = owner[s];
  if (!o) return;
  const int64_t p = off[t] + atomicAdd(&fill[t], 1);
  ckey[p] = pair_key(pred[(int64_t)t * n + (o - 1)], gt[o - 1]);
  ccnt[p] = count[s];
}

// a sorted row: run j (sorted positions [i0, i1)) is pair j of the segment at `at`; ccnt there is zero before, its head subtracts i0
// and its last element adds i1
__global__ __launch_bounds__(AI_BLOCK) void ks_runs(const uint64_t* __restrict__ skey, const int32_t* __restrict__ pos, int64_t n, int64_t at,
                                                    uint64_t* __restrict__ ckey, unsigned long long* __restrict__ ccnt) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int64_t j = at + pos[i];
  if (pos[i + 1] != pos[i]) {
    ckey[j] = skey[i];
    atomicAdd(&ccnt[j], (unsigned long long)(-i));
  }
  // the element in front of a head closes the run before it; the last element closes the last run
  if (i + 1 == n) {
    atomicAdd(&ccnt[at + pos[n] - 1], (unsigned long long)n);
  } else if (pos[i + 2] != pos[i + 1]) {
    atomicAdd(&ccnt[at + pos[i + 1] - 1], (unsigned long long)(i + 1));
  }
}

__global__ __launch_bounds__(AI_BLOCK) void ks_iota(uint32_t* __restrict__ a, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < n) a[i] = (uint32_t)i;
}

__global__ __launch_bounds__(AI_BLOCK) void ks_row_keys(const uint32_t* __restrict__ idx, int64_t total, const int64_t* __restrict__ off,
                                                        int32_t k, uint32_t* __restrict__ rk) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i < total) rk[i] = (uint32_t)segment_of(off, k, (int64_t)idx[i]);
}

__global__ __launch_bounds__(AI_BLOCK) void ks_gather(const uint32_t* __restrict__ idx, int64_t total, const uint64_t* __restrict__ ckey,
                                                      const unsigned long long* __restrict__ ccnt, uint64_t* __restrict__ fkey,
                                                      int64_t* __restrict__ fcnt) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= total) return;
  fkey[i] = ckey[idx[i]];
  fcnt[i] = (int64_t)ccnt[idx[i]];
}

// one thread per pair; the first pair of a label walks the label's pairs: m = its points, z = those with gt == 0 (rule S2, S3)
__global__ __launch_bounds__(AI_BLOCK) void ks_fold(const uint64_t* __restrict__ fkey, const int64_t* __restrict__ fcnt, int64_t total,
                                                    const int64_t* __restrict__ off, int32_t k, double threshold, int64_t min_points,
                                                    int32_t* __restrict__ pa, int32_t* __restrict__ pb, uint8_t* __restrict__ flags,
                                                    int64_t* __restrict__ area) {  // area (may be null): m, for every pair of the label
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= total) return;
  const uint64_t key = fkey[i];
  const int32_t u = pair_key_a(key);
  pa[i] = u;
  pb[i] = pair_key_b(key);
  const int32_t t = segment_of(off, k, i);
  if (i > off[t] && pair_key_a(fkey[i - 1]) == u) return;
  const int64_t end = off[t + 1];
  int64_t m = 0, z = 0, j = i;
  for (; j < end && pair_key_a(fkey[j]) == u; ++j) {
    m += fcnt[j];
    if (pair_key_b(fkey[j]) == 0) z = fcnt[j];
  }
  const uint8_t f = (uint8_t)(((double)z > threshold * (double)m ? 1 : 0) | (m < min_points ? 2 : 0));
  for (int64_t q = i; q < j; ++q) flags[q] = f;
  if (area)
    for (int64_t q = i; q < j; ++q) area[q] = m;
}

// grid (points / AI_BLOCK, k): the first pair of the point's label in its row's sorted pairs carries the label's flags
__global__ __launch_bounds__(AI_BLOCK) void ks_points(const int32_t* __restrict__ pred, int64_t n, const int64_t* __restrict__ off,
                                                      const uint64_t* __restrict__ fkey, const uint8_t* __restrict__ flags,
                                                      int32_t* __restrict__ removed, int32_t* __restrict__ scored) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int t = blockIdx.y;
  const int32_t u = pred[(int64_t)t * n + i];
  const uint64_t want = pair_key(u, INT32_MIN);
  int64_t lo = off[t], hi = off[t + 1];  // the first position in [lo, hi) whose key is >= want: it exists and has the label u
  while (lo < hi) {
    const int64_t h = (lo + hi) >> 1;
    if (fkey[h] < want)
      lo = h + 1;
    else
      hi = h;
  }
  const uint8_t f = flags[lo];
  if (removed) removed[(int64_t)t * n + i] = (f & 1) ? 0 : u;
  if (scored) scored[(int64_t)t * n + i] = f ? 0 : u;
}

// ------------------------------------------------------------------ the instance-level scores (ai_label_scores, rules Q1-Q8)
// The scorer walks the stored pairs only: every overlap is above 0, so a pair that is not stored (count 0) is no candidate.
//   kq_col_keys -- the key of the column view: (row, gt) of every pair; one stable sort gives gt-major segments, pred ascending inside
//   kq_cols     -- the first pair of a gt segment walks it: ag (Q3), the segment of every pair, inner(v) / ag(v) of a kept v (Q7)
//   kq_rows     -- one wave per row: the column index of every gt != 0, the counts of Q6, outer and S (Q7) in gt order
//   kq_match    -- one wave per (overlap, row): Q4 per lane, the candidates by a ballot, Q5 over them in pair order
#define KQ_WAVE 64
#define KQ_TAKEN_LDS 2048    // distinct gt != 0 of a row whose taken-flags (one bit each) live in LDS; more: in global scratch
#define KQ_MAX_OVERLAPS 16
#define KQ_ROW_INTS 4        // per row: n_pred, distinct gt != 0, whether gt 0 occurs, kept gt

__device__ __forceinline__ bool kq_scored(int32_t u, uint8_t f, uint8_t mask) { return u != 0 && (f & mask) == 0; }

// Q4: one division
__device__ __forceinline__ double kq_iou(int64_t c, int64_t ap, int64_t ag) {
#pragma clang fp contract(off)
  const int64_t uni = ap + ag - c;
  return (double)c / (double)(uni > 1 ? uni : 1);
}

// Q7: inner + c * (c / (ag + ap - c)), every operation rounded on its own
__device__ __forceinline__ double kq_assoc_add(double inner, int64_t c, int64_t ap, int64_t ag) {
#pragma clang fp contract(off)
  const double q = (double)c / (double)(ag + ap - c);
  const double p = (double)c * q;
  return inner + p;
}

__global__ __launch_bounds__(AI_BLOCK) void kq_col_keys(const uint64_t* __restrict__ fkey, int64_t total, const int64_t* __restrict__ off,
                                                        int32_t k, uint64_t* __restrict__ ckey, uint32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= total) return;
  ckey[i] = ((uint64_t)(uint32_t)segment_of(off, k, i) << 32) | (fkey[i] & 0xffffffffull);  // the low word is gt in its sort form
  idx[i] = (uint32_t)i;
}

// one thread per position j of the column view (skey sorted, sidx[j] = the pair's place in the pred-major order).  The head of a
// segment of gt v != 0 writes ag and the head's position inside the row for every pair of the segment, and for the head itself
// whether v is kept and inner(v) / ag(v).  Segments of v == 0 are passed over: no score reads ag(0).
__global__ __launch_bounds__(AI_BLOCK) void kq_cols(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ sidx, int64_t total,
                                                    const int64_t* __restrict__ off, const uint64_t* __restrict__ fkey,
                                                    const int64_t* __restrict__ fcnt, const uint8_t* __restrict__ flags,
                                                    const int64_t* __restrict__ area, int64_t min_points, int64_t* __restrict__ ag,
                                                    int32_t* __restrict__ seg, double* __restrict__ term, uint8_t* __restrict__ kept) {
#pragma clang fp contract(off)
  const int64_t j = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (j >= total) return;
  const uint64_t key = skey[j];
  if (j > 0 && skey[j - 1] == key) return;
  const int32_t v = pair_key_b(key);
  if (v == 0) return;
  const int64_t row_start = off[(int32_t)(key >> 32)];
  int64_t a = 0, end = j;
  for (; end < total && skey[end] == key; ++end) a += fcnt[sidx[end]];
  double inner = 0.0;
  for (int64_t q = j; q < end; ++q) {
    const uint32_t i = sidx[q];
    ag[i] = a;
    seg[i] = (int32_t)(j - row_start);
    if (v > 0 && pair_key_a(fkey[i]) > 0 && !(flags[i] & 2)) inner = kq_assoc_add(inner, fcnt[i], area[i], a);
  }
  const bool keep = a > min_points;
  kept[j] = keep ? 1 : 0;
  term[j] = keep ? inner / (double)a : 0.0;
}

// grid k, one wave: the row's column view 64 positions at a time, then its pairs.  col[j] at the head of a segment of gt != 0: the
// number of such segments before it in the row.  The kept terms are added in gt order by the whole wave in step: the order is the result.
__global__ __launch_bounds__(KQ_WAVE) void kq_rows(const uint64_t* __restrict__ skey, const double* __restrict__ term,
                                                   const uint8_t* __restrict__ kept, const uint64_t* __restrict__ fkey,
                                                   const uint8_t* __restrict__ flags, const int64_t* __restrict__ off, uint8_t mask,
                                                   int32_t* __restrict__ col, int32_t* __restrict__ row_ints, double* __restrict__ s_assoc) {
#pragma clang fp contract(off)
  const int t = blockIdx.x, lane = threadIdx.x;
  const int64_t b = off[t], e = off[t + 1];
  const unsigned long long below = (1ull << lane) - 1ull;
  int32_t n_col = 0, n_kept = 0, has_zero = 0, n_pred = 0;
  double outer = 0.0;
  for (int64_t base = b; base < e; base += KQ_WAVE) {
    const int64_t j = base + lane;
    const bool live = j < e;
    const uint64_t key = live ? skey[j] : 0ull;
    const bool head = live && (j == b || skey[j - 1] != key);
    const bool nz = head && pair_key_b(key) != 0;
    const bool kp = nz && kept[j];
    const unsigned long long m_nz = __ballot(nz);
    unsigned long long m_kp = __ballot(kp);
    if (__ballot(head && !nz)) has_zero = 1;
    if (nz) col[j] = n_col + __popcll(m_nz & below);
    n_col += __popcll(m_nz);
    n_kept += __popcll(m_kp);
    const double x = kp ? term[j] : 0.0;
    while (m_kp) {
      const int src = __ffsll((long long)m_kp) - 1;
      m_kp &= m_kp - 1ull;
      outer = outer + __shfl(x, src, KQ_WAVE);
    }
  }
  for (int64_t base = b; base < e; base += KQ_WAVE) {
    const int64_t i = base + lane;
    const bool live = i < e;
    const int32_t u = live ? pair_key_a(fkey[i]) : 0;
    const bool head = live && kq_scored(u, flags[i], mask) && (i == b || pair_key_a(fkey[i - 1]) != u);
    n_pred += __popcll(__ballot(head));
  }
  if (lane == 0) {
    row_ints[t * KQ_ROW_INTS + 0] = n_pred;
    row_ints[t * KQ_ROW_INTS + 1] = n_col;
    row_ints[t * KQ_ROW_INTS + 2] = has_zero;
    row_ints[t * KQ_ROW_INTS + 3] = n_kept;
    s_assoc[t] = n_kept ? outer / (double)n_kept : __longlong_as_double(0x7ff8000000000000ll);
  }
}

// grid (n_overlaps, k), one wave.  Every lane holds the same `matched` (the rank of the last label that hit: it outlives a 64-pair
// read, so a label whose pairs span two reads is not matched twice) and sees the same taken-flags: all lanes load and store the same
// word, each in its own program order, so no lane reads a flag another lane has yet to write.  The flags of (row, overlap) are this
// wave's alone.  hits is zeroed before: a hit writes 1.
__global__ __launch_bounds__(KQ_WAVE) void kq_match(const uint64_t* __restrict__ fkey, const int64_t* __restrict__ fcnt,
                                                    const uint8_t* __restrict__ flags, const int64_t* __restrict__ area,
                                                    const int64_t* __restrict__ ag, const int32_t* __restrict__ seg,
                                                    const int32_t* __restrict__ col, const int64_t* __restrict__ off,
                                                    const int32_t* __restrict__ row_ints, const double* __restrict__ overlaps, uint8_t mask,
                                                    uint32_t* __restrict__ taken_global, const int64_t* __restrict__ taken_off,
                                                    uint8_t* __restrict__ hits, int32_t* __restrict__ tp) {
  __shared__ uint32_t taken_lds[KQ_TAKEN_LDS / 32];
  const int o = blockIdx.x, t = blockIdx.y, n_o = gridDim.x, lane = threadIdx.x;
  for (int w = lane; w < KQ_TAKEN_LDS / 32; w += KQ_WAVE) taken_lds[w] = 0u;
  __syncthreads();
  int64_t before = (lane < t) ? row_ints[lane * KQ_ROW_INTS] : 0;  // the scored labels of the rows before this one (k <= 64)
  for (int d = 32; d > 0; d >>= 1) before += __shfl_xor(before, d, KQ_WAVE);
  const int32_t n_pred = row_ints[t * KQ_ROW_INTS], n_col = row_ints[t * KQ_ROW_INTS + 1];
  const bool in_lds = n_col <= KQ_TAKEN_LDS;
  // a row that may need them (more than KQ_TAKEN_LDS pairs) has (pairs + 31) / 32 zeroed words per overlap at taken_off[t]
  uint32_t* taken = taken_global + taken_off[t] + (int64_t)o * ((taken_off[t + 1] - taken_off[t]) / n_o);
  uint8_t* my_hits = hits + before * n_o + (int64_t)o * n_pred;
  const double thr = overlaps[o];
  const int64_t b = off[t], e = off[t + 1];
  const unsigned long long upto = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);
  int32_t heads_before = 0, matched = -1, n_hit = 0;
  for (int64_t base = b; base < e; base += KQ_WAVE) {
    const int64_t i = base + lane;
    const bool live = i < e;
    const uint64_t key = live ? fkey[i] : 0ull;
    const int32_t u = pair_key_a(key), v = pair_key_b(key);
    const bool scored = live && kq_scored(u, flags[i], mask);
    const bool head = scored && (i == b || pair_key_a(fkey[i - 1]) != u);
    const unsigned long long m_head = __ballot(head);
    // the label of a scored pair is the last scored head at or before it: in this read, or the last one of the reads before
    const int32_t rank = heads_before + __popcll(m_head & upto) - 1;
    bool cand = false;
    int32_t c_col = 0;
    if (scored && v != 0 && kq_iou(fcnt[i], area[i], ag[i]) >= thr) {
      cand = true;
      c_col = col[b + seg[i]];
    }
    unsigned long long m_cand = __ballot(cand);
    while (m_cand) {
      const int src = __ffsll((long long)m_cand) - 1;
      m_cand &= m_cand - 1ull;
      const int32_t r = __shfl(rank, src, KQ_WAVE), cc = __shfl(c_col, src, KQ_WAVE);
      if (r == matched) continue;
      const uint32_t bit = 1u << (cc & 31);
      const uint32_t word = in_lds ? taken_lds[cc >> 5] : taken[cc >> 5];
      if (word & bit) continue;
      if (in_lds)
        taken_lds[cc >> 5] = word | bit;
      else
        taken[cc >> 5] = word | bit;
      matched = r;
      ++n_hit;
      if (lane == 0) my_hits[r] = 1;
    }
    heads_before += __popcll(m_head);
  }
  if (lane == 0) tp[t * n_o + o] = n_hit;
}

// one round of pass 1 over `nr` rows (rows: host list, null = rows 0 .. nr - 1) with tables of `cap` slots
struct CountRound {
  DevBuf<uint32_t> owner;
  DevBuf<unsigned long long> count;
  DevBuf<int32_t> state, d_rows;  // state: claimed[nr], then outgrown[nr]
  std::vector<int32_t> rows, h_state;
  uint32_t cap = 0;
  int nr = 0;
  const int32_t* rows_dev() const { return rows.empty() ? nullptr : d_rows.p; }
  int32_t* claimed() { return state.p; }
  int32_t* outgrown() { return state.p + nr; }
};

int count_round(hipStream_t st, const int32_t* dpred, const int32_t* dgt, int64_t n, uint32_t cap, CountRound& c) {
  c.cap = cap;
  const size_t slots = (size_t)c.nr * cap;
  AI_TRY(c.owner.alloc(slots));
  AI_TRY(c.count.alloc(slots));
  AI_TRY(c.state.alloc((size_t)2 * c.nr));
  if (!c.rows.empty()) AI_TRY(upload(c.rows, c.d_rows, st));
  AI_HIP(hipMemsetAsync(c.owner.p, 0, slots * sizeof(uint32_t), st));
  AI_HIP(hipMemsetAsync(c.count.p, 0, slots * sizeof(unsigned long long), st));
  AI_HIP(hipMemsetAsync(c.state.p, 0, (size_t)2 * c.nr * sizeof(int32_t), st));
  const unsigned tiles = (unsigned)((n + KS_TILE - 1) / KS_TILE);
  hipLaunchKernelGGL(ks_count, dim3(tiles, c.nr), dim3(AI_BLOCK), 0, st, dpred, dgt, n, c.rows_dev(), cap, c.owner.p, c.count.p, c.claimed(),
                     c.outgrown());
  AI_KERNEL_CHECK();
  c.h_state.resize((size_t)2 * c.nr);
  AI_HIP(hipMemcpyAsync(c.h_state.data(), c.state.p, (size_t)2 * c.nr * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  return AI_OK;
}

int compact_round(hipStream_t st, const int32_t* dpred, const int32_t* dgt, int64_t n, CountRound& c, const int64_t* d_off, int32_t* fill,
                  uint64_t* ckey, unsigned long long* ccnt) {
  hipLaunchKernelGGL(ks_compact, dim3(c.cap / AI_BLOCK, c.nr), dim3(AI_BLOCK), 0, st, dpred, dgt, n, c.rows_dev(), c.cap,
                     (const uint32_t*)c.owner.p, (const unsigned long long*)c.count.p, (const int32_t*)c.outgrown(), d_off, fill, ckey, ccnt);
  AI_KERNEL_CHECK();
  return AI_OK;
}

// What both entries share: the checks of rule S5, and everything of a call up to and including pass 2 -- the sorted pairs of every row
// behind each other on the device with their counts and flags.  Queued on the context's stream; the synchronisations are pass 1's.
int check_rows(const char* me, const ai_ctx* ctx, const int32_t* pred, const int32_t* gt, int32_t k, int64_t n, double threshold,
               int64_t min_points, int mem_kind) {
  if (!ctx || (mem_kind != AI_MEM_HOST && mem_kind != AI_MEM_DEVICE)) return bad_arg(me, "bad argument");
  if (k < 1 || k > KS_MAX_ROWS) return bad_arg(me, "between 1 and 64 rows are expected");
  if (n < 0 || n >= ((int64_t)1 << 31) - 1) return bad_arg(me, "n is negative or does not fit the int32 range of the scan");
  if (!std::isfinite(threshold) || threshold < 0.0) return bad_arg(me, "the threshold must be finite and >= 0");
  if (min_points < 0) return bad_arg(me, "min_points must be >= 0");
  if (n > 0 && (!pred || !gt)) return bad_arg(me, "null label array");
  return AI_OK;
}

struct RowTables {
  DevBuf<int32_t> own_p, own_g, d_pa, d_pb;
  const int32_t *dpred = nullptr, *dgt = nullptr;
  std::vector<int64_t> off;  // k + 1: row t is the pairs off[t] .. off[t + 1] - 1
  int64_t total = 0;
  DevBuf<int64_t> d_off, fcnt, area;  // area: m of the pair's label (only with_area)
  DevBuf<uint64_t> fkey;
  DevBuf<uint8_t> d_flags;
};

int row_tables(ai_ctx* ctx, const char* me, const int32_t* pred, const int32_t* gt, int32_t k, int64_t n, double threshold,
               int64_t min_points, int mem_kind, bool with_area, RowTables& T) {
  hipStream_t st = ctx->stream;
  AI_TRY(to_device(pred, (size_t)k * n, mem_kind, T.own_p, &T.dpred, st));
  AI_TRY(to_device(gt, (size_t)n, mem_kind, T.own_g, &T.dgt, st));
  const int32_t *dpred = T.dpred, *dgt = T.dgt;

  // pass 1: every row with the first table, the rows that outgrow it with the second one, the rows that outgrow that by sorting
  std::vector<int64_t> distinct((size_t)k, -1);
  CountRound first, second;
  first.nr = k;
  AI_TRY(count_round(st, dpred, dgt, n, KS_TABLE_MIN, first));  // synchronisation 1
  for (int32_t t = 0; t < k; ++t) {
    if (first.h_state[(size_t)k + t])
      second.rows.push_back(t);
    else
      distinct[t] = first.h_state[t];
  }
  std::vector<int32_t> sorted_rows;
  second.nr = (int)second.rows.size();
  if (second.nr > 0) {
    AI_TRY(count_round(st, dpred, dgt, n, KS_TABLE_MAX, second));  // synchronisation 2
    for (int r = 0; r < second.nr; ++r) {
      if (second.h_state[(size_t)second.nr + r])
        sorted_rows.push_back(second.rows[r]);
      else
        distinct[second.rows[r]] = second.h_state[r];
    }
  }
  PairRuns runs;
  if (!sorted_rows.empty()) {
    std::vector<int32_t> tot(sorted_rows.size(), 0);
    for (size_t r = 0; r < sorted_rows.size(); ++r) {
      AI_TRY(sorted_pair_runs(st, dpred + (int64_t)sorted_rows[r] * n, dgt, n, runs));
      AI_HIP(hipMemcpyAsync(&tot[r], runs.pos.p + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    AI_HIP(hipStreamSynchronize(st));  // synchronisation 3
    for (size_t r = 0; r < sorted_rows.size(); ++r) distinct[sorted_rows[r]] = tot[r];
  }
  std::vector<int64_t>& off = T.off;
  off.assign((size_t)k + 1, 0);
  for (int32_t t = 0; t < k; ++t) off[t + 1] = off[t] + distinct[t];
  const int64_t total = T.total = off[k];
  if (total >= ((int64_t)1 << 31) - 1) return bad_arg(me, "the rows have 2^31 - 1 or more distinct pairs together");

  // the pairs of all rows behind each other, then sorted inside every row
  DevBuf<int64_t>&d_off = T.d_off, &fcnt = T.fcnt;
  DevBuf<int32_t> fill, &d_pa = T.d_pa, &d_pb = T.d_pb;
  DevBuf<uint64_t> ckey, skey, &fkey = T.fkey;
  DevBuf<unsigned long long> ccnt;
  DevBuf<uint32_t> idx, sidx, rk, srk;
  DevBuf<uint8_t>& d_flags = T.d_flags;
  AI_TRY(upload(off, d_off, st));
  AI_TRY(fill.alloc(k));
  AI_TRY(ckey.alloc(total));
  AI_TRY(ccnt.alloc(total));
  AI_HIP(hipMemsetAsync(fill.p, 0, (size_t)k * sizeof(int32_t), st));
  AI_HIP(hipMemsetAsync(ccnt.p, 0, (size_t)total * sizeof(unsigned long long), st));
  AI_TRY(compact_round(st, dpred, dgt, n, first, d_off.p, fill.p, ckey.p, ccnt.p));
  if (second.nr > 0) AI_TRY(compact_round(st, dpred, dgt, n, second, d_off.p, fill.p, ckey.p, ccnt.p));
  for (size_t r = 0; r < sorted_rows.size(); ++r) {  // the sort a second time: its first run gave the size of the segment
    const int32_t t = sorted_rows[r];
    AI_TRY(sorted_pair_runs(st, dpred + (int64_t)t * n, dgt, n, runs));
    hipLaunchKernelGGL(ks_runs, dim3(grid_for(n)), dim3(AI_BLOCK), 0, st, (const uint64_t*)runs.skey.p, (const int32_t*)runs.pos.p, n, off[t],
                       ckey.p, ccnt.p);
    AI_KERNEL_CHECK();
  }
  AI_TRY(idx.alloc(total));
  AI_TRY(sidx.alloc(total));
  AI_TRY(skey.alloc(total));
  AI_TRY(fkey.alloc(total));
  AI_TRY(fcnt.alloc(total));
  AI_TRY(d_pa.alloc(total));
  AI_TRY(d_pb.alloc(total));
  AI_TRY(d_flags.alloc(total));
  if (with_area) AI_TRY(T.area.alloc(total));
  hipLaunchKernelGGL(ks_iota, dim3(grid_for(total)), dim3(AI_BLOCK), 0, st, idx.p, total);
  AI_KERNEL_CHECK();
  AI_TRY(sort_pairs(st, ckey.p, skey.p, idx.p, sidx.p, total, 64));
  const uint32_t* order = sidx.p;
  if (k > 1) {  // stable by the row: every row keeps its place, inside it the pairs ascend
    AI_TRY(rk.alloc(total));
    AI_TRY(srk.alloc(total));
    hipLaunchKernelGGL(ks_row_keys, dim3(grid_for(total)), dim3(AI_BLOCK), 0, st, (const uint32_t*)sidx.p, total, (const int64_t*)d_off.p, k,
                       rk.p);
    AI_KERNEL_CHECK();
    AI_TRY(sort_pairs(st, rk.p, srk.p, sidx.p, idx.p, total, bits_for(k)));
    order = idx.p;
  }
  hipLaunchKernelGGL(ks_gather, dim3(grid_for(total)), dim3(AI_BLOCK), 0, st, order, total, (const uint64_t*)ckey.p,
                     (const unsigned long long*)ccnt.p, fkey.p, fcnt.p);
  // pass 2
  hipLaunchKernelGGL(ks_fold, dim3(grid_for(total)), dim3(AI_BLOCK), 0, st, (const uint64_t*)fkey.p, (const int64_t*)fcnt.p, total,
                     (const int64_t*)d_off.p, k, threshold, min_points, d_pa.p, d_pb.p, d_flags.p,
                     with_area ? T.area.p : nullptr);
  AI_KERNEL_CHECK();
  return AI_OK;
}

}  // namespace

extern "C" int ai_label_tables(ai_ctx* ctx, const int32_t* pred, const int32_t* gt, int32_t k, int64_t n, double threshold,
                               int64_t min_points, int mem_kind, int64_t cap, int32_t* pair_pred, int32_t* pair_gt, int64_t* pair_count,
                               uint8_t* pair_flags, int64_t* row_off, int32_t* pred_removed, int32_t* pred_scored) {
  const char* me = "ai_label_tables";
  if (!row_off || cap < 0 || (cap > 0 && (!pair_pred || !pair_gt || !pair_count || !pair_flags))) return bad_arg(me, "bad argument");
  AI_TRY(check_rows(me, ctx, pred, gt, k, n, threshold, min_points, mem_kind));
  if (n == 0) {
    for (int32_t t = 0; t <= k; ++t) row_off[t] = 0;
    return AI_OK;
  }
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  RowTables T;
  AI_TRY(row_tables(ctx, me, pred, gt, k, n, threshold, min_points, mem_kind, false, T));
  // pass 3
  DevBuf<int32_t> own_r, own_s;
  int32_t *drem = nullptr, *dsco = nullptr;
  if (pred_removed) AI_TRY(dev_out(pred_removed, (size_t)k * n, mem_kind, own_r, &drem));
  if (pred_scored) AI_TRY(dev_out(pred_scored, (size_t)k * n, mem_kind, own_s, &dsco));
  if (drem || dsco) {
    hipLaunchKernelGGL(ks_points, dim3(grid_for(n), k), dim3(AI_BLOCK), 0, st, T.dpred, n, (const int64_t*)T.d_off.p,
                       (const uint64_t*)T.fkey.p, (const uint8_t*)T.d_flags.p, drem, dsco);
    AI_KERNEL_CHECK();
    if (mem_kind != AI_MEM_DEVICE) {
      AI_TRY(to_caller(pred_removed, (const int32_t*)drem, (size_t)k * n, mem_kind, st));
      AI_TRY(to_caller(pred_scored, (const int32_t*)dsco, (size_t)k * n, mem_kind, st));
    }
  }
  const int64_t m = std::min<int64_t>(T.total, cap);
  if (m > 0) {
    AI_HIP(hipMemcpyAsync(pair_pred, T.d_pa.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AI_HIP(hipMemcpyAsync(pair_gt, T.d_pb.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AI_HIP(hipMemcpyAsync(pair_count, T.fcnt.p, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    AI_HIP(hipMemcpyAsync(pair_flags, T.d_flags.p, (size_t)m * sizeof(uint8_t), hipMemcpyDeviceToHost, st));
  }
  AI_HIP(hipStreamSynchronize(st));  // the last synchronisation
  for (int32_t t = 0; t <= k; ++t) row_off[t] = T.off[t];
  return AI_OK;
}

extern "C" int ai_label_scores(ai_ctx* ctx, const int32_t* pred, const int32_t* gt, int32_t k, int64_t n, double threshold,
                               int64_t min_points, int mem_kind, int32_t remove, const double* overlaps, int32_t n_overlaps, int64_t cap,
                               uint8_t* hits, int64_t* hit_off, int32_t* row_counts, int32_t* tp, double* s_assoc) {
  const char* me = "ai_label_scores";
  if (!hit_off || !row_counts || !tp || !s_assoc || !overlaps || cap < 0 || (cap > 0 && !hits)) return bad_arg(me, "bad argument");
  AI_TRY(check_rows(me, ctx, pred, gt, k, n, threshold, min_points, mem_kind));
  if (n_overlaps < 1 || n_overlaps > KQ_MAX_OVERLAPS) return bad_arg(me, "between 1 and 16 overlaps are expected");
  for (int32_t o = 0; o < n_overlaps; ++o)
    if (!std::isfinite(overlaps[o]) || !(overlaps[o] > 0.0) || overlaps[o] > 1.0) return bad_arg(me, "every overlap must lie in (0, 1]");
  if (n == 0) {
    for (int32_t t = 0; t <= k; ++t) hit_off[t] = 0;
    std::fill(row_counts, row_counts + (size_t)3 * k, 0);
    std::fill(tp, tp + (size_t)k * n_overlaps, 0);
    std::fill(s_assoc, s_assoc + k, std::nan(""));
    return AI_OK;
  }
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  RowTables T;
  AI_TRY(row_tables(ctx, me, pred, gt, k, n, threshold, min_points, mem_kind, true, T));
  const int64_t total = T.total;
  const uint8_t mask = remove ? 3 : 2;

  // the column view: the pairs by (row, gt), pred ascending inside a gt
  DevBuf<uint64_t> ckey, skey;
  DevBuf<uint32_t> idx, sidx, taken;
  DevBuf<int64_t> d_ag, d_taken_off;
  DevBuf<int32_t> d_seg, d_col, d_ints, d_tp;
  DevBuf<double> d_term, d_s, d_overlaps;
  DevBuf<uint8_t> d_kept, d_hits;
  AI_TRY(ckey.alloc(total));
  AI_TRY(skey.alloc(total));
  AI_TRY(idx.alloc(total));
  AI_TRY(sidx.alloc(total));
  AI_TRY(d_ag.alloc(total));
  AI_TRY(d_seg.alloc(total));
  AI_TRY(d_col.alloc(total));
  AI_TRY(d_term.alloc(total));
  AI_TRY(d_kept.alloc(total));
  AI_TRY(d_ints.alloc((size_t)k * KQ_ROW_INTS));
  AI_TRY(d_tp.alloc((size_t)k * n_overlaps));
  AI_TRY(d_s.alloc(k));
  AI_TRY(d_hits.alloc((size_t)total * n_overlaps));  // a row has no more scored labels than pairs
  std::vector<double> h_overlaps(overlaps, overlaps + n_overlaps);
  AI_TRY(upload(h_overlaps, d_overlaps, st));
  std::vector<int64_t> taken_off((size_t)k + 1, 0);  // in words: rows whose distinct gt may outgrow the LDS flags
  for (int32_t t = 0; t < k; ++t) {
    const int64_t pairs = T.off[t + 1] - T.off[t];
    taken_off[t + 1] = taken_off[t] + (pairs > KQ_TAKEN_LDS ? (pairs + 31) / 32 * n_overlaps : 0);
  }
  AI_TRY(upload(taken_off, d_taken_off, st));
  AI_TRY(taken.alloc((size_t)taken_off[k]));
  if (taken_off[k] > 0) AI_HIP(hipMemsetAsync(taken.p, 0, (size_t)taken_off[k] * sizeof(uint32_t), st));
  AI_HIP(hipMemsetAsync(d_hits.p, 0, (size_t)total * n_overlaps, st));
  hipLaunchKernelGGL(kq_col_keys, dim3(grid_for(total)), dim3(AI_BLOCK), 0, st, (const uint64_t*)T.fkey.p, total, (const int64_t*)T.d_off.p, k,
                     ckey.p, idx.p);
  AI_KERNEL_CHECK();
  AI_TRY(sort_pairs(st, ckey.p, skey.p, idx.p, sidx.p, total, 32 + bits_for(k)));
  hipLaunchKernelGGL(kq_cols, dim3(grid_for(total)), dim3(AI_BLOCK), 0, st, (const uint64_t*)skey.p, (const uint32_t*)sidx.p, total,
                     (const int64_t*)T.d_off.p, (const uint64_t*)T.fkey.p, (const int64_t*)T.fcnt.p, (const uint8_t*)T.d_flags.p,
                     (const int64_t*)T.area.p, min_points, d_ag.p, d_seg.p, d_term.p, d_kept.p);
  AI_KERNEL_CHECK();
  hipLaunchKernelGGL(kq_rows, dim3(k), dim3(KQ_WAVE), 0, st, (const uint64_t*)skey.p, (const double*)d_term.p, (const uint8_t*)d_kept.p,
                     (const uint64_t*)T.fkey.p, (const uint8_t*)T.d_flags.p, (const int64_t*)T.d_off.p, mask, d_col.p, d_ints.p, d_s.p);
  AI_KERNEL_CHECK();
  hipLaunchKernelGGL(kq_match, dim3(n_overlaps, k), dim3(KQ_WAVE), 0, st, (const uint64_t*)T.fkey.p, (const int64_t*)T.fcnt.p,
                     (const uint8_t*)T.d_flags.p, (const int64_t*)T.area.p, (const int64_t*)d_ag.p, (const int32_t*)d_seg.p,
                     (const int32_t*)d_col.p, (const int64_t*)T.d_off.p, (const int32_t*)d_ints.p, (const double*)d_overlaps.p, mask, taken.p,
                     (const int64_t*)d_taken_off.p, d_hits.p, d_tp.p);
  AI_KERNEL_CHECK();
  std::vector<int32_t> ints((size_t)k * KQ_ROW_INTS);
  AI_HIP(hipMemcpyAsync(ints.data(), d_ints.p, ints.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipMemcpyAsync(tp, d_tp.p, (size_t)k * n_overlaps * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  AI_HIP(hipMemcpyAsync(s_assoc, d_s.p, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));  // the per-row results: the last synchronisation of ai_label_tables
  hit_off[0] = 0;
  for (int32_t t = 0; t < k; ++t) {
    for (int q = 0; q < 3; ++q) row_counts[(size_t)3 * t + q] = ints[(size_t)t * KQ_ROW_INTS + q];
    hit_off[t + 1] = hit_off[t] + ints[(size_t)t * KQ_ROW_INTS];
  }
  const int64_t m = std::min<int64_t>(hit_off[k] * n_overlaps, cap);
  if (m > 0) {
    AI_HIP(hipMemcpyAsync(hits, d_hits.p, (size_t)m, hipMemcpyDeviceToHost, st));
    AI_HIP(hipStreamSynchronize(st));  // the one more: the hit bytes, whose number the device counted
  }
  return AI_OK;
}
