// Host-only part of the asynchronous frontier (class Flow in ai_flow.inc): the records of its segments and groups, the allocator of
// its stable task indices, the map of its pinned host area with the layouts of the three tables a harvest wave keeps there, and the
// rules that turn a harvested segment into children and groups.  Nothing here needs HIP: g++ -std=c++17 compiles the header on its
// own, and tests/test_host_flow.py runs it under the address and undefined-behaviour sanitizers.
// Everything has internal linkage.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <iterator>
#include <map>
#include <vector>

#include "ai_ncut_params.h"

namespace {

struct RangeAlloc {  // first-fit allocator of index ranges (stable task indices)
  std::map<int, int> fr;  // start -> length
  void init(int cap) {
    fr.clear();
    fr[0] = cap;
  }
  int alloc(int n) {
    for (auto it = fr.begin(); it != fr.end(); ++it)
      if (it->second >= n) {
        const int b = it->first, len = it->second;
        fr.erase(it);
        if (len > n) fr[b + n] = len - n;
        return b;
      }
    return -1;
  }
  void release(int b, int n) {
    auto it = fr.emplace(b, n).first;
    auto nx = std::next(it);
    if (nx != fr.end() && it->first + it->second == nx->first) {
      it->second += nx->second;
      fr.erase(nx);
    }
    if (it != fr.begin()) {
      auto pv = std::prev(it);
      if (pv->first + pv->second == it->first) {
        pv->second += it->second;
        fr.erase(it);
      }
    }
  }
};

struct FSeg {  // host record of a live segment
  int g0 = 0, n = 0, chunk = 0, par = 0;
  int slot = -1;          // Lanczos state (pool segments only)
  int t0 = 0, cap = 0;
  int f0 = -1, c0 = -1;   // stable fine / coarse index ranges (pool segments only)
  int m = 0;              // size of T at freeze
  int aux = 0;            // index in the list the record was derived from
  bool frozen = false;
  bool binary_child = false;  // child of a Fiedler cut (or a root): its connectivity is not known yet
  int vdelta = 0;             // slab row of position 0 of its chunk
  int warm_n = 0;             // (warm start) rows of the last SOLVED ancestor, whose second Ritz vector lies at this segment's positions in warm[]; 0: none
  int pca = 0;                // (principal-axis start) 1 + chunk while the segment is prepared without a solved ancestor and its graph kept its points; 0: not
  int restarts = 0;           // times the segment was solved again because its Ritz pair failed the true-residual test
  double prev_true = 0.0;     // the true residual that sent it back
  // cut tree (ai_ncut_tree): the threshold at which the boundary in front of the segment's first position appears, and the largest
  // cost among the cuts that produced the segment (a Fiedler cut costs its mcut, a split into components exactly 0); -inf at a root
  double front = -INFINITY, path = -INFINITY;
  void detach() { slot = f0 = c0 = -1; }  // it holds nothing of the pool (any more)
};

struct FLeaf {  // a group: where it starts, the height of the boundary in front of it, the mcut of the cut it was refused (NaN: never solved)
  int32_t g0;
  double front, cost;
};

static inline int fk_nf(int n) { return (n + AI_FINE_ROWS - 1) / AI_FINE_ROWS; }
static inline int fk_nc(int n) { return (n + AI_COARSE_ROWS - 1) / AI_COARSE_ROWS; }

// ------------------------------------------------------------------------------------------------- the pinned host area
// One allocation per context (ai_ctx::fpin), four regions back to back after the upload area:
//   up      PIN_UP      first half: the wave's stage area; second half: ring of pool record tables
//   status  PIN_STATUS  status[slot]: rows of T at which the device froze the slot's segment
//   res     PIN_RES     the named places below
//   hist    PIN_HIST    the wave's packed histories (HistRows); after the helper thread has read them, the component table
//   coef    PIN_COEF    the wave's Ritz coefficients (CoefTable)
constexpr size_t UPSLOT_BYTES = (size_t)256 << 10;
constexpr size_t PIN_UP = AI_FLOW_UPSLOTS * UPSLOT_BYTES;  // 8 MB
constexpr size_t STATUS_BYTES = (size_t)64 << 10;
constexpr size_t PIN_STATUS = STATUS_BYTES;
constexpr size_t PIN_RES = (size_t)1 << 20;
constexpr size_t PIN_HIST = (size_t)16 << 20;
constexpr size_t PIN_COEF = (size_t)8 << 20;
constexpr size_t PIN_TOTAL = PIN_UP + PIN_STATUS + PIN_RES + PIN_HIST + PIN_COEF;
constexpr size_t PIN_OFF_STATUS = PIN_UP;
constexpr size_t PIN_OFF_RES = PIN_OFF_STATUS + PIN_STATUS;
constexpr size_t PIN_OFF_HIST = PIN_OFF_RES + PIN_RES;
constexpr size_t PIN_OFF_COEF = PIN_OFF_HIST + PIN_HIST;

// the result region, by byte offset
constexpr size_t RES_COMP_TOTAL = 0;        // int32: components in the disconnected segments of a wave (total of start_wave's scan)
constexpr size_t RES_PROGRESS = 32;         // int32: the last Lanczos step whose update kernel has started (fk_update)
// The wave table.  Two tenants alternate here: stage 2 writes WaveResults (fk_sweep_final, fk_resid_final, the helper thread) and
// stage 3 reads it on the host BEFORE it launches anything; stage 3's fk_reset_slots then writes the children's component counts
// (int32 per child), which wave_finish reads; the next stage 2 is launched only after wave_finish.  One wave is in flight at a time,
// so each tenant is consumed before the other writes.
constexpr size_t RES_WAVE = 64;
constexpr size_t RES_SLAB_TABLE = PIN_RES / 2;   // double*[]: the Lanczos slabs (appended to, uploaded by sync_slabtab)
constexpr int WAVE_MAX_SEGS = 512;               // frozen segments one wave harvests at the most

static inline int32_t* res_comp_total(char* res) { return (int32_t*)(res + RES_COMP_TOTAL); }
static inline volatile int32_t* res_progress(char* res) { return (volatile int32_t*)(res + RES_PROGRESS); }
static inline char* res_wave(char* res) { return res + RES_WAVE; }
static inline int32_t* res_child_comps(char* res) { return (int32_t*)(res + RES_WAVE); }
static inline double** res_slab_table(char* res) { return (double**)(res + RES_SLAB_TABLE); }
// children one wave may prepare: their component counts end below the slab table
static inline bool res_child_comps_fit(size_t nchildren) { return RES_WAVE + nchildren * sizeof(int32_t) <= RES_SLAB_TABLE; }

// Results of a wave's nA harvested segments at res_wave(): {split[nA], ntrue[nA], kstar[nA]} as int32, padded to 16 bytes, then
// {mcut[nA], resid[nA], rtrue[nA]} as double.
struct WaveResults {
  size_t nA;
  constexpr explicit WaveResults(size_t nA_) : nA(nA_) {}
  constexpr size_t int_bytes() const { return ((size_t)3 * nA * sizeof(int32_t) + 15) & ~(size_t)15; }
  constexpr size_t bytes() const { return int_bytes() + (size_t)3 * nA * sizeof(double); }
  int32_t* split(char* base) const { return (int32_t*)base; }
  int32_t* ntrue(char* base) const { return split(base) + nA; }
  int32_t* kstar(char* base) const { return split(base) + 2 * nA; }
  double* mcut(char* base) const { return (double*)(base + int_bytes()); }
  double* resid(char* base) const { return mcut(base) + nA; }    // the device's estimate, copied from the history row
  double* rtrue(char* base) const { return mcut(base) + 2 * nA; }  // fk_resid_final: ||M ev - theta ev|| / ||ev||
};
static_assert(RES_WAVE + WaveResults(WAVE_MAX_SEGS).bytes() <= RES_SLAB_TABLE, "a full wave's result table ends below the slab table");

// Packed histories of a wave (fk_pack_hist): one row of pitch() doubles per harvested segment,
// {theta, resid, m, checksum, a[mp], b[mp], g[mp]}, mp = the largest size of T in the wave.
#define FK_HIST_HEAD 4   // doubles in front of a packed history row: theta, resid, m, checksum (fk_pack_hist)
struct HistRows {
  size_t mp;
  constexpr explicit HistRows(size_t mp_) : mp(mp_) {}
  constexpr size_t pitch() const { return (size_t)3 * mp + FK_HIST_HEAD; }
  constexpr size_t doubles(size_t rows) const { return rows * pitch(); }
  constexpr size_t bytes(size_t rows) const { return doubles(rows) * sizeof(double); }
  const double* row(const double* base, size_t i) const { return base + i * pitch(); }
  static double theta(const double* row) { return row[0]; }
  static double resid(const double* row) { return row[1]; }
  static double m_dev(const double* row) { return row[2]; }   // the DEVICE's size of T
  const double* a(const double* row) const { return row + FK_HIST_HEAD; }
  const double* b(const double* row) const { return a(row) + mp; }
  const double* g(const double* row) const { return b(row) + mp; }
  // the header checks of a row whose segment the host knows to have m rows of T: the device froze it at that size, and the sum of
  // the 64-bit patterns of theta, resid, a / b / g[0..m) and m is the row's fourth word (integer addition: any order)
  static bool m_matches(const double* row, int m) { return row[2] == (double)m; }
  bool sum_matches(const double* row, int m) const {
    auto bits = [](double v) {
      unsigned long long u;
      memcpy(&u, &v, sizeof u);
      return u;
    };
    unsigned long long sum = bits(row[0]) + bits(row[1]) + (unsigned long long)(long long)m;
    const double *av = a(row), *bv = b(row), *gv = g(row);
    for (int j = 0; j < m; ++j) sum += bits(av[j]) + bits(bv[j]) + bits(gv[j]);
    return bits(row[3]) == sum;
  }
  bool accepts(const double* row, int m) const { return m_matches(row, m) && sum_matches(row, m); }
};

// The component table of a wave's disconnected segments borrows the history region when it fits (the helper thread has read the
// histories by then): {troot[n], tsize[n]} as int32, first row and size of every component, by first row.
struct CompTable {
  size_t n;
  constexpr explicit CompTable(size_t n_) : n(n_) {}
  constexpr size_t bytes() const { return (size_t)2 * n * sizeof(int32_t); }
  constexpr bool fits_pinned() const { return bytes() <= PIN_HIST; }
  int32_t* troot(char* base) const { return (int32_t*)base; }
  int32_t* tsize(char* base) const { return (int32_t*)base + n; }
};

// Ritz coefficients of a wave, in doubles from a base that is the pinned host copy, the device copy or the guard log's copy:
// {cu[nA], theta[nA], m[nA] (int32 in a row of nA doubles), coef[nA][mp]} and, on the warm path, {cu2[nA], coef2[nA][mp]}.
struct CoefTable {
  size_t nA, mp;
  bool warm;
  constexpr CoefTable(size_t nA_, size_t mp_, bool warm_) : nA(nA_), mp(mp_), warm(warm_) {}
  static constexpr size_t head_doubles(size_t rows) { return 4 * rows; }   // the rows cu, theta, m, cu2
  constexpr size_t top_doubles() const { return 3 * nA + nA * mp; }        // the first vector's part
  constexpr size_t doubles() const { return top_doubles() + (warm ? nA + nA * mp : 0); }
  constexpr size_t bytes() const { return doubles() * sizeof(double); }
  // what a wave reserves: the four header rows whether or not it computes the second vector
  constexpr size_t reserved_bytes() const { return (head_doubles(nA) + (warm ? 2 : 1) * nA * mp) * sizeof(double); }
  template <typename D> D* cu(D* base) const { return base; }
  template <typename D> D* theta(D* base) const { return base + nA; }
  const int32_t* m(const double* base) const { return (const int32_t*)(base + 2 * nA); }
  int32_t* m(double* base) const { return (int32_t*)(base + 2 * nA); }
  template <typename D> D* coef(D* base, size_t i = 0) const { return base + 3 * nA + i * mp; }
  template <typename D> D* cu2(D* base) const { return base + top_doubles(); }
  template <typename D> D* coef2(D* base, size_t i = 0) const { return base + top_doubles() + nA + i * mp; }
};
static_assert(HistRows(4000).bytes(1) <= PIN_HIST && CoefTable(1, 4000, true).reserved_bytes() <= PIN_COEF,
              "one row of mcap = 4000 fits the pinned history and coefficient buffers");

// a wave of k segments whose largest T has mp rows fits the pinned buffers
static inline bool wave_fits(size_t k, size_t mp, bool warm) {
  return HistRows(mp).bytes(k) <= PIN_HIST && CoefTable(k, mp, warm).reserved_bytes() <= PIN_COEF;
}
// doubles of the device copy: an upload is at most PIN_COEF bytes; the header rows of a full wave and 64 doubles of slack behind it
constexpr size_t COEF_DEV_DOUBLES = PIN_COEF / sizeof(double) + CoefTable::head_doubles(WAVE_MAX_SEGS) + 64;

// ------------------------------------------------------------------------------------------------- what a harvested segment becomes
// A child of a harvested segment continues only if it may be split at all (normalized_cut.py:39-40 with the recursion's 1 %);
// otherwise it is a group that was never solved (cost NaN).  Heights of the cut tree: DESIGN.md section 21.
constexpr double CHILD_SPLIT_LIM = 0.01;

// The Ritz pair failed the true-residual test: the segment is solved again from scratch, like a connected child that joins the pool.
static inline void child_solve_again(const FSeg& s, double rtrue, std::vector<FSeg>& children) {
  FSeg ch;
  ch.g0 = s.g0;
  ch.n = s.n;
  ch.chunk = s.chunk;
  ch.par = s.par;       // not split: its graph stays where it is
  ch.vdelta = s.vdelta;
  ch.binary_child = false;
  ch.restarts = s.restarts + 1;
  ch.prev_true = rtrue;
  ch.warm_n = s.warm_n;   // (its own harvest wrote ev2 only: warm[] at its rows is still its ancestor's)
  ch.front = s.front;
  ch.path = s.path;
  children.push_back(ch);
}

// A Fiedler cut of s into its first ntrue positions (A) and the rest (B), at cost mcut.
struct CutSides {
  bool ok;            // false: an empty side (na / nb say which); nothing was appended
  int na, nb;
  bool contA, contB;  // the side continues (else it was appended to the leaves)
};
static inline CutSides children_of_cut(const FSeg& s, int ntrue, double mcut, int64_t n_orig, std::vector<FSeg>& children, std::vector<FLeaf>& leaves) {
  CutSides r{false, ntrue, s.n - ntrue, false, false};
  if (r.na <= 0 || r.nb <= 0) return r;
  r.ok = true;
  r.contA = eligible(r.na, n_orig, CHILD_SPLIT_LIM);
  r.contB = eligible(r.nb, n_orig, CHILD_SPLIT_LIM);
  FSeg ch;
  ch.chunk = s.chunk;
  ch.par = s.par ^ 1;
  ch.vdelta = s.vdelta;
  ch.binary_child = true;
  ch.warm_n = s.n;   // the children start from this segment's second Ritz vector (fk_partition carries it to their rows)
  ch.path = std::max(s.path, mcut);  // the boundary between the two sides appears once this cut and all its ancestors do
  if (r.contA) {
    ch.g0 = s.g0;
    ch.n = r.na;
    ch.front = s.front;
    children.push_back(ch);
  } else {
    leaves.push_back(FLeaf{s.g0, s.front, NAN});
  }
  if (r.contB) {
    ch.g0 = s.g0 + r.na;
    ch.n = r.nb;
    ch.front = ch.path;
    children.push_back(ch);
  } else {
    leaves.push_back(FLeaf{s.g0 + r.na, ch.path, NAN});
  }
  return r;
}

// The components of the disconnected segment s: its run of the wave's component table {troot, tsize}[nt] starts at ti (first row and
// size of each component, by first row) and ends where a component starts behind the segment; ti is advanced past it.
// cont[t] = 1 for every component that continues (the others were appended to the leaves).
enum CompStatus { COMP_OK = 0, COMP_NO_TILE, COMP_SHORT };   // a component outside the segment / its rows are not all covered
struct CompSplit {
  CompStatus status;
  int covered;   // rows of the segment the components cover
};
static inline CompSplit children_of_components(const FSeg& s, const int32_t* troot, const int32_t* tsize, size_t nt, size_t& ti, int64_t n_orig, int32_t* cont,
                                               std::vector<FSeg>& children, std::vector<FLeaf>& leaves) {
  int offp = 0;
  const double pcomp = std::max(s.path, 0.0);  // the cut between whole components costs exactly 0
  while (ti < nt && troot[ti] < s.g0 + s.n) {
    const int nc = tsize[ti];
    if (troot[ti] < s.g0 || nc <= 0 || offp + nc > s.n) return CompSplit{COMP_NO_TILE, offp};
    if (eligible(nc, n_orig, CHILD_SPLIT_LIM)) {
      FSeg ch;
      ch.chunk = s.chunk;
      ch.par = s.par ^ 1;
      ch.vdelta = s.vdelta;
      ch.g0 = s.g0 + offp;
      ch.n = nc;
      ch.warm_n = s.warm_n;     // inherited: the last solved ancestor's vector, carried through this split as well
      ch.binary_child = false;  // connected by construction
      ch.front = offp ? pcomp : s.front;
      ch.path = pcomp;
      children.push_back(ch);
      cont[ti] = 1;
    } else {
      leaves.push_back(FLeaf{s.g0 + offp, offp ? pcomp : s.front, NAN});
    }
    offp += nc;
    ++ti;
  }
  return CompSplit{offp == s.n ? COMP_OK : COMP_SHORT, offp};
}

}  // namespace
