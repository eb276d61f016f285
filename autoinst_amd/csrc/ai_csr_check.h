// The contract of a caller-built CSR (ai_csr_from_host): the checks that run on the host.  Plain C++ without HIP, so that a small
// stand-alone program can run them under the host sanitizers.
//
// A graph passes when every stored value is finite and > 0, no (row, col) is stored twice, and every entry (i, j) has a mirror
// (j, i) with the same bits.  Column order within a row, the diagonal and empty rows are the caller's business.  Why each rule:
// DESIGN.md, "The caller's CSR at the door".
#pragma once
#include <cfloat>
#include <cmath>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <utility>
#include <vector>

namespace ai_csr_check {

// position of column c in the ascending run col[s, e), or -1
inline int64_t find_col(const int32_t* col, int64_t s, int64_t e, int32_t c) {
  const int32_t* p = std::lower_bound(col + s, col + e, c);
  return (p != col + e && *p == c) ? (int64_t)(p - col) : -1;
}

inline bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

// Everywhere below: rp = n + 1 checked row pointers (rp[0] = 0, non-decreasing), col checked to lie in [0, n).  A function returns
// true when the graph keeps its rule; otherwise it writes a message that names the first offending row and column into msg and
// returns false.  "First" is the first stored entry for the rules on single values, the lowest row and then the lowest column for
// duplicates and mirrors.

// Every value finite and > 0.  *ascending: every row's columns ascend strictly as stored (such a row holds no duplicate).
inline bool values(int64_t n, const int32_t* rp, const int32_t* col, const double* val, bool* ascending, char* msg, size_t msg_len) {
  bool asc = true;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t s = rp[i], e = rp[i + 1];
    bool bad = false;
    for (int64_t k = s; k < e; ++k) bad |= !(val[k] > 0.0) | !(val[k] <= DBL_MAX);
    for (int64_t k = s + 1; k < e; ++k) asc &= col[k] > col[k - 1];
    if (!bad) continue;
    for (int64_t k = s; k < e; ++k) {
      const double v = val[k];
      if (v > 0.0 && v <= DBL_MAX) continue;
      const char* what = !std::isfinite(v) ? "is not finite" : (v < 0.0 ? "is negative" : "is a stored zero");
      snprintf(msg, msg_len, "ai_csr_from_host: the value %g at row %lld, column %d %s", v, (long long)i, col[k], what);
      return false;
    }
  }
  *ascending = asc;
  return true;
}

// A copy with every row sorted by column, for rows stored in another order; no (row, col) twice.
inline bool by_column(int64_t n, const int32_t* rp, const int32_t* col, const double* val, std::vector<int32_t>& scol,
                      std::vector<double>& sval, char* msg, size_t msg_len) {
  const int64_t nnz = rp[n];
  scol.assign(col, col + nnz);
  sval.assign(val, val + nnz);
  std::vector<std::pair<int32_t, double>> row;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t s = rp[i], e = rp[i + 1];
    bool asc = true;
    for (int64_t k = s + 1; k < e && asc; ++k) asc = scol[(size_t)k] > scol[(size_t)k - 1];
    if (asc) continue;
    row.resize((size_t)(e - s));
    for (int64_t k = s; k < e; ++k) row[(size_t)(k - s)] = {scol[(size_t)k], sval[(size_t)k]};
    std::sort(row.begin(), row.end());
    for (int64_t k = s; k < e; ++k) {
      scol[(size_t)k] = row[(size_t)(k - s)].first;
      sval[(size_t)k] = row[(size_t)(k - s)].second;
      if (k > s && scol[(size_t)k] == scol[(size_t)k - 1]) {
        snprintf(msg, msg_len, "ai_csr_from_host: row %lld stores column %d twice (duplicates are not summed)", (long long)i,
                 scol[(size_t)k]);
        return false;
      }
    }
  }
  return true;
}

// What is wrong with the entry (i, j) of a graph whose rows ascend strictly, given that its mirror is missing or differs.
inline void mirror_message(const int32_t* rp, const int32_t* c, const double* v, int64_t i, int32_t j, char* msg, size_t msg_len) {
  const int64_t e = find_col(c, rp[i], rp[i + 1], j), m = find_col(c, rp[j], rp[j + 1], (int32_t)i);
  if (m < 0 || e < 0)
    snprintf(msg, msg_len, "ai_csr_from_host: the entry at row %lld, column %d has no mirror at row %d, column %lld", (long long)i, j,
             j, (long long)i);
  else
    snprintf(msg, msg_len, "ai_csr_from_host: the entry at row %lld, column %d is %.17g, its mirror at row %d, column %lld is %.17g",
             (long long)i, j, v[e], j, (long long)i, v[m]);
}

// Every entry (i, j) of a graph whose rows ascend strictly has a mirror (j, i) with the same bits.  (ai_csr_from_host runs this
// on the host only for input whose rows it had to sort; rows stored in ascending order are checked by k_csr_mirror on the device.)
// Each entry above the diagonal looks its mirror up below it; the look-up is one-to-one (no duplicates), so when as many entries
// lie below the diagonal as above it, every one of them is the mirror of one above.
inline bool mirrors(int64_t n, const int32_t* rp, const int32_t* c, const double* v, char* msg, size_t msg_len) {
  int64_t upper = 0, lower = 0;
  bool ok = true;
  for (int64_t i = 0; i < n && ok; ++i)
    for (int64_t e = rp[i]; e < rp[i + 1]; ++e) {
      const int32_t j = c[e];
      if (j < i) ++lower;
      if (j <= i) continue;
      ++upper;
      const int64_t m = find_col(c, rp[j], rp[j + 1], (int32_t)i);
      if (m < 0 || !same_bits(v[m], v[e])) {
        ok = false;
        break;
      }
    }
  if (ok && upper == lower) return true;
  // refused: name the first entry, by row and then by column, whose mirror is missing or differs
  for (int64_t i = 0; i < n; ++i)
    for (int64_t e = rp[i]; e < rp[i + 1]; ++e) {
      const int32_t j = c[e];
      if (j == i) continue;
      const int64_t m = find_col(c, rp[j], rp[j + 1], (int32_t)i);
      if (m >= 0 && same_bits(v[m], v[e])) continue;
      mirror_message(rp, c, v, i, j, msg, msg_len);
      return false;
    }
  snprintf(msg, msg_len, "ai_csr_from_host: the graph is not symmetric");  // not reached: a failed count has an offending entry
  return false;
}

// The whole contract on the host: values, then duplicates, then mirrors.
inline bool check(int64_t n, const int32_t* rp, const int32_t* col, const double* val, char* msg, size_t msg_len) {
  bool ascending = true;
  if (!values(n, rp, col, val, &ascending, msg, msg_len)) return false;
  if (ascending) return mirrors(n, rp, col, val, msg, msg_len);
  std::vector<int32_t> scol;
  std::vector<double> sval;
  return by_column(n, rp, col, val, scol, sval, msg, msg_len) && mirrors(n, rp, scol.data(), sval.data(), msg, msg_len);
}

}  // namespace ai_csr_check
