// Hidden point removal on the device: open3d 0.17 PointCloud::HiddenPointRemoval as hidden_point_removal_o3d calls it
// (pipeline/utils/image/hidden_points_removal.py:6-25) from image_based_features_per_patch (pipeline/utils/image/image_utils.py:
// 155-204), for every view of a chunk in one call and without a hull:
//
//   ai_hidden_points -- a point is visible iff its flipped image is a vertex of the hull of the flipped points and the camera;
//                       that is a feasibility question in two unknowns (rules H1-H6 in include/autoinst_hip.h), decided per point
//                       by Seidel's incremental program: first over the points of the 27 direction cells around it (which proves
//                       almost every hidden point hidden), then, for the survivors, over all points of the view.
//
// Kernels and measurements: DESIGN.md section 22.  tests/hpr_ref.py restates the rules in NumPy, bit for bit.
#include <cmath>
#include <cstring>

#include "ai_entry.h"
#include "ai_runs.h"
#include "ai_xform.h"  // ai_xf: the fixed-order transform (H1)

namespace {

#define HP_GRID 64                                   // cells per axis of the direction grid over [-1, 1]^3 (H5)
#define HP_NCELL (HP_GRID * HP_GRID * HP_GRID)
#define HP_KEY_BITS 18
#define HP_BOX 1e12                                  // |t_k| <= HP_BOX (H4)
#define HP_TILE 256                                  // constraints staged in LDS per step of the global pass
#define HP_STEP 4                                    // constraints a lane of the global pass tests before it looks for a violated one

struct HpView {  // per view, written by kh_view
  double two_R, S;
  int32_t skip, pad;
};

// H1 and the extent of the view: the subset's points in the camera frame, and per block the min / max of every coordinate (a
// coordinate that is not finite goes in as +inf on both sides, as in kp_bounds)
__global__ __launch_bounds__(AI_BLOCK) void kh_xform(const double* __restrict__ cloud, const int32_t* __restrict__ subset, int64_t m,
                                                     const double* __restrict__ T, double* __restrict__ P, double* __restrict__ part) {
  __shared__ double sm[6][AI_BLOCK / 64];
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t j = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x; j < m; j += (int64_t)gridDim.x * AI_BLOCK) {
    const int64_t s = subset ? subset[j] : j;
    double c[3];
    ai_xf(T, cloud[s * 3], cloud[s * 3 + 1], cloud[s * 3 + 2], c[0], c[1], c[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      P[j * 3 + a] = c[a];
      const double v = fabs(c[a]) < INFINITY ? c[a] : INFINITY;
      mn[a] = fmin(mn[a], v);
      mx[a] = fmax(mx[a], v);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[a] = fmin(mn[a], __shfl_xor(mn[a], o, 64));
      mx[a] = fmax(mx[a], __shfl_xor(mx[a], o, 64));
    }
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      sm[a][w] = mn[a];
      sm[3 + a][w] = mx[a];
    }
  __syncthreads();
  if (threadIdx.x < 6) {
    double r = sm[threadIdx.x][0];
    for (int i = 1; i < AI_BLOCK / 64; ++i) r = (threadIdx.x < 3) ? fmin(r, sm[threadIdx.x][i]) : fmax(r, sm[threadIdx.x][i]);
    part[blockIdx.x * 6 + threadIdx.x] = r;
  }
}

// H2 and H6: the sphere of the view from the partial extents, or the view's skip mark.  One wave.
__global__ __launch_bounds__(64) void kh_view(const double* __restrict__ part, int nb, int64_t m, double radius_factor,
                                              HpView* __restrict__ view) {
#pragma clang fp contract(off)
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int b = threadIdx.x; b < nb; b += 64)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = fmin(mn[a], part[b * 6 + a]);
      mx[a] = fmax(mx[a], part[b * 6 + 3 + a]);
    }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[a] = fmin(mn[a], __shfl_xor(mn[a], o, 64));
      mx[a] = fmax(mx[a], __shfl_xor(mx[a], o, 64));
    }
  if (threadIdx.x != 0) return;
  const double dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
  const double D = sqrt((dx * dx + dy * dy) + dz * dz);
  const double R = radius_factor * D;
  const double two_R = 2.0 * R;
  // no point farther from the camera than the farthest corner of the box: every r_j = 2R - d_j stays positive
  const double fx = fmax(fabs(mn[0]), fabs(mx[0])), fy = fmax(fabs(mn[1]), fabs(mx[1])), fz = fmax(fabs(mn[2]), fabs(mx[2]));
  const double far = sqrt((fx * fx + fy * fy) + fz * fz);
  const bool ok = m >= 4 && R > 0.0 && fabs(two_R * two_R) < INFINITY && fabs(fx) < INFINITY && fabs(fy) < INFINITY &&
                  fabs(fz) < INFINITY && far < two_R;
  view->two_R = two_R;
  view->S = two_R * two_R;
  view->skip = ok ? 0 : 1;
  view->pad = 0;
}

__device__ __forceinline__ int hp_cell1(double e) {
#pragma clang fp contract(off)
  return min(max((int)floor((e + 1.0) * 32.0), 0), HP_GRID - 1);
}

// H2 per point and the key of H5: (ex, ey, ez, u) and the direction cell; the smallest u of the view (u > 0, so the bits of a
// double order as an integer and the minimum is exact whatever the order)
__global__ __launch_bounds__(AI_BLOCK) void kh_points(const double* __restrict__ P, int64_t m, const HpView* __restrict__ view,
                                                      double4* __restrict__ rec, uint32_t* __restrict__ key, int32_t* __restrict__ idx,
                                                      unsigned long long* __restrict__ umin) {
#pragma clang fp contract(off)
  const int64_t j = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  double u = INFINITY;
  if (j < m) {
    const double x = P[j * 3], y = P[j * 3 + 1], z = P[j * 3 + 2];
    double d = sqrt((x * x + y * y) + z * z);
    if (d == 0.0) d = 0.0001;
    double4 r;
    r.x = x / d;
    r.y = y / d;
    r.z = z / d;
    r.w = view->S / (view->two_R - d);
    rec[j] = r;
    key[j] = (uint32_t)((hp_cell1(r.z) * HP_GRID + hp_cell1(r.y)) * HP_GRID + hp_cell1(r.x));
    idx[j] = (int32_t)j;
    if (r.w > 0.0) u = r.w;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) u = fmin(u, __shfl_xor(u, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMin(umin, (unsigned long long)__double_as_longlong(u));
}

// the box of the directions of every tile of HP_TILE sorted records (min x, y, z, max x, y, z): one wave per tile
__global__ __launch_bounds__(AI_BLOCK) void kh_tiles(const double4* __restrict__ srec, int64_t m, const HpView* __restrict__ view,
                                                     double* __restrict__ box) {
  const int lane = threadIdx.x & 63;
  const int64_t tile = (int64_t)blockIdx.x * (AI_BLOCK / 64) + (threadIdx.x >> 6);
  const int64_t first = tile * HP_TILE;
  if (first >= m || view->skip) return;  // wave-uniform
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t p = first + lane; p < first + HP_TILE && p < m; p += 64) {
    const double4 r = srec[p];
    mn[0] = fmin(mn[0], r.x), mn[1] = fmin(mn[1], r.y), mn[2] = fmin(mn[2], r.z);
    mx[0] = fmax(mx[0], r.x), mx[1] = fmax(mx[1], r.y), mx[2] = fmax(mx[2], r.z);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn[a] = fmin(mn[a], __shfl_xor(mn[a], o, 64));
      mx[a] = fmax(mx[a], __shfl_xor(mx[a], o, 64));
    }
  if (lane == 0)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      box[tile * 6 + a] = mn[a];
      box[tile * 6 + 3 + a] = mx[a];
    }
}

__global__ __launch_bounds__(AI_BLOCK) void kh_gather(const double4* __restrict__ rec, const int32_t* __restrict__ order,
                                                      const uint32_t* __restrict__ skey, int64_t m, const HpView* __restrict__ view,
                                                      double4* __restrict__ srec, int32_t* __restrict__ cstart, int32_t* __restrict__ cend) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p >= m || view->skip) return;
  srec[p] = rec[order[p]];
  const uint32_t c = skey[p];
  if (c >= (uint32_t)HP_NCELL) return;  // cannot happen: the key is clamped
  if (p == 0 || skey[p - 1] != c) cstart[c] = (int32_t)p;
  if (p == m - 1 || skey[p + 1] != c) cend[c] = (int32_t)(p + 1);
}

// ----------------------------------------------------------------------------- the program of one point (H3, H4)
struct HpQ {
  double ex, ey, ez, u, ax, ay, az, bx, by, bz;
};

__device__ __forceinline__ HpQ hp_query(double ex, double ey, double ez, double u) {
#pragma clang fp contract(off)
  HpQ q;
  q.ex = ex, q.ey = ey, q.ez = ez, q.u = u;
  const double fx = fabs(ex), fy = fabs(ey), fz = fabs(ez);
  double cx, cy, cz;  // e x axis
  if (fx <= fy && fx <= fz) {
    cx = 0.0, cy = ez, cz = -ey;
  } else if (fy <= fz) {
    cx = -ez, cy = 0.0, cz = ex;
  } else {
    cx = ey, cy = -ex, cz = 0.0;
  }
  const double nrm = sqrt((cx * cx + cy * cy) + cz * cz);
  q.ax = cx / nrm, q.ay = cy / nrm, q.az = cz / nrm;
  q.bx = ey * q.az - ez * q.ay;
  q.by = ez * q.ax - ex * q.az;
  q.bz = ex * q.ay - ey * q.ax;
  return q;
}

__device__ __forceinline__ void hp_constraint(const HpQ& q, const double4 r, double& A0, double& A1, double& g) {
#pragma clang fp contract(off)
  double c = (q.ex * r.x + q.ey * r.y) + q.ez * r.z;
  if (r.x == q.ex && r.y == q.ey && r.z == q.ez) c = 1.0;
  const double wx = r.x - c * q.ex, wy = r.y - c * q.ey, wz = r.z - c * q.ez;
  A0 = (wx * q.ax + wy * q.ay) + wz * q.az;
  A1 = (wx * q.bx + wy * q.by) + wz * q.bz;
  g = r.w - c * q.u;
}

__device__ __forceinline__ double hp_lhs(double t0, double t1, double A0, double A1) {
#pragma clang fp contract(off)
  return t0 * A0 + t1 * A1;
}

struct HpLine {
  double p0, p1, d0, d1, lo, hi;
  bool bad;
};

__device__ __forceinline__ void hp_take(HpLine& ln, double A0, double A1, double g) {
#pragma clang fp contract(off)
  const double den = A0 * ln.d0 + A1 * ln.d1;
  const double num = g - (A0 * ln.p0 + A1 * ln.p1);
  if (den > 0.0)
    ln.hi = fmin(ln.hi, num / den);
  else if (den < 0.0)
    ln.lo = fmax(ln.lo, num / den);
  else if (num < 0.0)
    ln.bad = true;
}

// The re-solve of H4 by one whole wave (every lane active, q / t / the violated constraint the same in every lane): the earlier
// constraints are segments 0 .. s_cur - 1 of the wave's list in full and the first cnt_cur positions of segment s_cur; lane s
// holds segment s as [seg_st, seg_st + seg_len) of the sorted records.  false: infeasible.
__device__ __forceinline__ bool hp_resolve(const HpQ& q, const double4* __restrict__ rec, int32_t seg_st, int32_t seg_len, int s_cur,
                                           int32_t cnt_cur, double Ak0, double Ak1, double gk, double& t0, double& t1, int lane) {
#pragma clang fp contract(off)
  const double nn = Ak0 * Ak0 + Ak1 * Ak1;
  if (nn == 0.0) return false;
  const double f = ((t0 * Ak0 + t1 * Ak1) - gk) / nn;
  HpLine ln;
  ln.p0 = t0 - Ak0 * f;
  ln.p1 = t1 - Ak1 * f;
  ln.d0 = -Ak1;
  ln.d1 = Ak0;
  ln.lo = -INFINITY;
  ln.hi = INFINITY;
  ln.bad = false;
  hp_take(ln, 1.0, 0.0, HP_BOX);
  hp_take(ln, -1.0, 0.0, HP_BOX);
  hp_take(ln, 0.0, 1.0, HP_BOX);
  hp_take(ln, 0.0, -1.0, HP_BOX);
  for (int s = 0; s <= s_cur; ++s) {
    const int32_t st = __shfl(seg_st, s, 64);
    const int32_t n = s < s_cur ? __shfl(seg_len, s, 64) : cnt_cur;
    for (int32_t j = lane; j < n; j += 64) {
      double A0, A1, g;
      hp_constraint(q, rec[st + j], A0, A1, g);
      hp_take(ln, A0, A1, g);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ln.lo = fmax(ln.lo, __shfl_xor(ln.lo, o, 64));
    ln.hi = fmin(ln.hi, __shfl_xor(ln.hi, o, 64));
  }
  if (__any(ln.bad) || ln.lo > ln.hi) return false;
  const double s = fmin(fmax(0.0, ln.lo), ln.hi);
  t0 = ln.p0 + s * ln.d0;
  t1 = ln.p1 + s * ln.d1;
  return true;
}

// The skip rule of the global pass ("The skip rule"): true only if no record whose direction lies in the box b
// can be violated at t, with room for every rounding of the test itself.  cu bounds cos(angle to e_i) over the box from above;
// f(angle) = u_min - u_i cos - |t| sin bounds g - t.w from below and does not fall beyond the box's nearest angle once
// tan >= |t| / u_i there.  A NaN anywhere gives false.
#define HP_SKIP_EPS 1e-9
__device__ __forceinline__ bool hp_can_skip(const HpQ& q, double t0, double t1, const double* __restrict__ b, double u_min) {
#pragma clang fp contract(off)
  const double cu = ((fmax(q.ex * b[0], q.ex * b[3]) + fmax(q.ey * b[1], q.ey * b[4])) + fmax(q.ez * b[2], q.ez * b[5])) + 1e-15;
  const double s2 = 1.0 - cu * cu;
  if (!(cu < 1.0 && s2 >= 1e-6)) return false;
  const double sl = sqrt(s2);
  const double tn = sqrt(t0 * t0 + t1 * t1);
  const bool rising = cu <= 0.0 || sl * q.u >= (tn * cu) * (1.0 + HP_SKIP_EPS);
  const bool clear = (u_min - q.u * cu) - tn * sl > HP_SKIP_EPS * ((u_min + q.u) + tn);
  return rising && clear;
}

// stats of a view: [0] points the local pass proved hidden, [1] re-solves over all points, [2] most re-solves of one point,
// [3] points at the camera
__device__ __forceinline__ void hp_count_resolves(unsigned long long* stats, int nr) {
  atomicAdd(stats + 1, (unsigned long long)nr);
  atomicMax(stats + 2, (unsigned long long)nr);
}

// The local pass: one wave per point p (sorted position).  Lane s < 27 holds the s-th cell of the point's list (its own cell
// first); the wave tests 64 constraints of a cell per step against the current t, __ballot finds the first violated one, and the
// wave re-solves over everything before it.  A hidden point gets its flag here; a survivor leaves its t and its re-solve count.
__global__ __launch_bounds__(AI_BLOCK) void kh_local(const HpView* __restrict__ view, const double4* __restrict__ rec, int64_t m,
                                                     const int32_t* __restrict__ cstart, const int32_t* __restrict__ cend,
                                                     const int32_t* __restrict__ order, double* __restrict__ tstate,
                                                     int32_t* __restrict__ surv, int32_t* __restrict__ nres, uint8_t* __restrict__ flags,
                                                     unsigned long long* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * (AI_BLOCK / 64) + (threadIdx.x >> 6);
  if (p >= m) return;  // wave-uniform
  if (view->skip) {    // the scan and the compaction behind this kernel then find no survivor
    if (lane == 0) surv[p] = 0;
    return;
  }
  const double4 me = rec[p];
  if (me.x == 0.0 && me.y == 0.0 && me.z == 0.0) {  // at the camera (H5)
    if (lane == 0) {
      surv[p] = 0;
      flags[order[p]] = 0;
      atomicAdd(stats + 3, 1ull);
    }
    return;
  }
  const HpQ q = hp_query(me.x, me.y, me.z, me.w);
  const int cx = hp_cell1(me.x), cy = hp_cell1(me.y), cz = hp_cell1(me.z);
  int32_t seg_st = 0, seg_len = 0;
  if (lane < 27) {
    const int o = lane == 0 ? 13 : (lane <= 13 ? lane - 1 : lane);  // 0 .. 26 in (dz, dy, dx) order, the centre (13) first
    const int xx = cx + o % 3 - 1, yy = cy + (o / 3) % 3 - 1, zz = cz + o / 9 - 1;
    if (xx >= 0 && xx < HP_GRID && yy >= 0 && yy < HP_GRID && zz >= 0 && zz < HP_GRID) {
      const int32_t cc = (zz * HP_GRID + yy) * HP_GRID + xx;
      const int32_t s = cstart[cc];
      if (s >= 0) {
        seg_st = s;
        seg_len = cend[cc] - s;
      }
    }
  }
  double t0 = 0.0, t1 = 0.0;
  int nr = 0;
  bool feasible = true;
  for (int s = 0; s < 27 && feasible; ++s) {
    const int32_t st = __shfl(seg_st, s, 64), n = __shfl(seg_len, s, 64);
    int32_t from = 0;  // positions of this cell below `from` are behind the last re-solve
    int32_t base = 0;
    while (base < n) {  // every turn moves base or from forward: at most 2 n turns
      const int32_t j = base + lane;
      double A0 = 0.0, A1 = 0.0, g = 0.0;
      bool viol = false;
      if (j < n && j >= from) {
        hp_constraint(q, rec[st + j], A0, A1, g);
        viol = hp_lhs(t0, t1, A0, A1) > g;
      }
      const unsigned long long mask = __ballot(viol);
      if (!mask) {
        base += 64;
        continue;
      }
      const int L = __ffsll((long long)mask) - 1;
      const double Ak0 = __shfl(A0, L, 64), Ak1 = __shfl(A1, L, 64), gk = __shfl(g, L, 64);
      ++nr;
      if (!hp_resolve(q, rec, seg_st, seg_len, s, base + L, Ak0, Ak1, gk, t0, t1, lane)) {
        feasible = false;
        break;
      }
      from = base + L + 1;
    }
  }
  if (lane != 0) return;
  if (feasible) {
    tstate[p * 2] = t0;
    tstate[p * 2 + 1] = t1;
    nres[p] = nr;
    surv[p] = 1;
  } else {
    surv[p] = 0;
    flags[order[p]] = 0;
    atomicAdd(stats, 1ull);
    hp_count_resolves(stats, nr);
  }
}

// The global pass: one lane per survivor, the view's records through LDS in tiles, every lane of a block against the same
// constraint at a time (an LDS broadcast), HP_STEP constraints per look.  A lane that finds a violated constraint waits for its
// wave: the wave then re-solves for each such lane in turn, all 64 lanes over the earlier records, and the lane goes on behind
// the constraint.  No block waits for another; every loop ends with the tile.
__global__ __launch_bounds__(AI_BLOCK) void kh_global(const HpView* __restrict__ view, const double4* __restrict__ rec, int64_t m,
                                                      const int32_t* __restrict__ list, const int32_t* __restrict__ pos,
                                                      const double* __restrict__ tstate, const int32_t* __restrict__ nres,
                                                      const int32_t* __restrict__ order, const double* __restrict__ box,
                                                      const unsigned long long* __restrict__ umin, uint8_t* __restrict__ flags,
                                                      unsigned long long* __restrict__ count, unsigned long long* __restrict__ stats) {
  if (view->skip) return;
  const int32_t cnt = pos[m];
  const double u_min = __longlong_as_double((long long)*umin);
  const int64_t first = (int64_t)blockIdx.x * AI_BLOCK;
  if (first >= cnt) return;  // block-uniform
  __shared__ double4 tile[HP_TILE + HP_STEP];
  const int tid = threadIdx.x, lane = tid & 63;
  const bool active = first + tid < cnt;
  const int32_t p = active ? list[first + tid] : 0;
  const double4 me = rec[p];
  const HpQ q = hp_query(me.x, me.y, me.z, me.w);
  double t0 = tstate[(int64_t)p * 2], t1 = tstate[(int64_t)p * 2 + 1];
  int nr = active ? nres[p] : 0;
  bool feas = active;
  // a neutral record (direction 0, u = 1: 0 <= 1 for every query) behind the tile and behind the view's last record
  if (tid < HP_STEP) tile[HP_TILE + tid] = make_double4(0.0, 0.0, 0.0, 1.0);
  for (int64_t tb = 0; tb < m; tb += HP_TILE) {
    // a lane passes over a tile none of whose records can be violated at its t; a tile that every lane of the block passes over
    // is not staged.  The barrier also ends the block's use of the previous tile.
    const bool need = feas && !hp_can_skip(q, t0, t1, box + (tb / HP_TILE) * 6, u_min);
    if (!__syncthreads_or(need)) continue;
    if (tb + tid < m)
      tile[tid] = rec[tb + tid];
    else
      tile[tid] = make_double4(0.0, 0.0, 0.0, 1.0);
    __syncthreads();
    const int tl = (int)(m - tb < HP_TILE ? m - tb : HP_TILE);
    int jj = need ? 0 : tl;
    for (;;) {  // a turn without a violated constraint in the wave ends it; every other turn moves a lane's jj forward
      double Ak0 = 0.0, Ak1 = 0.0, gk = 0.0;
      bool viol = false;
      if (feas)
        for (; jj < tl; jj += HP_STEP) {
          int kk = 0;
#pragma unroll
          for (int k = 0; k < HP_STEP; ++k) {  // independent of each other; the first violated one is kept
            double A0, A1, g;
            hp_constraint(q, tile[jj + k], A0, A1, g);
            const bool first = !viol && hp_lhs(t0, t1, A0, A1) > g;
            Ak0 = first ? A0 : Ak0, Ak1 = first ? A1 : Ak1, gk = first ? g : gk;
            kk = first ? k : kk;
            viol |= first;
          }
          if (viol) {
            jj += kk;
            break;
          }
        }
      unsigned long long mask = __ballot(viol);
      if (!mask) break;
      while (mask) {
        const int L = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        HpQ ql;
        ql.ex = __shfl(q.ex, L, 64), ql.ey = __shfl(q.ey, L, 64), ql.ez = __shfl(q.ez, L, 64), ql.u = __shfl(q.u, L, 64);
        ql.ax = __shfl(q.ax, L, 64), ql.ay = __shfl(q.ay, L, 64), ql.az = __shfl(q.az, L, 64);
        ql.bx = __shfl(q.bx, L, 64), ql.by = __shfl(q.by, L, 64), ql.bz = __shfl(q.bz, L, 64);
        double u0 = __shfl(t0, L, 64), u1 = __shfl(t1, L, 64);
        const int32_t k = (int32_t)tb + __shfl(jj, L, 64);  // < m: a neutral record is never violated
        const bool ok = hp_resolve(ql, rec, 0, (int32_t)m, 0, k, __shfl(Ak0, L, 64), __shfl(Ak1, L, 64), __shfl(gk, L, 64), u0, u1, lane);
        if (lane == L) {
          ++nr;
          if (ok) {
            t0 = u0, t1 = u1;
            ++jj;
          } else {
            feas = false;
          }
        }
      }
    }
  }
  if (active) {
    flags[order[p]] = feas ? 1 : 0;
    hp_count_resolves(stats, nr);
  }
  const unsigned long long vis = __ballot(active && feas);
  if (lane == 0 && vis) atomicAdd(count, (unsigned long long)__popcll(vis));
}

__global__ __launch_bounds__(AI_BLOCK) void kh_subset_ok(const int32_t* __restrict__ subset, int64_t m, int64_t n_cloud, int32_t* __restrict__ bad) {
  const int64_t j = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (j < m && (subset[j] < 0 || subset[j] >= n_cloud)) *bad = 1;
}

}  // namespace

extern "C" int ai_hidden_points(ai_ctx* ctx, const double* cloud_xyz, int64_t n_cloud, const int32_t* subset, int64_t n_subset,
                                const double* T_pcd2cam, int32_t n_views, double radius_factor, int mem_kind, uint8_t* flags_out,
                                int64_t* count_out, int32_t* status_out, int64_t* stats_out) {
  const char* who = "ai_hidden_points";
  const int64_t lim = (int64_t)1 << 30;
  const int64_t m = subset ? n_subset : n_cloud;
  if (!ctx || n_cloud < 0 || n_cloud >= lim || n_subset < 0 || n_subset >= lim || n_views < 0 || (n_cloud > 0 && !cloud_xyz) ||
      (n_views > 0 && (!T_pcd2cam || !count_out || !status_out)) || (n_views > 0 && m > 0 && !flags_out) || !std::isfinite(radius_factor) ||
      (mem_kind != AI_MEM_HOST && mem_kind != AI_MEM_DEVICE))
    return bad_arg(who, "bad argument (null pointer, a size outside [0, 2^30), n_views < 0, radius_factor not finite)");
  for (int v = 0; v < n_views; ++v) {
    const double* T = T_pcd2cam + 16 * v;
    for (int k = 0; k < 16; ++k)
      if (!std::isfinite(T[k])) {
        ai_set_error("%s: T_pcd2cam of view %d is not finite", who, v);
        return AI_ERR_BAD_ARG;
      }
    if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0) {
      ai_set_error("%s: the last row of T_pcd2cam of view %d must be (0, 0, 0, 1)", who, v);
      return AI_ERR_BAD_ARG;
    }
  }
  if (n_views == 0) return AI_OK;
  AI_HIP(hipSetDevice(ctx->device));
  ArenaScope arena_scope(&ctx->arena);
  hipStream_t st = ctx->stream;
  DevBuf<double> own_c;
  DevBuf<int32_t> own_s, d_bad;
  const double* dc = nullptr;
  const int32_t* ds = nullptr;
  if (n_cloud > 0) AI_TRY(to_device(cloud_xyz, (size_t)n_cloud * 3, mem_kind, own_c, &dc, st));
  if (subset && m > 0) {
    AI_TRY(to_device(subset, (size_t)m, mem_kind, own_s, &ds, st));
    AI_TRY(d_bad.alloc(1));
    AI_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(kh_subset_ok, dim3(grid_for(m)), dim3(AI_BLOCK), 0, st, ds, m, n_cloud, d_bad.p);
    AI_KERNEL_CHECK();
    int32_t bad = 0;
    AI_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AI_HIP(hipStreamSynchronize(st));
    if (bad) return bad_arg(who, "subset holds a row outside [0, n_cloud)");
  }
  if (m < 4) {  // H6: no view has four points
    for (int v = 0; v < n_views; ++v) status_out[v] = 1;
    if (stats_out) memset(stats_out, 0, (size_t)n_views * 4 * sizeof(int64_t));
    return AI_OK;
  }

  const int nb = (int)std::min<int64_t>(grid_for(m), 1024);
  const unsigned gm = grid_for(m);
  DevBuf<double> d_T, d_P, d_part, d_t, d_box;
  DevBuf<double4> d_rec, d_srec;
  DevBuf<uint32_t> d_key, d_skey;
  DevBuf<int32_t> d_idx, d_order, d_cstart, d_cend, d_surv, d_list, d_nres, d_scan;
  DevBuf<uint8_t> d_tmp, own_flags;
  DevBuf<HpView> d_view;
  DevBuf<unsigned long long> d_cnt, d_umin;  // per view: the count, then the four stats; the bits of the smallest u
  AI_TRY(d_T.alloc((size_t)n_views * 16));
  AI_HIP(hipMemcpyAsync(d_T.p, T_pcd2cam, (size_t)n_views * 16 * sizeof(double), hipMemcpyHostToDevice, st));
  AI_TRY(d_P.alloc((size_t)m * 3));
  AI_TRY(d_part.alloc((size_t)nb * 6));
  AI_TRY(d_t.alloc((size_t)m * 2));
  AI_TRY(d_rec.alloc((size_t)m));
  AI_TRY(d_srec.alloc((size_t)m));
  AI_TRY(d_key.alloc((size_t)m));
  AI_TRY(d_skey.alloc((size_t)m));
  AI_TRY(d_idx.alloc((size_t)m));
  AI_TRY(d_order.alloc((size_t)m));
  AI_TRY(d_cstart.alloc(HP_NCELL));
  AI_TRY(d_cend.alloc(HP_NCELL));
  AI_TRY(d_surv.alloc((size_t)m + 1));
  AI_TRY(d_list.alloc((size_t)m));
  AI_TRY(d_nres.alloc((size_t)m));
  AI_TRY(d_scan.alloc(ai_scan_tmp_elems(m)));
  AI_TRY(d_view.alloc((size_t)n_views));
  const int64_t n_tiles = (m + HP_TILE - 1) / HP_TILE;
  AI_TRY(d_box.alloc((size_t)n_tiles * 6));
  AI_TRY(d_umin.alloc((size_t)n_views));
  AI_HIP(hipMemsetAsync(d_umin.p, 0xff, (size_t)n_views * sizeof(unsigned long long), st));
  AI_TRY(d_cnt.alloc((size_t)n_views * 5));
  AI_HIP(hipMemsetAsync(d_cnt.p, 0, (size_t)n_views * 5 * sizeof(unsigned long long), st));
  uint8_t* dflags = nullptr;
  AI_TRY(dev_out(flags_out, (size_t)n_views * m, mem_kind, own_flags, &dflags));

  for (int v = 0; v < n_views; ++v) {
    HpView* view = d_view.p + v;
    uint8_t* fl = dflags + (size_t)v * m;
    unsigned long long* cnt = d_cnt.p + (size_t)v * 5;
    hipLaunchKernelGGL(kh_xform, dim3(nb), dim3(AI_BLOCK), 0, st, dc, ds, m, (const double*)(d_T.p + 16 * v), d_P.p, d_part.p);
    AI_KERNEL_CHECK();
    hipLaunchKernelGGL(kh_view, dim3(1), dim3(64), 0, st, (const double*)d_part.p, nb, m, radius_factor, view);
    AI_KERNEL_CHECK();
    hipLaunchKernelGGL(kh_points, dim3(gm), dim3(AI_BLOCK), 0, st, (const double*)d_P.p, m, (const HpView*)view, d_rec.p, d_key.p, d_idx.p,
                       d_umin.p + v);
    AI_KERNEL_CHECK();
    AI_TRY(sort_pairs(st, d_key.p, d_skey.p, d_idx.p, d_order.p, m, HP_KEY_BITS, d_tmp));
    AI_HIP(hipMemsetAsync(d_cstart.p, 0xff, (size_t)HP_NCELL * sizeof(int32_t), st));
    AI_HIP(hipMemsetAsync(d_cend.p, 0, (size_t)HP_NCELL * sizeof(int32_t), st));
    hipLaunchKernelGGL(kh_gather, dim3(gm), dim3(AI_BLOCK), 0, st, (const double4*)d_rec.p, (const int32_t*)d_order.p,
                       (const uint32_t*)d_skey.p, m, (const HpView*)view, d_srec.p, d_cstart.p, d_cend.p);
    AI_KERNEL_CHECK();
    hipLaunchKernelGGL(kh_tiles, dim3((unsigned)((n_tiles + AI_BLOCK / 64 - 1) / (AI_BLOCK / 64))), dim3(AI_BLOCK), 0, st,
                       (const double4*)d_srec.p, m, (const HpView*)view, d_box.p);
    AI_KERNEL_CHECK();
    const unsigned gw = (unsigned)((m + AI_BLOCK / 64 - 1) / (AI_BLOCK / 64));
    hipLaunchKernelGGL(kh_local, dim3(gw), dim3(AI_BLOCK), 0, st, (const HpView*)view, (const double4*)d_srec.p, m,
                       (const int32_t*)d_cstart.p, (const int32_t*)d_cend.p, (const int32_t*)d_order.p, d_t.p, d_surv.p, d_nres.p, fl, cnt + 1);
    AI_KERNEL_CHECK();
    AI_TRY(ai_exclusive_scan_i32(st, d_surv.p, d_surv.p, m, d_scan.p));
    hipLaunchKernelGGL(kq_compact, dim3(gm), dim3(AI_BLOCK), 0, st, (const int32_t*)d_surv.p, m, d_list.p);
    AI_KERNEL_CHECK();
    // the number of survivors stays on the device: a block past it leaves at once
    hipLaunchKernelGGL(kh_global, dim3(gm), dim3(AI_BLOCK), 0, st, (const HpView*)view, (const double4*)d_srec.p, m,
                       (const int32_t*)d_list.p, (const int32_t*)d_surv.p, (const double*)d_t.p, (const int32_t*)d_nres.p,
                       (const int32_t*)d_order.p, (const double*)d_box.p, (const unsigned long long*)(d_umin.p + v), fl, cnt, cnt + 1);
    AI_KERNEL_CHECK();
  }
  std::vector<HpView> hv((size_t)n_views);
  std::vector<unsigned long long> hc((size_t)n_views * 5);
  AI_HIP(hipMemcpyAsync(hv.data(), d_view.p, hv.size() * sizeof(HpView), hipMemcpyDeviceToHost, st));
  AI_HIP(hipMemcpyAsync(hc.data(), d_cnt.p, hc.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  for (int v = 0; v < n_views; ++v) {
    status_out[v] = hv[v].skip ? 1 : 0;
    if (!hv[v].skip) {
      count_out[v] = (int64_t)hc[(size_t)v * 5];
      if (mem_kind != AI_MEM_DEVICE)
        AI_HIP(hipMemcpyAsync(flags_out + (size_t)v * m, dflags + (size_t)v * m, (size_t)m, hipMemcpyDeviceToHost, st));
    }
    if (stats_out)
      for (int k = 0; k < 4; ++k) stats_out[(size_t)v * 4 + k] = hv[v].skip ? 0 : (int64_t)hc[(size_t)v * 5 + 1 + k];
  }
  AI_HIP(hipStreamSynchronize(st));
  return AI_OK;
}
