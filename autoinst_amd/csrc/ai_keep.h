// Rules A1 and A2 of ai_aggregate_scans (include/autoinst_hip.h): which points of a scan the dataset's filter chain keeps.  Shared by
// ai_aggregate.hip (A1-A3) and ai_ground.hip (rule G1 of ai_ground_planes), so that the two entries cannot disagree about a point.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct AIKeep {
  uint32_t moving;         // A1 threshold
  float rmin, rmax;        // A2 bounds, rounded to float32 once
  int32_t use_moving, use_range;
};

// the switches and bounds from the entry points' arguments: moving_index < 0 and range_max < 0 switch a filter off
inline AIKeep ai_keep_rules(int32_t moving_index, double range_min, double range_max) {
  AIKeep k = {};
  k.use_moving = moving_index >= 0 ? 1 : 0;
  k.use_range = !(range_max < 0.0) ? 1 : 0;
  k.moving = k.use_moving ? (uint32_t)moving_index : 0u;
  k.rmin = (float)range_min;
  k.rmax = (float)range_max;
  return k;
}

// A1 and A2 for a point (x, y, z) with label word w.  The float32 norm: s = (x*x + y*y) + z*z, every step rounded; the square root
// is taken in float64 and rounded to float32, which is the correctly rounded float32 root (53 >= 2 * 24 + 2 bits).  A NaN
// coordinate gives a NaN r and fails both comparisons.
__device__ __forceinline__ bool ai_keep_point(const AIKeep& k, float x, float y, float z, uint32_t w) {
#pragma clang fp contract(off)
  bool keep = true;
  if (k.use_moving) keep = (w & 0xFFFFu) < k.moving;
  if (k.use_range) {
    const float s = (x * x + y * y) + z * z;
    const float r = (float)sqrt((double)s);
    keep = keep && r >= k.rmin && r <= k.rmax;
  }
  return keep;
}
