// The project's fixed-order point transform, shared by ai_camera.hip (step 1 of ai_camera_project), ai_scanpool.hip (rule R1 of
// ai_scan_pool) and ai_aggregate.hip (rule A4 of ai_aggregate_scans).  camera_api.transform_points is the same order on the host.
#pragma once
#include <hip/hip_runtime.h>

// open3d PointCloud::transform of one point: row r = ((T[r,0]*x + T[r,1]*y) + T[r,2]*z) + T[r,3], divided by row 3 (w).
// T: 16 doubles, row-major.  Every step is rounded on its own: no contraction.
__device__ __forceinline__ void ai_xf(const double* __restrict__ T, double x, double y, double z, double& ox, double& oy, double& oz) {
#pragma clang fp contract(off)
  const double a = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  const double b = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  const double c = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
  const double w = ((T[12] * x + T[13] * y) + T[14] * z) + T[15];
  ox = a / w;
  oy = b / w;
  oz = c / w;
}
