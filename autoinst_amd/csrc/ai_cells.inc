// The uniform cell list shared by the point-cloud searches (ai_points.hip, ai_camera.hip): the squared distance of every
// radius / nearest-point test, a dense grid of [start, end) cell ranges over points sorted by cell, and the host-to-device
// copy of a caller's buffer.  Included inside each user's anonymous namespace (every translation unit keeps its own copy).

// The squared distance of both searches, in the order of nanoflann's L2_Adaptor (what open3d's KDTreeFlann runs) and of
// cdist: (dx*dx + dy*dy) + dz*dz, every product and sum rounded on its own.  The default -ffp-contract=fast would fuse the
// two adds into v_fmac_f64 and move a point within an ulp of the radius, or a near-tie, to the other side
// (tests/test_gpu_edges.py).  No contraction in this function.
__device__ __forceinline__ double sq_dist3(double x, double y, double z, double px, double py, double pz) {
#pragma clang fp contract(off)
  const double dx = x - px, dy = y - py, dz = z - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

struct PGrid {
  double minx, miny, minz, inv_cell;
  int nx, ny, nz;
};

__device__ __forceinline__ void pcell_of(const PGrid& g, double x, double y, double z, int& cx, int& cy, int& cz) {
  cx = min(max((int)floor((x - g.minx) * g.inv_cell), 0), g.nx - 1);
  cy = min(max((int)floor((y - g.miny) * g.inv_cell), 0), g.ny - 1);
  cz = min(max((int)floor((z - g.minz) * g.inv_cell), 0), g.nz - 1);
}

__global__ __launch_bounds__(AI_BLOCK) void kp_bounds(const double* __restrict__ xyz, int64_t n, double* __restrict__ part) {
  __shared__ double sm[6][AI_BLOCK / 64];
  double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
  for (int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * AI_BLOCK)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      // fmin / fmax drop a NaN: a coordinate that is not finite goes in as +inf, so that build_cells' extent check sees it
      const double c = xyz[i * 3 + a];
      const double v = fabs(c) < INFINITY ? c : INFINITY;
      mn[a] = fmin(mn[a], v);
      mx[a] = fmax(mx[a], v);
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

// linear cell id as the sort key (the grid is small enough for 32 bits), value = point index
__global__ __launch_bounds__(AI_BLOCK) void kp_keys(const double* __restrict__ xyz, int64_t n, PGrid g, uint32_t* __restrict__ key,
                                                    int32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (i >= n) return;
  int cx, cy, cz;
  pcell_of(g, xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], cx, cy, cz);
  key[i] = (uint32_t)((cz * g.ny + cy) * g.nx + cx);
  idx[i] = (int32_t)i;
}

__global__ __launch_bounds__(AI_BLOCK) void kp_gather(const double* __restrict__ xyz, const int32_t* __restrict__ order,
                                                      const uint32_t* __restrict__ skey, int64_t n, double* __restrict__ X,
                                                      double* __restrict__ Y, double* __restrict__ Z, int32_t* __restrict__ cstart,
                                                      int32_t* __restrict__ cend) {
  const int64_t p = (int64_t)blockIdx.x * AI_BLOCK + threadIdx.x;
  if (p >= n) return;
  const int64_t o = order[p];
  X[p] = xyz[o * 3];
  Y[p] = xyz[o * 3 + 1];
  Z[p] = xyz[o * 3 + 2];
  const uint32_t c = skey[p];
  if (p == 0 || skey[p - 1] != c) cstart[c] = (int32_t)p;
  if (p == n - 1 || skey[p + 1] != c) cend[c] = (int32_t)(p + 1);
}

struct Cells {
  PGrid g;
  double cell;
  DevBuf<int32_t> order, cstart, cend;
  DevBuf<double> X, Y, Z;
};

int build_cells(ai_ctx* ctx, const double* d_xyz, int64_t n, double cell, Cells& C, const char* who) {
  hipStream_t st = ctx->stream;
  const int nb = 256;
  DevBuf<double> part;
  AI_TRY(part.alloc((size_t)nb * 6));
  hipLaunchKernelGGL(kp_bounds, dim3(nb), dim3(AI_BLOCK), 0, st, d_xyz, n, part.p);
  AI_KERNEL_CHECK();
  std::vector<double> hp((size_t)nb * 6);
  AI_HIP(hipMemcpyAsync(hp.data(), part.p, hp.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  AI_HIP(hipStreamSynchronize(st));
  double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
  for (int b = 0; b < nb; ++b)
    for (int a = 0; a < 3; ++a) {
      mn[a] = std::min(mn[a], hp[b * 6 + a]);
      mx[a] = std::max(mx[a], hp[b * 6 + 3 + a]);
    }
  for (int a = 0; a < 3; ++a)
    if (!(mn[a] <= mx[a]) || !(mx[a] - mn[a] < 1e15)) {
      ai_set_error("%s: coordinates are not finite", who);
      return AI_ERR_BAD_ARG;
    }
  // grow the cell until the dense table fits (a coarser grid only means more candidates per query)
  for (;;) {
    const double ex = (mx[0] - mn[0]) / cell, ey = (mx[1] - mn[1]) / cell, ez = (mx[2] - mn[2]) / cell;
    if ((floor(ex) + 1) * (floor(ey) + 1) * (floor(ez) + 1) <= (double)((int64_t)1 << 27)) break;
    cell *= 1.5;
  }
  C.cell = cell;
  C.g.minx = mn[0];
  C.g.miny = mn[1];
  C.g.minz = mn[2];
  C.g.inv_cell = 1.0 / cell;
  C.g.nx = (int)floor((mx[0] - mn[0]) / cell) + 1;
  C.g.ny = (int)floor((mx[1] - mn[1]) / cell) + 1;
  C.g.nz = (int)floor((mx[2] - mn[2]) / cell) + 1;
  const int64_t ncell = (int64_t)C.g.nx * C.g.ny * C.g.nz;
  const unsigned gb = (unsigned)((n + AI_BLOCK - 1) / AI_BLOCK);
  DevBuf<uint32_t> key, skey;
  DevBuf<int32_t> idx;
  AI_TRY(key.alloc(n));
  AI_TRY(skey.alloc(n));
  AI_TRY(idx.alloc(n));
  AI_TRY(C.order.alloc(n));
  AI_TRY(C.cstart.alloc(ncell));
  AI_TRY(C.cend.alloc(ncell));
  AI_TRY(C.X.alloc(n));
  AI_TRY(C.Y.alloc(n));
  AI_TRY(C.Z.alloc(n));
  hipLaunchKernelGGL(kp_keys, dim3(gb), dim3(AI_BLOCK), 0, st, d_xyz, n, C.g, key.p, idx.p);
  AI_KERNEL_CHECK();
  int bits = 1;
  while (((int64_t)1 << bits) < ncell) ++bits;
  size_t tmp_bytes = 0;
  AI_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, key.p, skey.p, idx.p, C.order.p, (size_t)n, 0, bits, st));
  DevBuf<uint8_t> tmp;
  AI_TRY(tmp.alloc(tmp_bytes));
  AI_HIP(rocprim::radix_sort_pairs(tmp.p, tmp_bytes, key.p, skey.p, idx.p, C.order.p, (size_t)n, 0, bits, st));
  AI_HIP(hipMemsetAsync(C.cstart.p, 0xff, (size_t)ncell * sizeof(int32_t), st));
  AI_HIP(hipMemsetAsync(C.cend.p, 0, (size_t)ncell * sizeof(int32_t), st));
  hipLaunchKernelGGL(kp_gather, dim3(gb), dim3(AI_BLOCK), 0, st, d_xyz, (const int32_t*)C.order.p, (const uint32_t*)skey.p, n, C.X.p, C.Y.p,
                     C.Z.p, C.cstart.p, C.cend.p);
  AI_KERNEL_CHECK();
  AI_HIP(hipStreamSynchronize(st));  // key / skey / idx / tmp go out of scope
  return AI_OK;
}

template <typename T>
int to_device(const T* src, size_t count, int mem_kind, DevBuf<T>& own, const T** dev, hipStream_t st) {
  if (mem_kind == AI_MEM_DEVICE) {
    *dev = src;
    return AI_OK;
  }
  AI_TRY(own.alloc(count));
  AI_HIP(hipMemcpyAsync(own.p, src, count * sizeof(T), hipMemcpyHostToDevice, st));
  *dev = own.p;
  return AI_OK;
}
