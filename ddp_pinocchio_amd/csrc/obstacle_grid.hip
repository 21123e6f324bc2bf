// obstacle_grid.hip -- the voxel grid of the obstacle slots of kind DDP_HIP_OBSTACLE_GRID (ddp_hip.h; the lookup: obstacle_grid.h):
// the resident field (ddp_hip_obstacle_set_grid, _grid_download, _grid_query) and the exact Euclidean distance transform that
// builds it from occupancy voxels on the device (ddp_hip_obstacle_set_occupancy), so that a scene refreshed every control cycle
// costs one upload of bytes and no round trip through the host.
//
// The transform.  D(v) = min over the source voxels s of |v - s|^2 is separable: three passes of g(i) = min_k f(k) + (i - k)^2
// along the lines of one axis, z then y then x, in int32 (the squared distances are exact integers below 2^31, so the result does
// not depend on the schedule).  Two transforms are wanted, D_occ (sources: occupied) and D_free (sources: free); they are
// independent and run as the two halves of one launch per pass (blockIdx.y / .z = which).  A line is at most
// DDP_HIP_MAX_GRID_DIM = 256 long, so the plain min-plus form with the line in LDS is enough: L reads per output.
//   z pass (edt_z_kernel): lines are contiguous, and so is a run of whole lines.  A workgroup owns as many whole lines as fit
//     into EDT_FLAT elements, reads the occupancy bytes of that run coalesced, leaves f = 0 / BIG in LDS line after line, and lane
//     e forms output e of the run: the lanes of a line read the same LDS word (a broadcast).
//   y and x passes (edt_strided_kernel): a line's elements are `stride` apart, but the lines of neighbouring iz (y pass), or of
//     neighbouring (iy, iz) (x pass), are neighbours in memory.  A workgroup owns EDT_LINES = 64 such lines: lane l holds line l,
//     so that every load and store of a wave is 64 consecutive words, and LDS is laid out [k][lane] (conflict-free both ways).
//     The four waves share the tile; each lane walks its line once per EDT_OUT = 8 outputs, which it keeps in registers.
//     In place: a workgroup has read its lines into LDS before it writes any of them, and no two workgroups share a line.
//   edt_finish_kernel: phi(v) from D_occ (v free) or D_free (v occupied), obstacle_grid_phi.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "capsule_cost.h"
#include "internal.h"
#include "obstacle_cost.h"

static constexpr int EDT_THREADS = 256;
static constexpr int EDT_LINES = 64;
static constexpr int EDT_OUT = 8;
static constexpr int EDT_FLAT = 4096;

// grid (tiles, 2): tile = lines_per_tile whole lines of length L (lines_per_tile * L <= EDT_FLAT), blockIdx.y = which
__global__ __launch_bounds__(EDT_THREADS) void edt_z_kernel(const uint8_t* occ, int32_t* d2, int64_t voxels, int32_t L, int64_t lines,
                                                            int32_t lines_per_tile) {
  __shared__ int32_t s[EDT_FLAT];
  const int which = blockIdx.y;
  const int64_t line0 = (int64_t)blockIdx.x * lines_per_tile;
  if (line0 >= lines) return;
  const int64_t nl = lines - line0 < lines_per_tile ? lines - line0 : lines_per_tile;
  const int ne = (int)(nl * L);
  const int64_t e0 = line0 * L;
  for (int e = threadIdx.x; e < ne; e += EDT_THREADS) s[e] = ((occ[e0 + e] != 0) == (which == 0)) ? 0 : GRID_EDT_BIG;
  __syncthreads();
  int32_t* out = d2 + which * voxels + e0;
  for (int e = threadIdx.x; e < ne; e += EDT_THREADS) {
    const int line = e / L, i = e - line * L;
    const int32_t* row = s + line * L;
    int32_t best = INT_MAX;
    for (int k = 0; k < L; ++k) {
      const int d = i - k;
      const int32_t v = row[k] + d * d;
      best = v < best ? v : best;
    }
    out[e] = best;
  }
}

// grid (ceil(ninner / EDT_LINES), nouter, 2); dynamic LDS: L * EDT_LINES words.  Line (o, j): element k at
// d2[which][o * outer_stride + j + k * stride], j < ninner
__global__ __launch_bounds__(EDT_THREADS) void edt_strided_kernel(int32_t* d2, int64_t voxels, int32_t L, int64_t stride, int64_t ninner,
                                                                  int64_t outer_stride) {
  extern __shared__ int32_t s_line[];   // [L][EDT_LINES]
  const int lane = threadIdx.x % EDT_LINES, seg = threadIdx.x / EDT_LINES;
  constexpr int NSEG = EDT_THREADS / EDT_LINES;
  const int64_t j = (int64_t)blockIdx.x * EDT_LINES + lane;
  const bool valid = j < ninner;
  int32_t* line = d2 + blockIdx.z * voxels + blockIdx.y * outer_stride + (valid ? j : 0);
  for (int k = seg; k < L; k += NSEG) s_line[k * EDT_LINES + lane] = valid ? line[k * stride] : GRID_EDT_BIG;
  __syncthreads();
  if (!valid) return;
  for (int i0 = seg * EDT_OUT; i0 < L; i0 += NSEG * EDT_OUT) {
    int32_t best[EDT_OUT];
#pragma unroll
    for (int r = 0; r < EDT_OUT; ++r) best[r] = INT_MAX;
    for (int k = 0; k < L; ++k) {
      const int32_t v = s_line[k * EDT_LINES + lane];
      const int d = i0 - k;
#pragma unroll
      for (int r = 0; r < EDT_OUT; ++r) {
        const int32_t c = v + (d + r) * (d + r);
        best[r] = c < best[r] ? c : best[r];
      }
    }
#pragma unroll
    for (int r = 0; r < EDT_OUT; ++r)
      if (i0 + r < L) line[(int64_t)(i0 + r) * stride] = best[r];
  }
}

__global__ __launch_bounds__(EDT_THREADS) void edt_finish_kernel(const uint8_t* occ, const int32_t* d2, int64_t voxels, int32_t cap, double cell,
                                                                 double* phi) {
  const int64_t v = (int64_t)blockIdx.x * EDT_THREADS + threadIdx.x;
  if (v >= voxels) return;
  const bool occupied = occ[v] != 0;
  phi[v] = obstacle_grid_phi(occupied, d2[(occupied ? voxels : 0) + v], cap, cell);
}

// ddp_hip_obstacle_grid_query: a lane per point, the lookup of the cost kernels
__global__ __launch_bounds__(EDT_THREADS) void obstacle_grid_query_kernel(ObstacleGridDev G, int64_t n, const double* points, double* val, double* grad) {
  const int64_t i = (int64_t)blockIdx.x * EDT_THREADS + threadIdx.x;
  if (i >= n) return;
  const double x[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
  double v, g[3];
  (void)obstacle_grid_lookup(G, x, &v, g);
  val[i] = v;
  if (grad) { grad[3 * i] = g[0]; grad[3 * i + 1] = g[1]; grad[3 * i + 2] = g[2]; }
}

// ddp_hip_obstacle_grid_segment_query: the rule of the capsule pairs of kind DDP_HIP_CAPSULE_VS_GRID (capsule_cost.h), SEG_LANES lanes
// per segment as the cost kernels deal a pair's samples: lane k looks up the samples k, k + 16, k + 32 and leaves phi in LDS; the
// group's first lane scans them in ascending j and forms point and gradient at j* by the sample routine again
static constexpr int SEG_LANES = 16;
__global__ __launch_bounds__(EDT_THREADS) void obstacle_grid_segment_query_kernel(ObstacleGridDev G, int64_t n, const double* seg, const int32_t* nint,
                                                                                  double* val, int32_t* jout, double* point, double* grad) {
  constexpr int PER = EDT_THREADS / SEG_LANES, NS = DDP_HIP_CAPSULE_GRID_MAX_INTERVALS + 1;
  __shared__ double s_phi[PER][NS];
  const int g = threadIdx.x / SEG_LANES, k = threadIdx.x % SEG_LANES;
  const int64_t i = (int64_t)blockIdx.x * PER + g;
  const bool valid = i < n;
  const double zero[3] = {0.0, 0.0, 0.0};
  double a0[3] = {0.0, 0.0, 0.0}, a1[3] = {0.0, 0.0, 0.0};
  int32_t N = 0;
  if (valid) {
    for (int a = 0; a < 3; ++a) { a0[a] = seg[6 * i + a]; a1[a] = seg[6 * i + 3 + a]; }
    N = nint[i];
    for (int j = k; j <= N; j += SEG_LANES) {
      double c[3], gj[3];
      capsule_grid_sample(G, a0, a1, zero, N, j, c, &s_phi[g][j], gj);
    }
  }
  __syncthreads();
  if (!valid || k != 0) return;
  double best = s_phi[g][0];
  int32_t bj = 0;
  for (int32_t j = 1; j <= N; ++j)
    if (capsule_grid_better(s_phi[g][j], best, false)) { best = s_phi[g][j]; bj = j; }
  double c[3], phi, gj[3];
  capsule_grid_sample(G, a0, a1, zero, N, best == INFINITY ? 0 : bj, c, &phi, gj);
  val[i] = phi;
  if (jout) jout[i] = best == INFINITY ? -1 : bj;
  for (int a = 0; a < 3; ++a) {
    if (point) point[3 * i + a] = c[a];
    if (grad) grad[3 * i + a] = gj[a];
  }
}

static int grid_entry_check(const ddp_hip_ctx* ctx) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & (DDP_HIP_FLAG_OBSTACLE_COST | DDP_HIP_FLAG_CAPSULE_COST))) return DDP_HIP_E_UNSUPPORTED;   // (grid slots, grid pairs)
  return DDP_HIP_OK;
}

// the field the next set call writes: the one not in force, grown to `voxels` doubles.  Nothing that runs reads it: the call that
// took it out of force waited for the stream
static int grid_back_buffer(ddp_hip_ctx* ctx, int64_t voxels, int* which) {
  const int b = ctx->og_cur == 0 ? 1 : 0;
  if (ctx->og_cap[b] < voxels) {
    double* p = nullptr;
    HIP_TRY(hipMalloc(&p, sizeof(double) * (size_t)voxels));
    if (ctx->og_phi[b]) (void)hipFree(ctx->og_phi[b]);
    ctx->og_phi[b] = p;
    ctx->og_cap[b] = voxels;
  }
  *which = b;
  return DDP_HIP_OK;
}

static void grid_commit(ddp_hip_ctx* ctx, int b, const int32_t* dims, const double* origin, double cell) {
  ctx->og_cur = b;
  ctx->og_cell = cell;
  for (int a = 0; a < 3; ++a) { ctx->og_n[a] = dims[a]; ctx->og_origin[a] = origin[a]; }
}

extern "C" int ddp_hip_obstacle_set_grid(ddp_hip_ctx* ctx, const int32_t* dims, const double* origin, double cell, const double* phi) {
  { const int rc = grid_entry_check(ctx); if (rc != DDP_HIP_OK) return rc; }
  if (!dims || !origin || !phi || !obstacle_grid_shape_ok(dims, origin, cell, DDP_HIP_MAX_GRID_DIM)) return DDP_HIP_E_ARG;
  const int64_t voxels = (int64_t)dims[0] * dims[1] * dims[2];
  for (int64_t v = 0; v < voxels; ++v)
    if (!isfinite(phi[v])) return DDP_HIP_E_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  int b;
  { const int rc = grid_back_buffer(ctx, voxels, &b); if (rc != DDP_HIP_OK) return rc; }
  HIP_TRY(hipMemcpyAsync(ctx->og_phi[b], phi, sizeof(double) * (size_t)voxels, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  grid_commit(ctx, b, dims, origin, cell);
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_obstacle_set_occupancy(ddp_hip_ctx* ctx, const int32_t* dims, const double* origin, double cell, const uint8_t* occ) {
  { const int rc = grid_entry_check(ctx); if (rc != DDP_HIP_OK) return rc; }
  if (!dims || !origin || !occ || !obstacle_grid_shape_ok(dims, origin, cell, DDP_HIP_MAX_GRID_DIM)) return DDP_HIP_E_ARG;
  const int32_t nx = dims[0], ny = dims[1], nz = dims[2];
  const int64_t voxels = (int64_t)nx * ny * nz;
  HIP_TRY(hipSetDevice(ctx->device));
  // the temporaries are kept between calls and grow with the largest grid seen
  if (ctx->og_tmp_cap < voxels) {
    int32_t* d2 = nullptr;
    uint8_t* oc = nullptr;
    if (hipMalloc(&d2, sizeof(int32_t) * (size_t)(2 * voxels)) != hipSuccess || hipMalloc(&oc, (size_t)voxels) != hipSuccess) {
      (void)hipGetLastError();
      if (d2) (void)hipFree(d2);
      return DDP_HIP_E_HIP;
    }
    if (ctx->og_d2) (void)hipFree(ctx->og_d2);
    if (ctx->og_occ) (void)hipFree(ctx->og_occ);
    ctx->og_d2 = d2; ctx->og_occ = oc; ctx->og_tmp_cap = voxels;
  }
  int b;
  { const int rc = grid_back_buffer(ctx, voxels, &b); if (rc != DDP_HIP_OK) return rc; }
  HIP_TRY(hipMemcpyAsync(ctx->og_occ, occ, (size_t)voxels, hipMemcpyHostToDevice, ctx->stream));
  const int64_t plane = (int64_t)ny * nz;
  const int32_t lines_per_tile = EDT_FLAT / nz;                               // nz <= 256: at least 16 whole lines
  const int64_t zlines = (int64_t)nx * ny;
  hipLaunchKernelGGL(edt_z_kernel, dim3((unsigned)((zlines + lines_per_tile - 1) / lines_per_tile), 2), dim3(EDT_THREADS), 0, ctx->stream, ctx->og_occ,
                     ctx->og_d2, voxels, nz, zlines, lines_per_tile);
  hipLaunchKernelGGL(edt_strided_kernel, dim3((unsigned)((nz + EDT_LINES - 1) / EDT_LINES), (unsigned)nx, 2), dim3(EDT_THREADS),
                     sizeof(int32_t) * (size_t)(ny * EDT_LINES), ctx->stream, ctx->og_d2, voxels, ny, (int64_t)nz, (int64_t)nz, plane);
  hipLaunchKernelGGL(edt_strided_kernel, dim3((unsigned)((plane + EDT_LINES - 1) / EDT_LINES), 1, 2), dim3(EDT_THREADS),
                     sizeof(int32_t) * (size_t)(nx * EDT_LINES), ctx->stream, ctx->og_d2, voxels, nx, plane, plane, (int64_t)0);
  hipLaunchKernelGGL(edt_finish_kernel, dim3((unsigned)((voxels + EDT_THREADS - 1) / EDT_THREADS)), dim3(EDT_THREADS), 0, ctx->stream, ctx->og_occ,
                     ctx->og_d2, voxels, obstacle_grid_cap(dims), cell, ctx->og_phi[b]);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  grid_commit(ctx, b, dims, origin, cell);
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_obstacle_grid_download(ddp_hip_ctx* ctx, int32_t* dims, double* origin, double* cell, double* phi) {
  { const int rc = grid_entry_check(ctx); if (rc != DDP_HIP_OK) return rc; }
  if (!dims || !origin || !cell || ctx->og_cur < 0) return DDP_HIP_E_ARG;
  for (int a = 0; a < 3; ++a) { dims[a] = ctx->og_n[a]; origin[a] = ctx->og_origin[a]; }
  *cell = ctx->og_cell;
  if (!phi) return DDP_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  const int64_t voxels = (int64_t)dims[0] * dims[1] * dims[2];
  HIP_TRY(hipMemcpyAsync(phi, ctx->og_phi[ctx->og_cur], sizeof(double) * (size_t)voxels, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_obstacle_grid_query(ddp_hip_ctx* ctx, int64_t n, const double* points, double* phi_out, double* grad_out) {
  { const int rc = grid_entry_check(ctx); if (rc != DDP_HIP_OK) return rc; }
  if (n < 0 || ctx->og_cur < 0 || (n > 0 && (!points || !phi_out))) return DDP_HIP_E_ARG;
  if (n == 0) return DDP_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  double* buf = nullptr;                                                     // points | values | gradients
  HIP_TRY(hipMalloc(&buf, sizeof(double) * (size_t)(7 * n)));
  double *val = buf + 3 * n, *grad = buf + 4 * n;
  hipError_t e = hipMemcpyAsync(buf, points, sizeof(double) * (size_t)(3 * n), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(obstacle_grid_query_kernel, dim3((unsigned)((n + EDT_THREADS - 1) / EDT_THREADS)), dim3(EDT_THREADS), 0, ctx->stream,
                       obstacle_grid_dev(ctx), n, buf, val, grad_out ? grad : nullptr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(phi_out, val, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && grad_out) e = hipMemcpyAsync(grad_out, grad, sizeof(double) * (size_t)(3 * n), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  (void)hipFree(buf);
  if (e != hipSuccess || es != hipSuccess) { (void)hipGetLastError(); return DDP_HIP_E_HIP; }
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_obstacle_grid_segment_query(ddp_hip_ctx* ctx, int64_t n, const double* seg, const int32_t* n_intervals, double* phi_out,
                                                   int32_t* j_out, double* point_out, double* grad_out) {
  { const int rc = grid_entry_check(ctx); if (rc != DDP_HIP_OK) return rc; }
  if (n < 0 || ctx->og_cur < 0 || (n > 0 && (!seg || !n_intervals || !phi_out))) return DDP_HIP_E_ARG;
  for (int64_t i = 0; i < n; ++i)
    if (n_intervals[i] < 0 || n_intervals[i] > DDP_HIP_CAPSULE_GRID_MAX_INTERVALS) return DDP_HIP_E_ARG;
  if (n == 0) return DDP_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  double* buf = nullptr;                                                     // segments | values | points | gradients | counts | j*
  HIP_TRY(hipMalloc(&buf, sizeof(double) * (size_t)(13 * n) + sizeof(int32_t) * (size_t)(2 * n)));
  double *val = buf + 6 * n, *point = buf + 7 * n, *grad = buf + 10 * n;
  int32_t *nint = reinterpret_cast<int32_t*>(buf + 13 * n), *jd = nint + n;
  hipError_t e = hipMemcpyAsync(buf, seg, sizeof(double) * (size_t)(6 * n), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(nint, n_intervals, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) {
    constexpr int per = EDT_THREADS / SEG_LANES;
    hipLaunchKernelGGL(obstacle_grid_segment_query_kernel, dim3((unsigned)((n + per - 1) / per)), dim3(EDT_THREADS), 0, ctx->stream,
                       obstacle_grid_dev(ctx), n, buf, nint, val, jd, point, grad);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(phi_out, val, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && j_out) e = hipMemcpyAsync(j_out, jd, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && point_out) e = hipMemcpyAsync(point_out, point, sizeof(double) * (size_t)(3 * n), hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && grad_out) e = hipMemcpyAsync(grad_out, grad, sizeof(double) * (size_t)(3 * n), hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  (void)hipFree(buf);
  if (e != hipSuccess || es != hipSuccess) { (void)hipGetLastError(); return DDP_HIP_E_HIP; }
  return DDP_HIP_OK;
}
