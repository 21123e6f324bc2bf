// obstacle_grid.h -- the voxel-grid obstacle kind (DDP_HIP_OBSTACLE_GRID, ddp_hip.h): a signed distance field on a regular grid,
// resident in the context and shared by the batch.  The lookup calls no HIP function and compiles for the host as well (in the
// manner of capsule_cost.h: host/test_obstacle_grid_block.cpp runs it alone).  It is the one function behind the value, clearance,
// derivative and query kernels (rbd::obstacle_distance in obstacle_cost.h; obstacle_grid_query_kernel in obstacle_grid.hip), so
// the four cannot disagree by a bit.  The field itself comes from the user (ddp_hip_obstacle_set_grid) or from an occupancy grid by
// the distance transform of obstacle_grid.hip (ddp_hip_obstacle_set_occupancy).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GRID_HD __host__ __device__
#else
#define GRID_HD
#endif

// What a kernel reads of the context's grid.  phi == nullptr: no grid is resident
struct ObstacleGridDev {
  const double* phi;               // [nx][ny][nz], phi[(ix * ny + iy) * nz + iz]
  int32_t n[3];                    // nodes per axis, 2 .. DDP_HIP_MAX_GRID_DIM
  double origin[3];                // world position of node (0, 0, 0)
  double cell;                     // node spacing > 0
};

enum GridLookup { GRID_INSIDE = 0, GRID_OUTSIDE = 1, GRID_NAN = 2 };

// 2 <= n_a <= max_dim, a finite origin, a finite cell > 0 (the checks of the two set calls that need no field)
static inline bool obstacle_grid_shape_ok(const int32_t* dims, const double* origin, double cell, int32_t max_dim) {
  for (int a = 0; a < 3; ++a)
    if (dims[a] < 2 || dims[a] > max_dim || !isfinite(origin[a])) return false;
  return isfinite(cell) && cell > 0.0;
}

// The trilinear interpolant of the field at the world point x and its gradient, by the rule ddp_hip.h pins:
//   s = (x - origin) / cell,   inside iff 0 <= s_a <= n_a - 1 on the three axes,   i_a = min(floor(s_a), n_a - 2),   f_a = s_a - i_a
//   val    = sum over the 8 corners of phi[i + c] prod_a (c_a ? f_a : 1 - f_a)
//   grad_a = (1 / cell) sum over the 8 corners of phi[i + c] (c_a ? +1 : -1) prod_{b != a} (c_b ? f_b : 1 - f_b)
// the corners in the order c = (0,0,0), (0,0,1), (0,1,0), ... (z fastest).  Outside: val = +inf, grad = 0 (free space).  A NaN
// coordinate: val and grad NaN.  At a node (f = 0) the value is the node's, exactly
GRID_HD static inline GridLookup obstacle_grid_lookup(const ObstacleGridDev& G, const double* x, double* val, double* grad) {
  double f[3] = {0.0, 0.0, 0.0};
  int64_t i[3] = {0, 0, 0};
  bool outside = false;
  for (int a = 0; a < 3; ++a) {
    const double s = (x[a] - G.origin[a]) / G.cell;
    if (s != s) { *val = NAN; grad[0] = grad[1] = grad[2] = NAN; return GRID_NAN; }
    if (!(s >= 0.0 && s <= (double)(G.n[a] - 1))) { outside = true; continue; }
    const double fl = floor(s);
    const int64_t ia = (int64_t)fl < (int64_t)(G.n[a] - 2) ? (int64_t)fl : (int64_t)(G.n[a] - 2);
    i[a] = ia;
    f[a] = s - (double)ia;
  }
  if (outside) { *val = INFINITY; grad[0] = grad[1] = grad[2] = 0.0; return GRID_OUTSIDE; }
  const int64_t ny = G.n[1], nz = G.n[2];
  const double* base = G.phi + (i[0] * ny + i[1]) * nz + i[2];
  const double w[3][2] = {{1.0 - f[0], f[0]}, {1.0 - f[1], f[1]}, {1.0 - f[2], f[2]}};
  double v = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
  for (int c = 0; c < 8; ++c) {
    const int cx = c >> 2, cy = (c >> 1) & 1, cz = c & 1;
    const double ph = base[(cx * ny + cy) * nz + cz];
    v += ph * (w[0][cx] * w[1][cy] * w[2][cz]);
    gx += (cx ? ph : -ph) * (w[1][cy] * w[2][cz]);
    gy += (cy ? ph : -ph) * (w[0][cx] * w[2][cz]);
    gz += (cz ? ph : -ph) * (w[0][cx] * w[1][cy]);
  }
  *val = v;
  grad[0] = gx / G.cell; grad[1] = gy / G.cell; grad[2] = gz / G.cell;
  return GRID_INSIDE;
}

// A grid slot's pair: geom = (shift s, margin m), the sphere (p, r) on the robot.  d = phi(p - s) - r - m, u = grad phi(p - s), not
// normalised: it is dd / dp of this d.  Returns false where the pair has no derivative: outside (d = +inf: the pair forms nothing
// and the clearance does not see it) and where the gradient is exactly zero (the rule of a sphere's centre at p)
GRID_HD static inline bool obstacle_grid_distance(const ObstacleGridDev& G, const double* g, const double* p, double r, double* d, double* u) {
  const double x[3] = {p[0] - g[0], p[1] - g[1], p[2] - g[2]};
  double val;
  const GridLookup where = obstacle_grid_lookup(G, x, &val, u);
  if (where == GRID_OUTSIDE) { *d = INFINITY; return false; }
  *d = val - r - g[3];
  return where == GRID_NAN || u[0] != 0.0 || u[1] != 0.0 || u[2] != 0.0;
}

// ---- the field from occupancy: what the transform's kernels and the host share ----------------------------------------------------
// squared index distances are int32; a voxel without a source holds GRID_EDT_BIG (+ up to 3 * 255^2 after the three passes, below
// 2^31) and reads as cap = nx^2 + ny^2 + nz^2 in the end, which every true distance lies below
#define GRID_EDT_BIG (1 << 29)
GRID_HD static inline int32_t obstacle_grid_cap(const int32_t* n) { return n[0] * n[0] + n[1] * n[1] + n[2] * n[2]; }
// phi of a voxel from the squared distance to the nearest voxel of the other kind: the surface lies halfway between two centres
GRID_HD static inline double obstacle_grid_phi(bool occupied, int32_t d2, int32_t cap, double cell) {
  const double dist = sqrt((double)(d2 < cap ? d2 : cap)) - 0.5;
  return occupied ? -cell * dist : cell * dist;
}
