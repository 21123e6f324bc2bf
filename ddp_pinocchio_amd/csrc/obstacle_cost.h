// obstacle_cost.h -- per-instance obstacle-avoidance costs (DDP_HIP_FLAG_OBSTACLE_COST, ddp_hip.h): collision spheres on the
// robot against per-instance spheres and half-spaces, a one-sided penalty.  The kernel-side description and the device helpers;
// the terms themselves are formed by kernels of their own in fwd.hip (cost values: obstacle_cost_kernel, summed by
// com_sum_kernel; clearances: obstacle_clearance_kernel) and lin.hip (derivatives: lin_obstacle_cost_kernel).
#pragma once
#include "frame_walk.h"
#include "internal.h"
#include "lie.h"
#include "obstacle_grid.h"
#include "rbd.h"

// What a kernel reads of the context's obstacle cost.  geom == nullptr: no terms (the flag is off, no points are set, or no
// non-zero weight has been uploaded: the block's CostBlock::live)
struct ObstacleCostDev {
  const double *geom, *weight;     // [batch][T+1][no][4], [batch][T+1][no]
  int32_t np, no;                  // collision points, obstacle slots
  int32_t joint[DDP_HIP_MAX_COLLISION_POINTS];
  int32_t kind[DDP_HIP_MAX_OBSTACLES];
  double off[DDP_HIP_MAX_COLLISION_POINTS][3];
  double radius[DDP_HIP_MAX_COLLISION_POINTS];
  ObstacleGridDev grid;            // what the slots of kind DDP_HIP_OBSTACLE_GRID read (phi == nullptr: no grid is resident)
  bool grid_slots;                 // some slot is of that kind: the kernels' GRID instantiation runs
};

inline ObstacleGridDev obstacle_grid_dev(const ddp_hip_ctx* ctx) {
  ObstacleGridDev g{};
  if (ctx->og_cur < 0) return g;
  g.phi = ctx->og_phi[ctx->og_cur];
  g.cell = ctx->og_cell;
  for (int a = 0; a < 3; ++a) { g.n[a] = ctx->og_n[a]; g.origin[a] = ctx->og_origin[a]; }
  return g;
}

// always: the description whether or not a weight is live (ddp_hip_obstacle_clearance works from the first set_points on)
inline ObstacleCostDev obstacle_cost_dev(const ddp_hip_ctx* ctx, bool always = false) {
  ObstacleCostDev c{};
  const CostBlock& k = ctx->cost[COST_OBSTACLE];
  if (!(always ? ctx->ob_np > 0 : k.live)) return c;
  c.geom = k.side[0];
  c.weight = k.side[1];
  c.np = ctx->ob_np;
  c.no = ctx->ob_no;
  for (int k = 0; k < ctx->ob_np; ++k) {
    c.joint[k] = ctx->ob_joint[k];
    c.radius[k] = ctx->ob_radius[k];
    for (int a = 0; a < 3; ++a) c.off[k][a] = ctx->ob_off[k][a];
  }
  for (int o = 0; o < ctx->ob_no; ++o) {
    c.kind[o] = ctx->ob_kind[o];
    c.grid_slots |= ctx->ob_kind[o] == DDP_HIP_OBSTACLE_GRID;
  }
  c.grid = obstacle_grid_dev(ctx);
  return c;
}

namespace rbd {

// The signed distance d_ko of the sphere (p, r) on the robot to an obstacle slot, and the direction u_ko = dd / dp:
//   sphere      g = (c, rho):  d = |p - c| - (r + rho),   u = (p - c) / |p - c|
//   half-space  g = (n, h):    d = n . p - h - r,         u = n
//   grid        g = (s, m):    d = phi(p - s) - r - m,    u = grad phi(p - s)      (obstacle_grid.h; outside the grid d = +inf)
// Returns false where u does not exist (a sphere's centre at p, a grid's zero gradient: the pair has its value and no derivative).
// GRID: some slot may be a grid's.  The kernels are instantiated both ways and a context without a grid slot runs the instruction
// stream it ran before the kind existed
template <bool GRID>
__device__ __forceinline__ bool obstacle_distance(const ObstacleCostDev& ob, int kind, const double* g, const double* p, double r, double* d, double* u) {
  if (GRID && kind == DDP_HIP_OBSTACLE_GRID) return obstacle_grid_distance(ob.grid, g, p, r, d, u);
  if (kind == DDP_HIP_OBSTACLE_HALFSPACE) {
    *d = (g[0] * p[0] + g[1] * p[1] + g[2] * p[2]) - g[3] - r;
    u[0] = g[0]; u[1] = g[1]; u[2] = g[2];
    return true;
  }
  const double x = p[0] - g[0], y = p[1] - g[1], z = p[2] - g[2];
  const double dist = sqrt(x * x + y * y + z * z);
  *d = dist - (r + g[3]);
  if (dist == 0.0) { u[0] = u[1] = u[2] = 0.0; return false; }
  u[0] = x / dist; u[1] = y / dist; u[2] = z / dist;
  return true;
}

// e = d < 0 ? d : 0 is non-zero: the pair is active.  Written so that a NaN distance (a non-finite state) is active as well and
// its term NaN, as the other cost kernels' terms are
__device__ __forceinline__ bool obstacle_active(double d) { return !(d >= 0.0); }

// 1/2 sum_o w_o e_ko^2 of one point over the live slots in ascending order, the pairs with w == 0 or e == 0 left out; *active:
// some pair took part.  The caller has found a live slot; a non-finite point gives NaN
template <bool GRID>
__device__ __forceinline__ double obstacle_point_term(const ObstacleCostDev& ob, int k, const double* p, const double* geom, const double* w,
                                                      bool* active) {
  double s = 0.0;
  bool act = false;
  if (!(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]))) { *active = true; return NAN; }   // (an infinite point is clear of a sphere)
  for (int o = 0; o < ob.no; ++o) {
    const double wo = w[o];
    if (wo == 0.0) continue;
    double d, u[3];
    (void)obstacle_distance<GRID>(ob, ob.kind[o], geom + 4 * o, p, ob.radius[k], &d, u);
    if (obstacle_active(d)) { s += wo * d * d; act = true; }
  }
  *active = act;
  return 0.5 * s;
}

// min(a, b) that keeps a NaN from either side: a non-finite state reports a NaN clearance, whichever point or slot it enters at
__device__ __forceinline__ double obstacle_min(double a, double b) { return (a != a || b >= a) ? a : b; }

// min_o d_ko of one point over the slots with w != 0 (+inf without one; NaN if any distance is)
template <bool GRID>
__device__ __forceinline__ double obstacle_point_clearance(const ObstacleCostDev& ob, int k, const double* p, const double* geom, const double* w) {
  double best = INFINITY;
  for (int o = 0; o < ob.no; ++o) {
    if (w[o] == 0.0) continue;
    double d, u[3];
    (void)obstacle_distance<GRID>(ob, ob.kind[o], geom + 4 * o, p, ob.radius[k], &d, u);
    best = obstacle_min(best, d);
  }
  return best;
}

// What the lanes of one wave leave each other for the derivatives at one configuration (lin_obstacle_cost_kernel, phase 2):
// lanes j < nj their joint (rbd::stage_joint_lane), the active lanes their point
struct ObstacleWaveLds {
  JointWorldLds jw;                            // a_j, o_j, the paths, R_0
  double p[DDP_HIP_MAX_COLLISION_POINTS][3];   // p_k of the active points
  double g[DDP_HIP_MAX_COLLISION_POINTS][3];   // g_k = sum_o w e u
  double M[DDP_HIP_MAX_COLLISION_POINTS][6];   // M_k = sum_o w u u^T: xx xy xz yy yz zz
  int idx[DDP_MAXJ];                           // the tangent columns of the active points' paths, ascending
};

// g_k and M_k of one point over its slots in ascending order, the pairs with w == 0 or e == 0 left out (and a sphere's centre at
// p: no direction).  Returns whether any pair took part
template <bool GRID>
__device__ __forceinline__ bool obstacle_point_reduce(const ObstacleCostDev& ob, int k, const double* p, const double* geom, const double* w,
                                                      double* g, double* M) {
  bool act = false;
  g[0] = g[1] = g[2] = 0.0;
  M[0] = M[1] = M[2] = M[3] = M[4] = M[5] = 0.0;
  for (int o = 0; o < ob.no; ++o) {
    const double wo = w[o];
    if (wo == 0.0) continue;
    double d, u[3];
    const bool has_u = obstacle_distance<GRID>(ob, ob.kind[o], geom + 4 * o, p, ob.radius[k], &d, u);
    if (!obstacle_active(d) || !has_u) continue;
    const double we = wo * d;
    g[0] += we * u[0]; g[1] += we * u[1]; g[2] += we * u[2];
    M[0] += wo * u[0] * u[0]; M[1] += wo * u[0] * u[1]; M[2] += wo * u[0] * u[2];
    M[3] += wo * u[1] * u[1]; M[4] += wo * u[1] * u[2]; M[5] += wo * u[2] * u[2];
    act = true;
  }
  return act;
}

// Phase 2, last step: the wave (lane tid of nt) adds, over the nu tangent columns of S.idx (the union of the active points'
// paths) alone,
//   gx[i] += sum_k P_k[:, i] . g_k,      gxx[i][j] += sum_k P_k[:, min]^T M_k P_k[:, max]      (Gauss-Newton)
// the active points (bit k of `active`) in ascending order, a point off whose path i or j lies left out, entry (i, j) in
// (min, max) order: the block stays symmetric bit for bit.  The columns of P_k are formed on the fly (rbd::point_column)
__device__ __forceinline__ void obstacle_add_wave(const DevModel& m, const ObstacleWaveLds& S, const ObstacleCostDev& ob, unsigned active, int nu,
                                                  int tid, int nt, int n, double* gx, double* gxx) {
  const bool ff = m.ff != 0;
  for (int r = tid; r < nu; r += nt) {
    const int i = S.idx[r];
    double s = 0.0;
    for (int k = 0; k < ob.np; ++k) {
      if (!((active >> k) & 1) || !((tangent_mask(ff, S.jw.mask[ob.joint[k]]) >> i) & 1)) continue;
      double c[3];
      point_column(m, ff, S.jw, i, S.p[k], c);
      s += c[0] * S.g[k][0] + c[1] * S.g[k][1] + c[2] * S.g[k][2];
    }
    gx[i] += s;
  }
  for (int e = tid; e < nu * nu; e += nt) {
    const int i = S.idx[e % nu], j = S.idx[e / nu];
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    double h = 0.0;
    bool hit = false;
    for (int k = 0; k < ob.np; ++k) {
      if (!((active >> k) & 1)) continue;
      const unsigned long long tm = tangent_mask(ff, S.jw.mask[ob.joint[k]]);
      if (!((tm >> i) & 1) || !((tm >> j) & 1)) continue;
      double cl[3], ch[3];
      point_column(m, ff, S.jw, lo, S.p[k], cl);
      point_column(m, ff, S.jw, hi, S.p[k], ch);
      const double* M = S.M[k];
      const double t0 = M[0] * ch[0] + M[1] * ch[1] + M[2] * ch[2];
      const double t1 = M[1] * ch[0] + M[3] * ch[1] + M[4] * ch[2];
      const double t2 = M[2] * ch[0] + M[4] * ch[1] + M[5] * ch[2];
      h += cl[0] * t0 + cl[1] * t1 + cl[2] * t2;
      hit = true;
    }
    if (hit) gxx[i + (int64_t)j * n] += h;
  }
}

}  // namespace rbd
