// self_collision_cost.h -- per-instance self-collision costs (DDP_HIP_FLAG_SELF_COLLISION_COST, ddp_hip.h): pairs of spheres on
// the robot, a one-sided penalty on their distance.  The kernel-side description and the device helpers; the terms themselves are
// formed by kernels of their own in fwd.hip (cost values: self_collision_cost_kernel, summed by com_sum_kernel; clearances:
// self_collision_clearance_kernel) and lin.hip (derivatives: lin_self_collision_cost_kernel).
#pragma once
#include "frame_walk.h"
#include "internal.h"
#include "lie.h"
#include "obstacle_cost.h"
#include "rbd.h"

// What a kernel reads of the context's self-collision cost.  margin == nullptr: no terms (the flag is off, no pairs are set, or
// no non-zero weight has been uploaded: the block's CostBlock::live)
struct SelfCollisionDev {
  const double *margin, *weight;   // [batch][T+1][npair] each
  int32_t np, npair;               // spheres, pairs
  int32_t joint[DDP_HIP_MAX_COLLISION_POINTS];
  uint8_t pa[DDP_HIP_MAX_COLLISION_PAIRS], pb[DDP_HIP_MAX_COLLISION_PAIRS];   // pair i: spheres pa[i], pb[i]
  double off[DDP_HIP_MAX_COLLISION_POINTS][3];
  double radius[DDP_HIP_MAX_COLLISION_POINTS];
};

// always: the description whether or not a weight is live (ddp_hip_self_collision_clearance works from the first set_pairs on)
inline SelfCollisionDev self_collision_dev(const ddp_hip_ctx* ctx, bool always = false) {
  SelfCollisionDev c{};
  const CostBlock& k = ctx->cost[COST_SELF_COLLISION];
  if (!(always ? ctx->sc_npair > 0 : k.live)) return c;
  c.margin = k.side[0];
  c.weight = k.side[1];
  c.np = ctx->sc_np;
  c.npair = ctx->sc_npair;
  for (int s = 0; s < ctx->sc_np; ++s) {
    c.joint[s] = ctx->sc_joint[s];
    c.radius[s] = ctx->sc_radius[s];
    for (int a = 0; a < 3; ++a) c.off[s][a] = ctx->sc_off[s][a];
  }
  for (int i = 0; i < ctx->sc_npair; ++i) { c.pa[i] = (uint8_t)ctx->sc_pa[i]; c.pb[i] = (uint8_t)ctx->sc_pb[i]; }
  return c;
}

namespace rbd {

// The signed distance d_i = |p_a - p_b| - (r_a + r_b + m_i) of pair i and, with u != nullptr, the direction u_i = (p_a - p_b) /
// |p_a - p_b| = dd / dp_a = -dd / dp_b.  Returns false where u does not exist (the centres coincide: the pair has its value and
// no derivative)
__device__ __forceinline__ bool self_collision_distance(const SelfCollisionDev& sc, int i, const double* pa, const double* pb, double margin,
                                                        double* d, double* u) {
  const double x = pa[0] - pb[0], y = pa[1] - pb[1], z = pa[2] - pb[2];
  const double dist = sqrt(x * x + y * y + z * z);
  *d = dist - (sc.radius[sc.pa[i]] + sc.radius[sc.pb[i]] + margin);
  if (dist == 0.0) {
    if (u) u[0] = u[1] = u[2] = 0.0;
    return false;
  }
  if (u) { u[0] = x / dist; u[1] = y / dist; u[2] = z / dist; }
  return true;
}

// What the lanes of one wave leave each other for the derivatives at one configuration (lin_self_collision_cost_kernel, phase 2):
// lanes j < nj their joint (rbd::stage_joint_lane), lanes k < np their sphere, the active pairs' lanes their pair
struct SelfCollisionWaveLds {
  JointWorldLds jw;                                // a_j, o_j, the paths, R_0
  double p[DDP_HIP_MAX_COLLISION_POINTS][3];       // p_k of every sphere
  double u[DDP_HIP_MAX_COLLISION_PAIRS][3];        // of the active pairs: u_i,
  double w[DDP_HIP_MAX_COLLISION_PAIRS];           // w_i,
  double we[DDP_HIP_MAX_COLLISION_PAIRS];          // w_i e_i,
  unsigned long long ca[DDP_HIP_MAX_COLLISION_PAIRS];   // the tangent columns on path(a_i) alone
  unsigned long long cb[DDP_HIP_MAX_COLLISION_PAIRS];   // ... and on path(b_i) alone
  int idx[DDP_MAXJ];                               // the union of them all, ascending
};

// z_i[c] of an active pair at a column c of its symmetric difference: + P_a[:, c] . u_i on a's side, - P_b[:, c] . u_i on b's.
// The column of P is formed on the fly (rbd::point_column)
__device__ __forceinline__ double self_collision_z(const DevModel& m, bool ff, const SelfCollisionWaveLds& S, const SelfCollisionDev& sc, int i,
                                                   int c) {
  const bool on_a = (S.ca[i] >> c) & 1;
  double col[3];
  point_column(m, ff, S.jw, c, S.p[on_a ? sc.pa[i] : sc.pb[i]], col);
  const double z = col[0] * S.u[i][0] + col[1] * S.u[i][1] + col[2] * S.u[i][2];
  return on_a ? z : -z;
}

// Phase 2, last step: the wave (lane tid of nt) adds, over the nu tangent columns of S.idx (the union of the active pairs'
// symmetric differences) alone,
//   gx[c] += sum_i (w e)_i z_i[c],      gxx[r][c] += sum_i w_i z_i[min] z_i[max]      (Gauss-Newton)
// the active pairs (bit i of `active`) in ascending order, a pair outside whose symmetric difference r or c lies left out, entry
// (r, c) in (min, max) order: the block stays symmetric bit for bit.  A column on both paths of a pair is in neither ca nor cb:
// the common ancestors -- a free-flyer root's six columns among them -- are never touched
__device__ __forceinline__ void self_collision_add_wave(const DevModel& m, const SelfCollisionWaveLds& S, const SelfCollisionDev& sc,
                                                        unsigned active, int nu, int tid, int nt, int n, double* gx, double* gxx) {
  const bool ff = m.ff != 0;
  for (int r = tid; r < nu; r += nt) {
    const int c = S.idx[r];
    double s = 0.0;
    for (int i = 0; i < sc.npair; ++i) {
      if (!((active >> i) & 1) || !(((S.ca[i] | S.cb[i]) >> c) & 1)) continue;
      s += S.we[i] * self_collision_z(m, ff, S, sc, i, c);
    }
    gx[c] += s;
  }
  for (int e = tid; e < nu * nu; e += nt) {
    const int r = S.idx[e % nu], c = S.idx[e / nu];
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    double h = 0.0;
    bool hit = false;
    for (int i = 0; i < sc.npair; ++i) {
      if (!((active >> i) & 1)) continue;
      const unsigned long long sd = S.ca[i] | S.cb[i];
      if (!((sd >> r) & 1) || !((sd >> c) & 1)) continue;
      h += S.w[i] * self_collision_z(m, ff, S, sc, i, lo) * self_collision_z(m, ff, S, sc, i, hi);
      hit = true;
    }
    if (hit) gxx[r + (int64_t)c * n] += h;
  }
}

}  // namespace rbd
