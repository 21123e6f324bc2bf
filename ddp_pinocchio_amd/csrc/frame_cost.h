// frame_cost.h -- per-instance frame-position costs (DDP_HIP_FLAG_FRAME_COST, ddp_hip.h) and frame-orientation costs
// (DDP_HIP_FLAG_FRAME_ORIENT_COST): the kernel-side description and the jacobians they need (the walks for the values,
// rbd::frame_point and rbd::frame_rotation, are frame_walk.h's).  The terms themselves are formed in fwd.hip (cost values) and
// lin.hip (derivatives).
#pragma once
#include "frame_walk.h"
#include "internal.h"
#include "lie.h"
#include "rbd.h"

// What a kernel reads of the context's frame cost.  target == nullptr: no terms (the flag is off, no frames are set, or no
// non-zero weight is resident: the block's CostBlock::live).  oquat == nullptr: no orientation terms, alike (their own block); the
// two sides are independent, and nf / joint are filled when either is live
struct FrameCostDev {
  const double *target, *weight;   // [batch][T+1][nf][3]
  const double *oquat, *oweight;   // [batch][T+1][nf][4] (unit quaternions x y z w), [batch][T+1][nf][3]
  int32_t nf, pad_;
  int32_t joint[DDP_HIP_MAX_COST_FRAMES];
  double off[DDP_HIP_MAX_COST_FRAMES][3];
};

inline FrameCostDev frame_cost_dev(const ddp_hip_ctx* ctx) {
  FrameCostDev f{};
  const CostBlock &fc = ctx->cost[COST_FRAME], &fo = ctx->cost[COST_ORIENT];
  if (!fc.live && !fo.live) return f;
  if (fc.live) { f.target = fc.side[0]; f.weight = fc.side[1]; }
  if (fo.live) { f.oquat = fo.side[0]; f.oweight = fo.side[1]; }
  f.nf = ctx->fc_nf;
  for (int k = 0; k < ctx->fc_nf; ++k) {
    f.joint[k] = ctx->fc_joint[k];
    for (int a = 0; a < 3; ++a) f.off[k][a] = ctx->fc_off[k][a];
  }
  return f;
}

namespace rbd {

// The frame's world position p and its true point jacobian P = dp / d(delta q) (3 x nv, stored at P[3 * column + row]; only
// the columns of the joints on the path root .. joint are written, their tangent indices are returned as a bit mask):
//   revolute joint i: a_i x (p - o_i), prismatic: a_i (world axis a_i, world origin o_i of joint i);
//   free-flyer root (body twists, linear part first): R_0 e_c and (R_0 e_c) x (p - o_0).
// Not rbd::frame_position's rows: those are the reference's WORLD-frame rows, whose lever arm goes to the world origin.
// chain, aw, ow: room for the path, its world axes (9 + 3 * joints doubles: a free-flyer root's rotation comes first) and its
// world origins (3 * joints doubles)
__device__ inline unsigned long long frame_point_jacobian(const DevModel& m, int joint, const double* off, const double* q, double* p,
                                                          double* P, int* chain, double* aw, double* ow) {
  int len = 0;
  for (int j = joint; j >= 0; j = m.parent[j]) chain[len++] = j;
  double oR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, op[3] = {0, 0, 0};
  for (int c = len - 1; c >= 0; --c) {
    const int i = chain[c];
    double E[9], r[3], Rc[9], t[3], nR[9];
    place(m, i, q, E, r);
    for (int k = 0; k < 3; ++k)
      for (int l = 0; l < 3; ++l) Rc[3 * k + l] = E[3 * l + k];
    mv3(oR, r, t);
    op[0] += t[0]; op[1] += t[1]; op[2] += t[2];
    mm3(oR, Rc, nR);
    for (int k = 0; k < 9; ++k) oR[k] = nR[k];
    if (i == 0 && m.ff) {
      for (int k = 0; k < 9; ++k) aw[k] = oR[k];             // the root's rotation: its columns are R_0 e_c
    } else {
      mv3(oR, m.axis[i], aw + 9 + 3 * c);
    }
    ow[3 * c] = op[0]; ow[3 * c + 1] = op[1]; ow[3 * c + 2] = op[2];
  }
  double t[3];
  mv3(oR, off, t);
  p[0] = op[0] + t[0]; p[1] = op[1] + t[1]; p[2] = op[2] + t[2];
  unsigned long long mask = 0;
  for (int c = len - 1; c >= 0; --c) {
    const int i = chain[c];
    const double lever[3] = {p[0] - ow[3 * c], p[1] - ow[3 * c + 1], p[2] - ow[3 * c + 2]};
    if (i == 0 && m.ff) {
      for (int cc = 0; cc < 3; ++cc) {
        const double e[3] = {aw[cc], aw[3 + cc], aw[6 + cc]};
        P[3 * cc] = e[0]; P[3 * cc + 1] = e[1]; P[3 * cc + 2] = e[2];
        cross3(e, lever, P + 3 * (3 + cc));
      }
      mask |= 63ull;
    } else {
      const int vi = m.ff ? i + 5 : i;
      const double* a = aw + 9 + 3 * c;
      if (m.jtype[i] == DDP_HIP_JOINT_REVOLUTE) cross3(a, lever, P + 3 * vi);
      else { P[3 * vi] = a[0]; P[3 * vi + 1] = a[1]; P[3 * vi + 2] = a[2]; }
      mask |= 1ull << vi;
    }
  }
  return mask;
}

// The frame's world rotation R (row-major) and its world angular jacobian W = d(world rotation vector) / d(delta q) (3 x nv,
// stored at W[3 * column + row]; only the columns that carry rotation are written, their tangent indices are returned as a bit
// mask): the world axis a_i of a revolute joint i on the path root .. joint, R_0 e_c for the angular columns 3 .. 5 of a
// free-flyer root; a prismatic joint and the root's linear columns 0 .. 2 have no column.  chain: room for the path
__device__ inline unsigned long long frame_rotation_jacobian(const DevModel& m, int joint, const double* q, double* R, double* W, int* chain) {
  int len = 0;
  for (int j = joint; j >= 0; j = m.parent[j]) chain[len++] = j;
  double oR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  unsigned long long mask = 0;
  for (int c = len - 1; c >= 0; --c) {
    const int i = chain[c];
    double E[9], r[3], Rc[9], nR[9];
    place(m, i, q, E, r);
    for (int k = 0; k < 3; ++k)
      for (int l = 0; l < 3; ++l) Rc[3 * k + l] = E[3 * l + k];
    mm3(oR, Rc, nR);
    for (int k = 0; k < 9; ++k) oR[k] = nR[k];
    if (i == 0 && m.ff) {
      for (int cc = 0; cc < 3; ++cc) { W[3 * (3 + cc)] = oR[cc]; W[3 * (3 + cc) + 1] = oR[3 + cc]; W[3 * (3 + cc) + 2] = oR[6 + cc]; }
      mask |= 56ull;
    } else if (m.jtype[i] == DDP_HIP_JOINT_REVOLUTE) {
      const int vi = m.ff ? i + 5 : i;
      mv3(oR, m.axis[i], W + 3 * vi);
      mask |= 1ull << vi;
    }
  }
  for (int k = 0; k < 9; ++k) R[k] = oR[k];
  return mask;
}

}  // namespace rbd
