// control_grav_cost.h -- per-instance gravity-compensated control costs (DDP_HIP_FLAG_CONTROL_GRAV_COST, ddp_hip.h): the
// kernel-side description, the wave's record of one configuration, and the gravity torque g(q) and its jacobian G formed from it.
// The terms themselves are formed by kernels of their own in fwd.hip (cost values: control_grav_cost_kernel, summed by
// com_sum_kernel) and lin.hip (derivatives: lin_control_grav_cost_kernel); model_api.hip evaluates one configuration with the
// same code.  The walk and the staged joint record are frame_walk.h's, a body's mass and first moment com_cost.h's.
#pragma once
#include "com_cost.h"
#include "frame_walk.h"
#include "internal.h"
#include "rbd.h"

// What a kernel reads of the context's control-gravity cost.  weight == nullptr: no terms (the flag is off, or no non-zero weight
// has been uploaded: the block's CostBlock::live)
struct ControlGravDev {
  const double *offset, *weight;   // [batch][T][m]: t < T alone (CostDesc::stage_only)
};

inline ControlGravDev control_grav_dev(const ddp_hip_ctx* ctx) {
  ControlGravDev c{};
  const CostBlock& k = ctx->cost[COST_CONTROL_GRAV];
  if (k.live) { c.offset = k.side[0]; c.weight = k.side[1]; }
  return c;
}

namespace rbd {

// With F = -gravity and sub(k) the bodies that tangent k moves, tangent k has
//   D_k = a_k x sum_sub m_b (p_b - o_k)   (rotation about the world axis a_k through o_k),      m_sub a_k   (translation along a_k)
// the change of the robot's first moment per unit of delta q_k, and g_k = F . D_k.  Turning an ancestor-or-same tangent c turns
// D_i as a whole, so dg_i / d(delta q_c) = F . (a_c x D_i) = a_c . (D_i x F); moving a strict descendant c changes the first
// moment below i by D_c, so dg_i / d(delta q_c) = F . (a_i x D_c) = a_i . (D_c x F).  A translation turns nothing: such a tangent
// on the ancestor side gives an entry that is identically zero, and it is left out.

// What the lanes of one wave leave each other of one configuration: lane j's joint in slot j, then by tangent index k
struct GravWaveLds {
  JointWorldLds jw;                    // a_j, o_j, the paths, R_0
  double m[DDP_MAXJ];                  // body mass m_j
  double mp[DDP_MAXJ][3];              // m_j p_j, p_j the world position of the body's CoM
  double ax[DDP_MAXJ][3];              // by tangent: the world rotation axis (a translation's: never read)
  double E[DDP_MAXJ][3];               // by tangent: D_k x F
  double g[DDP_MAXJ];                  // by tangent: g_k = F . D_k
  unsigned long long anc[DDP_MAXJ];    // by tangent: the rotational tangents of the joints on the path root .. joint(k), joint(k)'s own included
};

// the joint of tangent k: behind a free-flyer root (tangents 0 .. 5) joint j has tangent j + 5
__device__ __forceinline__ int grav_tangent_joint(bool ff, int k) { return ff ? (k < 6 ? 0 : k - 5) : k; }
// tangent k turns what it moves: a revolute joint, a free-flyer root's tangents 3 .. 5
template <class M>
__device__ __forceinline__ bool grav_tangent_rotational(const M& m, bool ff, int k) {
  if (ff && k < 6) return k >= 3;
  return m.jtype[ff ? k - 5 : k] == DDP_HIP_JOINT_REVOLUTE;
}

// Step 1 of 3: lane j < nj walks its joint's path once, m_j c_j riding along, and leaves its record in S.  (A workgroup barrier
// follows.)
__device__ __forceinline__ void grav_stage_lane(const DevModel& m, const double* q, int j, GravWaveLds& S) {
  double d[1][3];
  const double mass = body_mass_com(m, j, d[0]);
  stage_joint_lane<1>(m, q, j, S.jw, d);
  S.m[j] = mass;
#pragma unroll
  for (int k = 0; k < 3; ++k) S.mp[j][k] = mass * S.jw.o[j][k] + d[0][k];
}

// D x F and F . D of one tangent into its slot
__device__ __forceinline__ void grav_tangent_store(GravWaveLds& S, int k, const double* a, const double* D, const double* F) {
  cross3(D, F, S.E[k]);
  S.g[k] = dot3(F, D);
  S.ax[k][0] = a[0]; S.ax[k][1] = a[1]; S.ax[k][2] = a[2];
}

// Step 2 of 3: lane j < nj forms the mass and the first moment of its subtree by running over the records in ascending order and
// testing bit j of each record's path (a fixed order, no atomics), and from them D, E and g of its tangent -- a free-flyer root
// of its six; rot: the rotational tangents as a mask.  Every lane k < nv leaves anc[k].  (A workgroup barrier follows.)
__device__ __forceinline__ void grav_tangent_lane(const DevModel& m, int tid, unsigned long long rot, GravWaveLds& S) {
  const bool ff = m.ff != 0;
  const JointWorldLds& W = S.jw;
  if (tid < m.nv) S.anc[tid] = tangent_mask(ff, W.mask[grav_tangent_joint(ff, tid)]) & rot;
  if (tid >= m.nj) return;
  const int j = tid, nj = m.nj;
  const double F[3] = {-m.gravity[0], -m.gravity[1], -m.gravity[2]};
  double msub = 0.0, sub[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < nj; ++i)
    if ((W.mask[i] >> j) & 1) { msub += S.m[i]; sub[0] += S.mp[i][0]; sub[1] += S.mp[i][1]; sub[2] += S.mp[i][2]; }
  const double L[3] = {sub[0] - msub * W.o[j][0], sub[1] - msub * W.o[j][1], sub[2] - msub * W.o[j][2]};   // the first moment about o_j
  if (j == 0 && ff) {
    // the free-flyer root (body twists, linear part first): the whole robot along, then about, R_0 e_c
    for (int c = 0; c < 3; ++c) {
      const double e[3] = {W.R0[c], W.R0[3 + c], W.R0[6 + c]};
      const double Dl[3] = {msub * e[0], msub * e[1], msub * e[2]};
      double Dr[3];
      cross3(e, L, Dr);
      grav_tangent_store(S, c, e, Dl, F);
      grav_tangent_store(S, 3 + c, e, Dr, F);
    }
    return;
  }
  const double* a = W.a[j];
  double D[3];
  if (m.jtype[j] == DDP_HIP_JOINT_REVOLUTE) cross3(a, L, D);
  else { D[0] = msub * a[0]; D[1] = msub * a[1]; D[2] = msub * a[2]; }
  grav_tangent_store(S, ff ? j + 5 : j, a, D, F);
}

// Step 3 of 3: G_ic = dg_i / d(delta q_c) from the record -> the entry is on the pattern (else *val is left as it is).  On a
// fixed base (i, c) and (c, i) read the same two slots: G is symmetric bit for bit
__device__ __forceinline__ bool grav_entry(const GravWaveLds& S, bool ff, int i, int c, double* val) {
  if ((S.anc[i] >> c) & 1) { *val = dot3(S.ax[c], S.E[i]); return true; }                // c's joint is i's or an ancestor of it
  const bool same = ff ? (i < 6 && c < 6) : i == c;
  if (!same && ((S.anc[c] >> i) & 1)) { *val = dot3(S.ax[i], S.E[c]); return true; }     // c's joint is a strict descendant
  return false;
}

// g(q) alone, over the lanes of one group (the value kernel: `lpe` lanes per state, lane j the joint j): what lane j leaves the
// others -- mass, m_j p_j, the path -- and keeps for itself -- a_j, o_j
struct GravLane {
  double a[3], o[3];
};
template <class M>
__device__ __forceinline__ void grav_value_stage(const M& m, bool ff, int j, const double* q, double* mass, double* mp, unsigned long long* mask,
                                                 GravLane& own) {
  const bool root = j == 0 && ff;
  double o[1][3] = {{0.0, 0.0, 0.0}}, d[2][3];
  const double mj = body_mass_com(m, j, d[1]);
#pragma unroll
  for (int k = 0; k < 3; ++k) d[0][k] = root ? 0.0 : m.axis[j][k];
  *mask = walk_to_root<1, 2>(m, ff, j, q, o, d, 0);
  *mass = mj;
#pragma unroll
  for (int k = 0; k < 3; ++k) { mp[k] = mj * o[0][k] + d[1][k]; own.a[k] = d[0][k]; own.o[k] = o[0][k]; }
}
// ... and g of joint j's tangent (never a free-flyer root's: its rows carry no term) from the group's records, joints ascending
template <class M>
__device__ __forceinline__ double grav_value_joint(const M& m, int j, const double* mass, const double* mp, const unsigned long long* mask,
                                                   const GravLane& own) {
  const double F[3] = {-m.gravity[0], -m.gravity[1], -m.gravity[2]};
  double msub = 0.0, sub[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < m.nj; ++i)
    if ((mask[i] >> j) & 1) { msub += mass[i]; sub[0] += mp[3 * i]; sub[1] += mp[3 * i + 1]; sub[2] += mp[3 * i + 2]; }
  const double L[3] = {sub[0] - msub * own.o[0], sub[1] - msub * own.o[1], sub[2] - msub * own.o[2]};
  double D[3];
  if (m.jtype[j] == DDP_HIP_JOINT_REVOLUTE) cross3(own.a, L, D);
  else { D[0] = msub * own.a[0]; D[1] = msub * own.a[1]; D[2] = msub * own.a[2]; }
  return dot3(F, D);
}

}  // namespace rbd
