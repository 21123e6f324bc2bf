// com_cost.h -- per-instance centre-of-mass costs (DDP_HIP_FLAG_COM_COST, ddp_hip.h): the kernel-side description and the
// traversals they need.  The terms themselves are formed by kernels of their own in fwd.hip (cost values: com_cost_kernel,
// com_sum_kernel) and lin.hip (derivatives: lin_com_cost_kernel); model_api.hip evaluates one configuration with the same code.
#pragma once
#include "frame_walk.h"
#include "internal.h"
#include "lie.h"
#include "rbd.h"

// What a kernel reads of the context's CoM cost.  target == nullptr: no terms (the flag is off, or no non-zero weight has been
// uploaded: the block's CostBlock::live)
struct CoMCostDev {
  const double *target, *weight;   // [batch][T+1][3]
};

inline CoMCostDev com_cost_dev(const ddp_hip_ctx* ctx) {
  CoMCostDev c{};
  const CostBlock& k = ctx->cost[COST_COM];
  if (k.live) { c.target = k.side[0]; c.weight = k.side[1]; }
  return c;
}

namespace rbd {

// What the lanes of one wave leave each other for one configuration: lane j's joint in slot j
struct CoMWaveLds {
  JointWorldLds jw;                    // a_j, o_j (the joint frame's origin, a world point of the joint's axis), the paths, R_0
  double m[DDP_MAXJ];                  // body mass m_j
  double mp[DDP_MAXJ][3];              // m_j p_j, p_j the world position of the body's CoM
  double J[3 * DDP_MAXJ];              // Jc, stored at J[3 * column + row]
  double c[3];                         // c(q)
};

// Body j's mass, and m_j c_j, as the packed spatial inertia holds them (ctx.hip: pack_body_inertia; rows 3 .. 5, columns 0 .. 2
// are m [c]x^T)
template <class M>
__device__ __forceinline__ double body_mass_com(const M& m, int j, double* mc) {
  const double* I = m.I6[j];
  mc[0] = I[12]; mc[1] = I[15]; mc[2] = I[7];
  return I[9];
}

// m_j p_j and m_j of joint j alone: what the value of c(q) needs (no axis, no mask).  The walk carries o, the origin of the
// joint's frame (a point), and d = m_j c_j (a direction: rotations alone, so that m_j p_j = m_j o + d needs no division by a
// mass that may be 0)
template <class M>
__device__ __forceinline__ double com_body_point(const M& m, bool ff, int j, const double* q, double* mp) {
  double o[1][3] = {{0.0, 0.0, 0.0}}, d[1][3];
  const double mass = body_mass_com(m, j, d[0]);
  (void)walk_to_root<1, 1>(m, ff, j, q, o, d, -1);
  mp[0] = mass * o[0][0] + d[0][0]; mp[1] = mass * o[0][1] + d[0][1]; mp[2] = mass * o[0][2] + d[0][2];
  return mass;
}

// c = (sum_j m_j p_j) / (sum_j m_j) over the nj records mass[j], mp[3 j ..], joints in ascending order: the one order in which
// every kernel forms the sums, whichever lane does
__device__ __forceinline__ void com_fold(const double* mass, const double* mp, int nj, double* c) {
  double M = 0.0, s[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < nj; ++i) { M += mass[i]; s[0] += mp[3 * i]; s[1] += mp[3 * i + 1]; s[2] += mp[3 * i + 2]; }
  c[0] = s[0] / M; c[1] = s[1] / M; c[2] = s[2] / M;
}

// Jc by a wave, step 1 of 2: lane j < nj walks its joint's path once, m_j c_j riding along, and leaves its record in S.  (A
// workgroup barrier follows.)  Both steps come in a form that takes the record's parts: the balance-region kernels keep the same
// records inside the momentum's staged record (balance_region_cost.h)
__device__ __forceinline__ void com_stage_lane(const DevModel& m, const double* q, int j, JointWorldLds& jw, double* sm, double (*smp)[3]) {
  double d[1][3];
  const double mass = body_mass_com(m, j, d[0]);
  stage_joint_lane<1>(m, q, j, jw, d);
  sm[j] = mass;
#pragma unroll
  for (int k = 0; k < 3; ++k) smp[j][k] = mass * jw.o[j][k] + d[0][k];
}
__device__ __forceinline__ void com_stage_lane(const DevModel& m, const double* q, int j, CoMWaveLds& S) { com_stage_lane(m, q, j, S.jw, S.m, S.mp); }

// ... step 2 of 2: lane j < nj forms the mass and the first moment of its subtree by running over the records in ascending
// order and testing bit j of each record's path (a fixed order, no atomics), the totals alike, and from them its column(s) of
// Jc; lane 0 leaves c(q) as well.  The column is (f a_j) x lever, not point_column's a_j x lever scaled by f afterwards: scaling
// before the cross product rounds differently from scaling after it.  (A workgroup barrier follows.)
__device__ __forceinline__ void com_column_lane(const DevModel& m, int j, const JointWorldLds& W, const double* sm, const double (*smp)[3],
                                                double* sJ, double* sc) {
  const int nj = m.nj;
  double M = 0.0, tot[3] = {0.0, 0.0, 0.0}, msub = 0.0, sub[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < nj; ++i) {
    const double mi = sm[i];
    M += mi; tot[0] += smp[i][0]; tot[1] += smp[i][1]; tot[2] += smp[i][2];
    if ((W.mask[i] >> j) & 1) { msub += mi; sub[0] += smp[i][0]; sub[1] += smp[i][1]; sub[2] += smp[i][2]; }
  }
  if (j == 0) { sc[0] = tot[0] / M; sc[1] = tot[1] / M; sc[2] = tot[2] / M; }
  const double f = msub / M;
  double lever[3] = {0.0, 0.0, 0.0};
  if (msub != 0.0) { lever[0] = sub[0] / msub - W.o[j][0]; lever[1] = sub[1] / msub - W.o[j][1]; lever[2] = sub[2] / msub - W.o[j][2]; }
  if (j == 0 && m.ff) {
    // the free-flyer root (body twists, linear part first): its subtree is the whole robot, f = 1 and lever = c - o_0
    for (int cc = 0; cc < 3; ++cc) {
      const double e[3] = {f * W.R0[cc], f * W.R0[3 + cc], f * W.R0[6 + cc]};
      sJ[3 * cc] = e[0]; sJ[3 * cc + 1] = e[1]; sJ[3 * cc + 2] = e[2];
      cross3(e, lever, sJ + 3 * (3 + cc));
    }
    return;
  }
  const int vi = m.ff ? j + 5 : j;
  const double fa[3] = {f * W.a[j][0], f * W.a[j][1], f * W.a[j][2]};
  if (m.jtype[j] == DDP_HIP_JOINT_REVOLUTE) cross3(fa, lever, sJ + 3 * vi);
  else { sJ[3 * vi] = fa[0]; sJ[3 * vi + 1] = fa[1]; sJ[3 * vi + 2] = fa[2]; }
}
__device__ __forceinline__ void com_column_lane(const DevModel& m, int j, CoMWaveLds& S) { com_column_lane(m, j, S.jw, S.m, S.mp, S.J, S.c); }

}  // namespace rbd
