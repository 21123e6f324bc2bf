// com_cost.h -- per-instance centre-of-mass costs (DDP_HIP_FLAG_COM_COST, ddp_hip.h): the kernel-side description and the
// traversals they need.  The terms themselves are formed by kernels of their own in fwd.hip (cost values: com_cost_kernel,
// com_sum_kernel) and lin.hip (derivatives: lin_com_cost_kernel); model_api.hip evaluates one configuration with the same code.
#pragma once
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
  double m[DDP_MAXJ];                  // body mass m_j
  double mp[DDP_MAXJ][3];              // m_j p_j, p_j the world position of the body's CoM
  double a[DDP_MAXJ][3], o[DDP_MAXJ][3];   // world axis a_j, a world point o_j of the joint's axis (the joint frame's origin)
  unsigned long long mask[DDP_MAXJ];   // bit i: joint i is on the path root .. j (j itself included)
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

// v <- R_axis(angle) v, by the sine and cosine of the angle (Rodrigues, as frame_point forms it)
__device__ __forceinline__ void com_rotate(const double* a, double s, double omc, double* v) {
  double av[3], aav[3];
  cross3(a, v, av);
  cross3(a, av, aav);
  v[0] += s * av[0] + omc * aav[0]; v[1] += s * av[1] + omc * aav[1]; v[2] += s * av[2] + omc * aav[2];
}

// Joint `joint` seen from the world, walking joint -> root like frame_point with three vectors and no placements kept:
//   o: the origin of the joint's frame (a point: rotations and translations), d: m_j c_j (a direction: rotations alone, so
//   that m_j p_j = m_j o + d needs no division by a mass that may be 0), a: the joint's axis (a direction; 0 on a free-flyer
//   root).  Returns the path as a bit mask over joints.  M: DevModel or CoopModel
template <class M>
__device__ __forceinline__ unsigned long long com_walk(const M& m, bool ff, int joint, const double* q, double* o, double* d, double* a,
                                                       double* mass) {
  *mass = body_mass_com(m, joint, d);
  o[0] = o[1] = o[2] = 0.0;
  if (joint == 0 && ff) { a[0] = a[1] = a[2] = 0.0; }
  else { a[0] = m.axis[joint][0]; a[1] = m.axis[joint][1]; a[2] = m.axis[joint][2]; }
  unsigned long long mask = 0;
  for (int j = joint; j >= 0; j = m.parent[j]) {
    mask |= 1ull << j;
    double w[3];
    if (j == 0 && ff) {
      double R[9];
      lie::quat_to_R(q + 3, R);
      mv3(R, o, w); o[0] = w[0] + q[0]; o[1] = w[1] + q[1]; o[2] = w[2] + q[2];
      mv3(R, d, w); d[0] = w[0]; d[1] = w[1]; d[2] = w[2];
      mv3(R, a, w); a[0] = w[0]; a[1] = w[1]; a[2] = w[2];
      break;
    }
    const double* ax = m.axis[j];
    const double qj = q[ff ? j + 6 : j];
    if (m.jtype[j] == DDP_HIP_JOINT_REVOLUTE) {
      double s, c;
      sincos(qj, &s, &c);
      const double omc = 1.0 - c;
      com_rotate(ax, s, omc, o);
      com_rotate(ax, s, omc, d);
      if (j != joint) com_rotate(ax, s, omc, a);           // (a joint's own rotation leaves its axis where it is)
    } else {
      o[0] += ax[0] * qj; o[1] += ax[1] * qj; o[2] += ax[2] * qj;
    }
    mv3(m.Rp[j], o, w); o[0] = w[0] + m.pp[j][0]; o[1] = w[1] + m.pp[j][1]; o[2] = w[2] + m.pp[j][2];
    mv3(m.Rp[j], d, w); d[0] = w[0]; d[1] = w[1]; d[2] = w[2];
    mv3(m.Rp[j], a, w); a[0] = w[0]; a[1] = w[1]; a[2] = w[2];
  }
  return mask;
}

// m_j p_j and m_j of joint j alone: what the value of c(q) needs (no axis, no mask)
template <class M>
__device__ __forceinline__ double com_body_point(const M& m, bool ff, int j, const double* q, double* mp) {
  double o[3], d[3], a[3], mass;
  (void)com_walk(m, ff, j, q, o, d, a, &mass);
  mp[0] = mass * o[0] + d[0]; mp[1] = mass * o[1] + d[1]; mp[2] = mass * o[2] + d[2];
  return mass;
}

// c = (sum_j m_j p_j) / (sum_j m_j) over the nj records mass[j], mp[3 j ..], joints in ascending order: the one order in which
// every kernel forms the sums, whichever lane does
__device__ __forceinline__ void com_fold(const double* mass, const double* mp, int nj, double* c) {
  double M = 0.0, s[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < nj; ++i) { M += mass[i]; s[0] += mp[3 * i]; s[1] += mp[3 * i + 1]; s[2] += mp[3 * i + 2]; }
  c[0] = s[0] / M; c[1] = s[1] / M; c[2] = s[2] / M;
}

// Jc by a wave, step 1 of 2: lane j < nj walks its joint's path once and leaves its record in S.  (A workgroup barrier follows.)
__device__ __forceinline__ void com_stage_lane(const DevModel& m, const double* q, int j, CoMWaveLds& S) {
  double o[3], d[3], a[3], mass;
  S.mask[j] = com_walk(m, m.ff != 0, j, q, o, d, a, &mass);
  S.m[j] = mass;
#pragma unroll
  for (int k = 0; k < 3; ++k) { S.mp[j][k] = mass * o[k] + d[k]; S.a[j][k] = a[k]; S.o[j][k] = o[k]; }
}

// ... step 2 of 2: lane j < nj forms the mass and the first moment of its subtree by running over the records in ascending
// order and testing bit j of each record's path (a fixed order, no atomics), the totals alike, and from them its column(s) of
// Jc; lane 0 leaves c(q) as well.  (A workgroup barrier follows.)
__device__ __forceinline__ void com_column_lane(const DevModel& m, const double* q, int j, CoMWaveLds& S) {
  const int nj = m.nj;
  double M = 0.0, tot[3] = {0.0, 0.0, 0.0}, msub = 0.0, sub[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < nj; ++i) {
    const double mi = S.m[i];
    M += mi; tot[0] += S.mp[i][0]; tot[1] += S.mp[i][1]; tot[2] += S.mp[i][2];
    if ((S.mask[i] >> j) & 1) { msub += mi; sub[0] += S.mp[i][0]; sub[1] += S.mp[i][1]; sub[2] += S.mp[i][2]; }
  }
  if (j == 0) { S.c[0] = tot[0] / M; S.c[1] = tot[1] / M; S.c[2] = tot[2] / M; }
  const double f = msub / M;
  double lever[3] = {0.0, 0.0, 0.0};
  if (msub != 0.0) { lever[0] = sub[0] / msub - S.o[j][0]; lever[1] = sub[1] / msub - S.o[j][1]; lever[2] = sub[2] / msub - S.o[j][2]; }
  if (j == 0 && m.ff) {
    // the free-flyer root (body twists, linear part first): its subtree is the whole robot, f = 1 and lever = c - o_0
    double R[9];
    lie::quat_to_R(q + 3, R);
    for (int cc = 0; cc < 3; ++cc) {
      const double e[3] = {f * R[cc], f * R[3 + cc], f * R[6 + cc]};
      S.J[3 * cc] = e[0]; S.J[3 * cc + 1] = e[1]; S.J[3 * cc + 2] = e[2];
      cross3(e, lever, S.J + 3 * (3 + cc));
    }
    return;
  }
  const int vi = m.ff ? j + 5 : j;
  const double fa[3] = {f * S.a[j][0], f * S.a[j][1], f * S.a[j][2]};
  if (m.jtype[j] == DDP_HIP_JOINT_REVOLUTE) cross3(fa, lever, S.J + 3 * vi);
  else { S.J[3 * vi] = fa[0]; S.J[3 * vi + 1] = fa[1]; S.J[3 * vi + 2] = fa[2]; }
}

}  // namespace rbd
