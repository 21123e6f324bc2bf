// joint_accel_cost.h -- per-instance joint-acceleration costs (DDP_HIP_FLAG_JOINT_ACCEL_COST, ddp_hip.h): the kernel-side
// description and the forward dynamics of the value kernel.  The terms themselves are formed by kernels of their own in fwd.hip
// (cost values and ddp_hip_joint_accel: joint_accel_cost_kernel, summed by com_sum_kernel) and lin.hip (derivatives:
// lin_joint_accel_cost_kernel, on rbd_deriv.h's ff_derivatives_wave / tree_derivatives_wave).
#pragma once
#include "internal.h"
#include "rbd.h"

// What a kernel reads of the context's joint-acceleration cost.  weight == nullptr: no terms (the flag is off, or no non-zero weight
// has been uploaded: the block's CostBlock::live).  report != nullptr: ddp_hip_joint_accel -- the accelerations themselves go to
// report[trajectory][T][nv], the weights are ignored and no term is formed
struct JointAccelDev {
  const double *target, *weight;   // [batch][T+1][nv]; row T is read by no kernel
  double* report;
};

inline JointAccelDev joint_accel_dev(const ddp_hip_ctx* ctx, bool always = false) {
  JointAccelDev c{};
  const CostBlock& k = ctx->cost[COST_JOINT_ACCEL];
  if (k.live || always) { c.target = k.side[0]; c.weight = k.side[1]; }
  return c;
}

namespace rbd {

// doubles of LDS one evaluation of accel_group takes: the joints' records, then qdd
__host__ __device__ inline int accel_group_words(int nj, int nv) { return ABA_LDS_SLOTS * nj + nv; }

// qdd = aba(q, v, tau) by a group of nh lanes (a power of two, lane h of the group), the work-group's groups in step: the
// level-by-level traversal of aba_tree_coop (the same steps in the same order: aba_tree's arithmetic) with the joints' records at
// st[joint ABA_LDS_SLOTS + slot], a level wider than the group walked in rounds, and the free-flyer root (FF: S = identity on the
// body twist, joint i >= 1 reads q[i + 6], v[i + 5], tau[i + 5]) resolved in pass 3 as aba_tree resolves it.  Every thread of
// the work-group calls it (barriers); a group with live == false does no arithmetic.  Ends with a barrier: qdd (LDS) is visible
template <bool FF>
__device__ void accel_group(const DevModel& m, const double* q, const double* v, const double* tau, double* qdd, double* st, int h, int nh,
                            bool live) {
  auto S = [&](int joint, int slot) -> double& { return st[joint * ABA_LDS_SLOTS + slot]; };
  constexpr int oE = 0, oR = 9, oC = 12, oP = 18, oI = 24, oU = 45, oD = 51, oT = 52, oV = 53;
  constexpr int vo = FF ? 5 : 0;
  const int NL = m.n_levels;
  if (live)
    for (int i = h; i < m.nj; i += nh) {
      double E[9], R[3];
      step_place<FF>(m, i, q, E, R);
#pragma unroll
      for (int k = 0; k < 9; ++k) S(i, oE + k) = E[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) S(i, oR + k) = R[k];
    }
  __syncthreads();
  for (int L = 0; L < NL; ++L) {                 // pass 1, root -> leaves
    if (live)
      for (int idx = m.lvl_start[L] + h; idx < m.lvl_start[L + 1]; idx += nh) {
        const int i = m.lvl_joint[idx];
        double E[9], R[3], vel[6], vp[6], cb[6], pA[6], I6[21];
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = S(i, oE + k);
#pragma unroll
        for (int k = 0; k < 3; ++k) R[k] = S(i, oR + k);
        const int par = m.parent[i];
        if (par >= 0) {
#pragma unroll
          for (int k = 0; k < 6; ++k) vp[k] = S(par, oV + k);
        }
#pragma unroll
        for (int k = 0; k < 21; ++k) I6[k] = m.I6[i][k];
        const bool root = FF && i == 0;
        step_velocity(E, R, m.axis[i], m.jtype[i] == DDP_HIP_JOINT_REVOLUTE, root, root ? v : v + i + vo, par >= 0, vp, I6, vel, cb, pA);
#pragma unroll
        for (int k = 0; k < 6; ++k) { S(i, oV + k) = vel[k]; S(i, oC + k) = cb[k]; S(i, oP + k) = pA[k]; }
#pragma unroll
        for (int k = 0; k < 21; ++k) S(i, oI + k) = I6[k];
      }
    __syncthreads();
  }
  for (int L = NL - 1; L >= 0; --L) {            // pass 2, leaves -> root
    if (live)
      for (int idx = m.lvl_start[L] + h; idx < m.lvl_start[L + 1]; idx += nh) {
        const int i = m.lvl_joint[idx];
        const double* a = m.axis[i];
        const bool rev = m.jtype[i] == DDP_HIP_JOINT_REVOLUTE;
        double IA[21], U[6], pAi[6], cb[6];
#pragma unroll
        for (int k = 0; k < 21; ++k) IA[k] = S(i, oI + k);
#pragma unroll
        for (int k = 0; k < 6; ++k) { pAi[k] = S(i, oP + k); cb[k] = S(i, oC + k); }
        for (int ci = m.child_start[i]; ci < m.child_start[i + 1]; ++ci) {   // contributions, descending child index
          const int c = m.child_list[ci];
#pragma unroll
          for (int k = 0; k < 21; ++k) IA[k] += S(c, oI + k);
#pragma unroll
          for (int k = 0; k < 6; ++k) pAi[k] += S(c, oP + k);
        }
        if (FF && i == 0) {                          // the root's articulated inertia and bias force: resolved in pass 3
#pragma unroll
          for (int k = 0; k < 21; ++k) S(i, oI + k) = IA[k];
#pragma unroll
          for (int k = 0; k < 6; ++k) S(i, oP + k) = pAi[k];
          continue;
        }
        const double dinv = step_U(IA, a, rev, m.armature[i], U);
        const double ui = step_u(pAi, a, rev, tau[i + vo]);
#pragma unroll
        for (int k = 0; k < 6; ++k) S(i, oU + k) = U[k];
        S(i, oD) = dinv;
        S(i, oT) = ui;
        if (m.parent[i] >= 0) {
          double E[9], R[3], Ia[21], fp[6], Z[21];
#pragma unroll
          for (int k = 0; k < 9; ++k) E[k] = S(i, oE + k);
#pragma unroll
          for (int k = 0; k < 3; ++k) R[k] = S(i, oR + k);
          step_Ia(IA, U, dinv, Ia);
          step_force_up(E, R, pAi, cb, U, dinv, ui, Ia, fp);
          step_inertia_up(E, R, Ia, Z);               // this joint's contributions to its parent, left in its own slots
#pragma unroll
          for (int k = 0; k < 21; ++k) S(i, oI + k) = Z[k];
#pragma unroll
          for (int k = 0; k < 6; ++k) S(i, oP + k) = fp[k];
        }
      }
    __syncthreads();
  }
  for (int L = 0; L < NL; ++L) {                 // pass 3, root -> leaves
    if (live)
      for (int idx = m.lvl_start[L] + h; idx < m.lvl_start[L + 1]; idx += nh) {
        const int i = m.lvl_joint[idx];
        double E[9], R[3], ap[6], accp[6], cb[6];
#pragma unroll
        for (int k = 0; k < 9; ++k) E[k] = S(i, oE + k);
#pragma unroll
        for (int k = 0; k < 3; ++k) R[k] = S(i, oR + k);
#pragma unroll
        for (int k = 0; k < 6; ++k) cb[k] = S(i, oC + k);
        const int par = m.parent[i];
        if (par >= 0) {
#pragma unroll
          for (int k = 0; k < 6; ++k) accp[k] = S(par, oV + k);
        }
        step_accel_in(E, R, par >= 0, accp, m.gravity, ap);
        if (FF && i == 0) {
          double IAr[21], pAr[6], qs[6];
#pragma unroll
          for (int k = 0; k < 21; ++k) IAr[k] = S(i, oI + k);
#pragma unroll
          for (int k = 0; k < 6; ++k) pAr[k] = S(i, oP + k);
          step_accel_ff_root(IAr, pAr, tau, cb, ap, qs);
#pragma unroll
          for (int k = 0; k < 6; ++k) qdd[k] = qs[k];
        } else {
          double U[6];
#pragma unroll
          for (int k = 0; k < 6; ++k) U[k] = S(i, oU + k);
          qdd[i + vo] = step_accel(U, cb, S(i, oT), S(i, oD), m.axis[i], m.jtype[i] == DDP_HIP_JOINT_REVOLUTE, ap);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) S(i, oV + k) = ap[k];
      }
    __syncthreads();
  }
}

}  // namespace rbd
