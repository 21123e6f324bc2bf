// momentum_cost.h -- per-instance centroidal-momentum costs (DDP_HIP_FLAG_MOMENTUM_COST, ddp_hip.h): the kernel-side description
// and the traversals they need.  The terms themselves are formed by kernels of their own in fwd.hip (cost values:
// momentum_cost_kernel, summed by com_sum_kernel) and lin.hip (derivatives: lin_momentum_cost_kernel); model_api.hip evaluates one
// state with the same code.  It borrows body_mass_com from com_cost.h and frame_vel_term / vel_add_wave from frame_vel_cost.h: the
// residual has the frame-velocity term's shape (six axes, a delta-q half and a v half), with one "frame" whose path is every joint.
#pragma once
#include "com_cost.h"
#include "frame_vel_cost.h"
#include "frame_walk.h"
#include "internal.h"
#include "lie.h"
#include "rbd.h"

// What a kernel reads of the context's momentum cost.  target == nullptr: no terms (the flag is off, or no non-zero weight has
// been uploaded: the block's CostBlock::live)
struct MomentumCostDev {
  const double *target, *weight;   // [batch][T+1][6]: linear momentum, then angular momentum about the CoM, world axes
};

inline MomentumCostDev momentum_cost_dev(const ddp_hip_ctx* ctx) {
  MomentumCostDev c{};
  const CostBlock& k = ctx->cost[COST_MOMENTUM];
  if (k.live) { c.target = k.side[0]; c.weight = k.side[1]; }
  return c;
}

namespace rbd {

// Body j's rotational inertia about the origin of joint j's frame in world axes, applied to the world vector x: E Io E^T x, E[k]
// the world direction of the frame's axis k and Io = Ic + m [c]x [c]x^T the first rows of the packed spatial inertia
template <class M>
__device__ __forceinline__ void body_inertia_apply(const M& m, int j, const double (*E)[3], const double* x, double* y) {
  const double xb[3] = {dot3(E[0], x), dot3(E[1], x), dot3(E[2], x)};
  double yb[3];
  sym3_mv(m.I6[j], xb, yb);
#pragma unroll
  for (int k = 0; k < 3; ++k) y[k] = yb[0] * E[0][k] + yb[1] * E[1][k] + yb[2] * E[2][k];
}

// Body j's share of the momentum by ONE lane and one walk joint -> root, like frame_velocity: the origin o of joint j's frame, its
// velocity lo, the frame's angular velocity w and d = m_j c_j are carried in the current joint's axes (with `ang` the frame's
// three axes E as well), every joint adds its own rate and rotates them into its parent's axes.  No per-joint arrays, and no
// division by a mass that may be 0.  Leaves
//   mp = m_j p_j = m_j o + d,   ml = m_j pdot_j = m_j lo + w x d,   kO = p_j x m_j pdot_j + I_j w = o x ml + d x lo + E Io E^T w
// (kO about the world origin, with `ang` alone) and returns m_j
__device__ __forceinline__ double momentum_body(const DevModel& m, int joint, const double* q, const double* v, bool ang, double* mp, double* ml,
                                                double* kO) {
  const bool ff = m.ff != 0;
  double o[3] = {0.0, 0.0, 0.0}, lo[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0}, d[3], t[3];
  double E[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const double mass = body_mass_com(m, joint, d);
  for (int j = joint; j >= 0; j = m.parent[j]) {
    if (j == 0 && ff) {
      double R[9];
      lie::quat_to_R(q + 3, R);
      cross3(v + 3, o, t);
      lo[0] += v[0] + t[0]; lo[1] += v[1] + t[1]; lo[2] += v[2] + t[2];
      w[0] += v[3]; w[1] += v[4]; w[2] += v[5];
      dir_to_world(R, lo); dir_to_world(R, w); dir_to_world(R, d);
      if (ang) { dir_to_world(R, E[0]); dir_to_world(R, E[1]); dir_to_world(R, E[2]); }
      point_to_world(R, q, o);
      break;
    }
    const double* a = m.axis[j];
    const double qj = q[ff ? j + 6 : j], vj = v[ff ? j + 5 : j];
    if (m.jtype[j] == DDP_HIP_JOINT_REVOLUTE) {
      double s, c;
      sincos(qj, &s, &c);
      const double omc = 1.0 - c;
      axis_rotate(a, s, omc, o); axis_rotate(a, s, omc, lo); axis_rotate(a, s, omc, w); axis_rotate(a, s, omc, d);
      if (ang) { axis_rotate(a, s, omc, E[0]); axis_rotate(a, s, omc, E[1]); axis_rotate(a, s, omc, E[2]); }
      cross3(a, o, t);
      lo[0] += vj * t[0]; lo[1] += vj * t[1]; lo[2] += vj * t[2];
      w[0] += vj * a[0]; w[1] += vj * a[1]; w[2] += vj * a[2];
    } else {
      o[0] += a[0] * qj; o[1] += a[1] * qj; o[2] += a[2] * qj;
      lo[0] += vj * a[0]; lo[1] += vj * a[1]; lo[2] += vj * a[2];
    }
    point_to_parent(m, j, o);
    dir_to_parent(m, j, lo); dir_to_parent(m, j, w); dir_to_parent(m, j, d);
    if (ang) { dir_to_parent(m, j, E[0]); dir_to_parent(m, j, E[1]); dir_to_parent(m, j, E[2]); }
  }
  cross3(w, d, t);
#pragma unroll
  for (int k = 0; k < 3; ++k) { mp[k] = mass * o[k] + d[k]; ml[k] = mass * lo[k] + t[k]; }
  if (ang) {
    double t1[3], t2[3], t3[3];
    cross3(o, ml, t1);
    cross3(d, lo, t2);
    body_inertia_apply(m, joint, E, w, t3);
#pragma unroll
    for (int k = 0; k < 3; ++k) kO[k] = t1[k] + t2[k] + t3[k];
  }
  return mass;
}

// h = (l, k) from the nj body records rec[10 j ..] = m_j | m_j p_j | m_j pdot_j | kO_j, joints in ascending order: the one order
// in which every kernel forms the sums.  k = kO - c x l about c = sum m_j p_j / sum m_j, with `ang` alone
__device__ __forceinline__ void momentum_fold(const double* rec, int nj, bool ang, double* h) {
  double M = 0.0, s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < nj; ++i) {
    M += rec[10 * i];
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] += rec[10 * i + 1 + k];
  }
  h[0] = s[3]; h[1] = s[4]; h[2] = s[5];
  if (!ang) return;
  const double c[3] = {s[0] / M, s[1] / M, s[2] / M};
  double t[3];
  cross3(c, h, t);
  h[3] = s[6] - t[0]; h[4] = s[7] - t[1]; h[5] = s[8] - t[2];
}

// What the lanes of one wave leave each other for one state: lane j's joint and body in slot j, then the jacobians.  Spatial
// quantities are taken about the world origin; A, cm and idx are laid out as VelWaveLds has them, for vel_add_wave
struct MomWaveLds {
  JointWorldLds jw;                        // a_j, o_j, the paths, R_0
  double m[DDP_MAXJ];                      // body mass m_j
  double mp[DDP_MAXJ][3];                  // m_j p_j, p_j the world position of the body's CoM
  double IO[DDP_MAXJ][6];                  // I_j - m_j [p_j]x [p_j]x: the rotational inertia about the world origin (packed, sym3_mv)
  double sv[DDP_MAXJ][6];                  // S_j v_j: joint j's own rate as a twist (angular part, velocity at the world origin)
  double V[DDP_MAXJ][6];                   // body j's twist V_j = sum_{i on j's path} S_i v_i = (omega_j, vO_j)
  double hb[DDP_MAXJ][6];                  // body j's momentum (m_j pdot_j, kO_j)
  double A[1][2][DDP_MAXJ][6];             // A[0][0][c] = dh/d(delta q_c), A[0][1][c] = dh/dv_c
  unsigned long long cm[1][4];             // the tangent columns that carry something: cm[0][2 half + group] (VelWaveLds::cm)
  int idx[DDP_MAXJ];                       // every tangent column, ascending
  double h[6];                             // (l, k)
};

// The jacobians by a wave, step 1 of 3: lane j < nj walks its joint's path once, m_j c_j (and with `ang` the frame's three axes)
// riding along (stage_joint_lane), and leaves its body's record about the world origin and its own rate's twist in S.  (A
// workgroup barrier follows.)
__device__ __forceinline__ void mom_stage_lane(const DevModel& m, const double* q, const double* v, int j, bool ang, MomWaveLds& S) {
  const bool ff = m.ff != 0;
  double x[4][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const double mass = body_mass_com(m, j, x[0]);
  if (ang) stage_joint_lane<4>(m, q, j, S.jw, x);
  else stage_joint_lane<1>(m, q, j, S.jw, x);
  const double* o = S.jw.o[j];
  const double* a = S.jw.a[j];
  const double* d = x[0];
  S.m[j] = mass;
#pragma unroll
  for (int k = 0; k < 3; ++k) S.mp[j][k] = mass * o[k] + d[k];
  if (ang) {
    // E Io E^T + m (|o|^2 1 - o o^T) + 2 (o . d) 1 - d o^T - o d^T
    const double diag = mass * dot3(o, o) + 2.0 * dot3(o, d);
    int p = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      double e[3] = {0.0, 0.0, 0.0}, col[3];
      e[r] = 1.0;
      body_inertia_apply(m, j, x + 1, e, col);
#pragma unroll
      for (int c = 0; c <= r; ++c) S.IO[j][p++] = col[c] + (r == c ? diag : 0.0) - mass * o[r] * o[c] - d[r] * o[c] - o[r] * d[c];
    }
  }
  double* sv = S.sv[j];
  if (j == 0 && ff) {
    double lw[3], t[3];
    mv3(S.jw.R0, v + 3, sv);
    mv3(S.jw.R0, v, lw);
    cross3(o, sv, t);
    sv[3] = lw[0] + t[0]; sv[4] = lw[1] + t[1]; sv[5] = lw[2] + t[2];
    return;
  }
  const double vj = v[ff ? j + 5 : j];
  if (m.jtype[j] == DDP_HIP_JOINT_REVOLUTE) {
    double t[3];
    cross3(o, a, t);
#pragma unroll
    for (int k = 0; k < 3; ++k) { sv[k] = vj * a[k]; sv[3 + k] = vj * t[k]; }
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) { sv[k] = 0.0; sv[3 + k] = vj * a[k]; }
  }
}

// ... step 2 of 3: lane j < nj adds S_i v_i over its path in ascending order (a fixed order, no atomics): its body's twist, and
// from it the body's momentum m_j pdot_j = m_j vO_j + omega_j x m_j p_j and, with `ang`, kO_j = m_j p_j x vO_j + IO_j omega_j.  (A
// workgroup barrier follows.)
__device__ __forceinline__ void mom_prefix_lane(int j, bool ang, MomWaveLds& S) {
  double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[3];
  for (unsigned long long rest = S.jw.mask[j]; rest; rest &= rest - 1) {
    const int i = __builtin_ctzll(rest);
#pragma unroll
    for (int k = 0; k < 6; ++k) V[k] += S.sv[i][k];
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) S.V[j][k] = V[k];
  const double mass = S.m[j];
  const double mp[3] = {S.mp[j][0], S.mp[j][1], S.mp[j][2]};
  cross3(V, mp, t);
#pragma unroll
  for (int k = 0; k < 3; ++k) S.hb[j][k] = mass * V[3 + k] + t[k];
  if (ang) {
    double u[3];
    cross3(mp, V + 3, t);
    sym3_mv(S.IO[j], V, u);
#pragma unroll
    for (int k = 0; k < 3; ++k) S.hb[j][3 + k] = t[k] + u[k];
  }
}

// the momentum (lo, ko) of a body or subtree of mass ms, first moment mps and rotational inertia Is about the world origin that
// moves with the twist (al, be): lo = ms be + al x mps, and with `ang` ko = mps x be + Is al
__device__ __forceinline__ void mom_apply(double ms, const double* mps, const double* Is, const double* al, const double* be, bool ang, double* lo,
                                          double* ko) {
  double t[3];
  cross3(al, mps, t);
  lo[0] = ms * be[0] + t[0]; lo[1] = ms * be[1] + t[1]; lo[2] = ms * be[2] + t[2];
  if (!ang) return;
  double u[3];
  cross3(mps, be, t);
  sym3_mv(Is, al, u);
  ko[0] = t[0] + u[0]; ko[1] = t[1] + u[1]; ko[2] = t[2] + u[2];
}

// ... step 3 of 3: lane j < nj forms mass, first moment, inertia and momentum of its subtree by running over the records in
// ascending order and testing bit j of each record's path (a fixed order, no atomics), the totals alike, and from them its
// column(s) of dh/dv and dh/d(delta q) (ddp_hip.h), with S_j = (al, be) joint j's axis as a twist:
//   (lv, kv) = I_sub(S_j),  (l2, k2) = I_sub(S_j x V_j),  lq = al x l_sub - l2,  kq = al x kO_sub + be x l_sub - k2
//   dh/dv_j = (lv, kv - c x lv),   dh/dq_j = (lq, kq - (lv / M) x l - c x lq)
// With `ang` off the angular rows are not formed (their columns are not in S.cm).  A free-flyer root's linear columns have no
// dh/dq, and no angular part of dh/dv: they are not formed either.  Lane 0 leaves h and the masks.  (A workgroup barrier follows.)
__device__ __forceinline__ void mom_column_lane(const DevModel& m, int j, bool ang, MomWaveLds& S) {
  const int nj = m.nj;
  const bool ff = m.ff != 0;
  const JointWorldLds& W = S.jw;
  double M = 0.0, mpt[3] = {0.0, 0.0, 0.0}, ht[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double ms = 0.0, mps[3] = {0.0, 0.0, 0.0}, Is[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, hs[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < nj; ++i) {
    const bool sub = (W.mask[i] >> j) & 1;
    const double mi = S.m[i];
    M += mi;
    if (sub) ms += mi;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double x = S.mp[i][k], y = S.hb[i][k];
      mpt[k] += x; ht[k] += y;
      if (sub) { mps[k] += x; hs[k] += y; }
    }
    if (ang) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double y = S.hb[i][3 + k];
        ht[3 + k] += y;
        if (sub) hs[3 + k] += y;
      }
      if (sub) {
#pragma unroll
        for (int k = 0; k < 6; ++k) Is[k] += S.IO[i][k];
      }
    }
  }
  const double c[3] = {mpt[0] / M, mpt[1] / M, mpt[2] / M};
  double t[3], k3[3] = {0.0, 0.0, 0.0};
  if (ang) {
    cross3(c, ht, t);
    k3[0] = ht[3] - t[0]; k3[1] = ht[4] - t[1]; k3[2] = ht[5] - t[2];
  }
  if (j == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { S.h[k] = ht[k]; S.h[3 + k] = k3[k]; }
    const unsigned long long all = m.nv >= 64 ? ~0ull : (1ull << m.nv) - 1, moved = ff ? all & ~7ull : all;
    S.cm[0][0] = moved;
    S.cm[0][1] = ang ? moved : 0ull;
    S.cm[0][2] = all;
    S.cm[0][3] = ang ? moved : 0ull;
  }
  double lv[3], kv[3] = {0.0, 0.0, 0.0};
  if (j == 0 && ff) {
    // the free-flyer root (body twists, linear part first): its subtree is the whole robot
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      const double e[3] = {W.R0[cc], W.R0[3 + cc], W.R0[6 + cc]};
      double* Al = S.A[0][1][cc];
      double* Av = S.A[0][1][3 + cc];
      double* Aq = S.A[0][0][3 + cc];
      double be[3];
      Al[0] = M * e[0]; Al[1] = M * e[1]; Al[2] = M * e[2];
      cross3(W.o[0], e, be);
      mom_apply(ms, mps, Is, e, be, ang, lv, kv);
      Av[0] = lv[0]; Av[1] = lv[1]; Av[2] = lv[2];
      cross3(e, ht, t); Aq[0] = t[0]; Aq[1] = t[1]; Aq[2] = t[2];
      if (ang) {
        cross3(c, lv, t); Av[3] = kv[0] - t[0]; Av[4] = kv[1] - t[1]; Av[5] = kv[2] - t[2];
        cross3(e, k3, t); Aq[3] = t[0]; Aq[4] = t[1]; Aq[5] = t[2];
      }
    }
    return;
  }
  const int vi = ff ? j + 5 : j;
  const bool rev = m.jtype[j] == DDP_HIP_JOINT_REVOLUTE;
  double al[3] = {0.0, 0.0, 0.0}, be[3] = {W.a[j][0], W.a[j][1], W.a[j][2]};
  if (rev) {
    al[0] = be[0]; al[1] = be[1]; al[2] = be[2];
    cross3(W.o[j], al, be);
  }
  double* Aq = S.A[0][0][vi];
  double* Av = S.A[0][1][vi];
  mom_apply(ms, mps, Is, al, be, ang, lv, kv);
  // S_j x V_j = (al x omega_j, al x vO_j + be x omega_j)
  const double* V = S.V[j];
  double xa[3], xb[3], l2[3], k2[3] = {0.0, 0.0, 0.0}, lq[3], u[3];
  cross3(al, V, xa);
  cross3(al, V + 3, xb);
  cross3(be, V, t);
  xb[0] += t[0]; xb[1] += t[1]; xb[2] += t[2];
  mom_apply(ms, mps, Is, xa, xb, ang, l2, k2);
  cross3(al, hs, t);
#pragma unroll
  for (int k = 0; k < 3; ++k) { lq[k] = t[k] - l2[k]; Av[k] = lv[k]; Aq[k] = lq[k]; }
  if (!ang) return;
  cross3(c, lv, t);
  Av[3] = kv[0] - t[0]; Av[4] = kv[1] - t[1]; Av[5] = kv[2] - t[2];
  double kq[3];
  cross3(al, hs + 3, t);
  cross3(be, hs, u);
#pragma unroll
  for (int k = 0; k < 3; ++k) kq[k] = t[k] + u[k] - k2[k];
  const double jc[3] = {lv[0] / M, lv[1] / M, lv[2] / M};
  cross3(jc, ht, t);
  cross3(c, lq, u);
  Aq[3] = kq[0] - t[0] - u[0]; Aq[4] = kq[1] - t[1] - u[1]; Aq[5] = kq[2] - t[2] - u[2];
}

// The three steps by one wave (lane tid), barriers included: S.h, S.A, S.cm and S.idx are ready when it returns
__device__ __forceinline__ void mom_jacobians_wave(const DevModel& m, const double* q, const double* v, int tid, bool ang, MomWaveLds& S) {
  if (tid < m.nj) mom_stage_lane(m, q, v, tid, ang, S);
  if (tid < m.nv) S.idx[tid] = tid;
  __syncthreads();
  if (tid < m.nj) mom_prefix_lane(tid, ang, S);
  __syncthreads();
  if (tid < m.nj) mom_column_lane(m, tid, ang, S);
  __syncthreads();
}

}  // namespace rbd
