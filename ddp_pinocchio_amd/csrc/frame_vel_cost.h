// frame_vel_cost.h -- per-instance frame-velocity costs (DDP_HIP_FLAG_FRAME_VEL_COST, ddp_hip.h), of the cost frames of
// DDP_HIP_FLAG_FRAME_COST: the kernel-side description and the traversals they need.  The terms themselves are formed by kernels
// of their own in fwd.hip (cost values: frame_vel_cost_kernel, summed by com_sum_kernel) and lin.hip (derivatives:
// lin_frame_vel_cost_kernel); model_api.hip evaluates one state with the same code.
#pragma once
#include "frame_walk.h"
#include "internal.h"
#include "lie.h"
#include "rbd.h"

// What a kernel reads of the context's frame-velocity cost.  target == nullptr: no terms (the flag is off, no frames are set, or
// no non-zero weight has been uploaded: the block's CostBlock::live)
struct FrameVelCostDev {
  const double *target, *weight;   // [batch][T+1][nf][6]: linear part, then angular part, world axes
  int32_t nf, pad_;
  int32_t joint[DDP_HIP_MAX_COST_FRAMES];
  double off[DDP_HIP_MAX_COST_FRAMES][3];
};

inline FrameVelCostDev frame_vel_cost_dev(const ddp_hip_ctx* ctx) {
  FrameVelCostDev f{};
  const CostBlock& k = ctx->cost[COST_FRAME_VEL];
  if (!k.live) return f;
  f.target = k.side[0];
  f.weight = k.side[1];
  f.nf = ctx->fc_nf;
  for (int k = 0; k < ctx->fc_nf; ++k) {
    f.joint[k] = ctx->fc_joint[k];
    for (int a = 0; a < 3; ++a) f.off[k][a] = ctx->fc_off[k][a];
  }
  return f;
}

namespace rbd {

// The velocity of the point `off` of joint `joint` in world-aligned axes by ONE lane and one walk joint -> root, like frame_point:
// the point p, its linear velocity l and the frame's angular velocity w are carried in the current joint's axes, every joint
// adds its own rate (revolute: w += v_j a, l += v_j a x p; prismatic: l += v_j a; free-flyer root, body twist with the linear part
// first: l += v_lin + v_ang x p, w += v_ang) and rotates the three into its parent's axes.  No per-joint arrays.  lin / ang: form
// the linear / the angular quantities (pd / om are left alone otherwise).  Its own loop, not walk_to_root: the rates enter
// between a joint's rotation and the step to its parent; the step's pieces are the walk's (frame_walk.h)
__device__ __forceinline__ void frame_velocity(const DevModel& m, int joint, const double* off, const double* q, const double* v, bool lin,
                                               bool ang, double* pd, double* om) {
  const bool ff = m.ff != 0;
  double p[3] = {off[0], off[1], off[2]}, l[3] = {0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0}, t[3];
  for (int j = joint; j >= 0; j = m.parent[j]) {
    if (j == 0 && ff) {
      double R[9];
      lie::quat_to_R(q + 3, R);
      if (lin) {
        cross3(v + 3, p, t);
        l[0] += v[0] + t[0]; l[1] += v[1] + t[1]; l[2] += v[2] + t[2];
        dir_to_world(R, l);
      }
      if (ang) {
        w[0] += v[3]; w[1] += v[4]; w[2] += v[5];
        dir_to_world(R, w);
      }
      break;
    }
    const double* a = m.axis[j];
    const double qj = q[ff ? j + 6 : j], vj = v[ff ? j + 5 : j];
    if (m.jtype[j] == DDP_HIP_JOINT_REVOLUTE) {
      double s, c;
      sincos(qj, &s, &c);
      const double omc = 1.0 - c;
      axis_rotate(a, s, omc, p);
      if (lin) {
        axis_rotate(a, s, omc, l);
        cross3(a, p, t);
        l[0] += vj * t[0]; l[1] += vj * t[1]; l[2] += vj * t[2];
      }
      if (ang) {
        axis_rotate(a, s, omc, w);
        w[0] += vj * a[0]; w[1] += vj * a[1]; w[2] += vj * a[2];
      }
    } else {
      p[0] += a[0] * qj; p[1] += a[1] * qj; p[2] += a[2] * qj;
      if (lin) { l[0] += vj * a[0]; l[1] += vj * a[1]; l[2] += vj * a[2]; }
    }
    point_to_parent(m, j, p);
    if (lin) dir_to_parent(m, j, l);
    if (ang) dir_to_parent(m, j, w);
  }
  if (lin) { pd[0] = l[0]; pd[1] = l[1]; pd[2] = l[2]; }
  if (ang) { om[0] = w[0]; om[1] = w[1]; om[2] = w[2]; }
}

// 1/2 sum_a w_a r_a^2 of one frame, r = (pd - g_lin, om - g_ang); a term of weight 0 is left out
__device__ __forceinline__ double frame_vel_term(const double* w, const double* g, const double* pd, const double* om) {
  double s = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if (w[a] != 0.0) { const double r = pd[a] - g[a]; s += w[a] * r * r; }
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if (w[3 + a] != 0.0) { const double r = om[a] - g[3 + a]; s += w[3 + a] * r * r; }
  return 0.5 * s;
}

// What the lanes of one wave leave each other for one state: lane j's joint in slot j, then the frames' jacobians
struct VelWaveLds {
  JointWorldLds jw;                        // a_j, o_j, the paths, R_0
  double wv[DDP_MAXJ][3];                  // W_j v_j: v_j a_j (revolute), 0 (prismatic), R_0 v_ang (free-flyer root)
  double lv[DDP_MAXJ][3];                  // the part of P_j v_j that no lever arm enters: v_j a_j (prismatic), R_0 v_lin (root)
  double om[DDP_MAXJ][3];                  // omega_<=j = sum_{i <= j on j's path} W_i v_i
  double p[DDP_HIP_MAX_COST_FRAMES][3];    // p_f
  double vel[DDP_HIP_MAX_COST_FRAMES][6];  // (pdot_f, omega_f)
  // A_f = [ dr/d(delta q) | dr/dv ] by tangent column: A[f][0][c] = (D_c, E_c), A[f][1][c] = (P_c, W_c)
  double A[DDP_HIP_MAX_COST_FRAMES][2][DDP_MAXJ][6];
  // the tangent columns that carry something: cm[f][2 half + group], half 0 = delta q, 1 = v; group 0 = linear, 1 = angular
  unsigned long long cm[DDP_HIP_MAX_COST_FRAMES][4];
  int idx[DDP_MAXJ];                       // the tangent columns of the live frames' paths, ascending
};

// The jacobians by a wave, step 1 of 4: lane j < nj walks its joint's path once and leaves a_j, o_j, its path (stage_joint_lane)
// and what its own rate contributes (W_j v_j, and the lever-free part of P_j v_j) in S.  (A workgroup barrier follows.)
__device__ __forceinline__ void vel_stage_lane(const DevModel& m, const double* q, const double* v, int j, VelWaveLds& S) {
  const bool ff = m.ff != 0;
  stage_joint_lane<0>(m, q, j, S.jw, nullptr);
  if (j == 0 && ff) {
    mv3(S.jw.R0, v, S.lv[0]);
    mv3(S.jw.R0, v + 3, S.wv[0]);
    return;
  }
  const double vj = v[ff ? j + 5 : j];
  const bool rev = m.jtype[j] == DDP_HIP_JOINT_REVOLUTE;
#pragma unroll
  for (int k = 0; k < 3; ++k) { S.wv[j][k] = rev ? vj * S.jw.a[j][k] : 0.0; S.lv[j][k] = rev ? 0.0 : vj * S.jw.a[j][k]; }
}

// ... step 2 of 4: lane j < nj adds W_i v_i over its path in ascending order (a fixed order, no atomics): omega_<=j.  (A
// workgroup barrier follows.)
__device__ __forceinline__ void vel_prefix_lane(int j, VelWaveLds& S) {
  double s[3] = {0.0, 0.0, 0.0};
  for (unsigned long long rest = S.jw.mask[j]; rest; rest &= rest - 1) {
    const int i = __builtin_ctzll(rest);
    s[0] += S.wv[i][0]; s[1] += S.wv[i][1]; s[2] += S.wv[i][2];
  }
  S.om[j][0] = s[0]; S.om[j][1] = s[1]; S.om[j][2] = s[2];
}

// ... step 3 of 4, once per live frame f (the point p_f in S.p[f], joint jf): lane j on the frame's path adds P_i v_i over the
// path in ascending order, up to j (pdot_<=j) and over all of it (pdot_f; every lane of the path forms the same sum in the same
// order, so none waits for another), and forms its column(s) of P, W, D and E (ddp_hip.h).  lin / ang: the frame has a non-zero
// linear / angular weight; the other group's entries are not formed (their columns are not in S.cm).  Lane jf leaves the
// velocity and the masks of the columns that carry something.  (A workgroup barrier follows the last frame.)
__device__ __forceinline__ void vel_frame_lane(const DevModel& m, int j, int f, int jf, bool lin, bool ang, VelWaveLds& S) {
  const bool ff = m.ff != 0;
  const JointWorldLds& W = S.jw;
  const unsigned long long Mf = W.mask[jf];
  if (!((Mf >> j) & 1)) return;
  const double pf[3] = {S.p[f][0], S.p[f][1], S.p[f][2]};
  const double wf[3] = {S.om[jf][0], S.om[jf][1], S.om[jf][2]};
  const double wj[3] = {S.om[j][0], S.om[j][1], S.om[j][2]};
  double pd[3] = {0.0, 0.0, 0.0}, pj[3] = {0.0, 0.0, 0.0};
  if (lin)
    for (unsigned long long rest = Mf; rest; rest &= rest - 1) {
      const int i = __builtin_ctzll(rest);
      const double lever[3] = {pf[0] - W.o[i][0], pf[1] - W.o[i][1], pf[2] - W.o[i][2]};
      double c[3];
      cross3(S.wv[i], lever, c);
      const double term[3] = {S.lv[i][0] + c[0], S.lv[i][1] + c[1], S.lv[i][2] + c[2]};
      pd[0] += term[0]; pd[1] += term[1]; pd[2] += term[2];
      if (i <= j) { pj[0] += term[0]; pj[1] += term[1]; pj[2] += term[2]; }
    }
  if (j == jf) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { S.vel[f][k] = pd[k]; S.vel[f][3 + k] = wf[k]; }
    // the columns that carry something: P all of the path; W and E the revolute joints and the root's angular columns; D those
    // and the prismatic joints (the root's linear columns have neither D nor E)
    const unsigned long long all = tangent_mask(ff, Mf);
    unsigned long long rot = 0;
    for (unsigned long long rest = Mf; rest; rest &= rest - 1) {
      const int i = __builtin_ctzll(rest);
      if (i == 0 && ff) { rot |= 56ull; continue; }
      if (m.jtype[i] == DDP_HIP_JOINT_REVOLUTE) rot |= 1ull << (ff ? i + 5 : i);
    }
    S.cm[f][0] = lin ? (ff ? all & ~7ull : all) : 0ull;
    S.cm[f][1] = ang ? rot : 0ull;
    S.cm[f][2] = lin ? all : 0ull;
    S.cm[f][3] = ang ? rot : 0ull;
  }
  double t[3];
  if (j == 0 && ff) {
#pragma unroll
    for (int cc = 0; cc < 3; ++cc) {
      const double e[3] = {W.R0[cc], W.R0[3 + cc], W.R0[6 + cc]};
      double* Aq = S.A[f][0][3 + cc];
      double* Av = S.A[f][1][3 + cc];
      if (lin) {
        point_column(m, ff, W, cc, pf, S.A[f][1][cc]);
        point_column(m, ff, W, 3 + cc, pf, Av);
        cross3(e, pd, t); Aq[0] = t[0]; Aq[1] = t[1]; Aq[2] = t[2];
      }
      if (ang) {
        Av[3] = e[0]; Av[4] = e[1]; Av[5] = e[2];
        cross3(e, wf, t); Aq[3] = t[0]; Aq[4] = t[1]; Aq[5] = t[2];
      }
    }
    return;
  }
  const int vi = ff ? j + 5 : j;
  const double a[3] = {W.a[j][0], W.a[j][1], W.a[j][2]};
  double* Aq = S.A[f][0][vi];
  double* Av = S.A[f][1][vi];
  double P[3];
  if (lin) {
    point_column(m, ff, W, vi, pf, P);
    Av[0] = P[0]; Av[1] = P[1]; Av[2] = P[2];
  }
  if (m.jtype[j] == DDP_HIP_JOINT_REVOLUTE) {
    if (lin) {
      double d1[3], d2[3];
      cross3(wj, P, d1);
      const double rest[3] = {pd[0] - pj[0], pd[1] - pj[1], pd[2] - pj[2]};
      cross3(a, rest, d2);
      Aq[0] = d1[0] + d2[0]; Aq[1] = d1[1] + d2[1]; Aq[2] = d1[2] + d2[2];
    }
    if (ang) {
      Av[3] = a[0]; Av[4] = a[1]; Av[5] = a[2];
      const double dw[3] = {wf[0] - wj[0], wf[1] - wj[1], wf[2] - wj[2]};
      cross3(a, dw, t); Aq[3] = t[0]; Aq[4] = t[1]; Aq[5] = t[2];
    }
  } else if (lin) {
    cross3(wj, a, t); Aq[0] = t[0]; Aq[1] = t[1]; Aq[2] = t[2];
  }
}

// ... step 4 of 4: the wave (lane tid of nt) adds, over the rows and columns of the live frames' paths alone (nu tangent columns
// in S.idx: their delta-q rows, then their v rows),
//   gx[row] += sum_f sum_a A_f[a][row] (w_a r_a),   gxx[i][j] += sum_f sum_a A_f[a][min] w_a A_f[a][max]     (Gauss-Newton)
// the frames and axes in their fixed order and entry (i, j) in (min, max) order: the block stays symmetric bit for bit.  w / wr:
// weights and weighted residuals [nf][6] (0 where the weight is 0).  A term of weight 0, or of a column that carries nothing of
// the axis' group, is left out; an entry that no term reaches is not written.  Rec: VelWaveLds, or another record with its A, cm
// and idx (momentum_cost.h: one "frame" over every column)
template <class Rec>
__device__ __forceinline__ void vel_add_wave(const Rec& S, int nf, const double* w, const double* wr, int nu, int tid, int nt, int nv,
                                             int n, double* gx, double* gxx) {
  for (int k = tid; k < 2 * nu; k += nt) {
    const int h = k >= nu ? 1 : 0, c = S.idx[h ? k - nu : k];
    double s = 0.0;
    bool any = false;
    for (int f = 0; f < nf; ++f)
      for (int a = 0; a < 6; ++a) {
        if (w[6 * f + a] == 0.0 || !((S.cm[f][2 * h + a / 3] >> c) & 1)) continue;
        s += S.A[f][h][c][a] * wr[6 * f + a];
        any = true;
      }
    if (any) gx[h * nv + c] += s;
  }
  for (int e = tid; e < 4 * nu * nu; e += nt) {
    const int ki = e % (2 * nu), kj = e / (2 * nu);
    const int hi_ = ki >= nu ? 1 : 0, ci = S.idx[hi_ ? ki - nu : ki];
    const int hj_ = kj >= nu ? 1 : 0, cj = S.idx[hj_ ? kj - nu : kj];
    const int i = hi_ * nv + ci, j = hj_ * nv + cj;
    const bool swap = j < i;
    const int hl = swap ? hj_ : hi_, cl = swap ? cj : ci, hh = swap ? hi_ : hj_, ch = swap ? ci : cj;
    double s = 0.0;
    bool any = false;
    for (int f = 0; f < nf; ++f)
      for (int a = 0; a < 6; ++a) {
        const double wa = w[6 * f + a];
        if (wa == 0.0 || !((S.cm[f][2 * hl + a / 3] >> cl) & 1) || !((S.cm[f][2 * hh + a / 3] >> ch) & 1)) continue;
        s += S.A[f][hl][cl][a] * wa * S.A[f][hh][ch][a];
        any = true;
      }
    if (any) gxx[i + (int64_t)j * n] += s;
  }
}

}  // namespace rbd
