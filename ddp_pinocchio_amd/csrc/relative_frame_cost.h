// relative_frame_cost.h -- per-instance relative-placement costs between two robot frames (DDP_HIP_FLAG_RELATIVE_FRAME_COST,
// ddp_hip.h): the kernel-side description, the walk of a pair and the wave's record and add for the derivatives.  The terms
// themselves are formed by kernels of their own in fwd.hip (cost values: relative_frame_cost_kernel, summed by com_sum_kernel;
// residuals: relative_frame_error_kernel) and lin.hip (derivatives: lin_relative_frame_cost_kernel); model_api.hip evaluates one
// configuration with the same code.  The walk, the staged joint record, point_column and the column compaction are frame_walk.h's.
#pragma once
#include "frame_walk.h"
#include "internal.h"
#include "lie.h"
#include "rbd.h"

// What a kernel reads of the context's relative-frame cost.  weight == nullptr: no terms (the flag is off, no pairs are set, or
// no non-zero weight has been uploaded: the block's CostBlock::live)
struct RelativeFrameDev {
  const double *target, *quat, *weight;   // [batch][T+1][np][3], [..][4] (unit quaternions x y z w), [..][6]
  int32_t np, pad_;                       // pairs
  int32_t ja[DDP_HIP_MAX_FRAME_PAIRS], jb[DDP_HIP_MAX_FRAME_PAIRS];   // pair i: base frame on joint ja[i], tip frame on jb[i]
  double offa[DDP_HIP_MAX_FRAME_PAIRS][3], offb[DDP_HIP_MAX_FRAME_PAIRS][3];
};

// always: the description whether or not a weight is live (ddp_hip_relative_frame_error works from the first set_pairs on)
inline RelativeFrameDev relative_frame_dev(const ddp_hip_ctx* ctx, bool always = false) {
  RelativeFrameDev c{};
  const CostBlock& k = ctx->cost[COST_RELATIVE_FRAME];
  if (!(always ? ctx->rf_np > 0 : k.live)) return c;
  c.target = k.side[0];
  c.quat = k.side[1];
  c.weight = k.side[2];
  c.np = ctx->rf_np;
  for (int i = 0; i < ctx->rf_np; ++i) {
    c.ja[i] = ctx->rf_ja[i];
    c.jb[i] = ctx->rf_jb[i];
    for (int a = 0; a < 3; ++a) { c.offa[i][a] = ctx->rf_offa[i][a]; c.offb[i][a] = ctx->rf_offb[i][a]; }
  }
  return c;
}

namespace rbd {

// A pair at one configuration: what the two walks leave
struct RelativePlacement {
  double rel[3];      // R_a^T (p_b - p_a): B's point as seen from A, in A's joint axes
  double E[9];        // R_a^T R_b, row-major (with_rot only)
  double ca[3][3];    // ca[k] = R_a e_k: the columns of R_a (so row k of R_a^T)
  double cb[3][3];    // cb[k] = R_b e_k
  double pb[3];       // p_b
};

// The pair (joint ja, point offa) -> (joint jb, point offb) at q: two walks joint -> root, each with the frame's point and the
// three directions of its joint's axes.  with_rot == false: E is not formed.  M: DevModel or CoopModel
template <class M>
__device__ __forceinline__ void relative_placement(const M& m, bool ff, int ja, const double* offa, int jb, const double* offb, const double* q,
                                                   bool with_rot, RelativePlacement& P) {
  double pa[1][3] = {{offa[0], offa[1], offa[2]}}, pb[1][3] = {{offb[0], offb[1], offb[2]}};
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) P.ca[k][a] = P.cb[k][a] = k == a ? 1.0 : 0.0;
  (void)walk_to_root<1, 3>(m, ff, ja, q, pa, P.ca, -1);
  (void)walk_to_root<1, 3>(m, ff, jb, q, pb, P.cb, -1);
  const double d[3] = {pb[0][0] - pa[0][0], pb[0][1] - pa[0][1], pb[0][2] - pa[0][2]};
#pragma unroll
  for (int k = 0; k < 3; ++k) { P.rel[k] = dot3(P.ca[k], d); P.pb[k] = pb[0][k]; }
  if (with_rot)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) P.E[3 * i + j] = dot3(P.ca[i], P.cb[j]);
}

// The residual r = (r_pos, e_rot) of a placement.  g == nullptr: no target is read, r_pos is not formed; ref == nullptr: no
// quaternion is read and no log is formed (P.E is not read either)
__device__ __forceinline__ void relative_frame_residual(const RelativePlacement& P, const double* g, const double* ref, double* r) {
  if (g) { r[0] = P.rel[0] - g[0]; r[1] = P.rel[1] - g[1]; r[2] = P.rel[2] - g[2]; }
  if (ref) lie::so3_log_rel(ref, P.E, r + 3);
}

// 1/2 sum_a w_a r_a^2 of pair i of block bt1 at the state x, the position axes, then the rotation axes; a term of weight 0 is left
// out, and with three of them their half of the residual.  (The caller has seen a non-zero among the six.)
template <class M>
__device__ __forceinline__ double relative_frame_term(const M& m, const RelativeFrameDev& rf, int i, int64_t bt1, const double* x) {
  const double* w = rf.weight + (bt1 * rf.np + i) * 6;
  const bool pos = frame_weights_any(w), rot = frame_weights_any(w + 3);
  RelativePlacement P;
  relative_placement(m, m.ff != 0, rf.ja[i], rf.offa[i], rf.jb[i], rf.offb[i], x, rot, P);
  double r[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  relative_frame_residual(P, pos ? rf.target + (bt1 * rf.np + i) * 3 : nullptr, rot ? rf.quat + (bt1 * rf.np + i) * 4 : nullptr, r);
  double s = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
    if (w[a] != 0.0) s += w[a] * r[a] * r[a];
  return 0.5 * s;
}

// What the lanes of one wave leave each other for the derivatives at one configuration (lin_relative_frame_cost_kernel): lanes
// j < nj their joint (rbd::stage_joint_lane), the live pairs' lanes their pair; then the live pairs' columns
struct RelativeWaveLds {
  JointWorldLds jw;                                      // a_j, o_j, the paths, R_0
  double RaT[DDP_HIP_MAX_FRAME_PAIRS][9];                // of the live pairs: R_a^T (row-major),
  double JR[DDP_HIP_MAX_FRAME_PAIRS][9];                 // Jlog3(e_rot) R_b^T (rotation weights live),
  double pb[DDP_HIP_MAX_FRAME_PAIRS][3];                 // p_b,
  double w[DDP_HIP_MAX_FRAME_PAIRS][6];                  // w,
  double wr[DDP_HIP_MAX_FRAME_PAIRS][6];                 // w o r (0 where the weight is 0)
  unsigned long long ca[DDP_HIP_MAX_FRAME_PAIRS];        // the tangent columns on path(ja_i) alone
  unsigned long long cb[DDP_HIP_MAX_FRAME_PAIRS];        // ... and on path(jb_i) alone (0 | 0: the pair is not live)
  int idx[DDP_MAXJ];                                     // the union of them all, ascending: nu compacted columns
  double A[DDP_HIP_MAX_FRAME_PAIRS][DDP_MAXJ][6];        // J_i[:, idx[k]] at A[i][k]: rows 0 .. 2 J_pos, 3 .. 5 J_rot (revolute columns)
};

// Column c (a tangent index of pair i's symmetric difference: never a free-flyer root's) of J_i = [J_pos; J_rot] from the staged
// record: s_c R_a^T point_column(c, p_b), and for a revolute column s_c S.JR[i] a_c (Jlog3(e) R_b^T; with R_b^T alone there: the
// jacobian at e_rot = 0).  pos / rot: which half is formed; the other half of `col` is left as it is
__device__ __forceinline__ void relative_frame_column(const DevModel& m, bool ff, const RelativeWaveLds& S, int i, int c, bool pos, bool rot,
                                                      double* col) {
  const bool on_b = (S.cb[i] >> c) & 1;
  const int j = ff ? c - 5 : c;
  if (pos) {
    double P[3];
    point_column(m, ff, S.jw, c, S.pb[i], P);
    mv3(S.RaT[i], P, col);
    if (!on_b) { col[0] = -col[0]; col[1] = -col[1]; col[2] = -col[2]; }
  }
  if (rot && m.jtype[j] == DDP_HIP_JOINT_REVOLUTE) {
    mv3(S.JR[i], S.jw.a[j], col + 3);
    if (!on_b) { col[3] = -col[3]; col[4] = -col[4]; col[5] = -col[5]; }
  }
}

// The wave (lane tid of nt) stages the columns of the live pairs over the nu compacted columns of S.idx, A[i][k] = J_i[:, idx[k]]
// where idx[k] is in pair i's symmetric difference (a pair that is not live has none), the halves its weights ask for.  (A
// workgroup barrier follows.)
__device__ __forceinline__ void relative_frame_stage_columns(const DevModel& m, RelativeWaveLds& S, int np, int nu, int tid, int nt) {
  const bool ff = m.ff != 0;
  for (int e = tid; e < np * nu; e += nt) {
    const int i = e / nu, k = e % nu, c = S.idx[k];
    if (!(((S.ca[i] | S.cb[i]) >> c) & 1)) continue;
    const double* w = S.w[i];
    relative_frame_column(m, ff, S, i, c, w[0] != 0.0 || w[1] != 0.0 || w[2] != 0.0, w[3] != 0.0 || w[4] != 0.0 || w[5] != 0.0, S.A[i][k]);
  }
}

// ... and adds, over the nu compacted columns alone (rot: the tangent columns of revolute joints),
//   gx[c] += sum_i sum_a J_i[a][c] (w_a r_a),      gxx[r][c] += sum_i sum_a J_i[a][min] w_a J_i[a][max]      (Gauss-Newton)
// the pairs in ascending order, the three position axes, then the three rotation axes, entry (r, c) in (min, max) order: the block
// stays symmetric bit for bit.  A term of weight 0, a pair outside whose symmetric difference r or c lies and a rotation axis at a
// prismatic column are left out; an entry that no term reaches is not written.  A column on both paths of a pair is in neither ca
// nor cb: the common ancestors -- a free-flyer root's six columns among them -- are never touched.  The sibling of gn_add_wave /
// vel_add_wave for six rows on compacted delta-q columns: their records hold three rows, or a v half this term does not have
__device__ __forceinline__ void relative_frame_add_wave(const RelativeWaveLds& S, int np, unsigned long long rot, int nu, int tid, int nt, int n,
                                                        double* gx, double* gxx) {
  for (int k = tid; k < nu; k += nt) {
    const int c = S.idx[k];
    double s = 0.0;
    bool any = false;
    for (int i = 0; i < np; ++i) {
      if (!(((S.ca[i] | S.cb[i]) >> c) & 1)) continue;
      for (int a = 0; a < 6; ++a) {
        if (S.w[i][a] == 0.0 || (a >= 3 && !((rot >> c) & 1))) continue;
        s += S.A[i][k][a] * S.wr[i][a];
        any = true;
      }
    }
    if (any) gx[c] += s;
  }
  for (int e = tid; e < nu * nu; e += nt) {
    const int kr = e % nu, kc = e / nu;
    const int r = S.idx[kr], c = S.idx[kc];
    const int lo = kr < kc ? kr : kc, hi = kr < kc ? kc : kr;          // (idx ascends: the order of the tangent indices)
    const bool both_rot = ((rot >> r) & 1) && ((rot >> c) & 1);
    double h = 0.0;
    bool any = false;
    for (int i = 0; i < np; ++i) {
      const unsigned long long sd = S.ca[i] | S.cb[i];
      if (!((sd >> r) & 1) || !((sd >> c) & 1)) continue;
      for (int a = 0; a < 6; ++a) {
        const double wa = S.w[i][a];
        if (wa == 0.0 || (a >= 3 && !both_rot)) continue;
        h += S.A[i][lo][a] * wa * S.A[i][hi][a];
        any = true;
      }
    }
    if (any) gxx[r + (int64_t)c * n] += h;
  }
}

}  // namespace rbd
