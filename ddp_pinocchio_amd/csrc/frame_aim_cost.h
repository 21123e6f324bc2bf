// frame_aim_cost.h -- per-instance frame-aiming costs (DDP_HIP_FLAG_FRAME_AIM_COST, ddp_hip.h): "this axis of that frame points at
// this target, from this far".  The kernel-side description, the walk of a frame, the residual and the wave's record and add for
// the derivatives.  The terms themselves are formed by kernels of their own in fwd.hip (cost values: frame_aim_cost_kernel, summed
// by com_sum_kernel; the readback: frame_aim_error_kernel) and lin.hip (derivatives: lin_frame_aim_cost_kernel); model_api.hip
// evaluates one configuration with the same code.  The walk, the staged joint record, point_column and the column compaction are
// frame_walk.h's.
#pragma once
#include "frame_walk.h"
#include "internal.h"
#include "lie.h"
#include "rbd.h"

#define FRAME_AIM_MIN_RANGE 1e-12   // a line of sight of length l <= this has no direction: the frame forms nothing there

// What a kernel reads of the context's frame-aiming cost.  weight == nullptr: no terms (the flag is off, no frames are set, or no
// non-zero weight has been uploaded: the block's CostBlock::live)
struct FrameAimDev {
  const double *target, *weight;   // [batch][T+1][nf][4] = (g, rho), [batch][T+1][nf][2] = (w_aim, w_range)
  int32_t nf, pad_;                // aim frames
  int32_t joint[DDP_HIP_MAX_AIM_FRAMES];
  double off[DDP_HIP_MAX_AIM_FRAMES][3], axis[DDP_HIP_MAX_AIM_FRAMES][3];   // the eye and the unit axis, in the joint's coordinates
};

// always: the description whether or not a weight is live (ddp_hip_frame_aim_error works from the first set_frames on)
inline FrameAimDev frame_aim_dev(const ddp_hip_ctx* ctx, bool always = false) {
  FrameAimDev c{};
  const CostBlock& k = ctx->cost[COST_FRAME_AIM];
  if (!(always ? ctx->fa_nf > 0 : k.live)) return c;
  c.target = k.side[0];
  c.weight = k.side[1];
  c.nf = ctx->fa_nf;
  for (int i = 0; i < ctx->fa_nf; ++i) {
    c.joint[i] = ctx->fa_joint[i];
    for (int a = 0; a < 3; ++a) { c.off[i][a] = ctx->fa_off[i][a]; c.axis[i][a] = ctx->fa_axis[i][a]; }
  }
  return c;
}

namespace rbd {

// The eye p and the world direction n = R_j a of the frame (joint, off, axis) at q: one walk joint -> root with the point and the
// direction.  M: DevModel or CoopModel
template <class M>
__device__ __forceinline__ void frame_aim_walk(const M& m, bool ff, int joint, const double* off, const double* axis, const double* q, double* p,
                                               double* nw) {
  double pt[1][3] = {{off[0], off[1], off[2]}}, dir[1][3] = {{axis[0], axis[1], axis[2]}};
  (void)walk_to_root<1, 1>(m, ff, joint, q, pt, dir, -1);
#pragma unroll
  for (int k = 0; k < 3; ++k) { p[k] = pt[0][k]; nw[k] = dir[0][k]; }
}

// The line of sight from p to g: d = g - p, l = |d|, dh = d / l.  false: l <= FRAME_AIM_MIN_RANGE, dh is not formed
__device__ __forceinline__ bool frame_aim_sight(const double* p, const double* g, double* dh, double* l) {
  const double d[3] = {g[0] - p[0], g[1] - p[1], g[2] - p[2]};
  *l = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (*l <= FRAME_AIM_MIN_RANGE) return false;                        // (a NaN length goes on: a non-finite state gives a NaN term)
  const double s = 1.0 / *l;
  dh[0] = d[0] * s; dh[1] = d[1] * s; dh[2] = d[2] * s;
  return true;
}

// 1/2 (w_aim |n - dh|^2 + w_range (l - rho)^2) of frame i of block bt1 at the state x: the three aim rows first, then the range
// row; a term of weight 0 is left out (with w_range = 0 rho is not read).  false: nothing is formed (both weights 0: no walk; or
// l <= FRAME_AIM_MIN_RANGE)
template <class M>
__device__ __forceinline__ bool frame_aim_term(const M& m, const FrameAimDev& fa, int i, int64_t bt1, const double* x, double* term) {
  const double* w = fa.weight + (bt1 * fa.nf + i) * 2;
  const double wa = w[0], wr = w[1];
  if (wa == 0.0 && wr == 0.0) return false;
  const double* g = fa.target + (bt1 * fa.nf + i) * 4;
  double p[3], nw[3], dh[3], l;
  frame_aim_walk(m, m.ff != 0, fa.joint[i], fa.off[i], fa.axis[i], x, p, nw);
  if (!frame_aim_sight(p, g, dh, &l)) return false;
  double s = 0.0;
  if (wa != 0.0)
#pragma unroll
    for (int a = 0; a < 3; ++a) { const double r = nw[a] - dh[a]; s += wa * r * r; }
  if (wr != 0.0) { const double r = l - g[3]; s += wr * r * r; }
  *term = 0.5 * s;
  return true;
}

// What the lanes of one wave leave each other for the derivatives at one configuration (lin_frame_aim_cost_kernel): lanes j < nj
// their joint (rbd::stage_joint_lane), the frames' lanes their frame; then the live frames' columns
struct FrameAimWaveLds {
  JointWorldLds jw;                                      // a_j, o_j, the paths, R_0
  double p[DDP_HIP_MAX_AIM_FRAMES][3];                   // of the live frames: the eye,
  double nw[DDP_HIP_MAX_AIM_FRAMES][3];                  // the world direction n,
  double dh[DDP_HIP_MAX_AIM_FRAMES][3];                  // the unit line of sight,
  double il[DDP_HIP_MAX_AIM_FRAMES];                     // 1 / l,
  double w[DDP_HIP_MAX_AIM_FRAMES][4];                   // the rows' weights (w_aim three times, w_range),
  double wr[DDP_HIP_MAX_AIM_FRAMES][4];                  // w o r (0 where the weight is 0)
  int live[DDP_HIP_MAX_AIM_FRAMES];                      // the frame forms something here (a weight, and a line of sight)
  unsigned long long cols[DDP_HIP_MAX_AIM_FRAMES];       // the tangent columns of path(j_i) (0: the frame is not live)
  int idx[DDP_MAXJ];                                     // the union of them all, ascending: nu compacted columns
  double A[DDP_HIP_MAX_AIM_FRAMES][DDP_MAXJ][4];         // J_i[:, idx[k]] at A[i][k]: rows 0 .. 2 J_aim, row 3 J_range
};

// The world rotation axis of tangent column c: a revolute joint's a_c, R_0 e_(c-3) for the angular columns 3 .. 5 of a free-flyer
// root (the convention of the orientation cost).  false: the column carries no rotation (prismatic, the root's linear columns)
__device__ __forceinline__ bool rotation_column(const DevModel& m, bool ff, const JointWorldLds& S, int c, double* ax) {
  if (ff && c < 6) {
    if (c < 3) return false;
    const int k = c - 3;
    ax[0] = S.R0[k]; ax[1] = S.R0[3 + k]; ax[2] = S.R0[6 + k];
    return true;
  }
  const int j = ff ? c - 5 : c;
  if (m.jtype[j] != DDP_HIP_JOINT_REVOLUTE) return false;
  ax[0] = S.a[j][0]; ax[1] = S.a[j][1]; ax[2] = S.a[j][2];
  return true;
}

// The frame's lane leaves its record: walk, line of sight, weights and weighted residuals.  g: (target, rho), w: (w_aim, w_range)
__device__ __forceinline__ void frame_aim_stage_frame(const DevModel& m, bool ff, const FrameAimDev& fa, int i, const double* q, const double* g,
                                                      const double* w, FrameAimWaveLds& S) {
  const double wa = w[0], wr = w[1];
  S.live[i] = 0;
  if (wa == 0.0 && wr == 0.0) return;
  double p[3], nw[3], dh[3], l;
  frame_aim_walk(m, ff, fa.joint[i], fa.off[i], fa.axis[i], q, p, nw);
  if (!frame_aim_sight(p, g, dh, &l)) return;
  S.live[i] = 1;
  S.il[i] = 1.0 / l;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    S.p[i][a] = p[a]; S.nw[i][a] = nw[a]; S.dh[i][a] = dh[a];
    S.w[i][a] = wa;
    S.wr[i][a] = wa != 0.0 ? wa * (nw[a] - dh[a]) : 0.0;
  }
  S.w[i][3] = wr;
  S.wr[i][3] = wr != 0.0 ? wr * (l - g[3]) : 0.0;
}

// Column c (a tangent index on path(j_i)) of J_i = [J_aim; J_range] from the staged record, P = point_column(c, p):
//   J_aim[:, c] = (a_c x n, where c carries rotation) + (P - dh (dh . P)) / l,      J_range[c] = -dh . P
// aim / range: which rows are formed; the others of `col` are left as they are
__device__ __forceinline__ void frame_aim_column(const DevModel& m, bool ff, const FrameAimWaveLds& S, int i, int c, bool aim, bool range,
                                                 double* col) {
  double P[3];
  point_column(m, ff, S.jw, c, S.p[i], P);
  const double dP = dot3(S.dh[i], P);
  if (aim) {
    double ax[3], t[3] = {0.0, 0.0, 0.0};
    if (rotation_column(m, ff, S.jw, c, ax)) cross3(ax, S.nw[i], t);
#pragma unroll
    for (int a = 0; a < 3; ++a) col[a] = t[a] + (P[a] - S.dh[i][a] * dP) * S.il[i];
  }
  if (range) col[3] = -dP;
}

// The wave (lane tid of nt) stages the columns of the live frames over the nu compacted columns of S.idx, A[i][k] = J_i[:, idx[k]]
// where idx[k] is on frame i's path, the rows its weights ask for.  (A workgroup barrier follows.)
__device__ __forceinline__ void frame_aim_stage_columns(const DevModel& m, FrameAimWaveLds& S, int nf, int nu, int tid, int nt) {
  const bool ff = m.ff != 0;
  for (int e = tid; e < nf * nu; e += nt) {
    const int i = e / nu, k = e % nu, c = S.idx[k];
    if (!((S.cols[i] >> c) & 1)) continue;
    frame_aim_column(m, ff, S, i, c, S.w[i][0] != 0.0, S.w[i][3] != 0.0, S.A[i][k]);
  }
}

// ... and adds, over the nu compacted columns alone,
//   gx[c] += sum_i sum_a J_i[a][c] (w_a r_a),      gxx[r][c] += sum_i sum_a J_i[a][min] w_a J_i[a][max]      (Gauss-Newton)
// the frames in ascending order, the three aim rows, then the range row, entry (r, c) in (min, max) order: the block stays symmetric
// bit for bit.  A row of weight 0 and a frame off whose path r or c lies are left out; an entry that no row reaches is not written.
// The sibling of gn_add_wave / relative_frame_add_wave for four rows on compacted delta-q columns
__device__ __forceinline__ void frame_aim_add_wave(const FrameAimWaveLds& S, int nf, int nu, int tid, int nt, int n, double* gx, double* gxx) {
  for (int k = tid; k < nu; k += nt) {
    const int c = S.idx[k];
    double s = 0.0;
    bool any = false;
    for (int i = 0; i < nf; ++i) {
      if (!((S.cols[i] >> c) & 1)) continue;
      for (int a = 0; a < 4; ++a) {
        if (S.w[i][a] == 0.0) continue;
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
    double h = 0.0;
    bool any = false;
    for (int i = 0; i < nf; ++i) {
      if (!((S.cols[i] >> r) & 1) || !((S.cols[i] >> c) & 1)) continue;
      for (int a = 0; a < 4; ++a) {
        const double wa = S.w[i][a];
        if (wa == 0.0) continue;
        h += S.A[i][lo][a] * wa * S.A[i][hi][a];
        any = true;
      }
    }
    if (any) gxx[r + (int64_t)c * n] += h;
  }
}

}  // namespace rbd
