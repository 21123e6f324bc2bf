// lin.hip -- linearisation of cost, dynamics and constraints along the resident trajectory.
//
// Replaces problem_t::compute_derivatives (problem.hpp:956-998; the print-only self check :999-1139
// is not reproduced).  Every (instance, t, perturbation) is an independent forward-dynamics
// evaluation, so the stencils of
//   - the first order:  forward differences, eps = sqrt(DBL_EPSILON), perturbing with integrate_x /
//     integrate_u exactly like problem.hpp:105-126 (the reference takes Pinocchio's analytic ABA
//     derivatives here, problem.hpp:463-503; the closed-form pendulum keeps its analytic partials);
//   - the second order: finite_diff_hessian_compute mode 2 (problem.hpp:152-298, eps = eps_mach^(1/4))
//     or mode 1 (problem.hpp:67-150, for models with analytic first order)
// are laid out one evaluation per lane.
#include <float.h>
#include <math.h>
#include <stdlib.h>

#include "balance_region_cost.h"
#include "capsule_cost.h"
#include "com_cost.h"
#include "control_grav_cost.h"
#include "frame_aim_cost.h"
#include "frame_cost.h"
#include "frame_vel_cost.h"
#include "internal.h"
#include "joint_accel_cost.h"
#include "lin_common.h"
#include "momentum_cost.h"
#include "obstacle_cost.h"
#include "rbd.h"
#include "rbd_deriv.h"
#include "relative_frame_cost.h"
#include "self_collision_cost.h"
#include "state_limits.h"

namespace {



// cost derivatives, problem.hpp:958-959,982-987:  lx = 0, lxx = 0, lux = 0, lu = c u^T, luu = c I
__global__ void lin_cost_kernel(LinParams p) {
  const int64_t T = p.d.T;
  const int64_t bt = blockIdx.x;
  const int b = (int)(bt / T);
  const int64_t t = bt % T;
  const int n = (int)p.d.n, m = (int)p.d.m;
  const double c = p.model->c;
  const int tid = threadIdx.x;
  if (t == 0) {
    for (int i = tid; i < n; i += blockDim.x) p.lfx[(int64_t)b * n + i] = 0.0;
    for (int i = tid; i < n * n; i += blockDim.x) p.lfxx[(int64_t)b * n * n + i] = 0.0;
  }
  for (int i = tid; i < n; i += blockDim.x) p.lx[bt * n + i] = 0.0;
  for (int i = tid; i < n * n; i += blockDim.x) p.lxx[bt * n * n + i] = 0.0;
  for (int i = tid; i < m * n; i += blockDim.x) p.lux[bt * m * n + i] = 0.0;
  for (int i = tid; i < m; i += blockDim.x) p.lu[bt * m + i] = c * p.u[bt * m + i];
  for (int i = tid; i < m * m; i += blockDim.x) p.luu[bt * m * m + i] = (i % m == i / m) ? 1.0 * c : 0.0;
}

// Tracking cost (DDP_HIP_FLAG_TRACKING_COST, ddp_hip.h): one workgroup per (instance, t), t = 0 .. T; t = T writes lfx / lfxx.
// d = x (-) xref, J = dd/ddx: the identity but on a free-flyer root block, where it is Jlog6(d_root) (lie::se3_Jlog).
//   lx = J^T (wx o d), lxx = J^T diag(wx) J (Gauss-Newton on the root block: the term sum_k wx_k d_k d^2(d_k) is left out,
//   exact where d_root = 0), lu = c u + wu o (u - uref), luu = c I + diag(wu), lux = 0.
// Every entry of the dense blocks is stored, as lin_cost_kernel stores them.  A term of weight 0 is left out (fwd.hip:
// track_state_sum): with every weight 0 the bytes are lin_cost_kernel's, whatever the state.
__global__ void lin_track_cost_kernel(LinParams p) {
  const int64_t T = p.d.T;
  const int64_t bt1 = blockIdx.x;
  const int b = (int)(bt1 / (T + 1));
  const int64_t t = bt1 % (T + 1);
  const int n = (int)p.d.n, m = (int)p.d.m, nx = (int)p.d.nx, nv = (int)p.d.nv;
  const DevModel& md = *p.model;
  const int nq = nx - nv, r0 = md.ff ? 6 : 0;   // rows r0 .. n-1 of d are plain differences
  const double c = md.c;
  const int tid = threadIdx.x;
  __shared__ double s_d[2 * DDP_MAXJ], s_w[2 * DDP_MAXJ], s_J[36];
  const double* x = p.x + ((int64_t)b * (T + 1) + t) * nx;
  const double* xr = p.xref + ((int64_t)b * (T + 1) + t) * nx;
  const double* w = p.wx + ((int64_t)b * (T + 1) + t) * n;
  if (md.ff && tid == 0) { lie::se3_difference(xr, x, s_d); lie::se3_Jlog(s_d, s_J); }   // lie::difference_x, root rows
  for (int i = r0 + tid; i < n; i += blockDim.x) {
    const int k = i < nv ? i + (nq - nv) : nq + i - nv;
    s_d[i] = x[k] - xr[k];
  }
  for (int i = tid; i < n; i += blockDim.x) s_w[i] = w[i];
  __syncthreads();
  double* gx = t < T ? p.lx + (b * T + t) * n : p.lfx + (int64_t)b * n;
  double* gxx = t < T ? p.lxx + (b * T + t) * n * n : p.lfxx + (int64_t)b * n * n;
  for (int i = tid; i < n; i += blockDim.x) {
    double g;
    if (i < r0) { g = 0; for (int k = 0; k < 6; ++k) if (s_w[k] != 0.0) g += s_J[6 * k + i] * (s_w[k] * s_d[k]); }
    else g = s_w[i] != 0.0 ? s_w[i] * s_d[i] : 0.0;
    gx[i] = g;
  }
  for (int e = tid; e < n * n; e += blockDim.x) {
    const int i = e % n, j = e / n;
    double h = 0.0;
    if (i < r0 && j < r0) {   // (min, max) order: the block is symmetric bit for bit
      const int a = i < j ? i : j, a2 = i < j ? j : i;
      for (int k = 0; k < 6; ++k) if (s_w[k] != 0.0) h += s_J[6 * k + a] * s_w[k] * s_J[6 * k + a2];
    } else if (i == j) h = s_w[i];
    gxx[e] = h;
  }
  if (t == T) return;
  const int64_t bt = (int64_t)b * T + t;
  for (int i = tid; i < m * n; i += blockDim.x) p.lux[bt * m * n + i] = 0.0;
  for (int i = tid; i < m; i += blockDim.x) {
    const double u = p.u[bt * m + i];
    const double wu = p.wu[bt * m + i];
    p.lu[bt * m + i] = wu != 0.0 ? c * u + wu * (u - p.uref[bt * m + i]) : c * u;
  }
  for (int i = tid; i < m * m; i += blockDim.x) p.luu[bt * m * m + i] = (i % m == i / m) ? 1.0 * c + p.wu[bt * m + i % m] : 0.0;
}

// What the add-on cost kernels below know of their block bt1 = b (T+1) + t, t = 0 .. T (one workgroup each): the state, and the
// gradient and Hessian they add onto -- lx / lxx of (b, t), or lfx / lfxx at t = T
struct LinCostBlock {
  int b;
  int64_t t;
  const double* q;
  double *gx, *gxx;
};
__device__ __forceinline__ LinCostBlock lin_cost_block(const LinParams& p, int64_t bt1) {
  const int64_t T = p.d.T, n = p.d.n;
  LinCostBlock k;
  k.b = (int)(bt1 / (T + 1));
  k.t = bt1 % (T + 1);
  k.q = p.x + bt1 * p.d.nx;
  k.gx = k.t < T ? p.lx + ((int64_t)k.b * T + k.t) * n : p.lfx + (int64_t)k.b * n;
  k.gxx = k.t < T ? p.lxx + ((int64_t)k.b * T + k.t) * n * n : p.lfxx + (int64_t)k.b * n * n;
  return k;
}

// The Gauss-Newton add of the terms with three axes per frame (frame positions, frame orientations, CoM), by the wave:
//   gx[i] += sum_f sum_a A_f[a][i] (w_a r_a),   gxx[i][j] += sum_f sum_a A_f[a][min] w_a A_f[a][max]
// over the tangent columns i, j < nv that some frame's mask holds (mask_of(f): the columns of A_f that are written; 0: the frame
// is left out), frames and axes in their fixed order and entry (i, j) in (min, max) order: the block stays symmetric bit for
// bit.  A: A_f[a][i] at A[f lda + 3 i + a]; w / wr: weights and weighted residuals [nf][3].  A term of weight 0 is left out, an
// entry that no frame reaches is not touched
template <class MaskOf>
__device__ __forceinline__ void gn_add_wave(int nf, MaskOf mask_of, const double* A, int lda, const double* w, const double* wr, int nv, int n,
                                            double* gx, double* gxx) {
  const int tid = threadIdx.x;
  unsigned long long all = 0;
  for (int f = 0; f < nf; ++f) all |= mask_of(f);
  for (int i = tid; i < nv; i += blockDim.x) {
    if (!((all >> i) & 1)) continue;
    double s = 0.0;
    for (int f = 0; f < nf; ++f)
      if ((mask_of(f) >> i) & 1)
        for (int a = 0; a < 3; ++a)
          if (w[3 * f + a] != 0.0) s += A[f * lda + 3 * i + a] * wr[3 * f + a];
    gx[i] += s;
  }
  for (int e = tid; e < nv * nv; e += blockDim.x) {
    const int i = e % nv, j = e / nv;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    double h = 0.0;
    bool hit = false;
    for (int f = 0; f < nf; ++f)
      if (((mask_of(f) >> i) & 1) && ((mask_of(f) >> j) & 1)) {
        hit = true;
        for (int a = 0; a < 3; ++a)
          if (w[3 * f + a] != 0.0) h += A[f * lda + 3 * lo + a] * w[3 * f + a] * A[f * lda + 3 * hi + a];
      }
    if (hit) gxx[i + (int64_t)j * n] += h;
  }
}

// Frame-position cost (DDP_HIP_FLAG_FRAME_COST, ddp_hip.h): one wave per (instance, t), t = 0 .. T, after lin_cost_kernel /
// lin_track_cost_kernel on the same stream: their output is the starting point, and only the entries of the joints on the
// frames' paths are read and rewritten.  Lane f walks frame f's path once for p_f and the path columns of its point jacobian
// P_f (rbd::frame_point_jacobian), kept in LDS; then the wave adds
//   lx[i] += sum_f sum_a P_f[a][i] (w_a r_a),   lxx[i][j] += sum_f sum_a P_f[a][min] w_a P_f[a][max]     (Gauss-Newton)
// over the tangent rows i, j < nv, frames and axes in their fixed order and entry (i, j) in (min, max) order: the block stays
// symmetric bit for bit.  A term of weight 0 is left out, a block whose weights are all 0 returns at once.  t = T: lfx / lfxx
__global__ __launch_bounds__(64) void lin_frame_cost_kernel(LinParams p, FrameCostDev fc) {
  constexpr int F = DDP_HIP_MAX_COST_FRAMES;
  const int64_t bt1 = blockIdx.x;
  const int n = (int)p.d.n, nv = (int)p.d.nv;
  const int tid = threadIdx.x, nf = fc.nf;
  const double* g = fc.target + bt1 * nf * 3;
  const double* w = fc.weight + bt1 * nf * 3;
  if (!rbd::weights_any(w, 3 * nf)) return;
  const LinCostBlock blk = lin_cost_block(p, bt1);
  __shared__ double s_P[F][3 * DDP_MAXJ], s_aw[F][9 + 3 * DDP_MAXJ], s_ow[F][3 * DDP_MAXJ], s_w[F][3], s_wr[F][3];
  __shared__ int s_chain[F][DDP_MAXJ];
  __shared__ unsigned long long s_mask[F];
  if (tid < nf) {
    unsigned long long mask = 0;
    if (rbd::frame_weights_any(w + 3 * tid)) {
      double pf[3];
      const double off[3] = {fc.off[tid][0], fc.off[tid][1], fc.off[tid][2]};
      mask = rbd::frame_point_jacobian(*p.model, fc.joint[tid], off, blk.q, pf, s_P[tid], s_chain[tid], s_aw[tid], s_ow[tid]);
      for (int a = 0; a < 3; ++a) {
        const double wa = w[3 * tid + a];
        s_w[tid][a] = wa;
        s_wr[tid][a] = wa != 0.0 ? wa * (pf[a] - g[3 * tid + a]) : 0.0;
      }
    }
    s_mask[tid] = mask;
  }
  __syncthreads();
  gn_add_wave(nf, [&](int f) { return s_mask[f]; }, &s_P[0][0], 3 * DDP_MAXJ, &s_w[0][0], &s_wr[0][0], nv, n, blk.gx, blk.gxx);
}

// Frame-orientation cost (DDP_HIP_FLAG_FRAME_ORIENT_COST, ddp_hip.h): one wave per (instance, t), t = 0 .. T, after
// lin_frame_cost_kernel and before lin_limit_cost_kernel on the same stream (the fixed order of additions: cost, tracking, frame
// positions, frame orientations, limits).  Lane f walks frame f's path once for R_f and the path columns of its world angular
// jacobian W_f (rbd::frame_rotation_jacobian), forms e_f = log3(R_ref^T R_f) and turns the columns in place into those of
// A_f = Jlog3(e_f) R_f^T W_f, kept in LDS with w o e_f; then the wave adds
//   lx[i] += sum_f sum_a A_f[a][i] (w_a e_a),   lxx[i][j] += sum_f sum_a A_f[a][min] w_a A_f[a][max]     (Gauss-Newton)
// over the columns that carry rotation (revolute joints of the path, the angular columns of a free-flyer root), frames and axes
// in their fixed order and entry (i, j) in (min, max) order: the block stays symmetric bit for bit.  Nothing else is read or
// written.  A term of weight 0 is left out, a frame whose weights are 0 is not walked, a block whose weights are all 0 returns
// at once.  t = T: lfx / lfxx
__global__ __launch_bounds__(64) void lin_frame_orient_cost_kernel(LinParams p, FrameCostDev fc) {
  constexpr int F = DDP_HIP_MAX_COST_FRAMES;
  const int64_t bt1 = blockIdx.x;
  const int n = (int)p.d.n, nv = (int)p.d.nv;
  const int tid = threadIdx.x, nf = fc.nf;
  const double* r = fc.oquat + bt1 * nf * 4;
  const double* w = fc.oweight + bt1 * nf * 3;
  if (!rbd::weights_any(w, 3 * nf)) return;
  const LinCostBlock blk = lin_cost_block(p, bt1);
  __shared__ double s_A[F][3 * DDP_MAXJ], s_w[F][3], s_we[F][3];
  __shared__ int s_chain[F][DDP_MAXJ];
  __shared__ unsigned long long s_mask[F];
  if (tid < nf) {
    unsigned long long mask = 0;
    if (rbd::frame_weights_any(w + 3 * tid)) {
      double R[9], e[3], J[9], M[9];
      mask = rbd::frame_rotation_jacobian(*p.model, fc.joint[tid], blk.q, R, s_A[tid], s_chain[tid]);
      lie::so3_log_rel(r + 4 * tid, R, e);
      lie::so3_Jlog(e, J);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[3 * i + j] = J[3 * i] * R[3 * j] + J[3 * i + 1] * R[3 * j + 1] + J[3 * i + 2] * R[3 * j + 2];   // Jlog3 R_f^T
      for (int i = 0; i < nv; ++i) {
        if (!((mask >> i) & 1)) continue;
        const double wc[3] = {s_A[tid][3 * i], s_A[tid][3 * i + 1], s_A[tid][3 * i + 2]};
        rbd::mv3(M, wc, s_A[tid] + 3 * i);
      }
      for (int a = 0; a < 3; ++a) {
        const double wa = w[3 * tid + a];
        s_w[tid][a] = wa;
        s_we[tid][a] = wa != 0.0 ? wa * e[a] : 0.0;
      }
    }
    s_mask[tid] = mask;
  }
  __syncthreads();
  gn_add_wave(nf, [&](int f) { return s_mask[f]; }, &s_A[0][0], 3 * DDP_MAXJ, &s_w[0][0], &s_we[0][0], nv, n, blk.gx, blk.gxx);
}

// Soft state limits (DDP_HIP_FLAG_STATE_LIMITS, ddp_hip.h): one wave per (instance, t), t = 0 .. T, after lin_cost_kernel /
// lin_track_cost_kernel and lin_frame_cost_kernel on the same stream: their output is the starting point.  Lane i takes the
// tangent rows i, i + 64, ...; a row of weight 0 reads neither bound, and only a violated row (e != 0) is touched:
//   lx[i] += w_i e_i,   lxx[i][i] += w_i
// Nothing else is read or written (a diagonal entry: the block stays symmetric).  Rows 0 .. 5 of a free-flyer root carry no
// limit.  t = T: lfx / lfxx
__global__ __launch_bounds__(64) void lin_limit_cost_kernel(LinParams p, StateLimitsDev sl) {
  const int64_t bt1 = blockIdx.x;
  const int n = (int)p.d.n, nv = (int)p.d.nv, nx = (int)p.d.nx, nq = nx - nv;
  const LinCostBlock blk = lin_cost_block(p, bt1);
  const double* x = blk.q;
  const double* w = sl.weight + bt1 * n;
  const double* lo = sl.lo + bt1 * n;
  const double* hi = sl.hi + bt1 * n;
  double *gx = blk.gx, *gxx = blk.gxx;
  for (int i = (nx > n ? 6 : 0) + threadIdx.x; i < n; i += blockDim.x) {
    const double wi = w[i];
    if (wi == 0.0) continue;
    const double e = limit_excess(x[limit_coord(i, nv, nq)], lo[i], hi[i]);
    if (e == 0.0) continue;
    gx[i] += wi * e;
    gxx[i + (int64_t)i * n] += wi;
  }
}

// Centre-of-mass cost (DDP_HIP_FLAG_COM_COST, ddp_hip.h): one wave per (instance, t), t = 0 .. T, after every other cost kernel
// on the same stream (the fixed order of additions: cost, tracking, frame positions, frame orientations, limits, CoM): their
// output is the starting point.  Every joint has a column, so the work is lane-parallel over joints: lane j walks its own path
// once and leaves a_j, o_j, m_j p_j and the path as a bit mask in LDS (rbd::com_stage_lane); lane j then forms the mass and
// first moment of its subtree over the records in ascending order and its column of Jc (rbd::com_column_lane); then the wave adds
//   lx[i] += sum_a Jc[a][i] (w_a r_a),   lxx[i][j] += sum_a Jc[a][min] w_a Jc[a][max]     (Gauss-Newton),   r = c(q) - g
// over the tangent rows i, j < nv, the axes in their fixed order and entry (i, j) in (min, max) order: the block stays symmetric
// bit for bit.  It reads p.x and touches nothing but those entries.  A term of weight 0 is left out, a block whose three weights
// are 0 returns at once.  t = T: lfx / lfxx
__global__ __launch_bounds__(64) void lin_com_cost_kernel(LinParams p, CoMCostDev cm) {
  const int64_t bt1 = blockIdx.x;
  const int n = (int)p.d.n, nv = (int)p.d.nv;
  const int tid = threadIdx.x;
  const double* w = cm.weight + bt1 * 3;
  if (!rbd::frame_weights_any(w)) return;
  const DevModel& m = *p.model;
  const LinCostBlock blk = lin_cost_block(p, bt1);
  const double* q = blk.q;
  __shared__ rbd::CoMWaveLds S;
  __shared__ double s_w[3], s_wr[3];
  if (tid < m.nj) rbd::com_stage_lane(m, q, tid, S);
  __syncthreads();
  if (tid < m.nj) rbd::com_column_lane(m, tid, S);
  __syncthreads();
  if (tid < 3) {
    const double wa = w[tid];
    s_w[tid] = wa;
    s_wr[tid] = wa != 0.0 ? wa * (S.c[tid] - cm.target[bt1 * 3 + tid]) : 0.0;
  }
  __syncthreads();
  gn_add_wave(1, [](int) { return ~0ull; }, S.J, 0, s_w, s_wr, nv, n, blk.gx, blk.gxx);   // one "frame" whose mask is every column
}

// Frame-velocity cost (DDP_HIP_FLAG_FRAME_VEL_COST, ddp_hip.h): one wave per (instance, t), t = 0 .. T, after every other cost
// kernel on the same stream (the fixed order of additions: cost, tracking, frame positions, frame orientations, limits, CoM, frame
// velocities).  r_f = (P_f v - g_lin, W_f v - g_ang) depends on q and on v, so A_f = [dr/d(delta q) | dr/dv] fills the q-q, q-v,
// v-q and v-v blocks on the frame's path.  Lane-parallel over joints like lin_com_cost_kernel: lane j walks its own path once and
// leaves a_j, o_j, its rate's contributions and its path as a bit mask in LDS (rbd::vel_stage_lane), then forms omega_<=j over its
// path in ascending order (rbd::vel_prefix_lane); per live frame the lanes on the frame's path form pdot_<=j alike and their
// columns of P, W, D and E (rbd::vel_frame_lane); then the wave adds the gradient rows and the path x path entries
// (rbd::vel_add_wave: entry (i, j) in (min, max) order, symmetric bit for bit).  It reads p.x and touches nothing but those
// entries.  A term of weight 0 is left out, a frame whose six weights are 0 is not walked, a block without a live weight returns
// at once.  t = T: lfx / lfxx
__global__ __launch_bounds__(64) void lin_frame_vel_cost_kernel(LinParams p, FrameVelCostDev fv) {
  const int64_t bt1 = blockIdx.x;
  const int n = (int)p.d.n, nv = (int)p.d.nv;
  const int tid = threadIdx.x, nf = fv.nf;
  const double* w = fv.weight + bt1 * nf * 6;
  if (!rbd::weights_any(w, 6 * nf)) return;
  const DevModel& m = *p.model;
  const bool ff = m.ff != 0;
  const LinCostBlock blk = lin_cost_block(p, bt1);
  const double* q = blk.q;
  const double* v = q + m.nq;
  __shared__ rbd::VelWaveLds S;
  __shared__ double s_w[6 * DDP_HIP_MAX_COST_FRAMES], s_wr[6 * DDP_HIP_MAX_COST_FRAMES];
  if (tid < m.nj) rbd::vel_stage_lane(m, q, v, tid, S);
  for (int f = 0; f < nf; ++f)
    if (tid == 63 - f && (rbd::frame_weights_any(w + 6 * f) || rbd::frame_weights_any(w + 6 * f + 3)))
      rbd::frame_point(m, ff, fv.joint[f], fv.off[f], q, S.p[f]);
  __syncthreads();
  if (tid < m.nj) rbd::vel_prefix_lane(tid, S);
  __syncthreads();
  unsigned long long U = 0;
  for (int f = 0; f < nf; ++f) {
    const bool lin = rbd::frame_weights_any(w + 6 * f), ang = rbd::frame_weights_any(w + 6 * f + 3);
    if (!lin && !ang) continue;
    U |= rbd::tangent_mask(ff, S.jw.mask[fv.joint[f]]);
    if (tid < m.nj) rbd::vel_frame_lane(m, tid, f, fv.joint[f], lin, ang, S);
  }
  rbd::column_index_lane(U, tid, S.idx);
  __syncthreads();
  if (tid < 6 * nf) {
    const double wa = w[tid];
    s_w[tid] = wa;
    s_wr[tid] = wa != 0.0 ? wa * (S.vel[tid / 6][tid % 6] - fv.target[bt1 * nf * 6 + tid]) : 0.0;
  }
  __syncthreads();
  double *gx = blk.gx, *gxx = blk.gxx;
  rbd::vel_add_wave(S, nf, s_w, s_wr, __builtin_popcountll(U), tid, (int)blockDim.x, nv, n, gx, gxx);
}

// Centroidal-momentum cost (DDP_HIP_FLAG_MOMENTUM_COST, ddp_hip.h): one wave per (instance, t), t = 0 .. T, after every other cost
// kernel on the same stream (the fixed order of additions: ..., CoM, frame velocities, momentum).  r = h(q, v) - g depends on q and
// on v and every joint has a column in both halves of A = [dh/d(delta q) | dh/dv], so the term fills all of lx and lxx.  Lane-parallel
// over joints like lin_com_cost_kernel: lane j walks its own path once and leaves a_j, o_j, its path, its body's mass, first moment
// and inertia about the world origin and its own rate's twist in LDS (rbd::mom_stage_lane), then forms its body's twist over its
// path in ascending order and the body's momentum (rbd::mom_prefix_lane), then mass, first moment, inertia and momentum of its
// subtree over the records in ascending order and from them its column(s) of A (rbd::mom_column_lane); then the wave adds the
// gradient rows and the entries (rbd::vel_add_wave with one "frame" over every column: entry (i, j) in (min, max) order, symmetric
// bit for bit).  It reads p.x and touches nothing but lx / lxx.  A term of weight 0 is left out, with the three angular weights 0
// no inertia and no angular quantity is formed, a block whose six weights are 0 returns at once.  t = T: lfx / lfxx
__global__ __launch_bounds__(64) void lin_momentum_cost_kernel(LinParams p, MomentumCostDev mo) {
  const int64_t bt1 = blockIdx.x;
  const int n = (int)p.d.n, nv = (int)p.d.nv;
  const int tid = threadIdx.x;
  const double* w = mo.weight + bt1 * 6;
  if (!rbd::weights_any(w, 6)) return;
  const bool ang = rbd::frame_weights_any(w + 3);
  const DevModel& m = *p.model;
  const LinCostBlock blk = lin_cost_block(p, bt1);
  const double* q = blk.q;
  __shared__ rbd::MomWaveLds S;
  __shared__ double s_w[6], s_wr[6];
  rbd::mom_jacobians_wave(m, q, q + m.nq, tid, ang, S);
  if (tid < 6) {
    const double wa = w[tid];
    s_w[tid] = wa;
    s_wr[tid] = wa != 0.0 ? wa * (S.h[tid] - mo.target[bt1 * 6 + tid]) : 0.0;
  }
  __syncthreads();
  double *gx = blk.gx, *gxx = blk.gxx;
  rbd::vel_add_wave(S, 1, s_w, s_wr, nv, tid, (int)blockDim.x, nv, n, gx, gxx);
}

// Balance-region cost (DDP_HIP_FLAG_BALANCE_REGION_COST, ddp_hip.h): one wave per (instance, t), t = 0 .. T, after every other cost
// kernel on the same stream (the fixed order of additions: ..., frame velocities, momentum, balance regions).  The penalty is
// one-sided, so most waves have nothing to add: a block whose weights are all 0 returns at once, before any LDS access or barrier,
// and one whose live planes are all clear returns after the values, before any jacobian.  Lane j < nj walks its joint's path once
// and leaves a_j, o_j, its path, m_j and m_j p_j in LDS -- and, where a live plane has tau != 0, its rate's twist, then its body's
// twist and linear momentum (rbd::region_stage_wave: the CoM's stage lane, or the momentum's stage and prefix lanes with
// ang = false).  Lane o < n_planes folds c (and cdot) over the records in ascending order and leaves w, w e, tau and whether plane
// o is active.  Then lane j forms its column(s) of Jc (rbd::com_column_lane) and, where an active plane has tau != 0, of
// dl/d(delta q) (rbd::mom_column_lane, ang = false); the wave stages z_o of the active planes (rbd::region_stage_z) and adds the
// gradient rows and the entries (rbd::region_add_wave: planes ascending, entry (i, j) in (min, max) order, symmetric bit for bit).
// A plane with tau = 0 touches no v row or column.  It reads p.x and touches nothing but lx / lxx.  No scratch, no atomics.
// t = T: lfx / lfxx
__global__ __launch_bounds__(64) void lin_balance_region_cost_kernel(LinParams p, BalanceRegionDev br) {
  const int64_t bt1 = blockIdx.x;
  const int n = (int)p.d.n, nv = (int)p.d.nv;
  const int tid = threadIdx.x, np = br.np;
  const double* w = br.weight + bt1 * np;
  if (!rbd::weights_any(w, np)) return;
  const double* geom = br.geom + bt1 * np * 5;
  const DevModel& m = *p.model;
  const LinCostBlock blk = lin_cost_block(p, bt1);
  const double* q = blk.q;
  __shared__ rbd::BalanceWaveLds S;
  const bool rate = rbd::region_needs_rate(geom, w, np);
  rbd::region_stage_wave(m, q, q + m.nq, tid, rate, S);
  if (tid < np) {
    const double wo = w[tid];
    double we = 0.0;
    int act = 0;
    if (wo != 0.0) {
      double c[3], cd[3] = {0.0, 0.0, 0.0};
      rbd::region_point_lds(S, m.nj, rate, c, cd);
      const double d = rbd::region_distance(geom + 5 * tid, c, cd);
      if (rbd::obstacle_active(d)) { act = 1; we = wo * d; }
    }
    S.w[tid] = wo; S.we[tid] = we; S.tau[tid] = geom[5 * tid + 4]; S.act[tid] = act;
  }
  __syncthreads();
  bool any = false, rate_q = false;
  for (int o = 0; o < np; ++o)
    if (S.act[o]) { any = true; rate_q |= S.tau[o] != 0.0; }
  if (!any) return;
  rbd::region_columns_wave(m, tid, rate_q, S);
  rbd::region_stage_z(m, geom, np, tid, (int)blockDim.x, S);
  __syncthreads();
  double *gx = blk.gx, *gxx = blk.gxx;
  rbd::region_add_wave(S, np, nv, tid, (int)blockDim.x, n, gx, gxx);
}

// Relative-frame cost (DDP_HIP_FLAG_RELATIVE_FRAME_COST, ddp_hip.h): one wave per (instance, t), t = 0 .. T, after every other cost
// kernel on the same stream (the fixed order of additions: ..., momentum, balance regions, relative frames).  A block whose
// weights are all 0 returns at once, before any LDS access or barrier.  Lanes j < nj stage world axis, world origin and path of
// their joint in LDS (rbd::stage_joint_lane); lane 63 - i walks live pair i (rbd::relative_placement: two walks; the top lanes, so
// that on a robot of fewer than 60 joints no lane does both) and leaves R_a^T, Jlog3(e) R_b^T, p_b, w and w o r.  After the barrier
// every lane forms the two halves of each live pair's symmetric difference, path(ja) \ path(jb) and path(jb) \ path(ja), as column
// masks; their union is compacted (rbd::column_index_lane) and the 6 x n_u columns of each live pair are staged in LDS
// (rbd::relative_frame_stage_columns).  A joint on both paths moves both frames alike and is in neither half: the wave adds over
// the union of the symmetric differences alone (rbd::relative_frame_add_wave: pairs ascending, position axes, then rotation axes,
// entry (i, j) in (min, max) order, symmetric bit for bit).  It reads p.x and touches nothing but those entries.  A term of weight
// 0 is left out, a pair whose six weights are 0 is not walked, one whose rotation (position) weights are 0 reads no quaternion and
// forms no log (reads no target).  No scratch, no atomics.  t = T: lfx / lfxx
__global__ __launch_bounds__(64) void lin_relative_frame_cost_kernel(LinParams p, RelativeFrameDev rf) {
  const int64_t bt1 = blockIdx.x;
  const int n = (int)p.d.n;
  const int tid = threadIdx.x, np = rf.np;
  const double* w = rf.weight + bt1 * np * 6;
  if (!rbd::weights_any(w, 6 * np)) return;
  const DevModel& m = *p.model;
  const bool ff = m.ff != 0;
  const LinCostBlock blk = lin_cost_block(p, bt1);
  const double* q = blk.q;
  __shared__ rbd::RelativeWaveLds S;
  if (tid < m.nj) rbd::stage_joint_lane<0>(m, q, tid, S.jw, nullptr);
  const int i = 63 - tid;
  if (i < np && rbd::weights_any(w + 6 * i, 6)) {
    const bool pos = rbd::frame_weights_any(w + 6 * i), rot = rbd::frame_weights_any(w + 6 * i + 3);
    rbd::RelativePlacement P;
    rbd::relative_placement(m, ff, rf.ja[i], rf.offa[i], rf.jb[i], rf.offb[i], q, rot, P);
    double r[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    rbd::relative_frame_residual(P, pos ? rf.target + (bt1 * np + i) * 3 : nullptr, rot ? rf.quat + (bt1 * np + i) * 4 : nullptr, r);
    for (int k = 0; k < 3; ++k) {
      S.pb[i][k] = P.pb[k];
      for (int a = 0; a < 3; ++a) S.RaT[i][3 * k + a] = P.ca[k][a];
    }
    if (rot) {
      double J[9];
      lie::so3_Jlog(r + 3, J);
      for (int k = 0; k < 3; ++k)
        for (int a = 0; a < 3; ++a) S.JR[i][3 * k + a] = J[3 * k] * P.cb[0][a] + J[3 * k + 1] * P.cb[1][a] + J[3 * k + 2] * P.cb[2][a];   // Jlog3 R_b^T
    }
    for (int a = 0; a < 6; ++a) {
      const double wa = w[6 * i + a];
      S.w[i][a] = wa;
      S.wr[i][a] = wa != 0.0 ? wa * r[a] : 0.0;
    }
  }
  // the tangent columns of the revolute joints: the ones that carry rotation (a free-flyer root's are on every path)
  const unsigned long long revj = __ballot(tid < m.nj && !(ff && tid == 0) && m.jtype[tid] == DDP_HIP_JOINT_REVOLUTE);
  const unsigned long long rot_cols = ff ? (revj >> 1) << 6 : revj;
  __syncthreads();
  unsigned long long U = 0;
  for (int k = 0; k < np; ++k) {
    unsigned long long ca = 0, cb = 0;
    if (rbd::weights_any(w + 6 * k, 6)) {
      const unsigned long long ma = rbd::tangent_mask(ff, S.jw.mask[rf.ja[k]]), mb = rbd::tangent_mask(ff, S.jw.mask[rf.jb[k]]);
      ca = ma & ~mb;
      cb = mb & ~ma;
      U |= ca | cb;
    }
    if (k == tid) { S.ca[k] = ca; S.cb[k] = cb; }
  }
  rbd::column_index_lane(U, tid, S.idx);
  __syncthreads();
  const int nu = __builtin_popcountll(U);
  rbd::relative_frame_stage_columns(m, S, np, nu, tid, (int)blockDim.x);
  __syncthreads();
  double *gx = blk.gx, *gxx = blk.gxx;
  rbd::relative_frame_add_wave(S, np, rot_cols, nu, tid, (int)blockDim.x, n, gx, gxx);
}

// Control-gravity cost (DDP_HIP_FLAG_CONTROL_GRAV_COST, ddp_hip.h): one wave per (instance, t), t = 0 .. T-1, after every other
// cost kernel on the same stream (the fixed order of additions: ..., momentum, relative frames, control-gravity).  The first add-on
// kernel that writes lu / luu / lux.  A block whose m weights are all 0 returns at once, before any LDS access or barrier.  Lanes
// j < nj stage world axis, world origin, path, mass and first moment of their joint (rbd::grav_stage_lane), then form their
// subtree's sums and D, D x F and g of their tangent (rbd::grav_tangent_lane); lane i < m leaves w_i, w_i r_i (r = u - g - o) and
// makes the two additions of its own row, lu[i] += w_i r_i and luu[i][i] += w_i.  Then the wave forms the entries of G on the
// pattern into dynamic LDS (s_G[i nv + c] = G_ic, nv^2 doubles; an entry off the pattern is neither formed nor read) with
// lux[i][c] += -(w_i G_ic) for the live rows on the way, lane c gathers rel[c], the live rows whose G_ic is on the pattern, and
//   lx[c] += -sum_{i in rel[c]} G_ic (w_i r_i),      lxx[a][b] += sum_{i in rel[a] & rel[b]} G_i,min w_i G_i,max      (Gauss-Newton)
// rows ascending, entry (a, b) in (min, max) order: the block stays symmetric bit for bit.  An entry that no live row reaches is
// not written, a row of weight 0 is in no rel[].  It reads p.x and p.u.  No scratch, no atomics
__global__ __launch_bounds__(64) void lin_control_grav_cost_kernel(LinParams p, ControlGravDev cg) {
  const int64_t T = p.d.T;
  const int64_t bt = blockIdx.x;                        // b T + t, t < T: the record has no terminal row
  const int n = (int)p.d.n, nv = (int)p.d.nv, mu = (int)p.d.m;
  const int tid = threadIdx.x;
  const double* w = cg.weight + bt * mu;
  if (!rbd::weights_any(w, mu)) return;
  const DevModel& m = *p.model;
  const bool ff = m.ff != 0;
  const int64_t b = bt / T, t = bt % T;
  const double* q = p.x + (b * (T + 1) + t) * p.d.nx;
  __shared__ rbd::GravWaveLds S;
  __shared__ double s_w[DDP_MAXJ], s_wr[DDP_MAXJ];
  __shared__ unsigned long long s_rel[DDP_MAXJ];
  extern __shared__ double s_G[];
  if (tid < m.nj) rbd::grav_stage_lane(m, q, tid, S);
  const unsigned long long rot = __ballot(tid < nv && rbd::grav_tangent_rotational(m, ff, tid < nv ? tid : 0));
  const unsigned long long live = __ballot(tid < mu && w[tid < mu ? tid : 0] != 0.0);
  __syncthreads();
  rbd::grav_tangent_lane(m, tid, rot, S);
  __syncthreads();
  if (tid < mu) {
    const double wi = w[tid];
    double wr = 0.0;
    if (wi != 0.0) {
      wr = wi * (p.u[bt * mu + tid] - S.g[tid] - cg.offset[bt * mu + tid]);
      p.lu[bt * mu + tid] += wr;
      p.luu[bt * mu * mu + tid + (int64_t)tid * mu] += wi;
    }
    s_w[tid] = wi;
    s_wr[tid] = wr;
  }
  double* lux = p.lux + bt * mu * n;
  for (int e = tid; e < nv * nv; e += (int)blockDim.x) {
    const int c = e % nv, i = e / nv;
    double gic;
    if (!rbd::grav_entry(S, ff, i, c, &gic)) continue;
    s_G[e] = gic;
    if ((live >> i) & 1) lux[i + (int64_t)c * mu] += -(w[i] * gic);
  }
  if (tid < nv) {
    unsigned long long rel = 0;
    double unused;
    for (int i = 0; i < nv; ++i)
      if (((live >> i) & 1) && rbd::grav_entry(S, ff, i, tid, &unused)) rel |= 1ull << i;
    s_rel[tid] = rel;
  }
  __syncthreads();
  double* gx = p.lx + bt * n;
  double* gxx = p.lxx + bt * n * n;
  if (tid < nv && s_rel[tid]) {
    double s = 0.0;
    for (unsigned long long r = s_rel[tid]; r; r &= r - 1) {
      const int i = __builtin_ctzll(r);
      s += s_G[i * nv + tid] * s_wr[i];
    }
    gx[tid] += -s;
  }
  for (int e = tid; e < nv * nv; e += (int)blockDim.x) {
    const int a = e % nv, c = e / nv;
    const unsigned long long both = s_rel[a] & s_rel[c];
    if (!both) continue;
    const int lo = a < c ? a : c, hi = a < c ? c : a;
    double h = 0.0;
    for (unsigned long long r = both; r; r &= r - 1) {
      const int i = __builtin_ctzll(r);
      h += s_G[i * nv + lo] * s_w[i] * s_G[i * nv + hi];
    }
    gxx[a + (int64_t)c * n] += h;
  }
}

// Frame-aiming cost (DDP_HIP_FLAG_FRAME_AIM_COST, ddp_hip.h): one wave per (instance, t), t = 0 .. T, after every other cost kernel
// on the same stream (the fixed order of additions: ..., relative frames, control-gravity, frame aiming).  A block whose weights
// are all 0 returns at once, before any LDS access or barrier.  Lanes j < nj stage world axis, world origin and path of their
// joint in LDS (rbd::stage_joint_lane); lane 63 - i walks frame i (rbd::frame_aim_stage_frame: one walk with the eye and the axis;
// the top lanes, so that on a robot of fewer than 60 joints no lane does both) and leaves p, n, the line of sight, 1 / l, w and
// w o r -- or that the frame forms nothing here (both weights 0: no walk; l <= 1e-12).  After the barrier every lane forms the live
// frames' paths as column masks; their union is compacted (rbd::column_index_lane) and the 4 x n_u columns of each live frame are
// staged in LDS (rbd::frame_aim_stage_columns), then the wave adds over the union alone (rbd::frame_aim_add_wave: frames ascending,
// the three aim rows, then the range row, entry (i, j) in (min, max) order, symmetric bit for bit).  It reads p.x and touches
// nothing but those entries.  A term of weight 0 is left out: with w_aim = 0 no aim row is formed, with w_range = 0 rho is not
// read.  No scratch, no atomics.  t = T: lfx / lfxx
__global__ __launch_bounds__(64) void lin_frame_aim_cost_kernel(LinParams p, FrameAimDev fa) {
  const int64_t bt1 = blockIdx.x;
  const int n = (int)p.d.n;
  const int tid = threadIdx.x, nf = fa.nf;
  const double* w = fa.weight + bt1 * nf * 2;
  if (!rbd::weights_any(w, 2 * nf)) return;
  const DevModel& m = *p.model;
  const bool ff = m.ff != 0;
  const LinCostBlock blk = lin_cost_block(p, bt1);
  const double* q = blk.q;
  __shared__ rbd::FrameAimWaveLds S;
  if (tid < m.nj) rbd::stage_joint_lane<0>(m, q, tid, S.jw, nullptr);
  const int i = 63 - tid;
  if (i < nf) rbd::frame_aim_stage_frame(m, ff, fa, i, q, fa.target + (bt1 * nf + i) * 4, w + 2 * i, S);
  __syncthreads();
  unsigned long long U = 0;
  for (int k = 0; k < nf; ++k) {
    const unsigned long long ck = S.live[k] ? rbd::tangent_mask(ff, S.jw.mask[fa.joint[k]]) : 0ull;
    U |= ck;
    if (k == tid) S.cols[k] = ck;
  }
  rbd::column_index_lane(U, tid, S.idx);
  __syncthreads();
  const int nu = __builtin_popcountll(U);
  rbd::frame_aim_stage_columns(m, S, nf, nu, tid, (int)blockDim.x);
  __syncthreads();
  double *gx = blk.gx, *gxx = blk.gxx;
  rbd::frame_aim_add_wave(S, nf, nu, tid, (int)blockDim.x, n, gx, gxx);
}

// Joint-acceleration cost (DDP_HIP_FLAG_JOINT_ACCEL_COST, ddp_hip.h): one wave per (instance, t), t = 0 .. T-1, after every other
// cost kernel on the same stream (the fixed order of additions: ..., control-gravity, frame aiming, joint accelerations).  A block
// whose nv weights are all 0 returns at once, before any LDS access or barrier.  The wave runs the analytic recursion of
// rbd_deriv.h at (x_t, u_t) (tree_derivatives_wave on a fixed base, ff_derivatives_wave on a free-flyer root: analytic whatever
// the context's first order is; FX / FU are not read), which leaves T = [dtau/dq | dtau/dv], M^-1 and a = qdd in LDS.  Then
//   Z = [Zq Zv] = -M^-1 T, row-major nv x 2 nv, over the spent M and column records of FfLds (contiguous; the rows of weight != 0),
//   Zu = M^-1 where it stands (Zu_rj = X[r + j nv]),   w and w o r (r = a - a_ref) over the spent local placements,
// and the five additions, each entry by one lane as a sum over the rows of weight != 0 in ascending order (no atomics):
//   lx[j] += sum_r Z_rj (w r)_r,   lu[j] += sum_r Zu_rj (w r)_r,   lux[j][c] += sum_r Zu_rj w_r Z_rc,
//   lxx[a][c] += sum_r Z_ra w_r Z_rc,   luu[a][c] += sum_r Zu_ra w_r Zu_rc      for a >= c, the same number added at [c][a]:
// Gauss-Newton, symmetric bit for bit.  The products run on the vector ALU (lanes along a row of Z: conflict-free LDS reads, the
// other operand a broadcast).  No scratch; dynamic LDS FfLds<NJ>::TOTAL doubles
template <int NJ>
__global__ __launch_bounds__(64) void lin_joint_accel_cost_kernel(LinParams p, JointAccelDev ja) {
  typedef rbdd::FfLds<NJ> L;
  static_assert(NJ * NJ + L::CR * NJ >= 2 * NJ * NJ, "Z must fit over M and the column records");
  const int64_t T = p.d.T;
  const int64_t bt = blockIdx.x;                        // b T + t, t < T
  const int64_t row = bt / T * (T + 1) + bt % T;        // the record and X have T+1 rows per instance
  const int N = (int)p.d.nv, W2 = 2 * N, n = (int)p.d.n, mu = (int)p.d.m;
  const int tid = threadIdx.x;
  const double* w = ja.weight + row * N;
  if (!rbd::weights_any(w, N)) return;
  const DevModel& m = *p.model;
  const double* x = p.x + row * p.d.nx;
  const double* u = p.u + bt * mu;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  if (m.ff) rbdd::ff_derivatives_wave<NJ>(m, x, x + m.nq, u, lds, tid);
  else rbdd::tree_derivatives_wave<NJ>(m, x, x + m.nq, u, lds, tid);
  const double* s_X = lds + L::X;
  const double* s_T = lds + L::T;
  double* s_Z = lds + L::M;
  double* s_w = lds + L::LOC;
  double* s_wr = s_w + NJ;
  if (tid < N) {
    const double wi = w[tid];
    s_w[tid] = wi;
    s_wr[tid] = wi != 0.0 ? wi * (rbdd::wave_qdd<NJ>(lds)[tid] - ja.target[row * N + tid]) : 0.0;
  }
  __syncthreads();
  for (int r = 0; r < N; ++r) {
    if (s_w[r] == 0.0) continue;
    for (int j = tid; j < W2; j += 64) {
      double s = 0.0;
      for (int l = 0; l < N; ++l) s += s_X[r + l * N] * s_T[l * W2 + j];
      s_Z[r * W2 + j] = -s;
    }
  }
  __syncthreads();
  double* gx = p.lx + bt * n;
  double* gxx = p.lxx + bt * n * n;
  double* gu = p.lu + bt * mu;
  double* guu = p.luu + bt * mu * mu;
  double* gux = p.lux + bt * mu * n;
  for (int j = tid; j < W2; j += 64) {
    double s = 0.0;
    for (int r = 0; r < N; ++r)
      if (s_w[r] != 0.0) s += s_Z[r * W2 + j] * s_wr[r];
    gx[j] += s;
  }
  if (tid < N) {
    double s = 0.0;
    for (int r = 0; r < N; ++r)
      if (s_w[r] != 0.0) s += s_X[r + tid * N] * s_wr[r];
    gu[tid] += s;
  }
  for (int c = 0; c < W2; ++c)
    for (int a = c + tid; a < W2; a += 64) {
      double h = 0.0;
      for (int r = 0; r < N; ++r)
        if (s_w[r] != 0.0) h += s_Z[r * W2 + a] * s_w[r] * s_Z[r * W2 + c];
      gxx[a + (int64_t)c * n] += h;
      if (a != c) gxx[c + (int64_t)a * n] += h;
    }
  for (int j = 0; j < N; ++j)
    for (int c = tid; c < W2; c += 64) {
      double h = 0.0;
      for (int r = 0; r < N; ++r)
        if (s_w[r] != 0.0) h += s_X[r + j * N] * s_w[r] * s_Z[r * W2 + c];
      gux[j + (int64_t)c * mu] += h;
    }
  for (int c = 0; c < N; ++c)
    for (int a = c + tid; a < N; a += 64) {
      double h = 0.0;
      for (int r = 0; r < N; ++r)
        if (s_w[r] != 0.0) h += s_X[r + a * N] * s_w[r] * s_X[r + c * N];
      guu[a + (int64_t)c * mu] += h;
      if (a != c) guu[c + (int64_t)a * mu] += h;
    }
}

// Obstacle cost (DDP_HIP_FLAG_OBSTACLE_COST, ddp_hip.h): one wave per (instance, t), t = 0 .. T, after every other cost kernel
// on the same stream (the fixed order of additions: ..., frame aiming, joint accelerations, obstacles).  The penalty is one-sided, so most
// waves have nothing to add and must cost next to nothing.  A block whose weights are all 0 returns at once.  Phase 1: lane
// k < n_points walks point k (rbd::frame_point) and runs over its live slots in ascending order; a lane with an active pair
// (w != 0, e != 0, a direction u) forms g_k = sum_o w e u and the symmetric M_k = sum_o w u u^T on the way, in registers.  One
// wave-level vote (no LDS, no barrier) decides: a wave without an active pair returns here.  Phase 2: lanes j < nj stage world
// axis, world origin and path of their joint in LDS (rbd::stage_joint_lane), the active lanes their p_k, g_k, M_k; the wave
// then adds, over the union of the active points' paths alone,
//   lx[i] += sum_k P_k[:, i] . g_k,     lxx[i][j] += sum_k P_k[:, min]^T M_k P_k[:, max]     (Gauss-Newton)
// with the columns of P_k formed from the staged axes and origins (rbd::obstacle_add_wave: points in ascending order, entry
// (i, j) in (min, max) order, symmetric bit for bit).  It reads p.x and touches nothing but those entries.  No atomics.
// t = T: lfx / lfxx
template <bool GRID>
__global__ __launch_bounds__(64) void lin_obstacle_cost_kernel(LinParams p, ObstacleCostDev ob) {
  const int64_t bt1 = blockIdx.x;
  const int n = (int)p.d.n;
  const int tid = threadIdx.x;
  const double* w = ob.weight + bt1 * ob.no;
  if (!rbd::weights_any(w, ob.no)) return;
  const DevModel& m = *p.model;
  const bool ff = m.ff != 0;
  const LinCostBlock blk = lin_cost_block(p, bt1);
  const double* q = blk.q;
  double pk[3] = {0.0, 0.0, 0.0}, g[3], M[6];
  bool act = false;
  if (tid < ob.np) {
    const double off[3] = {ob.off[tid][0], ob.off[tid][1], ob.off[tid][2]};
    rbd::frame_point(m, ff, ob.joint[tid], off, q, pk);
    act = rbd::obstacle_point_reduce<GRID>(ob, tid, pk, ob.geom + bt1 * ob.no * 4, w, g, M);
  }
  const unsigned active = (unsigned)__ballot(act);                  // bit k: point k has an active pair
  if (active == 0) return;
  __shared__ rbd::ObstacleWaveLds S;
  if (tid < m.nj) rbd::stage_joint_lane<0>(m, q, tid, S.jw, nullptr);
  if (act) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { S.p[tid][a] = pk[a]; S.g[tid][a] = g[a]; }
#pragma unroll
    for (int a = 0; a < 6; ++a) S.M[tid][a] = M[a];
  }
  __syncthreads();
  unsigned long long U = 0;
  for (int k = 0; k < ob.np; ++k)
    if ((active >> k) & 1) U |= rbd::tangent_mask(ff, S.jw.mask[ob.joint[k]]);
  rbd::column_index_lane(U, tid, S.idx);
  __syncthreads();
  double *gx = blk.gx, *gxx = blk.gxx;
  rbd::obstacle_add_wave(m, S, ob, active, __builtin_popcountll(U), tid, (int)blockDim.x, n, gx, gxx);
}

// Self-collision cost (DDP_HIP_FLAG_SELF_COLLISION_COST, ddp_hip.h): one wave per (instance, t), t = 0 .. T, after every other cost
// kernel on the same stream (the fixed order of additions: ..., joint accelerations, obstacles, self-collision).  One-sided like the
// obstacle cost: most waves have nothing to add.  A block whose weights are all 0 returns at once.  Phase 1: lane k < n_points
// walks sphere k (rbd::frame_point); lane i < n_pairs fetches p_a and p_b from the lanes that hold them (cross-lane reads: no
// LDS) and forms d_i.  One wave-level vote decides: a wave without an active pair (w != 0, e != 0, a direction u) returns here,
// before any LDS access or barrier.  Phase 2: lanes j < nj stage world axis, world origin and path of their joint in LDS
// (rbd::stage_joint_lane), lanes k < n_points their p_k, the active pairs' lanes u_i, w_i, w_i e_i; after the barrier the same
// lanes leave the two halves of their pair's symmetric difference, path(a) \ path(b) and path(b) \ path(a), as column masks.  A
// joint on both paths moves both spheres alike and is in neither: the wave adds over the union of the symmetric differences alone
//   lx[c] += sum_i (w e)_i z_i[c],     lxx[r][c] += sum_i w_i z_i[min] z_i[max]     (Gauss-Newton)
// (rbd::self_collision_add_wave: pairs in ascending order, z formed on the fly, symmetric bit for bit).  It reads p.x and touches
// nothing but those entries.  No atomics.  t = T: lfx / lfxx
__global__ __launch_bounds__(64) void lin_self_collision_cost_kernel(LinParams p, SelfCollisionDev sc) {
  const int64_t bt1 = blockIdx.x;
  const int n = (int)p.d.n;
  const int tid = threadIdx.x;
  const double* w = sc.weight + bt1 * sc.npair;
  if (!rbd::weights_any(w, sc.npair)) return;
  const DevModel& m = *p.model;
  const bool ff = m.ff != 0;
  const LinCostBlock blk = lin_cost_block(p, bt1);
  const double* q = blk.q;
  double pk[3] = {0.0, 0.0, 0.0};
  if (tid < sc.np) {
    const double off[3] = {sc.off[tid][0], sc.off[tid][1], sc.off[tid][2]};
    rbd::frame_point(m, ff, sc.joint[tid], off, q, pk);
  }
  const bool pair_lane = tid < sc.npair;
  const int ia = pair_lane ? sc.pa[tid] : 0, ib = pair_lane ? sc.pb[tid] : 0;
  const double pa[3] = {__shfl(pk[0], ia), __shfl(pk[1], ia), __shfl(pk[2], ia)};
  const double pb[3] = {__shfl(pk[0], ib), __shfl(pk[1], ib), __shfl(pk[2], ib)};
  double d = 0.0, u[3] = {0.0, 0.0, 0.0}, wi = 0.0;
  bool act = false;
  if (pair_lane) {
    wi = w[tid];
    if (wi != 0.0) {
      const bool has_u = rbd::self_collision_distance(sc, tid, pa, pb, sc.margin[bt1 * sc.npair + tid], &d, u);
      act = rbd::obstacle_active(d) && has_u;
    }
  }
  const unsigned active = (unsigned)__ballot(act);                  // bit i: pair i is active
  if (active == 0) return;
  __shared__ rbd::SelfCollisionWaveLds S;
  if (tid < m.nj) rbd::stage_joint_lane<0>(m, q, tid, S.jw, nullptr);
  if (tid < sc.np) { S.p[tid][0] = pk[0]; S.p[tid][1] = pk[1]; S.p[tid][2] = pk[2]; }
  if (act) {
    S.u[tid][0] = u[0]; S.u[tid][1] = u[1]; S.u[tid][2] = u[2];
    S.w[tid] = wi;
    S.we[tid] = wi * d;
  }
  __syncthreads();
  unsigned long long U = 0;
  for (int i = 0; i < sc.npair; ++i) {
    if (!((active >> i) & 1)) continue;
    const unsigned long long ma = rbd::tangent_mask(ff, S.jw.mask[sc.joint[sc.pa[i]]]), mb = rbd::tangent_mask(ff, S.jw.mask[sc.joint[sc.pb[i]]]);
    U |= ma ^ mb;
    if (i == tid) { S.ca[i] = ma & ~mb; S.cb[i] = mb & ~ma; }
  }
  rbd::column_index_lane(U, tid, S.idx);
  __syncthreads();
  double *gx = blk.gx, *gxx = blk.gxx;
  rbd::self_collision_add_wave(m, S, sc, active, __builtin_popcountll(U), tid, (int)blockDim.x, n, gx, gxx);
}

// Capsule cost (DDP_HIP_FLAG_CAPSULE_COST, ddp_hip.h): one wave per (instance, t), t = 0 .. T, after every other cost kernel on the
// same stream (the fixed order of additions: ..., obstacles, self-collision, capsules).  One-sided like its two siblings: most waves
// have nothing to add.  A block whose weights are all 0 returns at once.  Phase 1: lane k < n_capsules walks both ends of capsule
// k in one walk (rbd::capsule_ends); lane i < n_pairs fetches the ends of its pair's robot capsules from the lanes that hold them
// (cross-lane reads: no LDS), reads a world body from the pair's geometry, and forms the closest points and d_i
// (rbd::capsule_distance).  One wave-level vote decides: a wave without an active pair (w != 0, e != 0, a direction u) returns
// here, before any LDS access or barrier.  Phase 2: lanes j < nj stage world axis, world origin and path of their joint in LDS
// (rbd::stage_joint_lane), the active pairs' lanes c_a, c_b, u_i, w_i, w_i e_i; after the barrier the same lanes leave their
// pair's two column masks: path(A) \ path(B) and path(B) \ path(A) of a robot pair, all of path(A) and nothing of a world pair.
// The wave adds over the union of the masks alone
//   lx[c] += sum_i (w e)_i z_i[c],     lxx[r][c] += sum_i w_i z_i[min] z_i[max]     (Gauss-Newton)
// (rbd::capsule_add_wave: pairs in ascending order, z formed on the fly at the closest points frozen in their joints, symmetric bit
// for bit).  It reads p.x and touches nothing but those entries.  No atomics.  t = T: lfx / lfxx.
// GRID (some pair is of kind DDP_HIP_CAPSULE_VS_GRID; the other instantiation is the code from before the kind): the capsules' lanes
// leave their ends in LDS, and the wave's 64 lanes take the (grid pair, sample) items of the description's flat list in strides
// and leave phi of each in LDS (the pairs with w == 0 are not looked up).  After a barrier a grid pair's own lane scans its values
// in ascending j (capsule_grid_better: smallest j on a tie, the first NaN before everything -- whatever the dealing) and forms the
// point and the gradient at j* by the sample routine again: the same bits as the scan on one lane (capsule_grid_closest).  The
// vote and everything behind it are as before.
// BOX (some pair is of kind DDP_HIP_CAPSULE_VS_BOX): the pair's own lane evaluates capsule_box_closest in phase 1 (rbd::capsule_distance);
// a box pair is a world pair with c_b = c_a and everything behind the vote is as before
static_assert(sizeof(LinParams) + sizeof(CapsuleCostDev) <= 4096, "the kernel's arguments must fit the kernarg segment");
template <bool GRID, bool BOX>
__global__ __launch_bounds__(64) void lin_capsule_cost_kernel(LinParams p, CapsuleCostDev cp) {
  const int64_t bt1 = blockIdx.x;
  const int n = (int)p.d.n;
  const int tid = threadIdx.x;
  const double* w = cp.weight + bt1 * cp.npair;
  if (!rbd::weights_any(w, cp.npair)) return;
  const DevModel& m = *p.model;
  const bool ff = m.ff != 0;
  const LinCostBlock blk = lin_cost_block(p, bt1);
  const double* q = blk.q;
  double e[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  if (tid < cp.nc) rbd::capsule_ends(m, ff, cp, tid, q, e);
  const bool pair_lane = tid < cp.npair;
  const int ia = pair_lane ? cp.pa[tid] : 0, ib = pair_lane ? cp.pb[tid] : 0;
  const double a0[3] = {__shfl(e[0][0], ia), __shfl(e[0][1], ia), __shfl(e[0][2], ia)};
  const double a1[3] = {__shfl(e[1][0], ia), __shfl(e[1][1], ia), __shfl(e[1][2], ia)};
  const double b0[3] = {__shfl(e[0][0], ib), __shfl(e[0][1], ib), __shfl(e[0][2], ib)};
  const double b1[3] = {__shfl(e[1][0], ib), __shfl(e[1][1], ib), __shfl(e[1][2], ib)};
  double d = 0.0, ca[3] = {0.0, 0.0, 0.0}, cb[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0}, wi = 0.0;
  bool act = false;
  [[maybe_unused]] const double* s_phi_of = nullptr;
  if constexpr (GRID) {
    __shared__ double s_e[DDP_HIP_MAX_CAPSULES][2][3];
    __shared__ double s_phi[DDP_HIP_MAX_CAPSULE_PAIRS * (DDP_HIP_CAPSULE_GRID_MAX_INTERVALS + 1)];
    if (tid < cp.nc) {
#pragma unroll
      for (int a = 0; a < 3; ++a) { s_e[tid][0][a] = e[0][a]; s_e[tid][1][a] = e[1][a]; }
    }
    __syncthreads();
    int i = 0;                                                       // the grid pair that holds item `it` (it only grows)
    for (int it = tid; it < cp.grid_items; it += (int)blockDim.x) {
      while (cp.kind[i] != DDP_HIP_CAPSULE_VS_GRID || it >= cp.gbase[i] + cp.nseg[cp.pa[i]] + 1) ++i;
      double phi = INFINITY;
      if (w[i] != 0.0) {
        double c[3], grad[3];
        capsule_grid_sample(cp.grid, s_e[cp.pa[i]][0], s_e[cp.pa[i]][1], cp.geom + (bt1 * cp.npair + i) * 8, cp.nseg[cp.pa[i]], it - cp.gbase[i], c, &phi, grad);
      }
      s_phi[it] = phi;
    }
    __syncthreads();
    s_phi_of = s_phi;
  }
  if (pair_lane) {
    wi = w[tid];
    if (wi != 0.0) {
      const double* g = cp.geom + (bt1 * cp.npair + tid) * 8;
      bool has_u;
      if (GRID && cp.kind[tid] == DDP_HIP_CAPSULE_VS_GRID) {
        const double* ph = s_phi_of + cp.gbase[tid];
        const int N = cp.nseg[ia];
        double best = ph[0], phi, grad[3] = {0.0, 0.0, 0.0};
        int bj = 0;
        for (int j = 1; j <= N; ++j)
          if (capsule_grid_better(ph[j], best, false)) { best = ph[j]; bj = j; }
        phi = best;
        if (best != INFINITY) capsule_grid_sample(cp.grid, a0, a1, g, N, bj, ca, &phi, grad);
        cb[0] = ca[0]; cb[1] = ca[1]; cb[2] = ca[2];
        has_u = capsule_grid_pair(phi, grad, cp.radius[ia], g[7], &d, u);
      } else {
        has_u = rbd::capsule_distance<false, BOX>(cp, tid, a0, a1, b0, b1, g, &d, ca, cb, u);
      }
      act = rbd::obstacle_active(d) && has_u;
    }
  }
  const unsigned active = (unsigned)__ballot(act);                  // bit i: pair i is active
  if (active == 0) return;
  __shared__ rbd::CapsuleWaveLds S;
  if (tid < m.nj) rbd::stage_joint_lane<0>(m, q, tid, S.jw, nullptr);
  if (act) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { S.ca[tid][a] = ca[a]; S.cb[tid][a] = cb[a]; S.u[tid][a] = u[a]; }
    S.w[tid] = wi;
    S.we[tid] = wi * d;
  }
  __syncthreads();
  unsigned long long U = 0;
  for (int i = 0; i < cp.npair; ++i)
    if ((active >> i) & 1) U |= rbd::capsule_masks_lane(cp, ff, i, S, i == tid);
  rbd::column_index_lane(U, tid, S.idx);
  __syncthreads();
  double *gx = blk.gx, *gxx = blk.gxx;
  rbd::capsule_add_wave(m, S, cp.npair, active, __builtin_popcountll(U), tid, (int)blockDim.x, n, gx, gxx);
}

template <int NJ>
__device__ __forceinline__ void load_xu(const LinParams& p, int b, int64_t t, double* x, double* u) {
  const int nx = (int)p.d.nx, m = (int)p.d.m;
  const double* xs = p.x + ((int64_t)b * (p.d.T + 1) + t) * nx;
  const double* us = p.u + ((int64_t)b * p.d.T + t) * m;
  for (int i = 0; i < nx; ++i) x[i] = xs[i];
  for (int i = 0; i < m; ++i) u[i] = us[i];
}

// f(x, u) at the base point (+ the analytic first order of the pendulum, problem.hpp:463-503 with
// pendulum_model.hpp:116-130)
template <int NJ>
__global__ void lin_base_kernel(LinParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t T = p.d.T;
  if (gid >= p.d.batch * T) return;
  const int b = (int)(gid / T);
  const int64_t t = gid % T;
  const DevModel& m = *p.model;
  const int nx = (int)p.d.nx;
  double x[2 * NJ + 1], u[NJ], f[2 * NJ + 1];
  load_xu<NJ>(p, b, t, x, u);
  rbd::eval_f<NJ>(m, x, u, f);
  for (int i = 0; i < nx; ++i) p.f_val[gid * nx + i] = f[i];
  if (!m.first_order_fd && m.kind == DDP_HIP_MODEL_PENDULUM) {
    double* fx = p.fx + gid * 4;
    double* fu = p.fu + gid * 2;
    const double aq = -9.81 / m.length * cos(x[0]);
    fx[0] = 1.0;
    fx[2] = 1.0 * m.dt;
    fx[1] = aq * m.dt;
    fx[3] = 0.0 * m.dt + 1.0;
    fu[0] = 0.0;
    fu[1] = (1.0 / m.mass) * m.dt;
  }
}

// forward-difference column j of [f_x | f_u]
template <int NJ>
__global__ void lin_first_kernel(LinParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t T = p.d.T;
  const int n = (int)p.d.n, mm = (int)p.d.m;
  const int W = n + mm;
  if (gid >= p.d.batch * T * W) return;
  const int j = (int)(gid % W);
  const int64_t bt = gid / W;
  const int b = (int)(bt / T);
  const int64_t t = bt % T;
  const DevModel& m = *p.model;
  double x[2 * NJ + 1], u[NJ], f[2 * NJ + 1];
  load_xu<NJ>(p, b, t, x, u);
  const double eps = sqrt(DBL_EPSILON);
  if (j < n) lie::perturb_x(m, x, j, eps); else u[j - n] = u[j - n] + eps;      // integrate_x / integrate_u (problem.hpp:107,117-118)
  rbd::eval_f<NJ>(m, x, u, f);
  const double* f0 = p.f_val + bt * p.d.nx;
  double* col = j < n ? p.fx + bt * n * n + (int64_t)j * n : p.fu + bt * n * mm + (int64_t)(j - n) * n;
  if (m.ff) {
    double df[2 * NJ];
    lie::difference_x(m, f0, f, df);                                             // difference_out on the group
    for (int k = 0; k < n; ++k) col[k] = df[k] / eps;
  } else {
    for (int k = 0; k < n; ++k) col[k] = (f[k] - f0[k]) / eps;
  }
}

// ---- second order, mode 2 (problem.hpp:152-298) --------------------------------------------------------
// q-dependent part of the ABA for the nv+1 configurations the mode-2 stencil visits more than once:
// cfg 0 = q, cfg 1+i = q + eps e_i (eps = eps_mach^(1/4), problem.hpp:188)
template <int NJ>
__global__ void lin_qcache_kernel(LinParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t T = p.d.T;
  const DevModel& m = *p.model;
  const int nv = m.nv, C = nv + 1;
  if (gid >= p.d.batch * T * C) return;
  const int cfg = (int)(gid % C);
  const int64_t bt = gid / C;
  const int b = (int)(bt / T);
  const int64_t t = bt % T;
  double x[2 * NJ], u[NJ];
  load_xu<NJ>(p, b, t, x, u);
  const double eps = sqrt(sqrt(DBL_EPSILON));
  if (cfg > 0) x[cfg - 1] = x[cfg - 1] + eps;
  rbd::aba_qpart<NJ>(m, x, p.qcache + (bt * C + cfg) * (int64_t)nv * rbd::QC_STRIDE);
}

// (q, v)-dependent part for the 2 nv + 1 (q, v) pairs shared by several stencil points:
// vcfg 0 = (q, v), 1+i = (q, v + eps e_i), nv+1+i = (q + eps e_i, v)
template <int NJ>
__global__ void lin_vcache_kernel(LinParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t T = p.d.T;
  const DevModel& m = *p.model;
  const int nv = m.nv, C = 2 * nv + 1;
  if (gid >= p.d.batch * T * C) return;
  const int vcfg = (int)(gid % C);
  const int64_t bt = gid / C;
  const int b = (int)(bt / T);
  const int64_t t = bt % T;
  double x[2 * NJ], u[NJ];
  load_xu<NJ>(p, b, t, x, u);
  const double eps = sqrt(sqrt(DBL_EPSILON));
  if (vcfg >= 1 && vcfg <= nv) x[nv + vcfg - 1] = x[nv + vcfg - 1] + eps;
  const int cfg = vcfg > nv ? vcfg - nv : 0;
  rbd::aba_vpart_cached<NJ>(m, p.qcache + (bt * (nv + 1) + cfg) * (int64_t)nv * rbd::QC_STRIDE, x + nv,
                            p.vcache + (bt * C + vcfg) * (int64_t)nv * rbd::VC_STRIDE);
}

// diagonal entries, :192-222
template <int NJ>
__global__ void lin_diag_kernel(LinParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t T = p.d.T;
  const int n = (int)p.d.n, mm = (int)p.d.m;
  const int W = n + mm;
  if (gid >= p.d.batch * T * W) return;
  const int i = (int)(gid % W);
  const int64_t bt = gid / W;
  const int b = (int)(bt / T);
  const int64_t t = bt % T;
  const DevModel& m = *p.model;
  double x[2 * NJ + 1], u[NJ], f1[2 * NJ + 1];
  load_xu<NJ>(p, b, t, x, u);
  const double eps = sqrt(sqrt(DBL_EPSILON));
  const double eps2 = eps * eps;
  const bool at_x = i < n;
  const int idx = at_x ? i : i - n;
  if (at_x) lie::perturb_x(m, x, idx, eps); else u[idx] = u[idx] + eps;
  // (ncfg == 1: the base point's caches alone, kept for the static first order under DDP_HIP_NO_QCACHE -- no block per stepped q)
  if (p.qcache && p.ncfg > 1) {
    const int nv = m.nv, cfg = (at_x && idx < nv) ? 1 + idx : 0;
    const double* qc = p.qcache + (bt * (nv + 1) + cfg) * (int64_t)nv * rbd::QC_STRIDE;
    if (!at_x) rbd::eval_f_ucached<NJ>(m, qc, p.vcache + (bt * (2 * nv + 1)) * (int64_t)nv * rbd::VC_STRIDE, x, u, f1);
    else rbd::eval_f_cached<NJ>(m, qc, x, u, f1);
  } else {
    rbd::eval_f<NJ>(m, x, u, f1);
  }
  const double* f0 = p.f_val + bt * p.d.nx;
  const double* fcol = at_x ? p.fx + bt * n * n + (int64_t)idx * n : p.fu + bt * n * mm + (int64_t)idx * n;
  double* tensor = at_x ? p.fxx + bt * n * n * n : p.fuu + bt * n * mm * mm;
  const int L = at_x ? n : mm;
  if (m.ff) {                       // difference_out on the group (problem.hpp:206), then the vector-space expression
    double dfv[2 * NJ];
    lie::difference_x(m, f0, f1, dfv);
    for (int k = 0; k < n; ++k) f1[k] = dfv[k];
  }
  for (int k = 0; k < n; ++k) {
    double df = m.ff ? f1[k] : f1[k] - f0[k];      // difference_out
    df -= eps * fcol[k];
    df *= 2;
    tensor[k + (int64_t)idx * n + (int64_t)idx * n * L] = df / eps2;
  }
}

// off-diagonal entries, :226-296: one lane per unordered pair i < j of the n+m directions.
// PAIRS = 0: every pair, full ABA (no caches).  PAIRS = 1: two q directions (both perturb the configuration: full
// ABA).  PAIRS = 2: (q or v, v): the q-dependent part comes from the q-cache.  PAIRS = 3: (q, v or u; u): only tau
// differs from a cached (q, v) pair, the evaluation is the force / acceleration passes alone.
template <int NJ, int PAIRS>
__global__ __launch_bounds__(LBS, (PAIRS == 1 || PAIRS == 0 ? 4 : 5)) void lin_offdiag_kernel(LinParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t T = p.d.T;
  const int n = (int)p.d.n, mm = (int)p.d.m;
  const int W = n + mm;
  const DevModel& m = *p.model;
  const int nv = m.nv;
  const int64_t TRI = (int64_t)nv * (nv - 1) / 2;
  const int64_t P = PAIRS == 0 ? (int64_t)W * (W - 1) / 2
                  : PAIRS == 1 ? TRI
                  : PAIRS == 2 ? (int64_t)nv * nv + TRI
                               : 2 * (int64_t)nv * nv + TRI;
  const bool valid = gid < p.d.batch * T * P;
  const int64_t pid = valid ? gid % P : 0;
  const int64_t bt = valid ? gid / P : 0;
  const int b = (int)(bt / T);
  const int64_t t = bt % T;
  auto tri = [](int64_t q, int Wd, int& ii, int& jj) {      // q -> (ii, jj), ii < jj < Wd, enumerated row by row
    int a = (int)floor(((2.0 * Wd - 1.0) - sqrt((2.0 * Wd - 1.0) * (2.0 * Wd - 1.0) - 8.0 * (double)q)) * 0.5);
    if (a < 0) a = 0;
    while ((int64_t)a * (2 * Wd - a - 1) / 2 > q) --a;
    while ((int64_t)(a + 1) * (2 * Wd - a - 2) / 2 <= q) ++a;
    ii = a;
    jj = (int)(q - (int64_t)a * (2 * Wd - a - 1) / 2) + a + 1;
  };
  int i, j;
  if (PAIRS == 0) tri(pid, W, i, j);
  else if (PAIRS == 1) tri(pid, nv, i, j);
  else if (PAIRS == 2) {
    if (pid < (int64_t)nv * nv) { i = (int)(pid / nv); j = nv + (int)(pid % nv); }                 // (q_i, v_j)
    else { tri(pid - (int64_t)nv * nv, nv, i, j); i += nv; j += nv; }                              // (v_i, v_j)
  } else {
    if (pid < 2 * (int64_t)nv * nv) { i = (int)(pid / nv); j = 2 * nv + (int)(pid % nv); }         // (q_i or v_i, u_j)
    else { tri(pid - 2 * (int64_t)nv * nv, nv, i, j); i += 2 * nv; j += 2 * nv; }                  // (u_i, u_j)
  }

  const double eps = sqrt(sqrt(DBL_EPSILON));
  const double eps2 = eps * eps;
  // PAIRS == 3 keeps no private copy of x, u or f(x+dx): the control is read through a functor and the output
  // rows are formed on the fly from the accelerations
  double f1[PAIRS == 3 ? 1 : 2 * NJ + 1], qdd[PAIRS == 3 ? NJ : 1];
  const double* xg = p.x + ((int64_t)b * (T + 1) + t) * p.d.nx;
  const double* ug = p.u + ((int64_t)b * T + t) * mm;
  if (valid) {
    if (PAIRS == 3) {
      const int cfg = i < nv ? 1 + i : 0;
      const int vcfg = i < nv ? nv + 1 + i : (i < 2 * nv ? 1 + (i - nv) : 0);
      const int iu = i - n, ju = j - n;
      rbd::aba_u_cached<NJ>(m, p.qcache + (bt * (nv + 1) + cfg) * (int64_t)nv * rbd::QC_STRIDE,
                            p.vcache + (bt * (2 * nv + 1) + vcfg) * (int64_t)nv * rbd::VC_STRIDE,
                            [&](int k) { double v = ug[k]; if (k == iu) v = v + eps; if (k == ju) v = v + eps; return v; }, qdd);
    } else {
      double x[2 * NJ + 1], u[NJ];
      load_xu<NJ>(p, b, t, x, u);
      // both directions in ONE step of the group (integrate_x of dx = eps e_i + eps e_j, problem.hpp:262-263): on a vector
      // space the two additions commute; on SE(3) the base twist eps (e_i + e_j) is integrated once
      if (PAIRS == 0 && m.ff && i < 6 && j < 6) {
        double nu[6] = {0, 0, 0, 0, 0, 0}, q7[7];
        nu[i] = eps; nu[j] = eps;
        lie::se3_integrate(x, nu, q7);
        for (int k = 0; k < 7; ++k) x[k] = q7[k];
      } else {
        if (i < n) lie::perturb_x(m, x, i, eps); else u[i - n] = u[i - n] + eps;
        if (j < n) lie::perturb_x(m, x, j, eps); else u[j - n] = u[j - n] + eps;
      }
      if (PAIRS == 2) {
        const int cfg = i < nv ? 1 + i : 0;
        rbd::eval_f_cached<NJ>(m, p.qcache + (bt * (nv + 1) + cfg) * (int64_t)nv * rbd::QC_STRIDE, x, u, f1);
      } else {
        rbd::eval_f<NJ>(m, x, u, f1);
        if (PAIRS == 0 && m.ff) {     // difference_out on the group (problem.hpp:268); the output stage then subtracts nothing
          double dfv[2 * NJ];
          lie::difference_x(m, p.f_val + bt * p.d.nx, f1, dfv);
          for (int k = 0; k < n; ++k) f1[k] = dfv[k];
        }
      }
    }
  }
  // row k of f(x + dx, u + du) (dynamics_t::eval_to, problem.hpp:441-461)
  auto f1_at = [&](int k) -> double {
    if (PAIRS != 3) return f1[k];
    if (k < nv) {
      const double xq = k == i ? xg[k] + eps : xg[k];
      const double xv = (nv + k) == i ? xg[nv + k] + eps : xg[nv + k];
      const double vo = m.dt * xv;
      return xq + vo;
    }
    const double xv = k == i ? xg[k] + eps : xg[k];
    return xv + qdd[k - nv] * m.dt;
  };

  // Output stage.  Each stencil point owns one 76-double column of a tensor (and reads five more columns);
  // done lane-per-point that is 64 scattered 8-byte accesses per instruction.  Instead the wave transposes the
  // f(x+dx) values through LDS, 16 rows at a time, and walks the points four at a time with 16 lanes on each
  // column: every access is four 128-byte runs.
  constexpr int CH = 16, EPI = LBS / CH;               // rows per chunk, points per instruction
  __shared__ double s_f[CH][LBS];
  __shared__ int s_i[LBS], s_j[LBS];
  __shared__ int64_t s_bt[LBS];
  const int lane = threadIdx.x;
  s_i[lane] = valid ? i : -1;
  s_j[lane] = j;
  s_bt[lane] = bt;
  const int kk = lane % CH, esub = lane / CH;
  for (int c0 = 0; c0 < n; c0 += CH) {
#pragma unroll
    for (int q = 0; q < CH; ++q)
      if (c0 + q < n && valid) s_f[q][lane] = f1_at(c0 + q);
    __syncthreads();
    const int k = c0 + kk;
    for (int r = 0; r < LBS / EPI; ++r) {
      const int e = r * EPI + esub;
      const int ie = s_i[e];
      if (ie < 0 || k >= n) continue;
      const int je = s_j[e];
      const int64_t bte = s_bt[e];
      const bool at_x_1 = ie < n, at_x_2 = je < n;
      const int idx_1 = at_x_1 ? ie : ie - n, idx_2 = at_x_2 ? je : je - n;
      const double* f0 = p.f_val + bte * p.d.nx;
      double* fxx = p.fxx + bte * n * n * n;
      double* fux = p.fux + bte * n * mm * n;
      double* fuu = p.fuu + bte * n * mm * mm;
      const double* fcol_1 = at_x_1 ? p.fx + bte * n * n + (int64_t)idx_1 * n : p.fu + bte * n * mm + (int64_t)idx_1 * n;
      const double* fcol_2 = at_x_2 ? p.fx + bte * n * n + (int64_t)idx_2 * n : p.fu + bte * n * mm + (int64_t)idx_2 * n;
      const double* tensor_1 = at_x_1 ? fxx : fuu;
      const double* tensor_2 = at_x_2 ? fxx : fuu;
      const int L1 = at_x_1 ? n : mm, L2 = at_x_2 ? n : mm;
      double* tensor;
      int L;
      if (at_x_1) { if (at_x_2) { tensor = fxx; L = n; } else { tensor = fux; L = mm; } }
      else { tensor = fuu; L = mm; }
      double df = (PAIRS == 0 && m.ff) ? s_f[kk][e] : s_f[kk][e] - f0[k];   // difference_out
      df -= eps * fcol_1[k];
      df -= eps * fcol_2[k];
      df *= 2;
      const double val = 0.5 * (df / eps2 - tensor_1[k + (int64_t)idx_1 * n + (int64_t)idx_1 * n * L1] -
                                tensor_2[k + (int64_t)idx_2 * n + (int64_t)idx_2 * n * L2]);
      tensor[k + (int64_t)idx_2 * n + (int64_t)idx_1 * n * L] = val;
      if (at_x_1 == at_x_2) tensor[k + (int64_t)idx_1 * n + (int64_t)idx_2 * n * L] = val;
    }
    __syncthreads();
  }
}

// ---- small-model paths (nv <= 6): first order as a device function, used by the constraint chain and mode 1
template <int NJ>
__device__ void first_order_f(const DevModel& m, const double* x, const double* u, double* fx, double* fu, double* f) {
  const int nv = m.nv, n = 2 * nv, mm = nv;
  if (!m.first_order_fd && m.kind == DDP_HIP_MODEL_TREE) {
    // analytic, as the reference: d_dynamics_aba (problem.hpp:495)
    if constexpr (NJ <= 6) rbdd::first_order_analytic_lane<NJ>(m, x, u, fx, fu, f);
    return;
  }
  rbd::eval_f<NJ>(m, x, u, f);
  if (!m.first_order_fd) {
    const double aq = -9.81 / m.length * cos(x[0]);
    fx[0] = 1.0; fx[2] = 1.0 * m.dt; fx[1] = aq * m.dt; fx[3] = 0.0 * m.dt + 1.0;
    fu[0] = 0.0; fu[1] = (1.0 / m.mass) * m.dt;
    return;
  }
  const double eps = sqrt(DBL_EPSILON);
  double xp[2 * NJ], up[NJ], fp[2 * NJ];
  for (int j = 0; j < n + mm; ++j) {
    for (int k = 0; k < n; ++k) xp[k] = x[k];
    for (int k = 0; k < mm; ++k) up[k] = u[k];
    if (j < n) xp[j] = x[j] + eps; else up[j - n] = u[j - n] + eps;
    rbd::eval_f<NJ>(m, xp, up, fp);
    double* col = j < n ? fx + j * n : fu + (j - n) * n;
    for (int k = 0; k < n; ++k) col[k] = (fp[k] - f[k]) / eps;
  }
}

// analytic first order of a small tree model (nv <= 6), one lane per (instance, t)
template <int NJ>
__global__ void lin_first_analytic_small_kernel(LinParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t T = p.d.T;
  if (gid >= p.d.batch * T) return;
  const int b = (int)(gid / T);
  const int64_t t = gid % T;
  const DevModel& m = *p.model;
  const int n = 2 * m.nv, mm = m.nv;
  double x[2 * NJ], u[NJ], f[2 * NJ];
  load_xu<NJ>(p, b, t, x, u);
  first_order_f<NJ>(m, x, u, p.fx + gid * n * n, p.fu + gid * n * mm, f);     // f_val itself is lin_base_kernel's (same arithmetic)
}

// constraint value through the advance chain (problem.hpp:563-567)
template <int NJ>
__device__ void eq_eval(const DevModel& m, const double* target, int e, const double* x, const double* u, double* out) {
  const int nx = m.nq + m.nv;
  double xa[2 * NJ + 1], xb[2 * NJ + 1];
  for (int i = 0; i < nx; ++i) xa[i] = x[i];
  for (int k = 0; k < m.eq_advance; ++k) {
    if (k + 1 < m.eq_advance) rbd::eval_f<NJ>(m, xa, u, xb);
    else { for (int i = m.nq; i < nx; ++i) xb[i] = xa[i]; rbd::eval_f_q<NJ>(m, xa, xb); }   // the constraint reads q only: no dynamics in the last step
    for (int i = 0; i < nx; ++i) xa[i] = xb[i];
  }
  if (m.eq_kind == DDP_HIP_EQ_CONFIG) {
    for (int i = 0; i < e; ++i) out[i] = xa[i] - target[i];
  } else {
    double pos[3];
    rbd::frame_position<NJ>(m, xa, pos, nullptr);
    for (int i = 0; i < e; ++i) out[i] = pos[i] - target[i];
  }
}

// constraint first order through the advance chain: constraint_advance_time_t::first_order_deriv,
// problem.hpp:569-605 (out_x = eq_n_x * fx_n, out_u = eq_n_x * fu_n; the inner eq_n_u is dropped as the
// reference asserts it to be zero), around config_constraint_t :808-845 / spatial_constraint_t :691-722
template <int NJ, int ADV>
__device__ void eq_first_order(const DevModel& m, const double* target, int e, const double* x, const double* u,
                               double* out_x, double* out_u, double* out) {
  constexpr int N = 2 * NJ, M = NJ, EM = NJ > 3 ? NJ : 3;
  const int nv = m.nv, n = 2 * nv, mm = nv;
  double Fx[ADV > 0 ? ADV : 1][N * N], Fu[ADV > 0 ? ADV : 1][N * M];
  double xa[N], xb[N];
  for (int i = 0; i < n; ++i) xa[i] = x[i];
  const int adv = m.eq_advance;
  for (int k = 0; k < adv; ++k) {
    first_order_f<NJ>(m, xa, u, Fx[k], Fu[k], xb);
    for (int i = 0; i < n; ++i) xa[i] = xb[i];
  }
  double ex[EM * N], tmp[EM * N];
  for (int i = 0; i < e * n; ++i) ex[i] = 0.0;
  if (m.eq_kind == DDP_HIP_EQ_CONFIG) {
    for (int i = 0; i < e; ++i) { out[i] = xa[i] - target[i]; ex[i + i * e] = 1.0; }   // d_difference_dq_finish = I
  } else {
    double pos[3], J[3 * NJ];
    rbd::frame_position<NJ>(m, xa, pos, J);
    for (int i = 0; i < e; ++i) out[i] = pos[i] - target[i];
    for (int j = 0; j < nv; ++j)
      for (int i = 0; i < e; ++i) ex[i + j * e] = J[i + 3 * j];
  }
  for (int i = 0; i < e * mm; ++i) out_u[i] = 0.0;
  for (int k = adv - 1; k >= 0; --k) {
    for (int j = 0; j < mm; ++j)
      for (int i = 0; i < e; ++i) {
        double s = 0;
        for (int l = 0; l < n; ++l) s += ex[i + l * e] * Fu[k][l + j * n];
        out_u[i + j * e] = s;
      }
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < e; ++i) {
        double s = 0;
        for (int l = 0; l < n; ++l) s += ex[i + l * e] * Fx[k][l + j * n];
        tmp[i + j * e] = s;
      }
    for (int i = 0; i < e * n; ++i) ex[i] = tmp[i];
  }
  for (int i = 0; i < e * n; ++i) out_x[i] = ex[i];
}

// ---- constraint chain, large models: the same chain rule as eq_first_order, as three kernels ---------------------
// (the per-lane variant above would need n x n private matrices per lane)
template <int NJ>
__global__ void eq_chain_kernel(LinParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t T = p.d.T;
  if (gid >= p.d.batch * T) return;
  const int b = (int)(gid / T);
  const int64_t t = gid % T;
  const int e = (int)p.ne[t];
  if (e == 0) return;
  const DevModel& m = *p.model;
  const int nv = m.nv, n = 2 * nv, K = m.eq_advance, nx = (int)p.d.nx;
  const int64_t Eo = p.Epre[t], Eb = (int64_t)b * p.d.Etot + Eo;
  double xa[2 * NJ + 1], xb[2 * NJ + 1], u[NJ];
  load_xu<NJ>(p, b, t, xa, u);
  for (int k = 0; k < K; ++k) {                          // x_{k+1} = f(x_k, u): the SAME u at every look-ahead step
    if (k + 1 < K || m.ff) rbd::eval_f<NJ>(m, xa, u, xb);   // (free flyer: eq_fdjac differences whole states on the group)
    else { for (int i = m.nq; i < nx; ++i) xb[i] = xa[i]; rbd::eval_f_q<NJ>(m, xa, xb); }   // x_K: only its configuration is read (the constraint, and eq_fdjac's
    for (int i = 0; i < nx; ++i) { xa[i] = xb[i]; p.eq_xk[(gid * K + k) * nx + i] = xb[i]; }  // q rows below) -- its velocity half is a placeholder
  }
  double* C = p.eq_c + gid * (int64_t)p.d.emax * n;
  for (int i = 0; i < e * n; ++i) C[i] = 0.0;
  const double* target = p.target + Eo;
  if (m.eq_kind == DDP_HIP_EQ_CONFIG) {
    for (int i = 0; i < e; ++i) { p.eq_val[Eb + i] = xa[i] - target[i]; C[i + i * e] = 1.0; }   // d_difference_dq_finish = I
  } else {
    double pos[3], J[3 * NJ];
    rbd::frame_position<NJ>(m, xa, pos, J);
    for (int i = 0; i < e; ++i) p.eq_val[Eb + i] = pos[i] - target[i];
    for (int j = 0; j < nv; ++j)
      for (int i = 0; i < e; ++i) C[i + j * e] = J[i + 3 * j];
  }
}

// forward-difference f_x at the look-ahead states x_1 .. x_{K-1}: one lane per (b, t, k, column)
template <int NJ>
__global__ void eq_fdjac_kernel(LinParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t T = p.d.T;
  const DevModel& m = *p.model;
  const int n = 2 * m.nv, K = m.eq_advance;
  if (K < 2 || gid >= p.d.batch * T * (K - 1) * n) return;
  const int j = (int)(gid % n);
  const int k = (int)((gid / n) % (K - 1));               // Jacobian at x_{k+1}
  const int64_t bt = gid / ((int64_t)n * (K - 1));
  const int b = (int)(bt / T);
  const int64_t t = bt % T;
  if (p.ne[t] == 0) return;
  double x[2 * NJ + 1], u[NJ], f[2 * NJ + 1];
  const int nx = (int)p.d.nx;
  const double* xk = p.eq_xk + (bt * K + k) * nx;          // x_{k+1}
  const double* xk1 = p.eq_xk + (bt * K + k + 1) * nx;     // x_{k+2} = f(x_{k+1}, u)
  const double* us = p.u + ((int64_t)b * T + t) * m.nv;
  for (int i = 0; i < nx; ++i) x[i] = xk[i];
  for (int i = 0; i < m.nv; ++i) u[i] = us[i];
  const double eps = sqrt(DBL_EPSILON);
  lie::perturb_x(m, x, j, eps);
  double* col = p.eq_fxk + (bt * (K - 1) + k) * (int64_t)n * n + (int64_t)j * n;
  if (k == K - 2 && !m.ff) {
    // f_x(x_{K-1}) is multiplied from the left by the base jacobian C = [C_q | 0] (both constraint kinds read q only) and by
    // nothing else: only its q rows matter, and those difference q+ = q + dt v -- no dynamics.  The very same values as the
    // full column's q rows (the v rows, multiplied by exact zeros in eq_combine, are written as zeros): 76 forward-dynamics
    // evaluations per constrained (instance, t) less.
    const int nv = m.nv;
    for (int i = 0; i < nv; ++i) { const double vo = m.dt * x[nv + i]; const double fq = x[i] + vo; col[i] = (fq - xk1[i]) / eps; }
    for (int i = nv; i < n; ++i) col[i] = 0.0;
    return;
  }
  rbd::eval_f<NJ>(m, x, u, f);
  if (m.ff) {
    double df[2 * NJ];
    lie::difference_x(m, xk1, f, df);
    for (int i = 0; i < n; ++i) col[i] = df[i] / eps;
  } else {
    for (int i = 0; i < n; ++i) col[i] = (f[i] - xk1[i]) / eps;
  }
}

// eq_x = C f_x(x_{K-1}) ... f_x(x_1) f_x(x_0),  eq_u = C f_x(x_{K-1}) ... f_x(x_1) f_u(x_0)   (problem.hpp:603-604)
__global__ void eq_combine_kernel(LinParams p) {
  const int64_t bt = blockIdx.x;
  const int64_t T = p.d.T;
  const int b = (int)(bt / T);
  const int64_t t = bt % T;
  const int e = (int)p.ne[t];
  if (e == 0) return;
  const int n = (int)p.d.n, mm = (int)p.d.m, K = p.model->eq_advance;
  const int64_t Eb = (int64_t)b * p.d.Etot + p.Epre[t];
  extern __shared__ double sm[];
  double* ex = sm;
  double* tmp = sm + (int64_t)p.d.emax * n;
  const double* C = p.eq_c + bt * (int64_t)p.d.emax * n;
  for (int i = threadIdx.x; i < e * n; i += blockDim.x) ex[i] = C[i];
  __syncthreads();
  for (int k = K - 2; k >= 0; --k) {
    const double* F = p.eq_fxk + (bt * (K - 1) + k) * (int64_t)n * n;
    for (int idx = threadIdx.x; idx < e * n; idx += blockDim.x) {
      const int i = idx % e, j = idx / e;
      double s = 0;
      for (int l = 0; l < n; ++l) s += ex[i + l * e] * F[l + (int64_t)j * n];
      tmp[idx] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < e * n; i += blockDim.x) ex[i] = tmp[i];
    __syncthreads();
  }
  const double* fx = p.fx + bt * n * n;
  const double* fu = p.fu + bt * n * mm;
  for (int idx = threadIdx.x; idx < e * n; idx += blockDim.x) {
    const int i = idx % e, j = idx / e;
    double s = 0;
    for (int l = 0; l < n; ++l) s += ex[i + l * e] * fx[l + j * n];
    p.eq_x[Eb * n + idx] = s;
  }
  for (int idx = threadIdx.x; idx < e * mm; idx += blockDim.x) {
    const int i = idx % e, j = idx / e;
    double s = 0;
    for (int l = 0; l < n; ++l) s += ex[i + l * e] * fu[l + j * n];
    p.eq_u[Eb * mm + idx] = s;
  }
}

#define MAXADV 4

template <int NJ>
__global__ void eq_first_kernel(LinParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t T = p.d.T;
  if (gid >= p.d.batch * T) return;
  const int b = (int)(gid / T);
  const int64_t t = gid % T;
  const int e = (int)p.ne[t];
  if (e == 0) return;
  const DevModel& m = *p.model;
  const int n = (int)p.d.n, mm = (int)p.d.m;
  const int64_t Eo = p.Epre[t], Eb = (int64_t)b * p.d.Etot + Eo;
  double x[2 * NJ], u[NJ];
  load_xu<NJ>(p, b, t, x, u);
  eq_first_order<NJ, MAXADV>(m, p.target + Eo, e, x, u, p.eq_x + Eb * n, p.eq_u + Eb * mm, p.eq_val + Eb);
}

// mode 1 (problem.hpp:67-150) for the dynamics (analytic first order only) and for the constraint chain
template <int NJ>
__global__ void second_m1_kernel(LinParams p, int is_eq) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t T = p.d.T;
  const int n = (int)p.d.n, mm = (int)p.d.m;
  const int W = n + mm;
  if (gid >= p.d.batch * T * W) return;
  const int i = (int)(gid % W);
  const int64_t bt = gid / W;
  const int b = (int)(bt / T);
  const int64_t t = bt % T;
  const DevModel& m = *p.model;
  constexpr int N = 2 * NJ, M = NJ, EM = NJ > 3 ? NJ : 3;
  double x[N], u[M];
  load_xu<NJ>(p, b, t, x, u);
  const double eps = sqrt(DBL_EPSILON);
  const bool at_x = i < n;
  const int idx = at_x ? i : i - n;
  if (at_x) x[idx] = x[idx] + eps; else u[idx] = u[idx] + eps;
  if (!is_eq) {
    double fx_[N * N], fu_[N * M], out_[N];
    first_order_f<NJ>(m, x, u, fx_, fu_, out_);
    const double* ox = p.fx + bt * n * n;
    const double* ou = p.fu + bt * n * mm;
    const int o = n;
    if (at_x) {
      for (int k = 0; k < o; ++k) {
        for (int j = 0; j < n; ++j) p.fxx[bt * n * n * n + k + (int64_t)j * o + (int64_t)idx * o * n] = (fx_[k + j * o] - ox[k + j * o]) / eps;
        for (int j = 0; j < mm; ++j) p.fux[bt * n * mm * n + k + (int64_t)j * o + (int64_t)idx * o * mm] = (fu_[k + j * o] - ou[k + j * o]) / eps;
      }
    } else {
      for (int k = 0; k < o; ++k)
        for (int j = 0; j < mm; ++j) p.fuu[bt * n * mm * mm + k + (int64_t)j * o + (int64_t)idx * o * mm] = (fu_[k + j * o] - ou[k + j * o]) / eps;
    }
  } else {
    const int e = (int)p.ne[t];
    if (e == 0) return;
    const int64_t Eo = p.Epre[t], Eb = (int64_t)b * p.d.Etot + Eo;
    double ex_[EM * N], eu_[EM * M], out_[EM];
    eq_first_order<NJ, MAXADV>(m, p.target + Eo, e, x, u, ex_, eu_, out_);
    const double* ox = p.eq_x + Eb * n;
    const double* ou = p.eq_u + Eb * mm;
    const int o = e;
    if (at_x) {
      for (int k = 0; k < o; ++k) {
        for (int j = 0; j < n; ++j) p.eq_xx[Eb * n * n + k + (int64_t)j * o + (int64_t)idx * o * n] = (ex_[k + j * o] - ox[k + j * o]) / eps;
        for (int j = 0; j < mm; ++j) p.eq_ux[Eb * mm * n + k + (int64_t)j * o + (int64_t)idx * o * mm] = (eu_[k + j * o] - ou[k + j * o]) / eps;
      }
    } else {
      for (int k = 0; k < o; ++k)
        for (int j = 0; j < mm; ++j) p.eq_uu[Eb * mm * mm + k + (int64_t)j * o + (int64_t)idx * o * mm] = (eu_[k + j * o] - ou[k + j * o]) / eps;
    }
  }
}

// mode 2 for the constraint chain: stage 0 = diagonal, stage 1 = off-diagonal
template <int NJ>
__global__ void eq_second_m2_kernel(LinParams p, int stage) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t T = p.d.T;
  const int n = (int)p.d.n, mm = (int)p.d.m;
  const int W = n + mm;
  const int64_t P = stage == 0 ? W : (int64_t)W * (W - 1) / 2;
  if (gid >= p.d.batch * T * P) return;
  const int64_t pid = gid % P;
  const int64_t bt = gid / P;
  const int b = (int)(bt / T);
  const int64_t t = bt % T;
  const int e = (int)p.ne[t];
  if (e == 0) return;
  int i, j;
  if (stage == 0) { i = (int)pid; j = -1; }
  else {
    i = (int)floor(((2.0 * W - 1.0) - sqrt((2.0 * W - 1.0) * (2.0 * W - 1.0) - 8.0 * (double)pid)) * 0.5);
    if (i < 0) i = 0;
    while ((int64_t)i * (2 * W - i - 1) / 2 > pid) --i;
    while ((int64_t)(i + 1) * (2 * W - i - 2) / 2 <= pid) ++i;
    j = (int)(pid - (int64_t)i * (2 * W - i - 1) / 2) + i + 1;
  }
  const DevModel& m = *p.model;
  constexpr int EM = NJ > 3 ? NJ : 3;
  double x[2 * NJ + 1], u[NJ], f1[EM];
  load_xu<NJ>(p, b, t, x, u);
  const double eps = sqrt(sqrt(DBL_EPSILON));
  const double eps2 = eps * eps;
  const int64_t Eo = p.Epre[t], Eb = (int64_t)b * p.d.Etot + Eo;
  const double* f0 = p.eq_val + Eb;
  double* exx = p.eq_xx + Eb * n * n;
  double* eux = p.eq_ux + Eb * mm * n;
  double* euu = p.eq_uu + Eb * mm * mm;
  const bool at_x_1 = i < n;
  const int idx_1 = at_x_1 ? i : i - n;
  const bool both_base = stage != 0 && m.ff && i < 6 && j < 6;     // one step of the group for a pair of base directions
  if (both_base) {
    double nu[6] = {0, 0, 0, 0, 0, 0}, q7[7];
    nu[i] = eps; nu[j] = eps;
    lie::se3_integrate(x, nu, q7);
    for (int k = 0; k < 7; ++k) x[k] = q7[k];
  } else if (at_x_1) lie::perturb_x(m, x, idx_1, eps); else u[idx_1] = u[idx_1] + eps;
  const double* fcol_1 = at_x_1 ? p.eq_x + Eb * n + (int64_t)idx_1 * e : p.eq_u + Eb * mm + (int64_t)idx_1 * e;
  const int L1 = at_x_1 ? n : mm;
  double* tensor_1 = at_x_1 ? exx : euu;
  if (stage == 0) {
    eq_eval<NJ>(m, p.target + Eo, e, x, u, f1);
    for (int k = 0; k < e; ++k) {
      double df = f1[k] - f0[k];
      df -= eps * fcol_1[k];
      df *= 2;
      tensor_1[k + (int64_t)idx_1 * e + (int64_t)idx_1 * e * L1] = df / eps2;
    }
    return;
  }
  const bool at_x_2 = j < n;
  const int idx_2 = at_x_2 ? j : j - n;
  if (both_base) {} else if (at_x_2) lie::perturb_x(m, x, idx_2, eps); else u[idx_2] = u[idx_2] + eps;
  const double* fcol_2 = at_x_2 ? p.eq_x + Eb * n + (int64_t)idx_2 * e : p.eq_u + Eb * mm + (int64_t)idx_2 * e;
  const int L2 = at_x_2 ? n : mm;
  const double* tensor_2 = at_x_2 ? exx : euu;
  double* tensor;
  int L;
  if (at_x_1) { if (at_x_2) { tensor = exx; L = n; } else { tensor = eux; L = mm; } }
  else { tensor = euu; L = mm; }
  eq_eval<NJ>(m, p.target + Eo, e, x, u, f1);
  for (int k = 0; k < e; ++k) {
    double df = f1[k] - f0[k];
    df -= eps * fcol_1[k];
    df -= eps * fcol_2[k];
    df *= 2;
    const double val = 0.5 * (df / eps2 - tensor_1[k + (int64_t)idx_1 * e + (int64_t)idx_1 * e * L1] -
                              tensor_2[k + (int64_t)idx_2 * e + (int64_t)idx_2 * e * L2]);
    tensor[k + (int64_t)idx_2 * e + (int64_t)idx_1 * e * L] = val;
    if (at_x_1 == at_x_2) tensor[k + (int64_t)idx_1 * e + (int64_t)idx_2 * e * L] = val;
  }
}

// T(:, i, j) = T(:, j, i) for i < j: the mirror images of a symmetric tensor's entries (f_xx: L = n; f_uu: L = m), which the
// static stencil leaves out while the backward sweep is known not to read them (LinParams::skip_qv_mirror); formed when
// somebody else asks for FXX / FUU
__global__ void tensor_mirror_kernel(double* Tn, int64_t BT, int n, int L) {
  const int64_t per = (int64_t)n * L * L, total = BT * per;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t bt = g / per, r = g % per;
    const int k = (int)(r % n), j = (int)((r / n) % L), c = (int)(r / ((int64_t)n * L));   // entry (k, j, c): column j of slab c
    if (j >= c) continue;
    double* T = Tn + bt * per;
    T[k + (int64_t)j * n + (int64_t)c * n * L] = T[k + (int64_t)c * n + (int64_t)j * n * L];   // its direct twin: column c of slab j
  }
}

// rows k < nv of every column of a tensor (O = n rows, `cols` columns per (instance, t)) to zero: what the static stencil
// relies on when it skips them (LinParams::skip_top)
__global__ void tensor_zero_top_kernel(double* Tn, int64_t total_cols, int n, int nv) {
  const int64_t total = total_cols * nv;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t col = g / nv;
    Tn[col * n + (g % nv)] = 0.0;
  }
}

// Packed records (LinParams::pack) back into the contract layout, in place: one workgroup per slab (grid: the n slabs of f_xx, the
// n of f_ux, the m of f_uu of every (instance, t)).  The packed image (L (nv + 2) doubles at the front of the slab) overlaps the
// contract image it becomes, so the whole of it goes through LDS before the first store.  Upper halves: +0.0 but the tops; f_uu
// has none.  Columns the symmetric stencil never wrote (j < slab) carry over whatever their records held: tensor_mirror_kernel
// overwrites all of them next.
constexpr int UNPACK_BS = 256;
__global__ __launch_bounds__(UNPACK_BS) void tensor_unpack_kernel(double* fxx, double* fux, double* fuu, int n, int m, int nv) {
  extern __shared__ __attribute__((aligned(16))) double s_rec[];   // n (nv + 2)
  const int per = 2 * n + m;
  const int64_t bt = blockIdx.x / per;
  const int s = (int)(blockIdx.x % per);
  double* slab;
  int L, c;
  bool tops;
  if (s < n) { c = s; L = n; tops = true; slab = fxx + (bt * n + c) * (int64_t)n * n; }
  else if (s < 2 * n) { c = s - n; L = m; tops = true; slab = fux + (bt * n + c) * (int64_t)n * m; }
  else { c = s - 2 * n; L = m; tops = false; slab = fuu + (bt * m + c) * (int64_t)n * m; }
  const int R = nv + 2, words = L * R;
  for (int e = threadIdx.x; e < words; e += UNPACK_BS) s_rec[e] = slab[e];
  __syncthreads();
  const int r0 = c % nv;
  for (int e = threadIdx.x; e < L * n; e += UNPACK_BS) {
    const int j = e / n, k = e - j * n;
    const double* rec = s_rec + j * R;
    double v = 0.0;
    if (k >= nv) v = rec[2 + (k - nv)];
    else if (tops && k == r0) v = rec[0];
    else if (tops && L == n && k == j % nv) v = rec[1];
    slab[e] = v;
  }
}

// doubles per (instance, t) of the q-cache: ncfg whole blocks, or the static stencil's base block + deltas
int64_t lin_qc_per_bt(const ddp_hip_ctx* ctx) {
  const LinPlan& pl = ctx->plan;
  return pl.qc_sparse ? lin_static_qc_per_bt(pl.topo) : (int64_t)pl.ncfg * ctx->d.nv * rbd::QC_STRIDE;
}

// ... of the v-cache: nvcfg whole entries, or the static stencil's base blocks + deltas
int64_t lin_vc_per_bt(const ddp_hip_ctx* ctx) {
  const LinPlan& pl = ctx->plan;
  return pl.vc_sparse ? lin_static_vc_per_bt(pl.topo) : (int64_t)pl.nvcfg * ctx->d.nv * rbd::VC_STRIDE;
}

LinParams make_params(ddp_hip_ctx* ctx) {
  LinParams p{};
  p.d = ctx->d;
  p.model = ctx->model_d;
  p.ne = ctx->ne_d;
  p.Epre = ctx->Epre_d;
  p.target = ctx->target_d;
  auto S = [&](int s) { return ctx->seq[s].ptr; };
  p.x = S(DDP_HIP_SEQ_X); p.u = S(DDP_HIP_SEQ_U);
  p.lfx = S(DDP_HIP_SEQ_LFX); p.lfxx = S(DDP_HIP_SEQ_LFXX);
  p.lx = S(DDP_HIP_SEQ_LX); p.lu = S(DDP_HIP_SEQ_LU); p.lxx = S(DDP_HIP_SEQ_LXX); p.lux = S(DDP_HIP_SEQ_LUX); p.luu = S(DDP_HIP_SEQ_LUU);
  p.f_val = S(DDP_HIP_SEQ_F_VAL); p.fx = S(DDP_HIP_SEQ_FX); p.fu = S(DDP_HIP_SEQ_FU);
  p.fxx = S(DDP_HIP_SEQ_FXX); p.fux = S(DDP_HIP_SEQ_FUX); p.fuu = S(DDP_HIP_SEQ_FUU);
  p.eq_val = S(DDP_HIP_SEQ_EQ_VAL); p.eq_x = S(DDP_HIP_SEQ_EQ_X); p.eq_u = S(DDP_HIP_SEQ_EQ_U);
  p.eq_xx = S(DDP_HIP_SEQ_EQ_XX); p.eq_ux = S(DDP_HIP_SEQ_EQ_UX); p.eq_uu = S(DDP_HIP_SEQ_EQ_UU);
  const LinPlan& pl = ctx->plan;
  p.has_tensors = pl.has_tensors ? 1 : 0;
  p.skip_top = pl.skip_top ? 1 : 0;
  p.skip_qv_mirror = pl.skip_qv_mirror ? 1 : 0;
  p.pack = pl.pack ? 1 : 0;
  p.eq_xk = ctx->eq_ws;
  if (p.eq_xk) { p.eq_fxk = p.eq_xk + pl.eq_fxk_off; p.eq_c = p.eq_xk + pl.eq_c_off; }
  p.qcache = ctx->lin_ws;
  p.ncfg = pl.ncfg; p.nvcfg = pl.nvcfg;
  p.qc_sparse = pl.qc_sparse ? 1 : 0;
  p.qc_bt = lin_qc_per_bt(ctx);
  p.vcache = p.qcache ? p.qcache + ctx->d.batch * ctx->d.T * p.qc_bt : nullptr;
  p.vc_sparse = pl.vc_sparse ? 1 : 0;
  p.vc_bt = lin_vc_per_bt(ctx);
  p.xref = S(DDP_HIP_SEQ_COST_XREF); p.wx = S(DDP_HIP_SEQ_COST_WX); p.uref = S(DDP_HIP_SEQ_COST_UREF); p.wu = S(DDP_HIP_SEQ_COST_WU);
  return p;
}

inline unsigned blocks_for(int64_t total) { return (unsigned)((total + LBS - 1) / LBS); }

// the constraint tensors eq_xx, eq_ux, eq_uu, in the form the plan names
template <int NJ>
int eq_second_order(ddp_hip_ctx* ctx, const LinParams& p, LinCall& call, uint32_t stages) {
  const Dims& d = ctx->d;
  const int64_t BT = d.batch * d.T;
  const int W = (int)(d.n + d.m);
  const int64_t P = (int64_t)W * (W - 1) / 2;
  switch (ctx->plan.eq_second) {
    case LinEqSecond::None: break;
    case LinEqSecond::Mode2:
      hipLaunchKernelGGL((eq_second_m2_kernel<NJ>), dim3(blocks_for(BT * W)), dim3(LBS), 0, ctx->stream, p, 0);
      hipLaunchKernelGGL((eq_second_m2_kernel<NJ>), dim3(blocks_for(BT * P)), dim3(LBS), 0, ctx->stream, p, 1);
      break;
    case LinEqSecond::Mode1Small:
      if constexpr (NJ <= 6) hipLaunchKernelGGL((second_m1_kernel<NJ>), dim3(blocks_for(BT * W)), dim3(LBS), 0, ctx->stream, p, 1);
      break;
    case LinEqSecond::Mode1Wave: {
      // (with LIN_SECOND among the stages this is the dynamics' own mode-1 pass as well: LinPlan::m1_fused)
      const int fl = LIN_ANA_EQ | ((stages & DDP_HIP_LIN_SECOND) ? LIN_ANA_F : 0);
      if (fl & LIN_ANA_F) prof_begin(ctx, DDP_HIP_K_LIN_SECOND);
      const int rc_ = lin_analytic_launch(ctx, p, call, 1, fl);
      if (fl & LIN_ANA_F) prof_end(ctx, DDP_HIP_K_LIN_SECOND);
      if (rc_ != DDP_HIP_OK) return rc_;
      break;
    }
    case LinEqSecond::Zeros:
      HIP_TRY(hipMemsetAsync(p.eq_xx, 0, sizeof(double) * (size_t)(ctx->seq[DDP_HIP_SEQ_EQ_XX].size * d.batch), ctx->stream));
      HIP_TRY(hipMemsetAsync(p.eq_ux, 0, sizeof(double) * (size_t)(ctx->seq[DDP_HIP_SEQ_EQ_UX].size * d.batch), ctx->stream));
      HIP_TRY(hipMemsetAsync(p.eq_uu, 0, sizeof(double) * (size_t)(ctx->seq[DDP_HIP_SEQ_EQ_UU].size * d.batch), ctx->stream));
      break;
  }
  return DDP_HIP_OK;
}

// One linearisation: the stages asked for, each on the leg ctx->plan names (the legs that need the one-lane kernels of small
// models are instantiated for NJ <= 6 only; the plan selects them for no other NJ)
template <int NJ>
int run_linearize(ddp_hip_ctx* ctx, const LinParams& p, LinCall& call, uint32_t stages) {
  const LinPlan& pl = ctx->plan;
  const Dims& d = ctx->d;
  const int64_t BT = d.batch * d.T;
  const int W = (int)(d.n + d.m);
  const int nv = (int)d.nv;
  [[maybe_unused]] constexpr bool small = NJ <= 6;
  const bool second_stage = (stages & DDP_HIP_LIN_SECOND) && pl.second != LinSecond::None;
  const bool eq_stage = (stages & DDP_HIP_LIN_EQ) && pl.eq != LinEq::None;
  const bool m1_fused = pl.m1_fused && eq_stage;   // LIN_SECOND's mode-1 pass is issued by the LIN_EQ stage
  // both orders of the static stencil in one call: the first order's u waves go on to the u diagonal of f_uu (lin_static.hip:
  // lin_static_first_tau_fused_kernel), and the second order runs without its UDiagonal launch
  const bool u_diag_fused = (stages & DDP_HIP_LIN_FIRST) && second_stage && pl.first == LinFirst::FdStatic &&
                            pl.second == LinSecond::Mode2Static && !ctx->sw.first_scalar;
  if (stages & DDP_HIP_LIN_COST) {
    if (ctx->flags & DDP_HIP_FLAG_TRACKING_COST)
      hipLaunchKernelGGL(lin_track_cost_kernel, dim3((unsigned)(BT + d.batch)), dim3(64), 0, ctx->stream, p);
    else hipLaunchKernelGGL(lin_cost_kernel, dim3((unsigned)BT), dim3(64), 0, ctx->stream, p);
    // the add-on terms, one kernel per live term, each adding onto what the ones before it left.  The fixed order of additions:
    // cost, tracking, frame positions, frame orientations, limits, CoM, frame velocities, momentum, balance regions, relative
    // frames, control-gravity, frame aiming, joint accelerations, obstacles, self-collision, capsules
    const dim3 blocks((unsigned)(BT + d.batch));
    const FrameCostDev fc = frame_cost_dev(ctx);
    const StateLimitsDev sl = state_limits_dev(ctx);
    const CoMCostDev cm = com_cost_dev(ctx);
    const FrameVelCostDev fv = frame_vel_cost_dev(ctx);
    const MomentumCostDev mo = momentum_cost_dev(ctx);
    const BalanceRegionDev br = balance_region_dev(ctx);
    const RelativeFrameDev rf = relative_frame_dev(ctx);
    const ControlGravDev cg = control_grav_dev(ctx);
    const FrameAimDev fa = frame_aim_dev(ctx);
    const JointAccelDev ja = joint_accel_dev(ctx);
    const ObstacleCostDev ob = obstacle_cost_dev(ctx);
    const SelfCollisionDev sc = self_collision_dev(ctx);
    const CapsuleCostDev cp = capsule_cost_dev(ctx);
    auto add = [&](bool live, auto kernel, const auto& dev) { if (live) hipLaunchKernelGGL(kernel, blocks, dim3(64), 0, ctx->stream, p, dev); };
    add(fc.target, lin_frame_cost_kernel, fc);
    add(fc.oquat, lin_frame_orient_cost_kernel, fc);
    add(sl.weight, lin_limit_cost_kernel, sl);
    add(cm.target, lin_com_cost_kernel, cm);
    add(fv.target, lin_frame_vel_cost_kernel, fv);
    add(mo.target, lin_momentum_cost_kernel, mo);
    add(br.geom, lin_balance_region_cost_kernel, br);
    add(rf.weight, lin_relative_frame_cost_kernel, rf);
    if (cg.weight)   // (t < T alone; G in dynamic LDS, nv^2 doubles)
      hipLaunchKernelGGL(lin_control_grav_cost_kernel, dim3((unsigned)BT), dim3(64), sizeof(double) * (size_t)(d.nv * d.nv), ctx->stream, p, cg);
    add(fa.weight, lin_frame_aim_cost_kernel, fa);
    if (ja.weight) {   // (t < T alone; nv <= 38 by the create-time check: the recursion's record in dynamic LDS, above 64 KB)
      constexpr int lds = (int)(sizeof(double) * rbdd::FfLds<DDP_HIP_MAX_JOINT_ACCEL_NV>::TOTAL);
      HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&lin_joint_accel_cost_kernel<DDP_HIP_MAX_JOINT_ACCEL_NV>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, lds));
      hipLaunchKernelGGL((lin_joint_accel_cost_kernel<DDP_HIP_MAX_JOINT_ACCEL_NV>), dim3((unsigned)BT), dim3(64), lds, ctx->stream, p, ja);
    }
    if (ob.grid_slots) add(ob.geom, lin_obstacle_cost_kernel<true>, ob);
    else add(ob.geom, lin_obstacle_cost_kernel<false>, ob);
    add(sc.margin, lin_self_collision_cost_kernel, sc);
    if (cp.grid_pairs && cp.box_pairs) add(cp.geom, lin_capsule_cost_kernel<true, true>, cp);
    else if (cp.grid_pairs) add(cp.geom, lin_capsule_cost_kernel<true, false>, cp);
    else if (cp.box_pairs) add(cp.geom, lin_capsule_cost_kernel<false, true>, cp);
    else add(cp.geom, lin_capsule_cost_kernel<false, false>, cp);
  }
  // the q- / v-caches of the mode-2 stencil also serve the first order (base configuration and base (q, v)), so they are built
  // ahead of whichever stage comes first
  bool caches_built = false;
  int static_rc = DDP_HIP_OK;
  auto build_caches = [&]() {
    if (caches_built) return;
    if (pl.topo) { const int rc_ = lin_static_launch(ctx, p, StaticLevel::Caches); if (rc_ != DDP_HIP_OK) static_rc = rc_; }
    else {
      hipLaunchKernelGGL((lin_qcache_kernel<NJ>), dim3(blocks_for(BT * (nv + 1))), dim3(LBS), 0, ctx->stream, p);
      hipLaunchKernelGGL((lin_vcache_kernel<NJ>), dim3(blocks_for(BT * (2 * nv + 1))), dim3(LBS), 0, ctx->stream, p);
    }
    caches_built = true;
  };
  if (stages & DDP_HIP_LIN_FIRST) {
    prof_begin(ctx, DDP_HIP_K_LIN_FIRST);
    hipLaunchKernelGGL((lin_base_kernel<NJ>), dim3(blocks_for(BT)), dim3(LBS), 0, ctx->stream, p);
    switch (pl.first) {
      case LinFirst::Base: break;
      case LinFirst::AnalyticSmall:
        if constexpr (small) hipLaunchKernelGGL((lin_first_analytic_small_kernel<NJ>), dim3(blocks_for(BT)), dim3(LBS), 0, ctx->stream, p);
        break;
      case LinFirst::AnalyticWave:
      case LinFirst::AnalyticFF: {
        const bool m1_next = pl.second == LinSecond::Mode1Wave && second_stage;   // its accelerations are formed now
        const int rc_ = lin_analytic_launch(ctx, p, call, 0, LIN_ANA_F | (m1_next ? LIN_ANA_ACCEL : 0) | (m1_next && eq_stage ? LIN_ANA_EQ << 4 : 0));
        if (rc_ != DDP_HIP_OK) return rc_;
        break;
      }
      case LinFirst::FdStatic: {
        build_caches();
        const int rc_ = lin_static_launch(ctx, p, u_diag_fused ? StaticLevel::FirstOrderUDiag : StaticLevel::FirstOrder);
        if (rc_ != DDP_HIP_OK) return rc_;
        break;
      }
      case LinFirst::FdGeneric:
        hipLaunchKernelGGL((lin_first_kernel<NJ>), dim3(blocks_for(BT * W)), dim3(LBS), 0, ctx->stream, p);
        break;
    }
    prof_end(ctx, DDP_HIP_K_LIN_FIRST);
  }
  if (second_stage) {
    const int64_t P = (int64_t)W * (W - 1) / 2, TRI = (int64_t)nv * (nv - 1) / 2, Pv = (int64_t)nv * nv + TRI, Pu = 2 * (int64_t)nv * nv + TRI;
    prof_begin(ctx, DDP_HIP_K_LIN_SECOND);
    switch (pl.second) {
      case LinSecond::None: break;
      case LinSecond::Mode2Static:
        build_caches();
        if (pl.forks) {   // the whole second order as one launch graph on the context's stream and the side stream
          const int rc_ = lin_static_launch(ctx, p, u_diag_fused ? StaticLevel::SecondOrderAfterUDiag : StaticLevel::SecondOrder);
          if (rc_ != DDP_HIP_OK) return rc_;
          break;
        }
        // torque level ahead of the other two: its row kernel also forms the diagonal entries of the q and v directions
        for (StaticLevel level : {StaticLevel::UDiagonal, StaticLevel::Torque, StaticLevel::Velocity, StaticLevel::Configuration}) {
          if (level == StaticLevel::UDiagonal && u_diag_fused) continue;
          const int rc_ = lin_static_launch(ctx, p, level);
          if (rc_ != DDP_HIP_OK) return rc_;
        }
        break;
      case LinSecond::Mode2Caches:
        build_caches();
        hipLaunchKernelGGL((lin_diag_kernel<NJ>), dim3(blocks_for(BT * W)), dim3(LBS), 0, ctx->stream, p);
        hipLaunchKernelGGL((lin_offdiag_kernel<NJ, 3>), dim3(blocks_for(BT * Pu)), dim3(LBS), 0, ctx->stream, p);
        hipLaunchKernelGGL((lin_offdiag_kernel<NJ, 2>), dim3(blocks_for(BT * Pv)), dim3(LBS), 0, ctx->stream, p);
        hipLaunchKernelGGL((lin_offdiag_kernel<NJ, 1>), dim3(blocks_for(BT * TRI)), dim3(LBS), 0, ctx->stream, p);
        break;
      case LinSecond::Mode2Plain:
        hipLaunchKernelGGL((lin_diag_kernel<NJ>), dim3(blocks_for(BT * W)), dim3(LBS), 0, ctx->stream, p);
        hipLaunchKernelGGL((lin_offdiag_kernel<NJ, 0>), dim3(blocks_for(BT * P)), dim3(LBS), 0, ctx->stream, p);
        break;
      case LinSecond::Mode1Small:
        if constexpr (small) hipLaunchKernelGGL((second_m1_kernel<NJ>), dim3(blocks_for(BT * W)), dim3(LBS), 0, ctx->stream, p, 0);
        break;
      case LinSecond::Mode1Wave:
        if (!m1_fused) { const int rc_ = lin_analytic_launch(ctx, p, call, 1, LIN_ANA_F); if (rc_ != DDP_HIP_OK) return rc_; }
        break;
      case LinSecond::Zeros:   // the Gauss-Newton variant
        HIP_TRY(hipMemsetAsync(p.fxx, 0, sizeof(double) * (size_t)(ctx->seq[DDP_HIP_SEQ_FXX].size * d.batch), ctx->stream));
        HIP_TRY(hipMemsetAsync(p.fux, 0, sizeof(double) * (size_t)(ctx->seq[DDP_HIP_SEQ_FUX].size * d.batch), ctx->stream));
        HIP_TRY(hipMemsetAsync(p.fuu, 0, sizeof(double) * (size_t)(ctx->seq[DDP_HIP_SEQ_FUU].size * d.batch), ctx->stream));
        break;
    }
    HIP_TRY(lin_join(ctx));   // (what was forked inside the bracket ends inside it)
    prof_end(ctx, DDP_HIP_K_LIN_SECOND);
  }
  if (eq_stage) {
    switch (pl.eq) {
      case LinEq::None: break;
      case LinEq::PerLane:
        if constexpr (small) hipLaunchKernelGGL((eq_first_kernel<NJ>), dim3(blocks_for(BT)), dim3(LBS), 0, ctx->stream, p);
        break;
      case LinEq::Analytic: {   // base point from the resident f_x, f_u
        const int rc_ = lin_analytic_launch(ctx, p, call, 0, LIN_ANA_EQ);
        if (rc_ != DDP_HIP_OK) return rc_;
        break;
      }
      case LinEq::Chain: {
        // chain rule as three kernels (round 3: the per-lane form differenced 2 x 18 full dynamics evaluations and multiplied
        // 12 x 12 matrices in ONE lane per (instance, t): 3.2 ms of latency at any size)
        const int K = ctx->model_h.eq_advance;
        if (K < 1) return DDP_HIP_E_UNSUPPORTED;
        hipLaunchKernelGGL((eq_chain_kernel<NJ>), dim3(blocks_for(BT)), dim3(LBS), 0, ctx->stream, p);
        if (pl.eq_jac == LinEqJac::Fd) hipLaunchKernelGGL((eq_fdjac_kernel<NJ>), dim3(blocks_for(BT * (K - 1) * d.n)), dim3(LBS), 0, ctx->stream, p);
        else if (pl.eq_jac == LinEqJac::FfLookahead) { const int rc_ = lin_analytic_ff_lookahead(ctx, p); if (rc_ != DDP_HIP_OK) return rc_; }
        hipLaunchKernelGGL(eq_combine_kernel, dim3((unsigned)BT), dim3(256), sizeof(double) * (size_t)(2 * d.emax * d.n), ctx->stream, p);
        break;
      }
    }
    const int rc_ = eq_second_order<NJ>(ctx, p, call, stages);
    if (rc_ != DDP_HIP_OK) return rc_;
  }
  HIP_TRY(hipGetLastError());
  return static_rc;
}

// ---- ctx->tensors: linearise's own two transitions (the other two follow ddp_hip_linearize_stages) ---------------------------
// Linearise is about to write the second order.  The record drops to Unknown until tensors_end_second: a call that returns an
// error in between leaves it there.  What the previous origin spares this call is decided first: the configuration rows the
// static stencil leaves alone must hold zeros (once per context, and again after somebody else has written to the tensors), and
// analytic mode 1 zeroes f_uu unless its own zeros are still there (lin_analytic.hip: launch_t, where that memset keeps its place)
int tensors_begin_second(ddp_hip_ctx* ctx, const LinParams& p, LinCall& call) {
  const TensorOrigin was = ctx->tensors.origin;
  ctx->tensors.origin = TensorOrigin::Unknown;
  ctx->tensors.packed = false;   // (records that are about to be overwritten, or contents nobody may rely on)
  call.fuu_zero = was == TensorOrigin::Analytic1;
  // (packed records have no zero rows: unpacking writes them)
  if (p.skip_top && !p.pack && was != TensorOrigin::Stencil) {
    const int64_t BT = ctx->d.batch * ctx->d.T, n = ctx->d.n, m = ctx->d.m;
    const int nv = (int)ctx->d.nv;
    hipLaunchKernelGGL(tensor_zero_top_kernel, dim3(8192), dim3(256), 0, ctx->stream, p.fxx, BT * n * n, (int)n, nv);
    hipLaunchKernelGGL(tensor_zero_top_kernel, dim3(8192), dim3(256), 0, ctx->stream, p.fux, BT * m * n, (int)n, nv);
    hipLaunchKernelGGL(tensor_zero_top_kernel, dim3(8192), dim3(256), 0, ctx->stream, p.fuu, BT * m * m, (int)n, nv);
    HIP_TRY(hipGetLastError());
  }
  return DDP_HIP_OK;
}

// Linearise has written the second order.  Mode 2 writes one value to both (i, j, k) and (i, k, j) (problem.hpp:283-292), mode 0
// leaves zeros: f_xx is symmetric bit for bit; mode 1's forward differences of jacobians are not.  (The run-time-tree kernels and
// mode 0 leave the stencil's zero rows as well -- a property of the values, not of who writes them -- but only the static mode-2
// path has been held to it bit for bit: tests/test_round3_boundary.py.)
void tensors_end_second(ddp_hip_ctx* ctx, const LinParams& p, const LinCall& call) {
  TensorState& t = ctx->tensors;
  if (ctx->model_h.fd_mode == 1) t.origin = call.fuu_zero ? TensorOrigin::Analytic1 : TensorOrigin::Unknown;   // (small models' mode 1: no structure kept)
  else t.origin = p.skip_top ? TensorOrigin::Stencil : TensorOrigin::Symmetric;
  t.mirror_pending = p.skip_qv_mirror != 0;
  t.packed = p.pack != 0;
}

}  // namespace

int lin_setup(ddp_hip_ctx* ctx) {
  const Dims& d = ctx->d;
  const int topo_id = ctx->model_h.kind == DDP_HIP_MODEL_TREE ? lin_static_supported(ctx->model_h) : 0;
  ctx->plan = lin_plan_decide(ctx->model_h, d, ctx->flags, ctx->sw, topo_id, sweep_plan(ctx).sym_ok);
  const LinPlan& pl = ctx->plan;
  if (pl.refuse) return pl.refuse;
  if (pl.ws_lin)
    HIP_TRY(hipMalloc(&ctx->lin_ws, sizeof(double) * (size_t)(d.batch * d.T * (lin_qc_per_bt(ctx) + lin_vc_per_bt(ctx)))));
  if (pl.ws_qws) {
    const int64_t BT = d.batch * d.T;
    // With the spine pre-pass forked ahead of the torque rows (LIN_FORK_SPINE) only the first slice's pre-pass runs beside them.
    // 3200 entries hold 13 330 spine sets of the Talos-like tree, its 64 seeds x 200 steps in one slice (measured: DESIGN.md
    // section 6b; the single-stream order is indifferent to the slice size)
    int64_t slice = (pl.forks & LIN_FORK_SPINE) ? 3200 : 1024;
    if (ctx->sw.qws_bt) slice = ctx->sw.qws_bt;   // tuning knob
    ctx->lin_qws_bt = BT < slice ? BT : slice;
    HIP_TRY(hipMalloc(&ctx->lin_qws, sizeof(double) * (size_t)(ctx->lin_qws_bt * lin_static_ws_per_bt(ctx->model_h))));
    if (pl.ws_qws2) {     // the full-ABA configuration level runs slice-pipelined on two streams
      HIP_TRY(hipMalloc(&ctx->lin_qws2, sizeof(double) * (size_t)(ctx->lin_qws_bt * lin_static_ws_per_bt(ctx->model_h))));
      HIP_TRY(hipStreamCreateWithFlags(&ctx->lin_stream2, hipStreamNonBlocking));
      for (int k = 0; k < 2; ++k) {
        HIP_TRY(hipEventCreateWithFlags(&ctx->lin_ev_up[k], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ctx->lin_ev_dn[k], hipEventDisableTiming));
      }
    }
  }
  if (pl.forks) {   // the concurrent schedule: one side stream and its events, for the context's life
    HIP_TRY(hipStreamCreateWithFlags(&ctx->lin_stream2, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&ctx->lin_ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ctx->lin_ev_done, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ctx->lin_ev_rows, hipEventDisableTiming));
  }
  { const int rc_ = lin_analytic_setup(ctx); if (rc_ != DDP_HIP_OK) return rc_; }
  if (pl.ws_eq) HIP_TRY(hipMalloc(&ctx->eq_ws, sizeof(double) * (size_t)pl.eq_words));   // look-ahead states / jacobians of the constraint chain
  if (pl.eq == LinEq::Chain) {
    // eq_combine_kernel keeps two e x n matrices in LDS: past the default 64 KB of dynamic LDS with a config constraint from nv = 46 on
    // (128 KB at nv = 64: it always fits the workgroup's 160 KB)
    const size_t lds = sizeof(double) * (size_t)(2 * d.emax * d.n);
    if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&eq_combine_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  return DDP_HIP_OK;
}
void lin_teardown(ddp_hip_ctx* ctx) {
  lin_analytic_teardown(ctx);
  for (int k = 0; k < 2; ++k) {
    if (ctx->lin_ev_up[k]) (void)hipEventDestroy(ctx->lin_ev_up[k]);
    if (ctx->lin_ev_dn[k]) (void)hipEventDestroy(ctx->lin_ev_dn[k]);
  }
  for (hipEvent_t ev : {ctx->lin_ev_fork, ctx->lin_ev_done, ctx->lin_ev_rows}) if (ev) (void)hipEventDestroy(ev);
  if (ctx->lin_stream2) (void)hipStreamDestroy(ctx->lin_stream2);
  if (ctx->lin_qws2) (void)hipFree(ctx->lin_qws2);
  if (ctx->lin_qws) (void)hipFree(ctx->lin_qws);
  if (ctx->eq_ws) (void)hipFree(ctx->eq_ws);
  if (ctx->lin_ws) (void)hipFree(ctx->lin_ws);
}

extern "C" int ddp_hip_linearize_stages(ddp_hip_ctx* ctx, uint32_t stages) {
  if (!ctx) return DDP_HIP_E_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  LinParams p = make_params(ctx);
  LinCall call;
  LinJoin joined(ctx);   // whatever this call leaves on the side stream is joined into ctx->stream on every way out
  const bool second = (stages & DDP_HIP_LIN_SECOND) && p.has_tensors;
  if (second) { const int rc_ = tensors_begin_second(ctx, p, call); if (rc_ != DDP_HIP_OK) return rc_; }
  int rc;
  switch (ctx->plan.nj) {
    case 1: rc = run_linearize<1>(ctx, p, call, stages); break;
    case 6: rc = run_linearize<6>(ctx, p, call, stages); break;
    case 38: rc = run_linearize<38>(ctx, p, call, stages); break;
    default: rc = run_linearize<64>(ctx, p, call, stages); break;
  }
  if (rc != DDP_HIP_OK) return rc;
  END_SYNC(ctx);
  if (second) tensors_end_second(ctx, p, call);
  return DDP_HIP_OK;
}

// ---- the other two transitions of ctx->tensors ------------------------------------------------------------------------------
int tensors_written_outside(ddp_hip_ctx* ctx, int seq) {
  if (seq != DDP_HIP_SEQ_FXX && seq != DDP_HIP_SEQ_FUX && seq != DDP_HIP_SEQ_FUU) return DDP_HIP_OK;
  TensorState& t = ctx->tensors;
  // packed records are unpacked first, all three tensors together: the caller overwrites part of one of them at most
  if (t.packed) { const int rc_ = lin_materialize_fxx(ctx); if (rc_ != DDP_HIP_OK) return rc_; }
  if (seq == DDP_HIP_SEQ_FUX) {
    // f_ux carries no symmetry: f_xx / f_uu stay as symmetric as they were (and as incomplete), the zero rows are gone
    t.origin = (t.origin == TensorOrigin::Symmetric || t.origin == TensorOrigin::Stencil) ? TensorOrigin::Symmetric : TensorOrigin::Unknown;
    return DDP_HIP_OK;
  }
  // what the caller does not overwrite (other instances, the other tensor) stays whole; no symmetry assumed from here on:
  // K3 reads every half-slab again (bwd_split.h)
  const int rc_ = lin_materialize_fxx(ctx);
  if (rc_ != DDP_HIP_OK) return rc_;
  t.origin = TensorOrigin::Unknown;
  return DDP_HIP_OK;
}

// the tensors materialised: packed records back in the contract layout, then the mirror images formed -- FXX / FUX / FUU complete
// for a reader that knows neither the records nor the skipped block (download, device_ptr, upload / fill, any sweep but the
// packed K3h).  Afterwards the state is what a linearisation without packing leaves: Stencil, read by the strided K3h
int lin_materialize_fxx(ddp_hip_ctx* ctx) {
  double* fxx = ctx->seq[DDP_HIP_SEQ_FXX].ptr;
  double* fuu = ctx->seq[DDP_HIP_SEQ_FUU].ptr;
  if (ctx->tensors.packed) {
    double* fux = ctx->seq[DDP_HIP_SEQ_FUX].ptr;
    const int64_t BT = ctx->d.batch * ctx->d.T, n = ctx->d.n, m = ctx->d.m, nv = ctx->d.nv;
    if (!fxx || !fux || !fuu || m > n) return DDP_HIP_E_UNSUPPORTED;
    hipLaunchKernelGGL(tensor_unpack_kernel, dim3((unsigned)(BT * (2 * n + m))), dim3(UNPACK_BS), sizeof(double) * (size_t)(n * (nv + 2)), ctx->stream,
                       fxx, fux, fuu, (int)n, (int)m, (int)nv);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->tensors.packed = false;
  }
  if (!ctx->tensors.mirror_pending) return DDP_HIP_OK;
  if (fxx && fuu) {
    const int64_t BT = ctx->d.batch * ctx->d.T;
    hipLaunchKernelGGL(tensor_mirror_kernel, dim3(8192), dim3(256), 0, ctx->stream, fxx, BT, (int)ctx->d.n, (int)ctx->d.n);
    hipLaunchKernelGGL(tensor_mirror_kernel, dim3(4096), dim3(256), 0, ctx->stream, fuu, BT, (int)ctx->d.n, (int)ctx->d.m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  ctx->tensors.mirror_pending = false;
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_linearize(ddp_hip_ctx* ctx) {
  return ddp_hip_linearize_stages(ctx, DDP_HIP_LIN_COST | DDP_HIP_LIN_FIRST | DDP_HIP_LIN_SECOND | DDP_HIP_LIN_EQ);
}
