// fwd.hip -- trajectory rollout, augmented cost and the forward sweep with batched line-search steps.
//
// Replaces make_trajectory (ddp.hpp:392-415), cost_seq_aug (ddp.hpp:699-735) and
// forward_pass<M> (ddp_fwd.ipp:9-67).  A rollout is sequential in t; the independent units are the
// (instance, step-size candidate) chains: one lane per chain, the candidates of one instance in
// adjacent lanes so that the gain matrices K_t are fetched once per wave.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>
#include <vector>

#include "balance_region_cost.h"
#include "capsule_cost.h"
#include "com_cost.h"
#include "control_grav_cost.h"
#include "frame_aim_cost.h"
#include "frame_cost.h"
#include "frame_vel_cost.h"
#include "internal.h"
#include "joint_accel_cost.h"
#include "momentum_cost.h"
#include "obstacle_cost.h"
#include "rbd.h"
#include "relative_frame_cost.h"
#include "self_collision_cost.h"
#include "state_limits.h"

namespace {

struct FwdParams {
  Dims d;
  const DevModel* model;
  const int64_t* ne;
  const int64_t* Epre;
  const double* target;
  const double *x_old, *u_old;
  double *x_new, *u_new;
  const double *fb_val, *fb_jac;
  const double *mult_origin, *mult_val, *mult_jac;
  const double* mu;
  double *costs_old, *costs_new;
  double *fw_x, *fw_u, *fw_dcost;
  double* step;
  double* dcost_acc;
  int32_t* state;
  int32_t n_alpha, round;
  int32_t no_linesearch;         // ddp_fwd.ipp:61-63: the full step is taken whatever the cost does
  int32_t cost_inline;           // latency kernel: 1 = forms sum_t (cost_new - cost_old) itself (no constraints), 0 = cand_cost_kernel does
  double* fw_cost;               // [batch][n_alpha][T+1] cost terms of the candidates (constrained problems on the latency path)
  const double *xref, *wx, *uref, *wu;   // tracking cost (DDP_HIP_FLAG_TRACKING_COST), else null
  int32_t track;
  const double *ctrl_lo, *ctrl_hi;       // control bounds (DDP_HIP_FLAG_CONTROL_BOUNDS), else null
  FrameCostDev fc;                       // frame-position cost (DDP_HIP_FLAG_FRAME_COST); fc.target null: no terms; fc.oquat null: no
                                         // orientation terms (DDP_HIP_FLAG_FRAME_ORIENT_COST)
  StateLimitsDev sl;                     // soft state limits (DDP_HIP_FLAG_STATE_LIMITS); sl.weight null: no terms
};

// constraint value at solver time t: constraint_advance_time_t::eval_to (problem.hpp:563-567) applied
// eq_advance times around config_constraint_t (:792-806) or spatial_constraint_t (:679-689)
template <int NJ>
__device__ void eval_eq(const DevModel& m, const double* target, int e, const double* x, const double* u, double* out) {
  const int nx = m.nq + m.nv;
  double xa[2 * NJ + 1], xb[2 * NJ + 1];
  for (int i = 0; i < nx; ++i) xa[i] = x[i];
  for (int k = 0; k < m.eq_advance; ++k) {
    if (k + 1 < m.eq_advance) rbd::eval_f<NJ>(m, xa, u, xb);
    else { for (int i = m.nq; i < nx; ++i) xb[i] = xa[i]; rbd::eval_f_q<NJ>(m, xa, xb); }   // the constraint reads q only (rbd.h: eval_f_q)
    for (int i = 0; i < nx; ++i) xa[i] = xb[i];
  }
  if (m.eq_kind == DDP_HIP_EQ_CONFIG) {
    for (int i = 0; i < e; ++i) out[i] = xa[i] - target[i];
  } else {
    double p[3];
    rbd::frame_position<NJ>(m, xa, p, nullptr);
    for (int i = 0; i < e; ++i) out[i] = p[i] - target[i];
  }
}

// 1/2 sum_i w_i d_i^2, d = x (-) xr (lie::difference_x, formed entry by entry): the state terms of the tracking cost
// (ddp_hip.h: DDP_HIP_FLAG_TRACKING_COST).  A term of weight 0 is left out, not multiplied by 0: a diverging rollout (inf)
// costs what it costs without the flag instead of NaN
__device__ __forceinline__ double track_state_sum(bool ff, int nv, const double* xr, const double* x, const double* w) {
  const int nq = ff ? nv + 1 : nv;
  double s = 0;
  int i = 0;
  if (ff) {
    double d6[6];
    lie::se3_difference(xr, x, d6);
    for (; i < 6; ++i) if (w[i] != 0.0) s += w[i] * d6[i] * d6[i];
  }
  for (; i < nv; ++i) { const double di = x[i + nq - nv] - xr[i + nq - nv]; if (w[i] != 0.0) s += w[i] * di * di; }
  for (; i < 2 * nv; ++i) { const double di = x[nq + i - nv] - xr[nq + i - nv]; if (w[i] != 0.0) s += w[i] * di * di; }
  return 0.5 * s;
}
// ... at time t of instance b; t = T: the terminal cost lf
__device__ __forceinline__ double track_state_cost(const FwdParams& p, int b, int64_t t, const double* x) {
  const int nv = (int)p.d.nv, nx = (int)p.d.nx;
  const int64_t bt = (int64_t)b * (p.d.T + 1) + t;
  return track_state_sum(nx > 2 * nv, nv, p.xref + bt * nx, x, p.wx + bt * 2 * nv);
}
// 1/2 sum_j wu_j (u_j - uref_j)^2 at time t < T of instance b
__device__ __forceinline__ double track_control_sum(const FwdParams& p, int b, int64_t t, const double* u) {
  const int nv = (int)p.d.nv;
  const double* ur = p.uref + ((int64_t)b * p.d.T + t) * nv;
  const double* wu = p.wu + ((int64_t)b * p.d.T + t) * nv;
  double su = 0;
  for (int i = 0; i < nv; ++i) { const double du = u[i] - ur[i]; if (wu[i] != 0.0) su += wu[i] * du * du; }
  return 0.5 * su;
}

// sum_a w_a (p_f(q)_a - g_a)^2 of frame f at (instance, t) pair bt1 = b (T + 1) + t (ddp_hip.h: DDP_HIP_FLAG_FRAME_COST).  A term
// of weight 0 is left out, and with all three of them the walk along the frame's path.  M: DevModel, or the CoopModel in LDS
template <class M>
__device__ __forceinline__ double frame_term(const FrameCostDev& fc, const M& m, bool ff, int f, int64_t bt1, const double* q) {
  const double* w = fc.weight + (bt1 * fc.nf + f) * 3;
  if (!rbd::frame_weights_any(w)) return 0.0;
  const double* g = fc.target + (bt1 * fc.nf + f) * 3;
  const double off[3] = {fc.off[f][0], fc.off[f][1], fc.off[f][2]};
  double pf[3], s = 0;
  rbd::frame_point(m, ff, fc.joint[f], off, q, pf);
  for (int a = 0; a < 3; ++a) { const double r = pf[a] - g[a]; if (w[a] != 0.0) s += w[a] * r * r; }
  return s;
}
// the frame terms of l at time t of instance b (t = T: of lf), one lane for all frames
__device__ double frame_cost_sum(const FrameCostDev& fc, const DevModel& m, int64_t bt1, const double* x) {
  double s = 0;
  for (int f = 0; f < fc.nf; ++f) s += frame_term(fc, m, m.ff != 0, f, bt1, x);
  return 0.5 * s;
}

// sum_a w_a e_a^2 of frame f at (instance, t) pair bt1, e = log3(R_ref^T R_f(q)) (ddp_hip.h: DDP_HIP_FLAG_FRAME_ORIENT_COST): a
// sibling of frame_term.  A term of weight 0 is left out, and with all three of them the walk along the frame's path
template <class M>
__device__ __forceinline__ double frame_orient_term(const FrameCostDev& fc, const M& m, bool ff, int f, int64_t bt1, const double* q) {
  const double* w = fc.oweight + (bt1 * fc.nf + f) * 3;
  if (!rbd::frame_weights_any(w)) return 0.0;
  double R[9], e[3], s = 0;
  rbd::frame_rotation(m, ff, fc.joint[f], q, R);
  lie::so3_log_rel(fc.oquat + (bt1 * fc.nf + f) * 4, R, e);
  for (int a = 0; a < 3; ++a) if (w[a] != 0.0) s += w[a] * e[a] * e[a];
  return s;
}
// the orientation terms of l at time t of instance b (t = T: of lf), one lane for all frames
__device__ double frame_orient_sum(const FrameCostDev& fc, const DevModel& m, int64_t bt1, const double* x) {
  double s = 0;
  for (int f = 0; f < fc.nf; ++f) s += frame_orient_term(fc, m, m.ff != 0, f, bt1, x);
  return 0.5 * s;
}

// 1/2 sum_i w_i e_i^2 over the tangent rows of the state at (instance, t) pair bt1, e_i the amount by which the row's state
// coordinate leaves [lo_i, hi_i] (ddp_hip.h: DDP_HIP_FLAG_STATE_LIMITS): a sibling of track_state_sum, one lane, rows in order.
// A row of weight 0 reads neither bound and a row inside its interval adds nothing: with limits that do not bind the sum is +0
__device__ __forceinline__ double limit_state_sum(const StateLimitsDev& sl, bool ff, int nv, int64_t bt1, const double* x) {
  const int nq = ff ? nv + 1 : nv, n = 2 * nv;
  const double* w = sl.weight + bt1 * n;
  const double* lo = sl.lo + bt1 * n;
  const double* hi = sl.hi + bt1 * n;
  double s = 0;
  for (int i = ff ? 6 : 0; i < n; ++i) {
    const double wi = w[i];
    if (wi == 0.0) continue;
    const double e = limit_excess(x[limit_coord(i, nv, nq)], lo[i], hi[i]);
    if (e != 0.0) s += wi * e * e;
  }
  return 0.5 * s;
}

// one term of cost_seq_aug (ddp.hpp:730): l + pe.ce + mu/2 |ce|^2
// FRAME: a level -- 0 none, 1 + the frame-position terms (DDP_HIP_FLAG_FRAME_COST), 2 + the frame-orientation terms after them
// (DDP_HIP_FLAG_FRAME_ORIENT_COST; the position side may be off there: fc.target null) -- in instantiations of their own of
// cost_kernel, forward_kernel and cand_cost_kernel: a run-time branch here moved the spills of the kernels that exist without
// the flag
// LIMIT: + the state-limit terms (DDP_HIP_FLAG_STATE_LIMITS), after the frame terms, in instantiations of their own alike
template <int NJ, int FRAME = 0, bool LIMIT = false>
__device__ double stage_cost(const FwdParams& p, const DevModel& m, int b, int64_t t, const double* x, const double* u, double mu) {
  const int nv = m.nv, n = 2 * nv, nx = m.nq + nv;
  double un = 0;
  for (int i = 0; i < nv; ++i) un += u[i] * u[i];
  double cost = 0.5 * m.c * un;                                   // problem_t::l, problem.hpp:937-942
  if (p.track) cost += track_state_cost(p, b, t, x) + track_control_sum(p, b, t, u);   // + the tracking terms
  if constexpr (FRAME == 1) cost += frame_cost_sum(p.fc, m, (int64_t)b * (p.d.T + 1) + t, x);   // + the frame terms
  if constexpr (FRAME == 2) {
    if (p.fc.target) cost += frame_cost_sum(p.fc, m, (int64_t)b * (p.d.T + 1) + t, x);
    cost += frame_orient_sum(p.fc, m, (int64_t)b * (p.d.T + 1) + t, x);                   // + the frame-orientation terms
  }
  if constexpr (LIMIT) cost += limit_state_sum(p.sl, m.ff != 0, nv, (int64_t)b * (p.d.T + 1) + t, x);   // + the state-limit terms
  const int e = (int)p.ne[t];
  if (e > 0) {
    double ce[NJ > 3 ? NJ : 3];
    const int64_t Eo = p.Epre[t], Etot = p.d.Etot;
    eval_eq<NJ>(m, p.target + Eo, e, x, u, ce);
    const double* org = p.mult_origin + ((int64_t)b * p.d.T + t) * nx;
    const double* val = p.mult_val + (int64_t)b * Etot + Eo;
    const double* jac = p.mult_jac + ((int64_t)b * Etot + Eo) * n;
    double dot = 0, sq = 0;
    double dxo[2 * NJ];
    if (m.ff) lie::difference_x(m, org, x, dxo);                  // x (-) origin on the group
    for (int i = 0; i < e; ++i) {
      double pe = val[i];                                         // mat_seq_common.hpp:105-115
      double s = 0;
      for (int l = 0; l < n; ++l) s += jac[i + (int64_t)l * e] * (m.ff ? dxo[l] : x[l] - org[l]);
      pe += s;
      dot += pe * ce[i];
      sq += ce[i] * ce[i];
    }
    cost += dot;
    cost += (mu / 2) * sq;
  }
  return cost;
}

template <int NJ>
__global__ void rollout_kernel(FwdParams p) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.d.batch) return;
  const DevModel& m = *p.model;
  const int nx = m.nq + m.nv, nu = m.nv;
  double* xs = const_cast<double*>(p.x_old) + (int64_t)b * (p.d.T + 1) * nx;
  const double* us = p.u_old + (int64_t)b * p.d.T * nu;
  double x[2 * NJ + 1], xn[2 * NJ + 1], u[NJ];
  for (int i = 0; i < nx; ++i) x[i] = xs[i];
  for (int64_t t = 0; t < p.d.T; ++t) {
    for (int i = 0; i < nu; ++i) u[i] = us[t * nu + i];
    rbd::eval_f<NJ>(m, x, u, xn);
    for (int i = 0; i < nx; ++i) { x[i] = xn[i]; xs[(t + 1) * nx + i] = xn[i]; }
  }
}

// problem_t::lf (problem.hpp:932-936: 0), or the tracking cost's terminal term
template <int FRAME = 0, bool LIMIT = false>
__device__ __forceinline__ double terminal_cost(const FwdParams& p, const DevModel& m, int b, const double* x) {
  double cost = p.track ? track_state_cost(p, b, p.d.T, x) : 0.0;
  if constexpr (FRAME == 1) cost += frame_cost_sum(p.fc, m, (int64_t)b * (p.d.T + 1) + p.d.T, x);
  if constexpr (FRAME == 2) {
    if (p.fc.target) cost += frame_cost_sum(p.fc, m, (int64_t)b * (p.d.T + 1) + p.d.T, x);
    cost += frame_orient_sum(p.fc, m, (int64_t)b * (p.d.T + 1) + p.d.T, x);
  }
  if constexpr (LIMIT) cost += limit_state_sum(p.sl, m.ff != 0, m.nv, (int64_t)b * (p.d.T + 1) + p.d.T, x);
  return cost;
}

// cost_seq_aug of one trajectory: one lane per (instance, t)
template <int NJ, int FRAME = 0, bool LIMIT = false>
__global__ void cost_kernel(FwdParams p, int which) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t T = p.d.T;
  if (gid >= p.d.batch * (T + 1)) return;
  const int b = (int)(gid / (T + 1));
  const int64_t t = gid % (T + 1);
  const DevModel& m = *p.model;
  const int nx = m.nq + m.nv, nu = m.nv;
  double* out = (which == 0 ? p.costs_old : p.costs_new) + (int64_t)b * (T + 1);
  const double* xs = (which == 0 ? p.x_old : p.x_new) + ((int64_t)b * (T + 1) + t) * nx;
  if (t == T) { out[T] = terminal_cost<FRAME, LIMIT>(p, m, b, xs); return; }
  const double* us = (which == 0 ? p.u_old : p.u_new) + ((int64_t)b * T + t) * nu;
  double x[2 * NJ + 1], u[NJ];
  for (int i = 0; i < nx; ++i) x[i] = xs[i];
  for (int i = 0; i < nu; ++i) u[i] = us[i];
  out[t] = stage_cost<NJ, FRAME, LIMIT>(p, m, b, t, x, u, p.mu[b]);
}

// closed-loop rollouts (ddp_fwd.ipp:39-51) of n_alpha candidate steps per instance + their summed cost
// difference (ddp_fwd.ipp:54-56)
template <int NJ, int FRAME = 0, bool LIMIT = false>
__global__ void forward_kernel(FwdParams p) {
  // the model table in LDS: the dynamics of every step read it joint by joint (axis, placement, inertia: some 40 words per joint
  // and evaluation), and from global memory each of those reads is a dependent L2 round trip of the one lane that rolls out
  __shared__ DevModel s_model;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(p.model);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&s_model);
    for (unsigned i = threadIdx.x; i < sizeof(DevModel) / 4; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int na = p.n_alpha;
  if (gid >= p.d.batch * na) return;
  const int b = gid / na, a = gid % na;
  if (p.state[b] != 0) return;
  const int cand = p.round * na + a;
  if (cand > 33) { p.fw_dcost[(int64_t)b * na + a] = INFINITY; return; }   // 2^-34 < 1e-10: never tried (ddp_fwd.ipp:35-37)
  const double step = ldexp(1.0, -cand);
  const DevModel& m = s_model;
  const int nv = m.nv, n = 2 * nv, nx = m.nq + nv, nu = nv;
  const int64_t T = p.d.T;
  const double mu = p.mu[b];
  const double* xo = p.x_old + (int64_t)b * (T + 1) * nx;
  const double* uo = p.u_old + (int64_t)b * T * nu;
  double* xw = p.fw_x + ((int64_t)b * na + a) * (T + 1) * nx;
  double* uw = p.fw_u + ((int64_t)b * na + a) * T * nu;
  const double* cold = p.costs_old + (int64_t)b * (T + 1);
  double x[2 * NJ + 1], xn[2 * NJ + 1], u[NJ], dx[2 * NJ];
  const double* x0 = p.x_new + (int64_t)b * (T + 1) * nx;        // x_new,0 is preset by the caller (ddp.hpp:752)
  for (int i = 0; i < nx; ++i) { x[i] = x0[i]; xw[i] = x0[i]; }
  double dsum = 0.0;
  for (int64_t t = 0; t < T; ++t) {
    const double* k = p.fb_val + ((int64_t)b * T + t) * nu;
    const double* K = p.fb_jac + ((int64_t)b * T + t) * nu * n;
    if (m.ff) lie::difference_x(m, xo + t * nx, x, dx);                       // :45 difference(out, old, new)
    else for (int i = 0; i < n; ++i) dx[i] = x[i] - xo[t * nx + i];
    for (int i = 0; i < nu; ++i) u[i] = uo[t * nu + i] + step * k[i];         // :47-48
    for (int i = 0; i < nu; ++i) {
      double s = 0;
      for (int l = 0; l < n; ++l) s += K[i + l * nu] * dx[l];
      u[i] += s;                                                              // :49
    }
    if (p.ctrl_lo) {
      // control bounds: this form, not fmin / fmax -- the NaN of a diverged candidate stays a NaN
      const double* lo = p.ctrl_lo + ((int64_t)b * T + t) * nu;
      const double* hi = p.ctrl_hi + ((int64_t)b * T + t) * nu;
      for (int i = 0; i < nu; ++i) u[i] = u[i] < lo[i] ? lo[i] : (u[i] > hi[i] ? hi[i] : u[i]);
    }
    for (int i = 0; i < nu; ++i) uw[t * nu + i] = u[i];
    const double c_new = stage_cost<NJ, FRAME, LIMIT>(p, m, b, t, x, u, mu);
    dsum += c_new - cold[t];
    rbd::eval_f<NJ>(m, x, u, xn);                                             // :50
    for (int i = 0; i < nx; ++i) { x[i] = xn[i]; xw[(t + 1) * nx + i] = xn[i]; }
  }
  dsum += terminal_cost<FRAME, LIMIT>(p, m, b, x) - cold[T];
  p.fw_dcost[(int64_t)b * na + a] = dsum;
}

// The tracking terms of one candidate of forward_kernel_lat2 at time t (t = T: lf, no control terms), by its 16 lanes h: lane h
// takes the state rows r0 + h, r0 + h + 16, ... and the controls h, h + 16, ...; lane 0 the six rows of a free-flyer root
// (lie::se3_difference); the 16 partial sums meet in a fixed butterfly.  Every lane of the wave calls it (the shuffles span
// the candidate's 16 lanes); not live: 0
template <bool FF>
__device__ __forceinline__ double track_lanes_sum(const FwdParams& p, int b, int64_t t, const double* x, const double* u, int h, bool live) {
  const int nv = (int)p.d.nv, n = 2 * nv, nx = (int)p.d.nx, nq = nx - nv, r0 = FF ? 6 : 0;
  constexpr int NH = 16;
  const int64_t T = p.d.T, bt1 = (int64_t)b * (T + 1) + t;
  const double* xr = p.xref + bt1 * nx;
  const double* w = p.wx + bt1 * n;
  double s = 0, su = 0;
  if (live) {
    if (FF && h == 0) {
      double d6[6];
      lie::se3_difference(xr, x, d6);
      for (int i = 0; i < 6; ++i) if (w[i] != 0.0) s += w[i] * d6[i] * d6[i];
    }
    for (int i = r0 + h; i < n; i += NH) {
      const int k = i < nv ? i + nq - nv : nq + i - nv;
      const double di = x[k] - xr[k];
      if (w[i] != 0.0) s += w[i] * di * di;
    }
    if (t < T) {
      const double* ur = p.uref + ((int64_t)b * T + t) * nv;
      const double* wu = p.wu + ((int64_t)b * T + t) * nv;
      for (int j = h; j < nv; j += NH) { const double du = u[j] - ur[j]; if (wu[j] != 0.0) su += wu[j] * du * du; }
    }
  }
  double v = 0.5 * s + 0.5 * su;
#pragma unroll
  for (int k = NH / 2; k >= 1; k /= 2) v += __shfl_xor(v, k, NH);
  return v;
}

// The frame terms of one candidate of forward_kernel_lat2 at time t (t = T: lf): lane h < nf walks frame h's path from the
// candidate's state and the model tables in LDS (the placements of q_t do not exist yet where this is called, and x_T never
// gets a dynamics step); the partial sums meet in the same fixed butterfly as track_lanes_sum's.  Every lane of the wave calls it
template <bool FF, class M>
__device__ __forceinline__ double frame_lanes_sum(const FwdParams& p, const M& cm, int b, int64_t t, const double* x, int h, bool live) {
  constexpr int NH = 16;
  double s = 0;
  if (live && h < p.fc.nf) s = frame_term(p.fc, cm, FF, h, (int64_t)b * (p.d.T + 1) + t, x);
  double v = 0.5 * s;
#pragma unroll
  for (int k = NH / 2; k >= 1; k /= 2) v += __shfl_xor(v, k, NH);
  return v;
}

// The frame terms of one candidate of a COST bit 3 instantiation: lane h < nf keeps frame h's position term as in
// frame_lanes_sum (none while the position side is off: fc.target null), lane 4 + h forms frame h's orientation term
// (frame_orient_term) from the same state and tables; the same fixed butterfly.  Every lane of the wave calls it
template <bool FF, class M>
__device__ __forceinline__ double frame_orient_lanes_sum(const FwdParams& p, const M& cm, int b, int64_t t, const double* x, int h, bool live) {
  constexpr int NH = 16;
  static_assert(2 * DDP_HIP_MAX_COST_FRAMES <= NH, "a lane per frame and kind of term");
  double s = 0;
  if (live) {
    if (h < DDP_HIP_MAX_COST_FRAMES) { if (h < p.fc.nf && p.fc.target) s = frame_term(p.fc, cm, FF, h, (int64_t)b * (p.d.T + 1) + t, x); }
    else if (h - DDP_HIP_MAX_COST_FRAMES < p.fc.nf) s = frame_orient_term(p.fc, cm, FF, h - DDP_HIP_MAX_COST_FRAMES, (int64_t)b * (p.d.T + 1) + t, x);
  }
  double v = 0.5 * s;
#pragma unroll
  for (int k = NH / 2; k >= 1; k /= 2) v += __shfl_xor(v, k, NH);
  return v;
}

// The state-limit terms of one candidate of forward_kernel_lat2 at time t (t = T: lf): lane h takes the tangent rows r0 + h,
// r0 + h + 16, ... (r0 = 6 on a free flyer, whose pose rows carry no limit), track_lanes_sum's split; a row of weight 0 reads
// neither bound; the partial sums meet in the same fixed butterfly.  Every lane of the wave calls it
template <bool FF>
__device__ __forceinline__ double limit_lanes_sum(const FwdParams& p, int b, int64_t t, const double* x, int h, bool live) {
  const int nv = (int)p.d.nv, n = 2 * nv, nq = (int)p.d.nx - nv, r0 = FF ? 6 : 0;
  constexpr int NH = 16;
  const int64_t bt1 = (int64_t)b * (p.d.T + 1) + t;
  const double* w = p.sl.weight + bt1 * n;
  const double* lo = p.sl.lo + bt1 * n;
  const double* hi = p.sl.hi + bt1 * n;
  double s = 0;
  if (live)
    for (int i = r0 + h; i < n; i += NH) {
      const double wi = w[i];
      if (wi == 0.0) continue;
      const double e = limit_excess(x[limit_coord(i, nv, nq)], lo[i], hi[i]);
      if (e != 0.0) s += wi * e * e;
    }
  double v = 0.5 * s;
#pragma unroll
  for (int k = NH / 2; k >= 1; k /= 2) v += __shfl_xor(v, k, NH);
  return v;
}

// Latency path of the same rollouts (trees of the Talos size): one 64-lane workgroup (= one wave) per (instance, four
// candidates), 16 lanes per candidate.  What a rollout waits for at every step is global memory: the 23 KB gain matrix K_t (written by the backward sweep a whole
// linearisation ago: an HBM read in the middle of the step), k_t, u_old, x_old, and the per-level reads of the model tables
// inside the traversal (dependent L2 round trips, three per tree level).  Here
//   * the model (inertias, axes, placements, level tables: rbd::CoopModel) is copied to LDS once per launch;
//   * K_{t+1}, k_{t+1}, u_old,t+1, x_old,t+1 are requested right after the control update of step t, travel while the forward
//     dynamics of step t run, and are parked in LDS at the end of the step (registers are the second buffer);
//   * the workgroup is a single wave, so the exchange points of the traversal are compiler fences, not s_barrier + vmcnt(0)
//     (rbd::coop_sync): the prefetch stays in flight through them;
//   * the gain product is row-parallel: lane h of a candidate owns rows h, h + 16, h + 32 of K_t dx and runs down the columns
//     in order (LDS reads, conflict-free; the four candidates read the same words).
// Four candidates per workgroup halve the per-joint state (72 KB), which is what makes room for K_t and the model.
template <int NJ>
struct FwdLat2Lds {
  static constexpr int NC = 4, NH = 16, n = 2 * NJ + 1, nu = NJ;   // n: room for the state of a free-flyer model (nq = nv + 1)
  double state[rbd::ABA_LDS_SLOTS * (NJ + NJ / 8) * NC];       // (+ NJ / 8: the bank skew of rbd::aba_tree_coop2w)
  double K[nu * n];
  double k[nu], uo[nu], xo[n];
  double dx[NC * n], x[NC * n], u[NC * nu], qdd[NC * nu];
  rbd::CoopModel<NJ> model;
};

// ... of the control-bounds instantiations: lo_t, hi_t beside k_t
template <int NJ>
struct FwdLat2LdsBox : FwdLat2Lds<NJ> {
  double lo[NJ], hi[NJ];
};

// ... of the pipelined form (PIPE below): two candidates per workgroup.  Per joint and candidate the q-part's record twice (step t's
// is read while step t + 1's is written), its contribution slots and the x-part's own slots, 2 x 41 + 21 + 19 = 122 words against
// 59: at four candidates 148 KB of state alone, at two 74 KB (118 KB with K_t and the model).  The state x twice as well: the helper
// wave writes q_{t+1} into the other copy while the leading wave still reads x_t
template <int NJ>
struct FwdPipeLds {
  static constexpr int NC = 2, NH = 16, n = 2 * NJ + 1, nu = NJ;
  double rec[2][rbd::ABA_PIPE_QSLOTS * NJ * NC];
  double z[rbd::ABA_PIPE_ZSLOTS * NJ * NC];
  double state[rbd::ABA_PIPE_XSLOTS * NJ * NC];
  double K[nu * n];
  double k[nu], uo[nu], xo[n];
  double dx[NC * n], x[2 * NC * n], u[NC * nu], qdd[NC * nu];
  rbd::CoopModel<NJ> model;
  int u_step;                                      // the hand-off inside a step: the t whose u_t is whole in `u` (rbd::lds_post / lds_await)
};
template <int NJ>
struct FwdPipeLdsBox : FwdPipeLds<NJ> {
  double lo[NJ], hi[NJ];
};

// The form a launch takes: the pipelined one while its grid, one workgroup per (instance, two candidates), fits the compute units
// (each workgroup fills a CU's LDS: more of them than CUs would run in two rounds where the four-candidate form runs in one)
static bool fwd_use_pipe(const ddp_hip_ctx* ctx, int64_t batch, int n_alpha) {
  return !ctx->sw.fwd_no_pipe && batch * ((n_alpha + 1) / 2) <= ctx->cu_count;
}

// The pipelined instantiations that run the third wave (the assistant, below).  Five closed-loop ones spilled 4 to 8 bytes more
// per lane with it than without (profiles/summary_fwd_assist.txt): those keep the two-wave pipelined body
constexpr bool fwd_pipe_assist(bool open, bool ff, int cost, bool box) {
  if (open || box) return true;
  return ff ? cost != 3 && cost != 6 && cost != 7 : cost != 3 && cost != 10;
}

#ifdef FWD_STAMPS
__device__ unsigned long long g_fwd_stamps[36];   // the leading wave's phases | the pipelined form's helper wave's | its assistant wave's
#endif

// OPEN: the open-loop rollout of make_trajectory (ddp.hpp:392-415) on the same machinery: one candidate, u = U as given, x to X
// FF: free-flyer root (nq = nv + 1): x_new (-) x_old and q (+) dt v go through SE(3) for the root (lie.h), the dynamics through
// rbd::aba_tree_coop2w's free-flyer form
// TRACK: the tracking cost (DDP_HIP_FLAG_TRACKING_COST) of an unconstrained problem, formed inline by the 16 lanes of a candidate
// (track_lanes_sum); an instantiation of its own, so that the kernel without it is the one it was
// COST: bit 0 the tracking terms (TRACK above), bit 1 the frame terms (DDP_HIP_FLAG_FRAME_COST: frame_lanes_sum), bit 2 the
// state-limit terms (DDP_HIP_FLAG_STATE_LIMITS: limit_lanes_sum, added after the other two), bit 3 the frame-orientation terms
// (DDP_HIP_FLAG_FRAME_ORIENT_COST: frame_orient_lanes_sum in the place of frame_lanes_sum; it implies bit 1), each combination an
// instantiation of its own as well
// BOX: control bounds (DDP_HIP_FLAG_CONTROL_BOUNDS): u is clamped to [lo_t, hi_t] after the control update; lo_t, hi_t ride in the
// prefetch beside k_t.  Closed loop only, an instantiation of its own as well
// PIPE: the pipelined form ("Forward"): q_{t+1} = q_t (+) dt v_t needs no dynamics, so the second wave forms
// it at the start of step t and runs the q-part of step t + 1's traversal (rbd::aba_pipe_q: placements, inertia sums, U, 1/D, Ia,
// X^T Ia X) into the record buffer (t + 1) & 1 while the leading wave runs step t's x-part (rbd::aba_pipe_x) on buffer t & 1; the
// two meet at ONE workgroup barrier per step.  Two candidates per workgroup (FwdPipeLds), grid = instances x ceil(n_alpha / 2).
// Iteration t = -1 is the prologue: the helper forms the q-part of step 0, the other waves wait.  A third wave, the assistant,
// takes everything of step t that needs x_t but not the dynamics: dx, K_t dx, u_t (to LDS, to fw_u), the inline cost terms and
// their sum, the prefetch of step t + 1's operands and their parking.  Pass 1 of the x-part reads no control, so the leading wave
// starts it right after the barrier and waits for u_t only between pass 1 and pass 2 (S.u_step: rbd::lds_post / lds_await; the
// assistant never waits on the leading wave ahead of its post).  K_t, k_t, u_old, x_old, lo_t, hi_t in LDS are the assistant's
// alone.  Every early return above the loop is workgroup-uniform and all three waves run T + 1 iterations with one barrier each,
// whatever `live` is.  (ASSIST: where fwd_pipe_assist says no, wave 0 keeps those parts ahead of pass 1 and there is no third wave)
template <int NJ, bool OPEN = false, bool FF = false, int COST = 0, bool BOX = false, bool PIPE = false>
__global__ __launch_bounds__(PIPE && fwd_pipe_assist(OPEN, FF, COST, BOX) ? 192 : 128) void forward_kernel_lat2(FwdParams p) {
  static_assert(!(OPEN && BOX), "the open-loop rollout applies U as given");
  constexpr bool TRACK = (COST & 1) != 0, FRAME = (COST & 2) != 0, LIMIT = (COST & 4) != 0, ORIENT = (COST & 8) != 0;
  static_assert(!ORIENT || FRAME, "the orientation terms are of the cost frames: bit 3 implies bit 1");
  using L = typename std::conditional<PIPE, typename std::conditional<BOX, FwdPipeLdsBox<NJ>, FwdPipeLds<NJ>>::type,
                                      typename std::conditional<BOX, FwdLat2LdsBox<NJ>, FwdLat2Lds<NJ>>::type>::type;
  constexpr int NC = L::NC, NH = L::NH;
  constexpr int n = 2 * NJ, nq = FF ? NJ + 1 : NJ, nx = nq + NJ, nu = NJ, XS = L::n;   // XS: stride of a candidate's state in LDS
  constexpr int K2 = nu * n / 2, KR = (K2 + 63) / 64;        // K_t as 16-byte words; words per lane
  static_assert((nu * n) % 2 == 0, "K_t is moved in 16-byte words");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  L& S = *reinterpret_cast<L*>(lds);
  const int na = OPEN ? 1 : p.n_alpha;
  const int groups = PIPE ? (na + NC - 1) / NC : 2;   // workgroups per instance
  const int b = OPEN ? blockIdx.x : blockIdx.x / groups, half = OPEN ? 0 : blockIdx.x % groups;
  if (!OPEN && p.state[b] != 0) return;
  if (half * NC >= na) return;
  // two waves: wave 0 runs the rollout, wave 1 joins it for the inertia half of the leaf -> root pass (rbd::aba_tree_coop2w), or
  // runs one step ahead of it (PIPE); ASSIST: wave 2, the assistant, forms the controls, the cost and the prefetch beside wave 0
  constexpr bool ASSIST = PIPE && fwd_pipe_assist(OPEN, FF, COST, BOX);
  constexpr int CTRL = ASSIST ? 2 : 0;               // the wave that owns u_t, dsum and request / park
  const int wave = threadIdx.x / 64, tid = threadIdx.x % 64, al0 = tid / NH, h = tid % NH;
  const int al = al0 < NC ? al0 : NC - 1;            // (PIPE: the upper lanes of a wave have no candidate; they stay inside the arrays)
  const int a = half * NC + al;
  const int cand = p.round * na + a;
  const bool mine = al0 < NC && a < na;
  const bool live = mine && cand <= 33;              // 2^-34 < 1e-10: never tried (ddp_fwd.ipp:35-37)
  if (!OPEN && mine && cand > 33 && h == 0 && wave == CTRL) p.fw_dcost[(int64_t)b * na + a] = INFINITY;
  const double step = ldexp(1.0, -cand);
  const int64_t T = p.d.T;
  const double* xo = p.x_old + (int64_t)b * (T + 1) * nx;
  const double* uo = p.u_old + (int64_t)b * T * nu;
  double* xw = OPEN ? const_cast<double*>(p.x_old) + (int64_t)b * (T + 1) * nx : p.fw_x + ((int64_t)b * na + (a < na ? a : 0)) * (T + 1) * nx;
  double* uw = OPEN ? nullptr : p.fw_u + ((int64_t)b * na + (a < na ? a : 0)) * T * nu;
  const double* cold = p.costs_old + (int64_t)b * (T + 1);
  const double* kg = p.fb_val + (int64_t)b * T * nu;
  const double* Kg = p.fb_jac + (int64_t)b * T * nu * n;
  double* dx = S.dx + al * XS;
  double* x = S.x + al * XS;
  double* u = S.u + al * nu;
  double* qdd = S.qdd + al * nu;
  if (wave == 0) {
    const DevModel& m = *p.model;
    rbd::CoopModel<NJ>& cm = S.model;
    for (int i = tid; i < NJ; i += 64) {
      for (int k2 = 0; k2 < 21; ++k2) cm.I6[i][k2] = m.I6[i][k2];
      for (int k2 = 0; k2 < 9; ++k2) cm.Rp[i][k2] = m.Rp[i][k2];
      for (int k2 = 0; k2 < 3; ++k2) { cm.axis[i][k2] = m.axis[i][k2]; cm.pp[i][k2] = m.pp[i][k2]; }
      cm.armature[i] = m.armature[i];
      cm.parent[i] = m.parent[i]; cm.jtype[i] = m.jtype[i];
      cm.lvl_joint[i] = m.lvl_joint[i]; cm.child_list[i] = m.child_list[i];
      cm.lvl_start[i] = m.lvl_start[i]; cm.child_start[i] = m.child_start[i];
    }
    if (tid == 0) {
      cm.lvl_start[NJ] = m.lvl_start[NJ]; cm.child_start[NJ] = m.child_start[NJ];
      cm.n_levels = m.n_levels; cm.nv = m.nv; cm.nj = m.nj;
      cm.gravity[0] = m.gravity[0]; cm.gravity[1] = m.gravity[1]; cm.gravity[2] = m.gravity[2];
      cm.dt = m.dt; cm.c = m.c;
    }
    // the role words (rbd::coop_role): lane (L, hh) of the wave takes level L's hh-th joint straight from the global tables
    for (int e = tid; e < 16 * NH; e += 64) {
      const int L = e / NH, hh = e % NH;
      unsigned long long r = 255;
      if (L < m.n_levels && m.lvl_start[L] + hh < m.lvl_start[L + 1]) {
        const int j = m.lvl_joint[m.lvl_start[L] + hh];
        int ch[rbd::ROLE_MAX_CHILDREN] = {0, 0, 0};
        const int nch = m.child_start[j + 1] - m.child_start[j];
        for (int c = 0; c < nch && c < rbd::ROLE_MAX_CHILDREN; ++c) ch[c] = m.child_list[m.child_start[j] + c];
        r = rbd::coop_role(j, m.parent[j], m.jtype[j] == DDP_HIP_JOINT_REVOLUTE, nch, ch);
      }
      cm.role[e] = r;
    }
  }
  typedef double d2 __attribute__((ext_vector_type(2)));
  d2 Kreg[KR];
  double kreg = 0.0, uoreg = 0.0, xoreg0 = 0.0, xoreg1 = 0.0, coldreg = 0.0;
  [[maybe_unused]] double loreg = 0.0, hireg = 0.0;
  auto request = [&](int64_t t) {                    // step t's operands: K_t, k_t, u_old,t, x_old,t, the old cost term
    const int iu = tid < nu ? tid : nu - 1;
    uoreg = uo[t * nu + iu];
    if constexpr (!OPEN) {
      const d2* Kt = reinterpret_cast<const d2*>(Kg + t * nu * n);
#pragma unroll
      for (int j = 0; j < KR; ++j) { const int e = j * 64 + tid; Kreg[j] = Kt[e < K2 ? e : K2 - 1]; }
      kreg = kg[t * nu + iu];
      if constexpr (BOX) { loreg = p.ctrl_lo[((int64_t)b * T + t) * nu + iu]; hireg = p.ctrl_hi[((int64_t)b * T + t) * nu + iu]; }
      xoreg0 = xo[t * nx + (tid < nx ? tid : nx - 1)];
      xoreg1 = xo[t * nx + (64 + tid < nx ? 64 + tid : nx - 1)];
      coldreg = cold[t];
    }
  };
  auto park = [&]() {
    if (tid < nu) S.uo[tid] = uoreg;
    if constexpr (!OPEN) {
      d2* Ks = reinterpret_cast<d2*>(S.K);
#pragma unroll
      for (int j = 0; j < KR; ++j) { const int e = j * 64 + tid; if (e < K2) Ks[e] = Kreg[j]; }
      if (tid < nu) S.k[tid] = kreg;
      if constexpr (BOX) { if (tid < nu) { S.lo[tid] = loreg; S.hi[tid] = hireg; } }
      if (tid < nx) S.xo[tid] = xoreg0;
      if (64 + tid < nx) S.xo[64 + tid] = xoreg1;
    }
  };
  static_assert(nx <= 128, "x_old is parked by two words per lane");
  // ASSIST: u_t is whole in S.u: the leading wave's pass 2 may start.  Every path of the control wave through step t posts once
  auto post_u = [&](int64_t t) { if constexpr (ASSIST) { if (tid == 0) rbd::lds_post(&S.u_step, (int)t); } };
  double cold_t = 0.0, dsum = 0.0;
  const double mc = p.model->c, mdt = p.model->dt;
  if (wave == CTRL) {
    request(0);
    const double* x0 = OPEN ? xw : p.x_new + (int64_t)b * (T + 1) * nx;   // x_new,0 is preset by the caller (ddp.hpp:752)
    if (live)
      for (int i = h; i < nx; i += NH) { const double v = x0[i]; x[i] = v; if (!OPEN) xw[i] = v; }
    park();
    cold_t = coldreg;
    if constexpr (ASSIST) { if (tid == 0) S.u_step = -1; }
  }
  rbd::wg_sync_lds();                              // the model tables are in LDS for all waves
  // one loop, one call site of the traversal for all waves (a second call site keeps the compiler from inlining it): the helper
  // waves skip the rollout's own parts and meet wave 0 at the traversal's workgroup barriers
  const bool lead = wave == 0, ctrl = wave == CTRL;
  rbd::FwdStamp* fs = nullptr;
#ifdef FWD_STAMPS
  rbd::FwdStamp fsv{};
  if (lead || PIPE) fs = &fsv;
  fsv.last = wall_clock64();
#endif
  for (int64_t t = PIPE ? -1 : 0; t < T; ++t) {
    if constexpr (PIPE) x = S.x + ((int)(t & 1) * NC + al) * XS;   // x_t; t = -1: the prologue
    if (ctrl && (!PIPE || t >= 0)) {
    if constexpr (OPEN) {
      if (live)
        for (int i = h; i < nu; i += NH) u[i] = S.uo[i];
      if constexpr (ASSIST) { rbd::coop_sync<true>(); post_u(t); }
    } else {
    if constexpr (FF) {
      if (live) {                                                              // :45 difference(out, old, new) on SE(3) x R^(nv-6) x R^nv
        if (h == 0) lie::se3_difference(S.xo, x, dx);
        for (int i = 6 + h; i < NJ; i += NH) dx[i] = x[i + 1] - S.xo[i + 1];
        for (int i = h; i < NJ; i += NH) dx[NJ + i] = x[nq + i] - S.xo[nq + i];
      }
    } else {
    if (live)
      for (int i = h; i < n; i += NH) dx[i] = x[i] - S.xo[i];                  // :45 difference(out, old, new)
    }
    rbd::coop_sync<true>();
    {
      constexpr int NR = (nu + NH - 1) / NH;
      double acc[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) acc[r] = 0.0;
      // fully unrolled: every LDS address is the lane's base plus an immediate (rolled, the loop spent 60 instructions per
      // column on address arithmetic for 3 multiply-adds)
      const double* Kr[NR];
#pragma unroll
      for (int r = 0; r < NR; ++r) { const int i = h + NH * r; Kr[r] = S.K + (i < nu ? i : nu - 1); }
#pragma unroll
      for (int l = 0; l < n; ++l) {
        const double d = dx[l];
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[r] += Kr[r][l * nu] * d;
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const int i = h + NH * r;
        if (i < nu && live) {
          double ui = S.uo[i] + step * S.k[i];                                  // :47-48
          ui += acc[r];                                                         // :49
          if constexpr (BOX) { const double lo = S.lo[i], hi = S.hi[i]; ui = ui < lo ? lo : (ui > hi ? hi : ui); }   // (a NaN stays a NaN)
          u[i] = ui;
          uw[t * nu + i] = ui;
        }
      }
    }
    rbd::coop_sync<true>();
    post_u(t);
    FSTAMP(fs, 0);
    double c_track = 0.0;
    if constexpr (TRACK) c_track = track_lanes_sum<FF>(p, b, t, x, u, h, live);
    if constexpr (FRAME && !ORIENT) c_track += frame_lanes_sum<FF>(p, S.model, b, t, x, h, live);
    if constexpr (ORIENT) c_track += frame_orient_lanes_sum<FF>(p, S.model, b, t, x, h, live);
    if constexpr (LIMIT) c_track += limit_lanes_sum<FF>(p, b, t, x, h, live);
    if (h == 0 && live && p.cost_inline) {
      double un = 0;
      for (int i = 0; i < nu; ++i) un += u[i] * u[i];
      double c_new = 0.5 * mc * un;                                             // problem_t::l (constrained problems: cand_cost_kernel)
      if constexpr (TRACK || FRAME || LIMIT) c_new += c_track;
      dsum += c_new - cold_t;
    }
    }
    rbd::coop_sync<true>();                          // K_t, k_t, ... have been read: their places are free for step t + 1
    FSTAMP(fs, 1);
    if (t + 1 < T) request(t + 1);
    FSTAMP(fs, 2);
    }
    if constexpr (PIPE) {
      double* xn = S.x + ((int)((t + 1) & 1) * NC + al) * XS;                    // x_{t+1}: q by the helper, v by the leading wave
      if (lead) {
        if (t >= 0) {
          rbd::aba_pipe_x<NJ, NC, NH, rbd::CoopModel<NJ>, FF>(S.model, S.rec[t & 1], x + nq, u, qdd, S.state, al, h, live, fs,
                                                              [&]() { if constexpr (ASSIST) rbd::lds_await(&S.u_step, (int)t); });   // :50
          if (live)
            for (int i = h; i < NJ; i += NH) {                                  // dynamics_t::eval_to, problem.hpp:441-461: the velocities
              const double vn = x[nq + i] + qdd[i] * mdt;
              xn[nq + i] = vn;
              xw[(t + 1) * nx + nq + i] = vn;
            }
          FSTAMP(fs, 7);
          if constexpr (!ASSIST) {
            if (t + 1 < T) { park(); cold_t = coldreg; }
            FSTAMP(fs, 8);
          }
        }
      } else if (ASSIST && ctrl) {
        if (t >= 0 && t + 1 < T) { park(); cold_t = coldreg; }   // this wave's own reads of step t are behind it
        FSTAMP(fs, 8);
      } else {
        if (t >= 0) {
          // ... the configuration: the one expression q_{t+1} comes from
          if constexpr (FF) {
            if (live && h == 0) {
              double dq[6], q7[7];
#pragma unroll
              for (int k = 0; k < 6; ++k) dq[k] = mdt * x[nq + k];
              lie::se3_integrate(x, dq, q7);
#pragma unroll
              for (int k = 0; k < 7; ++k) xn[k] = q7[k];
            }
            if (live)
              for (int i = 6 + h; i < NJ; i += NH) { const double vo = mdt * x[nq + i]; xn[i + 1] = x[i + 1] + vo; }
          } else {
            if (live)
              for (int i = h; i < NJ; i += NH) { const double vo = mdt * x[NJ + i]; xn[i] = x[i] + vo; }
          }
          rbd::coop_sync<true>();
          FSTAMP(fs, 0);
        }
        if (t + 1 < T) rbd::aba_pipe_q<NJ, NC, NH, rbd::CoopModel<NJ>, FF>(S.model, xn, S.rec[(t + 1) & 1], S.z, al, h, live, fs);
      }
      rbd::wg_sync_lds();                            // the step's one barrier: x_{t+1} and its record are whole
      FSTAMP(fs, wave == 1 ? 5 : 3);
      if (lead && t >= 0 && live)
        for (int i = h; i < nq; i += NH) xw[(t + 1) * nx + i] = xn[i];
      continue;
    }
    rbd::aba_tree_coop2w<NJ, NC, NH, rbd::CoopModel<NJ>, FF>(S.model, x, x + nq, u, qdd, S.state, al, h, live, wave, fs);   // :50
    if (!lead) continue;
    if constexpr (FF) {
      // dynamics_t::eval_to on the group (problem.hpp:441-461, rbd::eval_f's free-flyer branch): the root's pose by one lane,
      // ahead of the velocity updates it reads
      double q7[7];
      if (live && h == 0) {
        double dq[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) dq[k] = mdt * x[nq + k];
        lie::se3_integrate(x, dq, q7);
      }
      rbd::coop_sync<true>();
      if (live) {
        for (int i = 6 + h; i < NJ; i += NH) { const double vo = mdt * x[nq + i]; const double qn = x[i + 1] + vo; x[i + 1] = qn; xw[(t + 1) * nx + i + 1] = qn; }
        for (int i = h; i < NJ; i += NH) { const double vn = x[nq + i] + qdd[i] * mdt; x[nq + i] = vn; xw[(t + 1) * nx + nq + i] = vn; }
        if (h == 0) {
#pragma unroll
          for (int k = 0; k < 7; ++k) { x[k] = q7[k]; xw[(t + 1) * nx + k] = q7[k]; }
        }
      }
    } else {
    if (live)
      for (int i = h; i < NJ; i += NH) {                                        // dynamics_t::eval_to, problem.hpp:441-461
        const double vo = mdt * x[NJ + i];
        const double qn = x[i] + vo;
        const double vn = x[NJ + i] + qdd[i] * mdt;
        x[i] = qn; x[NJ + i] = vn;
        xw[(t + 1) * nx + i] = qn; xw[(t + 1) * nx + NJ + i] = vn;
      }
    }
    FSTAMP(fs, 7);
    if (t + 1 < T) { park(); cold_t = coldreg; }
    rbd::coop_sync<true>();
    FSTAMP(fs, 8);
  }
#ifdef FWD_STAMPS
  if (tid == 0 && blockIdx.x == 0)
    for (int i = 0; i < 12; ++i) g_fwd_stamps[12 * wave + i] = PIPE || lead ? fsv.acc[i] : 0;
#endif
  if constexpr (PIPE) x = S.x + ((int)(T & 1) * NC + al) * XS;                   // x_T
  double c_term = 0.0;
  if constexpr (TRACK) { if (ctrl) c_term = track_lanes_sum<FF>(p, b, T, x, u, h, live); }
  if constexpr (FRAME && !ORIENT) { if (ctrl) c_term += frame_lanes_sum<FF>(p, S.model, b, T, x, h, live); }
  if constexpr (ORIENT) { if (ctrl) c_term += frame_orient_lanes_sum<FF>(p, S.model, b, T, x, h, live); }
  if constexpr (LIMIT) { if (ctrl) c_term += limit_lanes_sum<FF>(p, b, T, x, h, live); }
  if (!OPEN && h == 0 && live && ctrl && p.cost_inline) {
    dsum += c_term - cold[T];
    p.fw_dcost[(int64_t)b * na + a] = dsum;
  }
}

// Constrained problems on the latency path.  Only the rollout is sequential in t; the cost terms of a rolled-out
// candidate (cost_seq_aug, ddp.hpp:699-735: l + pe . ce + mu/2 |ce|^2, with ce_t = eq(t, x_t, u_t) two look-ahead dynamics steps
// away, problem.hpp:563-567; lf at t = T) are independent across t: one lane per (instance, candidate, t), t = 0 .. T ...
template <int NJ, int FRAME = 0, bool LIMIT = false>
__global__ void cand_cost_kernel(FwdParams p) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t T = p.d.T;
  const int na = p.n_alpha;
  if (gid >= p.d.batch * na * (T + 1)) return;
  const int64_t t = gid % (T + 1);
  const int a = (int)((gid / (T + 1)) % na);
  const int b = (int)(gid / ((T + 1) * na));
  if (p.state[b] != 0 || p.round * na + a > 33) return;
  const DevModel& m = *p.model;
  const int nx = m.nq + m.nv, nu = m.nv;
  const double* xs = p.fw_x + (((int64_t)b * na + a) * (T + 1) + t) * nx;
  double x[2 * NJ + 1], u[NJ];
  for (int i = 0; i < nx; ++i) x[i] = xs[i];
  double* out = p.fw_cost + ((int64_t)b * na + a) * (T + 1) + t;
  if (t == T) { *out = terminal_cost<FRAME, LIMIT>(p, m, b, x); return; }
  const double* us = p.fw_u + (((int64_t)b * na + a) * T + t) * nu;
  for (int i = 0; i < nu; ++i) u[i] = us[i];
  *out = stage_cost<NJ, FRAME, LIMIT>(p, m, b, t, x, u, p.mu[b]);
}
// ... and one lane per (instance, candidate) adds the differences up in the order of forward_kernel (ddp_fwd.ipp:54-56)
__global__ void cand_sum_kernel(FwdParams p) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int na = p.n_alpha;
  if (gid >= p.d.batch * na) return;
  const int b = gid / na, a = gid % na;
  if (p.state[b] != 0 || p.round * na + a > 33) return;
  const int64_t T = p.d.T;
  const double* cold = p.costs_old + (int64_t)b * (T + 1);
  const double* cnew = p.fw_cost + ((int64_t)b * na + a) * (T + 1);
  double dsum = 0.0;
  for (int64_t t = 0; t < T; ++t) dsum += cnew[t] - cold[t];
  dsum += cnew[T] - cold[T];
  p.fw_dcost[(int64_t)b * na + a] = dsum;
}

// The add-on cost kernels below (CoM, frame velocities, momentum, balance regions, relative frames, control-gravity, frame aiming, joint accelerations, obstacles, self-collision, capsules) run over a list of `count` (trajectory, t) pairs, t = 0 .. T,
// `na` trajectories per instance.  Pair e: which trajectory, which t, whose instance, which block bt1 = b (T+1) + t of the term's
// data.  skip: nothing is written for this pair (past the list, or a candidate the rollout kernels skip: state != 0, beyond
// 2^-33; state == nullptr: a resident trajectory, none is skipped).  live: the pair is evaluated (the kernels narrow it further)
struct CostPair {
  int64_t traj, b, bt1;
  int t;
  bool skip, live;
};
__device__ __forceinline__ CostPair cost_pair_decode(int64_t e, int64_t count, int32_t T1, int32_t na, const int32_t* state, int32_t round) {
  CostPair p{0, 0, 0, 0, true, e < count};
  if (p.live) {
    p.traj = e / T1;
    p.t = (int)(e % T1);
    p.b = p.traj / na;
    if (state && (state[p.b] != 0 || round * na + (int)(p.traj % na) > 33)) p.live = false;
    p.bt1 = p.b * T1 + p.t;
  }
  p.skip = !p.live;
  return p;
}
// ... and what a pair's first lane leaves: add != 0: out[e] += sum, if some term was formed (COSTS_OLD / COSTS_NEW behind
// cost_kernel: x + 0 is x but for x = -0); add == 0: out[e] = sum (the candidates' array of a line-search round)
__device__ __forceinline__ void cost_pair_store(double* out, int64_t e, double sum, bool any, int32_t add) {
  if (add) { if (any) out[e] += sum; }
  else out[e] = sum;
}
// The value kernels with L lanes per pair (64 / L pairs per wave) share this body: decode the pair; lane k < n of the group forms
// one term, form(k, bt1, x, &term) -> formed (x: the pair's state), and leaves term and flag in LDS (s_term, s_formed: 64 entries
// each, the kernel's own); the group's first lane folds the n terms in ascending order -- the sum of the formed ones, or with MIN
// the rbd::obstacle_min of them all from +inf (no flags: s_formed may be null) -- and cost_pair_store writes the result
template <int L, bool MIN, class Form>
__device__ __forceinline__ void pair_lanes_fold(double* s_term, int32_t* s_formed, int n, const double* xs, int64_t traj_stride, int64_t count,
                                                int32_t T1, int32_t nx, int32_t na, const int32_t* state, int32_t round, double* out, int32_t add,
                                                Form form) {
  const int tid = threadIdx.x, g = tid / L, k = tid % L;
  const int64_t e = (int64_t)blockIdx.x * (64 / L) + g;
  const CostPair pr = cost_pair_decode(e, count, T1, na, state, round);
  double term = MIN ? INFINITY : 0.0;
  bool formed = false;
  if (pr.live && k < n) formed = form(k, pr.bt1, xs + pr.traj * traj_stride + (int64_t)pr.t * nx, &term);
  s_term[tid] = term;
  if (!MIN) s_formed[tid] = formed ? 1 : 0;
  __syncthreads();
  if (k != 0 || pr.skip) return;
  double acc = MIN ? INFINITY : 0.0;
  bool any = false;
  for (int i = 0; i < n; ++i) {
    if (MIN) acc = rbd::obstacle_min(acc, s_term[tid + i]);
    else if (s_formed[tid + i]) { acc += s_term[tid + i]; any = true; }
  }
  cost_pair_store(out, e, acc, any, add);
}

// The centre-of-mass terms (DDP_HIP_FLAG_COM_COST, ddp_hip.h) of a list of states, in kernels of their own that add onto what the
// kernels above leave (none of them knows the term).  The list: `count` (trajectory, t) pairs, t = 0 .. T, trajectory k's states
// at xs + k traj_stride, `na` trajectories per instance (1: a resident trajectory, n_alpha: the candidates of fw_x).  `lpe` lanes
// (a power of two >= the joint count) cooperate on one evaluation, 64 / lpe evaluations per wave: lane j walks joint j's path
// with its body's CoM alone (rbd::com_body_point: no per-joint arrays, no scratch) and leaves m_j p_j in LDS, the group's first
// lane adds them up in ascending order (rbd::com_fold) and forms 1/2 sum_a w_a (c_a - g_a)^2.  A term of weight 0 is left out,
// and with all three of them the walk: such a pair adds nothing (add != 0) or stores +0 (add == 0).  add != 0: out[pair] +=
// term (COSTS_OLD / COSTS_NEW behind cost_kernel); add == 0: out[pair] = term (the term's candidates' array in a line-search
// round), and the candidates the rollout kernels skip (state != 0, beyond 2^-33) are skipped here.  A non-finite state gives a
// NaN term, as frame_cost_sum does: the candidate's sum is NaN and select_kernel's `<= 0` does not accept it
__global__ __launch_bounds__(64) void com_cost_kernel(CoMCostDev cm, const DevModel* model, const double* xs, int64_t traj_stride,
                                                      int64_t count, int32_t T1, int32_t nx, int32_t na, int32_t lpe, const int32_t* state,
                                                      int32_t round, double* out, int32_t add) {
  __shared__ double s_m[64], s_mp[64 * 3];
  const DevModel& m = *model;
  const int tid = threadIdx.x, g = tid / lpe, j = tid % lpe;
  const int64_t e = (int64_t)blockIdx.x * (64 / lpe) + g;
  const CostPair pr = cost_pair_decode(e, count, T1, na, state, round);
  const int64_t traj = pr.traj, bt1 = pr.bt1;
  const int t = pr.t;
  const bool skip = pr.skip;
  bool live = pr.live;
  if (live && !rbd::frame_weights_any(cm.weight + bt1 * 3)) live = false;
  if (live && j < m.nj) s_m[tid] = rbd::com_body_point(m, m.ff != 0, j, xs + traj * traj_stride + (int64_t)t * nx, s_mp + 3 * tid);
  __syncthreads();
  if (j != 0 || skip) return;
  double term = 0.0;
  if (live) {
    const double* w = cm.weight + bt1 * 3;
    const double* gt = cm.target + bt1 * 3;
    double c[3], s = 0.0;
    rbd::com_fold(s_m + tid, s_mp + 3 * tid, m.nj, c);
    for (int a = 0; a < 3; ++a) { const double r = c[a] - gt[a]; if (w[a] != 0.0) s += w[a] * r * r; }
    term = 0.5 * s;
  }
  cost_pair_store(out, e, term, live, add);
}
// ... and one lane per (instance, candidate) adds a candidate's terms up in ascending t and adds the sum once onto what the
// rollout path left in fw_dcost (sum_t (new term without this one - COSTS_OLD[t]): COSTS_OLD holds the old trajectory's terms
// already), before select_kernel reads it.  A sum of +0 (an instance without weights) is not added: its -0 stays -0.  Named for
// its first user: it sums any add-on term's candidates (CostBlock::cand), once per live term and round
__global__ void com_sum_kernel(const double* cand, double* fw_dcost, const int32_t* state, int32_t batch, int32_t na, int32_t round, int64_t T) {
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= batch * na) return;
  const int b = gid / na, a = gid % na;
  if (state[b] != 0 || round * na + a > 33) return;                  // (beyond 2^-33 the INFINITY stays)
  const double* c = cand + (int64_t)gid * (T + 1);
  double s = 0.0;
  for (int64_t t = 0; t <= T; ++t) s += c[t];
  if (s != 0.0) fw_dcost[gid] += s;
}

// The frame-velocity terms (DDP_HIP_FLAG_FRAME_VEL_COST, ddp_hip.h) of a list of states, added on top like the CoM terms above:
// the same list (`count` (trajectory, t) pairs, trajectory k's states at xs + k traj_stride, `na` trajectories per instance), the
// same two uses (add != 0: out[pair] += term behind cost_kernel; add == 0: out[pair] = term, its candidates' array in a line-search
// round, with the candidates the rollout kernels skip skipped here).  DDP_HIP_MAX_COST_FRAMES lanes per pair, 16 pairs per wave: lane f walks
// frame f's path once, joint -> root, carrying the point, its velocity and the angular velocity (rbd::frame_velocity: no
// jacobian, no per-joint arrays), and leaves 1/2 sum_a w_a r_a^2 in LDS; the group's first lane adds the frames' terms in
// ascending order.  A term of weight 0 is left out, a frame whose six weights are 0 is not walked, and a pair without a live
// weight adds nothing (add != 0) or stores +0 (add == 0).  A non-finite state gives a NaN term, as com_cost_kernel's does
__global__ __launch_bounds__(64) void frame_vel_cost_kernel(FrameVelCostDev fv, const DevModel* model, const double* xs, int64_t traj_stride,
                                                            int64_t count, int32_t T1, int32_t nx, int32_t na, const int32_t* state,
                                                            int32_t round, double* out, int32_t add) {
  __shared__ double s_term[64];
  __shared__ int32_t s_walked[64];
  const DevModel& m = *model;
  pair_lanes_fold<DDP_HIP_MAX_COST_FRAMES, false>(s_term, s_walked, fv.nf, xs, traj_stride, count, T1, nx, na, state, round, out, add,
                                                  [&](int f, int64_t bt1, const double* x, double* term) {
    const double* w = fv.weight + (bt1 * fv.nf + f) * 6;
    const bool lin = rbd::frame_weights_any(w), ang = rbd::frame_weights_any(w + 3);
    if (!lin && !ang) return false;
    double pd[3] = {0.0, 0.0, 0.0}, om[3] = {0.0, 0.0, 0.0};
    rbd::frame_velocity(m, fv.joint[f], fv.off[f], x, x + m.nq, lin, ang, pd, om);
    *term = rbd::frame_vel_term(w, fv.target + (bt1 * fv.nf + f) * 6, pd, om);
    return true;
  });
}

// The centroidal-momentum terms (DDP_HIP_FLAG_MOMENTUM_COST, ddp_hip.h) of a list of states, added on top like the CoM terms above:
// the same list, the same two uses, the same `lpe` lanes per evaluation.  Lane j walks joint j's path once with its body alone
// (rbd::momentum_body: no jacobian, no per-joint arrays) and leaves m_j, m_j p_j, m_j pdot_j and its angular momentum about the
// world origin in LDS; the group's first lane adds them up in ascending order, shifts the angular part to the CoM
// (rbd::momentum_fold) and forms 1/2 sum_a w_a (h_a - g_a)^2.  A term of weight 0 is left out, with the three angular weights 0
// no inertia and no angular momentum is formed, and with all six the walk is left out: such a pair adds nothing (add != 0) or
// stores +0 (add == 0).  A non-finite state gives a NaN term, as com_cost_kernel's does
__global__ __launch_bounds__(64) void momentum_cost_kernel(MomentumCostDev mo, const DevModel* model, const double* xs, int64_t traj_stride,
                                                           int64_t count, int32_t T1, int32_t nx, int32_t na, int32_t lpe, const int32_t* state,
                                                           int32_t round, double* out, int32_t add) {
  __shared__ double s_rec[64 * 10];
  const DevModel& m = *model;
  const int tid = threadIdx.x, g = tid / lpe, j = tid % lpe;
  const int64_t e = (int64_t)blockIdx.x * (64 / lpe) + g;
  const CostPair pr = cost_pair_decode(e, count, T1, na, state, round);
  const double* w = mo.weight + pr.bt1 * 6;
  bool live = pr.live, ang = false;
  if (live && !rbd::weights_any(w, 6)) live = false;
  if (live) ang = rbd::frame_weights_any(w + 3);
  if (live && j < m.nj) {
    const double* x = xs + pr.traj * traj_stride + (int64_t)pr.t * nx;
    double* r = s_rec + 10 * tid;
    r[7] = r[8] = r[9] = 0.0;
    r[0] = rbd::momentum_body(m, j, x, x + m.nq, ang, r + 1, r + 4, r + 7);
  }
  __syncthreads();
  if (j != 0 || pr.skip) return;
  double term = 0.0;
  if (live) {
    double h[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    rbd::momentum_fold(s_rec + 10 * tid, m.nj, ang, h);
    term = rbd::frame_vel_term(w, mo.target + pr.bt1 * 6, h, h + 3);
  }
  cost_pair_store(out, e, term, live, add);
}

// The balance-region terms (DDP_HIP_FLAG_BALANCE_REGION_COST, ddp_hip.h) of a list of states, added on top like the momentum terms
// above: the same list, the same two uses, the same `lpe` lanes per evaluation.  Lane j walks joint j's path once with its body
// alone (rbd::momentum_body with ang = false: no inertia, no jacobian, no per-joint arrays) and leaves m_j, m_j p_j and m_j pdot_j
// in LDS; the group's first lane folds c in ascending order -- and cdot where a live plane of the row has tau != 0, else the
// rates are not summed (rbd::region_fold) -- and runs over the planes in ascending order.  A plane with w == 0 or e == 0 is left
// out, a state whose weights are all 0 is not walked, and a state without an active plane adds nothing (add != 0) or stores +0
// (add == 0).  A non-finite state gives a NaN term, as com_cost_kernel's does.  MARGIN (ddp_hip_balance_region_margin): over the
// (instance, t) pairs of one resident trajectory, min instead of sum: out[pair] = min over the planes with w != 0 of d_o, +inf
// where none is live, NaN where a d is
template <bool MARGIN>
__device__ __forceinline__ void balance_region_pairs(const BalanceRegionDev& br, const DevModel& m, double* s_rec, const double* xs,
                                                     int64_t traj_stride, int64_t count, int32_t T1, int32_t nx, int32_t na, int32_t lpe,
                                                     const int32_t* state, int32_t round, double* out, int32_t add) {
  const int tid = threadIdx.x, g = tid / lpe, j = tid % lpe;
  const int64_t e = (int64_t)blockIdx.x * (64 / lpe) + g;
  const CostPair pr = cost_pair_decode(e, count, T1, na, state, round);
  const double* w = br.weight + pr.bt1 * br.np;
  const double* geom = br.geom + pr.bt1 * br.np * 5;
  const bool live = pr.live && rbd::weights_any(w, br.np);
  if (live && j < m.nj) {
    const double* x = xs + pr.traj * traj_stride + (int64_t)pr.t * nx;
    double* r = s_rec + 7 * tid;
    r[0] = rbd::momentum_body(m, j, x, x + m.nq, false, r + 1, r + 4, nullptr);
  }
  __syncthreads();
  if (j != 0 || pr.skip) return;
  double acc = MARGIN ? INFINITY : 0.0;
  bool any = false;
  if (live) {
    double c[3], cd[3] = {0.0, 0.0, 0.0};
    rbd::region_fold(s_rec + 7 * tid, m.nj, rbd::region_needs_rate(geom, w, br.np), c, cd);
    for (int o = 0; o < br.np; ++o) {
      const double wo = w[o];
      if (wo == 0.0) continue;
      const double d = rbd::region_distance(geom + 5 * o, c, cd);
      if (MARGIN) acc = rbd::obstacle_min(acc, d);
      else if (rbd::obstacle_active(d)) { acc += wo * d * d; any = true; }
    }
  }
  cost_pair_store(out, e, MARGIN ? acc : 0.5 * acc, any, add);
}
__global__ __launch_bounds__(64) void balance_region_cost_kernel(BalanceRegionDev br, const DevModel* model, const double* xs, int64_t traj_stride,
                                                                 int64_t count, int32_t T1, int32_t nx, int32_t na, int32_t lpe,
                                                                 const int32_t* state, int32_t round, double* out, int32_t add) {
  __shared__ double s_rec[64 * 7];
  balance_region_pairs<false>(br, *model, s_rec, xs, traj_stride, count, T1, nx, na, lpe, state, round, out, add);
}
__global__ __launch_bounds__(64) void balance_region_margin_kernel(BalanceRegionDev br, const DevModel* model, const double* xs, int64_t count,
                                                                   int32_t nx, int32_t lpe, double* out) {
  __shared__ double s_rec[64 * 7];
  balance_region_pairs<true>(br, *model, s_rec, xs, nx, count, 1, nx, 1, lpe, nullptr, 0, out, 0);
}

// The relative-frame terms (DDP_HIP_FLAG_RELATIVE_FRAME_COST, ddp_hip.h) of a list of states, added on top like the frame-velocity
// terms above: the same list, the same two uses (add != 0: out[pair] += term behind cost_kernel; add == 0: out[pair] = term, its
// candidates' array in a line-search round, with the candidates the rollout kernels skip skipped here).  DDP_HIP_MAX_FRAME_PAIRS
// lanes per state, 16 states per wave: lane i walks frame pair i (rbd::relative_placement: two walks joint -> root, no jacobian, no
// per-joint arrays) and leaves 1/2 sum_a w_a r_a^2 in LDS; the group's first lane adds the pairs' terms in ascending order.  A term
// of weight 0 is left out, a pair whose six weights are 0 is not walked, one whose rotation (position) weights are 0 reads no
// quaternion and forms no log (reads no target), and a state without a live weight adds nothing (add != 0) or stores +0
// (add == 0).  A non-finite state gives a NaN term, as com_cost_kernel's does
__global__ __launch_bounds__(64) void relative_frame_cost_kernel(RelativeFrameDev rf, const DevModel* model, const double* xs, int64_t traj_stride,
                                                                 int64_t count, int32_t T1, int32_t nx, int32_t na, const int32_t* state,
                                                                 int32_t round, double* out, int32_t add) {
  __shared__ double s_term[64];
  __shared__ int32_t s_walked[64];
  const DevModel& m = *model;
  pair_lanes_fold<DDP_HIP_MAX_FRAME_PAIRS, false>(s_term, s_walked, rf.np, xs, traj_stride, count, T1, nx, na, state, round, out, add,
                                                  [&](int i, int64_t bt1, const double* x, double* term) {
    if (!rbd::weights_any(rf.weight + (bt1 * rf.np + i) * 6, 6)) return false;
    *term = rbd::relative_frame_term(m, rf, i, bt1, x);
    return true;
  });
}

// ddp_hip_relative_frame_error: one lane per (instance, t, pair) of one resident trajectory, out[(bt1 np + i) 6 ..] = the unweighted
// residual r = (r_pos, e_rot) of pair i against the resident target and reference, whatever the weights
__global__ __launch_bounds__(64) void relative_frame_error_kernel(RelativeFrameDev rf, const DevModel* model, const double* xs, int64_t count,
                                                                  int32_t nx, double* out) {
  const int64_t e = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (e >= count * rf.np) return;
  const int64_t bt1 = e / rf.np;
  const int i = (int)(e % rf.np);
  const DevModel& m = *model;
  rbd::RelativePlacement P;
  rbd::relative_placement(m, m.ff != 0, rf.ja[i], rf.offa[i], rf.jb[i], rf.offb[i], xs + bt1 * nx, true, P);
  rbd::relative_frame_residual(P, rf.target + e * 3, rf.quat + e * 4, out + e * 6);
}

// The control-gravity terms (DDP_HIP_FLAG_CONTROL_GRAV_COST, ddp_hip.h) of a list of states and their controls, added on top like
// the CoM terms above: the same list, the same two uses (add != 0: out[pair] += term behind cost_kernel; add == 0: out[pair] = term,
// its candidates' array in a line-search round, with the candidates the rollout kernels skip skipped here).  us: the controls that
// belong to xs, trajectory k's at us + k u_stride (U, U_NEW, or the candidates' fw_u: the controls the rollout applied, clamped
// where there are bounds).  `lpe` lanes (a power of two >= the joint count) cooperate on one evaluation, 64 / lpe per wave: lane
// j walks joint j's path once with its axis, its origin and its body's first moment (rbd::grav_value_stage: no jacobian, no
// scratch) and leaves mass, m_j p_j and the path in LDS; after the barrier lane j forms the sums of its subtree over the records in
// ascending order, g_j, and w_j r_j^2 with r_j = u_j - g_j - o_j; the group's first lane adds the rows' terms in ascending order.
// A term of weight 0 is left out (a free-flyer root's six rows always), and with all m of them the walk; t = T has no control and
// no term: such a pair adds nothing (add != 0) or stores +0 (add == 0).  A non-finite state gives a NaN term, as com_cost_kernel's does
__global__ __launch_bounds__(64) void control_grav_cost_kernel(ControlGravDev cg, const DevModel* model, const double* xs, int64_t traj_stride,
                                                               int64_t count, int32_t T1, int32_t nx, int32_t na, int32_t lpe, const double* us,
                                                               int64_t u_stride, const int32_t* state, int32_t round, double* out, int32_t add) {
  __shared__ double s_m[64], s_mp[64 * 3], s_term[64];
  __shared__ unsigned long long s_mask[64];
  __shared__ int32_t s_formed[64];
  const DevModel& m = *model;
  const bool ff = m.ff != 0;
  const int tid = threadIdx.x, g = tid / lpe, j = tid % lpe, base = tid - j, mu = m.nv;
  const int64_t e = (int64_t)blockIdx.x * (64 / lpe) + g;
  const CostPair pr = cost_pair_decode(e, count, T1, na, state, round);
  const int t = pr.t, T = T1 - 1;
  const int64_t bt = pr.b * T + t;                       // the record's rows are t < T
  bool live = pr.live && t < T;
  if (live && !rbd::weights_any(cg.weight + bt * mu, mu)) live = false;
  rbd::GravLane own;
  if (live && j < m.nj)
    rbd::grav_value_stage(m, ff, j, xs + pr.traj * traj_stride + (int64_t)t * nx, s_m + tid, s_mp + 3 * tid, s_mask + tid, own);
  __syncthreads();
  double term = 0.0;
  bool formed = false;
  if (live && j < m.nj && !(ff && j == 0)) {
    const int i = ff ? j + 5 : j;                        // the control row of joint j
    const double wi = cg.weight[bt * mu + i];
    if (wi != 0.0) {
      const double r = us[pr.traj * u_stride + (int64_t)t * mu + i] - rbd::grav_value_joint(m, j, s_m + base, s_mp + 3 * base, s_mask + base, own) -
                       cg.offset[bt * mu + i];
      term = wi * r * r;
      formed = true;
    }
  }
  s_term[tid] = term;
  s_formed[tid] = formed ? 1 : 0;
  __syncthreads();
  if (j != 0 || pr.skip) return;
  double acc = 0.0;
  for (int i = 0; i < m.nj; ++i)
    if (s_formed[tid + i]) acc += s_term[tid + i];
  cost_pair_store(out, e, 0.5 * acc, live, add);
}

// The frame-aiming terms (DDP_HIP_FLAG_FRAME_AIM_COST, ddp_hip.h) of a list of states, added on top like the frame-velocity terms
// above: the same list, the same two uses (add != 0: out[pair] += term behind cost_kernel; add == 0: out[pair] = term, its
// candidates' array in a line-search round, with the candidates the rollout kernels skip skipped here).  DDP_HIP_MAX_AIM_FRAMES
// lanes per state, 16 states per wave: lane i walks frame i (rbd::frame_aim_term: one walk joint -> root with the eye and the
// axis, no jacobian, no per-joint arrays) and leaves 1/2 (w_aim |r_aim|^2 + w_range r_range^2) in LDS; the group's first lane adds
// the frames' terms in ascending order.  A term of weight 0 is left out, a frame whose two weights are 0 is not walked, with
// w_range = 0 rho is not read, a frame whose line of sight is shorter than 1e-12 forms nothing, and a state without a formed term
// adds nothing (add != 0) or stores +0 (add == 0).  A non-finite state gives a NaN term, as com_cost_kernel's does
__global__ __launch_bounds__(64) void frame_aim_cost_kernel(FrameAimDev fa, const DevModel* model, const double* xs, int64_t traj_stride,
                                                            int64_t count, int32_t T1, int32_t nx, int32_t na, const int32_t* state,
                                                            int32_t round, double* out, int32_t add) {
  __shared__ double s_term[64];
  __shared__ int32_t s_formed[64];
  const DevModel& m = *model;
  pair_lanes_fold<DDP_HIP_MAX_AIM_FRAMES, false>(s_term, s_formed, fa.nf, xs, traj_stride, count, T1, nx, na, state, round, out, add,
                                                 [&](int i, int64_t bt1, const double* x, double* term) {
    return rbd::frame_aim_term(m, fa, i, bt1, x, term);
  });
}

// ddp_hip_frame_aim_error: one lane per (instance, t, frame) of one resident trajectory, out[(bt1 nf + i) 2 ..] = (theta, l) of
// frame i against the resident target, whatever the weights: theta = atan2(|n x dh|, n . dh), 0 where l <= 1e-12
__global__ __launch_bounds__(64) void frame_aim_error_kernel(FrameAimDev fa, const DevModel* model, const double* xs, int64_t count, int32_t nx,
                                                             double* out) {
  const int64_t e = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (e >= count * fa.nf) return;
  const int64_t bt1 = e / fa.nf;
  const int i = (int)(e % fa.nf);
  const DevModel& m = *model;
  double p[3], nw[3], dh[3], l, theta = 0.0;
  rbd::frame_aim_walk(m, m.ff != 0, fa.joint[i], fa.off[i], fa.axis[i], xs + bt1 * nx, p, nw);
  if (rbd::frame_aim_sight(p, fa.target + e * 4, dh, &l)) {
    double c[3];
    rbd::cross3(nw, dh, c);
    theta = atan2(sqrt(rbd::dot3(c, c)), rbd::dot3(nw, dh));
  }
  out[e * 2] = theta;
  out[e * 2 + 1] = l;
}

// The joint-acceleration terms (DDP_HIP_FLAG_JOINT_ACCEL_COST, ddp_hip.h) of a list of states and their controls, added on top like
// the control-gravity terms above: the same list, the same two uses, us and u_stride as there (the controls the rollout applied,
// clamped where there are bounds: the kernel knows no bounds).  `lpe` lanes cooperate on one evaluation, 64 / lpe per wave:
// a = aba(x_t, u_t) by rbd::accel_group (forward dynamics alone, no jacobian; never (v_{t+1} - v_t) / dt: the list need not be a
// rollout of its controls) with the joints' records and a in dynamic LDS (rbd::accel_group_words doubles per evaluation); the
// group's first lane adds w_i (a_i - a_ref_i)^2 over the rows of weight != 0 in ascending order.  A pair whose nv weights are
// all 0 does no arithmetic; t = T has no control and no term: such a pair adds nothing (add != 0) or stores +0 (add == 0).  A
// non-finite state gives a NaN term.  ja.report != nullptr (ddp_hip_joint_accel): the weights are ignored, a goes to
// report[trajectory][T][nv] and nothing to out.  No scratch
__global__ __launch_bounds__(64) void joint_accel_cost_kernel(JointAccelDev ja, const DevModel* model, const double* xs, int64_t traj_stride,
                                                              int64_t count, int32_t T1, int32_t nx, int32_t na, int32_t lpe, const double* us,
                                                              int64_t u_stride, const int32_t* state, int32_t round, double* out, int32_t add) {
  extern __shared__ double s_ja[];
  const DevModel& m = *model;
  const int tid = threadIdx.x, g = tid / lpe, h = tid % lpe, N = m.nv;
  const int64_t e = (int64_t)blockIdx.x * (64 / lpe) + g;
  const CostPair pr = cost_pair_decode(e, count, T1, na, state, round);
  const int t = pr.t, T = T1 - 1;
  const double* w = ja.weight + pr.bt1 * N;
  bool live = pr.live && t < T;
  if (live && !ja.report && !rbd::weights_any(w, N)) live = false;
  double* st = s_ja + g * rbd::accel_group_words(m.nj, N);
  double* s_a = st + rbd::ABA_LDS_SLOTS * m.nj;
  const double* x = xs + pr.traj * traj_stride + (int64_t)t * nx;
  const double* u = us + pr.traj * u_stride + (int64_t)t * N;
  if (m.ff) rbd::accel_group<true>(m, x, x + m.nq, u, s_a, st, h, lpe, live);
  else rbd::accel_group<false>(m, x, x + m.nq, u, s_a, st, h, lpe, live);
  if (ja.report) {
    if (live)
      for (int i = h; i < N; i += lpe) ja.report[(pr.traj * T + t) * N + i] = s_a[i];
    return;
  }
  if (h != 0 || pr.skip) return;
  double acc = 0.0;
  if (live) {
    const double* ref = ja.target + pr.bt1 * N;
    for (int i = 0; i < N; ++i) {
      const double wi = w[i];
      if (wi == 0.0) continue;
      const double r = s_a[i] - ref[i];
      acc += wi * r * r;
    }
  }
  cost_pair_store(out, e, 0.5 * acc, live, add);
}

// The obstacle terms (DDP_HIP_FLAG_OBSTACLE_COST, ddp_hip.h) of a list of states, added on top like the frame-velocity terms above:
// the same list, the same two uses (add != 0: out[pair] += term behind cost_kernel; add == 0: out[pair] = term, the candidates' array in a
// line-search round, with the candidates the rollout kernels skip skipped here).  DDP_HIP_MAX_COLLISION_POINTS lanes per pair, 4
// pairs per wave: lane k walks point k once (rbd::frame_point: no jacobian, no per-joint arrays) and leaves 1/2 sum_o w e^2 over
// its live slots in LDS; the group's first lane adds the points' terms in ascending order.  A pair (point, slot) with w == 0 or
// e == 0 is left out, a block whose weights are all 0 walks nothing, and a pair without an active term adds nothing (add != 0) or
// stores +0 (add == 0).  A non-finite state gives a NaN term, as com_cost_kernel's does
template <bool GRID>
__global__ __launch_bounds__(64) void obstacle_cost_kernel(ObstacleCostDev ob, const DevModel* model, const double* xs, int64_t traj_stride,
                                                           int64_t count, int32_t T1, int32_t nx, int32_t na, const int32_t* state,
                                                           int32_t round, double* out, int32_t add) {
  __shared__ double s_term[64];
  __shared__ int32_t s_act[64];
  const DevModel& m = *model;
  pair_lanes_fold<DDP_HIP_MAX_COLLISION_POINTS, false>(s_term, s_act, ob.np, xs, traj_stride, count, T1, nx, na, state, round, out, add,
                                                       [&](int k, int64_t bt1, const double* x, double* term) {
    const double* w = ob.weight + bt1 * ob.no;
    if (!rbd::weights_any(w, ob.no)) return false;
    const double off[3] = {ob.off[k][0], ob.off[k][1], ob.off[k][2]};
    double pk[3];
    bool act = false;
    rbd::frame_point(m, m.ff != 0, ob.joint[k], off, x, pk);
    *term = rbd::obstacle_point_term<GRID>(ob, k, pk, ob.geom + bt1 * ob.no * 4, w, &act);
    return act;
  });
}

// ddp_hip_obstacle_clearance: the same lane layout over the `count` (instance, t) pairs of one resident trajectory (a list of
// one-state trajectories, no candidates to skip), min instead of sum: out[pair] = min over points and over slots with w != 0 of
// d_ko, +inf where no slot is live, NaN where a distance is NaN
template <bool GRID>
__global__ __launch_bounds__(64) void obstacle_clearance_kernel(ObstacleCostDev ob, const DevModel* model, const double* xs, int64_t count,
                                                                int32_t nx, double* out) {
  __shared__ double s_min[64];
  const DevModel& m = *model;
  pair_lanes_fold<DDP_HIP_MAX_COLLISION_POINTS, true>(s_min, nullptr, ob.np, xs, nx, count, 1, nx, 1, nullptr, 0, out, 0,
                                                      [&](int k, int64_t e, const double* x, double* best) {
    const double* w = ob.weight + e * ob.no;
    if (!rbd::weights_any(w, ob.no)) return false;
    const double off[3] = {ob.off[k][0], ob.off[k][1], ob.off[k][2]};
    double pk[3];
    rbd::frame_point(m, m.ff != 0, ob.joint[k], off, x, pk);
    *best = rbd::obstacle_point_clearance<GRID>(ob, k, pk, ob.geom + e * ob.no * 4, w);
    return true;
  });
}

// The self-collision kernels below need two steps per state, so they do not fit pair_lanes_fold: DDP_HIP_MAX_COLLISION_POINTS lanes
// per pair of the list (a state), 4 states per wave.  Step 1: lane k < n_points of the group walks sphere k (rbd::frame_point) and
// leaves p_k in LDS (s_p: 64 x 3, the kernel's own).  After a barrier, step 2: the lanes take the collision pairs, lane k pair k,
// k + 16, ... (more than one per lane once n_pairs exceeds the group width), and leave w d^2 of an active pair -- with MIN: d of a
// pair with w != 0 -- and a flag in LDS (s_term, s_formed: 4 x DDP_HIP_MAX_COLLISION_PAIRS each).  After a second barrier the
// group's first lane folds in ascending pair order: 1/2 the sum of the formed ones, or with MIN the rbd::obstacle_min of them all
// from +inf, and cost_pair_store writes the result.  A state whose weights are all 0 is not walked
template <bool MIN>
__device__ __forceinline__ void self_collision_fold(const SelfCollisionDev& sc, const DevModel& m, double (*s_p)[3], double* s_term,
                                                    int32_t* s_formed, const double* xs, int64_t traj_stride, int64_t count, int32_t T1,
                                                    int32_t nx, int32_t na, const int32_t* state, int32_t round, double* out, int32_t add) {
  constexpr int L = DDP_HIP_MAX_COLLISION_POINTS, NP = DDP_HIP_MAX_COLLISION_PAIRS;
  const int tid = threadIdx.x, g = tid / L, k = tid % L;
  const int64_t e = (int64_t)blockIdx.x * (64 / L) + g;
  const CostPair pr = cost_pair_decode(e, count, T1, na, state, round);
  const double* w = sc.weight + pr.bt1 * sc.npair;
  const bool live = pr.live && rbd::weights_any(w, sc.npair);
  if (live && k < sc.np) {
    const double off[3] = {sc.off[k][0], sc.off[k][1], sc.off[k][2]};
    rbd::frame_point(m, m.ff != 0, sc.joint[k], off, xs + pr.traj * traj_stride + (int64_t)pr.t * nx, s_p[tid]);
  }
  __syncthreads();
  for (int i = k; i < NP; i += L) {
    double term = MIN ? INFINITY : 0.0;
    bool formed = false;
    if (live && i < sc.npair && w[i] != 0.0) {
      double d;
      (void)rbd::self_collision_distance(sc, i, s_p[g * L + sc.pa[i]], s_p[g * L + sc.pb[i]], sc.margin[pr.bt1 * sc.npair + i], &d, nullptr);
      if (MIN) { term = d; formed = true; }
      else if (rbd::obstacle_active(d)) { term = w[i] * d * d; formed = true; }
    }
    s_term[g * NP + i] = term;
    s_formed[g * NP + i] = formed ? 1 : 0;
  }
  __syncthreads();
  if (k != 0 || pr.skip) return;
  double acc = MIN ? INFINITY : 0.0;
  bool any = false;
  for (int i = 0; i < sc.npair; ++i) {
    if (!s_formed[g * NP + i]) continue;
    acc = MIN ? rbd::obstacle_min(acc, s_term[g * NP + i]) : acc + s_term[g * NP + i];
    any = true;
  }
  cost_pair_store(out, e, MIN ? acc : 0.5 * acc, any, add);
}

// The self-collision terms (DDP_HIP_FLAG_SELF_COLLISION_COST, ddp_hip.h) of a list of states, added on top like the obstacle terms
// above: the same list, the same two uses (add != 0: out[pair] += term behind cost_kernel; add == 0: out[pair] = term, the
// candidates' array in a line-search round, with the candidates the rollout kernels skip skipped here).  A pair of spheres with
// w == 0 or e == 0 is left out, and a state without an active pair adds nothing (add != 0) or stores +0 (add == 0).  A non-finite
// state gives a NaN term, as com_cost_kernel's does
__global__ __launch_bounds__(64) void self_collision_cost_kernel(SelfCollisionDev sc, const DevModel* model, const double* xs, int64_t traj_stride,
                                                                 int64_t count, int32_t T1, int32_t nx, int32_t na, const int32_t* state,
                                                                 int32_t round, double* out, int32_t add) {
  __shared__ double s_p[64][3], s_term[4 * DDP_HIP_MAX_COLLISION_PAIRS];
  __shared__ int32_t s_act[4 * DDP_HIP_MAX_COLLISION_PAIRS];
  self_collision_fold<false>(sc, *model, s_p, s_term, s_act, xs, traj_stride, count, T1, nx, na, state, round, out, add);
}

// ddp_hip_self_collision_clearance: the same layout over the `count` (instance, t) pairs of one resident trajectory (a list of
// one-state trajectories, no candidates to skip), min instead of sum: out[pair] = min over the pairs of spheres with w != 0 of d_i,
// +inf where none is live, NaN where a distance is NaN
__global__ __launch_bounds__(64) void self_collision_clearance_kernel(SelfCollisionDev sc, const DevModel* model, const double* xs, int64_t count,
                                                                      int32_t nx, double* out) {
  __shared__ double s_p[64][3], s_min[4 * DDP_HIP_MAX_COLLISION_PAIRS];
  __shared__ int32_t s_live[4 * DDP_HIP_MAX_COLLISION_PAIRS];
  self_collision_fold<true>(sc, *model, s_p, s_min, s_live, xs, nx, count, 1, nx, 1, nullptr, 0, out, 0);
}

// The capsule kernels below take the two steps of the self-collision kernels above: DDP_HIP_MAX_CAPSULES lanes per pair of the
// list (a state), 4 states per wave.  Step 1: lane k < n_capsules of the group walks both ends of capsule k in one walk
// (rbd::capsule_ends) and leaves them in LDS (s_e: 64 x 2 x 3, the kernel's own).  After a barrier, step 2: the lanes take the
// capsule pairs, lane k pair k and pair k + 16, form the closest points and d (rbd::capsule_distance: a world body is read from
// the pair's geometry) and leave w d^2 of an active pair -- with MIN: d of a pair with w != 0 -- and a flag in LDS (s_term,
// s_formed: 4 x DDP_HIP_MAX_CAPSULE_PAIRS each).  After a second barrier the group's first lane folds in ascending pair order: 1/2
// the sum of the formed ones, or with MIN the rbd::obstacle_min of them all from +inf, and cost_pair_store writes the result.  A
// state whose weights are all 0 is not walked.
// GRID (some pair is of kind DDP_HIP_CAPSULE_VS_GRID; the other instantiation is the code from before the kind): one lane running a
// grid pair's up to 33 independent lookups of 8 doubles one after another is a latency chain, and a line-search round runs it for
// every candidate.  So between the two steps the group's 16 lanes take the (grid pair, sample) items of the state in strides, item
// `it` of the description's flat list (CapsuleCostDev::gbase) by lane it % 16, and leave phi of each in LDS (s_phi: 4 x
// grid_items, dynamic).  After one more barrier the pair's own lane of step 2 scans its pair's values in ascending j
// (capsule_grid_better: smallest j on a tie, the first NaN before everything), which no dealing can change, and forms d; the
// value and the clearance need no gradient.
// BOX (some pair is of kind DDP_HIP_CAPSULE_VS_BOX): such a pair is one closed-form evaluation on its own lane in step 2
// (rbd::capsule_distance); nothing is dealt, and without a grid pair nothing of the grid's dealing is compiled in
template <bool MIN, bool GRID, bool BOX>
__device__ __forceinline__ void capsule_fold(const CapsuleCostDev& cp, const DevModel& m, double (*s_e)[2][3], double* s_term, int32_t* s_formed,
                                             double* s_phi, const double* xs, int64_t traj_stride, int64_t count, int32_t T1, int32_t nx, int32_t na,
                                             const int32_t* state, int32_t round, double* out, int32_t add) {
  constexpr int L = DDP_HIP_MAX_CAPSULES, NP = DDP_HIP_MAX_CAPSULE_PAIRS;
  const int tid = threadIdx.x, g = tid / L, k = tid % L;
  const int64_t e = (int64_t)blockIdx.x * (64 / L) + g;
  const CostPair pr = cost_pair_decode(e, count, T1, na, state, round);
  const double* w = cp.weight + pr.bt1 * cp.npair;
  const bool live = pr.live && rbd::weights_any(w, cp.npair);
  if (live && k < cp.nc) rbd::capsule_ends(m, m.ff != 0, cp, k, xs + pr.traj * traj_stride + (int64_t)pr.t * nx, s_e[tid]);
  __syncthreads();
  if constexpr (GRID) {
    int i = 0;                                                       // the grid pair that holds item `it` (it only grows)
    for (int it = k; it < cp.grid_items; it += L) {
      while (cp.kind[i] != DDP_HIP_CAPSULE_VS_GRID || it >= cp.gbase[i] + cp.nseg[cp.pa[i]] + 1) ++i;
      double phi = INFINITY;
      if (live && w[i] != 0.0) {
        const double (*ea)[3] = s_e[g * L + cp.pa[i]];
        double c[3], grad[3];
        capsule_grid_sample(cp.grid, ea[0], ea[1], cp.geom + (pr.bt1 * cp.npair + i) * 8, cp.nseg[cp.pa[i]], it - cp.gbase[i], c, &phi, grad);
      }
      s_phi[g * cp.grid_items + it] = phi;
    }
    __syncthreads();
  }
  for (int i = k; i < NP; i += L) {
    double term = MIN ? INFINITY : 0.0;
    bool formed = false;
    if (live && i < cp.npair && w[i] != 0.0) {
      const double (*ea)[3] = s_e[g * L + cp.pa[i]];
      const double (*eb)[3] = s_e[g * L + cp.pb[i]];
      double d, ca[3], cb[3], u[3];
      if (GRID && cp.kind[i] == DDP_HIP_CAPSULE_VS_GRID) {
        const double* ph = s_phi + g * cp.grid_items + cp.gbase[i];
        double best = ph[0];
        for (int j = 1; j <= cp.nseg[cp.pa[i]]; ++j)
          if (capsule_grid_better(ph[j], best, false)) best = ph[j];
        u[0] = u[1] = u[2] = 0.0;
        (void)capsule_grid_pair(best, u, cp.radius[cp.pa[i]], cp.geom[(pr.bt1 * cp.npair + i) * 8 + 7], &d, u);
      } else {
        (void)rbd::capsule_distance<false, BOX>(cp, i, ea[0], ea[1], eb[0], eb[1], cp.geom + (pr.bt1 * cp.npair + i) * 8, &d, ca, cb, u);
      }
      if (MIN) { term = d; formed = true; }
      else if (rbd::obstacle_active(d)) { term = w[i] * d * d; formed = true; }
    }
    s_term[g * NP + i] = term;
    s_formed[g * NP + i] = formed ? 1 : 0;
  }
  __syncthreads();
  if (k != 0 || pr.skip) return;
  double acc = MIN ? INFINITY : 0.0;
  bool any = false;
  for (int i = 0; i < cp.npair; ++i) {
    if (!s_formed[g * NP + i]) continue;
    acc = MIN ? rbd::obstacle_min(acc, s_term[g * NP + i]) : acc + s_term[g * NP + i];
    any = true;
  }
  cost_pair_store(out, e, MIN ? acc : 0.5 * acc, any, add);
}

// The capsule terms (DDP_HIP_FLAG_CAPSULE_COST, ddp_hip.h) of a list of states, added on top like the self-collision terms above:
// the same list, the same two uses (add != 0: out[pair] += term behind cost_kernel; add == 0: out[pair] = term, the candidates'
// array in a line-search round, with the candidates the rollout kernels skip skipped here).  A pair of bodies with w == 0 or
// e == 0 is left out, and a state without an active pair adds nothing (add != 0) or stores +0 (add == 0).  A non-finite state
// gives a NaN term, as com_cost_kernel's does.  GRID: 4 x grid_items doubles of dynamic LDS
extern __shared__ double s_capsule_phi[];
template <bool GRID, bool BOX>
__global__ __launch_bounds__(64) void capsule_cost_kernel(CapsuleCostDev cp, const DevModel* model, const double* xs, int64_t traj_stride,
                                                          int64_t count, int32_t T1, int32_t nx, int32_t na, const int32_t* state,
                                                          int32_t round, double* out, int32_t add) {
  __shared__ double s_e[64][2][3], s_term[4 * DDP_HIP_MAX_CAPSULE_PAIRS];
  __shared__ int32_t s_act[4 * DDP_HIP_MAX_CAPSULE_PAIRS];
  capsule_fold<false, GRID, BOX>(cp, *model, s_e, s_term, s_act, GRID ? s_capsule_phi : nullptr, xs, traj_stride, count, T1, nx, na, state, round, out, add);
}

// ddp_hip_capsule_clearance: the same layout over the `count` (instance, t) pairs of one resident trajectory (a list of one-state
// trajectories, no candidates to skip), min instead of sum: out[pair] = min over the capsule pairs with w != 0 of d_i, +inf where
// none is live, NaN where a distance is NaN
template <bool GRID, bool BOX>
__global__ __launch_bounds__(64) void capsule_clearance_kernel(CapsuleCostDev cp, const DevModel* model, const double* xs, int64_t count,
                                                               int32_t nx, double* out) {
  __shared__ double s_e[64][2][3], s_min[4 * DDP_HIP_MAX_CAPSULE_PAIRS];
  __shared__ int32_t s_live[4 * DDP_HIP_MAX_CAPSULE_PAIRS];
  capsule_fold<true, GRID, BOX>(cp, *model, s_e, s_min, s_live, GRID ? s_capsule_phi : nullptr, xs, nx, count, 1, nx, 1, nullptr, 0, out, 0);
}

// accept rule (ddp_fwd.ipp:56-60): the first (= largest) candidate with sum(new - old) <= 0; the winner's
// trajectory becomes (X_NEW, U_NEW).  grid = batch.
__global__ void select_kernel(FwdParams p) {
  const int b = blockIdx.x;
  // every wave must see the state as it was at launch: thread 0 rewrites it below, and a wave scheduled late would
  // otherwise leave before its share of the trajectory copy
  __shared__ int s_state, s_win, s_last;
  if (threadIdx.x == 0) s_state = p.state[b];
  __syncthreads();
  if (s_state != 0) return;
  const int na = p.n_alpha;
  const int64_t T = p.d.T;
  const int nx = (int)p.d.nx, nu = (int)p.d.m;
  if (threadIdx.x == 0) {
    int win = -1, last = -1;
    for (int a = 0; a < na; ++a) {
      const int cand = p.round * na + a;
      if (cand > 33) break;
      last = a;
      if (p.no_linesearch || p.fw_dcost[(int64_t)b * na + a] <= 0) { win = a; break; }
    }
    s_win = win;
    s_last = last;
    const bool floor_hit = (p.round * na + na - 1) >= 33;
    if (win >= 0) {
      p.state[b] = 1;
      p.step[b] = ldexp(1.0, -(p.round * na + win));
      p.dcost_acc[b] = p.fw_dcost[(int64_t)b * na + win];
    } else if (floor_hit) {
      p.state[b] = 2;
      p.step[b] = ldexp(1.0, -34);                 // the value `step` holds when the loop gives up
      p.dcost_acc[b] = last >= 0 ? p.fw_dcost[(int64_t)b * na + last] : 0.0;
    }
  }
  __syncthreads();
  const int src = s_win >= 0 ? s_win : s_last;     // on failure new_traj holds the last rollout tried
  if (src < 0) return;
  if (s_win < 0 && (p.round * na + na - 1) < 33) return;
  const double* xw = p.fw_x + ((int64_t)b * na + src) * (T + 1) * nx;
  const double* uw = p.fw_u + ((int64_t)b * na + src) * T * nu;
  double* xn = p.x_new + (int64_t)b * (T + 1) * nx;
  double* un = p.u_new + (int64_t)b * T * nu;
  for (int64_t i = threadIdx.x; i < (T + 1) * nx; i += blockDim.x) xn[i] = xw[i];
  for (int64_t i = threadIdx.x; i < T * nu; i += blockDim.x) un[i] = uw[i];
}

FwdParams make_params(ddp_hip_ctx* ctx) {
  FwdParams p{};
  p.d = ctx->d;
  p.model = ctx->model_d;
  p.ne = ctx->ne_d;
  p.Epre = ctx->Epre_d;
  p.target = ctx->target_d;
  auto S = [&](int s) { return ctx->seq[s].ptr; };
  p.x_old = S(DDP_HIP_SEQ_X); p.u_old = S(DDP_HIP_SEQ_U);
  p.x_new = S(DDP_HIP_SEQ_X_NEW); p.u_new = S(DDP_HIP_SEQ_U_NEW);
  p.fb_val = S(DDP_HIP_SEQ_FB_VAL); p.fb_jac = S(DDP_HIP_SEQ_FB_JAC);
  p.mult_origin = S(DDP_HIP_SEQ_MULT_ORIGIN); p.mult_val = S(DDP_HIP_SEQ_MULT_VAL); p.mult_jac = S(DDP_HIP_SEQ_MULT_JAC);
  p.mu = ctx->mu_d;
  p.costs_old = S(DDP_HIP_SEQ_COSTS_OLD); p.costs_new = S(DDP_HIP_SEQ_COSTS_NEW);
  p.fw_x = ctx->fw_x; p.fw_u = ctx->fw_u; p.fw_dcost = ctx->fw_dcost;
  p.step = ctx->step_d; p.dcost_acc = ctx->fw_dcost_acc_d; p.state = ctx->fw_state_d;
  p.n_alpha = ctx->n_alpha_max;
  p.track = (ctx->flags & DDP_HIP_FLAG_TRACKING_COST) ? 1 : 0;
  p.xref = S(DDP_HIP_SEQ_COST_XREF); p.wx = S(DDP_HIP_SEQ_COST_WX); p.uref = S(DDP_HIP_SEQ_COST_UREF); p.wu = S(DDP_HIP_SEQ_COST_WU);
  p.cost_inline = ctx->d.Etot == 0 ? 1 : 0;
  p.fw_cost = ctx->fw_cost;
  p.ctrl_lo = S(DDP_HIP_SEQ_CTRL_LO); p.ctrl_hi = S(DDP_HIP_SEQ_CTRL_HI);
  p.fc = frame_cost_dev(ctx);
  p.sl = state_limits_dev(ctx);
  p.round = 0;
  return p;
}

// the closed-loop instantiation of the latency kernel for (free-flyer root, inline cost terms, control bounds)
using Lat2Fn = void (*)(FwdParams);
Lat2Fn lat2_kernel(bool ff, int cost, bool box, bool pipe) {
#define LAT2_ROW(FF, COST) {{&forward_kernel_lat2<38, false, FF, COST, false, false>, &forward_kernel_lat2<38, false, FF, COST, false, true>}, \
                            {&forward_kernel_lat2<38, false, FF, COST, true, false>, &forward_kernel_lat2<38, false, FF, COST, true, true>}}
  // COST 8 .. 15: the orientation terms; bit 3 implies bit 1, so only 10, 11, 14 and 15 exist (slots 8 .. 11)
  static const Lat2Fn table[2][12][2][2] = {{LAT2_ROW(false, 0), LAT2_ROW(false, 1), LAT2_ROW(false, 2), LAT2_ROW(false, 3),
                                             LAT2_ROW(false, 4), LAT2_ROW(false, 5), LAT2_ROW(false, 6), LAT2_ROW(false, 7),
                                             LAT2_ROW(false, 10), LAT2_ROW(false, 11), LAT2_ROW(false, 14), LAT2_ROW(false, 15)},
                                            {LAT2_ROW(true, 0), LAT2_ROW(true, 1), LAT2_ROW(true, 2), LAT2_ROW(true, 3),
                                             LAT2_ROW(true, 4), LAT2_ROW(true, 5), LAT2_ROW(true, 6), LAT2_ROW(true, 7),
                                             LAT2_ROW(true, 10), LAT2_ROW(true, 11), LAT2_ROW(true, 14), LAT2_ROW(true, 15)}};
#undef LAT2_ROW
  if ((cost & 8) && !(cost & 2)) return nullptr;
  const int slot = (cost & 8) ? 8 + (cost & 1) + ((cost & 4) ? 2 : 0) : cost & 7;
  return table[ff ? 1 : 0][slot][box ? 1 : 0][pipe ? 1 : 0];
}
// the open-loop instantiation (ddp_hip_rollout)
Lat2Fn lat2_open_kernel(bool ff, bool pipe) {
  static const Lat2Fn table[2][2] = {{&forward_kernel_lat2<38, true, false, 0, false, false>, &forward_kernel_lat2<38, true, false, 0, false, true>},
                                     {&forward_kernel_lat2<38, true, true, 0, false, false>, &forward_kernel_lat2<38, true, true, 0, false, true>}};
  return table[ff ? 1 : 0][pipe ? 1 : 0];
}
// ... and the dynamic LDS of a launch
size_t lat2_lds(bool box, bool pipe) {
  if (pipe) return box ? sizeof(FwdPipeLdsBox<38>) : sizeof(FwdPipeLds<38>);
  return box ? sizeof(FwdLat2LdsBox<38>) : sizeof(FwdLat2Lds<38>);
}

#define DISPATCH_NJ(nv, CALL)                 \
  do {                                        \
    if ((nv) <= 1) { CALL(1); }               \
    else if ((nv) <= 6) { CALL(6); }          \
    else if ((nv) <= 38) { CALL(38); }        \
    else { CALL(64); }                        \
  } while (0)

}  // namespace

bool fwd_lat_supported(const ddp_hip_ctx* ctx) {
  const DevModel& m = ctx->model_h;
  // (constrained problems: the rollout runs on the latency kernel, the candidates' cost terms on cand_cost_kernel)
  if (m.kind != DDP_HIP_MODEL_TREE || ctx->d.nv != 38) return false;
  // the cooperative traversal: at most 8 joints per tree level (one helper lane each), 16 levels and 3 children per joint
  // (rbd::coop_role packs a lane's joint of a level into one word)
  if (m.max_level_width > 8 || m.n_levels > 16) return false;
  for (int j = 0; j < m.nj; ++j)
    if (m.child_start[j + 1] - m.child_start[j] > rbd::ROLE_MAX_CHILDREN) return false;
  return true;
}

int fwd_setup(ddp_hip_ctx* ctx) {
  const Dims& d = ctx->d;
  const int64_t B = d.batch, na = ctx->n_alpha_max;
  HIP_TRY(hipMalloc(&ctx->fw_x, sizeof(double) * (size_t)(B * na * (d.T + 1) * d.nx)));
  HIP_TRY(hipMalloc(&ctx->fw_u, sizeof(double) * (size_t)(B * na * d.T * d.m)));
  HIP_TRY(hipMalloc(&ctx->fw_dcost, sizeof(double) * (size_t)(B * na)));
  if (d.Etot > 0) HIP_TRY(hipMalloc(&ctx->fw_cost, sizeof(double) * (size_t)(B * na * (d.T + 1))));
  HIP_TRY(hipMalloc(&ctx->step_d, sizeof(double) * (size_t)B));
  HIP_TRY(hipMalloc(&ctx->fw_dcost_acc_d, sizeof(double) * (size_t)B));
  HIP_TRY(hipMalloc(&ctx->fw_state_d, sizeof(int32_t) * (size_t)B));
  if (d.nv == 38) {
    // per device, by every context (the attribute is not process-wide)
    for (int ff = 0; ff < 2; ++ff)
      for (int pipe = 0; pipe < 2; ++pipe)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(lat2_open_kernel(ff != 0, pipe != 0)), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lat2_lds(false, pipe != 0)));
    // the closed-loop instantiations this context's flags can reach (lat2_kernel)
    const bool frame = (ctx->flags & DDP_HIP_FLAG_FRAME_COST) != 0, bounds = (ctx->flags & DDP_HIP_FLAG_CONTROL_BOUNDS) != 0;
    const int costs = 1 | (frame ? 2 : 0) | ((ctx->flags & DDP_HIP_FLAG_STATE_LIMITS) ? 4 : 0) |
                      ((ctx->flags & DDP_HIP_FLAG_FRAME_ORIENT_COST) ? 8 : 0);   // the COST bits this context can set
    for (int ff = 0; ff < 2; ++ff)
      for (int cost = 0; cost < 16; ++cost)
        for (int box = 0; box < (bounds ? 2 : 1); ++box)
          for (int pipe = 0; pipe < 2; ++pipe)
            if (!(cost & ~costs) && (!(cost & 8) || (cost & 2)))
              HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(lat2_kernel(ff != 0, cost, box != 0, pipe != 0)),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lat2_lds(box != 0, pipe != 0)));
  }
  return DDP_HIP_OK;
}

void fwd_teardown(ddp_hip_ctx* ctx) {
  if (ctx->fw_x) (void)hipFree(ctx->fw_x);
  if (ctx->fw_u) (void)hipFree(ctx->fw_u);
  if (ctx->fw_dcost) (void)hipFree(ctx->fw_dcost);
  if (ctx->fw_cost) (void)hipFree(ctx->fw_cost);
  if (ctx->step_d) (void)hipFree(ctx->step_d);
  if (ctx->fw_dcost_acc_d) (void)hipFree(ctx->fw_dcost_acc_d);
  if (ctx->pick_pair_d) (void)hipFree(ctx->pick_pair_d);
  if (ctx->fw_state_d) (void)hipFree(ctx->fw_state_d);
}

#ifdef FWD_STAMPS
extern "C" int ddp_hip_debug_fwd_stamps(unsigned long long* out36) {
  return hipMemcpyFromSymbol(out36, HIP_SYMBOL(g_fwd_stamps), sizeof(unsigned long long) * 36) == hipSuccess ? 0 : -2;
}
#endif

extern "C" int ddp_hip_rollout(ddp_hip_ctx* ctx) {
  if (!ctx) return DDP_HIP_E_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  FwdParams p = make_params(ctx);
  if (fwd_lat_supported(ctx)) {
    // unconstrained trees of the Talos size: the open-loop form of the latency kernel (one workgroup per instance)
    const bool pipe = fwd_use_pipe(ctx, ctx->d.batch, 1);
    hipLaunchKernelGGL(lat2_open_kernel(ctx->model_h.ff != 0, pipe), dim3((unsigned)ctx->d.batch), dim3(pipe && fwd_pipe_assist(true, ctx->model_h.ff != 0, 0, false) ? 192 : 128), lat2_lds(false, pipe), ctx->stream, p);
  } else {
    const int bs = 64;
    const unsigned grid = (unsigned)((ctx->d.batch + bs - 1) / bs);
#define CALL(NJ) hipLaunchKernelGGL((rollout_kernel<NJ>), dim3(grid), dim3(bs), 0, ctx->stream, p)
    DISPATCH_NJ(ctx->d.nv, CALL);
#undef CALL
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DDP_HIP_OK;
}

// the (FRAME, LIMIT) instantiation that the resident cost data asks for: frames with a non-zero weight (level 2 only with a
// non-zero orientation weight), limits with one
#define DISPATCH_COST(p, LAUNCH)                               \
  do {                                                         \
    const bool fr_ = (p).fc.target != nullptr, or_ = (p).fc.oquat != nullptr, li_ = (p).sl.weight != nullptr; \
    if (or_ && li_) LAUNCH(2, true);                           \
    else if (or_) LAUNCH(2, false);                            \
    else if (fr_ && li_) LAUNCH(1, true);                      \
    else if (li_) LAUNCH(0, true);                             \
    else if (fr_) LAUNCH(1, false);                            \
    else LAUNCH(0, false);                                     \
  } while (0)

// The add-on kernels over `count` (trajectory, t) pairs of trajectories laid out like X (na per instance): one signature.  us: the
// controls that belong to xs, laid out like U (trajectory k's at us + k T m: U, U_NEW or the candidates' fw_u); the terms of the
// state alone ignore them
typedef void (*AddOnLaunch)(ddp_hip_ctx* ctx, const double* xs, const double* us, int na, int64_t count, const int32_t* state, int round, double* out, int add);

// ... and one launch: one wave per `lanes`-lane group of pairs, the kernel's view `dev` of its term first; mid: what a kernel takes
// between na and state (com_cost_kernel's lanes per evaluation)
template <class Kernel, class Dev, class... Mid>
static void launch_add_on(Kernel kernel, const Dev& dev, int lanes, ddp_hip_ctx* ctx, const double* xs, int na, int64_t count, const int32_t* state,
                          int round, double* out, int add, Mid... mid) {
  const Dims& d = ctx->d;
  const int64_t per = 64 / lanes;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((count + per - 1) / per)), dim3(64), 0, ctx->stream, dev, ctx->model_d, xs, (d.T + 1) * d.nx, count,
                     (int32_t)(d.T + 1), (int32_t)d.nx, (int32_t)na, mid..., state, (int32_t)round, out, (int32_t)add);
}

static void launch_com_cost(ddp_hip_ctx* ctx, const double* xs, const double* us, int na, int64_t count, const int32_t* state, int round, double* out, int add) {
  int32_t lpe = 8;
  while (lpe < ctx->model_h.nj) lpe *= 2;                            // (nj <= DDP_MAXJ = 64: one wave)
  launch_add_on(com_cost_kernel, com_cost_dev(ctx), lpe, ctx, xs, na, count, state, round, out, add, lpe);
}
static void launch_frame_vel_cost(ddp_hip_ctx* ctx, const double* xs, const double* us, int na, int64_t count, const int32_t* state, int round, double* out, int add) {
  launch_add_on(frame_vel_cost_kernel, frame_vel_cost_dev(ctx), DDP_HIP_MAX_COST_FRAMES, ctx, xs, na, count, state, round, out, add);
}
static void launch_momentum_cost(ddp_hip_ctx* ctx, const double* xs, const double* us, int na, int64_t count, const int32_t* state, int round, double* out, int add) {
  int32_t lpe = 8;
  while (lpe < ctx->model_h.nj) lpe *= 2;
  launch_add_on(momentum_cost_kernel, momentum_cost_dev(ctx), lpe, ctx, xs, na, count, state, round, out, add, lpe);
}
static void launch_balance_region_cost(ddp_hip_ctx* ctx, const double* xs, const double* us, int na, int64_t count, const int32_t* state, int round, double* out, int add) {
  int32_t lpe = 8;
  while (lpe < ctx->model_h.nj) lpe *= 2;
  launch_add_on(balance_region_cost_kernel, balance_region_dev(ctx), lpe, ctx, xs, na, count, state, round, out, add, lpe);
}
static void launch_relative_frame_cost(ddp_hip_ctx* ctx, const double* xs, const double* us, int na, int64_t count, const int32_t* state, int round, double* out, int add) {
  launch_add_on(relative_frame_cost_kernel, relative_frame_dev(ctx), DDP_HIP_MAX_FRAME_PAIRS, ctx, xs, na, count, state, round, out, add);
}
static void launch_control_grav_cost(ddp_hip_ctx* ctx, const double* xs, const double* us, int na, int64_t count, const int32_t* state, int round, double* out, int add) {
  int32_t lpe = 8;
  while (lpe < ctx->model_h.nj) lpe *= 2;
  launch_add_on(control_grav_cost_kernel, control_grav_dev(ctx), lpe, ctx, xs, na, count, state, round, out, add, lpe, us, ctx->d.T * ctx->d.m);
}
static void launch_frame_aim_cost(ddp_hip_ctx* ctx, const double* xs, const double* us, int na, int64_t count, const int32_t* state, int round, double* out, int add) {
  launch_add_on(frame_aim_cost_kernel, frame_aim_dev(ctx), DDP_HIP_MAX_AIM_FRAMES, ctx, xs, na, count, state, round, out, add);
}
// (one wave per two evaluations: a level of a tree is seldom wider than 32 joints; the records in dynamic LDS, < 64 KB at nv <= 38)
static constexpr int32_t kJointAccelLanes = 32;
static size_t joint_accel_lds(const ddp_hip_ctx* ctx) {
  return sizeof(double) * (size_t)((64 / kJointAccelLanes) * rbd::accel_group_words(ctx->model_h.nj, (int)ctx->d.nv));
}
static void launch_joint_accel(const JointAccelDev& ja, ddp_hip_ctx* ctx, const double* xs, const double* us, int na, int64_t count, const int32_t* state,
                               int round, double* out, int add) {
  const Dims& d = ctx->d;
  const int64_t per = 64 / kJointAccelLanes;
  hipLaunchKernelGGL(joint_accel_cost_kernel, dim3((unsigned)((count + per - 1) / per)), dim3(64), joint_accel_lds(ctx), ctx->stream, ja, ctx->model_d, xs,
                     (d.T + 1) * d.nx, count, (int32_t)(d.T + 1), (int32_t)d.nx, (int32_t)na, kJointAccelLanes, us, d.T * d.m, state, (int32_t)round, out,
                     (int32_t)add);
}
static void launch_joint_accel_cost(ddp_hip_ctx* ctx, const double* xs, const double* us, int na, int64_t count, const int32_t* state, int round, double* out, int add) {
  launch_joint_accel(joint_accel_dev(ctx), ctx, xs, us, na, count, state, round, out, add);
}
static void launch_obstacle_cost(ddp_hip_ctx* ctx, const double* xs, const double* us, int na, int64_t count, const int32_t* state, int round, double* out, int add) {
  const ObstacleCostDev ob = obstacle_cost_dev(ctx);
  launch_add_on(ob.grid_slots ? obstacle_cost_kernel<true> : obstacle_cost_kernel<false>, ob, DDP_HIP_MAX_COLLISION_POINTS, ctx, xs, na, count, state,
                round, out, add);
}
static void launch_self_collision_cost(ddp_hip_ctx* ctx, const double* xs, const double* us, int na, int64_t count, const int32_t* state, int round, double* out, int add) {
  launch_add_on(self_collision_cost_kernel, self_collision_dev(ctx), DDP_HIP_MAX_COLLISION_POINTS, ctx, xs, na, count, state, round, out, add);
}
// dynamic LDS of the capsule kernels' GRID instantiation: phi of every (grid pair, sample) item of the wave's four states (at most
// 4 x 32 x 33 doubles = 33 KB)
static size_t capsule_grid_lds(const CapsuleCostDev& cp) { return sizeof(double) * (size_t)((64 / DDP_HIP_MAX_CAPSULES) * cp.grid_items); }
static void launch_capsule_cost(ddp_hip_ctx* ctx, const double* xs, const double* us, int na, int64_t count, const int32_t* state, int round, double* out, int add) {
  const CapsuleCostDev cp = capsule_cost_dev(ctx);
  if (!cp.grid_pairs) {
    if (cp.box_pairs) launch_add_on(capsule_cost_kernel<false, true>, cp, DDP_HIP_MAX_CAPSULES, ctx, xs, na, count, state, round, out, add);
    else launch_add_on(capsule_cost_kernel<false, false>, cp, DDP_HIP_MAX_CAPSULES, ctx, xs, na, count, state, round, out, add);
    return;
  }
  const Dims& d = ctx->d;
  const int64_t per = 64 / DDP_HIP_MAX_CAPSULES;                      // (launch_add_on's launch with the samples' LDS)
  const auto kernel = cp.box_pairs ? capsule_cost_kernel<true, true> : capsule_cost_kernel<true, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)((count + per - 1) / per)), dim3(64), capsule_grid_lds(cp), ctx->stream, cp, ctx->model_d,
                     xs, (d.T + 1) * d.nx, count, (int32_t)(d.T + 1), (int32_t)d.nx, (int32_t)na, state, (int32_t)round, out, (int32_t)add);
}

// The terms formed out of line, in the fixed order of their additions (after everything cost_kernel / the rollout kernels form
// inline): CoM, frame velocities, momentum, balance regions, relative frames, control-gravity, frame aiming, joint
// accelerations, obstacles, self-collision, capsules.  launch_cost and ddp_hip_forward both walk this table and nothing else
struct AddOnTerm {
  int term;
  AddOnLaunch launch;
};
static const AddOnTerm kAddOn[] = {{COST_COM, launch_com_cost},
                                   {COST_FRAME_VEL, launch_frame_vel_cost},
                                   {COST_MOMENTUM, launch_momentum_cost},
                                   {COST_BALANCE_REGION, launch_balance_region_cost},
                                   {COST_RELATIVE_FRAME, launch_relative_frame_cost},
                                   {COST_CONTROL_GRAV, launch_control_grav_cost},
                                   {COST_FRAME_AIM, launch_frame_aim_cost},
                                   {COST_JOINT_ACCEL, launch_joint_accel_cost},
                                   {COST_OBSTACLE, launch_obstacle_cost},
                                   {COST_SELF_COLLISION, launch_self_collision_cost},
                                   {COST_CAPSULE, launch_capsule_cost}};

static int launch_cost(ddp_hip_ctx* ctx, FwdParams& p, int which) {
  const int bs = 64;
  const int64_t total = ctx->d.batch * (ctx->d.T + 1);
  const unsigned grid = (unsigned)((total + bs - 1) / bs);
#define CALL(NJ) hipLaunchKernelGGL((cost_kernel<NJ, FR, LI>), dim3(grid), dim3(bs), 0, ctx->stream, p, which)
#define LAUNCH(F, L) do { constexpr int FR = F; constexpr bool LI = L; DISPATCH_NJ(ctx->d.nv, CALL); } while (0)
  DISPATCH_COST(p, LAUNCH);
#undef LAUNCH
#undef CALL
  for (const AddOnTerm& a : kAddOn)                                   // + each live add-on term, onto what cost_kernel has left
    if (ctx->cost[a.term].live) a.launch(ctx, which == 0 ? p.x_old : p.x_new, which == 0 ? p.u_old : p.u_new, 1, total, nullptr, 0, which == 0 ? p.costs_old : p.costs_new, 1);
  HIP_TRY(hipGetLastError());
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_cost_seq_aug(ddp_hip_ctx* ctx, int which, const double* mu) {
  if (!ctx || !mu || (which != 0 && which != 1)) return DDP_HIP_E_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(ctx->mu_d, mu, sizeof(double) * (size_t)ctx->d.batch, hipMemcpyHostToDevice, ctx->stream));
  FwdParams p = make_params(ctx);
  int rc = launch_cost(ctx, p, which);
  if (rc != DDP_HIP_OK) return rc;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_obstacle_clearance(ddp_hip_ctx* ctx, int which, double* out) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_OBSTACLE_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (!out || (which != 0 && which != 1) || ctx->ob_np == 0) return DDP_HIP_E_ARG;   // (no points set: nothing to measure)
  HIP_TRY(hipSetDevice(ctx->device));
  const FwdParams p = make_params(ctx);
  const ObstacleCostDev ob = obstacle_cost_dev(ctx, true);
  const int64_t total = ctx->d.batch * (ctx->d.T + 1);
  const int64_t per = 64 / DDP_HIP_MAX_COLLISION_POINTS;
  hipLaunchKernelGGL(ob.grid_slots ? obstacle_clearance_kernel<true> : obstacle_clearance_kernel<false>, dim3((unsigned)((total + per - 1) / per)), dim3(64), 0, ctx->stream, ob, ctx->model_d,
                     which == 0 ? p.x_old : p.x_new, total, (int32_t)ctx->d.nx, ctx->ob_clear_d);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, ctx->ob_clear_d, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_self_collision_clearance(ddp_hip_ctx* ctx, int which, double* out) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_SELF_COLLISION_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (!out || (which != 0 && which != 1) || ctx->sc_npair == 0) return DDP_HIP_E_ARG;   // (no pairs set: nothing to measure)
  HIP_TRY(hipSetDevice(ctx->device));
  const FwdParams p = make_params(ctx);
  const SelfCollisionDev sc = self_collision_dev(ctx, true);
  const int64_t total = ctx->d.batch * (ctx->d.T + 1);
  const int64_t per = 64 / DDP_HIP_MAX_COLLISION_POINTS;
  hipLaunchKernelGGL(self_collision_clearance_kernel, dim3((unsigned)((total + per - 1) / per)), dim3(64), 0, ctx->stream, sc, ctx->model_d,
                     which == 0 ? p.x_old : p.x_new, total, (int32_t)ctx->d.nx, ctx->sc_clear_d);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, ctx->sc_clear_d, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_capsule_clearance(ddp_hip_ctx* ctx, int which, double* out) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_CAPSULE_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (!out || (which != 0 && which != 1) || ctx->cp_npair == 0) return DDP_HIP_E_ARG;   // (no pairs set: nothing to measure)
  HIP_TRY(hipSetDevice(ctx->device));
  const FwdParams p = make_params(ctx);
  const CapsuleCostDev cp = capsule_cost_dev(ctx, true);
  const int64_t total = ctx->d.batch * (ctx->d.T + 1);
  const int64_t per = 64 / DDP_HIP_MAX_CAPSULES;
  const auto clearance = cp.grid_pairs ? (cp.box_pairs ? capsule_clearance_kernel<true, true> : capsule_clearance_kernel<true, false>)
                                       : (cp.box_pairs ? capsule_clearance_kernel<false, true> : capsule_clearance_kernel<false, false>);
  hipLaunchKernelGGL(clearance, dim3((unsigned)((total + per - 1) / per)), dim3(64),
                     cp.grid_pairs ? capsule_grid_lds(cp) : 0, ctx->stream, cp, ctx->model_d,
                     which == 0 ? p.x_old : p.x_new, total, (int32_t)ctx->d.nx, ctx->cp_clear_d);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, ctx->cp_clear_d, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_relative_frame_error(ddp_hip_ctx* ctx, int which, double* out) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_RELATIVE_FRAME_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (!out || (which != 0 && which != 1) || ctx->rf_np == 0) return DDP_HIP_E_ARG;   // (no pairs set: nothing to measure)
  HIP_TRY(hipSetDevice(ctx->device));
  const FwdParams p = make_params(ctx);
  const RelativeFrameDev rf = relative_frame_dev(ctx, true);
  const int64_t total = ctx->d.batch * (ctx->d.T + 1);
  hipLaunchKernelGGL(relative_frame_error_kernel, dim3((unsigned)((total * rf.np + 63) / 64)), dim3(64), 0, ctx->stream, rf, ctx->model_d,
                     which == 0 ? p.x_old : p.x_new, total, (int32_t)ctx->d.nx, ctx->rf_err_d);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, ctx->rf_err_d, sizeof(double) * (size_t)(total * rf.np * 6), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_frame_aim_error(ddp_hip_ctx* ctx, int which, double* out) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_FRAME_AIM_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (!out || (which != 0 && which != 1) || ctx->fa_nf == 0) return DDP_HIP_E_ARG;   // (no frames set: nothing to measure)
  HIP_TRY(hipSetDevice(ctx->device));
  const FwdParams p = make_params(ctx);
  const FrameAimDev fa = frame_aim_dev(ctx, true);
  const int64_t total = ctx->d.batch * (ctx->d.T + 1);
  hipLaunchKernelGGL(frame_aim_error_kernel, dim3((unsigned)((total * fa.nf + 63) / 64)), dim3(64), 0, ctx->stream, fa, ctx->model_d,
                     which == 0 ? p.x_old : p.x_new, total, (int32_t)ctx->d.nx, ctx->fa_err_d);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, ctx->fa_err_d, sizeof(double) * (size_t)(total * fa.nf * 2), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_balance_region_margin(ddp_hip_ctx* ctx, int which, double* out) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_BALANCE_REGION_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (!out || (which != 0 && which != 1) || ctx->br_np == 0) return DDP_HIP_E_ARG;   // (no planes set: nothing to measure)
  HIP_TRY(hipSetDevice(ctx->device));
  const FwdParams p = make_params(ctx);
  const BalanceRegionDev br = balance_region_dev(ctx, true);
  const int64_t total = ctx->d.batch * (ctx->d.T + 1);
  int32_t lpe = 8;
  while (lpe < ctx->model_h.nj) lpe *= 2;
  const int64_t per = 64 / lpe;
  hipLaunchKernelGGL(balance_region_margin_kernel, dim3((unsigned)((total + per - 1) / per)), dim3(64), 0, ctx->stream, br, ctx->model_d,
                     which == 0 ? p.x_old : p.x_new, total, (int32_t)ctx->d.nx, lpe, ctx->br_margin_d);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, ctx->br_margin_d, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_joint_accel(ddp_hip_ctx* ctx, int which, double* out) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_JOINT_ACCEL_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (!out || (which != 0 && which != 1)) return DDP_HIP_E_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  const FwdParams p = make_params(ctx);
  JointAccelDev ja = joint_accel_dev(ctx, true);
  ja.report = ctx->ja_acc_d;
  const Dims& d = ctx->d;
  launch_joint_accel(ja, ctx, which == 0 ? p.x_old : p.x_new, which == 0 ? p.u_old : p.u_new, 1, d.batch * (d.T + 1), nullptr, 0, nullptr, 0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, ctx->ja_acc_d, sizeof(double) * (size_t)(d.batch * d.T * d.nv), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_forward(ddp_hip_ctx* ctx, const double* mu, int32_t n_alpha, double* step_out, double* dcost_out) {
  if (!ctx || !mu || !step_out || n_alpha < 0 || n_alpha > ctx->n_alpha_max) return DDP_HIP_E_ARG;
  // n_alpha == 0: do_linesearch == false (ddp_fwd.ipp:61-63) -- one rollout at step 1, accepted unconditionally
  const bool no_linesearch = n_alpha == 0;
  if (no_linesearch) n_alpha = 1;
  const Dims& d = ctx->d;
  const int64_t B = d.batch;
  HIP_TRY(hipSetDevice(ctx->device));
  if (ctx->flags & DDP_HIP_FLAG_CONTROL_BOUNDS) { const int rc_ = box_check(ctx); if (rc_ != DDP_HIP_OK) return rc_; }
  HIP_TRY(hipMemcpyAsync(ctx->mu_d, mu, sizeof(double) * (size_t)B, hipMemcpyHostToDevice, ctx->stream));
  std::vector<int32_t> state((size_t)B);
  for (int64_t b = 0; b < B; ++b) state[(size_t)b] = ctx->active_h[(size_t)b] ? 0 : 1;   // a frozen instance is not searched
  HIP_TRY(hipMemcpyAsync(ctx->fw_state_d, state.data(), sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, ctx->stream));
  FwdParams p = make_params(ctx);
  p.n_alpha = n_alpha;
  p.no_linesearch = no_linesearch ? 1 : 0;
  int rc = launch_cost(ctx, p, 0);                                   // ddp_fwd.ipp:24-26
  if (rc != DDP_HIP_OK) return rc;
  const int bs = 64;
  const unsigned grid = (unsigned)((B * n_alpha + bs - 1) / bs);
  bool floor_hit = false;
  for (int round = 0; round * n_alpha <= 33; ++round) {
    p.round = round;
    prof_begin(ctx, DDP_HIP_K_FWD_ROLLOUT);
    // tree models of the Talos size: the latency path (two workgroups per instance, 16 lanes per candidate); with constraints the
    // cost terms of the rolled-out candidates come from cand_cost_kernel (parallel over t) instead of the rollout itself
    const bool lat_path = fwd_lat_supported(ctx) && n_alpha <= 8;
    if (lat_path) {
      // the pipelined form while its grid fits the device (fwd_use_pipe), else four candidates per workgroup
      const bool pipe = fwd_use_pipe(ctx, B, n_alpha);
      const dim3 g((unsigned)(pipe ? B * ((n_alpha + 1) / 2) : 2 * B));
      // the cost terms an unconstrained problem forms inline: bit 0 tracking, bit 1 frames, bit 2 state limits (forward_kernel_lat2: COST)
      // bit 3 the frame orientations, which imply bit 1
      const int cost = p.cost_inline ? (p.track ? 1 : 0) | (p.fc.target ? 2 : 0) | (p.sl.weight ? 4 : 0) | (p.fc.oquat ? 10 : 0) : 0;
      const bool box = p.ctrl_lo != nullptr;
      const dim3 blk(pipe && fwd_pipe_assist(false, ctx->model_h.ff != 0, cost, box) ? 192 : 128);   // (the pipelined form's third wave)
      hipLaunchKernelGGL(lat2_kernel(ctx->model_h.ff != 0, cost, box, pipe), g, blk, lat2_lds(box, pipe), ctx->stream, p);
      if (!p.cost_inline) {
        const dim3 gc((unsigned)((B * n_alpha * (d.T + 1) + 63) / 64));
#define LAUNCH(F, L) hipLaunchKernelGGL((cand_cost_kernel<38, F, L>), gc, dim3(64), 0, ctx->stream, p)
        DISPATCH_COST(p, LAUNCH);
#undef LAUNCH
        hipLaunchKernelGGL(cand_sum_kernel, dim3((unsigned)((B * n_alpha + 63) / 64)), dim3(64), 0, ctx->stream, p);
      }
    } else {
#define CALL(NJ) hipLaunchKernelGGL((forward_kernel<NJ, FR, LI>), dim3(grid), dim3(bs), 0, ctx->stream, p)
#define LAUNCH(F, L) do { constexpr int FR = F; constexpr bool LI = L; DISPATCH_NJ(d.nv, CALL); } while (0)
      DISPATCH_COST(p, LAUNCH);
#undef LAUNCH
#undef CALL
    }
    prof_end(ctx, DDP_HIP_K_FWD_ROLLOUT);
    for (const AddOnTerm& a : kAddOn) {
      // a live term's candidates, whichever rollout path ran: over fw_x into the term's candidates' array, then summed once onto
      // fw_dcost (a candidate whose sum is +0 -- no weight, no obstacle touched -- has nothing added)
      const CostBlock& k = ctx->cost[a.term];
      if (!k.live) continue;
      a.launch(ctx, p.fw_x, p.fw_u, n_alpha, B * n_alpha * (d.T + 1), p.state, round, k.cand, 0);
      hipLaunchKernelGGL(com_sum_kernel, dim3((unsigned)((B * n_alpha + 63) / 64)), dim3(64), 0, ctx->stream, k.cand, p.fw_dcost, p.state,
                         (int32_t)B, (int32_t)n_alpha, (int32_t)round, d.T);
    }
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)B), dim3(256), 0, ctx->stream, p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(state.data(), ctx->fw_state_d, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    bool searching = false;
    for (int64_t b = 0; b < B; ++b) { searching |= state[(size_t)b] == 0; floor_hit |= state[(size_t)b] == 2; }
    if (!searching) break;
  }
  HIP_TRY(hipMemcpyAsync(step_out, ctx->step_d, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
  if (dcost_out)
    HIP_TRY(hipMemcpyAsync(dcost_out, ctx->fw_dcost_acc_d, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return floor_hit ? DDP_HIP_EV_LINESEARCH_FLOOR : DDP_HIP_OK;
}
