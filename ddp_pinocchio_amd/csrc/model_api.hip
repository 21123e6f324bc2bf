// model_api.hip -- point evaluations of the Model concept (pinocchio_model.hpp:77-186) on the device, for the B2 seam:
// a host-side ddp::pinocchio::model_t<double> (adapters/pinocchio_double.cpp) answers dynamics_aba / d_dynamics_aba /
// frame_coordinates / d_frame_coordinates for ONE configuration at a time through these calls.  They are plumbing (one
// lane, one launch and two copies per call); the hot path uses the batched entry points (ddp_hip_linearize, ...).
#include <math.h>
#include <string.h>

#include <new>

#include "balance_region_cost.h"
#include "capsule_cost.h"
#include "com_cost.h"
#include "control_grav_cost.h"
#include "frame_aim_cost.h"
#include "frame_vel_cost.h"
#include "internal.h"
#include "momentum_cost.h"
#include "rbd.h"
#include "rbd_deriv.h"
#include "relative_frame_cost.h"

extern void ddp_hip_fill_dev_model(const ddp_hip_model* mo, DevModel& dm);   // ctx.hip
extern bool ddp_hip_build_tables(DevModel& dm);
extern int ddp_hip_apply_armature(DevModel& mh, DevModel* md, hipStream_t stream, const double* armature);

struct ddp_hip_model_handle {
  int device = 0;
  DevModel model_h{};
  DevModel* model_d = nullptr;
  double* buf_d = nullptr;     // [in nq + 2 nv | out 3 nv nv + 4 nv]
  hipStream_t stream = nullptr;
};

namespace {

template <int NJ>
__global__ void model_aba_kernel(const DevModel* m, const double* in, double* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int nv = m->nv;
  if (m->kind == DDP_HIP_MODEL_PENDULUM) { out[0] = rbd::pendulum_acc(*m, in[0], in[2]); return; }
  const int nq = m->nq;
  double q[NJ + 1], v[NJ], tau[NJ], a[NJ];
  for (int i = 0; i < nq; ++i) q[i] = in[i];
  for (int i = 0; i < nv; ++i) { v[i] = in[nq + i]; tau[i] = in[nq + nv + i]; }
  rbd::aba_tree<NJ>(*m, q, v, tau, a);
  for (int i = 0; i < nv; ++i) out[i] = a[i];
}

template <int NJ>
__global__ void model_aba_deriv_kernel(const DevModel* m, const double* in, double* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int nv = m->nv;
  if (m->kind == DDP_HIP_MODEL_PENDULUM) {      // pendulum_model.hpp:116-130
    out[0] = -9.81 / m->length * cos(in[0]); out[1] = 0.0; out[2] = 1.0 / m->mass;
    return;
  }
  double q[NJ], v[NJ], tau[NJ], a[NJ];
  for (int i = 0; i < nv; ++i) { q[i] = in[i]; v[i] = in[nv + i]; tau[i] = in[2 * nv + i]; }
  rbdd::aba_derivatives_lane<NJ>(*m, q, v, tau, a, out, out + nv * nv, out + 2 * nv * nv);
}

// free-flyer root: the wave-cooperative recursion of the batched kernels (rbd_deriv.h: ff_derivatives_wave), one work-group
template <int NJ>
__global__ __launch_bounds__(64) void model_aba_deriv_ff_kernel(const DevModel* m, const double* in, double* out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int nv = m->nv, nq = m->nq;
  rbdd::ff_derivatives_wave<NJ>(*m, in, in + nq, in + nq + nv, lds, threadIdx.x);
  const double* X = lds + rbdd::FfLds<NJ>::X;
  for (int r = threadIdx.x; r < nv; r += blockDim.x)
    for (int c = 0; c < nv; ++c) {
      out[r + c * nv] = rbdd::ff_minv_T<NJ>(lds, nv, r, c);
      out[nv * nv + r + c * nv] = rbdd::ff_minv_T<NJ>(lds, nv, r, nv + c);
      out[2 * nv * nv + r + c * nv] = X[r + c * nv];
    }
}

template <int NJ>
__global__ void model_frame_kernel(const DevModel* m, const double* in, double* out, int want_jac) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double q[NJ + 1];
  for (int i = 0; i < m->nq; ++i) q[i] = in[i];
  rbd::frame_position<NJ>(*m, q, out, want_jac ? out + 3 : nullptr);
}

// c(q) and Jc by one wave, with the traversal of the CoM cost kernels (com_cost.h): out = c[3] | Jc[3 nv]
__global__ __launch_bounds__(64) void model_com_kernel(const DevModel* m, const double* in, double* out) {
  __shared__ rbd::CoMWaveLds S;
  const int tid = threadIdx.x;
  if (tid < m->nj) rbd::com_stage_lane(*m, in, tid, S);
  __syncthreads();
  if (tid < m->nj) rbd::com_column_lane(*m, tid, S);
  __syncthreads();
  if (tid < 3) out[tid] = S.c[tid];
  for (int i = tid; i < 3 * m->nv; i += blockDim.x) out[3 + i] = S.J[i];
}

// (pdot, omega) of the point `off` of joint `joint`, and A = [dr/d(delta q) | dr/dv], by one wave with the traversal of
// lin_frame_vel_cost_kernel (frame_vel_cost.h): in = q | v | off[3], out = vel6 | Jq[6 nv] | Jv[6 nv] (columns off the path 0)
__global__ __launch_bounds__(64) void model_frame_vel_kernel(const DevModel* m, const double* in, double* out, int joint) {
  __shared__ rbd::VelWaveLds S;
  const int tid = threadIdx.x, nv = m->nv;
  const bool ff = m->ff != 0;
  const double* q = in;
  const double* v = in + m->nq;
  if (tid < m->nj) rbd::vel_stage_lane(*m, q, v, tid, S);
  if (tid == 63) rbd::frame_point(*m, ff, joint, in + m->nq + nv, q, S.p[0]);
  __syncthreads();
  if (tid < m->nj) rbd::vel_prefix_lane(tid, S);
  __syncthreads();
  if (tid < m->nj) rbd::vel_frame_lane(*m, tid, 0, joint, true, true, S);
  __syncthreads();
  if (tid < 6) out[tid] = S.vel[0][tid];
  for (int i = tid; i < 12 * nv; i += blockDim.x) {
    const int h = i / (6 * nv), c = (i % (6 * nv)) / 6, a = i % 6;
    out[6 + i] = ((S.cm[0][2 * h + a / 3] >> c) & 1) ? S.A[0][h][c][a] : 0.0;
  }
}

// h = (l, k) and A = [dh/d(delta q) | dh/dv] by one wave, with the traversal of lin_momentum_cost_kernel (momentum_cost.h):
// in = q | v, out = h6 | Jq[6 nv] | Jv[6 nv] (the columns that are identically zero 0).  Always with the angular part and always
// all 6 + 12 nv outputs (they fit the handle's output area of 3 * 64 * 64 + 4 * 64 doubles), whether the caller asked for the
// jacobians or not: h6 of a call with them is bit for bit h6 of a call without
__global__ __launch_bounds__(64) void model_momentum_kernel(const DevModel* m, const double* in, double* out) {
  __shared__ rbd::MomWaveLds S;
  const int tid = threadIdx.x, nv = m->nv;
  rbd::mom_jacobians_wave(*m, in, in + m->nq, tid, true, S);
  if (tid < 6) out[tid] = S.h[tid];
  for (int i = tid; i < 12 * nv; i += blockDim.x) {
    const int h = i / (6 * nv), c = (i % (6 * nv)) / 6, a = i % 6;
    out[6 + i] = ((S.cm[0][2 * h + a / 3] >> c) & 1) ? S.A[0][h][c][a] : 0.0;
  }
}

// The placement of frame B = (jb, off_b) relative to A = (ja, off_a) and its jacobian at e_rot = 0 by one wave, with the traversal
// of lin_relative_frame_cost_kernel (relative_frame_cost.h): in = q | off_a[3] | off_b[3], out = rel3 | quat4 | J[6 nv] (column-major;
// columns on both paths or on neither 0, and the rotation rows of a prismatic column)
__global__ __launch_bounds__(64) void model_relative_frame_kernel(const DevModel* m, const double* in, double* out, int ja, int jb) {
  __shared__ rbd::RelativeWaveLds S;
  const int tid = threadIdx.x, nv = m->nv;
  const bool ff = m->ff != 0;
  if (tid < m->nj) rbd::stage_joint_lane<0>(*m, in, tid, S.jw, nullptr);
  if (tid == 63) {
    rbd::RelativePlacement P;
    rbd::relative_placement(*m, ff, ja, in + m->nq, jb, in + m->nq + 3, in, true, P);
    double qt[4];
    lie::R_to_quat_pos(P.E, qt);
    for (int k = 0; k < 3; ++k) {
      out[k] = P.rel[k];
      S.pb[0][k] = P.pb[k];
      for (int a = 0; a < 3; ++a) { S.RaT[0][3 * k + a] = P.ca[k][a]; S.JR[0][3 * k + a] = P.cb[k][a]; }   // (Jlog3(0) = I: R_b^T alone)
    }
    for (int k = 0; k < 4; ++k) out[3 + k] = qt[k];
  }
  __syncthreads();
  const unsigned long long ma = rbd::tangent_mask(ff, S.jw.mask[ja]), mb = rbd::tangent_mask(ff, S.jw.mask[jb]);
  if (tid == 0) { S.ca[0] = ma & ~mb; S.cb[0] = mb & ~ma; }
  __syncthreads();
  for (int c = tid; c < nv; c += blockDim.x) {
    double col[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (((ma ^ mb) >> c) & 1) rbd::relative_frame_column(*m, ff, S, 0, c, true, true, col);
    for (int a = 0; a < 6; ++a) out[7 + 6 * c + a] = col[a];
  }
}

// g(q) and G = dg / d(delta q) by one wave, with the traversal of lin_control_grav_cost_kernel (control_grav_cost.h): in = q,
// out = g[nv] | G[nv nv] (column-major; entries off the pattern 0).  want_jac == 0: g alone, by the same steps
__global__ __launch_bounds__(64) void model_gravity_torque_kernel(const DevModel* m, const double* in, double* out, int want_jac) {
  __shared__ rbd::GravWaveLds S;
  const int tid = threadIdx.x, nv = m->nv;
  const bool ff = m->ff != 0;
  if (tid < m->nj) rbd::grav_stage_lane(*m, in, tid, S);
  const unsigned long long rot = __ballot(tid < nv && rbd::grav_tangent_rotational(*m, ff, tid < nv ? tid : 0));
  __syncthreads();
  rbd::grav_tangent_lane(*m, tid, rot, S);
  __syncthreads();
  if (tid < nv) out[tid] = S.g[tid];
  if (!want_jac) return;
  for (int e = tid; e < nv * nv; e += blockDim.x) {
    double gic = 0.0;
    (void)rbd::grav_entry(S, ff, e % nv, e / nv, &gic);
    out[nv + e] = gic;
  }
}

// The eye p and the world axis n of the aim frame (joint, off, axis) and their jacobians by one wave, with the traversal of
// lin_frame_aim_cost_kernel (frame_aim_cost.h): in = q | off[3] | axis[3], out = p3 | n3 | J[6 nv] (column-major: the rows of p,
// point_column, then the rows of n, a_c x n; columns off the path 0, and the rows of n at a column that carries no rotation)
__global__ __launch_bounds__(64) void model_frame_axis_kernel(const DevModel* m, const double* in, double* out, int joint) {
  __shared__ rbd::JointWorldLds S;
  __shared__ double s_pn[6];
  const int tid = threadIdx.x, nv = m->nv;
  const bool ff = m->ff != 0;
  if (tid < m->nj) rbd::stage_joint_lane<0>(*m, in, tid, S, nullptr);
  if (tid == 63) {
    rbd::frame_aim_walk(*m, ff, joint, in + m->nq, in + m->nq + 3, in, s_pn, s_pn + 3);
    for (int k = 0; k < 6; ++k) out[k] = s_pn[k];
  }
  __syncthreads();
  const unsigned long long path = rbd::tangent_mask(ff, S.mask[joint]);
  for (int c = tid; c < nv; c += blockDim.x) {
    double col[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ax[3];
    if ((path >> c) & 1) {
      rbd::point_column(*m, ff, S, c, s_pn, col);
      if (rbd::rotation_column(*m, ff, S, c, ax)) rbd::cross3(ax, s_pn + 3, col + 3);
    }
    for (int a = 0; a < 6; ++a) out[6 + 6 * c + a] = col[a];
  }
}

// xi = c + tau cdot and its jacobians by one wave, with the traversal of lin_balance_region_cost_kernel (balance_region_cost.h):
// in = q | v | tau, out = xi3 | Jq[3 nv] | Jv[3 nv] (column-major).  Jq = Jc + tau dcq and Jv = tau Jc entry by entry, dcq the
// momentum's dl/dq entry divided by M (a free-flyer root's three linear columns: Jc alone).  tau = 0: the CoM's lanes alone, v is
// not read, Jq is Jc and Jv is 0
__global__ __launch_bounds__(64) void model_capture_point_kernel(const DevModel* m, const double* in, double* out) {
  __shared__ rbd::BalanceWaveLds S;
  const int tid = threadIdx.x, nv = m->nv;
  const double tau = in[m->nq + nv];
  const bool rate = tau != 0.0;
  rbd::region_stage_wave(*m, in, in + m->nq, tid, rate, S);
  rbd::region_columns_wave(*m, tid, rate, S);
  const double M = rbd::region_total_mass(S, m->nj);
  if (tid < 3) out[tid] = rate ? S.c[tid] + tau * (S.mo.h[tid] / M) : S.c[tid];
  for (int i = tid; i < 3 * nv; i += blockDim.x) {
    const double jc = S.J[i];
    out[3 + i] = rate && rbd::region_rate_column(*m, i / 3) ? jc + tau * (S.mo.A[0][0][i / 3][i % 3] / M) : jc;
    out[3 + 3 * nv + i] = rate ? tau * jc : 0.0;
  }
}

// The distance of the segments a0 .. a1 of joint ja and b0 .. b1 of joint jb and its gradient by one wave, with the traversal of
// lin_capsule_cost_kernel (capsule_cost.h): in = q | a0[3] | a1[3] | b0[3] | b1[3] (joint coordinates), out = D | ca3 | cb3 | J[nv]
// (columns on both paths or on neither 0; all 0 where D == 0)
__global__ __launch_bounds__(64) void model_capsule_pair_kernel(const DevModel* m, const double* in, double* out, int ja, int jb) {
  __shared__ rbd::CapsuleWaveLds S;
  __shared__ double s_D;
  const int tid = threadIdx.x, nv = m->nv;
  const bool ff = m->ff != 0;
  if (tid < m->nj) rbd::stage_joint_lane<0>(*m, in, tid, S.jw, nullptr);
  if (tid == 63) {
    const double* e = in + m->nq;
    double a[2][3] = {{e[0], e[1], e[2]}, {e[3], e[4], e[5]}}, b[2][3] = {{e[6], e[7], e[8]}, {e[9], e[10], e[11]}};
    (void)rbd::walk_to_root<2, 0>(*m, ff, ja, in, a, nullptr, -1);
    (void)rbd::walk_to_root<2, 0>(*m, ff, jb, in, b, nullptr, -1);
    const double D = capsule_closest_points(a[0], a[1], b[0], b[1], S.ca[0], S.cb[0]);
    for (int k = 0; k < 3; ++k) S.u[0][k] = D == 0.0 ? 0.0 : (S.ca[0][k] - S.cb[0][k]) / D;
    s_D = D;
    out[0] = D;
    for (int k = 0; k < 3; ++k) { out[1 + k] = S.ca[0][k]; out[4 + k] = S.cb[0][k]; }
  }
  __syncthreads();
  const unsigned long long ma = rbd::tangent_mask(ff, S.jw.mask[ja]), mb = rbd::tangent_mask(ff, S.jw.mask[jb]);
  if (tid == 0) { S.ma[0] = ma & ~mb; S.mb[0] = mb & ~ma; }
  __syncthreads();
  for (int c = tid; c < nv; c += blockDim.x) out[7 + c] = (((ma ^ mb) >> c) & 1) && s_D != 0.0 ? rbd::capsule_z(*m, ff, S, 0, c) : 0.0;
}

// One robot capsule (the segment a0 .. a1 of joint ja, radius r) against one oriented box at one configuration by the routine the
// cost kernels use (capsule_box_closest, capsule_cost.h): in = q | a0[3] | a1[3] | half[3] | pose[7] | r, out = d (margin 0) | s |
// ca3 | u3 | grad[nv] = P_ca^T u over all of path(A), a world pair (all 0 where f* == 0: the pair has no derivative there)
__global__ __launch_bounds__(64) void model_capsule_box_kernel(const DevModel* m, const double* in, double* out, int ja) {
  __shared__ rbd::CapsuleWaveLds S;
  __shared__ int s_has;
  const int tid = threadIdx.x, nv = m->nv;
  const bool ff = m->ff != 0;
  if (tid < m->nj) rbd::stage_joint_lane<0>(*m, in, tid, S.jw, nullptr);
  if (tid == 63) {
    const double* e = in + m->nq;
    double a[2][3] = {{e[0], e[1], e[2]}, {e[3], e[4], e[5]}};
    (void)rbd::walk_to_root<2, 0>(*m, ff, ja, in, a, nullptr, -1);
    double s, d;
    const double f = capsule_box_closest(a[0], a[1], e + 6, e + 9, &s, S.ca[0], S.u[0]);
    s_has = capsule_box_pair(f, e[16], 0.0, &d) ? 1 : 0;
    out[0] = d;
    out[1] = s;
    for (int k = 0; k < 3; ++k) { S.cb[0][k] = S.ca[0][k]; out[2 + k] = S.ca[0][k]; out[5 + k] = S.u[0][k]; }
  }
  __syncthreads();
  const unsigned long long ma = rbd::tangent_mask(ff, S.jw.mask[ja]);
  if (tid == 0) { S.ma[0] = ma; S.mb[0] = 0ull; }
  __syncthreads();
  for (int c = tid; c < nv; c += blockDim.x) out[8 + c] = ((ma >> c) & 1) && s_has ? rbd::capsule_z(*m, ff, S, 0, c) : 0.0;
}

#define MODEL_DISPATCH(nv, CALL)       \
  do {                                 \
    if ((nv) <= 6) { CALL(6); }        \
    else if ((nv) <= 38) { CALL(38); } \
    else { CALL(64); }                 \
  } while (0)

int run(ddp_hip_model_handle* h, const double* in, size_t n_in, double* out, size_t n_out, int what, int want_jac) {
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipMemcpyAsync(h->buf_d, in, sizeof(double) * n_in, hipMemcpyHostToDevice, h->stream));
  double* o = h->buf_d + 3 * DDP_MAXJ + 8;
  const int nv = h->model_h.nv;
  if (what == 0) {
#define CALL(NJ) hipLaunchKernelGGL((model_aba_kernel<NJ>), dim3(1), dim3(64), 0, h->stream, h->model_d, h->buf_d, o)
    MODEL_DISPATCH(nv, CALL);
#undef CALL
  } else if (what == 1) {
    // one lane holds the whole recursion in private memory: 38 joints is what its frame allows (the batched kernels of
    // lin_analytic.hip have no such limit)
    if (h->model_h.ff) {
      if (nv > 38) return DDP_HIP_E_UNSUPPORTED;
      const size_t lds = sizeof(double) * (size_t)rbdd::FfLds<38>::TOTAL;
      if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&model_aba_deriv_ff_kernel<38>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL((model_aba_deriv_ff_kernel<38>), dim3(1), dim3(64), lds, h->stream, h->model_d, h->buf_d, o);
    } else if (nv <= 6) hipLaunchKernelGGL((model_aba_deriv_kernel<6>), dim3(1), dim3(64), 0, h->stream, h->model_d, h->buf_d, o);
    else if (nv <= 38) hipLaunchKernelGGL((model_aba_deriv_kernel<38>), dim3(1), dim3(64), 0, h->stream, h->model_d, h->buf_d, o);
    else return DDP_HIP_E_UNSUPPORTED;
  } else if (what == 3) {
    hipLaunchKernelGGL(model_com_kernel, dim3(1), dim3(64), 0, h->stream, h->model_d, h->buf_d, o);
  } else if (what == 4) {
    hipLaunchKernelGGL(model_frame_vel_kernel, dim3(1), dim3(64), 0, h->stream, h->model_d, h->buf_d, o, want_jac);   // (want_jac: the joint)
  } else if (what == 5) {
    hipLaunchKernelGGL(model_momentum_kernel, dim3(1), dim3(64), 0, h->stream, h->model_d, h->buf_d, o);
  } else if (what == 7) {
    hipLaunchKernelGGL(model_gravity_torque_kernel, dim3(1), dim3(64), 0, h->stream, h->model_d, h->buf_d, o, want_jac);
  } else if (what == 6) {
    hipLaunchKernelGGL(model_relative_frame_kernel, dim3(1), dim3(64), 0, h->stream, h->model_d, h->buf_d, o, want_jac % DDP_MAXJ,
                       want_jac / DDP_MAXJ);   // (want_jac: the two joints)
  } else if (what == 9) {
    hipLaunchKernelGGL(model_capture_point_kernel, dim3(1), dim3(64), 0, h->stream, h->model_d, h->buf_d, o);
  } else if (what == 10) {
    hipLaunchKernelGGL(model_capsule_pair_kernel, dim3(1), dim3(64), 0, h->stream, h->model_d, h->buf_d, o, want_jac % DDP_MAXJ,
                       want_jac / DDP_MAXJ);   // (want_jac: the two joints)
  } else if (what == 11) {
    hipLaunchKernelGGL(model_capsule_box_kernel, dim3(1), dim3(64), 0, h->stream, h->model_d, h->buf_d, o, want_jac);   // (want_jac: the joint)
  } else if (what == 8) {
    hipLaunchKernelGGL(model_frame_axis_kernel, dim3(1), dim3(64), 0, h->stream, h->model_d, h->buf_d, o, want_jac);   // (want_jac: the joint)
  } else {
#define CALL(NJ) hipLaunchKernelGGL((model_frame_kernel<NJ>), dim3(1), dim3(64), 0, h->stream, h->model_d, h->buf_d, o, want_jac)
    MODEL_DISPATCH(nv, CALL);
#undef CALL
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, o, sizeof(double) * n_out, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return DDP_HIP_OK;
}

}  // namespace

extern "C" int ddp_hip_model_create(const ddp_hip_model* model, int device, ddp_hip_model_handle** out) {
  if (!model || !out) return DDP_HIP_E_ARG;
  *out = nullptr;
  if (model->nv < 1 || model->nv > DDP_MAXJ) return DDP_HIP_E_ARG;
  if (model->kind == DDP_HIP_MODEL_TREE) {
    if (!model->parent || !model->jtype || !model->axis || !model->Rp || !model->pp || !model->mass_j || !model->com || !model->Ic) return DDP_HIP_E_ARG;
    const int nj = model->jtype[0] == DDP_HIP_JOINT_FREEFLYER ? model->nv - 5 : model->nv;
    if (nj < 1) return DDP_HIP_E_ARG;
    for (int i = 0; i < nj; ++i)
      if (model->parent[i] >= i || model->parent[i] < -1) return DDP_HIP_E_ARG;
  } else if (model->kind != DDP_HIP_MODEL_PENDULUM) return DDP_HIP_E_ARG;
  int ndev = ddp_hip_device_count();
  if (ndev <= 0) return DDP_HIP_E_NODEVICE;
  if (device < 0 || device >= ndev) return DDP_HIP_E_ARG;
  HIP_TRY(hipSetDevice(device));
  ddp_hip_model_handle* h = new (std::nothrow) ddp_hip_model_handle();
  if (!h) return DDP_HIP_E_HIP;
  h->device = device;
  ddp_hip_fill_dev_model(model, h->model_h);
  if (model->kind == DDP_HIP_MODEL_TREE && !ddp_hip_build_tables(h->model_h)) { delete h; return DDP_HIP_E_UNSUPPORTED; }
  if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc(&h->model_d, sizeof(DevModel)) != hipSuccess ||
      hipMalloc(&h->buf_d, sizeof(double) * (size_t)(3 * DDP_MAXJ + 8 + 3 * DDP_MAXJ * DDP_MAXJ + 4 * DDP_MAXJ)) != hipSuccess ||
      hipMemcpy(h->model_d, &h->model_h, sizeof(DevModel), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipGetLastError();
    ddp_hip_model_destroy(h);
    return DDP_HIP_E_HIP;
  }
  *out = h;
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_model_destroy(ddp_hip_model_handle* h) {
  if (!h) return DDP_HIP_E_ARG;
  (void)hipSetDevice(h->device);
  if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
  if (h->model_d) (void)hipFree(h->model_d);
  if (h->buf_d) (void)hipFree(h->buf_d);
  delete h;
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_model_set_armature(ddp_hip_model_handle* h, const double* armature) {
  if (!h) return DDP_HIP_E_ARG;
  HIP_TRY(hipSetDevice(h->device));
  return ddp_hip_apply_armature(h->model_h, h->model_d, h->stream, armature);
}

extern "C" int ddp_hip_model_aba(ddp_hip_model_handle* h, const double* q, const double* v, const double* tau, double* qdd) {
  if (!h || !q || !v || !tau || !qdd) return DDP_HIP_E_ARG;
  const int nv = h->model_h.nv, nq = h->model_h.nq;
  double in[3 * DDP_MAXJ + 1];
  memcpy(in, q, sizeof(double) * nq); memcpy(in + nq, v, sizeof(double) * nv); memcpy(in + nq + nv, tau, sizeof(double) * nv);
  return run(h, in, (size_t)(nq + 2 * nv), qdd, (size_t)nv, 0, 0);
}

extern "C" int ddp_hip_model_aba_derivatives(ddp_hip_model_handle* h, const double* q, const double* v, const double* tau,
                                             double* dq, double* dv, double* dtau) {
  if (!h || !q || !v || !tau || !dq || !dv || !dtau) return DDP_HIP_E_ARG;
  const int nv = h->model_h.nv, nq = h->model_h.nq;     // a free-flyer root: nq = nv + 1, partials in the tangent
  double in[3 * DDP_MAXJ + 1];
  memcpy(in, q, sizeof(double) * nq); memcpy(in + nq, v, sizeof(double) * nv); memcpy(in + nq + nv, tau, sizeof(double) * nv);
  const size_t nn = (size_t)nv * nv;
  double* out = new (std::nothrow) double[3 * nn];
  if (!out) return DDP_HIP_E_HIP;
  const int rc = run(h, in, (size_t)(nq + 2 * nv), out, 3 * nn, 1, 0);
  if (rc == DDP_HIP_OK) { memcpy(dq, out, sizeof(double) * nn); memcpy(dv, out + nn, sizeof(double) * nn); memcpy(dtau, out + 2 * nn, sizeof(double) * nn); }
  delete[] out;
  return rc;
}

extern "C" int ddp_hip_model_frame(ddp_hip_model_handle* h, int32_t joint, const double off[3], const double* q, double* p3, double* J) {
  if (!h || !off || !q || !p3 || h->model_h.kind != DDP_HIP_MODEL_TREE || joint < 0 || joint >= h->model_h.nj) return DDP_HIP_E_ARG;
  const int nv = h->model_h.nv;
  HIP_TRY(hipSetDevice(h->device));
  // the frame is part of the (small) device model: patch it for this call
  h->model_h.frame_joint = joint;
  for (int k = 0; k < 3; ++k) h->model_h.frame_off[k] = off[k];
  HIP_TRY(hipMemcpyAsync(h->model_d, &h->model_h, sizeof(DevModel), hipMemcpyHostToDevice, h->stream));
  double out[3 + 3 * DDP_MAXJ];
  const int rc = run(h, q, (size_t)h->model_h.nq, out, (size_t)(3 + (J ? 3 * nv : 0)), 2, J ? 1 : 0);
  if (rc != DDP_HIP_OK) return rc;
  memcpy(p3, out, sizeof(double) * 3);
  if (J) memcpy(J, out + 3, sizeof(double) * 3 * nv);
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_model_com(ddp_hip_model_handle* h, const double* q, double* c3, double* J) {
  if (!h || !q || !c3 || h->model_h.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_ARG;
  const int nv = h->model_h.nv;
  double total = 0.0;
  for (int i = 0; i < h->model_h.nj; ++i) total += h->model_h.I6[i][9];   // the body masses (ctx.hip: pack_body_inertia)
  if (!(total > 0.0)) return DDP_HIP_E_ARG;
  double out[3 + 3 * DDP_MAXJ];
  const int rc = run(h, q, (size_t)h->model_h.nq, out, (size_t)(3 + (J ? 3 * nv : 0)), 3, 0);
  if (rc != DDP_HIP_OK) return rc;
  memcpy(c3, out, sizeof(double) * 3);
  if (J) memcpy(J, out + 3, sizeof(double) * 3 * nv);
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_model_frame_velocity(ddp_hip_model_handle* h, int32_t joint, const double off[3], const double* q, const double* v,
                                            double* vel6, double* Jq, double* Jv) {
  if (!h || !off || !q || !v || !vel6 || h->model_h.kind != DDP_HIP_MODEL_TREE || joint < 0 || joint >= h->model_h.nj) return DDP_HIP_E_ARG;
  const int nv = h->model_h.nv, nq = h->model_h.nq;
  double in[2 * DDP_MAXJ + 4];
  memcpy(in, q, sizeof(double) * nq); memcpy(in + nq, v, sizeof(double) * nv); memcpy(in + nq + nv, off, sizeof(double) * 3);
  double out[6 + 12 * DDP_MAXJ];
  const int rc = run(h, in, (size_t)(nq + nv + 3), out, (size_t)(6 + ((Jq || Jv) ? 12 * nv : 0)), 4, joint);
  if (rc != DDP_HIP_OK) return rc;
  memcpy(vel6, out, sizeof(double) * 6);
  if (Jq) memcpy(Jq, out + 6, sizeof(double) * 6 * nv);
  if (Jv) memcpy(Jv, out + 6 + 6 * nv, sizeof(double) * 6 * nv);
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_model_centroidal_momentum(ddp_hip_model_handle* h, const double* q, const double* v, double* h6, double* Jq, double* Jv) {
  if (!h || !q || !v || !h6 || h->model_h.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_ARG;
  const int nv = h->model_h.nv, nq = h->model_h.nq;
  double total = 0.0;
  for (int i = 0; i < h->model_h.nj; ++i) total += h->model_h.I6[i][9];   // the body masses (ctx.hip: pack_body_inertia)
  if (!(total > 0.0)) return DDP_HIP_E_ARG;
  double in[2 * DDP_MAXJ + 1];
  memcpy(in, q, sizeof(double) * nq); memcpy(in + nq, v, sizeof(double) * nv);
  double out[6 + 12 * DDP_MAXJ];
  const int rc = run(h, in, (size_t)(nq + nv), out, (size_t)(6 + ((Jq || Jv) ? 12 * nv : 0)), 5, 0);
  if (rc != DDP_HIP_OK) return rc;
  memcpy(h6, out, sizeof(double) * 6);
  if (Jq) memcpy(Jq, out + 6, sizeof(double) * 6 * nv);
  if (Jv) memcpy(Jv, out + 6 + 6 * nv, sizeof(double) * 6 * nv);
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_model_relative_frame(ddp_hip_model_handle* h, int32_t joint_a, const double off_a[3], int32_t joint_b, const double off_b[3],
                                            const double* q, double* p3, double* quat4, double* J) {
  if (!h || !off_a || !off_b || !q || !p3 || !quat4 || h->model_h.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_ARG;
  const int nv = h->model_h.nv, nq = h->model_h.nq, nj = h->model_h.nj;
  if (joint_a < 0 || joint_a >= nj || joint_b < 0 || joint_b >= nj || joint_a == joint_b) return DDP_HIP_E_ARG;
  double in[DDP_MAXJ + 1 + 6];
  memcpy(in, q, sizeof(double) * nq); memcpy(in + nq, off_a, sizeof(double) * 3); memcpy(in + nq + 3, off_b, sizeof(double) * 3);
  double out[7 + 6 * DDP_MAXJ];
  const int rc = run(h, in, (size_t)(nq + 6), out, (size_t)(7 + (J ? 6 * nv : 0)), 6, joint_a + DDP_MAXJ * joint_b);
  if (rc != DDP_HIP_OK) return rc;
  memcpy(p3, out, sizeof(double) * 3);
  memcpy(quat4, out + 3, sizeof(double) * 4);
  if (J) memcpy(J, out + 7, sizeof(double) * 6 * nv);
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_model_gravity_torque(ddp_hip_model_handle* h, const double* q, double* g, double* G) {
  if (!h || !q || !g || h->model_h.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_ARG;
  const size_t nv = (size_t)h->model_h.nv;
  double* out = new (std::nothrow) double[nv + nv * nv];
  if (!out) return DDP_HIP_E_HIP;
  const int rc = run(h, q, (size_t)h->model_h.nq, out, nv + (G ? nv * nv : 0), 7, G ? 1 : 0);
  if (rc == DDP_HIP_OK) {
    memcpy(g, out, sizeof(double) * nv);
    if (G) memcpy(G, out + nv, sizeof(double) * nv * nv);
  }
  delete[] out;
  return rc;
}

extern "C" int ddp_hip_model_frame_axis(ddp_hip_model_handle* h, int32_t joint, const double off[3], const double axis[3], const double* q, double* p3,
                                        double* n3, double* J) {
  if (!h || !off || !axis || !q || !p3 || !n3 || h->model_h.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_ARG;
  const int nv = h->model_h.nv, nq = h->model_h.nq;
  if (!cost_aim_frames_ok(h->model_h.nj, 1, &joint, off, axis)) return DDP_HIP_E_ARG;
  double in[DDP_MAXJ + 1 + 6];
  memcpy(in, q, sizeof(double) * nq); memcpy(in + nq, off, sizeof(double) * 3); memcpy(in + nq + 3, axis, sizeof(double) * 3);
  double out[6 + 6 * DDP_MAXJ];
  const int rc = run(h, in, (size_t)(nq + 6), out, (size_t)(6 + (J ? 6 * nv : 0)), 8, joint);
  if (rc != DDP_HIP_OK) return rc;
  memcpy(p3, out, sizeof(double) * 3);
  memcpy(n3, out + 3, sizeof(double) * 3);
  if (J) memcpy(J, out + 6, sizeof(double) * 6 * nv);
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_model_capture_point(ddp_hip_model_handle* h, const double* q, const double* v, double tau, double* xi3, double* Jq, double* Jv) {
  if (!h || !q || !v || !xi3 || h->model_h.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_ARG;
  if (!isfinite(tau) || tau < 0.0) return DDP_HIP_E_ARG;
  const int nv = h->model_h.nv, nq = h->model_h.nq;
  double total = 0.0;
  for (int i = 0; i < h->model_h.nj; ++i) total += h->model_h.I6[i][9];   // the body masses (ctx.hip: pack_body_inertia)
  if (!(total > 0.0)) return DDP_HIP_E_ARG;
  double in[2 * DDP_MAXJ + 2];
  memcpy(in, q, sizeof(double) * nq); memcpy(in + nq, v, sizeof(double) * nv);
  in[nq + nv] = tau;
  double out[3 + 6 * DDP_MAXJ];
  const int rc = run(h, in, (size_t)(nq + nv + 1), out, (size_t)(3 + ((Jq || Jv) ? 6 * nv : 0)), 9, 0);
  if (rc != DDP_HIP_OK) return rc;
  memcpy(xi3, out, sizeof(double) * 3);
  if (Jq) memcpy(Jq, out + 3, sizeof(double) * 3 * nv);
  if (Jv) memcpy(Jv, out + 3 + 3 * nv, sizeof(double) * 3 * nv);
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_model_capsule_pair(ddp_hip_model_handle* h, int32_t ja, const double a0[3], const double a1[3], int32_t jb, const double b0[3],
                                          const double b1[3], const double* q, double* D, double* ca3, double* cb3, double* J) {
  if (!h || !a0 || !a1 || !b0 || !b1 || !q || !D || !ca3 || !cb3 || h->model_h.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_ARG;
  const int nv = h->model_h.nv, nq = h->model_h.nq, nj = h->model_h.nj;
  if (ja < 0 || ja >= nj || jb < 0 || jb >= nj || ja == jb) return DDP_HIP_E_ARG;
  double in[DDP_MAXJ + 1 + 12];
  memcpy(in, q, sizeof(double) * nq);
  memcpy(in + nq, a0, sizeof(double) * 3); memcpy(in + nq + 3, a1, sizeof(double) * 3);
  memcpy(in + nq + 6, b0, sizeof(double) * 3); memcpy(in + nq + 9, b1, sizeof(double) * 3);
  for (int k = 0; k < 12; ++k)
    if (!isfinite(in[nq + k])) return DDP_HIP_E_ARG;
  double out[7 + DDP_MAXJ];
  const int rc = run(h, in, (size_t)(nq + 12), out, (size_t)(7 + (J ? nv : 0)), 10, ja + DDP_MAXJ * jb);
  if (rc != DDP_HIP_OK) return rc;
  *D = out[0];
  memcpy(ca3, out + 1, sizeof(double) * 3);
  memcpy(cb3, out + 4, sizeof(double) * 3);
  if (J) memcpy(J, out + 7, sizeof(double) * nv);
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_model_capsule_box(ddp_hip_model_handle* h, int32_t joint, const double a0[3], const double a1[3], double radius,
                                         const double half[3], const double pose[7], const double* q, double* d, double* s, double ca[3],
                                         double u[3], double* grad) {
  if (!h || !a0 || !a1 || !half || !pose || !q || !d || !s || !ca || !u || h->model_h.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_ARG;
  const int nv = h->model_h.nv, nq = h->model_h.nq, nj = h->model_h.nj;
  if (joint < 0 || joint >= nj || !isfinite(radius) || radius < 0.0) return DDP_HIP_E_ARG;
  double in[DDP_MAXJ + 1 + 17];
  memcpy(in, q, sizeof(double) * nq);
  memcpy(in + nq, a0, sizeof(double) * 3); memcpy(in + nq + 3, a1, sizeof(double) * 3);
  memcpy(in + nq + 6, half, sizeof(double) * 3); memcpy(in + nq + 9, pose, sizeof(double) * 7);
  in[nq + 16] = radius;
  for (int k = 0; k < 16; ++k)
    if (!isfinite(in[nq + k])) return DDP_HIP_E_ARG;
  if (!(half[0] > 0.0) || !(half[1] > 0.0) || !(half[2] > 0.0)) return DDP_HIP_E_ARG;
  if (!cost_quat_ok(pose[3] * pose[3] + pose[4] * pose[4] + pose[5] * pose[5] + pose[6] * pose[6])) return DDP_HIP_E_ARG;
  double out[8 + DDP_MAXJ];
  const int rc = run(h, in, (size_t)(nq + 17), out, (size_t)(8 + (grad ? nv : 0)), 11, joint);
  if (rc != DDP_HIP_OK) return rc;
  *d = out[0];
  *s = out[1];
  memcpy(ca, out + 2, sizeof(double) * 3);
  memcpy(u, out + 5, sizeof(double) * 3);
  if (grad) memcpy(grad, out + 8, sizeof(double) * nv);
  return DDP_HIP_OK;
}
