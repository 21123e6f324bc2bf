// rbd_deriv.h -- analytic partial derivatives of the forward dynamics of a tree of 1-DoF joints: what the reference's
// first_order_deriv (problem.hpp:463-503) takes from model_t::d_dynamics_aba (pinocchio_model.ipp:359-400, i.e.
// Pinocchio's computeABADerivatives; Pinocchio is absent, the recursion is restated from Carpentier & Mansard,
// "Analytical derivatives of rigid body dynamics algorithms", RSS 2018):
//     d qdd/dq = -M^-1 d tau/dq,   d qdd/dv = -M^-1 d tau/dv,   d qdd/d tau = M^-1,     tau = RNEA(q, v, qdd)
// with the partials of the inverse dynamics formed in WORLD coordinates.  J_i: world-frame axis of joint i (a spatial
// motion vector [angular; linear]); ov, oa: world-frame body velocities / accelerations (gravity folded into a_0);
// I_k: world-frame body inertia; h = I ov; of = I oa + ov x* h; B_k x = I_k (x x ov_k) + x x* h_k + ov_k x* (I_k x);
// Ic, Bc, ofc: sums over the subtree.  Then
//     u_j = J_j x ov_j,   g_j = u_j x ov_j - J_j x oa_j
//     i in path(j):           d tau_i/dq_j = J_i . (J_j x* ofc_j - Bc_j u_j + Ic_j g_j)
//                             d tau_i/dv_j = J_i . (Bc_j J_j - 2 Ic_j u_j),      M_ij = J_i . Ic_j J_j
//     j proper ancestor of i: d tau_i/dq_j = -(Bc_i^T J_i) . u_j + (Ic_i J_i) . g_j
//                             d tau_i/dv_j =  (Bc_i^T J_i) . J_j - 2 (Ic_i J_i) . u_j
// (derivation: DESIGN.md section 4b).  This header holds the pieces shared by the one-lane-per-evaluation variant
// (small models: the constraint chain and mode 1 of the UR5-like drivers) and the wave-per-evaluation kernels
// (lin_analytic.hip, the Talos-like tree).
#pragma once

#include "rbd.h"

namespace rbdd {

using rbd::cross3;
using rbd::crf;
using rbd::crm;
using rbd::mm3;
using rbd::mv3;

// world placement of joint i from its parent's: oR (row-major, world = oR * joint coordinates), op
__device__ __forceinline__ void world_placement(const DevModel& m, int i, double q, const double* oRp, const double* opp,
                                                double* oR, double* op) {
  double E[9], r[3], Rc[9];
  rbd::joint_placement(m, i, q, E, r);
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int l = 0; l < 3; ++l) Rc[3 * k + l] = E[3 * l + k];
  if (oRp) {
    double t[3];
    mm3(oRp, Rc, oR);
    mv3(oRp, r, t);
#pragma unroll
    for (int k = 0; k < 3; ++k) op[k] = opp[k] + t[k];
  } else {
#pragma unroll
    for (int k = 0; k < 9; ++k) oR[k] = Rc[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) op[k] = r[k];
  }
}

// J_i: the joint axis as a world-frame spatial motion vector (the linear part is the velocity of the body point that
// coincides with the world origin)
__device__ __forceinline__ void world_axis(const DevModel& m, int i, const double* oR, const double* op, double* J) {
  double aw[3];
  mv3(oR, m.axis[i], aw);
  if (m.jtype[i] == DDP_HIP_JOINT_REVOLUTE) {
    double t[3];
    cross3(op, aw, t);
    J[0] = aw[0]; J[1] = aw[1]; J[2] = aw[2]; J[3] = t[0]; J[4] = t[1]; J[5] = t[2];
  } else {
    J[0] = 0.0; J[1] = 0.0; J[2] = 0.0; J[3] = aw[0]; J[4] = aw[1]; J[5] = aw[2];
  }
}

// y = A x for a row-major 6 x 6 (ld 6), y = A^T x
__device__ __forceinline__ void m6v(const double* A, const double* x, double* y) {
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    double s = 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) s += A[6 * r + c] * x[c];
    y[r] = s;
  }
}
__device__ __forceinline__ void m6tv(const double* A, const double* x, double* y) {
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double s = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) s += A[6 * r + c] * x[r];
    y[c] = s;
  }
}

// world-frame spatial inertia (about the world origin) of the body of joint i: full 6 x 6, row-major.
// I6b is the body-frame inertia packed as in DevModel::I6 (lower triangle): I_world = X^-T I_body X^-1 is formed from
// the mass, the world-frame centre of mass and the rotated rotational inertia about the centre of mass.
__device__ __forceinline__ void world_inertia(const double* I6b, const double* oR, const double* op, double* I6) {
  // body frame: I6b = [Io, m cx; m cx^T, m 1] with Io about the joint origin; mass = I6b(3,3); m c = (I6b(2,4)... )
  const double mass = I6b[rbd::sidx(3, 3)];
  // m cx = [[0,-mcz,mcy],[mcz,0,-mcx],[-mcy,mcx,0]] stored at rows 0..2, cols 3..5
  const double mc[3] = {I6b[rbd::sidx(2, 4)], I6b[rbd::sidx(0, 5)], I6b[rbd::sidx(1, 3)]};   // (m cx)(2,1), (0,2), (1,0)
  double Io[9];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int l = 0; l < 3; ++l) Io[3 * k + l] = I6b[rbd::sidx(k, l)];
  // rotate: Io_w = oR Io oR^T (about the joint origin, world axes); m c_w = oR (m c)
  double T1[9], Iw[9], mcw[3];
  mm3(oR, Io, T1);
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int l = 0; l < 3; ++l) Iw[3 * k + l] = T1[3 * k] * oR[3 * l] + T1[3 * k + 1] * oR[3 * l + 1] + T1[3 * k + 2] * oR[3 * l + 2];
  mv3(oR, mc, mcw);
  // shift the reference point from the joint origin to the world origin: with d = op (joint origin in world coordinates),
  // m c_O = m c_w + m d;  I_O = I_w + (m c_w)x dx^T ... written out: I_O = I_w - [mcw]x [d]x - [d]x [mcw]x - m [d]x [d]x
  const double d[3] = {op[0], op[1], op[2]};
  const double mco[3] = {mcw[0] + mass * d[0], mcw[1] + mass * d[1], mcw[2] + mass * d[2]};
  const double cxw[9] = {0, -mcw[2], mcw[1], mcw[2], 0, -mcw[0], -mcw[1], mcw[0], 0};
  const double dx[9] = {0, -d[2], d[1], d[2], 0, -d[0], -d[1], d[0], 0};
  double A1[9], A2[9], A3[9];
  mm3(cxw, dx, A1);
  mm3(dx, cxw, A2);
  mm3(dx, dx, A3);
#pragma unroll
  for (int k = 0; k < 36; ++k) I6[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int l = 0; l < 3; ++l) I6[6 * k + l] = Iw[3 * k + l] - A1[3 * k + l] - A2[3 * k + l] - mass * A3[3 * k + l];
  const double cx[9] = {0, -mco[2], mco[1], mco[2], 0, -mco[0], -mco[1], mco[0], 0};
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int l = 0; l < 3; ++l) { I6[6 * k + l + 3] = cx[3 * k + l]; I6[6 * (k + 3) + l] = cx[3 * l + k]; }
  I6[21] = mass; I6[28] = mass; I6[35] = mass;
}

// B x = I (x x ov) + x x* h + ov x* (I x), column by column (row-major 6 x 6)
__device__ __forceinline__ void bias_matrix(const double* I6, const double* ov, const double* h, double* B) {
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    double e[6] = {0, 0, 0, 0, 0, 0}, exv[6], t1[6], t2[6], Icol[6], t3[6];
    e[c] = 1.0;
    crm(e, ov, exv);
    m6v(I6, exv, t1);
    crf(e, h, t2);
#pragma unroll
    for (int k = 0; k < 6; ++k) Icol[k] = I6[6 * k + c];
    crf(ov, Icol, t3);
#pragma unroll
    for (int k = 0; k < 6; ++k) B[6 * k + c] = t1[k] + t2[k] + t3[k];
  }
}

// Cholesky M = L L^T in place on the lower triangle (column-major, ld), then Minv = M^-1 (full, column-major, ld):
// the columns of the identity through the two substitutions.  One lane does everything: small models only.
template <int NJ>
__device__ void chol_inverse_lane(int N, double* M, double* Minv) {
  for (int k = 0; k < N; ++k) {
    double x = M[k + k * NJ];
    for (int j = 0; j < k; ++j) x -= M[k + j * NJ] * M[k + j * NJ];
    x = sqrt(x);
    M[k + k * NJ] = x;
    for (int i = k + 1; i < N; ++i) {
      double s = M[i + k * NJ];
      for (int j = 0; j < k; ++j) s -= M[i + j * NJ] * M[k + j * NJ];
      M[i + k * NJ] = s / x;
    }
  }
  for (int c = 0; c < N; ++c) {
    double* b = Minv + c * NJ;
    for (int i = 0; i < N; ++i) {
      double s = i == c ? 1.0 : 0.0;
      for (int l = 0; l < i; ++l) s -= M[i + l * NJ] * b[l];
      b[i] = s / M[i + i * NJ];
    }
    for (int i = N - 1; i >= 0; --i) {
      double s = b[i];
      for (int l = i + 1; l < N; ++l) s -= M[l + i * NJ] * b[l];
      b[i] = s / M[i + i * NJ];
    }
  }
}

// One lane: partials of qdd = ABA(q, v, tau).  dq, dv, dtau: nv x nv column-major with leading dimension nv.
// Private state O(NJ * 100) doubles: meant for NJ <= 6.
template <int NJ>
__device__ void aba_derivatives_lane(const DevModel& m, const double* q, const double* v, const double* tau, double* qdd,
                                     double* dq, double* dv, double* dtau) {
  const int N = m.nv;
  rbd::aba_tree<NJ>(m, q, v, tau, qdd);
  double oR[NJ][9], op[NJ][3], J[NJ][6], ov[NJ][6], oa[NJ][6], Ic[NJ][36], Bc[NJ][36], ofc[NJ][6];
  for (int i = 0; i < N; ++i) {
    const int par = m.parent[i];
    world_placement(m, i, q[i], par >= 0 ? oR[par] : nullptr, par >= 0 ? op[par] : nullptr, oR[i], op[i]);
    world_axis(m, i, oR[i], op[i], J[i]);
    double vJ[6], t6[6];
    for (int k = 0; k < 6; ++k) vJ[k] = J[i][k] * v[i];
    for (int k = 0; k < 6; ++k) ov[i][k] = (par >= 0 ? ov[par][k] : 0.0) + vJ[k];
    crm(ov[i], vJ, t6);
    for (int k = 0; k < 6; ++k) {
      const double ap = par >= 0 ? oa[par][k] : (k < 3 ? 0.0 : -m.gravity[k - 3]);
      oa[i][k] = ap + J[i][k] * qdd[i] + t6[k];
    }
    world_inertia(m.I6[i], oR[i], op[i], Ic[i]);
    double h[6], Ioa[6], vxh[6];
    m6v(Ic[i], ov[i], h);
    m6v(Ic[i], oa[i], Ioa);
    crf(ov[i], h, vxh);
    for (int k = 0; k < 6; ++k) ofc[i][k] = Ioa[k] + vxh[k];
    bias_matrix(Ic[i], ov[i], h, Bc[i]);
  }
  for (int i = N - 1; i >= 0; --i) {
    const int par = m.parent[i];
    if (par < 0) continue;
    for (int k = 0; k < 36; ++k) { Ic[par][k] += Ic[i][k]; Bc[par][k] += Bc[i][k]; }
    for (int k = 0; k < 6; ++k) ofc[par][k] += ofc[i][k];
  }
  double y[NJ][6], z[NJ][6], u[NJ][6], g[NJ][6], Fq[NJ][6], Fv[NJ][6];
  for (int i = 0; i < N; ++i) {
    double t1[6], t2[6], t3[6];
    m6v(Ic[i], J[i], y[i]);
    m6tv(Bc[i], J[i], z[i]);
    crm(J[i], ov[i], u[i]);
    crm(u[i], ov[i], t1);
    crm(J[i], oa[i], t2);
    for (int k = 0; k < 6; ++k) g[i][k] = t1[k] - t2[k];
    crf(J[i], ofc[i], t1);
    m6v(Bc[i], u[i], t2);
    m6v(Ic[i], g[i], t3);
    for (int k = 0; k < 6; ++k) Fq[i][k] = t1[k] - t2[k] + t3[k];
    m6v(Bc[i], J[i], t1);
    m6v(Ic[i], u[i], t2);
    for (int k = 0; k < 6; ++k) Fv[i][k] = t1[k] - 2.0 * t2[k];
  }
  double M[NJ * NJ], Tq[NJ * NJ], Tv[NJ * NJ], Minv[NJ * NJ];
  for (int k = 0; k < NJ * NJ; ++k) { M[k] = 0.0; Tq[k] = 0.0; Tv[k] = 0.0; }
  for (int j = 0; j < N; ++j) {
    for (int i = j; i >= 0; i = m.parent[i]) {
      double sq = 0, sv = 0, sm = 0;
      for (int k = 0; k < 6; ++k) { sq += J[i][k] * Fq[j][k]; sv += J[i][k] * Fv[j][k]; sm += J[i][k] * y[j][k]; }
      Tq[i + j * NJ] = sq; Tv[i + j * NJ] = sv;
      M[i + j * NJ] = sm; M[j + i * NJ] = sm;
    }
    for (int a = m.parent[j]; a >= 0; a = m.parent[a]) {
      double s1 = 0, s2 = 0, s3 = 0, s4 = 0;
      for (int k = 0; k < 6; ++k) { s1 += z[j][k] * u[a][k]; s2 += y[j][k] * g[a][k]; s3 += z[j][k] * J[a][k]; s4 += y[j][k] * u[a][k]; }
      Tq[j + a * NJ] = -s1 + s2;
      Tv[j + a * NJ] = s3 - 2.0 * s4;
    }
  }
  for (int i = 0; i < N; ++i) M[i + i * NJ] += m.armature[i];   // M + diag(armature)
  chol_inverse_lane<NJ>(N, M, Minv);
  for (int c = 0; c < N; ++c)
    for (int r = 0; r < N; ++r) {
      double sq = 0, sv = 0;
      for (int l = 0; l < N; ++l) { sq += Minv[r + l * NJ] * Tq[l + c * NJ]; sv += Minv[r + l * NJ] * Tv[l + c * NJ]; }
      dq[r + c * N] = -sq;
      dv[r + c * N] = -sv;
      dtau[r + c * N] = Minv[r + c * NJ];
    }
}

// first_order_deriv (problem.hpp:463-503) on a vector space: fx = [I, dt I; dt da/dq, I + dt da/dv], fu = [0; dt da/dtau]
template <int NJ>
__device__ void first_order_analytic_lane(const DevModel& m, const double* x, const double* u, double* fx, double* fu, double* f) {
  const int nv = m.nv, n = 2 * nv;
  double qdd[NJ], dq[NJ * NJ], dv[NJ * NJ], dt_[NJ * NJ];
  aba_derivatives_lane<NJ>(m, x, x + nv, u, qdd, dq, dv, dt_);
  for (int i = 0; i < nv; ++i) {                       // eval_to (:441-461)
    const double vo = m.dt * x[nv + i];
    f[i] = x[i] + vo;
    f[nv + i] = x[nv + i] + qdd[i] * m.dt;
  }
  for (int k = 0; k < n * n; ++k) fx[k] = 0.0;
  for (int k = 0; k < n * nv; ++k) fu[k] = 0.0;
  for (int j = 0; j < nv; ++j) {
    fx[j + j * n] = 1.0;
    fx[j + (nv + j) * n] = 1.0 * m.dt;
    for (int i = 0; i < nv; ++i) {
      fx[(nv + i) + j * n] = dq[i + j * nv] * m.dt;
      fx[(nv + i) + (nv + j) * n] = dv[i + j * nv] * m.dt + (i == j ? 1.0 : 0.0);
      fu[(nv + i) + j * n] = dt_[i + j * nv] * m.dt;
    }
  }
}

// ---- free-flyer root (SE(3), lie.h), one wave per evaluation ---------------------------------------------------------------
// The root contributes six columns J_0 .. J_5: the body-frame unit twists [linear; angular] of Pinocchio's JointModelFreeFlyer,
// expressed in world coordinates (J_k = oX_0 e_k).  Derivatives are taken along q (+) delta = integrate(q, delta), a right
// perturbation: perturbing column k of the root moves the whole tree rigidly by exp(J_k delta) in the world, exactly as a 1-DoF
// joint moves its subtree.  What differs:
//   - every root column lies in the "subtree" of every other one: d J_l / dq_k = J_k x J_l for all k, l of the root, so a
//     root-root entry takes the proper-ancestor form (which carries the rotation of J_i) in both orders;
//   - the root's parent is the world: u_k = J_k x 0 = 0 and g_k = -J_k x a_grav (a_grav = [0; -gravity], the world's
//     acceleration), and the root's velocity term is J_dot v = ov_0 x ov_0 = 0;
//   - d oa / dv_k = J_k x (ov - ov_0) below the root (the root's own acceleration carries no velocity term), so the velocity
//     partials use w_k = J_k x ov_0 where a 1-DoF joint has 2 u_j.
// With these, for columns i (row) and j (column) whose bodies lie on one path:
//   body(i) a proper ancestor of body(j), or i == j (1-DoF):  d tau_i/dq_j = J_i . Fq_j,  d tau_i/dv_j = J_i . Fv_j
//       Fq_j = J_j x* ofc_j - Bc_j u_j + Ic_j g_j,  Fv_j = Bc_j J_j - Ic_j w_j
//   body(j) a proper ancestor of body(i), or both in the root:  d tau_i/dq_j = -z_i . u_j + y_i . g_j,  d tau_i/dv_j = z_i . J_j - y_i . w_j
//       y_i = Ic_i J_i, z_i = Bc_i^T J_i;   M_ij = J_i . Ic J_j over the deeper body's composite inertia.
// The trajectory point's acceleration is formed here as well, from the same recursion: qdd = M^-1 (tau - RNEA(q, v, 0)).
// Column c belongs to body 0 (c < 6) or to joint c - 5; joint i >= 1 reads q[i + 6], v[i + 5] (rbd::place, rbd::aba_tree).
__device__ __forceinline__ int ff_body(int c) { return c < 6 ? 0 : c - 5; }

// LDS layout (doubles).  Body records (102): oR 9 | op 3 | ov 6 | oa 6 | Ic 36 | Bc 36 | f 6 (Ic | Bc | f: the subtree sums once
// they are formed); column records (48): J 6 | u 6 | g 6 | w 6 | y 6 | z 6 | Fq 6 | Fv 6.  T = [d tau/dq | d tau/dv] (nv x 2 nv,
// row-major) goes over the body records once they are spent; M is factorised in place (its lower triangle, column-major,
// ld nv), M^-1 is formed in X (column-major, ld nv).
template <int NJ> struct FfLds {
  static constexpr int BR = 102, CR = 48;
  static constexpr int LOC = 0, BOD = LOC + 12 * NJ, M = BOD + BR * NJ, COL = M + NJ * NJ, X = COL + CR * NJ, VEC = X + NJ * NJ,
                       PAR = VEC + 5 * NJ + 1, TOTAL = PAR + NJ;
  static constexpr int T = BOD;
  static_assert(BR * NJ >= 2 * NJ * NJ, "T must fit over the body records");
};

// Partials of qdd = ABA(q, v, tau) for a free-flyer model in the tangent (nq = nv + 1): leaves T in lds + FfLds::T and M^-1 in
// lds + FfLds::X, so that d qdd/dq = -M^-1 T(:, 0:nv), d qdd/dv = -M^-1 T(:, nv:2nv), d qdd/dtau = M^-1 (ff_minv_T_row).  Called by
// every thread of a one-wave work-group; q, v, tau may be global.  nv <= NJ <= 64.
template <int NJ>
__device__ void ff_derivatives_wave(const DevModel& m, const double* q, const double* v, const double* tau, double* lds, int lane) {
  typedef FfLds<NJ> L;
  constexpr int BR = L::BR, CR = L::CR;
  const int N = m.nv, NB = m.nj, W2 = 2 * N;
  const int nth = blockDim.x;
  double* s_loc = lds + L::LOC;
  double* s_bod = lds + L::BOD;
  double* s_M = lds + L::M;
  double* s_col = lds + L::COL;
  double* s_X = lds + L::X;
  double* s_q = lds + L::VEC;
  double* s_v = s_q + NJ + 1;
  double* s_tau = s_v + NJ;
  double* s_rhs = s_tau + NJ;
  double* s_qdd = s_rhs + NJ;
  int* s_par = reinterpret_cast<int*>(lds + L::PAR);
  for (int k = lane; k <= N; k += nth) s_q[k] = q[k];
  for (int k = lane; k < N; k += nth) { s_v[k] = v[k]; s_tau[k] = tau[k]; }
  for (int k = lane; k < NB; k += nth) s_par[k] = m.parent[k];
  for (int k = lane; k < N * N; k += nth) s_M[k] = 0.0;
  __syncthreads();
  // joint placements (parent coordinates = Rc child coordinates + r), then world placements along each body's path
  if (lane < NB) {
    double E[9], r[3];
    rbd::place(m, lane, s_q, E, r);
    double* o = s_loc + 12 * lane;
    for (int k = 0; k < 3; ++k)
      for (int l = 0; l < 3; ++l) o[3 * k + l] = E[3 * l + k];
    for (int k = 0; k < 3; ++k) o[9 + k] = r[k];
  }
  __syncthreads();
  if (lane < NB) {
    double oR[9], op[3];
    const double* o = s_loc + 12 * lane;
    for (int k = 0; k < 9; ++k) oR[k] = o[k];
    for (int k = 0; k < 3; ++k) op[k] = o[9 + k];
    for (int a = s_par[lane]; a >= 0; a = s_par[a]) {
      const double* wa = s_loc + 12 * a;
      double t9[9], t3[3];
      mm3(wa, oR, t9);
      mv3(wa, op, t3);
      for (int k = 0; k < 9; ++k) oR[k] = t9[k];
      for (int k = 0; k < 3; ++k) op[k] = wa[9 + k] + t3[k];
    }
    double* br = s_bod + BR * lane;
    for (int k = 0; k < 9; ++k) br[k] = oR[k];
    for (int k = 0; k < 3; ++k) br[9 + k] = op[k];
  }
  __syncthreads();
  // column axes J_c and J_c v_c (parked in the u slot)
  if (lane < N) {
    const int bc = ff_body(lane);
    const double* br = s_bod + BR * bc;
    double J[6];
    if (lane < 6) {
      const int k = lane % 3;
      const double aw[3] = {br[k], br[3 + k], br[6 + k]};   // oR e_k
      if (lane < 3) { J[0] = 0.0; J[1] = 0.0; J[2] = 0.0; J[3] = aw[0]; J[4] = aw[1]; J[5] = aw[2]; }
      else { double t[3]; cross3(br + 9, aw, t); J[0] = aw[0]; J[1] = aw[1]; J[2] = aw[2]; J[3] = t[0]; J[4] = t[1]; J[5] = t[2]; }
    } else {
      world_axis(m, bc, br, br + 9, J);
    }
    double* cr = s_col + CR * lane;
    for (int k = 0; k < 6; ++k) { cr[k] = J[k]; cr[6 + k] = J[k] * s_v[lane]; }
  }
  __syncthreads();
  // body velocities: ov_b = sum over the columns of the path of J_c v_c
  if (lane < NB) {
    double ov[6] = {0, 0, 0, 0, 0, 0};
    for (int a = lane; a >= 0; a = s_par[a]) {
      const int c0 = a == 0 ? 0 : a + 5, c1 = a == 0 ? 6 : a + 6;
      for (int c = c0; c < c1; ++c)
        for (int k = 0; k < 6; ++k) ov[k] += s_col[CR * c + 6 + k];
    }
    for (int k = 0; k < 6; ++k) s_bod[BR * lane + 12 + k] = ov[k];
  }
  __syncthreads();
  // velocity-product terms of the 1-DoF columns, ov_body x J_c v_c (parked in the g slot; the root's is zero)
  if (lane < N) {
    double* cr = s_col + CR * lane;
    if (lane < 6) { for (int k = 0; k < 6; ++k) cr[12 + k] = 0.0; }
    else crm(s_bod + BR * ff_body(lane) + 12, cr + 6, cr + 12);
  }
  __syncthreads();
  // per body at qdd = 0: oa0 = a_grav + path sum of the velocity products; world inertia, bias matrix, force f0 = I oa0 + ov x* I ov
  if (lane < NB) {
    double* br = s_bod + BR * lane;
    double oa[6] = {0, 0, 0, -m.gravity[0], -m.gravity[1], -m.gravity[2]};
    for (int a = lane; a >= 1; a = s_par[a])
      for (int k = 0; k < 6; ++k) oa[k] += s_col[CR * (a + 5) + 12 + k];
    double I6[36], B[36], h[6], Ioa[6], vxh[6];
    world_inertia(m.I6[lane], br, br + 9, I6);
    m6v(I6, br + 12, h);
    m6v(I6, oa, Ioa);
    crf(br + 12, h, vxh);
    bias_matrix(I6, br + 12, h, B);
    for (int k = 0; k < 6; ++k) { br[18 + k] = oa[k]; br[96 + k] = Ioa[k] + vxh[k]; }
    for (int k = 0; k < 36; ++k) { br[24 + k] = I6[k]; br[60 + k] = B[k]; }
  }
  __syncthreads();
  // subtree sums leaves -> root (Ic | Bc | f0): a thread only ever touches its own entries, children precede parents
  for (int i = NB - 1; i >= 1; --i) {
    const int par = s_par[i];
    for (int k = lane; k < 78; k += nth) s_bod[BR * par + 24 + k] += s_bod[BR * i + 24 + k];
  }
  __syncthreads();
  // y_c = Ic J_c; the bias torques J_c . f0c; M's lower triangle: M(c, i) = J_i . y_c for the columns i <= c on c's path
  if (lane < N) {
    const int bc = ff_body(lane);
    const double* br = s_bod + BR * bc;
    double* cr = s_col + CR * lane;
    double y[6], bias = 0.0;
    m6v(br + 24, cr, y);
    for (int k = 0; k < 6; ++k) { cr[24 + k] = y[k]; bias += cr[k] * br[96 + k]; }
    s_rhs[lane] = s_tau[lane] - bias;
    for (int a = bc; a >= 0; a = s_par[a]) {
      const int c0 = a == 0 ? 0 : a + 5, c1 = a == 0 ? (bc == 0 ? lane + 1 : 6) : a + 6;   // (the root's columns: i <= c among themselves)
      for (int i = c0; i < c1; ++i) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += s_col[CR * i + k] * y[k];
        s_M[lane + i * N] = s;
      }
    }
    s_M[lane + lane * N] += m.armature[bc];   // M + diag(armature); the root's six columns carry none (armature[0] is 0 there)
  }
  __syncthreads();
  // Cholesky M = L L^T in place (lower triangle): thread r owns row r
  for (int k = 0; k < N; ++k) {
    const double dk = sqrt(s_M[k + k * N]);
    __syncthreads();
    if (lane == k) s_M[k + k * N] = dk;
    if (lane > k && lane < N) s_M[lane + k * N] = s_M[lane + k * N] / dk;
    __syncthreads();
    if (lane > k && lane < N) {
      const double lrk = s_M[lane + k * N];
      for (int c = k + 1; c <= lane; ++c) s_M[lane + c * N] -= lrk * s_M[c + k * N];
    }
    __syncthreads();
  }
  // M^-1: thread c solves L L^T x = e_c into column c of X
  if (lane < N) {
    double* x = s_X + lane * N;
    for (int i = 0; i < N; ++i) {
      double s = i == lane ? 1.0 : 0.0;
      for (int l = 0; l < i; ++l) s -= s_M[i + l * N] * x[l];
      x[i] = s / s_M[i + i * N];
    }
    for (int i = N - 1; i >= 0; --i) {
      double s = x[i];
      for (int l = i + 1; l < N; ++l) s -= s_M[l + i * N] * x[l];
      x[i] = s / s_M[i + i * N];
    }
  }
  __syncthreads();
  if (lane < N) {
    double s = 0.0;
    for (int l = 0; l < N; ++l) s += s_X[lane + l * N] * s_rhs[l];
    s_qdd[lane] = s;
  }
  __syncthreads();
  // accelerations: oa = oa0 + alpha, alpha_b = path sum of J_c qdd_c; forces I_b alpha_b (over the spent placements) summed
  // leaves -> root and added to f0c: ofc
  if (lane < NB) {
    double* br = s_bod + BR * lane;
    double al[6] = {0, 0, 0, 0, 0, 0};
    for (int a = lane; a >= 0; a = s_par[a]) {
      const int c0 = a == 0 ? 0 : a + 5, c1 = a == 0 ? 6 : a + 6;
      for (int c = c0; c < c1; ++c)
        for (int k = 0; k < 6; ++k) al[k] += s_col[CR * c + k] * s_qdd[c];
    }
    double I6[36], f[6];
    world_inertia(m.I6[lane], br, br + 9, I6);
    m6v(I6, al, f);
    for (int k = 0; k < 6; ++k) { br[18 + k] += al[k]; s_loc[12 * lane + k] = f[k]; }
  }
  __syncthreads();
  for (int i = NB - 1; i >= 1; --i) {
    const int par = s_par[i];
    for (int k = lane; k < 6; k += nth) s_loc[12 * par + k] += s_loc[12 * i + k];
  }
  __syncthreads();
  for (int k = lane; k < 6 * NB; k += nth) s_bod[BR * (k / 6) + 96 + k % 6] += s_loc[12 * (k / 6) + k % 6];
  __syncthreads();
  // column quantities u | g | w | z | Fq | Fv
  if (lane < N) {
    const int bc = ff_body(lane);
    const double* br = s_bod + BR * bc;
    double* cr = s_col + CR * lane;
    const double* J = cr;
    const double* ov = br + 12;
    double u[6], g[6], w[6], t1[6], t2[6], t3[6];
    m6tv(br + 60, J, cr + 30);                            // z
    if (lane < 6) {
      const double ag[6] = {0, 0, 0, -m.gravity[0], -m.gravity[1], -m.gravity[2]};
      crm(J, ag, t1);
      for (int k = 0; k < 6; ++k) { u[k] = 0.0; g[k] = -t1[k]; }
      crm(J, ov, w);
    } else {
      crm(J, ov, u);
      crm(u, ov, t1);
      crm(J, br + 18, t2);
      for (int k = 0; k < 6; ++k) { g[k] = t1[k] - t2[k]; w[k] = 2.0 * u[k]; }
    }
    for (int k = 0; k < 6; ++k) { cr[6 + k] = u[k]; cr[12 + k] = g[k]; cr[18 + k] = w[k]; }
    crf(J, br + 96, t1);
    m6v(br + 60, u, t2);
    m6v(br + 24, g, t3);
    for (int k = 0; k < 6; ++k) cr[36 + k] = t1[k] - t2[k] + t3[k];
    m6v(br + 60, J, t1);
    m6v(br + 24, w, t2);
    for (int k = 0; k < 6; ++k) cr[42 + k] = t1[k] - t2[k];
  }
  __syncthreads();
  double* s_T = lds + L::T;
  for (int k = lane; k < N * W2; k += nth) s_T[k] = 0.0;
  __syncthreads();
  // T: thread c walks the bodies of its path; it writes row c (columns i of the path) and column c of the rows of its proper
  // ancestors' columns -- no entry has two writers
  if (lane < N) {
    const int c = lane, bc = ff_body(c);
    const double* cc = s_col + CR * c;
    for (int a = bc; a >= 0; a = s_par[a]) {
      const int c0 = a == 0 ? 0 : a + 5, c1 = a == 0 ? 6 : a + 6;
      for (int i = c0; i < c1; ++i) {
        const double* ci = s_col + CR * i;
        if (a == bc && i == c && c >= 6) {                // a 1-DoF column with itself
          double sq = 0, sv = 0;
          for (int k = 0; k < 6; ++k) { sq += cc[k] * cc[36 + k]; sv += cc[k] * cc[42 + k]; }
          s_T[c * W2 + c] = sq;
          s_T[c * W2 + N + c] = sv;
          continue;
        }
        if (a != bc) {                                    // i on a proper ancestor: d tau_i / d(q, v)_c
          double sq = 0, sv = 0;
          for (int k = 0; k < 6; ++k) { sq += ci[k] * cc[36 + k]; sv += ci[k] * cc[42 + k]; }
          s_T[i * W2 + c] = sq;
          s_T[i * W2 + N + c] = sv;
        }
        double sq = 0, sv = 0;                            // d tau_c / d(q, v)_i: a proper ancestor, or both in the root
        for (int k = 0; k < 6; ++k) {
          sq += -cc[30 + k] * ci[6 + k] + cc[24 + k] * ci[12 + k];
          sv += cc[30 + k] * ci[k] - cc[24 + k] * ci[18 + k];
        }
        s_T[c * W2 + i] = sq;
        s_T[c * W2 + N + i] = sv;
      }
    }
  }
  __syncthreads();
}

// The fixed-base sibling of ff_derivatives_wave: partials of qdd = ABA(q, v, tau) for a tree of 1-DoF joints on a fixed base
// (nq = nv, column c = joint c = body c), the recursion of aba_derivatives_lane in the cooperative layout above -- one wave, lane =
// joint, the records of FfLds<NJ>.  It leaves T = [d tau/dq | d tau/dv] in lds + FfLds::T, M^-1 in lds + FfLds::X and qdd in the
// last NJ doubles of FfLds::VEC's run (wave_qdd), as ff_derivatives_wave does.  What falls away against the free flyer: every
// column is a 1-DoF column with a parent frame that moves (u = J x ov, g = u x ov - J x oa, w = 2 u), no two columns share a body,
// and the root joint's velocity product enters oa0 like any other (it is zero: ov_0 = J_0 v_0).  A forest (several joints with
// parent -1) is allowed.  Called by every thread of a one-wave work-group; q, v, tau may be global.  nv <= NJ <= 64.
template <int NJ>
__device__ void tree_derivatives_wave(const DevModel& m, const double* q, const double* v, const double* tau, double* lds, int lane) {
  typedef FfLds<NJ> L;
  constexpr int BR = L::BR, CR = L::CR;
  const int N = m.nv, W2 = 2 * N;
  const int nth = blockDim.x;
  double* s_loc = lds + L::LOC;
  double* s_bod = lds + L::BOD;
  double* s_M = lds + L::M;
  double* s_col = lds + L::COL;
  double* s_X = lds + L::X;
  double* s_q = lds + L::VEC;
  double* s_v = s_q + NJ + 1;
  double* s_tau = s_v + NJ;
  double* s_rhs = s_tau + NJ;
  double* s_qdd = s_rhs + NJ;
  int* s_par = reinterpret_cast<int*>(lds + L::PAR);
  for (int k = lane; k < N; k += nth) { s_q[k] = q[k]; s_v[k] = v[k]; s_tau[k] = tau[k]; s_par[k] = m.parent[k]; }
  for (int k = lane; k < N * N; k += nth) s_M[k] = 0.0;
  __syncthreads();
  // joint placements (parent coordinates = Rc child coordinates + r), then world placements along each joint's path
  if (lane < N) {
    double E[9], r[3];
    rbd::joint_placement(m, lane, s_q[lane], E, r);
    double* o = s_loc + 12 * lane;
    for (int k = 0; k < 3; ++k)
      for (int l = 0; l < 3; ++l) o[3 * k + l] = E[3 * l + k];
    for (int k = 0; k < 3; ++k) o[9 + k] = r[k];
  }
  __syncthreads();
  if (lane < N) {
    double oR[9], op[3];
    const double* o = s_loc + 12 * lane;
    for (int k = 0; k < 9; ++k) oR[k] = o[k];
    for (int k = 0; k < 3; ++k) op[k] = o[9 + k];
    for (int a = s_par[lane]; a >= 0; a = s_par[a]) {
      const double* wa = s_loc + 12 * a;
      double t9[9], t3[3];
      mm3(wa, oR, t9);
      mv3(wa, op, t3);
      for (int k = 0; k < 9; ++k) oR[k] = t9[k];
      for (int k = 0; k < 3; ++k) op[k] = wa[9 + k] + t3[k];
    }
    double* br = s_bod + BR * lane;
    for (int k = 0; k < 9; ++k) br[k] = oR[k];
    for (int k = 0; k < 3; ++k) br[9 + k] = op[k];
    // the axis J_c and J_c v_c (parked in the u slot)
    double J[6];
    world_axis(m, lane, oR, op, J);
    double* cr = s_col + CR * lane;
    for (int k = 0; k < 6; ++k) { cr[k] = J[k]; cr[6 + k] = J[k] * s_v[lane]; }
  }
  __syncthreads();
  // body velocities: ov_b = sum over the path of J_c v_c
  if (lane < N) {
    double ov[6] = {0, 0, 0, 0, 0, 0};
    for (int a = lane; a >= 0; a = s_par[a])
      for (int k = 0; k < 6; ++k) ov[k] += s_col[CR * a + 6 + k];
    for (int k = 0; k < 6; ++k) s_bod[BR * lane + 12 + k] = ov[k];
    // the velocity-product term ov_c x J_c v_c (parked in the g slot)
    double* cr = s_col + CR * lane;
    crm(ov, cr + 6, cr + 12);
  }
  __syncthreads();
  // per body at qdd = 0: oa0 = a_grav + path sum of the velocity products; world inertia, bias matrix, force f0 = I oa0 + ov x* I ov
  if (lane < N) {
    double* br = s_bod + BR * lane;
    double oa[6] = {0, 0, 0, -m.gravity[0], -m.gravity[1], -m.gravity[2]};
    for (int a = lane; a >= 0; a = s_par[a])
      for (int k = 0; k < 6; ++k) oa[k] += s_col[CR * a + 12 + k];
    double I6[36], B[36], h[6], Ioa[6], vxh[6];
    world_inertia(m.I6[lane], br, br + 9, I6);
    m6v(I6, br + 12, h);
    m6v(I6, oa, Ioa);
    crf(br + 12, h, vxh);
    bias_matrix(I6, br + 12, h, B);
    for (int k = 0; k < 6; ++k) { br[18 + k] = oa[k]; br[96 + k] = Ioa[k] + vxh[k]; }
    for (int k = 0; k < 36; ++k) { br[24 + k] = I6[k]; br[60 + k] = B[k]; }
  }
  __syncthreads();
  // subtree sums leaves -> root (Ic | Bc | f0): a thread only ever touches its own entries, children precede parents
  for (int i = N - 1; i >= 1; --i) {
    const int par = s_par[i];
    if (par < 0) continue;
    for (int k = lane; k < 78; k += nth) s_bod[BR * par + 24 + k] += s_bod[BR * i + 24 + k];
  }
  __syncthreads();
  // y_c = Ic J_c; the bias torques J_c . f0c; M's lower triangle: M(c, i) = J_i . y_c for the joints i of c's path
  if (lane < N) {
    const double* br = s_bod + BR * lane;
    double* cr = s_col + CR * lane;
    double y[6], bias = 0.0;
    m6v(br + 24, cr, y);
    for (int k = 0; k < 6; ++k) { cr[24 + k] = y[k]; bias += cr[k] * br[96 + k]; }
    s_rhs[lane] = s_tau[lane] - bias;
    for (int i = lane; i >= 0; i = s_par[i]) {
      double s = 0.0;
      for (int k = 0; k < 6; ++k) s += s_col[CR * i + k] * y[k];
      s_M[lane + i * N] = s;
    }
    s_M[lane + lane * N] += m.armature[lane];   // M + diag(armature)
  }
  __syncthreads();
  // Cholesky M = L L^T in place (lower triangle): thread r owns row r
  for (int k = 0; k < N; ++k) {
    const double dk = sqrt(s_M[k + k * N]);
    __syncthreads();
    if (lane == k) s_M[k + k * N] = dk;
    if (lane > k && lane < N) s_M[lane + k * N] = s_M[lane + k * N] / dk;
    __syncthreads();
    if (lane > k && lane < N) {
      const double lrk = s_M[lane + k * N];
      for (int c = k + 1; c <= lane; ++c) s_M[lane + c * N] -= lrk * s_M[c + k * N];
    }
    __syncthreads();
  }
  // M^-1: thread c solves L L^T x = e_c into column c of X
  if (lane < N) {
    double* x = s_X + lane * N;
    for (int i = 0; i < N; ++i) {
      double s = i == lane ? 1.0 : 0.0;
      for (int l = 0; l < i; ++l) s -= s_M[i + l * N] * x[l];
      x[i] = s / s_M[i + i * N];
    }
    for (int i = N - 1; i >= 0; --i) {
      double s = x[i];
      for (int l = i + 1; l < N; ++l) s -= s_M[l + i * N] * x[l];
      x[i] = s / s_M[i + i * N];
    }
  }
  __syncthreads();
  if (lane < N) {
    double s = 0.0;
    for (int l = 0; l < N; ++l) s += s_X[lane + l * N] * s_rhs[l];
    s_qdd[lane] = s;
  }
  __syncthreads();
  // accelerations: oa = oa0 + alpha, alpha_b = path sum of J_c qdd_c; forces I_b alpha_b (over the spent placements) summed
  // leaves -> root and added to f0c: ofc
  if (lane < N) {
    double* br = s_bod + BR * lane;
    double al[6] = {0, 0, 0, 0, 0, 0};
    for (int a = lane; a >= 0; a = s_par[a])
      for (int k = 0; k < 6; ++k) al[k] += s_col[CR * a + k] * s_qdd[a];
    double I6[36], f[6];
    world_inertia(m.I6[lane], br, br + 9, I6);
    m6v(I6, al, f);
    for (int k = 0; k < 6; ++k) { br[18 + k] += al[k]; s_loc[12 * lane + k] = f[k]; }
  }
  __syncthreads();
  for (int i = N - 1; i >= 1; --i) {
    const int par = s_par[i];
    if (par < 0) continue;
    for (int k = lane; k < 6; k += nth) s_loc[12 * par + k] += s_loc[12 * i + k];
  }
  __syncthreads();
  for (int k = lane; k < 6 * N; k += nth) s_bod[BR * (k / 6) + 96 + k % 6] += s_loc[12 * (k / 6) + k % 6];
  __syncthreads();
  // column quantities u | g | w | z | Fq | Fv
  if (lane < N) {
    const double* br = s_bod + BR * lane;
    double* cr = s_col + CR * lane;
    const double* J = cr;
    const double* ov = br + 12;
    double u[6], g[6], w[6], t1[6], t2[6], t3[6];
    m6tv(br + 60, J, cr + 30);                            // z
    crm(J, ov, u);
    crm(u, ov, t1);
    crm(J, br + 18, t2);
    for (int k = 0; k < 6; ++k) { g[k] = t1[k] - t2[k]; w[k] = 2.0 * u[k]; }
    for (int k = 0; k < 6; ++k) { cr[6 + k] = u[k]; cr[12 + k] = g[k]; cr[18 + k] = w[k]; }
    crf(J, br + 96, t1);
    m6v(br + 60, u, t2);
    m6v(br + 24, g, t3);
    for (int k = 0; k < 6; ++k) cr[36 + k] = t1[k] - t2[k] + t3[k];
    m6v(br + 60, J, t1);
    m6v(br + 24, w, t2);
    for (int k = 0; k < 6; ++k) cr[42 + k] = t1[k] - t2[k];
  }
  __syncthreads();
  double* s_T = lds + L::T;
  for (int k = lane; k < N * W2; k += nth) s_T[k] = 0.0;
  __syncthreads();
  // T: thread c walks its path; it writes row c (columns i of the path) and column c of the rows of its proper ancestors -- no
  // entry has two writers
  if (lane < N) {
    const int c = lane;
    const double* cc = s_col + CR * c;
    double sq = 0, sv = 0;
    for (int k = 0; k < 6; ++k) { sq += cc[k] * cc[36 + k]; sv += cc[k] * cc[42 + k]; }
    s_T[c * W2 + c] = sq;
    s_T[c * W2 + N + c] = sv;
    for (int i = s_par[c]; i >= 0; i = s_par[i]) {
      const double* ci = s_col + CR * i;
      double aq = 0, av = 0, dq = 0, dv = 0;
      for (int k = 0; k < 6; ++k) {
        aq += ci[k] * cc[36 + k];                          // d tau_i / d(q, v)_c: i a proper ancestor
        av += ci[k] * cc[42 + k];
        dq += -cc[30 + k] * ci[6 + k] + cc[24 + k] * ci[12 + k];   // d tau_c / d(q, v)_i
        dv += cc[30 + k] * ci[k] - cc[24 + k] * ci[18 + k];
      }
      s_T[i * W2 + c] = aq;
      s_T[i * W2 + N + c] = av;
      s_T[c * W2 + i] = dq;
      s_T[c * W2 + N + i] = dv;
    }
  }
  __syncthreads();
}

// qdd of the trajectory point (after ff_derivatives_wave / tree_derivatives_wave): nv doubles
template <int NJ>
__device__ __forceinline__ const double* wave_qdd(const double* lds) { return lds + FfLds<NJ>::VEC + 4 * NJ + 1; }

// row r of -M^-1 T, column j (after ff_derivatives_wave)
template <int NJ>
__device__ __forceinline__ double ff_minv_T(const double* lds, int N, int r, int j) {
  const double* s_X = lds + FfLds<NJ>::X;
  const double* s_T = lds + FfLds<NJ>::T;
  double s = 0.0;
  for (int l = 0; l < N; ++l) s += s_X[r + l * N] * s_T[l * 2 * N + j];
  return -s;
}

}  // namespace rbdd
