// frame_walk.h -- the kinematics the add-on cost terms share (frame_cost.h, com_cost.h, frame_vel_cost.h, obstacle_cost.h): the
// walk from a joint to the root and its joint step, the per-joint record a wave stages in LDS for the derivative kernels, the
// compaction of a path's tangent columns and the true point-jacobian column formed from the record.  Each exists here once.
#pragma once
#include "internal.h"
#include "lie.h"
#include "rbd.h"

namespace rbd {

// a term of weight 0 is left out, and with all three of a frame the walk itself
__device__ __forceinline__ bool frame_weights_any(const double* w) { return w[0] != 0.0 || w[1] != 0.0 || w[2] != 0.0; }
// ... and with all n of a block the block's work
__device__ __forceinline__ bool weights_any(const double* w, int n) {
  bool any = false;
  for (int k = 0; k < n; ++k) any |= w[k] != 0.0;
  return any;
}

// The joint step, in pieces.  v <- R_axis(angle) v, by the sine and 1 - cosine of the angle (Rodrigues)
__device__ __forceinline__ void axis_rotate(const double* a, double s, double omc, double* v) {
  double av[3], aav[3];
  cross3(a, v, av);
  cross3(a, av, aav);
  v[0] += s * av[0] + omc * aav[0]; v[1] += s * av[1] + omc * aav[1]; v[2] += s * av[2] + omc * aav[2];
}
// a direction of joint j's axes in its parent's: d <- Rp d
template <class M>
__device__ __forceinline__ void dir_to_parent(const M& m, int j, double* d) {
  double w[3];
  mv3(m.Rp[j], d, w);
  d[0] = w[0]; d[1] = w[1]; d[2] = w[2];
}
// ... and a point: p <- Rp p + pp
template <class M>
__device__ __forceinline__ void point_to_parent(const M& m, int j, double* p) {
  double w[3];
  mv3(m.Rp[j], p, w);
  p[0] = w[0] + m.pp[j][0]; p[1] = w[1] + m.pp[j][1]; p[2] = w[2] + m.pp[j][2];
}
// a free-flyer root (R its rotation, row-major): d <- R d, p <- R p + trans
__device__ __forceinline__ void dir_to_world(const double* R, double* d) {
  double w[3];
  mv3(R, d, w);
  d[0] = w[0]; d[1] = w[1]; d[2] = w[2];
}
__device__ __forceinline__ void point_to_world(const double* R, const double* trans, double* p) {
  double w[3];
  mv3(R, p, w);
  p[0] = w[0] + trans[0]; p[1] = w[1] + trans[1]; p[2] = w[2] + trans[2];
}

// The walk joint -> root with NP points and ND directions of joint `joint`'s axes alone (no placements are kept); they arrive
// in world axes.  Every joint j on the way: a revolute one turns them by R_axis(q_j), a prismatic one moves the points by
// q_j axis; then Rp . + pp for the points and Rp . for the directions.  A free-flyer root: R(quat) . + trans and R(quat) .
// own_axis: the direction that `joint`'s own rotation leaves alone (its axis), or -1.  Returns the path as a bit mask over
// joints.  M: DevModel or CoopModel (the tables in LDS)
template <int NP, int ND, class M>
__device__ __forceinline__ unsigned long long walk_to_root(const M& m, bool ff, int joint, const double* q, double (*pt)[3], double (*dir)[3],
                                                           int own_axis) {
  unsigned long long mask = 0;
  for (int j = joint; j >= 0; j = m.parent[j]) {
    double s, c;                       // (declared ahead of the root's branch: the kernels keep the registers they had)
    mask |= 1ull << j;
    if (j == 0 && ff) {
      double R[9];
      lie::quat_to_R(q + 3, R);
#pragma unroll
      for (int k = 0; k < NP; ++k) point_to_world(R, q, pt[k]);
#pragma unroll
      for (int k = 0; k < ND; ++k) dir_to_world(R, dir[k]);
      break;
    }
    const double* a = m.axis[j];
    const double qj = q[ff ? j + 6 : j];
    if (m.jtype[j] == DDP_HIP_JOINT_REVOLUTE) {
      sincos(qj, &s, &c);
      const double omc = 1.0 - c;
#pragma unroll
      for (int k = 0; k < NP; ++k) axis_rotate(a, s, omc, pt[k]);
#pragma unroll
      for (int k = 0; k < ND; ++k)
        if (k != own_axis || j != joint) axis_rotate(a, s, omc, dir[k]);
    } else {
#pragma unroll
      for (int k = 0; k < NP; ++k) { pt[k][0] += a[0] * qj; pt[k][1] += a[1] * qj; pt[k][2] += a[2] * qj; }
    }
#pragma unroll
    for (int k = 0; k < NP; ++k) point_to_parent(m, j, pt[k]);
#pragma unroll
    for (int k = 0; k < ND; ++k) dir_to_parent(m, j, dir[k]);
  }
  return mask;
}

// World position of the point `off` of joint `joint`
template <class M>
__device__ __forceinline__ void frame_point(const M& m, bool ff, int joint, const double* off, const double* q, double* p) {
  double v[1][3] = {{off[0], off[1], off[2]}};
  (void)walk_to_root<1, 0>(m, ff, joint, q, v, nullptr, -1);
  p[0] = v[0][0]; p[1] = v[0][1]; p[2] = v[0][2];
}

// World rotation R (row-major, world = R body) of joint `joint`'s frame: the walk with the three columns R e_a
template <class M>
__device__ __forceinline__ void frame_rotation(const M& m, bool ff, int joint, const double* q, double* R) {
  double c[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  (void)walk_to_root<0, 3>(m, ff, joint, q, nullptr, c, -1);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) R[3 * r + k] = c[k][r];
}

// What the lanes of one wave leave each other of the joints at one configuration: lane j's joint in slot j
struct JointWorldLds {
  double a[DDP_MAXJ][3], o[DDP_MAXJ][3];   // world axis a_j (0 on a free-flyer root), world origin o_j of joint j's frame
  unsigned long long mask[DDP_MAXJ];       // bit i: joint i is on the path root .. j (j itself included)
  double R0[9];                            // a free-flyer root's rotation (row-major)
};

// Lane j < nj walks its joint's path once and leaves a_j, o_j and the path in S; lane 0 of a free-flyer model leaves the root's
// rotation.  extra: NX further directions of joint j's axes that ride along and come back in world axes.  (A workgroup
// barrier follows.)
template <int NX>
__device__ __forceinline__ void stage_joint_lane(const DevModel& m, const double* q, int j, JointWorldLds& S, double (*extra)[3]) {
  const bool ff = m.ff != 0, root = j == 0 && ff;
  double o[1][3] = {{0.0, 0.0, 0.0}}, d[1 + NX][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) d[0][k] = root ? 0.0 : m.axis[j][k];
#pragma unroll
  for (int x = 0; x < NX; ++x) { d[1 + x][0] = extra[x][0]; d[1 + x][1] = extra[x][1]; d[1 + x][2] = extra[x][2]; }
  S.mask[j] = walk_to_root<1, 1 + NX>(m, ff, j, q, o, d, 0);
#pragma unroll
  for (int k = 0; k < 3; ++k) { S.a[j][k] = d[0][k]; S.o[j][k] = o[0][k]; }
#pragma unroll
  for (int x = 0; x < NX; ++x) { extra[x][0] = d[1 + x][0]; extra[x][1] = d[1 + x][1]; extra[x][2] = d[1 + x][2]; }
  if (root) lie::quat_to_R(q + 3, S.R0);
}

// a path as a mask over tangent columns: joint j is column j, behind a free-flyer root column j + 5 and the root columns 0 .. 5
__device__ __forceinline__ unsigned long long tangent_mask(bool ff, unsigned long long joints) {
  return ff ? (((joints >> 1) << 6) | 63ull) : joints;
}

// the tangent columns of U (the same in every lane), ascending, into idx by lane `tid`.  (A workgroup barrier follows.)
__device__ __forceinline__ void column_index_lane(unsigned long long U, int tid, int* idx) {
  if (tid < 64 && ((U >> tid) & 1)) idx[__builtin_popcountll(U & ((1ull << tid) - 1))] = tid;
}

// Column i (a tangent index on the point's path) of the true point jacobian P = dp / d(delta q) of the world point p, from the
// staged axes and origins, as frame_point_jacobian forms it: a_j x (p - o_j) for a revolute joint, a_j for a prismatic one; a
// free-flyer root (body twists, linear part first): R_0 e_c and (R_0 e_c) x (p - o_0)
__device__ __forceinline__ void point_column(const DevModel& m, bool ff, const JointWorldLds& S, int i, const double* p, double* col) {
  if (ff && i < 6) {
    const int c = i < 3 ? i : i - 3;
    const double e[3] = {S.R0[c], S.R0[3 + c], S.R0[6 + c]};
    if (i < 3) { col[0] = e[0]; col[1] = e[1]; col[2] = e[2]; return; }
    const double lever[3] = {p[0] - S.o[0][0], p[1] - S.o[0][1], p[2] - S.o[0][2]};
    cross3(e, lever, col);
    return;
  }
  const int j = ff ? i - 5 : i;
  if (m.jtype[j] == DDP_HIP_JOINT_REVOLUTE) {
    const double lever[3] = {p[0] - S.o[j][0], p[1] - S.o[j][1], p[2] - S.o[j][2]};
    cross3(S.a[j], lever, col);
  } else {
    col[0] = S.a[j][0]; col[1] = S.a[j][1]; col[2] = S.a[j][2];
  }
}

}  // namespace rbd
