// capsule_cost.h -- per-instance capsule collision costs (DDP_HIP_FLAG_CAPSULE_COST, ddp_hip.h): capsules on the robot against each
// other, against per-instance world capsules, against half-spaces, against the context's voxel grid and against oriented boxes, a one-sided
// penalty on their distance.  First the closest-point routines, which call no HIP function and compile for the host as well (in the manner of
// advance_plan.h: host/test_capsule_block.cpp, host/test_capsule_grid_block.cpp and host/test_capsule_box_block.cpp run them alone); then, for the device compiler,
// the kernel-side description and the device helpers.
// The terms themselves are formed by kernels of their own in fwd.hip (cost values: capsule_cost_kernel, summed by com_sum_kernel;
// clearances: capsule_clearance_kernel), lin.hip (derivatives: lin_capsule_cost_kernel) and model_api.hip (one pair:
// model_capsule_pair_kernel, model_capsule_box_kernel).
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/ddp_hip/ddp_hip.h"
#include "obstacle_grid.h"

#if defined(__HIPCC__)
#define CAP_HD __host__ __device__
#define CAP_UNROLL _Pragma("unroll")
#else
#define CAP_HD
#define CAP_UNROLL
#endif

CAP_HD static inline double capsule_clamp01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }

// The parameters s, t in [0, 1] of the closest points a0 + s (a1 - a0) and b0 + t (b1 - b0) of two segments, by the rule ddp_hip.h
// pins: the degenerate cases first (a segment of length 0 is a point), then the interior solution for s, the t that belongs to
// it, and where that t leaves [0, 1] the end of B and the s that belongs to the end.  Parallel segments (den <= 0) start from
// s = 0.  Every product is rounded on its own (no contraction), so that a restatement in another language takes the same branches
CAP_HD static inline void capsule_closest_params(const double* a0, const double* a1, const double* b0, const double* b1, double* s_out,
                                                 double* t_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d1[3] = {a1[0] - a0[0], a1[1] - a0[1], a1[2] - a0[2]};
  const double d2[3] = {b1[0] - b0[0], b1[1] - b0[1], b1[2] - b0[2]};
  const double r[3] = {a0[0] - b0[0], a0[1] - b0[1], a0[2] - b0[2]};
  const double A = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2];
  const double E = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
  const double F = d2[0] * r[0] + d2[1] * r[1] + d2[2] * r[2];
  const double C = d1[0] * r[0] + d1[1] * r[1] + d1[2] * r[2];
  if (A == 0.0 && E == 0.0) { *s_out = 0.0; *t_out = 0.0; return; }
  if (A == 0.0) { *s_out = 0.0; *t_out = capsule_clamp01(F / E); return; }
  if (E == 0.0) { *t_out = 0.0; *s_out = capsule_clamp01(-C / A); return; }
  const double Bv = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
  const double den = A * E - Bv * Bv;
  double s = den > 0.0 ? capsule_clamp01((Bv * F - C * E) / den) : 0.0;
  double t = (Bv * s + F) / E;
  if (t < 0.0) { t = 0.0; s = capsule_clamp01(-C / A); }
  else if (t > 1.0) { t = 1.0; s = capsule_clamp01((Bv - C) / A); }
  *s_out = s;
  *t_out = t;
}

// ... and the two points themselves; returns their distance D
CAP_HD static inline double capsule_closest_points(const double* a0, const double* a1, const double* b0, const double* b1, double* ca, double* cb) {
  double s, t;
  capsule_closest_params(a0, a1, b0, b1, &s, &t);
  for (int k = 0; k < 3; ++k) {
    ca[k] = a0[k] + s * (a1[k] - a0[k]);
    cb[k] = b0[k] + t * (b1[k] - b0[k]);
  }
  const double x = ca[0] - cb[0], y = ca[1] - cb[1], z = ca[2] - cb[2];
  return sqrt(x * x + y * y + z * z);
}

// A segment against the half-space n . p >= h: the end with the smaller n . p (end0 wins a tie) into ca; returns n . ca - h
CAP_HD static inline double capsule_halfspace_point(const double* a0, const double* a1, const double* n, double h, double* ca) {
  const double p0 = n[0] * a0[0] + n[1] * a0[1] + n[2] * a0[2], p1 = n[0] * a1[0] + n[1] * a1[1] + n[2] * a1[2];
  const bool second = p1 < p0;
  const double* e = second ? a1 : a0;
  ca[0] = e[0]; ca[1] = e[1]; ca[2] = e[2];
  return (second ? p1 : p0) - h;
}

// ---- a segment against the voxel grid (DDP_HIP_CAPSULE_VS_GRID, ddp_hip.h) --------------------------------------------------------
// The number of intervals N of a robot capsule with the ends end0, end1 (joint frame) on a grid of spacing cell: 0 for a sphere,
// else ceil(L / cell) kept within 1 .. DDP_HIP_CAPSULE_GRID_MAX_INTERVALS.  Host arithmetic in double, every product rounded on its
// own (capsule_cost_dev calls it whenever a description is built: the state never enters)
CAP_HD static inline int32_t capsule_grid_intervals(const double* end0, const double* end1, double cell) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double dx = end1[0] - end0[0], dy = end1[1] - end0[1], dz = end1[2] - end0[2];
  const double L = sqrt(dx * dx + dy * dy + dz * dz);
  if (L == 0.0) return 0;
  const double r = ceil(L / cell);
  if (!(r < (double)DDP_HIP_CAPSULE_GRID_MAX_INTERVALS)) return DDP_HIP_CAPSULE_GRID_MAX_INTERVALS;
  return r < 1.0 ? 1 : (int32_t)r;
}

// Sample j of N: the material point c_j = a0 + (j / N) (a1 - a0) and the field there, phi_j and g_j at c_j - shift
// (obstacle_grid_lookup as it is: +inf and a zero gradient outside, NaN for a NaN coordinate)
CAP_HD static inline void capsule_grid_sample(const ObstacleGridDev& G, const double* a0, const double* a1, const double* shift, int32_t N, int32_t j,
                                              double* c, double* phi, double* grad) {
  const double sigma = N > 0 ? (double)j / (double)N : 0.0;
  double x[3];
  for (int k = 0; k < 3; ++k) {
    c[k] = a0[k] + sigma * (a1[k] - a0[k]);
    x[k] = c[k] - shift[k];
  }
  (void)obstacle_grid_lookup(G, x, phi, grad);
}

// The selection, one step of a scan in ascending j: does sample `phi` replace the best so far?  (first: there is none yet.)  A NaN
// that has been taken stays, a NaN replaces everything else, otherwise the strictly smaller value: the smallest j wins a tie
CAP_HD static inline bool capsule_grid_better(double phi, double best, bool first) {
  if (first) return true;
  if (best != best) return false;
  return phi != phi || phi < best;
}

// The rule: over the samples j = 0 .. N the smallest j attaining min_j phi_j (the first NaN before everything).  *j = -1 and
// *phi = +inf where every sample lies outside the grid (then c = a0, grad = 0); else c = c_j*, grad = g_j*.  The one definition
// behind the value, clearance, derivative and query kernels: those that deal the samples over lanes use capsule_grid_sample and
// capsule_grid_better, scan in ascending j and form point and gradient by capsule_grid_sample at j* again
CAP_HD static inline void capsule_grid_closest(const ObstacleGridDev& G, const double* a0, const double* a1, const double* shift, int32_t N, double* phi,
                                               int32_t* j, double* c, double* grad) {
  double best = INFINITY;
  int32_t bj = 0;
  for (int32_t s = 0; s <= N; ++s) {
    double cs[3], ps, gs[3];
    capsule_grid_sample(G, a0, a1, shift, N, s, cs, &ps, gs);
    if (capsule_grid_better(ps, best, s == 0)) { best = ps; bj = s; }
  }
  capsule_grid_sample(G, a0, a1, shift, N, best == INFINITY ? 0 : bj, c, phi, grad);
  *j = best == INFINITY ? -1 : bj;
}

// d, c_a = c_b and u of a grid pair from the selected sample: false where the pair has no derivative (every sample outside:
// d = +inf; a gradient of exactly zero)
CAP_HD static inline bool capsule_grid_pair(double phi, const double* grad, double ra, double margin, double* d, double* u) {
  u[0] = grad[0]; u[1] = grad[1]; u[2] = grad[2];
  if (phi == INFINITY) { *d = INFINITY; return false; }
  *d = phi - ra - margin;
  return phi != phi || u[0] != 0.0 || u[1] != 0.0 || u[2] != 0.0;
}

// ---- a segment against an oriented box (DDP_HIP_CAPSULE_VS_BOX, ddp_hip.h) --------------------------------------------------------
// The box's signed distance at p (box axes, half extents h): the length of the part of |p| - h above 0 where that is > 0, else the
// largest of |p_k| - h_k (<= 0: on or inside); NaN where a coordinate is
CAP_HD static inline double capsule_box_phi(double p0, double p1, double p2, const double* h) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double q0 = fabs(p0) - h[0], q1 = fabs(p1) - h[1], q2 = fabs(p2) - h[2];
  if (q0 != q0 || q1 != q1 || q2 != q2) return NAN;
  const double e0 = q0 > 0.0 ? q0 : 0.0, e1 = q1 > 0.0 ? q1 : 0.0, e2 = q2 > 0.0 ? q2 : 0.0;
  const double o = sqrt(e0 * e0 + e1 * e1 + e2 * e2);
  if (o > 0.0) return o;
  double m = q0;
  if (q1 > m) m = q1;
  if (q2 > m) m = q2;
  return m;
}

// What a search over the candidates carries: segment and box in box axes, the best candidate so far and, where that is a crossing
// of two of the six face lines, which two (else -1)
struct CapsuleBoxSearch {
  double a[3], dl[3], h[3];
  double s, f;
  int32_t li, lj;
  bool first;
};
// One candidate, in the order met: replaces the best only if strictly smaller (capsule_grid_better: the first NaN before everything)
CAP_HD static inline void capsule_box_try(CapsuleBoxSearch& B, double s, int32_t li, int32_t lj) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double f = capsule_box_phi(B.a[0] + s * B.dl[0], B.a[1] + s * B.dl[1], B.a[2] + s * B.dl[2], B.h);
  if (capsule_grid_better(f, B.f, B.first)) { B.f = f; B.s = s; B.li = li; B.lj = lj; }
  B.first = false;
}

// The rule of ddp_hip.h: the least signed distance f* of the box (half extents h, pose = centre(3) | quaternion x y z w, world =
// R box) along the segment a0 .. a1, the smallest parameter s* attaining it among the candidates, the point c_a = a0 + s* (a1 - a0)
// and the direction u = df* / dc_a, all in the world.  phi is convex, so f(s) = phi(p(s)) is convex on [0, 1] and on each
// sub-interval between two breakpoints (where p crosses a face plane) it is one smooth piece: outside the box the distance to one
// face, edge or corner (stationary point of a quadratic), inside the largest of six lines (a minimum only where two cross).  The
// candidates therefore hold the exact minimum.  The sub-intervals are walked in ascending order by taking the least breakpoint above
// the last one: the same candidates in the same order as after a sort, but for equal breakpoints, whose empty intervals add none.
// No array is indexed by a run-time value (on the device: registers only).  A quaternion of all zeros (fresh geometry, which no
// upload accepts) gives R = identity by the formula: the box is evaluated with its axes along the world's.
CAP_HD static inline double capsule_box_closest(const double* a0, const double* a1, const double* half, const double* pose, double* s_out, double* ca,
                                                double* u) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double x = pose[3], y = pose[4], z = pose[5], w = pose[6];
  const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)},
                          {2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)},
                          {2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)}};
  const double ra[3] = {a0[0] - pose[0], a0[1] - pose[1], a0[2] - pose[2]}, rb[3] = {a1[0] - pose[0], a1[1] - pose[1], a1[2] - pose[2]};
  CapsuleBoxSearch B;
  double bp[3][2];                                                   // the breakpoints of axis k at +h_k and -h_k (2: none)
CAP_UNROLL
  for (int k = 0; k < 3; ++k) {
    B.a[k] = R[0][k] * ra[0] + R[1][k] * ra[1] + R[2][k] * ra[2];
    const double bk = R[0][k] * rb[0] + R[1][k] * rb[1] + R[2][k] * rb[2];
    B.dl[k] = bk - B.a[k];
    B.h[k] = half[k];
    const double sp = (B.h[k] - B.a[k]) / B.dl[k], sm = (-B.h[k] - B.a[k]) / B.dl[k];
    bp[k][0] = B.dl[k] != 0.0 && sp > 0.0 && sp < 1.0 ? sp : 2.0;
    bp[k][1] = B.dl[k] != 0.0 && sm > 0.0 && sm < 1.0 ? sm : 2.0;
  }
  B.s = 0.0; B.f = 0.0; B.li = -1; B.lj = -1; B.first = true;
  // the six lines l_i(s) = +-p_k(s) - h_k, i = 2 k + (0: +, 1: -): value at 0 and slope
  const double c0[6] = {B.a[0] - B.h[0], -B.a[0] - B.h[0], B.a[1] - B.h[1], -B.a[1] - B.h[1], B.a[2] - B.h[2], -B.a[2] - B.h[2]};
  const double m0[6] = {B.dl[0], -B.dl[0], B.dl[1], -B.dl[1], B.dl[2], -B.dl[2]};
  double lo = 0.0;
  for (int it = 0; it < 7 && lo < 1.0; ++it) {
    double hi = 1.0;
CAP_UNROLL
    for (int k = 0; k < 3; ++k) {
      if (bp[k][0] > lo && bp[k][0] < hi) hi = bp[k][0];
      if (bp[k][1] > lo && bp[k][1] < hi) hi = bp[k][1];
    }
    const double mid = 0.5 * (lo + hi);
    capsule_box_try(B, lo, -1, -1);
    double A = 0.0, C = 0.0;
    bool outside = false;
CAP_UNROLL
    for (int k = 0; k < 3; ++k) {
      const double pm = B.a[k] + mid * B.dl[k];
      const double sg = pm > B.h[k] ? 1.0 : (pm < -B.h[k] ? -1.0 : 0.0);
      if (sg != 0.0) {
        outside = true;
        A = A + B.dl[k] * B.dl[k];
        C = C + B.dl[k] * (B.a[k] - sg * B.h[k]);
      }
    }
    if (outside) {
      const double s = -C / A;
      if (A > 0.0 && s > lo && s < hi) capsule_box_try(B, s, -1, -1);
    } else {
CAP_UNROLL
      for (int i = 0; i < 5; ++i)
CAP_UNROLL
        for (int j = i + 1; j < 6; ++j) {
          if (m0[i] == m0[j]) continue;
          const double s = (c0[j] - c0[i]) / (m0[i] - m0[j]);
          if (s > lo && s < hi) capsule_box_try(B, s, i, j);
        }
    }
    capsule_box_try(B, hi, -1, -1);
    lo = hi;
  }
  // the direction in box axes
  const double sb = B.s, fb = B.f;
  double p[3], n[3] = {0.0, 0.0, 0.0};
CAP_UNROLL
  for (int k = 0; k < 3; ++k) p[k] = B.a[k] + sb * B.dl[k];
  bool kink = false;
  if (!(fb > 0.0) && B.li >= 0) {
    double mi = 0.0, mj = 0.0;
CAP_UNROLL
    for (int i = 0; i < 6; ++i) {
      if (i == B.li) mi = m0[i];
      if (i == B.lj) mj = m0[i];
    }
    if ((mi > 0.0 && mj < 0.0) || (mi < 0.0 && mj > 0.0)) {
      kink = true;
      const double ai = fabs(mi), aj = fabs(mj), den = ai + aj;
CAP_UNROLL
      for (int i = 0; i < 6; ++i) {
        const double sgn = (i & 1) ? -1.0 : 1.0;
        if (i == B.li) n[i >> 1] = n[i >> 1] + sgn * aj;
        if (i == B.lj) n[i >> 1] = n[i >> 1] + sgn * ai;
      }
      n[0] = n[0] / den; n[1] = n[1] / den; n[2] = n[2] / den;
    }
  }
  if (fb > 0.0) {
CAP_UNROLL
    for (int k = 0; k < 3; ++k) {
      const double cl = p[k] < -B.h[k] ? -B.h[k] : (p[k] > B.h[k] ? B.h[k] : p[k]);
      n[k] = (p[k] - cl) / fb;
    }
  } else if (!kink) {
    // the first of the six lines that attains the largest value at s* (a NaN coordinate: line 0, and d is NaN)
    const double l[6] = {p[0] - B.h[0], -p[0] - B.h[0], p[1] - B.h[1], -p[1] - B.h[1], p[2] - B.h[2], -p[2] - B.h[2]};
    double best = l[0];
    int32_t bi = 0;
CAP_UNROLL
    for (int i = 1; i < 6; ++i)
      if (l[i] > best) { best = l[i]; bi = i; }
CAP_UNROLL
    for (int i = 0; i < 6; ++i)
      if (i == bi) n[i >> 1] = (i & 1) ? -1.0 : 1.0;
  }
CAP_UNROLL
  for (int k = 0; k < 3; ++k) {
    ca[k] = a0[k] + sb * (a1[k] - a0[k]);
    u[k] = R[k][0] * n[0] + R[k][1] * n[1] + R[k][2] * n[2];
  }
  *s_out = sb;
  return fb;
}

// d and whether the pair has a derivative (f* == 0 exactly: value only, the D == 0 rule of the segment kinds; a NaN is active)
CAP_HD static inline bool capsule_box_pair(double f, double ra, double margin, double* d) {
  *d = f - ra - margin;
  return f != 0.0;
}

#if defined(__HIPCC__)
#include "frame_walk.h"
#include "internal.h"
#include "lie.h"
#include "obstacle_cost.h"
#include "rbd.h"

// What a kernel reads of the context's capsule cost.  geom == nullptr: no terms (the flag is off, no pairs are set, or no
// non-zero weight has been uploaded: the block's CostBlock::live)
struct CapsuleCostDev {
  const double *geom, *weight;     // [batch][T+1][npair][8], [batch][T+1][npair]
  int32_t nc, npair;               // robot capsules, pairs
  int32_t joint[DDP_HIP_MAX_CAPSULES];
  uint8_t pa[DDP_HIP_MAX_CAPSULE_PAIRS], kind[DDP_HIP_MAX_CAPSULE_PAIRS], pb[DDP_HIP_MAX_CAPSULE_PAIRS];   // pair i: capsule pa[i] against kind[i] (pb[i]: a robot pair's)
  double end[DDP_HIP_MAX_CAPSULES][2][3];
  double radius[DDP_HIP_MAX_CAPSULES];
  // the pairs of kind DDP_HIP_CAPSULE_VS_GRID (behind everything else: a context without one reads what it read before the kind)
  int32_t grid_pairs;                             // how many: != 0 runs the kernels' GRID instantiation
  int32_t grid_items;                             // their samples in all: sum over them of nseg[pa] + 1
  int32_t nseg[DDP_HIP_MAX_CAPSULES];             // N_k of capsule k on the resident grid (capsule_grid_intervals)
  uint16_t gbase[DDP_HIP_MAX_CAPSULE_PAIRS];      // pair i of the kind: its first item (the others: not read)
  ObstacleGridDev grid;                           // the resident field (phi == nullptr: none)
  // the pairs of kind DDP_HIP_CAPSULE_VS_BOX (behind everything else again); pb[i] of such a pair is its shape
  int32_t box_pairs;                              // how many: != 0 runs the kernels' BOX instantiation
  double half[DDP_HIP_MAX_CAPSULE_BOXES][3];      // the half extents of the box shapes (ddp_hip_capsule_set_boxes)
};

// always: the description whether or not a weight is live (ddp_hip_capsule_clearance works from the first set_pairs on)
inline CapsuleCostDev capsule_cost_dev(const ddp_hip_ctx* ctx, bool always = false) {
  CapsuleCostDev c{};
  const CostBlock& k = ctx->cost[COST_CAPSULE];
  if (!(always ? ctx->cp_npair > 0 : k.live)) return c;
  c.geom = k.side[0];
  c.weight = k.side[1];
  c.nc = ctx->cp_nc;
  c.npair = ctx->cp_npair;
  for (int s = 0; s < ctx->cp_nc; ++s) {
    c.joint[s] = ctx->cp_joint[s];
    c.radius[s] = ctx->cp_radius[s];
    for (int e = 0; e < 2; ++e)
      for (int a = 0; a < 3; ++a) c.end[s][e][a] = ctx->cp_end[s][e][a];
  }
  for (int i = 0; i < ctx->cp_npair; ++i) {
    c.pa[i] = (uint8_t)ctx->cp_pa[i];
    c.kind[i] = (uint8_t)ctx->cp_kind[i];
    c.pb[i] = (uint8_t)ctx->cp_pb[i];
  }
  c.grid = obstacle_grid_dev(ctx);
  if (c.grid.phi) {
    for (int s = 0; s < ctx->cp_nc; ++s) c.nseg[s] = capsule_grid_intervals(ctx->cp_end[s][0], ctx->cp_end[s][1], c.grid.cell);
    for (int i = 0; i < ctx->cp_npair; ++i) {
      if (ctx->cp_kind[i] != DDP_HIP_CAPSULE_VS_GRID) continue;
      c.gbase[i] = (uint16_t)c.grid_items;
      c.grid_items += c.nseg[ctx->cp_pa[i]] + 1;
      ++c.grid_pairs;
    }
  }
  for (int i = 0; i < ctx->cp_npair; ++i) c.box_pairs += ctx->cp_kind[i] == DDP_HIP_CAPSULE_VS_BOX;
  for (int s = 0; s < ctx->cp_nbox; ++s)
    for (int a = 0; a < 3; ++a) c.half[s][a] = ctx->cp_half[s][a];
  return c;
}

namespace rbd {

// Both ends of robot capsule k in the world: one walk joint -> root with the two points (no jacobian, no per-joint arrays)
template <class M>
__device__ __forceinline__ void capsule_ends(const M& m, bool ff, const CapsuleCostDev& cp, int k, const double* q, double (*e)[3]) {
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int a = 0; a < 3; ++a) e[s][a] = cp.end[k][s][a];
  (void)walk_to_root<2, 0>(m, ff, cp.joint[k], q, e, nullptr, -1);
}

// The signed distance d_i of pair i, its closest points c_a, c_b and the direction u_i = dd / dc_a = -dd / dc_b.  a0, a1: the
// world ends of body A; b0, b1: those of body B where it is a robot capsule (else not read); g: the pair's eight doubles.
// Returns false where u does not exist (the closest points coincide: the pair has its value and no derivative).  GRID: some pair
// may be a grid's (the whole scan on this lane: the kernels that deal the samples over lanes do not come here for such a pair).  The
// kernels are instantiated both ways and a context without a grid pair runs the instruction stream it ran before the kind existed.
// BOX: some pair may be a box's, likewise (one evaluation of capsule_box_closest on the pair's own lane: g = centre, quaternion, m)
template <bool GRID, bool BOX>
__device__ __forceinline__ bool capsule_distance(const CapsuleCostDev& cp, int i, const double* a0, const double* a1, const double* b0,
                                                 const double* b1, const double* g, double* d, double* ca, double* cb, double* u) {
  const double ra = cp.radius[cp.pa[i]], margin = g[7];
  if (GRID && cp.kind[i] == DDP_HIP_CAPSULE_VS_GRID) {
    double phi, grad[3];
    int32_t j;
    capsule_grid_closest(cp.grid, a0, a1, g, cp.nseg[cp.pa[i]], &phi, &j, ca, grad);
    cb[0] = ca[0]; cb[1] = ca[1]; cb[2] = ca[2];
    return capsule_grid_pair(phi, grad, ra, margin, d, u);
  }
  if (BOX && cp.kind[i] == DDP_HIP_CAPSULE_VS_BOX) {
    double s;
    const double f = capsule_box_closest(a0, a1, cp.half[cp.pb[i]], g, &s, ca, u);
    cb[0] = ca[0]; cb[1] = ca[1]; cb[2] = ca[2];
    return capsule_box_pair(f, ra, margin, d);
  }
  if (cp.kind[i] == DDP_HIP_CAPSULE_VS_HALFSPACE) {
    *d = capsule_halfspace_point(a0, a1, g, g[3], ca) - ra - margin;
    cb[0] = ca[0]; cb[1] = ca[1]; cb[2] = ca[2];
    u[0] = g[0]; u[1] = g[1]; u[2] = g[2];
    return true;
  }
  const bool robot = cp.kind[i] == DDP_HIP_CAPSULE_VS_ROBOT;
  const double dist = capsule_closest_points(a0, a1, robot ? b0 : g, robot ? b1 : g + 3, ca, cb);
  *d = dist - (ra + (robot ? cp.radius[cp.pb[i]] : g[6]) + margin);
  if (dist == 0.0) { u[0] = u[1] = u[2] = 0.0; return false; }
  u[0] = (ca[0] - cb[0]) / dist; u[1] = (ca[1] - cb[1]) / dist; u[2] = (ca[2] - cb[2]) / dist;
  return true;
}

// What the lanes of one wave leave each other for the derivatives at one configuration (lin_capsule_cost_kernel, phase 2): lanes
// j < nj their joint (rbd::stage_joint_lane), the active pairs' lanes their pair
struct CapsuleWaveLds {
  JointWorldLds jw;                                      // a_j, o_j, the paths, R_0
  double ca[DDP_HIP_MAX_CAPSULE_PAIRS][3];               // of the active pairs: the closest point on A,
  double cb[DDP_HIP_MAX_CAPSULE_PAIRS][3];               // ... on B,
  double u[DDP_HIP_MAX_CAPSULE_PAIRS][3];                // u_i,
  double w[DDP_HIP_MAX_CAPSULE_PAIRS];                   // w_i,
  double we[DDP_HIP_MAX_CAPSULE_PAIRS];                  // w_i e_i,
  unsigned long long ma[DDP_HIP_MAX_CAPSULE_PAIRS];      // the tangent columns on path(A) alone (a world pair: all of path(A))
  unsigned long long mb[DDP_HIP_MAX_CAPSULE_PAIRS];      // ... and on path(B) alone (a world pair: none)
  int idx[DDP_MAXJ];                                     // the union of them all, ascending
};

// The two column masks of pair i from the staged paths, by its own lane.  (A workgroup barrier follows.)
__device__ __forceinline__ unsigned long long capsule_masks_lane(const CapsuleCostDev& cp, bool ff, int i, CapsuleWaveLds& S, bool mine) {
  const unsigned long long pa = tangent_mask(ff, S.jw.mask[cp.joint[cp.pa[i]]]);
  const unsigned long long pb = cp.kind[i] == DDP_HIP_CAPSULE_VS_ROBOT ? tangent_mask(ff, S.jw.mask[cp.joint[cp.pb[i]]]) : 0ull;
  if (mine) { S.ma[i] = pa & ~pb; S.mb[i] = pb & ~pa; }
  return pa ^ pb;
}

// z_i[c] of an active pair at a column c of its column set: + P_ca[:, c] . u_i on A's side, - P_cb[:, c] . u_i on B's.  The
// closest point is frozen in its joint: the column of P is that of a fixed point there, formed on the fly (rbd::point_column)
__device__ __forceinline__ double capsule_z(const DevModel& m, bool ff, const CapsuleWaveLds& S, int i, int c) {
  const bool on_a = (S.ma[i] >> c) & 1;
  double col[3];
  point_column(m, ff, S.jw, c, on_a ? S.ca[i] : S.cb[i], col);
  const double z = col[0] * S.u[i][0] + col[1] * S.u[i][1] + col[2] * S.u[i][2];
  return on_a ? z : -z;
}

// Phase 2, last step: the wave (lane tid of nt) adds, over the nu tangent columns of S.idx (the union of the active pairs' column
// sets) alone,
//   gx[c] += sum_i (w e)_i z_i[c],      gxx[r][c] += sum_i w_i z_i[min] z_i[max]      (Gauss-Newton)
// the active pairs (bit i of `active`) in ascending order, a pair outside whose column set r or c lies left out, entry (r, c) in
// (min, max) order: the block stays symmetric bit for bit.  A column on both paths of a robot pair is in neither mask
__device__ __forceinline__ void capsule_add_wave(const DevModel& m, const CapsuleWaveLds& S, int npair, unsigned active, int nu, int tid, int nt,
                                                 int n, double* gx, double* gxx) {
  const bool ff = m.ff != 0;
  for (int r = tid; r < nu; r += nt) {
    const int c = S.idx[r];
    double s = 0.0;
    for (int i = 0; i < npair; ++i) {
      if (!((active >> i) & 1) || !(((S.ma[i] | S.mb[i]) >> c) & 1)) continue;
      s += S.we[i] * capsule_z(m, ff, S, i, c);
    }
    gx[c] += s;
  }
  for (int e = tid; e < nu * nu; e += nt) {
    const int r = S.idx[e % nu], c = S.idx[e / nu];
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    double h = 0.0;
    bool hit = false;
    for (int i = 0; i < npair; ++i) {
      if (!((active >> i) & 1)) continue;
      const unsigned long long cs = S.ma[i] | S.mb[i];
      if (!((cs >> r) & 1) || !((cs >> c) & 1)) continue;
      h += S.w[i] * capsule_z(m, ff, S, i, lo) * capsule_z(m, ff, S, i, hi);
      hit = true;
    }
    if (hit) gxx[r + (int64_t)c * n] += h;
  }
}

}  // namespace rbd
#endif  // __HIPCC__
