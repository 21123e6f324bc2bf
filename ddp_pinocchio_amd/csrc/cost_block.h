// cost_block.h -- the per-instance add-on cost terms as records: what a term's arrays look like, and the
// parts of its upload that call no HIP function -- flag and range checks, the per-side validators, the non-zero scan, the live
// rule.  Host code without a device dependency: ctx.hip builds the upload path on it, host/test_cost_block.cpp runs it alone.
#pragma once

#include <math.h>
#include <stdint.h>

#include "ddp_hip/ddp_hip.h"

// The terms.  The order in which the kernels add them (after the stage cost and the tracking cost) is stated where they are launched:
// lin.hip launches one kernel per live term, fwd.hip forms the first three inline and walks kAddOn for the others, both in the order
// frame positions, frame orientations, limits, CoM, frame velocities, momentum, balance regions, relative frames, control-gravity,
// frame aiming, joint accelerations, obstacles, self-collision, capsules.  The enumerators are indices of ctx->cost[] and kCostDesc[] and follow that order but for
// COST_CONTROL_GRAV, COST_FRAME_AIM, COST_BALANCE_REGION, COST_JOINT_ACCEL and COST_CAPSULE: the host programs hold momentum, relative frames, obstacles and self-collision as neighbours
// and self-collision as the last (host/test_relative_frame_block.cpp, host/test_self_collision_block.cpp), so the term whose
// additions come between the relative frames' and the obstacles' has its index in front of that run; they hold frame velocities and
// control-gravity as neighbours too (host/test_control_grav_block.cpp), so the term whose additions come after control-gravity's
// has its index in front of the frame velocities'; and they hold the CoM, frame aiming and the frame velocities as neighbours
// (host/test_frame_aim_block.cpp), and momentum and the relative frames, so the term whose additions come between the momentum's and
// the relative frames' has its index in front of the CoM's.  With that every adjacency from the limits to self-collision is held by
// some host program (host/test_balance_region_block.cpp holds the limits and the balance regions), so the term whose additions come
// between frame aiming's and the obstacles', the joint accelerations, has its index in front of the limits'.  The capsules' additions come last of all, but
// self-collision is held as the last index and every adjacency from the frame orientations on is held, so their index stands between
// the frame positions' and the frame orientations' (host/test_capsule_block.cpp).  No order is read off the enumerators: the kernels' order is the
// order of the launches in lin.hip and of kAddOn in fwd.hip, nothing else
enum CostTerm : int32_t { COST_FRAME, COST_CAPSULE, COST_ORIENT, COST_JOINT_ACCEL, COST_LIMITS, COST_BALANCE_REGION, COST_COM, COST_FRAME_AIM, COST_FRAME_VEL, COST_CONTROL_GRAV, COST_MOMENTUM,
                          COST_RELATIVE_FRAME, COST_OBSTACLE, COST_SELF_COLLISION, COST_COUNT };

enum CostFill : int32_t { FILL_ZERO, FILL_NEG_INF, FILL_POS_INF, FILL_QUAT };   // FILL_QUAT: identity quaternions (0, 0, 0, 1)

#define COST_MAX_SIDES 3
#define COST_ITEMS_STATE 0          // CostDesc::max_items: one item per tangent row of the state, n
#define COST_ITEMS_CONTROL (-1)     // ... one item per control row, m
#define COST_ITEMS_VELOCITY (-2)    // ... one item per tangent row of v, nv

// What a term is made of.  A side is one array [batch][rows][items][unit], rows = T+1 (t = 0 .. T), or T for a term of the
// stages alone (stage_only: t = 0 .. T-1, no terminal row); the last side is the weights
struct CostDesc {
  uint32_t flag;                    // the creation flag that enables the term
  int32_t nside;
  int32_t unit[COST_MAX_SIDES];     // doubles per item
  int32_t fill[COST_MAX_SIDES];     // CostFill: what a side holds at create and after a change of layout
  int32_t max_items;                // items the arrays have room for; COST_ITEMS_STATE / _CONTROL / _VELOCITY: n / m / nv (CostBlock::max_items, set at create)
  bool fixed;                       // laid out at create for max_items; else by the frames / slots set, up to max_items
  bool cand;                        // the term has a candidates' array for the line search
  bool stage_only;                  // a term of l(t, x, u), t < T, alone: T rows per instance, not T+1 (a term that reads u has no row at T)
};

static const CostDesc kCostDesc[COST_COUNT] = {
    // flag, sides, doubles per item, fill, room, fixed, cand, stage_only
    {DDP_HIP_FLAG_FRAME_COST, 2, {3, 3, 0}, {FILL_ZERO, FILL_ZERO, 0}, DDP_HIP_MAX_COST_FRAMES, false, false, false},          // target | weight, per frame
    {DDP_HIP_FLAG_CAPSULE_COST, 2, {8, 1, 0}, {FILL_ZERO, FILL_ZERO, 0}, DDP_HIP_MAX_CAPSULE_PAIRS, false, true, false},      // geom | weight, per pair
    {DDP_HIP_FLAG_FRAME_ORIENT_COST, 2, {4, 3, 0}, {FILL_QUAT, FILL_ZERO, 0}, DDP_HIP_MAX_COST_FRAMES, false, false, false},   // quat | weight, per frame
    {DDP_HIP_FLAG_JOINT_ACCEL_COST, 2, {1, 1, 0}, {FILL_ZERO, FILL_ZERO, 0}, COST_ITEMS_VELOCITY, true, true, false},           // target | weight, per tangent row of v; row T carries no term
    {DDP_HIP_FLAG_STATE_LIMITS, 3, {1, 1, 1}, {FILL_NEG_INF, FILL_POS_INF, FILL_ZERO}, 0, true, false, false},                 // lo | hi | weight, per tangent row
    {DDP_HIP_FLAG_BALANCE_REGION_COST, 2, {5, 1, 0}, {FILL_ZERO, FILL_ZERO, 0}, DDP_HIP_MAX_REGION_PLANES, false, true, false},   // (n, h, tau) | weight, per plane slot
    {DDP_HIP_FLAG_COM_COST, 2, {3, 3, 0}, {FILL_ZERO, FILL_ZERO, 0}, 1, true, true, false},                                    // target | weight
    {DDP_HIP_FLAG_FRAME_AIM_COST, 2, {4, 2, 0}, {FILL_ZERO, FILL_ZERO, 0}, DDP_HIP_MAX_AIM_FRAMES, false, true, false},        // (target, stand-off) | (w_aim, w_range), per aim frame
    {DDP_HIP_FLAG_FRAME_VEL_COST, 2, {6, 6, 0}, {FILL_ZERO, FILL_ZERO, 0}, DDP_HIP_MAX_COST_FRAMES, false, true, false},       // target | weight, per frame
    {DDP_HIP_FLAG_CONTROL_GRAV_COST, 2, {1, 1, 0}, {FILL_ZERO, FILL_ZERO, 0}, COST_ITEMS_CONTROL, true, true, true},              // offset | weight, per control row, t < T
    {DDP_HIP_FLAG_MOMENTUM_COST, 2, {6, 6, 0}, {FILL_ZERO, FILL_ZERO, 0}, 1, true, true, false},                               // target | weight
    {DDP_HIP_FLAG_RELATIVE_FRAME_COST, 3, {3, 4, 6}, {FILL_ZERO, FILL_QUAT, FILL_ZERO}, DDP_HIP_MAX_FRAME_PAIRS, false, true, false},   // target | quat | weight, per pair
    {DDP_HIP_FLAG_OBSTACLE_COST, 2, {4, 1, 0}, {FILL_ZERO, FILL_ZERO, 0}, DDP_HIP_MAX_OBSTACLES, false, true, false},          // geom | weight, per slot
    {DDP_HIP_FLAG_SELF_COLLISION_COST, 2, {1, 1, 0}, {FILL_ZERO, FILL_ZERO, 0}, DDP_HIP_MAX_COLLISION_PAIRS, false, true, false},   // margin | weight, per pair
};

// One term of one context
struct CostBlock {
  const CostDesc* desc = nullptr;
  int32_t max_items = 0;            // the arrays are allocated for this many items per (instance, t) ...
  int32_t items = 0;                // ... and laid out by this many (frames / slots set); 0: no layout yet
  double* side[COST_MAX_SIDES] = {nullptr, nullptr, nullptr};   // device arrays (null: the flag is off)
  double* cand = nullptr;           // [batch][n_alpha_max][T+1] the candidates' terms of a line-search round, from the first non-zero weight on
  bool live = false;                // some non-zero weight is resident: the kernels form the term (cost_live_rule)
};

// rows of a side per instance, and doubles of side s per instance, as laid out now
static inline int64_t cost_rows(const CostBlock& k, int64_t T) { return k.desc->stage_only ? T : T + 1; }
static inline int64_t cost_side_words(const CostBlock& k, int s, int64_t T) { return cost_rows(k, T) * (int64_t)k.items * k.desc->unit[s]; }

// What the validators of one upload know beside the values
struct CostCheck {
  int64_t items = 0;                // per (instance, t)
  bool ff = false;                  // free-flyer root: the first six tangent rows carry no limit
  const int32_t* kind = nullptr;    // [items] obstacle slot kinds, or capsule pair kinds
  int64_t rows = 0;                 // rows of a side per instance (cost_rows): the joint accelerations' weights find row T by it
};
typedef bool (*CostSideOk)(const CostCheck& c, const double* v, int64_t words);

static inline bool cost_weight_ok(double w) { return isfinite(w) && w >= 0.0; }
static inline bool cost_quat_ok(double norm2) { return isfinite(norm2) && fabs(sqrt(norm2) - 1.0) <= 1e-10; }

static inline bool cost_finite_side(const CostCheck&, const double* v, int64_t words) {
  for (int64_t i = 0; i < words; ++i)
    if (!isfinite(v[i])) return false;
  return true;
}
static inline bool cost_weight_side(const CostCheck&, const double* v, int64_t words) {
  for (int64_t i = 0; i < words; ++i)
    if (!cost_weight_ok(v[i])) return false;
  return true;
}
// unit quaternions x y z w (a non-finite entry fails too)
static inline bool cost_quat_side(const CostCheck&, const double* v, int64_t words) {
  for (int64_t k = 0; k < words; k += 4)
    if (!cost_quat_ok(v[k] * v[k] + v[k + 1] * v[k + 1] + v[k + 2] * v[k + 2] + v[k + 3] * v[k + 3])) return false;
  return true;
}
// aim targets (g, rho): finite, and a stand-off rho >= 0
static inline bool cost_aim_target_side(const CostCheck&, const double* v, int64_t words) {
  for (int64_t k = 0; k < words; k += 4) {
    if (!isfinite(v[k]) || !isfinite(v[k + 1]) || !isfinite(v[k + 2]) || !isfinite(v[k + 3])) return false;
    if (v[k + 3] < 0.0) return false;
  }
  return true;
}
// obstacle geometry by slot kind: a sphere's radius >= 0, a half-space's unit normal; a grid's shift and margin are finite, no more
// (a margin may be negative)
static inline bool cost_obstacle_geom_side(const CostCheck& c, const double* v, int64_t words) {
  for (int64_t i = 0; i < words / 4; ++i) {
    const double* g = v + 4 * i;
    if (!isfinite(g[0]) || !isfinite(g[1]) || !isfinite(g[2]) || !isfinite(g[3])) return false;
    const int32_t kind = c.kind[i % c.items];
    if (kind == DDP_HIP_OBSTACLE_SPHERE) {
      if (g[3] < 0.0) return false;
    } else if (kind == DDP_HIP_OBSTACLE_HALFSPACE && fabs(sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) - 1.0) > 1e-10) {
      return false;
    }
  }
  return true;
}
// capsule pair geometry by pair kind, eight doubles: all finite (the last is the margin, the ignored ones too); a world capsule
// (b0, b1, rho, m) has rho >= 0, a half-space (n, h, ., ., ., m) a unit normal by the obstacle half-spaces' rule; a grid pair's
// (s, ., ., ., ., m) needs no more than that; a box pair's (c, quaternion x y z w, m) has a unit quaternion by cost_quat_ok
static inline bool cost_capsule_geom_side(const CostCheck& c, const double* v, int64_t words) {
  for (int64_t i = 0; i < words / 8; ++i) {
    const double* g = v + 8 * i;
    for (int a = 0; a < 8; ++a)
      if (!isfinite(g[a])) return false;
    const int32_t kind = c.kind[i % c.items];
    if (kind == DDP_HIP_CAPSULE_VS_CAPSULE) {
      if (g[6] < 0.0) return false;
    } else if (kind == DDP_HIP_CAPSULE_VS_HALFSPACE) {
      if (fabs(sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) - 1.0) > 1e-10) return false;
    } else if (kind == DDP_HIP_CAPSULE_VS_BOX) {
      if (!cost_quat_ok(g[3] * g[3] + g[4] * g[4] + g[5] * g[5] + g[6] * g[6])) return false;
    }
  }
  return true;
}
// balance-region planes (n, h, tau): finite, a unit normal by the half-spaces' rule, a time constant tau >= 0
static inline bool cost_region_geom_side(const CostCheck&, const double* v, int64_t words) {
  for (int64_t k = 0; k < words; k += 5) {
    const double* g = v + k;
    if (!isfinite(g[0]) || !isfinite(g[1]) || !isfinite(g[2]) || !isfinite(g[3]) || !isfinite(g[4])) return false;
    if (fabs(sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]) - 1.0) > 1e-10) return false;
    if (g[4] < 0.0) return false;
  }
  return true;
}
// a limit's sides: no NaN, no lower bound of +inf, no upper bound of -inf
static inline bool cost_limit_lo_side(const CostCheck&, const double* v, int64_t words) {
  for (int64_t i = 0; i < words; ++i)
    if (isnan(v[i]) || v[i] == INFINITY) return false;
  return true;
}
static inline bool cost_limit_hi_side(const CostCheck&, const double* v, int64_t words) {
  for (int64_t i = 0; i < words; ++i)
    if (isnan(v[i]) || v[i] == -INFINITY) return false;
  return true;
}
// ... and its weights: a free-flyer root's pose rows carry no limit.  (The control-gravity term's weights alike, with one item per
// control row: a free-flyer root's six rows carry no term)
static inline bool cost_limit_weight_side(const CostCheck& c, const double* v, int64_t words) {
  for (int64_t i = 0; i < words; ++i) {
    if (!cost_weight_ok(v[i])) return false;
    if (c.ff && i % c.items < 6 && v[i] != 0.0) return false;
  }
  return true;
}
// the joint accelerations' weights: the record has T+1 rows (c.rows) but the term is of t < T alone, so row T carries no weight
static inline bool cost_stage_weight_side(const CostCheck& c, const double* v, int64_t words) {
  for (int64_t i = 0; i < words; ++i) {
    if (!cost_weight_ok(v[i])) return false;
    if (i / c.items % c.rows == c.rows - 1 && v[i] != 0.0) return false;
  }
  return true;
}

// a self-collision pair list over n_points spheres (sphere k on joint[k]): indices in range, a != b, and not both spheres on one
// joint (their distance is constant).  Duplicate pairs are allowed
static inline bool cost_pair_list_ok(int32_t n_points, const int32_t* joint, int32_t n_pairs, const int32_t* a, const int32_t* b) {
  for (int32_t i = 0; i < n_pairs; ++i) {
    if (a[i] < 0 || a[i] >= n_points || b[i] < 0 || b[i] >= n_points) return false;
    if (a[i] == b[i] || joint[a[i]] == joint[b[i]]) return false;
  }
  return true;
}

// a capsule pair list over n_capsules robot capsules (capsule k on joint[k]): body A in range, a known kind, and for a robot pair
// body B in range, a != b and not both capsules on one joint (their distance is constant); pair_b of a world pair is not read
// (a box pair's is its shape).
// Duplicate pairs are allowed.  grid_resident: the context holds a voxel grid, which a pair of kind DDP_HIP_CAPSULE_VS_GRID needs (the
// obstacle slots' rule).  n_boxes: the box shapes set, of which a pair of kind DDP_HIP_CAPSULE_VS_BOX names one by b (with none set every
// such pair is refused)
static inline bool cost_capsule_pairs_ok(int32_t n_capsules, const int32_t* joint, int32_t n_pairs, const int32_t* a, const int32_t* kind,
                                         const int32_t* b, bool grid_resident, int32_t n_boxes) {
  for (int32_t i = 0; i < n_pairs; ++i) {
    if (a[i] < 0 || a[i] >= n_capsules) return false;
    if (kind[i] == DDP_HIP_CAPSULE_VS_CAPSULE || kind[i] == DDP_HIP_CAPSULE_VS_HALFSPACE) continue;
    if (kind[i] == DDP_HIP_CAPSULE_VS_GRID) {
      if (!grid_resident) return false;
      continue;
    }
    if (kind[i] == DDP_HIP_CAPSULE_VS_BOX) {
      if (b[i] < 0 || b[i] >= n_boxes) return false;
      continue;
    }
    if (kind[i] != DDP_HIP_CAPSULE_VS_ROBOT) return false;
    if (b[i] < 0 || b[i] >= n_capsules) return false;
    if (a[i] == b[i] || joint[a[i]] == joint[b[i]]) return false;
  }
  return true;
}
// ... without boxes
static inline bool cost_capsule_pairs_ok(int32_t n_capsules, const int32_t* joint, int32_t n_pairs, const int32_t* a, const int32_t* kind,
                                         const int32_t* b, bool grid_resident) {
  return cost_capsule_pairs_ok(n_capsules, joint, n_pairs, a, kind, b, grid_resident, 0);
}
// ... and without a grid
static inline bool cost_capsule_pairs_ok(int32_t n_capsules, const int32_t* joint, int32_t n_pairs, const int32_t* a, const int32_t* kind,
                                         const int32_t* b) {
  return cost_capsule_pairs_ok(n_capsules, joint, n_pairs, a, kind, b, false);
}

// a relative-frame pair list over a model of nj joints (pair i: base frame on joint ja[i], tip frame on jb[i]): joints in range,
// ja != jb (on one joint the relative placement is constant), offsets finite.  Duplicate pairs, and a pair in both orders, are allowed
static inline bool cost_frame_pairs_ok(int32_t nj, int32_t n_pairs, const int32_t* ja, const double* offa, const int32_t* jb, const double* offb) {
  for (int32_t i = 0; i < n_pairs; ++i) {
    if (ja[i] < 0 || ja[i] >= nj || jb[i] < 0 || jb[i] >= nj || ja[i] == jb[i]) return false;
    for (int a = 0; a < 3; ++a)
      if (!isfinite(offa[3 * i + a]) || !isfinite(offb[3 * i + a])) return false;
  }
  return true;
}

// an aim-frame list over a model of nj joints (frame i: the point off[i] and the axis axis[i] of joint[i]): joints in range,
// offsets finite, axes of unit length by the quaternions' rule (cost_quat_ok).  Several frames on one joint are allowed
static inline bool cost_aim_frames_ok(int32_t nj, int32_t n_frames, const int32_t* joint, const double* off, const double* axis) {
  for (int32_t i = 0; i < n_frames; ++i) {
    if (joint[i] < 0 || joint[i] >= nj) return false;
    for (int a = 0; a < 3; ++a)
      if (!isfinite(off[3 * i + a])) return false;
    const double* x = axis + 3 * i;
    if (!cost_quat_ok(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])) return false;
  }
  return true;
}

static inline bool cost_any_nonzero(const double* v, int64_t words) {
  for (int64_t i = 0; i < words; ++i)
    if (v[i] != 0.0) return true;
  return false;
}

// flag off -> E_UNSUPPORTED, bad range -> E_ARG (uploads and downloads alike)
static inline int cost_range_check(uint32_t ctx_flags, const CostBlock& k, int64_t batch, int64_t first, int64_t count) {
  if (!(ctx_flags & k.desc->flag)) return DDP_HIP_E_UNSUPPORTED;
  if (first < 0 || count < 0 || first + count > batch) return DDP_HIP_E_ARG;
  return DDP_HIP_OK;
}

// Everything an upload decides before it touches the device, in this order: flag, range, layout, every side of the whole range
// (nothing is written unless all of it is valid).  *copy: there is something to write; *nonzero: the weights carry a non-zero
static inline int cost_upload_check(uint32_t ctx_flags, const CostBlock& k, const CostCheck& c, int64_t batch, int64_t T,
                                    const double* const* host, const CostSideOk* ok, int64_t first, int64_t count, bool* copy,
                                    bool* nonzero) {
  *copy = *nonzero = false;
  const int rc = cost_range_check(ctx_flags, k, batch, first, count);
  if (rc != DDP_HIP_OK) return rc;
  if (k.items == 0) return DDP_HIP_E_ARG;                             // no frames / points set: the arrays have no shape yet
  bool any = false;
  for (int s = 0; s < k.desc->nside; ++s) {
    if (!host[s]) continue;
    any = true;
    if (!ok[s](c, host[s], cost_side_words(k, s, T) * count)) return DDP_HIP_E_ARG;
  }
  *copy = count != 0 && any;
  const int w = k.desc->nside - 1;
  *nonzero = host[w] && cost_any_nonzero(host[w], cost_side_words(k, w, T) * count);
  return DDP_HIP_OK;
}

// The live rule: an upload of weights with a non-zero entry switches the term's kernels on; only ONE upload of zeros for the
// whole batch (first 0, count batch) switches them off again.  Zeros arriving range by range leave the kernels launched, with
// the same bits: they skip zero weights themselves
static inline bool cost_live_rule(bool live, bool nonzero, int64_t first, int64_t count, int64_t batch) {
  return nonzero || (live && !(first == 0 && count == batch));
}
