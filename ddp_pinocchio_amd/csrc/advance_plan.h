// advance_plan.h -- the receding-horizon advance (ddp_hip_advance) as far as it calls no HIP function: which
// resident arrays a context's flags and layouts imply, what a row of each becomes, the per-word walk that moves one column of an
// array in place, and the argument checks.  Host code without a device dependency, in the manner of cost_block.h: advance.hip
// builds the entry point on it (its kernel runs adv_walk_column as it stands here), host/test_advance_plan.cpp runs it alone.
#pragma once

#include <math.h>
#include <stdint.h>

#include "cost_block.h"
#include "ddp_hip/ddp_hip.h"

#if defined(__HIPCC__)
#define ADV_HD __host__ __device__
#else
#define ADV_HD
#endif

// What the rows of an array become when the window moves on by s steps; `rows` counts the rows the rule walks (a terminal row
// is not among them), "old" is the value before the call
enum AdvRule : int32_t {
  ADV_HOLD,        // row[t] = old[t + s] for t < rows - s, old[rows - 1] after: the tail holds the last row
  ADV_ZERO_TAIL,   // row[t] = old[t + s] for t < rows - s, exact zeros after (the gains: no feedback where nothing was solved)
  ADV_ZERO,        // zeros everywhere (FB_VAL: the feed-forward step has been taken)
  ADV_TRAJ,        // ADV_HOLD over the T + 1 rows of X, then row 0 from the measured state where one was given
};

enum AdvKind : int32_t { ADV_SEQ, ADV_COST };   // a resident sequence (ddp_hip_seq), or side `side` of add-on cost term `id`

struct AdvArray {
  int32_t kind;      // AdvKind
  int32_t id;        // ddp_hip_seq, or CostTerm
  int32_t side;      // of a cost term
  int32_t rule;      // AdvRule
  int64_t rows;      // rows the rule walks: T, or T + 1 for the trajectory
  int64_t width;     // words per row
  bool terminal;     // one more row, T, follows the walked ones and is not touched: the terminal cost belongs to the end of the window
};

#define ADV_MAX_ARRAYS (10 + COST_COUNT * COST_MAX_SIDES)

// words per instance
static inline int64_t adv_inst_words(const AdvArray& a) { return (a.rows + (a.terminal ? 1 : 0)) * a.width; }

// Every array an advance moves, for a context of these flags whose cost blocks are laid out as `cost` says (items, not max_items;
// a block without a layout has no rows yet).  out: room for ADV_MAX_ARRAYS.  Returns the count
static inline int adv_plan_build(uint32_t flags, int64_t T, int64_t n, int64_t m, int64_t nx, const CostBlock* cost, AdvArray* out) {
  int k = 0;
  auto seq = [&](int id, int rule, int64_t rows, int64_t width, bool terminal) {
    out[k++] = AdvArray{ADV_SEQ, id, 0, rule, rows, width, terminal};
  };
  seq(DDP_HIP_SEQ_X, ADV_TRAJ, T + 1, nx, false);
  seq(DDP_HIP_SEQ_U, ADV_HOLD, T, m, false);
  seq(DDP_HIP_SEQ_FB_VAL, ADV_ZERO, T, m, false);
  seq(DDP_HIP_SEQ_FB_JAC, ADV_ZERO_TAIL, T, m * n, false);
  if (flags & DDP_HIP_FLAG_TRACKING_COST) {
    seq(DDP_HIP_SEQ_COST_XREF, ADV_HOLD, T, nx, true);
    seq(DDP_HIP_SEQ_COST_WX, ADV_HOLD, T, n, true);
    seq(DDP_HIP_SEQ_COST_UREF, ADV_HOLD, T, m, false);
    seq(DDP_HIP_SEQ_COST_WU, ADV_HOLD, T, m, false);
  }
  if (flags & DDP_HIP_FLAG_CONTROL_BOUNDS) {
    seq(DDP_HIP_SEQ_CTRL_LO, ADV_HOLD, T, m, false);
    seq(DDP_HIP_SEQ_CTRL_HI, ADV_HOLD, T, m, false);
  }
  for (int term = 0; term < COST_COUNT; ++term) {
    const CostBlock& b = cost[term];
    if (!b.desc || !(flags & b.desc->flag) || b.items <= 0) continue;
    for (int s = 0; s < b.desc->nside; ++s)
      out[k++] = AdvArray{ADV_COST, term, s, ADV_HOLD, T, (int64_t)b.items * b.desc->unit[s], !b.desc->stage_only};
  }
  return k;
}

// The row of the old array that row t takes after an advance by s (t < rows); -1: exact zeros
ADV_HD static inline int64_t adv_row_source(int32_t rule, int64_t rows, int64_t s, int64_t t) {
  if (rule == ADV_ZERO) return -1;
  if (t + s < rows) return t + s;
  return rule == ADV_ZERO_TAIL ? -1 : rows - 1;
}

// One word of a row through all walked rows of one instance, in place.  Single-use streams: on the device the loads and the
// stores bypass the caches' retention
#if defined(__HIP_DEVICE_COMPILE__)
#define ADV_LOAD(p) __builtin_nontemporal_load(p)
#define ADV_STORE(p, v) __builtin_nontemporal_store((v), (p))
#else
#define ADV_LOAD(p) (*(p))
#define ADV_STORE(p, v) (*(p) = (v))
#endif
#define ADV_UNROLL 8
#if defined(__clang__)
#define ADV_UNROLL_LOOP _Pragma("unroll")
#else
#define ADV_UNROLL_LOOP
#endif

// The walk of one column: col is the word in row 0, `stride` the words per row, `first` (or null) the word that row 0 takes
// instead (ADV_TRAJ: the measured state).  t goes upward; row t + s is loaded and row t stored.  The hazard argument: a store
// to row t comes after the loads of rows s .. t + s, and the loads still to come are of rows above t + s; as s >= 1, row t is
// either loaded already (t >= s) or never loaded (t < s), whatever the distance by which the loads run ahead.  The tail's value,
// old row rows - 1, is read before the first store.  No other lane touches the column: no barrier, no scratch copy, and
// ADV_UNROLL loads are in flight before their stores are issued
ADV_HD static inline void adv_walk_column(double* col, int64_t stride, int64_t rows, int32_t rule, int64_t s, const double* first) {
  if (rule == ADV_ZERO) {
    for (int64_t t = 0; t < rows; ++t) ADV_STORE(col + t * stride, 0.0);
    return;
  }
  const int64_t keep = rows > s ? rows - s : 0;   // rows that take a shifted value
  const double tail = rule == ADV_ZERO_TAIL ? 0.0 : ADV_LOAD(col + (rows - 1) * stride);
  const double head = first ? *first : 0.0;
  int64_t t = 0;
  for (; t + ADV_UNROLL <= keep; t += ADV_UNROLL) {
    double v[ADV_UNROLL];
    ADV_UNROLL_LOOP
    for (int k = 0; k < ADV_UNROLL; ++k) v[k] = ADV_LOAD(col + (t + k + s) * stride);
    ADV_UNROLL_LOOP
    for (int k = 0; k < ADV_UNROLL; ++k) ADV_STORE(col + (t + k) * stride, v[k]);
  }
  for (; t < keep; ++t) {
    const double v = ADV_LOAD(col + (t + s) * stride);
    ADV_STORE(col + t * stride, v);
  }
  for (; t < rows; ++t) ADV_STORE(col + t * stride, tail);
  if (first) ADV_STORE(col, head);
}

// Everything ddp_hip_advance refuses, before anything is written, in this order: the arguments (DDP_HIP_E_ARG), the measured
// states (a non-finite entry; on a free-flyer model a root quaternion off unit length by cost_quat_ok's rule: DDP_HIP_E_ARG), a
// context with constraint rows (DDP_HIP_E_UNSUPPORTED: ne[t] varies with t and the batch shares eq_target, so the multipliers
// have no well-defined shift).  x0: [batch][nx] or null
static inline int adv_args_check(int64_t T, int64_t Etot, int64_t batch, int64_t nx, bool ff, int64_t shift, const double* x0, int32_t mode) {
  if (shift < 1 || shift > T) return DDP_HIP_E_ARG;
  if (mode != DDP_HIP_ADVANCE_NO_ROLL && mode != DDP_HIP_ADVANCE_OPEN_LOOP && mode != DDP_HIP_ADVANCE_CLOSED_LOOP) return DDP_HIP_E_ARG;
  if (x0) {
    for (int64_t i = 0; i < batch * nx; ++i)
      if (!isfinite(x0[i])) return DDP_HIP_E_ARG;
    if (ff)
      for (int64_t b = 0; b < batch; ++b) {
        const double* qt = x0 + b * nx + 3;
        if (!cost_quat_ok(qt[0] * qt[0] + qt[1] * qt[1] + qt[2] * qt[2] + qt[3] * qt[3])) return DDP_HIP_E_ARG;
      }
  }
  if (Etot > 0) return DDP_HIP_E_UNSUPPORTED;
  return DDP_HIP_OK;
}
