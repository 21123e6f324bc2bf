// The device-free parts of the receding-horizon advance (ddp_hip_advance; ddp_pinocchio_amd/csrc/advance_plan.h): the descriptor of
// every array a context's flags and layouts imply -- enumerated over kCostDesc, so that a cost term added later is either moved or
// fails here --, the row-source function, the per-word upward walk the kernel runs (adv_walk_column, as it stands) on host arrays
// in place against a shift made from a copy, and the argument checks.  No HIP, no device: a plain host program.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../ddp_pinocchio_amd/csrc/advance_plan.h"

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
  } while (0)

static const int64_t B = 3;
static const int32_t NV = 8, N = 16, M = 8, NX = 17;                     // a free-flyer shape: nx = n + 1

// every term on, laid out: the fixed ones by their room, the others by fewer items than their room (items != max_items)
static void blocks(CostBlock* cost) {
  for (int t = 0; t < COST_COUNT; ++t) {
    CostBlock& k = cost[t];
    k = CostBlock();
    k.desc = &kCostDesc[t];
    const int32_t room = k.desc->max_items;
    k.max_items = room == COST_ITEMS_STATE ? N : room == COST_ITEMS_CONTROL ? M : room == COST_ITEMS_VELOCITY ? NV : room;
    k.items = k.desc->fixed ? k.max_items : (k.max_items > 1 ? k.max_items - 1 : 1);
  }
}

static uint32_t all_flags() {
  uint32_t f = DDP_HIP_FLAG_TRACKING_COST | DDP_HIP_FLAG_CONTROL_BOUNDS;
  for (int t = 0; t < COST_COUNT; ++t) f |= kCostDesc[t].flag;
  return f;
}

static const AdvArray* find(const AdvArray* plan, int n, int kind, int id, int side) {
  const AdvArray* hit = nullptr;
  for (int k = 0; k < n; ++k)
    if (plan[k].kind == kind && plan[k].id == id && plan[k].side == side) {
      CHECK(!hit);                                                       // once
      hit = &plan[k];
    }
  return hit;
}

// the plan of one horizon: what is in it, and with what shape
static void check_plan(int64_t T) {
  CostBlock cost[COST_COUNT];
  blocks(cost);
  AdvArray plan[ADV_MAX_ARRAYS];
  const int n = adv_plan_build(all_flags(), T, N, M, NX, cost, plan);
  int sides = 0;
  for (int t = 0; t < COST_COUNT; ++t) {
    const CostDesc& d = kCostDesc[t];
    CHECK(d.nside >= 1 && d.nside <= COST_MAX_SIDES);
    for (int s = 0; s < d.nside; ++s, ++sides) {
      const AdvArray* a = find(plan, n, ADV_COST, t, s);
      CHECK(a != nullptr);
      if (!a) continue;
      CHECK(a->rule == ADV_HOLD && a->rows == T);
      CHECK(a->terminal == !d.stage_only);
      CHECK(a->width == (int64_t)cost[t].items * d.unit[s]);
      CHECK(adv_inst_words(*a) == cost_side_words(cost[t], s, T));       // the advance and the uploads agree on the array
    }
  }
  CHECK(n == 10 + sides && n <= ADV_MAX_ARRAYS);
  struct { int id, rule; int64_t rows, width; bool terminal; } seqs[] = {
      {DDP_HIP_SEQ_X, ADV_TRAJ, T + 1, NX, false},       {DDP_HIP_SEQ_U, ADV_HOLD, T, M, false},
      {DDP_HIP_SEQ_FB_VAL, ADV_ZERO, T, M, false},       {DDP_HIP_SEQ_FB_JAC, ADV_ZERO_TAIL, T, (int64_t)M * N, false},
      {DDP_HIP_SEQ_COST_XREF, ADV_HOLD, T, NX, true},    {DDP_HIP_SEQ_COST_WX, ADV_HOLD, T, N, true},
      {DDP_HIP_SEQ_COST_UREF, ADV_HOLD, T, M, false},    {DDP_HIP_SEQ_COST_WU, ADV_HOLD, T, M, false},
      {DDP_HIP_SEQ_CTRL_LO, ADV_HOLD, T, M, false},      {DDP_HIP_SEQ_CTRL_HI, ADV_HOLD, T, M, false}};
  for (const auto& q : seqs) {
    const AdvArray* a = find(plan, n, ADV_SEQ, q.id, 0);
    CHECK(a != nullptr);
    if (a) CHECK(a->rule == q.rule && a->rows == q.rows && a->width == q.width && a->terminal == q.terminal);
  }
  // nothing else moves: BOX_STAT, the costs, the candidates, the derivatives, X_NEW / U_NEW and the origins (written whole afterwards)
  for (int id : {(int)DDP_HIP_SEQ_BOX_STAT, (int)DDP_HIP_SEQ_COSTS_OLD, (int)DDP_HIP_SEQ_COSTS_NEW, (int)DDP_HIP_SEQ_X_NEW, (int)DDP_HIP_SEQ_U_NEW,
                 (int)DDP_HIP_SEQ_FB_ORIGIN, (int)DDP_HIP_SEQ_MULT_ORIGIN, (int)DDP_HIP_SEQ_MULT_VAL, (int)DDP_HIP_SEQ_LX, (int)DDP_HIP_SEQ_FX})
    CHECK(find(plan, n, ADV_SEQ, id, 0) == nullptr);

  // a flag off, or a block without a layout, takes its arrays out; the four of every context stay
  CHECK(adv_plan_build(0, T, N, M, NX, cost, plan) == 4);
  CHECK(adv_plan_build(DDP_HIP_FLAG_TRACKING_COST, T, N, M, NX, cost, plan) == 8);
  CHECK(adv_plan_build(DDP_HIP_FLAG_CONTROL_BOUNDS, T, N, M, NX, cost, plan) == 6);
  for (int t = 0; t < COST_COUNT; ++t) {
    CHECK(adv_plan_build(kCostDesc[t].flag, T, N, M, NX, cost, plan) == 4 + kCostDesc[t].nside);
    CostBlock bare[COST_COUNT];
    blocks(bare);
    bare[t].items = 0;
    CHECK(adv_plan_build(kCostDesc[t].flag, T, N, M, NX, bare, plan) == 4);
  }
}

// every array of the plan, filled with values that differ in every (instance, row, word), walked in place word by word as the
// kernel's lanes walk it, against the shift made from a copy by the row-source function
static void check_walk(int64_t T, int64_t s, bool with_x0) {
  CostBlock cost[COST_COUNT];
  blocks(cost);
  AdvArray plan[ADV_MAX_ARRAYS];
  const int n = adv_plan_build(all_flags(), T, N, M, NX, cost, plan);
  std::vector<double> x0((size_t)(B * NX));
  for (size_t i = 0; i < x0.size(); ++i) x0[i] = -1000.0 - (double)i;
  for (int k = 0; k < n; ++k) {
    const AdvArray& a = plan[k];
    const int64_t iw = adv_inst_words(a);
    std::vector<double> old((size_t)(B * iw));
    for (size_t i = 0; i < old.size(); ++i) old[i] = 1.0 + (double)i + 0.001 * k;
    std::vector<double> got = old, ref = old;
    for (int64_t b = 0; b < B; ++b)
      for (int64_t t = 0; t < a.rows; ++t)
        for (int64_t w = 0; w < a.width; ++w) {
          const int64_t src = adv_row_source(a.rule, a.rows, s, t);
          double v = src < 0 ? 0.0 : old[(size_t)(b * iw + src * a.width + w)];
          if (a.rule == ADV_TRAJ && with_x0 && t == 0) v = x0[(size_t)(b * a.width + w)];
          ref[(size_t)(b * iw + t * a.width + w)] = v;
        }
    for (int64_t lane = 0; lane < B * a.width; ++lane) {                 // the kernel's flattening: instance x words of a row
      const int64_t b = lane / a.width, w = lane - b * a.width;
      const double* first = a.rule == ADV_TRAJ && with_x0 ? &x0[(size_t)(b * a.width + w)] : nullptr;
      adv_walk_column(got.data() + b * iw + w, a.width, a.rows, a.rule, s, first);
    }
    CHECK(memcmp(got.data(), ref.data(), sizeof(double) * got.size()) == 0);
    if (a.terminal)                                                      // row T is where it was
      for (int64_t b = 0; b < B; ++b)
        CHECK(memcmp(&got[(size_t)(b * iw + T * a.width)], &old[(size_t)(b * iw + T * a.width)], sizeof(double) * (size_t)a.width) == 0);
    // the rules in words: a tail row holds the last stage row (or zeros), row 0 the old row s
    if (a.rule == ADV_HOLD) CHECK(got[(size_t)((a.rows - 1) * a.width)] == old[(size_t)((a.rows - 1) * a.width)]);
    if (a.rule == ADV_HOLD || a.rule == ADV_ZERO_TAIL) CHECK(got[0] == (s < a.rows ? old[(size_t)(s * a.width)] : a.rule == ADV_HOLD ? old[(size_t)((a.rows - 1) * a.width)] : 0.0));
    if (a.rule == ADV_ZERO_TAIL) CHECK(got[(size_t)((a.rows - 1) * a.width)] == 0.0);
    if (a.rule == ADV_TRAJ) CHECK(got[(size_t)(T * a.width)] == old[(size_t)(T * a.width)] && got[0] == (with_x0 ? x0[0] : old[(size_t)(s * a.width)]));
  }
}

int main() {
  // ---- the row-source function ------------------------------------------------------------------------------------------------------
  CHECK(adv_row_source(ADV_HOLD, 5, 1, 0) == 1 && adv_row_source(ADV_HOLD, 5, 1, 3) == 4 && adv_row_source(ADV_HOLD, 5, 1, 4) == 4);
  CHECK(adv_row_source(ADV_HOLD, 5, 5, 0) == 4 && adv_row_source(ADV_HOLD, 5, 4, 0) == 4 && adv_row_source(ADV_HOLD, 5, 4, 1) == 4);
  CHECK(adv_row_source(ADV_ZERO_TAIL, 5, 2, 2) == 4 && adv_row_source(ADV_ZERO_TAIL, 5, 2, 3) == -1 && adv_row_source(ADV_ZERO_TAIL, 5, 5, 0) == -1);
  CHECK(adv_row_source(ADV_ZERO, 5, 1, 0) == -1 && adv_row_source(ADV_ZERO, 5, 1, 4) == -1);
  CHECK(adv_row_source(ADV_TRAJ, 6, 5, 0) == 5 && adv_row_source(ADV_TRAJ, 6, 5, 1) == 5 && adv_row_source(ADV_TRAJ, 6, 1, 4) == 5);   // X[t] = old[t + s], t <= T - s

  // ---- the plan and the walk: T in {1, 2, 5}, every s in 1 .. T; 12 and 20 put the unrolled part of the walk to work ----------------
  for (int64_t T : {(int64_t)1, (int64_t)2, (int64_t)5, (int64_t)12, (int64_t)20}) {
    check_plan(T);
    for (int64_t s = 1; s <= T; ++s)
      for (bool with_x0 : {false, true}) check_walk(T, s, with_x0);
  }

  // ---- the argument checks, in their order ------------------------------------------------------------------------------------------
  {
    const int64_t T = 5;
    std::vector<double> x0((size_t)(B * NX), 0.25);
    for (int64_t b = 0; b < B; ++b) { x0[(size_t)(b * NX + 3)] = 0.0; x0[(size_t)(b * NX + 4)] = 0.6; x0[(size_t)(b * NX + 5)] = 0.0; x0[(size_t)(b * NX + 6)] = 0.8; }
    for (int mode : {DDP_HIP_ADVANCE_NO_ROLL, DDP_HIP_ADVANCE_OPEN_LOOP, DDP_HIP_ADVANCE_CLOSED_LOOP}) {
      CHECK(adv_args_check(T, 0, B, NX, true, 1, nullptr, mode) == DDP_HIP_OK);
      CHECK(adv_args_check(T, 0, B, NX, true, T, x0.data(), mode) == DDP_HIP_OK);
      CHECK(adv_args_check(T, 0, B, NX, true, 0, nullptr, mode) == DDP_HIP_E_ARG);
      CHECK(adv_args_check(T, 0, B, NX, true, T + 1, nullptr, mode) == DDP_HIP_E_ARG);
      CHECK(adv_args_check(T, 0, B, NX, true, -1, nullptr, mode) == DDP_HIP_E_ARG);
      CHECK(adv_args_check(T, 7, B, NX, true, 1, nullptr, mode) == DDP_HIP_E_UNSUPPORTED);   // constraint rows
      CHECK(adv_args_check(T, 7, B, NX, true, 0, nullptr, mode) == DDP_HIP_E_ARG);           // ... after the arguments
    }
    CHECK(adv_args_check(T, 0, B, NX, true, 1, nullptr, 3) == DDP_HIP_E_ARG && adv_args_check(T, 0, B, NX, true, 1, nullptr, -1) == DDP_HIP_E_ARG);
    for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY})
      for (size_t at : {(size_t)0, x0.size() - 1, (size_t)(NX + 9)}) {
        std::vector<double> xb = x0;
        xb[at] = bad;
        CHECK(adv_args_check(T, 0, B, NX, true, 1, xb.data(), 0) == DDP_HIP_E_ARG);
        CHECK(adv_args_check(T, 0, B, NX, false, 1, xb.data(), 0) == DDP_HIP_E_ARG);
      }
    std::vector<double> xq = x0;                                         // the last instance's root quaternion off unit length
    xq[(size_t)((B - 1) * NX + 6)] = 0.8 + 1e-9;
    CHECK(adv_args_check(T, 0, B, NX, true, 1, xq.data(), 0) == DDP_HIP_E_ARG);
    CHECK(adv_args_check(T, 0, B, NX, false, 1, xq.data(), 0) == DDP_HIP_OK);                // (no quaternion without a free flyer)
    CHECK(adv_args_check(T, 0, B - 1, NX, true, 1, xq.data(), 0) == DDP_HIP_OK);             // (outside the batch: not read)
    xq[(size_t)((B - 1) * NX + 6)] = 0.8 + 1e-12;
    CHECK(adv_args_check(T, 0, B, NX, true, 1, xq.data(), 0) == DDP_HIP_OK);
  }

  if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
  printf("advance_plan: all checks passed\n");
  return 0;
}
