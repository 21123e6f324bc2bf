// The device-free parts of the control-gravity term (DDP_HIP_FLAG_CONTROL_GRAV_COST; ddp_pinocchio_amd/csrc/cost_block.h): its
// record -- the first with T rows per instance, not T+1 -- and what an upload of offsets and weights decides before it touches a
// device: the validators, the rule for a free-flyer root's six rows, the live rule.  No HIP, no device: a plain host program.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "../ddp_pinocchio_amd/csrc/cost_block.h"

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
  } while (0)

static const int64_t B = 3, T = 4;
static const int32_t M = 8;                                            // control rows: a free-flyer root's six, then two joints
static const uint32_t ON = DDP_HIP_FLAG_CONTROL_GRAV_COST;

static CostBlock block() {
  CostBlock k;
  k.desc = &kCostDesc[COST_CONTROL_GRAV];
  k.max_items = M;                                                     // (COST_ITEMS_CONTROL: set at create from the problem's m)
  k.items = M;
  return k;
}

static int check(bool ff, const std::vector<double>& offset, const std::vector<double>& weight, int64_t first, int64_t count, bool* copy,
                 bool* nonzero, uint32_t flags = ON) {
  const CostBlock k = block();
  CostCheck c;
  c.items = M;
  c.ff = ff;
  const double* host[COST_MAX_SIDES] = {offset.empty() ? nullptr : offset.data(), weight.empty() ? nullptr : weight.data(), nullptr};
  const CostSideOk ok[] = {cost_finite_side, cost_limit_weight_side};
  return cost_upload_check(flags, k, c, B, T, host, ok, first, count, copy, nonzero);
}

int main() {
  const double nan = NAN, inf = INFINITY;
  bool copy, nonzero;

  // ---- the record: offset | weight per control row, T rows, a candidates' array, fixed; its index stands in front of the run ------
  // ---- momentum, relative frames, obstacles, self-collision that the sibling programs hold together (the order of additions is the
  // ---- launch lists', not the enumerators') ---------------------------------------------------------------------------------------
  {
    const CostDesc& d = kCostDesc[COST_CONTROL_GRAV];
    CHECK(COST_CONTROL_GRAV == COST_FRAME_VEL + 1 && COST_CONTROL_GRAV == COST_MOMENTUM - 1);
    CHECK(COST_RELATIVE_FRAME == COST_MOMENTUM + 1 && COST_RELATIVE_FRAME == COST_OBSTACLE - 1);   // (what test_relative_frame_block.cpp holds)
    CHECK(COST_SELF_COLLISION == COST_OBSTACLE + 1 && COST_SELF_COLLISION == COST_COUNT - 1);      // (... and test_self_collision_block.cpp)
    CHECK(d.flag == 8192u);
    CHECK(d.nside == 2 && d.unit[0] == 1 && d.unit[1] == 1);
    CHECK(d.fill[0] == FILL_ZERO && d.fill[1] == FILL_ZERO);
    CHECK(d.max_items == COST_ITEMS_CONTROL && d.fixed && d.cand && d.stage_only);
    const CostBlock k = block();
    CHECK(cost_rows(k, T) == T);                                         // no terminal row: the public shape [T][m] is the record's
    CHECK(cost_side_words(k, 0, T) == T * M && cost_side_words(k, 1, T) == T * M);
    for (int t = 0; t < COST_COUNT; ++t) {                               // every other term keeps its T+1 rows; no flag twice
      CostBlock o;
      o.desc = &kCostDesc[t];
      o.items = 1;
      CHECK(cost_rows(o, T) == (t == COST_CONTROL_GRAV ? T : T + 1));
      CHECK(kCostDesc[t].stage_only == (t == COST_CONTROL_GRAV));
      for (int u = t + 1; u < COST_COUNT; ++u) CHECK(kCostDesc[t].flag != kCostDesc[u].flag);
    }
  }

  // ---- an upload's decisions: the words of a range are count x T x m, not count x (T+1) x m -------------------------------------
  {
    const size_t words = (size_t)(B * T * M);
    std::vector<double> o(words, -0.25), w(words, 0.0);
    CHECK(check(false, o, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    w[words - 1] = 1e-300;                                               // the last double of the range is read ...
    CHECK(check(false, o, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(false, o, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);   // ... and nothing beyond it
    CHECK(check(false, {}, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(false, o, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    CHECK(check(false, {}, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);
    for (double bad : {nan, inf, -inf}) {                                // a non-finite offset
      std::vector<double> ob = o;
      ob[words - 1] = bad;
      CHECK(check(false, ob, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(false, ob, {}, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(false, ob, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK);
    }
    for (double bad : {-1e-300, nan, inf, -inf}) {                       // a negative or non-finite weight
      std::vector<double> wb = w;
      wb[M + 7] = bad;
      CHECK(check(false, o, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(false, {}, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(true, {}, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
    }
    CHECK(check(false, o, w, 1, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);             // bad ranges
    CHECK(check(false, o, w, -1, 1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(false, o, w, 0, -1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(false, o, w, B, 0, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);
    CHECK(check(false, o, w, 0, B, &copy, &nonzero, DDP_HIP_FLAG_STATE_LIMITS | DDP_HIP_FLAG_TRACKING_COST) == DDP_HIP_E_UNSUPPORTED);   // the flag stands alone
    CHECK(check(false, o, w, -1, 1, &copy, &nonzero, 0) == DDP_HIP_E_UNSUPPORTED);          // ... and is checked first
  }

  // ---- the root-row rule: a free-flyer root's six rows carry no term -------------------------------------------------------------
  {
    const size_t words = (size_t)(B * T * M);
    std::vector<double> w(words, 0.0);
    for (size_t i = 0; i < words; ++i)
      if (i % M >= 6) w[i] = 0.5;
    CHECK(check(true, {}, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    for (int row : {0, 5})
      for (size_t bt : {(size_t)0, (size_t)(B * T - 1)}) {               // the first and the last (instance, t) of the range
        std::vector<double> wb = w;
        wb[bt * M + row] = 1e-300;
        CHECK(check(true, {}, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
        CHECK(check(false, {}, wb, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy);          // a fixed base: every row takes a weight
      }
    std::vector<double> w6 = w;                                          // row 6 is the first joint's
    w6[6] = 2.0;
    CHECK(check(true, {}, w6, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    std::vector<double> o(words, 3.0);                                   // offsets on the root rows are data without a term: accepted
    CHECK(check(true, o, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
  }

  // ---- the live rule on half-batch uploads --------------------------------------------------------------------------------------
  {
    bool live = false;
    live = cost_live_rule(live, true, 1, 1, B);                          // one instance's non-zero weights switch the kernels on
    CHECK(live);
    live = cost_live_rule(live, false, 0, 2, B);                         // zeros range by range leave them launched
    CHECK(live);
    live = cost_live_rule(live, false, 2, B - 2, B);
    CHECK(live);
    live = cost_live_rule(live, false, 0, B, B);                         // one upload of zeros for the whole batch switches them off
    CHECK(!live);
    live = cost_live_rule(live, false, 0, B - 1, B);
    CHECK(!live);
  }

  if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
  printf("control_grav_block: all checks passed\n");
  return 0;
}
