// The device-free parts of the joint-acceleration term (DDP_HIP_FLAG_JOINT_ACCEL_COST; ddp_pinocchio_amd/csrc/cost_block.h): its
// record -- one item per tangent row of v, T+1 rows of which row T belongs to no term -- and what an upload of targets and
// weights decides before it touches a device: the validators, the rule for row T, the live rule.  No HIP, no device: a plain
// host program.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "../ddp_pinocchio_amd/csrc/cost_block.h"

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
  } while (0)

static const int64_t B = 3, T = 4, T1 = T + 1;
static const int32_t NV = 8;                                           // tangent rows of v: a free-flyer root's six, then two joints
static const uint32_t ON = DDP_HIP_FLAG_JOINT_ACCEL_COST;

static CostBlock block() {
  CostBlock k;
  k.desc = &kCostDesc[COST_JOINT_ACCEL];
  k.max_items = NV;                                                    // (COST_ITEMS_VELOCITY: set at create from the problem's nv)
  k.items = NV;
  return k;
}

static int check(bool ff, const std::vector<double>& target, const std::vector<double>& weight, int64_t first, int64_t count, bool* copy,
                 bool* nonzero, uint32_t flags = ON) {
  const CostBlock k = block();
  CostCheck c;
  c.items = NV;
  c.ff = ff;
  c.rows = cost_rows(k, T);
  const double* host[COST_MAX_SIDES] = {target.empty() ? nullptr : target.data(), weight.empty() ? nullptr : weight.data(), nullptr};
  const CostSideOk ok[] = {cost_finite_side, cost_stage_weight_side};
  return cost_upload_check(flags, k, c, B, T, host, ok, first, count, copy, nonzero);
}

// weights 0.5 on every row t < T, 0 in row T
static std::vector<double> stage_weights() {
  std::vector<double> w((size_t)(B * T1 * NV), 0.0);
  for (size_t i = 0; i < w.size(); ++i)
    if ((int64_t)(i / NV) % T1 != T) w[i] = 0.5;
  return w;
}

int main() {
  const double nan = NAN, inf = INFINITY;
  bool copy, nonzero;

  // ---- the record: target | weight per tangent row of v, T+1 rows, a candidates' array, fixed; its index stands in front of the
  // ---- limits', every adjacency behind it as the sibling programs hold them (the order of additions is the launch lists') ---------
  {
    const CostDesc& d = kCostDesc[COST_JOINT_ACCEL];
    CHECK(COST_FRAME == 0 && COST_ORIENT == 2);                          // (the capsules' index stands between the two: test_capsule_block.cpp)
    CHECK(COST_JOINT_ACCEL == COST_ORIENT + 1 && COST_JOINT_ACCEL == COST_LIMITS - 1);
    CHECK(COST_BALANCE_REGION == COST_LIMITS + 1 && COST_COM == COST_BALANCE_REGION + 1);
    CHECK(COST_FRAME_AIM == COST_COM + 1 && COST_FRAME_VEL == COST_FRAME_AIM + 1);
    CHECK(COST_CONTROL_GRAV == COST_FRAME_VEL + 1 && COST_MOMENTUM == COST_CONTROL_GRAV + 1);
    CHECK(COST_RELATIVE_FRAME == COST_MOMENTUM + 1 && COST_OBSTACLE == COST_RELATIVE_FRAME + 1);
    CHECK(COST_SELF_COLLISION == COST_OBSTACLE + 1 && COST_SELF_COLLISION == COST_COUNT - 1);
    CHECK(d.flag == 65536u);
    CHECK(d.nside == 2 && d.unit[0] == 1 && d.unit[1] == 1);
    CHECK(d.fill[0] == FILL_ZERO && d.fill[1] == FILL_ZERO);
    CHECK(d.max_items == COST_ITEMS_VELOCITY && d.fixed && d.cand && !d.stage_only);
    const CostBlock k = block();
    CHECK(cost_rows(k, T) == T1);                                        // a terminal row like the other records': it carries no term
    CHECK(cost_side_words(k, 0, T) == T1 * NV && cost_side_words(k, 1, T) == T1 * NV);
    for (int t = 0; t < COST_COUNT; ++t) {                               // stage_only stays the control-gravity term's alone; no flag twice
      CHECK(kCostDesc[t].stage_only == (t == COST_CONTROL_GRAV));
      for (int u = t + 1; u < COST_COUNT; ++u) CHECK(kCostDesc[t].flag != kCostDesc[u].flag);
    }
  }

  // ---- an upload's decisions: the words of a range are count x (T+1) x nv ---------------------------------------------------------
  {
    const size_t words = (size_t)(B * T1 * NV);
    std::vector<double> a(words, -0.25), w(words, 0.0);
    CHECK(check(false, a, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    const size_t last = words - NV - 1;                                  // the last weight of the range that belongs to a term: row T-1
    w[last] = 1e-300;
    CHECK(check(false, a, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(false, a, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);   // ... and nothing beyond the range
    CHECK(check(false, {}, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(false, a, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    CHECK(check(false, {}, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);
    for (double bad : {nan, inf, -inf}) {                                // a non-finite target, row T's included (one copy per side)
      for (size_t at : {words - 1, (size_t)3}) {
        std::vector<double> ab = a;
        ab[at] = bad;
        CHECK(check(false, ab, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
        CHECK(check(false, ab, {}, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      }
      std::vector<double> ab = a;
      ab[words - 1] = bad;
      CHECK(check(false, ab, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK);
    }
    for (double bad : {-1e-300, nan, inf, -inf}) {                       // a negative or non-finite weight, in a stage row or in row T
      for (size_t at : {(size_t)(NV + 7), (size_t)(T * NV + 2)}) {
        std::vector<double> wb = w;
        wb[at] = bad;
        CHECK(check(false, a, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
        CHECK(check(false, {}, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
        CHECK(check(true, {}, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      }
    }
    CHECK(check(false, a, w, 1, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);             // bad ranges
    CHECK(check(false, a, w, -1, 1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(false, a, w, 0, -1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(false, a, w, B, 0, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);
    CHECK(check(false, a, w, 0, B, &copy, &nonzero, DDP_HIP_FLAG_STATE_LIMITS | DDP_HIP_FLAG_CONTROL_GRAV_COST) == DDP_HIP_E_UNSUPPORTED);   // the flag stands alone
    CHECK(check(false, a, w, -1, 1, &copy, &nonzero, 0) == DDP_HIP_E_UNSUPPORTED);          // ... and is checked first
  }

  // ---- row T carries no term: a non-zero weight there is refused, for every instance of the range and every row of v --------------
  {
    const std::vector<double> w = stage_weights();
    CHECK(check(false, {}, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    for (int64_t b : {(int64_t)0, B - 1})
      for (int row : {0, NV - 1}) {
        std::vector<double> wb = w;
        wb[(size_t)((b * T1 + T) * NV + row)] = 1e-300;
        CHECK(check(false, {}, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
        CHECK(check(true, {}, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
        if (b == B - 1) CHECK(check(false, {}, wb, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK && copy);   // (outside the range: not read)
      }
    std::vector<double> wt = w;                                          // row T-1 is a stage row
    wt[(size_t)((T - 1) * NV)] = 7.0;
    CHECK(check(false, {}, wt, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    std::vector<double> a((size_t)(B * T1 * NV), 3.0);                   // targets in row T are data without a term: accepted
    CHECK(check(false, a, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
  }

  // ---- a free-flyer root's six rows carry terms like any other: the rate of the body twist -----------------------------------------
  {
    std::vector<double> w((size_t)(B * T1 * NV), 0.0);
    for (int row : {0, 5}) w[(size_t)(NV + row)] = 1.5;                  // (instance 0, t = 1)
    CHECK(check(true, {}, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(false, {}, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(!cost_limit_weight_side([] { CostCheck c; c.items = NV; c.ff = true; return c; }(), w.data(), (int64_t)w.size()));   // (the limits' rule differs)
  }

  // ---- the live rule on half-batch uploads --------------------------------------------------------------------------------------
  {
    bool live = false;
    live = cost_live_rule(live, false, 0, B, B);                         // nothing but zeros: the kernels stay off
    CHECK(!live);
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
  printf("joint_accel_block: all checks passed\n");
  return 0;
}
