// The device-free parts of the balance-region term (DDP_HIP_FLAG_BALANCE_REGION_COST; ddp_pinocchio_amd/csrc/cost_block.h): its
// record, its index among the terms (the neighbour relations of the other host programs still hold), the geometry validator
// (unit normal, tau >= 0, all finite), what an upload of one side alone decides, and the live rule.  No HIP, no device: a plain
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

static const int64_t B = 3, T = 2;
static const uint32_t ON = DDP_HIP_FLAG_BALANCE_REGION_COST;

static CostBlock block(int32_t items) {
  CostBlock k;
  k.desc = &kCostDesc[COST_BALANCE_REGION];
  k.max_items = k.desc->max_items;
  k.items = items;
  return k;
}

static int check(int32_t items, const std::vector<double>& geom, const std::vector<double>& weight, int64_t first, int64_t count, bool* copy,
                 bool* nonzero, uint32_t flags = ON) {
  const CostBlock k = block(items);
  CostCheck c;
  c.items = items;
  const double* host[COST_MAX_SIDES] = {geom.empty() ? nullptr : geom.data(), weight.empty() ? nullptr : weight.data(), nullptr};
  const CostSideOk ok[] = {cost_region_geom_side, cost_weight_side};
  return cost_upload_check(flags, k, c, B, T, host, ok, first, count, copy, nonzero);
}

int main() {
  const double nan = NAN, inf = INFINITY;
  bool copy, nonzero;

  // ---- the record: (n, h, tau) | weight per plane slot, a candidates' array, laid out by set_planes, T+1 rows --------------------
  {
    const CostDesc& d = kCostDesc[COST_BALANCE_REGION];
    CHECK(COST_BALANCE_REGION == COST_LIMITS + 1 && COST_BALANCE_REGION == COST_COM - 1);
    CHECK(d.flag == 32768u && DDP_HIP_MAX_REGION_PLANES == 8);
    CHECK(d.nside == 2);
    CHECK(d.unit[0] == 5 && d.unit[1] == 1 && d.unit[2] == 0);
    CHECK(d.fill[0] == FILL_ZERO && d.fill[1] == FILL_ZERO);
    CHECK(d.max_items == DDP_HIP_MAX_REGION_PLANES && !d.fixed && d.cand && !d.stage_only);
    const CostBlock k = block(6);
    CHECK(cost_rows(k, T) == T + 1);
    CHECK(cost_side_words(k, 0, T) == (T + 1) * 6 * 5 && cost_side_words(k, 1, T) == (T + 1) * 6);
    for (int t = 0; t < COST_COUNT; ++t)                                 // every row of the table is the row of its term: no flag twice
      for (int u = t + 1; u < COST_COUNT; ++u) CHECK(kCostDesc[t].flag != kCostDesc[u].flag);
    // the relations the other host programs pin, and every neighbour's row still its own
    CHECK(COST_FRAME_AIM == COST_COM + 1 && COST_FRAME_AIM == COST_FRAME_VEL - 1);
    CHECK(COST_CONTROL_GRAV == COST_FRAME_VEL + 1 && COST_CONTROL_GRAV == COST_MOMENTUM - 1);
    CHECK(COST_RELATIVE_FRAME == COST_MOMENTUM + 1 && COST_RELATIVE_FRAME == COST_OBSTACLE - 1);
    CHECK(COST_SELF_COLLISION == COST_COUNT - 1);
    CHECK(kCostDesc[COST_FRAME].flag == DDP_HIP_FLAG_FRAME_COST && kCostDesc[COST_ORIENT].flag == DDP_HIP_FLAG_FRAME_ORIENT_COST);
    CHECK(kCostDesc[COST_LIMITS].flag == DDP_HIP_FLAG_STATE_LIMITS && kCostDesc[COST_COM].flag == DDP_HIP_FLAG_COM_COST);
    CHECK(kCostDesc[COST_FRAME_AIM].flag == DDP_HIP_FLAG_FRAME_AIM_COST && kCostDesc[COST_FRAME_VEL].flag == DDP_HIP_FLAG_FRAME_VEL_COST);
    CHECK(kCostDesc[COST_CONTROL_GRAV].flag == DDP_HIP_FLAG_CONTROL_GRAV_COST && kCostDesc[COST_MOMENTUM].flag == DDP_HIP_FLAG_MOMENTUM_COST);
    CHECK(kCostDesc[COST_RELATIVE_FRAME].flag == DDP_HIP_FLAG_RELATIVE_FRAME_COST && kCostDesc[COST_OBSTACLE].flag == DDP_HIP_FLAG_OBSTACLE_COST);
    CHECK(kCostDesc[COST_SELF_COLLISION].flag == DDP_HIP_FLAG_SELF_COLLISION_COST);
    for (int t = 0; t < COST_COUNT; ++t) CHECK(kCostDesc[t].stage_only == (t == COST_CONTROL_GRAV));
  }

  // ---- the geometry validator ---------------------------------------------------------------------------------------------------
  {
    CostCheck c;
    const double ok2[10] = {0.6, 0.0, -0.8, -3.5, 0.0, 0.0, 1.0, 0.0, 2.0, 0.35};   // tau = 0 is a time constant; h of either sign
    CHECK(cost_region_geom_side(c, ok2, 10));
    CHECK(cost_region_geom_side(c, ok2, 0));                             // nothing to read
    for (int at = 0; at < 10; ++at)
      for (double bad : {nan, inf, -inf}) {                              // a non-finite entry anywhere: n, h or tau, first or last plane
        double g[10];
        for (int k = 0; k < 10; ++k) g[k] = ok2[k];
        g[at] = bad;
        CHECK(!cost_region_geom_side(c, g, 10));
        CHECK(cost_region_geom_side(c, g, 5) == (at >= 5));              // ... beyond the words is not read
      }
    for (double bad : {0.6 + 2e-10, 0.6 - 2e-10, 0.0, 1.0}) {            // |n| = 1 +- 1.2e-10, 0.8, 1.28: the half-spaces' rule
      double g[10];
      for (int k = 0; k < 10; ++k) g[k] = ok2[k];
      g[0] = bad;
      CHECK(!cost_region_geom_side(c, g, 10));
    }
    {
      double g[10];
      for (int k = 0; k < 10; ++k) g[k] = ok2[k];
      g[0] = 0.6 + 5e-11;                                                // within 1e-10 of the sphere: accepted
      CHECK(cost_region_geom_side(c, g, 10));
      g[0] = 0.0; g[2] = 0.0;                                            // the zero vector is no normal
      CHECK(!cost_region_geom_side(c, g, 10));
      for (int k = 0; k < 10; ++k) g[k] = ok2[k];
      g[6] = 2.0;                                                        // a normal that is not normalised is refused, not rescaled
      CHECK(!cost_region_geom_side(c, g, 10));
      g[6] = 1.0; g[9] = -1e-300;                                        // tau < 0, the last plane's
      CHECK(!cost_region_geom_side(c, g, 10));
      CHECK(cost_region_geom_side(c, g, 5));
      g[9] = 0.0; g[4] = -0.1;                                           // ... and the first plane's
      CHECK(!cost_region_geom_side(c, g, 10));
      g[4] = 1e-300;                                                     // any tau > 0
      CHECK(cost_region_geom_side(c, g, 10));
    }
  }

  // ---- an upload's decisions ----------------------------------------------------------------------------------------------------
  {
    const int32_t np = 4;
    const size_t slots = (size_t)(B * (T + 1) * np);
    std::vector<double> g(5 * slots, 0.0), w(slots, 0.0);
    for (size_t i = 0; i < slots; ++i) { g[5 * i + (i % 3)] = i % 2 ? -1.0 : 1.0; g[5 * i + 3] = -0.04; g[5 * i + 4] = i % 2 ? 0.3 : 0.0; }
    CHECK(check(np, g, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    w[slots - 1] = 1e-300;                                               // the last double of the range is read
    CHECK(check(np, g, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(np, {}, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);    // weights alone need no geometry check
    CHECK(check(np, g, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);   // geometry alone says nothing about liveness
    CHECK(check(np, {}, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);
    CHECK(check(np, g, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);   // the non-zero lies beyond the range
    for (double bad : {nan, inf, -inf})
      for (size_t at : {(size_t)0, 5 * slots - 2, 5 * slots - 1}) {      // a non-finite normal entry, offset, time constant
        std::vector<double> gb = g;
        gb[at] = bad;
        CHECK(check(np, gb, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
        CHECK(check(np, gb, {}, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
        if (at != 0) CHECK(check(np, gb, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK);   // ... beyond the range is not read
      }
    {
      std::vector<double> gb = g;
      gb[5 * slots - 1] = -0.3;                                          // tau < 0
      CHECK(check(np, gb, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(np, {}, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy);              // a null geom is not looked at
      gb = g;
      gb[0] = 1.0 + 1e-9;                                                // a normal off unit length
      CHECK(check(np, gb, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(np, gb, w, 1, B - 1, &copy, &nonzero) == DDP_HIP_E_ARG);               // (host arrays start at `first`)
    }
    for (double bad : {-1e-300, nan, inf, -inf}) {                       // a bad weight
      std::vector<double> wb = w;
      wb[0] = bad;
      CHECK(check(np, g, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(np, {}, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
    }
    CHECK(check(0, g, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);              // before set_planes with a plane: no layout
    CHECK(check(0, {}, {}, 0, 0, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(np, g, w, 1, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);             // bad ranges
    CHECK(check(np, g, w, -1, 1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(np, g, w, 0, -1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(np, g, w, B, 0, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);
    CHECK(check(np, g, w, 0, B, &copy, &nonzero, DDP_HIP_FLAG_COM_COST | DDP_HIP_FLAG_MOMENTUM_COST | DDP_HIP_FLAG_OBSTACLE_COST) ==
          DDP_HIP_E_UNSUPPORTED);                                                         // the flag stands alone
    CHECK(check(np, g, w, -1, 1, &copy, &nonzero, 0) == DDP_HIP_E_UNSUPPORTED);           // ... and is checked first
  }

  // ---- the live rule on half-batch uploads --------------------------------------------------------------------------------------
  {
    bool live = false;
    live = cost_live_rule(live, false, 0, B, B);                         // zeros on a block that was never live
    CHECK(!live);
    live = cost_live_rule(live, true, 1, 1, B);                          // one instance's non-zero weights switch the kernels on
    CHECK(live);
    live = cost_live_rule(live, false, 0, 2, B);                         // zeros range by range leave them launched
    CHECK(live);
    live = cost_live_rule(live, false, 0, B, B);                         // one upload of zeros for the whole batch switches them off
    CHECK(!live);
  }

  if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
  printf("balance_region_block: all checks passed\n");
  return 0;
}
