// The device-free parts of the self-collision term (DDP_HIP_FLAG_SELF_COLLISION_COST; ddp_pinocchio_amd/csrc/cost_block.h): its
// record, the pair-list rules, and what an upload of margins and weights decides before it touches a device.  No HIP, no device:
// a plain host program.
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
static const uint32_t ON = DDP_HIP_FLAG_SELF_COLLISION_COST;

static CostBlock block(int32_t items) {
  CostBlock k;
  k.desc = &kCostDesc[COST_SELF_COLLISION];
  k.max_items = k.desc->max_items;
  k.items = items;
  return k;
}

static int check(int32_t items, const std::vector<double>& margin, const std::vector<double>& weight, int64_t first, int64_t count, bool* copy,
                 bool* nonzero, uint32_t flags = ON) {
  const CostBlock k = block(items);
  CostCheck c;
  c.items = items;
  const double* host[COST_MAX_SIDES] = {margin.empty() ? nullptr : margin.data(), weight.empty() ? nullptr : weight.data(), nullptr};
  const CostSideOk ok[] = {cost_finite_side, cost_weight_side};
  return cost_upload_check(flags, k, c, B, T, host, ok, first, count, copy, nonzero);
}

int main() {
  const double nan = NAN, inf = INFINITY;
  bool copy, nonzero;

  // ---- the record: margin | weight per pair, a candidates' array, laid out by set_pairs, last in the order of additions ------
  {
    const CostDesc& d = kCostDesc[COST_SELF_COLLISION];
    CHECK(COST_SELF_COLLISION == COST_OBSTACLE + 1 && COST_SELF_COLLISION == COST_COUNT - 1);
    CHECK(d.flag == 1024u && DDP_HIP_MAX_COLLISION_PAIRS == 32);
    CHECK(d.nside == 2 && d.unit[0] == 1 && d.unit[1] == 1 && d.fill[0] == FILL_ZERO && d.fill[1] == FILL_ZERO);
    CHECK(d.max_items == DDP_HIP_MAX_COLLISION_PAIRS && !d.fixed && d.cand);
    const CostBlock k = block(5);
    CHECK(cost_side_words(k, 0, T) == (T + 1) * 5 && cost_side_words(k, 1, T) == (T + 1) * 5);
  }

  // ---- the pair-list rules ------------------------------------------------------------------------------------------------------
  {
    const int32_t joint[4] = {0, 3, 3, 5};                               // spheres 1 and 2 sit on one joint
    const int32_t a[3] = {0, 0, 1}, b[3] = {1, 3, 3};
    CHECK(cost_pair_list_ok(4, joint, 3, a, b));
    CHECK(cost_pair_list_ok(4, joint, 0, a, b));                         // (the count's range is the caller's)
    const int32_t dup_a[2] = {0, 0}, dup_b[2] = {3, 3};
    CHECK(cost_pair_list_ok(4, joint, 2, dup_a, dup_b));                 // duplicates are allowed
    const int32_t rev_a[2] = {0, 3}, rev_b[2] = {3, 0};
    CHECK(cost_pair_list_ok(4, joint, 2, rev_a, rev_b));                 // ... and so is a pair in both orders
    const int32_t same_a[1] = {2}, same_b[1] = {2};
    CHECK(!cost_pair_list_ok(4, joint, 1, same_a, same_b));              // a == b
    const int32_t j_a[1] = {1}, j_b[1] = {2};
    CHECK(!cost_pair_list_ok(4, joint, 1, j_a, j_b));                    // both spheres on joint 3
    CHECK(!cost_pair_list_ok(4, joint, 1, j_b, j_a));
    const int32_t hi_a[1] = {0}, hi_b[1] = {4};
    CHECK(!cost_pair_list_ok(4, joint, 1, hi_a, hi_b));                  // an index one past the points
    CHECK(!cost_pair_list_ok(4, joint, 1, hi_b, hi_a));
    const int32_t neg_a[1] = {-1}, neg_b[1] = {0};
    CHECK(!cost_pair_list_ok(4, joint, 1, neg_a, neg_b));
    CHECK(!cost_pair_list_ok(4, joint, 1, neg_b, neg_a));
    const int32_t late_a[3] = {0, 0, 1}, late_b[3] = {1, 3, 2};          // the last pair of the list is read
    CHECK(!cost_pair_list_ok(4, joint, 3, late_a, late_b));
    CHECK(cost_pair_list_ok(4, joint, 2, late_a, late_b));               // ... and nothing beyond the count
    CHECK(cost_pair_list_ok(3, joint, 1, a, b) && !cost_pair_list_ok(3, joint, 2, a, b));   // sphere 3 is outside 3 points
  }

  // ---- an upload's decisions ----------------------------------------------------------------------------------------------------
  {
    const int32_t np = 5;
    const size_t words = (size_t)(B * (T + 1) * np);
    std::vector<double> m(words, -0.25), w(words, 0.0);                   // a negative margin is a margin
    CHECK(check(np, m, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    w[words - 1] = 1e-300;                                               // the last double of the range is read
    CHECK(check(np, m, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(np, {}, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(np, m, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    CHECK(check(np, {}, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);
    CHECK(check(np, m, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);   // the non-zero lies beyond the range
    for (double bad : {nan, inf, -inf}) {                                // a bad margin
      std::vector<double> mb = m;
      mb[words - 1] = bad;
      CHECK(check(np, mb, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(np, mb, {}, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(np, mb, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK);  // ... beyond the range is not read
    }
    for (double bad : {-1e-300, nan, inf, -inf}) {                       // a bad weight
      std::vector<double> wb = w;
      wb[1] = bad;
      CHECK(check(np, m, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(np, {}, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(np, m, wb, 1, B - 1, &copy, &nonzero) == DDP_HIP_E_ARG);   // (host arrays start at `first`)
    }
    CHECK(check(0, m, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);              // before set_pairs: no layout
    CHECK(check(0, {}, {}, 0, 0, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(np, m, w, 1, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);             // bad ranges
    CHECK(check(np, m, w, -1, 1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(np, m, w, 0, -1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(np, m, w, B, 0, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);
    CHECK(check(np, m, w, 0, B, &copy, &nonzero, DDP_HIP_FLAG_OBSTACLE_COST) == DDP_HIP_E_UNSUPPORTED);   // the flag stands alone
    CHECK(check(np, m, w, -1, 1, &copy, &nonzero, 0) == DDP_HIP_E_UNSUPPORTED);          // ... and is checked first
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
  printf("self_collision_block: all checks passed\n");
  return 0;
}
