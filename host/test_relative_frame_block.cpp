// The device-free parts of the relative-frame term (DDP_HIP_FLAG_RELATIVE_FRAME_COST; ddp_pinocchio_amd/csrc/cost_block.h): its
// record, the pair-list rules, and what an upload of targets, reference quaternions and weights decides before it touches a
// device.  No HIP, no device: a plain host program.
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
static const uint32_t ON = DDP_HIP_FLAG_RELATIVE_FRAME_COST;

static CostBlock block(int32_t items) {
  CostBlock k;
  k.desc = &kCostDesc[COST_RELATIVE_FRAME];
  k.max_items = k.desc->max_items;
  k.items = items;
  return k;
}

static int check(int32_t items, const std::vector<double>& target, const std::vector<double>& quat, const std::vector<double>& weight,
                 int64_t first, int64_t count, bool* copy, bool* nonzero, uint32_t flags = ON) {
  const CostBlock k = block(items);
  CostCheck c;
  c.items = items;
  const double* host[COST_MAX_SIDES] = {target.empty() ? nullptr : target.data(), quat.empty() ? nullptr : quat.data(),
                                        weight.empty() ? nullptr : weight.data()};
  const CostSideOk ok[] = {cost_finite_side, cost_quat_side, cost_weight_side};
  return cost_upload_check(flags, k, c, B, T, host, ok, first, count, copy, nonzero);
}

int main() {
  const double nan = NAN, inf = INFINITY;
  bool copy, nonzero;

  // ---- the record: target | quat | weight per pair, a candidates' array, laid out by set_pairs, between momentum and obstacles ---
  {
    const CostDesc& d = kCostDesc[COST_RELATIVE_FRAME];
    CHECK(COST_RELATIVE_FRAME == COST_MOMENTUM + 1 && COST_RELATIVE_FRAME == COST_OBSTACLE - 1);
    CHECK(d.flag == 4096u && DDP_HIP_MAX_FRAME_PAIRS == 4);
    CHECK(d.nside == 3 && COST_MAX_SIDES == 3);
    CHECK(d.unit[0] == 3 && d.unit[1] == 4 && d.unit[2] == 6);
    CHECK(d.fill[0] == FILL_ZERO && d.fill[1] == FILL_QUAT && d.fill[2] == FILL_ZERO);
    CHECK(d.max_items == DDP_HIP_MAX_FRAME_PAIRS && !d.fixed && d.cand);
    const CostBlock k = block(3);
    CHECK(cost_side_words(k, 0, T) == (T + 1) * 3 * 3 && cost_side_words(k, 1, T) == (T + 1) * 3 * 4 && cost_side_words(k, 2, T) == (T + 1) * 3 * 6);
    for (int t = 0; t < COST_COUNT; ++t)                                 // every row of the table is the row of its term: no flag twice
      for (int u = t + 1; u < COST_COUNT; ++u) CHECK(kCostDesc[t].flag != kCostDesc[u].flag);
  }

  // ---- the pair-list rules ------------------------------------------------------------------------------------------------------
  {
    const int32_t nj = 6;
    const int32_t ja[3] = {0, 2, 5}, jb[3] = {5, 3, 2};
    const double off[9] = {0.0, 0.1, -0.2, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0};
    CHECK(cost_frame_pairs_ok(nj, 3, ja, off, jb, off));
    CHECK(cost_frame_pairs_ok(nj, 0, ja, off, jb, off));                 // (the count's range is the caller's)
    const int32_t dup_a[2] = {1, 1}, dup_b[2] = {4, 4};
    CHECK(cost_frame_pairs_ok(nj, 2, dup_a, off, dup_b, off));           // duplicates are allowed
    const int32_t rev_a[2] = {1, 4}, rev_b[2] = {4, 1};
    CHECK(cost_frame_pairs_ok(nj, 2, rev_a, off, rev_b, off));           // ... and so is a pair with its roles swapped
    const int32_t same_a[1] = {3}, same_b[1] = {3};
    CHECK(!cost_frame_pairs_ok(nj, 1, same_a, off, same_b, off));        // both frames on one joint: a constant placement
    const int32_t hi_a[1] = {0}, hi_b[1] = {6};
    CHECK(!cost_frame_pairs_ok(nj, 1, hi_a, off, hi_b, off));            // a joint one past the model
    CHECK(!cost_frame_pairs_ok(nj, 1, hi_b, off, hi_a, off));
    CHECK(cost_frame_pairs_ok(7, 1, hi_a, off, hi_b, off));
    const int32_t neg_a[1] = {-1}, neg_b[1] = {0};
    CHECK(!cost_frame_pairs_ok(nj, 1, neg_a, off, neg_b, off));
    CHECK(!cost_frame_pairs_ok(nj, 1, neg_b, off, neg_a, off));
    const int32_t late_a[3] = {0, 2, 5}, late_b[3] = {5, 3, 5};          // the last pair of the list is read
    CHECK(!cost_frame_pairs_ok(nj, 3, late_a, off, late_b, off));
    CHECK(cost_frame_pairs_ok(nj, 2, late_a, off, late_b, off));         // ... and nothing beyond the count
    for (double bad : {nan, inf, -inf})
      for (int at : {0, 8}) {                                            // a non-finite offset, on either side, first or last double
        double ob[9];
        for (int k = 0; k < 9; ++k) ob[k] = off[k];
        ob[at] = bad;
        CHECK(!cost_frame_pairs_ok(nj, 3, ja, ob, jb, off));
        CHECK(!cost_frame_pairs_ok(nj, 3, ja, off, jb, ob));
        CHECK(cost_frame_pairs_ok(nj, 2, ja, off, jb, ob) == (at != 0)); // ... beyond the count is not read
      }
  }

  // ---- an upload's decisions ----------------------------------------------------------------------------------------------------
  {
    const int32_t np = 3;
    const size_t slots = (size_t)(B * (T + 1) * np);
    std::vector<double> g(3 * slots, -0.25), q(4 * slots, 0.0), w(6 * slots, 0.0);
    for (size_t i = 0; i < slots; ++i) { q[4 * i] = 0.6; q[4 * i + 3] = -0.8; }   // unit, w < 0: -ref is the same reference
    CHECK(check(np, g, q, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    w[6 * slots - 1] = 1e-300;                                           // the last double of the range is read
    CHECK(check(np, g, q, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(np, {}, {}, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(np, g, {}, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    CHECK(check(np, {}, q, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    CHECK(check(np, {}, {}, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);
    CHECK(check(np, g, q, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);   // the non-zero lies beyond the range
    for (double bad : {nan, inf, -inf}) {                                // a bad target
      std::vector<double> gb = g;
      gb[3 * slots - 1] = bad;
      CHECK(check(np, gb, q, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(np, gb, {}, {}, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(np, gb, q, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK);   // ... beyond the range is not read
    }
    for (double bad : {0.6 + 2e-10, 0.6 - 2e-10, 0.0, nan, inf}) {       // a quaternion off the unit sphere (|.| = 1 +- 1.2e-10), or not finite
      std::vector<double> qb = q;
      qb[4 * (slots - 1)] = bad;
      CHECK(check(np, g, qb, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(np, {}, qb, {}, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(np, g, qb, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK);
    }
    {
      std::vector<double> qz = q;                                        // the zero quaternion has no rotation
      qz[0] = qz[3] = 0.0;
      CHECK(check(np, {}, qz, {}, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      std::vector<double> qn = q;                                        // within 1e-10 of the sphere: accepted
      qn[0] = 0.6 + 5e-11;
      CHECK(check(np, {}, qn, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy);
    }
    for (double bad : {-1e-300, nan, inf, -inf}) {                       // a bad weight
      std::vector<double> wb = w;
      wb[1] = bad;
      CHECK(check(np, g, q, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(np, {}, {}, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(np, g, q, wb, 1, B - 1, &copy, &nonzero) == DDP_HIP_E_ARG);   // (host arrays start at `first`)
    }
    CHECK(check(0, g, q, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);            // before set_pairs: no layout
    CHECK(check(0, {}, {}, {}, 0, 0, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(np, g, q, w, 1, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);           // bad ranges
    CHECK(check(np, g, q, w, -1, 1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(np, g, q, w, 0, -1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(np, g, q, w, B, 0, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);
    CHECK(check(np, g, q, w, 0, B, &copy, &nonzero, DDP_HIP_FLAG_FRAME_COST | DDP_HIP_FLAG_FRAME_ORIENT_COST) == DDP_HIP_E_UNSUPPORTED);   // the flag stands alone
    CHECK(check(np, g, q, w, -1, 1, &copy, &nonzero, 0) == DDP_HIP_E_UNSUPPORTED);        // ... and is checked first
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
  printf("relative_frame_block: all checks passed\n");
  return 0;
}
