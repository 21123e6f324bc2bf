// The device-free parts of the capsule term (DDP_HIP_FLAG_CAPSULE_COST; ddp_pinocchio_amd/csrc/cost_block.h, capsule_cost.h): its
// record and index, the geometry validator by pair kind, the pair-list rules, what an upload decides before it touches a device,
// and the closest-point routine against a brute-force scan over a 201 x 201 grid of (s, t).  No HIP, no device: a plain host program.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "../ddp_pinocchio_amd/csrc/capsule_cost.h"
#include "../ddp_pinocchio_amd/csrc/cost_block.h"

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
  } while (0)

static const int64_t B = 3, T = 2;
static const uint32_t ON = DDP_HIP_FLAG_CAPSULE_COST;
static const int32_t KINDS[4] = {DDP_HIP_CAPSULE_VS_ROBOT, DDP_HIP_CAPSULE_VS_CAPSULE, DDP_HIP_CAPSULE_VS_HALFSPACE, DDP_HIP_CAPSULE_VS_CAPSULE};

static CostBlock block(int32_t items) {
  CostBlock k;
  k.desc = &kCostDesc[COST_CAPSULE];
  k.max_items = k.desc->max_items;
  k.items = items;
  return k;
}

static int check(int32_t items, const std::vector<double>& geom, const std::vector<double>& weight, int64_t first, int64_t count, bool* copy,
                 bool* nonzero, uint32_t flags = ON) {
  const CostBlock k = block(items);
  CostCheck c;
  c.items = items;
  c.kind = KINDS;
  const double* host[COST_MAX_SIDES] = {geom.empty() ? nullptr : geom.data(), weight.empty() ? nullptr : weight.data(), nullptr};
  const CostSideOk ok[] = {cost_capsule_geom_side, cost_weight_side};
  return cost_upload_check(flags, k, c, B, T, host, ok, first, count, copy, nonzero);
}

// a valid geometry for the four kinds of KINDS, every (instance, t)
static std::vector<double> good_geom() {
  std::vector<double> g((size_t)(B * (T + 1) * 4 * 8), 0.0);
  for (int64_t r = 0; r < B * (T + 1); ++r) {
    double* p = g.data() + r * 32;
    p[7] = -0.25;                                                        // robot: a negative margin is a margin
    p[8] = 1.0; p[11] = 2.0; p[14] = 0.0; p[15] = 0.1;                   // world capsule, rho = 0
    p[16] = 0.6; p[17] = 0.0; p[18] = 0.8; p[19] = -3.0; p[23] = 0.02;   // half-space, |n| = 1
    p[24] = 1.0; p[27] = 1.0; p[30] = 0.5; p[31] = 0.0;                  // a world sphere (b0 == b1)
  }
  return g;
}

// ---- the closest-point routine ---------------------------------------------------------------------------------------------------
static double dist2(const double* a0, const double* a1, const double* b0, const double* b1, double s, double t) {
  double d2 = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double x = a0[k] + s * (a1[k] - a0[k]) - b0[k] - t * (b1[k] - b0[k]);
    d2 += x * x;
  }
  return d2;
}

// the routine's distance is no larger than any point of the 201 x 201 grid (up to rounding), and no smaller than the grid's best
// by more than the grid can miss: the distance is 1-Lipschitz in each point, which moves at most half a cell, len / 400, per segment
static void check_against_scan(const double* a0, const double* a1, const double* b0, const double* b1) {
  double s, t, ca[3], cb[3];
  capsule_closest_params(a0, a1, b0, b1, &s, &t);
  CHECK(s >= 0.0 && s <= 1.0 && t >= 0.0 && t <= 1.0);
  const double D = capsule_closest_points(a0, a1, b0, b1, ca, cb);
  CHECK(fabs(D - sqrt(dist2(a0, a1, b0, b1, s, t))) <= 1e-14 * (1.0 + D));
  double best = INFINITY;
  for (int i = 0; i <= 200; ++i)
    for (int j = 0; j <= 200; ++j) {
      const double d2 = dist2(a0, a1, b0, b1, i / 200.0, j / 200.0);
      if (d2 < best) best = d2;
    }
  best = sqrt(best);
  const double la = sqrt(dist2(a0, a0, a1, a1, 0.0, 0.0)), lb = sqrt(dist2(b0, b0, b1, b1, 0.0, 0.0));
  CHECK(D <= best + 1e-12 * (1.0 + best));
  CHECK(D >= best - (la + lb) / 400.0 - 1e-12);
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static double rnd() {                                                    // uniform in [-1, 1)
  g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_rng >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

static void check_params(const double* a0, const double* a1, const double* b0, const double* b1, double s_want, double t_want) {
  double s, t;
  capsule_closest_params(a0, a1, b0, b1, &s, &t);
  CHECK(s == s_want && t == t_want);
  check_against_scan(a0, a1, b0, b1);
}

int main() {
  const double nan = NAN, inf = INFINITY;
  bool copy, nonzero;

  // ---- the record: geom (8) | weight per pair, a candidates' array, laid out by set_pairs; its index between the frame
  // ---- positions' and the frame orientations', every adjacency behind it as the sibling programs hold them ------------------------
  {
    const CostDesc& d = kCostDesc[COST_CAPSULE];
    CHECK(COST_FRAME == 0 && COST_CAPSULE == COST_FRAME + 1 && COST_ORIENT == COST_CAPSULE + 1);
    CHECK(COST_JOINT_ACCEL == COST_ORIENT + 1 && COST_SELF_COLLISION == COST_COUNT - 1);
    CHECK(d.flag == 131072u && DDP_HIP_MAX_CAPSULES == 16 && DDP_HIP_MAX_CAPSULE_PAIRS == 32);
    CHECK(DDP_HIP_CAPSULE_VS_ROBOT == 0 && DDP_HIP_CAPSULE_VS_CAPSULE == 1 && DDP_HIP_CAPSULE_VS_HALFSPACE == 2);
    CHECK(d.nside == 2 && d.unit[0] == 8 && d.unit[1] == 1 && d.fill[0] == FILL_ZERO && d.fill[1] == FILL_ZERO);
    CHECK(d.max_items == DDP_HIP_MAX_CAPSULE_PAIRS && !d.fixed && d.cand && !d.stage_only);
    const CostBlock k = block(5);
    CHECK(cost_rows(k, T) == T + 1);
    CHECK(cost_side_words(k, 0, T) == (T + 1) * 5 * 8 && cost_side_words(k, 1, T) == (T + 1) * 5);
    for (int t = 0; t < COST_COUNT; ++t)                                 // every row of the table is the row of its term: no flag twice
      for (int u = t + 1; u < COST_COUNT; ++u) CHECK(kCostDesc[t].flag != kCostDesc[u].flag);
    CHECK(kCostDesc[COST_FRAME].flag == DDP_HIP_FLAG_FRAME_COST && kCostDesc[COST_ORIENT].flag == DDP_HIP_FLAG_FRAME_ORIENT_COST);
  }

  // ---- the pair-list rules ------------------------------------------------------------------------------------------------------
  {
    const int32_t joint[4] = {0, 3, 3, 5};                               // capsules 1 and 2 sit on one joint
    const int32_t R = DDP_HIP_CAPSULE_VS_ROBOT, W = DDP_HIP_CAPSULE_VS_CAPSULE, H = DDP_HIP_CAPSULE_VS_HALFSPACE;
    const int32_t a[4] = {0, 0, 1, 2}, kind[4] = {R, R, W, H}, b[4] = {1, 3, 99, -7};   // a world pair's b is not read
    CHECK(cost_capsule_pairs_ok(4, joint, 4, a, kind, b));
    CHECK(cost_capsule_pairs_ok(4, joint, 0, a, kind, b));               // (the count's range is the caller's)
    const int32_t dup_a[2] = {0, 0}, dup_k[2] = {R, R}, dup_b[2] = {3, 3};
    CHECK(cost_capsule_pairs_ok(4, joint, 2, dup_a, dup_k, dup_b));      // duplicates are allowed
    const int32_t one_a[1] = {2}, one_b[1] = {2}, rk[1] = {R}, wk[1] = {W}, hk[1] = {H};
    CHECK(!cost_capsule_pairs_ok(4, joint, 1, one_a, rk, one_b));        // a == b
    CHECK(cost_capsule_pairs_ok(4, joint, 1, one_a, wk, one_b) && cost_capsule_pairs_ok(4, joint, 1, one_a, hk, one_b));
    const int32_t j_a[1] = {1}, j_b[1] = {2};
    CHECK(!cost_capsule_pairs_ok(4, joint, 1, j_a, rk, j_b));            // both capsules on joint 3
    CHECK(!cost_capsule_pairs_ok(4, joint, 1, j_b, rk, j_a));
    const int32_t hi_a[1] = {0}, hi_b[1] = {4};
    CHECK(!cost_capsule_pairs_ok(4, joint, 1, hi_a, rk, hi_b));          // an index one past the capsules
    CHECK(!cost_capsule_pairs_ok(4, joint, 1, hi_b, rk, hi_a));
    CHECK(!cost_capsule_pairs_ok(4, joint, 1, hi_b, wk, hi_a));          // body A of a world pair is checked too
    CHECK(!cost_capsule_pairs_ok(4, joint, 1, hi_b, hk, hi_a));
    const int32_t neg_a[1] = {-1}, neg_b[1] = {0};
    CHECK(!cost_capsule_pairs_ok(4, joint, 1, neg_a, rk, neg_b) && !cost_capsule_pairs_ok(4, joint, 1, neg_b, rk, neg_a));
    CHECK(!cost_capsule_pairs_ok(4, joint, 1, neg_a, hk, neg_b));
    for (int32_t bad : {-1, 3, 1000}) {                                  // an unknown kind
      const int32_t bk[1] = {bad};
      CHECK(!cost_capsule_pairs_ok(4, joint, 1, hi_a, bk, neg_b));
    }
    const int32_t late_k[4] = {R, R, W, 3};                              // the last pair of the list is read
    CHECK(!cost_capsule_pairs_ok(4, joint, 4, a, late_k, b));
    CHECK(cost_capsule_pairs_ok(4, joint, 3, a, late_k, b));             // ... and nothing beyond the count
  }

  // ---- the geometry validator, by kind ------------------------------------------------------------------------------------------
  {
    const std::vector<double> g = good_geom();
    CostCheck c;
    c.items = 4;
    c.kind = KINDS;
    CHECK(cost_capsule_geom_side(c, g.data(), (int64_t)g.size()));
    const size_t last = g.size() - 32;                                   // the last (instance, t) of the range is read
    for (int pair = 0; pair < 4; ++pair)
      for (int a = 0; a < 8; ++a)
        for (double bad : {nan, inf, -inf}) {                            // every entry finite, the ignored ones included
          std::vector<double> gb = g;
          gb[last + 8 * pair + a] = bad;
          CHECK(!cost_capsule_geom_side(c, gb.data(), (int64_t)gb.size()));
          CHECK(cost_capsule_geom_side(c, gb.data(), (int64_t)last));    // ... beyond the range is not read
        }
    std::vector<double> gb = g;
    gb[last + 8 + 6] = -1e-300;                                          // a world capsule's rho < 0
    CHECK(!cost_capsule_geom_side(c, gb.data(), (int64_t)gb.size()));
    gb = g;
    gb[last + 6] = -1.0;                                                 // ... is a robot pair's ignored entry,
    gb[last + 16 + 6] = -1.0;                                            // ... and a half-space's
    gb[last + 7] = gb[last + 15] = gb[last + 23] = -5.0;                 // and a margin may be negative
    CHECK(cost_capsule_geom_side(c, gb.data(), (int64_t)gb.size()));
    gb = g;
    gb[last + 16] = 0.6 + 2e-10;                                         // a half-space's normal off unit length
    CHECK(!cost_capsule_geom_side(c, gb.data(), (int64_t)gb.size()));
    gb[last + 16] = 0.6 + 1e-11;
    CHECK(cost_capsule_geom_side(c, gb.data(), (int64_t)gb.size()));
    gb = g;
    gb[last + 16] = gb[last + 18] = 0.0;                                 // the zero normal
    CHECK(!cost_capsule_geom_side(c, gb.data(), (int64_t)gb.size()));
    gb = g;
    gb[last + 8] = gb[last + 9] = gb[last + 10] = 0.0;                   // a world capsule's first three need not be unit
    CHECK(cost_capsule_geom_side(c, gb.data(), (int64_t)gb.size()));
  }

  // ---- an upload's decisions ----------------------------------------------------------------------------------------------------
  {
    const int32_t np = 4;
    const size_t words = (size_t)(B * (T + 1) * np);
    const std::vector<double> g = good_geom();
    std::vector<double> w(words, 0.0);
    CHECK(check(np, g, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    w[words - 1] = 1e-300;                                               // the last double of the range is read
    CHECK(check(np, g, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(np, {}, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(np, g, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    CHECK(check(np, {}, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);
    CHECK(check(np, g, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);   // the non-zero lies beyond the range
    std::vector<double> gb = g;
    gb[g.size() - 32 + 8 + 6] = -0.5;                                    // a bad geometry: rho < 0 in the last instance
    CHECK(check(np, gb, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
    CHECK(check(np, gb, {}, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
    CHECK(check(np, gb, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK);    // ... beyond the range is not read
    for (double bad : {-1e-300, nan, inf, -inf}) {                       // a bad weight
      std::vector<double> wb = w;
      wb[1] = bad;
      CHECK(check(np, g, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(np, {}, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
    }
    CHECK(check(0, g, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);               // before set_pairs: no layout
    CHECK(check(0, {}, {}, 0, 0, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(np, g, w, 1, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);              // bad ranges
    CHECK(check(np, g, w, -1, 1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(np, g, w, 0, -1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(np, g, w, B, 0, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);
    CHECK(check(np, g, w, 0, B, &copy, &nonzero, DDP_HIP_FLAG_OBSTACLE_COST | DDP_HIP_FLAG_SELF_COLLISION_COST) == DDP_HIP_E_UNSUPPORTED);   // the flag stands alone
    CHECK(check(np, g, w, -1, 1, &copy, &nonzero, 0) == DDP_HIP_E_UNSUPPORTED);           // ... and is checked first
  }

  // ---- the closest points: the pinned branches, each against the scan ---------------------------------------------------------------
  {
    const double o[3] = {0, 0, 0}, x1[3] = {1, 0, 0}, x2[3] = {2, 0, 0}, x3[3] = {3, 0, 0};
    const double p[3] = {0.25, 1, 0}, pl[3] = {-1, 1, 0}, pr[3] = {4, -2, 1};
    check_params(o, o, p, p, 0.0, 0.0);                                  // point - point
    check_params(o, o, o, o, 0.0, 0.0);                                  // ... and the same point: D == 0
    check_params(p, p, o, x1, 0.0, 0.25);                                // point - segment (A == 0): t = clamp(F / E)
    check_params(pl, pl, o, x1, 0.0, 0.0);
    check_params(pr, pr, o, x1, 0.0, 1.0);
    check_params(o, x1, p, p, 0.25, 0.0);                                // segment - point (E == 0): s = clamp(-C / A)
    check_params(o, x1, pl, pl, 0.0, 0.0);
    check_params(o, x1, pr, pr, 1.0, 0.0);
    const double y0[3] = {0, 1, 0}, y1[3] = {1, 1, 0}, y2[3] = {2, 1, 0}, y3[3] = {3, 1, 0}, ym[3] = {-2, 1, 0}, yn[3] = {-1, 1, 0};
    check_params(o, x1, y0, y1, 0.0, 0.0);                               // parallel, overlapping: den == 0 starts from s = 0
    check_params(o, x2, y1, y3, 0.5, 0.0);                               // parallel: t = (Bv 0 + F) / E < 0 -> t = 0, s = clamp(-C / A)
    check_params(o, x1, y2, y3, 1.0, 0.0);                               // parallel, B beyond A's end1
    check_params(o, x1, ym, yn, 0.0, 1.0);                               // parallel, B before A's end0: t > 1 -> t = 1, s = clamp((Bv - C) / A)
    check_params(o, x1, y1, y0, 0.0, 1.0);                               // anti-parallel
    const double c0[3] = {0.5, -1, 0}, c1[3] = {0.5, 1, 0};
    check_params(o, x1, c0, c1, 0.5, 0.5);                               // crossing: D == 0 in the interior
    const double u0[3] = {0.5, -1, 1}, u1[3] = {0.5, 1, 1};
    check_params(o, x1, u0, u1, 0.5, 0.5);                               // skew: the common perpendicular
    check_params(o, x1, x1, x2, 1.0, 0.0);                               // end to end, collinear
    check_params(o, x1, x2, x3, 1.0, 0.0);                               // collinear with a gap
    const double e0[3] = {1, 0, 0}, e1[3] = {1, 2, 0};
    check_params(o, x1, e0, e1, 1.0, 0.0);                               // end to end at a right angle
    const double t0[3] = {0.5, 1, 0}, t1[3] = {0.5, 3, 0};
    check_params(o, x1, t0, t1, 0.5, 0.0);                               // T-shaped: t clamps to 0, s recomputed
    const double v0[3] = {0.5, -3, 0}, v1[3] = {0.5, -1, 0};
    check_params(o, x1, v0, v1, 0.5, 1.0);                               // ... and to 1
    const double k0[3] = {-1, 0, 1}, k1[3] = {2, 0, 1};
    check_params(o, x1, k0, k1, 0.0, 1.0 / 3.0);                         // a tie along the overlap: s = 0 wins

    for (int trial = 0; trial < 300; ++trial) {                          // random segments, every few with a degenerate side
      double a0[3], a1[3], b0[3], b1[3];
      for (int k = 0; k < 3; ++k) { a0[k] = rnd(); a1[k] = rnd(); b0[k] = rnd(); b1[k] = rnd(); }
      if (trial % 7 == 3) for (int k = 0; k < 3; ++k) a1[k] = a0[k];
      if (trial % 11 == 5) for (int k = 0; k < 3; ++k) b1[k] = b0[k];
      if (trial % 13 == 6) for (int k = 0; k < 3; ++k) b1[k] = b0[k] + 0.7 * (a1[k] - a0[k]);   // parallel up to rounding
      check_against_scan(a0, a1, b0, b1);
    }
  }

  // ---- the half-space: the lower end, end0 on a tie ---------------------------------------------------------------------------------
  {
    const double n[3] = {0, 0, 1}, lo[3] = {1, 2, 0.5}, hi[3] = {3, 4, 2.0}, tie[3] = {7, 8, 0.5};
    double ca[3];
    CHECK(capsule_halfspace_point(lo, hi, n, 0.25, ca) == 0.25 && ca[0] == 1 && ca[1] == 2 && ca[2] == 0.5);
    CHECK(capsule_halfspace_point(hi, lo, n, 0.25, ca) == 0.25 && ca[0] == 1 && ca[1] == 2 && ca[2] == 0.5);
    CHECK(capsule_halfspace_point(lo, tie, n, 1.0, ca) == -0.5 && ca[0] == 1 && ca[1] == 2);   // end0 wins
    CHECK(capsule_halfspace_point(tie, lo, n, 1.0, ca) == -0.5 && ca[0] == 7 && ca[1] == 8);
    CHECK(capsule_halfspace_point(lo, lo, n, 0.0, ca) == 0.5 && ca[0] == 1);                    // a sphere
  }

  // ---- the live rule on half-batch uploads --------------------------------------------------------------------------------------
  {
    bool live = false;
    live = cost_live_rule(live, true, 1, 1, B);
    CHECK(live);
    live = cost_live_rule(live, false, 0, 2, B);
    CHECK(live);
    live = cost_live_rule(live, false, 0, B, B);
    CHECK(!live);
  }

  if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
  printf("capsule_block: all checks passed\n");
  return 0;
}
