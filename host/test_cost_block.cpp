// The device-free parts of the add-on cost terms' upload path (ddp_pinocchio_amd/csrc/cost_block.h) on small host arrays: the
// validators, the range arithmetic, the non-zero scan and the live rule.  No HIP, no device: a plain host program.
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
static const uint32_t ALL = DDP_HIP_FLAG_FRAME_COST | DDP_HIP_FLAG_FRAME_ORIENT_COST | DDP_HIP_FLAG_STATE_LIMITS | DDP_HIP_FLAG_COM_COST |
                            DDP_HIP_FLAG_FRAME_VEL_COST | DDP_HIP_FLAG_OBSTACLE_COST;

static CostBlock block(int term, int32_t items) {
  CostBlock k;
  k.desc = &kCostDesc[term];
  k.max_items = items;
  k.items = items;
  return k;
}

// one upload's decisions for a term whose sides are all `count` instances long
static int check(int term, int32_t items, const CostCheck& c, const std::vector<std::vector<double>>& sides, const CostSideOk* ok,
                 int64_t first, int64_t count, bool* copy, bool* nonzero, uint32_t flags = ALL) {
  const CostBlock k = block(term, items);
  const double* host[COST_MAX_SIDES] = {nullptr, nullptr, nullptr};
  for (size_t s = 0; s < sides.size(); ++s) host[s] = sides[s].empty() ? nullptr : sides[s].data();
  return cost_upload_check(flags, k, c, B, T, host, ok, first, count, copy, nonzero);
}

int main() {
  const double nan = NAN, inf = INFINITY;
  bool copy, nonzero;
  CostCheck c;

  // ---- validators: target / weight sides -----------------------------------------------------------------------------------
  {
    c.items = 1;
    const CostSideOk ok[] = {cost_finite_side, cost_weight_side};
    const size_t words = (size_t)(B * (T + 1) * 3);
    std::vector<double> tg(words, 0.25), w(words, 0.0);
    CHECK(check(COST_COM, 1, c, {tg, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    w[words - 1] = 2.0;                                                  // the last double of the range is read
    CHECK(check(COST_COM, 1, c, {tg, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(COST_COM, 1, c, {{}, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(COST_COM, 1, c, {tg, {}}, ok, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    CHECK(check(COST_COM, 1, c, {{}, {}}, ok, 0, B, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);   // every side null
    std::vector<double> bad = tg;
    bad[words - 1] = nan;
    CHECK(check(COST_COM, 1, c, {bad, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
    bad[words - 1] = inf;
    CHECK(check(COST_COM, 1, c, {bad, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
    bad = w;
    bad[1] = -1e-300;                                                    // a negative weight
    CHECK(check(COST_COM, 1, c, {tg, bad}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
    bad[1] = nan;
    CHECK(check(COST_COM, 1, c, {tg, bad}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
    bad[1] = inf;
    CHECK(check(COST_COM, 1, c, {tg, bad}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
    // a bad value beyond the range is not read: one instance of the three
    bad = w;
    bad[(size_t)((T + 1) * 3)] = -1.0;
    CHECK(check(COST_COM, 1, c, {tg, bad}, ok, 0, 1, &copy, &nonzero) == DDP_HIP_OK && !nonzero);

    // ---- range arithmetic, count == 0, flag, layout ------------------------------------------------------------------------
    CHECK(check(COST_COM, 1, c, {tg, w}, ok, 1, B - 1, &copy, &nonzero) == DDP_HIP_OK && copy);    // first + count == batch
    CHECK(check(COST_COM, 1, c, {tg, w}, ok, 1, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);    // one beyond
    CHECK(check(COST_COM, 1, c, {tg, w}, ok, B, 1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(COST_COM, 1, c, {tg, w}, ok, -1, 1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(COST_COM, 1, c, {tg, w}, ok, 0, -1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(COST_COM, 1, c, {tg, w}, ok, B, 0, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);   // count == 0 at the end
    CHECK(check(COST_COM, 1, c, {bad, bad}, ok, 0, 0, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero); // ... reads nothing
    CHECK(check(COST_COM, 1, c, {tg, w}, ok, 0, B, &copy, &nonzero, ALL & ~DDP_HIP_FLAG_COM_COST) == DDP_HIP_E_UNSUPPORTED);
    CHECK(check(COST_COM, 1, c, {tg, w}, ok, -1, 1, &copy, &nonzero, 0) == DDP_HIP_E_UNSUPPORTED);  // the flag is checked first
    CHECK(check(COST_FRAME, 0, c, {{}, {}}, ok, 0, 0, &copy, &nonzero) == DDP_HIP_E_ARG);           // no frames set: no layout
    CHECK(check(COST_FRAME, 0, c, {{}, {}}, ok, 0, B + 1, &copy, &nonzero) == DDP_HIP_E_ARG);
    const CostBlock k = block(COST_FRAME_VEL, 2);
    CHECK(cost_side_words(k, 0, T) == (T + 1) * 2 * 6 && cost_side_words(k, 1, T) == (T + 1) * 2 * 6);
    CHECK(cost_range_check(ALL, k, B, 0, B) == DDP_HIP_OK && cost_range_check(ALL, k, B, 0, B + 1) == DDP_HIP_E_ARG);
  }

  // ---- unit quaternions to 1e-10 ----------------------------------------------------------------------------------------------
  {
    c.items = 2;
    const CostSideOk ok[] = {cost_quat_side, cost_weight_side};
    const size_t slots = (size_t)(B * (T + 1) * 2);
    std::vector<double> q(slots * 4, 0.0), w(slots * 3, 1.0);
    for (size_t i = 0; i < slots; ++i) q[4 * i + 3] = 1.0;
    CHECK(check(COST_ORIENT, 2, c, {q, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    std::vector<double> bad = q;
    bad[4 * (slots - 1) + 3] = 1.0 + 2e-10;
    CHECK(check(COST_ORIENT, 2, c, {bad, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
    bad[4 * (slots - 1) + 3] = 1.0 - 2e-10;
    CHECK(check(COST_ORIENT, 2, c, {bad, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
    bad[4 * (slots - 1) + 3] = 1.0 + 5e-11;
    CHECK(check(COST_ORIENT, 2, c, {bad, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_OK);
    bad[4 * (slots - 1) + 3] = 0.0;                                      // the zero quaternion
    CHECK(check(COST_ORIENT, 2, c, {bad, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
    bad = q;
    bad[0] = nan;
    CHECK(check(COST_ORIENT, 2, c, {bad, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
  }

  // ---- obstacle geometry by slot kind -----------------------------------------------------------------------------------------
  {
    const int32_t kind[2] = {DDP_HIP_OBSTACLE_SPHERE, DDP_HIP_OBSTACLE_HALFSPACE};
    c.items = 2;
    c.kind = kind;
    const CostSideOk ok[] = {cost_obstacle_geom_side, cost_weight_side};
    const size_t slots = (size_t)(B * (T + 1) * 2);
    std::vector<double> g(slots * 4, 0.0), w(slots, 0.0);
    for (size_t i = 0; i < slots; i += 2) {
      g[4 * i + 0] = 1.0; g[4 * i + 1] = -2.0; g[4 * i + 2] = 3.0; g[4 * i + 3] = 0.5;    // a sphere: centre, radius
      g[4 * i + 4] = 0.6; g[4 * i + 5] = 0.0; g[4 * i + 6] = 0.8; g[4 * i + 7] = -4.0;     // a half-space: unit normal, offset < 0
    }
    CHECK(check(COST_OBSTACLE, 2, c, {g, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    std::vector<double> bad = g;
    bad[4 * (slots - 2) + 3] = -1e-12;                                   // a sphere of negative radius
    CHECK(check(COST_OBSTACLE, 2, c, {bad, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
    bad = g;
    bad[4 * (slots - 1) + 0] = 0.6 + 1e-9;                               // a non-unit normal
    CHECK(check(COST_OBSTACLE, 2, c, {bad, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
    bad = g;
    bad[4 * (slots - 1) + 3] = inf;
    CHECK(check(COST_OBSTACLE, 2, c, {bad, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
    bad = g;
    bad[3] = 0.0;                                                        // radius 0 is a point: accepted
    CHECK(check(COST_OBSTACLE, 2, c, {bad, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_OK);
    c.kind = nullptr;
  }

  // ---- state limits: sides with their infinities, the free-flyer rule ---------------------------------------------------------
  {
    const int32_t n = 14;
    c.items = n;
    const CostSideOk ok[] = {cost_limit_lo_side, cost_limit_hi_side, cost_limit_weight_side};
    const size_t words = (size_t)(B * (T + 1) * n);
    std::vector<double> lo(words, -inf), hi(words, inf), w(words, 0.0);
    CHECK(check(COST_LIMITS, n, c, {lo, hi, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    std::vector<double> bad = lo;
    bad[words - 1] = inf;                                                // lo = +inf
    CHECK(check(COST_LIMITS, n, c, {bad, hi, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
    bad[words - 1] = nan;
    CHECK(check(COST_LIMITS, n, c, {bad, hi, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
    bad = hi;
    bad[0] = -inf;
    CHECK(check(COST_LIMITS, n, c, {lo, bad, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(COST_LIMITS, n, c, {hi, lo, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);
    w[(size_t)n + 5] = 1.0;                                              // a pose row of the second slot
    CHECK(check(COST_LIMITS, n, c, {lo, hi, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_OK && nonzero);
    c.ff = true;
    CHECK(check(COST_LIMITS, n, c, {lo, hi, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG);      // ... of a free flyer
    w[(size_t)n + 5] = 0.0;
    w[(size_t)n + 6] = 1.0;                                              // the first joint row
    CHECK(check(COST_LIMITS, n, c, {lo, hi, w}, ok, 0, B, &copy, &nonzero) == DDP_HIP_OK && nonzero);
    c.ff = false;
  }

  // ---- the non-zero scan --------------------------------------------------------------------------------------------------------
  {
    const double z[4] = {0.0, -0.0, 0.0, 0.0}, y[4] = {0.0, 0.0, 0.0, 1e-300};
    CHECK(!cost_any_nonzero(z, 4) && cost_any_nonzero(y, 4) && !cost_any_nonzero(y, 3) && !cost_any_nonzero(y, 0));
  }

  // ---- the live rule over (was live, non-zero seen, whole batch) ----------------------------------------------------------------
  for (int was = 0; was < 2; ++was)
    for (int nz = 0; nz < 2; ++nz)
      for (int whole = 0; whole < 2; ++whole) {
        const bool want = nz || (was && !whole);                         // on by a non-zero; off only by whole-batch zeros
        CHECK(cost_live_rule(was != 0, nz != 0, 0, whole ? B : B - 1, B) == want);
        if (!whole) CHECK(cost_live_rule(was != 0, nz != 0, 1, B - 1, B) == want);   // (first != 0 is not the whole batch)
      }

  if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
  printf("cost_block: all checks passed\n");
  return 0;
}
