// The device-free parts of the frame-aiming term (DDP_HIP_FLAG_FRAME_AIM_COST; ddp_pinocchio_amd/csrc/cost_block.h): its record,
// its index among the terms, the frame-list rules (joints, offsets, the unit axis), and what an upload of targets with their
// stand-offs and of weights decides before it touches a device.  No HIP, no device: a plain host program.
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
static const uint32_t ON = DDP_HIP_FLAG_FRAME_AIM_COST;

static CostBlock block(int32_t items) {
  CostBlock k;
  k.desc = &kCostDesc[COST_FRAME_AIM];
  k.max_items = k.desc->max_items;
  k.items = items;
  return k;
}

static int check(int32_t items, const std::vector<double>& target, const std::vector<double>& weight, int64_t first, int64_t count, bool* copy,
                 bool* nonzero, uint32_t flags = ON) {
  const CostBlock k = block(items);
  CostCheck c;
  c.items = items;
  const double* host[COST_MAX_SIDES] = {target.empty() ? nullptr : target.data(), weight.empty() ? nullptr : weight.data(), nullptr};
  const CostSideOk ok[] = {cost_aim_target_side, cost_weight_side};
  return cost_upload_check(flags, k, c, B, T, host, ok, first, count, copy, nonzero);
}

int main() {
  const double nan = NAN, inf = INFINITY;
  bool copy, nonzero;

  // ---- the record: (g, rho) | (w_aim, w_range) per frame, a candidates' array, laid out by set_frames, T+1 rows ------------------
  {
    const CostDesc& d = kCostDesc[COST_FRAME_AIM];
    CHECK(COST_FRAME_AIM == COST_COM + 1 && COST_FRAME_AIM == COST_FRAME_VEL - 1);
    CHECK(d.flag == 16384u && DDP_HIP_MAX_AIM_FRAMES == 4);
    CHECK(d.nside == 2);
    CHECK(d.unit[0] == 4 && d.unit[1] == 2 && d.unit[2] == 0);
    CHECK(d.fill[0] == FILL_ZERO && d.fill[1] == FILL_ZERO);
    CHECK(d.max_items == DDP_HIP_MAX_AIM_FRAMES && !d.fixed && d.cand && !d.stage_only);
    const CostBlock k = block(3);
    CHECK(cost_rows(k, T) == T + 1);
    CHECK(cost_side_words(k, 0, T) == (T + 1) * 3 * 4 && cost_side_words(k, 1, T) == (T + 1) * 3 * 2);
    for (int t = 0; t < COST_COUNT; ++t)                                 // every row of the table is the row of its term: no flag twice
      for (int u = t + 1; u < COST_COUNT; ++u) CHECK(kCostDesc[t].flag != kCostDesc[u].flag);
    CHECK(kCostDesc[COST_COM].flag == DDP_HIP_FLAG_COM_COST && kCostDesc[COST_FRAME_VEL].flag == DDP_HIP_FLAG_FRAME_VEL_COST);   // the neighbours kept their rows
  }

  // ---- the frame-list rules -----------------------------------------------------------------------------------------------------
  {
    const int32_t nj = 6;
    const int32_t joint[3] = {0, 5, 5};                                  // two frames on one joint are allowed
    const double off[9] = {0.0, 0.1, -0.2, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0};
    const double axis[9] = {1.0, 0.0, 0.0, 0.0, 0.6, -0.8, 0.0, 0.0, -1.0};
    CHECK(cost_aim_frames_ok(nj, 3, joint, off, axis));
    CHECK(cost_aim_frames_ok(nj, 0, joint, off, axis));                  // (the count's range is the caller's)
    CHECK(cost_aim_frames_ok(nj, 0, nullptr, nullptr, nullptr));         // ... and with none nothing is read
    const int32_t hi[1] = {6}, neg[1] = {-1};
    CHECK(!cost_aim_frames_ok(nj, 1, hi, off, axis));                    // a joint one past the model
    CHECK(cost_aim_frames_ok(7, 1, hi, off, axis));
    CHECK(!cost_aim_frames_ok(nj, 1, neg, off, axis));
    const int32_t late[3] = {0, 5, 6};                                   // the last frame of the list is read
    CHECK(!cost_aim_frames_ok(nj, 3, late, off, axis));
    CHECK(cost_aim_frames_ok(nj, 2, late, off, axis));                   // ... and nothing beyond the count
    for (double bad : {nan, inf, -inf})
      for (int at : {0, 8}) {                                            // a non-finite offset, first or last double
        double ob[9];
        for (int k = 0; k < 9; ++k) ob[k] = off[k];
        ob[at] = bad;
        CHECK(!cost_aim_frames_ok(nj, 3, joint, ob, axis));
        CHECK(cost_aim_frames_ok(nj, 2, joint, ob, axis) == (at != 0));  // ... beyond the count is not read
      }
    // the axis rule: | |a| - 1 | <= 1e-10, the quaternions' rule
    for (double bad : {0.6 + 2e-10, 0.6 - 2e-10, 0.0, 1.0, nan, inf, -inf}) {   // |.| = 1 +- 1.2e-10, 0.8, 1.28, not finite
      double ab[9];
      for (int k = 0; k < 9; ++k) ab[k] = axis[k];
      ab[4] = bad;
      CHECK(!cost_aim_frames_ok(nj, 3, joint, off, ab));
      CHECK(cost_aim_frames_ok(nj, 1, joint, off, ab));                  // ... beyond the count is not read
    }
    {
      double az[9], an[9], a2[9];
      for (int k = 0; k < 9; ++k) az[k] = an[k] = a2[k] = axis[k];
      az[0] = 0.0;                                                       // the zero vector is no direction
      CHECK(!cost_aim_frames_ok(nj, 3, joint, off, az));
      an[4] = 0.6 + 5e-11;                                               // within 1e-10 of the sphere: accepted
      CHECK(cost_aim_frames_ok(nj, 3, joint, off, an));
      a2[8] = -2.0;                                                      // a direction that is not normalised is refused, not rescaled
      CHECK(!cost_aim_frames_ok(nj, 3, joint, off, a2));
    }
  }

  // ---- an upload's decisions ----------------------------------------------------------------------------------------------------
  {
    const int32_t nf = 3;
    const size_t slots = (size_t)(B * (T + 1) * nf);
    std::vector<double> g(4 * slots, -0.25), w(2 * slots, 0.0);
    for (size_t i = 0; i < slots; ++i) g[4 * i + 3] = 0.5;               // the stand-offs
    CHECK(check(nf, g, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    w[2 * slots - 1] = 1e-300;                                           // the last double of the range is read
    CHECK(check(nf, g, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(nf, {}, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && nonzero);
    CHECK(check(nf, g, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);
    CHECK(check(nf, {}, {}, 0, B, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);
    CHECK(check(nf, g, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK && copy && !nonzero);   // the non-zero lies beyond the range
    for (double bad : {nan, inf, -inf})
      for (size_t at : {(size_t)0, 4 * slots - 2, 4 * slots - 1}) {      // a non-finite target coordinate, a non-finite stand-off
        std::vector<double> gb = g;
        gb[at] = bad;
        CHECK(check(nf, gb, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
        CHECK(check(nf, gb, {}, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
        if (at != 0) CHECK(check(nf, gb, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK);   // ... beyond the range is not read
      }
    {
      std::vector<double> gb = g;                                        // a negative stand-off; a negative coordinate is a coordinate
      gb[4 * slots - 1] = -1e-300;
      CHECK(check(nf, gb, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
      CHECK(check(nf, gb, w, 0, B - 1, &copy, &nonzero) == DDP_HIP_OK);
      gb[4 * slots - 1] = 0.0;                                           // rho = 0 is a stand-off
      gb[4 * slots - 2] = -7.0;
      CHECK(check(nf, gb, w, 0, B, &copy, &nonzero) == DDP_HIP_OK && copy);
      gb[3] = -0.5;                                                      // the first stand-off is read
      CHECK(check(nf, gb, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
    }
    for (double bad : {-1e-300, nan, inf, -inf})                         // a bad weight, w_aim or w_range
      for (size_t at : {(size_t)0, (size_t)1}) {
        std::vector<double> wb = w;
        wb[at] = bad;
        CHECK(check(nf, g, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
        CHECK(check(nf, {}, wb, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);
        CHECK(check(nf, g, wb, 1, B - 1, &copy, &nonzero) == DDP_HIP_E_ARG);   // (host arrays start at `first`)
      }
    CHECK(check(0, g, w, 0, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);              // before set_frames: no layout
    CHECK(check(0, {}, {}, 0, 0, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(nf, g, w, 1, B, &copy, &nonzero) == DDP_HIP_E_ARG && !copy);             // bad ranges
    CHECK(check(nf, g, w, -1, 1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(nf, g, w, 0, -1, &copy, &nonzero) == DDP_HIP_E_ARG);
    CHECK(check(nf, g, w, B, 0, &copy, &nonzero) == DDP_HIP_OK && !copy && !nonzero);
    CHECK(check(nf, g, w, 0, B, &copy, &nonzero, DDP_HIP_FLAG_FRAME_COST | DDP_HIP_FLAG_FRAME_ORIENT_COST | DDP_HIP_FLAG_RELATIVE_FRAME_COST) ==
          DDP_HIP_E_UNSUPPORTED);                                                         // the flag stands alone
    CHECK(check(nf, g, w, -1, 1, &copy, &nonzero, 0) == DDP_HIP_E_UNSUPPORTED);           // ... and is checked first
  }

  // ---- the live rule on half-batch uploads --------------------------------------------------------------------------------------
  {
    bool live = false;
    live = cost_live_rule(live, true, 1, 1, B);                          // one instance's non-zero weights switch the kernels on
    CHECK(live);
    live = cost_live_rule(live, false, 0, 2, B);                         // zeros range by range leave them launched
    CHECK(live);
    live = cost_live_rule(live, false, 0, B, B);                         // one upload of zeros for the whole batch switches them off
    CHECK(!live);
  }

  if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
  printf("frame_aim_block: all checks passed\n");
  return 0;
}
