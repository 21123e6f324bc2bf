// The device-free parts of the capsule pairs of kind DDP_HIP_CAPSULE_VS_BOX (ddp_pinocchio_amd/csrc/capsule_cost.h, cost_block.h): the
// pinned search capsule_box_closest compiled for the host against a dense scan of the segment parameter on random cases, against
// cases worked out by hand with the exact s the rule gives (a sphere outside and inside; face, edge and corner; parallel to a
// face; along an edge; through the box at a kink; wholly inside; an end on a face; a rotated box against the same case in box
// axes), the geometry validator per kind and the pair-list rule with a box count.  No HIP, no device: a plain host program.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../ddp_pinocchio_amd/csrc/capsule_cost.h"
#include "../ddp_pinocchio_amd/csrc/cost_block.h"

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_fail; } \
  } while (0)

static bool near(double a, double b) { return fabs(a - b) <= 1e-14 * (1.0 + fabs(b)); }
static bool near3(const double* a, double x, double y, double z) { return near(a[0], x) && near(a[1], y) && near(a[2], z); }

static const double kUnit[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0};      // centre 0, axes along the world's

// a small generator of its own (the cases must not depend on the C library's)
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uni() {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(g_state >> 11) / 9007199254740992.0;
}
static double normal() { return sqrt(-2.0 * log(1.0 - uni())) * cos(6.283185307179586 * uni()); }

// ---- the routine against a 2001-point scan of s on 300 random cases, a seventh of them parallel to a face pair -----------------------
static void test_scan() {
  for (int n = 0; n < 300; ++n) {
    double half[3], pose[7], a0[3], a1[3], qn = 0.0;
    for (int k = 0; k < 3; ++k) {
      half[k] = 0.05 + 0.45 * uni();
      pose[k] = 0.2 * normal();
      a0[k] = 0.5 * normal();
      a1[k] = a0[k] + 0.4 * normal();
    }
    for (int k = 3; k < 7; ++k) { pose[k] = normal(); qn += pose[k] * pose[k]; }
    for (int k = 3; k < 7; ++k) pose[k] /= sqrt(qn);
    if (n % 7 == 0) {                                                    // an axis-aligned box and a segment in a plane z = const
      for (int k = 3; k < 6; ++k) pose[k] = 0.0;
      pose[6] = 1.0;
      a1[2] = a0[2];
    }
    double s, ca[3], u[3];
    const double f = capsule_box_closest(a0, a1, half, pose, &s, ca, u);
    CHECK(s >= 0.0 && s <= 1.0);
    double best = INFINITY;
    for (int j = 0; j <= 2000; ++j) {
      const double t = j / 2000.0, p[3] = {a0[0] + t * (a1[0] - a0[0]), a0[1] + t * (a1[1] - a0[1]), a0[2] + t * (a1[2] - a0[2])};
      double sj, cj[3], uj[3];
      const double fj = capsule_box_closest(p, p, half, pose, &sj, cj, uj);   // (a point: the signed distance itself)
      if (fj < best) best = fj;
    }
    const double len = sqrt((a1[0] - a0[0]) * (a1[0] - a0[0]) + (a1[1] - a0[1]) * (a1[1] - a0[1]) + (a1[2] - a0[2]) * (a1[2] - a0[2]));
    CHECK(f <= best + 1e-12);
    CHECK(f >= best - len / 2000.0);
    for (int k = 0; k < 3; ++k) CHECK(near(ca[k], a0[k] + s * (a1[k] - a0[k])));
    if (f > 0.0) CHECK(fabs(sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]) - 1.0) <= 1e-12);
  }
}

// ---- cases worked out by hand: half extents (1, 2, 3) unless said otherwise -------------------------------------------------------------
static void test_pinned() {
  const double h[3] = {1.0, 2.0, 3.0};
  double s, ca[3], u[3], f;
  {  // a sphere outside, beside the face +x
    const double a[3] = {3.0, 0.5, -1.0};
    f = capsule_box_closest(a, a, h, kUnit, &s, ca, u);
    CHECK(f == 2.0 && s == 0.0 && near3(ca, 3.0, 0.5, -1.0) && near3(u, 1.0, 0.0, 0.0));
  }
  {  // a sphere inside: the nearest face is -y (|y| - 2 = -0.5 is the largest of the three)
    const double a[3] = {0.25, -1.5, 1.0};
    f = capsule_box_closest(a, a, h, kUnit, &s, ca, u);
    CHECK(f == -0.5 && s == 0.0 && near3(u, 0.0, -1.0, 0.0));
  }
  {  // the closest feature a face: a tilted segment above +z, its low end over the face
    const double a0[3] = {0.5, 0.5, 5.0}, a1[3] = {0.0, -1.0, 4.0};
    f = capsule_box_closest(a0, a1, h, kUnit, &s, ca, u);
    CHECK(f == 1.0 && s == 1.0 && near3(u, 0.0, 0.0, 1.0));
  }
  {  // an edge: the segment crosses over the edge x = 1, z = 3 (along y) at right angles to the diagonal; closest at its middle
    const double a0[3] = {3.0, 0.0, 3.0}, a1[3] = {1.0, 0.0, 5.0};
    f = capsule_box_closest(a0, a1, h, kUnit, &s, ca, u);
    CHECK(s == 0.5 && near(f, sqrt(2.0)) && near3(ca, 2.0, 0.0, 4.0) && near3(u, sqrt(0.5), 0.0, sqrt(0.5)));
  }
  {  // a corner: a sphere off the corner (1, 2, 3)
    const double a[3] = {2.0, 4.0, 5.0};
    f = capsule_box_closest(a, a, h, kUnit, &s, ca, u);
    CHECK(f == 3.0 && s == 0.0 && near3(u, 1.0 / 3.0, 2.0 / 3.0, 2.0 / 3.0));
  }
  {  // ... and a segment whose interior point is closest to that corner
    const double a0[3] = {2.0, 3.0, 3.0}, a1[3] = {2.0, 2.0, 4.0};      // y - 2 = 1 - s, z - 3 = s: sum of squares least at s = 1/2
    f = capsule_box_closest(a0, a1, h, kUnit, &s, ca, u);
    CHECK(s == 0.5 && near(f, sqrt(1.5)) && near3(ca, 2.0, 2.5, 3.5));
  }
  {  // parallel to the face +z, all of it over the face: every s attains 0.5, the smallest wins
    const double a0[3] = {-0.5, 1.0, 3.5}, a1[3] = {0.5, -1.0, 3.5};
    f = capsule_box_closest(a0, a1, h, kUnit, &s, ca, u);
    CHECK(f == 0.5 && s == 0.0 && near3(u, 0.0, 0.0, 1.0));
  }
  {  // parallel to +z and longer than the face: the flat stretch begins where x enters the slab, s = 1/4
    const double a0[3] = {-2.0, 0.0, 3.5}, a1[3] = {2.0, 0.0, 3.5};
    f = capsule_box_closest(a0, a1, h, kUnit, &s, ca, u);
    CHECK(f == 0.5 && s == 0.25 && near3(ca, -1.0, 0.0, 3.5) && near3(u, 0.0, 0.0, 1.0));
  }
  {  // along the edge x = 1, z = 3: f == 0 from where y enters the slab (s = 1/4: y = -2); value and no derivative
    const double a0[3] = {1.0, -4.0, 3.0}, a1[3] = {1.0, 4.0, 3.0};
    f = capsule_box_closest(a0, a1, h, kUnit, &s, ca, u);
    double d;
    CHECK(f == 0.0 && s == 0.25 && !capsule_box_pair(f, 0.1, 0.05, &d) && near(d, -0.15));
  }
  {  // through the box at a kink: inside, l(0+) = x - 1 = -0.1 - s falls and l(1+) = y - 2 =
     // -2 + 1.9 s rises; they cross at s = 1.9 / 2.9, where both are -0.1 - 1.9 / 2.9 and every other line is lower: the least of the
     // largest line.  n = (|slope_j| n_i + |slope_i| n_j) / (|slope_i| + |slope_j|) = (1.9 e_x + 1 e_y) / 2.9
    const double a0[3] = {0.9, 0.0, 0.0}, a1[3] = {-0.1, 1.9, 0.0};
    f = capsule_box_closest(a0, a1, h, kUnit, &s, ca, u);
    CHECK(near(s, 1.9 / 2.9) && near(f, -0.1 - 1.9 / 2.9));
    CHECK(near3(u, 1.9 / 2.9, 1.0 / 2.9, 0.0));
  }
  {  // through the box parallel to the face +z, 0.5 under it: f = -0.5 on a whole stretch, the minimiser is not unique.  The rule
     // takes the first candidate that attains it, the crossing of the lines 0+ and 0- at s = 1/2; their slopes are opposite, so the
     // kink formula applies and gives n = 0 (ddp_hip.h: the direction is exact where the minimiser is unique)
    const double a0[3] = {-3.0, 0.0, 2.5}, a1[3] = {3.0, 0.0, 2.5};
    f = capsule_box_closest(a0, a1, h, kUnit, &s, ca, u);
    CHECK(f == -0.5 && s == 0.5 && near3(u, 0.0, 0.0, 0.0));
  }
  {  // wholly inside, no kink: the minimum at an end (the deeper one)
    const double a0[3] = {0.5, 0.0, 0.0}, a1[3] = {0.0, 0.0, 0.0};
    f = capsule_box_closest(a0, a1, h, kUnit, &s, ca, u);
    CHECK(f == -1.0 && s == 1.0 && near3(u, 1.0, 0.0, 0.0));             // (at the centre line 0+ is the first to attain -1)
  }
  {  // an end exactly on a face, the rest outside: f == 0 at s = 0
    const double a0[3] = {1.0, 0.0, 0.0}, a1[3] = {2.0, 0.0, 0.0};
    f = capsule_box_closest(a0, a1, h, kUnit, &s, ca, u);
    CHECK(f == 0.0 && s == 0.0);
  }
  {  // a rotated and shifted box against the same case in box axes: a quarter turn about z (x_box -> y_world), centre (1, -2, 0.5)
    const double r = sqrt(0.5), pose[7] = {1.0, -2.0, 0.5, 0.0, 0.0, r, r};
    const double b0[3] = {3.0, 0.0, 3.0}, b1[3] = {1.0, 0.0, 5.0};      // the edge case above, in box axes
    double w0[3], w1[3];
    // world = R box + c with R = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    w0[0] = -b0[1] + pose[0]; w0[1] = b0[0] + pose[1]; w0[2] = b0[2] + pose[2];
    w1[0] = -b1[1] + pose[0]; w1[1] = b1[0] + pose[1]; w1[2] = b1[2] + pose[2];
    f = capsule_box_closest(w0, w1, h, pose, &s, ca, u);
    CHECK(fabs(s - 0.5) <= 1e-14 && fabs(f - sqrt(2.0)) <= 1e-14);
    CHECK(fabs(u[0]) <= 1e-14 && fabs(u[1] - r) <= 1e-14 && fabs(u[2] - r) <= 1e-14);   // R (r, 0, r) = (0, r, r)
    CHECK(fabs(ca[0] - 1.0) <= 1e-14 && fabs(ca[1] - 0.0) <= 1e-14 && fabs(ca[2] - 4.5) <= 1e-14);
  }
  {  // a quaternion of all zeros is the identity by the formula (ddp_hip.h says so)
    const double zero[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, a[3] = {3.0, 0.5, -1.0};
    f = capsule_box_closest(a, a, h, zero, &s, ca, u);
    CHECK(f == 2.0 && near3(u, 1.0, 0.0, 0.0));
  }
  {  // a NaN end: the value is NaN, and the pair is active
    const double a0[3] = {3.0, 0.5, -1.0}, a1[3] = {NAN, 0.0, 0.0};
    f = capsule_box_closest(a0, a1, h, kUnit, &s, ca, u);
    double d;
    CHECK(f != f && capsule_box_pair(f, 0.0, 0.0, &d) && d != d);
  }
}

// ---- the geometry validator per kind and the pair list with a box count -------------------------------------------------------------------
static void test_host_logic() {
  CostCheck c;
  c.items = 1;
  const int32_t box[1] = {DDP_HIP_CAPSULE_VS_BOX}, cap[1] = {DDP_HIP_CAPSULE_VS_CAPSULE}, hs[1] = {DDP_HIP_CAPSULE_VS_HALFSPACE}, grid[1] = {DDP_HIP_CAPSULE_VS_GRID},
                robot[1] = {DDP_HIP_CAPSULE_VS_ROBOT};
  const double r = sqrt(0.5);
  double g[8] = {0.1, -0.2, 0.3, r, 0.0, 0.0, r, -0.05};
  c.kind = box;
  CHECK(cost_capsule_geom_side(c, g, 8));
  for (int e = 0; e < 8; ++e) {
    const double keep = g[e];
    g[e] = NAN;
    CHECK(!cost_capsule_geom_side(c, g, 8));
    g[e] = INFINITY;
    CHECK(!cost_capsule_geom_side(c, g, 8));
    g[e] = keep;
  }
  g[3] = r * (1.0 + 1e-9);                                               // not unit by the interface's rule
  CHECK(!cost_capsule_geom_side(c, g, 8));
  g[3] = r * (1.0 + 1e-11);
  CHECK(cost_capsule_geom_side(c, g, 8));
  g[3] = r;
  const double zeros[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // freshly reset geometry is no box pose ...
  CHECK(!cost_capsule_geom_side(c, zeros, 8));
  c.kind = robot;                                                        // ... but every other kind's rule is what it was
  CHECK(cost_capsule_geom_side(c, zeros, 8) && cost_capsule_geom_side(c, g, 8));
  c.kind = grid;
  CHECK(cost_capsule_geom_side(c, zeros, 8) && cost_capsule_geom_side(c, g, 8));
  c.kind = cap;
  CHECK(cost_capsule_geom_side(c, g, 8));                                // rho = g[6] = r >= 0
  c.kind = hs;
  CHECK(!cost_capsule_geom_side(c, g, 8));                               // (0.1, -0.2, 0.3) is no unit normal

  const int32_t joint[3] = {1, 2, 2};
  const int32_t a[3] = {0, 1, 2}, kinds[3] = {DDP_HIP_CAPSULE_VS_BOX, DDP_HIP_CAPSULE_VS_CAPSULE, DDP_HIP_CAPSULE_VS_BOX};
  const int32_t b_ok[3] = {1, 99, 1}, b_hi[3] = {1, 99, 2}, b_neg[3] = {-1, 0, 0};
  CHECK(cost_capsule_pairs_ok(3, joint, 3, a, kinds, b_ok, false, 2));   // several pairs may name one shape
  CHECK(!cost_capsule_pairs_ok(3, joint, 3, a, kinds, b_hi, false, 2));
  CHECK(cost_capsule_pairs_ok(3, joint, 3, a, kinds, b_hi, false, 3));
  CHECK(!cost_capsule_pairs_ok(3, joint, 3, a, kinds, b_neg, false, 2));
  CHECK(!cost_capsule_pairs_ok(3, joint, 3, a, kinds, b_ok, false, 0));  // no boxes set: every box pair is refused,
  CHECK(!cost_capsule_pairs_ok(3, joint, 3, a, kinds, b_ok, true));      // ... as by the forms without a count
  CHECK(!cost_capsule_pairs_ok(3, joint, 3, a, kinds, b_ok));
  const int32_t bad_a[3] = {3, 1, 2};
  CHECK(!cost_capsule_pairs_ok(3, joint, 3, bad_a, kinds, b_ok, false, 2));
  const int32_t unknown[3] = {5, DDP_HIP_CAPSULE_VS_CAPSULE, DDP_HIP_CAPSULE_VS_BOX};
  CHECK(!cost_capsule_pairs_ok(3, joint, 3, a, unknown, b_ok, true, 2));
  const int32_t mixed[3] = {DDP_HIP_CAPSULE_VS_GRID, DDP_HIP_CAPSULE_VS_ROBOT, DDP_HIP_CAPSULE_VS_BOX}, b_mixed[3] = {0, 0, 0};
  CHECK(cost_capsule_pairs_ok(3, joint, 3, a, mixed, b_mixed, true, 1));
  CHECK(!cost_capsule_pairs_ok(3, joint, 3, a, mixed, b_mixed, false, 1));   // the grid rule stands beside the box rule
}

int main() {
  test_scan();
  test_pinned();
  test_host_logic();
  if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
  printf("capsule box block: all checks passed\n");
  return 0;
}
