// The device-free parts of the capsule pairs of kind DDP_HIP_CAPSULE_VS_GRID (ddp_pinocchio_amd/csrc/capsule_cost.h, cost_block.h):
// the interval rule, the sampling routine compiled for the host against values worked out by hand on the 2 x 2 x 2 and 3 x 2 x 4
// grids of test_obstacle_grid_block.cpp (first-wins tie, all outside, partly outside, a NaN end), the dealt form of the scan
// against the scan itself, and the pair-list rule with and without a resident grid.  No HIP, no device: a plain host program.
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

static bool near(double a, double b) { return fabs(a - b) <= 1e-14 * (1.0 + fabs(b)); }

static ObstacleGridDev grid(const std::vector<double>& phi, int nx, int ny, int nz, double ox, double oy, double oz, double cell) {
  ObstacleGridDev G;
  G.phi = phi.data();
  G.n[0] = nx; G.n[1] = ny; G.n[2] = nz;
  G.origin[0] = ox; G.origin[1] = oy; G.origin[2] = oz;
  G.cell = cell;
  return G;
}

// ---- N_k = 0 for a sphere, else ceil(L / cell) within 1 .. 32 -------------------------------------------------------------------------
static void test_intervals() {
  const double o[3] = {0.3, -0.2, 0.1};
  CHECK(capsule_grid_intervals(o, o, 0.1) == 0);
  const double cell = 0.125;                                             // (a power of two: L / cell is exact)
  for (int k = 1; k <= 40; ++k) {
    const double L = k * cell;
    const double z[3] = {0.0, 0.0, 0.0}, zat[3] = {0.0, 0.0, L}, zun[3] = {0.0, 0.0, nextafter(L, 0.0)}, zov[3] = {0.0, 0.0, nextafter(L, 100.0)};
    const int cap = DDP_HIP_CAPSULE_GRID_MAX_INTERVALS;
    CHECK(capsule_grid_intervals(z, zat, cell) == (k < cap ? k : cap));
    CHECK(capsule_grid_intervals(z, zun, cell) == (k < cap ? k : cap));
    CHECK(capsule_grid_intervals(z, zov, cell) == (k + 1 < cap ? k + 1 : cap));
    CHECK(capsule_grid_intervals(zat, z, cell) == (k < cap ? k : cap));    // either direction
  }
  const double tiny[3] = {0.3, -0.2, 0.1 + 1e-300}, huge[3] = {1e300, 0.0, 0.0}, z[3] = {0.0, 0.0, 0.0};
  CHECK(capsule_grid_intervals(o, tiny, 0.1) == 0);                      // the end is the same double: a sphere
  const double small[3] = {0.0, 1e-200, 0.0};
  CHECK(capsule_grid_intervals(z, small, 0.1) == 0);                     // the products underflow: L == 0 by the pinned arithmetic
  const double shortish[3] = {0.0, 1e-9, 0.0};
  CHECK(capsule_grid_intervals(z, shortish, 0.1) == 1);                  // shorter than a cell: the two ends
  CHECK(capsule_grid_intervals(z, huge, 0.1) == DDP_HIP_CAPSULE_GRID_MAX_INTERVALS);
  const double diag[3] = {0.3, 0.4, 1.2};                                // L = 1.3
  CHECK(capsule_grid_intervals(z, diag, 0.1) == 13 || capsule_grid_intervals(z, diag, 0.1) == 14);
  CHECK(capsule_grid_intervals(z, diag, 0.5) == 3);
}

// the scan dealt over `lanes` lanes as the kernels deal it (each lane its samples, the values left in a table, then one scan in
// ascending j) selects what capsule_grid_closest selects, to the bit
static void check_dealt(const ObstacleGridDev& G, const double* a0, const double* a1, const double* s, int32_t N, int lanes) {
  double table[DDP_HIP_CAPSULE_GRID_MAX_INTERVALS + 1];
  for (int l = lanes - 1; l >= 0; --l)                                    // (the lanes in another order than the samples')
    for (int j = l; j <= N; j += lanes) {
      double c[3], g[3];
      capsule_grid_sample(G, a0, a1, s, N, j, c, &table[j], g);
    }
  double best = table[0];
  int32_t bj = 0;
  for (int32_t j = 1; j <= N; ++j)
    if (capsule_grid_better(table[j], best, false)) { best = table[j]; bj = j; }
  double phi, c[3], g[3];
  int32_t j;
  capsule_grid_closest(G, a0, a1, s, N, &phi, &j, c, g);
  CHECK(j == (best == INFINITY ? -1 : bj));
  CHECK((phi != phi && best != best) || phi == best);
}

// ---- 2 x 2 x 2: corners 1 2 3 5 7 11 13 17 (z fastest), origin (1, -1, 2), cell 0.5 ---------------------------------------------------
static void test_cube() {
  const std::vector<double> phi = {1, 2, 3, 5, 7, 11, 13, 17};
  const ObstacleGridDev G = grid(phi, 2, 2, 2, 1.0, -1.0, 2.0, 0.5);
  const double zero[3] = {0.0, 0.0, 0.0};
  double v, c[3], g[3];
  int32_t j;
  // along the x edge from corner 000 (1) to corner 100 (7), N = 4: the values 1, 2.5, 4, 5.5, 7: j* = 0
  const double a0[3] = {1.0, -1.0, 2.0}, a1[3] = {1.5, -1.0, 2.0};
  capsule_grid_closest(G, a0, a1, zero, 4, &v, &j, c, g);
  CHECK(j == 0 && v == 1.0 && c[0] == 1.0 && c[1] == -1.0 && c[2] == 2.0 && near(g[0], 12.0) && near(g[1], 4.0) && near(g[2], 2.0));
  // the other way round: j* = 4, the same point
  capsule_grid_closest(G, a1, a0, zero, 4, &v, &j, c, g);
  CHECK(j == 4 && v == 1.0 && c[0] == 1.0);
  // N = 0: the point lookup at a0, a1 not read for the point
  capsule_grid_closest(G, a1, a0, zero, 0, &v, &j, c, g);
  CHECK(j == 0 && v == 7.0 && c[0] == 1.5);
  // a shift: the segment lies 0.25 off and the shift brings it back
  const double s[3] = {0.25, -0.25, 0.25}, b0[3] = {1.25, -1.25, 2.25}, b1[3] = {1.75, -1.25, 2.25};
  capsule_grid_closest(G, b0, b1, s, 4, &v, &j, c, g);
  CHECK(j == 0 && v == 1.0 && c[0] == 1.25 && c[1] == -1.25 && c[2] == 2.25);        // c is the material point, not the shifted one
  // first wins a tie: a constant field, every sample -0.25
  const std::vector<double> flat(8, -0.25);
  const ObstacleGridDev F = grid(flat, 2, 2, 2, 1.0, -1.0, 2.0, 0.5);
  const double d1[3] = {1.5, -0.5, 2.5};
  capsule_grid_closest(F, a0, d1, zero, 7, &v, &j, c, g);
  CHECK(j == 0 && v == -0.25 && g[0] == 0.0 && g[1] == 0.0 && g[2] == 0.0);
  double d, u[3];
  CHECK(!capsule_grid_pair(v, g, 0.125, -0.5, &d, u) && near(d, -0.25 - 0.125 + 0.5));   // a zero gradient: value, no derivative
  // all outside: j = -1, +inf, c = a0, a zero gradient; the pair forms nothing
  const double f0[3] = {5.0, -0.5, 2.5}, f1[3] = {6.0, -0.5, 2.5};
  capsule_grid_closest(G, f0, f1, zero, 3, &v, &j, c, g);
  CHECK(j == -1 && v == INFINITY && c[0] == 5.0 && g[0] == 0.0 && g[1] == 0.0 && g[2] == 0.0);
  CHECK(!capsule_grid_pair(v, g, 0.125, 0.0, &d, u) && d == INFINITY);
  // partly outside: from the centre (59 / 8) out through the face x = 1.5, N = 4: samples at x = 1.25, 1.4375 inside, then outside;
  // phi grows with x, so j* = 0
  const double p0[3] = {1.25, -0.75, 2.25}, p1[3] = {2.0, -0.75, 2.25};
  capsule_grid_closest(G, p0, p1, zero, 4, &v, &j, c, g);
  CHECK(j == 0 && near(v, 7.375) && near(g[0], 18.5));
  // ... and entering: the first two samples are outside, sample 2 is the face x = 1 (mean of 1 2 3 5 = 2.75), sample 3 further in
  const double q0[3] = {0.5, -0.75, 2.25}, q1[3] = {1.5, -0.75, 2.25};
  capsule_grid_closest(G, q0, q1, zero, 4, &v, &j, c, g);
  CHECK(j == 2 && near(v, 2.75) && c[0] == 1.0);
  // a NaN end: every sample is NaN (0 * NaN), the first is taken; the pair is active with a NaN distance
  const double n1[3] = {1.5, NAN, 2.0};
  capsule_grid_closest(G, a0, n1, zero, 4, &v, &j, c, g);
  CHECK(j == 0 && v != v && g[1] != g[1]);
  CHECK(capsule_grid_pair(v, g, 0.125, 0.0, &d, u) && d != d);
  // the selection rule itself
  CHECK(capsule_grid_better(1.0, 2.0, false) && !capsule_grid_better(2.0, 2.0, false) && !capsule_grid_better(3.0, 2.0, false));
  CHECK(capsule_grid_better(NAN, -5.0, false) && !capsule_grid_better(-5.0, NAN, false) && !capsule_grid_better(NAN, NAN, false));
  CHECK(capsule_grid_better(1.0, INFINITY, false) && !capsule_grid_better(INFINITY, INFINITY, false) && capsule_grid_better(INFINITY, 0.0, true));
  for (int lanes : {1, 3, 16, 64}) {
    check_dealt(G, a0, a1, zero, 4, lanes);
    check_dealt(G, q0, q1, zero, 4, lanes);
    check_dealt(G, f0, f1, zero, 3, lanes);
    check_dealt(G, a0, n1, zero, 4, lanes);
    check_dealt(F, a0, d1, zero, 32, lanes);
  }
}

// ---- 3 x 2 x 4: phi(ix, iy, iz) = 10 ix + 3 iy - iz + ix iz, multilinear, cell 0.25 ---------------------------------------------------
static void test_box() {
  std::vector<double> phi(24);
  for (int ix = 0; ix < 3; ++ix)
    for (int iy = 0; iy < 2; ++iy)
      for (int iz = 0; iz < 4; ++iz) phi[(ix * 2 + iy) * 4 + iz] = 10.0 * ix + 3.0 * iy - iz + ix * iz;
  const ObstacleGridDev G = grid(phi, 3, 2, 4, 0.0, 0.0, 0.0, 0.25);
  const double zero[3] = {0.0, 0.0, 0.0};
  double v, c[3], g[3];
  int32_t j;
  // along z at (ix, iy) = (0, 0.5): phi = 1.5 - iz falls, so the far end wins; N = 3 puts the samples on the nodes: 1.5 .. -1.5
  const double a0[3] = {0.0, 0.125, 0.0}, a1[3] = {0.0, 0.125, 0.75};
  CHECK(capsule_grid_intervals(a0, a1, 0.25) == 3);
  capsule_grid_closest(G, a0, a1, zero, 3, &v, &j, c, g);
  CHECK(j == 3 && near(v, -1.5) && c[2] == 0.75 && near(g[0], 4.0 * 13.0) && near(g[1], 12.0) && near(g[2], -4.0));
  // along z at ix = 1: phi = 10 + 3 iy - iz + iz is constant in z: first wins, through the last cell of the axis
  const double b0[3] = {0.25, 0.0, 0.0}, b1[3] = {0.25, 0.0, 0.75};
  capsule_grid_closest(G, b0, b1, zero, 6, &v, &j, c, g);
  CHECK(j == 0 && v == 10.0);
  // through the last node (2, 1, 3) from outside the far corner: the last sample inside is the node itself at j = 2 of 4
  const double c0[3] = {0.5, 0.25, 0.75}, c1[3] = {1.0, 0.5, 1.5};
  capsule_grid_closest(G, c1, c0, zero, 4, &v, &j, c, g);
  CHECK(j == 4 && v == 26.0);
  // a diagonal: the samples' values by the function itself
  const double d0[3] = {0.05, 0.02, 0.7}, d1[3] = {0.45, 0.24, 0.1};
  const int N = 5;
  double best = INFINITY;
  int bj = -1;
  for (int s = 0; s <= N; ++s) {
    const double t = (double)s / N, x = (d0[0] + t * (d1[0] - d0[0])) / 0.25, y = (d0[1] + t * (d1[1] - d0[1])) / 0.25, z = (d0[2] + t * (d1[2] - d0[2])) / 0.25;
    const double f = 10.0 * x + 3.0 * y - z + x * z;
    if (f < best) { best = f; bj = s; }
  }
  capsule_grid_closest(G, d0, d1, zero, N, &v, &j, c, g);
  CHECK(j == bj && fabs(v - best) <= 1e-13 * (1.0 + fabs(best)));
  for (int lanes : {1, 2, 16}) {
    check_dealt(G, a0, a1, zero, 3, lanes);
    check_dealt(G, b0, b1, zero, 6, lanes);
    check_dealt(G, d0, d1, zero, N, lanes);
  }
}

// ---- the pair list: kind 3 needs a resident grid; the six-argument form is the one without ---------------------------------------------
static void test_pairs() {
  const int32_t joint[3] = {1, 2, 2};
  const int32_t a[4] = {0, 1, 2, 0}, b[4] = {1, 99, -5, 99};
  const int32_t with_grid[4] = {DDP_HIP_CAPSULE_VS_ROBOT, DDP_HIP_CAPSULE_VS_GRID, DDP_HIP_CAPSULE_VS_HALFSPACE, DDP_HIP_CAPSULE_VS_GRID};
  const int32_t without[4] = {DDP_HIP_CAPSULE_VS_ROBOT, DDP_HIP_CAPSULE_VS_CAPSULE, DDP_HIP_CAPSULE_VS_HALFSPACE, DDP_HIP_CAPSULE_VS_CAPSULE};
  CHECK(cost_capsule_pairs_ok(3, joint, 4, a, with_grid, b, true));      // (pair_b of a grid pair is not read)
  CHECK(!cost_capsule_pairs_ok(3, joint, 4, a, with_grid, b, false));
  CHECK(!cost_capsule_pairs_ok(3, joint, 4, a, with_grid, b));
  CHECK(cost_capsule_pairs_ok(3, joint, 4, a, without, b, true) && cost_capsule_pairs_ok(3, joint, 4, a, without, b, false));
  CHECK(cost_capsule_pairs_ok(3, joint, 4, a, without, b));
  const int32_t bad_a[4] = {0, 3, 2, 0};
  CHECK(!cost_capsule_pairs_ok(3, joint, 4, bad_a, with_grid, b, true));  // body A of a grid pair is checked like any other
  const int32_t unknown[4] = {DDP_HIP_CAPSULE_VS_ROBOT, 4, DDP_HIP_CAPSULE_VS_HALFSPACE, DDP_HIP_CAPSULE_VS_GRID};
  CHECK(!cost_capsule_pairs_ok(3, joint, 4, a, unknown, b, true));
  // the geometry validator needs nothing new: eight finite doubles, whatever their values
  CostCheck c;
  c.items = 1;
  const int32_t kind[1] = {DDP_HIP_CAPSULE_VS_GRID};
  c.kind = kind;
  double g[8] = {0.1, -0.2, 0.3, -7.0, 0.0, 1e9, -1.0, -0.05};
  CHECK(cost_capsule_geom_side(c, g, 8));
  for (int e = 0; e < 8; ++e) {
    const double keep = g[e];
    g[e] = NAN;
    CHECK(!cost_capsule_geom_side(c, g, 8));
    g[e] = INFINITY;
    CHECK(!cost_capsule_geom_side(c, g, 8));
    g[e] = keep;
  }
}

int main() {
  test_intervals();
  test_cube();
  test_box();
  test_pairs();
  if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
  printf("capsule grid block: all checks passed\n");
  return 0;
}
