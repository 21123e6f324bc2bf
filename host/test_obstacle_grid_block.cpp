// The device-free parts of the voxel-grid obstacle kind (DDP_HIP_OBSTACLE_GRID; ddp_pinocchio_amd/csrc/obstacle_grid.h,
// cost_block.h): the trilinear lookup, compiled for the host, against values worked out by hand on a 2 x 2 x 2 and a 3 x 2 x 4 grid,
// the inside test at both ends of each axis, a slot's distance, the shape rules of the set calls, the field's formula, and the
// geometry validator with the new kind.  No HIP, no device: a plain host program.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "../ddp_pinocchio_amd/csrc/cost_block.h"
#include "../ddp_pinocchio_amd/csrc/obstacle_grid.h"

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

// ---- 2 x 2 x 2: corners (ix, iy, iz) -> 1 2 3 5 7 11 13 17 in memory order (z fastest), origin (1, -1, 2), cell 0.5 ------------------
static void test_cube() {
  const std::vector<double> phi = {1, 2, 3, 5, 7, 11, 13, 17};
  const ObstacleGridDev G = grid(phi, 2, 2, 2, 1.0, -1.0, 2.0, 0.5);
  double v, g[3];
  // the centre: the mean of the corners, 59 / 8; grad_x = 2 ((7 + 11 + 13 + 17) - (1 + 2 + 3 + 5)) / 4 and alike
  const double c[3] = {1.25, -0.75, 2.25};
  CHECK(obstacle_grid_lookup(G, c, &v, g) == GRID_INSIDE);
  CHECK(near(v, 7.375) && near(g[0], 18.5) && near(g[1], 8.5) && near(g[2], 5.5));
  // f = (0.25, 0, 1): on the edge between corners 001 (2) and 101 (11): 0.75 * 2 + 0.25 * 11
  const double e[3] = {1.125, -1.0, 2.5};
  CHECK(obstacle_grid_lookup(G, e, &v, g) == GRID_INSIDE);
  CHECK(near(v, 4.25) && near(g[0], 18.0) && near(g[1], 7.5) && near(g[2], 3.5));
  // every corner exactly, the far ones through i = n - 2, f = 1
  for (int ix = 0; ix < 2; ++ix)
    for (int iy = 0; iy < 2; ++iy)
      for (int iz = 0; iz < 2; ++iz) {
        const double p[3] = {1.0 + 0.5 * ix, -1.0 + 0.5 * iy, 2.0 + 0.5 * iz};
        CHECK(obstacle_grid_lookup(G, p, &v, g) == GRID_INSIDE && v == phi[(ix * 2 + iy) * 2 + iz]);
      }
  // a slot: shift (0.25, 0.25, 0.25) brings the point back to the centre; d = phi - r - m, u = grad phi
  const double geom[4] = {0.25, 0.25, 0.25, -0.5}, p[3] = {1.5, -0.5, 2.5};
  double d, u[3];
  CHECK(obstacle_grid_distance(G, geom, p, 0.125, &d, u));
  CHECK(near(d, 7.375 - 0.125 + 0.5) && near(u[0], 18.5) && near(u[1], 8.5) && near(u[2], 5.5));
  // outside: +inf, no direction; a NaN point: NaN
  const double far[3] = {5.0, -0.5, 2.5};
  CHECK(!obstacle_grid_distance(G, geom, far, 0.125, &d, u) && d == INFINITY && u[0] == 0.0 && u[1] == 0.0 && u[2] == 0.0);
  const double bad[3] = {1.5, NAN, 2.5};
  CHECK(obstacle_grid_distance(G, geom, bad, 0.125, &d, u) && d != d && u[0] != u[0]);
  CHECK(obstacle_grid_lookup(G, bad, &v, g) == GRID_NAN && v != v);
  // a constant field: the gradient is exactly zero, the pair has its value and no derivative
  const std::vector<double> flat(8, -0.25);
  const ObstacleGridDev F = grid(flat, 2, 2, 2, 1.0, -1.0, 2.0, 0.5);
  CHECK(!obstacle_grid_distance(F, geom, p, 0.125, &d, u) && near(d, -0.25 - 0.125 + 0.5) && u[0] == 0.0 && u[1] == 0.0 && u[2] == 0.0);
}

// ---- 3 x 2 x 4: phi(ix, iy, iz) = 10 ix + 3 iy - iz + ix iz, multilinear, so the interpolant is the function itself ----------------
static void test_box() {
  const int n[3] = {3, 2, 4};
  std::vector<double> phi(24);
  for (int ix = 0; ix < 3; ++ix)
    for (int iy = 0; iy < 2; ++iy)
      for (int iz = 0; iz < 4; ++iz) phi[(ix * 2 + iy) * 4 + iz] = 10.0 * ix + 3.0 * iy - iz + ix * iz;
  const ObstacleGridDev G = grid(phi, 3, 2, 4, 0.0, 0.0, 0.0, 0.25);
  double v, g[3];
  // s = (1.5, 0.25, 2.5): 15 + 0.75 - 2.5 + 3.75 = 17; the gradient in index units (10 + z, 3, -1 + x) = (12.5, 3, 0.5), over cell
  const double p[3] = {0.375, 0.0625, 0.625};
  CHECK(obstacle_grid_lookup(G, p, &v, g) == GRID_INSIDE);
  CHECK(near(v, 17.0) && near(g[0], 50.0) && near(g[1], 12.0) && near(g[2], 2.0));
  // the last node, (2, 1, 3): 20 + 3 - 3 + 6 (an axis-order slip in the flat index reads another node)
  const double last[3] = {0.5, 0.25, 0.75};
  CHECK(obstacle_grid_lookup(G, last, &v, g) == GRID_INSIDE && v == 26.0);
  const double node[3] = {0.25, 0.0, 0.5};      // (1, 0, 2): 10 - 2 + 2
  CHECK(obstacle_grid_lookup(G, node, &v, g) == GRID_INSIDE && v == 10.0);
  // the inside test: both ends of each axis are inside, one step of the number line beyond them is outside
  for (int a = 0; a < 3; ++a) {
    double q[3] = {0.125, 0.125, 0.125};
    const double hi = 0.25 * (n[a] - 1);
    q[a] = 0.0;
    CHECK(obstacle_grid_lookup(G, q, &v, g) == GRID_INSIDE && isfinite(v));
    q[a] = -0.0;
    CHECK(obstacle_grid_lookup(G, q, &v, g) == GRID_INSIDE);
    q[a] = nextafter(0.0, -1.0);
    CHECK(obstacle_grid_lookup(G, q, &v, g) == GRID_OUTSIDE && v == INFINITY && g[0] == 0.0 && g[1] == 0.0 && g[2] == 0.0);
    q[a] = hi;
    CHECK(obstacle_grid_lookup(G, q, &v, g) == GRID_INSIDE && isfinite(v));
    q[a] = nextafter(hi, 10.0);
    CHECK(obstacle_grid_lookup(G, q, &v, g) == GRID_OUTSIDE && v == INFINITY);
    q[a] = INFINITY;
    CHECK(obstacle_grid_lookup(G, q, &v, g) == GRID_OUTSIDE);
    q[a] = -INFINITY;
    CHECK(obstacle_grid_lookup(G, q, &v, g) == GRID_OUTSIDE);
  }
}

static void test_rules() {
  const double o[3] = {0.0, -1.0, 2.0};
  const int32_t ok[3] = {2, 256, 7};
  CHECK(obstacle_grid_shape_ok(ok, o, 0.1, DDP_HIP_MAX_GRID_DIM));
  for (int a = 0; a < 3; ++a) {
    int32_t d[3] = {2, 256, 7};
    d[a] = 1;
    CHECK(!obstacle_grid_shape_ok(d, o, 0.1, DDP_HIP_MAX_GRID_DIM));
    d[a] = 257;
    CHECK(!obstacle_grid_shape_ok(d, o, 0.1, DDP_HIP_MAX_GRID_DIM));
    double ob[3] = {0.0, -1.0, 2.0};
    ob[a] = NAN;
    CHECK(!obstacle_grid_shape_ok(ok, ob, 0.1, DDP_HIP_MAX_GRID_DIM));
    ob[a] = INFINITY;
    CHECK(!obstacle_grid_shape_ok(ok, ob, 0.1, DDP_HIP_MAX_GRID_DIM));
  }
  for (double cell : {0.0, -0.1, (double)NAN, (double)INFINITY}) CHECK(!obstacle_grid_shape_ok(ok, o, cell, DDP_HIP_MAX_GRID_DIM));
  // the field: the surface halfway between two centres; no source reads as cap; the largest grid stays below the sentinel
  const int32_t n[3] = {7, 5, 9};
  CHECK(obstacle_grid_cap(n) == 49 + 25 + 81);
  CHECK(obstacle_grid_phi(false, 1, 155, 0.5) == 0.25 && obstacle_grid_phi(true, 1, 155, 0.5) == -0.25);
  CHECK(obstacle_grid_phi(false, 4, 155, 0.5) == 0.75 && obstacle_grid_phi(true, 9, 155, 2.0) == -5.0);
  CHECK(obstacle_grid_phi(false, GRID_EDT_BIG + 12, 155, 1.0) == sqrt(155.0) - 0.5);
  const int32_t big[3] = {256, 256, 256};
  CHECK(obstacle_grid_cap(big) < GRID_EDT_BIG && (int64_t)GRID_EDT_BIG + 3 * 262 * 262 < INT32_MAX);
}

// cost_obstacle_geom_side with the new kind: a grid slot's four doubles are finite, nothing more
static void test_geom_side() {
  const int32_t kinds[4] = {DDP_HIP_OBSTACLE_SPHERE, DDP_HIP_OBSTACLE_GRID, DDP_HIP_OBSTACLE_HALFSPACE, DDP_HIP_OBSTACLE_GRID};
  CostCheck c;
  c.items = 4;
  c.kind = kinds;
  std::vector<double> g = {0.0, 0.0, 0.0, 0.1,    3.0, -4.0, 0.0, -0.25,    0.6, 0.0, 0.8, -3.0,    0.0, 0.0, 0.0, 0.0,
                           1.0, 2.0, 3.0, 0.0,    0.1, 0.2, 0.3, 5.0,       0.0, 1.0, 0.0, 2.0,     -7.0, 0.0, 9.0, -1e-3};
  CHECK(cost_obstacle_geom_side(c, g.data(), (int64_t)g.size()));        // a shift of any length, a margin of either sign
  for (int i : {4, 5, 6, 7, 28, 31})
    for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY}) {
      std::vector<double> b = g;
      b[i] = bad;
      CHECK(!cost_obstacle_geom_side(c, b.data(), (int64_t)b.size()));
    }
  std::vector<double> b = g;
  b[3] = -0.1;                                                           // the sphere's radius rule still holds beside a grid slot
  CHECK(!cost_obstacle_geom_side(c, b.data(), (int64_t)b.size()));
  b = g;
  b[8] = 0.7;                                                            // ... and the half-space's unit normal
  CHECK(!cost_obstacle_geom_side(c, b.data(), (int64_t)b.size()));
  CHECK(DDP_HIP_OBSTACLE_GRID == 2 && DDP_HIP_MAX_GRID_DIM == 256);
}

int main() {
  test_cube();
  test_box();
  test_rules();
  test_geom_side();
  if (g_fail) { printf("%d check(s) failed\n", g_fail); return 1; }
  printf("obstacle grid block ok\n");
  return 0;
}
