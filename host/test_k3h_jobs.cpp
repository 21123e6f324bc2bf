// K3h's job lists (csrc/bwd_jobs.h) at the Talos shape, on the host: every needed column of the symmetric tensors rides in
// exactly one run of one unit, nothing else does, and the full units are full.  No HIP, no device.
#include <stdio.h>

#include <map>
#include <tuple>
#include <vector>

#include "../ddp_pinocchio_amd/csrc/bwd_jobs.h"

static int failures = 0;
static bool quiet = false;   // (while the checker is tried on a list that is wrong on purpose)
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) { if (!quiet) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

struct Stats {
  int units = 0, filled = 0, max_cols = 0, max_runs = 0;
};

// needed: f_xx (c, j >= c), f_ux (c, every j), f_uu (c, j >= c)
static bool needed(int tensor, int slab, int j, int n, int m) {
  if (tensor == K3H_FXX) return slab >= 0 && slab < n && j >= slab && j < n;
  if (tensor == K3H_FUX) return slab >= 0 && slab < n && j >= 0 && j < m;
  if (tensor == K3H_FUU) return slab >= 0 && slab < m && j >= slab && j < m;
  return false;
}

// every needed column exactly once, no other column; per-unit limits
static Stats check_units(const std::vector<K3hUnit>& us, int n, int m) {
  Stats st;
  std::map<std::tuple<int, int, int>, int> seen;
  for (const K3hUnit& un : us) {
    const int cols = k3h_unit_columns(un);
    if (cols == 0) continue;                     // (the filler of the last job)
    ++st.units;
    st.filled += cols;
    if (cols > st.max_cols) st.max_cols = cols;
    int runs = 0;
    for (const K3hRun& r : un.run) {
      if (r.cnt > 0) ++runs;
      for (int j = r.j0; j < r.j0 + r.cnt; ++j) {
        CHECK(needed(r.tensor, r.slab, j, n, m));
        ++seen[std::make_tuple((int)r.tensor, (int)r.slab, j)];
      }
    }
    if (runs > st.max_runs) st.max_runs = runs;
    // the kernel's lookup: slot jj of the unit is the jj-th column of the runs in order, and the slots past the last are empty
    int jj = 0;
    for (const K3hRun& r : un.run)
      for (int j = r.j0; j < r.j0 + r.cnt; ++j, ++jj) {
        const K3hCol c = k3h_col(un, jj);
        CHECK(c.need && c.tensor == r.tensor && c.slab == r.slab && c.j == j);
      }
    for (; jj < n; ++jj) CHECK(!k3h_col(un, jj).need);
  }
  int want = 0;
  for (int tensor = K3H_FXX; tensor <= K3H_FUU; ++tensor)
    for (int slab = 0; slab < n; ++slab)
      for (int j = 0; j < n; ++j)
        if (needed(tensor, slab, j, n, m)) {
          ++want;
          const auto it = seen.find(std::make_tuple(tensor, slab, j));
          CHECK(it != seen.end() && it->second == 1);
        }
  CHECK((int)seen.size() == want);
  CHECK(st.filled == want);
  return st;
}

int main() {
  const int n = 76, m = 38;
  const int needed_cols = n * (n + 1) / 2 + n * m + m * (m + 1) / 2;
  CHECK(needed_cols == 6555);
  static_assert(K3H_UNITS_PER_JOB == 3 || K3H_UNITS_PER_JOB == 4, "units per job");
  static_assert(K3H_UNITS_PER_JOB * 76 <= 512, "one output entry per lane");

  // the full units
  std::vector<K3hUnit> us = k3h_full_units(n, m);
  CHECK(k3h_units_in_bounds(us, n, m));
  const int real_units = (int)us.size();
  const int njobs = k3h_pad_to_jobs(us, K3H_UNITS_PER_JOB);
  CHECK((int)us.size() == njobs * K3H_UNITS_PER_JOB);                     // every job has the compiled number of units at most
  CHECK(njobs == (real_units + K3H_UNITS_PER_JOB - 1) / K3H_UNITS_PER_JOB);
  CHECK(k3h_units_in_bounds(us, n, m));
  const Stats full = check_units(us, n, m);
  CHECK(full.units == real_units);
  CHECK(full.max_cols <= n);
  CHECK(full.max_runs <= K3H_RUNS && K3H_RUNS == 4);
  CHECK(full.filled == needed_cols);
  CHECK(full.units == 87);
  CHECK(K3H_UNITS_PER_JOB != 3 || njobs == 29);
  CHECK((double)full.filled >= 0.95 * (double)(full.units * n));
  printf("full units: %d units in %d jobs of %d, %d of %d slots filled (%.3f)\n", full.units, njobs, K3H_UNITS_PER_JOB, full.filled,
         full.units * n, (double)full.filled / (double)(full.units * n));

  // the column jobs through the same checker
  const std::vector<BwdJob> jh = k3h_column_jobs(n, m);
  std::vector<K3hUnit> cu;
  int max_units = 0;
  for (const BwdJob& job : jh) {
    const std::vector<K3hUnit> ju = k3h_column_job_units(job, n, m);
    if ((int)ju.size() > max_units) max_units = (int)ju.size();
    cu.insert(cu.end(), ju.begin(), ju.end());
  }
  CHECK(jh.size() == 45);
  CHECK(max_units == 3);
  const Stats col = check_units(cu, n, m);
  CHECK(col.units == 133);
  CHECK(col.filled == needed_cols);
  CHECK(col.max_cols <= n && col.max_runs <= K3H_RUNS);
  printf("column jobs: %d units in %d jobs, %d of %d slots filled (%.3f)\n", col.units, (int)jh.size(), col.filled, col.units * n,
         (double)col.filled / (double)(col.units * n));

  // the checker itself: a list with a column twice, one with a column missing and one out of its slab are caught
  {
    std::vector<K3hUnit> bad = k3h_full_units(n, m);
    bad[1].run[1].slab = 0;                                                // an f_xx tail moved to slab 0: doubled there, missing here
    const int before = failures;
    quiet = true;
    check_units(bad, n, m);
    quiet = false;
    const bool caught = failures > before;
    failures = before;
    CHECK(caught);
    bad = k3h_full_units(n, m);
    bad[0].run[0].cnt = (int16_t)(n + 1);
    CHECK(!k3h_units_in_bounds(bad, n, m));
  }

  if (failures) { printf("%d check(s) failed\n", failures); return 1; }
  printf("k3h jobs ok\n");
  return 0;
}
