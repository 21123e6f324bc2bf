// bwd_jobs.h -- the job lists of the backward sweep's tensor stream (K3 / K3h, bwd_split.h), built on the host.  Plain C++: no
// HIP, no device (host/test_k3h_jobs.cpp checks the lists without either).
//
// K3h streams the symmetric tensors of one (instance, t) in UNITS of at most N column slots: a workgroup loads its units, reduces
// each (one barrier, M / 2 dependent adds per column) and adds one contraction per lane to Q.  Of slab c of f_xx / f_uu only the
// columns j >= c are needed, so a unit that is "slab c" (the column jobs below) spends its slot, its barrier and its reduction on
// N - c columns.  The full units pair the tails of two slabs whose lengths add up to N (or M), so that every unit but one is full:
// at (76, 38) 6 555 needed columns ride in 87 units instead of 133.
#pragma once

#include <stdint.h>

#include <vector>

#ifdef __HIPCC__
#define K3H_HD __host__ __device__ inline
#else
#define K3H_HD inline
#endif

struct BwdJob {
  int32_t kind;   // 0: x-columns (Q_xx, Q_ux, Q_x), 1: u-columns (Q_uu, Q_u); 2, 10, 11: bwd_split.h
  int32_t c0, cn;
  int32_t pad_;
};

// units a K3h workgroup takes (3 or 4: one output entry per lane needs K3H_UNITS_PER_JOB * N <= 512 lanes)
#ifndef K3H_UNITS_PER_JOB
#define K3H_UNITS_PER_JOB 3
#endif
constexpr int K3H_RUNS = 4;
enum : int16_t { K3H_FXX = 0, K3H_FUX = 1, K3H_FUU = 2 };

// cnt consecutive columns j0 .. j0 + cnt - 1 of one slab: in the packed layout one contiguous piece of records, (nv + 2) doubles
// each, slab_base + j0 (nv + 2) doubles on
struct K3hRun {
  int16_t tensor, slab, j0, cnt;
};
// the column slots of a unit, in order: run 0's columns, then run 1's, ...; an unused run has cnt 0
struct K3hUnit {
  K3hRun run[K3H_RUNS];
};

struct K3hCol {
  int tensor, slab, j;
  bool need;   // the slot holds a column at all
};
// column slot jj of a unit: which run it falls in
K3H_HD K3hCol k3h_col(const K3hUnit& un, int jj) {
  const int s1 = un.run[0].cnt, s2 = s1 + un.run[1].cnt, s3 = s2 + un.run[2].cnt, s4 = s3 + un.run[3].cnt;
  const int k = (jj >= s1) + (jj >= s2) + (jj >= s3);
  const K3hRun r = k == 0 ? un.run[0] : k == 1 ? un.run[1] : k == 2 ? un.run[2] : un.run[3];
  const int s = k == 0 ? 0 : k == 1 ? s1 : k == 2 ? s2 : s3;
  return K3hCol{r.tensor, r.slab, r.j0 + (jj - s), jj < s4};
}
K3H_HD int k3h_unit_columns(const K3hUnit& un) { return un.run[0].cnt + un.run[1].cnt + un.run[2].cnt + un.run[3].cnt; }

// The column jobs (the strided K3h, and the packed one under DDP_HIP_K3H_COLUMN_JOBS): x-columns in pairs (kind 10: f_xx slab c0 |
// f_xx slab c0 + 1 | f_ux slabs c0, c0 + 1), u-columns in groups of 6 (kind 11: f_uu slabs in pairs), the rest in one
inline std::vector<BwdJob> k3h_column_jobs(int n, int m) {
  std::vector<BwdJob> jh;
  for (int c = 0; c < n; c += 2) jh.push_back(BwdJob{10, c, 2, 0});
  for (int c = 0; c < m; c += 6) jh.push_back(BwdJob{11, c, (m - c) < 6 ? (m - c) : 6, 0});
  return jh;
}
// ... and what their units hold, as runs of needed columns (for the checker: the kernel works the slots out itself)
inline std::vector<K3hUnit> k3h_column_job_units(const BwdJob& job, int n, int m) {
  std::vector<K3hUnit> us;
  auto tail = [](int16_t tensor, int c, int len) { return K3hRun{tensor, (int16_t)c, (int16_t)c, (int16_t)(len - c)}; };
  const int c0 = job.c0;
  if (job.kind == 10) {
    us.push_back(K3hUnit{{tail(K3H_FXX, c0, n), {}, {}, {}}});
    us.push_back(K3hUnit{{tail(K3H_FXX, c0 + 1, n), {}, {}, {}}});
    us.push_back(K3hUnit{{K3hRun{K3H_FUX, (int16_t)c0, 0, (int16_t)m}, K3hRun{K3H_FUX, (int16_t)(c0 + 1), 0, (int16_t)m}, {}, {}}});
  } else {
    for (int u = 0; u < job.cn / 2; ++u) us.push_back(K3hUnit{{tail(K3H_FUU, c0 + 2 * u, m), tail(K3H_FUU, c0 + 2 * u + 1, m), {}, {}}});
  }
  return us;
}

// The full units (n = 2 m, m even): a tail of n - c columns and one of c columns make n.
//   f_xx: slab 0 alone; slabs c and n - c, c = 1 .. m - 1; slab m alone (m columns)
//   f_ux: slabs 2 k and 2 k + 1 (every column of both)
//   f_uu: slabs c and m - c, c = 1 .. m / 2 - 1, make m columns: two such pairs per unit; slabs 0 and m / 2 together
inline std::vector<K3hUnit> k3h_full_units(int n, int m) {
  std::vector<K3hUnit> us;
  auto tail = [](int16_t tensor, int c, int len) { return K3hRun{tensor, (int16_t)c, (int16_t)c, (int16_t)(len - c)}; };
  us.push_back(K3hUnit{{tail(K3H_FXX, 0, n), {}, {}, {}}});
  for (int c = 1; c < m; ++c) us.push_back(K3hUnit{{tail(K3H_FXX, c, n), tail(K3H_FXX, n - c, n), {}, {}}});
  us.push_back(K3hUnit{{tail(K3H_FXX, m, n), {}, {}, {}}});
  for (int c = 0; c < n; c += 2) us.push_back(K3hUnit{{K3hRun{K3H_FUX, (int16_t)c, 0, (int16_t)m}, K3hRun{K3H_FUX, (int16_t)(c + 1), 0, (int16_t)m}, {}, {}}});
  for (int c = 1; c < m / 2; c += 2) {
    K3hUnit un{{tail(K3H_FUU, c, m), tail(K3H_FUU, m - c, m), {}, {}}};
    if (c + 1 < m / 2) { un.run[2] = tail(K3H_FUU, c + 1, m); un.run[3] = tail(K3H_FUU, m - c - 1, m); }
    us.push_back(un);
  }
  us.push_back(K3hUnit{{tail(K3H_FUU, 0, m), tail(K3H_FUU, m / 2, m), {}, {}}});
  return us;
}

// What the kernel relies on, checked before a list is uploaded: every run lies inside its slab (so every record read lies inside
// the tensor), a unit has at most n columns, unused runs are all zeros
inline bool k3h_units_in_bounds(const std::vector<K3hUnit>& us, int n, int m) {
  for (const K3hUnit& un : us) {
    if (k3h_unit_columns(un) > n) return false;
    for (const K3hRun& r : un.run) {
      if (r.cnt < 0 || r.j0 < 0 || r.slab < 0 || r.tensor < K3H_FXX || r.tensor > K3H_FUU) return false;
      if (r.cnt == 0) { if (r.tensor || r.slab || r.j0) return false; continue; }
      const int slabs = r.tensor == K3H_FUU ? m : n, cols = r.tensor == K3H_FXX ? n : m;
      if (r.slab >= slabs || r.j0 + r.cnt > cols) return false;
    }
  }
  return true;
}

// the list a launch of (jobs, batch) workgroups walks: K3H_UNITS_PER_JOB units per job, the last job filled up with empty units
inline int k3h_pad_to_jobs(std::vector<K3hUnit>& us, int units_per_job) {
  while (us.size() % (size_t)units_per_job) us.push_back(K3hUnit{});
  return (int)(us.size() / (size_t)units_per_job);
}
