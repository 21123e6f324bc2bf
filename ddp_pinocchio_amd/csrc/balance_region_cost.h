// balance_region_cost.h -- per-instance balance-region costs (DDP_HIP_FLAG_BALANCE_REGION_COST, ddp_hip.h): one-sided half-plane
// penalties on xi = c + tau cdot, the CoM or the capture point.  The kernel-side description and the device pieces; the terms
// themselves are formed by kernels of their own in fwd.hip (cost values: balance_region_cost_kernel, summed by com_sum_kernel;
// margins: balance_region_margin_kernel) and lin.hip (derivatives: lin_balance_region_cost_kernel); model_api.hip evaluates one
// state with the same code.  Built on com_cost.h (c, Jc) and on momentum_cost.h with ang = false (cdot = l / M and its q
// jacobian): no inertia and no angular momentum is formed.  Both share the momentum's staged record, MomWaveLds: its stage lane
// leaves the records the CoM lanes read (jw, m, mp), so one walk per joint serves both.
#pragma once
#include <stddef.h>

#include "com_cost.h"
#include "internal.h"
#include "momentum_cost.h"
#include "obstacle_cost.h"

// What a kernel reads of the context's balance-region cost.  geom == nullptr: no terms (the flag is off, no planes are set, or no
// non-zero weight has been uploaded: the block's CostBlock::live)
struct BalanceRegionDev {
  const double *geom, *weight;     // [batch][T+1][np][5] = (n, h, tau), [batch][T+1][np]
  int32_t np;                      // plane slots
};

// always: the description whether or not a weight is live (ddp_hip_balance_region_margin works from the first set_planes on)
inline BalanceRegionDev balance_region_dev(const ddp_hip_ctx* ctx, bool always = false) {
  BalanceRegionDev c{};
  const CostBlock& k = ctx->cost[COST_BALANCE_REGION];
  if (!(always ? ctx->br_np > 0 : k.live)) return c;
  c.geom = k.side[0];
  c.weight = k.side[1];
  c.np = ctx->br_np;
  return c;
}

namespace rbd {

// some live plane (w != 0) of the np slots tests a point that moves with v: cdot has to be formed
__device__ __forceinline__ bool region_needs_rate(const double* geom, const double* w, int np) {
  for (int o = 0; o < np; ++o)
    if (w[o] != 0.0 && geom[5 * o + 4] != 0.0) return true;
  return false;
}

// d = n . xi - h of the plane g = (n, h, tau) at xi = c + tau cdot; with tau = 0 xi is c itself and cd is not read
__device__ __forceinline__ double region_distance(const double* g, const double* c, const double* cd) {
  double xi[3] = {c[0], c[1], c[2]};
  const double tau = g[4];
  if (tau != 0.0) { xi[0] = c[0] + tau * cd[0]; xi[1] = c[1] + tau * cd[1]; xi[2] = c[2] + tau * cd[2]; }
  return (g[0] * xi[0] + g[1] * xi[1] + g[2] * xi[2]) - g[3];
}

// c and, with `rate`, cdot from the nj body records rec[7 j ..] = m_j | m_j p_j | m_j pdot_j (rbd::momentum_body with ang = false),
// joints in ascending order: the one order in which every kernel forms the sums
__device__ __forceinline__ void region_fold(const double* rec, int nj, bool rate, double* c, double* cd) {
  double M = 0.0, s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < nj; ++i) {
    M += rec[7 * i];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += rec[7 * i + 1 + k];
    if (rate) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s[3 + k] += rec[7 * i + 4 + k];
    }
  }
  c[0] = s[0] / M; c[1] = s[1] / M; c[2] = s[2] / M;
  if (rate) { cd[0] = s[3] / M; cd[1] = s[4] / M; cd[2] = s[5] / M; }
}

// What the lanes of one wave leave each other for the derivatives at one state.  mo is the momentum's record: with ang = false its
// IO and the angular halves of sv, V, hb and A stay unused -- the price of sharing its lanes as they are.  z_o of the active planes
// (2 nv doubles each: the q part, then at nv the v part) gets no room of its own: once the column lanes are through, IO, sv and V
// are dead, and the three arrays, which follow each other in the record, hold the eight rows (region_z)
struct BalanceWaveLds {
  MomWaveLds mo;                                       // jw, m, mp (the CoM's records too); sv, V, hb, A[0][0] = dl/d(delta q), h = l
  double J[3 * DDP_MAXJ];                              // Jc, stored at J[3 * column + row] (CoMWaveLds::J)
  double c[3];                                         // c(q)
  double w[DDP_HIP_MAX_REGION_PLANES], we[DDP_HIP_MAX_REGION_PLANES], tau[DDP_HIP_MAX_REGION_PLANES];   // w_o, w_o e_o, tau_o
  int act[DDP_HIP_MAX_REGION_PLANES];                  // w != 0 and e != 0
};
static_assert(offsetof(MomWaveLds, sv) == offsetof(MomWaveLds, IO) + sizeof(double) * 6 * DDP_MAXJ &&
                  offsetof(MomWaveLds, V) == offsetof(MomWaveLds, sv) + sizeof(double) * 6 * DDP_MAXJ,
              "region_z: IO, sv and V are one run of 18 DDP_MAXJ doubles");
static_assert(DDP_HIP_MAX_REGION_PLANES * 2 * DDP_MAXJ <= 18 * DDP_MAXJ, "region_z: the rows fit that run");

// Row o of z.  Valid from the barrier behind the column lanes on (region_columns_wave): nothing reads IO, sv or V after it
__device__ __forceinline__ double* region_z(BalanceWaveLds& S, int o) { return &S.mo.IO[0][0] + o * 2 * DDP_MAXJ; }
__device__ __forceinline__ const double* region_z(const BalanceWaveLds& S, int o) { return &S.mo.IO[0][0] + o * 2 * DDP_MAXJ; }

// The total mass, the records in ascending order (as com_column_lane and mom_column_lane form it)
__device__ __forceinline__ double region_total_mass(const BalanceWaveLds& S, int nj) {
  double M = 0.0;
  for (int i = 0; i < nj; ++i) M += S.mo.m[i];
  return M;
}

// Step 1: the staged records by one wave (lane tid), barriers included.  Without `rate` the CoM's stage lane alone (v is not
// read); with it the momentum's stage and prefix lanes, ang = false, whose m and mp are the CoM's
__device__ __forceinline__ void region_stage_wave(const DevModel& m, const double* q, const double* v, int tid, bool rate, BalanceWaveLds& S) {
  if (tid < m.nj) {
    if (rate) mom_stage_lane(m, q, v, tid, false, S.mo);
    else com_stage_lane(m, q, tid, S.mo.jw, S.mo.m, S.mo.mp);
  }
  __syncthreads();
  if (!rate) return;
  if (tid < m.nj) mom_prefix_lane(tid, false, S.mo);
  __syncthreads();
}

// c and, with `rate`, cdot = l / M from the staged records, ascending (what com_column_lane leaves in c and mom_column_lane in h)
__device__ __forceinline__ void region_point_lds(const BalanceWaveLds& S, int nj, bool rate, double* c, double* cd) {
  double M = 0.0, s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < nj; ++i) {
    M += S.mo.m[i];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += S.mo.mp[i][k];
    if (rate) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s[3 + k] += S.mo.hb[i][k];
    }
  }
  c[0] = s[0] / M; c[1] = s[1] / M; c[2] = s[2] / M;
  if (rate) { cd[0] = s[3] / M; cd[1] = s[4] / M; cd[2] = s[5] / M; }
}

// Step 2: Jc and c by the CoM's column lane and, with `rate_q`, dl/d(delta q) (and dl/dv, unused) by the momentum's, ang = false.
// (Barrier included.)
__device__ __forceinline__ void region_columns_wave(const DevModel& m, int tid, bool rate_q, BalanceWaveLds& S) {
  if (tid < m.nj) {
    com_column_lane(m, tid, S.mo.jw, S.mo.m, S.mo.mp, S.J, S.c);
    if (rate_q) mom_column_lane(m, tid, false, S.mo);
  }
  __syncthreads();
}

// Entry (row a, tangent column i) of d cdot / d(delta q): the momentum's dl/dq entry divided by M.  A free-flyer root's three
// linear columns are identically zero and not formed: the caller leaves them out
__device__ __forceinline__ bool region_rate_column(const DevModel& m, int i) { return !(m.ff != 0 && i < 3); }

// Step 3: z_o of the active planes (ddp_hip.h: Jc . n first, then + tau (dcq . n); the v part tau (Jc . n), with tau != 0 alone)
__device__ __forceinline__ void region_stage_z(const DevModel& m, const double* geom, int np, int tid, int nt, BalanceWaveLds& S) {
  const int nv = m.nv;
  const double M = region_total_mass(S, m.nj);
  for (int e = tid; e < np * nv; e += nt) {
    const int o = e / nv, i = e % nv;
    if (!S.act[o]) continue;
    const double* g = geom + 5 * o;
    const double tau = g[4];
    const double jn = dot3(S.J + 3 * i, g);
    double zq = jn;
    if (tau != 0.0) {
      if (region_rate_column(m, i)) {
        const double* A = S.mo.A[0][0][i];
        const double dq[3] = {A[0] / M, A[1] / M, A[2] / M};
        zq = jn + tau * dot3(dq, g);
      }
      region_z(S, o)[nv + i] = tau * jn;
    }
    region_z(S, o)[i] = zq;
  }
}

// Step 4: the wave (lane tid of nt) adds gx[i] += sum_o (w e)_o z_o[i] and gxx[i][j] += sum_o (z_o[min] w_o) z_o[max] over the
// active planes in ascending order, entry (i, j) in (min, max) order: symmetric bit for bit.  A plane with tau = 0 takes no part
// in a v row or column; an entry no active plane reaches is not written
__device__ __forceinline__ void region_add_wave(const BalanceWaveLds& S, int np, int nv, int tid, int nt, int n, double* gx, double* gxx) {
  for (int i = tid; i < n; i += nt) {
    double s = 0.0;
    bool hit = false;
    for (int o = 0; o < np; ++o) {
      if (!S.act[o] || (i >= nv && S.tau[o] == 0.0)) continue;
      s += S.we[o] * region_z(S, o)[i];
      hit = true;
    }
    if (hit) gx[i] += s;
  }
  for (int e = tid; e < n * n; e += nt) {
    const int i = e % n, j = e / n;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    double h = 0.0;
    bool hit = false;
    for (int o = 0; o < np; ++o) {
      if (!S.act[o] || (hi >= nv && S.tau[o] == 0.0)) continue;
      h += region_z(S, o)[lo] * S.w[o] * region_z(S, o)[hi];
      hit = true;
    }
    if (hit) gxx[i + (int64_t)j * n] += h;
  }
}

}  // namespace rbd
