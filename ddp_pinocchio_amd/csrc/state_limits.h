// state_limits.h -- per-instance soft state limits (DDP_HIP_FLAG_STATE_LIMITS, ddp_hip.h): the kernel-side description and the
// one term every kernel forms the same way.  The terms are added in fwd.hip (cost values) and lin.hip (derivatives).
#pragma once
#include "internal.h"

// What a kernel reads of the context's state limits: three arrays [batch][T+1][n] over the tangent rows (n = 2 nv).
// weight == nullptr: no terms (the flag is off, or no non-zero weight is resident: CostBlock::live)
struct StateLimitsDev {
  const double *lo, *hi, *weight;
};

inline StateLimitsDev state_limits_dev(const ddp_hip_ctx* ctx) {
  StateLimitsDev s{};
  const CostBlock& k = ctx->cost[COST_LIMITS];
  if (k.live) { s.lo = k.side[0]; s.hi = k.side[1]; s.weight = k.side[2]; }
  return s;
}

// index in x of the state coordinate of tangent row i (fwd.hip: track_state_sum's plain rows); nq = nv + 1 on a free flyer
__device__ __forceinline__ int limit_coord(int i, int nv, int nq) { return i < nv ? i + nq - nv : nq + i - nv; }

// e = s - lo below the interval, s - hi above it, 0 inside (and for a NaN)
__device__ __forceinline__ double limit_excess(double s, double lo, double hi) { return s < lo ? s - lo : (s > hi ? s - hi : 0.0); }
