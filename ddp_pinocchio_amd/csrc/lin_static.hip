// lin_static.hip -- second-order finite differences (finite_diff_hessian_compute mode 2, problem.hpp:152-298) for
// trees whose TOPOLOGY is known at compile time.
//
// The generic kernels of lin.hip keep the per-joint state of an evaluation in private arrays indexed by run-time
// joint / slot numbers; those arrays live in scratch (HBM-backed) and their traffic is what bounds the stencil
// (profiles/: 39 KB written per evaluation at the Talos size).  Here the parent table is a template parameter: every
// loop over the joints is expanded at compile time, every index is a constant and the running state of an
// evaluation lives in registers.  One wave = 64 stencil points that share their configuration q (and, at the
// torque level, their velocity): what the articulated-body algorithm derives from q (and v) alone is read from the
// q- / v-caches -- wave-uniform blocks, copied into LDS with every load in flight and read as broadcasts by the row and
// pair kernels of the velocity and torque levels and by the first order's u waves, walked through the scalar path by
// the first order's q and v waves -- and each lane only carries what its own perturbation changes.  The arithmetic is the operation sequence of
// rbd::aba_u_cached / rbd::aba_vu_cached.
#include <float.h>
#include <math.h>
#include <stdlib.h>

#include <type_traits>
#include <utility>

#include "internal.h"
#include "lin_common.h"
#include "rbd.h"

#ifndef DEV_NO_EMIT
#define DEV_NO_EMIT 0
#endif
namespace {

// ---- compiled-in topologies -------------------------------------------------------------------------------------
// Talos-like humanoid (models.cpp:build_tree38): floating base as 3 prismatic + 3 revolute joints, two 6-joint legs,
// a 2-joint torso, two 8-joint arms, a 2-joint head
struct TopoTalos38 {
  static constexpr int N = 38;
  static constexpr int parent[N] = {-1, 0, 1, 2, 3, 4,            // base
                                    5, 6, 7, 8, 9, 10,            // left leg
                                    5, 12, 13, 14, 15, 16,        // right leg
                                    5, 18,                        // torso
                                    19, 20, 21, 22, 23, 24, 25, 26,   // left arm
                                    19, 28, 29, 30, 31, 32, 33, 34,   // right arm
                                    19, 36};                      // head
  static constexpr int prismatic[N] = {1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                       0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};

// UR5-like serial arm (models.cpp:build_chain6; test/pinocchio_ddp.cpp shape): one chain of six revolute joints
struct TopoChain6 {
  static constexpr int N = 6;
  static constexpr int parent[N] = {-1, 0, 1, 2, 3, 4};
  static constexpr int prismatic[N] = {0, 0, 0, 0, 0, 0};
};

}  // namespace
#include "topo_extra.h"     // generated topologies (tools/gen_topology.py): struct Topo<Name> ..., DDP_TOPO_EXTRA(X)
namespace {

template <class T> constexpr bool has_child(int k) {
  for (int c = k + 1; c < T::N; ++c) if (T::parent[c] == k) return true;
  return false;
}
template <class T> constexpr int largest_child(int k) {
  int r = -1;
  for (int c = k + 1; c < T::N; ++c) if (T::parent[c] == k) r = c;
  return r;
}
// the largest-index child of its parent contributes first in the leaf -> root pass
template <class T> constexpr bool first_contrib(int k) { return T::parent[k] >= 0 && largest_child<T>(T::parent[k]) == k; }

template <class T>
bool topo_matches(const DevModel& m) {
  if (m.kind != DDP_HIP_MODEL_TREE || m.nv != T::N) return false;
  for (int i = 0; i < T::N; ++i)
    if (m.parent[i] != T::parent[i] || (m.jtype[i] == DDP_HIP_JOINT_PRISMATIC) != (T::prismatic[i] != 0)) return false;
  return true;
}

// ---- the q-cache as a base block and deltas (LinPlan::qc_sparse) ---------------------------------------------------------
// In the local-frame ABA, record K of configuration 1+g (q_g stepped) differs from the base record in E | r (12 words) if
// K == g, and in U | 1/D | Ia (28 words) if K is a strict ancestor of g; everything else is the base record bit for bit
// ("configuration level by splice" below).  Per (instance, t) the cache therefore holds
//   the base block        [N][QC_STRIDE]        at 0       configuration 0, the layout every base reader knows
//   the delta blocks      [N][12 + MAXD * 28]   at DELTA   of stepped joint g: E | r of g at q_g + eps, then U | 1/D | Ia of g's
//                                                          strict ancestors at configuration 1+g, root first (by depth)
// (padded to the deepest joint's depth: 143 KB per (instance, t) for the Talos-like tree, base block included, against 474 KB
// for its 39 whole blocks)
template <class T>
struct QcLayout {
  static constexpr int N = T::N, ER = 12, UD = rbd::QC_STRIDE - ER;
  static constexpr int max_depth() {
    int best = 1;
    for (int k = 0; k < N; ++k) { int d = 0; for (int a = T::parent[k]; a >= 0; a = T::parent[a]) ++d; if (d > best) best = d; }
    return best;
  }
  static constexpr int MAXD = max_depth();
  static constexpr int DW = ER + MAXD * UD;                          // doubles per delta block
  static constexpr int DELTA = N * rbd::QC_STRIDE, WORDS = DELTA + N * DW;
  static constexpr int PATH0 = DELTA + ER;                           // path record (g, d) at PATH0 + g * DW + d * UD
};
// strict ancestors of every joint as bit masks (bit K of anc[g] <=> K is a strict ancestor of g): what a row wave selects by.
// The ancestors of a joint have smaller indices than it, so among the ancestors of g the one of depth d is the d-th set bit
template <class T> struct AncTab { unsigned long long anc[T::N]; };
template <class T> constexpr AncTab<T> make_anc_tab() {
  static_assert(T::N <= 64, "ancestor masks are 64 bits wide");
  AncTab<T> t{};
  for (int k = 0; k < T::N; ++k) for (int a = T::parent[k]; a >= 0; a = T::parent[a]) t.anc[k] |= 1ull << a;
  return t;
}
template <class T> __device__ const AncTab<T> g_anc_tab = make_anc_tab<T>();
// Where word e of joint K's record at configuration 1+g lives, counted from the (instance, t)'s q-cache (g = -1, anc = 0: the
// base configuration).  A blend of finished offsets by 0 / 1 weights: no control flow
template <class T>
__device__ __forceinline__ int qc_word(int g, unsigned long long anc, int K, int e) {
  using L = QcLayout<T>;
  const int d = __popcll(anc & ((1ull << K) - 1ull));                // depth of K, where K is an ancestor of g
  const int base = K * rbd::QC_STRIDE + e, own = L::DELTA + g * L::DW + e, path = L::PATH0 + g * L::DW + d * L::UD + (e - L::ER);
  const int w_own = (int)(e < L::ER) & (int)(K == g), w_path = (int)(e >= L::ER) & (int)((anc >> K) & 1ull);
  return base + w_own * (own - base) + w_path * (path - base);
}

// ---- the v-cache as base blocks and deltas (LinPlan::vc_sparse) ----------------------------------------------------------
// Of the v records (cb | pA0 | Ia cb), a q_g step changes those of g's strict ancestors (their Ia) and of g's subtree, g included
// (their link velocities); a v_g step those of g's subtree.  A subtree is one contiguous index range.  Per (instance, t), in records
// of VC_STRIDE doubles and packed exactly (no padding to the deepest joint):
//   entry 0               [N]                  at 0     the base (q, v), as the configuration fill writes it
//   the v-step base block [N]                  at VB    the unstepped point as the v-step fill's own instruction stream forms it
//   q-step deltas of g    [depth g + |sub g|]  at qoff[g]   strict ancestors root first (the popcount rule of qc_word), then the subtree
//   v-step deltas of g    [|sub g|]            at voff[g]   the subtree
// (165 KB per (instance, t) for the Talos-like tree against 421 KB for its 77 whole entries)
template <class T>
struct VcTab { int qoff[T::N], voff[T::N], sub[T::N]; int words; };   // offsets in doubles from the (instance, t)'s v-cache; subtree sizes
template <class T>
constexpr VcTab<T> make_vc_tab() {
  constexpr int N = T::N, R = rbd::VC_STRIDE;
  VcTab<T> t{};
  int depth[N] = {};
  for (int k = 0; k < N; ++k)
    for (int a = T::parent[k]; a >= 0; a = T::parent[a]) { ++depth[k]; ++t.sub[a]; }
  for (int k = 0; k < N; ++k) ++t.sub[k];          // the joint itself
  int off = 2 * N * R;
  for (int g = 0; g < N; ++g) { t.qoff[g] = off; off += (depth[g] + t.sub[g]) * R; }
  for (int g = 0; g < N; ++g) { t.voff[g] = off; off += t.sub[g] * R; }
  t.words = off;
  return t;
}
template <class T>
struct VcLayout {
  static constexpr int N = T::N, R = rbd::VC_STRIDE;
  static constexpr int VB = N * R;                                   // the v-step base block
  static constexpr int WORDS = make_vc_tab<T>().words;
};
template <class T> __device__ const VcTab<T> g_vc_tab = make_vc_tab<T>();
// Where word e of joint K's v record lives at the point a row reads, counted from the (instance, t)'s v-cache: kind 0, q_g stepped
// (g = -1, anc = 0: entry 0), anc the strict ancestors of g; kind 1, v_g stepped (anc is not looked at).  Like qc_word a blend of
// finished offsets by 0 / 1 weights
template <class T>
__device__ __forceinline__ int vc_word(int kind, int g, unsigned long long anc, int K, int e) {
  using L = VcLayout<T>;
  const VcTab<T>& tab = g_vc_tab<T>;
  const int gi = g < 0 ? 0 : g;
  const int nsub = g < 0 ? 0 : tab.sub[gi];
  const int off = kind ? tab.voff[gi] : tab.qoff[gi];
  const unsigned long long a = kind ? 0ull : anc;
  const int dg = __popcll(a), d = __popcll(a & ((1ull << K) - 1ull));      // depth of g; of K, where K is an ancestor of g
  const int base = kind * L::VB + K * L::R + e, below = off + (dg + K - g) * L::R + e, path = off + d * L::R + e;
  const int w_below = (int)(K >= g) & (int)(K < g + nsub), w_path = (int)((a >> K) & 1ull);
  return base + w_below * (below - base) + w_path * (path - base);
}
// ---- per-lane state ----------------------------------------------------------------------------------------------
template <class T>
struct TauState {
  double acc[T::N][6];   // leaf -> root: bias-force accumulators of the joints that have children; root -> leaf: accelerations
  double uu[T::N];       // u_i = tau_i - S_i^T pA_i, then the joint acceleration
};

// leaf -> root step of joint K for a new tau (rbd::aba_u_cached, first loop)
// qc: the (E | r | U | 1/D) part of the q-cache, QS doubles per joint (the cache itself, or a copy of it in LDS)
template <class T, int K, int QS>
__device__ __forceinline__ void tau_up(const DevModel& m, const double* __restrict__ qc, const double* __restrict__ vc,
                                       double tauK, TauState<T>& s) {
  constexpr int o = T::prismatic[K] ? 3 : 0;
  const double* E = qc + K * QS;
  const double* r = E + 9;
  const double* U = E + 12;
  const double dinv = E[18];
  const double* pA0 = vc + K * rbd::VC_STRIDE + 6;
  const double* Iac = vc + K * rbd::VC_STRIDE + 12;
  const double* a = m.axis[K];
  double pAi[6];
  if constexpr (has_child<T>(K)) {
#pragma unroll
    for (int k = 0; k < 6; ++k) pAi[k] = s.acc[K][k];
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) pAi[k] = pA0[k];
  }
  double sp = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) sp += a[k] * pAi[o + k];
  const double ui = tauK - sp;
  s.uu[K] = ui;
  constexpr int par = T::parent[K];
  if constexpr (par >= 0) {
    double pa[6], fp[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) pa[k] = pAi[k] + Iac[k] + U[k] * (ui * dinv);
    rbd::xform_force_T(E, r, pa, fp);
    if constexpr (first_contrib<T>(K)) {
      const double* pp0 = vc + par * rbd::VC_STRIDE + 6;
#pragma unroll
      for (int k = 0; k < 6; ++k) s.acc[par][k] = pp0[k] + fp[k];
    } else {
#pragma unroll
      for (int k = 0; k < 6; ++k) s.acc[par][k] += fp[k];
    }
  }
  if constexpr (QS == rbd::QC_STRIDE || (K % 2) == 0) __builtin_amdgcn_sched_barrier(0);   // keep the operand loads of the next joint out of this one: SGPRs would spill
}

// root -> leaf step of joint K (rbd::aba_u_cached, second loop); leaves the joint acceleration in uu[K]
template <class T, int K, int QS>
__device__ __forceinline__ void tau_down(const DevModel& m, const double* __restrict__ qc, const double* __restrict__ vc,
                                         TauState<T>& s) {
  constexpr int o = T::prismatic[K] ? 3 : 0;
  const double* E = qc + K * QS;
  const double* r = E + 9;
  const double* U = E + 12;
  const double dinv = E[18];
  const double* cb = vc + K * rbd::VC_STRIDE;
  double ap[6];
  constexpr int par = T::parent[K];
  if constexpr (par >= 0) rbd::xform_motion(E, r, s.acc[par], ap);
  else {
    const double a0[6] = {0, 0, 0, -m.gravity[0], -m.gravity[1], -m.gravity[2]};
    rbd::xform_motion(E, r, a0, ap);
  }
  double sum = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) { ap[k] += cb[k]; sum += U[k] * ap[k]; }
  const double qd = (s.uu[K] - sum) * dinv;
  s.uu[K] = qd;
  if constexpr (has_child<T>(K)) {
    const double* a = m.axis[K];
#pragma unroll
    for (int k = 0; k < 6; ++k) s.acc[K][k] = ap[k];
    s.acc[K][o] += a[0] * qd; s.acc[K][o + 1] += a[1] * qd; s.acc[K][o + 2] += a[2] * qd;
  }
  if constexpr (QS == rbd::QC_STRIDE || (K % 2) == 0) __builtin_amdgcn_sched_barrier(0);
}

template <class T, int QS, class TauFn, int... Ks>
__device__ __forceinline__ void tau_up_all(const DevModel& m, const double* __restrict__ qc, const double* __restrict__ vc, TauFn tau,
                                           TauState<T>& s, std::integer_sequence<int, Ks...>) {
  (tau_up<T, T::N - 1 - Ks, QS>(m, qc, vc, tau(T::N - 1 - Ks), s), ...);
}
// the joints HI, HI - 1, ..., LO of the leaf -> root pass
template <class T, int QS, int HI, class TauFn, int... Ks>
__device__ __forceinline__ void tau_up_range(const DevModel& m, const double* __restrict__ qc, const double* __restrict__ vc, TauFn tau,
                                             TauState<T>& s, std::integer_sequence<int, Ks...>) {
  (tau_up<T, HI - Ks, QS>(m, qc, vc, tau(HI - Ks), s), ...);
}
template <class T, int QS, int... Ks>
__device__ __forceinline__ void tau_down_all(const DevModel& m, const double* __restrict__ qc, const double* __restrict__ vc,
                                             TauState<T>& s, std::integer_sequence<int, Ks...>) {
  (tau_down<T, Ks, QS>(m, qc, vc, s), ...);
}

// copy of the (E | r | U | 1/D) part of a q-cache block in LDS, PS doubles per joint: the scalar path fills at about
// 2 bytes per clock and CU, so operands that both tree passes need are read from LDS instead (as broadcast reads)
constexpr int PS = 20;
template <int NV>
__device__ __forceinline__ void stage_placements(double* sp, const double* __restrict__ qc, int lane) {
  for (int idx = lane; idx < NV * 19; idx += LBS) {
    const int K = idx / 19, e = idx - K * 19;
    sp[K * PS + e] = qc[K * rbd::QC_STRIDE + e];
  }
}

template <class T> constexpr bool parents_at_least(int from, int lo) {
  for (int k = from; k < T::N; ++k) if (T::parent[k] < lo) return false;
  return true;
}
// where the two-phase staging of a row's operands splits the joints: the largest KH <= N / 2 such that the joints above KH
// only touch records KH .. N-1 (their own and their parents'); 19 for the Talos-like tree (its arms hang from joint 19),
// 0 (no second phase) for a tree whose upper half reaches back to the root
template <class T> constexpr int stage_split() {
  for (int kh = T::N / 2; kh > 0; --kh) if (parents_at_least<T>(kh + 1, kh)) return kh;
  return 0;
}

// Two-phase staging of a row's operands (E | r | U | 1/D from the q-cache block, the whole v-cache block): the records of the
// joints KH .. NV-1 -- where the leaf -> root pass starts -- are waited for and parked first; the loads of the joints 0 .. KH-1
// are issued at the same time, stay in flight (in registers) while the first half of the pass runs and are parked in front of
// the second half.  A row wave otherwise spends a quarter of its life waiting for its 17 KB of operands before it does anything.
template <int NV, int K0, int K1, bool WITH_V = true>
struct StageRegs {
  static constexpr int NPW = (K1 - K0) * 19, NVW = WITH_V ? (K1 - K0) * rbd::VC_STRIDE : 0;
  static constexpr int CP = (NPW + LBS - 1) / LBS, CV = (NVW + LBS - 1) / LBS;
  double rp[CP], rv[CV > 0 ? CV : 1];
  __device__ __forceinline__ void load(const double* __restrict__ qc, const double* __restrict__ vc, int lane) {
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      int idx = c * LBS + lane;
      idx = idx < NPW ? idx : NPW - 1;
      const int K = K0 + idx / 19, e = idx % 19;
      rp[c] = qc[K * rbd::QC_STRIDE + e];
    }
#pragma unroll
    for (int c = 0; c < CV; ++c) {
      int idx = c * LBS + lane;
      idx = idx < NVW ? idx : NVW - 1;
      rv[c] = vc[K0 * rbd::VC_STRIDE + idx];
    }
  }
  // the same words from the base + deltas layout: qc0 the (instance, t)'s q-cache, the row's configuration 1+g (qc_word)
  // VSP (LinPlan::vc_sparse): vc is the (instance, t)'s v-cache and the row's point is (vkind, vg) with the ancestors vanc
  // (vc_word); else vc is the row's whole entry
  template <class T, bool VSP>
  __device__ __forceinline__ void load_sparse(const double* __restrict__ qc0, int g, unsigned long long anc, const double* __restrict__ vc,
                                              int vkind, int vg, unsigned long long vanc, int lane) {
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      int idx = c * LBS + lane;
      idx = idx < NPW ? idx : NPW - 1;
      const int K = K0 + idx / 19, e = idx % 19;
      rp[c] = qc0[qc_word<T>(g, anc, K, e)];
    }
#pragma unroll
    for (int c = 0; c < CV; ++c) {
      int idx = c * LBS + lane;
      idx = idx < NVW ? idx : NVW - 1;
      if constexpr (VSP) {
        const int K = K0 + idx / rbd::VC_STRIDE, e = idx % rbd::VC_STRIDE;
        rv[c] = vc[vc_word<T>(vkind, vg, vanc, K, e)];
      } else {
        rv[c] = vc[K0 * rbd::VC_STRIDE + idx];
      }
    }
  }
  // (no branches: the lanes past the end store the last word again -- control flow in the middle of the evaluation would split
  // its basic block, and the optimiser then moves it away from its operand loads, see the notes on scalar-path hygiene)
  __device__ __forceinline__ void park(double* sp, double* sv, int lane) const {
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      int idx = c * LBS + lane;
      idx = idx < NPW ? idx : NPW - 1;
      const int K = K0 + idx / 19, e = idx % 19;
      sp[K * PS + e] = rp[c];
    }
#pragma unroll
    for (int c = 0; c < CV; ++c) {
      int idx = c * LBS + lane;
      idx = idx < NVW ? idx : NVW - 1;
      sv[K0 * rbd::VC_STRIDE + idx] = rv[c];
    }
  }
};

__device__ __forceinline__ void tri_index(int64_t q, int Wd, int& ii, int& jj) {   // q -> (ii, jj), ii < jj < Wd, row by row
  int a = (int)floor(((2.0 * Wd - 1.0) - sqrt((2.0 * Wd - 1.0) * (2.0 * Wd - 1.0) - 8.0 * (double)q)) * 0.5);
  if (a < 0) a = 0;
  while ((int64_t)a * (2 * Wd - a - 1) / 2 > q) --a;
  while ((int64_t)(a + 1) * (2 * Wd - a - 2) / 2 <= q) ++a;
  ii = a;
  jj = (int)(q - (int64_t)a * (2 * Wd - a - 1) / 2) + a + 1;
}

// Where row k of a tensor column lives, counted from the column's base: k in the contract layout; in a packed record
// (LinParams::pack: [top0, top1, rows NV .. n-1]) the rows k >= NV behind the two tops, row r0 -- the slab direction's
// configuration row -- at top0, and the one other configuration row a column can hold at top1.  rec_zero: the rows a packed
// column does not hold (exact zeros in the contract layout); with r0 = -1 all of its configuration rows (u directions).
// A reader asks rec_row for every row and lets rec_zero discard: for those rows rec_row names top1, which a diagonal or u
// column never writes, so that load of unwritten memory is intended -- it stays inside the record and its value is dropped
template <int NV> __device__ __forceinline__ int rec_row(bool pack, int k, int r0) { return !pack ? k : (k >= NV ? k - NV + 2 : (k == r0 ? 0 : 1)); }
template <int NV> __device__ __forceinline__ bool rec_zero(bool pack, int k, int r0) { return pack && k < NV && k != r0; }

// ---- output stage of the pair kernels (problem.hpp:226-296) -----------------------------------------------------------
// NP: points per pass of the output stage (LBS: all of the wave's at once; LBS / 2: the torque-level pair kernel, whose
// accelerations are in registers until then, emits its two half-waves one after the other and needs half the LDS)
template <int NV, int NP = LBS>
struct OutStage {
  double qdd[NP * (NV + 1)];    // point-major, odd row stride: (joint k, point e) at qdd[e * (NV + 1) + k] -- conflict-free for the
                                // evaluation (lane = point) and for the output stage (16 lanes = 16 consecutive joints of one point)
  int pij[NP];                  // the point: first direction | second direction << 8 | valid << 16 (the six column addresses of a
                                // point are functions of these and of wave-uniform bases: recomputed by the lanes that emit it)
};

// Each stencil point owns one n-double column of a tensor (two for a symmetric pair) and reads four more columns (its two
// first-order columns and its two diagonal second-order columns).  Every lane leaves the accelerations of its evaluation and
// the six column addresses of its point in LDS.  Then a 16-lane group takes one point at a time: the lanes read the point's
// addresses once (LDS broadcasts) and own the rows k = kk + 16 j of its columns -- x_k, f_k sit in registers for the whole
// stage, an element costs four loads, at most one (conflict-free) LDS read and the store(s); two points per group in flight.
// (Round 1's form walked four points per 16-row chunk and re-read the addresses for every chunk: 8 LDS reads per element, the
// acceleration among them 16-way bank-conflicted; the stage was 12.5 ms of the 86 ms linearisation.)
// pass: which NP-block of the wave's lanes owns the slots this time (the caller has put their accelerations into S.qdd)
// PACK: the tensors are packed records (the diagonal columns read here as well as the columns written); a compile-time matter
// inside the stage.  UU: every point of the caller is a (u_i, u_j) pair -- with records no configuration row is read or written
// then (used under PACK only: the contract-layout code of every caller is what it was)
template <int NV, int NP, bool PACK, bool UU>
__device__ __forceinline__ void offdiag_emit_as(const LinParams& p, OutStage<NV, NP>& S, bool valid, int i, int j, int64_t bt,
                                                const double* __restrict__ xg, double dt, int pass) {
  constexpr int n = 2 * NV, mm = NV;
  // points in flight per group: two; one where the caller still holds the accelerations of the second half in registers
  constexpr int RW = 16, NJ = (n + RW - 1) / RW, GRP = LBS / RW, PPG = NP / GRP, NB = NP == LBS ? 2 : 1;
  static_assert(PPG % NB == 0, "points per group");
  const double eps = sqrt(sqrt(DBL_EPSILON));
  const double eps2 = eps * eps;
  const int lane = threadIdx.x;
  if (lane / NP == pass) S.pij[lane % NP] = i | (j << 8) | ((valid ? 1 : 0) << 16);
  double* const fxx = p.fxx + bt * n * n * n;
  double* const fux = p.fux + bt * n * mm * n;
  double* const fuu = p.fuu + bt * n * mm * mm;
  const double* const fxb = p.fx + bt * n * n;
  const double* const fub = p.fu + bt * n * mm;
  __syncthreads();
  const int kk = lane % RW, grp = lane / RW;
  const double* f0 = p.f_val + bt * n;
  constexpr bool pack = PACK, uu = UU && PACK;
  const bool skip_top = PACK || p.skip_top != 0;   // (packed records come with the skipped rows)
  constexpr int cs = pack ? NV + 2 : n;    // doubles from one tensor column to the next
  double f0k[NJ], xk[NJ], xvk[NJ];
#pragma unroll
  for (int jx = 0; jx < NJ; ++jx) {
    const int k = kk + RW * jx;
    const int kc = k < n ? k : n - 1;
    f0k[jx] = f0[kc];
    xk[jx] = xg[kc];
    xvk[jx] = kc < NV ? xg[NV + kc] : 0.0;
  }
  if (DEV_NO_EMIT) return;
  for (int pt = 0; pt < PPG; pt += NB) {
    double a1[NB][NJ], a2[NB][NJ], d1[NB][NJ], d2[NB][NJ];
    double* o0[NB];
    double* o1[NB];
    int ie[NB], je[NB], ee[NB], r2[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int e = (pt + u) * GRP + grp;
      ee[u] = e;
      const int pk = S.pij[e];
      const int i1 = pk & 255, j1 = (pk >> 8) & 255;
      ie[u] = i1;
      je[u] = j1;
      const bool at_x_1 = !uu && i1 < n, at_x_2 = !uu && j1 < n;
      const int idx_1 = at_x_1 ? i1 : i1 - n, idx_2 = at_x_2 ? j1 : j1 - n;
      double* tensor;
      int L;
      if (at_x_1) { if (at_x_2) { tensor = fxx; L = n; } else { tensor = fux; L = mm; } }
      else { tensor = fuu; L = mm; }
      r2[u] = at_x_1 ? idx_1 % NV : -1;
      o0[u] = (pk >> 16) ? tensor + (int64_t)idx_2 * cs + (int64_t)idx_1 * n * L : nullptr;
      o1[u] = ((pk >> 16) && at_x_1 == at_x_2 && !p.skip_qv_mirror) ? tensor + (int64_t)idx_1 * n + (int64_t)idx_2 * n * L : nullptr;   // (never with pack)
      if (o0[u]) {
        const double* q0 = at_x_1 ? fxb + (int64_t)idx_1 * n : fub + (int64_t)idx_1 * n;
        const double* q1 = at_x_2 ? fxb + (int64_t)idx_2 * n : fub + (int64_t)idx_2 * n;
        const double* q2 = at_x_1 ? fxx + (int64_t)idx_1 * cs + (int64_t)idx_1 * n * n : fuu + (int64_t)idx_1 * cs + (int64_t)idx_1 * n * mm;
        const double* q3 = at_x_2 ? fxx + (int64_t)idx_2 * cs + (int64_t)idx_2 * n * n : fuu + (int64_t)idx_2 * cs + (int64_t)idx_2 * n * mm;
        const int r3 = at_x_2 ? idx_2 % NV : -1;   // the one configuration row a diagonal column holds (r2: that of the first direction's)
#pragma unroll
        for (int jx = 0; jx < NJ; ++jx) {
          const int k = kk + RW * jx;
          const int kc = k < n ? k : n - 1;
          a1[u][jx] = q0[kc]; a2[u][jx] = q1[kc];
          const double v2 = q2[rec_row<NV>(pack, kc, r2[u])], v3 = q3[rec_row<NV>(pack, kc, r3)];
          d1[u][jx] = rec_zero<NV>(pack, kc, r2[u]) ? 0.0 : v2;
          d2[u][jx] = rec_zero<NV>(pack, kc, r3) ? 0.0 : v3;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (!o0[u]) continue;
#pragma unroll
      for (int jx = 0; jx < NJ; ++jx) {
        const int k = kk + RW * jx;
        if (k >= n) continue;
        // configuration rows: q+ = q + dt v does not see the dynamics; row k < nv of a stencil point differs from the base point's
        // only when one of the two directions is q_k or v_k -- every other entry is an exact zero, already in memory (skip_top)
        if (skip_top && k < NV && (uu || !((ie[u] < n && ie[u] % NV == k) || (je[u] < n && je[u] % NV == k)))) continue;
        // row k of f(x + dx, u + du) (dynamics_t::eval_to, problem.hpp:441-461)
        double xs = k == ie[u] ? xk[jx] + eps : xk[jx];
        if (k == je[u]) xs = xs + eps;
        double fv;
        if (k < NV) {
          double xv = (NV + k) == ie[u] ? xvk[jx] + eps : xvk[jx];
          if (NV + k == je[u]) xv = xv + eps;
          const double vo = dt * xv;
          fv = xs + vo;
        } else {
          fv = xs + S.qdd[ee[u] * (NV + 1) + (k - NV)] * dt;
        }
        double df = fv - f0k[jx];                         // difference_out
        df -= eps * a1[u][jx];
        df -= eps * a2[u][jx];
        df *= 2;
        const double val = 0.5 * (df / eps2 - d1[u][jx] - d2[u][jx]);
        o0[u][rec_row<NV>(pack, k, r2[u])] = val;
        if (o1[u]) o1[u][k] = val;
      }
    }
  }
}

// the layout picked at run time, for the callers with registers to spare (velocity and configuration pairs)
template <int NV, int NP>
__device__ __forceinline__ void offdiag_emit(const LinParams& p, OutStage<NV, NP>& S, bool valid, int i, int j, int64_t bt,
                                             const double* __restrict__ xg, double dt, int pass = 0) {
  if (p.pack) offdiag_emit_as<NV, NP, true, false>(p, S, valid, i, j, bt, xg, dt, pass);
  else offdiag_emit_as<NV, NP, false, false>(p, S, valid, i, j, bt, xg, dt, pass);
}

// ---- output stage for a row of the stencil: first direction i shared by the wave, second direction jb + lane -----
// The NV columns such a wave owns are one contiguous block of its tensor (element (k, lane) at k + lane n), and so is the
// block of first-order columns they read.  The accelerations are left in LDS lane-major with an odd row stride.
template <int NV>
struct RowStage {
  // rows 0 .. NV-1: the row's points; row NV: the torque-level kernel's extra point (direction i alone: DIAG_ROW below);
  // row NV+1: where the idle lanes of the wave leave their values.  12.5 KB at NV = 38: twelve workgroups per CU
  double q[(NV + 2) * (NV + 1)];
};

// Lane = (column group cg = lane / 16, kk = lane % 16) owns the rows k = kk + 16 j of four columns at a time, so that what
// depends on the row k of f alone is touched once per lane: x_k, f_k, the first-order and diagonal columns of direction i sit
// in registers (read straight from global: 128-byte runs, the same lines for the four column groups); per element there is
// one read of the block of first-order columns, one of the diagonal column of the second direction, at most one LDS read (the
// acceleration, rows k >= NV) and the store(s).
// DIAG_ROW = false: the diagonal second-order column (i, i) is read from d1g.  DIAG_ROW = true (torque-level rows): lane NV
// of the wave has evaluated the point "direction i alone" on the same cached operands (an otherwise idle lane); the column
// (problem.hpp:192-222: 2 ((f(x + eps e_i) - f(x)) - eps f_col_i) / eps^2) is formed here, kept for the row's own
// off-diagonal entries and written to d1g for the velocity- and configuration-level kernels that follow.
// out: the block [NV][n]; mirror (or null): column c at mirror + c * mstride; a2: contiguous [NV][n]; d2: column c at
// d2 + c * dstride; i: first direction (an x index); jb: x index of the second direction of column 0, or >= 2 NV for u directions
template <int NV, bool DIAG_ROW, class ST>
__device__ __forceinline__ void rowblock_emit(const ST& S, int lane, int i, int jb, double* __restrict__ out, double* __restrict__ mirror,
                                              int64_t mstride, const double* __restrict__ a2, const double* __restrict__ d2, int64_t dstride,
                                              double dt, const double* __restrict__ f0g, const double* __restrict__ a1g,
                                              double* __restrict__ d1g, const double* __restrict__ xg, bool skip_top = false, bool pack = false) {
  constexpr int n = 2 * NV, RW = 16, NJ = (n + RW - 1) / RW, CG = LBS / RW, NIT = (NV + CG - 1) / CG;
  const int r1 = i % NV;                             // the configuration row the first direction (an x direction) touches
  const int cs = pack ? NV + 2 : n;                  // doubles from one column of `out` to the next (pack: records; the caller's out, d2, dstride, d1g are the records')
  const double eps = sqrt(sqrt(DBL_EPSILON));
  const double eps2 = eps * eps;
  const int kk = lane % RW, cg = lane / RW;
  double xk[NJ], xvk[NJ], f0k[NJ], a1k[NJ], d1k[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int k = kk + RW * j;
    const int kc = k < n ? k : n - 1;
    f0k[j] = f0g[kc];
    a1k[j] = a1g[kc];
    double x = xg[kc];
    if (kc == i) x = x + eps;
    xk[j] = x;
    double xv = xg[kc < NV ? NV + kc : kc];
    if (NV + kc == i) xv = xv + eps;
    xvk[j] = xv;
    if constexpr (DIAG_ROW) {
      // problem.hpp:192-222 for direction i alone: 2 ((f(x + eps e_i) - f(x)) - eps f_col_i) / eps^2; row NV of S.q is the
      // evaluation of that point (the wave's otherwise idle lane NV)
      double fv;
      if (kc < NV) {
        const double vo = dt * xv;
        fv = x + vo;
      } else {
        fv = x + S.q[NV * (NV + 1) + (kc - NV)] * dt;
      }
      double df = fv - f0k[j];
      df -= eps * a1k[j];
      df *= 2;
      const double dd = df / eps2;
      d1k[j] = dd;
      if (cg == 0 && k < n && !(skip_top && k < NV && k != r1)) d1g[rec_row<NV>(pack, k, r1)] = dd;   // (a configuration row other than r1: an exact zero, in memory)
    } else {
      const double v = d1g[rec_row<NV>(pack, kc, r1)];
      d1k[j] = rec_zero<NV>(pack, kc, r1) ? 0.0 : v;
    }
  }
  // software-pipelined over the column groups: the operands of group it + 1 are requested before group it is formed and stored
  // (the evaluation's registers are dead here: room for a second operand buffer)
  double va2[2][NJ], vd2[2][NJ];
  auto fetch = [&](int it, double (&A)[NJ], double (&D)[NJ]) {
    const int c = it * CG + cg;
    const int cc = c < NV ? c : NV - 1;
    const int rd = jb + cc < n ? (jb + cc) % NV : -1;   // the one configuration row the column's diagonal column holds
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int k = kk + RW * j;
      const int kc = k < n ? k : n - 1;
      A[j] = a2[kc + cc * n];
      const double v = d2[rec_row<NV>(pack, kc, rd) + cc * dstride];
      D[j] = rec_zero<NV>(pack, kc, rd) ? 0.0 : v;
    }
  };
  auto form = [&](int it, const double (&A)[NJ], const double (&D)[NJ]) {
    const int c = it * CG + cg;
    const bool cv = c < NV;
    const int cc = cv ? c : NV - 1;
    const int jp = jb + cc;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int k = kk + RW * j;
      if (!(cv && k < n)) continue;
      // configuration rows other than those of the two directions: exact zeros, already in memory (LinParams::skip_top)
      if (skip_top && k < NV && k != r1 && !(jp < n && jp % NV == k)) continue;
      // row k of f(x + dx, u + du) (dynamics_t::eval_to, problem.hpp:441-461)
      double x = xk[j];
      if (k == jp) x = x + eps;
      double fv;
      if (k < NV) {
        double xv = xvk[j];
        if (NV + k == jp) xv = xv + eps;
        const double vo = dt * xv;
        fv = x + vo;
      } else {
        fv = x + S.q[cc * (NV + 1) + (k - NV)] * dt;
      }
      double df = fv - f0k[j];                          // difference_out
      df -= eps * a1k[j];
      df -= eps * A[j];
      df *= 2;
      const double val = 0.5 * (df / eps2 - d1k[j] - D[j]);
      out[rec_row<NV>(pack, k, r1) + c * cs] = val;
      if (mirror) mirror[k + c * mstride] = val;
    }
  };
  if (DEV_NO_EMIT) return;
  fetch(0, va2[0], vd2[0]);
  for (int it = 0; it < NIT; it += 2) {
    if (it + 1 < NIT) fetch(it + 1, va2[1], vd2[1]);
    form(it, va2[0], vd2[0]);
    if (it + 1 < NIT) {
      if (it + 2 < NIT) fetch(it + 2, va2[0], vd2[0]);
      form(it + 1, va2[1], vd2[1]);
    }
  }
}

// The output stages read their parameters from the kernel-argument segment (LinParams is every emitting kernel's first argument),
// and only behind the evaluation and a sched_barrier: taken from `p` they would be loaded at kernel entry and stay live through the
// whole evaluation, and the scalar registers would spill.  Through the address-space-4 pointer the reads stay scalar loads.
typedef __attribute__((address_space(4))) const LinParams* kernarg_t;
__device__ __forceinline__ kernarg_t kernarg_params() { return (kernarg_t)__builtin_amdgcn_kernarg_segment_ptr(); }
// ... and the part of them the off-diagonal output stage (offdiag_emit) takes, as a LinParams of its own
__device__ __forceinline__ LinParams emit_params() {
  const kernarg_t kp = kernarg_params();
  LinParams po;
  po.f_val = kp->f_val; po.fx = kp->fx; po.fu = kp->fu; po.fxx = kp->fxx; po.fux = kp->fux; po.fuu = kp->fuu; po.skip_qv_mirror = kp->skip_qv_mirror; po.skip_top = kp->skip_top; po.pack = kp->pack;
  return po;
}

// ---- torque level: the (x_i, u_j) and (u_i, u_j) points -------------------------------------------------------------
// One wave per group; the groups of one (instance, t):
//   g <  nv        : (q_g, u_lane)       cfg 1+g, vcfg nv+1+g   38 of 64 lanes
//   g <  2 nv      : (v_{g-nv}, u_lane)  cfg 0,   vcfg 1+(g-nv) 38 of 64 lanes
//   g >= 2 nv      : (u_i, u_j) pairs    cfg 0,   vcfg 0        64 pairs per wave
// PACK (pairs only): the output stage writes packed records.  An instantiation of its own because this kernel sits at its
// register bound: with the layout picked at run time inside the stage it gains scratch (132 -> 148-164 B per lane in three forms
// tried), as a template parameter the contract-layout kernel is untouched and the record one needs no scratch
// SP (rows only): the q-cache is a base block and deltas; the staged LDS image is the same, word by word
// VSP (rows only, with SP): so is the v-cache (VcLayout): rows g < nv read entry 0 and the q-step deltas of g, rows g >= nv the v-step
// base block and the v-step deltas of g - nv
template <class T, bool ROWS, bool PACK = false, bool SP = false, bool VSP = false>
__global__ __launch_bounds__(LBS, ROWS ? 1 : 3) void lin_static_tau_kernel(LinParams p) {
  constexpr int nv = T::N, n = 2 * nv;
  constexpr int TRI = nv * (nv - 1) / 2, GU = (TRI + LBS - 1) / LBS, G = ROWS ? 2 * nv : GU;
  const int64_t bt = blockIdx.x / G;
  const int g = (int)(blockIdx.x % G) + (ROWS ? 0 : 2 * nv);
  const int lane = threadIdx.x;
  const int64_t Tn = p.d.T;
  const int b = (int)(bt / Tn);
  const int64_t t = bt % Tn;
  const DevModel& m = *p.model;
  int i, j, cfg, vcfg;
  bool valid;
  if (g < nv) { i = g; j = n + lane; cfg = 1 + g; vcfg = nv + 1 + g; valid = lane < nv; }
  else if (g < 2 * nv) { i = g; j = n + lane; cfg = 0; vcfg = 1 + (g - nv); valid = lane < nv; }
  else {
    const int pid = (g - 2 * nv) * LBS + lane;
    valid = pid < TRI;
    tri_index(valid ? pid : 0, nv, i, j);
    i += n; j += n; cfg = 0; vcfg = 0;
  }
  const double eps = sqrt(sqrt(DBL_EPSILON));
  static_assert(ROWS || !SP, "the pairs read the base block alone");
  const double* __restrict__ qc = p.qcache + bt * p.qc_bt + (SP ? 0 : cfg * (nv * rbd::QC_STRIDE));
  static_assert(SP || !VSP, "the base + deltas v-cache comes with the base + deltas q-cache");
  const double* __restrict__ vc = p.vcache + bt * p.vc_bt + (VSP ? 0 : vcfg * (nv * rbd::VC_STRIDE));
  const double* __restrict__ xg = p.x + ((int64_t)b * (Tn + 1) + t) * n;
  const double* __restrict__ ug = p.u + ((int64_t)b * Tn + t) * nv;
  const int iu = i - n, ju = j - n;
  const int gq = cfg - 1;                                                         // the stepped joint, -1: none (SP)
  [[maybe_unused]] const unsigned long long ganc = SP && cfg > 0 ? g_anc_tab<T>.anc[gq] : 0ull;
  [[maybe_unused]] const int vkind = g < nv ? 0 : 1, vg = g < nv ? g : g - nv;   // the row's v point (VSP)
  // the staged operands are dead once the acceleration pass is over, the output stage's buffers (rows: RowStage, pairs: OutStage)
  // are not alive before: one LDS region for all of them (the evaluation and the output stage are a barrier apart)
  __shared__ union TauLds { double P[nv * PS + nv * rbd::VC_STRIDE]; RowStage<nv> S; OutStage<nv, LBS / 2> O; } s_lds;
  double* s_P = s_lds.P;
  // the v-cache block goes to LDS as well, in one coalesced pass (all of it in flight at once).  Through the scalar path its
  // 76 per-joint reads are 76 serialised L2 round trips per wave (measured on the rows: 19.5 -> 17.6 ms at 64 seeds)
  double* s_V = s_P + nv * PS;
  constexpr int KH = stage_split<T>();
  StageRegs<nv, 0, (KH > 0) ? KH : 1> lower;   // (KH == 0: joint 0 once more, harmless)            // joints 0 .. KH-1: in flight through the first half of the leaf -> root pass
  {
    StageRegs<nv, KH, nv> upper;
    if constexpr (SP) { upper.template load_sparse<T, VSP>(qc, gq, ganc, vc, vkind, vg, ganc, lane); lower.template load_sparse<T, VSP>(qc, gq, ganc, vc, vkind, vg, ganc, lane); }
    else { upper.load(qc, vc, lane); lower.load(qc, vc, lane); }
    upper.park(s_P, s_V, lane);
    rbd::coop_sync<true>();                         // one wave per workgroup: LDS is in order, no vmcnt(0) behind this fence
  }
  TauState<T> s;
  auto tau = [&](int k) { double v = ug[k]; if (k == iu) v = v + eps; if (k == ju) v = v + eps; return v; };
  // joints nv-1 .. KH+1 only touch records KH .. nv-1 (their own and their parents': checked below), joint KH needs its parent's
  static_assert(parents_at_least<T>(KH + 1, KH), "the first half of the pass must not reach below record KH");
  tau_up_range<T, PS, nv - 1>(m, s_P, s_V, tau, s, std::make_integer_sequence<int, nv - 1 - KH>{});
  lower.park(s_P, s_V, lane);
  rbd::coop_sync<true>();
  tau_up_range<T, PS, KH>(m, s_P, s_V, tau, s, std::make_integer_sequence<int, KH + 1>{});
  tau_down_all<T, PS>(m, s_P, s_V, s, std::make_integer_sequence<int, nv>{});
  // the output stage reads its pointers from the kernel-argument segment only now (kernarg_params)
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (ROWS) {
    const kernarg_t kp = kernarg_params();
    RowStage<nv>& S = s_lds.S;
    const int mm = nv;
    __syncthreads();                       // every lane is done with the staged operands
    // unconditional on purpose: under `if (valid)` the optimiser sinks the whole evaluation into the branch, away from
    // its operand loads, and every operand then spills
    const int row = lane <= nv ? lane : nv + 1;      // lane nv: direction i alone (its second direction index falls off the controls)
#pragma unroll
    for (int k = 0; k < nv; ++k) S.q[row * (nv + 1) + k] = s.uu[k];
    // (the staging loop comes after these stores: the evaluation must meet its first use in its own basic block)
    __syncthreads();     // row nv of q is another lane's
    // column (k, u_c) of the (x_i, u) slab of f_ux: k + c n + i n m
    const bool pack = kp->pack != 0;
    const int64_t cs = pack ? nv + 2 : n;     // column stride of the tensors: records or contract columns
    rowblock_emit<nv, true>(S, lane, i, n, kp->fux + bt * n * mm * n + (int64_t)i * n * mm, nullptr, 0, kp->fu + bt * n * mm,
                            kp->fuu + bt * n * mm * mm, cs + (int64_t)n * mm, m.dt, kp->f_val + bt * n,
                            kp->fx + bt * n * n + (int64_t)i * n, kp->fxx + bt * n * n * n + (int64_t)i * cs + (int64_t)i * n * n, xg, kp->skip_top != 0, pack);
  } else {
    OutStage<nv, LBS / 2>& S = s_lds.O;
    const LinParams po = emit_params();
    const double dt = m.dt;
    __syncthreads();                       // every lane is done with the staged operands
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
      if (pass) __syncthreads();                  // the first half's slots have been read
      if (lane / (LBS / 2) == pass) {
#pragma unroll
        for (int k = 0; k < nv; ++k) S.qdd[(lane % (LBS / 2)) * (nv + 1) + k] = s.uu[k];
      }
      offdiag_emit_as<nv, LBS / 2, PACK, true>(po, S, valid, i, j, bt, xg, dt, pass);
    }
  }
}

// ---- velocity level: the (q_i, v_j) and (v_i, v_j) points ----------------------------------------------------------
// The evaluation is rbd::aba_vu_cached (velocity pass, bias-force pass, acceleration pass on the cached q-part), but
// its first two passes are walked chain by chain (a chain = a run of single-child joints): down a chain computing the
// link velocities, back up it forming the bias forces, so that only one chain's velocities are alive at a time; the
// velocity of a branching joint is formed when its first child chain needs it.  The third pass recomputes the link
// velocities on its way down instead of keeping 12 doubles per joint from the first.  u_i lives in registers in the row
// and pair kernels below (VelCtx<0>), in the LDS buffer the output stage reads the accelerations from elsewhere.
template <class T> constexpr int n_children(int k) {
  int c = 0;
  for (int j = k + 1; j < T::N; ++j) if (T::parent[j] == k) ++c;
  return c;
}
template <class T> constexpr bool chain_start(int k) { return T::parent[k] < 0 || T::parent[k] != k - 1 || n_children<T>(T::parent[k]) > 1; }
template <class T> constexpr bool chain_end(int k) { return k == T::N - 1 || chain_start<T>(k + 1); }
template <class T> constexpr int chain_first(int k) { while (!chain_start<T>(k)) --k; return k; }
// longest chain of the tree: sizes the LDS buffer of the chain-wise sweeps (8 for the Talos-like tree: its arms)
template <class T> constexpr int max_chain() {
  int best = 1;
  for (int k = 0; k < T::N; ++k)
    if (chain_end<T>(k)) { const int len = k - chain_first<T>(k) + 1; if (len > best) best = len; }
  return best;
}

// ---- the joint steps the static sweeps share ------------------------------------------------------------------------------
// The per-joint arithmetic of the local-frame ABA with the joint type a compile-time constant (o: where the joint's axis sits in a
// motion vector, 0 revolute / 3 prismatic), on pointers and register arrays, written once.  A sweep family (velocity level,
// configuration level, cache fill, v-cache rows) fetches its operands its own way, calls the steps and stores the results its own way.
// The order of the floating-point operations in a step is part of it: the families are held bit-equal to each other by tests.

// joint motion vector vJ = S_K v_K (the first loop of rbd::aba_tree / aba_vu_cached)
template <int o>
__device__ __forceinline__ void step_joint_motion(const double* a, double vK, double* vJ) {
#pragma unroll
  for (int k = 0; k < 6; ++k) vJ[k] = 0.0;
  vJ[o] = a[0] * vK; vJ[o + 1] = a[1] * vK; vJ[o + 2] = a[2] * vK;
}
// link velocity v_K = X_K v_parent + vJ (the same loop); ROOT: no parent, vel_par is not read
template <bool ROOT>
__device__ __forceinline__ void step_link_vel(const double* E, const double* r, const double* vel_par, const double* vJ, double* vel) {
  if constexpr (!ROOT) rbd::xform_motion(E, r, vel_par, vel);
  else {
#pragma unroll
    for (int k = 0; k < 6; ++k) vel[k] = 0.0;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) vel[k] += vJ[k];
}
// bias force of a link that no child has contributed to yet: pA = v x* (I v) (rbd::aba_tree, first loop)
__device__ __forceinline__ void step_bias_force0(const double* I6, const double* vel, double* pA) {
  double Iv[6];
  rbd::sym6_mv(I6, vel, Iv);
  rbd::crf(vel, Iv, pA);
}
// U = IA S and 1/D = 1 / (S^T U + arm), arm the joint's armature (rbd::aba_tree / aba_qpart, leaf -> root loop)
template <int o>
__device__ __forceinline__ void step_U_dinv(const double* IA, const double* a, double arm, double* U, double& dinv) {
  double d = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r) U[r] = IA[rbd::sidx(r, o)] * a[0] + IA[rbd::sidx(r, o + 1)] * a[1] + IA[rbd::sidx(r, o + 2)] * a[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) d += a[k] * U[o + k];
  d += arm;
  dinv = 1.0 / d;
}
// Ia = IA - U U^T / D (the same loop)
__device__ __forceinline__ void step_Ia(const double* IA, const double* U, double dinv, double* Ia) {
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int cc = 0; cc <= r; ++cc) Ia[rbd::sidx(r, cc)] = IA[rbd::sidx(r, cc)] - U[r] * U[cc] * dinv;
}
// u_K = tau_K - S^T pA (the same loop).  tau_K is read where it is used, behind the sum: passed by value, its load moves ahead of the
// sum and the dense velocity rows of the Talos-like tree gain 8 B of scratch (profiles/summary_static_shared_steps.txt)
template <int o>
__device__ __forceinline__ double step_u(const double* a, const double* pA, const double* tauK) {
  double sp = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) sp += a[k] * pA[o + k];
  return *tauK - sp;
}
// force handed up to the parent: fp = X^T (pA + Ia cb + U u / D) (the same loop; the inertia handed up is rbd::add_xtix)
__device__ __forceinline__ void step_force_up(const double* E, const double* r, const double* pA, const double* Iac, const double* U,
                                              double ui, double dinv, double* fp) {
  double pa[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) pa[k] = pA[k] + Iac[k] + U[k] * (ui * dinv);
  rbd::xform_force_T(E, r, pa, fp);
}
// acceleration step of joint K (the root -> leaf loop of rbd::aba_tree / aba_vu_cached), the link velocity recomputed on the way:
// uK holds u_K on entry and the joint acceleration on return; vel / acc of the parent are read (a root starts from gravity), those
// of K are left for its children.  acc holds the bias-force accumulators of the pass before until this step overwrites them
template <class T, int K>
__device__ __forceinline__ void step_accel(const DevModel* m, const double* E, const double* r, const double* U, double dinv, double vK,
                                           double& uK, double (&vel_all)[T::N][6], double (&acc_all)[T::N][6]) {
  constexpr int o = T::prismatic[K] ? 3 : 0;
  constexpr int par = T::parent[K];
  const double* a = m->axis[K];
  double vJ[6], vel[6], cb[6], ap[6];
  step_joint_motion<o>(a, vK, vJ);
  if constexpr (par >= 0) {
    rbd::xform_motion(E, r, vel_all[par], vel);
    rbd::xform_motion(E, r, acc_all[par], ap);
  } else {
    const double a0[6] = {0, 0, 0, -m->gravity[0], -m->gravity[1], -m->gravity[2]};
#pragma unroll
    for (int k = 0; k < 6; ++k) vel[k] = 0.0;
    rbd::xform_motion(E, r, a0, ap);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) vel[k] += vJ[k];
  rbd::crm(vel, vJ, cb);
  double sum = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) { ap[k] += cb[k]; sum += U[k] * ap[k]; }
  const double qd = (uK - sum) * dinv;
  uK = qd;
  if constexpr (has_child<T>(K)) {
#pragma unroll
    for (int k = 0; k < 6; ++k) { vel_all[K][k] = vel[k]; acc_all[K][k] = ap[k]; }
    acc_all[K][o] += a[0] * qd; acc_all[K][o + 1] += a[1] * qd; acc_all[K][o + 2] += a[2] * qd;
  }
}
// the v-part record of a joint, cb | pA0 | Ia cb (rbd::aba_vpart_cached), into rec[18]
__device__ __forceinline__ void step_vpart(const double* I6, const double* Ia, const double* vel, const double* vJ, double* rec) {
  rbd::crm(vel, vJ, rec);
  step_bias_force0(I6, vel, rec + 6);
  rbd::sym6_mv(Ia, rec, rec + 12);
}

template <class T>
struct VelState {
  double vel[T::N][6];   // link velocities (a chain at a time, plus the branching joints)
  double acc[T::N][6];   // bias-force accumulators, then link accelerations
  double uu[T::N];       // u_i, then the joint acceleration (contexts with UQS == 0; else they live in LDS behind uq)
};

template <int UQS_, int QS_ = rbd::QC_STRIDE>
struct VelCtx {
  static constexpr int UQS = UQS_;   // stride between consecutive joints of this lane's u_i / acceleration buffer in LDS;
                                     // 0: no buffer, the values stay in registers (VelState::uu)
  static constexpr int QS = QS_;     // doubles per joint of the (E | r | U | 1/D) block behind qp
  static constexpr bool V_STEPPED = true;   // the lane steps velocities (lane_v)
  static constexpr bool LDS_VEL = false;    // a chain's link velocities stay in registers (VelState::vel)
  const DevModel* m;
  const double* qp;                  // (E | r | U | 1/D): the q-cache block itself, or its copy in LDS
  const double* __restrict__ qc;
  const double* __restrict__ xg;
  const double* __restrict__ ug;
  double* uq;            // LDS: u_i, then the joint acceleration, of this lane (joint K at uq[K * UQS])
  int i, j;              // perturbed directions (x indices; q directions do not change v)
  double eps;
  // operands of joint K: E | r (12 doubles; buf: room for a context that has to form them), U | 1/D (7 doubles), and the
  // product Ia cb, which is all the evaluator takes from Ia
  template <int K> __device__ __forceinline__ const double* er(double*) const { return qp + K * QS; }
  template <int K> __device__ __forceinline__ const double* er_down(double* b) const { return er<K>(b); }   // E | r again, in the acceleration pass
  template <int K> __device__ __forceinline__ const double* ud() const { return qp + K * QS + 12; }
  // Ia cb (ud: what ud<K>() returned)
  template <int K> __device__ __forceinline__ void ia_cb(const double*, const double* cb, double* Iac) const { rbd::sym6_mv(qc + K * rbd::QC_STRIDE + 19, cb, Iac); }
  template <int K> __device__ __forceinline__ const double* ud_down() const { return ud<K>(); }   // U | 1/D again, in the acceleration pass
};

// v_K of this lane's point: stepped at the velocity level, the base one in the contexts whose points differ in q alone
template <int NV, class C>
__device__ __forceinline__ double lane_v(const C& c, int K) {
  double v = c.xg[NV + K];
  if constexpr (C::V_STEPPED) {
    if (NV + K == c.i) v = v + c.eps;
    if (NV + K == c.j) v = v + c.eps;
  }
  return v;
}

// ---- the chain drivers: generic over the context (what a context has to offer: VelCtx) -------------------------------------
// A chain's link velocities live in registers (VelState::vel, the velocity level) or in LDS (C::LDS_VEL: the sweeps that also carry
// articulated inertias -- full ABA, cache fill -- slot K - F of c.lvel); the branching joints' stay in registers in both forms.
template <class T, int K, class C>
__device__ __forceinline__ void joint_vel(const C& c, const double* E, const double* vel_par, double* vel) {
  double vJ[6];
  step_joint_motion<T::prismatic[K] ? 3 : 0>(c.m->axis[K], lane_v<T::N>(c, K), vJ);
  step_link_vel<(T::parent[K] < 0)>(E, E + 9, vel_par, vJ, vel);
}
// velocity of joint K from the root (used for the branching joints).  A joint's E | r is fetched behind its ancestors' steps: fetched
// ahead of them, every placement of the path is alive at once where a context forms it (the cache fill and the full-ABA sweep of
// the Talos-like tree spilled 48 to 64 B more that way)
template <class T, int K, class C>
__device__ __forceinline__ void vel_from_root(const C& c, double* vel) {
  double Pb[12], vp[6];
  if constexpr (T::parent[K] >= 0) vel_from_root<T, T::parent[K]>(c, vp);
  const double* E = c.template er<K>(Pb);
  joint_vel<T, K>(c, E, vp, vel);
}

// register form: joints K .. E of a chain
template <class T, int K, int E, class C>
__device__ __forceinline__ void chain_down(const C& c, VelState<T>& s) {
  double Pb[12];
  joint_vel<T, K>(c, c.template er<K>(Pb), s.vel[T::parent[K] >= 0 ? T::parent[K] : 0], s.vel[K]);   // (a root: no parent is read)
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (K < E) chain_down<T, K + 1, E>(c, s);
}
// LDS form: joints K .. E of the chain that starts at F go to slots K - F; `cur` carries the velocity of the previous joint
template <class T, int K, int F, int E, class C>
__device__ __forceinline__ void chain_down_lds(const C& c, double* cur) {
  double Pb[12], vel[6];
  joint_vel<T, K>(c, c.template er<K>(Pb), cur, vel);
#pragma unroll
  for (int k = 0; k < 6; ++k) { cur[k] = vel[k]; c.lvel[((K - F) * 6 + k) * LBS] = vel[k]; }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (K < E) chain_down_lds<T, K + 1, F, E>(c, cur);
}
// LDS form: the velocity of joint K of the chain that starts at F, or of the joint the chain hangs from (K < F: a branching joint)
template <class T, int K, int F, class C>
__device__ __forceinline__ void chain_vel_load(const C& c, const double (&vel_all)[T::N][6], double* vel) {
  if constexpr (K >= F) {
#pragma unroll
    for (int k = 0; k < 6; ++k) vel[k] = c.lvel[((K - F) * 6 + k) * LBS];
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) vel[k] = vel_all[K][k];
  }
}

// leaf -> root step of the velocity level (rbd::aba_vu_cached, second loop) for the joints K .. F of a chain
template <class T, int K, int F, class C>
__device__ __forceinline__ void chain_up(const C& c, VelState<T>& s) {
  constexpr int o = T::prismatic[K] ? 3 : 0;
  double Pb[12];
  const double* E = c.template er<K>(Pb);
  const double* r = E + 9;
  const double* U = c.template ud<K>();
  const double dinv = U[6];
  const double* a = c.m->axis[K];
  double pAi[6];
  if constexpr (has_child<T>(K)) {
#pragma unroll
    for (int k = 0; k < 6; ++k) pAi[k] = s.acc[K][k];
  } else {
    step_bias_force0(c.m->I6[K], s.vel[K], pAi);
  }
  const double ui = step_u<o>(a, pAi, c.ug + K);
  if constexpr (C::UQS == 0) s.uu[K] = ui; else c.uq[K * C::UQS] = ui;
  constexpr int par = T::parent[K];
  if constexpr (par >= 0) {
    double vJ[6], cb[6], Iac[6], fp[6];
    step_joint_motion<o>(a, lane_v<T::N>(c, K), vJ);
    rbd::crm(s.vel[K], vJ, cb);
    c.template ia_cb<K>(U, cb, Iac);
    step_force_up(E, r, pAi, Iac, U, ui, dinv, fp);
    if constexpr (first_contrib<T>(K)) {
      double p0[6];
      step_bias_force0(c.m->I6[par], s.vel[par], p0);
#pragma unroll
      for (int k = 0; k < 6; ++k) s.acc[par][k] = p0[k] + fp[k];
    } else {
#pragma unroll
      for (int k = 0; k < 6; ++k) s.acc[par][k] += fp[k];
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (K > F) chain_up<T, K - 1, F>(c, s);
}

// Chains in descending order of their joints: a chain is processed when the fold reaches its last joint -- down it for the link
// velocities, back up it with the family's leaf -> root step (the chain_up overload of the family's context and state)
template <class T, int K, class C, class S>
__device__ __forceinline__ void chain_at(const C& c, S& s) {
  if constexpr (chain_end<T>(K)) {
    constexpr int F = chain_first<T>(K), P = T::parent[F];
    if constexpr (P >= 0) {
      // the largest-index child chain of a branching joint is the first to need (and to form) that joint's velocity
      if constexpr (first_contrib<T>(F) && n_children<T>(P) > 1) vel_from_root<T, P>(c, s.vel[P]);
    }
    if constexpr (C::LDS_VEL) {
      double cur[6] = {0, 0, 0, 0, 0, 0};
      if constexpr (P >= 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) cur[k] = s.vel[P][k];
      }
      chain_down_lds<T, F, F, K>(c, cur);
    } else {
      chain_down<T, F, K>(c, s);
    }
    chain_up<T, K, F>(c, s);
  }
}
template <class T, class C, class S, int... Ks>
__device__ __forceinline__ void chains_up_all(const C& c, S& s, std::integer_sequence<int, Ks...>) {
  (chain_at<T, T::N - 1 - Ks>(c, s), ...);
}

// acceleration pass (rbd::aba_vu_cached, third loop), link velocities recomputed on the way
template <class T, int K, class C>
__device__ __forceinline__ void vel_down(const C& c, VelState<T>& s) {
  double Pb[12];
  const double* E = c.template er_down<K>(Pb);
  const double* U = c.template ud_down<K>();
  double* uK;
  if constexpr (C::UQS == 0) uK = &s.uu[K]; else uK = c.uq + K * C::UQS;
  step_accel<T, K>(c.m, E, E + 9, U, U[6], lane_v<T::N>(c, K), *uK, s.vel, s.acc);
  __builtin_amdgcn_sched_barrier(0);
}
template <class T, class C, int... Ks>
__device__ __forceinline__ void vel_down_all(const C& c, VelState<T>& s, std::integer_sequence<int, Ks...>) {
  (vel_down<T, Ks>(c, s), ...);
}

// One wave per group; the groups of one (instance, t):
//   ROWS:  g < nv : (q_g, v_lane)      cfg 1+g   38 of 64 lanes, row-block output (+ mirror image)
//   !ROWS: (v_i, v_j) pairs, cfg 0, 64 pairs per wave, generic output in two half-wave passes
// (the pairs: 2 waves per SIMD and no scratch, or -DDDP_VEL_PAIR_WAVES=3 with 208 B of it: the A/B build of DESIGN.md section 4)
#ifndef DDP_VEL_PAIR_WAVES
#define DDP_VEL_PAIR_WAVES 2
#endif
template <class T, bool ROWS, bool SP = false>
__global__ __launch_bounds__(LBS, ROWS ? 3 : DDP_VEL_PAIR_WAVES) void lin_static_vel_kernel(LinParams p) {
  static_assert(ROWS || !SP, "the pairs read the base block alone");
  constexpr int nv = T::N, n = 2 * nv;
  constexpr int TRI = nv * (nv - 1) / 2, GU = (TRI + LBS - 1) / LBS, G = ROWS ? nv : GU;
  const int64_t bt = blockIdx.x / G;
  const int g = (int)(blockIdx.x % G);
  const int lane = threadIdx.x;
  const int64_t Tn = p.d.T;
  const int b = (int)(bt / Tn);
  const int64_t t = bt % Tn;
  int i, j, cfg;
  bool valid;
  if (ROWS) { i = g; j = nv + lane; cfg = 1 + g; valid = lane < nv; }
  else {
    const int pid = g * LBS + lane;
    valid = pid < TRI;
    tri_index(valid ? pid : 0, nv, i, j);
    i += nv; j += nv; cfg = 0;
  }
  // u_i / the accelerations stay in registers, and the staged operands (dead after the acceleration pass) share their LDS with
  // the output stage's buffers (alive after it).  Pairs: the output stage takes the wave's points in two halves (PairStage)
  struct PairStage { OutStage<nv, LBS / 2> O; double spare[nv + 1]; };   // spare: where the half that is not emitted leaves its values
  using Stage = typename std::conditional<ROWS, RowStage<nv>, PairStage>::type;
  // the whole q-cache block of the wave's configuration (placements, U, 1/D and the articulated inertias: 12 KB) is staged in
  // LDS, all of its loads in flight at once; nothing of the evaluation goes through the scalar path's serialised round trips
  __shared__ union VelLds { Stage S; double P[nv * rbd::QC_STRIDE]; } s_lds;
  Stage& S = s_lds.S;
  double* s_P = s_lds.P;
  VelCtx<0, rbd::QC_STRIDE> c;
  c.m = p.model;
  c.qc = p.qcache + bt * p.qc_bt + (SP ? 0 : cfg * (nv * rbd::QC_STRIDE));
  c.qp = s_P;
  c.xg = p.x + ((int64_t)b * (Tn + 1) + t) * n;
  c.ug = p.u + ((int64_t)b * Tn + t) * nv;
  c.i = i; c.j = j;
  c.eps = sqrt(sqrt(DBL_EPSILON));
  c.uq = nullptr;
  {
    constexpr int NW = nv * rbd::QC_STRIDE, CW = (NW + LBS - 1) / LBS;
    double rq[CW];
    // (SP: word by word from the base block or the row's delta block -- the same image as the dense block of configuration 1+g)
    [[maybe_unused]] const unsigned long long ganc = SP ? g_anc_tab<T>.anc[g] : 0ull;
#pragma unroll
    for (int r = 0; r < CW; ++r) {
      int idx = r * LBS + lane;
      idx = idx < NW ? idx : NW - 1;
      if constexpr (SP) idx = qc_word<T>(g, ganc, idx / rbd::QC_STRIDE, idx % rbd::QC_STRIDE);
      rq[r] = c.qc[idx];
    }
#pragma unroll
    for (int r = 0; r < CW; ++r) { const int idx = r * LBS + lane; s_P[idx < NW ? idx : NW - 1] = rq[r]; }
    c.qc = s_P;
    rbd::coop_sync<true>();
  }
  VelState<T> s;
  chains_up_all<T>(c, s, std::make_integer_sequence<int, nv>{});
  vel_down_all<T>(c, s, std::make_integer_sequence<int, nv>{});
  __builtin_amdgcn_sched_barrier(0);
  const double dt = c.m->dt;
  if constexpr (ROWS) {
    const kernarg_t kp = kernarg_params();
    double* fxx = kp->fxx + bt * n * n * n;
    const double* fxb = kp->fx + bt * n * n;
    __syncthreads();                       // every lane is done with the staged operands
    // lane-major with an odd stride (the layout the row-block output reads), idle lanes share the spare row; unconditional
    // stores right behind the evaluation (see the torque-level kernel)
    const int row = valid ? lane : nv;
#pragma unroll
    for (int k = 0; k < nv; ++k) S.q[row * (nv + 1) + k] = s.uu[k];
    __syncthreads();
    // column (k, v_c) of slab q_i of f_xx: k + (nv + c) n + i n n; its mirror image: column q_i of slab v_c
    const bool pack = kp->pack != 0;
    const int64_t cs = pack ? nv + 2 : n;     // column stride of f_xx: records or contract columns
    rowblock_emit<nv, false>(S, lane, i, nv, fxx + (int64_t)nv * cs + (int64_t)i * n * n,
                             kp->skip_qv_mirror ? nullptr : fxx + (int64_t)i * n + (int64_t)nv * n * n, (int64_t)n * n,
                             fxb + (int64_t)nv * n, fxx + (int64_t)nv * cs + (int64_t)nv * n * n, cs + (int64_t)n * n, dt,
                             kp->f_val + bt * n, fxb + (int64_t)i * n, fxx + (int64_t)i * cs + (int64_t)i * n * n, c.xg, kp->skip_top != 0, pack);
  } else {
    constexpr int NP = LBS / 2;
    const LinParams po = emit_params();
    __syncthreads();                       // every lane is done with the staged operands
    // point-major with an odd stride (OutStage); the second half of the wave parks its values in the spare row for now.
    // Unconditional stores right behind the evaluation (see the torque-level kernel)
    double* const own = &S.O.qdd[(lane % NP) * (nv + 1)];
    double* const row = lane < NP ? own : S.spare;
#pragma unroll
    for (int k = 0; k < nv; ++k) row[k] = s.uu[k];
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
      if (pass) {
        __syncthreads();                  // the first half's slots have been read
        if (lane >= NP) {
#pragma unroll
          for (int k = 0; k < nv; ++k) own[k] = s.uu[k];
        }
      }
      offdiag_emit<nv, NP>(po, S.O, valid, i, j, bt, c.xg, dt, pass);
    }
  }
}

// ---- configuration level, full ABA: the first-order q columns, and the (q_i, q_j) points under DDP_HIP_CFG_FULL_ABA ----
// (the (q_i, q_j) points otherwise: "configuration level by splice" below)
// Every point has its own configuration, so the whole articulated-body algorithm runs per lane (rbd::aba_tree): the
// chain-wise sweep of the velocity level, with the articulated inertias accumulated alongside the bias forces.  Only
// the placements of joints i and j differ from the base configuration: each lane fetches those two from the q-cache of
// configurations 1+i and 1+j once, everything else comes through the scalar path.  What the third pass needs from the
// second (U, 1/D, u: 8 doubles per joint) does not fit in registers or LDS; it goes through a per-wave workspace,
// written and read back once, 512-byte coalesced rows.
constexpr int WS_PER_JOINT = 8;

template <class T>
struct CfgState {
  double vel[T::N][6];
  double accP[T::N][6];
  double accI[T::N][21];
  double w[2][WS_PER_JOINT];   // third pass: workspace values of the current / next joint
};

template <class T>
struct CfgCtx {
  static constexpr bool V_STEPPED = false;
  static constexpr bool LDS_VEL = true;
  const DevModel* __restrict__ m;
  const double* __restrict__ qc0;   // q-cache of the base configuration
  const double* __restrict__ xg;
  const double* __restrict__ ug;
  double* __restrict__ W;           // this lane's column of the wave's workspace: (K, e) at W[(K * 8 + e) * LBS]
  double* lvel;                     // LDS: link velocities of the chain being swept, (slot, k) at lvel[(slot * 6 + k) * LBS]
  int i, j;
  const double* own;                // null: joints i, j take E | r from configurations 1+i, 1+j of the q-cache;
                                    // else this lane's own E | r of joint i (first order: a step the cache does not hold)
  // E | r of joint K at q_K and at q_K + eps (configuration 1+K of the q-cache): both wave-uniform, selected per lane into P
  template <int K> __device__ __forceinline__ const double* er(double* P) const {
    const double* base = qc0 + K * rbd::QC_STRIDE;
    const double* pert = own ? own : qc0 + ((int64_t)(1 + K) * T::N + K) * rbd::QC_STRIDE;
    const bool mine = K == i || K == j;
#pragma unroll
    for (int e = 0; e < 12; ++e) P[e] = mine ? pert[e] : base[e];
    return P;
  }
};

// leaf -> root step of the full ABA (rbd::aba_tree, second loop) for the joints K .. F of a chain
template <class T, int K, int F>
__device__ __forceinline__ void chain_up(const CfgCtx<T>& c, CfgState<T>& s) {
  constexpr int o = T::prismatic[K] ? 3 : 0;
  const double* a = c.m->axis[K];
  double IA[21], pAi[6], U[6], velK[6], dinv;
  chain_vel_load<T, K, F>(c, s.vel, velK);
  if constexpr (has_child<T>(K)) {
#pragma unroll
    for (int k = 0; k < 21; ++k) IA[k] = s.accI[K][k];
#pragma unroll
    for (int k = 0; k < 6; ++k) pAi[k] = s.accP[K][k];
  } else {
#pragma unroll
    for (int k = 0; k < 21; ++k) IA[k] = c.m->I6[K][k];
    step_bias_force0(c.m->I6[K], velK, pAi);
  }
  step_U_dinv<o>(IA, a, c.m->armature[K], U, dinv);
  const double ui = step_u<o>(a, pAi, c.ug + K);
#pragma unroll
  for (int k = 0; k < 6; ++k) c.W[(K * WS_PER_JOINT + k) * LBS] = U[k];
  c.W[(K * WS_PER_JOINT + 6) * LBS] = dinv;
  c.W[(K * WS_PER_JOINT + 7) * LBS] = ui;
  constexpr int par = T::parent[K];
  if constexpr (par >= 0) {
    double Pb[12], Ia[21], vJ[6], cb[6], Iac[6], fp[6];
    const double* P = c.template er<K>(Pb);
    step_joint_motion<o>(a, lane_v<T::N>(c, K), vJ);
    step_Ia(IA, U, dinv, Ia);
    rbd::crm(velK, vJ, cb);
    rbd::sym6_mv(Ia, cb, Iac);
    step_force_up(P, P + 9, pAi, Iac, U, ui, dinv, fp);
    if constexpr (first_contrib<T>(K)) {
      double velP[6];
      chain_vel_load<T, par, F>(c, s.vel, velP);
#pragma unroll
      for (int k = 0; k < 21; ++k) s.accI[par][k] = c.m->I6[par][k];
      step_bias_force0(c.m->I6[par], velP, s.accP[par]);
    }
    rbd::add_xtix(P, P + 9, Ia, s.accI[par]);
#pragma unroll
    for (int k = 0; k < 6; ++k) s.accP[par][k] += fp[k];
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (K > F) chain_up<T, K - 1, F>(c, s);
}

// acceleration pass (rbd::aba_tree, third loop); link velocities recomputed, (U, 1/D, u) read back one joint ahead
// where the acceleration pass leaves joint K's acceleration: uq[K * STRIDE] (STRIDE = LBS: [joint][lane] rows of the
// pair output stage; STRIDE = 1: this lane's own row)
template <int STRIDE_>
struct CfgDownOut { double* uq; static constexpr int STRIDE = STRIDE_; };

template <class T, int K, class O>
__device__ __forceinline__ void cfg_down(const CfgCtx<T>& c, CfgState<T>& s, const O& out) {
  if constexpr (K + 1 < T::N) {
#pragma unroll
    for (int e = 0; e < WS_PER_JOINT; ++e) s.w[(K + 1) & 1][e] = c.W[((K + 1) * WS_PER_JOINT + e) * LBS];
  }
  const double* U = s.w[K & 1];
  const double vK = lane_v<T::N>(c, K);
  double Pb[12], uK = U[7];
  const double* P = c.template er<K>(Pb);
  step_accel<T, K>(c.m, P, P + 9, U, U[6], vK, uK, s.vel, s.accP);
  out.uq[K * (O::STRIDE == LBS ? LBS : 1)] = uK;
  __builtin_amdgcn_sched_barrier(0);
}
template <class T, class O, int... Ks>
__device__ __forceinline__ void cfg_down_all(const CfgCtx<T>& c, CfgState<T>& s, const O& out, std::integer_sequence<int, Ks...>) {
  (cfg_down<T, Ks>(c, s, out), ...);
}

// One wave = 64 (q_i, q_j) pairs, i < j, in two kernels: the fused velocity / articulated-inertia / bias-force sweep
// (register hungry: one wave per SIMD), then the acceleration pass and the output stage (light: several waves per
// SIMD hide the workspace reads).  The pointers the evaluation reads through are separate restrict-qualified arguments:
// the workspace stores must not turn the scalar operand loads that follow them into per-lane loads.
template <class T>
__device__ __forceinline__ void cfg_setup(CfgCtx<T>& c, const LinParams& p, const DevModel* __restrict__ model, const double* __restrict__ qcache,
                                          const double* __restrict__ xs, const double* __restrict__ us, double* __restrict__ ws,
                                          int64_t bt0, int64_t& bt, bool& valid) {
  constexpr int nv = T::N, n = 2 * nv;
  constexpr int TRI = nv * (nv - 1) / 2, GU = (TRI + LBS - 1) / LBS;
  bt = bt0 + blockIdx.x / GU;
  const int g = (int)(blockIdx.x % GU);
  const int lane = threadIdx.x;
  const int64_t Tn = p.d.T;
  const int b = (int)(bt / Tn);
  const int64_t t = bt % Tn;
  const int pid = g * LBS + lane;
  valid = pid < TRI;
  tri_index(valid ? pid : 0, nv, c.i, c.j);
  c.m = model;
  c.qc0 = qcache + bt * p.qc_bt;          // (whole blocks: LinPlan::qc_sparse is off with the full-ABA level)
  c.xg = xs + ((int64_t)b * (Tn + 1) + t) * n;
  c.ug = us + ((int64_t)b * Tn + t) * nv;
  c.W = ws + (int64_t)blockIdx.x * (nv * WS_PER_JOINT * LBS) + lane;
  c.own = nullptr;
}

template <class T>
__global__ __launch_bounds__(LBS) void lin_static_cfg_up_kernel(LinParams p, const DevModel* __restrict__ model, const double* __restrict__ qcache,
                                                                const double* __restrict__ xs, const double* __restrict__ us,
                                                                double* __restrict__ ws, int64_t bt0) {
  constexpr int nv = T::N;
  constexpr int MAXCH = max_chain<T>();  // longest chain of the topology
  __shared__ double s_vel[MAXCH * 6 * LBS];
  CfgCtx<T> c;
  int64_t bt;
  bool valid;
  cfg_setup<T>(c, p, model, qcache, xs, us, ws, bt0, bt, valid);
  c.lvel = s_vel + threadIdx.x;
  CfgState<T> s;
  chains_up_all<T>(c, s, std::make_integer_sequence<int, nv>{});
}

template <class T>
__global__ __launch_bounds__(LBS) void lin_static_cfg_down_kernel(LinParams p, const DevModel* __restrict__ model, const double* __restrict__ qcache,
                                                                  const double* __restrict__ xs, const double* __restrict__ us,
                                                                  double* __restrict__ ws, int64_t bt0) {
  constexpr int nv = T::N;
  __shared__ OutStage<nv> S;
  CfgCtx<T> c;
  int64_t bt;
  bool valid;
  cfg_setup<T>(c, p, model, qcache, xs, us, ws, bt0, bt, valid);
  c.lvel = nullptr;
  CfgState<T> s;
#pragma unroll
  for (int e = 0; e < WS_PER_JOINT; ++e) s.w[0][e] = c.W[e * LBS];
  CfgDownOut<nv + 1> o{&S.qdd[threadIdx.x * (nv + 1)]};
  cfg_down_all<T>(c, s, o, std::make_integer_sequence<int, nv>{});
  __builtin_amdgcn_sched_barrier(0);
  offdiag_emit<nv, LBS>(emit_params(), S, valid, c.i, c.j, bt, c.xg, model->dt);
}

// ---- configuration level by splice: the (q_i, q_j) points from cached q-parts --------------------------------------
// In the local-frame ABA the record of joint K is E | r (a function of q_K alone) and U | 1/D | Ia (functions of the q of
// the strict descendants of K alone).  At q + eps e_i + eps e_j, with S_x the strict ancestors of x:
//   E | r of K        : configuration 1+K of the q-cache if K is i or j, else the base configuration;
//   U | 1/D | Ia of K : base if K is in neither S_i nor S_j; configuration 1+i if in S_i only; configuration 1+j if in
//                       S_j only; recomputed only on the spine S_i & S_j (a path that ends at the root), from I6[K] and its
//                       children's X^T Ia X in the order of the q-cache kernel, each child's Ia by the same rule.
// The spine records are formed by a pre-pass (a lane per pair); with them a point is a velocity-level evaluation whose
// per-joint operands are selected per lane: no per-lane inertia state, nothing handed from pass to pass but u_i.
// What the evaluator takes from Ia is Ia cb alone, and on the spine cb is the base one (the link velocity of K moves with the q of
// K and of its ancestors only): the pre-pass forms Ia cb with the cb of v-cache entry 0 and a spine record is U | 1/D | Ia cb.
constexpr int SREC = 13;            // doubles per spine record: U[6] | 1/D | Ia cb[6]

// The pairs of one (instance, t) are dealt to the lanes in the order of their spine's deepest joint (`top`), ties in tri_index order:
// the lanes of a wave then mostly walk the same joints (little divergence, the same model constants, in the pre-pass), and the records
// of one top are laid out [depth][pair of that top], so that what a wave writes or gathers for one joint is one contiguous run.
template <class T>
struct SpineTab {
  static constexpr int N = T::N, TRI = N * (N - 1) / 2;
  static_assert(N >= 2 && N <= 64, "ancestor masks are 64 bits wide");
  unsigned long long mask[N];       // desc_mask: bit i set <=> the joint is a strict ancestor of i
  unsigned long long anc[N];        // the transpose: bit K set <=> K is a strict ancestor of the joint
  int depth[N];                     // number of strict ancestors
  int nrec;                         // records per (instance, t): the sum of the spine lengths
  // per lane slot (pairs ordered by top):
  short pi[TRI], pj[TRI];           // the pair, i < j
  short top[TRI];                   // deepest joint of its spine S_i & S_j (-1: empty); the spine is top and its ancestors
  int rbase[TRI], rstride[TRI];     // the record of its spine joint of depth d: rbase + d * rstride
};
template <class T>
constexpr SpineTab<T> make_spine_tab() {
  SpineTab<T> t{};
  for (int k = 0; k < T::N; ++k)
    for (int a = T::parent[k]; a >= 0; a = T::parent[a]) { ++t.depth[k]; t.mask[a] |= 1ull << k; t.anc[k] |= 1ull << a; }
  // counting sort by top + 1
  int cnt[T::N + 2] = {}, start[T::N + 2] = {}, goff[T::N + 2] = {};
  for (int i = 0; i < T::N; ++i)
    for (int j = i + 1; j < T::N; ++j) {
      int a = T::parent[i];
      while (a >= 0 && !((t.mask[a] >> j) & 1)) a = T::parent[a];
      ++cnt[a + 1];
    }
  for (int g = 0; g <= T::N; ++g) {
    start[g + 1] = start[g] + cnt[g];
    goff[g + 1] = goff[g] + cnt[g] * (g == 0 ? 0 : t.depth[g - 1] + 1);
  }
  t.nrec = goff[T::N + 1];
  int fill[T::N + 2] = {};
  for (int i = 0; i < T::N; ++i)
    for (int j = i + 1; j < T::N; ++j) {
      int a = T::parent[i];
      while (a >= 0 && !((t.mask[a] >> j) & 1)) a = T::parent[a];
      const int g = a + 1, rank = fill[g]++, slot = start[g] + rank;
      t.pi[slot] = (short)i; t.pj[slot] = (short)j; t.top[slot] = (short)a;
      t.rbase[slot] = goff[g] + rank;
      t.rstride[slot] = cnt[g];
    }
  return t;
}
template <class T> __device__ const SpineTab<T> g_spine_tab = make_spine_tab<T>();
template <class T> constexpr unsigned long long desc_mask(int k) { return make_spine_tab<T>().mask[k]; }
template <class T> constexpr int depth_of(int k) { return make_spine_tab<T>().depth[k]; }
template <class T> constexpr int spine_records() { return make_spine_tab<T>().nrec; }
// on some pair's spine: at least two strict descendants
template <class T> constexpr bool spine_joint(int k) { const unsigned long long mk = desc_mask<T>(k); return (mk & (mk - 1)) != 0; }

// Workgroups x and x + 8 run on the same XCD: the GU waves of one (instance, t) are dealt to one XCD, whose L2 then serves
// their re-reads of that (instance, t)'s q-cache block and spine records.  Grid: GU workgroups for each of nb rounded up
// to a multiple of 8; false: a padding workgroup.
template <int GU>
__device__ __forceinline__ bool xcd_slot(int nb, int& btl, int& g) {
  const int x = (int)blockIdx.x, s = x >> 3;
  btl = (s / GU) * 8 + (x & 7);
  g = s % GU;
  return btl < nb;
}

// One lane per pair: its spine from the deepest joint to the root (the expressions of the cache fill's chain_up).  Joint indices are
// run-time values here, so the per-joint constants come from the model in memory, register arrays are indexed by constants only and
// the joint type is a select: the U | 1/D | Ia block below is step_U_dinv / step_Ia in that run-time form, kept as it was.
// SP: the stepped configurations' records come from the delta blocks (they are exactly the records a step changes)
template <class T, bool SP>
__global__ __launch_bounds__(LBS) void lin_static_spine_kernel(const DevModel* __restrict__ model, const double* __restrict__ qcache, int64_t qc_bt,
                                                               const double* __restrict__ vcache, int64_t vc_bt, double* __restrict__ spine, int64_t bt0, int nb) {
  constexpr int nv = T::N, TRI = nv * (nv - 1) / 2, GU = (TRI + LBS - 1) / LBS, NREC = spine_records<T>();
  int btl, g;
  if (!xcd_slot<GU>(nb, btl, g)) return;
  const int slot = g * LBS + (int)threadIdx.x;
  if (slot >= TRI) return;                                  // (no barrier below)
  const SpineTab<T>& tab = g_spine_tab<T>;
  const DevModel& m = *model;
  const int i = tab.pi[slot], j = tab.pj[slot];
  const int rstride = tab.rstride[slot];
  [[maybe_unused]] const unsigned long long anc_i = tab.anc[i], anc_j = tab.anc[j];
  const double* __restrict__ qc0 = qcache + (bt0 + btl) * qc_bt;
  const double* __restrict__ vc0 = vcache + (bt0 + btl) * vc_bt;   // entry 0: the base (q, v), first in either layout
  double* __restrict__ out = spine + ((int64_t)btl * NREC + tab.rbase[slot]) * SREC;
  double Ia[21];
#pragma unroll
  for (int k = 0; k < 21; ++k) Ia[k] = 0.0;
  int prev = -1;
  for (int K = tab.top[slot]; K >= 0; K = m.parent[K]) {
    double IA[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) IA[k] = m.I6[K][k];
    for (int sl = m.child_start[K]; sl < m.child_start[K + 1]; ++sl) {     // descending index: the order of the leaf -> root pass
      const int c = m.child_list[sl];
      const unsigned long long mc = tab.mask[c];
      const int cfg_p = (c == i || c == j) ? 1 + c : 0;
      const int cfg_i = ((mc >> i) & 1) ? 1 + i : (((mc >> j) & 1) ? 1 + j : 0);   // (c == prev: on the spine, the value just formed)
      const double *Pg, *Ig;
      if constexpr (SP) {
        using L = QcLayout<T>;
        Pg = qc0 + (cfg_p ? L::DELTA + c * L::DW : c * rbd::QC_STRIDE);
        // (the depth of c among the stepped joint's ancestors by counting, not from the table: no load ahead of the Ia loads)
        const int dc = __popcll((((mc >> i) & 1) ? anc_i : anc_j) & ((1ull << c) - 1ull));
        Ig = qc0 + (cfg_i ? L::PATH0 + (cfg_i - 1) * L::DW + dc * L::UD + 7 : c * rbd::QC_STRIDE + 19);
      } else {
        Pg = qc0 + ((int64_t)cfg_p * nv + c) * rbd::QC_STRIDE;
        Ig = qc0 + ((int64_t)cfg_i * nv + c) * rbd::QC_STRIDE + 19;
      }
      double P[12], Ic[21];
#pragma unroll
      for (int k = 0; k < 12; ++k) P[k] = Pg[k];
#pragma unroll
      for (int k = 0; k < 21; ++k) { const double v = Ig[k]; Ic[k] = c == prev ? Ia[k] : v; }
      rbd::add_xtix(P, P + 9, Ic, IA);
    }
    const bool pris = m.jtype[K] == DDP_HIP_JOINT_PRISMATIC;
    const double* a = m.axis[K];
    double U[6], d = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double u0 = IA[rbd::sidx(r, 0)] * a[0] + IA[rbd::sidx(r, 1)] * a[1] + IA[rbd::sidx(r, 2)] * a[2];
      const double u3 = IA[rbd::sidx(r, 3)] * a[0] + IA[rbd::sidx(r, 4)] * a[1] + IA[rbd::sidx(r, 5)] * a[2];
      U[r] = pris ? u3 : u0;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) d += a[k] * (pris ? U[3 + k] : U[k]);
    d += m.armature[K];
    const double dinv = 1.0 / d;
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int cc = 0; cc <= r; ++cc) Ia[rbd::sidx(r, cc)] = IA[rbd::sidx(r, cc)] - U[r] * U[cc] * dinv;
    double cb[6], Iac[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) cb[k] = vc0[K * rbd::VC_STRIDE + k];
    rbd::sym6_mv(Ia, cb, Iac);
    double* o = out + (int64_t)tab.depth[K] * rstride * SREC;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[k] = U[k];
    o[6] = dinv;
#pragma unroll
    for (int k = 0; k < 6; ++k) o[7 + k] = Iac[k];
    prev = K;
  }
}

// The velocity-level evaluator's context for a (q_i, q_j) point.  Every operand is read through a per-lane pointer: E | r of K
// from the base configuration or from configuration 1+K; U | 1/D | Ia of a joint with children from one of the sources above
// (re-reads of the (instance, t)'s q-cache block and spine records, mostly the same address in every lane).  Branch-free:
// selections by integer arithmetic and one select between two finished pointers -- a conditional address computation becomes a
// branch, and control flow in the middle of the evaluation tears it away from its operand loads.
// SP: records of configuration 1+g come from the delta block of g (E | r of g, U | 1/D | Ia of g's ancestors by depth); the
// selections keep their form, only the offsets differ
template <class T, bool SP>
struct SpliceCtx {
  using L = QcLayout<T>;
  static constexpr int UQS = 1;
  static constexpr bool V_STEPPED = false;   // q directions do not change v
  static constexpr bool LDS_VEL = false;
  const DevModel* m;
  const double* __restrict__ qc0;   // q-cache of the (instance, t): configuration c at qc0 + c * nv * QC_STRIDE
  const double* __restrict__ xg;
  const double* __restrict__ ug;
  const double* __restrict__ spb;   // spine records of the (instance, t)
  int rbase, rstride;               // ... this lane's: the joint of depth d at spb + (rbase + d * rstride) * SREC
  double* uq;
  int i, j;                         // perturbed joints, i < j
  unsigned long long ai, aj;        // their strict ancestors (SpineTab::anc): K is in S_i <=> bit K of ai
  template <int K> __device__ __forceinline__ const double* er(double*) const {
    const int own = (int)(K == i) | (int)(K == j);
    if constexpr (SP) return qc0 + (K * rbd::QC_STRIDE + own * (L::DELTA + K * L::DW - K * rbd::QC_STRIDE));
    else return qc0 + (K * rbd::QC_STRIDE + own * ((1 + K) * T::N * rbd::QC_STRIDE));
  }
  template <int K> __device__ __forceinline__ const double* ud() const {
    constexpr int DK = depth_of<T>(K);
    if constexpr (desc_mask<T>(K) == 0) return qc0 + (K * rbd::QC_STRIDE + 12);     // a leaf: nothing below it moves
    else {
      const int si = (int)((ai >> K) & 1), sj = (int)((aj >> K) & 1);
      const int cfg = (si & (sj ^ 1)) * (1 + i) + (sj & (si ^ 1)) * (1 + j);
      // (SP: cfg - 1 is the stepped joint whose delta block holds the record, at this joint's depth)
      const double* p = SP ? qc0 + ((K * rbd::QC_STRIDE + 12) + (si ^ sj) * (L::PATH0 - L::DW + DK * L::UD - (K * rbd::QC_STRIDE + 12)) + cfg * L::DW)
                           : qc0 + ((cfg * T::N + K) * rbd::QC_STRIDE + 12);
      if constexpr (!spine_joint<T>(K)) return p;
      else {
        const double* q = spb + (rbase + DK * rstride) * SREC;
        return (si & sj) ? q : p;
      }
    }
  }
  // The same addresses, written differently on purpose: recognised as the same values, the per-lane pointers of the leaf -> root
  // pass would stay alive until the acceleration pass comes by, and the kernel would not fit two waves per SIMD
  template <int K> __device__ __forceinline__ const double* er_down(double*) const {
    const int64_t own = (K - i) * (K - j) == 0 ? (SP ? (int64_t)(L::DELTA + K * L::DW - K * rbd::QC_STRIDE) : (int64_t)(1 + K) * T::N * rbd::QC_STRIDE) : 0;
    return qc0 + K * rbd::QC_STRIDE + own;
  }
  template <int K> __device__ __forceinline__ const double* ud_down() const {
    constexpr int DK = depth_of<T>(K);
    if constexpr (desc_mask<T>(K) == 0) return qc0 + (K * rbd::QC_STRIDE + 12);
    else {
      const bool si = (ai >> K) & 1, sj = (aj >> K) & 1;
      const int cfg = sj ? 1 + j : (si ? 1 + i : 0);
      const double* p = SP ? qc0 + (cfg ? (int64_t)(cfg - 1) * L::DW + (L::PATH0 + DK * L::UD) : (int64_t)(K * rbd::QC_STRIDE + 12))
                           : qc0 + (int64_t)cfg * (T::N * rbd::QC_STRIDE) + (K * rbd::QC_STRIDE + 12);
      if constexpr (!spine_joint<T>(K)) return p;
      else {
        const double* q = spb + ((int64_t)rbase + (int64_t)DK * rstride) * SREC;
        return ((ai & aj) >> K) & 1 ? q : p;
      }
    }
  }
  // Ia cb: off the spine from the 21 entries behind U | 1/D; on it the pre-pass has formed it (behind U | 1/D as well: for the
  // other lanes those six doubles are the head of Ia, loaded anyway), and Ia is read from the base record and not used
  template <int K> __device__ __forceinline__ void ia_cb(const double* ud, const double* cb, double* Iac) const {
    if constexpr (!spine_joint<T>(K)) rbd::sym6_mv(ud + 7, cb, Iac);
    else {
      const int on = (int)(((ai & aj) >> K) & 1);
      const double* pIa = on ? qc0 + (K * rbd::QC_STRIDE + 19) : ud + 7;
      const double w1 = (double)on, w0 = (double)(on ^ 1);
      double t[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) t[k] = ud[7 + k];
      rbd::sym6_mv(pIa, cb, Iac);
      // (an exact blend by weights 0 and 1, all values finite: as a select the product would be sunk into a branch)
#pragma unroll
      for (int k = 0; k < 6; ++k) Iac[k] = w1 * t[k] + w0 * Iac[k];
    }
  }
};
// One wave = 64 (q_i, q_j) pairs, i < j: the velocity-level pair kernel on spliced operands
template <class T, bool SP>
__global__ __launch_bounds__(LBS, 2) void lin_static_cfg_pair_kernel(LinParams p, const double* __restrict__ spine, int64_t bt0, int nb) {
  constexpr int nv = T::N, n = 2 * nv;
  constexpr int TRI = nv * (nv - 1) / 2, GU = (TRI + LBS - 1) / LBS, NREC = spine_records<T>();
  int btl, g;
  if (!xcd_slot<GU>(nb, btl, g)) return;                    // the whole workgroup (one wave), ahead of every barrier
  const int64_t bt = bt0 + btl;
  const int lane = threadIdx.x;
  const int64_t Tn = p.d.T;
  const int b = (int)(bt / Tn);
  const int64_t t = bt % Tn;
  const int slot = g * LBS + lane;
  const bool valid = slot < TRI;
  const int sc = valid ? slot : 0;
  const SpineTab<T>& tab = g_spine_tab<T>;
  __shared__ OutStage<nv> S;
  SpliceCtx<T, SP> c;
  c.i = tab.pi[sc]; c.j = tab.pj[sc];
  c.ai = tab.anc[c.i];
  c.aj = tab.anc[c.j];
  c.rbase = tab.rbase[sc]; c.rstride = tab.rstride[sc];
  c.m = p.model;
  c.qc0 = p.qcache + bt * p.qc_bt;
  c.xg = p.x + ((int64_t)b * (Tn + 1) + t) * n;
  c.ug = p.u + ((int64_t)b * Tn + t) * nv;
  c.spb = spine + (int64_t)btl * NREC * SREC;
  c.uq = &S.qdd[lane * (nv + 1)];
  VelState<T> s;
  chains_up_all<T>(c, s, std::make_integer_sequence<int, nv>{});
  vel_down_all<T>(c, s, std::make_integer_sequence<int, nv>{});
  __builtin_amdgcn_sched_barrier(0);
  offdiag_emit<nv, LBS>(emit_params(), S, valid, c.i, c.j, bt, c.xg, c.m->dt);
}

// ---- first order: forward differences of f (problem.hpp:105-126 stepping, eps = sqrt(DBL_EPSILON)) -------------------
// Three waves per (instance, t): lane d < nv perturbs q_d (LEVEL 1, full evaluation with its own placement of joint
// d), v_d (LEVEL 2, velocity level on the base configuration) or u_d (LEVEL 3, torque level on the base (q, v)).
// Column d of f_x / f_u is (f(x + eps e_d) - f(x)) / eps; the nv columns of a wave are one contiguous block.
// DIAG: the same single-direction evaluations with eps = eps_mach^(1/4) give the diagonal second-order entries
// (problem.hpp:192-222): column (d, d) of the tensor is 2 ((f(x + eps e_d) - f(x)) - eps f_col_d) / eps^2; `out` then
// points at column (0, 0) of the level's tensor block, consecutive columns ostride apart, fcol at the level's first-order block
template <int NV, bool DIAG>
__device__ __forceinline__ void first_output(const double* q /* LDS, lane-major, stride NV + 1 */, int lane, int d0, double* __restrict__ out,
                                             int64_t ostride, const double* __restrict__ fcol, const double* __restrict__ f0,
                                             const double* __restrict__ xg, double dt, double eps, bool skip_top = false, bool pack = false) {
  constexpr int n = 2 * NV, TOT = NV * n;
  const double eps2 = eps * eps;
  for (int e = lane; e < TOT; e += LBS) {
    const int c = e / n, k = e - c * n;
    const int d = d0 + c;                        // perturbed direction of this column (an x index, or >= n for u)
    if (DIAG && skip_top && k < NV && !(d < n && d % NV == k)) continue;   // configuration rows: exact zeros, in memory (LinParams::skip_top)
    double xk = xg[k];
    if (k == d) xk = xk + eps;
    double fv;
    if (k < NV) {
      double xv = xg[NV + k];
      if (NV + k == d) xv = xv + eps;
      const double vo = dt * xv;
      fv = xk + vo;
    } else {
      fv = xk + q[c * (NV + 1) + (k - NV)] * dt;
    }
    if constexpr (DIAG) {
      double df = fv - f0[k];
      df -= eps * fcol[e];
      df *= 2;
      out[rec_row<NV>(pack, k, d < n ? d % NV : -1) + c * ostride] = df / eps2;
    } else {
      out[e] = (fv - f0[k]) / eps;
    }
  }
}

template <class T, int LEVEL, bool DIAG>
__global__ __launch_bounds__(LBS) void lin_static_first_kernel(LinParams p, const DevModel* __restrict__ model, const double* __restrict__ qcache,
                                                               const double* __restrict__ xs, const double* __restrict__ us,
                                                               double* __restrict__ ws, int64_t bt0) {
  constexpr int nv = T::N, n = 2 * nv;
  const int64_t bt = bt0 + blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t Tn = p.d.T;
  const int b = (int)(bt / Tn);
  const int64_t t = bt % Tn;
  const bool valid = lane < nv;
  const double eps = DIAG ? sqrt(sqrt(DBL_EPSILON)) : sqrt(DBL_EPSILON);
  const double* __restrict__ qc0 = qcache + bt * p.qc_bt;      // the base block: first in either layout
  const double* __restrict__ xg = xs + ((int64_t)b * (Tn + 1) + t) * n;
  const double* __restrict__ ug = us + ((int64_t)b * Tn + t) * nv;
  __shared__ double s_q[(nv + 1) * (nv + 1)];
  double* uq = s_q + (valid ? lane : nv) * (nv + 1);
  if constexpr (LEVEL == 3) {
    const double* __restrict__ vc = p.vcache + bt * p.vc_bt;     // entry 0
    TauState<T> s;
    auto tau = [&](int k) { double v = ug[k]; if (k == lane) v = v + eps; return v; };
    tau_up_all<T, rbd::QC_STRIDE>(*model, qc0, vc, tau, s, std::make_integer_sequence<int, nv>{});
    tau_down_all<T, rbd::QC_STRIDE>(*model, qc0, vc, s, std::make_integer_sequence<int, nv>{});
#pragma unroll
    for (int k = 0; k < nv; ++k) uq[k] = s.uu[k];
  } else if constexpr (LEVEL == 2) {
    VelCtx<1> c;
    c.m = model; c.qc = qc0; c.qp = qc0; c.xg = xg; c.ug = ug; c.uq = uq;
    c.i = nv + lane; c.j = -1; c.eps = eps;
    VelState<T> s;
    chains_up_all<T>(c, s, std::make_integer_sequence<int, nv>{});
    vel_down_all<T>(c, s, std::make_integer_sequence<int, nv>{});
  } else {
    constexpr int MAXCH = max_chain<T>();
    __shared__ double s_vel[MAXCH * 6 * LBS];
    __shared__ double s_own[12 * LBS];
    if constexpr (!DIAG) {
      double E[9], r[3];
      const int jn = valid ? lane : 0;
      rbd::joint_placement(*model, jn, xg[jn] + eps, E, r);
#pragma unroll
      for (int e = 0; e < 9; ++e) s_own[lane * 12 + e] = E[e];
#pragma unroll
      for (int e = 0; e < 3; ++e) s_own[lane * 12 + 9 + e] = r[e];
    }
    CfgCtx<T> c;
    c.m = model; c.qc0 = qc0; c.xg = xg; c.ug = ug;
    c.W = ws + (int64_t)blockIdx.x * (nv * WS_PER_JOINT * LBS) + lane;
    c.lvel = s_vel + lane;
    c.i = valid ? lane : 0; c.j = -1;
    c.own = DIAG ? nullptr : s_own + lane * 12;     // eps_mach^(1/4) steps are the ones the q-cache holds
    CfgState<T> s;
    chains_up_all<T>(c, s, std::make_integer_sequence<int, nv>{});
#pragma unroll
    for (int e = 0; e < WS_PER_JOINT; ++e) s.w[0][e] = c.W[e * LBS];
    CfgDownOut<nv + 1> o{uq};
    cfg_down_all<T>(c, s, o, std::make_integer_sequence<int, nv>{});
  }
  __builtin_amdgcn_sched_barrier(0);
  const kernarg_t kp = kernarg_params();
  __syncthreads();
  if constexpr (!DIAG) {
    if (double* ao = kp->accel_out) {           // accelerations of the nv perturbed points of this level ([pair][3 nv directions: q, v, u | the point itself][nv]), for the analytic mode-1 pass
      ao += bt * (3 * nv + 1) * nv;
      double* al = ao + (LEVEL - 1) * nv * nv;
      for (int e = lane; e < nv * nv; e += LBS) { const int c = e / nv; al[e] = s_q[c * (nv + 1) + (e - c * nv)]; }
      // level 2: the idle lanes (no direction of theirs) have evaluated the unperturbed point into the spare row
      if (LEVEL == 2 && lane < nv) ao[3 * nv * nv + lane] = s_q[nv * (nv + 1) + lane];
      return;
    }
  }
  double* fcol = LEVEL == 3 ? kp->fu + bt * n * nv : kp->fx + bt * n * n + (LEVEL == 2 ? nv * n : 0);
  double* out = fcol;
  int64_t ostride = n;
  if constexpr (DIAG) {
    // column (d, d): f_xx at d (n + n n), f_uu at d (n + n m)
    const int64_t cs = kp->pack ? nv + 2 : n;     // column stride of the tensors: records (LinParams::pack) or contract columns
    if (LEVEL == 3) { out = kp->fuu + bt * n * nv * nv; ostride = cs + (int64_t)n * nv; }
    else { ostride = cs + (int64_t)n * n; out = kp->fxx + bt * n * n * n + (LEVEL == 2 ? nv * ostride : 0); }
  }
  first_output<nv, DIAG>(s_q, lane, LEVEL == 1 ? 0 : (LEVEL == 2 ? nv : n), out, ostride, fcol, kp->f_val + bt * n, xg, model->dt, eps, kp->skip_top != 0,
                         DIAG && kp->pack != 0);
}

// ---- first order along u, and the u diagonal, on LDS-staged operands ----------------------------------------------------------
// The same evaluations as lin_static_first_kernel<T, 3, *> (one wave per (instance, t), lane d perturbs u_d), with the operand
// path of the tau rows: E | r | U | 1/D of the base block and v-cache entry 0 are copied into LDS with every load in flight, and
// the evaluators read broadcasts from there instead of one dependent scalar-load round trip per joint stage.  The operation
// sequence of an evaluation is the scalar-path kernel's (tau_up / tau_down): the outputs are equal bit for bit
// (tests/test_first_staged.py).  The staged operands and the buffer the output stage reads the accelerations from share one LDS
// region, a barrier apart, which keeps a wave at 12 KB of LDS and the kernels at three waves per SIMD.
// (The v directions stay on lin_static_first_kernel<T, 2, false>: staged like the velocity rows the kernel was no faster -- DESIGN.md
// section 6b.)

// one torque-level evaluation of the wave's nv points (lane d: u_d + eps) on the two-phase staging of the tau rows; the joint
// accelerations are left in s.uu
template <class T>
__device__ __forceinline__ void first_tau_eval(const DevModel& m, const double* __restrict__ qc0, const double* __restrict__ vc,
                                               const double* __restrict__ ug, int lane, double eps, double* s_P, TauState<T>& s) {
  constexpr int nv = T::N;
  double* s_V = s_P + nv * PS;
  constexpr int KH = stage_split<T>();
  StageRegs<nv, 0, (KH > 0) ? KH : 1> lower;       // joints 0 .. KH-1: in flight through the first half of the leaf -> root pass
  {
    StageRegs<nv, KH, nv> upper;
    upper.load(qc0, vc, lane); lower.load(qc0, vc, lane);
    upper.park(s_P, s_V, lane);
    rbd::coop_sync<true>();                         // one wave per workgroup: LDS is in order
  }
  auto tau = [&](int k) { double v = ug[k]; if (k == lane) v = v + eps; return v; };
  static_assert(parents_at_least<T>(KH + 1, KH), "the first half of the pass must not reach below record KH");
  tau_up_range<T, PS, nv - 1>(m, s_P, s_V, tau, s, std::make_integer_sequence<int, nv - 1 - KH>{});
  lower.park(s_P, s_V, lane);
  rbd::coop_sync<true>();
  tau_up_range<T, PS, KH>(m, s_P, s_V, tau, s, std::make_integer_sequence<int, KH + 1>{});
  tau_down_all<T, PS>(m, s_P, s_V, s, std::make_integer_sequence<int, nv>{});
  __builtin_amdgcn_sched_barrier(0);
}

// DIAG false: the u columns (f_u, or the accelerations with accel_out set); true: the diagonal columns (u_d, u_d) of f_uu from
// the resident f_u (StaticLevel::UDiagonal)
template <class T, bool DIAG>
__global__ __launch_bounds__(LBS, 3) void lin_static_first_tau_kernel(LinParams p) {
  constexpr int nv = T::N, n = 2 * nv;
  const int64_t bt = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t Tn = p.d.T;
  const int b = (int)(bt / Tn);
  const int64_t t = bt % Tn;
  const DevModel& m = *p.model;
  const double* __restrict__ qc0 = p.qcache + bt * p.qc_bt;      // the base block: first in either layout
  const double* __restrict__ vc = p.vcache + bt * p.vc_bt;       // entry 0
  const double* __restrict__ xg = p.x + ((int64_t)b * (Tn + 1) + t) * n;
  const double* __restrict__ ug = p.u + ((int64_t)b * Tn + t) * nv;
  __shared__ union FirstTauLds { double P[nv * PS + nv * rbd::VC_STRIDE]; double q[(nv + 1) * (nv + 1)]; } s_lds;
  const double eps = DIAG ? sqrt(sqrt(DBL_EPSILON)) : sqrt(DBL_EPSILON);
  TauState<T> s;
  first_tau_eval<T>(m, qc0, vc, ug, lane, eps, s_lds.P, s);
  const kernarg_t kp = kernarg_params();
  __syncthreads();                         // every lane is done with the staged operands
  double* uq = s_lds.q + (lane < nv ? lane : nv) * (nv + 1);     // idle lanes share the spare row
#pragma unroll
  for (int k = 0; k < nv; ++k) uq[k] = s.uu[k];
  __syncthreads();
  if constexpr (!DIAG) {
    if (double* ao = kp->accel_out) {             // (lin_static_first_kernel: the u directions' block)
      double* al = ao + bt * (3 * nv + 1) * nv + 2 * nv * nv;
      for (int e = lane; e < nv * nv; e += LBS) { const int c = e / nv; al[e] = s_lds.q[c * (nv + 1) + (e - c * nv)]; }
      return;
    }
    double* fcol = kp->fu + bt * n * nv;
    first_output<nv, false>(s_lds.q, lane, n, fcol, n, fcol, kp->f_val + bt * n, xg, m.dt, eps);
  } else {
    // column (d, d) of f_uu at d (cs + n m): records (LinParams::pack) or contract columns
    const int64_t cs = kp->pack ? nv + 2 : n;
    first_output<nv, true>(s_lds.q, lane, n, kp->fuu + bt * n * nv * nv, cs + (int64_t)n * nv, kp->fu + bt * n * nv, kp->f_val + bt * n, xg, m.dt,
                           eps, kp->skip_top != 0, kp->pack != 0);
  }
}

// f_u and the u diagonal of one (instance, t) from one staged image: a workgroup of two waves, wave 0 evaluating at
// eps = sqrt(eps_mach), wave 1 at eps_mach^(1/4) -- the same instructions on a wave-uniform step.  Wave 0 then emits f_u; behind a
// workgroup barrier wave 1 emits the diagonal columns of f_uu, subtracting eps * f_u as it reads it back from memory: the stored
// value.  (Both evaluations in ONE wave would put the second behind the global stores of the first output stage: its reads of
// the model are then no longer provably unclobbered, leave the scalar path, and the kernel spills -- 168 VGPRs and 168 B of
// scratch per lane for the Talos-like tree in that form.)  Wave 1 keeps its accelerations in registers across wave 0's output
// stage; its first store behind the evaluation is unconditional (into a row of its own that nobody reads), like every
// evaluation's in this file.
template <class T>
__global__ __launch_bounds__(2 * LBS, 3) void lin_static_first_tau_fused_kernel(LinParams p) {
  constexpr int nv = T::N, n = 2 * nv;
  const int64_t bt = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / LBS), lane = (int)threadIdx.x % LBS;
  const int64_t Tn = p.d.T;
  const int b = (int)(bt / Tn);
  const int64_t t = bt % Tn;
  const DevModel& m = *p.model;
  const double* __restrict__ qc0 = p.qcache + bt * p.qc_bt;      // the base block: first in either layout
  const double* __restrict__ vc = p.vcache + bt * p.vc_bt;       // entry 0
  const double* __restrict__ xg = p.x + ((int64_t)b * (Tn + 1) + t) * n;
  const double* __restrict__ ug = p.u + ((int64_t)b * Tn + t) * nv;
  struct Out { double q[(nv + 1) * (nv + 1)]; double park[nv + 1]; };
  __shared__ union FirstTauFusedLds { double P[nv * PS + nv * rbd::VC_STRIDE]; Out o; } s_lds;
  double* s_P = s_lds.P;
  double* s_V = s_P + nv * PS;
  const double eps1 = sqrt(DBL_EPSILON), eps2 = sqrt(sqrt(DBL_EPSILON));
  const double eps = wave ? eps2 : eps1;
  {
    // E | r | U | 1/D of the base block and v-cache entry 0, copied by the two waves together, every load ahead of the first LDS store
    constexpr int NPW = nv * 19, NVW = nv * rbd::VC_STRIDE, NT = 2 * LBS;
    constexpr int CP = (NPW + NT - 1) / NT, CV = (NVW + NT - 1) / NT;
    const int tid = (int)threadIdx.x;
    double rp[CP], rv[CV];
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      int idx = c * NT + tid;
      idx = idx < NPW ? idx : NPW - 1;
      rp[c] = qc0[(idx / 19) * rbd::QC_STRIDE + idx % 19];
    }
#pragma unroll
    for (int c = 0; c < CV; ++c) {
      int idx = c * NT + tid;
      idx = idx < NVW ? idx : NVW - 1;
      rv[c] = vc[idx];
    }
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      int idx = c * NT + tid;
      idx = idx < NPW ? idx : NPW - 1;
      s_P[(idx / 19) * PS + idx % 19] = rp[c];
    }
#pragma unroll
    for (int c = 0; c < CV; ++c) {
      int idx = c * NT + tid;
      idx = idx < NVW ? idx : NVW - 1;
      s_V[idx] = rv[c];
    }
    __syncthreads();
  }
  TauState<T> s;
  auto tau = [&](int k) { double v = ug[k]; if (k == lane) v = v + eps; return v; };
  tau_up_all<T, PS>(m, s_P, s_V, tau, s, std::make_integer_sequence<int, nv>{});
  tau_down_all<T, PS>(m, s_P, s_V, s, std::make_integer_sequence<int, nv>{});
  __builtin_amdgcn_sched_barrier(0);
  const kernarg_t kp = kernarg_params();
  __syncthreads();                         // both waves are done with the staged operands
  double* const own = s_lds.o.q + (lane < nv ? lane : nv) * (nv + 1);     // idle lanes share the spare row
  double* const row = wave ? s_lds.o.park : own;
#pragma unroll
  for (int k = 0; k < nv; ++k) row[k] = s.uu[k];
  rbd::coop_sync<true>();                  // q is wave 0's alone here
  if (wave == 0) {
    double* fcol = kp->fu + bt * n * nv;
    first_output<nv, false>(s_lds.o.q, lane, n, fcol, n, fcol, kp->f_val + bt * n, xg, m.dt, eps1);
  }
  __syncthreads();                         // f_u is in memory for wave 1, and q has been read
  if (wave == 1) {
#pragma unroll
    for (int k = 0; k < nv; ++k) own[k] = s.uu[k];
    rbd::coop_sync<true>();
    // column (d, d) of f_uu at d (cs + n m): records (LinParams::pack) or contract columns
    const int64_t cs = kp->pack ? nv + 2 : n;
    first_output<nv, true>(s_lds.o.q, lane, n, kp->fuu + bt * n * nv * nv, cs + (int64_t)n * nv, kp->fu + bt * n * nv, kp->f_val + bt * n, xg, m.dt,
                           eps2, kp->skip_top != 0, kp->pack != 0);
  }
}

// ---- q- and v-caches ------------------------------------------------------------------------------------------------
// lin_static_qvcache_kernel: one wave per (instance, t), lane c = configuration c of the mode-2 stencil (0: q, 1+i:
// q + eps e_i).  The chain-wise sweep of the configuration level, reduced to what the caches hold: rbd::aba_qpart
// (E | r | U | 1/D | Ia per joint) and, at the base velocity, rbd::aba_vpart_cached (cb | pA0 | Ia cb) -- v-cache entry 0
// for the base configuration, nv+1+i for configuration 1+i.
// SP (LinPlan::qc_sparse): the lane of configuration 1+g stores the records its step changes -- E | r of g and U | 1/D | Ia of
// g's strict ancestors -- into the delta block of g (QcLayout), and everything else, like the base configuration's lane, onto the
// base block.  The chain itself is the same in every lane (the v-part needs all of it).
template <class T, int K>
__device__ __forceinline__ void placement_static(const DevModel& m, double q, double* P) {
  const double* Rp = m.Rp[K];
  const double* a = m.axis[K];
  double* E = P;
  double* r = P + 9;
  if constexpr (!T::prismatic[K]) {
    double sn, cs;
    sincos(q, &sn, &cs);
    const double Kx[9] = {0, -a[2], a[1], a[2], 0, -a[0], -a[1], a[0], 0};
    double K2[9], RJ[9], Rc[9];
    rbd::mm3(Kx, Kx, K2);
    const double omc = 1.0 - cs;
#pragma unroll
    for (int k = 0; k < 9; ++k) RJ[k] = sn * Kx[k] + omc * K2[k];
    RJ[0] += 1.0; RJ[4] += 1.0; RJ[8] += 1.0;
    rbd::mm3(Rp, RJ, Rc);
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int l = 0; l < 3; ++l) E[3 * k + l] = Rc[3 * l + k];
    r[0] = m.pp[K][0]; r[1] = m.pp[K][1]; r[2] = m.pp[K][2];
  } else {
    const double dd[3] = {a[0] * q, a[1] * q, a[2] * q};
    double Rd[3];
    rbd::mv3(Rp, dd, Rd);
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int l = 0; l < 3; ++l) E[3 * k + l] = Rp[3 * l + k];
    r[0] = m.pp[K][0] + Rd[0]; r[1] = m.pp[K][1] + Rd[1]; r[2] = m.pp[K][2] + Rd[2];
  }
}

template <class T, bool SP_, bool VSP_>
struct QvCtx {
  static constexpr bool SP = SP_, VSP = VSP_;
  static constexpr bool V_STEPPED = false;
  static constexpr bool LDS_VEL = true;
  const DevModel* __restrict__ m;
  const double* __restrict__ xg;
  double* qc;                  // this lane's q-cache block (SP: the base block of its (instance, t), which all of its lanes store onto)
  double* qown;                // SP, a stepped configuration: E | r of the stepped joint, the head of its delta block
  double* qpath;               // SP, a stepped configuration: the path records behind it ([depth][28])
  unsigned long long anc;      // SP: strict ancestors of the stepped joint
  double* __restrict__ vc;     // this lane's v-cache block (VSP: entry 0 of its (instance, t), which all of its lanes store onto)
  int vpath;                   // VSP, a stepped configuration: its q-step deltas, counted from vc -- the records of the ancestors ([depth][18]) ...
  int vsub;                    // ... and behind them those of the subtree, counted so that joint K's is at vc + vsub + K * 18
  int sub_end;                 // VSP: one past the stepped joint's subtree, jn .. sub_end - 1 (0: no step)
  double* lvel;                // LDS: link velocities of the chain being swept
  int jn;                      // joint whose position this lane steps (-1: none)
  double eps;
  // E | r of joint K at this lane's configuration, formed into P
  template <int K> __device__ __forceinline__ const double* er(double* P) const {
    double q = xg[K];
    if (K == jn) q = q + eps;
    placement_static<T, K>(*m, q, P);
    return P;
  }
};
template <class T>
struct QvState {
  double vel[T::N][6];
  double accI[T::N][21];
};
// leaf -> root step of the cache fill (rbd::aba_qpart, and rbd::aba_vpart_cached at the base velocity) for the joints K .. F of a chain
template <class T, int K, int F, bool SP, bool VSP>
__device__ __forceinline__ void chain_up(const QvCtx<T, SP, VSP>& c, QvState<T>& s) {
  constexpr int o = T::prismatic[K] ? 3 : 0;
  const double* a = c.m->axis[K];
  double Pb[12], IA[21], U[6], Ia[21], vel[6], dinv;
  const double* P = c.template er<K>(Pb);
  chain_vel_load<T, K, F>(c, s.vel, vel);
  if constexpr (has_child<T>(K)) {
#pragma unroll
    for (int k = 0; k < 21; ++k) IA[k] = s.accI[K][k];
  } else {
#pragma unroll
    for (int k = 0; k < 21; ++k) IA[k] = c.m->I6[K][k];
  }
  step_U_dinv<o>(IA, a, c.m->armature[K], U, dinv);
  step_Ia(IA, U, dinv, Ia);
  constexpr int par = T::parent[K];
  if constexpr (par >= 0) {
    if constexpr (first_contrib<T>(K)) {
#pragma unroll
      for (int k = 0; k < 21; ++k) s.accI[par][k] = c.m->I6[par][k];
    }
    rbd::add_xtix(P, P + 9, Ia, s.accI[par]);
  }
  double vJ[6], vrec[18];
  step_joint_motion<o>(a, lane_v<T::N>(c, K), vJ);
  step_vpart(c.m->I6[K], Ia, vel, vJ, vrec);
  // where the two halves of the record go.  SP: a half the lane's step changes goes to its delta block; any other half IS the
  // base record, bit for bit (the same instructions on the same operands in every lane), and is stored onto it: the lanes of an
  // (instance, t) then write one line with one value instead of a line each.  Selected addresses, not predicated stores: with
  // control flow in the chain the compiler contracts its products and sums differently from the dense kernel
  double* qo_er = c.qc + K * rbd::QC_STRIDE;
  double* qo_ud = qo_er + 12;
  if constexpr (SP) {
    constexpr int DK = depth_of<T>(K);       // (a constant expression: the table is not to be built at run time)
    qo_er = K == c.jn ? c.qown : qo_er;
    if constexpr (has_child<T>(K)) qo_ud = ((c.anc >> K) & 1ull) ? c.qpath + DK * QcLayout<T>::UD : qo_ud;
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) qo_er[k] = P[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) qo_ud[k] = U[k];
  qo_ud[6] = dinv;
#pragma unroll
  for (int k = 0; k < 21; ++k) qo_ud[7 + k] = Ia[k];
  // the v record likewise (VSP): one the step changes -- an ancestor's or the subtree's -- goes to the lane's q-step deltas, any other
  // onto entry 0, where the base configuration's lane stores the same bits
  // (an offset from the one pointer is selected, not a pointer: the stores stay global stores)
  int voff = K * rbd::VC_STRIDE;
  if constexpr (VSP) {
    constexpr int DK = depth_of<T>(K);
    voff = (K >= c.jn) & (K < c.sub_end) ? c.vsub + K * rbd::VC_STRIDE : voff;
    if constexpr (has_child<T>(K)) voff = ((c.anc >> K) & 1ull) ? c.vpath + DK * rbd::VC_STRIDE : voff;
  }
  double* vo = c.vc + voff;
#pragma unroll
  for (int k = 0; k < 18; ++k) vo[k] = vrec[k];
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (K > F) chain_up<T, K - 1, F>(c, s);
}

template <class T, bool SP, bool VSP = false>
__global__ __launch_bounds__(LBS, 2) void lin_static_qvcache_kernel(LinParams p, const DevModel* __restrict__ model, const double* __restrict__ xs,
                                                                 double* __restrict__ qcache, double* __restrict__ vcache) {
  constexpr int nv = T::N, n = 2 * nv, MAXCH = max_chain<T>();
  const int lane = threadIdx.x;
  const int64_t Tn = p.d.T;
  // a lane per (instance, t, configuration), 64 per wave: with a wave per (instance, t) 25 of its lanes (ncfg = nv + 1) or 63 of them
  // (the base configuration alone: first-order-only contexts, the accelerations of the analytic mode-1 pass) idle through a 38-joint chain
  const int64_t e = (int64_t)blockIdx.x * LBS + lane;    // evaluation: (instance, t) x configuration, 64 per wave whatever ncfg is
  const int64_t bt = e / p.ncfg;
  const int cfgi = (int)(e - bt * p.ncfg);
  const int b = (int)(bt / Tn);
  const int64_t t = bt % Tn;
  __shared__ double s_vel[MAXCH * 6 * LBS];
  if (bt >= p.d.batch * Tn) return;                       // (no workgroup barrier below)
  static_assert(SP || !VSP, "the base + deltas v-cache comes with the base + deltas q-cache");
  QvCtx<T, SP, VSP> c;
  c.m = model;
  c.xg = xs + ((int64_t)b * (Tn + 1) + t) * n;
  c.qc = qcache + bt * p.qc_bt + (SP ? 0 : cfgi * (nv * rbd::QC_STRIDE));
  {
    const int g = cfgi > 0 ? cfgi - 1 : 0;
    c.qown = c.qc + (QcLayout<T>::DELTA + g * QcLayout<T>::DW);
    c.qpath = c.qown + QcLayout<T>::ER;
    c.anc = g_anc_tab<T>.anc[g];
    c.vc = vcache + bt * p.vc_bt + (VSP || cfgi == 0 ? 0 : (nv + cfgi) * (nv * rbd::VC_STRIDE));
    c.vpath = g_vc_tab<T>.qoff[g];
    c.vsub = c.vpath + (__popcll(c.anc) - g) * rbd::VC_STRIDE;
    c.sub_end = cfgi > 0 ? g + g_vc_tab<T>.sub[g] : 0;
  }
  c.lvel = s_vel + lane;
  c.jn = cfgi - 1;
  c.eps = sqrt(sqrt(DBL_EPSILON));
  QvState<T> s;
  chains_up_all<T>(c, s, std::make_integer_sequence<int, nv>{});
}

// lin_static_vcache_kernel: v-cache entries 1 + i = (q, v + eps e_i): first pass of the ABA on the cached base q-part
// VSP (LinPlan::vc_sparse): lane g stores the records of its subtree (K in g .. sub_end - 1: the ones its step changes) into its v-step
// deltas (vc + vown + K * 18) and every other record onto the v-step base block (vc), and lane nv runs the chain unstepped and stores the
// whole base block: outside g's subtree the lanes g and nv execute the same instructions on the same operands.  Selected
// addresses, as in the configuration fill
template <class T, int K, bool VSP>
__device__ __forceinline__ void vc_joint(const DevModel& m, const double* __restrict__ qc, const double* __restrict__ xg, int iv, double eps,
                                         double (&vel)[T::N][6], double* __restrict__ vc, int vown, int sub_end) {
  constexpr int o = T::prismatic[K] ? 3 : 0;
  const double* E = qc + K * rbd::QC_STRIDE;
  const double* r = E + 9;
  const double* Ia = E + 19;
  const double* a = m.axis[K];
  double vK = xg[T::N + K];
  if (K == iv) vK = vK + eps;
  double vJ[6], vrec[18];
  step_joint_motion<o>(a, vK, vJ);
  step_link_vel<(T::parent[K] < 0)>(E, r, vel[T::parent[K] >= 0 ? T::parent[K] : 0], vJ, vel[K]);
  step_vpart(m.I6[K], Ia, vel[K], vJ, vrec);
  int voff = K * rbd::VC_STRIDE;
  if constexpr (VSP) voff = (K >= iv) & (K < sub_end) ? vown + K * rbd::VC_STRIDE : voff;
  double* vo = vc + voff;
#pragma unroll
  for (int k = 0; k < 18; ++k) vo[k] = vrec[k];
  __builtin_amdgcn_sched_barrier(0);
}
template <class T, bool VSP, int... Ks>
__device__ __forceinline__ void vc_all(const DevModel& m, const double* __restrict__ qc, const double* __restrict__ xg, int iv, double eps,
                                       double (&vel)[T::N][6], double* __restrict__ vc, int vown, int sub_end, std::integer_sequence<int, Ks...>) {
  (vc_joint<T, Ks, VSP>(m, qc, xg, iv, eps, vel, vc, vown, sub_end), ...);
}
template <class T, bool VSP>
__global__ __launch_bounds__(LBS) void lin_static_vcache_kernel(LinParams p, const DevModel* __restrict__ model, const double* __restrict__ xs,
                                                                const double* __restrict__ qcache, double* __restrict__ vcache) {
  constexpr int nv = T::N, n = 2 * nv;
  const int64_t bt = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t Tn = p.d.T;
  const int b = (int)(bt / Tn);
  const int64_t t = bt % Tn;
  if (lane >= nv + (VSP ? 1 : 0)) return;
  const double* __restrict__ qc = qcache + bt * p.qc_bt;       // the base block
  const double* __restrict__ xg = xs + ((int64_t)b * (Tn + 1) + t) * n;
  double* vc0 = vcache + bt * p.vc_bt;
  double* vc = vc0 + (VSP ? VcLayout<T>::VB : (1 + lane) * (nv * rbd::VC_STRIDE));
  const int g = lane < nv ? lane : 0;
  const int vown = g_vc_tab<T>.voff[g] - g * rbd::VC_STRIDE - VcLayout<T>::VB;   // counted from vc
  const int sub_end = lane < nv ? g + g_vc_tab<T>.sub[g] : 0;
  double vel[nv][6];
  vc_all<T, VSP>(*model, qc, xg, lane, sqrt(sqrt(DBL_EPSILON)), vel, vc, vown, sub_end, std::make_integer_sequence<int, nv>{});
}

}  // namespace

int lin_static_supported(const DevModel& m) {
  if (m.ff) return 0;            // compiled-in topologies are trees of 1-DoF joints
  if (topo_matches<TopoTalos38>(m)) return 1;
  if (topo_matches<TopoChain6>(m)) return 2;
#define DDP_TOPO_MATCH(ID, TOPO) if (topo_matches<TOPO>(m)) return (ID) - 1;   // generated topologies: lin_path ID, internal id ID - 1
  DDP_TOPO_EXTRA(DDP_TOPO_MATCH)
#undef DDP_TOPO_MATCH
  return 0;
}

// doubles of workspace one (instance, t) needs at the configuration level
// (the larger of: the sweep's 8 doubles per joint and lane, which the first-order q columns and the full-ABA level need, and
// the pairs' spine records)
int64_t lin_static_qc_per_bt(int topo) {
  if (topo == 1) return QcLayout<TopoTalos38>::WORDS;
  if (topo == 2) return QcLayout<TopoChain6>::WORDS;
#define DDP_TOPO_QC(ID, TOPO) if (topo == (ID) - 1) return QcLayout<TOPO>::WORDS;
  DDP_TOPO_EXTRA(DDP_TOPO_QC)
#undef DDP_TOPO_QC
  return 0;
}

// doubles per (instance, t) of the base + deltas v-cache (LinPlan::vc_sparse)
int64_t lin_static_vc_per_bt(int topo) {
  if (topo == 1) return VcLayout<TopoTalos38>::WORDS;
  if (topo == 2) return VcLayout<TopoChain6>::WORDS;
#define DDP_TOPO_VC(ID, TOPO) if (topo == (ID) - 1) return VcLayout<TOPO>::WORDS;
  DDP_TOPO_EXTRA(DDP_TOPO_VC)
#undef DDP_TOPO_VC
  return 0;
}

int64_t lin_static_ws_per_bt(const DevModel& m) {
  const int64_t nv = m.nv, TRI = nv * (nv - 1) / 2, GU = (TRI + LBS - 1) / LBS;
  int64_t rec = 0;
  for (int i = 0; i < nv; ++i)
    for (int j = i + 1; j < nv; ++j) {
      const auto anc = [&](int a, int x) { for (int k = m.parent[x]; k >= 0; k = m.parent[k]) if (k == a) return true; return false; };
      int a = m.parent[i];
      while (a >= 0 && !anc(a, j)) a = m.parent[a];
      for (; a >= 0; a = m.parent[a]) ++rec;
    }
  const int64_t sweep = GU * nv * WS_PER_JOINT * LBS, splice = rec * SREC;
  return sweep > splice ? sweep : splice;
}

// the kernels that exist for both q-cache layouts, each launched in the form LinParams::qc_sparse names
template <class T>
static void launch_qvcache(const LinParams& p, int64_t BT, hipStream_t s) {
  const dim3 grid((unsigned)((BT * p.ncfg + LBS - 1) / LBS));
  if (p.vc_sparse) hipLaunchKernelGGL((lin_static_qvcache_kernel<T, true, true>), grid, dim3(LBS), 0, s, p, p.model, p.x, p.qcache, p.vcache);
  else if (p.qc_sparse) hipLaunchKernelGGL((lin_static_qvcache_kernel<T, true>), grid, dim3(LBS), 0, s, p, p.model, p.x, p.qcache, p.vcache);
  else hipLaunchKernelGGL((lin_static_qvcache_kernel<T, false>), grid, dim3(LBS), 0, s, p, p.model, p.x, p.qcache, p.vcache);
}
template <class T>
static void launch_tau_rows(const LinParams& p, int64_t BT, hipStream_t s) {
  const dim3 grid((unsigned)(BT * 2 * T::N));
  if (p.vc_sparse) hipLaunchKernelGGL((lin_static_tau_kernel<T, true, false, true, true>), grid, dim3(LBS), 0, s, p);
  else if (p.qc_sparse) hipLaunchKernelGGL((lin_static_tau_kernel<T, true, false, true>), grid, dim3(LBS), 0, s, p);
  else hipLaunchKernelGGL((lin_static_tau_kernel<T, true>), grid, dim3(LBS), 0, s, p);
}
template <class T>
static void launch_vel_rows(const LinParams& p, int64_t BT, hipStream_t s) {
  const dim3 grid((unsigned)(BT * T::N));
  if (p.qc_sparse) hipLaunchKernelGGL((lin_static_vel_kernel<T, true, true>), grid, dim3(LBS), 0, s, p);
  else hipLaunchKernelGGL((lin_static_vel_kernel<T, true>), grid, dim3(LBS), 0, s, p);
}

// the diagonal second-order entries of the u directions, from the resident f_u
template <class T>
static void launch_u_diagonal(ddp_hip_ctx* ctx, const LinParams& p) {
  const int64_t BT = ctx->d.batch * ctx->d.T;
  if (ctx->sw.first_scalar) hipLaunchKernelGGL((lin_static_first_kernel<T, 3, true>), dim3((unsigned)BT), dim3(LBS), 0, ctx->stream, p, p.model, p.qcache, p.x, p.u, ctx->lin_qws, (int64_t)0);
  else hipLaunchKernelGGL((lin_static_first_tau_kernel<T, true>), dim3((unsigned)BT), dim3(LBS), 0, ctx->stream, p);
}

// the first-order kernels along the q, v and (with_u) u directions: jacobian columns, or accelerations with p.accel_out set;
// u_diag: the u waves go on to the diagonal columns of f_uu (StaticLevel::FirstOrderUDiag, never with the scalar-path kernels)
template <class T>
static void launch_first_columns(ddp_hip_ctx* ctx, const LinParams& p, bool with_u, bool u_diag = false) {
  const int64_t BT = ctx->d.batch * ctx->d.T;
  constexpr int nv = T::N, TRI = nv * (nv - 1) / 2, GU = (TRI + LBS - 1) / LBS;
  const int64_t per = ctx->lin_qws_bt * GU;     // one wave per (instance, t) uses one of the GU workspace slots of a slice entry
  for (int64_t bt0 = 0; bt0 < BT; bt0 += per) {
    const int64_t nb = BT - bt0 < per ? BT - bt0 : per;
    hipLaunchKernelGGL((lin_static_first_kernel<T, 1, false>), dim3((unsigned)nb), dim3(LBS), 0, ctx->stream, p, p.model, p.qcache, p.x, p.u, ctx->lin_qws, bt0);
  }
  hipLaunchKernelGGL((lin_static_first_kernel<T, 2, false>), dim3((unsigned)BT), dim3(LBS), 0, ctx->stream, p, p.model, p.qcache, p.x, p.u, ctx->lin_qws, (int64_t)0);
  if (!with_u) return;
  // (DDP_HIP_FIRST_SCALAR: the u waves walk the cache blocks through the scalar path)
  if (ctx->sw.first_scalar) hipLaunchKernelGGL((lin_static_first_kernel<T, 3, false>), dim3((unsigned)BT), dim3(LBS), 0, ctx->stream, p, p.model, p.qcache, p.x, p.u, ctx->lin_qws, (int64_t)0);
  else if (u_diag) hipLaunchKernelGGL((lin_static_first_tau_fused_kernel<T>), dim3((unsigned)BT), dim3(2 * LBS), 0, ctx->stream, p);
  else hipLaunchKernelGGL((lin_static_first_tau_kernel<T, false>), dim3((unsigned)BT), dim3(LBS), 0, ctx->stream, p);
}

// the configuration level's slices on `s`: spine pre-pass, then the pair kernel on spliced operands, in slices of (instance, t)
// whose spine records share the workspace.  The workspace is sized for lin_qws_bt sweeps (lin_static_ws_per_bt: the first-order q
// columns run one); a spine set is smaller, so a slice holds more of them (Talos: 4.2 x; few long launches instead of many short
// ones).  rows_done (or null): an event the first pair kernel waits for, behind its spine pre-pass (LIN_FORK_SPINE)
template <class T>
static int launch_cfg_slices(ddp_hip_ctx* ctx, const LinParams& p, hipStream_t s, hipEvent_t rows_done) {
  const int64_t BT = ctx->d.batch * ctx->d.T;
  constexpr int nv = T::N, TRI = nv * (nv - 1) / 2, GU = (TRI + LBS - 1) / LBS;
  constexpr int64_t NREC = spine_records<T>(), SWEEP = (int64_t)GU * nv * WS_PER_JOINT * LBS;
  constexpr int64_t WS_BT = SWEEP > NREC * SREC ? SWEEP : NREC * SREC;
  const int64_t per = NREC > 0 ? ctx->lin_qws_bt * WS_BT / (NREC * SREC) : BT;
  for (int64_t bt0 = 0; bt0 < BT; bt0 += per) {
    const int nb = (int)(BT - bt0 < per ? BT - bt0 : per);
    const dim3 grid((unsigned)((nb + 7) / 8 * 8 * GU));
    if (p.qc_sparse) hipLaunchKernelGGL((lin_static_spine_kernel<T, true>), grid, dim3(LBS), 0, s, p.model, p.qcache, p.qc_bt, p.vcache, p.vc_bt, ctx->lin_qws, bt0, nb);
    else hipLaunchKernelGGL((lin_static_spine_kernel<T, false>), grid, dim3(LBS), 0, s, p.model, p.qcache, p.qc_bt, p.vcache, p.vc_bt, ctx->lin_qws, bt0, nb);
    if (rows_done) { HIP_TRY(hipStreamWaitEvent(s, rows_done, 0)); rows_done = nullptr; }
    if (p.qc_sparse) hipLaunchKernelGGL((lin_static_cfg_pair_kernel<T, true>), grid, dim3(LBS), 0, s, p, ctx->lin_qws, bt0, nb);
    else hipLaunchKernelGGL((lin_static_cfg_pair_kernel<T, false>), grid, dim3(LBS), 0, s, p, ctx->lin_qws, bt0, nb);
  }
  return DDP_HIP_OK;
}

// Mode 2's second order under the concurrent schedule (LinPlan::forks; the reads and writes of every kernel: DESIGN.md section
// 4r).  The u diagonal and the torque rows come first: the rows read every first-order column and the u diagonal, and leave the
// q / v diagonal columns every other point reads.  Behind them the configuration slices run on the side stream beside the (u, u)
// pairs and the velocity level: every off-diagonal point, its mirror image included, belongs to one kernel, so the two branches
// write disjoint columns in every layout.  The first spine pre-pass reads the caches alone and writes the workspace, which the
// first order's q columns are done with at this point of the stream: it starts beside the u diagonal.  Each fork is taken only
// with its LinFork bit; without it the kernels keep their place in the single-stream order.  The caller joins the side stream
// (lin.hip: ahead of the bracket's end).  u_diag_done: the first order's u waves have left the u diagonal already
// (StaticLevel::FirstOrderUDiag); the spine pre-pass then starts beside the torque rows alone.
template <class T>
static int launch_second_order(ddp_hip_ctx* ctx, const LinParams& p, bool u_diag_done) {
  const int64_t BT = ctx->d.batch * ctx->d.T;
  constexpr int nv = T::N, TRI = nv * (nv - 1) / 2, GU = (TRI + LBS - 1) / LBS;
  const bool fork_cfg = (ctx->plan.forks & LIN_FORK_CFG) != 0, spine_ahead = fork_cfg && (ctx->plan.forks & LIN_FORK_SPINE);
  hipStream_t s0 = ctx->stream;
  if (spine_ahead) HIP_TRY(lin_fork(ctx));
  if (!u_diag_done) launch_u_diagonal<T>(ctx, p);
  launch_tau_rows<T>(p, BT, s0);
  if (fork_cfg) {
    if (spine_ahead) HIP_TRY(hipEventRecord(ctx->lin_ev_rows, s0));
    else HIP_TRY(lin_fork(ctx));                    // (taken behind the rows: nothing more to wait for)
    const int rc_ = launch_cfg_slices<T>(ctx, p, ctx->lin_stream2, spine_ahead ? ctx->lin_ev_rows : nullptr);
    if (rc_ != DDP_HIP_OK) return rc_;
  }
  if (p.pack) hipLaunchKernelGGL((lin_static_tau_kernel<T, false, true>), dim3((unsigned)(BT * GU)), dim3(LBS), 0, s0, p);
  else hipLaunchKernelGGL((lin_static_tau_kernel<T, false, false>), dim3((unsigned)(BT * GU)), dim3(LBS), 0, s0, p);
  launch_vel_rows<T>(p, BT, s0);
  hipLaunchKernelGGL((lin_static_vel_kernel<T, false>), dim3((unsigned)(BT * GU)), dim3(LBS), 0, s0, p);
  if (!fork_cfg) { const int rc_ = launch_cfg_slices<T>(ctx, p, s0, nullptr); if (rc_ != DDP_HIP_OK) return rc_; }
  return DDP_HIP_OK;
}

template <class T>
static int lin_static_launch_t(ddp_hip_ctx* ctx, const LinParams& p, StaticLevel level) {
  const int64_t BT = ctx->d.batch * ctx->d.T;
  constexpr int nv = T::N, TRI = nv * (nv - 1) / 2, GU = (TRI + LBS - 1) / LBS;
  if (level == StaticLevel::Torque) {             // torque-level points (replaces lin_offdiag_kernel<NJ, 3>)
    launch_tau_rows<T>(p, BT, ctx->stream);
    if (p.pack) hipLaunchKernelGGL((lin_static_tau_kernel<T, false, true>), dim3((unsigned)(BT * GU)), dim3(LBS), 0, ctx->stream, p);
    else hipLaunchKernelGGL((lin_static_tau_kernel<T, false, false>), dim3((unsigned)(BT * GU)), dim3(LBS), 0, ctx->stream, p);
  } else if (level == StaticLevel::Caches) {
    launch_qvcache<T>(p, BT, ctx->stream);
    if (p.nvcfg > 1 && p.vc_sparse) hipLaunchKernelGGL((lin_static_vcache_kernel<T, true>), dim3((unsigned)BT), dim3(LBS), 0, ctx->stream, p, p.model, p.x, p.qcache, p.vcache);
    else if (p.nvcfg > 1) hipLaunchKernelGGL((lin_static_vcache_kernel<T, false>), dim3((unsigned)BT), dim3(LBS), 0, ctx->stream, p, p.model, p.x, p.qcache, p.vcache);
  } else if (level == StaticLevel::AccelXU || level == StaticLevel::AccelX) {   // -> p.accel_out, after the base caches
    if (!p.accel_out) return DDP_HIP_E_ARG;
    launch_qvcache<T>(p, BT, ctx->stream);
    launch_first_columns<T>(ctx, p, level == StaticLevel::AccelXU);
  } else if (level == StaticLevel::FirstOrder) {
    launch_first_columns<T>(ctx, p, true);
  } else if (level == StaticLevel::FirstOrderUDiag) {
    if (ctx->sw.first_scalar || !p.fuu) return DDP_HIP_E_ARG;   // (lin.hip asks for it on the staged kernels of a context with tensors alone)
    launch_first_columns<T>(ctx, p, true, true);
  } else if (level == StaticLevel::SecondOrder || level == StaticLevel::SecondOrderAfterUDiag) {
    { const int rc_ = launch_second_order<T>(ctx, p, level == StaticLevel::SecondOrderAfterUDiag); if (rc_ != DDP_HIP_OK) return rc_; }
  } else if (level == StaticLevel::UDiagonal) {
    // diagonal second-order entries of the u directions; those of the q and v directions are formed by the torque-level
    // row kernel (Torque) on an otherwise idle lane, which therefore runs ahead of Velocity and Configuration
    launch_u_diagonal<T>(ctx, p);
  } else if (level == StaticLevel::Configuration && !ctx->sw.cfg_full_aba) {
    { const int rc_ = launch_cfg_slices<T>(ctx, p, ctx->stream, nullptr); if (rc_ != DDP_HIP_OK) return rc_; }
  } else if (level == StaticLevel::Configuration) {
    // DDP_HIP_CFG_FULL_ABA (development A/B): every point runs the whole articulated-body algorithm.
    // In slices of (instance, t), so that the per-wave workspace stays small.  The sweep kernel of slice k+1 (one wave per
    // SIMD, long waves) and the acceleration / output kernel of slice k run on two streams with two workspaces: each
    // fills the other's tail instead of leaving the chip to drain between launches.
    const int64_t per = ctx->lin_qws_bt;
    hipStream_t s0 = ctx->stream, s1 = ctx->lin_stream2;
    int k = 0;
    for (int64_t bt0 = 0; bt0 < BT; bt0 += per, ++k) {
      const int64_t nb = BT - bt0 < per ? BT - bt0 : per;
      const int w = k & 1;
      double* ws = w ? ctx->lin_qws2 : ctx->lin_qws;
      // a failed wait / record would silently turn into a race on the shared workspace: every return code is checked
      if (k >= 2) HIP_TRY(hipStreamWaitEvent(s0, ctx->lin_ev_dn[w], 0));        // slice k-2 is done with this workspace
      hipLaunchKernelGGL((lin_static_cfg_up_kernel<T>), dim3((unsigned)(nb * GU)), dim3(LBS), 0, s0, p, p.model, p.qcache, p.x, p.u, ws, bt0);
      HIP_TRY(hipEventRecord(ctx->lin_ev_up[w], s0));
      HIP_TRY(hipStreamWaitEvent(s1, ctx->lin_ev_up[w], 0));
      hipLaunchKernelGGL((lin_static_cfg_down_kernel<T>), dim3((unsigned)(nb * GU)), dim3(LBS), 0, s1, p, p.model, p.qcache, p.x, p.u, ws, bt0);
      HIP_TRY(hipEventRecord(ctx->lin_ev_dn[w], s1));
    }
    if (k >= 1) HIP_TRY(hipStreamWaitEvent(s0, ctx->lin_ev_dn[0], 0));
    if (k >= 2) HIP_TRY(hipStreamWaitEvent(s0, ctx->lin_ev_dn[1], 0));
  } else if (level == StaticLevel::Velocity) {
    launch_vel_rows<T>(p, BT, ctx->stream);
    hipLaunchKernelGGL((lin_static_vel_kernel<T, false>), dim3((unsigned)(BT * GU)), dim3(LBS), 0, ctx->stream, p);
  }
  HIP_TRY(hipGetLastError());
  return DDP_HIP_OK;
}

int lin_static_launch(ddp_hip_ctx* ctx, const LinParams& p, StaticLevel level) {
  if (ctx->plan.topo == 1) return lin_static_launch_t<TopoTalos38>(ctx, p, level);
  if (ctx->plan.topo == 2) return lin_static_launch_t<TopoChain6>(ctx, p, level);
#define DDP_TOPO_LAUNCH(ID, TOPO) if (ctx->plan.topo == (ID) - 1) return lin_static_launch_t<TOPO>(ctx, p, level);
  DDP_TOPO_EXTRA(DDP_TOPO_LAUNCH)
#undef DDP_TOPO_LAUNCH
  return DDP_HIP_E_UNSUPPORTED;
}
