// lin_common.h -- parameter block shared by the linearisation translation units (lin.hip, lin_static.hip)
#pragma once
#include "internal.h"

struct LinParams {
  Dims d;
  const DevModel* model;
  const int64_t* ne;
  const int64_t* Epre;
  const double* target;
  const double *x, *u;
  double *lfx, *lfxx, *lx, *lu, *lxx, *lux, *luu;
  double *f_val, *fx, *fu, *fxx, *fux, *fuu;
  double *eq_val, *eq_x, *eq_u, *eq_xx, *eq_ux, *eq_uu;
  int32_t has_tensors;
  double *eq_xk, *eq_fxk, *eq_c;   // large-model constraint chain workspace: x_1..x_K | f_x(x_1..x_{K-1}) | base jacobian
  double* vcache;   // [batch*T][2nv+1][nv*VC_STRIDE]: (q, v)-dependent part at (q,v), (q, v+eps e_i), (q+eps e_i, v);
                    // with vc_sparse, per (instance, t): entry 0, the v-step base block and the records a step changes (lin_static.hip: VcLayout)
  int64_t vc_bt;    // doubles per (instance, t) of the v-cache: nvcfg * nv * VC_STRIDE, or VcLayout::WORDS
  int32_t vc_sparse;   // LinPlan::vc_sparse
  double* qcache;   // [batch*T][nv+1][nv*QC_STRIDE]: q-dependent part of the ABA at the base q and at q + eps e_i (mode 2);
                    // with qc_sparse, per (instance, t): the base block and the records a step changes (lin_static.hip: QcLayout)
  int64_t qc_bt;    // doubles per (instance, t) of the q-cache: ncfg * nv * QC_STRIDE, or QcLayout::WORDS
  int32_t qc_sparse;   // LinPlan::qc_sparse
  int32_t skip_qv_mirror;   // static stencil: do not write the mirror images f_xx(:, i, j), f_uu(:, i, j), i < j, of the symmetric pairs --
                            // the backward sweep never reads them when it knows the tensors symmetric (bwd_split.h: only the columns
                            // j >= c of slab c); formed on demand for any other reader (lin.hip: lin_materialize_fxx)
  int32_t skip_top;         // static stencil: the configuration rows k < nv of a tensor column are exact zeros except at k = (first
                            // direction) mod nv and k = (second direction) mod nv -- q+ = q + dt v is affine, and row k of every stencil
                            // point but those two is bit for bit the base point's -- so only those two and the rows k >= nv are formed
                            // and stored; the other rows hold the zeros lin.hip: tensor_zero_top_kernel left there
  int32_t pack;             // static stencil (with skip_top and skip_qv_mirror): the tensors are left as packed records, not in the contract
                            // layout.  A slab keeps its base address; inside it column j is the record [top0, top1, rows nv .. n-1] of
                            // nv + 2 doubles at slab + j (nv + 2): top0 the entry of row (slab direction) mod nv, top1 that of row j mod nv
                            // where it is another row (x columns only); f_uu's tops are never written.  K3h streams the records
                            // (bwd_split.h); any other reader has them unpacked first (lin.hip: lin_materialize_fxx)
  double* accel_out;     // static first-order kernels, levels 1 and 2: when set, the wave stores the accelerations of its nv perturbed
                         // points, [pair][3 nv directions: q, v, u | the unperturbed point][nv], instead of the jacobian columns (lin_analytic.hip: mode 1 reads them)
  int32_t ncfg, nvcfg;   // entries per (instance, t) of the q- / v-cache: nv+1 / 2nv+1 with the mode-2 stencil resident,
                         // 1 / 1 when only the first order is formed (tensor-free contexts: base configuration and base (q, v))
  const double *xref, *wx, *uref, *wu;   // tracking cost (DDP_HIP_FLAG_TRACKING_COST), else null
};

constexpr int LBS = 64;

// static-topology second-order path (lin_static.hip): returns non-zero when the model's tree matches a compiled-in
// topology; the launcher covers the velocity- and torque-level stencil points of finite_diff_hessian_compute mode 2
int lin_static_supported(const DevModel& m);   // 0: none, else the id of the compiled-in topology
enum class StaticLevel {
  Caches,          // the q- and v-caches every other level reads
  FirstOrder,      // f_x, f_u: the first-order kernels along q, v, u
  UDiagonal,       // mode 2: diagonal second-order entries of the u directions
  Torque,          // mode 2: torque-level stencil points (and the diagonal entries of the q and v directions)
  Velocity,        // mode 2: velocity-level stencil points
  Configuration,   // mode 2: (q_i, q_j) stencil points
  SecondOrder,     // mode 2, concurrent schedule (LinPlan::forks): UDiagonal, Torque, Velocity and Configuration as one launch graph
  FirstOrderUDiag, // FirstOrder whose u waves also leave the u diagonal of f_uu (a call that runs both orders of a mode-2 context)
  SecondOrderAfterUDiag,   // SecondOrder behind FirstOrderUDiag: without UDiagonal
  AccelX,          // mode 1: accelerations at x + sqrt(eps_mach) e_k into p.accel_out (builds the base caches itself)
  AccelXU,         // ... and at u + sqrt(eps_mach) e_k
};
int lin_static_launch(ddp_hip_ctx* ctx, const LinParams& p, StaticLevel level);   // DDP_HIP_OK or an error code
int64_t lin_static_ws_per_bt(const DevModel& m);
int64_t lin_static_qc_per_bt(int topo);   // doubles per (instance, t) of the base + deltas q-cache of a compiled-in topology (LinPlan::qc_sparse)
int64_t lin_static_vc_per_bt(int topo);   // ... of its base + deltas v-cache (LinPlan::vc_sparse)

// analytic first order / mode-1 second order of large tree models (lin_analytic.hip): stage 0 = f_x, f_u at the
// trajectory points (problem.hpp:463-503), stage 1 = forward differences of those jacobians (problem.hpp:67-150)
int lin_analytic_setup(ddp_hip_ctx* ctx);
void lin_analytic_teardown(ddp_hip_ctx* ctx);
// flags: LIN_ANA_F the dynamics' outputs, LIN_ANA_EQ the constraint chain's (problem.hpp:569-620 on the analytic jacobians)
constexpr int LIN_ANA_F = 1, LIN_ANA_EQ = 2;
constexpr int LIN_ANA_ACCEL = 4;   // stage 0: the mode-1 pass follows in this linearisation call -- form its accelerations now and take the trajectory point's from them
int lin_analytic_launch(ddp_hip_ctx* ctx, const LinParams& p, LinCall& call, int stage, int flags);
// free-flyer models: analytic f_x at the constraint chain's look-ahead states x_1 .. x_{K-1} (after lin.hip: eq_chain_kernel)
int lin_analytic_ff_lookahead(ddp_hip_ctx* ctx, const LinParams& p);
