// ctx.hip -- context life cycle, resident sequences, profiling.  gfx950 only.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <new>

#include "internal.h"

extern "C" int ddp_hip_abi_version(void) { return DDP_HIP_ABI_VERSION; }

extern "C" const char* ddp_hip_strerror(int code) {
  switch (code) {
    case DDP_HIP_OK: return "ok";
    case DDP_HIP_EV_LLT_RESTART: return "backward sweep restarted after a non-positive LLT pivot";
    case DDP_HIP_EV_LINESEARCH_FLOOR: return "line search reached step < 1e-10";
    case DDP_HIP_E_ARG: return "invalid argument";
    case DDP_HIP_E_HIP: return "HIP runtime error";
    case DDP_HIP_E_NODEVICE: return "no HIP device (there is no CPU fallback)";
    case DDP_HIP_E_UNSUPPORTED: return "unsupported configuration";
    case DDP_HIP_E_MAX_RESTARTS: return "backward sweep exceeded max_restarts";
    case DDP_HIP_E_COMM: return "RCCL error";
    default: return "unknown";
  }
}

extern "C" int ddp_hip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

static void pack_body_inertia(const ddp_hip_model* m, int i, double* out21) {
  // spatial inertia [Ic + m cx cx^T, m cx; m cx^T, m 1] (Featherstone RBDA eq. 2.63), lower triangle
  double I6[6][6];
  memset(I6, 0, sizeof(I6));
  const double* c = m->com + 3 * i;
  double mass = m->mass_j[i];
  double cx[3][3] = {{0, -c[2], c[1]}, {c[2], 0, -c[0]}, {-c[1], c[0], 0}};
  for (int k = 0; k < 3; ++k)
    for (int l = 0; l < 3; ++l) {
      double cc = 0;
      for (int j = 0; j < 3; ++j) cc += cx[k][j] * cx[l][j];
      I6[k][l] = m->Ic[9 * i + 3 * k + l] + mass * cc;
      I6[k][l + 3] = mass * cx[k][l];
      I6[k + 3][l] = mass * cx[l][k];
    }
  I6[3][3] = I6[4][4] = I6[5][5] = mass;
  int p = 0;
  for (int r = 0; r < 6; ++r)
    for (int cc2 = 0; cc2 <= r; ++cc2) out21[p++] = I6[r][cc2];
}

// Slot tables for the small-state tree traversals (rbd.h: aba_u_cached).  Leaf->root (descending index): a joint's
// accumulator is allocated when its largest-index child contributes and freed once the joint itself is processed.
// Root->leaf (ascending index): a joint's value is kept from when it is processed until its largest-index child
// has read it.  For a humanoid tree a handful of slots suffice.
static bool build_slot_tables(DevModel& dm) {
  const int N = dm.nj;
  int largest_child[DDP_MAXJ];
  for (int i = 0; i < N; ++i) { dm.has_child[i] = 0; largest_child[i] = -1; dm.slot_up[i] = -1; dm.slot_down[i] = -1; }
  for (int i = 0; i < N; ++i)
    if (dm.parent[i] >= 0) { dm.has_child[dm.parent[i]] = 1; if (i > largest_child[dm.parent[i]]) largest_child[dm.parent[i]] = i; }
  for (int i = 0; i < N; ++i) {
    const int par = dm.parent[i];
    dm.first_contrib[i] = dm.last_child[i] = (par >= 0 && largest_child[par] == i) ? 1 : 0;
  }
  const int MAXS = 16;
  bool used[MAXS];
  int n_slots = 0;
  for (int k = 0; k < MAXS; ++k) used[k] = false;
  for (int i = N - 1; i >= 0; --i) {            // leaf -> root
    const int par = dm.parent[i];
    if (par >= 0 && dm.first_contrib[i]) {
      int k = 0;
      while (k < MAXS && used[k]) ++k;
      if (k == MAXS) return false;
      used[k] = true;
      dm.slot_up[par] = k;
      if (k + 1 > n_slots) n_slots = k + 1;
    }
    if (dm.slot_up[i] >= 0) used[dm.slot_up[i]] = false;   // the joint is processed: its accumulator is consumed
  }
  for (int k = 0; k < MAXS; ++k) used[k] = false;
  for (int i = 0; i < N; ++i) {                 // root -> leaf
    if (dm.has_child[i]) {
      int k = 0;
      while (k < MAXS && used[k]) ++k;
      if (k == MAXS) return false;
      used[k] = true;
      dm.slot_down[i] = k;
      if (k + 1 > n_slots) n_slots = k + 1;
    }
    const int par = dm.parent[i];
    if (par >= 0 && dm.last_child[i]) used[dm.slot_down[par]] = false;
  }
  dm.n_slots = n_slots;
  // level schedule + children lists
  int level[DDP_MAXJ];
  int nl = 0;
  for (int i = 0; i < N; ++i) { level[i] = dm.parent[i] >= 0 ? level[dm.parent[i]] + 1 : 0; if (level[i] + 1 > nl) nl = level[i] + 1; }
  dm.n_levels = nl;
  dm.max_level_width = 0;
  int pos = 0;
  for (int L = 0; L < nl; ++L) {
    dm.lvl_start[L] = pos;
    for (int i = 0; i < N; ++i) if (level[i] == L) dm.lvl_joint[pos++] = i;
    if (pos - dm.lvl_start[L] > dm.max_level_width) dm.max_level_width = pos - dm.lvl_start[L];
  }
  dm.lvl_start[nl] = pos;
  pos = 0;
  for (int i = 0; i < N; ++i) {
    dm.child_start[i] = pos;
    for (int c = N - 1; c > i; --c) if (dm.parent[c] == i) dm.child_list[pos++] = c;
  }
  dm.child_start[N] = pos;
  return n_slots <= 8;   // rbd::MAX_SLOTS
}

// the model table of the C-ABI as the device-side DevModel (shared with model_api.hip)
void ddp_hip_fill_dev_model(const ddp_hip_model* mo, DevModel& dm) {
  memset(&dm, 0, sizeof(dm));
  dm.kind = mo->kind; dm.nv = mo->nv; dm.mass = mo->mass; dm.length = mo->length;
  dm.ff = (mo->kind == DDP_HIP_MODEL_TREE && mo->jtype && mo->jtype[0] == DDP_HIP_JOINT_FREEFLYER) ? 1 : 0;
  dm.nj = dm.ff ? mo->nv - 5 : mo->nv;
  dm.nq = dm.ff ? mo->nv + 1 : mo->nv;
  for (int k = 0; k < 3; ++k) dm.gravity[k] = mo->gravity[k];
  if (mo->kind != DDP_HIP_MODEL_TREE) return;
  for (int i = 0; i < dm.nj; ++i) {
    dm.parent[i] = mo->parent[i]; dm.jtype[i] = mo->jtype[i];
    for (int k = 0; k < 3; ++k) { dm.axis[i][k] = mo->axis[3 * i + k]; dm.pp[i][k] = mo->pp[3 * i + k]; }
    for (int k = 0; k < 9; ++k) dm.Rp[i][k] = mo->Rp[9 * i + k];
    pack_body_inertia(mo, i, dm.I6[i]);
  }
}
bool ddp_hip_build_tables(DevModel& dm) { return build_slot_tables(dm); }

static int64_t seq_size_of(const Dims& d, int s) {
  const int64_t T = d.T, n = d.n, m = d.m, nx = d.nx, E = d.Etot;
  switch (s) {
    case DDP_HIP_SEQ_X: case DDP_HIP_SEQ_X_NEW: return (T + 1) * nx;
    case DDP_HIP_SEQ_U: case DDP_HIP_SEQ_U_NEW: return T * m;
    case DDP_HIP_SEQ_LFX: return n;
    case DDP_HIP_SEQ_LFXX: return n * n;
    case DDP_HIP_SEQ_LX: return T * n;
    case DDP_HIP_SEQ_LU: return T * m;
    case DDP_HIP_SEQ_LXX: return T * n * n;
    case DDP_HIP_SEQ_LUX: return T * m * n;
    case DDP_HIP_SEQ_LUU: return T * m * m;
    case DDP_HIP_SEQ_F_VAL: return T * nx;
    case DDP_HIP_SEQ_FX: return T * n * n;
    case DDP_HIP_SEQ_FU: return T * n * m;
    case DDP_HIP_SEQ_FXX: return T * n * n * n;
    case DDP_HIP_SEQ_FUX: return T * n * m * n;
    case DDP_HIP_SEQ_FUU: return T * n * m * m;
    case DDP_HIP_SEQ_EQ_VAL: return E;
    case DDP_HIP_SEQ_EQ_X: return E * n;
    case DDP_HIP_SEQ_EQ_U: return E * m;
    case DDP_HIP_SEQ_EQ_XX: return E * n * n;
    case DDP_HIP_SEQ_EQ_UX: return E * m * n;
    case DDP_HIP_SEQ_EQ_UU: return E * m * m;
    case DDP_HIP_SEQ_MULT_ORIGIN: return T * nx;
    case DDP_HIP_SEQ_MULT_VAL: return E;
    case DDP_HIP_SEQ_MULT_JAC: return E * n;
    case DDP_HIP_SEQ_FB_ORIGIN: return T * nx;
    case DDP_HIP_SEQ_FB_VAL: return T * m;
    case DDP_HIP_SEQ_FB_JAC: return T * m * n;
    case DDP_HIP_SEQ_VX_TRACE: return T * n;
    case DDP_HIP_SEQ_VXX_TRACE: return T * n * n;
    case DDP_HIP_SEQ_COSTS_OLD: case DDP_HIP_SEQ_COSTS_NEW: return T + 1;
    case DDP_HIP_SEQ_COST_XREF: return (T + 1) * nx;
    case DDP_HIP_SEQ_COST_WX: return (T + 1) * n;
    case DDP_HIP_SEQ_COST_UREF: case DDP_HIP_SEQ_COST_WU: return T * m;
    case DDP_HIP_SEQ_CTRL_LO: case DDP_HIP_SEQ_CTRL_HI: return T * m;
    case DDP_HIP_SEQ_BOX_STAT: return T * 2;
    default: return -1;
  }
}

static bool is_tensor_seq(int s) {
  return s == DDP_HIP_SEQ_FXX || s == DDP_HIP_SEQ_FUX || s == DDP_HIP_SEQ_FUU || s == DDP_HIP_SEQ_EQ_XX ||
         s == DDP_HIP_SEQ_EQ_UX || s == DDP_HIP_SEQ_EQ_UU;
}
static bool is_trace_seq(int s) { return s == DDP_HIP_SEQ_VX_TRACE || s == DDP_HIP_SEQ_VXX_TRACE; }
static bool is_cost_seq(int s) { return s >= DDP_HIP_SEQ_COST_XREF && s <= DDP_HIP_SEQ_COST_WU; }
static bool is_box_seq(int s) { return s >= DDP_HIP_SEQ_CTRL_LO && s <= DDP_HIP_SEQ_BOX_STAT; }
static bool nan_init_seq(int s) {
  // mat_seq_t storage is NaN-poisoned at construction (detail/mat_seq.hpp:34-37); uninit_derivative_storage
  // then zeroes every derivative sequence except f_val, and leaves lfx / lfxx NaN (ddp.hpp:441-442,476-511)
  return s == DDP_HIP_SEQ_LFX || s == DDP_HIP_SEQ_LFXX || s == DDP_HIP_SEQ_F_VAL || s == DDP_HIP_SEQ_FB_ORIGIN ||
         s == DDP_HIP_SEQ_FB_VAL || s == DDP_HIP_SEQ_FB_JAC || s == DDP_HIP_SEQ_X || s == DDP_HIP_SEQ_U ||
         s == DDP_HIP_SEQ_X_NEW || s == DDP_HIP_SEQ_U_NEW || is_trace_seq(s);
}

__global__ void fill_kernel(double* p, int64_t n, double v) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = v;
}

static int fill_device(ddp_hip_ctx* ctx, double* p, int64_t n, double v) {
  if (n <= 0) return DDP_HIP_OK;
  if (v == 0.0) {
    HIP_TRY(hipMemsetAsync(p, 0, (size_t)n * sizeof(double), ctx->stream));
    return DDP_HIP_OK;
  }
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(fill_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, p, n, v);
  HIP_TRY(hipGetLastError());
  return DDP_HIP_OK;
}

// A term's arrays as they are at create: allocated (once) for max_items, every side at its fill value over that whole capacity,
// the term off, laid out by `items`.  ddp_hip_create, and the set_frames / set_points entry points when the layout changes
static int cost_block_setup(ddp_hip_ctx* ctx, int term, int32_t items) {
  CostBlock& k = ctx->cost[term];
  const int64_t slots = ctx->d.batch * cost_rows(k, ctx->d.T) * k.max_items;
  for (int s = 0; s < k.desc->nside; ++s) {
    const int64_t words = slots * k.desc->unit[s];
    const int fill = k.desc->fill[s];
    if (!k.side[s]) HIP_TRY(hipMalloc(&k.side[s], sizeof(double) * (size_t)words));
    if (fill == FILL_QUAT) {   // (a zero-filled quaternion has no rotation)
      std::vector<double> qt((size_t)words, 0.0);
      for (size_t i = 3; i < qt.size(); i += 4) qt[i] = 1.0;
      HIP_TRY(hipMemcpyAsync(k.side[s], qt.data(), sizeof(double) * qt.size(), hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(hipStreamSynchronize(ctx->stream));
    } else {
      const int rc = fill_device(ctx, k.side[s], words, fill == FILL_NEG_INF ? -INFINITY : fill == FILL_POS_INF ? INFINITY : 0.0);
      if (rc != DDP_HIP_OK) return rc;
    }
  }
  k.items = items;
  k.live = false;
  ctx->adv_dirty = true;   // (the advance's descriptor table goes by the layout)
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_create(const ddp_hip_problem* prob, int device, uint32_t flags, ddp_hip_ctx** out) {
  if (!prob || !out) return DDP_HIP_E_ARG;
  *out = nullptr;
  const ddp_hip_model& mo = prob->model;
  if (prob->T < 1 || prob->batch < 1 || mo.nv < 1 || mo.nv > DDP_MAXJ) return DDP_HIP_E_ARG;
  if (mo.kind != DDP_HIP_MODEL_PENDULUM && mo.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_ARG;
  if (mo.kind == DDP_HIP_MODEL_PENDULUM && mo.nv != 1) return DDP_HIP_E_ARG;
  if (prob->fd_mode < 0 || prob->fd_mode > 2) return DDP_HIP_E_ARG;
  if ((flags & DDP_HIP_FLAG_FRAME_COST) && mo.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_UNSUPPORTED;   // frames are points of a tree's joints
  if ((flags & DDP_HIP_FLAG_FRAME_ORIENT_COST) && !(flags & DDP_HIP_FLAG_FRAME_COST)) return DDP_HIP_E_ARG;   // the orientation terms are of the cost frames
  if ((flags & DDP_HIP_FLAG_FRAME_VEL_COST) && !(flags & DDP_HIP_FLAG_FRAME_COST)) return DDP_HIP_E_ARG;   // the velocity terms alike
  if ((flags & DDP_HIP_FLAG_OBSTACLE_COST) && mo.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_UNSUPPORTED;   // collision points are points of a tree's joints
  if ((flags & DDP_HIP_FLAG_SELF_COLLISION_COST) && mo.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_UNSUPPORTED;   // the spheres alike
  if ((flags & DDP_HIP_FLAG_CAPSULE_COST) && mo.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_UNSUPPORTED;   // ... and the capsules
  if ((flags & DDP_HIP_FLAG_RELATIVE_FRAME_COST) && mo.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_UNSUPPORTED;   // the frame pairs alike
  if ((flags & DDP_HIP_FLAG_CONTROL_GRAV_COST) && mo.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_UNSUPPORTED;   // g(q) is of a tree's bodies
  if ((flags & DDP_HIP_FLAG_FRAME_AIM_COST) && mo.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_UNSUPPORTED;   // aim frames are frames of a tree's joints
  if (flags & DDP_HIP_FLAG_JOINT_ACCEL_COST) {
    if (mo.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_UNSUPPORTED;   // a = aba(q, v, u) of a tree
    if (mo.nv > DDP_HIP_MAX_JOINT_ACCEL_NV) return DDP_HIP_E_UNSUPPORTED;   // the recursion's LDS record beside the jacobian: the 38 instantiation alone
  }
  if (flags & (DDP_HIP_FLAG_COM_COST | DDP_HIP_FLAG_MOMENTUM_COST | DDP_HIP_FLAG_BALANCE_REGION_COST)) {
    if (mo.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_UNSUPPORTED;   // the CoM, the momentum about it and the capture point are of a tree's bodies
    if (!mo.mass_j || !mo.jtype) return DDP_HIP_E_ARG;
    double total = 0.0;
    for (int i = 0; i < (mo.jtype[0] == DDP_HIP_JOINT_FREEFLYER ? mo.nv - 5 : mo.nv); ++i) total += mo.mass_j[i];
    if (!(total > 0.0) || !isfinite(total)) return DDP_HIP_E_ARG;      // c(q) divides by the total mass
  }
  if (prob->eq_kind != DDP_HIP_EQ_NONE && (!prob->ne || prob->eq_advance < 0 || prob->eq_advance > 4)) return DDP_HIP_E_ARG;
  if (prob->eq_kind == DDP_HIP_EQ_FRAME && (mo.kind != DDP_HIP_MODEL_TREE || prob->frame_joint < 0 ||
                                            prob->frame_joint >= (mo.jtype && mo.jtype[0] == DDP_HIP_JOINT_FREEFLYER ? mo.nv - 5 : mo.nv)))
    return DDP_HIP_E_ARG;
  bool ff = false;
  if (mo.kind == DDP_HIP_MODEL_TREE) {
    if (!mo.parent || !mo.jtype || !mo.axis || !mo.Rp || !mo.pp || !mo.mass_j || !mo.com || !mo.Ic) return DDP_HIP_E_ARG;
    ff = mo.jtype[0] == DDP_HIP_JOINT_FREEFLYER;
    const int nj = ff ? mo.nv - 5 : mo.nv;
    if (nj < 1 || (ff && mo.parent[0] != -1)) return DDP_HIP_E_ARG;
    for (int i = 0; i < nj; ++i) {
      if (mo.parent[i] >= i || mo.parent[i] < -1) return DDP_HIP_E_ARG;
      if (i > 0 && mo.jtype[i] != DDP_HIP_JOINT_REVOLUTE && mo.jtype[i] != DDP_HIP_JOINT_PRISMATIC) return DDP_HIP_E_ARG;   // one free flyer, at the root
    }
    // Lie-group configurations: forward-differenced (the north star) or analytic jacobians (lin_analytic.hip:
    // ana_ff_first_kernel, the reference's own first order), mode 0 / mode 2 / tensor-free only -- the reference's mode 1
    // asserts nq == nv itself (problem.hpp:78-81); the config constraint subtracts configurations (problem.hpp:785-790),
    // meaningless on a quaternion: frame constraints only
    if (ff && (prob->fd_mode == 1 || prob->eq_kind == DDP_HIP_EQ_CONFIG)) return DDP_HIP_E_UNSUPPORTED;
  }
  int ndev = ddp_hip_device_count();
  if (ndev <= 0) return DDP_HIP_E_NODEVICE;
  if (device < 0 || device >= ndev) return DDP_HIP_E_ARG;
  HIP_TRY(hipSetDevice(device));

  ddp_hip_ctx* ctx = new (std::nothrow) ddp_hip_ctx();
  if (!ctx) return DDP_HIP_E_HIP;
  ctx->device = device;
  ctx->flags = flags;
  ctx->sw = read_switches();
  if (hipDeviceGetAttribute(&ctx->cu_count, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) { delete ctx; return DDP_HIP_E_HIP; }
  ctx->active_h.assign((size_t)prob->batch, 1);
  Dims& d = ctx->d;
  d.T = prob->T; d.nv = mo.nv; d.n = 2 * (int64_t)mo.nv; d.m = mo.nv; d.nx = 2 * (int64_t)mo.nv + (ff ? 1 : 0); d.batch = prob->batch;
  ctx->ne_h.assign((size_t)d.T, 0);
  ctx->Epre_h.assign((size_t)d.T + 1, 0);
  d.emax = 0;
  for (int64_t t = 0; t < d.T; ++t) {
    int64_t e = (prob->eq_kind != DDP_HIP_EQ_NONE && prob->ne) ? prob->ne[t] : 0;
    if (e < 0) { delete ctx; return DDP_HIP_E_ARG; }
    if (prob->eq_kind == DDP_HIP_EQ_CONFIG && e != 0 && e != mo.nv) { delete ctx; return DDP_HIP_E_ARG; }
    if (prob->eq_kind == DDP_HIP_EQ_FRAME && e != 0 && e != 3) { delete ctx; return DDP_HIP_E_ARG; }
    ctx->ne_h[(size_t)t] = e;
    ctx->Epre_h[(size_t)t + 1] = ctx->Epre_h[(size_t)t] + e;
    if (e > d.emax) d.emax = e;
  }
  d.Etot = ctx->Epre_h[(size_t)d.T];

#define CTX_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e__ = (expr);                                                       \
    if (e__ != hipSuccess) { (void)hipGetLastError(); ddp_hip_destroy(ctx); return DDP_HIP_E_HIP; } \
  } while (0)

  CTX_TRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  CTX_TRY(hipMalloc(&ctx->ne_d, sizeof(int64_t) * (size_t)d.T));
  CTX_TRY(hipMalloc(&ctx->Epre_d, sizeof(int64_t) * (size_t)(d.T + 1)));
  CTX_TRY(hipMemcpy(ctx->ne_d, ctx->ne_h.data(), sizeof(int64_t) * (size_t)d.T, hipMemcpyHostToDevice));
  CTX_TRY(hipMemcpy(ctx->Epre_d, ctx->Epre_h.data(), sizeof(int64_t) * (size_t)(d.T + 1), hipMemcpyHostToDevice));
  if (d.Etot > 0) {
    if (!prob->eq_target) { ddp_hip_destroy(ctx); return DDP_HIP_E_ARG; }
    CTX_TRY(hipMalloc(&ctx->target_d, sizeof(double) * (size_t)d.Etot));
    CTX_TRY(hipMemcpy(ctx->target_d, prob->eq_target, sizeof(double) * (size_t)d.Etot, hipMemcpyHostToDevice));
  }

  DevModel& dm = ctx->model_h;
  ddp_hip_fill_dev_model(&mo, dm);
  for (int k = 0; k < 3; ++k) dm.frame_off[k] = prob->frame_off[k];
  dm.dt = prob->dt; dm.c = prob->c;
  dm.eq_kind = prob->eq_kind; dm.eq_advance = prob->eq_advance; dm.frame_joint = prob->frame_joint;
  dm.first_order_fd = prob->first_order_fd; dm.fd_mode = prob->fd_mode;
  if (mo.kind == DDP_HIP_MODEL_TREE && !build_slot_tables(dm)) { ddp_hip_destroy(ctx); return DDP_HIP_E_UNSUPPORTED; }
  CTX_TRY(hipMalloc(&ctx->model_d, sizeof(DevModel)));
  CTX_TRY(hipMemcpy(ctx->model_d, &dm, sizeof(DevModel), hipMemcpyHostToDevice));

  const double qnan = std::numeric_limits<double>::quiet_NaN();
  for (int s = 0; s < DDP_HIP_SEQ_COUNT; ++s) {
    int64_t sz = seq_size_of(d, s);
    if (!(flags & DDP_HIP_FLAG_CONTROL_BOUNDS) && is_box_seq(s)) sz = 0;   // (ddp_hip_seq_size: 0, uploads refused)
    ctx->seq[s].size = sz;
    if ((flags & DDP_HIP_FLAG_NO_TENSORS) && is_tensor_seq(s)) continue;
    if (!(flags & DDP_HIP_FLAG_TRACE) && is_trace_seq(s)) continue;
    if (!(flags & DDP_HIP_FLAG_TRACKING_COST) && is_cost_seq(s)) continue;
    if (sz <= 0) continue;
    CTX_TRY(hipMalloc(&ctx->seq[s].ptr, sizeof(double) * (size_t)(sz * d.batch)));
    const double v0 = s == DDP_HIP_SEQ_CTRL_LO ? -INFINITY : s == DDP_HIP_SEQ_CTRL_HI ? INFINITY : nan_init_seq(s) ? qnan : 0.0;
    if (fill_device(ctx, ctx->seq[s].ptr, sz * d.batch, v0) != DDP_HIP_OK) {
      ddp_hip_destroy(ctx);
      return DDP_HIP_E_HIP;
    }
  }
  if (flags & DDP_HIP_FLAG_TRACKING_COST) {
    // the reference state starts at the neutral state at every t (weights and reference controls start at 0): a zero-filled
    // root quaternion would make the cost NaN even under zero weights
    std::vector<double> xr((size_t)(ctx->seq[DDP_HIP_SEQ_COST_XREF].size * d.batch), 0.0);
    if (ff)
      for (size_t k = 0; k < xr.size(); k += (size_t)d.nx) xr[k + 6] = 1.0;
    CTX_TRY(hipMemcpyAsync(ctx->seq[DDP_HIP_SEQ_COST_XREF].ptr, xr.data(), sizeof(double) * xr.size(), hipMemcpyHostToDevice, ctx->stream));
    CTX_TRY(hipStreamSynchronize(ctx->stream));
  }
  for (int term = 0; term < COST_COUNT; ++term) {
    // frames, aim frames, frame pairs, region planes, obstacle slots, self-collision pairs and capsule pairs: no layout until they are set; limits (lo = -inf, hi = +inf, w = 0: no limit anywhere), CoM, momentum
    // and control-gravity (one item per control row, T rows): fixed
    CostBlock& k = ctx->cost[term];
    k.desc = &kCostDesc[term];
    k.max_items = k.desc->max_items == COST_ITEMS_STATE ? (int32_t)d.n : k.desc->max_items == COST_ITEMS_CONTROL ? (int32_t)d.m :
                  k.desc->max_items == COST_ITEMS_VELOCITY ? (int32_t)d.nv : k.desc->max_items;
    if (!(flags & k.desc->flag)) continue;
    const int rc_ = cost_block_setup(ctx, term, k.desc->fixed ? k.max_items : 0);
    if (rc_ != DDP_HIP_OK) { ddp_hip_destroy(ctx); return rc_; }
  }
  if (flags & DDP_HIP_FLAG_OBSTACLE_COST) CTX_TRY(hipMalloc(&ctx->ob_clear_d, sizeof(double) * (size_t)(d.batch * (d.T + 1))));
  if (flags & DDP_HIP_FLAG_SELF_COLLISION_COST) CTX_TRY(hipMalloc(&ctx->sc_clear_d, sizeof(double) * (size_t)(d.batch * (d.T + 1))));
  if (flags & DDP_HIP_FLAG_CAPSULE_COST) CTX_TRY(hipMalloc(&ctx->cp_clear_d, sizeof(double) * (size_t)(d.batch * (d.T + 1))));
  if (flags & DDP_HIP_FLAG_RELATIVE_FRAME_COST)
    CTX_TRY(hipMalloc(&ctx->rf_err_d, sizeof(double) * (size_t)(d.batch * (d.T + 1) * DDP_HIP_MAX_FRAME_PAIRS * 6)));
  if (flags & DDP_HIP_FLAG_FRAME_AIM_COST)
    CTX_TRY(hipMalloc(&ctx->fa_err_d, sizeof(double) * (size_t)(d.batch * (d.T + 1) * DDP_HIP_MAX_AIM_FRAMES * 2)));
  if (flags & DDP_HIP_FLAG_JOINT_ACCEL_COST) CTX_TRY(hipMalloc(&ctx->ja_acc_d, sizeof(double) * (size_t)(d.batch * d.T * d.nv)));
  if (flags & DDP_HIP_FLAG_BALANCE_REGION_COST) CTX_TRY(hipMalloc(&ctx->br_margin_d, sizeof(double) * (size_t)(d.batch * (d.T + 1))));
  int rc = bwd_setup(ctx);
  if (rc == DDP_HIP_OK) rc = fwd_setup(ctx);
  if (rc == DDP_HIP_OK) rc = lin_setup(ctx);
  if (rc != DDP_HIP_OK) { ddp_hip_destroy(ctx); return rc; }
  CTX_TRY(hipStreamSynchronize(ctx->stream));
#undef CTX_TRY
  *out = ctx;
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_destroy(ddp_hip_ctx* ctx) {
  if (!ctx) return DDP_HIP_E_ARG;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  lin_teardown(ctx);
  adv_teardown(ctx);
  fwd_teardown(ctx);
  bwd_teardown(ctx);
  for (int s = 0; s < DDP_HIP_SEQ_COUNT; ++s)
    if (ctx->seq[s].ptr) (void)hipFree(ctx->seq[s].ptr);
  for (CostBlock& k : ctx->cost) {
    for (double* p : k.side)
      if (p) (void)hipFree(p);
    if (k.cand) (void)hipFree(k.cand);
  }
  if (ctx->ob_clear_d) (void)hipFree(ctx->ob_clear_d);
  for (double* p : ctx->og_phi)
    if (p) (void)hipFree(p);
  if (ctx->og_d2) (void)hipFree(ctx->og_d2);
  if (ctx->og_occ) (void)hipFree(ctx->og_occ);
  if (ctx->sc_clear_d) (void)hipFree(ctx->sc_clear_d);
  if (ctx->cp_clear_d) (void)hipFree(ctx->cp_clear_d);
  if (ctx->rf_err_d) (void)hipFree(ctx->rf_err_d);
  if (ctx->fa_err_d) (void)hipFree(ctx->fa_err_d);
  if (ctx->ja_acc_d) (void)hipFree(ctx->ja_acc_d);
  if (ctx->br_margin_d) (void)hipFree(ctx->br_margin_d);
  if (ctx->ne_d) (void)hipFree(ctx->ne_d);
  if (ctx->Epre_d) (void)hipFree(ctx->Epre_d);
  if (ctx->target_d) (void)hipFree(ctx->target_d);
  if (ctx->model_d) (void)hipFree(ctx->model_d);
  for (int k = 0; k < DDP_HIP_K_COUNT; ++k) {
    for (auto e : ctx->prof[k].starts) (void)hipEventDestroy(e);
    for (auto e : ctx->prof[k].stops) (void)hipEventDestroy(e);
  }
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return DDP_HIP_OK;
}

extern "C" void* ddp_hip_stream(ddp_hip_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

extern "C" int ddp_hip_synchronize(ddp_hip_ctx* ctx) {
  if (!ctx) return DDP_HIP_E_ARG;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DDP_HIP_OK;
}

extern "C" int64_t ddp_hip_batch(const ddp_hip_ctx* ctx) { return ctx ? ctx->d.batch : -1; }

extern "C" int64_t ddp_hip_seq_size(const ddp_hip_ctx* ctx, int seq) {
  if (!ctx || seq < 0 || seq >= DDP_HIP_SEQ_COUNT) return -1;
  return ctx->seq[seq].size;
}

extern "C" double* ddp_hip_device_ptr(ddp_hip_ctx* ctx, int seq) {
  if (!ctx || seq < 0 || seq >= DDP_HIP_SEQ_COUNT) return nullptr;
  if (seq == DDP_HIP_SEQ_FXX || seq == DDP_HIP_SEQ_FUX || seq == DDP_HIP_SEQ_FUU) (void)hipSetDevice(ctx->device);   // (the tensors may have to be unpacked, the mirror images formed)
  if (tensors_written_outside(ctx, seq) != DDP_HIP_OK) return nullptr;   // the caller may write through the pointer
  return ctx->seq[seq].ptr;
}

static int check_range(ddp_hip_ctx* ctx, int seq, int64_t first, int64_t count) {
  if (!ctx || seq < 0 || seq >= DDP_HIP_SEQ_COUNT) return DDP_HIP_E_ARG;
  if (first < 0 || count < 0 || first + count > ctx->d.batch) return DDP_HIP_E_ARG;
  if (ctx->seq[seq].size > 0 && !ctx->seq[seq].ptr) return DDP_HIP_E_UNSUPPORTED;  // not allocated under the create flags
  return DDP_HIP_OK;
}

// what the tracking cost accepts (DDP_HIP_FLAG_TRACKING_COST): finite, non-negative weights; unit root quaternions
// (cost_weight_ok, cost_quat_ok: cost_block.h)

// what a control bound accepts (DDP_HIP_FLAG_CONTROL_BOUNDS): no NaN, no lower bound of +inf, no upper bound of -inf
static bool bound_ok(int seq, double v) { return !isnan(v) && !(seq == DDP_HIP_SEQ_CTRL_LO ? v == INFINITY : v == -INFINITY); }

static bool cost_values_ok(const ddp_hip_ctx* ctx, int seq, const double* host, int64_t words) {
  if (seq == DDP_HIP_SEQ_CTRL_LO || seq == DDP_HIP_SEQ_CTRL_HI) {
    for (int64_t i = 0; i < words; ++i)
      if (!bound_ok(seq, host[i])) return false;
    return true;
  }
  if (seq == DDP_HIP_SEQ_COST_WX || seq == DDP_HIP_SEQ_COST_WU) {
    for (int64_t i = 0; i < words; ++i)
      if (!cost_weight_ok(host[i])) return false;
  } else if (seq == DDP_HIP_SEQ_COST_XREF && ctx->model_h.ff) {
    for (int64_t k = 0; k < words; k += ctx->d.nx) {
      const double* qt = host + k + 3;
      if (!cost_quat_ok(qt[0] * qt[0] + qt[1] * qt[1] + qt[2] * qt[2] + qt[3] * qt[3])) return false;
    }
  }
  return true;
}

extern "C" int ddp_hip_upload(ddp_hip_ctx* ctx, int seq, const double* host, int64_t first, int64_t count) {
  int rc = check_range(ctx, seq, first, count);
  if (rc != DDP_HIP_OK) return rc;
  int64_t sz = ctx->seq[seq].size;
  if (is_box_seq(seq) && !(ctx->flags & DDP_HIP_FLAG_CONTROL_BOUNDS)) return DDP_HIP_E_UNSUPPORTED;
  if (sz == 0 || count == 0) return DDP_HIP_OK;
  if (!host) return DDP_HIP_E_ARG;
  if (!cost_values_ok(ctx, seq, host, sz * count)) return DDP_HIP_E_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  { const int rc_ = tensors_written_outside(ctx, seq); if (rc_ != DDP_HIP_OK) return rc_; }
  HIP_TRY(hipMemcpyAsync(ctx->seq[seq].ptr + first * sz, host, sizeof(double) * (size_t)(sz * count), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (seq == DDP_HIP_SEQ_CTRL_LO || seq == DDP_HIP_SEQ_CTRL_HI) ctx->box_dirty = true;
  return DDP_HIP_OK;
}

// lo <= hi can only be checked once both sequences are there: the sweeps ask before they launch, and the bounds are read
// back only after an upload of either
int box_check(ddp_hip_ctx* ctx) {
  if (!ctx->box_dirty) return DDP_HIP_OK;
  const size_t words = (size_t)(ctx->seq[DDP_HIP_SEQ_CTRL_LO].size * ctx->d.batch);
  std::vector<double> lo(words), hi(words);
  HIP_TRY(hipMemcpyAsync(lo.data(), ctx->seq[DDP_HIP_SEQ_CTRL_LO].ptr, sizeof(double) * words, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipMemcpyAsync(hi.data(), ctx->seq[DDP_HIP_SEQ_CTRL_HI].ptr, sizeof(double) * words, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < words; ++i)
    if (lo[i] > hi[i]) return DDP_HIP_E_ARG;
  ctx->box_dirty = false;
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_download(ddp_hip_ctx* ctx, int seq, double* host, int64_t first, int64_t count) {
  int rc = check_range(ctx, seq, first, count);
  if (rc != DDP_HIP_OK) return rc;
  int64_t sz = ctx->seq[seq].size;
  if (sz == 0 || count == 0) return DDP_HIP_OK;
  if (!host) return DDP_HIP_E_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  if (seq == DDP_HIP_SEQ_FXX || seq == DDP_HIP_SEQ_FUU || (seq == DDP_HIP_SEQ_FUX && ctx->tensors.packed)) { const int rc_ = lin_materialize_fxx(ctx); if (rc_ != DDP_HIP_OK) return rc_; }
  HIP_TRY(hipMemcpyAsync(host, ctx->seq[seq].ptr + first * sz, sizeof(double) * (size_t)(sz * count), hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_fill(ddp_hip_ctx* ctx, int seq, double value) {
  int rc = check_range(ctx, seq, 0, 0);
  if (rc != DDP_HIP_OK) return rc;
  if ((seq == DDP_HIP_SEQ_COST_WX || seq == DDP_HIP_SEQ_COST_WU) && !cost_weight_ok(value)) return DDP_HIP_E_ARG;
  if (seq == DDP_HIP_SEQ_COST_XREF && ctx->model_h.ff && !cost_quat_ok(4 * value * value)) return DDP_HIP_E_ARG;
  if ((seq == DDP_HIP_SEQ_CTRL_LO || seq == DDP_HIP_SEQ_CTRL_HI) && !bound_ok(seq, value)) return DDP_HIP_E_ARG;
  if (seq == DDP_HIP_SEQ_CTRL_LO || seq == DDP_HIP_SEQ_CTRL_HI) ctx->box_dirty = true;
  HIP_TRY(hipSetDevice(ctx->device));
  { const int rc_ = tensors_written_outside(ctx, seq); if (rc_ != DDP_HIP_OK) return rc_; }
  return fill_device(ctx, ctx->seq[seq].ptr, ctx->seq[seq].size * ctx->d.batch, value);
}

// ---- the add-on cost terms (cost_block.h): one upload path, one download path ------------------------------
// host[s] == nullptr leaves side s as it is.  The order of the checks is part of the interface: null context, flag, range, layout,
// every side of the whole range (cost_upload_check), and only then the device: `before_copy` (state limits), the candidates'
// array at the first non-zero weight, the copies, one synchronise, the live rule
static int cost_block_upload(ddp_hip_ctx* ctx, int term, const double* const* host, const CostSideOk* ok, int64_t first, int64_t count,
                             int (*before_copy)(ddp_hip_ctx*, const double* const*, int64_t, int64_t) = nullptr) {
  if (!ctx) return DDP_HIP_E_ARG;
  CostBlock& k = ctx->cost[term];
  const Dims& d = ctx->d;
  CostCheck c;
  c.items = k.items; c.ff = ctx->model_h.ff != 0; c.kind = term == COST_CAPSULE ? ctx->cp_kind : ctx->ob_kind; c.rows = cost_rows(k, d.T);
  bool copy, nonzero;
  const int rc = cost_upload_check(ctx->flags, k, c, d.batch, d.T, host, ok, first, count, &copy, &nonzero);
  if (rc != DDP_HIP_OK || !copy) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  if (before_copy) { const int rc_ = before_copy(ctx, host, first, count); if (rc_ != DDP_HIP_OK) return rc_; }
  // the candidates' term array of the line search exists from the first non-zero weight on (fwd.hip: addon_terms)
  if (nonzero && k.desc->cand && !k.cand) HIP_TRY(hipMalloc(&k.cand, sizeof(double) * (size_t)(d.batch * ctx->n_alpha_max * (d.T + 1))));
  for (int s = 0; s < k.desc->nside; ++s) {
    const int64_t sz = cost_side_words(k, s, d.T);
    if (host[s]) HIP_TRY(hipMemcpyAsync(k.side[s] + first * sz, host[s], sizeof(double) * (size_t)(sz * count), hipMemcpyHostToDevice, ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (host[k.desc->nside - 1]) k.live = cost_live_rule(k.live, nonzero, first, count, d.batch);
  return DDP_HIP_OK;
}

static int cost_block_download(ddp_hip_ctx* ctx, int term, double* const* host, int64_t first, int64_t count) {
  if (!ctx) return DDP_HIP_E_ARG;
  const CostBlock& k = ctx->cost[term];
  const int rc = cost_range_check(ctx->flags, k, ctx->d.batch, first, count);
  if (rc != DDP_HIP_OK) return rc;
  bool any = false;
  for (int s = 0; s < k.desc->nside; ++s) any |= host[s] != nullptr;
  if (k.items == 0 || count == 0 || !any) return DDP_HIP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  for (int s = 0; s < k.desc->nside; ++s) {
    const int64_t sz = cost_side_words(k, s, ctx->d.T);
    if (host[s]) HIP_TRY(hipMemcpyAsync(host[s], k.side[s] + first * sz, sizeof(double) * (size_t)(sz * count), hipMemcpyDeviceToHost, ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return DDP_HIP_OK;
}

// frames shared by the batch: of the position, orientation and velocity terms
extern "C" int ddp_hip_frame_cost_set_frames(ddp_hip_ctx* ctx, int32_t n_frames, const int32_t* joint, const double* off) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_FRAME_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (n_frames < 1 || n_frames > DDP_HIP_MAX_COST_FRAMES || !joint || !off) return DDP_HIP_E_ARG;
  for (int f = 0; f < n_frames; ++f) {
    if (joint[f] < 0 || joint[f] >= ctx->model_h.nj) return DDP_HIP_E_ARG;
    for (int a = 0; a < 3; ++a)
      if (!isfinite(off[3 * f + a])) return DDP_HIP_E_ARG;
  }
  if (n_frames != ctx->fc_nf) {
    // another count is another layout: the three terms' data start again as at create
    HIP_TRY(hipSetDevice(ctx->device));
    for (int term : {COST_FRAME, COST_ORIENT, COST_FRAME_VEL})
      if (ctx->flags & kCostDesc[term].flag) { const int rc_ = cost_block_setup(ctx, term, n_frames); if (rc_ != DDP_HIP_OK) return rc_; }
  }
  ctx->fc_nf = n_frames;
  for (int f = 0; f < n_frames; ++f) {
    ctx->fc_joint[f] = joint[f];
    for (int a = 0; a < 3; ++a) ctx->fc_off[f][a] = off[3 * f + a];
  }
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_frame_cost_upload(ddp_hip_ctx* ctx, const double* target, const double* weight, int64_t first, int64_t count) {
  const double* host[] = {target, weight};
  const CostSideOk ok[] = {cost_finite_side, cost_weight_side};
  return cost_block_upload(ctx, COST_FRAME, host, ok, first, count);
}
extern "C" int ddp_hip_frame_cost_download(ddp_hip_ctx* ctx, double* target, double* weight, int64_t first, int64_t count) {
  double* host[] = {target, weight};
  return cost_block_download(ctx, COST_FRAME, host, first, count);
}

extern "C" int ddp_hip_frame_orient_upload(ddp_hip_ctx* ctx, const double* quat, const double* weight, int64_t first, int64_t count) {
  const double* host[] = {quat, weight};
  const CostSideOk ok[] = {cost_quat_side, cost_weight_side};
  return cost_block_upload(ctx, COST_ORIENT, host, ok, first, count);
}
extern "C" int ddp_hip_frame_orient_download(ddp_hip_ctx* ctx, double* quat, double* weight, int64_t first, int64_t count) {
  double* host[] = {quat, weight};
  return cost_block_download(ctx, COST_ORIENT, host, first, count);
}

extern "C" int ddp_hip_frame_vel_upload(ddp_hip_ctx* ctx, const double* target, const double* weight, int64_t first, int64_t count) {
  const double* host[] = {target, weight};
  const CostSideOk ok[] = {cost_finite_side, cost_weight_side};
  return cost_block_upload(ctx, COST_FRAME_VEL, host, ok, first, count);
}
extern "C" int ddp_hip_frame_vel_download(ddp_hip_ctx* ctx, double* target, double* weight, int64_t first, int64_t count) {
  double* host[] = {target, weight};
  return cost_block_download(ctx, COST_FRAME_VEL, host, first, count);
}

// collision points and slot kinds shared by the batch; geometry and weights per (instance, t, slot)
extern "C" int ddp_hip_obstacle_set_points(ddp_hip_ctx* ctx, int32_t n_points, const int32_t* joint, const double* off, const double* radius,
                                           int32_t n_obstacles, const int32_t* kind) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_OBSTACLE_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (n_points < 1 || n_points > DDP_HIP_MAX_COLLISION_POINTS || n_obstacles < 1 || n_obstacles > DDP_HIP_MAX_OBSTACLES) return DDP_HIP_E_ARG;
  if (!joint || !off || !radius || !kind) return DDP_HIP_E_ARG;
  for (int k = 0; k < n_points; ++k) {
    if (joint[k] < 0 || joint[k] >= ctx->model_h.nj) return DDP_HIP_E_ARG;
    for (int a = 0; a < 3; ++a)
      if (!isfinite(off[3 * k + a])) return DDP_HIP_E_ARG;
    if (!isfinite(radius[k]) || radius[k] < 0.0) return DDP_HIP_E_ARG;
  }
  for (int o = 0; o < n_obstacles; ++o)
    if (kind[o] != DDP_HIP_OBSTACLE_SPHERE && kind[o] != DDP_HIP_OBSTACLE_HALFSPACE &&
        !(kind[o] == DDP_HIP_OBSTACLE_GRID && ctx->og_cur >= 0))   // (a grid slot needs a grid: ddp_hip_obstacle_set_grid / _set_occupancy first)
      return DDP_HIP_E_ARG;
  bool same = n_points == ctx->ob_np && n_obstacles == ctx->ob_no;
  for (int o = 0; same && o < n_obstacles; ++o) same = kind[o] == ctx->ob_kind[o];
  if (!same) {
    // other counts are another layout, other kinds another meaning of the four doubles: geometry and weights start again at 0
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc_ = cost_block_setup(ctx, COST_OBSTACLE, n_obstacles);
    if (rc_ != DDP_HIP_OK) return rc_;
  }
  ctx->ob_np = n_points;
  ctx->ob_no = n_obstacles;
  for (int k = 0; k < n_points; ++k) {
    ctx->ob_joint[k] = joint[k];
    ctx->ob_radius[k] = radius[k];
    for (int a = 0; a < 3; ++a) ctx->ob_off[k][a] = off[3 * k + a];
  }
  for (int o = 0; o < n_obstacles; ++o) ctx->ob_kind[o] = kind[o];
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_obstacle_upload(ddp_hip_ctx* ctx, const double* geom, const double* weight, int64_t first, int64_t count) {
  const double* host[] = {geom, weight};
  const CostSideOk ok[] = {cost_obstacle_geom_side, cost_weight_side};
  return cost_block_upload(ctx, COST_OBSTACLE, host, ok, first, count);
}
extern "C" int ddp_hip_obstacle_download(ddp_hip_ctx* ctx, double* geom, double* weight, int64_t first, int64_t count) {
  double* host[] = {geom, weight};
  return cost_block_download(ctx, COST_OBSTACLE, host, first, count);
}

// spheres and pairs shared by the batch; a margin and a weight per (instance, t, pair)
extern "C" int ddp_hip_self_collision_set_pairs(ddp_hip_ctx* ctx, int32_t n_points, const int32_t* joint, const double* off, const double* radius,
                                                int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_b) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_SELF_COLLISION_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (n_points < 2 || n_points > DDP_HIP_MAX_COLLISION_POINTS || n_pairs < 1 || n_pairs > DDP_HIP_MAX_COLLISION_PAIRS) return DDP_HIP_E_ARG;
  if (!joint || !off || !radius || !pair_a || !pair_b) return DDP_HIP_E_ARG;
  for (int k = 0; k < n_points; ++k) {
    if (joint[k] < 0 || joint[k] >= ctx->model_h.nj) return DDP_HIP_E_ARG;
    for (int a = 0; a < 3; ++a)
      if (!isfinite(off[3 * k + a])) return DDP_HIP_E_ARG;
    if (!isfinite(radius[k]) || radius[k] < 0.0) return DDP_HIP_E_ARG;
  }
  if (!cost_pair_list_ok(n_points, joint, n_pairs, pair_a, pair_b)) return DDP_HIP_E_ARG;
  bool same = n_pairs == ctx->sc_npair;
  for (int i = 0; same && i < n_pairs; ++i) same = pair_a[i] == ctx->sc_pa[i] && pair_b[i] == ctx->sc_pb[i];
  if (!same) {
    // another list is another meaning of the per-pair data: margins and weights start again at 0
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc_ = cost_block_setup(ctx, COST_SELF_COLLISION, n_pairs);
    if (rc_ != DDP_HIP_OK) return rc_;
  }
  ctx->sc_np = n_points;
  ctx->sc_npair = n_pairs;
  for (int k = 0; k < n_points; ++k) {
    ctx->sc_joint[k] = joint[k];
    ctx->sc_radius[k] = radius[k];
    for (int a = 0; a < 3; ++a) ctx->sc_off[k][a] = off[3 * k + a];
  }
  for (int i = 0; i < n_pairs; ++i) { ctx->sc_pa[i] = pair_a[i]; ctx->sc_pb[i] = pair_b[i]; }
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_self_collision_upload(ddp_hip_ctx* ctx, const double* margin, const double* weight, int64_t first, int64_t count) {
  const double* host[] = {margin, weight};
  const CostSideOk ok[] = {cost_finite_side, cost_weight_side};
  return cost_block_upload(ctx, COST_SELF_COLLISION, host, ok, first, count);
}
extern "C" int ddp_hip_self_collision_download(ddp_hip_ctx* ctx, double* margin, double* weight, int64_t first, int64_t count) {
  double* host[] = {margin, weight};
  return cost_block_download(ctx, COST_SELF_COLLISION, host, first, count);
}

// robot capsules and pairs shared by the batch; eight doubles of geometry and a weight per (instance, t, pair)
extern "C" int ddp_hip_capsule_set_pairs(ddp_hip_ctx* ctx, int32_t n_capsules, const int32_t* joint, const double* end0, const double* end1,
                                         const double* radius, int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_kind,
                                         const int32_t* pair_b) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_CAPSULE_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (n_capsules < 1 || n_capsules > DDP_HIP_MAX_CAPSULES || n_pairs < 1 || n_pairs > DDP_HIP_MAX_CAPSULE_PAIRS) return DDP_HIP_E_ARG;
  if (!joint || !end0 || !end1 || !radius || !pair_a || !pair_kind || !pair_b) return DDP_HIP_E_ARG;
  for (int k = 0; k < n_capsules; ++k) {
    if (joint[k] < 0 || joint[k] >= ctx->model_h.nj) return DDP_HIP_E_ARG;
    for (int a = 0; a < 3; ++a)
      if (!isfinite(end0[3 * k + a]) || !isfinite(end1[3 * k + a])) return DDP_HIP_E_ARG;
    if (!isfinite(radius[k]) || radius[k] < 0.0) return DDP_HIP_E_ARG;
  }
  if (!cost_capsule_pairs_ok(n_capsules, joint, n_pairs, pair_a, pair_kind, pair_b, ctx->og_cur >= 0, ctx->cp_nbox)) return DDP_HIP_E_ARG;   // (a grid pair needs a grid, a box pair its box)
  bool same = n_capsules == ctx->cp_nc && n_pairs == ctx->cp_npair;
  for (int i = 0; same && i < n_pairs; ++i) same = pair_kind[i] == ctx->cp_kind[i];
  if (!same) {
    // other counts are another layout, other kinds another meaning of the eight doubles: geometry and weights start again at 0
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc_ = cost_block_setup(ctx, COST_CAPSULE, n_pairs);
    if (rc_ != DDP_HIP_OK) return rc_;
  }
  ctx->cp_nc = n_capsules;
  ctx->cp_npair = n_pairs;
  for (int k = 0; k < n_capsules; ++k) {
    ctx->cp_joint[k] = joint[k];
    ctx->cp_radius[k] = radius[k];
    for (int a = 0; a < 3; ++a) { ctx->cp_end[k][0][a] = end0[3 * k + a]; ctx->cp_end[k][1][a] = end1[3 * k + a]; }
  }
  for (int i = 0; i < n_pairs; ++i) {
    ctx->cp_pa[i] = pair_a[i];
    ctx->cp_kind[i] = pair_kind[i];
    ctx->cp_pb[i] = pair_kind[i] == DDP_HIP_CAPSULE_VS_ROBOT || pair_kind[i] == DDP_HIP_CAPSULE_VS_BOX ? pair_b[i] : 0;
  }
  return DDP_HIP_OK;
}

// the box shapes of the pairs of kind DDP_HIP_CAPSULE_VS_BOX, shared by the batch: context state like the capsules, read whenever a
// description is built for a launch
extern "C" int ddp_hip_capsule_set_boxes(ddp_hip_ctx* ctx, int32_t n_boxes, const double* half) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_CAPSULE_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (n_boxes < 0 || n_boxes > DDP_HIP_MAX_CAPSULE_BOXES || (n_boxes > 0 && !half)) return DDP_HIP_E_ARG;
  for (int k = 0; k < 3 * n_boxes; ++k)
    if (!isfinite(half[k]) || !(half[k] > 0.0)) return DDP_HIP_E_ARG;
  for (int i = 0; i < ctx->cp_npair; ++i)
    if (ctx->cp_kind[i] == DDP_HIP_CAPSULE_VS_BOX && ctx->cp_pb[i] >= n_boxes) return DDP_HIP_E_ARG;   // (a live pair keeps its box)
  ctx->cp_nbox = n_boxes;
  for (int k = 0; k < 3 * n_boxes; ++k) ctx->cp_half[k / 3][k % 3] = half[k];
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_capsule_upload(ddp_hip_ctx* ctx, const double* geom, const double* weight, int64_t first, int64_t count) {
  const double* host[] = {geom, weight};
  const CostSideOk ok[] = {cost_capsule_geom_side, cost_weight_side};
  return cost_block_upload(ctx, COST_CAPSULE, host, ok, first, count);
}
extern "C" int ddp_hip_capsule_download(ddp_hip_ctx* ctx, double* geom, double* weight, int64_t first, int64_t count) {
  double* host[] = {geom, weight};
  return cost_block_download(ctx, COST_CAPSULE, host, first, count);
}

// frame pairs shared by the batch; a target, a reference quaternion and six weights per (instance, t, pair)
extern "C" int ddp_hip_relative_frame_set_pairs(ddp_hip_ctx* ctx, int32_t n_pairs, const int32_t* joint_a, const double* off_a, const int32_t* joint_b,
                                                const double* off_b) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_RELATIVE_FRAME_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (n_pairs < 1 || n_pairs > DDP_HIP_MAX_FRAME_PAIRS || !joint_a || !off_a || !joint_b || !off_b) return DDP_HIP_E_ARG;
  if (!cost_frame_pairs_ok(ctx->model_h.nj, n_pairs, joint_a, off_a, joint_b, off_b)) return DDP_HIP_E_ARG;
  bool same = n_pairs == ctx->rf_np;
  for (int i = 0; same && i < n_pairs; ++i) same = joint_a[i] == ctx->rf_ja[i] && joint_b[i] == ctx->rf_jb[i];
  if (!same) {
    // other joints are another meaning of the per-pair data: targets and weights start again at 0, references at the identity
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc_ = cost_block_setup(ctx, COST_RELATIVE_FRAME, n_pairs);
    if (rc_ != DDP_HIP_OK) return rc_;
  }
  ctx->rf_np = n_pairs;
  for (int i = 0; i < n_pairs; ++i) {
    ctx->rf_ja[i] = joint_a[i];
    ctx->rf_jb[i] = joint_b[i];
    for (int a = 0; a < 3; ++a) { ctx->rf_offa[i][a] = off_a[3 * i + a]; ctx->rf_offb[i][a] = off_b[3 * i + a]; }
  }
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_relative_frame_upload(ddp_hip_ctx* ctx, const double* target, const double* quat, const double* weight, int64_t first,
                                             int64_t count) {
  const double* host[] = {target, quat, weight};
  const CostSideOk ok[] = {cost_finite_side, cost_quat_side, cost_weight_side};
  return cost_block_upload(ctx, COST_RELATIVE_FRAME, host, ok, first, count);
}
extern "C" int ddp_hip_relative_frame_download(ddp_hip_ctx* ctx, double* target, double* quat, double* weight, int64_t first, int64_t count) {
  double* host[] = {target, quat, weight};
  return cost_block_download(ctx, COST_RELATIVE_FRAME, host, first, count);
}

// an offset and a weight per (instance, t < T, control row): the record's rows are T (CostDesc::stage_only), the public shape
extern "C" int ddp_hip_control_grav_cost_upload(ddp_hip_ctx* ctx, const double* offset, const double* weight, int64_t first, int64_t count) {
  const double* host[] = {offset, weight};
  const CostSideOk ok[] = {cost_finite_side, cost_limit_weight_side};   // (a free-flyer root's six rows carry no term)
  return cost_block_upload(ctx, COST_CONTROL_GRAV, host, ok, first, count);
}
extern "C" int ddp_hip_control_grav_cost_download(ddp_hip_ctx* ctx, double* offset, double* weight, int64_t first, int64_t count) {
  double* host[] = {offset, weight};
  return cost_block_download(ctx, COST_CONTROL_GRAV, host, first, count);
}

// aim frames shared by the batch; a target with its stand-off and two weights per (instance, t, frame)
extern "C" int ddp_hip_frame_aim_set_frames(ddp_hip_ctx* ctx, int32_t n_frames, const int32_t* joint, const double* off, const double* axis) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_FRAME_AIM_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (n_frames < 0 || n_frames > DDP_HIP_MAX_AIM_FRAMES || (n_frames > 0 && (!joint || !off || !axis))) return DDP_HIP_E_ARG;
  if (!cost_aim_frames_ok(ctx->model_h.nj, n_frames, joint, off, axis)) return DDP_HIP_E_ARG;
  bool same = n_frames == ctx->fa_nf;
  for (int i = 0; same && i < n_frames; ++i) same = joint[i] == ctx->fa_joint[i];
  if (!same) {
    // other joints are another meaning of the per-frame data: targets, stand-offs and weights start again at 0
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc_ = cost_block_setup(ctx, COST_FRAME_AIM, n_frames);
    if (rc_ != DDP_HIP_OK) return rc_;
  }
  ctx->fa_nf = n_frames;
  for (int i = 0; i < n_frames; ++i) {
    ctx->fa_joint[i] = joint[i];
    for (int a = 0; a < 3; ++a) { ctx->fa_off[i][a] = off[3 * i + a]; ctx->fa_axis[i][a] = axis[3 * i + a]; }
  }
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_frame_aim_upload(ddp_hip_ctx* ctx, const double* target, const double* weight, int64_t first, int64_t count) {
  const double* host[] = {target, weight};
  const CostSideOk ok[] = {cost_aim_target_side, cost_weight_side};
  return cost_block_upload(ctx, COST_FRAME_AIM, host, ok, first, count);
}
extern "C" int ddp_hip_frame_aim_download(ddp_hip_ctx* ctx, double* target, double* weight, int64_t first, int64_t count) {
  double* host[] = {target, weight};
  return cost_block_download(ctx, COST_FRAME_AIM, host, first, count);
}

// a plane count shared by the batch; a plane (n, h, tau) and a weight per (instance, t, slot)
extern "C" int ddp_hip_balance_region_set_planes(ddp_hip_ctx* ctx, int32_t n_planes) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!(ctx->flags & DDP_HIP_FLAG_BALANCE_REGION_COST)) return DDP_HIP_E_UNSUPPORTED;
  if (n_planes < 0 || n_planes > DDP_HIP_MAX_REGION_PLANES) return DDP_HIP_E_ARG;
  if (n_planes != ctx->br_np) {
    // another count is another layout: geometry and weights start again at 0
    HIP_TRY(hipSetDevice(ctx->device));
    const int rc_ = cost_block_setup(ctx, COST_BALANCE_REGION, n_planes);
    if (rc_ != DDP_HIP_OK) return rc_;
  }
  ctx->br_np = n_planes;
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_balance_region_upload(ddp_hip_ctx* ctx, const double* geom, const double* weight, int64_t first, int64_t count) {
  const double* host[] = {geom, weight};
  const CostSideOk ok[] = {cost_region_geom_side, cost_weight_side};
  return cost_block_upload(ctx, COST_BALANCE_REGION, host, ok, first, count);
}
extern "C" int ddp_hip_balance_region_download(ddp_hip_ctx* ctx, double* geom, double* weight, int64_t first, int64_t count) {
  double* host[] = {geom, weight};
  return cost_block_download(ctx, COST_BALANCE_REGION, host, first, count);
}

// a target and a weight per (instance, t, tangent row of v): T+1 rows like the other records, row T without a term (a weight there: E_ARG)
extern "C" int ddp_hip_joint_accel_cost_upload(ddp_hip_ctx* ctx, const double* target, const double* weight, int64_t first, int64_t count) {
  const double* host[] = {target, weight};
  const CostSideOk ok[] = {cost_finite_side, cost_stage_weight_side};
  return cost_block_upload(ctx, COST_JOINT_ACCEL, host, ok, first, count);
}
extern "C" int ddp_hip_joint_accel_cost_download(ddp_hip_ctx* ctx, double* target, double* weight, int64_t first, int64_t count) {
  double* host[] = {target, weight};
  return cost_block_download(ctx, COST_JOINT_ACCEL, host, first, count);
}

extern "C" int ddp_hip_com_cost_upload(ddp_hip_ctx* ctx, const double* target, const double* weight, int64_t first, int64_t count) {
  const double* host[] = {target, weight};
  const CostSideOk ok[] = {cost_finite_side, cost_weight_side};
  return cost_block_upload(ctx, COST_COM, host, ok, first, count);
}
extern "C" int ddp_hip_com_cost_download(ddp_hip_ctx* ctx, double* target, double* weight, int64_t first, int64_t count) {
  double* host[] = {target, weight};
  return cost_block_download(ctx, COST_COM, host, first, count);
}

extern "C" int ddp_hip_momentum_cost_upload(ddp_hip_ctx* ctx, const double* target, const double* weight, int64_t first, int64_t count) {
  const double* host[] = {target, weight};
  const CostSideOk ok[] = {cost_finite_side, cost_weight_side};
  return cost_block_upload(ctx, COST_MOMENTUM, host, ok, first, count);
}
extern "C" int ddp_hip_momentum_cost_download(ddp_hip_ctx* ctx, double* target, double* weight, int64_t first, int64_t count) {
  double* host[] = {target, weight};
  return cost_block_download(ctx, COST_MOMENTUM, host, first, count);
}

// state limits: lo <= hi, before anything is written: a side that arrives alone is held against the resident other side (read
// back: uploads are not a hot path)
static int limits_lo_le_hi(ddp_hip_ctx* ctx, const double* const* host, int64_t first, int64_t count) {
  const double *l = host[0], *h = host[1];
  if (!l && !h) return DDP_HIP_OK;
  const CostBlock& k = ctx->cost[COST_LIMITS];
  const int64_t sz = cost_side_words(k, 0, ctx->d.T), words = sz * count;
  std::vector<double> other;
  if (!l || !h) {
    other.resize((size_t)words);
    HIP_TRY(hipMemcpyAsync(other.data(), k.side[l ? 1 : 0] + first * sz, sizeof(double) * (size_t)words, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    (l ? h : l) = other.data();
  }
  for (int64_t i = 0; i < words; ++i)
    if (l[i] > h[i]) return DDP_HIP_E_ARG;
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_state_limits_upload(ddp_hip_ctx* ctx, const double* lo, const double* hi, const double* weight, int64_t first,
                                           int64_t count) {
  const double* host[] = {lo, hi, weight};
  const CostSideOk ok[] = {cost_limit_lo_side, cost_limit_hi_side, cost_limit_weight_side};
  return cost_block_upload(ctx, COST_LIMITS, host, ok, first, count, limits_lo_le_hi);
}
extern "C" int ddp_hip_state_limits_download(ddp_hip_ctx* ctx, double* lo, double* hi, double* weight, int64_t first, int64_t count) {
  double* host[] = {lo, hi, weight};
  return cost_block_download(ctx, COST_LIMITS, host, first, count);
}

extern "C" int ddp_hip_set_async(ddp_hip_ctx* ctx, int on) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!on && ctx->async_mode) { HIP_TRY(hipSetDevice(ctx->device)); HIP_TRY(hipStreamSynchronize(ctx->stream)); }
  ctx->async_mode = on != 0;
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_set_active(ddp_hip_ctx* ctx, const int32_t* active) {
  if (!ctx) return DDP_HIP_E_ARG;
  ctx->all_active = true;
  for (int64_t b = 0; b < ctx->d.batch; ++b) {
    ctx->active_h[(size_t)b] = (!active || active[b]) ? 1 : 0;
    if (!ctx->active_h[(size_t)b]) ctx->all_active = false;
  }
  return DDP_HIP_OK;
}

// Joint armature [nv] into a resident model (shared with model_api.hip): checked as a whole first, so a refused call leaves the
// old values in force; then the stream is drained (kernels in flight read the old values to their end) and the array alone is
// written.  DevModel keeps it by joint, like axis: tangent row i of a fixed-base model is joint i, of a free-flyer model joint i - 5
int ddp_hip_apply_armature(DevModel& mh, DevModel* md, hipStream_t stream, const double* armature) {
  if (!armature) return DDP_HIP_E_ARG;
  if (mh.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_UNSUPPORTED;   // the pendulum's closed form is the reference's own
  const int vo = mh.ff ? 5 : 0;
  for (int i = 0; i < mh.nv; ++i) {
    if (!std::isfinite(armature[i]) || armature[i] < 0.0) return DDP_HIP_E_ARG;
    if (mh.ff && i < 6 && armature[i] != 0.0) return DDP_HIP_E_ARG;   // the six rows of the free-flyer root carry none
  }
  HIP_TRY(hipStreamSynchronize(stream));
  double a[DDP_MAXJ] = {};
  for (int j = mh.ff ? 1 : 0; j < mh.nj; ++j) a[j] = armature[j + vo];
  HIP_TRY(hipMemcpy(md->armature, a, sizeof(a), hipMemcpyHostToDevice));
  memcpy(mh.armature, a, sizeof(a));
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_set_armature(ddp_hip_ctx* ctx, const double* armature) {
  if (!ctx) return DDP_HIP_E_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  return ddp_hip_apply_armature(ctx->model_h, ctx->model_d, ctx->stream, armature);
}

extern "C" int ddp_hip_get_armature(ddp_hip_ctx* ctx, double* armature) {
  if (!ctx || !armature) return DDP_HIP_E_ARG;
  const DevModel& mh = ctx->model_h;
  if (mh.kind != DDP_HIP_MODEL_TREE) return DDP_HIP_E_UNSUPPORTED;
  for (int i = 0; i < mh.nv; ++i) armature[i] = (mh.ff && i < 6) ? 0.0 : mh.armature[mh.ff ? i - 5 : i];
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_ctx_info(const ddp_hip_ctx* ctx, ddp_hip_info* out) {
  if (!ctx || !out) return DDP_HIP_E_ARG;
  const Dims& d = ctx->d;
  out->device = ctx->device;
  out->lin_path = ctx->plan.lin_path;
  out->first_order = ctx->plan.first_order;
  out->bwd_path = sweep_plan(ctx).fast ? 1 : 0;
  out->fwd_path = fwd_lat_supported(ctx) ? 1 : 0;
  out->has_tensors = ctx->plan.has_tensors ? 1 : 0;
  int64_t bytes = 0;
  for (int s = 0; s < DDP_HIP_SEQ_COUNT; ++s)
    if (ctx->seq[s].ptr) bytes += 8 * ctx->seq[s].size * d.batch;
  out->hbm_bytes = bytes;
  return DDP_HIP_OK;
}

extern "C" int ddp_hip_swap_traj(ddp_hip_ctx* ctx) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (!ctx->all_active) {
    // a frozen instance keeps its trajectory: it is cloned into the buffers that become (X, U)
    HIP_TRY(hipSetDevice(ctx->device));
    const int64_t sx = ctx->seq[DDP_HIP_SEQ_X].size, su = ctx->seq[DDP_HIP_SEQ_U].size;
    for (int64_t b = 0; b < ctx->d.batch; ++b) {
      if (ctx->active_h[(size_t)b]) continue;
      HIP_TRY(hipMemcpyAsync(ctx->seq[DDP_HIP_SEQ_X_NEW].ptr + b * sx, ctx->seq[DDP_HIP_SEQ_X].ptr + b * sx, sizeof(double) * (size_t)sx, hipMemcpyDeviceToDevice, ctx->stream));
      HIP_TRY(hipMemcpyAsync(ctx->seq[DDP_HIP_SEQ_U_NEW].ptr + b * su, ctx->seq[DDP_HIP_SEQ_U].ptr + b * su, sizeof(double) * (size_t)su, hipMemcpyDeviceToDevice, ctx->stream));
    }
  }
  // swap(traj, new_traj), ddp.hpp:826: the resident buffers trade places, nothing moves in HBM
  std::swap(ctx->seq[DDP_HIP_SEQ_X].ptr, ctx->seq[DDP_HIP_SEQ_X_NEW].ptr);
  std::swap(ctx->seq[DDP_HIP_SEQ_U].ptr, ctx->seq[DDP_HIP_SEQ_U_NEW].ptr);
  return DDP_HIP_OK;
}

// ---- profiling: HIP events on the context's own stream around every launch of a kernel class --
void prof_begin(ddp_hip_ctx* ctx, int kid, hipStream_t stream) {
  if (!(ctx->profile_mask & (2u << kid))) return;
  if (!stream) stream = ctx->stream;
  ProfSlot& p = ctx->prof[kid];
  if (p.used == p.starts.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { (void)hipGetLastError(); return; }
    p.starts.push_back(a);
    p.stops.push_back(b);
  }
  (void)hipEventRecord(p.starts[p.used], stream);
}
void prof_end(ddp_hip_ctx* ctx, int kid, hipStream_t stream) {
  if (!(ctx->profile_mask & (2u << kid))) return;
  if (!stream) stream = ctx->stream;
  ProfSlot& p = ctx->prof[kid];
  if (p.used >= p.stops.size()) return;
  (void)hipEventRecord(p.stops[p.used], stream);
  ++p.used;
}
static void prof_collect(ddp_hip_ctx* ctx) {
  (void)hipStreamSynchronize(ctx->stream);
  for (int k = 0; k < DDP_HIP_K_COUNT; ++k) {
    ProfSlot& p = ctx->prof[k];
    for (size_t i = 0; i < p.used; ++i) {
      float ms = 0;
      if (hipEventElapsedTime(&ms, p.starts[i], p.stops[i]) == hipSuccess) { p.total_ms += ms; ++p.launches; }
      else (void)hipGetLastError();
    }
    p.used = 0;
  }
}

extern "C" int ddp_hip_profile_enable(ddp_hip_ctx* ctx, int on) {
  if (!ctx) return DDP_HIP_E_ARG;
  if (ctx->profile_mask && !on) prof_collect(ctx);
  ctx->profile_mask = on == 1 ? ~0u : (uint32_t)on;      // 1: every class; else bit (1 + kernel_id) selects a class
  return DDP_HIP_OK;
}
extern "C" int ddp_hip_profile_reset(ddp_hip_ctx* ctx) {
  if (!ctx) return DDP_HIP_E_ARG;
  prof_collect(ctx);
  for (int k = 0; k < DDP_HIP_K_COUNT; ++k) { ctx->prof[k].total_ms = 0; ctx->prof[k].launches = 0; }
  return DDP_HIP_OK;
}
extern "C" int ddp_hip_profile_get(ddp_hip_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches) {
  if (!ctx || kernel_id < 0 || kernel_id >= DDP_HIP_K_COUNT) return DDP_HIP_E_ARG;
  prof_collect(ctx);
  if (total_ms) *total_ms = ctx->prof[kernel_id].total_ms;
  if (launches) *launches = ctx->prof[kernel_id].launches;
  return DDP_HIP_OK;
}

// Bytes of f_xx / f_ux / f_uu the contraction kernel (K3) reads per (instance, step) with the tensors in their current state:
// everything (tensors from outside), the columns j >= c of slab c (symmetric: this context's own mode-2 / zero tensors), or the
// lower halves of those columns plus the (at most) two non-zero entries of each upper half (the static stencil's own tensors).
// (From packed records K3h takes the two upper-half entries of a column as one 16-byte word whether or not the second is used:
// about 1 % more than the closed form below, which counts what the contraction needs.)
extern "C" int64_t ddp_hip_bwd_stream_bytes(const ddp_hip_ctx* ctx) {
  if (!ctx) return -1;
  if (ctx->flags & DDP_HIP_FLAG_NO_TENSORS) return 0;
  const int64_t n = ctx->d.n, m = ctx->d.m;
  const SweepPlan s = sweep_plan(ctx);
  if (s.half_mode == 1) {
    const int64_t cxx = n * (n + 1) / 2, cux = n * m, cuu = m * (m + 1) / 2;
    return 8 * ((cxx + cux + cuu) * (n - m) + 2 * cxx - n + cux);       // lower halves + two entries per f_xx column (one on its diagonal), one per f_ux column
  }
  if (s.half_mode == 2)
    return 8 * (n * n + n * m) * (n - m);                                // analytic mode 1: the lower halves of f_xx and f_ux, nothing of f_uu
  if (s.sym) return 8 * (n * (n * (n + 1) / 2) + n * n * m + n * (m * (m + 1) / 2));
  return 8 * (n * n * n + n * n * m + n * m * m);
}

extern "C" int64_t ddp_hip_bwd_algorithmic_bytes(const ddp_hip_ctx* ctx) {
  if (!ctx) return -1;
  const Dims& d = ctx->d;
  const int64_t n = d.n, m = d.m, nx = d.nx, T = d.T;
  // B_bwd = 8 T [(n+m+n^2+mn+m^2) + (n^2+nm) + (n^3+n^2 m+n m^2) + (m+mn+nx)] + eq terms
  int64_t per_step = (n + m + n * n + m * n + m * m) + (n * n + n * m) + (m + m * n + nx);
  if (!(ctx->flags & DDP_HIP_FLAG_NO_TENSORS)) per_step += n * n * n + n * n * m + n * m * m;
  int64_t words = T * per_step;
  for (int64_t t = 0; t < T; ++t) {
    int64_t e = ctx->ne_h[(size_t)t];
    words += (e + e * n + e * m) + (e + e * n);
    if (!(ctx->flags & DDP_HIP_FLAG_NO_TENSORS)) words += e * n * n + e * m * n + e * m * m;
  }
  return 8 * words;
}
