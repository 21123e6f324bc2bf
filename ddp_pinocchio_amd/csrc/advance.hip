// advance.hip -- ddp_hip_advance: the receding-horizon shift of everything a context holds per time step, in place on the resident
// data, and the re-roll from the measured state through the launch paths of fwd.hip.  The pure part -- which
// arrays, what a row becomes, the per-word walk, the argument checks -- is advance_plan.h.
#include "advance_plan.h"
#include "internal.h"

namespace {

// One array of the shift as the kernel sees it.  X and U trade places with X_NEW and U_NEW at every swap_traj, so the table, which
// is built once per layout, names them by slot and the launch hands their addresses over
enum AdvSlot : int32_t { ADV_SLOT_BASE, ADV_SLOT_X, ADV_SLOT_U };
struct AdvDev {
  double* base;          // [batch][inst_words] (ADV_SLOT_BASE)
  int64_t inst_words;    // words per instance, a terminal row included
  int64_t rows, width;   // AdvArray's
  int64_t block_begin;   // the array's first workgroup of the launch
  int32_t rule, slot;
};

constexpr int ADV_BLOCK = 256;

// One lane owns one word of a row of one (array, instance) pair and walks it through t (adv_walk_column: the hazard argument is
// there).  Lanes are flattened over instance x words of a row, so a row of three words still fills its waves, and neighbouring
// lanes hold neighbouring words: every load and store of a wave is one contiguous run but at an instance's edge.  A workgroup
// belongs to one array (the table is scanned with uniform, scalar reads)
__global__ __launch_bounds__(ADV_BLOCK) void advance_shift_kernel(const AdvDev* tab, int32_t narr, double* X, double* U, const double* x0,
                                                                  int64_t batch, int64_t s) {
  int a = 0;
  while (a + 1 < narr && tab[a + 1].block_begin <= (int64_t)blockIdx.x) ++a;
  const AdvDev d = tab[a];
  const int64_t lane = ((int64_t)blockIdx.x - d.block_begin) * ADV_BLOCK + threadIdx.x;
  if (lane >= batch * d.width) return;
  const int64_t b = lane / d.width, w = lane - b * d.width;
  double* base = d.slot == ADV_SLOT_X ? X : d.slot == ADV_SLOT_U ? U : d.base;
  const double* first = d.rule == ADV_TRAJ && x0 ? x0 + b * d.width + w : nullptr;
  adv_walk_column(base + b * d.inst_words + w, d.width, d.rows, d.rule, s, first);
}

// The state ddp_hip_solve documents as its input: X_NEW / U_NEW clones of X / U, FB_ORIGIN[t] = MULT_ORIGIN[t] = X[t], t < T
__global__ void advance_finish_kernel(const double* X, const double* U, double* Xn, double* Un, double* fb_origin, double* mult_origin,
                                      int64_t batch, int64_t T, int64_t nx, int64_t m) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t sx = (T + 1) * nx, so = T * nx;
  for (int64_t i = i0; i < batch * sx; i += stride) {
    const int64_t b = i / sx, r = i - b * sx;
    const double v = X[i];
    Xn[i] = v;
    if (r < so) { fb_origin[b * so + r] = v; mult_origin[b * so + r] = v; }
  }
  for (int64_t i = i0; i < batch * T * m; i += stride) Un[i] = U[i];
}

// the table of the context's flags and layouts as they are now; device memory on the first call only
int adv_setup(ddp_hip_ctx* ctx) {
  const Dims& d = ctx->d;
  if (!ctx->adv_tab_d) HIP_TRY(hipMalloc(&ctx->adv_tab_d, sizeof(AdvDev) * ADV_MAX_ARRAYS));
  if (!ctx->adv_x0_d) HIP_TRY(hipMalloc(&ctx->adv_x0_d, sizeof(double) * (size_t)(d.batch * d.nx)));
  if (ctx->adv_mu_h.empty()) { ctx->adv_mu_h.assign((size_t)d.batch, 1.0); ctx->adv_step_h.assign((size_t)d.batch, 0.0); }
  if (!ctx->adv_dirty) return DDP_HIP_OK;
  AdvArray plan[ADV_MAX_ARRAYS];
  AdvDev tab[ADV_MAX_ARRAYS];
  const int narr = adv_plan_build(ctx->flags, d.T, d.n, d.m, d.nx, ctx->cost, plan);
  int64_t blocks = 0;
  for (int k = 0; k < narr; ++k) {
    const AdvArray& a = plan[k];
    AdvDev& t = tab[k];
    t.slot = a.kind == ADV_SEQ && a.id == DDP_HIP_SEQ_X ? ADV_SLOT_X : a.kind == ADV_SEQ && a.id == DDP_HIP_SEQ_U ? ADV_SLOT_U : ADV_SLOT_BASE;
    t.base = t.slot != ADV_SLOT_BASE ? nullptr : a.kind == ADV_SEQ ? ctx->seq[a.id].ptr : ctx->cost[a.id].side[a.side];
    t.inst_words = adv_inst_words(a);
    t.rows = a.rows; t.width = a.width; t.rule = a.rule;
    t.block_begin = blocks;
    // the plan and the context agree on every array's size, or nothing is launched
    if (a.kind == ADV_SEQ ? t.inst_words != ctx->seq[a.id].size || !ctx->seq[a.id].ptr
                          : t.inst_words != cost_side_words(ctx->cost[a.id], a.side, d.T) || !ctx->cost[a.id].side[a.side])
      return DDP_HIP_E_UNSUPPORTED;
    blocks += (d.batch * a.width + ADV_BLOCK - 1) / ADV_BLOCK;
  }
  if (blocks > 0x7fffffff) return DDP_HIP_E_UNSUPPORTED;
  HIP_TRY(hipMemcpyAsync(ctx->adv_tab_d, tab, sizeof(AdvDev) * (size_t)narr, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));   // (tab lives on this frame)
  ctx->adv_narr = narr;
  ctx->adv_blocks = blocks;
  ctx->adv_dirty = false;
  return DDP_HIP_OK;
}

int adv_finish(ddp_hip_ctx* ctx) {
  const Dims& d = ctx->d;
  auto S = [&](int s) { return ctx->seq[s].ptr; };
  int64_t blocks = (d.batch * (d.T + 1) * d.nx + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(advance_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, S(DDP_HIP_SEQ_X), S(DDP_HIP_SEQ_U),
                     S(DDP_HIP_SEQ_X_NEW), S(DDP_HIP_SEQ_U_NEW), S(DDP_HIP_SEQ_FB_ORIGIN), S(DDP_HIP_SEQ_MULT_ORIGIN), d.batch, d.T, d.nx, d.m);
  HIP_TRY(hipGetLastError());
  return DDP_HIP_OK;
}

}  // namespace

void adv_teardown(ddp_hip_ctx* ctx) {
  if (ctx->adv_tab_d) (void)hipFree(ctx->adv_tab_d);
  if (ctx->adv_x0_d) (void)hipFree(ctx->adv_x0_d);
  ctx->adv_tab_d = nullptr;
  ctx->adv_x0_d = nullptr;
}

extern "C" int ddp_hip_advance(ddp_hip_ctx* ctx, int64_t shift, const double* x0, int32_t mode) {
  if (!ctx) return DDP_HIP_E_ARG;
  const Dims& d = ctx->d;
  int rc = adv_args_check(d.T, d.Etot, d.batch, d.nx, ctx->model_h.ff != 0, shift, x0, mode);
  if (rc != DDP_HIP_OK) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  // (the closed-loop roll would refuse some lo > hi after the shift had been written)
  if (mode == DDP_HIP_ADVANCE_CLOSED_LOOP && (ctx->flags & DDP_HIP_FLAG_CONTROL_BOUNDS)) { rc = box_check(ctx); if (rc != DDP_HIP_OK) return rc; }
  rc = adv_setup(ctx);
  if (rc != DDP_HIP_OK) return rc;
  if (x0) HIP_TRY(hipMemcpyAsync(ctx->adv_x0_d, x0, sizeof(double) * (size_t)(d.batch * d.nx), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(advance_shift_kernel, dim3((unsigned)ctx->adv_blocks), dim3(ADV_BLOCK), 0, ctx->stream, (const AdvDev*)ctx->adv_tab_d,
                     ctx->adv_narr, ctx->seq[DDP_HIP_SEQ_X].ptr, ctx->seq[DDP_HIP_SEQ_U].ptr, x0 ? ctx->adv_x0_d : (const double*)nullptr,
                     d.batch, shift);
  HIP_TRY(hipGetLastError());
  if (mode == DDP_HIP_ADVANCE_OPEN_LOOP) {
    rc = ddp_hip_rollout(ctx);
    if (rc != DDP_HIP_OK) return rc;
  } else if (mode == DDP_HIP_ADVANCE_CLOSED_LOOP) {
    // ddp_hip_forward(n_alpha = 0) and the buffer swap of ddp_hip_swap_traj, with every instance active for their duration: the
    // backward graph's keys see the swap they always see.  X_NEW[0] = X[0] comes with the clone
    rc = adv_finish(ctx);
    if (rc != DDP_HIP_OK) return rc;
    const std::vector<int32_t> active = ctx->active_h;
    const bool all_active = ctx->all_active;
    ctx->active_h.assign((size_t)d.batch, 1);
    ctx->all_active = true;
    rc = ddp_hip_forward(ctx, ctx->adv_mu_h.data(), 0, ctx->adv_step_h.data(), nullptr);
    if (rc >= 0) rc = ddp_hip_swap_traj(ctx);
    ctx->active_h = active;
    ctx->all_active = all_active;
    if (rc < 0) return rc;
  }
  rc = adv_finish(ctx);
  if (rc != DDP_HIP_OK) return rc;
  END_SYNC(ctx);
  return DDP_HIP_OK;
}
