// internal.h -- context layout shared by the translation units of libddp_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "bwd_jobs.h"
#include "cost_block.h"
#include "ddp_hip/ddp_hip.h"

#define DDP_MAXJ DDP_HIP_MAX_JOINTS

// Device-side model table (tree of 1-DoF joints or the closed-form pendulum); lives in HBM, read
// through the scalar / L2 path by every dynamics kernel.
struct DevModel {
  int32_t kind, nv;              // nv: velocity (tangent) dimension
  int32_t ff, nj, nq, pad0_;     // free-flyer root (SE(3), lie.h); number of joints (nv - 5 with a free flyer, else nv); configuration dimension
  double mass, length;
  double gravity[3];
  double dt, c;
  int32_t parent[DDP_MAXJ];
  int32_t jtype[DDP_MAXJ];
  double axis[DDP_MAXJ][3];
  double Rp[DDP_MAXJ][9];
  double pp[DDP_MAXJ][3];
  double I6[DDP_MAXJ][21];  // body spatial inertia, packed lower triangle (row-major: (r,c), c<=r at r(r+1)/2+c)
  // small-state traversal tables (ctx.hip:build_slot_tables): a joint's running sum lives in one of a few slots
  int32_t has_child[DDP_MAXJ];      // joint has at least one child
  int32_t first_contrib[DDP_MAXJ];  // joint is the largest-index child of its parent (contributes first, leaf->root)
  int32_t last_child[DDP_MAXJ];     // joint is the largest-index child of its parent (read last, root->leaf)
  int32_t slot_up[DDP_MAXJ];        // slot of the joint's accumulator in the leaf->root pass (-1: leaf)
  int32_t slot_down[DDP_MAXJ];      // slot of the joint's value in the root->leaf pass (-1: leaf)
  int32_t n_slots;
  // level schedule for the wave-cooperative traversals: joints sorted by tree depth (rbd.h: aba_tree_coop walks these tables; the
  // forward kernel's traversals read them packed into one role word per lane and level, CoopModel::role)
  int32_t n_levels, max_level_width;
  int32_t lvl_start[DDP_MAXJ + 1];  // joints of level L are lvl_joint[lvl_start[L] .. lvl_start[L+1])
  int32_t lvl_joint[DDP_MAXJ];
  int32_t child_start[DDP_MAXJ + 1]; // children of joint i (descending index) are child_list[child_start[i] .. child_start[i+1])
  int32_t child_list[DDP_MAXJ];
  // constraint chain
  int32_t eq_kind, eq_advance, frame_joint, first_order_fd, fd_mode, pad_;
  double frame_off[3];
  // joint armature (reflected rotor inertia), by joint like axis: D = S^T IA S + armature, M_ii += armature.  Zero at create,
  // written by ddp_hip_set_armature / ddp_hip_model_set_armature; the free-flyer root (joint 0 of an ff model) carries none
  double armature[DDP_MAXJ];
};

// Everything a kernel needs to find a block of a flat sequence.
struct Dims {
  int64_t T, n, m, nx, nv, batch;
  int64_t Etot;   // sum_t ne[t]
  int64_t emax;
};

struct SeqBuf {
  double* ptr = nullptr;   // [batch][size]
  int64_t size = 0;        // per-instance element count
};

// Development switches (DDP_HIP_*), read once by ddp_hip_create (lin_plan.cpp: read_switches): a context
// keeps the paths it was created with.  A tuning knob of 0 is unset (or out of its range): the context's own choice holds.
struct DevSwitches {
  bool generic_bwd = false;    // GENERIC_BWD: the run-time-shaped sweep at the Talos shape as well
  bool k3_no_sym = false;      // K3_NO_SYM: K3 reads every half-slab (and the static stencil writes the mirror images)
  bool k3_no_half = false;     // K3_NO_HALF: no K3h
  bool k3_no_pack = false;     // K3_NO_PACK: the static stencil writes the contract layout, K3h reads it strided (no packed records)
  bool k3h_column_jobs = false;   // K3H_COLUMN_JOBS: the packed K3h on the column jobs of the strided one (133 units per instance), not on full units
  bool fxx_full = false;       // FXX_FULL: the static stencil writes the configuration rows and the mirror images
  bool no_static = false;      // NO_STATIC: the generic level kernels instead of the static-topology ones
  bool no_qcache = false;      // NO_QCACHE: no configuration caches
  bool qcache_dense = false;   // QCACHE_DENSE: the static stencil's q-cache keeps a whole block per stepped configuration (no base + deltas layout)
  bool vcache_dense = false;   // VCACHE_DENSE: the static stencil's v-cache keeps its 2 nv + 1 whole entries (no base + deltas layout)
  bool first_scalar = false;   // FIRST_SCALAR: the static first order's u waves and the u diagonal as two kernels on the scalar path (no LDS staging, no fused launch)
  bool cfg_full_aba = false;   // CFG_FULL_ABA: the (q_i, q_j) points of the static stencil run the whole ABA (two kernels, two streams)
  bool ana_own_aba = false;    // ANA_OWN_ABA: the analytic pass forms its own accelerations
  bool ana_split = false;      // ANA_SPLIT: the three-kernel analytic path with its HBM workspaces
  bool ana_eq_kernel = false;  // ANA_EQ_KERNEL: the constraint tensors in a kernel of their own
  bool bwd_no_graph = false;   // BWD_NO_GRAPH: the sweep is enqueued launch by launch, not replayed as a hipGraph
  bool solve_sync = false;     // SOLVE_SYNC: ddp_hip_solve waits for the stream at every call
  bool fwd_no_pipe = false;    // FWD_NO_PIPE: the forward latency kernel in its four-candidate form, never the pipelined one
  bool lin_serial = false;     // LIN_SERIAL: every kernel of a linearisation on the context's stream, in the single-stream order (no side streams)
  int32_t lin_forks = 0;       // LIN_FORKS (1..3): the LinFork bits a concurrent linearisation keeps (A/B of one fork at a time)
  int32_t bwd_cbx = 0, bwd_cbu = 0;   // BWD_CBX (1..8), BWD_CBU (1..16): columns per job of K3 / bwd_assemble
  int64_t qws_bt = 0;          // QWS_BT (16..65536): (instance, t) pairs per configuration-level workspace slice
  int64_t ana_bt = 0;          // ANA_BT (1..65536): (instance, t) pairs per analytic workspace slice
};

// The backward sweep a context runs on its tensors as they are (bwd.hip: sweep_plan)
struct SweepPlan {
  bool fast;       // the Talos-shape kernels K5 / K3 / K4' (bwd_v2.h); else the run-time-shaped pair
  bool sym_ok;     // ... which would read symmetric tensors by halves: the static stencil may leave the mirror images out
  bool sym;        // ... and they are symmetric now (TensorState): K3 reads one of each pair of mirrored half-slabs
  int32_t half_mode;   // K3h (bwd_split.h: bwd_contract_half): 0 off, 1 the static stencil's tensors, 2 analytic mode 1
  bool packed;         // half_mode 1 on the stencil's packed records (TensorState::packed)
};

// Which kernels a context's linearisation runs and which workspaces they need: decided once, by lin_plan_decide (lin_plan.cpp, a
// pure function of what ddp_hip_create was given), stored by lin_setup and read by everything else.
enum class LinFirst : int32_t {
  Base,            // f alone (lin_base_kernel): the pendulum's closed-form jacobians come with it
  AnalyticSmall,   // one lane per (instance, t) (lin_first_analytic_small_kernel)
  AnalyticWave,    // one wave per evaluation (lin_analytic.hip: stage 0)
  AnalyticFF,      // free-flyer root (lin_analytic.hip: ana_ff_first_kernel)
  FdStatic,        // forward differences on the static-topology kernels, from the base point's caches
  FdGeneric,       // forward differences on the run-time tree (lin_first_kernel)
};
enum class LinSecond : int32_t {
  None,            // tensor-free context
  Zeros,           // mode 0
  Mode2Static,     // the stencil on the static-topology kernels
  Mode2Caches,     // the stencil on the run-time tree, from the q- / v-caches
  Mode2Plain,      // the stencil on the run-time tree, every point a full evaluation
  Mode1Small,      // forward differences of the analytic jacobians, one lane per direction (second_m1_kernel)
  Mode1Wave,       // ... one wave per evaluation (lin_analytic.hip: stage 1)
};
enum class LinEq : int32_t {
  None,            // no constraint rows
  PerLane,         // small vector-space models with analytic jacobians: the whole chain in one lane (eq_first_kernel)
  Analytic,        // large trees with analytic jacobians (lin_analytic.hip: ana_eq_kernel)
  Chain,           // forward-differenced jacobians, and free-flyer models: eq_chain / look-ahead jacobians / eq_combine
};
// The forks of a static-topology linearisation's schedule (LinPlan::forks): each moves kernels that depend
// on nothing the context's stream is running onto the side stream, and is joined back before the profiling bracket it was forked in ends
enum LinFork : uint32_t {
  LIN_FORK_CFG = 1,        // the configuration level (spine + pairs, slice by slice) beside the velocity level
  LIN_FORK_SPINE = 2,      // ... its first spine pre-pass already beside the u diagonal and the torque rows (with LIN_FORK_CFG)
  LIN_FORK_DEFAULT = LIN_FORK_CFG | LIN_FORK_SPINE,
};
enum class LinEqJac : int32_t { None, Fd, FfLookahead };   // Chain with K > 1: where f_x at the look-ahead states comes from
enum class LinEqSecond : int32_t { None, Zeros, Mode2, Mode1Small, Mode1Wave };   // the constraint tensors: as LinSecond
struct LinPlan {
  int32_t refuse = 0;          // DDP_HIP_E_UNSUPPORTED: ddp_hip_create refuses the context (lin_setup returns it)
  int32_t nj = 0;              // the NJ instantiation of lin.hip's kernels: 1 / 6 / 38 / 64
  int32_t topo = 0;            // id of the compiled-in topology whose kernels run (lin_static.hip), 0: none
  LinFirst first = LinFirst::Base;
  LinSecond second = LinSecond::None;
  LinEq eq = LinEq::None;
  LinEqJac eq_jac = LinEqJac::None;
  LinEqSecond eq_second = LinEqSecond::None;
  bool eq_inline = false;      // Mode1Wave, config constraint: its tensors come out of the evaluation waves (no ana_eq_kernel, no slices)
  bool accel_static = false;   // Mode1Wave: the perturbed points' accelerations come from the static first-order kernels (ana_A)
  bool accel_with_u = false;   // ... along the u directions as well (the constraint chain differences along them)
  bool m1_fused = false;       // Mode1Wave: the pass is issued by the LIN_EQ stage, together with the constraint tensors
  int32_t ncfg = 0, nvcfg = 0; // q- / v-cache entries per (instance, t)
  bool qc_sparse = false;      // the static stencil's q-cache is the base block and, per stepped joint, the records its step changes
                               // (caches); false: ncfg whole blocks
  bool vc_sparse = false;      // with qc_sparse: the v-cache is entry 0, a v-step base block and the records a q or v step changes; false:
                               // nvcfg whole entries
  bool has_tensors = false;    // FXX / FUX / FUU are resident
  bool skip_top = false;       // LinParams::skip_top
  bool skip_qv_mirror = false; // LinParams::skip_qv_mirror
  bool pack = false;           // LinParams::pack: the static stencil leaves packed records, which K3h streams
  // the workspaces that exist (lin_setup, lin_analytic_setup allocate exactly these)
  bool ws_lin = false, ws_qws = false, ws_qws2 = false;   // the caches; the static path's configuration-level workspace; its twin + stream
  bool ws_ana_T = false, ws_ana_M = false, ws_ana_M0 = false, ws_ana_A = false, ws_ana_F = false;
  bool ws_eq = false;
  bool ana_sliced = false;     // lin_analytic.hip takes the model: ctx->ana_nbt is set
  int64_t eq_fxk_off = 0, eq_c_off = 0, eq_words = 0;   // eq_ws: x_1..x_K | f_x(x_1..x_{K-1}) at eq_fxk_off | base jacobian at eq_c_off
  uint32_t forks = 0;          // LinFork bits: the schedule's forks onto the side streams (0: the single-stream order)
  int32_t lin_path = 0, first_order = 0;   // what ddp_hip_ctx_info reports
};
DevSwitches read_switches();   // lin_plan.cpp: the one place in the library that reads the environment
LinPlan lin_plan_decide(const DevModel& m, const Dims& d, uint32_t flags, const DevSwitches& sw, int topo_id, bool sweep_sym_ok);

// What FXX / FUX / FUU hold, as far as a reader inside the library may rely on it.  The record changes
// only through the four transitions declared below (lin.hip); sweep_plan reads it and nothing else about the tensors.
enum class TensorOrigin : int32_t {
  Unknown,     // never written, written from outside (upload / fill / device_ptr), or left by a linearisation that failed: no structure
  Symmetric,   // this context's mode 2 on the run-time-tree kernels, or mode 0: f_xx and f_uu symmetric bit for bit
  Stencil,     // the static mode-2 stencil's own: symmetric, and the configuration rows k < nv zeros but two entries per column
  Analytic1,   // analytic mode 1's own (lin_analytic.hip): zero configuration rows, zero f_uu, not symmetric
};
struct TensorState {
  TensorOrigin origin = TensorOrigin::Unknown;
  // the static stencil left the mirror images f_xx(:, i, j), f_uu(:, i, j), i < j, out (LinParams::skip_qv_mirror).  Its own bit
  // because it outlives the origin: an upload of FUX alone takes Stencil to Symmetric and leaves the images unwritten
  bool mirror_pending = false;
  // the three tensors hold the static stencil's packed records (LinParams::pack), not the contract layout: only the packed K3h
  // reads them as they are, every other reader goes through lin_materialize_fxx first.  Implies origin == Stencil
  bool packed = false;
};

// State of one linearisation call (lin.hip: ddp_hip_linearize_stages creates it, lin_analytic.hip reads and marks it)
struct LinCall {
  bool ana_A_fresh = false;    // ana_A was formed by stage 0 of this call
  bool ana_M0_fresh = false;   // ana_M0 was written by stage 0 of this call
  bool fuu_zero = false;       // F_UU holds exact zeros: analytic mode 1 left them (TensorOrigin::Analytic1 at entry) or has just written them
};

struct ProfSlot {
  std::vector<hipEvent_t> starts, stops;
  size_t used = 0;
  double total_ms = 0;
  int64_t launches = 0;
};

struct ddp_hip_ctx {
  int device = 0;
  int cu_count = 0;                    // the device's compute units, read once at create (fwd.hip: which form a forward launch takes)
  uint32_t flags = 0;
  hipStream_t stream = nullptr;
  Dims d{};
  std::vector<int64_t> ne_h, Epre_h;   // [T], [T+1]
  int64_t* ne_d = nullptr;             // [T]
  int64_t* Epre_d = nullptr;           // [T+1] prefix sums of ne
  double* target_d = nullptr;          // [Etot]
  DevModel model_h{};
  DevModel* model_d = nullptr;
  SeqBuf seq[DDP_HIP_SEQ_COUNT];
  DevSwitches sw;

  // backward workspace, per instance
  double* ws_V = nullptr;      // [batch][n + n*n]          V_x | V_xx
  double* ws_Q = nullptr;      // [batch][n + m + n*n + m*n + m*m]   Q_x | Q_u | Q_xx | Q_ux | Q_uu
  double* reg_d = nullptr;     // [batch]
  double* mu_d = nullptr;      // [batch]
  int32_t* status_d = nullptr; // [batch] 0 active, 1 failed this attempt, 2 done
  int64_t* restarts_d = nullptr;
  BwdJob* jobs_d = nullptr;
  BwdJob* jobs_half_d = nullptr;  // K3h's job list (bwd_split.h: bwd_contract_half)
  int32_t njobs_half = 0;
  K3hUnit* units_half_d = nullptr;   // the packed K3h's full units (bwd_jobs.h), K3H_UNITS_PER_JOB per job
  int32_t njobs_units = 0;
  TensorState tensors;            // what FXX / FUX / FUU hold
  BwdJob* jobs_sym_d = nullptr;   // K3's job list for symmetric tensors (bwd_split.h, job kind 2)
  int32_t njobs = 0;
  int32_t cbx = 0, cbu = 0;
  // the sweep as an instantiated hipGraph (600 launches per sweep otherwise pay the enqueue cost every time);
  // one per state of the kernel arguments (the X buffers trade places at every swap_traj)
  struct BwdGraph { const void* key_x = nullptr; uint64_t key_misc = 0; hipGraphExec_t exec = nullptr; hipGraph_t graph = nullptr; };
  BwdGraph bwd_graph[4];
  int bwd_graph_next = 0;

  // forward workspace
  double* fw_x = nullptr;      // [batch][n_alpha_max][(T+1)*nx]
  double* fw_u = nullptr;      // [batch][n_alpha_max][T*m]
  double* fw_dcost = nullptr;  // [batch][n_alpha_max]
  double* fw_cost = nullptr;   // [batch][n_alpha_max][T+1] candidates' cost terms (constrained problems on the latency path)
  double* fw_cost_old = nullptr; // [batch]
  double* step_d = nullptr;    // [batch]
  int32_t* fw_state_d = nullptr; // [batch] 0 searching, 1 accepted, 2 floor hit
  double* fw_dcost_acc_d = nullptr; // [batch]
  int32_t n_alpha_max = 8;
  double* pick_pair_d = nullptr;  // best-cost pick of a single-rank run (comm.cpp: ddp_hip_shard_pick)

  // linearize workspace
  double* eq_ws = nullptr;     // constraint-chain workspace (large models)
  double* lin_ws = nullptr;
  LinPlan plan;                // what the linearisation runs (set by lin_setup)
  double* lin_qws = nullptr;   // configuration-level workspace of the static path, lin_qws_bt (instance, t) pairs at a time
  int64_t lin_qws_bt = 0;
  double* lin_qws2 = nullptr;  // second workspace + stream + events (DDP_HIP_CFG_FULL_ABA only): the two full-ABA kernels of consecutive slices overlap
  hipStream_t lin_stream2 = nullptr;
  hipEvent_t lin_ev_up[2] = {nullptr, nullptr}, lin_ev_dn[2] = {nullptr, nullptr};
  // the concurrent schedule (LinPlan::forks) runs its side branch on lin_stream2: fork / done events, and the torque rows'
  // completion.  lin_side_busy: work has been forked onto the side stream and not joined back yet (LinJoin)
  hipEvent_t lin_ev_fork = nullptr, lin_ev_done = nullptr, lin_ev_rows = nullptr;
  bool lin_side_busy = false;
  double* ana_T = nullptr;     // analytic-derivative workspace (lin_analytic.hip): T = [dtau/dq | dtau/dv] per evaluation of a slice
  double* ana_M = nullptr;     // ... and M / M^-1 per configuration of a slice
  double* ana_F = nullptr;     // ... and the v rows of f_x at the perturbed points (mode-1 constraint tensors)
  double* ana_M0 = nullptr;    // [B T][nv][nv] M^-1 at the trajectory points (fused analytic path, mode 1)
  double* ana_A = nullptr;     // [B T][2nv][nv] accelerations of the mode-1 perturbed points (static first-order kernels, StaticLevel::AccelX)
  int64_t ana_nbt = 0;         // (instance, t) pairs per slice

  // per-instance activity (ddp_hip_set_active): an inactive instance is frozen -- the sweeps skip it and swap_traj
  // keeps its trajectory (solve<M> returns an instance at its first optimum, ddp.hpp:799-800)
  std::vector<int32_t> active_h;   // [batch], 1 = active
  bool all_active = true;

  // the per-instance add-on cost terms (cost_block.h; ctx.hip: ddp_hip_*_upload / _download): one record
  // each.  What the batch shares -- the geometry -- stays beside them
  CostBlock cost[COST_COUNT];
  // the cost frames (ddp_hip_frame_cost_set_frames): of the position, orientation and velocity terms alike
  int32_t fc_nf = 0;                          // cost frames set (0: none yet)
  int32_t fc_joint[DDP_HIP_MAX_COST_FRAMES] = {};
  double fc_off[DDP_HIP_MAX_COST_FRAMES][3] = {};
  // the collision points and the obstacle slots' kinds (ddp_hip_obstacle_set_points)
  int32_t ob_np = 0, ob_no = 0;               // collision points and obstacle slots set (0: none yet)
  int32_t ob_joint[DDP_HIP_MAX_COLLISION_POINTS] = {};
  double ob_off[DDP_HIP_MAX_COLLISION_POINTS][3] = {};
  double ob_radius[DDP_HIP_MAX_COLLISION_POINTS] = {};
  int32_t ob_kind[DDP_HIP_MAX_OBSTACLES] = {};
  double* ob_clear_d = nullptr;               // [batch][T+1] what ddp_hip_obstacle_clearance hands back
  // the voxel grid the slots of kind DDP_HIP_OBSTACLE_GRID read (ddp_hip_obstacle_set_grid / _set_occupancy, obstacle_grid.hip):
  // two fields, the one in force (og_cur) and the one the next set call writes, so that a failed call leaves the old grid in force
  // and a scene refreshed at the same shape allocates nothing
  double* og_phi[2] = {nullptr, nullptr};     // [nx][ny][nz] each
  int64_t og_cap[2] = {0, 0};                 // their sizes in doubles
  int32_t og_cur = -1;                        // -1: no grid yet
  int32_t og_n[3] = {};
  double og_origin[3] = {}, og_cell = 0.0;
  int32_t* og_d2 = nullptr;                   // [2][voxels] the transform's squared distances (D_occ, D_free), kept between calls
  uint8_t* og_occ = nullptr;                  // [voxels] the occupancy as uploaded, kept likewise
  int64_t og_tmp_cap = 0;                     // voxels the two hold
  // the self-collision spheres and the pairs of them (ddp_hip_self_collision_set_pairs)
  int32_t sc_np = 0, sc_npair = 0;            // spheres and pairs set (0: none yet)
  int32_t sc_joint[DDP_HIP_MAX_COLLISION_POINTS] = {};
  double sc_off[DDP_HIP_MAX_COLLISION_POINTS][3] = {};
  double sc_radius[DDP_HIP_MAX_COLLISION_POINTS] = {};
  int32_t sc_pa[DDP_HIP_MAX_COLLISION_PAIRS] = {}, sc_pb[DDP_HIP_MAX_COLLISION_PAIRS] = {};
  double* sc_clear_d = nullptr;               // [batch][T+1] what ddp_hip_self_collision_clearance hands back
  // the robot capsules and the pairs they take part in (ddp_hip_capsule_set_pairs)
  int32_t cp_nc = 0, cp_npair = 0;            // capsules and pairs set (0: none yet)
  int32_t cp_joint[DDP_HIP_MAX_CAPSULES] = {};
  double cp_end[DDP_HIP_MAX_CAPSULES][2][3] = {};
  double cp_radius[DDP_HIP_MAX_CAPSULES] = {};
  int32_t cp_pa[DDP_HIP_MAX_CAPSULE_PAIRS] = {}, cp_kind[DDP_HIP_MAX_CAPSULE_PAIRS] = {}, cp_pb[DDP_HIP_MAX_CAPSULE_PAIRS] = {};
  int32_t cp_nbox = 0;                        // the box shapes of the pairs of kind DDP_HIP_CAPSULE_VS_BOX (ddp_hip_capsule_set_boxes)
  double cp_half[DDP_HIP_MAX_CAPSULE_BOXES][3] = {};
  double* cp_clear_d = nullptr;               // [batch][T+1] what ddp_hip_capsule_clearance hands back
  // the relative-frame pairs (ddp_hip_relative_frame_set_pairs): base frame A = (rf_ja, rf_offa), tip frame B = (rf_jb, rf_offb)
  int32_t rf_np = 0;                          // pairs set (0: none yet)
  int32_t rf_ja[DDP_HIP_MAX_FRAME_PAIRS] = {}, rf_jb[DDP_HIP_MAX_FRAME_PAIRS] = {};
  double rf_offa[DDP_HIP_MAX_FRAME_PAIRS][3] = {}, rf_offb[DDP_HIP_MAX_FRAME_PAIRS][3] = {};
  double* rf_err_d = nullptr;                 // [batch][T+1][DDP_HIP_MAX_FRAME_PAIRS][6] what ddp_hip_relative_frame_error hands back
  // the aim frames (ddp_hip_frame_aim_set_frames): the eye fa_off and the unit axis fa_axis of joint fa_joint
  int32_t fa_nf = 0;                          // frames set (0: none yet)
  int32_t fa_joint[DDP_HIP_MAX_AIM_FRAMES] = {};
  double fa_off[DDP_HIP_MAX_AIM_FRAMES][3] = {}, fa_axis[DDP_HIP_MAX_AIM_FRAMES][3] = {};
  double* fa_err_d = nullptr;                 // [batch][T+1][DDP_HIP_MAX_AIM_FRAMES][2] what ddp_hip_frame_aim_error hands back

  // the balance-region planes (ddp_hip_balance_region_set_planes): a count alone, the planes themselves are per-instance data
  int32_t br_np = 0;                          // plane slots set (0: none yet)
  double* ja_acc_d = nullptr;                 // [batch][T][nv] what ddp_hip_joint_accel hands back
  double* br_margin_d = nullptr;              // [batch][T+1] what ddp_hip_balance_region_margin hands back

  bool box_dirty = false;       // CTRL_LO / CTRL_HI were uploaded since lo <= hi was last checked (ctx.hip: box_check)

  // the receding-horizon advance (advance.hip, advance_plan.h): allocated by the first ddp_hip_advance, freed by adv_teardown
  void* adv_tab_d = nullptr;    // the descriptor table, one record per array the shift moves
  double* adv_x0_d = nullptr;   // [batch][nx] the measured states on their way to X[0]
  int32_t adv_narr = 0;         // records in the table ...
  int64_t adv_blocks = 0;       // ... and the workgroups of one shift launch
  bool adv_dirty = true;        // a cost block's layout changed since the table was built (ctx.hip: cost_block_setup)
  std::vector<double> adv_mu_h, adv_step_h;   // [batch] what the closed-loop roll hands ddp_hip_forward

  bool async_mode = false;     // ddp_hip_set_async: entry points that hand nothing back to the host do not wait for the stream
  uint32_t profile_mask = 0;   // bit (1 + kernel_id): that kernel class is bracketed by HIP events
  ProfSlot prof[DDP_HIP_K_COUNT];
};

#define HIP_TRY(expr)                                   \
  do {                                                  \
    hipError_t e__ = (expr);                            \
    if (e__ != hipSuccess) { (void)hipGetLastError(); return DDP_HIP_E_HIP; } \
  } while (0)

// end of an entry point that returns nothing to the host: wait for the stream unless the context is in asynchronous mode
#define END_SYNC(ctx) do { if (!(ctx)->async_mode) HIP_TRY(hipStreamSynchronize((ctx)->stream)); } while (0)

// The side stream of the concurrent linearisation schedule.  lin_fork: it continues from where ctx->stream stands now; lin_join:
// ctx->stream continues only after what it holds.  Nothing else in the library looks at the side stream: the entry point that
// may fork holds a LinJoin, whose destructor joins whatever is still out, on every return path.
inline hipError_t lin_fork(ddp_hip_ctx* ctx) {
  hipError_t e = hipEventRecord(ctx->lin_ev_fork, ctx->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(ctx->lin_stream2, ctx->lin_ev_fork, 0);
  if (e == hipSuccess) ctx->lin_side_busy = true;
  return e;
}
inline hipError_t lin_join(ddp_hip_ctx* ctx) {
  if (!ctx->lin_side_busy) return hipSuccess;
  hipError_t e = hipEventRecord(ctx->lin_ev_done, ctx->lin_stream2);
  if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ctx->lin_ev_done, 0);
  // a join that cannot be enqueued leaves no order between the streams: the host waits instead
  if (e != hipSuccess) { (void)hipGetLastError(); (void)hipStreamSynchronize(ctx->lin_stream2); }
  ctx->lin_side_busy = false;
  return e;
}
struct LinJoin {
  ddp_hip_ctx* ctx;
  explicit LinJoin(ddp_hip_ctx* c) : ctx(c) {}
  LinJoin(const LinJoin&) = delete;
  LinJoin& operator=(const LinJoin&) = delete;
  ~LinJoin() { (void)lin_join(ctx); }
};

// profile helpers (ctx.hip)
void prof_begin(ddp_hip_ctx* ctx, int kid, hipStream_t stream = nullptr);   // stream: the one the kernel is launched on (default: the context's)
void prof_end(ddp_hip_ctx* ctx, int kid, hipStream_t stream = nullptr);

// per-op launchers implemented in their own translation units
int bwd_setup(ddp_hip_ctx* ctx);
SweepPlan sweep_plan(const ddp_hip_ctx* ctx);
void bwd_teardown(ddp_hip_ctx* ctx);
int bwd_lds_check(const ddp_hip_ctx* ctx);       // DDP_HIP_E_UNSUPPORTED if the sweep's kernels need more LDS than a workgroup has (nv = 64; with control bounds nv >= 58)
int box_check(ddp_hip_ctx* ctx);                  // control bounds: DDP_HIP_E_ARG if an upload left some lo > hi (ctx.hip)
int fwd_setup(ddp_hip_ctx* ctx);
bool fwd_lat_supported(const ddp_hip_ctx* ctx);   // the latency kernels of the forward sweep apply (tree, no constraints, Talos size)
void fwd_teardown(ddp_hip_ctx* ctx);
void adv_teardown(ddp_hip_ctx* ctx);              // advance.hip
int lin_setup(ddp_hip_ctx* ctx);
// the transitions of ctx->tensors (lin.hip); linearise's own two (about to write / has written the second order) are local to it
int tensors_written_outside(ddp_hip_ctx* ctx, int seq);   // ddp_hip_device_ptr / upload / fill of `seq`: a no-op unless it is FXX / FUX / FUU
int lin_materialize_fxx(ddp_hip_ctx* ctx);   // packed records back in the contract layout, the mirror images formed: FXX / FUX / FUU complete for readers other than the sweep they were left for
void lin_teardown(ddp_hip_ctx* ctx);

// best-cost pick, device side (pick.hip): {cost, global index} of the local best / of G gathered pairs
int pick_local_launch(ddp_hip_ctx* ctx, int64_t rank, int64_t nranks, double* out_pair, hipStream_t stream);
int pick_final_launch(const double* pairs, int G, double* out_pair, hipStream_t stream);

static inline int64_t seq_block_offset_regular(int64_t t, int64_t stride) { return t * stride; }
