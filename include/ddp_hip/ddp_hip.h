/*
 * ddp_hip.h -- C-ABI of the MI355X-native DDP sweep library (libddp_hip.so).
 *
 * This is the drop-in boundary of the build.  The reference (s-elkazdadi/ddp-pinocchio) has no
 * FFI: its seams are C++ template/ODR seams.  Each entry point below replaces one
 * reference interface (cited file:line, relative to the reference root) and is what a host-side
 * binding (the Eigen adapter of INTEGRATION.md, a ctypes stub, ...) would bind:
 *
 *   reference interface                                            entry point
 *   -------------------------------------------------------------  ---------------------------
 *   ddp_solver_t ctor + uninit_derivative_storage ddp.hpp:430-514   ddp_hip_create / _destroy
 *   model_t ctor (pinocchio_model.ipp:119-160)                      ddp_hip_create (model table)
 *   mat_seq_t::data() views  detail/mat_seq.hpp:43-44               ddp_hip_upload / _download / _device_ptr
 *   make_trajectory          ddp.hpp:392-415                        ddp_hip_rollout
 *   problem_t::compute_derivatives  problem.hpp:956-998             ddp_hip_linearize
 *   backward_pass<M>         ddp_bwd.ipp:9-155 (decl ddp.hpp:845)   ddp_hip_backward
 *   forward_pass<M>          ddp_fwd.ipp:9-67  (decl ddp.hpp:855)   ddp_hip_forward
 *   cost_seq_aug             ddp.hpp:699-735                        ddp_hip_cost_seq_aug
 *   swap(traj, new_traj)     ddp.hpp:826                            ddp_hip_swap_traj
 *   update_origin            detail/mat_seq_common.hpp:62-89        ddp_hip_update_origin
 *   optimality_obj / _constr ddp.hpp:576-627, 516-523               ddp_hip_optimality
 *   multiplier update        ddp.hpp:680-688 (in update_derivatives) ddp_hip_update_multipliers
 *   solve<M>                 ddp.hpp:745-842                        ddp_hip_solve (+ ddp_hip_set_active)
 *   (new: multi-seed shard)                           ddp_hip_comm_* / ddp_hip_shard_best
 *
 * Conventions
 *  - All scalars are IEEE double; all dimensions and indices int64_t (utils.hpp:117 index_t).
 *  - A context owns `batch` independent problem instances (same model and horizon, different
 *    trajectories / derivatives); every sequence is resident in HBM as [batch][flat], where `flat`
 *    is exactly the reference's flat layout: block t at sum_{s<t} rows(s)*cols(s), column-major
 *    (detail/mat_seq.hpp:61-73); tensors (i=out, j=left, k=right) at i + j*O + k*O*L
 *    (detail/tensor.hpp:141-147).  ddp_hip_seq_size() returns the per-instance element count.
 *  - Return value: 0 ok, >0 numerical event, <0 usage / HIP error.  Nothing throws, nothing
 *    terminates.  One context = one HIP stream; contexts are independent; a single context is not
 *    re-entrant.  There is NO CPU fallback: without a HIP device ddp_hip_create fails with
 *    DDP_HIP_E_NODEVICE.
 */
#ifndef DDP_HIP_H
#define DDP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDP_HIP_ABI_VERSION 3

enum {
  DDP_HIP_OK = 0,
  DDP_HIP_EV_LLT_RESTART = 1,       /* at least one instance restarted its backward sweep (ddp_bwd.ipp:105-132) */
  DDP_HIP_EV_LINESEARCH_FLOOR = 2,  /* at least one instance hit step < 1e-10 (ddp_fwd.ipp:35-37) */
  DDP_HIP_E_ARG = -1,
  DDP_HIP_E_HIP = -2,
  DDP_HIP_E_NODEVICE = -3,
  DDP_HIP_E_UNSUPPORTED = -4,
  DDP_HIP_E_MAX_RESTARTS = -5,
  DDP_HIP_E_COMM = -6
};

enum { DDP_HIP_MODEL_PENDULUM = 0, DDP_HIP_MODEL_TREE = 1 };
enum { DDP_HIP_EQ_NONE = 0, DDP_HIP_EQ_CONFIG = 1, DDP_HIP_EQ_FRAME = 2 };
/* FREEFLYER: joint 0 only (parent -1): an SE(3) joint, q = [p(3), quaternion x y z w], v = [linear(3), angular(3)] in the
 * body frame (Pinocchio's JointModelFreeFlyer); the model then has nq = nv + 1 and nv - 5 joints.  Derivatives are taken in
 * the tangent along q (+) delta = integrate(q, delta); with either first order, fd_mode 0 or 2 and no config constraint */
enum { DDP_HIP_JOINT_REVOLUTE = 0, DDP_HIP_JOINT_PRISMATIC = 1, DDP_HIP_JOINT_FREEFLYER = 2 };

#define DDP_HIP_MAX_JOINTS 64

/* Model concept (pinocchio_model.hpp:77-186, pendulum_model.hpp:10-133): a tree of 1-DoF joints (nq == nv, the case FD
 * mode 1 requires: problem.hpp:78-81), optionally hanging from a free-flyer root (a Lie-group configuration, nq = nv + 1:
 * pinocchio_model.ipp:222-321), or the closed-form pendulum.  The per-joint arrays have nv entries, nv - 5 with a free flyer. */
typedef struct ddp_hip_model {
  int32_t kind;
  int32_t nv;                    /* velocity / tangent dimension */
  double mass, length;           /* pendulum: pendulum_model.hpp:24-26 (g = 9.81) */
  const int32_t* parent;         /* [nv], parent[i] < i, -1 = world */
  const int32_t* jtype;          /* [nv] DDP_HIP_JOINT_* */
  const double* axis;            /* [nv*3] unit joint axis, joint frame */
  const double* Rp;              /* [nv*9] row-major: parent coords = Rp * joint coords */
  const double* pp;              /* [nv*3] joint origin in the parent frame */
  const double* mass_j;          /* [nv] */
  const double* com;             /* [nv*3] */
  const double* Ic;              /* [nv*9] rotational inertia about the com */
  double gravity[3];
} ddp_hip_model;

/* problem_t / dynamics_t / constraint chain (problem.hpp:343-525, 527-870, 872-1150) */
typedef struct ddp_hip_problem {
  ddp_hip_model model;
  double dt;                     /* dynamics_t::dt  problem.hpp:522 */
  double c;                      /* problem_t::c    problem.hpp:1147 */
  int64_t T;                     /* horizon; index_begin = 0, index_end = T */
  int64_t batch;                 /* independent instances resident in this context */
  int32_t eq_kind;               /* DDP_HIP_EQ_* */
  int32_t eq_advance;            /* constraint_advance_time_t wrappers (reference drivers: 2) */
  const int64_t* ne;             /* [T] eq rows at solver time t; NULL = no constraints */
  const double* eq_target;       /* concatenated over t, ne[t] doubles each (shared by the batch) */
  int32_t frame_joint;
  double frame_off[3];
  int32_t first_order_fd;        /* 0 analytic (the pendulum's closed form; trees: ABA derivatives, free-flyer root included,
                                    nv <= 38 with a free flyer), 1 forward FD with eps = sqrt(DBL_EPSILON) */
  int32_t fd_mode;               /* second order: 0 none (tensors zero), 1 problem.hpp:67-150, 2 problem.hpp:152-298 */
} ddp_hip_problem;

/* resident sequences (derivative_storage_t ddp.hpp:52-245, trajectory_t trajectory.hpp:9-113,
 * affine_vector_function_seq_t mat_seq_common.hpp:12-177) */
enum ddp_hip_seq {
  DDP_HIP_SEQ_X = 0, DDP_HIP_SEQ_U, DDP_HIP_SEQ_X_NEW, DDP_HIP_SEQ_U_NEW,
  DDP_HIP_SEQ_LFX, DDP_HIP_SEQ_LFXX,
  DDP_HIP_SEQ_LX, DDP_HIP_SEQ_LU, DDP_HIP_SEQ_LXX, DDP_HIP_SEQ_LUX, DDP_HIP_SEQ_LUU,
  DDP_HIP_SEQ_F_VAL, DDP_HIP_SEQ_FX, DDP_HIP_SEQ_FU, DDP_HIP_SEQ_FXX, DDP_HIP_SEQ_FUX, DDP_HIP_SEQ_FUU,
  DDP_HIP_SEQ_EQ_VAL, DDP_HIP_SEQ_EQ_X, DDP_HIP_SEQ_EQ_U, DDP_HIP_SEQ_EQ_XX, DDP_HIP_SEQ_EQ_UX, DDP_HIP_SEQ_EQ_UU,
  DDP_HIP_SEQ_MULT_ORIGIN, DDP_HIP_SEQ_MULT_VAL, DDP_HIP_SEQ_MULT_JAC,
  DDP_HIP_SEQ_FB_ORIGIN, DDP_HIP_SEQ_FB_VAL, DDP_HIP_SEQ_FB_JAC,
  DDP_HIP_SEQ_VX_TRACE, DDP_HIP_SEQ_VXX_TRACE,   /* V_x / V_xx after every step (parity only) */
  DDP_HIP_SEQ_COSTS_OLD, DDP_HIP_SEQ_COSTS_NEW,  /* T+1 doubles each (cost_seq_aug) */
  /* per-instance quadratic tracking cost (DDP_HIP_FLAG_TRACKING_COST; not allocated without it) */
  DDP_HIP_SEQ_COST_XREF,   /* [T+1][nx] reference states (create: the neutral state: q neutral, unit root quaternion, v = 0) */
  DDP_HIP_SEQ_COST_WX,     /* [T+1][n]  state weights, tangent rows (create: 0) */
  DDP_HIP_SEQ_COST_UREF,   /* [T][m]    reference controls (create: 0) */
  DDP_HIP_SEQ_COST_WU,     /* [T][m]    control weights (create: 0) */
  /* per-instance control bounds (DDP_HIP_FLAG_CONTROL_BOUNDS; not allocated without it) */
  DDP_HIP_SEQ_CTRL_LO,     /* [T][m]    lower bounds on u_t (create: -inf = none) */
  DDP_HIP_SEQ_CTRL_HI,     /* [T][m]    upper bounds on u_t (create: +inf = none) */
  DDP_HIP_SEQ_BOX_STAT,    /* [T][2]    written by ddp_hip_backward: clamped controls, projected-Newton iterations of step t */
  DDP_HIP_SEQ_COUNT
};

typedef struct ddp_hip_ctx ddp_hip_ctx;

/* create flags */
#define DDP_HIP_FLAG_NO_TENSORS 1u   /* do not allocate fxx/fux/fuu/eq_xx/eq_ux/eq_uu (Gauss-Newton sweeps only) */
#define DDP_HIP_FLAG_TRACE 2u        /* allocate the V_x / V_xx trace sequences */
/* Allocate the COST_* sequences and optimise, per instance b, with d_t = x_t (-) xref[b][t] (lie::difference_x: a plain
 * subtraction on vector-space models, log6(Mref^-1 M) on a free-flyer root's six rows):
 *   l(t, x, u) = c/2 |u|^2 + 1/2 sum_i wx[t][i] d_i^2 + 1/2 sum_j wu[t][j] (u_j - uref[t][j])^2      t < T
 *   lf(x_T)    = 1/2 sum_i wx[T][i] d_T,i^2
 * instead of the reference's fixed c/2 |u|^2, lf = 0 (problem.hpp:932-942); the constraint terms of cost_seq_aug are unchanged.
 * Derivatives in the tangent at x, J = dd/ddx (the identity but on a free-flyer root block: Jlog6(d_root)):
 *   lx = J^T (wx o d), lxx = J^T diag(wx) J, lu = c u + wu o (u - uref), luu = c I + diag(wu), lux = 0, lfx / lfxx alike at T.
 * lxx is exact on vector-space models and Gauss-Newton on the root block (the term sum_i wx_i d_i d^2(d_i) is dropped: exact
 * where d_root = 0).  ddp_hip_upload refuses (DDP_HIP_E_ARG) negative or non-finite weights and, on a free-flyer model, a
 * reference root quaternion with | |quat| - 1 | > 1e-10; writes through ddp_hip_device_ptr are the caller's responsibility.
 * A term of weight 0 is left out (not multiplied by 0): with all weights 0 a context computes bit for bit what it computes
 * without the flag. */
#define DDP_HIP_FLAG_TRACKING_COST 4u
/* Allocate CTRL_LO / CTRL_HI / BOX_STAT and keep lo[t] <= u_t <= hi[t], per instance (control-limited DDP: Tassa, Mansard,
 * Todorov, ICRA 2014).  The backward step solves, instead of Q_uu k = -Q_u over R^m, the box QP
 *   min_k 1/2 k^T H k + Q_u^T k,  lo_t - u_t <= k <= hi_t - u_t,   H = Q_uu + reg I (lower triangle)
 * by projected Newton steps (at most 32; Armijo 0.1, halving) from k = clip(0), then takes k and K from the final clamped set
 * alone: k_c on its bound, k_f = -H_ff^-1 (Q_u,f + H_fc k_c), K_c = 0, K_f = -H_ff^-1 Q_ux,f.  A pivot <= 0 of any H_ff fails the
 * step as ddp_bwd.ipp:105-110 does.  V_x / V_xx keep the reference's lines.  The forward rollouts clamp u = u < lo ? lo : (u > hi ?
 * hi : u) after the control update (ddp_fwd.ipp:47-49; ddp_hip_rollout applies U as given), and optimality_obj leaves out the
 * components of a control on a bound whose gradient points out of the box.  -inf / +inf: no bound on that side.  ddp_hip_upload
 * refuses (DDP_HIP_E_ARG) a NaN, a lo of +inf, a hi of -inf; ddp_hip_backward / ddp_hip_forward return DDP_HIP_E_ARG if some
 * lo > hi (checked after an upload of either); writes through ddp_hip_device_ptr are the caller's responsibility.  With bounds
 * that never bind a context computes bit for bit what it computes without the flag. */
#define DDP_HIP_FLAG_CONTROL_BOUNDS 8u
/* Carry up to DDP_HIP_MAX_COST_FRAMES cost frames -- frame f is the point off_f fixed in joint joint_f (the convention of
 * ddp_hip_problem.frame_joint / frame_off), shared by the batch -- and add, per instance b, with p_f(q) the frame's world
 * position, targets g[b][t][f] in R^3 and weights w[b][t][f] in R^3 (per world axis, >= 0), r_f = p_f(q_t) - g[b][t][f]:
 *   l(t, x, u) += 1/2 sum_f sum_a w[b][t][f][a] r_f,a^2      t < T
 *   lf(x_T)    += 1/2 sum_f sum_a w[b][T][f][a] r_f,a^2
 * to whatever the context optimises otherwise (c/2 |u|^2, the tracking terms, the constraint terms of cost_seq_aug).
 * Derivatives in the tangent at x, P_f = dp_f / d(delta q) (3 x nv, the true point jacobian: a_i x (p_f - o_i) for a revolute
 * joint i on the path root .. joint_f with world axis a_i and world origin o_i, a_i for a prismatic one, R_0 e_c and
 * (R_0 e_c) x (p_f - o_0) on a free-flyer root; NOT the WORLD-frame rows of ddp_hip_model_frame):
 *   lx[q rows] += sum_f P_f^T (w o r_f),  lxx[q, q] += sum_f P_f^T diag(w) P_f,  lfx / lfxx alike at T;
 * velocity rows and columns, lu, luu and lux are untouched.  lxx is Gauss-Newton (the term sum_a w_a r_a d^2 p_a is dropped:
 * exact where r = 0) and symmetric bit for bit.  The frame data travels through ddp_hip_frame_cost_* below, not through
 * ddp_hip_upload.  At create there are no frames; tree models only (a pendulum: DDP_HIP_E_UNSUPPORTED).  A term of weight 0 is
 * left out (not multiplied by 0): with no frames or all weights 0 a context computes bit for bit what it computes without the
 * flag. */
#define DDP_HIP_FLAG_FRAME_COST 16u
#define DDP_HIP_MAX_COST_FRAMES 4
/* Carry, per instance b, t = 0 .. T and tangent row i = 0 .. n-1 (n = 2 nv: configuration rows 0 .. nv-1, velocity rows
 * nv .. 2nv-1), a lower bound lo, an upper bound hi and a weight w >= 0, and add the soft limit (a one-sided quadratic penalty
 * on the amount by which a state coordinate leaves [lo, hi]) to whatever the context optimises otherwise.  With s_i(x) the
 * state coordinate of row i (x[i + nq - nv] for i < nv, else x[nq + i - nv]):
 *   e_i = s_i < lo_i ? s_i - lo_i : (s_i > hi_i ? s_i - hi_i : 0)
 *   l(t, x, u) += 1/2 sum_i w[b][t][i] e_i^2      t < T
 *   lf(x_T)    += 1/2 sum_i w[b][T][i] e_i^2
 * Derivatives in the tangent at x, for the rows with w_i != 0 and e_i != 0 only:
 *   lx[i] += w_i e_i,  lxx[i][i] += w_i,  lfx / lfxx alike at T;
 * lu, luu, lux and the off-diagonal entries are untouched.  The Hessian is exact wherever the cost is twice differentiable
 * and positive semidefinite.  -inf / +inf: no bound on that side.  At create lo = -inf, hi = +inf, w = 0.  A term with w = 0
 * or e = 0 is left out (not multiplied by 0), and a row of weight 0 reads neither bound.  Tangent rows 0 .. 5 of a free-flyer
 * root are a pose on SE(3) and carry no limit; its six velocity rows and every 1-DoF joint's rows are ordinary rows.  The
 * pendulum is supported.  The data travels through ddp_hip_state_limits_* below, not through ddp_hip_upload; an upload is refused
 * (DDP_HIP_E_ARG, nothing written) for a NaN, a lo of +inf, a hi of -inf, a negative or non-finite weight, a non-zero weight on rows
 * 0 .. 5 of a free-flyer model and lo > hi.  Two exactness properties: with nothing uploaded or every weight 0, and with
 * non-zero weights and bounds that neither the trajectory nor any line-search candidate violates, a context computes bit for
 * bit what it computes without the flag. */
#define DDP_HIP_FLAG_STATE_LIMITS 32u
/* Give the cost frames of DDP_HIP_FLAG_FRAME_COST (valid only together with it: alone, ddp_hip_create returns DDP_HIP_E_ARG) an
 * orientation term, which makes a cost frame a full placement cost.  With R_f(q) the world rotation of joint joint_f's frame
 * (world = R body; off_f plays no part), per instance b a reference rotation given as a unit quaternion r[b][t][f] = (x y z w)
 * (the convention of the free-flyer root) with rotation R_ref, and weights w[b][t][f] in R^3 (>= 0):
 *   e_f = log3(R_ref^T R_f(q_t)) in R^3, |e_f| <= pi
 *   l(t, x, u) += 1/2 sum_f sum_a w[b][t][f][a] e_f,a^2      t < T
 *   lf(x_T)    += 1/2 sum_f sum_a w[b][T][f][a] e_f,a^2
 * to whatever the context optimises otherwise.  The components of e are along the frame's own axes, which are the reference
 * frame's too (exp(e) e = e): w = (w, w, 0) on a foot whose z axis is vertical at the target means "flat, yaw free".
 * Derivatives in the tangent at x, W_f (3 x nv) the world angular jacobian (the world axis a_i of a revolute joint i on the path
 * root .. joint_f, R_0 e_c for the angular columns 3 .. 5 of a free-flyer root; a prismatic joint and the root's linear columns
 * have no column), A_f = Jlog3(e_f) R_f^T W_f, Jlog3(e) = I + 1/2 [e]x + d(|e|^2) [e]x^2:
 *   lx[q rows] += sum_f A_f^T (w o e_f),  lxx[q, q] += sum_f A_f^T diag(w) A_f,  lfx / lfxx alike at T;
 * velocity rows and columns, lu, luu and lux are untouched, and columns that carry no rotation are left out, not added as
 * zeros.  lxx is Gauss-Newton (the term sum_a w_a e_a d^2 e_a is dropped: exact where e = 0), positive semidefinite and symmetric
 * bit for bit.  At |e| = pi the log is not differentiable: the value there is what the quaternion logarithm gives (one of the
 * two axes +-e, decided by rounding), and r and -r are the same reference.  At create every quaternion is (0, 0, 0, 1) and every
 * weight 0.  The data travels through ddp_hip_frame_orient_* below, not through ddp_hip_upload or ddp_hip_device_ptr.  A term of
 * weight 0 is left out (not multiplied by 0), a frame whose three orientation weights are 0 is not walked, and position and
 * orientation weights are independent: with nothing uploaded or all orientation weights 0 a context computes bit for bit what
 * it computes with DDP_HIP_FLAG_FRAME_COST alone. */
#define DDP_HIP_FLAG_FRAME_ORIENT_COST 64u
/* Give every instance a centre-of-mass (CoM) tracking term: balance tasks.  The model is a tree with body masses m_i (mass_j),
 * body CoMs c_i in the joint frame (com) and total mass M = sum_i m_i > 0 (else ddp_hip_create returns DDP_HIP_E_ARG):
 *   c(q) = (1/M) sum_i m_i p_i(q),      p_i(q) = world position of the point c_i of joint i
 * Per instance b and t = 0 .. T a target g[b][t] in R^3 and weights w[b][t] in R^3 (per world axis, >= 0), r = c(q_t) - g[b][t]:
 *   l(t, x, u) += 1/2 sum_a w[b][t][a] r_a^2      t < T
 *   lf(x_T)    += 1/2 sum_a w[b][T][a] r_a^2
 * to whatever the context optimises otherwise; "CoM over the foot, height free" is w = (w, w, 0).
 * Derivatives in the tangent at x, Jc = dc / d(delta q) (3 x nv), by column, with m_sub_j and c_sub_j the mass and the CoM of
 * the subtree rooted at joint j (itself included), a_j the world axis and o_j the world origin of joint j:
 *   revolute joint j:   (m_sub_j / M) a_j x (c_sub_j - o_j)          prismatic joint j:   (m_sub_j / M) a_j
 *   free-flyer root (body twists, linear part first): R_0 e_c for the linear columns, (R_0 e_c) x (c - o_0) for the angular ones;
 * equivalently Jc = (1/M) sum_i m_i P_i with P_i the true point jacobian of DDP_HIP_FLAG_FRAME_COST.
 *   lx[q rows] += Jc^T (w o r),  lxx[q, q] += Jc^T diag(w) Jc,  lfx / lfxx alike at T;
 * velocity rows and columns, lu, luu and lux are untouched.  lxx is Gauss-Newton (the term sum_a w_a r_a d^2 c_a is dropped:
 * exact where r = 0); entry (i, j) is formed in (min, max) order with the axes in fixed order: symmetric bit for bit.  The data
 * travels through ddp_hip_com_cost_* below, not through ddp_hip_upload or ddp_hip_device_ptr.  At create targets and weights
 * are 0.  A term of weight 0 is left out (not multiplied by 0); with nothing uploaded or every weight 0 a context computes bit
 * for bit what it computes without the flag.  Tree models only (the pendulum: DDP_HIP_E_UNSUPPORTED).  The flag combines with
 * every other flag: the terms are formed by kernels of their own, which add onto what the other terms' kernels leave. */
#define DDP_HIP_FLAG_COM_COST 128u
/* Give every cost frame of DDP_HIP_FLAG_FRAME_COST a velocity term as well: "arrive at rest", "touch down with zero foot
 * velocity", "move the hand along x at 0.2 m/s".  Valid only together with DDP_HIP_FLAG_FRAME_COST (alone: ddp_hip_create returns
 * DDP_HIP_E_ARG); the frames are those of ddp_hip_frame_cost_set_frames.  For frame f (point off_f of joint joint_f, world position
 * p_f), with P_f the true point jacobian and W_f the world angular jacobian of the two flags above, the frame's velocity in
 * world-aligned axes is
 *   pdot_f = P_f(q) v   (the point's linear velocity),      omega_f = W_f(q) v   (the angular velocity of joint_f's frame)
 * with v the tangent velocity of the state (on a free-flyer root its first six entries are the body twist, linear part first).
 * Per instance b, t = 0 .. T and frame f a target g[b][t][f] in R^6 (desired linear, then angular velocity, world axes) and weights
 * w[b][t][f] in R^6 (>= 0), r_f = (pdot_f - g_lin, omega_f - g_ang):
 *   l(t, x, u) += 1/2 sum_f sum_a w[b][t][f][a] r_f,a^2      t < T
 *   lf(x_T)    += 1/2 sum_f sum_a w[b][T][f][a] r_f,a^2
 * to whatever the context optimises otherwise.  Derivatives in the tangent at x: A_f = [ dr/d(delta q) | dr/dv ] (6 x 2 nv), the
 * right half [P_f; W_f], the left half [D; E] by column of the joints j on the path root .. joint_f, with a_j the world axis and
 * o_j the world origin of joint j and the prefix sums over the path joints up to and including j (the root's six columns
 * included)  omega_<=j = sum_{i<=j} W_i v_i,  pdot_<=j = sum_{i<=j} P_i v_i:
 *   revolute j:    D_j = omega_<=j x (a_j x (p_f - o_j)) + a_j x (pdot_f - pdot_<=j),      E_j = a_j x (omega_f - omega_<=j)
 *   prismatic j:   D_j = omega_<=j x a_j,                                                  E_j = 0
 *   free-flyer root: linear columns 0 .. 2: D = E = 0;  angular column 3 + c: D = (R_0 e_c) x pdot_f,  E = (R_0 e_c) x omega_f
 *   lx[rows] += sum_f A_f^T (w o r_f),   lxx[rows, rows] += sum_f A_f^T diag(w) A_f,   lfx / lfxx alike at T,
 * the rows being the path's q rows and v rows: the term fills the q-q, q-v, v-q and v-v blocks on the path.  Rows and columns off
 * the path, lu, luu and lux are untouched; columns that carry nothing (a prismatic joint's angular part, the root's linear D
 * columns) are left out, not added as zeros.  lxx is Gauss-Newton (the term sum_a w_a r_a d^2 r_a is dropped: exact where r = 0,
 * positive semidefinite); entry (i, j) is formed in (min, max) order with the frames and axes in fixed order: symmetric bit for
 * bit.  The data travels through ddp_hip_frame_vel_* below.  At create targets and weights are 0.  A term of weight 0 is left out
 * (not multiplied by 0): a frame whose six weights are 0 is not walked, one whose three angular (linear) weights are 0 forms no
 * angular (linear) quantities, and with nothing uploaded or every weight 0 a context computes bit for bit what it computes with
 * DDP_HIP_FLAG_FRAME_COST alone.  The flag combines with every other flag: the terms are formed by kernels of their own, which
 * add onto what the other terms' kernels leave (after the CoM's). */
#define DDP_HIP_FLAG_FRAME_VEL_COST 256u
/* Say where the robot must not go: collision spheres on the robot against obstacles that every instance carries for itself, as
 * a one-sided soft cost -- "reach past the table edge", "the swing foot clears the step", "stay 10 cm away from that person".
 * Collision points, shared by the batch, up to DDP_HIP_MAX_COLLISION_POINTS: point k is the point off_k fixed in joint joint_k
 * (the convention of the cost frames) with a radius r_k >= 0, a sphere on the robot; p_k(q) is its world position.  Obstacle
 * slots, shared by the batch, up to DDP_HIP_MAX_OBSTACLES: slot o has a kind, DDP_HIP_OBSTACLE_SPHERE or
 * DDP_HIP_OBSTACLE_HALFSPACE.  Per instance b, t = 0 .. T and slot o four doubles geom[b][t][o] and a weight w[b][t][o] >= 0
 * (per-instance scenes; obstacles that move with t):
 *   sphere:      geom = (centre c, radius rho >= 0),             d_ko = |p_k - c| - (r_k + rho),   u_ko = (p_k - c) / |p_k - c|
 *   half-space:  geom = (unit normal n, offset h), free side n . p >= h,   d_ko = n . p_k - h - r_k,   u_ko = n
 * A safety margin is part of the radii or of the offset.  With e_ko = d_ko < 0 ? d_ko : 0:
 *   l(t, x, u) += 1/2 sum_k sum_o w[b][t][o] e_ko^2      t < T
 *   lf(x_T)    += 1/2 sum_k sum_o w[b][T][o] e_ko^2
 * to whatever the context optimises otherwise.  Derivatives in the tangent at x, with P_k the true point jacobian of
 * DDP_HIP_FLAG_FRAME_COST and z_ko = P_k^T u_ko, over the pairs with w != 0 and e != 0 only:
 *   lx[q rows] += sum w e_ko z_ko,   lxx[q rows, q rows] += sum w z_ko z_ko^T,   lfx / lfxx alike at T.
 * Velocity rows and columns, lu, luu, lux and the q rows off every active point's path are untouched.  lxx is Gauss-Newton (the
 * curvature of the sphere distance and d^2 p_k are dropped: positive semidefinite); entry (i, j) is formed in (min, max) order
 * with the points, then the slots in ascending order: symmetric bit for bit.  A sphere pair with |p_k - c| == 0 contributes its
 * value 1/2 w (r_k + rho)^2 and no derivative.  A pair with w == 0 or e == 0 is left out (not multiplied by 0, not added as
 * +0): with nothing uploaded, with every weight 0, and with non-zero weights on obstacles that neither the trajectory nor any
 * line-search candidate touches, a context computes bit for bit what it computes without the flag.  The data travels through
 * ddp_hip_obstacle_* below; at create no points are set and geometry and weights are 0.  Tree models only (the pendulum:
 * DDP_HIP_E_UNSUPPORTED).  The flag combines with every other flag: the terms are formed by kernels of their own, which add onto
 * what the other terms' kernels leave (last, after the frame velocities').
 *
 * A third slot kind, DDP_HIP_OBSTACLE_GRID, reads its distance from a voxel grid: a workspace as a depth camera sees it, which
 * eight primitives cannot say.  The context holds at most one grid, shared by the batch and by every slot of the kind
 * (ddp_hip_obstacle_set_grid takes a signed distance field, ddp_hip_obstacle_set_occupancy builds one on the device from occupancy
 * voxels): dims (nx, ny, nz), 2 <= n_a <= DDP_HIP_MAX_GRID_DIM, origin[3] the world position of node (0, 0, 0), cell > 0 the node
 * spacing on the three axes, and nx ny nz doubles phi[(ix ny + iy) nz + iz].  The slot's four doubles are geom = (shift s(3),
 * margin m), all finite, m of either sign: every instance can see the scene displaced, and a scanned object can move with t.
 * The distance is the trilinear interpolant and the direction its gradient:
 *   s = (p_k - shift - origin) / cell (per axis);  inside iff 0 <= s_a <= n_a - 1 on the three axes
 *   i_a = min(floor(s_a), n_a - 2),  f_a = s_a - i_a
 *   phi(p)  = sum over the 8 corners c of phi[i + c] prod_a (c_a ? f_a : 1 - f_a)
 *   grad_a  = (1 / cell) sum over the 8 corners c of phi[i + c] (c_a ? +1 : -1) prod_{b != a} (c_b ? f_b : 1 - f_b)
 *   d_ko = phi(p_k) - r_k - m,   u_ko = grad phi(p_k)      (not normalised: it is dd/dp of this d)
 * Outside the grid is free space: d = +inf, the pair forms nothing and ddp_hip_obstacle_clearance does not see it -- size the grid
 * to the workspace and close it with half-space slots where that matters.  A gradient that is exactly zero has the pair's value
 * and no derivative (the rule of a sphere's centre at p); a non-finite point is NaN as for the other kinds.  Everything else is
 * the text above: e, z = P_k^T u, the pairs left out, the bit-for-bit rules.  A context whose slots are all spheres and
 * half-spaces computes the same bits whether or not a grid is resident.  ddp_hip_advance shifts a grid slot's geom and weight
 * rows like the others'; the grid itself is not a per-t table and stays. */
#define DDP_HIP_FLAG_OBSTACLE_COST 512u
#define DDP_HIP_MAX_COLLISION_POINTS 16
#define DDP_HIP_MAX_OBSTACLES 8
#define DDP_HIP_OBSTACLE_SPHERE 0
#define DDP_HIP_OBSTACLE_HALFSPACE 1
#define DDP_HIP_OBSTACLE_GRID 2
#define DDP_HIP_MAX_GRID_DIM 256
/* Say "do not run one part of the robot through another": pairs of spheres on the robot, a one-sided soft cost on their distance
 * -- "the hand stays out of the torso", "the knees do not cross".  Both ends of a pair move with q, which the obstacle flag cannot
 * express.  The flag stands alone: it needs no DDP_HIP_FLAG_OBSTACLE_COST and has its own spheres.  Spheres, shared by the batch,
 * up to DDP_HIP_MAX_COLLISION_POINTS: sphere k is the point off_k fixed in joint joint_k (the convention of the cost frames and
 * of the obstacle flag's collision points) with a radius r_k >= 0; p_k(q) is its world position.  Pairs, shared by the batch, up
 * to DDP_HIP_MAX_COLLISION_PAIRS: pair i = (a_i, b_i) of sphere indices, the two on different joints.  Per instance b, t = 0 .. T
 * and pair i a margin m[b][t][i] (finite, may be negative) and a weight w[b][t][i] >= 0:
 *   D_i = |p_a - p_b|,   d_i = D_i - (r_a + r_b + m_i),   u_i = (p_a - p_b) / D_i
 *   e_i = d_i < 0 ? d_i : 0          (a NaN distance is active and its term NaN)
 *   l(t, x, u) += 1/2 sum_i w[b][t][i] e_i^2      t < T
 *   lf(x_T)    += 1/2 sum_i w[b][T][i] e_i^2
 * to whatever the context optimises otherwise.  Derivatives in the tangent at x, over the pairs with w != 0, e != 0 and D_i != 0
 * only, with P_k the true point jacobian of DDP_HIP_FLAG_FRAME_COST:
 *   z_i[c] = + P_a[:, c] . u_i     c a tangent column of path(a_i) that is not on path(b_i)
 *   z_i[c] = - P_b[:, c] . u_i     c a tangent column of path(b_i) that is not on path(a_i)
 *            nothing                c on both paths or on neither
 *   lx[q rows] += sum_i w e_i z_i,   lxx[q rows, q rows] += sum_i w z_i z_i^T,   lfx / lfxx alike at T.
 * The distance of two points does not change when a common ancestor joint moves: for a column on both paths the two
 * contributions cancel (a revolute joint: a x (p_a - p_b) is perpendicular to u; a prismatic one: a - a = 0; a free-flyer root:
 * the same in its six columns), and such a column is left out, not added as rounding residue.  The term therefore touches the
 * symmetric difference of the two paths only; velocity rows and columns, lu, luu, lux, every q row outside the symmetric
 * differences of the active pairs and a free-flyer root's six rows are untouched.  lxx is Gauss-Newton (the term w e grad^2 d is
 * dropped: positive semidefinite); entry (r, c) is formed in (min, max) order with the pairs in ascending order: symmetric bit
 * for bit, no atomics.  A pair with D_i == 0 contributes its value 1/2 w (r_a + r_b + m)^2 and no derivative.  A pair with
 * w == 0 or e == 0 is left out (not multiplied by 0, not added as +0): with nothing uploaded, with every weight 0, and with
 * non-zero weights on pairs that neither the trajectory nor any line-search candidate brings within their margin, a context
 * computes bit for bit what it computes without the flag.  The data travels through ddp_hip_self_collision_* below; at create no
 * pairs are set and margins and weights are 0.  Tree models only (the pendulum: DDP_HIP_E_UNSUPPORTED).  The flag combines with
 * every other flag: the terms are formed by kernels of their own, which add onto what the other terms' kernels leave (last,
 * after the obstacles'). */
#define DDP_HIP_FLAG_SELF_COLLISION_COST 1024u
#define DDP_HIP_MAX_COLLISION_PAIRS 32
/* Say how much momentum the robot as a whole may carry: "do not build up angular momentum in the swing phase", "land with zero
 * momentum", "regulate the CoM velocity to 0.3 m/s forward", "spin up for the jump".  The flag stands alone and needs no other
 * flag.  The centroidal momentum h(q, v) = A_G(q) v in world-aligned axes: for body j with mass m_j, p_j(q) the world position of
 * its CoM (point com[j] of joint j), R_j the world rotation of joint j's frame, I_j = R_j Ic_j R_j^T, omega_j the angular velocity
 * of that frame and pdot_j the velocity of p_j (omega_f and pdot_f of DDP_HIP_FLAG_FRAME_VEL_COST for the frame (j, com[j])),
 * M = sum_j m_j and c = sum_j m_j p_j / M,
 *   l = sum_j m_j pdot_j                                     (linear momentum, M cdot)
 *   k = sum_j [ m_j (p_j - c) x pdot_j + I_j omega_j ]       (angular momentum about the centre of mass)
 *   h = (l, k) in R^6.
 * Per instance b and t = 0 .. T a target g[b][t] in R^6 and weights w[b][t] in R^6 (>= 0), r = h - g[b][t]:
 *   l(t, x, u) += 1/2 sum_a w[b][t][a] r_a^2      t < T
 *   lf(x_T)    += 1/2 sum_a w[b][T][a] r_a^2
 * to whatever the context optimises otherwise; with w = (w, w, w, 0, 0, 0) a CoM-velocity cost scaled by M^2.  Derivatives in the
 * tangent at x, A = [ dh/d(delta q) | dh/dv ] (6 x 2 nv), by column, formed by subtree with spatial quantities about the world
 * origin: S_i = (al, be) joint i's axis as a twist (revolute: al = a_i, be = o_i x a_i; prismatic: al = 0, be = a_i, with a_i the
 * world axis and o_i the world origin of joint i), V_i = (omega_i, vO_i) body i's twist, and for a motion (al', be') the momentum
 * of the subtree rooted at i (itself included)
 *   I_sub(i)(al', be') = sum_{j in sub(i)} ( m_j u_j,  p_j x m_j u_j + I_j al' ),   u_j = be' + al' x p_j;
 * with (l_sub, kO_sub) the subtree's momentum about the origin:
 *   (lv, kv) = I_sub(i)(S_i)                          dh/dv_i = ( lv,  kv - c x lv )
 *   X = S_i x V_i = ( al x omega_i,  al x vO_i + be x omega_i ),      (l2, k2) = I_sub(i)(X)
 *   lq = al x l_sub - l2,    kq = al x kO_sub + be x l_sub - k2       dh/dq_i = ( lq,  kq - (lv / M) x l - c x lq )
 *   free-flyer root (body twists, linear part first; e_c column c of R_0): dh/dv = (M e_c, 0) for the linear columns and I_sub(0)
 *   applied to (e_c, o_0 x e_c), shifted to c alike, for the angular ones; dh/dq = 0 for the linear columns and (e_c x l, e_c x k)
 *   for the angular ones.
 *   lx += A^T (w o r) over all 2 nv rows,   lxx += A^T diag(w) A  (the q-q, q-v, v-q and v-v blocks),   lfx / lfxx alike at T;
 * lu, luu and lux are untouched.  Columns that are identically zero (the root's linear dh/dq, the angular part of the root's
 * linear dh/dv) are left out, not added as rounding residue.  lxx is Gauss-Newton (the term sum_a w_a r_a d^2 h_a is dropped: exact
 * where r = 0, positive semidefinite); entry (i, j) is formed in (min, max) order with the axes in fixed order: symmetric bit for
 * bit, no atomics.  The data travels through ddp_hip_momentum_cost_* below.  At create targets and weights are 0.  A term of
 * weight 0 is left out (not multiplied by 0): a block whose six weights are 0 forms nothing, one whose three angular weights
 * are 0 forms no inertia and no angular momentum, and with nothing uploaded or every weight 0 a context computes bit for bit what
 * it computes without the flag.  Tree models only (the pendulum: DDP_HIP_E_UNSUPPORTED); a total mass M <= 0 is DDP_HIP_E_ARG.
 * The flag combines with every other flag: the terms are formed by kernels of their own, which add onto what the other terms'
 * kernels leave (after the frame velocities', before the obstacles'). */
#define DDP_HIP_FLAG_MOMENTUM_COST 2048u
/* Say "keep this frame where it is relative to that frame": "carry the box: the right hand stays 30 cm from the left one, in the
 * left hand's axes, palm facing it", "keep the tray level relative to the chest while the legs walk", "keep the feet parallel and a
 * hip-width apart".  Two world-frame targets would fix the pair's common motion too, which is what such a task wants left free.
 * The flag stands alone: it needs no DDP_HIP_FLAG_FRAME_COST and has its own frames.  Pairs, shared by the batch, up to
 * DDP_HIP_MAX_FRAME_PAIRS: pair i has a base frame A = (joint ja_i, point offa_i) and a tip frame B = (joint jb_i, point offb_i),
 * both by the convention of the cost frames, ja_i != jb_i (on one joint the relative placement is constant); one joint may be an
 * ancestor of the other.  With p_a, p_b the points' world positions and R_a, R_b the world rotations of the two joints' frames
 * (world = R body), per instance b, t = 0 .. T and pair i a target g[b][t][i] in R^3 (B's point as seen from A, in A's joint
 * axes), a unit quaternion ref[b][t][i] = (x y z w) (R_ref: B's axes as seen from A's) and weights w[b][t][i] in R^6 (>= 0):
 *   r_pos = R_a^T (p_b - p_a) - g,      e_rot = log3(R_ref^T R_a^T R_b), |e_rot| <= pi,      r = (r_pos, e_rot)
 *   l(t, x, u) += 1/2 sum_i sum_a w[b][t][i][a] r_a^2      t < T
 *   lf(x_T)    += 1/2 sum_i sum_a w[b][T][i][a] r_a^2
 * to whatever the context optimises otherwise.  Derivatives in the tangent at x, by tangent column c, with s_c = +1 where c is on
 * path(jb) alone and s_c = -1 where c is on path(ja) alone, a_c the world axis and o_c the world origin of column c's joint:
 *   c on both paths or on neither:  nothing
 *   J_pos[:, c] = s_c R_a^T point_column(c, p_b)       point_column: a_c x (p_b - o_c) revolute, a_c prismatic -- about p_b on BOTH sides
 *   J_rot[:, c] = s_c Jlog3(e_rot) R_b^T a_c           revolute only: a prismatic column has no rotation part and it is left out
 *   lx[q rows] += J^T (w o r),   lxx[q, q] += J^T diag(w) J,   lfx / lfxx alike at T.
 * The A side uses p_b because d(R_a^T d) = R_a^T (dd - dw_a x d) with d = p_b - p_a: for a revolute column on A's side alone,
 * -a x (p_a - o) - a x (p_b - p_a) = -a x (p_b - o).  A relative placement does not change when a common ancestor joint moves: for
 * a column on both paths the two halves cancel identically, and such a column -- a free-flyer root's six always -- is left out, not
 * added as rounding residue.  The orientation convention is that of DDP_HIP_FLAG_FRAME_ORIENT_COST, applied to R_a^T R_b: a
 * perturbation acts as R_a^T R_b exp([R_b^T (dw_b - dw_a)]x), with the same Jlog3; ref and -ref are the same reference, and at
 * |e_rot| = pi the same words apply as there.  The term touches the symmetric differences of the live pairs' paths only: velocity
 * rows and columns, lu, luu, lux, every other q row and a free-flyer root's six rows are untouched.  lxx is Gauss-Newton (the term
 * sum_a w_a r_a d^2 r_a is dropped: exact where r = 0, positive semidefinite); pairs ascending, the three position axes, then the
 * three rotation axes, entry (i, j) formed in (min, max) order: symmetric bit for bit, no atomics.  A term of weight 0 is left out
 * (not multiplied by 0): a pair whose six weights are 0 is not walked, one whose three rotation weights are 0 reads no quaternion
 * and forms no log, one whose three position weights are 0 reads no target, and with nothing uploaded or every weight 0 a context
 * computes bit for bit what it computes without the flag.  The data travels through ddp_hip_relative_frame_* below; at create no
 * pairs are set.  Tree models only (the pendulum: DDP_HIP_E_UNSUPPORTED).  The flag combines with every other flag: the terms are
 * formed by kernels of their own, which add onto what the other terms' kernels leave (after the momentum's, before the
 * obstacles'). */
#define DDP_HIP_FLAG_RELATIVE_FRAME_COST 4096u
#define DDP_HIP_MAX_FRAME_PAIRS 4
/* Regularise the control about the torque that merely holds the robot up: on an arm or a humanoid under gravity 1/2 c |u|^2 (and
 * a tracking cost against a reference fixed in advance) penalises *holding the posture*, and every task term has to out-shout the
 * weight of the robot.  g(q) in R^nv is the generalised gravity torque, defined by the model's own forward dynamics: the control
 * for which aba(q, v = 0, u = g(q)) = 0 (no sign or frame convention enters).  Per instance b and t = 0 .. T-1 an offset
 * o[b][t] in R^m and weights w[b][t] in R^m (>= 0, finite), m = nv:
 *   r(q, u) = u - g(q) - o,      l(t, x, u) += 1/2 sum_j w_j r_j^2      t < T      (there is no control at T: no terminal term)
 * to whatever the context optimises otherwise.  With G = dg / d(delta q) (nv x nv, in the tangent at q) the term adds
 *   lu += w o r,   luu += diag(w),   lux[:, q columns] += -diag(w) G,   lx[q rows] += -G^T (w o r),   lxx[q, q] += G^T diag(w) G.
 * The first add-on term that writes lu / luu / lux.  With F = -gravity, a_k the world rotation axis of tangent k (a revolute
 * joint's axis; a free-flyer root's R_0 e_c for its three rotation tangents; none for a prismatic joint and the root's
 * translations), sub(k) the bodies that tangent k moves, and D_k = a_k x sum_sub m_b (p_b - o_k) (rotation), m_sub a_k
 * (translation):  g_k = F . D_k, and for tangent i with k on the path root .. i (k's joint an ancestor of i's, or the same joint)
 *   G_ik = a_k . (D_i x F)      (k rotational; 0 for a translation),      G_ki = the same for k's joint a strict ancestor of i's:
 * turning an ancestor turns the subtree's axis and lever alike, moving a descendant changes the ancestor's first moment by D.  On
 * a fixed base G is the Hessian of the potential energy and symmetric, bit for bit.  G_ik is formed only when i and k lie on one
 * root path, and of those only the entries whose ancestor side is rotational: everything else is identically zero and is left
 * out, not added as zeros -- a free-flyer root's three translation columns among them, while its three rotation columns are there
 * (turning the base turns gravity in the body).  The velocity rows and columns, lfx and lfxx are untouched.  lxx is Gauss-Newton
 * (sum_j w_j r_j d^2 g_j is dropped: exact where r = 0, positive semidefinite): rows ascending, entry (i, j) formed in (min, max)
 * order, symmetric bit for bit, no atomics; an entry that no live row reaches is not written.  A term of weight 0 is left out
 * (not multiplied by 0), a (b, t) whose weights are all 0 forms nothing, and with nothing uploaded or every weight 0 a context
 * computes bit for bit what it computes without the flag.  A free-flyer root's six rows carry no term (a weight there:
 * DDP_HIP_E_ARG, as for the pose rows of DDP_HIP_FLAG_STATE_LIMITS).  With DDP_HIP_FLAG_CONTROL_BOUNDS r is formed from the
 * control the rollout applied: the clamped one, as stored in U / U_NEW and the candidates' controls.  The data travels through
 * ddp_hip_control_grav_cost_* below; at create offsets and weights are 0.  Tree models only (the pendulum: DDP_HIP_E_UNSUPPORTED).
 * The flag stands alone and combines with every other flag: the terms are formed by kernels of their own, which add onto what the
 * other terms' kernels leave (after the relative frames', before the obstacles'). */
#define DDP_HIP_FLAG_CONTROL_GRAV_COST 8192u
/* Say "this axis looks at that point": "the head camera keeps the object in view while the arms work", "the gripper's approach
 * axis points at the grasp point before it closes", "the tool points at the seam from 30 cm away".  The orientation cost cannot
 * say it: its reference is a fixed rotation, while the direction to a target changes with the frame's own position.  Aiming fixes
 * two degrees of freedom about a direction that depends on q through the frame's own point, and leaves the roll about the axis
 * and -- without a range weight -- the distance free.  The flag stands alone: it needs no DDP_HIP_FLAG_FRAME_COST and has its own
 * frames.  Aim frames, shared by the batch, up to DDP_HIP_MAX_AIM_FRAMES: frame i is a joint j_i, a point off_i in the joint's
 * coordinates (the eye) and a unit axis a_i in the joint's axes; several frames may sit on one joint.  With p the point's world
 * position and n = R_j a the axis' world direction, per instance b, t = 0 .. T and frame i a target point g in R^3 (world), a
 * stand-off rho >= 0 and two weights w_aim, w_range (>= 0, finite):
 *   d = g - p,   l = |d|,   dh = d / l
 *   r_aim   = n - dh       (R^3; |r_aim| = 2 sin(theta / 2), theta the angle between the axis and the line of sight: zero only
 *                           when aligned and monotone up to theta = pi -- not n x dh, which is also zero looking away)
 *   r_range = l - rho
 *   l(t, x, u) += 1/2 sum_i (w_aim |r_aim|^2 + w_range r_range^2)      t < T
 *   lf(x_T)    += the same with row T
 * to whatever the context optimises otherwise.  Derivatives in the tangent at x, on the tangent columns c of path(j_i) only, with
 * point_column(c, p) as in the relative-frame text (a_c x (p - o_c) revolute, a_c prismatic; a free-flyer root's six columns by
 * the conventions of DDP_HIP_FLAG_FRAME_COST and DDP_HIP_FLAG_FRAME_ORIENT_COST: R_0 e_c and (R_0 e_c) x (p - o_0), the latter
 * three carrying the rotation axis R_0 e_c):
 *   J_aim[:, c] = (a_c x n, where c carries rotation)  +  (I - dh dh^T) point_column(c, p) / l
 *   J_range[c]  = -dh . point_column(c, p)
 *   lx[q rows] += J^T (w o r),   lxx[q, q] += J^T diag(w) J,   lfx / lfxx alike at T.
 * lxx is Gauss-Newton (sum_a w_a r_a d^2 r_a is dropped: exact where r = 0, positive semidefinite): frames ascending, the three
 * aim rows first, then the range row, entry (i, j) formed in (min, max) order: symmetric bit for bit, no atomics.  Velocity rows
 * and columns, lu, luu, lux and every q row off the live frames' paths are not written.  A term of weight 0 is left out (not
 * multiplied by 0): a frame with both weights 0 is not walked, with w_aim = 0 no aim row is formed, with w_range = 0 rho is not
 * read, and with nothing uploaded or every weight 0 a context computes bit for bit what it computes without the flag.  The
 * degenerate line of sight: where l <= 1e-12 the direction to the target does not exist, and frame i forms nothing at that
 * (b, t) -- no value and no derivative, of the aim rows and of the range row alike.  The data travels through ddp_hip_frame_aim_*
 * below; at create no frames are set.  Tree models only (the pendulum: DDP_HIP_E_UNSUPPORTED).  The flag combines with every other
 * flag: the terms are formed by kernels of their own, which add onto what the other terms' kernels leave (after the
 * control-gravity terms', before the obstacles'). */
#define DDP_HIP_FLAG_FRAME_AIM_COST 16384u
#define DDP_HIP_MAX_AIM_FRAMES 4
/* Say "stay balanced": "the centre of mass stays over the support polygon while the arms work", "the capture point stays over the
 * feet during the step".  A balance task is an inequality: DDP_HIP_FLAG_COM_COST pulls the CoM towards a point and fights every
 * reach, DDP_HIP_FLAG_MOMENTUM_COST regulates cdot; neither leaves the robot free inside a region.  The batch shares a plane count
 * (ddp_hip_balance_region_set_planes, up to DDP_HIP_MAX_REGION_PLANES); per instance b, t = 0 .. T and plane slot o five doubles
 * geom = (n, h, tau) -- a unit normal n in world axes, an offset h, a time constant tau >= 0 -- and a weight w >= 0.  With
 *   c(q)       the centre of mass of DDP_HIP_FLAG_COM_COST
 *   cdot(q, v) = Jc(q) v = l / M      (l the linear momentum of DDP_HIP_FLAG_MOMENTUM_COST, M the total mass)
 *   xi_o = c + tau_o cdot             (tau = 0: the CoM itself, no velocity quantity is read;  tau = 1 / omega_0 = sqrt(z_c / g):
 *                                      the capture point, where the robot must step to come to rest)
 *   d_o  = n_o . xi_o - h_o           (formed as (n_0 xi_0 + n_1 xi_1 + n_2 xi_2) - h; the free side is d >= 0, a safety margin
 *                                      goes into h)
 *   e_o  = !(d_o >= 0) ? d_o : 0      (a NaN d is active and its term NaN, the self-collision rule)
 *   l(t, x, u) += 1/2 sum_o w e_o^2      t < T
 *   lf(x_T)    += the same with row T
 * to whatever the context optimises otherwise.  tau lives per plane: each plane tests its own point, so one context holds "CoM
 * inside the polygon" (tau = 0) on some slots and "capture point inside the polygon" on others, and per-instance, per-t geometry
 * gives support polygons that change with the gait phase.  Derivatives in the tangent at x, over the planes with w != 0 and
 * e != 0 only, with dcq = d cdot / d(delta q) the linear rows of the momentum flag's dh/dq, each entry divided by M:
 *   z_o = [ (Jc + tau_o dcq)^T n_o  |  tau_o Jc^T n_o ]      (2 nv)
 *   lx += sum_o w e_o z_o,   lxx += sum_o w z_o z_o^T,   lfx / lfxx alike at T;   lu, luu, lux untouched.
 * Column i of z's q part is associated as (Jc[:, i] . n) + tau (dcq[:, i] . n) -- Jc . n first, then the product tau (dcq . n)
 * added -- and of its v part as tau (Jc[:, i] . n); the gradient entry is (w e) z[i] and the second-order entry
 * (z[min] w) z[max].  ddp_hip_model_capture_point forms the matrices entry by entry, Jc + tau dcq and tau Jc, with the same Jc and
 * dcq.  A free-flyer root's three linear columns of dcq are identically zero and are left out.  A plane with tau = 0 forms no
 * velocity quantity and touches neither the v rows nor the v columns; if no live plane (w != 0) of an (instance, t) has
 * tau != 0, cdot is not formed at all, and if no active one has, dcq is not.  lxx is Gauss-Newton (w e d^2 d is dropped:
 * positive semidefinite); planes ascending, entry (i, j) formed in (min, max) order: symmetric bit for bit, no atomics.  A plane
 * with w == 0 or e == 0 is left out (not multiplied by 0, not added as +0): with nothing uploaded, with every weight 0, and
 * with non-zero weights on planes that neither the trajectory nor any line-search candidate violates, a context computes bit for
 * bit what it computes without the flag.  The data travels through ddp_hip_balance_region_* below; at create no planes are set.
 * Tree models only (the pendulum: DDP_HIP_E_UNSUPPORTED); a total mass M <= 0 is DDP_HIP_E_ARG.  The flag stands alone and
 * combines with every other flag: the terms are formed by kernels of their own, which add onto what the other terms' kernels
 * leave (after the momentum's, before the relative frames'). */
#define DDP_HIP_FLAG_BALANCE_REGION_COST 32768u
#define DDP_HIP_MAX_REGION_PLANES 8
/* Say how hard the robot accelerates: "move smoothly", "arrive at rest and stay at rest", "do not jerk the torso", "follow this
 * acceleration profile".  A weight on v damps speed, not its change, and a weight on u penalises torque, a poor stand-in for
 * acceleration on a robot whose inertia varies by orders of magnitude between the wrist and the hip.  The first term whose
 * residual goes through the dynamics itself.  Per instance b, t = 0 .. T-1 and tangent row i = 0 .. nv-1 a target
 * a_ref[b][t][i] (finite) and a weight w[b][t][i] >= 0:
 *   a = aba(q_t, v_t, u_t),      r = a - a_ref[b][t],      l(t, x, u) += 1/2 sum_i w_i r_i^2      t < T
 * with a the model's own forward dynamics (what ddp_hip_model_aba returns), the six root rows of a free flyer included: the
 * rate of the body twist [linear; angular].  There is no control at T and no term at T.  Derivatives are taken in the tangent at
 * x: with Z = [Zq | Zv | Zu] = [da/d(delta q) | da/dv | M^-1] = [-M^-1 dtau/dq | -M^-1 dtau/dv | M^-1] (nv x 3 nv, dense: what
 * ddp_hip_model_aba_derivatives returns), over the rows with w_i != 0 alone,
 *   lx += [Zq Zv]^T (w o r),   lu += Zu^T (w o r),
 *   lxx += [Zq Zv]^T diag(w) [Zq Zv],   lux += Zu^T diag(w) [Zq Zv],   luu += Zu^T diag(w) Zu      (Gauss-Newton: sum_i w_i r_i
 * d^2 a_i is dropped; exact where r = 0, positive semidefinite).  The jacobians are the analytic ones whatever first_order_fd /
 * fd_mode the context uses for FX / FU: the term neither reads FX / FU nor depends on the order of the linearisation's stages.  lxx
 * and luu are formed on the lower triangle with the diagonal and mirrored: symmetric bit for bit; every sum runs over the rows in
 * ascending order, no atomics: reproducible run to run.  A row of weight 0 is left out (not multiplied by 0), a (b, t) whose
 * weights are all 0 forms nothing, and with nothing uploaded or every weight 0 no kernel of the term is launched: the context
 * computes bit for bit what it computes without the flag.  With DDP_HIP_FLAG_CONTROL_BOUNDS a is formed from the control the
 * rollout applied: the clamped one, as stored in U / U_NEW and the candidates' controls.  The values are formed by the forward
 * dynamics at (x_t, u_t), never by (v_{t+1} - v_t) / dt: ddp_hip_cost_seq_aug is also asked about trajectories that are no
 * rollouts of their controls.  The data travels through ddp_hip_joint_accel_cost_* below; at create targets and weights are 0.
 * Tree models only (the pendulum: DDP_HIP_E_UNSUPPORTED), fixed base or free-flyer root, with nv <= 38 (39 .. 64:
 * DDP_HIP_E_UNSUPPORTED at create -- the limit of ddp_hip_model_aba_derivatives and of the free-flyer first order: the
 * recursion's LDS record does not fit beside the jacobian at 64).  The flag stands alone and combines with every other flag: the
 * terms are formed by kernels of their own, which add onto what the other terms' kernels leave (after frame aiming's, before the
 * obstacles'). */
#define DDP_HIP_FLAG_JOINT_ACCEL_COST 65536u
#define DDP_HIP_MAX_JOINT_ACCEL_NV 38
/* Say "keep the limbs off the table edge, off the pole, off each other and off the floor" with the shape a limb has: a capsule, a
 * segment fixed in a joint swept by a radius.  Spheres (DDP_HIP_FLAG_OBSTACLE_COST, DDP_HIP_FLAG_SELF_COLLISION_COST) either leave
 * holes along a forearm or are so fat that the hands cannot come near each other.  The flag stands alone: it needs neither of the
 * two and has its own bodies.  Robot capsules, shared by the batch, up to DDP_HIP_MAX_CAPSULES: capsule k is the segment from
 * end0_k to end1_k, both points fixed in joint joint_k (the convention of the cost frames), with a radius r_k >= 0; end0 == end1
 * is a sphere.  Pairs, shared by the batch, up to DDP_HIP_MAX_CAPSULE_PAIRS: body A of pair i is robot capsule pair_a[i], body B
 * is what pair_kind[i] says.  Per instance b, t = 0 .. T and pair i eight doubles geom[b][t][i] and a weight w[b][t][i] >= 0; the
 * last geom entry is always the margin m (finite, may be negative):
 *   DDP_HIP_CAPSULE_VS_ROBOT      B is robot capsule pair_b[i] (another joint's);  geom = (., ., ., ., ., ., ., m), the first seven
 *                                 ignored but finite
 *   DDP_HIP_CAPSULE_VS_CAPSULE    B is a world capsule of the pair's own: geom = (b0(3), b1(3), rho >= 0, m), a world segment
 *                                 with a radius that moves with t and differs per instance
 *   DDP_HIP_CAPSULE_VS_HALFSPACE  B is a half-space: geom = (n(3), h, ., ., ., m), n unit by the obstacle half-spaces' rule
 *                                 (| |n| - 1 | <= 1e-10), the free side n . p >= h
 * With c_a, c_b the closest points of the two segments (below):
 *   D_i = |c_a - c_b|,   d_i = D_i - (r_a + r_b + m)   (a world capsule: r_b = rho),   u_i = (c_a - c_b) / D_i
 *   half-space:  d_i = min_end (n . p_end) - h - r_a - m,   c_a the end with the smaller n . p (end0 wins a tie),   u_i = n
 *   e_i = d_i < 0 ? d_i : 0          (a NaN distance is active and its term NaN)
 *   l(t, x, u) += 1/2 sum_i w[b][t][i] e_i^2      t < T
 *   lf(x_T)    += 1/2 sum_i w[b][T][i] e_i^2
 * to whatever the context optimises otherwise.  The closest points of the segments a0 + s d1 and b0 + t d2 are pinned: with
 * d1 = a1 - a0, d2 = b1 - b0, r = a0 - b0, A = d1 . d1, E = d2 . d2, F = d2 . r, C = d1 . r, Bv = d1 . d2, den = A E - Bv^2 and
 * clamp to [0, 1]:
 *   A == 0 and E == 0:  s = t = 0;       A == 0:  s = 0, t = clamp(F / E);       E == 0:  t = 0, s = clamp(-C / A);
 *   otherwise  s = den > 0 ? clamp((Bv F - C E) / den) : 0,  t = (Bv s + F) / E;  t < 0: t = 0, s = clamp(-C / A);
 *              t > 1: t = 1, s = clamp((Bv - C) / A);
 *   c_a = a0 + s d1,   c_b = b0 + t d2
 * (capsule_closest_params in csrc/capsule_cost.h, a routine that compiles for the host as well).  Derivatives in the tangent at x,
 * over the pairs with w != 0, e != 0 and (the two segment kinds) D_i != 0 only.  The closest points are frozen in their joints
 * with s and t held -- by the envelope theorem the parameters do not move d to first order -- so the pair is a sphere pair at
 * c_a and c_b, and with P_c the true point jacobian of DDP_HIP_FLAG_FRAME_COST at the point c:
 *   z_i[c] = + P_{c_a}[:, c] . u_i     c a tangent column of path(A) that is not on path(B)
 *   z_i[c] = - P_{c_b}[:, c] . u_i     c a tangent column of path(B) that is not on path(A)       (robot pairs alone)
 *            nothing                    c on both paths or on neither
 *   lx[q rows] += sum_i w e_i z_i,   lxx[q rows, q rows] += sum_i w z_i z_i^T,   lfx / lfxx alike at T.
 * A column on both paths of a robot pair -- a free-flyer root's six always -- is left out, not added as rounding residue, as for
 * DDP_HIP_FLAG_SELF_COLLISION_COST.  A world body has no path: all of path(A), a free-flyer root's six columns included, carries
 * + P . u.  Velocity rows and columns, lu, luu, lux and every q row outside the active pairs' column sets are untouched.  lxx is
 * Gauss-Newton (positive semidefinite); entry (r, c) is formed in (min, max) order with the pairs in ascending order: symmetric
 * bit for bit, no atomics.  A pair with D_i == 0 contributes its value and no derivative.  A pair with w == 0 or e == 0 is left
 * out (not multiplied by 0, not added as +0): with nothing uploaded, with every weight 0, and with non-zero weights on pairs that
 * neither the trajectory nor any line-search candidate brings within their margin, a context computes bit for bit what it
 * computes without the flag.  The data travels through ddp_hip_capsule_* below; at create no pairs are set and geometry and
 * weights are 0.  Tree models only (the pendulum: DDP_HIP_E_UNSUPPORTED).  The flag combines with every other flag: the terms are
 * formed by kernels of their own, which add onto what the other terms' kernels leave (last, after self-collision's).
 *
 * A fourth pair kind, DDP_HIP_CAPSULE_VS_GRID, reads the context's voxel grid (ddp_hip_obstacle_set_grid / _set_occupancy, which a
 * context created with this flag accepts as well): "keep the forearm out of the scanned shelf" without a string of spheres.
 *   DDP_HIP_CAPSULE_VS_GRID       B is the resident signed distance field: geom = (shift s(3), ., ., ., ., m), all eight finite,
 *                                 entries 3 .. 6 ignored; shift and margin mean what they mean for a DDP_HIP_OBSTACLE_GRID slot
 * The segment of body A is sampled at N_k + 1 material points, N_k fixed by the capsule and the resident grid, not by the state:
 *   L_k = sqrt(dx^2 + dy^2 + dz^2) of end1_k - end0_k in the joint's frame (host, double, each product rounded on its own)
 *   N_k = 0 if L_k == 0 (a sphere), else min(DDP_HIP_CAPSULE_GRID_MAX_INTERVALS, max(1, (int)ceil(L_k / cell)))
 * recomputed whenever the description is built for a launch: a new grid needs no second ddp_hip_capsule_set_pairs.  With a0, a1
 * the world ends of body A:
 *   sigma_j = (double)j / (double)N, j = 0 .. N (sigma_0 = 0 when N = 0),   c_j = a0 + sigma_j (a1 - a0),   x_j = c_j - s,
 *   (phi_j, g_j) = the trilinear lookup of DDP_HIP_OBSTACLE_GRID at x_j (obstacle_grid_lookup), +inf outside the grid
 *   j* = the smallest j attaining min_j phi_j; a NaN sample wins over everything, the first NaN taken
 *   every sample outside: d_i = +inf, the pair forms nothing and ddp_hip_capsule_clearance does not see it (the grid slot's rule)
 *   otherwise d_i = phi_j* - r_a - m,   c_a = c_b = c_j*,   u_i = g_j* (not normalised: it is dd / dp of this d)
 * (capsule_grid_intervals, capsule_grid_closest in csrc/capsule_cost.h, host and device).  e, the cost and the "left out" rules
 * are those above.  c_j* is frozen in A's joint, so the pair is a world pair: all of path(A) carries + P_{c_a}^T u, a free-flyer
 * root's six columns included; u == 0 exactly means value and no derivative; lxx is Gauss-Newton in (min, max) order, pairs
 * ascending.  There is no sub-sample refinement: the term is the minimum over N + 1 material points of the trilinear field, a
 * piecewise-smooth function whose exact derivative (where the argmin is unique) is the frozen-point one, so the line search's
 * values and the lineariser's derivatives agree without an envelope argument; a refinement would claim accuracy below a cell,
 * which the field does not have.  For a 1-Lipschitz field the continuous minimum along the segment is at least
 * min_j phi_j - L_k / (2 N_k): a caller who wants a bound puts that into the margin.  A capsule with L_k > 32 cell is sampled
 * coarser than the grid.  ddp_hip_capsule_set_pairs accepts the kind only while a grid is resident.
 *
 * A fifth pair kind, DDP_HIP_CAPSULE_VS_BOX, is the shape a workspace is made of: an oriented box (a table top, a shelf board, a
 * tote).  The shapes, up to DDP_HIP_MAX_CAPSULE_BOXES half-extent triples h > 0 along the box's own axes, are shared by the batch
 * (ddp_hip_capsule_set_boxes); pair_b[i] names the shape, several pairs may name one, and each pair has its own pose per
 * instance and t:
 *   DDP_HIP_CAPSULE_VS_BOX        B is box shape pair_b[i]: geom = (centre c(3), quaternion x y z w (4), m), all eight finite, the
 *                                 quaternion unit (| |q| - 1 | <= 1e-10) with world = R(q) box, R by the free-flyer's formula
 * The distance is exact, by a pinned search (capsule_box_closest in csrc/capsule_cost.h, host and device, every product rounded on
 * its own).  With a = R^T (a0 - c), b = R^T (a1 - c), dl = b - a, p(s) = a + s dl and the box's signed distance
 *   phi(p) = | max(|p| - h, 0) |_2 if that is > 0, else max_k (|p_k| - h_k)            (NaN where a coordinate is)
 * f(s) = phi(p(s)) is convex on [0, 1], and between two crossings of a face plane it is one smooth piece:
 *   1. breakpoints: 0, 1 and, for every axis k with dl_k != 0 and either sign, s = (+-h_k - a_k) / dl_k where 0 < s < 1 (+ before
 *      -), sorted ascending; equal values change nothing (an empty interval adds no new candidate)
 *   2. for consecutive breakpoints lo <= hi the pattern sg_k of p(1/2 (lo + hi)): +1 for p_k > h_k, -1 for p_k < -h_k, else 0
 *   3. candidates, in this order: lo; then, if some sg_k != 0 (outside), with A = sum dl_k^2 and C = sum dl_k (a_k - sg_k h_k) over
 *      those k in ascending k, s = -C / A if A > 0 and lo < s < hi; if all sg_k = 0 (inside), with the six lines
 *      l_i(s) = +-p_k(s) - h_k in the order i = (0+, 0-, 1+, 1-, 2+, 2-), for each pair i < j in lexicographic order whose slopes
 *      differ, s = (l_j(0) - l_i(0)) / (slope_i - slope_j) if lo < s < hi; last hi
 *   4. f is evaluated at every candidate in the order met and a candidate replaces the best only if strictly smaller: the smallest s,
 *      first met, wins a tie; a NaN wins over everything, the first one taken.  This gives s*, f*, c_a = a0 + s* (a1 - a0)
 *   5. u = R n with n in box axes: f* > 0: n = (p - clamp(p, -h, h)) / f*;  f* <= 0 and the winner a crossing of the lines i, j
 *      with slopes of opposite sign: n = (|slope_j| n_i + |slope_i| n_j) / (|slope_i| + |slope_j|), n_i the outward normal of
 *      face i -- the derivative of a min-max at its kink, not of unit length (as the grid kind's u is not);  otherwise n is the
 *      normal of the first line in the order above that attains max_i l_i(s*)
 *   d_i = f* - r_a - m,   c_b = c_a,   u_i = u
 * Convexity makes the search exact: the minimum of a convex f over [0, 1] is at an end or where a smooth piece is stationary, and
 * every such point is a candidate.  e, the cost, the Gauss-Newton block and the "left out" rules are those above.  The pair is a
 * world pair: with s* held (the envelope argument above) all of path(A) carries + P_{c_a}^T u, a free-flyer root's six columns
 * included.  f* == 0 exactly means value and no derivative (the D == 0 rule).  Inside the box the direction is exact where the
 * minimiser is unique; where the segment runs parallel to the nearest face the smallest s is taken and the direction is that
 * face's normal, one of the subgradients.  The penalty pushes a limb out through the nearest face, so a plate thinner than the
 * step the solver takes can be crossed unseen: inflate the margin of such a pair until box plus margin is thicker than that.
 * Geometry is validated on upload only; freshly reset geometry is all zeros, no unit quaternion, and a pair whose weight is 0 is
 * never evaluated.  Were a zero quaternion evaluated, R would be the identity by the formula: the box with its axes along the
 * world's, a defined value. */
#define DDP_HIP_FLAG_CAPSULE_COST 131072u
#define DDP_HIP_MAX_CAPSULES 16
#define DDP_HIP_MAX_CAPSULE_PAIRS 32
#define DDP_HIP_CAPSULE_VS_ROBOT 0      /* the other body is a robot capsule */
#define DDP_HIP_CAPSULE_VS_CAPSULE 1    /* ... a world capsule of the pair's own, per instance and t */
#define DDP_HIP_CAPSULE_VS_HALFSPACE 2  /* ... a half-space, per instance and t */
#define DDP_HIP_CAPSULE_VS_GRID 3       /* ... the context's voxel grid (ddp_hip_obstacle_set_grid / _set_occupancy) */
#define DDP_HIP_CAPSULE_GRID_MAX_INTERVALS 32
#define DDP_HIP_CAPSULE_VS_BOX 4        /* ... an oriented box of the pair's own pose, per instance and t (ddp_hip_capsule_set_boxes) */
#define DDP_HIP_MAX_CAPSULE_BOXES 8

int ddp_hip_abi_version(void);
const char* ddp_hip_strerror(int code);
int ddp_hip_device_count(void);

int ddp_hip_create(const ddp_hip_problem* prob, int device, uint32_t flags, ddp_hip_ctx** out);
int ddp_hip_destroy(ddp_hip_ctx* ctx);
/* the context's HIP stream (hipStream_t as void*) */
void* ddp_hip_stream(ddp_hip_ctx* ctx);
int ddp_hip_synchronize(ddp_hip_ctx* ctx);
/* Asynchronous mode (off by default).  On: the entry points that hand nothing back to the host -- ddp_hip_linearize[_stages],
 * ddp_hip_update_origin, ddp_hip_update_multipliers, ddp_hip_swap_traj -- enqueue their work on the context's stream and return
 * without waiting; the entry points that return values (ddp_hip_optimality, ddp_hip_backward, ddp_hip_forward, downloads ...)
 * synchronise as always, and everything is stream-ordered.  ddp_hip_solve runs its loop in this mode: per iteration the host
 * waits three times -- for the stopping test's two scalars, for the sweep's restart status, for the line search's accept state
 * -- instead of at every call.  Switching it off waits for the stream. */
int ddp_hip_set_async(ddp_hip_ctx* ctx, int on);

int64_t ddp_hip_batch(const ddp_hip_ctx* ctx);                       /* instances resident in the context */
int64_t ddp_hip_seq_size(const ddp_hip_ctx* ctx, int seq);           /* elements per instance */
double* ddp_hip_device_ptr(ddp_hip_ctx* ctx, int seq);               /* [batch][seq_size], device memory */
int ddp_hip_upload(ddp_hip_ctx* ctx, int seq, const double* host, int64_t first_instance, int64_t n_instances);
int ddp_hip_download(ddp_hip_ctx* ctx, int seq, double* host, int64_t first_instance, int64_t n_instances);
int ddp_hip_fill(ddp_hip_ctx* ctx, int seq, double value);
/* The frame cost of a context created with DDP_HIP_FLAG_FRAME_COST (else DDP_HIP_E_UNSUPPORTED), stream-ordered like
 * ddp_hip_upload.  set_frames: n_frames in 1 .. DDP_HIP_MAX_COST_FRAMES, joint[n_frames] inside the model, off[n_frames][3]
 * finite (else DDP_HIP_E_ARG); it may be called again: with the same count the targets and weights stay, with another they
 * are reset to 0.  upload / download: host arrays [n_instances][T+1][n_frames][3]; a NULL pointer leaves that side as it is;
 * an upload before frames are set, a negative or non-finite weight and a non-finite target are refused (DDP_HIP_E_ARG). */
int ddp_hip_frame_cost_set_frames(ddp_hip_ctx* ctx, int32_t n_frames, const int32_t* joint, const double* off);
int ddp_hip_frame_cost_upload(ddp_hip_ctx* ctx, const double* target, const double* weight, int64_t first_instance, int64_t n_instances);
int ddp_hip_frame_cost_download(ddp_hip_ctx* ctx, double* target, double* weight, int64_t first_instance, int64_t n_instances);
/* The orientation terms of the cost frames, of a context created with DDP_HIP_FLAG_FRAME_ORIENT_COST (else
 * DDP_HIP_E_UNSUPPORTED), stream-ordered like ddp_hip_frame_cost_upload.  Host arrays quat [n_instances][T+1][n_frames][4] and
 * weight [n_instances][T+1][n_frames][3] over the frames of ddp_hip_frame_cost_set_frames; a NULL pointer leaves that side as it
 * is.  An upload is refused as a whole (DDP_HIP_E_ARG, nothing written) before frames are set, for a bad instance range, a
 * non-finite value, a quaternion whose norm differs from 1 by more than 1e-10 and a negative weight.
 * ddp_hip_frame_cost_set_frames with another frame count resets the orientation data to identity quaternions and weights 0;
 * with the same count it stays. */
int ddp_hip_frame_orient_upload(ddp_hip_ctx* ctx, const double* quat, const double* weight, int64_t first_instance, int64_t n_instances);
int ddp_hip_frame_orient_download(ddp_hip_ctx* ctx, double* quat, double* weight, int64_t first_instance, int64_t n_instances);
/* The state limits of a context created with DDP_HIP_FLAG_STATE_LIMITS (else DDP_HIP_E_UNSUPPORTED), stream-ordered like
 * ddp_hip_frame_cost_upload.  Host arrays [n_instances][T+1][n]; a NULL pointer leaves that side as it is; a bad instance range
 * is DDP_HIP_E_ARG.  An upload is refused as a whole (DDP_HIP_E_ARG, nothing written) for the values listed at the flag;
 * lo <= hi is checked inside the upload, a side that arrives alone against the resident other side. */
int ddp_hip_state_limits_upload(ddp_hip_ctx* ctx, const double* lo, const double* hi, const double* weight, int64_t first_instance,
                                int64_t n_instances);
int ddp_hip_state_limits_download(ddp_hip_ctx* ctx, double* lo, double* hi, double* weight, int64_t first_instance, int64_t n_instances);
/* The CoM targets and weights of a context created with DDP_HIP_FLAG_COM_COST (else DDP_HIP_E_UNSUPPORTED), stream-ordered like
 * ddp_hip_frame_cost_upload.  Host arrays [n_instances][T+1][3]; a NULL pointer leaves that side as it is.  An upload is refused
 * as a whole (DDP_HIP_E_ARG, nothing written) for a bad instance range, a non-finite target and a negative or non-finite
 * weight. */
int ddp_hip_com_cost_upload(ddp_hip_ctx* ctx, const double* target, const double* weight, int64_t first_instance, int64_t n_instances);
int ddp_hip_com_cost_download(ddp_hip_ctx* ctx, double* target, double* weight, int64_t first_instance, int64_t n_instances);
/* The velocity targets and weights of the cost frames in a context created with DDP_HIP_FLAG_FRAME_VEL_COST (else
 * DDP_HIP_E_UNSUPPORTED), stream-ordered like ddp_hip_frame_orient_upload.  Host arrays [n_instances][T+1][n_frames][6] (linear
 * part, then angular part); a NULL pointer leaves that side as it is.  An upload is refused as a whole (DDP_HIP_E_ARG, nothing
 * written) before frames are set, for a bad instance range, a non-finite target and a negative or non-finite weight.
 * ddp_hip_frame_cost_set_frames with another frame count resets this data to 0 as well; with the same count it stays. */
int ddp_hip_frame_vel_upload(ddp_hip_ctx* ctx, const double* target, const double* weight, int64_t first_instance, int64_t n_instances);
int ddp_hip_frame_vel_download(ddp_hip_ctx* ctx, double* target, double* weight, int64_t first_instance, int64_t n_instances);
/* The collision points and the obstacle slots of a context created with DDP_HIP_FLAG_OBSTACLE_COST (else DDP_HIP_E_UNSUPPORTED),
 * shared by the batch: joint[n_points], off[n_points][3], radius[n_points], kind[n_obstacles].  DDP_HIP_E_ARG for counts outside
 * 1 .. DDP_HIP_MAX_COLLISION_POINTS or 1 .. DDP_HIP_MAX_OBSTACLES, a joint outside the model, a non-finite offset, a negative or
 * non-finite radius, an unknown kind, and DDP_HIP_OBSTACLE_GRID while no grid is resident.  It may be called again: with the
 * same two counts and the same kinds the per-instance data stays (points may move, radii may change), otherwise geometry and
 * weights are reset to 0. */
int ddp_hip_obstacle_set_points(ddp_hip_ctx* ctx, int32_t n_points, const int32_t* joint, const double* off, const double* radius,
                                int32_t n_obstacles, const int32_t* kind);
/* The obstacles' geometry and weights, stream-ordered like ddp_hip_com_cost_upload.  Host arrays [n_instances][T+1][n_obstacles][4]
 * and [n_instances][T+1][n_obstacles]; a NULL pointer leaves that side as it is.  An upload is refused as a whole (DDP_HIP_E_ARG,
 * nothing written) before ddp_hip_obstacle_set_points, for a bad instance range, a non-finite value, a negative weight, a negative
 * sphere radius and a half-space normal n with | |n| - 1 | > 1e-10 (a grid slot's shift and margin: finite).  A geom that
 * arrives alone is checked against the slot kinds; weights that arrive alone need no geometry check. */
int ddp_hip_obstacle_upload(ddp_hip_ctx* ctx, const double* geom, const double* weight, int64_t first_instance, int64_t n_instances);
int ddp_hip_obstacle_download(ddp_hip_ctx* ctx, double* geom, double* weight, int64_t first_instance, int64_t n_instances);
/* "Did the result collide, where, by how much": out[batch][T+1] (host) = min over the collision points and over the slots with
 * w != 0 of d_ko along X (which = 0) or X_NEW (which = 1), +inf where no slot is live.  From the first
 * ddp_hip_obstacle_set_points on (before: DDP_HIP_E_ARG), live weights or not. */
int ddp_hip_obstacle_clearance(ddp_hip_ctx* ctx, int which, double* out);
/* The grid of the slots of kind DDP_HIP_OBSTACLE_GRID and of the capsule pairs of kind DDP_HIP_CAPSULE_VS_GRID, in a context
 * created with DDP_HIP_FLAG_OBSTACLE_COST or DDP_HIP_FLAG_CAPSULE_COST (with neither: DDP_HIP_E_UNSUPPORTED).  set_grid takes a field made elsewhere, phi[nx][ny][nz] (host, C order).  set_occupancy takes voxels in
 * the same index order, occ != 0 meaning occupied, and builds the field on the device by an exact Euclidean distance transform:
 * with D_occ(v) (D_free(v)) the least squared index distance from voxel v to an occupied (a free) voxel, nx^2 + ny^2 + nz^2 where
 * there is none,
 *   phi(v) = +cell (sqrt(D_occ(v)) - 0.5) for a free v,   phi(v) = -cell (sqrt(D_free(v)) - 0.5) for an occupied v:
 * the surface lies halfway between a free voxel's centre and its occupied neighbour's, and an all-free or all-occupied grid stays
 * finite.  The squared distances are exact integers, so phi does not depend on how the transform is scheduled.  Either call may be
 * repeated at any time between other calls, with other dims as well; the new grid replaces the old one for everything that runs
 * afterwards (slots, their geometry and weights stay).  Both run on the context's stream and wait for it before they return.
 * DDP_HIP_E_ARG for a NULL pointer, a dim outside 2 .. DDP_HIP_MAX_GRID_DIM, a non-finite origin, a cell that is not finite and
 * positive and, for set_grid, a non-finite value of phi.  A refused call, and one that cannot allocate (DDP_HIP_E_HIP), leaves
 * the old grid in force. */
int ddp_hip_obstacle_set_grid(ddp_hip_ctx* ctx, const int32_t dims[3], const double origin[3], double cell, const double* phi);
int ddp_hip_obstacle_set_occupancy(ddp_hip_ctx* ctx, const int32_t dims[3], const double origin[3], double cell, const uint8_t* occ);
/* The resident grid: dims, origin, cell and, unless phi is NULL (shape only), the field.  Before any grid: DDP_HIP_E_ARG. */
int ddp_hip_obstacle_grid_download(ddp_hip_ctx* ctx, int32_t dims[3], double origin[3], double* cell, double* phi);
/* phi and (unless grad_out is NULL) grad phi of the resident grid at n world points (host, points[n][3]), by the device function
 * the cost kernels use: +inf and a zero gradient outside the grid, NaN for a point with a NaN coordinate.  n >= 0.  Before any
 * grid: DDP_HIP_E_ARG.  A diagnostic call, not one for a control loop: it allocates a device buffer of 7 n doubles and frees it
 * before it returns (unlike the transform's temporaries, which the context keeps), and waits for the context's stream. */
int ddp_hip_obstacle_grid_query(ddp_hip_ctx* ctx, int64_t n, const double* points, double* phi_out, double* grad_out);
/* "What does the capsule cost see along this limb": the rule of DDP_HIP_CAPSULE_VS_GRID on n world segments (host, seg[n][6] =
 * (a0, a1), the shift already taken off) with n_intervals[n] intervals each, 0 .. DDP_HIP_CAPSULE_GRID_MAX_INTERVALS, by the device
 * routine the cost kernels use (capsule_grid_closest), one segment per lane group.  phi_out[n] = min_j phi_j (+inf: every sample
 * outside; NaN: a NaN sample), j_out[n] = j* (-1: every sample outside), point_out[n][3] = c_j*, grad_out[n][3] = g_j* (where
 * every sample is outside: the point a0 and a zero gradient); the last three may be NULL.  Refusals are those of
 * ddp_hip_obstacle_grid_query, and DDP_HIP_E_ARG for an interval count out of range.  A diagnostic call like that one. */
int ddp_hip_obstacle_grid_segment_query(ddp_hip_ctx* ctx, int64_t n, const double* seg, const int32_t* n_intervals, double* phi_out,
                                        int32_t* j_out, double* point_out, double* grad_out);
/* The spheres and the pairs of a context created with DDP_HIP_FLAG_SELF_COLLISION_COST (else DDP_HIP_E_UNSUPPORTED), shared by the
 * batch: joint[n_points], off[n_points][3], radius[n_points], pair_a[n_pairs], pair_b[n_pairs].  DDP_HIP_E_ARG for n_points
 * outside 2 .. DDP_HIP_MAX_COLLISION_POINTS, n_pairs outside 1 .. DDP_HIP_MAX_COLLISION_PAIRS, a joint outside the model, a
 * non-finite offset, a negative or non-finite radius, a sphere index outside the points, a == b, and both spheres of a pair on
 * the same joint (their distance is constant).  Duplicate pairs are allowed.  It may be called again: with the same pair count
 * and the same (a, b) list the per-instance data stays (points may move, radii may change), otherwise margins and weights are
 * reset to 0. */
int ddp_hip_self_collision_set_pairs(ddp_hip_ctx* ctx, int32_t n_points, const int32_t* joint, const double* off, const double* radius,
                                     int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_b);
/* The pairs' margins and weights, stream-ordered like ddp_hip_obstacle_upload.  Host arrays [n_instances][T+1][n_pairs] each; a
 * NULL pointer leaves that side as it is.  An upload is refused as a whole (DDP_HIP_E_ARG, nothing written) before
 * ddp_hip_self_collision_set_pairs, for a bad instance range, a non-finite margin and a negative or non-finite weight. */
int ddp_hip_self_collision_upload(ddp_hip_ctx* ctx, const double* margin, const double* weight, int64_t first_instance, int64_t n_instances);
int ddp_hip_self_collision_download(ddp_hip_ctx* ctx, double* margin, double* weight, int64_t first_instance, int64_t n_instances);
/* "Did the result fold into itself, where, by how much": out[batch][T+1] (host) = min over the pairs with w != 0 of d_i along X
 * (which = 0) or X_NEW (which = 1), +inf where no pair is live, NaN where a distance is.  From the first
 * ddp_hip_self_collision_set_pairs on (before: DDP_HIP_E_ARG), live weights or not. */
int ddp_hip_self_collision_clearance(ddp_hip_ctx* ctx, int which, double* out);
/* The momentum targets and weights of a context created with DDP_HIP_FLAG_MOMENTUM_COST (else DDP_HIP_E_UNSUPPORTED),
 * stream-ordered like ddp_hip_com_cost_upload.  Host arrays [n_instances][T+1][6] (linear part, then angular part); a NULL pointer
 * leaves that side as it is.  An upload is refused as a whole (DDP_HIP_E_ARG, nothing written) for a bad instance range, a
 * non-finite target and a negative or non-finite weight. */
int ddp_hip_momentum_cost_upload(ddp_hip_ctx* ctx, const double* target, const double* weight, int64_t first_instance, int64_t n_instances);
int ddp_hip_momentum_cost_download(ddp_hip_ctx* ctx, double* target, double* weight, int64_t first_instance, int64_t n_instances);
/* The frame pairs of a context created with DDP_HIP_FLAG_RELATIVE_FRAME_COST (else DDP_HIP_E_UNSUPPORTED), shared by the batch:
 * joint_a[n_pairs], off_a[n_pairs][3], joint_b[n_pairs], off_b[n_pairs][3].  DDP_HIP_E_ARG for n_pairs outside
 * 1 .. DDP_HIP_MAX_FRAME_PAIRS, a joint outside the model, joint_a[i] == joint_b[i] and a non-finite offset.  It may be called
 * again: with the same count and the same joints the per-instance data stays (the points may move), otherwise targets and weights
 * are reset to 0 and the references to identity quaternions. */
int ddp_hip_relative_frame_set_pairs(ddp_hip_ctx* ctx, int32_t n_pairs, const int32_t* joint_a, const double* off_a, const int32_t* joint_b,
                                     const double* off_b);
/* The pairs' targets, references and weights, stream-ordered like ddp_hip_frame_orient_upload.  Host arrays
 * [n_instances][T+1][n_pairs][3], [..][4] and [..][6] (position weights, then rotation weights); a NULL pointer leaves that side
 * as it is.  An upload is refused as a whole (DDP_HIP_E_ARG, nothing written) before ddp_hip_relative_frame_set_pairs, for a bad
 * instance range, a non-finite value, a quaternion whose norm differs from 1 by more than 1e-10 and a negative weight. */
int ddp_hip_relative_frame_upload(ddp_hip_ctx* ctx, const double* target, const double* quat, const double* weight, int64_t first_instance,
                                  int64_t n_instances);
int ddp_hip_relative_frame_download(ddp_hip_ctx* ctx, double* target, double* quat, double* weight, int64_t first_instance, int64_t n_instances);
/* "Did the grasp hold": out[batch][T+1][n_pairs][6] (host) = the unweighted residual r = (r_pos, e_rot) of every pair along X
 * (which = 0) or X_NEW (which = 1), against the resident targets and references.  From the first
 * ddp_hip_relative_frame_set_pairs on (before: DDP_HIP_E_ARG), live weights or not. */
int ddp_hip_relative_frame_error(ddp_hip_ctx* ctx, int which, double* out);
/* The control-gravity terms of a context created with DDP_HIP_FLAG_CONTROL_GRAV_COST (else DDP_HIP_E_UNSUPPORTED), stream-ordered
 * like ddp_hip_momentum_cost_upload.  Host arrays [n_instances][T][m]: offsets and weights, one per control row and t < T; a NULL
 * pointer leaves that side as it is.  An upload is refused as a whole (DDP_HIP_E_ARG, nothing written) for a bad instance range, a
 * non-finite offset, a negative or non-finite weight and a non-zero weight on one of a free-flyer root's six rows. */
int ddp_hip_control_grav_cost_upload(ddp_hip_ctx* ctx, const double* offset, const double* weight, int64_t first_instance, int64_t n_instances);
int ddp_hip_control_grav_cost_download(ddp_hip_ctx* ctx, double* offset, double* weight, int64_t first_instance, int64_t n_instances);
/* The aim frames of a context created with DDP_HIP_FLAG_FRAME_AIM_COST (else DDP_HIP_E_UNSUPPORTED), shared by the batch:
 * joint[n_frames], off[n_frames][3], axis[n_frames][3].  DDP_HIP_E_ARG for n_frames outside 0 .. DDP_HIP_MAX_AIM_FRAMES, a joint
 * outside the model, a non-finite offset and an axis whose length differs from 1 by more than 1e-10 (the quaternions' rule).  It
 * may be called again: with the same count and the same joints the per-instance data stays (the points and the axes may move),
 * otherwise targets, stand-offs and weights are reset to 0.  n_frames = 0 takes the frames away. */
int ddp_hip_frame_aim_set_frames(ddp_hip_ctx* ctx, int32_t n_frames, const int32_t* joint, const double* off, const double* axis);
/* The frames' targets and weights, stream-ordered like ddp_hip_frame_cost_upload.  Host arrays [n_instances][T+1][n_frames][4] =
 * (g, rho) and [n_instances][T+1][n_frames][2] = (w_aim, w_range); a NULL pointer leaves that side as it is.  An upload is refused
 * as a whole (DDP_HIP_E_ARG, nothing written) before ddp_hip_frame_aim_set_frames, for a bad instance range, a non-finite target
 * or stand-off, a negative stand-off and a negative or non-finite weight. */
int ddp_hip_frame_aim_upload(ddp_hip_ctx* ctx, const double* target, const double* weight, int64_t first_instance, int64_t n_instances);
int ddp_hip_frame_aim_download(ddp_hip_ctx* ctx, double* target, double* weight, int64_t first_instance, int64_t n_instances);
/* "Did it stay in view, from how far": out[batch][T+1][n_frames][2] (host) = (theta, l) of every frame along X (which = 0) or
 * X_NEW (which = 1), against the resident targets: theta in radians, the angle between the axis and the line of sight, formed as
 * atan2(|n x dh|, n . dh), and l the distance from the eye to the target (theta = 0 where l <= 1e-12).  From the first
 * ddp_hip_frame_aim_set_frames with a frame on (before: DDP_HIP_E_ARG), live weights or not. */
int ddp_hip_frame_aim_error(ddp_hip_ctx* ctx, int which, double* out);
/* The plane count of a context created with DDP_HIP_FLAG_BALANCE_REGION_COST (else DDP_HIP_E_UNSUPPORTED), shared by the batch:
 * n_planes in 0 .. DDP_HIP_MAX_REGION_PLANES (else DDP_HIP_E_ARG).  It may be called again: with the same count the per-instance
 * data stays, another count resets geometry and weights to 0.  n_planes = 0 takes the planes away. */
int ddp_hip_balance_region_set_planes(ddp_hip_ctx* ctx, int32_t n_planes);
/* The planes' geometry and weights, stream-ordered like ddp_hip_obstacle_upload.  Host arrays [n_instances][T+1][n_planes][5] =
 * (n, h, tau) and [n_instances][T+1][n_planes]; a NULL pointer leaves that side as it is.  An upload is refused as a whole
 * (DDP_HIP_E_ARG, nothing written) before ddp_hip_balance_region_set_planes with a count >= 1, for a bad instance range, a
 * non-finite value, a normal n with | |n| - 1 | > 1e-10 (the obstacle half-spaces' rule), tau < 0 and a negative weight. */
int ddp_hip_balance_region_upload(ddp_hip_ctx* ctx, const double* geom, const double* weight, int64_t first_instance, int64_t n_instances);
int ddp_hip_balance_region_download(ddp_hip_ctx* ctx, double* geom, double* weight, int64_t first_instance, int64_t n_instances);
/* "Did it stay balanced, by how much": out[batch][T+1] (host) = min over the planes with w != 0 of d_o along X (which = 0) or
 * X_NEW (which = 1), +inf where no plane is live, NaN where a d is.  From the first ddp_hip_balance_region_set_planes with a
 * plane on (before: DDP_HIP_E_ARG), live weights or not. */
int ddp_hip_balance_region_margin(ddp_hip_ctx* ctx, int which, double* out);
/* The joint-acceleration terms of a context created with DDP_HIP_FLAG_JOINT_ACCEL_COST (else DDP_HIP_E_UNSUPPORTED), stream-ordered
 * like ddp_hip_momentum_cost_upload.  Host arrays [n_instances][T+1][nv]: targets and weights, one per tangent row of v; row T
 * belongs to no term (there is no control at T), keeps what it held at create and is read by no kernel.  A NULL pointer leaves
 * that side as it is.  An upload is refused as a whole (DDP_HIP_E_ARG, nothing written) for a bad instance range, a non-finite
 * target, a negative or non-finite weight and a non-zero weight in row T.  A free-flyer root's six rows carry terms like any other. */
int ddp_hip_joint_accel_cost_upload(ddp_hip_ctx* ctx, const double* target, const double* weight, int64_t first_instance, int64_t n_instances);
int ddp_hip_joint_accel_cost_download(ddp_hip_ctx* ctx, double* target, double* weight, int64_t first_instance, int64_t n_instances);
/* "How hard did it accelerate": out[batch][T][nv] = aba(x_t, u_t) along X / U (which = 0) or X_NEW / U_NEW (which = 1), formed by
 * the cost kernel's forward dynamics in one launch, live weights or not. */
int ddp_hip_joint_accel(ddp_hip_ctx* ctx, int which, double* out);
/* The robot capsules and the pairs of a context created with DDP_HIP_FLAG_CAPSULE_COST (else DDP_HIP_E_UNSUPPORTED), shared by the
 * batch: joint[n_capsules], end0[n_capsules][3], end1[n_capsules][3], radius[n_capsules], pair_a[n_pairs], pair_kind[n_pairs],
 * pair_b[n_pairs] (read for DDP_HIP_CAPSULE_VS_ROBOT pairs alone).  DDP_HIP_E_ARG for n_capsules outside
 * 1 .. DDP_HIP_MAX_CAPSULES, n_pairs outside 1 .. DDP_HIP_MAX_CAPSULE_PAIRS, a joint outside the model, a non-finite end, a
 * negative or non-finite radius, a capsule index outside the capsules, an unknown kind, DDP_HIP_CAPSULE_VS_GRID while no grid is
 * resident, and a robot pair with a == b or with both capsules on the same joint (their distance is constant).  Duplicate pairs are allowed.  It may be called again: with the same
 * two counts and the same kinds the per-instance data stays (capsules may move, radii may change, a pair may name other capsules),
 * otherwise geometry and weights are reset to 0.  A pair of kind DDP_HIP_CAPSULE_VS_BOX reads pair_b[i] as the index of a box shape,
 * 0 .. n_boxes - 1 of ddp_hip_capsule_set_boxes (outside, or with no boxes set: DDP_HIP_E_ARG). */
int ddp_hip_capsule_set_pairs(ddp_hip_ctx* ctx, int32_t n_capsules, const int32_t* joint, const double* end0, const double* end1,
                              const double* radius, int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_kind, const int32_t* pair_b);
/* The box shapes of the pairs of kind DDP_HIP_CAPSULE_VS_BOX, shared by the batch, in a context created with DDP_HIP_FLAG_CAPSULE_COST
 * (else DDP_HIP_E_UNSUPPORTED): half[n_boxes][3] (host), the half extents along the box's own axes, each finite and > 0.
 * DDP_HIP_E_ARG, with nothing changed, for n_boxes outside 0 .. DDP_HIP_MAX_CAPSULE_BOXES, a bad extent, and a call that would leave
 * a box pair already set without its shape (pair_b >= n_boxes).  It may be called again: extents may change while the pairs stand,
 * and the next launch reads the new ones. */
int ddp_hip_capsule_set_boxes(ddp_hip_ctx* ctx, int32_t n_boxes, const double* half);
/* The pairs' geometry and weights, stream-ordered like ddp_hip_obstacle_upload.  Host arrays [n_instances][T+1][n_pairs][8] and
 * [n_instances][T+1][n_pairs]; a NULL pointer leaves that side as it is.  An upload is refused as a whole (DDP_HIP_E_ARG, nothing
 * written) before ddp_hip_capsule_set_pairs, for a bad instance range, a non-finite geom entry (the ignored ones included), a
 * world capsule's rho < 0, a half-space normal n with | |n| - 1 | > 1e-10, a box pair's quaternion q with | |q| - 1 | > 1e-10 and a negative or non-finite weight.  A geom that
 * arrives alone is checked against the pair kinds; weights that arrive alone need no geometry check. */
int ddp_hip_capsule_upload(ddp_hip_ctx* ctx, const double* geom, const double* weight, int64_t first_instance, int64_t n_instances);
int ddp_hip_capsule_download(ddp_hip_ctx* ctx, double* geom, double* weight, int64_t first_instance, int64_t n_instances);
/* "Did a limb touch, where, by how much": out[batch][T+1] (host) = min over the pairs with w != 0 of d_i along X (which = 0) or
 * X_NEW (which = 1), +inf where no pair is live, NaN where a distance is.  From the first ddp_hip_capsule_set_pairs on (before:
 * DDP_HIP_E_ARG), live weights or not. */
int ddp_hip_capsule_clearance(ddp_hip_ctx* ctx, int which, double* out);

/* make_trajectory (ddp.hpp:392-415): X[0] and U given -> X[1..T] */
int ddp_hip_rollout(ddp_hip_ctx* ctx);
/* compute_derivatives (problem.hpp:956-998) along (X, U) -> all derivative sequences */
int ddp_hip_linearize(ddp_hip_ctx* ctx);
/* the same, stage by stage (cost terms :982-987 | first order f :463-503 | second order f :50-341 |
 * constraint chain :527-870); the later stages read what the earlier ones left resident */
#define DDP_HIP_LIN_COST 1u
#define DDP_HIP_LIN_FIRST 2u
#define DDP_HIP_LIN_SECOND 4u
#define DDP_HIP_LIN_EQ 8u
int ddp_hip_linearize_stages(ddp_hip_ctx* ctx, uint32_t stages);

/* backward_pass<primal_dual_affine_multipliers> (ddp_bwd.ipp:9-155).
 * reg_io / mu_io: host arrays [batch], in-out (ddp_bwd.ipp:106-110,154); restarts_out: host [batch] or NULL.
 * max_restarts bounds the reference's unbounded while(!success).
 * DDP_HIP_E_UNSUPPORTED, ahead of any launch, where the sweep's kernels need more LDS than a workgroup has: 64 joints, or 58
 * and more with DDP_HIP_FLAG_CONTROL_BOUNDS (ddp_hip_solve answers the same way). */
int ddp_hip_backward(ddp_hip_ctx* ctx, double* reg_io, double* mu_io, int64_t* restarts_out, int64_t max_restarts);

/* forward_pass (ddp_fwd.ipp:9-67) with the step halving evaluated n_alpha candidates at a time:
 * candidates 2^0 .. 2^-(n_alpha-1) roll out concurrently, the LARGEST accepted one is kept (the same
 * decision sequential halving makes); if none is accepted the next n_alpha candidates follow, until
 * step < 1e-10.  mu: host [batch]; step_out: host [batch]; dcost_out: host [batch] or NULL
 * (sum_t(cost_new - cost_old) of the returned step).  X_NEW[0] must hold x_0 (ddp.hpp:752).
 * n_alpha == 0: do_linesearch == false (ddp_fwd.ipp:61-63) -- the full step is rolled out once and taken whatever the
 * cost does (step_out = 1, X_NEW / U_NEW = that rollout). */
int ddp_hip_forward(ddp_hip_ctx* ctx, const double* mu, int32_t n_alpha, double* step_out, double* dcost_out);

/* cost_seq_aug (ddp.hpp:699-735) of (X,U) [which=0] or (X_NEW,U_NEW) [which=1] into COSTS_OLD / COSTS_NEW */
int ddp_hip_cost_seq_aug(ddp_hip_ctx* ctx, int which, const double* mu);
/* swap(traj, new_traj) (ddp.hpp:826) */
int ddp_hip_swap_traj(ddp_hip_ctx* ctx);

/* The receding-horizon advance (model-predictive control: solve, apply the first control, move the window on by `shift` steps, take
 * the measured state, solve again), on the resident data: nothing is downloaded.  s = shift, 1 <= s <= T; "old" is the value before
 * the call; x0: host [batch][nx], the measured states, or NULL (X[0] becomes the old X[s]).  The call applies to every instance,
 * whatever ddp_hip_set_active says, and leaves the active mask as it is.
 *   arrays with T rows (U, COST_UREF, COST_WU, CTRL_LO, CTRL_HI, every side of the control-gravity block):
 *     row[t] = old[t + s] for t < T - s,  row[t] = old[T - 1] for t >= T - s: a tail row holds the last stage row.
 *   arrays with T + 1 rows whose last row is the terminal cost (COST_XREF, COST_WX, every side of every other add-on cost block,
 *   as it is laid out now): rows 0 .. T-1 by the rule above; row T is not touched -- the terminal cost belongs to the end of the
 *   window, not to an absolute time (the joint accelerations' weights keep their zero row T this way).
 *   X:       X[t] = old[t + s] for t <= T - s,  old[T] for t > T - s (finite rows under the tail's zero gains), then X[0] = x0.
 *   FB_JAC:  FB_JAC[t] = old[t + s] for t < T - s, exact zeros in the tail.    FB_VAL: 0 everywhere (the step has been taken).
 * What new information enters the window at its far end (targets, obstacles, bounds of the new steps) is the caller's to upload,
 * with the uploads above, after the call.  Then, by mode:
 *   NO_ROLL      nothing more.
 *   OPEN_LOOP    X[1..T] = the rollout of the shifted U from X[0]: bit for bit what ddp_hip_rollout gives (U as given, no clamp).
 *   CLOSED_LOOP  u_t = clamp(U[t] + K[t] (x_t (-) X[t])), x_{t+1} = f(x_t, u_t) with the shifted U, K = FB_JAC and X: bit for bit
 *                what ddp_hip_forward(n_alpha = 0) followed by ddp_hip_swap_traj gives with every instance active, X_NEW[0] = X[0]
 *                and FB_VAL = 0 (the clamp with DDP_HIP_FLAG_CONTROL_BOUNDS alone); COSTS_OLD is written as that call writes it.
 *                x_0 is X[0] itself, so u_0 = clamp(U[0]) and the gains act from t = 1 on, on what x_1 = f(x0, u_0) differs by.
 * On return FB_ORIGIN[t] = MULT_ORIGIN[t] = X[t] for t < T and X_NEW / U_NEW are clones of X / U: the context is the input
 * ddp_hip_solve documents.  Not touched, and stale exactly as after an upload of X: BOX_STAT, COSTS_OLD / COSTS_NEW (but for
 * CLOSED_LOOP's), the candidates' arrays, every derivative sequence and what the context knows about its tensors.  Which add-on
 * terms are live does not change (rows are permuted and repeated, never created), nor whether lo <= hi has been checked (a
 * CLOSED_LOOP call checks it first, as ddp_hip_forward does).
 * Refused before anything is written: ctx NULL, s < 1, s > T, an unknown mode, a non-finite entry of x0 and, on a free-flyer model,
 * a root quaternion of x0 with | |quat| - 1 | > 1e-10 (DDP_HIP_E_ARG); a context with constraint rows (DDP_HIP_E_UNSUPPORTED: ne[t]
 * varies with t and the batch shares eq_target, so the multipliers have no well-defined shift).  Everything runs on the context's
 * stream; NO_ROLL honours ddp_hip_set_async, the rolling modes wait where ddp_hip_rollout / ddp_hip_forward do. */
#define DDP_HIP_ADVANCE_NO_ROLL     0   /* shift and refill only */
#define DDP_HIP_ADVANCE_OPEN_LOOP   1   /* ... then X[1..T] = rollout of the shifted U from X[0] (as ddp_hip_rollout: U as given) */
#define DDP_HIP_ADVANCE_CLOSED_LOOP 2   /* ... then u_t = clamp(U[t] + K[t] (x_t (-) X[t])), x_{t+1} = f(x_t, u_t), with the shifted U, K, X */
int ddp_hip_advance(ddp_hip_ctx* ctx, int64_t shift, const double* x0, int32_t mode);

/* ---- outer augmented-Lagrangian loop (solve<M>, ddp.hpp:745-842): the parts of update_derivatives
 * (ddp.hpp:642-696) between compute_derivatives and backward_pass, on the resident sequences ---------- */
/* affine_vector_function_seq_t::update_origin (mat_seq_common.hpp:62-89) with x_new = X:
 * val += jac (X - origin); origin = X.  which = 0: the multipliers (MULT_*), 1: the control feedback (FB_*) */
int ddp_hip_update_origin(ddp_hip_ctx* ctx, int which);
/* optimality_obj (ddp.hpp:576-627) and optimality_constr (ddp.hpp:516-523) of (X, multipliers, derivatives);
 * mu, obj_out, constr_out: host [batch] */
int ddp_hip_optimality(ddp_hip_ctx* ctx, const double* mu, double* obj_out, double* constr_out);
/* p.val += mu (eq + eq_u k), p.jac += mu (eq_x + eq_u K) (ddp.hpp:680-688); mu: host [batch] */
int ddp_hip_update_multipliers(ddp_hip_ctx* ctx, const double* mu);

/* Per-instance activity.  solve<M> returns an instance the moment it reaches its optimum (ddp.hpp:799-800); in a batch
 * the others go on.  An inactive instance is frozen: ddp_hip_backward / ddp_hip_forward skip it (its reg / mu / step
 * entries are left as they are) and ddp_hip_swap_traj keeps its (X, U).  active: host [batch] of 0 / 1, NULL = all. */
int ddp_hip_set_active(ddp_hip_ctx* ctx, const int32_t* active);

/* Joint armature: the rotor inertia reflected through the gearbox, N^2 I_rotor, a constant added to the joint's diagonal
 * inertia.  armature: host [nv], one entry a_i >= 0 per tangent row of a 1-DoF joint (kg m^2 revolute, kg prismatic), shared by
 * the batch; the six rows of a free-flyer root carry none (0).  The forward dynamics becomes
 *     qdd = (M(q) + diag(a))^-1 (tau - h(q, v)),   h = RNEA(q, v, 0) unchanged;
 * in the articulated-body algorithm D_i = S_i^T IA_i S_i + a_i and nothing else.  Everything that evaluates f(x, u) or its
 * derivatives follows: rollout, linearise (FD and analytic, both orders), forward, the joint-acceleration cost and
 * ddp_hip_joint_accel.  The gravity torque g(q), the centre of mass and the centroidal momentum are those of the links and do
 * not change (rotor momentum is not modelled).
 * ddp_hip_set_armature waits for the context's stream and writes the values into the resident model: every launch after it
 * sees them; it may be repeated at any time between other calls.  A context it was never called on, or called with zeros,
 * computes bit for bit what it computed without the feature.  DDP_HIP_E_ARG: NULL, a non-finite or negative entry, a non-zero
 * entry in a free-flyer root's rows; DDP_HIP_E_UNSUPPORTED: the pendulum model.  A refused call leaves the old values in force.
 * ddp_hip_get_armature hands the values in force back (zeros after create). */
int ddp_hip_set_armature(ddp_hip_ctx* ctx, const double* armature /* [nv] */);
int ddp_hip_get_armature(ddp_hip_ctx* ctx, double* armature /* [nv] */);

/* solve<primal_dual_affine_multipliers> (ddp.hpp:745-842) for every instance of the context, each with the reference's
 * per-problem semantics: an instance stops at its first optimum (result 1, `iterations` = the iteration that found it)
 * or after max_iterations (result 0), whatever its batch-mates do.  In: X / U the initial trajectory, X_NEW / U_NEW a
 * clone of it (ddp.hpp:752), MULT_* the initial multipliers (val 0, jac the seed the reference draws with setRandom(),
 * origin = X: ddp.hpp:759-764).  Out: the final trajectory in X / U, the feedback in FB_*, log[batch]. */
typedef struct ddp_hip_solver_params {   /* solver_parameters_t, ddp.hpp:42-50 */
  int64_t max_iterations;
  double optimality_stopping_threshold;
  double mu, reg, w, n;
  int32_t n_alpha;        /* line-search candidates per round (1 = the reference's sequential halving) */
  int32_t pad_;
  int64_t max_restarts;   /* bound on the reference's unbounded while(!success) of backward_pass */
} ddp_hip_solver_params;
typedef struct ddp_hip_solve_log {
  int64_t iterations;
  int32_t result;         /* 0 max_iterations reached, 1 optimum attained */
  int32_t pad_;
  double mu, reg, w, n, last_step, opt_obj, opt_constr;
} ddp_hip_solve_log;
int ddp_hip_solve(ddp_hip_ctx* ctx, const ddp_hip_solver_params* params, ddp_hip_solve_log* log);

/* Which implementation each phase of this context runs (a model whose tree matches no compiled-in topology gets the
 * run-time-tree stencil kernels, several times slower: visible here instead of silently) */
typedef struct ddp_hip_info {
  int32_t device;
  int32_t lin_path;       /* 0 closed form (pendulum), 1 run-time-tree kernels (any topology), 2 static TopoTalos38, 3 static TopoChain6,
                           * >= 4 a generated static topology (tools/gen_topology.py -> csrc/topo_extra.h; shipped: 4 Arm7, 5 Biped12).
                           * With first_order == 2 and fd_mode 1 a static topology means: the forward dynamics of the perturbed points come
                           * from the static first-order kernels (one ABA per (instance, t) instead of 2 nv + 1) */
  int32_t first_order;    /* 0 analytic (pendulum_model.hpp:116-130), 1 forward FD (north star), 2 analytic ABA derivatives */
  int32_t bwd_path;       /* 0 run-time-shaped bwd_assemble / bwd_gains, 1 split K3 bwd_contract / K4 bwd_riccati */
  int32_t fwd_path;       /* 0 one lane per rollout, 1 latency path (two workgroups per instance; constrained problems: + parallel cost kernel) */
  int32_t has_tensors;
  int64_t hbm_bytes;      /* bytes of the resident sequences */
} ddp_hip_info;
int ddp_hip_ctx_info(const ddp_hip_ctx* ctx, ddp_hip_info* out);

/* ---- measurement ------------------------------------------------------------------------- */
enum ddp_hip_kernel_id {
  DDP_HIP_K_BWD_ASSEMBLE = 0,   /* Q assembly + tensor contraction (the HBM-bound kernel) */
  DDP_HIP_K_BWD_GAINS,          /* LLT, gains, V update */
  DDP_HIP_K_FWD_ROLLOUT,
  DDP_HIP_K_LIN_FIRST,
  DDP_HIP_K_LIN_SECOND,
  DDP_HIP_K_COUNT
};
/* when enabled, HIP events bracket every launch of the selected kernel classes on the context's stream.
 * on: 0 off; 1 every class; otherwise a bit mask, bit (1 + kernel_id) selects class kernel_id (an event pair costs
 * a few microseconds of stream time per launch: K4's 200 launches per sweep are worth leaving out of a timed run) */
int ddp_hip_profile_enable(ddp_hip_ctx* ctx, int on);
int ddp_hip_profile_reset(ddp_hip_ctx* ctx);
int ddp_hip_profile_get(ddp_hip_ctx* ctx, int kernel_id, double* total_ms, int64_t* launches);
/* algorithmic bytes of one backward sweep of ONE instance (SURVEY.md 8d formula B_bwd) */
int64_t ddp_hip_bwd_algorithmic_bytes(const ddp_hip_ctx* ctx);
/* bytes of f_xx / f_ux / f_uu the tensor contraction physically reads per (instance, step) with the tensors in their current
 * state: all of them (tensors from outside); the columns j >= c of slab c (this context's own mode-2 tensors: symmetric bit for
 * bit); or the lower halves of those columns plus the two non-zero entries of each upper half (the static stencil's tensors: the
 * configuration rows of f are affine, their second differences exact zeros) -- see csrc/bwd_split.h */
int64_t ddp_hip_bwd_stream_bytes(const ddp_hip_ctx* ctx);

/* ---- multi-GPU shard (new, no reference counterpart) ----------------------- */
#define DDP_HIP_COMM_ID_BYTES 128
typedef struct ddp_hip_comm ddp_hip_comm;
int ddp_hip_comm_unique_id(unsigned char id[DDP_HIP_COMM_ID_BYTES]);
int ddp_hip_comm_init(const unsigned char id[DDP_HIP_COMM_ID_BYTES], int rank, int nranks, int device, ddp_hip_comm** out);
int ddp_hip_comm_destroy(ddp_hip_comm* comm);
/* min over ranks of local_cost, and the smallest global index attaining it (RCCL has no MINLOC):
 * two 8-byte all-reduces over xGMI */
int ddp_hip_shard_best(ddp_hip_comm* comm, double local_cost, int64_t local_global_index,
                       double* best_cost, int64_t* best_global_index);
/* The pick on resident data, as ONE collective.  Ownership rule: global instance s lives on rank s mod G at local position
 * s div G.  Every rank forms the cost of the trajectory ddp_hip_forward just produced for each of its instances
 * (sum_t COSTS_OLD + the accepted step's cost difference), takes its local argmin on the device, one 16-byte ncclAllGather
 * of {cost, global index} over xGMI, argmin of the G pairs on the device, one 16-byte read-back.  comm == NULL: a single
 * rank (the same device work without the collective). */
int ddp_hip_shard_pick(ddp_hip_comm* comm, ddp_hip_ctx* ctx, double* best_cost, int64_t* best_global_index);
/* Optional: the winner's trajectory and gains (X, U, FB_ORIGIN, FB_VAL, FB_JAC of global instance best_global_index) from
 * its owner into local instance dst_local of every rank: one grouped ncclBroadcast between the resident sequences
 * (~4.9 MB at the Talos shape).  comm == NULL: a device copy. */
int ddp_hip_shard_broadcast(ddp_hip_comm* comm, ddp_hip_ctx* ctx, int64_t best_global_index, int64_t dst_local);

/* ---- the Model concept point by point (pinocchio_model.hpp:77-186), for a host-side model_t<double> (seam B2, see
 * adapters/pinocchio_double.cpp).  One configuration per call, evaluated on the device by the same rigid-body code the
 * batched entry points use: plumbing, not a hot path.  Matrices nv x nv column-major. ------------------------------ */
typedef struct ddp_hip_model_handle ddp_hip_model_handle;
int ddp_hip_model_create(const ddp_hip_model* model, int device, ddp_hip_model_handle** out);
int ddp_hip_model_destroy(ddp_hip_model_handle* h);
/* joint armature of the handle's model (ddp_hip_set_armature: the same values, checks and error codes): ddp_hip_model_aba and
 * ddp_hip_model_aba_derivatives called after it use D_i + a_i / M + diag(a) */
int ddp_hip_model_set_armature(ddp_hip_model_handle* h, const double* armature /* [nv] */);
/* model_t::dynamics_aba, pinocchio_model.ipp:337-356 */
int ddp_hip_model_aba(ddp_hip_model_handle* h, const double* q, const double* v, const double* tau, double* qdd);
/* model_t::d_dynamics_aba, pinocchio_model.ipp:359-400: d qdd/dq, d qdd/dv, d qdd/dtau = M^-1, each nv x nv; with a free-flyer
 * root the q partials are taken in the tangent (q (+) delta), nq = nv + 1 inputs in q */
int ddp_hip_model_aba_derivatives(ddp_hip_model_handle* h, const double* q, const double* v, const double* tau,
                                  double* dq, double* dv, double* dtau);
/* model_t::frame_coordinates / d_frame_coordinates, pinocchio_model.ipp:418-462 (J: 3 x nv, may be NULL; the reference's
 * WORLD-frame rows) */
int ddp_hip_model_frame(ddp_hip_model_handle* h, int32_t joint, const double off[3], const double* q, double* p3, double* J);
/* The centre of mass c(q) of a tree model and, if J is not NULL, Jc = dc / d(delta q) as 3 x nv column-major: the true jacobian
 * of DDP_HIP_FLAG_COM_COST, formed by the traversal the cost kernels use.  For targets such as "where the CoM is now, plus 5 cm" */
int ddp_hip_model_com(ddp_hip_model_handle* h, const double* q, double* c3, double* J);
/* The velocity vel6 = (pdot, omega) of the point `off` of joint `joint` at the state (q, v), world-aligned axes, as
 * DDP_HIP_FLAG_FRAME_VEL_COST defines it, and, where not NULL, its jacobians Jq = d vel6 / d(delta q) = [D; E] and
 * Jv = d vel6 / dv = [P; W], each 6 x nv column-major, formed by the traversal the cost kernels use.  For targets such as "half
 * the hand's present speed" */
int ddp_hip_model_frame_velocity(ddp_hip_model_handle* h, int32_t joint, const double off[3], const double* q, const double* v,
                                 double* vel6, double* Jq, double* Jv);
/* The centroidal momentum h6 = (l, k) of a tree model at the state (q, v), world-aligned axes, as DDP_HIP_FLAG_MOMENTUM_COST
 * defines it, and, where not NULL, its jacobians Jq = dh / d(delta q) and Jv = dh / dv = A_G, each 6 x nv column-major, formed by
 * the traversal the cost kernels use.  A total mass <= 0: DDP_HIP_E_ARG.  For targets such as "half the present momentum" */
int ddp_hip_model_centroidal_momentum(ddp_hip_model_handle* h, const double* q, const double* v, double* h6, double* Jq, double* Jv);
/* The placement of frame B = (joint_b, off_b) relative to frame A = (joint_a, off_a) of a tree model at the configuration q, as
 * DDP_HIP_FLAG_RELATIVE_FRAME_COST defines it: p3 = R_a^T (p_b - p_a), quat4 the quaternion of R_a^T R_b (x y z w, w >= 0) and,
 * where not NULL, J = [J_pos; R_b^T (W_b - W_a)] as 6 x nv column-major, the jacobian of r at e_rot = 0, formed by the traversal the
 * cost kernels use (columns on both paths or on neither are 0).  joint_a == joint_b: DDP_HIP_E_ARG.  For targets such as "as the
 * hands are now" */
int ddp_hip_model_relative_frame(ddp_hip_model_handle* h, int32_t joint_a, const double off_a[3], int32_t joint_b, const double off_b[3],
                                 const double* q, double* p3, double* quat4, double* J);
/* The generalised gravity torque g(q) [nv] of a tree model at the configuration q, as DDP_HIP_FLAG_CONTROL_GRAV_COST defines it
 * (aba(q, 0, g(q)) = 0), and, where not NULL, G = dg / d(delta q) as nv x nv column-major (G[i + nv j] = dg_i / d(delta q_j);
 * entries off the pattern are 0), formed by the traversal the cost kernels use.  A free-flyer root's six rows are returned as
 * well: the definition covers them, only the cost leaves them out.  For targets and warm starts: "start from U = g(q0)" */
int ddp_hip_model_gravity_torque(ddp_hip_model_handle* h, const double* q, double* g, double* G);
/* The eye and the axis of the aim frame (joint, off, axis) of a tree model at the configuration q, as DDP_HIP_FLAG_FRAME_AIM_COST
 * defines them: p3 the point's world position, n3 = R_j axis the axis' world direction and, where not NULL, J as 6 x nv
 * column-major: the rows of p (point_column), then the rows of n (a_c x n where column c carries rotation), formed by the
 * traversal the cost kernels use (columns off the joint's path are 0).  An axis off unit length (1e-10): DDP_HIP_E_ARG.  For
 * targets such as "what it looks at now, one metre ahead: g = p + n" */
int ddp_hip_model_frame_axis(ddp_hip_model_handle* h, int32_t joint, const double off[3], const double axis[3], const double* q, double* p3,
                             double* n3, double* J);
/* The test point xi = c + tau cdot of DDP_HIP_FLAG_BALANCE_REGION_COST of a tree model at the state (q, v) (tau = 0: the CoM;
 * tau = sqrt(z_c / g): the capture point): xi3 and, where not NULL, Jq = Jc + tau d cdot / d(delta q) and Jv = tau Jc, each
 * 3 x nv column-major, formed entry by entry by the traversal the cost kernels use (a free-flyer root's three linear columns of
 * Jq are Jc's alone).  tau < 0 or non-finite, or a total mass <= 0: DDP_HIP_E_ARG.  For targets such as "the plane 4 cm behind
 * where the capture point is now" */
int ddp_hip_model_capture_point(ddp_hip_model_handle* h, const double* q, const double* v, double tau, double* xi3, double* Jq, double* Jv);
/* The distance of two robot capsules of a tree model at the configuration q, as DDP_HIP_FLAG_CAPSULE_COST defines it: the segment
 * a0 .. a1 fixed in joint ja against b0 .. b1 fixed in joint jb (ja != jb, else DDP_HIP_E_ARG; a non-finite end alike).  *D the
 * distance of the closest points, ca3 and cb3 the two points in the world and, where not NULL, J = dD / d(delta q) as nv doubles,
 * formed by the traversal the cost kernels use: + P_ca . u on path(ja) alone, - P_cb . u on path(jb) alone, 0 elsewhere, and all 0
 * where D == 0.  No radius and no margin enter: d = D - (r_a + r_b + m).  For margins such as "2 cm less than they are apart now" */
int ddp_hip_model_capsule_pair(ddp_hip_model_handle* h, int32_t ja, const double a0[3], const double a1[3], int32_t jb, const double b0[3],
                               const double b1[3], const double* q, double* D, double* ca3, double* cb3, double* J);
/* One robot capsule of a tree model against one oriented box at the configuration q, as DDP_HIP_CAPSULE_VS_BOX defines it, by the
 * device routine the cost kernels use: the segment a0 .. a1 fixed in `joint` with the radius `radius` >= 0, the box of half extents
 * half[3] > 0 at pose[7] = (centre, unit quaternion x y z w).  *d the signed distance f* - radius (margin 0), *s the segment
 * parameter s*, ca the closest point on the segment axis in the world, u = dd / dc_a and, where not NULL, grad[nv] = P_{c_a}^T u
 * over all of path(joint) (all 0 where f* == 0).  A joint outside the model, a non-finite entry, an extent <= 0 or a quaternion
 * that is not unit: DDP_HIP_E_ARG. */
int ddp_hip_model_capsule_box(ddp_hip_model_handle* h, int32_t joint, const double a0[3], const double a1[3], double radius,
                              const double half[3], const double pose[7], const double* q, double* d, double* s, double ca[3], double u[3],
                              double* grad);

/* ---- built-in seeded model tables (no URDF exists offline: SURVEY.md D4, 8d) -------------- */
/* ..._FF: the same robots on a free-flyer root instead of a fixed base / 3 prismatic + 3 revolute base joints */
enum { DDP_HIP_BUILTIN_PENDULUM = 0, DDP_HIP_BUILTIN_CHAIN6 = 1, DDP_HIP_BUILTIN_TREE38 = 2, DDP_HIP_BUILTIN_CHAIN6_FF = 3, DDP_HIP_BUILTIN_TREE38_FF = 4 };
/* fills caller-provided arrays (sized for DDP_HIP_MAX_JOINTS) and points `out` at them */
typedef struct ddp_hip_model_storage {
  int32_t parent[DDP_HIP_MAX_JOINTS];
  int32_t jtype[DDP_HIP_MAX_JOINTS];
  double axis[DDP_HIP_MAX_JOINTS * 3];
  double Rp[DDP_HIP_MAX_JOINTS * 9];
  double pp[DDP_HIP_MAX_JOINTS * 3];
  double mass_j[DDP_HIP_MAX_JOINTS];
  double com[DDP_HIP_MAX_JOINTS * 3];
  double Ic[DDP_HIP_MAX_JOINTS * 9];
} ddp_hip_model_storage;
int ddp_hip_builtin_model(int which, uint64_t seed, ddp_hip_model_storage* storage, ddp_hip_model* out);

#ifdef __cplusplus
}
#endif
#endif
