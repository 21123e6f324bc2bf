"""ctypes binding of libddp_hip.so (include/ddp_hip/ddp_hip.h).

Plumbing only: loads the in-tree shared library, mirrors the C structs and exposes thin numpy
helpers used by tests/ and bench.py.  There is no CPU fallback here or anywhere in the package:
if the library (or a HIP device) is missing, the calls fail loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DDP_HIP_LIB", os.path.join(_HERE, "libddp_hip.so"))   # override: development A/B builds

MAX_JOINTS = 64

OK = 0
EV_LLT_RESTART = 1
EV_LINESEARCH_FLOOR = 2
E_ARG, E_HIP, E_NODEVICE, E_UNSUPPORTED, E_MAX_RESTARTS, E_COMM = -1, -2, -3, -4, -5, -6

MODEL_PENDULUM, MODEL_TREE = 0, 1
EQ_NONE, EQ_CONFIG, EQ_FRAME = 0, 1, 2
BUILTIN_PENDULUM, BUILTIN_CHAIN6, BUILTIN_TREE38, BUILTIN_CHAIN6_FF, BUILTIN_TREE38_FF = 0, 1, 2, 3, 4
JOINT_REVOLUTE, JOINT_PRISMATIC, JOINT_FREEFLYER = 0, 1, 2
FLAG_NO_TENSORS, FLAG_TRACE, FLAG_TRACKING_COST, FLAG_CONTROL_BOUNDS = 1, 2, 4, 8
FLAG_FRAME_COST = 16
FLAG_STATE_LIMITS = 32
FLAG_FRAME_ORIENT_COST = 64
FLAG_COM_COST = 128
FLAG_FRAME_VEL_COST = 256
FLAG_OBSTACLE_COST = 512
FLAG_SELF_COLLISION_COST = 1024
FLAG_MOMENTUM_COST = 2048
FLAG_RELATIVE_FRAME_COST = 4096
FLAG_CONTROL_GRAV_COST = 8192
FLAG_FRAME_AIM_COST = 16384
FLAG_BALANCE_REGION_COST = 32768
FLAG_JOINT_ACCEL_COST = 65536
FLAG_CAPSULE_COST = 131072
MAX_COST_FRAMES = 4
MAX_COLLISION_POINTS, MAX_OBSTACLES = 16, 8
MAX_COLLISION_PAIRS = 32
MAX_FRAME_PAIRS = 4
MAX_AIM_FRAMES = 4
MAX_CAPSULES, MAX_CAPSULE_PAIRS = 16, 32
CAPSULE_VS_ROBOT, CAPSULE_VS_CAPSULE, CAPSULE_VS_HALFSPACE = 0, 1, 2
CAPSULE_VS_GRID, CAPSULE_GRID_MAX_INTERVALS = 3, 32
CAPSULE_VS_BOX, MAX_CAPSULE_BOXES = 4, 8
OBSTACLE_SPHERE, OBSTACLE_HALFSPACE = 0, 1
OBSTACLE_GRID, MAX_GRID_DIM = 2, 256
LIN_COST, LIN_FIRST, LIN_SECOND, LIN_EQ = 1, 2, 4, 8
ADVANCE_NO_ROLL, ADVANCE_OPEN_LOOP, ADVANCE_CLOSED_LOOP = 0, 1, 2

SEQ_NAMES = [
    "X", "U", "X_NEW", "U_NEW", "LFX", "LFXX", "LX", "LU", "LXX", "LUX", "LUU",
    "F_VAL", "FX", "FU", "FXX", "FUX", "FUU",
    "EQ_VAL", "EQ_X", "EQ_U", "EQ_XX", "EQ_UX", "EQ_UU",
    "MULT_ORIGIN", "MULT_VAL", "MULT_JAC", "FB_ORIGIN", "FB_VAL", "FB_JAC",
    "VX_TRACE", "VXX_TRACE", "COSTS_OLD", "COSTS_NEW",
    "COST_XREF", "COST_WX", "COST_UREF", "COST_WU",
    "CTRL_LO", "CTRL_HI", "BOX_STAT",
]
SEQ = {name: i for i, name in enumerate(SEQ_NAMES)}

K_BWD_ASSEMBLE, K_BWD_GAINS, K_FWD_ROLLOUT, K_LIN_FIRST, K_LIN_SECOND = range(5)

# every symbol include/ddp_hip/ddp_hip.h declares
EXPORTS = [
    "ddp_hip_abi_version", "ddp_hip_strerror", "ddp_hip_device_count", "ddp_hip_create", "ddp_hip_destroy",
    "ddp_hip_stream", "ddp_hip_synchronize", "ddp_hip_set_async", "ddp_hip_seq_size", "ddp_hip_device_ptr", "ddp_hip_upload",
    "ddp_hip_download", "ddp_hip_fill", "ddp_hip_rollout", "ddp_hip_linearize", "ddp_hip_linearize_stages",
    "ddp_hip_backward",
    "ddp_hip_forward", "ddp_hip_cost_seq_aug", "ddp_hip_swap_traj",
    "ddp_hip_update_origin", "ddp_hip_optimality", "ddp_hip_update_multipliers", "ddp_hip_profile_enable",
    "ddp_hip_profile_reset", "ddp_hip_profile_get", "ddp_hip_bwd_algorithmic_bytes", "ddp_hip_bwd_stream_bytes", "ddp_hip_comm_unique_id",
    "ddp_hip_comm_init", "ddp_hip_comm_destroy", "ddp_hip_shard_best", "ddp_hip_shard_pick", "ddp_hip_shard_broadcast",
    "ddp_hip_builtin_model",
    "ddp_hip_batch", "ddp_hip_set_active", "ddp_hip_solve", "ddp_hip_ctx_info",
    "ddp_hip_model_create", "ddp_hip_model_destroy", "ddp_hip_model_aba", "ddp_hip_model_aba_derivatives", "ddp_hip_model_frame",
    "ddp_hip_frame_cost_set_frames", "ddp_hip_frame_cost_upload", "ddp_hip_frame_cost_download",
    "ddp_hip_frame_orient_upload", "ddp_hip_frame_orient_download",
    "ddp_hip_state_limits_upload", "ddp_hip_state_limits_download",
    "ddp_hip_com_cost_upload", "ddp_hip_com_cost_download", "ddp_hip_model_com",
    "ddp_hip_frame_vel_upload", "ddp_hip_frame_vel_download", "ddp_hip_model_frame_velocity",
    "ddp_hip_obstacle_set_points", "ddp_hip_obstacle_upload", "ddp_hip_obstacle_download", "ddp_hip_obstacle_clearance",
    "ddp_hip_obstacle_set_grid", "ddp_hip_obstacle_set_occupancy", "ddp_hip_obstacle_grid_download", "ddp_hip_obstacle_grid_query",
    "ddp_hip_obstacle_grid_segment_query",
    "ddp_hip_self_collision_set_pairs", "ddp_hip_self_collision_upload", "ddp_hip_self_collision_download",
    "ddp_hip_self_collision_clearance",
    "ddp_hip_momentum_cost_upload", "ddp_hip_momentum_cost_download", "ddp_hip_model_centroidal_momentum",
    "ddp_hip_relative_frame_set_pairs", "ddp_hip_relative_frame_upload", "ddp_hip_relative_frame_download",
    "ddp_hip_relative_frame_error", "ddp_hip_model_relative_frame",
    "ddp_hip_control_grav_cost_upload", "ddp_hip_control_grav_cost_download", "ddp_hip_model_gravity_torque",
    "ddp_hip_frame_aim_set_frames", "ddp_hip_frame_aim_upload", "ddp_hip_frame_aim_download", "ddp_hip_frame_aim_error",
    "ddp_hip_model_frame_axis",
    "ddp_hip_balance_region_set_planes", "ddp_hip_balance_region_upload", "ddp_hip_balance_region_download",
    "ddp_hip_balance_region_margin", "ddp_hip_model_capture_point",
    "ddp_hip_joint_accel_cost_upload", "ddp_hip_joint_accel_cost_download", "ddp_hip_joint_accel",
    "ddp_hip_capsule_set_pairs", "ddp_hip_capsule_upload", "ddp_hip_capsule_download", "ddp_hip_capsule_clearance",
    "ddp_hip_model_capsule_pair", "ddp_hip_capsule_set_boxes", "ddp_hip_model_capsule_box",
    "ddp_hip_advance",
    "ddp_hip_set_armature", "ddp_hip_get_armature", "ddp_hip_model_set_armature",
]

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)


class Model(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("nv", C.c_int32), ("mass", C.c_double), ("length", C.c_double),
        ("parent", _ip), ("jtype", _ip), ("axis", _dp), ("Rp", _dp), ("pp", _dp),
        ("mass_j", _dp), ("com", _dp), ("Ic", _dp), ("gravity", C.c_double * 3),
    ]


class Problem(C.Structure):
    _fields_ = [
        ("model", Model), ("dt", C.c_double), ("c", C.c_double), ("T", C.c_int64), ("batch", C.c_int64),
        ("eq_kind", C.c_int32), ("eq_advance", C.c_int32), ("ne", _lp), ("eq_target", _dp),
        ("frame_joint", C.c_int32), ("frame_off", C.c_double * 3),
        ("first_order_fd", C.c_int32), ("fd_mode", C.c_int32),
    ]


class SolverParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int64), ("optimality_stopping_threshold", C.c_double), ("mu", C.c_double),
                ("reg", C.c_double), ("w", C.c_double), ("n", C.c_double), ("n_alpha", C.c_int32), ("pad_", C.c_int32),
                ("max_restarts", C.c_int64)]


class SolveLog(C.Structure):
    _fields_ = [("iterations", C.c_int64), ("result", C.c_int32), ("pad_", C.c_int32), ("mu", C.c_double), ("reg", C.c_double),
                ("w", C.c_double), ("n", C.c_double), ("last_step", C.c_double), ("opt_obj", C.c_double),
                ("opt_constr", C.c_double)]


class Info(C.Structure):
    _fields_ = [("device", C.c_int32), ("lin_path", C.c_int32), ("first_order", C.c_int32), ("bwd_path", C.c_int32),
                ("fwd_path", C.c_int32), ("has_tensors", C.c_int32), ("hbm_bytes", C.c_int64)]


class ModelStorage(C.Structure):
    _fields_ = [
        ("parent", C.c_int32 * MAX_JOINTS), ("jtype", C.c_int32 * MAX_JOINTS),
        ("axis", C.c_double * (MAX_JOINTS * 3)), ("Rp", C.c_double * (MAX_JOINTS * 9)),
        ("pp", C.c_double * (MAX_JOINTS * 3)), ("mass_j", C.c_double * MAX_JOINTS),
        ("com", C.c_double * (MAX_JOINTS * 3)), ("Ic", C.c_double * (MAX_JOINTS * 9)),
    ]


_lib = None


def lib():
    """Loads libddp_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    L.ddp_hip_abi_version.restype = C.c_int
    L.ddp_hip_strerror.restype = C.c_char_p
    L.ddp_hip_strerror.argtypes = [C.c_int]
    L.ddp_hip_device_count.restype = C.c_int
    L.ddp_hip_create.argtypes = [C.POINTER(Problem), C.c_int, C.c_uint32, C.POINTER(C.c_void_p)]
    L.ddp_hip_destroy.argtypes = [C.c_void_p]
    L.ddp_hip_stream.restype = C.c_void_p
    L.ddp_hip_stream.argtypes = [C.c_void_p]
    L.ddp_hip_synchronize.argtypes = [C.c_void_p]
    L.ddp_hip_set_async.argtypes = [C.c_void_p, C.c_int]
    L.ddp_hip_seq_size.restype = C.c_int64
    L.ddp_hip_seq_size.argtypes = [C.c_void_p, C.c_int]
    L.ddp_hip_device_ptr.restype = C.c_void_p
    L.ddp_hip_device_ptr.argtypes = [C.c_void_p, C.c_int]
    L.ddp_hip_upload.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int64, C.c_int64]
    L.ddp_hip_download.argtypes = [C.c_void_p, C.c_int, _dp, C.c_int64, C.c_int64]
    L.ddp_hip_fill.argtypes = [C.c_void_p, C.c_int, C.c_double]
    if hasattr(L, "ddp_hip_frame_cost_upload"):      # (DDP_HIP_LIB may name an older build for an A/B run: set_frame_cost then fails there)
        L.ddp_hip_frame_cost_set_frames.argtypes = [C.c_void_p, C.c_int32, _ip, _dp]
        L.ddp_hip_frame_cost_upload.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_frame_cost_download.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
    if hasattr(L, "ddp_hip_frame_orient_upload"):    # (likewise: set_frame_orient_cost fails on an older build)
        L.ddp_hip_frame_orient_upload.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_frame_orient_download.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
    if hasattr(L, "ddp_hip_state_limits_upload"):    # (likewise: set_state_limits fails on an older build)
        L.ddp_hip_state_limits_upload.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_state_limits_download.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int64, C.c_int64]
    if hasattr(L, "ddp_hip_com_cost_upload"):        # (likewise: set_com_cost and ModelHandle.com fail on an older build)
        L.ddp_hip_com_cost_upload.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_com_cost_download.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_model_com.argtypes = [C.c_void_p, _dp, _dp, _dp]
    if hasattr(L, "ddp_hip_frame_vel_upload"):       # (likewise: set_frame_vel_cost and ModelHandle.frame_velocity)
        L.ddp_hip_frame_vel_upload.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_frame_vel_download.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_model_frame_velocity.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp]
    if hasattr(L, "ddp_hip_obstacle_upload"):        # (likewise: set_obstacle_points, set_obstacle_cost, obstacle_clearance)
        L.ddp_hip_obstacle_set_points.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), _dp, _dp, C.c_int32, C.POINTER(C.c_int32)]
        L.ddp_hip_obstacle_upload.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_obstacle_download.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_obstacle_clearance.argtypes = [C.c_void_p, C.c_int, _dp]
    if hasattr(L, "ddp_hip_obstacle_set_grid"):      # (likewise: set_obstacle_grid, set_obstacle_occupancy, obstacle_grid, obstacle_grid_query)
        L.ddp_hip_obstacle_set_grid.argtypes = [C.c_void_p, _ip, _dp, C.c_double, _dp]
        L.ddp_hip_obstacle_set_occupancy.argtypes = [C.c_void_p, _ip, _dp, C.c_double, C.POINTER(C.c_uint8)]
        L.ddp_hip_obstacle_grid_download.argtypes = [C.c_void_p, _ip, _dp, _dp, _dp]
        L.ddp_hip_obstacle_grid_query.argtypes = [C.c_void_p, C.c_int64, _dp, _dp, _dp]
    if hasattr(L, "ddp_hip_obstacle_grid_segment_query"):      # (likewise: obstacle_grid_segment_query)
        L.ddp_hip_obstacle_grid_segment_query.argtypes = [C.c_void_p, C.c_int64, _dp, _ip, _dp, _ip, _dp, _dp]
    if hasattr(L, "ddp_hip_capsule_set_boxes"):      # (likewise: set_capsule_boxes, ModelHandle.capsule_box)
        L.ddp_hip_capsule_set_boxes.argtypes = [C.c_void_p, C.c_int32, _dp]
        L.ddp_hip_model_capsule_box.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, C.c_double, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]
    if hasattr(L, "ddp_hip_self_collision_upload"):  # (likewise: set_self_collision_pairs, set_self_collision_cost, self_collision_clearance)
        L.ddp_hip_self_collision_set_pairs.argtypes = [C.c_void_p, C.c_int32, _ip, _dp, _dp, C.c_int32, _ip, _ip]
        L.ddp_hip_self_collision_upload.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_self_collision_download.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_self_collision_clearance.argtypes = [C.c_void_p, C.c_int, _dp]
    if hasattr(L, "ddp_hip_momentum_cost_upload"):   # (likewise: set_momentum_cost and ModelHandle.centroidal_momentum)
        L.ddp_hip_momentum_cost_upload.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_momentum_cost_download.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_model_centroidal_momentum.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp]
    if hasattr(L, "ddp_hip_relative_frame_upload"):  # (likewise: set_relative_frame_pairs, set_relative_frame_cost, relative_frame_error, ModelHandle.relative_frame)
        L.ddp_hip_relative_frame_set_pairs.argtypes = [C.c_void_p, C.c_int32, _ip, _dp, _ip, _dp]
        L.ddp_hip_relative_frame_upload.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_relative_frame_download.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_relative_frame_error.argtypes = [C.c_void_p, C.c_int, _dp]
        L.ddp_hip_model_relative_frame.argtypes = [C.c_void_p, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp, _dp, _dp]
    if hasattr(L, "ddp_hip_control_grav_cost_upload"):  # (likewise: set_control_grav_cost and ModelHandle.gravity_torque)
        L.ddp_hip_control_grav_cost_upload.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_control_grav_cost_download.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_model_gravity_torque.argtypes = [C.c_void_p, _dp, _dp, _dp]
    if hasattr(L, "ddp_hip_frame_aim_upload"):  # (likewise: set_aim_frames, set_frame_aim_cost, frame_aim_error, ModelHandle.frame_axis)
        L.ddp_hip_frame_aim_set_frames.argtypes = [C.c_void_p, C.c_int32, _ip, _dp, _dp]
        L.ddp_hip_frame_aim_upload.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_frame_aim_download.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_frame_aim_error.argtypes = [C.c_void_p, C.c_int, _dp]
        L.ddp_hip_model_frame_axis.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp]
    if hasattr(L, "ddp_hip_joint_accel_cost_upload"):  # (likewise: set_joint_accel_cost, joint_accel_cost, joint_accel)
        L.ddp_hip_joint_accel_cost_upload.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_joint_accel_cost_download.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_joint_accel.argtypes = [C.c_void_p, C.c_int, _dp]
    if hasattr(L, "ddp_hip_balance_region_upload"):  # (likewise: set_balance_region_planes, set_balance_region_cost, balance_region_margin, ModelHandle.capture_point)
        L.ddp_hip_balance_region_set_planes.argtypes = [C.c_void_p, C.c_int32]
        L.ddp_hip_balance_region_upload.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_balance_region_download.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_balance_region_margin.argtypes = [C.c_void_p, C.c_int, _dp]
        L.ddp_hip_model_capture_point.argtypes = [C.c_void_p, _dp, _dp, C.c_double, _dp, _dp, _dp]
    if hasattr(L, "ddp_hip_capsule_upload"):  # (likewise: set_capsule_pairs, set_capsule_cost, capsule_clearance, ModelHandle.capsule_pair)
        L.ddp_hip_capsule_set_pairs.argtypes = [C.c_void_p, C.c_int32, _ip, _dp, _dp, _dp, C.c_int32, _ip, _ip, _ip]
        L.ddp_hip_capsule_upload.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_capsule_download.argtypes = [C.c_void_p, _dp, _dp, C.c_int64, C.c_int64]
        L.ddp_hip_capsule_clearance.argtypes = [C.c_void_p, C.c_int, _dp]
        L.ddp_hip_model_capsule_pair.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, C.c_int32, _dp, _dp, _dp, _dp, _dp, _dp, _dp]
    if hasattr(L, "ddp_hip_advance"):  # (likewise: Context.advance and solver.mpc_step)
        L.ddp_hip_advance.argtypes = [C.c_void_p, C.c_int64, _dp, C.c_int32]
    L.ddp_hip_rollout.argtypes = [C.c_void_p]
    L.ddp_hip_linearize.argtypes = [C.c_void_p]
    L.ddp_hip_linearize_stages.argtypes = [C.c_void_p, C.c_uint32]
    L.ddp_hip_backward.argtypes = [C.c_void_p, _dp, _dp, _lp, C.c_int64]
    L.ddp_hip_forward.argtypes = [C.c_void_p, _dp, C.c_int32, _dp, _dp]
    L.ddp_hip_cost_seq_aug.argtypes = [C.c_void_p, C.c_int, _dp]
    L.ddp_hip_swap_traj.argtypes = [C.c_void_p]
    L.ddp_hip_update_origin.argtypes = [C.c_void_p, C.c_int]
    L.ddp_hip_optimality.argtypes = [C.c_void_p, _dp, _dp, _dp]
    L.ddp_hip_update_multipliers.argtypes = [C.c_void_p, _dp]
    L.ddp_hip_profile_enable.argtypes = [C.c_void_p, C.c_int]
    L.ddp_hip_profile_reset.argtypes = [C.c_void_p]
    L.ddp_hip_profile_get.argtypes = [C.c_void_p, C.c_int, _dp, _lp]
    L.ddp_hip_bwd_algorithmic_bytes.restype = C.c_int64
    L.ddp_hip_bwd_stream_bytes.restype = C.c_int64
    L.ddp_hip_bwd_stream_bytes.argtypes = [C.c_void_p]
    L.ddp_hip_bwd_algorithmic_bytes.argtypes = [C.c_void_p]
    L.ddp_hip_comm_unique_id.argtypes = [C.POINTER(C.c_ubyte)]
    L.ddp_hip_comm_init.argtypes = [C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.ddp_hip_comm_destroy.argtypes = [C.c_void_p]
    L.ddp_hip_shard_best.argtypes = [C.c_void_p, C.c_double, C.c_int64, _dp, _lp]
    L.ddp_hip_shard_pick.argtypes = [C.c_void_p, C.c_void_p, _dp, _lp]
    L.ddp_hip_shard_broadcast.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
    L.ddp_hip_builtin_model.argtypes = [C.c_int, C.c_uint64, C.POINTER(ModelStorage), C.POINTER(Model)]
    L.ddp_hip_batch.restype = C.c_int64
    L.ddp_hip_batch.argtypes = [C.c_void_p]
    L.ddp_hip_set_active.argtypes = [C.c_void_p, _ip]
    L.ddp_hip_solve.argtypes = [C.c_void_p, C.POINTER(SolverParams), C.POINTER(SolveLog)]
    L.ddp_hip_ctx_info.argtypes = [C.c_void_p, C.POINTER(Info)]
    L.ddp_hip_model_create.argtypes = [C.POINTER(Model), C.c_int, C.POINTER(C.c_void_p)]
    L.ddp_hip_model_destroy.argtypes = [C.c_void_p]
    L.ddp_hip_model_aba.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp]
    L.ddp_hip_model_aba_derivatives.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp, _dp]
    L.ddp_hip_model_frame.argtypes = [C.c_void_p, C.c_int32, _dp, _dp, _dp, _dp]
    if hasattr(L, "ddp_hip_set_armature"):           # (likewise: set_armature / get_armature, ModelHandle.set_armature)
        L.ddp_hip_set_armature.argtypes = [C.c_void_p, _dp]
        L.ddp_hip_get_armature.argtypes = [C.c_void_p, _dp]
        L.ddp_hip_model_set_armature.argtypes = [C.c_void_p, _dp]
    _lib = L
    return L


class DdpHipError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        super().__init__(f"{where}: {lib().ddp_hip_strerror(code).decode()} ({code})")


def _check(code, where):
    if code < 0:
        raise DdpHipError(code, where)
    return code


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return a.ctypes.data_as(_dp)


def _armature(armature, nv):
    """joint armature as a contiguous [nv] array; a wrong length is refused here, before any device call"""
    a = _f64(armature).reshape(-1)
    if a.size != nv:
        raise ValueError(f"armature has {a.size} entries, the model has nv = {nv}")
    return a


class BuiltinModel:
    """Seeded model table from the library (ddp_hip_builtin_model), as numpy arrays."""

    def __init__(self, which, seed=0):
        self.storage = ModelStorage()
        self.model = Model()
        _check(lib().ddp_hip_builtin_model(which, seed, C.byref(self.storage), C.byref(self.model)), "builtin_model")
        self.kind, self.nv = self.model.kind, self.model.nv
        self.mass, self.length = self.model.mass, self.model.length
        self.gravity = np.array(list(self.model.gravity))
        st = self.storage
        # a free-flyer root (jtype[0] == JOINT_FREEFLYER) owns six of the nv velocities: nv - 5 joints, nq = nv + 1
        self.ff = self.kind == MODEL_TREE and st.jtype[0] == JOINT_FREEFLYER
        self.nj = nv = self.nv - 5 if self.ff else self.nv
        self.nq = self.nv + 1 if self.ff else self.nv
        self.parent = np.array(st.parent[:nv], dtype=np.int32)
        self.jtype = np.array(st.jtype[:nv], dtype=np.int32)
        self.axis = np.array(st.axis[:3 * nv]).reshape(nv, 3)
        self.Rp = np.array(st.Rp[:9 * nv]).reshape(nv, 3, 3)
        self.pp = np.array(st.pp[:3 * nv]).reshape(nv, 3)
        self.mass_j = np.array(st.mass_j[:nv])
        self.com = np.array(st.com[:3 * nv]).reshape(nv, 3)
        self.Ic = np.array(st.Ic[:9 * nv]).reshape(nv, 3, 3)

    def neutral(self):
        """neutral configuration (pinocchio::neutral): zeros, unit quaternion for a free-flyer root"""
        q = np.zeros(self.nq)
        if self.ff:
            q[6] = 1.0
        return q


class TableModel(BuiltinModel):
    """A tree of 1-DoF joints given as arrays (what adapters/urdf_reader.hpp produces from a URDF, or any robot description
    the host has): parent[nv] (parent[i] < i, -1 = world), jtype[nv] (JOINT_REVOLUTE / JOINT_PRISMATIC), axis[nv][3] (unit,
    joint frame), Rp[nv][3][3] and pp[nv][3] (placement in the parent frame), mass_j[nv], com[nv][3], Ic[nv][3][3] (about the
    com).  Same attributes as BuiltinModel, so the product (ProblemSpec) and the oracle take it alike."""

    def __init__(self, parent, jtype, axis, Rp, pp, mass_j, com, Ic, gravity=(0.0, 0.0, -9.81)):
        nv = len(parent)
        assert 1 <= nv <= 64
        self.storage = ModelStorage()
        self.model = Model()
        st = self.storage
        self.parent = np.ascontiguousarray(parent, dtype=np.int32)
        self.jtype = np.ascontiguousarray(jtype, dtype=np.int32)
        self.axis, self.Rp, self.pp = _f64(axis).reshape(nv, 3), _f64(Rp).reshape(nv, 3, 3), _f64(pp).reshape(nv, 3)
        self.mass_j, self.com, self.Ic = _f64(mass_j).reshape(nv), _f64(com).reshape(nv, 3), _f64(Ic).reshape(nv, 3, 3)
        for name, arr in (("parent", self.parent), ("jtype", self.jtype), ("axis", self.axis), ("Rp", self.Rp), ("pp", self.pp),
                          ("mass_j", self.mass_j), ("com", self.com), ("Ic", self.Ic)):
            dst = getattr(st, name)
            flat = arr.reshape(-1)
            for i in range(flat.size):
                dst[i] = flat[i]
        m = self.model
        m.kind, m.nv, m.mass, m.length = MODEL_TREE, nv, 0.0, 0.0
        m.parent = C.cast(st.parent, _ip); m.jtype = C.cast(st.jtype, _ip)
        m.axis = C.cast(st.axis, _dp); m.Rp = C.cast(st.Rp, _dp); m.pp = C.cast(st.pp, _dp)
        m.mass_j = C.cast(st.mass_j, _dp); m.com = C.cast(st.com, _dp); m.Ic = C.cast(st.Ic, _dp)
        m.gravity = (C.c_double * 3)(*[float(g) for g in gravity])
        self.kind, self.nv, self.mass, self.length = MODEL_TREE, nv, 0.0, 0.0
        self.gravity = np.array([float(g) for g in gravity])
        self.ff, self.nj, self.nq = False, nv, nv


class ModelHandle:
    """Point evaluations of the Model concept on the device (ddp_hip_model_*, seam B2)"""

    def __init__(self, model, device=0):
        self.model, self.nv, self.nq = model, model.nv, getattr(model, "nq", model.nv)
        self._h = C.c_void_p()
        _check(lib().ddp_hip_model_create(C.byref(model.model), device, C.byref(self._h)), "model_create")

    def close(self):
        if self._h:
            lib().ddp_hip_model_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_armature(self, armature):
        """Joint armature [nv] of the handle's model (ddp_hip_model_set_armature): aba / aba_derivatives after it use
        D_i + a_i.  None passes NULL (refused)."""
        a = None if armature is None else _armature(armature, self.nv)
        _check(lib().ddp_hip_model_set_armature(self._h, None if a is None else _ptr(a)), "model_set_armature")

    def aba(self, q, v, tau):
        q, v, tau, out = _f64(q), _f64(v), _f64(tau), np.zeros(self.nv)
        _check(lib().ddp_hip_model_aba(self._h, _ptr(q), _ptr(v), _ptr(tau), _ptr(out)), "model_aba")
        return out

    def aba_derivatives(self, q, v, tau):
        q, v, tau = _f64(q), _f64(v), _f64(tau)
        n = self.nv
        dq, dv, dt = np.zeros(n * n), np.zeros(n * n), np.zeros(n * n)
        _check(lib().ddp_hip_model_aba_derivatives(self._h, _ptr(q), _ptr(v), _ptr(tau), _ptr(dq), _ptr(dv), _ptr(dt)), "model_aba_derivatives")
        return dq.reshape(n, n).T.copy(), dv.reshape(n, n).T.copy(), dt.reshape(n, n).T.copy()

    def frame(self, joint, off, q, jac=True):
        off, q = _f64(off), _f64(q)
        p3, J = np.zeros(3), np.zeros(3 * self.nv)
        _check(lib().ddp_hip_model_frame(self._h, joint, _ptr(off), _ptr(q), _ptr(p3), _ptr(J) if jac else None), "model_frame")
        return p3, J.reshape(self.nv, 3).T.copy()


    def com(self, q, jacobian=False):
        """The centre of mass c(q) of a tree model; with jacobian=True (c, Jc), Jc = dc / d(delta q) as (3, nv): the true
        jacobian of FLAG_COM_COST (ddp_hip.h)"""
        q = _f64(q)
        c3, J = np.zeros(3), np.zeros(3 * self.nv)
        _check(lib().ddp_hip_model_com(self._h, _ptr(q), _ptr(c3), _ptr(J) if jacobian else None), "model_com")
        return (c3, J.reshape(self.nv, 3).T.copy()) if jacobian else c3
    def frame_velocity(self, joint, off, q, v, jacobian=False):
        """The velocity (pdot, omega) of the point `off` of joint `joint` at the state (q, v), world-aligned axes, as (6,); with
        jacobian=True (vel6, Jq, Jv), Jq = d vel6 / d(delta q) and Jv = d vel6 / dv as (6, nv): the jacobians of
        FLAG_FRAME_VEL_COST (ddp_hip.h)"""
        q, v, off = _f64(q), _f64(v), _f64(off)
        vel, Jq, Jv = np.zeros(6), np.zeros(6 * self.nv), np.zeros(6 * self.nv)
        _check(lib().ddp_hip_model_frame_velocity(self._h, int(joint), _ptr(off), _ptr(q), _ptr(v), _ptr(vel), _ptr(Jq) if jacobian else None,
                                                  _ptr(Jv) if jacobian else None), "model_frame_velocity")
        return (vel, Jq.reshape(self.nv, 6).T.copy(), Jv.reshape(self.nv, 6).T.copy()) if jacobian else vel

    def centroidal_momentum(self, q, v, jacobian=False):
        """The centroidal momentum h = (l, k) of a tree model at the state (q, v), world-aligned axes, k about the centre of
        mass, as (6,); with jacobian=True (h6, Jq, Jv), Jq = dh / d(delta q) and Jv = dh / dv = A_G as (6, nv): the jacobians of
        FLAG_MOMENTUM_COST (ddp_hip.h)"""
        q, v = _f64(q), _f64(v)
        h6, Jq, Jv = np.zeros(6), np.zeros(6 * self.nv), np.zeros(6 * self.nv)
        _check(lib().ddp_hip_model_centroidal_momentum(self._h, _ptr(q), _ptr(v), _ptr(h6), _ptr(Jq) if jacobian else None,
                                                       _ptr(Jv) if jacobian else None), "model_centroidal_momentum")
        return (h6, Jq.reshape(self.nv, 6).T.copy(), Jv.reshape(self.nv, 6).T.copy()) if jacobian else h6

    def relative_frame(self, joint_a, off_a, joint_b, off_b, q, jacobian=False):
        """The placement of frame B = (joint_b, off_b) relative to frame A = (joint_a, off_a) at q, as FLAG_RELATIVE_FRAME_COST
        defines it (ddp_hip.h): (p3, quat4) = R_a^T (p_b - p_a) and the quaternion of R_a^T R_b (x y z w, w >= 0); with
        jacobian=True (p3, quat4, J), J = [J_pos; R_b^T (W_b - W_a)] as (6, nv), the jacobian of the residual at e_rot = 0"""
        off_a, off_b, q = _f64(off_a), _f64(off_b), _f64(q)
        if off_a.shape != (3,) or off_b.shape != (3,):
            raise ValueError("relative_frame: every off is a 3-vector")
        p3, qt, J = np.zeros(3), np.zeros(4), np.zeros(6 * self.nv)
        _check(lib().ddp_hip_model_relative_frame(self._h, int(joint_a), _ptr(off_a), int(joint_b), _ptr(off_b), _ptr(q), _ptr(p3), _ptr(qt),
                                                  _ptr(J) if jacobian else None), "model_relative_frame")
        return (p3, qt, J.reshape(self.nv, 6).T.copy()) if jacobian else (p3, qt)

    def frame_axis(self, joint, off, axis, q, jacobian=False):
        """The eye and the axis of the aim frame (joint, off, axis) at q, as FLAG_FRAME_AIM_COST defines them (ddp_hip.h):
        (p3, n3), the point's world position and the axis' world direction; with jacobian=True (p3, n3, J), J = [dp; dn] /
        d(delta q) as (6, nv).  For targets such as what it looks at now, one metre ahead: g = p + n"""
        off, axis, q = _f64(off), _f64(axis), _f64(q)
        if off.shape != (3,) or axis.shape != (3,):
            raise ValueError("frame_axis: off and axis are 3-vectors")
        p3, n3, J = np.zeros(3), np.zeros(3), np.zeros(6 * self.nv)
        _check(lib().ddp_hip_model_frame_axis(self._h, int(joint), _ptr(off), _ptr(axis), _ptr(q), _ptr(p3), _ptr(n3),
                                              _ptr(J) if jacobian else None), "model_frame_axis")
        return (p3, n3, J.reshape(self.nv, 6).T.copy()) if jacobian else (p3, n3)

    def capsule_pair(self, joint_a, a0, a1, joint_b, b0, b1, q, jacobian=False):
        """The distance of two robot capsules at q, as FLAG_CAPSULE_COST defines it (ddp_hip.h): the segment a0 .. a1 fixed in
        joint_a against b0 .. b1 fixed in joint_b (another joint).  (D, ca, cb): the distance of the closest points and the two
        points in the world; with jacobian=True (D, ca, cb, J), J = dD / d(delta q) as (nv,).  No radius and no margin enter.
        For margins such as "2 cm less than they are apart now" """
        a0, a1, b0, b1, q = _f64(a0), _f64(a1), _f64(b0), _f64(b1), _f64(q)
        if any(e.shape != (3,) for e in (a0, a1, b0, b1)):
            raise ValueError("capsule_pair: every end is a 3-vector")
        D, ca, cb, J = np.zeros(1), np.zeros(3), np.zeros(3), np.zeros(self.nv)
        _check(lib().ddp_hip_model_capsule_pair(self._h, int(joint_a), _ptr(a0), _ptr(a1), int(joint_b), _ptr(b0), _ptr(b1), _ptr(q), _ptr(D),
                                                _ptr(ca), _ptr(cb), _ptr(J) if jacobian else None), "model_capsule_pair")
        return (float(D[0]), ca, cb, J) if jacobian else (float(D[0]), ca, cb)

    def capsule_box(self, joint, a0, a1, radius, half, pose, q, gradient=False):
        """One robot capsule against one oriented box at q, as CAPSULE_VS_BOX defines it (ddp_hip.h), by the device routine the cost
        kernels use: the segment a0 .. a1 fixed in `joint` with `radius`, the box of half extents half (3,) at pose (7,) = (centre,
        unit quaternion x y z w).  (d, s, ca, u): the signed distance with margin 0, the segment parameter, the closest point on the
        segment axis in the world and u = dd / dc_a; with gradient=True (d, s, ca, u, grad), grad = P_ca^T u as (nv,)"""
        a0, a1, half, pose, q = _f64(a0), _f64(a1), _f64(half), _f64(pose), _f64(q)
        if any(e.shape != (3,) for e in (a0, a1, half)) or pose.shape != (7,):
            raise ValueError("capsule_box: a0, a1 and half are 3-vectors, pose is (centre, quaternion x y z w)")
        d, s, ca, u, g = np.zeros(1), np.zeros(1), np.zeros(3), np.zeros(3), np.zeros(self.nv)
        _check(lib().ddp_hip_model_capsule_box(self._h, int(joint), _ptr(a0), _ptr(a1), float(radius), _ptr(half), _ptr(pose), _ptr(q), _ptr(d),
                                               _ptr(s), _ptr(ca), _ptr(u), _ptr(g) if gradient else None), "model_capsule_box")
        return (float(d[0]), float(s[0]), ca, u, g) if gradient else (float(d[0]), float(s[0]), ca, u)

    def capture_point(self, q, v, tau, jacobian=False):
        """The test point xi = c + tau cdot of FLAG_BALANCE_REGION_COST (ddp_hip.h) at the state (q, v) as (3,): the centre of mass
        at tau = 0, the capture point at tau = sqrt(z_c / g); with jacobian=True (xi, Jq, Jv), Jq = Jc + tau d cdot / d(delta q)
        and Jv = tau Jc as (3, nv).  For targets such as the plane 4 cm behind where the capture point is now"""
        q, v = _f64(q), _f64(v)
        xi, Jq, Jv = np.zeros(3), np.zeros(3 * self.nv), np.zeros(3 * self.nv)
        _check(lib().ddp_hip_model_capture_point(self._h, _ptr(q), _ptr(v), float(tau), _ptr(xi), _ptr(Jq) if jacobian else None,
                                                 _ptr(Jv) if jacobian else None), "model_capture_point")
        return (xi, Jq.reshape(self.nv, 3).T.copy(), Jv.reshape(self.nv, 3).T.copy()) if jacobian else xi

    def gravity_torque(self, q, jacobian=False):
        """The generalised gravity torque g(q) of a tree model as (nv,): the control that holds the robot at rest, aba(q, 0, g) = 0,
        as FLAG_CONTROL_GRAV_COST defines it (ddp_hip.h); with jacobian=True (g, G), G = dg / d(delta q) as (nv, nv).  A
        free-flyer root's six rows are returned as well.  For targets and warm starts: "start from U = g(q0)" """
        q = _f64(q)
        g, G = np.zeros(self.nv), np.zeros(self.nv * self.nv)
        _check(lib().ddp_hip_model_gravity_torque(self._h, _ptr(q), _ptr(g), _ptr(G) if jacobian else None), "model_gravity_torque")
        return (g, G.reshape(self.nv, self.nv).T.copy()) if jacobian else g



class ProblemSpec:
    """Host-side description of problem_t (problem.hpp:872-1150) for one context."""

    def __init__(self, model, T, dt=0.01, c=1.0, batch=1, eq_kind=EQ_NONE, eq_advance=2, ne=None, eq_target=None,
                 frame_joint=0, frame_off=(0.0, 0.0, 0.0), first_order_fd=None, fd_mode=0, armature=None):
        self.model = model
        # joint armature [nv] (ddp_hip_set_armature), applied by Context right after create; None: none
        self.armature = None if armature is None else _armature(armature, model.nv)
        self.T, self.dt, self.c, self.batch = int(T), float(dt), float(c), int(batch)
        self.eq_kind, self.eq_advance = int(eq_kind), int(eq_advance)
        self.ne = np.zeros(self.T, dtype=np.int64) if ne is None else np.ascontiguousarray(ne, dtype=np.int64)
        self.eq_target = _f64(np.zeros(0) if eq_target is None else eq_target)
        self.frame_joint, self.frame_off = int(frame_joint), tuple(float(v) for v in frame_off)
        if first_order_fd is None:
            first_order_fd = 0 if model.kind == MODEL_PENDULUM else 1
        self.first_order_fd, self.fd_mode = int(first_order_fd), int(fd_mode)
        self.nv = model.nv
        self.n, self.m, self.nx = 2 * model.nv, model.nv, getattr(model, "nq", model.nv) + model.nv
        self.Etot = int(self.ne.sum())

    def c_struct(self):
        p = Problem()
        p.model = self.model.model
        p.dt, p.c, p.T, p.batch = self.dt, self.c, self.T, self.batch
        p.eq_kind, p.eq_advance = self.eq_kind, self.eq_advance
        p.ne = self.ne.ctypes.data_as(_lp)
        p.eq_target = _ptr(self.eq_target) if self.eq_target.size else None
        p.frame_joint = self.frame_joint
        p.frame_off = (C.c_double * 3)(*self.frame_off)
        p.first_order_fd, p.fd_mode = self.first_order_fd, self.fd_mode
        return p


class Context:
    """One ddp_hip context (= `batch` resident problem instances on one GPU)."""

    def __init__(self, spec, device=0, flags=0):
        self.spec = spec
        self._h = C.c_void_p()
        self._c_problem = spec.c_struct()
        _check(lib().ddp_hip_create(C.byref(self._c_problem), device, flags, C.byref(self._h)), "ddp_hip_create")
        self.batch = spec.batch
        self.n_cost_frames = 0
        self.n_obstacles = 0
        self.n_collision_pairs = 0
        self.n_frame_pairs = 0
        self.n_aim_frames = 0
        if getattr(spec, "armature", None) is not None:
            try:
                self.set_armature(spec.armature)
            except Exception:
                self.close()
                raise

    def set_armature(self, armature):
        """Joint armature [nv] (reflected rotor inertia; ddp_hip_set_armature): waits for the stream, every launch after it sees
        the values.  None passes NULL (refused)."""
        a = None if armature is None else _armature(armature, self.spec.nv)
        _check(lib().ddp_hip_set_armature(self._h, None if a is None else _ptr(a)), "set_armature")

    def get_armature(self):
        out = np.zeros(self.spec.nv)
        _check(lib().ddp_hip_get_armature(self._h, _ptr(out)), "get_armature")
        return out

    def close(self):
        if self._h:
            lib().ddp_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def seq_size(self, name):
        return int(lib().ddp_hip_seq_size(self._h, SEQ[name]))

    def device_ptr(self, name):
        return lib().ddp_hip_device_ptr(self._h, SEQ[name])

    def upload(self, name, arr, first=0, count=None):
        arr = _f64(arr)
        count = self.batch - first if count is None else count
        assert arr.size == self.seq_size(name) * count, (name, arr.size, self.seq_size(name), count)
        _check(lib().ddp_hip_upload(self._h, SEQ[name], _ptr(arr), first, count), f"upload {name}")

    def download(self, name, first=0, count=None):
        count = self.batch - first if count is None else count
        out = np.empty((count, self.seq_size(name)), dtype=np.float64)
        _check(lib().ddp_hip_download(self._h, SEQ[name], _ptr(out), first, count), f"download {name}")
        return out

    def set_tracking_cost(self, xref=None, wx=None, uref=None, wu=None, first=0, count=None):
        """The tracking cost of instances first .. first + count - 1 (a context created with FLAG_TRACKING_COST; ddp_hip.h):
        xref (T+1, nx), wx (T+1, n), uref (T, m), wu (T, m), each either one array for every instance of the range or
        (count, ...) with one per instance.  None leaves that sequence as it is."""
        count = self.batch - first if count is None else count
        sp = self.spec
        shapes = {"COST_XREF": (sp.T + 1, sp.nx), "COST_WX": (sp.T + 1, sp.n), "COST_UREF": (sp.T, sp.m), "COST_WU": (sp.T, sp.m)}
        for name, arr in (("COST_XREF", xref), ("COST_WX", wx), ("COST_UREF", uref), ("COST_WU", wu)):
            if arr is None:
                continue
            arr = _f64(arr)
            shape = shapes[name]
            if arr.shape == shape:
                arr = np.broadcast_to(arr, (count,) + shape)
            elif arr.shape != (count,) + shape:
                raise ValueError(f"{name}: shape {arr.shape}, expected {shape} or {(count,) + shape}")
            self.upload(name, arr, first, count)

    def set_control_bounds(self, lo=None, hi=None, first=0, count=None):
        """The control bounds lo <= u_t <= hi of instances first .. first + count - 1 (a context created with
        FLAG_CONTROL_BOUNDS; ddp_hip.h): a scalar or an (m,) vector for every step, a (T, m) array for every instance of the
        range, or (count, T, m) with one per instance.  -inf / +inf: no bound on that side.  None leaves that side as it is
        (the library then checks lo <= hi at the next sweep)."""
        count = self.batch - first if count is None else count
        sp = self.spec
        full = (count, sp.T, sp.m)
        arrs = {}
        for name, arr in (("CTRL_LO", lo), ("CTRL_HI", hi)):
            if arr is None:
                continue
            arr = np.asarray(arr, dtype=np.float64)
            if arr.ndim > 3 or (arr.ndim == 3 and arr.shape != full) or (arr.ndim == 2 and arr.shape != full[1:]) or \
                    (arr.ndim == 1 and arr.shape != full[2:]):
                raise ValueError(f"{name}: shape {arr.shape}, expected a scalar, {full[2:]}, {full[1:]} or {full}")
            arrs[name] = np.ascontiguousarray(np.broadcast_to(arr, full))
        if len(arrs) == 2 and bool(np.any(arrs["CTRL_LO"] > arrs["CTRL_HI"])):
            raise ValueError("set_control_bounds: some lo > hi")
        for name, arr in arrs.items():
            self.upload(name, arr, first, count)

    def _cost_sides(self, where, sides, first, count):
        """The sides of one add-on cost term's upload, checked before the library is touched: each side is (label, array or
        None, per-instance shape, further accepted shapes).  An array is (count,) + per, per, or one of the further shapes,
        and is broadcast to (count,) + per.  Returns (count, the contiguous arrays or None per side)"""
        count = self.batch - first if count is None else count
        out = []
        for label, arr, per, extra in sides:
            if arr is not None:
                arr = np.asarray(arr, dtype=np.float64)
                full = (count,) + tuple(per)
                accepted = (full, tuple(per)) + tuple(extra)
                if arr.shape not in accepted:
                    raise ValueError(f"{where} {label}: shape {arr.shape}, expected one of {accepted[::-1]}")
                arr = np.ascontiguousarray(np.broadcast_to(arr, full))
            out.append(arr)
        return count, out

    def _cost_upload(self, fn, where, arrs, first, count):
        """... and their single library call (no side given: no call)"""
        if any(a is not None for a in arrs):
            _check(fn(self._h, *[_ptr(a) if a is not None else None for a in arrs], first, count), where)

    def _cost_download(self, fn, where, pers, first, count):
        """One add-on cost term's sides of instances first .. first + count - 1, each (count,) + per"""
        count = self.batch - first if count is None else count
        out = tuple(np.zeros((max(count, 0),) + tuple(per)) for per in pers)
        _check(fn(self._h, *[_ptr(a) for a in out], first, count), where)
        return out

    def set_frame_cost(self, frames=None, target=None, weight=None, first=0, count=None):
        """The frame-position cost (a context created with FLAG_FRAME_COST; ddp_hip.h).  frames: a list of up to
        MAX_COST_FRAMES (joint, off) pairs, shared by the batch (another count than before resets targets and weights to 0).
        target / weight of instances first .. first + count - 1: (T+1, F, 3) for every instance of the range or
        (count, T+1, F, 3) with one per instance; weight also takes (F, 3), (3,) and scalars by broadcast.  None leaves that
        side as it is."""
        n_frames = self.n_cost_frames
        if frames is not None:
            frames = list(frames)
            n_frames = len(frames)
            joint = np.ascontiguousarray([int(j) for j, _ in frames], dtype=np.int32)
            off = [np.asarray(o, dtype=np.float64) for _, o in frames]
            if any(o.shape != (3,) for o in off):
                raise ValueError("set_frame_cost frames: every off is a 3-vector")
            off = _f64(off).reshape(-1)
        per = (self.spec.T + 1, n_frames, 3)
        count, arrs = self._cost_sides("set_frame_cost", (("target", target, per, ()), ("weight", weight, per, (per[1:], per[2:], ()))),
                                       first, count)
        if frames is not None:
            _check(lib().ddp_hip_frame_cost_set_frames(self._h, n_frames, joint.ctypes.data_as(_ip), _ptr(off)), "frame_cost_set_frames")
            self.n_cost_frames = n_frames
        self._cost_upload(lib().ddp_hip_frame_cost_upload, "frame_cost_upload", arrs, first, count)

    def frame_cost(self, first=0, count=None):
        """(target, weight) of instances first .. first + count - 1, each (count, T+1, F, 3)"""
        per = (self.spec.T + 1, self.n_cost_frames, 3)
        return self._cost_download(lib().ddp_hip_frame_cost_download, "frame_cost_download", (per, per), first, count)

    def set_frame_orient_cost(self, quat=None, weight=None, first=0, count=None):
        """The orientation terms of the cost frames (a context created with FLAG_FRAME_COST | FLAG_FRAME_ORIENT_COST, frames
        set through set_frame_cost; ddp_hip.h).  quat: reference rotations as unit quaternions (x y z w), weight: per axis of
        the frame, >= 0; of instances first .. first + count - 1: (T+1, F, 4) / (T+1, F, 3) for every instance of the range or
        (count, T+1, F, .) with one per instance; weight also takes (F, 3), (3,) and scalars by broadcast.  None leaves that
        side as it is."""
        T1, F = self.spec.T + 1, self.n_cost_frames
        count, arrs = self._cost_sides("set_frame_orient_cost", (("quat", quat, (T1, F, 4), ()), ("weight", weight, (T1, F, 3), ((F, 3), (3,), ()))),
                                       first, count)
        if arrs[0] is not None and not bool(np.all(np.abs(np.sqrt(np.sum(arrs[0] ** 2, axis=-1)) - 1.0) <= 1e-10)):
            raise ValueError("set_frame_orient_cost quat: every quaternion has unit norm (to 1e-10)")
        self._cost_upload(lib().ddp_hip_frame_orient_upload, "frame_orient_upload", arrs, first, count)

    def frame_orient_cost(self, first=0, count=None):
        """(quat, weight) of instances first .. first + count - 1: (count, T+1, F, 4) and (count, T+1, F, 3)"""
        T1, F = self.spec.T + 1, self.n_cost_frames
        return self._cost_download(lib().ddp_hip_frame_orient_download, "frame_orient_download", ((T1, F, 4), (T1, F, 3)), first, count)

    def set_com_cost(self, target=None, weight=None, first=0, count=None):
        """The centre-of-mass terms of instances first .. first + count - 1 (a context created with FLAG_COM_COST; ddp_hip.h).
        target: world positions, weight: per world axis, >= 0; each (T+1, 3) for every instance of the range or
        (count, T+1, 3) with one per instance; weight also takes (3,) and scalars for every step.  None leaves that side as
        it is."""
        per = (self.spec.T + 1, 3)
        count, arrs = self._cost_sides("set_com_cost", (("target", target, per, ()), ("weight", weight, per, ((3,), ()))), first, count)
        self._cost_upload(lib().ddp_hip_com_cost_upload, "com_cost_upload", arrs, first, count)

    def com_cost(self, first=0, count=None):
        """(target, weight) of instances first .. first + count - 1, each (count, T+1, 3)"""
        per = (self.spec.T + 1, 3)
        return self._cost_download(lib().ddp_hip_com_cost_download, "com_cost_download", (per, per), first, count)

    def set_frame_vel_cost(self, target=None, weight=None, first=0, count=None):
        """The frame-velocity terms of instances first .. first + count - 1 (a context created with FLAG_FRAME_VEL_COST; ddp_hip.h),
        of the F frames of set_frame_cost.  target: desired linear, then angular velocity in world axes, weight: per axis, >= 0;
        each (T+1, F, 6) for every instance of the range or (count, T+1, F, 6) with one per instance; weight also takes (6,) and
        scalars for every step and frame.  None leaves that side as it is."""
        per = (self.spec.T + 1, getattr(self, "n_cost_frames", 0), 6)
        count, arrs = self._cost_sides("set_frame_vel_cost", (("target", target, per, ()), ("weight", weight, per, ((6,), ()))), first, count)
        self._cost_upload(lib().ddp_hip_frame_vel_upload, "frame_vel_upload", arrs, first, count)

    def frame_vel_cost(self, first=0, count=None):
        """(target, weight) of instances first .. first + count - 1, each (count, T+1, F, 6)"""
        per = (self.spec.T + 1, getattr(self, "n_cost_frames", 0), 6)
        return self._cost_download(lib().ddp_hip_frame_vel_download, "frame_vel_download", (per, per), first, count)

    def set_momentum_cost(self, target=None, weight=None, first=0, count=None):
        """The centroidal-momentum terms of instances first .. first + count - 1 (a context created with FLAG_MOMENTUM_COST;
        ddp_hip.h).  target: desired linear, then angular momentum (about the centre of mass) in world axes, weight: per axis,
        >= 0; each (T+1, 6) for every instance of the range or (count, T+1, 6) with one per instance; weight also takes (6,) and
        scalars for every step.  None leaves that side as it is."""
        per = (self.spec.T + 1, 6)
        count, arrs = self._cost_sides("set_momentum_cost", (("target", target, per, ()), ("weight", weight, per, ((6,), ()))), first, count)
        self._cost_upload(lib().ddp_hip_momentum_cost_upload, "momentum_cost_upload", arrs, first, count)

    def momentum_cost(self, first=0, count=None):
        """(target, weight) of instances first .. first + count - 1, each (count, T+1, 6)"""
        per = (self.spec.T + 1, 6)
        return self._cost_download(lib().ddp_hip_momentum_cost_download, "momentum_cost_download", (per, per), first, count)

    def set_control_grav_cost(self, offset=None, weight=None, first=0, count=None):
        """The control-gravity terms of instances first .. first + count - 1 (a context created with FLAG_CONTROL_GRAV_COST;
        ddp_hip.h): 1/2 sum_j w_j (u_j - g_j(q) - o_j)^2 at t < T.  offset, weight: (T, m) for every instance of the range or
        (count, T, m) with one per instance; both also take (m,) and scalars by broadcast.  weight >= 0, and 0 on a free-flyer
        root's six rows.  None leaves that side as it is."""
        per, extra = (self.spec.T, self.spec.m), ((self.spec.m,), ())
        count, arrs = self._cost_sides("set_control_grav_cost", (("offset", offset, per, extra), ("weight", weight, per, extra)), first, count)
        self._cost_upload(lib().ddp_hip_control_grav_cost_upload, "control_grav_cost_upload", arrs, first, count)

    def control_grav_cost(self, first=0, count=None):
        """(offset, weight) of instances first .. first + count - 1, each (count, T, m)"""
        per = (self.spec.T, self.spec.m)
        return self._cost_download(lib().ddp_hip_control_grav_cost_download, "control_grav_cost_download", (per, per), first, count)

    def set_aim_frames(self, frames):
        """The aim frames [(joint, off, axis), ...] (0 .. MAX_AIM_FRAMES of them; off: the eye, a point in the joint's
        coordinates; axis: a unit vector in the joint's axes) of a context created with FLAG_FRAME_AIM_COST (ddp_hip.h), shared
        by the batch.  With the same count and the same joints as before the per-instance data stays (points and axes may move),
        else targets, stand-offs and weights are reset to 0"""
        frames = list(frames)
        if any(len(f) != 3 for f in frames):
            raise ValueError("set_aim_frames: every frame is (joint, off, axis)")
        joint = np.ascontiguousarray([int(f[0]) for f in frames], dtype=np.int32)
        off = [np.asarray(f[1], dtype=np.float64) for f in frames]
        axis = [np.asarray(f[2], dtype=np.float64) for f in frames]
        if any(o.shape != (3,) for o in off + axis):
            raise ValueError("set_aim_frames: every off and every axis is a 3-vector")
        off, axis = _f64(off).reshape(-1), _f64(axis).reshape(-1)
        _check(lib().ddp_hip_frame_aim_set_frames(self._h, len(frames), joint.ctypes.data_as(_ip), _ptr(off), _ptr(axis)), "frame_aim_set_frames")
        self.n_aim_frames = len(frames)

    def set_frame_aim_cost(self, target=None, weight=None, first=0, count=None):
        """The frame-aiming terms of instances first .. first + count - 1 (a context created with FLAG_FRAME_AIM_COST; ddp_hip.h),
        of the F frames of set_aim_frames.  target: (g, rho), the world point the axis looks at and the stand-off >= 0, weight:
        (w_aim, w_range) >= 0; (T+1, F, 4) / (T+1, F, 2) for every instance of the range or (count, T+1, F, .) with one per
        instance; weight also takes (F, 2), (2,) and scalars by broadcast.  None leaves that side as it is.  The frame count is
        the one this object last passed to set_aim_frames; before that call there is no shape to check against and the call
        raises ValueError."""
        T1, F = self.spec.T + 1, getattr(self, "n_aim_frames", 0)
        if not F:
            raise ValueError("set_frame_aim_cost: no frames yet, call set_aim_frames first")
        count, arrs = self._cost_sides("set_frame_aim_cost", (("target", target, (T1, F, 4), ()), ("weight", weight, (T1, F, 2), ((F, 2), (2,), ()))),
                                       first, count)
        self._cost_upload(lib().ddp_hip_frame_aim_upload, "frame_aim_upload", arrs, first, count)

    def get_frame_aim_cost(self, first=0, count=None):
        """(target, weight) of instances first .. first + count - 1: (count, T+1, F, 4) and (count, T+1, F, 2)"""
        T1, F = self.spec.T + 1, getattr(self, "n_aim_frames", 0)    # (0 before set_aim_frames: empty arrays)
        return self._cost_download(lib().ddp_hip_frame_aim_download, "frame_aim_download", ((T1, F, 4), (T1, F, 2)), first, count)

    def frame_aim_error(self, which=0):
        """(batch, T+1, F, 2): (theta, l) of every aim frame along X (which = 0) or X_NEW (which = 1) against the resident targets,
        live weights or not: the angle between the axis and the line of sight in radians, and the distance to the target"""
        out = np.zeros((self.batch, self.spec.T + 1, getattr(self, "n_aim_frames", 0), 2))
        _check(lib().ddp_hip_frame_aim_error(self._h, int(which), _ptr(out)), "frame_aim_error")
        return out

    def set_balance_region_planes(self, n_planes):
        """The plane count (0 .. MAX_REGION_PLANES) of a context created with FLAG_BALANCE_REGION_COST (ddp_hip.h), shared by the
        batch.  With the same count as before the per-instance data stays, else geometry and weights are reset to 0; 0 takes the
        planes away"""
        _check(lib().ddp_hip_balance_region_set_planes(self._h, int(n_planes)), "balance_region_set_planes")
        self.n_region_planes = int(n_planes)

    def set_balance_region_cost(self, geom=None, weight=None, first=0, count=None):
        """The balance-region terms of instances first .. first + count - 1 (a context created with FLAG_BALANCE_REGION_COST;
        ddp_hip.h), of the P plane slots of set_balance_region_planes.  geom: (n, h, tau) -- a unit normal in world axes, the
        offset and the time constant >= 0 of the tested point c + tau cdot (free side n . xi - h >= 0) -- as (P, 5) for every
        instance and t, (T+1, P, 5) for every instance or (count, T+1, P, 5); weight: >= 0, as (P,), (T+1, P) or (count, T+1, P).
        None leaves that side as it is.  The plane count is the one this object last passed to set_balance_region_planes; before
        that call there is no shape to check against and the call raises ValueError."""
        T1, P = self.spec.T + 1, getattr(self, "n_region_planes", 0)
        if not P:
            raise ValueError("set_balance_region_cost: no planes yet, call set_balance_region_planes first")
        count, arrs = self._cost_sides("set_balance_region_cost", (("geom", geom, (T1, P, 5), ((P, 5),)), ("weight", weight, (T1, P), ((P,),))),
                                       first, count)
        self._cost_upload(lib().ddp_hip_balance_region_upload, "balance_region_upload", arrs, first, count)

    def get_balance_region_cost(self, first=0, count=None):
        """(geom, weight) of instances first .. first + count - 1: (count, T+1, P, 5) and (count, T+1, P)"""
        T1, P = self.spec.T + 1, getattr(self, "n_region_planes", 0)    # (0 before set_balance_region_planes: empty arrays)
        return self._cost_download(lib().ddp_hip_balance_region_download, "balance_region_download", ((T1, P, 5), (T1, P)), first, count)

    def balance_region_margin(self, which=0):
        """(batch, T+1): the least d_o = n . (c + tau cdot) - h over the planes of non-zero weight along X (which = 0) or X_NEW
        (which = 1); +inf where no plane is live, negative where the tested point has left the region"""
        out = np.zeros((self.batch, self.spec.T + 1))
        _check(lib().ddp_hip_balance_region_margin(self._h, int(which), _ptr(out)), "balance_region_margin")
        return out

    def set_joint_accel_cost(self, target=None, weight=None, first=0, count=None):
        """The joint-acceleration terms of instances first .. first + count - 1 (a context created with FLAG_JOINT_ACCEL_COST;
        ddp_hip.h): 1/2 sum_i w_i (a_i - target_i)^2 at t < T with a = aba(q_t, v_t, u_t), a free-flyer root's six rows included.
        target, weight: (T, nv) for every instance of the range or (count, T, nv) with one per instance; both also take (nv,)
        and scalars by broadcast.  weight >= 0.  None leaves that side as it is.  (The library's record has a row T that belongs
        to no term: the zero row is appended here, a (T+1, nv) array is refused.)"""
        per, extra = (self.spec.T, self.spec.nv), ((self.spec.nv,), ())
        count, arrs = self._cost_sides("set_joint_accel_cost", (("target", target, per, extra), ("weight", weight, per, extra)), first, count)
        arrs = [None if a is None else np.ascontiguousarray(np.concatenate([a, np.zeros((count, 1, self.spec.nv))], axis=1)) for a in arrs]
        self._cost_upload(lib().ddp_hip_joint_accel_cost_upload, "joint_accel_cost_upload", arrs, first, count)

    def joint_accel_cost(self, first=0, count=None):
        """(target, weight) of instances first .. first + count - 1, each (count, T, nv)"""
        per = (self.spec.T + 1, self.spec.nv)
        target, weight = self._cost_download(lib().ddp_hip_joint_accel_cost_download, "joint_accel_cost_download", (per, per), first, count)
        return np.ascontiguousarray(target[:, :-1]), np.ascontiguousarray(weight[:, :-1])

    def joint_accel(self, which=0):
        """(batch, T, nv): the accelerations a_t = aba(x_t, u_t) along X / U (which = 0) or X_NEW / U_NEW (which = 1) of a
        context created with FLAG_JOINT_ACCEL_COST, live weights or not ("how hard did it accelerate")"""
        out = np.zeros((self.batch, self.spec.T, self.spec.nv))
        _check(lib().ddp_hip_joint_accel(self._h, int(which), _ptr(out)), "joint_accel")
        return out

    def set_relative_frame_pairs(self, pairs):
        """The frame pairs [((joint_a, off_a), (joint_b, off_b)), ...] (1 .. MAX_FRAME_PAIRS of them, the two frames of a pair on
        different joints) of a context created with FLAG_RELATIVE_FRAME_COST (ddp_hip.h), shared by the batch: base frame A, tip
        frame B.  With the same count and the same joints as before the per-instance data stays (the points may move), else
        targets and weights are reset to 0 and the references to identity quaternions"""
        pairs = list(pairs)
        if any(len(p) != 2 or len(p[0]) != 2 or len(p[1]) != 2 for p in pairs):
            raise ValueError("set_relative_frame_pairs: every pair is ((joint_a, off_a), (joint_b, off_b))")
        ja = np.ascontiguousarray([int(p[0][0]) for p in pairs], dtype=np.int32)
        jb = np.ascontiguousarray([int(p[1][0]) for p in pairs], dtype=np.int32)
        offa = [np.asarray(p[0][1], dtype=np.float64) for p in pairs]
        offb = [np.asarray(p[1][1], dtype=np.float64) for p in pairs]
        if any(o.shape != (3,) for o in offa + offb):
            raise ValueError("set_relative_frame_pairs: every off is a 3-vector")
        offa, offb = _f64(offa).reshape(-1), _f64(offb).reshape(-1)
        _check(lib().ddp_hip_relative_frame_set_pairs(self._h, len(pairs), ja.ctypes.data_as(_ip), _ptr(offa), jb.ctypes.data_as(_ip),
                                                      _ptr(offb)), "relative_frame_set_pairs")
        self.n_frame_pairs = len(pairs)

    def set_relative_frame_cost(self, target=None, quat=None, weight=None, first=0, count=None):
        """The relative-frame terms of instances first .. first + count - 1 (a context created with FLAG_RELATIVE_FRAME_COST;
        ddp_hip.h), of the P pairs of set_relative_frame_pairs.  target: B's point as seen from A in A's joint axes, quat: B's
        axes as seen from A's as unit quaternions (x y z w), weight: three position axes, then three rotation axes, >= 0; each
        (T+1, P, 3 | 4 | 6) for every instance of the range or (count, T+1, P, .) with one per instance; weight also takes (P, 6),
        (6,) and scalars by broadcast.  None leaves that side as it is.  The pair count is the one this object last passed to
        set_relative_frame_pairs; before that call there is no shape to check against and the call raises ValueError."""
        T1, P = self.spec.T + 1, getattr(self, "n_frame_pairs", 0)
        if not P:
            raise ValueError("set_relative_frame_cost: no pairs yet, call set_relative_frame_pairs first")
        count, arrs = self._cost_sides("set_relative_frame_cost", (("target", target, (T1, P, 3), ()), ("quat", quat, (T1, P, 4), ()),
                                                                   ("weight", weight, (T1, P, 6), ((P, 6), (6,), ()))), first, count)
        if arrs[1] is not None and not bool(np.all(np.abs(np.sqrt(np.sum(arrs[1] ** 2, axis=-1)) - 1.0) <= 1e-10)):
            raise ValueError("set_relative_frame_cost quat: every quaternion has unit norm (to 1e-10)")
        self._cost_upload(lib().ddp_hip_relative_frame_upload, "relative_frame_upload", arrs, first, count)

    def relative_frame_cost(self, first=0, count=None):
        """(target, quat, weight) of instances first .. first + count - 1: (count, T+1, P, 3), (.., 4) and (.., 6)"""
        T1, P = self.spec.T + 1, getattr(self, "n_frame_pairs", 0)    # (0 before set_relative_frame_pairs: empty arrays)
        return self._cost_download(lib().ddp_hip_relative_frame_download, "relative_frame_download", ((T1, P, 3), (T1, P, 4), (T1, P, 6)),
                                   first, count)

    def relative_frame_error(self, which=0):
        """(batch, T+1, P, 6): the unweighted residual r = (r_pos, e_rot) of every pair along X (which = 0) or X_NEW (which = 1),
        against the resident targets and references, live weights or not"""
        out = np.zeros((self.batch, self.spec.T + 1, getattr(self, "n_frame_pairs", 0), 6))
        _check(lib().ddp_hip_relative_frame_error(self._h, int(which), _ptr(out)), "relative_frame_error")
        return out

    def set_obstacle_points(self, points, kinds):
        """The collision points [(joint, off, radius), ...] (up to MAX_COLLISION_POINTS spheres on the robot) and the kinds of the
        obstacle slots (OBSTACLE_SPHERE / OBSTACLE_HALFSPACE / OBSTACLE_GRID, up to MAX_OBSTACLES) of a context created with
        FLAG_OBSTACLE_COST (ddp_hip.h), shared by the batch.  OBSTACLE_GRID needs a resident grid (set_obstacle_grid or
        set_obstacle_occupancy first).  With the same counts and kinds as before the per-instance data stays, else it is reset"""
        joint = np.ascontiguousarray([int(p[0]) for p in points], dtype=np.int32)
        off = np.ascontiguousarray([p[1] for p in points], dtype=np.float64).reshape(-1)
        radius = np.ascontiguousarray([p[2] for p in points], dtype=np.float64)
        kind = np.ascontiguousarray([int(k) for k in kinds], dtype=np.int32)
        if off.size != 3 * len(joint):
            raise ValueError("set_obstacle_points: every point is (joint, (x, y, z), radius)")
        ip = C.POINTER(C.c_int32)
        _check(lib().ddp_hip_obstacle_set_points(self._h, len(joint), joint.ctypes.data_as(ip), _ptr(off), _ptr(radius), len(kind),
                                                 kind.ctypes.data_as(ip)), "obstacle_set_points")
        self.n_obstacles = len(kind)

    def set_obstacle_cost(self, geom=None, weight=None, first=0, count=None):
        """The obstacles of instances first .. first + count - 1 (a context created with FLAG_OBSTACLE_COST; ddp_hip.h), of the
        n_obs slots of set_obstacle_points.  geom: (c, rho) of a sphere, (n, h) of a half-space, (shift, margin) of a grid slot (the
        grid is seen displaced by shift; d = phi(p - shift) - r - margin), as (n_obs, 4) for every instance
        and t, (T+1, n_obs, 4) for every instance or (count, T+1, n_obs, 4); weight: >= 0, as (n_obs,), (T+1, n_obs) or
        (count, T+1, n_obs).  None leaves that side as it is.  The slot count is the one this object last passed to
        set_obstacle_points; before that call there is no shape to check against and the call raises ValueError."""
        T1, no = self.spec.T + 1, getattr(self, "n_obstacles", 0)
        if not no:
            raise ValueError("set_obstacle_cost: no obstacle slots yet, call set_obstacle_points first")
        count, arrs = self._cost_sides("set_obstacle_cost", (("geom", geom, (T1, no, 4), ((no, 4),)), ("weight", weight, (T1, no), ((no,),))),
                                       first, count)
        self._cost_upload(lib().ddp_hip_obstacle_upload, "obstacle_upload", arrs, first, count)

    def obstacle_cost(self, first=0, count=None):
        """(geom, weight) of instances first .. first + count - 1: (count, T+1, n_obs, 4) and (count, T+1, n_obs)"""
        T1, no = self.spec.T + 1, getattr(self, "n_obstacles", 0)               # (0 before set_obstacle_points: empty arrays)
        return self._cost_download(lib().ddp_hip_obstacle_download, "obstacle_download", ((T1, no, 4), (T1, no)), first, count)

    def obstacle_clearance(self, which=0):
        """(batch, T+1): the least signed distance of a collision point to an obstacle of non-zero weight along X (which = 0) or
        X_NEW (which = 1); +inf where no slot is live, negative where the robot penetrates"""
        out = np.zeros((self.batch, self.spec.T + 1))
        _check(lib().ddp_hip_obstacle_clearance(self._h, int(which), _ptr(out)), "obstacle_clearance")
        return out

    @staticmethod
    def _grid_args(who, field, origin, cell, dtype):
        """dims, origin and the C-contiguous field of a set_obstacle_grid / set_obstacle_occupancy call, shapes checked"""
        field = np.asarray(field)
        if field.ndim != 3:
            raise ValueError(f"{who}: the grid is an array of shape (nx, ny, nz), got {field.shape}")
        origin = np.ascontiguousarray(origin, dtype=np.float64)
        if origin.shape != (3,):
            raise ValueError(f"{who}: origin is (x, y, z), got shape {origin.shape}")
        if np.ndim(cell) != 0:
            raise ValueError(f"{who}: cell is one number, the node spacing on the three axes")
        return np.ascontiguousarray(field.shape, dtype=np.int32), origin, float(cell), np.ascontiguousarray(field, dtype=dtype)

    def set_obstacle_grid(self, phi, origin, cell):
        """The signed distance field of the OBSTACLE_GRID slots and the CAPSULE_VS_GRID pairs (a context created with
        FLAG_OBSTACLE_COST or FLAG_CAPSULE_COST; ddp_hip.h): phi of
        shape (nx, ny, nz), 2 <= n <= MAX_GRID_DIM, finite; origin the world position of node (0, 0, 0); cell > 0 the node
        spacing.  Replaces the resident grid, of whatever shape; waits for the context's stream"""
        dims, origin, cell, phi = self._grid_args("set_obstacle_grid", phi, origin, cell, np.float64)
        _check(lib().ddp_hip_obstacle_set_grid(self._h, dims.ctypes.data_as(_ip), _ptr(origin), cell, _ptr(phi)), "obstacle_set_grid")

    def set_obstacle_occupancy(self, occ, origin, cell):
        """The same from occupancy voxels occ of shape (nx, ny, nz), non-zero (or True) meaning occupied: the field is built on the
        device by an exact Euclidean distance transform, the surface halfway between a free voxel and its occupied neighbour"""
        occ = np.asarray(occ)
        if occ.dtype == np.bool_:
            occ = occ.view(np.uint8)
        elif occ.dtype != np.uint8:
            occ = (occ != 0).view(np.uint8)           # (a bool or uint8 array that is C-contiguous is passed as it is, no copy)
        dims, origin, cell, occ = self._grid_args("set_obstacle_occupancy", occ, origin, cell, np.uint8)
        _check(lib().ddp_hip_obstacle_set_occupancy(self._h, dims.ctypes.data_as(_ip), _ptr(origin), cell,
                                                    occ.ctypes.data_as(C.POINTER(C.c_uint8))), "obstacle_set_occupancy")

    def obstacle_grid(self):
        """(phi, origin, cell) of the resident grid: (nx, ny, nz), (3,) and a float"""
        dims, origin, cell = np.zeros(3, dtype=np.int32), np.zeros(3), C.c_double(0.0)
        _check(lib().ddp_hip_obstacle_grid_download(self._h, dims.ctypes.data_as(_ip), _ptr(origin), C.byref(cell), None), "obstacle_grid_download")
        phi = np.zeros(tuple(int(n) for n in dims))
        _check(lib().ddp_hip_obstacle_grid_download(self._h, dims.ctypes.data_as(_ip), _ptr(origin), C.byref(cell), _ptr(phi)), "obstacle_grid_download")
        return phi, origin, cell.value

    def obstacle_grid_query(self, points, grad=True):
        """phi at the world points (n, 3) by the device function the cost kernels use, and with grad its gradient (n, 3): +inf and
        a zero gradient outside the grid.  Returns phi, or (phi, grad)"""
        points = np.ascontiguousarray(points, dtype=np.float64)
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError(f"obstacle_grid_query: points is (n, 3), got {points.shape}")
        n = points.shape[0]
        val, g = np.zeros(n), (np.zeros((n, 3)) if grad else None)
        _check(lib().ddp_hip_obstacle_grid_query(self._h, n, _ptr(points), _ptr(val), _ptr(g) if grad else None), "obstacle_grid_query")
        return (val, g) if grad else val

    def obstacle_grid_segment_query(self, segments, n_intervals):
        """What the capsule cost sees along a limb: the rule of the CAPSULE_VS_GRID pairs (ddp_hip.h) on the world segments (n, 6)
        = (a0, a1), the shift already taken off, with n_intervals (one number or (n,), 0 .. CAPSULE_GRID_MAX_INTERVALS) intervals
        each, by the device routine the cost kernels use.  Returns (phi, j, point, grad): the least sample value (+inf: every
        sample outside the grid), its index j* (-1: every sample outside), the sample point (n, 3) and the gradient there (n, 3)"""
        segments = np.ascontiguousarray(segments, dtype=np.float64)
        if segments.ndim != 2 or segments.shape[1] != 6:
            raise ValueError(f"obstacle_grid_segment_query: segments is (n, 6), got {segments.shape}")
        n = segments.shape[0]
        if np.ndim(n_intervals) == 0:
            n_intervals = np.full(n, int(n_intervals))
        nint = np.ascontiguousarray(n_intervals, dtype=np.int32)
        if nint.shape != (n,):
            raise ValueError(f"obstacle_grid_segment_query: n_intervals is one number or ({n},), got {nint.shape}")
        val, j, point, g = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros((n, 3)), np.zeros((n, 3))
        _check(lib().ddp_hip_obstacle_grid_segment_query(self._h, n, _ptr(segments), nint.ctypes.data_as(_ip), _ptr(val), j.ctypes.data_as(_ip),
                                                         _ptr(point), _ptr(g)), "obstacle_grid_segment_query")
        return val, j, point, g

    def set_self_collision_pairs(self, points, pairs):
        """The spheres [(joint, off, radius), ...] (2 .. MAX_COLLISION_POINTS of them) and the pairs [(a, b), ...] of sphere indices
        (up to MAX_COLLISION_PAIRS, the two spheres of a pair on different joints) of a context created with
        FLAG_SELF_COLLISION_COST (ddp_hip.h), shared by the batch.  With the same pair list as before the per-instance data stays
        (points may move, radii may change), else margins and weights are reset to 0"""
        points, pairs = list(points), list(pairs)
        if any(len(p) != 3 for p in points) or any(len(p) != 2 for p in pairs):
            raise ValueError("set_self_collision_pairs: every point is (joint, (x, y, z), radius), every pair (a, b)")
        joint = np.ascontiguousarray([int(p[0]) for p in points], dtype=np.int32)
        off = np.ascontiguousarray([p[1] for p in points], dtype=np.float64).reshape(-1)
        radius = np.ascontiguousarray([p[2] for p in points], dtype=np.float64)
        if off.size != 3 * len(joint) or radius.shape != (len(joint),):
            raise ValueError("set_self_collision_pairs: every point is (joint, (x, y, z), radius)")
        pa = np.ascontiguousarray([int(p[0]) for p in pairs], dtype=np.int32)
        pb = np.ascontiguousarray([int(p[1]) for p in pairs], dtype=np.int32)
        _check(lib().ddp_hip_self_collision_set_pairs(self._h, len(joint), joint.ctypes.data_as(_ip), _ptr(off), _ptr(radius), len(pa),
                                                      pa.ctypes.data_as(_ip), pb.ctypes.data_as(_ip)), "self_collision_set_pairs")
        self.n_collision_pairs = len(pa)

    def set_self_collision_cost(self, margin=None, weight=None, first=0, count=None):
        """The self-collision terms of instances first .. first + count - 1 (a context created with FLAG_SELF_COLLISION_COST;
        ddp_hip.h), of the n_pairs pairs of set_self_collision_pairs.  margin: finite, may be negative; weight: >= 0; each as
        (n_pairs,) for every instance and t, (T+1, n_pairs) for every instance or (count, T+1, n_pairs).  None leaves that side
        as it is.  The pair count is the one this object last passed to set_self_collision_pairs; before that call there is no
        shape to check against and the call raises ValueError."""
        T1, npair = self.spec.T + 1, getattr(self, "n_collision_pairs", 0)
        if not npair:
            raise ValueError("set_self_collision_cost: no pairs yet, call set_self_collision_pairs first")
        count, arrs = self._cost_sides("set_self_collision_cost", (("margin", margin, (T1, npair), ((npair,),)),
                                                                   ("weight", weight, (T1, npair), ((npair,),))), first, count)
        self._cost_upload(lib().ddp_hip_self_collision_upload, "self_collision_upload", arrs, first, count)

    def self_collision_cost(self, first=0, count=None):
        """(margin, weight) of instances first .. first + count - 1, each (count, T+1, n_pairs)"""
        T1, npair = self.spec.T + 1, getattr(self, "n_collision_pairs", 0)      # (0 before set_self_collision_pairs: empty arrays)
        return self._cost_download(lib().ddp_hip_self_collision_download, "self_collision_download", ((T1, npair), (T1, npair)), first, count)

    def self_collision_clearance(self, which=0):
        """(batch, T+1): the least signed distance d_i of a pair of non-zero weight along X (which = 0) or X_NEW (which = 1);
        +inf where no pair is live, negative where two spheres are closer than their radii and margin allow"""
        out = np.zeros((self.batch, self.spec.T + 1))
        _check(lib().ddp_hip_self_collision_clearance(self._h, int(which), _ptr(out)), "self_collision_clearance")
        return out

    def set_capsule_pairs(self, capsules, pairs):
        """The robot capsules [(joint, end0, end1, radius), ...] (1 .. MAX_CAPSULES of them; end0 == end1 is a sphere) and the
        pairs [(a, kind, b), ...] (up to MAX_CAPSULE_PAIRS) of a context created with FLAG_CAPSULE_COST (ddp_hip.h), shared by the
        batch: body A of a pair is capsule a, body B robot capsule b on another joint (CAPSULE_VS_ROBOT), or a world capsule
        (CAPSULE_VS_CAPSULE) or a half-space (CAPSULE_VS_HALFSPACE) of the pair's own per-instance geometry, or the resident voxel
        grid (CAPSULE_VS_GRID: set_obstacle_grid or set_obstacle_occupancy first, which such a context accepts); b is then not read
        and (a, kind) is accepted.  Or an oriented box (CAPSULE_VS_BOX: b is the index of a shape of set_capsule_boxes, called
        first; the pose is the pair's own per-instance geometry).  With the same counts and kinds as before the per-instance data stays, else it is reset to 0"""
        capsules, pairs = list(capsules), list(pairs)
        if any(len(c) != 4 for c in capsules) or any(len(p) not in (2, 3) for p in pairs):
            raise ValueError("set_capsule_pairs: every capsule is (joint, (x, y, z), (x, y, z), radius), every pair (a, kind, b)")
        joint = np.ascontiguousarray([int(c[0]) for c in capsules], dtype=np.int32)
        end0 = np.ascontiguousarray([c[1] for c in capsules], dtype=np.float64).reshape(-1)
        end1 = np.ascontiguousarray([c[2] for c in capsules], dtype=np.float64).reshape(-1)
        radius = np.ascontiguousarray([c[3] for c in capsules], dtype=np.float64)
        if end0.size != 3 * len(joint) or end1.size != 3 * len(joint) or radius.shape != (len(joint),):
            raise ValueError("set_capsule_pairs: every capsule is (joint, (x, y, z), (x, y, z), radius)")
        pa = np.ascontiguousarray([int(p[0]) for p in pairs], dtype=np.int32)
        kind = np.ascontiguousarray([int(p[1]) for p in pairs], dtype=np.int32)
        pb = np.ascontiguousarray([int(p[2]) if len(p) == 3 else 0 for p in pairs], dtype=np.int32)
        _check(lib().ddp_hip_capsule_set_pairs(self._h, len(joint), joint.ctypes.data_as(_ip), _ptr(end0), _ptr(end1), _ptr(radius), len(pa),
                                               pa.ctypes.data_as(_ip), kind.ctypes.data_as(_ip), pb.ctypes.data_as(_ip)), "capsule_set_pairs")
        self.n_capsule_pairs = len(pa)

    def set_capsule_boxes(self, half):
        """The box shapes of the CAPSULE_VS_BOX pairs (a context created with FLAG_CAPSULE_COST; ddp_hip.h), shared by the batch: half
        of shape (n_boxes, 3), 0 .. MAX_CAPSULE_BOXES rows, the half extents along the box's own axes, each finite and > 0.  It may be
        called again (extents may change while the pairs stand), but not so as to leave a box pair without its shape"""
        half = np.ascontiguousarray(half, dtype=np.float64).reshape(-1, 3)
        _check(lib().ddp_hip_capsule_set_boxes(self._h, half.shape[0], _ptr(half) if half.size else None), "capsule_set_boxes")

    def set_capsule_cost(self, geom=None, weight=None, first=0, count=None):
        """The capsule terms of instances first .. first + count - 1 (a context created with FLAG_CAPSULE_COST; ddp_hip.h), of the
        n_pairs pairs of set_capsule_pairs.  geom: eight doubles per pair, the last the margin -- (., ., ., ., ., ., ., m) of a
        robot pair, (b0, b1, rho, m) of a world capsule, (n, h, ., ., ., m) of a half-space, (s, ., ., ., ., m) of a grid pair (the
        shift s of the grid as for an OBSTACLE_GRID slot; the capsule is sampled at its N + 1 material points, N from its length and
        the grid's cell, and the least trilinear value counts), (c, quaternion x y z w, m) of a box pair (the box's centre and its axes
        in the world, a unit quaternion) -- as (n_pairs, 8) for every instance
        and t, (T+1, n_pairs, 8) for every instance or (count, T+1, n_pairs, 8); weight: >= 0, as (n_pairs,), (T+1, n_pairs) or
        (count, T+1, n_pairs).  None leaves that side as it is.  The pair count is the one this object last passed to
        set_capsule_pairs; before that call there is no shape to check against and the call raises ValueError."""
        T1, npair = self.spec.T + 1, getattr(self, "n_capsule_pairs", 0)
        if not npair:
            raise ValueError("set_capsule_cost: no pairs yet, call set_capsule_pairs first")
        count, arrs = self._cost_sides("set_capsule_cost", (("geom", geom, (T1, npair, 8), ((npair, 8),)),
                                                            ("weight", weight, (T1, npair), ((npair,),))), first, count)
        self._cost_upload(lib().ddp_hip_capsule_upload, "capsule_upload", arrs, first, count)

    def capsule_cost(self, first=0, count=None):
        """(geom, weight) of instances first .. first + count - 1: (count, T+1, n_pairs, 8) and (count, T+1, n_pairs)"""
        T1, npair = self.spec.T + 1, getattr(self, "n_capsule_pairs", 0)        # (0 before set_capsule_pairs: empty arrays)
        return self._cost_download(lib().ddp_hip_capsule_download, "capsule_download", ((T1, npair, 8), (T1, npair)), first, count)

    def capsule_clearance(self, which=0):
        """(batch, T+1): the least signed distance d_i of a pair of non-zero weight along X (which = 0) or X_NEW (which = 1);
        +inf where no pair is live, negative where two bodies are closer than their radii and margin allow"""
        out = np.zeros((self.batch, self.spec.T + 1))
        _check(lib().ddp_hip_capsule_clearance(self._h, int(which), _ptr(out)), "capsule_clearance")
        return out

    def set_state_limits(self, lo=None, hi=None, weight=None, first=0, count=None):
        """The soft state limits of instances first .. first + count - 1 (a context created with FLAG_STATE_LIMITS; ddp_hip.h),
        over the tangent rows (n = 2 nv: configuration rows, then velocity rows): each of lo, hi, weight a scalar or an (n,)
        vector for every step, a (T+1, n) array for every instance of the range, or (count, T+1, n) with one per instance.
        -inf / +inf: no bound on that side.  None leaves that side as it is (the library then holds the side that arrives
        against the resident other one)."""
        per, extra = (self.spec.T + 1, self.spec.n), ((self.spec.n,), ())
        count, arrs = self._cost_sides("set_state_limits", (("lo", lo, per, extra), ("hi", hi, per, extra), ("weight", weight, per, extra)),
                                       first, count)
        if arrs[0] is not None and arrs[1] is not None and bool(np.any(arrs[0] > arrs[1])):
            raise ValueError("set_state_limits: some lo > hi")
        self._cost_upload(lib().ddp_hip_state_limits_upload, "state_limits_upload", arrs, first, count)

    def state_limits(self, first=0, count=None):
        """(lo, hi, weight) of instances first .. first + count - 1, each (count, T+1, n)"""
        per = (self.spec.T + 1, self.spec.n)
        return self._cost_download(lib().ddp_hip_state_limits_download, "state_limits_download", (per, per, per), first, count)

    def fill(self, name, value):
        _check(lib().ddp_hip_fill(self._h, SEQ[name], float(value)), f"fill {name}")

    def synchronize(self):
        _check(lib().ddp_hip_synchronize(self._h), "synchronize")

    def rollout(self):
        return _check(lib().ddp_hip_rollout(self._h), "rollout")

    def linearize(self, stages=None):
        if stages is None:
            return _check(lib().ddp_hip_linearize(self._h), "linearize")
        return _check(lib().ddp_hip_linearize_stages(self._h, stages), "linearize_stages")

    def backward(self, reg, mu, max_restarts=64):
        reg = _f64(np.broadcast_to(reg, (self.batch,))).copy()
        mu = _f64(np.broadcast_to(mu, (self.batch,))).copy()
        restarts = np.zeros(self.batch, dtype=np.int64)
        rc = _check(lib().ddp_hip_backward(self._h, _ptr(reg), _ptr(mu), restarts.ctypes.data_as(_lp), max_restarts),
                    "backward")
        return rc, reg, mu, restarts

    def forward(self, mu, n_alpha=8):
        mu = _f64(np.broadcast_to(mu, (self.batch,))).copy()
        step = np.zeros(self.batch)
        dcost = np.zeros(self.batch)
        rc = _check(lib().ddp_hip_forward(self._h, _ptr(mu), n_alpha, _ptr(step), _ptr(dcost)), "forward")
        return rc, step, dcost

    def cost_seq_aug(self, which, mu):
        mu = _f64(np.broadcast_to(mu, (self.batch,))).copy()
        return _check(lib().ddp_hip_cost_seq_aug(self._h, which, _ptr(mu)), "cost_seq_aug")

    def bwd_stream_bytes(self):
        return int(lib().ddp_hip_bwd_stream_bytes(self._h))

    def set_async(self, on=True):
        _check(lib().ddp_hip_set_async(self._h, 1 if on else 0), "set_async")

    def swap_traj(self):
        _check(lib().ddp_hip_swap_traj(self._h), "swap_traj")

    def advance(self, shift, x0=None, mode=ADVANCE_CLOSED_LOOP):
        """Moves the window on by `shift` steps on the resident data (ddp_hip_advance; ddp_hip.h): the trajectory, the gains and
        every per-step table of every instance, then the re-roll `mode` asks for.  x0: the measured states, (nx,) for every
        instance or (batch, nx); None: X[0] becomes the old X[shift].  shift in 1 .. T"""
        sp = self.spec
        if isinstance(shift, bool) or int(shift) != shift or not 1 <= int(shift) <= sp.T:
            raise ValueError(f"advance: shift {shift!r}, expected an integer in 1 .. {sp.T}")
        if mode not in (ADVANCE_NO_ROLL, ADVANCE_OPEN_LOOP, ADVANCE_CLOSED_LOOP):
            raise ValueError(f"advance: mode {mode!r}, expected ADVANCE_NO_ROLL, ADVANCE_OPEN_LOOP or ADVANCE_CLOSED_LOOP")
        if x0 is not None:
            x0 = np.asarray(x0, dtype=np.float64)
            if x0.shape not in ((sp.nx,), (self.batch, sp.nx)):
                raise ValueError(f"advance x0: shape {x0.shape}, expected {(sp.nx,)} or {(self.batch, sp.nx)}")
            x0 = np.ascontiguousarray(np.broadcast_to(x0, (self.batch, sp.nx)))
        return _check(lib().ddp_hip_advance(self._h, int(shift), _ptr(x0) if x0 is not None else None, int(mode)), "advance")

    def shard_pick(self, comm=None):
        """(best cost, global index) over every instance of every rank of `comm` (a Comm, or None: this context alone):
        the cost of the trajectory `forward` just produced; one 16-byte all-gather (ddp_hip_shard_pick)"""
        c, i = C.c_double(), C.c_int64()
        _check(lib().ddp_hip_shard_pick(comm._h if comm is not None else None, self._h, C.byref(c), C.byref(i)), "shard_pick")
        return c.value, i.value

    def shard_broadcast(self, best_global_index, dst_local=0, comm=None):
        """the winner's X, U, FB_* from its owner (rank = index mod G, local position index div G) into local instance
        dst_local of every rank (ddp_hip_shard_broadcast)"""
        _check(lib().ddp_hip_shard_broadcast(comm._h if comm is not None else None, self._h, int(best_global_index), int(dst_local)),
               "shard_broadcast")

    def update_origin(self, which):
        _check(lib().ddp_hip_update_origin(self._h, which), "update_origin")

    def optimality(self, mu):
        mu = _f64(np.broadcast_to(mu, (self.batch,))).copy()
        obj = np.zeros(self.batch)
        constr = np.zeros(self.batch)
        _check(lib().ddp_hip_optimality(self._h, _ptr(mu), _ptr(obj), _ptr(constr)), "optimality")
        return obj, constr

    def update_multipliers(self, mu):
        mu = _f64(np.broadcast_to(mu, (self.batch,))).copy()
        _check(lib().ddp_hip_update_multipliers(self._h, _ptr(mu)), "update_multipliers")

    def set_active(self, active=None):
        """active: [batch] of 0 / 1 (None = all): inactive instances are frozen (ddp_hip_set_active)"""
        if active is None:
            _check(lib().ddp_hip_set_active(self._h, None), "set_active")
            return
        a = np.ascontiguousarray(np.broadcast_to(active, (self.batch,)), dtype=np.int32)
        _check(lib().ddp_hip_set_active(self._h, a.ctypes.data_as(_ip)), "set_active")

    def solve(self, max_iterations, threshold, mu, reg, w, n, n_alpha=8, max_restarts=1000):
        """solve<M> (ddp.hpp:745-842) of every instance (ddp_hip_solve); returns (rc, dict of per-instance arrays)"""
        sp = SolverParams(int(max_iterations), float(threshold), float(mu), float(reg), float(w), float(n), int(n_alpha), 0,
                          int(max_restarts))
        logs = (SolveLog * self.batch)()
        rc = _check(lib().ddp_hip_solve(self._h, C.byref(sp), logs), "solve")
        out = {k: np.array([getattr(l, k) for l in logs]) for k, _ in SolveLog._fields_ if k != "pad_"}
        out["done"] = out["result"] == 1
        return rc, out

    def info(self):
        i = Info()
        _check(lib().ddp_hip_ctx_info(self._h, C.byref(i)), "ctx_info")
        return {k: getattr(i, k) for k, _ in Info._fields_}

    def profile_enable(self, on=True, kernels=None):
        """on: every kernel class; kernels: an iterable of K_* ids to bracket only those"""
        mask = (1 if on else 0) if kernels is None else sum(2 << k for k in kernels)
        _check(lib().ddp_hip_profile_enable(self._h, mask), "profile_enable")

    def profile_reset(self):
        _check(lib().ddp_hip_profile_reset(self._h), "profile_reset")

    def profile_get(self, kernel_id):
        ms = C.c_double()
        n = C.c_int64()
        _check(lib().ddp_hip_profile_get(self._h, kernel_id, C.byref(ms), C.byref(n)), "profile_get")
        return ms.value, n.value

    def bwd_algorithmic_bytes(self):
        return int(lib().ddp_hip_bwd_algorithmic_bytes(self._h))


class Comm:
    """The library's own RCCL communicator (csrc/comm.cpp).  `unique_id()` on rank 0, the 128 bytes travel to the other
    ranks by whatever means the host has (bench.py: torch.distributed), then Comm(uid, rank, nranks, device) on every rank."""

    @staticmethod
    def unique_id():
        uid = (C.c_ubyte * 128)()
        _check(lib().ddp_hip_comm_unique_id(uid), "comm_unique_id")
        return bytes(uid)

    def __init__(self, uid, rank, nranks, device):
        buf = (C.c_ubyte * 128)(*uid)
        self._h = C.c_void_p()
        _check(lib().ddp_hip_comm_init(buf, rank, nranks, device, C.byref(self._h)), "comm_init")
        self.rank, self.nranks = rank, nranks

    def best(self, cost, gidx):
        c, i = C.c_double(), C.c_int64()
        _check(lib().ddp_hip_shard_best(self._h, float(cost), int(gidx), C.byref(c), C.byref(i)), "shard_best")
        return c.value, i.value

    def close(self):
        if self._h:
            lib().ddp_hip_comm_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
