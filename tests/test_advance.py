"""The receding-horizon advance (ddp_hip_advance, Context.advance, solver.mpc_step): the window of everything a context holds per
time step moves on by s steps on the resident data, and the trajectory is re-rolled from the measured state.

The yardstick is np_advance below: the header's row rules applied to downloaded arrays.  Together with the existing entry points
(upload, rollout, forward(n_alpha=0), swap_traj) it is the composed path a caller had before, so every comparison is bit for bit
(np.array_equal on the raw doubles); there is no tolerance anywhere.

Shapes: T = 5, B = 3 (the middle instance catches instance-stride errors), s in {1, 2, T-1, T}: s = 1 is the overlap case of the
in-place walk, s = T-1 leaves one shifted row, s = T is all tail.  chain6ff has nx = 13 and n = 12 (an nx / n stride mix-up shows)
and takes the lane-per-rollout forward path, tree38 / tree38ff the latency path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import test_frame_cost as fc
import test_obstacle_cost as ob
import test_relative_frame_cost as rf
import test_tracking_cost as tc
from ddp_pinocchio_amd import capi, solver
from problems import make
from test_com_cost import make_any

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "host")
T, B = 5, 3
SHIFTS = (1, 2, T - 1, T)


# ---- the yardstick -------------------------------------------------------------------------------------------------------------
def np_advance(a, s, rule="hold", terminal=False):
    """a: (B, rows, ...), rows = the walked rows plus one terminal row where `terminal`.  hold: row[t] = old[t + s] while t + s is
    a walked row, the last walked row after; zero_tail: zeros after; zero: zeros everywhere.  A terminal row stays"""
    a = np.asarray(a)
    out = a.copy()
    R = a.shape[1] - (1 if terminal else 0)
    for t in range(R):
        if rule == "zero":
            out[:, t] = 0.0
        elif t + s < R:
            out[:, t] = a[:, t + s]
        elif rule == "zero_tail":
            out[:, t] = 0.0
        else:
            out[:, t] = a[:, R - 1]
    return out


def np_advance_x(X, s, x0=None):
    """the trajectory (B, T+1, nx): X[t] = old[t + s] for t <= T - s, old[T] after, then X[0] = x0"""
    out = np_advance(X, s)
    if x0 is not None:
        out[:, 0] = x0
    return out


def _x(ctx, name="X"):
    return ctx.download(name).reshape(ctx.batch, ctx.spec.T + 1, ctx.spec.nx)


def _u(ctx, name="U"):
    return ctx.download(name).reshape(ctx.batch, ctx.spec.T, ctx.spec.m)


def _unit(q):
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _random_states(o, rng, shape):
    x = rng.normal(size=shape + (o.nx,))
    if o.nq != o.nv:
        x[..., 3:7] = _unit(x[..., 3:7])
    return x


def _nudged(o, X, s, rng, size=1e-3):
    """the old X[s] of every instance moved by `size` in the tangent"""
    return np.stack([tc._integrate_x(o, X[b, s], size * rng.normal(size=o.n)) for b in range(X.shape[0])])


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_interface_constants_and_symbol():
    """the header and EXPORTS agree on the new name, the three modes are the header's, the ABI stays 3 and there are 40 sequences"""
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert re.search(r"\bint ddp_hip_advance\(ddp_hip_ctx\* ctx, int64_t shift, const double\* x0, int32_t mode\);", header)
    assert "ddp_hip_advance" in capi.EXPORTS and hasattr(capi.lib(), "ddp_hip_advance")
    modes = dict(re.findall(r"#define DDP_HIP_ADVANCE_(\w+)\s+(\d+)", header))
    assert modes == {"NO_ROLL": "0", "OPEN_LOOP": "1", "CLOSED_LOOP": "2"}
    assert (capi.ADVANCE_NO_ROLL, capi.ADVANCE_OPEN_LOOP, capi.ADVANCE_CLOSED_LOOP) == (0, 1, 2)
    assert re.search(r"#define DDP_HIP_ABI_VERSION 3\b", header) and capi.lib().ddp_hip_abi_version() == 3
    assert len(capi.SEQ_NAMES) == 40
    assert capi.lib().ddp_hip_advance(None, 1, None, 0) == capi.E_ARG


def test_advance_rejects_bad_arguments_without_a_device():
    """Context.advance checks shift, mode and the shape of x0 before the library is touched"""
    _, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx._h = spec, B, None
    for kw in (dict(shift=0), dict(shift=T + 1), dict(shift=-1), dict(shift=1.5), dict(shift=True), dict(shift=1, mode=3), dict(shift=1, mode=-1),
               dict(shift=1, x0=np.zeros(o.nx + 1)), dict(shift=1, x0=np.zeros(o.n)), dict(shift=1, x0=np.zeros((B + 1, o.nx))),
               dict(shift=1, x0=np.zeros((B, o.nx, 1))), dict(shift=1, x0=0.0)):
        with pytest.raises(ValueError):
            ctx.advance(**kw)


def test_advance_plan_host_logic():
    """host/test_advance_plan.cpp: the descriptors over every entry of kCostDesc, the row-source function, the kernel's in-place
    walk on host arrays against a copy-based shift for T in {1, 2, 5} and every s, and the argument checks"""
    subprocess.check_call(["make", "-s", "-C", HOST, "test_advance_plan"])
    out = subprocess.run([os.path.join(HOST, "test_advance_plan")], capture_output=True, text=True)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr


def test_yardstick_checks_itself():
    """advancing by a and then by b equals advancing by a + b on every hold and zero-tail rule (and on the trajectory); row T of a
    terminal-row array never moves; the rules in words on a small case"""
    rng = np.random.default_rng(1)
    for T_ in (1, 2, 5, 7):
        a_t = rng.normal(size=(B, T_, 4))           # T rows
        a_t1 = rng.normal(size=(B, T_ + 1, 3))      # T + 1 rows, the last the terminal cost
        X = rng.normal(size=(B, T_ + 1, 5))
        for a in range(1, T_ + 1):
            for b in range(1, T_ - a + 1):
                for rule in ("hold", "zero_tail", "zero"):
                    assert np.array_equal(np_advance(np_advance(a_t, a, rule), b, rule), np_advance(a_t, a + b, rule))
                    assert np.array_equal(np_advance(np_advance(a_t1, a, rule, True), b, rule, True), np_advance(a_t1, a + b, rule, True))
                assert np.array_equal(np_advance_x(np_advance_x(X, a), b), np_advance_x(X, a + b))
            for rule in ("hold", "zero_tail", "zero"):
                assert np.array_equal(np_advance(a_t1, a, rule, True)[:, T_], a_t1[:, T_])
    a = np.arange(5.0).reshape(1, 5, 1) + 1                       # rows 1 2 3 4 5
    assert np_advance(a, 2).ravel().tolist() == [3, 4, 5, 5, 5]
    assert np_advance(a, 2, "zero_tail").ravel().tolist() == [3, 4, 5, 0, 0]
    assert np_advance(a, 2, terminal=True).ravel().tolist() == [3, 4, 4, 4, 5]
    assert np_advance(a, 5).ravel().tolist() == [5, 5, 5, 5, 5] and np_advance(a, 4, terminal=True).ravel().tolist() == [4, 4, 4, 4, 5]
    assert np_advance_x(a, 4, x0=np.array([[9.0]])).ravel().tolist() == [9, 5, 5, 5, 5]


# ---- GPU: NO_ROLL, everything resident -----------------------------------------------------------------------------------------
def _everything_flags():
    return (capi.FLAG_NO_TENSORS | capi.FLAG_TRACKING_COST | capi.FLAG_CONTROL_BOUNDS | capi.FLAG_FRAME_COST | capi.FLAG_STATE_LIMITS |
            capi.FLAG_CONTROL_GRAV_COST | capi.FLAG_JOINT_ACCEL_COST | capi.FLAG_RELATIVE_FRAME_COST | capi.FLAG_OBSTACLE_COST)


_dp = C.POINTER(C.c_double)


def _joint_accel_raw(ctx):
    """the joint accelerations' record as the library holds it: (B, T+1, nv) each, row T included"""
    tgt, w = (np.zeros((ctx.batch, ctx.spec.T + 1, ctx.spec.nv)) for _ in range(2))
    assert capi.lib().ddp_hip_joint_accel_cost_download(ctx._h, tgt.ctypes.data_as(_dp), w.ctypes.data_as(_dp), 0, ctx.batch) == 0
    return tgt, w


def _upload_everything(ctx, model, o, rng):
    """valid random data, different in every (instance, t, item), in every table of _everything_flags()"""
    nv, n, m, ff = o.nv, o.n, o.m, o.nq != o.nv
    free = np.ones(n); free[:6 if ff else 0] = 0.0               # a free-flyer root's pose rows carry no limit
    freeu = np.ones(m); freeu[:6 if ff else 0] = 0.0             # ... and its six control rows no gravity term
    ctx.set_tracking_cost(xref=_random_states(o, rng, (B, T + 1)), wx=rng.uniform(0.1, 2, size=(B, T + 1, n)),
                          uref=rng.normal(size=(B, T, m)), wu=rng.uniform(0.1, 2, size=(B, T, m)))
    ctx.set_control_bounds(lo=-rng.uniform(1, 2, size=(B, T, m)), hi=rng.uniform(1, 2, size=(B, T, m)))
    ctx.set_frame_cost(frames=fc.pick_frames(model, 4)[:2], target=rng.normal(size=(B, T + 1, 2, 3)), weight=rng.uniform(0.1, 2, size=(B, T + 1, 2, 3)))
    lo = rng.normal(size=(B, T + 1, n)); hi = lo + rng.uniform(0.1, 1, size=lo.shape)
    lo[rng.uniform(size=lo.shape) < 0.2] = -np.inf; hi[rng.uniform(size=hi.shape) < 0.2] = np.inf       # three sides, infinite fills
    ctx.set_state_limits(lo=lo, hi=hi, weight=rng.uniform(0.1, 2, size=lo.shape) * free)
    ctx.set_control_grav_cost(offset=rng.normal(size=(B, T, m)), weight=rng.uniform(0.1, 2, size=(B, T, m)) * freeu)
    ctx.set_joint_accel_cost(target=rng.normal(size=(B, T, nv)), weight=rng.uniform(0.1, 2, size=(B, T, nv)))
    pairs = rf.pick_pairs(model)[:2]
    ctx.set_relative_frame_pairs(pairs)
    ctx.set_relative_frame_cost(target=rng.normal(size=(B, T + 1, 2, 3)), quat=_unit(rng.normal(size=(B, T + 1, 2, 4))),
                                weight=rng.uniform(0.1, 2, size=(B, T + 1, 2, 6)))
    kinds = (capi.OBSTACLE_SPHERE, capi.OBSTACLE_HALFSPACE, capi.OBSTACLE_SPHERE)                       # 3 slots of 8
    geom = rng.normal(size=(B, T + 1, 3, 4))
    geom[:, :, 0, 3] = np.abs(geom[:, :, 0, 3]); geom[:, :, 2, 3] = np.abs(geom[:, :, 2, 3])
    geom[:, :, 1, :3] = _unit(geom[:, :, 1, :3])
    ob.set_task(ctx, ob.pick_points(model), kinds, geom, rng.uniform(0.1, 2, size=(B, T + 1, 3)))


def _tables(ctx, everything):
    """name -> (array (B, rows, width), rule, terminal row) of every array the advance moves but X"""
    Bc, T_ = ctx.batch, ctx.spec.T

    def seq(name, rows):
        return ctx.download(name).reshape(Bc, rows, -1)
    d = {"U": (seq("U", T_), "hold", False), "FB_VAL": (seq("FB_VAL", T_), "zero", False), "FB_JAC": (seq("FB_JAC", T_), "zero_tail", False)}
    if not everything:
        return d
    for name in ("COST_XREF", "COST_WX"):
        d[name] = (seq(name, T_ + 1), "hold", True)
    for name in ("COST_UREF", "COST_WU", "CTRL_LO", "CTRL_HI"):
        d[name] = (seq(name, T_), "hold", False)
    blocks = {"frame": ctx.frame_cost(), "limits": ctx.state_limits(), "relative": ctx.relative_frame_cost(), "obstacle": ctx.obstacle_cost(),
              "accel": _joint_accel_raw(ctx)}
    for name, sides in blocks.items():
        for k, a in enumerate(sides):
            d[f"{name}{k}"] = (a.reshape(Bc, T_ + 1, -1), "hold", True)
    for k, a in enumerate(ctx.control_grav_cost()):                   # stage_only: T rows
        d[f"grav{k}"] = (a.reshape(Bc, T_, -1), "hold", False)
    return d


UNTOUCHED = ("LX", "LXX", "FX", "COSTS_OLD", "COSTS_NEW", "LFX")


@pytest.mark.gpu
@pytest.mark.parametrize("everything", [True, False])
@pytest.mark.parametrize("name", ["chain6ff", "tree38"])
def test_no_roll_moves_every_table(gpu, name, everything):
    """NO_ROLL with every table resident and random (and on a flag-free context): after the advance every array equals the
    yardstick, X_NEW / U_NEW equal X / U, FB_ORIGIN / MULT_ORIGIN equal X[:T], terminal rows and everything else are unchanged"""
    model, spec, o = make_any(name, T, batch=B, fd_mode=0, first_order_fd=0 if name.endswith("ff") else None)
    rng = np.random.default_rng(7)
    with capi.Context(spec, flags=_everything_flags() if everything else capi.FLAG_NO_TENSORS) as ctx:
        if everything:
            _upload_everything(ctx, model, o, rng)
            ctx.upload("BOX_STAT", rng.normal(size=(B, T * 2)))
        ctx.upload("X", _random_states(o, rng, (B, T + 1))); ctx.upload("U", rng.normal(size=(B, T, o.m)))
        ctx.upload("X_NEW", _random_states(o, rng, (B, T + 1))); ctx.upload("U_NEW", rng.normal(size=(B, T, o.m)))
        for s_ in ("FB_ORIGIN", "FB_VAL", "FB_JAC", "MULT_ORIGIN") + UNTOUCHED:
            ctx.upload(s_, rng.normal(size=(B, ctx.seq_size(s_))))
        ctx.set_active([1, 0, 1])                                     # the call applies to every instance all the same
        for s in SHIFTS:
            for with_x0 in (False, True):
                X0, before = _x(ctx), _tables(ctx, everything)
                keep = {k: ctx.download(k) for k in UNTOUCHED + (("BOX_STAT",) if everything else ())}
                x0 = _random_states(o, rng, (B,)) if with_x0 else None
                ctx.advance(s, x0, capi.ADVANCE_NO_ROLL)
                Xe = np_advance_x(X0, s, x0)
                assert np.array_equal(_x(ctx), Xe), (s, with_x0)
                after = _tables(ctx, everything)
                for k, (a, rule, terminal) in before.items():
                    assert np.array_equal(after[k][0], np_advance(a, s, rule, terminal)), (k, s, with_x0)
                    if terminal:
                        assert np.array_equal(after[k][0][:, -1], a[:, -1]), k
                assert not after["FB_VAL"][0].any() and not after["FB_JAC"][0][:, T - s:].any()
                assert np.array_equal(_x(ctx, "X_NEW"), Xe) and np.array_equal(_u(ctx, "U_NEW"), after["U"][0])
                for k in ("FB_ORIGIN", "MULT_ORIGIN"):
                    assert np.array_equal(ctx.download(k).reshape(B, T, o.nx), Xe[:, :T]), k
                for k, a in keep.items():
                    assert np.array_equal(ctx.download(k), a), k
                ctx.upload("FB_VAL", rng.normal(size=(B, T * o.m))); ctx.upload("FB_JAC", rng.normal(size=(B, T * o.m * o.n)))
        if everything:
            assert np.array_equal(_joint_accel_raw(ctx)[1][:, T], np.zeros((B, o.nv)))      # the zero-weight row T is still there


# ---- GPU: the two rolls ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("with_x0", [False, True])
@pytest.mark.parametrize("name", ["chain6ff", "tree38"])
def test_open_loop_equals_rollout(gpu, name, with_x0):
    """OPEN_LOOP: X / U equal those of a twin context given the yardstick's shifted X[0] and U and ctx.rollout()"""
    model, spec, o = make_any(name, T, batch=B, fd_mode=0, first_order_fd=0 if name.endswith("ff") else None)
    xs, us = tc._trajs(o, model, B, 11)
    rng = np.random.default_rng(12)
    with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx, capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as twin:
        for s in SHIFTS:
            tc._setup(ctx, xs, us)
            X0, U0 = _x(ctx), _u(ctx)
            x0 = _nudged(o, X0, s, rng) if with_x0 else None
            ctx.advance(s, x0, capi.ADVANCE_OPEN_LOOP)
            Xs = np_advance_x(X0, s, x0)
            Xs[:, 1:] = np.nan                                        # (the twin's rollout reads X[0] alone)
            twin.upload("X", Xs); twin.upload("U", np_advance(U0, s))
            twin.rollout()
            X1, U1 = _x(ctx), _u(ctx)
            assert np.array_equal(X1, _x(twin)) and np.array_equal(U1, _u(twin)), s
            assert np.array_equal(X1[:, 0], x0 if with_x0 else X0[:, s]) and np.all(np.isfinite(X1))
            assert np.array_equal(_x(ctx, "X_NEW"), X1) and np.array_equal(_u(ctx, "U_NEW"), U1)
            assert np.array_equal(ctx.download("FB_ORIGIN").reshape(B, T, o.nx), X1[:, :T])
            assert np.array_equal(ctx.download("MULT_ORIGIN").reshape(B, T, o.nx), X1[:, :T])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain6ff", "tree38ff"])
def test_closed_loop_equals_forward_and_swap(gpu, name):
    """CLOSED_LOOP with the gains a real linearize + backward left, x0 the old X[s] moved by 1e-3 in the tangent and instance 1
    frozen: X / U equal the composed path on a twin context -- uploads of the yardstick's X, U, FB_JAC, FB_VAL = 0 (and bounds),
    forward(n_alpha=0) with every instance active, swap_traj.  tree38ff: bounds drawn about the downloaded U, tight enough that
    some control of the re-roll sits on one (asserted)"""
    bounded = name == "tree38ff"
    flags = capi.FLAG_NO_TENSORS | capi.FLAG_TRACKING_COST | (capi.FLAG_CONTROL_BOUNDS if bounded else 0)
    model, spec, o = make_any(name, T, batch=B, fd_mode=0, first_order_fd=0)
    xs, us = tc._trajs(o, model, B, 21, held=True)
    ref = tc.random_ref(o, model, xs, us, B, 22)
    rng = np.random.default_rng(23)
    clamped = 0
    with capi.Context(spec, flags=flags) as ctx, capi.Context(spec, flags=flags) as twin:
        for s in SHIFTS:
            ctx.set_active(None)
            tc._setup(ctx, xs, us)
            tc.upload_ref(ctx, ref)
            if bounded:
                ctx.set_control_bounds(lo=-np.inf, hi=np.inf)
            ctx.linearize()
            rc, _, _, _ = ctx.backward(0.0, 1.0)
            assert rc == 0
            X0, U0, K0 = _x(ctx), _u(ctx), ctx.download("FB_JAC").reshape(B, T, -1)
            assert np.all(np.isfinite(K0)) and np.all(np.abs(K0).reshape(B, T, -1).max(axis=2) > 0)
            if bounded:
                lo, hi = U0 - rng.uniform(2e-4, 2e-3, size=U0.shape), U0 + rng.uniform(2e-4, 2e-3, size=U0.shape)
                ctx.set_control_bounds(lo=lo, hi=hi)
            x0 = _nudged(o, X0, s, rng)
            ctx.set_active([1, 0, 1])
            ctx.advance(s, x0, capi.ADVANCE_CLOSED_LOOP)
            # the composed path
            Xs = np_advance_x(X0, s, x0)
            twin.upload("X", Xs); twin.upload("U", np_advance(U0, s)); twin.upload("X_NEW", Xs); twin.upload("U_NEW", np_advance(U0, s))
            twin.upload("FB_JAC", np_advance(K0, s, "zero_tail")); twin.upload("FB_VAL", np.zeros((B, T * o.m)))
            tc.upload_ref(twin, ref)
            if bounded:
                twin.set_control_bounds(lo=np_advance(lo, s), hi=np_advance(hi, s))
            rc, step, _ = twin.forward(np.ones(B), n_alpha=0)
            assert rc == 0 and np.all(step == 1.0)
            twin.swap_traj()
            X1, U1 = _x(ctx), _u(ctx)
            assert np.array_equal(X1, _x(twin)) and np.array_equal(U1, _u(twin)), s
            assert np.array_equal(X1[:, 0], x0) and np.all(np.isfinite(X1)) and np.all(np.isfinite(U1))
            # (x_0 is X[0] itself, so the feedback acts from t = 1 on, through x_1 = f(x0, U[0]); with s >= T - 1 the gains of
            # t >= 1 are a tail's zeros and U stays the shifted U)
            if s < T - 1:
                assert not np.array_equal(U1[1], np_advance(U0, s)[1])    # the frozen instance was advanced and fed back like the others
            assert np.array_equal(_x(ctx, "X_NEW"), X1) and np.array_equal(_u(ctx, "U_NEW"), U1)
            assert np.array_equal(ctx.download("FB_ORIGIN").reshape(B, T, o.nx), X1[:, :T])
            if bounded:
                los, his = np_advance(lo, s), np_advance(hi, s)
                assert np.all(U1 >= los) and np.all(U1 <= his)
                clamped += int(np.sum((U1 == los) | (U1 == his)))
                print("closed loop", name, s, "controls on a bound", int(np.sum((U1 == los) | (U1 == his))), "of", U1.size)
    if bounded:
        assert clamped > 0                                            # the case does not pass vacuously


@pytest.mark.gpu
def test_twice_one_is_two(gpu):
    """from an X that ctx.rollout() made, advance(1, None, OPEN_LOOP) twice equals advance(2, None, OPEN_LOOP) once, on X, U and
    the cost tables"""
    name = "chain6ff"
    flags = capi.FLAG_NO_TENSORS | capi.FLAG_TRACKING_COST | capi.FLAG_FRAME_COST | capi.FLAG_CONTROL_GRAV_COST
    model, spec, o = make_any(name, T, batch=B, fd_mode=0, first_order_fd=0)
    xs, us = tc._trajs(o, model, B, 31)
    ref = tc.random_ref(o, model, xs, us, B, 32)
    rng = np.random.default_rng(33)
    frames = fc.pick_frames(model, 3)
    ftgt, fw = rng.normal(size=(B, T + 1, 3, 3)), rng.uniform(0.1, 2, size=(B, T + 1, 3, 3))
    goff, gw = rng.normal(size=(B, T, o.m)), rng.uniform(0.1, 2, size=(B, T, o.m))
    gw[:, :, :6] = 0.0
    got = []
    for shifts in ((1, 1), (2,)):
        with capi.Context(spec, flags=flags) as ctx:
            tc._setup(ctx, xs, us)
            tc.upload_ref(ctx, ref)
            ctx.set_frame_cost(frames=frames, target=ftgt, weight=fw)
            ctx.set_control_grav_cost(offset=goff, weight=gw)
            ctx.rollout()
            for s in shifts:
                ctx.advance(s, None, capi.ADVANCE_OPEN_LOOP)
            got.append({"X": _x(ctx), "U": _u(ctx), **{k: ctx.download(k) for k in ("COST_XREF", "COST_WX", "COST_UREF", "COST_WU")},
                        "frame": np.stack(ctx.frame_cost()), "grav": np.stack(ctx.control_grav_cost())})
    for k in got[0]:
        assert np.array_equal(got[0][k], got[1][k]), k
    assert np.array_equal(got[1]["frame"], np.stack([np_advance(ftgt, 2, terminal=True), np_advance(fw, 2, terminal=True)]))
    assert np.array_equal(got[1]["U"], np_advance(us.reshape(B, T, o.m), 2))


# ---- GPU: refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_write_nothing(gpu):
    """s = 0, s = T + 1, mode 3, a NaN in x0 and a non-unit root quaternion are DDP_HIP_E_ARG, a context with constraint rows
    DDP_HIP_E_UNSUPPORTED; after each refusal a download shows that nothing was written"""
    L = capi.lib()
    model, spec, o = make_any("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    xs, us = tc._trajs(o, model, B, 41)
    rng = np.random.default_rng(42)
    names = ("X", "U", "X_NEW", "U_NEW", "FB_ORIGIN", "FB_VAL", "FB_JAC", "MULT_ORIGIN", "COST_XREF", "COST_WX", "COST_UREF", "COST_WU")

    def unchanged(ctx, snap):
        return all(np.array_equal(ctx.download(k), v) for k, v in snap.items())
    with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | capi.FLAG_TRACKING_COST) as ctx:
        tc._setup(ctx, xs, us)
        tc.upload_ref(ctx, tc.random_ref(o, model, xs, us, B, 43))
        for k in ("FB_ORIGIN", "FB_VAL", "FB_JAC", "MULT_ORIGIN"):
            ctx.upload(k, rng.normal(size=(B, ctx.seq_size(k))))
        snap = {k: ctx.download(k) for k in names}
        good = np.ascontiguousarray(xs.reshape(B, T + 1, o.nx)[:, 1])
        ptr = good.ctypes.data_as(_dp)
        for shift, mode in ((0, 0), (T + 1, 0), (-1, 2), (1, 3), (1, -1)):
            assert L.ddp_hip_advance(ctx._h, shift, ptr, mode) == capi.E_ARG, (shift, mode)
            assert L.ddp_hip_advance(ctx._h, shift, None, mode) == capi.E_ARG, (shift, mode)
            assert unchanged(ctx, snap)
        bad = good.copy(); bad[B - 1, o.nx - 1] = np.nan
        quat = good.copy(); quat[1, 3:7] *= 1.0 + 1e-9
        for x0 in (bad, quat):
            for mode in (capi.ADVANCE_NO_ROLL, capi.ADVANCE_OPEN_LOOP, capi.ADVANCE_CLOSED_LOOP):
                with pytest.raises(capi.DdpHipError) as e:
                    ctx.advance(1, x0, mode)
                assert e.value.code == capi.E_ARG
                assert unchanged(ctx, snap)
        ctx.advance(1, good, capi.ADVANCE_NO_ROLL)                    # ... and the good arguments are taken
        assert not unchanged(ctx, snap)
    model, spec, o = make("chain6", T, batch=B, fd_mode=0)            # config constraint at every step
    xs, us = tc._trajs(o, model, B, 44)
    with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
        tc._setup(ctx, xs, us, tc._mults(o, xs[0], 45), o.Etot)
        snap = {k: ctx.download(k) for k in ("X", "U", "X_NEW", "U_NEW", "MULT_ORIGIN", "MULT_VAL", "MULT_JAC")}
        for mode in (capi.ADVANCE_NO_ROLL, capi.ADVANCE_OPEN_LOOP, capi.ADVANCE_CLOSED_LOOP):
            with pytest.raises(capi.DdpHipError) as e:
                ctx.advance(1, None, mode)
            assert e.value.code == capi.E_UNSUPPORTED
            assert unchanged(ctx, snap)


# ---- GPU: the loop runs ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mpc_loop_runs(gpu):
    """chain6ff, T = 8, B = 2, tracking towards a posture: solve, solver.mpc_step(shift=1, x0=None), solve.  X[0] is the old X[1] bit
    for bit, the logs carry valid result codes, every trajectory is finite, and mpc_step equals advance followed by solve on a twin"""
    T_, B_ = 8, 2
    model, spec, o = make_any("chain6ff", T_, batch=B_, fd_mode=0, first_order_fd=0)
    xs, us = tc._trajs(o, model, B_, 51, held=True)
    rng = np.random.default_rng(52)
    posture = np.stack([tc._integrate_x(o, xs[b].reshape(T_ + 1, o.nx)[0], np.concatenate([0.2 * rng.normal(size=o.nv), np.zeros(o.nv)]))
                        for b in range(B_)])
    wx = np.concatenate([np.full(o.nv, 20.0), np.full(o.nv, 1.0)])
    args = dict(max_iterations=6, threshold=1e-9, mu=1e2, reg=0.0, w=1e-1, n=10.0)
    flags = capi.FLAG_NO_TENSORS | capi.FLAG_TRACKING_COST
    out = []
    for use_mpc_step in (True, False):
        with capi.Context(spec, flags=flags) as ctx:
            tc._setup(ctx, xs, us)
            ctx.upload("MULT_ORIGIN", xs[:, :T_ * o.nx])
            ctx.set_tracking_cost(xref=np.broadcast_to(posture[:, None, :], (B_, T_ + 1, o.nx)), wx=wx[None, :] * np.ones((T_ + 1, 1)))
            log0 = solver.solve(ctx, **args)
            X1 = _x(ctx)
            if use_mpc_step:
                log1 = solver.mpc_step(ctx, 1, None, None, **args)
            else:
                ctx.advance(1, None, capi.ADVANCE_CLOSED_LOOP)
                log1 = solver.solve(ctx, **args)
            log2 = solver.solve(ctx, **args)
            X2, U2 = _x(ctx), _u(ctx)
            for lg in (log0, log1, log2):
                assert set(np.unique(lg["result"])) <= {0, 1} and np.all(lg["iterations"] >= 0) and np.all(lg["iterations"] <= args["max_iterations"])
            print("mpc loop", "mpc_step" if use_mpc_step else "advance + solve", "iterations", log0["iterations"], log1["iterations"], log2["iterations"])
            assert np.array_equal(X2[:, 0], X1[:, 1])
            assert np.all(np.isfinite(X1)) and np.all(np.isfinite(X2)) and np.all(np.isfinite(U2))
            out.append((X2, U2, log1["iterations"], log1["result"]))
    for a, b in zip(*out):
        assert np.array_equal(a, b)
