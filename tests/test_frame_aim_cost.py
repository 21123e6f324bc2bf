"""Per-instance frame-aiming costs (DDP_HIP_FLAG_FRAME_AIM_COST, include/ddp_hip/ddp_hip.h): aim frame i is a joint j, a point off
of it (the eye) and a unit axis a of its axes; with p the point's world position, n = R_j a and a target g with a stand-off rho,

    d = g - p,  l = |d|,  dh = d / l,   r_aim = n - dh,   r_range = l - rho,   l += 1/2 sum_i (w_aim |r_aim|^2 + w_range r_range^2)

and a frame whose l <= 1e-12 forms nothing.  The oracle has no such cost, so the yardstick is the numpy restatement below, built on
Oracle.frame_position and Oracle.frame_jacobian(world_aligned=True) (the point jacobian P) and test_frame_orient_cost.py's frame_R /
frame_W (the world angular jacobian W):  J_aim = -[n]x W + (I - dh dh^T) P / l,  J_range = -dh^T P, exact zero off path(j).  The
other helpers are test_relative_frame_cost.py's, test_frame_orient_cost.py's and test_frame_vel_cost.py's, reused by import.

Tolerances are those of the same comparisons in the neighbouring files: TOL_FD (yardstick against differences), TOL_LIN (linearise,
cost values, the readback), TOL_FWD (forward against the emulation), TOL_SWEEP (stepwise sweep).

check_task asserts on the yardstick alone that every live frame has 0.3 <= l <= 2 and 0.1 <= theta <= 2.5."""
import os
import re
import subprocess

import numpy as np
import pytest

import test_com_cost as cm
import test_control_grav_cost as cg
import test_frame_cost as fc
import test_frame_orient_cost as fo
import test_frame_vel_cost as fv
import test_momentum_cost as mo
import test_obstacle_cost as ob
import test_relative_frame_cost as rf
import test_self_collision_cost as sc
import test_state_limits as sl
import test_tracking_cost as tc
from problems import make
from synth import rel_err, stepwise_backward_check

ROOT = rf.ROOT
H = rf.H                       # 1e-3, the step of the 5-point central differences
W5 = rf.W5
DERIVS = fc.DERIVS
NAMES = fc.NAMES
make_any = cm.make_any
_trajs, _setup = tc._trajs, tc._setup
frame_R, frame_W = fo.frame_R, fo.frame_W
_emulate_forward = ob._emulate_forward
rand_q = rf.rand_q
TOL_FD = 1e-8                  # the neighbours' test_yardstick_gradient
TOL_LIN = 1e-12                # ... test_linearize_matches_definition, test_cost_seq_aug
TOL_FWD = 1e-9                 # ... test_forward_matches_emulation
TOL_SWEEP = 1e-10              # ... the stepwise sweep check
TOL_HOLD = 1e-12               # the issue's: "uploading g = p + n l0 with rho = l0 leaves |r| <= 1e-12", and the readback's
MIN_RANGE = 1e-12              # the header's: a line of sight no longer than this forms nothing

OFFS = [(0.1, -0.05, 0.2), (0.02, 0.04, 0.15), (-0.06, 0.03, 0.05), (0.04, 0.07, -0.02)]
AXES = [(1.0, 0.0, 0.0), (0.0, 0.6, -0.8), (0.0, 0.0, -1.0), (0.48, -0.6, 0.64)]


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def pick_aim_frames(model):
    """Four frames (joint, off, axis): a leaf, a mid-chain joint of its path, a leaf of a second branch (on a chain: the leaf's
    parent), and a second frame on the first leaf with another eye and another axis"""
    parent = [int(p) for p in model.parent]
    nj = len(parent)
    depth = [0] * nj
    for j in range(nj):
        depth[j] = depth[parent[j]] + 1 if parent[j] >= 0 else 0
    leaves = sorted((j for j in range(nj) if j not in parent), key=lambda j: (-depth[j], j))
    leaf = leaves[0]
    path = fv.path_of(model, leaf)
    mid = path[len(path) // 2]
    other = leaves[1] if len(leaves) > 1 else parent[leaf]
    joints = [leaf, mid, other, leaf]
    for a in AXES:
        assert abs(np.linalg.norm(a) - 1.0) <= 1e-12
    return [(j, OFFS[k], AXES[k]) for k, j in enumerate(joints)]


def path_cols(model, j):
    return [c for i in fv.path_of(model, j) for c in fv.cols_of(model, i)]


def eye_axis(o, frame, q):
    """(p, n): the eye's world position and the axis' world direction"""
    j, off, a = frame
    return o.frame_position(j, off, q), frame_R(o, j, q) @ np.asarray(a)


def sight(p, g):
    """(dh, l), or (None, l) where l <= MIN_RANGE"""
    d = g[:3] - p
    l = float(np.linalg.norm(d))
    return (d / l if l > MIN_RANGE else None), l


def residual(o, frame, q, g):
    """r = (r_aim, r_range) and (theta, l); None where the line of sight is degenerate"""
    p, n = eye_axis(o, frame, q)
    dh, l = sight(p, g)
    if dh is None:
        return None, (0.0, l)
    theta = float(np.arctan2(np.linalg.norm(np.cross(n, dh)), n @ dh))
    return np.concatenate([n - dh, [l - g[3]]]), (theta, l)


def pn_J(o, model, frame, q):
    """[dp; dn] / d(delta q) (6, nv): the point jacobian and -[n]x W, the columns off the path exact zero"""
    j, off, a = frame
    R = frame_R(o, j, q)
    n = R @ np.asarray(a)
    cols = path_cols(model, j)
    J = np.zeros((6, o.nv))
    J[:3, cols] = o.frame_jacobian(j, off, q, world_aligned=True)[:, cols]
    J[3:, cols] = np.cross(frame_W(o, j, q, R)[:, cols], n[:, None], axis=0)       # w x n per column
    return J, cols


def fa_J(o, model, frame, q, g):
    """J = [J_aim; J_range] (4, nv) at q, the columns off the path exact zero; and the path's columns"""
    p, n = eye_axis(o, frame, q)
    dh, l = sight(p, g)
    Jpn, cols = pn_J(o, model, frame, q)
    J = np.zeros((4, o.nv))
    J[:3] = Jpn[3:] + (np.eye(3) - np.outer(dh, dh)) @ Jpn[:3] / l
    J[3] = -dh @ Jpn[:3]
    return J, cols


def fa_term(o, frames, q, g_t, w_t):
    """1/2 sum_i (w_aim |r_aim|^2 + w_range r_range^2) at one configuration, frames ascending; a frame whose two weights are 0 is
    not walked, a degenerate one forms nothing"""
    s = 0.0
    for i, frame in enumerate(frames):
        if not np.any(w_t[i] != 0.0):
            continue
        r, _ = residual(o, frame, q, g_t[i])
        if r is None:
            continue
        s += 0.5 * (w_t[i][0] * np.sum(r[:3] ** 2) + w_t[i][1] * r[3] ** 2)
    return s


def fa_terms(o, frames, xs, g, w):
    X = xs.reshape(o.T + 1, o.nx)
    return np.array([fa_term(o, frames, X[t][:o.nq], g[t], w[t]) for t in range(o.T + 1)])


def fa_errors(o, frames, xs, g):
    X = xs.reshape(o.T + 1, o.nx)
    return np.array([[residual(o, frame, X[t][:o.nq], g[t][i])[1] for i, frame in enumerate(frames)] for t in range(o.T + 1)])


def fa_grad_hess(o, model, frames, x, g_t, w_t):
    """(lx, lxx) contributions at one state and the tangent rows of the live frames' paths (a mask over n)"""
    nv, n = o.nv, o.n
    gr, Hm, rows = np.zeros(n), np.zeros((n, n)), np.zeros(n, dtype=bool)
    q = x[:o.nq]
    for i, frame in enumerate(frames):
        if not np.any(w_t[i] != 0.0):
            continue
        r, _ = residual(o, frame, q, g_t[i])
        if r is None:
            continue
        J, cols = fa_J(o, model, frame, q, g_t[i])
        rows[cols] = True
        w4 = np.array([w_t[i][0]] * 3 + [w_t[i][1]])
        gr[:nv] += J.T @ (w4 * r)
        for a in range(4):                               # entry (i, j) and (j, i) alike: symmetric bit for bit
            Hm[:nv, :nv] += w4[a] * np.outer(J[a], J[a])
    return gr, Hm, rows


def fa_derivs(o, model, frames, xs, g, w):
    X = xs.reshape(o.T + 1, o.nx)
    out = {"LX": [], "LXX": [], "rows": []}
    for t in range(o.T + 1):
        gr, Hm, rows = fa_grad_hess(o, model, frames, X[t], g[t], w[t])
        out["rows"].append(rows)
        if t == o.T:
            out["LFX"], out["LFXX"] = gr, Hm.ravel(order="F")
        else:
            out["LX"].append(gr); out["LXX"].append(Hm.ravel(order="F"))
    out["LX"], out["LXX"] = np.concatenate(out["LX"]), np.concatenate(out["LXX"])
    return out


def random_task(o, frames, xs, B, seed, wscale=1.0, lo=0.1, hi=2.5):
    """targets (B, T+1, F, 4): g at distance l in [0.3, 2] from the present eye, in a direction theta in [lo, hi] off the present
    axis; rho = l +- 1 .. 10 cm; weights (B, T+1, F, 2) > 0"""
    rng = np.random.default_rng(seed)
    T, F = o.T, len(frames)
    g = np.zeros((B, T + 1, F, 4))
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            for i, frame in enumerate(frames):
                p, n = eye_axis(o, frame, X[t][:o.nq])
                u = np.cross(n, rng.normal(size=3))
                u /= np.linalg.norm(u)
                th, l = rng.uniform(lo, hi), rng.uniform(0.3, 2.0)
                g[b, t, i, :3] = p + l * (np.cos(th) * n + np.sin(th) * u)
                g[b, t, i, 3] = l + rng.uniform(0.01, 0.1) * rng.choice([-1.0, 1.0])
    return g, wscale * rng.uniform(0.1, 2.0, size=(B, T + 1, F, 2))


def check_task(o, frames, xs, g, w, lo=0.1, hi=2.5):
    """the conditions on the inputs, on the yardstick alone; returns which (instance, t) blocks carry a weight"""
    B, T = xs.shape[0], o.T
    live = np.zeros((B, T + 1), dtype=bool)
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            for i, frame in enumerate(frames):
                if not np.any(w[b, t, i] != 0.0):
                    continue
                live[b, t] = True
                _, (theta, l) = residual(o, frame, X[t][:o.nq], g[b, t, i])
                assert 0.3 - 1e-9 <= l <= 2.0 + 1e-9, (b, t, i, l)
                assert lo - 1e-9 <= theta <= hi + 1e-9, (b, t, i, theta)
                assert g[b, t, i, 3] >= 0.0
    return live


def set_task(ctx, frames, g=None, w=None):
    ctx.set_aim_frames(frames)
    if g is not None or w is not None:
        ctx.set_frame_aim_cost(target=g, weight=w)


# ---- CPU: the yardstick checks itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain6", "tree38", "chain6ff", "tree38ff", "table7"])
def test_yardstick_gradient(name):
    """J against the 5-point central difference of r along q (+) (+-h e_c) over all nv columns, [dp; dn] alike; columns off the
    path exact zero in the yardstick and zero within the tolerance in the differences.  lx against the central difference of the
    term; the Gauss-Newton block symmetric bit for bit, its least eigenvalue >= -1e-12 of its largest entry, zero velocity rows
    and columns and zero rows off the live frames' paths"""
    T = 2
    model, _, o = make_any(name, T, fd_mode=0)
    frames = pick_aim_frames(model)
    assert len(frames) == 4 and frames[0][0] == frames[3][0]
    xs, us = _trajs(o, model, 1, 3)
    g, w = random_task(o, frames, xs, 1, 4)
    check_task(o, frames, xs, g, w)
    X = xs[0].reshape(T + 1, o.nx)
    nv, n = o.nv, o.n
    for t in (1, T):
        q = X[t][:o.nq]
        for i, frame in enumerate(frames):
            J, cols = fa_J(o, model, frame, q, g[0, t, i])
            Jpn, _ = pn_J(o, model, frame, q)
            off = [c for c in range(nv) if c not in cols]
            assert cols and np.all(J[:, off] == 0.0) and np.all(Jpn[:, off] == 0.0)
            fd, fdpn = np.zeros((4, nv)), np.zeros((6, nv))
            for c in range(nv):
                e = np.zeros(nv); e[c] = H
                for s, cw in W5:
                    qs = o.integrate(q, s * e)
                    fd[:, c] += cw * residual(o, frame, qs, g[0, t, i])[0] / H
                    fdpn[:, c] += cw * np.concatenate(eye_axis(o, frame, qs)) / H
            scale = max(1.0, np.max(np.abs(J)))
            print("yardstick", name, t, i, np.max(np.abs(fd - J)), np.max(np.abs(fdpn - Jpn)))
            assert np.max(np.abs(fd - J)) <= TOL_FD * scale, (i, np.max(np.abs(fd - J)))
            assert np.max(np.abs(fdpn - Jpn)) <= TOL_FD * max(1.0, np.max(np.abs(Jpn))), (i, np.max(np.abs(fdpn - Jpn)))
            assert np.max(np.abs(fd[:, off])) <= TOL_FD * scale if off else True
        gr, Hm, rows = fa_grad_hess(o, model, frames, X[t], g[0, t], w[0, t])
        assert np.max(np.abs(gr[:nv])) > 0 and rows.any()

        def cost_at(dx):
            return fa_term(o, frames, tc._integrate_x(o, X[t], dx)[:o.nq], g[0, t], w[0, t])
        fd = np.zeros(n)
        for c in range(n):
            e = np.zeros(n); e[c] = H
            fd[c] = sum(cw * cost_at(s * e) for s, cw in W5) / H
        assert np.max(np.abs(fd - gr)) <= TOL_FD * max(1.0, np.max(np.abs(gr))), np.max(np.abs(fd - gr))
        assert np.array_equal(Hm, Hm.T)
        assert np.all(Hm[nv:, :] == 0.0) and np.all(Hm[:, nv:] == 0.0) and np.all(gr[nv:] == 0.0)
        assert np.all(gr[~rows] == 0.0) and np.all(Hm[~rows, :] == 0.0)
        assert np.min(np.linalg.eigvalsh(Hm)) >= -1e-12 * np.max(np.abs(Hm))


def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.FLAG_FRAME_AIM_COST == 16384 and re.search(r"#define\s+DDP_HIP_FLAG_FRAME_AIM_COST\s+16384u", header)
    assert capi.MAX_AIM_FRAMES == 4 and re.search(r"#define\s+DDP_HIP_MAX_AIM_FRAMES\s+4\b", header)
    L = capi.lib()
    for name in ("ddp_hip_frame_aim_set_frames", "ddp_hip_frame_aim_upload", "ddp_hip_frame_aim_download", "ddp_hip_frame_aim_error",
                 "ddp_hip_model_frame_axis"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    for name in ("set_aim_frames", "set_frame_aim_cost", "get_frame_aim_cost", "frame_aim_error"):
        assert hasattr(capi.Context, name), name
    assert hasattr(capi.ModelHandle, "frame_axis")
    assert "l <= 1e-12" in header                                    # the degenerate line of sight is stated
    # shapes are checked before anything reaches the library: a context object without a device will do
    T, B, F = 5, 2, 3
    model, spec, _ = make("chain6", T, batch=B, fd_mode=0)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx._h, ctx.n_aim_frames = spec, B, None, 0
    with pytest.raises(ValueError, match="set_aim_frames"):
        ctx.set_frame_aim_cost(weight=np.zeros(2))
    ctx.n_aim_frames = F
    for kw in (dict(target=np.zeros((T, F, 4))), dict(target=np.zeros((T + 1, F + 1, 4))), dict(target=np.zeros((T + 1, F, 3))),
               dict(target=np.zeros(4)), dict(target=np.zeros((B + 1, T + 1, F, 4))), dict(target=np.zeros((B, T + 1, F, 4)), count=1),
               dict(weight=np.zeros((T + 1, F))), dict(weight=np.zeros(3)), dict(weight=np.zeros((F + 1, 2))),
               dict(weight=np.zeros((T + 1, F, 3))), dict(weight=np.zeros((B + 1, T + 1, F, 2))),
               dict(target=np.zeros((T + 1, F, 4)), weight=np.zeros((T + 1, F + 1, 2)))):
        with pytest.raises(ValueError):
            ctx.set_frame_aim_cost(**kw)
    off, ax = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)
    for bad in ([(0, off)], [(0, (0.0, 0.0), ax)], [(0, off, (1.0, 0.0))], [(0, off, ax, 1.0)], [0]):
        with pytest.raises((ValueError, TypeError)):
            ctx.set_aim_frames(bad)


def test_frame_aim_block_host_logic():
    """host/test_frame_aim_block.cpp: the term's record and index, the frame-list rules with the unit axis, and what an upload of
    targets, stand-offs and weights decides (csrc/cost_block.h), which need no device"""
    host = os.path.join(ROOT, "host")
    subprocess.check_call(["make", "-s", "-C", host, "test_frame_aim_block"])
    out = subprocess.run([os.path.join(host, "test_frame_aim_block")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def FLAG(capi):
    return capi.FLAG_FRAME_AIM_COST


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,fd_mode,fo_,fwd_path", [
    ("tree38", 12, 2, None, 1),                 # latency forward
    ("chain6ff", 10, 2, 0, 0),                  # lane-per-rollout forward
    ("tree38_frame", 12, 0, None, 1),           # constrained: the candidates' costs from cand_cost_kernel
])
@pytest.mark.parametrize("mode", ["no_frames", "nothing", "zero_weights"])
def test_zero_weights_change_nothing(gpu, name, T, fd_mode, fo_, fwd_path, mode):
    """flag on with no frames, with frames set and nothing uploaded, and with targets far away but every weight 0: linearise, both
    costs, sweep and forward are bit for bit what the flag-off context computes, on both forward paths and the constrained one"""
    capi = gpu
    mu, B = 10.0, 2
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 31, held=True)
    mults = tc._mults(o, xs[0], 32)
    frames = pick_aim_frames(model)
    g, w = random_task(o, frames, xs, B, 33)
    g[..., :3] += 50.0
    out = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_TRACE | (FLAG(capi) if on else 0)) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            _setup(ctx, xs, us, mults, o.Etot)
            if on and mode == "nothing":
                set_task(ctx, frames)
            if on and mode == "zero_weights":
                set_task(ctx, frames, g, np.zeros_like(w))
            out[on] = fc._run_all(ctx, mu, name == "tree38")
    fc._same(out[False], out[True])
    assert np.all(np.isfinite(out[True]["LX"])) and np.all(np.isfinite(out[True]["X_NEW"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_", [("tree38", None), ("chain6ff", 0)])
@pytest.mark.parametrize("part", ["aim", "range"])
def test_weight_partitions(gpu, name, fo_, part):
    """aim: with w_range = 0 the result is bit for bit independent of the uploaded rho.  range: with w_aim = 0 it differs from the
    flag-off run and equals the yardstick's range-only terms"""
    capi = gpu
    T, B, mu = 10, 2, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 35, held=True)
    frames = pick_aim_frames(model)
    g, w = random_task(o, frames, xs, B, 36, wscale=0.1)
    w[..., 1 if part == "aim" else 0] = 0.0
    g2 = g.copy()
    g2[..., 3] = np.random.default_rng(37).uniform(0.0, 5.0, size=g2[..., 3].shape)
    with capi.Context(spec, flags=capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us)
        off = fc._run_all(ctx, mu, False)
    out = []
    for other in ((False, True) if part == "aim" else (False,)):
        with capi.Context(spec, flags=FLAG(capi) | capi.FLAG_TRACE) as ctx:
            _setup(ctx, xs, us)
            set_task(ctx, frames, g2 if other else g, w)
            out.append(fc._run_all(ctx, mu, False))
    assert not np.array_equal(out[0]["LX"], off["LX"]) and not np.array_equal(out[0]["COSTS_OLD"], off["COSTS_OLD"])
    if part == "aim":
        fc._same(out[0], out[1])
        return
    for b in range(B):                                   # the yardstick with w_aim = 0 is the range rows alone
        add = fa_derivs(o, model, frames, xs[b], g[b], w[b])
        for s in ("LX", "LXX", "LFX", "LFXX"):
            e = rel_err(out[0][s][b], off[s][b] + add[s])
            print("range only", name, s, b, e)
            assert e <= TOL_LIN, (s, b, e)
        e = rel_err(out[0]["COSTS_OLD"][b], off["COSTS_OLD"][b] + fa_terms(o, frames, xs[b], g[b], w[b]))
        assert e <= TOL_LIN, ("COSTS_OLD", b, e)


LIN_CASES = [("chain6", 2, None, ""), ("tree38", 2, None, ""), ("chain6ff", 2, 0, ""), ("tree38ff", 0, 0, "nt"),
             ("table7", 2, None, ""), ("tree38", 2, None, "all")]


def _lin_task(o, frames, xs, B, T):
    g, w = random_task(o, frames, xs, B, 43)
    w[1, 2] = 0.0; w[0, T] = 0.0; w[2, 0] = 0.0      # whole blocks without a weight
    w[0, 1, 0, 1] = 0.0                              # a frame without a range weight,
    w[1, 3, 1, 0] = 0.0                              # one without an aim weight,
    w[2, 4, 2] = 0.0                                 # one that is not walked,
    w[1, T, 3, 1] = 0.0; w[0, 2, 3, 0] = 0.0         # and the second frame of the shared joint, either way
    return g, w


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_,flags", LIN_CASES)
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, name, fd_mode, fo_, flags, stages):
    """LX, LXX, LFX, LFXX against the flag-off values plus the definition's terms, batch 3 with different data per instance, four
    frames (two of them on one joint), through ddp_hip_linearize and ddp_hip_linearize_stages(LIN_COST); LXX / LFXX symmetric bit
    for bit; LU, LUU, LUX, every velocity row and column and the q rows off the live frames' paths bit for bit the flag-off
    values; blocks whose weights are 0 bit for bit flag-off, the others differ.  "all": every other cost flag live beside it
    (the order of additions); "nt": tensor-free; chain6ff: the analytic first-order free-flyer path"""
    capi = gpu
    T, B = 6, 3
    model, spec, o = make_any(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 41)
    frames = pick_aim_frames(model)
    g, w = _lin_task(o, frames, xs, B, T)
    live = check_task(o, frames, xs, g, w)
    assert live.sum() == live.size - 3
    cframes = fc.pick_frames(model, 3)
    base = capi.FLAG_NO_TENSORS if flags == "nt" else 0
    if flags == "all":
        base |= (capi.FLAG_TRACKING_COST | capi.FLAG_FRAME_COST | capi.FLAG_FRAME_ORIENT_COST | capi.FLAG_FRAME_VEL_COST
                 | capi.FLAG_STATE_LIMITS | capi.FLAG_COM_COST | capi.FLAG_MOMENTUM_COST | capi.FLAG_RELATIVE_FRAME_COST
                 | capi.FLAG_CONTROL_GRAV_COST | capi.FLAG_OBSTACLE_COST | capi.FLAG_SELF_COLLISION_COST)
        ref = tc.random_ref(o, model, xs, us, B, 44)
        ftask = fc.random_task(o, xs, cframes, B, 45)
        otask = fo.random_orient(o, xs, cframes, B, 47)
        vtask = fv.random_task(o, xs, cframes, B, 49)
        lim = sl.random_limits(o, xs, B, 46)
        ctask = cm.random_task(o, model, xs, B, 48)
        mtask = mo.random_task(o, model, xs, B, 51)
        pairs = rf.pick_pairs(model)
        rtask = rf._lin_task(o, pairs, xs, B, T)
        gtask = cg.random_task(o, model, B, 53)
        opts = ob.pick_points(model)
        obtask = ob.random_task(o, opts, ob.KINDS, xs, B, 50)
        scpairs = sc.all_pairs(opts)
        sctask = sc.random_task(o, opts, scpairs, xs, B, 52)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (FLAG(capi) if on else 0)) as ctx:
            _setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
            if flags == "all":
                tc.upload_ref(ctx, ref)
                ctx.set_frame_cost(frames=cframes, target=ftask[0], weight=ftask[1])
                ctx.set_frame_orient_cost(quat=otask[0], weight=otask[1])
                ctx.set_frame_vel_cost(target=vtask[0], weight=vtask[1])
                ctx.set_state_limits(lo=lim[0], hi=lim[1], weight=lim[2])
                ctx.set_com_cost(target=ctask[0], weight=ctask[1])
                ctx.set_momentum_cost(target=mtask[0], weight=mtask[1])
                rf.set_task(ctx, pairs, *rtask)
                ctx.set_control_grav_cost(offset=gtask[0], weight=gtask[1])
                ob.set_task(ctx, opts, ob.KINDS, *obtask)
                sc.set_task(ctx, opts, scpairs, *sctask)
            if on:
                set_task(ctx, frames, g, w)
            ctx.linearize(None if stages is None else capi.LIN_COST)
            got[on] = {s: ctx.download(s) for s in DERIVS}
    n, nv = o.n, o.nv
    worst = 0.0
    for b in range(B):
        add = fa_derivs(o, model, frames, xs[b], g[b], w[b])
        for s in ("LX", "LXX", "LFX", "LFXX"):
            ex = got[False][s][b] + add[s]
            assert (b == 0 and s in ("LFX", "LFXX")) or np.max(np.abs(add[s])) > 0
            e = rel_err(got[True][s][b], ex)
            worst = max(worst, e)
            print("linearize", name, flags, stages, s, b, e)
            assert e <= TOL_LIN, (s, b, e)
        for s in ("LU", "LUU", "LUX"):
            assert np.array_equal(got[True][s][b], got[False][s][b]), s
        for t in range(T + 1):
            key, k = ("LXX", t) if t < T else ("LFXX", 0)
            blk = got[True][key][b][k * n * n:(k + 1) * n * n].reshape(n, n)
            off = got[False][key][b][k * n * n:(k + 1) * n * n].reshape(n, n)
            gk, go = ("LX", t) if t < T else ("LFX", 0)
            gon, goff = got[True][gk][b][go * n:(go + 1) * n], got[False][gk][b][go * n:(go + 1) * n]
            rows = add["rows"][t]
            assert rows.any() == live[b, t] and not rows[nv:].any()
            assert np.array_equal(blk, blk.T)
            assert np.array_equal(blk[~rows, :], off[~rows, :]) and np.array_equal(blk[:, ~rows], off[:, ~rows])
            assert np.array_equal(gon[~rows], goff[~rows])
            if live[b, t]:
                assert not np.array_equal(blk, off) and not np.array_equal(gon, goff)
            else:
                assert np.array_equal(blk, off) and np.array_equal(gon, goff)
    print("linearize", name, flags, stages, "worst", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_", [("tree38", 0, None), ("chain6ff", 0, 0), ("chain6", 2, None), ("tree38_frame", 0, None)])
def test_cost_seq_aug_and_error(gpu, name, fd_mode, fo_):
    """COSTS_OLD / COSTS_NEW (which = 0 / 1) against the flag-off context's values plus the numpy terms, lf included; a block
    without a weight keeps the flag-off value bit for bit; ddp_hip_frame_aim_error against the yardstick's (theta, l) along X and
    X_NEW to 1e-12, whatever the weights"""
    capi = gpu
    T, B, mu = 6, 3, 30.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 51)
    xs2, us2 = _trajs(o, model, B, 61)
    frames = pick_aim_frames(model)
    g, w = random_task(o, frames, xs, B, 52)
    w[1, 3] = 0.0; w[0, T] = 0.0; w[2, 1, 1] = 0.0; w[0, 2, 0, 1] = 0.0; w[1, 0, 2, 0] = 0.0
    live = check_task(o, frames, xs, g, w)
    mults = tc._mults(o, xs[0], 53)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | (FLAG(capi) if on else 0)) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
            if on:
                set_task(ctx, frames, g, w)
                err = {0: ctx.frame_aim_error(0), 1: ctx.frame_aim_error(1)}
            ctx.cost_seq_aug(0, mu)
            ctx.cost_seq_aug(1, mu)
            got[on] = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
    for which, X in ((0, xs), (1, xs2)):
        for b in range(B):
            add = fa_terms(o, frames, X[b], g[b], w[b])
            ex = got[False][which][b] + add
            assert np.array_equal(add != 0.0, live[b])
            e = rel_err(got[True][which][b], ex)
            ref = fa_errors(o, frames, X[b], g[b])
            ee = float(np.max(np.abs(err[which][b] - ref)))
            print("cost_seq_aug", name, which, b, e, "error", ee)
            assert e <= TOL_LIN, (which, b, e)
            assert err[which][b].shape == (T + 1, len(frames), 2) and ee <= TOL_LIN, (which, b, ee)
            assert np.array_equal(got[True][which][b][~live[b]], got[False][which][b][~live[b]])


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_,fwd_path", [("tree38", None, 1), ("chain6ff", 0, 0), ("tree38_frame", None, 1)])
@pytest.mark.parametrize("k_scale", [1.0, 3.0])
def test_forward_matches_emulation(gpu, name, fo_, fwd_path, k_scale):
    """accepted step, X_NEW, U_NEW and dcost against Oracle.forward_alpha rollouts costed with numpy, the aiming terms included,
    with n_alpha = 1 and 8, which also give the same accepted step and X_NEW as each other; k_scale 3 overshoots, so that the
    first candidates are refused and the halving runs (asserted on the emulation).  Every candidate tried decides by more than
    1e-9 of the sum of the cost terms' magnitudes; only then are decisions compared"""
    capi = gpu
    T, mu = 12, 1.0
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo_)
    frames = pick_aim_frames(model)
    xs, us = _trajs(o, model, 1, 81, held=True)
    g, w = random_task(o, frames, xs, 1, 82, wscale=20.0)
    check_task(o, frames, xs, g, w)
    mults = tc._mults(o, xs[0], 87)
    res = {}
    with capi.Context(spec, flags=FLAG(capi) | capi.FLAG_NO_TENSORS) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        _setup(ctx, xs, us, mults, o.Etot)
        set_task(ctx, frames, g, w)
        ctx.linearize()
        _, _, mu_o, _ = ctx.backward(0.0, mu)
        if k_scale != 1.0:
            ctx.upload("FB_VAL", k_scale * ctx.download("FB_VAL"))
        fb = {"origin": ctx.download("FB_ORIGIN")[0], "val": ctx.download("FB_VAL")[0], "jac": ctx.download("FB_JAC")[0]}
        for n_alpha in (1, 8):
            rc, step, dcost = ctx.forward(mu_o, n_alpha=n_alpha)
            res[n_alpha] = (step[0], dcost[0], ctx.download("X_NEW")[0], ctx.download("U_NEW")[0], ctx.frame_aim_error(1)[0])

    def cost(X, U):
        return o.cost_seq_aug(X, U, mults, mu_o[0]) + fa_terms(o, frames, X, g[0], w[0])
    em = _emulate_forward(o, xs[0], us[0], mults, fb, mu_o[0], 8, cost)
    assert em is not None
    step_ref, xn_ref, un_ref, new, margins = em
    print("forward", name, k_scale, "step", res[8][0], step_ref, "dcost", res[8][1], new, "margins", margins)
    assert min(margins) > 1e-9, margins
    if k_scale != 1.0:
        assert step_ref < 1.0 and len(margins) > 1                             # the first candidates are refused
    for n_alpha in (1, 8):
        step, dcost, xn, un, err = res[n_alpha]
        assert step == step_ref, (step, step_ref)
        assert rel_err(xn, xn_ref) < TOL_FWD and rel_err(un, un_ref) < TOL_FWD
        assert abs(dcost - new) <= TOL_FWD * max(1.0, abs(new)), (dcost, new)
        assert rel_err(err, fa_errors(o, frames, xn_ref, g[0])) < TOL_FWD
    assert res[1][0] == res[8][0] and np.array_equal(res[1][2], res[8][2])


@pytest.mark.gpu
def test_sweep_matches_oracle(gpu):
    """the backward sweep with the device's LX / LXX carrying the term against Oracle.backward, tree38: restarts, mu and reg
    identical, every step redone alone by the oracle from the device's V(t+1) to 1e-10 (stepwise_backward_check)"""
    from oracle.binding import Oracle
    capi = gpu
    name, T, mu = "tree38", 12, 1.0
    model, spec, o = make(name, T, fd_mode=2)
    xs, us = _trajs(o, model, 1, 71, held=True)
    frames = pick_aim_frames(model)
    g, w = random_task(o, frames, xs, 1, 72, wscale=0.1, lo=0.1, hi=0.3)   # (small: the sweep must stay positive definite)
    check_task(o, frames, xs, g, w, hi=0.3)
    mults = tc._mults(o, xs[0], 73)
    n = o.n
    with capi.Context(spec, flags=FLAG(capi) | capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        set_task(ctx, frames, g, w)
        ctx.linearize()
        rc, reg, mu_out, restarts = ctx.backward(0.0, mu)
        d = o.alloc_derivs()
        for k, s in NAMES.items():
            if ctx.seq_size(s):
                d[k][:ctx.seq_size(s)] = ctx.download(s)[0]
        assert np.max(np.abs(d["lfx"][:n])) > 0
        ref_b = o.backward(d, xs[0], mults, 0.0, mu)
        print("sweep", name, "device restarts", int(restarts[0]), "oracle", ref_b["restarts"], "mu", mu_out[0], ref_b["mu"], "reg", reg[0], ref_b["reg"])
        assert int(restarts[0]) == ref_b["restarts"] and mu_out[0] == ref_b["mu"] and reg[0] == ref_b["reg"]
        got = {s: ctx.download(s)[0] for s in ("FB_JAC", "FB_VAL", "VX_TRACE", "VXX_TRACE")}
    assert np.max(np.abs(got["VX_TRACE"])) > 0

    def one_step_oracle(t):
        return Oracle(model, 1, dt=0.01, c=1.0, fd_mode=2)
    assert not o.Etot
    worst = stepwise_backward_check(one_step_oracle, o, d, xs[0], mults, reg[0], mu_out[0], got["VX_TRACE"], got["VXX_TRACE"],
                                    got["FB_VAL"], got["FB_JAC"], range(T))
    print("stepwise worst", worst)
    assert worst < TOL_SWEEP, worst


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_,flags", [("chain6ff", 2, 0, 0), ("tree38", 0, 0, 1)])
def test_instances_are_independent(gpu, name, fd_mode, fo_, flags):
    """batch 2 through linearise, sweep, forward: other targets, stand-offs and weights for instance 1 leave instance 0's outputs
    bit-identical"""
    capi = gpu
    T, B, mu = 10, 2, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    frames = pick_aim_frames(model)
    xs, us = _trajs(o, model, B, 91, held=True)
    t1 = random_task(o, frames, xs, B, 92, wscale=0.1)
    t2 = random_task(o, frames, xs, B, 93, wscale=0.3)
    out = []
    for other in (False, True):
        g, w = (a.copy() for a in t1)
        if other:
            g[1], w[1] = t2[0][1], t2[1][1]
        with capi.Context(spec, flags=FLAG(capi) | capi.FLAG_TRACE | flags) as ctx:
            _setup(ctx, xs, us)
            set_task(ctx, frames, g, w)
            out.append(fc._run_all(ctx, mu, False))
    a, b = out
    assert not np.array_equal(a["LX"][1], b["LX"][1]) and not np.array_equal(a["COSTS_OLD"][1], b["COSTS_OLD"][1])
    fc._same(fo._first(a), fo._first(b))


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,flags", [("chain6", 2, 0), ("tree38", 0, 1)])
def test_solve_matches_stepwise(gpu, name, fd_mode, flags):
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B, iters, thr, mu, w_, n_ = 10, 2, 4, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode)
    frames = pick_aim_frames(model)
    xs, us = _trajs(o, model, B, 101, held=True)
    g, w = random_task(o, frames, xs, B, 104, hi=1.0)
    mults = tc._mults(o, xs[0], 103)

    def run(stepwise):
        with capi.Context(spec, flags=FLAG(capi) | flags) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if o.Etot:
                ctx.upload("MULT_ORIGIN", xs[:, :T * o.nx])
            set_task(ctx, frames, g, w)
            log = (solver.solve_stepwise if stepwise else solver.solve)(ctx, iters, thr, mu, 0.0, w_, n_)
            return log, ctx.download("X"), ctx.download("U")
    la, xa, ua = run(False)
    lb, xb, ub = run(True)
    assert np.all(np.isfinite(xa))
    assert not np.array_equal(xa, xs)
    assert np.array_equal(xa, xb) and np.array_equal(ua, ub)
    for k in ("iterations", "mu", "reg", "w", "n", "last_step", "opt_obj", "opt_constr"):
        assert np.array_equal(np.asarray(la[k]), np.asarray(lb[k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain6", "tree38", "chain6ff", "tree38ff", "table7"])
def test_model_frame_axis(gpu, name):
    """ddp_hip_model_frame_axis against the yardstick (p, n, J = [dp; dn]) and J against differences; uploading g = p + n l0
    with rho = l0 leaves |r| <= 1e-12 (|r_aim| = 2 sin(theta / 2), r_range = l - l0, from the readback)"""
    capi = gpu
    T, B = 2, 2
    model, spec, o = make_any(name, T, batch=B, fd_mode=0)
    frames = pick_aim_frames(model)
    rng = np.random.default_rng(5)
    nv = o.nv
    l0 = 0.7
    with capi.ModelHandle(model) as h:
        for k in range(2):
            q = rand_q(o, rng)
            for i, (j, off, ax) in enumerate(frames):
                p3, n3, J = h.frame_axis(j, off, ax, q, jacobian=True)
                p_only, n_only = h.frame_axis(j, off, ax, q)
                assert np.array_equal(p3, p_only) and np.array_equal(n3, n_only)
                py, ny = eye_axis(o, frames[i], q)
                Jy, cols = pn_J(o, model, frames[i], q)
                ep, en, eJ = rel_err(p3, py), rel_err(n3, ny), rel_err(J, Jy)
                print("model_frame_axis", name, k, i, ep, en, eJ)
                assert abs(np.linalg.norm(n3) - 1.0) <= 1e-10
                assert ep <= TOL_LIN and en <= TOL_LIN and eJ <= TOL_LIN
                assert np.all(J[:, [c for c in range(nv) if c not in cols]] == 0.0)
                if k == 0 and i < 2:
                    fd = np.zeros((6, nv))
                    for c in range(nv):
                        e = np.zeros(nv); e[c] = H
                        for s, cw in W5:
                            fd[:, c] += cw * np.concatenate(eye_axis(o, frames[i], o.integrate(q, s * e))) / H
                    assert np.max(np.abs(fd - J)) <= TOL_FD * max(1.0, np.max(np.abs(J))), np.max(np.abs(fd - J))
        j, off, ax = frames[0]
        for bad in ((-1, ax), (len(model.parent), ax), (j, (1.0, 0.0, 1e-4)), (j, (0.0, 0.0, 0.0)), (j, (np.nan, 0.0, 0.0))):
            with pytest.raises(capi.DdpHipError) as exc:
                h.frame_axis(bad[0], off, bad[1], q)
            assert exc.value.code == capi.E_ARG
        # "what it looks at now, l0 ahead": uploaded as target with rho = l0 it is held to rounding
        xs, us = _trajs(o, model, B, 7)
        F = len(frames)
        g = np.zeros((B, T + 1, F, 4))
        for b in range(B):
            X = xs[b].reshape(T + 1, o.nx)
            for t in range(T + 1):
                for i, (j, off, ax) in enumerate(frames):
                    p3, n3 = h.frame_axis(j, off, ax, X[t][:o.nq])
                    g[b, t, i] = np.concatenate([p3 + l0 * n3, [l0]])
    with capi.Context(spec, flags=FLAG(capi) | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        set_task(ctx, frames, g, 1.0)
        err = ctx.frame_aim_error(0)
        ctx.cost_seq_aug(0, 1.0)
        with_term = ctx.download("COSTS_OLD")
        ctx.set_frame_aim_cost(weight=0.0)
        ctx.cost_seq_aug(0, 1.0)
        without = ctx.download("COSTS_OLD")
    r = np.stack([2.0 * np.sin(0.5 * err[..., 0]), err[..., 1] - l0], axis=-1)
    print("hold", name, float(np.max(np.abs(r))))
    assert err.shape == (B, T + 1, F, 2) and np.max(np.abs(r)) <= TOL_HOLD, np.max(np.abs(r))
    assert np.max(np.abs(with_term - without)) <= TOL_HOLD


@pytest.mark.gpu
def test_look_at_task(gpu):
    """tree38, a head-like leaf with a camera axis and a target that moves across t, from a posture that looks about 1 rad off: a
    few iterations of the stepwise loop bring the angle at T below its initial value and lower the cost.  No absolute angle is
    fixed"""
    capi = gpu
    T, mu, iters = 12, 1.0, 6
    model, spec, o = make("tree38", T, fd_mode=0)
    frames = pick_aim_frames(model)[:1]
    xs, us = _trajs(o, model, 1, 111, held=True)
    q0 = xs[0][:o.nq]
    p0, n0 = eye_axis(o, frames[0], q0)
    u = np.cross(n0, [0.3, -0.5, 0.8]); u /= np.linalg.norm(u)
    v = np.cross(n0, u)
    g = np.zeros((T + 1, 1, 4))
    for t in range(T + 1):                               # 1 rad off the present axis, one metre away, drifting sideways by 20 cm
        g[t, 0, :3] = p0 + np.cos(1.0) * n0 + np.sin(1.0) * u + 0.2 * (t / T) * v
        g[t, 0, 3] = 1.0
    w = np.zeros((T + 1, 1, 2)); w[:, 0, 0] = 50.0; w[T, 0, 0] = 2000.0
    with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | FLAG(capi)) as ctx:
        _setup(ctx, xs, us)
        set_task(ctx, frames, g, w)
        th0 = ctx.frame_aim_error(0)[0, T, 0, 0]
        ctx.cost_seq_aug(0, mu)
        c0 = float(np.sum(ctx.download("COSTS_OLD")[0]))
        moved = 0
        for _ in range(iters):
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            rc, step, dcost = ctx.forward(mu_o, n_alpha=8)
            if step[0] > 0.0:
                ctx.swap_traj()
                moved += 1
        th1 = ctx.frame_aim_error(0)[0, T, 0, 0]
        ctx.cost_seq_aug(0, mu)
        c1 = float(np.sum(ctx.download("COSTS_OLD")[0]))
    print("look-at: theta at T", th0, "->", th1, "cost", c0, "->", c1, "accepted steps", moved)
    assert 0.8 <= th0 <= 1.2
    assert moved > 0 and th1 < th0 and c1 < c0, (th0, th1, c0, c1)


@pytest.mark.gpu
def test_degenerate_line_of_sight(gpu):
    """a resident l <= 1e-12 (the target uploaded equal to the frame's own point at X[0]): cost and derivatives are finite and
    equal, bit for bit, what the other frames form alone; the yardstick's rule gives the same to the linearise tolerance"""
    capi = gpu
    T, B, mu = 4, 2, 10.0
    model, spec, o = make("tree38", T, batch=B, fd_mode=0)
    frames = pick_aim_frames(model)
    xs, us = _trajs(o, model, B, 121)
    g, w = random_task(o, frames, xs, B, 122)
    with capi.ModelHandle(model) as h:
        p3, _ = h.frame_axis(*frames[1], xs[0][:o.nq])
    g[0, 0, 1, :3] = p3
    w_alone = w.copy(); w_alone[0, 0, 1] = 0.0
    assert residual(o, frames[1], xs[0][:o.nq], g[0, 0, 1])[0] is None
    got = {}
    for key, ww in (("degenerate", w), ("alone", w_alone)):
        with capi.Context(spec, flags=FLAG(capi)) as ctx:
            _setup(ctx, xs, us)
            set_task(ctx, frames, g, ww)
            ctx.linearize()
            got[key] = {s: ctx.download(s) for s in DERIVS}
            ctx.cost_seq_aug(0, mu)
            got[key]["COSTS_OLD"] = ctx.download("COSTS_OLD")
            if key == "degenerate":
                err = ctx.frame_aim_error(0)
    assert err[0, 0, 1, 1] <= MIN_RANGE and err[0, 0, 1, 0] == 0.0
    for s in got["alone"]:
        assert np.all(np.isfinite(got["degenerate"][s])), s
        assert np.array_equal(got["degenerate"][s][0], got["alone"][s][0]), s
    with capi.Context(spec) as ctx:
        _setup(ctx, xs, us)
        ctx.linearize()
        off = {s: ctx.download(s) for s in ("LX", "LXX")}
    add = fa_derivs(o, model, frames, xs[0], g[0], w[0])
    for s in ("LX", "LXX"):
        assert rel_err(got["degenerate"][s][0], off[s][0] + add[s]) <= TOL_LIN, s


@pytest.mark.gpu
def test_refusals_and_defaults(gpu):
    """every refusal of the entry points, the defaults, set_frames again (the same joints keep the data, others reset it) and the
    live rule on half-batch uploads of zeros"""
    import ctypes as C
    capi = gpu
    T, B = 4, 4
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    frames = pick_aim_frames(model)
    F = len(frames)
    nj = len(model.parent)
    L = capi.lib()
    dp = C.POINTER(C.c_double)

    def code(fn):
        with pytest.raises(capi.DdpHipError) as exc:
            fn()
        return exc.value.code
    with capi.Context(spec) as ctx:                                   # a context without the flag
        assert code(lambda: ctx.set_aim_frames(frames)) == capi.E_UNSUPPORTED
        with pytest.raises(ValueError):                              # the wrapper has no frame count to check shapes against
            ctx.set_frame_aim_cost(weight=1.0)
        z = np.ones(B * (T + 1) * F * 2)
        assert L.ddp_hip_frame_aim_upload(ctx._h, None, z.ctypes.data_as(dp), 0, 1) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.get_frame_aim_cost()) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.frame_aim_error()) == capi.E_UNSUPPORTED
    pend = capi.BuiltinModel(capi.BUILTIN_PENDULUM)
    with pytest.raises(capi.DdpHipError) as exc:
        capi.Context(capi.ProblemSpec(pend, T, fd_mode=2), flags=FLAG(capi))
    assert exc.value.code == capi.E_UNSUPPORTED
    with capi.Context(spec, flags=FLAG(capi)) as ctx:                 # the flag stands alone: no frame-cost flag beside it
        z = np.ones(B * (T + 1) * F * 2)
        assert L.ddp_hip_frame_aim_upload(ctx._h, None, z.ctypes.data_as(dp), 0, B) == capi.E_ARG   # before set_frames
        assert code(lambda: ctx.frame_aim_error()) == capi.E_ARG
        g0, w0 = ctx.get_frame_aim_cost()
        assert g0.shape == (B, T + 1, 0, 4) and w0.shape == (B, T + 1, 0, 2)
        j, off, ax = frames[0]
        for bad in (frames + frames[:1], [(nj, off, ax)], [(-1, off, ax)], [(j, (0.0, np.nan, 0.0), ax)], [(j, off, (np.inf, 0.0, 0.0))],
                    [(j, off, (1.0, 1e-4, 0.0))], [(j, off, (0.0, 0.0, 0.0))], frames[:2] + [(j, off, (2.0, 0.0, 0.0))]):
            assert code(lambda: ctx.set_aim_frames(bad)) == capi.E_ARG, bad
        assert code(lambda: ctx.frame_aim_error()) == capi.E_ARG      # a refused set_frames sets nothing
        ctx.set_aim_frames([])                                       # no frames is a list
        assert code(lambda: ctx.frame_aim_error()) == capi.E_ARG
        ctx.set_aim_frames(frames)
        g0, w0 = ctx.get_frame_aim_cost()                             # defaults: targets, stand-offs and weights 0
        assert g0.shape == (B, T + 1, F, 4) and np.all(g0 == 0.0) and w0.shape == (B, T + 1, F, 2) and np.all(w0 == 0.0)
        rng = np.random.default_rng(5)
        gg = rng.normal(size=(B, T + 1, F, 4)); gg[..., 3] = np.abs(gg[..., 3])
        wg = rng.uniform(0, 1, size=(B, T + 1, F, 2))
        for bad in (-1e-3, np.nan, np.inf):
            wb = wg[0].copy(); wb[1, 2, 1] = bad
            assert code(lambda: ctx.set_frame_aim_cost(weight=wb)) == capi.E_ARG, bad
            assert code(lambda: ctx.set_frame_aim_cost(target=gg, weight=wb)) == capi.E_ARG, bad
        for bad, at in ((np.nan, 0), (np.inf, 1), (-np.inf, 3), (np.nan, 3), (-1e-3, 3)):   # a bad coordinate, a bad stand-off
            gb = gg[0].copy(); gb[2, 1, at] = bad
            assert code(lambda: ctx.set_frame_aim_cost(target=gb, weight=wg)) == capi.E_ARG, (bad, at)
            assert code(lambda: ctx.set_frame_aim_cost(target=gb)) == capi.E_ARG, (bad, at)
        assert code(lambda: ctx.set_frame_aim_cost(weight=wg[0], first=B, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_frame_aim_cost(weight=wg[0], first=-1, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_frame_aim_cost(weight=wg[0], first=1, count=B)) == capi.E_ARG
        assert code(lambda: ctx.get_frame_aim_cost(first=1, count=B)) == capi.E_ARG
        big = np.zeros((B + 1) * (T + 1) * F * 4)
        assert L.ddp_hip_frame_aim_upload(ctx._h, None, big.ctypes.data_as(dp), 0, B + 1) == capi.E_ARG
        assert L.ddp_hip_frame_aim_error(ctx._h, 2, big.ctypes.data_as(dp)) == capi.E_ARG
        assert L.ddp_hip_frame_aim_error(ctx._h, 0, None) == capi.E_ARG
        g1, w1 = ctx.get_frame_aim_cost()
        assert np.all(g1 == 0.0) and np.all(w1 == 0.0)                # refused uploads wrote nothing
        ctx.set_frame_aim_cost(target=gg, weight=wg)
        g1, w1 = ctx.get_frame_aim_cost()
        assert np.array_equal(g1, gg) and np.array_equal(w1, wg)
        ctx.set_frame_aim_cost(target=2.0 * gg[1], first=1, count=1)  # one side, one instance; the others stay
        g1, w1 = ctx.get_frame_aim_cost()
        assert np.array_equal(g1[0], gg[0]) and np.array_equal(g1[1], 2.0 * gg[1]) and np.array_equal(w1, wg)
        g2, w2 = ctx.get_frame_aim_cost(first=1, count=2)             # the round trip of a range of instances
        assert np.array_equal(g2, g1[1:3]) and np.array_equal(w2, wg[1:3])
        bw = np.array([1.5, 0.0])
        ctx.set_frame_aim_cost(weight=bw, first=1, count=2)           # broadcast: (2,)
        assert np.array_equal(ctx.get_frame_aim_cost()[1][1:3], np.broadcast_to(bw, (2, T + 1, F, 2)))
        assert np.array_equal(ctx.get_frame_aim_cost()[1][0], wg[0])
        # set_frames again: the same joints keep the data (eyes and axes may move), other joints reset it
        moved = [(jj, tuple(0.5 * np.asarray(of)), tuple(-np.asarray(a))) for jj, of, a in frames]
        ctx.set_aim_frames(moved)
        g3, w3 = ctx.get_frame_aim_cost()
        assert np.array_equal(g3, g1) and np.any(w3 != 0.0)
        ctx.set_aim_frames(frames[:-1] + [(frames[1][0],) + frames[-1][1:]])   # the same count, one frame on another joint
        g4, w4 = ctx.get_frame_aim_cost()
        assert np.all(g4 == 0.0) and np.all(w4 == 0.0)
        ctx.set_frame_aim_cost(weight=1.0)
        ctx.set_aim_frames(frames[:2])
        g5, w5 = ctx.get_frame_aim_cost()
        assert g5.shape == (B, T + 1, 2, 4) and np.all(g5 == 0.0) and np.all(w5 == 0.0)
        # the live rule: zeros that arrive half-batch by half-batch leave the kernels launched, with the flag-off bits
        xs, us = _trajs(o, model, B, 161)
        _setup(ctx, xs, us)
        ctx.set_aim_frames(frames)
        ctx.linearize()
        off_ = {s: ctx.download(s) for s in DERIVS}
        g, w = random_task(o, frames, xs, B, 162)
        ctx.set_frame_aim_cost(target=g, weight=w)
        ctx.linearize()
        assert not np.array_equal(ctx.download("LX"), off_["LX"])
        ctx.set_frame_aim_cost(weight=0.0, first=0, count=B // 2)
        ctx.linearize()
        lx = ctx.download("LX")
        assert np.array_equal(lx[:B // 2], off_["LX"][:B // 2]) and not np.array_equal(lx[B // 2:], off_["LX"][B // 2:])
        ctx.set_frame_aim_cost(weight=0.0, first=B // 2, count=B - B // 2)
        ctx.linearize()
        for s in DERIVS:
            assert np.array_equal(ctx.download(s), off_[s]), s
        assert np.max(np.abs(ctx.frame_aim_error(0)[0] - fa_errors(o, frames, xs[0], g[0]))) <= TOL_LIN   # live weights or not
