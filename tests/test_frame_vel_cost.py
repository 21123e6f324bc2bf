"""Per-instance frame-velocity costs (DDP_HIP_FLAG_FRAME_VEL_COST, include/ddp_hip/ddp_hip.h), of the cost frames of
DDP_HIP_FLAG_FRAME_COST:

    r_f = (P_f(q) v - g_lin, W_f(q) v - g_ang),   l(t, x, u) += 1/2 sum_f sum_a w[b][t][f][a] r_f,a^2,   lf(x_T) alike with w[b][T]

with P_f the true point jacobian of the frame's point and W_f the world angular jacobian of its joint's frame.  The oracle has no
such cost, so the yardstick is the numpy restatement below: P_f from Oracle.frame_jacobian(world_aligned=True), W_f from
test_frame_orient_cost.frame_W, and the configuration half of the residual's jacobian (D = d(P_f v)/d(delta q), E = d(W_f v)/
d(delta q)) written out analytically from the world axes a_j (the columns of W_f and, for a prismatic joint, of P_f) and the world
origins o_j = frame_position(j, 0, q) of the joints on the frame's path; test_yardstick_gradient holds it against central
differences.  The helpers of test_tracking_cost.py, test_frame_cost.py, test_frame_orient_cost.py, test_state_limits.py and
test_com_cost.py are reused by import; tolerances are theirs."""
import os
import re

import numpy as np
import pytest

import test_com_cost as cm
import test_frame_cost as fc
import test_frame_orient_cost as fo
import test_state_limits as sl
import test_tracking_cost as tc
from problems import make
from synth import rel_err, stepwise_backward_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 1e-3
DERIVS = fc.DERIVS
NAMES = fc.NAMES
MODELS = ["chain6", "tree38", "chain6ff", "tree38ff", "table7"]
make_any = cm.make_any
_trajs, _setup = tc._trajs, tc._setup
REVOLUTE = 0                                             # capi.JOINT_REVOLUTE (asserted in test_interface_constants)
ZERO3 = (0.0, 0.0, 0.0)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def path_of(model, j):
    """the joints root .. j, ascending"""
    out = []
    while j >= 0:
        out.append(int(j))
        j = int(model.parent[j])
    return out[::-1]


def cols_of(model, j):
    """the tangent columns of joint j: a free-flyer root owns 0 .. 5, the joints behind it j + 5"""
    if model.ff:
        return list(range(6)) if j == 0 else [j + 5]
    return [j]


def path_rows(o, model, frames):
    """the tangent rows (configuration rows, then velocity rows) of the frames' paths, as a boolean mask over n"""
    on = np.zeros(o.n, dtype=bool)
    for j, _ in frames:
        for i in path_of(model, j):
            for c in cols_of(model, i):
                on[c] = on[o.nv + c] = True
    return on


def frame_PW(o, j, off, q):
    P = o.frame_jacobian(j, off, q, world_aligned=True)
    return P, fo.frame_W(o, j, q, fo.frame_R(o, j, q))


def frame_velocity(o, j, off, q, v):
    """(pdot_f, omega_f) = (P_f v, W_f v)"""
    P, W = frame_PW(o, j, off, q)
    return np.concatenate([P @ v, W @ v])


def vel_jacobians(o, model, j, off, q, v):
    """(vel6, Jq, Jv): Jv = [P; W], Jq = [D; E] by column of the joints i on the path, with the prefix sums over the path up to
    and including i (a free-flyer root's six columns included):
      revolute   D_i = w_<=i x (a_i x (p_f - o_i)) + a_i x (pdot_f - pdot_<=i),   E_i = a_i x (omega_f - w_<=i)
      prismatic  D_i = w_<=i x a_i,                                               E_i = 0
      free-flyer root, angular column 3 + c:  D = (R_0 e_c) x pdot_f,  E = (R_0 e_c) x omega_f;  linear columns: 0"""
    P, W = frame_PW(o, j, off, q)
    pd, om = P @ v, W @ v
    pf = o.frame_position(j, off, q)
    D, E = np.zeros_like(P), np.zeros_like(P)
    w_le, p_le = np.zeros(3), np.zeros(3)
    for i in path_of(model, j):
        cols = cols_of(model, i)
        w_le = w_le + W[:, cols] @ v[cols]
        p_le = p_le + P[:, cols] @ v[cols]
        if model.ff and i == 0:
            R0 = fo.frame_R(o, 0, q)
            for c in range(3):
                D[:, 3 + c] = np.cross(R0[:, c], pd)
                E[:, 3 + c] = np.cross(R0[:, c], om)
            continue
        ci = cols[0]
        if int(model.jtype[i]) == REVOLUTE:
            a = W[:, ci]
            oi = o.frame_position(i, ZERO3, q)
            D[:, ci] = np.cross(w_le, np.cross(a, pf - oi)) + np.cross(a, pd - p_le)
            E[:, ci] = np.cross(a, om - w_le)
        else:
            D[:, ci] = np.cross(w_le, P[:, ci])
    return np.concatenate([pd, om]), np.vstack([D, E]), np.vstack([P, W])


def vel_terms(o, xs, frames, tgt, w):
    """the frame-velocity terms of one instance per t (T+1 values; the last belongs to lf); tgt, w: (T+1, F, 6).  A frame whose
    weights are all 0 is not walked"""
    X = xs.reshape(o.T + 1, o.nx)
    out = np.zeros(o.T + 1)
    for t in range(o.T + 1):
        for f, (j, off) in enumerate(frames):
            if not np.any(w[t][f] != 0.0):
                continue
            r = frame_velocity(o, j, off, X[t][:o.nq], X[t][o.nq:]) - tgt[t][f]
            out[t] += 0.5 * np.sum(w[t][f] * r * r)
    return out


def vel_grad_hess(o, model, x, frames, tgt_t, w_t, drop_q=False):
    """(lx, lxx) contributions at one state, n and n x n: A^T (w o r) and the Gauss-Newton A^T diag(w) A, A = [D; E | P; W].
    drop_q: without D and E (what an implementation that forgot them would form)"""
    n = o.n
    g, Hm = np.zeros(n), np.zeros((n, n))
    q, v = x[:o.nq], x[o.nq:]
    for f, (j, off) in enumerate(frames):
        if not np.any(w_t[f] != 0.0):
            continue
        vel, Jq, Jv = vel_jacobians(o, model, j, off, q, v)
        A = np.hstack([np.zeros_like(Jq) if drop_q else Jq, Jv])
        g += A.T @ (w_t[f] * (vel - tgt_t[f]))
        for a in range(6):                               # entry (i, j) and (j, i) alike: symmetric bit for bit
            Hm += w_t[f][a] * np.outer(A[a], A[a])
    return g, Hm


def vel_derivs(o, model, xs, frames, tgt, w):
    """what the terms add to LX, LXX, LFX, LFXX of one instance, in the library's flat (column-major) layout"""
    X = xs.reshape(o.T + 1, o.nx)
    out = {"LX": [], "LXX": []}
    for t in range(o.T + 1):
        g, Hm = vel_grad_hess(o, model, X[t], frames, tgt[t], w[t])
        if t == o.T:
            out["LFX"], out["LFXX"] = g, Hm.ravel(order="F")
        else:
            out["LX"].append(g); out["LXX"].append(Hm.ravel(order="F"))
    out["LX"], out["LXX"] = np.concatenate(out["LX"]), np.concatenate(out["LXX"])
    return out


def random_task(o, xs, frames, B, seed, wscale=1.0, spread=0.2):
    """per-instance targets near the frames' velocities along the trajectories (xs: (B, ...)) and positive weights, each
    (B, T+1, F, 6)"""
    rng = np.random.default_rng(seed)
    T, F = o.T, len(frames)
    tgt = np.zeros((B, T + 1, F, 6))
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            for f, (j, off) in enumerate(frames):
                tgt[b, t, f] = frame_velocity(o, j, off, X[t][:o.nq], X[t][o.nq:]) + spread * rng.normal(size=6)
    return tgt, wscale * rng.uniform(0.1, 2.0, size=(B, T + 1, F, 6))


def _moving(xs, o, seed, sigma=0.5):
    """the same trajectories with non-zero velocities at every t (a held trajectory stands still: D and E would be 0)"""
    rng = np.random.default_rng(seed)
    X = xs.reshape(xs.shape[0], o.T + 1, o.nx).copy()
    X[:, :, o.nq:] += sigma * rng.normal(size=X[:, :, o.nq:].shape)
    return X.reshape(xs.shape)


def _on(capi):
    return capi.FLAG_FRAME_COST | capi.FLAG_FRAME_VEL_COST


# ---- CPU: the yardstick checks itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_yardstick_gradient(name):
    """lx against the 5-point central difference of the numpy cost along x (+) (+-h e_j) over all 2 nv tangent directions; with
    the target at the current velocity (r = 0, where Gauss-Newton is exact) lxx against the central difference of the gradient;
    lxx symmetric bit for bit; the q rows, the v rows and the q-v block non-zero; rows off every frame's path exactly zero"""
    T = 2
    model, _, o = make_any(name, T, fd_mode=0)
    frames = fc.pick_frames(model, 3)
    xs, us = _trajs(o, model, 1, 3)
    xs = _moving(xs, o, 5)
    tgt, w = random_task(o, xs, frames, 1, 4)
    X = xs[0].reshape(T + 1, o.nx)
    nv, n = o.nv, o.n
    on = path_rows(o, model, frames)
    w5 = ((-2, 1.0 / 12), (-1, -8.0 / 12), (1, 8.0 / 12), (2, -1.0 / 12))
    for t in (1, T):
        g, Hm = vel_grad_hess(o, model, X[t], frames, tgt[0][t], w[0][t])
        assert np.max(np.abs(g[:nv])) > 0 and np.max(np.abs(g[nv:])) > 0
        assert np.max(np.abs(Hm[:nv, :nv])) > 0 and np.max(np.abs(Hm[nv:, nv:])) > 0 and np.max(np.abs(Hm[:nv, nv:])) > 0
        assert np.all(g[~on] == 0.0) and np.all(Hm[~on, :] == 0.0) and np.all(Hm[:, ~on] == 0.0)
        assert np.array_equal(Hm, Hm.T)

        def cost_at(dx):
            X2 = X.copy()
            X2[t] = tc._integrate_x(o, X[t], dx)
            return vel_terms(o, X2.ravel(), frames, tgt[0], w[0])[t]
        fd = np.zeros(n)
        for j in range(n):
            e = np.zeros(n); e[j] = H
            fd[j] = sum(cw * cost_at(s * e) for s, cw in w5) / H
        assert np.max(np.abs(fd - g)) <= 1e-8 * max(1.0, np.max(np.abs(g))), np.max(np.abs(fd - g))
        g_noq = vel_grad_hess(o, model, X[t], frames, tgt[0][t], w[0][t], drop_q=True)[0]
        assert np.max(np.abs(fd - g_noq)) > 1e-4 * np.max(np.abs(g))         # D and E matter at these inputs
        tgt0 = np.stack([frame_velocity(o, j, off, X[t][:o.nq], X[t][o.nq:]) for j, off in frames])
        _, H0 = vel_grad_hess(o, model, X[t], frames, tgt0, w[0][t])

        def grad_at(dx):
            return vel_grad_hess(o, model, tc._integrate_x(o, X[t], dx), frames, tgt0, w[0][t])[0]
        fdh = np.zeros((n, n))
        for j in range(n):
            e = np.zeros(n); e[j] = H
            fdh[:, j] = sum(cw * grad_at(s * e) for s, cw in w5) / H
        assert np.max(np.abs(fdh - H0)) <= 1e-8 * max(1.0, np.max(np.abs(H0))), np.max(np.abs(fdh - H0))
        assert np.array_equal(H0, H0.T)


def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.FLAG_FRAME_VEL_COST == 256 and re.search(r"#define\s+DDP_HIP_FLAG_FRAME_VEL_COST\s+256u", header)
    assert capi.JOINT_REVOLUTE == REVOLUTE
    L = capi.lib()
    for name in ("ddp_hip_frame_vel_upload", "ddp_hip_frame_vel_download", "ddp_hip_model_frame_velocity"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    assert len(capi.SEQ_NAMES) == 40
    assert hasattr(capi.Context, "set_frame_vel_cost") and hasattr(capi.Context, "frame_vel_cost")
    assert hasattr(capi.ModelHandle, "frame_velocity")
    # shapes are checked before anything reaches the library: a context object without a device will do
    T, B, F = 5, 2, 3
    model, spec, _ = make("chain6", T, batch=B, fd_mode=0)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx._h, ctx.n_cost_frames = spec, B, None, F
    for kw in (dict(target=np.zeros((T, F, 6))), dict(target=np.zeros(6)), dict(target=0.0), dict(target=np.zeros((B + 1, T + 1, F, 6))),
               dict(target=np.zeros((T + 1, F + 1, 6))), dict(weight=np.zeros((T + 1, F, 3))), dict(weight=np.zeros(3)),
               dict(weight=np.zeros((B, T + 1, F, 6)), count=1), dict(target=np.zeros((T + 1, F, 6)), weight=np.zeros((T, F, 6)))):
        with pytest.raises(ValueError):
            ctx.set_frame_vel_cost(**kw)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_model_frame_velocity(gpu, name):
    """ddp_hip_model_frame_velocity: the traversal on the device in isolation, vel6, Jq and Jv against the yardstick to 1e-12"""
    capi = gpu
    model, _, o = make_any(name, 2, fd_mode=0)
    frames = fc.pick_frames(model, 3)
    rng = np.random.default_rng(5)
    with capi.ModelHandle(model) as h:
        for k in range(3):
            q, v = rng.normal(size=o.nq), rng.normal(size=o.nv)
            if o.nq != o.nv:
                q[3:7] /= np.linalg.norm(q[3:7])
            j, off = frames[k]
            vel, Jq, Jv = h.frame_velocity(j, off, q, v, jacobian=True)
            vel_only = h.frame_velocity(j, off, q, v)
            ev, eq, ej = (rel_err(a, b) for a, b in zip((vel, Jq, Jv), vel_jacobians(o, model, j, off, q, v)))
            print("model_frame_velocity", name, k, ev, eq, ej)
            assert np.array_equal(vel, vel_only)
            assert np.max(np.abs(Jv)) > 0 and (np.max(np.abs(Jq)) > 0 or k == 0)    # (tree38's joint 0 is prismatic: no D, no E)
            assert ev <= 1e-12 and eq <= 1e-12 and ej <= 1e-12, (ev, eq, ej)


LIN_CASES = [("chain6", 2, None, ""), ("tree38", 2, None, ""), ("chain6ff", 2, 0, ""), ("tree38ff", 0, 0, "nt"),
             ("table7", 2, None, ""), ("tree38", 2, None, "all")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_,flags", LIN_CASES)
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, name, fd_mode, fo_, flags, stages):
    """LX, LXX, LFX, LFXX against the flag-off values plus the definition's terms, batch 3 with different targets and weights
    per instance, through ddp_hip_linearize and ddp_hip_linearize_stages(LIN_COST); LXX / LFXX symmetric bit for bit; LU, LUU,
    LUX and every row and column off the frames' paths bit for bit the flag-off values.  "all": tracking, frame positions, frame
    orientations, state limits and the CoM cost live beside it"""
    capi = gpu
    T, B = 6, 3
    model, spec, o = make_any(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    frames = fc.pick_frames(model, 3)
    xs, us = _trajs(o, model, B, 41)
    tgt, w = random_task(o, xs, frames, B, 42)
    w[1, 2, 1, 1] = 0.0; w[0, T, 2, 5] = 0.0; w[0, 1, 0, 3] = 0.0   # single zero weights among the others
    w[2, :, 0, 3:] = 0.0                                # one frame with only linear weights, at every t for one instance
    w[2, :, 1, :3] = 0.0                                # one frame with only angular weights
    w[0, 3, 2, :] = 0.0                                 # one frame off at one (instance, t)
    w[1, 4, :, :] = 0.0                                 # one (instance, t) with all weights off
    ref = tc.random_ref(o, model, xs, us, B, 44)
    ftask = fc.random_task(o, xs, frames, B, 45)
    otask = fo.random_orient(o, xs, frames, B, 47)
    lim = sl.random_limits(o, xs, B, 46)
    ctask = cm.random_task(o, model, xs, B, 48)
    base = capi.FLAG_FRAME_COST | (capi.FLAG_NO_TENSORS if flags == "nt" else 0)
    if flags == "all":
        base |= capi.FLAG_TRACKING_COST | capi.FLAG_FRAME_ORIENT_COST | capi.FLAG_STATE_LIMITS | capi.FLAG_COM_COST
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (capi.FLAG_FRAME_VEL_COST if on else 0)) as ctx:
            _setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
            ctx.set_frame_cost(frames=frames)
            if flags == "all":
                tc.upload_ref(ctx, ref)
                ctx.set_frame_cost(target=ftask[0], weight=ftask[1])
                ctx.set_frame_orient_cost(quat=otask[0], weight=otask[1])
                ctx.set_state_limits(lo=lim[0], hi=lim[1], weight=lim[2])
                ctx.set_com_cost(target=ctask[0], weight=ctask[1])
            if on:
                ctx.set_frame_vel_cost(target=tgt, weight=w)
            ctx.linearize(None if stages is None else capi.LIN_COST)
            got[on] = {s: ctx.download(s) for s in DERIVS}
    n, nv = o.n, o.nv
    off_path = ~path_rows(o, model, frames)
    worst = 0.0
    for b in range(B):
        add = vel_derivs(o, model, xs[b], frames, tgt[b], w[b])
        for s in ("LX", "LXX", "LFX", "LFXX"):
            ex = got[False][s][b] + add[s]
            assert np.max(np.abs(add[s])) > 0
            worst = max(worst, rel_err(got[True][s][b], ex))
            assert rel_err(got[True][s][b], ex) <= 1e-12, (s, b, rel_err(got[True][s][b], ex))
        assert np.max(np.abs(add["LXX"].reshape(T, n, n)[:, nv:, :nv])) > 0        # the q-v coupling is there
        for s in ("LU", "LUU", "LUX"):
            assert np.array_equal(got[True][s][b], got[False][s][b]), s
        for t in range(T + 1):
            key, k = ("LXX", t) if t < T else ("LFXX", 0)
            blk = got[True][key][b][k * n * n:(k + 1) * n * n].reshape(n, n)
            off = got[False][key][b][k * n * n:(k + 1) * n * n].reshape(n, n)
            assert np.array_equal(blk, blk.T)
            assert np.array_equal(blk[off_path, :], off[off_path, :]) and np.array_equal(blk[:, off_path], off[:, off_path])
            gk, go = ("LX", t) if t < T else ("LFX", 0)
            gon, goff = got[True][gk][b][go * n:(go + 1) * n], got[False][gk][b][go * n:(go + 1) * n]
            assert np.array_equal(gon[off_path], goff[off_path])
            if b == 1 and t == 4:                       # the (instance, t) whose weights are all 0 is untouched
                assert np.array_equal(blk, off) and np.array_equal(gon, goff)
            else:
                assert not np.array_equal(blk, off)
    print("linearize", name, flags, stages, "worst", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_", [("tree38", 0, None), ("chain6ff", 0, 0), ("chain6", 2, None), ("tree38_frame", 0, None)])
def test_cost_seq_aug(gpu, name, fd_mode, fo_):
    """COSTS_OLD / COSTS_NEW (which = 0 / 1) against the oracle's augmented cost plus the numpy terms, lf included"""
    capi = gpu
    T, B, mu = 12, 2, 30.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    frames = fc.pick_frames(model, 3)
    xs, us = _trajs(o, model, B, 51)
    xs2, us2 = _trajs(o, model, B, 61)
    tgt, w = random_task(o, xs, frames, B, 52)
    w[1, 3, :, :] = 0.0
    w[0, 5, 1, :] = 0.0
    w[0, :, 2, 3:] = 0.0
    w[1, :, 0, :3] = 0.0
    mults = tc._mults(o, xs[0], 53)
    with capi.Context(spec, flags=_on(capi) | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
        ctx.set_frame_cost(frames=frames)
        ctx.set_frame_vel_cost(target=tgt, weight=w)
        ctx.cost_seq_aug(0, mu)
        ctx.cost_seq_aug(1, mu)
        got = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
    for which, (X, U) in ((0, (xs, us)), (1, (xs2, us2))):
        for b in range(B):
            add = vel_terms(o, X[b], frames, tgt[b], w[b])
            ex = o.cost_seq_aug(X[b], U[b], mults, mu) + add
            assert got[which][b][T] != 0.0 and add[T] != 0.0
            assert rel_err(got[which][b], ex) <= 1e-12, (which, b, rel_err(got[which][b], ex))


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,mu", [("tree38", 60, 1.0), ("chain6", 30, 10.0)])
def test_sweep_parity_nonzero_value(gpu, name, T, mu):
    """the backward sweep with the q-v block of the frame-velocity cost in LXX: Oracle.backward on the flag-off device
    derivatives plus the yardstick's terms against the device sweep with the flag on: restarts, mu and reg identical, every
    step redone alone by the oracle from the device's V(t+1) lands on the device's k_t, K_t, V_x(t), V_xx(t) to 1e-10
    (stepwise_backward_check).  Tree38 at T = 60 runs on K3h"""
    from oracle.binding import Oracle
    capi = gpu
    model, spec, o = make(name, T, fd_mode=2)
    frames = fc.pick_frames(model, 3)
    xs, us = _trajs(o, model, 1, 71, held=True)
    xs = _moving(xs, o, 74, sigma=0.1)
    tgt, w = random_task(o, xs, frames, 1, 72, wscale=0.1, spread=0.05)
    mults = tc._mults(o, xs[0], 73)
    n, m = o.n, o.m
    d = o.alloc_derivs()
    with capi.Context(spec, flags=capi.FLAG_FRAME_COST | capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.set_frame_cost(frames=frames)
        ctx.linearize()
        for k, s in NAMES.items():
            if ctx.seq_size(s):
                d[k][:ctx.seq_size(s)] = ctx.download(s)[0]
    add = vel_derivs(o, model, xs[0], frames, tgt[0], w[0])
    for k, s in (("lx", "LX"), ("lxx", "LXX"), ("lfx", "LFX"), ("lfxx", "LFXX")):
        d[k][:add[s].size] += add[s]
    assert np.max(np.abs(add["LXX"].reshape(T, n, n)[:, o.nv:, :o.nv])) > 0
    with capi.Context(spec, flags=_on(capi) | capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.set_frame_cost(frames=frames)
        ctx.set_frame_vel_cost(target=tgt, weight=w)
        ctx.linearize()
        if name == "tree38":
            assert ctx.bwd_stream_bytes() == tc._k3h_bytes(n, m)
        for s in ("LX", "LXX", "LFX", "LFXX"):
            assert rel_err(ctx.download(s)[0], d[{v: k for k, v in NAMES.items()}[s]][:ctx.seq_size(s)]) <= 1e-12, s
        rc, reg, mu_out, restarts = ctx.backward(0.0, mu)
        ref_b = o.backward(d, xs[0], mults, 0.0, mu)
        print("sweep", name, "device restarts", int(restarts[0]), "oracle", ref_b["restarts"], "mu", mu_out[0], ref_b["mu"], "reg", reg[0], ref_b["reg"])
        assert int(restarts[0]) == ref_b["restarts"] and mu_out[0] == ref_b["mu"] and reg[0] == ref_b["reg"]
        got = {s: ctx.download(s)[0] for s in ("FB_JAC", "FB_VAL", "VX_TRACE", "VXX_TRACE")}
    assert np.max(np.abs(got["VX_TRACE"])) > 0

    def one_step_oracle(t):
        e = int(o.ne[t])
        if not e:
            return Oracle(model, 1, dt=0.01, c=1.0, fd_mode=2)
        return Oracle(model, 1, dt=0.01, c=1.0, fd_mode=2, eq_kind=spec.eq_kind, eq_advance=2, ne=np.array([e], dtype=np.int64),
                      eq_target=np.zeros(e))
    worst = stepwise_backward_check(one_step_oracle, o, d, xs[0], mults, reg[0], mu_out[0], got["VX_TRACE"], got["VXX_TRACE"],
                                    got["FB_VAL"], got["FB_JAC"], range(T))
    print("stepwise worst", worst)
    assert worst < 1e-10, worst


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,fd_mode,fo_,extra,fwd_path", [
    ("tree38", 24, 2, None, "", 1),                 # latency forward
    ("chain6ff", 10, 2, 0, "", 0),                  # lane-per-rollout forward
    ("tree38_frame", 24, 0, None, "", 1),           # constrained: the candidates' costs from cand_cost_kernel
    ("tree38", 24, 2, None, "box", 1),
])
@pytest.mark.parametrize("mode", ["nothing", "zero_weights", "zero_instance"])
def test_zero_weights_change_nothing(gpu, name, T, fd_mode, fo_, extra, fwd_path, mode):
    """flag on with nothing uploaded, or targets far away but every weight 0: bit for bit what the FLAG_FRAME_COST context
    computes.  zero_instance: batch 2, instance 1 carries non-zero weights (the kernels run), instance 0 none: instance 0 is bit
    for bit the flag-off context's instance 0"""
    capi = gpu
    mu = 10.0
    B = 2 if mode == "zero_instance" else 1
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    frames = fc.pick_frames(model, 3)
    xs, us = _trajs(o, model, B, 31, held=True)
    mults = tc._mults(o, xs[0], 32)
    tgt, w = random_task(o, xs, frames, B, 33, spread=1.0)
    if mode == "zero_instance":
        w[0] = 0.0
        w *= 0.05
    else:
        w[:] = 0.0
    base = capi.FLAG_FRAME_COST | capi.FLAG_TRACE | (capi.FLAG_CONTROL_BOUNDS if extra == "box" else 0)
    out = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (capi.FLAG_FRAME_VEL_COST if on else 0)) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            _setup(ctx, xs, us, mults, o.Etot)
            ctx.set_frame_cost(frames=frames)
            if extra == "box":
                ctx.set_control_bounds(lo=-1e6, hi=1e6)
            if on and mode != "nothing":
                ctx.set_frame_vel_cost(target=tgt, weight=w)
            out[on] = fc._run_all(ctx, mu, name == "tree38")
    a, b = out[False], out[True]
    if mode == "zero_instance":
        assert not np.array_equal(a["LX"][1], b["LX"][1])            # the terms are there for instance 1
        assert not np.array_equal(a["COSTS_OLD"][1], b["COSTS_OLD"][1])
        a = {k: (tuple(np.asarray(v)[..., :1] for v in a[k][1:]) if isinstance(a[k], tuple) else (a[k][:1] if k != "stream" else a[k])) for k in a}
        b = {k: (tuple(np.asarray(v)[..., :1] for v in b[k][1:]) if isinstance(b[k], tuple) else (b[k][:1] if k != "stream" else b[k])) for k in b}
    fc._same(a, b)
    assert np.all(np.isfinite(b["LX"])) and np.all(np.isfinite(b["X_NEW"]))


FORWARD_CASES = [c + (False,) for c in cm.FORWARD_CASES] + [("tree38", None, 1, "", 8, 3.0, True)]
# Weights of 50: the terms are material in every candidate's cost (1e3 .. 1e5 of some 6e6) and the 3 x overshoot is rejected at
# the full step, so the halving runs; with weights of 200 (box) or 2000 the velocity gains are so stiff that the overshot full
# step of tree38 diverges (states of 1e10 .. 1e12 within 16 steps, on the oracle's rollout alone), and a rollout that grows by
# 1e12 amplifies the last-bit differences between any two correct rollouts beyond the 1e-9 the comparison asks: FWD_XMAX is
# asserted on the emulation
FWD_WSCALE, FWD_SPREAD, FWD_XMAX = 50.0, 0.02, 1e4


def _forward_inputs(name, fo_):
    T = 16
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo_)
    frames = fc.pick_frames(model, 3)
    xs, us = _trajs(o, model, 1, 81, held=True)
    tgt, w = random_task(o, xs, frames, 1, 82, wscale=FWD_WSCALE, spread=FWD_SPREAD)
    ctask = cm.random_task(o, model, xs, 1, 86, wscale=2000.0, spread=0.02)
    mults = tc._mults(o, xs[0], 85)
    return T, model, spec, o, frames, xs, us, tgt, w, ctask, mults


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_,fwd_path,extra,n_alpha,k_scale,with_com", FORWARD_CASES)
def test_forward_matches_emulation(gpu, name, fo_, fwd_path, extra, n_alpha, k_scale, with_com):
    """accepted step, X_NEW, U_NEW and dcost against Oracle.forward_alpha rollouts costed with numpy, the frame-velocity terms
    included; k_scale 3 overshoots so that the halving runs; box: control bounds that bind on every third control (the emulation
    clamps); with_com: the CoM cost live as well (both sums are added).  The device adds the terms' sum in another association
    than the emulation: the test first asserts, on the emulation alone, that every candidate tried decides by more than 1e-9 of
    the sum of the cost terms' magnitudes, and only then compares decisions"""
    capi = gpu
    mu = 1.0
    T, model, spec, o, frames, xs, us, tgt, w, ctask, mults = _forward_inputs(name, fo_)
    blo = bhi = None
    flags = _on(capi) | capi.FLAG_NO_TENSORS | (capi.FLAG_CONTROL_BOUNDS if extra == "box" else 0) | (capi.FLAG_COM_COST if with_com else 0)
    with capi.Context(spec, flags=flags) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.set_frame_cost(frames=frames)
        ctx.set_frame_vel_cost(target=tgt, weight=w)
        if with_com:
            ctx.set_com_cost(target=ctask[0], weight=ctask[1])
        ctx.linearize()
        _, _, mu_o, _ = ctx.backward(0.0, mu)
        if k_scale != 1.0:
            ctx.upload("FB_VAL", k_scale * ctx.download("FB_VAL"))
        fb = {"origin": ctx.download("FB_ORIGIN")[0], "val": ctx.download("FB_VAL")[0], "jac": ctx.download("FB_JAC")[0]}
        if extra == "box":
            rng = np.random.default_rng(83)
            width = 0.5 * np.abs(fb["val"]).reshape(T, o.m) / k_scale
            tight = (np.arange(o.m) % 3 == 0)[None, :]
            blo = np.where(tight, us[0].reshape(T, o.m) - width * rng.uniform(0.2, 1, size=(T, o.m)), -np.inf)
            bhi = np.where(tight, us[0].reshape(T, o.m) + width * rng.uniform(0.2, 1, size=(T, o.m)), np.inf)
            ctx.set_control_bounds(lo=blo, hi=bhi)
        rc, step, dcost = ctx.forward(mu_o, n_alpha=n_alpha)
        xn, un = ctx.download("X_NEW")[0], ctx.download("U_NEW")[0]

    def cost(X, U):
        c = o.cost_seq_aug(X, U, mults, mu_o[0]) + vel_terms(o, X, frames, tgt[0], w[0])
        return c + cm.com_terms(o, model, X, ctask[0][0], ctask[1][0]) if with_com else c
    em = cm._emulate_forward(o, xs[0], us[0], mults, fb, mu_o[0], n_alpha, cost, blo, bhi)
    assert em is not None
    step_ref, xn_ref, un_ref, new, margins = em
    print("forward", name, extra, n_alpha, k_scale, with_com, "step", step[0], step_ref, "dcost", dcost[0], new, "margins", margins)
    assert min(margins) > 1e-9, margins               # a condition on the inputs: the decisions do not hang on rounding
    assert np.max(np.abs(xn_ref)) < FWD_XMAX          # ... and the rollout compared has not diverged (FWD_WSCALE's comment)
    assert step[0] == step_ref, (step, step_ref)
    if extra == "box":
        Un = un.reshape(T, o.m)
        assert np.any(Un == blo) or np.any(Un == bhi)
    assert rel_err(xn, xn_ref) < 1e-9 and rel_err(un, un_ref) < 1e-9
    assert abs(dcost[0] - new) <= 1e-9 * max(1.0, abs(new)), (dcost[0], new)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_,flags", [("chain6ff", 2, 0, 0), ("tree38", 0, 0, 1)])
def test_instances_are_independent(gpu, name, fd_mode, fo_, flags):
    """batch 3 through linearise, both costs, sweep, forward: instance 1 computed alone equals its values in the batch bit for bit"""
    capi = gpu
    T, B, mu = 12, 3, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    _, spec1, _ = make(name, T, batch=1, fd_mode=fd_mode, first_order_fd=fo_)
    frames = fc.pick_frames(model, 3)
    xs, us = _trajs(o, model, B, 91, held=True)
    tgt, w = random_task(o, xs, frames, B, 92, wscale=10.0, spread=0.05)
    out = []
    for sp, s_ in ((spec, slice(0, B)), (spec1, slice(1, 2))):
        with capi.Context(sp, flags=_on(capi) | capi.FLAG_TRACE | flags) as ctx:
            _setup(ctx, xs[s_], us[s_])
            ctx.set_frame_cost(frames=frames)
            ctx.set_frame_vel_cost(target=tgt[s_], weight=w[s_])
            out.append(fc._run_all(ctx, mu, False))
    a, b = out
    assert not np.array_equal(a["LX"][1], a["LX"][0])
    for k in a:
        if isinstance(a[k], tuple):
            for u, v in zip(a[k][1:], b[k][1:]):
                assert np.array_equal(np.asarray(u)[1], np.asarray(v)[0]), k
        else:
            assert np.array_equal(a[k][1], b[k][0]), k


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,flags", [("chain6", 2, 0), ("tree38", 0, 1)])
def test_solve_matches_stepwise(gpu, name, fd_mode, flags):
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B, iters, thr, mu, w_, n_ = 10, 2, 5, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode)
    frames = fc.pick_frames(model, 3)
    xs, us = _trajs(o, model, B, 101, held=True)
    tgt, w = random_task(o, xs, frames, B, 102, wscale=10.0)
    mults = tc._mults(o, xs[0], 103)

    def run(stepwise):
        with capi.Context(spec, flags=_on(capi) | flags) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if o.Etot:
                ctx.upload("MULT_ORIGIN", xs[:, :T * o.nx])
            ctx.set_frame_cost(frames=frames)
            ctx.set_frame_vel_cost(target=tgt, weight=w)
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
def test_refusals_and_defaults(gpu):
    import ctypes as C
    capi = gpu
    T, B, F = 4, 3, 3
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    frames = fc.pick_frames(model, F)
    L = capi.lib()
    dp = C.POINTER(C.c_double)

    def code(fn):
        with pytest.raises(capi.DdpHipError) as exc:
            fn()
        return exc.value.code
    with capi.Context(spec, flags=capi.FLAG_FRAME_COST) as ctx:       # a context without the flag
        ctx.set_frame_cost(frames=frames)
        assert code(lambda: ctx.set_frame_vel_cost(weight=1.0)) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.frame_vel_cost()) == capi.E_UNSUPPORTED
    with pytest.raises(capi.DdpHipError) as exc:                      # the flag without the frames' flag
        capi.Context(spec, flags=capi.FLAG_FRAME_VEL_COST)
    assert exc.value.code == capi.E_ARG
    pend = capi.BuiltinModel(capi.BUILTIN_PENDULUM)
    with pytest.raises(capi.DdpHipError) as exc:
        capi.Context(capi.ProblemSpec(pend, T, fd_mode=2), flags=_on(capi))
    assert exc.value.code == capi.E_UNSUPPORTED
    with capi.Context(spec, flags=_on(capi)) as ctx:
        z = np.zeros(B * (T + 1) * F * 6)
        assert L.ddp_hip_frame_vel_upload(ctx._h, z.ctypes.data_as(dp), z.ctypes.data_as(dp), 0, B) == capi.E_ARG   # no frames yet
        ctx.set_frame_cost(frames=frames)
        t0, w0 = ctx.frame_vel_cost()                                   # create: targets 0, weights 0
        assert t0.shape == (B, T + 1, F, 6) and np.all(t0 == 0.0) and np.all(w0 == 0.0)
        rng = np.random.default_rng(5)
        tg, wg = rng.normal(size=(B, T + 1, F, 6)), rng.uniform(0, 1, size=(B, T + 1, F, 6))
        ctx.set_frame_vel_cost(target=tg, weight=wg)
        for bad in (-1e-3, np.nan, np.inf):
            wb = np.ones((T + 1, F, 6)); wb[1, 2, 4] = bad
            assert code(lambda: ctx.set_frame_vel_cost(weight=wb)) == capi.E_ARG, bad
            assert code(lambda: ctx.set_frame_vel_cost(target=np.zeros((T + 1, F, 6)), weight=wb)) == capi.E_ARG, bad
        for bad in (np.nan, -np.inf):
            tb = np.ones((T + 1, F, 6)); tb[2, 1, 3] = bad
            assert code(lambda: ctx.set_frame_vel_cost(target=tb, weight=1.0)) == capi.E_ARG, bad
        assert code(lambda: ctx.set_frame_vel_cost(weight=0.0, first=B, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_frame_vel_cost(weight=0.0, first=-1, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_frame_vel_cost(weight=0.0, first=1, count=B)) == capi.E_ARG
        assert code(lambda: ctx.frame_vel_cost(first=1, count=B)) == capi.E_ARG
        assert L.ddp_hip_frame_vel_upload(ctx._h, z.ctypes.data_as(dp), z.ctypes.data_as(dp), 0, B + 1) == capi.E_ARG
        t1, w1 = ctx.frame_vel_cost()
        assert np.array_equal(t1, tg) and np.array_equal(w1, wg)        # a refused upload leaves both sides as they were
        ctx.set_frame_vel_cost(target=tg[1] + 1.0, first=1, count=1)    # one side, one instance; the weights stay
        t1, w1 = ctx.frame_vel_cost()
        assert np.array_equal(t1[0], tg[0]) and np.array_equal(t1[1], tg[1] + 1.0) and np.array_equal(t1[2], tg[2]) and np.array_equal(w1, wg)
        t2, w2 = ctx.frame_vel_cost(first=1, count=2)                   # the round trip of a range of instances
        assert np.array_equal(t2, t1[1:]) and np.array_equal(w2, wg[1:])
        six = np.array([1.0, 2.0, 0.0, 0.5, 0.0, 3.0])
        ctx.set_frame_vel_cost(weight=six, first=1, count=2)            # broadcast: (6,) and scalar
        assert np.array_equal(ctx.frame_vel_cost()[1][1:], np.broadcast_to(six, (2, T + 1, F, 6)))
        assert np.array_equal(ctx.frame_vel_cost()[1][0], wg[0])
        ctx.set_frame_vel_cost(weight=0.5)
        assert np.all(ctx.frame_vel_cost()[1] == 0.5)
        ctx.set_frame_cost(frames=[(j, tuple(2 * x for x in off)) for j, off in frames])   # the same count: the data stays
        assert np.all(ctx.frame_vel_cost()[1] == 0.5) and np.array_equal(ctx.frame_vel_cost()[0], t1)
        ctx.set_frame_cost(frames=frames[:2])                           # another count: back to 0
        t3, w3 = ctx.frame_vel_cost()
        assert t3.shape == (B, T + 1, 2, 6) and np.all(t3 == 0.0) and np.all(w3 == 0.0)
        ctx.linearize()                                                 # and the terms are off: the frame-cost context's values
        lx_on = ctx.download("LX")
    with capi.Context(spec, flags=capi.FLAG_FRAME_COST) as ctx:
        ctx.set_frame_cost(frames=frames[:2])
        ctx.linearize()
        assert np.array_equal(ctx.download("LX"), lx_on)


@pytest.mark.gpu
def test_velocity_task_descends(gpu):
    """tree38, T = 20, held trajectory; one hand frame is asked to move at 0.05 m/s along world x with zero angular velocity at
    every t, the terminal weight 10 x larger: over ten iterations the total cost never increases over accepted steps and the
    velocity residual at t = T/2 ends smaller than it started"""
    capi = gpu
    T, mu, iters = 20, 1.0, 10
    model, spec, o = make("tree38", T, fd_mode=0)
    frames = fc.pick_frames(model, 1)
    j, off = frames[0]
    xs, us = _trajs(o, model, 1, 111, held=True)
    goal = np.array([0.05, 0.0, 0.0, 0.0, 0.0, 0.0])
    tgt = np.tile(goal, (T + 1, 1, 1))
    # the held posture costs c/2 |u|^2 of some 4e5 per step in gravity torques (test_com_shift_descends): a residual of 0.05 m/s
    # weighs 1/2 w 0.0025, so weights below 1e8 leave the term a rounding error beside it and the cheapest trajectory is to let
    # go and fall
    w = np.full((T + 1, 1, 6), 1e9)
    w[T] = 1e10

    def err(X):
        x = X.reshape(T + 1, o.nx)[T // 2]
        return np.linalg.norm(frame_velocity(o, j, off, x[:o.nq], x[o.nq:]) - goal)
    with capi.Context(spec, flags=_on(capi) | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        ctx.set_frame_cost(frames=frames)
        ctx.set_frame_vel_cost(target=tgt, weight=w)
        costs, steps = [], []
        for _ in range(iters):
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            rc, step, dcost = ctx.forward(mu_o, n_alpha=8)
            costs.append(ctx.download("COSTS_OLD")[0].sum())
            steps.append(step[0])
            ctx.swap_traj()
        final = ctx.download("X")[0]
    print("velocity task costs", costs, "steps", steps, "error", err(xs[0]), "->", err(final))
    for a, b in zip(costs, costs[1:]):
        assert b <= a * (1 + 1e-12), costs
    assert costs[-1] < costs[0]
    assert err(final) < err(xs[0]), (err(xs[0]), err(final))
