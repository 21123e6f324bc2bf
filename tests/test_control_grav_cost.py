"""Per-instance gravity-compensated control costs (DDP_HIP_FLAG_CONTROL_GRAV_COST, include/ddp_hip/ddp_hip.h):

    r = u_t - g(q_t) - o[b][t],   l(t, x, u) += 1/2 sum_j w[b][t][j] r_j^2,  t < T;   aba(q, 0, g(q)) = 0

The oracle has no such cost, so the yardstick is the numpy restatement below, by another route than the device's subtree sweep:
the potential energy V(q) = -sum_b m_b gravity . p_b(q) body by body, g = dV/d(delta q) = -sum_b m_b P_b^T gravity with the
oracle's point jacobians P_b of the bodies' centres of mass, and G = dg/d(delta q) from the derivative of a point jacobian's
column, d P_b[:, i] / d(delta q_j) = W_b[:, lo] x P_b[:, hi] (lo: the ancestor of the two, W_b the world angular jacobian).
test_yardstick_pins holds g against the oracle's own dynamics and G against central differences of g.  The helpers of the other
cost terms' tests are reused by import; tolerances are theirs."""
import os
import re
import subprocess

import numpy as np
import pytest

import test_com_cost as cm
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 1e-3
DERIVS = fc.DERIVS
NAMES = fc.NAMES
MODELS = fv.MODELS
make_any = cm.make_any
_trajs, _setup, _moving = tc._trajs, tc._setup, fv._moving
REVOLUTE = fv.REVOLUTE


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def tangent_joint(model, k):
    return (0 if k < 6 else k - 5) if model.ff else k


def tangent_rotational(model, k):
    if model.ff and k < 6:
        return k >= 3
    return int(model.jtype[tangent_joint(model, k)]) == REVOLUTE


def pattern(model):
    """(related, formed), nv x nv booleans over (row i, column c).  related: the joints of i and c lie on one root path.  formed:
    the entries the library forms -- of the related ones those whose ancestor side turns what it moves (the column's joint an
    ancestor of the row's or the same joint: the column rotational; a strict descendant: the row rotational); the others are
    identically zero"""
    nv = model.nv
    paths = [set(fv.path_of(model, tangent_joint(model, k))) for k in range(nv)]
    rel, formed = np.zeros((nv, nv), dtype=bool), np.zeros((nv, nv), dtype=bool)
    for i in range(nv):
        for c in range(nv):
            ji, jc = tangent_joint(model, i), tangent_joint(model, c)
            if jc in paths[i]:                       # the column's joint is the row's or an ancestor of it
                rel[i, c], formed[i, c] = True, tangent_rotational(model, c)
            elif ji in paths[c]:
                rel[i, c], formed[i, c] = True, tangent_rotational(model, i)
    return rel, formed


def grav_torque(o, model, q, jacobian=True):
    """(g, G) per body (G None without `jacobian`); G carries exact zeros where the two joints share no root path"""
    m = np.asarray(model.mass_j)
    grav = np.asarray(model.gravity, dtype=np.float64)
    nv = model.nv
    g = np.zeros(nv)
    G = np.zeros((nv, nv)) if jacobian else None
    for b in range(len(m)):
        P = o.frame_jacobian(b, model.com[b], q, world_aligned=True)
        g -= m[b] * (P.T @ grav)
        if not jacobian:
            continue
        W = fo.frame_W(o, b, q, fo.frame_R(o, b, q))
        on = [c for j in fv.path_of(model, b) for c in fv.cols_of(model, j)]
        for i in on:
            for c in on:
                same = tangent_joint(model, i) == tangent_joint(model, c)
                lo, hi = (c, i) if same else (min(i, c), max(i, c))   # on one joint the direction acts first; else the ancestor
                G[i, c] -= m[b] * float(grav @ np.cross(W[:, lo], P[:, hi]))
    return g, G


def cg_terms(o, model, xs, us, off, w):
    """the terms of one instance per t (T+1 values; the last is 0: no control at T); off, w: (T, m).  A weight of 0 is left out"""
    X, U = xs.reshape(o.T + 1, o.nx), us.reshape(o.T, o.m)
    out = np.zeros(o.T + 1)
    for t in range(o.T):
        if not np.any(w[t] != 0.0):
            continue
        r = U[t] - grav_torque(o, model, X[t][:o.nq], jacobian=False)[0] - off[t]
        out[t] = 0.5 * np.sum(w[t] * r * r)
    return out


def cg_derivs(o, model, xs, us, off, w):
    """what the terms add to LU, LUU, LUX, LX, LXX of one instance, in the library's flat (column-major) layout"""
    X, U = xs.reshape(o.T + 1, o.nx), us.reshape(o.T, o.m)
    n, m, nv = o.n, o.m, o.nv
    out = {s: [] for s in ("LU", "LUU", "LUX", "LX", "LXX")}
    for t in range(o.T):
        lu, luu, lux, lx, lxx = np.zeros(m), np.zeros((m, m)), np.zeros((m, n)), np.zeros(n), np.zeros((n, n))
        if np.any(w[t] != 0.0):
            g, G = grav_torque(o, model, X[t][:o.nq])
            r = U[t] - g - off[t]
            lu = w[t] * r
            luu = np.diag(w[t])
            lux[:, :nv] = -w[t][:, None] * G
            lx[:nv] = -G.T @ (w[t] * r)
            for i in range(m):                           # entry (a, b) and (b, a) alike: symmetric bit for bit
                lxx[:nv, :nv] += w[t][i] * np.outer(G[i], G[i])
        for s, v in (("LU", lu), ("LUU", luu.ravel(order="F")), ("LUX", lux.ravel(order="F")), ("LX", lx), ("LXX", lxx.ravel(order="F"))):
            out[s].append(v)
    return {s: np.concatenate(v) for s, v in out.items()}


def random_task(o, model, B, seed, wscale=1.0, spread=0.5):
    """offsets and positive weights, each (B, T, m); a free-flyer root's six rows carry no weight"""
    rng = np.random.default_rng(seed)
    off = spread * rng.normal(size=(B, o.T, o.m))
    w = wscale * rng.uniform(0.1, 2.0, size=(B, o.T, o.m))
    if model.ff:
        w[:, :, :6] = 0.0
    return off, w


def _state(o, rng):
    q = rng.normal(size=o.nq)
    if o.nq != o.nv:
        q[3:7] /= np.linalg.norm(q[3:7])
    return q


def FLAG(capi):
    return capi.FLAG_CONTROL_GRAV_COST


# ---- CPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_yardstick_pins(name):
    """(i) the oracle's dynamics at (q, v = 0, u = g_yard(q)) returns the state unchanged: |x+ - x| <= 1e-11 dt max(1, |g|), the
    "few ulp" bound of test_dynamics_parity (1e-11 relative) on an acceleration formed from torques of size |g|, times dt;
    (ii) G_yard against the 5-point central difference of g_yard through the model's integrate, at test_momentum_cost's
    yardstick tolerance; G symmetric on the fixed-base models; exact zeros where two joints share no root path and in a
    free-flyer root's translation columns, and nothing but rounding where the ancestor side is a translation.  A check of the
    numpy restatement alone: it calls nothing of the library's new code"""
    model, _, o = make_any(name, 2, fd_mode=0)
    rng = np.random.default_rng(7)
    nv, dt = o.nv, 0.01
    rel, formed = pattern(model)
    w5 = ((-2, 1.0 / 12), (-1, -8.0 / 12), (1, 8.0 / 12), (2, -1.0 / 12))
    for k in range(2 if nv <= 13 else 1):
        q = _state(o, rng)
        g, G = grav_torque(o, model, q)
        x = np.concatenate([q, np.zeros(nv)])
        xp = o.eval_f(x, g)
        scale = max(1.0, np.max(np.abs(g)))
        print("yardstick", name, "max|g|", np.max(np.abs(g)), "|x+ - x|", np.max(np.abs(xp - x)))
        assert np.max(np.abs(g)) > 1.0
        assert np.max(np.abs(xp - x)) <= 1e-11 * dt * scale, np.max(np.abs(xp - x))
        fd = np.zeros((nv, nv))
        for j in range(nv):
            e = np.zeros(nv); e[j] = H
            fd[:, j] = sum(cw * grav_torque(o, model, o.integrate(q, s * e), jacobian=False)[0] for s, cw in w5) / H
        assert np.max(np.abs(fd - G)) <= 1e-8 * max(1.0, np.max(np.abs(G))), np.max(np.abs(fd - G))
        assert np.all(G[~rel] == 0.0)
        assert np.max(np.abs(G[rel & ~formed]), initial=0.0) <= 1e-12 * np.max(np.abs(G))
        if model.ff:
            assert np.all(G[:, :3] == 0.0)
            assert np.max(np.abs(G[6:, 3:6])) > 0      # turning the base turns gravity in the body
        else:
            assert np.max(np.abs(G - G.T)) <= 1e-12 * np.max(np.abs(G))


def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.FLAG_CONTROL_GRAV_COST == 8192 and re.search(r"#define\s+DDP_HIP_FLAG_CONTROL_GRAV_COST\s+8192u", header)
    L = capi.lib()
    for name in ("ddp_hip_control_grav_cost_upload", "ddp_hip_control_grav_cost_download", "ddp_hip_model_gravity_torque"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    assert len(capi.SEQ_NAMES) == 40
    assert hasattr(capi.Context, "set_control_grav_cost") and hasattr(capi.Context, "control_grav_cost")
    assert hasattr(capi.ModelHandle, "gravity_torque")
    assert fv.REVOLUTE == capi.JOINT_REVOLUTE
    # shapes are checked before anything reaches the library: a context object without a device will do.  The public shape is
    # (T, m): a (T+1, m) array is refused
    T, B = 5, 2
    model, spec, _ = make("chain6", T, batch=B, fd_mode=0)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx._h = spec, B, None
    for kw in (dict(offset=np.zeros((T + 1, 6))), dict(offset=np.zeros(5)), dict(offset=np.zeros((B + 1, T, 6))),
               dict(weight=np.zeros((T + 1, 6))), dict(weight=np.zeros(3)), dict(weight=np.zeros((B, T, 6)), count=1),
               dict(offset=np.zeros((T, 6)), weight=np.zeros((T, 5)))):
        with pytest.raises(ValueError):
            ctx.set_control_grav_cost(**kw)


def test_host_program():
    """host/test_control_grav_block.cpp: the record, the validators, the root-row rule, T against T+1 rows, the live rule"""
    host = os.path.join(ROOT, "host")
    subprocess.run(["make", "-C", host, "test_control_grav_block"], check=True, capture_output=True)
    run = subprocess.run([os.path.join(host, "test_control_grav_block")], capture_output=True, text=True)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout + run.stderr


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_model_gravity_torque(gpu, name):
    """ddp_hip_model_gravity_torque: the traversal on the device in isolation, g and G against the yardstick to 1e-12 (root rows
    included); jacobian=False returns the same g bit for bit; G is 0 off the pattern the library forms, symmetric bit for bit on
    a fixed base"""
    capi = gpu
    model, _, o = make_any(name, 2, fd_mode=0)
    rng = np.random.default_rng(5)
    _, formed = pattern(model)
    with capi.ModelHandle(model) as hd:
        for k in range(3):
            q = _state(o, rng)
            g, G = hd.gravity_torque(q, jacobian=True)
            gy, Gy = grav_torque(o, model, q)
            eg, eG = rel_err(g, gy), rel_err(G, Gy)
            print("model_gravity_torque", name, k, eg, eG)
            assert np.array_equal(g, hd.gravity_torque(q))
            assert eg <= 1e-12 and eG <= 1e-12, (eg, eG)
            assert np.all(G[~formed] == 0.0) and np.any(G[formed] != 0.0)   # (chain6's parallel axes: zeros on the pattern too)
            if not model.ff:
                assert np.array_equal(G, G.T)


LIN_CASES = [("chain6", 2, None, ""), ("tree38", 2, None, ""), ("chain6ff", 2, 0, ""), ("tree38ff", 0, 0, "nt"),
             ("table7", 2, None, ""), ("chain6", 0, None, ""), ("tree38", 2, None, "all")]


def _lin_task(o, model, B, T):
    off, w = random_task(o, model, B, 42)
    j0 = 6 if model.ff else 0
    w[1, 2, :] = 0.0                                     # one (instance, t) with all weights off
    w[0, 1, j0 + 1] = 0.0; w[2, 0, o.m - 1] = 0.0        # single zero weights among the others
    w[2, 3, :] = 0.0; w[2, 3, j0 + 4] = 0.7              # one (instance, t) with a single live row (one with rotational ancestors on every model)
    return off, w


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_,flags", LIN_CASES)
def test_linearize_matches_definition(gpu, name, fd_mode, fo_, flags):
    """LU, LUU, LUX, LX, LXX after linearize against the flag-off values plus the yardstick's five additions (1e-12, the
    linearise tolerance of the momentum and relative-frame tests), batch 3 with different data per instance, fd_mode 0 and 2;
    LFX / LFXX, every velocity row and column, and every entry that no live row reaches -- LUX off the formed pattern, LX / LXX
    where no live row's pattern holds the column(s), a free-flyer root's translation columns among them -- bit for bit the
    flag-off values; LXX symmetric bit for bit; an (instance, t) whose weights are 0 keeps the flag-off bits.  "all": every
    other cost flag live beside it (the term's kernel runs between the relative frames' and the obstacles')"""
    capi = gpu
    T, B = 6, 3
    model, spec, o = make_any(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 41)
    off, w = _lin_task(o, model, B, T)
    frames = fc.pick_frames(model, 3)
    base = capi.FLAG_NO_TENSORS if flags == "nt" else 0
    if flags == "all":
        base |= (capi.FLAG_TRACKING_COST | capi.FLAG_FRAME_COST | capi.FLAG_FRAME_ORIENT_COST | capi.FLAG_FRAME_VEL_COST
                 | capi.FLAG_STATE_LIMITS | capi.FLAG_COM_COST | capi.FLAG_MOMENTUM_COST | capi.FLAG_RELATIVE_FRAME_COST
                 | capi.FLAG_OBSTACLE_COST | capi.FLAG_SELF_COLLISION_COST)
        ref = tc.random_ref(o, model, xs, us, B, 44)
        ftask = fc.random_task(o, xs, frames, B, 45)
        otask = fo.random_orient(o, xs, frames, B, 47)
        vtask = fv.random_task(o, xs, frames, B, 49)
        lim = sl.random_limits(o, xs, B, 46)
        ctask = cm.random_task(o, model, xs, B, 48)
        mtask = mo.random_task(o, model, xs, B, 51)
        pairs = rf.pick_pairs(model)
        rtask = rf._lin_task(o, pairs, xs, B, T)
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
                ctx.set_frame_cost(frames=frames, target=ftask[0], weight=ftask[1])
                ctx.set_frame_orient_cost(quat=otask[0], weight=otask[1])
                ctx.set_frame_vel_cost(target=vtask[0], weight=vtask[1])
                ctx.set_state_limits(lo=lim[0], hi=lim[1], weight=lim[2])
                ctx.set_com_cost(target=ctask[0], weight=ctask[1])
                ctx.set_momentum_cost(target=mtask[0], weight=mtask[1])
                rf.set_task(ctx, pairs, *rtask)
                ob.set_task(ctx, opts, ob.KINDS, *obtask)
                sc.set_task(ctx, opts, scpairs, *sctask)
            if on:
                ctx.set_control_grav_cost(offset=off, weight=w)
            ctx.linearize()
            got[on] = {s: ctx.download(s) for s in DERIVS}
    n, nv, m = o.n, o.nv, o.m
    _, formed = pattern(model)
    worst = 0.0
    for b in range(B):
        add = cg_derivs(o, model, xs[b], us[b], off[b], w[b])
        for s in ("LU", "LUU", "LUX", "LX", "LXX"):
            ex = got[False][s][b] + add[s]
            assert np.max(np.abs(add[s])) > 0
            e = rel_err(got[True][s][b], ex)
            worst = max(worst, e)
            assert e <= 1e-12, (s, b, e)
        for s in ("LFX", "LFXX"):
            assert np.array_equal(got[True][s][b], got[False][s][b]), s
        for t in range(T):
            live = w[b, t] != 0.0
            reach = formed & live[:, None]                                # (row, column): a live row forms the entry
            cols = reach.any(axis=0)                                     # the q columns some live row reaches
            lux_on, lux_off = (got[k]["LUX"][b][t * m * n:(t + 1) * m * n].reshape(n, m).T for k in (True, False))
            lxx_on, lxx_off = (got[k]["LXX"][b][t * n * n:(t + 1) * n * n].reshape(n, n).T for k in (True, False))
            lx_on, lx_off = (got[k]["LX"][b][t * n:(t + 1) * n] for k in (True, False))
            assert np.array_equal(lxx_on, lxx_on.T)
            assert np.array_equal(lux_on[:, nv:], lux_off[:, nv:]) and np.array_equal(lux_on[:, :nv][~reach], lux_off[:, :nv][~reach])
            assert np.array_equal(lx_on[nv:], lx_off[nv:]) and np.array_equal(lx_on[:nv][~cols], lx_off[:nv][~cols])
            shared = (reach[:, :, None] & reach[:, None, :]).any(axis=0)  # (a, b): some live row reaches both
            assert np.array_equal(lxx_on[nv:, :], lxx_off[nv:, :]) and np.array_equal(lxx_on[:, nv:], lxx_off[:, nv:])
            assert np.array_equal(lxx_on[:nv, :nv][~shared], lxx_off[:nv, :nv][~shared])
            if model.ff:
                assert not cols[:3].any() and (cols[3:6].all() or not live.any())
            if b == 1 and t == 2:                        # the (instance, t) whose weights are all 0 is untouched
                for s, sz in (("LU", m), ("LUU", m * m), ("LUX", m * n), ("LX", n), ("LXX", n * n)):
                    assert np.array_equal(got[True][s][b][t * sz:(t + 1) * sz], got[False][s][b][t * sz:(t + 1) * sz]), s
            else:
                assert not np.array_equal(lux_on, lux_off) and not np.array_equal(lxx_on, lxx_off)
    print("linearize", name, fd_mode, flags, "worst", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_", [("tree38", 0, None), ("chain6ff", 0, 0), ("table7", 2, None), ("tree38_frame", 0, None)])
def test_cost_seq_aug(gpu, name, fd_mode, fo_):
    """COSTS_OLD / COSTS_NEW (which = 0 / 1: X with U, X_NEW with U_NEW) against the oracle's augmented cost plus the numpy
    terms; the entry at T is the flag-off one bit for bit (no control there)"""
    capi = gpu
    T, B, mu = 6, 2, 30.0
    model, spec, o = make_any(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 51)
    xs2, us2 = _trajs(o, model, B, 61)
    off, w = random_task(o, model, B, 52)
    w[1, 3, :] = 0.0
    w[0, :, o.m - 2] = 0.0
    mults = tc._mults(o, xs[0], 53)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | (FLAG(capi) if on else 0)) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
            if on:
                ctx.set_control_grav_cost(offset=off, weight=w)
            ctx.cost_seq_aug(0, mu)
            ctx.cost_seq_aug(1, mu)
            got[on] = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
    for which, (X, U) in ((0, (xs, us)), (1, (xs2, us2))):
        for b in range(B):
            add = cg_terms(o, model, X[b], U[b], off[b], w[b])
            ex = o.cost_seq_aug(X[b], U[b], mults, mu) + add
            assert np.all(add[:T][np.arange(T) != 3 if b == 1 else slice(None)] > 0) and add[T] == 0.0
            assert rel_err(got[True][which][b], ex) <= 1e-12, (which, b, rel_err(got[True][which][b], ex))
            assert got[True][which][b][T] == got[False][which][b][T]
            if b == 1:
                assert got[True][which][b][3] == got[False][which][b][3]


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,mu", [("tree38", 60, 1.0), ("chain6", 30, 10.0)])
def test_sweep_parity(gpu, name, T, mu):
    """the backward sweep with the term live, the first with LUX != 0: Oracle.backward on the flag-off device derivatives plus
    the yardstick's terms against the device sweep with the flag on: restarts, mu and reg identical, every step redone alone by
    the oracle from the device's V(t+1) lands on the device's k_t, K_t, V_x(t), V_xx(t) to 1e-10 (stepwise_backward_check)"""
    from oracle.binding import Oracle
    capi = gpu
    model, spec, o = make(name, T, fd_mode=2)
    xs, us = _trajs(o, model, 1, 71, held=True)
    off, w = random_task(o, model, 1, 72, wscale=0.01, spread=0.5)
    mults = tc._mults(o, xs[0], 73)
    d = o.alloc_derivs()
    with capi.Context(spec, flags=capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.linearize()
        for k, s in NAMES.items():
            if ctx.seq_size(s):
                d[k][:ctx.seq_size(s)] = ctx.download(s)[0]
    add = cg_derivs(o, model, xs[0], us[0], off[0], w[0])
    back = {v: k for k, v in NAMES.items()}
    for s in add:
        d[back[s]][:add[s].size] += add[s]
    with capi.Context(spec, flags=FLAG(capi) | capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.set_control_grav_cost(offset=off, weight=w)
        ctx.linearize()
        assert np.max(np.abs(ctx.download("LUX")[0])) > 0
        for s in add:
            assert rel_err(ctx.download(s)[0], d[back[s]][:ctx.seq_size(s)]) <= 1e-12, s
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
@pytest.mark.parametrize("name,T,fd_mode,fo_,fwd_path", [
    ("tree38", 24, 2, None, 1),                     # latency forward
    ("chain6ff", 10, 2, 0, 0),                      # lane-per-rollout forward
])
@pytest.mark.parametrize("mode", ["nothing", "zero_weights", "zero_instance"])
def test_zero_weights_change_nothing(gpu, name, T, fd_mode, fo_, fwd_path, mode):
    """flag on with nothing uploaded, or offsets far away but every weight 0: linearise, both costs, sweep and forward bit for
    bit what the flag-off context computes.  zero_instance: batch 2, instance 1 carries non-zero weights (the kernels run),
    instance 0 none: instance 0 is bit for bit the flag-off context's instance 0"""
    capi = gpu
    mu = 10.0
    B = 2 if mode == "zero_instance" else 1
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 31, held=True)
    mults = tc._mults(o, xs[0], 32)
    off, w = random_task(o, model, B, 33, wscale=0.01, spread=5.0)
    if mode == "zero_instance":
        w[0] = 0.0
    else:
        w[:] = 0.0
    out = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_TRACE | (FLAG(capi) if on else 0)) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            _setup(ctx, xs, us, mults, o.Etot)
            if on and mode != "nothing":
                ctx.set_control_grav_cost(offset=off, weight=w)
            out[on] = fc._run_all(ctx, mu, name == "tree38")
    a, b = out[False], out[True]
    if mode == "zero_instance":
        assert not np.array_equal(a["LUX"][1], b["LUX"][1])          # the terms are there for instance 1
        assert not np.array_equal(a["COSTS_OLD"][1], b["COSTS_OLD"][1])
        a = {k: (tuple(np.asarray(v)[..., :1] for v in a[k][1:]) if isinstance(a[k], tuple) else (a[k][:1] if k != "stream" else a[k])) for k in a}
        b = {k: (tuple(np.asarray(v)[..., :1] for v in b[k][1:]) if isinstance(b[k], tuple) else (b[k][:1] if k != "stream" else b[k])) for k in b}
    fc._same(a, b)
    assert np.all(np.isfinite(b["LX"])) and np.all(np.isfinite(b["X_NEW"]))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["nothing", "zero_weights"])
def test_zero_weights_change_nothing_solve(gpu, mode):
    """... and a whole solve: X, U and the log bit for bit the flag-off context's"""
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B = 10, 2
    model, spec, o = make("chain6", T, batch=B, fd_mode=2)
    xs, us = _trajs(o, model, B, 35, held=True)
    mults = tc._mults(o, xs[0], 36)
    off, _ = random_task(o, model, B, 37, spread=5.0)
    out = {}
    for on in (False, True):
        with capi.Context(spec, flags=FLAG(capi) if on else 0) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if o.Etot:
                ctx.upload("MULT_ORIGIN", xs[:, :T * o.nx])
            if on and mode != "nothing":
                ctx.set_control_grav_cost(offset=off, weight=0.0)
            log = solver.solve(ctx, 4, 1e-9, 1e2, 0.0, 1e-1, 10.0)
            out[on] = (log, ctx.download("X"), ctx.download("U"))
    assert np.array_equal(out[True][1], out[False][1]) and np.array_equal(out[True][2], out[False][2])
    for k in ("iterations", "mu", "reg", "w", "n", "last_step", "opt_obj", "opt_constr"):
        assert np.array_equal(np.asarray(out[True][0][k]), np.asarray(out[False][0][k])), k


# (name, first_order_fd, forward path, n_alpha, k_scale, control bounds)
FORWARD_CASES = [("tree38", None, 1, 1, 1.0, False), ("tree38", None, 1, 8, 3.0, False), ("chain6ff", 0, 0, 1, 1.0, False),
                 ("chain6ff", 0, 0, 8, 3.0, False), ("tree38", None, 1, 8, 1.0, True)]
# G's entries are subtree masses times g times lever arms (some 4e2 on tree38), so a weight of 0.01 gives lxx the curvature a
# frame-velocity weight of some 100 gives (test_frame_vel_cost.FWD_WSCALE: stiffer gains let the overshot full step diverge);
# offsets of some 5 keep the terms material beside c/2 |u|^2.  FWD_XMAX is asserted on the emulation
FWD_WSCALE, FWD_SPREAD, FWD_XMAX = 0.01, 5.0, 1e4


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_,fwd_path,n_alpha,k_scale,box", FORWARD_CASES)
def test_forward_matches_emulation(gpu, name, fo_, fwd_path, n_alpha, k_scale, box):
    """accepted step, X_NEW, U_NEW and dcost against Oracle.forward_alpha rollouts costed with numpy, the terms formed from each
    candidate's own controls; k_scale 3 overshoots so that the halving runs; box: control bounds that bind on every third
    control -- the emulation clamps, and r is formed from the clamped control.  The device adds the terms' sum in another
    association than the emulation: the test first asserts, on the emulation alone, that every candidate tried decides by more
    than 1e-9 of the sum of the cost terms' magnitudes, and only then compares decisions"""
    capi = gpu
    mu = 1.0
    T = 16
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, 1, 81, held=True)
    off, w = random_task(o, model, 1, 82, wscale=FWD_WSCALE, spread=FWD_SPREAD)
    mults = tc._mults(o, xs[0], 85)
    blo = bhi = None
    flags = FLAG(capi) | capi.FLAG_NO_TENSORS | (capi.FLAG_CONTROL_BOUNDS if box else 0)
    with capi.Context(spec, flags=flags) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.set_control_grav_cost(offset=off, weight=w)
        ctx.linearize()
        _, _, mu_o, _ = ctx.backward(0.0, mu)
        if k_scale != 1.0:
            ctx.upload("FB_VAL", k_scale * ctx.download("FB_VAL"))
        fb = {"origin": ctx.download("FB_ORIGIN")[0], "val": ctx.download("FB_VAL")[0], "jac": ctx.download("FB_JAC")[0]}
        if box:
            rng = np.random.default_rng(83)
            width = 0.5 * np.abs(fb["val"]).reshape(T, o.m) / k_scale
            tight = (np.arange(o.m) % 3 == 0)[None, :]
            blo = np.where(tight, us[0].reshape(T, o.m) - width * rng.uniform(0.2, 1, size=(T, o.m)), -np.inf)
            bhi = np.where(tight, us[0].reshape(T, o.m) + width * rng.uniform(0.2, 1, size=(T, o.m)), np.inf)
            ctx.set_control_bounds(lo=blo, hi=bhi)
        rc, step, dcost = ctx.forward(mu_o, n_alpha=n_alpha)
        xn, un = ctx.download("X_NEW")[0], ctx.download("U_NEW")[0]

    def cost(X, U):
        return o.cost_seq_aug(X, U, mults, mu_o[0]) + cg_terms(o, model, X, U, off[0], w[0])
    em = cm._emulate_forward(o, xs[0], us[0], mults, fb, mu_o[0], n_alpha, cost, blo, bhi)
    assert em is not None
    step_ref, xn_ref, un_ref, new, margins = em
    share = cg_terms(o, model, xn_ref, un_ref, off[0], w[0]).sum() / np.sum(np.abs(cost(xn_ref, un_ref)))
    print("forward", name, n_alpha, k_scale, box, "step", step[0], step_ref, "dcost", dcost[0], new, "margins", margins, "share", share)
    assert share > 1e-6                               # the terms are material in the candidate's cost
    assert min(margins) > 1e-9, margins               # a condition on the inputs: the decisions do not hang on rounding
    assert np.max(np.abs(xn_ref)) < FWD_XMAX          # ... and the rollout compared has not diverged
    if k_scale != 1.0:
        assert step_ref < 1.0                         # the halving ran
    assert step[0] == step_ref, (step, step_ref)
    if box:
        Un = un.reshape(T, o.m)
        assert np.any(Un == blo) or np.any(Un == bhi)
        # the unclamped control would give other terms: r is seen to use the clamped one
        raw = o.forward_alpha(step_ref, xs[0], us[0], mults, fb, mu_o[0])[2]
        assert not np.array_equal(raw, un_ref)
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
    xs, us = _trajs(o, model, B, 91, held=True)
    off, w = random_task(o, model, B, 92, wscale=0.01)
    out = []
    for sp, s_ in ((spec, slice(0, B)), (spec1, slice(1, 2))):
        with capi.Context(sp, flags=FLAG(capi) | capi.FLAG_TRACE | flags) as ctx:
            _setup(ctx, xs[s_], us[s_])
            ctx.set_control_grav_cost(offset=off[s_], weight=w[s_])
            out.append(fc._run_all(ctx, mu, False))
    a, b = out
    assert not np.array_equal(a["LUX"][1], a["LUX"][0])
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
    xs, us = _trajs(o, model, B, 101, held=True)
    off, w = random_task(o, model, B, 102, wscale=0.01)
    mults = tc._mults(o, xs[0], 103)

    def run(stepwise):
        with capi.Context(spec, flags=FLAG(capi) | flags) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if o.Etot:
                ctx.upload("MULT_ORIGIN", xs[:, :T * o.nx])
            ctx.set_control_grav_cost(offset=off, weight=w)
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
    T, B = 4, 3
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    m = o.m
    L = capi.lib()
    dp = C.POINTER(C.c_double)

    def code(fn):
        with pytest.raises(capi.DdpHipError) as exc:
            fn()
        return exc.value.code
    with capi.Context(spec) as ctx:                                   # a context without the flag
        assert code(lambda: ctx.set_control_grav_cost(weight=0.0)) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.control_grav_cost()) == capi.E_UNSUPPORTED
    pend = capi.BuiltinModel(capi.BUILTIN_PENDULUM)
    with pytest.raises(capi.DdpHipError) as exc:
        capi.Context(capi.ProblemSpec(pend, T, fd_mode=2), flags=capi.FLAG_CONTROL_GRAV_COST)
    assert exc.value.code == capi.E_UNSUPPORTED
    with capi.Context(spec, flags=capi.FLAG_CONTROL_GRAV_COST) as ctx:  # the flag stands alone
        o0, w0 = ctx.control_grav_cost()                                # create: offsets 0, weights 0; the public shape is (T, m)
        assert o0.shape == (B, T, m) and w0.shape == (B, T, m) and np.all(o0 == 0.0) and np.all(w0 == 0.0)
        rng = np.random.default_rng(5)
        og, wg = rng.normal(size=(B, T, m)), rng.uniform(0, 1, size=(B, T, m))
        wg[:, :, :6] = 0.0
        ctx.set_control_grav_cost(offset=og, weight=wg)
        for bad in (-1e-3, np.nan, np.inf):
            wb = np.zeros((T, m)); wb[:, 6:] = 1.0; wb[1, 8] = bad
            assert code(lambda: ctx.set_control_grav_cost(weight=wb)) == capi.E_ARG, bad
            assert code(lambda: ctx.set_control_grav_cost(offset=np.zeros((T, m)), weight=wb)) == capi.E_ARG, bad
        for bad in (np.nan, -np.inf):
            ob_ = np.ones((T, m)); ob_[2, 3] = bad
            assert code(lambda: ctx.set_control_grav_cost(offset=ob_)) == capi.E_ARG, bad
        for row in (0, 5):                                              # a weight on one of the free-flyer root's six rows
            wr = np.zeros((T, m)); wr[T - 1, row] = 1e-3
            assert code(lambda: ctx.set_control_grav_cost(weight=wr)) == capi.E_ARG, row
        assert code(lambda: ctx.set_control_grav_cost(weight=1.0)) == capi.E_ARG     # (the scalar reaches the root rows too)
        assert code(lambda: ctx.set_control_grav_cost(weight=0.0, first=B, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_control_grav_cost(weight=0.0, first=-1, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_control_grav_cost(weight=0.0, first=1, count=B)) == capi.E_ARG
        assert code(lambda: ctx.control_grav_cost(first=1, count=B)) == capi.E_ARG
        z = np.zeros((B + 1) * T * m)
        assert L.ddp_hip_control_grav_cost_upload(ctx._h, z.ctypes.data_as(dp), z.ctypes.data_as(dp), 0, B + 1) == capi.E_ARG
        o1, w1 = ctx.control_grav_cost()
        assert np.array_equal(o1, og) and np.array_equal(w1, wg)        # a refused upload leaves both sides as they were
        ctx.set_control_grav_cost(offset=og[1] + 1.0, first=1, count=1) # one side, one instance; the weights stay
        o1, w1 = ctx.control_grav_cost()
        assert np.array_equal(o1[0], og[0]) and np.array_equal(o1[1], og[1] + 1.0) and np.array_equal(o1[2], og[2]) and np.array_equal(w1, wg)
        ctx.set_control_grav_cost(weight=wg[2] * 2.0, first=2, count=1) # ... and the other side alone; the offsets stay
        o2, w2 = ctx.control_grav_cost(first=1, count=2)                # the round trip of a range of instances
        assert np.array_equal(o2, o1[1:]) and np.array_equal(w2[0], wg[1]) and np.array_equal(w2[1], wg[2] * 2.0)
        row = np.concatenate([np.zeros(6), np.arange(1.0, m - 5)])
        ctx.set_control_grav_cost(offset=0.25, weight=row, first=1, count=2)   # broadcast: scalar and (m,)
        assert np.array_equal(ctx.control_grav_cost()[1][1:], np.broadcast_to(row, (2, T, m)))
        assert np.all(ctx.control_grav_cost()[0][1:] == 0.25) and np.array_equal(ctx.control_grav_cost()[1][0], wg[0])
    model6, spec6, _ = make("chain6", T, batch=B, fd_mode=0)
    with capi.Context(spec6, flags=capi.FLAG_CONTROL_GRAV_COST) as ctx: # a fixed base: every row takes a weight
        ctx.set_control_grav_cost(weight=1.0)
        assert np.all(ctx.control_grav_cost()[1] == 1.0)


@pytest.mark.gpu
def test_holding_torque_is_free(gpu):
    """chain6 under gravity, posture tracking of the start plus this term, started from U = g(q0) (ModelHandle.gravity_torque)
    at rest: the first linearisation has r = 0 at t = 0 and LU there is the flag-off LU bit for bit; after a few iterations
    max |u - g(q)| along the result is below that of the same problem solved with the flag off and the same total control weight
    (there as a tracking weight about uref = 0: |u|^2 itself); the cost over accepted steps never increases"""
    capi = gpu
    T, iters, mu, wu = 20, 6, 1.0, 5.0
    model, spec, o = make("chain6", T, fd_mode=0)
    rng = np.random.default_rng(3)
    q0 = 0.5 * rng.normal(size=o.nq)
    with capi.ModelHandle(model) as hd:
        g0 = hd.gravity_torque(q0)
    x0 = np.concatenate([q0, np.zeros(o.nv)])
    us = np.tile(g0, T)[None, :]
    xs = o.rollout(x0, us[0])[None, :]
    X0 = xs[0].reshape(T + 1, o.nx)
    assert np.max(np.abs(X0 - x0)) < 1e-9                # the holding torque holds
    ref = {"xref": np.tile(x0, T + 1).reshape(1, T + 1, o.nx), "wx": np.full((1, T + 1, o.n), 10.0),
           "uref": np.zeros((1, T, o.m)), "wu": np.zeros((1, T, o.m))}

    def dev(X, U):
        X, U = X.reshape(T + 1, o.nx), U.reshape(T, o.m)
        return max(np.max(np.abs(U[t] - grav_torque(o, model, X[t][:o.nq], jacobian=False)[0])) for t in range(T))
    res, lu0 = {}, {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_NO_TENSORS | (FLAG(capi) if on else 0)) as ctx:
            _setup(ctx, xs, us)
            r_ = dict(ref)
            if on:
                ctx.set_control_grav_cost(weight=wu)
            else:
                r_["wu"] = np.full((1, T, o.m), wu)
            tc.upload_ref(ctx, ref)                      # (the control weights still 0: the flag-off LU that the term adds onto)
            ctx.linearize()
            lu0[on] = ctx.download("LU")[0][:o.m].copy()
            tc.upload_ref(ctx, r_)
            costs = []
            for it in range(iters):
                ctx.linearize()
                _, _, mu_o, _ = ctx.backward(0.0, mu)
                ctx.forward(mu_o, n_alpha=8)
                costs.append(ctx.download("COSTS_OLD")[0].sum())
                ctx.swap_traj()
            res[on] = (dev(ctx.download("X")[0], ctx.download("U")[0]), costs)
    assert np.array_equal(lu0[True], lu0[False]) and np.max(np.abs(lu0[True])) > 0   # r = 0 at t = 0: nothing is added to LU there
    print("holding torque: max|u - g| flag on", res[True][0], "flag off", res[False][0], "costs", res[True][1])
    for a, b in zip(res[True][1], res[True][1][1:]):
        assert b <= a * (1 + 1e-12), res[True][1]
    assert res[True][0] < res[False][0], (res[True][0], res[False][0])
