"""Per-instance centroidal-momentum costs (DDP_HIP_FLAG_MOMENTUM_COST, include/ddp_hip/ddp_hip.h):

    h = (l, k),  l = sum_j m_j pdot_j,  k = sum_j [ m_j (p_j - c) x pdot_j + I_j omega_j ],   r = h(q_t, v_t) - g[b][t]
    l(t, x, u) += 1/2 sum_a w[b][t][a] r_a^2,   lf(x_T) alike with w[b][T]

The oracle has no such cost, so the yardstick is the numpy restatement below in the per-body form: for body j the frame-velocity
jacobians P_j, W_j, D_j, E_j of its CoM point (test_frame_vel_cost.vel_jacobians), R_j (test_frame_orient_cost.frame_R), c and Jc
(test_com_cost.com, com_jac) and m_j, com_j, Ic_j from the model.  The device forms the same jacobians by subtree with spatial
quantities about the world origin (momentum_cost.h): another route to the same numbers.  test_yardstick_gradient holds the
yardstick against central differences, against M Jc v and, on the free-flyer models, against the oracle's joint-space inertia
matrix.  The helpers of the other cost terms' tests are reused by import; tolerances are theirs."""
import os
import re

import numpy as np
import pytest

import test_com_cost as cm
import test_frame_cost as fc
import test_frame_orient_cost as fo
import test_frame_vel_cost as fv
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


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def momentum_jacobians(o, model, q, v, jacobian=True):
    """(h6, Jq, Jv) in the per-body form (ddp_hip.h; Jq = Jv = None without `jacobian`)"""
    m = np.asarray(model.mass_j)
    M = m.sum()
    c = cm.com(o, model, q)
    h = np.zeros(6)
    Jq, Jv = np.zeros((6, o.nv)), np.zeros((6, o.nv))
    Jc = cm.com_jac(o, model, q) if jacobian else None
    for j in range(len(m)):
        p = o.frame_position(j, model.com[j], q)
        R = fo.frame_R(o, j, q)
        I = R @ np.asarray(model.Ic[j]) @ R.T
        if jacobian:
            vel, DE, PW = fv.vel_jacobians(o, model, j, model.com[j], q, v)
        else:
            vel = fv.frame_velocity(o, j, model.com[j], q, v)
        pd, om = vel[:3], vel[3:]
        h[:3] += m[j] * pd
        h[3:] += m[j] * np.cross(p - c, pd) + I @ om
        if not jacobian:
            continue
        D, E, P, W = DE[:3], DE[3:], PW[:3], PW[3:]
        Jv[:3] += m[j] * P
        Jv[3:] += m[j] * np.cross(p - c, P, axis=0) + I @ W
        Jq[:3] += m[j] * D
        Jq[3:] += (m[j] * np.cross(P - Jc, pd[:, None], axis=0) + m[j] * np.cross(p - c, D, axis=0)
                   + np.cross(W, (I @ om)[:, None], axis=0) - I @ np.cross(W, om[:, None], axis=0) + I @ E)
    return (h, Jq, Jv) if jacobian else (h, None, None)


def momentum(o, model, q, v):
    return momentum_jacobians(o, model, q, v, jacobian=False)[0]


def mom_terms(o, model, xs, tgt, w):
    """the momentum terms of one instance per t (T+1 values; the last belongs to lf); tgt, w: (T+1, 6).  A block whose weights
    are all 0 forms nothing"""
    X = xs.reshape(o.T + 1, o.nx)
    out = np.zeros(o.T + 1)
    for t in range(o.T + 1):
        if not np.any(w[t] != 0.0):
            continue
        r = momentum(o, model, X[t][:o.nq], X[t][o.nq:]) - tgt[t]
        out[t] = 0.5 * np.sum(w[t] * r * r)
    return out


def mom_grad_hess(o, model, x, tgt_t, w_t, drop_q=False):
    """(lx, lxx) contributions at one state, n and n x n: A^T (w o r) and the Gauss-Newton A^T diag(w) A, A = [Jq | Jv].
    drop_q: without Jq (what an implementation that forgot it would form)"""
    n = o.n
    g, Hm = np.zeros(n), np.zeros((n, n))
    if not np.any(w_t != 0.0):
        return g, Hm
    h, Jq, Jv = momentum_jacobians(o, model, x[:o.nq], x[o.nq:])
    A = np.hstack([np.zeros_like(Jq) if drop_q else Jq, Jv])
    g += A.T @ (w_t * (h - tgt_t))
    for a in range(6):                                   # entry (i, j) and (j, i) alike: symmetric bit for bit
        Hm += w_t[a] * np.outer(A[a], A[a])
    return g, Hm


def mom_derivs(o, model, xs, tgt, w, drop_q=False):
    """what the terms add to LX, LXX, LFX, LFXX of one instance, in the library's flat (column-major) layout"""
    X = xs.reshape(o.T + 1, o.nx)
    out = {"LX": [], "LXX": []}
    for t in range(o.T + 1):
        g, Hm = mom_grad_hess(o, model, X[t], tgt[t], w[t], drop_q)
        if t == o.T:
            out["LFX"], out["LFXX"] = g, Hm.ravel(order="F")
        else:
            out["LX"].append(g); out["LXX"].append(Hm.ravel(order="F"))
    out["LX"], out["LXX"] = np.concatenate(out["LX"]), np.concatenate(out["LXX"])
    return out


def random_task(o, model, xs, B, seed, wscale=1.0, spread=0.2):
    """per-instance targets near the momentum along the trajectories (xs: (B, ...)) and positive weights, each (B, T+1, 6)"""
    rng = np.random.default_rng(seed)
    T = o.T
    tgt = np.zeros((B, T + 1, 6))
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            tgt[b, t] = momentum(o, model, X[t][:o.nq], X[t][o.nq:]) + spread * rng.normal(size=6)
    return tgt, wscale * rng.uniform(0.1, 2.0, size=(B, T + 1, 6))


def _state(o, rng):
    q, v = rng.normal(size=o.nq), rng.normal(size=o.nv)
    if o.nq != o.nv:
        q[3:7] /= np.linalg.norm(q[3:7])
    return q, v


# ---- CPU: the yardstick checks itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_yardstick_gradient(name):
    """lx against the 5-point central difference of the numpy cost along x (+) (+-h e_j) over all 2 nv tangent directions; with
    the target at h (r = 0, where Gauss-Newton is exact) lxx against the central difference of the gradient; lxx symmetric bit
    for bit; the gradient and the q-v block non-zero; l = M Jc v; on the free-flyer models R_0 (M(q) v)[0:3] = l and
    R_0 (M(q) v)[3:6] = k + (c - o_0) x l with M(q) the oracle's joint-space inertia matrix.  A check of the numpy restatement
    alone: it calls nothing of the library's new code, so unlike every other test of this file it also passes without the feature"""
    T = 2
    model, _, o = make_any(name, T, fd_mode=0)
    xs, us = _trajs(o, model, 1, 3)
    xs = _moving(xs, o, 5)
    tgt, w = random_task(o, model, xs, 1, 4)
    X = xs[0].reshape(T + 1, o.nx)
    nv, n = o.nv, o.n
    M = float(np.sum(model.mass_j))
    w5 = ((-2, 1.0 / 12), (-1, -8.0 / 12), (1, 8.0 / 12), (2, -1.0 / 12))
    small = n <= 26                                      # the 38-joint models: one t, and every sixth column of lxx
    for t in ((1, T) if small else (T,)):
        q, v = X[t][:o.nq], X[t][o.nq:]
        h = momentum(o, model, q, v)
        assert np.max(np.abs(h[:3] - M * cm.com_jac(o, model, q) @ v)) <= 1e-12 * max(1.0, np.max(np.abs(h)))
        if o.nq != o.nv:
            R0, c = fo.frame_R(o, 0, q), cm.com(o, model, q)
            Mv = o.crba(q) @ v
            assert np.max(np.abs(R0 @ Mv[:3] - h[:3])) <= 1e-10 * max(1.0, np.max(np.abs(h)))
            assert np.max(np.abs(R0 @ Mv[3:6] - (h[3:] + np.cross(c - q[:3], h[:3])))) <= 1e-10 * max(1.0, np.max(np.abs(h)))
        g, Hm = mom_grad_hess(o, model, X[t], tgt[0][t], w[0][t])
        assert np.max(np.abs(g[:nv])) > 0 and np.max(np.abs(g[nv:])) > 0
        # (chain6's axes are parallel: of a planar chain the rows of dh/dq and of dh/dv that carry something are disjoint)
        assert np.max(np.abs(Hm[:nv, :nv])) > 0 and np.max(np.abs(Hm[nv:, nv:])) > 0 and (np.max(np.abs(Hm[:nv, nv:])) > 0 or name == "chain6")
        assert np.array_equal(Hm, Hm.T)

        def cost_at(dx):
            X2 = X.copy()
            X2[t] = tc._integrate_x(o, X[t], dx)
            return mom_terms(o, model, X2.ravel(), tgt[0], w[0])[t]
        fd = np.zeros(n)
        for j in range(n):
            e = np.zeros(n); e[j] = H
            fd[j] = sum(cw * cost_at(s * e) for s, cw in w5) / H
        assert np.max(np.abs(fd - g)) <= 1e-8 * max(1.0, np.max(np.abs(g))), np.max(np.abs(fd - g))
        g_noq = mom_grad_hess(o, model, X[t], tgt[0][t], w[0][t], drop_q=True)[0]
        assert np.max(np.abs(fd - g_noq)) > 1e-4 * np.max(np.abs(g))         # dh/dq matters at these inputs
        if t != T:
            continue
        _, H0 = mom_grad_hess(o, model, X[t], h, w[0][t])

        def grad_at(dx):
            return mom_grad_hess(o, model, tc._integrate_x(o, X[t], dx), h, w[0][t])[0]
        cols = list(range(0, n, 1 if small else 6))
        fdh = np.zeros((n, len(cols)))
        for k, j in enumerate(cols):
            e = np.zeros(n); e[j] = H
            fdh[:, k] = sum(cw * grad_at(s * e) for s, cw in w5) / H
        assert np.max(np.abs(fdh - H0[:, cols])) <= 1e-8 * max(1.0, np.max(np.abs(H0))), np.max(np.abs(fdh - H0[:, cols]))
        assert np.array_equal(H0, H0.T)


def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.FLAG_MOMENTUM_COST == 2048 and re.search(r"#define\s+DDP_HIP_FLAG_MOMENTUM_COST\s+2048u", header)
    L = capi.lib()
    for name in ("ddp_hip_momentum_cost_upload", "ddp_hip_momentum_cost_download", "ddp_hip_model_centroidal_momentum"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    assert len(capi.SEQ_NAMES) == 40
    assert hasattr(capi.Context, "set_momentum_cost") and hasattr(capi.Context, "momentum_cost")
    assert hasattr(capi.ModelHandle, "centroidal_momentum")
    # shapes are checked before anything reaches the library: a context object without a device will do
    T, B = 5, 2
    model, spec, _ = make("chain6", T, batch=B, fd_mode=0)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx._h = spec, B, None
    for kw in (dict(target=np.zeros((T, 6))), dict(target=np.zeros(6)), dict(target=0.0), dict(target=np.zeros((B + 1, T + 1, 6))),
               dict(weight=np.zeros((T + 1, 3))), dict(weight=np.zeros(3)), dict(weight=np.zeros((B, T + 1, 6)), count=1),
               dict(target=np.zeros((T + 1, 6)), weight=np.zeros((T, 6)))):
        with pytest.raises(ValueError):
            ctx.set_momentum_cost(**kw)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_model_centroidal_momentum(gpu, name):
    """ddp_hip_model_centroidal_momentum: the traversal on the device in isolation, h6, Jq and Jv against the yardstick to 1e-12"""
    capi = gpu
    model, _, o = make_any(name, 2, fd_mode=0)
    rng = np.random.default_rng(5)
    with capi.ModelHandle(model) as hd:
        for k in range(3):
            q, v = _state(o, rng)
            h, Jq, Jv = hd.centroidal_momentum(q, v, jacobian=True)
            h_only = hd.centroidal_momentum(q, v)
            eh, eq, ej = (rel_err(a, b) for a, b in zip((h, Jq, Jv), momentum_jacobians(o, model, q, v)))
            print("model_centroidal_momentum", name, k, eh, eq, ej)
            assert np.array_equal(h, h_only)
            assert np.max(np.abs(Jv)) > 0 and np.max(np.abs(Jq)) > 0
            assert eh <= 1e-12 and eq <= 1e-12 and ej <= 1e-12, (eh, eq, ej)


LIN_CASES = fv.LIN_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_,flags", LIN_CASES)
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, name, fd_mode, fo_, flags, stages):
    """LX, LXX, LFX, LFXX against the flag-off values plus the definition's terms, batch 3 with different targets and weights
    per instance, through ddp_hip_linearize and ddp_hip_linearize_stages(LIN_COST); LXX / LFXX symmetric bit for bit; LU, LUU
    and LUX bit for bit the flag-off values; an (instance, t) whose six weights are 0 keeps the flag-off bits; the device is not
    the yardstick without its delta-q half.  "all": tracking, frame positions, orientations and velocities, state limits and the
    CoM cost live beside it.  Here the zero weights are one (instance, t), b = 1, t = 4; a whole instance with zero weights
    inside a live batch is test_zero_weights_change_nothing[zero_instance].  Measured on an MI355X: 2.1e-13 at worst (tree38, "all"; entries of LXX reach 1e4), 1.2e-14 on chain6"""
    capi = gpu
    T, B = 6, 3
    model, spec, o = make_any(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    frames = fc.pick_frames(model, 3)
    xs, us = _trajs(o, model, B, 41)
    xs = _moving(xs, o, 40)
    tgt, w = random_task(o, model, xs, B, 42)
    w[1, 2, 1] = 0.0; w[0, T, 5] = 0.0; w[0, 1, 3] = 0.0  # single zero weights among the others
    w[2, :, 3:] = 0.0                                   # one instance with only linear weights, at every t
    w[0, 3, :3] = 0.0                                   # one (instance, t) with only angular weights
    w[1, 4, :] = 0.0                                    # one (instance, t) with all weights off
    base = capi.FLAG_NO_TENSORS if flags == "nt" else 0
    if flags == "all":
        base |= (capi.FLAG_TRACKING_COST | capi.FLAG_FRAME_COST | capi.FLAG_FRAME_ORIENT_COST | capi.FLAG_FRAME_VEL_COST
                 | capi.FLAG_STATE_LIMITS | capi.FLAG_COM_COST)
        ref = tc.random_ref(o, model, xs, us, B, 44)
        ftask = fc.random_task(o, xs, frames, B, 45)
        otask = fo.random_orient(o, xs, frames, B, 47)
        lim = sl.random_limits(o, xs, B, 46)
        ctask = cm.random_task(o, model, xs, B, 48)
        vtask = fv.random_task(o, xs, frames, B, 49)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (capi.FLAG_MOMENTUM_COST if on else 0)) as ctx:
            _setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
            if flags == "all":
                tc.upload_ref(ctx, ref)
                ctx.set_frame_cost(frames=frames, target=ftask[0], weight=ftask[1])
                ctx.set_frame_orient_cost(quat=otask[0], weight=otask[1])
                ctx.set_state_limits(lo=lim[0], hi=lim[1], weight=lim[2])
                ctx.set_com_cost(target=ctask[0], weight=ctask[1])
                ctx.set_frame_vel_cost(target=vtask[0], weight=vtask[1])
            if on:
                ctx.set_momentum_cost(target=tgt, weight=w)
            ctx.linearize(None if stages is None else capi.LIN_COST)
            got[on] = {s: ctx.download(s) for s in DERIVS}
    n, nv = o.n, o.nv
    worst = 0.0
    for b in range(B):
        add = mom_derivs(o, model, xs[b], tgt[b], w[b])
        for s in ("LX", "LXX", "LFX", "LFXX"):
            ex = got[False][s][b] + add[s]
            assert np.max(np.abs(add[s])) > 0
            worst = max(worst, rel_err(got[True][s][b], ex))
            assert rel_err(got[True][s][b], ex) <= 1e-12, (s, b, rel_err(got[True][s][b], ex))
        assert np.max(np.abs(add["LXX"].reshape(T, n, n)[:, nv:, :nv])) > 0 or name == "chain6"   # the q-v coupling is there (planar chain: none)
        if b == 0:                                      # negative control: the delta-q half is in the device's values
            noq = mom_derivs(o, model, xs[b], tgt[b], w[b], drop_q=True)
            assert rel_err(got[True]["LX"][b], got[False]["LX"][b] + noq["LX"]) > 1e-6
            assert rel_err(got[True]["LXX"][b], got[False]["LXX"][b] + noq["LXX"]) > 1e-6
        for s in ("LU", "LUU", "LUX"):
            assert np.array_equal(got[True][s][b], got[False][s][b]), s
        for t in range(T + 1):
            key, k = ("LXX", t) if t < T else ("LFXX", 0)
            blk = got[True][key][b][k * n * n:(k + 1) * n * n].reshape(n, n)
            off = got[False][key][b][k * n * n:(k + 1) * n * n].reshape(n, n)
            assert np.array_equal(blk, blk.T)
            gk, go = ("LX", t) if t < T else ("LFX", 0)
            gon, goff = got[True][gk][b][go * n:(go + 1) * n], got[False][gk][b][go * n:(go + 1) * n]
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
    T, B, mu = 6, 2, 30.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 51)
    xs2, us2 = _trajs(o, model, B, 61)
    xs, xs2 = _moving(xs, o, 54), _moving(xs2, o, 64)
    tgt, w = random_task(o, model, xs, B, 52)
    w[1, 3, :] = 0.0
    w[0, :, 3:] = 0.0
    w[1, 2, :3] = 0.0
    mults = tc._mults(o, xs[0], 53)
    with capi.Context(spec, flags=capi.FLAG_MOMENTUM_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
        ctx.set_momentum_cost(target=tgt, weight=w)
        ctx.cost_seq_aug(0, mu)
        ctx.cost_seq_aug(1, mu)
        got = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
    for which, (X, U) in ((0, (xs, us)), (1, (xs2, us2))):
        for b in range(B):
            add = mom_terms(o, model, X[b], tgt[b], w[b])
            ex = o.cost_seq_aug(X[b], U[b], mults, mu) + add
            assert got[which][b][T] != 0.0 and add[T] != 0.0
            assert rel_err(got[which][b], ex) <= 1e-12, (which, b, rel_err(got[which][b], ex))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tree38", "chain6ff", "table7"])
def test_angular_weights_off(gpu, name):
    """weights (w, w, w, 0, 0, 0): the terms are 1/2 w |M Jc v - g|^2, a CoM-velocity cost scaled by M^2"""
    capi = gpu
    T, B, mu = 4, 3, 1.0
    model, spec, o = make_any(name, T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 121)
    xs = _moving(xs, o, 122)
    tgt, w = random_task(o, model, xs, B, 123)
    w[:, :, 3:] = 0.0
    M = float(np.sum(model.mass_j))
    with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        ctx.cost_seq_aug(0, mu)
        off = ctx.download("COSTS_OLD")
    with capi.Context(spec, flags=capi.FLAG_MOMENTUM_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        ctx.set_momentum_cost(target=tgt, weight=w)
        ctx.cost_seq_aug(0, mu)
        got = ctx.download("COSTS_OLD")
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        add = np.array([0.5 * np.sum(w[b, t, :3] * (M * cm.com_jac(o, model, X[t][:o.nq]) @ X[t][o.nq:] - tgt[b, t, :3]) ** 2)
                        for t in range(T + 1)])
        assert np.all(add > 0)
        assert rel_err(got[b], off[b] + add) <= 1e-12, (b, rel_err(got[b], off[b] + add))


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,mu", [("tree38", 60, 1.0), ("chain6", 30, 10.0)])
def test_sweep_parity_nonzero_value(gpu, name, T, mu):
    """the backward sweep with the momentum cost in LXX (all four blocks): Oracle.backward on the flag-off device derivatives plus
    the yardstick's terms against the device sweep with the flag on: restarts, mu and reg identical, every step redone alone by
    the oracle from the device's V(t+1) lands on the device's k_t, K_t, V_x(t), V_xx(t) to 1e-10 (stepwise_backward_check)"""
    from oracle.binding import Oracle
    capi = gpu
    model, spec, o = make(name, T, fd_mode=2)
    xs, us = _trajs(o, model, 1, 71, held=True)
    xs = _moving(xs, o, 74, sigma=0.1)
    tgt, w = random_task(o, model, xs, 1, 72, wscale=0.01, spread=0.05)
    mults = tc._mults(o, xs[0], 73)
    n, m = o.n, o.m
    d = o.alloc_derivs()
    with capi.Context(spec, flags=capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.linearize()
        for k, s in NAMES.items():
            if ctx.seq_size(s):
                d[k][:ctx.seq_size(s)] = ctx.download(s)[0]
    add = mom_derivs(o, model, xs[0], tgt[0], w[0])
    for k, s in (("lx", "LX"), ("lxx", "LXX"), ("lfx", "LFX"), ("lfxx", "LFXX")):
        d[k][:add[s].size] += add[s]
    assert np.max(np.abs(add["LXX"].reshape(T, n, n)[:, o.nv:, :o.nv])) > 0 or name == "chain6"
    with capi.Context(spec, flags=capi.FLAG_MOMENTUM_COST | capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.set_momentum_cost(target=tgt, weight=w)
        ctx.linearize()
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
@pytest.mark.parametrize("name,T,fd_mode,fo_,fwd_path", [
    ("tree38", 24, 2, None, 1),                     # latency forward
    ("chain6ff", 10, 2, 0, 0),                      # lane-per-rollout forward
    ("tree38_frame", 24, 0, None, 1),               # constrained: the candidates' costs from cand_cost_kernel
])
@pytest.mark.parametrize("mode", ["nothing", "zero_weights", "zero_instance"])
def test_zero_weights_change_nothing(gpu, name, T, fd_mode, fo_, fwd_path, mode):
    """flag on with nothing uploaded, or targets far away but every weight 0: bit for bit what the flag-off context computes.
    zero_instance: batch 2, instance 1 carries non-zero weights (the kernels run), instance 0 none: instance 0 is bit for bit
    the flag-off context's instance 0"""
    capi = gpu
    mu = 10.0
    B = 2 if mode == "zero_instance" else 1
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 31, held=True)
    xs = _moving(xs, o, 34, sigma=0.1)
    mults = tc._mults(o, xs[0], 32)
    tgt, w = random_task(o, model, xs, B, 33, spread=1.0)
    if mode == "zero_instance":
        w[0] = 0.0
        w *= 0.05
    else:
        w[:] = 0.0
    out = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_TRACE | (capi.FLAG_MOMENTUM_COST if on else 0)) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            _setup(ctx, xs, us, mults, o.Etot)
            if on and mode != "nothing":
                ctx.set_momentum_cost(target=tgt, weight=w)
            out[on] = fc._run_all(ctx, mu, name == "tree38")
    a, b = out[False], out[True]
    if mode == "zero_instance":
        assert not np.array_equal(a["LX"][1], b["LX"][1])            # the terms are there for instance 1
        assert not np.array_equal(a["COSTS_OLD"][1], b["COSTS_OLD"][1])
        a = {k: (tuple(np.asarray(v)[..., :1] for v in a[k][1:]) if isinstance(a[k], tuple) else (a[k][:1] if k != "stream" else a[k])) for k in a}
        b = {k: (tuple(np.asarray(v)[..., :1] for v in b[k][1:]) if isinstance(b[k], tuple) else (b[k][:1] if k != "stream" else b[k])) for k in b}
    fc._same(a, b)
    assert np.all(np.isfinite(b["LX"])) and np.all(np.isfinite(b["X_NEW"]))


# (name, first_order_fd, forward path, n_alpha, k_scale, with the CoM and frame-velocity costs)
FORWARD_CASES = [("tree38", None, 1, 1, 1.0, False), ("tree38", None, 1, 8, 3.0, False), ("chain6ff", 0, 0, 1, 3.0, False),
                 ("chain6ff", 0, 0, 8, 1.0, False), ("tree38", None, 1, 8, 3.0, True)]
# A_G's entries are subtree masses times lever arms (some 50 on tree38), so a weight of 0.05 gives the curvature a frame-velocity
# weight of some 100 gives (test_frame_vel_cost.FWD_WSCALE: stiffer velocity gains let the overshot full step diverge); targets 20
# away keep the terms material beside the other cost terms.  FWD_XMAX is asserted on the emulation
FWD_WSCALE, FWD_SPREAD, FWD_XMAX = 0.05, 20.0, 1e4


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_,fwd_path,n_alpha,k_scale,with_others", FORWARD_CASES)
def test_forward_matches_emulation(gpu, name, fo_, fwd_path, n_alpha, k_scale, with_others):
    """accepted step, X_NEW, U_NEW and dcost against Oracle.forward_alpha rollouts costed with numpy, the momentum terms included;
    k_scale 3 overshoots so that the halving runs; with_others: the CoM and frame-velocity costs live as well (the order of
    additions: CoM, frame velocities, momentum).  The device adds the terms' sum in another association than the emulation: the
    test first asserts, on the emulation alone, that every candidate tried decides by more than 1e-9 of the sum of the cost terms'
    magnitudes, and only then compares decisions"""
    capi = gpu
    mu = 1.0
    T = 16
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo_)
    frames = fc.pick_frames(model, 3)
    xs, us = _trajs(o, model, 1, 81, held=True)
    xs = _moving(xs, o, 84, sigma=0.1)
    tgt, w = random_task(o, model, xs, 1, 82, wscale=FWD_WSCALE, spread=FWD_SPREAD)
    ctask = cm.random_task(o, model, xs, 1, 86, wscale=2000.0, spread=0.02)
    vtask = fv.random_task(o, xs, frames, 1, 87, wscale=fv.FWD_WSCALE, spread=fv.FWD_SPREAD)
    mults = tc._mults(o, xs[0], 85)
    flags = capi.FLAG_MOMENTUM_COST | capi.FLAG_NO_TENSORS
    if with_others:
        flags |= capi.FLAG_COM_COST | capi.FLAG_FRAME_COST | capi.FLAG_FRAME_VEL_COST
    with capi.Context(spec, flags=flags) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.set_momentum_cost(target=tgt, weight=w)
        if with_others:
            ctx.set_com_cost(target=ctask[0], weight=ctask[1])
            ctx.set_frame_cost(frames=frames)
            ctx.set_frame_vel_cost(target=vtask[0], weight=vtask[1])
        ctx.linearize()
        _, _, mu_o, _ = ctx.backward(0.0, mu)
        if k_scale != 1.0:
            ctx.upload("FB_VAL", k_scale * ctx.download("FB_VAL"))
        fb = {"origin": ctx.download("FB_ORIGIN")[0], "val": ctx.download("FB_VAL")[0], "jac": ctx.download("FB_JAC")[0]}
        rc, step, dcost = ctx.forward(mu_o, n_alpha=n_alpha)
        xn, un = ctx.download("X_NEW")[0], ctx.download("U_NEW")[0]

    def cost(X, U):
        c = o.cost_seq_aug(X, U, mults, mu_o[0]) + mom_terms(o, model, X, tgt[0], w[0])
        if with_others:
            c = c + cm.com_terms(o, model, X, ctask[0][0], ctask[1][0]) + fv.vel_terms(o, X, frames, vtask[0][0], vtask[1][0])
        return c
    em = cm._emulate_forward(o, xs[0], us[0], mults, fb, mu_o[0], n_alpha, cost)
    assert em is not None
    step_ref, xn_ref, un_ref, new, margins = em
    share = mom_terms(o, model, xn_ref, tgt[0], w[0]).sum() / np.sum(np.abs(cost(xn_ref, un_ref)))
    print("forward", name, n_alpha, k_scale, with_others, "step", step[0], step_ref, "dcost", dcost[0], new, "margins", margins, "share", share)
    assert share > 1e-6                               # the momentum terms are material in the candidate's cost
    assert min(margins) > 1e-9, margins               # a condition on the inputs: the decisions do not hang on rounding
    assert np.max(np.abs(xn_ref)) < FWD_XMAX          # ... and the rollout compared has not diverged
    assert step[0] == step_ref, (step, step_ref)
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
    xs = _moving(xs, o, 93, sigma=0.1)
    tgt, w = random_task(o, model, xs, B, 92, wscale=0.05, spread=0.5)
    out = []
    for sp, s_ in ((spec, slice(0, B)), (spec1, slice(1, 2))):
        with capi.Context(sp, flags=capi.FLAG_MOMENTUM_COST | capi.FLAG_TRACE | flags) as ctx:
            _setup(ctx, xs[s_], us[s_])
            ctx.set_momentum_cost(target=tgt[s_], weight=w[s_])
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
    xs, us = _trajs(o, model, B, 101, held=True)
    xs = _moving(xs, o, 104, sigma=0.1)
    tgt, w = random_task(o, model, xs, B, 102, wscale=0.05)
    mults = tc._mults(o, xs[0], 103)

    def run(stepwise):
        with capi.Context(spec, flags=capi.FLAG_MOMENTUM_COST | flags) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if o.Etot:
                ctx.upload("MULT_ORIGIN", xs[:, :T * o.nx])
            ctx.set_momentum_cost(target=tgt, weight=w)
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
    L = capi.lib()
    dp = C.POINTER(C.c_double)

    def code(fn):
        with pytest.raises(capi.DdpHipError) as exc:
            fn()
        return exc.value.code
    with capi.Context(spec) as ctx:                                   # a context without the flag
        assert code(lambda: ctx.set_momentum_cost(weight=1.0)) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.momentum_cost()) == capi.E_UNSUPPORTED
    pend = capi.BuiltinModel(capi.BUILTIN_PENDULUM)
    with pytest.raises(capi.DdpHipError) as exc:
        capi.Context(capi.ProblemSpec(pend, T, fd_mode=2), flags=capi.FLAG_MOMENTUM_COST)
    assert exc.value.code == capi.E_UNSUPPORTED
    with capi.Context(spec, flags=capi.FLAG_MOMENTUM_COST) as ctx:      # the flag stands alone
        t0, w0 = ctx.momentum_cost()                                    # create: targets 0, weights 0
        assert t0.shape == (B, T + 1, 6) and np.all(t0 == 0.0) and np.all(w0 == 0.0)
        rng = np.random.default_rng(5)
        tg, wg = rng.normal(size=(B, T + 1, 6)), rng.uniform(0, 1, size=(B, T + 1, 6))
        ctx.set_momentum_cost(target=tg, weight=wg)
        for bad in (-1e-3, np.nan, np.inf):
            wb = np.ones((T + 1, 6)); wb[1, 4] = bad
            assert code(lambda: ctx.set_momentum_cost(weight=wb)) == capi.E_ARG, bad
            assert code(lambda: ctx.set_momentum_cost(target=np.zeros((T + 1, 6)), weight=wb)) == capi.E_ARG, bad
        for bad in (np.nan, -np.inf):
            tb = np.ones((T + 1, 6)); tb[2, 3] = bad
            assert code(lambda: ctx.set_momentum_cost(target=tb, weight=1.0)) == capi.E_ARG, bad
        assert code(lambda: ctx.set_momentum_cost(weight=0.0, first=B, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_momentum_cost(weight=0.0, first=-1, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_momentum_cost(weight=0.0, first=1, count=B)) == capi.E_ARG
        assert code(lambda: ctx.momentum_cost(first=1, count=B)) == capi.E_ARG
        z = np.zeros(B * (T + 1) * 6)
        assert L.ddp_hip_momentum_cost_upload(ctx._h, z.ctypes.data_as(dp), z.ctypes.data_as(dp), 0, B + 1) == capi.E_ARG
        t1, w1 = ctx.momentum_cost()
        assert np.array_equal(t1, tg) and np.array_equal(w1, wg)        # a refused upload leaves both sides as they were
        ctx.set_momentum_cost(target=tg[1] + 1.0, first=1, count=1)     # one side, one instance; the weights stay
        t1, w1 = ctx.momentum_cost()
        assert np.array_equal(t1[0], tg[0]) and np.array_equal(t1[1], tg[1] + 1.0) and np.array_equal(t1[2], tg[2]) and np.array_equal(w1, wg)
        ctx.set_momentum_cost(weight=wg[2] + 1.0, first=2, count=1)     # ... and the other side alone; the targets stay
        t2, w2 = ctx.momentum_cost(first=1, count=2)                    # the round trip of a range of instances
        assert np.array_equal(t2, t1[1:]) and np.array_equal(w2[0], wg[1]) and np.array_equal(w2[1], wg[2] + 1.0)
        six = np.array([1.0, 2.0, 0.0, 0.5, 0.0, 3.0])
        ctx.set_momentum_cost(weight=six, first=1, count=2)             # broadcast: (6,) and scalar
        assert np.array_equal(ctx.momentum_cost()[1][1:], np.broadcast_to(six, (2, T + 1, 6)))
        assert np.array_equal(ctx.momentum_cost()[1][0], wg[0])
        ctx.set_momentum_cost(weight=0.5)
        assert np.all(ctx.momentum_cost()[1] == 0.5) and np.array_equal(ctx.momentum_cost()[0], t1)
    massless = cm.table_model()
    massless = capi.TableModel(massless.parent, massless.jtype, massless.axis, massless.Rp, massless.pp, 0.0 * massless.mass_j,
                               massless.com, massless.Ic)
    with pytest.raises(capi.DdpHipError) as exc:                      # M <= 0
        capi.Context(capi.ProblemSpec(massless, T, fd_mode=2, first_order_fd=1), flags=capi.FLAG_MOMENTUM_COST)
    assert exc.value.code == capi.E_ARG


@pytest.mark.gpu
def test_momentum_task_descends(gpu):
    """tree38, T = 20, a moving initial trajectory; the target is zero momentum with angular weights alone at every t, the terminal
    weight 10 x larger: over a few iterations the total cost never increases over accepted steps, and sum_t |k_t|^2 of the result
    is smaller than that of the initial trajectory"""
    capi = gpu
    T, mu, iters = 20, 1.0, 6
    model, spec, o = make("tree38", T, fd_mode=0)
    xs, us = _trajs(o, model, 1, 111, held=True)
    xs = _moving(xs, o, 112, sigma=0.5)
    tgt = np.zeros((T + 1, 6))
    # the moving start carries |k|^2 of some 2e3 per step (the base joints move the whole 88 kg) beside c/2 |u|^2 of some 4e5 in
    # gravity torques.  The start is no rollout, so the first forward pass meets states off the old trajectory at any step
    # length: with weights of 100 and more (A_G's entries are some 40) the feedback gains are so stiff that no step length
    # descends; a weight of 1 takes sum |k|^2 from 4.3e4 to some 5e3 in six iterations, where the flag-off solve leaves 3.9e4
    w = np.zeros((T + 1, 6))
    w[:, 3:] = 1.0
    w[T, 3:] = 10.0

    def k2(X):
        return sum(np.sum(momentum(o, model, x[:o.nq], x[o.nq:])[3:] ** 2) for x in X.reshape(T + 1, o.nx))
    with capi.Context(spec, flags=capi.FLAG_MOMENTUM_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        ctx.set_momentum_cost(target=tgt, weight=w)
        costs, steps = [], []
        for _ in range(iters):
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            rc, step, dcost = ctx.forward(mu_o, n_alpha=8)
            costs.append(ctx.download("COSTS_OLD")[0].sum())
            steps.append(step[0])
            ctx.swap_traj()
        final = ctx.download("X")[0]
    print("momentum task costs", costs, "steps", steps, "sum |k|^2", k2(xs[0]), "->", k2(final))
    for a, b in zip(costs, costs[1:]):
        assert b <= a * (1 + 1e-12), costs
    assert costs[-1] < costs[0]
    assert k2(final) < k2(xs[0]), (k2(xs[0]), k2(final))
