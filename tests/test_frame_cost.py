"""Per-instance frame-position (task-space) costs (DDP_HIP_FLAG_FRAME_COST, include/ddp_hip/ddp_hip.h):

    l(t, x, u) += 1/2 sum_f sum_a w[b][t][f][a] r_f,a^2,   lf(x_T) += 1/2 sum_f sum_a w[b][T][f][a] r_f,a^2,   r_f = p_f(q_t) - g[b][t][f]

with p_f the world position of the point off_f of joint joint_f.  The oracle has no such cost, so the yardstick is the numpy
restatement below, built on Oracle.frame_position and Oracle.frame_jacobian(world_aligned=True) (the true point jacobian; the
default WORLD-frame rows are not dp/dq), Oracle.integrate, forward_alpha, backward and cost_seq_aug.  Where the tracking flag
is set as well, its terms come from the helpers of test_tracking_cost.py.  Tolerances are those of test_tracking_cost.py."""
import os
import re

import numpy as np
import pytest

import test_tracking_cost as tc
from problems import held_trajectory, initial_trajectory, make
from synth import rel_err, stepwise_backward_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 1e-3
DERIVS = ("LX", "LXX", "LU", "LUU", "LUX", "LFX", "LFXX")
NAMES = {"lfx": "LFX", "lfxx": "LFXX", "lx": "LX", "lu": "LU", "lxx": "LXX", "lux": "LUX", "luu": "LUU", "f_val": "F_VAL",
         "fx": "FX", "fu": "FU", "fxx": "FXX", "fux": "FUX", "fuu": "FUU", "eq_val": "EQ_VAL", "eq_x": "EQ_X", "eq_u": "EQ_U",
         "eq_xx": "EQ_XX", "eq_ux": "EQ_UX", "eq_uu": "EQ_UU"}


# ---- frames ----------------------------------------------------------------------------------------------------------------
def pick_frames(model, F):
    """F = 1: a leaf; 3: a root-side joint, a mid-tree joint, a leaf; 4: + a second leaf (on a chain: the leaf's parent); each
    with a non-zero offset"""
    parent = [int(p) for p in model.parent]
    nj = len(parent)
    depth = [0] * nj
    for j in range(nj):
        depth[j] = depth[parent[j]] + 1 if parent[j] >= 0 else 0
    leaves = [j for j in range(nj) if j not in parent]
    leaf = max(leaves, key=lambda j: (depth[j], j))
    path = [leaf]
    while parent[path[-1]] >= 0:
        path.append(parent[path[-1]])
    mid = path[len(path) // 2]
    others = [j for j in leaves if j != leaf]
    second = max(others, key=lambda j: (depth[j], -j)) if others else parent[leaf]
    offs = [(0.1, -0.05, 0.2), (-0.03, 0.12, 0.07), (0.02, 0.04, 0.15), (0.05, -0.1, -0.08)]
    joints = {1: [leaf], 3: [0, mid, leaf], 4: [0, mid, leaf, second]}[F]
    sel = {1: [2], 3: [0, 1, 2], 4: [0, 1, 2, 3]}[F]
    return [(j, offs[k]) for j, k in zip(joints, sel)]


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def frame_terms(o, xs, frames, tgt, w):
    """the frame terms of one instance per t (T+1 values; the last belongs to lf); tgt, w: (T+1, F, 3)"""
    X = xs.reshape(o.T + 1, o.nx)
    out = np.zeros(o.T + 1)
    for t in range(o.T + 1):
        for f, (j, off) in enumerate(frames):
            r = o.frame_position(j, off, X[t][:o.nq]) - tgt[t][f]
            out[t] += 0.5 * np.sum(w[t][f] * r * r)
    return out


def frame_grad_hess(o, x, frames, tgt_t, w_t):
    """(lx, lxx) contributions at one state, n and n x n: P^T (w o r) and the Gauss-Newton P^T diag(w) P on the q rows"""
    nv, n = o.nv, o.n
    g, Hm = np.zeros(n), np.zeros((n, n))
    for f, (j, off) in enumerate(frames):
        q = x[:o.nq]
        r = o.frame_position(j, off, q) - tgt_t[f]
        P = o.frame_jacobian(j, off, q, world_aligned=True)
        g[:nv] += P.T @ (w_t[f] * r)
        for a in range(3):                               # entry (i, j) and (j, i) alike: symmetric bit for bit
            Hm[:nv, :nv] += w_t[f][a] * np.outer(P[a], P[a])
    return g, Hm


def frame_derivs(o, xs, frames, tgt, w):
    """what the frame terms add to LX, LXX, LFX, LFXX of one instance, in the library's flat (column-major) layout"""
    X = xs.reshape(o.T + 1, o.nx)
    out = {"LX": [], "LXX": []}
    for t in range(o.T + 1):
        g, Hm = frame_grad_hess(o, X[t], frames, tgt[t], w[t])
        if t == o.T:
            out["LFX"], out["LFXX"] = g, Hm.ravel(order="F")
        else:
            out["LX"].append(g); out["LXX"].append(Hm.ravel(order="F"))
    out["LX"], out["LXX"] = np.concatenate(out["LX"]), np.concatenate(out["LXX"])
    return out


def random_task(o, xs, frames, B, seed, wscale=1.0, spread=0.2):
    """per-instance targets near the frames' positions along the trajectories (xs: (B, ...)) and positive weights"""
    rng = np.random.default_rng(seed)
    T, F = o.T, len(frames)
    tgt = np.zeros((B, T + 1, F, 3))
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            for f, (j, off) in enumerate(frames):
                tgt[b, t, f] = o.frame_position(j, off, X[t][:o.nq]) + spread * rng.normal(size=3)
    return tgt, wscale * rng.uniform(0.1, 2.0, size=(B, T + 1, F, 3))


def _trajs(o, model, B, seed, held=False):
    return tc._trajs(o, model, B, seed, held=held)


def _setup(ctx, xs, us, mults=None, Etot=0):
    tc._setup(ctx, xs, us, mults, Etot)


# ---- CPU: the yardstick checks itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain6", "tree38", "chain6ff", "tree38ff"])
@pytest.mark.parametrize("F", [1, 3, 4])
def test_yardstick_gradient(name, F):
    """lx against the 5-point central difference of the numpy cost along x (+) (+-h e_j); with the targets at p_f(q) (r = 0,
    where Gauss-Newton is exact) lxx against the central difference of the gradient; lxx symmetric bit for bit with zero
    velocity rows and columns"""
    T = 2
    model, _, o = make(name, T, fd_mode=0)
    frames = pick_frames(model, F)
    xs, us = _trajs(o, model, 1, 3)
    tgt, w = random_task(o, xs, frames, 1, 4)
    X = xs[0].reshape(T + 1, o.nx)
    nv, n = o.nv, o.n
    w5 = ((-2, 1.0 / 12), (-1, -8.0 / 12), (1, 8.0 / 12), (2, -1.0 / 12))
    for t in (1, T):
        g, Hm = frame_grad_hess(o, X[t], frames, tgt[0][t], w[0][t])
        assert np.max(np.abs(g[:nv])) > 0

        def cost_at(dx):
            X2 = X.copy()
            X2[t] = tc._integrate_x(o, X[t], dx)
            return frame_terms(o, X2.ravel(), frames, tgt[0], w[0])[t]
        fd = np.zeros(n)
        for j in range(n):
            e = np.zeros(n); e[j] = H
            fd[j] = sum(cw * cost_at(s * e) for s, cw in w5) / H
        assert np.max(np.abs(fd - g)) <= 1e-8 * max(1.0, np.max(np.abs(g))), np.max(np.abs(fd - g))
        # r = 0 at X[t]: the gradient's central difference is the Gauss-Newton block
        tgt0 = np.stack([o.frame_position(j, off, X[t][:o.nq]) for j, off in frames])
        _, H0 = frame_grad_hess(o, X[t], frames, tgt0, w[0][t])

        def grad_at(dx):
            return frame_grad_hess(o, tc._integrate_x(o, X[t], dx), frames, tgt0, w[0][t])[0]
        fdh = np.zeros((n, n))
        for j in range(n):
            e = np.zeros(n); e[j] = H
            fdh[:, j] = sum(cw * grad_at(s * e) for s, cw in w5) / H
        # (free-flyer models: the gradient at x (+) dx lives in the tangent at x (+) dx, but it vanishes at dx = 0, so the
        # change of tangent basis does not enter its first derivative)
        assert np.max(np.abs(fdh - H0)) <= 1e-8 * max(1.0, np.max(np.abs(H0))), np.max(np.abs(fdh - H0))
        assert np.array_equal(Hm, Hm.T)
        assert np.all(Hm[nv:, :] == 0.0) and np.all(Hm[:, nv:] == 0.0) and np.all(g[nv:] == 0.0)


def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.FLAG_FRAME_COST == 16 and re.search(r"#define\s+DDP_HIP_FLAG_FRAME_COST\s+16u", header)
    assert capi.MAX_COST_FRAMES == 4 and re.search(r"#define\s+DDP_HIP_MAX_COST_FRAMES\s+4\b", header)
    L = capi.lib()
    for name in ("ddp_hip_frame_cost_set_frames", "ddp_hip_frame_cost_upload", "ddp_hip_frame_cost_download"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert len(capi.SEQ_NAMES) == 40 and capi.SEQ_NAMES[-3:] == ["CTRL_LO", "CTRL_HI", "BOX_STAT"]
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    assert re.search(r"DDP_HIP_SEQ_BOX_STAT,[^\n]*\n\s*DDP_HIP_SEQ_COUNT", header)        # no ddp_hip_seq entries added
    # shapes are checked before anything reaches the library: a context object without a device will do
    T, B = 5, 2
    model, spec, _ = make("chain6", T, batch=B, fd_mode=0)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx.n_cost_frames, ctx._h = spec, B, 3, None
    for kw in (dict(target=np.zeros((T, 3, 3))), dict(target=np.zeros((T + 1, 2, 3))), dict(target=np.zeros((3, 3))),
               dict(target=0.0), dict(weight=np.zeros((T + 1, 3))), dict(weight=np.zeros((B + 1, T + 1, 3, 3))),
               dict(weight=np.zeros((B, T + 1, 3, 3)), count=1), dict(weight=np.zeros(2)),
               dict(frames=[(0, (0, 0, 0))], target=np.zeros((T + 1, 3, 3))), dict(frames=[(0, (0.0, 0.0))])):
        with pytest.raises(ValueError):
            ctx.set_frame_cost(**kw)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _run_all(ctx, mu, with_stream):
    """linearise, both costs, sweep, forward: everything test 4 compares"""
    ctx.linearize()
    r = {s: ctx.download(s) for s in DERIVS}
    if with_stream:
        r["stream"] = ctx.bwd_stream_bytes()
    ctx.cost_seq_aug(0, mu)
    r["COSTS_OLD"] = ctx.download("COSTS_OLD")
    ctx.cost_seq_aug(1, mu)
    r["COSTS_NEW"] = ctx.download("COSTS_NEW")
    rc, reg, mu_out, restarts = ctx.backward(0.0, mu)
    r["bwd"] = (rc, reg, mu_out, restarts)
    for s in ("FB_ORIGIN", "FB_VAL", "FB_JAC", "VX_TRACE"):
        r[s] = ctx.download(s)
    rc, step, dcost = ctx.forward(mu_out, n_alpha=8)
    r["fwd"] = (rc, step, dcost)
    r["X_NEW"], r["U_NEW"] = ctx.download("X_NEW"), ctx.download("U_NEW")
    r["COSTS_OLD_FWD"] = ctx.download("COSTS_OLD")
    return r


def _same(a, b):
    for k in a:
        if isinstance(a[k], tuple):
            for u, v in zip(a[k], b[k]):
                assert np.array_equal(u, v), k
        else:
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,fd_mode,fo,extra,fwd_path", [
    ("tree38", 24, 2, None, "", 1),                 # latency forward
    ("chain6ff", 10, 2, 0, "", 0),                  # lane-per-rollout forward
    ("tree38_frame", 24, 0, None, "", 1),           # constrained: the candidates' costs from cand_cost_kernel
    ("tree38", 24, 2, None, "track", 1),
    ("tree38", 24, 2, None, "box", 1),
])
@pytest.mark.parametrize("mode", ["no_frames", "zero_weights", "zero_instance"])
def test_zero_weights_change_nothing(gpu, name, T, fd_mode, fo, extra, fwd_path, mode):
    """flag on with no frames set, or frames and targets far away but every weight 0: bit for bit what the flag-off context
    computes.  zero_instance: batch 2, instance 1 carries non-zero weights (the frame kernels run), instance 0 none: instance 0
    is bit for bit the flag-off context's instance 0"""
    capi = gpu
    mu = 10.0
    B = 2 if mode == "zero_instance" else 1
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    frames = pick_frames(model, 3)
    xs, us = _trajs(o, model, B, 31, held=True)
    mults = tc._mults(o, xs[0], 32)
    tgt, w = random_task(o, xs, frames, B, 33, spread=1.0)
    if mode == "zero_instance":
        w[0] = 0.0
        w *= 0.05
    else:
        w[:] = 0.0
    base = capi.FLAG_TRACE | (capi.FLAG_TRACKING_COST if extra == "track" else 0) | (capi.FLAG_CONTROL_BOUNDS if extra == "box" else 0)
    ref = tc.random_ref(o, model, xs, us, B, 34, wscale=0.05, spread=0.05)
    out = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (capi.FLAG_FRAME_COST if on else 0)) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            _setup(ctx, xs, us, mults, o.Etot)
            if extra == "track":
                tc.upload_ref(ctx, ref)
            if extra == "box":
                ctx.set_control_bounds(lo=-1e6, hi=1e6)
            if on and mode != "no_frames":
                ctx.set_frame_cost(frames=frames, target=tgt, weight=w)
            out[on] = _run_all(ctx, mu, name == "tree38")
    a, b = out[False], out[True]
    if mode == "zero_instance":
        assert not np.array_equal(a["LX"][1], b["LX"][1])            # the frame terms are there for instance 1
        a = {k: (tuple(np.asarray(v)[..., :1] for v in a[k][1:]) if isinstance(a[k], tuple) else (a[k][:1] if k != "stream" else a[k])) for k in a}
        b = {k: (tuple(np.asarray(v)[..., :1] for v in b[k][1:]) if isinstance(b[k], tuple) else (b[k][:1] if k != "stream" else b[k])) for k in b}
    _same(a, b)
    assert np.all(np.isfinite(b["LX"])) and np.all(np.isfinite(b["X_NEW"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo,flags,F", [
    ("chain6", 2, None, "", 3), ("tree38", 2, None, "", 4), ("chain6ff", 2, 0, "", 4), ("tree38ff", 0, 0, "nt", 3),
    ("tree38", 2, None, "track", 1)])
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, name, fd_mode, fo, flags, F, stages):
    """LX, LXX, LFX, LFXX against the flag-off values plus the definition's terms, batch 3 with different targets and weights
    per instance, through ddp_hip_linearize and ddp_hip_linearize_stages(LIN_COST); LXX symmetric bit for bit; LU, LUU, LUX
    bit for bit the flag-off values"""
    capi = gpu
    T, B = 6, 3
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    frames = pick_frames(model, F)
    xs, us = _trajs(o, model, B, 41)
    tgt, w = random_task(o, xs, frames, B, 42)
    w[1, 2, 0, 1] = 0.0                                # single zero weights among the others
    if F > 1:
        w[2, :, 1, :] = 0.0                            # a frame switched off for one instance
    ref = tc.random_ref(o, model, xs, us, B, 44)
    base = (capi.FLAG_TRACKING_COST if flags == "track" else 0) | (capi.FLAG_NO_TENSORS if flags == "nt" else 0)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (capi.FLAG_FRAME_COST if on else 0)) as ctx:
            _setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
            if flags == "track":
                tc.upload_ref(ctx, ref)
            if on:
                ctx.set_frame_cost(frames=frames, target=tgt, weight=w)
            ctx.linearize(None if stages is None else capi.LIN_COST)
            got[on] = {s: ctx.download(s) for s in DERIVS}
    n = o.n
    for b in range(B):
        add = frame_derivs(o, xs[b], frames, tgt[b], w[b])
        if flags == "track":
            base_ex = tc.expected_derivs(o, 1.0, xs[b], us[b], ref, b)
            for s in ("LX", "LXX", "LFX", "LFXX"):
                assert rel_err(got[True][s][b], base_ex[s] + add[s]) <= 1e-12, (s, b)
        for s in ("LX", "LXX", "LFX", "LFXX"):
            ex = got[False][s][b] + add[s]
            assert np.max(np.abs(add[s])) > 0
            assert rel_err(got[True][s][b], ex) <= 1e-12, (s, b, rel_err(got[True][s][b], ex))
        for s in ("LU", "LUU", "LUX"):
            assert np.array_equal(got[True][s][b], got[False][s][b]), s
        for t in range(T):
            blk = got[True]["LXX"][b][t * n * n:(t + 1) * n * n].reshape(n, n)
            assert np.array_equal(blk, blk.T)
        blk = got[True]["LFXX"][b].reshape(n, n)
        assert np.array_equal(blk, blk.T)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo,F", [("tree38", 0, None, 4), ("chain6ff", 0, 0, 3), ("chain6", 2, None, 1), ("tree38_frame", 0, None, 3)])
def test_cost_seq_aug(gpu, name, fd_mode, fo, F):
    """COSTS_OLD / COSTS_NEW (which = 0 / 1) against the oracle's augmented cost plus the numpy frame terms, lf included"""
    capi = gpu
    T, B, mu = 12, 2, 30.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    frames = pick_frames(model, F)
    xs, us = _trajs(o, model, B, 51)
    xs2, us2 = _trajs(o, model, B, 61)
    tgt, w = random_task(o, xs, frames, B, 52)
    mults = tc._mults(o, xs[0], 53)
    with capi.Context(spec, flags=capi.FLAG_FRAME_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
        ctx.set_frame_cost(frames=frames, target=tgt, weight=w)
        ctx.cost_seq_aug(0, mu)
        ctx.cost_seq_aug(1, mu)
        got = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
    for which, (X, U) in ((0, (xs, us)), (1, (xs2, us2))):
        for b in range(B):
            ex = o.cost_seq_aug(X[b], U[b], mults, mu) + frame_terms(o, X[b], frames, tgt[b], w[b])
            assert got[which][b][T] != 0.0
            assert rel_err(got[which][b], ex) <= 1e-12, (which, b, rel_err(got[which][b], ex))


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,mu", [("tree38", 60, 1.0), ("chain6", 30, 10.0)])
def test_sweep_parity_nonzero_value(gpu, name, T, mu):
    """the backward sweep with V_x != 0 from the frame cost, on the device's own derivatives against Oracle.backward: restarts,
    mu and reg identical, every step redone alone by the oracle from the device's V(t+1) to 1e-10 (stepwise_backward_check).
    Tree38 at T = 60 runs on K3h"""
    from oracle.binding import Oracle
    capi = gpu
    model, spec, o = make(name, T, fd_mode=2)
    frames = pick_frames(model, 3)
    xs, us = _trajs(o, model, 1, 71, held=True)
    tgt, w = random_task(o, xs, frames, 1, 72, wscale=0.1, spread=0.05)
    mults = tc._mults(o, xs[0], 73)
    n, m = o.n, o.m
    with capi.Context(spec, flags=capi.FLAG_FRAME_COST | capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.set_frame_cost(frames=frames, target=tgt, weight=w)
        ctx.linearize()
        if name == "tree38":
            assert ctx.bwd_stream_bytes() == tc._k3h_bytes(n, m)
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
        e = int(o.ne[t])
        if not e:
            return Oracle(model, 1, dt=0.01, c=1.0, fd_mode=2)
        return Oracle(model, 1, dt=0.01, c=1.0, fd_mode=2, eq_kind=spec.eq_kind, eq_advance=2, ne=np.array([e], dtype=np.int64),
                      eq_target=np.zeros(e))
    worst = stepwise_backward_check(one_step_oracle, o, d, xs[0], mults, reg[0], mu_out[0], got["VX_TRACE"], got["VXX_TRACE"],
                                    got["FB_VAL"], got["FB_JAC"], range(T))
    print("stepwise worst", worst)
    assert worst < 1e-10, worst


def _full_cost(o, c, xs, us, frames, tgt, w, ref=None):
    out = frame_terms(o, xs, frames, tgt, w)
    if ref is not None:
        out += tc.track_terms(o, c, xs, us, ref)
    out[:o.T] += 0.5 * c * np.sum(us.reshape(o.T, o.m) ** 2, axis=1)
    return out


def _rollout(o, step, xs, us, fb, mu, lo, hi):
    if lo is None:
        _, xn, un = o.forward_alpha(step, xs, us, o.alloc_affine(0), fb, mu)
        return xn, un
    T, n, m, nx = o.T, o.n, o.m, o.nx
    X, U = xs.reshape(T + 1, nx), us.reshape(T, m)
    x = X[0].copy()
    xn, un = [x.copy()], []
    for t in range(T):
        K = fb["jac"][t * m * n:(t + 1) * m * n].reshape((m, n), order="F")
        u = U[t] + step * fb["val"][t * m:(t + 1) * m]
        u = u + K @ tc._diff(o, X[t], x)
        u = np.where(u < lo[t], lo[t], np.where(u > hi[t], hi[t], u))
        un.append(u)
        x = o.eval_f(x, u)
        xn.append(x.copy())
    return np.concatenate(xn), np.concatenate(un)


def _emulate_forward(o, c, xs, us, fb, mu, n_alpha, frames, tgt, w, lo=None, hi=None, ref=None):
    """sequential halving with the numpy cost: the first step 2^-k with sum_t (new - old) <= 0 (n_alpha = 0: the full step)"""
    old = _full_cost(o, c, xs, us, frames, tgt, w, ref).sum()
    for k in range(34):
        step = 2.0 ** -k
        xn, un = _rollout(o, step, xs, us, fb, mu, lo, hi)
        new = _full_cost(o, c, xn, un, frames, tgt, w, ref).sum()
        if n_alpha == 0 or new - old <= 0:
            return step, xn, un, new - old
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo,fwd_path,F,box,track", [
    ("tree38", None, 1, 4, False, False), ("chain6ff", 0, 0, 3, False, False), ("tree38ff", 0, 1, 3, False, False),
    ("tree38", None, 1, 1, True, False),
    ("tree38", None, 1, 3, False, True),            # tracking and frame terms inline together
    ("tree38ff", 0, 1, 3, True, False),             # free-flyer root with bounds
    ("tree38ff", 0, 1, 4, True, True),              # ... and with both kinds of terms
    ("chain6ff", 0, 0, 1, True, True)])             # lane-per-rollout forward with everything
@pytest.mark.parametrize("n_alpha", [0, 1, 8])
@pytest.mark.parametrize("k_scale", [1.0, 3.0])
def test_forward_matches_emulation(gpu, name, fo, fwd_path, F, box, track, n_alpha, k_scale):
    """accepted step, X_NEW, U_NEW and dcost against Oracle.forward_alpha rollouts costed with numpy; k_scale 3 overshoots so
    that the halving runs; box: control bounds that bind, the emulation clamps (test_control_bounds.py: _clamped_rollout);
    track: the tracking flag as well, its terms (test_tracking_cost.py: track_terms) add"""
    capi = gpu
    T, c, mu = 16, 1.0, 1.0
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo)
    frames = pick_frames(model, F)
    xs, us = _trajs(o, model, 1, 81, held=True)
    tgt, w = random_task(o, xs, frames, 1, 82, wscale=20.0, spread=0.1)
    lo = hi = None
    ref = tc.random_ref(o, model, xs, us, 1, 84, spread=0.2) if track else None
    flags = capi.FLAG_FRAME_COST | capi.FLAG_NO_TENSORS | (capi.FLAG_CONTROL_BOUNDS if box else 0) | (capi.FLAG_TRACKING_COST if track else 0)
    with capi.Context(spec, flags=flags) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        _setup(ctx, xs, us)
        if track:
            tc.upload_ref(ctx, ref)
        ctx.set_frame_cost(frames=frames, target=tgt, weight=w)
        ctx.linearize()
        ctx.backward(0.0, mu)
        if k_scale != 1.0:
            ctx.upload("FB_VAL", k_scale * ctx.download("FB_VAL"))
        fb = {"origin": ctx.download("FB_ORIGIN")[0], "val": ctx.download("FB_VAL")[0], "jac": ctx.download("FB_JAC")[0]}
        if box:
            rng = np.random.default_rng(83)
            width = 0.5 * np.abs(fb["val"]).reshape(T, o.m)
            lo = us[0].reshape(T, o.m) - width * rng.uniform(0.2, 1, size=(T, o.m))
            hi = us[0].reshape(T, o.m) + width * rng.uniform(0.2, 1, size=(T, o.m))
            ctx.set_control_bounds(lo=lo, hi=hi)
        rc, step, dcost = ctx.forward(mu, n_alpha=n_alpha)
        xn, un = ctx.download("X_NEW")[0], ctx.download("U_NEW")[0]
    em = _emulate_forward(o, c, xs[0], us[0], fb, mu, n_alpha, frames, tgt[0], w[0], lo, hi, ref)
    assert em is not None
    step_ref, xn_ref, un_ref, new = em
    print("forward", name, n_alpha, k_scale, "step", step[0], step_ref, "dcost", dcost[0], new)
    assert step[0] == step_ref, (step, step_ref)
    if box:
        Un = un.reshape(T, o.m)
        assert np.any(Un == lo) or np.any(Un == hi)
    assert rel_err(xn, xn_ref) < 1e-9 and rel_err(un, un_ref) < 1e-9
    assert abs(dcost[0] - new) <= 1e-9 * max(1.0, abs(new)), (dcost[0], new)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo,flags", [("chain6ff", 2, 0, 0), ("tree38", 0, 0, 1)])
def test_instances_are_independent(gpu, name, fd_mode, fo, flags):
    """batch 2 through linearise, sweep, forward: another target for instance 1 leaves instance 0's outputs bit-identical"""
    capi = gpu
    T, B, mu = 12, 2, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    frames = pick_frames(model, 3)
    xs, us = _trajs(o, model, B, 91, held=True)
    tgt, w = random_task(o, xs, frames, B, 92, wscale=0.1, spread=0.1)
    out = []
    for shift in (0.0, 0.3):
        tg = tgt.copy()
        tg[1] += shift
        with capi.Context(spec, flags=capi.FLAG_FRAME_COST | capi.FLAG_TRACE | flags) as ctx:
            _setup(ctx, xs, us)
            ctx.set_frame_cost(frames=frames, target=tg, weight=w)
            out.append(_run_all(ctx, mu, False))
    a, b = out
    assert not np.array_equal(a["LX"][1], b["LX"][1]) and not np.array_equal(a["COSTS_OLD"][1], b["COSTS_OLD"][1])
    for k in a:
        if isinstance(a[k], tuple):
            for u, v in zip(a[k][1:], b[k][1:]):
                assert np.array_equal(np.asarray(u)[0], np.asarray(v)[0]), k
        else:
            assert np.array_equal(a[k][0], b[k][0]), k


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,flags", [("chain6", 2, 0), ("tree38", 0, 1)])
def test_solve_matches_stepwise(gpu, name, fd_mode, flags):
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B, iters, thr, mu, w_, n_ = 10, 2, 5, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode)
    frames = pick_frames(model, 3)
    xs, us = _trajs(o, model, B, 101, held=True)
    tgt, w = random_task(o, xs, frames, B, 102)
    mults = tc._mults(o, xs[0], 103)

    def run(stepwise):
        with capi.Context(spec, flags=capi.FLAG_FRAME_COST | flags) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if o.Etot:
                ctx.upload("MULT_ORIGIN", xs[:, :T * o.nx])
            ctx.set_frame_cost(frames=frames, target=tgt, weight=w)
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
def test_reach_task_descends(gpu):
    """tree38, T = 40, two leaf frames reaching for points 0.15 away from where they are, with running and terminal weights:
    sum_t COSTS_OLD never increases over 8 iterations and both frames end closer to their goals than they began"""
    capi = gpu
    T, mu, iters = 40, 1.0, 8
    model, spec, o = make("tree38", T, fd_mode=0)
    fr = pick_frames(model, 4)
    frames = [fr[2], fr[3]]
    xs, us = _trajs(o, model, 1, 111)
    q0 = xs[0][:o.nq]
    rng = np.random.default_rng(112)
    goal = np.stack([o.frame_position(j, off, q0) + 0.15 * rng.normal(size=3) / np.sqrt(3) for j, off in frames])
    tgt = np.tile(goal, (T + 1, 1, 1))
    w = np.full((T + 1, 2, 3), 10.0)
    w[T] = 1000.0

    def errs(X):
        qT = X.reshape(T + 1, o.nx)[T][:o.nq]
        return [np.linalg.norm(o.frame_position(j, off, qT) - goal[f]) for f, (j, off) in enumerate(frames)]
    with capi.Context(spec, flags=capi.FLAG_FRAME_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        ctx.set_frame_cost(frames=frames, target=tgt, weight=w)
        costs = []
        for _ in range(iters):
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            rc, step, dcost = ctx.forward(mu_o, n_alpha=8)
            costs.append(ctx.download("COSTS_OLD")[0].sum())
            ctx.swap_traj()
        final = ctx.download("X")[0]
    print("reach costs", costs, "errors", errs(xs[0]), "->", errs(final))
    for a, b in zip(costs, costs[1:]):
        assert b <= a * (1 + 1e-12), costs
    assert costs[-1] < costs[0]
    e0, e1 = errs(xs[0]), errs(final)
    assert e1[0] < e0[0] and e1[1] < e0[1], (e0, e1)


@pytest.mark.gpu
def test_refusals_and_defaults(gpu):
    import ctypes as C
    capi = gpu
    T, B = 4, 2
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    L = capi.lib()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def code(fn):
        with pytest.raises(capi.DdpHipError) as exc:
            fn()
        return exc.value.code
    with capi.Context(spec) as ctx:                                   # a context without the flag
        assert code(lambda: ctx.set_frame_cost(frames=[(1, (0, 0, 0.1))])) == capi.E_UNSUPPORTED
        ctx.n_cost_frames = 1
        assert code(lambda: ctx.set_frame_cost(weight=1.0)) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.frame_cost()) == capi.E_UNSUPPORTED
    pend = capi.BuiltinModel(capi.BUILTIN_PENDULUM)
    with pytest.raises(capi.DdpHipError) as exc:
        capi.Context(capi.ProblemSpec(pend, T, fd_mode=2), flags=capi.FLAG_FRAME_COST)
    assert exc.value.code == capi.E_UNSUPPORTED
    with capi.Context(spec, flags=capi.FLAG_FRAME_COST) as ctx:
        # before frames are set: nothing to download, uploads refused
        t0, w0 = ctx.frame_cost()
        assert t0.shape == (B, T + 1, 0, 3) and w0.shape == (B, T + 1, 0, 3)
        assert code(lambda: ctx.set_frame_cost(weight=1.0)) == capi.E_ARG
        z = np.zeros(B * (T + 1) * 3)
        assert L.ddp_hip_frame_cost_upload(ctx._h, z.ctypes.data_as(dp), z.ctypes.data_as(dp), 0, B) == capi.E_ARG
        nj = model.nj
        assert code(lambda: ctx.set_frame_cost(frames=[])) == capi.E_ARG
        assert code(lambda: ctx.set_frame_cost(frames=[(1, (0, 0, 0))] * 5)) == capi.E_ARG
        assert code(lambda: ctx.set_frame_cost(frames=[(nj, (0, 0, 0))])) == capi.E_ARG
        assert code(lambda: ctx.set_frame_cost(frames=[(-1, (0, 0, 0))])) == capi.E_ARG
        assert code(lambda: ctx.set_frame_cost(frames=[(1, (0, np.nan, 0))])) == capi.E_ARG
        assert code(lambda: ctx.set_frame_cost(frames=[(1, (0, np.inf, 0))])) == capi.E_ARG
        assert ctx.n_cost_frames == 0
        frames = pick_frames(model, 3)
        ctx.set_frame_cost(frames=frames)
        t0, w0 = ctx.frame_cost()                                       # create: targets 0, weights 0
        assert t0.shape == (B, T + 1, 3, 3) and np.all(t0 == 0.0) and np.all(w0 == 0.0)
        for bad in (-1e-3, np.nan, np.inf):
            wb = np.ones((T + 1, 3, 3)); wb[1, 2, 0] = bad
            assert code(lambda: ctx.set_frame_cost(weight=wb)) == capi.E_ARG, bad
        for bad in (np.nan, -np.inf):
            tb = np.ones((T + 1, 3, 3)); tb[2, 1, 1] = bad
            assert code(lambda: ctx.set_frame_cost(target=tb, weight=1.0)) == capi.E_ARG, bad
        t0, w0 = ctx.frame_cost()
        assert np.all(t0 == 0.0) and np.all(w0 == 0.0)                  # a refused upload leaves both sides as they were
        rng = np.random.default_rng(5)
        tg, wg = rng.normal(size=(B, T + 1, 3, 3)), rng.uniform(0, 1, size=(B, T + 1, 3, 3))
        ctx.set_frame_cost(target=tg, weight=wg)
        t1, w1 = ctx.frame_cost()
        assert np.array_equal(t1, tg) and np.array_equal(w1, wg)
        ctx.set_frame_cost(target=tg[1] + 1.0, first=1, count=1)        # one side, one instance; the weights stay
        t1, w1 = ctx.frame_cost()
        assert np.array_equal(t1[0], tg[0]) and np.array_equal(t1[1], tg[1] + 1.0) and np.array_equal(w1, wg)
        ctx.set_frame_cost(weight=np.array([1.0, 2.0, 3.0]))            # broadcast: (3,), (F, 3), scalar
        assert np.array_equal(ctx.frame_cost()[1], np.broadcast_to([1.0, 2.0, 3.0], (B, T + 1, 3, 3)))
        ctx.set_frame_cost(weight=np.arange(9.0).reshape(3, 3))
        assert np.array_equal(ctx.frame_cost()[1], np.broadcast_to(np.arange(9.0).reshape(3, 3), (B, T + 1, 3, 3)))
        ctx.set_frame_cost(weight=0.5)
        assert np.all(ctx.frame_cost()[1] == 0.5)
        ctx.set_frame_cost(frames=frames[::-1])                         # the same count: targets and weights stay
        t2, w2 = ctx.frame_cost()
        assert np.array_equal(t2, t1) and np.all(w2 == 0.5)
        ctx.set_frame_cost(frames=frames[:2])                           # another count: both reset to 0
        t3, w3 = ctx.frame_cost()
        assert t3.shape == (B, T + 1, 2, 3) and np.all(t3 == 0.0) and np.all(w3 == 0.0)
        assert code(lambda: ctx.frame_cost(first=1, count=B)) == capi.E_ARG
