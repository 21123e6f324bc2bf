"""Per-instance frame-orientation costs (DDP_HIP_FLAG_FRAME_ORIENT_COST, include/ddp_hip/ddp_hip.h), of the cost frames of
DDP_HIP_FLAG_FRAME_COST:

    e_f = log3(R_ref^T R_f(q_t)),   l(t, x, u) += 1/2 sum_f sum_a w[b][t][f][a] e_f,a^2,   lf(x_T) alike with w[b][T]

with R_f the world rotation of joint joint_f's frame and R_ref the rotation of the unit quaternion r[b][t][f] (x y z w).  The
oracle has no such cost, so the yardstick is the numpy restatement below, built only on the oracle's public kinematics: the
columns of R_f are frame_position(j, e_a, q) - frame_position(j, 0, q), and the world angular jacobian W_f comes from
1/2 sum_a (R e_a) x (P_{e_a} - P_0) with P = frame_jacobian(world_aligned=True).  The position terms, tracking terms and limit
terms next to it come from the helpers of test_frame_cost.py, test_tracking_cost.py and test_state_limits.py; tolerances are
those of test_frame_cost.py.  References are R_f(q_t) exp(-a) with |a| in [0.05, 2.5] rad: both sides of so3_coeffs' series
switch at 0.2 rad, clear of pi."""
import os
import re

import numpy as np
import pytest

import test_frame_cost as fc
import test_state_limits as sl
import test_tracking_cost as tc
from problems import make
from synth import rel_err, stepwise_backward_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 1e-3
DERIVS = fc.DERIVS
NAMES = fc.NAMES


# ---- SO(3) in numpy --------------------------------------------------------------------------------------------------------
def quat_to_R(qt):
    x, y, z, w = qt
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def R_to_quat(M):
    """x y z w, by the largest of trace and diagonal entries (no cancellation at any angle), normalised"""
    tr = M[0, 0] + M[1, 1] + M[2, 2]
    if tr > 0:
        s = 2 * np.sqrt(tr + 1)
        qt = [(M[2, 1] - M[1, 2]) / s, (M[0, 2] - M[2, 0]) / s, (M[1, 0] - M[0, 1]) / s, 0.25 * s]
    elif M[0, 0] > M[1, 1] and M[0, 0] > M[2, 2]:
        s = 2 * np.sqrt(1 + M[0, 0] - M[1, 1] - M[2, 2])
        qt = [0.25 * s, (M[0, 1] + M[1, 0]) / s, (M[0, 2] + M[2, 0]) / s, (M[2, 1] - M[1, 2]) / s]
    elif M[1, 1] > M[2, 2]:
        s = 2 * np.sqrt(1 + M[1, 1] - M[0, 0] - M[2, 2])
        qt = [(M[0, 1] + M[1, 0]) / s, 0.25 * s, (M[1, 2] + M[2, 1]) / s, (M[0, 2] - M[2, 0]) / s]
    else:
        s = 2 * np.sqrt(1 + M[2, 2] - M[0, 0] - M[1, 1])
        qt = [(M[0, 2] + M[2, 0]) / s, (M[1, 2] + M[2, 1]) / s, 0.25 * s, (M[1, 0] - M[0, 1]) / s]
    qt = np.array(qt)
    return qt / np.linalg.norm(qt)


def log3_quat(M):
    """log of a rotation matrix through its quaternion: 2 atan2(|v|, w) v / |v|"""
    qt = R_to_quat(M)
    if qt[3] < 0:
        qt = -qt
    nn = np.linalg.norm(qt[:3])
    if nn < 1e-8:
        return 2.0 * qt[:3] / qt[3]
    return 2 * np.arctan2(nn, qt[3]) / nn * qt[:3]


def log3_matrix(M):
    """the same log from the antisymmetric part and the trace (good away from pi)"""
    v = 0.5 * np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
    nn = np.linalg.norm(v)
    if nn < 1e-8:
        return v
    return np.arctan2(nn, 0.5 * (np.trace(M) - 1)) / nn * v


def skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def exp3(a):
    t = np.linalg.norm(a)
    if t < 1e-8:
        return np.eye(3) + skew(a)
    K = skew(a / t)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def Jlog3(e):
    """I + 1/2 [e]x + d [e]x^2, d = (1 - (t/2) cot(t/2)) / t^2"""
    t2 = float(e @ e)
    if t2 < 1e-4:
        d = 1.0 / 12 + t2 / 720 + t2 * t2 / 30240
    else:
        t = np.sqrt(t2)
        d = (1 - 0.5 * t / np.tan(0.5 * t)) / t2
    E = skew(e)
    return np.eye(3) + 0.5 * E + d * (E @ E)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def frame_R(o, j, q):
    """R_f: its columns are frame_position(j, e_a, q) - frame_position(j, 0, q)"""
    p0 = o.frame_position(j, (0.0, 0.0, 0.0), q)
    return np.stack([o.frame_position(j, tuple(e), q) - p0 for e in np.eye(3)], axis=1)


def frame_W(o, j, q, R):
    """the world angular jacobian (3 x nv): column i is w_i with d(R e_a) = w_i x (R e_a), and sum_a r_a x (w x r_a) = 2 w"""
    P0 = o.frame_jacobian(j, (0.0, 0.0, 0.0), q, world_aligned=True)
    W = np.zeros_like(P0)
    for a, e in enumerate(np.eye(3)):
        dP = o.frame_jacobian(j, tuple(e), q, world_aligned=True) - P0
        W += 0.5 * np.cross(R[:, a][:, None], dP, axis=0)
    return W


def orient_error(o, j, q, qt, log=log3_quat):
    return log(quat_to_R(qt).T @ frame_R(o, j, q))


def orient_terms(o, xs, frames, quat, w, log=log3_quat):
    """the orientation terms of one instance per t (T+1 values; the last belongs to lf); quat (T+1, F, 4), w (T+1, F, 3).  A
    frame whose weights are all 0 is not walked"""
    X = xs.reshape(o.T + 1, o.nx)
    out = np.zeros(o.T + 1)
    for t in range(o.T + 1):
        for f, (j, _) in enumerate(frames):
            if not np.any(w[t][f] != 0.0):
                continue
            e = orient_error(o, j, X[t][:o.nq], quat[t][f], log)
            out[t] += 0.5 * np.sum(w[t][f] * e * e)
    return out


def orient_grad_hess(o, x, frames, quat_t, w_t):
    """(lx, lxx) contributions at one state: A^T (w o e) and the Gauss-Newton A^T diag(w) A on the q rows, A = Jlog3(e) R^T W"""
    nv, n = o.nv, o.n
    g, Hm = np.zeros(n), np.zeros((n, n))
    q = x[:o.nq]
    for f, (j, _) in enumerate(frames):
        if not np.any(w_t[f] != 0.0):
            continue
        R = frame_R(o, j, q)
        e = log3_quat(quat_to_R(quat_t[f]).T @ R)
        A = Jlog3(e) @ R.T @ frame_W(o, j, q, R)
        g[:nv] += A.T @ (w_t[f] * e)
        for a in range(3):                               # entry (i, j) and (j, i) alike: symmetric bit for bit
            Hm[:nv, :nv] += w_t[f][a] * np.outer(A[a], A[a])
    return g, Hm


def orient_derivs(o, xs, frames, quat, w):
    """what the orientation terms add to LX, LXX, LFX, LFXX of one instance, in the library's flat (column-major) layout"""
    X = xs.reshape(o.T + 1, o.nx)
    out = {"LX": [], "LXX": []}
    for t in range(o.T + 1):
        g, Hm = orient_grad_hess(o, X[t], frames, quat[t], w[t])
        if t == o.T:
            out["LFX"], out["LFXX"] = g, Hm.ravel(order="F")
        else:
            out["LX"].append(g); out["LXX"].append(Hm.ravel(order="F"))
    out["LX"], out["LXX"] = np.concatenate(out["LX"]), np.concatenate(out["LXX"])
    return out


def random_orient(o, xs, frames, B, seed, wscale=1.0, lo=0.05, hi=2.5):
    """per-instance references R_f(q_t) exp(-a), |a| uniform in [lo, hi] rad (one in three below so3_coeffs' switch at 0.2
    when lo allows), as unit quaternions of either sign, and positive weights"""
    rng = np.random.default_rng(seed)
    T, F = o.T, len(frames)
    quat = np.zeros((B, T + 1, F, 4))
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            for f, (j, _) in enumerate(frames):
                ax = rng.normal(size=3)
                ang = rng.uniform(lo, min(hi, 0.19)) if (rng.uniform() < 1.0 / 3 and lo < 0.19) else rng.uniform(lo, hi)
                qt = R_to_quat(frame_R(o, j, X[t][:o.nq]) @ exp3(-ang * ax / np.linalg.norm(ax)))
                quat[b, t, f] = qt if rng.uniform() < 0.5 else -qt
    return quat, wscale * rng.uniform(0.1, 2.0, size=(B, T + 1, F, 3))


def identity_quat(shape):
    qt = np.zeros(shape + (4,))
    qt[..., 3] = 1.0
    return qt


# ---- CPU: the yardstick checks itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain6", "tree38", "chain6ff", "tree38ff"])
def test_yardstick_gradient(name):
    """lx against the 5-point central difference of the numpy cost along x (+) (+-h e_j); with the references at R_f(q) (e = 0,
    where Gauss-Newton is exact) lxx against the central difference of the gradient; lxx symmetric bit for bit with zero
    velocity rows and columns.  Four frames (joint 0, a mid-tree joint, two leaves)"""
    T = 2
    model, _, o = make(name, T, fd_mode=0)
    frames = fc.pick_frames(model, 4)
    xs, us = tc._trajs(o, model, 1, 3)
    quat, w = random_orient(o, xs, frames, 1, 4)
    X = xs[0].reshape(T + 1, o.nx)
    nv, n = o.nv, o.n
    w5 = ((-2, 1.0 / 12), (-1, -8.0 / 12), (1, 8.0 / 12), (2, -1.0 / 12))
    t = 1
    g, Hm = orient_grad_hess(o, X[t], frames, quat[0][t], w[0][t])
    assert np.max(np.abs(g[:nv])) > 0

    def cost_at(dx):
        X2 = X.copy()
        X2[t] = tc._integrate_x(o, X[t], dx)
        return orient_terms(o, X2.ravel(), frames, quat[0], w[0])[t]
    fd = np.zeros(n)
    for j in range(n):
        e = np.zeros(n); e[j] = H
        fd[j] = sum(cw * cost_at(s * e) for s, cw in w5) / H
    assert np.max(np.abs(fd - g)) <= 1e-8 * max(1.0, np.max(np.abs(g))), np.max(np.abs(fd - g))
    # e = 0 at X[t]: the gradient's central difference is the Gauss-Newton block
    q0 = np.stack([R_to_quat(frame_R(o, j, X[t][:o.nq])) for j, _ in frames])
    g0, H0 = orient_grad_hess(o, X[t], frames, q0, w[0][t])
    assert np.max(np.abs(g0)) <= 1e-13

    def grad_at(dx):
        return orient_grad_hess(o, tc._integrate_x(o, X[t], dx), frames, q0, w[0][t])[0]
    fdh = np.zeros((n, n))
    for j in range(n):
        e = np.zeros(n); e[j] = H
        fdh[:, j] = sum(cw * grad_at(s * e) for s, cw in w5) / H
    assert np.max(np.abs(fdh - H0)) <= 1e-8 * max(1.0, np.max(np.abs(H0))), np.max(np.abs(fdh - H0))
    assert np.array_equal(Hm, Hm.T)
    assert np.all(Hm[nv:, :] == 0.0) and np.all(Hm[:, nv:] == 0.0) and np.all(g[nv:] == 0.0)
    # the two logs agree on these inputs, and r / -r are the same reference
    for f, (j, _) in enumerate(frames):
        ea = orient_error(o, j, X[t][:o.nq], quat[0][t][f])
        eb = orient_error(o, j, X[t][:o.nq], -quat[0][t][f], log3_matrix)
        assert np.max(np.abs(ea - eb)) <= 1e-13 and 0.04 < np.linalg.norm(ea) < 2.6


def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.FLAG_FRAME_ORIENT_COST == 64 and re.search(r"#define\s+DDP_HIP_FLAG_FRAME_ORIENT_COST\s+64u", header)
    L = capi.lib()
    for name in ("ddp_hip_frame_orient_upload", "ddp_hip_frame_orient_download"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert len(capi.SEQ_NAMES) == 40 and capi.SEQ_NAMES[-3:] == ["CTRL_LO", "CTRL_HI", "BOX_STAT"]
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    assert re.search(r"DDP_HIP_SEQ_BOX_STAT,[^\n]*\n\s*DDP_HIP_SEQ_COUNT", header)        # no ddp_hip_seq entries added
    # shapes and unit norms are checked before anything reaches the library: a context object without a device will do
    T, B = 5, 2
    model, spec, _ = make("chain6", T, batch=B, fd_mode=0)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx.n_cost_frames, ctx._h = spec, B, 3, None
    bad_q = identity_quat((T + 1, 3)); bad_q[2, 1, 3] = 1.0 + 1e-8
    zero_q = np.zeros((T + 1, 3, 4))
    nan_q = identity_quat((T + 1, 3)); nan_q[0, 0, 0] = np.nan
    for kw in (dict(quat=identity_quat((T, 3))), dict(quat=identity_quat((T + 1, 2))), dict(quat=np.zeros((T + 1, 3, 3))),
               dict(quat=identity_quat((3,))), dict(quat=identity_quat((B + 1, T + 1, 3))),
               dict(quat=identity_quat((B, T + 1, 3)), count=1), dict(quat=bad_q), dict(quat=zero_q), dict(quat=nan_q),
               dict(weight=np.zeros((T + 1, 3))), dict(weight=np.zeros((B + 1, T + 1, 3, 3))), dict(weight=np.zeros(2)),
               dict(weight=np.zeros((T + 1, 3, 4)))):
        with pytest.raises(ValueError):
            ctx.set_frame_orient_cost(**kw)
    assert hasattr(ctx, "frame_orient_cost")


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _flags(capi):
    return capi.FLAG_FRAME_COST | capi.FLAG_FRAME_ORIENT_COST


def _first(r):
    """instance 0's share of a _run_all result"""
    return {k: (tuple(np.asarray(v)[..., :1] for v in r[k][1:]) if isinstance(r[k], tuple) else (r[k][:1] if k != "stream" else r[k]))
            for k in r}


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,fd_mode,fo,extra,fwd_path", [
    ("tree38", 12, 2, None, "", 1),                 # latency forward
    ("chain6ff", 10, 2, 0, "", 0),                  # lane-per-rollout forward
    ("tree38_frame", 12, 0, None, "", 1),           # constrained: the candidates' costs from cand_cost_kernel
    ("tree38", 12, 2, None, "track", 1),
    ("tree38", 12, 2, None, "box", 1),
    ("tree38", 12, 2, None, "limit", 1),
])
@pytest.mark.parametrize("mode", ["nothing_uploaded", "zero_weights", "no_frames", "zero_instance"])
def test_zero_weights_change_nothing(gpu, name, T, fd_mode, fo, extra, fwd_path, mode):
    """nothing_uploaded / zero_weights: both flags, live position weights, no orientation upload or references far away with
    every orientation weight 0: bit for bit what DDP_HIP_FLAG_FRAME_COST alone computes.  no_frames: both flags and no frames:
    bit for bit the context without either.  zero_instance: batch 2, instance 1 carries orientation weights (the level-2
    kernels run), instance 0 none: instance 0 is bit for bit the position-only context's instance 0"""
    capi = gpu
    mu = 10.0
    B = 2 if mode == "zero_instance" else 1
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    frames = fc.pick_frames(model, 3)
    xs, us = tc._trajs(o, model, B, 31, held=True)
    mults = tc._mults(o, xs[0], 32)
    tgt, w = fc.random_task(o, xs, frames, B, 33, spread=0.2)
    w *= 0.05
    quat, ow = random_orient(o, xs, frames, B, 35, wscale=0.05)
    if mode == "zero_instance":
        ow[0] = 0.0
    else:
        ow[:] = 0.0
    base = capi.FLAG_TRACE | {"": 0, "track": capi.FLAG_TRACKING_COST, "box": capi.FLAG_CONTROL_BOUNDS, "limit": capi.FLAG_STATE_LIMITS}[extra]
    ref = tc.random_ref(o, model, xs, us, B, 34, wscale=0.05, spread=0.05)
    lim = sl.random_limits(o, xs, B, 36, wscale=0.05)
    out = {}
    for on in (False, True):
        fl = (_flags(capi) if on else (0 if mode == "no_frames" else capi.FLAG_FRAME_COST))
        with capi.Context(spec, flags=base | fl) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            tc._setup(ctx, xs, us, mults, o.Etot)
            if extra == "track":
                tc.upload_ref(ctx, ref)
            if extra == "box":
                ctx.set_control_bounds(lo=-1e6, hi=1e6)
            if extra == "limit":
                ctx.set_state_limits(lo=lim[0], hi=lim[1], weight=lim[2])
            if mode != "no_frames":
                ctx.set_frame_cost(frames=frames, target=tgt, weight=w)
                if on and mode != "nothing_uploaded":
                    ctx.set_frame_orient_cost(quat=quat, weight=ow)
            out[on] = fc._run_all(ctx, mu, name == "tree38")
    a, b = out[False], out[True]
    if mode == "zero_instance":
        assert not np.array_equal(a["LX"][1], b["LX"][1])            # the orientation terms are there for instance 1
        assert not np.array_equal(a["COSTS_OLD"][1], b["COSTS_OLD"][1])
        a, b = _first(a), _first(b)
    fc._same(a, b)
    assert np.all(np.isfinite(b["LX"])) and np.all(np.isfinite(b["X_NEW"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo,flags,F", [
    ("chain6", 2, None, "", 3), ("tree38", 2, None, "", 4), ("chain6ff", 2, 0, "", 4), ("tree38ff", 0, 0, "nt", 3),
    ("tree38", 2, None, "track+limit", 1)])
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, name, fd_mode, fo, flags, F, stages):
    """LX, LXX, LFX, LFXX against the position-only context's values plus the definition's terms, batch 3 with different
    references and weights per instance, through ddp_hip_linearize and ddp_hip_linearize_stages(LIN_COST); single zero weights,
    one frame switched off for one instance, one frame with position weights only beside one with orientation weights only;
    LXX symmetric bit for bit; LU, LUU, LUX bit for bit the position-only values"""
    capi = gpu
    T, B = 6, 3
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    frames = fc.pick_frames(model, F)
    xs, us = tc._trajs(o, model, B, 41)
    tgt, w = fc.random_task(o, xs, frames, B, 42)
    quat, ow = random_orient(o, xs, frames, B, 45)
    ow[1, 2, 0, 1] = 0.0                               # single zero weights among the others
    ow[0, :, 0, 2] = 0.0
    if F > 1:
        ow[2, :, 1, :] = 0.0                           # a frame switched off for one instance
        ow[:, :, 0, :] = 0.0                           # frame 0 (joint 0): position weights only ...
        w[:, :, F - 1, :] = 0.0                        # ... the last frame (a leaf): orientation weights only
        ow[1, :, 0, :] = 1.5                           # (but joint 0's orientation for instance 1: a path of length 1)
    ref = tc.random_ref(o, model, xs, us, B, 44)
    lim = sl.random_limits(o, xs, B, 46)
    base = (capi.FLAG_TRACKING_COST | capi.FLAG_STATE_LIMITS if flags == "track+limit" else 0) | (capi.FLAG_NO_TENSORS if flags == "nt" else 0)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (_flags(capi) if on else capi.FLAG_FRAME_COST)) as ctx:
            tc._setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
            if flags == "track+limit":
                tc.upload_ref(ctx, ref)
                ctx.set_state_limits(lo=lim[0], hi=lim[1], weight=lim[2])
            ctx.set_frame_cost(frames=frames, target=tgt, weight=w)
            if on:
                ctx.set_frame_orient_cost(quat=quat, weight=ow)
            ctx.linearize(None if stages is None else capi.LIN_COST)
            got[on] = {s: ctx.download(s) for s in DERIVS}
    n = o.n
    worst = 0.0
    for b in range(B):
        add = orient_derivs(o, xs[b], frames, quat[b], ow[b])
        for s in ("LX", "LXX", "LFX", "LFXX"):
            ex = got[False][s][b] + add[s]
            assert np.max(np.abs(add[s])) > 0
            err = rel_err(got[True][s][b], ex)
            worst = max(worst, err)
            print("linearize", name, flags, stages, s, b, err)
            assert err <= 1e-12, (s, b, err)
        for s in ("LU", "LUU", "LUX"):
            assert np.array_equal(got[True][s][b], got[False][s][b]), s
        for t in range(T):
            blk = got[True]["LXX"][b][t * n * n:(t + 1) * n * n].reshape(n, n)
            assert np.array_equal(blk, blk.T)
        blk = got[True]["LFXX"][b].reshape(n, n)
        assert np.array_equal(blk, blk.T)
    print("linearize worst", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo,F", [("tree38", 0, None, 4), ("chain6ff", 0, 0, 3), ("chain6", 2, None, 1), ("tree38_frame", 0, None, 3)])
def test_cost_seq_aug(gpu, name, fd_mode, fo, F):
    """COSTS_OLD / COSTS_NEW (which = 0 / 1) against the oracle's augmented cost plus the numpy position and orientation terms,
    lf included; a reference given as -r yields the same costs"""
    capi = gpu
    T, B, mu = 8, 2, 30.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    frames = fc.pick_frames(model, F)
    xs, us = tc._trajs(o, model, B, 51)
    xs2, us2 = tc._trajs(o, model, B, 61)
    tgt, w = fc.random_task(o, xs, frames, B, 52)
    quat, ow = random_orient(o, xs, frames, B, 54)
    mults = tc._mults(o, xs[0], 53)
    got = {}
    with capi.Context(spec, flags=_flags(capi) | capi.FLAG_NO_TENSORS) as ctx:
        tc._setup(ctx, xs, us, mults, o.Etot)
        ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
        ctx.set_frame_cost(frames=frames, target=tgt, weight=w)
        for sign in (1.0, -1.0):
            ctx.set_frame_orient_cost(quat=sign * quat, weight=ow)
            ctx.cost_seq_aug(0, mu)
            ctx.cost_seq_aug(1, mu)
            got[sign] = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
    for which, (X, U) in ((0, (xs, us)), (1, (xs2, us2))):
        for b in range(B):
            add = orient_terms(o, X[b], frames, quat[b], ow[b])
            assert np.all(add > 0)
            ex = o.cost_seq_aug(X[b], U[b], mults, mu) + fc.frame_terms(o, X[b], frames, tgt[b], w[b]) + add
            assert got[1.0][which][b][T] != 0.0
            err = rel_err(got[1.0][which][b], ex)
            print("cost_seq_aug", name, which, b, err)
            assert err <= 1e-12, (which, b, err)
            assert rel_err(got[-1.0][which][b], got[1.0][which][b]) <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,mu", [("tree38", 60, 1.0), ("chain6", 30, 10.0)])
def test_sweep_parity_nonzero_value(gpu, name, T, mu):
    """the backward sweep with V_x != 0 from the orientation cost, on the device's own derivatives against Oracle.backward:
    restarts, mu and reg identical, every step redone alone by the oracle from the device's V(t+1) to 1e-10
    (stepwise_backward_check).  Tree38 at T = 60 runs on K3h, as in test_frame_cost.py"""
    from oracle.binding import Oracle
    capi = gpu
    model, spec, o = make(name, T, fd_mode=2)
    frames = fc.pick_frames(model, 3)
    xs, us = tc._trajs(o, model, 1, 71, held=True)
    quat, ow = random_orient(o, xs, frames, 1, 72, wscale=0.1, lo=0.05, hi=0.1)   # (small: the sweep must stay positive definite)
    mults = tc._mults(o, xs[0], 73)
    n, m = o.n, o.m
    with capi.Context(spec, flags=_flags(capi) | capi.FLAG_TRACE) as ctx:
        tc._setup(ctx, xs, us, mults, o.Etot)
        ctx.set_frame_cost(frames=frames)
        ctx.set_frame_orient_cost(quat=quat, weight=ow)
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


def _emulate_forward(o, xs, us, mults, fb, mu, cost, lo=None, hi=None):
    """sequential halving with the numpy cost: the first step 2^-k with sum_t (new - old) <= 0"""
    old = cost(xs, us).sum()
    for k in range(34):
        step = 2.0 ** -k
        if lo is None:
            _, xn, un = o.forward_alpha(step, xs, us, mults, fb, mu)
        else:
            xn, un = fc._rollout(o, step, xs, us, fb, mu, lo, hi)
        new = cost(xn, un).sum()
        if new - old <= 0:
            return step, xn, un, new - old
    return None


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo,fwd_path,F,extra", [
    ("tree38", None, 1, 4, ""), ("tree38", None, 1, 1, "box"), ("tree38", None, 1, 4, "track+limit"),
    ("tree38ff", 0, 1, 1, ""), ("tree38ff", 0, 1, 4, "box+track+limit"),
    ("tree38_frame", None, 1, 4, ""),               # constrained: the candidates' costs from cand_cost_kernel
    ("chain6", None, 0, 4, ""),                     # lane-per-rollout forward, fixed base (config constraint at every step)
    ("chain6ff", 0, 0, 1, ""), ("chain6ff", 0, 0, 4, "box+track+limit")])
@pytest.mark.parametrize("k_scale", [1.0, 3.0])
def test_forward_matches_emulation(gpu, name, fo, fwd_path, F, extra, k_scale):
    """accepted step, X_NEW, U_NEW and dcost against Oracle.forward_alpha rollouts costed with numpy (Oracle.cost_seq_aug +
    position + orientation terms + tracking and limit terms where flagged), with n_alpha = 1 and 8, which also give the same
    accepted step and X_NEW as each other; k_scale 3 overshoots so that the halving runs; box: control bounds that bind on every
    third control, the emulation clamps"""
    capi = gpu
    T, c, mu = 12, 1.0, 1.0
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo)
    frames = fc.pick_frames(model, F)
    xs, us = tc._trajs(o, model, 1, 81, held=True)
    tgt, w = fc.random_task(o, xs, frames, 1, 82, wscale=20.0, spread=0.1)
    quat, ow = random_orient(o, xs, frames, 1, 85, wscale=5.0)
    mults = tc._mults(o, xs[0], 87)
    box, track, limit = "box" in extra, "track" in extra, "limit" in extra
    ref = tc.random_ref(o, model, xs, us, 1, 84, spread=0.2) if track else None
    lim = sl.random_limits(o, xs, 1, 86, wscale=5.0) if limit else None
    lo = hi = None
    flags = _flags(capi) | capi.FLAG_NO_TENSORS | (capi.FLAG_CONTROL_BOUNDS if box else 0) | (capi.FLAG_TRACKING_COST if track else 0) | \
        (capi.FLAG_STATE_LIMITS if limit else 0)
    res = {}
    with capi.Context(spec, flags=flags) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        tc._setup(ctx, xs, us, mults, o.Etot)
        if track:
            tc.upload_ref(ctx, ref)
        if limit:
            ctx.set_state_limits(lo=lim[0], hi=lim[1], weight=lim[2])
        ctx.set_frame_cost(frames=frames, target=tgt, weight=w)
        ctx.set_frame_orient_cost(quat=quat, weight=ow)
        ctx.linearize()
        _, _, mu_o, _ = ctx.backward(0.0, mu)
        if k_scale != 1.0:
            ctx.upload("FB_VAL", k_scale * ctx.download("FB_VAL"))
        fb = {"origin": ctx.download("FB_ORIGIN")[0], "val": ctx.download("FB_VAL")[0], "jac": ctx.download("FB_JAC")[0]}
        if box:
            rng = np.random.default_rng(83)
            width = 0.5 * np.abs(fb["val"]).reshape(T, o.m) / k_scale
            tight = (np.arange(o.m) % 3 == 0)[None, :]
            lo = np.where(tight, us[0].reshape(T, o.m) - width * rng.uniform(0.2, 1, size=(T, o.m)), -np.inf)
            hi = np.where(tight, us[0].reshape(T, o.m) + width * rng.uniform(0.2, 1, size=(T, o.m)), np.inf)
            ctx.set_control_bounds(lo=lo, hi=hi)
        for n_alpha in (1, 8):
            rc, step, dcost = ctx.forward(mu_o, n_alpha=n_alpha)
            res[n_alpha] = (step[0], dcost[0], ctx.download("X_NEW")[0], ctx.download("U_NEW")[0])

    def cost(X, U):
        out = o.cost_seq_aug(X, U, mults, mu_o[0]) + fc.frame_terms(o, X, frames, tgt[0], w[0]) + orient_terms(o, X, frames, quat[0], ow[0])
        if track:
            out += tc.track_terms(o, c, X, U, ref)
        if limit:
            out += sl.limit_terms(o, X, lim[0][0], lim[1][0], lim[2][0])
        return out
    em = _emulate_forward(o, xs[0], us[0], mults, fb, mu_o[0], cost, lo, hi)
    assert em is not None
    step_ref, xn_ref, un_ref, new = em
    for n_alpha in (1, 8):
        step, dcost, xn, un = res[n_alpha]
        print("forward", name, extra, n_alpha, k_scale, "step", step, step_ref, "dcost", dcost, new)
        assert step == step_ref, (step, step_ref)
        if box:
            Un = un.reshape(T, o.m)
            assert np.any(Un == lo) or np.any(Un == hi)
        assert rel_err(xn, xn_ref) < 1e-9 and rel_err(un, un_ref) < 1e-9
        assert abs(dcost - new) <= 1e-9 * max(1.0, abs(new)), (dcost, new)
    assert res[1][0] == res[8][0] and np.array_equal(res[1][2], res[8][2])


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo,flags", [("chain6ff", 2, 0, 0), ("tree38", 0, 0, 1)])
def test_instances_are_independent(gpu, name, fd_mode, fo, flags):
    """batch 2 through linearise, sweep, forward: other references and weights for instance 1 leave instance 0's outputs
    bit-identical"""
    capi = gpu
    T, B, mu = 10, 2, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    frames = fc.pick_frames(model, 3)
    xs, us = tc._trajs(o, model, B, 91, held=True)
    quat, ow = random_orient(o, xs, frames, B, 92, wscale=0.1)
    quat2, ow2 = random_orient(o, xs, frames, B, 93, wscale=0.3)
    out = []
    for other in (False, True):
        qt, wt = quat.copy(), ow.copy()
        if other:
            qt[1], wt[1] = quat2[1], ow2[1]
        with capi.Context(spec, flags=_flags(capi) | capi.FLAG_TRACE | flags) as ctx:
            tc._setup(ctx, xs, us)
            ctx.set_frame_cost(frames=frames)
            ctx.set_frame_orient_cost(quat=qt, weight=wt)
            out.append(fc._run_all(ctx, mu, False))
    a, b = out
    assert not np.array_equal(a["LX"][1], b["LX"][1]) and not np.array_equal(a["COSTS_OLD"][1], b["COSTS_OLD"][1])
    fc._same(_first(a), _first(b))


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,flags", [("chain6", 2, 0), ("tree38", 0, 1)])
def test_solve_matches_stepwise(gpu, name, fd_mode, flags):
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B, iters, thr, mu, w_, n_ = 10, 2, 4, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode)
    frames = fc.pick_frames(model, 3)
    xs, us = tc._trajs(o, model, B, 101, held=True)
    tgt, w = fc.random_task(o, xs, frames, B, 102)
    quat, ow = random_orient(o, xs, frames, B, 104, hi=1.0)
    mults = tc._mults(o, xs[0], 103)

    def run(stepwise):
        with capi.Context(spec, flags=_flags(capi) | flags) as ctx:
            tc._setup(ctx, xs, us, mults, o.Etot)
            if o.Etot:
                ctx.upload("MULT_ORIGIN", xs[:, :T * o.nx])
            ctx.set_frame_cost(frames=frames, target=tgt, weight=w)
            ctx.set_frame_orient_cost(quat=quat, weight=ow)
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
@pytest.mark.parametrize("name,fo", [("tree38", None), ("chain6ff", 0)])
def test_orientation_task_descends(gpu, name, fo):
    """terminal and running orientation weights only (no position weights), two instances with different goals 0.5 rad away
    from where a leaf frame and the free-flyer root (fixed base: a mid-tree joint) are: over a few iterations no accepted step increases the total cost, which ends
    below where it began, and every instance ends with a smaller terminal orientation angle (the frames' angles summed,
    measured with the yardstick) than its initial trajectory's"""
    capi = gpu
    T, B, mu, iters = 16, 2, 1.0, 5
    model, spec, o = make(name, T, batch=B, fd_mode=0, first_order_fd=fo)
    fr = fc.pick_frames(model, 3)
    frames = [fr[0], fr[2]] if o.nq != o.nv else [fr[1], fr[2]]   # (joint 0 of the fixed-base tree is prismatic: its rotation is fixed)
    xs, us = tc._trajs(o, model, B, 111)
    rng = np.random.default_rng(112)
    quat = np.zeros((B, T + 1, 2, 4))
    for b in range(B):
        q0 = xs[b][:o.nq]
        for f, (j, _) in enumerate(frames):
            ax = rng.normal(size=3)
            quat[b, :, f] = R_to_quat(frame_R(o, j, q0) @ exp3(0.5 * ax / np.linalg.norm(ax)))
    ow = np.full((B, T + 1, 2, 3), 10.0)
    ow[:, T] = 1000.0

    def angles(X, b):
        qT = X.reshape(T + 1, o.nx)[T][:o.nq]
        return [np.linalg.norm(orient_error(o, j, qT, quat[b, T, f])) for f, (j, _) in enumerate(frames)]
    with capi.Context(spec, flags=_flags(capi) | capi.FLAG_NO_TENSORS) as ctx:
        tc._setup(ctx, xs, us)
        ctx.set_frame_cost(frames=frames)
        ctx.set_frame_orient_cost(quat=quat, weight=ow)
        costs = []
        for _ in range(iters):
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            rc, step, dcost = ctx.forward(mu_o, n_alpha=8)
            costs.append(ctx.download("COSTS_OLD").sum(axis=1))
            assert np.all(dcost <= 0)
            ctx.swap_traj()
        ctx.cost_seq_aug(0, mu_o)
        costs.append(ctx.download("COSTS_OLD").sum(axis=1))
        final = ctx.download("X")
    costs = np.array(costs)
    print("orientation task", name, "costs", costs.tolist())
    for b in range(B):
        a0, a1 = angles(xs[b], b), angles(final[b], b)
        print("  instance", b, "terminal angles", a0, "->", a1)
        for c0, c1 in zip(costs[:, b], costs[1:, b]):
            assert c1 <= c0 * (1 + 1e-12), costs[:, b]
        assert costs[-1, b] < costs[0, b]
        assert sum(a1) < sum(a0), (a0, a1)


@pytest.mark.gpu
def test_refusals_and_defaults(gpu):
    import ctypes as C
    capi = gpu
    T, B = 4, 2
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    L = capi.lib()
    dp = C.POINTER(C.c_double)

    def code(fn):
        with pytest.raises(capi.DdpHipError) as exc:
            fn()
        return exc.value.code
    with pytest.raises(capi.DdpHipError) as exc:                      # flag 64 without flag 16
        capi.Context(spec, flags=capi.FLAG_FRAME_ORIENT_COST)
    assert exc.value.code == capi.E_ARG
    frames = fc.pick_frames(model, 3)
    with capi.Context(spec, flags=capi.FLAG_FRAME_COST) as ctx:       # a context without the flag
        ctx.set_frame_cost(frames=frames)
        assert code(lambda: ctx.set_frame_orient_cost(weight=1.0)) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.frame_orient_cost()) == capi.E_UNSUPPORTED
    with capi.Context(spec, flags=_flags(capi)) as ctx:
        # before frames are set: nothing to download, uploads refused
        q0, w0 = ctx.frame_orient_cost()
        assert q0.shape == (B, T + 1, 0, 4) and w0.shape == (B, T + 1, 0, 3)
        z = np.zeros(B * (T + 1) * 4); z[3::4] = 1.0
        assert L.ddp_hip_frame_orient_upload(ctx._h, z.ctypes.data_as(dp), None, 0, B) == capi.E_ARG
        assert code(lambda: ctx.set_frame_orient_cost(weight=1.0)) == capi.E_ARG
        ctx.set_frame_cost(frames=frames)
        ident = identity_quat((B, T + 1, 3))
        q0, w0 = ctx.frame_orient_cost()                                # create: identity quaternions, weights 0
        assert np.array_equal(q0, ident) and np.all(w0 == 0.0)
        rng = np.random.default_rng(5)
        qg = rng.normal(size=(B, T + 1, 3, 4)); qg /= np.linalg.norm(qg, axis=-1, keepdims=True)
        wg = rng.uniform(0, 1, size=(B, T + 1, 3, 3))
        for bad in (-1e-3, np.nan, np.inf):
            wb = np.ones((T + 1, 3, 3)); wb[1, 2, 0] = bad
            assert code(lambda: ctx.set_frame_orient_cost(quat=qg, weight=wb)) == capi.E_ARG, bad
        # the library's own check of the quaternions (the Python layer refuses them first: straight through the C entry point)
        for bad in (np.nan, np.inf, 1.0 + 1e-6):
            qb = qg.copy()
            if np.isfinite(bad):
                qb[1, 2, 1] *= bad
            else:
                qb[1, 2, 1, 3] = bad
            assert L.ddp_hip_frame_orient_upload(ctx._h, qb.ctypes.data_as(dp), wg.ctypes.data_as(dp), 0, B) == capi.E_ARG, bad
        assert L.ddp_hip_frame_orient_upload(ctx._h, qg.ctypes.data_as(dp), wg.ctypes.data_as(dp), 1, B) == capi.E_ARG   # bad range
        assert L.ddp_hip_frame_orient_upload(ctx._h, qg.ctypes.data_as(dp), wg.ctypes.data_as(dp), -1, 1) == capi.E_ARG
        q1, w1 = ctx.frame_orient_cost()
        assert np.array_equal(q1, ident) and np.all(w1 == 0.0)          # a refused upload leaves both sides as they were
        ctx.set_frame_orient_cost(quat=qg, weight=wg)
        q1, w1 = ctx.frame_orient_cost()
        assert np.array_equal(q1, qg) and np.array_equal(w1, wg)
        ctx.set_frame_orient_cost(quat=-qg[1], first=1, count=1)        # one side, one instance; the weights stay
        q1, w1 = ctx.frame_orient_cost()
        assert np.array_equal(q1[0], qg[0]) and np.array_equal(q1[1], -qg[1]) and np.array_equal(w1, wg)
        ctx.set_frame_orient_cost(weight=np.array([1.0, 2.0, 0.0]))     # broadcast
        assert np.array_equal(ctx.frame_orient_cost()[1], np.broadcast_to([1.0, 2.0, 0.0], (B, T + 1, 3, 3)))
        tg = rng.normal(size=(B, T + 1, 3, 3))
        ctx.set_frame_cost(frames=frames[::-1], target=tg, weight=0.5)  # the same count: the orientation data stays
        q2, w2 = ctx.frame_orient_cost()
        assert np.array_equal(q2, q1) and np.array_equal(w2, np.broadcast_to([1.0, 2.0, 0.0], (B, T + 1, 3, 3)))
        ctx.set_frame_cost(frames=frames[:2])                           # another count: the defaults return
        q3, w3 = ctx.frame_orient_cost()
        assert q3.shape == (B, T + 1, 2, 4) and np.array_equal(q3, identity_quat((B, T + 1, 2))) and np.all(w3 == 0.0)
        assert code(lambda: ctx.frame_orient_cost(first=1, count=B)) == capi.E_ARG
