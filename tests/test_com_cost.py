"""Per-instance centre-of-mass costs (DDP_HIP_FLAG_COM_COST, include/ddp_hip/ddp_hip.h):

    l(t, x, u) += 1/2 sum_a w[b][t][a] r_a^2,   lf(x_T) += 1/2 sum_a w[b][T][a] r_a^2,   r = c(q_t) - g[b][t]

with c(q) = sum_j m_j p_j(q) / M, p_j the world position of body j's centre of mass.  The oracle has no such cost, so the
yardstick is the numpy restatement below, built on Oracle.frame_position and Oracle.frame_jacobian(world_aligned=True) with
m and c from model.mass_j / model.com: c = sum m_j frame_position(j, com_j, q) / M, Jc = sum m_j frame_jacobian(j, com_j, q) / M.
The helpers of test_tracking_cost.py, test_frame_cost.py and test_state_limits.py are reused by import; tolerances are theirs."""
import os
import re

import numpy as np
import pytest

import test_frame_cost as fc
import test_state_limits as sl
import test_tracking_cost as tc
from problems import make
from synth import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 1e-3
DERIVS = fc.DERIVS


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def com(o, model, q):
    m = np.asarray(model.mass_j)
    return sum(m[j] * o.frame_position(j, model.com[j], q) for j in range(len(m))) / m.sum()


def com_jac(o, model, q):
    m = np.asarray(model.mass_j)
    return sum(m[j] * o.frame_jacobian(j, model.com[j], q, world_aligned=True) for j in range(len(m))) / m.sum()


def com_terms(o, model, xs, tgt, w):
    """the CoM terms of one instance per t (T+1 values; the last belongs to lf); tgt, w: (T+1, 3)"""
    X = xs.reshape(o.T + 1, o.nx)
    out = np.zeros(o.T + 1)
    for t in range(o.T + 1):
        r = com(o, model, X[t][:o.nq]) - tgt[t]
        out[t] = 0.5 * np.sum(w[t] * r * r)
    return out


def com_grad_hess(o, model, x, tgt_t, w_t):
    """(lx, lxx) contributions at one state, n and n x n: Jc^T (w o r) and the Gauss-Newton Jc^T diag(w) Jc on the q rows"""
    nv, n = o.nv, o.n
    g, Hm = np.zeros(n), np.zeros((n, n))
    q = x[:o.nq]
    r = com(o, model, q) - tgt_t
    J = com_jac(o, model, q)
    g[:nv] = J.T @ (w_t * r)
    for a in range(3):                                   # entry (i, j) and (j, i) alike: symmetric bit for bit
        Hm[:nv, :nv] += w_t[a] * np.outer(J[a], J[a])
    return g, Hm


def com_derivs(o, model, xs, tgt, w):
    """what the CoM terms add to LX, LXX, LFX, LFXX of one instance, in the library's flat (column-major) layout"""
    X = xs.reshape(o.T + 1, o.nx)
    out = {"LX": [], "LXX": []}
    for t in range(o.T + 1):
        g, Hm = com_grad_hess(o, model, X[t], tgt[t], w[t])
        if t == o.T:
            out["LFX"], out["LFXX"] = g, Hm.ravel(order="F")
        else:
            out["LX"].append(g); out["LXX"].append(Hm.ravel(order="F"))
    out["LX"], out["LXX"] = np.concatenate(out["LX"]), np.concatenate(out["LXX"])
    return out


def random_task(o, model, xs, B, seed, wscale=1.0, spread=0.1):
    """per-instance targets near the CoM along the trajectories (xs: (B, ...)) and positive weights, each (B, T+1, 3)"""
    rng = np.random.default_rng(seed)
    T = o.T
    tgt = np.zeros((B, T + 1, 3))
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            tgt[b, t] = com(o, model, X[t][:o.nq]) + spread * rng.normal(size=3)
    return tgt, wscale * rng.uniform(0.1, 2.0, size=(B, T + 1, 3))


def table_model():
    """a small tree given as arrays: a branch at joint 1, which is prismatic and no leaf; a second prismatic joint at a leaf"""
    from ddp_pinocchio_amd import capi
    rng = np.random.default_rng(77)
    parents = [-1, 0, 1, 1, 3, 0, 5]
    R, P = capi.JOINT_REVOLUTE, capi.JOINT_PRISMATIC
    jtype = [R, P, R, R, P, R, R]
    nv = len(parents)
    axis = rng.normal(size=(nv, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    Rp = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(nv)])
    for k in range(nv):
        if np.linalg.det(Rp[k]) < 0:
            Rp[k][:, 0] = -Rp[k][:, 0]
    pp = rng.uniform(0.05, 0.3, size=(nv, 3)) * rng.choice([-1.0, 1.0], size=(nv, 3))
    mass = rng.uniform(0.5, 5.0, size=nv)
    cm = rng.uniform(-0.05, 0.05, size=(nv, 3))
    Ic = np.stack([np.diag(mass[k] * rng.uniform(0.01, 0.05, size=3)) for k in range(nv)])
    return capi.TableModel(parents, jtype, axis, Rp, pp, mass, cm, Ic)


def make_any(name, T, batch=1, fd_mode=2, first_order_fd=None):
    """problems.make, or the prismatic TableModel ("table7") as an unconstrained problem"""
    if name != "table7":
        return make(name, T, batch=batch, fd_mode=fd_mode, first_order_fd=first_order_fd)
    from ddp_pinocchio_amd import capi
    from oracle.binding import Oracle
    model = table_model()
    kw = dict(dt=0.01, c=1.0, fd_mode=fd_mode, first_order_fd=1, eq_kind=capi.EQ_NONE, ne=np.zeros(T, dtype=np.int64))
    return model, capi.ProblemSpec(model, T, batch=batch, **kw), Oracle(model, T, **kw)


_trajs, _setup = tc._trajs, tc._setup


# ---- CPU: the yardstick checks itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain6", "tree38", "chain6ff", "tree38ff"])
def test_yardstick_gradient(name):
    """lx against the 5-point central difference of the numpy cost along x (+) (+-h e_j); with the target at c(q) (r = 0, where
    Gauss-Newton is exact) lxx against the central difference of the gradient; lxx symmetric bit for bit with zero velocity
    rows and columns"""
    T = 2
    model, _, o = make(name, T, fd_mode=0)
    xs, us = _trajs(o, model, 1, 3)
    tgt, w = random_task(o, model, xs, 1, 4)
    X = xs[0].reshape(T + 1, o.nx)
    nv, n = o.nv, o.n
    w5 = ((-2, 1.0 / 12), (-1, -8.0 / 12), (1, 8.0 / 12), (2, -1.0 / 12))
    for t in (1, T):
        g, Hm = com_grad_hess(o, model, X[t], tgt[0][t], w[0][t])
        assert np.max(np.abs(g[:nv])) > 0

        def cost_at(dx):
            X2 = X.copy()
            X2[t] = tc._integrate_x(o, X[t], dx)
            return com_terms(o, model, X2.ravel(), tgt[0], w[0])[t]
        fd = np.zeros(n)
        for j in range(n):
            e = np.zeros(n); e[j] = H
            fd[j] = sum(cw * cost_at(s * e) for s, cw in w5) / H
        assert np.max(np.abs(fd - g)) <= 1e-8 * max(1.0, np.max(np.abs(g))), np.max(np.abs(fd - g))
        tgt0 = com(o, model, X[t][:o.nq])
        _, H0 = com_grad_hess(o, model, X[t], tgt0, w[0][t])

        def grad_at(dx):
            return com_grad_hess(o, model, tc._integrate_x(o, X[t], dx), tgt0, w[0][t])[0]
        fdh = np.zeros((n, n))
        for j in range(n):
            e = np.zeros(n); e[j] = H
            fdh[:, j] = sum(cw * grad_at(s * e) for s, cw in w5) / H
        assert np.max(np.abs(fdh - H0)) <= 1e-8 * max(1.0, np.max(np.abs(H0))), np.max(np.abs(fdh - H0))
        assert np.array_equal(Hm, Hm.T)
        assert np.all(Hm[nv:, :] == 0.0) and np.all(Hm[:, nv:] == 0.0) and np.all(g[nv:] == 0.0)


def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.FLAG_COM_COST == 128 and re.search(r"#define\s+DDP_HIP_FLAG_COM_COST\s+128u", header)
    L = capi.lib()
    for name in ("ddp_hip_com_cost_upload", "ddp_hip_com_cost_download", "ddp_hip_model_com"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    assert len(capi.SEQ_NAMES) == 40
    assert hasattr(capi.Context, "set_com_cost") and hasattr(capi.Context, "com_cost") and hasattr(capi.ModelHandle, "com")
    # shapes are checked before anything reaches the library: a context object without a device will do
    T, B = 5, 2
    model, spec, _ = make("chain6", T, batch=B, fd_mode=0)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx._h = spec, B, None
    for kw in (dict(target=np.zeros((T, 3))), dict(target=np.zeros(3)), dict(target=0.0), dict(target=np.zeros((B + 1, T + 1, 3))),
               dict(weight=np.zeros((T + 1, 2))), dict(weight=np.zeros(2)), dict(weight=np.zeros((B, T + 1, 3)), count=1),
               dict(target=np.zeros((T + 1, 3)), weight=np.zeros((T, 3)))):
        with pytest.raises(ValueError):
            ctx.set_com_cost(**kw)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain6", "tree38", "chain6ff", "tree38ff", "table7"])
def test_model_com(gpu, name):
    """ddp_hip_model_com: the traversal on the device in isolation, c and Jc against the yardstick to 1e-12"""
    capi = gpu
    model, _, o = make_any(name, 2, fd_mode=0)
    rng = np.random.default_rng(5)
    with capi.ModelHandle(model) as h:
        for k in range(3):
            q = rng.normal(size=o.nq)
            if o.nq != o.nv:
                q[3:7] /= np.linalg.norm(q[3:7])
            c, J = h.com(q, jacobian=True)
            c_only = h.com(q)
            ec, eJ = rel_err(c, com(o, model, q)), rel_err(J, com_jac(o, model, q))
            print("model_com", name, k, ec, eJ)
            assert np.array_equal(c, c_only)
            assert ec <= 1e-12 and eJ <= 1e-12, (ec, eJ)


LIN_CASES = [("chain6", 2, None, ""), ("tree38", 2, None, ""), ("chain6ff", 2, 0, ""), ("tree38ff", 0, 0, "nt"),
             ("tree38", 2, None, "all"), ("table7", 2, None, "")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo,flags", LIN_CASES)
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, name, fd_mode, fo, flags, stages):
    """LX, LXX, LFX, LFXX against the flag-off values plus the definition's terms, batch 3 with different targets and weights
    per instance, through ddp_hip_linearize and ddp_hip_linearize_stages(LIN_COST); LXX / LFXX symmetric bit for bit; LU, LUU,
    LUX and every velocity row and column bit for bit the flag-off values.  "all": tracking, frame cost and state limits live"""
    capi = gpu
    T, B = 6, 3
    model, spec, o = make_any(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    xs, us = _trajs(o, model, B, 41)
    tgt, w = random_task(o, model, xs, B, 42)
    w[1, 2, 1] = 0.0; w[0, T, 2] = 0.0                # single zero weights among the others
    w[2, :, 0] = 0.0                                  # one axis off at every t for one instance
    w[1, 4, :] = 0.0                                  # one (instance, t) with all three off
    ref = tc.random_ref(o, model, xs, us, B, 44)
    frames = fc.pick_frames(model, 3)
    ftask = fc.random_task(o, xs, frames, B, 45)
    lim = sl.random_limits(o, xs, B, 46)
    base = capi.FLAG_NO_TENSORS if flags == "nt" else 0
    if flags == "all":
        base |= capi.FLAG_TRACKING_COST | capi.FLAG_FRAME_COST | capi.FLAG_STATE_LIMITS
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (capi.FLAG_COM_COST if on else 0)) as ctx:
            _setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
            if flags == "all":
                tc.upload_ref(ctx, ref)
                ctx.set_frame_cost(frames=frames, target=ftask[0], weight=ftask[1])
                ctx.set_state_limits(lo=lim[0], hi=lim[1], weight=lim[2])
            if on:
                ctx.set_com_cost(target=tgt, weight=w)
            ctx.linearize(None if stages is None else capi.LIN_COST)
            got[on] = {s: ctx.download(s) for s in DERIVS}
    n, nv = o.n, o.nv
    worst = 0.0
    for b in range(B):
        add = com_derivs(o, model, xs[b], tgt[b], w[b])
        for s in ("LX", "LXX", "LFX", "LFXX"):
            ex = got[False][s][b] + add[s]
            assert np.max(np.abs(add[s])) > 0
            worst = max(worst, rel_err(got[True][s][b], ex))
            assert rel_err(got[True][s][b], ex) <= 1e-12, (s, b, rel_err(got[True][s][b], ex))
        for s in ("LU", "LUU", "LUX"):
            assert np.array_equal(got[True][s][b], got[False][s][b]), s
        for t in range(T + 1):
            key, k = ("LXX", t) if t < T else ("LFXX", 0)
            blk = got[True][key][b][k * n * n:(k + 1) * n * n].reshape(n, n)
            off = got[False][key][b][k * n * n:(k + 1) * n * n].reshape(n, n)
            assert np.array_equal(blk, blk.T)
            assert np.array_equal(blk[nv:, :], off[nv:, :]) and np.array_equal(blk[:, nv:], off[:, nv:])
            gk, go = ("LX", t) if t < T else ("LFX", 0)
            assert np.array_equal(got[True][gk][b][go * n + nv:(go + 1) * n], got[False][gk][b][go * n + nv:(go + 1) * n])
        # the (instance, t) whose three weights are 0 is untouched
        if b == 1:
            assert np.array_equal(got[True]["LXX"][b][4 * n * n:5 * n * n], got[False]["LXX"][b][4 * n * n:5 * n * n])
    print("linearize", name, flags, stages, "worst", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo", [("tree38", 0, None), ("chain6ff", 0, 0), ("chain6", 2, None), ("tree38_frame", 0, None)])
def test_cost_seq_aug(gpu, name, fd_mode, fo):
    """COSTS_OLD / COSTS_NEW (which = 0 / 1) against the oracle's augmented cost plus the numpy CoM terms, lf included"""
    capi = gpu
    T, B, mu = 12, 2, 30.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    xs, us = _trajs(o, model, B, 51)
    xs2, us2 = _trajs(o, model, B, 61)
    tgt, w = random_task(o, model, xs, B, 52)
    w[1, 3, :] = 0.0
    mults = tc._mults(o, xs[0], 53)
    with capi.Context(spec, flags=capi.FLAG_COM_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
        ctx.set_com_cost(target=tgt, weight=w)
        ctx.cost_seq_aug(0, mu)
        ctx.cost_seq_aug(1, mu)
        got = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
    for which, (X, U) in ((0, (xs, us)), (1, (xs2, us2))):
        for b in range(B):
            ex = o.cost_seq_aug(X[b], U[b], mults, mu) + com_terms(o, model, X[b], tgt[b], w[b])
            assert got[which][b][T] != 0.0
            assert rel_err(got[which][b], ex) <= 1e-12, (which, b, rel_err(got[which][b], ex))


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,fd_mode,fo,extra,fwd_path", [
    ("tree38", 24, 2, None, "", 1),                 # latency forward
    ("chain6ff", 10, 2, 0, "", 0),                  # lane-per-rollout forward
    ("tree38_frame", 24, 0, None, "", 1),           # constrained: the candidates' costs from cand_cost_kernel
    ("tree38", 24, 2, None, "box", 1),
])
@pytest.mark.parametrize("mode", ["nothing", "zero_weights", "zero_instance"])
def test_zero_weights_change_nothing(gpu, name, T, fd_mode, fo, extra, fwd_path, mode):
    """flag on with nothing uploaded, or targets far away but every weight 0: bit for bit what the flag-off context computes.
    zero_instance: batch 2, instance 1 carries non-zero weights (the CoM kernels run), instance 0 none: instance 0 is bit for
    bit the flag-off context's instance 0"""
    capi = gpu
    mu = 10.0
    B = 2 if mode == "zero_instance" else 1
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    xs, us = _trajs(o, model, B, 31, held=True)
    mults = tc._mults(o, xs[0], 32)
    tgt, w = random_task(o, model, xs, B, 33, spread=1.0)
    if mode == "zero_instance":
        w[0] = 0.0
        w *= 0.05
    else:
        w[:] = 0.0
    base = capi.FLAG_TRACE | (capi.FLAG_CONTROL_BOUNDS if extra == "box" else 0)
    out = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (capi.FLAG_COM_COST if on else 0)) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            _setup(ctx, xs, us, mults, o.Etot)
            if extra == "box":
                ctx.set_control_bounds(lo=-1e6, hi=1e6)
            if on and mode != "nothing":
                ctx.set_com_cost(target=tgt, weight=w)
            out[on] = fc._run_all(ctx, mu, name == "tree38")
    a, b = out[False], out[True]
    if mode == "zero_instance":
        assert not np.array_equal(a["LX"][1], b["LX"][1])            # the CoM terms are there for instance 1
        assert not np.array_equal(a["COSTS_OLD"][1], b["COSTS_OLD"][1])
        a = {k: (tuple(np.asarray(v)[..., :1] for v in a[k][1:]) if isinstance(a[k], tuple) else (a[k][:1] if k != "stream" else a[k])) for k in a}
        b = {k: (tuple(np.asarray(v)[..., :1] for v in b[k][1:]) if isinstance(b[k], tuple) else (b[k][:1] if k != "stream" else b[k])) for k in b}
    fc._same(a, b)
    assert np.all(np.isfinite(b["LX"])) and np.all(np.isfinite(b["X_NEW"]))


def _emulate_forward(o, xs, us, mults, fb, mu, n_alpha, cost, lo=None, hi=None):
    """sequential halving with the full numpy cost, the CoM terms included: the first step 2^-k with sum_t (new - old) <= 0
    (n_alpha = 0: the full step).  Returns the step, the rollout, sum(new - old) and, of every candidate tried, |sum(new - old)|
    over sum |cost terms|: how far each decision is from the rounding of another order of additions"""
    old = cost(xs, us)
    margins = []
    for k in range(34):
        step = 2.0 ** -k
        if lo is None:
            _, xn, un = o.forward_alpha(step, xs, us, mults, fb, mu)
        else:
            xn, un = fc._rollout(o, step, xs, us, fb, mu, lo, hi)
        new = cost(xn, un)
        diff = new.sum() - old.sum()
        margins.append(abs(diff) / (np.sum(np.abs(new)) + np.sum(np.abs(old))))
        if n_alpha == 0 or diff <= 0:
            return step, xn, un, diff, margins
    return None


FORWARD_CASES = [(name, fo, path, extra, na, ks)
                 for name, fo, path, extra in (("tree38", None, 1, ""), ("chain6ff", 0, 0, ""), ("tree38_frame", None, 1, ""),
                                               ("tree38", None, 1, "box"))
                 for na in (0, 1, 8) for ks in (1.0, 3.0)]


def _forward_inputs(name, fo):
    T = 16
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo)
    xs, us = _trajs(o, model, 1, 81, held=True)
    tgt, w = random_task(o, model, xs, 1, 82, wscale=2000.0, spread=0.02)
    mults = tc._mults(o, xs[0], 85)
    return T, model, spec, o, xs, us, tgt, w, mults


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo,fwd_path,extra,n_alpha,k_scale", FORWARD_CASES)
def test_forward_matches_emulation(gpu, name, fo, fwd_path, extra, n_alpha, k_scale):
    """accepted step, X_NEW, U_NEW and dcost against Oracle.forward_alpha rollouts costed with numpy, the CoM terms included;
    k_scale 3 overshoots so that the halving runs; box: control bounds that bind on every third control (the emulation clamps).
    The device adds the CoM sum in another association than the emulation: the test first asserts, on the emulation alone, that
    every candidate tried decides by more than 1e-9 of the sum of the cost terms' magnitudes, and only then compares decisions"""
    capi = gpu
    mu = 1.0
    T, model, spec, o, xs, us, tgt, w, mults = _forward_inputs(name, fo)
    blo = bhi = None
    flags = capi.FLAG_COM_COST | capi.FLAG_NO_TENSORS | (capi.FLAG_CONTROL_BOUNDS if extra == "box" else 0)
    with capi.Context(spec, flags=flags) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.set_com_cost(target=tgt, weight=w)
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
        return o.cost_seq_aug(X, U, mults, mu_o[0]) + com_terms(o, model, X, tgt[0], w[0])
    em = _emulate_forward(o, xs[0], us[0], mults, fb, mu_o[0], n_alpha, cost, blo, bhi)
    assert em is not None
    step_ref, xn_ref, un_ref, new, margins = em
    print("forward", name, extra, n_alpha, k_scale, "step", step[0], step_ref, "dcost", dcost[0], new, "margins", margins)
    assert min(margins) > 1e-9, margins               # a condition on the inputs: the decisions do not hang on rounding
    assert step[0] == step_ref, (step, step_ref)
    if extra == "box":
        Un = un.reshape(T, o.m)
        assert np.any(Un == blo) or np.any(Un == bhi)
    assert rel_err(xn, xn_ref) < 1e-9 and rel_err(un, un_ref) < 1e-9
    assert abs(dcost[0] - new) <= 1e-9 * max(1.0, abs(new)), (dcost[0], new)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo,flags", [("chain6ff", 2, 0, 0), ("tree38", 0, 0, 1)])
def test_instances_are_independent(gpu, name, fd_mode, fo, flags):
    """batch 3 through linearise, both costs, sweep, forward: instance 1 computed alone equals its values in the batch bit for bit"""
    capi = gpu
    T, B, mu = 12, 3, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    _, spec1, _ = make(name, T, batch=1, fd_mode=fd_mode, first_order_fd=fo)
    xs, us = _trajs(o, model, B, 91, held=True)
    tgt, w = random_task(o, model, xs, B, 92, wscale=10.0, spread=0.05)
    out = []
    for sp, s_ in ((spec, slice(0, B)), (spec1, slice(1, 2))):
        with capi.Context(sp, flags=capi.FLAG_COM_COST | capi.FLAG_TRACE | flags) as ctx:
            _setup(ctx, xs[s_], us[s_])
            ctx.set_com_cost(target=tgt[s_], weight=w[s_])
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
    tgt, w = random_task(o, model, xs, B, 102, wscale=10.0)
    mults = tc._mults(o, xs[0], 103)

    def run(stepwise):
        with capi.Context(spec, flags=capi.FLAG_COM_COST | flags) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if o.Etot:
                ctx.upload("MULT_ORIGIN", xs[:, :T * o.nx])
            ctx.set_com_cost(target=tgt, weight=w)
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
def test_com_shift_descends(gpu):
    """tree38, T = 20, held trajectory; the target is the initial CoM moved 5 cm sideways at every t, the terminal weight 10 x
    larger: over ten iterations the total cost never increases over accepted steps and the CoM ends closer to the target"""
    capi = gpu
    T, mu, iters = 20, 1.0, 10
    model, spec, o = make("tree38", T, fd_mode=0)
    xs, us = _trajs(o, model, 1, 111, held=True)
    with capi.ModelHandle(model) as h:
        c0 = h.com(xs[0][:o.nq])
    goal = c0 + np.array([0.0, 0.05, 0.0])
    tgt = np.tile(goal, (T + 1, 1))
    # the held posture costs c/2 |u|^2 of some 4e5 per step in gravity torques: weights below 1e7 leave the CoM term a rounding
    # error beside it, and the cheapest trajectory is to let go and fall
    w = np.full((T + 1, 3), 1e8)
    w[T] = 1e9

    def err(X):
        return np.linalg.norm(com(o, model, X.reshape(T + 1, o.nx)[T][:o.nq]) - goal)
    with capi.Context(spec, flags=capi.FLAG_COM_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        ctx.set_com_cost(target=tgt, weight=w)
        costs, steps = [], []
        for _ in range(iters):
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            rc, step, dcost = ctx.forward(mu_o, n_alpha=8)
            costs.append(ctx.download("COSTS_OLD")[0].sum())
            steps.append(step[0])
            ctx.swap_traj()
        final = ctx.download("X")[0]
    print("com shift costs", costs, "steps", steps, "error", err(xs[0]), "->", err(final))
    for a, b in zip(costs, costs[1:]):
        assert b <= a * (1 + 1e-12), costs
    assert costs[-1] < costs[0]
    assert err(final) < err(xs[0]), (err(xs[0]), err(final))


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
        assert code(lambda: ctx.set_com_cost(weight=1.0)) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.com_cost()) == capi.E_UNSUPPORTED
    pend = capi.BuiltinModel(capi.BUILTIN_PENDULUM)
    with pytest.raises(capi.DdpHipError) as exc:
        capi.Context(capi.ProblemSpec(pend, T, fd_mode=2), flags=capi.FLAG_COM_COST)
    assert exc.value.code == capi.E_UNSUPPORTED
    with capi.Context(spec, flags=capi.FLAG_COM_COST) as ctx:
        t0, w0 = ctx.com_cost()                                         # create: targets 0, weights 0
        assert t0.shape == (B, T + 1, 3) and np.all(t0 == 0.0) and np.all(w0 == 0.0)
        rng = np.random.default_rng(5)
        tg, wg = rng.normal(size=(B, T + 1, 3)), rng.uniform(0, 1, size=(B, T + 1, 3))
        ctx.set_com_cost(target=tg, weight=wg)
        for bad in (-1e-3, np.nan, np.inf):
            wb = np.ones((T + 1, 3)); wb[1, 2] = bad
            assert code(lambda: ctx.set_com_cost(weight=wb)) == capi.E_ARG, bad
            assert code(lambda: ctx.set_com_cost(target=np.zeros((T + 1, 3)), weight=wb)) == capi.E_ARG, bad
        for bad in (np.nan, -np.inf):
            tb = np.ones((T + 1, 3)); tb[2, 1] = bad
            assert code(lambda: ctx.set_com_cost(target=tb, weight=1.0)) == capi.E_ARG, bad
        assert code(lambda: ctx.set_com_cost(weight=0.0, first=B, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_com_cost(weight=0.0, first=-1, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_com_cost(weight=0.0, first=1, count=B)) == capi.E_ARG
        assert code(lambda: ctx.com_cost(first=1, count=B)) == capi.E_ARG
        z = np.zeros(B * (T + 1) * 3)
        assert L.ddp_hip_com_cost_upload(ctx._h, z.ctypes.data_as(dp), z.ctypes.data_as(dp), 0, B + 1) == capi.E_ARG
        t1, w1 = ctx.com_cost()
        assert np.array_equal(t1, tg) and np.array_equal(w1, wg)        # a refused upload leaves both sides as they were
        ctx.set_com_cost(target=tg[1] + 1.0, first=1, count=1)          # one side, one instance; the weights stay
        t1, w1 = ctx.com_cost()
        assert np.array_equal(t1[0], tg[0]) and np.array_equal(t1[1], tg[1] + 1.0) and np.array_equal(t1[2], tg[2]) and np.array_equal(w1, wg)
        t2, w2 = ctx.com_cost(first=1, count=2)                         # the round trip of a range of instances
        assert np.array_equal(t2, t1[1:]) and np.array_equal(w2, wg[1:])
        ctx.set_com_cost(weight=np.array([1.0, 2.0, 0.0]), first=1, count=2)    # broadcast: (3,) and scalar
        assert np.array_equal(ctx.com_cost()[1][1:], np.broadcast_to([1.0, 2.0, 0.0], (2, T + 1, 3)))
        assert np.array_equal(ctx.com_cost()[1][0], wg[0])
        ctx.set_com_cost(weight=0.5)
        assert np.all(ctx.com_cost()[1] == 0.5)
