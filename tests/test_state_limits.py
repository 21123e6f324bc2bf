"""Per-instance soft state limits (DDP_HIP_FLAG_STATE_LIMITS, include/ddp_hip/ddp_hip.h): per instance b, t = 0 .. T and
tangent row i (rows 0 .. nv-1 configuration, nv .. 2nv-1 velocity), with s_i the row's state coordinate,

    e_i = s_i < lo_i ? s_i - lo_i : (s_i > hi_i ? s_i - hi_i : 0)
    l(t, x, u) += 1/2 sum_i w[b][t][i] e_i^2,   lf(x_T) += 1/2 sum_i w[b][T][i] e_i^2
    lx[i] += w_i e_i,   lxx[i][i] += w_i      for the rows with w_i != 0 and e_i != 0 only

The oracle has no such cost, so the yardstick is the numpy restatement below, beside Oracle.forward_alpha, backward, integrate
and the helpers of test_tracking_cost.py / test_frame_cost.py.  Tolerances are those files' own."""
import os
import re

import numpy as np
import pytest

import test_frame_cost as fc
import test_tracking_cost as tc
from problems import make
from synth import rel_err, stepwise_backward_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 1e-3
DERIVS = fc.DERIVS
NAMES = fc.NAMES


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def coords(o, X):
    """s: the state coordinates of the n tangent rows; X (..., nx) -> (..., n).  Row i < nv: x[i + nq - nv], else x[nq + i - nv]"""
    return np.concatenate([X[..., o.nq - o.nv:o.nq], X[..., o.nq:]], axis=-1)


def excess(s, lo, hi):
    return np.where(s < lo, s - lo, np.where(s > hi, s - hi, 0.0))


def limit_terms(o, xs, lo, hi, w):
    """the limit terms of one instance per t (T+1 values; the last belongs to lf); lo, hi, w: (T+1, n).  A term with w = 0 or
    e = 0 is left out, not multiplied by 0"""
    e = excess(coords(o, xs.reshape(o.T + 1, o.nx)), lo, hi)
    on = (w != 0.0) & (e != 0.0)
    return 0.5 * np.sum(np.where(on, w * np.where(on, e, 0.0) ** 2, 0.0), axis=1)


def limit_grad_hess(o, x, lo_t, hi_t, w_t):
    """(lx, lxx) contributions at one state: w o e and diag(w) over the violated rows"""
    e = excess(coords(o, x), lo_t, hi_t)
    on = (w_t != 0.0) & (e != 0.0)
    return np.where(on, w_t * np.where(on, e, 0.0), 0.0), np.diag(np.where(on, w_t, 0.0))


def limit_derivs(o, xs, lo, hi, w):
    """what the limit terms add to LX, LXX, LFX, LFXX of one instance, in the library's flat (column-major) layout"""
    X = xs.reshape(o.T + 1, o.nx)
    out = {"LX": [], "LXX": []}
    for t in range(o.T + 1):
        g, Hm = limit_grad_hess(o, X[t], lo[t], hi[t], w[t])
        if t == o.T:
            out["LFX"], out["LFXX"] = g, Hm.ravel(order="F")
        else:
            out["LX"].append(g); out["LXX"].append(Hm.ravel(order="F"))
    out["LX"], out["LXX"] = np.concatenate(out["LX"]), np.concatenate(out["LXX"])
    return out


def random_limits(o, xs, B, seed, wscale=1.0):
    """per (b, t, i): a third of the rows violated below (lo = s + U(0.05, 0.3), hi = lo + U(0.1, 1)), a third above, the rest
    with the state strictly inside (by U(0.05, 0.5) on either side); one row in ten one-sided (+-inf on a side that is not
    violated); weights U(0.1, 2), 0 on a free-flyer root's rows 0 .. 5.  Asserts that all three cases occur among the q rows
    and among the v rows that carry a weight"""
    rng = np.random.default_rng(seed)
    T, n, nv = o.T, o.n, o.nv
    S = coords(o, np.asarray(xs).reshape(B, T + 1, o.nx))
    N = B * (T + 1)
    cat = np.stack([rng.permutation(np.arange(N) % 3) for _ in range(n)], axis=1).reshape(B, T + 1, n)   # 0 below, 1 above, 2 inside
    gap, width = rng.uniform(0.05, 0.3, size=S.shape), rng.uniform(0.1, 1.0, size=S.shape)
    in_lo, in_hi = rng.uniform(0.05, 0.5, size=S.shape), rng.uniform(0.05, 0.5, size=S.shape)
    lo = np.where(cat == 0, S + gap, np.where(cat == 1, S - gap - width, S - in_lo))
    hi = np.where(cat == 0, S + gap + width, np.where(cat == 1, S - gap, S + in_hi))
    one = rng.uniform(size=S.shape) < 0.1
    side = rng.uniform(size=S.shape) < 0.5
    hi = np.where(one & ((cat == 0) | ((cat == 2) & side)), np.inf, hi)
    lo = np.where(one & ((cat == 1) | ((cat == 2) & ~side)), -np.inf, lo)
    w = wscale * rng.uniform(0.1, 2.0, size=S.shape)
    r0 = 6 if o.nq != nv else 0
    w[..., :r0] = 0.0
    e = excess(S, lo, hi)
    for rows in (slice(r0, nv), slice(nv, n)):
        if rows.stop > rows.start:
            assert np.any(e[..., rows] < 0) and np.any(e[..., rows] > 0) and np.any(e[..., rows] == 0)
    assert np.all(lo <= hi) and (S.size < 100 or (np.any(np.isinf(lo)) and np.any(np.isinf(hi))))
    assert np.all((np.abs(e) > 10 * H) | ((S - lo > 10 * H) & (hi - S > 10 * H)))    # no kink within a stencil of step H
    return lo, hi, w


def _trajs(o, model, B, seed, held=False):
    return tc._trajs(o, model, B, seed, held=held and o.nv > 1)     # (the pendulum has no computed-torque hold)


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.FLAG_STATE_LIMITS == 32 and re.search(r"#define\s+DDP_HIP_FLAG_STATE_LIMITS\s+32u", header)
    L = capi.lib()
    for name in ("ddp_hip_state_limits_upload", "ddp_hip_state_limits_download"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    assert len(capi.SEQ_NAMES) == 40
    assert re.search(r"DDP_HIP_SEQ_BOX_STAT,[^\n]*\n\s*DDP_HIP_SEQ_COUNT", header)        # no ddp_hip_seq entries added
    # shapes and lo > hi are checked before anything reaches the library: a context object without a device will do
    T, B = 5, 2
    model, spec, _ = make("chain6", T, batch=B, fd_mode=0)
    n = spec.n
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx.n_cost_frames, ctx._h = spec, B, 0, None
    for kw in (dict(lo=np.zeros((T, n))), dict(hi=np.zeros(n + 1)), dict(weight=np.zeros((T + 1, n - 1))),
               dict(weight=np.zeros((B + 1, T + 1, n))), dict(lo=np.zeros((B, T + 1, n)), count=1), dict(hi=np.zeros((1, 1, 1, n))),
               dict(weight=np.zeros((B, T, n))), dict(lo=1.0, hi=0.0), dict(lo=np.full(n, 0.5), hi=np.zeros((T + 1, n))),
               dict(lo=np.zeros((B, T + 1, n)), hi=np.concatenate([np.ones((B, T + 1, n - 1)), -np.ones((B, T + 1, 1))], axis=2))):
        with pytest.raises(ValueError):
            ctx.set_state_limits(**kw)


@pytest.mark.parametrize("name", ["chain6", "tree38", "chain6ff", "tree38ff"])
def test_yardstick_gradient(name):
    """lx against the 5-point central difference of the numpy cost along x (+) (+-h e_j), lxx against the central difference
    of the gradient (random_limits keeps every kink more than 10 h away), to 1e-8 relative; lxx diagonal, zero root rows"""
    T = 2
    model, _, o = make(name, T, fd_mode=0)
    xs, us = _trajs(o, model, 1, 3)
    lo, hi, w = random_limits(o, xs, 1, 4)
    X = xs[0].reshape(T + 1, o.nx)
    n = o.n
    w5 = ((-2, 1.0 / 12), (-1, -8.0 / 12), (1, 8.0 / 12), (2, -1.0 / 12))
    for t in (1, T):
        g, Hm = limit_grad_hess(o, X[t], lo[0][t], hi[0][t], w[0][t])
        assert np.max(np.abs(g)) > 0

        def cost_at(dx):
            X2 = X.copy()
            X2[t] = tc._integrate_x(o, X[t], dx)
            return limit_terms(o, X2.ravel(), lo[0], hi[0], w[0])[t]

        def grad_at(dx):
            return limit_grad_hess(o, tc._integrate_x(o, X[t], dx), lo[0][t], hi[0][t], w[0][t])[0]
        fd, fdh = np.zeros(n), np.zeros((n, n))
        for j in range(n):
            e = np.zeros(n); e[j] = H
            fd[j] = sum(cw * cost_at(s * e) for s, cw in w5) / H
            fdh[:, j] = sum(cw * grad_at(s * e) for s, cw in w5) / H
        assert np.max(np.abs(fd - g)) <= 1e-8 * max(1.0, np.max(np.abs(g))), np.max(np.abs(fd - g))
        assert np.max(np.abs(fdh - Hm)) <= 1e-8 * max(1.0, np.max(np.abs(Hm))), np.max(np.abs(fdh - Hm))
        assert np.array_equal(Hm, np.diag(np.diag(Hm))) and np.all(np.diag(Hm) >= 0) and np.any(np.diag(Hm) > 0)
        if o.nq != o.nv:
            assert np.all(g[:6] == 0.0) and np.all(Hm[:6, :6] == 0.0)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _first(r):
    """instance 0 of what fc._run_all returns (the sweep's and the forward's return codes belong to the whole batch)"""
    return {k: (tuple(np.asarray(v)[..., :1] for v in r[k][1:]) if isinstance(r[k], tuple) else (r[k][:1] if k != "stream" else r[k]))
            for k in r}


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,fd_mode,fo,extra,fwd_path", [
    ("tree38", 24, 2, None, "", 1),                 # latency forward
    ("chain6ff", 10, 2, 0, "", 0),                  # lane-per-rollout forward
    ("tree38_frame", 24, 0, None, "", 1),           # constrained: the candidates' costs from cand_cost_kernel
    ("pendulum", 5, 2, None, "", None),
    ("tree38", 24, 2, None, "track", 1),
    ("tree38", 24, 2, None, "box", 1),
    ("tree38", 24, 2, None, "frame", 1),
])
@pytest.mark.parametrize("mode", ["nothing_uploaded", "zero_weights", "wide", "quiet_instance"])
def test_limits_that_do_not_bind_change_nothing(gpu, name, T, fd_mode, fo, extra, fwd_path, mode):
    """flag on with nothing uploaded, with tight bounds under zero weights, or with non-zero weights under bounds of +-1e6 (the
    limit kernels run): bit for bit what the flag-off context computes, derivatives, both cost sequences, gains, V_x trace,
    accepted step, X_NEW / U_NEW.  quiet_instance: batch 2, instance 1 binds, instance 0 has zero weights and is bit for bit the
    flag-off context's instance 0"""
    capi = gpu
    mu = 10.0
    B = 2 if mode == "quiet_instance" else 1
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    xs, us = _trajs(o, model, B, 31, held=True)
    mults = tc._mults(o, xs[0], 32)
    lo, hi, w = random_limits(o, xs, B, 33, wscale=0.05)
    if mode == "zero_weights":
        w[:] = 0.0
    elif mode == "wide":
        lo[:], hi[:] = -1e6, 1e6
    elif mode == "quiet_instance":
        w[0] = 0.0
    frames = fc.pick_frames(model, 3) if extra == "frame" else None
    if frames:
        tgt, wf = fc.random_task(o, xs, frames, B, 35, wscale=0.05, spread=0.1)
    ref = tc.random_ref(o, model, xs, us, B, 34, wscale=0.05, spread=0.05)
    base = capi.FLAG_TRACE | {"": 0, "track": capi.FLAG_TRACKING_COST, "box": capi.FLAG_CONTROL_BOUNDS, "frame": capi.FLAG_FRAME_COST}[extra]
    out = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (capi.FLAG_STATE_LIMITS if on else 0)) as ctx:
            if fwd_path is not None:
                assert ctx.info()["fwd_path"] == fwd_path
            tc._setup(ctx, xs, us, mults, o.Etot)
            if extra == "track":
                tc.upload_ref(ctx, ref)
            if extra == "box":
                ctx.set_control_bounds(lo=-1e6, hi=1e6)
            if frames:
                ctx.set_frame_cost(frames=frames, target=tgt, weight=wf)
            if on and mode != "nothing_uploaded":
                ctx.set_state_limits(lo=lo, hi=hi, weight=w)
            out[on] = fc._run_all(ctx, mu, name == "tree38")
    a, b = out[False], out[True]
    if mode == "quiet_instance":
        assert not np.array_equal(a["LX"][1], b["LX"][1])            # the limit terms are there for instance 1
        a, b = _first(a), _first(b)
    fc._same(a, b)
    assert np.all(np.isfinite(b["LX"])) and np.all(np.isfinite(b["X_NEW"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo,flags", [
    ("chain6", 2, None, ""), ("tree38", 2, None, ""), ("chain6ff", 2, 0, ""), ("tree38ff", 0, 0, "nt"), ("pendulum", 2, None, ""),
    ("tree38", 2, None, "track+frame")])
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, name, fd_mode, fo, flags, stages):
    """LX, LXX, LFX, LFXX against the flag-off values plus the definition's terms, batch 2 with different limits per instance,
    through ddp_hip_linearize and ddp_hip_linearize_stages(LIN_COST); LU, LUU, LUX bit for bit the flag-off values; LXX
    symmetric bit for bit"""
    capi = gpu
    T, B = 4, 2
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    xs, us = _trajs(o, model, B, 41)
    lo, hi, w = random_limits(o, xs, B, 42)
    w[1, 2, -1] = 0.0                                  # a single zero weight among the others
    both = flags == "track+frame"
    base = ((capi.FLAG_TRACKING_COST | capi.FLAG_FRAME_COST) if both else 0) | (capi.FLAG_NO_TENSORS if flags == "nt" else 0)
    if both:
        ref = tc.random_ref(o, model, xs, us, B, 44)
        frames = fc.pick_frames(model, 3)
        tgt, wf = fc.random_task(o, xs, frames, B, 45)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (capi.FLAG_STATE_LIMITS if on else 0)) as ctx:
            tc._setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
            if both:
                tc.upload_ref(ctx, ref)
                ctx.set_frame_cost(frames=frames, target=tgt, weight=wf)
            if on:
                ctx.set_state_limits(lo=lo, hi=hi, weight=w)
            ctx.linearize(None if stages is None else capi.LIN_COST)
            got[on] = {s: ctx.download(s) for s in DERIVS}
    n = o.n
    for b in range(B):
        add = limit_derivs(o, xs[b], lo[b], hi[b], w[b])
        for s in ("LX", "LXX", "LFX", "LFXX"):
            ex = got[False][s][b] + add[s]
            assert np.max(np.abs(add[s])) > 0
            print("linearize", name, s, b, rel_err(got[True][s][b], ex))
            assert rel_err(got[True][s][b], ex) <= 1e-12, (s, b, rel_err(got[True][s][b], ex))
        for s in ("LU", "LUU", "LUX"):
            assert np.array_equal(got[True][s][b], got[False][s][b]), s
        for t in range(T):
            blk = got[True]["LXX"][b][t * n * n:(t + 1) * n * n].reshape(n, n)
            assert np.array_equal(blk, blk.T)
        blk = got[True]["LFXX"][b].reshape(n, n)
        assert np.array_equal(blk, blk.T)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo", [("tree38", 0, None), ("chain6ff", 0, 0), ("chain6", 2, None), ("tree38_frame", 0, None),
                                             ("pendulum", 2, None)])
def test_cost_seq_aug(gpu, name, fd_mode, fo):
    """COSTS_OLD / COSTS_NEW (which = 0 / 1) against the flag-off context's plus the numpy limit terms, lf included"""
    capi = gpu
    T, B, mu = 12, 2, 30.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    xs, us = _trajs(o, model, B, 51)
    xs2, us2 = _trajs(o, model, B, 61)
    lo, hi, w = random_limits(o, xs, B, 52)
    mults = tc._mults(o, xs[0], 53)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | (capi.FLAG_STATE_LIMITS if on else 0)) as ctx:
            tc._setup(ctx, xs, us, mults, o.Etot)
            ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
            if on:
                ctx.set_state_limits(lo=lo, hi=hi, weight=w)
            ctx.cost_seq_aug(0, mu)
            ctx.cost_seq_aug(1, mu)
            got[on] = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
    for which, X in ((0, xs), (1, xs2)):
        for b in range(B):
            add = limit_terms(o, X[b], lo[b], hi[b], w[b])
            ex = got[False][which][b] + add
            assert np.any(add[:T] != 0.0) and (which == 1 or o.n == 2 or add[T] != 0.0)
            print("cost_seq_aug", name, which, b, rel_err(got[True][which][b], ex))
            assert rel_err(got[True][which][b], ex) <= 1e-12, (which, b, rel_err(got[True][which][b], ex))


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,mu", [("tree38", 60, 1.0), ("chain6", 30, 10.0)])
def test_sweep_parity_nonzero_value(gpu, name, T, mu):
    """the backward sweep with V_x != 0 from the limits alone, on the device's own derivatives against Oracle.backward:
    restarts, mu and reg identical, every step redone alone by the oracle from the device's V(t+1) to 1e-10
    (stepwise_backward_check).  Tree38 at T = 60 runs on K3h"""
    from oracle.binding import Oracle
    capi = gpu
    model, spec, o = make(name, T, fd_mode=2)
    xs, us = _trajs(o, model, 1, 71, held=True)
    lo, hi, w = random_limits(o, xs, 1, 72, wscale=0.1)
    mults = tc._mults(o, xs[0], 73)
    n, m = o.n, o.m
    with capi.Context(spec, flags=capi.FLAG_STATE_LIMITS | capi.FLAG_TRACE) as ctx:
        tc._setup(ctx, xs, us, mults, o.Etot)
        ctx.set_state_limits(lo=lo, hi=hi, weight=w)
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


def _full_cost(o, xs, us, mults, mu, lim, frames=None, task=None, ref=None):
    """the augmented cost per t (Oracle.cost_seq_aug: c/2 |u|^2 + the constraint terms) + the limit terms (+ frames, tracking)"""
    out = o.cost_seq_aug(xs, us, mults, mu) + limit_terms(o, xs, *lim)
    if frames is not None:
        out += fc.frame_terms(o, xs, frames, *task)
    if ref is not None:
        out += tc.track_terms(o, 1.0, xs, us, ref)
    return out


def _emulate_forward(o, xs, us, mults, fb, mu, n_alpha, cost, lo=None, hi=None):
    """sequential halving with the numpy cost: the first step 2^-k with sum_t (new - old) <= 0 (n_alpha = 0: the full step)"""
    old = cost(xs, us).sum()
    for k in range(34):
        step = 2.0 ** -k
        if lo is None:
            _, xn, un = o.forward_alpha(step, xs, us, mults, fb, mu)
        else:
            xn, un = fc._rollout(o, step, xs, us, fb, mu, lo, hi)
        new = cost(xn, un).sum()
        if n_alpha == 0 or new - old <= 0:
            return step, xn, un, new - old
    return None


FORWARD_CASES = [(name, fo, path, "", na, ks)
                 for name, fo, path in (("tree38", None, 1), ("chain6ff", 0, 0), ("tree38ff", 0, 1), ("tree38_frame", None, 1))
                 for na in (0, 1, 8) for ks in (1.0, 3.0)]
FORWARD_CASES += [("tree38", None, 1, extra, 8, 3.0) for extra in ("box", "track", "frame")]   # one case each with the other flags


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo,fwd_path,extra,n_alpha,k_scale", FORWARD_CASES)
def test_forward_matches_emulation(gpu, name, fo, fwd_path, extra, n_alpha, k_scale):
    """accepted step, X_NEW, U_NEW and dcost against Oracle.forward_alpha rollouts costed with numpy; k_scale 3 overshoots so
    that the halving runs; box: control bounds that bind on every third control (the emulation clamps; bounds on every control
    would clamp the overshoot away and the full step would be accepted); track / frame: those flags as well"""
    capi = gpu
    T, mu = 16, 1.0
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo)
    xs, us = _trajs(o, model, 1, 81, held=True)
    lo, hi, w = random_limits(o, xs, 1, 82, wscale=5.0)
    mults = tc._mults(o, xs[0], 85)
    blo = bhi = None
    ref = tc.random_ref(o, model, xs, us, 1, 84, spread=0.2) if extra == "track" else None
    frames = fc.pick_frames(model, 3) if extra == "frame" else None
    task = tuple(a[0] for a in fc.random_task(o, xs, frames, 1, 86, wscale=20.0, spread=0.1)) if frames else None
    flags = capi.FLAG_STATE_LIMITS | capi.FLAG_NO_TENSORS | {"": 0, "box": capi.FLAG_CONTROL_BOUNDS, "track": capi.FLAG_TRACKING_COST,
                                                             "frame": capi.FLAG_FRAME_COST}[extra]
    with capi.Context(spec, flags=flags) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        tc._setup(ctx, xs, us, mults, o.Etot)
        if ref is not None:
            tc.upload_ref(ctx, ref)
        if frames:
            ctx.set_frame_cost(frames=frames, target=task[0], weight=task[1])
        ctx.set_state_limits(lo=lo, hi=hi, weight=w)
        ctx.linearize()
        _, _, mu_o, _ = ctx.backward(0.0, mu)
        if k_scale != 1.0:
            ctx.upload("FB_VAL", k_scale * ctx.download("FB_VAL"))
        fb = {"origin": ctx.download("FB_ORIGIN")[0], "val": ctx.download("FB_VAL")[0], "jac": ctx.download("FB_JAC")[0]}
        if extra == "box":
            # every third control is held within 0.1 - 0.5 |k| of U (it binds at any step tried); the others are free, so the
            # tripled k still overshoots and the halving runs (bounds on every control clamp the overshoot away: step 1)
            rng = np.random.default_rng(83)
            width = 0.5 * np.abs(fb["val"]).reshape(T, o.m) / k_scale
            tight = (np.arange(o.m) % 3 == 0)[None, :]
            blo = np.where(tight, us[0].reshape(T, o.m) - width * rng.uniform(0.2, 1, size=(T, o.m)), -np.inf)
            bhi = np.where(tight, us[0].reshape(T, o.m) + width * rng.uniform(0.2, 1, size=(T, o.m)), np.inf)
            ctx.set_control_bounds(lo=blo, hi=bhi)
        rc, step, dcost = ctx.forward(mu_o, n_alpha=n_alpha)
        xn, un = ctx.download("X_NEW")[0], ctx.download("U_NEW")[0]

    def cost(X, U):
        return _full_cost(o, X, U, mults, mu_o[0], (lo[0], hi[0], w[0]), frames, task, ref)
    em = _emulate_forward(o, xs[0], us[0], mults, fb, mu_o[0], n_alpha, cost, blo, bhi)
    assert em is not None
    step_ref, xn_ref, un_ref, new = em
    print("forward", name, extra, n_alpha, k_scale, "step", step[0], step_ref, "dcost", dcost[0], new)
    assert step[0] == step_ref, (step, step_ref)
    if k_scale != 1.0 and n_alpha:
        assert step[0] < 1.0
    if extra == "box":
        Un = un.reshape(T, o.m)
        assert np.any(Un == blo) or np.any(Un == bhi)
    assert rel_err(xn, xn_ref) < 1e-9 and rel_err(un, un_ref) < 1e-9
    assert abs(dcost[0] - new) <= 1e-9 * max(1.0, abs(new)), (dcost[0], new)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo,flags", [("chain6ff", 2, 0, 0), ("tree38", 0, 0, 1)])
def test_instances_are_independent(gpu, name, fd_mode, fo, flags):
    """batch 3, three different sets of limits, through ddp_hip_solve: each instance as a batch-1 context given its own data"""
    capi = gpu
    T, B = 12, 3
    iters, thr, mu, w_, n_ = 4, 1e-9, 10.0, 1e-1, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo)
    _, spec1, _ = make(name, T, batch=1, fd_mode=fd_mode, first_order_fd=fo)
    xs, us = _trajs(o, model, B, 91, held=True)
    lo, hi, w = random_limits(o, xs, B, 92)

    def run(sp, sl):
        with capi.Context(sp, flags=capi.FLAG_STATE_LIMITS | flags) as ctx:
            tc._setup(ctx, xs[sl], us[sl])
            ctx.set_state_limits(lo=lo[sl], hi=hi[sl], weight=w[sl])
            _, log = ctx.solve(iters, thr, mu, 0.0, w_, n_, n_alpha=8)
            return log, ctx.download("X"), ctx.download("U"), ctx.info()
    lb, Xb, Ub, ib = run(spec, slice(0, B))
    assert len({tuple(Xb[b][-o.nx:]) for b in range(B)}) == B
    assert not np.array_equal(Xb, xs)
    for b in range(B):
        l1, X1, U1, i1 = run(spec1, slice(b, b + 1))
        for k in ("iterations", "result", "last_step", "mu", "reg"):
            assert l1[k][0] == lb[k][b], (k, b)
        assert rel_err(X1[0], Xb[b]) <= 1e-12 and rel_err(U1[0], Ub[b]) <= 1e-12
        same = {k: v for k, v in i1.items() if k != "hbm_bytes"} == {k: v for k, v in ib.items() if k != "hbm_bytes"}
        if same:
            assert np.array_equal(X1[0], Xb[b]) and np.array_equal(U1[0], Ub[b])
            for k in ("opt_obj", "opt_constr", "w", "n"):
                assert l1[k][0] == lb[k][b], (k, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,flags", [("chain6", 2, 0), ("tree38", 0, 1)])
def test_solve_matches_stepwise(gpu, name, fd_mode, flags):
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B, iters, thr, mu, w_, n_ = 10, 2, 5, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode)
    xs, us = _trajs(o, model, B, 101, held=True)
    lo, hi, w = random_limits(o, xs, B, 102)
    mults = tc._mults(o, xs[0], 103)

    def run(stepwise):
        with capi.Context(spec, flags=capi.FLAG_STATE_LIMITS | flags) as ctx:
            tc._setup(ctx, xs, us, mults, o.Etot)
            if o.Etot:
                ctx.upload("MULT_ORIGIN", xs[:, :T * o.nx])
            ctx.set_state_limits(lo=lo, hi=hi, weight=w)
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
def test_velocity_limit_tightens_with_weight(gpu):
    """the pendulum swing-up of test_tracking_cost.py::test_pendulum_terminal_weight (T = 100, terminal weight 1e3 on
    q_T = 3.14, 300 iterations), then with |v| <= 0.6 v_peak at every t under weights 1, 1e2, 1e4: the peak violation
    max_t max(|v_t| - 0.6 v_peak, 0) decreases strictly with the weight and stays below 0.4 v_peak, the unlimited one.
    (The violations are printed; DESIGN.md section 4k records them once measured.)"""
    capi = gpu
    T, target = 100, 3.14
    model = capi.BuiltinModel(capi.BUILTIN_PENDULUM)
    spec = capi.ProblemSpec(model, T, dt=0.01, c=1.0, batch=1, fd_mode=2)
    from oracle.binding import Oracle
    o = Oracle(model, T, dt=0.01, c=1.0, fd_mode=2)
    us = np.zeros(T)
    xs = o.rollout(np.zeros(2), us)
    xref = np.zeros((T + 1, 2)); xref[T, 0] = target
    wx = np.zeros((T + 1, 2)); wx[T, 0] = 1e3

    def solve(vmax, wv):
        with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_STATE_LIMITS) as ctx:
            tc._setup(ctx, xs[None], us[None])
            ctx.set_tracking_cost(xref=xref, wx=wx)
            if vmax is not None:
                ctx.set_state_limits(lo=np.array([-np.inf, -vmax]), hi=np.array([np.inf, vmax]), weight=np.array([0.0, wv]))
            ctx.solve(300, 1e-9, 1e2, 0.0, 1e-1, 10.0, n_alpha=8)
            X = ctx.download("X")[0].reshape(T + 1, 2)
        assert np.all(np.isfinite(X))
        return X
    v_peak = np.max(np.abs(solve(None, 0.0)[:, 1]))
    assert v_peak > 0
    viol = []
    for wv in (1.0, 1e2, 1e4):
        X = solve(0.6 * v_peak, wv)
        viol.append(float(np.max(np.maximum(np.abs(X[:, 1]) - 0.6 * v_peak, 0.0))))
    print("velocity limit: v_peak", v_peak, "violations", viol, "unlimited", 0.4 * v_peak)
    assert viol[0] > viol[1] > viol[2], viol
    assert all(v < 0.4 * v_peak for v in viol), (viol, v_peak)


@pytest.mark.gpu
def test_joint_limit_descends(gpu):
    """tree38, T = 40, tensor-free, a posture-tracking cost whose reference (the held posture) lies 0.3 rad outside position
    limits on ten joints: sum_t COSTS_OLD never increases over 8 iterations and the summed position violation ends below the
    initial one"""
    capi = gpu
    T, mu, iters = 40, 1.0, 8
    model, spec, o = make("tree38", T, fd_mode=0)
    xs, us = _trajs(o, model, 1, 111, held=True)
    nv, n = o.nv, o.n
    posture = xs[0][:nv].copy()
    xref = np.tile(np.concatenate([posture, np.zeros(nv)]), (T + 1, 1))
    wx = np.tile(np.concatenate([np.full(nv, 10.0), np.full(nv, 0.1)]), (T + 1, 1))
    joints = np.random.default_rng(112).choice(nv, size=10, replace=False)
    lo, hi, w = np.full(n, -np.inf), np.full(n, np.inf), np.zeros(n)
    hi[joints] = posture[joints] - 0.3
    w[joints] = 100.0

    def violation(X):
        return float(np.sum(np.maximum(X.reshape(T + 1, o.nx)[:, joints] - hi[joints], 0.0)))
    with capi.Context(spec, flags=capi.FLAG_TRACKING_COST | capi.FLAG_STATE_LIMITS | capi.FLAG_NO_TENSORS) as ctx:
        tc._setup(ctx, xs, us)
        ctx.set_tracking_cost(xref=xref, wx=wx)
        ctx.set_state_limits(lo=lo, hi=hi, weight=w)
        costs = []
        for _ in range(iters):
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            rc, step, dcost = ctx.forward(mu_o, n_alpha=8)
            costs.append(ctx.download("COSTS_OLD")[0].sum())
            ctx.swap_traj()
        final = ctx.download("X")[0]
    print("joint limit costs", costs, "violation", violation(xs[0]), "->", violation(final))
    for a, b in zip(costs, costs[1:]):
        assert b <= a * (1 + 1e-12), costs
    assert violation(xs[0]) > 0 and violation(final) < violation(xs[0])


@pytest.mark.gpu
def test_refusals_and_defaults(gpu):
    import ctypes as C
    capi = gpu
    T, B = 4, 2
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    n = o.n
    L = capi.lib()
    dp = C.POINTER(C.c_double)
    full = (B, T + 1, n)

    def code(fn):
        with pytest.raises(capi.DdpHipError) as exc:
            fn()
        return exc.value.code
    with capi.Context(spec) as ctx:                                   # a context without the flag
        assert code(lambda: ctx.set_state_limits(weight=0.0)) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.state_limits()) == capi.E_UNSUPPORTED
    with capi.Context(spec, flags=capi.FLAG_STATE_LIMITS) as ctx:
        lo0, hi0, w0 = ctx.state_limits()                              # create: no limit anywhere
        assert lo0.shape == full and np.all(lo0 == -np.inf) and np.all(hi0 == np.inf) and np.all(w0 == 0.0)
        rng = np.random.default_rng(5)
        lo1 = rng.normal(size=full)
        hi1 = lo1 + rng.uniform(0.0, 1.0, size=full)
        hi1[0, 1, 7] = lo1[0, 1, 7]                                    # lo == hi is allowed
        lo1[1, 2, 8], hi1[1, 3, 9] = -np.inf, np.inf
        w1 = rng.uniform(0.0, 1.0, size=full); w1[..., :6] = 0.0
        ctx.set_state_limits(lo=lo1, hi=hi1, weight=w1)

        def resident_is(lo, hi, w):
            a, b, c = ctx.state_limits()
            return np.array_equal(a, lo) and np.array_equal(b, hi) and np.array_equal(c, w)
        assert resident_is(lo1, hi1, w1)

        def bad(arr, idx, v):
            out = arr.copy(); out[idx] = v
            return out
        at = (1, 2, 7)
        refused = [dict(lo=bad(lo1, at, np.nan)), dict(hi=bad(hi1, at, np.nan)), dict(weight=bad(w1, at, np.nan)),
                   dict(lo=bad(lo1, at, np.inf)), dict(hi=bad(hi1, at, -np.inf)),
                   dict(weight=bad(w1, at, -1e-3)), dict(weight=bad(w1, at, np.inf)),
                   dict(weight=bad(w1, (0, 3, 5), 0.5)), dict(weight=bad(w1, (1, 0, 0), 1e-9)),     # a free-flyer root's pose rows
                   dict(lo=bad(lo1, at, hi1[at] + 1e-9)),                                          # lo alone above the resident hi
                   dict(hi=bad(hi1, at, lo1[at] - 1e-9)),                                          # hi alone below the resident lo
                   dict(lo=bad(lo1, at, hi1[at] + 1.0), weight=w1 + 1.0 * (np.arange(n) >= 6))]    # nothing of a refused upload lands
        for kw in refused:
            assert code(lambda: ctx.set_state_limits(**kw)) == capi.E_ARG, list(kw)
            assert resident_is(lo1, hi1, w1), list(kw)
        # lo > hi with both sides in one call, past capi's own check
        lo_b = bad(lo1, at, hi1[at] + 1.0)
        assert L.ddp_hip_state_limits_upload(ctx._h, lo_b.ctypes.data_as(dp), hi1.ctypes.data_as(dp), None, 0, B) == capi.E_ARG
        assert resident_is(lo1, hi1, w1)
        # a bad instance range
        assert code(lambda: ctx.state_limits(first=1, count=B)) == capi.E_ARG
        assert code(lambda: ctx.set_state_limits(weight=0.0, first=B, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_state_limits(weight=0.0, first=-1, count=1)) == capi.E_ARG
        # a NULL side is left as it is; a partial-range upload lands in its range only
        hi2 = hi1.copy(); hi2[1] = hi1[1] + 1.0
        ctx.set_state_limits(hi=hi2[1], first=1, count=1)
        assert resident_is(lo1, hi2, w1)
        w2 = w1.copy(); w2[0] = 0.25 * (np.arange(n) >= 6)
        ctx.set_state_limits(weight=0.25 * (np.arange(n) >= 6), first=0, count=1)          # an (n,) vector for every step
        assert resident_is(lo1, hi2, w2)
        ctx.set_state_limits(lo=-2.0, hi=np.full((T + 1, n), 3.0))                          # a scalar and (T+1, n) for the batch
        assert resident_is(np.full(full, -2.0), np.full(full, 3.0), w2)
        l1, h1, _ = ctx.state_limits(first=1, count=1)
        assert l1.shape == (1, T + 1, n) and np.all(l1 == -2.0) and np.all(h1 == 3.0)
    _, spec_v, _ = make("chain6", T, fd_mode=0)
    with capi.Context(spec_v, flags=capi.FLAG_STATE_LIMITS) as ctx:
        ctx.set_state_limits(weight=1.0)                               # rows 0 .. 5 are ordinary rows without a free flyer
        assert np.all(ctx.state_limits()[2] == 1.0)
