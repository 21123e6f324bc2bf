"""The three-wave pipelined form of the forward latency kernel (fwd.hip: forward_kernel_lat2<…, PIPE>; DESIGN.md section 4, "The
pipelined form"): the assistant wave forms dx, K dx, u_t, the inline cost terms and the prefetch beside the leading wave's pass 1
and hands u_t over through one LDS word.  Every expression and its order are the two-wave form's, so a default context and one
created under DDP_HIP_FWD_NO_PIPE agree bit for bit on X_NEW, U_NEW, step and dcost.

Every case linearises and runs the backward sweep on the device first, on trajectories with non-zero velocities at every t.  The
plain problem's cost is c/2 |u|^2 alone: its value function has no state terms and the sweep's K_t is zero, so the cases without
a state cost add random gains to the sweep's (per instance, the same in both contexts); with a tracking, frame or limit term the
sweep's own K_t is non-zero and is used as it is.  tree38, T = 4, batch 3 unless a case says otherwise."""
import functools

import numpy as np
import pytest

import test_frame_cost as fc
import test_frame_orient_cost as fo
import test_state_limits as sl
import test_tracking_cost as tc
from problems import make, random_state

pytestmark = pytest.mark.gpu

T, B = 4, 3
OUTS = ("X_NEW", "U_NEW")


@functools.lru_cache(maxsize=None)
def problem(name, T=T, B=B):
    """(model, spec, oracle, X, U), once per shape.  tree38: a posture held under computed-torque control from a moving start,
    random u on top (tests/test_sparse_caches.py::_problem); tree38ff: a random state with a unit quaternion, random controls"""
    if name == "tree38":
        model, spec, o = make(name, T, batch=B, fd_mode=2, first_order_fd=1)
    else:
        model, spec, o = make(name, T, batch=B, fd_mode=0, first_order_fd=0)
    nv, nq = model.nv, o.nx - model.nv
    X, U = [], []
    for b in range(B):
        rng = np.random.default_rng(40 + b)
        if name == "tree38":
            q0 = 0.3 * rng.normal(size=nv)
            x = np.concatenate([q0, 0.2 * rng.normal(size=nv)])
            x0, us = x.copy(), np.zeros(T * nv)
            for t in range(T):
                us[t * nv:(t + 1) * nv] = o.rnea(x[:nv], x[nv:], -100.0 * (x[:nv] - q0) - 20.0 * x[nv:]) + 0.3 * rng.normal(size=nv)
                x = o.eval_f(x, us[t * nv:(t + 1) * nv])
        else:
            x0, us = random_state(model, rng, 0.3), 0.3 * rng.normal(size=T * nv)
        xs = o.rollout(x0, us)
        assert np.all(np.isfinite(xs)) and all(np.max(np.abs(xs[t * o.nx + nq:(t + 1) * o.nx])) > 0 for t in range(T))
        X.append(xs)
        U.append(us)
    return model, spec, o, np.stack(X), np.stack(U)


def _add_gains(ctx):
    """random gains on top of the sweep's, instance b from a generator of its own (the same whatever the batch)"""
    K = ctx.download("FB_JAC")
    for b in range(K.shape[0]):
        K[b] += 0.1 * np.random.default_rng(700 + b).normal(size=K.shape[1])
    ctx.upload("FB_JAC", K)


def _forward(capi, spec, X, U, n_alpha, flags=0, setup=None, after_backward=_add_gains, active=None, first=0, count=None):
    """linearise, backward and one forward of instances first .. first + count - 1 in a context of their own"""
    count = spec.batch if count is None else count
    with capi.Context(spec, flags=flags) as ctx:
        assert ctx.info()["fwd_path"] == 1
        for s, arr in (("X", X), ("U", U), ("X_NEW", X), ("U_NEW", U)):
            ctx.upload(s, arr[first:first + count])
        if setup:
            setup(ctx)
        ctx.linearize()
        _, _, mu, _ = ctx.backward(0.0, 1.0)
        if after_backward:
            after_backward(ctx)
        out = {"K": ctx.download("FB_JAC"), "k": ctx.download("FB_VAL")}
        if active is not None:
            ctx.set_active(active)
        rc, step, dcost = ctx.forward(mu, n_alpha=n_alpha)
        out.update({s: ctx.download(s) for s in OUTS})
    live = np.ones(count, dtype=bool) if active is None else np.asarray(active, dtype=bool)
    out["step"], out["dcost"], out["rc"] = step[live], dcost[live], rc    # (the forward writes no step for a frozen instance)
    return out


def _pair(capi, monkeypatch, spec, X, U, n_alpha, **kw):
    got = _forward(capi, spec, X, U, n_alpha, **kw)
    monkeypatch.setenv("DDP_HIP_FWD_NO_PIPE", "1")
    ref = _forward(capi, spec, X, U, n_alpha, **kw)
    monkeypatch.delenv("DDP_HIP_FWD_NO_PIPE")
    return got, ref


def _same(got, ref):
    assert got["rc"] == ref["rc"]
    assert np.all(np.isfinite(ref["K"])) and np.any(ref["K"] != 0.0)          # the gain product is exercised
    for s in ("K", "k") + OUTS + ("step", "dcost"):
        assert np.all(np.isfinite(ref[s])), s
        assert np.array_equal(got[s], ref[s]), (s, float(np.max(np.abs(got[s] - ref[s]))))


@pytest.mark.parametrize("n_alpha", [8, 3, 1])
def test_assist_bit_for_bit(gpu, monkeypatch, n_alpha):
    """n_alpha = 8: the full set; 3: the last workgroup holds one candidate; 1: a candidate alone in its workgroup"""
    model, spec, o, X, U = problem("tree38")
    got, ref = _pair(gpu, monkeypatch, spec, X, U, n_alpha)
    _same(got, ref)
    assert np.any(got["U_NEW"] != U)                             # a candidate was rolled out and copied


def test_assist_later_rounds(gpu, monkeypatch):
    """the sweep's feed-forward with its sign turned is an ascent direction: every step size is rejected, all five rounds of eight
    run (round * n_alpha + a up to 39: the lanes of candidates 34 .. 39 are never tried and leave INFINITY), the call reports the
    floor"""
    capi = gpu
    model, spec, o, X, U = problem("tree38")

    def turn(ctx):
        _add_gains(ctx)
        ctx.upload("FB_VAL", -ctx.download("FB_VAL"))

    got, ref = _pair(capi, monkeypatch, spec, X, U, 8, after_backward=turn)
    assert ref["rc"] == capi.EV_LINESEARCH_FLOOR and np.all(ref["step"] == 2.0 ** -34)
    _same(got, ref)


def test_assist_free_flyer(gpu, monkeypatch):
    """the SE(3) difference of the root on the assistant wave, the root's step_accel_ff_root reading u in pass 3"""
    capi = gpu
    model, spec, o, X, U = problem("tree38ff")
    got, ref = _pair(capi, monkeypatch, spec, X, U, 8, flags=capi.FLAG_NO_TENSORS)
    _same(got, ref)
    assert np.any(got["U_NEW"] != U)


def test_assist_control_bounds(gpu, monkeypatch):
    """BOX: a band of 1e-3 around the old controls, far inside the unconstrained update: controls of the accepted rollout sit on it"""
    capi = gpu
    model, spec, o, X, U = problem("tree38")
    lo, hi = U.reshape(B, T, model.nv) - 1e-3, U.reshape(B, T, model.nv) + 1e-3
    got, ref = _pair(capi, monkeypatch, spec, X, U, 8, flags=capi.FLAG_CONTROL_BOUNDS, setup=lambda ctx: ctx.set_control_bounds(lo=lo, hi=hi))
    _same(got, ref)
    u = got["U_NEW"].reshape(B, T, model.nv)
    assert np.all((u >= lo) & (u <= hi)) and np.any((u == lo) | (u == hi))


def _tracking(capi, model, o, X, U):
    ref = tc.random_ref(o, model, X, U, B, 61)
    return capi.FLAG_TRACKING_COST, lambda ctx: tc.upload_ref(ctx, ref)


def _frames(capi, model, o, X, U):
    frames = fc.pick_frames(model, 3)
    tgt, w = fc.random_task(o, X, frames, B, 62)
    return capi.FLAG_FRAME_COST, lambda ctx: ctx.set_frame_cost(frames=frames, target=tgt, weight=w)


def _orient(capi, model, o, X, U):
    frames = fc.pick_frames(model, 3)
    tgt, w = fc.random_task(o, X, frames, B, 63)
    quat, wq = fo.random_orient(o, X, frames, B, 64)

    def setup(ctx):
        ctx.set_frame_cost(frames=frames, target=tgt, weight=w)
        ctx.set_frame_orient_cost(quat=quat, weight=wq)
    return capi.FLAG_FRAME_COST | capi.FLAG_FRAME_ORIENT_COST, setup


def _limits(capi, model, o, X, U):
    lo, hi, w = sl.random_limits(o, X, B, 65)
    return capi.FLAG_STATE_LIMITS, lambda ctx: ctx.set_state_limits(lo=lo, hi=hi, weight=w)


@pytest.mark.parametrize("term", [_tracking, _frames, _orient, _limits], ids=["cost1", "cost2", "cost10", "cost4"])
def test_assist_inline_cost_terms(gpu, monkeypatch, term):
    """one context per inline term (COST 1, 2, 8 + 2, 4): its lane sums, the frame walks among them, run on the assistant wave
    and its dsum decides the line search.  (COST 8 + 2 on a fixed root is one of the five instantiations that keep the two-wave
    pipelined body, fwd.hip: fwd_pipe_assist: the same check holds for it)"""
    capi = gpu
    model, spec, o, X, U = problem("tree38")
    flags, setup = term(capi, model, o, X, U)
    got, ref = _pair(capi, monkeypatch, spec, X, U, 8, flags=flags, setup=setup, after_backward=None)   # the sweep's own gains
    _same(got, ref)
    assert np.any(got["dcost"] != 0.0)


@pytest.mark.parametrize("name", ["tree38", "tree38ff"])
def test_assist_rollout(gpu, monkeypatch, name):
    """ctx.rollout(): the open-loop instantiation, whose assistant copies u_old and prefetches"""
    capi = gpu
    model, spec, o, X, U = problem(name)
    out = []
    for no_pipe in (False, True):
        if no_pipe:
            monkeypatch.setenv("DDP_HIP_FWD_NO_PIPE", "1")
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS) as ctx:
            bad = np.full_like(X, np.nan); bad[:, :o.nx] = X[:, :o.nx]
            ctx.upload("X", bad); ctx.upload("U", U)
            ctx.rollout()
            out.append(ctx.download("X"))
    monkeypatch.delenv("DDP_HIP_FWD_NO_PIPE")
    assert np.all(np.isfinite(out[1])) and np.array_equal(out[0], out[1])
    assert np.max(np.abs(out[0] - X)) < 1e-9                     # (and it is the oracle's rollout)


def test_assist_frozen_instance(gpu, monkeypatch):
    """state[b] != 0: the workgroups of a frozen instance return above the loop, all three waves together"""
    model, spec, o, X, U = problem("tree38")
    got, ref = _pair(gpu, monkeypatch, spec, X, U, 8, active=[1, 0, 1])
    _same(got, ref)
    assert np.array_equal(got["X_NEW"][1], X[1]) and np.array_equal(got["U_NEW"][1], U[1])
    assert np.any(got["U_NEW"][0] != U[0]) and np.any(got["U_NEW"][2] != U[2])


def test_assist_form_selection_unchanged(gpu):
    """batch x ceil(n_alpha / 2) workgroups beyond the compute units: fwd_use_pipe still takes the four-candidate form (the info()
    path is what it was), and its first instances agree bit for bit with a three-instance, pipelined run of them"""
    import ctypes as C
    capi = gpu
    n = C.c_int(0)
    assert capi.lib().hipDeviceGetAttribute(C.byref(n), 63, 0) == 0          # hipDeviceAttributeMultiprocessorCount
    bmax = n.value // 4
    assert 3 <= bmax <= 256, n.value
    model, spec, o, X, U = problem("tree38", 2, bmax + 1)
    big = _forward(capi, spec, X, U, 8)
    _, spec3, _ = make("tree38", 2, batch=3, fd_mode=2, first_order_fd=1)
    small = _forward(capi, spec3, X, U, 8, count=3)
    for s in ("K",) + OUTS + ("step", "dcost"):
        assert np.all(np.isfinite(big[s])), s
        assert np.array_equal(big[s][:3], small[s]), s
