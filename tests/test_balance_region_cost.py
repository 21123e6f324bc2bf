"""Per-instance balance-region costs (DDP_HIP_FLAG_BALANCE_REGION_COST, include/ddp_hip/ddp_hip.h):

    xi_o = c + tau_o cdot,   d_o = n_o . xi_o - h_o,   e_o = !(d_o >= 0) ? d_o : 0
    l(t, x, u) += 1/2 sum_o w e_o^2,   lf(x_T) alike with row T

The oracle has no such cost, so the yardstick is the numpy restatement below, built on the helpers of the neighbouring modules:
c and Jc from test_com_cost (com, com_jac), cdot = l / M and d cdot / d(delta q) from rows 0 .. 2 of
test_momentum_cost.momentum_jacobians divided by M.  test_yardstick_gradient holds it against central differences.  The emulated
forward, the task generators' conventions and make_any come from those modules by import; the tolerances are the project's own
for the same comparisons."""
import os
import re
import subprocess

import numpy as np
import pytest

import test_com_cost as cm
import test_frame_cost as fc
import test_momentum_cost as mo
import test_obstacle_cost as ob
import test_tracking_cost as tc
from problems import make
from synth import rel_err, stepwise_backward_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 1e-3
TOL_FD, TOL_LIN, TOL_FWD, TOL_SWEEP = 1e-8, 1e-12, 1e-9, 1e-10
DERIVS = fc.DERIVS
NAMES = fc.NAMES
MODELS = ["chain6", "chain6ff", "tree38", "tree38ff", "table7"]
W5 = ob.W5
make_any = cm.make_any
_trajs, _setup, _moving = tc._trajs, tc._setup, mo._moving
NP = 6                                                   # plane slots of the generated tasks: even slots tau = 0, odd slots tau in [0.1, 0.5]


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def mass(model):
    return float(np.sum(model.mass_j))


def point(o, model, x, tau, jacobian=False):
    """xi = c + tau cdot at the state x; with `jacobian` (xi, Jq, Jv), each (3, nv).  tau = 0 reads no velocity"""
    q, v = x[:o.nq], x[o.nq:]
    c = cm.com(o, model, q)
    Jc = cm.com_jac(o, model, q) if jacobian else None
    if tau == 0.0:
        return (c, Jc, np.zeros((3, o.nv))) if jacobian else c
    M = mass(model)
    h, Hq, _ = mo.momentum_jacobians(o, model, q, v, jacobian=jacobian)
    xi = c + tau * (h[:3] / M)
    return (xi, Jc + tau * (Hq[:3] / M), tau * Jc) if jacobian else xi


def distances(o, model, x, g_t, live=None):
    """d_o of every plane of g_t (P, 5) at the state x (nan-free inputs); planes with live[o] false are not evaluated (0)"""
    pts = {}
    d = np.zeros(len(g_t))
    for i, g in enumerate(g_t):
        if live is not None and not live[i]:
            continue
        tau = float(g[4])
        if tau not in pts:
            pts[tau] = point(o, model, x, tau)
        d[i] = g[:3] @ pts[tau] - g[3]
    return d


def br_terms(o, model, xs, geom, w):
    """the terms of one instance per t (T+1 values; the last belongs to lf); geom (T+1, P, 5), w (T+1, P)"""
    X = xs.reshape(o.T + 1, o.nx)
    out = np.zeros(o.T + 1)
    for t in range(o.T + 1):
        live = w[t] != 0.0
        if not live.any():
            continue
        d = distances(o, model, X[t], geom[t], live)
        e = np.where(live & ~(d >= 0), d, 0.0)
        out[t] = 0.5 * np.sum(w[t] * e * e)
    return out


def br_margin(o, model, xs, geom, w):
    """min over the planes with w != 0 of d_o per t, +inf where none is live"""
    X = xs.reshape(o.T + 1, o.nx)
    out = np.full(o.T + 1, np.inf)
    for t in range(o.T + 1):
        live = w[t] != 0.0
        if live.any():
            out[t] = np.min(distances(o, model, X[t], geom[t], live)[live])
    return out


def br_grad_hess(o, model, x, g_t, w_t, drop_q=False):
    """(lx, lxx, active) contributions at one state: sum w e z and the Gauss-Newton sum w z z^T over the planes with w != 0 and
    e != 0.  drop_q: without tau d cdot / dq (what an implementation that forgot it would form)"""
    n, nv = o.n, o.nv
    g, Hm = np.zeros(n), np.zeros((n, n))
    live = w_t != 0.0
    act = np.zeros(len(g_t), dtype=bool)
    if not live.any():
        return g, Hm, act
    d = distances(o, model, x, g_t, live)
    act = live & ~(d >= 0)
    jac = {}
    for i in np.nonzero(act)[0]:
        tau = float(g_t[i][4])
        if tau not in jac:
            jac[tau] = point(o, model, x, tau, jacobian=True)
        _, Jq, Jv = jac[tau]
        if drop_q:
            Jq = cm.com_jac(o, model, x[:o.nq])
        z = np.concatenate([Jq.T @ g_t[i][:3], Jv.T @ g_t[i][:3]])
        g += w_t[i] * d[i] * z
        Hm += w_t[i] * np.outer(z, z)
    return g, Hm, act


def br_derivs(o, model, xs, geom, w, drop_q=False):
    """what the terms add to LX, LXX, LFX, LFXX of one instance, in the library's flat (column-major) layout"""
    X = xs.reshape(o.T + 1, o.nx)
    out = {"LX": [], "LXX": []}
    for t in range(o.T + 1):
        g, Hm, _ = br_grad_hess(o, model, X[t], geom[t], w[t], drop_q)
        if t == o.T:
            out["LFX"], out["LFXX"] = g, Hm.ravel(order="F")
        else:
            out["LX"].append(g); out["LXX"].append(Hm.ravel(order="F"))
    out["LX"], out["LXX"] = np.concatenate(out["LX"]), np.concatenate(out["LXX"])
    return out


def random_task(o, model, xs, B, seed, wscale=1.0, p_clear=0.5, depth=(0.01, 0.1), P=NP):
    """geom (B, T+1, P, 5) and weights (B, T+1, P): per (instance, t, slot) a random unit normal, tau = 0 on the even slots and
    tau in [0.1, 0.5] on the odd ones, and an offset that leaves the tested point clear by `depth` with probability p_clear, else
    violated by as much"""
    rng = np.random.default_rng(seed)
    T = o.T
    geom, w = np.zeros((B, T + 1, P, 5)), wscale * rng.uniform(0.5, 5.0, size=(B, T + 1, P))
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            for s_ in range(P):
                n = ob._unit(rng)
                tau = 0.0 if s_ % 2 == 0 else rng.uniform(0.1, 0.5)
                dep = rng.uniform(*depth)
                sd = dep if rng.uniform() < p_clear else -dep
                geom[b, t, s_] = np.concatenate([n, [n @ point(o, model, X[t], tau) - sd, tau]])
    return geom, w


def check_task(o, model, trajs, geom, w, fractions=True):
    """the conditions on the inputs, on the yardstick alone: along every trajectory of `trajs` (each (B, ...): the resident ones
    and the emulated line-search candidates) every live plane has |d| >= 1e-6, so that device and yardstick agree on which
    planes are active; of the first one at least a quarter of the (b, t, o) triples are active and at least a quarter clear.
    Returns the first one's activity (B, T+1, P)"""
    first = None
    for xs in trajs:
        B, T = xs.shape[0], o.T
        active = np.zeros(w.shape, dtype=bool)
        for b in range(B):
            X = xs[b].reshape(T + 1, o.nx)
            for t in range(T + 1):
                live = w[b, t] != 0.0
                d = distances(o, model, X[t], geom[b, t], live)
                assert np.all(np.abs(d[live]) >= 1e-6), (b, t, d)
                active[b, t] = live & (d < 0)
        if first is None:
            first = active
    if fractions:
        assert 4 * first.sum() >= first.size and 4 * (~first).sum() >= first.size, (first.sum(), first.size)
    return first


def set_task(ctx, geom=None, weight=None, P=NP):
    ctx.set_balance_region_planes(P)
    if geom is not None or weight is not None:
        ctx.set_balance_region_cost(geom=geom, weight=weight)


def _on(capi):
    return capi.FLAG_BALANCE_REGION_COST


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_yardstick_gradient(name):
    """lx against the 5-point central difference (H = 1e-3) of the numpy cost along x (+) (+-h e_j) over all 2 nv tangent
    directions at TOL_FD, with planes violated or clear by 5 .. 10 cm (the one-sided term is C^1 alone: no plane changes side
    inside the stencil); lxx symmetric bit for bit and positive semidefinite; the v half of the gradient non-zero, and zero with
    the tau != 0 slots switched off.  A check of the numpy restatement alone: it calls nothing of the library's new code"""
    T = 2
    model, _, o = make_any(name, T, fd_mode=0)
    xs, us = _trajs(o, model, 1, 3)
    xs = _moving(xs, o, 5)
    geom, w = random_task(o, model, xs, 1, 4, depth=(0.05, 0.1))
    act = check_task(o, model, [xs], geom, w)
    X = xs[0].reshape(T + 1, o.nx)
    nv, n = o.nv, o.n
    for t in ((1, T) if n <= 26 else (T,)):
        assert act[0, t].any() and act[0, t, 1::2].any() and act[0, t, 0::2].any()
        g, Hm, a = br_grad_hess(o, model, X[t], geom[0, t], w[0, t])
        assert np.array_equal(a, act[0, t])
        assert np.max(np.abs(g[:nv])) > 0 and np.max(np.abs(g[nv:])) > 0
        assert np.array_equal(Hm, Hm.T) and np.min(np.linalg.eigvalsh(Hm)) >= -1e-12 * np.max(np.abs(Hm))
        w0 = w[0, t].copy(); w0[1::2] = 0.0
        g0, H0, _ = br_grad_hess(o, model, X[t], geom[0, t], w0)
        assert np.all(g0[nv:] == 0.0) and np.all(H0[nv:, :] == 0.0) and np.all(H0[:, nv:] == 0.0) and np.max(np.abs(g0)) > 0

        def cost_at(dx):
            x2 = tc._integrate_x(o, X[t], dx)
            live = w[0, t] != 0.0
            d = distances(o, model, x2, geom[0, t], live)
            assert np.array_equal(live & (d < 0), act[0, t])          # the stencil stays on one side of every plane
            return 0.5 * np.sum(w[0, t] * np.where(d < 0, d, 0.0) ** 2)
        fd = np.zeros(n)
        for j in range(n):
            e = np.zeros(n); e[j] = H
            fd[j] = sum(cw * cost_at(s * e) for s, cw in W5) / H
        err = np.max(np.abs(fd - g)) / max(1.0, np.max(np.abs(g)))
        print("yardstick", name, t, err)
        assert err <= TOL_FD, err
        g_noq = br_grad_hess(o, model, X[t], geom[0, t], w[0, t], drop_q=True)[0]
        assert np.max(np.abs(fd - g_noq)) > 1e-4 * np.max(np.abs(g))        # tau d cdot / dq matters at these inputs


def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.FLAG_BALANCE_REGION_COST == 32768 and re.search(r"#define\s+DDP_HIP_FLAG_BALANCE_REGION_COST\s+32768u", header)
    assert re.search(r"#define\s+DDP_HIP_MAX_REGION_PLANES\s+8\b", header)
    L = capi.lib()
    for name in ("ddp_hip_balance_region_set_planes", "ddp_hip_balance_region_upload", "ddp_hip_balance_region_download",
                 "ddp_hip_balance_region_margin", "ddp_hip_model_capture_point"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    assert len(capi.SEQ_NAMES) == 40
    for name in ("set_balance_region_planes", "set_balance_region_cost", "get_balance_region_cost", "balance_region_margin"):
        assert hasattr(capi.Context, name), name
    assert hasattr(capi.ModelHandle, "capture_point")
    # shapes are checked before anything reaches the library: a context object without a device will do
    T, B, P = 5, 2, 3
    model, spec, _ = make("chain6", T, batch=B, fd_mode=0)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx._h = spec, B, None
    with pytest.raises(ValueError, match="set_balance_region_planes"):
        ctx.set_balance_region_cost(weight=np.zeros(P))
    ctx.n_region_planes = P
    for kw in (dict(geom=np.zeros((P, 4))), dict(geom=np.zeros(5)), dict(geom=np.zeros((T, P, 5))), dict(geom=np.zeros((B + 1, T + 1, P, 5))),
               dict(weight=np.zeros(P - 1)), dict(weight=0.0), dict(weight=np.zeros((T, P))), dict(weight=np.zeros((B, T + 1, P)), count=1),
               dict(geom=np.zeros((P, 5)), weight=np.zeros((T + 1, P + 1)))):
        with pytest.raises(ValueError):
            ctx.set_balance_region_cost(**kw)


def test_balance_region_block_host_logic():
    """host/test_balance_region_block.cpp: the term's record and index, the geometry validator and what an upload of planes and
    weights decides (csrc/cost_block.h), which need no device"""
    host = os.path.join(ROOT, "host")
    subprocess.check_call(["make", "-s", "-C", host, "test_balance_region_block"])
    out = subprocess.run([os.path.join(host, "test_balance_region_block")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _state(o, rng):
    q, v = rng.normal(size=o.nq), rng.normal(size=o.nv)
    if o.nq != o.nv:
        q[3:7] /= np.linalg.norm(q[3:7])
    return np.concatenate([q, v])


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_model_capture_point(gpu, name):
    """ModelHandle.capture_point against the yardstick: xi, Jq, Jv to TOL_LIN; tau = 0 gives Jv exactly zero, xi and Jq bit for
    bit ModelHandle.com's c and jacobian, and reads no velocity (a NaN v changes nothing); a free-flyer root's three linear columns
    of Jq are bit for bit Jc's (d cdot / dq is left out there); the refusals"""
    capi = gpu
    model, _, o = make_any(name, 2, fd_mode=0)
    rng = np.random.default_rng(5)
    with capi.ModelHandle(model) as hd:
        for k, tau in enumerate((0.31, 0.1, 0.0)):
            x = _state(o, rng)
            q, v = x[:o.nq], x[o.nq:]
            xi, Jq, Jv = hd.capture_point(q, v, tau, jacobian=True)
            assert np.array_equal(xi, hd.capture_point(q, v, tau))
            ex = point(o, model, x, tau, jacobian=True)
            errs = [rel_err(a, b) if np.max(np.abs(b)) > 0 else float(np.max(np.abs(a))) for a, b in zip((xi, Jq, Jv), ex)]
            print("capture_point", name, tau, errs)
            assert max(errs) <= TOL_LIN, errs
            c, Jc = hd.com(q, jacobian=True)
            if tau == 0.0:
                assert np.all(Jv == 0.0) and np.array_equal(Jq, Jc) and np.array_equal(xi, c)
                xn, Jqn, Jvn = hd.capture_point(q, np.full(o.nv, np.nan), 0.0, jacobian=True)
                assert np.array_equal(xn, xi) and np.array_equal(Jqn, Jq) and np.all(Jvn == 0.0)
            else:
                assert np.max(np.abs(Jv)) > 0 and not np.array_equal(Jq, Jc)
                if o.nq != o.nv:
                    assert np.array_equal(Jq[:, :3], Jc[:, :3]) and not np.array_equal(Jq[:, 3:6], Jc[:, 3:6])
        x = _state(o, rng)
        for bad in (-1e-3, np.nan, np.inf, -np.inf):
            with pytest.raises(capi.DdpHipError) as exc:
                hd.capture_point(x[:o.nq], x[o.nq:], bad)
            assert exc.value.code == capi.E_ARG, bad


LIN_CASES = [("chain6", 2, None, ""), ("tree38", 2, None, ""), ("chain6ff", 2, 0, ""), ("tree38ff", 0, 0, "nt")]


def _lin_task(o, model, xs, B, T, seed):
    geom, w = random_task(o, model, xs, B, seed)
    w[1, :, 1::2] = 0.0                                  # instance 1: every live plane has tau = 0
    w[0, 1, 0] = 0.0; w[2, T, 3] = 0.0                   # single zero weights among the others
    w[2, 2, :] = 0.0                                     # one (instance, t) with all weights off
    for s_ in range(NP):                                 # one (instance, t) whose live planes are all clear: h moved to the free side
        X = xs[0].reshape(T + 1, o.nx)[3]
        geom[0, 3, s_, 3] = geom[0, 3, s_, :3] @ point(o, model, X, float(geom[0, 3, s_, 4])) - 0.05
    return geom, w


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_,flags", LIN_CASES)
@pytest.mark.parametrize("stages", [None, 1])
def test_linearize_matches_definition(gpu, name, fd_mode, fo_, flags, stages):
    """LX, LXX, LFX, LFXX against the flag-off values plus the definition's terms at TOL_LIN, batch 3 and T = 4 (15 (instance, t)
    pairs) with different planes and weights per instance, through ddp_hip_linearize and ddp_hip_linearize_stages(LIN_COST);
    LXX / LFXX symmetric bit for bit; LU, LUU and LUX bit for bit the flag-off values; instance 1, whose live planes all have
    tau = 0, keeps the flag-off bits in every v row and column; an (instance, t) whose weights are all 0 and one whose live planes
    are all clear keep the flag-off bits altogether; the device is not the yardstick without tau d cdot / dq"""
    capi = gpu
    T, B = 4, 3
    model, spec, o = make_any(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 41)
    xs = _moving(xs, o, 40)
    geom, w = _lin_task(o, model, xs, B, T, 42)
    act = check_task(o, model, [xs], geom, w)
    assert not act[0, 3].any() and not act[2, 2].any()
    base = capi.FLAG_NO_TENSORS if flags == "nt" else 0
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=base | (_on(capi) if on else 0)) as ctx:
            _setup(ctx, xs, us, tc._mults(o, xs[0], 43), o.Etot)
            if on:
                set_task(ctx, geom, w)
            ctx.linearize(None if stages is None else capi.LIN_COST)
            got[on] = {s: ctx.download(s) for s in DERIVS}
    n, nv = o.n, o.nv
    worst = 0.0
    for b in range(B):
        add = br_derivs(o, model, xs[b], geom[b], w[b])
        for s in ("LX", "LXX", "LFX", "LFXX"):
            ex = got[False][s][b] + add[s]
            assert np.max(np.abs(add[s])) > 0
            e = rel_err(got[True][s][b], ex)
            worst = max(worst, e)
            assert e <= TOL_LIN, (s, b, e)
        if b == 0:                                       # negative control: tau d cdot / dq is in the device's values
            noq = br_derivs(o, model, xs[b], geom[b], w[b], drop_q=True)
            assert rel_err(got[True]["LX"][b], got[False]["LX"][b] + noq["LX"]) > 1e-6
        for s in ("LU", "LUU", "LUX"):
            assert np.array_equal(got[True][s][b], got[False][s][b]), s
        for t in range(T + 1):
            key, k = ("LXX", t) if t < T else ("LFXX", 0)
            blk = got[True][key][b][k * n * n:(k + 1) * n * n].reshape(n, n)
            off = got[False][key][b][k * n * n:(k + 1) * n * n].reshape(n, n)
            assert np.array_equal(blk, blk.T)
            gk, go = ("LX", t) if t < T else ("LFX", 0)
            gon, goff = got[True][gk][b][go * n:(go + 1) * n], got[False][gk][b][go * n:(go + 1) * n]
            if not act[b, t].any():                      # nothing active: untouched
                assert np.array_equal(blk, off) and np.array_equal(gon, goff)
                continue
            assert not np.array_equal(blk[:nv, :nv], off[:nv, :nv]) and not np.array_equal(gon[:nv], goff[:nv])
            if not act[b, t, 1::2].any():                # every active plane has tau = 0: the v rows and columns are untouched
                assert np.array_equal(blk[nv:, :], off[nv:, :]) and np.array_equal(blk[:, nv:], off[:, nv:]) and np.array_equal(gon[nv:], goff[nv:])
            else:
                assert not np.array_equal(blk[nv:, nv:], off[nv:, nv:]) and not np.array_equal(gon[nv:], goff[nv:])
    assert not act[1, :, 1::2].any() and act[1].any() and act[0, :, 1::2].any()
    print("linearize", name, flags, stages, "worst", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_", [("tree38", 0, None), ("chain6ff", 0, 0), ("chain6", 2, None)])
def test_cost_seq_aug(gpu, name, fd_mode, fo_):
    """COSTS_OLD / COSTS_NEW (which = 0 / 1) against the oracle's augmented cost plus the numpy terms, lf included; a t without an
    active plane keeps the flag-off bits"""
    capi = gpu
    T, B, mu = 4, 3, 30.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 51)
    xs2, us2 = _trajs(o, model, B, 61)
    xs, xs2 = _moving(xs, o, 54), _moving(xs2, o, 64)
    geom, w = _lin_task(o, model, xs, B, T, 52)
    act = check_task(o, model, [xs, xs2], geom, w)
    mults = tc._mults(o, xs[0], 53)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | (_on(capi) if on else 0)) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
            if on:
                set_task(ctx, geom, w)
            ctx.cost_seq_aug(0, mu)
            ctx.cost_seq_aug(1, mu)
            got[on] = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
    for which, (X, U) in ((0, (xs, us)), (1, (xs2, us2))):
        for b in range(B):
            add = br_terms(o, model, X[b], geom[b], w[b])
            ex = o.cost_seq_aug(X[b], U[b], mults, mu) + add
            assert np.sum(add != 0.0) >= 2
            e = rel_err(got[True][which][b], ex)
            print("cost_seq_aug", name, which, b, e)
            assert e <= TOL_LIN, (which, b, e)
            assert np.array_equal(got[True][which][b][add == 0.0], got[False][which][b][add == 0.0])
    assert np.array_equal(got[True][0][0][3], got[False][0][0][3]) and not act[0, 3].any()


def _run(ctx, mu, with_stream):
    """fc._run_all (linearise, both costs, sweep, forward with 8 candidates), then a forward with one candidate per round"""
    r = fc._run_all(ctx, mu, with_stream)
    rc, step, dcost = ctx.forward(r["bwd"][2], n_alpha=1)
    r["fwd1"] = (rc, step, dcost)
    r["X_NEW1"], r["U_NEW1"] = ctx.download("X_NEW"), ctx.download("U_NEW")
    return r


def _far_task(o, model, xs, B, seed):
    """non-zero weights on planes 10 m on the free side of the tested points"""
    geom, w = random_task(o, model, xs, B, seed, wscale=50.0, p_clear=1.0)
    geom[..., 3] -= 10.0
    return geom, w


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,fd_mode,fo_,fwd_path", [("tree38", 8, 2, None, 1), ("chain6ff", 8, 2, 0, 0)])
@pytest.mark.parametrize("mode", ["nothing", "zero_weights", "far"])
def test_untouched_planes_change_nothing(gpu, name, T, fd_mode, fo_, fwd_path, mode):
    """flag on with nothing uploaded, with violated planes but every weight 0, and with non-zero weights on planes 10 m on the
    free side (the kernels run and find no active plane): linearise, both costs, sweep and forward (8 candidates and 1) are bit
    for bit what the flag-off context computes, on both forward paths"""
    capi = gpu
    mu, B = 10.0, 3
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 31, held=True)
    xs = _moving(xs, o, 34, sigma=0.1)
    mults = tc._mults(o, xs[0], 32)
    if mode == "far":
        geom, w = _far_task(o, model, xs, B, 33)
        assert np.min([br_margin(o, model, xs[b], geom[b], w[b]) for b in range(B)]) > 5.0
    else:
        geom, w = random_task(o, model, xs, B, 33, p_clear=0.0)
        w[:] = 0.0
    out = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_TRACE | (_on(capi) if on else 0)) as ctx:
            assert ctx.info()["fwd_path"] == fwd_path
            _setup(ctx, xs, us, mults, o.Etot)
            if on and mode != "nothing":
                set_task(ctx, geom, w)
            out[on] = _run(ctx, mu, name == "tree38")
            if on and mode == "far":
                assert np.min(ctx.balance_region_margin(1)) > 5.0         # the accepted candidate stayed clear as well
    fc._same(out[False], out[True])
    assert np.all(np.isfinite(out[True]["LX"])) and np.all(np.isfinite(out[True]["X_NEW"]))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["nothing", "zero_weights", "far"])
def test_solve_with_untouched_planes_changes_nothing(gpu, mode):
    """a short ddp_hip_solve in the three cases: the log and the result are bit for bit the flag-off solve's"""
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B, iters, thr, mu, w_, n_ = 6, 2, 3, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make("tree38", T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 101, held=True)
    geom, w = _far_task(o, model, xs, B, 102)
    if mode == "zero_weights":
        geom[..., 3] += 10.1
        w[:] = 0.0
    res = {}
    for on in (False, True):
        with capi.Context(spec, flags=_on(capi) if on else 0) as ctx:
            _setup(ctx, xs, us)
            if on and mode != "nothing":
                set_task(ctx, geom, w)
            log = solver.solve(ctx, iters, thr, mu, 0.0, w_, n_)
            res[on] = (log, ctx.download("X"), ctx.download("U"))
            if on and mode == "far":
                assert np.min(ctx.balance_region_margin(0)) > 5.0
    assert not np.array_equal(res[True][1], xs)
    assert np.array_equal(res[False][1], res[True][1]) and np.array_equal(res[False][2], res[True][2])
    for k in ("iterations", "mu", "reg", "w", "n", "last_step", "opt_obj", "opt_constr"):
        assert np.array_equal(np.asarray(res[False][0][k]), np.asarray(res[True][0][k])), k


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_", [("tree38", None), ("chain6ff", 0)])
def test_cross_term_identity(gpu, name, fo_):
    """one plane with tau = 0, n = e_x and h beyond the CoM at every (b, t): the term is 1/2 w (c_x - h)^2, what a
    DDP_HIP_FLAG_COM_COST context with weights (w, 0, 0) and target g_x = h forms.  LX, LXX, LFX, LFXX and the cost sequence agree
    to TOL_LIN (two traversals: not bit for bit)"""
    capi = gpu
    T, B, mu = 4, 3, 1.0
    model, spec, o = make(name, T, batch=B, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 131)
    xs = _moving(xs, o, 132)
    rng = np.random.default_rng(133)
    wt = rng.uniform(0.5, 5.0, size=(B, T + 1))
    geom, tgt, wc = np.zeros((B, T + 1, 1, 5)), np.zeros((B, T + 1, 3)), np.zeros((B, T + 1, 3))
    for b in range(B):
        X = xs[b].reshape(T + 1, o.nx)
        for t in range(T + 1):
            hx = cm.com(o, model, X[t][:o.nq])[0] + rng.uniform(0.02, 0.2)          # violated: c_x - h < 0
            geom[b, t, 0] = (1.0, 0.0, 0.0, hx, 0.0)
            tgt[b, t, 0], wc[b, t, 0] = hx, wt[b, t]
    act = check_task(o, model, [xs], geom, wt[..., None], fractions=False)
    assert act.all()
    got = {}
    for which in ("region", "com"):
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | (_on(capi) if which == "region" else capi.FLAG_COM_COST)) as ctx:
            _setup(ctx, xs, us)
            if which == "region":
                set_task(ctx, geom, wt[..., None], P=1)
            else:
                ctx.set_com_cost(target=tgt, weight=wc)
            ctx.linearize()
            got[which] = {s: ctx.download(s) for s in ("LX", "LXX", "LFX", "LFXX")}
            ctx.cost_seq_aug(0, mu)
            got[which]["COSTS_OLD"] = ctx.download("COSTS_OLD")
    for s in got["com"]:
        assert np.max(np.abs(got["com"][s])) > 0
        e = rel_err(got["region"][s], got["com"][s])
        print("cross", name, s, e)
        assert e <= TOL_LIN, (s, e)


def _fwd_problem(name, fo_, T=8):
    model, spec, o = make(name, T, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, 1, 81, held=True)
    xs = _moving(xs, o, 84, sigma=0.1)
    geom, w = random_task(o, model, xs, 1, 82, wscale=FWD_WSCALE)
    mults = tc._mults(o, xs[0], 85)
    return model, spec, o, xs, us, geom, w, mults


def _candidates(o, xs, us, mults, fb, mu, upto):
    """the rollouts at the steps 1, 1/2, .. 2^-upto: the line search's candidates up to and beyond the accepted one"""
    return [o.forward_alpha(2.0 ** -k, xs, us, mults, fb, mu)[1][None] for k in range(upto + 1)]


# planes violated by 1 .. 10 cm: a weight of some 1e3 makes the terms material beside c/2 |u|^2 of a held posture
FWD_WSCALE, FWD_KSCALE = 300.0, 3.0


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_,fwd_path", [("tree38", None, 1), ("chain6ff", 0, 0)])
@pytest.mark.parametrize("n_alpha", [1, 3, 8])
def test_forward_matches_emulation(gpu, name, fo_, fwd_path, n_alpha):
    """accepted step, dcost, X_NEW and U_NEW against Oracle.forward_alpha rollouts costed with numpy, the terms included, on the
    latency path (tree38) and the lane path (chain6ff); the feed-forward is scaled by 3 so that the halving runs.  On the
    emulation alone the test first asserts that every candidate tried decides by more than 1e-9 of the sum of the cost terms'
    magnitudes and that no live plane of any candidate lies within 1e-6 of its point, and only then compares decisions"""
    capi = gpu
    mu = 1.0
    model, spec, o, xs, us, geom, w, mults = _fwd_problem(name, fo_)
    T = o.T
    check_task(o, model, [xs], geom, w)
    with capi.Context(spec, flags=_on(capi) | capi.FLAG_NO_TENSORS) as ctx:
        assert ctx.info()["fwd_path"] == fwd_path
        _setup(ctx, xs, us, mults, o.Etot)
        set_task(ctx, geom, w)
        ctx.linearize()
        _, _, mu_o, _ = ctx.backward(0.0, mu)
        ctx.upload("FB_VAL", FWD_KSCALE * ctx.download("FB_VAL"))
        fb = {"origin": ctx.download("FB_ORIGIN")[0], "val": ctx.download("FB_VAL")[0], "jac": ctx.download("FB_JAC")[0]}
        rc, step, dcost = ctx.forward(mu_o, n_alpha=n_alpha)
        xn, un = ctx.download("X_NEW")[0], ctx.download("U_NEW")[0]
        marg = ctx.balance_region_margin(1)[0]

    def cost(X, U):
        return o.cost_seq_aug(X, U, mults, mu_o[0]) + br_terms(o, model, X, geom[0], w[0])
    em = cm._emulate_forward(o, xs[0], us[0], mults, fb, mu_o[0], n_alpha, cost)
    assert em is not None
    step_ref, xn_ref, un_ref, new, margins = em
    tried = len(margins)
    # every candidate a round of n_alpha evaluates, beyond the accepted one too
    upto = min(33, ((tried - 1) // n_alpha + 1) * n_alpha - 1)
    check_task(o, model, _candidates(o, xs[0], us[0], mults, fb, mu_o[0], upto), geom, w, fractions=False)
    share = br_terms(o, model, xn_ref, geom[0], w[0]).sum() / np.sum(np.abs(cost(xn_ref, un_ref)))
    print("forward", name, n_alpha, "step", step[0], step_ref, "dcost", dcost[0], new, "margins", margins, "share", share)
    assert share > 1e-6                                  # the terms are material in the candidate's cost
    assert tried > 1                                     # the halving ran
    assert min(margins) > 1e-9, margins
    assert step[0] == step_ref, (step, step_ref)
    assert abs(dcost[0] - new) <= TOL_FWD * max(1.0, abs(new)), (dcost[0], new)
    assert rel_err(xn, xn_ref) < TOL_FWD and rel_err(un, un_ref) < TOL_FWD
    assert rel_err(marg, br_margin(o, model, xn_ref, geom[0], w[0])) < TOL_FWD


@pytest.mark.gpu
def test_sweep_stepwise(gpu):
    """the backward sweep with the device's LX / LXX carrying the term (a non-zero value, all four blocks) against the oracle,
    tree38 at T = 4: restarts, mu and reg identical, every step redone alone by the oracle from the device's V(t+1) lands on the
    device's k_t, K_t, V_x(t), V_xx(t) to TOL_SWEEP (synth.stepwise_backward_check)"""
    from oracle.binding import Oracle
    capi = gpu
    name, T, mu = "tree38", 4, 1.0
    model, spec, o = make(name, T, fd_mode=2)
    xs, us = _trajs(o, model, 1, 71, held=True)
    xs = _moving(xs, o, 74, sigma=0.1)
    geom, w = random_task(o, model, xs, 1, 72, wscale=10.0)
    act = check_task(o, model, [xs], geom, w)
    mults = tc._mults(o, xs[0], 73)
    n = o.n
    with capi.Context(spec, flags=_on(capi) | capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        set_task(ctx, geom, w)
        ctx.linearize()
        rc, reg, mu_out, restarts = ctx.backward(0.0, mu)
        d = o.alloc_derivs()
        for k, s in NAMES.items():
            if ctx.seq_size(s):
                d[k][:ctx.seq_size(s)] = ctx.download(s)[0]
        add = br_derivs(o, model, xs[0], geom[0], w[0])
        assert np.max(np.abs(add["LX"])) > 0 and np.max(np.abs(add["LXX"].reshape(T, n, n)[:, o.nv:, :o.nv])) > 0 and act[0, :, 1::2].any()
        assert rel_err(d["lx"][:T * n], add["LX"]) <= TOL_LIN               # (c/2 |u|^2 has no lx: the term is all of it)
        ref_b = o.backward(d, xs[0], mults, 0.0, mu)
        print("sweep", name, "device restarts", int(restarts[0]), "oracle", ref_b["restarts"], "mu", mu_out[0], ref_b["mu"], "reg", reg[0], ref_b["reg"])
        assert int(restarts[0]) == ref_b["restarts"] and mu_out[0] == ref_b["mu"] and reg[0] == ref_b["reg"]
        got = {s: ctx.download(s)[0] for s in ("FB_JAC", "FB_VAL", "VX_TRACE", "VXX_TRACE")}
    assert np.max(np.abs(got["VX_TRACE"])) > 0 and not o.Etot

    def one_step_oracle(t):
        return Oracle(model, 1, dt=0.01, c=1.0, fd_mode=2)
    worst = stepwise_backward_check(one_step_oracle, o, d, xs[0], mults, reg[0], mu_out[0], got["VX_TRACE"], got["VXX_TRACE"],
                                    got["FB_VAL"], got["FB_JAC"], range(T))
    print("stepwise worst", worst)
    assert worst < TOL_SWEEP, worst


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,fo_,flags", [("chain6ff", 2, 0, 0), ("tree38", 0, 0, 1)])
def test_instances_are_independent(gpu, name, fd_mode, fo_, flags):
    """batch 3 through linearise, both costs, sweep, forward: instance 1 carries zero weights and equals the flag-off context's
    instance 1 bit for bit, whatever the others carry; and with instance 0's planes changed, instances 1 and 2 keep their bits"""
    capi = gpu
    T, B, mu = 4, 3, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 91, held=True)
    xs = _moving(xs, o, 93, sigma=0.1)
    geom, w = random_task(o, model, xs, B, 92, wscale=10.0)
    w[1] = 0.0
    geom2, w2 = geom.copy(), w.copy()
    geom2[0], w2[0] = random_task(o, model, xs[:1], 1, 94, wscale=30.0)
    out = []
    for g_, w_ in ((None, None), (geom, w), (geom2, w2)):
        with capi.Context(spec, flags=capi.FLAG_TRACE | flags | (_on(capi) if g_ is not None else 0)) as ctx:
            _setup(ctx, xs, us)
            if g_ is not None:
                set_task(ctx, g_, w_)
            out.append(fc._run_all(ctx, mu, False))
    off, a, b = out

    def pick(r, i):
        return {k: (tuple(np.asarray(v)[..., i] if np.ndim(v) else v for v in r[k]) if isinstance(r[k], tuple) else r[k][i]) for k in r}
    assert not np.array_equal(a["LX"][0], off["LX"][0]) and not np.array_equal(a["LX"][0], b["LX"][0])
    assert not np.array_equal(a["COSTS_OLD"][2], off["COSTS_OLD"][2])
    fc._same(pick(off, 1), pick(a, 1))
    fc._same(pick(a, 1), pick(b, 1))
    fc._same(pick(a, 2), pick(b, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("name,fd_mode,flags", [("chain6", 2, 0), ("tree38", 0, 1)])
def test_solve_matches_stepwise(gpu, name, fd_mode, flags):
    from ddp_pinocchio_amd import solver
    capi = gpu
    T, B, iters, thr, mu, w_, n_ = 6, 2, 4, 1e-9, 1e2, 1e-1, 10.0
    model, spec, o = make(name, T, batch=B, fd_mode=fd_mode)
    xs, us = _trajs(o, model, B, 101, held=True)
    xs = _moving(xs, o, 104, sigma=0.1)
    geom, w = random_task(o, model, xs, B, 102, wscale=30.0)
    mults = tc._mults(o, xs[0], 103)

    def run(stepwise, on=True):
        with capi.Context(spec, flags=flags | (_on(capi) if on else 0)) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if o.Etot:
                ctx.upload("MULT_ORIGIN", xs[:, :T * o.nx])
            if on:
                set_task(ctx, geom, w)
            log = (solver.solve_stepwise if stepwise else solver.solve)(ctx, iters, thr, mu, 0.0, w_, n_)
            return log, ctx.download("X"), ctx.download("U")
    la, xa, ua = run(False)
    lb, xb, ub = run(True)
    assert np.all(np.isfinite(xa))
    assert not np.array_equal(xa, xs) and not np.array_equal(xa, run(False, on=False)[1])
    assert np.array_equal(xa, xb) and np.array_equal(ua, ub)
    for k in ("iterations", "mu", "reg", "w", "n", "last_step", "opt_obj", "opt_constr"):
        assert np.array_equal(np.asarray(la[k]), np.asarray(lb[k])), k


@pytest.mark.gpu
def test_combination_and_order(gpu):
    """tracking, CoM, momentum, balance regions and obstacles live together on tree38.  The position of the additions, bit for
    bit: a context with the balance regions alone (or the obstacles alone) leaves exactly the term's own sums in LX / LXX -- the
    stage cost c/2 |u|^2 has none -- so with A = tracking + CoM + momentum, the context A + regions must hold fl(A + regions'
    sums) (after the momentum's) and the context A + regions + obstacles fl(that + the obstacles' sums) (before the obstacles');
    an implementation that added the regions after the obstacles would round differently.  The cost sequence with everything
    live against the yardsticks' sum at TOL_LIN"""
    capi = gpu
    T, B, mu = 4, 3, 1.0
    model, spec, o = make("tree38", T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 141)
    xs = _moving(xs, o, 142)
    geom, w = random_task(o, model, xs, B, 143, wscale=3.0)
    check_task(o, model, [xs], geom, w)
    ref = tc.random_ref(o, model, xs, us, B, 144)
    ctask = cm.random_task(o, model, xs, B, 145)
    mtask = mo.random_task(o, model, xs, B, 146)
    pts = ob.pick_points(model)
    og, ow = ob.random_task(o, pts, ob.KINDS, xs, B, 147)
    A = capi.FLAG_TRACKING_COST | capi.FLAG_COM_COST | capi.FLAG_MOMENTUM_COST
    seqs = ("LX", "LXX", "LFX", "LFXX")
    got = {}
    for key, flags in (("region", _on(capi)), ("obstacle", capi.FLAG_OBSTACLE_COST), ("A", A), ("A+r", A | _on(capi)),
                       ("A+r+o", A | _on(capi) | capi.FLAG_OBSTACLE_COST)):
        with capi.Context(spec, flags=flags | capi.FLAG_NO_TENSORS) as ctx:
            _setup(ctx, xs, us)
            if flags & A:
                tc.upload_ref(ctx, ref)
                ctx.set_com_cost(target=ctask[0], weight=ctask[1])
                ctx.set_momentum_cost(target=mtask[0], weight=mtask[1])
            if flags & _on(capi):
                set_task(ctx, geom, w)
            if flags & capi.FLAG_OBSTACLE_COST:
                ob.set_task(ctx, pts, ob.KINDS, og, ow)
            ctx.linearize()
            got[key] = {s: ctx.download(s) for s in seqs}
            ctx.cost_seq_aug(0, mu)
            got[key]["COSTS_OLD"] = ctx.download("COSTS_OLD")
    for s in seqs:
        assert np.max(np.abs(got["region"][s])) > 0 and np.max(np.abs(got["obstacle"][s])) > 0
        for b in range(B):                               # the lone contexts hold the terms' own sums
            assert rel_err(got["region"][s][b], br_derivs(o, model, xs[b], geom[b], w[b])[s]) <= TOL_LIN
        assert np.array_equal(got["A+r"][s], got["A"][s] + got["region"][s]), s
        assert np.array_equal(got["A+r+o"][s], got["A+r"][s] + got["obstacle"][s]), s
        assert not np.array_equal(got["A+r+o"][s], (got["A"][s] + got["obstacle"][s]) + got["region"][s]), s   # the other order rounds differently somewhere
    mults = tc._mults(o, xs[0], 148)
    for b in range(B):
        ex = (o.cost_seq_aug(xs[b], us[b], mults, mu) + tc.track_terms(o, 1.0, xs[b], us[b], ref, b) + cm.com_terms(o, model, xs[b], ctask[0][b], ctask[1][b])
              + mo.mom_terms(o, model, xs[b], mtask[0][b], mtask[1][b]) + br_terms(o, model, xs[b], geom[b], w[b])
              + ob.ob_terms(o, pts, ob.KINDS, xs[b], og[b], ow[b]))
        e = rel_err(got["A+r+o"]["COSTS_OLD"][b], ex)
        assert e <= TOL_LIN, (b, e)


@pytest.mark.gpu
@pytest.mark.parametrize("name,fo_", [("tree38", None), ("chain6ff", 0), ("table7", None)])
def test_margin(gpu, name, fo_):
    """ddp_hip_balance_region_margin against the yardstick to TOL_LIN along X, +inf where no plane is live, E_ARG before
    set_planes with a plane, +inf everywhere before any weight is live, and which = 1 along X_NEW after a forward"""
    capi = gpu
    T, B, mu = 4, 3, 10.0
    model, spec, o = make_any(name, T, batch=B, fd_mode=0, first_order_fd=fo_)
    xs, us = _trajs(o, model, B, 121, held=name != "table7")
    xs = _moving(xs, o, 122, sigma=0.1)
    geom, w = random_task(o, model, xs, B, 124, wscale=10.0, p_clear=0.85)     # (six planes each: mostly clear, so that some minima are positive)
    w[1, 2, :] = 0.0; w[2, T, :] = 0.0; w[0, 1, 1] = 0.0
    check_task(o, model, [xs], geom, w, fractions=False)
    with capi.Context(spec, flags=_on(capi) | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        for n0 in (None, 0):
            if n0 is not None:
                ctx.set_balance_region_planes(n0)
            with pytest.raises(capi.DdpHipError) as exc:
                ctx.balance_region_margin(0)
            assert exc.value.code == capi.E_ARG
        ctx.set_balance_region_planes(NP)
        assert np.all(ctx.balance_region_margin(0) == np.inf)             # planes set, no live weight
        ctx.set_balance_region_cost(geom=geom, weight=w)
        got = ctx.balance_region_margin(0)
        ex = np.stack([br_margin(o, model, xs[b], geom[b], w[b]) for b in range(B)])
        assert got[1, 2] == np.inf and got[2, T] == np.inf and np.array_equal(np.isinf(got), np.isinf(ex))
        fin = np.isfinite(ex)
        assert np.min(ex[fin]) < 0 < np.max(ex[fin])
        e = np.max(np.abs(got[fin] - ex[fin]) / np.maximum(1.0, np.abs(ex[fin])))
        print("margin", name, e)
        assert e <= TOL_LIN, e
        ctx.linearize()
        _, _, mu_o, _ = ctx.backward(0.0, mu)
        ctx.forward(mu_o, n_alpha=8)
        xn = ctx.download("X_NEW")
        got1 = ctx.balance_region_margin(1)
        ex1 = np.stack([br_margin(o, model, xn[b], geom[b], w[b]) for b in range(B)])
        assert np.array_equal(np.isinf(got1), np.isinf(ex1))
        e1 = np.max(np.abs(got1[fin] - ex1[fin]) / np.maximum(1.0, np.abs(ex1[fin])))
        assert e1 <= TOL_FWD, e1                          # (X_NEW is the device's own rollout: the states agree, the margin with them)
        assert np.array_equal(ctx.balance_region_margin(0), got)          # X is where it was


@pytest.mark.gpu
def test_margin_keeps_nan(gpu):
    """a NaN velocity at one (instance, t): the margin there is NaN where a live plane has tau != 0 -- whichever slot it has, the
    finite planes folded after it -- and finite where every live plane has tau = 0 (no velocity quantity is read); the term
    follows: NaN in the cost sequence there, and only there"""
    capi = gpu
    T, B = 2, 2
    model, spec, o = make("tree38", T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 151)
    geom, w = random_task(o, model, xs, B, 152)
    w[1, :, 1::2] = 0.0                                  # instance 1: tau = 0 alone
    bad = xs.copy()
    bad[:, 1 * o.nx + o.nq + 3] = np.nan
    with capi.Context(spec, flags=_on(capi) | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, bad, us)
        set_task(ctx, geom, w)
        got = ctx.balance_region_margin(0)
        ctx.cost_seq_aug(0, 1.0)
        costs = ctx.download("COSTS_OLD")
    ex = np.stack([br_margin(o, model, xs[b], geom[b], w[b]) for b in range(B)])
    assert np.isnan(got[0, 1]) and np.all(np.isfinite(got[0, [0, 2]])) and np.all(np.isfinite(got[1]))
    assert rel_err(got[0, [0, 2]], ex[0, [0, 2]]) <= TOL_LIN and rel_err(got[1], ex[1]) <= TOL_LIN
    assert np.isnan(costs[0, 1]) and np.all(np.isfinite(costs[0, [0, 2]])) and np.all(np.isfinite(costs[1]))


@pytest.mark.gpu
def test_refusals_and_defaults(gpu):
    import ctypes as C
    capi = gpu
    T, B, P = 3, 3, 4
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    L = capi.lib()
    dp = C.POINTER(C.c_double)

    def code(fn):
        with pytest.raises(capi.DdpHipError) as exc:
            fn()
        return exc.value.code

    def raw_upload(ctx, g, w_, first=0, count=B):
        return L.ddp_hip_balance_region_upload(ctx._h, g.ctypes.data_as(dp) if g is not None else None,
                                               w_.ctypes.data_as(dp) if w_ is not None else None, first, count)
    z = np.zeros(1)
    with capi.Context(spec) as ctx:                                   # a context without the flag
        assert code(lambda: ctx.set_balance_region_planes(2)) == capi.E_UNSUPPORTED
        assert raw_upload(ctx, z, z) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.get_balance_region_cost()) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.balance_region_margin(0)) == capi.E_UNSUPPORTED
    pend = capi.BuiltinModel(capi.BUILTIN_PENDULUM)
    with pytest.raises(capi.DdpHipError) as exc:
        capi.Context(capi.ProblemSpec(pend, T, fd_mode=2), flags=_on(capi))
    assert exc.value.code == capi.E_UNSUPPORTED
    massless = cm.table_model()
    massless = capi.TableModel(massless.parent, massless.jtype, massless.axis, massless.Rp, massless.pp, 0.0 * massless.mass_j,
                               massless.com, massless.Ic)
    with pytest.raises(capi.DdpHipError) as exc:                      # M <= 0
        capi.Context(capi.ProblemSpec(massless, T, fd_mode=2, first_order_fd=1), flags=_on(capi))
    assert exc.value.code == capi.E_ARG
    with capi.Context(spec, flags=_on(capi)) as ctx:                  # the flag stands alone
        g0, w0 = ctx.get_balance_region_cost()                        # create: no planes, empty arrays
        assert g0.shape == (B, T + 1, 0, 5) and w0.shape == (B, T + 1, 0)
        big = np.zeros(B * (T + 1) * 8 * 5)
        assert raw_upload(ctx, big, big) == capi.E_ARG                # an upload before set_planes
        for bad in (-1, 9):
            assert code(lambda: ctx.set_balance_region_planes(bad)) == capi.E_ARG
        ctx.set_balance_region_planes(0)
        assert raw_upload(ctx, big, big) == capi.E_ARG                # ... and with a count of 0
        ctx.set_balance_region_planes(P)
        g0, w0 = ctx.get_balance_region_cost()                        # a download after set_planes: zeros
        assert g0.shape == (B, T + 1, P, 5) and np.all(g0 == 0.0) and np.all(w0 == 0.0)
        rng = np.random.default_rng(5)
        gg = np.zeros((B, T + 1, P, 5))
        gg[..., :3] = rng.normal(size=(B, T + 1, P, 3)); gg[..., :3] /= np.linalg.norm(gg[..., :3], axis=-1, keepdims=True)
        gg[..., 3] = rng.normal(size=(B, T + 1, P)); gg[..., 4] = rng.uniform(0, 0.5, size=(B, T + 1, P)); gg[:, :, 0, 4] = 0.0
        wg = rng.uniform(0, 1, size=(B, T + 1, P))
        ctx.set_balance_region_cost(geom=gg, weight=wg)
        for bad in (-1e-3, np.nan, np.inf):                           # a bad weight
            wb = np.ones((T + 1, P)); wb[1, 2] = bad
            assert code(lambda: ctx.set_balance_region_cost(weight=wb)) == capi.E_ARG, bad
            assert code(lambda: ctx.set_balance_region_cost(geom=gg[0], weight=wb)) == capi.E_ARG, bad
        for at, bad in ((0, np.nan), (3, np.inf), (4, np.nan), (4, -np.inf), (4, -1e-9), (1, 2.0)):
            gb = gg[0].copy(); gb[2, 1, at] = bad                     # a non-finite value, tau < 0, a normal off unit length
            assert code(lambda: ctx.set_balance_region_cost(geom=gb)) == capi.E_ARG, (at, bad)
            assert code(lambda: ctx.set_balance_region_cost(geom=gb, weight=wg[0])) == capi.E_ARG, (at, bad)
        gz = gg[0].copy(); gz[0, 0, :3] = 0.0                         # the zero vector is no normal
        assert code(lambda: ctx.set_balance_region_cost(geom=gz)) == capi.E_ARG
        assert code(lambda: ctx.set_balance_region_cost(weight=np.zeros(P), first=B, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_balance_region_cost(weight=np.zeros(P), first=-1, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_balance_region_cost(weight=np.zeros(P), first=1, count=B)) == capi.E_ARG
        assert code(lambda: ctx.get_balance_region_cost(first=1, count=B)) == capi.E_ARG
        for which in (-1, 2):
            assert code(lambda: ctx.balance_region_margin(which)) == capi.E_ARG
        g1, w1 = ctx.get_balance_region_cost()
        assert np.array_equal(g1, gg) and np.array_equal(w1, wg)        # a refused upload leaves both sides as they were
        ctx.set_balance_region_cost(weight=wg[1] + 1.0, first=1, count=1)   # one side, one instance; the geometry stays
        g1, w1 = ctx.get_balance_region_cost()
        assert np.array_equal(g1, gg) and np.array_equal(w1[1], wg[1] + 1.0) and np.array_equal(w1[[0, 2]], wg[[0, 2]])
        g2 = gg[2].copy(); g2[..., 3] += 1.0
        ctx.set_balance_region_cost(geom=g2, first=2, count=1)          # ... and the other side alone; the weights stay
        g3, w3 = ctx.get_balance_region_cost(first=1, count=2)          # the round trip of a range of instances
        assert np.array_equal(g3[0], gg[1]) and np.array_equal(g3[1], g2) and np.array_equal(w3, w1[1:])
        ctx.set_balance_region_cost(geom=gg[0, 0], weight=wg[0, 0])     # broadcast: (P, 5) and (P,)
        assert np.array_equal(ctx.get_balance_region_cost()[0], np.broadcast_to(gg[0, 0], (B, T + 1, P, 5)))
        assert np.array_equal(ctx.get_balance_region_cost()[1], np.broadcast_to(wg[0, 0], (B, T + 1, P)))
        ctx.set_balance_region_planes(P)                                # the same count keeps the data
        assert np.array_equal(ctx.get_balance_region_cost()[1], np.broadcast_to(wg[0, 0], (B, T + 1, P)))
        ctx.set_balance_region_planes(P - 1)                            # another count resets it
        g4, w4 = ctx.get_balance_region_cost()
        assert g4.shape == (B, T + 1, P - 1, 5) and np.all(g4 == 0.0) and np.all(w4 == 0.0)
        assert np.all(ctx.balance_region_margin(0) == np.inf)
        ctx.set_balance_region_planes(0)                                # 0 takes the planes away
        assert code(lambda: ctx.balance_region_margin(0)) == capi.E_ARG


def _balance_task(capi, T, weight, iters, mu=1.0):
    """tree38 from a held posture, the 6 cm box 5 cm ahead of the CoM and the hand pulled back: (costs per iteration, steps, the
    margins at the start, at the end, the yardstick's at the start)"""
    model, spec, o = make("tree38", T, fd_mode=0)
    xs, us = _trajs(o, model, 1, 161, held=True)
    X0 = xs[0].reshape(T + 1, o.nx)[0]
    centre = cm.com(o, model, X0[:o.nq]) + np.array([0.05, 0.0, 0.0])
    planes = [((1.0, 0.0, 0.0), 0.0), ((-1.0, 0.0, 0.0), 0.0), ((0.0, 1.0, 0.0), 0.3), ((0.0, -1.0, 0.0), 0.3)]
    geom = np.array([list(n) + [np.dot(n, centre) - 0.03, tau] for n, tau in planes])      # inside: n . (xi - centre) >= -3 cm
    w = np.full(4, weight)
    frames = fc.pick_frames(model, 3)[2:3]                                                 # a leaf: the hand
    p0 = o.frame_position(frames[0][0], np.asarray(frames[0][1]), X0[:o.nq])
    ftgt = np.broadcast_to(p0 + np.array([-0.15, 0.0, 0.0]), (T + 1, 1, 3))
    with capi.Context(spec, flags=_on(capi) | capi.FLAG_FRAME_COST | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        ctx.set_frame_cost(frames=frames, target=ftgt, weight=50.0)
        set_task(ctx, geom, w, P=4)
        start = ctx.balance_region_margin(0)[0]
        costs, steps = [], []
        for _ in range(iters):
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            rc, step, dcost = ctx.forward(mu_o, n_alpha=8)
            costs.append(ctx.download("COSTS_OLD")[0].sum())
            steps.append(step[0])
            ctx.swap_traj()
        end = ctx.balance_region_margin(0)[0]
    ex = br_margin(o, model, xs[0], np.broadcast_to(geom, (T + 1, 4, 5)), np.broadcast_to(w, (T + 1, 4)))
    return costs, steps, start, end, ex


TASK_T, TASK_WEIGHT, TASK_ITERS = 20, 1e6, 8     # (weights of 1e5 and less leave the fall of c/2 |u|^2 in charge: the CoM moves by a millimetre)


@pytest.mark.gpu
def test_balance_task(gpu):
    """A task that means something: tree38 from a held posture, four vertical planes (n_z = 0) making a 6 cm box whose centre is
    5 cm from the present CoM -- two opposite slots test the CoM (tau = 0), the other two the capture point (tau = 0.3) -- and a
    hand frame cost pulling the other way.  The start violates the box by 2 cm.  After a bounded number of solve iterations the
    least margin over t >= T / 2 is greater than at the start, and the cost never increases from one iteration to the next"""
    T = TASK_T
    costs, steps, start, end, ex = _balance_task(gpu, T, TASK_WEIGHT, TASK_ITERS)
    print("balance task costs", costs, "steps", steps, "margin", start[T // 2:].min(), "->", end[T // 2:].min())
    assert rel_err(start, ex) <= TOL_LIN
    assert -0.021 < start[T // 2:].min() < -0.019                                           # the start is 2 cm outside
    for a, b in zip(costs, costs[1:]):
        assert b <= a * (1 + 1e-12), costs
    assert costs[-1] < costs[0]
    assert end[T // 2:].min() > start[T // 2:].min(), (start, end)
