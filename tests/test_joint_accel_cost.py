"""Per-instance joint-acceleration costs (DDP_HIP_FLAG_JOINT_ACCEL_COST, ddp_hip.h):
    a = aba(q_t, v_t, u_t),   r = a - a_ref[b][t],   l(t, x, u) += 1/2 sum_i w_i r_i^2   (t < T; nothing at T)
with the Gauss-Newton blocks Z^T W Z, Z = [da/d(delta q) | da/dv | M^-1] over the rows of weight != 0.  The yardstick is the
oracle: o.aba and o.aba_derivatives, the products in numpy.  Shapes are the smallest at which a joint mix-up, a root-row slip, a T
against T+1 stride error and a candidate-index error show: T = 3 or 4, B = 2 or 3, on the five models of the neighbours' tests."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import test_balance_region_cost as br
import test_com_cost as cm
import test_control_grav_cost as cg
import test_frame_aim_cost as fa
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
MODELS = ["chain6", "chain6ff", "table7", "tree38", "tree38ff"]
ADDS = ("LX", "LXX", "LU", "LUU", "LUX")
make_any = cm.make_any
_trajs, _setup = tc._trajs, tc._setup
_emulate_forward = cm._emulate_forward
# everything that passes through M^-1 is held to 1e-10 * scale against the oracle (test_analytic_derivs.py); values to the 1e-12 the
# ABA itself is held to (test_model_point_evaluations); the line search to the neighbours' 1e-9
TOL_LIN, TOL_ABA, TOL_FWD, TOL_SWEEP = 1e-10, 1e-12, 1e-9, 1e-10


# ---- the yardstick ---------------------------------------------------------------------------------------------------------
def accel(o, x, u):
    return o.aba(x[:o.nq], x[o.nq:], u)


def ja_accels(o, xs, us):
    X, U = xs.reshape(o.T + 1, o.nx), us.reshape(o.T, o.m)
    return np.stack([accel(o, X[t], U[t]) for t in range(o.T)])


def ja_terms(o, xs, us, aref, w, bound=False):
    """(T+1,): 1/2 sum_i w_i (a_i - aref_i)^2 over the rows of weight != 0, 0 at T; bound: 1/2 sum_i w_i (|a_i| + |aref_i|)^2"""
    A = ja_accels(o, xs, us)
    out = np.zeros(o.T + 1)
    for t in range(o.T):
        live = w[t] != 0.0
        r = (np.abs(A[t]) + np.abs(aref[t])) if bound else (A[t] - aref[t])
        out[t] = 0.5 * np.sum(w[t][live] * r[live] ** 2)
    return out


class Jacobians:
    """Z = (da/d(delta q), da/dv, da/du) at a point.  Fixed base: o.aba_derivatives.  The oracle's analytic recursion covers trees
    of 1-DoF joints alone (oracle/ddp_oracle.c: a free-flyer model's first order is differenced there), so on a free-flyer root
    the jacobians are the library's ddp_hip_model_aba_derivatives (an entry point from before this term, run on the device), which
    check_against_oracle holds to the 5-point central difference of o.aba through o.integrate"""

    def __init__(self, capi, model, o):
        self.o, self.hd = o, capi.ModelHandle(model) if model.ff else None

    def __call__(self, q, v, u):
        return self.hd.aba_derivatives(q, v, u) if self.hd else self.o.aba_derivatives(q, v, u)

    def close(self):
        if self.hd:
            self.hd.close()


W5 = ((-2, 1.0 / 12), (-1, -8.0 / 12), (1, 8.0 / 12), (2, -1.0 / 12))


def fd_jacobians(o, q, v, u):
    """the 5-point central difference of o.aba through o.integrate, H = 1e-3: (nv, 3 nv)"""
    nv = o.nv
    fd = np.zeros((nv, 3 * nv))
    for j in range(nv):
        e = np.zeros(nv); e[j] = H
        fd[:, j] = sum(cw * o.aba(o.integrate(q, s * e), v, u) for s, cw in W5) / H
        fd[:, nv + j] = sum(cw * o.aba(q, v + s * e, u) for s, cw in W5) / H
        fd[:, 2 * nv + j] = sum(cw * o.aba(q, v, u + s * e) for s, cw in W5) / H
    return fd


def check_against_oracle(zfun, o, x, u, what):
    q, v = x[:o.nq], x[o.nq:]
    Z = np.hstack(zfun(q, v, u))
    err, scale = np.max(np.abs(fd_jacobians(o, q, v, u) - Z)), max(1.0, np.max(np.abs(Z)))
    print("yardstick", what, "max|Z|", np.max(np.abs(Z)), "err", err, "max|v|", np.max(np.abs(v)))
    assert np.max(np.abs(v)) > 0 and np.max(np.abs(Z[:, :o.nv])) > 0
    assert err <= 1e-8 * scale, (what, err, scale)


def ja_derivs(o, xs, us, aref, w, zfun=None):
    """the five additions per t < T, column-major, concatenated over t like the device's sequences"""
    zfun = zfun or o.aba_derivatives
    X, U = xs.reshape(o.T + 1, o.nx), us.reshape(o.T, o.m)
    out = {s: [] for s in ADDS}
    for t in range(o.T):
        q, v = X[t][:o.nq], X[t][o.nq:]
        live = w[t] != 0.0
        Zq, Zv, Zu = zfun(q, v, U[t])
        Zx, Zu, wl = np.hstack([Zq, Zv])[live], Zu[live], w[t][live]
        wr = wl * (o.aba(q, v, U[t]) - aref[t])[live]
        blocks = {"LX": Zx.T @ wr, "LU": Zu.T @ wr, "LXX": Zx.T @ (wl[:, None] * Zx), "LUU": Zu.T @ (wl[:, None] * Zu),
                  "LUX": Zu.T @ (wl[:, None] * Zx)}
        for s in ADDS:
            out[s].append(np.asarray(blocks[s]).ravel(order="F"))
    return {s: np.concatenate(v) for s, v in out.items()}


def random_task(o, xs, us, B, seed, wscale=1.0, spread=1.0):
    """targets about the present accelerations (B, T, nv) and weights in [0.1, 2] wscale"""
    rng = np.random.default_rng(seed)
    A = np.stack([ja_accels(o, xs[b], us[b]) for b in range(B)])
    aref = A + spread * np.maximum(1.0, np.abs(A)) * rng.normal(size=A.shape)
    w = wscale * rng.uniform(0.1, 2.0, size=A.shape)
    return aref, w


def FLAG(capi):
    return capi.FLAG_JOINT_ACCEL_COST


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_interface_constants():
    from ddp_pinocchio_amd import capi
    header = open(os.path.join(ROOT, "include", "ddp_hip", "ddp_hip.h")).read()
    assert capi.FLAG_JOINT_ACCEL_COST == 65536 and re.search(r"#define\s+DDP_HIP_FLAG_JOINT_ACCEL_COST\s+65536u", header)
    L = capi.lib()
    for name in ("ddp_hip_joint_accel_cost_upload", "ddp_hip_joint_accel_cost_download", "ddp_hip_joint_accel"):
        assert name in capi.EXPORTS and re.search(r"\b" + name + r"\s*\(", header) and hasattr(L, name), name
    assert L.ddp_hip_abi_version() == 3 and re.search(r"#define\s+DDP_HIP_ABI_VERSION\s+3\b", header)
    assert len(capi.SEQ_NAMES) == 40
    for name in ("set_joint_accel_cost", "joint_accel_cost", "joint_accel"):
        assert hasattr(capi.Context, name), name
    # shapes are checked before anything reaches the library: a context object without a device will do.  The public shape is
    # (T, nv): a (T+1, nv) array is refused, a (T, nv) one passes the wrapper (and only then meets the missing handle)
    T, B = 5, 2
    model, spec, _ = make("chain6", T, batch=B, fd_mode=0)
    ctx = capi.Context.__new__(capi.Context)
    ctx.spec, ctx.batch, ctx._h = spec, B, None
    for kw in (dict(target=np.zeros((T + 1, 6))), dict(target=np.zeros(5)), dict(target=np.zeros((B + 1, T, 6))),
               dict(weight=np.zeros((T + 1, 6))), dict(weight=np.zeros(3)), dict(weight=np.zeros((B, T, 6)), count=1),
               dict(target=np.zeros((T, 6)), weight=np.zeros((T, 5)))):
        with pytest.raises(ValueError):
            ctx.set_joint_accel_cost(**kw)
    count, arrs = ctx._cost_sides("set_joint_accel_cost", (("target", np.zeros((T, 6)), (T, 6), ((6,), ())), ("weight", np.ones(6), (T, 6), ((6,), ()))), 1, 1)
    assert count == 1 and arrs[0].shape == (1, T, 6) and arrs[1].shape == (1, T, 6)
    ctx.set_joint_accel_cost()                            # no side: no call, and (T, nv) passes the shape check above


def test_host_block():
    """host/test_joint_accel_block.cpp: the record (2 sides, nv items, T+1 rows, not stage_only), the enumerator's position and
    the neighbours' adjacencies, the validators with the rule for row T, a free-flyer root's rows, the live rule"""
    host = os.path.join(ROOT, "host")
    subprocess.run(["make", "-C", host, "test_joint_accel_block"], check=True, capture_output=True)
    run = subprocess.run([os.path.join(host, "test_joint_accel_block")], capture_output=True, text=True)
    assert run.returncode == 0 and "all checks passed" in run.stdout, run.stdout + run.stderr


@pytest.mark.parametrize("name", [n for n in MODELS if not n.endswith("ff")])
def test_yardstick_pins(name):
    """o.aba_derivatives against the 5-point central difference of o.aba through o.integrate (H = 1e-3) at states of the
    generators' scale, 1e-8 max(1, |Z|) like the neighbours' yardstick checks, da/du included.  The fixed-base models: the
    oracle has no analytic jacobian for a free-flyer root (Jacobians; test_linearize_matches_definition holds that yardstick to
    the same difference).  A check of the oracle alone: it calls nothing of the library's new code"""
    model, _, o = make_any(name, 3, fd_mode=0)
    xs, us = _trajs(o, model, 1, 7)
    X, U = xs[0].reshape(o.T + 1, o.nx), us[0].reshape(o.T, o.m)
    for t in (1, 2):
        check_against_oracle(o.aba_derivatives, o, X[t], U[t], (name, t))


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _lin_task(o, xs, us, B, T):
    aref, w = random_task(o, xs, us, B, 42)
    w[1] = 0.0                                            # one instance with all weights 0
    w[0, 1, 1] = 0.0; w[0, 2, o.nv - 1] = 0.0; w[2, 0, 0] = 0.0; w[2, 1, ::2] = 0.0   # a sprinkling of zero-weight rows
    w[2, 2, :] = 0.0; w[2, 2, min(7, o.nv - 2)] = 0.7     # one (instance, t) with a single live row
    w[0, T - 1, :] = 0.0                                  # one (instance, t) without a weight among live ones
    return aref, w


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_linearize_matches_definition(gpu, name):
    """LX, LXX, LU, LUU, LUX after linearize against the flag-off values plus the numpy products of the oracle's jacobians at
    1e-10 * scale (TOL_LIN: what the project holds everything that passes through M^-1 to); every other sequence bit for bit the
    flag-off one; the additions to LXX and LUU symmetric bit for bit; the instance and the (instance, t) whose weights are all
    0 bit for bit flag-off; with first_order_fd 0 and 1 the five sequences are the same bits (the term is analytic whatever
    FX / FU are formed by).  [measured on an MI355X: see DESIGN.md section 4z]"""
    capi = gpu
    T, B = 4, 3
    got = {}
    for fo_ in (0, 1):
        model, spec, o = make_any(name, T, batch=B, fd_mode=0, first_order_fd=fo_)
        xs, us = _trajs(o, model, B, 41)
        aref, w = _lin_task(o, xs, us, B, T)
        mults = tc._mults(o, xs[0], 43)
        for on in (False, True):
            with capi.Context(spec, flags=FLAG(capi) if on else 0) as ctx:
                _setup(ctx, xs, us, mults, o.Etot)
                if on:
                    ctx.set_joint_accel_cost(target=aref, weight=w)
                ctx.linearize()
                got[fo_, on] = {s: ctx.download(s) for s in DERIVS if ctx.seq_size(s)}
    n, m = o.n, o.m
    worst = {s: 0.0 for s in ADDS}
    zfun = Jacobians(capi, model, o)
    if model.ff:
        check_against_oracle(zfun, o, xs[0].reshape(T + 1, o.nx)[1], us[0].reshape(T, m)[1], name)
    adds = [ja_derivs(o, xs[b], us[b], aref[b], w[b], zfun) for b in range(B)]
    zfun.close()
    for fo_ in (0, 1):
        on, off = got[fo_, True], got[fo_, False]
        for s in on:
            if s not in ADDS:
                assert np.array_equal(on[s], off[s]), s
        for b in range(B):
            add = adds[b]
            for s in ADDS:
                if b == 1:
                    assert np.array_equal(on[s][b], off[s][b]), s       # the instance whose weights are all 0
                    continue
                assert np.max(np.abs(add[s])) > 0
                e = rel_err(on[s][b], off[s][b] + add[s])
                worst[s] = max(worst[s], e)
                assert e <= TOL_LIN, (s, b, fo_, e)
            for t in range(T):
                dxx = (on["LXX"][b] - off["LXX"][b])[t * n * n:(t + 1) * n * n].reshape(n, n)
                duu = (on["LUU"][b] - off["LUU"][b])[t * m * m:(t + 1) * m * m].reshape(m, m)
                assert np.array_equal(dxx, dxx.T) and np.array_equal(duu, duu.T)
                if not np.any(w[b, t]):
                    for s, sz in (("LU", m), ("LUU", m * m), ("LUX", m * n), ("LX", n), ("LXX", n * n)):
                        assert np.array_equal(on[s][b][t * sz:(t + 1) * sz], off[s][b][t * sz:(t + 1) * sz]), (s, b, t)
                else:
                    assert np.any(dxx != 0.0) and np.any(duu != 0.0)
    for s in ADDS:
        assert np.array_equal(got[0, True][s], got[1, True][s]), s
    print("linearize", name, "worst", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_cost_values(gpu, name):
    """ddp_hip_cost_seq_aug (which 0 and 1: X with U, X_NEW with U_NEW, trajectories that are no rollouts of their controls) minus
    the flag-off values against 1/2 sum w (o.aba - a_ref)^2, per t within 1e-12 * 1/2 sum w (|a| + |a_ref|)^2 (the bound the ABA is
    held to, through the square) plus the rounding of the sum the term is added to; the entry at T is exactly the flag-off one"""
    capi = gpu
    T, B, mu = 4, 3, 30.0
    model, spec, o = make_any(name, T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 51)
    xs2, us2 = _trajs(o, model, B, 61)
    us2 = us2[::-1].copy()                                # (X_NEW is not the rollout of U_NEW)
    aref, w = random_task(o, xs, us, B, 52)
    w[1, 2, :] = 0.0
    w[0, :, o.nv - 2] = 0.0
    mults = tc._mults(o, xs[0], 53)
    got = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_NO_TENSORS | (FLAG(capi) if on else 0)) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
            if on:
                ctx.set_joint_accel_cost(target=aref, weight=w)
            ctx.cost_seq_aug(0, mu)
            ctx.cost_seq_aug(1, mu)
            got[on] = {0: ctx.download("COSTS_OLD"), 1: ctx.download("COSTS_NEW")}
    worst = 0.0
    for which, (X, U) in ((0, (xs, us)), (1, (xs2, us2))):
        for b in range(B):
            add = ja_terms(o, X[b], U[b], aref[b], w[b])
            bound = ja_terms(o, X[b], U[b], aref[b], w[b], bound=True)
            on, off = got[True][which][b], got[False][which][b]
            assert on[T] == off[T] and add[T] == 0.0
            for t in range(T):
                if b == 1 and t == 2:
                    assert on[t] == off[t]
                    continue
                assert add[t] > 0
                tol = TOL_ABA * bound[t] + 4 * np.finfo(float).eps * abs(on[t])   # (+ the rounding of off + term and of on - off)
                worst = max(worst, abs((on[t] - off[t]) - add[t]) / tol)
                assert abs((on[t] - off[t]) - add[t]) <= tol, (which, b, t, on[t] - off[t], add[t], tol)
    print("cost values", name, "worst error / tolerance", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_joint_accel_report(gpu, name):
    """Context.joint_accel against o.aba to 1e-12 along X / U and X_NEW / U_NEW, with every weight 0 (nothing uploaded)"""
    capi = gpu
    T, B = 3, 2
    model, spec, o = make_any(name, T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 71)
    xs2, us2 = _trajs(o, model, B, 75)
    with capi.Context(spec, flags=FLAG(capi) | capi.FLAG_NO_TENSORS) as ctx:
        _setup(ctx, xs, us)
        ctx.upload("X_NEW", xs2); ctx.upload("U_NEW", us2)
        for which, (X, U) in ((0, (xs, us)), (1, (xs2, us2))):
            a = ctx.joint_accel(which)
            assert a.shape == (B, T, o.nv)
            ex = np.stack([ja_accels(o, X[b], U[b]) for b in range(B)])
            e = rel_err(a, ex)
            print("joint_accel", name, which, e, "max|a|", np.max(np.abs(ex)))
            assert e < TOL_ABA, (which, e)
        assert np.all(ctx.joint_accel_cost()[1] == 0.0)


FWD_WSCALE = 1e-3     # accelerations of the held trajectories are some 1 .. 100 rad/s^2: the terms are material beside c/2 |u|^2, the sweep stays positive definite


def _forward_case(capi, name, n_alpha, box):
    mu, T, B = 1.0, 4, 2
    model, spec, o = make_any(name, T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 81, held=name != "table7")
    aref, w = random_task(o, xs, us, B, 82, wscale=FWD_WSCALE, spread=0.5)
    w[1, 1, 0] = 0.0
    mults = tc._mults(o, xs[0], 85)
    blo = bhi = None
    flags = FLAG(capi) | capi.FLAG_NO_TENSORS | (capi.FLAG_CONTROL_BOUNDS if box else 0)
    with capi.Context(spec, flags=flags) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.set_joint_accel_cost(target=aref, weight=w)
        ctx.linearize()
        _, _, mu_o, _ = ctx.backward(0.0, mu)
        fbs = [{"origin": ctx.download("FB_ORIGIN")[b], "val": ctx.download("FB_VAL")[b], "jac": ctx.download("FB_JAC")[b]} for b in range(B)]
        if box:
            rng = np.random.default_rng(83)
            val = np.stack([fb["val"] for fb in fbs]).reshape(B, T, o.m)
            width = 0.5 * np.abs(val)
            tight = (np.arange(o.m) % 3 == 0)[None, None, :]
            U0 = us.reshape(B, T, o.m)
            blo = np.where(tight, U0 - width * rng.uniform(0.2, 1, size=U0.shape), -np.inf)
            bhi = np.where(tight, U0 + width * rng.uniform(0.2, 1, size=U0.shape), np.inf)
            ctx.set_control_bounds(lo=blo, hi=bhi)
        rc, step, dcost = ctx.forward(mu_o, n_alpha=n_alpha)
        xn, un = ctx.download("X_NEW"), ctx.download("U_NEW")
        ctx.cost_seq_aug(1, mu_o)
        cnew = ctx.download("COSTS_NEW")
        anew = ctx.joint_accel(1)
    for b in range(B):
        def cost(X, U):
            return o.cost_seq_aug(X, U, mults, mu_o[b]) + ja_terms(o, X, U, aref[b], w[b])
        em = _emulate_forward(o, xs[b], us[b], mults, fbs[b], mu_o[b], n_alpha, cost, None if blo is None else blo[b], None if bhi is None else bhi[b])
        assert em is not None
        step_ref, xn_ref, un_ref, new, margins = em
        share = ja_terms(o, xn_ref, un_ref, aref[b], w[b]).sum() / np.sum(np.abs(cost(xn_ref, un_ref)))
        print("forward", name, n_alpha, box, b, "step", step[b], step_ref, "dcost", dcost[b], new, "margins", margins, "share", share)
        assert share > 1e-6                               # the terms are material in the candidate's cost
        assert min(margins) > 1e-9, margins               # a condition on the inputs: the decisions do not hang on rounding
        assert step[b] == step_ref, (b, step, step_ref)
        assert rel_err(xn[b], xn_ref) < TOL_FWD and rel_err(un[b], un_ref) < TOL_FWD
        assert abs(dcost[b] - new) <= TOL_FWD * max(1.0, abs(new)), (dcost[b], new)
        assert rel_err(cnew[b], cost(xn_ref, un_ref)) < TOL_FWD
        assert rel_err(anew[b], ja_accels(o, xn_ref, un_ref)) < TOL_FWD
        if box:
            Un = un[b].reshape(T, o.m)
            assert np.any(Un == blo[b]) or np.any(Un == bhi[b])
            raw = o.forward_alpha(step_ref, xs[b], us[b], mults, fbs[b], mu_o[b])[2]
            assert not np.array_equal(raw, un_ref)         # the unclamped control would give other terms


@pytest.mark.gpu
@pytest.mark.parametrize("n_alpha", [1, 3, 8])
@pytest.mark.parametrize("name", MODELS)
def test_forward_line_search(gpu, name, n_alpha):
    """chosen step, dcost, X_NEW / U_NEW, COSTS_NEW and the accelerations along the accepted candidate against the sequential
    emulation (Oracle.forward_alpha rollouts costed with numpy, the term formed from each candidate's own controls), 1e-9, per
    instance of a batch of 2.  The test first asserts, on the emulation alone, that every candidate tried decides by more than
    1e-9 of the sum of the cost terms' magnitudes, and only then compares decisions"""
    _forward_case(gpu, name, n_alpha, False)


@pytest.mark.gpu
@pytest.mark.parametrize("n_alpha", [1, 3, 8])
def test_forward_line_search_bounds(gpu, n_alpha):
    """... with DDP_HIP_FLAG_CONTROL_BOUNDS and bounds that bind on every third control, chain6: the emulation clamps, and the
    term is formed from the clamped control"""
    _forward_case(gpu, "chain6", n_alpha, True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain6", "chain6ff"])
def test_backward_stepwise(gpu, name):
    """the backward sweep (unchanged) on derivatives that carry the term: the flag-off device derivatives plus the yardstick's
    five additions equal the flag-on ones (1e-10), Oracle.backward on them takes the device's restarts, mu and reg, and every
    step redone alone by the oracle from the device's V(t+1) lands on the device's k_t, K_t, V_x(t), V_xx(t) to 1e-10"""
    from oracle.binding import Oracle
    capi = gpu
    T, mu = 4, 10.0
    model, spec, o = make(name, T, fd_mode=0)
    xs, us = _trajs(o, model, 1, 71, held=True)
    aref, w = random_task(o, xs, us, 1, 72, wscale=FWD_WSCALE, spread=0.5)
    mults = tc._mults(o, xs[0], 73)
    d = o.alloc_derivs()
    with capi.Context(spec, flags=capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.linearize()
        for k, s in NAMES.items():
            if ctx.seq_size(s):
                d[k][:ctx.seq_size(s)] = ctx.download(s)[0]
    zfun = Jacobians(capi, model, o)
    add = ja_derivs(o, xs[0], us[0], aref[0], w[0], zfun)
    zfun.close()
    back = {v: k for k, v in NAMES.items()}
    for s in add:
        d[back[s]][:add[s].size] += add[s]
    with capi.Context(spec, flags=FLAG(capi) | capi.FLAG_TRACE) as ctx:
        _setup(ctx, xs, us, mults, o.Etot)
        ctx.set_joint_accel_cost(target=aref, weight=w)
        ctx.linearize()
        assert np.max(np.abs(ctx.download("LUX")[0])) > 0
        for s in add:
            assert rel_err(ctx.download(s)[0], d[back[s]][:ctx.seq_size(s)]) <= TOL_LIN, s
            d[back[s]][:ctx.seq_size(s)] = ctx.download(s)[0]           # the sweep is checked on the device's own derivatives
        rc, reg, mu_out, restarts = ctx.backward(0.0, mu)
        ref_b = o.backward(d, xs[0], mults, 0.0, mu)
        print("sweep", name, "device restarts", int(restarts[0]), "oracle", ref_b["restarts"], "mu", mu_out[0], ref_b["mu"], "reg", reg[0], ref_b["reg"])
        assert int(restarts[0]) == ref_b["restarts"] and mu_out[0] == ref_b["mu"] and reg[0] == ref_b["reg"]
        got = {s: ctx.download(s)[0] for s in ("FB_JAC", "FB_VAL", "VX_TRACE", "VXX_TRACE")}
    assert np.max(np.abs(got["VX_TRACE"])) > 0

    def one_step_oracle(t):
        e = int(o.ne[t])
        if not e:
            return Oracle(model, 1, dt=0.01, c=1.0, fd_mode=0)
        return Oracle(model, 1, dt=0.01, c=1.0, fd_mode=0, eq_kind=spec.eq_kind, eq_advance=2, ne=np.array([e], dtype=np.int64),
                      eq_target=np.zeros(e))
    worst = stepwise_backward_check(one_step_oracle, o, d, xs[0], mults, reg[0], mu_out[0], got["VX_TRACE"], got["VXX_TRACE"],
                                    got["FB_VAL"], got["FB_JAC"], range(T))
    print("stepwise worst", worst)
    assert worst < TOL_SWEEP, worst


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["nothing", "zero_halves", "zero_after_live"])
@pytest.mark.parametrize("name", MODELS)
def test_zero_weights_bit_for_bit(gpu, name, mode):
    """flag on with nothing uploaded; zeros uploaded in two half-batch ranges after live weights (the live rule: the kernels stay
    launched and skip every block); one whole-batch upload of zeros after live weights (the kernels are off again): linearise,
    both costs, sweep and forward bit for bit what the flag-off context computes"""
    capi = gpu
    T, B, mu = 4, 2, 10.0
    model, spec, o = make_any(name, T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 31, held=name != "table7")
    mults = tc._mults(o, xs[0], 32)
    aref, w = random_task(o, xs, us, B, 33, wscale=FWD_WSCALE, spread=5.0)
    out = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_TRACE | (FLAG(capi) if on else 0)) as ctx:
            _setup(ctx, xs, us, mults, o.Etot)
            if on and mode != "nothing":
                ctx.set_joint_accel_cost(target=aref, weight=w)
                ctx.linearize()
                assert not np.array_equal(ctx.download("LUX"), out[False]["LUX"])    # the terms were there
                if mode == "zero_halves":
                    ctx.set_joint_accel_cost(weight=0.0, first=0, count=1)
                    ctx.set_joint_accel_cost(weight=0.0, first=1, count=1)
                else:
                    ctx.set_joint_accel_cost(weight=0.0)
                _setup(ctx, xs, us, mults, o.Etot)
            out[on] = fc._run_all(ctx, mu, False)
    fc._same(out[False], out[True])
    assert np.all(np.isfinite(out[True]["LX"])) and np.all(np.isfinite(out[True]["X_NEW"]))


def _other_terms(capi, ctx, o, model, xs, us, B, T):
    """a small task for each of the other add-on terms"""
    frames = fc.pick_frames(model, 3)
    tc.upload_ref(ctx, tc.random_ref(o, model, xs, us, B, 44))
    ftask = fc.random_task(o, xs, frames, B, 45)
    otask = fo.random_orient(o, xs, frames, B, 47)
    vtask = fv.random_task(o, xs, frames, B, 49)
    lim = sl.random_limits(o, xs, B, 46)
    ctask = cm.random_task(o, model, xs, B, 48)
    mtask = mo.random_task(o, model, xs, B, 51)
    pairs = rf.pick_pairs(model)
    opts = ob.pick_points(model)
    scpairs = sc.all_pairs(opts)
    ctx.set_frame_cost(frames=frames, target=ftask[0], weight=ftask[1])
    ctx.set_frame_orient_cost(quat=otask[0], weight=otask[1])
    ctx.set_frame_vel_cost(target=vtask[0], weight=vtask[1])
    ctx.set_state_limits(lo=lim[0], hi=lim[1], weight=lim[2])
    ctx.set_com_cost(target=ctask[0], weight=ctask[1])
    ctx.set_momentum_cost(target=mtask[0], weight=mtask[1])
    rf.set_task(ctx, pairs, *rf._lin_task(o, pairs, xs, B, T))
    ob.set_task(ctx, opts, ob.KINDS, *ob.random_task(o, opts, ob.KINDS, xs, B, 50))
    sc.set_task(ctx, opts, scpairs, *sc.random_task(o, opts, scpairs, xs, B, 52))
    ctx.set_control_grav_cost(*cg.random_task(o, model, B, 53))
    aim = fa.pick_aim_frames(model)
    fa.set_task(ctx, aim, *fa.random_task(o, aim, xs, B, 54))
    br.set_task(ctx, *br.random_task(o, model, xs, B, 55))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain6ff", "tree38"])
def test_combines_with_other_terms(gpu, name):
    """every creation flag on (tracking, control bounds without a bound, the fourteen other add-on terms with a small task each,
    the trace): the new term's additions equal the all-but-this context's difference at 1e-10 * scale, and with this term's
    weights 0 (uploaded range by range: its kernels launched) the others' contributions are unchanged bit for bit"""
    capi = gpu
    T, B, mu = 4, 3, 10.0
    model, spec, o = make_any(name, T, batch=B, fd_mode=0)
    xs, us = _trajs(o, model, B, 141)
    xs = fv._moving(xs, o, 142)
    aref, w = random_task(o, xs, us, B, 143)
    others = (capi.FLAG_TRACE | capi.FLAG_TRACKING_COST | capi.FLAG_CONTROL_BOUNDS | capi.FLAG_FRAME_COST | capi.FLAG_STATE_LIMITS
              | capi.FLAG_FRAME_ORIENT_COST | capi.FLAG_COM_COST | capi.FLAG_FRAME_VEL_COST | capi.FLAG_OBSTACLE_COST
              | capi.FLAG_SELF_COLLISION_COST | capi.FLAG_MOMENTUM_COST | capi.FLAG_RELATIVE_FRAME_COST | capi.FLAG_CONTROL_GRAV_COST
              | capi.FLAG_FRAME_AIM_COST | capi.FLAG_BALANCE_REGION_COST)
    got = {}
    for key in ("without", "with", "zero"):
        with capi.Context(spec, flags=others | (0 if key == "without" else FLAG(capi))) as ctx:
            _setup(ctx, xs, us)
            _other_terms(capi, ctx, o, model, xs, us, B, T)
            if key != "without":
                ctx.set_joint_accel_cost(target=aref, weight=w)
            if key == "zero":
                for b in range(B):
                    ctx.set_joint_accel_cost(weight=0.0, first=b, count=1)
            ctx.linearize()
            got[key] = {s: ctx.download(s) for s in DERIVS if ctx.seq_size(s)}
            ctx.cost_seq_aug(0, mu)
            got[key]["COSTS_OLD"] = ctx.download("COSTS_OLD")
    for s in got["without"]:
        assert np.array_equal(got["zero"][s], got["without"][s]), s
        if s not in ADDS and s != "COSTS_OLD":
            assert np.array_equal(got["with"][s], got["without"][s]), s
    worst = 0.0
    zfun = Jacobians(capi, model, o)
    adds = [ja_derivs(o, xs[b], us[b], aref[b], w[b], zfun) for b in range(B)]
    zfun.close()
    for b in range(B):
        add = adds[b]
        for s in ADDS:
            assert not np.array_equal(got["with"][s][b], got["without"][s][b])
            e = rel_err(got["with"][s][b], got["without"][s][b] + add[s])
            worst = max(worst, e)
            assert e <= TOL_LIN, (s, b, e)
        terms = ja_terms(o, xs[b], us[b], aref[b], w[b])
        assert rel_err(got["with"]["COSTS_OLD"][b], got["without"]["COSTS_OLD"][b] + terms) <= TOL_FWD
    print("combines", name, "worst", worst)


@pytest.mark.gpu
def test_per_instance_ranges(gpu):
    capi = gpu
    T, B = 3, 3
    model, spec, o = make("chain6ff", T, batch=B, fd_mode=0, first_order_fd=0)
    nv = o.nv
    L = capi.lib()
    dp = C.POINTER(C.c_double)

    def code(fn):
        with pytest.raises(capi.DdpHipError) as exc:
            fn()
        return exc.value.code
    with capi.Context(spec) as ctx:                                   # a context without the flag
        assert code(lambda: ctx.set_joint_accel_cost(weight=0.0)) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.joint_accel_cost()) == capi.E_UNSUPPORTED
        assert code(lambda: ctx.joint_accel()) == capi.E_UNSUPPORTED
    pend = capi.BuiltinModel(capi.BUILTIN_PENDULUM)
    with pytest.raises(capi.DdpHipError) as exc:
        capi.Context(capi.ProblemSpec(pend, T, fd_mode=2), flags=FLAG(capi))
    assert exc.value.code == capi.E_UNSUPPORTED
    big = tree_of(44)
    kw = dict(dt=0.01, c=1.0, fd_mode=0, first_order_fd=1, eq_kind=capi.EQ_NONE, ne=np.zeros(T, dtype=np.int64))
    with pytest.raises(capi.DdpHipError) as exc:                      # nv 39 .. 64: the 38 instantiation alone
        capi.Context(capi.ProblemSpec(big, T, **kw), flags=FLAG(capi))
    assert exc.value.code == capi.E_UNSUPPORTED
    with capi.Context(capi.ProblemSpec(big, T, **kw)):                # ... and the model itself is fine without the flag
        pass
    with capi.Context(spec, flags=FLAG(capi)) as ctx:                 # the flag stands alone
        a0, w0 = ctx.joint_accel_cost()                               # create: targets 0, weights 0; the public shape is (T, nv)
        assert a0.shape == (B, T, nv) and w0.shape == (B, T, nv) and np.all(a0 == 0.0) and np.all(w0 == 0.0)
        rng = np.random.default_rng(5)
        ag, wg = rng.normal(size=(B, T, nv)), rng.uniform(0, 1, size=(B, T, nv))
        ctx.set_joint_accel_cost(target=ag, weight=wg)                # a free-flyer root's six rows take weights
        for bad in (-1e-3, np.nan, np.inf):
            wb = np.ones((T, nv)); wb[1, 8] = bad
            assert code(lambda: ctx.set_joint_accel_cost(weight=wb)) == capi.E_ARG, bad
            assert code(lambda: ctx.set_joint_accel_cost(target=np.zeros((T, nv)), weight=wb)) == capi.E_ARG, bad
        for bad in (np.nan, -np.inf):
            ab = np.ones((T, nv)); ab[2, 3] = bad
            assert code(lambda: ctx.set_joint_accel_cost(target=ab)) == capi.E_ARG, bad
        assert code(lambda: ctx.set_joint_accel_cost(weight=0.0, first=B, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_joint_accel_cost(weight=0.0, first=-1, count=1)) == capi.E_ARG
        assert code(lambda: ctx.set_joint_accel_cost(weight=0.0, first=1, count=B)) == capi.E_ARG
        assert code(lambda: ctx.joint_accel_cost(first=1, count=B)) == capi.E_ARG
        z = np.zeros((B + 1) * (T + 1) * nv)
        assert L.ddp_hip_joint_accel_cost_upload(ctx._h, z.ctypes.data_as(dp), z.ctypes.data_as(dp), 0, B + 1) == capi.E_ARG
        zt = np.zeros((B, T + 1, nv)); zt[B - 1, T, nv - 1] = 1e-3      # a non-zero weight in row T, through the raw C call
        assert L.ddp_hip_joint_accel_cost_upload(ctx._h, None, zt.ctypes.data_as(dp), 0, B) == capi.E_ARG
        zt[B - 1, T, nv - 1] = 0.0; zt[B - 1, T - 1, nv - 1] = 1e-3     # ... row T-1 is a stage row
        assert L.ddp_hip_joint_accel_cost_upload(ctx._h, None, zt.ctypes.data_as(dp), 0, B) == 0
        ctx.set_joint_accel_cost(weight=wg)
        a1, w1 = ctx.joint_accel_cost()
        assert np.array_equal(a1, ag) and np.array_equal(w1, wg)      # a refused upload leaves both sides as they were
        raw_a, raw_w = np.zeros((B, T + 1, nv)), np.zeros((B, T + 1, nv))
        assert L.ddp_hip_joint_accel_cost_download(ctx._h, raw_a.ctypes.data_as(dp), raw_w.ctypes.data_as(dp), 0, B) == 0
        assert np.array_equal(raw_a[:, :T], ag) and np.all(raw_a[:, T] == 0.0) and np.all(raw_w[:, T] == 0.0)
        ctx.set_joint_accel_cost(target=ag[1] + 1.0, first=1, count=1)  # one side, one instance; the weights stay
        a1, w1 = ctx.joint_accel_cost()
        assert np.array_equal(a1[0], ag[0]) and np.array_equal(a1[1], ag[1] + 1.0) and np.array_equal(a1[2], ag[2]) and np.array_equal(w1, wg)
        ctx.set_joint_accel_cost(weight=wg[2] * 2.0, first=2, count=1)  # ... and the other side alone; the targets stay
        a2, w2 = ctx.joint_accel_cost(first=1, count=2)                 # the round trip of a range of instances
        assert np.array_equal(a2, a1[1:]) and np.array_equal(w2[0], wg[1]) and np.array_equal(w2[1], wg[2] * 2.0)
        row = np.arange(1.0, nv + 1)
        ctx.set_joint_accel_cost(target=0.25, weight=row, first=1, count=2)   # broadcast: scalar and (nv,)
        assert np.array_equal(ctx.joint_accel_cost()[1][1:], np.broadcast_to(row, (2, T, nv)))
        assert np.all(ctx.joint_accel_cost()[0][1:] == 0.25) and np.array_equal(ctx.joint_accel_cost()[1][0], wg[0])


def tree_of(nj):
    """a fixed-base tree of nj revolute joints given as arrays (three chains from the first joint), for the create-time refusal above 38"""
    from ddp_pinocchio_amd import capi
    rng = np.random.default_rng(79)
    parents = [-1] + [0 if i <= 3 else i - 3 for i in range(1, nj)]
    axis = rng.normal(size=(nj, 3)); axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    Rp = np.tile(np.eye(3), (nj, 1, 1))
    pp = rng.uniform(0.05, 0.3, size=(nj, 3))
    mass = rng.uniform(0.5, 5.0, size=nj)
    Ic = np.stack([np.diag(mass[k] * rng.uniform(0.01, 0.05, size=3)) for k in range(nj)])
    return capi.TableModel(parents, [capi.JOINT_REVOLUTE] * nj, axis, Rp, pp, mass, rng.uniform(-0.05, 0.05, size=(nj, 3)), Ic)


@pytest.mark.gpu
def test_whole_solve_smooths(gpu):
    """chain6 without constraints reaching for a tip point 0.15 away (test_frame_cost's reach task: running weight 10, terminal
    1000), T = 20, with and without a uniform acceleration weight about a_ref = 0: ddp_hip_solve converges on both (optimality
    below 1e-6 within 60 iterations), max_t |joint_accel| of the weighted run is below the unweighted run's, and the weighted
    problem's cost never increases over the accepted iterations of the stepwise loop"""
    from ddp_pinocchio_amd import solver
    from oracle.binding import Oracle
    capi = gpu
    T, mu, wa = 20, 1.0, 1e-2
    model = capi.BuiltinModel(capi.BUILTIN_CHAIN6)
    kw = dict(dt=0.01, c=1.0, fd_mode=0, first_order_fd=0, eq_kind=capi.EQ_NONE, ne=np.zeros(T, dtype=np.int64))
    spec, o = capi.ProblemSpec(model, T, batch=1, **kw), Oracle(model, T, **kw)
    frames = fc.pick_frames(model, 1)
    xs, us = _trajs(o, model, 1, 111, held=True)
    q0 = xs[0][:o.nq]
    rng = np.random.default_rng(112)
    goal = o.frame_position(frames[0][0], frames[0][1], q0) + 0.15 * rng.normal(size=3) / np.sqrt(3)
    tgt = np.tile(goal, (T + 1, 1, 1))
    wf = np.full((T + 1, 1, 3), 10.0)
    wf[T] = 1000.0
    res = {}
    for on in (False, True):
        with capi.Context(spec, flags=capi.FLAG_FRAME_COST | capi.FLAG_NO_TENSORS | FLAG(capi)) as ctx:
            _setup(ctx, xs, us)
            ctx.set_frame_cost(frames=frames, target=tgt, weight=wf)
            if on:
                ctx.set_joint_accel_cost(weight=wa)
            log = solver.solve(ctx, 60, 1e-6, mu, 0.0, 1e-1, 10.0)
            amax = np.max(np.abs(ctx.joint_accel(0)))
            res[on] = (bool(log["done"][0]), int(log["iterations"][0]), amax, float(log["opt_obj"][0]))
    print("whole solve: (done, iterations, max|a|, opt_obj) unweighted", res[False], "weighted", res[True])
    assert res[False][0] and res[True][0]
    assert res[True][2] < res[False][2]
    with capi.Context(spec, flags=capi.FLAG_FRAME_COST | capi.FLAG_NO_TENSORS | FLAG(capi)) as ctx:
        _setup(ctx, xs, us)
        ctx.set_frame_cost(frames=frames, target=tgt, weight=wf)
        ctx.set_joint_accel_cost(weight=wa)
        costs = []
        for _ in range(8):
            ctx.linearize()
            _, _, mu_o, _ = ctx.backward(0.0, mu)
            ctx.forward(mu_o, n_alpha=8)
            costs.append(ctx.download("COSTS_OLD")[0].sum())
            ctx.swap_traj()
    print("weighted costs", costs)
    for a, b in zip(costs, costs[1:]):
        assert b <= a * (1 + 1e-12), costs
    assert costs[-1] < costs[0]
